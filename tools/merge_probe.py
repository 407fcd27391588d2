#!/usr/bin/env python3
"""tools/merge_probe.py [--rows 1e6,1e7] [--runs 3] [--host-runs 1] [--parts 4] [--seed 7] [--json profiles/merge_probe.json]
                        [--kernel-stats profiles/merge_kernel_stats.csv] [--keep DIR] [--device-only]

The merge behind `-t N`, host code against the device (mCaller.merge_like_sort_uniq / merge_like_sort_uniq_device), file to file
on the same box, in the same call, alternating: device, host, device, host ...  The rows are `-m A`-shaped and made from a seed:
UUID read names (a third begin with a letter: key 0), 100 rows a read in file order, `repr()` features; --parts part files, each a
run of whole reads, one row in 10^4 repeated in another part.  Every device result is compared with the host's bytes.
--json: seconds, ratio, the read / copies / kernels / write split and the rounds of the last device run (mc_rows_merge_last_stats).
--kernel-stats: the kernels' times from a `rocprofv3 --kernel-trace --stats` run of this tool's own (--device-only, the smallest
size), a fresh process."""
import glob
import json
import os
import shutil
import statistics
import subprocess
import sys
import tempfile
import time

import numpy as np

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))

PEAK_BYTES_PER_S = 8.0e12          # MI355X HBM3E
ROWS_PER_READ = 100


def arg(name, default):
    a = sys.argv[1:]
    return a[a.index(name) + 1] if name in a else default


def write_parts(d, n_rows, n_parts, seed):
    """-> paths of the master copies of the part files (hard-linked under the names a run consumes), rows written."""
    rng = np.random.default_rng(seed)
    n_reads = max(1, n_rows // ROWS_PER_READ)
    feats = [repr(float(v)).encode() for v in np.round(rng.normal(0.0, 2.0, 8192), 2)]
    probs = [repr(float(v)).encode() for v in rng.random(4096)]
    contexts = [bytes(b'ACGT'[i] for i in rng.integers(0, 4, 5)) + b'M' + bytes(b'ACGT'[i] for i in rng.integers(0, 4, 5)) for _ in range(1024)]
    per_part = (n_reads + n_parts - 1) // n_parts
    paths, written, carry = [], 0, []
    for p in range(n_parts):
        path = os.path.join(d, 'master.tmp%d' % p)
        paths.append(path)
        with open(path, 'wb') as fh:
            fh.writelines(carry)                             # rows of the part before, once more: what uniq is for
            written += len(carry)
            carry = []
            for r in range(p * per_part, min(n_reads, (p + 1) * per_part)):
                h = rng.bytes(16).hex()
                name = ('%s-%s-%s-%s-%s' % (h[:8], h[8:12], h[12:16], h[16:20], h[20:])).encode()
                strand = b'+' if r & 1 else b'-'
                pos = np.cumsum(rng.integers(1, 9, ROWS_PER_READ)) + int(rng.integers(0, 4000000))
                fi = rng.integers(0, len(feats), (ROWS_PER_READ, 6))
                ci = rng.integers(0, len(contexts), ROWS_PER_READ)
                pi = rng.integers(0, len(probs), ROWS_PER_READ)
                rows = [b'ecoli_syn\t%s\t%d\t%s\t%s\t%s\t%s\t%s\n' % (name, pos[i], contexts[ci[i]], b','.join([feats[k] for k in fi[i]]), strand,
                                                                   b'm6A' if pi[i] & 1 else b'A', probs[pi[i]]) for i in range(ROWS_PER_READ)]
                fh.writelines(rows)
                written += len(rows)
                if r % 100 == 0:
                    carry.append(rows[r % ROWS_PER_READ])
    return paths, written


def link_parts(masters, d):
    paths = []
    for i, m in enumerate(masters):
        paths.append(os.path.join(d, 'rows.diffs.6.tmp%d' % i))
        if os.path.exists(paths[-1]):
            os.remove(paths[-1])
        os.link(m, paths[-1])
    return paths


def kernel_stats(out_csv, rows, parts, seed):
    """The kernels' times of the device path alone, from a rocprofv3 run of this tool in a process of its own."""
    d = tempfile.mkdtemp(prefix='mc_merge_stats_')
    try:
        cmd = ['rocprofv3', '--kernel-trace', '--stats', '--output-format', 'csv', '-d', d, '--', sys.executable, os.path.abspath(__file__),
               '--device-only', '--rows', str(rows), '--runs', '3', '--parts', str(parts), '--seed', str(seed)]
        subprocess.run(cmd, check=True, timeout=900, stdout=subprocess.DEVNULL)
        found = glob.glob(os.path.join(d, '**', '*kernel_stats.csv'), recursive=True)
        if not found:
            raise RuntimeError('rocprofv3 left no kernel_stats.csv under %s' % d)
        shutil.copy(found[0], out_csv)
    finally:
        shutil.rmtree(d, ignore_errors=True)


def main():
    from mcaller_amd import mCaller
    from mcaller_amd.device import get_device
    sizes = [int(float(x)) for x in arg('--rows', '1e6,1e7').split(',')]
    runs, host_runs, n_parts, seed = int(arg('--runs', '3')), int(arg('--host-runs', '1')), int(arg('--parts', '4')), int(arg('--seed', '7'))
    device_only = '--device-only' in sys.argv
    os.environ['MCALLER_MERGE_DEVICE'] = '1'
    d = arg('--keep', None) or tempfile.mkdtemp(prefix='mc_merge_probe_')
    os.makedirs(d, exist_ok=True)
    results = []
    for n in sizes:
        masters, rows = write_parts(d, n, n_parts, seed)
        n_bytes = sum(os.path.getsize(m) for m in masters)
        outs = [os.path.join(d, 'host.merged'), os.path.join(d, 'device.merged')]
        mCaller.merge_like_sort_uniq_device(link_parts(masters, d), outs[1])          # warm-up: pinned blocks, the first launches
        assert mCaller.last_merge['by'] == 'device', mCaller.last_merge
        t_dev, t_host, ms_all, st = [], [], [], None
        for i in range(max(runs, 0 if device_only else host_runs)):
            if i < runs:
                paths = link_parts(masters, d)
                t = time.perf_counter()
                mCaller.merge_like_sort_uniq_device(paths, outs[1])
                t_dev.append(time.perf_counter() - t)
                assert mCaller.last_merge['by'] == 'device', mCaller.last_merge
                st = get_device().merge_rows_last_stats()
                ms_all.append({k: v for k, v in st.items() if k.startswith('ms_')})       # the call's own split of the run
            if i < host_runs and not device_only:
                paths = link_parts(masters, d)
                t = time.perf_counter()
                mCaller.merge_like_sort_uniq(paths, outs[0])
                t_host.append(time.perf_counter() - t)
        r = dict(rows=rows, parts=n_parts, file_bytes=n_bytes, device_s=statistics.median(t_dev), device_all_s=t_dev, device_all_ms=ms_all, device_runs=runs, stats=st,
                 rounds=st['n_rounds'], passes=st['n_passes'], kernel_ms=st['ms_kernels'], kernel_bytes=st['kernel_bytes'],
                 kernel_fraction_of_peak=st['kernel_bytes'] / (st['ms_kernels'] * 1e-3) / PEAK_BYTES_PER_S if st['ms_kernels'] > 0 else None)
        if t_host:
            with open(outs[0], 'rb') as a, open(outs[1], 'rb') as b:
                while True:
                    x, y = a.read(1 << 24), b.read(1 << 24)
                    assert x == y, 'the device merge differs from the host function\'s'
                    if not x:
                        break
            r.update(host_s=statistics.median(t_host), host_all_s=t_host, host_runs=host_runs, ratio=statistics.median(t_host) / r['device_s'],
                     bytes_equal=True)
        results.append(r)
        print('%9d rows %6.1f MB  host %s s  device %7.3f s  %s read %.1f ms, H2D %.1f ms, kernels %.1f ms (%.4f of peak), D2H %.1f ms, '
              'write %.1f ms; %d rounds, %d passes, %d lines out, %d tied after the key'
              % (rows, n_bytes / 1e6, '%8.2f' % r['host_s'] if t_host else 'not run', r['device_s'], 'x%-7.1f' % r['ratio'] if t_host else '', st['ms_read'],
                 st['ms_h2d'], st['ms_kernels'], r['kernel_fraction_of_peak'] or 0.0, st['ms_d2h'], st['ms_write'], st['n_rounds'], st['n_passes'],
                 st['n_lines_out'], st['n_tied_after_key']), flush=True)
        for m in masters + outs:
            if os.path.exists(m):
                os.remove(m)
    out = arg('--json', None)
    if out:
        with open(out, 'w') as fh:
            json.dump(dict(tool='tools/merge_probe.py', seed=seed, rows_per_read=ROWS_PER_READ, peak_bytes_per_s=PEAK_BYTES_PER_S, results=results), fh, indent=1)
            fh.write('\n')
    stats_csv = arg('--kernel-stats', None)
    if stats_csv and not device_only:
        get_device().merge_rows_release()
        kernel_stats(stats_csv, min(sizes), n_parts, seed)
    if not arg('--keep', None):
        shutil.rmtree(d, ignore_errors=True)


if __name__ == '__main__':
    main()
