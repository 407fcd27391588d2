#!/usr/bin/env python3
"""tools/bedpos_probe.py [--cases 1e5:2e4,1e6:2e4] [--runs 5] [--host-runs 1] [--json profiles/bedpos_probe.json]
                         [--kernel-stats profiles/bedpos_kernel_stats.csv] [--keep DIR] [--device-only] [--seed 7]

make_bed -p, host code against the device (make_bed.summarise_diffs(positions=...) / summarise_diffs_device(positions=...)), file to
file on the same box: the device's median of --runs after a warm-up, the host function --host-runs times (its time goes with the
number of SITES: six t-tests by SciPy each), with mc_bed_last_stats of the last device run.  Every device result is compared with
the host's bytes.

A case is rows:sites.  The file is synthetic: rows of seven repr() values drawn around a per-site centre, sites in random order,
every second site listed in the positions file (so the position set has work to do), depth = rows / sites on average.
--kernel-stats: the kernels' times from a `rocprofv3 --kernel-trace --stats` run of this tool's own (--device-only, the first case)."""
import glob
import json
import os
import random
import shutil
import statistics
import subprocess
import sys
import tempfile
import time
import warnings

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))


def arg(name, default):
    a = sys.argv[1:]
    return a[a.index(name) + 1] if name in a else default


def write_case(d, n_rows, n_sites, seed):
    """-> (diffs path, positions path, rows at listed sites)."""
    rng = random.Random(seed)
    centres = [[rng.choice([0.0, 0.3, -1.0, 2.0]) for _ in range(7)] for _ in range(256)]
    path, pos = os.path.join(d, 'probe.eventalign.diffs.6'), os.path.join(d, 'probe.positions')
    wanted = 0
    with open(path, 'w') as fh:
        for i in range(n_rows):
            s = rng.randrange(n_sites)
            c = centres[s & 255]
            fh.write('ecoli_syn\tread%d\t%d\tTTGCAMTTCAG\t%s\t%s\t%s\t%s\n' % (i // 40, 1000 + 3 * s, ','.join(repr(rng.gauss(m, 1.5)) for m in c),
                                                                       '+-'[s & 1], 'm6A' if rng.random() < 0.4 else 'A', repr(round(rng.random(), 2))))
            wanted += (s % 4) < 2
    with open(pos, 'w') as fh:
        for s in range(n_sites):
            if (s % 4) < 2:
                fh.write('ecoli_syn\t%d\t%d\t%s\n' % (1000 + 3 * s, 1001 + 3 * s, '+-'[s & 1]))
    return path, pos, wanted


def kernel_stats(out_csv, case, seed):
    """The kernels' times of the device path alone, from a rocprofv3 run of this tool in a process of its own."""
    d = tempfile.mkdtemp(prefix='mc_bedpos_stats_')
    try:
        cmd = ['rocprofv3', '--kernel-trace', '--stats', '--output-format', 'csv', '-d', d, '--', sys.executable, os.path.abspath(__file__),
               '--device-only', '--cases', case, '--runs', '3', '--seed', str(seed)]
        subprocess.run(cmd, check=True, timeout=900, stdout=subprocess.DEVNULL)
        found = glob.glob(os.path.join(d, '**', '*kernel_stats.csv'), recursive=True)
        if not found:
            raise RuntimeError('rocprofv3 left no kernel_stats.csv under %s' % d)
        shutil.copy(found[0], out_csv)
    finally:
        shutil.rmtree(d, ignore_errors=True)


def main():
    from mcaller_amd import make_bed
    from mcaller_amd.device import get_device
    cases = arg('--cases', '1e5:2e4,1e6:2e4')
    runs, host_runs, seed = int(arg('--runs', '5')), int(arg('--host-runs', '1')), int(arg('--seed', '7'))
    device_only = '--device-only' in sys.argv
    d = arg('--keep', None) or tempfile.mkdtemp(prefix='mc_bedpos_probe_')
    os.makedirs(d, exist_ok=True)
    results = []
    for case in cases.split(','):
        n_rows, n_sites = (int(float(x)) for x in case.split(':'))
        path, pos, wanted = write_case(d, n_rows, n_sites, seed)
        outs = [os.path.join(d, 'host.bed'), os.path.join(d, 'device.bed')]

        def device():
            make_bed.summarise_diffs_device(path, outs[1], 15, 0.5, positions=pos, with_probs=False, quiet=True)
            assert make_bed.last_summary['by'] == 'device', make_bed.last_summary
        device()                                           # warm-up: pinned blocks, the first launches
        t_dev, t_host, ms_all = [], [], []
        for _ in range(runs):
            t = time.perf_counter()
            device()
            t_dev.append(time.perf_counter() - t)
            ms_all.append({k: v for k, v in get_device().bed_last_stats().items() if k.startswith('ms_')})       # the call's own split of the run
        st = get_device().bed_last_stats()
        r = dict(rows=n_rows, sites=n_sites, rows_at_listed_sites=wanted, file_bytes=os.path.getsize(path), positions_bytes=os.path.getsize(pos),
                 device_s=statistics.median(t_dev), device_all_s=t_dev, device_all_ms=ms_all, device_runs=runs, stats=st, kernel_ms=st['ms_kernels'])
        if not device_only:
            for _ in range(host_runs):
                t = time.perf_counter()
                with warnings.catch_warnings():
                    warnings.simplefilter('ignore')
                    make_bed.summarise_diffs(path, outs[0], 15, 0.5, positions=pos)
                t_host.append(time.perf_counter() - t)
            assert open(outs[0], 'rb').read() == open(outs[1], 'rb').read(), 'the device summary differs from the host function\'s'
            r.update(host_s=statistics.median(t_host), host_all_s=t_host, host_runs=host_runs, ratio=statistics.median(t_host) / r['device_s'],
                     bytes_equal=True)
        results.append(r)
        print('%9d rows %7d sites %6.1f MB  host %s s  device %7.4f s  %s read %.1f ms, H2D %.1f ms, kernels %.1f ms, D2H %.1f ms; %d entries'
              % (n_rows, n_sites, r['file_bytes'] / 1e6, '%8.2f' % r['host_s'] if t_host else 'not run', r['device_s'],
                 'x%-7.1f' % r['ratio'] if t_host else '', st['ms_read'], st['ms_h2d'], st['ms_kernels'], st['ms_d2h'], st['n_entries']), flush=True)
    out = arg('--json', None)
    if out:
        with open(out, 'w') as fh:
            json.dump(dict(tool='tools/bedpos_probe.py', seed=seed, results=results), fh, indent=1)
            fh.write('\n')
    stats_csv = arg('--kernel-stats', None)
    if stats_csv and not device_only:
        get_device().bed_release()
        kernel_stats(stats_csv, cases.split(',')[0], seed)
    if not arg('--keep', None):
        shutil.rmtree(d, ignore_errors=True)


if __name__ == '__main__':
    main()
