#!/usr/bin/env python3
"""tools/compare_probe.py [--sites 1e4,1e5] [--runs 5] [--host-runs 1] [--host-max 1e4] [--json profiles/compare_probe.json]
                         [--kernel-stats profiles/compare_kernel_stats.csv] [--keep DIR] [--device-only] [--host-only] [--seed 7]
                         [--fisher] [--fdr]

Two --vo BED files to the rows of compare_genomes, host statement against device, file to file on the same box:
  host    compare_genomes.compare_by_position          (four SciPy calls a site in a Python loop)
  device  compare_genomes.compare_by_position_device   (csrc/compare/mc_bedcompare.hip)
medians of --runs after a warm-up, with mc_bed_compare_last_stats of the last device run.  Every device file is compared with the
host's, byte for byte, wherever the host ran (cases of up to --host-max sites: the host takes milliseconds a site).  A pair the device
declines is recorded with its reason and not timed.

The files: N shared sites on one contig, depths 15 .. 60 in each file, probabilities in hundredths, every fourth site of bed2
shifted up by 0.3; bed2 in reverse order and with one line in ten of its own.  --host-only needs no GPU.
--fisher / --fdr: the same legs with compare_genomes' flags of those names (profiles/compare_fdr_probe.json); the files' fracs are
then counts over their reads, str(np.mean(p >= 0.5)) as make_bed writes them, in place of the four-decimal ones.
--kernel-stats: the kernels' times from a `rocprofv3 --kernel-trace --stats` run of this tool's own (--device-only, the smallest
case)."""
import glob
import json
import os
import shutil
import statistics
import subprocess
import sys
import tempfile
import time

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))


def arg(name, default):
    a = sys.argv[1:]
    return a[a.index(name) + 1] if name in a else default


def flags():
    return {k: True for k in ('fisher', 'fdr') if '--' + k in sys.argv[1:]}


def write_pair(p1, p2, n, seed, counts=False):
    """-> (bytes of bed1, bytes of bed2, probabilities in both)."""
    import numpy as np
    rng = np.random.default_rng(seed)
    l1, l2, total = [], [], 0
    for i in range(n):
        n1, n2 = (int(v) for v in rng.integers(15, 61, 2))
        x, y = np.round(rng.random(n1), 2), np.round(rng.random(n2), 2)
        if i % 4 == 0:
            y = np.round(np.clip(y + 0.3, 0.0, 1.0), 2)
        total += n1 + n2
        strand = '+-'[i & 1]
        for lines, v in ((l1, x), (l2, y)):
            frac = str((v >= 0.5).mean()) if counts else repr(round(float((v >= 0.5).mean()), 4))
            lines.append('contig_1\t%d\t%d\tGATC\t%s\t%s\t%d\t%s\n' % (100 + 5 * i, 101 + 5 * i, frac, strand,
                                                                     len(v), ','.join(repr(float(p)) for p in v)))
        if i % 10 == 0:
            l2.append('contig_2\t%d\t%d\tGATC\t0.5\t%s\t2\t0.25,0.75\n' % (100 + 5 * i, 101 + 5 * i, strand))
    open(p1, 'w').write(''.join(l1))
    open(p2, 'w').write(''.join(l2[::-1]))
    return os.path.getsize(p1), os.path.getsize(p2), total


def kernel_stats(out_csv, sites, seed):
    """The kernels' times of the device path alone, from a rocprofv3 run of this tool in a process of its own."""
    d = tempfile.mkdtemp(prefix='mc_compare_stats_')
    try:
        cmd = ['rocprofv3', '--kernel-trace', '--stats', '--output-format', 'csv', '-d', d, '--', sys.executable, os.path.abspath(__file__),
               '--device-only', '--sites', str(sites), '--runs', '3', '--seed', str(seed)] + ['--' + k for k in flags()]
        subprocess.run(cmd, check=True, timeout=900, stdout=subprocess.DEVNULL)
        found = glob.glob(os.path.join(d, '**', '*kernel_stats.csv'), recursive=True)
        if not found:
            raise RuntimeError('rocprofv3 left no kernel_stats.csv under %s' % d)
        shutil.copy(found[0], out_csv)
    finally:
        shutil.rmtree(d, ignore_errors=True)


def main():
    from mcaller_amd import _lib, compare_genomes
    sizes = [int(float(x)) for x in arg('--sites', '1e4,1e5').split(',')]
    runs, host_runs, seed = int(arg('--runs', '5')), int(arg('--host-runs', '1')), int(arg('--seed', '7'))
    host_max = int(float(arg('--host-max', '1e4')))
    device_only, host_only = '--device-only' in sys.argv, '--host-only' in sys.argv
    d = arg('--keep', None) or tempfile.mkdtemp(prefix='mc_compare_probe_')
    os.makedirs(d, exist_ok=True)
    cores = int(_lib.lib().mc_host_cores())
    results = []
    for n in sizes:
        p1, p2 = os.path.join(d, 'a%d.bed' % n), os.path.join(d, 'b%d.bed' % n)
        out_d, out_h = os.path.join(d, 'device%d.tsv' % n), os.path.join(d, 'host%d.tsv' % n)
        b1, b2, n_values = write_pair(p1, p2, n, seed, counts=bool(flags()))
        r = dict(sites=n, bed1_bytes=b1, bed2_bytes=b2, probabilities=n_values, **flags())
        if not host_only:
            from mcaller_amd.device import get_device

            def device():
                compare_genomes.compare_by_position_device(p1, p2, out=out_d, **flags())
                return compare_genomes.last_compare

            who = device()                                      # warm-up: pinned blocks, the first launches, the files in the page cache
            if who['by'] != 'device':                           # (a declined pair is no measurement: the reason is the result)
                r.update(declined=who['reason'], stats=get_device().bed_compare_last_stats())
                results.append(r)
                print(json.dumps(r), flush=True)
                continue
            t_dev, ms_all, st = [], [], None
            for _ in range(runs):
                t = time.perf_counter()
                device()
                t_dev.append(time.perf_counter() - t)
                st = get_device().bed_compare_last_stats()
                ms_all.append({k: v for k, v in st.items() if k.startswith('ms_')})
            r.update(device_s=statistics.median(t_dev), device_all_s=t_dev, device_all_ms=ms_all, device_runs=runs, stats=st,
                     kernel_ms=st['ms_kernels'])
        if not device_only and n <= host_max:
            t_host = []
            for _ in range(host_runs):
                t = time.perf_counter()
                compare_genomes.compare_by_position(p1, p2, out=out_h, **flags())
                t_host.append(time.perf_counter() - t)
            r.update(host_s=statistics.median(t_host), host_all_s=t_host, host_runs=host_runs, host_cores=cores,
                     host_ms_per_site=1e3 * statistics.median(t_host) / n)
            if not host_only:
                assert open(out_h, 'rb').read() == open(out_d, 'rb').read(), 'the device\'s rows differ from the host statement\'s'
                r.update(ratio=r['host_s'] / r['device_s'], files_equal=True)
        results.append(r)
        print(json.dumps({k: v for k, v in r.items() if not k.endswith('_all_s') and k != 'device_all_ms'}), flush=True)
        for p in (p1, p2, out_d, out_h):
            if os.path.exists(p) and not arg('--keep', None):
                os.remove(p)
    out = arg('--json', None)
    if out:
        with open(out, 'w') as fh:
            json.dump(dict(tool='tools/compare_probe.py', seed=seed, results=results), fh, indent=1)
            fh.write('\n')
    stats_csv = arg('--kernel-stats', None)
    if stats_csv and not device_only and not host_only:
        from mcaller_amd.device import get_device
        get_device().bed_compare_release()
        kernel_stats(stats_csv, min(sizes), seed)
    if not arg('--keep', None):
        shutil.rmtree(d, ignore_errors=True)


if __name__ == '__main__':
    main()
