#!/usr/bin/env python3
"""tools/phase_probe.py [--sites 2e3,2e4] [--runs 3] [--host-runs 3] [--host-max 2e4] [--json profiles/phase_probe.json]
                       [--kernel-stats profiles/phase_kernel_stats.csv] [--keep DIR] [--device-only] [--host-only] [--seed 7]

One `-m GATC`-like .diffs file to the three files of phase_reads --fdr --reads --linked_bed, host statement against device, file to
file on the same box:
  host    phase_reads.phase_reads          (dicts of reads, a NumPy window walk per read, Fisher's test in exact rationals per pair)
  device  phase_reads.phase_reads_device   (csrc/compare/mc_sitegroup.inc, mc_readphase.inc)
medians of --runs after a warm-up, with mc_reads_phase_last_stats of the last device run.  Every device file is compared with the
host's, byte for byte, wherever the host ran (cases of up to --host-max sites).  A file the device declines is recorded with its
reason and not timed.

The file: N sites on one contig and strand, 50 .. 450 bases apart; reads over 10 .. 60 consecutive sites, as many as give the sites a
depth of 15 .. 60; six slot deviations and a read quality a row, the rows read by read.  Every read belongs to one of two planted
populations: at every fourth site population 1 is methylated and population 0 is not (5 % noise), everywhere else nine calls in ten
are methylated.  --host-only needs no GPU.
--kernel-stats: the kernels' times from a `rocprofv3 --kernel-trace --stats` run of this tool's own (--device-only, the smallest
case; kernel trace alone, no counters): each new kernel's share."""
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


def write_file(path, n, seed):
    """-> (bytes of the file, its rows, its reads)."""
    import numpy as np
    rng = np.random.default_rng(seed)
    pos = 1000 + np.cumsum(rng.integers(50, 451, n))
    n_reads = max(1, int(n * 37.5 / 35.0))
    rows = 0
    with open(path, 'w') as fh:
        for r in range(n_reads):
            k = int(rng.integers(10, 61))
            first = int(rng.integers(0, max(1, n - k + 1)))
            sites = np.arange(first, min(n, first + k))
            planted = (sites % 4 == 0)
            meth = np.where(planted, (r & 1) != (rng.random(len(sites)) < 0.05), rng.random(len(sites)) < 0.9)
            vals = np.round(rng.normal(0.0, 1.0, (len(sites), 7)), 2)
            for i, s in enumerate(sites):
                fh.write('contig_1\tread_%d\t%d\tGGATGMTCTGA\t%s\t+\t%s\t%s\n' % (r, pos[s], ','.join(repr(float(v)) for v in vals[i]),
                                                                               'm6A' if meth[i] else 'A', '0.9' if meth[i] else '0.1'))
            rows += len(sites)
    return os.path.getsize(path), rows, n_reads


def kernel_stats(out_csv, sites, seed):
    """The kernels' times of the device path alone, from a rocprofv3 run of this tool in a process of its own."""
    d = tempfile.mkdtemp(prefix='mc_phase_stats_')
    try:
        cmd = ['rocprofv3', '--kernel-trace', '--stats', '--output-format', 'csv', '-d', d, '--', sys.executable, os.path.abspath(__file__),
               '--device-only', '--sites', str(sites), '--runs', '3', '--seed', str(seed)]
        subprocess.run(cmd, check=True, timeout=600, stdout=subprocess.DEVNULL)
        found = glob.glob(os.path.join(d, '**', '*kernel_stats.csv'), recursive=True)
        if not found:
            raise RuntimeError('rocprofv3 left no kernel_stats.csv under %s' % d)
        shutil.copy(found[0], out_csv)
    finally:
        shutil.rmtree(d, ignore_errors=True)


def main():
    from mcaller_amd import _lib, phase_reads
    sizes = [int(float(x)) for x in arg('--sites', '2e3,2e4').split(',')]
    runs, host_runs, seed = int(arg('--runs', '3')), int(arg('--host-runs', '3')), int(arg('--seed', '7'))
    host_max = int(float(arg('--host-max', '2e4')))
    device_only, host_only = '--device-only' in sys.argv, '--host-only' in sys.argv
    d = arg('--keep', None) or tempfile.mkdtemp(prefix='mc_phase_probe_')
    os.makedirs(d, exist_ok=True)
    cores = int(_lib.lib().mc_host_cores())
    kw = dict(depth=15, max_dist=1000, min_reads=10, min_margin=2, fdr=True, threshold=2.0)
    results = []
    for n in sizes:
        p = os.path.join(d, 'reads%d.diffs.6' % n)
        out_d, out_h = os.path.join(d, 'device%d.tsv' % n), os.path.join(d, 'host%d.tsv' % n)
        n_bytes, n_rows, n_reads = write_file(p, n, seed)
        r = dict(sites=n, reads=n_reads, file_bytes=n_bytes, rows=n_rows, **kw)

        def run(fn, out):
            fn(p, out=out, reads=out + '.reads', linked_bed=out + '.bed', **kw)
            return phase_reads.last_phase

        if not host_only:
            from mcaller_amd.device import get_device
            who = run(phase_reads.phase_reads_device, out_d)    # warm-up: pinned blocks, the first launches, the file in the page cache
            if who['by'] != 'device':                           # (a declined file is no measurement: the reason is the result)
                r.update(declined=who['reason'], stats=get_device().reads_phase_last_stats())
                results.append(r)
                print(json.dumps(r), flush=True)
                continue
            t_dev, ms_all, st = [], [], None
            for _ in range(runs):
                t = time.perf_counter()
                who = run(phase_reads.phase_reads_device, out_d)
                t_dev.append(time.perf_counter() - t)
                st = get_device().reads_phase_last_stats()
                ms_all.append({k: v for k, v in st.items() if k.startswith('ms_')})
            r.update(device_s=statistics.median(t_dev), device_all_s=t_dev, device_all_ms=ms_all, device_runs=runs, stats=st,
                     kernel_ms=st['ms_kernels'], n_pairs=who['n_pairs'], n_linked=who['n_linked'])
        if not device_only and n <= host_max:
            t_host = []
            for _ in range(host_runs):
                t = time.perf_counter()
                who = run(phase_reads.phase_reads, out_h)
                t_host.append(time.perf_counter() - t)
            r.update(host_s=statistics.median(t_host), host_all_s=t_host, host_runs=host_runs, host_cores=cores, n_pairs=who['n_pairs'],
                     n_linked=who['n_linked'])
            if not host_only:
                for ext in ('', '.reads', '.bed'):
                    assert open(out_h + ext, 'rb').read() == open(out_d + ext, 'rb').read(), 'the device\'s %s file differs from the host statement\'s' % (ext or 'rows')
                r.update(ratio=r['host_s'] / r['device_s'], files_equal=True)
        results.append(r)
        print(json.dumps({k: v for k, v in r.items() if not k.endswith('_all_s') and k != 'device_all_ms'}), flush=True)
    out = arg('--json', None)
    if out:
        with open(out, 'w') as fh:
            json.dump(dict(tool='tools/phase_probe.py', seed=seed, results=results), fh, indent=1)
            fh.write('\n')
    stats_csv = arg('--kernel-stats', None)
    if stats_csv and not device_only and not host_only:
        from mcaller_amd.device import get_device
        get_device().reads_phase_release()
        kernel_stats(stats_csv, min(sizes), seed)
    if not arg('--keep', None):
        shutil.rmtree(d, ignore_errors=True)


if __name__ == '__main__':
    main()
