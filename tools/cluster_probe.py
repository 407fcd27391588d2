#!/usr/bin/env python3
"""tools/cluster_probe.py [--sites 2e3,2e4] [--deep 4] [--runs 3] [--host-runs 3] [--host-max 2e3] [--json profiles/cluster_probe.json]
                         [--kernel-stats profiles/cluster_kernel_stats.csv] [--keep DIR] [--device-only] [--host-only] [--seed 7]

One `-m A`-like .diffs file to the rows of cluster_sites --mixed_bed, host statement against device, file to file on the same box:
  host    cluster_sites.cluster_sites          (NumPy distances and a merge loop per site in Python)
  device  cluster_sites.cluster_sites_device   (csrc/compare/mc_sitegroup.inc, mc_sitecluster.inc)
medians of --runs after a warm-up, with mc_sites_cluster_last_stats of the last device run.  Every device file is compared with the
host's, byte for byte, wherever the host ran (cases of up to --host-max sites).  A file the device declines is recorded with its reason
and not timed.

The file: N sites on one contig, 15 .. 60 rows each, and --deep sites of 100, 200, 400, ... rows (capped at --max_depth 1024); six slot
deviations in hundredths and a read quality a row, the rows in the order of the reads (sites interleaved); every fourth site carries
a planted second population -- half of its rows shifted by 2.5 in the even slots and labelled m6A.  --host-only needs no GPU.
--kernel-stats: the kernels' times from a `rocprofv3 --kernel-trace --stats` run of this tool's own (--device-only, the smallest
case): each new kernel's share."""
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

SLOTS = 6


def arg(name, default):
    a = sys.argv[1:]
    return a[a.index(name) + 1] if name in a else default


def write_file(path, n, deep, seed):
    """-> (bytes of the file, its rows)."""
    import numpy as np
    rng = np.random.default_rng(seed)
    depth = np.concatenate([rng.integers(15, 61, n), np.minimum(100 * 2 ** np.arange(deep), 1100)]).astype(np.int64)
    site = rng.permutation(np.repeat(np.arange(len(depth)), depth))      # the rows in the order of the reads
    second = (site % 4 == 0) & (rng.random(len(site)) < 0.5)
    vals = rng.normal(0.0, 1.0, (len(site), SLOTS))
    vals[:, ::2] += np.where(second, 2.5, 0.0)[:, None]
    vals = np.round(vals, 2)
    qual = np.round(rng.uniform(7.0, 12.0, len(site)), 2)
    with open(path, 'w') as fh:
        for r, s in enumerate(site):
            fh.write('contig_1\tread_%d\t%d\t%s\t%s,%r\t%s\t%s\t0.5\n' % (r, 100 + 5 * s, 'ACCAGMTCTGA' if s % 4 == 0 else 'ACCATMCGTGA',
                                                                     ','.join(repr(float(v)) for v in vals[r]), float(qual[r]), '+-'[s & 1],
                                                                     'm6A' if second[r] else 'A'))
    return os.path.getsize(path), len(site)


def kernel_stats(out_csv, sites, deep, seed):
    """The kernels' times of the device path alone, from a rocprofv3 run of this tool in a process of its own."""
    d = tempfile.mkdtemp(prefix='mc_cluster_stats_')
    try:
        cmd = ['rocprofv3', '--kernel-trace', '--stats', '--output-format', 'csv', '-d', d, '--', sys.executable, os.path.abspath(__file__),
               '--device-only', '--sites', str(sites), '--deep', str(deep), '--runs', '3', '--seed', str(seed)]
        subprocess.run(cmd, check=True, timeout=600, stdout=subprocess.DEVNULL)
        found = glob.glob(os.path.join(d, '**', '*kernel_stats.csv'), recursive=True)
        if not found:
            raise RuntimeError('rocprofv3 left no kernel_stats.csv under %s' % d)
        shutil.copy(found[0], out_csv)
    finally:
        shutil.rmtree(d, ignore_errors=True)


def main():
    from mcaller_amd import _lib, cluster_sites
    sizes = [int(float(x)) for x in arg('--sites', '2e3,2e4').split(',')]
    runs, host_runs, seed, deep = int(arg('--runs', '3')), int(arg('--host-runs', '3')), int(arg('--seed', '7')), int(arg('--deep', '4'))
    host_max = int(float(arg('--host-max', '2e3')))
    device_only, host_only = '--device-only' in sys.argv, '--host-only' in sys.argv
    d = arg('--keep', None) or tempfile.mkdtemp(prefix='mc_cluster_probe_')
    os.makedirs(d, exist_ok=True)
    cores = int(_lib.lib().mc_host_cores())
    kw = dict(depth=15, max_depth=1024, metric='correlation', min_minor=0.2, min_gap=1.3)
    results = []
    for n in sizes:
        p = os.path.join(d, 'reads%d.diffs.6' % n)
        out_d, out_h = os.path.join(d, 'device%d.tsv' % n), os.path.join(d, 'host%d.tsv' % n)
        n_bytes, n_rows = write_file(p, n, deep, seed)
        r = dict(sites=n, deep_sites=deep, columns=SLOTS, file_bytes=n_bytes, rows=n_rows, **kw)
        if not host_only:
            from mcaller_amd.device import get_device

            def device():
                cluster_sites.cluster_sites_device(p, out=out_d, mixed_bed=out_d + '.bed', **kw)
                return cluster_sites.last_cluster

            who = device()                                      # warm-up: pinned blocks, the first launches, the file in the page cache
            if who['by'] != 'device':                           # (a declined file is no measurement: the reason is the result)
                r.update(declined=who['reason'], stats=get_device().sites_cluster_last_stats())
                results.append(r)
                print(json.dumps(r), flush=True)
                continue
            t_dev, ms_all, st = [], [], None
            for _ in range(runs):
                t = time.perf_counter()
                who = device()
                t_dev.append(time.perf_counter() - t)
                st = get_device().sites_cluster_last_stats()
                ms_all.append({k: v for k, v in st.items() if k.startswith('ms_')})
            r.update(device_s=statistics.median(t_dev), device_all_s=t_dev, device_all_ms=ms_all, device_runs=runs, stats=st,
                     kernel_ms=st['ms_kernels'], n_mixed=who['n_mixed'])
        if not device_only and n <= host_max:
            t_host = []
            for _ in range(host_runs):
                t = time.perf_counter()
                cluster_sites.cluster_sites(p, out=out_h, mixed_bed=out_h + '.bed', **kw)
                t_host.append(time.perf_counter() - t)
            r.update(host_s=statistics.median(t_host), host_all_s=t_host, host_runs=host_runs, host_cores=cores,
                     host_ms_per_site=1e3 * statistics.median(t_host) / (n + deep))
            if not host_only:
                assert open(out_h, 'rb').read() == open(out_d, 'rb').read(), 'the device\'s rows differ from the host statement\'s'
                assert open(out_h + '.bed', 'rb').read() == open(out_d + '.bed', 'rb').read(), 'the device\'s bed differs from the host statement\'s'
                r.update(ratio=r['host_s'] / r['device_s'], files_equal=True)
        results.append(r)
        print(json.dumps({k: v for k, v in r.items() if not k.endswith('_all_s') and k != 'device_all_ms'}), flush=True)
    out = arg('--json', None)
    if out:
        with open(out, 'w') as fh:
            json.dump(dict(tool='tools/cluster_probe.py', seed=seed, results=results), fh, indent=1)
            fh.write('\n')
    stats_csv = arg('--kernel-stats', None)
    if stats_csv and not device_only and not host_only:
        from mcaller_amd.device import get_device
        get_device().sites_cluster_release()
        kernel_stats(stats_csv, min(sizes), deep, seed)
    if not arg('--keep', None):
        shutil.rmtree(d, ignore_errors=True)


if __name__ == '__main__':
    main()
