#!/usr/bin/env python3
"""tools/currents_probe.py [--sites 2e3,2e4] [--runs 3] [--host-runs 3] [--host-max 2e3] [--json profiles/currents_probe.json]
                          [--kernel-stats profiles/currents_kernel_stats.csv] [--keep DIR] [--device-only] [--host-only] [--seed 7]

Two `-m A`-like .diffs files (a native sample and a control) to the rows of compare_currents --fdr --sig_bed, host statement against
device, file to file on the same box:
  host    compare_currents.compare_currents          (four SciPy calls a site and column in a Python loop)
  device  compare_currents.compare_currents_device   (csrc/compare/mc_sitegroup.inc, mc_curcompare.inc)
medians of --runs after a warm-up, with mc_currents_compare_last_stats of the last device run.  Every device file is compared with the
host's, byte for byte, wherever the host ran (cases of up to --host-max sites: the host takes milliseconds a site and column).  A pair
the device declines is recorded with its reason and not timed.

The files: N shared sites on one contig, 15 .. 60 rows in each file, six slot deviations in hundredths and a read quality a row, the
rows of a file in the order of the reads (sites interleaved); every fourth site stands in a GATC context and carries a planted shift
of its native deviations (1.5 / (1 + slot)).  --host-only needs no GPU.
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


def write_pair(p1, p2, n, seed):
    """-> (bytes of the native file, bytes of the control, rows in both)."""
    import numpy as np
    rng = np.random.default_rng(seed)
    total = 0
    for path, native in ((p1, True), (p2, False)):
        depth = rng.integers(15, 61, n)
        site = rng.permutation(np.repeat(np.arange(n), depth))          # the rows in the order of the reads
        shift = np.where((site % 4 == 0) & native, 1.5, 0.0)[:, None] / (1.0 + np.arange(SLOTS))
        vals = np.round(rng.normal(0.0, 1.0, (len(site), SLOTS)) + shift, 2)
        qual = np.round(rng.uniform(7.0, 12.0, len(site)), 2)
        total += len(site)
        with open(path, 'w') as fh:
            for r, s in enumerate(site):
                fh.write('contig_1\tread_%d\t%d\t%s\t%s,%r\t%s\tA\t0.5\n' % (r, 100 + 5 * s, 'ACCAGMTCTGA' if s % 4 == 0 else 'ACCATMCGTGA',
                                                                         ','.join(repr(float(v)) for v in vals[r]), float(qual[r]), '+-'[s & 1]))
    return os.path.getsize(p1), os.path.getsize(p2), total


def kernel_stats(out_csv, sites, seed):
    """The kernels' times of the device path alone, from a rocprofv3 run of this tool in a process of its own."""
    d = tempfile.mkdtemp(prefix='mc_currents_stats_')
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
    from mcaller_amd import _lib, compare_currents
    sizes = [int(float(x)) for x in arg('--sites', '2e3,2e4').split(',')]
    runs, host_runs, seed = int(arg('--runs', '3')), int(arg('--host-runs', '3')), int(arg('--seed', '7'))
    host_max = int(float(arg('--host-max', '2e3')))
    device_only, host_only = '--device-only' in sys.argv, '--host-only' in sys.argv
    d = arg('--keep', None) or tempfile.mkdtemp(prefix='mc_currents_probe_')
    os.makedirs(d, exist_ok=True)
    cores = int(_lib.lib().mc_host_cores())
    kw = dict(depth=15, fdr=True, by='mwu', threshold=2.0)
    results = []
    for n in sizes:
        p1, p2 = os.path.join(d, 'native%d.diffs.6' % n), os.path.join(d, 'control%d.diffs.6' % n)
        out_d, out_h = os.path.join(d, 'device%d.tsv' % n), os.path.join(d, 'host%d.tsv' % n)
        b1, b2, n_rows = write_pair(p1, p2, n, seed)
        r = dict(sites=n, columns=SLOTS, native_bytes=b1, control_bytes=b2, rows=n_rows, **kw)
        if not host_only:
            from mcaller_amd.device import get_device

            def device():
                compare_currents.compare_currents_device(p1, p2, out=out_d, sig_bed=out_d + '.bed', **kw)
                return compare_currents.last_compare

            who = device()                                      # warm-up: pinned blocks, the first launches, the files in the page cache
            if who['by'] != 'device':                           # (a declined pair is no measurement: the reason is the result)
                r.update(declined=who['reason'], stats=get_device().currents_compare_last_stats())
                results.append(r)
                print(json.dumps(r), flush=True)
                continue
            t_dev, ms_all, st = [], [], None
            for _ in range(runs):
                t = time.perf_counter()
                who = device()
                t_dev.append(time.perf_counter() - t)
                st = get_device().currents_compare_last_stats()
                ms_all.append({k: v for k, v in st.items() if k.startswith('ms_')})
            r.update(device_s=statistics.median(t_dev), device_all_s=t_dev, device_all_ms=ms_all, device_runs=runs, stats=st,
                     kernel_ms=st['ms_kernels'], n_sig=who['n_sig'])
        if not device_only and n <= host_max:
            t_host = []
            for _ in range(host_runs):
                t = time.perf_counter()
                compare_currents.compare_currents(p1, p2, out=out_h, sig_bed=out_h + '.bed', **kw)
                t_host.append(time.perf_counter() - t)
            r.update(host_s=statistics.median(t_host), host_all_s=t_host, host_runs=host_runs, host_cores=cores,
                     host_ms_per_site_and_column=1e3 * statistics.median(t_host) / (n * SLOTS))
            if not host_only:
                assert open(out_h, 'rb').read() == open(out_d, 'rb').read(), 'the device\'s rows differ from the host statement\'s'
                assert open(out_h + '.bed', 'rb').read() == open(out_d + '.bed', 'rb').read(), 'the device\'s bed differs from the host statement\'s'
                r.update(ratio=r['host_s'] / r['device_s'], files_equal=True)
        results.append(r)
        print(json.dumps({k: v for k, v in r.items() if not k.endswith('_all_s') and k != 'device_all_ms'}), flush=True)
    out = arg('--json', None)
    if out:
        with open(out, 'w') as fh:
            json.dump(dict(tool='tools/currents_probe.py', seed=seed, results=results), fh, indent=1)
            fh.write('\n')
    stats_csv = arg('--kernel-stats', None)
    if stats_csv and not device_only and not host_only:
        from mcaller_amd.device import get_device
        get_device().currents_compare_release()
        kernel_stats(stats_csv, min(sizes), seed)
    if not arg('--keep', None):
        shutil.rmtree(d, ignore_errors=True)


if __name__ == '__main__':
    main()
