#!/usr/bin/env python3
"""tools/bedgff_probe.py [--cases 1e6,1e7] [--runs 5] [--host-runs 1] [--json profiles/bedgff_probe.json]
                         [--kernel-stats profiles/bedgff_kernel_stats.csv] [--keep DIR] [--device-only] [--seed 7] [--no-ref]

make_bed --gff --vo --ref, host code against the device (make_bed.summarise_diffs(ref=...) / summarise_diffs_device(ref=...) with
MCALLER_BED_GFF_DEVICE=1), file to file on the same box, host and device alternating: the device's median of --runs after a
warm-up, the host function --host-runs times, with mc_bed_last_stats of the last device run.  Every device result is compared
with the host's bytes.

A case is a number of rows.  The file is synthetic and `-m A`-shaped: a site every third base of one contig, rows in read order
(runs of neighbouring sites), 17-digit probabilities, depth 20 on average; the FASTA is one contig of 4.6 million bases, 80 to a line.
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

GENOME = 4600000


def arg(name, default):
    a = sys.argv[1:]
    return a[a.index(name) + 1] if name in a else default


def write_fasta(d, seed):
    rng = random.Random(seed)
    path = os.path.join(d, 'probe.fasta')
    block = ''.join(rng.choice('ACGT') for _ in range(100003))          # (a prime-ish period: no window repeats soon)
    seq = (block * (GENOME // len(block) + 1))[:GENOME]
    with open(path, 'w') as fh:
        fh.write('>ecoli_syn synthetic, %d bases\n' % GENOME)
        fh.write('\n'.join(seq[i:i + 80] for i in range(0, GENOME, 80)) + '\n')
    return path


def write_case(d, n_rows, seed):
    rng = random.Random(seed)
    n_sites = max(1, n_rows // 20)
    path = os.path.join(d, 'probe.eventalign.diffs.6')
    with open(path, 'w') as fh:
        i = 0
        while i < n_rows:
            s0, strand = rng.randrange(n_sites), '+-'[rng.random() < 0.5]
            for s in range(s0, min(s0 + 40, n_sites)):                   # a read: 40 neighbouring sites
                if i >= n_rows:
                    break
                p = rng.random()
                fh.write('ecoli_syn\tread%d\t%d\tTTGCAMTTCAG\t1.72,-1.48,1.64,-1.9,0.53,2.725,7.05\t%s\t%s\t%s\n'
                         % (i // 40, 1000 + 3 * s, strand, 'm6A' if p >= 0.5 else 'A', repr(p)))
                i += 1
    return path, n_sites


def kernel_stats(out_csv, case, seed, extra):
    """The kernels' times of the device path alone, from a rocprofv3 run of this tool in a process of its own."""
    d = tempfile.mkdtemp(prefix='mc_bedgff_stats_')
    try:
        cmd = ['rocprofv3', '--kernel-trace', '--stats', '--output-format', 'csv', '-d', d, '--', sys.executable, os.path.abspath(__file__),
               '--device-only', '--cases', case, '--runs', '3', '--seed', str(seed)] + extra
        subprocess.run(cmd, check=True, timeout=900, stdout=subprocess.DEVNULL)
        found = glob.glob(os.path.join(d, '**', '*kernel_stats.csv'), recursive=True)
        if not found:
            raise RuntimeError('rocprofv3 left no kernel_stats.csv under %s' % d)
        shutil.copy(found[0], out_csv)
    finally:
        shutil.rmtree(d, ignore_errors=True)


def main():
    os.environ['MCALLER_BED_GFF_DEVICE'] = '1'
    from mcaller_amd import make_bed
    from mcaller_amd.device import get_device
    cases = arg('--cases', '1e6,1e7')
    runs, host_runs, seed = int(arg('--runs', '5')), int(arg('--host-runs', '1')), int(arg('--seed', '7'))
    device_only, no_ref = '--device-only' in sys.argv, '--no-ref' in sys.argv
    d = arg('--keep', None) or tempfile.mkdtemp(prefix='mc_bedgff_probe_')
    os.makedirs(d, exist_ok=True)
    ref = None if no_ref else write_fasta(d, seed)
    results = []
    for case in cases.split(','):
        n_rows = int(float(case))
        path, n_sites = write_case(d, n_rows, seed)
        outs = [os.path.join(d, 'host.gff'), os.path.join(d, 'device.gff')]
        kw = dict(with_probs=True, gff=True, ref=ref, quiet=True)

        def device():
            make_bed.summarise_diffs_device(path, outs[1], 15, 0.5, **kw)
            assert make_bed.last_summary['by'] == 'device', make_bed.last_summary

        def host():
            with warnings.catch_warnings():
                warnings.simplefilter('ignore')
                make_bed.summarise_diffs(path, outs[0], 15, 0.5, **kw)
        device()                                           # warm-up: pinned blocks, the first launches
        t_dev, t_host = [], []
        for k in range(max(runs, 0 if device_only else host_runs)):
            if k < runs:
                t = time.perf_counter()
                device()
                t_dev.append(time.perf_counter() - t)
            if not device_only and k < host_runs:
                t = time.perf_counter()
                host()
                t_host.append(time.perf_counter() - t)
        st = get_device().bed_last_stats()
        r = dict(rows=n_rows, sites=n_sites, file_bytes=os.path.getsize(path), fasta_bytes=os.path.getsize(ref) if ref else 0,
                 device_s=statistics.median(t_dev), device_all_s=t_dev, device_runs=runs, stats=st, kernel_ms=st['ms_kernels'])
        if t_host:
            assert open(outs[0], 'rb').read() == open(outs[1], 'rb').read(), 'the device summary differs from the host function\'s'
            r.update(host_s=statistics.median(t_host), host_all_s=t_host, host_runs=host_runs, ratio=statistics.median(t_host) / r['device_s'],
                     bytes_equal=True)
        results.append(r)
        print('%9d rows %7d sites %6.1f MB  host %s s  device %7.4f s  %s read %.1f ms, H2D %.1f ms, kernels %.1f ms, D2H %.1f ms; %d written'
              % (n_rows, n_sites, r['file_bytes'] / 1e6, '%8.2f' % r['host_s'] if t_host else 'not run', r['device_s'],
                 'x%-7.1f' % r['ratio'] if t_host else '', st['ms_read'], st['ms_h2d'], st['ms_kernels'], st['ms_d2h'], st['n_sites']), flush=True)
    out = arg('--json', None)
    if out:
        with open(out, 'w') as fh:
            json.dump(dict(tool='tools/bedgff_probe.py', seed=seed, options='--gff --vo' + ('' if no_ref else ' --ref'), results=results), fh, indent=1)
            fh.write('\n')
    stats_csv = arg('--kernel-stats', None)
    if stats_csv and not device_only:
        get_device().bed_release()
        kernel_stats(stats_csv, cases.split(',')[0], seed, ['--no-ref'] if no_ref else [])
    if not arg('--keep', None):
        shutil.rmtree(d, ignore_errors=True)


if __name__ == '__main__':
    main()
