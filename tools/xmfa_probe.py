#!/usr/bin/env python3
"""tools/xmfa_probe.py [--bases 4.6e6] [--runs 3] [--json profiles/xmfa_probe.json] [--kernel-stats profiles/xmfa_kernel_stats.csv]
                      [--keep DIR] [--device-only] [--host-only] [--seed 7]

Two genomes with their own assemblies compared through a Mauve alignment, host statement against device, file to file on the same
box:
  host    compare_genomes.compare_by_position(xmfa_path=...)          (NumPy over the columns, four SciPy calls a site)
  device  compare_genomes.compare_by_position_device(xmfa_path=...)   (csrc/compare/mc_xmfamap.inc, mc_bedcompare.hip)
medians of --runs after a warm-up; the map alone as well (compare_genomes.xmfa_map against Device.xmfa_map, view included).  The
device's rows are compared with the host's byte for byte, its map with the host's.

The pair: a random genome of --bases bases on one contig and a copy on two contigs (a contig break) with an indel of 1 .. 30 bases
about every 50 kb and its middle tenth inverted: three blocks (+/+, +/-, +/+), wrapped at 80; a site at the A of every GATC of
genome 1 at depths 15 .. 60, nine in ten with their partner in bed2.
--kernel-stats: the kernels' times from a `rocprofv3 --kernel-trace --stats` run of this tool's own (--device-only); kx_pack and
kx_columns get the bytes they touch over their time, beside the 8 TB/s peak."""
import csv
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

PEAK_TBS = 8.0


def arg(name, default):
    a = sys.argv[1:]
    return a[a.index(name) + 1] if name in a else default


def wrapped(text, width=80):
    return '\n'.join(text[i:i + width] for i in range(0, len(text), width))


def write_pair(d, n_bases, seed):
    """The five files -> dict of paths and figures."""
    import numpy as np
    from mcaller_amd import compare_genomes as CG
    rng = np.random.default_rng(seed)
    genome = np.frombuffer(b'ACGT', dtype=np.uint8)[rng.integers(0, 4, n_bases)]
    cuts = [0, int(n_bases * 0.45), int(n_bases * 0.55), n_bases]
    blocks, at2 = [], 0
    for k in range(3):
        a0, a1 = cuts[k], cuts[k + 1]
        t1, t2, pos = [], [], a0
        while pos < a1:
            step = min(a1 - pos, int(rng.integers(30000, 70000)))
            piece = genome[pos:pos + step].tobytes().decode()
            t1.append(piece); t2.append(piece)
            pos += step
            if pos < a1:
                n = int(rng.integers(1, 31))
                if rng.random() < 0.5:                                 # bases genome 2 lacks
                    n = min(n, a1 - pos)
                    t1.append(genome[pos:pos + n].tobytes().decode()); t2.append('-' * n)
                    pos += n
                else:                                                  # bases of its own
                    t1.append('-' * n); t2.append('ACGT'[int(rng.integers(4))] * n)
        t1, t2 = ''.join(t1), ''.join(t2)
        n2 = len(t2) - t2.count('-')
        blocks.append((a0 + 1, a1, '+', t1, at2 + 1, at2 + n2, '+-'[k == 1], t2))
        at2 += n2
    P = {name: os.path.join(d, name) for name in ('a.bed', 'b.bed', 'ab.xmfa', 'a.fai', 'b.fai')}
    with open(P['ab.xmfa'], 'w') as fo:
        fo.write('#FormatVersion Mauve1\n')
        for s1, e1, st1, t1, s2, e2, st2, t2 in blocks:
            fo.write('> 1:%d-%d %s a.fasta\n%s\n> 2:%d-%d %s b.fasta\n%s\n=\n' % (s1, e1, st1, wrapped(t1), s2, e2, st2, wrapped(t2)))
    open(P['a.fai'], 'w').write('contig_a\t%d\t10\t80\t81\n' % n_bases)
    open(P['b.fai'], 'w').write('contig_b1\t%d\t11\t80\t81\ncontig_b2\t%d\t99\t80\t81\n' % (at2 // 2, at2 - at2 // 2))
    # the sites: the A of every GATC
    g = genome
    hits = np.flatnonzero((g[:-3] == 71) & (g[1:-2] == 65) & (g[2:-1] == 84) & (g[3:] == 67)) + 1
    contigs1, contigs2 = CG._contigs(P['a.fai']), CG._contigs(P['b.fai'])
    g2, flip = CG.xmfa_map(P['ab.xmfa'], n_bases, (1, 2), at2)
    l1, l2, values = [], [], 0
    for i, p in enumerate(hits.tolist()):
        n1, n2 = (int(v) for v in rng.integers(15, 61, 2))
        x, y = np.round(rng.random(n1), 2), np.round(rng.random(n2), 2)
        if i % 4 == 0:
            y = np.round(np.clip(y + 0.3, 0.0, 1.0), 2)
        row = lambda chrom, start, strand, v: '%s\t%d\t%d\tGATC\t%s\t%s\t%d\t%s\n' % (
            chrom, start, start + 1, repr(round(float((v >= 0.5).mean()), 4)), strand, len(v), ','.join(repr(float(q)) for q in v))
        l1.append(row('contig_a', p, '+', x))
        image = CG.lift_key(('contig_a', str(p), str(p + 1), '+'), contigs1, contigs2, g2, flip)
        if image is not None and i % 10 != 9:
            l2.append(row(image[0], int(image[1]), image[3], y))
            values += n1 + n2
    open(P['a.bed'], 'w').write(''.join(l1))
    open(P['b.bed'], 'w').write(''.join(l2[::-1]))
    P.update(n1=n_bases, n2=at2, sites=len(l1), partners=len(l2), probabilities=values, xmfa_bytes=os.path.getsize(P['ab.xmfa']),
             bed1_bytes=os.path.getsize(P['a.bed']), bed2_bytes=os.path.getsize(P['b.bed']))
    return P


def kernel_stats(out_csv, n_bases, seed):
    d = tempfile.mkdtemp(prefix='mc_xmfa_stats_')
    try:
        cmd = ['rocprofv3', '--kernel-trace', '--stats', '--output-format', 'csv', '-d', d, '--', sys.executable, os.path.abspath(__file__),
               '--device-only', '--bases', str(n_bases), '--runs', '3', '--seed', str(seed)]
        subprocess.run(cmd, check=True, timeout=900, stdout=subprocess.DEVNULL)
        found = glob.glob(os.path.join(d, '**', '*kernel_stats.csv'), recursive=True)
        if not found:
            raise RuntimeError('rocprofv3 left no kernel_stats.csv under %s' % d)
        shutil.copy(found[0], out_csv)
    finally:
        shutil.rmtree(d, ignore_errors=True)


def traffic(stats_csv, xs):
    """kx_pack and kx_columns: the bytes they touch (the text of the paired entries once and the planes' words; a column's share of
    four words of planes and prefixes and the 8 bytes of its atomicMin, read and written) over their average time."""
    touched = {'kx_pack': 2 * xs['n_columns'] + 16 * xs['n_words'], 'kx_columns': 32 * xs['n_words'] + 16 * xs['n_mapped']}
    out = {}
    for row in csv.DictReader(open(stats_csv)):
        for name, n_bytes in touched.items():
            if name in row.get('Name', ''):
                ns = float(row['AverageNs'])
                out[name] = dict(bytes=n_bytes, average_us=ns / 1e3, tb_per_s=n_bytes / ns / 1e3, of_peak=n_bytes / ns / 1e3 / PEAK_TBS)
    return out


def main():
    import numpy as np
    from mcaller_amd import _lib, compare_genomes as CG
    n_bases, runs, seed = int(float(arg('--bases', '4.6e6'))), int(arg('--runs', '3')), int(arg('--seed', '7'))
    device_only, host_only = '--device-only' in sys.argv, '--host-only' in sys.argv
    d = arg('--keep', None) or tempfile.mkdtemp(prefix='mc_xmfa_probe_')
    os.makedirs(d, exist_ok=True)
    P = write_pair(d, n_bases, seed)
    lift = dict(xmfa_path=P['ab.xmfa'], fai1=P['a.fai'], fai2=P['b.fai'])
    out_d, out_h = os.path.join(d, 'device.tsv'), os.path.join(d, 'host.tsv')
    r = {k: v for k, v in P.items() if not k.endswith(('.bed', '.xmfa', '.fai'))}
    r['host_cores'] = int(_lib.lib().mc_host_cores())
    if not host_only:
        from mcaller_amd.device import get_device
        dev = get_device()

        def device():
            CG.compare_by_position_device(P['a.bed'], P['b.bed'], out=out_d, **lift)
            return CG.last_compare

        who = device()
        if who['by'] != 'device':
            r.update(declined=who['reason'], stats=dev.bed_compare_last_stats(), map_stats=dev.xmfa_map_last_stats())
        else:
            t_dev, t_map = [], []
            for _ in range(runs):
                t = time.perf_counter()
                device()
                t_dev.append(time.perf_counter() - t)
            cs, xs = dev.bed_compare_last_stats(), dev.xmfa_map_last_stats()
            for _ in range(runs):
                t = time.perf_counter()
                dev_g2, dev_flip, why = dev.xmfa_map(path=P['ab.xmfa'], n1=P['n1'], n2=P['n2'])
                t_map.append(time.perf_counter() - t)
            dev.xmfa_map_release()
            r.update(device_s=statistics.median(t_dev), device_all_s=t_dev, device_map_s=statistics.median(t_map), device_runs=runs,
                     n_sites=who['n_sites'], n_unaligned=who['n_unaligned'], stats=cs, map_stats=xs, map_kernel_ms=xs['ms_kernels'])
    if not device_only:
        t_host, t_map = [], []
        for _ in range(runs):
            t = time.perf_counter()
            CG.compare_by_position(P['a.bed'], P['b.bed'], out=out_h, **lift)
            t_host.append(time.perf_counter() - t)
        for _ in range(runs):
            t = time.perf_counter()
            host_g2, host_flip = CG.xmfa_map(P['ab.xmfa'], P['n1'], (1, 2), P['n2'])
            t_map.append(time.perf_counter() - t)
        r.update(host_s=statistics.median(t_host), host_all_s=t_host, host_map_s=statistics.median(t_map), host_runs=runs)
        if 'device_s' in r:
            assert open(out_h, 'rb').read() == open(out_d, 'rb').read(), "the device's rows differ from the host statement's"
            assert np.array_equal(host_g2, dev_g2) and np.array_equal(host_flip, dev_flip), "the device's map differs from the host's"
            r.update(ratio=r['host_s'] / r['device_s'], map_ratio=r['host_map_s'] / r['device_map_s'], files_equal=True, maps_equal=True)
    stats_csv = arg('--kernel-stats', None)
    if stats_csv and 'device_s' in r and not device_only:
        get_device().bed_compare_release()
        kernel_stats(stats_csv, n_bases, seed)
        r['traffic'] = traffic(stats_csv, r['map_stats'])
    print(json.dumps({k: v for k, v in r.items() if not k.endswith('_all_s')}), flush=True)
    out = arg('--json', None)
    if out:
        with open(out, 'w') as fh:
            json.dump(dict(tool='tools/xmfa_probe.py', seed=seed, result=r), fh, indent=1)
            fh.write('\n')
    if not arg('--keep', None):
        shutil.rmtree(d, ignore_errors=True)


if __name__ == '__main__':
    main()
