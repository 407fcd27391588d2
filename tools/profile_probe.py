#!/usr/bin/env python3
"""tools/profile_probe.py [--contigs 3000] [--mean-length 2000] [--neighbours 10] [--runs 3] [--host-runs 3] [--seed 7]
                         [--json profiles/profile_probe.json] [--kernel-stats profiles/profile_kernel_stats.csv] [--keep DIR]
                         [--device-only] [--host-only]

A synthetic assembly and two make_bed summaries to the two files of motif_profile, host statement against device, file to file on
the same box:
  host    motif_profile.motif_profile          (NumPy)
  device  motif_profile.motif_profile_device   (csrc/motifs/mc_motifprofile.inc)
medians of --runs after a warm-up (the files are in the page cache by then), with mc_motif_profile_last_stats of the last device run:
the split into read, copies and kernels.  Both of the device's files are compared with the host's byte for byte.  A call the device
declines is recorded with its reason and not timed.  --device-only leaves the host statement out: the result says "not timed".

The assembly: --contigs contigs of 0.5 to 1.5 x --mean-length random bases, each drawn from one of six "organisms"; an organism
methylates its own 5 or 6 of the 16 motifs below.  90 % of the sites are covered; a covered site of a motif its organism methylates
is called with probability 0.95, any other with probability 0.01.  The bed lists the called sites, the control the other covered
sites of the 16 motifs.  The second size of the README row is --contigs 30000.

--json: the result goes under the key of its contig count into the file, beside what other sizes left there.  --kernel-stats: the
kernels' times from a `rocprofv3 --kernel-trace --stats` run of this tool's own (--device-only, no counters in that run), the
program behind `--`, under its own time limit; the kq_* kernels' mean times go into the result with the bytes each moves by
construction over that time against the 8 TB/s peak, and for kq_nn the pairs per second.  --host-only needs no GPU."""
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

MOTIFS = ['GATC:2', 'CATG:2', 'GTAC:3', 'TCGA:4', 'AGCT:1', 'TTAA:3', 'ACGT:1', 'TGCA:4', 'GANTC:2', 'CCAGG:3', 'GCAGC:3', 'RAATTY:3',
          'CTGCAG:5', 'GAATTC:3', 'GGTACC:4', 'AAGCTT:2']
N_ORGANISMS = 6
PEAK_BYTES_PER_S = 8e12


def arg(name, default):
    a = sys.argv[1:]
    return a[a.index(name) + 1] if name in a else default


def write_case(d, n_contigs, mean_length, seed):
    """-> (reference, bed, control paths, dict of figures)."""
    import numpy as np
    from mcaller_amd import motif_profile as MP
    rng = np.random.default_rng(seed)
    lens = rng.integers(mean_length // 2, mean_length * 3 // 2 + 1, n_contigs)
    organism = rng.integers(0, N_ORGANISMS, n_contigs)
    active = np.zeros((N_ORGANISMS, len(MOTIFS)), dtype=bool)
    for o in range(N_ORGANISMS):
        active[o, rng.choice(len(MOTIFS), 5 + o % 2, replace=False)] = True
    at = np.zeros(n_contigs + 1, dtype=np.int64)
    at[1:] = np.cumsum(lens + MP.PAD)
    G = int(at[-1])
    of_pos = np.repeat(np.arange(n_contigs), lens + MP.PAD)
    inside = np.arange(G) - at[of_pos] < lens[of_pos]
    code = np.where(inside, rng.integers(0, 4, G), 4).astype(np.uint8)
    specs = MP.parse_profile_motifs(','.join(MOTIFS), 'A')
    site = np.zeros((2, G), dtype=bool)
    meth = np.zeros((2, G), dtype=bool)
    for m, spec in enumerate(specs):
        for s, table in enumerate(spec.strands()):
            marks = MP._marks(code, *table[0])
            site[s] |= marks
            meth[s] |= marks & active[organism[of_pos], m]
    covered = site & (rng.random((2, G)) < 0.9)
    called = covered & (rng.random((2, G)) < np.where(meth, 0.95, 0.01))
    names = ['contig_%d' % i for i in range(n_contigs)]
    ref, bed, ctl = os.path.join(d, 'ref.fasta'), os.path.join(d, 'sites.bed'), os.path.join(d, 'control.bed')
    letters = np.frombuffer(b'ACGTN', dtype=np.uint8)[code].tobytes()
    with open(ref, 'wb') as fh:
        for i, name in enumerate(names):
            seq = letters[at[i]:at[i] + lens[i]]
            fh.write(b'>%s organism_%d\n' % (name.encode(), organism[i]))
            fh.write(b'\n'.join(seq[j:j + 80] for j in range(0, len(seq), 80)) + b'\n')
    for path, mask in ((bed, called), (ctl, covered & ~called)):
        with open(path, 'w') as fh:
            for s, strand in enumerate('+-'):
                g = np.nonzero(mask[s])[0]
                c = of_pos[g]
                p = g - at[c]
                fh.write(''.join('%s\t%d\t%d\tNNNNNNN\t0.9\t%s\t20\n' % (names[ci], pi, pi + 1, strand) for ci, pi in zip(c.tolist(), p.tolist())))
    return ref, bed, ctl, dict(contigs=n_contigs, bases=int(lens.sum()), motifs=len(MOTIFS), sites=int(site.sum()), called=int(called.sum()),
                               control=int((covered & ~called).sum()), ref_bytes=os.path.getsize(ref), bed_bytes=os.path.getsize(bed),
                               control_bytes=os.path.getsize(ctl))


def kernel_stats(out_csv, more):
    """The kernels' times of the device path alone, from a rocprofv3 run of this tool in a process of its own -> {kernel: mean ns}."""
    d = tempfile.mkdtemp(prefix='mc_profile_stats_')
    try:
        cmd = ['timeout', '-k', '10', '600', 'rocprofv3', '--kernel-trace', '--stats', '--output-format', 'csv', '-d', d, '--', sys.executable,
               os.path.abspath(__file__), '--device-only', '--runs', '2'] + list(more)
        subprocess.run(cmd, check=True, stdout=subprocess.DEVNULL)
        found = glob.glob(os.path.join(d, '**', '*kernel_stats.csv'), recursive=True)
        if not found:
            raise RuntimeError('rocprofv3 left no kernel_stats.csv under %s' % d)
        shutil.copy(found[0], out_csv)
    finally:
        shutil.rmtree(d, ignore_errors=True)
    mean = {}
    with open(out_csv) as fh:
        for row in csv.DictReader(fh):
            name = (row.get('Name') or '').split('(')[0].split('::')[-1].strip()
            if name.startswith('kq_') and row.get('AverageNs'):
                mean[name] = float(row['AverageNs'])
    return mean


def main():
    from mcaller_amd import _lib, motif_profile as MP
    n_contigs, mean_length, K = int(arg('--contigs', '3000')), int(arg('--mean-length', '2000')), int(arg('--neighbours', '10'))
    runs, host_runs, seed = int(arg('--runs', '3')), int(arg('--host-runs', '3')), int(arg('--seed', '7'))
    device_only, host_only = '--device-only' in sys.argv, '--host-only' in sys.argv
    d = arg('--keep', None) or tempfile.mkdtemp(prefix='mc_profile_probe_')
    os.makedirs(d, exist_ok=True)
    ref, bed, ctl, r = write_case(d, n_contigs, mean_length, seed)
    r.update(neighbours=K, host_cores=int(_lib.lib().mc_host_cores()))
    kw = dict(motifs=','.join(MOTIFS), neighbours=K)
    out_d, nn_d, out_h, nn_h = (os.path.join(d, n) for n in ('device.tsv', 'device.nn', 'host.tsv', 'host.nn'))
    if not host_only:
        from mcaller_amd.device import get_device

        def device():
            MP.motif_profile_device(ref, bed, ctl, out=out_d, nn=nn_d, **kw)
            return MP.last_report

        who = device()                                          # warm-up: pinned blocks, the first launches, the files in the page cache
        if who['by'] != 'device':                               # (a declined call is no measurement: the reason is the result)
            r.update(declined=who['reason'], stats=get_device().motif_profile_last_stats())
        else:
            t_dev, st = [], None
            for _ in range(runs):
                t = time.perf_counter()
                device()
                t_dev.append(time.perf_counter() - t)
                st = get_device().motif_profile_last_stats()
            r.update(device_s=statistics.median(t_dev), device_all_s=t_dev, device_runs=runs, stats=st,
                     split_ms={k: st[k] for k in ('ms_read', 'ms_h2d', 'ms_kernels', 'ms_d2h', 'ms_total', 'ms_counts', 'ms_neighbours')},
                     first_rows=open(out_d).read().splitlines()[:3], first_neighbours=open(nn_d).read().splitlines()[:3])
    if device_only:
        r.update(host_s='not timed')
    else:
        t_host = []
        for _ in range(host_runs):
            t = time.perf_counter()
            MP.motif_profile(ref, bed, ctl, out=out_h, nn=nn_h, **kw)
            t_host.append(time.perf_counter() - t)
        r.update(host_s=statistics.median(t_host), host_all_s=t_host, host_runs=host_runs, host_counts=MP.last_counts)
        if 'device_s' in r:
            assert open(out_h, 'rb').read() == open(out_d, 'rb').read(), 'the device\'s profile differs from the host statement\'s'
            assert open(nn_h, 'rb').read() == open(nn_d, 'rb').read(), 'the device\'s neighbours differ from the host statement\'s'
            r.update(ratio=r['host_s'] / r['device_s'], files_equal=True)
    stats_csv = arg('--kernel-stats', None)
    if stats_csv and not device_only and not host_only and 'stats' in r and 'declined' not in r:
        from mcaller_amd.device import get_device
        get_device().motif_profile_release()
        mean_ns = kernel_stats(stats_csv, ['--contigs', str(n_contigs), '--mean-length', str(mean_length), '--neighbours', str(K), '--seed', str(seed)])
        st = r['stats']
        B, M = st['n_bins'], len(MOTIFS)
        n_words = (r['bases'] + 64 * n_contigs) // 64               # (about: every contig is padded to whole words)
        moved = {'kq_count': n_words * 8 * 7 + B * M * 12,          # three code planes, four site planes, the counters
                 'kq_profile': B * M * (12 + 8 + 8) + B * 8,
                 'kq_rows': B * M * (12 + 16) + st['n_out_bytes'],
                 'kq_nn': B * (M * 8 + 8) * ((B + 63) // 64) + B * K * 16,      # every workgroup stages every candidate once
                 'kq_nn_sizes': B * K * (16 + 8), 'kq_nn_rows': B * K * (16 + 16) + st['n_nn_bytes']}
        r['kernels'] = {k: dict(mean_us=v / 1e3, bytes_by_construction=moved.get(k), share_of_peak=(moved[k] / (v * 1e-9) / PEAK_BYTES_PER_S if k in moved else None))
                        for k, v in mean_ns.items()}
        if 'kq_nn' in mean_ns:
            r['kernels']['kq_nn']['pairs_per_s'] = B * (B - 1) / (mean_ns['kq_nn'] * 1e-9)
    print(json.dumps(r), flush=True)
    out = arg('--json', None)
    if out:
        doc = dict(tool='tools/profile_probe.py', seed=seed, sizes={})
        if os.path.exists(out):
            with open(out) as fh:
                doc = json.load(fh)
        doc['sizes'][str(n_contigs)] = r
        with open(out, 'w') as fh:
            json.dump(doc, fh, indent=1)
            fh.write('\n')
    if not arg('--keep', None):
        shutil.rmtree(d, ignore_errors=True)


if __name__ == '__main__':
    main()
