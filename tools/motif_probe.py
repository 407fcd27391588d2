#!/usr/bin/env python3
"""tools/motif_probe.py [--bases 4.6e6] [--runs 3] [--host-runs 1] [--json profiles/motif_probe.json]
                       [--kernel-stats profiles/motif_kernel_stats.csv] [--keep DIR] [--device-only] [--host-only] [--seed 7]
                       [--iupac] [--iterative [--max-motifs 16]]

A reference and two make_bed summaries to the rows of find_motifs, host statement against device, file to file on the same box:
  host    find_motifs.find_motifs          (NumPy)
  device  find_motifs.find_motifs_device   (csrc/motifs/mc_motifscan.hip)
medians of --runs after a warm-up, with mc_motif_report_last_stats of the last device run.  The device's file is compared with the
host's byte for byte.  A call the device declines is recorded with its reason and not timed.

The genome: --bases random bases on one contig with AACNNNNNNGTGC planted every ~8000 bases.  Methylated: the A of every GATC
and the second A of every AACNNNNNNGTGC, on both strands; 90 % of all candidates are covered, 1 % of the covered others are false
calls.  The first rows must be GATC:2 and AACNNNNNNGTGC:2.
--iupac: the same two legs with find_motifs --iupac (csrc/motifs/mc_motifiupac.inc).  GANTC and CAAYNNNNNRTAC are planted beside
the others, each every ~8000 bases with random letters under its degenerate positions, and the A of every GANTC and the second A
of every CAAYNNNNNRTAC are methylated too; the first rows (in the result) hold GANTC:2, GATC:2 and AACNNNNNNGTGC:2, and
CAAYNNNNNRTAC as the rows of the seven-letter shapes that explain it (CAANNNNNNRTAC:3, CAAYNNNNNNTAC:3).  Meant to be
run with --host-runs 3 --json profiles/motif_iupac_probe.json --kernel-stats profiles/motif_iupac_kernel_stats.csv; the stats of
mc_motif_report_iupac_last_stats go into the result.
--iterative: the two legs with find_motifs --iterative (csrc/motifs/mc_motifiter.inc) on the genome of --iupac, in the plain mode or,
with --iupac, in that mode; the rows AND the --unexplained files are compared.  mc_motif_report_iter_last_stats goes into the result
with ms_first_round and the mean of the later rounds (ms_later_rounds / (n_rounds - 1): each holds the explain step of the row
before it, km_uncount and the selection; in --iupac the lattices are made anew in every round).  Meant to be run with --host-runs 3
--json profiles/motif_iter_probe.json --kernel-stats profiles/motif_iter_kernel_stats.csv.
--host-only needs no GPU.  --kernel-stats: the kernels' times from a `rocprofv3 --kernel-trace --stats` run of this tool's own
(--device-only), the program behind `--`, under its own time limit."""
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

BIPARTITE = 'AACNNNNNNGTGC'
DEGENERATE = ('GANTC', 'CAAYNNNNNRTAC')        # --iupac plants these too
SETS = {'A': 'A', 'C': 'C', 'G': 'G', 'T': 'T', 'R': 'AG', 'Y': 'CT', 'N': 'ACGT'}


def arg(name, default):
    a = sys.argv[1:]
    return a[a.index(name) + 1] if name in a else default


def occurrences(seq, motif):
    """Starts of `motif` (letters of SETS; N: any letter) in the uint8 array seq."""
    import numpy as np
    n = len(seq) - len(motif) + 1
    hit = np.ones(n, dtype=bool)
    for i, ch in enumerate(motif):
        if ch != 'N':
            hit &= np.isin(seq[i:i + n], [ord(c) for c in SETS[ch]])
    return np.nonzero(hit)[0]


def write_case(d, n_bases, seed, iupac=False):
    """-> (reference, bed, control paths, dict of figures)."""
    import numpy as np
    rng = np.random.default_rng(seed)
    seq = np.frombuffer(b'ACGT', dtype=np.uint8)[rng.integers(0, 4, n_bases)].copy()
    fixed = [(i, ord(ch)) for i, ch in enumerate(BIPARTITE) if ch != 'N']
    for at in range(4000, n_bases - 100, 8000):
        for i, c in fixed:
            seq[at + i] = c
    if iupac:
        letters = np.frombuffer(b'ACGT', dtype=np.uint8)
        for motif, first in zip(DEGENERATE, (1000, 6000)):
            for at in range(first, n_bases - 100, 8000):
                for i, ch in enumerate(motif):
                    if ch != 'N':
                        seq[at + i] = ord(SETS[ch][rng.integers(0, len(SETS[ch]))]) if len(SETS[ch]) > 1 else ord(ch)
                    else:
                        seq[at + i] = letters[rng.integers(0, 4)]
    meth = np.zeros((2, n_bases), dtype=bool)                 # [strand][position]
    gatc = occurrences(seq, 'GATC')
    meth[0, gatc + 1] = True
    meth[1, gatc + 2] = True                                  # GATC is its own reverse complement: the T at +2 is the A of '-'
    meth[0, occurrences(seq, BIPARTITE) + 1] = True
    meth[1, occurrences(seq, 'GCACNNNNNNGTT') + 11] = True      # the motif on '-': its second A is the T at +11 of the reverse complement
    if iupac:
        gantc = occurrences(seq, 'GANTC')                     # its own reverse complement: the T at +3 is the A of '-'
        meth[0, gantc + 1] = True
        meth[1, gantc + 3] = True
        meth[0, occurrences(seq, 'CAAYNNNNNRTAC') + 2] = True
        meth[1, occurrences(seq, 'GTAYNNNNNRTTG') + 10] = True  # on '-': its second A is the T at +10 of the reverse complement
    cand = np.stack([seq == ord('A'), seq == ord('T')])
    covered = cand & (rng.random((2, n_bases)) < 0.9)
    called = covered & (meth | (rng.random((2, n_bases)) < 0.01))
    ref, bed, ctl = os.path.join(d, 'ref.fasta'), os.path.join(d, 'sites.bed'), os.path.join(d, 'control.bed')
    with open(ref, 'wb') as fh:
        fh.write(b'>contig_1 synthetic\n')
        text = seq.tobytes()
        fh.write(b'\n'.join(text[i:i + 80] for i in range(0, n_bases, 80)) + b'\n')
    for path, mask in ((bed, called), (ctl, covered & ~called)):
        with open(path, 'w') as fh:
            for s, strand in enumerate('+-'):
                fh.write(''.join('contig_1\t%d\t%d\tNNNNNNN\t0.9\t%s\t20\n' % (p, p + 1, strand) for p in np.nonzero(mask[s])[0].tolist()))
    return ref, bed, ctl, dict(bases=n_bases, candidates=int(cand.sum()), called=int(called.sum()), control=int((covered & ~called).sum()),
                               bed_bytes=os.path.getsize(bed), control_bytes=os.path.getsize(ctl))


def kernel_stats(out_csv, n_bases, seed, iupac=False, more=()):
    """The kernels' times of the device path alone, from a rocprofv3 run of this tool in a process of its own."""
    d = tempfile.mkdtemp(prefix='mc_motif_stats_')
    try:
        cmd = ['timeout', '-k', '10', '600', 'rocprofv3', '--kernel-trace', '--stats', '--output-format', 'csv', '-d', d, '--', sys.executable,
               os.path.abspath(__file__), '--device-only', '--bases', str(n_bases), '--runs', '2', '--seed', str(seed)]
        cmd += (['--iupac'] if iupac else []) + list(more)
        subprocess.run(cmd, check=True, stdout=subprocess.DEVNULL)
        found = glob.glob(os.path.join(d, '**', '*kernel_stats.csv'), recursive=True)
        if not found:
            raise RuntimeError('rocprofv3 left no kernel_stats.csv under %s' % d)
        shutil.copy(found[0], out_csv)
    finally:
        shutil.rmtree(d, ignore_errors=True)


def main():
    from mcaller_amd import _lib, find_motifs
    n_bases = int(float(arg('--bases', '4.6e6')))
    runs, host_runs, seed = int(arg('--runs', '3')), int(arg('--host-runs', '1')), int(arg('--seed', '7'))
    device_only, host_only, iupac = '--device-only' in sys.argv, '--host-only' in sys.argv, '--iupac' in sys.argv
    iterative, max_motifs = '--iterative' in sys.argv, int(arg('--max-motifs', '16'))
    d = arg('--keep', None) or tempfile.mkdtemp(prefix='mc_motif_probe_')
    os.makedirs(d, exist_ok=True)
    ref, bed, ctl, r = write_case(d, n_bases, seed, iupac or iterative)
    r['iupac'] = iupac
    out_d, out_h = os.path.join(d, 'device.tsv'), os.path.join(d, 'host.tsv')
    left_d, left_h = os.path.join(d, 'device.bed'), os.path.join(d, 'host.bed')
    more = {}
    if iterative:
        r.update(iterative=True, max_motifs=max_motifs)
        more = dict(iterative=True, max_motifs=max_motifs)
    r['host_cores'] = int(_lib.lib().mc_host_cores())
    if not host_only:
        from mcaller_amd.device import get_device

        def device():
            find_motifs.find_motifs_device(ref, bed, ctl, out=out_d, iupac=iupac, **(dict(more, unexplained=left_d) if iterative else {}))
            return find_motifs.last_report

        who = device()                                          # warm-up: pinned blocks, the first launches, the files in the page cache
        if who['by'] != 'device':                               # (a declined call is no measurement: the reason is the result)
            r.update(declined=who['reason'], stats=get_device().motif_report_last_stats())
        else:
            t_dev, st = [], None
            for _ in range(runs):
                t = time.perf_counter()
                device()
                t_dev.append(time.perf_counter() - t)
                st = get_device().motif_report_last_stats()
            r.update(device_s=statistics.median(t_dev), device_all_s=t_dev, device_runs=runs, stats=st, kernel_ms=st['ms_kernels'],
                     first_rows=open(out_d).read().splitlines()[:6 if iupac else 4])
            if iupac:
                r.update(iupac_stats=get_device().motif_report_iupac_last_stats())
            if iterative:
                it = get_device().motif_report_iter_last_stats()
                r.update(iter_stats=it, rows=open(out_d).read().splitlines(), ms_first_round=it['ms_first_round'],
                         ms_later_round_mean=it['ms_later_rounds'] / (it['n_rounds'] - 1) if it['n_rounds'] > 1 else None)
    if not device_only:
        t_host = []
        for _ in range(host_runs):
            t = time.perf_counter()
            find_motifs.find_motifs(ref, bed, ctl, out=out_h, iupac=iupac, **(dict(more, unexplained=left_h) if iterative else {}))
            t_host.append(time.perf_counter() - t)
        r.update(host_s=statistics.median(t_host), host_all_s=t_host, host_runs=host_runs)
        if 'device_s' in r:
            assert open(out_h, 'rb').read() == open(out_d, 'rb').read(), 'the device\'s rows differ from the host statement\'s'
            if iterative:
                assert open(left_h, 'rb').read() == open(left_d, 'rb').read(), 'the device\'s left-over sites differ from the host statement\'s'
            r.update(ratio=r['host_s'] / r['device_s'], files_equal=True)
    print(json.dumps(r), flush=True)
    out = arg('--json', None)
    if out:
        with open(out, 'w') as fh:
            json.dump(dict(tool='tools/motif_probe.py', seed=seed, result=r), fh, indent=1)
            fh.write('\n')
    stats_csv = arg('--kernel-stats', None)
    if stats_csv and not device_only and not host_only:
        from mcaller_amd.device import get_device
        get_device().motif_report_release()
        kernel_stats(stats_csv, n_bases, seed, iupac, ['--iterative', '--max-motifs', str(max_motifs)] if iterative else [])
    if not arg('--keep', None):
        shutil.rmtree(d, ignore_errors=True)


if __name__ == '__main__':
    main()
