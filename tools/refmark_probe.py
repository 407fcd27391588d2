#!/usr/bin/env python3
"""tools/refmark_probe.py [--bases 4.6e6,2.5e8] [--specs GATC,GANTC,'GANTC,CAAYNNNNNRTAC:3,CRAANNNNNNNTGC:3+4' as ;-separated list]
                         [--runs 5] [--json profiles/refmark_probe.json] [--kernel-stats profiles/refmark_kernel_stats.csv]
                         [--device-only] [--seed 7]

The site masks of a --motifs spec made on the GPU (mc_ctx_set_reference_iupac: k_ref_planes, k_mark_iupac) against what marked the
same sites before --motifs existed, on one random contig of --bases bases:
  GATC              mc_ctx_set_reference_motif (k_mark_words) on the device, mc_mark_motifs on the host
  degenerate specs  refmark.methylate_positions over the list of sites, both strands (what a -p file costs once it is written)
and against the host's own marking of the spec (mc_mark_iupac).  Medians of --runs after a warm-up; a device call is timed from
the raw bases on the host to the masks and the site numbering on the device (staging, the copy and the kernels).  The device's
masks are compared with the host's marking every time.
--kernel-stats: the kernels' own times from a `rocprofv3 --kernel-trace --stats` run of this tool in a process of its own
(--device-only)."""
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

SPECS = 'GATC;GANTC;GANTC,CAAYNNNNNRTAC:3,CRAANNNNNNNTGC:3+4'


def arg(name, default):
    a = sys.argv[1:]
    return a[a.index(name) + 1] if name in a else default


def median_s(fn, runs):
    fn()                                                     # warm-up: allocations, the first launches
    ts = []
    for _ in range(runs):
        t = time.perf_counter()
        fn()
        ts.append(time.perf_counter() - t)
    return statistics.median(ts), ts


def kernel_stats(out_csv, argv):
    d = tempfile.mkdtemp(prefix='mc_refmark_stats_')
    try:
        cmd = ['rocprofv3', '--kernel-trace', '--stats', '--output-format', 'csv', '-d', d, '--', sys.executable, os.path.abspath(__file__),
               '--device-only'] + argv
        subprocess.run(cmd, check=True, timeout=900, stdout=subprocess.DEVNULL)
        found = glob.glob(os.path.join(d, '**', '*kernel_stats.csv'), recursive=True)
        if not found:
            raise RuntimeError('rocprofv3 left no kernel_stats.csv under %s' % d)
        shutil.copy(found[0], out_csv)
    finally:
        shutil.rmtree(d, ignore_errors=True)


def main():
    import numpy as np
    from mcaller_amd import refmark
    from mcaller_amd.device import get_device
    sizes = [int(float(x)) for x in arg('--bases', '4.6e6,2.5e8').split(',')]
    specs = arg('--specs', SPECS).split(';')
    runs, seed = int(arg('--runs', '5')), int(arg('--seed', '7'))
    device_only = '--device-only' in sys.argv
    dev = get_device()
    d = tempfile.mkdtemp(prefix='mc_refmark_probe_')
    results = []
    for n in sizes:
        rng = np.random.default_rng(seed)
        fa = os.path.join(d, 'probe%d.fa' % n)
        with open(fa, 'wb') as fh:
            fh.write(b'>probe\n' + np.frombuffer(b'ACGT', dtype=np.uint8)[rng.integers(0, 4, n)].tobytes() + b'\n')
        for text in specs:
            spec = refmark.parse_motifs(text, 'A')
            ref = refmark.MarkedReference(fa, 'A', spec, None)
            raw, native = ref.raw_arrays(), ref.iupac_for_the_device()
            n_words = int(raw['n_words'])
            r = dict(bases=n, spec=spec.text, runs=runs)
            r['device_s'], r['device_all_s'] = median_s(lambda: dev.set_reference_iupac(raw, native), runs)
            _, mf, mr, _, _, _, n_sites = dev.fetch_reference(int(raw['n_seq_bytes']), n_words, 1)
            r['n_sites'] = int(n_sites)
            if not device_only:
                def host():
                    ref.meth.clear()
                    ref.mark(0)
                r['host_iupac_s'], _ = median_s(host, min(runs, 3))
                want = ref.device_arrays()
                assert np.array_equal(mf, want['mbits_fwd']) and np.array_equal(mr, want['mbits_rev']), 'the device masks differ from the host marking'
                r['masks_equal_host'] = True
                if text == 'GATC':
                    lit = refmark.MarkedReference(fa, 'A', 'GATC', None)
                    dm = lit.motif_for_the_device()
                    r['parent'] = 'mc_ctx_set_reference_motif; mc_mark_motifs'
                    r['parent_device_s'], _ = median_s(lambda: dev.set_reference_motif(raw, *dm), runs)
                    _, lf, lr, _, _, _, _ = dev.fetch_reference(int(raw['n_seq_bytes']), n_words, 1)
                    assert np.array_equal(lf, mf) and np.array_equal(lr, mr), 'k_mark_words and k_mark_iupac disagree on GATC'

                    def host_literal():
                        lit.meth.clear()
                        lit.mark(0)
                    r['parent_host_s'], _ = median_s(host_literal, min(runs, 3))
                else:
                    upper = ref.upper(0)
                    sites = [np.nonzero(np.unpackbits(m.view(np.uint8), bitorder='little')[:n])[0].tolist() for m in (mf, mr)]
                    r['parent'] = 'refmark.methylate_positions over the site list'

                    def by_positions():
                        return (refmark.methylate_positions(upper, sites[0], 'A'), refmark.methylate_positions(upper, sites[1], 'T'))
                    r['parent_host_s'], _ = median_s(by_positions, 1)
                    assert by_positions() == tuple(ref.meth[0]), 'positions mode over the site list differs'
            results.append(r)
            print('%10d bases  %-46s %9d sites  device %8.4f s  host mc_mark_iupac %s  before: %s' % (
                n, spec.text, r['n_sites'], r['device_s'], '%8.4f s' % r['host_iupac_s'] if 'host_iupac_s' in r else 'not run',
                ', '.join('%s %.4f s' % (k, r[k]) for k in ('parent_device_s', 'parent_host_s') if k in r) or 'not run'), flush=True)
        os.remove(fa)
    shutil.rmtree(d, ignore_errors=True)
    out = arg('--json', None)
    if out:
        with open(out, 'w') as fh:
            json.dump(dict(tool='tools/refmark_probe.py', seed=seed, results=results), fh, indent=1)
            fh.write('\n')
    stats_csv = arg('--kernel-stats', None)
    if stats_csv and not device_only:
        kernel_stats(stats_csv, ['--bases', arg('--bases', '4.6e6,2.5e8'), '--specs', arg('--specs', SPECS), '--runs', '3', '--seed', str(seed)])


if __name__ == '__main__':
    main()
