#!/usr/bin/env python3
"""tools/bed_probe.py [--rows 1e6,1e7] [--runs 5] [--host-runs 5] [--json profiles/bed_probe.json] [--keep DIR]

The summary of a dense `.diffs.6` file, host code against the device (make_bed.summarise_diffs / summarise_diffs_device), file to
file on the same box: median of --runs after a warm-up (the host function: --host-runs, it takes a minute at 10^7 rows), for
BED and for --vo, with mc_bed_last_stats of the last device run.

The file: a synthetic eventalign table (synth.make_table, written by mc_synth_write_tsv) called with `-m A` -- the rows are the
caller's own, ~0.13 per event.  A size the base file does not reach is made of copies of it, the contig renamed per copy
(`ecoli_syn.3`), so that every copy brings its own sites.  Every device result is compared with the host's bytes."""
import contextlib
import io
import json
import os
import statistics
import sys
import tempfile
import time

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))

PEAK_BYTES_PER_S = 8.0e12          # MI355X HBM3E


def arg(name, default):
    a = sys.argv[1:]
    return a[a.index(name) + 1] if name in a else default


def base_file(d, n_rows):
    """-> path of a dense .diffs.6 with about n_rows rows, its row count."""
    from mcaller_amd import mCaller, synth
    codes = synth.genome()
    table, qual = synth.make_table(int(n_rows / 0.125), seed=5, codes=codes)
    paths = synth.write_inputs(table, qual, codes, d)
    model = os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), 'mcaller_amd', 'models', 'r95_twobase_model_NN_6_m6A.npz')
    with contextlib.redirect_stdout(io.StringIO()):
        mCaller.main(['-m', 'A', '-r', paths['fasta'], '-e', paths['tsv'], '-f', paths['fastq'], '-d', model])
    os.remove(paths['tsv'])
    out = paths['tsv'][:-4] + '.diffs.6'
    with open(out, 'rb') as fh:
        return out, sum(chunk.count(b'\n') for chunk in iter(lambda: fh.read(1 << 24), b''))


def copies_of(base, n_base, n_rows, path):
    text = open(base, 'rb').read()
    times = max(1, int(round(n_rows / float(n_base))))
    with open(path, 'wb') as out:
        for i in range(times):
            out.write(text if i == 0 else (b'\n' + text).replace(b'\necoli_syn\t', b'\necoli_syn.%d\t' % i)[1:])
    return times * n_base


def timed(fn, runs, warm=True):
    if warm:
        fn()                                               # warm-up
    times = []
    for _ in range(runs):
        t = time.perf_counter()
        fn()
        times.append(time.perf_counter() - t)
    return statistics.median(times), times


def main():
    from mcaller_amd import make_bed
    from mcaller_amd.device import get_device
    sizes = [int(float(x)) for x in arg('--rows', '1e6,1e7').split(',')]
    runs, host_runs = int(arg('--runs', '5')), int(arg('--host-runs', '5'))
    d = arg('--keep', None) or tempfile.mkdtemp(prefix='mc_bed_probe_')
    os.makedirs(d, exist_ok=True)
    base, n_base = base_file(d, min(min(sizes), 10 ** 6))
    results = []
    for n in sizes:
        path = os.path.join(d, 'probe%d.diffs.6' % n)
        rows = copies_of(base, n_base, n, path)
        for vo in (False, True):
            outs = [os.path.join(d, 'host.bed'), os.path.join(d, 'device.bed')]
            host = lambda: make_bed.summarise_diffs(path, outs[0], 1, 0.5, with_probs=vo, quiet=True)
            ms_all = []                                        # the call's own split of every device run, the warm-up included

            def dev():
                make_bed.summarise_diffs_device(path, outs[1], 1, 0.5, with_probs=vo, quiet=True)
                ms_all.append({k: v for k, v in get_device().bed_last_stats().items() if k.startswith('ms_')})
            t_dev, all_dev = timed(dev, runs)
            assert make_bed.last_summary['by'] == 'device', make_bed.last_summary
            st = get_device().bed_last_stats()
            t_host, all_host = timed(host, host_runs, warm=host_runs > 1)       # (a single host run: the interpreter has nothing to warm)
            assert open(outs[0], 'rb').read() == open(outs[1], 'rb').read(), 'the device summary differs from the host function\'s'
            r = dict(rows=rows, file_bytes=os.path.getsize(path), vo=vo, host_s=t_host, device_s=t_dev, ratio=t_host / t_dev,
                     host_runs=host_runs, device_runs=runs, host_all_s=all_host, device_all_s=all_dev, device_all_ms=ms_all[-runs:], stats=st,
                     kernel_ms=st['ms_kernels'], kernel_bytes=st['kernel_bytes'],
                     kernel_fraction_of_peak=st['kernel_bytes'] / (st['ms_kernels'] * 1e-3) / PEAK_BYTES_PER_S if st['ms_kernels'] > 0 else None)
            results.append(r)
            print('%9d rows %s  host %8.3f s  device %7.4f s  x%-7.1f read %.1f ms, H2D %.1f ms, kernels %.1f ms (%.3f of peak), D2H %.1f ms; '
                  '%d entries, %d sites, longest probe %d' % (rows, '--vo' if vo else 'BED ', t_host, t_dev, t_host / t_dev, st['ms_read'], st['ms_h2d'],
                                                             st['ms_kernels'], r['kernel_fraction_of_peak'] or 0.0, st['ms_d2h'], st['n_entries'],
                                                             st['n_sites'], st['longest_probe']), flush=True)
        os.remove(path)
    out = arg('--json', None)
    if out:
        with open(out, 'w') as fh:
            json.dump(dict(tool='tools/bed_probe.py', options='-d 1 -t 0.5', peak_bytes_per_s=PEAK_BYTES_PER_S, results=results), fh, indent=1)
            fh.write('\n')


if __name__ == '__main__':
    main()
