#!/usr/bin/env python3
"""tools/trainrows_probe.py [--rows 1e5,1e6] [--runs 5] [--host-runs 3] [--json profiles/trainrows_probe.json] [--keep DIR]

A `--training_tsv` file to the arrays a fit starts from, host code against the device, file to arrays on the same box:
  host    load_mCaller_data.tsv2matrix + train_model.balanced_rows + np.asarray(fp64)   (what `--training_tsv` did before)
  device  load_mCaller_data.tsv2matrix_device + train_model.balanced_arrays             (csrc/train/mc_trainrows.hip)
median of --runs after a warm-up (the host: --host-runs), with mc_train_rows_last_stats of the last device run.

The file: N labelled rows like a `.diffs.6.train` file's -- seven features, each repr() of the mean of one to four 4-decimal
values, two labels, ~3000 distinct 11-character contexts.  Every device result is compared with the host's, floats by bits."""
import json
import os
import random
import statistics
import sys
import tempfile
import time

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))


def arg(name, default):
    a = sys.argv[1:]
    return a[a.index(name) + 1] if name in a else default


def write_rows(path, n, seed=1):
    rng = random.Random(seed)
    contexts = []
    for _ in range(3000):
        c = [rng.choice('ACGT') for _ in range(11)]
        c[5] = 'M'
        contexts.append(''.join(c))
    with open(path, 'w') as out:
        block = []
        for i in range(n):
            feats = []
            for _ in range(6):
                k = rng.randint(1, 4)
                x = sum(rng.randint(-120000, 120000) for _ in range(k)) / 1e4 / k
                feats.append(repr(x if abs(x) >= 1e-7 else 0.25))     # (a residue like 3.5e-16 is outside mc_decimal.h's exponents: a decline)
            feats.append(repr(rng.randint(50000, 140000) / 1e4))
            block.append('ecoli\t%08x-read_Basecall_2D_template\t%d\t%s\t%s\t%s\t%s\n'
                         % (rng.getrandbits(32), rng.randrange(1, 4600000), rng.choice(contexts), ','.join(feats), rng.choice('+-'),
                            'm6A' if rng.random() < 0.5 else 'A'))
            if len(block) == 65536:
                out.write(''.join(block))
                block = []
        out.write(''.join(block))
    return os.path.getsize(path)


def timed(fn, runs, warm=True):
    if warm:
        fn()
    times = []
    for _ in range(runs):
        t = time.perf_counter()
        fn()
        times.append(time.perf_counter() - t)
    return statistics.median(times), times


def main():
    import numpy as np
    from mcaller_amd import load_mCaller_data as L
    from mcaller_amd import train_model
    from mcaller_amd.device import get_device
    sizes = [int(float(x)) for x in arg('--rows', '1e5,1e6').split(',')]
    runs, host_runs = int(arg('--runs', '5')), int(arg('--host-runs', '3'))
    d = arg('--keep', None) or tempfile.mkdtemp(prefix='mc_trainrows_probe_')
    os.makedirs(d, exist_ok=True)
    results = []
    for n in sizes:
        path = os.path.join(d, 'probe%d.diffs.6.train' % n)
        n_bytes = write_rows(path, n)
        got = {}
        parts = {}

        def host():
            t0 = time.perf_counter()
            sig, grp = L.tsv2matrix(path, 'A')
            t1 = time.perf_counter()
            labs, sigs, grps = train_model.balanced_rows(sig['general'], grp['general'])
            X = np.asarray(sigs, dtype=np.float64)
            t2 = time.perf_counter()
            parts['host'] = dict(tsv2matrix_s=t1 - t0, balance_asarray_s=t2 - t1)
            got['host'] = (labs, X, grps)

        def device():
            t0 = time.perf_counter()
            sig, grp = L.tsv2matrix_device(path, 'A')
            t1 = time.perf_counter()
            assert L.last_load['by'] == 'device', L.last_load
            labs, X, grps = train_model.balanced_arrays(sig['general'], grp['general'])
            t2 = time.perf_counter()
            parts['device'] = dict(tsv2matrix_device_s=t1 - t0, balance_s=t2 - t1)
            got['device'] = (labs, X, grps)
            ms_all.append({k: v for k, v in get_device().training_rows_last_stats().items() if k.startswith('ms_')})       # the call's own split of the run

        ms_all = []
        t_dev, all_dev = timed(device, runs)
        st = get_device().training_rows_last_stats()
        t_host, all_host = timed(host, host_runs, warm=host_runs > 1)
        h, v = got['host'], got['device']
        assert h[0] == v[0] and h[1].tobytes() == v[1].tobytes() and h[2] == [c.decode('ascii') for c in v[2].tolist()], \
            'the device matrices differ from the host function\'s'
        r = dict(rows=n, file_bytes=n_bytes, host_s=t_host, device_s=t_dev, ratio=t_host / t_dev, host_runs=host_runs, device_runs=runs,
                 host_all_s=all_host, device_all_s=all_dev, device_all_ms=ms_all[-runs:], host_parts=parts['host'], device_parts=parts['device'], stats=st,
                 kernel_ms=st['ms_kernels'])
        results.append(r)
        print('%9d rows  host %7.3f s (tsv2matrix %.3f)  device %7.4f s  x%-6.1f  read %.1f ms, H2D %.1f ms, kernels %.2f ms, D2H %.1f ms, '
              'call %.1f ms; %d kept rows, %d features' % (n, t_host, parts['host']['tsv2matrix_s'], t_dev, t_host / t_dev, st['ms_read'], st['ms_h2d'],
                                                           st['ms_kernels'], st['ms_d2h'], st['ms_total'], st['n_kept'], st['n_features']), flush=True)
        os.remove(path)
    out = arg('--json', None)
    if out:
        with open(out, 'w') as fh:
            json.dump(dict(tool='tools/trainrows_probe.py', results=results), fh, indent=1)
            fh.write('\n')


if __name__ == '__main__':
    main()
