#!/usr/bin/env python3
"""tools/evaluate_probe.py [--sites 50000] [--runs 3] [--json profiles/evaluate_probe.json]
                           [--kernel-stats profiles/evaluate_kernel_stats.csv] [--keep DIR] [--device-only] [--seed 7]

evaluate, host statement against the device (evaluate.evaluate_calls / evaluate_calls_device), file to file on the same box: the
median of --runs of each (the device after a warm-up), once with the default depths and once with 16 depths up to 1024, with
mc_eval_last_stats of the last device run.  Every device result is compared with the host's bytes; a device run that declines
(a rounding tie in an expected table) is recorded as declined, with no ratio.

The files are synthetic: --sites labelled sites of depth 15 .. 60 (about 1.9 10^6 rows at the default), both classes, calls correlated
with the truth, two-decimal probabilities, rows in random order, one unlabelled and one non-M row in forty.
--kernel-stats: the kernels' times from a `rocprofv3 --kernel-trace --stats` run of this tool's own (--device-only, 16 depths)."""
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

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))

DEPTHS_16 = (1, 2, 3, 5, 8, 10, 15, 20, 30, 40, 50, 60, 128, 256, 512, 1024)


def arg(name, default):
    a = sys.argv[1:]
    return a[a.index(name) + 1] if name in a else default


def write_case(d, n_sites, seed):
    """-> (diffs path, positions path, rows)."""
    rng = random.Random(seed)
    path, pos = os.path.join(d, 'probe.eventalign.diffs.6'), os.path.join(d, 'probe.positions')
    rows = []
    with open(pos, 'w') as fh:
        for s in range(n_sites):
            positive = rng.random() < 0.5
            fh.write('ecoli_syn\t%d\t%s\t%s\t\n' % (1000 + 3 * s, '+-'[s & 1], 'm6A' if positive else 'A'))
            for i in range(rng.randint(15, 60)):
                p = min(1.0, max(0.0, rng.gauss(0.65 if positive else 0.35, 0.25)))
                text = repr(round(p, 2))
                rows.append('ecoli_syn\tread%d\t%d\tTTGCAMTTCAG\t-0.4,1.6,7.05\t%s\t%s\t%s\n' % (i, 1000 + 3 * s, '+-'[s & 1], 'm6A' if float(text) >= 0.5 else 'A', text))
            if s % 40 == 0:
                rows.append('ecoli_syn\tread0\t%d\tTTGCAMTTCAG\t-0.4,1.6,7.05\t+\tA\t0.5\n' % (1001 + 3 * s))
                rows.append('ecoli_syn\tread0\t%d\tTTGCAATTCAG\t-0.4,1.6,7.05\t+\tA\t0.5\n' % (1000 + 3 * s))
    rng.shuffle(rows)
    with open(path, 'w') as fh:
        fh.writelines(rows)
    return path, pos, len(rows)


def kernel_stats(out_csv, n_sites, seed):
    """The kernels' times of the device path alone, from a rocprofv3 run of this tool in a process of its own."""
    d = tempfile.mkdtemp(prefix='mc_eval_stats_')
    try:
        cmd = ['rocprofv3', '--kernel-trace', '--stats', '--output-format', 'csv', '-d', d, '--', sys.executable, os.path.abspath(__file__),
               '--device-only', '--sites', str(n_sites), '--runs', '3', '--seed', str(seed)]
        subprocess.run(cmd, check=True, timeout=900, stdout=subprocess.DEVNULL)
        found = glob.glob(os.path.join(d, '**', '*kernel_stats.csv'), recursive=True)
        if not found:
            raise RuntimeError('rocprofv3 left no kernel_stats.csv under %s' % d)
        shutil.copy(found[0], out_csv)
    finally:
        shutil.rmtree(d, ignore_errors=True)


def main():
    from mcaller_amd import evaluate
    from mcaller_amd.device import get_device
    n_sites, runs, seed = int(float(arg('--sites', '50000'))), int(arg('--runs', '3')), int(arg('--seed', '7'))
    device_only = '--device-only' in sys.argv
    d = arg('--keep', None) or tempfile.mkdtemp(prefix='mc_eval_probe_')
    os.makedirs(d, exist_ok=True)
    path, pos, n_rows = write_case(d, n_sites, seed)
    results = []
    for name, depths in (('16 depths up to 1024', DEPTHS_16),) if device_only else (('default depths', evaluate.DEFAULT_DEPTHS), ('16 depths up to 1024', DEPTHS_16)):
        data = evaluate.evaluate_calls_device(path, pos, 15, depths)              # warm-up: pinned blocks, the first launches
        reason = evaluate.last_eval['reason']
        t_dev, t_host, ms_all = [], [], []
        for _ in range(runs):
            t = time.perf_counter()
            data = evaluate.evaluate_calls_device(path, pos, 15, depths)
            t_dev.append(time.perf_counter() - t)
            ms_all.append({k: v for k, v in get_device().eval_calls_last_stats().items() if k.startswith('ms_')})
        st = get_device().eval_calls_last_stats()
        r = dict(case=name, depths=list(depths), sites=n_sites, rows=n_rows, file_bytes=os.path.getsize(path), positions_bytes=os.path.getsize(pos),
                 device_s=statistics.median(t_dev), device_all_s=t_dev, device_all_ms=ms_all, device_runs=runs, stats=st,
                 served=data is not None, decline=reason)
        if not device_only:
            want = None
            for _ in range(runs):
                t = time.perf_counter()
                want = evaluate.evaluate_calls(path, pos, 15, depths)
                t_host.append(time.perf_counter() - t)
            r.update(host_s=statistics.median(t_host), host_all_s=t_host, host_runs=runs)
            if data is not None:
                assert data == want, 'the device evaluation differs from the host statement\'s'
                r.update(ratio=r['host_s'] / r['device_s'], bytes_equal=True)
        results.append(r)
        print('%-22s %8d rows %6d sites %6.1f MB  host %s s  device %7.4f s %s %s  truth %.1f ms, rows %.1f ms, expect %.1f ms, finish %.1f ms'
              % (name, n_rows, n_sites, r['file_bytes'] / 1e6, '%8.2f' % r['host_s'] if t_host else 'not run', r['device_s'],
                 'x%-7.1f' % r['ratio'] if 'ratio' in r else '', 'served' if data is not None else 'DECLINED: %s' % reason,
                 st['ms_truth'], st['ms_rows'], st['ms_expect'], st['ms_finish']), flush=True)
    out = arg('--json', None)
    if out:
        with open(out, 'w') as fh:
            json.dump(dict(tool='tools/evaluate_probe.py', seed=seed, results=results), fh, indent=1)
            fh.write('\n')
    stats_csv = arg('--kernel-stats', None)
    if stats_csv and not device_only:
        get_device().eval_calls_release()
        kernel_stats(stats_csv, n_sites, seed)
    if not arg('--keep', None):
        shutil.rmtree(d, ignore_errors=True)


if __name__ == '__main__':
    main()
