#!/usr/bin/env python3
"""tools/fastq_probe.py [--reads 1e4,1e5] [--runs 5] [--host-runs 5] [--json profiles/fastq_probe.json]
                       [--kernel-stats profiles/fastq_kernel_stats.csv] [--keep DIR] [--device-only] [--seed 7]

A FASTQ file to the {read key: mean phred} dict, host reader against device reader, file to dict on the same box:
  host    read_qual.extract_read_quality          (csrc/mc_fastq.cpp on the cores this process may use)
  device  read_qual.extract_read_quality_device   (csrc/fastq/mc_fastqual.hip)
medians of --runs after a warm-up, with mc_fastq_quality_last_stats of the last device run.  Every device dict is compared with the
host's: the keys in order, the means by bits.

The file: N reads whose lengths are log-normal (sigma 1, mean about 8 kb, capped at 10^6; about one in a thousand above 10^5),
four-line records with nanopore-style titles, phred 0..59.
--kernel-stats: the kernels' times from a `rocprofv3 --kernel-trace --stats` run of this tool's own (--device-only, the smallest
file)."""
import glob
import json
import math
import os
import shutil
import statistics
import subprocess
import sys
import tempfile
import time

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))

PEAK_BYTES_PER_S = 8.0e12          # MI355X HBM3E


def arg(name, default):
    a = sys.argv[1:]
    return a[a.index(name) + 1] if name in a else default


def write_fastq(path, n, seed):
    """-> (bytes, bases, reads above 10^5 bases, the longest read)."""
    import numpy as np
    rng = np.random.default_rng(seed)
    lengths = np.minimum(rng.lognormal(math.log(8000.0) - 0.5, 1.0, n), 1e6).astype(np.int64)
    room = 1 << 22
    bases = np.frombuffer(b'ACGT', dtype=np.uint8)[rng.integers(0, 4, room + 10 ** 6)].tobytes()
    quals = rng.integers(33, 93, room + 10 ** 6, dtype=np.uint8).tobytes()
    starts = rng.integers(0, room, (n, 2))
    with open(path, 'wb', buffering=1 << 24) as out:
        for i in range(n):
            k = int(lengths[i])
            a, b = int(starts[i, 0]), int(starts[i, 1])
            out.write(b'@%08x-%04x-4c1d-9f6a-%012x_Basecall_1D_template runid=%040x read=%d ch=%d\n' % (i * 2654435761 % (1 << 32), i % 65536, i, seed, i, i % 512))
            out.write(bases[a:a + k])
            out.write(b'\n+\n')
            out.write(quals[b:b + k])
            out.write(b'\n')
    return os.path.getsize(path), int(lengths.sum()), int((lengths > 10 ** 5).sum()), int(lengths.max())


def kernel_stats(out_csv, reads, seed):
    """The kernels' times of the device path alone, from a rocprofv3 run of this tool in a process of its own."""
    d = tempfile.mkdtemp(prefix='mc_fastq_stats_')
    try:
        cmd = ['rocprofv3', '--kernel-trace', '--stats', '--output-format', 'csv', '-d', d, '--', sys.executable, os.path.abspath(__file__),
               '--device-only', '--reads', str(reads), '--runs', '3', '--seed', str(seed)]
        subprocess.run(cmd, check=True, timeout=900, stdout=subprocess.DEVNULL)
        found = glob.glob(os.path.join(d, '**', '*kernel_stats.csv'), recursive=True)
        if not found:
            raise RuntimeError('rocprofv3 left no kernel_stats.csv under %s' % d)
        shutil.copy(found[0], out_csv)
    finally:
        shutil.rmtree(d, ignore_errors=True)


def main():
    import numpy as np
    from mcaller_amd import _lib, read_qual
    from mcaller_amd.device import get_device
    sizes = [int(float(x)) for x in arg('--reads', '1e4,1e5').split(',')]
    runs, host_runs, seed = int(arg('--runs', '5')), int(arg('--host-runs', '5')), int(arg('--seed', '7'))
    device_only = '--device-only' in sys.argv
    d = arg('--keep', None) or tempfile.mkdtemp(prefix='mc_fastq_probe_')
    os.makedirs(d, exist_ok=True)
    cores = int(_lib.lib().mc_host_cores())
    results = []
    for n in sizes:
        path = os.path.join(d, 'probe%d.fastq' % n)
        n_bytes, n_bases, n_long, longest = write_fastq(path, n, seed)
        got = {}

        def device():
            got['device'] = read_qual.extract_read_quality_device(path)
            assert read_qual.last_read['by'] == 'device', read_qual.last_read

        def host():
            got['host'] = read_qual.extract_read_quality(path)

        device()                                                # warm-up: pinned blocks, the first launches, the file in the page cache
        t_dev, t_host, ms_all, st = [], [], [], None
        for _ in range(runs):
            t = time.perf_counter()
            device()
            t_dev.append(time.perf_counter() - t)
            st = get_device().fastq_qualities_last_stats()
            ms_all.append({k: v for k, v in st.items() if k.startswith('ms_')})       # the call's own split of the run
        r = dict(reads=n, file_bytes=n_bytes, bases=n_bases, reads_above_1e5=n_long, longest_read=longest, device_s=statistics.median(t_dev),
                 device_all_s=t_dev, device_all_ms=ms_all, device_runs=runs, stats=st, kernel_ms=st['ms_kernels'], piece_bytes=st['piece_bytes'],
                 kernel_bytes=3 * n_bytes + n_bases,           # the text three times (newlines twice, the classes), the quality lines once
                 kernel_fraction_of_peak=(3 * n_bytes + n_bases) / (st['ms_kernels'] * 1e-3) / PEAK_BYTES_PER_S if st['ms_kernels'] > 0 else None)
        if not device_only:
            host()
            for _ in range(host_runs):
                t = time.perf_counter()
                host()
                t_host.append(time.perf_counter() - t)
            h, v = got['host'], got['device']
            assert list(h) == list(v), 'the device reader\'s keys differ from the host reader\'s'
            assert np.asarray(list(h.values())).tobytes() == np.asarray(list(v.values())).tobytes(), 'the device reader\'s means differ'
            r.update(host_s=statistics.median(t_host), host_all_s=t_host, host_runs=host_runs, host_cores=cores,
                     ratio=statistics.median(t_host) / r['device_s'], dicts_equal=True)
        results.append(r)
        print('%8d reads %8.1f MB (%d above 10^5 bases, longest %d)  host %s s on %d cores  device %7.4f s  %s read %.1f ms, H2D %.1f ms, '
              'kernels %.2f ms (%.3f of peak), D2H %.2f ms; %d lines, %d pieces of %d bytes'
              % (n, n_bytes / 1e6, n_long, longest, '%7.4f' % r['host_s'] if t_host else 'not run', cores, r['device_s'],
                 'x%-6.2f' % r['ratio'] if t_host else '', st['ms_read'], st['ms_h2d'], st['ms_kernels'], r['kernel_fraction_of_peak'] or 0.0,
                 st['ms_d2h'], st['n_lines'], st['n_pieces'], st['piece_bytes']), flush=True)
        os.remove(path)
    out = arg('--json', None)
    if out:
        with open(out, 'w') as fh:
            json.dump(dict(tool='tools/fastq_probe.py', seed=seed, peak_bytes_per_s=PEAK_BYTES_PER_S, results=results), fh, indent=1)
            fh.write('\n')
    stats_csv = arg('--kernel-stats', None)
    if stats_csv and not device_only:
        get_device().fastq_qualities_release()
        kernel_stats(stats_csv, min(sizes), seed)
    if not arg('--keep', None):
        shutil.rmtree(d, ignore_errors=True)


if __name__ == '__main__':
    main()
