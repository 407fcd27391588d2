"""Small texts for the feed the four file pipelines share (mcaller_amd/csrc/mc_textfeed.h; tests/test_gpu_textfeed.py): one case per
pipeline -- the bed summary (a `.diffs` text with a positions list and a FASTA: three files in one call), the merge behind `-t N`,
the rows of a `--training_tsv` file, the read qualities of a FASTQ file -- made from the texts the pipelines' own tests use, each
of 800 bytes to a few KB, so that MCALLER_TEXT_STAGE_BYTES=256 cuts it into more than three blocks.  A case runs its pipeline on
files (`run_file`), on the same bytes as host texts (`run_text`) and through the host function (`run_host`); the three results
compare equal.  `mixed` is the sequence the shared stages make possible: every pipeline in turn on one context."""
import os

import numpy as np

KNOB = 'MCALLER_TEXT_STAGE_BYTES'
PIPELINES = ('bed', 'merge', 'train', 'fastq')
BLOCKS = ('n', 'n-1', 'half', 'half-1', 'third', '256')


def block_size(which, n):
    """The stage sizes of one text of n bytes: one block; a last block of one byte; exactly two blocks; three, the third tiny (the
    first reuse of stage 0, so the event wait); three blocks; many, with lines across every edge."""
    half = -(-n // 2)
    return {'n': n, 'n-1': n - 1, 'half': half, 'half-1': half - 1, 'third': -(-n // 3), '256': 256}[which]


class Case(object):
    """files: {name: bytes}, written to `directory` under their names; the first is the text the stats count (n bytes)."""

    def __init__(self, name, directory, files, none):
        self.name, self.dir, self.files, self.none = name, str(directory), files, none
        self.n = len(next(iter(files.values())))
        self.paths = {}
        for key, blob in files.items():
            self.paths[key] = os.path.join(self.dir, '%s.%s' % (name, key))
            with open(self.paths[key], 'wb') as fh:
                fh.write(blob)

    def check_stats(self, dev):
        st = self.stats(dev)
        assert st['n_bytes'] == self.n and st['ms_read'] > 0, (self.name, st)
        assert {k: st[k] for k in self.none} == self.none, (self.name, st)


class Bed(Case):
    KW = dict(gff=True, min_depth=1)

    def __init__(self, directory):
        from tests import gffstats_files as G
        fasta, text = G.ref_cases()['repeated_id']
        lines = text.splitlines(True)[::6]                             # (every contig and both strands stay)
        listed = [b'\t'.join([f[0], f[2], b'%d' % (int(f[2]) + 1), f[5]]) + b'\n' for f in (l.split(b'\t') for l in lines[::2])]
        positions = b''.join(listed)
        while len(positions) <= 512:
            positions += positions                                     # (a position listed twice is listed)
        Case.__init__(self, 'bed', directory, dict(diffs=b''.join(lines), positions=positions, fasta=fasta * 2),
                      dict(decline_reason=0, decline_line=-1))

    def run_file(self, dev):
        blob, n, why = dev.bed_summarise(path=self.paths['diffs'], positions_path=self.paths['positions'], ref_path=self.paths['fasta'], **self.KW)
        assert why is None, why
        return blob, n

    def run_text(self, dev):
        blob, n, why = dev.bed_summarise(text=self.files['diffs'], positions_text=self.files['positions'], ref_text=self.files['fasta'], **self.KW)
        assert why is None, why
        return blob, n

    def run_host(self):
        from mcaller_amd import make_bed
        out = os.path.join(self.dir, 'bed.host')
        n = make_bed.summarise_diffs(self.paths['diffs'], out, 1, 0.5, positions=self.paths['positions'], gff=True, ref=self.paths['fasta'])
        with open(out, 'rb') as fh:
            return fh.read(), n

    def stats(self, dev):
        return dev.bed_last_stats()


class Merge(Case):
    def __init__(self, directory, parts=None, name='merge'):
        from tests import merge_files as MF
        if parts is None:
            parts = [b''.join(MF.edge_cases()['cli_host_dealt'])]      # (the three parts as one file)
        self.parts = parts
        Case.__init__(self, name, directory, {'part%d' % i: p for i, p in enumerate(parts)}, dict(decline_reason=0, decline_line=-1, decline_file=-1))
        self.n = sum(len(p) for p in parts)

    def run_file(self, dev, want_decline=False):
        out = os.path.join(self.dir, self.name + '.merged')
        n, why = dev.merge_rows(paths=[self.paths['part%d' % i] for i in range(len(self.parts))], out_path=out)
        if want_decline:
            assert n is None and not os.path.exists(out) and not os.path.exists(out + '.merging')
            return why
        assert why is None, why
        with open(out, 'rb') as fh:
            blob = fh.read()
        os.remove(out)
        assert n == blob.count(b'\n')
        return blob

    def run_text(self, dev):
        blob, why = dev.merge_rows(text=b''.join(self.parts))
        assert why is None, why
        return blob

    def run_host(self):
        from tests import merge_files as MF
        return MF.host_merge(self.parts, self.dir)

    def stats(self, dev):
        return dev.merge_rows_last_stats()


class Train(Case):
    def __init__(self, directory):
        from tests import train_rows_files as T
        text, info = T.random_file(1, 8)
        assert info['long_line'] < 0 and info['n_labels'] == 2
        Case.__init__(self, 'train', directory, dict(train=text), dict(decline_reason=0, decline_line=-1))

    @staticmethod
    def _result(labels, sig, grp, why):
        assert why is None, why
        return labels, {k: (v.shape, v.tobytes()) for k, v in sig.items()}, {k: v.tolist() for k, v in grp.items()}

    @staticmethod
    def _pairs():
        from mcaller_amd.extract_contexts import base_models
        return sorted(base_models('A', False))

    def run_file(self, dev):
        return self._result(*dev.training_rows(path=self.paths['train'], pairs=self._pairs()))

    def run_text(self, dev):
        return self._result(*dev.training_rows(text=self.files['train'], pairs=self._pairs()))

    def run_host(self):
        """tsv2matrix's dicts in the device result's form: one sub-model key, labels in first-occurrence order."""
        from mcaller_amd import load_mCaller_data as L
        signals, contexts = L.tsv2matrix(self.paths['train'], 'A')
        (key, sig), = signals.items()
        nf = max(len(r) for rows in sig.values() for r in rows)
        X = {k: np.asarray(v, dtype=np.float64).reshape(len(v), nf) for k, v in sig.items()}
        return list(sig), {k: (v.shape, v.tobytes()) for k, v in X.items()}, {k: [c.encode('ascii') for c in v] for k, v in contexts[key].items()}

    def stats(self, dev):
        return dev.training_rows_last_stats()


class Fastq(Case):
    def __init__(self, directory):
        from tests import fastq_cases as F
        Case.__init__(self, 'fastq', directory, dict(fastq=F.random_fastq(np.random.default_rng(11), 4)), dict(decline_reason=0, decline_line=-1))

    @staticmethod
    def _result(keys, means, why):
        assert why is None, why
        return keys, means.tobytes()

    def run_file(self, dev):
        return self._result(*dev.fastq_qualities(path=self.paths['fastq']))

    def run_text(self, dev):
        return self._result(*dev.fastq_qualities(text=self.files['fastq']))

    def run_host(self):
        from mcaller_amd import _lib
        keys, means, decline = _lib.fastq_records_host(self.files['fastq'])
        assert decline is None
        return keys, means.tobytes()

    def stats(self, dev):
        return dev.fastq_qualities_last_stats()


def cases(directory):
    """{pipeline: case}, the files written under `directory`."""
    made = dict(bed=Bed(directory), merge=Merge(directory), train=Train(directory), fastq=Fastq(directory))
    assert all(800 <= case.n <= 8192 for case in made.values()), {name: case.n for name, case in made.items()}
    return made


def sized_part(size, seed):
    """A part file of exactly `size` bytes: rows of tests/merge_files.py, the last line filled up; no line of another seed's."""
    from tests import merge_files as MF
    if size == 0:
        return b''
    out, room = [], size
    for row in MF.name_rows(MF.CLI_HOST_NAMES, seed=seed, times=1):
        row = b's%d' % seed + row
        if room - len(row) < 12:
            break
        out.append(row)
        room -= len(row)
    out.append(b'fill%d\t%d\t' % (seed, seed) + b'f' * (room - len(b'fill%d\t%d\t\n' % (seed, seed))) + b'\n')
    part = b''.join(out)
    assert len(part) == size and part.endswith(b'\n')
    return part


def mixed(dev, directory):
    """FASTQ, bed, training rows, merge and FASTQ again on one context, no release in between, the knob as the caller set it: every
    result is its text= twin's.  Then every release, and one small call of each pipeline."""
    made = cases(directory)
    twins = {name: case.run_text(dev) for name, case in made.items()}
    for name in ('fastq', 'bed', 'train', 'merge', 'fastq'):
        assert made[name].run_file(dev) == twins[name], name
        made[name].check_stats(dev)
    dev.fastq_qualities_release()
    dev.bed_release()
    dev.training_rows_release()
    dev.merge_rows_release()
    for name in PIPELINES:
        assert made[name].run_file(dev) == twins[name], ('behind the releases', name)
        assert made[name].run_text(dev) == twins[name], ('behind the releases', name)
