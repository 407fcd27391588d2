"""The host frame the ten file pipelines share (mcaller_amd/csrc/mc_textfeed.h: pipeline_call, fetch_out, release_pipeline, fits):
what a call leaves in the context -- its result, its stats, its pinned blocks -- behind a release, behind a decline, for an
empty result and under the three memory knobs.  Every pipeline runs a few lines of the texts its own tests use; what the
results ARE is those tests' business, here a result is held against the same call's earlier result."""
import pytest

from mcaller_amd import _lib
from tests import bed_files as B
from tests import cluster_cases as CK
from tests import currents_cases as K
from tests import evaluate_cases as EC
from tests import fastq_cases as F
from tests import gpu_compare_cases as GC
from tests import merge_files as MF
from tests import motif_sites as MS
from tests import sitegroup_cases as SG
from tests import textfeed_cases as TF
from tests import xmfa_cases as X

pytestmark = pytest.mark.gpu

NAMES = ('bed', 'merge', 'train', 'fastq', 'eval', 'cmp', 'currents', 'clusters', 'xmfa', 'motif')


def write(directory, name, blob):
    path = str(directory / name)
    with open(path, 'wb') as fh:
        fh.write(blob)
    return path


class Pipe(object):
    """One pipeline: run(dev, 'text' | 'path') -> its result, comparable and without a reason; decline(dev, monkeypatch) -> what
    the device method returned for an input it declines; after it `declined`: what the stats must say (the call's own byte
    counts, the reason, the line) and `zeroed`: the counters a good call fills."""
    knob = None

    def stats(self, dev):
        return getattr(dev, self.last_stats)()

    def release(self, dev):
        getattr(dev, self.releaser)()

    def knob_decline(self, dev, monkeypatch, call):
        monkeypatch.setenv(self.knob, '1')
        got = call()
        monkeypatch.delenv(self.knob)
        return got


class Fed(Pipe):
    """The four pipelines tests/textfeed_cases.py has cases of."""

    def __init__(self, directory, name, last_stats, releaser, zeroed):
        self.case = getattr(TF, name.capitalize())(directory)
        self.last_stats, self.releaser, self.zeroed = last_stats, releaser, zeroed

    def run(self, dev, how):
        return self.case.run_text(dev) if how == 'text' else self.case.run_file(dev)


class Bed(Fed):
    def __init__(self, directory):
        Fed.__init__(self, directory, 'bed', 'bed_last_stats', 'bed_release', ('n_counted', 'n_entries', 'n_sites', 'n_out_bytes'))

    def decline(self, dev, monkeypatch):
        text, opts, reason, line = B.decline_cases()['six_fields']
        self.declined = dict(n_bytes=len(text), decline_reason=reason, decline_line=line)
        self.why, self.none = 'declines', (None, 0)
        return dev.bed_summarise(text=text, min_depth=opts['depth'], mod_threshold=opts['thresh'])


class Merge(Fed):
    def __init__(self, directory):
        Fed.__init__(self, directory, 'merge', 'merge_rows_last_stats', 'merge_rows_release', ('n_lines_out', 'n_out_bytes', 'n_rounds'))

    def decline(self, dev, monkeypatch):
        parts, reason, line = MF.decline_cases()['carriage_return']
        text = b''.join(parts)
        self.declined = dict(n_bytes=len(text), decline_reason=_lib.MERGE_DECLINE[reason], decline_line=line, decline_file=0)
        self.why, self.none = 'declines', (None,)
        return dev.merge_rows(text=text)


class Train(Fed):
    def __init__(self, directory):
        Fed.__init__(self, directory, 'train', 'training_rows_last_stats', 'training_rows_release', ('n_kept', 'n_labels', 'n_features'))

    def decline(self, dev, monkeypatch):
        good = 'c\tr\t5\tAAAAAMGAAAA\t1.5,2.5,-3.25,4.0,5.5,6.75\t+\tm6A'
        text = '\n'.join([good, '', good, '']).encode()                # an empty line: fewer than 7 fields
        self.declined = dict(n_bytes=len(text), decline_reason=3, decline_line=1)
        self.why, self.none = 'declines', (None, None, None)
        return dev.training_rows(text=text, pairs=self.case._pairs())


class Fastq(Fed):
    def __init__(self, directory):
        Fed.__init__(self, directory, 'fastq', 'fastq_qualities_last_stats', 'fastq_qualities_release', ('n_records', 'n_pieces'))

    def decline(self, dev, monkeypatch):
        name, text, reason, line = F.DECLINES[1]                       # a blank line between records
        self.declined = dict(n_bytes=len(text), decline_reason=reason, decline_line=line)
        self.why, self.none = 'declines', (None, None)
        return dev.fastq_qualities(text=text)


class Eval(Pipe):
    last_stats, releaser, knob = 'eval_calls_last_stats', 'eval_calls_release', 'MCALLER_EVAL_DEVICE_BYTES'
    zeroed = ('n_rows', 'n_pos_lines', 'n_kept', 'n_sites', 'n_expect')
    KW = dict(min_depth=3, depths=(1, 2, 3, 5, 10))

    def __init__(self, directory):
        self.diffs, self.positions = EC.random_case(6)                  # (no value near a rounding tie: tests/test_gpu_evaluate_calls.py)
        self.paths = write(directory, 'e.diffs.6', self.diffs), write(directory, 'e.positions', self.positions)

    def run(self, dev, how):
        if how == 'text':
            blob, why = dev.eval_calls(text=self.diffs, positions_text=self.positions, **self.KW)
        else:
            blob, why = dev.eval_calls(path=self.paths[0], positions_path=self.paths[1], **self.KW)
        assert why is None, why
        return blob

    def decline(self, dev, monkeypatch):
        diffs = self.diffs + b'\n'
        self.declined = dict(n_bytes=len(diffs), n_pos_bytes=len(self.positions), decline_reason=_lib.EVAL_DECLINE['memory'], decline_line=-1,
                             decline_file=0)
        self.why, self.none = 'do not fit', (None,)
        return self.knob_decline(dev, monkeypatch, lambda: dev.eval_calls(text=diffs, positions_text=self.positions, **self.KW))


class Cmp(Pipe):
    last_stats, releaser, knob = 'bed_compare_last_stats', 'bed_compare_release', 'MCALLER_CMP_DEVICE_BYTES'
    zeroed = ('n_lines1', 'n_lines2', 'n_sites', 'n_values', 'n_out_bytes')

    def __init__(self, directory):
        self.t1, self.t2 = GC.key_pair()
        self.paths = write(directory, 'c1.bed', self.t1), write(directory, 'c2.bed', self.t2)

    def run(self, dev, how):
        got = dev.bed_compare(text1=self.t1, text2=self.t2) if how == 'text' else dev.bed_compare(path1=self.paths[0], path2=self.paths[1])
        assert got[-1] is None, got[-1]
        return got

    def decline(self, dev, monkeypatch):
        t2 = self.t2 + b'\n'
        self.declined = dict(n_bytes1=len(self.t1), n_bytes2=len(t2), decline_reason=_lib.CMP_DECLINE['memory'], decline_line=-1, decline_file=0)
        self.why, self.none = 'do not fit', (None, 0)
        return self.knob_decline(dev, monkeypatch, lambda: dev.bed_compare(text1=self.t1, text2=t2))


class Currents(Pipe):
    last_stats, releaser, knob = 'currents_compare_last_stats', 'currents_compare_release', 'MCALLER_CMP_DEVICE_BYTES'
    zeroed = ('n_lines1', 'n_lines2', 'n_keys', 'n_sites', 'n_values', 'n_out_bytes', 'n_bed_bytes', 'n_sig')
    KW = dict(depth=3, by='t', threshold=0.0)

    def __init__(self, directory):
        self.t1, self.t2 = K.seeded_pair(40, 3, 4, seed=53, c=2)
        self.paths = write(directory, 'n.diffs.6', self.t1), write(directory, 'k.diffs.6', self.t2)

    def run(self, dev, how):
        if how == 'text':
            got = dev.currents_compare(text1=self.t1, text2=self.t2, **self.KW)
        else:
            got = dev.currents_compare(path1=self.paths[0], path2=self.paths[1], **self.KW)
        assert got[-1] is None, got[-1]
        return got

    def decline(self, dev, monkeypatch):
        t2 = self.t2 + b'\n'
        self.declined = dict(n_bytes1=len(self.t1), n_bytes2=len(t2), decline_reason=_lib.CMP_DECLINE['memory'], decline_line=-1, decline_file=0)
        self.why, self.none = 'do not fit', (None, None, 0, 0)
        return self.knob_decline(dev, monkeypatch, lambda: dev.currents_compare(text1=self.t1, text2=t2, **self.KW))


class Clusters(Pipe):
    last_stats, releaser, knob = 'sites_cluster_last_stats', 'sites_cluster_release', 'MCALLER_CMP_DEVICE_BYTES'
    zeroed = ('n_lines', 'n_keys', 'n_candidates', 'n_sites', 'n_rows', 'n_out_bytes', 'n_bed_bytes')
    KW = dict(depth=3, mixed=True, min_minor=0.0, min_gap=0.0)

    def __init__(self, directory):
        self.text = CK.seeded_text(40, 3, 4, seed=53, c=2)
        self.path = write(directory, 'reads.diffs.6', self.text)

    def run(self, dev, how):
        got = dev.sites_cluster(text=self.text, **self.KW) if how == 'text' else dev.sites_cluster(path=self.path, **self.KW)
        assert got[-1] is None, got[-1]
        return got

    def decline(self, dev, monkeypatch):
        text = self.text + b'\n'
        self.declined = dict(n_bytes=len(text), decline_reason=_lib.CMP_DECLINE['memory'], decline_line=-1)
        self.why, self.none = 'do not fit', (None, None, 0, 0)
        return self.knob_decline(dev, monkeypatch, lambda: dev.sites_cluster(text=text, **self.KW))


class Xmfa(Pipe):
    last_stats, releaser = 'xmfa_map_last_stats', 'xmfa_map_release'
    zeroed = ('n_paired_blocks', 'n_columns', 'n_words', 'n_mapped')

    def __init__(self, directory):
        self.c = X.identity_case()
        self.path = write(directory, 'a.xmfa', self.c['xmfa'])

    def run(self, dev, how):
        src = dict(text=self.c['xmfa']) if how == 'text' else dict(path=self.path)
        g2, flip, why = dev.xmfa_map(n1=self.c['n1'], n2=self.c['n2'], seqs=self.c['seqs'], **src)
        assert why is None, why
        return g2.tobytes(), flip.tobytes()

    def decline(self, dev, monkeypatch):
        text, reason, line = X.bad_xmfas()['carriage return']
        self.declined = dict(n_bytes=len(text), n1=8, n2=8, decline_reason=_lib.CMP_DECLINE[reason], decline_line=line)
        self.why, self.none = 'declines', (None, None)
        return dev.xmfa_map(text=text, n1=8, n2=8)


class Motif(Pipe):
    last_stats, releaser, knob = 'motif_report_last_stats', 'motif_report_release', 'MCALLER_MOTIF_DEVICE_BYTES'
    zeroed = ('n_lines1', 'n_lines2', 'n_candidates', 'n_sites', 'n_control', 'n_selected', 'n_rows', 'n_out_bytes')

    def __init__(self, directory):
        contigs, bed, control, shapes = MS.placed_case()
        self.ref, self.bed, self.control = dict(contigs), MS.bed_text(bed, 'vo'), MS.bed_text(control)
        self.KW = dict(shapes=shapes, min_sites=1, min_fraction=0.0, keep_all=True)
        self.paths = write(directory, 'm.bed', self.bed), write(directory, 'm.control.bed', self.control)

    def run(self, dev, how):
        if how == 'text':
            got = dev.motif_report(self.ref, text=self.bed, control_text=self.control, **self.KW)
        else:
            got = dev.motif_report(self.ref, path=self.paths[0], control_path=self.paths[1], **self.KW)
        assert got[-1] is None and got[1] > 0, got[1:]
        return got

    def decline(self, dev, monkeypatch):
        bed = self.bed + b'\n'
        self.declined = dict(n_bytes1=len(bed), n_bytes2=len(self.control), decline_reason=_lib.MOTIF_DECLINE['memory'], decline_line=-1,
                             decline_file=0)
        self.why, self.none = 'do not fit', (None, 0)
        return self.knob_decline(dev, monkeypatch, lambda: dev.motif_report(self.ref, text=bed, control_text=self.control, **self.KW))


MAKERS = dict(bed=Bed, merge=Merge, train=Train, fastq=Fastq, eval=Eval, cmp=Cmp, currents=Currents, clusters=Clusters, xmfa=Xmfa, motif=Motif)


@pytest.fixture(scope='module')
def dev():
    from mcaller_amd.device import get_device
    return get_device()


@pytest.fixture(scope='module')
def pipes(tmp_path_factory):
    directory = tmp_path_factory.mktemp('frame')
    return {name: MAKERS[name](directory) for name in NAMES}


def counts(stats):
    """The stats without the milliseconds."""
    return {k: v for k, v in stats.items() if not k.startswith('ms_')}


@pytest.mark.parametrize('name', NAMES)
def test_release_and_reuse(dev, pipes, name):
    p = pipes[name]
    first = p.run(dev, 'text')
    p.release(dev)
    assert p.run(dev, 'path') == first, 'from a path, behind the release'
    assert p.run(dev, 'text') == first, 'from a text, behind the release'
    p.release(dev)
    p.release(dev)                                                     # nothing left to free
    assert p.run(dev, 'text') == first, 'behind two releases'


def test_release_on_a_context_that_never_ran(pipes):
    from mcaller_amd.device import Device
    fresh = Device()
    try:
        for name in NAMES:
            pipes[name].release(fresh)
            pipes[name].release(fresh)
            st = pipes[name].stats(fresh)
            assert all(v == 0 for k, v in st.items() if k != 'decline_line'), (name, st)
    finally:
        fresh.close()


@pytest.mark.parametrize('name', NAMES)
def test_a_decline_leaves_nothing_behind(dev, pipes, monkeypatch, name):
    p = pipes[name]
    first = p.run(dev, 'text')
    first_stats = counts(p.stats(dev))
    got = p.decline(dev, monkeypatch)
    st = p.stats(dev)
    assert tuple(got[:-1]) == p.none and got[-1] and p.why in got[-1], got
    assert {k: st[k] for k in p.declined} == p.declined, (name, st)
    assert (p.declined['decline_line'] < 0) == ('(line' not in got[-1]), got[-1]
    assert {k: st[k] for k in p.zeroed} == dict.fromkeys(p.zeroed, 0), (name, st)
    assert any(first_stats[k] for k in p.zeroed), (name, first_stats)  # (the good call had filled them)
    assert p.run(dev, 'text') == first
    assert counts(p.stats(dev)) == first_stats


def empty_calls(p):
    """{pipeline: (a call whose result is no byte at all, the result)}"""
    other = SG.empty_pairs()['no shared key']
    return {
        'bed': (lambda dev: dev.bed_summarise(text=b''), (b'', 0, None)),
        'bed, no site deep enough': (lambda dev: dev.bed_summarise(text=p['bed'].case.files['diffs'], min_depth=10 ** 6), (b'', 0, None)),
        'merge': (lambda dev: dev.merge_rows(text=b''), (b'', None)),
        'cmp': (lambda dev: dev.bed_compare(text1=b'', text2=b''), (b'', 0, None)),
        'cmp, no shared key': (lambda dev: dev.bed_compare(text1=p['cmp'].t1, text2=b''), (b'', 0, None)),
        'currents': (lambda dev: dev.currents_compare(text1=b'', text2=b'', depth=3), (b'', b'', 0, 0, None)),
        'currents, no shared key': (lambda dev: dev.currents_compare(text1=other[0], text2=other[1], depth=3), (b'', b'', 0, 0, None)),
        'clusters': (lambda dev: dev.sites_cluster(text=b'', depth=3), (b'', b'', 0, 0, None)),
        'clusters, no site deep enough': (lambda dev: dev.sites_cluster(text=p['clusters'].text, depth=100), (b'', b'', 0, 0, None)),
    }


def test_empty_outputs(dev, pipes):
    """No byte of output is b'' and no decline, whether the pipeline's pinned block is there (behind a larger result) or not
    (behind a release)."""
    for what, (call, want) in empty_calls(pipes).items():
        p = pipes[what.split(',')[0]]
        p.release(dev)
        assert call(dev) == want, (what, 'behind a release')
        p.run(dev, 'text')
        assert call(dev) == want, (what, 'behind a larger result')
        assert p.stats(dev)['decline_reason'] == 0, what


def test_the_evaluation_of_empty_texts(dev, pipes):
    """eval_calls has no empty result: its file holds the tables' frame whatever the texts hold.  Empty texts give that frame, the
    same bytes behind a release and behind a larger result."""
    p = pipes['eval']
    p.release(dev)
    blob, why = dev.eval_calls(text=b'', positions_text=b'', **p.KW)
    assert why is None and blob.startswith(b'#level\t') and blob.count(b'\n') == 1 + (2 + len(p.KW['depths'])) * 102
    assert len(p.run(dev, 'text')) > 0
    assert dev.eval_calls(text=b'', positions_text=b'', **p.KW) == (blob, None)


@pytest.mark.parametrize('name', ('eval', 'cmp', 'motif'))
def test_the_memory_knobs(dev, pipes, monkeypatch, name):
    """A knob of 1 byte declines with the memory reason; an empty one is no knob."""
    p = pipes[name]
    first = p.run(dev, 'text')
    got = p.decline(dev, monkeypatch)
    assert got[0] is None and 'do not fit' in got[-1] and p.stats(dev)['decline_reason'] == p.declined['decline_reason']
    monkeypatch.setenv(p.knob, '')
    assert p.run(dev, 'text') == first
    assert p.stats(dev)['decline_reason'] == 0
