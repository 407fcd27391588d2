"""The feed the four file pipelines share (mcaller_amd/csrc/mc_textfeed.h): a file read in blocks through the context's two pinned
stages gives what its text gives, whatever the block size -- MCALLER_TEXT_STAGE_BYTES sets it, down to 256 bytes, so texts of a few KB
(tests/textfeed_cases.py) go through every path of the read loop: one block, a last block of one byte, the first reuse of a stage
behind its event, lines across every block edge, several files in one call, the merge's output leaving through the same stages."""
import os
import subprocess
import sys

import pytest

from tests import helpers as H
from tests import textfeed_cases as C

pytestmark = pytest.mark.gpu


@pytest.fixture(scope='module')
def dev():
    from mcaller_amd.device import get_device
    return get_device()


@pytest.fixture(scope='module')
def cases(dev, tmp_path_factory):
    """{pipeline: case}, with every case's text= result (made once, the knob unset) -- which is the host function's."""
    assert C.KNOB not in os.environ
    made = C.cases(tmp_path_factory.mktemp('textfeed'))
    for case in made.values():
        case.twin = case.run_text(dev)
        assert case.twin == case.run_host(), case.name
    return made


@pytest.mark.parametrize('which', C.BLOCKS)
@pytest.mark.parametrize('name', C.PIPELINES)
def test_a_file_in_blocks_of_every_size_equals_its_text(dev, cases, monkeypatch, name, which):
    case = cases[name]
    k = C.block_size(which, case.n)
    assert 256 <= k <= case.n and (which == '256' or k > 256)
    monkeypatch.setenv(C.KNOB, str(k))
    assert case.run_file(dev) == case.twin, (name, k)
    case.check_stats(dev)


def test_bed_takes_three_files_through_the_feed_in_one_call(dev, cases, monkeypatch):
    case = cases['bed']
    assert all(len(blob) > 2 * 256 for blob in case.files.values())
    monkeypatch.setenv(C.KNOB, '256')
    assert case.run_file(dev) == case.twin and case.twin[1] > 0
    case.check_stats(dev)


def _entry_points(dev, cases, tmp_path):
    """{entry point: (its sources' names, which of them may be null, call(**sources) -> (rc, status) with every other argument
    sound, works() -> the pipeline's small case, from files, gives the host's result on the context)}.  The bed summary, the training
    rows and the FASTQ qualities run their case of tests/textfeed_cases.py; the comparison, the alignment map and the motif finder
    have none there and run the smallest case of their own tests."""
    import ctypes
    import numpy as np
    from mcaller_amd import _lib, compare_genomes as CG, find_motifs as FM
    from tests import gpu_compare_cases as GC, motif_sites as MS, xmfa_cases as X
    L, ctx = _lib.lib(), dev._ctx
    by = ctypes.byref

    def call(name, *args):
        status = ctypes.c_int32(77)
        return getattr(L, name)(ctx, *args, by(status)), status.value

    out, n_out, n, view = ctypes.c_void_p(), ctypes.c_int64(), ctypes.c_int64(), _lib.TrainRowsView()
    fq_view, ref, params = _lib.FastqQualityView(), _lib.RefView(), _lib.MotifParams()
    prm = _lib.BedParams(1, 0.5, 0, 0, 0, 0)

    def case_works(name):
        return lambda: cases[name].run_file(dev) == cases[name].twin

    t1, t2 = GC.key_pair()
    (tmp_path / 'a.bed').write_bytes(t1)
    (tmp_path / 'b.bed').write_bytes(t2)
    cmp_want = CG.compare_rows(str(tmp_path / 'a.bed'), str(tmp_path / 'b.bed'))

    def compare_works():
        return dev.bed_compare(path1=str(tmp_path / 'a.bed'), path2=str(tmp_path / 'b.bed')) == cmp_want + (None,)

    xc = X.identity_case()
    (tmp_path / 'x.xmfa').write_bytes(xc['xmfa'])
    want_g2, want_flip = CG.xmfa_map(str(tmp_path / 'x.xmfa'), xc['n1'], xc['seqs'], xc['n2'])

    def xmfa_works():
        g2, flip, why = dev.xmfa_map(path=str(tmp_path / 'x.xmfa'), n1=xc['n1'], n2=xc['n2'], seqs=xc['seqs'])
        dev.xmfa_map_release()
        return why is None and np.array_equal(g2, want_g2) and np.array_equal(flip, want_flip)

    contigs, bed, control, shapes = MS.placed_case()
    m_bed, m_ctl, m_kw = MS.bed_text(bed, 'vo'), MS.bed_text(control), dict(min_sites=1, min_fraction=0.0, keep_all=True)
    for key, blob in (('ref.fasta', MS.fasta(contigs)), ('sites.bed', m_bed), ('control.bed', m_ctl)):
        (tmp_path / key).write_bytes(blob)
    m_n = FM.find_motifs(str(tmp_path / 'ref.fasta'), str(tmp_path / 'sites.bed'), str(tmp_path / 'control.bed'), out=str(tmp_path / 'host.tsv'),
                         shapes=shapes, **m_kw)
    m_want = ((tmp_path / 'host.tsv').read_bytes(), m_n, None)
    m_ref = FM.read_reference(str(tmp_path / 'ref.fasta'))

    def motif_works():
        return dev.motif_report(m_ref, path=str(tmp_path / 'sites.bed'), control_path=str(tmp_path / 'control.bed'), shapes=FM.parse_shapes(shapes),
                                **m_kw) == m_want

    return {
        'mc_bed_summarise': (('src', 'positions', 'fasta'), ('positions', 'fasta'), lambda src, positions, fasta: call(
            'mc_bed_summarise', src, positions, fasta, by(prm), by(out), by(n_out), by(n)), case_works('bed')),
        'mc_motif_report': (('bed', 'control'), ('control',), lambda bed, control: call(
            'mc_motif_report', by(ref), bed, control, by(params), 0, 0, by(out), by(n_out), by(n)), motif_works),
        'mc_bed_compare': (('bed1', 'bed2'), (), lambda bed1, bed2: call(
            'mc_bed_compare', bed1, bed2, None, None, by(out), by(n_out), by(n), None), compare_works),
        'mc_xmfa_map': (('src',), (), lambda src: call('mc_xmfa_map', src, 1, 2, 8, 8, None), xmfa_works),
        'mc_train_rows': (('src',), (), lambda src: call('mc_train_rows', src, b'', 0, by(view)), case_works('train')),
        'mc_fastq_quality': (('src',), (), lambda src: call('mc_fastq_quality', src, by(fq_view)), case_works('fastq')),
    }


def test_every_entry_point_refuses_a_source_that_is_none_and_runs_its_pipeline_afterwards(dev, cases, tmp_path):
    """What mc_textfeed.h's text_source checks, for every source of the six entry points that take mc_text_source: no kernel runs in
    a refusal, the error names the entry point, and the context does the pipeline's small case behind every one of them."""
    import ctypes
    from mcaller_amd import _lib
    L = _lib.lib()
    text = b'x\ty\n'                                                   # (a sound source beside the one on trial; never reached)
    keep = ctypes.c_char_p(text)
    at = ctypes.cast(keep, ctypes.c_void_p)
    folder = ctypes.cast(ctypes.c_char_p(os.fsencode(str(tmp_path))), ctypes.c_void_p)
    sound = _lib.TextSource(at, None, len(text))
    refused = dict(both=_lib.TextSource(at, folder, len(text)), neither=_lib.TextSource(None, None, 1), negative=_lib.TextSource(at, None, -1))
    points = _entry_points(dev, cases, tmp_path)
    assert len(points) == 6
    for name, (sources, optional, call, works) in points.items():
        for on_trial in sources:
            trials = dict(refused, folder=_lib.TextSource(None, folder, 0))
            if on_trial not in optional:
                trials['null'] = None
            for what, source in trials.items():
                args = {s: ctypes.byref(sound) for s in sources}
                args[on_trial] = None if source is None else ctypes.byref(source)
                rc, status = call(**args)
                said = L.mc_last_error()
                if what == 'folder':
                    assert rc < 0 and b'is not a readable file' in said and status != 1, (name, on_trial, rc, said, status)
                else:
                    assert rc == -12, (name, on_trial, what, rc, said)
                assert name.encode() in said, (name, on_trial, what, said)
                assert works(), (name, on_trial, what)
    # mc_bed_params.site_stats: --gff --vo declines without it and is made with it
    by = ctypes.byref
    diffs = cases['bed'].files['diffs']
    src = _lib.TextSource(ctypes.cast(ctypes.c_char_p(diffs), ctypes.c_void_p), None, len(diffs))
    seen = []
    for site_stats in (0, 1):
        prm = _lib.BedParams(1, 0.5, 0, 1, 1, site_stats)
        out, n_out, n, status = ctypes.c_void_p(), ctypes.c_int64(), ctypes.c_int64(), ctypes.c_int32(77)
        assert L.mc_bed_summarise(dev._ctx, by(src), None, None, by(prm), by(out), by(n_out), by(n), by(status)) == 0
        seen.append((status.value, dev.bed_last_stats()['decline_reason'], n_out.value > 0 and n.value > 0))
    assert seen == [(1, _lib.ABI.constants['MC_BED_DECLINE_OPTIONS'], False), (0, 0, True)], seen


SIZES = (0, 45, 255, 256, 257, 700)          # an empty part, one line, file ends beside and on a block edge, three blocks


@pytest.mark.parametrize('order', ['in_order', 'reversed'])
def test_merge_part_files_on_and_beside_the_block_edges(dev, tmp_path, monkeypatch, order):
    """Six part files through 256-byte blocks: the block count -- which stage a block goes through, and whether it waits -- runs
    across the files, and the output (more than two blocks) leaves through the same stages."""
    parts = [C.sized_part(size, seed) for seed, size in enumerate(SIZES)]
    assert parts[1].count(b'\n') == 1
    if order == 'reversed':
        parts.reverse()
    case = C.Merge(tmp_path, parts, name=order)
    want = case.run_host()
    assert len(want) > 2 * 256
    monkeypatch.setenv(C.KNOB, '256')
    assert case.run_text(dev) == want
    assert case.run_file(dev) == want
    case.check_stats(dev)


@pytest.mark.parametrize('cut', ['newline_alone_in_the_last_block', 'last_byte_alone_in_the_last_block'])
def test_merge_part_without_its_last_newline_at_a_block_edge(dev, tmp_path, monkeypatch, cut):
    """The part of 257 bytes without the newline that was the only byte of its last block; and the part of 256 bytes with one byte
    more, which then is: the decline names the file and the line it names with the knob unset."""
    from mcaller_amd import _lib
    parts = [C.sized_part(size, seed) for seed, size in enumerate(SIZES)]
    at = SIZES.index(257) if cut == 'newline_alone_in_the_last_block' else SIZES.index(256)
    parts[at] = parts[at][:-1] if at == SIZES.index(257) else parts[at] + b'x'
    assert len(parts[at]) in (256, 257) and not parts[at].endswith(b'\n')
    case = C.Merge(tmp_path, parts, name='cut')
    seen = []
    for knob in (None, '256'):
        if knob:
            monkeypatch.setenv(C.KNOB, knob)
        why = case.run_file(dev, want_decline=True)
        st = case.stats(dev)
        seen.append((why, st['decline_reason'], st['decline_line'], st['decline_file']))
    assert seen[0] == seen[1], seen
    assert seen[0][1] == _lib.MERGE_DECLINE['no_newline'] and seen[0][3] == at
    assert seen[0][2] == b''.join(parts[:at + 1]).count(b'\n') and '(line %d)' % (seen[0][2] + 1) in seen[0][0]


def _declining(name, tmp_path):
    """-> (run, stats): one text per pipeline that its own tests see declined, long enough for more than three blocks of 256 bytes."""
    from mcaller_amd.device import get_device
    dev = get_device()
    if name == 'bed':
        from tests import bedpos_files as P
        text, ptext, opts, _, _ = P.decline_cases()['positions_high_byte']
        files = dict(diffs=text, positions=ptext)
        run = lambda p: dev.bed_summarise(path=p['diffs'], positions_path=p['positions'], **opts)[2]       # noqa: E731
        stats = dev.bed_last_stats
    elif name == 'merge':
        from tests import merge_files as MF
        rows = MF.name_rows(MF.CLI_HOST_NAMES)
        files = dict(part=b''.join(rows[:20]) + b'chr1\tab\r\t3\n' + rows[20])
        run = lambda p: dev.merge_rows(paths=[p['part']], out_path=str(tmp_path / 'declined.merged'))[1]    # noqa: E731
        stats = dev.merge_rows_last_stats
    elif name == 'train':
        from tests.test_gpu_train_rows import GOOD
        files = dict(train=((GOOD + '\n') * 16 + GOOD.replace('\tr\t', '\tréad\t') + '\n').encode('utf-8'))
        run = lambda p: dev.training_rows(path=p['train'], pairs=C.Train._pairs())[3]                      # noqa: E731
        stats = dev.training_rows_last_stats
    else:
        from tests import fastq_cases as F
        import numpy as np
        files = dict(fastq=F.random_fastq(np.random.default_rng(3), 4) + b'@r\xe9\nAC\n+\nII\n')
        run = lambda p: dev.fastq_qualities(path=p['fastq'])[2]                                            # noqa: E731
        stats = dev.fastq_qualities_last_stats
    assert len(next(iter(files.values()))) > 3 * 256
    paths = {}
    for key, blob in files.items():
        paths[key] = str(tmp_path / key)
        with open(paths[key], 'wb') as fh:
            fh.write(blob)
    return (lambda: run(paths)), stats


@pytest.mark.parametrize('name', C.PIPELINES)
def test_a_decline_is_the_same_in_small_blocks(tmp_path, monkeypatch, name):
    run, stats = _declining(name, tmp_path)
    seen = []
    for knob in (None, '256'):
        if knob:
            monkeypatch.setenv(C.KNOB, knob)
        why = run()
        st = stats()
        seen.append((why, st['decline_reason'], st['decline_line']))
    assert seen[0] == seen[1], seen
    assert 'declines' in seen[0][0] and seen[0][1] > 0 and seen[0][2] > 0 and '(line %d)' % (seen[0][2] + 1) in seen[0][0]


def test_every_pipeline_in_turn_on_one_context(dev, tmp_path, monkeypatch):
    monkeypatch.setenv(C.KNOB, '256')
    C.mixed(dev, tmp_path)


def test_every_pipeline_in_turn_with_poisoned_allocations(tmp_path):
    env = dict(os.environ, MCALLER_POISON='1', PYTHONPATH=H.REPO)
    env[C.KNOB] = '256'
    done = subprocess.run([sys.executable, os.path.join(H.REPO, 'tests', '_textfeed_mixed_worker.py'), str(tmp_path)], env=env,
                          stdout=subprocess.PIPE, stderr=subprocess.STDOUT, timeout=300)
    assert done.returncode == 0 and b'mixed ok' in done.stdout, done.stdout.decode('utf-8', 'replace')[-2000:]
