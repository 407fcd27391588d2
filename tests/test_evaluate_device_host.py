"""`python -m mcaller_amd.evaluate --device` as far as a machine without a GPU shows it: the flag parses, a decline is said and the
host statement makes the file, no GPU is an error and never a silent host run, and last_eval keeps its keys."""
import ctypes

import pytest

from tests import evaluate_cases as EC

KEYS = {'by', 'reason', 'n_rows', 'n_kept', 'n_unlabelled', 'n_not_m', 'n_sites', 'n_pos_sites', 'n_neg_sites'}


def _files(tmp_path):
    diffs, positions = EC.random_case(6)
    (tmp_path / 'a.diffs.6').write_bytes(diffs)
    (tmp_path / 'p.txt').write_bytes(positions)
    return diffs, positions, ['-f', str(tmp_path / 'a.diffs.6'), '-p', str(tmp_path / 'p.txt'), '-d', '3', '--depths', '1,2,5', '-o', str(tmp_path / 'o.tsv')]


def test_the_flag_parses_and_a_decline_runs_the_host_statement(tmp_path, monkeypatch, capsys):
    from mcaller_amd import evaluate as E
    diffs, positions, argv = _files(tmp_path)
    want = E.evaluate_calls(diffs, positions, 3, (1, 2, 5))
    asked = []

    def declines(d, p, min_depth, depths):
        asked.append((d, p, min_depth, list(depths)))
        E.last_eval.update(by=None, reason='the device evaluation declines: a test')
        return None
    monkeypatch.setattr(E, 'evaluate_calls_device', declines)
    out = E.main(['--device'] + argv)
    assert asked == [(argv[1], argv[3], 3, [1, 2, 5])] and open(out, 'rb').read() == want
    assert E.last_eval['by'] == 'host' and E.last_eval['reason'] == 'the device evaluation declines: a test' and set(E.last_eval) == KEYS
    assert 'declines: a test' in capsys.readouterr().err
    # served: the device's bytes are the file, the host statement does not run
    monkeypatch.setattr(E, 'evaluate_calls_device', lambda *a: E.last_eval.update(by='device', reason=None) or b'served\n')
    monkeypatch.setattr(E, 'evaluate_calls', lambda *a: 1 / 0)
    assert open(E.main(['--device'] + argv), 'rb').read() == b'served\n' and E.last_eval['by'] == 'device' and set(E.last_eval) == KEYS


def test_without_the_flag_no_device_is_asked(tmp_path, monkeypatch):
    from mcaller_amd import evaluate as E
    diffs, positions, argv = _files(tmp_path)
    monkeypatch.setattr(E, 'evaluate_calls_device', lambda *a: 1 / 0)
    assert open(E.main(argv), 'rb').read() == E.evaluate_calls(diffs, positions, 3, (1, 2, 5))
    assert E.last_eval['by'] == 'host' and E.last_eval['reason'] is None and set(E.last_eval) == KEYS


def test_no_gpu_means_an_error_not_the_host_statement(tmp_path):
    """Without a GPU `--device` fails loudly (this test only asserts behaviour on GPU-less machines)."""
    from mcaller_amd import _lib
    from mcaller_amd import evaluate as E
    L = _lib.lib()
    ctx = ctypes.c_void_p()
    if L.mc_ctx_create(0, ctypes.byref(ctx)) == 0:                     # a GPU is present: fine, clean up
        L.mc_ctx_destroy(ctx)
        return
    _, _, argv = _files(tmp_path)
    with pytest.raises(_lib.McError, match='no CPU fallback'):
        E.main(['--device'] + argv)
    assert not (tmp_path / 'o.tsv').exists()
