"""The cases of tests/profile_cases.py hold what they claim, on the CPU and by the brute force alone: a case that stopped exercising
its edge (a genome re-drawn, a threshold moved) fails here instead of passing everywhere for nothing."""
import pytest

from tests import profile_cases as PC


@pytest.mark.parametrize('name', [c.name for c in PC.CASES])
def test_case_holds_its_claims(name):
    R = PC.expected(name)
    for what, claim in PC.BY_NAME[name].claims:
        assert claim(R), (name, what)
    assert R.n_rows == R.profile.count(b'\n') and len(R.nn_rows) == R.nn.count(b'\n')


def test_the_shapes_the_issue_names_are_all_there():
    names = ' '.join(c.name for c in PC.CASES)
    for piece in ('1_and_32_letters', 'window_edge', 'contig_ends', 'n_and_lower', 'overlapping', 'sharing_sites', '64_motifs', 'window_64_',
                  'window_65_', 'window_100_', 'without_a_site', 'identical_profiles', 'cuts_some', 'cuts_all') + \
            tuple('neighbours_of_%d_bins' % b for b in (1, 2, 63, 64, 65, 257)):
        assert piece in names, piece
    ks = {c.kw.get('neighbours') for c in PC.CASES}
    assert {1, 16} <= ks and any(c.kw.get('neighbours', 0) > len(c.contigs) - 1 for c in PC.CASES if c.kw.get('neighbours'))
    assert any(len(c.kw['motifs'].split(',')) == 64 for c in PC.CASES) and any(',' not in c.kw['motifs'] for c in PC.CASES)
