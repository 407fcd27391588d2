"""The specs and the FASTA of the --motifs tests (uses nothing from mcaller_amd).

The FASTA has the shape of tests/test_gpu_refmark.py's -- 300 001 random bases with a lower-case stretch, `GATC`, `A`, a contig
with `M` and `N`, 5 000 bases over ACGTN -- plus, for every entry of the spec under test: contigs of length 0, 1, m - 1 and m; a
contig that ends in the first m - 1 letters of an occurrence followed by one that starts with the rest; and a contig with
occurrences planted so that each letter of the motif in turn falls on a 64-base edge and on a 32-bit word edge that is no
64-base edge, and with occurrences at positions 0 and L - m."""
import numpy as np

from tests import iupac_sites as S

M32 = 'GA' + 'N' * 13 + 'RY' + 'N' * 13 + 'TC'          # 32 letters
EIGHT = 'GANTC,GATC,CAAYNNNNNRTAC:3,CRAANNNNNNNTGC:3+4,TTAA:3,ACGT,RAY,' + M32 + ':2'
SPECS = (('GANTC', 'A'), ('AA', 'A'), ('NAN', 'A'), ('CAAYNNNNNRTAC:3', 'A'), ('CRAANNNNNNNTGC:3+4', 'A'), (M32, 'A'), (EIGHT, 'A'),
         ('A', 'A'), ('RGATCY', 'C'))

_common = None


def common_contigs():
    global _common
    if _common is None:
        rng = np.random.default_rng(11)
        seqs = {'big': ''.join(rng.choice(list('ACGT'), 300001)), 'tiny': 'GATC', 'empty_like': 'A',
                'with_m_and_n': 'ACGMTNNNGATCMMGATCGATC' * 40, 'mid': ''.join(rng.choice(list('ACGTN'), 5000))}
        seqs['big'] = seqs['big'][:700].lower() + seqs['big'][700:150000] + 'gatcGATCgAtC' + seqs['big'][150000:] + 'GATC'
        _common = list(seqs.items())
    return _common


def occurrence(motif, rng):
    return ''.join(rng.choice(list(S.SETS[ch])) for ch in motif)


def edge_contig(motif, rng):
    """Letter i of an occurrence at position 256 (i + 1) (a 64-base edge) and at 256 (i + 1) + 96 (a word edge that is no 64-base
    edge), for every i; occurrences at 0 and L - m."""
    m = len(motif)
    buf = list(rng.choice(list('ACGT'), 256 * (m + 2)))
    starts = [0, len(buf) - m]
    for i in range(m):
        starts += [256 * (i + 1) - i, 256 * (i + 1) + 96 - i]
    for q in starts:
        buf[q:q + m] = occurrence(motif, rng)
    return ''.join(buf), starts


def contigs_for(spec, base):
    """[(name, sequence)]: the common contigs, then the spec's own."""
    rng = np.random.default_rng(len(spec) + 1000 * ord(base))
    out = list(common_contigs()) + [('len0', ''), ('len1', base)]
    for k, (motif, _) in enumerate(S.entries_of(spec, base)):
        m = len(motif)
        hit = occurrence(motif, rng)
        out += [('m%d_minus1' % k, hit[:m - 1]), ('m%d_exact' % k, hit),
                ('m%d_head' % k, ''.join(rng.choice(list('ACGT'), 70)) + hit[:m - 1]),
                ('m%d_tail' % k, hit[m - 1:] + ''.join(rng.choice(list('ACGT'), 70))),
                ('m%d_edges' % k, edge_contig(motif, rng)[0])]
    return out


def write_fasta(path, contigs):
    with open(path, 'w') as fh:
        for name, seq in contigs:
            fh.write('>%s extra words\n' % name + '\n'.join(seq[i:i + 60] for i in range(0, len(seq), 60)) + '\n')
