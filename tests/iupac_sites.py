"""The rule of --motifs restated by brute force in NumPy (uses nothing from mcaller_amd): for every start all letters lie in their
sets, and the called offsets are OR-ed.  A sequence letter other than A, C, G, T matches nothing."""
import numpy as np

SETS = {'A': 'A', 'C': 'C', 'G': 'G', 'T': 'T', 'R': 'AG', 'Y': 'CT', 'S': 'CG', 'W': 'AT', 'K': 'GT', 'M': 'AC',
        'B': 'CGT', 'D': 'AGT', 'H': 'ACT', 'V': 'ACG', 'N': 'ACGT'}
COMP = {'A': 'T', 'C': 'G', 'G': 'C', 'T': 'A'}
LETTER_OF = {frozenset(v): k for k, v in SETS.items()}


def entries_of(spec, base):
    """'MOTIF[:I+J],...' -> [(motif, [0-based called offsets])]; without indices: every letter equal to base."""
    out = []
    for entry in spec.upper().split(','):
        motif, _, idx = entry.partition(':')
        out.append((motif, [int(t) - 1 for t in idx.split('+')] if idx else [i for i, ch in enumerate(motif) if ch == base]))
    return out


def reverse_complement(motif, offsets):
    rc = ''.join(LETTER_OF[frozenset(COMP[b] for b in SETS[ch])] for ch in reversed(motif))
    return rc, [len(motif) - 1 - j for j in offsets]


def sites(seq, entries):
    """bool[len(seq)]: the positions the entries mark on the upper-cased sequence (one strand: the motifs as given)."""
    s = np.frombuffer(seq.upper().encode('latin1'), dtype=np.uint8)
    marked = np.zeros(len(s), dtype=bool)
    for motif, offsets in entries:
        m = len(motif)
        if m > len(s):
            continue
        starts = np.ones(len(s) - m + 1, dtype=bool)
        for i, ch in enumerate(motif):
            starts &= np.isin(s[i:len(s) - m + 1 + i], np.frombuffer(SETS[ch].encode(), dtype=np.uint8))
        for j in offsets:
            marked[j:len(s) - m + 1 + j] |= starts
    return marked


def strands(seq, spec, base):
    """(marked '+', marked '-') for a spec: the '-' strand looks for the reverse complements, offsets mirrored."""
    entries = entries_of(spec, base)
    return sites(seq, entries), sites(seq, [reverse_complement(m, o) for m, o in entries])


def strings(seq, spec, base):
    """(meth_fwd, meth_rev): the upper-cased sequence with 'M' at the marked positions (a literal 'M' stays)."""
    out = []
    for marked in strands(seq, spec, base):
        b = np.frombuffer(seq.upper().encode('latin1'), dtype=np.uint8).copy()
        b[marked] = ord('M')
        out.append(b.tobytes().decode('latin1'))
    return out[0], out[1]
