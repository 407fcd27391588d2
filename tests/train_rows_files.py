"""Generated `.diffs.<k>.train` texts for the device reader's tests (tests/test_gpu_train_rows.py), seeded; and the comparison of
a device result with tsv2matrix's, floats by their bits."""
import random

LABELS = ('m6A', 'A', 'unsure')
SIZES = (1, 2, 255, 256, 257, 513, 3001)       # lines: below, at and above a 256-line workgroup, a third one, a second scan block of 1024 counts


def _number(rng):
    kind = rng.random()
    if kind < 0.06:
        return repr(rng.choice((1e-05, -2.5e-06, 3.0000000000000004e-05, 1e-07)))
    n = rng.randint(1, 6)
    x = sum(rng.randint(-150000, 150000) / 1e4 for _ in range(n)) / n
    return repr(x if abs(x) >= 1e-7 else 0.25)   # (a sum that should be zero leaves a residue like 3.5e-16: outside mc_decimal.h's exponents, a decline)


def _context(rng, length):
    bases = [rng.choice('ACGT') for _ in range(length)]
    bases[length // 2] = rng.choice('MAT')
    bases[length // 2 + 1] = rng.choice('ACGTM')
    return ''.join(bases)


def random_file(seed, n_lines):
    """-> (text: bytes, what it holds: dict).  What varies with the seed: the trailing newline, 1-3 labels, a second label first
    seen on a left-out row, a label with only left-out rows, the kinds of left-out rows (5 features, a literal 0, garbage), 7- and
    8-field rows, 6 or 7 features (uniform in a file), one line with a 40 KB read name, contexts of 11 and 5 characters, labels
    with a trailing blank."""
    rng = random.Random(seed * 7919 + n_lines)
    n_labels = 1 + seed % 3
    nf = 6 + (seed // 3) % 2
    second_on_left_out = n_labels >= 2 and (seed // 2) % 2 == 0
    only_left_out = LABELS[n_labels - 1] if n_labels >= 2 and seed % 4 == 1 else None
    long_line = rng.randrange(n_lines) if seed % 2 == 0 else -1
    seen = set()
    lines = []
    for i in range(n_lines):
        label = LABELS[0] if i == 0 else rng.choice(LABELS[:n_labels])
        left_out = rng.random() < 0.25 or label == only_left_out
        if second_on_left_out and label != LABELS[0] and LABELS[1] not in seen:
            label, left_out = LABELS[1], True
        seen.add(label)
        if left_out:
            kind = rng.randrange(4)
            if kind == 0:
                feats = [_number(rng) for _ in range(5)]
            elif kind == 1:
                feats = [_number(rng) for _ in range(nf)]
                feats[rng.randrange(nf)] = '0'
            elif kind == 2:
                feats = ['abc', '0', '1e', ' 1', 'nan', '--', '1_0'][:rng.randint(2, 7)] + ['0']
            else:
                feats = ['x', '', 'inf']
        else:
            feats = [_number(rng) for _ in range(nf)]
        name = 'read%d_Basecall_2D_template' % rng.randrange(10 ** 6)
        if i == long_line:
            name = 'R' * 40000 + name
        context = _context(rng, 11 if rng.random() < 0.7 else 5)
        shown = label + (' ' if rng.random() < 0.2 else '')
        fields = ['ecoli', name, str(rng.randrange(1, 10 ** 7)), context, ','.join(feats), rng.choice('+-'), shown]
        if rng.random() < 0.4:
            fields.append(rng.choice(('0.93', ' 0.5 ', '1.0')))
        lines.append('\t'.join(fields))
    text = '\n'.join(lines) + ('\n' if seed % 4 < 2 else '')
    return text.encode('ascii'), dict(n_labels=len(seen), nf=nf, long_line=long_line, only_left_out=only_left_out)


def plain(signals, contexts):
    """Both dicts as nested lists in key order, floats as their hex (so that -0.0 and 0.0 differ), contexts as str: what a device
    result and a host result are compared by."""
    def rows_of(rows):
        rows = rows.tolist() if hasattr(rows, 'tolist') else rows
        return [[float(v).hex() for v in row] for row in rows]

    def ctx_of(rows):
        rows = rows.tolist() if hasattr(rows, 'tolist') else rows
        return [c.decode('ascii') if isinstance(c, bytes) else c for c in rows]
    sig = [(key, [(label, rows_of(rows)) for label, rows in by_label.items()]) for key, by_label in signals.items()]
    ctx = [(key, [(label, ctx_of(rows)) for label, rows in by_label.items()]) for key, by_label in contexts.items()]
    return sig, ctx
