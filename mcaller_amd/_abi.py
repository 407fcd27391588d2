"""The C ABI as include/mcaller_hip.h states it, read for ctypes: integer constants, structs, prototypes.

The header is the one statement of the ABI; _lib.py takes its struct classes, its constants and every function's argtypes / restype
from here.  What the reader understands is the subset of C the header's first comment names; anything else stops the import
(AbiError) instead of leaving a struct or a function untyped.
"""
import ctypes as C
import os
import re

HEADER_PATH = os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), 'include', 'mcaller_hip.h')

SCALARS = {'char': C.c_char, 'int': C.c_int, 'float': C.c_float, 'double': C.c_double,
           'int8_t': C.c_int8, 'uint8_t': C.c_uint8, 'int16_t': C.c_int16, 'uint16_t': C.c_uint16,
           'int32_t': C.c_int32, 'uint32_t': C.c_uint32, 'int64_t': C.c_int64, 'uint64_t': C.c_uint64}

# [const] type, stars (each may carry a const), name, array sizes
_DECL = re.compile(r'(?:const\s+)?(\w+)\s*((?:\*\s*(?:const\b\s*)?)*)\s*\b(\w+)\s*((?:\[[^\][]+\]\s*)*)')
_RETURN = re.compile(r'(?:const\s+)?(\w+)\s*(\**)')
_HANDLE = re.compile(r'typedef\s+struct\s+(\w+)\s+(\w+)')
_STRUCT = re.compile(r'typedef\s+struct\s+(\w+)\s*\{(.*)\}\s*(\w+)', re.S)
_PROTOTYPE = re.compile(r'([^()]*?)\b(\w+)\s*\(([^()]*)\)')
_SIZE = re.compile(r'\[([^\][]+)\]')
_LITERAL = re.compile(r'(0[xX][0-9a-fA-F]+|\d+)[uUlL]*')
_CALL = re.compile(r'\b(mc_[a-z_0-9]+)\s*\(')          # a function's name where it is declared (tests/test_abi.py uses the same)


class AbiError(ImportError):
    """Something in the header that the reader does not understand."""


class Abi(object):
    """constants: {name: int}; structs: {C name: ctypes.Structure class}; handles: names of the opaque structs;
    functions: {name: (restype, [argtypes])}."""

    def __init__(self, text):
        self.constants, self.structs, self.handles, self.functions = {}, {}, set(), {}
        text = re.sub(r'/\*.*?\*/', ' ', text, flags=re.S)
        declared = set(_CALL.findall(text))
        text = re.sub(r'^[ \t]*#\s*ifdef\s+__cplusplus\s*$.*?^[ \t]*#\s*endif\s*$', '', text, flags=re.S | re.M)   # extern "C" { ... }
        text = re.sub(r'^[ \t]*#(.*)$', lambda m: self._directive(m.group(1)) or '', text, flags=re.M)
        depth, start = 0, 0
        for m in re.finditer(r'[{};]', text):                   # a statement ends at a ';' outside braces
            depth += (m.group() == '{') - (m.group() == '}')
            if m.group() == ';' and depth == 0:
                self._statement(text[start:m.start()].strip())
                start = m.end()
        if depth != 0 or text[start:].strip():
            raise AbiError('mcaller_hip.h: text that is no declaration: %r' % text[start:].strip()[:80])
        if declared != set(self.functions):
            raise AbiError('mcaller_hip.h: declarations the reader missed: %s' % sorted(declared ^ set(self.functions)))

    def value(self, expr):
        """An integer expression over literals (decimal, hex, u / l suffixes) and earlier constants."""
        def term(m):
            word = m.group(0)
            if word in self.constants:
                return str(self.constants[word])
            if _LITERAL.fullmatch(word):
                return str(int(word.rstrip('uUlL'), 0))
            raise AbiError('mcaller_hip.h: %r in the integer expression %r' % (word, expr))
        plain = re.sub(r'\w+', term, expr)
        if not plain.strip() or re.search(r'[^-\d\s+*()<>|&~]', plain):
            raise AbiError('mcaller_hip.h: not an integer expression: %r' % expr)
        try:
            return int(eval(plain, {'__builtins__': {}}))       # digits, + - * ( ) << >> | & ~ only
        except Exception:
            raise AbiError('mcaller_hip.h: not an integer expression: %r' % expr)

    def _directive(self, line):
        m = re.fullmatch(r'\s*define\s+(\w+)\s*(.*?)\s*', line)
        if m and m.group(2):
            self.constants[m.group(1)] = self.value(m.group(2))
        elif not m and not re.fullmatch(r'\s*(ifndef\s+\w+|endif|include\s*<stdint\.h>)\s*', line):
            raise AbiError('mcaller_hip.h: directive #%s' % line.strip())

    def _statement(self, s):
        m = _HANDLE.fullmatch(s)
        if m and m.group(1) == m.group(2):
            self.handles.add(m.group(1))
            return
        m = _STRUCT.fullmatch(s)
        if m and m.group(1) == m.group(3):
            fields = []
            for line in m.group(2).split(';'):
                if line.strip():
                    fields += [(name, self._ctype(base, stars, dims, line)) for name, base, stars, dims in self._declarators(line)]
            self.structs[m.group(1)] = type(m.group(1), (C.Structure,), {'_fields_': fields, '__doc__': '%s (include/mcaller_hip.h).' % m.group(1)})
            return
        m = _PROTOTYPE.fullmatch(s)
        r = m and _RETURN.fullmatch(m.group(1).strip())
        if not r:
            raise AbiError('mcaller_hip.h: neither a struct nor a prototype: %r' % s[:80])
        base, stars = r.group(1), len(r.group(2))
        restype = None if (base, stars) == ('void', 0) else C.c_char_p if (base, stars) == ('char', 1) else self._ctype(base, stars, [], s)
        argtypes = []
        if m.group(3).strip() != 'void':
            for p in m.group(3).split(','):
                (_, base, stars, dims), = self._declarators(p)
                if dims:                                        # (`double out3[3]`: a pointer)
                    stars, dims = stars + 1, []
                argtypes.append(C.POINTER(self.structs[base]) if stars == 1 and base in self.structs else self._ctype(base, stars, dims, s))
        self.functions[m.group(2)] = (restype, argtypes)

    def _declarators(self, text):
        """'int32_t n_labels, pad' / 'const char *const *names' / 'char shapes[A][B + 8]' -> [(name, base type, stars, [sizes])]"""
        parts = [p.strip() for p in text.split(',')]
        first = _DECL.fullmatch(parts[0])
        if not first:
            raise AbiError('mcaller_hip.h: cannot split the declaration %r' % text.strip())
        out = []
        for p in parts:
            m = _DECL.fullmatch(p if p is parts[0] else first.group(1) + ' ' + p)
            if not m:
                raise AbiError('mcaller_hip.h: cannot split the declaration %r' % text.strip())
            out.append((m.group(3), m.group(1), m.group(2).count('*'), [self.value(d) for d in _SIZE.findall(m.group(4))]))
        return out

    def _known(self, base, stars, where):
        if not (base in SCALARS or base in self.structs or (stars and (base == 'void' or base in self.handles))):
            raise AbiError('mcaller_hip.h: unknown type %r in %r' % (base + ' ' + '*' * stars, ' '.join(where.split())[:80]))

    def _ctype(self, base, stars, dims, where):
        """A field's type, or that of a parameter that is no pointer to a header struct: every pointer is a c_void_p."""
        self._known(base, stars, where)
        t = C.c_void_p if stars else SCALARS.get(base) or self.structs[base]
        for n in reversed(dims):
            if n < 1:
                raise AbiError('mcaller_hip.h: array size %d in %r' % (n, where.strip()))
            t = t * n
        return t

    def prefixed(self, prefix):
        """The constants whose names start with `prefix`, by the rest of the name in lower case (a decline table)."""
        return {name[len(prefix):].lower(): v for name, v in self.constants.items() if name.startswith(prefix)}

    def declare(self, library):
        """argtypes and restype of every declared function, set on a loaded CDLL."""
        for name, (restype, argtypes) in self.functions.items():
            fn = getattr(library, name)
            fn.restype, fn.argtypes = restype, argtypes


def load(path=HEADER_PATH):
    if not os.path.exists(path):
        raise ImportError('%s is missing: the ctypes binding reads the C ABI from it' % path)
    with open(path) as f:
        return Abi(f.read())
