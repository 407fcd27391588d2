"""The C-ABI library loads on a machine without a GPU and exports every symbol include/mcaller_hip.h declares."""
import ctypes
import os
import re

from tests import helpers as H


def test_library_exports_every_declared_symbol():
    from mcaller_amd import _lib
    header = open(os.path.join(H.REPO, 'include', 'mcaller_hip.h')).read()
    header = re.sub(r'/\*.*?\*/', '', header, flags=re.S)
    names = sorted(set(re.findall(r'\b(mc_[a-z_0-9]+)\s*\(', header)))
    assert len(names) >= 15
    L = ctypes.CDLL(_lib.LIB_PATH)
    missing = [n for n in names if not hasattr(L, n)]
    assert not missing, missing
    _lib.lib()
    assert b'mcaller_hip' in _lib.lib().mc_version()


def test_no_gpu_means_error_not_fallback():
    """Without a GPU the device entry points fail loudly (this test only asserts behaviour on GPU-less machines)."""
    from mcaller_amd import _lib
    L = _lib.lib()
    ctx = ctypes.c_void_p()
    rc = L.mc_ctx_create(0, ctypes.byref(ctx))
    if rc == 0:                       # a GPU is present: fine, clean up
        L.mc_ctx_destroy(ctx)
        return
    assert rc < 0 and b'no CPU fallback' in L.mc_last_error()


def test_product_never_imports_the_oracle():
    for root, _, files in os.walk(os.path.join(H.REPO, 'mcaller_amd')):
        for f in files:
            if f.endswith('.py'):
                src = open(os.path.join(root, f)).read()
                assert 'oracle' not in re.sub(r'#.*', '', src).replace('"""', ''), f


def _declared_names():
    """The function names of the header, as test_library_exports_every_declared_symbol finds them."""
    header = re.sub(r'/\*.*?\*/', '', open(os.path.join(H.REPO, 'include', 'mcaller_hip.h')).read(), flags=re.S)
    return header, set(re.findall(r'\b(mc_[a-z_0-9]+)\s*\(', header))


def test_every_library_call_from_python_has_argtypes():
    """A ctypes call without argtypes passes a Python int as a C int: a byte offset beyond 2^31 arrives cut (mc_eventalign_read_cuts_at
    did, for a day).  Every mc_* function the package calls is typed on the loaded library, with as many arguments as the header's
    prototype has parameters."""
    import glob
    from mcaller_amd import _lib
    here = os.path.join(H.REPO, 'mcaller_amd')
    src = ''.join(open(f).read() for f in glob.glob(os.path.join(here, '*.py')))
    called = set(re.findall(r'\b(?:lib\(\)|L|_lib\.lib\(\))\.(mc_[a-z0-9_]+)\(', src))
    assert len(called) >= 100
    header, _ = _declared_names()
    for name in sorted(called):
        params = re.search(r'\b%s\s*\(([^()]*)\)' % name, header).group(1).strip()
        n_params = 0 if params == 'void' else params.count(',') + 1
        argtypes = getattr(_lib.lib(), name).argtypes
        assert argtypes is not None and len(argtypes) == n_params, (name, argtypes, n_params)


def test_the_reader_misses_no_declaration_and_refuses_what_it_does_not_know():
    import pytest
    from mcaller_amd import _abi, _lib
    _, names = _declared_names()
    assert set(_lib.ABI.functions) == names and len(names) >= 140
    ok = '#define MC_N 4\ntypedef struct mc_h mc_h;\ntypedef struct mc_s { int32_t a[MC_N + 1], b; const mc_h *h; } mc_s;\n' \
         'int64_t mc_f(mc_h *h, const mc_s *s, const char *text, double out2[2]);\nconst char *mc_g(void);\nvoid mc_v(float x);\n'
    abi = _abi.Abi(ok)
    s = abi.structs['mc_s']
    assert abi.constants == {'MC_N': 4} and ctypes.sizeof(s) == 32 and [f[0] for f in s._fields_] == ['a', 'b', 'h']
    assert abi.functions == {'mc_f': (ctypes.c_int64, [ctypes.c_void_p, ctypes.POINTER(s), ctypes.c_void_p, ctypes.c_void_p]),
                             'mc_g': (ctypes.c_char_p, []), 'mc_v': (None, [ctypes.c_float])}
    for bad in ('int mc_f(size_t n);',                               # an unknown type name
                'typedef struct mc_s { long double x; } mc_s;',      # a field it cannot split
                'typedef struct mc_s { int32_t a[MC_M]; } mc_s;',    # an array size that is no integer
                'typedef struct mc_s { int32_t a : 3; } mc_s;',
                'int mc_f(int (*callback)(int));',
                'mc_unknown *mc_f(void);',
                '#define MC_TWICE(x) (2 * (x))\n',
                'typedef int32_t mc_int;',
                'int mc_f(int a) { return a; }'):
        with pytest.raises(_abi.AbiError):
            _abi.Abi(ok + bad)
    with pytest.raises(ImportError, match='no_such_header.h'):
        _abi.load(os.path.join(H.REPO, 'include', 'no_such_header.h'))


def test_struct_layouts_and_constants_are_the_compilers(tmp_path):
    """Every struct the binding derives from the header has the size, the field offsets and the field sizes gcc gives it, and every
    constant its value: a program that includes the header prints them."""
    import subprocess
    from mcaller_amd import _lib
    abi = _lib.ABI
    assert len(abi.structs) >= 24 and len(abi.constants) >= 100
    lines = ['#include <stdio.h>', '#include <stddef.h>', '#include "mcaller_hip.h"', 'int main(void) {']
    expected = []
    for name, cls in sorted(abi.structs.items()):
        lines.append('printf("%s %%zu\\n", sizeof(%s));' % (name, name))
        expected.append('%s %d' % (name, ctypes.sizeof(cls)))
        for field, _ in cls._fields_:
            lines.append('printf("%s.%s %%zu %%zu\\n", offsetof(%s, %s), sizeof(((%s *)0)->%s));' % (name, field, name, field, name, field))
            expected.append('%s.%s %d %d' % (name, field, getattr(cls, field).offset, getattr(cls, field).size))
    for name, v in sorted(abi.constants.items()):
        lines.append('printf("%s %%lld\\n", (long long)(%s));' % (name, name))
        expected.append('%s %d' % (name, v))
    lines += ['return 0;', '}']
    src, exe = tmp_path / 'layout.c', tmp_path / 'layout'
    src.write_text('\n'.join(lines) + '\n')
    subprocess.check_call(['gcc', '-std=c11', '-Wall', '-Werror', '-I', os.path.join(H.REPO, 'include'), '-o', str(exe), str(src)])
    got = subprocess.check_output([str(exe)]).decode().splitlines()
    assert got == expected, [(g, e) for g, e in zip(got, expected) if g != e][:10]
    # what _lib.py hands on under its own names is the header's
    k = abi.constants
    assert (_lib.MC_MAX_K, _lib.E_NO_FREE_SLOT, _lib.TrainRowsView.MAX_LABELS) == (k['MC_MAX_K'], k['MC_E_NO_FREE_SLOT'], k['MC_TRAINROWS_MAX_LABELS'])
    assert (_lib.F_KMER_EQ, _lib.F_MODEL_N, _lib.F_SEG_START, _lib.F_NAME_START) == (k['MC_F_KMER_EQ'], k['MC_F_MODEL_N'], k['MC_F_SEG_START'], k['MC_F_NAME_START'])
    assert (_lib.I_EMPTY_MASK, _lib.I_REV, _lib.I_TOO_MANY, _lib.I_MULTI, _lib.I_EDGE, _lib.I_NEXT_SHIFT) == \
        (k['MC_I_EMPTY_MASK'], k['MC_I_REV'], k['MC_I_TOO_MANY'], k['MC_I_MULTI'], k['MC_I_EDGE'], k['MC_I_NEXT_SHIFT'])
    for table, prefix in ((_lib.MOTIF_DECLINE, 'MC_MOTIF_DECLINE_'), (_lib.CMP_DECLINE, 'MC_CMP_DECLINE_'),
                          (_lib.FASTQ_DECLINE, 'MC_FASTQ_DECLINE_'), (_lib.MERGE_DECLINE, 'MC_MERGE_DECLINE_')):
        assert len(table) >= 6 and all(k[prefix + name.upper()] == v for name, v in table.items())
    assert _lib.CMP_DECLINE['tie'] == 16 and _lib.MERGE_DECLINE['memory'] == 6 and _lib.I_TOO_MANY == 0x200 and _lib.E_NO_FREE_SLOT == -16


def test_every_kernel_of_the_pass_path_is_in_the_hashed_sources():
    """bench.KERNEL_SOURCES is what ties a PMC traffic figure to the kernels it was measured on: every file it names exists, and every
    file under csrc/ that defines a kernel is on it, or is one of the --train fit units (which no pass runs)."""
    import bench
    fits = {'mc_train.hip', 'mc_forest_fit.hip', 'mc_svm_fit.hip', 'mc_simple_fit.hip', 'mc_fit.h'}
    missing = [f for f in bench.KERNEL_SOURCES if not os.path.isfile(os.path.join(H.REPO, f))]
    assert not missing, missing
    hashed = {os.path.basename(f) for f in bench.KERNEL_SOURCES}
    csrc = os.path.join(H.REPO, 'mcaller_amd', 'csrc')
    with_kernels = {f for f in os.listdir(csrc) if os.path.isfile(os.path.join(csrc, f)) and '__global__' in open(os.path.join(csrc, f), errors='replace').read()}
    assert len(with_kernels) >= 10
    assert with_kernels <= hashed | fits, sorted(with_kernels - hashed - fits)
