"""The C-ABI library loads and exports every symbol include/pyglm_hip.h declares (no compute calls: no GPU needed)."""
import ctypes
import os
import re

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def declared_symbols():
    text = open(os.path.join(ROOT, "include", "pyglm_hip.h")).read()
    text = re.sub(r"/\*.*?\*/", "", text, flags=re.S)
    return sorted(set(re.findall(r"\b(pgl_[a-z0-9_]+)\s*\(", text)))


def test_header_declares_the_expected_surface():
    syms = declared_symbols()
    for must in ["pgl_pg_draw", "pgl_weighted_gram", "pgl_activation", "pgl_pg_loglik", "pgl_flip_decide", "pgl_sample_weights", "pgl_last_error"]:
        assert must in syms


def test_library_exports_every_declared_symbol():
    from pyglm_amd import _lib
    assert os.path.exists(_lib.LIB_PATH), "build first: python -c 'import __graft_entry__ as g; g.build()'"
    lib = ctypes.CDLL(_lib.LIB_PATH)
    for s in declared_symbols():
        assert hasattr(lib, s), "libpyglm_hip.so does not export %s" % s
    assert sorted(_lib.SIGNATURES) == declared_symbols()      # the ctypes table mirrors the header 1:1
    assert _lib.load().pgl_abi_version() == _lib.ABI_VERSION == 11
    assert _lib.load().pgl_flip_kmax() == 512 and _lib.load().pgl_flip_window_blocks(5) == 64
    # host-side constants of the integer Gram: bits of the column norms per number of moduli, fewest moduli at the fp64 level
    lib = _lib.load()
    assert [lib.pgl_i8_norm_bits(k, 100000) for k in (12, 13, 14, 15)] == [46, 50, 54, 58]
    assert lib.pgl_i8_max_planes() == 15 and lib.pgl_i8_min_planes(100000) == 13 and 50.7 < __import__('math').log2(lib.pgl_i8_norm_limit(13, 100000)) < 50.8


def test_struct_layouts_match_header_field_order():
    from pyglm_amd import _lib
    text = re.sub(r"/\*.*?\*/", "", open(os.path.join(ROOT, "include", "pyglm_hip.h")).read(), flags=re.S)
    for cname, cls in [("pgl_flip_t", _lib.FlipState), ("pgl_chol_t", _lib.CholState), ("pgl_dataset_t", _lib.Dataset), ("pgl_sweep_t", _lib.Sweep),
                       ("pgl_stage_times_t", _lib.StageTimes)]:
        body = re.search(r"typedef struct \{([^{}]*)\} %s;" % cname, text).group(1)
        body = re.sub(r"/\*.*?\*/", "", body, flags=re.S)
        names = []
        for decl in body.split(";"):
            decl = decl.strip()
            if not decl:
                continue
            for part in decl.split(","):
                names.append(re.findall(r"([A-Za-z_0-9]+)\s*$", re.sub(r"\[[^\]]*\]", "", part).strip())[0])
        assert names == [f[0] for f in cls._fields_], (cname, names)


SNIPPET = """
#ifndef SNIPPET_H
#define SNIPPET_H
#include <stdint.h>
extern "C" {
#define PGL_NSTAGES 3
#define PGL_NEGATIVE -2
typedef struct { int T; const double* X; } pgl_dataset_t;   /* a comment; with, punctuation (inside) */
typedef struct {
    int nb, N, B;
    double ms[PGL_NSTAGES];
    int calls[2]; unsigned int mask;
    const pgl_dataset_t* datasets; int ndatasets;
    long long* moments;
} pgl_thing_t;
int pgl_nothing(void);
const char* pgl_text(int i);
size_t pgl_bytes(int N, long ld);
double pgl_limit(int nplanes, int T);
int pgl_fold(const pgl_thing_t* s, long long* moments,   /* a prototype over three lines */
             unsigned long long seed, uint64_t elem0, uint32_t draw,
             long long big, unsigned int mask, size_t n, const double* Y, void* hip_stream);
}
#endif
"""


def test_parser_on_literal_snippets():
    from ctypes import POINTER, c_char_p, c_double, c_int, c_long, c_longlong, c_size_t, c_uint, c_uint32, c_uint64, c_ulonglong, c_void_p
    from pyglm_amd._lib import parse_header
    consts, structs, funcs = parse_header(SNIPPET)
    assert consts == {"PGL_NSTAGES": 3, "PGL_NEGATIVE": -2}           # the include guard is no constant
    ds, th = structs["pgl_dataset_t"], structs["pgl_thing_t"]
    assert list(structs) == ["pgl_dataset_t", "pgl_thing_t"] and ds.__name__ == "Dataset" and issubclass(th, ctypes.Structure)
    assert ds._fields_ == [("T", c_int), ("X", c_void_p)]
    assert th._fields_ == [("nb", c_int), ("N", c_int), ("B", c_int), ("ms", c_double * 3), ("calls", c_int * 2), ("mask", c_uint),
                           ("datasets", POINTER(ds)), ("ndatasets", c_int), ("moments", c_void_p)]
    assert funcs == {"pgl_nothing": (c_int, []), "pgl_text": (c_char_p, [("i", c_int)]), "pgl_bytes": (c_size_t, [("N", c_int), ("ld", c_long)]),
                     "pgl_limit": (c_double, [("nplanes", c_int), ("T", c_int)]),
                     "pgl_fold": (c_int, [("s", POINTER(th)), ("moments", c_void_p), ("seed", c_ulonglong), ("elem0", c_uint64), ("draw", c_uint32),
                                          ("big", c_longlong), ("mask", c_uint), ("n", c_size_t), ("Y", c_void_p), ("hip_stream", c_void_p)])}
    assert parse_header("") == ({}, {}, {})


@pytest.mark.parametrize("text, named", [
    ("int pgl_f(float16 x);", "float16"),                                  # unknown type
    ("int pgl_f(float16* x);", "float16"),
    ("typedef struct { float16 x; } pgl_s_t;", "float16"),
    ("pgl_s_t pgl_f(int x);", "pgl_s_t"),                                  # ... as a return type
    ("typedef struct { int x; } pgl_s_t; int pgl_f(pgl_s_t s);", "pgl_f"),  # a struct by value
    ("int pgl_f(int a, double);", "double"),                               # unnamed parameter
    ("int pgl_f(int a, const double*);", "pgl_f"),
    ("int pgl_f(long long);", "pgl_f"),
    ("int pgl_f();", "pgl_f"),
    ("typedef struct { double* a, b; } pgl_s_t;", "double* a, b"),
    ("typedef struct { double ms[PGL_UNKNOWN]; } pgl_s_t;", "PGL_UNKNOWN"),
    ("int pgl_f(int a); static int x = 3; int pgl_g(int b);", "static int x = 3"),     # stray text between declarations
    ("int pgl_f(int a);\n// a line comment\nint pgl_g(int b);", "a line comment"),
    ("int pgl_f(int a) { return a; }", "return a"),
    ("typedef struct { struct { int x; } in; } pgl_s_t;", "typedef struct"),
    ("#define PGL_RATE 1.5\nint pgl_f(int a);", "PGL_RATE"),
])
def test_parser_refuses_what_it_cannot_classify(text, named):
    from pyglm_amd._lib import PglError, parse_header
    with pytest.raises(PglError) as e:
        parse_header(text)
    assert named in str(e.value), str(e.value)


def header_constants():
    return {k: int(v) for k, v in re.findall(r"^#define\s+(PGL_\w+)\s+(-?\d+)\s*$", open(os.path.join(ROOT, "include", "pyglm_hip.h")).read(), flags=re.M)}


def test_constants_are_the_headers():
    from pyglm_amd import _lib, rescale, simulate
    consts = header_constants()
    assert len(consts) == 10 and consts["PGL_ABI_VERSION"] == 11 and not hasattr(_lib, "PYGLM_HIP_H")
    for name, value in consts.items():
        assert getattr(_lib, name) == value and type(getattr(_lib, name)) is int, name
    assert _lib.CONSTANTS == consts and _lib.ABI_VERSION == consts["PGL_ABI_VERSION"] and _lib.NSTAGES == consts["PGL_NSTAGES"]
    assert simulate.PGL_LAG_MAX == consts["PGL_LAG_MAX"] and simulate.PGL_ISI_MAX_BINS == consts["PGL_ISI_MAX_BINS"]
    assert (simulate.LAG_I8, simulate.LAG_F64) == (consts["PGL_LAG_I8"], consts["PGL_LAG_F64"]) == (0, 1)
    assert simulate.PGL_COND_MAX_FREE == consts["PGL_COND_MAX_FREE"] and simulate.BINOMIAL_MAX_N == consts["PGL_SIM_BINOMIAL_MAX_N"]
    assert rescale.PGL_RESCALE_MAX_BINS == consts["PGL_RESCALE_MAX_BINS"]


def test_binding_is_derived_for_every_prototype():
    """argument types, parameter names and return types of the whole header: one row per function, every type classified"""
    from pyglm_amd import _lib
    assert sorted(_lib.FUNCTIONS) == sorted(_lib.PARAMS) == sorted(_lib.SIGNATURES) == declared_symbols() and len(_lib.FUNCTIONS) == 65
    for name, (restype, params) in _lib.FUNCTIONS.items():
        assert _lib.SIGNATURES[name] == [t for _, t in params] and _lib.PARAMS[name] == [p for p, _ in params]
        assert len(set(_lib.PARAMS[name])) == len(params), name
    by_ret = {}
    for name, (restype, _) in _lib.FUNCTIONS.items():
        by_ret.setdefault(restype, []).append(name)
    assert sorted(by_ret[ctypes.c_char_p]) == ["pgl_last_error", "pgl_stage_name"] and by_ret[ctypes.c_double] == ["pgl_i8_norm_limit"]
    assert sorted(by_ret[ctypes.c_size_t]) == sorted(n for n in _lib.FUNCTIONS if n.endswith("_bytes")) and len(by_ret[ctypes.c_size_t]) == 7
    assert set(by_ret) == {ctypes.c_int, ctypes.c_char_p, ctypes.c_double, ctypes.c_size_t}
    assert _lib.PARAMS["pgl_pg_loglik_ex"][-5:] == ["seed", "sweep", "neuron0", "elem0", "hip_stream"]
    assert _lib.SIGNATURES["pgl_pg_loglik_ex"][-5:] == [ctypes.c_uint64] * 4 + [ctypes.c_void_p]
    assert _lib.SIGNATURES["pgl_simulate"][_lib.PARAMS["pgl_simulate"].index("seed")] is ctypes.c_ulonglong
    assert _lib.SIGNATURES["pgl_sweep"][0] is ctypes.POINTER(_lib.Sweep) and _lib.SIGNATURES["pgl_sweep_dims"][3:] == [ctypes.c_void_p] * 3
    assert dict(_lib.Sweep._fields_)["datasets"] is ctypes.POINTER(_lib.Dataset) and dict(_lib.Sweep._fields_)["times"] is ctypes.POINTER(_lib.StageTimes)


def _c_compiler():
    import shutil
    for cc in ("cc", "gcc", "clang"):
        if shutil.which(cc):
            return shutil.which(cc)
    hipcc = shutil.which("hipcc")          # the ROCm root is where the compiler the build uses lives: <root>/bin/hipcc
    clang = os.path.join(os.environ.get("ROCM_PATH") or os.path.dirname(os.path.dirname(os.path.realpath(hipcc or "/"))), "llvm", "bin", "clang")
    return clang if os.path.exists(clang) else None


def test_struct_layouts_match_the_compiler(tmp_path):
    """sizeof of the five structs and offsetof of every field, as a C compiler lays the header out, against the ctypes classes"""
    import subprocess
    from pyglm_amd import _lib
    cc = _c_compiler()
    if cc is None:
        pytest.skip("no C compiler: none of cc, gcc, clang on PATH and no <ROCm root>/llvm/bin/clang")
    structs = {c: getattr(_lib, py) for c, py in _lib._CLASS_NAMES.items()}
    lines = ["#include <stdio.h>", "#include <stddef.h>", '#include "pyglm_hip.h"', "int main(void) {"]
    for c, cls in structs.items():
        lines.append('    printf("%s %%zu\\n", sizeof(%s));' % (c, c))
        lines += ['    printf("%s.%s %%zu\\n", offsetof(%s, %s));' % (c, f, c, f) for f, _ in cls._fields_]
    src = tmp_path / "layout.c"
    src.write_text("\n".join(lines + ["    return 0;", "}", ""]))
    subprocess.run([cc, "-I", os.path.join(ROOT, "include"), str(src), "-o", str(tmp_path / "layout")], check=True)
    out = subprocess.run([str(tmp_path / "layout")], check=True, capture_output=True, text=True).stdout
    got = {k: int(v) for k, v in (line.split() for line in out.splitlines())}
    want = {}
    for c, cls in structs.items():
        want[c] = ctypes.sizeof(cls)
        want.update({"%s.%s" % (c, f): getattr(cls, f).offset for f, _ in cls._fields_})
    assert got == want
    assert [got[c] for c in ("pgl_flip_t", "pgl_chol_t", "pgl_dataset_t", "pgl_stage_times_t", "pgl_sweep_t")] == [184, 152, 112, 336, 464]
    assert (got["pgl_sweep_t.times"], got["pgl_sweep_t.obs_param"], got["pgl_stage_times_t.mask"]) == (448, 456, 328)


def test_call_by_parameter_name():
    """call(name, **by_name) orders the keywords by the header's parameter names; pgl_sweep_dims launches nothing and returns its values
    through host out-parameters (call itself returns only the zero status)"""
    from pyglm_amd import _lib
    from pyglm_amd._lib import call
    assert os.path.exists(_lib.LIB_PATH), "build first: python -c 'import __graft_entry__ as g; g.build()'"

    def dims(**kw):
        out = [ctypes.c_int(-1) for _ in range(3)]
        if kw:
            assert call("pgl_sweep_dims", Dp=ctypes.byref(out[0]), ldn=ctypes.byref(out[1]), ldj=ctypes.byref(out[2]), **kw) == 0
        else:
            assert call("pgl_sweep_dims", 7, 3, 5, *[ctypes.byref(o) for o in out]) == 0
        return [o.value for o in out]

    assert dims() == dims(N=7, B=3, nloc=5) == dims(nloc=5, B=3, N=7) == [32, 6, 32]       # D + 1 = 22 and D + 2 = 23 up to 16; nloc up to even
    assert dims(nloc=3, N=7, B=5) == [48, 4, 48]          # the names, not the order written, place a value
    out = ctypes.c_int(-1)
    assert call("pgl_sweep_dims", N=7, B=3, nloc=5, Dp=None, ldn=None, ldj=ctypes.byref(out)) == 0 and out.value == 32

    class Untouched(object):
        def __getattr__(self, name):
            raise AssertionError("the library was touched: %s" % name)
    lib, _lib._lib = _lib._lib, Untouched()
    try:
        for kw, args, words in [(dict(N=7, B=3, nloc=5, Dp=None, ldn=None, ldj=None, stream=None), (), ("stream",)),     # unknown name
                                (dict(N=7, B=3, Dp=None, ldn=None, ldj=None), (), ("nloc",)),                          # missing name
                                (dict(nloc=5, Dp=None, ldn=None, ldj=None), (7, 3), ("nloc",))]:                       # a mix
            with pytest.raises(TypeError) as e:
                call("pgl_sweep_dims", *args, **kw)
            assert "pgl_sweep_dims" in str(e.value) and all("'%s'" % w in str(e.value) for w in words), str(e.value)
    finally:
        _lib._lib = lib


def test_shipped_library_reads_no_environment_variable():
    """tuning knobs live behind -DPGL_AB (`make -C pyglm_amd/csrc ab`), which the package never loads: no getenv in the product sources outside
    that fence, and none imported by the shipped library"""
    import subprocess
    from pyglm_amd import _lib
    src = os.path.join(ROOT, "pyglm_amd", "csrc")
    for f in sorted(os.listdir(src)):
        if f.endswith((".hip", ".h")):
            text = open(os.path.join(src, f)).read()
            text = re.sub(r"#ifdef PGL_AB\n.*?#else", "", text, flags=re.S)
            assert "getenv" not in text, f
    nm = subprocess.run(["nm", "-D", "--undefined-only", _lib.LIB_PATH], capture_output=True, text=True)
    if nm.returncode == 0:
        assert "getenv" not in nm.stdout


def test_no_gpu_means_loud_failure():
    import torch
    if torch.cuda.is_available():
        pytest.skip("a GPU is present")
    from pyglm_amd._lib import PglError
    from pyglm_amd.engine import GibbsEngine
    with pytest.raises(PglError):
        GibbsEngine(4, 1)


def test_product_never_imports_the_oracle():
    for dirpath, _, files in os.walk(os.path.join(ROOT, "pyglm_amd")):
        for f in files:
            if f.endswith(".py"):
                src = open(os.path.join(dirpath, f)).read()
                assert not re.search(r"^\s*(from|import)\s+oracle\b", src, flags=re.M), f
