"""ctypes binding of libpyglm_hip.so, derived at import from the one statement of its C ABI, include/pyglm_hip.h: argument and return types,
parameter names, struct layouts and constants. Fails loudly when the library is absent, and when the header holds a declaration the
parser below cannot classify completely."""
import ctypes
import os
import re

_HERE = os.path.dirname(os.path.abspath(__file__))
LIB_PATH = os.path.join(_HERE, "lib", "libpyglm_hip.so")
HEADER = os.path.join(os.path.dirname(_HERE), "include", "pyglm_hip.h")
# the entries added beside ABI 11 (the dispersion fold): a header of the same regular shape, parsed into tables of its own -- FUNCTIONS,
# SIGNATURES, PARAMS and CONSTANTS describe pyglm_hip.h alone
HEADER_DISPERSION = os.path.join(os.path.dirname(_HERE), "include", "pyglm_hip_dispersion.h")
# the entries of the chain diagnostics (batch means, conditional edge probabilities): a third header, tables of its own likewise
HEADER_DIAGNOSTICS = os.path.join(os.path.dirname(_HERE), "include", "pyglm_hip_diagnostics.h")
# the entries of the learned network priors (block-assignment scan, block counts, partition fold): a fourth header, tables of its own likewise
HEADER_SBM = os.path.join(os.path.dirname(_HERE), "include", "pyglm_hip_sbm.h")
# the entries of the external covariates (offset, fold, draw, the sweep under an offset): a fifth header, tables of its own likewise; it takes
# pgl_sweep_t from pyglm_hip.h (parse_header's `known`)
HEADER_COVARIATES = os.path.join(os.path.dirname(_HERE), "include", "pyglm_hip_covariates.h")
# the entries of the latent common input (the fold over neurons per time bin, the draw of x_t): a sixth header, tables of its own likewise
HEADER_LATENTS = os.path.join(os.path.dirname(_HERE), "include", "pyglm_hip_latents.h")
# the entry of the latents' temporal prior (the block-tridiagonal draw): a seventh header, tables of its own likewise
HEADER_LATENT_DYNAMICS = os.path.join(os.path.dirname(_HERE), "include", "pyglm_hip_latent_dynamics.h")
# the entries of free-running simulation under covariates and latents (pgl_simulate under an offset, the offset, the latents' prior paths):
# an eighth header, tables of its own likewise
HEADER_SIMULATE_OFFSET = os.path.join(os.path.dirname(_HERE), "include", "pyglm_hip_simulate_offset.h")


class PglError(RuntimeError):
    pass


_SCALARS = {"int": ctypes.c_int, "long": ctypes.c_long, "long long": ctypes.c_longlong, "unsigned int": ctypes.c_uint,
            "unsigned long long": ctypes.c_ulonglong, "double": ctypes.c_double, "size_t": ctypes.c_size_t, "uint32_t": ctypes.c_uint32,
            "uint64_t": ctypes.c_uint64, "uint8_t": ctypes.c_uint8}
_TYPE_WORDS = {w for t in _SCALARS for w in t.split()} | {"const", "void", "char"}
_CLASS_NAMES = {"pgl_flip_t": "FlipState", "pgl_chol_t": "CholState", "pgl_dataset_t": "Dataset", "pgl_stage_times_t": "StageTimes",
                "pgl_sweep_t": "Sweep"}


def parse_header(text, known=None, header="pyglm_hip.h"):
    """The declarations of a C header in the header's own regular style -> (constants {name: int}, structs {typedef name: ctypes.Structure
    class}, functions {name: (restype, [(parameter name, ctypes type), ...])}). A pointer to a struct typedef of the header is POINTER(its
    class), every other pointer -- a pointer to pointers of a scalar type too -- c_void_p. known: the struct classes of a header this one
    includes ({typedef name: class}); a pointer to one of them is POINTER(its class). header: the header's file name, for the errors. Raises
    PglError, naming the header and the declaration, on whatever it cannot classify: no default type."""
    consts, structs, funcs = {}, {}, {}

    def directive(m):    # '#define PGL_<NAME> <integer>' is a constant and a define without a value an include guard; other directives drop out
        d = re.fullmatch(r"define\s+(\w+)(?:\s+(.*\S))?\s*", m.group(1))
        if d and d.group(2) is not None:
            if not (d.group(1).startswith("PGL_") and re.fullmatch(r"-?\d+", d.group(2))):
                raise PglError("%s: '#%s' does not define an integer PGL_ constant" % (header, m.group(1).strip()))
            consts[d.group(1)] = int(d.group(2))
        return ""

    def ctype(spec, decl):
        words = spec.replace("*", " * ").split()
        base, stars = " ".join(w for w in words if w not in ("const", "*")), words.count("*")
        if stars == 0 and base in _SCALARS:
            return _SCALARS[base]
        if stars == 1 and (base in structs or base in (known or {})):
            return ctypes.POINTER(structs[base] if base in structs else known[base])
        if (stars == 1 and (base in _SCALARS or base == "void")) or (stars == 2 and base in _SCALARS):
            return ctypes.c_void_p
        raise PglError("%s: unknown type '%s' in: %s" % (header, spec.strip(), decl))

    def named(spec, decl):    # 'type name' or 'type name[DIM]' -> (type text, name, ctypes type)
        m = re.fullmatch(r"(.*[\s*])(\w+)\s*(?:\[\s*(\w+)\s*\])?", spec.strip(), flags=re.S)
        if not m or m.group(2) in _TYPE_WORDS:
            raise PglError("%s: no name for '%s' in: %s" % (header, spec.strip(), decl))
        t, dim = ctype(m.group(1), decl), m.group(3)
        if dim is not None and not (dim.isdigit() or dim in consts):
            raise PglError("%s: unknown array size '%s' in: %s" % (header, dim, decl))
        return m.group(1), m.group(2), t if dim is None else t * (int(dim) if dim.isdigit() else consts[dim])

    def struct(m):
        fields = []
        for decl in filter(None, (" ".join(d.split()) for d in m.group(1).split(";"))):
            first, *more = decl.split(",")
            spec, name, t = named(first, decl)
            if more and "*" in spec:
                raise PglError("%s: several declarators after a pointer type in: %s" % (header, decl))
            fields += [(name, t)] + [named(spec + d, decl)[1:] for d in more]
        structs[m.group(2)] = type(_CLASS_NAMES.get(m.group(2), m.group(2)), (ctypes.Structure,), {"_fields_": fields})
        return ""

    text = re.sub(r"/\*.*?\*/", " ", text, flags=re.S)
    text = re.sub(r"^[ \t]*#[ \t]*(.*)$", directive, text, flags=re.M)
    text = re.sub(r'\A\s*extern\s+"C"\s*\{(.*)\}\s*\Z', r"\1", text, flags=re.S)
    text = re.sub(r"\btypedef\s+struct\s*\{([^{}]*)\}\s*(\w+)\s*;", struct, text)
    for decl in filter(None, (" ".join(d.split()) for d in text.split(";"))):
        m = re.fullmatch(r"(.*[\s*])(\w+)\s*\((.*)\)", decl)
        if not m:
            raise PglError("%s: text that is no declaration: %s" % (header, decl))
        ret, name, params = m.groups()
        restype = ctypes.c_char_p if ret.replace("*", " * ").split() == ["const", "char", "*"] else ctype(ret, decl)
        funcs[name] = (restype, [] if params.strip() == "void" else [named(p, decl)[1:] for p in params.split(",")])
    return consts, structs, funcs


with open(HEADER) as _fh:
    CONSTANTS, _structs, FUNCTIONS = parse_header(_fh.read())
globals().update(CONSTANTS)                                       # PGL_LAG_MAX, PGL_ISI_MAX_BINS, ...: every integer #define of the header
ABI_VERSION, NSTAGES = CONSTANTS["PGL_ABI_VERSION"], CONSTANTS["PGL_NSTAGES"]
FlipState, CholState, Dataset, StageTimes, Sweep = (_structs[c] for c in _CLASS_NAMES)
SIGNATURES = {f: [t for _, t in params] for f, (_, params) in FUNCTIONS.items()}    # symbol -> argument types
PARAMS = {f: [p for p, _ in params] for f, (_, params) in FUNCTIONS.items()}        # symbol -> parameter names, in the header's order
with open(HEADER_DISPERSION) as _fh:
    DISPERSION_CONSTANTS, _, DISPERSION_FUNCTIONS = parse_header(_fh.read(), header=os.path.basename(HEADER_DISPERSION))
globals().update(DISPERSION_CONSTANTS)                            # PGL_PURPOSE_DISPERSION, PGL_DISPERSION_ROWS, ...
DISPERSION_PARAMS = {f: [p for p, _ in params] for f, (_, params) in DISPERSION_FUNCTIONS.items()}
with open(HEADER_DIAGNOSTICS) as _fh:
    DIAGNOSTICS_CONSTANTS, _, DIAGNOSTICS_FUNCTIONS = parse_header(_fh.read(), header=os.path.basename(HEADER_DIAGNOSTICS))
globals().update(DIAGNOSTICS_CONSTANTS)                           # PGL_DIAG_MAX_LEVELS, PGL_DIAG_EDGE, ...
DIAGNOSTICS_PARAMS = {f: [p for p, _ in params] for f, (_, params) in DIAGNOSTICS_FUNCTIONS.items()}
with open(HEADER_SBM) as _fh:
    SBM_CONSTANTS, _, SBM_FUNCTIONS = parse_header(_fh.read(), header=os.path.basename(HEADER_SBM))
globals().update(SBM_CONSTANTS)                                   # PGL_SBM_MAX_BLOCKS, PGL_SBM_MAX_N, PGL_PURPOSE_SBM
SBM_PARAMS = {f: [p for p, _ in params] for f, (_, params) in SBM_FUNCTIONS.items()}
with open(HEADER_COVARIATES) as _fh:
    COVARIATES_CONSTANTS, _, COVARIATES_FUNCTIONS = parse_header(_fh.read(), known=_structs, header=os.path.basename(HEADER_COVARIATES))
globals().update(COVARIATES_CONSTANTS)                            # PGL_COVARIATE_MAX, PGL_COVARIATE_ROWS
COVARIATES_PARAMS = {f: [p for p, _ in params] for f, (_, params) in COVARIATES_FUNCTIONS.items()}
with open(HEADER_LATENTS) as _fh:
    LATENTS_CONSTANTS, _, LATENTS_FUNCTIONS = parse_header(_fh.read(), header=os.path.basename(HEADER_LATENTS))
globals().update(LATENTS_CONSTANTS)                               # PGL_LATENT_MAX, PGL_LATENT_LDS_COLS, PGL_PURPOSE_LATENT
LATENTS_PARAMS = {f: [p for p, _ in params] for f, (_, params) in LATENTS_FUNCTIONS.items()}
with open(HEADER_LATENT_DYNAMICS) as _fh:
    LATENT_DYNAMICS_CONSTANTS, _, LATENT_DYNAMICS_FUNCTIONS = parse_header(_fh.read(), header=os.path.basename(HEADER_LATENT_DYNAMICS))
LATENT_DYNAMICS_PARAMS = {f: [p for p, _ in params] for f, (_, params) in LATENT_DYNAMICS_FUNCTIONS.items()}
with open(HEADER_SIMULATE_OFFSET) as _fh:
    SIMULATE_OFFSET_CONSTANTS, _, SIMULATE_OFFSET_FUNCTIONS = parse_header(_fh.read(), header=os.path.basename(HEADER_SIMULATE_OFFSET))
globals().update(SIMULATE_OFFSET_CONSTANTS)                       # PGL_PURPOSE_SIM_LATENT, PGL_SIM_LATENT_MAX
SIMULATE_OFFSET_PARAMS = {f: [p for p, _ in params] for f, (_, params) in SIMULATE_OFFSET_FUNCTIONS.items()}
_lib = None


def _params(name):
    """the parameter names of entry `name`, of whichever header declares it"""
    for table in (PARAMS, DISPERSION_PARAMS, DIAGNOSTICS_PARAMS, COVARIATES_PARAMS, LATENTS_PARAMS, LATENT_DYNAMICS_PARAMS,
                  SIMULATE_OFFSET_PARAMS):
        if name in table:
            return table[name]
    return SBM_PARAMS[name]


def load():
    """Load the HIP library (once). No fallback: a missing library is an error."""
    global _lib
    if _lib is not None:
        return _lib
    if not os.path.exists(LIB_PATH):
        raise PglError("libpyglm_hip.so not found at %s -- build it with `python -c 'import __graft_entry__ as g; g.build()'` "
                       "or `make -C pyglm_amd/csrc` (there is no CPU fallback)" % LIB_PATH)
    import torch  # noqa: F401  -- FIRST: PyTorch-ROCm carries its own HIP runtime; a process must bind one runtime only, and the library's
    #                      dependency on libamdhip64 has to resolve to the copy torch has loaded (loading the library first leaves
    #                      two runtimes in the process: "no ROCm-capable device is detected" at the first launch)
    lib = ctypes.CDLL(LIB_PATH)
    for functions in (FUNCTIONS, DISPERSION_FUNCTIONS, DIAGNOSTICS_FUNCTIONS, SBM_FUNCTIONS, COVARIATES_FUNCTIONS, LATENTS_FUNCTIONS,
                      LATENT_DYNAMICS_FUNCTIONS, SIMULATE_OFFSET_FUNCTIONS):
        for name, (restype, params) in functions.items():
            fn = getattr(lib, name)     # AttributeError if the export is missing
            fn.argtypes = [t for _, t in params]
            fn.restype = restype
    if lib.pgl_abi_version() != ABI_VERSION:
        raise PglError("libpyglm_hip.so ABI version %d != %d (rebuild: make -C pyglm_amd/csrc)" % (lib.pgl_abi_version(), ABI_VERSION))
    _lib = lib
    return lib


def source_hash():
    """sha256 (first 16 hex digits) over the kernel sources of the library -- pyglm_amd/csrc/*.hip, *.h and the Makefile, in name order, plus
    the eight headers under include/: committed hardware-counter summaries (profiles/*.json) record the hash they were taken at, and bench.py quotes them
    only while it still matches"""
    import hashlib
    h = hashlib.sha256()
    src = os.path.join(_HERE, "csrc")
    files = [os.path.join(src, f) for f in sorted(os.listdir(src)) if f.endswith((".hip", ".h")) or f == "Makefile"]
    files += [HEADER, HEADER_DISPERSION, HEADER_DIAGNOSTICS, HEADER_SBM, HEADER_COVARIATES, HEADER_LATENTS, HEADER_LATENT_DYNAMICS, HEADER_SIMULATE_OFFSET]
    for f in files:
        h.update(os.path.basename(f).encode() + b"\0")
        with open(f, "rb") as fh:
            h.update(fh.read())
    return h.hexdigest()[:16]


def call(name, *args, **by_name):
    """name(*args), or name(**by_name) with the keywords put in the order of the header's parameter names; raises PglError on a non-zero status"""
    if by_name:
        names = _params(name)
        if args:
            raise TypeError("%s: positional values mixed with keyword '%s'" % (name, next(iter(by_name))))
        missing = [k for k in names if k not in by_name]
        if missing or len(by_name) != len(names):
            unknown = [k for k in by_name if k not in names]
            raise TypeError("%s %s '%s'" % (name, "has no parameter" if unknown else "is missing parameter", (unknown or missing)[0]))
        args = [by_name[k] for k in names]
    lib = load()
    rc = getattr(lib, name)(*args)
    if rc != 0:
        raise PglError("%s failed (%d): %s" % (name, rc, lib.pgl_last_error().decode()))
    return rc


def ptr(t):
    """device pointer of a torch tensor (or None)"""
    return None if t is None else ctypes.c_void_p(t.data_ptr())
