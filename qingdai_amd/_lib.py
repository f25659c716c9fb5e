"""
qingdai_amd/_lib.py -- ctypes binding of libqingdai_hip.so, read from include/qingdai_hip.h.

The header is the one statement of the C ABI: its integer constants and enumerators (C), its structs (qd_X) and its
prototypes (SYMBOLS, PROTOTYPES, SIGNATURES) are parsed from it here and written nowhere else.  `call` is the one way into the
library: it marshals every argument by the parameter the header declares and checks the return code.

There is no CPU fallback: if the HIP library is missing or no GPU is visible the
product raises.  (The oracle under oracle/ is test infrastructure and is never
imported from here.)
"""
from __future__ import annotations

import ctypes
import os
import re
import types

import numpy as np

_HERE = os.path.dirname(os.path.abspath(__file__))
LIB_PATH = os.environ.get("QD_LIB_PATH") or os.path.join(_HERE, "libqingdai_hip.so")     # QD_LIB_PATH: developer A/B builds
HEADER_PATH = os.path.join(_HERE, "..", "include", "qingdai_hip.h")


class QdError(RuntimeError):
    pass


# ---- the header reader -------------------------------------------------------------------------------------------------------
_SCALARS = {"int": ctypes.c_int, "int32_t": ctypes.c_int32, "int64_t": ctypes.c_int64, "long long": ctypes.c_longlong,
            "size_t": ctypes.c_size_t, "double": ctypes.c_double}
NP_OF = {"int": np.intc, "int32_t": np.int32, "int64_t": np.int64, "long long": np.longlong, "size_t": np.uintp, "double": np.float64,
         "uint8_t": np.uint8, "uint64_t": np.uint64}                                    # the NumPy twin of what an array parameter may be of
_C_OF = {**_SCALARS, "uint8_t": ctypes.c_uint8, "uint64_t": ctypes.c_uint64}         # ... and the ctypes twin, and the pointer to it
_PTR_OF = {k: ctypes.POINTER(t) for k, t in _C_OF.items()}
_POINTEES = set(_SCALARS) | {"void", "char", "uint8_t", "uint64_t", "qd_handle"}      # what a pointer or array may be of
_ITEM = re.compile(r"""\s*(?:
      \#[ \t]*define[ \t]+(?P<define>QD_\w+)[ \t]+(?P<value>\w+)[ \t]*$
    | \#(?![ \t]*define[ \t]+QD_)[^\n]*$ | extern\s+"C"\s*\{ | \}
    | (?:typedef\s+)?enum\s*\w*\s*\{(?P<enum>[^{}]*)\}\s*\w*\s*;
    | typedef\s+struct\s+(?P<struct>\w+)\s*\{(?P<members>[^{}]*)\}\s*(?P=struct)\s*;
    | typedef\s+struct\s+\w+\s*\*\s*qd_handle\s*;
    | (?P<proto>[^;{}\#]*\([^;{}\#]*\))\s*;
    )""", re.M | re.X)
_DECL = re.compile(r"(?P<const>const\s+)?(?P<base>long\s+long|\w+)\s*(?P<ptr>\*{0,2})\s*(?P<names>[\w\s,\[\]]*)")
_NAME = re.compile(r"(?P<name>\w*)\s*(?P<dims>(?:\[\s*\w*\s*\]\s*)*)")


def _integer(token, consts, where):
    if token in consts:
        return consts[token]
    try:
        return int(token, 0)
    except ValueError:
        raise QdError(f"include/qingdai_hip.h: '{token}' is no integer and no earlier constant, in: {where}") from None


def _decl(text, structs, where):
    """'const double* x', 'int32_t a, b', 'double rgb[N][3]' -> (const?, base type, pointer stars, [(name, [dims])])"""
    m = _DECL.fullmatch(text.strip())
    names = [_NAME.fullmatch(n.strip()) for n in m.group("names").split(",")] if m else [None]
    if not all(names):
        raise QdError(f"include/qingdai_hip.h: cannot parse '{' '.join(text.split())}' in: {where}")
    base = " ".join(m.group("base").split())
    if base not in _POINTEES and base not in structs:
        raise QdError(f"include/qingdai_hip.h: unknown type '{base}' in: {where}")
    return bool(m.group("const")), base, m.group("ptr"), [(n.group("name"), re.findall(r"\[\s*(\w*)\s*\]", n.group("dims"))) for n in names]


def _value_type(base, by_value, where):
    if base not in by_value:
        raise QdError(f"include/qingdai_hip.h: a '{base}' cannot be passed or stored by value, in: {where}")
    return by_value[base]


def _param(text, structs, where):
    """One parameter (or return type) -> (its ctypes type, (name, kind, base type, is_const)).  The one rule of the binding:
    scalars by their ctypes twin, qd_handle a void pointer, qd_handle* / void** a pointer to one, const char* a C string,
    const qd_X* a pointer to that struct; every other pointer and every array parameter a void pointer.  The kinds, which
    `call` marshals by: scalar, handle, handle_out, cstring, struct_ptr, array (of a type of NP_OF), void_ptr."""
    const, base, ptr, [(name, dims)] = _decl(text, structs, where)
    if not (dims or ptr):
        return _value_type(base, {**_SCALARS, "qd_handle": ctypes.c_void_p}, where), (name, "handle" if base == "qd_handle" else "scalar", base, const)
    if (base, ptr) in (("qd_handle", "*"), ("void", "**")) and not dims:
        return ctypes.POINTER(ctypes.c_void_p), (name, "handle_out", base, const)
    if const and ptr == "*" and not dims and (base == "char" or base in structs):
        return (ctypes.c_char_p, (name, "cstring", base, const)) if base == "char" else (ctypes.POINTER(structs[base]), (name, "struct_ptr", base, const))
    return ctypes.c_void_p, (name, "array" if base in NP_OF else "void_ptr", base, const)


def parse_header(text):
    """The text of a C header in the style of include/qingdai_hip.h -> a namespace of
         constants   {name: int}: every `#define QD_* <integer or earlier constant>` and every enumerator, in header order
         structs     {name: ctypes.Structure subclass}: every `typedef struct qd_X { ... } qd_X;`
         prototypes  {name: (restype, [argtypes])}: every function declared, by the rule of _param
         signatures  {name: [(parameter name, kind, base type, is_const)]}: what the header says of each parameter
    Anything else at the top level, an unknown type word or an unreadable declaration raises a QdError that names it."""
    text = re.sub(r"/\*.*?\*/|//[^\n]*", " ", text, flags=re.S)
    consts, structs, protos, sigs = {}, {}, {}, {}
    pos = 0
    while text[pos:].strip():
        m = _ITEM.match(text, pos)
        if not m:
            raise QdError(f"include/qingdai_hip.h: cannot parse the declaration '{' '.join(text[pos:].split(';')[0].split())}'")
        pos = m.end()
        where = " ".join(m.group(0).split())
        if m.group("define"):
            consts[m.group("define")] = _integer(m.group("value"), consts, where)
        elif m.group("enum") is not None:
            nxt = 0
            for item in filter(None, (i.strip() for i in m.group("enum").split(","))):
                name, eq, val = (p.strip() for p in item.partition("="))
                if not re.fullmatch(r"\w+", name) or (eq and not re.fullmatch(r"\w+", val)):
                    raise QdError(f"include/qingdai_hip.h: cannot parse the enumerator '{item}' in: {where}")
                consts[name] = nxt = _integer(val, consts, where) if eq else nxt
                nxt += 1
        elif m.group("struct"):
            fields = []
            for member in filter(None, (s.strip() for s in m.group("members").split(";"))):
                _, base, ptr, names = _decl(member, structs, where)
                for name, dims in names:
                    t = ctypes.c_void_p if ptr else _value_type(base, {**_SCALARS, **structs}, where)
                    for d in reversed(dims):
                        t = t * _integer(d, consts, where)
                    fields.append((name, t))
            structs[m.group("struct")] = type(m.group("struct"), (ctypes.Structure,),
                                              {"_fields_": fields, "__doc__": f"include/qingdai_hip.h: {m.group('struct')}"})
        elif m.group("proto"):
            head, _, params = m.group("proto").rstrip()[:-1].partition("(")
            ret = re.fullmatch(r"(.*?)(\w+)\s*", head, flags=re.S)
            if not ret or not ret.group(1).strip():
                raise QdError(f"include/qingdai_hip.h: cannot parse the declaration '{where}'")
            args = [] if params.strip() in ("", "void") else [_param(p, structs, where) for p in params.split(",")]
            if not all(sig[0] for _, sig in args):
                raise QdError(f"include/qingdai_hip.h: a parameter without a name in: {where}")
            protos[ret.group(2)] = (_param(ret.group(1), structs, where)[0], [t for t, _ in args])
            sigs[ret.group(2)] = [sig for _, sig in args]
    return types.SimpleNamespace(constants=consts, structs=structs, prototypes=protos, signatures=sigs)


with open(HEADER_PATH, encoding="utf-8") as _f:
    HEADER = parse_header(_f.read())
C = HEADER.constants                  # every integer constant and enumerator of the header, by its C name
PROTOTYPES = HEADER.prototypes
SIGNATURES = HEADER.signatures        # {symbol: [(parameter name, kind, base type, is_const)]}: what `call` marshals by
SYMBOLS = list(PROTOTYPES)            # every symbol include/qingdai_hip.h declares
globals().update(HEADER.structs)      # qd_grid_desc, qd_params, qd_eco_params, ...: the header's structs, by their C names


def _enum(prefix):
    """The header's names that begin with `prefix`, without it, in header order -> value"""
    return {k[len(prefix):]: v for k, v in C.items() if k.startswith(prefix)}


# field ids (enum qd_field): FIELDS are the f64 slabs, F also holds the masks and the diversity results
F = {n: i for n, i in _enum("QD_F_").items() if n != "COUNT_F64"}
FIELDS = [n for n, i in F.items() if i < C["QD_F_COUNT_F64"]]
R_SUM, R_COSMEAN, R_MAX, R_MIN, R_MAXABS = (C["QD_R_" + n] for n in ("SUM", "COSWEIGHTED_MEAN", "MAX", "MIN", "MAXABS"))

TRUECOLOR_MAX_BANDS = C["QD_TRUECOLOR_MAX_BANDS"]
STATEFRAME_PANELS = C["QD_STATEFRAME_PANELS"]
STATEFRAME_MAX_LEVELS = C["QD_STATEFRAME_MAX_LEVELS"]
STATEFRAME_GUTTER = C["QD_STATEFRAME_GUTTER"]
STATEFRAME_SCAN_N = C["QD_STATEFRAME_SCAN_N"]
TILES_MAX = C["QD_TILES_MAX"]
TILES_MAX_RANKS = C["QD_TILES_MAX_RANKS"]
TILE = _enum("QD_TILE_")              # enum qd_tile_source
TILE_SOURCES = tuple(TILE)

SPAN_LOG_CAP = C["QD_SPAN_LOG_CAP"]                  # records a span lane's device log holds between two drains
PHYTO_DAILY_LOG_W = C["QD_PHYTO_DAILY_LOG_W"]        # doubles per [PhytoDiag] record
ECO_DAILY_LOG_W = C["QD_ECO_DAILY_LOG_W"]            # doubles per daily vegetation record {firings, LAI_min, LAI_mean, LAI_max}
INDIV_DAILY_LOG_W = C["QD_INDIV_DAILY_LOG_W"]        # doubles per record of the individuals' daily step {firings, beta_hint, n_cells, levels}
BUDGET_LOG_W = C["QD_BUDGET_LOG_W"]                  # doubles per budget diagnostics record (budget_diag.REC names the slots)
ROUTE_LOG_W = C["QD_ROUTE_LOG_W"]                    # doubles per routing event record (routing.LOG_KEYS)
HISTORY_MAX_ENTRIES = C["QD_HISTORY_MAX_ENTRIES"]
SERIES_MAX_ENTRIES = C["QD_SERIES_MAX_ENTRIES"]
SERIES_LOG_CAP = C["QD_SERIES_LOG_CAP"]              # records the series lane's device log holds between two drains
SERIES_STATS = C["QD_SERIES_STATS"]                  # mean, min, max, nan_count in front of an entry's zonal means
SPECTRA_MAX_ENTRIES = C["QD_SPECTRA_MAX_ENTRIES"]
SPECTRA_LOG_CAP = C["QD_SPECTRA_LOG_CAP"]            # records the spectra lane's device log holds between two drains
SPECTRA_STATS = C["QD_SPECTRA_STATS"]                # the count of non-finite rows behind an entry's n_bins powers
DRIFT_MAX = C["QD_DRIFT_MAX"]                        # particles of one drifter population
DRIFT_MAX_SAMPLES = C["QD_DRIFT_MAX_SAMPLES"]        # sampled planes of one drifter population
STATE_DIGEST_MAX = C["QD_STATE_DIGEST_MAX"]          # refs per qd_state_digest call
STATE_SCALARS_N = C["QD_STATE_SCALARS_N"]
# enum qd_state_scalar: the slots of qd_state_scalars_get / set, by their lower-case names
STATE_SCALAR_SLOT = {n.lower(): i for n, i in _enum("QD_SS_").items()}
# enum qd_state_ref: the resident planes without a field id, as Device.digest names them ("PHYTO_TRACER:3", "HISTORY_SUM:0")
STATE_REFS = _enum("QD_SR_")
STATE_REF_COUNT = {"PHYTO_TRACER": C["QD_STATE_REF_TRACERS"], "HISTORY_SUM": C["QD_STATE_REF_HISTORY_SUMS"]}     # the indexed ones: name:k with k below this


def state_ref(name):
    """A plane's name -> the ref qd_state_digest takes: a field name of F (f64 fields and the two masks), a name of STATE_REFS, or
    an indexed one, "PHYTO_TRACER:s" / "HISTORY_SUM:k", or "SPECTRA_SUMS" / "FLOW_SUMS" / "SPHARM_SUMS" / "EDDY_SUMS" /
    "EDDY_ANCHORS" / "EXTREMES_VALUES" / "EXTREMES_COUNTS" / "EXTREMES_HIST"."""
    if name in FIELDS or name in ("LAND_MASK", "ICE_MASK"):
        return F[name]
    if name == "SPECTRA_SUMS":                        # a ref of its own beside the enum (QD_STATE_REF_SPECTRA_SUMS)
        return C["QD_STATE_REF_SPECTRA_SUMS"]
    if name == "FLOW_SUMS":                           # likewise (QD_STATE_REF_FLOW_SUMS)
        return C["QD_STATE_REF_FLOW_SUMS"]
    if name == "SPHARM_SUMS":                         # likewise (QD_STATE_REF_SPHARM_SUMS)
        return C["QD_STATE_REF_SPHARM_SUMS"]
    if name in ("EDDY_SUMS", "EDDY_ANCHORS"):         # likewise (QD_STATE_REF_EDDY_SUMS, QD_STATE_REF_EDDY_ANCHORS)
        return C["QD_STATE_REF_" + name]
    if name in ("EXTREMES_VALUES", "EXTREMES_COUNTS", "EXTREMES_HIST"):     # likewise (QD_STATE_REF_EXTREMES_*)
        return C["QD_STATE_REF_" + name]
    base, _, idx = str(name).partition(":")
    if base in STATE_REF_COUNT and idx.isdigit() and int(idx) < STATE_REF_COUNT[base]:
        return STATE_REFS[base] + int(idx)
    if base in STATE_REFS and base not in STATE_REF_COUNT and not idx:
        return STATE_REFS[base]
    raise KeyError(f"'{name}' names no resident plane (a field of FIELDS, LAND_MASK, ICE_MASK, {', '.join(STATE_REFS)})")


# enum qd_step_flag: bit k of qd_step_n's flags switches STEP_BITS[k], named as Device.step_n's keywords
_STEP = {n.lower(): v for n, v in _enum("QD_STEP_").items()}
STEP_BITS = tuple(sorted(_STEP, key=_STEP.get))


def step_flags(**on):
    return sum(_STEP[k] for k, v in on.items() if v)


# ---- the one call seam -----------------------------------------------------------------------------------------------------------
class OUT:
    """In the place of an output pointer: `call` allocates it and returns what the library stored.  OUT = one element, handed
    back as a Python number; OUT(n) = n elements, handed back as an ndarray."""

    def __init__(self, n):
        self.n = int(n)


def _refuse(symbol, name, why):
    raise TypeError(f"{symbol}: {name}: {why}")


def call(lib, symbol, args, *, last_error, error=QdError, what=None):
    """Call `symbol` of `lib` with `args` marshalled by its declaration in the header, and check its return code.
         scalar          a number or bool -> int / float
         const char*     str or bytes -> bytes
         const qd_X*     an instance of that struct -> a pointer to it (a ctypes array of them passes as it is)
         const T*, T[N]  anything np.ascontiguousarray(x, dtype=NP_OF[T]) takes; the temporary lives until the call returns
         T*, T[N]        OUT / OUT(n), a ctypes instance or array of T, or a C-contiguous writeable ndarray of exactly NP_OF[T];
                         anything else is a TypeError before the library is entered
         void*           an address, or a C-contiguous ndarray (writeable unless the parameter is const)
         handles         as they are
    None is NULL for every pointer.  A non-zero return raises error(f"{what or symbol} failed: " + last_error()).  -> the values
    of the OUT arguments in parameter order: None, the one value, or a tuple."""
    sig = SIGNATURES[symbol]
    if len(args) != len(sig):
        raise TypeError(f"{symbol} takes {len(sig)} arguments, {len(args)} were given")
    passed, outs, keep = [], [], []                              # keep: the arrays passed by a bare address, alive until the return
    for (name, kind, base, const), x in zip(sig, args):
        if kind == "scalar":
            x = float(x) if base == "double" else int(x)
        elif x is None or kind in ("handle", "handle_out"):
            pass
        elif kind == "cstring":
            x = x.encode() if isinstance(x, str) else x
        elif kind == "struct_ptr":
            if isinstance(x, ctypes.Structure):                  # a ctypes array of them passes as it is
                if type(x).__name__ != base:
                    _refuse(symbol, name, f"a {type(x).__name__} where a {base} is declared")
                x = ctypes.pointer(x)
        elif kind == "void_ptr":
            if isinstance(x, np.ndarray):
                if not x.flags.c_contiguous or not (const or x.flags.writeable):
                    _refuse(symbol, name, "the array must be C-contiguous" + ("" if const else " and writeable"))
                keep.append(x)
                x = x.ctypes.data
        elif const:
            x = np.ascontiguousarray(x, dtype=NP_OF[base]).ctypes.data_as(_PTR_OF[base])      # the pointer holds the temporary
        elif x is OUT or isinstance(x, OUT):
            outs.append(((_C_OF[base] * (1 if x is OUT else x.n))(), x is OUT, base))
            x = outs[-1][0]
        elif isinstance(x, np.ndarray):
            if x.dtype != NP_OF[base] or not x.flags.c_contiguous or not x.flags.writeable:
                _refuse(symbol, name, f"an output must be a C-contiguous writeable {np.dtype(NP_OF[base]).name} array, not "
                                      f"{x.dtype.name}{'' if x.flags.c_contiguous else ', strided'}{'' if x.flags.writeable else ', read-only'}")
            x = x.ctypes.data_as(_PTR_OF[base])
        elif isinstance(x, _C_OF[base]):
            x = ctypes.pointer(x)
        elif not (isinstance(x, ctypes.Array) and x._type_ is _C_OF[base]):
            _refuse(symbol, name, f"an output must be OUT, an ndarray or a ctypes {base}, not a {type(x).__name__}")
        passed.append(x)
    if getattr(lib, symbol)(*passed) != 0:
        raise error(f"{what or symbol} failed: " + (last_error() or b"?").decode())
    got = [c[0] if one else np.frombuffer(c, dtype=NP_OF[base]) for c, one, base in outs]
    return None if not got else got[0] if len(got) == 1 else tuple(got)


_lib = None


def load():
    """Load the HIP library; fail loudly when it is absent (no fallback path exists)."""
    global _lib
    if _lib is not None:
        return _lib
    if not os.path.exists(LIB_PATH):
        raise QdError(f"{LIB_PATH} not found: build it with `python -c 'import __graft_entry__ as g; g.build()'` "
                      f"or `make -C qingdai_amd/csrc` (hipcc, gfx950). There is no CPU fallback.")
    lib = ctypes.CDLL(LIB_PATH, mode=ctypes.RTLD_GLOBAL)
    for name, (restype, argtypes) in PROTOTYPES.items():
        fn = getattr(lib, name)
        fn.restype, fn.argtypes = restype, argtypes
    _lib = lib
    return lib
