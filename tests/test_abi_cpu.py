"""CPU: the one place where the C ABI is checked, for every symbol, struct and constant at once.  The binding is read from
include/qingdai_hip.h (qingdai_amd/_lib.py: parse_header); here the library's exports are compared with the declared names, the
derived structs and constants with what a C compiler makes of the same header, the reader with small header texts, and the
parameter tables with the derived struct.  Product and oracle defaults agree; no compute calls."""
import ctypes
import os
import re
import shutil
import subprocess

import numpy as np
import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
INCLUDE = os.path.join(ROOT, "include")


def _header():
    return re.sub(r"/\*.*?\*/", "", open(os.path.join(INCLUDE, "qingdai_hip.h")).read(), flags=re.S)


def _tool(env, *names):
    """$env, else the first of `names` on the PATH, else the LLVM one that comes with hipcc; none: the test fails."""
    found = [os.environ.get(env)] + [shutil.which(n) for n in names]
    hipcc = shutil.which("hipcc") or "/opt/rocm/bin/hipcc"
    for d in ("../llvm/bin", "../lib/llvm/bin"):
        found += [os.path.join(os.path.dirname(os.path.realpath(hipcc)), d, n) for n in names if n.startswith(("clang", "llvm-"))]
    found = [f for f in found if f and (shutil.which(f) or os.path.exists(f))]
    assert found, f"none of ${env}, {', '.join(names)} found"
    return found[0]


# ---------------------------------------------------------------- exports
def test_library_exports_every_declared_symbol():
    from qingdai_amd import _lib
    lib = _lib.load()
    declared = set(re.findall(r"\b(qd_[a-z0-9_]+)\s*\(", _header()))          # a second, looser reading of the header
    assert declared == set(_lib.SYMBOLS) and len(_lib.SYMBOLS) == len(declared), declared ^ set(_lib.SYMBOLS)
    out = subprocess.run([_tool("NM", "nm", "llvm-nm"), "-D", "--defined-only", _lib.LIB_PATH], check=True, capture_output=True, text=True).stdout
    exported = set(re.findall(r"\bT (qd_\w+)$", out, flags=re.M))
    assert exported == declared, exported ^ declared
    assert lib.qd_abi_version() == 1 == _lib.C["QD_ABI_VERSION"]
    h = _header()
    for s in _lib.SYMBOLS:
        n_params = re.search(rf"\b{s}\s*\(([^)]*)\)", h).group(1)
        n_params = 0 if n_params.strip() == "void" else n_params.count(",") + 1
        assert len(getattr(lib, s).argtypes) == n_params == len(_lib.PROTOTYPES[s][1]), s
        assert getattr(lib, s).restype is (ctypes.c_char_p if s == "qd_last_error" else ctypes.c_int), s


# ---------------------------------------------------------------- layout and values against a compiler
_KIND = {"d": "double", "i": "int32", "l": "int64", "q": "int64", "P": "other"}


def _leaf(t, expr):
    while issubclass(t, ctypes.Array):
        t, expr = t._type_, expr + "[0]"
    return _KIND[t._type_] if isinstance(getattr(t, "_type_", None), str) else "other", expr


def test_layout_and_constants_match_the_compiler(tmp_path):
    """sizeof, offsetof, member size and element type of every derived struct field, and the value of every derived constant and
    enumerator, as the host C compiler has them from the same header."""
    from qingdai_amd import _lib
    assert set(re.findall(r"typedef\s+struct\s+(\w+)\s*\{", _header())) == set(_lib.HEADER.structs) and len(_lib.HEADER.structs) == 13
    assert set(re.findall(r"\bQD_[A-Z0-9_]+\b", _header())) == set(_lib.C)          # every constant the header spells, and no other
    lines, want = [], []
    for name, cls in _lib.HEADER.structs.items():
        assert getattr(_lib, name) is cls
        lines.append(f'printf("S {name} %zu\\n", sizeof({name}));')
        want.append(f"S {name} {ctypes.sizeof(cls)}")
        for f, t in cls._fields_:
            kind, leaf = _leaf(t, f"(({name}*)0)->{f}")
            lines.append(f'printf("F {name}.{f} %zu %zu %s\\n", offsetof({name}, {f}), sizeof((({name}*)0)->{f}), KIND({leaf}));')
            want.append(f"F {name}.{f} {getattr(cls, f).offset} {getattr(cls, f).size} {kind}")
    for name, v in _lib.C.items():
        lines.append(f'printf("C {name} %lld\\n", (long long){name});')
        want.append(f"C {name} {v}")
    src = tmp_path / "abi.c"
    src.write_text('#include <stdio.h>\n#include "qingdai_hip.h"\n'
                   '#define KIND(x) _Generic((x), double: "double", int: "int32", long: "int64", long long: "int64", default: "other")\n'
                   "int main(void) {\n" + "\n".join(lines) + "\nreturn 0;\n}\n")
    cc = _tool("CC", "cc", "clang")
    subprocess.run([cc, "-std=c11", "-I", INCLUDE, str(src), "-o", str(tmp_path / "abi")], check=True)
    got = subprocess.run([str(tmp_path / "abi")], check=True, capture_output=True, text=True).stdout.split("\n")[:-1]
    assert got == want, [(g, w) for g, w in zip(got, want) if g != w][:10]
    assert ctypes.sizeof(_lib.qd_params) == 1016 and ctypes.sizeof(_lib.qd_eco_params) == 6 * 8 + 6 * 4


def test_field_ids_match_header():
    from qingdai_amd import _lib
    h = _header()
    ids = re.findall(r"QD_F_([A-Z0-9_]+)", h[h.index("enum qd_field {"):h.index("QD_F_COUNT_F64")])
    assert ids == _lib.FIELDS and [_lib.F[n] for n in ids] == list(range(_lib.C["QD_F_COUNT_F64"]))
    assert set(_lib.F) - set(ids) == {"LAND_MASK", "ICE_MASK", "ECO_DIV_LS", "ECO_DIV_ALPHA", "ECO_DIV_BC", "ECO_DIV_SUMMARY"}
    assert (_lib.R_SUM, _lib.R_COSMEAN, _lib.R_MAX, _lib.R_MIN, _lib.R_MAXABS) == (0, 1, 2, 3, 4)
    assert _lib.TILE_SOURCES == tuple(_lib.TILE) and list(_lib.TILE.values()) == list(range(9)) and _lib.TILE["HOST_PLANE"] == 8
    assert _lib.STEP_BITS == ("with_ocean", "with_physics", "pass_albedo", "with_hydrology", "energy_diag", "ecology", "phyto", "routing",
                              "phyto_daily", "eco_daily")
    assert [_lib.step_flags(**{k: True}) for k in _lib.STEP_BITS] == [1 << k for k in range(10)]
    assert _lib.step_flags(with_ocean=True, routing=1, phyto=0) == 129
    # the numbers the library's own sources use come from the same header: no second definition, no bare flag literal
    csrc = os.path.join(ROOT, "qingdai_amd", "csrc")
    for f in os.listdir(csrc):
        if f.endswith((".hip", ".h")):
            assert not re.search(r"#\s*define\s+(QD_SPAN_LOG_CAP|QD_ROUTE_LOG_W)\b", open(os.path.join(csrc, f)).read()), f
    step_n = open(os.path.join(csrc, "qd_api.hip")).read()
    step_n = step_n[step_n.index('extern "C" int qd_step_n'):]
    assert not re.search(r"\bflags\s*&\s*\d", step_n) and step_n.count("flags & QD_STEP_") == 10


def test_step_form_tallies_close_the_enum():
    """qd_step_forms: the tallies since qd_create (QD_SF_CNT_* / QD_SF_MAX_*) are the last enumerators before QD_SF_N, behind the
    QD_SF_LAST_* notes -- the report's older entries keep their places -- and Device.step_forms names every entry from the header."""
    from qingdai_amd import _lib
    sf = sorted((v, k) for k, v in _lib.C.items() if k.startswith("QD_SF_"))
    assert [v for v, _ in sf] == list(range(len(sf))) and sf[-1] == (_lib.C["QD_SF_N"], "QD_SF_N")
    names = [k for _, k in sf[:-1]]
    tallies = ["QD_SF_CNT_DYN_STREAM", "QD_SF_CNT_DYN_TILE", "QD_SF_CNT_OCN_STREAM", "QD_SF_CNT_OCN_TILE", "QD_SF_CNT_SPLIT", "QD_SF_CNT_SPLIT_REDO",
               "QD_SF_CNT_STREAM_PAIR", "QD_SF_CNT_STREAM_PUSH", "QD_SF_CNT_SUB_BAND_TAIL", "QD_SF_CNT_SUB_ROUND2", "QD_SF_MAX_TAIL_SEGS",
               "QD_SF_MAX_MOM_SEGS", "QD_SF_CNT_TAIL_FIX", "QD_SF_CNT_DYN_TILE_FAST", "QD_SF_CNT_OCN_TILE_FAST", "QD_SF_CNT_TILE_EXACT",
               "QD_SF_CNT_TILE_SHIFT", "QD_SF_CNT_TILE_SLAB_EDGE"]
    assert names[-len(tallies):] == tallies and names[-len(tallies) - 1] == "QD_SF_LAST_OCN_FORM"
    assert _lib.C["QD_SF_DYN_STREAM"] == 0 and _lib.C["QD_SF_LAST_NSUB"] == 27 and _lib.C["QD_SF_CNT_DYN_STREAM"] == 36
    assert not [k for k in names if k.startswith(("QD_SF_CNT_", "QD_SF_MAX_")) and k not in tallies]


# ---------------------------------------------------------------- the reader, on small header texts
_TYPES = '''
#define QD_N 4
#define QD_M QD_N            /* an earlier constant */
enum { QD_A = 1, QD_B = 2, QD_C = 0x10 };
enum qd_run { QD_RUN_0, QD_RUN_1, QD_RUN_7 = 7, QD_RUN_8, QD_RUN_N = QD_N, QD_RUN_5 };   // running, with jumps
typedef struct qd_in { int32_t a, b; double x; } qd_in;
typedef struct qd_out {
    qd_in cell[QD_N];          /* a nested struct array */
    double rgb[QD_M][3];
    int64_t mark[2];
    const uint8_t* mask;
} qd_out;
typedef struct qd_ctx* qd_handle;
'''


def test_reader_constants_enums_and_structs():
    from qingdai_amd._lib import parse_header
    h = parse_header(_TYPES)
    assert h.constants == {"QD_N": 4, "QD_M": 4, "QD_A": 1, "QD_B": 2, "QD_C": 16, "QD_RUN_0": 0, "QD_RUN_1": 1, "QD_RUN_7": 7,
                           "QD_RUN_8": 8, "QD_RUN_N": 4, "QD_RUN_5": 5}
    assert list(h.structs) == ["qd_in", "qd_out"] and not h.prototypes
    qd_in, qd_out = h.structs["qd_in"], h.structs["qd_out"]
    assert qd_in._fields_ == [("a", ctypes.c_int32), ("b", ctypes.c_int32), ("x", ctypes.c_double)] and ctypes.sizeof(qd_in) == 16
    assert [n for n, _ in qd_out._fields_] == ["cell", "rgb", "mark", "mask"]
    t = dict(qd_out._fields_)
    assert t["cell"]._type_ is qd_in and t["cell"]._length_ == 4
    assert t["rgb"]._length_ == 4 and t["rgb"]._type_._length_ == 3 and t["rgb"]._type_._type_ is ctypes.c_double      # rgb[4][3]
    assert t["mark"]._type_ is ctypes.c_int64 and t["mark"]._length_ == 2 and t["mask"] is ctypes.c_void_p
    assert (qd_out.cell.offset, qd_out.rgb.offset, qd_out.mark.offset, qd_out.mask.offset, ctypes.sizeof(qd_out)) == (0, 64, 160, 176, 184)
    o = qd_out()
    o.rgb[3][2], o.cell[1].x = 0.5, 2.0
    assert o.rgb[3][2] == 0.5 and o.cell[1].x == 2.0
    assert (qd_in(1, 2, 3.0).x, qd_in(b=5).b) == (3.0, 5)                      # positional and keyword construction


def test_reader_prototypes():
    from qingdai_amd._lib import parse_header
    vp, i, d = ctypes.c_void_p, ctypes.c_int, ctypes.c_double
    h = parse_header(_TYPES + '''
int qd_version(void);
const char* qd_error(qd_handle h);   /* NULL allowed */
int qd_broken(qd_handle h, const double* F,
              int n, double* out);
int qd_wide(qd_handle h, int64_t steps, size_t bytes, int32_t k, long long* wrong, long long big, double dt);
int qd_arrays(qd_handle h, const double star[3], double out[10], const int32_t* fire, const uint8_t* mask, uint64_t* digest);
int qd_make(const qd_in* desc, qd_out* result, qd_handle* out, void** ring, qd_handle* handles, const char* name, const void* raw);
''')
    assert list(h.prototypes) == ["qd_version", "qd_error", "qd_broken", "qd_wide", "qd_arrays", "qd_make"]
    assert h.prototypes["qd_version"] == (i, [])
    assert h.prototypes["qd_error"] == (ctypes.c_char_p, [vp])
    assert h.prototypes["qd_broken"] == (i, [vp, vp, i, vp])                   # a prototype broken over two lines
    assert h.prototypes["qd_wide"] == (i, [vp, ctypes.c_int64, ctypes.c_size_t, ctypes.c_int32, vp, ctypes.c_longlong, d])
    assert h.prototypes["qd_arrays"] == (i, [vp] * 6)                          # arrays and every plain pointer: void pointers
    p = ctypes.POINTER
    assert h.prototypes["qd_make"][1][1:] == [vp, p(vp), p(vp), p(vp), ctypes.c_char_p, vp]
    assert h.prototypes["qd_make"][1][0] is p(h.structs["qd_in"])             # const qd_X*: a pointer to the derived struct
    # what the header says of each parameter: (name, kind, base type, is_const)
    assert h.signatures["qd_version"] == [] and list(h.signatures) == list(h.prototypes)
    assert h.signatures["qd_arrays"] == [("h", "handle", "qd_handle", False), ("star", "array", "double", True), ("out", "array", "double", False),
                                         ("fire", "array", "int32_t", True), ("mask", "array", "uint8_t", True), ("digest", "array", "uint64_t", False)]
    assert [s[1] for s in h.signatures["qd_make"]] == ["struct_ptr", "void_ptr", "handle_out", "handle_out", "handle_out", "cstring", "void_ptr"]
    from qingdai_amd._lib import NP_OF, _C_OF, SIGNATURES as S                # one pinned entry per kind, from the real header
    assert S["qd_step_n"] == [("h", "handle", "qd_handle", False), ("n", "scalar", "int", False), ("dt", "scalar", "double", False),
                              ("flags", "scalar", "int", False), ("stars", "array", "double", True)]
    assert S["qd_tiles_scan"][1] == ("refs", "struct_ptr", "qd_tile_ref", True) and S["qd_tiles_scan"][4] == ("argmax_cell", "array", "int64_t", False)
    assert S["qd_eco_state_restore"][1] == ("lai", "void_ptr", "void", True)
    assert S["qd_timing_select"][1] == ("name", "cstring", "char", True)
    assert S["qd_create"][3] == ("out", "handle_out", "qd_handle", False) and S["qd_create"][2] == ("q_init_rh", "scalar", "double", False)
    assert set(NP_OF) == set(_C_OF) and all(np.dtype(NP_OF[b]) == np.dtype(t) for b, t in _C_OF.items())


@pytest.mark.parametrize("text, names", [
    ("int qd_f(qd_handle h, unsigned n);", ("unsigned", "qd_f")),               # an unknown type word: never a silent int
    ("int qd_f(qd_handle h, float x);", ("float", "qd_f")),
    ("int qd_f(qd_handle h, const qd_nope* p);", ("qd_nope", "qd_f")),
    ("float qd_f(qd_handle h);", ("float", "qd_f")),
    ("int qd_f(qd_handle h, qd_in by_value);", ("qd_in", "qd_f")),
    ("typedef struct qd_s { int32_t a; short b; } qd_s;", ("short", "qd_s")),
    ("typedef struct qd_s { double v[QD_MISSING]; } qd_s;", ("QD_MISSING", "qd_s")),
    ("int qd_f(qd_handle h, unsigned long n);", ("unsigned long n", "qd_f")),   # declarations the reader cannot parse
    ("int qd_f(qd_handle h, int (*cb)(int));", ("qd_f",)),
    ("int qd_f(qd_handle h, int n;", ("qd_f",)),
    ("int qd_global;", ("qd_global",)),
    ("qd_f(qd_handle h);", ("qd_f",)),
    ("#define QD_W (4)", ("QD_W",)),
    ("enum { QD_X = 1 << 3 };", ("QD_X",)),
    ("enum { QD_X = QD_LATER };\n#define QD_LATER 1", ("QD_LATER", "QD_X")),
    ("int qd_f(qd_handle h, int);", ("name", "qd_f")),                          # a parameter without a name: the seam's errors name it
])
def test_reader_is_strict(text, names):
    from qingdai_amd._lib import QdError, parse_header
    with pytest.raises(QdError) as e:
        parse_header("typedef struct qd_ctx* qd_handle;\ntypedef struct qd_in { int32_t a; } qd_in;\n" + text)
    assert all(n in str(e.value) for n in names), str(e.value)


# ---------------------------------------------------------------- params.py against the derived struct
def test_param_struct_layout_matches_header(monkeypatch):
    """The tables of params.py name exactly the derived struct's fields with its types; QdParams fills the struct by name, whatever
    the order of the tables (the layout itself: test_layout_and_constants_match_the_compiler)."""
    from qingdai_amd import _lib, params
    assert params.qd_params is _lib.qd_params
    table = [(n, ctypes.c_double) for n, _, _ in params._DOUBLES] + [(n, ctypes.c_int32) for n, _, _ in params._INTS]
    assert len(dict(table)) == len(table) == len(_lib.qd_params._fields_) and dict(table) == dict(_lib.qd_params._fields_)
    s = params.QdParams(g=3.5, orog_enable=1, seaice_enabled=0).to_struct()
    assert (s.g, s.orog_enable, s.seaice_enabled, s.H) == (3.5, 1, 0, 8000.0)
    for broken in (params._DOUBLES[1:], params._DOUBLES + [("extra", None, 0.0)], params._DOUBLES[:-1] + [params._DOUBLES[0]]):
        monkeypatch.setattr(params, "_DOUBLES", broken)
        with pytest.raises(_lib.QdError, match="differ"):
            params._check_tables()
    monkeypatch.undo()
    monkeypatch.setattr(params, "_INTS", params._INTS[:-1] + [("g", None, 0)])          # a double listed as an int
    with pytest.raises(_lib.QdError, match="differ"):
        params._check_tables()


def test_product_defaults_equal_oracle_defaults():
    import qd_oracle as qo
    from qingdai_amd import QdParams
    o = qo.defaults()
    p = QdParams().as_oracle_kwargs()
    for k, v in vars(o).items():
        assert k in p, k
        pv = p[k]
        if isinstance(v, float) and v != v:
            assert pv != pv, k
        else:
            assert pv == v, (k, pv, v)


def test_env_parsing(monkeypatch):
    from qingdai_amd import QdParams
    monkeypatch.setenv("QD_MOM_SCHEME", "primitive")
    monkeypatch.setenv("QD_FILTER_TYPE", "hyper4")
    monkeypatch.setenv("QD_ENERGY_W", "1")
    monkeypatch.setenv("QD_OCEAN_OUTLIER", "clamp")
    monkeypatch.setenv("QD_K4_U", "1e14")
    p = QdParams.from_env()
    assert (p.mom_scheme, p.filter_type, p.energy_w, p.ocean_outlier, p.k4_u) == (1, 1, 1.0, 1, 1e14)
    assert p.k4_v != p.k4_v and p.pcond_ref != p.pcond_ref      # unset -> NaN


def test_no_gpu_fails_loudly():
    """Without a GPU the product must raise, never fall back."""
    from conftest import _gpu_visible
    if _gpu_visible():
        pytest.skip("GPU present")
    import qingdai_amd as qa
    from qingdai_amd._lib import QdError
    g = qa.SphericalGrid(19, 36)
    with pytest.raises(QdError):
        qa.SpectralModel(g, np.zeros((19, 36)), land_mask=np.zeros((19, 36), dtype=np.uint8))


def test_topography_seed42_fingerprint():
    import hashlib
    import qd_oracle as qo
    from qingdai_amd.topography import create_land_sea_mask
    m = create_land_sea_mask(qo.Grid(181, 360))
    assert int(m.sum()) == 16242
    assert hashlib.sha1(m.tobytes()).hexdigest().startswith("17de315c9bb5")
