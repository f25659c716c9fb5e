"""CPU: the one call seam of the C ABI, _lib.call / Device.call, around a fake library (no GPU, no libqingdai_hip.so): one Python
callable per symbol, which records what it was handed and reads or writes the memory behind the addresses through ctypes.  The
signatures are the real header's.  Then the product itself: every literal call site names a declared symbol with the declared
number of arguments, and nothing reaches the library past the seam."""
import ast
import ctypes
import glob
import os
import re

import numpy as np
import pytest

from qingdai_amd import _lib
from qingdai_amd._lib import OUT, QdError
from qingdai_amd.device import Device

PKG = os.path.join(os.path.dirname(os.path.abspath(__file__)), "..", "qingdai_amd")
DP, I64P = ctypes.POINTER(ctypes.c_double), ctypes.POINTER(ctypes.c_int64)


def addr(p):
    """What the seam hands over for a pointer: None, an address or a ctypes pointer / array -> the address (0 for NULL)"""
    return 0 if p is None else p if isinstance(p, int) else ctypes.cast(p, ctypes.c_void_p).value or 0


def doubles(p, n):
    return np.ctypeslib.as_array(ctypes.cast(addr(p), DP), shape=(n,)).copy()


class FakeLib:
    """fns: {symbol: callable(*args) -> rc or None}.  Every call is recorded before the callable runs."""

    def __init__(self, **fns):
        self.fns, self.calls, self.error = fns, [], b"the programmed error"

    def __getattr__(self, name):
        if name not in self.fns:
            raise AttributeError(name)

        def fn(*args):
            self.calls.append((name, args))
            return self.fns[name](*args) or 0
        return fn

    def qd_last_error(self, h):
        return self.error


def device(**fns):
    dev = object.__new__(Device)
    dev.lib, dev.h, dev._host, dev.shape = FakeLib(**fns), ctypes.c_void_p(1), {}, (3, 4)
    return dev


# ---------------------------------------------------------------- 1. inputs
VALUES = np.arange(12, dtype=np.float64).reshape(3, 4) * 0.5 - 1.0        # exact in float32 too


@pytest.mark.parametrize("form", ["float32", "fortran", "strided", "list"])
def test_input_arrives_as_contiguous_float64(form):
    x = {"float32": VALUES.astype(np.float32), "fortran": np.asfortranarray(VALUES), "strided": np.repeat(VALUES, 2, axis=1)[:, ::2],
         "list": VALUES.tolist()}[form]
    assert form == "list" or x.dtype != np.float64 or not x.flags.c_contiguous
    before = [list(r) for r in x] if form == "list" else (x.copy(), x.dtype, x.strides)
    seen = []
    dev = device(qd_op_laplacian=lambda h, F, kind, out: seen.append(doubles(F, 12)))        # read while the call is in progress
    out = np.empty((3, 4))
    assert dev.call("qd_op_laplacian", x, 0, out) is None
    assert np.array_equal(seen[0], VALUES.ravel())
    assert (x == before) if form == "list" else (np.array_equal(x, before[0]) and (x.dtype, x.strides) == before[1:])
    (_, (h, F, kind, o)), = dev.lib.calls
    assert h is dev.h and kind == 0 and type(kind) is int and addr(o) == out.ctypes.data


# ---------------------------------------------------------------- 2. outputs
@pytest.mark.parametrize("form", ["float32", "strided", "readonly", "list"])
def test_unfit_output_is_refused_before_the_call(form):
    out = {"float32": np.empty((3, 4), dtype=np.float32), "strided": np.empty((3, 8))[:, ::2],
           "readonly": np.broadcast_to(np.zeros(4), (3, 4)), "list": [0.0] * 12}[form]
    dev = device(qd_op_laplacian=lambda *a: 0)
    with pytest.raises(TypeError, match=r"qd_op_laplacian: out: ") as e:
        dev.call("qd_op_laplacian", VALUES, 0, out)
    assert dev.lib.calls == [], str(e.value)


def test_ctypes_outputs_pass():
    def fill(h, out):
        ctypes.cast(addr(out), DP)[9] = 4.5
    dev = device(qd_energy_diagnostics=fill, qd_reduce=lambda h, f, op, out: ctypes.cast(addr(out), DP).__setitem__(0, 2.5))
    arr, one = (ctypes.c_double * 10)(), ctypes.c_double(0.0)
    assert dev.call("qd_energy_diagnostics", arr) is None and arr[9] == 4.5
    assert dev.call("qd_reduce", 3, 1, one) is None and one.value == 2.5
    with pytest.raises(TypeError, match="qd_reduce: out: "):
        dev.call("qd_reduce", 3, 1, ctypes.c_float(0.0))
    with pytest.raises(TypeError, match="qd_energy_diagnostics: out: "):
        dev.call("qd_energy_diagnostics", (ctypes.c_int64 * 10)())


# ---------------------------------------------------------------- 3. OUT
def test_out_marker():
    def store(p, typ, *vals):
        q = ctypes.cast(addr(p), typ)
        for k, v in enumerate(vals):
            q[k] = v
    dev = device(qd_eco_daily_state=lambda h, n: store(n, I64P, 7),
                 qd_energy_diagnostics=lambda h, out: store(out, DP, *range(10)),
                 qd_get_step_counter=lambda h, a, o: (store(a, I64P, 11), store(o, I64P, 22))[0],
                 qd_timing_get=lambda h, name, ms, n: (store(ms, DP, 0.25), store(n, I64P, 3))[0],
                 qd_stateframe_scan=lambda h, out, marks: (store(out, DP, 1.5), store(marks, I64P, 5, 6))[0])
    n = dev.call("qd_eco_daily_state", OUT)
    assert n == 7 and type(n) is int
    e = dev.call("qd_energy_diagnostics", OUT(10))
    assert isinstance(e, np.ndarray) and e.dtype == np.float64 and e.tolist() == [float(k) for k in range(10)]
    assert dev.call("qd_get_step_counter", OUT, OUT) == (11, 22)
    ms, cnt = dev.call("qd_timing_get", "k_x", OUT, OUT)
    assert (ms, cnt) == (0.25, 3) and type(ms) is float and type(cnt) is int
    out, marks = dev.call("qd_stateframe_scan", OUT(_lib.STATEFRAME_SCAN_N), OUT(2))
    assert out.shape == (_lib.STATEFRAME_SCAN_N,) and out[0] == 1.5 and marks.dtype == np.int64 and marks.tolist() == [5, 6]
    assert dev.counters() == (11, 22) and dev.eco_daily_firings() == 7 and dev.timing_get("k_x") == (0.25, 3)


# ---------------------------------------------------------------- 4. pass-through
def test_none_struct_and_string_pass_through():
    seen = {}
    dev = device(qd_eco_daily_step=lambda h, soil: seen.update(soil=soil),
                 qd_eco_configure=lambda h, p, size: seen.update(k=p.contents.k_canopy, size=size),
                 qd_timing_select=lambda h, name: seen.update(name=name),
                 qd_eco_state_restore=lambda h, lai, f32, w, ns, nl, mx: seen.update(lai=lai, f32=f32, w=doubles(w, 2), mx=mx))
    dev.call("qd_eco_daily_step", None)
    assert seen["soil"] is None
    p = _lib.qd_eco_params(k_canopy=0.625)
    dev.call("qd_eco_configure", p, ctypes.sizeof(p))
    assert seen["k"] == 0.625 and seen["size"] == ctypes.sizeof(_lib.qd_eco_params)
    with pytest.raises(TypeError, match="qd_eco_configure: p: "):
        dev.call("qd_eco_configure", _lib.qd_grid_desc(), 8)
    dev.call("qd_timing_select", "k_ocn:4")
    assert seen["name"] == b"k_ocn:4"
    dev.call("qd_timing_select", b"raw")
    assert seen["name"] == b"raw"
    lai = np.ones((3, 4), dtype=np.float32)                          # const void*: any dtype, by its address
    dev.call("qd_eco_state_restore", lai, np.bool_(True), (0.25, 0.75), np.int64(2), 1, np.float32(2.0))
    assert seen["lai"] == lai.ctypes.data and seen["f32"] == 1 and type(seen["f32"]) is int and seen["w"].tolist() == [0.25, 0.75]
    assert seen["mx"] == 2.0 and type(seen["mx"]) is float
    with pytest.raises(TypeError, match="qd_eco_state_restore: lai: "):
        dev.call("qd_eco_state_restore", np.ones((3, 8), dtype=np.float32)[:, ::2], 1, (1.0,), 1, 1, 2.0)
    dev2 = device(qd_download=lambda *a: 0)
    with pytest.raises(TypeError, match="qd_download: host_global: "):   # void*, not const: the array must be writeable
        dev2.call("qd_download", 0, np.broadcast_to(np.zeros(4), (3, 4)), 96)
    assert dev2.lib.calls == []


# ---------------------------------------------------------------- 5. errors
class OtherError(RuntimeError):
    pass


def test_argument_count_and_return_code():
    dev = device(qd_sync=lambda h: -3, qd_reduce=lambda *a: 0)
    with pytest.raises(TypeError, match=r"qd_reduce takes 4 arguments, 3 were given"):
        dev.call("qd_reduce", 1, 2)
    assert dev.lib.calls == []
    with pytest.raises(QdError) as e:
        dev.call("qd_sync")
    assert str(e.value) == "qd_sync failed: the programmed error"
    with pytest.raises(OtherError) as e:
        dev.call("qd_sync", error=OtherError)
    assert str(e.value) == "qd_sync failed: the programmed error"
    with pytest.raises(QdError) as e:
        dev.call("qd_sync", what="qd_download(TS)")
    assert str(e.value) == "qd_download(TS) failed: the programmed error"
    dev.lib.error = None
    with pytest.raises(QdError) as e:
        _lib.call(dev.lib, "qd_sync", (dev.h,), last_error=lambda: None)
    assert str(e.value) == "qd_sync failed: ?"


# ---------------------------------------------------------------- 6. every literal call site against the header
def call_sites():
    """(file:line, symbol node, positional argument nodes, arguments the seam adds) of every x.call(...) and _lib.call(...); the one
    site left out is Device.call's own forwarding line"""
    forwards = 0
    for path in sorted(glob.glob(os.path.join(PKG, "*.py"))):
        for node in ast.walk(ast.parse(open(path, encoding="utf-8").read())):
            if not (isinstance(node, ast.Call) and isinstance(node.func, ast.Attribute) and node.func.attr == "call"):
                continue
            where = f"{os.path.basename(path)}:{node.lineno}"
            if isinstance(node.func.value, ast.Name) and node.func.value.id == "_lib":        # _lib.call(lib, symbol, (args), ...)
                if os.path.basename(path) == "device.py" and isinstance(node.args[1], ast.Name) and node.args[1].id == "symbol":
                    forwards += 1
                    continue
                assert isinstance(node.args[2], (ast.Tuple, ast.List)), where
                yield where, node.args[1], node.args[2].elts, 0
            elif isinstance(node.func.value, ast.Name) and node.func.value.id == "Device":     # Device.call(dev, symbol, ...)
                yield where, node.args[1], node.args[2:], 1
            else:
                yield where, node.args[0], node.args[1:], 1
    assert forwards == 1


def test_every_call_site_matches_the_header():
    sites = list(call_sites())
    assert len(sites) > 120
    for where, sym, args, added in sites:
        assert isinstance(sym, ast.Constant) and isinstance(sym.value, str), f"{where}: the symbol is not a literal"
        assert sym.value in _lib.SIGNATURES, f"{where}: {sym.value} is not declared in include/qingdai_hip.h"
        assert not any(isinstance(a, ast.Starred) for a in args), f"{where}: a *splat hides the argument count"
        assert len(args) + added == len(_lib.SIGNATURES[sym.value]), f"{where}: {sym.value} takes {len(_lib.SIGNATURES[sym.value])} arguments"


# ---------------------------------------------------------------- 7. no bypass
def test_nothing_reaches_the_library_past_the_seam():
    allowed = {"device.py": ("qd_create", "qd_destroy")}              # no handle yet / the handle's end; _chk names no symbol
    for path in sorted(glob.glob(os.path.join(PKG, "*.py"))):
        name = os.path.basename(path)
        if name == "_lib.py":
            continue
        for n, line in enumerate(open(path, encoding="utf-8"), 1):
            for sym in re.findall(r"\.lib\.(qd_\w+)", line):
                assert sym == "qd_last_error" or sym in allowed.get(name, ()), f"{name}:{n}: {sym} is called past the seam"
            assert "._chk(" not in line, f"{name}:{n}: the product checks a return code by hand"
