"""CPU: the host reference of the state digest (tests/state_digest_ref.py) -- fixed vectors whose values were worked out term by
term with Python integers, additivity over row blocks with global indices, and sensitivity to every kind of bit change the digest
exists to see.  The name -> ref mapping of the binding and the ids of the header are checked along."""
import os
import re

import numpy as np
import pytest

import state_digest_ref as ref

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
M = (1 << 64) - 1


def _mix(z):                                                  # Python integers, no NumPy: a second statement of mix64
    z ^= z >> 30
    z = (z * 0xBF58476D1CE4E5B9) & M
    z ^= z >> 27
    z = (z * 0x94D049BB133111EB) & M
    z ^= z >> 31
    return z


def _digest_int(ws, i0=0):
    return sum(_mix((w + (i0 + i + 1) * 0x9E3779B97F4A7C15) & M) for i, w in enumerate(ws)) & M


def test_fixed_vectors_cpu():
    nan1 = np.array([0x7FF8000000000001], dtype=np.uint64).view(np.float64)[0]
    f64 = np.array([1.0, -0.0, nan1])
    # the three terms: mix64(bits + (i + 1) * 0x9E3779B97F4A7C15)
    assert [int(t) for t in ref.mix64(ref.words(f64) + np.arange(1, 4, dtype=np.uint64) * ref.GOLD)] == \
        [0x88D7C35BBBF3EDED, 0xC46FA638A6309012, 0xB19E265982B03DDC]
    assert ref.digest(f64) == 0xFEE58FEDE4D4BBDB
    assert ref.digest(np.array([1.5, -2.0], dtype=np.float32)) == 0x65D78B4D3E7BE2A3
    assert ref.digest(np.array([0, 255, 7], dtype=np.uint8)) == 0xB83DA26261FB84C6
    assert ref.digest(np.zeros(0)) == 0 and ref.digest(np.zeros(1)) == 0xE220A8397B1DCDAF      # the index alone carries a zero
    assert ref.fnv1a64("") == 0xCBF29CE484222325 and ref.fnv1a64("run") == 0x89B2A81960C55A4A
    assert ref.run_digest({"U": 1, "V": 2}) == 0xDBE2C9AF0D148EA4 == ref.run_digest({"V": 2, "U": 1})


@pytest.mark.parametrize("dtype", [np.float64, np.float32, np.uint8])
def test_agrees_with_python_integers_cpu(dtype):
    rng = np.random.default_rng(11)
    size = np.dtype(dtype).itemsize
    raw = rng.integers(0, 256, 997 * size, dtype=np.uint8)
    a = raw.view(dtype)
    ws = [int.from_bytes(raw[k * size:(k + 1) * size].tobytes(), "little") for k in range(997)]
    assert ref.digest(a) == _digest_int(ws)
    assert ref.digest(a[100:], index0=100) == _digest_int(ws[100:], 100)


def test_additive_over_row_blocks_cpu():
    rng = np.random.default_rng(3)
    a = rng.integers(0, 2**64, (37, 73), dtype=np.uint64).view(np.float64)
    whole = ref.digest(a)
    for cuts in ([0, 37], [0, 1, 37], [0, 5, 6, 20, 37]):
        parts = sum(ref.digest(a[r0:r1], index0=r0 * 73) for r0, r1 in zip(cuts[:-1], cuts[1:])) & M
        assert parts == whole, cuts
    assert sum(ref.digest(a[r0:r1]) for r0, r1 in ((0, 5), (5, 37))) & M != whole        # local indices would not add up


def test_sensitive_to_every_bit_change_cpu():
    rng = np.random.default_rng(4)
    a = rng.standard_normal((19, 36))
    a[3, 4], a[7, 7] = 0.0, np.nan
    base = ref.digest(a)

    def changed(fn):
        b = a.copy()
        fn(b)
        return ref.digest(b)
    def flip_lowest(b):
        b.view(np.uint64)[5, 6] ^= np.uint64(1)
    def minus_zero(b):
        b[3, 4] = -0.0
    def other_nan(b):
        b.view(np.uint64)[7, 7] ^= np.uint64(0x10)
    def swap(b):
        b[0, 0], b[0, 1] = a[0, 1], a[0, 0]
    seen = {base}
    for fn in (flip_lowest, minus_zero, other_nan, swap):
        d = changed(fn)
        assert d not in seen, fn.__name__
        seen.add(d)
    assert np.isnan(a[7, 7]) and a[0, 0] != a[0, 1]
    # the element size is part of the plane: the same numbers as f32 are another digest
    assert ref.digest(a.astype(np.float32)) != base


def test_names_and_header_ids_cpu():
    from qingdai_amd import _lib
    # the ids and constants themselves against the header as a compiler reads it: tests/test_abi_cpu.py
    assert _lib.STATE_REFS == {"PHYTO_TRACER": 200, "ROUTE_BUFFER": 300, "ROUTE_FLOW": 301, "ROUTE_LAKES": 302, "ECO_LAI_STACK": 310,
                               "INDIV_E_DAY": 320, "INDIV_STRESS": 321, "HISTORY_SUM": 400}
    assert _lib.STATE_REF_COUNT == {"PHYTO_TRACER": 64, "HISTORY_SUM": _lib.HISTORY_MAX_ENTRIES}
    from qingdai_amd import checkpoint
    assert _lib.C["QD_ABI_VERSION"] == checkpoint.ABI_VERSION == _lib.load().qd_abi_version()
    assert checkpoint.abi_version(type("D", (), {"lib": _lib.load()})()) == checkpoint.ABI_VERSION
    # the slots are enum qd_state_scalar of the header, and qd_digest.hip reads and writes them by those names only
    assert (_lib.C["QD_SS_PHYTO_DAILY_STEPS"], _lib.C["QD_SS_ECO_DAILY_FIRED"], _lib.C["QD_SS_INDIV_DAILY_FIRED"], _lib.C["QD_SS_LAST_NSUB"]) == (17, 18, 19, 20)
    slots = open(os.path.join(ROOT, "qingdai_amd", "csrc", "qd_digest.hip")).read()
    assert "17 daily phytoplankton steps   18 daily vegetation firings   19 firings of the individuals' daily step   20 last_nsub" in slots
    slots = slots[slots.index('extern "C" int qd_state_scalars_get'):]
    assert not re.search(r"\b(in|out)\[\d+\]", slots) and slots.count("QD_SS_PHYTO_DAILY_STEPS") == 2
    assert (_lib.STATE_SCALAR_SLOT["phyto_daily_steps"], _lib.STATE_SCALAR_SLOT["eco_daily_fired"], _lib.STATE_SCALAR_SLOT["indiv_daily_fired"]) == (17, 18, 19)
    assert (_lib.STATE_SCALAR_SLOT["cloud_eff_valid"], _lib.STATE_SCALAR_SLOT["has_elevation"], _lib.STATE_SCALAR_SLOT["last_nsub"]) == (0, 1, 20)
    assert len(_lib.STATE_SCALAR_SLOT) == 22 and max(_lib.STATE_SCALAR_SLOT.values()) + 10 < _lib.STATE_SCALARS_N
    assert _lib.state_ref("U") == 0 and _lib.state_ref("ICE_MASK") == 101 and _lib.state_ref("ROUTE_LAKES") == 302
    assert _lib.state_ref("PHYTO_TRACER:3") == 203 and _lib.state_ref("HISTORY_SUM:31") == 431
    for bad in ("PHYTO_TRACER", "PHYTO_TRACER:64", "HISTORY_SUM:32", "ROUTE_FLOW:1", "NOPE", "ECO_DIV_LS"):
        with pytest.raises(KeyError, match="names no resident plane"):
            _lib.state_ref(bad)
