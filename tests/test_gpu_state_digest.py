"""GPU (-m gpu): Device.digest against the host reference (tests/state_digest_ref.py), exactly -- the digest is integer arithmetic
and has one answer.  Every f64 field, both masks and the ecology's f32 maps (QD_ECO_F32=1) in ONE call, on planes filled with random
bit patterns (NaN payloads, infinities, denormals, both zeros), at
    5 x 8      40 cells: fewer than a wave, an even pair count of 20 and u8 planes shorter than a workgroup
    19 x 36    the suite's small grid
    37 x 73    an odd cell count: the scalar tail, and 1350 pairs + 1
    181 x 360  more cells than one pass of the grid (52 entries share 8 workgroups per CU): the stride loop turns
and the planes without a field id (tracers, whose slabs start 8 bytes off a 16-byte boundary at an odd stride; history sums; the
routing buffers; the LAI stack; the individuals' buffers) where their subsystem is configured, and the refusals where it is not."""
import os

import numpy as np
import pytest

import state_digest_ref as ref

pytestmark = pytest.mark.gpu

F32_MAPS = ("ECO_LAI", "ECO_LAI_SNAP", "ECO_F", "ECO_ALPHA", "ECO_ALPHA_BANDED")


def _clean_env(monkeypatch, env=None):
    for k in [k for k in os.environ if k.startswith(("QD_ECO_", "QD_PHYTO_"))]:
        monkeypatch.delenv(k)
    for k, v in (env or {}).items():
        monkeypatch.setenv(str(k), str(v))


def _device(shape, monkeypatch, f32):
    import qingdai_amd as qa
    from qingdai_amd.device import Device
    from qingdai_amd.ecology import EcologyAdapter
    _clean_env(monkeypatch, {"QD_ECO_DIAG": "0", "QD_ECO_NS": "2"})
    grid = qa.SphericalGrid(*shape)
    dev = Device(grid)
    land = (np.random.default_rng(1).random(shape) < 0.4).astype(np.uint8)
    dev.upload_now("LAND_MASK", land)
    eco = EcologyAdapter(grid, land, dev=dev, albedo_couple=False, f32_maps=f32)
    return dev, eco


def _fill(dev, shape, seed, f32):
    """Random bit patterns into every field and both masks -> {name: the array whose stored bits the device holds}."""
    from qingdai_amd import _lib
    rng = np.random.default_rng(seed)
    want = {}
    for name in _lib.FIELDS:
        if f32 and name in F32_MAPS:                            # the slab stores f32(x): finite values, an infinity, both zeros
            a = rng.standard_normal(shape) * 10.0 ** rng.integers(-30, 30, shape)
            a.flat[:3] = (np.inf, 0.0, -0.0)
            want[name] = a.astype(np.float32)
        else:
            a = rng.integers(0, 2**64, shape, dtype=np.uint64).view(np.float64)
            a.flat[:6] = (np.nan, -np.nan, np.inf, -np.inf, 0.0, -0.0)
            want[name] = a
        dev.upload_now(name, a)
    for name in ("LAND_MASK", "ICE_MASK"):
        want[name] = rng.integers(0, 256, shape, dtype=np.uint8)
        dev.upload_now(name, want[name])
    return want


@pytest.mark.parametrize("shape", [(5, 8), (19, 36), (37, 73), (181, 360)], ids=lambda s: f"{s[0]}x{s[1]}")
def test_digest_equals_reference(gpu, shape, monkeypatch):
    dev, _eco = _device(shape, monkeypatch, f32=True)
    want = _fill(dev, shape, seed=shape[0], f32=True)
    names = list(want)
    assert len(names) == 52
    got = dev.digest(names)                                     # ONE call, one launch
    assert got.dtype == np.uint64 and got.shape == (52,)
    for n, g in zip(names, got):
        assert int(g) == ref.digest(want[n]), (n, hex(int(g)), hex(ref.digest(want[n])))
    assert np.array_equal(dev.digest(names), got)               # `out` is zeroed in front of every launch
    assert np.array_equal(dev.digest(names[::-1]), got[::-1])   # an entry's value does not depend on its row of the grid
    # one changed cell in the last element of the last entry: that digest moves, no other
    last = want[names[-1]].copy()
    last.flat[-1] ^= np.uint8(1)
    dev.upload_now(names[-1], last)
    again = dev.digest(names)
    assert np.array_equal(again[:-1], got[:-1]) and again[-1] != got[-1] and int(again[-1]) == ref.digest(last)
    # and the last f64 cell of an f64 plane, which an odd cell count leaves to the scalar tail
    u = want["U"].copy()
    u.view(np.uint64).flat[-1] ^= np.uint64(1)
    dev.upload_now("U", u)
    assert int(dev.digest(["U"])[0]) == ref.digest(u) != ref.digest(want["U"])
    dev.close()


def test_f64_maps_without_the_f32_switch(gpu, monkeypatch):
    dev, _eco = _device((19, 36), monkeypatch, f32=False)
    want = _fill(dev, (19, 36), seed=7, f32=False)
    got = dev.digest(list(F32_MAPS))
    assert [int(g) for g in got] == [ref.digest(want[n]) for n in F32_MAPS]
    assert all(want[n].dtype == np.float64 for n in F32_MAPS)
    dev.close()


def test_planes_without_a_field_id_and_refusals(gpu, monkeypatch):
    import qingdai_amd as qa
    from qingdai_amd._lib import QdError
    from qingdai_amd.device import Device
    from qingdai_amd.ecology import IndividualPool, PopulationDaily
    shape = (37, 73)                                            # odd cells: tracer s = 1 and history entry planes start off / on a 16-byte boundary
    dev, eco = _device(shape, monkeypatch, f32=False)
    for name, what in (("PHYTO_TRACER:0", "phytoplankton tracers are not configured"), ("ROUTE_BUFFER", "river routing is not configured"),
                       ("ECO_LAI_STACK", "daily vegetation step is not configured"), ("INDIV_E_DAY", "individuals are not configured"),
                       ("HISTORY_SUM:0", "history accumulators are not configured")):
        with pytest.raises(QdError, match=what):
            dev.digest(["U", name])
    rng = np.random.default_rng(9)
    # tracers
    dev.phyto_configure(3, 5.0e3, 0.7)
    C = rng.integers(0, 2**64, (3,) + shape, dtype=np.uint64).view(np.float64)
    dev.phyto_upload(C)
    got = dev.digest([f"PHYTO_TRACER:{s}" for s in range(3)])
    assert [int(g) for g in got] == [ref.digest(C[s]) for s in range(3)]
    with pytest.raises(QdError, match="PHYTO_TRACER \\+ 3: the species index is not below the tracer count"):
        dev.digest(["PHYTO_TRACER:3"])
    # history sums, restored and read back
    dev.history_configure([(0, "TS", None), (1, "U", "V"), (0, "H", None)])
    sums = rng.integers(0, 2**64, (3,) + shape, dtype=np.uint64).view(np.float64)
    dev.history_restore(sums, 17)
    back, count = dev.history_read()
    assert count == 17 and np.array_equal(back.view(np.uint64), sums.view(np.uint64))
    got = dev.digest([f"HISTORY_SUM:{k}" for k in range(3)])
    assert [int(g) for g in got] == [ref.digest(sums[k]) for k in range(3)]
    with pytest.raises(QdError, match="HISTORY_SUM \\+ 3: the entry index is not below the entry count"):
        dev.digest(["HISTORY_SUM:3"])
    # the LAI stack as one plane, the individuals' buffers
    PopulationDaily(eco.pop)
    stack = rng.random((eco.pop.Ns, eco.pop.K) + shape)
    dev.eco_daily_set_layers(stack.reshape((-1,) + shape))
    assert int(dev.digest(["ECO_LAI_STACK"])[0]) == ref.digest(stack)
    land = (np.random.default_rng(1).random(shape) < 0.4).astype(np.uint8)
    pool = IndividualPool(eco.grid, land, eco, sample_frac=0.1, per_cell=7)
    E, S = rng.random(pool.n_indiv) * 1e4, rng.integers(0, 9, pool.n_indiv).astype(float)
    pool.reset(E, S)
    got = dev.digest(["INDIV_E_DAY", "INDIV_STRESS"])
    assert [int(g) for g in got] == [ref.digest(E), ref.digest(S)]
    # scalars: what was read is what a set puts back
    sc = dev.state_scalars()
    sc2 = sc.copy()
    sc2[0], sc2[2:5] = 1.0, (3.5, 9.0, 42.0)
    dev.set_state_scalars(sc2)
    assert np.array_equal(dev.state_scalars(), sc2)
    dev.close()
    band = Device(qa.SphericalGrid(73, 144), row0=20, n_rows=30, halo=6)
    with pytest.raises(QdError, match="latitude bands are not supported"):
        band.digest(["U"])
    band.close()
