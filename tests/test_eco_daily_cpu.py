"""CPU: the daily vegetation step's host side and its NumPy restatement, no GPU and no libqingdai_hip.so: the restatement against
the reference's goldens (bitwise), the species-mode policy, the environment parsing, the day-accumulator schedule, the rollback
contract of the third span participant around a stub library, the driver's refusal of QD_ECO_MUT_RATE > 0, the new ABI names."""
import ctypes
import glob
import json
import os

import numpy as np
import pytest

import eco_daily_ref as ref
from qingdai_amd import _lib
from qingdai_amd._lib import QdError
from qingdai_amd.device import Device

HERE = os.path.dirname(os.path.abspath(__file__))
GOLDENS = sorted(glob.glob(os.path.join(HERE, "golden", "eco_daily_*_19x36.npz")))
CASES = ["defaults", "layers", "rate_clipped", "seam", "spread_moore", "spread_vn"]
OUT_KEYS = ("LAI_layers_SK", "total_LAI", "age_days", "seed_bank", "spread_gate", "E_day")


def _env_of(z):
    return {str(k): str(v) for k, v in zip(z["env_keys"], z["env_vals"])}


def _clean_env(monkeypatch, env=None):
    for k in [k for k in os.environ if k.startswith("QD_ECO_")]:
        monkeypatch.delenv(k)
    for k, v in (env or {}).items():
        monkeypatch.setenv(k, v)


def test_every_case_has_a_golden_cpu():
    assert [os.path.basename(p)[10:-10] for p in GOLDENS] == CASES


@pytest.mark.parametrize("path", GOLDENS, ids=lambda p: os.path.basename(p)[10:-10])
def test_restatement_matches_reference_bitwise_cpu(path):
    z = np.load(path)
    land = z["land_mask"] == 1
    cfg = ref.Cfg.from_env(_env_of(z), z["modes"], z["species_weights"])
    st = ref.State(land, z["L0"].copy(), np.zeros(land.shape), np.zeros(land.shape), z["bank0"].copy(), land.astype(float))
    n = int(z["n_days"])
    probe = {}
    for d in range(n):
        st.E_day = z["E_days"][d].copy()
        assert np.array_equal(ref.soil_index(z["W_land"][d], z["glacier"], cfg.soil_cap), z["soil"][d])
        ref.step_daily(st, cfg, z["soil"][d], probe)
        tag = {0: "first", n - 1: "last"}.get(d)
        if tag:
            got = dict(zip(OUT_KEYS, (st.layers, st.total(), st.age, st.bank, st.gate, st.E_day)))
            for k, v in got.items():
                assert np.array_equal(v, z[f"{tag}_{k}"]), (tag, k)
            assert np.array_equal(np.sum(np.sum(st.layers, axis=0), axis=0), z[f"{tag}_LAI"])
            s = st.summary()
            assert [s["LAI_min"], s["LAI_mean"], s["LAI_max"]] == list(z[f"{tag}_summary"])
    assert probe and min(probe.values()) > 1e-9, probe          # no input sits on a branch (the generator's condition)
    assert json.loads(str(z["meta"]))["probe"] == probe


def test_goldens_cover_what_they_claim_cpu():
    z = {c: np.load(p) for c, p in zip(CASES, GOLDENS)}
    d = z["defaults"]                                           # K == 1, no spread: the layers never move, the age does
    assert d["L0"].shape[:2] == (20, 1) and np.array_equal(d["last_LAI_layers_SK"], d["L0"]) and d["last_age_days"].max() == 3.0
    y = z["layers"]
    assert y["L0"].shape[:2] == (4, 3) and not np.isfinite(y["E_days"][0]).all() and (y["E_days"][0] == 0.0).any()
    land = y["land_mask"] == 1
    assert (y["soil"][0][land] > 0.3).any() and (y["soil"][0][land] < 0.3).any() and (y["glacier"][land] != 0).any()
    v = z["spread_vn"]
    assert sorted(set(map(str, v["modes"]))) == ["diffusion", "seed"] and v["land_mask"][0].any() and v["land_mask"][-1].any()
    m = z["spread_moore"]
    assert m["bank0"].max() > 0 and np.isclose(m["first_seed_bank"].max(), 2.0 * 0.75 * 0.9)      # QD_ECO_SEED_BANK_MAX reached
    assert float(_env_of(z["rate_clipped"])["QD_ECO_SPREAD_RATE"]) == 0.9


def test_seam_golden_has_land_on_both_sides_of_the_longitude_seam_cpu(monkeypatch):
    """The other five goldens hold no land in the last column.  This one has land in column 0 and in column nlon-1 on the same rows,
    both pole rows and the four corners among them, the Moore neighbourhood, the deepest stack and both spread modes -- and its
    expected values depend on the wrap: a restatement whose east-west shift does not wrap misses them in the seam columns."""
    z = np.load(os.path.join(HERE, "golden", "eco_daily_seam_19x36.npz"))
    land = z["land_mask"] == 1
    both = land[:, 0] & land[:, -1]
    assert both[0] and both[-1] and both.sum() >= 6 and land[0, 0] and land[0, -1] and land[-1, 0] and land[-1, -1]
    assert (both & ~land[:, 1] & ~land[:, -2]).any()            # seam cells whose only east-west land neighbour is across the seam
    env = _env_of(z)
    assert z["L0"].shape[:2] == (2, 8) and env["QD_ECO_SPREAD_NEIGHBORS"] == "moore" and int(z["n_days"]) == 3
    assert sorted(map(str, z["modes"])) == ["diffusion", "seed"] and z["bank0"].max() > 0
    cfg = ref.Cfg.from_env(env, z["modes"], z["species_weights"])

    def run():
        st = ref.State(land, z["L0"].copy(), z["E_days"][0].copy(), np.zeros(land.shape), z["bank0"].copy(), land.astype(float))
        return ref.step_daily(st, cfg, z["soil"][0]).layers

    assert np.array_equal(run(), z["first_LAI_layers_SK"])
    roll = np.roll

    def no_wrap(x, shift, axis):                                # np.roll whose longitude shift brings zeros in, not the far column
        out = roll(x, shift=shift, axis=axis)
        dx = shift[1]
        if dx > 0:
            out[..., :dx] = 0
        elif dx < 0:
            out[..., dx:] = 0
        return out

    monkeypatch.setattr(np, "roll", no_wrap)
    broken = run()
    monkeypatch.undo()
    diff = np.any(broken != z["first_LAI_layers_SK"], axis=(0, 1))
    assert diff[:, 0].any() and diff[:, -1].any() and diff[0, 0] and diff[-1, -1] and not diff[:, 3:-3].any()


def test_two_and_more_firings_in_one_step_cpu():
    """dt = 2.5 days: the reference's literal `while accum >= day` loop (run_simulation.py:1785-1789) fires 2, 3, 2, 3 ... times per
    step; daily_counts gives the same counts and the same accumulator for any cut of the steps."""
    from qingdai_amd.ecology import daily_counts
    day = 2 * np.pi / 8.726646259971648e-5
    dt = 2.5 * day
    accum, fired = 0.0, []
    for _ in range(41):
        accum += dt
        k = 0
        while accum >= day:
            accum -= day
            k += 1
        fired.append(k)
    assert set(fired) == {2, 3} and sum(fired) in (102, 103)
    for cuts in ([41], [1] * 41, [2, 3, 36], [40, 1]):
        a, got = 0.0, []
        for n in cuts:
            f, a = daily_counts(a, dt, n, day)
            assert f.dtype == np.int32
            got += [int(x) for x in f]
        assert got == fired and a == accum, cuts


@pytest.mark.parametrize("path", GOLDENS, ids=lambda p: os.path.basename(p)[10:-10])
def test_species_mode_policy_reproduces_goldens_cpu(path, monkeypatch):
    from qingdai_amd.ecology import species_modes_from_env
    z = np.load(path)
    env = _env_of(z)
    _clean_env(monkeypatch, env)
    w = z["species_weights"]
    assert species_modes_from_env(len(w), w, "QD_ECO_SPECIES_WEIGHTS" in env) == [str(m) for m in z["modes"]]


class _FakeDev:
    def __init__(self):
        self.calls = []

    def eco_daily_configure(self, params, mode, w):
        self.calls.append(("configure", list(mode), np.asarray(w).copy()))

    def eco_daily_set_layers(self, layers):
        self.calls.append(("layers", layers.shape))

    def upload_now(self, name, arr):
        self.calls.append(("upload", name))


class _FakePop:
    def __init__(self, S=3, K=2, shape=(5, 8)):
        self._dev, self.shape, self.Ns, self.K = _FakeDev(), shape, S, K
        self.species_weights = np.full(S, 1.0 / S)
        self.LAI_layers_SK = np.zeros((S, K) + shape)
        self.land = np.ones(shape, dtype=bool)
        self.daily = None


def test_env_parsing_and_fallbacks_cpu(monkeypatch):
    from qingdai_amd.ecology import PopulationDaily
    _clean_env(monkeypatch)
    p = PopulationDaily(_FakePop(), day_seconds=100.0).params
    got = {n: getattr(p, n) for n, _ in p._fields_}
    assert got == dict(n_species=3, n_layers=2, spread=0, moore=0, gate_soil=1, reserved=0, lai_max=5.0, k_canopy=0.5, growth_per_j=2.0e-5,
                       senesce_per_day=0.01, stress_thresh=0.3, stress_strength=1.0, soil_cap=50.0, repro_frac=0.2, spread_rate=0.0,
                       soil_exp=1.0, upfrac=0.1, dlai_max=0.02, seed_energy=1.0, seed_scale=1.0, seedling_lai=0.02, retain=0.2,
                       bank_max=1000.0, seed_dlai_max=0.01, germ_frac=0.10, bank_decay=0.02)
    _clean_env(monkeypatch, {"QD_ECO_SPREAD_ENABLE": "1", "QD_ECO_SPREAD_RATE": "0.9", "QD_ECO_SPREAD_NEIGHBORS": " Moore ",
                             "QD_ECO_REPRO_FRACTION": "1.5", "QD_ECO_SEED_ENERGY": "0", "QD_ECO_LAI_MAX": "junk",
                             "QD_ECO_SPREAD_SOIL_EXP": "junk", "QD_ECO_SOIL_WATER_CAP": "junk", "QD_ECO_SPECIES_1_MODE": "SEED",
                             "QD_ECO_SPECIES_0_MODE": "diffusion", "QD_ECO_SPECIES_2_MODE": "diffusion"})
    pop = _FakePop()
    d = PopulationDaily(pop, day_seconds=100.0)
    p = d.params
    assert (p.spread, p.moore, p.spread_rate, p.repro_frac, p.seed_energy, p.lai_max) == (1, 1, 0.5, 0.95, 1e-12, 5.0)
    assert (p.gate_soil, p.soil_cap) == (0, 50.0)               # an unparsable exponent means the land-mask gate; the cap falls back
    assert d.species_modes == ["diffusion", "seed", "diffusion"] and pop.daily is d
    kind = [c[0] for c in pop._dev.calls]
    assert kind == ["configure", "layers", "upload"] and pop._dev.calls[0][1] == [0, 1, 0]
    _clean_env(monkeypatch, {"QD_ECO_SPREAD_ENABLE": "1", "QD_ECO_SPREAD_RATE": "-1"})
    assert PopulationDaily(_FakePop(), day_seconds=100.0).params.spread == 0


def test_schedule_is_the_reference_accumulator_cpu():
    from qingdai_amd.ecology import daily_counts
    day, dt = 2 * np.pi / 8.726646259971648e-5, 700.0           # dt does not divide the day
    accum, fired = 0.0, []
    for s in range(400):                                        # the reference's loop, step by step
        accum += dt
        k = 0
        while accum >= day:
            accum -= day
            k += 1
        fired.append(k)
    a, got = 0.0, []
    for n in (1, 37, 200, 162):                                 # any chunking gives the same firings and the same accumulator
        f, a = daily_counts(a, dt, n, day)
        got += list(f)
    assert got == fired and a == accum and sum(fired) == int(400 * dt // day) == 3
    f, a = daily_counts(0.0, 2.5 * day, 2, day)                 # dt > day: more than one firing in a step
    assert list(f) == [2, 3] and abs(a) < 1e-6


# ---- the span participant around a stub library (as tests/test_span_rollback_cpu.py does for the other two lanes)
N, DT = 30, 300.0
CALLS = ("qd_eco_daily_schedule", "qd_route_schedule", "qd_phyto_daily_schedule", "qd_step_n")


class StubLib:
    def __init__(self, fail=None):
        self.fail, self.calls = fail, []

    def __getattr__(self, name):
        if name not in CALLS:
            raise AttributeError(name)

        def fn(h, *args):
            self.calls.append((name, args))
            return -1 if name == self.fail else 0
        return fn

    def qd_last_error(self, h):
        return b"programmed failure"

    def qd_destroy(self, h):
        return 0


def _stub_device(fail=None):
    dev = object.__new__(Device)
    dev.lib, dev.h, dev._host = StubLib(fail), ctypes.c_void_p(1), {}
    return dev


def _participant(dev):
    from qingdai_amd.ecology import PopulationDaily
    d = object.__new__(PopulationDaily)
    d.dev, d.day_seconds, d.accum_day, d.n_firings = dev, 3000.0, 1200.0, 2
    return d


def _routing(dev):
    from qingdai_amd.routing import RiverRouting
    r = object.__new__(RiverRouting)
    r.dev, r.dt_hydro_seconds, r.t_accum, r._steps = dev, 3600.0, 1200.0, 5
    return r


@pytest.mark.parametrize("fail", ["qd_eco_daily_schedule", "qd_route_schedule", "qd_step_n"])
def test_failure_restores_the_day_accumulator_cpu(fail):
    dev = _stub_device(fail)
    d, r = _participant(dev), _routing(dev)
    with pytest.raises(QdError, match=fail):
        dev.step_n(np.zeros((N, 7)), DT, with_physics=True, with_hydrology=True, ecology=True, routing=r, eco_daily=d)
    assert (d.accum_day, d.n_firings) == (1200.0, 2) and (r.t_accum, r._steps) == (1200.0, 5)
    assert [c[0] for c in dev.lib.calls].count("qd_step_n") == (1 if fail == "qd_step_n" else 0)


def test_success_advances_as_schedule_alone_cpu():
    dev = _stub_device()
    d = _participant(dev)
    dev.step_n(np.zeros((N, 7)), DT, with_physics=True, ecology=True, eco_daily=d)
    (name, args), = [c for c in dev.lib.calls if c[0] == "qd_step_n"]
    assert args[0] == N and args[2] == 2 | 4 | 32 | 512           # bit9 is the lane's flag, bit5 the ecology it needs
    sched, = [c for c in dev.lib.calls if c[0] == "qd_eco_daily_schedule"]
    assert sched[1][0] == N
    twin = _participant(None)
    fire = twin.schedule(DT, N)
    assert int(fire.sum()) == 3 and d.accum_day == twin.accum_day and d.n_firings == 2 + 3
    with pytest.raises(ValueError, match="step_n: the PopulationDaily runs on another device handle"):
        dev.step_n(np.zeros((N, 7)), DT, with_physics=True, ecology=True, eco_daily=_participant(_stub_device()))


def test_driver_refuses_mutation_with_the_device_daily_step_cpu():
    from qingdai_amd.driver import eco_daily_enabled
    assert eco_daily_enabled({}) is False and eco_daily_enabled({"QD_ECO_MUT_RATE": "0.3"}) is False      # the switch defaults to 0
    assert eco_daily_enabled({"QD_ECO_DAILY": "1"}) is True and eco_daily_enabled({"QD_ECO_DAILY": "1", "QD_ECO_MUT_RATE": "0"}) is True
    with pytest.raises(ValueError, match="QD_ECO_DAILY=1 does not support QD_ECO_MUT_RATE > 0"):
        eco_daily_enabled({"QD_ECO_DAILY": "1", "QD_ECO_MUT_RATE": "0.01"})


def test_diag_line_format_cpu():
    from qingdai_amd.ecology import eco_daily_line
    assert eco_daily_line([3.0, 0.1949, 0.2051, 1.0]) == "[Ecology] daily: LAI(min/mean/max)=0.19/0.21/1.00"


def test_abi_names_cpu():
    # names, layout and constants against the header and the library: tests/test_abi_cpu.py, for every symbol and struct
    assert _lib.STEP_BITS.index("eco_daily") == 9 and _lib.step_flags(eco_daily=True) == 512
    assert {"ECO_AGE", "ECO_SEEDBANK", "ECO_GATE"} <= set(_lib.FIELDS)
    assert ctypes.sizeof(_lib.qd_eco_daily_params) == 6 * 4 + 20 * 8
