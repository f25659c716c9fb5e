"""GPU (-m gpu): the daily vegetation step on the device (qd_eco_daily_*, the third span lane): the class seam against the
reference's goldens after one and three firings, a 721 x 1440 firing against the NumPy restatement (and run twice), the lane
inside one qd_step_n span against the same span cut at the day boundaries with the host path, a run without the switch, the
driver's `[Ecology] daily:` lines, and the refusals.

Tolerance.  The goldens of the reference's own class are the yardstick; deviations are max |a - b| / max |b| per array (util.relerr).
The starting bound is the 1e-14 relative that tests/test_gpu_ecology.py gives the f64 sub-daily step's multi-term results; the
bound in force is ten times the largest deviation measured on the MI355X over all cases and arrays, never looser than the start
(MEASURED and BOUND below).  Measured on the MI355X over the six goldens: 3.25e-16 (layers; seam 3.11e-16, spread_moore 2.47e-16,
spread_vn 1.97e-16, defaults 1.12e-16, rate_clipped 2.3e-18); the largest figure any test of this file printed is 4.5e-16 (the
721 x 1440 firing against the restatement).  Every test prints its deviations.  The defaults case (no exp / pow on its path) must
come out bitwise."""
import glob
import os

import numpy as np
import pytest

import eco_daily_ref as ref
from util import relerr

pytestmark = pytest.mark.gpu

HERE = os.path.dirname(os.path.abspath(__file__))
GOLDENS = sorted(glob.glob(os.path.join(HERE, "golden", "eco_daily_*_19x36.npz")))
START = 1e-14
MEASURED = 3.3e-16                 # largest deviation from the goldens on the MI355X (3.247e-16, rounded up; see the docstring)
BOUND = START if MEASURED is None else min(START, 10 * MEASURED)
PROGNOSTIC = ("U", "V", "H", "TS", "Q", "CLOUD", "HICE", "W_LAND", "S_SNOW", "ALBEDO")


def _clean_env(monkeypatch, env=None):
    for k in [k for k in os.environ if k.startswith(("QD_ECO_", "QD_PHYTO_"))]:
        monkeypatch.delenv(k)
    for k, v in (env or {}).items():
        monkeypatch.setenv(str(k), str(v))


def _pop_on(grid_shape, land_mask):
    import qingdai_amd as qa
    from qingdai_amd.device import Device
    from qingdai_amd.ecology import EcologyAdapter
    grid = qa.SphericalGrid(*grid_shape)
    dev = Device(grid)
    dev.upload_now("LAND_MASK", land_mask)
    eco = EcologyAdapter(grid, land_mask, dev=dev, albedo_couple=True)
    return dev, eco.pop


def _state(pop):
    return {"LAI_layers_SK": pop.LAI_layers_SK.copy(), "total_LAI": pop.total_LAI(), "age_days": pop.age_days, "seed_bank": pop.seed_bank,
            "spread_gate": pop._spread_gate, "E_day": pop.E_day}


@pytest.mark.parametrize("path", GOLDENS, ids=lambda p: os.path.basename(p)[10:-10])
def test_class_seam_vs_reference_goldens(gpu, path, monkeypatch):
    from qingdai_amd.ecology import PopulationDaily
    z = np.load(path)
    case = os.path.basename(path)[10:-10]
    _clean_env(monkeypatch, dict(zip(z["env_keys"], z["env_vals"])))
    dev, pop = _pop_on(z["land_mask"].shape, z["land_mask"])
    daily = PopulationDaily(pop)
    assert daily.species_modes == [str(m) for m in z["modes"]] and np.array_equal(pop.species_weights, z["species_weights"])
    pop.push_layers(z["L0"], init=True)
    pop.seed_bank = z["bank0"]
    before = pop.state()
    n, worst = int(z["n_days"]), 0.0
    for d in range(n):
        pop.E_day = z["E_days"][d]
        pop.step_daily(z["soil"][d])
        tag = {0: "first", n - 1: "last"}.get(d)
        if not tag:
            continue
        got = _state(pop)
        errs = {k: relerr(v, z[f"{tag}_{k}"]) for k, v in got.items()}
        rec = daily.log()[-1]
        errs["summary"] = relerr([rec["LAI_min"], rec["LAI_mean"], rec["LAI_max"]], z[f"{tag}_summary"])
        assert rec["step"] == d + 1
        print(case, tag, {k: f"{e:.2e}" for k, e in errs.items()})
        worst = max(worst, max(errs.values()))
        for k, e in errs.items():
            assert e <= BOUND, (case, tag, k, e)
        assert np.all(got["E_day"] == 0.0) and np.array_equal(got["age_days"], z[f"{tag}_age_days"])
        if case == "defaults":                                  # no exp, no pow on the path: bitwise
            for k, v in got.items():
                assert np.array_equal(v, z[f"{tag}_{k}"]), k
    print(f"{case}: largest deviation from the reference {worst:.3e} (bound {BOUND:.1e})")
    after = pop.state()                                         # the canopy snapshot and its clock are untouched by a firing
    assert (after["hours"], after["next_recompute_hours"], after["n_recompute"]) == (before["hours"], before["next_recompute_hours"], before["n_recompute"])
    assert dev.eco_daily_firings() == n == daily.n_firings
    dev.close()


def test_seam_soil_argument_forms(gpu, monkeypatch):
    """step_daily(None) is a dry day, a scalar fills the map, NULL on the C side takes W_LAND and GLACIER."""
    from qingdai_amd.ecology import PopulationDaily
    z = np.load(GOLDENS[1])
    _clean_env(monkeypatch, dict(zip(z["env_keys"], z["env_vals"])))
    land = z["land_mask"]
    out = []
    for form in ("none", "zeros", "scalar", "full", "resident", "map"):
        dev, pop = _pop_on(land.shape, land)
        PopulationDaily(pop)
        pop.push_layers(z["L0"], init=True)
        pop.E_day = z["E_days"][1]
        if form == "resident":
            dev.upload_now("W_LAND", z["W_land"][1]); dev.upload_now("GLACIER", z["glacier"])
            dev.eco_daily_step(None)
        else:
            pop.step_daily({"none": None, "zeros": np.zeros(land.shape), "scalar": 0.25, "full": np.full(land.shape, 0.25),
                            "map": z["soil"][1]}[form])
        out.append(pop.LAI_layers_SK.copy())
        dev.close()
    assert np.array_equal(out[0], out[1]) and np.array_equal(out[2], out[3]) and np.array_equal(out[4], out[5])
    assert not np.array_equal(out[0], out[2])


def test_full_size_firing_vs_restatement(gpu, monkeypatch):
    from qingdai_amd.ecology import PopulationDaily
    from qingdai_amd.topography import create_land_sea_mask
    import qingdai_amd as qa
    env = {"QD_ECO_COHORT_K": "2", "QD_ECO_SPREAD_ENABLE": "1", "QD_ECO_SPREAD_RATE": "0.1", "QD_ECO_RAND_SEED": "7",
           "QD_ECO_SEED_ENERGY": "500", "QD_ECO_SPREAD_SOIL_EXP": "1.5"}
    _clean_env(monkeypatch, env)
    mask = create_land_sea_mask(qa.SphericalGrid(721, 1440))
    land = mask == 1
    r = np.random.default_rng(3)
    S, K = 20, 2
    L0 = r.uniform(0.0, 0.15, (S, K, 721, 1440)) * land
    E = r.uniform(0.0, 2.0e4, (721, 1440))
    soil = r.uniform(0.0, 0.9, (721, 1440))
    bank0 = r.uniform(0.0, 3.0, (721, 1440)) * land
    runs = []
    for _ in range(2):
        dev, pop = _pop_on((721, 1440), mask)
        daily = PopulationDaily(pop)
        assert (pop.Ns, pop.K) == (S, K) and len(set(daily.species_modes)) == 2
        pop.push_layers(L0, init=True)
        pop.seed_bank = bank0
        pop.E_day = E
        pop.step_daily(soil)
        runs.append((_state(pop), daily.log()[-1], daily.species_modes, pop.species_weights.copy()))
        dev.close()
    for k in runs[0][0]:
        assert np.array_equal(runs[0][0][k], runs[1][0][k]), k  # two runs: bit-identical
    assert runs[0][1] == runs[1][1]
    got, rec, modes, w = runs[0]
    st = ref.State(land, L0.copy(), E.copy(), np.zeros(land.shape), bank0.copy(), land.astype(float))
    ref.step_daily(st, ref.Cfg.from_env(env, modes, w), soil)
    want = {"LAI_layers_SK": st.layers, "total_LAI": st.total(), "age_days": st.age, "seed_bank": st.bank, "spread_gate": st.gate,
            "E_day": st.E_day}
    errs = {k: relerr(got[k], want[k]) for k in want}
    s = st.summary()
    errs["summary"] = relerr([rec["LAI_min"], rec["LAI_mean"], rec["LAI_max"]], [s["LAI_min"], s["LAI_mean"], s["LAI_max"]])
    print("721x1440", {k: f"{e:.2e}" for k, e in errs.items()})
    assert np.abs(st.layers - L0).max() > 0.01 and (st.age[land] == 1.0).any()
    for k, e in errs.items():
        assert e <= (1e-12 if k == "summary" else BOUND), (k, e)     # the mean of 3e5 cells: pairwise on the host, blocked on the device


def _sim(monkeypatch, env, daily_hook=None, day=7000.0):
    import qingdai_amd as qa
    from qingdai_amd.driver import Simulation
    _clean_env(monkeypatch, env)
    nlat, nlon = 37, 72
    sim = Simulation(nlat, nlon, params=qa.QdParams(), use_ocean=False, quiet=True, individuals=False, daily_hook=daily_hook)
    sim.day_seconds = day
    if sim.eco_daily is not None:
        sim.eco_daily.day_seconds = day
    r = np.random.default_rng(8)
    lat = np.deg2rad(sim.grid.lat_mesh)
    land = sim.land_mask == 1
    sim.gcm.h, sim.gcm.T_s = 8000.0 - 10500.0 * np.sin(lat) ** 2, 262.0 + 36.0 * np.cos(lat) ** 2
    sim.dev.set("S_SNOW", np.where(land & (np.abs(sim.grid.lat_mesh) > 55), 60.0, 0.0))
    sim.dev.set("W_LAND", np.where(land, 40.0 * r.random((nlat, nlon)), 0.0))
    S, K = sim.eco.pop.Ns, sim.eco.pop.K
    sim.eco.pop.push_layers(np.abs(r.normal(0.2, 0.15, (S, K, nlat, nlon))) * land, init=True)
    return sim


def _fields(sim, names):
    for k in names:
        sim.dev._host.pop(k, None)
    return {k: sim.dev.get(k).copy() for k in names}


LANE_ENV = {"QD_ECO_NS": "4", "QD_ECO_COHORT_K": "2", "QD_ECO_LAI_GROWTH": "4e-8", "QD_ECO_SPREAD_ENABLE": "1", "QD_ECO_SPREAD_RATE": "0.1",
            "QD_ECO_SEED_ENERGY": "2e4", "QD_ECO_RAND_SEED": "2", "QD_ECO_LIGHT_UPDATE_EVERY_HOURS": "1"}


def test_lane_in_span_vs_host_path_cut_at_the_boundaries(gpu, monkeypatch):
    """One qd_step_n span of 60 steps crossing two (shortened) day boundaries with the lane, against the same 60 steps cut at the
    boundaries by a daily_hook that runs the NumPy restatement on downloaded state and pushes the layers back."""
    lane = _sim(monkeypatch, {**LANE_ENV, "QD_ECO_DAILY": "1"})
    assert lane.eco_daily is not None and len(set(lane.eco_daily.species_modes)) == 2
    lane.run_steps(60)
    assert lane.dev.eco_daily_firings() == 2 == lane.eco_daily.n_firings

    host = {}

    def hook(sim_, soil_idx, glacier):
        pop = sim_.eco.pop
        if "st" not in host:
            land = pop.land
            host["st"] = ref.State(land, None, None, np.zeros(land.shape), np.zeros(land.shape), land.astype(float))
            host["cfg"] = ref.Cfg.from_env({k: v for k, v in os.environ.items() if k.startswith("QD_ECO_")}, lane.eco_daily.species_modes,
                                           pop.species_weights)
        st = host["st"]
        st.layers, st.E_day = pop.LAI_layers_SK.copy(), pop.E_day
        ref.step_daily(st, host["cfg"], soil_idx)
        pop.E_day = 0.0
        pop.push_layers(st.layers)
        host["n"] = host.get("n", 0) + 1

    cut = _sim(monkeypatch, LANE_ENV, daily_hook=hook)
    assert cut.eco_daily is None
    cut.run_steps(60)
    assert host["n"] == 2
    a, b = lane.eco.pop, cut.eco.pop
    errs = {"layers": relerr(a.LAI_layers_SK, b.LAI_layers_SK), "E_day": relerr(a.E_day, b.E_day), "ECO_LAI": relerr(a.total_LAI(), b.total_LAI()),
            "age": relerr(a.age_days, host["st"].age), "bank": relerr(a.seed_bank, host["st"].bank)}
    fa, fb = _fields(lane, PROGNOSTIC + ("ECO_ALPHA", "ECO_F")), _fields(cut, PROGNOSTIC + ("ECO_ALPHA", "ECO_F"))
    for k in fa:
        errs[k] = float(np.nanmax(np.abs(fa[k] - fb[k]))) / max(float(np.nanmax(np.abs(fb[k]))), 1e-300)
        assert np.array_equal(np.isnan(fa[k]), np.isnan(fb[k])), k
    print({k: f"{e:.2e}" for k, e in errs.items()})
    assert a.state() == b.state()                               # the same canopy recomputes on the same steps
    for k in ("layers", "ECO_LAI", "age", "bank"):
        assert errs[k] <= BOUND, (k, errs[k])
    assert errs["E_day"] <= 1e-14
    for k in fa:                                                # the last-bit LAI differences reach the fields through the albedo only
        assert errs[k] <= 1e-12, (k, errs[k])
    # the next sub-step's alpha map
    lane.run_steps(1); cut.run_steps(1)
    na, nb = _fields(lane, ("ECO_ALPHA",))["ECO_ALPHA"], _fields(cut, ("ECO_ALPHA",))["ECO_ALPHA"]
    assert np.array_equal(np.isnan(na), np.isnan(nb)) and np.nanmax(np.abs(na - nb)) <= 1e-14
    lane.dev.close(); cut.dev.close()


def test_switch_unset_changes_nothing_and_an_idle_lane_is_free(gpu, monkeypatch):
    """Without QD_ECO_DAILY the driver builds no lane and a span is what it was; with it, a span that crosses no day boundary is
    bit-identical to that."""
    plain = _sim(monkeypatch, LANE_ENV)
    assert plain.eco_daily is None
    plain.run_steps(20)
    zero = _sim(monkeypatch, {**LANE_ENV, "QD_ECO_DAILY": "0"})
    assert zero.eco_daily is None
    zero.run_steps(20)
    idle = _sim(monkeypatch, {**LANE_ENV, "QD_ECO_DAILY": "1"})
    idle.run_steps(20)                                          # 6000 s < the 7000 s day
    assert idle.dev.eco_daily_firings() == 0
    names = PROGNOSTIC + ("ECO_LAI", "ECO_EDAY", "ECO_ALPHA", "ECO_F")
    fp, fz, fi = _fields(plain, names), _fields(zero, names), _fields(idle, names)
    for k in names:
        assert np.array_equal(fp[k], fz[k], equal_nan=True) and np.array_equal(fp[k], fi[k], equal_nan=True), k
    assert plain.eco.pop.state() == idle.eco.pop.state()
    for s in (plain, zero, idle):
        s.dev.close()


def test_driver_main_prints_daily_lines_and_lai_moves(gpu, tmp_path, monkeypatch, capsys):
    from qingdai_amd import driver
    for k in [k for k in os.environ if k.startswith("QD_")]:
        monkeypatch.delenv(k)
    env = {"QD_N_LAT": "37", "QD_N_LON": "72", "QD_SIM_DAYS": "2.05", "QD_DATA_DIR": str(tmp_path / "data"), "QD_DYN_DIAG_PRINT": "0",
           "QD_USE_OCEAN": "0", "QD_AUTOSAVE_ENABLE": "0", "QD_HYDRO_ENABLE": "0", "QD_ECO_INDIV_ENABLE": "0", "QD_PHYTO_ENABLE": "0",
           "QD_ECO_DAILY": "1", "QD_ECO_COHORT_K": "2", "QD_ECO_LAI_GROWTH": "2e-8"}
    for k, v in env.items():
        monkeypatch.setenv(k, v)
    monkeypatch.chdir(tmp_path)
    assert driver.main() == 0
    out = capsys.readouterr().out
    lines = [l for l in out.splitlines() if l.startswith("[Ecology] daily: LAI(min/mean/max)=")]
    assert len(lines) == 2, out
    assert "[Ecology] daily step on the device: K=2, Ns=20" in out
    vals = [tuple(float(x) for x in l.split("=")[1].split("/")) for l in lines]
    assert all(v[0] <= v[1] <= v[2] for v in vals) and vals[-1][1] != 0.20 and vals[-1][2] > 0.20      # the LAI left its t = 0 value
    # the mutation switch is refused at start-up
    monkeypatch.setenv("QD_ECO_MUT_RATE", "0.05")
    with pytest.raises(ValueError, match="QD_ECO_DAILY=1 does not support QD_ECO_MUT_RATE > 0"):
        driver.main()
    # without the switch: no lines, as before
    monkeypatch.delenv("QD_ECO_MUT_RATE"); monkeypatch.delenv("QD_ECO_DAILY"); monkeypatch.setenv("QD_SIM_DAYS", "1.05")
    assert driver.main() == 0
    assert "[Ecology] daily" not in capsys.readouterr().out


def test_refusals(gpu, monkeypatch):
    import ctypes
    import qingdai_amd as qa
    from qingdai_amd._lib import QdError, SPAN_LOG_CAP
    from qingdai_amd.device import Device
    from qingdai_amd.ecology import PopulationDaily
    _clean_env(monkeypatch, {"QD_ECO_NS": "2"})
    z = np.load(GOLDENS[0])
    land = z["land_mask"]
    stars = qa.ThermalForcing(qa.SphericalGrid(*land.shape), qa.OrbitalSystem()).star_table(300.0 * np.arange(4))
    dp = ctypes.POINTER(ctypes.c_double)

    def step_n(dev, n, flags):
        st = np.ascontiguousarray(stars[:n])
        return dev.lib.qd_step_n(dev.h, n, 300.0, flags, st.ctypes.data_as(dp)), (dev.lib.qd_last_error(dev.h) or b"").decode()

    # bit9 without a configure
    dev, pop = _pop_on(land.shape, land)
    rc, err = step_n(dev, 4, 2 | 32 | 512)
    assert rc != 0 and "bit9 set but qd_eco_daily_configure has not been called" in err
    with pytest.raises(QdError, match="qd_eco_daily_configure has not been called"):
        dev.eco_daily_step(None)
    with pytest.raises(QdError, match="qd_eco_daily_configure has not been called"):
        dev.eco_daily_log()
    daily = PopulationDaily(pop)
    # without bit5
    dev.eco_daily_schedule(np.zeros(4, dtype=np.int32))
    rc, err = step_n(dev, 4, 2 | 512)
    assert rc != 0 and "needs the ecology sub-step (bit5)" in err
    # a schedule whose length is not the span's, and none at all (a span that began consumed its schedule)
    dev.eco_daily_schedule(np.zeros(3, dtype=np.int32))
    rc, err = step_n(dev, 4, 2 | 32 | 512)
    assert rc != 0 and "needs a qd_eco_daily_schedule of exactly n steps" in err
    # a span whose firings do not fit into the log
    dev.eco_daily_schedule(np.array([SPAN_LOG_CAP, 1, 0, 0], dtype=np.int32))
    rc, err = step_n(dev, 4, 2 | 32 | 512)
    assert rc != 0 and "would overflow the summary log" in err
    # a log without room
    pop.step_daily(0.5); pop.step_daily(0.5)
    buf, n = np.empty(4), ctypes.c_int32(0)
    assert dev.lib.qd_eco_daily_log(dev.h, buf.ctypes.data_as(dp), 1, ctypes.byref(n)) != 0
    assert "more records than room" in dev.lib.qd_last_error(dev.h).decode()
    assert len(daily.log()) == 2 and daily.log() == []
    # a good span still runs after the refusals
    dev.eco_daily_schedule(np.array([0, 1, 0, 0], dtype=np.int32))
    rc, err = step_n(dev, 4, 2 | 32 | 512)
    assert rc == 0, err
    assert [r["step"] for r in daily.log()] == [3]
    rc, err = step_n(dev, 4, 2 | 32 | 512)
    assert rc != 0 and "needs a qd_eco_daily_schedule of exactly n steps" in err
    # wrong plane count, struct size
    with pytest.raises(QdError, match="plane count is not n_species \\* n_layers"):
        dev.eco_daily_set_layers(np.zeros((3,) + land.shape))
    assert dev.lib.qd_eco_daily_configure(dev.h, ctypes.byref(daily.params), 8, (ctypes.c_int32 * 2)(0, 0), (ctypes.c_double * 2)(0.5, 0.5)) != 0
    dev.close()
    # banded handles
    band = Device(qa.SphericalGrid(73, 144), row0=20, n_rows=30, halo=6)
    rc = band.lib.qd_eco_daily_configure(band.h, ctypes.byref(daily.params), ctypes.sizeof(daily.params), (ctypes.c_int32 * 2)(0, 0),
                                         (ctypes.c_double * 2)(0.5, 0.5))
    assert rc != 0 and b"latitude bands are not supported" in band.lib.qd_last_error(band.h)
    assert band.lib.qd_eco_daily_step(band.h, None) != 0 and b"whole-globe" in band.lib.qd_last_error(band.h)
    one = np.zeros((1, 7))
    rc = band.lib.qd_step_n(band.h, 1, 300.0, 2 | 512, one.ctypes.data_as(dp))
    assert rc != 0 and b"whole-globe" in band.lib.qd_last_error(band.h)
    band.close()


# ---------------------------------------------------------------------------------------------------------------- kernel edges
def test_two_and_three_firings_in_one_step_vs_seam_calls(gpu, monkeypatch):
    """dt = 2.5 days: the first step of a span fires twice, the second three times (qd_step_n loops over the step's count).  Against the
    same state advanced by as many seam calls of pop.step_daily (soil index from the downloaded W_LAND and GLACIER) followed by
    a step whose lane is idle: state, fields and log records bit-identical, and the device counts every firing."""
    names = PROGNOSTIC + ("ECO_LAI", "ECO_EDAY", "ECO_ALPHA", "ECO_F", "ECO_AGE", "ECO_SEEDBANK", "ECO_GATE")
    span = _sim(monkeypatch, {**LANE_ENV, "QD_ECO_DAILY": "1"}, day=1.0e9)
    seam = _sim(monkeypatch, {**LANE_ENV, "QD_ECO_DAILY": "1"}, day=1.0e9)
    for s in (span, seam):
        s.eco.pop.seed_bank = np.where(s.land_mask == 1, 0.5, 0.0)
        s.run_steps(3)                                          # GLACIER, W_LAND and E_day are the loop's own before the firings
        assert s.dev.eco_daily_firings() == 0
    span.eco_daily.day_seconds, span.eco_daily.accum_day = span.dt / 2.5, 0.0
    log_span, log_seam, total = [], [], 0
    drain = span.dev.eco_daily_log

    def keep():                                                 # the driver drains the log after every span: keep what it drains
        out = drain()
        log_span.extend({"step": int(r[0]), "LAI_min": float(r[1]), "LAI_mean": float(r[2]), "LAI_max": float(r[3])} for r in out)
        return out
    span.dev.eco_daily_log = keep
    for want in (2, 3):
        span.run_steps(1)
        for _ in range(want):
            f = _fields(seam, ("W_LAND", "GLACIER"))
            seam.eco.pop.step_daily(ref.soil_index(f["W_LAND"], f["GLACIER"], 50.0))
        log_seam += seam.eco_daily.log()
        seam.run_steps(1)
        total += want
        assert span.dev.eco_daily_firings() == total == seam.dev.eco_daily_firings() and span.eco_daily.n_firings == total
        fa, fb = _fields(span, names), _fields(seam, names)
        for k in names:
            assert np.array_equal(fa[k], fb[k], equal_nan=True), (want, k)
        assert np.array_equal(span.eco.pop.LAI_layers_SK, seam.eco.pop.LAI_layers_SK)
        assert span.eco.pop.state() == seam.eco.pop.state()
    assert log_span == log_seam and [r["step"] for r in log_span] == [1, 2, 3, 4, 5]
    span.dev.close(); seam.dev.close()


def test_f32_maps_store_the_f64_total_rounded_once(gpu, monkeypatch):
    """QD_ECO_F32=1 (k_ecod_finish's f32 store of ECO_LAI): one seam firing of the seam golden leaves layers, age, bank and gate
    bit-identical to the f64 run -- the arithmetic is f64 either way -- and ECO_LAI is exactly float32 of the f64 run's ECO_LAI."""
    from qingdai_amd.ecology import PopulationDaily
    z = np.load(os.path.join(HERE, "golden", "eco_daily_seam_19x36.npz"))
    out = {}
    for f32 in ("0", "1"):
        _clean_env(monkeypatch, {**dict(zip(z["env_keys"], z["env_vals"])), "QD_ECO_F32": f32})
        dev, pop = _pop_on(z["land_mask"].shape, z["land_mask"])
        daily = PopulationDaily(pop)
        pop.push_layers(z["L0"], init=True)
        pop.seed_bank = z["bank0"]
        pop.E_day = z["E_days"][0]
        pop.step_daily(z["soil"][0])
        out[f32] = (_state(pop), daily.log()[-1])
        dev.close()
    a, b = out["0"][0], out["1"][0]
    for k in ("LAI_layers_SK", "age_days", "seed_bank", "spread_gate", "E_day"):
        assert np.array_equal(a[k], b[k]), k
    assert np.array_equal(b["total_LAI"], a["total_LAI"].astype(np.float32).astype(np.float64))
    assert not np.array_equal(b["total_LAI"], a["total_LAI"])  # the store really is f32
    assert out["0"][1] == out["1"][1]                           # the summary is taken from the f64 total in both


EDGE_ENV = {"QD_ECO_NS": "3", "QD_ECO_COHORT_K": "5", "QD_ECO_SPREAD_ENABLE": "1", "QD_ECO_SPREAD_RATE": "0.2", "QD_ECO_SPREAD_NEIGHBORS": "moore",
            "QD_ECO_SEED_ENERGY": "300", "QD_ECO_SPREAD_SOIL_EXP": "2", "QD_ECO_SPECIES_0_MODE": "seed", "QD_ECO_SPECIES_1_MODE": "diffusion",
            "QD_ECO_SPECIES_2_MODE": "seed"}


def _edge_masks():
    r = np.random.default_rng(17)
    one = np.zeros((9, 24), np.uint8); one[4, 11] = 1
    corner = np.zeros((9, 24), np.uint8); corner[0, 0] = 1      # isolated, and every neighbour is across a seam
    return {"no_land": np.zeros((9, 24), np.uint8), "all_land": np.ones((9, 24), np.uint8), "one_cell": one, "one_corner_cell": corner,
            "nlon20_below_a_wavefront": (r.random((7, 20)) < 0.6).astype(np.uint8),
            "nlon100_not_a_multiple_of_64": (r.random((9, 100)) < 0.6).astype(np.uint8),
            "nlon300_two_blocks_per_row": (r.random((6, 300)) < 0.6).astype(np.uint8)}


@pytest.mark.parametrize("case", list(_edge_masks()))
def test_degenerate_masks_and_row_lengths_vs_restatement(gpu, monkeypatch, case):
    """Two firings on masks and row lengths where an indexing slip shows: no land at all (summary record {n, 0, 0, 0}), all land,
    one isolated land cell (in the interior, and in a corner where all eight neighbours lie across a seam), rows shorter than
    one wavefront, rows that are no multiple of 64, rows longer than one block.  Against the NumPy restatement (which the
    reference's goldens pin bitwise), Moore neighbourhood, K = 5, both spread modes, soil exponent 2 (no device pow)."""
    from qingdai_amd.ecology import PopulationDaily
    _clean_env(monkeypatch, EDGE_ENV)
    mask = _edge_masks()[case]
    land = mask == 1
    r = np.random.default_rng(sum(map(ord, case)))
    S, K = 3, 5
    L0 = r.uniform(0.0, 0.2, (S, K) + mask.shape) * land
    bank0 = r.uniform(0.0, 2.0, mask.shape) * land
    dev, pop = _pop_on(mask.shape, mask)
    daily = PopulationDaily(pop)
    assert (pop.Ns, pop.K) == (S, K) and daily.species_modes == ["seed", "diffusion", "seed"]
    pop.push_layers(L0, init=True)
    pop.seed_bank = bank0
    st = ref.State(land, L0.copy(), None, np.zeros(mask.shape), bank0.copy(), land.astype(float))
    cfg = ref.Cfg.from_env(EDGE_ENV, daily.species_modes, pop.species_weights)
    for d in range(2):
        E, soil = r.uniform(0.0, 2.0e4, mask.shape), r.uniform(0.0, 0.9, mask.shape)
        pop.E_day = E
        pop.step_daily(soil)
        st.E_day = E.copy()
        ref.step_daily(st, cfg, soil)
        got = _state(pop)
        want = {"LAI_layers_SK": st.layers, "total_LAI": st.total(), "age_days": st.age, "seed_bank": st.bank, "spread_gate": st.gate,
                "E_day": st.E_day}
        errs = {k: relerr(got[k], want[k]) for k in want}
        rec, s = daily.log()[-1], st.summary()
        errs["summary"] = relerr([rec["LAI_min"], rec["LAI_mean"], rec["LAI_max"]], [s["LAI_min"], s["LAI_mean"], s["LAI_max"]])
        print(case, d, {k: f"{e:.2e}" for k, e in errs.items()})
        assert rec["step"] == d + 1
        for k, e in errs.items():
            assert e <= BOUND, (case, d, k, e)
        assert np.array_equal(got["age_days"], st.age) and np.all(got["LAI_layers_SK"][:, :, ~land] == 0.0)
        if case == "no_land":
            assert rec == {"step": d + 1, "LAI_min": 0.0, "LAI_mean": 0.0, "LAI_max": 0.0} and not got["LAI_layers_SK"].any()
    if land.any():
        assert np.abs(st.layers - L0).max() > 1e-3
    dev.close()
