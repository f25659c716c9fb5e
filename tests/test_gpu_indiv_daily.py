"""GPU (-m gpu): IndividualPool.step_daily on the device (qd_indiv_daily_*, behind every firing of the bit9 lane): the class seam
against the reference's goldens over both days, one qd_step_n span against the same steps cut at the day boundaries with seam
calls, several firings in one step, the switch off, QD_ECO_F32=1, degenerate pools and row lengths against the NumPy
restatement, the refusals, the driver's lines, and one 721 x 1440 firing with the default pool.

Tolerance.  The goldens of the reference's own classes are the yardstick; deviations are max |a - b| / max |b| per array over the
entries that are finite in the golden (NaN and inf must sit where the golden has them).  The starting bound is the 1e-14 that
tests/test_gpu_eco_daily.py starts from; the bound in force is ten times the largest deviation measured on the MI355X over all
cases, arrays and both days, never looser than the start (MEASURED and BOUND below; the margin covers the blocked land sums of the
species weights against NumPy's pairwise nansum and the device exp of the vegetation step in front).  Stress days and the E_day
reset must be exact.  Every test prints its deviations."""
import ctypes
import glob
import os

import numpy as np
import pytest

import eco_daily_ref as pref
import indiv_daily_ref as iref

pytestmark = pytest.mark.gpu

HERE = os.path.dirname(os.path.abspath(__file__))
GOLDENS = sorted(glob.glob(os.path.join(HERE, "golden", "indiv_daily_*_19x36.npz")))
START = 1e-14
MEASURED = 4.1e-16                 # largest deviation from the goldens on the MI355X (4.003e-16, `wide`, rounded up; `full` 3.79e-16)
BOUND = START if MEASURED is None else min(START, 10 * MEASURED)


def _case(path):
    return os.path.basename(path)[12:-10]


def dev_of(a, b):
    """max |a - b| / max |b| over the entries finite in b; the others must be the same NaN / inf."""
    a, b = np.asarray(a, dtype=float), np.asarray(b, dtype=float)
    fin = np.isfinite(b)
    assert np.array_equal(a[~fin], b[~fin], equal_nan=True), "non-finite entries differ"
    if not fin.any():
        return 0.0
    return float(np.max(np.abs(a[fin] - b[fin]))) / max(float(np.max(np.abs(b[fin]))), 1e-300)


def _clean_env(monkeypatch, env=None):
    for k in [k for k in os.environ if k.startswith(("QD_ECO_", "QD_PHYTO_"))]:
        monkeypatch.delenv(k)
    for k, v in (env or {}).items():
        monkeypatch.setenv(str(k), str(v))


def _build(land_mask, with_daily=True):
    """-> (dev, eco, pop, pool) with the vegetation step and the individuals' step configured from the environment."""
    import qingdai_amd as qa
    from qingdai_amd.device import Device
    from qingdai_amd.ecology import EcologyAdapter, IndividualDaily, IndividualPool, PopulationDaily
    grid = qa.SphericalGrid(*land_mask.shape)
    dev = Device(grid)
    dev.upload_now("LAND_MASK", land_mask)
    eco = EcologyAdapter(grid, land_mask, dev=dev, albedo_couple=True)
    PopulationDaily(eco.pop)
    pool = IndividualPool(grid, land_mask, eco, sample_frac=0.02, per_cell=150)
    if with_daily:
        IndividualDaily(pool, eco.pop)
    return dev, eco, eco.pop, pool


def _from_golden(z, monkeypatch, extra=None):
    _clean_env(monkeypatch, {**dict(zip(z["env_keys"], z["env_vals"])), **(extra or {})})
    dev, eco, pop, pool = _build(z["land_mask"])
    assert np.array_equal(pool.sample_j, z["sample_j"]) and np.array_equal(pool.sample_i, z["sample_i"])
    assert np.array_equal(pool.indiv_species_id, z["species_id"]) and np.array_equal(pool.indiv_tol, z["indiv_tol"])
    assert np.array_equal(pool.daily.levels, z["levels"])
    pop.push_layers(z["L0"], init=True)
    pop.seed_bank = z["bank0"]
    pool.reset(None, z["stress0"])
    return dev, eco, pop, pool


def _day(z, d, eco, pop, pool):
    pop.E_day = z["E_days"][d]
    pop.step_daily(z["soil"][d])
    pool.reset(z["E_indiv"][d], pool.indiv_water_stress_days)
    pool.step_daily(eco, z["soil"][d], Ts_map=None, day_length_hours=24.0)


def _state(pop, pool):
    E, st = pool._pull()
    return {"LAI_layers_SK": pop.LAI_layers_SK.copy(), "LAI": pop.total_LAI(), "seed_bank": pop.seed_bank,
            "species_weights": np.array(pop.species_weights), "stress_days": st, "E_indiv": E}


@pytest.mark.parametrize("path", GOLDENS, ids=_case)
def test_class_seam_vs_reference_goldens(gpu, path, monkeypatch):
    z = np.load(path)
    case = _case(path)
    dev, eco, pop, pool = _from_golden(z, monkeypatch)
    before = pop.state()
    worst = 0.0
    for d in range(2):
        _day(z, d, eco, pop, pool)
        got = _state(pop, pool)
        rec = pool.daily.log()[-1]
        errs = {k: dev_of(v, z[f"day{d + 1}_{k}"]) for k, v in got.items()}
        errs["beta_hint"] = dev_of(rec["beta_hint"], z[f"day{d + 1}_beta_hint"])
        print(case, d + 1, {k: f"{e:.2e}" for k, e in errs.items()})
        worst = max(worst, max(errs.values()))
        assert (rec["step"], rec["n_cells"], rec["levels"]) == (d + 1, len(z["sample_j"]), int(z["levels"].max()))
        assert pool.daily.lines([rec])[0] == str(z["lines"][d])
        for k, e in errs.items():
            assert e <= BOUND, (case, d + 1, k, e)
        assert np.all(got["E_indiv"] == 0.0) and np.array_equal(got["stress_days"], z[f"day{d + 1}_stress_days"])
    print(f"{case}: largest deviation from the reference {worst:.3e} (bound {BOUND:.1e})")
    after = pop.state()                                         # the canopy snapshot and its clock are untouched by a firing
    assert (after["hours"], after["next_recompute_hours"], after["n_recompute"]) == (before["hours"], before["next_recompute_hours"], before["n_recompute"])
    assert dev.indiv_daily_firings() == 2 == dev.eco_daily_firings()
    dev.close()


def test_f32_maps_store_the_f64_total_rounded_once(gpu, monkeypatch):
    z = np.load(os.path.join(HERE, "golden", "indiv_daily_full_19x36.npz"))
    out = {}
    for f32 in ("0", "1"):
        dev, eco, pop, pool = _from_golden(z, monkeypatch, {"QD_ECO_F32": f32})
        _day(z, 0, eco, pop, pool)
        out[f32] = _state(pop, pool)
        dev.close()
    a, b = out["0"], out["1"]
    for k in ("LAI_layers_SK", "seed_bank", "species_weights", "stress_days", "E_indiv"):
        assert np.array_equal(a[k], b[k]), k
    assert np.array_equal(b["LAI"], a["LAI"].astype(np.float32).astype(np.float64)) and not np.array_equal(b["LAI"], a["LAI"])


# ---------------------------------------------------------------------------------------------------------------- the lane
LANE_ENV = {"QD_ECO_NS": "4", "QD_ECO_COHORT_K": "2", "QD_ECO_LAI_GROWTH": "4e-8", "QD_ECO_SPREAD_ENABLE": "1", "QD_ECO_SPREAD_RATE": "0.1",
            "QD_ECO_SEED_ENERGY": "2e4", "QD_ECO_RAND_SEED": "2", "QD_ECO_LIGHT_UPDATE_EVERY_HOURS": "1", "QD_ECO_DAILY": "1",
            "QD_ECO_INDIV_SAMPLE_FRAC": "0.3", "QD_ECO_INDIV_PER_CELL": "6", "QD_ECO_LAI_GROWTH_RATE": "0.05", "QD_ECO_INDIV_SUBSTEPS_PER_DAY": "48"}
NAMES = ("U", "V", "H", "TS", "Q", "CLOUD", "HICE", "W_LAND", "S_SNOW", "ALBEDO", "ECO_LAI", "ECO_EDAY", "ECO_ALPHA", "ECO_F", "ECO_AGE",
         "ECO_SEEDBANK", "ECO_GATE")


def _sim(monkeypatch, env, day=7000.0):
    import qingdai_amd as qa
    from qingdai_amd.driver import Simulation
    _clean_env(monkeypatch, env)
    nlat, nlon = 37, 72
    sim = Simulation(nlat, nlon, params=qa.QdParams(), use_ocean=False, quiet=True)
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


def _fields(sim, names=NAMES):
    for k in names:
        sim.dev._host.pop(k, None)
    return {k: sim.dev.get(k).copy() for k in names}


def _all(sim):
    out = _fields(sim)
    out["layers"] = sim.eco.pop.LAI_layers_SK.copy()
    out["indiv_E"], out["indiv_stress"] = sim.indiv._pull()
    if sim.indiv_daily is not None:
        out["weights"] = np.array(sim.eco.pop.species_weights)
    return out


def _seam_firing(sim):
    f = _fields(sim, ("W_LAND", "GLACIER"))
    soil = pref.soil_index(f["W_LAND"], f["GLACIER"], 50.0)
    sim.eco.pop.step_daily(soil)
    sim.indiv.step_daily(sim.eco, soil)


def test_span_vs_seam_calls_cut_at_the_boundaries(gpu, monkeypatch):
    """One qd_step_n span of 60 steps crossing two (shortened) day boundaries with the switch on, against the same steps cut at
    the boundaries with the two seam calls made from the host: bit-identical state, individuals and both logs."""
    env = {**LANE_ENV, "QD_ECO_INDIV_DAILY": "1"}
    span = _sim(monkeypatch, env)
    assert span.indiv_daily is not None and span.indiv.n_cells > 10
    span.run_steps(60)
    assert span.dev.indiv_daily_firings() == 2 == span.dev.eco_daily_firings()
    seam = _sim(monkeypatch, env, day=1.0e12)                   # the lane never fires by itself
    fire, _ = __import__("qingdai_amd.ecology", fromlist=["daily_counts"]).daily_counts(0.0, seam.dt, 60, 7000.0)
    for s in range(60):
        for _ in range(int(fire[s])):                           # the firing sits at the top of step s
            _seam_firing(seam)
        seam.run_steps(1)
    assert int(fire.sum()) == 2
    a, b = _all(span), _all(seam)
    for k in a:
        assert np.array_equal(a[k], b[k], equal_nan=True), k
    assert span.eco.pop.state() == seam.eco.pop.state()
    # the logs were drained by the driver after its chunks; the next firing's records agree and carry the count
    _seam_firing(span); _seam_firing(seam)
    assert span.eco_daily.log() == seam.eco_daily.log() and span.indiv_daily.log() == seam.indiv_daily.log()
    span.dev.close(); seam.dev.close()


def test_two_and_three_firings_in_one_step_vs_seam_call_pairs(gpu, monkeypatch):
    env = {**LANE_ENV, "QD_ECO_INDIV_DAILY": "1"}
    span, seam = _sim(monkeypatch, env, day=1.0e12), _sim(monkeypatch, env, day=1.0e12)
    for s in (span, seam):
        s.eco.pop.seed_bank = np.where(s.land_mask == 1, 0.5, 0.0)
        s.run_steps(3)
    span.eco_daily.day_seconds, span.eco_daily.accum_day = span.dt / 2.5, 0.0
    keep = {"pop": [], "ind": []}
    drain_p, drain_i = span.dev.eco_daily_log, span.dev.indiv_daily_log
    span.dev.eco_daily_log = lambda: (lambda o: (keep["pop"].extend(o.tolist()), o)[1])(drain_p())
    span.dev.indiv_daily_log = lambda: (lambda o: (keep["ind"].extend(o.tolist()), o)[1])(drain_i())
    want_p, want_i, total = [], [], 0
    for want in (2, 3):
        span.run_steps(1)
        for _ in range(want):
            _seam_firing(seam)
        want_p += seam.dev.eco_daily_log().tolist(); want_i += seam.dev.indiv_daily_log().tolist()
        seam.run_steps(1)
        total += want
        assert span.dev.indiv_daily_firings() == total == seam.dev.indiv_daily_firings() == span.dev.eco_daily_firings()
        a, b = _all(span), _all(seam)
        for k in a:
            assert np.array_equal(a[k], b[k], equal_nan=True), (want, k)
    assert keep["pop"] == want_p and keep["ind"] == want_i and [r[0] for r in keep["ind"]] == [1, 2, 3, 4, 5]
    span.dev.close(); seam.dev.close()


def test_switch_off_changes_nothing(gpu, monkeypatch):
    """QD_ECO_INDIV_DAILY unset or 0: no configuration on the device, the lane's span is what it was (fields, stack, individuals,
    log records), and the individuals' buffers keep accumulating."""
    runs = {}
    for tag, env in (("unset", LANE_ENV), ("zero", {**LANE_ENV, "QD_ECO_INDIV_DAILY": "0"})):
        sim = _sim(monkeypatch, env)
        assert sim.indiv_daily is None and sim.eco_daily is not None
        recs = []
        drain = sim.dev.eco_daily_log
        sim.dev.eco_daily_log = lambda d=drain, r=recs: (lambda o: (r.extend(o.tolist()), o)[1])(d())
        sim.run_steps(30)
        assert sim.dev.indiv_daily_firings() == 0 and sim.dev.eco_daily_firings() == 1
        with pytest.raises(Exception, match="qd_indiv_daily_configure has not been called"):
            sim.dev.indiv_daily_log()
        runs[tag] = (_all(sim), recs)
        sim.dev.close()
    for k in runs["unset"][0]:
        assert np.array_equal(runs["unset"][0][k], runs["zero"][0][k], equal_nan=True), k
    assert runs["unset"][1] == runs["zero"][1] and len(runs["zero"][1]) == 1
    assert runs["zero"][0]["indiv_E"].max() > 0.0               # nothing consumed them


# ---------------------------------------------------------------------------------------------------------------- other shapes
def _shape_masks():
    r = np.random.default_rng(23)
    one = np.zeros((9, 24), np.uint8); one[4, 11] = 1
    return {"no_land": (np.zeros((9, 24), np.uint8), "1.0"), "one_sampled_cell": (one, "1.0"),
            "nlon20": ((r.random((7, 20)) < 0.6).astype(np.uint8), "0.6"), "nlon100": ((r.random((9, 100)) < 0.6).astype(np.uint8), "0.5")}


SHAPE_ENV = {"QD_ECO_NS": "9", "QD_ECO_COHORT_K": "2", "QD_ECO_INDIV_PER_CELL": "11", "QD_ECO_LAI_GROWTH_RATE": "0.05", "QD_ECO_SEED_ENERGY": "300",
             "QD_ECO_SPREAD_ENABLE": "0"}


@pytest.mark.parametrize("case", list(_shape_masks()))
def test_other_shapes_vs_restatement(gpu, monkeypatch, case):
    """Two days on pools and row lengths where an indexing slip shows: no land (the reference still samples max(1, 0) cells from
    none: refused), one sampled cell (the [S, 1] tables are one contiguous run), rows shorter than a wavefront and no multiple
    of 64.  S = 9 on K = 2; the vegetation step in front has no spread, so no device exp reaches the stack and everything but
    the weights is bitwise."""
    mask, frac = _shape_masks()[case]
    _clean_env(monkeypatch, {**SHAPE_ENV, "QD_ECO_INDIV_SAMPLE_FRAC": frac})
    land = mask == 1
    if case == "no_land":
        with pytest.raises(Exception):
            _build(mask)
        return
    dev, eco, pop, pool = _build(mask)
    r = np.random.default_rng(sum(map(ord, case)))
    S, K, N = pop.Ns, pop.K, pool.n_indiv
    L0 = r.uniform(0.0, 0.2, (S, K) + mask.shape) * land
    bank0 = r.uniform(0.0, 2.0, mask.shape) * land
    pop.push_layers(L0, init=True)
    pop.seed_bank = bank0
    stress = r.uniform(0.0, 3.0, N)
    pool.reset(None, stress)
    env = dict(os.environ)
    pcfg = pref.Cfg.from_env(env, pop.daily.species_modes, np.array(pop.species_weights))
    pst = pref.State(land, L0.copy(), None, np.zeros(mask.shape), bank0.copy(), land.astype(float))
    ist = iref.State(land, None, None, pool.sample_j, pool.sample_i, pool.per_cell, pool.indiv_species_id, pool.indiv_tol, None, stress.copy())
    for d in range(2):
        Eg, soil, Ei = r.uniform(0.0, 2.0e4, mask.shape), r.uniform(0.0, 0.9, mask.shape), r.uniform(0.0, 2.0e3, N)
        pop.E_day = Eg
        pop.step_daily(soil)
        pool.reset(Ei, pool.indiv_water_stress_days)
        pool.step_daily(eco, soil)
        pst.E_day = Eg.copy()
        pref.step_daily(pst, pcfg, soil)
        ist.layers, ist.bank, ist.E = pst.layers, pst.bank, Ei.copy()
        info = iref.step_daily(ist, iref.Cfg.from_env(env), soil, pool.daily.levels)
        pst.layers, pst.bank = ist.layers, ist.bank
        pcfg.weights = ist.weights
        got = _state(pop, pool)
        want = {"LAI_layers_SK": ist.layers, "LAI": ist.LAI, "seed_bank": ist.bank, "species_weights": ist.weights, "stress_days": ist.stress,
                "E_indiv": ist.E}
        errs = {k: dev_of(got[k], want[k]) for k in want}
        rec = pool.daily.log()[-1]
        errs["beta_hint"] = dev_of(rec["beta_hint"], info["beta_hint"])
        print(case, d + 1, {k: f"{e:.2e}" for k, e in errs.items()})
        for k, e in errs.items():
            assert e <= BOUND, (case, d + 1, k, e)
        assert np.array_equal(got["stress_days"], ist.stress) and np.all(got["E_indiv"] == 0.0)
    assert np.abs(ist.layers - L0).max() > 1e-4
    dev.close()


# ---------------------------------------------------------------------------------------------------------------- refusals
def test_refusals_and_log_overflow(gpu, monkeypatch):
    import qingdai_amd as qa
    from qingdai_amd._lib import QdError, SPAN_LOG_CAP, qd_indiv_daily_params
    from qingdai_amd.device import Device
    from qingdai_amd.ecology import EcologyAdapter, IndividualDaily, IndividualPool, PopulationDaily
    z = np.load(os.path.join(HERE, "golden", "indiv_daily_sparse_19x36.npz"))
    _clean_env(monkeypatch, dict(zip(z["env_keys"], z["env_vals"])))
    land = z["land_mask"]
    grid = qa.SphericalGrid(*land.shape)
    dev = Device(grid)
    dev.upload_now("LAND_MASK", land)
    eco = EcologyAdapter(grid, land, dev=dev, albedo_couple=True)
    dp, ip = ctypes.POINTER(ctypes.c_double), ctypes.POINTER(ctypes.c_int32)
    params = qd_indiv_daily_params(n_species=3, n_layers=1, per_cell=7, seed_couple=1, stress_penalty=0.2, lai_grow=0.002, lai_decay=0.001,
                                   recruit_frac=0.2, stress_decay=0.5, repro_frac=0.2, seed_energy=1.0, retain=0.2, bank_max=1000.0, lai_max=5.0)
    sp, lv = np.ascontiguousarray(z["species_id"], dtype=np.int32), np.ascontiguousarray(z["levels"], dtype=np.int32)

    def configure(p=params, size=None, species=sp, levels=lv, d=dev):
        rc = d.lib.qd_indiv_daily_configure(d.h, ctypes.byref(p), ctypes.sizeof(p) if size is None else size, species.ctypes.data_as(ip),
                                            levels.ctypes.data_as(ip))
        return rc, (d.lib.qd_last_error(d.h) or b"").decode()

    for fn, what in ((lambda: dev.indiv_daily_step(None), "qd_indiv_daily_step"), (dev.indiv_daily_log, "qd_indiv_daily_log"),
                     (lambda: dev.indiv_daily_weights(3), "qd_indiv_daily_weights")):
        with pytest.raises(QdError, match="qd_indiv_daily_configure has not been called"):
            fn()
    rc, err = configure()
    assert rc != 0 and "qd_indiv_configure has not been called" in err
    pool = IndividualPool(grid, land, eco)
    rc, err = configure()
    assert rc != 0 and "qd_eco_daily_configure has not been called" in err
    with pytest.raises(ValueError, match="needs a population whose daily step runs on the device"):
        IndividualDaily(pool, eco.pop)
    PopulationDaily(eco.pop)
    assert configure(size=8)[0] != 0 and "struct size mismatch" in configure(size=8)[1]
    bad = qd_indiv_daily_params.from_buffer_copy(params); bad.n_species = 4
    assert "are not the stack's" in configure(p=bad)[1]
    bad = qd_indiv_daily_params.from_buffer_copy(params); bad.per_cell = 6
    assert "n_cells * per_cell is not n_indiv" in configure(p=bad)[1]
    s2 = sp.copy(); s2[5] = 3
    assert "species id outside" in configure(species=s2)[1]
    assert "does not keep the order" in configure(levels=np.ones_like(lv))[1]
    l2 = lv.copy(); l2[0] = 0
    assert "level outside" in configure(levels=l2)[1]
    assert dev.indiv_daily_firings() == 0
    rc, err = configure()
    assert rc == 0, err
    with pytest.raises(QdError, match="no firing yet"):
        dev.indiv_daily_weights(3)
    # a span whose firings do not fit into the individuals' log, although they fit into the lane's
    stars = qa.ThermalForcing(grid, qa.OrbitalSystem()).star_table(300.0 * np.arange(4))

    def step_n(n, flags):
        st = np.ascontiguousarray(stars[:n])
        return dev.lib.qd_step_n(dev.h, n, 300.0, flags, st.ctypes.data_as(dp)), (dev.lib.qd_last_error(dev.h) or b"").decode()

    dev.indiv_daily_step(np.full(land.shape, 0.5))              # one record of the individuals', none of the lane's
    dev.eco_daily_schedule(np.array([SPAN_LOG_CAP, 0, 0, 0], dtype=np.int32))
    rc, err = step_n(4, 2 | 32 | 512)
    assert rc != 0 and "would overflow their log" in err
    assert dev.indiv_daily_firings() == 1 and dev.eco_daily_firings() == 0          # refused before anything ran
    buf, n = np.empty(4), ctypes.c_int32(0)
    dev.indiv_daily_step(np.full(land.shape, 0.5))
    assert dev.lib.qd_indiv_daily_log(dev.h, buf.ctypes.data_as(dp), 1, ctypes.byref(n)) != 0
    assert "more records than room" in dev.lib.qd_last_error(dev.h).decode()
    assert [int(r[0]) for r in dev.indiv_daily_log()] == [1, 2] and len(dev.indiv_daily_log()) == 0
    with pytest.raises(QdError, match="n_species is not the configured one"):
        dev.indiv_daily_weights(5)
    # a good span still runs after the refusals, and a new pool or stack drops the configuration
    dev.eco_daily_schedule(np.array([0, 1, 0, 0], dtype=np.int32))
    rc, err = step_n(4, 2 | 32 | 512)
    assert rc == 0, err
    assert [int(r[0]) for r in dev.indiv_daily_log()] == [3] and dev.eco_daily_firings() == 1
    pool.configure()
    assert dev.indiv_daily_firings() == 0
    with pytest.raises(QdError, match="qd_indiv_daily_configure has not been called"):
        dev.indiv_daily_step(None)
    dev.close()
    band = Device(qa.SphericalGrid(73, 144), row0=20, n_rows=30, halo=6)
    rc, err = configure(d=band)
    assert rc != 0 and "latitude bands are not supported" in err
    assert band.lib.qd_indiv_daily_step(band.h, None) != 0 and b"whole-globe" in band.lib.qd_last_error(band.h)
    band.close()


def test_driver_main_prints_one_line_per_firing_and_no_note(gpu, tmp_path, monkeypatch, capsys):
    from qingdai_amd import driver
    for k in [k for k in os.environ if k.startswith("QD_")]:
        monkeypatch.delenv(k)
    env = {"QD_N_LAT": "37", "QD_N_LON": "72", "QD_SIM_DAYS": "3.05", "QD_DATA_DIR": str(tmp_path / "data"), "QD_DYN_DIAG_PRINT": "0",
           "QD_USE_OCEAN": "0", "QD_AUTOSAVE_ENABLE": "0", "QD_HYDRO_ENABLE": "0", "QD_PHYTO_ENABLE": "0", "QD_ECO_DAILY": "1",
           "QD_ECO_INDIV_DAILY": "1", "QD_ECO_NS": "4", "QD_ECO_INDIV_SAMPLE_FRAC": "0.2", "QD_ECO_INDIV_PER_CELL": "8"}
    for k, v in env.items():
        monkeypatch.setenv(k, v)
    monkeypatch.chdir(tmp_path)
    assert driver.main() == 0
    out = capsys.readouterr().out
    lines = [l for l in out.splitlines() if l.startswith("[EcoIndiv] daily applied to ")]
    assert len(lines) == 3 == len([l for l in out.splitlines() if l.startswith("[Ecology] daily: LAI(min/mean/max)=")]), out
    assert all(" cells × 8 indiv; mean max species share per cell ~ 0." in l and l.endswith("(lower→more even).") for l in lines)
    assert "IndividualPool.step_daily is not run" not in out and "[EcoIndiv] daily step on the device:" in out
    # without the switch the note is back and no line is printed; with it and without its lane it is refused
    monkeypatch.delenv("QD_ECO_INDIV_DAILY"); monkeypatch.setenv("QD_SIM_DAYS", "1.05")
    assert driver.main() == 0
    out = capsys.readouterr().out
    assert "[Ecology] note: IndividualPool.step_daily is not run by the device daily step." in out and "[EcoIndiv] daily applied" not in out
    monkeypatch.setenv("QD_ECO_INDIV_DAILY", "1"); monkeypatch.delenv("QD_ECO_DAILY")
    with pytest.raises(ValueError, match="QD_ECO_INDIV_DAILY=1 needs QD_ECO_DAILY=1"):
        driver.main()


def test_full_size_firing_default_pool(gpu, monkeypatch):
    """721 x 1440, the driver's pool (2 % of land, 150 per cell, 20 species, one layer): one firing against the restatement
    within BOUND, two runs bit-identical.  Prints the level count and the kernel-group time."""
    from qingdai_amd.topography import create_land_sea_mask
    import qingdai_amd as qa
    _clean_env(monkeypatch, {"QD_ECO_LAI_GROWTH_RATE": "0.02"})
    mask = create_land_sea_mask(qa.SphericalGrid(721, 1440))
    land = mask == 1
    r = np.random.default_rng(3)
    S, K = 20, 1
    L0 = r.uniform(0.0, 0.15, (S, K, 721, 1440)) * land
    soil = r.uniform(0.0, 0.9, (721, 1440))
    bank0 = r.uniform(0.0, 3.0, (721, 1440)) * land
    runs = []
    for _ in range(2):
        dev, eco, pop, pool = _build(mask)
        N = pool.n_indiv
        Ei, stress = np.random.default_rng(4).uniform(0.0, 2.0e3, N), np.random.default_rng(5).uniform(0.0, 3.0, N)
        assert (pop.Ns, pop.K, pool.per_cell) == (S, K, 150) and pool.n_cells == max(1, int(0.02 * land.sum()))
        pop.push_layers(L0, init=True)
        pop.seed_bank = bank0
        pool.reset(Ei, stress)
        dev.timing(True)
        pool.step_daily(eco, soil)
        dev.sync()
        ms, n = dev.timing_get("indiv_daily")
        runs.append((_state(pop, pool), pool.daily.log()[-1]))
        print(f"721x1440: {pool.n_cells} cells, {N} individuals, {pool.daily.n_levels} levels, firing {ms:.3f} ms ({n} group)")
        levels = pool.daily.levels
        keep = (pool.sample_j, pool.sample_i, pool.indiv_species_id, pool.indiv_tol)
        dev.close()
    for k in runs[0][0]:
        assert np.array_equal(runs[0][0][k], runs[1][0][k]), k
    assert runs[0][1] == runs[1][1]
    ist = iref.State(land, L0.copy(), bank0.copy(), keep[0], keep[1], 150, keep[2], keep[3], Ei.copy(), stress.copy())
    info = iref.step_daily(ist, iref.Cfg.from_env({"QD_ECO_LAI_GROWTH_RATE": "0.02"}), soil, levels)
    got, rec = runs[0]
    want = {"LAI_layers_SK": ist.layers, "LAI": ist.LAI, "seed_bank": ist.bank, "species_weights": ist.weights, "stress_days": ist.stress,
            "E_indiv": ist.E}
    errs = {k: dev_of(got[k], want[k]) for k in want}
    errs["beta_hint"] = dev_of(rec["beta_hint"], info["beta_hint"])
    print("721x1440", {k: f"{e:.2e}" for k, e in errs.items()})
    assert np.abs(ist.layers - L0).max() > 1e-3
    for k, e in errs.items():
        assert e <= BOUND, (k, e)
