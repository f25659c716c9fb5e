"""GPU (-m gpu): saving and resuming the vegetation state.  qd_eco_state_restore in its f32 and f64 forms against the goldens of the
reference's own load_autosave, for every case, and the sub-daily step and the daily firing that follow the load; the exact resume
of QD_ECO_PERSIST=2 on a second handle, with spread and individuals; the driver run twice in one working directory.

Tolerances.  The restore is one clip, one divide and one multiply per plane in IEEE arithmetic, and ECO_LAI is their sum in a fixed
order: one answer, tolerance 0 (np.array_equal, NaN matching NaN).  The sub-daily step that follows is held to what
tests/test_gpu_ecology.py holds it to -- 1e-15 absolute on the canopy factor, the alpha map and the banded albedo (one device exp,
values in [0, 1]), 1e-14 relative on E_day -- and the daily firing to the BOUND of tests/test_gpu_eco_daily.py (3.3e-15 relative to
the array's scale, ages exact).  The resume compares two handles of this build with each other: bit-equal.
"""
import ctypes
import glob
import os
import re

import numpy as np
import pytest

import eco_state_ref as ref

pytestmark = pytest.mark.gpu

HERE = os.path.dirname(os.path.abspath(__file__))
GOLD = os.path.join(HERE, "golden")
GOLDENS = sorted(p for p in glob.glob(os.path.join(GOLD, "eco_state_*_f*_*x*.npz")) if "mismatch" not in p)
SUB_ABS, EDAY_REL, DAILY_BOUND = 1e-15, 1e-14, 3.3e-15


def _case(p):
    return "_".join(os.path.basename(p).split("_")[2:4])


def dev_of(a, b):
    """max |a - b| / max |b| over the entries finite in b; the others must be the same NaN / inf."""
    a, b = np.asarray(a, dtype=float), np.asarray(b, dtype=float)
    fin = np.isfinite(b)
    assert np.array_equal(a[~fin], b[~fin], equal_nan=True), "non-finite entries differ"
    if not fin.any():
        return 0.0
    return float(np.max(np.abs(a[fin] - b[fin]))) / max(float(np.max(np.abs(b[fin]))), 1e-300)


def abs_of(a, b):
    a, b = np.asarray(a, dtype=float), np.asarray(b, dtype=float)
    assert np.array_equal(np.isnan(a), np.isnan(b)), "NaN entries differ"
    return float(np.nanmax(np.abs(a - b))) if np.isfinite(b).any() else 0.0


def _clean_env(monkeypatch, env=None):
    for k in [k for k in os.environ if k.startswith(("QD_ECO_", "QD_PHYTO_"))]:
        monkeypatch.delenv(k)
    for k, v in (env or {}).items():
        monkeypatch.setenv(str(k), str(v))


def _build(land_mask, daily=True, indiv=False):
    import qingdai_amd as qa
    from qingdai_amd.device import Device
    from qingdai_amd.ecology import EcologyAdapter, IndividualDaily, IndividualPool, PopulationDaily
    grid = qa.SphericalGrid(*land_mask.shape)
    dev = Device(grid)
    dev.upload_now("LAND_MASK", land_mask)
    eco = EcologyAdapter(grid, land_mask, dev=dev, albedo_couple=True)
    if daily:
        PopulationDaily(eco.pop)
    pool = None
    if indiv:
        pool = IndividualPool(grid, land_mask, eco, sample_frac=0.1, per_cell=40)
        IndividualDaily(pool, eco.pop)
    return dev, eco, eco.pop, pool


def _file_of(z, tmp_path):
    """The golden's file arrays as the file the reference would have read: NetCDF for float32, NPZ for float64."""
    from qingdai_amd import ncio
    arrays = {k[5:]: z[k] for k in z.files if k.startswith("file_")}
    if arrays["LAI"].dtype == np.float32:
        path = str(tmp_path / "ecology.nc")
        S, NB = arrays["R_species_nb"].shape
        ncio.write_nc(path, {"lat": arrays["LAI"].shape[0], "lon": arrays["LAI"].shape[1], "species": S, "band": NB},
                      {"LAI": ("f4", ("lat", "lon"), arrays["LAI"]), "species_weights": ("f4", ("species",), arrays["species_weights"]),
                       "bands_lambda_centers": ("f4", ("band",), arrays["bands_lambda_centers"]),
                       "R_species_nb": ("f4", ("species", "band"), arrays["R_species_nb"])}, dict(ref.NC_ATTRS))
    else:
        path = str(tmp_path / "ecology.npz")
        np.savez(path, **arrays)
    return path


@pytest.mark.parametrize("path", GOLDENS, ids=_case)
def test_restore_and_following_steps_vs_reference_goldens(gpu, path, monkeypatch, tmp_path):
    z = np.load(path)
    case = _case(path)
    _clean_env(monkeypatch, {**dict(zip(z["env_keys"], z["env_vals"])), "QD_ECO_DIAG": "0"})
    dev, eco, pop, _ = _build(z["land_mask"])
    S, K = z["load_LAI_layers_SK"].shape[:2]
    assert pop.daily.species_modes == [str(m) for m in z["modes"]] and (pop.Ns, pop.K) == (S, K)
    age0, bank0 = np.random.default_rng(5).uniform(0.0, 7.0, (2,) + pop.shape)
    dev.upload_now("ECO_AGE", age0)
    dev.upload_now("ECO_SEEDBANK", bank0)
    # 1. the kernel itself: the stack where it lives and ECO_LAI, bit for bit
    lai = z["file_LAI"]
    dev.eco_state_restore(lai, z["load_species_weights"].astype(np.float64), K, float(z["lai_max"]))
    stack = dev.eco_daily_get_layers(S, K)
    assert np.array_equal(stack, z["load_LAI_layers_SK"], equal_nan=True), case
    assert np.array_equal(pop.total_LAI(), z["load_total_LAI"], equal_nan=True), case
    other = ref.load_rule(lai.astype(np.float64 if lai.dtype == np.float32 else np.float32), z["load_species_weights"], K, float(z["lai_max"]))[2]
    assert not np.array_equal(stack, other, equal_nan=True)     # the other form's arithmetic would not have passed
    assert np.array_equal(pop.age_days, age0) and np.array_equal(pop.seed_bank, bank0)            # untouched, as in the reference
    # 2. the same through the class seam, from the file the reference would have read
    pop.push_layers(np.zeros((S, K) + pop.shape))
    assert eco.load_autosave(_file_of(z, tmp_path)) is True
    assert np.array_equal(pop.LAI_layers_SK, z["load_LAI_layers_SK"], equal_nan=True)
    assert np.array_equal(pop.total_LAI(), z["load_total_LAI"], equal_nan=True)
    assert pop.species_weights.dtype == z["load_species_weights"].dtype and np.array_equal(pop.species_weights, z["load_species_weights"])
    assert np.array_equal(pop._species_R_leaf, z["load_R_leaf"])
    assert np.array_equal(pop.age_days, age0) and np.array_equal(pop.seed_bank, bank0)            # put back behind the lane's configure
    # 3. the sub-daily step that follows
    pop.seed_bank = np.zeros(pop.shape)
    dev.upload_now("ECO_AGE", np.zeros(pop.shape))
    alpha = eco.step_subdaily(z["isr"], None, 300.0)
    A, w_b = eco.get_surface_albedo_bands()
    dev._host.pop("ECO_F", None)
    errs = {"alpha": abs_of(alpha, z["sub_alpha"]), "A_bands": abs_of(A, z["sub_A_bands"]), "f": abs_of(dev.get("ECO_F"), z["sub_f"])}
    e_day = dev_of(pop.E_day, z["sub_E_day"])
    print(case, "sub-daily", {k: f"{e:.2e}" for k, e in errs.items()}, f"E_day {e_day:.2e}")
    assert max(errs.values()) < SUB_ABS and e_day < EDAY_REL and np.array_equal(w_b, z["sub_w_b"])
    # 4. the daily firing that follows
    pop.step_daily(z["soil"])
    got = {"LAI_layers_SK": pop.LAI_layers_SK, "total_LAI": pop.total_LAI(), "seed_bank": pop.seed_bank, "spread_gate": pop._spread_gate}
    errs = {k: dev_of(v, z["day_" + k]) for k, v in got.items()}
    print(case, "daily", {k: f"{e:.2e}" for k, e in errs.items()})
    for k, e in errs.items():
        assert e <= DAILY_BOUND, (case, k, e)
    assert np.array_equal(pop.age_days, z["day_age_days"]) and np.all(pop.E_day == 0.0)
    dev.close()


def test_restore_without_a_daily_lane_and_refusals(gpu, monkeypatch):
    import qingdai_amd as qa
    from qingdai_amd._lib import QdError
    from qingdai_amd.device import Device
    z = np.load(os.path.join(GOLD, "eco_state_mixed_f32_19x36.npz"))
    _clean_env(monkeypatch, dict(zip(z["env_keys"], z["env_vals"])))
    dev, eco, pop, _ = _build(z["land_mask"], daily=False)
    w = z["load_species_weights"].astype(np.float64)
    dev.eco_state_restore(z["file_LAI"], w, 2, 5.0)             # no resident stack: ECO_LAI alone
    assert np.array_equal(pop.total_LAI(), z["load_total_LAI"], equal_nan=True)
    with pytest.raises(QdError, match="n_layers out of range"):
        dev.eco_state_restore(z["file_LAI"], w, 9, 5.0)
    with pytest.raises(QdError, match="n_species out of range"):
        dev.eco_state_restore(z["file_LAI"], np.full(65, 1 / 65), 2, 5.0)
    with pytest.raises(ValueError, match="LAI plane"):
        dev.eco_state_restore(z["file_LAI"][:5], w, 2, 5.0)
    from qingdai_amd.ecology import PopulationDaily
    PopulationDaily(pop)
    with pytest.raises(QdError, match="not the resident stack's"):
        dev.eco_state_restore(z["file_LAI"], w, 1, 5.0)
    dev.close()
    band = Device(qa.SphericalGrid(73, 144), row0=20, n_rows=30, halo=6)
    plane = np.zeros((73, 144), dtype=np.float32)
    rc = band.lib.qd_eco_state_restore(band.h, plane.ctypes.data, 1, w.ctypes.data_as(ctypes.POINTER(ctypes.c_double)), 3, 2, 5.0)
    assert rc != 0 and b"latitude bands are not supported" in band.lib.qd_last_error(band.h)
    band.close()


def _fire(eco, pop, pool, soil, E_day=None, E_indiv=None):
    if E_day is not None:
        pop.E_day = E_day
    pop.step_daily(soil)
    if E_indiv is not None:
        pool.reset(E_indiv, pool.indiv_water_stress_days)
    pool.step_daily(eco, soil)


def _state(pop, pool):
    E, st = pool._pull()
    return {"LAI_layers_SK": pop.LAI_layers_SK.copy(), "ECO_LAI": pop.total_LAI(), "age_days": pop.age_days, "seed_bank": pop.seed_bank,
            "species_weights": np.array(pop.species_weights), "indiv_E_day": E, "indiv_stress_days": st}


def test_exact_resume_on_a_second_handle(gpu, monkeypatch, tmp_path):
    """Handle A fires three daily steps (vegetation with spread, then the individuals) and saves after the first -- once at level 2,
    once at level 1; fresh handles load and fire the other two."""
    from qingdai_amd import ncio
    z = np.load(os.path.join(GOLD, "eco_state_mixed_f64_19x36.npz"))
    env = {**dict(zip(z["env_keys"], z["env_vals"])), "QD_ECO_DIAG": "0", "QD_ECO_LAI_INIT": "0.6"}
    _clean_env(monkeypatch, env)
    land = z["land_mask"]
    rng = np.random.default_rng(77)
    soil = rng.uniform(0.0, 0.9, (3,) + land.shape)
    E_days = rng.uniform(2.0e3, 2.0e4, (3,) + land.shape)
    dev_a, eco_a, pop_a, pool_a = _build(land, indiv=True)
    E_ind = rng.uniform(0.0, 5.0e3, (3, pool_a.n_indiv))
    pop_a.push_layers(rng.uniform(0.0, 0.6, pop_a.LAI_layers_SK.shape) * (land == 1), init=True)
    pool_a.reset(None, rng.integers(0, 6, pool_a.n_indiv).astype(float))
    _fire(eco_a, pop_a, pool_a, soil[0], E_days[0], E_ind[0])
    eco_a.step_subdaily(z["isr"], None, 300.0)                  # E_day, the individuals' buffers and the clocks are not at rest
    pool_a.try_substep(z["isr"] * 0.5, z["isr"] * 0.5, eco_a, np.clip(soil[0], 0, 1), 300.0)
    pop_a.daily.accum_day = 1234.5
    p2, p1 = str(tmp_path / "two" / "ecology.nc"), str(tmp_path / "one" / "ecology.nc")
    assert eco_a.save_autosave(p2, 1.0, extended=True, indiv=pool_a) and eco_a.save_autosave(p1, 1.0, extended=False)
    saved = _state(pop_a, pool_a)
    saved_clock, saved_eday = pop_a.state(), pop_a.E_day
    assert saved["age_days"].max() >= 1.0 and saved["seed_bank"].max() > 0 and saved_eday.max() > 0 and saved["indiv_stress_days"].max() > 0
    _fire(eco_a, pop_a, pool_a, soil[1])                        # day 2 on the E_day the sub-step left
    _fire(eco_a, pop_a, pool_a, soil[2], E_days[2], E_ind[2])
    want = _state(pop_a, pool_a)
    dev_a.close()

    # B: a fresh handle starts from QD_ECO_LAI_INIT; the level-2 file puts everything back
    dev_b, eco_b, pop_b, pool_b = _build(land, indiv=True)
    assert not np.array_equal(pop_b.LAI_layers_SK, saved["LAI_layers_SK"])
    assert eco_b.load_autosave(p2, indiv=pool_b) is True
    got = _state(pop_b, pool_b)
    for k in saved:
        assert np.array_equal(got[k], saved[k]), ("after the load", k)
    clock = pop_b.state()
    assert (clock["hours"], clock["next_recompute_hours"], clock["step_count"]) == (saved_clock["hours"], saved_clock["next_recompute_hours"], saved_clock["step_count"])
    assert np.array_equal(pop_b.E_day, saved_eday) and pop_b.daily.accum_day == 1234.5
    _fire(eco_b, pop_b, pool_b, soil[1])
    _fire(eco_b, pop_b, pool_b, soil[2], E_days[2], E_ind[2])
    got = _state(pop_b, pool_b)
    for k in want:
        assert np.array_equal(got[k], want[k]), ("two firings after the resume", k)
    dev_b.close()

    # C: the level-1 file holds the reference's variables alone -> the reference rule; age and seed bank are not the load's business
    v, _ = ncio.read_nc(p1)
    assert not [k for k in v if k.startswith("qd_")] and v["LAI"].dtype == np.float32
    dev_c, eco_c, pop_c, pool_c = _build(land, indiv=True)
    age0, bank0 = rng.uniform(0.0, 7.0, (2,) + land.shape)
    dev_c.upload_now("ECO_AGE", age0)
    dev_c.upload_now("ECO_SEEDBANK", bank0)
    assert eco_c.load_autosave(p1, indiv=pool_c) is True
    L, sw, stack, tot = ref.load_rule(v["LAI"], v["species_weights"], pop_c.K, 5.0)
    assert np.array_equal(pop_c.LAI_layers_SK, stack) and np.array_equal(pop_c.total_LAI(), tot) and np.array_equal(pop_c.species_weights, sw)
    assert np.array_equal(pop_c.age_days, age0) and np.array_equal(pop_c.seed_bank, bank0)
    assert not np.array_equal(pop_c.LAI_layers_SK, saved["LAI_layers_SK"])        # one f32 plane does not hold the stack
    dev_c.close()


def test_driver_saves_and_resumes(gpu, tmp_path, monkeypatch, capsys):
    from qingdai_amd import driver, ncio
    for k in [k for k in os.environ if k.startswith("QD_")]:
        monkeypatch.delenv(k)
    env = {"QD_N_LAT": "19", "QD_N_LON": "36", "QD_SIM_DAYS": "1.3", "QD_DYN_DIAG_PRINT": "0", "QD_USE_OCEAN": "0", "QD_HYDRO_ENABLE": "0",
           "QD_PHYTO_ENABLE": "0", "QD_ECO_INDIV_ENABLE": "0", "QD_ECO_DAILY": "1", "QD_ECO_PERSIST": "2", "QD_ECO_COHORT_K": "2",
           "QD_ECO_NS": "3", "QD_ECO_SPREAD_ENABLE": "1", "QD_ECO_SPREAD_RATE": "0.1", "QD_ECO_RAND_SEED": "3", "QD_ECO_AUTOSAVE_KEEP": "2"}
    for k, v in env.items():
        monkeypatch.setenv(k, v)
    monkeypatch.chdir(tmp_path)
    assert driver.main() == 0
    out = capsys.readouterr().out
    assert "[Ecology] autosave load" not in out and "[Ecology] Autosave written: data/ecology.nc" in out
    names = os.listdir(tmp_path / "data")
    assert "ecology.nc" in names and "genes.json" in names
    assert 1 <= len([n for n in names if re.fullmatch(r"ecology_\d{8}T\d{6}Z\.nc", n)]) <= 2
    v, _ = ncio.read_nc(str(tmp_path / "data" / "ecology.nc"))
    assert v["qd_LAI_layers_SK"].shape == (3, 2, 19, 36) and v["qd_age_days"].max() == 1.0 and float(v["qd_accum_day"]) > 0
    seen = {}
    boot = driver.Simulation.bootstrap_ecology

    def spy(sim):                                               # behind the loads, before the first step
        seen["stack"], seen["age"], seen["accum"] = sim.eco.pop.LAI_layers_SK.copy(), sim.eco.pop.age_days, sim.eco_daily.accum_day
        return boot(sim)
    monkeypatch.setattr(driver.Simulation, "bootstrap_ecology", spy)
    assert driver.main() == 0
    out = capsys.readouterr().out
    assert "[Ecology] autosave load OK from 'data/ecology.nc'" in out and "exact resume from the qd_* extension variables" in out
    assert np.array_equal(seen["stack"], v["qd_LAI_layers_SK"]) and np.array_equal(seen["age"], v["qd_age_days"])
    assert seen["accum"] == float(v["qd_accum_day"])
    assert len([n for n in os.listdir(tmp_path / "data") if re.fullmatch(r"ecology_\d{8}T\d{6}Z\.nc", n)]) <= 2
    # without the switch: neither file, no line
    monkeypatch.undo()
    for k in [k for k in os.environ if k.startswith("QD_")]:
        monkeypatch.delenv(k)
    for k, v_ in env.items():
        if k != "QD_ECO_PERSIST":
            monkeypatch.setenv(k, v_)
    monkeypatch.setenv("QD_DATA_DIR", str(tmp_path / "plain"))
    monkeypatch.setenv("QD_SIM_DAYS", "0.3")
    monkeypatch.chdir(tmp_path)
    assert driver.main() == 0
    out = capsys.readouterr().out
    assert "[Ecology] autosave" not in out and "[Ecology] Autosave" not in out
    assert "atmosphere.nc" in os.listdir(tmp_path / "plain") and not [n for n in os.listdir(tmp_path / "plain") if n.startswith(("ecology", "genes"))]
