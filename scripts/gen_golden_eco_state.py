"""Regenerate tests/golden/eco_state_<case>_<f32|f64>_<grid>.npz and tests/golden/genes_eco_state_mixed.json from the reference's
EcologyAdapter and PopulationManager (pygcm/ecology/adapter.py, population.py).

Needs a checkout of the reference project (default ../reference next to this repository, or --reference DIR) and NumPy >= 2 (the
float32 case records what NumPy's promotion rules make of float32 file arrays).  Each case sets its QD_ECO_* environment, builds the
reference's adapter on a hand-made land mask and loads one autosave file into it:

  f32   netCDF4 is not needed: load_autosave is handed an `.npz` that holds float32 LAI, species_weights, bands_lambda_centers and
        R_species_nb -- the arrays a NetCDF file of the reference's layout yields -- so its arithmetic runs in float32;
  f64   the file is the reference's own NPZ save (save_autosave of a first adapter whose pop.LAI is the case's plane).

Recorded: the file's arrays; after the load LAI, LAI_layers_SK, species_weights, total_LAI() and _species_R_leaf; after one
step_subdaily the alpha map, E_day and get_surface_albedo_bands(); after one step_daily(soil) with spread on the stack, the age,
the seed bank, LAI and total_LAI().  The LAI planes hold negatives, values above lai_max, NaN, +inf, exact zeros, one float32
subnormal (1e-42), values on ocean cells, and land on both pole rows; one case has an all-ocean mask.  Three more files hold a load
with another species count, one with another band count (advanced=NO, with the printed lines) and a malformed file (LAI not 2-D).

tests/eco_state_ref.py must reproduce every load bitwise, and tests/eco_daily_ref.py the daily step; the script asserts both, and
that no finite input of the daily step sits on a branch (see gen_golden_eco_daily.py).
"""
import argparse
import contextlib
import io
import json
import os
import sys
import tempfile

import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))
OUT = os.path.join(HERE, "..", "tests", "golden")
DT = 300.0

SPREAD = {"QD_ECO_SPREAD_ENABLE": "1", "QD_ECO_SPREAD_RATE": "0.1", "QD_ECO_SEED_ENERGY": "200", "QD_ECO_DIAG": "0"}
CASES = {
    # 19 x 36, S = 3, K = 2, mixed spread modes
    "mixed": dict(grid=(19, 36), env={**SPREAD, "QD_ECO_SPECIES_WEIGHTS": "0.5,0.3,0.2", "QD_ECO_COHORT_K": "2",
                                      "QD_ECO_SPECIES_0_MODE": "seed", "QD_ECO_SPECIES_1_MODE": "diffusion", "QD_ECO_SPECIES_2_MODE": "seed",
                                      "QD_ECO_SPECIES_0_PEAKS": "440:35:0.7, 670:25:0.9", "QD_ECO_SPECIES_1_DROUGHT_TOL": "0.45",
                                      "QD_ECO_SPECIES_2_PEAKS": "500:60:0.5", "QD_ECO_SPECIES_2_IDENTITY": "shrub",
                                      "QD_ECO_SPECIES_1_ALLOC_ROOT": "0.5", "QD_ECO_SPECIES_2_LIFESPAN_DAYS": "900"}),
    # the default population: 20 species, one layer
    "ns20": dict(grid=(19, 36), env={**SPREAD, "QD_ECO_RAND_SEED": "7"}),
    "k8": dict(grid=(19, 36), env={**SPREAD, "QD_ECO_NS": "1", "QD_ECO_COHORT_K": "8", "QD_ECO_SPECIES_0_MODE": "diffusion"}),
    # one row crosses a 64- and a 128-lane boundary and ends in a tail
    "wide": dict(grid=(5, 130), env={**SPREAD, "QD_ECO_SPECIES_WEIGHTS": "0.2,0.2,0.6", "QD_ECO_COHORT_K": "2", "QD_ECO_SPREAD_NEIGHBORS": "moore",
                                     "QD_ECO_SPECIES_0_MODE": "diffusion", "QD_ECO_SPECIES_1_MODE": "seed", "QD_ECO_SPECIES_2_MODE": "diffusion"}),
    "noland": dict(grid=(19, 36), env={**SPREAD, "QD_ECO_SPECIES_WEIGHTS": "0.5,0.3,0.2", "QD_ECO_COHORT_K": "2", "QD_ECO_RAND_SEED": "3"},
                   ocean=True, kinds=("f32",)),
}


def set_env(env):
    for k in [k for k in os.environ if k.startswith("QD_ECO_")]:
        del os.environ[k]
    os.environ.update(env)


def land_mask(rng, shape, ocean=False):
    nlat, nlon = shape
    if ocean:
        return np.zeros(shape, dtype=np.uint8)
    m = (rng.uniform(size=shape) < 0.55).astype(np.uint8)
    m[:, (5 * nlon) // 6:] = 0
    m[0, 2:nlon // 2] = 1                            # land on both pole rows
    m[-1, 5:(2 * nlon) // 3] = 1
    return m


def lai_plane(rng, land, lai_max):
    """Every kind of value the restore has to carry, on land and on ocean cells alike."""
    nlat, nlon = land.shape
    L = rng.uniform(0.0, 3.0, land.shape)
    L[1, 3:6] = -rng.uniform(0.1, 2.0, 3)            # negatives -> 0
    L[2, 4:8] = lai_max + rng.uniform(0.1, 3.0, 4)  # above lai_max -> lai_max
    L[3, 2:7] = 0.0                                  # exact zeros
    L[0, 3] = 1e-42                                  # a float32 subnormal (a normal float64)
    L[nlat // 2, 5] = np.nan                         # np.clip passes NaN
    L[nlat // 2 + 1, 9] = np.inf                     # -> lai_max
    L[-1, nlon - 1] = 2.5                            # the last cell of the grid
    for (j, i) in ((nlat // 2, 5), (nlat // 2 + 1, 9), (1, 4), (2, 5), (3, 3), (0, 3)):
        if land.any():
            land[j, i] = 1                           # the special values sit on land
    return L


def after_load(pop):
    return {"load_LAI": np.array(pop.LAI), "load_LAI_layers_SK": pop.LAI_layers_SK.copy(), "load_species_weights": np.array(pop.species_weights),
            "load_total_LAI": pop.total_LAI().copy(), "load_R_leaf": np.array(pop._species_R_leaf)}


def run_case(name, spec, kind, mods, ref, dref):
    EcologyAdapter, SphericalGrid = mods
    set_env(spec["env"])
    rng = np.random.default_rng(sum(map(ord, name)))
    shape = spec["grid"]
    land = land_mask(rng, shape, spec.get("ocean", False))
    grid = SphericalGrid(*shape)
    lai_max = float(os.environ.get("QD_ECO_LAI_MAX", "5.0"))
    plane = lai_plane(rng, land, lai_max)
    eco = EcologyAdapter(grid, land.astype(int))
    pop = eco.pop
    S, K, NB = pop.Ns, pop.K, eco.bands.nbands
    w_file = rng.uniform(0.1, 1.0, S)
    if S >= 3:
        w_file[1] = -0.25                            # clipped to 0: a species whose planes are exactly zero
    R_file = np.clip(np.asarray(pop._species_R_leaf) * 0.9 + 0.05, 0.0, 1.0)
    tmp = tempfile.mkdtemp()
    path = os.path.join(tmp, "ecology.npz")
    if kind == "f32":
        arrays = dict(LAI=plane.astype(np.float32), species_weights=w_file.astype(np.float32),
                      bands_lambda_centers=np.asarray(eco.bands.lambda_centers, dtype=np.float32), R_species_nb=R_file.astype(np.float32))
        np.savez(path, **arrays)
    else:
        src = EcologyAdapter(grid, land.astype(int))                 # the reference's own NPZ save
        src.pop.LAI = plane.copy()
        src.pop.species_weights = w_file.copy()
        src.pop.set_species_reflectance_bands(R_file)
        assert src.save_autosave(path, day_value=1.25)
        with np.load(path) as z:
            arrays = {k: z[k] for k in z.files}
        assert arrays["LAI"].dtype == np.float64
    assert eco.load_autosave(path, on_mismatch="fallback") is True
    out = dict(land_mask=land, env_keys=np.array(sorted(spec["env"])), env_vals=np.array([spec["env"][k] for k in sorted(spec["env"])]),
               modes=np.array(pop.species_modes), lai_max=lai_max, K=K, **{"file_" + k: v for k, v in arrays.items()})
    out.update(after_load(pop))
    # the restatement reproduces the load bitwise, in both of its spellings
    L, sw, stack, tot = ref.load_rule(arrays["LAI"], arrays["species_weights"], K, lai_max)
    for a, b, what in ((L, pop.LAI, "LAI"), (sw, pop.species_weights, "weights"), (stack, pop.LAI_layers_SK, "stack"), (tot, pop.total_LAI(), "total")):
        assert a.dtype == np.asarray(b).dtype and np.array_equal(a, b, equal_nan=True), f"{name}/{kind}: restated {what} differs"
    if kind == "f32":
        for a, b in zip(ref.load_rule_f32(arrays["LAI"], arrays["species_weights"], K, lai_max), (L, sw, stack, tot)):
            assert np.array_equal(a, b, equal_nan=True), f"{name}: the float32 spelling differs"
        st64 = ref.load_rule(arrays["LAI"].astype(np.float64), arrays["species_weights"].astype(np.float64), K, lai_max)[2]
        assert not np.array_equal(st64, stack, equal_nan=True), f"{name}: float64 arithmetic would give the same stack"
    last_bit = np.nanmax(np.abs(np.asarray(pop.LAI, dtype=float) - pop.total_LAI()))
    # one sub-daily step, then one daily step
    isr = rng.uniform(0.0, 60.0, shape)
    isr[:, 0:3] = 0.0
    alpha = eco.step_subdaily(isr, 0.0, DT)
    A_b, w_b = eco.get_surface_albedo_bands()
    out.update(isr=isr, sub_alpha=alpha, sub_A_bands=A_b, sub_w_b=w_b, sub_E_day=pop.E_day.copy(), sub_f=np.array(pop._canopy_f_cached))
    soil = np.clip(rng.uniform(0.0, 0.9, shape), 0.0, 1.0)
    cfg = dref.Cfg.from_env(spec["env"], pop.species_modes, pop.species_weights)
    st = dref.State(land == 1, pop.LAI_layers_SK.copy(), pop.E_day.copy(), pop.age_days.copy(), pop.seed_bank.copy(), (land == 1).astype(float))
    pop.step_daily(soil)
    dref.step_daily(st, cfg, soil)
    # the branch probe runs on a copy without the subnormal cell: its 1e-42 is next to zero by construction, and it reaches the
    # device bit for bit (the restore is exact), so no device exp / pow can move it across
    probe = {}
    st_p = dref.State(land == 1, out["load_LAI_layers_SK"].copy(), out["sub_E_day"].copy(), np.zeros(shape), np.zeros(shape), (land == 1).astype(float))
    st_p.layers[:, :, 0, 3] = 0.0
    dref.step_daily(st_p, cfg, soil, probe)
    for a, b, what in ((st.layers, pop.LAI_layers_SK, "layers"), (st.age, pop.age_days, "age"), (st.bank, pop.seed_bank, "bank"),
                       (st.total(), pop.total_LAI(), "total")):
        assert np.array_equal(a, b, equal_nan=True), f"{name}/{kind}: the daily restatement's {what} differs from the reference"
    bad = {k: v for k, v in probe.items() if not v > 1e-9}
    assert not bad, f"{name}/{kind}: inputs on a branch {bad}"
    out.update(soil=soil, day_LAI_layers_SK=pop.LAI_layers_SK.copy(), day_age_days=pop.age_days.copy(), day_seed_bank=pop.seed_bank.copy(),
               day_LAI=np.array(pop.LAI), day_total_LAI=pop.total_LAI().copy(), day_spread_gate=np.array(pop._spread_gate))
    out["meta"] = json.dumps({"case": name, "kind": kind, "grid": list(shape), "S": S, "K": K, "NB": int(NB), "probe": probe,
                              "LAI_vs_total_LAI": float(last_bit), "ocean_cells_nonzero": int(np.sum((land == 0) & (out["load_total_LAI"] != 0)))})
    fn = f"eco_state_{name}_{kind}_{shape[0]}x{shape[1]}.npz"
    np.savez_compressed(os.path.join(OUT, fn), **out)
    print(f"{fn}: S={S} K={K} modes={pop.species_modes} |LAI - total_LAI| max {last_bit:.2e} NaN cells after the day "
          f"{int(np.isnan(out['day_total_LAI']).sum())} min probe {min(probe.values()) if probe else None}")
    return eco, arrays


def run_mismatch(mods, ref):
    """On the `mixed` run: a file with 4 species, one with NB + 1 bands, a malformed one."""
    EcologyAdapter, SphericalGrid = mods
    spec = CASES["mixed"]
    set_env({**spec["env"], "QD_ECO_DIAG": "1"})
    rng = np.random.default_rng(4242)
    shape = spec["grid"]
    land = land_mask(rng, shape)
    plane = lai_plane(rng, land, 5.0).astype(np.float32)
    grid = SphericalGrid(*shape)
    tmp = tempfile.mkdtemp()
    out = dict(land_mask=land, env_keys=np.array(sorted(spec["env"])), env_vals=np.array([spec["env"][k] for k in sorted(spec["env"])]))

    def load(tag, arrays, **kw):
        path = os.path.join(tmp, tag + ".npz")
        np.savez(path, **arrays)
        with contextlib.redirect_stdout(io.StringIO()):
            eco = EcologyAdapter(grid, land.astype(int))
        before = after_load(eco.pop)
        buf = io.StringIO()
        with contextlib.redirect_stdout(buf):
            ok = eco.load_autosave(path, **kw)
        out.update({f"{tag}_file_{k}": v for k, v in arrays.items()})
        out[f"{tag}_ok"] = bool(ok)
        out[f"{tag}_lines"] = np.array(buf.getvalue().splitlines())
        out.update({f"{tag}_{k}": v for k, v in after_load(eco.pop).items()})
        return eco, before

    nb = None
    eco0 = EcologyAdapter(grid, land.astype(int))
    nb = eco0.bands.nbands
    centers = np.asarray(eco0.bands.lambda_centers, dtype=np.float32)
    w4 = np.array([0.4, 0.1, 0.3, 0.2], dtype=np.float32)
    R4 = rng.uniform(0.1, 0.9, (4, nb)).astype(np.float32)
    eco, _ = load("species4", dict(LAI=plane, species_weights=w4, bands_lambda_centers=centers, R_species_nb=R4))
    assert eco.pop.Ns == 4 and eco.pop.LAI_layers_SK.shape[0] == 4 and out["species4_ok"]
    w3 = np.array([0.2, 0.5, 0.3], dtype=np.float32)
    centers_x = np.linspace(380, 780, nb + 1).astype(np.float32)
    eco, before = load("bands", dict(LAI=plane, species_weights=w3, bands_lambda_centers=centers_x,
                                     R_species_nb=rng.uniform(0.1, 0.9, (3, nb + 1)).astype(np.float32)))
    assert out["bands_ok"] and np.array_equal(out["bands_load_R_leaf"], before["load_R_leaf"]) and "advanced=NO" in out["bands_lines"][-1]
    eco, _ = load("bands_ignore", dict(LAI=plane, species_weights=w3, bands_lambda_centers=centers_x,
                                       R_species_nb=rng.uniform(0.1, 0.9, (3, nb + 1)).astype(np.float32)), on_mismatch="ignore")
    assert len(out["bands_ignore_lines"]) == 1
    eco, before = load("malformed", dict(LAI=np.stack([plane, plane]), species_weights=w3, bands_lambda_centers=centers, R_species_nb=R4[:3]))
    assert out["malformed_ok"] is False
    for k, v in before.items():
        assert np.array_equal(out["malformed_" + k], v, equal_nan=True)
    fn = f"eco_state_mismatch_f32_{shape[0]}x{shape[1]}.npz"
    np.savez_compressed(os.path.join(OUT, fn), **out)
    print(fn, {t: list(out[f"{t}_lines"]) for t in ("species4", "bands", "bands_ignore", "malformed")})


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reference", default=os.path.join(HERE, "..", "..", "reference"))
    ap.add_argument("cases", nargs="*", default=list(CASES))
    a = ap.parse_args()
    sys.path.insert(0, os.path.abspath(a.reference))
    sys.path.insert(0, os.path.join(HERE, "..", "tests"))
    assert int(np.__version__.split(".")[0]) >= 2, "the float32 case records NumPy >= 2 promotion"
    from pygcm.ecology.adapter import EcologyAdapter
    from pygcm.grid import SphericalGrid
    import eco_state_ref as ref
    import eco_daily_ref as dref
    mods = (EcologyAdapter, SphericalGrid)
    for name in a.cases:
        for kind in CASES[name].get("kinds", ("f32", "f64")):
            eco, _ = run_case(name, CASES[name], kind, mods, ref, dref)
            if name == "mixed" and kind == "f64":                    # the genes document of that run, by the reference's writer
                set_env(CASES[name]["env"])
                assert eco.save_genes_json(os.path.join(OUT, "genes_eco_state_mixed.json"), day_value=1.25)
    if "mixed" in a.cases:
        run_mismatch(mods, ref)


if __name__ == "__main__":
    main()
