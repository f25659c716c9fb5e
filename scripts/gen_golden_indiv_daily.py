"""Regenerate tests/golden/indiv_daily_<case>_19x36.npz from the reference's PopulationManager and IndividualPool
(pygcm/ecology/population.py, pygcm/ecology/individuals.py).

Needs a checkout of the reference project (default ../reference next to this repository, or --reference DIR); it is imported at
run time and none of its text is held here.  Each case sets its QD_ECO_* environment, builds the reference's PopulationManager
and, on a stand-in adapter that carries it, the reference's IndividualPool on a hand-made 19 x 36 land mask, overwrites the state
(LAI layers, seed bank, stress days) with the case's inputs and runs two days: pop.step_daily(soil), then
indiv.step_daily(adapter, soil) on that day's synthetic E_day of the individuals.  The golden holds the inputs, the environment
as data, the pool (sampled cells, species ids, tolerances) and after each day LAI_layers_SK, LAI, seed_bank, species_weights,
the stress days, the individuals' E_day, beta_hint (tapped from the module's np.mean call) and the printed line.

With tests/eco_daily_ref.py and tests/indiv_daily_ref.py (which must reproduce both days bitwise, the cell loop run level by
level) the script asserts that no compared quantity of any case is within 1e-9 (relative) of a branch it does not sit on exactly.
"""
import argparse
import contextlib
import io
import json
import os
import sys
import types

import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))
OUT = os.path.join(HERE, "..", "tests", "golden")
NLAT, NLON, DAYS = 19, 36, 2


def coast_mask(rng):
    m = (rng.uniform(size=(NLAT, NLON)) < 0.5).astype(np.uint8)
    m[:, 28:] = 0                                   # an ocean basin: sampled cells with ocean neighbours
    m[7:9, 3:9] = 0
    return m


def seam_mask(rng):
    """Land on both pole rows, in columns 0 and NLON-1 of the same rows, and at the four corners."""
    m = (rng.uniform(size=(NLAT, NLON)) < 0.45).astype(np.uint8)
    m[:, 12:20] = 0
    rows = [0, 1, 4, 5, 9, 13, 14, NLAT - 2, NLAT - 1]
    m[rows, 0] = 1
    m[rows, -1] = 1
    m[[0, NLAT - 1], 1:4] = 1
    m[[0, NLAT - 1], -4:-1] = 1
    return m


POP = {"QD_ECO_SPREAD_ENABLE": "1", "QD_ECO_SPREAD_RATE": "0.1", "QD_ECO_SEED_ENERGY": "200", "QD_ECO_RAND_SEED": "3"}
CASES = {
    # every land cell in row-major order: every cell conflicts with its neighbours; the seam mask; bare land; lai_max reached
    "full": dict(env={**POP, "QD_ECO_NS": "4", "QD_ECO_COHORT_K": "3", "QD_ECO_INDIV_SAMPLE_FRAC": "1.0", "QD_ECO_INDIV_PER_CELL": "5",
                      "QD_ECO_LAI_MAX": "1.2", "QD_ECO_LAI_GROWTH_RATE": "0.05", "QD_ECO_SPECIES_1_DROUGHT_TOL": "0.55"}, mask="seam", l_max=0.19),
    # seed-42 order: a later cell lies north or west of an earlier one; K = 1
    "sparse": dict(env={**POP, "QD_ECO_NS": "3", "QD_ECO_COHORT_K": "1", "QD_ECO_INDIV_SAMPLE_FRAC": "0.3", "QD_ECO_INDIV_PER_CELL": "7",
                        "QD_ECO_SPECIES_0_DROUGHT_TOL": "0.6", "QD_ECO_LAI_GROWTH_RATE": "0.02"}, mask="seam", l_max=0.3),
    # the eight-accumulator sums: K = 8 and S = 9
    "wide": dict(env={**POP, "QD_ECO_NS": "9", "QD_ECO_COHORT_K": "8", "QD_ECO_INDIV_SAMPLE_FRAC": "0.3", "QD_ECO_INDIV_PER_CELL": "5",
                      "QD_ECO_LAI_DECAY_RATE": "0.004", "QD_ECO_SPECIES_4_DROUGHT_TOL": "0.7"}, mask="coast", l_max=0.05),
    # the default species count on one layer: the strided column sum over 20 species
    "ns20": dict(env={**POP, "QD_ECO_INDIV_SAMPLE_FRAC": "0.5", "QD_ECO_INDIV_PER_CELL": "30", "QD_ECO_LAI_RECRUIT_FRAC": "0.5",
                      "QD_ECO_LAI_GROWTH_RATE": "0.03"}, mask="coast", l_max=0.1),
    # no stress penalty (the cell's mean stress drops out), no seed coupling
    "plain": dict(env={**POP, "QD_ECO_NS": "3", "QD_ECO_COHORT_K": "2", "QD_ECO_INDIV_SAMPLE_FRAC": "0.4", "QD_ECO_INDIV_PER_CELL": "6",
                       "QD_ECO_INDIV_STRESS_PENALTY": "0", "QD_ECO_INDIV_SEED_COUPLE": "0", "QD_ECO_INDIV_STRESS_DECAY": "0.25"},
                  mask="coast", l_max=0.3),
    # NaN and inf in the individuals' E_day
    "nonfinite": dict(env={**POP, "QD_ECO_NS": "4", "QD_ECO_COHORT_K": "2", "QD_ECO_INDIV_SAMPLE_FRAC": "0.3", "QD_ECO_INDIV_PER_CELL": "5"},
                      mask="coast", l_max=0.3, nonfinite=True),
}


class NumpyTap:
    """Stands in for the module's `np`: everything is NumPy's, and the result of its one np.mean call (beta_hint) is kept."""
    last_mean = None

    def __getattr__(self, name):
        return getattr(np, name)

    def mean(self, *a, **k):
        self.last_mean = np.mean(*a, **k)
        return self.last_mean


def run_case(name, spec, PopulationManager, ind_mod, pref, iref, plan_levels, seed):
    for k in [k for k in os.environ if k.startswith("QD_ECO_")]:
        del os.environ[k]
    os.environ.update(spec["env"])
    env = spec["env"]
    rng = np.random.default_rng(sum(map(ord, name)) + seed)
    land = seam_mask(rng) if spec["mask"] == "seam" else coast_mask(rng)
    pop = PopulationManager(land.astype(int), diag=False)
    S, K = pop.LAI_layers_SK.shape[:2]
    tol_s = np.array([float(env.get(f"QD_ECO_SPECIES_{s}_DROUGHT_TOL", "0.3")) for s in range(S)])
    adapter = types.SimpleNamespace(bands=types.SimpleNamespace(nbands=8), pop=pop,
                                    genes_list=[types.SimpleNamespace(drought_tolerance=float(t)) for t in tol_s])
    grid = types.SimpleNamespace(lat_mesh=np.zeros((NLAT, NLON)))
    tap = NumpyTap()
    ind_mod.np = tap
    buf = io.StringIO()
    with contextlib.redirect_stdout(buf):
        indiv = ind_mod.IndividualPool(grid, land.astype(int), adapter, sample_frac=0.02, per_cell=150, diag=True)
    C, N, pc = indiv.n_cells, indiv.n_indiv, indiv.per_cell
    lai_max = float(env.get("QD_ECO_LAI_MAX", "5.0"))
    L0 = rng.uniform(0.0, spec["l_max"], (S, K, NLAT, NLON)) * (land == 1)
    L0[:, :, 4:6, 20:26] = 0.0                      # bare land: total_old exactly 0
    E_grid = rng.uniform(0.2, 1.0, (DAYS, NLAT, NLON)) * 2.0e4
    W = rng.uniform(0.0, 40.0, (DAYS, NLAT, NLON))  # soil index 0 .. 0.8 around the tolerances
    glacier = np.zeros((NLAT, NLON), dtype=bool)
    glacier[0, :] = True
    cap = 50.0
    soil = np.stack([pref.soil_index(W[d], glacier, cap) for d in range(DAYS)])
    bank0 = rng.uniform(0.0, 1.0, (NLAT, NLON)) * (land == 1)
    E_ind = rng.uniform(0.0, 1.0, (DAYS, N)) * np.repeat(rng.uniform(0.2, 2.0, (DAYS, C)), pc, axis=1) * 2.0e3
    E_ind[:, rng.uniform(size=N) < 0.1] = 0.0
    if C > 3:
        E_ind[0, 2 * pc:3 * pc] = 0.0               # a cell without energy: denom is the bare 1e-12
    stress0 = rng.uniform(0.0, 3.0, N)
    stress0[rng.uniform(size=N) < 0.15] = 363.7     # reaches the cap of 365 on the second dry day
    if spec.get("nonfinite"):
        E_ind[0, 1], E_ind[0, pc + 2], E_ind[1, 3 * pc] = np.nan, np.inf, np.inf
    pop.LAI_layers_SK[...] = L0
    pop.seed_bank[...] = bank0
    indiv.indiv_water_stress_days[...] = stress0
    levels = plan_levels(indiv.sample_j, indiv.sample_i, NLAT, NLON)
    out = dict(land_mask=land, L0=L0, E_days=E_grid, W_land=W, glacier=glacier.astype(np.float64), soil=soil, bank0=bank0,
               E_indiv=E_ind, stress0=stress0, sample_j=indiv.sample_j, sample_i=indiv.sample_i, per_cell=pc,
               species_id=indiv.indiv_species_id.astype(np.int32), tol_species=tol_s, indiv_tol=indiv.indiv_tol, levels=levels,
               env_keys=np.array(sorted(env)), env_vals=np.array([env[k] for k in sorted(env)]),
               modes=np.array(pop.species_modes), species_weights0=pop.species_weights.copy(), n_days=DAYS)
    pcfg = pref.Cfg.from_env(env, pop.species_modes, pop.species_weights)
    pst = pref.State(land == 1, L0.copy(), None, np.zeros((NLAT, NLON)), bank0.copy(), (land == 1).astype(float))
    icfg = iref.Cfg.from_env(env)
    ist = iref.State(land == 1, None, None, indiv.sample_j.copy(), indiv.sample_i.copy(), pc, indiv.indiv_species_id.copy(),
                     indiv.indiv_tol.copy(), None, stress0.copy())
    probe, lines, parity = {}, [], []
    for d in range(DAYS):
        pop.E_day[...] = E_grid[d]
        pop.step_daily(soil[d])
        indiv.indiv_E_day[...] = E_ind[d]
        with contextlib.redirect_stdout(buf):
            buf.seek(0); buf.truncate()
            indiv.step_daily(adapter, soil[d], Ts_map=None, day_length_hours=24.0)
            lines.append(buf.getvalue().strip())
        beta = float(tap.last_mean)
        # the restatements, day by day
        pst.E_day = E_grid[d].copy()
        pref.step_daily(pst, pcfg, soil[d], probe)
        ist.layers, ist.bank, ist.E = pst.layers, pst.bank, E_ind[d].copy()
        info = iref.step_daily(ist, icfg, soil[d], levels, probe)
        pst.layers, pst.bank = ist.layers, ist.bank
        pcfg.weights = ist.weights
        parity.append(int(np.sum(info["denom"] > 0)) % 2)
        for a, b, what in ((ist.layers, pop.LAI_layers_SK, "layers"), (ist.LAI, pop.LAI, "LAI"), (ist.bank, pop.seed_bank, "bank"),
                           (ist.weights, pop.species_weights, "weights"), (ist.stress, indiv.indiv_water_stress_days, "stress"),
                           (ist.E, indiv.indiv_E_day, "E"), (np.float64(info["beta_hint"]), np.float64(beta), "beta_hint")):
            assert np.array_equal(a, b, equal_nan=True), f"{name} day {d}: the restatement's {what} differs from the reference"
        tag = f"day{d + 1}"
        out.update({f"{tag}_LAI_layers_SK": pop.LAI_layers_SK.copy(), f"{tag}_LAI": pop.LAI.copy(), f"{tag}_seed_bank": pop.seed_bank.copy(),
                    f"{tag}_species_weights": pop.species_weights.copy(), f"{tag}_stress_days": indiv.indiv_water_stress_days.copy(),
                    f"{tag}_E_indiv": indiv.indiv_E_day.copy(), f"{tag}_beta_hint": beta, f"{tag}_medE": info["medE"],
                    f"{tag}_n_positive": int(np.sum(info["denom"] > 0))})
    bad = {k: v for k, v in probe.items() if not (v > 1e-9 or v == 0.0)}      # 0.0: exactly on it (a bank clipped to its cap)
    if bad:
        return bad
    out["lines"] = np.array(lines)
    out["meta"] = json.dumps({"case": name, "nlat": NLAT, "nlon": NLON, "probe": probe, "input_seed": seed, "n_levels": int(levels.max())})
    np.savez_compressed(os.path.join(OUT, f"indiv_daily_{name}_{NLAT}x{NLON}.npz"), **out)
    tot = np.sum(out["day2_LAI_layers_SK"], axis=(0, 1))
    print(f"{name}: S={S} K={K} C={C} per_cell={pc} levels={int(levels.max())} positive denominators {out['day1_n_positive']}/"
          f"{out['day2_n_positive']} at lai_max {int(np.sum(tot == lai_max))} stress at 365 "
          f"{int(np.sum(out['day2_stress_days'] == 365.0))} LAI moved {float(np.abs(tot - np.sum(L0, axis=(0, 1))).max()):.3g} "
          f"weights {np.round(out['day2_species_weights'], 3)[:4]} min probe {min(probe.values()):.2e}\n   {lines[-1]}")


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reference", default=os.path.join(HERE, "..", "..", "reference"))
    ap.add_argument("cases", nargs="*", default=list(CASES))
    a = ap.parse_args()
    sys.path.insert(0, os.path.abspath(a.reference))
    sys.path.insert(0, os.path.join(HERE, "..", "tests"))
    sys.path.insert(0, os.path.join(HERE, ".."))
    from pygcm.ecology.population import PopulationManager
    import pygcm.ecology.individuals as ind_mod
    import eco_daily_ref as pref
    import indiv_daily_ref as iref
    from qingdai_amd.ecology import plan_levels
    for name in a.cases:
        for seed in range(1000, 1040):               # the first input seed that leaves no compared quantity within 1e-9 of a branch
            bad = run_case(name, CASES[name], PopulationManager, ind_mod, pref, iref, plan_levels, seed)
            if not bad:
                break
            print(f"{name}: input seed {seed} sits on a branch {bad}")
        assert not bad, f"{name}: no input seed without a branch hit"


if __name__ == "__main__":
    main()
