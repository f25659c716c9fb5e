"""Regenerate tests/golden/eco_daily_<case>_19x36.npz from the reference's PopulationManager (pygcm/ecology/population.py).

Needs a checkout of the reference project (default ../reference next to this repository, or --reference DIR).  Each case sets
its QD_ECO_* environment, builds the reference's PopulationManager on a hand-made land mask, overwrites its state (LAI layers,
seed bank) with the case's inputs and runs step_daily three times, each time on that day's E_day and soil index (the driver's
clip(W_land / cap, 0, 1) * !glacier).  The golden holds the inputs, the environment as data, the species modes and weights, and
after the first and the third day LAI_layers_SK, LAI, total_LAI, age_days, seed_bank, _spread_gate, E_day and summary().

Device exp / pow differ from NumPy's in the last bits, so no input may sit on a branch: with tests/eco_daily_ref.py (which must
reproduce the reference bitwise) the script asserts that every compared quantity of every case -- cap_sum vs 0, LAI vs 0 and
lai_max, the increments vs their caps, the seed bank vs its cap, soil vs the stress threshold -- is farther than 1e-9 (relative)
from its threshold, unless it is exactly zero by construction.
"""
import argparse
import json
import os
import sys

import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))
OUT = os.path.join(HERE, "..", "tests", "golden")
NLAT, NLON, DAYS = 19, 36, 3


def land_mask(rng, poles):
    m = (rng.uniform(size=(NLAT, NLON)) < 0.55).astype(np.uint8)
    m[:, 30:] = 0                                   # an ocean basin, so coasts exist on both axes
    m[7:9, 3:9] = 0
    if poles:                                       # land on both pole rows: np.roll's axis-0 wrap carries LAI between them
        m[0, 2:20] = 1
        m[-1, 5:25] = 1
    return m


def seam_mask(rng):
    """Land on both sides of the east-west seam: columns 0 and NLON-1 on the same rows, among them both pole rows (so the four
    corners are land and each corner's Moore neighbourhood wraps both axes at once), with ocean columns next to them on some rows."""
    m = (rng.uniform(size=(NLAT, NLON)) < 0.45).astype(np.uint8)
    m[:, 12:20] = 0                                 # the ocean basin sits mid-grid: the seam itself is a continent
    rows = [0, 1, 4, 5, 9, 13, 14, NLAT - 2, NLAT - 1]
    m[rows, 0] = 1
    m[rows, -1] = 1
    m[[4, 13], 1] = 0                               # land on the seam whose only east-west land neighbour is across it
    m[[4, 13], -2] = 0
    m[[0, NLAT - 1], 1:4] = 1                       # pole rows: land runs up to the corners from both sides
    m[[0, NLAT - 1], -4:-1] = 1
    return m


def inputs(rng, S, K, land, e_scale, l_max=0.6):
    L0 = rng.uniform(0.0, l_max, (S, K, NLAT, NLON)) * (land == 1)
    L0[:, :, 4:6, 10:14] = 0.0                      # bare land: LAI exactly 0 (the equal splits)
    E = rng.uniform(0.2, 1.0, (DAYS, NLAT, NLON)) * e_scale
    E[:, 10:12, 0:8] = 0.0                          # no light: cap_sum exactly 0
    E[0, 2, 3], E[0, 3, 4], E[0, 12, 20] = np.nan, np.inf, -np.inf
    W = rng.uniform(0.0, 40.0, (DAYS, NLAT, NLON))  # soil index 0 .. 0.8 around the stress threshold 0.3
    glacier = np.zeros((NLAT, NLON), dtype=bool)
    glacier[0:2, :] = True
    glacier[15, 5:9] = True
    return L0, E, W, glacier


CASES = {
    "defaults": dict(env={"QD_ECO_RAND_SEED": "11"}, poles=False, e_scale=2.0e4),
    "layers": dict(env={"QD_ECO_NS": "4", "QD_ECO_COHORT_K": "3", "QD_ECO_RAND_SEED": "5"}, poles=False, e_scale=2.0e4),
    "spread_vn": dict(env={"QD_ECO_SPECIES_WEIGHTS": "0.4,0.3,0.2,0.1", "QD_ECO_COHORT_K": "2", "QD_ECO_SPREAD_ENABLE": "1",
                           "QD_ECO_SPREAD_RATE": "0.1", "QD_ECO_SPREAD_SOIL_EXP": "2", "QD_ECO_SEED_ENERGY": "200",
                           "QD_ECO_SPECIES_0_MODE": "seed", "QD_ECO_SPECIES_1_MODE": "diffusion",
                           "QD_ECO_SPECIES_2_MODE": "diffusion", "QD_ECO_SPECIES_3_MODE": "seed"}, poles=True, e_scale=2.0e4),
    "spread_moore": dict(env={"QD_ECO_NS": "3", "QD_ECO_COHORT_K": "2", "QD_ECO_SPREAD_ENABLE": "1", "QD_ECO_SPREAD_RATE": "0.2",
                              "QD_ECO_SPREAD_NEIGHBORS": "moore", "QD_ECO_SPREAD_GATE_SOIL": "0", "QD_ECO_SEED_ENERGY": "500",
                              "QD_ECO_SEED_BANK_RETAIN": "0.35", "QD_ECO_SEED_BANK_MAX": "2.0", "QD_ECO_SEED_GERMINATE_FRAC": "0.25",
                              "QD_ECO_SEED_BANK_DECAY": "0.1", "QD_ECO_SPECIES_0_MODE": "diffusion",
                              "QD_ECO_SPECIES_1_MODE": "seed", "QD_ECO_SPECIES_2_MODE": "seed"}, poles=True, e_scale=2.0e4, bank=1.5),
    "rate_clipped": dict(env={"QD_ECO_SPECIES_WEIGHTS": "0.1,0.6,0.3", "QD_ECO_COHORT_K": "1", "QD_ECO_SPREAD_ENABLE": "1",
                              "QD_ECO_SPREAD_RATE": "0.9", "QD_ECO_SEED_ENERGY": "1000", "QD_ECO_RAND_SEED": "4",
                              "QD_ECO_SPECIES_0_MODE": "diffusion"}, poles=True, e_scale=2.0e4),
    # land on both sides of the longitude seam, at both pole rows and the four corners; Moore, the deepest stack (K = 8)
    "seam": dict(env={"QD_ECO_NS": "2", "QD_ECO_COHORT_K": "8", "QD_ECO_SPREAD_ENABLE": "1", "QD_ECO_SPREAD_RATE": "0.15",
                      "QD_ECO_SPREAD_NEIGHBORS": "moore", "QD_ECO_SPREAD_GATE_SOIL": "0", "QD_ECO_SEED_ENERGY": "400",
                      "QD_ECO_SPECIES_0_MODE": "diffusion", "QD_ECO_SPECIES_1_MODE": "seed"}, mask="seam", e_scale=2.0e4, bank=1.0,
                 l_max=0.15),
}


def snapshot(pop, tag):
    s = pop.summary()
    return {f"{tag}_LAI_layers_SK": pop.LAI_layers_SK.copy(), f"{tag}_LAI": pop.LAI.copy(), f"{tag}_total_LAI": pop.total_LAI().copy(),
            f"{tag}_age_days": pop.age_days.copy(), f"{tag}_seed_bank": pop.seed_bank.copy(), f"{tag}_spread_gate": pop._spread_gate.copy(),
            f"{tag}_E_day": pop.E_day.copy(), f"{tag}_summary": np.array([s["LAI_min"], s["LAI_mean"], s["LAI_max"]])}


def run_case(name, spec, PopulationManager, ref):
    for k in [k for k in os.environ if k.startswith("QD_ECO_")]:
        del os.environ[k]
    os.environ.update(spec["env"])
    rng = np.random.default_rng(sum(map(ord, name)))
    land = seam_mask(rng) if spec.get("mask") == "seam" else land_mask(rng, spec["poles"])
    pop = PopulationManager(land.astype(int), diag=False)
    S, K = pop.LAI_layers_SK.shape[:2]
    L0, E, W, glacier = inputs(rng, S, K, land, spec["e_scale"], spec.get("l_max", 0.6))
    bank0 = rng.uniform(0.0, spec.get("bank", 0.0), (NLAT, NLON)) * (land == 1) if spec.get("bank") else np.zeros((NLAT, NLON))
    cap = float(os.environ.get("QD_ECO_SOIL_WATER_CAP", "50.0"))
    soil = np.stack([ref.soil_index(W[d], glacier, cap) for d in range(DAYS)])
    pop.LAI_layers_SK[...] = L0
    pop.seed_bank[...] = bank0
    out = dict(land_mask=land, L0=L0, E_days=E, W_land=W, glacier=glacier.astype(np.float64), soil=soil, bank0=bank0,
               env_keys=np.array(sorted(spec["env"])), env_vals=np.array([spec["env"][k] for k in sorted(spec["env"])]),
               modes=np.array(pop.species_modes), species_weights=pop.species_weights.copy(), n_days=DAYS)
    cfg = ref.Cfg.from_env(spec["env"], pop.species_modes, pop.species_weights)
    st = ref.State(land == 1, L0.copy(), np.zeros((NLAT, NLON)), np.zeros((NLAT, NLON)), bank0.copy(), (land == 1).astype(float))
    probe = {}
    for d in range(DAYS):
        pop.E_day[...] = E[d]
        pop.step_daily(soil[d])
        st.E_day = E[d].copy()
        ref.step_daily(st, cfg, soil[d], probe)
        if d in (0, DAYS - 1):
            out.update(snapshot(pop, "first" if d == 0 else "last"))
        for a, b, what in ((st.layers, pop.LAI_layers_SK, "layers"), (st.age, pop.age_days, "age"), (st.bank, pop.seed_bank, "bank"),
                           (st.gate, pop._spread_gate, "gate"), (st.total(), pop.total_LAI(), "total")):
            assert np.array_equal(a, b), f"{name} day {d}: the restatement's {what} differs from the reference"
    bad = {k: v for k, v in probe.items() if not v > 1e-9}
    assert not bad, f"{name}: inputs on a branch {bad}"
    out["meta"] = json.dumps({"case": name, "nlat": NLAT, "nlon": NLON, "probe": probe})
    np.savez_compressed(os.path.join(OUT, f"eco_daily_{name}_{NLAT}x{NLON}.npz"), **out)
    first, last = out["first_total_LAI"], out["last_total_LAI"]
    print(f"{name}: S={S} K={K} modes={pop.species_modes} summary {out['last_summary']} seeded age zeros "
          f"{int(np.sum((out['last_age_days'] == 0) & (land == 1)))} bank max {out['last_seed_bank'].max():.3g} "
          f"LAI moved {float(np.abs(last - np.sum(L0, axis=(0, 1))).max()):.3g} min probe {min(probe.values()):.2e}")


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reference", default=os.path.join(HERE, "..", "..", "reference"))
    ap.add_argument("cases", nargs="*", default=list(CASES))
    a = ap.parse_args()
    sys.path.insert(0, os.path.abspath(a.reference))
    sys.path.insert(0, os.path.join(HERE, "..", "tests"))
    from pygcm.ecology.population import PopulationManager
    import eco_daily_ref as ref
    for name in a.cases:
        run_case(name, CASES[name], PopulationManager, ref)


if __name__ == "__main__":
    main()
