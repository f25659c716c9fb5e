"""Regenerate tests/golden/speciation_<case>_<nlat>x<nlon>.npz and tests/golden/genes_export_speciation.json from the reference's
EcologyAdapter (pygcm/ecology/adapter.py) and PopulationManager (pygcm/ecology/population.py).

Needs a checkout of the reference project (default ../reference next to this repository, or --reference DIR); it is imported at
run time and none of its text is held here.  Each case sets its QD_ECO_* environment, builds the reference's adapter on a hand-made
land mask, overwrites the state (LAI layers, seed bank) with the case's inputs and, under np.random.seed(s), runs seven daily
steps through EcologyAdapter.step_daily: two plain firings, a firing with a forced hit (mut_rate = 1 for that day, 0 otherwise, so
the global generator is drawn from only where the reference draws for a mutation), two plain firings, a second forced hit, one
plain firing.  The golden holds the inputs, the environment as data, the seed, and after every firing LAI_layers_SK, pop.LAI,
total_LAI(), species_weights, age_days and seed_bank; for every hit the stack as add_species_from_parent found it, the parent it
was given, the rand() and the choice's uniform draw, the mutated gene, the reflectance table, and the printed line.

With tests/speciation_ref.py (which must reproduce every stage bitwise) the script ASSERTS that the uniform draw behind every
np.random.choice lies more than 1e-9 from each edge of the cumulative weights -- so the blocked land sums of the device cannot
change the parent -- and takes the first seed for which that and the case's own demand (a given parent) hold.
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
N_FIRINGS, HITS = 7, (2, 5)

SPREAD = {"QD_ECO_SPREAD_ENABLE": "1", "QD_ECO_SPREAD_RATE": "0.1", "QD_ECO_SEED_ENERGY": "200", "QD_ECO_RAND_SEED": "3"}
BASE = {"QD_ECO_DIAG": "0", "QD_ECO_SPECIES_MAX": "64"}
CASES = {
    # n_species * n_layers 8, 9, 24, 25 before the first split, on one layer
    "p8": dict(env={**BASE, **SPREAD, "QD_ECO_NS": "8"}, land=0.2),
    "p9": dict(env={**BASE, **SPREAD, "QD_ECO_NS": "9"}, land=0.2),
    "p24": dict(env={**BASE, **SPREAD, "QD_ECO_NS": "24"}, land=0.12),
    "p25": dict(env={**BASE, **SPREAD, "QD_ECO_NS": "25"}, land=0.12),
    # the species counts at which the kernel's register table changes size: 7 -> 8 -> 9 and 23 -> 24 -> 25
    "e8": dict(env={**BASE, **SPREAD, "QD_ECO_NS": "7", "QD_ECO_COHORT_K": "2"}, land=0.2),
    "e24": dict(env={**BASE, **SPREAD, "QD_ECO_NS": "23"}, land=0.12),
    # the default species count on one layer
    "ns20": dict(env={**BASE, "QD_ECO_RAND_SEED": "3"}, land=0.12),
    # the first hit's parent is species 0 / the last species
    "parent0": dict(env={**BASE, **SPREAD, "QD_ECO_NS": "3", "QD_ECO_COHORT_K": "3"}, land=0.45, parent=0),
    "parentlast": dict(env={**BASE, **SPREAD, "QD_ECO_NS": "3", "QD_ECO_COHORT_K": "3"}, land=0.45, parent=2),
    # QD_ECO_MUT_EPS above the clip at 0.5
    "eps07": dict(env={**BASE, **SPREAD, "QD_ECO_NS": "3", "QD_ECO_COHORT_K": "2", "QD_ECO_MUT_EPS": "0.7"}, land=0.45),
    # a NaN and a value above lai_max in the stack (no spread, one layer: a firing only germinates on land and keeps them)
    "nonfinite": dict(env={**BASE, "QD_ECO_NS": "4", "QD_ECO_RAND_SEED": "3"}, land=0.45, nonfinite=True),
    # a mask without land: uniform weights
    "noland": dict(env={**BASE, **SPREAD, "QD_ECO_NS": "3", "QD_ECO_COHORT_K": "2"}, land=0.0),
    # species_max reached by the first hit: the second prints the skip
    "smax": dict(env={**BASE, **SPREAD, "QD_ECO_NS": "3", "QD_ECO_COHORT_K": "2", "QD_ECO_SPECIES_MAX": "4", "QD_ECO_DIAG": "1",
                      "QD_ECO_SPREAD_ENABLE": "0"}, land=0.45),
    # one species: the new index 1 spreads by seed, the next new index 2 by diffusion
    "modes": dict(env={**BASE, **SPREAD, "QD_ECO_NS": "1", "QD_ECO_COHORT_K": "2", "QD_ECO_SPECIES_0_MODE": "diffusion",
                       "QD_ECO_MUT_EPS": "0.3"}, land=0.45),
    # ragged rows
    "wide": dict(env={**BASE, **SPREAD, "QD_ECO_NS": "3", "QD_ECO_COHORT_K": "2", "QD_ECO_SPREAD_NEIGHBORS": "moore"}, land=0.45,
                 grid=(5, 130)),
}


class RandomTap:
    """Stands in for the adapter module's `np.random`: the global generator's own functions, with what rand() and choice()
    returned kept; choice() is preceded by a copy of the generator's state, from which the uniform draw it uses is read."""

    def __init__(self):
        self.rand_values, self.choice_u, self.choice_p = [], [], []

    def __getattr__(self, name):
        return getattr(np.random, name)

    def rand(self, *a):
        v = np.random.rand(*a)
        self.rand_values.append(float(v))
        return v

    def choice(self, a, p=None):
        probe = np.random.RandomState()
        probe.set_state(np.random.get_state())
        u = float(probe.random_sample())
        out = np.random.choice(a, p=p)
        cdf = np.cumsum(p)
        cdf /= cdf[-1]
        assert int(cdf.searchsorted(u, side="right")) == int(out), "the uniform draw read ahead is not the one choice() used"
        self.choice_u.append(u)
        self.choice_p.append(np.array(p, dtype=float))
        return out


class NumpyTap:
    def __init__(self, random):
        self.random = random

    def __getattr__(self, name):
        return getattr(np, name)


def gene_record(g):
    return {"identity": g.identity, "alloc": [g.alloc_root, g.alloc_stem, g.alloc_leaf], "leaf_area_per_energy": g.leaf_area_per_energy,
            "peaks": [[p.center_nm, p.width_nm, p.height] for p in g.absorption_peaks], "drought_tolerance": g.drought_tolerance,
            "gdd_germinate": g.gdd_germinate, "lifespan_days": int(g.lifespan_days), "provenance": g.provenance}


def run_case(name, spec, adapter_mod, sref, pref, seed, export_to=None):
    for k in [k for k in os.environ if k.startswith("QD_ECO_")]:
        del os.environ[k]
    os.environ.update(spec["env"])
    env = spec["env"]
    nlat, nlon = spec.get("grid", (19, 36))
    rng = np.random.default_rng(sum(map(ord, name)) + 77)
    land = (rng.uniform(size=(nlat, nlon)) < spec["land"]).astype(np.uint8)
    grid = types.SimpleNamespace(lat_mesh=np.zeros((nlat, nlon)))
    tap = RandomTap()
    adapter_mod.np = NumpyTap(tap)
    buf = io.StringIO()
    with contextlib.redirect_stdout(buf):
        eco = adapter_mod.EcologyAdapter(grid, land.astype(int))
    pop = eco.pop
    S, K = pop.LAI_layers_SK.shape[:2]
    L0 = rng.uniform(0.0, 0.3, (S, K, nlat, nlon)) * (land == 1)
    L0[:, :, 2:4, 5:9] = 0.0                        # bare land
    if spec.get("nonfinite"):
        (lj, li), (mj, mi) = np.argwhere(land == 1)[[3, 7]]
        (oj, oi), (pj, pi) = np.argwhere(land == 0)[[5, 9]]
        L0[1, 0, lj, li] = np.nan                   # on land: the species' land sum skips it
        L0[2, 0, oj, oi] = np.nan
        L0[0, 0, mj, mi] = 7.5                      # above lai_max on land: the first firing's germination clips it
        L0[3, 0, pj, pi] = 7.5                      # ... on the ocean: only the event's clip touches it
    E_days = rng.uniform(0.2, 1.0, (N_FIRINGS, nlat, nlon)) * 2.0e4
    soil = rng.uniform(0.0, 0.9, (N_FIRINGS, nlat, nlon))
    bank0 = rng.uniform(0.0, 2.0, (nlat, nlon)) * (land == 1)
    pop.LAI_layers_SK[...] = L0
    pop.seed_bank[...] = bank0
    out = dict(land_mask=land, L0=L0, E_days=E_days, soil=soil, bank0=bank0, modes=np.array(pop.species_modes),
               species_weights0=pop.species_weights.copy(), env_keys=np.array(sorted(env)), env_vals=np.array([env[k] for k in sorted(env)]),
               n_firings=N_FIRINGS, hit_firings=np.array(HITS), seed=seed, w_b=np.asarray(eco.w_b, dtype=float),
               genes0=json.dumps([gene_record(g) for g in eco.genes_list]))
    pre = {}
    inner = pop.add_species_from_parent

    def add_species(parent_idx, frac=0.02):
        pre["stack"], pre["parent"], pre["frac"] = pop.LAI_layers_SK.copy(), int(parent_idx), float(frac)
        return inner(parent_idx, frac=frac)
    pop.add_species_from_parent = add_species
    np.random.seed(seed)
    hit, lines = 0, []
    for d in range(N_FIRINGS):
        pop.E_day[...] = E_days[d]
        eco.mut_rate = 1.0 if d in HITS else 0.0
        pre.clear()
        n_genes = len(eco.genes_list)
        with contextlib.redirect_stdout(buf):
            buf.seek(0); buf.truncate()
            eco.step_daily(soil[d])
            text = buf.getvalue()
        assert "failed" not in text, text
        tag = f"s{d + 1}"
        out.update({f"{tag}_stack": pop.LAI_layers_SK.copy(), f"{tag}_LAI": pop.LAI.copy(), f"{tag}_total_LAI": pop.total_LAI().copy(),
                    f"{tag}_weights": pop.species_weights.copy(), f"{tag}_age": pop.age_days.copy(), f"{tag}_bank": pop.seed_bank.copy()})
        if d in HITS:
            hit += 1
            lines.append([l for l in text.splitlines() if "mutation" in l])
            out[f"hit{hit}_rand"] = tap.rand_values[hit - 1]
            out[f"hit{hit}_split"] = bool(pre)
            if pre:
                assert len(eco.genes_list) == n_genes + 1 == pop.Ns
                u, p = tap.choice_u[-1], tap.choice_p[-1]
                edges = np.concatenate([[0.0], np.cumsum(p) / np.cumsum(p)[-1]])
                gap = float(np.min(np.abs(edges - u)))
                if not gap > 1e-9:
                    return f"choice draw {u} within {gap:.1e} of a cumulative-weight edge"
                if hit == 1 and spec.get("parent") is not None and pre["parent"] != spec["parent"]:
                    return f"first parent {pre['parent']}"
                out.update({f"hit{hit}_pre_stack": pre["stack"], f"hit{hit}_parent": pre["parent"], f"hit{hit}_frac": pre["frac"],
                            f"hit{hit}_choice_u": u, f"hit{hit}_choice_gap": gap, f"hit{hit}_gene": json.dumps(gene_record(eco.genes_list[-1])),
                            f"hit{hit}_R": np.asarray(pop._species_R_leaf, dtype=float).copy()})
    out["lines"] = json.dumps(lines)
    out["n_rand"] = len(tap.rand_values)
    # the restatement, stage by stage
    z = {k: (np.asarray(v) if not isinstance(v, (str, bool, int, float)) else v) for k, v in out.items()}
    for tag, got in sref.replay(z):
        for k, v in got.items():
            assert np.array_equal(v, out[f"{tag}_{k}"], equal_nan=True), f"{name} {tag}: the restatement's {k} differs from the reference"
    out["meta"] = json.dumps({"case": name, "nlat": nlat, "nlon": nlon, "seed": seed, "final_species": int(pop.Ns)})
    np.savez_compressed(os.path.join(OUT, f"speciation_{name}_{nlat}x{nlon}.npz"), **out)
    if export_to is not None:
        with contextlib.redirect_stdout(buf):
            eco.export_genes(export_to, 12.34)
        os.replace(os.path.join(export_to, "genes_day_012.3.json"), os.path.join(OUT, "genes_export_speciation.json"))
    print(f"{name}: {nlat}x{nlon} S={S}->{pop.Ns} K={K} seed={seed} parents "
          f"{[out.get(f'hit{h}_parent') for h in (1, 2)]} gaps {[out.get(f'hit{h}_choice_gap') for h in (1, 2)]} lines {lines}")
    return None


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reference", default=os.path.join(HERE, "..", "..", "reference"))
    ap.add_argument("cases", nargs="*", default=list(CASES))
    a = ap.parse_args()
    sys.path.insert(0, os.path.abspath(a.reference))
    sys.path.insert(0, os.path.join(HERE, "..", "tests"))
    sys.path.insert(0, os.path.join(HERE, ".."))
    import pygcm.ecology.adapter as adapter_mod
    import eco_daily_ref as pref
    import speciation_ref as sref
    import tempfile
    for name in a.cases:
        for seed in range(100, 160):
            with tempfile.TemporaryDirectory() as tmp:
                bad = run_case(name, CASES[name], adapter_mod, sref, pref, seed, export_to=tmp if name == "modes" else None)
            if not bad:
                break
            print(f"{name}: seed {seed} refused: {bad}")
        assert not bad, f"{name}: no seed found"


if __name__ == "__main__":
    main()
