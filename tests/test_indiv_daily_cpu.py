"""CPU: the individuals' daily step off the device -- the staged NumPy restatement (tests/indiv_daily_ref.py) against the
reference's goldens bitwise over both days with the cell loop run level by level, the properties of `plan_levels`, a wrong plan
that misses the golden, np.sum's order spelled out, the parsing and defaults of every variable, the start-up refusals, the
diagnostic line and the ABI surface."""
import ctypes
import glob
import os
import re

import numpy as np
import pytest

import eco_daily_ref as pref
import indiv_daily_ref as iref
from qingdai_amd import _lib
from qingdai_amd.ecology import footprint, indiv_daily_line, plan_levels, spill_targets

HERE = os.path.dirname(os.path.abspath(__file__))
GOLDENS = sorted(glob.glob(os.path.join(HERE, "golden", "indiv_daily_*_19x36.npz")))
CASES = ("full", "nonfinite", "ns20", "plain", "sparse", "wide")


def _case(path):
    return os.path.basename(path)[12:-10]


def replay(z, levels="plan", days=None):
    """Both days of a golden through the two restatements -> per day the state the golden records."""
    env = dict(zip(z["env_keys"], z["env_vals"]))
    land = z["land_mask"] == 1
    pcfg = pref.Cfg.from_env(env, [str(m) for m in z["modes"]], z["species_weights0"])
    pst = pref.State(land, z["L0"].copy(), None, np.zeros(land.shape), z["bank0"].copy(), land.astype(float))
    ist = iref.State(land, None, None, z["sample_j"], z["sample_i"], int(z["per_cell"]), z["species_id"], z["indiv_tol"], None,
                     z["stress0"].copy())
    lv = {"plan": plan_levels(z["sample_j"], z["sample_i"], *land.shape), "sequential": None,
          "one_level": np.ones(len(z["sample_j"]), dtype=np.int32)}[levels]
    out = []
    for d in range(int(z["n_days"]) if days is None else days):
        pst.E_day = z["E_days"][d].copy()
        pref.step_daily(pst, pcfg, z["soil"][d])
        ist.layers, ist.bank, ist.E = pst.layers, pst.bank, z["E_indiv"][d].copy()
        info = iref.step_daily(ist, iref.Cfg.from_env(env), z["soil"][d], lv)
        pst.layers, pst.bank = ist.layers, ist.bank
        pcfg.weights = ist.weights
        out.append({"LAI_layers_SK": ist.layers.copy(), "LAI": ist.LAI.copy(), "seed_bank": ist.bank.copy(),
                    "species_weights": ist.weights.copy(), "stress_days": ist.stress.copy(), "E_indiv": ist.E.copy(),
                    "beta_hint": np.float64(info["beta_hint"]), "medE": np.float64(info["medE"])})
    return out


def test_every_case_has_a_golden_cpu():
    assert tuple(_case(p) for p in GOLDENS) == CASES
    for p in GOLDENS:
        assert os.path.getsize(p) < (1 << 20)


@pytest.mark.parametrize("path", GOLDENS, ids=_case)
@pytest.mark.parametrize("levels", ["plan", "sequential"])
def test_restatement_matches_reference_bitwise_cpu(path, levels):
    z = np.load(path)
    for d, got in enumerate(replay(z, levels)):
        for k, v in got.items():
            assert np.array_equal(v, z[f"day{d + 1}_{k}"], equal_nan=True), (_case(path), d, k)
    assert np.array_equal(plan_levels(z["sample_j"], z["sample_i"], 19, 36), z["levels"])


def test_one_level_for_everything_misses_the_full_golden_cpu():
    """SAMPLE_FRAC=1.0: every cell conflicts with a neighbour, so a plan without levels is another computation.  `one_level`
    keeps the stable order inside the level, which on the host is still the sequential loop -- so the wrong plan is shown the
    way a device runs it: every cell of the level reads the stack as it was before the level."""
    z = np.load(os.path.join(HERE, "golden", "indiv_daily_full_19x36.npz"))
    env = dict(zip(z["env_keys"], z["env_vals"]))
    land = z["land_mask"] == 1
    pst = pref.State(land, z["L0"].copy(), z["E_days"][0].copy(), np.zeros(land.shape), z["bank0"].copy(), land.astype(float))
    pref.step_daily(pst, pref.Cfg.from_env(env, [str(m) for m in z["modes"]], z["species_weights0"]), z["soil"][0])
    ist = iref.State(land, pst.layers, pst.bank, z["sample_j"], z["sample_i"], int(z["per_cell"]), z["species_id"], z["indiv_tol"],
                     z["E_indiv"][0].copy(), z["stress0"].copy())
    c = iref.Cfg.from_env(env)
    Wt, mean, denom = iref.cell_tables(ist, c)
    medE = iref.median_positive(denom)
    before, L = ist.layers.copy(), ist.layers.copy()
    for ci in range(len(z["sample_j"])):                       # one level: every cell sees the pre-level stack, deltas are summed
        one = before.copy()
        iref.one_cell(one, ci, int(z["sample_j"][ci]), int(z["sample_i"][ci]), Wt[ci], mean[ci], denom[ci], medE, c)
        L += one - before
    wrong = np.clip(np.maximum(L, 0.0), 0.0, c.lai_max)
    assert not np.array_equal(wrong, z["day1_LAI_layers_SK"])
    assert np.max(np.abs(wrong - z["day1_LAI_layers_SK"])) > 1e-6


def _masks():
    r = np.random.default_rng(5)
    out = [(np.load(p)["sample_j"], np.load(p)["sample_i"], 19, 36) for p in GOLDENS]
    for H, W, frac in ((5, 4, 1.0), (9, 24, 0.7), (19, 36, 0.2), (7, 20, 1.0)):
        idx = np.flatnonzero(r.random(H * W) < 0.6)
        idx = r.permutation(idx)[:max(1, int(frac * idx.size))]
        out.append((idx // W, idx % W, H, W))
    return out


@pytest.mark.parametrize("k", range(len(GOLDENS) + 4))
def test_plan_levels_properties_cpu(k):
    sj, si, H, W = _masks()[k]
    lv = plan_levels(sj, si, H, W)
    fps = [footprint(int(j), int(i), H, W) for j, i in zip(sj, si)]
    assert lv.dtype == np.int32 and lv.min() == 1
    for a in range(len(fps)):
        earlier = [lv[b] for b in range(a) if fps[a] & fps[b]]
        assert all(lv[a] > x for x in earlier)                 # every conflicting pair keeps its order
        assert lv[a] == 1 + max(earlier, default=0)            # and no level is higher than it must be
    for level in np.unique(lv):                                # within a level the footprints are disjoint
        seen = set()
        for a in np.flatnonzero(lv == level):
            assert not (seen & fps[a])
            seen |= fps[a]


def test_spill_targets_are_the_reference_zip_cpu():
    assert spill_targets(5, 7, 19, 36) == [(4, 6), (6, 8), (5, 7), (5, 7)] == iref.spill_targets(5, 7, 19, 36)
    assert spill_targets(0, 0, 19, 36) == [(0, 35), (1, 1), (0, 0), (0, 0)]
    assert spill_targets(18, 35, 19, 36) == [(17, 34), (18, 0), (18, 35), (18, 35)]


def test_np_sum_order_cpu():
    """The order the device restates for runs of 1 .. 64 terms is NumPy's, contiguous or strided."""
    r = np.random.default_rng(2)
    for n in range(1, 65):
        a = r.uniform(0.0, 1.0, n) * 10.0 ** r.integers(-8, 8, n)
        assert iref.np_sum(a) == np.sum(a), n
        b = np.zeros((n, 1, 3, 3)); b[:, 0, 1, 2] = a          # the [S, 1] column of a stack: a strided run
        assert iref.np_sum(a) == np.sum(b[:, :, 1, 2], axis=0)[0], n


def test_goldens_cover_what_they_claim_cpu():
    z = {_case(p): np.load(p) for p in GOLDENS}
    shapes = {k: v["L0"].shape[:2] for k, v in z.items()}
    assert shapes["sparse"] == (3, 1) and shapes["full"] == (4, 3) and shapes["wide"] == (9, 8) and shapes["ns20"] == (20, 1)
    full = z["full"]
    land = full["land_mask"] == 1
    assert len(full["sample_j"]) == land.sum() and np.array_equal(np.flatnonzero(land), full["sample_j"] * 36 + full["sample_i"])
    assert land[0].any() and land[-1].any() and land[[0, 0, -1, -1], [0, -1, 0, -1]].all() and (land[:, 0] & land[:, -1]).any()
    sp = z["sparse"]
    flat = sp["sample_j"].astype(int) * 36 + sp["sample_i"]
    assert (np.diff(flat) < 0).any() and int(sp["levels"].max()) > 1
    parity = {int(v[f"day{d}_n_positive"]) % 2 for v in z.values() for d in (1, 2)}
    assert parity == {0, 1}
    assert float(dict(zip(z["plain"]["env_keys"], z["plain"]["env_vals"]))["QD_ECO_INDIV_STRESS_PENALTY"]) == 0.0
    assert dict(zip(z["plain"]["env_keys"], z["plain"]["env_vals"]))["QD_ECO_INDIV_SEED_COUPLE"] == "0"
    assert np.isnan(z["nonfinite"]["E_indiv"]).any() and np.isinf(z["nonfinite"]["E_indiv"]).any()
    for v in z.values():
        assert (v["day2_stress_days"] == 365.0).any() and np.all(v["day1_E_indiv"] == 0.0)
        S, pc = v["L0"].shape[0], int(v["per_cell"])
        cnt = np.zeros((len(v["sample_j"]), S)); np.add.at(cnt, (np.repeat(np.arange(len(v["sample_j"])), pc), v["species_id"]), 1)
        if pc == 5:
            assert (cnt == 0).any()                            # (species, cell) pairs without an individual
        ocean_nb = [not (v["land_mask"][jj, ii] == 1) for j, i in zip(v["sample_j"], v["sample_i"]) for jj, ii in spill_targets(int(j), int(i), 19, 36)]
        assert any(ocean_nb)
    # a cell that reaches lai_max, a cell with total_old == 0, cells above and below medE (recruits occur)
    got = replay(full, days=1)[0]
    tot1 = np.sum(z["full"]["day1_LAI_layers_SK"], axis=(0, 1))
    assert np.isclose(tot1, 1.2, rtol=0, atol=1e-9).any() or (tot1 > 1.19).any()
    assert (np.sum(full["L0"], axis=(0, 1))[land] == 0.0).any()
    assert np.array_equal(got["LAI_layers_SK"], full["day1_LAI_layers_SK"])


def test_env_parsing_and_defaults_cpu(monkeypatch):
    from qingdai_amd.ecology import IndividualDaily

    class Dev:
        def indiv_daily_configure(self, params, species, levels):
            self.got = (params, np.asarray(species), np.asarray(levels))

        def indiv_daily_firings(self):
            return 0

    def build(env):
        for k in [k for k in os.environ if k.startswith("QD_ECO_")]:
            monkeypatch.delenv(k)
        for k, v in env.items():
            monkeypatch.setenv(k, v)
        dev = Dev()
        daily = type("D", (), {"repro_fraction": float(env.get("QD_ECO_REPRO_FRACTION", "0.2")),
                               "params": type("P", (), {"lai_max": float(env.get("QD_ECO_LAI_MAX", "5.0"))})()})()
        pop = type("Pop", (), {"daily": daily, "_dev": dev, "Ns": 3, "K": 2, "_weights": np.ones(3) / 3, "indiv_daily": None,
                               "species_weights": None})()
        pool = type("Pool", (), {"per_cell": 4, "sample_j": np.array([1, 1, 2]), "sample_i": np.array([1, 2, 3]), "h": 19, "w": 36,
                                 "indiv_species_id": np.zeros(12, dtype=np.int32), "daily": None})()
        return IndividualDaily(pool, pop), dev, pool, pop

    d, dev, pool, pop = build({})
    p = d.params
    assert (p.n_species, p.n_layers, p.per_cell, p.seed_couple) == (3, 2, 4, 1)
    assert (p.stress_penalty, p.lai_grow, p.lai_decay, p.recruit_frac, p.stress_decay) == (0.2, 0.002, 0.001, 0.2, 0.5)
    assert (p.repro_frac, p.seed_energy, p.retain, p.bank_max, p.lai_max) == (0.2, 1.0, 0.2, 1000.0, 5.0)
    assert ctypes.sizeof(p) == 4 * 4 + 10 * 8 and list(dev.got[2]) == [1, 1, 2] and d.n_levels == 2
    assert pool.daily is d and pop.indiv_daily is d
    d, *_ = build({"QD_ECO_INDIV_STRESS_PENALTY": "0", "QD_ECO_LAI_GROWTH_RATE": "0.05", "QD_ECO_LAI_DECAY_RATE": "0.004",
                   "QD_ECO_LAI_RECRUIT_FRAC": "0.5", "QD_ECO_INDIV_SEED_COUPLE": "0", "QD_ECO_INDIV_STRESS_DECAY": "0.25",
                   "QD_ECO_REPRO_FRACTION": "0.3", "QD_ECO_SEED_ENERGY": "200", "QD_ECO_SEED_BANK_RETAIN": "0.35",
                   "QD_ECO_SEED_BANK_MAX": "2.0", "QD_ECO_LAI_MAX": "1.2"})
    p = d.params
    assert (p.stress_penalty, p.lai_grow, p.lai_decay, p.recruit_frac, p.seed_couple, p.stress_decay) == (0.0, 0.05, 0.004, 0.5, 0, 0.25)
    assert (p.repro_frac, p.seed_energy, p.retain, p.bank_max, p.lai_max) == (0.3, 200.0, 0.35, 2.0, 1.2)
    # the seed-coupling block swallows a value that does not parse and goes without the coupling; the others are errors
    d, *_ = build({"QD_ECO_SEED_BANK_RETAIN": "much"})
    assert d.params.seed_couple == 0
    with pytest.raises(ValueError):
        build({"QD_ECO_LAI_GROWTH_RATE": "fast"})
    with pytest.raises(ValueError, match="needs a population whose daily step runs on the device"):
        IndividualDaily(pool, type("Pop", (), {"daily": None})())


def test_driver_switch_and_refusals_cpu():
    from qingdai_amd.driver import indiv_daily_enabled
    ok = dict(eco_daily=True, ecology=True, population=True, individuals=True, daily_hook=False)
    assert indiv_daily_enabled({}, **ok) is False and indiv_daily_enabled({"QD_ECO_INDIV_DAILY": "0"}, **ok) is False
    assert indiv_daily_enabled({}, **{**ok, "eco_daily": False}) is False            # off: nothing is asked
    assert indiv_daily_enabled({"QD_ECO_INDIV_DAILY": "1"}, **ok) is True
    for key, word in (("eco_daily", "QD_ECO_DAILY=1"), ("ecology", "QD_ECO_ENABLE=1"), ("population", "a population"),
                      ("individuals", "individuals"), ("daily_hook", "no daily_hook")):
        with pytest.raises(ValueError, match="QD_ECO_INDIV_DAILY=1 needs .*" + re.escape(word)):
            indiv_daily_enabled({"QD_ECO_INDIV_DAILY": "1"}, **{**ok, key: not ok[key]})


def test_diag_line_is_the_references_cpu():
    for p in GOLDENS:
        z = np.load(p)
        for d in (1, 2):
            assert indiv_daily_line(len(z["sample_j"]), int(z["per_cell"]), float(z[f"day{d}_beta_hint"])) == str(z["lines"][d - 1])


def test_abi_names_cpu():
    # names, layout and constants against the header and the library: tests/test_abi_cpu.py, for every symbol and struct
    assert _lib.INDIV_DAILY_LOG_W == 4
    src = open(os.path.join(HERE, "..", "qingdai_amd", "csrc", "qd_indiv_daily.hip")).read()
    assert "atomic" not in src.replace("no atomics", "")
