"""CPU: speciation's host side and its NumPy restatement, no GPU and no libqingdai_hip.so.  The restatement of the event and the
seven-stage sequences against the reference's goldens (bitwise); Gene.mutated and Speciation.event against the goldens' parents,
genes and reflectance tables, draw for draw from np.random.RandomState(seed); the draw memo (the same events whatever the chunk
cuts are, also when a step holds several firings); the driver's start-up refusals and its acceptance with the switch; the export
document against the reference's own file; the new ABI name."""
import glob
import json
import os
import re
import types

import numpy as np
import pytest

import speciation_ref as ref

HERE = os.path.dirname(os.path.abspath(__file__))
GOLD = os.path.join(HERE, "golden")
GOLDENS = sorted(glob.glob(os.path.join(GOLD, "speciation_*_*x*.npz")))
CASES = ["e24", "e8", "eps07", "modes", "noland", "nonfinite", "ns20", "p24", "p25", "p8", "p9", "parent0", "parentlast", "smax", "wide"]


def _case(p):
    return os.path.basename(p).split("_")[1]


def _clean_env(monkeypatch, env=None):
    for k in [k for k in os.environ if k.startswith("QD_ECO_")]:
        monkeypatch.delenv(k)
    for k, v in (env or {}).items():
        monkeypatch.setenv(k, v)


def _gene(rec):
    from qingdai_amd.ecology import Gene
    return Gene(identity=rec["identity"], alloc_root=rec["alloc"][0], alloc_stem=rec["alloc"][1], alloc_leaf=rec["alloc"][2],
                leaf_area_per_energy=rec["leaf_area_per_energy"], peaks=[tuple(p) for p in rec["peaks"]],
                drought_tolerance=rec["drought_tolerance"], gdd_germinate=rec["gdd_germinate"], lifespan_days=rec["lifespan_days"],
                provenance=rec["provenance"])


def _record(g):
    return {"identity": g.identity, "alloc": [g.alloc_root, g.alloc_stem, g.alloc_leaf], "leaf_area_per_energy": g.leaf_area_per_energy,
            "peaks": [list(p) for p in g.peaks], "drought_tolerance": g.drought_tolerance, "gdd_germinate": g.gdd_germinate,
            "lifespan_days": int(g.lifespan_days), "provenance": g.provenance}


def test_every_case_has_a_golden_cpu():
    assert [_case(p) for p in GOLDENS] == CASES
    assert os.path.basename(GOLDENS[-1]) == "speciation_wide_5x130.npz" and os.path.exists(os.path.join(GOLD, "genes_export_speciation.json"))


@pytest.mark.parametrize("path", GOLDENS, ids=_case)
def test_restatement_matches_reference_bitwise_cpu(path):
    z = np.load(path)
    env = ref.env_of(z)
    frac, lai_max, land = float(env.get("QD_ECO_MUT_EPS", "0.02")), float(env.get("QD_ECO_LAI_MAX", "5.0")), z["land_mask"] == 1
    for h in (1, 2):                                            # the event alone, from the stack the reference's split found
        if not bool(z[f"hit{h}_split"]):
            continue
        tag = f"s{int(z['hit_firings'][h - 1]) + 1}"
        assert float(z[f"hit{h}_frac"]) == frac
        new = ref.split(z[f"hit{h}_pre_stack"], int(z[f"hit{h}_parent"]), frac, lai_max)
        assert np.array_equal(new, z[f"{tag}_stack"], equal_nan=True) and np.array_equal(ref.total(new), z[f"{tag}_LAI"], equal_nan=True)
        assert np.array_equal(ref.weights(new, land), z[f"{tag}_weights"])
    stages = ref.replay(z)                                      # the whole sequence, firings included
    assert [t for t, _ in stages] == [f"s{d + 1}" for d in range(7)]
    for tag, got in stages:
        for k, v in got.items():
            assert np.array_equal(v, z[f"{tag}_{k}"], equal_nan=True), (tag, k)


def test_goldens_cover_what_they_claim_cpu():
    z = {_case(p): np.load(p) for p in GOLDENS}
    planes = {c: z[c]["L0"].shape[0] * z[c]["L0"].shape[1] for c in z}
    assert (planes["p8"], planes["p9"], planes["p24"], planes["p25"]) == (8, 9, 24, 25)
    assert z["e8"]["s3_stack"].shape[0] == 8 and z["e8"]["s6_stack"].shape[0] == 9                # the kernel's species-table sizes
    assert z["e24"]["s3_stack"].shape[0] == 24 and z["e24"]["s6_stack"].shape[0] == 25
    assert z["ns20"]["L0"].shape[:2] == (20, 1)
    assert int(z["parent0"]["hit1_parent"]) == 0 and int(z["parentlast"]["hit1_parent"]) == z["parentlast"]["L0"].shape[0] - 1
    assert ref.env_of(z["eps07"])["QD_ECO_MUT_EPS"] == "0.7"
    pre, post = z["eps07"]["hit1_pre_stack"], z["eps07"]["s3_stack"]
    p = int(z["eps07"]["hit1_parent"])
    assert np.array_equal(post[-1], np.clip(0.5 * pre[p], 0.0, 5.0))                             # 0.7 is clipped to 0.5
    nf_pre, nf_post = z["nonfinite"]["hit1_pre_stack"], z["nonfinite"]["s3_stack"]
    land = z["nonfinite"]["land_mask"] == 1
    assert np.isnan(nf_pre[:, :, land]).any() and np.isnan(nf_pre[:, :, ~land]).any() and (nf_pre > 5.0).any()
    assert np.isnan(nf_post).sum() >= np.isnan(nf_pre).sum() and not (nf_post > 5.0).any() and np.isfinite(z["nonfinite"]["s3_weights"]).all()
    assert not z["noland"]["land_mask"].any() and np.array_equal(z["noland"]["s3_weights"], np.full(4, 0.25))
    assert bool(z["smax"]["hit1_split"]) and not bool(z["smax"]["hit2_split"]) and z["smax"]["s7_stack"].shape[0] == 4
    assert json.loads(str(z["smax"]["lines"]))[1] == ["[Ecology] mutation skipped: species_max=4 reached."]
    assert [str(m) for m in z["modes"]["modes"]] == ["diffusion"] and z["modes"]["s7_stack"].shape[0] == 3
    for c in z:                                                 # no parent hangs on the last bits of the weights
        for h in (1, 2):
            if bool(z[c][f"hit{h}_split"]):
                assert float(z[c][f"hit{h}_choice_gap"]) > 1e-9, (c, h)


def test_new_index_one_spreads_by_seed_cpu():
    """The modes golden moves differently when the new index 1 is given `diffusion`: the mode rule is live in it."""
    z = np.load(os.path.join(GOLD, "speciation_modes_19x36.npz"))
    real = ref.new_mode
    try:
        ref.new_mode = lambda index: "diffusion"
        wrong = dict(ref.replay(z))
    finally:
        ref.new_mode = real
    assert np.array_equal(wrong["s3"]["stack"], z["s3_stack"]) and not np.array_equal(wrong["s4"]["stack"], z["s4_stack"])
    from qingdai_amd.ecology import new_species_mode
    assert [new_species_mode(i) for i in (0, 1, 2, 20)] == ["diffusion", "seed", "diffusion", "diffusion"]


# ------------------------------------------------------------------ the host classes on a stub population
class StubPop:
    """What Speciation.event asks of a PopulationCanopy, with the split through the restatement."""

    def __init__(self, stack, weights, land, lai_max=5.0):
        self.stack, self.species_weights, self.land, self.lai_max = stack, np.array(weights, dtype=float), land, lai_max
        self.R = None
        self.calls = []

    @property
    def Ns(self):
        return self.stack.shape[0]

    def add_species_from_parent(self, parent, frac=0.02):
        self.calls.append((int(parent), float(frac)))
        self.stack = ref.split(self.stack, parent, frac, self.lai_max)
        self.species_weights = ref.weights(self.stack, self.land)
        return self.Ns - 1

    def set_species_reflectance_bands(self, R):
        self.R = np.clip(np.asarray(R, dtype=float), 0.0, 1.0)


def _adapter(z, genes=None, diag=False):
    from qingdai_amd import spectral as sp
    bands = sp.make_bands()
    w_b = sp.band_weights_from_mode(bands)
    pop = StubPop(z["L0"].copy(), z["species_weights0"], z["land_mask"] == 1)
    genes = [_gene(r) for r in json.loads(str(z["genes0"]))] if genes is None else genes
    return types.SimpleNamespace(pop=pop, genes_list=genes, bands=bands, w_b=w_b, _diag=diag)


@pytest.mark.parametrize("path", GOLDENS, ids=_case)
def test_event_and_mutated_gene_match_reference_draw_for_draw_cpu(path, monkeypatch, capsys):
    """RandomState(seed) through the seven stages: rand() only on the forced hits, then choice, then the gene's draws -- the parent,
    the gene (every field bitwise) and the reflectance table are the reference's."""
    from qingdai_amd.ecology import Speciation
    z = np.load(path)
    env = ref.env_of(z)
    _clean_env(monkeypatch, env)
    ad = _adapter(z, diag=env.get("QD_ECO_DIAG") == "1")
    assert np.array_equal(ad.w_b, z["w_b"])
    spec = Speciation(mut_rate=0.0, rng=np.random.RandomState(int(z["seed"])))
    assert spec.mut_eps == float(env.get("QD_ECO_MUT_EPS", "0.02")) and spec.species_max == int(env["QD_ECO_SPECIES_MAX"])
    hit, lines = 0, []
    for d in range(7):
        spec.mut_rate = 1.0 if d in z["hit_firings"].tolist() else 0.0
        if spec.mut_rate:                                      # the stack and the weights the reference's event found
            hit += 1
            if bool(z[f"hit{hit}_split"]):
                ad.pop.stack = z[f"hit{hit}_pre_stack"].copy()
        capsys.readouterr()
        idx = spec.event(ad)
        out = capsys.readouterr().out.splitlines()
        if not spec.mut_rate:
            assert idx is None and out == []
            continue
        lines.append(out)
        if not bool(z[f"hit{hit}_split"]):
            assert idx is None
            continue
        tag = f"s{d + 1}"
        assert idx == ad.pop.Ns - 1 == len(ad.genes_list) - 1
        assert ad.pop.calls[-1] == (int(z[f"hit{hit}_parent"]), float(z[f"hit{hit}_frac"]))
        assert _record(ad.genes_list[-1]) == json.loads(str(z[f"hit{hit}_gene"]))
        assert np.array_equal(ad.pop.R, z[f"hit{hit}_R"]) and np.array_equal(ad.pop.species_weights, z[f"{tag}_weights"])
    assert lines == json.loads(str(z["lines"])) and spec.n_done == 7


def _drive(cuts, seed, dt, day, look=0):
    """The driver's chunk rule without a device: speciation_due names the steps before a hit's step; the firings of a span pass,
    those of the hit's step go through event() one by one -> (events, firings)."""
    from qingdai_amd.driver import Simulation
    from qingdai_amd.ecology import Speciation, daily_counts
    z = np.load(os.path.join(GOLD, "speciation_parent0_19x36.npz"))
    ad = _adapter(z)
    sim = Simulation.__new__(Simulation)
    sim.dt = dt
    sim.eco_daily = lane = types.SimpleNamespace(accum_day=0.0, day_seconds=day)
    sim.speciation = spec = Speciation(mut_rate=0.3, mut_eps=0.02, species_max=1000, rng=np.random.RandomState(seed))
    events, firings = [], 0
    for n in cuts:
        if look:
            sim.speciation_due(n + look)                        # a look further than the chunk that then runs
        left = n
        while left > 0:
            k = sim.speciation_due(left)
            run = left if k is None else k
            if run > 0:
                fire, lane.accum_day = daily_counts(lane.accum_day, dt, run, day)
                spec.passed(int(fire.sum()))
                firings += int(fire.sum())
                left -= run
            if k is not None:
                fire, lane.accum_day = daily_counts(lane.accum_day, dt, 1, day)
                hit = False
                for q in range(int(fire[0])):
                    if spec.event(ad) is not None:
                        hit = True
                        events.append((firings + q + 1, ad.pop.calls[-1][0]))
                assert hit                                      # the step was named for a hit
                firings += int(fire[0])
                left -= 1
    return events, firings, [_record(g) for g in ad.genes_list], ad.pop.stack


@pytest.mark.parametrize("dt,day", [(300.0, 1000.0), (2500.0, 1000.0)], ids=["day_over_dt", "several_firings_a_step"])
def test_draw_memo_same_stream_whatever_the_cuts_cpu(dt, day):
    from qingdai_amd.ecology import Speciation, daily_counts
    z = np.load(os.path.join(GOLD, "speciation_parent0_19x36.npz"))
    total = 120
    # firing by firing, no looking ahead: the reference's order of draws
    ad = _adapter(z)
    spec = Speciation(mut_rate=0.3, mut_eps=0.02, species_max=1000, rng=np.random.RandomState(11))
    fire, _ = daily_counts(0.0, dt, total, day)
    want, f = [], 0
    for c in fire.tolist():
        for _ in range(c):
            f += 1
            if spec.event(ad) is not None:
                want.append((f, ad.pop.calls[-1][0]))
    genes, stack = [_record(g) for g in ad.genes_list], ad.pop.stack
    assert len(want) >= 5 and f == int(fire.sum())
    for cuts, look in (([total], 0), ([1] * total, 0), ([7, 13, 50, 50], 0), ([40, 40, 40], 60), ([3] * 40, 200)):
        ev, n, g, st = _drive(cuts, 11, dt, day, look)
        assert (ev, n) == (want, f), (cuts, look)
        assert g == genes and np.array_equal(st, stack)


def test_hit_ahead_draws_once_and_not_without_a_rate_cpu():
    from qingdai_amd.ecology import Speciation

    class Counting(np.random.RandomState):
        n = 0

        def rand(self, *a):
            self.n += 1
            return super().rand(*a)
    rng = Counting(3)
    spec = Speciation(mut_rate=0.5, rng=rng, env={})
    a = [spec.hit_ahead(k) for k in (1, 2, 3)]
    assert rng.n == 3 and [spec.hit_ahead(k) for k in (1, 2, 3)] == a and rng.n == 3
    off = Speciation(mut_rate=0.0, rng=rng, env={})
    assert off.hit_ahead(1) is False and off.event(None) is None and rng.n == 3
    assert (off.mut_eps, off.species_max) == (0.02, 8)
    bad = Speciation(env={"QD_ECO_MUT_RATE": "x", "QD_ECO_MUT_EPS": "y", "QD_ECO_SPECIES_MAX": "2.5"})
    assert (bad.mut_rate, bad.mut_eps, bad.species_max) == (0.0, 0.02, 8)


def test_struck_firings_leave_the_schedule_and_keep_the_clock_cpu():
    from qingdai_amd.ecology import PopulationDaily, daily_counts
    sent = []
    lane = PopulationDaily.__new__(PopulationDaily)
    lane.accum_day, lane.day_seconds, lane.struck = 900.0, 1000.0, 0
    lane.dev = types.SimpleNamespace(eco_daily_schedule=lambda f: sent.append(np.array(f)))
    clock = lane.span_clock()
    lane.struck = 1
    assert lane.span_schedule(0.0, 300.0, 4) == 1 and sent[-1].tolist() == [0, 0, 0, 1] and lane.struck == 0      # [1, 0, 0, 1] as the clock has it
    assert lane.accum_day == daily_counts(900.0, 300.0, 4, 1000.0)[1]
    lane.span_restore(clock)
    assert (lane.accum_day, lane.struck) == (900.0, 0)
    lane.struck = 2
    with pytest.raises(ValueError, match="struck out"):
        lane.span_schedule(0.0, 300.0, 4)


# ------------------------------------------------------------------ the driver's switch
def test_driver_switch_refusals_and_acceptance_cpu():
    from qingdai_amd.driver import eco_daily_enabled, speciation_enabled
    on = {"QD_ECO_DAILY": "1", "QD_ECO_SPECIATION": "1", "QD_ECO_MUT_RATE": "0.05"}
    ok = dict(eco_daily=True, daily_hook=False)
    assert speciation_enabled({}, **ok) is False and speciation_enabled({"QD_ECO_SPECIATION": "0"}, **ok) is False
    assert eco_daily_enabled(on) is True and speciation_enabled(on, **ok) is True
    with pytest.raises(ValueError, match="QD_ECO_DAILY=1 does not support QD_ECO_MUT_RATE > 0"):           # today's message at 0
        eco_daily_enabled({"QD_ECO_DAILY": "1", "QD_ECO_MUT_RATE": "0.05", "QD_ECO_SPECIATION": "0"})
    with pytest.raises(ValueError, match="QD_ECO_SPECIATION=1 needs QD_ECO_DAILY=1"):
        speciation_enabled(on, eco_daily=False, daily_hook=False)
    with pytest.raises(ValueError, match="QD_ECO_SPECIATION=1 needs no daily_hook"):
        speciation_enabled(on, eco_daily=True, daily_hook=True)
    with pytest.raises(ValueError, match="does not run with QD_ECO_INDIV_DAILY=1"):
        speciation_enabled({**on, "QD_ECO_INDIV_DAILY": "1"}, **ok)
    for eps in ("0", "-0.1"):
        with pytest.raises(ValueError, match="needs QD_ECO_MUT_EPS > 0"):
            speciation_enabled({**on, "QD_ECO_MUT_EPS": eps}, **ok)
    with pytest.raises(ValueError, match="needs QD_ECO_SPECIES_MAX <= 64"):
        speciation_enabled({**on, "QD_ECO_SPECIES_MAX": "65"}, **ok)
    assert speciation_enabled({**on, "QD_ECO_SPECIES_MAX": "64", "QD_ECO_MUT_EPS": "0.7"}, **ok) is True


# ------------------------------------------------------------------ genes export
def test_export_document_matches_the_reference_file_cpu(tmp_path, monkeypatch, capsys):
    from qingdai_amd.ecology import EcologyAdapter, genes_export_document, genes_export_path
    z = np.load(os.path.join(GOLD, "speciation_modes_19x36.npz"))
    with open(os.path.join(GOLD, "genes_export_speciation.json"), encoding="utf-8") as f:
        want = json.load(f)
    _clean_env(monkeypatch, ref.env_of(z))
    ad = _adapter(z)
    genes = [_gene(r) for r in json.loads(str(z["genes0"]))] + [_gene(json.loads(str(z[f"hit{h}_gene"]))) for h in (1, 2)]
    doc = genes_export_document(genes, ad.bands, ad.w_b, z["s7_weights"], 12.34)
    assert doc == want and list(doc) == list(want) and [list(g) for g in doc["genes"]] == [list(g) for g in want["genes"]]
    assert "species_weights" not in doc and len(doc["genes"]) == 3 and all("weight" in g and "lambda_edges_nm" in g for g in doc["genes"])
    assert doc["genes"][1]["identity"].endswith("_mut") and doc["genes"][1]["provenance"] is None
    assert os.path.basename(genes_export_path("o", 12.34)) == "genes_day_012.3.json" == os.path.basename(genes_export_path("o", 12.3))
    eco = EcologyAdapter.__new__(EcologyAdapter)
    eco._genes, eco.bands, eco.w_b, eco._diag = genes, ad.bands, ad.w_b, True
    eco.pop = types.SimpleNamespace(species_weights=z["s7_weights"])
    eco.export_genes(str(tmp_path / "out"), 12.34)
    path = str(tmp_path / "out" / "genes_day_012.3.json")
    assert capsys.readouterr().out == f"[Ecology] Genes exported: {path} (Ns=3, schema=3)\n"
    with open(path, encoding="utf-8") as f:
        assert json.load(f) == want


# ------------------------------------------------------------------ ABI
def test_abi_name_declared_and_listed_cpu():
    with open(os.path.join(HERE, "..", "include", "qingdai_hip.h")) as f:
        h = f.read()
    assert re.search(r"int qd_eco_daily_speciate\(qd_handle h, int parent, double frac, double\* weights_out\);", h)
    lib = os.path.join(HERE, "..", "qingdai_amd", "libqingdai_hip.so")
    if os.path.exists(lib):
        with open(lib, "rb") as f:
            assert b"qd_eco_daily_speciate\x00" in f.read()
