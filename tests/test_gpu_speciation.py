"""GPU (-m gpu): speciation on the device (qd_eco_daily_speciate, QD_ECO_SPECIATION=1).  (a) the entry point against every event of
the reference's goldens; (b) the goldens' whole seven-stage sequences -- firings, the draws of np.random.RandomState(seed), events,
the firings after them -- through the class seam; (c) ragged rows and degenerate masks against the NumPy restatement, QD_ECO_F32=1, the refusals; (d) a driver
run with the switch on and a generator that never hits against the run with the switch off; (e) a driver run whose hits fall
mid-chunk against the same run driven firing by firing; (f) diversity, autosave / resume and the genes export after an event.

Tolerances.  Deviations are max |a - b| / max |b| per array (util.relerr).
  stack, ECO_LAI of an event   bit for bit (the split is one multiply and one subtract, the sums run in NumPy's order).
  weights of an event          the land sums are blocked on the device and pairwise in NumPy: a reordered sum of n non-negative
                               terms moves by at most (n - 1) 2^-53 relative, their ratio by twice that: 2 (n - 1) 2^-53 with
                               n = land cells (WEIGHT_BOUND(n); 6.8e-14 at the 308 land cells of the largest mask here).
                               MEASURED_WEIGHTS is the largest deviation the MI355X gave over all goldens.
  firings                      the rule of tests/test_gpu_eco_daily.py (its BOUND) for every stage before the first event.
  firings behind an event      germination adds w_s * add to layer 0 with the device's weights, so the stack may move by the
                               weights' deviation: POST_BOUND = max(BOUND, 4 * MEASURED_POST), never above WEIGHT_BOUND(n).
                               MEASURED_POST is the largest deviation of a stage behind an event from the reference golden.
Measured on the MI355X over the fifteen goldens: weights of an event 5.74e-16 at most (p9; the ragged shapes of (c) 3.54e-16); a
stage behind an event 7.59e-16 at most (modes; stack), against 6.51e-16 for the stages before one -- so 4 * MEASURED_POST = 3.0e-15
stays below BOUND = 3.3e-15 and nothing is widened.  Every test prints its deviations before it asserts."""
import glob
import json
import os

import numpy as np
import pytest

import speciation_ref as ref
from util import relerr

pytestmark = pytest.mark.gpu

HERE = os.path.dirname(os.path.abspath(__file__))
GOLD = os.path.join(HERE, "golden")
GOLDENS = sorted(glob.glob(os.path.join(GOLD, "speciation_*_*x*.npz")))
BOUND = min(1e-14, 10 * 3.3e-16)       # tests/test_gpu_eco_daily.py: START and 10 x MEASURED
MEASURED_WEIGHTS = 5.8e-16             # largest deviation of an event's weights from the goldens on the MI355X
MEASURED_POST = 7.6e-16                # largest deviation of a stage behind an event from the goldens on the MI355X
PROGNOSTIC = ("U", "V", "H", "TS", "Q", "CLOUD", "HICE", "W_LAND", "S_SNOW", "ALBEDO")
ECO_FIELDS = ("ECO_LAI", "ECO_EDAY", "ECO_AGE", "ECO_SEEDBANK", "ECO_GATE", "ECO_ALPHA", "ECO_F", "ECO_ALPHA_BANDED")


def WEIGHT_BOUND(n_land):
    return 2.0 * max(n_land - 1, 0) * 2.0 ** -53


def POST_BOUND(n_land):
    return BOUND if MEASURED_POST is None else min(max(BOUND, 4 * MEASURED_POST), max(BOUND, WEIGHT_BOUND(n_land)))


def _case(p):
    return os.path.basename(p).split("_")[1]


def _clean_env(monkeypatch, env=None):
    for k in [k for k in os.environ if k.startswith(("QD_ECO_", "QD_PHYTO_", "QD_OUTPUT_DIR"))]:
        monkeypatch.delenv(k)
    for k, v in (env or {}).items():
        monkeypatch.setenv(str(k), str(v))


def _eco_on(shape, land_mask):
    import qingdai_amd as qa
    from qingdai_amd.device import Device
    from qingdai_amd.ecology import EcologyAdapter, PopulationDaily
    grid = qa.SphericalGrid(*shape)
    dev = Device(grid)
    dev.upload_now("LAND_MASK", land_mask)
    eco = EcologyAdapter(grid, land_mask, dev=dev, albedo_couple=True)
    PopulationDaily(eco.pop)
    return dev, eco


def _wdev(got, want):
    return float(np.max(np.abs(got - want) / np.maximum(np.abs(want), 1e-300)))


# ------------------------------------------------------------------ (a) the entry point against every event of the goldens
@pytest.mark.parametrize("path", GOLDENS, ids=_case)
def test_entry_point_vs_reference_goldens(gpu, path, monkeypatch):
    z = np.load(path)
    env = ref.env_of(z)
    land = z["land_mask"]
    n_land = int((land == 1).sum())
    for h in (1, 2):
        if not bool(z[f"hit{h}_split"]):
            continue
        pre, tag = z[f"hit{h}_pre_stack"], f"s{int(z['hit_firings'][h - 1]) + 1}"
        S, K = pre.shape[:2]
        _clean_env(monkeypatch, {**env, "QD_ECO_NS": S, "QD_ECO_COHORT_K": K})
        dev, eco = _eco_on(land.shape, land)
        pop = eco.pop
        assert (pop.Ns, pop.K) == (S, K)
        pop.push_layers(pre, init=True)
        age, bank = z[f"{tag}_age"], z[f"{tag}_bank"]
        dev.upload_now("ECO_AGE", age); dev.upload_now("ECO_SEEDBANK", bank)
        before, fired = pop.state(), dev.eco_daily_firings()
        idx = pop.add_species_from_parent(int(z[f"hit{h}_parent"]), float(z[f"hit{h}_frac"]))
        assert idx == S == pop.Ns - 1 and pop.daily.params.n_species == S + 1
        assert pop.daily.species_modes[-1] == ("seed" if S == 1 else "diffusion") and len(pop.daily.species_modes) == S + 1
        stack, lai, w = pop.LAI_layers_SK, pop.total_LAI(), pop.species_weights
        dw = _wdev(w, z[f"{tag}_weights"])
        print(f"{_case(path)} hit {h}: S={S}->{S + 1} K={K} parent={int(z[f'hit{h}_parent'])} weights deviation {dw:.3e} "
              f"(bound {WEIGHT_BOUND(n_land):.3e}, n={n_land})")
        assert stack.shape == z[f"{tag}_stack"].shape and np.array_equal(stack, z[f"{tag}_stack"], equal_nan=True)
        assert np.array_equal(lai, z[f"{tag}_LAI"], equal_nan=True)
        assert dw <= WEIGHT_BOUND(n_land) and w.shape == (S + 1,)
        # what the event leaves alone
        assert np.array_equal(pop.age_days, age) and np.array_equal(pop.seed_bank, bank) and dev.eco_daily_firings() == fired
        after = pop.state()
        assert (after["hours"], after["next_recompute_hours"], after["n_recompute"]) == (before["hours"], before["next_recompute_hours"], before["n_recompute"])
        dev.close()


# ------------------------------------------------------------------ (b) the whole sequences through the class seam
@pytest.mark.parametrize("path", GOLDENS, ids=_case)
def test_sequence_vs_reference_goldens(gpu, path, monkeypatch, capsys):
    from qingdai_amd.ecology import Speciation
    z = np.load(path)
    env = ref.env_of(z)
    land = z["land_mask"]
    n_land = int((land == 1).sum())
    _clean_env(monkeypatch, env)
    dev, eco = _eco_on(land.shape, land)
    pop = eco.pop
    assert pop.daily.species_modes == [str(m) for m in z["modes"]] and np.array_equal(pop.species_weights, z["species_weights0"])
    pop.push_layers(z["L0"], init=True)
    pop.seed_bank = z["bank0"]
    spec = Speciation(mut_rate=0.0, rng=np.random.RandomState(int(z["seed"])))
    hit, events, lines, worst_pre, worst_post, worst_w = 0, 0, [], 0.0, 0.0, 0.0
    for d in range(int(z["n_firings"])):
        tag = f"s{d + 1}"
        pop.E_day = z["E_days"][d]
        pop.step_daily(z["soil"][d])
        spec.mut_rate = 1.0 if d in z["hit_firings"].tolist() else 0.0
        capsys.readouterr()
        idx = spec.event(eco)
        out = capsys.readouterr().out
        split = False
        if spec.mut_rate:
            hit += 1
            lines.append([l for l in out.splitlines() if "mutation" in l])
            split = bool(z[f"hit{hit}_split"])
            assert (idx is not None) == split
            if split:
                events += 1
                g = eco.genes_list[-1]
                want = json.loads(str(z[f"hit{hit}_gene"]))
                assert pop.daily.species_modes[-1] == ref.new_mode(pop.Ns - 1)
                assert (g.identity, [list(p) for p in g.peaks], g.lifespan_days) == (want["identity"], want["peaks"], want["lifespan_days"])
                assert np.array_equal(pop._species_R_leaf, z[f"hit{hit}_R"])
        got = {"stack": pop.LAI_layers_SK, "LAI": pop.total_LAI(), "age": pop.age_days, "bank": pop.seed_bank}
        want = {"stack": z[f"{tag}_stack"], "LAI": z[f"{tag}_LAI"] if split else z[f"{tag}_total_LAI"], "age": z[f"{tag}_age"], "bank": z[f"{tag}_bank"]}
        assert got["stack"].shape == want["stack"].shape, tag
        finite = {k: np.isfinite(want[k]) for k in want}
        errs = {k: relerr(np.where(finite[k], got[k], 0.0), np.where(finite[k], want[k], 0.0)) for k in want}
        for k in want:
            assert np.array_equal(np.isnan(got[k]), np.isnan(want[k])), (tag, k)
        dw = _wdev(pop.species_weights, z[f"{tag}_weights"])
        with capsys.disabled():
            print(_case(path), tag, {k: f"{e:.2e}" for k, e in errs.items()}, f"weights {dw:.2e}", "behind an event" if events else "")
        bound = POST_BOUND(n_land) if events and not (split and events == 1) else BOUND
        if events:
            worst_post, worst_w = max(worst_post, max(errs.values())), max(worst_w, dw)
        else:
            worst_pre = max(worst_pre, max(errs.values()))
        for k, e in errs.items():
            assert e <= bound, (tag, k, e, bound)
        # the first event's weights come from a stack within BOUND of the reference's; the second event's from one within POST_BOUND
        assert dw <= WEIGHT_BOUND(n_land) + (POST_BOUND(n_land) if events > 1 else 0.0), (tag, dw)
        assert np.array_equal(got["age"], want["age"])
    with capsys.disabled():
        print(f"{_case(path)}: largest deviation before an event {worst_pre:.3e}, behind one {worst_post:.3e} (bound {POST_BOUND(n_land):.3e}), "
              f"weights {worst_w:.3e} (bound {WEIGHT_BOUND(n_land):.3e})")
    assert lines == json.loads(str(z["lines"])) and pop.Ns == json.loads(str(z["meta"]))["final_species"]
    assert dev.eco_daily_firings() == 7 == pop.daily.n_firings and spec.n_done == 7
    dev.close()


# ------------------------------------------------------------------ (c) ragged rows, degenerate masks, against the restatement
@pytest.mark.parametrize("n_lon", [4, 63, 65, 130, 257])
@pytest.mark.parametrize("mask", ["mixed", "all_land", "no_land"])
def test_ragged_rows_and_degenerate_masks_vs_restatement(gpu, n_lon, mask, monkeypatch):
    """The smallest handle is 5 x 4 (qd_create refuses n_lon < 4), so 4 stands for the narrowest row; 257 crosses the block width."""
    S, K, n_lat = 9, 2, 5
    _clean_env(monkeypatch, {"QD_ECO_NS": S, "QD_ECO_COHORT_K": K, "QD_ECO_LAI_MAX": "1.5"})
    r = np.random.default_rng(n_lon)
    land = {"mixed": (r.uniform(size=(n_lat, n_lon)) < 0.5), "all_land": np.ones((n_lat, n_lon), bool), "no_land": np.zeros((n_lat, n_lon), bool)}[mask]
    land = land.astype(np.uint8)
    L = r.uniform(-0.2, 2.0, (S, K, n_lat, n_lon))              # below zero and above lai_max, on land and off it
    L[3, 1, 2, n_lon - 1] = np.nan
    L[8, 0, 4, 0] = np.inf
    dev, eco = _eco_on((n_lat, n_lon), land)
    pop = eco.pop
    pop.push_layers(L, init=True)
    pop.add_species_from_parent(8, 0.3)
    want = ref.split(L, 8, 0.3, 1.5)
    got, w, ww = pop.LAI_layers_SK, pop.species_weights, ref.weights(want, land == 1)
    dw = _wdev(w, ww)
    print(f"5x{n_lon} {mask}: weights deviation {dw:.3e} (bound {WEIGHT_BOUND(int(land.sum())):.3e})")
    assert np.array_equal(got, want, equal_nan=True) and np.array_equal(pop.total_LAI(), ref.total(want), equal_nan=True)
    assert dw <= WEIGHT_BOUND(int(land.sum())) and (mask != "no_land" or np.array_equal(w, np.full(S + 1, 1.0 / (S + 1))))
    pop.add_species_from_parent(-3, 0.9)                        # clipped to parent 0 and f = 0.5; the grown stack splits again
    want2 = ref.split(want, 0, 0.5, 1.5)
    assert np.array_equal(pop.LAI_layers_SK, want2, equal_nan=True) and pop.Ns == S + 2
    dev.close()


def test_f32_maps_store_the_events_lai_as_f32(gpu, monkeypatch):
    """QD_ECO_F32=1: the event's ECO_LAI is the f64 sum rounded once to f32, as the individuals' stack pass stores it; the stack and
    the weights do not change."""
    z = np.load(os.path.join(GOLD, "speciation_parent0_19x36.npz"))
    out = {}
    for f32 in ("0", "1"):
        _clean_env(monkeypatch, {**ref.env_of(z), "QD_ECO_F32": f32})
        dev, eco = _eco_on(z["land_mask"].shape, z["land_mask"])
        eco.pop.push_layers(z["hit1_pre_stack"], init=True)
        eco.pop.add_species_from_parent(int(z["hit1_parent"]), float(z["hit1_frac"]))
        out[f32] = (eco.pop.LAI_layers_SK.copy(), eco.pop.species_weights.copy(), eco.pop.total_LAI())
        dev.close()
    a, b = out["0"], out["1"]
    assert np.array_equal(a[0], b[0]) and np.array_equal(a[1], b[1])
    assert np.array_equal(b[2], a[2].astype(np.float32).astype(np.float64)) and not np.array_equal(b[2], a[2])


def test_refusals(gpu, monkeypatch):
    from qingdai_amd._lib import QdError
    import qingdai_amd as qa
    from qingdai_amd.device import Device
    _clean_env(monkeypatch, {"QD_ECO_NS": "64"})
    land = (np.random.default_rng(0).uniform(size=(5, 130)) < 0.5).astype(np.uint8)
    dev = Device(qa.SphericalGrid(5, 130))
    with pytest.raises(QdError, match="qd_eco_daily_configure has not been called"):
        dev.eco_daily_speciate(0, 0.02, 3)
    dev.close()
    dev, eco = _eco_on((5, 130), land)
    with pytest.raises(QdError, match="n_species \\+ 1 out of range"):
        eco.pop.add_species_from_parent(0, 0.02)
    assert eco.pop.Ns == 64
    dev.close()
    _clean_env(monkeypatch, {"QD_ECO_NS": "3"})
    dev, eco = _eco_on((5, 130), land)
    for frac in (0.0, -1.0, float("nan")):
        with pytest.raises(QdError, match="frac <= 0 splits nothing"):
            eco.pop.add_species_from_parent(0, frac)
    from qingdai_amd.ecology import IndividualPool, IndividualDaily
    monkeypatch.setenv("QD_ECO_INDIV_SAMPLE_FRAC", "0.2"); monkeypatch.setenv("QD_ECO_INDIV_PER_CELL", "4")
    pool = IndividualPool(eco.grid, land, eco)
    IndividualDaily(pool, eco.pop)
    with pytest.raises(QdError, match="qd_indiv_daily_configure is in force"):
        eco.pop.add_species_from_parent(0, 0.02)
    assert eco.pop.Ns == 3 and eco.pop.LAI_layers_SK.shape[0] == 3
    dev.close()


# ------------------------------------------------------------------ driver runs
class NeverHits(np.random.RandomState):
    draws = 0

    def rand(self, *a):
        self.draws += 1
        return 0.999


LANE_ENV = {"QD_ECO_NS": "3", "QD_ECO_COHORT_K": "2", "QD_ECO_LAI_GROWTH": "4e-8", "QD_ECO_SPREAD_ENABLE": "1", "QD_ECO_SPREAD_RATE": "0.1",
            "QD_ECO_SEED_ENERGY": "2e4", "QD_ECO_RAND_SEED": "2", "QD_ECO_LIGHT_UPDATE_EVERY_HOURS": "1", "QD_ECO_DAILY": "1",
            "QD_ECO_BANDS_COUPLE": "1", "QD_ECO_SPECIES_1_PEAKS": "520:35:0.7"}
SPEC_ENV = {**LANE_ENV, "QD_ECO_SPECIATION": "1", "QD_ECO_MUT_RATE": "1.0", "QD_ECO_MUT_EPS": "0.3", "QD_ECO_SPECIES_MAX": "5"}
DAY = 7000.0                            # 23.3 steps of 300 s: the firings fall on run-local steps 23 and 46


def _sim(monkeypatch, env, rng=None):
    import qingdai_amd as qa
    from qingdai_amd.driver import Simulation
    _clean_env(monkeypatch, env)
    nlat, nlon = 19, 36
    sim = Simulation(nlat, nlon, params=qa.QdParams(), use_ocean=False, quiet=True, individuals=False, speciation_rng=rng)
    sim.day_seconds = DAY
    sim.eco_daily.day_seconds = DAY
    r = np.random.default_rng(8)
    lat = np.deg2rad(sim.grid.lat_mesh)
    land = sim.land_mask == 1
    sim.gcm.h, sim.gcm.T_s = 8000.0 - 10500.0 * np.sin(lat) ** 2, 262.0 + 36.0 * np.cos(lat) ** 2
    sim.dev.set("S_SNOW", np.where(land & (np.abs(sim.grid.lat_mesh) > 55), 60.0, 0.0))
    sim.dev.set("W_LAND", np.where(land, 40.0 * r.random((nlat, nlon)), 0.0))
    S, K = sim.eco.pop.Ns, sim.eco.pop.K
    sim.eco.pop.push_layers(np.abs(r.normal(0.2, 0.15, (S, K, nlat, nlon))) * land, init=True)
    sim.eco.banded_alpha()                                      # the banded map exists from the start, as in the reference
    return sim


def _fields(sim, names=PROGNOSTIC + ECO_FIELDS):
    for k in names:
        sim.dev._host.pop(k, None)
    return {k: sim.dev.get(k).copy() for k in names}


def _same(a, b):
    return [k for k in a if not np.array_equal(a[k], b[k], equal_nan=True)]


def test_switch_on_without_a_hit_changes_nothing(gpu, monkeypatch, capsys):
    """(d) a generator that never hits: every field and every printed line equal the run with the switch off."""
    off = _sim(monkeypatch, {**LANE_ENV, "QD_ECO_DIAG": "1"})
    assert off.speciation is None
    capsys.readouterr()
    off.run_steps(25); off.run_steps(35)
    lines_off = capsys.readouterr().out
    rng = NeverHits(1)
    on = _sim(monkeypatch, {**SPEC_ENV, "QD_ECO_MUT_RATE": "0.5", "QD_ECO_DIAG": "1"}, rng=rng)
    assert on.speciation is not None and on.speciation.rng is rng
    capsys.readouterr()
    on.run_steps(25); on.run_steps(35)
    lines_on = capsys.readouterr().out
    assert lines_on == lines_off and lines_on.count("[Ecology] daily: LAI(min/mean/max)=") == 2
    assert rng.draws == 2 == on.speciation.n_done and on.speciation.n_events == 0 and on.eco.pop.Ns == 3
    assert _same(_fields(off), _fields(on)) == [] and np.array_equal(off.eco.pop.LAI_layers_SK, on.eco.pop.LAI_layers_SK)
    assert off.eco.pop.state() == on.eco.pop.state() and off.dev.eco_daily_firings() == on.dev.eco_daily_firings() == 2
    off.dev.close(); on.dev.close()


def _by_hand(sim, n):
    """n steps, every firing through the class seam BEFORE its step (the reference's order), the event behind it, the banded
    alpha refreshed on a hit, the step then run with the firing struck out of the lane's schedule."""
    from qingdai_amd.ecology import daily_counts
    lane = sim.eco_daily
    for _ in range(n):
        fire, _a = daily_counts(lane.accum_day, float(sim.dt), 1, lane.day_seconds)
        for _q in range(int(fire[0])):
            sim.dev.eco_daily_step(None)
            lane._fired(1)
            sim.dev.eco_daily_log()
            if sim.speciation.event(sim.eco) is not None:
                sim.eco.banded_alpha()
        lane.struck = int(fire[0])
        sim._run_lanes(1)


def test_hit_mid_chunk_equals_the_run_driven_firing_by_firing(gpu, monkeypatch):
    """(e) the hits of RandomState(5) fall on steps 23 and 46 of one 60-step call.  The step that holds the first hit already sees
    the new species: its ALBEDO and banded alpha differ from the run without speciation, and equal the run driven by hand."""
    chunked = _sim(monkeypatch, SPEC_ENV, rng=np.random.RandomState(5))
    manual = _sim(monkeypatch, SPEC_ENV, rng=np.random.RandomState(5))
    plain = _sim(monkeypatch, LANE_ENV)
    assert chunked.speciation_due(60) == 23 and chunked.speciation_due(23) is None and chunked.speciation_due(24) == 23
    chunked.run_steps(24); _by_hand(manual, 24); plain.run_steps(24)                          # up to and including the hit's step
    assert chunked.eco.pop.Ns == manual.eco.pop.Ns == 4 and plain.eco.pop.Ns == 3 and chunked.speciation.n_events == 1
    fc, fm, fp = _fields(chunked), _fields(manual), _fields(plain)
    assert _same(fc, fm) == [], _same(fc, fm)
    assert not np.array_equal(fc["ECO_ALPHA_BANDED"], fp["ECO_ALPHA_BANDED"], equal_nan=True)
    assert not np.array_equal(fc["ALBEDO"], fp["ALBEDO"])      # the split came BEFORE the rest of the step
    for k in ("ECO_AGE", "ECO_SEEDBANK", "ECO_EDAY", "ECO_GATE"):
        assert np.array_equal(fc[k], fp[k]), k                 # the event leaves them alone
    chunked.run_steps(36); _by_hand(manual, 36)
    assert chunked.eco.pop.Ns == manual.eco.pop.Ns == 5 and chunked.speciation.n_events == 2 == manual.speciation.n_events
    fc, fm = _fields(chunked), _fields(manual)
    assert _same(fc, fm) == [], _same(fc, fm)
    assert np.array_equal(chunked.eco.pop.LAI_layers_SK, manual.eco.pop.LAI_layers_SK) and chunked.eco.pop.LAI_layers_SK.shape[0] == 5
    assert np.array_equal(chunked.eco.pop.species_weights, manual.eco.pop.species_weights)
    assert [g.identity for g in chunked.eco.genes_list] == [g.identity for g in manual.eco.genes_list]
    assert chunked.eco.genes_list[3].identity.endswith("_mut") and chunked.eco_daily.species_modes == manual.eco_daily.species_modes
    assert chunked.dev.eco_daily_firings() == manual.dev.eco_daily_firings() == 2 and chunked.eco.pop.state() == manual.eco.pop.state()
    for s in (chunked, manual, plain):
        s.dev.close()


def test_after_an_event_diversity_autosave_resume_and_genes_export(gpu, monkeypatch, tmp_path, capsys):
    """(f) one event, then: diversity() has Ns + 1 species; genes_day_*.json has Ns + 1 entries, one file per firing; an autosave at
    QD_ECO_PERSIST=2 read by a fresh start gives the same state bit for bit, and the next firing on both stays equal."""
    env = {**SPEC_ENV, "QD_ECO_PERSIST": "2", "QD_ECO_GENES_EXPORT": "1", "QD_OUTPUT_DIR": str(tmp_path / "out"), "QD_ECO_DIAG": "1",
           "QD_ECO_SPECIES_MAX": "4", "QD_ECO_BANDS_COUPLE": "0"}
    sim = _sim(monkeypatch, env, rng=np.random.RandomState(5))
    capsys.readouterr()
    sim.run_steps(50)                                           # firings on steps 23 (the event) and 46 (species_max reached)
    out = capsys.readouterr().out
    pop = sim.eco.pop
    assert pop.Ns == 4 and "new species idx=3; Ns=4" in out and "[Ecology] mutation skipped: species_max=4 reached." in out
    files = sorted(glob.glob(str(tmp_path / "out" / "genes_day_*.json")))
    assert out.count("[Ecology] Genes exported:") == 2 and len(files) >= 1
    t23, t46 = 23 * 300.0, 46 * 300.0
    days = [(t23 - ((24 * 300.0) - DAY)) / DAY, (t46 - ((47 * 300.0) - 2 * DAY)) / DAY]
    assert [os.path.basename(f) for f in files] == sorted({f"genes_day_{d:05.1f}.json" for d in days})
    with open(files[-1], encoding="utf-8") as f:
        doc = json.load(f)
    assert len(doc["genes"]) == 4 and doc["genes"][3]["identity"].endswith("_mut") and len([g["weight"] for g in doc["genes"]]) == 4
    assert doc["source"] == "PyGCM.EcologyAdapter.export_genes"
    alpha, bc, L_s, summary = pop.diversity()
    assert L_s.shape[0] == 4 and np.array_equal(L_s, np.sum(np.maximum(pop.LAI_layers_SK, 0.0), axis=1))
    assert sim.save_ecology(str(tmp_path / "data"), 1.5) is not None
    with open(tmp_path / "data" / "genes.json", encoding="utf-8") as f:
        saved = json.load(f)
    assert len(saved["genes"]) == 4 and len(saved["species_weights"]) == 4
    fresh = _sim(monkeypatch, env, rng=np.random.RandomState(6))
    assert fresh.eco.pop.Ns == 3 and fresh.load_ecology(str(tmp_path / "data")) is True
    a, b = pop, fresh.eco.pop
    assert b.Ns == 4 and fresh.eco_daily.params.n_species == 4 and fresh.eco_daily.species_modes == sim.eco_daily.species_modes
    assert np.array_equal(a.LAI_layers_SK, b.LAI_layers_SK) and np.array_equal(a.species_weights, b.species_weights)
    assert np.array_equal(a._species_R_leaf.astype(np.float32), b._species_R_leaf.astype(np.float32)) and fresh.eco_daily.accum_day == sim.eco_daily.accum_day
    names = ("ECO_LAI", "ECO_EDAY", "ECO_AGE", "ECO_SEEDBANK")
    assert _same(_fields(sim, names), _fields(fresh, names)) == []
    assert [g.identity for g in fresh.eco.genes_list] == [g.identity for g in sim.eco.genes_list]
    soil = np.random.default_rng(4).uniform(0.0, 0.9, a.shape)
    a.step_daily(soil); b.step_daily(soil)                      # germination by the restored weights, spread by the restored modes
    assert np.array_equal(a.LAI_layers_SK, b.LAI_layers_SK) and _same(_fields(sim, names), _fields(fresh, names)) == []
    sim.dev.close(); fresh.dev.close()
