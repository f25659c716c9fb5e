"""GPU (-m gpu): the three span lanes -- river routing (bit7), the daily phytoplankton step (bit8), the daily vegetation step (bit9) --
together in the configuration the reference driver runs by default: ocean, ecology with individuals, tracers, routing, and both
daily switches on, 37 x 72, the three clocks shortened so that one short span holds several firings of every lane and the
firings coincide in every combination.

a. Partition invariance, bitwise: one span, one-step spans, a partition cut around firing steps and that partition shifted
   by one step leave identical state and logs (README / DESIGN claim bit-identity for lazy diagnostics, the hoisted
   precipitation block, the merged final launch and the tail lists).  Also without individuals, with QD_ECO_F32=1, and through
   Device.step_n without the hydrology commit (where only the ecology flag keeps the lazily stored GLACIER fresh for bit9).
b. Each lane's footprint with the others on: routing feeds nothing back, an uncoupled phytoplankton lane touches nothing but
   its own state, an idle lane equals an absent one.
c. Against the CPU composition of tests/all_on_ref.py.

Tolerance of (c).  Deviations are max |a - b| / max |b| per array (util.relerr).  The single-lane loop tests hold 1e-9 against the
same oracles (test_gpu_ecology.py, test_gpu_phyto_daily.py): that is the starting bound per field.  MEASURED holds the largest
deviation per field on the MI355X; the bound in force is min(1e-9, 10 x measured) -- the factor ten covers reduction-order
differences between boxes (the convention of test_gpu_eco_daily.py).  The routing closure error is a cancellation residue and is
held relative to the event's mass input, as test_gpu_routing.py holds it."""
import os

import numpy as np
import pytest

from test_gpu_eco_daily import PROGNOSTIC
from test_gpu_routing import synthetic_network
from util import relerr

pytestmark = pytest.mark.gpu

NLAT, NLON, DT = 37, 72, 300.0
ROUTE_STEPS, PHYTO_DAY_STEPS, ECO_DAY_STEPS = 3, 4.5, 3.5         # the three clocks in steps, set independently
FIELDS = PROGNOSTIC + ("UO", "VO", "ETA", "SST", "ECO_LAI", "ECO_EDAY", "ECO_ALPHA", "ECO_F", "WATER_ALPHA", "KD490", "PHYTO_N")
PHYTO_OWN = ("WATER_ALPHA", "KD490", "PHYTO_N", "tracers", "log_phyto")
ROUTE_OWN = ("route_flow", "route_buffer", "route_lakes", "log_route")
ENV = {"QD_ECO_NS": "4", "QD_ECO_COHORT_K": "2", "QD_ECO_LAI_GROWTH": "4e-8", "QD_ECO_SPREAD_ENABLE": "1", "QD_ECO_SPREAD_RATE": "0.1",
       "QD_ECO_SEED_ENERGY": "2e4", "QD_ECO_RAND_SEED": "2", "QD_ECO_LIGHT_UPDATE_EVERY_HOURS": "1", "QD_ECO_DIAG": "0",
       "QD_ECO_INDIV_SAMPLE_FRAC": "0.05", "QD_ECO_INDIV_PER_CELL": "7", "QD_ECO_INDIV_SUBSTEPS_PER_DAY": "120",
       "QD_PHYTO_ENABLE": "1", "QD_PHYTO_NSPECIES": "4", "QD_PHYTO_DIAG": "0"}
START = 1e-9
# largest deviation from the CPU composition per field, MI355X, 24 steps (test_all_on_vs_cpu_composition prints them)
MEASURED = {"U": 5.8e-16, "V": 3.1e-14, "H": 2.5e-16, "TS": 1.5e-15, "Q": 1.1e-13, "CLOUD": 1.1e-12, "HICE": 0.0, "W_LAND": 1.8e-16, "S_SNOW": 3.7e-15,
            "ALBEDO": 3.6e-13, "UO": 7.9e-14, "VO": 9.7e-14, "ETA": 3.8e-15, "SST": 7.9e-16, "ECO_LAI": 1.6e-16, "ECO_EDAY": 1.9e-16, "ECO_ALPHA": 2.0e-16,
            "ECO_F": 1.5e-16, "tracers": 5.3e-16, "layers": 1.6e-16, "WATER_ALPHA": 2.1e-16, "KD490": 3.4e-16, "PHYTO_N": 1.6e-16, "age": 0.0,
            "bank": 1.8e-16, "indiv_E_day": 2.0e-16, "indiv_stress": 0.0, "route_flow": 1.6e-17, "route_buffer": 0.0, "route_lakes": 1.3e-15,
            "log_route_ocean_inflow": 2.0e-16, "log_route_closure_over_input": 2.3e-16, "log_phyto": 2.2e-16, "log_eco": 2.6e-16}


def bound(field):
    return START if MEASURED is None else min(START, 10 * MEASURED[field])


def schedules(n, route_steps=ROUTE_STEPS, phyto_day=PHYTO_DAY_STEPS, eco_day=ECO_DAY_STEPS):
    """The three lanes' firing steps over n steps from t = 0, derived on the host with the host clocks themselves."""
    from qingdai_amd.ecology import daily_counts
    from qingdai_amd.phyto import daily_schedule
    from qingdai_amd.routing import RiverRouting
    r = object.__new__(RiverRouting)
    r.dt_hydro_seconds, r.t_accum, r._steps = route_steps * DT, 0.0, 0
    route = (r.schedule(DT, n) != 0.0).astype(int)
    phyto = daily_schedule(0.0, 0.0, DT, n, phyto_day * DT)[0].astype(int)
    eco = daily_counts(0.0, DT, n, eco_day * DT)[0].astype(int)
    return route, phyto, eco


def assert_schedules_overlap(n):
    route, phyto, eco = schedules(n)
    r, p, e = route > 0, phyto > 0, eco > 0
    assert (r & p & e).any(), "no step fires all three lanes"
    assert (r & p & ~e).any() and (r & e & ~p).any() and (p & e & ~r).any(), "a pair of lanes never fires alone together"
    assert (r[:-1] & e[1:]).any(), "no routing event step is directly followed by a vegetation firing step"
    assert r.sum() >= 2 and p.sum() >= 2 and e.sum() >= 2
    return route, phyto, eco


def initial_state(sim):
    r = np.random.default_rng(8)
    lat = np.deg2rad(sim.grid.lat_mesh)
    land = sim.land_mask == 1
    S = sim.phyto.S
    out = {"h": 8000.0 - 10500.0 * np.sin(lat) ** 2, "T_s": 262.0 + 36.0 * np.cos(lat) ** 2,
           "S_snow": np.where(land & (np.abs(sim.grid.lat_mesh) > 55), 60.0, 0.0), "W_land": np.where(land, 40.0 * r.random((NLAT, NLON)), 0.0)}
    if sim.eco is not None:
        Ns, K = sim.eco.pop.Ns, sim.eco.pop.K
        out["layers"] = np.abs(r.normal(0.2, 0.15, (Ns, K, NLAT, NLON))) * land
        out["bank"] = r.uniform(0.0, 2.0, (NLAT, NLON)) * land
    out["C"] = np.abs(r.lognormal(np.log(0.3), 0.5, (S, NLAT, NLON))) * ~land
    out["N"] = np.where(~land, r.uniform(0.2, 2.0, (NLAT, NLON)), 0.0)
    return out


def all_on(monkeypatch, env=None, *, routing=True, phyto_daily=True, eco_daily=True, individuals=True, ecology=True,
           route_steps=ROUTE_STEPS, phyto_idle=False, eco_day=ECO_DAY_STEPS):
    """The all-on Simulation at 37 x 72 with shortened clocks and a seeded state -> (sim, the drained logs, the initial state)."""
    import qingdai_amd as qa
    from qingdai_amd.driver import Simulation
    from qingdai_amd.routing import RiverRouting
    for k in [k for k in os.environ if k.startswith(("QD_ECO_", "QD_PHYTO_"))]:
        monkeypatch.delenv(k)
    for k, v in {**ENV, "QD_PHYTO_DAILY": "1" if phyto_daily else "0", "QD_ECO_DAILY": "1" if eco_daily else "0", **(env or {})}.items():
        monkeypatch.setenv(k, v)
    sim = Simulation(NLAT, NLON, params=qa.QdParams(), use_ocean=True, quiet=True, ecology=ecology, individuals=individuals)
    assert sim.ocean is not None and sim.phyto is not None and sim.phyto_transport
    assert (sim.phyto_daily is not None) == phyto_daily and (sim.eco_daily is not None) == (eco_daily and ecology)
    assert (sim.indiv is not None) == (individuals and ecology)
    sim.network = None
    if routing:
        sim.network = synthetic_network(sim.land_mask, 4)
        sim.routing = RiverRouting.from_arrays(sim.grid, dt_hydro_hours=route_steps * DT / 3600.0, diag=False, dev=sim.dev, **sim.network)
    if sim.phyto_daily is not None:
        sim.phyto_daily.day_seconds = PHYTO_DAY_STEPS * DT
        if phyto_idle:
            sim.phyto_daily.phyto_next_time = 1.0e12
    if sim.eco_daily is not None:
        sim.eco_daily.day_seconds = eco_day * DT
        assert len(set(sim.eco_daily.species_modes)) == 2
    init = initial_state(sim)
    sim.gcm.h, sim.gcm.T_s = init["h"], init["T_s"]
    sim.dev.set("S_SNOW", init["S_snow"])
    sim.dev.set("W_LAND", init["W_land"])
    if sim.eco is not None:
        sim.eco.pop.push_layers(init["layers"], init=True)
        sim.eco.pop.seed_bank = init["bank"]
    sim.phyto.C_phyto_s = init["C"]
    if sim.phyto_daily is not None:
        sim.phyto_daily.N = init["N"]
    # _run_chunk drains the three device logs after every span: keep what it drains
    logs = {"log_phyto": [], "log_route": [], "log_eco": []}
    for key, name in (("log_phyto", "phyto_daily_log"), ("log_route", "route_events"), ("log_eco", "eco_daily_log")):
        def tap(orig=getattr(sim.dev, name), key=key):
            out = orig()
            logs[key] += [[float(x) for x in (r.values() if isinstance(r, dict) else r)] for r in out]
            return out
        setattr(sim.dev, name, tap)
    return sim, logs, init


def snapshot(sim, logs):
    dev = sim.dev
    for k in FIELDS + ("GLACIER",):
        dev._host.pop(k, None)
    out = {k: dev.get(k).copy() for k in FIELDS}
    out["tracers"] = sim.phyto.C_phyto_s.copy()
    if sim.eco is not None:
        out.update({"layers": sim.eco.pop.LAI_layers_SK.copy(), "age": sim.eco.pop.age_days, "bank": sim.eco.pop.seed_bank})
    if sim.indiv is not None:
        out["indiv_E_day"], out["indiv_stress"] = sim.indiv._pull()
    if getattr(sim, "routing", None) is not None:
        d = sim.routing.diagnostics()
        out.update({"route_flow": np.array(d["flow_accum_kgps"], copy=True), "route_buffer": sim.routing.buffer_kg().copy()})
        if d["lake_volume_kg"] is not None:
            out["route_lakes"] = np.array(d["lake_volume_kg"], copy=True)
    out.update({k: np.array(v, dtype=np.float64).reshape(len(v), -1) if v else np.zeros((0, 0)) for k, v in logs.items()})
    return out


def run(monkeypatch, cuts, env=None, **kw):
    sim, logs, _ = all_on(monkeypatch, env, **kw)
    for n in cuts:
        sim.run_steps(n)
    out = snapshot(sim, logs)
    sim.dev.close()
    return out


def assert_identical(a, b, what, skip=()):
    assert set(a) == set(b), (what, set(a) ^ set(b))
    bad = [k for k in a if k not in skip and not (a[k].shape == b[k].shape and np.array_equal(a[k], b[k], equal_nan=True))]
    assert not bad, f"{what}: not bit-identical: {bad}"


def cut_partition(n, route, phyto, eco):
    """Span boundaries just before and just after one firing step of every lane, the step that fires all three and the routing
    event that a vegetation firing follows directly: each of those steps is a span of its own, so a cut falls before it, the step
    is the first, the last and the only step of a span, and a cut falls after it.  -> (span lengths, the same shifted by one step)."""
    r, p, e = route > 0, phyto > 0, eco > 0
    picks = {int(np.nonzero(x)[0][1]) for x in (r, p, e)} | {int(np.nonzero(r & p & e)[0][0]), int(np.nonzero(r[:-1] & e[1:])[0][0])}
    out = []
    for shift in (0, 1):
        b = sorted({min(max(f + d + shift, 1), n - 1) for f in picks for d in (0, 1)})
        out.append([int(x) for x in np.diff([0] + b + [n])])
        assert sum(out[-1]) == n and min(out[-1]) >= 1
    return out


# ------------------------------------------------------------------------------------------------------------------------ (a)
@pytest.mark.parametrize("variant", ["default", "no_individuals", "f32_maps"])
def test_partition_invariance_is_bitwise(gpu, monkeypatch, variant):
    n = 48
    route, phyto, eco = assert_schedules_overlap(n)
    cut, shifted = cut_partition(n, route, phyto, eco)
    kw = {"individuals": variant != "no_individuals"}
    env = {"QD_ECO_F32": "1"} if variant == "f32_maps" else None
    whole = run(monkeypatch, [n], env, **kw)
    assert whole["log_route"].shape[0] == route.sum() and whole["log_phyto"].shape[0] == phyto.sum() and whole["log_eco"].shape[0] == eco.sum()
    assert list(whole["log_route"][:, 0]) == [float(s + 1) for s in np.nonzero(route)[0]]
    assert ("indiv_E_day" in whole) == kw["individuals"] and np.isfinite(whole["U"]).all()
    for name, cuts in (("one-step spans", [1] * n), ("cut at firing steps", cut), ("cut at firing steps, shifted", shifted)):
        assert_identical(whole, run(monkeypatch, cuts, env, **kw), f"{variant}: one span vs {name} {cuts}")


def test_partition_invariance_without_the_hydrology_commit(gpu, monkeypatch):
    """Device.step_n with the ocean, the physics, the ecology and bit9 but no hydrology commit and no transport: inside a span only
    the ecology flag makes the physics store GLACIER, which the daily vegetation step reads at the top of the next step."""
    n = 24
    _, _, eco = assert_schedules_overlap(n)
    outs = []
    for cuts in ([n], [1] * n, [5, 1, 1, 6, 11]):
        sim, logs, _ = all_on(monkeypatch, routing=False, phyto_daily=False)
        t = 0.0
        for k in cuts:
            times = t + DT * np.arange(k)
            sim.dev.step_n(sim.forcing.star_table(times), DT, with_ocean=True, with_physics=True, pass_albedo=False, with_hydrology=False,
                           ecology=True, eco_daily=sim.eco_daily)
            t += DT * k
            sim.dev.eco_daily_log()
        assert sim.dev.eco_daily_firings() == eco.sum()
        sim.dev._host.pop("GLACIER", None)
        assert sim.dev.get("GLACIER").any()                     # ice sheets exist: a stale mask would change the soil index
        outs.append(snapshot(sim, logs))
        sim.dev.close()
    assert_identical(outs[0], outs[1], "no commit: one span vs one-step spans")
    assert_identical(outs[0], outs[2], "no commit: one span vs cut spans")


# ------------------------------------------------------------------------------------------------------------------------ (b)
def test_each_lanes_footprint_with_the_others_on(gpu, monkeypatch):
    n = 24
    route, phyto, eco = assert_schedules_overlap(n)
    runs = {(r, p, e): run(monkeypatch, [n], routing=r, phyto_daily=p, eco_daily=e) for r in (0, 1) for p in (0, 1) for e in (0, 1)}
    # routing on vs off: no feedback, with both daily lanes firing and with either or neither
    for p in (0, 1):
        for e in (0, 1):
            on, off = runs[(1, p, e)], runs[(0, p, e)]
            assert on["log_route"].shape[0] == route.sum() and on["route_flow"].max() > 0.0
            assert_identical({k: v for k, v in on.items() if k not in ROUTE_OWN}, {k: v for k, v in off.items() if k not in ROUTE_OWN},
                             f"routing on vs off (phyto {p}, eco {e})")
    # the phytoplankton lane without its albedo coupling: only its own state differs from the lane absent
    uncoupled = run(monkeypatch, [n], {"QD_PHYTO_ALBEDO_COUPLE": "0"})
    assert uncoupled["log_phyto"].shape[0] == phyto.sum() and relerr(uncoupled["PHYTO_N"], runs[(1, 0, 1)]["PHYTO_N"]) > 1e-3
    assert_identical(uncoupled, runs[(1, 0, 1)], "QD_PHYTO_ALBEDO_COUPLE=0 vs the phytoplankton lane off", skip=PHYTO_OWN)
    # a lane whose clock crosses no boundary in the span equals that lane absent
    idle_route = run(monkeypatch, [n], route_steps=1000)
    assert idle_route["log_route"].size == 0 and idle_route["route_buffer"].max() > 0.0
    assert_identical({k: v for k, v in idle_route.items() if k not in ROUTE_OWN}, {k: v for k, v in runs[(0, 1, 1)].items() if k not in ROUTE_OWN},
                     "idle routing vs no routing")
    idle_phyto = run(monkeypatch, [n], phyto_idle=True)
    assert idle_phyto["log_phyto"].size == 0
    assert_identical(idle_phyto, runs[(1, 0, 1)], "idle phytoplankton lane vs absent", skip=("WATER_ALPHA", "KD490", "PHYTO_N"))
    idle_eco = run(monkeypatch, [n], eco_day=1000)
    assert idle_eco["log_eco"].size == 0
    assert_identical(idle_eco, runs[(1, 1, 0)], "idle vegetation lane vs absent")
    # not vacuous: every lane moved its state, and both albedo blends acted
    full, no_phyto, no_eco_lane = runs[(1, 1, 1)], runs[(1, 0, 1)], runs[(1, 1, 0)]
    assert relerr(full["layers"], no_eco_lane["layers"]) > 1e-3 and relerr(full["tracers"], no_phyto["tracers"]) > 1e-3
    import qingdai_amd as qa
    from qingdai_amd.topography import create_land_sea_mask
    land = create_land_sea_mask(qa.SphericalGrid(NLAT, NLON)) == 1
    open_ocean = ~land & (full["HICE"] == 0.0) & (no_phyto["HICE"] == 0.0)
    assert open_ocean.any() and (full["ALBEDO"][open_ocean] != no_phyto["ALBEDO"][open_ocean]).any()
    no_ecology = run(monkeypatch, [n], ecology=False, eco_daily=False)
    bare = land & (full["S_SNOW"] == 0.0) & (no_ecology["S_SNOW"] == 0.0)
    assert bare.any() and (full["ALBEDO"][bare] != no_ecology["ALBEDO"][bare]).any()


# ------------------------------------------------------------------------------------------------------------------------ (c)
def nan_relerr(a, b):
    a, b = np.asarray(a, dtype=float), np.asarray(b, dtype=float)
    assert a.shape == b.shape and np.array_equal(np.isnan(a), np.isnan(b))
    if not np.isfinite(b).any():
        return 0.0
    return float(np.nanmax(np.abs(a - b))) / max(float(np.nanmax(np.abs(b))), 1e-300)


def test_all_on_vs_cpu_composition(gpu, monkeypatch):
    from all_on_ref import AllOnTwin
    n = 24
    route, phyto, eco = assert_schedules_overlap(n)
    sim, logs, init = all_on(monkeypatch)
    env = {k: v for k, v in os.environ.items() if k.startswith("QD_ECO_")}
    twin = AllOnTwin(sim, init, env, network=sim.network, dt_hydro_seconds=ROUTE_STEPS * DT, phyto_fire=phyto, eco_fire=eco)
    sim.run_steps(7)                                            # two spans, the second one starting inside every lane's day
    sim.run_steps(n - 7)
    got = snapshot(sim, logs)
    for _ in range(n):
        twin.step(DT)
    want = twin.fields()
    land = sim.land_mask == 1
    got["ECO_F"] = np.where(land, got["ECO_F"], np.nan)
    errs = {k: nan_relerr(got[k], want[k]) for k in want}
    # the logs: steps and firing counts exactly, values to tolerance
    lr, lp, le = got["log_route"], got["log_phyto"], got["log_eco"]
    assert [int(x) for x in lr[:, 0]] == [e["step"] for e in twin.seq.events] == [int(s) + 1 for s in np.nonzero(route)[0]]
    assert list(lr[:, 1]) == [e["event_dt"] for e in twin.seq.events]
    assert list(lp[:, 0]) == [r[0] for r in twin.phyto_log] and len(lp) == phyto.sum()
    assert list(le[:, 0]) == [r[0] for r in twin.eco_log] and len(le) == eco.sum() == sim.dev.eco_daily_firings()
    errs["log_route_ocean_inflow"] = relerr(lr[:, 2], [e["ocean_inflow_kgps"] for e in twin.seq.events])
    errs["log_route_closure_over_input"] = max(abs(g - e["mass_closure_error_kg"]) / max(abs(e["mass_input_kg"]), 1e-300)
                                               for g, e in zip(lr[:, 3], twin.seq.events))
    errs["log_phyto"] = max(relerr(lp[:, c], np.array(twin.phyto_log)[:, c]) for c in (1, 2, 3))
    errs["log_eco"] = max(relerr(le[:, c], np.array(twin.eco_log)[:, c]) for c in (1, 2, 3))
    print("MEASURED = {" + ", ".join(f'"{k}": {e:.1e}' for k, e in errs.items()) + "}")
    if MEASURED is not None:
        assert set(MEASURED) == set(errs), set(MEASURED) ^ set(errs)
    over = {k: (e, bound(k)) for k, e in errs.items() if not e <= bound(k)}
    assert not over, over
    # not vacuous: every lane moved its state by more than 1e-3 relative
    assert relerr(want["layers"], init["layers"]) > 1e-3 and relerr(want["tracers"], init["C"]) > 1e-3 and relerr(want["PHYTO_N"], init["N"]) > 1e-3
    assert len(twin.seq.events) >= 2 and want["route_flow"].max() > 0.0 and twin.drv.indiv.n_fired >= 2
    assert twin.drv.glacier.any() and (want["age"] > 0).any() and relerr(want["bank"], init["bank"]) > 1e-3
    sim.dev.close()
