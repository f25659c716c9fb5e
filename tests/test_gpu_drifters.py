"""GPU (-m gpu): the drifter lane (csrc/qd_drift.hip, qingdai_amd/drifters.py).

The step is restated in NumPy (drifters.advance_reference), so everything here is bitwise (NaN equals NaN, the sign of a zero counts):
  1 the kernel alone through the class seam against the restatement, at the wave and block tails and on placed particles;
  2 one span against one-step spans against the class seam, and against the restatement on the planes Device.get returns;
  3 no effect on the model and on the other lanes; one launch per step when on, none and no directory when off;
  4 a lazily stored diagnostic as the sampled plane inside a long span;
  5 the refusals;
  6 driver.main, with and without the log-room cut;
  7 a run stopped inside a window and resumed (QD_CHECKPOINT=1) against the uncut run."""
import os
import re

import numpy as np
import pytest

from test_gpu_budget_diag import make, fetch, DT

pytestmark = pytest.mark.gpu


def same(a, b):
    """np.array_equal with NaN == NaN, and the same sign on every zero."""
    a, b = np.asarray(a, dtype=np.float64), np.asarray(b, dtype=np.float64)
    return a.shape == b.shape and np.array_equal(a, b, equal_nan=True) and np.array_equal(np.signbit(a) | np.isnan(a), np.signbit(b) | np.isnan(b))


# ---------------------------------------------------------------- 1: the kernel alone
SHAPES = [(19, 36), (37, 72), (5, 130)]
COUNTS = [(1, 1), (63, 63), (64, 64), (65, 65), (257, 257), (0, 65), (65, 0)]
STEP_DT = 86400.0


def velocity_planes(rng, grid, a):
    """U, V in m/s, built in cells per step: random displacements of about a cell, southward rows at the south pole and northward
    ones at the north pole (pole crossers), a row of 3.5 periods per step (multi-wrap), one node of 5 (n_lat - 1) rows per step
    (over range), one +inf and one NaN cell."""
    n_lat, n_lon = grid.n_lat, grid.n_lon
    P = n_lon - 1
    dc = rng.normal(0.0, 1.2, size=(n_lat, n_lon))
    dr = rng.normal(0.0, 0.6, size=(n_lat, n_lon))
    dr[:2, :], dr[-2:, :] = -0.7, 0.7
    mid = n_lat // 2
    dc[mid, :] = 3.5 * P
    dr[mid, 7] = 5.0 * (n_lat - 1)
    kr = a * np.deg2rad(grid.lat[1] - grid.lat[0]) / STEP_DT
    kc = a * np.deg2rad(360.0 / P) / STEP_DT
    U, V = dc * kc, dr * kr
    U[1, 20] = np.inf
    V[n_lat - 2, 25] = np.nan
    return U, V


def placed(grid):
    """(r, c) of the particles whose place is the test: the ends of both intervals, integer nodes, pole crossers, seam crossers,
    the multi-wrap row, the over-range node, the inf and NaN corners (one of them with weight zero)."""
    n_lat, n_lon = grid.n_lat, grid.n_lon
    rmax, P, mid = float(n_lat - 1), float(n_lon - 1), n_lat // 2
    top = np.nextafter(P, 0.0)
    pts = [(0.0, 0.0), (rmax, top), (0.0, top), (rmax, 0.0), (2.0, 3.0), (float(mid), 11.0), (rmax - 1, 30.0),      # ends, nodes
           (0.25, 5.5), (0.5, top), (rmax - 0.25, 9.25), (rmax - 0.5, 0.0),                                       # pole crossers
           (2.5, 0.1), (2.5, P - 0.1), (2.25, 0.3), (2.75, P - 0.3), (2.0, 0.05), (3.0, top),                     # seam, both ways
           (float(mid), 4.0), (mid + 0.25, 17.5), (mid - 0.25, P - 0.5),                                          # multi-wrap
           (float(mid), 7.0),                                                                                     # over range: dead
           (1.5, 20.5), (1.0, 19.0), (1.0, 21.0),                                                                 # +inf corner
           (n_lat - 2.5, 24.5), (float(n_lat - 2), 24.0), (float(n_lat - 2), 26.0)]                               # NaN, one of weight zero
    return np.array(pts, dtype=np.float64)


def island_mask(grid):
    land = np.zeros((grid.n_lat, grid.n_lon), dtype=np.uint8)
    land[:, 0] = land[:, -1] = 1
    land[2, 12] = 1                                               # a one-cell island
    return land


@pytest.mark.parametrize("shape", SHAPES)
def test_kernel_alone(gpu, shape):
    import qingdai_amd as qa
    from qingdai_amd import drifters as D
    from qingdai_amd._lib import QdError
    from qingdai_amd.device import Device
    grid = qa.SphericalGrid(*shape)
    dev = Device(grid)
    a = float(dev.params.a)
    rng = np.random.default_rng(shape[0] * 1000 + shape[1])
    planes = {}
    planes["U"], planes["V"] = velocity_planes(rng, grid, a)
    planes["UO"], planes["VO"] = velocity_planes(rng, grid, a)
    for name in ("TS", "H", "SST", "Q"):
        planes[name] = rng.normal(size=shape) * 10.0 ** rng.integers(-3, 4, size=shape)
    planes["H"][0, 0] = np.nan
    land = island_mask(grid)
    for name, x in planes.items():
        dev.upload_now(name, x)
    dev.upload_now("LAND_MASK", land)
    lat, sec = np.asarray(grid.lat, dtype=np.float64), D.sec_table(grid.lat)
    fixed = placed(grid)
    rmax, P = shape[0] - 1, shape[1] - 1
    fill = np.stack([rng.uniform(0, rmax, 300), rng.uniform(0, P, 300) * (1 - 1e-12)], axis=1)
    pool = np.concatenate([fixed, fill])
    samples = (["TS", "H", "Q"], ["SST"])
    seen = dict(dead=0, blocked=0, poles=0, wraps=0)
    for n_atm, n_ocn in COUNTS:
        seeds = [(pool[:n, 0].copy(), pool[:n, 1].copy()) for n in (n_atm, n_ocn)]
        cap = dev.drift_configure(seeds[0], seeds[1], samples[0], samples[1], sec)
        ns = (len(samples[0]) if n_atm else 0, len(samples[1]) if n_ocn else 0)
        width = D.record_width(n_atm, ns[0], n_ocn, ns[1])
        assert cap == D.log_capacity(width) == 16
        ref = [[seeds[q][0], seeds[q][1], np.zeros(len(seeds[q][0])), np.zeros(len(seeds[q][0]))] for q in (0, 1)]
        for k in range(3):
            dev.drift_advance(STEP_DT, record=(k != 1))
            before = [r[0].copy() for r in ref]
            ref[0] = list(D.advance_reference(*ref[0], planes["U"], planes["V"], None, lat, STEP_DT, a, False))
            ref[1] = list(D.advance_reference(*ref[1], planes["UO"], planes["VO"], land, lat, STEP_DT, a, True))
            atm, ocn = dev.drift_state()
            for q, got in ((0, atm), (1, ocn)):
                for j, what in enumerate(("r", "c", "status", "blocked")[:got.shape[0]]):
                    assert same(got[j], ref[q][j]), (shape, n_atm, n_ocn, k, POP[q], what, np.flatnonzero(got[j] != ref[q][j])[:5])
            if k == 0 and n_atm >= 63:
                near_pole = (before[0] < 0.6) | (before[0] > rmax - 0.6)
                seen["poles"] += int(np.count_nonzero(near_pole & (ref[0][2] == 0)))
                seen["wraps"] += int(np.count_nonzero((np.floor(before[0]) == shape[0] // 2) & (ref[0][2] == 0)))
        recs = dev.drift_log()
        assert recs.shape == (2, width) and len(dev.drift_log()) == 0
        parts = D.split_records(recs[1:], n_atm, ns[0], n_ocn, ns[1])
        for q, pop in enumerate(POP):                             # the last record is the last state, with the samples at it
            b = parts[pop][0]
            for j in range(3 + q):
                assert same(b[j], ref[q][j]), (shape, pop, j)
            for j, name in enumerate(samples[q][:ns[q]]):
                assert same(b[3 + q + j], D.sample_reference(planes[name], ref[q][0], ref[q][1])), (shape, pop, name)
        seen["dead"] += int(ref[0][2].sum() + ref[1][2].sum())
        seen["blocked"] += int(ref[1][3].sum())
        if n_atm >= 63:                                          # the placed particles did what they were placed for
            st = ref[0][2]
            assert st[20] == 1 and st[21] == 1 and st[24] == 1 and st[25] == 1        # over range, +inf, NaN, NaN of weight zero
            assert (ref[0][0] >= 0).all() and (ref[0][0] <= rmax).all() and (ref[0][1] >= 0).all() and (ref[0][1] < P).all()
    assert seen["dead"] > 8 and seen["blocked"] > 0 and seen["poles"] > 0 and seen["wraps"] > 0, seen
    # the class seam's own refusals, and the state put back
    atm, ocn = dev.drift_state()
    dev.drift_state_set(atm, ocn)
    assert all(same(x, y) for x, y in zip(dev.drift_state(), (atm, ocn)))
    bad = atm.copy()
    bad[1, 0] = float(P)
    with pytest.raises(QdError, match=r"qd_drift_state_set: a column coordinate is non-finite or outside \[0, n_lon - 1\)"):
        dev.drift_state_set(bad, ocn)
    assert all(same(x, y) for x, y in zip(dev.drift_state(), (atm, ocn)))
    dev.drift_configure(None, None, [], [], None)                # releases
    with pytest.raises(QdError, match="qd_drift_advance: not configured"):
        dev.drift_advance(STEP_DT)
    dev.close()


POP = ("atm", "ocn")


# ---------------------------------------------------------------- 2: a span equals single steps
def attach(sim, tmp_path, *, every=1, S=None, lane=True, n=(70, 70), **cfg):
    """A Drifters on the run's handle; lane=False: configured, but no participant of the spans (the class seam's twin)."""
    from qingdai_amd import drifters as D
    days = D.EVERY_DAYS if S is None else S * DT / sim.day_seconds
    sim.drifter_lines = []
    d = D.Drifters(sim, cfg=D.default_config(n_atm=n[0], n_ocn=n[1], every=every, every_days=days, **cfg), out=sim.drifter_lines.append,
                   output_dir=str(tmp_path))
    assert S is None or d.S == S
    sim.drifters = d if lane else None
    return d


@pytest.mark.parametrize("env", [None, {"QD_FUSED": "0"}], ids=["default", "unfused"])
def test_span_equals_single_steps(gpu, monkeypatch, tmp_path, env):
    from qingdai_amd import drifters as D
    got, states = [], []
    sim = make(monkeypatch, 19, 36, routing=False, env=env)
    d = attach(sim, tmp_path, every=2)
    assert d.n["atm"] == 70 and 0 < d.n["ocn"] < 70 and d.cap == 16
    first = d.state()
    sim.run_steps(6)
    got.append(d.window()[0])
    states.append(d.state())
    assert d.window()[2].tolist() == [0, 2, 4]
    sim.dev.close()
    # one-step spans, and beside them the restatement on what Device.get returns behind each span
    sim = make(monkeypatch, 19, 36, routing=False, env=env)
    d = attach(sim, tmp_path, every=2)
    a, lat, land = float(sim.dev.params.a), np.asarray(sim.grid.lat), np.asarray(sim.land_mask)
    ref = {p: [first[p][0], first[p][1], first[p][2], first[p][3] if p == "ocn" else np.zeros(d.n[p])] for p in POP}
    moved = 0
    for _ in range(6):
        sim.run_steps(1)
        f = fetch(sim.dev, ("U", "V", "UO", "VO"))
        before = ref["atm"][0].copy()
        ref["atm"] = list(D.advance_reference(*ref["atm"], f["U"], f["V"], None, lat, DT, a, False))
        ref["ocn"] = list(D.advance_reference(*ref["ocn"], f["UO"], f["VO"], land, lat, DT, a, True))
        moved += int(np.count_nonzero(before != ref["atm"][0]))
    got.append(d.window()[0])
    states.append(d.state())
    for p in POP:
        for j in range(states[1][p].shape[0]):
            assert same(states[1][p][j], ref[p][j]), (p, j)
    assert moved > 6 * 50                                        # liveness: the particles move on every step
    sim.dev.close()
    # the class seam behind spans that run without the lane
    sim = make(monkeypatch, 19, 36, routing=False, env=env)
    d = attach(sim, tmp_path, every=2, lane=False)
    for i in range(6):
        sim.run_steps(1)
        sim.dev.drift_advance(DT, record=(i % 2 == 0))
    got.append(sim.dev.drift_log())
    states.append(d.state())
    sim.dev.close()
    assert got[0].shape == (3, d.width)
    for k in (1, 2):
        assert same(got[k], got[0]), k
        assert all(same(states[k][p], states[0][p]) for p in POP), k
    parts = d.split(got[0])
    assert np.isfinite(got[0]).all() and not parts["atm"][:, 2].any() and not parts["ocn"][:, 2].any()
    assert not np.array_equal(parts["atm"][0, 1], parts["atm"][2, 1]) and not np.array_equal(parts["ocn"][0, :2], parts["ocn"][2, :2])
    assert not os.path.exists(tmp_path / "drifters") and sim.drifter_lines == []


# ---------------------------------------------------------------- 3: the model and the other lanes do not notice
def test_no_effect_on_the_model(gpu, monkeypatch, tmp_path):
    from qingdai_amd import ncio
    from test_gpu_history import attach as attach_history
    runs = {}
    for on in (False, True):
        out = tmp_path / ("on" if on else "off")
        sim = make(monkeypatch, 19, 36, fires={0: 3, 2: 1, 5: 3})
        assert sim.routing is not None and sim.budget is not None
        attach_history(sim, out, S=4)
        if on:
            attach(sim, out, S=3)
        sim.dev.timing(True)
        for n in (2, 4):
            sim.run_steps(n)
        sim.dev.sync()
        launches = sim.dev.timing_get("drifters")[1]
        sim.dev.timing(False)
        files = sorted(os.listdir(out / "history"))
        runs[on] = dict(files=files, arrays=[ncio.read_nc(str(out / "history" / f))[0] for f in files], sums=sim.dev.history_read(),
                        budget=list(sim.budget_lines), history=list(sim.history_lines), digest=sim.digest(), launches=launches,
                        drifters=sorted(os.listdir(out / "drifters")) if os.path.exists(out / "drifters") else None)
        sim.dev.close()
    off, on = runs[False], runs[True]
    assert off["launches"] == 0 and off["drifters"] is None      # at 0: no drifters scope in the timing tables, no directory
    assert on["launches"] == 6 and len(on["drifters"]) == 2      # exactly one launch per step; windows 0-2 and 3-5
    assert on["files"] == off["files"] and len(off["files"]) == 1
    for va, vb in zip(on["arrays"], off["arrays"]):
        assert va.keys() == vb.keys() and all(np.asarray(va[k]).tobytes() == np.asarray(vb[k]).tobytes() for k in va)
    assert on["sums"][1] == off["sums"][1] and on["sums"][0].tobytes() == off["sums"][0].tobytes()
    assert on["budget"] == off["budget"] and len(off["budget"]) > 0 and on["history"] == off["history"]
    assert on["digest"] == off["digest"] and len(off["digest"]) > 20


# ---------------------------------------------------------------- 4: a lazily stored diagnostic as the sampled plane
def test_lazy_sampled_plane(gpu, monkeypatch, tmp_path):
    """Device.step_n without the hydrology bit: inside a span only the last step stores OLR -- unless a reader comes with the span.
    The value a particle takes on a mid-span step is the one it takes when the span ends there."""
    flags = dict(with_ocean=True, with_physics=True, pass_albedo=False, with_hydrology=False)
    got = []
    for cuts in ([1, 1, 1, 1, 1], [5]):
        sim = make(monkeypatch, 19, 36, routing=False)
        d = attach(sim, tmp_path, sample_atm=["OLR", "TS"], sample_ocn=["EFLUX"])
        stars = sim.forcing.star_table(DT * np.arange(5))
        i = 0
        for n in cuts:
            sim.dev.step_n(stars[i:i + n], DT, drifters=d, **flags)
            d.span_deliver(DT)
            i += n
        got.append(d.window()[0])
        sim.dev.close()
    assert got[0].shape == (5, d.width) and same(got[0], got[1])
    olr = d.split(got[1])["atm"][:, 3]
    assert np.isfinite(olr).all() and (olr > 50.0).all() and all(not np.array_equal(olr[i], olr[i + 1]) for i in range(4))


# ---------------------------------------------------------------- 5: refusals
def test_refusals(gpu, monkeypatch, tmp_path):
    import qingdai_amd as qa
    from qingdai_amd import drifters as D
    from qingdai_amd._lib import QdError
    from qingdai_amd.bands import BandGroup
    from qingdai_amd.device import Device
    grid = qa.SphericalGrid(5, 6)
    dev = Device(grid)
    sec = D.sec_table(grid.lat)
    one = (np.array([1.0]), np.array([2.0]))
    with pytest.raises(QdError, match=r"qd_drift_configure: PRECIP cannot be sampled: the lane reads behind a step's last launch, and inside a "
                                      r"span the hoisted precipitation block has by then overwritten it with the next step's"):
        dev.drift_configure(one, None, ["PRECIP"], [], sec)
    with pytest.raises(QdError, match="qd_drift_configure: a sampled field is not an f64 plane"):
        dev.drift_configure(one, None, ["LAND_MASK"], [], sec)
    with pytest.raises(QdError, match="qd_drift_configure: at most 4 sampled planes per population"):
        dev.drift_configure(one, None, ["TS", "H", "Q", "U", "V"], [], sec)
    for r, c, what in ((-0.5, 1.0, r"a row coordinate is non-finite or outside \[0, n_lat - 1\]"), (4.5, 1.0, "a row coordinate"),
                       (np.nan, 1.0, "a row coordinate"), (1.0, 5.0, r"a column coordinate is non-finite or outside \[0, n_lon - 1\)"),
                       (1.0, -1e-9, "a column coordinate"), (1.0, np.inf, "a column coordinate")):
        with pytest.raises(QdError, match="qd_drift_configure: initial position: " + what):
            dev.drift_configure(None, (np.array([1.0, r]), np.array([1.0, c])), [], [], sec)
    with pytest.raises(QdError, match=r"qd_drift_configure: a population holds 0 to QD_DRIFT_MAX \(1048576\) particles"):
        dev.call("qd_drift_configure", (1 << 20) + 1, None, None, 0, None, None, 0, None, 0, None, sec, qa._lib.OUT)
    with pytest.raises(QdError, match=r"qd_drift_configure: a population holds 0 to QD_DRIFT_MAX"):
        dev.call("qd_drift_configure", 0, None, None, -1, None, None, 0, None, 0, None, sec, qa._lib.OUT)
    for call in (dev.drift_advance, dev.drift_log, dev.drift_reset, dev.drift_state, lambda: dev.drift_schedule([1, 1])):
        with pytest.raises(QdError, match="not configured"):     # none of the refused calls left a configuration
            call(*((DT,) if call == dev.drift_advance else ()))
    assert dev.drift_configure(one, one, ["TS"], ["SST"], sec) == 16       # the handle is as usable as before
    dev.drift_advance(DT, record=True)
    assert dev.drift_log().shape == (1, 4 + 5)
    dev.close()
    grp = BandGroup(qa.SphericalGrid(73, 144), 2)
    with pytest.raises(QdError, match=r"qd_drift_configure: the drifters need a whole-globe handle \(world == 1, n_rows == n_lat\); latitude "
                                      r"bands are not supported"):
        grp.devs[0].drift_configure(one, None, [], [], D.sec_table(np.linspace(-90, 90, 73)))
    grp.close()
    # spans: an ocn population without the ocean step, the wrong schedule length, more records than the log holds -- nothing runs
    sim = make(monkeypatch, 19, 36, routing=False)
    sec = D.sec_table(sim.grid.lat)
    cap = sim.dev.drift_configure(one, one, ["TS"], ["SST"], sec)
    flags = dict(with_physics=True, pass_albedo=False, with_hydrology=True)
    stars = sim.forcing.star_table(DT * np.arange(cap + 1))
    counters, state = sim.dev.counters(), sim.dev.drift_state()
    sim.dev.drift_schedule([1, 0])
    with pytest.raises(QdError, match=r"qd_step_n: the ocn drifters need the ocean step \(bit0\)"):
        sim.dev.step_n(stars[:2], DT, with_ocean=False, **flags)
    sim.dev.drift_schedule([1, 1, 1])
    with pytest.raises(QdError, match="a qd_drift_schedule must cover exactly the n steps of the span"):
        sim.dev.step_n(stars[:2], DT, with_ocean=True, **flags)
    sim.dev.drift_schedule(np.ones(cap + 1, dtype=np.int32))
    with pytest.raises(QdError, match="the span's drifter records would overflow the lane's log"):
        sim.dev.step_n(stars, DT, with_ocean=True, **flags)
    assert sim.dev.counters() == counters and len(sim.dev.drift_log()) == 0
    assert all(same(x, y) for x, y in zip(sim.dev.drift_state(), state))
    sim.dev.step_n(stars[:2], DT, with_ocean=True, **flags)      # the refused spans left no schedule behind: the lane sleeps
    assert sim.dev.counters()[0] == counters[0] + 2 and all(same(x, y) for x, y in zip(sim.dev.drift_state(), state))
    sim.dev.drift_schedule([0, 1])
    sim.dev.step_n(stars[:2], DT, with_ocean=True, **flags)
    assert sim.dev.drift_log().shape == (1, 4 + 5) and not same(sim.dev.drift_state()[0], state[0])
    sim.dev.close()
    # the host's refusals: the ocean that is off, a sample list that asks too much
    dry = make(monkeypatch, 19, 36, routing=False, ocean=False)
    with pytest.raises(ValueError, match="the ocn population needs the ocean, which is off in this run"):
        D.Drifters(dry, ocn=([0.0], [10.0]))
    with pytest.raises(ValueError, match="QD_DRIFT_SAMPLE_ATM: field 'SST' needs the ocean, which is off in this run"):
        D.Drifters(dry, cfg=D.default_config(sample_atm=["SST"]))
    d = D.Drifters(dry, cfg=D.default_config(n_atm=9, n_ocn=9), output_dir=str(tmp_path))      # no ocean: no ocn population
    assert d.n == {"atm": 9, "ocn": 0}
    dry.drifters = d
    dry.run_steps(2)
    assert d.window()[0].shape == (1, 9 * 5)
    dry.dev.close()


# ---------------------------------------------------------------- 6: the driver
def _set_env(monkeypatch, env):
    for k in [k for k in os.environ if k.startswith("QD_")]:
        monkeypatch.delenv(k)
    for k, v in env.items():
        monkeypatch.setenv(k, str(v))


def test_driver_main(gpu, tmp_path, monkeypatch, capsys):
    from qingdai_amd import driver, ncio
    env = {"QD_N_LAT": "19", "QD_N_LON": "36", "QD_SIM_DAYS": "0.125", "QD_ECO_ENABLE": "0", "QD_DYN_DIAG_PRINT": "0", "QD_USE_OCEAN": "1",
           "QD_HYDRO_ENABLE": "0", "QD_DRIFTERS": "1", "QD_DRIFT_EVERY_DAYS": "0.05", "QD_DRIFT_EVERY": "2", "QD_DRIFT_N_ATM": "100",
           "QD_DRIFT_N_OCN": "100"}
    day = 72000.0
    outs = {}
    for name, extra in (("on", {}), ("cut", {"QD_DRIFT_LOG_CAP": "2"})):
        _set_env(monkeypatch, {**env, **extra})
        d = tmp_path / name
        d.mkdir()
        monkeypatch.chdir(d)
        assert driver.main() == 0
        out = capsys.readouterr().out
        lines = [s for s in out.splitlines() if s.startswith("[Drifters]")]
        assert len(lines) == 3 and [int(re.search(r": (\d+) records", s).group(1)) for s in lines] == [6, 6, 3], out
        assert all(re.fullmatch(r"\[Drifters\] day \d+\.\d+–\d+\.\d+: \d+ records \| atm \d+/\d+ \| ocn \d+/\d+/\d+", s) for s in lines), lines
        files = sorted(os.listdir(d / "output" / "drifters"))
        assert len(files) == 3 and all(re.fullmatch(r"drifters_day_\d+\.\d+_\d+\.\d+\.nc", f) for f in files), files
        outs[name] = (lines, files, [ncio.read_nc(str(d / "output" / "drifters" / f))[0] for f in files])
    lines, files, arrays = outs["on"]
    n_ocn = None
    for f, v, (steps, complete) in zip(files, arrays, ((range(0, 12, 2), 1), (range(12, 24, 2), 1), (range(24, 30, 2), 0))):
        steps = list(steps)
        assert v["step"].tolist() == steps and v["time_seconds"].tolist() == [k * DT for k in steps], f
        assert (int(v["complete"]), int(v["sample_every"]), float(v["dt_seconds"])) == (complete, 2, DT)
        a, b = (float(x) for x in re.fullmatch(r"drifters_day_(.+)_(.+)\.nc", f).groups())
        assert abs(a - steps[0] * DT / day) <= 0.005 and abs(b - steps[-1] * DT / day) <= 0.005, f
        assert set(v) == {"time_seconds", "step", "atm_lat", "atm_lon", "atm_status", "atm_ts", "atm_h", "ocn_lat", "ocn_lon", "ocn_status",
                          "ocn_blocked", "ocn_sst", "dt_seconds", "sample_every", "complete"}
        n_ocn = v["ocn_lat"].shape[1]
        assert v["atm_lat"].shape == (len(steps), 100) and 0 < n_ocn < 100 and v["ocn_sst"].shape == (len(steps), n_ocn)
        assert (np.abs(v["atm_lat"]) <= 90.0).all() and (v["atm_lon"] >= 0.0).all() and (v["atm_lon"] < 360.0).all()
        assert not v["atm_status"].any() and not v["ocn_status"].any()
        assert (v["atm_ts"] > 200.0).all() and (v["atm_ts"] < 330.0).all() and (v["ocn_sst"] > 260.0).all() and (v["atm_h"] > 5000.0).all()
    assert not np.array_equal(arrays[0]["atm_lon"][0], arrays[2]["atm_lon"][-1])       # they drift
    # the log-room cut changes neither the lines nor a byte of a variable
    assert outs["cut"][0] == lines and outs["cut"][1] == files
    for va, vb in zip(arrays, outs["cut"][2]):
        assert va.keys() == vb.keys() and all(np.asarray(va[k]).tobytes() == np.asarray(vb[k]).tobytes() for k in va)
    # the same run without the switch: no directory, no line
    _set_env(monkeypatch, {k: v for k, v in env.items() if k != "QD_DRIFTERS"})
    off = tmp_path / "off"
    off.mkdir()
    monkeypatch.chdir(off)
    assert driver.main() == 0
    assert "[Drifters]" not in capsys.readouterr().out and not os.path.exists(off / "output" / "drifters")


# ---------------------------------------------------------------- 7: stopped inside a window and resumed
def test_resumed_run_writes_the_uncut_runs_files(gpu, tmp_path, monkeypatch, capsys):
    from qingdai_amd import driver, ncio

    def env(data, days, **extra):
        e = {"QD_N_LAT": "19", "QD_N_LON": "36", "QD_DT_SECONDS": "300", "QD_SIM_DAYS": str(days), "QD_DYN_DIAG_PRINT": "0", "QD_ECO_ENABLE": "0",
             "QD_HYDRO_ENABLE": "0", "QD_USE_OCEAN": "1", "QD_DATA_DIR": str(tmp_path / data), "QD_OUTPUT_DIR": str(tmp_path / ("out_" + data)),
             "QD_DRIFTERS": "1", "QD_DRIFT_EVERY_DAYS": "0.05", "QD_DRIFT_EVERY": "3", "QD_DRIFT_N_ATM": "60", "QD_DRIFT_N_OCN": "60",
             "QD_DRIFT_SAMPLE_ATM": "TS,OLR", "QD_CHECKPOINT": "1"}
        e.update(extra)
        return e
    monkeypatch.chdir(tmp_path)
    _set_env(monkeypatch, env("whole", 0.125))                   # 30 steps: windows 0-11 and 12-23, 24-29 stays open
    assert driver.main() == 0
    whole = capsys.readouterr().out
    assert whole.count("[Drifters] day ") == 2 and " 30 steps" in whole and "[Checkpoint] (final) wrote" in whole
    _set_env(monkeypatch, env("cut", 0.0625))                    # 15 steps: stopped inside the window 12-23
    assert driver.main() == 0
    first = capsys.readouterr().out
    assert first.count("[Drifters] day ") == 1 and " 15 steps" in first and "[Checkpoint] loaded" not in first
    assert driver.main() == 0
    second = capsys.readouterr().out
    assert "[Checkpoint] loaded" in second and "step 15" in second and second.count("[Drifters] day ") == 1      # each file written once
    files = lambda d: sorted(os.listdir(tmp_path / ("out_" + d) / "drifters"))
    assert files("cut") == files("whole") and len(files("whole")) == 2
    for name in files("whole"):
        va, vb = (ncio.read_nc(str(tmp_path / ("out_" + d) / "drifters" / name))[0] for d in ("whole", "cut"))
        assert va.keys() == vb.keys() and all(np.asarray(va[k]).tobytes() == np.asarray(vb[k]).tobytes() for k in va), name
        assert int(va["complete"]) == 1 and len(va["step"]) == 4
    wa, wb = (ncio.read_nc(str(tmp_path / d / "checkpoint.nc")) for d in ("whole", "cut"))
    assert wa[1]["run_digest"] == wb[1]["run_digest"]
    for k in ("drift_records", "drift_times", "drift_steps", "drift_clock", "drift_atm", "drift_ocn"):     # the open window and the particles
        assert np.asarray(wa[0][k]).tobytes() == np.asarray(wb[0][k]).tobytes(), k
    assert wa[0]["drift_clock"].tolist() == [30.0, 2.0] and wa[0]["drift_steps"].tolist() == [24.0, 27.0]
    assert wa[0]["drift_atm"].shape == (3, 60) and wa[0]["drift_ocn"].shape[0] == 4 and wa[0]["drift_atm"].dtype == np.float64
    key = re.search(r"drifters=([^;]+)", wa[1]["subsystems"]).group(1)
    assert re.fullmatch(r"atm=60:TS,OLR\|ocn=\d+:SST\|every=3", key), key
    # another drifter configuration, or none in the file: refused with the subsystem wording
    _set_env(monkeypatch, env("cut", 0.0625, QD_DRIFT_EVERY="2"))
    assert driver.main() == 2
    assert f"the subsystem set differs: the drifters lane is '{key}' in the file and '{key[:-1]}2' in this run" in capsys.readouterr().out
    _set_env(monkeypatch, env("plain", 0.0625, QD_DRIFTERS="0"))
    assert driver.main() == 0
    capsys.readouterr()
    _set_env(monkeypatch, env("plain", 0.0625))                  # a checkpoint taken without the lane, a run with it: strict mode refuses
    assert driver.main() == 2
    assert f"the subsystem set differs: the drifters lane is '-' in the file and '{key}' in this run" in capsys.readouterr().out
