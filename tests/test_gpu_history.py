"""GPU (-m gpu): the time-mean history lane (csrc/qd_history.hip, qingdai_amd/history.py).

The accumulation is `sum = sum + x` per cell in step order, so everything here but the oracle comparison is bitwise:
  1 the kernel alone through the class seam (qd_history_sample) at ragged shapes against NumPy's sequential adds;
  2 a 7-step span with the lane against 7 one-step spans without it, whose fields are downloaded after every step -- the
    definition of a sample -- and against a 7-step span without the lane (no perturbation);
  3 the mean over 4 steps against the mean of DriverOracle's fields after each of its 4 steps, at the bounds
    test_gpu_parity.py::test_driver_loop_vs_oracle holds for the end state (a mean of values within a bound is within it);
  4 chunking, the other lanes, windows and the file; a refused span;
  5 driver.main."""
import ctypes
import os
import re

import numpy as np
import pytest

from test_gpu_budget_diag import make, fetch, RESTART, DT

pytestmark = pytest.mark.gpu

STATE = RESTART + ("PRECIP", "ALBEDO", "EFLUX", "PCOND", "OLR", "ISR", "RUNOFF", "QNET", "C_SNOW")


def same(a, b):
    """np.array_equal with NaN == NaN, and the same sign on every zero."""
    a, b = np.asarray(a), np.asarray(b)
    return np.array_equal(a, b, equal_nan=True) and np.array_equal(np.signbit(a) | np.isnan(a), np.signbit(b) | np.isnan(b))


# ---------------------------------------------------------------- 1: the kernel alone
POOL = ("TS", "H", "U", "V", "Q", "CLOUD", "HICE", "ALBEDO", "OLR", "W_LAND", "UO", "VO", "PRECIP", "ETA")
PAIRS = (("U", "V"), ("UO", "VO"), ("TS", "H"))


def entry_list(n):
    """n entries: planes of the pool in turn, every fourth entry a pair."""
    out = []
    for k in range(n):
        out.append((1,) + PAIRS[(k // 4) % len(PAIRS)] if k % 4 == 3 else (0, POOL[k % len(POOL)], None))
    return out


def field_values(r, shape, round_):
    """Finite random planes with a few special cells: NaN, +inf, -inf, -0.0; the pairs get one (0, 0) cell and one with a huge
    component, whose square overflows."""
    n = shape[0] * shape[1]
    v = {}
    for j, name in enumerate(POOL):
        x = r.normal(size=n) * 10.0 ** r.integers(-3, 4)
        cells = np.random.default_rng(j).choice(n, size=4, replace=False)      # the same cells in every round
        x[cells[0]] = np.nan if round_ != 1 else 1.5          # round 1 leaves that cell finite: a NaN then comes from the sum alone
        x[cells[1]] = np.inf
        x[cells[2]] = -np.inf if round_ == 0 else np.inf      # -inf first, +inf later: inf - inf in the sum
        x[cells[3]] = -0.0
        v[name] = x.reshape(shape)
    for a, b in PAIRS:
        v[a].flat[n - 1], v[b].flat[n - 1] = 0.0, 0.0         # the last cell: the scalar tail of an odd grid
        v[a].flat[n // 2], v[b].flat[n // 2] = 1e200, 3.0
    return v


def host_value(entry, v):
    op, a, b = entry
    if op == 0:
        return v[a]
    with np.errstate(all="ignore"):
        return np.sqrt(v[a] * v[a] + v[b] * v[b])


@pytest.mark.parametrize("shape", [(5, 5), (7, 256), (9, 257), (10, 600)])
def test_kernel_alone(gpu, shape):
    import qingdai_amd as qa
    from qingdai_amd.device import Device
    dev = Device(qa.SphericalGrid(*shape))
    r = np.random.default_rng(shape[0] * 1000 + shape[1])
    for n in (1, 5, 32):
        entries = entry_list(n)
        dev.history_configure(entries)
        sums, count = dev.history_read()
        assert sums.shape == (n,) + shape and count == 0 and not sums.any()
        acc = np.zeros((n,) + shape)
        for round_ in range(3):
            v = field_values(r, shape, round_)
            for name, x in v.items():
                dev.upload_now(name, x)
            dev.history_sample()
            with np.errstate(all="ignore"):
                for k, e in enumerate(entries):
                    acc[k] = acc[k] + host_value(e, v)
        sums, count = dev.history_read()
        assert count == 3
        for k, e in enumerate(entries):
            assert same(sums[k], acc[k]), (shape, n, k, e)
        if n == 32:
            assert np.isnan(acc).any() and np.isinf(acc).any() and np.isfinite(acc).sum() > acc.size // 2
            pair = [k for k, e in enumerate(entries) if e[0] == 1][0]
            assert np.isinf(acc[pair].flat[shape[0] * shape[1] // 2]) and acc[pair].flat[-1] == 0.0
        dev.history_reset()
        sums, count = dev.history_read()
        assert count == 0 and not sums.any() and not np.signbit(sums).any()
    dev.history_configure([])                                # releases
    from qingdai_amd._lib import QdError
    with pytest.raises(QdError, match="not configured"):
        dev.history_sample()
    dev.close()


def test_refusals(gpu):
    import qingdai_amd as qa
    from qingdai_amd._lib import F, QdError
    from qingdai_amd.bands import BandGroup
    from qingdai_amd.device import Device
    dev = Device(qa.SphericalGrid(5, 6))
    with pytest.raises(QdError, match="at most 32 entries"):
        dev.history_configure(entry_list(33))
    ip = ctypes.POINTER(ctypes.c_int32)

    def raw(op, a, b):
        arr = [np.ascontiguousarray(x, dtype=np.int32) if x is not None else None for x in (op, a, b)]
        rc = dev.lib.qd_history_configure(dev.h, len(op), *[x.ctypes.data_as(ip) if x is not None else None for x in arr])
        return rc, (dev.lib.qd_last_error(dev.h) or b"").decode()
    rc, msg = raw([2], [F["TS"]], [-1])
    assert rc != 0 and "unknown op" in msg
    for bad in (F["LAND_MASK"], -1, len(POOL) + 1000):
        rc, msg = raw([0], [bad], [-1])
        assert rc != 0 and "field a is not an f64 plane" in msg, bad
    rc, msg = raw([1], [F["U"]], [F["ICE_MASK"]])
    assert rc != 0 and "field b is not an f64 plane" in msg
    rc, msg = raw([1], [F["U"]], None)
    assert rc != 0 and "op 1 needs a second field b" in msg
    rc, msg = raw([1], [F["PRECIP"]], [F["U"]])
    assert rc != 0 and "cannot pair PRECIP" in msg
    with pytest.raises(QdError, match="qd_history_read: not configured"):      # none of the refused calls left a configuration
        dev.history_read()
    with pytest.raises(QdError, match="qd_history_schedule: not configured"):
        dev.history_schedule([1, 1])
    dev.close()
    grp = BandGroup(qa.SphericalGrid(73, 144), 2)
    with pytest.raises(QdError, match=r"needs? a whole-globe handle \(world == 1, n_rows == n_lat\); latitude bands are not supported"):
        grp.devs[0].history_configure([(0, "TS", None)])
    grp.close()


# ---------------------------------------------------------------- 2: a span equals single steps
def attach(sim, tmp_path, *, k=1, S=None, fields=None, cls=None, lines=None):
    from qingdai_amd import history as hs
    days = hs.EVERY_DAYS if S is None else S * DT / sim.day_seconds
    cfg = {"enabled": True, "every_days": days, "sample_every": k, "fields": fields}
    sim.history_lines = [] if lines is None else lines
    sim.history = (cls or hs.History)(sim.dev, sim.grid, cfg, with_ocean=sim.ocean is not None, dt=DT, day=sim.day_seconds,
                                      out=sim.history_lines.append, output_dir=str(tmp_path))
    assert S is None or sim.history.S == S
    return sim.history


def sources(names):
    from qingdai_amd import history as hs
    return sorted({f for n in names for f in (hs.DERIVED[n] if n in hs.DERIVED else (n,))})


def entry_values(names, v):
    from qingdai_amd import history as hs
    return np.stack([host_value((1,) + hs.DERIVED[n] if n in hs.DERIVED else (0, n, None), v) for n in names])


def single_steps(sim, names, nsteps):
    """nsteps one-step spans without the lane -> the entries' values after every step [nsteps][n][n_lat][n_lon]."""
    assert getattr(sim, "history", None) is None
    out = []
    for _ in range(nsteps):
        sim.run_steps(1)
        out.append(entry_values(names, fetch(sim.dev, sources(names))))
    return np.stack(out)


def host_sums(values, flags):
    acc = np.zeros_like(values[0])
    with np.errstate(all="ignore"):
        for x, f in zip(values, flags):
            if f:
                acc = acc + x
    return acc


TWINS = {"19x36": (19, 36, True), "19x36_no_ocean": (19, 36, False), "37x72": (37, 72, True), "25x400": (25, 400, False)}
_twin_cache = {}


def twin_reference(monkeypatch, case):
    """Twin A (7 one-step spans, downloads after each) and the lane-free 7-step span's end state, once per case."""
    from qingdai_amd import history as hs
    if case not in _twin_cache:
        nlat, nlon, ocean = TWINS[case]
        a = make(monkeypatch, nlat, nlon, ocean=ocean, routing=False)
        names = hs.resolve_fields(None, ocean)
        values = single_steps(a, names, 7)
        a.dev.close()
        c = make(monkeypatch, nlat, nlon, ocean=ocean, routing=False)
        c.run_steps(7)
        state = fetch(c.dev, [k for k in STATE if ocean or k not in ("UO", "VO", "ETA", "SST", "QNET")])
        c.dev.close()
        values.setflags(write=False)
        _twin_cache[case] = (names, values, state)
    return _twin_cache[case]


@pytest.mark.parametrize("k", [1, 3])
@pytest.mark.parametrize("case", list(TWINS))
def test_span_equals_single_steps(gpu, monkeypatch, tmp_path, case, k):
    from qingdai_amd import history as hs
    nlat, nlon, ocean = TWINS[case]
    names, values, state = twin_reference(monkeypatch, case)
    assert len(names) == (23 if ocean else 17)
    # liveness: PRECIP moves from step to step, so a sample taken behind the hoisted precipitation block would be the wrong step's
    p = names.index("PRECIP")
    assert any(not np.array_equal(values[i, p], values[i + 1, p]) for i in range(6))
    b = make(monkeypatch, nlat, nlon, ocean=ocean, routing=False)
    h = attach(b, tmp_path, k=k)
    b.run_steps(7)                                           # one span: the window is 2400 steps long
    sums, count = b.dev.history_read()
    flags = hs.schedule(0, 7, h.S, k)
    assert count == int(flags.sum()) == h.n_open == (7 if k == 1 else 3)
    want = host_sums(values, flags)
    for j, n in enumerate(names):
        assert same(sums[j], want[j]), (case, k, n, float(np.nanmax(np.abs(sums[j] - want[j]))))
    end = fetch(b.dev, list(state))
    for f in state:                                          # the lane reads: the state is that of a span without it
        assert same(end[f], state[f]), (case, k, f)
    assert b.history_lines == [] and not os.path.exists(tmp_path / "history")
    b.dev.close()


def test_lazily_stored_fields_are_stored_on_sampled_steps(gpu, monkeypatch, tmp_path):
    """Device.step_n without the hydrology bit: inside a span only the last step stores OLR, EFLUX, LHREL, ISR_A, C_SNOW ... unless
    a reader comes with the span.  The lane is one when an entry reads such a field: the sums of a 4-step span equal those of
    four one-step spans, each of which is its own last step."""
    from qingdai_amd import history as hs
    names = ["OLR", "EFLUX", "LHREL", "ISR_A", "C_SNOW", "TS"]
    flags = dict(with_ocean=True, with_physics=True, pass_albedo=False, with_hydrology=False)
    a = make(monkeypatch, 19, 36, routing=False)
    stars = a.forcing.star_table(DT * np.arange(4))
    values = []
    for i in range(4):
        a.dev.step_n(stars[i:i + 1], DT, **flags)
        values.append(entry_values(names, fetch(a.dev, names)))
    a.dev.close()
    assert any(not np.array_equal(values[i][0], values[i + 1][0]) for i in range(3))       # OLR moves from step to step
    b = make(monkeypatch, 19, 36, routing=False)
    h = attach(b, tmp_path, k=2, fields=names)
    b.dev.step_n(stars, DT, history=h, **flags)
    sums, count = b.dev.history_read()
    assert count == 2 and h.i == 4
    want = host_sums(values, hs.schedule(0, 4, h.S, 2))
    for j, n in enumerate(names):
        assert same(sums[j], want[j]), n
    b.dev.close()


# ---------------------------------------------------------------- 3: against the oracle
@pytest.mark.parametrize("use_ocean", [1, 0])
def test_mean_vs_oracle(gpu, tmp_path, use_ocean):
    """The set-up of test_gpu_parity.py::test_driver_loop_vs_oracle: 61 x 96, 4 steps, the cold state."""
    import qd_oracle as qo
    import qingdai_amd as qa
    from qd_oracle.driver import DriverOracle
    from qingdai_amd.driver import Simulation
    from test_gpu_parity import STEP_TOL
    from util import relerr
    nlat, nlon, nsteps = 61, 96, 4
    sim = Simulation(nlat, nlon, params=qa.QdParams(), use_ocean=bool(use_ocean), quiet=True, ecology=False)
    lat = np.deg2rad(sim.grid.lat_mesh)
    h0 = 8000.0 - 10500.0 * np.sin(lat) ** 2
    Ts0 = 262.0 + 36.0 * np.cos(lat) ** 2
    S0 = np.where((sim.land_mask == 1) & (np.abs(sim.grid.lat_mesh) > 55), 30.0, 0.0)
    sim.gcm.h, sim.gcm.T_s = h0, Ts0
    sim.dev.set("S_SNOW", S0)
    g = qo.Grid(nlat, nlon)
    P = qo.defaults()
    m = qo.AtmosOracle(g, sim.friction, sim.land_mask, P, C_s_map=np.where(sim.land_mask == 1, 3e6, P.Cs_ocean).astype(float))
    m.h, m.T_s = h0.copy(), Ts0.copy()
    oc = qo.OceanOracle(g, sim.land_mask, P, init_Ts=np.full((nlat, nlon), 288.0)) if use_ocean else None
    d = DriverOracle(g, m, oc, qo.Forcing(g), sim.land_mask, sim.base_albedo, P)
    d.S_snow = S0.copy()
    hist = attach(sim, tmp_path)
    sim.run_steps(nsteps)
    sums, count = sim.dev.history_read()
    assert count == nsteps
    got = dict(zip(hist.names, sums / count))
    want = {}
    for i in range(nsteps):
        d.step(i * 300.0, 300)
        now = {"U": m.u, "V": m.v, "H": m.h, "TS": m.T_s, "Q": m.q, "CLOUD": m.cloud_cover, "PRECIP": d.precip, "ALBEDO": d.albedo,
               "S_SNOW": d.S_snow, "W_LAND": d.W_land, "RUNOFF": d.R_flux}
        if use_ocean:
            now.update(UO=oc.uo, ETA=oc.eta, SST=oc.Ts)
        for name, x in now.items():
            want[name] = want.get(name, 0.0) + np.asarray(x, dtype=np.float64)
    errs = {name: relerr(got[name], x / nsteps) for name, x in want.items()}
    print(errs)
    assert len(errs) == (14 if use_ocean else 11)
    for name, e in errs.items():
        assert e < (1e-7 if name in ("UO", "ETA") else STEP_TOL), (name, e)
    sim.dev.close()


# ---------------------------------------------------------------- 4: chunking, other lanes, windows
FIRES = {0: 3, 2: 1, 5: 3}


def test_chunking_with_routing_and_budget(gpu, monkeypatch, tmp_path):
    got = []
    for cuts in ([7], [3, 4], [1] * 7):
        sim = make(monkeypatch, 37, 72, fires=FIRES)
        assert sim.routing is not None and sim.budget is not None
        attach(sim, tmp_path, k=1)
        for n in cuts:
            sim.run_steps(n)
        sums, count = sim.dev.history_read()
        assert count == 7 and len(sim.budget_lines) > 0
        got.append((sums, fetch(sim.dev, RESTART), sim.dev.route_download("BUFFER")))
        sim.dev.close()
    for sums, state, buf in got[1:]:
        assert sums.tobytes() == got[0][0].tobytes() and buf.tobytes() == got[0][2].tobytes()
        for f in state:
            assert state[f].tobytes() == got[0][1][f].tobytes(), f


def test_window_file(gpu, monkeypatch, tmp_path):
    from qingdai_amd import history as hs, ncio
    a = make(monkeypatch, 37, 72, fires=FIRES)
    names = hs.resolve_fields(None, True)
    values = single_steps(a, names, 4)
    a.dev.close()
    b = make(monkeypatch, 37, 72, fires=FIRES)
    h = attach(b, tmp_path, S=4)
    b.run_steps(7)
    files = sorted(os.listdir(tmp_path / "history"))
    assert len(files) == 1 and files == [os.path.basename(p) for p in h.files], files
    v, _ = ncio.read_nc(str(tmp_path / "history" / files[0]))
    mean = host_sums(values, [1] * 4) / np.float64(4)
    for j, n in enumerate(names):
        assert same(v[n.lower()], mean[j]), n
    assert int(v["complete"]) == 1 and int(v["n_samples"]) == 4 and int(v["sample_every"]) == 1
    assert float(v["t_start_seconds"]) == 0.0 and float(v["t_end_seconds"]) == 3 * DT and float(v["dt_seconds"]) == DT
    assert len(b.history_lines) == 1 and b.history_lines[0].startswith("[History] day ") and ": 4 samples | TS=" in b.history_lines[0]
    sums, count = b.dev.history_read()
    assert count == 3 == h.n_open and h.t_first == 4 * DT and h.t_last == 6 * DT and h.steps_to_window_end() == 1
    b.dev.close()


def test_wrong_schedule_length_runs_nothing(gpu, monkeypatch, tmp_path):
    from qingdai_amd import history as hs
    from qingdai_amd._lib import QdError

    class Short(hs.History):
        def span_schedule(self, t0, dt, n):
            k = super().span_schedule(t0, dt, n)
            self.dev.history_schedule(hs.schedule(self.i, n + 1, self.S, self.sample_every))
            return k
    sim = make(monkeypatch, 19, 36, fires=FIRES)
    h = attach(sim, tmp_path, cls=Short)
    before = fetch(sim.dev, RESTART)
    clocks = (sim.t, sim._step_index, h.span_clock(), sim.budget.span_clock(), sim.dev.counters())
    with pytest.raises(QdError, match="a qd_history_schedule must cover exactly the n steps of the span"):
        sim.run_steps(3)
    assert (sim.t, sim._step_index, h.span_clock(), sim.budget.span_clock(), sim.dev.counters()) == clocks
    after = fetch(sim.dev, RESTART)
    for f in before:
        assert before[f].tobytes() == after[f].tobytes(), f
    assert sim.dev.history_read()[1] == 0 and sim.budget_lines == []
    # the refused span left no schedule behind: the lane-free span after it runs
    lane, sim.history = sim.history, None
    sim.run_steps(2)
    assert sim._step_index == 2 and sim.dev.history_read()[1] == 0 and lane.i == 0
    sim.dev.close()


# ---------------------------------------------------------------- 5: the driver
def test_driver_main(gpu, tmp_path, monkeypatch, capsys):
    from qingdai_amd import driver, ncio
    for k in list(os.environ):
        if k.startswith("QD_"):
            monkeypatch.delenv(k)
    env = {"QD_N_LAT": "19", "QD_N_LON": "36", "QD_SIM_DAYS": "0.125", "QD_ECO_ENABLE": "0", "QD_DYN_DIAG_PRINT": "0", "QD_USE_OCEAN": "1",
           "QD_HYDRO_ENABLE": "0", "QD_HISTORY": "1", "QD_HISTORY_EVERY_DAYS": "0.05"}
    for k, v in env.items():
        monkeypatch.setenv(k, v)
    on = tmp_path / "on"
    on.mkdir()
    monkeypatch.chdir(on)
    assert driver.main() == 0
    out = capsys.readouterr().out
    day = 72000.0
    lines = [s for s in out.splitlines() if s.startswith("[History]")]
    assert len(lines) == 3 and [int(re.search(r": (\d+) samples", s).group(1)) for s in lines] == [12, 12, 6], out
    files = sorted(os.listdir(on / "output" / "history"))
    assert len(files) == 3 and all(re.fullmatch(r"history_day_\d+\.\d+_\d+\.\d+\.nc", f) for f in files), files
    seen = []
    for f, (first, last, n, complete) in zip(files, ((0, 11, 12, 1), (12, 23, 12, 1), (24, 29, 6, 0))):
        v, _ = ncio.read_nc(str(on / "output" / "history" / f))
        assert (int(v["n_samples"]), int(v["complete"]), int(v["sample_every"])) == (n, complete, 1), f
        assert float(v["t_start_seconds"]) == first * DT and float(v["t_end_seconds"]) == last * DT and float(v["dt_seconds"]) == DT
        a, b = (float(x) for x in re.fullmatch(r"history_day_(.+)_(.+)\.nc", f).groups())
        assert abs(a - first * DT / day) <= 0.005 and abs(b - last * DT / day) <= 0.005, f     # two decimals: |label - t / day| <= 0.005
        assert v["ts"].shape == (19, 36) and v["ts"].dtype == np.float64 and np.isfinite(v["ts"]).all() and "current_speed" in v
        seen.append(np.array(v["ts"]))
    assert not np.array_equal(seen[0], seen[1])
    # the same run without the switch: no directory, no line
    monkeypatch.delenv("QD_HISTORY")
    off = tmp_path / "off"
    off.mkdir()
    monkeypatch.chdir(off)
    assert driver.main() == 0
    assert "[History]" not in capsys.readouterr().out and not os.path.exists(off / "output" / "history")
