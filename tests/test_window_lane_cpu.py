"""
The shared host side of the eight windowed lanes (qingdai_amd/window_lane.py), on a fake device: the window clock, the span
protocol's rollback, the forms of t0, the log lanes' drain check, the drifters' log cap, the atomic write, Simulation.flush_window and
the environment helpers.  Plain NumPy, no GPU.
"""
import math
import os
import types

import numpy as np
import pytest

import qingdai_amd as qa
from qingdai_amd import drifters, driver, eddy, extremes, flow, history, ncio, series, spectra, spharm, window_lane as wl

DT, DAY = 300.0, 72000.0
N_LAT, N_LON = 7, 12
LOG_LANES = ("series", "spectra", "drifters", "flow", "spharm")
SUM_LANES = ("history", "eddy", "extremes")


class FakeDev:
    """What the eight lanes ask of a Device: <lane>_configure, _schedule (recorded in `flags`; raises with fail_upload), _log (hands
    back the queued records, `short` fewer), _reset (counted), and history_read for the one sum lane that is flushed here."""

    def __init__(self, cap=16):
        self.params = types.SimpleNamespace(omega=2.0 * np.pi / DAY, a=6.371e6)
        self.cap, self.flags, self.queue, self.resets = cap, [], [], 0
        self.fail_upload, self.short = False, 0
        self.sums, self.count = np.ones((1, N_LAT, N_LON)), 0

    def __getattr__(self, name):
        verb = name.partition("_")[2]
        if verb not in ("configure", "schedule", "log", "reset"):
            raise AttributeError(name)
        return getattr(self, "_" + verb)

    def _configure(self, *args):
        return self.cap                              # (what drift_configure returns; the others return nothing that is read)

    def _schedule(self, flags):
        if self.fail_upload:
            raise RuntimeError("the upload failed")
        self.flags.append(np.asarray(flags).tolist())

    def _log(self, want=None):
        out, self.queue = self.queue[:len(self.queue) - self.short], []
        return np.array(out).reshape(len(out), -1)

    def _reset(self):
        self.resets += 1
        self.count = 0

    def history_read(self):
        return self.sums, self.count


def make(name, tmp_path=None, S=5, every=2, cap=16, lines=None):
    """The lane `name` on a FakeDev, with S steps per window and every `every`-th of them sampled -> (lane, dev)."""
    dev, grid = FakeDev(cap), qa.SphericalGrid(N_LAT, N_LON)
    days = S * DT / DAY
    kw = dict(dt=DT, day=DAY, out=(lines if lines is not None else []).append, output_dir=None if tmp_path is None else str(tmp_path))
    if name == "history":
        lane = history.History(dev, grid, {"every_days": days, "sample_every": every, "fields": ["TS"]}, with_ocean=False, **kw)
    elif name == "series":
        lane = series.Series(dev, grid, {"every_days": days, "every": every, "zonal": True, "fields": ["TS"]}, with_ocean=False, **kw)
    elif name == "spectra":
        lane = spectra.Spectra(dev, grid, {"every_days": days, "every": every, "lat": False, "fields": ["U"]}, with_ocean=False, **kw)
    elif name == "drifters":
        sim = types.SimpleNamespace(dev=dev, grid=grid, ocean=None, dt=DT, day_seconds=DAY, land_mask=np.zeros((N_LAT, N_LON), dtype=np.uint8))
        lane = drifters.Drifters(sim, atm=([0.0, 10.0], [5.0, 50.0]), cfg=drifters.default_config(every=every, every_days=days),
                                 out=kw["out"], output_dir=kw["output_dir"])
    elif name == "flow":
        lane = flow.Flow(dev, grid, {"every_days": days, "every": every}, **kw)
    elif name == "spharm":
        lane = spharm.Spharm(dev, grid, {"every_days": days, "every": every, "two_d": False, "fields": ["H"]}, with_ocean=False, **kw)
    elif name == "eddy":
        lane = eddy.Eddy(dev, grid, {"every_days": days, "sample_every": every, "pairs": "U*V", "maps": False}, with_ocean=False, **kw)
    else:
        lane = extremes.Extremes(dev, grid, {"every_days": days, "sample_every": every}, with_ocean=False, fields=["TS"], thresholds="",
                                 bins="", **kw)
    assert lane.S == S and lane.i == 0 and lane.NAME == name and isinstance(lane, wl.LogWindowLane if name in LOG_LANES else wl.SumWindowLane)
    return lane, dev


def run_span(lane, dev, n, t0=None):
    """The span protocol as Device.step_n and the driver walk it; the fake device queues one record per sampled step."""
    k = lane.span_schedule(t0, DT, n)
    if isinstance(lane, wl.LogWindowLane):
        for step in k[2]:
            dev.queue.append(np.full(lane.width, float(step)))
    else:
        dev.count += k[2]
    lane._fired(k)
    return lane.span_deliver(DT)


def clock_state(lane):
    """Every clock attribute of a lane, and what a log lane holds."""
    if isinstance(lane, wl.SumWindowLane):
        return (lane.i, lane.t_first, lane.t_last, lane.n_open)
    return (lane.i, [(t.tolist(), s.tolist()) for t, s in lane._pending], [r.tolist() for r in lane.recs],
            [t.tolist() for t in lane.times], [s.tolist() for s in lane.steps])


# ------------------------------------------------------------------------------------- the window clock
@pytest.mark.parametrize("name", driver.WINDOW_LANES)
@pytest.mark.parametrize("S, every, spans", [(1, 1, (1, 1, 1)),            # every step is a window
                                             (5, 2, (5, 5, 5)),            # the phase restarts at each window: 0, 2, 4 | 5, 7, 9 | ...
                                             (5, 2, (3, 4, 3, 5))])        # the second span crosses a window's end
def test_window_clock(name, S, every, spans):
    lane, dev = make(name, S=S, every=every)
    i = 0
    for n in spans:
        assert lane.steps_to_window_end() == S - i % S
        assert [lane.steps_to_window_end(j) for j in range(i, i + n)] == [S - j % S for j in range(i, i + n)]
        run_span(lane, dev, n)
        brute = [1 if ((i + j) % S) % every == 0 else 0 for j in range(n)]
        assert dev.flags[-1] == brute == history.schedule(i, n, S, every).tolist() == wl.schedule(i, n, S, every).tolist()
        i += n
        assert lane.i == i and lane.window_closed() == (i % S == 0)
    assert not make(name, S=S, every=every)[0].window_closed()           # before the first step no window has closed
    assert history.schedule is wl.schedule and history.steps_per_window is wl.steps_per_window and history.label_decimals is wl.label_decimals


# ------------------------------------------------------------------------------------- a span that does not run
@pytest.mark.parametrize("name", driver.WINDOW_LANES)
def test_clock_restore(name):
    lane, dev = make(name)
    k = lane.span_schedule(None, DT, 3)              # one span that ran and is not yet delivered: a log lane then holds _pending
    lane._fired(k)
    before = clock_state(lane)
    assert before[0] == 3
    dev.fail_upload = True
    clock = lane.span_clock()
    with pytest.raises(RuntimeError, match="the upload failed"):
        lane.span_schedule(None, DT, 4)
    lane.span_restore(clock)
    assert clock_state(lane) == before and lane.span_clock() == clock
    dev.fail_upload = False                          # and one that was scheduled but whose device call failed
    clock = lane.span_clock()
    lane.span_schedule(None, DT, 4)
    lane.span_restore(clock)
    assert clock_state(lane) == before and lane.span_clock() == clock


# ------------------------------------------------------------------------------------- the three forms of t0
def test_span_times_literal():
    assert wl.span_times(3, None, 300.0, 3).tolist() == [900.0, 1200.0, 1500.0]
    assert wl.span_times(3, 1000.0, 300.0, 3).tolist() == [1000.0, 1300.0, 1600.0]
    assert wl.span_times(3, np.float64(1000.0), 300.0, 3).tolist() == [1000.0, 1300.0, 1600.0]
    assert wl.span_times(3, [7.0, 8.0, 11.0], 300.0, 3).tolist() == [7.0, 8.0, 11.0]
    assert wl.span_times(3, np.array([7, 8, 11]), 300.0, 3).dtype == np.float64


@pytest.mark.parametrize("name", driver.WINDOW_LANES)
@pytest.mark.parametrize("t0, sampled", [(None, [1200.0, 1500.0]), (1000.0, [1300.0, 1600.0]), ([7.0, 8.0, 11.0, 12.0], [8.0, 11.0])])
def test_t0_forms_through_a_lane(name, t0, sampled):
    lane, dev = make(name, S=5, every=2)
    run_span(lane, dev, 3)
    k = lane.span_schedule(t0, DT, 4)                # steps 3, 4 | 5, 6: sampled are step 4 (position 4) and step 5 (position 0)
    assert dev.flags[-1] == [0, 1, 1, 0]
    if name in SUM_LANES:
        assert k == (4, (sampled[0], sampled[1]), 2)
    else:
        assert k[0] == 4 and k[1].tolist() == sampled and k[2].tolist() == [4, 5] and k[2].dtype == np.int64


# ------------------------------------------------------------------------------------- the log lanes
@pytest.mark.parametrize("name", LOG_LANES)
def test_short_drain_is_an_error(name):
    lane, dev = make(name, S=5, every=2)
    assert len(run_span(lane, dev, 3)) == 2 and len(lane.window()[0]) == 2
    dev.short = 1
    with pytest.raises(RuntimeError) as e:
        run_span(lane, dev, 5)                       # steps 3 .. 7: sampled at 4, 5, 7
    assert str(e.value) == f"{type(lane).__name__}: the device log held 2 records where the schedule says 3"
    assert type(lane).__name__ == {"series": "Series", "spectra": "Spectra", "drifters": "Drifters", "flow": "Flow", "spharm": "Spharm"}[name]


@pytest.mark.parametrize("name", LOG_LANES)
def test_window_and_restore_window(name):
    lane, dev = make(name, S=5, every=2)
    empty = lane.window()
    assert [np.shape(x) for x in empty] == [(0, lane.width), (0,), (0,)] and empty[2].dtype == np.int64
    assert run_span(lane, dev, 2).shape == (1, lane.width) and run_span(lane, dev, 1).shape == (1, lane.width)
    assert lane.span_deliver(DT).shape == (0, lane.width)                # nothing pending: nothing asked of the device
    recs, times, steps = lane.window()
    assert steps.tolist() == [0, 2] and times.tolist() == [0.0, 600.0] and recs[:, 0].tolist() == [0.0, 2.0]
    other, _ = make(name, S=5, every=2)
    other.restore_window(recs, times, steps, lane.i)
    assert other.i == 3 and all(np.array_equal(a, b) for a, b in zip(other.window(), (recs, times, steps)))
    other.restore_window(np.empty((0, lane.width)), [], [], 0)
    assert other.i == 0 and len(other.window()[0]) == 0


# ------------------------------------------------------------------------------------- the drifters' log cap
@pytest.mark.parametrize("cap", [1, 2, 16])
@pytest.mark.parametrize("every", [1, 3])
def test_drifters_log_cap(cap, every):
    S = 12
    lane, _ = make("drifters", S=S, every=every, cap=cap)
    assert lane.cap == cap
    for pos in range(S):
        steps = records = 0
        while True:                                  # walk the window from pos: stop behind the cap-th record or the window's last step
            p = pos + steps
            steps += 1
            records += p % every == 0
            if records == cap or p == S - 1:
                break
        assert lane.steps_to_window_end(pos) == lane.steps_to_window_end(pos + 3 * S) == steps, (cap, every, pos)


# ------------------------------------------------------------------------------------- the atomic write
def test_write_atomic(tmp_path, monkeypatch):
    path = str(tmp_path / "sub" / "dir" / "x.nc")
    dims, variables = {"n": 3}, {"a": ("f8", ("n",), np.arange(3.0))}
    wl.write_atomic(path, dims, variables)           # makes the directories
    first = open(path, "rb").read()
    assert os.listdir(os.path.dirname(path)) == ["x.nc"] and np.array_equal(ncio.read_nc(path)[0]["a"], np.arange(3.0))
    real = ncio.write_nc

    def half_then_raise(tmp, dims, variables, attrs=None):
        real(tmp, dims, variables)
        assert tmp == path + ".part" and os.path.exists(tmp)
        raise OSError("the disk is full")
    monkeypatch.setattr(ncio, "write_nc", half_then_raise)
    with pytest.raises(OSError, match="the disk is full"):
        wl.write_atomic(path, dims, {"a": ("f8", ("n",), np.zeros(3))})
    assert os.listdir(os.path.dirname(path)) == ["x.nc"] and open(path, "rb").read() == first
    monkeypatch.setattr(ncio, "write_nc", real)
    wl.write_atomic(path, dims, {"a": ("f8", ("n",), np.zeros(3))})
    assert np.array_equal(ncio.read_nc(path)[0]["a"], np.zeros(3))
    assert wl.window_file_name("flow", 0.5, 12.25, 1) == "flow_day_00.5_12.2.nc" == flow.file_name(0.5, 12.25)
    assert wl.window_file_name("eddy", 0.5, 12.25, 3) == "eddy_day_00.500_12.250.nc" == eddy.file_name(0.5, 12.25, 3)


# ------------------------------------------------------------------------------------- Simulation.flush_window
@pytest.mark.parametrize("name, tag", [("series", "Series"), ("history", "History")])
def test_flush_window_failure_is_not_fatal(name, tag, tmp_path, monkeypatch, capsys):
    lines = []
    lane, dev = make(name, tmp_path, S=5, every=2, lines=lines)
    sim = driver.Simulation.__new__(driver.Simulation)
    setattr(sim, name, lane)
    run_span(lane, dev, 5)
    assert lane.window_closed()
    real = ncio.write_nc

    def boom(*a, **k):
        raise OSError("no space left")
    monkeypatch.setattr(ncio, "write_nc", boom)
    resets = dev.resets
    assert getattr(sim, "flush_" + name)() is None
    assert capsys.readouterr().out == f"[{tag}] window skipped: no space left\n" and lines == [] and lane.files == []
    if name == "series":                             # drop() ran: the window is gone
        assert len(lane.window()[0]) == 0
    else:
        assert dev.resets == resets + 1 and (lane.t_first, lane.t_last, lane.n_open) == (None, None, 0)
    assert not os.path.exists(str(tmp_path / name)) or os.listdir(str(tmp_path / name)) == []
    monkeypatch.setattr(ncio, "write_nc", real)      # the run continues: the next window is written
    run_span(lane, dev, 5)
    path = sim.flush_window(name)
    assert path == lane.files[0] and os.path.basename(path) == f"{name}_day_00.02_00.04.nc" and os.listdir(os.path.dirname(path)) == [os.path.basename(path)]
    assert len(lines) == 1 and lines[0].startswith(f"[{tag}] day 0.02–0.04: 3 samples | TS=") and capsys.readouterr().out == ""
    assert sim.flush_window(name) is None            # an empty window writes nothing


def test_driver_orders():
    assert driver.WINDOW_LANES == ("history", "series", "spectra", "drifters", "flow", "spharm", "eddy", "extremes")
    assert driver.MID_RUN_FLUSH_ORDER == ("flow", "spharm", "eddy", "extremes", "history", "series", "spectra", "drifters")
    sim = driver.Simulation.__new__(driver.Simulation)
    assert sim._window_lanes() == {}
    sim.flow, sim.history = make("flow")[0], make("history")[0]
    assert list(sim._window_lanes()) == ["history", "flow"]
    for name in driver.WINDOW_LANES:
        assert callable(getattr(sim, "enable_" + name)) and callable(getattr(sim, "flush_" + name))


# ------------------------------------------------------------------------------------- the environment helpers
@pytest.mark.parametrize("value", ["", "x", "0", "-3", "nan", "inf", None, ["4"]])
def test_env_helpers_fall_back(value):
    env = {"K": value}
    assert wl.env_every(env, "K", 7) == 7
    assert wl.env_days(env, "K", 10.0) == 10.0
    assert wl.env_int(env, "K", 7) == (7 if value not in ("0", "-3") else int(value))


def test_env_helpers_values():
    assert wl.env_int({}, "K", 3) == 3 and wl.env_int({"K": " 12 "}, "K", 3) == 12 and wl.env_int({"K": 5}, "K", 3) == 5
    assert wl.env_every({"K": "4"}, "K", 24) == 4 and wl.env_every({}, "K", 24) == 24 and wl.env_every({"K": "4.0"}, "K", 24) == 24
    assert wl.env_days({"K": "0.25"}, "K") == 0.25 and wl.env_days({}, "K") == 10.0 and wl.env_days({"K": "-inf"}, "K", 2.0) == 2.0
    assert wl.env_days({"K": "1e-3"}, "K") == 1e-3 and math.isfinite(wl.env_days({"K": "1e400"}, "K"))
    # history's reader, the one that used to let a value that is no text raise
    cfg = history.read_env({"QD_HISTORY": 1.0, "QD_HISTORY_EVERY_DAYS": None, "QD_HISTORY_SAMPLE_EVERY": [2]})
    assert cfg == {"enabled": True, "every_days": 10.0, "sample_every": 1, "fields": None}
    for mod, switch in ((history, "QD_HISTORY"), (series, "QD_SERIES"), (spectra, "QD_SPECTRA"), (drifters, "QD_DRIFTERS"),
                        (flow, "QD_FLOW"), (spharm, "QD_SPHARM"), (eddy, "QD_EDDY"), (extremes, "QD_EXTREMES")):
        assert mod.read_env({})["enabled"] is False and mod.read_env({switch: "1"})["enabled"] is True
        assert mod.read_env({switch: "1"})["every_days"] == 10.0
