"""CPU: the host side of the time-mean history lane (qingdai_amd/history.py): the switches, the window clock and its schedules, the
file, the ABI.  No device: the file test uses a stand-in whose history_read returns known sums."""
import os
import re

import numpy as np
import pytest

from qingdai_amd import history as hs

HERE = os.path.dirname(os.path.abspath(__file__))
DT, DAY = 300.0, 72000.0


# ---------------------------------------------------------------- environment
def test_defaults():
    cfg = hs.read_env({})
    assert cfg == {"enabled": False, "every_days": 10.0, "sample_every": 1, "fields": None}
    cfg = hs.read_env({"QD_HISTORY": "1"})
    assert cfg["enabled"] and cfg["every_days"] == 10.0 and cfg["sample_every"] == 1 and cfg["fields"] is None
    dry = hs.resolve_fields(None, with_ocean=False)
    wet = hs.resolve_fields(None, with_ocean=True)
    assert dry == "TS,H,U,V,Q,CLOUD,HICE,PRECIP,ALBEDO,ISR,OLR,EFLUX,PCOND,W_LAND,S_SNOW,RUNOFF,WIND_SPEED".split(",")
    assert wet == dry + "SST,UO,VO,ETA,QNET,CURRENT_SPEED".split(",")
    assert len(wet) <= 32
    assert hs.entries_for(["TS", "WIND_SPEED", "CURRENT_SPEED"]) == [(0, "TS", None), (1, "U", "V"), (1, "UO", "VO")]


def test_field_names():
    cfg = hs.read_env({"QD_HISTORY": "1", "QD_HISTORY_FIELDS": " ts, Precip ,wind_speed,c_snow"})
    assert cfg["fields"] == ["TS", "PRECIP", "WIND_SPEED", "C_SNOW"]
    assert hs.resolve_fields(cfg["fields"], with_ocean=False) == cfg["fields"]
    with pytest.raises(ValueError, match="unknown field 'VORTICITY'"):
        hs.read_env({"QD_HISTORY": "1", "QD_HISTORY_FIELDS": "TS,vorticity"})
    with pytest.raises(ValueError, match="unknown field 'LAND_MASK'"):        # a mask is no f64 plane
        hs.read_env({"QD_HISTORY": "1", "QD_HISTORY_FIELDS": "LAND_MASK"})
    for name in ("SST", "current_speed"):
        with pytest.raises(ValueError, match=f"'{name.upper()}' needs the ocean"):
            hs.resolve_fields(hs.parse_fields(name), with_ocean=False)
    assert hs.resolve_fields(hs.parse_fields("sst"), with_ocean=True) == ["SST"]
    with pytest.raises(ValueError, match="33 entries, at most 32"):
        hs.parse_fields(",".join(["TS"] * 33))
    assert len(hs.parse_fields(",".join(["TS"] * 32))) == 32
    # the switch off: the list is not even looked at
    assert hs.read_env({"QD_HISTORY": "0", "QD_HISTORY_FIELDS": "nonsense"})["fields"] is None


@pytest.mark.parametrize("text", ["abc", "0", "-3", "nan", ""])
def test_numeric_fallbacks(text):
    cfg = hs.read_env({"QD_HISTORY": "1", "QD_HISTORY_EVERY_DAYS": text, "QD_HISTORY_SAMPLE_EVERY": text})
    assert cfg["every_days"] == 10.0 and cfg["sample_every"] == 1


def test_numeric_values_and_switch_off():
    cfg = hs.read_env({"QD_HISTORY": "1", "QD_HISTORY_EVERY_DAYS": "0.5", "QD_HISTORY_SAMPLE_EVERY": "4"})
    assert cfg["every_days"] == 0.5 and cfg["sample_every"] == 4
    for env in ({}, {"QD_HISTORY": "0"}, {"QD_HISTORY": "2"}, {"QD_HISTORY": "x"}):
        assert hs.from_env(None, None, env) is None             # nothing is touched: neither the device nor the grid


# ---------------------------------------------------------------- clock
def test_steps_per_window():
    assert hs.steps_per_window(10, DAY, DT) == 2400
    assert hs.steps_per_window(0.01, DAY, DT) == 2
    assert hs.steps_per_window(1e-6, DAY, DT) == 1
    assert hs.steps_per_window(0.05, DAY, DT) == 12


def replay(i0, n, S, k):
    return [1 if ((i0 + s) % S) % k == 0 else 0 for s in range(n)]


@pytest.mark.parametrize("k", [1, 3])
def test_schedules(k):
    S = 7
    mid = hs.schedule(3, 3, S, k)                        # starts mid-window, stays inside
    end = hs.schedule(3, 4, S, k)                        # ends on the window's last step (index 6)
    over = hs.schedule(5, 6, S, k)                       # straddles the boundary between 6 and 7
    assert mid.dtype == np.int32 and mid.tolist() == replay(3, 3, S, k)
    assert end.tolist() == replay(3, 4, S, k) and over.tolist() == replay(5, 6, S, k)
    if k == 1:
        assert mid.tolist() == [1, 1, 1] and over.tolist() == [1] * 6
    else:
        assert mid.tolist() == [1, 0, 0] and end.tolist() == [1, 0, 0, 1]
        # 5, 6 | 7, 8, 9, 10: the phase restarts with the window -- step 6 is sampled (6 % 3 == 0) and so is step 7 (position 0)
        assert over.tolist() == [0, 1, 1, 0, 0, 1]
    # cutting a window into spans does not move its samples
    whole = hs.schedule(0, 3 * S, S, k).tolist()
    assert whole == hs.schedule(0, 5, S, k).tolist() + hs.schedule(5, 9, S, k).tolist() + hs.schedule(14, 7, S, k).tolist()
    assert whole[:S] == whole[S:2 * S] == whole[2 * S:]


class StandIn:
    """A device that records what the History asks of it."""

    def __init__(self, sums=None, count=0):
        self.sums, self.count, self.calls = sums, count, []
        self.params = type("P", (), {"omega": 2.0 * np.pi / DAY})()

    def history_configure(self, entries):
        self.calls.append(("configure", list(entries)))

    def history_schedule(self, flags):
        self.calls.append(("schedule", np.asarray(flags).tolist()))

    def history_read(self):
        return self.sums, self.count

    def history_reset(self):
        self.calls.append(("reset",))
        self.count = 0


def make(tmp_path, sums=None, count=0, fields="TS,PRECIP,WIND_SPEED", every="0.05", k="1", out=None):
    import qingdai_amd as qa
    grid = qa.SphericalGrid(5, 6)
    dev = StandIn(sums, count)
    lines = [] if out is None else out
    cfg = hs.read_env({"QD_HISTORY": "1", "QD_HISTORY_FIELDS": fields, "QD_HISTORY_EVERY_DAYS": every, "QD_HISTORY_SAMPLE_EVERY": k})
    h = hs.History(dev, grid, cfg, with_ocean=False, dt=DT, day=DAY, out=lines.append, output_dir=str(tmp_path))
    return h, dev, grid, lines


def test_window_end_and_span_protocol(tmp_path):
    h, dev, _, _ = make(tmp_path, every="0.05", k="3")
    assert h.S == 12 and dev.calls[0] == ("configure", [(0, "TS", None), (0, "PRECIP", None), (1, "U", "V")])
    assert [h.steps_to_window_end(i) for i in (0, 5, 11, 12, 23)] == [12, 7, 1, 12, 1]
    clock = h.span_clock()
    k = h.span_schedule(None, DT, 5)
    assert dev.calls[-1] == ("schedule", [1, 0, 0, 1, 0]) and k == (5, (0.0, 3 * DT), 2)
    h.span_restore(clock)                                 # a span that did not run leaves the clock alone
    assert h.i == 0 and h.n_open == 0 and h.t_first is None
    h._fired(h.span_schedule(1000.0, DT, 5))
    assert (h.i, h.t_first, h.t_last, h.n_open) == (5, 1000.0, 1000.0 + 3 * DT, 2) and not h.window_closed()
    times = 1000.0 + DT * np.arange(5, 12)
    h._fired(h.span_schedule(times, DT, 7))               # the driver hands the span's n times
    assert dev.calls[-1] == ("schedule", [0, 1, 0, 0, 1, 0, 0])
    assert (h.i, h.t_first, h.t_last, h.n_open) == (12, 1000.0, 1000.0 + 9 * DT, 4) and h.window_closed()
    assert h.steps_to_window_end() == 12


# ---------------------------------------------------------------- file
@pytest.mark.parametrize("complete", [1, 0])
def test_file(tmp_path, complete):
    from qingdai_amd import ncio
    r = np.random.default_rng(5)
    sums = r.normal(size=(3, 5, 6)) * 1e3
    sums[1, 2, 3] = np.nan
    sums[2, 0, 0] = np.inf
    h, dev, grid, lines = make(tmp_path, sums.copy(), 7, k="2")
    h.t_first, h.t_last, h.n_open = 600.0, 4200.0, 7
    path = h.flush(complete=complete)
    a, b = 600.0 / DAY, 4200.0 / DAY
    assert os.path.basename(path) == f"history_day_{a:05.2f}_{b:05.2f}.nc" and re.fullmatch(r"history_day_\d+\.\d+_\d+\.\d+\.nc", os.path.basename(path))
    assert os.path.dirname(path) == os.path.join(str(tmp_path), "history")
    assert os.listdir(os.path.dirname(path)) == [os.path.basename(path)]                # no temporary file is left
    v, _ = ncio.read_nc(path)
    assert set(v) == {"lat", "lon", "ts", "precip", "wind_speed", "n_samples", "t_start_seconds", "t_end_seconds", "dt_seconds",
                      "sample_every", "complete"}
    for k, name in enumerate(("ts", "precip", "wind_speed")):
        assert v[name].dtype == np.float64 and v[name].shape == (5, 6)
        assert np.array_equal(v[name], sums[k] / 7, equal_nan=True), name
    assert np.array_equal(v["lat"], grid.lat) and np.array_equal(v["lon"], grid.lon) and v["lat"].dtype == np.float64
    assert int(v["n_samples"]) == 7 and int(v["sample_every"]) == 2 and int(v["complete"]) == complete
    _, full, _ = ncio.read_nc_full(path)
    assert {k: c for k, (c, _, _) in full.items() if k in ("n_samples", "sample_every", "complete")} == dict.fromkeys(("n_samples", "sample_every", "complete"), "i4")
    assert all(full[k][0] == "f8" and full[k][1] == () for k in ("t_start_seconds", "t_end_seconds", "dt_seconds"))
    assert full["ts"][1] == ("lat", "lon") and full["lat"][1] == ("lat",) and full["lon"][1] == ("lon",)
    assert float(v["t_start_seconds"]) == 600.0 and float(v["t_end_seconds"]) == 4200.0 and float(v["dt_seconds"]) == DT
    assert len(lines) == 1 and lines[0].startswith(f"[History] day {a:.2f}–{b:.2f}: 7 samples | TS=") and " PRECIP=nan " in lines[0]
    w = np.maximum(np.cos(np.deg2rad(grid.lat_mesh)), 0.0)
    assert f"TS={float(np.sum(w * (sums[0] / 7)) / np.sum(w)):.6g}" in lines[0]
    assert dev.calls[-1] == ("reset",) and h.n_open == 0 and h.t_first is None
    assert h.flush() is None and len(lines) == 1            # an empty window writes nothing


def test_failed_write_leaves_nothing_behind(tmp_path, monkeypatch):
    from qingdai_amd import ncio
    h, dev, _, lines = make(tmp_path, np.ones((3, 5, 6)), 2)
    h.t_first, h.t_last, h.n_open = 0.0, 300.0, 2

    def broken(path, dims, variables, attrs=None):
        open(path, "w").write("half a file")
        raise OSError("disk full")
    monkeypatch.setattr(ncio, "write_nc", broken)
    with pytest.raises(OSError, match="disk full"):
        h.flush()
    assert os.listdir(tmp_path / "history") == [] and lines == [] and h.files == []
    assert h.n_open == 2 and ("reset",) not in dev.calls       # the window is still there for the caller to decide
    h.drop()
    assert dev.calls[-1] == ("reset",) and h.n_open == 0 and h.t_first is None and h.t_last is None


def test_labels():
    assert hs.file_name(0.0, 9.99583, 1) == "history_day_00.0_10.0.nc"          # the frames' `05.1f`
    assert hs.label_decimals(10.0) == hs.label_decimals(1.0) == hs.label_decimals(0.1) == 1
    assert hs.label_decimals(0.05) == 2 and hs.label_decimals(0.01) == 2 and hs.label_decimals(0.004) == 3
    # the windows of a 0.05-day run keep their names apart
    d = hs.label_decimals(0.05)
    names = {hs.file_name(k * 0.05, k * 0.05 + 11 * DT / DAY, d) for k in range(40)}
    assert len(names) == 40


def test_six_entries_in_the_line(tmp_path):
    fields = "TS,H,U,V,Q,CLOUD,HICE,PRECIP"
    h, _, _, lines = make(tmp_path, np.ones((8, 5, 6)), 2, fields=fields)
    h.flush(0.0, 0.5)
    assert [s.split("=")[0] for s in lines[0].split("|")[1].split()] == fields.split(",")[:6]
    assert "day 0.00–0.50: 2 samples" in lines[0]


# ---------------------------------------------------------------- ABI
def test_abi_surface():
    from qingdai_amd import _lib
    from qingdai_amd.device import Device
    for n in ("qd_history_configure", "qd_history_schedule", "qd_history_sample", "qd_history_read", "qd_history_reset"):
        assert hasattr(Device, n[3:]), n            # that the header declares and the library exports them: tests/test_abi_cpu.py
    assert _lib.HISTORY_MAX_ENTRIES == 32
    assert "history" not in " ".join(_lib.STEP_BITS)        # no flag bit: a schedule turns the lane on
    src = open(os.path.join(HERE, "..", "qingdai_amd", "csrc", "qd_span.h")).read()
    assert "QD_LANE_HISTORY" in src
