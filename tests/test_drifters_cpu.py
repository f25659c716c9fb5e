"""CPU: the host side of the drifter lane (qingdai_amd/drifters.py) -- the NumPy restatement of the device's step on cases worked by
hand, the seeds, the environment, the window clock with its log-room cut, and the window file through a stand-in device."""
import os
import types

import numpy as np
import pytest

import qingdai_amd as qa
from qingdai_amd import drifters as D
from qingdai_amd import ncio

A = 6.371e6
DT = 300.0


def planes(grid, u=0.0, v=0.0):
    shape = (grid.n_lat, grid.n_lon)
    return np.full(shape, float(u)), np.full(shape, float(v))


def step(grid, r, c, U, V, dt=DT, land=None, status=None, blocked=None):
    r, c = np.atleast_1d(np.asarray(r, dtype=np.float64)), np.atleast_1d(np.asarray(c, dtype=np.float64))
    status = np.zeros_like(r) if status is None else status
    blocked = np.zeros_like(r) if blocked is None else blocked
    return D.advance_reference(r, c, status, blocked, U, V, land, grid.lat, dt, A, land is not None)


def v_for(grid, dr, dt=DT):
    """The meridional speed that moves a particle by dr rows in dt."""
    return dr * A * np.deg2rad(grid.lat[1] - grid.lat[0]) / dt


def u_for(grid, dc, r, dt=DT):
    """The zonal speed that moves a particle on the integer row r by dc columns in dt."""
    return dc * A * np.deg2rad(360.0 / (grid.n_lon - 1)) / (dt * D.sec_table(grid.lat)[int(r)])


# ---------------------------------------------------------------- the metric
def test_solid_body_rotation_converges():
    """u = U0 cos(lat_j), v = 0: the latitude stays bit-exact (dr is exactly 0) and the error of the longitude rate, which is that
    of the interpolated sec * u against 1, falls like the square of the row spacing."""
    U0, err = 10.0, {}
    for n in (19, 37, 73, 145):
        grid = qa.SphericalGrid(n, 2 * (n - 1) + 1)
        lat = np.asarray(grid.lat, dtype=np.float64)
        U = np.repeat((U0 * np.cos(np.deg2rad(lat)))[:, None], grid.n_lon, axis=1)
        phi = np.linspace(-60.0, 60.0, 4801)
        r, c = D.to_index(phi, np.full(phi.shape, 10.0), grid)
        r1, c1, status, _ = step(grid, r, c, U, np.zeros_like(U))
        assert np.array_equal(r1, r) and not status.any()
        rate = (c1 - c) * np.deg2rad(360.0 / (grid.n_lon - 1)) / DT
        err[n] = float(np.abs(rate / (U0 / A) - 1.0).max())
    print(err, err[37] / err[73], err[73] / err[145], err[19] / err[37])
    assert err[37] / err[73] >= 3.5 and err[73] / err[145] >= 3.5
    assert 4.0e-3 < err[37] < 5.5e-3                               # 4.72e-3 on the bare interpolation


# ---------------------------------------------------------------- fold, by hand, on exact binary values
def test_fold_by_hand():
    grid = qa.SphericalGrid(19, 37)                                # P = 36, P / 2 = 18: every value below is exact
    P = 36.0
    U, V = planes(grid, v=v_for(grid, -0.5))
    dr = V[0, 0] * DT / (A * np.deg2rad(grid.lat[1] - grid.lat[0]))
    assert dr == -0.5                                              # the hand values are the arithmetic's
    r1, c1, status, _ = step(grid, 0.25, 3.0, U, V)
    assert (r1[0], c1[0], status[0]) == (0.25, 3.0 + P / 2, 0.0)   # 0.25 - 0.5 = -0.25 -> 0.25, half a turn
    r1, c1, status, _ = step(grid, 17.75, 30.0, U, -V)
    assert (r1[0], c1[0], status[0]) == (17.75, 30.0 + P / 2 - P, 0.0)      # the north pole: 18.25 -> 17.75, 48 wraps to 12
    # fold itself
    r, c, ok = D.fold([-0.25, 18.25, 5.0, 5.0, -19.0, 40.0, np.nan, 5.0], [3.0, 30.0, -0.5, 36.0 * 3 + 7.0, 0.0, 0.0, 0.0, np.inf], 19, 37)
    assert ok.tolist() == [True, True, True, True, False, False, False, False]
    assert r[:4].tolist() == [0.25, 17.75, 5.0, 5.0] and c[:4].tolist() == [21.0, 12.0, 35.5, 7.0]
    assert D.fold([1.0], [36.0], 19, 37)[1][0] == 0.0 and D.fold([1.0], [-36.0], 19, 37)[1][0] == 0.0
    # a zonal step of 3.5 periods on an integer row lands where c + 0.5 P does
    u = u_for(grid, 3.5 * P, 9)
    U, V = planes(grid, u=u)
    dc = u * DT * D.sec_table(grid.lat)[9] / (A * np.deg2rad(360.0 / 36.0))
    r1, c1, status, _ = step(grid, 9.0, 4.0, U, V)
    want = 4.0 + dc
    assert abs(dc - 3.5 * P) < 1e-9 and status[0] == 0.0 and r1[0] == 9.0
    assert c1[0] == want - P * np.floor(want / P) and abs(c1[0] - (4.0 + 0.5 * P)) < 1e-9
    # |dr| >= 2 (n_lat - 1): still outside after one reflection -> dead, where it was
    for sign in (1.0, -1.0):
        U, V = planes(grid, v=sign * v_for(grid, 36.5))
        r1, c1, status, _ = step(grid, 9.0, 4.0, U, V)
        assert (r1[0], c1[0], status[0]) == (9.0, 4.0, 1.0)


# ---------------------------------------------------------------- dead and blocked
def test_dead_particles():
    grid = qa.SphericalGrid(19, 37)
    for which, bad in (("u", np.inf), ("v", np.nan), ("v", -np.inf)):
        U, V = planes(grid, u=5.0, v=1.0)
        (U if which == "u" else V)[9, 4] = bad
        r1, c1, status, _ = step(grid, [9.5, 3.0], [4.5, 20.0], U, V)
        assert (r1[0], c1[0], status[0]) == (9.5, 4.5, 1.0), which         # the bad corner is one of its four
        assert status[1] == 0.0 and c1[1] != 20.0                          # its neighbour far away moves
    # a NaN in a corner of weight zero still kills: 0 * NaN is NaN
    U, V = planes(grid, u=5.0, v=1.0)
    U[10, 5] = np.nan                                              # (r, c) = (9, 4) exactly: the corners (10, .) and (., 5) weigh 0
    r1, c1, status, _ = step(grid, 9.0, 4.0, U, V)
    assert (r1[0], c1[0], status[0]) == (9.0, 4.0, 1.0)
    # dead never moves again, whatever the planes say afterwards
    U, V = planes(grid, u=5.0, v=1.0)
    r2, c2, status2, _ = step(grid, r1, c1, U, V, status=status)
    assert (r2[0], c2[0], status2[0]) == (9.0, 4.0, 1.0)
    # a non-finite dt kills everything and moves nothing
    r3, c3, status3, _ = step(grid, [2.0, 3.0], [1.0, 2.0], U, V, dt=np.inf)
    assert status3.tolist() == [1.0, 1.0] and r3.tolist() == [2.0, 3.0]


def test_blocked_particles():
    grid = qa.SphericalGrid(19, 37)
    land = np.zeros((19, 37), dtype=np.uint8)
    land[9, 10] = 1                                                # a one-cell island
    land[:, 0] = land[:, 36] = 1                                   # and land on the seam
    U, V = planes(grid, u=u_for(grid, 1.0, 9))
    # (9, 9.25) + 1 column -> (9, 10.25): nearest cell (9, 10) is land: rejected, counted.  (8.4, 9.25) moves along the coast:
    # its nearest cell is (8, 10), ocean
    sec = D.sec_table(grid.lat)
    r1, c1, status, blocked = step(grid, [9.0, 9.0], [9.25, 12.0], U, V, land=land)
    assert (r1[0], c1[0], blocked[0], status[0]) == (9.0, 9.25, 1.0, 0.0)
    assert c1[1] > 12.9 and blocked[1] == 0.0
    r1, c1, status, blocked = step(grid, [8.4], [9.25], U, V, land=land)
    assert blocked[0] == 0.0 and c1[0] > 10.0 and r1[0] == 8.4 and sec[8] > sec[9]
    # the seam: c' = 35.6 has the nearest column 36, which is column 0: land
    r1, c1, status, blocked = step(grid, [9.0], [34.6], U, V, land=land)
    assert (c1[0], blocked[0]) == (34.6, 1.0)
    r2, c2, _, blocked = step(grid, r1, c1, U, V, land=land, blocked=blocked)
    assert (c2[0], blocked[0]) == (34.6, 2.0)
    # without the ocean flag the mask is not read and blocked is carried
    r1, c1, _, blocked = D.advance_reference([9.0], [9.25], [0.0], [7.0], U, V, land, grid.lat, DT, A, False)
    assert c1[0] > 10.0 and blocked[0] == 7.0


def test_sample_reference_is_the_oracles_bilinear():
    from qd_oracle import numerics
    r = np.random.default_rng(5)
    f = r.normal(size=(7, 12))
    rr, cc = r.uniform(0, 6, 50), r.uniform(0, 11, 50) * (1 - 1e-12)
    rr[:3], cc[:3] = [0.0, 6.0, 3.0], [0.0, np.nextafter(11.0, 0.0), 4.0]
    assert np.array_equal(D.sample_reference(f, rr, cc), numerics.bilinear_wrap(f, rr, cc))


# ---------------------------------------------------------------- seeds
def test_seeds():
    grid = qa.SphericalGrid(19, 36)
    r, c = D.seed_fibonacci(500, grid)
    r2, c2 = D.seed_fibonacci(500, grid)
    assert np.array_equal(r, r2) and np.array_equal(c, c2) and len(r) == 500
    assert (r >= 0).all() and (r <= 18).all() and (c >= 0).all() and (c < 35).all()
    lat, _ = D.to_degrees(r, c, 19, 36)
    assert abs(np.sin(np.deg2rad(lat)).mean()) < 1e-3 and len(np.unique(np.round(c, 6))) > 490      # even in sin(lat), spread in lon
    land = np.zeros((19, 36), dtype=np.uint8)
    land[4:12, 3:20] = 1
    land[:, 0] = 1
    ro, co = D.seed_fibonacci(500, grid, land)
    jr, jc = D.nearest_cell(ro, co, 36)
    assert 0 < len(ro) < 500 and not land[jr, jc].any()
    assert len(D.seed_fibonacci(0, grid)[0]) == 0
    rr, cc = D.to_index([-90.0, 90.0, 0.0, 0.0], [0.0, 360.0, -10.0, 725.0], grid)
    assert rr.tolist() == [0.0, 18.0, 9.0, 9.0] and cc[0] == 0.0 and cc[1] == 0.0 and abs(cc[2] - 35 * 350 / 360) < 1e-9 and abs(cc[3] - 35 * 5 / 360) < 1e-9
    with pytest.raises(ValueError, match="not finite"):
        D.to_index([np.nan], [0.0], grid)


# ---------------------------------------------------------------- the environment
def test_read_env():
    cfg = D.read_env({})
    assert cfg == {"enabled": False, "n_atm": 4096, "n_ocn": 4096, "every": 24, "every_days": 10.0, "sample_atm": ["TS", "H"],
                   "sample_ocn": ["SST"], "log_cap": None}
    cfg = D.read_env({"QD_DRIFTERS": "1", "QD_DRIFT_N_ATM": "7", "QD_DRIFT_N_OCN": "0", "QD_DRIFT_EVERY": "3", "QD_DRIFT_EVERY_DAYS": "0.5",
                      "QD_DRIFT_SAMPLE_ATM": "olr, q", "QD_DRIFT_SAMPLE_OCN": "", "QD_DRIFT_LOG_CAP": "2"})
    assert cfg == {"enabled": True, "n_atm": 7, "n_ocn": 0, "every": 3, "every_days": 0.5, "sample_atm": ["OLR", "Q"], "sample_ocn": [],
                   "log_cap": 2}
    for bad in ("0", "-4", "x"):
        assert D.read_env({"QD_DRIFTERS": "1", "QD_DRIFT_EVERY": bad})["every"] == 24
    for bad in ("0", "-1", "nan", "inf", "x"):
        assert D.read_env({"QD_DRIFTERS": "1", "QD_DRIFT_EVERY_DAYS": bad})["every_days"] == 10.0
    assert D.read_env({"QD_DRIFTERS": "1", "QD_DRIFT_N_ATM": "x"})["n_atm"] == 4096
    with pytest.raises(ValueError, match=r"QD_DRIFT_N_OCN: 1048577 particles, a population holds 0 to 1048576"):
        D.read_env({"QD_DRIFTERS": "1", "QD_DRIFT_N_OCN": str((1 << 20) + 1)})
    with pytest.raises(ValueError, match="QD_DRIFT_N_ATM: -1 particles"):
        D.read_env({"QD_DRIFTERS": "1", "QD_DRIFT_N_ATM": "-1"})
    with pytest.raises(ValueError, match="QD_DRIFT_SAMPLE_ATM: unknown field 'NOPE'"):
        D.read_env({"QD_DRIFTERS": "1", "QD_DRIFT_SAMPLE_ATM": "TS,NOPE"})
    with pytest.raises(ValueError, match="QD_DRIFT_SAMPLE_ATM: PRECIP cannot be sampled: inside a span the hoisted precipitation block"):
        D.read_env({"QD_DRIFTERS": "1", "QD_DRIFT_SAMPLE_ATM": "PRECIP"})
    with pytest.raises(ValueError, match="QD_DRIFT_SAMPLE_OCN: 5 fields, at most 4"):
        D.read_env({"QD_DRIFTERS": "1", "QD_DRIFT_SAMPLE_OCN": "SST,UO,VO,ETA,QNET"})
    with pytest.raises(ValueError, match="QD_DRIFT_SAMPLE_ATM: 'WIND_SPEED' is no plane"):
        D.read_env({"QD_DRIFTERS": "1", "QD_DRIFT_SAMPLE_ATM": "WIND_SPEED"})
    assert D.read_env({"QD_DRIFT_SAMPLE_ATM": "NOPE"})["enabled"] is False          # off: nothing is parsed, nothing refused
    assert D.log_capacity(D.record_width(4096, 2, 4096, 1)) == 16
    assert D.log_capacity(D.record_width(1 << 20, 4, 1 << 20, 4)) == 2 and D.log_capacity(1 << 26) == 1


# ---------------------------------------------------------------- the window clock and the file, on a stand-in device
class StandInDevice:
    """What a Drifters needs of a Device: it remembers the schedules and hands back made-up records."""

    def __init__(self, cap=16):
        self.cap, self.flags, self.queued, self.made = cap, [], 0, 0

    def drift_configure(self, atm, ocn, sample_atm, sample_ocn, sec_row):
        self.n = (len(atm[0]), len(ocn[0]))
        self.ns = (len(sample_atm), len(sample_ocn))
        self.width = D.record_width(self.n[0], self.ns[0], self.n[1], self.ns[1])
        assert np.array_equal(sec_row, D.sec_table(np.linspace(-90, 90, len(sec_row))))
        return self.cap

    def drift_schedule(self, flags):
        self.flags.append(np.asarray(flags).copy())
        self.queued += int(np.count_nonzero(flags))
        assert self.queued <= self.cap, "the span would overflow the device log"

    def drift_log(self, want):
        n, self.queued = self.queued, 0
        rec = np.zeros((n, self.width))
        na, no = self.n
        for k in range(n):
            parts = D.split_records(rec[k:k + 1], na, self.ns[0], no, self.ns[1])
            parts["atm"][0, 0, :], parts["atm"][0, 1, :] = 9.0, np.arange(na) % 35
            parts["atm"][0, 2, :1] = 1.0                           # one dead
            parts["ocn"][0, 0, :], parts["ocn"][0, 1, :] = 4.5, 17.5
            parts["ocn"][0, 3, :] = 2.0
            parts["ocn"][0, 4:, :] = 280.0 + self.made          # the record's number in the run, however the run is cut
            self.made += 1
        return rec


def stand_in(tmp_path, lines, ocean=True, cap=16, **cfg):
    grid = qa.SphericalGrid(19, 36)
    sim = types.SimpleNamespace(dev=StandInDevice(cap), grid=grid, ocean=object() if ocean else None, dt=DT, day_seconds=72000.0,
                                land_mask=np.zeros((19, 36), dtype=np.uint8))
    return sim, D.Drifters(sim, cfg=D.default_config(**cfg), out=lines.append, output_dir=str(tmp_path))


def run(dri, n):
    """What Simulation._run_cut does with the lane."""
    spans = []
    while n > 0:
        k = min(n, dri.steps_to_window_end())
        dri._fired(dri.span_schedule(None, DT, k))
        dri.span_deliver(DT)
        spans.append(k)
        n -= k
        if dri.window_closed():
            dri.flush()
    return spans


def test_window_clock_and_log_room(tmp_path):
    lines = []
    _, dri = stand_in(tmp_path, lines, n_atm=5, n_ocn=3, every=2, every_days=0.05)        # S = 12 steps, records at 0, 2, ..., 10
    assert dri.S == 12 and dri.cap == 16 and dri.n == {"atm": 5, "ocn": 3}
    assert [dri.steps_to_window_end(i) for i in (0, 1, 11, 12, 23)] == [12, 11, 1, 12, 1]
    assert run(dri, 30) == [12, 12, 6] and len(dri.files) == 2
    recs, times, steps = dri.window()
    assert steps.tolist() == [24, 26, 28] and times.tolist() == [24 * DT, 26 * DT, 28 * DT]
    # the log-room cut: a cap of 2 ends a chunk with the step of the second record since the drain
    lines2 = []
    _, small = stand_in(tmp_path / "small", lines2, n_atm=5, n_ocn=3, every=2, every_days=0.05, log_cap=2)
    assert small.cap == 2 and [small.steps_to_window_end(i) for i in (0, 1, 2, 3, 9, 10, 11)] == [3, 4, 3, 4, 3, 2, 1]
    assert run(small, 30) == [3, 4, 4, 1, 3, 4, 4, 1, 3, 3]        # never more than two records in a span
    assert all(np.count_nonzero(f) <= 2 for f in small.dev.flags)
    assert [os.path.basename(f) for f in small.files] == [os.path.basename(f) for f in dri.files] and lines2 == lines
    for fa, fb in zip(dri.files, small.files):                     # the cut does not change the file
        va, vb = ncio.read_nc(fa)[0], ncio.read_nc(fb)[0]
        assert va.keys() == vb.keys() and all(np.asarray(va[k]).tobytes() == np.asarray(vb[k]).tobytes() for k in va)
    # a device log smaller than the wish wins; the clock goes back when a span did not run
    _, tiny = stand_in(tmp_path / "tiny", [], cap=1, n_atm=5, n_ocn=3, every=2, every_days=0.05, log_cap=8)
    assert tiny.cap == 1 and tiny.steps_to_window_end() == 1 and tiny.steps_to_window_end(1) == 2
    clock = tiny.span_clock()
    tiny._fired(tiny.span_schedule(None, DT, 1))
    tiny.span_restore(clock)
    assert tiny.i == 0 and tiny._pending == []


def test_window_file(tmp_path):
    lines = []
    sim, dri = stand_in(tmp_path, lines, n_atm=5, n_ocn=3, every=3, every_days=0.05)
    run(dri, 12)
    assert [os.path.basename(f) for f in dri.files] == ["drifters_day_00.00_00.04.nc"] and os.path.dirname(dri.files[0]) == str(tmp_path / "drifters")
    v, _ = ncio.read_nc(dri.files[0])
    assert set(v) == {"time_seconds", "step", "atm_lat", "atm_lon", "atm_status", "atm_ts", "atm_h", "ocn_lat", "ocn_lon", "ocn_status",
                      "ocn_blocked", "ocn_sst", "dt_seconds", "sample_every", "complete"}
    assert v["step"].tolist() == [0, 3, 6, 9] and v["time_seconds"].tolist() == [0.0, 900.0, 1800.0, 2700.0]
    assert v["atm_lat"].shape == (4, 5) and v["ocn_lon"].shape == (4, 3) and (v["atm_lat"] == 0.0).all()
    assert np.array_equal(v["atm_lon"][0], np.arange(5) * (360.0 / 35)) and (v["ocn_lat"] == -90.0 + 4.5 * 10.0).all()
    assert v["atm_status"][:, 0].tolist() == [1, 1, 1, 1] and not v["atm_status"][:, 1:].any() and (v["ocn_blocked"] == 2).all()
    assert v["ocn_sst"][:, 0].tolist() == [280.0, 281.0, 282.0, 283.0]
    assert (int(v["complete"]), int(v["sample_every"]), float(v["dt_seconds"])) == (1, 3, DT)
    assert lines == ["[Drifters] day 0.00–0.04: 4 records | atm 4/1 | ocn 3/0/6"]
    # an open window is written with complete = 0, an empty one not at all
    run(dri, 4)
    path = dri.flush(complete=0)
    assert int(ncio.read_nc(path)[0]["complete"]) == 0 and ncio.read_nc(path)[0]["step"].tolist() == [12, 15]
    assert dri.flush(complete=0) is None and len(dri.files) == 2
    # the window travels through window() / restore_window()
    run(dri, 2)                                                    # steps 16, 17: no record (12 + 6 = 18 is the next)
    run(dri, 1)
    recs, times, steps = dri.window()
    _, other = stand_in(tmp_path / "b", [], n_atm=5, n_ocn=3, every=3, every_days=0.05)
    other.restore_window(recs, times, steps, dri.i)
    assert other.i == 19 and all(np.array_equal(a, b) for a, b in zip(other.window(), (recs, times, steps)))
    assert other.key() == dri.key() == "atm=5:TS,H|ocn=3:SST|every=3"
    # without the ocean: no ocn population from the environment, and a caller's ocn seeds are refused
    _, dry = stand_in(tmp_path / "dry", [], ocean=False, n_atm=5, n_ocn=3)
    assert dry.n == {"atm": 5, "ocn": 0} and dry.samples["ocn"] == []
    with pytest.raises(ValueError, match="the ocn population needs the ocean, which is off in this run"):
        D.Drifters(types.SimpleNamespace(**{**vars(sim), "ocean": None}), ocn=([0.0], [10.0]))
    with pytest.raises(ValueError, match="QD_DRIFT_SAMPLE_ATM: field 'SST' needs the ocean"):
        stand_in(tmp_path / "dry2", [], ocean=False, sample_atm=["SST"])
    # caller-chosen seeds
    own = D.Drifters(sim, atm=([0.0, 45.0], [10.0, 350.0]), out=lines.append, output_dir=str(tmp_path))
    assert own.n == {"atm": 2, "ocn": 0} and own.width == 2 * 5
