"""GPU (-m gpu): the per-step series lane (csrc/qd_series.hip, qingdai_amd/series.py).

The summation order is fixed, so everything here is bitwise (NaN equals NaN; the sign of every zero counts) but the a-priori bounds:
  1 the kernel alone through the class seam at ragged shapes against series.reduce_reference, with 1, 5 and 32 entries, zonal on
    and off, and the fsum bounds of tests/test_series_cpu.py on the device's own values;
  2 the refusals;
  3 one span against a cut span against one-step spans with a class-seam sample behind each;
  4 lazily stored diagnostics and PRECIP inside a long span;
  5 no effect on the other lanes and on the state; no series scope in the timing tables when the lane is off;
  6 driver.main;
  7 a run stopped inside a window and resumed (QD_CHECKPOINT=1) against the uncut run."""
import os
import re

import numpy as np
import pytest

from test_gpu_budget_diag import make, fetch, DT
from test_series_cpu import exact_bounds_hold

pytestmark = pytest.mark.gpu


def same(a, b):
    """np.array_equal with NaN == NaN, and the same sign on every zero."""
    a, b = np.asarray(a, dtype=np.float64), np.asarray(b, dtype=np.float64)
    return np.array_equal(a, b, equal_nan=True) and np.array_equal(np.signbit(a) | np.isnan(a), np.signbit(b) | np.isnan(b))


# ---------------------------------------------------------------- 1: the kernel alone
POOL = ("TS", "H", "U", "V", "Q", "CLOUD", "HICE", "ALBEDO", "OLR", "W_LAND", "UO", "VO", "PRECIP", "ETA")
PAIRS = (("U", "V"), ("UO", "VO"), ("TS", "H"))
SHAPES = [(5, 5), (6, 63), (7, 64), (9, 130), (9, 257), (10, 600)]


def entry_list(n):
    """n entries: planes of the pool in turn, every fourth entry a pair."""
    return [(1,) + PAIRS[(k // 4) % len(PAIRS)] if k % 4 == 3 else (0, POOL[k % len(POOL)], None) for k in range(n)]


def field_values(r, shape):
    """Mixed signs and magnitudes over eight orders; H holds one NaN, Q one +inf, CLOUD is all NaN, HICE is all -0.0, ALBEDO has
    a row of zeros of one sign, UO holds +inf and -inf in one row."""
    v = {name: r.normal(size=shape) * 10.0 ** r.integers(-4, 5, size=shape) for name in POOL}
    n = shape[0] * shape[1]
    v["H"].flat[n // 3] = np.nan
    v["Q"].flat[n // 2] = np.inf
    v["CLOUD"][:] = np.nan
    v["HICE"][:] = -0.0
    v["ALBEDO"][shape[0] // 2, :] = 0.0
    v["UO"][1, 0], v["UO"][1, shape[1] - 1] = np.inf, -np.inf
    return v


def host_plane(entry, v):
    op, a, b = entry
    if op == 0:
        return v[a]
    with np.errstate(all="ignore"):
        return np.sqrt(v[a] * v[a] + v[b] * v[b])


def reference_record(entries, v, lat, zonal):
    from qingdai_amd import series
    out = []
    for e in entries:
        mean, mn, mx, nan, z = series.reduce_reference(host_plane(e, v), lat)
        out.append(np.concatenate([[mean, mn, mx, float(nan)], z if zonal else []]))
    return np.concatenate(out)


@pytest.mark.parametrize("shape", SHAPES)
def test_kernel_alone(gpu, shape):
    import qingdai_amd as qa
    from qingdai_amd import series
    from qingdai_amd._lib import QdError
    from qingdai_amd.device import Device
    grid = qa.SphericalGrid(*shape)
    dev = Device(grid)
    lat = np.asarray(grid.lat, dtype=np.float64).reshape(-1)
    v = field_values(np.random.default_rng(shape[0] * 1000 + shape[1]), shape)
    for name, x in v.items():
        dev.upload_now(name, x)
    per_entry = {}                                           # entry -> its part of a record, whatever the configuration
    for n, zonal, order in ((1, 1, 1), (5, 1, 1), (5, 0, 1), (32, 1, 1), (32, 0, 1), (32, 1, -1), (1, 0, 1)):
        entries = entry_list(n)[::order]
        dev.series_configure(entries, zonal, series.row_weights(lat))
        dev.series_sample()
        recs = dev.series_log()
        width = series.record_width(n, shape[0], zonal)
        assert recs.shape == (1, width)
        want = reference_record(entries, v, lat, zonal)
        per = width // n
        for k, e in enumerate(entries):
            got, ref = recs[0, k * per:(k + 1) * per], want[k * per:(k + 1) * per]
            assert same(got, ref), (shape, n, zonal, order, k, e, got[:4], ref[:4])
            # the same planes in another configuration (entry count, order, zonal): the same bits
            assert same(got[:4], per_entry.setdefault((e, "stats"), got[:4].copy())), (shape, n, zonal, order, e)
            if zonal:
                assert same(got[4:], per_entry.setdefault((e, "zonal"), got[4:].copy())), (shape, n, zonal, order, e)
        assert len(dev.series_log()) == 0                        # drained
        if (n, zonal, order) == (5, 1, 1):                       # the a-priori bounds hold for what the device computed
            checked = 0
            for k, e in enumerate(entries):
                x = host_plane(e, v)
                if np.isfinite(x).all():
                    got = recs[0, k * per:(k + 1) * per]
                    assert got[3] == 0 and got[1] == x.min() and got[2] == x.max()
                    print(shape, e, exact_bounds_hold(x, lat, got[0], got[4:]))
                    checked += 1
            assert checked >= 2
        if n == 32:                                              # the special planes came through as the reference says
            stats = recs[0].reshape(n, per)[:, :4]
            by = {e: stats[k] for k, e in enumerate(entries)}
            assert np.isnan(by[(0, "CLOUD", None)][:3]).all() and by[(0, "CLOUD", None)][3] == shape[0] * shape[1]
            assert np.isnan(by[(0, "H", None)][0]) and by[(0, "H", None)][3] == 1 and np.isfinite(by[(0, "H", None)][1:3]).all()
            assert by[(0, "Q", None)][0] == np.inf and by[(0, "Q", None)][2] == np.inf and by[(0, "Q", None)][3] == 0
            assert np.isnan(by[(0, "UO", None)][0]) and by[(0, "UO", None)][1] == -np.inf and by[(0, "UO", None)][3] == 0
            assert by[(0, "HICE", None)][0] == 0.0 and not np.signbit(by[(0, "HICE", None)][0]) and np.signbit(by[(0, "HICE", None)][1])
            assert by[(1, "TS", "H")][3] == 1
    # two samples queue two records, oldest first; a reset forgets them
    dev.series_sample()
    dev.upload_now("TS", v["TS"] + 1.0)
    dev.series_sample()
    recs = dev.series_log()
    assert recs.shape[0] == 2 and same(recs[0], reference_record(entry_list(1), v, lat, 0))
    assert same(recs[1], reference_record(entry_list(1), {**v, "TS": v["TS"] + 1.0}, lat, 0))
    dev.series_sample()
    dev.series_reset()
    assert len(dev.series_log()) == 0
    dev.series_configure([], 0, None)                            # releases
    with pytest.raises(QdError, match="qd_series_sample: not configured"):
        dev.series_sample()
    dev.close()


# ---------------------------------------------------------------- 2: refusals
def test_refusals(gpu, monkeypatch):
    import qingdai_amd as qa
    from qingdai_amd import series
    from qingdai_amd._lib import SERIES_LOG_CAP, QdError
    from qingdai_amd.bands import BandGroup
    from qingdai_amd.device import Device
    grid = qa.SphericalGrid(5, 6)
    dev = Device(grid)
    w = series.row_weights(grid.lat)
    with pytest.raises(QdError, match="qd_series_configure: at most 32 entries"):
        dev.series_configure(entry_list(33), 1, w)
    with pytest.raises(QdError, match=r"qd_series_configure: unknown op \(0 = field a, 1 = sqrt\(a\*a \+ b\*b\)\)"):
        dev.series_configure([(2, "TS", None)], 1, w)
    with pytest.raises(QdError, match="qd_series_configure: op 1 cannot pair PRECIP with another field"):
        dev.series_configure([(1, "PRECIP", "U")], 1, w)
    with pytest.raises(QdError, match="qd_series_configure: field a is not an f64 plane"):
        dev.series_configure([(0, "LAND_MASK", None)], 1, w)
    for call in (dev.series_sample, dev.series_log, dev.series_reset, lambda: dev.series_schedule([1, 1])):
        with pytest.raises(QdError, match="not configured"):     # none of the refused calls left a configuration
            call()
    dev.close()
    grp = BandGroup(qa.SphericalGrid(73, 144), 2)
    with pytest.raises(QdError, match=r"need a whole-globe handle \(world == 1, n_rows == n_lat\); latitude bands are not supported"):
        grp.devs[0].series_configure([(0, "TS", None)], 1, series.row_weights(np.linspace(-90, 90, 73)))
    grp.close()
    # a span: the wrong schedule length, more samples than the log holds -- nothing runs
    sim = make(monkeypatch, 19, 36, routing=False)
    sim.dev.series_configure([(0, "TS", None)], 0, series.row_weights(sim.grid.lat))
    flags = dict(with_ocean=True, with_physics=True, pass_albedo=False, with_hydrology=True)
    counters = sim.dev.counters()
    stars = sim.forcing.star_table(DT * np.arange(SERIES_LOG_CAP + 1))
    sim.dev.series_schedule([1, 1, 1])
    with pytest.raises(QdError, match="a qd_series_schedule must cover exactly the n steps of the span"):
        sim.dev.step_n(stars[:2], DT, **flags)
    sim.dev.step_n(stars[:2], DT, **flags)                       # the refused span left no schedule behind
    assert sim.dev.counters()[0] == counters[0] + 2 and len(sim.dev.series_log()) == 0
    counters = sim.dev.counters()
    sim.dev.series_schedule(np.ones(SERIES_LOG_CAP + 1, dtype=np.int32))
    with pytest.raises(QdError, match="the span's series records would overflow the log of QD_SERIES_LOG_CAP"):
        sim.dev.step_n(stars, DT, **flags)
    assert sim.dev.counters() == counters and len(sim.dev.series_log()) == 0
    sim.dev.close()


def test_f32_map_is_refused_and_found_stale(gpu, monkeypatch):
    """A map the ecology keeps as f32 is no f64 plane: refused at configure; turned f32 behind a configure, found at span begin."""
    from qingdai_amd import series
    from qingdai_amd._lib import QdError
    from qingdai_amd.ecology import EcologyAdapter
    sim = make(monkeypatch, 19, 36, routing=False)               # no ecology yet: ECO_LAI is an f64 plane like any other
    w = series.row_weights(sim.grid.lat)
    sim.dev.series_configure([(0, "TS", None), (0, "ECO_LAI", None)], 1, w)
    monkeypatch.setenv("QD_ECO_DIAG", "0")
    eco = EcologyAdapter(sim.grid, sim.land_mask, dev=sim.dev, f32_maps=True)      # the handle's ecology, its maps as f32 slabs
    assert int(eco.params.map_f32) == 1
    counters = sim.dev.counters()
    stars = sim.forcing.star_table(DT * np.arange(2))
    sim.dev.series_schedule([1, 1])
    with pytest.raises(QdError, match=r"qd_step_n: a series field is no longer an f64 plane \(qd_series_configure again\)"):
        sim.dev.step_n(stars, DT, with_ocean=True, with_physics=True, pass_albedo=False, with_hydrology=True)
    with pytest.raises(QdError, match="qd_series_sample: a series field is no longer an f64 plane"):
        sim.dev.series_sample()
    assert sim.dev.counters() == counters and len(sim.dev.series_log()) == 0
    with pytest.raises(QdError, match="qd_series_configure: field a is not an f64 plane"):
        sim.dev.series_configure([(0, "ECO_LAI", None)], 1, w)
    sim.dev.close()


# ---------------------------------------------------------------- 3: a span equals single steps
def attach(sim, tmp_path, *, every=1, S=None, fields=None, zonal=True, lane=True):
    """A Series on the run's handle; lane=False: configured, but no participant of the spans (the class seam's twin)."""
    from qingdai_amd import series
    days = series.EVERY_DAYS if S is None else S * DT / sim.day_seconds
    cfg = {"enabled": True, "every": every, "zonal": zonal, "every_days": days, "fields": fields}
    sim.series_lines = []
    s = series.Series(sim.dev, sim.grid, cfg, with_ocean=sim.ocean is not None, dt=DT, day=sim.day_seconds, out=sim.series_lines.append,
                      output_dir=str(tmp_path))
    assert S is None or s.S == S
    sim.series = s if lane else None
    return s


@pytest.mark.parametrize("every", [1, 2])
def test_span_equals_single_steps(gpu, monkeypatch, tmp_path, every):
    got = []
    for cuts in ([6], [2, 4]):
        sim = make(monkeypatch, 19, 36, routing=False)
        s = attach(sim, tmp_path, every=every)
        assert len(s.names) == 23
        for n in cuts:
            sim.run_steps(n)
        recs, times, steps = s.window()
        assert steps.tolist() == list(range(0, 6, every)) and times.tolist() == [k * DT for k in range(0, 6, every)]
        got.append(recs)
        sim.dev.close()
    sim = make(monkeypatch, 19, 36, routing=False)
    s = attach(sim, tmp_path, every=every, lane=False)
    for i in range(6):
        sim.run_steps(1)
        if i % every == 0:
            sim.dev.series_sample()
    got.append(sim.dev.series_log())
    sim.dev.close()
    assert got[0].shape == (6 // every, 23 * (4 + 19))
    for k, r in enumerate(got[1:]):
        assert same(r, got[0]), (every, k)
    from qingdai_amd import series
    stats, zonal = series.split_records(got[0], 23, 19, True)
    assert np.isfinite(got[0]).all() and not stats[:, :, 3].any()
    p = s.names.index("PRECIP")                                  # liveness: a record is its own step's
    assert any(not np.array_equal(zonal[i, p], zonal[i + 1, p]) for i in range(6 // every - 1))
    assert not os.path.exists(tmp_path / "series") and sim.series_lines == []


# ---------------------------------------------------------------- 4: lazily stored diagnostics and PRECIP inside a span
def test_lazy_diagnostics_and_precip_are_the_steps_own(gpu, monkeypatch, tmp_path):
    """Device.step_n without the hydrology bit: inside a span only the last step stores OLR ... unless a reader comes with the
    span; and the next step's precipitation block overwrites PRECIP inside the ocean step.  The record of step s is the reduction
    of what Device.get returns behind a span that ends with s."""
    from qingdai_amd import series
    names = ["OLR", "PRECIP", "TS", "EFLUX"]
    flags = dict(with_ocean=True, with_physics=True, pass_albedo=False, with_hydrology=False)
    a = make(monkeypatch, 19, 36, routing=False)
    lat = np.asarray(a.grid.lat, dtype=np.float64).reshape(-1)
    stars = a.forcing.star_table(DT * np.arange(5))
    want = []
    for i in range(5):
        a.dev.step_n(stars[i:i + 1], DT, **flags)
        want.append(reference_record([(0, n, None) for n in names], fetch(a.dev, names), lat, True))
    a.dev.close()
    b = make(monkeypatch, 19, 36, routing=False)
    s = attach(b, tmp_path, fields=names)
    b.dev.step_n(stars, DT, series=s, **flags)
    recs = s.span_deliver(DT)
    assert recs.shape == (5, 4 * (4 + 19)) and s.i == 5
    for i in range(5):
        assert same(recs[i], want[i]), i
    per = 4 + 19
    for k in (0, 1):                                             # OLR and PRECIP move from step to step
        assert all(not np.array_equal(recs[i, k * per:(k + 1) * per], recs[i + 1, k * per:(k + 1) * per]) for i in range(4)), names[k]
    b.dev.close()


# ---------------------------------------------------------------- 5: the other lanes and the state do not notice
FIRES = {0: 3, 2: 1, 5: 3}


def test_no_effect_on_the_other_lanes(gpu, monkeypatch, tmp_path):
    from qingdai_amd import ncio
    from test_gpu_history import attach as attach_history
    runs = {}
    for on in (False, True):
        out = tmp_path / ("on" if on else "off")
        sim = make(monkeypatch, 19, 36, fires=FIRES)
        assert sim.routing is not None and sim.budget is not None
        attach_history(sim, out, S=4)
        if on:
            attach(sim, out, S=3)
        sim.dev.timing(True)
        for n in (3, 4):
            sim.run_steps(n)
        sim.dev.sync()
        launches = sim.dev.timing_get("series")[1]
        sim.dev.timing(False)
        files = sorted(os.listdir(out / "history"))
        runs[on] = dict(files=files, arrays=[ncio.read_nc(str(out / "history" / f))[0] for f in files], sums=sim.dev.history_read(),
                        budget=list(sim.budget_lines), history=list(sim.history_lines), digest=sim.digest(), launches=launches,
                        series=sorted(os.listdir(out / "series")) if os.path.exists(out / "series") else None)
        sim.dev.close()
    off, on = runs[False], runs[True]
    assert off["launches"] == 0 and off["series"] is None        # at 0: no series scope in the timing tables, no directory
    assert on["launches"] == 2 * 7 and len(on["series"]) == 2    # PRECIP's group and the others', every step; windows 0-2 and 3-5
    assert on["files"] == off["files"] and len(off["files"]) == 1
    for va, vb in zip(on["arrays"], off["arrays"]):
        assert va.keys() == vb.keys() and all(np.asarray(va[k]).tobytes() == np.asarray(vb[k]).tobytes() for k in va)
    assert on["sums"][1] == off["sums"][1] == 3 and on["sums"][0].tobytes() == off["sums"][0].tobytes()
    assert on["budget"] == off["budget"] and len(off["budget"]) > 0 and on["history"] == off["history"]
    assert on["digest"] == off["digest"] and len(off["digest"]) > 20


# ---------------------------------------------------------------- 6: the driver
def _set_env(monkeypatch, env):
    for k in [k for k in os.environ if k.startswith("QD_")]:
        monkeypatch.delenv(k)
    for k, v in env.items():
        monkeypatch.setenv(k, str(v))


def test_driver_main(gpu, tmp_path, monkeypatch, capsys):
    from qingdai_amd import driver, ncio, series
    env = {"QD_N_LAT": "19", "QD_N_LON": "36", "QD_SIM_DAYS": "0.125", "QD_ECO_ENABLE": "0", "QD_DYN_DIAG_PRINT": "0", "QD_USE_OCEAN": "1",
           "QD_HYDRO_ENABLE": "0", "QD_SERIES": "1", "QD_SERIES_EVERY_DAYS": "0.05", "QD_SERIES_EVERY": "2"}
    _set_env(monkeypatch, env)
    on = tmp_path / "on"
    on.mkdir()
    monkeypatch.chdir(on)
    assert driver.main() == 0
    out = capsys.readouterr().out
    day = 72000.0
    lines = [s for s in out.splitlines() if s.startswith("[Series]")]
    assert len(lines) == 3 and [int(re.search(r": (\d+) samples", s).group(1)) for s in lines] == [6, 6, 3], out
    assert all(re.fullmatch(r"\[Series\] day \d+\.\d+–\d+\.\d+: \d+ samples \| TS=\S+→\S+ H=\S+→\S+ U=\S+→\S+ V=\S+→\S+ Q=\S+→\S+ CLOUD=\S+→\S+", s)
               for s in lines), lines
    files = sorted(os.listdir(on / "output" / "series"))
    assert len(files) == 3 and all(re.fullmatch(r"series_day_\d+\.\d+_\d+\.\d+\.nc", f) for f in files), files
    names = [n.lower() for n in series.history.resolve_fields(None, True)]
    first_ts = []
    for f, (steps, complete) in zip(files, ((range(0, 12, 2), 1), (range(12, 24, 2), 1), (range(24, 30, 2), 0))):
        v, _ = ncio.read_nc(str(on / "output" / "series" / f))
        steps = list(steps)
        assert v["step"].tolist() == steps and v["time_seconds"].tolist() == [k * DT for k in steps], f
        assert (int(v["complete"]), int(v["sample_every"]), int(v["zonal"]), float(v["dt_seconds"])) == (complete, 2, 1, DT)
        a, b = (float(x) for x in re.fullmatch(r"series_day_(.+)_(.+)\.nc", f).groups())
        assert abs(a - steps[0] * DT / day) <= 0.005 and abs(b - steps[-1] * DT / day) <= 0.005, f
        assert v["lat"].shape == (19,) and set(v) == ({"time_seconds", "step", "lat", "dt_seconds", "sample_every", "zonal", "complete"} |
                                                      {f"{n}_{q}" for n in names for q in ("mean", "min", "max", "nan", "zonal")})
        for n in names:
            assert v[f"{n}_mean"].shape == (len(steps),) and v[f"{n}_zonal"].shape == (len(steps), 19) and not v[f"{n}_nan"].any(), n
            # a weighted mean lies between the extrema, up to its rounding: gamma_{36 + 2 * 19 + 4} = 78 * 2^-53 of the largest |x|
            slack = 78 * 2.0 ** -52 * np.maximum(np.abs(v[f"{n}_min"]), np.abs(v[f"{n}_max"]))
            assert np.isfinite(v[f"{n}_zonal"]).all() and (v[f"{n}_min"] - slack <= v[f"{n}_mean"]).all(), n
            assert (v[f"{n}_mean"] <= v[f"{n}_max"] + slack).all(), n
        assert (v["ts_mean"] > 200.0).all() and (v["ts_mean"] < 330.0).all()
        first_ts.append(float(v["ts_mean"][0]))
    assert len(set(first_ts)) == 3
    # the same run without the switch: no directory, no line
    monkeypatch.delenv("QD_SERIES")
    off = tmp_path / "off"
    off.mkdir()
    monkeypatch.chdir(off)
    assert driver.main() == 0
    assert "[Series]" not in capsys.readouterr().out and not os.path.exists(off / "output" / "series")


# ---------------------------------------------------------------- 7: stopped inside a window and resumed
def test_resumed_run_writes_the_uncut_runs_files(gpu, tmp_path, monkeypatch, capsys):
    from qingdai_amd import driver, ncio

    def env(data, days, **extra):
        e = {"QD_N_LAT": "19", "QD_N_LON": "36", "QD_DT_SECONDS": "300", "QD_SIM_DAYS": str(days), "QD_DYN_DIAG_PRINT": "0", "QD_ECO_ENABLE": "0",
             "QD_HYDRO_ENABLE": "0", "QD_USE_OCEAN": "1", "QD_DATA_DIR": str(tmp_path / data), "QD_OUTPUT_DIR": str(tmp_path / ("out_" + data)),
             "QD_SERIES": "1", "QD_SERIES_EVERY_DAYS": "0.05", "QD_SERIES_FIELDS": "TS,PRECIP,OLR,WIND_SPEED,SST", "QD_CHECKPOINT": "1"}
        e.update(extra)
        return e
    monkeypatch.chdir(tmp_path)
    _set_env(monkeypatch, env("whole", 0.125))                   # 30 steps: windows 0-11 and 12-23, 24-29 stays open
    assert driver.main() == 0
    whole = capsys.readouterr().out
    assert whole.count("[Series] day ") == 2 and " 30 steps" in whole and "[Checkpoint] (final) wrote" in whole
    _set_env(monkeypatch, env("cut", 0.0625))                    # 15 steps: stopped inside the window 12-23
    assert driver.main() == 0
    first = capsys.readouterr().out
    assert first.count("[Series] day ") == 1 and " 15 steps" in first and "[Checkpoint] loaded" not in first
    assert driver.main() == 0
    second = capsys.readouterr().out
    assert "[Checkpoint] loaded" in second and "step 15" in second and second.count("[Series] day ") == 1      # each file written once
    files = lambda d: sorted(os.listdir(tmp_path / ("out_" + d) / "series"))
    assert files("cut") == files("whole") and len(files("whole")) == 2
    for name in files("whole"):
        va, vb = (ncio.read_nc(str(tmp_path / ("out_" + d) / "series" / name))[0] for d in ("whole", "cut"))
        assert va.keys() == vb.keys() and all(np.asarray(va[k]).tobytes() == np.asarray(vb[k]).tobytes() for k in va), name
        assert int(va["complete"]) == 1 and len(va["step"]) == 12
    wa, wb = (ncio.read_nc(str(tmp_path / d / "checkpoint.nc")) for d in ("whole", "cut"))
    assert wa[1]["run_digest"] == wb[1]["run_digest"]
    for k in ("series_records", "series_times", "series_steps", "series_clock"):     # the open window 24-29 travels in the file
        assert np.asarray(wa[0][k]).tobytes() == np.asarray(wb[0][k]).tobytes(), k
    assert wa[0]["series_clock"].tolist() == [30.0, 6.0] and wa[0]["series_steps"].tolist() == [24.0, 25.0, 26.0, 27.0, 28.0, 29.0]
    assert "series=TS,PRECIP,OLR,WIND_SPEED,SST|zonal=1|every=1" in wa[1]["subsystems"]
    # another series configuration, or none: refused with the subsystem wording
    _set_env(monkeypatch, env("cut", 0.0625, QD_SERIES_ZONAL="0"))
    assert driver.main() == 2
    assert "the subsystem set differs: the series lane is 'TS,PRECIP,OLR,WIND_SPEED,SST|zonal=1|every=1' in the file and " \
           "'TS,PRECIP,OLR,WIND_SPEED,SST|zonal=0|every=1' in this run" in capsys.readouterr().out
    _set_env(monkeypatch, env("cut", 0.0625, QD_SERIES="0"))
    assert driver.main() == 2
    assert "the subsystem set differs: the series lane is 'TS,PRECIP,OLR,WIND_SPEED,SST|zonal=1|every=1' in the file and '-' in this run" \
           in capsys.readouterr().out
