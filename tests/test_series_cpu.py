"""CPU (-m "not gpu"): the host side of the per-step series lane (qingdai_amd/series.py) and the header's declarations.

reduce_reference restates the kernel's summation order in NumPy; here it is held against exact arithmetic (fractions) with the
standard a-priori bounds of floating-point summation, u = 2^-53, gamma_k = k u / (1 - k u):
    |zonal_j - exact| <= gamma_{n_lon} sum_i |x_ji| / n_lon
    |mean - exact|    <= gamma_{n_lon + 2 n_lat + 4} sum_ji w_j |x_ji| / (n_lon W)
(a sum of n terms in ANY order errs by at most gamma_{n-1} sum |x|; the products w_j S_j, the sum W, the product n_lon W and the
divisions add one rounding each).  The bounds are derived, not tuned: a failure means the order is wrong."""
import os
import re
from fractions import Fraction

import numpy as np
import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
U = Fraction(1, 2 ** 53)
SHAPES = [(5, 5), (6, 63), (7, 64), (9, 130), (9, 257), (10, 600), (70, 36)]


def gamma(k):
    return k * U / (1 - k * U)


def lat_of(n_lat):
    return np.linspace(-90.0, 90.0, n_lat)


def wide_plane(r, shape):
    """Finite, mixed signs, magnitudes over twelve orders."""
    return r.normal(size=shape) * 10.0 ** r.integers(-6, 7, size=shape)


def exact_bounds_hold(plane, lat, mean, zonal):
    """The two fsum bounds of the module docstring, in exact rational arithmetic -> (worst zonal ratio, mean ratio), each <= 1."""
    from qingdai_amd import series
    n_lat, n_lon = plane.shape
    w = [Fraction(float(x)) for x in series.row_weights(lat)]
    X = [[Fraction(float(x)) for x in row] for row in plane]
    W = sum(w)
    worst = Fraction(0)
    for j in range(n_lat):
        exact = sum(X[j]) / n_lon
        bound = gamma(n_lon) * sum(abs(x) for x in X[j]) / n_lon
        err = abs(Fraction(float(zonal[j])) - exact)
        assert err <= bound, (j, float(err), float(bound))
        if bound:
            worst = max(worst, err / bound)
    exact = sum(w[j] * sum(X[j]) for j in range(n_lat)) / (n_lon * W)
    bound = gamma(n_lon + 2 * n_lat + 4) * sum(w[j] * sum(abs(x) for x in X[j]) for j in range(n_lat)) / (n_lon * W)
    err = abs(Fraction(float(mean)) - exact)
    assert err <= bound, (float(err), float(bound))
    return float(worst), float(err / bound) if bound else 0.0


# ---------------------------------------------------------------- reduce_reference
@pytest.mark.parametrize("shape", SHAPES)
def test_reference_against_exact_arithmetic(shape):
    from qingdai_amd import series
    r = np.random.default_rng(shape[0] * 1000 + shape[1])
    lat = lat_of(shape[0])
    for _ in range(3):
        x = wide_plane(r, shape)
        mean, mn, mx, nan, zonal = series.reduce_reference(x, lat, shape[1])
        assert (mn, mx, nan) == (float(x.min()), float(x.max()), 0) and zonal.shape == (shape[0],)
        print(shape, exact_bounds_hold(x, lat, mean, zonal))


def test_reference_order_is_the_documented_one():
    """Spelled out with Python floats for one row of 300 cells and 70 rows: lane l owns 128 k + 2 l and 128 k + 2 l + 1."""
    from qingdai_amd import series
    r = np.random.default_rng(7)
    n_lat, n_lon = 70, 300
    x, lat = wide_plane(r, (n_lat, n_lon)), lat_of(n_lat)

    def wave(v):
        v = list(v)
        o = 32
        while o:
            for l in range(o):
                v[l] = v[l] + v[l + o]
            o //= 2
        return v[0]
    S = []
    for j in range(n_lat):
        acc = [0.0] * 64
        for l in range(64):
            k = 0
            while 128 * k + 2 * l < n_lon:
                for c in (128 * k + 2 * l, 128 * k + 2 * l + 1):
                    if c < n_lon:
                        acc[l] = acc[l] + float(x[j, c])
                k += 1
        S.append(wave(acc))
    w = [float(v) for v in series.row_weights(lat)]
    num, W = [0.0] * 64, [0.0] * 64
    for l in range(64):
        for j in range(l, n_lat, 64):
            num[l] = num[l] + w[j] * S[j]
            W[l] = W[l] + w[j]
    mean, _, _, _, zonal = series.reduce_reference(x, lat, n_lon)
    assert mean == wave(num) / (float(n_lon) * wave(W))
    assert zonal.tolist() == [s / float(n_lon) for s in S]


def test_reference_special_values():
    from qingdai_amd import series
    lat = lat_of(6)
    x = np.arange(36.0).reshape(6, 6) - 10.0
    x[2, 3] = np.nan
    mean, mn, mx, nan, zonal = series.reduce_reference(x, lat)
    assert np.isnan(mean) and nan == 1 and (mn, mx) == (-10.0, 25.0)
    assert np.isnan(zonal[2]) and np.isfinite(np.delete(zonal, 2)).all()
    x[2, 3] = np.inf
    mean, mn, mx, nan, zonal = series.reduce_reference(x, lat)
    assert mean == np.inf and zonal[2] == np.inf and mx == np.inf and mn == -10.0 and nan == 0
    x[2, 4] = -np.inf                                            # inf - inf in one row
    mean, mn, mx, nan, zonal = series.reduce_reference(x, lat)
    assert np.isnan(mean) and np.isnan(zonal[2]) and (mn, mx, nan) == (-np.inf, np.inf, 0)
    mean, mn, mx, nan, zonal = series.reduce_reference(np.full((6, 6), np.nan), lat)
    assert np.isnan([mean, mn, mx]).all() and nan == 36 and np.isnan(zonal).all()
    mean, mn, mx, nan, zonal = series.reduce_reference(np.full((6, 6), -0.0), lat)       # the accumulators start at +0.0
    assert mean == 0.0 and not np.signbit(mean) and not np.signbit(zonal).any() and np.signbit(mn) and np.signbit(mx)
    with pytest.raises(ValueError, match="n_lon is 7"):
        series.reduce_reference(x, lat, 7)
    assert np.array_equal(series.row_weights(lat), np.maximum(np.cos(np.deg2rad(lat)), 0.0))


# ---------------------------------------------------------------- environment, clock
def test_read_env():
    from qingdai_amd import series
    d = series.read_env({})
    assert d == {"enabled": False, "every": 1, "zonal": True, "every_days": 10.0, "fields": None}
    d = series.read_env({"QD_SERIES": "1", "QD_SERIES_EVERY": "3", "QD_SERIES_ZONAL": "0", "QD_SERIES_EVERY_DAYS": "0.5",
                         "QD_SERIES_FIELDS": " ts, wind_speed ,PRECIP"})
    assert d == {"enabled": True, "every": 3, "zonal": False, "every_days": 0.5, "fields": ["TS", "WIND_SPEED", "PRECIP"]}
    for bad in ("x", "", "0", "-2", "1.5"):
        assert series.read_env({"QD_SERIES": "1", "QD_SERIES_EVERY": bad})["every"] == 1, bad
    for bad in ("x", "0", "-1", "nan", "inf"):
        assert series.read_env({"QD_SERIES": "1", "QD_SERIES_EVERY_DAYS": bad})["every_days"] == 10.0, bad
    for off in ("0", "2", "yes", ""):
        assert series.read_env({"QD_SERIES": off})["enabled"] is False, off
    assert series.read_env({"QD_SERIES": "1", "QD_SERIES_ZONAL": "x"})["zonal"] is True
    with pytest.raises(ValueError, match=r"QD_SERIES_FIELDS: unknown field 'NOPE'"):
        series.read_env({"QD_SERIES": "1", "QD_SERIES_FIELDS": "TS,NOPE"})
    with pytest.raises(ValueError, match=r"QD_SERIES_FIELDS: 33 entries, at most 32"):
        series.read_env({"QD_SERIES": "1", "QD_SERIES_FIELDS": ",".join(["TS"] * 33)})
    assert series.read_env({"QD_SERIES": "0", "QD_SERIES_FIELDS": "NOPE"})["fields"] is None       # off: the list is not looked at
    assert series.from_env(None, None, {"QD_SERIES": "0"}) is None and series.from_env(None, None, {}) is None
    # history's own messages keep its variable's name
    from qingdai_amd import history
    with pytest.raises(ValueError, match=r"QD_HISTORY_FIELDS: unknown field 'NOPE'"):
        history.parse_fields("NOPE")
    with pytest.raises(ValueError, match=r"QD_SERIES_FIELDS: field 'SST' needs the ocean"):
        history.resolve_fields(["SST"], False, var=series.FIELDS_VAR)


class FakeDev:
    """What a Series asks of a Device, recorded; series_log hands back rows that carry their own number."""

    def __init__(self, omega=2.0 * np.pi / 72000.0):
        import types
        self.params = types.SimpleNamespace(omega=omega)
        self.configured, self.scheduled, self.queue = None, [], []

    def series_configure(self, entries, zonal, w_row):
        self.configured = (list(entries), bool(zonal), np.array(w_row))

    def series_schedule(self, flags):
        self.scheduled.append(np.array(flags))

    def series_log(self, max_records=None):
        out, self.queue = self.queue, []
        assert max_records is None or len(out) <= max_records
        return np.array(out).reshape(len(out), -1) if out else np.empty((0, 1))


def make_series(tmp_path, *, S=4, every=1, zonal=True, fields=("TS", "WIND_SPEED"), n_lat=5, lines=None):
    import types
    from qingdai_amd import series
    dev = FakeDev()
    grid = types.SimpleNamespace(lat=lat_of(n_lat), n_lat=n_lat)
    cfg = {"enabled": True, "every": every, "zonal": zonal, "every_days": S * 300.0 / 72000.0, "fields": list(fields)}
    s = series.Series(dev, grid, cfg, with_ocean=True, dt=300.0, day=72000.0, out=(lines if lines is not None else []).append,
                      output_dir=str(tmp_path))
    assert s.S == S
    return s, dev


def run_span(s, dev, n, t0=None):
    """The span protocol as Device.step_n and the driver walk it; the fake device queues one record per sampled step."""
    k = s.span_schedule(t0, 300.0, n)
    for step in k[2]:
        dev.queue.append(np.full(s.width, float(step)))
    s._fired(k)
    return s.span_deliver(300.0)


def test_schedule_and_window_clock_are_historys(tmp_path):
    from qingdai_amd import history
    s, dev = make_series(tmp_path, S=5, every=2)
    assert dev.configured[0] == [(0, "TS", None), (1, "U", "V")] and dev.configured[1] is True
    assert np.array_equal(dev.configured[2], np.maximum(np.cos(np.deg2rad(lat_of(5))), 0.0))
    assert s.width == 2 * (4 + 5)
    i = 0
    for n in (3, 1, 4, 7, 2):
        assert s.steps_to_window_end() == 5 - i % 5
        clock = s.span_clock()
        k = s.span_schedule(None, 300.0, n)
        assert np.array_equal(dev.scheduled[-1], history.schedule(i, n, 5, 2)) and dev.scheduled[-1].dtype == np.int32
        assert k[0] == n and np.array_equal(k[2], i + np.flatnonzero(history.schedule(i, n, 5, 2)))
        assert np.array_equal(k[1], k[2] * 300.0)
        s.span_restore(clock)                                    # a refused span: the clock stays
        assert s.i == i and s.span_clock() == clock
        recs = run_span(s, dev, n)
        i += n
        assert s.i == i and len(recs) == int(history.schedule(i - n, n, 5, 2).sum()) and s.window_closed() == (i % 5 == 0)
    recs, times, steps = s.window()
    want = np.flatnonzero(history.schedule(0, 17, 5, 2))
    assert np.array_equal(steps, want) and np.array_equal(times, want * 300.0) and np.array_equal(recs[:, 0], want.astype(float))
    # the span's own times win over the step index
    s2, dev2 = make_series(tmp_path, S=5)
    run_span(s2, dev2, 3, t0=1000.0)
    run_span(s2, dev2, 2, t0=np.array([5000.0, 5300.0]))
    assert s2.window()[1].tolist() == [1000.0, 1300.0, 1600.0, 5000.0, 5300.0] and s2.window()[2].tolist() == [0, 1, 2, 3, 4]
    k = s2.span_schedule(None, 300.0, 1)                         # a sampled step whose record never came
    s2._fired(k)
    with pytest.raises(RuntimeError, match="the device log held 0 records where the schedule says 1"):
        s2.span_deliver(300.0)


# ---------------------------------------------------------------- the file
@pytest.mark.parametrize("zonal", [True, False])
def test_window_file(tmp_path, zonal):
    from qingdai_amd import ncio, series
    lines = []
    s, dev = make_series(tmp_path, S=4, zonal=zonal, lines=lines)
    n_lat, width = 5, s.width
    assert width == 2 * (4 + (5 if zonal else 0))
    r = np.random.default_rng(3)
    recs = r.normal(size=(4, width))
    per = width // 2
    recs[:, 3], recs[:, per + 3] = [0, 2, 0, 7], [1, 0, 0, 0]
    k = s.span_schedule(1200.0, 300.0, 4)
    dev.queue = list(recs)
    s._fired(k)
    s.span_deliver(300.0)
    assert s.window_closed()
    path = s.flush()
    assert path == str(tmp_path / "series" / "series_day_00.02_00.03.nc") and s.files == [path] and not os.path.exists(path + ".part")
    assert os.listdir(tmp_path / "series") == ["series_day_00.02_00.03.nc"]
    v, _ = ncio.read_nc(path)
    want = {"time_seconds", "step", "lat", "dt_seconds", "sample_every", "zonal", "complete"}
    for name in ("ts", "wind_speed"):
        want |= {f"{name}_mean", f"{name}_min", f"{name}_max", f"{name}_nan"} | ({f"{name}_zonal"} if zonal else set())
    assert set(v) == want
    i8 = np.int64 if ncio.backend() == "netCDF4" else np.float64        # classic NetCDF has no 64-bit integer
    assert v["time_seconds"].dtype == np.float64 and v["time_seconds"].tolist() == [1200.0, 1500.0, 1800.0, 2100.0]
    assert v["step"].dtype == i8 and v["step"].tolist() == [0, 1, 2, 3]
    assert np.array_equal(v["lat"], lat_of(5)) and v["lat"].dtype == np.float64
    for e, name in enumerate(("ts", "wind_speed")):
        for q, stat in enumerate(("mean", "min", "max")):
            assert v[f"{name}_{stat}"].dtype == np.float64 and v[f"{name}_{stat}"].tobytes() == recs[:, e * per + q].tobytes()
        assert v[f"{name}_nan"].dtype == np.int32 and v[f"{name}_nan"].tolist() == recs[:, e * per + 3].astype(int).tolist()
        if zonal:
            assert v[f"{name}_zonal"].shape == (4, n_lat) and v[f"{name}_zonal"].tobytes() == recs[:, e * per + 4:(e + 1) * per].tobytes()
    assert (float(v["dt_seconds"]), int(v["sample_every"]), int(v["zonal"]), int(v["complete"])) == (300.0, 1, int(zonal), 1)
    assert len(lines) == 1
    m = re.fullmatch(r"\[Series\] day 0\.02–0\.03: 4 samples \| TS=(\S+)→(\S+) WIND_SPEED=(\S+)→(\S+)", lines[0])
    assert m and [float(g) for g in m.groups()] == [float(f"{x:.6g}") for x in (recs[0, 0], recs[3, 0], recs[0, per], recs[3, per])]
    # the window is gone; an open one is written with complete = 0, an empty one not at all
    assert s.flush() is None and len(s.window()[0]) == 0
    k = s.span_schedule(2400.0, 300.0, 2)
    dev.queue = list(recs[:2])
    s._fired(k)
    s.span_deliver(300.0)
    assert not s.window_closed() and s.steps_to_window_end() == 2
    v, _ = ncio.read_nc(s.flush(complete=0))
    assert int(v["complete"]) == 0 and v["step"].tolist() == [4, 5] and len(lines) == 2


def test_only_six_entries_in_the_line_and_restore_window(tmp_path):
    lines = []
    names = ("TS", "H", "U", "V", "Q", "CLOUD", "HICE", "OLR")
    s, dev = make_series(tmp_path, S=3, zonal=False, fields=names, lines=lines)
    run_span(s, dev, 2)
    recs, times, steps = s.window()
    t, dev2 = make_series(tmp_path, S=3, zonal=False, fields=names, lines=lines)
    t.restore_window(recs, times, steps, s.i)
    assert t.i == 2 and all(np.array_equal(a, b) for a, b in zip(t.window(), s.window()))
    run_span(t, dev2, 1)
    assert t.window_closed() and t.flush() is not None
    assert lines[0].count("=") == 6 and " HICE=" not in lines[0] and ": 3 samples | TS=0→2 " in lines[0]


# ---------------------------------------------------------------- the header
def test_header_declares_the_series_abi():
    from qingdai_amd import _lib
    text = open(os.path.join(ROOT, "include", "qingdai_hip.h"), encoding="utf-8").read()
    assert (_lib.C["QD_SERIES_MAX_ENTRIES"], _lib.C["QD_SERIES_LOG_CAP"], _lib.C["QD_SERIES_STATS"]) == (32, 256, 4)
    assert _lib.C["QD_ABI_VERSION"] == 1 and _lib.C["QD_SERIES_LOG_CAP"] > 200          # the driver's longest chunk
    sig = {name: [(p[0], p[2]) for p in _lib.SIGNATURES[name]][1:] for name in _lib.SYMBOLS if name.startswith("qd_series_")}
    assert sig == {
        "qd_series_configure": [("n", "int"), ("op", "int32_t"), ("a", "int32_t"), ("b", "int32_t"), ("zonal", "int"), ("w_row", "double")],
        "qd_series_schedule": [("steps", "int"), ("sample", "int32_t")],
        "qd_series_sample": [],
        "qd_series_log": [("out", "double"), ("max", "int"), ("n", "int")],
        "qd_series_reset": []}
    for name in sig:                                             # each with a comment on its line
        assert re.search(r"^int " + name + r"\(.*\);\s*/\*.+\*/\s*$", text, re.M), name
    for macro in ("QD_SERIES_MAX_ENTRIES", "QD_SERIES_LOG_CAP", "QD_SERIES_STATS"):
        assert re.search(r"^#define " + macro + r" \d+\s*/\*.+\*/\s*$", text, re.M), macro
