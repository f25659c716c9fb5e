"""CPU (-m "not gpu"): the host side of the zonal spectra lane (qingdai_amd/spectra.py) and the header's declarations.

dft_reference is the definition P(k) = c_k |X(k)|^2 / n^2 in extended precision (u_e = 2^-64 on x87 long double, 2^-80 through
mpmath).  It is held against np.fft.rfft (pocketfft, f64) with the a-priori bound the device test uses, u = 2^-53,
gamma_m = m u / (1 - m u):
    a bin of a DFT is a sum of n products x_i w_i with |w_i| = 1.  Summed in ANY order (a tree, an FFT's butterflies, with or without
    FMA contraction) with each w_i taken from a table correct within 2u, every path from x_i to the result carries at most n - 1
    additions, one product and the table's error: Re X and Im X each err by at most E = gamma_{n+3} sum_i |x_i|.  Then
    |X^|^2 - |X|^2 = 2 (Re X dRe + Im X dIm) + dRe^2 + dIm^2 <= 2 (|Re X| + |Im X|) E + 2 E^2, and the two squares, their sum, the
    factor c_k (exact) and the division by n^2 (exact in f64 for the grids here) add at most four roundings of the result, within
    8u P with room for the reference's own rounding to f64:
        |P^ - P| <= (c_k / n^2) (2 (|Re X| + |Im X|) E + 2 E^2) + 8 u P.
The bound is derived, not tuned: a misplaced bin or a wrong twiddle misses it by many orders of magnitude."""
import os
import re

import numpy as np
import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
U = 2.0 ** -53


def lat_of(n_lat):
    return np.linspace(-90.0, 90.0, n_lat)


def power_bound(x, P, re, im):
    """The bound of the module docstring for rows x [n_lat][n] and their reference P, Re X, Im X -> [n_lat][n_bins]."""
    from qingdai_amd import spectra
    n = x.shape[-1]
    m = n + 3
    E = (m * U / (1.0 - m * U)) * np.abs(x).sum(axis=-1, keepdims=True)
    return spectra.bin_weights(n) / float(n * n) * (2.0 * (np.abs(re) + np.abs(im)) * E + 2.0 * E * E) + 8.0 * U * P


# ---------------------------------------------------------------- dft_reference
@pytest.mark.parametrize("n", [1, 2, 5, 60, 63, 64, 125, 257, 360])
def test_reference_against_rfft(n):
    from qingdai_amd import spectra
    r = np.random.default_rng(n)
    x = r.normal(size=(3, n)) * 10.0 ** r.integers(-3, 4, size=(3, n))
    P, re, im = spectra.dft_reference(x, parts=True)
    assert P.shape == (3, n // 2 + 1) and P.dtype == np.float64
    X = np.fft.rfft(x, axis=1)
    got = spectra.bin_weights(n) * (X.real ** 2 + X.imag ** 2) / float(n * n)
    bound = power_bound(x, P, re, im)
    assert (np.abs(got - P) <= bound).all(), float((np.abs(got - P) / bound).max())
    assert np.allclose(re, X.real, rtol=0, atol=1e-12 * np.abs(x).sum()) and np.allclose(im, X.imag, rtol=0, atol=1e-12 * np.abs(x).sum())
    # one row in, one row out
    assert np.array_equal(spectra.dft_reference(x[1]), P[1])


@pytest.mark.parametrize("n", [5, 8, 60, 63, 72, 130])
def test_reference_exact_rows_and_parseval(n):
    from qingdai_amd import spectra
    kN = n // 2
    i = np.arange(n)
    tiny = 1e-30                                                 # (2^-64 n)^2: what extended precision leaves in an empty bin
    P = spectra.dft_reference(np.full(n, 3.0))
    assert abs(P[0] - 9.0) <= 1e-15 and (P[1:] <= tiny).all()             # a constant row has only bin 0
    for m in sorted({1, max(1, kN - 1), kN}):
        P = spectra.dft_reference(np.cos(2.0 * np.pi * m * i / n))
        want = 1.0 if (n % 2 == 0 and m == kN) else 0.5          # cos(pi i) is the alternating row: all of its variance, 1
        assert abs(P[m] - want) <= 1e-14, (m, P[m])
        assert (np.delete(P, m) <= 1e-28).all(), (m, np.delete(P, m).max())       # (the f64 rounding of the cosine itself)
    if n % 2 == 0:
        P = spectra.dft_reference(np.where(i % 2 == 0, 2.0, -2.0))
        assert P[kN] == 4.0 and (P[:kN] <= tiny).all()            # the alternating row has bin n / 2 alone
    r = np.random.default_rng(n)
    x = r.normal(size=(4, n)) * 10.0 ** r.integers(-2, 3, size=(4, 1))
    P = spectra.dft_reference(x)
    ms = (x.astype(np.longdouble) ** 2).mean(axis=1).astype(np.float64)
    assert np.allclose(P.sum(axis=1), ms, rtol=(kN + 4) * U * 2, atol=0.0)          # Parseval
    x[2, n // 2] = np.nan
    x[0, 0] = np.inf
    Q = spectra.dft_reference(x)
    assert np.isnan(Q[[0, 2]]).all() and np.array_equal(Q[[1, 3]], P[[1, 3]])


def test_combine_reference_order_is_the_documented_one():
    """Spelled out with Python floats for 150 rows: lane l takes the rows l, l + 64, ... and then the five halvings."""
    from qingdai_amd import series, spectra
    r = np.random.default_rng(11)
    n_lat, nb = 150, 7
    P, lat = np.abs(r.normal(size=(n_lat, nb))) * 10.0 ** r.integers(-6, 7, size=(n_lat, nb)), lat_of(n_lat)
    w = [float(v) for v in series.row_weights(lat)]

    def wave(v):
        v = list(v)
        o = 32
        while o:
            for l in range(o):
                v[l] = v[l] + v[l + o]
            o //= 2
        return v[0]
    want = []
    for k in range(nb):
        num, W = [0.0] * 64, [0.0] * 64
        for l in range(64):
            for j in range(l, n_lat, 64):
                num[l] = num[l] + w[j] * float(P[j, k])
                W[l] = W[l] + w[j]
        want.append(wave(num) / wave(W))
    got = spectra.combine_reference(P, lat)
    assert got.tolist() == want
    P[3] = np.nan
    assert np.isnan(spectra.combine_reference(P, lat)).all()
    with pytest.raises(ValueError, match="one latitude per row"):
        spectra.combine_reference(P, lat[:-1])


def test_hi_frac():
    from qingdai_amd import spectra
    P = np.arange(10.0)                                          # kN = 9: k >= ceil(6.75) = 7
    assert spectra.hi_frac(P) == (7 + 8 + 9) / 45.0
    P2 = np.stack([P, np.zeros(10), np.r_[5.0, np.zeros(9)]])
    got = spectra.hi_frac(P2)
    assert got[0] == (7 + 8 + 9) / 45.0 and np.isnan(got[1]) and np.isnan(got[2])
    assert spectra.hi_frac(np.array([1.0, 2.0])) == 1.0         # kN = 1: the band is bin 1
    assert np.isnan(spectra.hi_frac(np.array([1.0])))            # kN = 0: no band
    assert spectra.hi_frac(np.ones(5)) == 2.0 / 4.0              # kN = 4: k >= 3


# ---------------------------------------------------------------- environment
def test_read_env():
    from qingdai_amd import spectra
    d = spectra.read_env({})
    assert d == {"enabled": False, "every": 24, "lat": True, "every_days": 10.0, "fields": None}
    d = spectra.read_env({"QD_SPECTRA": "1", "QD_SPECTRA_EVERY": "3", "QD_SPECTRA_LAT": "0", "QD_SPECTRA_EVERY_DAYS": "0.5",
                          "QD_SPECTRA_FIELDS": " u, wind_speed ,PRECIP"})
    assert d == {"enabled": True, "every": 3, "lat": False, "every_days": 0.5, "fields": ["U", "WIND_SPEED", "PRECIP"]}
    for bad in ("x", "", "0", "-2", "1.5"):
        assert spectra.read_env({"QD_SPECTRA": "1", "QD_SPECTRA_EVERY": bad})["every"] == 24, bad
    for bad in ("x", "0", "-1", "nan", "inf"):
        assert spectra.read_env({"QD_SPECTRA": "1", "QD_SPECTRA_EVERY_DAYS": bad})["every_days"] == 10.0, bad
    for off in ("0", "2", "yes", ""):
        assert spectra.read_env({"QD_SPECTRA": off})["enabled"] is False, off
    assert spectra.read_env({"QD_SPECTRA": "1", "QD_SPECTRA_LAT": "x"})["lat"] is True
    with pytest.raises(ValueError, match=r"QD_SPECTRA_FIELDS: unknown field 'NOPE'"):
        spectra.read_env({"QD_SPECTRA": "1", "QD_SPECTRA_FIELDS": "U,NOPE"})
    with pytest.raises(ValueError, match=r"QD_SPECTRA_FIELDS: 33 entries, at most 32"):
        spectra.read_env({"QD_SPECTRA": "1", "QD_SPECTRA_FIELDS": ",".join(["U"] * 33)})
    assert spectra.read_env({"QD_SPECTRA": "0", "QD_SPECTRA_FIELDS": "NOPE"})["fields"] is None     # off: the list is not looked at
    assert spectra.from_env(None, None, {"QD_SPECTRA": "0"}) is None and spectra.from_env(None, None, {}) is None
    assert spectra.resolve_fields(None, False) == ["U", "V", "H", "Q", "CLOUD"] == spectra.resolve_fields(None, True)
    with pytest.raises(ValueError, match=r"QD_SPECTRA_FIELDS: field 'SST' needs the ocean"):
        spectra.resolve_fields(["SST"], False)
    assert spectra.resolve_fields(["SST", "U"], True) == ["SST", "U"]


class FakeDev:
    """What a Spectra asks of a Device, recorded; spectra_log hands back the rows that were queued."""

    def __init__(self, omega=2.0 * np.pi / 72000.0):
        import types
        self.params = types.SimpleNamespace(omega=omega)
        self.configured, self.scheduled, self.queue, self.resets = None, [], [], 0
        self.sums, self.count = None, 0

    def spectra_configure(self, entries, lat_resolved, w_row):
        self.configured = (list(entries), bool(lat_resolved), np.array(w_row))

    def spectra_schedule(self, flags):
        self.scheduled.append(np.array(flags))

    def spectra_log(self, max_records=None):
        out, self.queue = self.queue, []
        assert max_records is None or len(out) <= max_records
        return np.array(out).reshape(len(out), -1) if out else np.empty((0, 1))

    def spectra_sums(self):
        return self.sums, self.count

    def spectra_sums_set(self, sums, count):
        self.sums, self.count = np.array(sums), int(count)

    def spectra_reset(self):
        self.resets += 1
        self.count = 0


def make_spectra(tmp_path, *, S=4, every=1, lat=True, fields=("U", "V", "WIND_SPEED"), n_lat=5, n_lon=12, lines=None):
    import types
    from qingdai_amd import spectra
    dev = FakeDev()
    grid = types.SimpleNamespace(lat=lat_of(n_lat), lon=np.linspace(0, 360, n_lon), n_lat=n_lat, n_lon=n_lon)
    cfg = {"enabled": True, "every": every, "lat": lat, "every_days": S * 300.0 / 72000.0, "fields": list(fields)}
    s = spectra.Spectra(dev, grid, cfg, with_ocean=True, dt=300.0, day=72000.0, out=(lines if lines is not None else []).append,
                        output_dir=str(tmp_path))
    assert s.S == S
    return s, dev


def run_span(s, dev, n, t0=None):
    k = s.span_schedule(t0, 300.0, n)
    for step in k[2]:
        dev.queue.append(np.full(s.width, float(step)))
    s._fired(k)
    return s.span_deliver(300.0)


def test_schedule_and_window_clock_are_historys(tmp_path):
    from qingdai_amd import history
    s, dev = make_spectra(tmp_path, S=5, every=2)
    assert dev.configured[0] == [(0, "U", None), (0, "V", None), (1, "U", "V")] and dev.configured[1] is True
    assert np.array_equal(dev.configured[2], np.maximum(np.cos(np.deg2rad(lat_of(5))), 0.0))
    assert s.width == 3 * (7 + 1)
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
    k = s.span_schedule(None, 300.0, 1)                          # (step 17 is sampled: 17 % 5 = 2) a record that never came
    s._fired(k)
    with pytest.raises(RuntimeError, match="the device log held 0 records where the schedule says 1"):
        s.span_deliver(300.0)
    # the default cadence: every 24th step of a window, ten per planet-day of 72000 s at 300 s
    from qingdai_amd import spectra
    assert spectra.EVERY == 24 and int(history.schedule(0, 240, 2400, 24).sum()) == 10


@pytest.mark.parametrize("lat", [True, False])
def test_window_file(tmp_path, lat):
    from qingdai_amd import ncio, spectra
    lines = []
    s, dev = make_spectra(tmp_path, S=4, lat=lat, lines=lines)
    n_lat, nb, width = 5, 7, s.width
    per = nb + 1
    r = np.random.default_rng(3)
    recs = np.abs(r.normal(size=(4, width)))
    recs[:, nb], recs[:, per + nb], recs[:, 2 * per + nb] = [0, 2, 0, 5], [1, 0, 0, 0], [0, 0, 0, 0]
    recs[2, per + 1:per + nb] = 0.0                              # V at the third sample: nothing beside the mean
    sums = np.abs(r.normal(size=(3, n_lat, nb)))
    dev.sums, dev.count = (sums, 4) if lat else (None, 0)
    k = s.span_schedule(1200.0, 300.0, 4)
    dev.queue = list(recs)
    s._fired(k)
    s.span_deliver(300.0)
    assert s.window_closed()
    resets = dev.resets
    path = s.flush()
    assert dev.resets == resets + 1                              # the device's sums start the next window from zero
    assert path == str(tmp_path / "spectra" / "spectra_day_00.02_00.03.nc") and s.files == [path] and not os.path.exists(path + ".part")
    assert os.listdir(tmp_path / "spectra") == ["spectra_day_00.02_00.03.nc"]
    v, _ = ncio.read_nc(path)
    want = {"time_seconds", "step", "wavenumber", "lat", "dt_seconds", "sample_every", "lat_resolved", "n_samples", "complete", "ke_power"}
    for name in ("u", "v", "wind_speed"):
        want |= {f"{name}_power", f"{name}_bad_rows", f"{name}_hi_frac"} | ({f"{name}_power_lat"} if lat else set())
    assert set(v) == want
    i8 = np.int64 if ncio.backend() == "netCDF4" else np.float64
    assert v["time_seconds"].tolist() == [1200.0, 1500.0, 1800.0, 2100.0] and v["step"].dtype == i8 and v["step"].tolist() == [0, 1, 2, 3]
    assert v["wavenumber"].tolist() == list(range(nb)) and np.array_equal(v["lat"], lat_of(5))
    for e, name in enumerate(("u", "v", "wind_speed")):
        P = recs[:, e * per:e * per + nb]
        assert v[f"{name}_power"].dtype == np.float64 and v[f"{name}_power"].tobytes() == np.ascontiguousarray(P).tobytes()
        assert v[f"{name}_bad_rows"].dtype == np.int32 and v[f"{name}_bad_rows"].tolist() == recs[:, e * per + nb].astype(int).tolist()
        hf = P[:, 5:].sum(axis=1) / P[:, 1:].sum(axis=1) if name != "v" else None     # kN = 6: k >= ceil(4.5) = 5
        if hf is not None:
            assert np.array_equal(v[f"{name}_hi_frac"], hf)
        else:
            assert np.isnan(v["v_hi_frac"][2]) and np.isfinite(np.delete(v["v_hi_frac"], 2)).all()
        if lat:
            assert v[f"{name}_power_lat"].shape == (n_lat, nb) and np.array_equal(v[f"{name}_power_lat"], sums[e] / 4.0)
    assert np.array_equal(v["ke_power"], 0.5 * (recs[:, 0:nb] + recs[:, per:per + nb]))
    assert (float(v["dt_seconds"]), int(v["sample_every"]), int(v["lat_resolved"]), int(v["n_samples"]), int(v["complete"])) == \
        (300.0, 1, int(lat), 4, 1)
    assert len(lines) == 1
    m = re.fullmatch(r"\[Spectra\] day 0\.02–0\.03: 4 samples \| U hi=(\S+)→(\S+) V hi=(\S+)→(\S+) WIND_SPEED hi=(\S+)→(\S+)", lines[0])
    hf = spectra.hi_frac(recs.reshape(4, 3, per)[:, :, :nb])
    assert m and [float(g) for g in m.groups()] == [float(f"{x:.6g}") for x in (hf[0, 0], hf[3, 0], hf[0, 1], hf[3, 1], hf[0, 2], hf[3, 2])]
    # the window is gone; an open one is written with complete = 0, an empty one not at all
    assert s.flush() is None and len(s.window()[0]) == 0
    k = s.span_schedule(2400.0, 300.0, 2)
    dev.queue = list(recs[:2])
    dev.sums, dev.count = (sums, 2) if lat else (None, 0)
    s._fired(k)
    s.span_deliver(300.0)
    assert not s.window_closed() and s.steps_to_window_end() == 2
    v, _ = ncio.read_nc(s.flush(complete=0))
    assert int(v["complete"]) == 0 and v["step"].tolist() == [4, 5] and len(lines) == 2 and "ke_power" in v


def test_no_ke_without_both_winds_six_entries_in_the_line_and_restore_window(tmp_path):
    from qingdai_amd import ncio
    lines = []
    names = ("U", "H", "Q", "CLOUD", "TS", "HICE", "OLR", "PRECIP")
    s, dev = make_spectra(tmp_path, S=3, lat=True, fields=names, lines=lines)
    run_span(s, dev, 2)
    recs, times, steps = s.window()
    sums = np.ones((8, 5, 7))
    t, dev2 = make_spectra(tmp_path, S=3, lat=True, fields=names, lines=lines)
    t.restore_window(recs, times, steps, s.i, sums=sums, count=2)
    assert t.i == 2 and all(np.array_equal(a, b) for a, b in zip(t.window(), s.window()))
    assert dev2.count == 2 and np.array_equal(dev2.sums, sums)
    run_span(t, dev2, 1)
    dev2.count = 3
    assert t.window_closed()
    v, _ = ncio.read_nc(t.flush())
    assert "ke_power" not in v and int(v["n_samples"]) == 3 and np.array_equal(v["u_power_lat"], np.ones((5, 7)) / 3.0)
    assert lines[0].count(" hi=") == 6 and " OLR hi=" not in lines[0] and ": 3 samples | U hi=" in lines[0]


# ---------------------------------------------------------------- the header
def test_header_declares_the_spectra_abi():
    from qingdai_amd import _lib
    text = open(os.path.join(ROOT, "include", "qingdai_hip.h"), encoding="utf-8").read()
    assert (_lib.C["QD_SPECTRA_MAX_ENTRIES"], _lib.C["QD_SPECTRA_LOG_CAP"], _lib.C["QD_SPECTRA_STATS"]) == (32, 256, 1)
    assert _lib.C["QD_ABI_VERSION"] == 1 and _lib.C["QD_SPECTRA_LOG_CAP"] > 200          # the driver's longest chunk
    assert _lib.state_ref("SPECTRA_SUMS") == _lib.C["QD_STATE_REF_SPECTRA_SUMS"] == 500 and "SPECTRA_SUMS" not in _lib.STATE_REFS
    sig = {name: [(p[0], p[2]) for p in _lib.SIGNATURES[name]][1:] for name in _lib.SYMBOLS if name.startswith("qd_spectra_")}
    assert sig == {
        "qd_spectra_configure": [("n", "int"), ("op", "int32_t"), ("a", "int32_t"), ("b", "int32_t"), ("lat_resolved", "int"), ("w_row", "double")],
        "qd_spectra_schedule": [("steps", "int"), ("sample", "int32_t")],
        "qd_spectra_sample": [],
        "qd_spectra_log": [("out", "double"), ("max", "int"), ("n", "int")],
        "qd_spectra_sums_get": [("sums", "double"), ("count", "int64_t")],
        "qd_spectra_sums_set": [("sums", "double"), ("count", "int64_t")],
        "qd_spectra_reset": []}
    for name in sig:                                             # each with a comment on its line
        assert re.search(r"^int " + name + r"\(.*\);\s*/\*.+\*/\s*$", text, re.M), name
    for macro in ("QD_SPECTRA_MAX_ENTRIES", "QD_SPECTRA_LOG_CAP", "QD_SPECTRA_STATS"):
        assert re.search(r"^#define " + macro + r" \d+\s*/\*.+\*/\s*$", text, re.M), macro
    assert "QD_SPECTRA" not in "".join(f"{k}" for k in _lib._STEP)                       # no flag bit
