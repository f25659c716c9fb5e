"""CPU: the definition of the flow lane (qingdai_amd/flow.py) and its host side, without a device.

  vortdiv_reference against the reference's own SphericalGrid.vorticity / .divergence (tests/golden/flow_*.npz, written by
  scripts/gen_golden_flow.py), bit for bit on the rows 1 .. N - 2; the pole rule; the grid weights; L(psi) = zeta - mean(zeta); the
  zero weighted mean; second-order convergence on an analytic streamfunction; the f64 solve against the extended one; the reduction
  order of the record; environment, window clock, window file, and the round trip of a Flow's open window through what the
  checkpoint carries (window(), sums(), the clock -> restore_window)."""
import glob
import os
import re
import types

import numpy as np
import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
A = 6.371e6


def grid_of(n_lat, n_lon):
    import qingdai_amd as qa
    return qa.SphericalGrid(n_lat, n_lon)


def tables(n_lat, n_lon, a=A):
    from qingdai_amd import flow
    return flow.grid_tables(grid_of(n_lat, n_lon), a)


def bits(a, b):
    a, b = np.asarray(a, dtype=np.float64), np.asarray(b, dtype=np.float64)
    return np.array_equal(a, b, equal_nan=True) and np.array_equal(np.signbit(a) | np.isnan(a), np.signbit(b) | np.isnan(b))


# ---------------------------------------------------------------- zeta, delta
GOLDEN = sorted(glob.glob(os.path.join(ROOT, "tests", "golden", "flow_*.npz")))


def test_goldens_are_there():
    assert len(GOLDEN) == 7 and all(os.path.getsize(p) < 64 * 1024 for p in GOLDEN)


@pytest.mark.parametrize("path", GOLDEN, ids=[os.path.basename(p)[5:-4] for p in GOLDEN])
def test_vortdiv_is_the_references_on_interior_rows(path):
    from qingdai_amd import flow
    z = np.load(path)
    assert set(z.files) == {"shape", "radius", "u", "v", "zeta", "delta"}            # inputs and the reference's two results only
    n_lat, n_lon = (int(x) for x in z["shape"])
    g = flow.grid_tables(grid_of(n_lat, n_lon), float(z["radius"]))
    zeta, delta = flow.vortdiv_reference(z["u"], z["v"], g)
    assert bits(zeta[1:-1], z["zeta"][1:-1]) and bits(delta[1:-1], z["delta"][1:-1])
    assert np.isfinite(zeta).all() and np.isfinite(delta).all()
    # the pole rows: one value along the row, far from the reference's 1e6-fold junk, and no larger than the wind allows
    for x in (zeta, delta):
        for row in (0, -1):
            assert (x[row] == x[row, 0]).all()
            assert abs(x[row, 0]) <= 2.0 * max(np.abs(z["u"]).max(), np.abs(z["v"]).max()) / (g.a * np.sin(g.dlat / 2))


def test_pole_rule_and_lane_order():
    from qingdai_amd import flow, series
    g = tables(7, 300)
    r = np.random.default_rng(5)
    u, v = r.normal(size=(7, 300)), r.normal(size=(7, 300))
    zeta, delta = flow.vortdiv_reference(u, v, g)
    n, wP = 300, g.w[0]
    for x, out, sn, ss in ((u, zeta, 1.0, -1.0), (v, delta, -1.0, 1.0)):
        SN = series.reduce_reference((0.5 * (x[-1] + x[-2]))[None, :], [0.0])[4][0] * n          # the zonal mean times n: the row sum
        assert np.isclose(out[-1, 0], sn * g.ch[5] * SN / (g.a * wP * n), rtol=1e-14, atol=0.0)
        SS = flow._row_sums(0.5 * (x[0] + x[1]))
        assert out[0, 0] == ss * ((g.ch[0] * SS) / ((g.a * wP) * n))
    # _row_sums is the row stage of series.reduce_reference, bit for bit
    x = r.normal(size=(3, 300)) * 10.0 ** r.integers(-6, 7, size=(3, 300))
    assert bits(flow._row_sums(x) / np.float64(300), series.reduce_reference(x, [0.0, 10.0, 20.0])[4])
    # a solid-body rotation u = U cos(lat): the cap's circulation gives the analytic 2 U / a at the north pole within O(dphi^2)
    g = tables(37, 72)
    lat = np.deg2rad(grid_of(37, 72).lat)[:, None]
    zeta, delta = flow.vortdiv_reference(-30.0 * np.cos(lat) * np.ones((37, 72)), np.zeros((37, 72)), g)
    assert abs(zeta[-1, 0] / (-2 * 30.0 / g.a * np.sin(np.pi / 2)) - 1.0) < 2.0 * g.dlat ** 2 and abs(zeta[0, 0] + zeta[-1, 0]) < 1e-18
    assert not delta[0].any() and not delta[-1].any()


def test_grid_weights_sum_to_two():
    for shape in ((3, 4), (5, 4), (19, 36), (37, 72), (131, 12), (721, 1440)):
        g = tables(*shape)
        assert abs(g.w.sum() - 2.0) <= 4 * shape[0] * np.finfo(float).eps, shape
        assert (g.w > 0).all() and g.w[0] == g.w[-1] == 2.0 * np.sin(g.dlat / 4) ** 2
        assert g.tab.shape == (6, shape[0]) and g.lam.shape == (shape[1] // 2 + 1,) and g.lam[0] == 0.0 and (g.lam[1:] < 0).all()
        assert np.array_equal(g.c, np.cos(np.deg2rad(np.linspace(-90, 90, shape[0])))) and g.dlon == np.deg2rad(360.0 / (shape[1] - 1))
    with pytest.raises(ValueError, match="n_lat >= 3 and n_lon >= 4"):
        tables(2, 8)


# ---------------------------------------------------------------- the solve
def random_winds(shape, seed=0):
    r = np.random.default_rng(shape[0] * 10000 + shape[1] + seed)
    lat = np.deg2rad(np.linspace(-90, 90, shape[0]))[:, None]
    return 8.0 * np.cos(lat) + 10.0 * r.normal(size=shape), 5.0 * r.normal(size=shape)


@pytest.mark.parametrize("shape", [(3, 4), (5, 4), (19, 36), (9, 45), (7, 26), (37, 72)])
def test_laplacian_of_the_solution_is_the_right_side(shape):
    """L psi = zeta - mean(zeta) in grid space, the identity that defines the solve.  The bound: psi carries a relative rounding
    error of a few eps times log-size factors, and L amplifies by at most its largest eigenvalue 4 / (a^2 dlam^2 c_1^2) +
    4 / (a^2 dphi^2) against the smallest non-zero one, about 2 / a^2: kappa eps, with a factor 16 for the sums' lengths."""
    from qingdai_amd import flow
    g = tables(*shape)
    u, v = random_winds(shape)
    r = flow.helmholtz_reference(u, v, g)
    kappa = (4.0 / (g.dlon ** 2 * g.c[1] ** 2) + 4.0 / g.dlat ** 2) / 2.0
    tol = 16 * kappa * np.finfo(float).eps
    for sol, rhs, mean in ((r.psi, r.zeta, r.zeta_mean), (r.chi, r.delta, r.div_mean)):
        assert np.isclose(mean, flow.weighted_mean(rhs, g), rtol=0, atol=1e-13 * np.abs(rhs).max())
        err = np.abs(flow.laplacian_reference(sol, g) - (rhs - mean)).max() / np.abs(rhs).max()
        assert err <= tol, (shape, err, tol)
        assert abs(flow.weighted_mean(sol, g)) <= 16 * np.finfo(float).eps * np.abs(sol).max()      # psi's own weighted mean is zero
        assert (sol[0] == sol[0, 0]).all() and (sol[-1] == sol[-1, 0]).all()                         # a pole holds one value


def analytic(n_lat, n_lon):
    """Solid body plus a wavenumber-4 Rossby-Haurwitz wave, sampled on the true-periodic longitude 2 pi i / n; the grid's columns are
    dlam apart with n dlam != 2 pi, so v, a zonal derivative, is scaled by 2 pi / (n dlam) to stay the wind of this psi on the
    grid as the discrete operators see it."""
    from qingdai_amd import flow
    g = tables(n_lat, n_lon)
    phi = np.deg2rad(np.linspace(-90, 90, n_lat))[:, None]
    lam = (2 * np.pi * np.arange(n_lon) / n_lon)[None, :]
    om = K = 7.8e-6
    m = 4
    a = g.a
    psi = -a * a * om * np.sin(phi) + a * a * K * np.cos(phi) ** m * np.sin(phi) * np.cos(m * lam)
    dpsi_dphi = -a * a * om * np.cos(phi) + a * a * K * np.cos(m * lam) * (np.cos(phi) ** (m + 1) - m * np.cos(phi) ** (m - 1) * np.sin(phi) ** 2)
    dpsi_dlam = -m * a * a * K * np.cos(phi) ** m * np.sin(phi) * np.sin(m * lam)
    u = -dpsi_dphi / a
    v = np.zeros_like(u)
    v[1:-1] = (dpsi_dlam / (a * np.cos(phi)))[1:-1] * (2 * np.pi / (n_lon * g.dlon))
    return g, psi - flow.weighted_mean(psi, g), u, v


def test_second_order_convergence_and_a_rotational_wind_has_no_chi():
    from qingdai_amd import flow
    err, chi = [], []
    for shape in ((19, 36), (37, 72), (73, 144)):
        g, psi, u, v = analytic(*shape)
        r = flow.helmholtz_reference(u, v, g)
        err.append(np.abs(r.psi - psi).max() / np.abs(psi).max())
        chi.append(np.abs(r.chi).max() / np.abs(psi).max())
    print("psi error", err, "chi size", chi)
    assert err[0] < 0.03
    for k in (0, 1):                                             # second order: the ratio per doubling lies between 3 and 5
        assert 3.0 < err[k] / err[k + 1] < 5.0, err
        assert 3.0 < chi[k] / chi[k + 1] < 5.0, chi              # and |chi| of a purely rotational wind shrinks at the same order


@pytest.mark.parametrize("shape", [(3, 4), (19, 36), (7, 35), (91, 180)])
def test_f64_solve_against_the_extended_one(shape):
    """The yardstick of tests/test_gpu_flow.py: the f64 restatement differs from the extended solve by rounding alone."""
    from qingdai_amd import flow
    g = tables(*shape)
    u, v = random_winds(shape)
    r, x = flow.helmholtz_reference(u, v, g), flow.helmholtz_reference(u, v, g, extended=True)
    assert bits(r.zeta, x.zeta) and bits(r.delta, x.delta)       # zeta and delta are f64 quantities in both
    for a, b in ((r.psi, x.psi), (r.chi, x.chi)):
        e = np.abs(a - b).max() / np.abs(b).max()
        assert 0.0 < e < 64 * max(shape) * np.finfo(float).eps / 8, (shape, e)


def test_mpmath_path_agrees_with_longdouble(monkeypatch):
    pytest.importorskip("mpmath")
    from qingdai_amd import flow
    if not flow._wide():
        pytest.skip("np.longdouble is f64 here: the mpmath path is the extended one already")
    g = tables(5, 8)
    u, v = random_winds((5, 8))
    a = flow.helmholtz_reference(u, v, g, extended=True)
    monkeypatch.setattr(flow, "_wide", lambda: False)
    b = flow.helmholtz_reference(u, v, g, extended=True)
    assert np.abs(a.psi - b.psi).max() <= 4 * np.finfo(float).eps * np.abs(a.psi).max()


def test_a_non_finite_wind_makes_psi_and_chi_nan_everywhere():
    from qingdai_amd import flow
    g = tables(9, 12)
    u, v = random_winds((9, 12))
    u[4, 5] = np.inf
    v[7, 0] = np.nan
    r = flow.helmholtz_reference(u, v, g)
    assert np.isnan(r.psi).all() and np.isnan(r.chi).all()
    rec = flow.scalars_reference(u, v, r.zeta, r.delta, r.psi, r.chi, g)
    k = {n: q for q, n in enumerate(flow.REC)}
    assert rec[k["bad_rows"]] == 2 and np.isnan(rec[k["ke"]]) and rec[k["psi_min"]] == np.inf and rec[k["psi_max"]] == -np.inf


def test_record_is_what_it_says():
    from qingdai_amd import flow
    shape = (19, 300)
    g = tables(*shape)
    u, v = random_winds(shape)
    r = flow.helmholtz_reference(u, v, g)
    rec = dict(zip(flow.REC, flow.scalars_reference(u, v, r.zeta, r.delta, r.psi, r.chi, g)))
    wm = lambda x: flow.weighted_mean(x, g)
    inner = lambda x: np.concatenate([np.zeros((1, shape[1])), x[1:-1], np.zeros((1, shape[1]))])
    assert np.isclose(rec["vort_global"], wm(r.zeta), rtol=1e-9, atol=1e-20) and np.isclose(rec["vort_global"], r.zeta_mean, rtol=1e-9, atol=1e-20)
    assert np.isclose(rec["vort_rms"], np.sqrt(wm(r.zeta ** 2)), rtol=1e-13) and np.isclose(rec["div_rms"], np.sqrt(wm(r.delta ** 2)), rtol=1e-13)
    assert rec["vort_maxabs"] == np.abs(r.zeta).max() and rec["div_maxabs"] == np.abs(r.delta).max()
    assert (rec["psi_min"], rec["psi_max"], rec["chi_min"], rec["chi_max"]) == (r.psi.min(), r.psi.max(), r.chi.min(), r.chi.max())
    assert np.isclose(rec["ke"], wm(inner(0.5 * (u * u + v * v))), rtol=1e-13) and rec["bad_rows"] == 0
    assert 0 < rec["ke_rot"] and 0 < rec["ke_div"]
    # a purely rotational wind: its energy is the rotational part's up to the discretisation, the divergent part is small
    g, psi, u, v = analytic(73, 144)
    r = flow.helmholtz_reference(u, v, g)
    rec = dict(zip(flow.REC, flow.scalars_reference(u, v, r.zeta, r.delta, r.psi, r.chi, g)))
    assert abs(rec["ke_rot"] / rec["ke"] - 1.0) < 0.02 and rec["ke_div"] < 1e-4 * rec["ke"]


# ---------------------------------------------------------------- environment, clock, files
def test_read_env():
    from qingdai_amd import flow
    assert flow.read_env({}) == {"enabled": False, "every": 24, "every_days": 10.0}
    assert flow.read_env({"QD_FLOW": "1", "QD_FLOW_EVERY": "3", "QD_FLOW_EVERY_DAYS": "0.5"}) == {"enabled": True, "every": 3, "every_days": 0.5}
    for bad in ("x", "", "0", "-2", "1.5"):
        assert flow.read_env({"QD_FLOW": "1", "QD_FLOW_EVERY": bad})["every"] == 24, bad
    for bad in ("x", "0", "-1", "nan", "inf"):
        assert flow.read_env({"QD_FLOW": "1", "QD_FLOW_EVERY_DAYS": bad})["every_days"] == 10.0, bad
    for off in ("0", "2", "yes", ""):
        assert flow.read_env({"QD_FLOW": off})["enabled"] is False, off
    assert flow.from_env(None, None, {"QD_FLOW": "0"}) is None and flow.from_env(None, None, {}) is None       # off: nothing is touched


class FakeDev:
    """What a Flow asks of a Device, recorded; flow_log hands back the rows that were queued."""

    def __init__(self):
        self.params = types.SimpleNamespace(omega=2.0 * np.pi / 72000.0, a=A)
        self.configured, self.scheduled, self.queue, self.resets = None, [], [], 0
        self.sums, self.count = np.zeros((4, 5, 12)), 0

    def flow_configure(self, tables):
        self.configured = tables

    def flow_schedule(self, flags):
        self.scheduled.append(np.array(flags))

    def flow_log(self, max_records=None):
        out, self.queue = self.queue, []
        assert max_records is None or len(out) <= max_records
        return np.array(out).reshape(len(out), -1) if out else np.empty((0, 14))

    def flow_sums(self):
        return self.sums, self.count

    def flow_sums_set(self, sums, count):
        self.sums, self.count = np.array(sums), int(count)

    def flow_reset(self):
        self.resets += 1
        self.count = 0


def make_flow(tmp_path, *, S=4, every=1, lines=None):
    from qingdai_amd import flow
    dev = FakeDev()
    f = flow.Flow(dev, grid_of(5, 12), {"enabled": True, "every": every, "every_days": S * 300.0 / 72000.0}, dt=300.0, day=72000.0,
                  out=(lines if lines is not None else []).append, output_dir=str(tmp_path))
    assert f.S == S and f.width == flow.REC_W == 14
    return f, dev


def run_span(f, dev, n, t0=None):
    k = f.span_schedule(t0, 300.0, n)
    for step in k[2]:
        dev.queue.append(np.full(f.width, float(step) + 1.0))
    f._fired(k)
    return f.span_deliver(300.0)


def test_schedule_and_window_clock_are_historys(tmp_path):
    from qingdai_amd import flow, history
    f, dev = make_flow(tmp_path, S=5, every=2)
    assert dev.configured.tab.shape == (6, 5) and dev.configured.geom.tolist() == [A, np.deg2rad(45.0), np.deg2rad(360.0 / 11)]
    i = 0
    for n in (3, 1, 4, 7, 2):
        assert f.steps_to_window_end() == 5 - i % 5
        clock = f.span_clock()
        k = f.span_schedule(None, 300.0, n)
        assert np.array_equal(dev.scheduled[-1], history.schedule(i, n, 5, 2)) and dev.scheduled[-1].dtype == np.int32
        assert k[0] == n and np.array_equal(k[2], i + np.flatnonzero(history.schedule(i, n, 5, 2))) and np.array_equal(k[1], k[2] * 300.0)
        f.span_restore(clock)                                    # a refused span: the clock stays
        assert f.i == i and f.span_clock() == clock
        recs = run_span(f, dev, n)
        i += n
        assert f.i == i and len(recs) == int(history.schedule(i - n, n, 5, 2).sum()) and f.window_closed() == (i % 5 == 0)
    recs, times, steps = f.window()
    want = np.flatnonzero(history.schedule(0, 17, 5, 2))
    assert np.array_equal(steps, want) and np.array_equal(times, want * 300.0) and np.array_equal(recs[:, 0], want + 1.0)
    k = f.span_schedule(None, 300.0, 1)                          # (step 17 is sampled) a record that never came
    f._fired(k)
    with pytest.raises(RuntimeError, match="the device log held 0 records where the schedule says 1"):
        f.span_deliver(300.0)
    assert flow.EVERY == 24 and int(history.schedule(0, 240, 2400, 24).sum()) == 10      # ten samples per planet-day by default


def test_window_file_and_the_round_trip_of_an_open_window(tmp_path):
    from qingdai_amd import flow, ncio
    lines = []
    f, dev = make_flow(tmp_path, S=4, lines=lines)
    r = np.random.default_rng(3)
    recs = r.normal(size=(4, 14))
    recs[:, 13] = [0, 2, 0, 1]
    sums = r.normal(size=(4, 5, 12))
    dev.sums, dev.count = sums, 4
    k = f.span_schedule(1200.0, 300.0, 4)
    dev.queue = list(recs)
    f._fired(k)
    f.span_deliver(300.0)
    assert f.window_closed()
    resets = dev.resets
    path = f.flush()
    assert dev.resets == resets + 1                              # the device's sums start the next window from zero
    assert path == str(tmp_path / "flow" / "flow_day_00.02_00.03.nc") and f.files == [path] and os.listdir(tmp_path / "flow") == ["flow_day_00.02_00.03.nc"]
    v, _ = ncio.read_nc(path)
    assert set(v) == ({"time_seconds", "step", "lat", "lon", "dt_seconds", "sample_every", "n_samples", "complete", "psi_mean", "chi_mean",
                       "vort_mean", "div_mean"} | set(flow.REC))
    assert v["time_seconds"].tolist() == [1200.0, 1500.0, 1800.0, 2100.0] and v["step"].tolist() == [0, 1, 2, 3]
    for q, name in enumerate(("psi", "chi", "vort", "div")):
        assert v[f"{name}_mean"].shape == (5, 12) and np.array_equal(v[f"{name}_mean"], sums[q] / 4.0)
    for q, name in enumerate(flow.REC[:-1]):
        assert v[name].dtype == np.float64 and np.array_equal(v[name], recs[:, q]), name
    assert v["bad_rows"].dtype == np.int32 and v["bad_rows"].tolist() == [0, 2, 0, 1]
    assert (float(v["dt_seconds"]), int(v["sample_every"]), int(v["n_samples"]), int(v["complete"])) == (300.0, 1, 4, 1)
    assert len(lines) == 1 and re.fullmatch(r"\[Flow\] day 0\.02–0\.03: 4 samples \| vort rms=\S+→\S+ div rms=\S+→\S+ KE=\S+ rot=\S+ div=\S+ bad=3",
                                            lines[0]), lines
    assert f.flush() is None and len(f.window()[0]) == 0         # the window is gone; an empty one is not written
    # an open window travels: what the checkpoint carries (window(), sums(), the clock) restores a second Flow to the same state
    run_span(f, dev, 2, t0=2400.0)
    dev.sums, dev.count = sums * 2.0, 2
    w, (s, c) = f.window(), f.sums()
    t, dev2 = make_flow(tmp_path / "resumed", S=4, lines=lines)
    t.restore_window(w[0], w[1], w[2], f.i, sums=s, count=c)
    assert t.i == f.i == 6 and all(np.array_equal(a, b) for a, b in zip(t.window(), w)) and dev2.count == 2 and np.array_equal(dev2.sums, s)
    assert not t.window_closed() and t.steps_to_window_end() == 2
    for x, d in ((f, dev), (t, dev2)):
        run_span(x, d, 2, t0=3000.0)
        d.count = 4
        assert x.window_closed()
    pa, pb = f.flush(), t.flush()
    assert os.path.basename(pa) == os.path.basename(pb) and open(pa, "rb").read() == open(pb, "rb").read()
    v, _ = ncio.read_nc(pb)
    assert int(v["complete"]) == 1 and v["step"].tolist() == [4, 5, 6, 7]


# ---------------------------------------------------------------- the header
def test_header_declares_the_flow_abi():
    from qingdai_amd import _lib
    assert (_lib.C["QD_FLOW_LOG_CAP"], _lib.C["QD_FLOW_TAB"], _lib.C["QD_FLOW_PLANES"], _lib.C["QD_FLOW_REC_W"]) == (256, 6, 4, 14)
    assert _lib.C["QD_ABI_VERSION"] == 1 and _lib.C["QD_FLOW_LOG_CAP"] > 200             # the driver's longest chunk
    assert _lib.state_ref("FLOW_SUMS") == _lib.C["QD_STATE_REF_FLOW_SUMS"] == 501 and "FLOW_SUMS" not in _lib.STATE_REFS
    sig = {name: [(p[0], p[2]) for p in _lib.SIGNATURES[name]][1:] for name in _lib.SYMBOLS if name.startswith("qd_flow_") and name != "qd_flow_solve_grid"}
    assert sig == {
        "qd_flow_configure": [("tab", "double"), ("lam", "double"), ("geom", "double")],
        "qd_flow_schedule": [("steps", "int"), ("sample", "int32_t")],
        "qd_flow_sample": [],
        "qd_flow_log": [("out", "double"), ("max", "int"), ("n", "int")],
        "qd_flow_sums_get": [("sums", "double"), ("count", "int64_t")],
        "qd_flow_sums_set": [("sums", "double"), ("count", "int64_t")],
        "qd_flow_reset": [],
        "qd_flow_solve": [("u", "double"), ("v", "double"), ("zeta", "double"), ("delta", "double"), ("psi", "double"), ("chi", "double")]}
    assert [p[0] for p in _lib.SIGNATURES["qd_flow_solve_grid"]][:3] == ["n_lat", "n_lon", "device"]
    csrc = os.path.join(ROOT, "qingdai_amd", "csrc")
    assert '#include "qd_rowfft.h"' in open(os.path.join(csrc, "qd_spectra.hip")).read()      # one FFT, shared
    assert "QD_LANE_FLOW" in open(os.path.join(csrc, "qd_span.h")).read()
