"""GPU (-m gpu): the spherical-harmonic lane (csrc/qd_spharm.hip, qingdai_amd/spharm.py).

  1 the kernels alone through qd_spharm_analyse (a handle has at least five rows) and qd_spharm_analyse_grid (no handle), at the
    smallest shapes where each form can go wrong: 5 x 8 (N = 2, the smallest handle; both seams, the same bits), 3 x 8 (below a
    handle), 19 x 36 (FFT form), 9 x 45 (odd n_lon), 20 x 36 (even n_lat: no equator row), 33 x 24 (n_lon sets N), 7 x 26 (direct
    row form), 131 x 12 (66 latitude pairs: a lane takes a second pair), 19 x 36 under QD_SPHARM_FORM=direct; and the two row counts on
    each side of the places where the Legendre kernel changes form (2, 6, 12 pairs per lane): 256 | 257 and 768 | 769 rows, at
    n_lon = 8 through the seam without a handle.
      coefficients   against spharm.analyse_reference(extended=True).  The yardstick is measured, as in tests/test_gpu_flow.py: the
                     f64 NumPy restatement's own error e64 = max |c64 - cext| / max |cext| at the same shape and plane; the device may
                     exceed it by a factor of 8 (its sums run in another order -- the FFT, the hemispheres folded, 64 lanes --, and
                     each reordering of a few dozen terms legitimately moves a few ulps).  The pairs are printed; DESIGN.md section 7
                     lists them.
      the record     P(n), ms and the bad rows against spharm.power_reference of the device's own coefficients, bit for bit
      forms          the FFT and the direct row form of 19 x 36 agree within the same bound
      round trip     a synthesised band-limited plane gives its coefficients back within 8 times the f64 reference's recovery error
      a NaN          one NaN in the plane: every coefficient and every bin NaN, bad rows = 1; the clean call behind it gives the
                     first call's bits; the class seam leaves the sums alone
      VORT / DIV     on a handle: the lane's record of these entries is, bit for bit, the seam's record of flow.vortdiv_reference of
                     the resident U and V
  2 the lane at 19 x 36: a span against a cut span against single steps with a class-seam sample behind each, bitwise; lane off
    equals the state digest of a run that never heard of the lane; driver.main writes two windows and an open one with the
    documented variables; a run cut inside a window and resumed writes the uncut run's bytes; more samples than the log holds and a
    band handle are refused with the lane's own text."""
import ctypes
import os
import re

import numpy as np
import pytest

from test_gpu_budget_diag import make, fetch, DT
from test_gpu_series import same, _set_env

pytestmark = pytest.mark.gpu

SHAPES = [(5, 8), (3, 8), (19, 36), (9, 45), (20, 36), (33, 24), (7, 26), (131, 12), (256, 8), (257, 8), (768, 8), (769, 8)]
CASES = [(s, "default") for s in SHAPES] + [((19, 36), "direct")]
FACTOR = 8.0
_REF, _GOT = {}, {}


def plane_of(shape):
    """The u plane of the flow test's winds()."""
    n_lat, n = shape
    r = np.random.default_rng(n_lat * 10000 + n)
    lat = np.deg2rad(np.linspace(-90, 90, n_lat))[:, None]
    return 8.0 * np.cos(lat) + 10.0 * r.normal(size=shape)


def reference(shape):
    """(tables, plane, the f64 restatement, the extended analysis, random coefficients, their plane, the f64 recovery error) of a
    shape, computed once."""
    from qingdai_amd import spharm
    if shape not in _REF:
        g = spharm.tables(*shape)
        x = plane_of(shape)
        r = np.random.default_rng(shape[0] + shape[1])
        c = np.triu(r.normal(size=(g.N + 1, g.N + 1)) + 1j * r.normal(size=(g.N + 1, g.N + 1)))
        c[0] = c[0].real
        y = spharm.synthesise(c, g, extended=True)
        e_cpu = float(np.abs(spharm.analyse_reference(y, g) - c).max())
        _REF[shape] = (g, x, spharm.analyse_reference(x, g), spharm.analyse_reference(x, g, extended=True), c, y, e_cpu)
    return _REF[shape]


def relerr(x, ref):
    return float(np.abs(x - ref).max() / np.abs(ref).max())


def analyse(shape, x, dev=None):
    """-> (coef, rec) from the device: through the handle's seam, or without a handle."""
    from qingdai_amd import spharm
    if dev is None:
        r = spharm.analyse_grid(shape[0], shape[1], x)
        return r.coef, r.rec
    return dev.spharm_analyse(x)


def check_record(coef, rec, x, g, bad_rows=0):
    from qingdai_amd import spharm
    P, ms, bad = spharm.power_reference(coef, x, g)
    assert same(rec[:g.N + 1], P) and same(rec[g.N + 1], ms) and rec[g.N + 2] == bad == bad_rows, (rec, P, ms, bad)


@pytest.mark.parametrize("shape,form", CASES, ids=[f"{s[0]}x{s[1]}-{f}" for s, f in CASES])
def test_analyse(gpu, monkeypatch, shape, form):
    import qingdai_amd as qa
    from qingdai_amd.device import Device
    if form == "direct":
        monkeypatch.setenv("QD_SPHARM_FORM", "direct")
    else:
        monkeypatch.delenv("QD_SPHARM_FORM", raising=False)
    g, x, c64, cext, c_rand, y, e_cpu = reference(shape)
    dev = None
    if 5 <= shape[0] <= 131:
        dev = Device(qa.SphericalGrid(*shape))
        dev.spharm_configure([(0, "H", None)], True, g)
    coef, rec = analyse(shape, x, dev)
    assert np.isfinite(coef.real).all() and np.isfinite(coef.imag).all() and not np.tril(coef, -1).any()
    e64, edev = relerr(c64, cext), relerr(coef, cext)
    print(f"spharm {shape[0]}x{shape[1]} {form} (N = {g.N}): f64 restatement {e64:.3e} device {edev:.3e} ratio {edev / e64:.2f}")
    assert e64 > 0.0 and edev <= FACTOR * e64, (shape, form, e64, edev)
    check_record(coef, rec, x, g)
    _GOT[(shape, form)] = coef
    if (shape, "default") in _GOT and (shape, "direct") in _GOT:             # the two row forms of one grid
        d = float(np.abs(_GOT[(shape, "default")] - _GOT[(shape, "direct")]).max() / np.abs(cext).max())
        print(f"spharm {shape[0]}x{shape[1]} fft against direct: {d:.3e} ({d / e64:.2f} of the f64 restatement's error)")
        assert d <= FACTOR * e64, (shape, d, e64)
    # the round trip of a band-limited plane
    back, rec_y = analyse(shape, y, dev)
    e_dev = float(np.abs(back - c_rand).max())
    print(f"spharm {shape[0]}x{shape[1]} {form} round trip: f64 reference {e_cpu:.3e} device {e_dev:.3e}")
    assert e_dev <= FACTOR * e_cpu, (shape, form, e_cpu, e_dev)
    check_record(back, rec_y, y, g)
    assert abs(rec_y[:g.N + 1].sum() / rec_y[g.N + 1] - 1.0) <= 1e-13       # Parseval: the plane is band-limited
    # one NaN in the plane: every coefficient, every bin; nothing else is disturbed
    xb = x.copy()
    xb[shape[0] // 2, shape[1] // 3] = np.nan
    cb, rb = analyse(shape, xb, dev)
    assert np.isnan(cb.real).all() and np.isnan(cb.imag).all() and np.isnan(rb[:g.N + 2]).all() and rb[g.N + 2] == 1, (shape, form, rb)
    check_record(cb, rb, xb, g, bad_rows=1)
    again = analyse(shape, x, dev)
    assert same(again[0].real, coef.real) and same(again[0].imag, coef.imag) and same(again[1], rec), (shape, form)
    if dev is None:
        return
    if shape == (5, 8):                                          # the seam without a handle runs the same kernels
        other = analyse(shape, x)
        assert same(other[0].real, coef.real) and same(other[0].imag, coef.imag) and same(other[1], rec)
    sums, count = dev.spharm_sums()                              # the class seam on a host plane leaves the sums and the log alone
    assert count == 0 and not sums.any() and len(dev.spharm_log()) == 0
    dev.close()


def test_vort_and_div_entries_are_the_flow_lanes(gpu, monkeypatch):
    from qingdai_amd import flow, spharm
    monkeypatch.delenv("QD_SPHARM_FORM", raising=False)
    sim = make(monkeypatch, 19, 36, routing=False)
    sim.run_steps(3)
    g = spharm.grid_tables(sim.grid)
    fg = flow.grid_tables(sim.grid, sim.dev.params.a)
    names = ["VORT", "H", "DIV", "WIND_SPEED"]
    sim.dev.spharm_configure(spharm.entries_for(names), True, g, fg)
    sim.dev.spharm_sample()
    recs = sim.dev.spharm_log()
    assert recs.shape == (1, spharm.record_width(4, g.N))
    power, ms, bad = spharm.split_records(recs, 4, g.N)
    sums, count = sim.dev.spharm_sums()
    assert count == 1 and sums.shape == (4, g.N + 1, g.N + 1)
    w = fetch(sim.dev, ["U", "V", "H"])
    zeta, delta = flow.vortdiv_reference(w["U"], w["V"], fg)
    planes = {"VORT": zeta, "DIV": delta, "H": w["H"], "WIND_SPEED": np.sqrt(w["U"] * w["U"] + w["V"] * w["V"])}
    for q, name in enumerate(names):
        coef, rec = sim.dev.spharm_analyse(planes[name])
        assert same(rec[:g.N + 1], power[0, q]) and same(rec[g.N + 1], ms[0, q]) and rec[g.N + 2] == bad[0, q] == 0, name
        term = spharm.bin_weights(g.N)[:, None] * (coef.real * coef.real + coef.imag * coef.imag)      # [m][n]
        assert same(sums[q], term.T), name
        assert power[0, q].sum() > 0 and float(spharm.resid(power[0, q], ms[0, q])) < 1.0, name
    sim.dev.close()


# ---------------------------------------------------------------- 2: the lane
def attach(sim, tmp_path, *, every=1, S=None, lane=True, fields=None):
    """A Spharm on the run's handle; lane=False: configured, but no participant of the spans (the class seam's twin)."""
    from qingdai_amd import spharm
    days = spharm.EVERY_DAYS if S is None else S * DT / sim.day_seconds
    sim.spharm_lines = []
    f = spharm.Spharm(sim.dev, sim.grid, {"enabled": True, "every": every, "every_days": days, "two_d": True, "fields": fields},
                      with_ocean=True, dt=DT, day=sim.day_seconds, out=sim.spharm_lines.append, output_dir=str(tmp_path))
    assert S is None or f.S == S
    sim.spharm = f if lane else None
    return f


@pytest.mark.parametrize("every", [1, 2])
def test_span_equals_single_steps(gpu, monkeypatch, tmp_path, every):
    monkeypatch.delenv("QD_SPHARM_FORM", raising=False)
    fields = ["VORT", "DIV", "H", "PRECIP"]                      # PRECIP: sampled in front of the ocean step inside a span
    got = []
    for cuts in ([6], [2, 4]):
        sim = make(monkeypatch, 19, 36, routing=False)
        f = attach(sim, tmp_path, every=every, fields=fields)
        for n in cuts:
            sim.run_steps(n)
        recs, times, steps = f.window()
        assert steps.tolist() == list(range(0, 6, every)) and times.tolist() == [k * DT for k in range(0, 6, every)]
        got.append((recs, f.sums()))
        sim.dev.close()
    sim = make(monkeypatch, 19, 36, routing=False)
    f = attach(sim, tmp_path, every=every, lane=False, fields=fields)
    for i in range(6):
        sim.run_steps(1)
        if i % every == 0:
            sim.dev.spharm_sample()
    got.append((sim.dev.spharm_log(), sim.dev.spharm_sums()))
    sim.dev.close()
    N = f.N
    assert got[0][0].shape == (6 // every, 4 * (N + 3)) and got[0][1][0].shape == (4, N + 1, N + 1)
    for k, (recs, (sums, count)) in enumerate(got):
        assert same(recs, got[0][0]) and same(sums, got[0][1][0]) and count == 6 // every, (every, k)
    assert np.isfinite(got[0][0]).all() and got[0][1][0].any()
    assert all(not np.array_equal(got[0][0][i], got[0][0][i + 1]) for i in range(6 // every - 1))
    assert not os.path.exists(tmp_path / "spharm") and sim.spharm_lines == []


KERNELS = ("spharm_vortdiv", "spharm_rows", "spharm_leg", "spharm_record")


def test_lane_off_equals_the_parent_digest_and_refusals(gpu, monkeypatch, tmp_path):
    import qingdai_amd as qa
    from qingdai_amd import flow, spharm
    from qingdai_amd._lib import C, QdError
    from qingdai_amd.device import Device
    monkeypatch.delenv("QD_SPHARM_FORM", raising=False)
    runs = {}
    for on in (False, True):
        sim = make(monkeypatch, 19, 36, routing=False)
        if on:
            attach(sim, tmp_path / "on", S=3)
        sim.dev.timing(True)
        for n in (3, 4):
            sim.run_steps(n)
        sim.dev.sync()
        launches = [sim.dev.timing_get(k)[1] for k in KERNELS]
        sim.dev.timing(False)
        runs[on] = dict(digest=sim.digest(), launches=launches, lines=list(getattr(sim, "spharm_lines", [])),
                        files=sorted(os.listdir(tmp_path / "on" / "spharm")) if on else None)
        if not on:
            with pytest.raises(QdError, match="qd_state_digest: ref SPHARM_SUMS: the 2D sums of the spherical-harmonic lane are not configured"):
                sim.dev.digest(["SPHARM_SUMS"])
            for call in (sim.dev.spharm_sample, sim.dev.spharm_log, sim.dev.spharm_reset, lambda: sim.dev.spharm_schedule([1]),
                         sim.dev.spharm_sums, lambda: sim.dev.spharm_analyse(np.zeros((19, 36)))):
                with pytest.raises(QdError, match="not configured"):
                    call()
            g = spharm.grid_tables(sim.grid)
            with pytest.raises(QdError, match="qd_spharm_configure: a grid of 19 x 36 has the truncation N = 9, the tables are for N = 8"):
                sim.dev.call("qd_spharm_configure", 1, [0], [qa._lib.F["H"]], [-1], 1, 8, g.w, g.mu, g.seed_pairs, g.A, g.B, None, None)
            with pytest.raises(QdError, match="qd_spharm_configure: op 1 cannot pair PRECIP with another field"):
                sim.dev.spharm_configure([(1, "PRECIP", "U")], True, g)
            with pytest.raises(QdError, match="qd_spharm_configure: a VORT or DIV entry needs the flow lane's grid table"):
                sim.dev.call("qd_spharm_configure", 1, [C["QD_SPHARM_OP_VORT"]], [-1], [-1], 1, 9, g.w, g.mu, g.seed_pairs, g.A, g.B, None, None)
            with pytest.raises(QdError, match="not configured"):                  # none of the refused calls left a configuration
                sim.dev.spharm_log()
        else:
            # more samples than the log holds, the wrong schedule length: refused with the lane's own text, nothing runs
            cap = C["QD_SPHARM_LOG_CAP"]
            flags = dict(with_ocean=True, with_physics=True, pass_albedo=False, with_hydrology=True)
            stars = sim.forcing.star_table(DT * np.arange(cap + 1))
            counters = sim.dev.counters()
            sim.dev.spharm_schedule(np.ones(cap + 1, dtype=np.int32))
            with pytest.raises(QdError, match=r"qd_step_n: the span's spharm records would overflow the log of QD_SPHARM_LOG_CAP \(drain it "
                                              r"with qd_spharm_log first\)"):
                sim.dev.step_n(stars, DT, **flags)
            sim.dev.spharm_schedule([1, 1, 1])
            with pytest.raises(QdError, match="a qd_spharm_schedule must cover exactly the n steps of the span"):
                sim.dev.step_n(stars[:2], DT, **flags)
            assert sim.dev.counters() == counters and len(sim.dev.spharm_log()) == 0
        sim.dev.close()
    off, on = runs[False], runs[True]
    # per sampled step one vorticity / divergence launch and one of each stage (VORT, DIV, H are all sampled behind the step)
    assert off["launches"] == [0] * 4 and on["launches"] == [7] * 4
    assert len(on["files"]) == 2 and len(on["lines"]) == 2 and all(s.startswith("[SphSpec] day ") for s in on["lines"])
    d_on = {k: v for k, v in on["digest"].items() if k not in ("SPHARM_SUMS", "run")}
    d_off = {k: v for k, v in off["digest"].items() if k != "run"}
    assert d_on == d_off and len(d_off) > 20 and "SPHARM_SUMS" in on["digest"] and "SPHARM_SUMS" not in off["digest"]
    # a band handle
    band = Device(qa.SphericalGrid(73, 144), row0=20, n_rows=30, halo=6)
    g = spharm.tables(73, 144)
    n1 = g.N + 1
    arr = lambda a: np.ascontiguousarray(a, dtype=np.float64).ctypes.data_as(ctypes.c_void_p)
    rc = band.lib.qd_spharm_configure(band.h, 1, (ctypes.c_int32 * 1)(0), (ctypes.c_int32 * 1)(qa._lib.F["H"]), (ctypes.c_int32 * 1)(-1), 1, g.N,
                                      arr(g.w), arr(g.mu), arr(g.seed_pairs), arr(g.A), arr(g.B), None, None)
    assert rc != 0 and b"qd_spharm_configure: the spherical-harmonic spectra need a whole-globe handle" in band.lib.qd_last_error(band.h)
    assert b"latitude bands are not supported" in band.lib.qd_last_error(band.h) and n1 == 37
    band.close()


def _env(tmp_path, data, days, **extra):
    e = {"QD_N_LAT": "19", "QD_N_LON": "36", "QD_DT_SECONDS": "300", "QD_SIM_DAYS": str(days), "QD_DYN_DIAG_PRINT": "0", "QD_ECO_ENABLE": "0",
         "QD_HYDRO_ENABLE": "0", "QD_USE_OCEAN": "1", "QD_DATA_DIR": str(tmp_path / data), "QD_OUTPUT_DIR": str(tmp_path / ("out_" + data)),
         "QD_SPHARM": "1", "QD_SPHARM_EVERY_DAYS": "0.05", "QD_SPHARM_EVERY": "2"}
    e.update(extra)
    return e


def test_driver_main(gpu, tmp_path, monkeypatch, capsys):
    from qingdai_amd import driver, ncio
    monkeypatch.chdir(tmp_path)
    _set_env(monkeypatch, _env(tmp_path, "on", 0.125))           # 30 steps: windows 0-11 and 12-23, 24-29 is written open
    assert driver.main() == 0
    out = capsys.readouterr().out
    lines = [s for s in out.splitlines() if s.startswith("[SphSpec]")]
    assert len(lines) == 3 and [int(re.search(r": (\d+) samples", s).group(1)) for s in lines] == [6, 6, 3], out
    assert all(re.fullmatch(r"\[SphSpec\] day \d+\.\d+–\d+\.\d+: \d+ samples \| KE slope=\S+→\S+ VORT resid=\S+→\S+ DIV resid=\S+→\S+ "
                            r"H resid=\S+→\S+", s) for s in lines), lines
    d = tmp_path / "out_on" / "spharm"
    files = sorted(os.listdir(d))
    assert len(files) == 3 and all(re.fullmatch(r"spharm_day_\d+\.\d+_\d+\.\d+\.nc", f) for f in files), files
    per = {f"{n}_{s}" for n in ("vort", "div", "h") for s in ("power", "meansq", "resid", "bad_rows", "power_nm")}
    for f, (steps, complete) in zip(files, ((range(0, 12, 2), 1), (range(12, 24, 2), 1), (range(24, 30, 2), 0))):
        v, _ = ncio.read_nc(str(d / f))
        steps = list(steps)
        assert v["step"].tolist() == steps and v["time_seconds"].tolist() == [k * DT for k in steps], f
        assert (int(v["complete"]), int(v["sample_every"]), int(v["n_samples"]), float(v["dt_seconds"]), int(v["truncation"])) == \
               (complete, 2, len(steps), DT, 9)
        assert set(v) == per | {"time_seconds", "step", "degree", "ke_power", "ke_rot_power", "ke_div_power", "ke_slope", "truncation",
                                "dt_seconds", "sample_every", "n_samples", "complete"}
        assert v["degree"].tolist() == list(range(10))
        for n in ("vort", "div", "h"):
            P, ms = v[f"{n}_power"], v[f"{n}_meansq"]
            assert P.shape == (len(steps), 10) and np.isfinite(P).all() and (P >= 0).all() and (ms > 0).all() and not v[f"{n}_bad_rows"].any()
            assert (v[f"{n}_resid"] < 1.0).all() and np.allclose(v[f"{n}_resid"], 1.0 - P.sum(axis=1) / ms, rtol=0, atol=1e-15), (f, n)
            nm = v[f"{n}_power_nm"]
            assert nm.shape == (10, 10) and not np.triu(nm, 1).any() and np.allclose(nm.sum(axis=1), P.mean(axis=0), rtol=1e-12, atol=0)
        assert np.array_equal(v["ke_power"], v["ke_rot_power"] + v["ke_div_power"]) and (v["ke_power"][:, 1:] > 0).all()
        assert not v["ke_power"][:, 0].any() and np.isnan(v["ke_slope"]).all()          # N / 2 = 4 < 8: no bins to fit at this size
    monkeypatch.delenv("QD_SPHARM")                              # the same run without the switch: no directory, no line
    monkeypatch.setenv("QD_OUTPUT_DIR", str(tmp_path / "out_off"))
    monkeypatch.setenv("QD_DATA_DIR", str(tmp_path / "off"))
    assert driver.main() == 0
    assert "[SphSpec]" not in capsys.readouterr().out and not os.path.exists(tmp_path / "out_off" / "spharm")


def test_resumed_run_writes_the_uncut_runs_files(gpu, tmp_path, monkeypatch, capsys):
    from qingdai_amd import driver, ncio
    monkeypatch.chdir(tmp_path)
    ck = dict(QD_CHECKPOINT="1", QD_SPHARM_EVERY="1")
    _set_env(monkeypatch, _env(tmp_path, "whole", 0.125, **ck))  # 30 steps: windows 0-11 and 12-23, 24-29 stays open
    assert driver.main() == 0
    whole = capsys.readouterr().out
    assert whole.count("[SphSpec] day ") == 2 and " 30 steps" in whole and "[Checkpoint] (final) wrote" in whole
    _set_env(monkeypatch, _env(tmp_path, "cut", 0.0625, **ck))   # 15 steps: stopped inside the window 12-23
    assert driver.main() == 0
    first = capsys.readouterr().out
    assert first.count("[SphSpec] day ") == 1 and " 15 steps" in first and "[Checkpoint] loaded" not in first
    assert driver.main() == 0
    second = capsys.readouterr().out
    assert "[Checkpoint] loaded" in second and "step 15" in second and second.count("[SphSpec] day ") == 1      # each file written once
    files = lambda d: sorted(os.listdir(tmp_path / ("out_" + d) / "spharm"))
    assert files("cut") == files("whole") and len(files("whole")) == 2
    for name in files("whole"):
        a, b = (open(tmp_path / ("out_" + d) / "spharm" / name, "rb").read() for d in ("whole", "cut"))
        assert a == b, name
        v, _ = ncio.read_nc(str(tmp_path / "out_whole" / "spharm" / name))
        assert int(v["complete"]) == 1 and len(v["step"]) == 12 and int(v["n_samples"]) == 12
    wa, wb = (ncio.read_nc(str(tmp_path / d / "checkpoint.nc")) for d in ("whole", "cut"))
    assert wa[1]["run_digest"] == wb[1]["run_digest"] and wa[1]["digest_SPHARM_SUMS"] == wb[1]["digest_SPHARM_SUMS"]
    for k in ("spharm_records", "spharm_times", "spharm_steps", "spharm_clock", "spharm_sums"):       # the open window 24-29 travels
        assert np.asarray(wa[0][k]).tobytes() == np.asarray(wb[0][k]).tobytes(), k
    assert wa[0]["spharm_clock"].tolist() == [30.0, 6.0, 6.0] and wa[0]["spharm_steps"].tolist() == [24.0, 25.0, 26.0, 27.0, 28.0, 29.0]
    assert wa[0]["spharm_sums"].shape == (3, 10, 10) and "spharm=VORT,DIV,H|every=1|2d=1" in wa[1]["subsystems"]
    _set_env(monkeypatch, _env(tmp_path, "cut", 0.0625, QD_CHECKPOINT="1", QD_SPHARM="0"))    # a lane-on file by a lane-off run
    assert driver.main() == 2
    assert "the subsystem set differs: the spharm lane is 'VORT,DIV,H|every=1|2d=1' in the file and '-' in this run" in capsys.readouterr().out
