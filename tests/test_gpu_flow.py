"""GPU (-m gpu): the flow lane (csrc/qd_flow.hip, qingdai_amd/flow.py): vorticity, divergence, streamfunction, velocity potential.

  1 the kernels alone through qd_flow_solve at the smallest shapes where each form can go wrong: 3 x 4 (one interior row), 5 x 4,
    19 x 36 (FFT passes 4 3 3), 9 x 45 (odd n, FFT), 7 x 35 and 7 x 26 (direct), 5 x 600 (more butterflies than threads), 131 x 12
    (the elimination walks past a wave's worth of rows), 19 x 36 under QD_FLOW_FORM=direct.  A handle has at least five rows
    (qd_create refuses fewer), so 3 x 4 runs the same kernels through qd_flow_solve_grid, the seam without a handle; 5 x 4 runs
    through both seams and gives the same bits.
      zeta, delta     flow.vortdiv_reference, bit for bit, pole rows included
      the record      flow.scalars_reference of the device's own planes, bit for bit
      psi, chi        against the extended-precision flow.helmholtz_reference.  The yardstick is measured, not fixed: the f64 NumPy
                      restatement's own max-relative error e64 = max |x64 - xext| / max |xext| at the same shape and winds; the device
                      may exceed it by a factor of 8 (its FFT sums in another order, and each reordering of a few dozen terms
                      legitimately moves a few ulps).  The pairs are printed, and DESIGN.md section 7 lists them.
      forms           FFT and direct form agree within the same bound
      a NaN           one NaN in U: psi and chi NaN in every cell, bad = 1; the clean solve behind it gives the first one's bits
  2 the lane at 19 x 36: a span against a cut span against single steps with a class-seam sample behind each, bitwise; lane off
    equals the state digest of a run that never heard of the lane; driver.main writes two windows and an open one with the
    documented variables; a run cut inside a window and resumed writes the uncut run's bytes; more samples than the log holds are
    refused with the lane's own text."""
import os
import re

import numpy as np
import pytest

from test_gpu_budget_diag import make, fetch, DT
from test_gpu_series import same, _set_env

pytestmark = pytest.mark.gpu

SHAPES = [(3, 4), (5, 4), (19, 36), (9, 45), (7, 35), (7, 26), (5, 600), (131, 12)]
CASES = [(s, "default") for s in SHAPES] + [((19, 36), "direct")]
FACTOR = 8.0
_REF, _GOT = {}, {}


def winds(shape):
    n_lat, n = shape
    r = np.random.default_rng(n_lat * 10000 + n)
    lat = np.deg2rad(np.linspace(-90, 90, n_lat))[:, None]
    return 8.0 * np.cos(lat) + 10.0 * r.normal(size=shape), 5.0 * r.normal(size=shape)


def reference(shape, g):
    """(u, v, the f64 restatement, the extended solve) of a shape, computed once."""
    from qingdai_amd import flow
    if shape not in _REF:
        u, v = winds(shape)
        _REF[shape] = (u, v, flow.helmholtz_reference(u, v, g), flow.helmholtz_reference(u, v, g, extended=True))
    return _REF[shape]


def relerr(x, ref):
    return float(np.abs(x - ref).max() / np.abs(ref).max())


def solve(shape, u, v, dev=None):
    """-> (zeta, delta, psi, chi, rec) from the device: through the handle's seam, or without a handle."""
    import qingdai_amd as qa
    from qingdai_amd import flow
    if dev is None:
        r = flow.solve_grid(qa.SphericalGrid(*shape), qa.QdParams().a, u, v)
        return r.zeta, r.delta, r.psi, r.chi, r.rec
    out = dev.flow_solve(u, v)
    recs = dev.flow_log()
    assert recs.shape == (1, flow.REC_W) and len(dev.flow_log()) == 0
    return out + (recs[0],)


@pytest.mark.parametrize("shape,form", CASES, ids=[f"{s[0]}x{s[1]}-{f}" for s, f in CASES])
def test_solve(gpu, monkeypatch, shape, form):
    import qingdai_amd as qa
    from qingdai_amd import flow
    from qingdai_amd.device import Device
    if form == "direct":
        monkeypatch.setenv("QD_FLOW_FORM", "direct")
    else:
        monkeypatch.delenv("QD_FLOW_FORM", raising=False)
    grid = qa.SphericalGrid(*shape)
    a = qa.QdParams().a
    g = flow.grid_tables(grid, a)
    u, v, r64, ext = reference(shape, g)
    dev = None
    if shape[0] >= 5:
        dev = Device(grid)
        assert dev.params.a == a
        dev.flow_configure(g)
    zeta, delta, psi, chi, rec = solve(shape, u, v, dev)
    assert same(zeta, r64.zeta) and same(delta, r64.delta), (shape, form)
    want = flow.scalars_reference(u, v, zeta, delta, psi, chi, g)
    assert np.array_equal(rec, want), (shape, form, dict(zip(flow.REC, zip(rec, want))))
    assert rec[flow.REC.index("bad_rows")] == 0 and np.isfinite(rec).all()
    for name, x, x64, xext in (("psi", psi, r64.psi, ext.psi), ("chi", chi, r64.chi, ext.chi)):
        e64, edev = relerr(x64, xext), relerr(x, xext)
        print(f"flow {shape[0]}x{shape[1]} {form} {name}: f64 restatement {e64:.3e} device {edev:.3e} ratio {edev / e64:.2f}")
        assert e64 > 0.0 and edev <= FACTOR * e64, (shape, form, name, e64, edev)
        assert abs(flow.weighted_mean(x, g)) <= 64 * np.finfo(float).eps * np.abs(x).max(), (shape, form, name)
    _GOT[(shape, form)] = (psi, chi)
    if (shape, "default") in _GOT and (shape, "direct") in _GOT:             # the two forms of one grid
        for q, (name, xext) in enumerate((("psi", ext.psi), ("chi", ext.chi))):
            d = float(np.abs(_GOT[(shape, "default")][q] - _GOT[(shape, "direct")][q]).max() / np.abs(xext).max())
            e64 = relerr((r64.psi, r64.chi)[q], xext)
            print(f"flow {shape[0]}x{shape[1]} fft against direct {name}: {d:.3e} ({d / e64:.2f} of the f64 restatement's error)")
            assert d <= FACTOR * e64, (shape, name, d, e64)
    if dev is None:
        return
    if shape == (5, 4):                                          # the seam without a handle runs the same kernels
        for x, y in zip(solve(shape, u, v), (zeta, delta, psi, chi, rec)):
            assert same(x, y)
    # one NaN in U: every cell of psi and chi, one bad row; nothing else is disturbed
    ub = u.copy()
    ub[shape[0] // 2, shape[1] // 3] = np.nan
    zb, db, pb, cb, rb = solve(shape, ub, v, dev)
    zw, dw = flow.vortdiv_reference(ub, v, g)
    assert same(zb, zw) and same(db, dw) and np.isnan(pb).all() and np.isnan(cb).all(), (shape, form)
    wantb = flow.scalars_reference(ub, v, zb, db, pb, cb, g)
    assert np.array_equal(rb, wantb, equal_nan=True) and rb[flow.REC.index("bad_rows")] == 1, (shape, form, rb, wantb)
    again = solve(shape, u, v, dev)
    for x, y in zip(again, (zeta, delta, psi, chi, rec)):
        assert same(x, y), (shape, form)
    sums, count = dev.flow_sums()                                # the class seam on host planes leaves the sums alone
    assert count == 0 and not sums.any()
    dev.close()


# ---------------------------------------------------------------- 2: the lane
def attach(sim, tmp_path, *, every=1, S=None, lane=True):
    """A Flow on the run's handle; lane=False: configured, but no participant of the spans (the class seam's twin)."""
    from qingdai_amd import flow
    days = flow.EVERY_DAYS if S is None else S * DT / sim.day_seconds
    sim.flow_lines = []
    f = flow.Flow(sim.dev, sim.grid, {"enabled": True, "every": every, "every_days": days}, dt=DT, day=sim.day_seconds,
                  out=sim.flow_lines.append, output_dir=str(tmp_path))
    assert S is None or f.S == S
    sim.flow = f if lane else None
    return f


@pytest.mark.parametrize("every", [1, 2])
def test_span_equals_single_steps(gpu, monkeypatch, tmp_path, every):
    from qingdai_amd import flow
    monkeypatch.delenv("QD_FLOW_FORM", raising=False)
    got = []
    for cuts in ([6], [2, 4]):
        sim = make(monkeypatch, 19, 36, routing=False)
        f = attach(sim, tmp_path, every=every)
        for n in cuts:
            sim.run_steps(n)
        recs, times, steps = f.window()
        assert steps.tolist() == list(range(0, 6, every)) and times.tolist() == [k * DT for k in range(0, 6, every)]
        got.append((recs, f.sums()))
        sim.dev.close()
    sim = make(monkeypatch, 19, 36, routing=False)
    f = attach(sim, tmp_path, every=every, lane=False)
    planes = []
    for i in range(6):
        sim.run_steps(1)
        if i % every == 0:
            sim.dev.flow_sample()
            w = fetch(sim.dev, ["U", "V"])
            planes.append((w["U"], w["V"]))
    got.append((sim.dev.flow_log(), sim.dev.flow_sums()))
    # a record is its own step's: the host-plane seam on the downloaded winds gives the lane's record, and the sums add up
    total = np.zeros((4, 19, 36))
    for k, (u, v) in enumerate(planes):
        zeta, delta, psi, chi = sim.dev.flow_solve(u, v)
        assert same(sim.dev.flow_log()[0], got[0][0][k]), (every, k)
        total = total + np.stack([psi, chi, zeta, delta])
    sim.dev.close()
    assert got[0][0].shape == (6 // every, flow.REC_W) and got[0][1][0].shape == (4, 19, 36)
    for k, (recs, (sums, count)) in enumerate(got):
        assert same(recs, got[0][0]) and same(sums, got[0][1][0]) and count == 6 // every, (every, k)
    assert same(total, got[0][1][0])
    assert np.isfinite(got[0][0]).all() and not got[0][0][:, -1].any()
    assert all(not np.array_equal(got[0][0][i], got[0][0][i + 1]) for i in range(6 // every - 1))
    assert not os.path.exists(tmp_path / "flow") and sim.flow_lines == []


def test_lane_off_equals_the_parent_digest_and_refusals(gpu, monkeypatch, tmp_path):
    from qingdai_amd._lib import C, QdError
    monkeypatch.delenv("QD_FLOW_FORM", raising=False)
    runs = {}
    for on in (False, True):
        sim = make(monkeypatch, 19, 36, routing=False)
        if on:
            attach(sim, tmp_path / "on", S=3)
        sim.dev.timing(True)
        for n in (3, 4):
            sim.run_steps(n)
        sim.dev.sync()
        launches = [sim.dev.timing_get(k)[1] for k in ("flow_vortdiv", "flow_fwd", "flow_lat", "flow_inv", "flow_finish", "flow_record")]
        sim.dev.timing(False)
        runs[on] = dict(digest=sim.digest(), launches=launches, lines=list(getattr(sim, "flow_lines", [])),
                        files=sorted(os.listdir(tmp_path / "on" / "flow")) if on else None)
        if not on:
            with pytest.raises(QdError, match="qd_state_digest: ref FLOW_SUMS: the flow lane is not configured"):
                sim.dev.digest(["FLOW_SUMS"])
            for call in (sim.dev.flow_sample, sim.dev.flow_log, sim.dev.flow_reset, lambda: sim.dev.flow_schedule([1]), sim.dev.flow_sums):
                with pytest.raises(QdError, match="not configured"):
                    call()
        else:
            # more samples than the log holds, the wrong schedule length: refused with the lane's own text, nothing runs
            cap = C["QD_FLOW_LOG_CAP"]
            flags = dict(with_ocean=True, with_physics=True, pass_albedo=False, with_hydrology=True)
            stars = sim.forcing.star_table(DT * np.arange(cap + 1))
            counters = sim.dev.counters()
            sim.dev.flow_schedule(np.ones(cap + 1, dtype=np.int32))
            with pytest.raises(QdError, match=r"qd_step_n: the span's flow records would overflow the log of QD_FLOW_LOG_CAP \(drain it "
                                              r"with qd_flow_log first\)"):
                sim.dev.step_n(stars, DT, **flags)
            sim.dev.flow_schedule([1, 1, 1])
            with pytest.raises(QdError, match="a qd_flow_schedule must cover exactly the n steps of the span"):
                sim.dev.step_n(stars[:2], DT, **flags)
            assert sim.dev.counters() == counters and len(sim.dev.flow_log()) == 0
        sim.dev.close()
    off, on = runs[False], runs[True]
    assert off["launches"] == [0] * 6 and on["launches"] == [7] * 6          # six launches per sampled step, none without the lane
    assert len(on["files"]) == 2 and len(on["lines"]) == 2 and all(s.startswith("[Flow] day ") for s in on["lines"])
    d_on = {k: v for k, v in on["digest"].items() if k not in ("FLOW_SUMS", "run")}
    d_off = {k: v for k, v in off["digest"].items() if k != "run"}
    assert d_on == d_off and len(d_off) > 20 and "FLOW_SUMS" in on["digest"] and "FLOW_SUMS" not in off["digest"]


def _env(tmp_path, data, days, **extra):
    e = {"QD_N_LAT": "19", "QD_N_LON": "36", "QD_DT_SECONDS": "300", "QD_SIM_DAYS": str(days), "QD_DYN_DIAG_PRINT": "0", "QD_ECO_ENABLE": "0",
         "QD_HYDRO_ENABLE": "0", "QD_USE_OCEAN": "1", "QD_DATA_DIR": str(tmp_path / data), "QD_OUTPUT_DIR": str(tmp_path / ("out_" + data)),
         "QD_FLOW": "1", "QD_FLOW_EVERY_DAYS": "0.05", "QD_FLOW_EVERY": "2"}
    e.update(extra)
    return e


def test_driver_main(gpu, tmp_path, monkeypatch, capsys):
    from qingdai_amd import driver, flow, ncio
    monkeypatch.chdir(tmp_path)
    _set_env(monkeypatch, _env(tmp_path, "on", 0.125))           # 30 steps: windows 0-11 and 12-23, 24-29 is written open
    assert driver.main() == 0
    out = capsys.readouterr().out
    lines = [s for s in out.splitlines() if s.startswith("[Flow]")]
    assert len(lines) == 3 and [int(re.search(r": (\d+) samples", s).group(1)) for s in lines] == [6, 6, 3], out
    assert all(re.fullmatch(r"\[Flow\] day \d+\.\d+–\d+\.\d+: \d+ samples \| vort rms=\S+→\S+ div rms=\S+→\S+ KE=\S+ rot=\S+ div=\S+ bad=0", s)
               for s in lines), lines
    d = tmp_path / "out_on" / "flow"
    files = sorted(os.listdir(d))
    assert len(files) == 3 and all(re.fullmatch(r"flow_day_\d+\.\d+_\d+\.\d+\.nc", f) for f in files), files
    for f, (steps, complete) in zip(files, ((range(0, 12, 2), 1), (range(12, 24, 2), 1), (range(24, 30, 2), 0))):
        v, _ = ncio.read_nc(str(d / f))
        steps = list(steps)
        assert v["step"].tolist() == steps and v["time_seconds"].tolist() == [k * DT for k in steps], f
        assert (int(v["complete"]), int(v["sample_every"]), int(v["n_samples"]), float(v["dt_seconds"])) == (complete, 2, len(steps), DT)
        assert set(v) == ({"time_seconds", "step", "lat", "lon", "dt_seconds", "sample_every", "n_samples", "complete"} | set(flow.REC) |
                          {"psi_mean", "chi_mean", "vort_mean", "div_mean"})
        for name in ("psi_mean", "chi_mean", "vort_mean", "div_mean"):
            assert v[name].shape == (19, 36) and np.isfinite(v[name]).all() and v[name].any(), (f, name)
        for name in flow.REC:
            assert v[name].shape == (len(steps),) and np.isfinite(v[name]).all(), (f, name)
        assert (v["ke_rot"] > 0).all() and (v["ke"] > 0).all() and (v["vort_rms"] > 0).all() and not v["bad_rows"].any()
        assert (v["psi_min"] < 0).all() and (v["psi_max"] > 0).all()
        # the window mean of vorticity, weighted like a record, is the mean of the records' global means up to rounding
        g = flow.grid_tables(types_grid(19, 36), 1.0)
        assert abs(flow.weighted_mean(v["vort_mean"], g) - v["vort_global"].mean()) <= 1e-12 * v["vort_rms"].max()
    monkeypatch.delenv("QD_FLOW")                                # the same run without the switch: no directory, no line
    monkeypatch.setenv("QD_OUTPUT_DIR", str(tmp_path / "out_off"))
    monkeypatch.setenv("QD_DATA_DIR", str(tmp_path / "off"))
    assert driver.main() == 0
    assert "[Flow]" not in capsys.readouterr().out and not os.path.exists(tmp_path / "out_off" / "flow")


def types_grid(n_lat, n_lon):
    import qingdai_amd as qa
    return qa.SphericalGrid(n_lat, n_lon)


def test_resumed_run_writes_the_uncut_runs_files(gpu, tmp_path, monkeypatch, capsys):
    from qingdai_amd import driver, ncio
    monkeypatch.chdir(tmp_path)
    ck = dict(QD_CHECKPOINT="1", QD_FLOW_EVERY="1")
    _set_env(monkeypatch, _env(tmp_path, "whole", 0.125, **ck))  # 30 steps: windows 0-11 and 12-23, 24-29 stays open
    assert driver.main() == 0
    whole = capsys.readouterr().out
    assert whole.count("[Flow] day ") == 2 and " 30 steps" in whole and "[Checkpoint] (final) wrote" in whole
    _set_env(monkeypatch, _env(tmp_path, "cut", 0.0625, **ck))   # 15 steps: stopped inside the window 12-23
    assert driver.main() == 0
    first = capsys.readouterr().out
    assert first.count("[Flow] day ") == 1 and " 15 steps" in first and "[Checkpoint] loaded" not in first
    assert driver.main() == 0
    second = capsys.readouterr().out
    assert "[Checkpoint] loaded" in second and "step 15" in second and second.count("[Flow] day ") == 1       # each file written once
    files = lambda d: sorted(os.listdir(tmp_path / ("out_" + d) / "flow"))
    assert files("cut") == files("whole") and len(files("whole")) == 2
    for name in files("whole"):
        a, b = (open(tmp_path / ("out_" + d) / "flow" / name, "rb").read() for d in ("whole", "cut"))
        assert a == b, name
        v, _ = ncio.read_nc(str(tmp_path / "out_whole" / "flow" / name))
        assert int(v["complete"]) == 1 and len(v["step"]) == 12 and int(v["n_samples"]) == 12
    wa, wb = (ncio.read_nc(str(tmp_path / d / "checkpoint.nc")) for d in ("whole", "cut"))
    assert wa[1]["run_digest"] == wb[1]["run_digest"] and wa[1]["digest_FLOW_SUMS"] == wb[1]["digest_FLOW_SUMS"]
    for k in ("flow_records", "flow_times", "flow_steps", "flow_clock", "flow_sums"):       # the open window 24-29 travels
        assert np.asarray(wa[0][k]).tobytes() == np.asarray(wb[0][k]).tobytes(), k
    assert wa[0]["flow_clock"].tolist() == [30.0, 6.0, 6.0] and wa[0]["flow_steps"].tolist() == [24.0, 25.0, 26.0, 27.0, 28.0, 29.0]
    assert wa[0]["flow_sums"].shape == (4, 19, 36) and "flow=every=1" in wa[1]["subsystems"]
    _set_env(monkeypatch, _env(tmp_path, "cut", 0.0625, QD_CHECKPOINT="1", QD_FLOW="0"))    # a lane-on file by a lane-off run
    assert driver.main() == 2
    assert "the subsystem set differs: the flow lane is 'every=1' in the file and '-' in this run" in capsys.readouterr().out
