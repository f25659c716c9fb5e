"""GPU (-m gpu): the eddy lane (csrc/qd_eddy.hip, qingdai_amd/eddy.py).

  1 k_eddy_accum alone through qd_eddy_sample, planes fed with Device.set, bit for bit against eddy.accumulate_reference: 5 x 5 (odd
    grid: the scalar tail), 6 x 63, 7 x 64, 7 x 256, 9 x 257, 10 x 600; 1 field / 1 pair, 5 / 8 (the default list's shape), 16 / 32
    (the limits: the LDS form of 16 fields) and six variances; three samples each (the first-sample path and the steady path); planes
    that hold NaN, +-inf, -0.0 and a product that overflows.  k_eddy_zonal bit for bit against eddy.zonal_reference at the series
    lane's row shapes (below, at and above one and two trips of a wave).  Every refusal with its text.
  2 the lane at 19 x 36: one 7-step span against seven one-step spans whose fields are downloaded and fed to accumulate_reference, and
    against the class seam; the model's digest equals that of a run without the lane (with and without the ocean, sample_every 1
    and 3, QD_FUSED=0); chunkings with the routing, budget and history lanes on; a window inside run_steps; OLR inside a span without
    the hydrology bit; the other lanes' files; one launch per sampled step; driver.main; a run cut inside a window and resumed."""
import ctypes
import os
import re

import numpy as np
import pytest

from test_gpu_budget_diag import make, fetch, DT
from test_gpu_series import same, _set_env

pytestmark = pytest.mark.gpu

SHAPES = [(5, 5), (6, 63), (7, 64), (7, 256), (9, 257), (10, 600)]
ZONAL_SHAPES = [(5, 5), (6, 63), (7, 64), (9, 130), (9, 257)]
POOL = ("U", "V", "TS", "Q", "H", "CLOUD", "HICE", "ALBEDO", "OLR", "W_LAND", "UO", "VO", "ETA", "SST", "LH", "EFLUX")


def configurations():
    """name -> (fields, pairs)"""
    from qingdai_amd import eddy
    f5, p8, _ = eddy.parse_pairs(eddy.DEFAULT_PAIRS)
    p32 = [(i, j) for i in range(16) for j in range(i, 16) if (i * 7 + j * 3) % 4 == 0][:31] + [(15, 2)]      # q < p too
    return {"1x1": (["TS"], [(0, 0)]), "5x8": (f5, p8), "16x32": (list(POOL), p32),
            "variances": (list(POOL[:6]), [(k, k) for k in range(6)])}


def sample_values(shape, fields, t):
    """Sample t of every field: magnitudes over eight orders around a mean; from sample 0 on the second field holds a NaN, the third
    +inf and -inf, the fourth is all -0.0 in sample 0 and +0.0 later, the fifth holds 1e200 against an anchor of -1e200 (d * d
    overflows); the last cell of the grid is special in the first field (the scalar tail of an odd grid)."""
    r = np.random.default_rng(shape[0] * 100000 + shape[1] * 10 + t)
    n = shape[0] * shape[1]
    v = {}
    for k, name in enumerate(fields):
        x = 300.0 * (k % 3) + r.normal(size=shape) * 10.0 ** r.integers(-4, 3, size=shape)
        if k == 1:
            x.flat[n // 3] = np.nan
        if k == 2:
            x.flat[n // 2], x.flat[n // 2 + 1] = np.inf, -np.inf if t < 2 else np.inf
        if k == 3:
            x[:] = -0.0 if t == 0 else 0.0
        if k == 4:
            x.flat[1] = -1e200 if t == 0 else 1e200
        if k == 0:
            x.flat[n - 1] = (-1.0) ** t * 1e-300
        v[name] = x
    return v


@pytest.mark.parametrize("shape", SHAPES)
def test_kernel_alone(gpu, shape):
    import qingdai_amd as qa
    from qingdai_amd import eddy
    from qingdai_amd.device import Device
    dev = Device(qa.SphericalGrid(*shape))
    for name, (fields, pairs) in configurations().items():
        dev.eddy_configure(fields, pairs)
        state, samples = None, []
        for t in range(3):
            v = sample_values(shape, fields, t)
            for f, x in v.items():
                dev.set(f, x)
            dev.eddy_sample()
            samples.append(np.stack([v[f] for f in fields]))
            r, S, Cs, count = dev.eddy_read()
            state = eddy.accumulate_reference(samples[-1:], pairs, state=state)
            assert count == state[3] == t + 1
            for what, got, want in (("anchors", r, state[0]), ("sums", S, state[1]), ("pair sums", Cs, state[2])):
                assert same(got, want), (shape, name, t, what, np.argwhere(~(np.asarray(got).view(np.int64) == np.asarray(want).view(np.int64)))[:4])
        whole = eddy.accumulate_reference(samples, pairs)
        assert all(same(a, b) for a, b in zip(whole[:3], state[:3]))
        if len(fields) >= 5:                                     # the special values came through as the definition says
            assert np.isnan(S[1].flat[shape[0] * shape[1] // 3]) and np.isnan(S[2].flat[shape[0] * shape[1] // 2])      # inf - inf
            assert not S[3].any() and not np.signbit(S[3]).any()                     # -0.0 - -0.0 = +0.0, and + +0.0
            k = [i for i, pq in enumerate(pairs) if pq == (4, 4)]
            assert S[4].flat[1] == 4e200 and (not k or Cs[k[0]].flat[1] == np.inf)
        dev.eddy_reset()                                         # a reset: the next sample is a window's first again
        dev.eddy_sample()
        r, S, Cs, count = dev.eddy_read()
        with np.errstate(invalid="ignore"):
            zero = samples[-1] - samples[-1]                      # +0.0, NaN where the sample is not finite
        assert count == 1 and same(r, samples[-1]) and same(S, zero) and not np.nan_to_num(Cs, nan=0.0, posinf=0.0).any()
    dev.eddy_configure([], [])                                   # releases
    from qingdai_amd._lib import QdError
    with pytest.raises(QdError, match="eddy: not configured"):
        dev.eddy_sample()
    dev.close()


@pytest.mark.parametrize("shape", ZONAL_SHAPES)
def test_zonal_sums(gpu, shape):
    import qingdai_amd as qa
    from qingdai_amd import eddy
    from qingdai_amd.device import Device
    dev = Device(qa.SphericalGrid(*shape))
    for name in ("5x8", "16x32"):
        fields, pairs = configurations()[name]
        dev.eddy_configure(fields, pairs)
        for t in range(3):
            for f, x in sample_values(shape, fields, t).items():
                dev.set(f, x)
            dev.eddy_sample()
        _, S, Cs, _ = dev.eddy_read()
        got = dev.eddy_zonal()
        assert got.shape == (len(pairs), 4, shape[0]) and same(got, eddy.zonal_reference(S, Cs, pairs)), (shape, name)
        assert np.isfinite(got).any() and np.isnan(got).any()
        assert same(dev.eddy_zonal(), got)                        # reading does not move the state
    dev.close()


def test_refusals(gpu, monkeypatch):
    import qingdai_amd as qa
    from qingdai_amd._lib import F, QdError
    from qingdai_amd.device import Device
    from qingdai_amd.ecology import EcologyAdapter
    sim = make(monkeypatch, 19, 36, routing=False)
    dev = sim.dev
    ids = [F[n] for n in POOL]
    raw = lambda fields, p, q: dev.call("qd_eddy_configure", len(fields), fields, len(p), p, q)
    for call in (dev.eddy_sample, dev.eddy_read, dev.eddy_zonal, dev.eddy_reset, lambda: dev.eddy_schedule([1]),
                 lambda: dev.call("qd_eddy_restore", np.zeros(1), np.zeros(1), np.zeros(1), 0)):
        with pytest.raises(QdError, match=r"eddy: not configured \(qd_eddy_configure first\)"):
            call()
    for ref in ("EDDY_SUMS", "EDDY_ANCHORS"):
        with pytest.raises(QdError, match=f"qd_state_digest: ref {ref}: the eddy statistics are not configured"):
            dev.digest([ref])
    for args, why in (((([9999], [0], [0])), "eddy: field 0 is not an f64 plane"),
                      (([F["TS"], -1], [0], [1]), "eddy: field 1 is not an f64 plane"),
                      (([F["LAND_MASK"]], [0], [0]), "eddy: field 0 is not an f64 plane"),
                      (([F["V"], F["PRECIP"]], [0], [1]), "eddy: PRECIP is sampled in front of the ocean step, every other field behind the "
                                                           "step's last launch: a product across the two places has no meaning"),
                      (([F["U"], F["V"], F["U"]], [0], [1]), "eddy: field 2 is named twice"),
                      (([F["U"], F["V"]], [0, 1], [1, 2]), "eddy: pair 1 has an index outside the 2 fields"),
                      (([F["U"], F["V"]], [0, -1], [1, 0]), "eddy: pair 1 has an index outside the 2 fields"),
                      (([F["U"], F["V"]], [0, 1, 0], [1, 1, 1]), r"eddy: pair 2 is pair 0 again \(the order of the two fields does not count\)"),
                      (([F["U"], F["V"]], [0, 1], [1, 0]), "eddy: pair 1 is pair 0 again"),
                      ((ids + [F["QNET"]], [0], [0]), "eddy: at most 16 fields"),
                      ((ids, [0] * 33, list(range(16)) * 2 + [0]), "eddy: at most 32 pairs"),
                      (([F["U"]], [], []), "eddy: no pair")):
        with pytest.raises(QdError, match=why):
            raw(*args)
    with pytest.raises(QdError, match="eddy: not configured"):   # none of the refused calls left a configuration
        dev.eddy_read()
    # a span: the wrong schedule length is refused with the lane's own text, nothing runs, and the schedule is gone
    dev.eddy_configure(["TS", "ECO_LAI"], [(0, 1)])
    flags = dict(with_ocean=True, with_physics=True, pass_albedo=False, with_hydrology=True)
    stars = sim.forcing.star_table(DT * np.arange(3))
    counters = dev.counters()
    dev.eddy_schedule([1, 1, 1])
    with pytest.raises(QdError, match="eddy: qd_step_n: a qd_eddy_schedule must cover exactly the n steps of the span"):
        dev.step_n(stars[:2], DT, **flags)
    assert dev.counters() == counters and dev.eddy_read()[3] == 0
    with pytest.raises(QdError, match="eddy: qd_eddy_restore: negative sample count"):
        dev.eddy_restore(*dev.eddy_read()[:3], -1)
    # a map the ecology turns into an f32 slab behind the configure: found at span begin and at the class seam
    monkeypatch.setenv("QD_ECO_DIAG", "0")
    eco = EcologyAdapter(sim.grid, sim.land_mask, dev=dev, f32_maps=True)
    assert int(eco.params.map_f32) == 1
    dev.eddy_schedule([1, 1])
    with pytest.raises(QdError, match=r"eddy: a field is no longer an f64 plane \(qd_eddy_configure again\)"):
        dev.step_n(stars[:2], DT, **flags)
    with pytest.raises(QdError, match="eddy: a field is no longer an f64 plane"):
        dev.eddy_sample()
    assert dev.counters() == counters and dev.eddy_read()[3] == 0
    with pytest.raises(QdError, match="eddy: field 1 is not an f64 plane"):
        dev.eddy_configure(["TS", "ECO_LAI"], [(0, 1)])
    dev.close()
    # a band handle
    band = Device(qa.SphericalGrid(73, 144), row0=20, n_rows=30, halo=6)
    one = (ctypes.c_int32 * 1)
    rc = band.lib.qd_eddy_configure(band.h, 1, one(F["TS"]), 1, one(0), one(0))
    assert rc != 0 and b"eddy: the eddy statistics need a whole-globe handle" in band.lib.qd_last_error(band.h)
    assert b"latitude bands are not supported" in band.lib.qd_last_error(band.h)
    band.close()


# ---------------------------------------------------------------- 2: the lane
def attach(sim, tmp_path, *, every=1, S=None, pairs=None, maps=True, lane=True):
    """An Eddy on the run's handle; lane=False: configured, but no participant of the spans (the class seam's twin)."""
    from qingdai_amd import eddy
    days = eddy.EVERY_DAYS if S is None else S * DT / sim.day_seconds
    sim.eddy_lines = []
    e = eddy.Eddy(sim.dev, sim.grid, {"enabled": True, "pairs": pairs or eddy.DEFAULT_PAIRS, "sample_every": every, "every_days": days,
                                      "maps": maps}, with_ocean=sim.ocean is not None, dt=DT, day=sim.day_seconds,
                  out=sim.eddy_lines.append, output_dir=str(tmp_path))
    assert S is None or e.S == S
    sim.eddy = e if lane else None
    return e


def model_digest(sim):
    return {k: v for k, v in sim.digest().items() if k not in ("EDDY_SUMS", "EDDY_ANCHORS", "run")}


def state_same(a, b):
    return a[3] == b[3] and all(same(x, y) for x, y in zip(a[:3], b[:3]))


@pytest.mark.parametrize("ocean,every,fused", [(True, 1, None), (True, 3, None), (False, 1, None), (False, 3, None), (True, 1, "0"), (True, 3, "0")])
def test_span_equals_single_steps(gpu, monkeypatch, tmp_path, ocean, every, fused):
    from qingdai_amd import eddy
    env = {} if fused is None else {"QD_FUSED": fused}
    pairs = eddy.DEFAULT_PAIRS + (",VO*SST,SST*SST" if ocean else "")
    sim = make(monkeypatch, 19, 36, ocean=ocean, routing=False, env=env)
    e = attach(sim, tmp_path, every=every, pairs=pairs)
    sim.run_steps(7)                                             # one span
    span, span_digest = sim.dev.eddy_read(), model_digest(sim)
    assert "EDDY_SUMS" in sim.digest() and "EDDY_ANCHORS" in sim.digest() and (e.i, e.n_open) == (7, len(range(0, 7, every)))
    sim.dev.close()
    sim = make(monkeypatch, 19, 36, ocean=ocean, routing=False, env=env)
    e = attach(sim, tmp_path, every=every, pairs=pairs, lane=False)
    samples = []
    for i in range(7):                                           # seven one-step spans, the class seam behind each sampled one
        sim.run_steps(1)
        if i % every == 0:
            w = fetch(sim.dev, e.fields)
            samples.append(np.stack([w[f] for f in e.fields]))
            sim.dev.eddy_sample()
    seam = sim.dev.eddy_read()
    sim.dev.close()
    want = eddy.accumulate_reference(samples, e.pairs)
    assert state_same(span, want) and state_same(seam, want), (ocean, every, fused)
    assert span[3] == len(samples) == len(range(0, 7, every)) and np.isfinite(span[2]).all() and all(c.any() for c in span[2])
    sim = make(monkeypatch, 19, 36, ocean=ocean, routing=False, env=env)
    sim.run_steps(7)                                             # the same span without the lane: the model does not notice
    assert "EDDY_SUMS" not in sim.digest() and model_digest(sim) == span_digest and len(span_digest) > 20
    sim.dev.close()


FIRES = {0: 3, 2: 1, 5: 3}


def test_chunkings_with_the_other_lanes_and_a_window_inside_a_run(gpu, monkeypatch, tmp_path):
    from qingdai_amd import eddy, ncio
    from test_gpu_history import attach as attach_history
    runs = {}
    for name, cuts in (("whole", (7,)), ("two", (3, 4)), ("single", (1,) * 7), ("off", (7,))):
        out = tmp_path / name
        sim = make(monkeypatch, 19, 36, fires=FIRES)
        assert sim.routing is not None and sim.budget is not None
        attach_history(sim, out, S=4)
        e = attach(sim, out, S=4) if name != "off" else None
        sim.dev.timing(True)
        samples = []
        for n in cuts:
            sim.run_steps(n)
            if name == "single":
                w = fetch(sim.dev, e.fields)
                samples.append(np.stack([w[f] for f in e.fields]))
        sim.dev.sync()
        launches = sim.dev.timing_get("eddy")[1]
        sim.dev.timing(False)
        hist = sorted(os.listdir(out / "history"))
        runs[name] = dict(state=sim.dev.eddy_read() if e else None, digest=model_digest(sim), launches=launches, samples=samples,
                          lines=list(sim.eddy_lines) if e else [], hist=[open(out / "history" / f, "rb").read() for f in hist],
                          hist_sums=sim.dev.history_read(), budget=list(sim.budget_lines), history=list(sim.history_lines),
                          files=sorted(os.listdir(out / "eddy")) if os.path.exists(out / "eddy") else None, e=e)
        sim.dev.close()
    whole, off = runs["whole"], runs["off"]
    # a 4-step window inside run_steps(7): one file behind step 3, steps 4-6 stand in the planes
    samples = runs["single"]["samples"]
    pairs = whole["e"].pairs
    assert state_same(whole["state"], eddy.accumulate_reference(samples[4:], pairs)) and whole["state"][3] == 3
    for name in ("two", "single"):
        assert state_same(runs[name]["state"], whole["state"]), name
        assert runs[name]["files"] == whole["files"] and runs[name]["lines"] == whole["lines"] and runs[name]["digest"] == whole["digest"]
        for f in whole["files"]:
            assert open(tmp_path / name / "eddy" / f, "rb").read() == open(tmp_path / "whole" / "eddy" / f, "rb").read(), (name, f)
    assert len(whole["files"]) == 1 and len(whole["lines"]) == 1 and whole["lines"][0].startswith("[Eddy] day ")
    v, _ = ncio.read_nc(str(tmp_path / "whole" / "eddy" / whole["files"][0]))
    r, S, Cs, N = eddy.accumulate_reference(samples[:4], pairs)
    parts = eddy.decompose(eddy.zonal_reference(S, Cs, pairs), N, eddy.time_means(r, S, N), pairs)
    assert int(v["n_samples"]) == 4 and int(v["complete"]) == 1
    for k, (A, B) in enumerate(whole["e"].labels):
        for part in eddy.PARTS:
            assert same(v[f"{A}_{B}_{part}".lower()], parts[part][k]), (A, B, part)
    assert same(v["u_v_cov"], eddy.covariance_maps(S, Cs, pairs, N)[0]) and same(v["ts_mean"], eddy.time_means(r, S, N)[2])
    # the other lanes and the model do not notice; no eddy scope at 0, one launch per sampled step otherwise
    assert off["launches"] == 0 and off["files"] is None and whole["launches"] == runs["two"]["launches"] == runs["single"]["launches"] == 7
    assert whole["hist"] == off["hist"] and len(off["hist"]) == 1 and whole["budget"] == off["budget"] and len(off["budget"]) > 0
    assert whole["history"] == off["history"] and whole["digest"] == off["digest"] and len(off["digest"]) > 20
    assert whole["hist_sums"][1] == off["hist_sums"][1] == 3 and whole["hist_sums"][0].tobytes() == off["hist_sums"][0].tobytes()


def test_one_launch_per_sampled_step(gpu, monkeypatch, tmp_path):
    sim = make(monkeypatch, 19, 36, routing=False)
    attach(sim, tmp_path, every=3, S=5)
    sim.dev.timing(True)
    sim.run_steps(12)                                            # windows 0-4, 5-9, 10-11: positions 0 and 3 of each are sampled
    sim.dev.sync()
    assert sim.dev.timing_get("eddy")[1] == 5 and len(sim.eddy_lines) == 2 and sim.dev.eddy_read()[3] == 1
    assert [int(re.search(r": (\d+) samples", s).group(1)) for s in sim.eddy_lines] == [2, 2]
    sim.dev.timing(False)
    sim.dev.close()


def test_lazy_diagnostic_inside_a_span(gpu, monkeypatch, tmp_path):
    """Device.step_n without the hydrology bit: inside a span only the last step stores OLR -- unless a reader comes with the span."""
    from qingdai_amd import eddy
    flags = dict(with_ocean=True, with_physics=True, pass_albedo=False, with_hydrology=False)
    a = make(monkeypatch, 19, 36, routing=False)
    stars = a.forcing.star_table(DT * np.arange(5))
    samples = []
    for i in range(5):
        a.dev.step_n(stars[i:i + 1], DT, **flags)
        w = fetch(a.dev, ["OLR", "TS"])
        samples.append(np.stack([w["OLR"], w["TS"]]))
    a.dev.close()
    b = make(monkeypatch, 19, 36, routing=False)
    e = attach(b, tmp_path, pairs="OLR*TS,OLR*OLR")
    b.dev.step_n(stars, DT, eddy=e, **flags)
    got = b.dev.eddy_read()
    assert e.i == 5 and state_same(got, eddy.accumulate_reference(samples, e.pairs))
    assert all(not np.array_equal(samples[i][0], samples[i + 1][0]) for i in range(4)) and got[2][1].any()
    b.dev.close()


def _env(tmp_path, data, days, **extra):
    e = {"QD_N_LAT": "19", "QD_N_LON": "36", "QD_DT_SECONDS": "300", "QD_SIM_DAYS": str(days), "QD_DYN_DIAG_PRINT": "0", "QD_ECO_ENABLE": "0",
         "QD_HYDRO_ENABLE": "0", "QD_USE_OCEAN": "1", "QD_DATA_DIR": str(tmp_path / data), "QD_OUTPUT_DIR": str(tmp_path / ("out_" + data)),
         "QD_EDDY": "1", "QD_EDDY_EVERY_DAYS": "0.05", "QD_EDDY_SAMPLE_EVERY": "2"}
    e.update(extra)
    return e


def test_driver_main(gpu, tmp_path, monkeypatch, capsys):
    from qingdai_amd import driver, eddy, ncio
    monkeypatch.chdir(tmp_path)
    _set_env(monkeypatch, _env(tmp_path, "on", 0.125))           # 30 steps: windows 0-11 and 12-23, 24-29 is written open
    assert driver.main() == 0
    out = capsys.readouterr().out
    lines = [s for s in out.splitlines() if s.startswith("[Eddy]")]
    assert len(lines) == 3 and [int(re.search(r": (\d+) samples", s).group(1)) for s in lines] == [6, 6, 3], out
    assert all(re.fullmatch(r"\[Eddy\] day \d+\.\d+–\d+\.\d+: \d+ samples \| U\*V transient max \|\.\| at lat -?\d+\.\d+: \S+", s) for s in lines), lines
    d = tmp_path / "out_on" / "eddy"
    files = sorted(os.listdir(d))
    assert len(files) == 3 and all(re.fullmatch(r"eddy_day_\d+\.\d+_\d+\.\d+\.nc", f) for f in files), files
    fields, pairs, labels = eddy.parse_pairs(eddy.DEFAULT_PAIRS)
    names = {f"{a}_{b}_{part}".lower() for a, b in labels for part in eddy.PARTS + ("cov",)} | {f"{f}_mean".lower() for f in fields}
    for f, (n, complete) in zip(files, ((6, 1), (6, 1), (3, 0))):
        v, _ = ncio.read_nc(str(d / f))
        assert set(v) == names | {"lat", "lon", "n_samples", "t_start_seconds", "t_end_seconds", "dt_seconds", "sample_every", "maps", "complete"}
        assert (int(v["n_samples"]), int(v["complete"]), int(v["sample_every"]), int(v["maps"]), float(v["dt_seconds"])) == (n, complete, 2, 1, DT)
        for a, b in labels:
            p = f"{a}_{b}".lower()
            assert v[p + "_total"].shape == (19,) and v[p + "_cov"].shape == (19, 36) and np.isfinite(v[p + "_total"]).all()
            assert np.array_equal(v[p + "_total"], (v[p + "_mean"] + v[p + "_stationary"]) + v[p + "_transient"])
            np.testing.assert_allclose(v[p + "_transient"], v[p + "_cov"].mean(axis=1), rtol=1e-6, atol=1e-12 * np.abs(v[p + "_cov"]).max())
        assert v["u_u_transient"].any() and v["u_u_transient"].max() > 0 and (v["ts_mean"] > 150).all()
    monkeypatch.delenv("QD_EDDY")                                # the same run without the switch: no directory, no line
    monkeypatch.setenv("QD_OUTPUT_DIR", str(tmp_path / "out_off"))
    monkeypatch.setenv("QD_DATA_DIR", str(tmp_path / "off"))
    assert driver.main() == 0
    assert "[Eddy]" not in capsys.readouterr().out and not os.path.exists(tmp_path / "out_off" / "eddy")


def test_resumed_run_writes_the_uncut_runs_files(gpu, tmp_path, monkeypatch, capsys):
    from qingdai_amd import driver, eddy, ncio
    monkeypatch.chdir(tmp_path)
    ck = dict(QD_CHECKPOINT="1", QD_EDDY_SAMPLE_EVERY="1")
    _set_env(monkeypatch, _env(tmp_path, "whole", 0.125, **ck))  # 30 steps: windows 0-11 and 12-23, 24-29 stays open
    assert driver.main() == 0
    whole = capsys.readouterr().out
    assert whole.count("[Eddy] day ") == 2 and " 30 steps" in whole and "[Checkpoint] (final) wrote" in whole
    _set_env(monkeypatch, _env(tmp_path, "cut", 0.0625, **ck))   # 15 steps: stopped inside the window 12-23
    assert driver.main() == 0
    first = capsys.readouterr().out
    assert first.count("[Eddy] day ") == 1 and " 15 steps" in first and "[Checkpoint] loaded" not in first
    assert driver.main() == 0
    second = capsys.readouterr().out
    assert "[Checkpoint] loaded" in second and "step 15" in second and second.count("[Eddy] day ") == 1      # each file written once
    files = lambda d: sorted(os.listdir(tmp_path / ("out_" + d) / "eddy"))
    assert files("cut") == files("whole") and len(files("whole")) == 2
    for name in files("whole"):
        a, b = (open(tmp_path / ("out_" + d) / "eddy" / name, "rb").read() for d in ("whole", "cut"))
        assert a == b, name
        v, _ = ncio.read_nc(str(tmp_path / "out_whole" / "eddy" / name))
        assert int(v["complete"]) == 1 and int(v["n_samples"]) == 12
    wa, wb = (ncio.read_nc(str(tmp_path / d / "checkpoint.nc")) for d in ("whole", "cut"))
    assert wa[1]["run_digest"] == wb[1]["run_digest"]
    for k in ("digest_EDDY_SUMS", "digest_EDDY_ANCHORS"):
        assert wa[1][k] == wb[1][k], k
    for k in ("eddy_anchors", "eddy_sums", "eddy_pair_sums", "eddy_clock"):      # the open window 24-29 travels
        assert np.asarray(wa[0][k]).tobytes() == np.asarray(wb[0][k]).tobytes(), k
    clock = np.asarray(wa[0]["eddy_clock"])
    assert clock[[0, 3, 4]].tolist() == [30.0, 6.0, 6.0] and clock[2] - clock[1] == 5 * DT and wa[0]["eddy_pair_sums"].shape == (8, 19, 36)
    assert f"eddy={eddy.DEFAULT_PAIRS}|every=1|maps=1" in wa[1]["subsystems"]
    _set_env(monkeypatch, _env(tmp_path, "cut", 0.0625, QD_CHECKPOINT="1", QD_EDDY="0"))      # a lane-on file by a lane-off run
    assert driver.main() == 2
    assert f"the subsystem set differs: the eddy lane is '{eddy.DEFAULT_PAIRS}|every=1|maps=1' in the file and '-' in this run" in capsys.readouterr().out
