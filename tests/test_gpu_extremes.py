"""GPU (-m gpu): the extremes lane (csrc/qd_extremes.hip, qingdai_amd/extremes.py).

  1 k_ext_accum alone through qd_extremes_sample, planes fed with Device.set, bit for bit against extremes.accumulate_reference after
    every one of four samples: 5 x 5, 6 x 63, 7 x 64, 7 x 65, 7 x 256, 9 x 257, 10 x 600 (rows shorter than a wave, at and one past a
    wave and a workgroup, several workgroups to a row with a ragged end; rows are not dealt to workgroups by a loop);
    1 entry alone, the default lists, the limits (16 entries with two derived ones, 16 thresholds with both cmp, 8 histograms with
    nb = 1, 2, 64, 255, 256); planes that hold NaN in the first, a middle and the last sample, a cell that is NaN throughout, +-inf,
    -0.0 then +0.0, ties, subnormals, values on and beside every edge, a field of zeros in one bin and one wholly under; closure;
    reset; release.  Every refusal with its text.
  2 the lane at 19 x 36: one 7-step span against seven one-step spans whose fields are downloaded and fed to accumulate_reference,
    and against the class seam (PRECIP: the early group; OLR: a lazily stored diagnostic); the model's digest equals that of a run
    without the lane; chunkings with the history, series and eddy lanes on and a window inside run_steps; launch counts;
    driver.main; a run cut inside a window and resumed."""
import ctypes
import os
import re

import numpy as np
import pytest

from test_gpu_budget_diag import make, fetch, DT
from test_gpu_series import same, _set_env

pytestmark = pytest.mark.gpu

SHAPES = [(5, 5), (6, 63), (7, 64), (7, 65), (7, 256), (9, 257), (10, 600)]
POOL = ("TS", "H", "U", "V", "Q", "CLOUD", "HICE", "ALBEDO", "OLR", "W_LAND", "UO", "VO", "PRECIP", "ETA")
ZEROS = ("HICE", "ALBEDO")                 # all +0.0 in the limits configuration: one bin, and wholly under


def lin(nb):
    return np.linspace(-2.0, 3.0, nb + 1)


def configurations():
    """name -> (entry names, thresholds [(name, cmp, value)], hists [(name, edges)])"""
    from qingdai_amd import extremes as ex
    default = list(ex.DEFAULT_FIELDS + ex.DEFAULT_OCEAN_FIELDS)
    names16 = list(POOL) + ["WIND_SPEED", "CURRENT_SPEED"]
    return {"1": (["TS"], [], []),
            "default": (default, ex.parse_thresholds(ex.DEFAULT_THRESHOLDS, default), ex.parse_bins(ex.DEFAULT_BINS, default)),
            "limits": (names16, [(n, "<>"[k % 2], 0.5) for k, n in enumerate(names16)],
                       [("TS", lin(1)), ("H", lin(2)), ("U", lin(64)), ("V", lin(255)), ("Q", lin(256)), ("HICE", np.array([0.0, 1.0])),
                        ("ALBEDO", np.array([1.0, 2.0, 3.0])), ("WIND_SPEED", ex.make_edges("log", 1e-3, 1e2, 60))])}


def sources(names):
    from qingdai_amd import history as hs
    return sorted({f for n in names for f in (hs.DERIVED[n] if n in hs.DERIVED else (n,))})


def sample_values(shape, names, hists, t, zeros=()):
    """Sample t of every source plane.  The first cells of a binned plane hold values on and beside its edges; the last nine cells
    of every plane the hostile values."""
    r = np.random.default_rng(shape[0] * 100000 + shape[1] * 10 + t)
    n = shape[0] * shape[1]
    edges = {name: np.asarray(e) for name, e in hists}
    v = {}
    for k, name in enumerate(sources(names)):
        if name == "TS":
            x = 273.15 + 25.0 * r.normal(size=shape) if "TS" not in edges or edges["TS"][-1] > 100 else 0.5 + r.normal(size=shape)
        elif name == "PRECIP":
            x = np.where(r.random(shape) < 0.6, 0.0, np.exp(r.normal(-11.0, 2.5, shape)))       # zero over most of the globe
        else:
            x = 0.5 + r.normal(size=shape) * 10.0 ** r.integers(-3, 1, size=shape)
        flat = x.reshape(-1)
        if name in edges:
            e = edges[name]
            vals = np.concatenate([e, np.nextafter(e, -np.inf), np.nextafter(e, np.inf)])
            m = min(n - 9, vals.size)
            flat[:m] = np.roll(vals, -5 * t)[:m]
        flat[n - 1] = np.nan if t == 0 else flat[n - 1]
        flat[n - 2] = np.nan if t == 2 else flat[n - 2]
        flat[n - 3] = np.nan if t == 3 else flat[n - 3]
        flat[n - 4] = np.nan
        flat[n - 5] = np.inf if t in (1, 3) else flat[n - 5]
        flat[n - 6] = -np.inf if t == 2 else flat[n - 6]
        flat[n - 7] = (-0.0, 0.0, 0.25, -0.0)[t]
        flat[n - 8] = 5.0e3 if t in (1, 3) else 0.3
        flat[n - 9] = 5e-324 * (t + 1)
        if name in zeros:
            x[:] = 0.0
        v[name] = x
    return v


def state_same(a, b):
    for k in ("vmax", "vmin"):
        if not np.array_equal(np.asarray(a[k], dtype=np.float64).view(np.int64), np.asarray(b[k], dtype=np.float64).view(np.int64)):
            return False
    return (a["n"] == b["n"] and all(np.array_equal(a[k], b[k]) for k in ("tmax", "tmin", "nan", "thr")) and
            len(a["hist"]) == len(b["hist"]) and all(np.array_equal(x, y) for x, y in zip(a["hist"], b["hist"])))


def where_differs(a, b):
    return [k for k in ("vmax", "vmin", "tmax", "tmin", "nan", "thr") if not np.array_equal(a[k], b[k], equal_nan=k[0] == "v")] + \
           [f"hist{h}" for h, (x, y) in enumerate(zip(a["hist"], b["hist"])) if not np.array_equal(x, y)] + ([] if a["n"] == b["n"] else ["n"])


def indexed(names, thresholds, hists):
    return [(names.index(n), c, x) for n, c, x in thresholds], [(names.index(n), e) for n, e in hists]


@pytest.mark.parametrize("shape", SHAPES)
def test_kernel_alone(gpu, shape):
    import qingdai_amd as qa
    from qingdai_amd import extremes as ex, history as hs
    from qingdai_amd._lib import QdError
    from qingdai_amd.device import Device
    dev = Device(qa.SphericalGrid(*shape))
    n = shape[0] * shape[1]
    for name, (names, thresholds, hists) in configurations().items():
        thr, hst = indexed(names, thresholds, hists)
        dev.extremes_configure(hs.entries_for(names), thr, hst)
        fresh = dev.extremes_read()
        assert fresh["n"] == 0 and np.isneginf(fresh["vmax"]).all() and np.isposinf(fresh["vmin"]).all() and (fresh["tmax"] == -1).all()
        assert (fresh["tmin"] == -1).all() and not fresh["nan"].any() and not fresh["thr"].any() and not any(h.any() for h in fresh["hist"])
        state, samples = None, []
        zeros = ZEROS if name == "limits" else ()
        for t in range(4):
            v = sample_values(shape, names, hists, t, zeros)
            for f, x in v.items():
                dev.set(f, x)
            dev.extremes_sample()
            samples.append(ex.entry_values(names, v.__getitem__))
            got = dev.extremes_read()
            state = ex.accumulate_reference(samples[-1:], thr, hst, state=state)
            assert got["n"] == state["n"] == t + 1
            assert state_same(got, state), (shape, name, t, where_differs(got, state))
            for table in got["hist"]:                            # closure
                assert np.array_equal(table.sum(axis=1), np.full(shape[0], shape[1] * (t + 1)))
        assert state_same(ex.accumulate_reference(samples, thr, hst), state)
        e0 = 0                                                   # the hostile cells of the first entry, as the definition says
        flat = lambda key: got[key][e0].reshape(-1)
        assert flat("tmax")[n - 4] == -1 and flat("tmin")[n - 4] == -1 and flat("nan")[n - 4] == 4 and np.isneginf(flat("vmax")[n - 4])
        assert flat("nan")[n - 1] == 1 and flat("nan")[n - 2] == 1 and flat("nan")[n - 3] == 1 and flat("tmax")[n - 1] >= 1
        assert flat("vmax")[n - 5] == np.inf and flat("tmax")[n - 5] == 1 and flat("vmin")[n - 6] == -np.inf and flat("tmin")[n - 6] == 2
        assert flat("tmin")[n - 7] == 0 and np.signbit(flat("vmin")[n - 7]) and flat("tmax")[n - 8] == 1 and flat("tmin")[n - 8] == 0
        assert flat("vmin")[n - 9] == 5e-324 and flat("vmax")[n - 9] == 2e-323 and flat("tmax")[n - 9] == 3
        if name == "limits":
            k = [h[0] for h in hists]
            one, under = got["hist"][k.index("HICE")], got["hist"][k.index("ALBEDO")]
            assert (one[:, 1] == 4 * shape[1]).all() and (under[:, 0] == 4 * shape[1]).all() and one.sum() == under.sum() == 4 * n
            t_hice = got["thr"][names.index("HICE")]              # 0.0 < 0.5 in every sample: one spell of four
            assert (t_hice == np.array([4, 4, 4, 1], dtype=np.uint32)).all()
            assert sum(int(h.shape[1]) for h in got["hist"]) == sum(e.size + 2 for _, e in hists)
        back = dev.extremes_read()                               # restore is read's inverse
        dev.extremes_reset()
        dev.extremes_restore(back)
        assert state_same(dev.extremes_read(), back)
        dev.extremes_reset()                                     # a reset: the next sample is a window's first again
        dev.extremes_sample()
        assert state_same(dev.extremes_read(), ex.accumulate_reference(samples[-1:], thr, hst))
    dev.extremes_configure([])                                   # releases
    with pytest.raises(QdError, match=r"extremes: not configured \(qd_extremes_configure first\)"):
        dev.extremes_sample()
    dev.close()


def test_refusals(gpu, monkeypatch):
    import qingdai_amd as qa
    from qingdai_amd._lib import F, QdError
    from qingdai_amd.device import Device
    sim = make(monkeypatch, 19, 36, routing=False)
    dev = sim.dev
    for call in (dev.extremes_sample, dev.extremes_reset, lambda: dev.extremes_schedule([1]),
                 lambda: dev.call("qd_extremes_read", np.zeros(1), np.zeros(1, dtype=np.int32), None, None, np.zeros(1, dtype=np.int64)),
                 lambda: dev.call("qd_extremes_restore", np.zeros(1), np.zeros(1, dtype=np.int32), None, None, 0)):
        with pytest.raises(QdError, match=r"extremes: not configured \(qd_extremes_configure first\)"):
            call()
    for ref in ("EXTREMES_VALUES", "EXTREMES_COUNTS", "EXTREMES_HIST"):
        with pytest.raises(QdError, match=f"qd_state_digest: ref {ref}: the extremes lane is not configured"):
            dev.digest([ref])
    TS, LT, GT = F["TS"], ord("<"), ord(">")

    def raw(op, a, b, thr=(), hists=(), edges=()):
        return dev.call("qd_extremes_configure", len(op), op, a, b, len(thr), [t[0] for t in thr] or None, [t[1] for t in thr] or None,
                        [t[2] for t in thr] or None, len(hists), [h[0] for h in hists] or None, [h[1] for h in hists] or None,
                        np.asarray(edges, dtype=np.float64) if len(edges) else None)
    one = ([0], [TS], [-1])
    for args, kw, why in ((([0] * 17, [TS] * 17, [-1] * 17), {}, "extremes: at most 16 entries"),
                          (one, dict(thr=[(0, LT, 1.0)] * 17), "extremes: at most 16 thresholds"),
                          (one, dict(hists=[(0, 1)] * 9, edges=[0.0, 1.0] * 9), "extremes: at most 8 histograms"),
                          (one, dict(hists=[(0, 257)], edges=np.arange(258.0)), "extremes: histogram 0: at most 256 bins"),
                          (([2], [TS], [-1]), {}, r"extremes: unknown op \(0 = field a, 1 = sqrt\(a\*a \+ b\*b\)\)"),
                          (([0], [9999], [-1]), {}, "extremes: field a is not an f64 plane"),
                          (([0], [F["LAND_MASK"]], [-1]), {}, "extremes: field a is not an f64 plane"),
                          (([1], [TS], [-1]), {}, "extremes: field b is not an f64 plane"),
                          (([1], [F["PRECIP"]], [TS]), {}, "extremes: op 1 cannot pair PRECIP with another field"),
                          (one, dict(thr=[(1, LT, 1.0)]), "extremes: threshold 0 has an entry index outside the 1 entries"),
                          (one, dict(thr=[(0, LT, 1.0), (-1, GT, 1.0)]), "extremes: threshold 1 has an entry index outside the 1 entries"),
                          (one, dict(thr=[(0, ord("="), 1.0)]), r"extremes: threshold 0: cmp is neither '<' \(60\) nor '>' \(62\)"),
                          (one, dict(thr=[(0, 0, 1.0)]), "extremes: threshold 0: cmp is neither"),
                          (one, dict(thr=[(0, LT, np.inf)]), "extremes: threshold 0: the value is not finite"),
                          (one, dict(thr=[(0, GT, np.nan)]), "extremes: threshold 0: the value is not finite"),
                          (one, dict(hists=[(1, 1)], edges=[0.0, 1.0]), "extremes: histogram 0 has an entry index outside the 1 entries"),
                          (one, dict(hists=[(0, 0)], edges=[0.0]), "extremes: histogram 0: fewer than 2 edges"),
                          (one, dict(hists=[(0, 2)], edges=[0.0, 1.0, 1.0]), "extremes: histogram 0: the edges are not finite and strictly increasing"),
                          (one, dict(hists=[(0, 1), (0, 2)], edges=[0.0, 1.0, 0.0, 2.0, 1.0]), "extremes: histogram 1: the edges are not finite and strictly"),
                          (one, dict(hists=[(0, 2)], edges=[0.0, np.nan, 1.0]), "extremes: histogram 0: the edges are not finite"),
                          (one, dict(hists=[(0, 1)], edges=[0.0, np.inf]), "extremes: histogram 0: the edges are not finite")):
        with pytest.raises(QdError, match=why):
            raw(*args, **kw)
    with pytest.raises(QdError, match="extremes: not configured"):       # none of the refused calls left a configuration
        dev.extremes_sample()
    # a span: the wrong schedule length is refused with the lane's own text, nothing runs, and the schedule is gone
    dev.extremes_configure([(0, "TS", None), (0, "PRECIP", None)], [(0, "<", 273.15)], [(1, [0.0, 1.0])])
    flags = dict(with_ocean=True, with_physics=True, pass_albedo=False, with_hydrology=True)
    stars = sim.forcing.star_table(DT * np.arange(3))
    counters = dev.counters()
    dev.extremes_schedule([1, 1, 1])
    with pytest.raises(QdError, match="extremes: qd_step_n: a qd_extremes_schedule must cover exactly the n steps of the span"):
        dev.step_n(stars[:2], DT, **flags)
    assert dev.counters() == counters and dev.extremes_read()["n"] == 0
    with pytest.raises(QdError, match="extremes: qd_extremes_restore: the sample count is negative"):
        dev.extremes_restore(dict(dev.extremes_read(), n=-1))
    with pytest.raises(ValueError, match="extremes_restore: expected vmax of shape"):
        dev.extremes_restore(dict(dev.extremes_read(), vmax=np.zeros((1, 19, 36))))
    # through the environment: the line names the item
    for env, why in (({"QD_EXTREMES_THRESHOLDS": "SST<280", "QD_EXTREMES_FIELDS": "TS"}, "QD_EXTREMES_THRESHOLDS: 'SST<280': 'SST' is not among"),
                     ({"QD_EXTREMES_BINS": "TS:log:0:1:4"}, "QD_EXTREMES_BINS: 'TS:log:0:1:4': log bins need lo > 0"),
                     ({"QD_EXTREMES_BINS": "TS:lin:2:1:4"}, "QD_EXTREMES_BINS: 'TS:lin:2:1:4': hi is not above lo"),
                     ({"QD_EXTREMES_BINS": "TS:lin:1:2:300"}, "300 bins, 1 to 256"),
                     ({"QD_EXTREMES_THRESHOLDS": "TS<1,TS<1"}, "the threshold 'TS<1' is named twice"),
                     ({"QD_EXTREMES_THRESHOLDS": "TS~1"}, "'TS~1' is not NAME<value or NAME>value"),
                     ({"QD_EXTREMES_FIELDS": "NOPE"}, "QD_EXTREMES_FIELDS: unknown field 'NOPE'")):
        with pytest.raises(ValueError, match=re.escape(why)):
            sim.enable_extremes(dict(env, QD_EXTREMES="1"))
    assert sim.enable_extremes({"QD_EXTREMES": "0", "QD_EXTREMES_FIELDS": "NOPE"}) is None and sim.extremes is None
    dev.close()
    # a band handle
    band = Device(qa.SphericalGrid(73, 144), row0=20, n_rows=30, halo=6)
    i1 = (ctypes.c_int32 * 1)
    rc = band.lib.qd_extremes_configure(band.h, 1, i1(0), i1(TS), i1(-1), 0, None, None, None, 0, None, None, None)
    assert rc != 0 and b"extremes: the extremes lane needs a whole-globe handle" in band.lib.qd_last_error(band.h)
    assert b"latitude bands are not supported" in band.lib.qd_last_error(band.h)
    band.close()


# ---------------------------------------------------------------- 2: the lane
FIELDS = "TS,PRECIP,WIND_SPEED,H,OLR"
THRESHOLDS = "TS<273.15,PRECIP>1.1574e-5,OLR>200"
BINS = "PRECIP:log:1e-8:1e-2:60,TS:lin:150:350:100,WIND_SPEED:lin:0:100:100,OLR:lin:100:350:50"


def attach(sim, tmp_path, *, every=1, S=None, fields=FIELDS, thresholds=THRESHOLDS, bins=BINS, lane=True):
    """An Extremes on the run's handle; lane=False: configured, but no participant of the spans (the class seam's twin)."""
    from qingdai_amd import extremes as ex
    days = ex.EVERY_DAYS if S is None else S * DT / sim.day_seconds
    sim.extremes_lines = []
    fields = fields + (",SST" if sim.ocean is not None and "SST" not in fields else "")
    e = ex.Extremes(sim.dev, sim.grid, {"enabled": True, "sample_every": every, "every_days": days}, with_ocean=sim.ocean is not None, dt=DT,
                    day=sim.day_seconds, out=sim.extremes_lines.append, output_dir=str(tmp_path), fields=fields, thresholds=thresholds, bins=bins)
    assert S is None or e.S == S
    sim.extremes = e if lane else None
    return e


def model_digest(sim):
    return {k: v for k, v in sim.digest().items() if not k.startswith("EXTREMES_") and k != "run"}


def reference(e, samples):
    from qingdai_amd import extremes as ex
    thr, hst = indexed(e.names, e.thresholds, e.hists)
    return ex.accumulate_reference(samples, thr, hst)


def grab(sim, e):
    from qingdai_amd import extremes as ex
    return ex.entry_values(e.names, fetch(sim.dev, sources(e.names)).__getitem__)


@pytest.mark.parametrize("ocean,every,fused", [(True, 1, None), (True, 3, None), (False, 1, None), (False, 3, None), (True, 1, "0")])
def test_span_equals_single_steps(gpu, monkeypatch, tmp_path, ocean, every, fused):
    env = {} if fused is None else {"QD_FUSED": fused}
    sim = make(monkeypatch, 19, 36, ocean=ocean, routing=False, env=env)
    e = attach(sim, tmp_path, every=every)
    sim.run_steps(7)                                             # one span
    span, span_digest, full = sim.dev.extremes_read(), model_digest(sim), sim.digest()
    assert all(k in full for k in ("EXTREMES_VALUES", "EXTREMES_COUNTS", "EXTREMES_HIST")) and (e.i, e.n_open) == (7, len(range(0, 7, every)))
    sim.dev.close()
    sim = make(monkeypatch, 19, 36, ocean=ocean, routing=False, env=env)
    e = attach(sim, tmp_path, every=every, lane=False)
    samples = []
    for i in range(7):                                           # seven one-step spans, the class seam behind each sampled one
        sim.run_steps(1)
        if i % every == 0:
            samples.append(grab(sim, e))
            sim.dev.extremes_sample()
    seam = sim.dev.extremes_read()
    sim.dev.close()
    want = reference(e, samples)
    assert state_same(span, want), (ocean, every, fused, where_differs(span, want))
    assert state_same(seam, want), (ocean, every, fused, where_differs(seam, want))
    assert span["n"] == len(samples) and np.isfinite(span["vmax"]).all() and (span["tmax"] >= 0).all()
    p, olr = e.names.index("PRECIP"), e.names.index("OLR")
    assert span["vmax"][p].any() and span["hist"][0].sum() == span["n"] * 19 * 36 and span["vmax"][olr].min() > 50.0
    assert len(samples) < 2 or not np.array_equal(samples[0][p], samples[1][p])     # the early group's field moves from step to step
    sim = make(monkeypatch, 19, 36, ocean=ocean, routing=False, env=env)
    sim.run_steps(7)                                             # the same span without the lane: the model does not notice
    assert "EXTREMES_VALUES" not in sim.digest() and model_digest(sim) == span_digest and len(span_digest) > 20
    sim.dev.close()


def test_lazy_diagnostic_inside_a_span(gpu, monkeypatch, tmp_path):
    """Device.step_n without the hydrology bit: inside a span only the last step stores OLR -- unless a reader comes with the span."""
    flags = dict(with_ocean=True, with_physics=True, pass_albedo=False, with_hydrology=False)
    a = make(monkeypatch, 19, 36, routing=False)
    ea = attach(a, tmp_path, fields="OLR,PRECIP,TS", thresholds="OLR>200", bins="OLR:lin:100:350:50", lane=False)
    stars = a.forcing.star_table(DT * np.arange(5))
    samples = []
    for i in range(5):
        a.dev.step_n(stars[i:i + 1], DT, **flags)
        samples.append(grab(a, ea))
    a.dev.close()
    b = make(monkeypatch, 19, 36, routing=False)
    e = attach(b, tmp_path, fields="OLR,PRECIP,TS", thresholds="OLR>200", bins="OLR:lin:100:350:50")
    b.dev.step_n(stars, DT, extremes=e, **flags)
    got, want = b.dev.extremes_read(), reference(e, samples)
    assert e.i == 5 and state_same(got, want), where_differs(got, want)
    assert all(not np.array_equal(samples[i][0], samples[i + 1][0]) for i in range(4))
    b.dev.close()


FIRES = {0: 3, 2: 1, 5: 3}


def test_chunkings_with_the_other_lanes_and_a_window_inside_a_run(gpu, monkeypatch, tmp_path):
    from qingdai_amd import extremes as ex, ncio
    from test_gpu_eddy import attach as attach_eddy
    from test_gpu_history import attach as attach_history
    from test_gpu_series import attach as attach_series
    runs = {}
    for name, cuts in (("whole", (7,)), ("two", (3, 4)), ("single", (1,) * 7), ("off", (7,))):
        out = tmp_path / name
        sim = make(monkeypatch, 19, 36, fires=FIRES)
        attach_history(sim, out, S=4)
        attach_series(sim, out, S=4)
        attach_eddy(sim, out, S=4)
        e = attach(sim, out, S=4) if name != "off" else None
        sim.dev.timing(True)
        samples = []
        for n in cuts:
            sim.run_steps(n)
            if name == "single":
                samples.append(grab(sim, e))
        sim.dev.sync()
        launches = sim.dev.timing_get("extremes")[1]
        sim.dev.timing(False)
        others = {d: [open(out / d / f, "rb").read() for f in sorted(os.listdir(out / d))] for d in ("history", "series", "eddy")}
        runs[name] = dict(state=sim.dev.extremes_read() if e else None, digest=model_digest(sim), launches=launches, samples=samples,
                          lines=list(sim.extremes_lines) if e else [], others=others, budget=list(sim.budget_lines),
                          history=list(sim.history_lines), files=sorted(os.listdir(out / "extremes")) if os.path.exists(out / "extremes") else None, e=e)
        sim.dev.close()
    whole, off = runs["whole"], runs["off"]
    samples = runs["single"]["samples"]
    # a 4-step window inside run_steps(7): one file behind step 3, steps 4-6 stand in the planes
    want = reference(whole["e"], samples[4:])
    assert state_same(whole["state"], want) and whole["state"]["n"] == 3, where_differs(whole["state"], want)
    for name in ("two", "single"):
        assert state_same(runs[name]["state"], whole["state"]), name
        assert runs[name]["files"] == whole["files"] and runs[name]["lines"] == whole["lines"] and runs[name]["digest"] == whole["digest"]
        for f in whole["files"]:
            assert open(tmp_path / name / "extremes" / f, "rb").read() == open(tmp_path / "whole" / "extremes" / f, "rb").read(), (name, f)
    assert len(whole["files"]) == 1 and len(whole["lines"]) == 1 and whole["lines"][0].startswith("[Extremes] day ")
    v, _ = ncio.read_nc(str(tmp_path / "whole" / "extremes" / whole["files"][0]))
    first = reference(whole["e"], samples[:4])
    assert int(v["n_samples"]) == 4 and int(v["complete"]) == 1
    assert same(v["ts_max"], first["vmax"][0]) and same(v["precip_min"], first["vmin"][1]) and np.array_equal(v["precip_hist"], first["hist"][0])
    assert np.array_equal(v["ts_tmax_seconds"], float(v["t_start_seconds"]) + first["tmax"][0] * DT)
    # the other lanes and the model do not notice; no scope at 0, two launches per sampled step (PRECIP: the early group) otherwise
    assert off["launches"] == 0 and off["files"] is None and whole["launches"] == runs["two"]["launches"] == runs["single"]["launches"] == 14
    assert whole["others"] == off["others"] and all(len(off["others"][d]) == 1 for d in off["others"])
    assert whole["budget"] == off["budget"] and len(off["budget"]) > 0 and whole["history"] == off["history"]
    assert whole["digest"] == off["digest"] and len(off["digest"]) > 20


def test_launch_counts(gpu, monkeypatch, tmp_path):
    for fields, thr, bins, per_step in ((FIELDS, THRESHOLDS, BINS, 2), ("TS,WIND_SPEED", "TS<273.15", "TS:lin:150:350:100", 1),
                                        ("PRECIP", "PRECIP>1e-5", "PRECIP:log:1e-8:1e-2:60", 1)):
        sim = make(monkeypatch, 19, 36, routing=False, ocean=False)
        attach(sim, tmp_path / str(per_step) / fields[:2], every=3, S=5, fields=fields, thresholds=thr, bins=bins)
        sim.dev.timing(True)
        sim.run_steps(12)                                        # windows 0-4, 5-9, 10-11: positions 0 and 3 of each are sampled
        sim.dev.sync()
        assert sim.dev.timing_get("extremes")[1] == 5 * per_step and len(sim.extremes_lines) == 2 and sim.dev.extremes_read()["n"] == 1
        assert [int(re.search(r": (\d+) samples", s).group(1)) for s in sim.extremes_lines] == [2, 2]
        sim.dev.timing(False)
        sim.dev.close()
    sim = make(monkeypatch, 19, 36, routing=False, ocean=False)     # the lane off: no scope at all
    sim.dev.timing(True)
    sim.run_steps(12)
    sim.dev.sync()
    assert sim.dev.timing_get("extremes")[1] == 0 and sim.extremes is None
    sim.dev.close()


def test_python_use_with_the_callers_own_edges(gpu, monkeypatch, tmp_path):
    from qingdai_amd import extremes as ex, ncio
    sim = make(monkeypatch, 19, 36, routing=False)
    edges = np.array([200.0, 250.0, 273.15, 290.0, 330.0])
    lines = []
    e = ex.Extremes(sim, cfg={"every_days": 4 * DT / sim.day_seconds, "sample_every": 1}, fields=["TS", "CURRENT_SPEED"],
                    thresholds=[("TS", ">", 285.0)], bins={"TS": edges}, out=lines.append, output_dir=str(tmp_path))
    assert e.dev is sim.dev and e.S == 4 and e.names == ["TS", "CURRENT_SPEED"] and e.thresholds == [("TS", ">", 285.0)]
    sim.extremes = e
    sim.run_steps(4)                                             # the window closes behind the span
    assert len(e.files) == 1 and len(lines) == 1 and sim.dev.extremes_read()["n"] == 0
    v, _ = ncio.read_nc(e.files[0])
    assert np.array_equal(v["ts_edges"], edges) and v["ts_hist"].shape == (19, 7) and np.array_equal(v["ts_hist"].sum(axis=1), np.full(19, 36 * 4))
    assert np.array_equal(v["ts_gt_285_freq"], v["ts_gt_285_count"] / 4) and v["ts_gt_285_count"].any() and (v["current_speed_min"] >= 0).all()
    assert re.fullmatch(r"\[Extremes\] day \S+: 4 samples \| TS max=\S+ at \(-?\d+\.\d+, \d+\.\d+\) \| TS p99=\S+ TS_gt_285 freq=\S+", lines[0]), lines
    sim.dev.close()


def _env(tmp_path, data, days, **extra):
    e = {"QD_N_LAT": "19", "QD_N_LON": "36", "QD_DT_SECONDS": "300", "QD_SIM_DAYS": str(days), "QD_DYN_DIAG_PRINT": "0", "QD_ECO_ENABLE": "0",
         "QD_HYDRO_ENABLE": "0", "QD_USE_OCEAN": "1", "QD_DATA_DIR": str(tmp_path / data), "QD_OUTPUT_DIR": str(tmp_path / ("out_" + data)),
         "QD_EXTREMES": "1", "QD_EXTREMES_EVERY_DAYS": "0.05", "QD_EXTREMES_SAMPLE_EVERY": "2"}
    e.update(extra)
    return e


def test_driver_main(gpu, tmp_path, monkeypatch, capsys):
    from qingdai_amd import driver, extremes as ex, ncio
    monkeypatch.chdir(tmp_path)
    hist = dict(QD_HISTORY="1", QD_HISTORY_EVERY_DAYS="0.05", QD_HISTORY_SAMPLE_EVERY="2", QD_HISTORY_FIELDS="TS,H,SST")
    _set_env(monkeypatch, _env(tmp_path, "on", 0.125, **hist))   # 30 steps: windows 0-11 and 12-23, 24-29 is written open
    assert driver.main() == 0
    out = capsys.readouterr().out
    lines = [s for s in out.splitlines() if s.startswith("[Extremes]")]
    assert len(lines) == 3 and [int(re.search(r": (\d+) samples", s).group(1)) for s in lines] == [6, 6, 3], out
    assert all(re.fullmatch(r"\[Extremes\] day \d+\.\d+–\d+\.\d+: \d+ samples \| TS max=\S+ at \(-?\d+\.\d+, \d+\.\d+\) \| PRECIP p99=\S+ "
                            r"TS_lt_273p15 freq=\S+", s) for s in lines), lines
    d, dh = tmp_path / "out_on" / "extremes", tmp_path / "out_on" / "history"
    files, hfiles = sorted(os.listdir(d)), sorted(os.listdir(dh))
    assert len(files) == 3 == len(hfiles) and all(re.fullmatch(r"extremes_day_\d+\.\d+_\d+\.\d+\.nc", f) for f in files), files
    names = ["TS", "PRECIP", "WIND_SPEED", "H", "SST"]
    labels = [ex.threshold_label(*t).lower() for t in ex.parse_thresholds(ex.DEFAULT_THRESHOLDS, names)]
    want = {"lat", "lon", "quantile_levels", "n_samples", "t_start_seconds", "t_end_seconds", "dt_seconds", "sample_every", "complete"}
    want |= {f"{n.lower()}_{k}" for n in names for k in ("max", "min", "tmax_seconds", "tmin_seconds", "nan")}
    want |= {f"{t}_{k}" for t in labels for k in ("count", "spells", "open", "freq", "longest_seconds", "mean_spell_seconds")}
    want |= {f"{n}_{k}" for n in ("precip", "ts", "wind_speed") for k in ("edges", "hist", "pdf", "under_frac", "over_frac", "nan_frac", "quantiles")}
    for f, hf, (n, complete) in zip(files, hfiles, ((6, 1), (6, 1), (3, 0))):
        v, _ = ncio.read_nc(str(d / f))
        h, _ = ncio.read_nc(str(dh / hf))
        assert set(v) == want
        assert (int(v["n_samples"]), int(v["complete"]), int(v["sample_every"]), float(v["dt_seconds"])) == (n, complete, 2, DT)
        assert v["ts_max"].shape == (19, 36) and v["precip_hist"].shape == (19, 63) and v["precip_edges"].shape == (61,) and v["ts_pdf"].shape == (100,)
        assert v["ts_quantiles"].shape == (4,) and v["ts_lt_273p15_count"].shape == (19, 36)
        for t in labels:
            assert np.array_equal(v[t + "_freq"], v[t + "_count"] / n) and (v[t + "_open"] <= v[t + "_count"]).all()
            assert (v[t + "_longest_seconds"] <= n * 2 * DT).all() and (v[t + "_spells"] <= v[t + "_count"]).all()
        for name in ("precip", "ts", "wind_speed"):
            assert np.array_equal(v[name + "_hist"].sum(axis=1), np.full(19, 36 * n))
        assert int(h["n_samples"]) == n                          # the same samples: the mean lies between the extremes
        for name in ("ts", "h", "sst"):
            assert (v[name + "_min"] <= h[name]).all() and (h[name] <= v[name + "_max"]).all(), name
            assert (v[name + "_tmax_seconds"] >= float(v["t_start_seconds"])).all() and (v[name + "_tmax_seconds"] <= float(v["t_end_seconds"])).all()
        assert not v["ts_nan"].any() and (v["ts_max"] > 150).all() and abs(v["ts_pdf"].sum() - 1.0) < 1e-12
    monkeypatch.delenv("QD_EXTREMES")                            # the same run without the switch: no directory, no line
    monkeypatch.setenv("QD_OUTPUT_DIR", str(tmp_path / "out_off"))
    monkeypatch.setenv("QD_DATA_DIR", str(tmp_path / "off"))
    assert driver.main() == 0
    assert "[Extremes]" not in capsys.readouterr().out and not os.path.exists(tmp_path / "out_off" / "extremes")
    for hf in hfiles:                                            # and the history files of the lane-off run are the lane-on run's
        assert open(tmp_path / "out_off" / "history" / hf, "rb").read() == open(dh / hf, "rb").read()


def test_resumed_run_writes_the_uncut_runs_files(gpu, tmp_path, monkeypatch, capsys):
    from qingdai_amd import driver, ncio
    monkeypatch.chdir(tmp_path)
    ck = dict(QD_CHECKPOINT="1", QD_EXTREMES_SAMPLE_EVERY="1")
    _set_env(monkeypatch, _env(tmp_path, "whole", 0.125, **ck))  # 30 steps: windows 0-11 and 12-23, 24-29 stays open
    assert driver.main() == 0
    whole = capsys.readouterr().out
    assert whole.count("[Extremes] day ") == 2 and " 30 steps" in whole and "[Checkpoint] (final) wrote" in whole
    _set_env(monkeypatch, _env(tmp_path, "cut", 0.0625, **ck))   # 15 steps: stopped inside the window 12-23
    assert driver.main() == 0
    first = capsys.readouterr().out
    assert first.count("[Extremes] day ") == 1 and " 15 steps" in first and "[Checkpoint] loaded" not in first
    assert driver.main() == 0
    second = capsys.readouterr().out
    assert "[Checkpoint] loaded" in second and "step 15" in second and second.count("[Extremes] day ") == 1      # each file written once
    files = lambda d: sorted(os.listdir(tmp_path / ("out_" + d) / "extremes"))
    assert files("cut") == files("whole") and len(files("whole")) == 2
    for name in files("whole"):
        a, b = (open(tmp_path / ("out_" + d) / "extremes" / name, "rb").read() for d in ("whole", "cut"))
        assert a == b, name
        v, _ = ncio.read_nc(str(tmp_path / "out_whole" / "extremes" / name))
        assert int(v["complete"]) == 1 and int(v["n_samples"]) == 12
    wa, wb = (ncio.read_nc(str(tmp_path / d / "checkpoint.nc")) for d in ("whole", "cut"))
    assert wa[1]["run_digest"] == wb[1]["run_digest"]
    for k in ("digest_EXTREMES_VALUES", "digest_EXTREMES_COUNTS", "digest_EXTREMES_HIST"):
        assert wa[1][k] == wb[1][k], k
    for k in ("extremes_values", "extremes_counts", "extremes_thresholds", "extremes_hist", "extremes_clock"):      # the open window 24-29 travels
        assert np.asarray(wa[0][k]).tobytes() == np.asarray(wb[0][k]).tobytes(), k
    clock = np.asarray(wa[0]["extremes_clock"])
    assert clock[[0, 3, 4]].tolist() == [30.0, 6.0, 6.0] and clock[2] - clock[1] == 5 * DT and wa[0]["extremes_values"].shape == (2, 5, 19, 36)
    assert "extremes=TS,PRECIP,WIND_SPEED,H,SST|TS_lt_273p15,PRECIP_gt_1p1574em05|" in wa[1]["subsystems"]
    _set_env(monkeypatch, _env(tmp_path, "cut", 0.0625, QD_CHECKPOINT="1", QD_EXTREMES="0"))      # a lane-on file by a lane-off run
    assert driver.main() == 2
    assert re.search(r"the subsystem set differs: the extremes lane is 'TS,PRECIP,WIND_SPEED,H,SST\|.*\|every=1' in the file and '-' in this run",
                     capsys.readouterr().out)
