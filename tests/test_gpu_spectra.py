"""GPU (-m gpu): the zonal spectra lane (csrc/qd_spectra.hip, qingdai_amd/spectra.py).

  1 the kernel alone through the class seam at the shapes where it changes form (direct, radix 2 / 3 / 4 / 5, below one wave, the
    largest grid), with 1, 5 and 32 entries, lat-resolved sums on and off, every smooth shape also under QD_SPECTRA_FORM=direct.
    Every bin of every row is held against spectra.dft_reference (extended precision) with the a-priori bound
        |P^ - P| <= (c_k / n^2) (2 (|Re X| + |Im X|) E + 2 E^2) + 8 u P,    E = gamma_{n+3} sum_i |x_i|,  u = 2^-53,
    derived in tests/test_spectra_cpu.py: Re X and Im X are sums of n products x_i w_i, |w_i| = 1, each w_i from a table within 2u;
    in ANY order (the direct loop, the FFT's butterflies, with or without FMA) a path from x_i to the result carries at most n - 1
    additions, a product and the table's error, so each part errs by at most E; squaring gives the first term; the two squares,
    their sum and the division round four times, inside 8 u P.  A misplaced bin or a wrong twiddle misses it by orders of magnitude.
    The cross-row combination is bitwise: spectra.combine_reference of the device's own per-row powers;
  2 the refusals;
  3 one span against a cut span against one-step spans with a class-seam sample behind each: bitwise;
  4 lazily stored diagnostics and PRECIP inside a long span;
  5 no effect on the other lanes and on the state; no spectra scope in the timing tables when the lane is off;
  6 driver.main;
  7 a run stopped inside a window and resumed (QD_CHECKPOINT=1) against the uncut run."""
import os
import re

import numpy as np
import pytest

from test_gpu_budget_diag import make, fetch, DT
from test_gpu_series import same, _set_env
from test_spectra_cpu import power_bound

pytestmark = pytest.mark.gpu


# ---------------------------------------------------------------- 1: the kernel alone
#          shape       smooth (an FFT by default)
# (a handle has at least five rows -- qd_create refuses fewer -- so the cases drawn up as 3 x 60, 4 x 72, 3 x 125, 2 x 243, 3 x 1440
# and 2 x 2880 run with five rows of the same length: the row length is what selects the kernel's path)
SHAPES = [((5, 5), False), ((5, 60), True), ((6, 63), False), ((7, 64), True), ((5, 72), True), ((5, 125), True), ((9, 130), False),
          ((5, 243), True), ((9, 257), False), ((5, 360), True), ((5, 1440), True), ((5, 2880), True)]
CASES = [(s, "default") for s, _ in SHAPES] + [(s, "direct") for s, smooth in SHAPES if smooth]
POOL = [(0, "U", None), (1, "U", "V"), (0, "H", None), (0, "OLR", None), (0, "TS", None), (0, "V", None), (0, "Q", None),
        (0, "CLOUD", None), (0, "HICE", None), (0, "ALBEDO", None)]
COSINE_M = lambda kN: sorted({1, max(1, kN - 1), kN})


_REF = {}


def entry_list(n):
    return [POOL[k % len(POOL)] for k in range(n)]


def field_values(r, shape):
    """U, V seeded normal rows; H single cosines at m = 1, kN - 1, kN (row j: the j-th of them in turn); Q constant rows; CLOUD the
    alternating row; TS rows spanning 1e-150 .. 1e150; HICE all -0.0; OLR normal with one NaN and one +inf in different rows;
    ALBEDO the same plane without them."""
    n_lat, n = shape
    i = np.arange(n)
    kN = n // 2
    v = {"U": r.normal(size=shape) * 10.0 ** r.integers(-3, 4, size=shape), "V": r.normal(size=shape)}
    ms = COSINE_M(kN)
    v["H"] = np.stack([(1.0 + j) * np.cos(2.0 * np.pi * ms[j % len(ms)] * i / n) for j in range(n_lat)])
    v["Q"] = np.repeat((np.arange(n_lat) - 0.75)[:, None], n, axis=1)
    v["CLOUD"] = np.repeat(np.where(i % 2 == 0, 1.5, -1.5)[None, :], n_lat, axis=0) * (1.0 + np.arange(n_lat))[:, None]
    v["TS"] = np.sign(r.normal(size=shape)) * 10.0 ** r.uniform(-150.0, 150.0, size=shape)
    v["TS"][:, 0], v["TS"][:, n - 1] = 1e150, 1e-150
    v["HICE"] = np.full(shape, -0.0)
    v["ALBEDO"] = r.normal(size=shape)
    v["OLR"] = v["ALBEDO"].copy()
    v["OLR"][0, n // 3] = np.nan
    v["OLR"][n_lat - 1, n - 1] = np.inf
    return v


def host_plane(entry, v):
    op, a, b = entry
    if op == 0:
        return v[a]
    with np.errstate(all="ignore"):
        return np.sqrt(v[a] * v[a] + v[b] * v[b])


@pytest.mark.parametrize("shape,form", CASES, ids=[f"{s[0]}x{s[1]}-{f}" for s, f in CASES])
def test_kernel_alone(gpu, monkeypatch, shape, form):
    import qingdai_amd as qa
    from qingdai_amd import series, spectra
    from qingdai_amd._lib import QdError
    from qingdai_amd.device import Device
    if form == "direct":
        monkeypatch.setenv("QD_SPECTRA_FORM", "direct")
    else:
        monkeypatch.delenv("QD_SPECTRA_FORM", raising=False)
    n_lat, n = shape
    nb, kN = n // 2 + 1, n // 2
    grid = qa.SphericalGrid(*shape)
    dev = Device(grid)
    lat = np.asarray(grid.lat, dtype=np.float64).reshape(-1)
    w = series.row_weights(lat)
    if shape not in _REF:                                        # computed once, shared by both forms and every configuration
        v = field_values(np.random.default_rng(n_lat * 10000 + n), shape)
        _REF[shape] = (v, {e: spectra.dft_reference(host_plane(e, v), parts=True) for e in POOL})
    v, ref = _REF[shape]
    for name, x in v.items():
        dev.upload_now(name, x)
    per_entry = {}
    worst = 0.0
    for n_e, lat_resolved in ((1, 1), (5, 1), (5, 0), (32, 1), (32, 0), (1, 0)):
        entries = entry_list(n_e)
        dev.spectra_configure(entries, lat_resolved, w)
        dev.spectra_sample()
        recs = dev.spectra_log()
        assert recs.shape == (1, spectra.record_width(n_e, n)) and len(dev.spectra_log()) == 0
        power, bad = spectra.split_records(recs, n_e, n)
        if not lat_resolved:
            with pytest.raises(QdError, match="qd_spectra_sums_get: the configuration is not lat-resolved"):
                dev.spectra_sums()
            for k, e in enumerate(entries):                      # the record does not depend on the sums being kept
                assert same(power[0, k], per_entry[e][0]) and bad[0, k] == per_entry[e][1], (shape, form, n_e, e)
            continue
        sums, count = dev.spectra_sums()
        assert count == 1 and sums.shape == (n_e, n_lat, nb)
        for k, e in enumerate(entries):
            x = host_plane(e, v)
            P, re_x, im_x = ref[e]
            rows_bad = ~np.isfinite(x).all(axis=1)
            got = sums[k]                                        # after exactly one sample the sums are the per-row powers
            assert np.isnan(got[rows_bad]).all() and bad[0, k] == rows_bad.sum(), (shape, form, e)
            ok = ~rows_bad
            bound = power_bound(x[ok], P[ok], re_x[ok], im_x[ok])
            err = np.abs(got[ok] - P[ok])
            ratio = float((err / np.where(bound > 0, bound, 1.0)).max()) if ok.any() else 0.0
            worst = max(worst, ratio)
            assert (err <= bound).all(), (shape, form, n_e, e, ratio)
            # the cross-row order, bit for bit, from the device's own rows
            assert same(power[0, k], spectra.combine_reference(got, lat)), (shape, form, n_e, e)
            # the same planes in another configuration: the same bits
            first = per_entry.setdefault(e, (power[0, k].copy(), bad[0, k], got.copy()))
            assert same(power[0, k], first[0]) and same(got, first[2]), (shape, form, n_e, e)
        if n_e == 5:
            by = {e: sums[k] for k, e in enumerate(entries)}
            ms = COSINE_M(kN)
            for j in range(n_lat):                               # a single cosine: all of the variance in its bin
                Pj = by[(0, "H", None)][j]
                assert Pj[ms[j % len(ms)]] >= (1.0 - 1e-12) * Pj.sum(), (shape, form, j)
            assert np.isnan(by[(0, "OLR", None)][[0, n_lat - 1]]).all() and bad[0, 3] == (2 if n_lat > 1 else 1)
        if n_e == 32:
            by = {e: sums[k] for k, e in enumerate(entries)}
            if n_lat > 2:                                        # finite rows beside the bad ones are what they are without them
                assert same(by[(0, "OLR", None)][1:n_lat - 1], by[(0, "ALBEDO", None)][1:n_lat - 1])
            assert same(by[(0, "HICE", None)], np.zeros((n_lat, nb)))                 # all -0.0: +0.0 everywhere
            # sampled twice: identical bits -- the second record is the first, the sums are exactly twice the rows
            dev.spectra_sample()
            again = dev.spectra_log()
            sums2, count2 = dev.spectra_sums()
            assert same(again, recs) and count2 == 2 and same(sums2, sums + sums)
    print(shape, form, "worst error / bound", worst)
    # two samples queue two records, oldest first; a reset forgets them and zeroes the sums
    dev.spectra_configure(entry_list(1), 1, w)
    dev.spectra_sample()
    dev.upload_now("U", v["U"] + 1.0)
    dev.spectra_sample()
    recs = dev.spectra_log()
    assert recs.shape[0] == 2 and same(recs[0, :nb], per_entry[POOL[0]][0]) and not same(recs[1], recs[0])
    dev.spectra_sample()
    dev.spectra_reset()
    assert len(dev.spectra_log()) == 0
    sums, count = dev.spectra_sums()
    assert count == 0 and same(sums, np.zeros_like(sums))
    dev.spectra_sums_set(np.full_like(sums, 2.5), 7)
    sums, count = dev.spectra_sums()
    assert count == 7 and same(sums, np.full_like(sums, 2.5))
    assert dev.digest(["SPECTRA_SUMS"])[0] != 0
    dev.spectra_configure([], 0, None)                           # releases
    with pytest.raises(QdError, match="qd_spectra_sample: not configured"):
        dev.spectra_sample()
    dev.close()


# ---------------------------------------------------------------- 2: refusals
def test_refusals(gpu, monkeypatch, tmp_path):
    import qingdai_amd as qa
    from qingdai_amd import series, spectra
    from qingdai_amd._lib import SPECTRA_LOG_CAP, QdError
    from qingdai_amd.bands import BandGroup
    from qingdai_amd.device import Device
    monkeypatch.delenv("QD_SPECTRA_FORM", raising=False)
    grid = qa.SphericalGrid(5, 6)
    dev = Device(grid)
    w = series.row_weights(grid.lat)
    with pytest.raises(QdError, match="qd_spectra_configure: at most 32 entries"):
        dev.spectra_configure(entry_list(33), 1, w)
    with pytest.raises(QdError, match=r"qd_spectra_configure: unknown op \(0 = field a, 1 = sqrt\(a\*a \+ b\*b\)\)"):
        dev.spectra_configure([(2, "U", None)], 1, w)
    with pytest.raises(QdError, match="qd_spectra_configure: op 1 cannot pair PRECIP with another field"):
        dev.spectra_configure([(1, "PRECIP", "U")], 1, w)
    with pytest.raises(QdError, match="qd_spectra_configure: field a is not an f64 plane"):
        dev.spectra_configure([(0, "LAND_MASK", None)], 1, w)
    for call in (dev.spectra_sample, dev.spectra_log, dev.spectra_reset, lambda: dev.spectra_schedule([1, 1]), dev.spectra_sums):
        with pytest.raises(QdError, match="not configured"):     # none of the refused calls left a configuration
            call()
    with pytest.raises(QdError, match="qd_state_digest: ref SPECTRA_SUMS: the lat-resolved spectra sums are not configured"):
        dev.digest(["SPECTRA_SUMS"])
    dev.close()
    # a row whose working set does not fit: one line that names the limit; the other form of the same grid fits and runs
    dev = Device(qa.SphericalGrid(5, 6480))
    w2 = series.row_weights(np.linspace(-90, 90, 5))
    monkeypatch.setenv("QD_SPECTRA_FORM", "direct")
    with pytest.raises(QdError, match=r"qd_spectra_configure: a row of n_lon = 6480 needs 155528 bytes of LDS, a workgroup may take 153600 of "
                                      r"the CU's 163840$"):
        dev.spectra_configure([(0, "U", None)], 1, w2)
    monkeypatch.delenv("QD_SPECTRA_FORM")
    x = np.random.default_rng(1).normal(size=(5, 6480))
    dev.upload_now("U", x)
    dev.spectra_configure([(0, "U", None)], 1, w2)               # 106952 bytes: above the 64 KB a workgroup takes by default
    dev.spectra_sample()
    P, re_x, im_x = spectra.dft_reference(x, parts=True)
    got = dev.spectra_sums()[0][0]
    assert (np.abs(got - P) <= power_bound(x, P, re_x, im_x)).all()
    dev.close()
    dev = Device(qa.SphericalGrid(5, 9600))
    with pytest.raises(QdError, match=r"a row of n_lon = 9600 needs 158440 bytes of LDS, a workgroup may take 153600"):
        dev.spectra_configure([(0, "U", None)], 1, w2)
    dev.close()
    grp = BandGroup(qa.SphericalGrid(73, 144), 2)
    with pytest.raises(QdError, match=r"qd_spectra_configure: the spectra need a whole-globe handle \(world == 1, n_rows == n_lat\); "
                                      r"latitude bands are not supported"):
        grp.devs[0].spectra_configure([(0, "U", None)], 1, series.row_weights(np.linspace(-90, 90, 73)))
    grp.close()
    # a span: the wrong schedule length, more samples than the log holds -- nothing runs
    sim = make(monkeypatch, 19, 36, routing=False)
    sim.dev.spectra_configure([(0, "U", None)], 0, series.row_weights(sim.grid.lat))
    flags = dict(with_ocean=True, with_physics=True, pass_albedo=False, with_hydrology=True)
    counters = sim.dev.counters()
    stars = sim.forcing.star_table(DT * np.arange(SPECTRA_LOG_CAP + 1))
    sim.dev.spectra_schedule([1, 1, 1])
    with pytest.raises(QdError, match="a qd_spectra_schedule must cover exactly the n steps of the span"):
        sim.dev.step_n(stars[:2], DT, **flags)
    sim.dev.step_n(stars[:2], DT, **flags)                       # the refused span left no schedule behind
    assert sim.dev.counters()[0] == counters[0] + 2 and len(sim.dev.spectra_log()) == 0
    counters = sim.dev.counters()
    sim.dev.spectra_schedule(np.ones(SPECTRA_LOG_CAP + 1, dtype=np.int32))
    with pytest.raises(QdError, match="the span's spectra records would overflow the log of QD_SPECTRA_LOG_CAP"):
        sim.dev.step_n(stars, DT, **flags)
    assert sim.dev.counters() == counters and len(sim.dev.spectra_log()) == 0
    # the host's refusals: an unknown field, an ocean field without the ocean
    with pytest.raises(ValueError, match="QD_SPECTRA_FIELDS: unknown field 'NOPE'"):
        spectra.from_env(sim.dev, sim.grid, {"QD_SPECTRA": "1", "QD_SPECTRA_FIELDS": "U,NOPE"})
    with pytest.raises(ValueError, match="QD_SPECTRA_FIELDS: field 'SST' needs the ocean, which is off in this run"):
        spectra.from_env(sim.dev, sim.grid, {"QD_SPECTRA": "1", "QD_SPECTRA_FIELDS": "U,SST"}, with_ocean=False, day=72000.0)
    sim.dev.close()


# ---------------------------------------------------------------- 3: a span equals single steps
def attach(sim, tmp_path, *, every=1, S=None, fields=None, lat=True, lane=True):
    """A Spectra on the run's handle; lane=False: configured, but no participant of the spans (the class seam's twin)."""
    from qingdai_amd import spectra
    days = spectra.EVERY_DAYS if S is None else S * DT / sim.day_seconds
    cfg = {"enabled": True, "every": every, "lat": lat, "every_days": days, "fields": fields}
    sim.spectra_lines = []
    s = spectra.Spectra(sim.dev, sim.grid, cfg, with_ocean=sim.ocean is not None, dt=DT, day=sim.day_seconds, out=sim.spectra_lines.append,
                        output_dir=str(tmp_path))
    assert S is None or s.S == S
    sim.spectra = s if lane else None
    return s


SPAN_FIELDS = ["U", "V", "H", "Q", "CLOUD", "PRECIP", "OLR", "WIND_SPEED"]


@pytest.mark.parametrize("every", [1, 2])
def test_span_equals_single_steps(gpu, monkeypatch, tmp_path, every):
    monkeypatch.delenv("QD_SPECTRA_FORM", raising=False)
    got = []
    for cuts in ([6], [2, 4]):
        sim = make(monkeypatch, 19, 36, routing=False)
        s = attach(sim, tmp_path, every=every, fields=SPAN_FIELDS)
        for n in cuts:
            sim.run_steps(n)
        recs, times, steps = s.window()
        assert steps.tolist() == list(range(0, 6, every)) and times.tolist() == [k * DT for k in range(0, 6, every)]
        got.append((recs, s.sums()))
        sim.dev.close()
    sim = make(monkeypatch, 19, 36, routing=False)
    s = attach(sim, tmp_path, every=every, fields=SPAN_FIELDS, lane=False)
    for i in range(6):
        sim.run_steps(1)
        if i % every == 0:
            sim.dev.spectra_sample()
    got.append((sim.dev.spectra_log(), sim.dev.spectra_sums()))
    sim.dev.close()
    assert got[0][0].shape == (6 // every, 8 * (19 + 1)) and got[0][1][0].shape == (8, 19, 19)
    for k, (recs, (sums, count)) in enumerate(got):
        assert same(recs, got[0][0]) and same(sums, got[0][1][0]) and count == 6 // every, (every, k)
    from qingdai_amd import spectra
    power, bad = spectra.split_records(got[0][0], 8, 36)
    assert np.isfinite(got[0][0]).all() and not bad.any() and (power >= 0.0).all()
    p = SPAN_FIELDS.index("PRECIP")                              # liveness: a record is its own step's
    assert any(not np.array_equal(power[i, p], power[i + 1, p]) for i in range(6 // every - 1))
    assert not os.path.exists(tmp_path / "spectra") and sim.spectra_lines == []


# ---------------------------------------------------------------- 4: lazily stored diagnostics and PRECIP inside a span
def test_lazy_diagnostics_and_precip_are_the_steps_own(gpu, monkeypatch, tmp_path):
    """Device.step_n without the hydrology bit: inside a span only the last step stores OLR ... unless a reader comes with the
    span; and the next step's precipitation block overwrites PRECIP inside the ocean step.  The record of step s is the class-seam
    record behind a span that ends with s."""
    monkeypatch.delenv("QD_SPECTRA_FORM", raising=False)
    names = ["OLR", "PRECIP", "U", "EFLUX"]
    flags = dict(with_ocean=True, with_physics=True, pass_albedo=False, with_hydrology=False)
    a = make(monkeypatch, 19, 36, routing=False)
    attach(a, tmp_path, fields=names, lane=False)
    stars = a.forcing.star_table(DT * np.arange(5))
    for i in range(5):
        a.dev.step_n(stars[i:i + 1], DT, **flags)
        a.dev.spectra_sample()
    want = a.dev.spectra_log()
    a.dev.close()
    b = make(monkeypatch, 19, 36, routing=False)
    s = attach(b, tmp_path, fields=names)
    b.dev.step_n(stars, DT, spectra=s, **flags)
    recs = s.span_deliver(DT)
    assert recs.shape == (5, 4 * (19 + 1)) and s.i == 5 and same(recs, want)
    per = 19 + 1
    for k in (0, 1):                                             # OLR and PRECIP move from step to step
        assert all(not np.array_equal(recs[i, k * per:(k + 1) * per], recs[i + 1, k * per:(k + 1) * per]) for i in range(4)), names[k]
    b.dev.close()


# ---------------------------------------------------------------- 5: the other lanes and the state do not notice
FIRES = {0: 3, 2: 1, 5: 3}


def test_no_effect_on_the_other_lanes(gpu, monkeypatch, tmp_path):
    from qingdai_amd import ncio
    from test_gpu_history import attach as attach_history
    from test_gpu_series import attach as attach_series
    monkeypatch.delenv("QD_SPECTRA_FORM", raising=False)
    runs = {}
    for on in (False, True):
        out = tmp_path / ("on" if on else "off")
        sim = make(monkeypatch, 19, 36, fires=FIRES)
        assert sim.routing is not None and sim.budget is not None
        attach_history(sim, out, S=4)
        attach_series(sim, out, S=5)
        if on:
            attach(sim, out, S=3, fields=["U", "V", "PRECIP"])
        sim.dev.timing(True)
        for n in (3, 4):
            sim.run_steps(n)
        sim.dev.sync()
        launches = (sim.dev.timing_get("spectra")[1], sim.dev.timing_get("spectra_combine")[1])
        sim.dev.timing(False)
        files = sorted(os.listdir(out / "history"))
        sfiles = sorted(os.listdir(out / "series"))
        runs[on] = dict(files=files, arrays=[ncio.read_nc(str(out / "history" / f))[0] for f in files], sums=sim.dev.history_read(),
                        sfiles=sfiles, sarrays=[ncio.read_nc(str(out / "series" / f))[0] for f in sfiles], open_series=sim.series.window(),
                        budget=list(sim.budget_lines), history=list(sim.history_lines), series=list(sim.series_lines),
                        routing=fetch(sim.dev, ["RUNOFF"]), digest=sim.digest(), launches=launches,
                        spectra=sorted(os.listdir(out / "spectra")) if os.path.exists(out / "spectra") else None)
        sim.dev.close()
    off, on = runs[False], runs[True]
    assert off["launches"] == (0, 0) and off["spectra"] is None  # at 0: no spectra scope in the timing tables, no directory
    assert on["launches"] == (2 * 7, 2 * 7) and len(on["spectra"]) == 2      # PRECIP's group and the others', every step
    assert on["files"] == off["files"] and len(off["files"]) == 1 and on["sfiles"] == off["sfiles"] and len(off["sfiles"]) == 1
    for va, vb in zip(on["arrays"] + on["sarrays"], off["arrays"] + off["sarrays"]):
        assert va.keys() == vb.keys() and all(np.asarray(va[k]).tobytes() == np.asarray(vb[k]).tobytes() for k in va)
    assert on["sums"][1] == off["sums"][1] == 3 and on["sums"][0].tobytes() == off["sums"][0].tobytes()
    assert all(np.asarray(a).tobytes() == np.asarray(b).tobytes() for a, b in zip(on["open_series"], off["open_series"]))
    assert on["budget"] == off["budget"] and len(off["budget"]) > 0 and on["history"] == off["history"] and on["series"] == off["series"]
    assert on["routing"]["RUNOFF"].tobytes() == off["routing"]["RUNOFF"].tobytes()
    d_on = {k: v for k, v in on["digest"].items() if k not in ("SPECTRA_SUMS", "run")}
    d_off = {k: v for k, v in off["digest"].items() if k != "run"}
    assert d_on == d_off and len(d_off) > 20 and "SPECTRA_SUMS" in on["digest"] and "SPECTRA_SUMS" not in off["digest"]


# ---------------------------------------------------------------- 6: the driver
def test_driver_main(gpu, tmp_path, monkeypatch, capsys):
    from qingdai_amd import driver, ncio, spectra
    env = {"QD_N_LAT": "19", "QD_N_LON": "36", "QD_SIM_DAYS": "0.125", "QD_ECO_ENABLE": "0", "QD_DYN_DIAG_PRINT": "0", "QD_USE_OCEAN": "1",
           "QD_HYDRO_ENABLE": "0", "QD_SPECTRA": "1", "QD_SPECTRA_EVERY_DAYS": "0.05", "QD_SPECTRA_EVERY": "2"}
    _set_env(monkeypatch, env)
    on = tmp_path / "on"
    on.mkdir()
    monkeypatch.chdir(on)
    assert driver.main() == 0
    out = capsys.readouterr().out
    day = 72000.0
    lines = [s for s in out.splitlines() if s.startswith("[Spectra]")]
    assert len(lines) == 3 and [int(re.search(r": (\d+) samples", s).group(1)) for s in lines] == [6, 6, 3], out
    assert all(re.fullmatch(r"\[Spectra\] day \d+\.\d+–\d+\.\d+: \d+ samples \| U hi=\S+→\S+ V hi=\S+→\S+ H hi=\S+→\S+ Q hi=\S+→\S+ "
                            r"CLOUD hi=\S+→\S+", s) for s in lines), lines
    files = sorted(os.listdir(on / "output" / "spectra"))
    assert len(files) == 3 and all(re.fullmatch(r"spectra_day_\d+\.\d+_\d+\.\d+\.nc", f) for f in files), files
    names = [n.lower() for n in spectra.DEFAULT_FIELDS]
    first = []
    for f, (steps, complete) in zip(files, ((range(0, 12, 2), 1), (range(12, 24, 2), 1), (range(24, 30, 2), 0))):
        v, _ = ncio.read_nc(str(on / "output" / "spectra" / f))
        steps = list(steps)
        assert v["step"].tolist() == steps and v["time_seconds"].tolist() == [k * DT for k in steps], f
        assert (int(v["complete"]), int(v["sample_every"]), int(v["lat_resolved"]), int(v["n_samples"]), float(v["dt_seconds"])) == \
            (complete, 2, 1, len(steps), DT)
        a, b = (float(x) for x in re.fullmatch(r"spectra_day_(.+)_(.+)\.nc", f).groups())
        assert abs(a - steps[0] * DT / day) <= 0.005 and abs(b - steps[-1] * DT / day) <= 0.005, f
        assert v["lat"].shape == (19,) and v["wavenumber"].tolist() == list(range(19))
        assert set(v) == ({"time_seconds", "step", "wavenumber", "lat", "dt_seconds", "sample_every", "lat_resolved", "n_samples", "complete",
                           "ke_power"} | {f"{n}_{q}" for n in names for q in ("power", "bad_rows", "hi_frac", "power_lat")})
        for n in names:
            assert v[f"{n}_power"].shape == (len(steps), 19) and v[f"{n}_power_lat"].shape == (19, 19) and not v[f"{n}_bad_rows"].any(), n
            assert np.isfinite(v[f"{n}_power"]).all() and (v[f"{n}_power"] >= 0).all() and np.isfinite(v[f"{n}_power_lat"]).all(), n
            assert (np.isnan(v[f"{n}_hi_frac"]) | ((v[f"{n}_hi_frac"] >= 0) & (v[f"{n}_hi_frac"] <= 1))).all(), n
            # the window mean of the rows, combined like a record, is the mean of the records up to rounding
            from qingdai_amd import series
            w = series.row_weights(v["lat"])
            assert np.allclose((w[:, None] * v[f"{n}_power_lat"]).sum(axis=0) / w.sum(), v[f"{n}_power"].mean(axis=0), rtol=1e-12, atol=0.0), n
        assert np.array_equal(v["ke_power"], 0.5 * (v["u_power"] + v["v_power"]))
        first.append(float(v["u_power"][0, 1]))
    assert len(set(first)) == 3
    # the same run without the switch: no directory, no line
    monkeypatch.delenv("QD_SPECTRA")
    off = tmp_path / "off"
    off.mkdir()
    monkeypatch.chdir(off)
    assert driver.main() == 0
    assert "[Spectra]" not in capsys.readouterr().out and not os.path.exists(off / "output" / "spectra")


# ---------------------------------------------------------------- 7: stopped inside a window and resumed
def test_resumed_run_writes_the_uncut_runs_files(gpu, tmp_path, monkeypatch, capsys):
    from qingdai_amd import driver, ncio

    def env(data, days, **extra):
        e = {"QD_N_LAT": "19", "QD_N_LON": "36", "QD_DT_SECONDS": "300", "QD_SIM_DAYS": str(days), "QD_DYN_DIAG_PRINT": "0", "QD_ECO_ENABLE": "0",
             "QD_HYDRO_ENABLE": "0", "QD_USE_OCEAN": "1", "QD_DATA_DIR": str(tmp_path / data), "QD_OUTPUT_DIR": str(tmp_path / ("out_" + data)),
             "QD_SPECTRA": "1", "QD_SPECTRA_EVERY_DAYS": "0.05", "QD_SPECTRA_EVERY": "1", "QD_SPECTRA_FIELDS": "U,PRECIP,OLR,WIND_SPEED,SST",
             "QD_CHECKPOINT": "1"}
        e.update(extra)
        return e
    monkeypatch.chdir(tmp_path)
    _set_env(monkeypatch, env("whole", 0.125))                   # 30 steps: windows 0-11 and 12-23, 24-29 stays open
    assert driver.main() == 0
    whole = capsys.readouterr().out
    assert whole.count("[Spectra] day ") == 2 and " 30 steps" in whole and "[Checkpoint] (final) wrote" in whole
    _set_env(monkeypatch, env("cut", 0.0625))                    # 15 steps: stopped inside the window 12-23
    assert driver.main() == 0
    first = capsys.readouterr().out
    assert first.count("[Spectra] day ") == 1 and " 15 steps" in first and "[Checkpoint] loaded" not in first
    assert driver.main() == 0
    second = capsys.readouterr().out
    assert "[Checkpoint] loaded" in second and "step 15" in second and second.count("[Spectra] day ") == 1     # each file written once
    files = lambda d: sorted(os.listdir(tmp_path / ("out_" + d) / "spectra"))
    assert files("cut") == files("whole") and len(files("whole")) == 2
    for name in files("whole"):
        va, vb = (ncio.read_nc(str(tmp_path / ("out_" + d) / "spectra" / name))[0] for d in ("whole", "cut"))
        assert va.keys() == vb.keys() and all(np.asarray(va[k]).tobytes() == np.asarray(vb[k]).tobytes() for k in va), name
        assert int(va["complete"]) == 1 and len(va["step"]) == 12 and int(va["n_samples"]) == 12 and "sst_power_lat" in va
    wa, wb = (ncio.read_nc(str(tmp_path / d / "checkpoint.nc")) for d in ("whole", "cut"))
    assert wa[1]["run_digest"] == wb[1]["run_digest"] and wa[1]["digest_SPECTRA_SUMS"] == wb[1]["digest_SPECTRA_SUMS"]
    for k in ("spectra_records", "spectra_times", "spectra_steps", "spectra_clock", "spectra_sums"):    # the open window 24-29 travels
        assert np.asarray(wa[0][k]).tobytes() == np.asarray(wb[0][k]).tobytes(), k
    assert wa[0]["spectra_clock"].tolist() == [30.0, 6.0, 6.0] and wa[0]["spectra_steps"].tolist() == [24.0, 25.0, 26.0, 27.0, 28.0, 29.0]
    assert wa[0]["spectra_sums"].shape == (5, 19, 19)
    key = "U,PRECIP,OLR,WIND_SPEED,SST|every=1|lat=1"
    assert "spectra=" + key in wa[1]["subsystems"]
    # another spectra configuration, or none: refused with the subsystem wording; and a lane-off file by a lane-on run
    _set_env(monkeypatch, env("cut", 0.0625, QD_SPECTRA_LAT="0"))
    assert driver.main() == 2
    assert f"the subsystem set differs: the spectra lane is '{key}' in the file and '{key[:-1]}0' in this run" in capsys.readouterr().out
    _set_env(monkeypatch, env("cut", 0.0625, QD_SPECTRA="0"))
    assert driver.main() == 2
    assert f"the subsystem set differs: the spectra lane is '{key}' in the file and '-' in this run" in capsys.readouterr().out
    _set_env(monkeypatch, env("off", 0.0625, QD_SPECTRA="0"))
    assert driver.main() == 0
    capsys.readouterr()
    _set_env(monkeypatch, env("off", 0.0625))
    assert driver.main() == 2
    assert f"the subsystem set differs: the spectra lane is '-' in the file and '{key}' in this run" in capsys.readouterr().out
