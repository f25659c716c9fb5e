"""GPU (-m gpu): the fused step kernels against the oracle at the ragged grid shapes where their launchers change form
(tests/step_form_cases.py): n_lon of 63 / 64 / 65, n_lat of 11 / 12 / 13, a last column strip or group of one column (58 k + 1,
60 k + 1, 62 k + 1), one and two streaming row strips, two column tiles of the tile kernels, the 38-row threshold of k_ocn_fused.
Whole-globe handles only; every grid has at most ~3 500 cells.

Which form ran is not guessed from the shape: every case asserts the form report (Device.step_forms, qd_step_forms) against the
form its row was written for, and test_table_reaches_every_form asserts that the rows together reach every momentum form, every
tail kernel, the deferred mean both ways, the fix list both ways and a last strip of 1, < 3 and >= 3 columns.

The runs that compare one device form with another are test_gpu_bands._run(1, ...) restated (run_forms below: the same uploads and
the same qd_step_n call, plus the form report read before the handle closes), cached per (shape, switches, state).

  family                          bound (relative to the field's max-norm) and where it comes from       worst measured (MI355X)
  atmosphere step, 2 steps        STEP_TOL = 1e-9 (test_gpu_parity.py); the oracle's own answer to a     1.2e-14  LH_release_last, (27, 125)
                                  1e-15 wind perturbation is <= 5e-12 (test_step_form_cases_cpu.py)      (u, v, h, q: <= 3.9e-15)
  ocean, one 20 s sub-step x 2    1e-12, eta 1e-10 (test_gpu_atsize.py: nothing amplified yet); all      4.6e-16  vo, (47, 61); eta 7.0e-14, (12, 64)
                                  rows, pole rows, last two columns
  ocean, 3 steps of 2-6 sub-steps STEP_TOL; sub-step counts equal; oracle sensitivity <= 3e-12           2.6e-12  eta, (47, 61)
  coupled loop, 3 steps           atmosphere / surface: STEP_TOL.  uo, vo, eta: 1000 x the CPU-measured  atmosphere 5.0e-14 cloud, (13, 65)
                                  sensitivity of DriverOracle, floored at STEP_TOL, capped at 1e-7:      eta 1.3e-11 (13, 65), 2.5e-12 (25, 117),
                                  sensitivity 5.7e-16 / 4.4e-16 / 1.8e-15 at (13, 65) / (25, 117) /      2.9e-12 (29, 121)
                                  (29, 121) -> bound 1e-9 at all three
  form against form               bit for bit: QD_FUSED_FAST=0 / 3, QD_TAIL_GENERAL=1 (also spikes and   0: bit-equal
                                  NaN in columns 0, n_lon - 1 and the last group), QD_TAIL_FIX=0,
                                  QD_MEAN_IN_MOMENTUM=0
                                  TAIL_TOL = 1e-11 (test_gpu_bands.py): QD_OCN_TAIL=0, QD_TAIL_V=1,      7.2e-13  QD_OCN_TAIL=0, (25, 117)
                                  QD_OCN_FUSED=1 (+ QD_FUSED_SEQ=1)
                                  QD_FUSED=0: 1e-9, uo / vo / eta 1e-7 (test_fused_kernel_paths_agree)   1.9e-11  (25, 117)

Found here and fixed (qd_ocntail.hip, k_ocn_tail_fast): at 29 x 121 (60 k + 1 columns) the slim SST wave of the group before the last
holds column n_lon - 1 on lane 62; its folded gather wants columns 0 and 1 = lanes 63 and 64, and lane 64 is lane 0 of the wave
(column 58).  The SST of column n_lon - 2 was off by 2.1e-12 against the oracle after one sub-step (the general form, the two-launch
form and the unfused kernels agreed with it to 1.9e-16), and QD_TAIL_GENERAL=1 was not bit-equal from the spike state.
"""
import numpy as np
import pytest

import step_form_cases as sc
from util import STATE, DIAG, relerr, run_device_time_step, run_oracle_time_step

pytestmark = pytest.mark.gpu

STEP_TOL, TAIL_TOL = sc.STEP_TOL, sc.TAIL_TOL
SWITCH_NAMES = ("QD_FUSED", "QD_FUSED_FAST", "QD_OCN_TAIL", "QD_TAIL_GENERAL", "QD_TAIL_FIX", "QD_MEAN_IN_MOMENTUM", "QD_TAIL_V",
                "QD_OCN_FUSED", "QD_FUSED_SEQ")
OCEAN_FIELDS = ("UO", "VO", "ETA")

_RUNS = {}          # (shape, switches, state) -> ({field: array}, form report)


def set_switches(monkeypatch, switches):
    """The switches are read in qd_create: the environment is set before the handle is built."""
    for s in SWITCH_NAMES:
        monkeypatch.delenv(s, raising=False)
    for k, v in sc.env_of(switches).items():
        monkeypatch.setenv(k, v)


def spikes(shape):
    """test_fast_tail_waves_equal_the_general_ones_bit_for_bit's spike / NaN state, placed in column 0, column n_lon - 1 and the first
    column of the last column group of k_ocn_tail_fast (60 columns a group)"""
    nlat, nlon = shape
    jl = (-(-nlon // 60) - 1) * 60

    def mutate(st):
        st["UO"] = np.zeros(shape); st["VO"] = np.zeros(shape)
        st["UO"][nlat // 2, 0] = 1e6; st["VO"][nlat // 3, nlon - 1] = -2e6; st["UO"][nlat // 2 + 2, jl] = np.nan
        st["VO"][nlat // 2 - 1, jl] = 3e5
    return mutate


def run_forms(monkeypatch, shape, switches=(), state="seeded"):
    """test_gpu_bands._run(1, n_lat, n_lon, 3, dict(energy_w=1, ocean_cfl=step_form_cases.run_cfl), True, True) under `switches`"""
    key = (tuple(shape), tuple(switches), state)
    if key not in _RUNS:
        from qingdai_amd.device import Device
        from test_gpu_bands import _seed_state, _setup
        set_switches(monkeypatch, switches)
        nlat, nlon = shape
        qa, grid, mask, alb, fric, p = _setup(nlat, nlon, dict(energy_w=1.0, ocean_cfl=sc.run_cfl(shape)))
        stars = qa.ThermalForcing(qa.SphericalGrid(nlat, nlon), qa.OrbitalSystem()).star_table([i * sc.DT for i in range(sc.NSTEPS)])
        st = _seed_state(nlat, nlon, 3)
        if state == "spikes":
            spikes(shape)(st)
        dev = Device(grid, p)
        for k, v in {"LAND_MASK": mask, "FRICTION": fric, "BASE_ALBEDO": alb, **st}.items():
            dev.upload_now(k, v)
        dev.step_n(stars, sc.DT, with_ocean=True, with_physics=True, pass_albedo=True)
        out = {k: dev.get(k).copy() for k in ("U", "V", "H", "TS", "Q", "CLOUD", "HICE", "UO", "VO", "ETA", "SST")}
        forms = dev.step_forms()
        dev.close()
        _RUNS[key] = (out, forms)
    return _RUNS[key]


def expected_forms(shape, switch=None):
    want = dict(sc.CASES[tuple(shape)]["forms"])
    if switch:
        for k in sc.SWITCH_FREE.get(switch, ()):
            want.pop(k, None)
        want.update(sc.SWITCH_FORMS[switch])
        if switch.startswith("QD_OCN_FUSED"):
            ok = want["fused_ok"]
            want.update(last_use_fused1=ok, last_tail_kernel=4 if ok else 1)
    # the report holds the geometry of the forms the handle takes, zeros for the others
    if want.get("dyn_stream") == 0:
        want = {k: v for k, v in want.items() if not (k.startswith(("dyn_", "ocn_")) and not k.endswith("_stream"))}
    if want.get("tail_kernel") == 0:
        want = {k: v for k, v in want.items() if not k.startswith("tail_") or k == "tail_kernel"}
        want.pop("last_tail_acc", None)
    return want


# ---------------------------------------------------------------- which form ran
@pytest.mark.parametrize("shape", sc.SHAPES)
def test_form_report(gpu, monkeypatch, shape):
    """The form report of the row's default handle and of every switch the row crosses, against the form the row was written for."""
    runs = [None] + list(sc.CASES[shape]["switches"])
    if "QD_OCN_FUSED=1" in runs:
        runs.append("QD_OCN_FUSED=1,QD_FUSED_SEQ=1")
    for sw in runs:
        switches = tuple(sw.split(",")) if sw else ()
        _, forms = run_forms(monkeypatch, shape, switches)
        print(shape, sw, forms)
        want = expected_forms(shape, switches[0] if switches else None)
        if len(switches) == 2:
            want["fused_seq"] = want["fused_ok"]
        assert forms["last_nsub"] >= 2, (shape, sw, forms["last_nsub"])
        diff = {k: (forms[k], v) for k, v in want.items() if forms[k] != v}
        assert not diff, (shape, sw, "got, want:", diff)


def test_table_reaches_every_form(gpu, monkeypatch):
    """If a launcher threshold moves, this fails instead of the table silently losing a form."""
    seen = []
    for shape in sc.SHAPES:
        for sw in [()] + [(s,) for s in sc.CASES[shape]["switches"]]:
            seen.append((shape, sw, run_forms(monkeypatch, shape, sw)[1]))
    def any_(**kv):
        return any(all(f[k] == v for k, v in kv.items()) for _, _, f in seen)
    assert any_(last_dyn_form=1) and any_(last_ocn_form=1)                                    # streaming momentum
    assert any_(last_dyn_form=2, tile_dyn_fast=0) and any_(last_ocn_form=2, tile_ocn_fast=0)   # tiles, EXACT
    assert any(f["last_dyn_form"] == 2 and f["tile_dyn_fast"] > 0 and f["tile_ocn_fast"] > 0 for _, _, f in seen)      # tiles, FAST
    assert any(f["last_dyn_form"] == 2 and f["tile_ntr"] > 1 and sh[0] % f["tile_tr"] for sh, _, f in seen)             # ragged last row tile
    assert any_(last_dyn_form=0, last_ocn_form=0)                                            # unfused reference-order kernels
    assert any_(dyn_stream=1, dyn_nrs=1) and any(f["dyn_stream"] == 1 and f["dyn_nrs"] == 2 and f["dyn_vb"] > 0 for _, _, f in seen)
    for kernel in (0, 1, 2, 3, 4):                                                             # two launches, fast storing, fast fix list, stream, fused
        assert any_(last_tail_kernel=kernel), kernel
    assert any_(last_mean_form=1) and any_(last_mean_form=0, last_use_tail=1)
    assert any_(last_fix_now=1, last_tail_kernel=2) and any_(last_fix_now=0, last_tail_kernel=1)
    assert any_(last_use_tail=1, tail_general=1) and any_(fused_ok=0, dyn_stream=1) and any_(last_use_fused1=1)
    # a last column strip / group of one column, of fewer than the three halo columns, and of at least three
    strips = {sc.last_widths(sh[1])[0] for sh, _, f in seen if f["last_dyn_form"] in (1, 2)}
    groups = {sc.last_widths(sh[1])[1] for sh, _, f in seen if f["last_tail_kernel"] in (1, 2)}
    groups_v = {sc.last_widths(sh[1])[2] for sh, _, f in seen if f["last_tail_kernel"] == 3}
    stream_strips = {sc.last_widths(sh[1])[0] for sh, _, f in seen if f["last_dyn_form"] == 1}
    tile_strips = {sc.last_widths(sh[1])[0] for sh, _, f in seen if f["last_dyn_form"] == 2}
    assert 1 in stream_strips and 1 in tile_strips and 1 in groups and 1 in groups_v, (stream_strips, tile_strips, groups, groups_v)
    for widths in (strips, groups):
        assert min(widths) < 3 and max(widths) >= 3, widths
    for sh, _, f in seen:                                                                      # the report's strip counts are the shape's
        if f["dyn_stream"]:
            assert f["dyn_ntc"] == -(-sh[1] // 58) and f["ocn_ntc"] == f["dyn_ntc"]
        if f["tail_kernel"]:
            assert f["tail_ntc"] == -(-sh[1] // (60 if f["tail_kernel"] == 1 else 62))


# ---------------------------------------------------------------- atmosphere step against the oracle
_ORACLE_TS = {}


def _atmosphere(shape, over):
    key = (shape, tuple(sorted(over.items())))
    meta, d = sc.ts_case(shape, over)
    if key not in _ORACLE_TS:
        _ORACLE_TS[key] = run_oracle_time_step(meta, d)
    o = _ORACLE_TS[key]
    m = run_device_time_step(meta, d)
    errs = {k: relerr(getattr(m, k), getattr(o, k)) for k in STATE + DIAG + ("cloud_eff_last",)}
    forms = m._dev.step_forms()
    print("atmosphere", shape, over, "form", forms["last_dyn_form"], {k: f"{e:.1e}" for k, e in errs.items()})
    assert forms["last_dyn_form"] == sc.CASES[shape]["forms"].get("last_dyn_form", 1)
    for k, e in errs.items():
        assert e < STEP_TOL, (shape, over, k, e)


@pytest.mark.parametrize("shape", sc.SHAPES)
def test_atmosphere_step_vs_oracle(gpu, monkeypatch, shape):
    """run_device_time_step against run_oracle_time_step, step_form_cases.ATM_NSTEPS steps from the wet / cloudy / icy seeded state"""
    set_switches(monkeypatch, ())
    _atmosphere(shape, {})


@pytest.mark.parametrize("over", [{"filter_type": "hyper4"}, {"mom_scheme": 1}], ids=["hyper4", "primitive"])
@pytest.mark.parametrize("shape", sc.MODE_SHAPES)
def test_atmosphere_step_modes_vs_oracle(gpu, monkeypatch, shape, over):
    """The same with filter_type = hyper4 and with the primitive momentum scheme (k_dyn_stream<true>)"""
    set_switches(monkeypatch, ())
    _atmosphere(shape, over)


# ---------------------------------------------------------------- ocean step against the oracle
def _ocean_pairs(oc, oo):
    return {"uo": (oc.uo, oo.uo), "vo": (oc.vo, oo.vo), "eta": (oc.eta, oo.eta), "SST": (oc.Ts, oo.Ts)}


@pytest.mark.parametrize("shape", sc.SHAPES)
def test_ocean_single_substep_every_row_vs_oracle(gpu, monkeypatch, shape):
    """test_ocean_single_substep_every_row_vs_oracle_at_721x1440 at the table's shapes: one 20 s step (one sub-step) from a fast state,
    then a second that applies the deferred mean; every row, the two pole rows and the last two columns on their own."""
    import qd_oracle as qo
    import qingdai_amd as qa
    set_switches(monkeypatch, ())
    nlat, nlon = shape
    mask, s = sc.fast_ocean_state(shape)
    oo = qo.OceanOracle(qo.Grid(nlat, nlon), mask, qo.defaults(), init_Ts=s["sst"].copy())
    oo.uo, oo.vo, oo.eta = s["uo"].copy(), s["vo"].copy(), s["eta"].copy()
    oc = qa.WindDrivenSlabOcean(qa.SphericalGrid(nlat, nlon), mask, 50.0, init_Ts=s["sst"])
    oc.uo, oc.vo, oc.eta = s["uo"], s["vo"], s["eta"]
    tol = {"uo": 1e-12, "vo": 1e-12, "eta": 1e-10, "SST": 1e-12}
    for k in range(2):
        oc.step(20.0, s["u_atm"], s["v_atm"], Q_net=s["qnet"], ice_mask=s["ice"])
        oo.step(20.0, s["u_atm"], s["v_atm"], Q_net=s["qnet"], ice_mask=s["ice"])
        assert oc.last_n_sub == oo.last_n_sub == 1
        pairs = _ocean_pairs(oc, oo)
        errs = {kk: relerr(a, b) for kk, (a, b) in pairs.items()}
        capped = int(np.sum(np.hypot(oo.uo, oo.vo) > 2.999))
        print("ocean one sub-step", shape, k, {kk: f"{e:.1e}" for kk, e in errs.items()}, "cells at the cap:", capped)
        assert capped > 0
        for kk, (a, b) in pairs.items():
            scale = max(float(np.max(np.abs(b))), 1e-300)
            for what, sel in (("all", np.s_[:, :]), ("pole rows", np.s_[[0, nlat - 1], :]), ("last two columns", np.s_[:, nlon - 2:])):
                e = float(np.max(np.abs(a[sel] - b[sel]))) / scale
                assert e < tol[kk], (shape, k, kk, what, e)
    want = sc.CASES[shape]["forms"]
    forms = oc._dev.step_forms()
    assert forms["last_ocn_form"] == want.get("last_ocn_form", 1) and forms["last_use_tail"] == want.get("last_use_tail", 1), forms


@pytest.mark.parametrize("shape", sc.SHAPES)
def test_ocean_three_steps_vs_oracle(gpu, monkeypatch, shape):
    """Three full steps at the row's ocean_cfl (2-6 sub-steps: the deferred-mean forms) against OceanOracle"""
    import qd_oracle as qo
    import qingdai_amd as qa
    set_switches(monkeypatch, ())
    nlat, nlon = shape
    cfl = sc.CASES[shape]["cfl"]
    mask, d = sc.ocean_case(shape)
    oo = qo.OceanOracle(qo.Grid(nlat, nlon), mask, qo.defaults(ocean_cfl=cfl), init_Ts=d["init_Ts"].copy())
    oo.uo, oo.vo, oo.eta = d["init_uo"].copy(), d["init_vo"].copy(), d["init_eta"].copy()
    oc = qa.WindDrivenSlabOcean(qa.SphericalGrid(nlat, nlon), mask, 50.0, init_Ts=d["init_Ts"], params=qa.QdParams(ocean_cfl=cfl))
    oc.uo, oc.vo, oc.eta = d["init_uo"], d["init_vo"], d["init_eta"]
    for _ in range(sc.NSTEPS):
        oc.step(sc.DT, d["u_atm"], d["v_atm"], Q_net=d["Q_net"], ice_mask=d["ice_mask"])
        oo.step(sc.DT, d["u_atm"], d["v_atm"], Q_net=d["Q_net"], ice_mask=d["ice_mask"])
        assert oc.last_n_sub == oo.last_n_sub and 2 <= oo.last_n_sub <= 6, (oc.last_n_sub, oo.last_n_sub)
    errs = {k: relerr(a, b) for k, (a, b) in _ocean_pairs(oc, oo).items()}
    forms = oc._dev.step_forms()
    print("ocean three steps", shape, "n_sub", oo.last_n_sub, "mean_form", forms["last_mean_form"], {k: f"{e:.1e}" for k, e in errs.items()})
    assert forms["last_mean_form"] == sc.CASES[shape]["forms"].get("last_mean_form", forms["last_mean_form"])
    for k, e in errs.items():
        assert e < STEP_TOL, (shape, k, e)


# ---------------------------------------------------------------- coupled loop against DriverOracle
@pytest.mark.parametrize("shape", sc.COUPLED_SHAPES)
def test_coupled_loop_vs_driver_oracle(gpu, monkeypatch, shape):
    """test_driver_loop_vs_oracle (ocean on, physics on, the cold low-h state) at three of the shapes, three steps.  uo, vo, eta:
    1000 x the oracle's own sensitivity to a 1e-15 perturbation of the wind (step_form_cases.coupled_bound)."""
    import qingdai_amd as qa
    from qingdai_amd.driver import Simulation
    set_switches(monkeypatch, ())
    nlat, nlon = shape
    sim = Simulation(nlat, nlon, params=qa.QdParams(), use_ocean=True, quiet=True, ecology=False)
    st = sc.coupled_state(shape, sim.land_mask)
    sim.gcm.h, sim.gcm.T_s, sim.gcm.u, sim.gcm.v = st["h"], st["T_s"], st["u"], st["v"]
    sim.dev.set("S_SNOW", st["S_snow"])
    m, oc, d = sc.coupled_oracle(shape, sim.land_mask, sim.base_albedo, sim.friction)
    sim.run_steps(sc.NSTEPS)
    pairs = {"u": (sim.gcm.u, m.u), "v": (sim.gcm.v, m.v), "h": (sim.gcm.h, m.h), "T_s": (sim.gcm.T_s, m.T_s),
             "q": (sim.gcm.q, m.q), "cloud": (sim.gcm.cloud_cover, m.cloud_cover), "precip": (sim.dev.get("PRECIP"), d.precip),
             "albedo": (sim.dev.get("ALBEDO"), d.albedo), "S_snow": (sim.dev.get("S_SNOW"), d.S_snow),
             "C_snow": (sim.dev.get("C_SNOW"), d.C_snow), "W_land": (sim.dev.get("W_LAND"), d.W_land),
             "runoff": (sim.dev.get("RUNOFF"), d.R_flux), "SST": (sim.ocean.Ts, oc.Ts),
             "uo": (sim.ocean.uo, oc.uo), "vo": (sim.ocean.vo, oc.vo), "eta": (sim.ocean.eta, oc.eta)}
    errs = {k: relerr(a, b) for k, (a, b) in pairs.items()}
    bound = sc.coupled_bound(shape)
    print("coupled", shape, "n_sub", oc.last_n_sub, "sensitivity", sc.COUPLED_SENS[shape], "bound", bound, {k: f"{e:.1e}" for k, e in errs.items()},
          "snow cells:", int((d.S_snow > 0).sum()))
    assert (d.S_snow > 0).sum() > 0                                  # the snow branch fired
    assert sim.dev.last_ocean_nsub() == oc.last_n_sub
    for k, e in errs.items():
        assert e < (bound if k in ("uo", "vo", "eta") else STEP_TOL), (shape, k, e)


# ---------------------------------------------------------------- form against form
def _bit_equal(a, b, what):
    for k in a:
        assert np.array_equal(a[k], b[k], equal_nan=True), (what, k, relerr(np.nan_to_num(a[k]), np.nan_to_num(b[k])))


@pytest.mark.parametrize("shape", sc.SHAPES)
def test_forms_agree(gpu, monkeypatch, shape):
    """Each switch of the row against the row's default run: bit for bit where the forms do the same arithmetic in the same order
    (QD_FUSED_FAST, QD_TAIL_GENERAL also from the spike / NaN state, QD_TAIL_FIX, QD_MEAN_IN_MOMENTUM), TAIL_TOL where only the order
    of the eta sum differs (QD_OCN_TAIL=0, QD_TAIL_V=1), test_fused_kernel_paths_agree's bounds against the unfused kernels."""
    base, _ = run_forms(monkeypatch, shape)
    worst = {}
    for sw in sc.CASES[shape]["switches"]:
        got, _ = run_forms(monkeypatch, shape, (sw,))
        if sw in ("QD_FUSED_FAST=0", "QD_FUSED_FAST=3", "QD_TAIL_GENERAL=1", "QD_TAIL_FIX=0", "QD_MEAN_IN_MOMENTUM=0"):
            _bit_equal(got, base, (shape, sw))
            if sw == "QD_TAIL_GENERAL=1":
                _bit_equal(run_forms(monkeypatch, shape, (sw,), "spikes")[0], run_forms(monkeypatch, shape, (), "spikes")[0], (shape, sw, "spikes"))
            continue
        errs = {k: relerr(got[k], base[k]) for k in base}
        worst[sw] = max(errs.values())
        for k, e in errs.items():
            if sw == "QD_FUSED=0":
                assert e < (1e-7 if k in OCEAN_FIELDS else 1e-9), (shape, sw, k, e)
            elif sw in ("QD_OCN_TAIL=0", "QD_TAIL_V=1"):
                assert e < TAIL_TOL, (shape, sw, k, e)
            else:
                assert sw == "QD_OCN_FUSED=1" and e < TAIL_TOL, (shape, sw, k, e)
        if sw == "QD_OCN_FUSED=1":                            # the same launch with every strip on its sequential form
            seq, _ = run_forms(monkeypatch, shape, (sw, "QD_FUSED_SEQ=1"))
            for k in base:
                assert relerr(seq[k], base[k]) < TAIL_TOL, (shape, sw, "QD_FUSED_SEQ=1", k, relerr(seq[k], base[k]))
    print("forms", shape, {k: f"{e:.1e}" for k, e in worst.items()})
