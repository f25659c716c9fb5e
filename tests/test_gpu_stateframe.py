"""GPU (-m gpu): the 15-panel state frame on the device (qd_stateframe_*, qingdai_amd/csrc/qd_stateframe.hip) against the goldens
recorded from the reference's plot_state under matplotlib, small and awkward shapes against the NumPy restatement
(tests/stateframe_ref.py), the footprint of a render on the state, driver.main with the switch on and off, and the refusals.

What must be exact and what has a tolerance.  Fourteen fields are pointwise f64 arithmetic with contraction off (sqrt is correctly
rounded): field stack, scan extremes, levels, band indices and pixels must equal the restatement's bit for bit, with no cell excused.
The vorticity (panel 9) is a stencil held to the operator tolerance of tests/test_gpu_parity.py (1e-13 of the max-norm,
stateframe_ref.VORT_TOL); its band index and its pixel may differ only at cells within 1e-9 of the level range of a level, at most
1 % of the panel's cells (scripts/gen_golden_stateframe.py asserts that the golden inputs stay under that cap).

The driver test and the oracle.  The panels 5 and 11 of every firing are held to the oracle driver's precipitation and albedo of the
firing step at the whole-step tolerance of tests/test_gpu_parity.py (STEP_TOL = 1e-9 of the max-norm), in the configuration that
test uses for the driver loop (dt = 300 s, ecology, plankton and routing off).  The run starts at QD_ORBIT_EPOCH_SECONDS = 2900 so
that the two firings (steps 0 and 3, three steps apart) carry different file names; the first firing has no precipitation yet
(a start from rest), the second has it on most cells, and the test asserts that.  The fields of both firings must also equal, bit
for bit, those of a twin that ran one step per call with QD_HOIST_PRECIP=0 and QD_LAZY_DIAG=0, whose PRECIP / ALBEDO / EFLUX /
PCOND / OLR are the step's own by construction."""
import ctypes
import glob
import json
import os

import numpy as np
import pytest

import stateframe_ref as ref

pytestmark = pytest.mark.gpu

HERE = os.path.dirname(os.path.abspath(__file__))
GOLDENS = sorted(glob.glob(os.path.join(HERE, "golden", "stateframe_*_19x36.npz")))
STEP_TOL = 1e-9


def _case(path):
    return os.path.basename(path)[len("stateframe_"):-len("_19x36.npz")]


def _device(shape, inp):
    import qingdai_amd as qa
    from qingdai_amd.device import Device
    dev = Device(qa.SphericalGrid(*shape))
    dev.upload_now("LAND_MASK", np.asarray(inp["land_mask"]).astype(np.uint8))
    for fid, key in ref.INPUTS.items():
        dev.upload_now(fid, np.asarray(inp[key], dtype=np.float64))
    return dev


def _frame(dev, ocean, flow=None, lake=None, routed=False):
    """One frame through qingdai_amd.stateframe.StateFrame on a bare Device -> (StateFrame, mosaic, bands, fields)."""
    import types
    from qingdai_amd.stateframe import StateFrame
    routing = types.SimpleNamespace(lake_mask=lake) if routed else None
    sf = StateFrame(dev, routing=routing, ocean=ocean)
    img = sf.render(want_stacks=True, flow=flow)
    return sf, img, sf.bands(), sf.fields()


def _compare(what, sf, img, bands, F, inp, lat, ocean, flow=None, lake=None, p0=1.0e5, rho_a=1.2, H=8000.0, cap=True):
    """The device's frame against the restatement of the same inputs.  cap: at most 1 % of the vorticity panel's cells may lie next to a
    level (inputs made for the test; a model state at rest has whole rows of zero vorticity on the middle level)."""
    from qingdai_amd import stateframe as sfm
    e = sfm.read_env()
    want_F = ref.fields(inp, lat, ps_abs=e["ps_abs"], ocean=ocean, p0=p0, rho_a=rho_a, H=H)
    want_scan = ref.scan(want_F, inp["isr_A"], inp["isr_B"])
    n_lat, n_lon = want_F.shape[1:]
    # the field stack: exact, the vorticity to the operator tolerance
    for k in range(15):
        if k == 8:
            ok = np.isfinite(want_F[k])
            assert np.array_equal(ok, np.isfinite(F[k])), what
            dev = float(np.max(np.abs(F[k][ok] - want_F[k][ok]))) / float(np.max(np.abs(want_F[k][ok])))
            print(f"{what}: vorticity deviation {dev:.3e} of the max-norm (bound {ref.VORT_TOL:.0e})")
            assert dev <= ref.VORT_TOL, (what, dev)
        else:
            assert np.array_equal(F[k], want_F[k], equal_nan=True), (what, k)
    # the scan: exact for the pointwise panels, |vort| max and the vorticity extremes to the tolerance
    got = sf.scan
    assert np.array_equal(got["t_min"], want_scan["t_min"], equal_nan=True) and np.array_equal(got["t_max"], want_scan["t_max"], equal_nan=True), what
    for p in ref.AUTO_PANELS:
        if p == 9:
            scale = max(abs(want_scan["auto"][9][0]), abs(want_scan["auto"][9][1]))
            assert np.allclose(got["auto"][9], want_scan["auto"][9], rtol=0, atol=ref.VORT_TOL * scale), what
        else:
            assert got["auto"][p] == want_scan["auto"][p], (what, p, got["auto"][p], want_scan["auto"][p])
    assert abs(got["vmax"] - want_scan["vmax"]) <= ref.VORT_TOL * want_scan["vmax"], what
    assert got["marks"] == want_scan["marks"] and got["mark_values"] == want_scan["mark_values"], what
    # the table of the restatement's scan: identical levels except for the vorticity panel
    want_tab = sfm.build_table(want_scan, e, ocean=ocean)
    for k in range(15):
        a, b = sf.table["panels"][k], want_tab["panels"][k]
        assert a["constant"] == b["constant"] and (a["levels"] is None) == (b["levels"] is None), (what, k)
        if a["levels"] is not None and k != 8:
            assert a["levels"].tobytes() == b["levels"].tobytes() and np.array_equal(a["colours"], b["colours"]), (what, k)
    # bands and pixels: the device's own fields and table through the restatement must give the device's bands and mosaic exactly;
    # against the restatement's own fields only the vorticity panel may differ, at cells next to a level
    own_bands, own_img = ref.render(F, sf.table, inp["land_mask"], flow=flow, lake=lake, river_min=e["river_min"], river_alpha=e["river_alpha"],
                                    lake_alpha=e["lake_alpha"])
    assert np.array_equal(bands, own_bands), what
    assert np.array_equal(img, own_img), what
    want_bands, want_img = ref.render(want_F, want_tab, inp["land_mask"], flow=flow, lake=lake, river_min=e["river_min"],
                                      river_alpha=e["river_alpha"], lake_alpha=e["lake_alpha"])
    excused = np.zeros((15, n_lat, n_lon), dtype=bool)
    lev9 = want_tab["panels"][8]["levels"]
    excused[8] = ref.near_level(want_F[8], lev9)
    if lev9 is not None and cap:                                # the cap, the extreme cells aside: they sit on the end levels by construction
        ends = (want_F[8] == lev9[0]) | (want_F[8] == lev9[-1])
        assert (excused[8] & ~ends).mean() <= 0.01, (what, (excused[8] & ~ends).mean())
    excused[8] &= F[8] != want_F[8]                             # a cell whose vorticity came out bit for bit needs no excuse
    assert np.array_equal(bands[~excused], want_bands[~excused]), what
    for k in range(15):
        a, b = ref.tile(img, k, n_lat, n_lon), ref.tile(want_img, k, n_lat, n_lon)
        assert np.array_equal(a[~excused[k]], b[~excused[k]]), (what, k)
    gut = np.ones(img.shape[:2], dtype=bool)
    for k in range(15):
        y0, x0 = sfm.tile_origin(k, n_lat, n_lon)
        gut[y0:y0 + n_lat, x0:x0 + n_lon] = False
    assert img.shape == sfm.mosaic_shape(n_lat, n_lon) + (3,) and np.all(img[gut] == 255), what
    return want_F, want_tab


@pytest.mark.parametrize("path", GOLDENS, ids=_case)
def test_c_abi_vs_reference_goldens(gpu, path, monkeypatch):
    z = np.load(path)
    meta = ref.golden_meta(z)
    ref.set_env(monkeypatch, meta["env"])
    dev = _device((19, 36), z)
    assert np.array_equal(dev.grid.lat, z["lat"]) and (dev.params.p0, dev.params.rho_a, dev.params.H) == (meta["p0"], meta["rho_a"], meta["H"])
    routed = meta["routing"]
    flow, lake = (z["flow"], z["lake_mask"]) if routed else (None, None)
    sf, img, bands, F = _frame(dev, meta["ocean"], flow=flow, lake=lake, routed=routed)
    _compare(meta["case"], sf, img, bands, F, z, z["lat"], meta["ocean"], flow=flow, lake=lake)
    # against what matplotlib recorded: the arrays handed to contourf, its levels, its band colours
    for k in range(15):
        want = z["fields"][k]
        if k == 8:
            ok = np.isfinite(want)
            assert np.max(np.abs(F[k][ok] - want[ok])) <= ref.VORT_TOL * np.max(np.abs(want[ok]))
        else:
            assert np.array_equal(F[k], want, equal_nan=True), k
        p, lev = sf.table["panels"][k], z[f"levels_{k}"]
        assert p["constant"] == meta["constant"][k]
        if len(lev) == 0 or p["constant"]:
            continue
        if k == 8:
            assert np.allclose(p["levels"], lev, rtol=0, atol=2 * ref.VORT_TOL * lev[-1])
        else:
            assert p["levels"].tobytes() == lev.tobytes(), k
            assert np.max(np.abs(p["colours"] - z[f"colours_{k}"])) <= 1e-12, k
        excused = ref.near_level(want, lev) if k == 8 else np.zeros(want.shape, dtype=bool)
        assert np.array_equal(bands[k][~excused], ref.band_index(want, lev, p["extend"])[~excused]), k
    if routed:
        assert sf.params.rivers == 1 and sf.params.lakes == 1
    # twice: identical bytes; without the stacks the same mosaic and a refused download
    from qingdai_amd._lib import QdError
    again = sf.render(want_stacks=True, flow=flow)
    assert again.tobytes() == img.tobytes() and np.array_equal(sf.bands(), bands) and np.array_equal(sf.fields(), F, equal_nan=True)
    assert sf.render(flow=flow).tobytes() == img.tobytes()
    with pytest.raises(QdError, match="did not keep the stacks"):
        sf.bands()
    dev.close()


def _synthetic(shape, seed, mark_cols):
    r = np.random.default_rng(seed)
    land = (r.uniform(size=shape) < 0.5).astype(np.uint8)
    land[0, :] = 1
    land[-1, : shape[1] // 2] = 1                                # land on both pole rows: their coast test clips the latitude
    land[1, 1] = 0
    isr_A, isr_B = r.uniform(0.0, 700.0, shape), r.uniform(0.0, 300.0, shape)
    isr_A[0, mark_cols[0]] = 900.0                               # star A on the bottom row, star B on the top row
    isr_B[-1, mark_cols[1]] = 900.0
    inp = {"land_mask": land, "T_s": r.uniform(250.0, 305.0, shape), "h": r.uniform(-300.0, 300.0, shape), "SST": r.uniform(271.0, 303.0, shape),
           "precip": np.where(r.uniform(size=shape) < 0.3, 0.0, r.uniform(0.0, 5e-4, shape)), "cloud": r.uniform(-0.1, 1.1, shape),
           "u": r.uniform(-30.0, 30.0, shape), "v": r.uniform(-20.0, 20.0, shape), "uo": r.uniform(-1.0, 1.0, shape),
           "vo": r.uniform(-0.5, 0.5, shape), "isr_A": isr_A, "isr_B": isr_B, "isr": isr_A + isr_B, "albedo": r.uniform(0.0, 0.9, shape),
           "olr": r.uniform(150.0, 300.0, shape), "q": r.uniform(0.0, 0.02, shape), "E": r.uniform(0.0, 1e-4, shape),
           "P_cond": r.uniform(0.0, 1e-4, shape)}
    flow = 10.0 ** r.uniform(4.0, 8.0, shape)
    lake = (r.uniform(size=shape) < 0.2).astype(np.uint8)
    return inp, flow, lake


@pytest.mark.parametrize("shape,mark_cols,ocean", [((5, 4), (0, 3), True), ((7, 65), (64, 0), False), ((19, 36), (17, 35), True)],
                         ids=["5x4", "7x65", "19x36"])
def test_shapes_vs_restatement(gpu, shape, mark_cols, ocean, monkeypatch):
    """5 x 4: fewer cells than a wave, coast on the pole rows, marks clipped at the bottom and the top row and wrapping at the columns
    0 and 3.  7 x 65: one column past a 64-lane wave -- the periodic neighbours of the coast and of the vorticity and a mark wrapping
    at the columns 64 and 0 cross the wave edge; two workgroups.  19 x 36: 684 cells, a partial last workgroup."""
    ref.set_env(monkeypatch, {"QD_RIVER_ALPHA": "0.6", "QD_LAKE_ALPHA": "0.25", "QD_RIVER_MIN_KGPS": "2.5e5"})
    inp, flow, lake = _synthetic(shape, 100 * shape[0] + shape[1], mark_cols)
    dev = _device(shape, inp)
    sf, img, bands, F = _frame(dev, ocean, flow=flow, lake=lake, routed=True)
    _compare(f"{shape[0]}x{shape[1]}", sf, img, bands, F, inp, dev.grid.lat, ocean, flow=flow, lake=lake)
    n_lon = shape[1]
    assert sf.scan["marks"] == [mark_cols[0], (shape[0] - 1) * n_lon + mark_cols[1]]
    t10 = ref.tile(img, 9, *shape)
    assert t10[0, mark_cols[0]].tolist() == [0, 255, 255] and t10[1, (mark_cols[0] + 1) % n_lon].tolist() == [0, 255, 255]
    assert t10[1, (mark_cols[0] - 1) % n_lon].tolist() == [0, 255, 255]
    assert t10[-1, (mark_cols[1] + 1) % n_lon].tolist() == [255, 255, 0] and t10[-1, (mark_cols[1] - 1) % n_lon].tolist() == [255, 255, 0]
    assert t10[-2, mark_cols[1]].tolist() == [255, 255, 0]
    cst = ref.coast(inp["land_mask"])
    assert cst[0].any() and np.all(ref.tile(img, 5, *shape)[cst] == 0)
    dev.close()


def test_ties_and_nan_in_the_argmax(gpu, monkeypatch):
    """np.argmax: the first of equal maxima in row-major order; a NaN beats every number."""
    ref.set_env(monkeypatch, {})
    inp, _, _ = _synthetic((7, 65), 5, (3, 9))
    inp["isr_A"][:] = 10.0
    inp["isr_A"][2, 64] = inp["isr_A"][2, 63] = inp["isr_A"][5, 0] = 50.0      # the tie spans two workgroups
    inp["isr_B"][4, 1] = np.nan
    inp["isr_B"][6, 7] = np.nan
    inp["isr"] = np.nan_to_num(inp["isr_A"] + inp["isr_B"])
    dev = _device((7, 65), inp)
    sf, img, bands, F = _frame(dev, True)
    assert sf.scan["marks"] == [2 * 65 + 63, 4 * 65 + 1] == [int(np.argmax(inp["isr_A"])), int(np.argmax(inp["isr_B"]))]
    assert sf.scan["mark_values"][0] == 50.0 and np.isnan(sf.scan["mark_values"][1])
    dev.close()


def test_render_leaves_the_state_alone(gpu, monkeypatch):
    from qingdai_amd import driver, _lib
    from qingdai_amd.stateframe import StateFrame
    ref.set_env(monkeypatch, {"QD_PHYTO_DAILY": "1"})
    sim = driver.Simulation(n_lat=19, n_lon=36, use_ocean=True, quiet=True)
    sim.bootstrap_ecology()
    sim.run_steps(3)

    def state():
        out = {}
        for name in _lib.FIELDS:
            sim.dev._host.pop(name, None)
            out[name] = sim.dev.get(name).copy()
        out["tracers"] = sim.dev.phyto_download()
        out["counters"] = np.array(sim.dev.counters())
        return out
    before = state()
    sf = StateFrame(sim)
    img = sf.render(want_stacks=True)
    assert img.shape == (5 * 19 + 24, 3 * 36 + 16, 3) and sf.params.ocean == 1
    after = state()
    for k in before:
        assert np.array_equal(before[k], after[k], equal_nan=True), k
    # the resident inputs, downloaded and put through the restatement, give the frame the device made
    inp = {key: after[fid] for fid, key in ref.INPUTS.items()}
    inp["land_mask"] = sim.land_mask
    dp = sim.dev.params
    _compare("resident state", sf, img, sf.bands(), sf.fields(), inp, sim.grid.lat, True, p0=dp.p0, rho_a=dp.rho_a, H=dp.H, cap=False)
    sim.dev.close()


def _main_env(tmp_path, monkeypatch, extra):
    env = {"QD_N_LAT": "19", "QD_N_LON": "36", "QD_DT_SECONDS": "300", "QD_SIM_DAYS": "0.02", "QD_PLOT_EVERY_DAYS": "0.0105",
           "QD_ORBIT_EPOCH_SECONDS": "2900",
           "QD_DYN_DIAG_PRINT": "0", "QD_AUTOSAVE_LOAD": "0", "QD_ECO_ENABLE": "0", "QD_PHYTO_ENABLE": "0", "QD_HYDRO_ENABLE": "0"}
    env.update(extra)
    ref.set_env(monkeypatch, env)


def test_driver_main_writes_the_frames(gpu, tmp_path, monkeypatch, capsys):
    """Interval 3 steps (0.0105 d of 86400 s over dt = 300 s), 5 steps from t = 2900 s: firings at the steps 0 and 3, named by
    t_i / day = 0.040 and 0.053, i.e. 000.0 and 000.1.  Ecology, plankton and routing are off: the configuration the oracle driver
    restates."""
    import qd_oracle as qo
    from qd_oracle.driver import DriverOracle
    from qingdai_amd import driver
    from qingdai_amd.imgio import read_png
    from qingdai_amd.stateframe import StateFrame
    from util import relerr
    monkeypatch.chdir(tmp_path)
    _main_env(tmp_path, monkeypatch, {"QD_DATA_DIR": str(tmp_path / "data0"), "QD_STATE_PLOT": "0", "QD_TRUECOLOR": "1",
                                      "QD_OUTPUT_DIR": str(tmp_path / "out0")})
    assert driver.main() == 0
    off = capsys.readouterr().out
    assert " 5 steps" in off and not [f for f in os.listdir(tmp_path / "out0") if f.startswith("state_day_")]
    assert "[Plots] only the true-colour frame is produced by the device driver, every 3 steps; the matplotlib panels are not." in off
    order = []
    import qingdai_amd.imgio as imgio
    real_write = imgio.write_png
    monkeypatch.setattr(imgio, "write_png", lambda path, img: (order.append(os.path.basename(path)), real_write(path, img))[1])
    _main_env(tmp_path, monkeypatch, {"QD_DATA_DIR": str(tmp_path / "data1"), "QD_STATE_PLOT": "1", "QD_TRUECOLOR": "1",
                                      "QD_OUTPUT_DIR": str(tmp_path / "out1")})
    assert driver.main() == 0
    on = capsys.readouterr().out
    monkeypatch.setattr(imgio, "write_png", real_write)
    names = ["state_day_000.0", "state_day_000.1"]
    assert sorted(os.listdir(tmp_path / "out1")) == sorted([n + ".png" for n in names] + [n + ".json" for n in names] +
                                                           ["true_color_day_000.0.png", "true_color_day_000.1.png"])
    # the state frame is written before the true-colour frame of the same firing
    assert order == ["state_day_000.0.png", "true_color_day_000.0.png", "state_day_000.1.png", "true_color_day_000.1.png"]
    assert "[Plots] the 15-panel state frame" in on and "frame skipped" not in on
    # with the switch at 0 the run prints what it printed before: the lines of the two runs differ only in the [Plots] line
    strip = lambda s: [ln for ln in s.splitlines() if not ln.startswith("[Plots]") and "steps/s" not in ln]      # noqa: E731
    assert strip(on) == strip(off)
    twin_day = 2 * np.pi / driver.PLANET_OMEGA
    for n in names:
        side = json.load(open(tmp_path / "out1" / (n + ".json"), encoding="utf-8"))
        assert len(side["panels"]) == 15 and side["panels"][0]["title"] == "Surface Temperature (°C)" and side["layout"]["tile"] == [19, 36]
        assert read_png(str(tmp_path / "out1" / (n + ".png"))).shape == (5 * 19 + 24, 3 * 36 + 16, 3)
    assert json.load(open(tmp_path / "out1" / "state_day_000.1.json", encoding="utf-8"))["t_days"] == pytest.approx(3800.0 / twin_day, abs=1e-12)
    # a twin stepped in main's chunks renders the same frames; its panels 5 and 11 against the oracle driver's firing step
    _main_env(tmp_path, monkeypatch, {"QD_DATA_DIR": str(tmp_path / "data2")})
    twin = driver.Simulation()
    twin.t = 2900.0
    sf = StateFrame(twin)
    g, P = qo.Grid(19, 36), qo.defaults()
    m = qo.AtmosOracle(g, twin.friction, twin.land_mask, P, C_s_map=np.where(twin.land_mask == 1, 3e6, P.Cs_ocean).astype(float))
    oc = qo.OceanOracle(g, twin.land_mask, P, init_Ts=np.full((19, 36), 288.0))
    orc = DriverOracle(g, m, oc, qo.Forcing(g), twin.land_mask, twin.base_albedo, P)
    hist = []
    for i in range(4):
        orc.step(2900.0 + i * 300.0, 300)
        hist.append((np.nan_to_num(orc.precip) * 86400.0, orc.albedo.copy()))
    assert not hist[0][0].any() and (hist[3][0] > 0).sum() > 19 * 36 // 2      # the second firing has real precipitation
    assert relerr(hist[2][0], hist[3][0]) > 0.1 and relerr(hist[2][1], hist[3][1]) > 1e-3      # and a step's values are not its neighbour's
    frames = {}
    for name, n, step in zip(names, (1, 3), (0, 3)):
        twin.run_steps(n)
        img = sf.render(want_stacks=True)
        assert np.array_equal(read_png(str(tmp_path / "out1" / (name + ".png"))), img), name
        F = sf.fields()
        frames[step] = F
        e5 = relerr(F[4], hist[step][0]) if hist[step][0].any() else float(np.max(np.abs(F[4])))
        e11 = relerr(F[10], hist[step][1])
        print(f"firing step {step}: panel 5 vs the oracle's precipitation {e5:.3e}, panel 11 vs its albedo {e11:.3e} (bound {STEP_TOL:.0e})")
        assert e5 <= STEP_TOL and e11 <= STEP_TOL, (step, e5, e11)
    twin.dev.close()
    # ... and bit for bit the fields of a run that took one step per call, hoisted nothing and stored every diagnostic on every step
    _main_env(tmp_path, monkeypatch, {"QD_DATA_DIR": str(tmp_path / "data3"), "QD_HOIST_PRECIP": "0", "QD_LAZY_DIAG": "0"})
    plain = driver.Simulation()
    plain.t = 2900.0
    sp = StateFrame(plain)
    for step in range(4):
        plain.run_steps(1)
        if step in frames:
            sp.render(want_stacks=True)
            assert np.array_equal(sp.fields(), frames[step], equal_nan=True), step
    plain.dev.close()


def test_resident_flow_map_of_a_routed_run(gpu, tmp_path, monkeypatch, capsys):
    """flow = NULL: the render reads the routing state's own flow map, as the driver does whenever routing is live.  The panels 1 and 8
    (and every other pixel) against the restatement fed with route_download("FLOW") and the network's lake mask."""
    from qingdai_amd import driver
    from qingdai_amd.stateframe import StateFrame
    monkeypatch.chdir(tmp_path)
    _main_env(tmp_path, monkeypatch, {"QD_DT_SECONDS": "2400", "QD_HYDRO_ENABLE": "1", "QD_HYDRO_AUTOGEN": "1", "QD_HYDRO_DT_HOURS": "2",
                                      "QD_HYDRO_NETCDF": str(tmp_path / "hydrology.nc"), "QD_RIVER_MIN_KGPS": "1.0"})
    sim = driver.Simulation()
    assert sim.enable_routing() is not None
    sim.run_steps(4)                                            # the first routing event falls on the third step
    flow = np.asarray(sim.dev.route_download("FLOW"), dtype=np.float64).reshape(19, 36)
    river = (flow >= 1.0) & (sim.land_mask == 1)
    assert river.sum() > 0
    sf = StateFrame(sim)
    img = sf.render(want_stacks=True)
    assert sf.params.rivers == 1
    lm = getattr(getattr(sim.routing, "net", None), "lake_mask", None)
    lm = getattr(sim.routing, "lake_mask", None) if lm is None else lm
    lake = np.asarray(lm).astype(float).astype(np.uint8) if lm is not None and np.any(lm) else None
    assert sf.params.lakes == (0 if lake is None else 1)
    inp = {}
    for fid, key in ref.INPUTS.items():
        sim.dev._host.pop(fid, None)
        inp[key] = sim.dev.get(fid).copy()
    inp["land_mask"] = sim.land_mask
    dp = sim.dev.params
    _compare("routed run", sf, img, sf.bands(), sf.fields(), inp, sim.grid.lat, True, flow=flow, lake=lake, p0=dp.p0, rho_a=dp.rho_a, H=dp.H,
             cap=False)
    # the overlay is really there: without the flow map the restatement paints other pixels on the two panels, and only there
    plain = ref.render(sf.fields(), sf.table, sim.land_mask, flow=None, lake=lake)[1]
    changed = np.any(img != plain, axis=-1)
    for k in range(15):
        assert ref.tile(changed, k, 19, 36).any() == (k in (0, 7)), k
    capsys.readouterr()
    sim.dev.close()


def test_a_failed_write_does_not_stop_the_run(gpu, tmp_path, monkeypatch, capsys):
    from qingdai_amd import driver
    monkeypatch.chdir(tmp_path)
    (tmp_path / "blocked").write_text("a file where the output directory should be")
    _main_env(tmp_path, monkeypatch, {"QD_DATA_DIR": str(tmp_path / "data"), "QD_STATE_PLOT": "1", "QD_OUTPUT_DIR": str(tmp_path / "blocked")})
    assert driver.main() == 0
    out = capsys.readouterr().out
    assert out.count("[StatePlot] frame skipped") == 1 and "--- Simulation Finished ---" in out


def test_refusals(gpu, monkeypatch):
    import qingdai_amd as qa
    from qingdai_amd import _lib, stateframe as sfm
    from qingdai_amd._lib import QdError
    from qingdai_amd.device import Device
    ref.set_env(monkeypatch, {})
    dev = Device(qa.SphericalGrid(19, 36))
    p = _lib.qd_stateframe_params(0, 1, 0, 0, 1.0e5, 1.2, 8000.0, 1e6, 0.35, 0.40)
    table = _lib.qd_stateframe_table()
    for k in range(15):
        table.panel[k].constant = 1
    with pytest.raises(QdError, match="qd_stateframe_configure has not been called"):
        dev.stateframe_scan()
    with pytest.raises(QdError, match="qd_stateframe_configure has not been called"):
        dev.stateframe_render(table)
    with pytest.raises(QdError, match="no frame on this handle"):
        dev.stateframe_image()
    assert dev.lib.qd_stateframe_configure(dev.h, ctypes.byref(p), ctypes.sizeof(p) - 8, None) != 0
    assert b"struct size mismatch" in dev.lib.qd_last_error(dev.h)
    lakes = _lib.qd_stateframe_params.from_buffer_copy(bytes(p))
    lakes.lakes = 1
    with pytest.raises(QdError, match="lakes set without a lake mask"):
        dev.stateframe_configure(lakes)
    dev.stateframe_configure(p)
    with pytest.raises(QdError, match="qd_stateframe_scan has not been called"):
        dev.stateframe_render(table)
    dev.stateframe_scan()
    assert dev.lib.qd_stateframe_render(dev.h, ctypes.byref(table), ctypes.sizeof(table) - 8, None, 0) != 0
    assert b"struct size mismatch" in dev.lib.qd_last_error(dev.h)
    table.panel[3].constant, table.panel[3].n_levels = 0, 33
    with pytest.raises(QdError, match="more than QD_STATEFRAME_MAX_LEVELS"):
        dev.stateframe_render(table)
    table.panel[3].n_levels = 1
    with pytest.raises(QdError, match="at least 2 levels"):
        dev.stateframe_render(table)
    table.panel[3].constant = 1
    rivers = _lib.qd_stateframe_params.from_buffer_copy(bytes(p))
    rivers.rivers = 1
    dev.stateframe_configure(rivers)
    dev.stateframe_scan()
    with pytest.raises(QdError, match="no routing network is configured"):
        dev.stateframe_render(table)
    dev.stateframe_configure(p)
    dev.stateframe_scan()
    assert dev.lib.qd_set_step_counter(dev.h, 7, 7) == 0       # the handle has stepped since the scan: its plane and extremes are stale
    with pytest.raises(QdError, match="stepped since qd_stateframe_scan"):
        dev.stateframe_render(table)
    dev.stateframe_scan()
    dev.stateframe_render(table)
    img = dev.stateframe_image()
    assert set(np.unique(img).tolist()) <= {0, 255}              # every panel constant: white tiles with the coast overlay (no land: all white)
    buf = np.zeros(5, dtype=np.uint8)
    with pytest.raises(QdError, match="size mismatch"):
        dev._chk(dev.lib.qd_stateframe_download(dev.h, 0, buf.ctypes.data, 5), "qd_stateframe_download")
    with pytest.raises(QdError, match="which must be 0"):
        dev._chk(dev.lib.qd_stateframe_download(dev.h, 3, buf.ctypes.data, 5), "qd_stateframe_download")
    with pytest.raises(QdError, match="did not keep the stacks"):
        dev.stateframe_fields()
    with pytest.raises(ValueError, match="at most 32"):
        tab = sfm.build_table(sfm.unpack_scan(*dev.stateframe_scan()), None)
        tab["panels"][4]["levels"] = np.linspace(0, 30, 40)
        tab["panels"][4]["colours"] = sfm.band_colours("Blues", tab["panels"][4]["levels"], True)
        sfm.pack_table(tab)
    dev.close()
    band = Device(qa.SphericalGrid(73, 144), row0=20, n_rows=30, halo=6)
    assert band.lib.qd_stateframe_configure(band.h, ctypes.byref(p), ctypes.sizeof(p), None) != 0
    assert b"latitude bands are not supported" in band.lib.qd_last_error(band.h)
    marks = (ctypes.c_int64 * 2)()
    out = (ctypes.c_double * _lib.STATEFRAME_SCAN_N)()
    assert band.lib.qd_stateframe_scan(band.h, out, marks) != 0 and b"latitude bands are not supported" in band.lib.qd_last_error(band.h)
    assert band.lib.qd_stateframe_render(band.h, ctypes.byref(table), ctypes.sizeof(table), None, 0) != 0
    assert b"latitude bands are not supported" in band.lib.qd_last_error(band.h)
    band.close()
