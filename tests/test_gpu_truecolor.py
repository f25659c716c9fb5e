"""GPU (-m gpu): the true-colour frame on the device (qd_truecolor_*, qingdai_amd/csrc/qd_truecolor.hip) against the goldens
recorded from the reference's plot_true_color, small and awkward shapes against the NumPy restatement (tests/truecolor_ref.py),
the u8 rounding and the row flip, the footprint of a render on the state, driver.main with the switch on and off, and the refusals.

Tolerance (truecolor_ref.START / MEASURED / BOUND).  The masks, the tie cells and the NaN positions must be exact.  The f64 rgb and
the two sea-ice numbers go through the device's exp and pow and, for the sums, a blocked order; their deviation is max |a - b| over
the entries that are not NaN.  The bound in force is ten times the largest deviation measured on the MI355X over the seven goldens,
never looser than 1e-12.  Measured on the MI355X: 2.220e-16 at most (the sea-ice numbers of six goldens; the rgb 1.110e-16 at most,
0 for `base` and `rivers`, which take no pow), so the bound in force is 2.3e-15.  Every test prints its deviations."""
import ctypes
import glob
import os

import numpy as np
import pytest

import truecolor_ref as ref

pytestmark = pytest.mark.gpu

HERE = os.path.dirname(os.path.abspath(__file__))
GOLDENS = sorted(glob.glob(os.path.join(HERE, "golden", "truecolor_*_19x36.npz")))


def _case(path):
    return os.path.basename(path)[len("truecolor_"):-len("_19x36.npz")]


def _device(shape, inp):
    import qingdai_amd as qa
    from qingdai_amd.device import Device
    dev = Device(qa.SphericalGrid(*shape))
    dev.upload_now("LAND_MASK", np.asarray(inp["land_mask"]).astype(np.uint8))
    for fid, key in ref.FIELDS.items():
        dev.upload_now(fid, np.asarray(inp[key], dtype=np.float64))
    return dev


def _render(dev, cfg):
    p, eco_tab, phyto_tab, lake, bands, flow = cfg
    dev.truecolor_configure(p, eco_tab, phyto_tab, bands, lake)
    area, mean_h = dev.truecolor_render(want_f64=True, flow=flow)
    return {"rgb": dev.truecolor_rgb(), "img": dev.truecolor_image(), "sea_ice": np.array([area, mean_h])}


def deviation(got, want):
    got, want = np.asarray(got, dtype=float), np.asarray(want, dtype=float)
    assert got.shape == want.shape and np.array_equal(np.isnan(got), np.isnan(want)), "NaN positions differ"
    ok = ~np.isnan(want)
    return float(np.max(np.abs(got[ok] - want[ok]))) if ok.any() else 0.0


def _check(got, want, what):
    e_rgb, e_ice = deviation(got["rgb"], want["rgb"]), deviation(got["sea_ice"], want["sea_ice"])
    print(f"{what}: rgb {e_rgb:.3e} sea ice {e_ice:.3e} (bound {ref.BOUND:.1e})")
    assert e_rgb <= ref.BOUND and e_ice <= ref.BOUND, (what, e_rgb, e_ice)
    # the u8 image is exactly the stated rounding of the device's own rgb, and within one level of the rounding of the expected rgb
    assert np.array_equal(got["img"], ref.quantise(got["rgb"])), what
    assert int(np.max(np.abs(got["img"].astype(int) - ref.quantise(want["rgb"]).astype(int)))) <= 1, what
    return max(e_rgb, e_ice)


@pytest.mark.parametrize("path", GOLDENS, ids=_case)
def test_c_abi_vs_reference_goldens(gpu, path, monkeypatch):
    from qingdai_amd.truecolor import truecolor_line
    z = np.load(path)
    case = _case(path)
    ref.set_env(monkeypatch, ref.golden_meta(z)["env"])
    dev = _device((19, 36), z)
    assert np.array_equal(dev.grid.lat, z["lat"])
    cfg = ref.golden_config(z)
    got = _render(dev, cfg)
    worst = _check(got, z, case)
    print(f"{case}: largest deviation from the reference {worst:.3e}")
    p = cfg[0]
    assert truecolor_line(got["sea_ice"][0], got["sea_ice"][1], float(p.ice_frac_thr), float(p.cloud_alpha)) == str(z["line"])
    cloud3 = z["cloud"][..., None]
    if case == "base":
        # the sea-ice mask as the output shows it: the ice-coloured cells under the cloud blend, exactly the reference's mask
        ice = np.clip(np.array(ref.ICE) * (1.0 - p.cloud_alpha * cloud3) + (p.cloud_alpha * cloud3) * p.cloud_white, 0.0, 1.0)
        assert np.array_equal(np.all(got["rgb"] == ice, axis=-1), z["sea_ice_mask"])
        # the row flip: only the northern rows carry the ice cap, so the image matches the golden flipped and not the golden as it lies
        assert z["sea_ice_mask"][-4:].sum() > 40 and z["sea_ice_mask"][1:4].sum() == 0
        want8 = ref.quantise(z["rgb"])
        assert int(np.max(np.abs(got["img"].astype(int) - want8.astype(int)))) <= 1
        assert int(np.max(np.abs(got["img"].astype(int) - want8[::-1].astype(int)))) > 100
        assert np.array_equal(got["img"][0], ref.quantise(got["rgb"])[0]) and np.array_equal(got["img"][0], ref.quantise(got["rgb"][-1:])[0])
    if case == "nonfinite":
        nanpix = np.isnan(z["rgb"]).any(axis=-1)
        assert nanpix.sum() == 1 and np.isnan(got["rgb"][nanpix]).all() and got["img"][::-1][nanpix].tolist() == [[0, 0, 0]]
    # twice: identical bytes
    again = _render(dev, cfg)
    assert again["img"].tobytes() == got["img"].tobytes() and np.array_equal(again["rgb"], got["rgb"], equal_nan=True)
    assert np.array_equal(again["sea_ice"], got["sea_ice"])
    # a render without the f64 copy gives the same image and refuses the f64 download
    from qingdai_amd._lib import QdError
    dev.truecolor_render(want_f64=False, flow=cfg[5])
    assert dev.truecolor_image().tobytes() == got["img"].tobytes()
    with pytest.raises(QdError, match="did not keep the f64 rgb"):
        dev.truecolor_rgb()
    dev.close()


def test_empty_mask_gives_zero_mean(gpu, monkeypatch):
    z = dict(np.load([p for p in GOLDENS if _case(p) == "base"][0]))
    ref.set_env(monkeypatch, {})
    z["h_ice"] = np.zeros_like(z["h_ice"])
    dev = _device((19, 36), z)
    from qingdai_amd.truecolor import build_config
    got = _render(dev, build_config(None, None, None, None) + (None, None))
    assert got["sea_ice"].tolist() == [0.0, 0.0]
    _check(got, ref.render(z, build_config(None, None, None, None)[0]), "empty mask")
    dev.close()


def _synthetic(shape, nb, seed):
    """Random inputs with every overlay on and nb bands in both band sets -> (inputs, config)."""
    from qingdai_amd import _lib
    r = np.random.default_rng(seed)
    land = (r.uniform(size=shape) < 0.5).astype(np.uint8)
    inp = {"land_mask": land, "h_ice": np.where(r.uniform(size=shape) < 0.5, 0.0, r.uniform(0.2, 2.0, shape)),
           "C_snow": r.uniform(-0.2, 1.4, shape), "cloud": r.uniform(0.0, 1.0, shape), "T_s": r.uniform(250.0, 300.0, shape),
           "isr_A": r.uniform(0.0, 700.0, shape), "isr_B": r.uniform(0.0, 300.0, shape), "eco_f": r.uniform(-0.1, 1.1, shape)}
    inp["isr_A"][:, : shape[1] // 3] = 0.0
    inp["isr_B"][:, : shape[1] // 2] = 0.0                      # a night side on the left third
    inp["isr"] = inp["isr_A"] + inp["isr_B"]
    p = _lib.qd_truecolor_params(1, 1, 0, 1, 1, 1, 1, nb, nb, 0, 0.5, 0.15, 0.2, 0.6, 1.8, 1.35, 0.2, 2.2, 0.85, 262.0, 0.6, 0.95, 1e6, 0.45, 0.4)

    def tab(rows):
        t = r.uniform(0.05, 1.0, (rows, nb))
        t[-6:-3] /= t[-6:-3].sum(axis=1, keepdims=True)          # the channel weights are normalised
        return t
    bands = r.uniform(0.0, 0.3, (nb,) + shape)
    bands[:, land == 1] = np.nan
    flow = 10.0 ** r.uniform(4.0, 8.0, shape)
    lake = (r.uniform(size=shape) < 0.2).astype(np.uint8)
    return inp, (p, tab(7), tab(6), lake, bands, flow)


@pytest.mark.parametrize("shape", [(5, 4), (7, 65)], ids=lambda s: f"{s[0]}x{s[1]}")
@pytest.mark.parametrize("nb", [1, 16])
def test_shapes_vs_restatement(gpu, shape, nb):
    """5 x 4: the smallest grid qd_create accepts, fewer cells than one wave; 7 x 65: a row longer than a wave, two workgroups."""
    inp, cfg = _synthetic(shape, nb, 100 * shape[0] + nb)
    dev = _device(shape, inp)
    got = _render(dev, cfg)
    p, eco_tab, phyto_tab, lake, bands, flow = cfg
    want = ref.render(inp, p, eco_tab, phyto_tab, bands, lake, flow, lat=dev.grid.lat)
    _check(got, want, f"{shape[0]}x{shape[1]} nb={nb}")
    dev.close()


def test_render_leaves_the_state_alone(gpu, monkeypatch):
    from qingdai_amd import driver, _lib
    from qingdai_amd.truecolor import TrueColor
    ref.set_env(monkeypatch, {"QD_PHYTO_DAILY": "1"})
    sim = driver.Simulation(n_lat=19, n_lon=36, use_ocean=True, quiet=True)
    sim.bootstrap_ecology()
    sim.run_steps(3)

    def state():
        out = {}
        for name in _lib.FIELDS:
            sim.dev._host.pop(name, None)
            out[name] = sim.dev.get(name).copy()
        out["bands"] = sim.phyto_daily.get_alpha_maps()[0]
        out["tracers"] = sim.dev.phyto_download()
        out["counters"] = np.array(sim.dev.counters())
        return out
    before = state()
    tc = TrueColor(sim)
    img, area, mean_h = tc.render(want_f64=True)
    assert tc.params.veg == 1 and tc.params.oceancolor == 1 and img.shape == (19, 36, 3) and np.isfinite(tc.rgb()).all()
    after = state()
    for k in before:
        assert np.array_equal(before[k], after[k], equal_nan=True), k
    # the resident inputs, downloaded and put through the restatement, give the frame the device made
    inp = {key: after[fid] for fid, key in ref.FIELDS.items()}
    inp["land_mask"] = sim.land_mask
    from qingdai_amd.truecolor import build_config
    p, eco_tab, phyto_tab, lake = build_config(None, sim.eco, sim.phyto_daily, None)
    want = ref.render(inp, p, eco_tab, phyto_tab, after["bands"], lake, None, lat=sim.grid.lat)
    _check({"rgb": tc.rgb(), "img": img, "sea_ice": np.array([area, mean_h])}, want, "resident state")
    ocean_open = (sim.land_mask == 0) & ~want["sea_ice_mask"]
    plain = ref.render(inp, build_config(None, None, None, None)[0], lat=sim.grid.lat)["rgb"]
    assert np.any(want["rgb"][ocean_open] != plain[ocean_open]) and np.any(want["rgb"][sim.land_mask == 1] != plain[sim.land_mask == 1])
    sim.dev.close()


def _main_env(tmp_path, monkeypatch, extra):
    env = {"QD_N_LAT": "19", "QD_N_LON": "36", "QD_DT_SECONDS": "2400", "QD_SIM_DAYS": "0.222", "QD_PLOT_EVERY_DAYS": "0.085",
           "QD_DYN_DIAG_PRINT": "0", "QD_AUTOSAVE_LOAD": "0", "QD_PHYTO_DAILY": "1", "QD_HYDRO_AUTOGEN": "1", "QD_HYDRO_DT_HOURS": "2",
           "QD_HYDRO_NETCDF": str(tmp_path / "hydrology.nc"), "QD_RIVER_MIN_KGPS": "1.0", "QD_LOAD_PLANKTON": "0"}
    env.update(extra)
    ref.set_env(monkeypatch, env)


def test_driver_main_writes_the_frames(gpu, tmp_path, monkeypatch, capsys):
    """Interval 3 steps (0.085 d of 86400 s over dt = 2400 s), 7 steps: frames at the steps 0, 3 and 6, named by t_i / day = 0, 0.1, 0.2."""
    from qingdai_amd import driver, ncio
    from qingdai_amd.imgio import read_png
    from qingdai_amd.truecolor import TrueColor, plot_interval_steps
    monkeypatch.chdir(tmp_path)
    _main_env(tmp_path, monkeypatch, {"QD_DATA_DIR": str(tmp_path / "data0")})
    assert plot_interval_steps(os.environ, 2400) == 3
    assert driver.main() == 0                                   # the switch unset
    plain = capsys.readouterr().out
    assert "[TrueColor]" not in plain and not os.path.exists(tmp_path / "output")
    assert "[Plots] matplotlib panels are not produced by the device driver (out of the hot path)." in plain and " 7 steps" in plain
    _main_env(tmp_path, monkeypatch, {"QD_DATA_DIR": str(tmp_path / "data1"), "QD_TRUECOLOR": "1", "QD_ECO_DIVERSITY_ENABLE": "1",
                                      "QD_ECO_DIVERSITY_EVERY_DAYS": "0.15"})
    assert driver.main() == 0
    on = capsys.readouterr().out
    names = ["true_color_day_000.0.png", "true_color_day_000.1.png", "true_color_day_000.2.png"]
    assert sorted(f for f in os.listdir(tmp_path / "output") if f.endswith(".png")) == names
    lines = [ln for ln in on.splitlines() if ln.startswith("[TrueColor]")]
    assert len(lines) == 3 and all("sea_ice_area≈" in ln and "(thr=0.15, alpha=0.6)" in ln for ln in lines)
    assert "[Plots] only the true-colour frame is produced" in on and "frame skipped" not in on
    # the diversity clock fires on the steps 0 and 5 (t / day = 0 and 0.1667 >= 0.15), the frames on 0, 3, 6: both keep their steps
    div = [ln.split(":")[0] for ln in on.splitlines() if ln.startswith("[Diversity]")]
    assert div == ["[Diversity] day 0.00", "[Diversity] day 0.17"], div
    # the final state of the two runs (the restart layout is f4 for both)
    a, _ = ncio.read_nc(str(tmp_path / "data0" / "atmosphere.nc"), list(driver.RESTART_VARS))
    b, _ = ncio.read_nc(str(tmp_path / "data1" / "atmosphere.nc"), list(driver.RESTART_VARS))
    for k in a:
        assert np.array_equal(np.asarray(a[k]), np.asarray(b[k]), equal_nan=True), k
    # a twin stepped to the same steps renders the same frames and prints the same lines
    _main_env(tmp_path, monkeypatch, {"QD_DATA_DIR": str(tmp_path / "data2")})
    twin = driver.Simulation()
    twin.enable_routing()
    twin.bootstrap_ecology()
    tc = TrueColor(twin)
    for name, n, line in zip(names, (1, 3, 3), lines):
        twin.run_steps(n)
        img, area, mean_h = tc.render()
        assert np.array_equal(read_png(str(tmp_path / "output" / name)), img), name
        assert tc.line(area, mean_h) == line
        assert img.shape == (19, 36, 3)
    assert tc.params.rivers == 1 and tc.params.veg == 1 and tc.params.oceancolor == 1
    capsys.readouterr()
    # ... and equals, bit for bit, a run that was never cut into chunks and never rendered
    whole = driver.Simulation()
    whole.enable_routing()
    whole.bootstrap_ecology()
    whole.run_steps(7)
    from qingdai_amd import _lib
    for name in _lib.FIELDS:
        for s in (twin, whole):
            s.dev._host.pop(name, None)
        assert np.array_equal(twin.dev.get(name), whole.dev.get(name), equal_nan=True), name
    assert np.array_equal(twin.dev.route_download("FLOW"), whole.dev.route_download("FLOW"))
    twin.dev.close()
    whole.dev.close()


def test_a_failed_write_does_not_stop_the_run(gpu, tmp_path, monkeypatch, capsys):
    from qingdai_amd import driver
    monkeypatch.chdir(tmp_path)
    (tmp_path / "blocked").write_text("a file where the output directory should be")
    _main_env(tmp_path, monkeypatch, {"QD_DATA_DIR": str(tmp_path / "data"), "QD_TRUECOLOR": "1", "QD_OUTPUT_DIR": str(tmp_path / "blocked"),
                                      "QD_HYDRO_ENABLE": "0", "QD_PHYTO_DAILY": "0", "QD_SIM_DAYS": "0.05"})
    assert driver.main() == 0
    out = capsys.readouterr().out
    assert out.count("[TrueColor] frame skipped") == 1 and "--- Simulation Finished ---" in out


def test_refusals(gpu, monkeypatch):
    import qingdai_amd as qa
    from qingdai_amd import _lib
    from qingdai_amd._lib import QdError
    from qingdai_amd.device import Device
    from qingdai_amd.truecolor import build_config
    ref.set_env(monkeypatch, {})
    p = build_config(None, None, None, None)[0]
    dev = Device(qa.SphericalGrid(19, 36))
    with pytest.raises(QdError, match="qd_truecolor_configure has not been called"):
        dev.truecolor_render()
    with pytest.raises(QdError, match="no frame on this handle"):
        dev.truecolor_image()
    assert dev.lib.qd_truecolor_configure(dev.h, ctypes.byref(p), ctypes.sizeof(p) - 8, None, None, None, None) != 0
    assert b"struct size mismatch" in dev.lib.qd_last_error(dev.h)
    bad = _lib.qd_truecolor_params.from_buffer_copy(bytes(p))
    bad.veg, bad.nb_eco = 1, 17
    with pytest.raises(QdError, match="band counts out of range"):
        dev.truecolor_configure(bad, np.zeros((7, 17)))
    bad.nb_eco = 0
    with pytest.raises(QdError, match="needs nb_eco >= 1"):
        dev.truecolor_configure(bad)
    rivers = _lib.qd_truecolor_params.from_buffer_copy(bytes(p))
    rivers.rivers = 1
    dev.truecolor_configure(rivers)
    with pytest.raises(QdError, match="no routing network is configured"):
        dev.truecolor_render()
    dev.truecolor_configure(p)
    dev.truecolor_render()
    buf = np.zeros(5, dtype=np.uint8)
    with pytest.raises(QdError, match="size mismatch"):
        dev._chk(dev.lib.qd_truecolor_download(dev.h, 0, buf.ctypes.data, 5), "qd_truecolor_download")
    with pytest.raises(QdError, match="which must be 0"):
        dev._chk(dev.lib.qd_truecolor_download(dev.h, 2, buf.ctypes.data, 5), "qd_truecolor_download")
    dev.close()
    band = Device(qa.SphericalGrid(73, 144), row0=20, n_rows=30, halo=6)
    assert band.lib.qd_truecolor_configure(band.h, ctypes.byref(p), ctypes.sizeof(p), None, None, None, None) != 0
    assert b"latitude bands are not supported" in band.lib.qd_last_error(band.h)
    assert band.lib.qd_truecolor_render(band.h, 0, None, None) != 0 and b"latitude bands are not supported" in band.lib.qd_last_error(band.h)
    band.close()
