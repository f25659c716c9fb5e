"""GPU (-m gpu): the tiles of the ecology, plankton and ISR figures on the device (qd_tiles_*, qingdai_amd/csrc/qd_tiles.hip) against
the goldens recorded from the reference's plot_ecology, plot_plankton_species and plot_isr_components under matplotlib, the scan and
the radix select against NumPy, the resident stack against a host stack, the footprint of a render on the state, driver.main with
the switch on and off, and the refusals.

Everything here is exact.  The planes involve no exp, log or pow and the stacks are reduced plane after plane as NumPy reduces them:
planes are compared with np.array_equal (NaNs in the same cells), band indices on every cell (scripts/gen_golden_figures.py proves that
no finite cell of a golden sits on an interior level), the mosaic byte for byte against the bytes built from the colours matplotlib
recorded.  min, max, argmax and an order statistic are selections: the device returns the value NumPy returns (either zero may stand
for a zero in a sort)."""
import ctypes
import json
import os

import numpy as np
import pytest

import figures_ref as ref

pytestmark = pytest.mark.gpu


def _device(shape, inp, species=None):
    """A bare Device holding the inputs of the figures: the three canopy maps, the two ISR planes, the tracers."""
    import qingdai_amd as qa
    from qingdai_amd.device import Device
    dev = Device(qa.SphericalGrid(*shape))
    dev.upload_now("LAND_MASK", np.asarray(inp["land_mask"]).astype(np.uint8))
    for fid, key in (("ECO_LAI", "lai"), ("ECO_ALPHA", "alpha"), ("ECO_ALPHA_BANDED", "banded"), ("ISR_A", "isr_A"), ("ISR_B", "isr_B")):
        if key in inp:
            dev.upload_now(fid, np.asarray(inp[key], dtype=np.float64))
    if "C" in inp:
        dev.phyto_configure(len(inp["C"]), 0.0, 0.7)
        dev.phyto_upload(np.asarray(inp["C"], dtype=np.float64))
    return dev


def _golden_tile(tl, k, fg_obj, bands, planes, img, rec, land, what):
    """Tile k of a rendered figure against what contourf was handed, the band of every cell and the bytes of the recorded colours."""
    field, lev, col, m = rec
    assert np.array_equal(planes[k], field, equal_nan=True), what
    assert tl["constant"] == m["constant"], what
    want = dict(tl)
    if not tl["constant"]:
        assert tl["levels"].tobytes() == lev.tobytes(), what
        assert np.array_equal(bands[k], ref.band_index(field, lev, tl["extend"])), what
        want["colours"] = col                                   # matplotlib's own face colours
    else:
        assert np.all(bands[k] == -1), what
    _, want_img = ref.render([field], [want], land)
    assert np.array_equal(ref.tile(img, k, 19, 36), ref.tile(want_img, 0, 19, 36)), what


@pytest.mark.parametrize("path", ref.GOLDENS, ids=ref.case_of)
def test_c_abi_vs_reference_goldens(gpu, path, monkeypatch):
    from qingdai_amd import figures as fgm
    from qingdai_amd._lib import QdError
    z = np.load(path)
    meta = ref.golden_meta(z)
    ref.set_env(monkeypatch, meta["env"])
    dev = _device((19, 36), z)
    assert np.array_equal(dev.grid.lat, z["lat"]) and np.array_equal(dev.grid.lon, z["lon"])
    land, t = z["land_mask"], meta["t_days"]
    fg = fgm.Figures(dev, population=meta["eco"], layers=z["layers"] if meta["eco"] else None, alpha=meta["eco"], banded=meta["eco"],
                     phyto_species=meta["SP"])
    # ---- ecology
    img = fg.ecology(t, want_stacks=True)
    n = 5 if meta["eco"] else 3
    bands, planes, tiles = fg.bands(), fg.planes(), fg.tiles
    assert img.shape == fgm.mosaic_shape(n, 19, 36) + (3,) and len(tiles) == n
    rec = ref.golden_tiles(z, meta, "ecology")
    assert sorted(rec) == [k for k, tl in enumerate(tiles) if not tl["unavailable"]]
    for k in rec:
        _golden_tile(tiles[k], k, fg, bands, planes, img, rec[k], land, (meta["case"], "ecology", k))
    for k, tl in enumerate(tiles):
        if tl["unavailable"]:                                    # white under the coast
            _, want_img = ref.render([None], [tl], land)
            assert np.array_equal(ref.tile(img, k, 19, 36), ref.tile(want_img, 0, 19, 36)) and np.all(bands[k] == -1) and np.isnan(planes[k]).all()
    gut = np.ones(img.shape[:2], dtype=bool)
    for k in range(n):
        y0, x0 = fgm.tile_origin(k, 19, 36)
        gut[y0:y0 + 19, x0:x0 + 36] = False
    assert np.all(img[gut] == 255)
    # the whole mosaic again from the device's own planes and table through the restatement; twice: identical bytes
    own_bands, own_img = ref.render(planes, tiles, land)
    assert np.array_equal(bands, own_bands) and np.array_equal(img, own_img)
    assert fg.ecology(t).tobytes() == img.tobytes()
    with pytest.raises(QdError, match="did not keep the stacks"):
        fg.bands()
    # ---- plankton
    rec = ref.golden_tiles(z, meta, "plankton")
    for s in ((0, 1) if meta["SP"] >= 2 else (0,)):
        img = fg.plankton(t, s, want_stacks=True)
        assert img.shape == (27, 44, 3)
        want_vmax = rec[s][3]["vmax"]
        print(f"{meta['case']}: species {s} vmax {fg.vmax!r} (the reference chose {want_vmax!r})")
        assert fg.vmax == want_vmax
        _golden_tile(fg.tiles[0], 0, fg, fg.bands(), fg.planes(), img, rec[s], land, (meta["case"], "plankton", s))
    # ---- ISR
    img = fg.isr(t, want_stacks=True)
    g, tiles, bands, planes = meta["figures"]["isr"], fg.tiles, fg.bands(), fg.planes()
    assert img.shape == fgm.mosaic_shape(2, 19, 36) + (3,)
    assert [tl["mark"][1] for tl in tiles] == [int(np.argmax(z["isr_A"])), int(np.argmax(z["isr_B"]))]
    if g["raised"]:
        assert tiles[0]["constant"] and tiles[1]["constant"] and np.all(bands == -1)
        assert np.array_equal(planes[0], z["isr_A"]) and np.array_equal(planes[1], z["isr_B"])
        assert fg.line.startswith("[Diagnostics] Day 12.25: Subsolar separation")
    else:
        assert meta["printed"] == [fg.line]
        rec = ref.golden_tiles(z, meta, "isr")
        for k in (0, 1):
            field, lev, col, m = rec[k]
            assert np.array_equal(planes[k], field, equal_nan=True) and tiles[k]["levels"].tobytes() == lev.tobytes()
            assert np.array_equal(bands[k], ref.band_index(field, lev, False))
            mk = [q for q in g["marks"] if q["tile"] == k][0]
            cell = tiles[k]["mark"][1]
            assert (float(z["lat"][cell // 36]), float(z["lon"][cell % 36])) == (mk["lat"], mk["lon"])
        want = [dict(tiles[k], colours=rec[k][2]) for k in (0, 1)]
        assert np.array_equal(img, ref.render(planes, want, land)[1])
        a = ref.tile(img, 0, 19, 36)
        r, c = divmod(tiles[0]["mark"][1], 36)
        assert a[r, c].tolist() == [0, 255, 255]                   # the cyan x
    dev.close()


def _plane_cases(shape, seed):
    r = np.random.default_rng(seed)
    n = shape[0] * shape[1]
    base = r.uniform(-3.0, 7.0, shape)
    cases = {"random": base.copy()}
    x = base.copy(); x.ravel()[r.choice(n, max(1, n // 5), replace=False)] = np.nan; cases["nans"] = x                # noqa: E702
    cases["equal"] = np.full(shape, 2.5)
    x = 1.0 + np.arange(n, dtype=np.float64).reshape(shape)[::-1, ::-1] % 7 * 2.0 ** -52; cases["low_bits"] = x      # noqa: E702
    x = np.round(base); x.ravel()[::3] = 0.0; x.ravel()[1::5] = -0.0; cases["signed_zeros"] = x                     # noqa: E702
    x = base.copy(); x.ravel()[[0, n // 2]] = np.inf; x.ravel()[n - 1] = -np.inf; x.ravel()[1] = np.nan; cases["inf"] = x   # noqa: E702
    cases["tiny"] = base * 1e-310                                 # subnormals: the keys differ only in the low digits
    x = base * 10.0 ** r.uniform(-200, 200, shape); cases["wide"] = x                                                # noqa: E702
    return cases


@pytest.mark.parametrize("shape", [(5, 4), (7, 65), (19, 36)], ids=["5x4", "7x65", "19x36"])
def test_scan_and_order_statistics_vs_numpy(gpu, shape, monkeypatch):
    """5 x 4: fewer cells than a wave, one workgroup; 7 x 65: two workgroups, the last one ragged (455 = 256 + 199); 19 x 36: three
    (684 = 2 x 256 + 172).  Every pass of the select is exercised by values that share their upper key bytes."""
    ref.set_env(monkeypatch, {})
    n = shape[0] * shape[1]
    land = np.zeros(shape, dtype=np.uint8)
    dev = _device(shape, {"land_mask": land})
    dev.tiles_configure()
    for name, x in _plane_cases(shape, 31 * shape[0] + shape[1]).items():
        dev.upload_now("ISR_A", x)
        dev.upload_now("ISR_B", x[::-1].copy())
        got = dev.tiles_scan([("ISR_A", 0), ("ISR_B", 0)])
        for g, plane in zip(got, (x, x[::-1])):
            want = ref.scan(plane)
            assert g["min"] == want["min"] and g["max"] == want["max"] and g["nan"] == want["nan"] and g["argmax"] == want["argmax"], (name, g, want)
            assert g["argmax_value"] == want["argmax_value"] or (np.isnan(g["argmax_value"]) and np.isnan(want["argmax_value"])), name
        v = np.sort(x.ravel())
        v = v[~np.isnan(v)]
        ranks = list(range(v.size)) if n <= 20 else sorted({0, v.size // 2, v.size - 2, v.size - 1, v.size // 3, int(0.99 * (v.size - 1))})
        for k in range(0, len(ranks), 4):
            count, vals = dev.tiles_order_stats("ISR_A", 0, ranks[k:k + 4])
            assert count == v.size, name
            assert np.array_equal(vals, v[ranks[k:k + 4]]), (name, ranks[k:k + 4], vals, v[ranks[k:k + 4]])
        # two ranks at once in both orders, a repeated rank, a rank that is not below the count
        a, b = 0, v.size - 1
        assert np.array_equal(dev.tiles_order_stats("ISR_A", 0, [a, b])[1], v[[a, b]]), name
        assert np.array_equal(dev.tiles_order_stats("ISR_A", 0, [b, a])[1], v[[b, a]]), name
        count, vals = dev.tiles_order_stats("ISR_A", 0, [b, b, v.size, a])
        assert count == v.size and np.array_equal(vals[[0, 1, 3]], v[[b, b, a]]) and np.isnan(vals[2]), name
        count, vals = dev.tiles_order_stats("ISR_A", 0, [])
        assert count == v.size and vals.size == 0
    # n = 1, n = 2 and an empty plane
    for keep in (1, 2, 0):
        x = np.full(shape, np.nan)
        x.ravel()[[n - 1, 3][:keep]] = [4.0, -1.5][:keep]
        dev.upload_now("ISR_A", x)
        count, vals = dev.tiles_order_stats("ISR_A", 0, [0, 1])
        assert count == keep
        want = np.sort(x.ravel())[:keep]
        assert np.array_equal(vals[:keep], want[:2]) and np.isnan(vals[keep:]).all()
        s = dev.tiles_scan([("ISR_A", 0)])[0]
        assert s["nan"] and s["argmax"] == int(np.argmax(x)) and np.isnan(s["argmax_value"])
        assert (s["min"], s["max"]) == ((np.inf, -np.inf) if keep == 0 else (float(np.nanmin(x)), float(np.nanmax(x))))
    # np.argmax's tie rule across workgroups
    x = np.full(shape, 10.0)
    x.ravel()[[n - 1, n // 2, n // 2 + 1]] = 50.0
    dev.upload_now("ISR_A", x)
    assert dev.tiles_scan([("ISR_A", 0)])[0]["argmax"] == n // 2 == int(np.argmax(x))
    dev.close()


def test_percentile_of_the_plankton_plane_is_numpys(gpu, monkeypatch):
    """The device's two order statistics through the host's linear rule against np.nanpercentile of the masked plane, on the ragged
    shape, with duplicates (the zeros the advection clips to), an inf and NaNs on ocean cells."""
    from qingdai_amd import figures as fgm
    ref.set_env(monkeypatch, {})
    r = np.random.default_rng(7)
    shape = (7, 65)
    land = (r.uniform(size=shape) < 0.4).astype(np.uint8)
    C = r.uniform(0.0, 1.2, (2,) + shape) ** 4
    C[0][r.uniform(size=shape) < 0.3] = 0.0
    C[1, 2, 3], C[1, 4, 64] = np.inf, np.nan
    dev = _device(shape, {"land_mask": land, "C": C})
    fg = fgm.Figures(dev, population=False, phyto_species=2)
    for s in (0, 1):
        fg.plankton(1.0, s, want_stacks=True)
        f = C[s].copy()
        f[land == 1] = np.nan
        want = float(np.nanpercentile(f, 99.0))
        print(f"species {s}: vmax {fg.vmax!r}, np.nanpercentile {want!r}")
        assert fg.vmax == want and np.array_equal(fg.planes()[0], f, equal_nan=True)
    dev.close()


def _eco_env(tmp_path, extra=None):
    env = {"QD_N_LAT": "19", "QD_N_LON": "36", "QD_DT_SECONDS": "300", "QD_DYN_DIAG_PRINT": "0", "QD_AUTOSAVE_LOAD": "0", "QD_HYDRO_ENABLE": "0",
           "QD_ECO_ENABLE": "1", "QD_ECO_DAILY": "1", "QD_ECO_NS": "3", "QD_ECO_COHORT_K": "2", "QD_ECO_DIAG": "0",
           "QD_PHYTO_ENABLE": "1", "QD_PHYTO_DAILY": "1", "QD_PHYTO_NSPECIES": "2", "QD_PHYTO_DIAG": "0", "QD_DATA_DIR": str(tmp_path / "data")}
    env.update(extra or {})
    return env


def test_resident_stack_vs_host_stack_and_no_side_effects(gpu, tmp_path, monkeypatch):
    """After qd_eco_daily_configure and one daily step the canopy-height and density planes from the resident stack equal those from
    the downloaded stack handed in as a host stack, and both equal the restatement; rendering every figure between two spans leaves
    every downloaded field, the tracers, the step counters, the eco state and the lane logs as they were."""
    from qingdai_amd import driver, _lib
    from qingdai_amd import figures as fgm
    monkeypatch.chdir(tmp_path)
    ref.set_env(monkeypatch, _eco_env(tmp_path, {"QD_ECO_HEIGHT_SCALE_M": "12.5"}))
    sim = driver.Simulation(n_lat=19, n_lon=36, use_ocean=True, quiet=True)
    sim.bootstrap_ecology()
    sim.run_steps(3)
    pop = sim.eco.pop
    assert pop.daily is not None and (pop.Ns, pop.K) == (3, 2)
    pop.step_daily(0.6)

    def state():
        out = {}
        for name in _lib.FIELDS:                                 # a passive probe: a cached download would be sent back by the next flush,
            sim.dev._host.pop(name, None)                        # and qd_upload marks ELEVATION, CLOUD_EFF and the alpha maps as given
            out[name] = sim.dev.get(name).copy()
            sim.dev._host.pop(name, None)
        out["tracers"] = sim.dev.phyto_download()
        out["counters"] = np.array(sim.dev.counters())
        out["layers"] = sim.dev.eco_daily_get_layers(3, 2)
        out["eco_state"] = np.array([float(v) for v in pop.state().values()])
        out["firings"] = np.array([sim.dev.eco_daily_firings(), sim.dev.indiv_daily_firings()])
        return out
    before = state()
    fg = fgm.Figures(sim)
    img = fg.ecology(0.5, want_stacks=True)
    tiles, planes = fg.tiles, fg.planes()
    assert len(tiles) == 5 and not tiles[3]["unavailable"] and img.shape == fgm.mosaic_shape(5, 19, 36) + (3,)
    fg.plankton(0.5, 0), fg.plankton(0.5, 1), fg.isr(0.5)
    after = state()
    for k in before:
        assert np.array_equal(before[k], after[k], equal_nan=True), k
    inp = {"land_mask": sim.land_mask, "layers": after["layers"], "lai": after["ECO_LAI"], "alpha": after["ECO_ALPHA"], "banded": after["ECO_ALPHA_BANDED"]}
    assert np.array_equal(planes[3], ref.plane("CANOPY_HEIGHT", 0, inp, 12.5)) and planes[3].max() > 0
    assert np.array_equal(planes[4], ref.plane("SPECIES_DENSITY", 0, inp)) and planes[4].max() > 0
    assert np.array_equal(planes[0], ref.plane("LAI", 0, inp))
    host = fgm.Figures(sim.dev, population=True, layers=after["layers"], alpha=not tiles[1]["unavailable"], banded=False)
    host.ecology(0.5, want_stacks=True)
    hp = host.planes()
    assert np.array_equal(hp[3], planes[3]) and np.array_equal(hp[4], planes[4]) and np.array_equal(hp[0], planes[0])
    assert host.tiles[2]["unavailable"] and np.isnan(hp[2]).all()
    # a span after the renders runs as if they had not happened
    sim.run_steps(2)
    twin = driver.Simulation(n_lat=19, n_lon=36, use_ocean=True, quiet=True)
    twin.bootstrap_ecology()
    twin.run_steps(3)
    twin.eco.pop.step_daily(0.6)
    twin.run_steps(2)
    for name in ("TS", "U", "H", "ECO_LAI", "ECO_ALPHA", "ECO_ALPHA_BANDED", "SST", "PRECIP"):
        sim.dev._host.pop(name, None), twin.dev._host.pop(name, None)
        assert np.array_equal(sim.dev.get(name).copy(), twin.dev.get(name).copy(), equal_nan=True), name
        sim.dev._host.pop(name, None), twin.dev._host.pop(name, None)
    sim.dev.close(), twin.dev.close()


def test_driver_main_writes_the_figures(gpu, tmp_path, monkeypatch, capsys):
    """Interval 3 steps, 5 steps from t = 2900 s: firings at the steps 0 and 3, named 000.0 and 000.1 (tests/test_gpu_stateframe.py)."""
    from qingdai_amd import driver
    from qingdai_amd.imgio import read_png
    import qingdai_amd.imgio as imgio
    monkeypatch.chdir(tmp_path)
    common = {"QD_SIM_DAYS": "0.02", "QD_PLOT_EVERY_DAYS": "0.0105", "QD_ORBIT_EPOCH_SECONDS": "2900", "QD_STATE_PLOT": "1", "QD_TRUECOLOR": "1",
              "QD_PLOT_ISR": "1", "QD_ECO_DIAG": "1", "QD_LOAD_PLANKTON": "0"}
    finals = {}
    real_sim = driver.Simulation

    def keep(*a, **k):
        finals["sim"] = real_sim(*a, **k)
        return finals["sim"]
    monkeypatch.setattr(driver, "Simulation", keep)

    def fields_of(sim):
        out = {}
        for name in ("TS", "U", "V", "H", "Q", "SST", "ECO_LAI", "ECO_ALPHA", "ECO_ALPHA_BANDED", "ALBEDO", "PRECIP", "ECO_EDAY"):
            sim.dev._host.pop(name, None)
            out[name] = sim.dev.get(name).copy()
            sim.dev._host.pop(name, None)
        out["tracers"] = sim.dev.phyto_download()
        return out
    ref.set_env(monkeypatch, _eco_env(tmp_path, dict(common, QD_FIGURES="0", QD_OUTPUT_DIR=str(tmp_path / "out0"), QD_DATA_DIR=str(tmp_path / "d0"))))
    assert driver.main() == 0
    off, end_off = capsys.readouterr().out, fields_of(finals["sim"])
    assert "figures are not." in off and not os.path.exists(tmp_path / "out0" / "plankton")
    order = []
    real_write = imgio.write_png
    monkeypatch.setattr(imgio, "write_png", lambda path, img: (order.append(os.path.relpath(path, tmp_path / "out1")), real_write(path, img))[1])
    ref.set_env(monkeypatch, _eco_env(tmp_path, dict(common, QD_FIGURES="1", QD_OUTPUT_DIR=str(tmp_path / "out1"), QD_DATA_DIR=str(tmp_path / "d1"))))
    assert driver.main() == 0
    on, end_on = capsys.readouterr().out, fields_of(finals["sim"])
    monkeypatch.setattr(imgio, "write_png", real_write)
    per_firing = ["state_day_{}.png", "true_color_day_{}.png", os.path.join("plankton", "species0_day_{}.png"),
                  os.path.join("plankton", "species1_day_{}.png"), "ecology_day_{}.png", "isr_components_day_{}.png"]
    assert order == [p.format(d) for d in ("000.0", "000.1") for p in per_firing]
    for d in ("000.0", "000.1"):
        for p, n in zip(per_firing[2:], (1, 1, 5, 2)):
            path = str(tmp_path / "out1" / p.format(d))
            assert read_png(path).shape == (27, n * 36 + 4 * (n + 1), 3), p
            side = json.load(open(path[:-4] + ".json", encoding="utf-8"))
            assert len(side["tiles"]) == n and side["suptitle"] is None and side["layout"]["tile"] == [19, 36]
    eco = json.load(open(tmp_path / "out1" / "ecology_day_000.1.json", encoding="utf-8"))
    assert [t["cmap"] for t in eco["tiles"]] == ["YlGn", "cividis", "cividis", "Greens", "viridis"] and not eco["tiles"][0]["unavailable"]
    assert not eco["tiles"][2]["unavailable"]                      # the banded map: computed by the run or by the panel's fallback
    # the lines: those of the run without the switch, apart from [Plots], steps/s and the new lines
    new = [ln for ln in on.splitlines() if ln.startswith("[Diagnostics] Day") or ln.startswith("[Ecology] Panel fallback")]
    assert len([ln for ln in new if ln.startswith("[Diagnostics]")]) == 2 and "skipped" not in on
    strip = lambda s: [ln for ln in s.splitlines() if not ln.startswith("[Plots]") and "steps/s" not in ln and ln not in new]      # noqa: E731
    assert strip(on) == strip(off)
    plots = [ln for ln in on.splitlines() if ln.startswith("[Plots]")][0]
    assert "plankton, ecology, ISR figures" in plots and "figures are not" not in plots and "every 3 steps" in plots
    for k in end_off:
        assert np.array_equal(end_off[k], end_on[k], equal_nan=True), k


def test_a_failed_write_does_not_stop_the_run(gpu, tmp_path, monkeypatch, capsys):
    from qingdai_amd import driver
    monkeypatch.chdir(tmp_path)
    (tmp_path / "blocked").write_text("a file where the output directory should be")
    ref.set_env(monkeypatch, _eco_env(tmp_path, {"QD_SIM_DAYS": "0.02", "QD_PLOT_EVERY_DAYS": "0.0105", "QD_FIGURES": "1", "QD_PLOT_ISR": "1",
                                                 "QD_ECO_DIAG": "1", "QD_PHYTO_DIAG": "1", "QD_LOAD_PLANKTON": "0",
                                                 "QD_OUTPUT_DIR": str(tmp_path / "blocked")}))
    assert driver.main() == 0
    out = capsys.readouterr().out
    assert out.count("[PlanktonViz] skipped: ") == 1 and out.count("[EcologyViz] skipped: ") == 1 and out.count("[ISRViz] figure skipped: ") == 1
    assert out.count("[Diagnostics] Day") == 2 and "--- Simulation Finished ---" in out


def test_refusals(gpu, monkeypatch):
    import qingdai_amd as qa
    from qingdai_amd import _lib
    from qingdai_amd import figures as fgm
    from qingdai_amd._lib import QdError
    from qingdai_amd.device import Device
    ref.set_env(monkeypatch, {})
    dev = Device(qa.SphericalGrid(19, 36))
    white = _lib.qd_tile_desc(source=_lib.TILE["ISR_A"], constant=1, mark_cell=-1)
    with pytest.raises(QdError, match="qd_tiles_configure has not been called"):
        dev.tiles_scan([("ISR_A", 0)])
    with pytest.raises(QdError, match="qd_tiles_configure has not been called"):
        dev.tiles_render([white])
    with pytest.raises(QdError, match="qd_tiles_configure has not been called"):
        dev.tiles_order_stats("ISR_A", 0, [0])
    with pytest.raises(QdError, match="no figure on this handle"):
        dev.tiles_image()
    dev.tiles_configure()
    with pytest.raises(QdError, match=r"1\.\.QD_TILES_MAX"):
        dev.tiles_render([white] * 9)
    with pytest.raises(QdError, match=r"1\.\.QD_TILES_MAX"):
        dev.tiles_scan([("ISR_A", 0)] * 9)
    with pytest.raises(QdError, match="at most QD_TILES_MAX_RANKS"):
        dev.tiles_order_stats("ISR_A", 0, [0, 1, 2, 3, 4])
    with pytest.raises(QdError, match="a rank is negative"):
        dev.tiles_order_stats("ISR_A", 0, [-1])
    assert dev.lib.qd_tiles_render(dev.h, ctypes.byref(white), ctypes.sizeof(white) - 8, 1, 0) != 0
    assert b"struct size mismatch" in dev.lib.qd_last_error(dev.h)
    many = _lib.qd_tile_desc(source=_lib.TILE["ISR_A"], n_levels=33, mark_cell=-1)
    with pytest.raises(QdError, match="more than QD_STATEFRAME_MAX_LEVELS"):
        dev.tiles_render([many])
    many.n_levels = 1
    with pytest.raises(QdError, match="at least 2 levels"):
        dev.tiles_render([many])
    for src in ("CANOPY_HEIGHT", "SPECIES_DENSITY"):
        with pytest.raises(QdError, match="there is neither"):
            dev.tiles_render([_lib.qd_tile_desc(source=_lib.TILE[src], constant=1, mark_cell=-1)])
        with pytest.raises(QdError, match="there is neither"):
            dev.tiles_order_stats(src, 0, [0])
    with pytest.raises(QdError, match="no tracers on this handle"):
        dev.tiles_scan([("PLANKTON", 0)])
    with pytest.raises(QdError, match="no host plane on this handle"):
        dev.tiles_scan([("HOST_PLANE", 0)])
    with pytest.raises(QdError, match="unknown tile source"):
        dev.tiles_scan([(9, 0)])
    dev.phyto_configure(2, 0.0, 0.7)
    dev.tiles_configure(10.0, np.zeros((3, 2, 19, 36)))
    for src, idx in (("PLANKTON", 2), ("PLANKTON", -1), ("SPECIES_DENSITY", 3), ("SPECIES_DENSITY", -1)):
        with pytest.raises(QdError, match="species index out of range"):
            dev.tiles_render([_lib.qd_tile_desc(source=_lib.TILE[src], index=idx, constant=1, mark_cell=-1)])
        with pytest.raises(QdError, match="species index out of range"):
            dev.tiles_scan([(src, idx)])
    with pytest.raises(ValueError, match="layers must be"):
        dev.tiles_configure(10.0, np.zeros((3, 2, 19, 35)))
    with pytest.raises(QdError, match="n_layers out of range"):
        dev.tiles_configure(10.0, np.zeros((1, 9, 19, 36)))
    dev.tiles_render([white])
    assert np.all(dev.tiles_image() == 255)                      # no land: no coast
    buf = np.zeros(5, dtype=np.uint8)
    with pytest.raises(QdError, match="size mismatch"):
        dev._chk(dev.lib.qd_tiles_download(dev.h, 0, buf.ctypes.data, 5), "qd_tiles_download")
    with pytest.raises(QdError, match="which must be 0"):
        dev._chk(dev.lib.qd_tiles_download(dev.h, 3, buf.ctypes.data, 5), "qd_tiles_download")
    with pytest.raises(QdError, match="did not keep the stacks"):
        dev.tiles_planes()
    with pytest.raises(ValueError, match="at most 8"):
        fgm.pack_tiles([fgm.plankton_tile(0.0, 0, 1.0)] * 9)
    dev.close()
    band = Device(qa.SphericalGrid(73, 144), row0=20, n_rows=30, halo=6)
    assert band.lib.qd_tiles_configure(band.h, 10.0, None, 0, 0) != 0 and b"latitude bands are not supported" in band.lib.qd_last_error(band.h)
    refs = (_lib.qd_tile_ref * 1)()
    out, cells, cnt = (ctypes.c_double * 4)(), (ctypes.c_int64 * 1)(), ctypes.c_int64(0)
    assert band.lib.qd_tiles_scan(band.h, refs, 1, out, cells) != 0 and b"latitude bands are not supported" in band.lib.qd_last_error(band.h)
    assert band.lib.qd_tiles_order_stats(band.h, 6, 0, cells, 1, out, ctypes.byref(cnt)) != 0
    assert b"latitude bands are not supported" in band.lib.qd_last_error(band.h)
    assert band.lib.qd_tiles_render(band.h, ctypes.byref(white), ctypes.sizeof(white), 1, 0) != 0
    assert b"latitude bands are not supported" in band.lib.qd_last_error(band.h)
    with pytest.raises(QdError, match="latitude bands are not supported"):
        fgm.Figures(band, population=False).configure()
    band.close()
