"""CPU: the host side of the state frame (qingdai_amd/stateframe.py) and its NumPy restatement (tests/stateframe_ref.py) against
what matplotlib recorded while the reference's plot_state ran (tests/golden/stateframe_*.npz, scripts/gen_golden_stateframe.py):
the auto levels bit for bit, the band colours to 1e-12, the fifteen handed-in arrays exactly (the vorticity to the operator
tolerance), the levels of every panel, the band rule, the mosaic geometry, the sidecar, the plot clock and the driver's order."""
import glob
import io
import json
import os
from contextlib import redirect_stdout

import numpy as np
import pytest

import stateframe_ref as ref

HERE = os.path.dirname(os.path.abspath(__file__))
GOLDENS = sorted(glob.glob(os.path.join(HERE, "golden", "stateframe_*_19x36.npz")))


def _case(path):
    return os.path.basename(path)[len("stateframe_"):-len("_19x36.npz")]


def _table(z, monkeypatch):
    """-> (meta, the restatement's field stack, its scan, the table the product builds from that scan)."""
    from qingdai_amd import stateframe as sf
    meta = ref.golden_meta(z)
    ref.set_env(monkeypatch, meta["env"])
    e = sf.read_env()
    F = ref.fields(z, z["lat"], ps_abs=e["ps_abs"], ocean=meta["ocean"], p0=meta["p0"], rho_a=meta["rho_a"], H=meta["H"])
    scan = ref.scan(F, z["isr_A"], z["isr_B"])
    return meta, F, scan, sf.build_table(scan, e, ocean=meta["ocean"])


def test_the_six_cases_exist():
    assert sorted(_case(p) for p in GOLDENS) == ["constant", "default", "nonfinite", "noocean", "ps_abs", "rivers"]


def test_auto_levels_are_matplotlibs_bit_for_bit():
    from qingdai_amd.stateframe import auto_levels
    z = np.load(os.path.join(HERE, "golden", "stateframe_levels.npz"))
    assert len(z["zmin"]) >= 300
    for a, b, n, want in zip(z["zmin"], z["zmax"], z["count"], z["levels"]):
        got = auto_levels(float(a), float(b), 20)
        assert got.dtype == np.float64 and got.tobytes() == want[:n].tobytes(), (a, b, got, want[:n])


def test_the_default_step_table():
    """The part that is easy to get wrong: one entry below (0.1 x all but the last) and one above (10 x the second)."""
    from qingdai_amd import stateframe as sf
    assert sf._EXT_STEPS.tolist() == [0.1, 0.15000000000000002, 0.2, 0.25, 0.30000000000000004, 0.4, 0.5, 0.6000000000000001, 0.8,
                                      1.0, 1.5, 2.0, 2.5, 3.0, 4.0, 5.0, 6.0, 8.0, 10.0, 15.0]
    assert sf.auto_levels(0.0, 1.0).tolist() == [0.0] + [k * 0.05 for k in range(1, 21)]


@pytest.mark.parametrize("path", GOLDENS, ids=_case)
def test_fields_levels_and_colours_vs_matplotlib(path, monkeypatch):
    from qingdai_amd import stateframe as sf
    z = np.load(path)
    meta, F, scan, tab = _table(z, monkeypatch)
    names = sf.panels(sf.read_env()["ps_abs"], meta["ocean"])
    for k in range(15):
        want = z["fields"][k]
        if k == 8:
            ok = np.isfinite(want)
            assert np.array_equal(ok, np.isfinite(F[k]))
            assert np.max(np.abs(F[k][ok] - want[ok])) <= ref.VORT_TOL * np.max(np.abs(want[ok]))
        else:
            assert np.array_equal(F[k], want, equal_nan=True), k
        p = tab["panels"][k]
        assert names[k][2] == meta["cmaps"][k], k                # the colormap the reference names
        assert p["extend"] == (meta["extend"][k] == "max")
        assert p["constant"] == meta["constant"][k], k
        lev = z[f"levels_{k}"]
        if len(lev) == 0:                                       # the panels 7 and 8 with an ocean: streamplot, no contourf
            assert k in (6, 7) and p["levels"] is not None and not p["constant"]
            continue
        if p["constant"]:
            assert p["levels"] is None and meta["n_arg"][k] == 20
            continue
        if k == 8:                                              # linspace(-vmax, vmax, 21) of a vmax that agrees to the tolerance
            assert len(p["levels"]) == len(lev) == 21 and np.allclose(p["levels"], lev, rtol=0, atol=ref.VORT_TOL * lev[-1] * 2)
            mid_colours = sf.band_colours("PuOr", lev)
        else:
            assert p["levels"].tobytes() == lev.tobytes(), (k, p["levels"], lev)
            mid_colours = p["colours"]
        assert mid_colours.shape == z[f"colours_{k}"].shape == (len(lev) - 1 + int(p["extend"]), 3)
        assert np.max(np.abs(mid_colours - z[f"colours_{k}"])) <= 1e-12, k
    # the shared temperature levels: np.linspace between the extremes of the three fields
    three = np.stack([z["fields"][0], z["fields"][1], z["fields"][3]])
    assert tab["panels"][0]["levels"][0] == np.nanmin(three) and tab["panels"][0]["levels"][-1] == np.nanmax(three)
    for k in (1, 3):
        assert np.array_equal(tab["panels"][k]["levels"], tab["panels"][0]["levels"])
    assert tab["marks"] == [int(np.argmax(z["isr_A"])), int(np.argmax(z["isr_B"]))]


@pytest.mark.parametrize("path", GOLDENS, ids=_case)
def test_band_rule_on_the_golden_arrays(path):
    z = np.load(path)
    meta = ref.golden_meta(z)
    for k in range(15):
        lev, fld = z[f"levels_{k}"], z["fields"][k]
        if len(lev) < 2 or meta["constant"][k]:
            continue
        ext = meta["extend"][k] == "max"
        b = ref.band_index(fld, lev, ext)
        fin = np.isfinite(fld)
        assert np.all(b[~fin] == -1)
        inside = fin & (fld >= lev[0]) & (fld <= lev[-1])
        assert np.all(b[inside] >= 0) and np.all(b[inside] <= len(lev) - 2)
        i = b[inside].astype(int)
        assert np.all(lev[i] <= fld[inside]) and np.all((fld[inside] < lev[i + 1]) | ((i == len(lev) - 2) & (fld[inside] == lev[-1])))
        assert np.all(b[fin & (fld < lev[0])] == -1)
        assert np.all(b[fin & (fld > lev[-1])] == (len(lev) - 1 if ext else -1))
        if meta["n_arg"][k] == 0 and k in (0, 1, 3):            # the extremes sit on the end levels: first band and closed top band
            assert b[fld == lev[-1]].tolist() == [len(lev) - 2] * int((fld == lev[-1]).sum())
    if meta["case"] == "constant":
        cloud = ref.band_index(z["fields"][5], z["levels_5"])
        assert cloud[3, 3:9].tolist() == [-1] * 6 and cloud[4, 3:9].tolist() == [-1] * 6 and cloud[5, 3:9].tolist() == [9] * 6
    if meta["case"] == "default":
        rain = ref.band_index(z["fields"][4], z["levels_4"], True)
        assert (rain == 10).sum() > 0 and np.all(z["fields"][4][rain == 10] > 30.0) and (rain == 0).sum() > 100      # z = 0 sits on level 0
        alb = ref.band_index(z["fields"][10], z["levels_10"])
        assert alb[2, 3:6].tolist() == [-1, -1, -1]
    if meta["case"] == "nonfinite":
        assert ref.band_index(z["fields"][13], z["levels_13"])[5, 15] == -1 and np.isinf(z["fields"][13][5, 15])
        assert np.isnan(z["fields"][8]).sum() == 2                # the cells north and south of the NaN in u


@pytest.mark.parametrize("path", GOLDENS, ids=_case)
def test_mosaic_geometry_and_overlays(path, monkeypatch):
    from qingdai_amd import stateframe as sf
    z = np.load(path)
    meta, F, scan, tab = _table(z, monkeypatch)
    routed = meta["routing"]
    bands, img = ref.render(F, tab, z["land_mask"], flow=z["flow"] if routed else None, lake=z["lake_mask"] if routed else None)
    assert img.shape == sf.mosaic_shape(19, 36) + (3,) == (5 * 19 + 24, 3 * 36 + 16, 3) and img.dtype == np.uint8
    gut = np.ones(img.shape[:2], dtype=bool)
    for k in range(15):
        y0, x0 = sf.tile_origin(k, 19, 36)
        assert (y0, x0) == (4 + (k // 3) * 23, 4 + (k % 3) * 40)
        gut[y0:y0 + 19, x0:x0 + 36] = False
    assert gut.sum() == img.shape[0] * img.shape[1] - 15 * 19 * 36 and np.all(img[gut] == 255)
    cst = ref.coast(z["land_mask"])
    assert cst.any() and np.all(z["land_mask"][cst] == 1)
    assert np.all(ref.tile(img, 2, 19, 36)[cst] == 0) and np.all(ref.tile(img, 11, 19, 36)[cst] == 255)      # black; white on the OLR panel
    # panel 10: no coast, the two marks; northernmost row on top
    t10 = ref.tile(img, 9, 19, 36)
    ra, ca = divmod(tab["marks"][0], 36)
    rb, cb = divmod(tab["marks"][1], 36)
    if (ra, ca) != (rb, cb):
        assert t10[ra, ca].tolist() == [0, 255, 255]
    assert t10[rb, cb].tolist() == [255, 255, 0]
    y0, x0 = sf.tile_origin(9, 19, 36)
    assert img[y0 + 18 - rb, x0 + cb].tolist() == [255, 255, 0]
    if meta["case"] == "constant":
        for k in (13, 14):
            t = ref.tile(img, k, 19, 36)
            assert np.all(bands[k] == -1) and np.all(t[~cst] == 255) and np.all(t[cst] == 0)
    if routed:
        plain = ref.render(F, tab, z["land_mask"])[1]
        river = (z["flow"] >= 1e6) & (z["land_mask"] == 1)
        assert river[3:8, 4:8].all() and not river[3:8, 8:12].any() and not river[10, 30] and z["lake_mask"][9, 31] == 1
        changed = np.any(img != plain, axis=-1)
        for k in range(15):
            d = ref.tile(changed, k, 19, 36)
            if k in (0, 7):
                assert d[river & ~cst].all() and d[9, 31] and not d[(~river) & (z["lake_mask"] == 0)].any()
            else:
                assert not d.any()


def test_sidecar_and_frame_name(monkeypatch):
    from qingdai_amd import stateframe as sf
    z = np.load([p for p in GOLDENS if _case(p) == "noocean"][0])
    meta, F, scan, tab = _table(z, monkeypatch)
    assert sf.frame_name(12.25) == "state_day_012.2.png" and sf.frame_name(0.0) == "state_day_000.0.png"
    s = json.loads(json.dumps(sf.sidecar(tab, 12.25, z["lat"], z["lon"]), ensure_ascii=False))
    assert s["t_days"] == 12.25 and len(s["panels"]) == 15 and s["layout"] == {"rows": 5, "cols": 3, "gutter": 4, "tile": [19, 36]}
    assert [p["title"] for p in s["panels"]][:3] == ["Surface Temperature (°C)", "Atmospheric Temperature (°C)", "Sea-level Pressure Anomaly (hPa, diag)"]
    assert s["panels"][7]["title"] == "Geopotential Height Anomaly (m)" and s["panels"][7]["cmap"] == "RdBu_r" and s["panels"][7]["unit"] == "m"
    assert s["panels"][4]["extend"] == "max" and s["panels"][4]["levels"] == np.linspace(0, 30, 11).tolist()
    assert s["panels"][9]["unit"] == "W/m²" and not any(p["constant"] for p in s["panels"])
    ra, ca = divmod(tab["marks"][0], 36)
    assert s["stars"]["A"] == {"lat": float(z["lat"][ra]), "lon": float(z["lon"][ca])}
    monkeypatch.setenv("QD_PLOT_PS_MODE", "ABS")
    assert sf.build_table(scan, None, ocean=True)["panels"][2]["title"] == "Sea-level Pressure (hPa, diag)"
    assert sf.build_table(scan, None, ocean=True)["panels"][7]["title"] == "Ocean Currents (m/s)"


def test_read_env_and_pack_table(monkeypatch):
    from qingdai_amd import stateframe as sf, _lib
    ref.set_env(monkeypatch, {})
    e = sf.read_env()
    assert (e["ps_abs"], e["rivers"], e["river_min"], e["river_alpha"], e["lake_alpha"]) == (False, True, 1e6, 0.35, 0.40)
    monkeypatch.setenv("QD_RIVER_ALPHA", "not a number")
    assert sf.read_env()["rivers"] is False and sf.read_env()["overlay_ok"] is False
    import ctypes
    assert ctypes.sizeof(_lib.qd_stateframe_params) == 64 and ctypes.sizeof(_lib.qd_stateframe_panel) == 16 + 32 * 8 + 32 * 24
    assert ctypes.sizeof(_lib.qd_stateframe_table) == 15 * 1040 + 16
    scan = {"t_min": np.array([1.0, 2.0, np.nan]), "t_max": np.array([5.0, 9.0, np.nan]), "vmax": float("nan"), "marks": [3, -1],
            "auto": {p: (float("inf"), float("-inf")) for p in sf.AUTO_PANELS}}
    tab = sf.build_table(scan, e)
    assert tab["panels"][0]["levels"].tolist() == np.linspace(1.0, 9.0, 20).tolist()
    assert [p["constant"] for p in tab["panels"]] == [k + 1 in sf.AUTO_PANELS for k in range(15)]
    t = sf.pack_table(tab)
    assert t.panel[0].n_levels == 20 and t.panel[2].n_levels == 0 and t.panel[2].constant == 1 and t.panel[4].extend_max == 1
    assert (t.panel[9].coast, t.panel[11].coast, t.panel[0].coast) == (0, 2, 1) and list(t.mark_cell) == [3, -1]
    assert t.panel[4].rgb[10][:] == list(sf.cmap_table("Blues")[-1])
    tab["panels"][0]["levels"] = np.linspace(0.0, 1.0, 33)
    tab["panels"][0]["colours"] = sf.band_colours("coolwarm", tab["panels"][0]["levels"])
    with pytest.raises(ValueError, match="at most 32"):
        sf.pack_table(tab)


def test_plot_clock_and_driver_order(monkeypatch):
    """The state frame fires on the true-colour frame's clock and is written first (run_simulation.py:2426-2429), behind the
    diversity diagnostics and before the figures (:2404-2490): the calls recorded through the driver's own loop."""
    from qingdai_amd import driver
    from qingdai_amd.truecolor import firing_steps, plot_interval_steps
    assert plot_interval_steps({"QD_PLOT_EVERY_DAYS": "0.085"}, 2400) == 3 and firing_steps(4, 6, 3) == [2, 5]
    calls = []

    class Stub:
        def write_frame(self, t_days, output_dir=None):
            calls.append(("frame", self.name, round(t_days, 6)))
            return "path", "[TrueColor] line"

    sim = driver.Simulation.__new__(driver.Simulation)
    sim.dt, sim.day_seconds = 2400, 86400.0
    sim.t = 0.0
    sim.stateframe, sim.truecolor = Stub(), Stub()
    sim.stateframe.name, sim.truecolor.name = "state", "truecolor"
    sim.plot_every = 3
    assert sim.plot_due(0, 7) == (1, 0.0)
    assert [(k, day, run.__name__) for k, day, run in sim.outputs_due(1, 7)] == [(3, 2 * 2400 / 86400, "run_stateframe"), (3, 2 * 2400 / 86400, "run_truecolor")]
    monkeypatch.setattr(driver.Simulation, "run_steps", lambda self, n: (calls.append(("steps", n)), self._span_times(n)) and None)
    with redirect_stdout(io.StringIO()):
        sim.run_loop(5)
    assert calls == [("steps", 1), ("frame", "state", 0.0), ("frame", "truecolor", 0.0), ("steps", 3), ("frame", "state", round(3 * 2400 / 86400, 6)),
                     ("frame", "truecolor", round(3 * 2400 / 86400, 6)), ("steps", 1)]
    # every cadence on one step: diversity, the state frame, the true-colour frame, the figures
    monkeypatch.setattr(driver.Simulation, "run_diversity", lambda self, t_days: calls.append(("diversity", round(t_days, 6))) or
                        setattr(self, "diversity_next_day", t_days + self.diversity_every))
    monkeypatch.setattr(driver.Simulation, "run_figures", lambda self, t_days: calls.append(("figures", round(t_days, 6))))
    sim.t = 0.0
    sim.figures, sim.diversity_on, sim.diversity_every = object(), True, 6 * 2400 / 86400
    del calls[:]
    with redirect_stdout(io.StringIO()):
        sim.run_loop(7)
    both = [("diversity", 0.0), ("frame", "state", 0.0), ("frame", "truecolor", 0.0), ("figures", 0.0)]
    d3, d6 = round(3 * 2400 / 86400, 6), round(6 * 2400 / 86400, 6)
    assert calls == [("steps", 1)] + both + [("steps", 3)] + [c[:-1] + (d3,) for c in both[1:]] + [("steps", 3)] + [c[:-1] + (d6,) for c in both]
    sim.stateframe = None
    assert [run for _, _, run in sim.outputs_due(0, 7)] == [sim.run_diversity, sim.run_truecolor, sim.run_figures]
    sim.truecolor = sim.figures = None                          # the clock may stand; with no output on it nothing is due
    sim.diversity_on = False
    assert sim.outputs_due(0, 7) == []


def test_plots_line_with_the_switch_off_is_todays(monkeypatch):
    from qingdai_amd import driver
    sim = driver.Simulation.__new__(driver.Simulation)
    sim.dt = 300
    ref.set_env(monkeypatch, {})
    assert sim.enable_stateframe() is None and sim.stateframe is None
    assert driver.plots_line(None, None, sim) == "[Plots] matplotlib panels are not produced by the device driver (out of the hot path)."
    sim.plot_every = 288
    assert driver.plots_line(None, object(), sim) == ("[Plots] only the true-colour frame is produced by the device driver, every 288 steps; "
                                                     "the matplotlib panels are not.")
    on = driver.plots_line(object(), object(), sim)
    assert "15-panel state frame" in on and "true-colour frame" in on and "every 288 steps" in on
    assert "true-colour" not in driver.plots_line(object(), None, sim)
