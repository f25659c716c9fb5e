"""CPU: the host side of the ecology, plankton and ISR figures (qingdai_amd/figures.py) and its NumPy restatement
(tests/figures_ref.py) against what matplotlib and the reference's own functions recorded (tests/golden/figures_*.npz,
scripts/gen_golden_figures.py): np.nanpercentile's linear rule from two order statistics as a number, the planes handed to contourf
bit for bit, the levels bit for bit, the band colours to 1e-12 (the bound of tests/test_stateframe_cpu.py: the tables are matplotlib's
own, the midpoint arithmetic is restated), file names, the [Diagnostics] line, the sidecars, the switches and the [Plots] line."""
import json
import os
import types

import numpy as np
import pytest

import figures_ref as ref

CASES = ["allland", "flat", "full", "k1", "night", "noeco", "nonfinite", "vmax_env"]


def test_the_eight_cases_exist():
    assert sorted(ref.case_of(p) for p in ref.GOLDENS) == CASES


def _np_percentile(x):
    with np.errstate(all="ignore"):
        import warnings
        with warnings.catch_warnings():
            warnings.simplefilter("ignore")
            return float(np.nanpercentile(x, 99.0))


def _same_number(a, b):
    return (np.isnan(a) and np.isnan(b)) or a == b


def test_percentile_rule_is_numpys():
    from qingdai_amd import figures as fg
    rng = np.random.default_rng(99)
    arrays = []
    for n in list(range(1, 41)) + [99, 100, 101, 102, 200, 201, 202, 399, 400] + [int(k) for k in rng.integers(1, 401, 300)]:
        x = rng.uniform(-2.0, 5.0, n)
        kind = rng.integers(0, 6)
        if kind == 1:
            x = np.round(x)                                     # duplicates
        elif kind == 2:
            x[rng.uniform(size=n) < 0.3] = np.nan
        elif kind == 3:
            x[rng.uniform(size=n) < 0.05] = np.inf
        elif kind == 4:
            x[rng.uniform(size=n) < 0.05] = -np.inf
            x[rng.uniform(size=n) < 0.2] = np.nan
        elif kind == 5:
            x = x * 10.0 ** rng.uniform(-300, 300)
        arrays.append(x)
    arrays += [np.full(7, np.nan), np.array([np.inf]), np.array([3.0, np.inf]), np.full(101, 2.5), np.array([0.0, -0.0, 0.0])]
    assert len(arrays) > 300
    for x in arrays:
        got = fg.nanpercentile(ref.host_order_stats(x), 99.0)
        want = _np_percentile(x)
        assert _same_number(got, want), (x.size, got, want)
    # the sizes where 0.99 (n - 1) is an integer: the weight is exactly 0 there
    for n in (1, 101, 201):
        lo, hi, t = fg.percentile_plan(n)
        assert 0 <= lo < n and 0 <= hi < n and (n == 1 or (lo == int(0.99 * (n - 1) + 0.5) and abs(t) < 1e-12))


def test_plankton_vmax_rule():
    from qingdai_amd import figures as fg
    x = np.array([0.1, 0.2, np.nan, 0.4])
    os_ = ref.host_order_stats(x)
    assert fg.plankton_vmax("0.5", os_) == 0.5 and fg.plankton_vmax(" 2 ", os_) == 2.0
    assert fg.plankton_vmax(None, os_) == _np_percentile(x)
    assert fg.plankton_vmax("abc", os_) == 0.4                  # float() raises: np.nanmax
    assert fg.plankton_vmax("-1", os_) == 1e-3 and fg.plankton_vmax("inf", os_) == 1e-3
    assert fg.plankton_vmax(None, ref.host_order_stats(np.full(5, np.nan))) == 1e-3
    assert fg.plankton_vmax(None, ref.host_order_stats(np.array([-1.0, -2.0]))) == 1e-3


def test_env_parsing():
    from qingdai_amd import figures as fg
    e = fg.read_env({})
    assert (e["plot_phyto"], e["plot_eco"], e["plot_isr"], e["vmax_env"], e["height_scale"]) == (True, True, False, None, 10.0)
    assert e["eco_diag"] and e["phyto_diag"]
    e = fg.read_env({"QD_PLOT_PHYTO": "0", "QD_ECO_PLOT": "0", "QD_PLOT_ISR": "1", "QD_PHYTO_VMAX": "  ", "QD_ECO_HEIGHT_SCALE_M": "x",
                     "QD_ECO_DIAG": "0", "QD_PHYTO_DIAG": "0"})
    assert (e["plot_phyto"], e["plot_eco"], e["plot_isr"], e["vmax_env"], e["height_scale"]) == (False, False, True, None, 10.0)
    assert not e["eco_diag"] and not e["phyto_diag"]
    assert fg.read_env({"QD_PHYTO_VMAX": "0.5", "QD_ECO_HEIGHT_SCALE_M": "25"})["vmax_env"] == "0.5"
    assert fg.read_env({"QD_ECO_HEIGHT_SCALE_M": "25"})["height_scale"] == 25.0
    assert not fg.figures_enabled({}) and not fg.figures_enabled({"QD_FIGURES": "0"}) and fg.figures_enabled({"QD_FIGURES": "1"})


def _host_figures(z, meta):
    """The three figures of a golden's inputs through the product's host code and the restatement's planes and scan ->
    {"ecology": (tiles, planes), "plankton": [(tiles, planes, vmax), ...], "isr": (tiles, planes, line)}."""
    from qingdai_amd import figures as fg
    e = fg.read_env(meta["env"])
    t = meta["t_days"]
    out = {}
    tiles = fg.ecology_tiles(t, meta["eco"], meta["eco"], meta["eco"])
    planes = [None if tl["unavailable"] else ref.plane(tl["source"], tl["index"], z, e["height_scale"]) for tl in tiles]
    scan = {k: (ref.scan(planes[k])["min"], ref.scan(planes[k])["max"]) for k, tl in enumerate(tiles) if not tl["unavailable"] and k not in (1, 2)}
    out["ecology"] = (fg.ecology_levels(tiles, scan), planes)
    out["plankton"] = []
    for s in ((0, 1) if meta["SP"] >= 2 else (0,)):
        p = ref.plane("PLANKTON", s, z)
        vmax = fg.plankton_vmax(e["vmax_env"], ref.host_order_stats(p))
        out["plankton"].append(([fg.plankton_tile(t, s, vmax)], [p], vmax))
    a, b = ref.scan(z["isr_A"]), ref.scan(z["isr_B"])
    out["isr"] = (fg.isr_tiles(t, a["argmax_value"], b["argmax_value"], a["argmax"], b["argmax"]), [np.asarray(z["isr_A"]), np.asarray(z["isr_B"])],
                  fg.separation_line(t, z["lat"], z["lon"], a["argmax"], b["argmax"]))
    return out


def _check_tile(tl, plane, rec, what):
    """One tile of the product against what contourf was handed and what it chose."""
    field, lev, col, m = rec
    assert np.array_equal(plane, field, equal_nan=True), what      # the handed-in array, bit for bit
    assert tl["cmap"] == m["cmap"] and tl["extend"] == (m["extend"] == "max"), what
    assert tl["constant"] == m["constant"], what
    if tl["constant"]:
        assert tl["levels"] is None and m["n_arg"] == 20, what
        return
    assert tl["levels"].tobytes() == lev.tobytes(), (what, tl["levels"], lev)
    assert tl["colours"].shape == col.shape and np.max(np.abs(tl["colours"] - col)) <= 1e-12, what
    # the band rule on every cell: a cell of band i lies in [lev[i], lev[i + 1]), the last band closed above
    b = ref.band_index(field, lev, tl["extend"])
    fin = np.isfinite(field)
    assert np.all(b[~fin] == -1), what
    inside = fin & (field >= lev[0]) & (field <= lev[-1])
    assert np.array_equal(b >= 0, inside), what
    assert np.all(lev[b[inside]] <= field[inside]) and np.all(field[inside] <= lev[b[inside] + 1]), what


@pytest.mark.parametrize("path", ref.GOLDENS, ids=ref.case_of)
def test_planes_levels_and_colours_vs_the_reference(path):
    from qingdai_amd import figures as fg
    z = np.load(path)
    meta = ref.golden_meta(z)
    figs = _host_figures(z, meta)
    t = meta["t_days"]
    assert meta["suptitle"] is None                              # the Whittaker annotation is never drawn
    # ---- ecology
    tiles, planes = figs["ecology"]
    rec = ref.golden_tiles(z, meta, "ecology")
    assert meta["figures"]["ecology"]["files"] == [fg.ecology_name(t)]
    assert len(tiles) == (5 if meta["eco"] else 3)
    assert sorted(rec) == [k for k, tl in enumerate(tiles) if not tl["unavailable"]]
    if not meta["eco"]:
        assert [tl["unavailable"] for tl in tiles] == [True, True, True]
    for k in rec:
        _check_tile(tiles[k], planes[k], rec[k], (meta["case"], "ecology", k))
    assert [tl["coast"] for tl in tiles] == [1] * len(tiles) and [tl["cmap"] for tl in tiles][:3] == ["YlGn", "cividis", "cividis"]
    if meta["case"] == "flat":
        assert tiles[0]["constant"] and not tiles[3]["constant"]
    # ---- plankton
    rec = ref.golden_tiles(z, meta, "plankton")
    assert meta["figures"]["plankton"]["files"] == [fg.plankton_name(s, t) for s in range(len(figs["plankton"]))]
    assert len(figs["plankton"]) == (2 if meta["SP"] >= 2 else 1) == len(rec)
    for s, (tl, pl, vmax) in enumerate(figs["plankton"]):
        assert vmax == rec[s][3]["vmax"], (meta["case"], s, vmax, rec[s][3]["vmax"])
        _check_tile(tl[0], pl[0], rec[s], (meta["case"], "plankton", s))
        assert tl[0]["coast"] == 1 and len(tl[0]["levels"]) == 21
    if meta["case"] == "vmax_env":
        assert figs["plankton"][0][2] == 0.5
    if meta["case"] == "allland":
        assert figs["plankton"][0][2] == 1e-3
    # ---- ISR
    tiles, planes, line = figs["isr"]
    g = meta["figures"]["isr"]
    rec = ref.golden_tiles(z, meta, "isr")
    assert g["raised"] == (meta["case"] == "night")
    if g["raised"]:
        assert tiles[0]["constant"] and tiles[1]["constant"] and line.startswith("[Diagnostics] Day 12.25: Subsolar separation")
    else:
        assert g["files"] == [fg.isr_name(t)] and meta["printed"] == [line]
        for k in (0, 1):
            _check_tile(tiles[k], planes[k], rec[k], (meta["case"], "isr", k))
            mk = [m for m in g["marks"] if m["tile"] == k][0]
            kind, cell = tiles[k]["mark"]
            assert (mk["marker"], mk["colour"]) == (("x", "cyan") if kind == fg.MARK_X else ("+", "yellow")) and kind == k + 1
            assert (float(z["lat"][cell // 36]), float(z["lon"][cell % 36])) == (mk["lat"], mk["lon"])
        assert tiles[0]["levels"].tobytes() == tiles[1]["levels"].tobytes() and [tl["coast"] for tl in tiles] == [0, 0]


def test_isr_levels_that_contourf_refuses():
    from qingdai_amd import figures as fg
    for a, b in ((0.0, 0.0), (float("nan"), 5.0), (float("inf"), 1.0)):
        tiles = fg.isr_tiles(1.0, a, b, 3, 4)
        assert tiles[0]["constant"] and tiles[1]["constant"] and tiles[0]["mark"] == (1, 3) and tiles[1]["mark"] == (2, 4)
    assert not fg.isr_tiles(1.0, 5.0, float("nan"), 3, 4)[0]["constant"]       # Python's max(5.0, nan) is 5.0, as in the reference


def test_names_sidecar_and_packing():
    from qingdai_amd import figures as fg, _lib
    assert fg.ecology_name(12.25) == "ecology_day_012.2.png" and fg.isr_name(0.04) == "isr_components_day_000.0.png"
    assert fg.plankton_name(1, 3.96) == os.path.join("plankton", "species1_day_004.0.png")
    assert fg.mosaic_shape(5, 19, 36) == (27, 5 * 36 + 24) and fg.tile_origin(2, 19, 36) == (4, 4 + 2 * 40)
    z = np.load([p for p in ref.GOLDENS if ref.case_of(p) == "full"][0])
    meta = ref.golden_meta(z)
    figs = _host_figures(z, meta)
    tiles = figs["isr"][0]
    side = fg.sidecar("isr_components", tiles, 12.25, z["lat"], z["lon"], diagnostics=figs["isr"][2])
    side = json.loads(json.dumps(side, ensure_ascii=False))
    assert side["figure"] == "isr_components" and side["suptitle"] is None and side["layout"] == {"rows": 1, "cols": 2, "gutter": 4, "tile": [19, 36]}
    assert side["tiles"][0]["title"] == "ISR - Star A (Day 12.25)" and side["tiles"][1]["mark"]["kind"] == "+" and side["tiles"][0]["mark"]["colour"] == "cyan"
    assert side["tiles"][0]["levels"] == [float(v) for v in tiles[0]["levels"]] and side["tiles"][0]["coast"] is None
    assert side["diagnostics"] == meta["printed"][0]
    eco = fg.sidecar("ecology", fg.ecology_levels(fg.ecology_tiles(1.0, False, False, False), {}), 1.0, z["lat"], z["lon"])
    assert [t["unavailable"] for t in eco["tiles"]] == [True] * 3 and [t["levels"] for t in eco["tiles"]] == [None] * 3
    assert [t["title"] for t in eco["tiles"]] == ["LAI (Day 1.00)", "Ecology alpha (scalar)", "Ecology alpha (banded)"]
    packed = fg.pack_tiles(figs["ecology"][0])
    assert len(packed) == 5 and [p.source for p in packed] == [0, 1, 2, 3, 4] and packed[1].n_levels == 17 and packed[1].levels[16] == 0.8
    assert packed[0].mark_cell == -1 and packed[0].coast == 1 and ctypes_size(_lib.qd_tile_desc) == 8 * 4 + 8 + 32 * 8 + 32 * 24
    with pytest.raises(ValueError, match="at most 8"):
        fg.pack_tiles(figs["ecology"][0] * 2)
    big = dict(figs["ecology"][0][1], levels=np.linspace(0, 1, 40), colours=np.zeros((39, 3)))
    with pytest.raises(ValueError, match="at most 32"):
        fg.pack_tiles([big])


def ctypes_size(t):
    import ctypes
    return ctypes.sizeof(t)


def test_plots_line_wordings():
    from qingdai_amd.driver import plots_line
    sim = types.SimpleNamespace(plot_every=3, figure_names=lambda: (["plankton", "ecology", "ISR"], {}))
    assert plots_line(None, None, sim) == "[Plots] matplotlib panels are not produced by the device driver (out of the hot path)."
    assert plots_line(None, object(), sim) == ("[Plots] only the true-colour frame is produced by the device driver, every 3 steps; "
                                               "the matplotlib panels are not.")
    assert plots_line(object(), None, sim) == ("[Plots] the 15-panel state frame (state_day_*.png + .json, no axes) produced by the device "
                                               "driver, every 3 steps; the ocean, plankton, ISR and ecology figures are not.")
    assert plots_line(object(), object(), sim, None) == ("[Plots] the 15-panel state frame (state_day_*.png + .json, no axes) and the true-colour "
                                                         "frame produced by the device driver, every 3 steps; the ocean, plankton, ISR and "
                                                         "ecology figures are not.")
    on = plots_line(object(), object(), sim, object())
    assert "plankton, ecology, ISR figures" in on and "figures are not" not in on and "every 3 steps" in on and "state frame" in on
    only = plots_line(None, None, sim, object())
    assert only.startswith("[Plots] the plankton, ecology, ISR figures") and "state frame" not in only and "true-colour" not in only


def test_the_old_colour_tables_are_unchanged():
    """Greens was added; the twelve tables the state frame reads are what they were (their values, held here by a digest taken
    before the addition, and their order in the file)."""
    import hashlib
    from qingdai_amd import stateframe as sf
    with open(sf.CMAPS_JSON, encoding="ascii") as f:
        tables = json.load(f)
    old = ["coolwarm", "viridis", "Blues", "Greys", "RdBu_r", "PuOr", "magma", "cividis", "plasma", "GnBu", "YlGn", "BuPu"]
    assert list(tables) == old + ["Greens"]
    assert all(np.array(tables[k]).shape == (256, 3) for k in tables)
    digest = hashlib.sha256("".join(k + repr(tables[k]) for k in old).encode()).hexdigest()
    assert digest == OLD_TABLES_SHA256
    assert sf.cmap_table("Greens")[0].tolist() == [0.9686274509803922, 0.9882352941176471, 0.9607843137254902]


OLD_TABLES_SHA256 = "05595467e02d1d271bcc6d74e5bba051d92754f082ae930b007d9232296d0892"
