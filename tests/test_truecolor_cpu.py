"""CPU: the host side of the true-colour frame (qingdai_amd/truecolor.py, imgio.py) and the NumPy restatement the GPU tests lean
on (tests/truecolor_ref.py) against the goldens recorded from the reference's plot_true_color
(scripts/gen_golden_truecolor.py): masks and tie cells exactly, rgb within truecolor_ref.BOUND with identical NaN positions, the
environment and the channel weights, the PNG writer, and the reference's plot clock against hand-listed steps."""
import glob
import os

import numpy as np
import pytest

import truecolor_ref as ref

HERE = os.path.dirname(os.path.abspath(__file__))
GOLDENS = sorted(glob.glob(os.path.join(HERE, "golden", "truecolor_*_19x36.npz")))
CASES = ["all_nondefault", "base", "nonfinite", "oceancolour", "rivers", "veg", "veg_nolai"]


def _case(path):
    return os.path.basename(path)[len("truecolor_"):-len("_19x36.npz")]


def test_every_case_has_a_golden():
    assert [_case(p) for p in GOLDENS] == CASES


@pytest.mark.parametrize("path", GOLDENS, ids=_case)
def test_restatement_vs_reference_goldens(path, monkeypatch):
    z = np.load(path)
    ref.set_env(monkeypatch, ref.golden_meta(z)["env"])
    p, eco_tab, phyto_tab, lake, bands, flow = ref.golden_config(z)
    got = ref.render(z, p, eco_tab, phyto_tab, bands, lake, flow, lat=z["lat"])
    assert np.array_equal(got["sea_ice_mask"], z["sea_ice_mask"])
    want = z["rgb"]
    assert np.array_equal(np.isnan(got["rgb"]), np.isnan(want))
    ok = ~np.isnan(want)
    dev = float(np.max(np.abs(got["rgb"][ok] - want[ok])))
    dev2 = float(np.max(np.abs(got["sea_ice"] - z["sea_ice"])))
    print(f"{_case(path)}: rgb {dev:.3e} sea ice {dev2:.3e} (bound {ref.BOUND:.1e})")
    assert dev <= ref.BOUND and dev2 <= ref.BOUND
    case = _case(path)
    land = z["land_mask"] == 1
    if case == "base":                                          # the tie cells: C at the threshold is snow, one ulp below and NaN are not
        bare = np.array(ref.LAND) * (1.0 - p.cloud_alpha * z["cloud"][..., None]) + (p.cloud_alpha * z["cloud"][..., None]) * p.cloud_white
        assert not np.any(np.all(got["rgb"][4, 4:8] == bare[4, 4:8], axis=-1))
        assert np.array_equal(got["rgb"][5:7, 4:8], bare[5:7, 4:8])
    if case == "rivers":                                        # flow at river_min is a river, one ulp below is not; ocean cells carry neither
        pr = dict(p=p, eco_tab=eco_tab, phyto_tab=phyto_tab, phyto_bands=bands, lake_mask=lake, lat=z["lat"])
        dry = ref.render(z, flow=np.zeros_like(z["flow"]), **pr)["rgb"]
        changed = np.any(got["rgb"] != dry, axis=-1)
        assert changed[3:8, 4:8].all() and not changed[3:8, 8:12].any() and not changed[~land].any()
        assert z["lake_mask"][9, 31] == 1 and not land[9, 31]
    if case == "nonfinite":
        assert int(np.isnan(want).any(axis=-1).sum()) == 1 and got["img"][::-1][np.isnan(want).any(axis=-1)].tolist() == [[0, 0, 0]]
    if case == "oceancolour":                                   # sea-ice cells stay ice-coloured under the overlay
        ice = np.array(ref.ICE) * (1.0 - p.cloud_alpha * z["cloud"][..., None]) + (p.cloud_alpha * z["cloud"][..., None]) * p.cloud_white
        assert np.array_equal(got["rgb"][z["sea_ice_mask"]], np.clip(ice, 0.0, 1.0)[z["sea_ice_mask"]])


@pytest.mark.parametrize("path", GOLDENS, ids=_case)
def test_environment_and_printed_line(path, monkeypatch):
    from qingdai_amd.truecolor import read_env, truecolor_line, frame_name
    z = np.load(path)
    env = ref.golden_meta(z)["env"]
    ref.set_env(monkeypatch, env)
    e = read_env()
    names = {"h_ice_ref": ("QD_HICE_REF", 0.5), "ice_frac_thr": ("QD_TRUECOLOR_ICE_FRAC", 0.15), "snow_cover_frac": ("QD_SNOW_COVER_FRAC", 0.20),
             "snow_vis_alpha": ("QD_SNOW_VIS_ALPHA", 0.60), "veg_gamma": ("QD_ECO_TRUECOLOR_GAMMA", 1.8), "veg_sat": ("QD_ECO_TRUECOLOR_SAT", 1.35),
             "oc_blend": ("QD_OC_BLEND", 0.85), "snow_thresh": ("QD_SNOW_THRESH", 273.15), "cloud_alpha": ("QD_TRUECOLOR_CLOUD_ALPHA", 0.60),
             "cloud_white": ("QD_TRUECOLOR_CLOUD_WHITE", 0.95), "river_min": ("QD_RIVER_MIN_KGPS", 1e6), "river_alpha": ("QD_RIVER_ALPHA", 0.45),
             "lake_alpha": ("QD_LAKE_ALPHA", 0.40)}
    for k, (name, default) in names.items():
        assert e[k] == float(env.get(name, default)), k
    assert e["oc_gamma"] == float(env.get("QD_OC_GAMMA", env.get("QD_ECO_TRUECOLOR_GAMMA", 2.2)))
    assert e["snow_by_ts"] == (env.get("QD_TRUECOLOR_SNOW_BY_TS", "0") == "1") and e["snow_by_swe"] and e["veg"] and e["rivers"]
    # the recorded line of the reference from the recorded numbers
    assert truecolor_line(z["sea_ice"][0], z["sea_ice"][1], e["ice_frac_thr"], e["cloud_alpha"]) == str(z["line"])
    assert frame_name(ref.golden_meta(z)["t_days"]) == "true_color_day_012.2.png"


def test_environment_fallbacks(monkeypatch):
    from qingdai_amd.truecolor import read_env
    ref.set_env(monkeypatch, {"QD_ECO_TRUECOLOR_GAMMA": "x", "QD_ECO_TRUECOLOR_SAT": "", "QD_OC_BLEND": "no"})
    e = read_env()
    assert (e["veg_gamma"], e["veg_sat"], e["oc_gamma"], e["oc_blend"]) == (1.8, 1.35, 2.2, 0.85)
    ref.set_env(monkeypatch, {"QD_ECO_TRUECOLOR_GAMMA": "2.0"})
    assert read_env()["oc_gamma"] == 2.0                        # QD_OC_GAMMA falls back to the vegetation gamma before its own 2.2
    ref.set_env(monkeypatch, {"QD_ECO_TRUECOLOR_GAMMA": "2.0", "QD_OC_GAMMA": "1.5"})
    assert read_env()["oc_gamma"] == 1.5
    ref.set_env(monkeypatch, {"QD_RIVER_ALPHA": "x"})           # the reference's river block fails as a whole: no rivers, no lakes
    e = read_env()
    assert not e["rivers"] and not e["overlay_ok"]
    ref.set_env(monkeypatch, {"QD_HICE_REF": "x"})
    with pytest.raises(ValueError):
        read_env()


def test_channel_weights(monkeypatch):
    from qingdai_amd.truecolor import channel_weights, band_centers, build_config
    z = np.load([p for p in GOLDENS if _case(p) == "all_nondefault"][0])
    ref.set_env(monkeypatch, ref.golden_meta(z)["env"])
    p, eco_tab, phyto_tab, lake, _bands, _flow = ref.golden_config(z)
    assert (p.nb_eco, p.nb_phyto, p.veg, p.veg_f_one, p.oceancolor, p.rivers, p.lakes, p.soil_ref) == (12, 5, 1, 0, 1, 1, 1, 0.3)
    lam = z["eco_lambda"]
    assert np.array_equal(band_centers(ref.stand_ins(z)[0].bands, 12), lam)
    for row, (mu, sg) in zip(eco_tab[1:4], ((610.0, 50.0), (550.0, 40.0), (460.0, 40.0))):
        w = np.exp(-((lam - mu) ** 2) / (2.0 * sg ** 2))
        assert np.array_equal(row, w / (float(np.sum(w)) + 1e-12)) and abs(row.sum() - 1.0) < 1e-10
        assert int(np.argmax(row)) == int(np.argmin(np.abs(lam - mu)))
    assert np.array_equal(eco_tab[0], z["eco_R_eff"])
    assert np.array_equal(band_centers(None, 4), np.linspace(420.0, 680.0, 4))              # the coarse fallback
    assert np.array_equal(band_centers(ref.stand_ins(z)[1].bands, 5), z["phyto_lambda"])
    assert all(np.array_equal(a, b) for a, b in zip(channel_weights(z["phyto_lambda"]), phyto_tab[0:3]))
    assert np.all(eco_tab[6] != 1.0) and np.array_equal(lake, (z["lake_mask"] != 0).astype(np.uint8))       # the Rayleigh mode reached the tables
    z2 = np.load([p for p in GOLDENS if _case(p) == "veg_nolai"][0])
    ref.set_env(monkeypatch, ref.golden_meta(z2)["env"])
    p2 = build_config(None, *ref.stand_ins(z2))[0]
    assert (p2.veg, p2.veg_f_one, p2.nb_eco, p2.oceancolor, p2.rivers, p2.lakes) == (1, 1, 16, 0, 0, 0)
    big = ref.stand_ins(z2)[0]
    big.bands = type(big.bands)(17, np.zeros(18), np.zeros(17), np.zeros(17))
    with pytest.raises(ValueError, match="at most 16"):
        build_config(None, big, None, None)


@pytest.mark.parametrize("shape", [(5, 4), (19, 36)])
def test_png_round_trip(shape, tmp_path):
    from qingdai_amd.imgio import write_png, read_png
    img = np.random.default_rng(shape[0]).integers(0, 256, shape + (3,), dtype=np.uint8)
    img[0, 0], img[-1, -1] = (0, 0, 0), (255, 255, 255)
    path = str(tmp_path / "a.png")
    write_png(path, img)
    assert np.array_equal(read_png(path), img)
    raw = open(path, "rb").read()
    assert raw[:8] == b"\x89PNG\r\n\x1a\n" and raw[12:16] == b"IHDR" and raw[-8:-4] == b"IEND"
    try:
        from PIL import Image
    except ImportError:
        Image = None
    if Image is not None:
        with Image.open(path) as im:
            assert im.mode == "RGB" and im.size == (shape[1], shape[0]) and np.array_equal(np.asarray(im), img)
    with pytest.raises(ValueError):
        write_png(path, img.astype(np.float64))
    with pytest.raises(ValueError):
        write_png(path, img[..., 0])


def test_png_reader_undoes_the_filters(tmp_path):
    """read_png on scanlines filtered with Sub, Up, Average and Paeth (which write_png never emits)."""
    import struct
    import zlib
    from qingdai_amd.imgio import read_png, _chunk, _SIG
    img = np.random.default_rng(1).integers(0, 256, (5, 4, 3), dtype=np.uint8)
    lines, prev = [], np.zeros(12, dtype=np.int64)
    for y in range(5):
        cur = img[y].reshape(12).astype(np.int64)
        a = np.concatenate([np.zeros(3, dtype=np.int64), cur[:-3]])
        c = np.concatenate([np.zeros(3, dtype=np.int64), prev[:-3]])
        ft = y % 5
        pa, pb, pc = np.abs(prev - c), np.abs(a - c), np.abs(a + prev - 2 * c)
        paeth = np.where((pa <= pb) & (pa <= pc), a, np.where(pb <= pc, prev, c))
        pred = [np.zeros(12, dtype=np.int64), a, prev, (a + prev) // 2, paeth][ft]
        lines.append(bytes([ft]) + ((cur - pred) & 255).astype(np.uint8).tobytes())
        prev = cur
    path = str(tmp_path / "f.png")
    with open(path, "wb") as f:
        f.write(_SIG + _chunk(b"IHDR", struct.pack(">IIBBBBB", 4, 5, 8, 2, 0, 0, 0)) + _chunk(b"IDAT", zlib.compress(b"".join(lines))) +
                _chunk(b"IEND", b""))
    assert np.array_equal(read_png(path), img)


def test_plot_clock_against_hand_listed_steps():
    from qingdai_amd.truecolor import plot_interval_steps, firing_steps
    from qingdai_amd.driver import chunk_until
    # 0.03125 d = 2700 s: dt = 300 divides it (9 steps), dt = 400 does not (6.75 -> 6), dt = 4000 is longer than it (0 -> 1)
    env = {"QD_PLOT_EVERY_DAYS": "0.03125"}
    assert [plot_interval_steps(env, dt) for dt in (300, 400, 4000)] == [9, 6, 1]
    assert plot_interval_steps({}, 300) == 2880                 # the default: 10 days
    assert firing_steps(0, 20, 9) == [0, 9, 18]
    assert firing_steps(0, 20, 6) == [0, 6, 12, 18]
    assert firing_steps(0, 4, 1) == [0, 1, 2, 3]
    assert firing_steps(10, 20, 9) == [8, 17]                   # run-local index 18 and 27
    assert firing_steps(1, 5, 9) == []
    # the chunks of a 20-step run at interval 9 through the driver's loop: each ends with a firing step, behind which the frame runs
    from qingdai_amd.driver import Simulation
    chunks, frames = [], []

    class Sim(Simulation):
        def run_steps(self, n):
            chunks.append(n)
            _, self._t = self._span_times(n)

        def run_truecolor(self, t_days):
            frames.append((sum(chunks) - 1, t_days))
    sim = Sim.__new__(Sim)
    sim.dt, sim.day_seconds, sim.truecolor, sim.plot_every = 300.0, 86400.0, object(), 9
    sim.t = 0.0
    sim.run_loop(20)
    assert chunks == [1, 9, 9, 1] and frames == [(0, 0.0), (9, 9 * 300.0 / 86400.0), (18, 18 * 300.0 / 86400.0)]
    # the earlier of two cadences ends the chunk; both on one step end it once
    assert chunk_until(0.0, 300.0, None, 50, fire_in=min(7, 3)) == 3 and chunk_until(0.0, 300.0, None, 50, fire_in=min(4, 4)) == 4
