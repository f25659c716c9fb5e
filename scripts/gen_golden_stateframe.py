"""Regenerate tests/golden/stateframe_<case>_19x36.npz and tests/golden/stateframe_levels.npz from the reference's plot_state
(scripts/run_simulation.py:330-537) under real matplotlib.

Needs a checkout of the reference project (default ../reference next to this repository, or --reference DIR) and matplotlib (Agg).
Each case builds 19 x 36 inputs by hand, sets the case's QD_* environment and calls the reference's plot_state with its real
SphericalGrid and namespace stand-ins for `gcm`, `ocean` and `routing`.  Axes.contourf and Axes.streamplot are wrapped for the call:
every contourf call records the array handed in, its `levels`, `extend` and `cmap` arguments and the resulting cs.levels and
cs.get_facecolor(); every streamplot call records its `color` array (the speed the panels 7 and 8 of the device frame fill).
pyplot.savefig is replaced, so no file is written; matplotlib itself is not restated anywhere.

The golden holds the inputs, the environment of the case and, per panel, what was recorded.  The script asserts what the tests rely
on: fewer than 1 % of the cells of any panel lie within 1e-9 (levels[-1] - levels[0]) of a level (cells that sit exactly on an end
level aside: the extremes do by construction) and the two argmax cells are unique.

stateframe_levels.npz: about 300 (zmin, zmax) ranges from 1e-9 to 1e6 in width and offset with the levels contourf(levels=20)
chose for them (a 2 x 2 array with those extremes is contoured for each).
"""
import argparse
import json
import os
import sys
import types

import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))
OUT = os.path.join(HERE, "..", "tests", "golden")
NLAT, NLON = 19, 36
INPUTS = ("T_s", "h", "SST", "precip", "cloud", "u", "v", "uo", "vo", "isr", "isr_A", "isr_B", "albedo", "olr", "q", "E", "P_cond")


def base_inputs(rng):
    s = (NLAT, NLON)
    land = (rng.uniform(size=s) < 0.45).astype(np.int64)
    land[:, 28:34] = 0                                  # an ocean basin
    land[3:8, 4:12] = 1                                 # a continent
    land[NLAT - 2:, 10:20] = 1                          # land on the northern pole rows
    land[0, 0:5] = 1                                    # and on the southern one
    precip = np.where(rng.uniform(size=s) < 0.4, 0.0, rng.uniform(0.0, 5e-4, s))      # up to 43 mm/day: above the top level
    albedo = rng.uniform(0.05, 0.75, s)
    albedo[2, 3:6] = 0.85                               # above the last level: white
    isr_A, isr_B = rng.uniform(0.0, 700.0, s), rng.uniform(0.0, 400.0, s)
    isr_B[:, 0:9] = 0.0                                 # one star below the horizon there; the maximum is elsewhere
    d = dict(land_mask=land, T_s=rng.uniform(250.0, 305.0, s), h=rng.uniform(-300.0, 300.0, s), SST=rng.uniform(271.0, 303.0, s),
             precip=precip, cloud=rng.uniform(0.0, 1.0, s), u=rng.uniform(-30.0, 30.0, s), v=rng.uniform(-20.0, 20.0, s),
             uo=rng.uniform(-1.0, 1.0, s), vo=rng.uniform(-0.5, 0.5, s), isr_A=isr_A, isr_B=isr_B, isr=isr_A + isr_B, albedo=albedo,
             olr=rng.uniform(150.0, 300.0, s), q=rng.uniform(0.0, 0.02, s), E=rng.uniform(0.0, 1e-4, s), P_cond=rng.uniform(0.0, 1e-4, s),
             flow=np.zeros(s), lake_mask=np.zeros(s, dtype=np.uint8))
    d["cloud"][rng.uniform(size=s) < 0.2] = 0.0
    return d


def flow_map(rng, d, river_min):
    land = d["land_mask"] == 1
    flow = np.where(land, 10.0 ** rng.uniform(3.0, 8.0, (NLAT, NLON)), 0.0)
    flow[3:8, 4:8] = river_min                          # exactly at the threshold: a river (>=)
    flow[3:8, 8:12] = np.nextafter(river_min, 0.0)      # one ulp below: none
    flow[10, 30] = 5.0 * river_min                      # a large flow on an ocean cell: masked by land
    d["flow"] = flow
    lake = ((rng.uniform(size=(NLAT, NLON)) < 0.1) & land).astype(np.uint8)
    lake[9, 31] = 1                                     # a lake flag on an ocean cell: plot_state contours the mask as it is
    d["lake_mask"] = lake


def case_default(rng):
    return base_inputs(rng), {}, dict(ocean=True, routing=False)


def case_noocean(rng):
    return base_inputs(rng), {}, dict(ocean=False, routing=False)


def case_ps_abs(rng):
    return base_inputs(rng), {"QD_PLOT_PS_MODE": "abs"}, dict(ocean=True, routing=False)


def case_rivers(rng):
    d = base_inputs(rng)
    flow_map(rng, d, 1e6)
    return d, {}, dict(ocean=True, routing=True)


def case_nonfinite(rng):
    d = base_inputs(rng)
    d["T_s"][4, 7] = np.nan
    d["T_s"][12, 30] = np.nan
    d["precip"][6, 6] = np.nan
    d["q"][10, 3] = np.nan
    d["u"][9, 20] = np.nan                              # the vorticity of the cells north and south of it is NaN
    d["E"][5, 15] = np.inf                              # nan_to_num -> 1.8e308, times 86400 -> inf: masked by contourf
    return d, {}, dict(ocean=True, routing=False)


def case_constant(rng):
    d = base_inputs(rng)
    d["E"][:] = 0.0
    d["P_cond"][:] = 0.0
    d["cloud"][3, 3:9] = 1.25                           # above the last level: white
    d["cloud"][4, 3:9] = -0.25                          # below the first
    d["cloud"][5, 3:9] = 1.0                            # on the last level: the closed top band
    return d, {}, dict(ocean=True, routing=False)


CASES = {"default": case_default, "noocean": case_noocean, "ps_abs": case_ps_abs, "rivers": case_rivers, "nonfinite": case_nonfinite,
         "constant": case_constant}


def near_level_fraction(z, lev):
    """The share of the finite cells of z that lie within 1e-9 of the level range of a level, those exactly on an end level aside."""
    z = np.asarray(z, dtype=float)
    ok = np.isfinite(z) & (z != lev[0]) & (z != lev[-1])
    if not ok.any():
        return 0.0
    dist = np.min(np.abs(z[ok][:, None] - np.asarray(lev)[None, :]), axis=1)
    return float(np.mean(dist <= 1e-9 * (lev[-1] - lev[0])))


def run_case(name, rs, SphericalGrid):
    from matplotlib.axes import Axes
    rng = np.random.default_rng(sum(map(ord, "stateframe_" + name)))
    d, env, has = CASES[name](rng)
    for k in [k for k in os.environ if k.startswith("QD_")]:
        del os.environ[k]
    os.environ.update(env)
    grid = SphericalGrid(NLAT, NLON)
    p0, rho_a, H = 1.0e5, 1.2, 8000.0
    gcm = types.SimpleNamespace(T_s=d["T_s"], h=d["h"], u=d["u"], v=d["v"], isr=d["isr"], isr_A=d["isr_A"], isr_B=d["isr_B"], olr=d["olr"],
                                q=d["q"], E_flux_last=d["E"], P_cond_flux_last=d["P_cond"], H=H,
                                hum_params=types.SimpleNamespace(p0=p0, rho_a=rho_a))
    ocean = types.SimpleNamespace(Ts=d["SST"], uo=d["uo"], vo=d["vo"]) if has["ocean"] else None
    routing = types.SimpleNamespace(diagnostics=lambda: {"flow_accum_kgps": d["flow"]}, lake_mask=d["lake_mask"]) if has["routing"] else None
    rec, saved_name = {}, {}
    real_contourf, real_streamplot = Axes.contourf, Axes.streamplot

    def panel_of(ax):
        return int(ax.get_subplotspec().num1)

    def contourf(ax, *a, **kw):
        cs = real_contourf(ax, *a, **kw)
        lev_arg = kw.get("levels")
        rec[panel_of(ax)] = dict(field=np.array(a[2], dtype=float, copy=True), cmap=str(kw.get("cmap")), extend=str(kw.get("extend", "neither")),
                                 levels_arg=-1.0 * np.ones(1) if np.isscalar(lev_arg) else np.array(lev_arg, dtype=float),
                                 n_arg=int(lev_arg) if np.isscalar(lev_arg) else 0,
                                 levels=np.array(cs.levels, dtype=float), colours=np.array(cs.get_facecolor(), dtype=float)[:, :3])
        return cs

    def streamplot(ax, *a, **kw):
        rec[panel_of(ax)] = dict(field=np.array(kw["color"], dtype=float, copy=True), cmap=str(kw.get("cmap")), extend="neither",
                                 levels_arg=np.zeros(0), n_arg=0, levels=np.zeros(0), colours=np.zeros((0, 3)))
        return real_streamplot(ax, *a, **kw)

    saved = (Axes.contourf, Axes.streamplot, rs.plt.savefig)
    Axes.contourf, Axes.streamplot = contourf, streamplot
    rs.plt.savefig = lambda *a, **k: saved_name.update(filename=a[0])
    try:
        with np.errstate(all="ignore"):
            rs.plot_state(grid, gcm, d["land_mask"], d["precip"], d["cloud"], d["albedo"], 12.25, "out", ocean=ocean, routing=routing)
    finally:
        Axes.contourf, Axes.streamplot, rs.plt.savefig = saved
    assert os.path.basename(saved_name["filename"]) == "state_day_012.2.png" and sorted(rec) == list(range(15)), sorted(rec)
    # the conditions the tests rely on
    worst, constant = 0.0, []
    for k in range(15):
        z = rec[k]["field"][np.isfinite(rec[k]["field"])]
        # the stated departure: a data-dependent level rule on a field without a range leaves the panel white ("constant")
        constant.append(bool(rec[k]["n_arg"] > 0 and (z.size == 0 or z.max() - z.min() <= 1e-12 * max(abs(z.min()), abs(z.max())))))
        if len(rec[k]["levels"]) >= 2 and not constant[k]:
            frac = near_level_fraction(rec[k]["field"], rec[k]["levels"])
            worst = max(worst, frac)
            assert frac < 0.01, f"{name}: panel {k + 1} has {frac:.3%} of its cells within 1e-9 of a level"
    for key in ("isr_A", "isr_B"):
        a = d[key]
        assert int((a == np.nanmax(a)).sum()) == 1 and not np.isnan(a).any(), f"{name}: {key} ties for its argmax"
    meta = {"case": name, "nlat": NLAT, "nlon": NLON, "env": env, "ocean": bool(has["ocean"]), "routing": bool(has["routing"]),
            "p0": p0, "rho_a": rho_a, "H": H, "t_days": 12.25, "cmaps": [rec[k]["cmap"] for k in range(15)],
            "extend": [rec[k]["extend"] for k in range(15)], "n_arg": [rec[k]["n_arg"] for k in range(15)], "constant": constant}
    arrays = {}
    for k in range(15):
        arrays[f"levels_arg_{k}"], arrays[f"levels_{k}"], arrays[f"colours_{k}"] = rec[k]["levels_arg"], rec[k]["levels"], rec[k]["colours"]
    np.savez_compressed(os.path.join(OUT, f"stateframe_{name}_{NLAT}x{NLON}.npz"), lat=grid.lat, lon=grid.lon,
                        land_mask=d["land_mask"].astype(np.int8), flow=d["flow"], lake_mask=d["lake_mask"],
                        fields=np.stack([rec[k]["field"] for k in range(15)]), meta=json.dumps(meta), **{k: d[k] for k in INPUTS}, **arrays)
    print(f"{name}: 15 panels, levels {[len(rec[k]['levels']) for k in range(15)]}, constant {[k + 1 for k in range(15) if constant[k]]}, "
          f"worst near-level share {worst:.3%}")


def level_ranges():
    import matplotlib.pyplot as plt
    rng = np.random.default_rng(20)
    rows = []
    for i in range(300):
        w = 10.0 ** rng.uniform(-9, 6)
        off = [0.0, 1.0, -1.0][i % 3] * 10.0 ** rng.uniform(-9, 6)
        zmin = off + rng.uniform(-1.0, 1.0) * w
        rows.append((zmin, zmin + w))
    rows += [(0.0, 1.0), (-1.0, 1.0), (0.0, 30.0), (999.0, 1001.0), (1e5, 1e5 + 1e-3), (-273.15, 40.0), (0.0, 1e-9), (-5e-5, 7e-5)]
    fig, ax = plt.subplots()
    zmin, zmax, lev, cnt = [], [], np.full((len(rows), 32), np.nan), []
    for k, (a, b) in enumerate(rows):
        if not b > a:
            continue
        cs = ax.contourf(np.array([[a, b], [a, b]]), levels=20)
        zmin.append(a), zmax.append(b), cnt.append(len(cs.levels))
        assert len(cs.levels) <= 32
        lev[len(cnt) - 1, :len(cs.levels)] = cs.levels
    plt.close(fig)
    np.savez_compressed(os.path.join(OUT, "stateframe_levels.npz"), zmin=np.array(zmin), zmax=np.array(zmax), count=np.array(cnt),
                        levels=lev[:len(cnt)])
    print(f"stateframe_levels: {len(cnt)} ranges, {min(cnt)}..{max(cnt)} levels")


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reference", default=os.path.join(HERE, "..", "..", "reference"))
    ap.add_argument("cases", nargs="*", default=list(CASES) + ["levels"])
    a = ap.parse_args()
    root = os.path.abspath(a.reference)
    sys.path.insert(0, root)
    sys.path.insert(0, os.path.join(root, "scripts"))
    os.environ["MPLBACKEND"] = "Agg"
    import run_simulation as rs                         # the reference driver (its main() runs only under __main__)
    from pygcm.grid import SphericalGrid
    for name in a.cases:
        if name == "levels":
            level_ranges()
        else:
            run_case(name, rs, SphericalGrid)


if __name__ == "__main__":
    main()
