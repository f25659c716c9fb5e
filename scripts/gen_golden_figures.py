"""Regenerate tests/golden/figures_<case>_19x36.npz from the reference's plot_ecology (scripts/run_simulation.py:954-1060),
plot_plankton_species (:828-889) and plot_isr_components (:891-951) under real matplotlib.

Needs a checkout of the reference project (default ../reference next to this repository, or --reference DIR) and matplotlib (Agg).
Each case builds 19 x 36 inputs by hand, sets the case's QD_* environment and calls the reference's own three functions with its real
SphericalGrid and namespace stand-ins for `gcm` and `phyto`; the canopy height and the species densities come from the reference's
PopulationManager.canopy_height_map / species_density_maps, called unbound on a stand-in with LAI_layers_SK, K, Ns, shape and land.
Axes.contourf and Axes.scatter are wrapped for the calls: every contourf call records the array handed in, its `levels`, `extend` and
`cmap` arguments and the resulting cs.levels and cs.get_facecolor(); every scatter call its position.  pyplot.savefig is replaced, so
no figure is written; what the functions print is captured.  matplotlib itself is not restated anywhere.

The golden holds the inputs, the environment and, per figure and tile, what was recorded (arrays and one JSON meta string).  The
script asserts what the tests rely on: no finite cell of a compared tile sits exactly on an interior level, so band indices are
compared on every cell; and the argmax cell of an ISR plane is unique wherever the case says so (`mark_unique`).
"""
import argparse
import contextlib
import io
import json
import os
import sys
import tempfile
import types

import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))
OUT = os.path.join(HERE, "..", "tests", "golden")
NLAT, NLON = 19, 36
T_DAYS = 12.25


def base(rng, S=3, K=3, SP=3):
    s = (NLAT, NLON)
    land = (rng.uniform(size=s) < 0.45).astype(np.int64)
    land[:, 28:34] = 0                                  # an ocean basin
    land[3:8, 4:12] = 1                                 # a continent
    land[NLAT - 2:, 10:20] = 1                          # land on the northern pole rows
    land[0, 0:5] = 1                                    # and on the southern one
    layers = rng.uniform(0.0, 1.5, (S, K) + s)          # ocean cells hold values too: the maps must mask them
    layers[:, :, 5, 5:8] = 0.0                          # bare land
    lai = np.where(land == 1, layers.sum(axis=(0, 1)), 0.0)
    alpha = np.where(land == 1, rng.uniform(0.05, 0.75, s), np.nan)
    alpha[4, 5:7] = 0.85                                # above the last level: white
    banded = np.where(land == 1, rng.uniform(0.05, 0.75, s), np.nan)
    C = rng.uniform(0.0, 1.3, (SP,) + s) ** 3
    C[:, land == 1] = 0.0
    C[0, 9, 30] = -0.01                                 # a negative concentration: white
    isr_A, isr_B = rng.uniform(0.0, 700.0, s), rng.uniform(0.0, 400.0, s)
    isr_B[:, 0:9] = 0.0                                 # one star below the horizon there; the maximum is elsewhere
    return dict(land_mask=land, layers=layers, lai=lai, alpha=alpha, banded=banded, C=C, isr_A=isr_A, isr_B=isr_B)


def case_full(rng):
    return base(rng), {}, dict(eco=True)


def case_k1(rng):
    return base(rng, S=1, K=1, SP=1), {"QD_ECO_HEIGHT_SCALE_M": "25"}, dict(eco=True)


def case_nonfinite(rng):
    d = base(rng)
    d["layers"][1, 2, 4, 6] = np.nan
    d["layers"][0, 0, 6, 9] = np.nan
    d["layers"][2, 1, 3:6, 10] = -0.7                   # negative layers count as 0
    d["layers"][:, :, 7, 11] = -1.0
    d["lai"][6, 5] = np.nan
    d["alpha"][5, 8] = np.nan
    d["banded"][6, 8] = np.inf                          # nan_to_num -> 1.8e308: above every level
    d["C"][0, 10, 29] = np.nan
    d["C"][0, 11, 31] = np.inf
    d["C"][1, 12, 32] = np.inf
    return d, {}, dict(eco=True)


def case_noeco(rng):
    return base(rng), {}, dict(eco=False)


def case_vmax_env(rng):
    return base(rng), {"QD_PHYTO_VMAX": "0.5"}, dict(eco=True)


def case_allland(rng):
    d = base(rng)
    d["land_mask"][:] = 1
    d["lai"] = d["layers"].sum(axis=(0, 1))
    d["alpha"] = rng.uniform(0.05, 0.75, d["lai"].shape)
    d["banded"] = rng.uniform(0.05, 0.75, d["lai"].shape)
    return d, {}, dict(eco=True)


def case_flat(rng):
    d = base(rng)
    d["lai"][:] = 0.0
    d["isr_B"][:] = 0.0
    return d, {}, dict(eco=True, mark_unique=[True, False])


def case_night(rng):
    d = base(rng)
    d["isr_A"][:] = 0.0
    d["isr_B"][:] = 0.0
    return d, {}, dict(eco=True, mark_unique=[False, False])


CASES = {"full": case_full, "k1": case_k1, "nonfinite": case_nonfinite, "noeco": case_noeco, "vmax_env": case_vmax_env,
         "allland": case_allland, "flat": case_flat, "night": case_night}


def on_interior_level(z, lev):
    z = np.asarray(z, dtype=float)
    return int(np.isin(z[np.isfinite(z)], np.asarray(lev)[1:-1]).sum()) if len(lev) > 2 else 0


def run_case(name, rs, SphericalGrid, PopulationManager):
    from matplotlib.axes import Axes
    rng = np.random.default_rng(sum(map(ord, "figures_" + name)))
    d, env, has = CASES[name](rng)
    for k in [k for k in os.environ if k.startswith("QD_")]:
        del os.environ[k]
    os.environ.update(env)
    grid = SphericalGrid(NLAT, NLON)
    land = d["land_mask"]
    S, K = d["layers"].shape[:2]
    calls, marks, saved = [], [], []
    real_contourf, real_scatter, real_savefig = Axes.contourf, Axes.scatter, rs.plt.savefig

    def contourf(ax, *a, **kw):
        cs = real_contourf(ax, *a, **kw)
        lev_arg = kw.get("levels")
        calls.append(dict(tile=int(ax.get_subplotspec().num1), field=np.array(a[2], dtype=float, copy=True), cmap=str(kw.get("cmap")),
                          extend=str(kw.get("extend", "neither")), n_arg=int(lev_arg) if np.isscalar(lev_arg) else 0,
                          levels_arg=np.zeros(0) if np.isscalar(lev_arg) else np.array(lev_arg, dtype=float),
                          levels=np.array(cs.levels, dtype=float), colours=np.array(cs.get_facecolor(), dtype=float)[:, :3]))
        return cs

    def scatter(ax, x, y, *a, **kw):
        marks.append(dict(tile=int(ax.get_subplotspec().num1), lon=float(np.ravel(x)[0]), lat=float(np.ravel(y)[0]), marker=str(kw.get("marker")),
                          colour=str(kw.get("c"))))
        return real_scatter(ax, x, y, *a, **kw)

    Axes.contourf, Axes.scatter = contourf, scatter
    rs.plt.savefig = lambda *a, **k: saved.append(str(a[0]))
    figs, printed, suptitle = {}, io.StringIO(), "unset"
    real_close = rs.plt.close
    cwd = os.getcwd()
    try:
        with tempfile.TemporaryDirectory() as tmp, np.errstate(all="ignore"), contextlib.redirect_stdout(printed):
            os.chdir(tmp)                                   # plot_plankton_species makes out/plankton
            # ---- ecology
            pop = types.SimpleNamespace(LAI_layers_SK=d["layers"], K=K, Ns=S, shape=(NLAT, NLON), land=(land == 1))
            kw = dict(lai=None, alpha_ecology=None, alpha_banded=None, canopy_height=None, species_density=None)
            if has["eco"]:
                kw = dict(lai=d["lai"], alpha_ecology=d["alpha"], alpha_banded=d["banded"],
                          canopy_height=PopulationManager.canopy_height_map(pop), species_density=PopulationManager.species_density_maps(pop))
            holder = {}
            rs.plt.close = lambda fig=None: holder.update(suptitle=getattr(fig, "_suptitle", None))
            rs.plot_ecology(grid, land, T_DAYS, "out", **kw)
            suptitle = holder.get("suptitle")
            rs.plt.close = real_close
            figs["ecology"] = (list(calls), list(marks), list(saved), False)
            calls.clear(), marks.clear(), saved.clear()
            # ---- plankton
            rs.plot_plankton_species(grid, types.SimpleNamespace(C_phyto_s=d["C"]), land, T_DAYS, "out")
            for k, c in enumerate(calls):
                c["tile"] = k                               # one figure per species: number them in call order
            figs["plankton"] = (list(calls), list(marks), list(saved), False)
            calls.clear(), marks.clear(), saved.clear()
            # ---- ISR
            raised = False
            try:
                rs.plot_isr_components(grid, types.SimpleNamespace(isr_A=d["isr_A"], isr_B=d["isr_B"]), T_DAYS, "out")
            except ValueError:
                raised = True                               # contourf: "Contour levels must be increasing"
            figs["isr"] = (list(calls), list(marks), list(saved), raised)
            os.chdir(cwd)
    finally:
        os.chdir(cwd)
        Axes.contourf, Axes.scatter, rs.plt.savefig, rs.plt.close = real_contourf, real_scatter, real_savefig, real_close
        rs.plt.close("all")
    assert suptitle is None, f"{name}: plot_ecology drew a suptitle: {suptitle!r}"
    meta = {"case": name, "nlat": NLAT, "nlon": NLON, "env": env, "eco": bool(has["eco"]), "S": S, "K": K, "SP": int(d["C"].shape[0]),
            "t_days": T_DAYS, "suptitle": None, "printed": [ln for ln in printed.getvalue().splitlines() if ln.startswith("[Diagnostics]")],
            "mark_unique": has.get("mark_unique", [True, True]), "figures": {}}
    arrays = {}
    for fig, (cl, mk, sv, raised) in figs.items():
        tiles = []
        for c in cl:
            z = c["field"][np.isfinite(c["field"])]
            constant = bool(c["n_arg"] > 0 and (z.size == 0 or z.max() - z.min() <= 1e-12 * max(abs(z.min()), abs(z.max()))))
            if not constant:
                hit = on_interior_level(c["field"], c["levels"])
                assert hit == 0, f"{name}: {fig} tile {c['tile']} has {hit} cells exactly on an interior level"
            key = f"{fig}_{c['tile']}"
            arrays[key + "_field"], arrays[key + "_levels"], arrays[key + "_colours"] = c["field"], c["levels"], c["colours"]
            arrays[key + "_levels_arg"] = c["levels_arg"]
            tiles.append({"tile": c["tile"], "cmap": c["cmap"], "extend": c["extend"], "n_arg": c["n_arg"], "constant": constant,
                          "vmax": float(c["levels"][-1])})
        meta["figures"][fig] = {"tiles": tiles, "marks": mk, "files": [os.path.relpath(p, "out") for p in sv], "raised": raised}
    for key, uniq in zip(("isr_A", "isr_B"), meta["mark_unique"]):
        if uniq:
            a = d[key]
            assert int((a == np.nanmax(a)).sum()) == 1 and not np.isnan(a).any(), f"{name}: {key} ties for its argmax"
    np.savez_compressed(os.path.join(OUT, f"figures_{name}_{NLAT}x{NLON}.npz"), lat=grid.lat, lon=grid.lon, land_mask=land.astype(np.int8),
                        layers=d["layers"], lai=d["lai"], alpha=d["alpha"], banded=d["banded"], C=d["C"], isr_A=d["isr_A"], isr_B=d["isr_B"],
                        meta=json.dumps(meta), **arrays)
    print(f"{name}: " + ", ".join(f"{fig} {[t['tile'] for t in m['tiles']]}{' (raised)' if m['raised'] else ''} -> {m['files']}"
                                  for fig, m in meta["figures"].items()))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reference", default=os.path.join(HERE, "..", "..", "reference"))
    ap.add_argument("cases", nargs="*", default=list(CASES))
    a = ap.parse_args()
    root = os.path.abspath(a.reference)
    sys.path.insert(0, root)
    sys.path.insert(0, os.path.join(root, "scripts"))
    os.environ["MPLBACKEND"] = "Agg"
    import run_simulation as rs                         # the reference driver (its main() runs only under __main__)
    from pygcm.grid import SphericalGrid
    from pygcm.ecology.population import PopulationManager
    for name in a.cases:
        run_case(name, rs, SphericalGrid, PopulationManager)


if __name__ == "__main__":
    main()
