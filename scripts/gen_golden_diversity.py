"""Regenerate tests/golden/diversity_<case>_19x36.npz from the reference's diversity diagnostics (pygcm/ecology/diversity.py).

Needs a checkout of the reference project (default ../reference next to this repository, or --reference DIR) and matplotlib, which
the reference module imports.  Each case builds a land mask and a [S, K, lat, lon] LAI stack by hand, forms L_s the way the
reference's _get_species_lai_SK does and calls its compute_alpha_eff_map, compute_local_bray_curtis and compute_whittaker_beta.
The golden holds the inputs (stack, land_mask, lat) and the outputs (L_s, alpha_map, bc_local, summary = alpha_mean, gamma_eff,
beta_whittaker).

The summary goes into a text file with four decimals, and the device's log / exp differ from NumPy's in the last bits: the script
asserts that no finite summary value lies within 1e-9 of a rounding boundary of the fourth decimal.
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


def mixed_mask(rng):
    m = (rng.uniform(size=(NLAT, NLON)) < 0.6).astype(np.int64)
    m[:, 28:34] = 0                                 # an ocean basin
    m[8:10, 2:7] = 0
    m[0, 3:22] = 1                                  # land on both pole rows: the clipped row makes a pole cell its own neighbour
    m[-1, 6:30] = 1
    m[4:7, 10:15] = 1                               # the bare block (below) is land
    return m


def seam_mask(rng):
    """Land in columns 0 and NLON-1 on the same rows, among them both pole rows: the four corners are land."""
    m = (rng.uniform(size=(NLAT, NLON)) < 0.45).astype(np.int64)
    m[:, 12:20] = 0
    rows = [0, 1, 4, 5, 9, 13, 14, NLAT - 2, NLAT - 1]
    m[rows, 0] = 1
    m[rows, -1] = 1
    m[[4, 13], 1] = 0                               # seam cells whose only east-west land neighbour lies across the seam
    m[[4, 13], -2] = 0
    m[[0, NLAT - 1], 1:4] = 1
    m[[0, NLAT - 1], -4:-1] = 1
    return m


def case_mixed(rng):
    land = mixed_mask(rng)
    L = rng.uniform(0.0, 0.4, (20, 2, NLAT, NLON)) * (land == 1)
    L[:, :, 4:7, 10:15] = 0.0                       # bare land: alpha NaN there, Bray-Curtis 1 beside it
    L[3:9, :, 12:16, 0:9] = 0.0                     # some species exactly absent
    L[15, :, :, 20:] = 0.0
    return land, L


def case_seam(rng):
    land = seam_mask(rng)
    return land, rng.uniform(0.0, 0.2, (3, 8, NLAT, NLON)) * (land == 1)


def case_single(rng):
    land = mixed_mask(rng)
    return land, rng.uniform(0.05, 1.0, (1, 1, NLAT, NLON)) * (land == 1)


def case_nonfinite(rng):
    land = mixed_mask(rng)
    land[10:14, 16:24] = 1
    L = rng.uniform(-0.2, 0.5, (4, 2, NLAT, NLON))  # negative entries everywhere (clamped), ocean cells carry values too
    L[:, :, 4:7, 10:15] = 0.0
    L[1, 0, 11, 18] = np.nan                        # on land, with land neighbours on all sides
    L[2, 1, 12, 21] = np.inf
    L[0, 1, 15, 3] = np.nan
    L[3, 0, 2, 8] = np.inf
    L[1, 1, 0, 5] = np.nan                          # on a pole row
    return land, L


def case_noland(rng):
    return np.zeros((NLAT, NLON), dtype=np.int64), rng.uniform(0.0, 0.5, (3, 1, NLAT, NLON))


def case_wide(rng):
    land = mixed_mask(rng)
    L = rng.uniform(0.0, 0.1, (64, 1, NLAT, NLON)) * (land == 1)
    L[40:, :, 0:9, :] = 0.0
    return land, L


CASES = {"mixed": case_mixed, "seam": case_seam, "single": case_single, "nonfinite": case_nonfinite, "noland": case_noland,
         "wide": case_wide}


def rounding_margin(x, decimals=4):
    """Distance of x from the nearest value at which its `decimals`-digit rounding flips."""
    y = abs(x) * 10.0 ** decimals
    return abs((y - np.floor(y)) - 0.5) / 10.0 ** decimals


def run_case(name, div):
    rng = np.random.default_rng(sum(map(ord, "diversity_" + name)))
    land, stack = CASES[name](rng)
    lat = np.linspace(-90.0, 90.0, NLAT)
    lat_mesh = np.meshgrid(np.linspace(0.0, 360.0, NLON), lat)[1]
    eco = types.SimpleNamespace(pop=types.SimpleNamespace(LAI_layers_SK=stack))
    with np.errstate(all="ignore"):
        L_s, H, W = div._get_species_lai_SK(eco)
        alpha = div.compute_alpha_eff_map(L_s, land)
        bc = div.compute_local_bray_curtis(L_s, land)
        wh = div.compute_whittaker_beta(L_s, land, lat_mesh)
    assert (H, W) == (NLAT, NLON) and np.array_equal(wh["alpha_map"], alpha, equal_nan=True)
    summary = np.array([wh["alpha_mean"], wh["gamma_eff"], wh["beta_whittaker"]])
    for k, x in zip(("alpha_mean", "gamma_eff", "beta_whittaker"), summary):
        assert not np.isfinite(x) or x > 1e11 or rounding_margin(x) > 1e-9, f"{name}: {k} = {x!r} sits on a rounding boundary"
    meta = {"case": name, "nlat": NLAT, "nlon": NLON, "n_species": int(stack.shape[0]), "n_layers": int(stack.shape[1])}
    np.savez_compressed(os.path.join(OUT, f"diversity_{name}_{NLAT}x{NLON}.npz"), stack=stack, land_mask=land.astype(np.int8), lat=lat,
                        L_s=L_s, alpha_map=alpha, bc_local=bc, summary=summary, meta=json.dumps(meta))
    land_b = land == 1
    print(f"{name}: S={stack.shape[0]} K={stack.shape[1]} land {int(land_b.sum())} alpha NaN on land {int(np.isnan(alpha[land_b]).sum())} "
          f"bc NaN on land {int(np.isnan(bc[land_b]).sum())} bc == 1 {int(np.sum(bc == 1.0))} summary {summary}")


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reference", default=os.path.join(HERE, "..", "..", "reference"))
    ap.add_argument("cases", nargs="*", default=list(CASES))
    a = ap.parse_args()
    sys.path.insert(0, os.path.abspath(a.reference))
    os.environ.setdefault("MPLBACKEND", "Agg")
    from pygcm.ecology import diversity as div
    for name in a.cases:
        run_case(name, div)


if __name__ == "__main__":
    main()
