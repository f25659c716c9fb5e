"""Regenerate tests/golden/topogen_<case>_<shape>.npz from the reference's procedural topography (pygcm/topography.py:
generate_elevation_map, create_land_sea_mask_from_elevation, generate_base_properties).

Needs a checkout of the reference project (default ../reference next to this repository, or --reference DIR) and scipy.  Each
golden holds the case (shape, seed, parameters as JSON, target land fraction), the reference's centres and amplitudes (recorded
while it runs), its elevation, sea level, mask, base albedo and friction, and three
margins that say how well-conditioned the case is: elev_gap, the smallest non-zero |elevation - sea level|, and the two
cumulative-weight margins around the quantile index, cw[idx] - q and q - cw[idx - 1].  The noise is not stored:
qingdai_amd.topogen.draw regenerates it.
"""
import argparse
import json
import os
import sys

import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(HERE)
OUT = os.path.join(ROOT, "tests", "golden")

CLI = {"N_CONTINENTS": 3, "CONTINENT_SIGMA_DEG": 30.0, "CONTINENT_SHAPE_P": 2.0, "CONT_MIN_DIST_DEG": 40.0, "W_VLF": 0.35,
       "FBM_OCTAVES": 5, "HURST_H": 0.8, "W1": 1.0, "W3": 0.6, "SCALE_M": 4500.0}
WIDE = {"N_CONTINENTS": 6, "CONTINENT_SIGMA_DEG": 18.0, "CONTINENT_SHAPE_P": 1.5, "CONT_MIN_DIST_DEG": 55.0, "W_VLF": 0.5,
        "FBM_OCTAVES": 3, "HURST_H": 0.6, "W1": 0.8, "W3": 0.9, "SCALE_M": 3000.0}
CROWDED = {"N_CONTINENTS": 12, "CONT_MIN_DIST_DEG": 90.0, "FBM_OCTAVES": 7}
MAIN = (("default", {}, 42, 0.29), ("cli", CLI, 42, 0.40), ("wide", WIDE, 7, 0.55), ("crowded", CROWDED, 3, 0.10))
DEGENERATE = (("flat", {"W1": 0.0, "W3": 0.0}, 42, 0.29), ("nocont", {"N_CONTINENTS": 0}, 42, 0.29),
              ("nooct", {"FBM_OCTAVES": 0}, 42, 0.29))
SHAPES = ((13, 24), (19, 36), (37, 72))


def margins(elev, grid, sea, q):
    """the reference's _weighted_quantile, step by step, for the distances of its decision from the next one"""
    w = np.maximum(np.cos(np.deg2rad(grid.lat_mesh)), 0.0).ravel()
    v = elev.ravel()
    order = np.argsort(v)
    vs, cw = v[order], np.cumsum(w[order])
    cw /= cw[-1]
    idx = int(np.clip(np.searchsorted(cw, q, side="left"), 0, v.size - 1))
    assert float(vs[idx]) == sea
    above = float(cw[idx] - q)
    below = float(q - cw[idx - 1]) if idx > 0 else float(q)
    gap = np.abs(elev - sea)
    gap = gap[gap > 0.0]
    return (float(gap.min()) if gap.size else 0.0), above, below


class Recorder:
    """The reference's generator with the amplitudes (its last vector uniform draw) kept; the centres themselves are read off
    the arguments of _great_circle_distance_rad, which the reference calls once per continent."""

    def __init__(self, rng, log):
        self.rng, self.log = rng, log

    def uniform(self, lo, hi, size=None):
        out = self.rng.uniform(lo, hi, size=size)
        if size is not None:
            self.log["amps"] = np.array(out, dtype=float)
        return out

    def standard_normal(self, size=None):
        return self.rng.standard_normal(size=size)


def run_case(rtopo, grid_cls, name, shape, params, seed, frac):
    grid = grid_cls(*shape)
    log = {"amps": np.zeros(0), "lats": [], "lons": []}
    make_rng, dist = rtopo._rng, rtopo._great_circle_distance_rad

    def recording_dist(lat, lon, lat0, lon0):
        log["lats"].append(float(lat0))
        log["lons"].append(float(lon0))
        return dist(lat, lon, lat0, lon0)

    rtopo._rng = lambda s: Recorder(make_rng(s), log) if int(s) == int(seed) else make_rng(s)
    rtopo._great_circle_distance_rad = recording_dist
    try:
        elev = rtopo.generate_elevation_map(grid, seed=seed, params=dict(params))
    finally:
        rtopo._rng, rtopo._great_circle_distance_rad = make_rng, dist
    assert np.array_equal(elev, rtopo.generate_elevation_map(grid, seed=seed, params=dict(params)))     # recording changed nothing
    n_cont = int(params.get("N_CONTINENTS", 3))
    lats, lons = np.array(log["lats"], dtype=float), np.array(log["lons"], dtype=float)
    amps = log["amps"] if n_cont else np.zeros(0)
    assert lats.shape == lons.shape == amps.shape == (n_cont,)
    mask, sea = rtopo.create_land_sea_mask_from_elevation(elev, grid, target_land_frac=frac)
    alb, fric = rtopo.generate_base_properties(mask, elevation=elev, grid=grid)
    gap, above, below = margins(elev, grid, sea, 1.0 - float(frac))
    path = os.path.join(OUT, f"topogen_{name}_{shape[0]}x{shape[1]}.npz")
    np.savez_compressed(path, shape=np.array(shape), seed=np.int64(seed), params=np.array(json.dumps(params)),
                        target_land_frac=np.float64(frac), cont_lats=lats, cont_lons=lons, cont_amps=amps, elevation=elev,
                        sea_level_m=np.float64(sea), land_mask=mask.astype(np.uint8), base_albedo=alb, friction=fric,
                        elev_gap=np.float64(gap), cw_above=np.float64(above), cw_below=np.float64(below))
    print(f"{path}: sea {sea:.3f} m, land cells {int(mask.sum())}, elev_gap {gap:.3e} m, cw margins {above:.2e} / {below:.2e}, "
          f"{os.path.getsize(path) / 1024:.0f} KiB")


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reference", default=os.path.join(ROOT, "..", "reference"))
    a = ap.parse_args()
    ref = os.path.abspath(a.reference)
    if not os.path.isdir(os.path.join(ref, "pygcm")):
        sys.exit(f"reference checkout not found at {ref}")
    sys.path.insert(0, ref)
    sys.path.insert(1, ROOT)
    from pygcm.grid import SphericalGrid
    from pygcm import topography as rtopo
    for shape in SHAPES:
        for name, params, seed, frac in MAIN:
            run_case(rtopo, SphericalGrid, name, shape, params, seed, frac)
    for name, params, seed, frac in DEGENERATE:
        run_case(rtopo, SphericalGrid, name, (19, 36), params, seed, frac)


if __name__ == "__main__":
    main()
