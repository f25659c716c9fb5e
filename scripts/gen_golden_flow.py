"""Regenerate tests/golden/flow_*.npz from the reference's SphericalGrid.vorticity and SphericalGrid.divergence.

Needs a checkout of the reference project (default ../reference next to this repository, or --reference DIR).  Each golden holds
the case's inputs (the shape, the winds u and v, the planet radius the reference used) and the reference's two results, zeta and
delta -- nothing else, on small grids.  tests/test_flow_cpu.py holds flow.vortdiv_reference to them bit for bit on the rows
1 .. n_lat - 2 (on the pole rows the reference divides by a capped cosine of 1e-6 and the flow lane has a rule of its own).
"""
import argparse
import os
import sys

import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(HERE)
OUT = os.path.join(ROOT, "tests", "golden")

# name -> (n_lat, n_lon, kind): seeded normal winds over a zonal jet; magnitudes over eight orders; a solid-body rotation
CASES = {"normal_3x4": (3, 4, "normal"), "normal_5x4": (5, 4, "normal"), "normal_19x36": (19, 36, "normal"), "normal_9x45": (9, 45, "normal"),
         "wide_7x35": (7, 35, "wide"), "solid_19x36": (19, 36, "solid"), "normal_25x48": (25, 48, "normal")}


def winds(n_lat, n_lon, kind):
    r = np.random.default_rng(n_lat * 10000 + n_lon)
    lat = np.deg2rad(np.linspace(-90, 90, n_lat))[:, None]
    if kind == "solid":
        return 30.0 * np.cos(lat) * np.ones((n_lat, n_lon)), np.zeros((n_lat, n_lon))
    u, v = 8.0 * np.cos(lat) + 10.0 * r.normal(size=(n_lat, n_lon)), 5.0 * r.normal(size=(n_lat, n_lon))
    if kind == "wide":
        u, v = u * 10.0 ** r.integers(-4, 5, size=u.shape), v * 10.0 ** r.integers(-4, 5, size=v.shape)
    return u, v


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reference", default=os.path.join(ROOT, "..", "reference"))
    a = ap.parse_args()
    ref = os.path.abspath(a.reference)
    if not os.path.isdir(os.path.join(ref, "pygcm")):
        sys.exit(f"reference checkout not found at {ref}")
    sys.path.insert(0, ref)
    from pygcm import constants
    from pygcm.grid import SphericalGrid
    for name, (n_lat, n_lon, kind) in CASES.items():
        g = SphericalGrid(n_lat, n_lon)
        u, v = winds(n_lat, n_lon, kind)
        with np.errstate(all="ignore"):
            zeta, delta = g.vorticity(u, v), g.divergence(u, v)
        path = os.path.join(OUT, f"flow_{name}.npz")
        np.savez_compressed(path, shape=np.array([n_lat, n_lon]), radius=np.float64(constants.PLANET_RADIUS), u=u, v=v, zeta=zeta, delta=delta)
        print(f"{path}: {os.path.getsize(path) / 1024:.1f} KiB")


if __name__ == "__main__":
    main()
