#!/usr/bin/env python3
"""Drop-in for the reference's `python -m scripts.generate_hydrology_maps` (P014): the offline river network -- pit fill,
D8 flow directions, lakes, lake outlets and the topological flow order -- built on the MI355X (qingdai_amd.hydronet) and
written to a NetCDF with the reference's dimensions, variables and attributes.  Same options and the same fallback: without a
readable --topo the procedural seed-42 mask with zero elevation."""
import argparse
import os
import sys
import time

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))

import numpy as np  # noqa: E402

from qingdai_amd import topography as topo  # noqa: E402
from qingdai_amd.grid import SphericalGrid  # noqa: E402
from qingdai_amd.hydronet import generate_network, write_network  # noqa: E402


def main(argv=None):
    ap = argparse.ArgumentParser(description="Generate P014 hydrology routing network NetCDF (on the device).")
    ap.add_argument("--topo", type=str, default=os.getenv("QD_TOPO_NC", ""),
                    help="Path to topography NetCDF (contains land_mask and optional elevation). If empty, fallback is used.")
    ap.add_argument("--out", type=str, default="data/hydrology_network.nc", help="Output NetCDF path")
    ap.add_argument("--nlat", type=int, default=121, help="Grid latitude count if fallback topography is used")
    ap.add_argument("--nlon", type=int, default=240, help="Grid longitude count if fallback topography is used")
    ap.add_argument("--pit-eps", type=float, default=1e-3, help="Pit filling epsilon")
    ap.add_argument("--pit-iters", type=int, default=200, help="Max iterations for pit filling")
    a = ap.parse_args(argv)
    grid = SphericalGrid(a.nlat, a.nlon)
    elevation = None
    if a.topo and os.path.exists(a.topo):
        try:
            elevation, land_mask, _alb, _fric = topo.load_topography_from_netcdf(a.topo, grid)
            print(f"[HydroNet] Loaded topography from '{a.topo}'.")
        except Exception as e:      # noqa: BLE001
            print(f"[HydroNet] Failed to load '{a.topo}': {e}\nFalling back to procedural mask.")
            land_mask, elevation = topo.create_land_sea_mask(grid), None
    else:
        print("[HydroNet] No topography specified or file missing. Using fallback.")
        land_mask = topo.create_land_sea_mask(grid)
    if elevation is None:
        elevation = np.zeros_like(grid.lat_mesh, dtype=float)
    print(f"[HydroNet] Pit filling elevation over land (iters={a.pit_iters}, eps={a.pit_eps}), D8 flow directions, lakes and "
          f"the topological flow order on the device...")
    t0 = time.perf_counter()
    net = generate_network(grid, land_mask.astype(np.uint8), elevation.astype(float), eps=a.pit_eps, max_iters=a.pit_iters)
    print(f"[HydroNet] Built in {time.perf_counter() - t0:.2f} s: {net['sweeps']} pit-fill sweeps, {net['n_lakes']} lakes.")
    print(f"[HydroNet] Writing network to '{a.out}'...")
    write_network(a.out, grid, net)
    print("[HydroNet] Done.")
    return 0


if __name__ == "__main__":
    sys.exit(main())
