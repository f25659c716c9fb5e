"""Regenerate tests/golden/hydronet_*.npz from the reference's network generator (scripts/generate_hydrology_maps.py:
pit_fill, compute_flow_to_index, identify_lakes, compute_lake_outlets, topo_sort_flow_order).

Needs a checkout of the reference project (default ../reference next to this repository, or --reference DIR); netCDF4 is not
needed.  Each golden holds the case's inputs (land mask, eps, max_iters; the elevation itself only where neither
qingdai_amd.topography nor a builder of tests/hydronet_cases.py regenerates it bit for bit), the reference's outputs (the
filled elevation over land only: ocean cells are never changed), the number of pit-fill sweeps the reference ran, and the spherical_distance tables as the reference computes them
(scalar np.deg2rad / np.cos per cell pair).
"""
import argparse
import os
import sys

import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(HERE)
OUT = os.path.join(ROOT, "tests", "golden")


def ref_tables(grid):
    """lat1 = np.deg2rad(grid.lat[j1]) ... np.cos(0.5 * (lat1 + lat2)), one numpy scalar at a time, as spherical_distance does."""
    n_lat, n_lon = grid.n_lat, grid.n_lon
    lat = np.array([np.deg2rad(grid.lat[j]) for j in range(n_lat)], dtype=np.float64)
    lon = np.array([np.deg2rad(grid.lon[i]) for i in range(n_lon)], dtype=np.float64)
    cos_pair = np.zeros((n_lat, 3), dtype=np.float64)
    for j in range(n_lat):
        for k, dj in enumerate((-1, 0, 1)):
            if 0 <= j + dj < n_lat:
                cos_pair[j, k] = np.cos(0.5 * (np.deg2rad(grid.lat[j]) + np.deg2rad(grid.lat[j + dj])))
    return lat, lon, cos_pair


def run_case(ghm, grid_cls, name, n_lat, n_lon, land, elev, elev_src, max_iters, eps=1e-3):
    grid = grid_cls(n_lat, n_lon)
    land = np.asarray(land).astype(np.uint8)
    elev = np.asarray(elev, dtype=float)
    n_land = int((land == 1).sum())
    calls = [0]
    nb = ghm.neighbors_d8

    def counting(*a):
        calls[0] += 1
        return nb(*a)

    ghm.neighbors_d8 = counting                        # pit_fill asks once per land cell and sweep
    try:
        ef = ghm.pit_fill(elev.copy(), land, max_iters=max_iters, eps=eps)
    finally:
        ghm.neighbors_d8 = nb
    assert calls[0] % n_land == 0
    sweeps = calls[0] // n_land
    ft = ghm.compute_flow_to_index(grid, ef, land)
    lm, lid, nl = ghm.identify_lakes(ft, land)
    outlet = ghm.compute_lake_outlets(grid, ef, lm, lid, land) if nl > 0 else np.zeros(0, np.int32)
    order = ghm.topo_sort_flow_order(ft, land)
    assert np.array_equal(ef[land != 1], elev[land != 1])
    lat, lon, cos_pair = ref_tables(grid)
    out = dict(shape=np.array([n_lat, n_lon]), eps=np.float64(eps), max_iters=np.int64(max_iters), elev_src=np.array(elev_src),
               land_mask=land, ef_land=ef[land == 1], flow_to_index=ft.astype(np.int32), flow_order=order.astype(np.int32),
               lake_mask=lm.astype(np.uint8), lake_id=lid.astype(np.int32), lake_outlet_index=np.asarray(outlet, np.int32),
               n_lakes=np.int64(nl), sweeps=np.int64(sweeps), lat_rad=lat, lon_rad=lon, cos_pair=cos_pair)
    if elev_src == "stored":
        out["elevation"] = elev
    path = os.path.join(OUT, f"hydronet_{name}.npz")
    np.savez_compressed(path, **out)
    n_out = int(np.sum(np.asarray(outlet) >= 0))
    print(f"{path}: {sweeps} sweeps, {nl} lakes ({n_out} with a land outlet), {os.path.getsize(path) / 1024:.0f} KiB")


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reference", default=os.path.join(ROOT, "..", "reference"))
    a = ap.parse_args()
    ref = os.path.abspath(a.reference)
    if not os.path.isdir(os.path.join(ref, "pygcm")):
        sys.exit(f"reference checkout not found at {ref}")
    sys.path.insert(0, ref)
    sys.path.insert(1, ROOT)
    sys.path.insert(2, os.path.join(ROOT, "tests"))
    from pygcm.grid import SphericalGrid
    from pygcm import topography as rtopo
    from scripts import generate_hydrology_maps as ghm
    import qingdai_amd as qa
    from qingdai_amd import topography as qtopo
    import hydronet_cases as hc

    def procedural(n_lat, n_lon):
        g = SphericalGrid(n_lat, n_lon)
        land = rtopo.create_land_sea_mask(g)
        elev = rtopo.generate_elevation_map(g, seed=42)
        mine = qtopo.generate_elevation_map(qa.SphericalGrid(n_lat, n_lon), seed=42)
        assert np.array_equal(land, qtopo.create_land_sea_mask(qa.SphericalGrid(n_lat, n_lon)))
        return land, elev, ("procedural" if np.array_equal(elev.view(np.uint64), mine.view(np.uint64)) else "stored")

    for n_lat, n_lon in ((19, 36), (73, 144)):
        land, _, _ = procedural(n_lat, n_lon)
        run_case(ghm, SphericalGrid, f"zero_{n_lat}x{n_lon}", n_lat, n_lon, land, np.zeros((n_lat, n_lon)), "zero", 200)
    for n_lat, n_lon in ((73, 144), (181, 360)):
        land, elev, src = procedural(n_lat, n_lon)
        for it in (200, 1, 3):
            run_case(ghm, SphericalGrid, f"proc_{n_lat}x{n_lon}_it{it}", n_lat, n_lon, land, elev, src, it)
    land, elev = hc.valley_field(25, 400, 5)
    run_case(ghm, SphericalGrid, "valley_25x400", 25, 400, land, elev, "stored", 40)
    land, elev = hc.inland_field(37, 72, 6)
    run_case(ghm, SphericalGrid, "inland_37x72", 37, 72, land, elev, "stored", 2)
    # the hostile-terrain cases of tests/hydronet_cases.py: the builder regenerates the field, so none is stored
    for name, build in hc.GOLDENED.items():
        land, elev, eps, max_iters = build()
        again = build()[1]
        assert np.array_equal(elev.view(np.uint64), again.view(np.uint64))
        run_case(ghm, SphericalGrid, name, *elev.shape, land, elev, f"case:{name}", max_iters, eps=eps)


if __name__ == "__main__":
    main()
