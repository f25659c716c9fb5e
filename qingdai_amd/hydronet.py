"""
qingdai_amd/hydronet.py -- the offline river network (P014, scripts/generate_hydrology_maps.py) built on the device.

The reference generator is five pure-Python loops (generate_hydrology_maps.py:84-311): a Gauss-Seidel pit fill, D8 steepest
descent, lake labelling, lake outlets and Kahn's topological order.  `generate_network` runs all five in qd_hydronet_build
(qingdai_amd/csrc/qd_hydronet.hip) and returns the reference's arrays bit for bit; `write_network` writes them with the
reference's dimensions, variables and attributes, ready for `RiverRouting`.

The spherical_distance operands that need NumPy's own rounding -- np.deg2rad of the axes and the cosine of every row pair --
are computed here (`host_tables`), exactly as the reference writes them; the rest of the distance is IEEE f64 on the device.
"""
from __future__ import annotations

import numpy as np

from ._lib import OUT
from .params import PLANET_RADIUS

NETWORK_KEYS = ("land_mask", "elevation_filled", "flow_to_index", "flow_order", "lake_mask", "lake_id", "lake_outlet_index")
INDEXING = "row-major (i=lon index, j=lat index), idx=j*n_lon+i"


def host_tables(grid):
    """-> (lat_rad [n_lat], lon_rad [n_lon], cos_pair [n_lat, 3]): lat1 = np.deg2rad(grid.lat[j1]) etc. and
    np.cos(0.5 * (lat1 + lat2)) for the neighbour rows j + dj, dj = -1, 0, 1 (generate_hydrology_maps.py:64-81).
    The entries past the poles are 0 and never read."""
    lat = np.deg2rad(np.asarray(grid.lat, dtype=np.float64))
    lon = np.deg2rad(np.asarray(grid.lon, dtype=np.float64))
    n_lat = lat.size
    cos_pair = np.zeros((n_lat, 3), dtype=np.float64)
    for k, dj in enumerate((-1, 0, 1)):
        j = np.arange(max(0, -dj), min(n_lat, n_lat - dj))
        cos_pair[j, k] = np.cos(0.5 * (lat[j] + lat[j + dj]))
    return np.ascontiguousarray(lat), np.ascontiguousarray(lon), cos_pair


class HydroNetError(RuntimeError):
    pass


def generate_network(grid, land_mask, elevation=None, eps=1e-3, max_iters=200, dev=None):
    """The reference generator's five routines on the device -> dict with the reference's names and dtypes:
    land_mask u1, elevation_filled f64, flow_to_index i8, flow_order i8, lake_mask u1, lake_id i4, lake_outlet_index i4
    (empty without lakes), plus 'n_lakes' and 'sweeps' (pit-fill sweeps run).

    elevation None is the reference driver's zeros.  `dev`: a whole-globe Device of the grid (default: the grid's own, else a
    fresh one).  Raises HydroNetError for what the device refuses (bad shape, land_mask values other than 0 / 1, non-finite
    elevation on land or next to it)."""
    n_lat, n_lon = int(grid.n_lat), int(grid.n_lon)
    land = np.ascontiguousarray(np.asarray(land_mask).astype(np.uint8))
    if land.shape != (n_lat, n_lon):
        raise HydroNetError(f"land_mask shape {land.shape} != grid shape {(n_lat, n_lon)}")
    if elevation is None:
        elev = np.zeros((n_lat, n_lon), dtype=np.float64)
    else:
        elev = np.ascontiguousarray(np.asarray(elevation, dtype=np.float64))
        if elev.shape != (n_lat, n_lon):
            raise HydroNetError(f"elevation shape {elev.shape} != grid shape {(n_lat, n_lon)}")
    if dev is None:
        dev = getattr(grid, "_device", None)
        if dev is None:
            from .device import Device
            dev = Device(grid)
    lat, lon, cos_pair = host_tables(grid)
    cells = n_lat * n_lon
    ef = np.zeros((n_lat, n_lon), dtype=np.float64)
    ft = np.zeros((n_lat, n_lon), dtype=np.int32)
    order = np.zeros(cells, dtype=np.int32)
    lmask = np.zeros((n_lat, n_lon), dtype=np.uint8)
    lid = np.zeros((n_lat, n_lon), dtype=np.int32)
    outlet = np.zeros(cells, dtype=np.int32)
    n_land, nl = dev.call("qd_hydronet_build", n_lat, n_lon, land, elev, eps, max_iters, lat, lon, cos_pair, PLANET_RADIUS, ef, ft, order,
                          lmask, lid, outlet, cells, OUT, OUT, error=HydroNetError)
    return {"land_mask": land, "elevation_filled": ef, "flow_to_index": ft.astype(np.int64),
            "flow_order": order[:n_land].astype(np.int64), "lake_mask": lmask, "lake_id": lid,
            "lake_outlet_index": outlet[:nl].copy(), "n_lakes": nl, "sweeps": dev.call("qd_hydronet_sweeps", OUT)}


def write_network(path, grid, net, auto=False):
    """The generator's NetCDF (generate_hydrology_maps.py:329-362; the driver's auto path run_simulation.py:1098-1123 when
    `auto`): dims lat / lon / n_land (/ n_lakes when > 0), f4 axes, u1 masks (i1 in classic NetCDF), f4 filled elevation,
    i4 indices, and the reference's global attributes."""
    from .ncio import write_nc
    n_lat, n_lon = int(grid.n_lat), int(grid.n_lon)
    land = np.asarray(net["land_mask"]).astype(np.uint8)
    n_lakes = int(np.max(net["lake_id"])) if np.asarray(net["lake_id"]).size else 0
    dims = {"lat": n_lat, "lon": n_lon, "n_land": int((land == 1).sum())}
    if n_lakes > 0:
        dims["n_lakes"] = n_lakes
    v = {"lat": ("f4", ("lat",), np.asarray(grid.lat).astype(np.float32)),
         "lon": ("f4", ("lon",), np.asarray(grid.lon).astype(np.float32)),
         "land_mask": ("u1", ("lat", "lon"), land),
         "elevation_filled": ("f4", ("lat", "lon"), np.asarray(net["elevation_filled"]).astype(np.float32)),
         "flow_to_index": ("i4", ("lat", "lon"), np.asarray(net["flow_to_index"]).astype(np.int32)),
         "flow_order": ("i4", ("n_land",), np.asarray(net["flow_order"]).astype(np.int32)),
         "lake_mask": ("u1", ("lat", "lon"), np.asarray(net["lake_mask"]).astype(np.uint8)),
         "lake_id": ("i4", ("lat", "lon"), np.asarray(net["lake_id"]).astype(np.int32))}
    if n_lakes > 0 and net.get("lake_outlet_index") is not None:
        v["lake_outlet_index"] = ("i4", ("n_lakes",), np.asarray(net["lake_outlet_index"]).astype(np.int32))
    if auto:
        attrs = {"title": "Qingdai Hydrology Network (auto-generated)", "indexing": INDEXING, "projection": "latlon",
                 "created_by": "scripts/run_simulation.py (auto)"}
    else:
        attrs = {"title": "Qingdai Hydrology Network", "indexing": INDEXING, "projection": "latlon",
                 "created_by": "scripts/generate_hydrology_maps.py",
                 "notes": "D8 routing; simple pit filling; lakes are terminal sinks; outlets not discovered in v1"}
    write_nc(path, dims, v, attrs)
