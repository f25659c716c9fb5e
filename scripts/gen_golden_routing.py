"""Regenerate tests/golden/routing_*.npz from the reference's RiverRouting (pygcm/routing.py).

Needs a checkout of the reference project (default ../reference next to this repository, or --reference DIR);
netCDF4 is not needed: the network goes to RiverRouting through an in-memory stand-in for its Dataset.

Each golden holds the network variables (net_*), the grid shape, dt and dt_hydro, the base fields of the
per-step inputs (step k: R = R0 + k R1, P = P0 + k P1, E = E0, all f64), every event's diagnostics, and the
final buffer and t_accum.
"""
import argparse
import os
import sys
import tempfile

import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))
OUT = os.path.join(HERE, "..", "tests", "golden")


class _Var:
    def __init__(self, a):
        self.a = a

    def __getitem__(self, k):
        return self.a[k]


class _MemDataset:
    store = {}

    def __init__(self, path, mode="r"):
        self.variables = {k: _Var(v) for k, v in self.store[path].items()}

    def __enter__(self):
        return self

    def __exit__(self, *a):
        return False


def _smooth_field(rng, n_lat, n_lon, k=4):
    lat = np.linspace(-np.pi / 2, np.pi / 2, n_lat)[:, None]
    lon = np.linspace(0, 2 * np.pi, n_lon)[None, :]
    f = np.zeros((n_lat, n_lon))
    for _ in range(k):
        a, b, c, d = rng.uniform(0.5, 4.0), rng.integers(1, 6), rng.uniform(0, 2 * np.pi), rng.uniform(0, 2 * np.pi)
        f += rng.uniform(200, 800) * np.sin(a * lat + c) * np.cos(b * lon + d)
    return f + rng.normal(0, 40.0, (n_lat, n_lon))


def procedural_network(ghm, grid, seed, pit_iters):
    from pygcm.topography import create_land_sea_mask
    land = create_land_sea_mask(grid)
    rng = np.random.default_rng(seed)
    elev = np.where(land == 1, 1000.0 + _smooth_field(rng, grid.n_lat, grid.n_lon), 0.0)
    ef = ghm.pit_fill(elev.copy(), land, max_iters=pit_iters, eps=1e-3)
    ft = ghm.compute_flow_to_index(grid, ef, land)
    order = ghm.topo_sort_flow_order(ft, land)
    lm, lid, nl = ghm.identify_lakes(ft, land)
    v = dict(land_mask=land.astype(np.uint8), flow_to_index=ft.astype(np.int64), flow_order=order.astype(np.int64),
             lake_mask=lm, lake_id=lid)
    if nl > 0:
        v["lake_outlet_index"] = ghm.compute_lake_outlets(grid, ef, lm, lid, land).astype(np.int64)
    return v


def adversarial_network(n_lat, n_lon, seed, variant):
    """Hand-made edge cases: downstream into ocean cells, into earlier-processed cells, into the cell itself, out of the
    order; lakes with every kind of outlet."""
    rng = np.random.default_rng(seed)
    n = n_lat * n_lon
    land = np.zeros((n_lat, n_lon), np.uint8)
    land[2:n_lat - 2, 3:n_lon - 3] = 1
    land[n_lat // 2, n_lon // 2:n_lon // 2 + 3] = 0               # an inland ocean strip
    lf = land.ravel() == 1
    idx = np.arange(n)
    ft = np.full(n, -1, np.int64)
    land_idx = idx[lf]
    # mostly "next cell to the east", with adversarial exceptions
    ft[land_idx] = land_idx + 1
    pick = rng.choice(land_idx, size=land_idx.size // 6, replace=False)
    kinds = rng.integers(0, 5, pick.size)
    ocean_idx = idx[~lf]
    ft[pick[kinds == 0]] = rng.choice(ocean_idx, (kinds == 0).sum())          # into an ocean cell
    ft[pick[kinds == 1]] = pick[kinds == 1] - 2 * n_lon                        # upstream / earlier
    ft[pick[kinds == 2]] = pick[kinds == 2]                                    # itself
    ft[pick[kinds == 3]] = -1                                                  # ocean sink
    ft[pick[kinds == 4]] = pick[kinds == 4] + n_lon                            # a row further down (later)
    ft = np.where((ft < 0) | (ft >= n), -1, ft)
    v = dict(land_mask=land, flow_to_index=ft.reshape(n_lat, n_lon))
    # lakes: ids 1..6 on small blocks
    lake_mask = np.zeros((n_lat, n_lon), np.int32)
    lake_id = np.zeros((n_lat, n_lon), np.int32)
    blocks = [(4, 5), (4, 12), (7, 8), (9, 20), (12, 6), (13, 25)]
    for k, (j, i) in enumerate(blocks, start=1):
        lake_mask[j:j + 2, i:i + 2] = 1
        lake_id[j:j + 2, i:i + 2] = k
    lake_mask[5, 30] = 1                       # a lake cell without an id: its mass vanishes
    lake_mask[10, 30] = -1                     # counted by the P-E update, not routed as a lake
    lake_id[10, 30] = 2
    v["lake_mask"], v["lake_id"] = lake_mask, lake_id
    if variant == "index":
        v["flow_order"] = np.concatenate([land_idx[::-1][: land_idx.size // 3], land_idx[: 2 * land_idx.size // 3]])
        v["flow_order"] = np.unique(v["flow_order"])[rng.permutation(np.unique(v["flow_order"]).size)]
        # outlets: ocean sink, later land cell, earlier land cell, ocean cell, beyond the grid, a land cell
        v["lake_outlet_index"] = np.array([-1, 14 * n_lon + 28, 3 * n_lon + 4, n_lat // 2 * n_lon + n_lon // 2, n + 5,
                                           11 * n_lon + 10], np.int64)
    elif variant == "ij":
        # no flow_order: the fallback (ascending land cells); outlets as (i, j)
        v["lake_outlet_i"] = np.array([28, 4, 0, 10, 15, 9], np.int64)
        v["lake_outlet_j"] = np.array([14, 3, 0, 11, 8, 6], np.int64)
    elif variant == "short":
        # a short outlet array: n_lakes coerced to 3; lake ids 4..6 are kept off lake cells (the reference would fail there)
        lake_mask[lake_id >= 4] = 0
        v["lake_mask"] = lake_mask
        v["lake_outlet_index"] = np.array([-1, 14 * n_lon + 28, 6 * n_lon + 9], np.int64)
    elif variant == "store":
        pass                                   # no outlets at all: every lake stores its inflow
    return v


def run_case(RR, grid_cls, name, n_lat, n_lon, v, dt, dt_hydro_hours, nsteps, seed):
    rng = np.random.default_rng(seed + 1)
    grid = grid_cls(n_lat, n_lon)
    land = np.asarray(v["land_mask"]) > 0
    R0 = np.where(land, rng.uniform(0, 2e-5, (n_lat, n_lon)), np.nan)       # NaN runoff over ocean: masked by the network land
    R1 = np.where(land, rng.normal(0, 1e-6, (n_lat, n_lon)), 0.0)
    neg = land & (rng.random((n_lat, n_lon)) < 0.05)
    R0 = np.where(neg, -rng.uniform(0, 3e-5, (n_lat, n_lon)), R0)           # negative runoff on some land cells
    P0 = rng.uniform(0, 5e-5, (n_lat, n_lon))
    P1 = rng.normal(0, 1e-6, (n_lat, n_lon))
    E0 = rng.uniform(0, 4e-5, (n_lat, n_lon))
    with tempfile.NamedTemporaryFile(suffix=".nc") as f:
        _MemDataset.store[f.name] = {k: np.asarray(a) for k, a in v.items()}
        rr = RR(grid, f.name, dt_hydro_hours=dt_hydro_hours, diag=False)
    ev_step, ev_flow, ev_ocean, ev_err, ev_lake = [], [], [], [], []
    for k in range(nsteps):
        R, P, E = R0 + k * R1, P0 + k * P1, E0
        cache = rr._diag_cache
        rr.step(R, dt, precip_flux=P, evap_flux=E)
        if rr._diag_cache is not cache:
            d = rr.diagnostics()
            ev_step.append(k)
            ev_flow.append(d["flow_accum_kgps"])
            ev_ocean.append(d["ocean_inflow_kgps"])
            ev_err.append(d["mass_closure_error_kg"])
            ev_lake.append(d["lake_volume_kg"] if d["lake_volume_kg"] is not None else np.zeros(0))
    out = {f"net_{k}": np.asarray(a) for k, a in v.items()}
    out.update(shape=np.array([n_lat, n_lon]), dt=np.float64(dt), dt_hydro_hours=np.float64(dt_hydro_hours),
               nsteps=np.int64(nsteps), R0=R0, R1=R1, P0=P0, P1=P1, E0=E0, ev_step=np.array(ev_step, np.int64),
               ev_flow=np.array(ev_flow), ev_ocean=np.array(ev_ocean), ev_err=np.array(ev_err),
               ev_lake=np.array(ev_lake), n_lakes=np.int64(rr.n_lakes), buffer=rr.buffer_kg.copy(),
               t_accum=np.float64(rr.t_accum))
    path = os.path.join(OUT, f"routing_{name}.npz")
    np.savez_compressed(path, **out)
    print(f"{path}: {len(ev_step)} events, n_lakes={rr.n_lakes}, {os.path.getsize(path) / 1024:.0f} KiB")


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reference", default=os.path.join(HERE, "..", "..", "reference"))
    a = ap.parse_args()
    ref = os.path.abspath(a.reference)
    if not os.path.isdir(os.path.join(ref, "pygcm")):
        sys.exit(f"reference checkout not found at {ref}")
    sys.path.insert(0, ref)
    import pygcm.routing as prt
    from pygcm.grid import SphericalGrid
    from scripts import generate_hydrology_maps as ghm
    prt.Dataset = _MemDataset
    RR = prt.RiverRouting
    g37 = SphericalGrid(37, 72)
    g73 = SphericalGrid(73, 144)
    run_case(RR, SphericalGrid, "proc_37x72", 37, 72, procedural_network(ghm, g37, 42, 3), 900.0, 1.0, 10, 42)
    run_case(RR, SphericalGrid, "proc_73x144", 73, 144, procedural_network(ghm, g73, 42, 3), 1000.0, 1.0, 9, 43)
    for variant, seed in (("index", 7), ("ij", 8), ("short", 9), ("store", 10)):
        run_case(RR, SphericalGrid, f"adv_{variant}_19x36", 19, 36, adversarial_network(19, 36, seed, variant), 1000.0, 1.0, 9, seed)


if __name__ == "__main__":
    main()
