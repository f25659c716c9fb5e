"""Plain restatements of the network generator's rules (generate_hydrology_maps.py:64-311), for checks at sizes the goldens
do not reach: one Gauss-Seidel pit-fill sweep in Python, D8 in NumPy from the host tables, and the lakes, outlets and Kahn
order in Python.  Written from the rules, not from the reference's program text."""
from collections import deque

import numpy as np

from qingdai_amd.params import PLANET_RADIUS

DIRS = [(dj, di) for dj in (-1, 0, 1) for di in (-1, 0, 1) if (dj, di) != (0, 0)]


def case_inputs(z):
    """-> (grid shape, land_mask, elevation, eps, max_iters) of a hydronet golden."""
    import qingdai_amd as qa
    from qingdai_amd.topography import generate_elevation_map
    n_lat, n_lon = (int(x) for x in z["shape"])
    src = str(z["elev_src"])
    if src == "zero":
        elev = np.zeros((n_lat, n_lon))
    elif src == "procedural":
        elev = generate_elevation_map(qa.SphericalGrid(n_lat, n_lon), seed=42)
    elif src.startswith("case:"):                      # a builder of tests/hydronet_cases.py regenerates the field
        import hydronet_cases
        land, elev, _, _ = hydronet_cases.GOLDENED[src[5:]]()
        assert elev.shape == (n_lat, n_lon) and np.array_equal(land, z["land_mask"]), src
    else:
        elev = np.asarray(z["elevation"], dtype=float)
    return (n_lat, n_lon), np.asarray(z["land_mask"]), elev, float(z["eps"]), int(z["max_iters"])


def golden_filled(z, elev):
    land = np.asarray(z["land_mask"]) == 1
    ef = np.array(elev, dtype=float)
    ef[land] = z["ef_land"]
    return ef


def pit_fill_sweeps(elev, land, eps, sweeps):
    """Up to `sweeps` in-place row-major sweeps over the land cells -> (filled, sweeps run).  A land cell at or below the
    min of its D8 neighbours (longitude wraps, the poles do not) becomes min + eps when that is higher; the sweeps stop
    after one that changed nothing."""
    n_lat, n_lon = elev.shape
    e = [list(map(float, row)) for row in np.asarray(elev, dtype=float)]
    L = [list(row) for row in (np.asarray(land) == 1)]
    eps = float(eps)
    run = 0
    for _ in range(sweeps):
        run += 1
        changed = False
        for j in range(n_lat):
            rows = [e[jj] for jj in (j - 1, j, j + 1) if 0 <= jj < n_lat]
            lrow, row = L[j], e[j]
            for i in range(n_lon):
                if not lrow[i]:
                    continue
                w, east = i - 1, (i + 1) % n_lon
                m = min(min(r[w], r[i], r[east]) for r in rows if r is not row)
                m = min(m, row[w], row[east])
                if row[i] <= m:
                    v = m + eps
                    if v > row[i]:
                        row[i] = v
                        changed = True
        if not changed:
            break
    return np.array(e), run


def d8(grid_lat_rad, grid_lon_rad, cos_pair, land, z):
    """Steepest descent, first of equal slopes in (dj, di) order; -1 for ocean, flat or uphill cells and for a steepest
    neighbour in the ocean."""
    n_lat, n_lon = z.shape
    land = np.asarray(land) == 1
    best = np.full((n_lat, n_lon), -np.inf)
    bidx = np.full((n_lat, n_lon), -1, np.int64)
    jj0, ii0 = np.meshgrid(np.arange(n_lat), np.arange(n_lon), indexing="ij")
    for dj, di in DIRS:
        jj = jj0 + dj
        ok = (jj >= 0) & (jj < n_lat)
        jc = np.clip(jj, 0, n_lat - 1)
        ii = (ii0 + di) % n_lon
        dlon = grid_lon_rad[ii] - grid_lon_rad[ii0]
        dlon = np.where(dlon > np.pi, dlon - 2 * np.pi, np.where(dlon < -np.pi, dlon + 2 * np.pi, dlon))
        x = dlon * cos_pair[jj0, dj + 1]
        y = grid_lat_rad[jc] - grid_lat_rad[jj0]
        with np.errstate(invalid="ignore", divide="ignore"):
            dist = PLANET_RADIUS * np.sqrt(x * x + y * y)
            slope = (z - z[jc, ii]) / dist
        upd = ok & (dist > 0) & (slope > best)
        best = np.where(upd, slope, best)
        bidx = np.where(upd, jc * n_lon + ii, bidx)
    lf = land.ravel()
    out = np.where((best > 0) & (bidx >= 0) & lf[np.clip(bidx, 0, None)].reshape(n_lat, n_lon), bidx, -1)
    return np.where(land, out, -1)


def neighbours(j, i, n_lat, n_lon):
    for dj, di in DIRS:
        jj = j + dj
        if 0 <= jj < n_lat:
            yield jj, (i + di) % n_lon


def lakes(flow, land):
    """D8 components of land & flow == -1, numbered 1.. by their smallest row-major cell."""
    n_lat, n_lon = land.shape
    term = (np.asarray(land) == 1) & (np.asarray(flow) == -1)
    lid = np.zeros((n_lat, n_lon), np.int32)
    k = 0
    for j, i in zip(*np.nonzero(term)):
        if lid[j, i]:
            continue
        k += 1
        lid[j, i] = k
        q = [(j, i)]
        while q:
            a, b = q.pop()
            for jj, ii in neighbours(a, b, n_lat, n_lon):
                if term[jj, ii] and not lid[jj, ii]:
                    lid[jj, ii] = k
                    q.append((jj, ii))
    return term.astype(np.uint8), lid, k


def outlets(z, lake_mask, lake_id, land, n_lakes):
    """Per lake: -1 when a lake cell has an ocean neighbour, else the first lowest non-lake land neighbour in (lake cell
    row-major, neighbour) order, -1 without one."""
    n_lat, n_lon = land.shape
    best = [np.inf] * n_lakes
    pick = [-1] * n_lakes
    ocean = [False] * n_lakes
    for j, i in zip(*np.nonzero(lake_mask)):
        k = int(lake_id[j, i]) - 1
        if ocean[k]:
            continue
        for jj, ii in neighbours(j, i, n_lat, n_lon):
            if lake_mask[jj, ii] == 1:
                continue
            if land[jj, ii] == 0:
                ocean[k] = True
                break
            v = float(z[jj, ii])
            if v < best[k]:
                best[k], pick[k] = v, jj * n_lon + ii
    return np.array([-1 if ocean[k] else pick[k] for k in range(n_lakes)], np.int32)


def flow_order(flow, land):
    """Kahn's algorithm with a FIFO queue over the land cells; never-placed land cells appended in index order."""
    lf = (np.asarray(land) == 1).ravel()
    f = np.asarray(flow).ravel()
    indeg = np.zeros(lf.size, np.int64)
    src = np.nonzero(lf & (f >= 0))[0]
    dst = f[src]
    dst = dst[lf[dst]]
    np.add.at(indeg, dst, 1)
    indeg = indeg.tolist()
    fl = f.tolist()
    lfl = lf.tolist()
    q = deque(np.nonzero(lf & (np.asarray(indeg) == 0))[0].tolist())
    order = []
    while q:
        u = q.popleft()
        order.append(u)
        d = fl[u]
        if d >= 0 and lfl[d]:
            indeg[d] -= 1
            if indeg[d] == 0:
                q.append(d)
    if len(order) < int(lf.sum()):
        seen = set(order)
        order += [c for c in np.nonzero(lf)[0].tolist() if c not in seen]
    return np.array(order, np.int64)
