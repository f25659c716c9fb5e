"""Hostile terrain and size edges for the network generator (qd_hydronet.hip), shared by test_hydronet_cases_cpu.py and
test_gpu_hydronet_cases.py.

Builders return (land u1, elevation f64, eps, max_iters) from seeded NumPy generators, so no elevation is committed: a golden
of one of these cases names its builder (elev_src "case:<name>") and hydronet_ref.case_inputs rebuilds the field.  CASES
holds every case by name; GOLDENED those small enough for a golden of the reference's generator
(scripts/gen_golden_hydronet.py), RESTATED the wide ones that are checked against the restatements of hydronet_ref alone.

`chunk_model` is the pit fill as the header comment of qd_hydronet.hip states it -- chunks of 16 cells, the two trajectories
from -inf and +inf until they meet on equal bits, the carry from the nearest merged chunk to the west, the dirty-row rule --
in plain Python.  It reports per row visit which chunks never merged, so a test can tell that a case reaches the serial
carry walk.  `pitfill_lds_bytes` restates the kernel's LDS layout.

Not covered on purpose: the flow order's `placed < n_land` branch.  It needs a cycle, and D8 on a field (filled or not)
cannot produce one through the public entry, as every edge goes strictly downhill.
"""
import math

import numpy as np

PF_CHUNK = 16                 # HN_PF_C
PF_THREADS = 256              # HN_PF_T
SCAN_TILE = 2048              # HN_SCAN_TILE
ORDER_SLICE = 1024            # HN_ORDER_T
LDS_DEFAULT = 64 * 1024       # above it the launch needs the enlarged dynamic-LDS attribute
LDS_STATIC = 256              # the kernel's static LDS: the scratch of __syncthreads_or's workgroup reduction (64 ints)
LDS_LIMIT = 160 * 1024 - LDS_STATIC   # a workgroup's 160 KiB less the static part: qd_hydronet_build refuses above it


# ---------------------------------------------------------------- the two fields of the first goldens
def valley_field(n_lat, n_lon, seed):
    """Land everywhere (both pole rows included) but an ocean blob; a seeded rough field, and a closed east-west valley
    whose floor rises eastward by less than eps per cell: the in-row chain of the pit fill carries along the whole valley."""
    rng = np.random.default_rng(seed)
    land = np.ones((n_lat, n_lon), np.uint8)
    jj, ii = np.meshgrid(np.arange(n_lat), np.arange(n_lon), indexing="ij")
    land[((jj - n_lat // 4) ** 2 + ((ii - n_lon // 8) / 3.0) ** 2) < 9] = 0
    elev = 500.0 + 200.0 * np.sin(jj / 3.0) * np.cos(ii / 7.0) + rng.normal(0.0, 30.0, (n_lat, n_lon))
    j0, a, b = n_lat // 2, n_lon // 8, n_lon - n_lon // 8
    elev[j0 - 1:j0 + 2, a - 1:b + 1] = 2000.0
    elev[j0, a:b] = 10.0 + 1e-4 * np.arange(b - a)
    return land, np.where(land == 1, elev, -100.0)


def inland_field(n_lat, n_lon, seed):
    """Mostly land, quantised elevation (flats and ties in D8 slopes and lake outlets): after a short fill the pits are lakes
    that touch no ocean and drain through real outlets."""
    rng = np.random.default_rng(seed)
    land = np.ones((n_lat, n_lon), np.uint8)
    land[:3, :] = 0
    land[-2:, : n_lon // 3] = 0
    elev = np.round(rng.uniform(0.0, 6.0, (n_lat, n_lon))) * 50.0
    return land, np.where(land == 1, elev, 0.0)


# ---------------------------------------------------------------- builders
def _rough(rng, n_lat, n_lon):
    return 500.0 + rng.normal(0.0, 30.0, (n_lat, n_lon))


def seam_valley(n_lat=9, n_lon=272, seed=21, rising=True):
    """A walled valley on the middle row that crosses the seam: its floor runs eastward from column n/2 over n-1 and 0 to
    n/4 - 1, 1e-4 per cell up (or down, the twin), less than eps.  Going up eastward no chunk of the floor merges, so the run
    of never-merged chunks reaches the row's last chunk and the carry is walked up to cell n-1, which reads the new cell 0."""
    rng = np.random.default_rng(seed)
    land = np.ones((n_lat, n_lon), np.uint8)
    land[0, :5] = 0
    elev = _rough(rng, n_lat, n_lon)
    j0 = n_lat // 2
    elev[j0 - 1:j0 + 2, :] = 2000.0
    cols = (n_lon // 2 + np.arange(n_lon // 2 + n_lon // 4)) % n_lon
    elev[j0, cols] = 10.0 + (1e-4 if rising else -1e-4) * np.arange(cols.size)
    return land, elev, 1e-3, 30


def ring(n_lat=7, n_lon=50, seed=22):
    """A flat floor on a whole row between walls: cell 0 reads the last sweep's cell n-1, cell n-1 the new cell 0, and the
    floor climbs by eps a sweep until the sweeps run out."""
    rng = np.random.default_rng(seed)
    land = np.ones((n_lat, n_lon), np.uint8)
    land[n_lat - 1, 7] = 0
    elev = _rough(rng, n_lat, n_lon)
    j0 = n_lat // 2
    elev[j0 - 1:j0 + 2, :] = 2000.0
    elev[j0, :] = 10.0
    return land, elev, 1e-3, 80


def _quantised(n_lat, n_lon, seed, max_iters):
    rng = np.random.default_rng(seed)
    land = (rng.random((n_lat, n_lon)) < 0.8).astype(np.uint8)
    elev = np.round(rng.uniform(0.0, 6.0, (n_lat, n_lon))) * 10.0
    return land, elev, 1e-3, max_iters


def tiny(n_lat, n_lon, seed=23):
    """qd_create's minima and rows of one partial chunk, one whole chunk, two chunks and a cell: 80 % land, multiples of 10."""
    return _quantised(n_lat, n_lon, seed + 100 * n_lat + n_lon, 50)


def scan_edges(n_lat, n_lon, seed=24):
    """A cell count that is a whole number of scan tiles (2048): the last tile is full."""
    assert (n_lat * n_lon) % SCAN_TILE == 0
    return _quantised(n_lat, n_lon, seed + n_lat, 3)


SIGNED_ZERO_PITS = ((3, 5), (5, 12), (6, 19))


def signed_zero(n_lat=9, n_lon=24, seed=25, max_iters=0):
    """Land except row 0, a random mix of +0.0 and -0.0 with three pits at -5.  Unfilled, each pit is a one-cell lake whose
    outlet candidates are its eight neighbours, all zero, of both signs; the first pit's first candidate is +0.0 and a later
    one -0.0, so an outlet key that kept the sign would pick the later one where the reference's strict < keeps the first."""
    rng = np.random.default_rng(seed)
    land = np.ones((n_lat, n_lon), np.uint8)
    land[0, :] = 0
    elev = np.where(rng.random((n_lat, n_lon)) < 0.5, 0.0, -0.0)
    for j, i in SIGNED_ZERO_PITS:
        elev[j, i] = -5.0
    j, i = SIGNED_ZERO_PITS[0]
    elev[j - 1, i - 1] = 0.0
    elev[j - 1, i] = -0.0
    return land, elev, 1e-3, max_iters


def all_land_flat(n_lat=5, n_lon=12):
    """No ocean and no slope: one lake of every cell, with neither an ocean neighbour nor a land neighbour outside it."""
    return np.ones((n_lat, n_lon), np.uint8), np.zeros((n_lat, n_lon)), 1e-3, 0


def serpentine(n_lat=33, n_lon=64):
    """All land, unfilled.  Odd rows are walls at 100 with a three-cell gap, by turns at the east end and at the west end; the
    last column is a wall from pole to pole, or the gaps of neighbouring walls would touch across the seam.  The floor is one
    lake whose smallest label has to travel the whole snake."""
    elev = np.zeros((n_lat, n_lon))
    elev[1::2, :] = 100.0
    elev[:, n_lon - 1] = 100.0
    for k, j in enumerate(range(1, n_lat, 2)):
        lo = n_lon - 4 if k % 2 == 0 else 0
        elev[j, lo:lo + 3] = 0.0
    return np.ones((n_lat, n_lon), np.uint8), elev, 1e-3, 0


def seam_pole_lake(n_lat=9, n_lon=40):
    """All land, unfilled: a flat strip on columns n-2, n-1, 0, 1 of every row, the pole rows included, and flanks that rise
    away from it in steps of 10, so every outlet candidate ties."""
    i = np.arange(n_lon)
    d = np.minimum.reduce([np.minimum((i - c) % n_lon, (c - i) % n_lon) for c in (n_lon - 2, n_lon - 1, 0, 1)])
    elev = np.tile(10.0 * d, (n_lat, 1))
    return np.ones((n_lat, n_lon), np.uint8), elev, 1e-3, 0


def cone(n_lat=9, n_lon=12):
    """All land, unfilled: a square pyramid upside down, so all eight neighbours of its tip drain into the tip."""
    jj, ii = np.meshgrid(np.arange(n_lat), np.arange(n_lon), indexing="ij")
    di = np.minimum((ii - n_lon // 2) % n_lon, (n_lon // 2 - ii) % n_lon)
    elev = 100.0 * np.maximum(np.abs(jj - n_lat // 2), di)
    return np.ones((n_lat, n_lon), np.uint8), elev.astype(float), 1e-3, 0


EPS_EDGES_BASE = 1000.0


def eps_edges(eps, n_lat=37, n_lon=72, seed=6):
    """The inland field with an eps of 0.5 (every flat climbs far), and with an eps of 1e-14, below half an ulp of its
    elevations: m + eps == m, so a cell level with its lowest neighbour stays only by the `m + eps > e` guard, and the first
    sweep changes nothing.  For that the field is made ready in two ways.  Its multiples of 50 stand on a base of 1000 (half an
    ulp is 5.7e-14 from 512 up, but 3.6e-15 at 50 and nothing at 0, where 1e-14 still moves a cell), and its strict pits,
    which any eps fills up to their lowest neighbour, are filled beforehand: what is left are flats, level with that
    neighbour."""
    land, elev = inland_field(n_lat, n_lon, seed)
    if eps < 1e-3:
        from hydronet_ref import pit_fill_sweeps
        elev, run = pit_fill_sweeps(np.where(land == 1, elev + EPS_EDGES_BASE, elev), land, eps, 50)
        assert run < 50
    return land, elev, eps, 5


def vplane(n_lat=13, n_lon=4320, seed=26):
    """A V-shaped plane, 100 j + 0.5 |i - n/2| with 0.01 of noise, row 0 ocean: the rows near the poles drain along
    themselves to the middle column, a run of more than two thousand Kahn generations.  The first generations are a whole
    row each (the row below drains along itself and feeds nothing north), so the row is 4320 cells wide: at 2880 columns no
    generation would pass the 4096 cells asked of this case."""
    rng = np.random.default_rng(seed)
    land = np.ones((n_lat, n_lon), np.uint8)
    land[0, :] = 0
    jj, ii = np.meshgrid(np.arange(n_lat), np.arange(n_lon), indexing="ij")
    elev = 100.0 * jj + 0.5 * np.abs(ii - n_lon // 2) + rng.normal(0.0, 0.01, (n_lat, n_lon))
    return land, elev, 1e-3, 3


def wide(n_lon, n_lat=13, seed=27):
    """Rows wider than the widest the other tests build: 90 % random land on a rough field and a walled valley on row 6 over
    columns 101 .. n-102 (all land) that rises 1e-4 per cell.  1940 / 1941 columns straddle the pit fill's 64 KiB of LDS,
    2880 is the large configuration's width, 4097 gives a lane two chunks, 4846 is the widest row the build accepts (4853 would
    fill the 160 KiB by itself, without the kernel's 256 B of static LDS)."""
    rng = np.random.default_rng(seed + n_lon)
    land = (rng.random((n_lat, n_lon)) < 0.9).astype(np.uint8)
    elev = _rough(rng, n_lat, n_lon)
    a, b = 101, n_lon - 101
    land[5:8, a - 1:b + 1] = 1
    elev[5:8, a - 1:b + 1] = 2000.0
    elev[6, a:b] = 10.0 + 1e-4 * np.arange(b - a)
    return land, elev, 1e-3, 6


TINY_SHAPES = ((5, 4), (5, 5), (6, 17), (5, 16), (7, 33))
WIDE_COLUMNS = (1940, 1941, 2880, 4097, 4846)

GOLDENED = {
    "seam_valley_rise_9x272": lambda: seam_valley(rising=True),
    "seam_valley_fall_9x272": lambda: seam_valley(rising=False),
    "ring_7x50": ring,
    **{f"tiny_{a}x{b}": (lambda a=a, b=b: tiny(a, b)) for a, b in TINY_SHAPES},
    "scan_edges_32x64": lambda: scan_edges(32, 64),
    "scan_edges_64x96": lambda: scan_edges(64, 96),
    "signed_zero_it0_9x24": lambda: signed_zero(max_iters=0),
    "signed_zero_it5_9x24": lambda: signed_zero(max_iters=5),
    "all_land_flat_5x12": all_land_flat,
    "serpentine_33x64": serpentine,
    "seam_pole_lake_9x40": seam_pole_lake,
    "cone_9x12": cone,
    "eps_tiny_37x72": lambda: eps_edges(1e-14),
    "eps_large_37x72": lambda: eps_edges(0.5),
}
RESTATED = {
    "vplane_13x4320": vplane,
    **{f"wide_13x{n}": (lambda n=n: wide(n)) for n in WIDE_COLUMNS},
}
CASES = {**GOLDENED, **RESTATED}


# ---------------------------------------------------------------- the kernel's LDS layout and sweep, restated
def pitfill_lds_bytes(n_lat, n_lon):
    """Three cached rows and the row's new values (f64), per chunk a tail (f64) and a merge count (i32), the row's land flags
    and two changed-flags per row (bytes)."""
    nch = -(-n_lon // PF_CHUNK)
    return 4 * n_lon * 8 + nch * (8 + 4) + n_lon + 2 * n_lat


def _same_bits(a, b):
    return a == b and (a != 0.0 or math.copysign(1.0, a) == math.copysign(1.0, b))


def chunk_model(elev, land, eps, max_iters, chunk=PF_CHUNK):
    """-> (filled, sweeps run, visits); visits is a list of (sweep, row, never) per row swept, never[k] true where chunk k's
    trajectories did not meet within the chunk."""
    n_lat, n = np.shape(elev)
    e = [list(map(float, row)) for row in np.asarray(elev, dtype=float)]
    L = [list(row) for row in (np.asarray(land) == 1)]
    eps = float(eps)
    nch = -(-n // chunk)
    inf = math.inf

    def f(l, ei, m):
        me = m + eps
        return me if (l and ei <= m and me > ei) else ei

    visits = []
    chg_prev = [False] * n_lat
    run = 0
    for it in range(1, max_iters + 1):
        run = it
        chg_cur = [False] * n_lat
        prev_changed = False
        for j in range(n_lat):
            if not (it == 1 or prev_changed or chg_prev[j] or (j + 1 < n_lat and chg_prev[j + 1])):
                prev_changed = False
                continue
            cur, lrow = e[j], L[j]
            others = [e[jj] for jj in (j - 1, j + 1) if 0 <= jj < n_lat]
            # A[i]: the min of the non-west neighbours of cell i >= 1, but for the new cell 0 east of cell n-1
            A = [inf] * n
            for i in range(1, n):
                ip = i + 1 if i + 1 < n else 0
                a = cur[ip] if i + 1 < n else inf
                for r in others:
                    a = min(a, r[i - 1], r[i], r[ip])
                A[i] = a
            a0 = min(cur[n - 1], cur[1])
            for r in others:
                a0 = min(a0, r[n - 1], r[0], r[1])
            x0 = f(lrow[0], cur[0], a0)
            A[n - 1] = min(x0, A[n - 1])
            nv = list(cur)
            nv[0] = x0
            mrg, tail = [0] * nch, [0.0] * nch
            for k in range(nch):
                i0, i1 = k * chunk, min((k + 1) * chunk, n)
                lo, hi, x, met, p = -inf, inf, 0.0, False, i1 - i0
                for i in range(i0, i1):
                    if i == 0:
                        x, met, p = x0, True, 0
                    elif met:
                        x = nv[i] = f(lrow[i], cur[i], min(x, A[i]))
                    else:
                        lo = f(lrow[i], cur[i], min(lo, A[i]))
                        hi = f(lrow[i], cur[i], min(hi, A[i]))
                        if _same_bits(lo, hi):
                            met, p, x = True, i - i0, lo
                            nv[i] = x
                mrg[k], tail[k] = p, x
            never = [mrg[k] == min(chunk, n - k * chunk) for k in range(nch)]
            for k in range(nch):
                if mrg[k] == 0:
                    continue
                q = k - 1
                while never[q]:
                    q -= 1
                x = tail[q]
                for i in range((q + 1) * chunk, k * chunk + mrg[k]):
                    x = f(lrow[i], cur[i], min(x, A[i]))
                    if i >= k * chunk:
                        nv[i] = x
            visits.append((it, j, never))
            changed = any(not _same_bits(a, b) for a, b in zip(nv, cur))
            e[j] = nv
            chg_cur[j] = prev_changed = changed
        if not any(chg_cur):
            break
        chg_prev = chg_cur
    return np.array(e), run, visits


def kahn_generations(flow, land):
    """-> the sizes of Kahn's generations: the land cells of in-degree 0, then those whose last predecessor was in the
    generation before, and so on (one barrier round of k_hn_order_gen each, walked in slices of 1024)."""
    lf = (np.asarray(land) == 1).ravel()
    f = np.asarray(flow).ravel()
    has = lf & (f >= 0)
    has[has] = lf[f[has]]
    rem = np.bincount(f[has], minlength=f.size)
    gen = np.nonzero(lf & (rem == 0))[0]
    sizes = []
    while gen.size:
        sizes.append(int(gen.size))
        d = f[gen[has[gen]]]
        np.subtract.at(rem, d, 1)
        d = np.unique(d)
        gen = d[rem[d] == 0]
    return sizes


def longest_never_run(never):
    """-> (length of the longest run of never-merged chunks, whether a run of that length ends in the row's last chunk)."""
    best, cur, at_end = 0, 0, False
    for k, v in enumerate(never):
        cur = cur + 1 if v else 0
        if cur > best or (cur == best and cur > 0 and k == len(never) - 1):
            best, at_end = cur, k == len(never) - 1
    return best, at_end


_RESTATED = {}


def restated(name):
    """The five stages of case `name` by the restatements of hydronet_ref, computed once and shared read-only:
    dict(land, elevation, eps, max_iters, sweeps, elevation_filled, flow_to_index, lake_mask, lake_id, n_lakes,
    lake_outlet_index, flow_order)."""
    if name not in _RESTATED:
        import hydronet_ref as hr
        import qingdai_amd as qa
        from qingdai_amd.hydronet import host_tables
        land, elev, eps, max_iters = CASES[name]()
        ef, sweeps = hr.pit_fill_sweeps(elev, land, eps, max_iters)
        flow = hr.d8(*host_tables(qa.SphericalGrid(*elev.shape)), land, ef)
        lm, lid, nl = hr.lakes(flow, land)
        out = dict(land=land, elevation=elev, eps=eps, max_iters=max_iters, sweeps=sweeps, elevation_filled=ef, flow_to_index=flow,
                   lake_mask=lm, lake_id=lid, n_lakes=nl, lake_outlet_index=hr.outlets(ef, lm, lid, land, nl),
                   flow_order=hr.flow_order(flow, land))
        for v in out.values():
            if isinstance(v, np.ndarray):
                v.setflags(write=False)
        _RESTATED[name] = out
    return _RESTATED[name]
