"""
qingdai_amd/spharm.py -- spherical-harmonic power spectra (QD_SPHARM=1), host side of csrc/qd_spharm.hip: power per TOTAL
wavenumber n on the sphere, the view in which a global model's dissipation is judged.

Nothing the reference has.  On every sampled step of the device loop each selected field is analysed on the device into
spherical-harmonic coefficients up to a triangular truncation N, and one record per sample -- per entry P(0 .. N), the mean square
and the count of bad rows -- stays in the lane's device log.  This file is the DEFINITION; the device is held to it
(tests/test_gpu_spharm.py).

Grid: n = n_lon columns, periodic by index, lambda_i = 2 pi i / n; L = n_lat - 1, rows j = 0 .. L with mu_j = sin(-pi / 2 + j pi / L),
+-1 exactly on the pole rows.  These are the Chebyshev extreme points in mu, and Clenshaw-Curtis weights on them integrate
polynomials in mu up to degree n_lat - 1 exactly, so the analysis is exact (no least squares) for the triangular truncation
    N = min((n_lat - 1) // 2, (n_lon - 1) // 2)                                                          (T360 at 721 x 1440).
  1 row transform   X_j(m) = (1 / n) sum_i x[j][i] exp(-2 pi i im / n),  m = 0 .. N
  2 weights         w_j = (g_j / L) [1 - sum_{k=1}^{L // 2} b_k / (4 k^2 - 1) cos(2 k j pi / L)],  g_j = 1 on the poles, 2 otherwise,
                    b_k = 1 for 2 k = L, 2 otherwise; sum_j w_j = 2
  3 Legendre        Pbar_n^m normalised so that (1 / 2) int Pbar^2 dmu = 1:  Pbar_m^m = prod_{k=1}^{m} sqrt((2k + 1) / (2k)) (1 - mu^2)^(m/2),
                    Pbar_n^m = A_n^m (mu Pbar_{n-1}^m - B_n^m Pbar_{n-2}^m) for n > m from Pbar_{m-1}^m = 0,
                    A_n^m = sqrt((4 n^2 - 1) / (n^2 - m^2)),  B_n^m = sqrt(((n - 1)^2 - m^2) / (4 (n - 1)^2 - 1))
                    (so A_{m+1}^m = sqrt(2m + 3), B_{m+1}^m = 0).  Weights, mu, the seeds Pbar_m^m(mu_j) and A, B are host DATA, built
                    in extended precision and rounded once (tables); the recurrence itself runs in f64.
  4 coefficients    x_n^m = (1 / 2) sum_j w_j Pbar_n^m(mu_j) X_j(m), complex, 0 <= m <= n <= N
  5 power           P(n) = sum_{m=0}^{n} c_m |x_n^m|^2,  c_0 = 1, c_m = 2 otherwise; for a field band-limited to N, sum_n P(n) is the
                    sphere mean of x^2
  6 mean square     ms = (1 / 2) sum_j w_j mean_i x[j][i]^2  and  resid = 1 - sum_n P(n) / ms: the share of variance beyond the
                    truncation, aliased part included -- how far to trust the bins near N.
Entries are history's (its parser, ocean-only rule, refusals and sampling places) and two names of this lane alone, VORT and DIV:
the flow lane's zeta and delta (flow.vortdiv_reference, pole caps included), produced by the flow lane's kernel; they do not need
QD_FLOW=1.  With both selected the host forms ke_rot(n) = a^2 P_zeta(n) / (2 n (n + 1)), ke_div(n) likewise from P_delta, and
ke = ke_rot + ke_div for n >= 1 (0 at n = 0).  A non-finite value anywhere in a plane makes every coefficient and every bin of that
plane NaN (the transform couples every cell), and the rows that hold one are counted.

analyse_reference is the definition in f64 and in extended precision, power_reference the device's order of P, ms and the bad
rows restated bit for bit, synthesise the inverse transform (host only, for tests).  Windows, clock, labels and files follow the
spectra lane: <QD_OUTPUT_DIR, default output>/spharm/spharm_day_{a}_{b}.nc.  Nothing here touches the device at import.
"""
from __future__ import annotations

import functools
import types

import numpy as np

from . import flow, history, order
from ._lib import C
from .window_lane import LogWindowLane, env_days, env_dt, env_every, env_int, i8_code, window_file_name

FIELDS_VAR = "QD_SPHARM_FIELDS"
DEFAULT_FIELDS = ("VORT", "DIV", "H")
OWN = {"VORT": C["QD_SPHARM_OP_VORT"], "DIV": C["QD_SPHARM_OP_DIV"]}      # the entry ops of this lane alone
EVERY_DAYS, EVERY, TWO_D = 10.0, 24, 1
STATS = C["QD_SPHARM_STATS"]                         # ms and the bad-row count behind an entry's N + 1 powers
LOG_CAP = C["QD_SPHARM_LOG_CAP"]
MAX_LAT = C["QD_SPHARM_MAX_LAT"]                     # rows the Legendre kernel's widest form takes


def truncation(n_lat, n_lon):
    """N = min((n_lat - 1) // 2, (n_lon - 1) // 2); a grid with N < 1 is refused."""
    N = min((int(n_lat) - 1) // 2, (int(n_lon) - 1) // 2)
    if N < 1:
        raise ValueError(f"spharm: a grid of {int(n_lat)} x {int(n_lon)} gives the truncation N = {N}; N >= 1 is needed "
                         f"(n_lat >= 3 and n_lon >= 3)")
    return N


# ------------------------------------------------------------------------------------- the tables, in extended precision
def _math(kind):
    """(number from an int, pi, sqrt, cos, sin) of a working precision: np.longdouble, or mpmath at 80 bits as object arrays."""
    if kind == "mpmath":
        import mpmath
        mpmath.mp.prec = 80
        vec = lambda f: np.vectorize(f, otypes=[object])
        num = lambda x: vec(lambda t: mpmath.mpf(int(t)))(np.asarray(x))
        return num, +mpmath.pi, vec(mpmath.sqrt), vec(mpmath.cos), vec(mpmath.sin)
    ld = np.longdouble
    return (lambda x: np.asarray(x).astype(ld)), ld(4) * np.arctan(ld(1)), np.sqrt, np.cos, np.sin


def _round(x):
    return np.array([float(t) for t in np.ravel(x)], dtype=np.float64).reshape(np.shape(x))


@functools.lru_cache(maxsize=16)
def _tables(n_lat, n_lon, kind):
    """w, mu [n_lat], seed [N + 1][n_lat] = Pbar_m^m(mu_j), A, B [N + 1 (m)][N + 1 (n)] in the working precision `kind`.  The
    hemispheres mirror exactly: row L - j holds w_j and -mu_j, the equator row of an odd n_lat mu = 0."""
    N, L = truncation(n_lat, n_lon), n_lat - 1
    num, pi, sqrt, cos, sin = _math(kind)
    half = L // 2 + 1                                        # rows 0 .. L // 2
    j = np.arange(half)
    # angles as pi r / (2 L), r an integer, folded into [0, pi / 4] by cos / sin of the complement, so the mirror images are exact
    def cs(r):                                               # cos, sin(pi r / (2 L)) for integers 0 <= r <= L (the first quadrant)
        r = np.asarray(r, dtype=np.int64)
        lo = 2 * r <= L
        a = num(np.where(lo, r, L - r)) * (pi / num(2 * L))
        ca, sa = cos(a), sin(a)
        return np.where(lo, ca, sa), np.where(lo, sa, ca)
    cq, sq = cs(2 * j)                                       # cos, sin(j pi / L), j <= L / 2
    mu_h, cphi_h = -cq, sq                                   # mu_j = sin(-pi / 2 + j pi / L) = -cos(j pi / L); cos(phi_j) = sin(j pi / L)
    if L % 2 == 0:
        mu_h[-1] = mu_h[-1] * 0                              # the equator row
    one = num(1)
    # Clenshaw-Curtis: cos(2 k j pi / L) = cos(pi r / L) with r = 2 k j mod 2 L, from a table over the full turn built by symmetry
    t = np.arange(2 * L)
    fold = np.where(t <= L, t, 2 * L - t)                    # cos(pi t / L) = cos(pi (2 L - t) / L)
    q = np.where(fold <= L // 2, fold, L - fold)             # ... = -cos(pi (L - t) / L) beyond the quarter turn
    cq2, _ = cs(np.minimum(2 * q, L))
    tab = np.where(fold <= L // 2, cq2, -cq2)
    if L % 2 == 0:
        tab[fold == L // 2] = tab[0] * 0
    k = np.arange(1, L // 2 + 1)
    b = num(np.where(2 * k == L, 1, 2)) / num(4 * k * k - 1)
    s = (tab[(2 * k[None, :] * j[:, None]) % (2 * L)] * b[None, :]).sum(axis=1)
    w_h = num(np.where(j == 0, 1, 2)) / num(L) * (one - s)
    mirror = lambda x, sign: np.concatenate([x, sign * x[:n_lat - half][::-1]])
    w, mu, cphi = mirror(w_h, 1), mirror(mu_h, -1), mirror(cphi_h, 1)
    # seeds: Pbar_m^m = c_m cos(phi)^m, c_m = prod sqrt((2k + 1) / (2k)), by running products
    seed = np.empty((N + 1, n_lat), dtype=w.dtype)
    seed[0] = cphi * 0 + one
    run, c_run = cphi * 0 + one, one
    for m in range(1, N + 1):
        run = run * cphi
        c_run = c_run * sqrt(num(2 * m + 1) / num(2 * m))
        seed[m] = c_run * run
    mm, nn = np.meshgrid(np.arange(N + 1), np.arange(N + 1), indexing="ij")
    up = nn > mm
    A = np.where(up, sqrt(num(np.where(up, 4 * nn * nn - 1, 1)) / num(np.where(up, nn * nn - mm * mm, 1))), one * 0)
    B = np.where(up, sqrt(num(np.where(up, (nn - 1) ** 2 - mm * mm, 0)) / num(np.where(up, np.maximum(4 * (nn - 1) ** 2 - 1, 1), 1))), one * 0)
    return w, mu, seed, A, B


def _ext_kind():
    return flow._kind(True)


def tables(n_lat, n_lon):
    """The tables of the transform as f64 DATA, rounded once from extended precision, shared by the device and the f64 reference ->
    namespace(n_lat, n_lon, N, L, npairs, w, mu [n_lat], seed [N + 1][n_lat], A, B [N + 1][N + 1] indexed [m][n], seed_pairs
    [N + 1][npairs]: the seeds of the rows 0 .. npairs - 1, what the device takes)."""
    n_lat, n_lon = int(n_lat), int(n_lon)
    N = truncation(n_lat, n_lon)
    w, mu, seed, A, B = (_round(x) for x in _tables(n_lat, n_lon, _ext_kind()))
    npairs = (n_lat + 1) // 2
    return types.SimpleNamespace(n_lat=n_lat, n_lon=n_lon, N=N, L=n_lat - 1, npairs=npairs, w=w, mu=mu, seed=seed, A=A, B=B,
                                 seed_pairs=np.ascontiguousarray(seed[:, :npairs]))


def grid_tables(grid):
    return tables(np.asarray(grid.lat).size, np.asarray(grid.lon).size)


def legendre(g, m, extended=False):
    """Pbar_n^m(mu_j) [N + 1 (n)][n_lat] by the recurrence of the definition, rows n < m zero: in f64 on the f64 tables, or with
    extended=True in extended precision on the unrounded tables."""
    if extended:
        w, mu, seed, A, B = _tables(g.n_lat, g.n_lon, _ext_kind())
    else:
        mu, seed, A, B = g.mu, g.seed, g.A, g.B
    P = np.empty((g.N + 1, g.n_lat), dtype=mu.dtype)
    P[:] = mu[0] * 0
    P[m] = seed[m]
    p1, p2 = seed[m], seed[m] * 0
    for n in range(m + 1, g.N + 1):
        p1, p2 = A[m, n] * (mu * p1 - B[m, n] * p2), p1
        P[n] = p1
    return P


def _row_transform(plane, g, kind):
    """X_j(m) [n_lat][N + 1] as (Re, Im) in the working precision: direct sums, i ascending through the dot product."""
    n = g.n_lon
    x = flow._conv(plane, kind)
    tc, ts = flow._twiddles(n, kind)
    idx = (np.arange(n)[:, None] * np.arange(g.N + 1)[None, :]) % n
    one = tc[0] / tc[0]
    return x.dot(tc[idx]) / (one * n), -(x.dot(ts[idx])) / (one * n)


def analyse_reference(plane, g, extended=False):
    """The definition at the top of this file -> coef [N + 1 (m)][N + 1 (n)] complex128, x_n^m at [m][n], zero for n < m.  In f64 on
    the f64 tables, or with extended=True in extended precision (np.longdouble where it is wider than f64, mpmath at 80 bits
    elsewhere) on the unrounded tables, rounded once at the end.  Every row is taken by itself: no use of the hemispheres' symmetry."""
    x = np.ascontiguousarray(plane, dtype=np.float64)
    if x.shape != (g.n_lat, g.n_lon):
        raise ValueError(f"analyse_reference: the plane is [{g.n_lat}][{g.n_lon}]")
    N = g.N
    out = np.zeros((N + 1, N + 1), dtype=np.complex128)
    if not np.isfinite(x).all():
        out[:] = complex(np.nan, np.nan)
        return out
    kind = flow._kind(extended)
    w = _tables(g.n_lat, g.n_lon, kind)[0] if extended else g.w
    XR, XI = _row_transform(x, g, kind)
    half = w[0] / w[0] / 2
    for m in range(N + 1):
        Pw = legendre(g, m, extended) * w[None, :]
        re, im = half * Pw.dot(XR[:, m]), half * Pw.dot(XI[:, m])
        out[m, m:] = _round(re)[m:] + 1j * _round(im)[m:]
    return out


def synthesise(coef, g, extended=False):
    """The inverse transform, host only: x[j][i] = sum_m c_m Re(sum_n x_n^m Pbar_n^m(mu_j) exp(i m lambda_i)), c_0 = 1, c_m = 2
    otherwise -> plane [n_lat][n_lon] f64 (with extended=True computed in extended precision and rounded once)."""
    coef = np.asarray(coef, dtype=np.complex128)
    N, n = g.N, g.n_lon
    if coef.shape != (N + 1, N + 1):
        raise ValueError(f"synthesise: coef is [{N + 1}][{N + 1}], x_n^m at [m][n]")
    kind = flow._kind(extended)
    tc, ts = flow._twiddles(n, kind)
    cr, ci = flow._conv(coef.real, kind), flow._conv(coef.imag, kind)
    out = None
    for m in range(N + 1):
        P = legendre(g, m, extended)                          # [n][j]
        fr, fi = cr[m].dot(P), ci[m].dot(P)                   # F_j(m) = sum_n x_n^m Pbar_n^m(mu_j)
        idx = (np.arange(n) * m) % n
        term = fr[:, None] * tc[idx][None, :] - fi[:, None] * ts[idx][None, :]
        term = term if m == 0 else term + term
        out = term if out is None else out + term
    return _round(out)


def bin_weights(N):
    c = np.full(int(N) + 1, 2.0)
    c[0] = 1.0
    return c


def power_reference(coef, plane=None, g=None):
    """The device's order, restated bit for bit.  coef [m][n] -> P [N + 1]: per n, from +0.0, m ascending,
    P = P + c_m * (re * re + im * im) (every product and sum rounded; the build has -ffp-contract=off).  With the plane and the
    tables also (P, ms, bad rows): per row the sum of x^2 in the lane order of series.reduce_reference, divided by n (NaN on a
    row that holds a non-finite value); across rows lane l of 64 takes the rows l, l + 64, ... ascending, acc = acc + w_j ms_j, the
    five halvings of csrc/qd_blockred.h, ms = 0.5 acc."""
    coef = np.asarray(coef, dtype=np.complex128)
    N = coef.shape[0] - 1
    c = bin_weights(N)
    re, im = np.ascontiguousarray(coef.real), np.ascontiguousarray(coef.imag)
    with np.errstate(all="ignore"):
        P = np.zeros(N + 1)
        for m in range(N + 1):
            P = P + c[m] * (re[m] * re[m] + im[m] * im[m])   # (n < m: the coefficient is +0, and P never holds -0)
        if plane is None:
            return P
        x = np.ascontiguousarray(plane, dtype=np.float64)
        bad = ~np.isfinite(x).all(axis=1)
        msrow = np.where(bad, np.nan, flow._row_sums(x * x) / np.float64(g.n_lon))
        rows = order.lanes(g.w * msrow, 64, 0.0)
        acc = np.zeros(64)
        for k in range(rows.shape[0]):
            acc = acc + rows[k]
        return P, 0.5 * float(order.wave(acc, np.add)), int(bad.sum())


def resid(P, ms):
    """1 - sum_n P(n) / ms, NaN where ms is 0."""
    P, ms = np.asarray(P, dtype=np.float64), np.asarray(ms, dtype=np.float64)
    with np.errstate(invalid="ignore", divide="ignore"):
        return np.where(ms == 0.0, np.nan, 1.0 - P.sum(axis=-1) / np.where(ms == 0.0, 1.0, ms))


def ke_spectra(P_vort, P_div, radius):
    """(ke, ke_rot, ke_div) [..., N + 1] from the powers of zeta and delta: a^2 P(n) / (2 n (n + 1)) for n >= 1, 0 at n = 0."""
    Pz, Pd = np.asarray(P_vort, dtype=np.float64), np.asarray(P_div, dtype=np.float64)
    n = np.arange(Pz.shape[-1], dtype=np.float64)
    f = np.zeros_like(n)
    f[1:] = np.float64(radius) ** 2 / (2.0 * n[1:] * (n[1:] + 1.0))
    rot, div = Pz * f, Pd * f
    return rot + div, rot, div


def ke_slope(ke):
    """The least-squares slope of log ke on log n over 8 <= n <= N / 2, per record; NaN when fewer than 4 positive bins lie there."""
    ke = np.asarray(ke, dtype=np.float64).reshape(-1, np.shape(ke)[-1])
    N = ke.shape[1] - 1
    out = np.full(len(ke), np.nan)
    n = np.arange(8, N // 2 + 1)
    for k, row in enumerate(ke):
        v = row[8:N // 2 + 1]
        ok = np.isfinite(v) & (v > 0.0)
        if ok.sum() >= 4:
            out[k] = np.polyfit(np.log(n[ok].astype(np.float64)), np.log(v[ok]), 1)[0]
    return out


def record_width(n_entries, N):
    return int(n_entries) * (int(N) + 1 + STATS)


def split_records(recs, n_entries, N):
    """[n][width] records -> (power [n][n_entries][N + 1], ms [n][n_entries], bad_rows [n][n_entries])."""
    r = np.asarray(recs, dtype=np.float64).reshape(-1, int(n_entries), int(N) + 1 + STATS)
    return r[:, :, :N + 1], r[:, :, N + 1], r[:, :, N + 2]


def analyse_grid(n_lat, n_lon, plane, device=0):
    """The device's kernels on a host plane without a handle (qd_spharm_analyse_grid: any grid with N >= 1; qd_create needs five
    rows) -> namespace(coef [m][n] complex, rec [N + 1 + STATS])."""
    from . import _lib
    g = tables(n_lat, n_lon)
    lib = _lib.load()
    x = np.ascontiguousarray(plane, dtype=np.float64)
    if x.shape != (g.n_lat, g.n_lon):
        raise ValueError(f"analyse_grid: the plane is [{g.n_lat}][{g.n_lon}]")
    re, im, rec = np.empty((g.N + 1, g.N + 1)), np.empty((g.N + 1, g.N + 1)), np.empty(g.N + 1 + STATS)
    _lib.call(lib, "qd_spharm_analyse_grid", (g.n_lat, g.n_lon, device, g.N, g.w, g.mu, g.seed_pairs, g.A, g.B, x, re, im, rec),
              last_error=lambda: lib.qd_last_error(None))
    return types.SimpleNamespace(coef=re + 1j * im, rec=rec)


# ------------------------------------------------------------------------------------- environment
def parse_fields(text):
    """QD_SPHARM_FIELDS -> upper-cased names, in order: history's names and VORT, DIV; an unknown name, or more than 32, raises a
    ValueError that names it."""
    names = [s.strip().upper() for s in str(text).split(",") if s.strip()]
    for n in names:
        if n not in OWN and n not in history.FIELDS and n not in history.DERIVED:
            raise ValueError(f"{FIELDS_VAR}: unknown field '{n}' (an f64 plane as Device.get takes it, WIND_SPEED, CURRENT_SPEED, VORT or DIV)")
    if len(names) > C["QD_SPHARM_MAX_ENTRIES"]:
        raise ValueError(f"{FIELDS_VAR}: {len(names)} entries, at most {C['QD_SPHARM_MAX_ENTRIES']}")
    return names


def read_env(env):
    """-> dict: enabled (QD_SPHARM, default 0), every (QD_SPHARM_EVERY, default 24; unparsable or < 1 -> 24), two_d (QD_SPHARM_2D,
    default 1), every_days (QD_SPHARM_EVERY_DAYS, default 10; unparsable or <= 0 -> 10), fields (QD_SPHARM_FIELDS parsed, or None =
    VORT,DIV,H)."""
    enabled = env_int(env, "QD_SPHARM", 0) == 1
    text = env.get(FIELDS_VAR)
    fields = parse_fields(text) if (enabled and text is not None and str(text).strip()) else None
    return {"enabled": enabled, "every": env_every(env, "QD_SPHARM_EVERY", EVERY), "two_d": env_int(env, "QD_SPHARM_2D", TWO_D) != 0,
            "every_days": env_days(env, "QD_SPHARM_EVERY_DAYS", EVERY_DAYS), "fields": fields}


def resolve_fields(fields, with_ocean):
    """The run's entry names: VORT,DIV,H, or the named ones under history's ocean-only rule."""
    if fields is None:
        return list(DEFAULT_FIELDS)
    for n in fields:
        if n in history.OCEAN_ONLY and not with_ocean:
            raise ValueError(f"{FIELDS_VAR}: field '{n}' needs the ocean, which is off in this run (QD_USE_OCEAN)")
    return list(fields)


def entries_for(names):
    """names -> [(op, a, b)] as Device.spharm_configure takes them: history's entries, and (QD_SPHARM_OP_VORT / _DIV, None, None)."""
    return [(OWN[n], None, None) if n in OWN else history.entries_for([n])[0] for n in names]


def file_name(a_days, b_days, decimals=1):
    return window_file_name("spharm", a_days, b_days, decimals)


def window_variables(names, recs, times, steps, N, dt, every, complete, radius, sums=None, count=0):
    """One window as ncio.write_nc takes it -> (dims, variables).  recs [n][width], times [n] s, steps [n] run-local indices; sums
    [n_entries][N + 1 (n)][N + 1 (m)] with their sample count under QD_SPHARM_2D=1, else None."""
    N = int(N)
    n = int(np.shape(recs)[0])
    power, ms, bad = split_records(recs, len(names), N)
    v = {"time_seconds": ("f8", ("time",), np.asarray(times, dtype=np.float64).reshape(n)),
         "step": (i8_code(), ("time",), np.asarray(steps, dtype=np.int64).reshape(n)),
         "degree": ("f8", ("n",), np.arange(N + 1, dtype=np.float64))}
    for q, name in enumerate(names):
        low = name.lower()
        v[f"{low}_power"] = ("f8", ("time", "n"), np.ascontiguousarray(power[:, q, :]))
        v[f"{low}_meansq"] = ("f8", ("time",), np.ascontiguousarray(ms[:, q]))
        v[f"{low}_resid"] = ("f8", ("time",), np.ascontiguousarray(resid(power[:, q, :], ms[:, q])))
        v[f"{low}_bad_rows"] = ("i4", ("time",), bad[:, q].astype(np.int32))
        if sums is not None:
            with np.errstate(invalid="ignore", divide="ignore"):
                v[f"{low}_power_nm"] = ("f8", ("n", "m"), np.asarray(sums[q], dtype=np.float64) / np.float64(count))
    if "VORT" in names and "DIV" in names:
        ke, rot, div = ke_spectra(power[:, names.index("VORT"), :], power[:, names.index("DIV"), :], radius)
        v["ke_power"], v["ke_rot_power"], v["ke_div_power"] = (("f8", ("time", "n"), np.ascontiguousarray(x)) for x in (ke, rot, div))
        v["ke_slope"] = ("f8", ("time",), ke_slope(ke))
    v.update(truncation=("i4", (), N), dt_seconds=("f8", (), float(dt)), sample_every=("i4", (), int(every)),
             n_samples=("i4", (), n), complete=("i4", (), 1 if complete else 0))
    return {"time": n, "n": N + 1, "m": N + 1}, v


class Spharm(LogWindowLane):
    """The lane's participant in Device.step_n (like Spectra): the clock and the span protocol are window_lane's, flush() writes the
    window's file.  drop() forgets the delivered records, _pending, and on the device the log, the sums and their sample count."""
    NAME, TAG = "spharm", "SphSpec"

    def __init__(self, dev, grid, cfg, with_ocean=True, dt=300.0, day=None, out=print, output_dir=None):
        self.names = resolve_fields(cfg.get("fields"), with_ocean)
        self.two_d = bool(cfg["two_d"])
        self.tables = grid_tables(grid)                  # (a grid with N < 1 is refused here)
        self.N = self.tables.N
        self.radius = float(dev.params.a)
        super().__init__(dev, grid, cfg, out, dt, day, cfg["every_days"], cfg["every"], record_width(len(self.names), self.N), output_dir)
        needs_flow = any(n in OWN for n in self.names)
        dev.spharm_configure(entries_for(self.names), self.two_d, self.tables,
                             flow.grid_tables(grid, dev.params.a) if needs_flow else None)

    def key(self):
        """What a checkpoint's subsystem set says of this lane."""
        return f"{','.join(self.names)}|every={self.every}|2d={int(self.two_d)}"

    def _upload(self, flags):
        self.dev.spharm_schedule(flags)

    def _drain(self, want):
        return self.dev.spharm_log(want)

    def sums(self):
        """The 2D sum planes as they stand on the device -> (sums [n_entries][N + 1 (n)][N + 1 (m)], count), or (None, 0)."""
        return self.dev.spharm_sums() if self.two_d else (None, 0)

    def restore_window(self, recs, times, steps, i, sums=None, count=0):
        """The inverse of window(), sums() and the clock, for an exact resume (checkpoint.py)."""
        super().restore_window(recs, times, steps, i)
        if self.two_d and sums is not None:
            self.dev.spharm_sums_set(sums, int(count))

    def _window_file(self, complete):
        recs, times, steps = self.window()
        if len(recs) == 0:
            return None
        sums, count = self.sums()
        a, b = float(times[0]) / self.day, float(times[-1]) / self.day
        dims, variables = window_variables(self.names, recs, times, steps, self.N, self.dt, self.every, complete, self.radius,
                                           sums=sums, count=count)
        d = self.decimals
        parts = []
        if "ke_slope" in variables:
            sl = variables["ke_slope"][2]
            parts.append(f"KE slope={sl[0]:.6g}→{sl[-1]:.6g}")
        for n in self.names[:6]:
            r = variables[f"{n.lower()}_resid"][2]
            parts.append(f"{n} resid={r[0]:.6g}→{r[-1]:.6g}")
        return a, b, dims, variables, f"[SphSpec] day {a:.{d}f}–{b:.{d}f}: {len(recs)} samples | " + " ".join(parts)

    def drop(self):
        super().drop()
        self._pending = []
        self.dev.spharm_reset()


def from_env(dev, grid, env, with_ocean=True, dt=None, day=None, out=print):
    """QD_SPHARM (default 0) -> a Spharm on this handle, or None: at 0 nothing is configured, allocated, scheduled or launched."""
    cfg = read_env(env)
    if not cfg["enabled"]:
        return None
    return Spharm(dev, grid, cfg, with_ocean=with_ocean, dt=env_dt(env, dt), day=day, out=out)
