"""
qingdai_amd/flow.py -- flow kinematics of the winds (QD_FLOW=1), host side of csrc/qd_flow.hip: relative vorticity zeta, divergence
delta, streamfunction psi and velocity potential chi.

The reference defines SphericalGrid.vorticity and .divergence and goes no further.  Here, on every sampled step of the device loop,
the resident (U, V) give zeta and delta, the two Poisson problems L psi = zeta - mean(zeta), L chi = delta - mean(delta) are solved
on the device, one record of scalars stays in the lane's device log, and psi, chi, zeta, delta are added into four resident sum
planes.  This file is the DEFINITION; the device is held to it (tests/test_gpu_flow.py).

Grid quantities (grid_tables; N = n_lat rows j, the rows 0 and N - 1 are the poles; n = n_lon columns i, periodic by index as the
reference's np.roll treats them): dphi = grid.dlat_rad, dlam = grid.dlon_rad (the reference's 2 pi / (n - 1): n dlam != 2 pi, and
the discrete system uses dlam as it is), a the planet radius, phi_j = -pi / 2 + j dphi,
    c_j = cos(deg2rad(lat_j))       c_{j+1/2} = cos(phi_j + dphi / 2)
    w_j = 2 c_j sin(dphi / 2) on the rows 1 .. N - 2,  w_P = 2 sin^2(dphi / 4) on each pole       (sum_j w_j = 2).
zeta, delta (vortdiv_reference): on the rows 1 .. N - 2 exactly SphericalGrid.vorticity(u, v) and .divergence(u, v), in the
reference's operation order.  The reference divides the pole rows by a capped cosine of 1e-6; here a pole row holds the circulation
and the outflow of the polar cap of radius dphi / 2, constant along the row: with S(x) the row sum of (x[pole] + x[next row]) / 2 in
the lane order of series.reduce_reference and val(x) = (c_half S(x)) / ((a w_P) n),
    zeta_N = +val(u),  zeta_S = -val(u),  delta_N = -val(v),  delta_S = +val(v).
The Laplacian (laplacian_reference), finite volume: on the rows 1 .. N - 2
    a^2 (L psi)[j, i] = [ dphi / (c_j dlam^2) (psi[j, i+1] - 2 psi[j, i] + psi[j, i-1])
                          + (c_{j+1/2} (psi[j+1, i] - psi[j, i]) - c_{j-1/2} (psi[j, i] - psi[j-1, i])) / dphi ] / w_j
and a pole holds one value, a^2 (L psi)_S = c_{1/2} sum_i (psi[1, i] - psi_S) / (n dphi w_P), the north pole likewise.
The solve (helmholtz_reference): mean(zeta) = sum_j w_j sum_i zeta[j, i] / (n sum_j w_j) is the part no psi can carry; it is removed
and reported.  After a row DFT Z_j(k), k = 0 .. n // 2, the zonal second difference is lam_k = -(4 / dlam^2) sin^2(pi k / n).
k >= 1: psi^ = 0 on the poles and the rows 1 .. N - 2 form a real tridiagonal system, the same for Re and Im; multiplied by w_j:
lower c_{j-1/2} / dphi, upper c_{j+1/2} / dphi, diagonal -(upper + lower) + lam_k dphi / c_j, right side a^2 w_j Z_j(k); strictly
diagonally dominant, so Thomas elimination without pivoting (one reciprocal per row) is stable.  k = 0 (all N rows, singular): with
r_l = Z_l(0) - n mean(zeta), F_j = sum_{l <= j} a^2 w_l r_l and psi^_{j+1} = psi^_j + F_j dphi / c_{j+1/2} from psi^_0 = 0; then
the w-weighted mean is removed.  An inverse row DFT gives psi; chi likewise from delta.  A non-finite value anywhere in u or v makes
psi and chi NaN in every cell: the solve couples every cell.
The record (REC; scalars_reference restates the device's reduction order bit for bit): the global means of zeta and delta, their rms
and max |.|, min and max of psi and chi, the kinetic energies sum_j w_j sum_i (u^2 + v^2) / 2 / (n sum_j w_j) of (U, V), of the
rotational wind (-dpsi / (a dphi), dpsi / (a c dlam)) and of the divergent wind (dchi / (a c dlam), dchi / (a dphi)) by centred
differences -- all three over the rows 1 .. N - 2, a pole row adds 0 --, and the count of rows of U or V that hold a non-finite value.

Windows, clock, labels and files follow the spectra lane: <QD_OUTPUT_DIR, default output>/flow/flow_day_{a}_{b}.nc.  Nothing here
touches the device at import.
"""
from __future__ import annotations

import types

import numpy as np

from . import order
from ._lib import C
from .window_lane import LogWindowLane, env_days, env_dt, env_every, env_int, i8_code, window_file_name

EVERY_DAYS, EVERY = 10.0, 24
REC = ("vort_global", "div_global", "vort_rms", "div_rms", "vort_maxabs", "div_maxabs", "psi_min", "psi_max", "chi_min", "chi_max",
       "ke", "ke_rot", "ke_div", "bad_rows")
REC_W = C["QD_FLOW_REC_W"]
PLANES = ("psi", "chi", "vort", "div")               # the sum planes, in the device's order
assert len(REC) == REC_W and [C[k] for k in ("QD_FLOW_ZETA_MEAN", "QD_FLOW_KE", "QD_FLOW_BAD")] == [0, 10, 13] and C["QD_FLOW_PLANES"] == len(PLANES)


# ------------------------------------------------------------------------------------- grid quantities
def grid_tables(grid, radius):
    """The grid quantities of the discrete system as f64 DATA, shared by the device and by both precisions of the reference ->
    namespace(n_lat, n_lon, a, dlat, dlon, c, ch, w, chd, e, aw [n_lat] each, lam [n_lon // 2 + 1], tab [6][n_lat], geom [3]):
    c = c_j, ch = c_{j+1/2} (0 in the last place), w = w_j, chd = ch / dphi, e = dphi / c_j (0 on the poles), aw = a^2 w_j."""
    lat = np.asarray(grid.lat, dtype=np.float64).reshape(-1)
    N, n = lat.size, int(np.asarray(grid.lon).size)
    if N < 3 or n < 4:
        raise ValueError("flow: the grid needs n_lat >= 3 and n_lon >= 4")
    dlat, dlon, a = np.float64(grid.dlat_rad), np.float64(grid.dlon_rad), np.float64(radius)
    c = np.cos(np.deg2rad(lat))
    phi = -np.pi / 2 + np.arange(N) * dlat
    ch = np.zeros(N)
    ch[:-1] = np.cos(phi[:-1] + dlat / 2)
    w = 2.0 * c * np.sin(dlat / 2)
    w[0] = w[-1] = 2.0 * np.sin(dlat / 4) ** 2
    e = np.zeros(N)
    e[1:-1] = dlat / c[1:-1]
    chd, aw = ch / dlat, (a * a) * w
    k = np.arange(n // 2 + 1)
    lam = -(4.0 / (dlon * dlon)) * np.sin(np.pi * k / n) ** 2
    return types.SimpleNamespace(n_lat=N, n_lon=n, a=a, dlat=dlat, dlon=dlon, c=c, ch=ch, w=w, chd=chd, e=e, aw=aw, lam=lam,
                                 tab=np.ascontiguousarray(np.stack([c, ch, w, chd, e, aw])), geom=np.array([a, dlat, dlon]))


# ------------------------------------------------------------------------------------- the device's reduction order, in NumPy
def _row_sums(x):
    """[..., n] -> [...]: the row stage of series.reduce_reference (lane l owns the cells 128 k + 2 l and 128 k + 2 l + 1)."""
    x = np.asarray(x, dtype=np.float64)
    cells = order.lanes(x, 128, 0.0).reshape(x.shape[:-1] + (-1, 64, 2))
    acc = np.zeros(x.shape[:-1] + (64,))
    for k in range(cells.shape[-3]):
        acc = acc + cells[..., k, :, 0]
        acc = acc + cells[..., k, :, 1]
    return order.wave(acc, np.add)


def _cross_mean(S, w, n):
    """The second stage of series.reduce_reference with the weights w: lane l takes the rows l, l + 64, ..."""
    rows_w, rows_p = order.lanes(w, 64, 0.0), order.lanes(w * S, 64, 0.0)
    num, W = np.zeros(64), np.zeros(64)
    for k in range(rows_w.shape[0]):
        num = num + rows_p[k]
        W = W + rows_w[k]
    return order.wave(num, np.add) / (np.float64(n) * order.wave(W, np.add))


def vortdiv_reference(u, v, g):
    """(zeta, delta) [n_lat][n_lon] as the top of this file defines them; g = grid_tables(...).  The rows 1 .. N - 2 are the
    reference's SphericalGrid.vorticity / .divergence bit for bit (its expressions, its order)."""
    u, v = (np.ascontiguousarray(x, dtype=np.float64) for x in (u, v))
    N, n = g.n_lat, g.n_lon
    if u.shape != (N, n) or v.shape != (N, n):
        raise ValueError(f"vortdiv_reference: u and v are [{N}][{n}] planes")
    with np.errstate(all="ignore"):
        cos_lat = g.c[:, None]
        pre = 1 / (g.a * np.maximum(cos_lat, 1e-6))
        dv_dlon = (np.roll(v, -1, axis=1) - np.roll(v, 1, axis=1)) / (2 * g.dlon)
        du_dlon = (np.roll(u, -1, axis=1) - np.roll(u, 1, axis=1)) / (2 * g.dlon)
        ucos, vcos = u * cos_lat, v * cos_lat
        ducos = (np.roll(ucos, -1, axis=0) - np.roll(ucos, 1, axis=0)) / (2 * g.dlat)
        dvcos = (np.roll(vcos, -1, axis=0) - np.roll(vcos, 1, axis=0)) / (2 * g.dlat)
        zeta, delta = pre * (dv_dlon - ducos), pre * (du_dlon + dvcos)
        den = (g.a * g.w[0]) * np.float64(n)
        for row, nxt, chalf, sz, sd in ((0, 1, g.ch[0], -1.0, 1.0), (N - 1, N - 2, g.ch[N - 2], 1.0, -1.0)):
            vu = (chalf * _row_sums(0.5 * (u[row] + u[nxt]))) / den
            vv = (chalf * _row_sums(0.5 * (v[row] + v[nxt]))) / den
            zeta[row, :] = sz * vu
            delta[row, :] = sd * vv
    return zeta, delta


def scalars_reference(u, v, zeta, delta, psi, chi, g):
    """The record of a sample, REC, from the planes as the device holds them, in the device's reduction order, bit for bit."""
    u, v, zeta, delta, psi, chi = (np.ascontiguousarray(x, dtype=np.float64) for x in (u, v, zeta, delta, psi, chi))
    N, n = g.n_lat, g.n_lon
    rec = np.zeros(REC_W)
    with np.errstate(all="ignore"):
        for q, x in enumerate((zeta, delta)):
            rec[q] = _cross_mean(_row_sums(x), g.w, n)
            rec[2 + q] = np.sqrt(_cross_mean(_row_sums(x * x), g.w, n))
            rec[4 + q] = np.fmax.reduce(np.abs(x).ravel(), initial=0.0)
        for q, x in enumerate((psi, chi)):
            rec[6 + 2 * q] = np.fmin.reduce(x.ravel(), initial=np.inf)
            rec[7 + 2 * q] = np.fmax.reduce(x.ravel(), initial=-np.inf)
        S = np.zeros(N)
        S[1:-1] = _row_sums(0.5 * (u[1:-1] * u[1:-1] + v[1:-1] * v[1:-1]))
        rec[10] = _cross_mean(S, g.w, n)
        ac = g.a * g.c[1:-1, None]
        for q, x in enumerate((psi, chi)):
            d_dphi = (x[2:] - x[:-2]) / (2 * g.dlat)
            d_dlam = ((np.roll(x, -1, axis=1) - np.roll(x, 1, axis=1)) / (2 * g.dlon))[1:-1]
            if q == 0:
                a_, b_ = -(d_dphi / g.a), d_dlam / ac
            else:
                a_, b_ = d_dlam / ac, d_dphi / g.a
            S = np.zeros(N)
            S[1:-1] = _row_sums(0.5 * (a_ * a_ + b_ * b_))
            rec[11 + q] = _cross_mean(S, g.w, n)
        rec[13] = float((~(np.isfinite(u).all(axis=1) & np.isfinite(v).all(axis=1))).sum())
    return rec


# ------------------------------------------------------------------------------------- the solve, in f64 and in extended precision
def _wide():
    return np.finfo(np.longdouble).nmant > np.finfo(np.float64).nmant


def _kind(extended):
    return "f64" if not extended else ("longdouble" if _wide() else "mpmath")


def _conv(x, kind):
    x = np.asarray(x, dtype=np.float64)
    if kind == "f64":
        return x
    if kind == "longdouble":
        return x.astype(np.longdouble)
    import mpmath
    return np.array([mpmath.mpf(float(t)) for t in x.ravel()], dtype=object).reshape(x.shape)


def _twiddles(n, kind):
    """cos / sin(2 pi t / n), t = 0 .. n - 1, in the working precision (f64: the extended table rounded once, as the device's)."""
    if kind == "mpmath":
        import mpmath
        mpmath.mp.prec = 80
        t = [mpmath.mpf(2 * k) / n for k in range(n)]
        return np.array([mpmath.cospi(x) for x in t], dtype=object), np.array([mpmath.sinpi(x) for x in t], dtype=object)
    if _wide():
        from .spectra import _twiddles_longdouble
        c, s = _twiddles_longdouble(n)
        return (c, s) if kind == "longdouble" else (c.astype(np.float64), s.astype(np.float64))
    ang = 2.0 * np.pi * np.arange(n) / n
    return np.cos(ang), np.sin(ang)


def _poisson(field, g, kind):
    """One of the two solves in the working precision `kind` -> (solution [n_lat][n_lon], the removed mean), both in that
    precision.  The row transforms are direct sums (i ascending through the dot product), the Thomas elimination is the device's."""
    N, n, K = g.n_lat, g.n_lon, g.n_lon // 2 + 1
    x = _conv(field, kind)
    w, aw, chd, e, lam = (_conv(t, kind) for t in (g.w, g.aw, g.chd, g.e, g.lam))
    tc, ts = _twiddles(n, kind)
    idx = (np.arange(n)[:, None] * np.arange(K)[None, :]) % n                  # [i][k]
    Cm, Sm = tc[idx], ts[idx]
    ZR, ZI = x.dot(Cm), -(x.dot(Sm))                                            # [row][k]
    one = w[0] / w[0]
    nn = one * n
    mean = (w * ZR[:, 0]).sum() / (nn * w.sum())
    PR, PI = ZR * (one * 0), ZI * (one * 0)
    # k = 0: two prefix sums from the south pole, then the weighted mean goes
    r = ZR[:, 0] - nn * mean
    Fa = np.cumsum(aw * r)
    p0 = np.concatenate([Fa[:1] * 0, np.cumsum(Fa[:-1] / chd[:-1])])
    PR[:, 0] = p0 - (w * p0).sum() / w.sum()
    # k >= 1: Thomas elimination over the rows 1 .. N - 2, every k at once
    if K > 1:
        lk = lam[1:]
        cp = np.empty((N, K - 1), dtype=PR.dtype)
        cpv, dr, di = lk * 0, lk * 0, lk * 0
        for j in range(1, N - 1):
            lo, up = chd[j - 1], chd[j]
            inv = one / ((-(up + lo) + e[j] * lk) - lo * cpv)
            cpv = up * inv
            dr = (aw[j] * ZR[j, 1:] - lo * dr) * inv
            di = (aw[j] * ZI[j, 1:] - lo * di) * inv
            cp[j], PR[j, 1:], PI[j, 1:] = cpv, dr, di
        xr, xi = lk * 0, lk * 0
        for j in range(N - 2, 0, -1):
            xr, xi = PR[j, 1:] - cp[j] * xr, PI[j, 1:] - cp[j] * xi
            PR[j, 1:], PI[j, 1:] = xr, xi
    f = np.full(K, 2.0)
    f[0] = 1.0
    if n % 2 == 0:
        f[-1] = 1.0
    f = _conv(f, kind)
    out = ((PR * f).dot(Cm.T) - (PI * f).dot(Sm.T)) / nn
    return out, mean


def helmholtz_reference(u, v, g, extended=False):
    """The definition at the top of this file -> namespace(zeta, delta, psi, chi [n_lat][n_lon], zeta_mean, div_mean), all f64.
    zeta and delta are f64 quantities (vortdiv_reference); the two solves run in f64, or with extended=True in extended precision
    (np.longdouble where it is wider than f64, mpmath at 80 bits elsewhere) on the same f64 grid tables, rounded once at the end."""
    zeta, delta = vortdiv_reference(u, v, g)
    kind = _kind(extended)
    bad = not (np.isfinite(np.asarray(u, dtype=np.float64)).all() and np.isfinite(np.asarray(v, dtype=np.float64)).all())
    out = {}
    with np.errstate(all="ignore"):
        for name, field in (("psi", zeta), ("chi", delta)):
            if bad:
                out[name], out[name + "_m"] = np.full(zeta.shape, np.nan), np.nan
                continue
            sol, mean = _poisson(field, g, kind)
            out[name] = np.array(sol, dtype=np.float64) if kind != "mpmath" else np.array([[float(t) for t in row] for row in sol])
            out[name + "_m"] = float(mean)
    return types.SimpleNamespace(zeta=zeta, delta=delta, psi=out["psi"], chi=out["chi"], zeta_mean=out["psi_m"], div_mean=out["chi_m"])


def laplacian_reference(psi, g):
    """L psi [n_lat][n_lon] in f64, as the top of this file states it (a pole row holds the pole's one value, taken from column 0)."""
    p = np.asarray(psi, dtype=np.float64)
    N, n = g.n_lat, g.n_lon
    out = np.empty((N, n))
    zon = (np.roll(p, -1, axis=1) - 2 * p + np.roll(p, 1, axis=1))[1:-1] * (g.dlat / (g.c[1:-1, None] * g.dlon ** 2))
    mer = (g.ch[1:-1, None] * (p[2:] - p[1:-1]) - g.ch[:-2, None] * (p[1:-1] - p[:-2])) / g.dlat
    out[1:-1] = (zon + mer) / g.w[1:-1, None]
    out[0] = g.ch[0] * (p[1] - p[0, 0]).sum() / (n * g.dlat * g.w[0])
    out[-1] = g.ch[N - 2] * (p[-2] - p[-1, 0]).sum() / (n * g.dlat * g.w[-1])
    return out / (g.a * g.a)


def weighted_mean(x, g):
    """sum_j w_j sum_i x[j, i] / (n sum_j w_j)."""
    return float((g.w * np.asarray(x, dtype=np.float64).sum(axis=1)).sum() / (g.n_lon * g.w.sum()))


def solve_grid(grid, radius, u, v, device=0):
    """The device's kernels on host planes without a handle (qd_flow_solve_grid: any n_lat >= 3, n_lon >= 4; qd_create needs five
    rows) -> namespace(zeta, delta, psi, chi, rec)."""
    from . import _lib
    g = grid_tables(grid, radius)
    lib = _lib.load()
    u, v = (np.ascontiguousarray(x, dtype=np.float64) for x in (u, v))
    if u.shape != (g.n_lat, g.n_lon) or v.shape != u.shape:
        raise ValueError(f"solve_grid: u and v are [{g.n_lat}][{g.n_lon}] planes")
    o = [np.empty(u.shape) for _ in range(4)]
    rec = np.empty(REC_W)
    _lib.call(lib, "qd_flow_solve_grid", (g.n_lat, g.n_lon, device, g.tab, g.lam, g.geom, u, v, o[0], o[1], o[2], o[3], rec),
              last_error=lambda: lib.qd_last_error(None))
    return types.SimpleNamespace(zeta=o[0], delta=o[1], psi=o[2], chi=o[3], rec=rec)


# ------------------------------------------------------------------------------------- environment
def read_env(env):
    """-> dict: enabled (QD_FLOW, default 0), every (QD_FLOW_EVERY, default 24: ten samples per planet-day at the default 300 s step;
    unparsable or < 1 -> 24), every_days (QD_FLOW_EVERY_DAYS, default 10; unparsable or <= 0 -> 10)."""
    return {"enabled": env_int(env, "QD_FLOW", 0) == 1, "every": env_every(env, "QD_FLOW_EVERY", EVERY),
            "every_days": env_days(env, "QD_FLOW_EVERY_DAYS", EVERY_DAYS)}


def file_name(a_days, b_days, decimals=1):
    return window_file_name("flow", a_days, b_days, decimals)


def window_variables(recs, times, steps, lat, lon, dt, every, complete, sums, count):
    """One window as ncio.write_nc takes it -> (dims, variables).  recs [n][REC_W], times [n] s, steps [n] run-local indices, sums
    [4][n_lat][n_lon] with their sample count."""
    lat, lon = (np.asarray(x, dtype=np.float64).reshape(-1) for x in (lat, lon))
    recs = np.asarray(recs, dtype=np.float64).reshape(-1, REC_W)
    n = len(recs)
    v = {"time_seconds": ("f8", ("time",), np.asarray(times, dtype=np.float64).reshape(n)),
         "step": (i8_code(), ("time",), np.asarray(steps, dtype=np.int64).reshape(n)),
         "lat": ("f8", ("lat",), lat), "lon": ("f8", ("lon",), lon)}
    with np.errstate(invalid="ignore", divide="ignore"):
        for q, name in enumerate(PLANES):
            v[f"{name}_mean"] = ("f8", ("lat", "lon"), np.asarray(sums[q], dtype=np.float64) / np.float64(count))
    for q, name in enumerate(REC[:-1]):
        v[name] = ("f8", ("time",), np.ascontiguousarray(recs[:, q]))
    v[REC[-1]] = ("i4", ("time",), recs[:, -1].astype(np.int32))
    v.update(dt_seconds=("f8", (), float(dt)), sample_every=("i4", (), int(every)), n_samples=("i4", (), n),
             complete=("i4", (), 1 if complete else 0))
    return {"time": n, "lat": int(lat.size), "lon": int(lon.size)}, v


class Flow(LogWindowLane):
    """The lane's participant in Device.step_n (like Spectra): the clock and the span protocol are window_lane's, flush() writes the
    window's file.  drop() forgets the delivered records, _pending, and on the device the log, the sums and their sample count."""
    NAME, TAG = "flow", "Flow"

    def __init__(self, dev, grid, cfg, dt=300.0, day=None, out=print, output_dir=None):
        super().__init__(dev, grid, cfg, out, dt, day, cfg["every_days"], cfg["every"], REC_W, output_dir)
        self.lat = np.asarray(grid.lat, dtype=np.float64).reshape(-1)
        self.lon = np.asarray(grid.lon, dtype=np.float64).reshape(-1)
        self.tables = grid_tables(grid, dev.params.a)
        dev.flow_configure(self.tables)

    def key(self):
        """The lane's part of a checkpoint's subsystem set."""
        return f"every={int(self.every)}"

    def _upload(self, flags):
        self.dev.flow_schedule(flags)

    def _drain(self, want):
        return self.dev.flow_log(want)

    def sums(self):
        """The sum planes as they stand on the device -> (sums [4][n_lat][n_lon], count)."""
        return self.dev.flow_sums()

    def restore_window(self, recs, times, steps, i, sums=None, count=0):
        """The inverse of window(), sums() and the clock, for an exact resume (checkpoint.py)."""
        super().restore_window(recs, times, steps, i)
        if sums is not None:
            self.dev.flow_sums_set(sums, int(count))

    def _window_file(self, complete):
        recs, times, steps = self.window()
        if len(recs) == 0:
            return None
        sums, count = self.sums()
        a, b = float(times[0]) / self.day, float(times[-1]) / self.day
        dims, variables = window_variables(recs, times, steps, self.lat, self.lon, self.dt, self.every, complete, sums, count)
        d, k = self.decimals, {name: q for q, name in enumerate(REC)}
        line = (f"[Flow] day {a:.{d}f}–{b:.{d}f}: {len(recs)} samples | vort rms={recs[0, k['vort_rms']]:.6g}→{recs[-1, k['vort_rms']]:.6g} "
                f"div rms={recs[0, k['div_rms']]:.6g}→{recs[-1, k['div_rms']]:.6g} KE={recs[-1, k['ke']]:.6g} "
                f"rot={recs[-1, k['ke_rot']]:.6g} div={recs[-1, k['ke_div']]:.6g} bad={int(recs[:, k['bad_rows']].sum())}")
        return a, b, dims, variables, line

    def drop(self):
        super().drop()
        self._pending = []
        self.dev.flow_reset()


def from_env(dev, grid, env, dt=None, day=None, out=print):
    """QD_FLOW (default 0) -> a Flow on this handle, or None: at 0 nothing is configured, allocated, scheduled or launched."""
    cfg = read_env(env)
    if not cfg["enabled"]:
        return None
    return Flow(dev, grid, cfg, dt=env_dt(env, dt), day=day, out=out)
