"""
qingdai_amd/spectra.py -- zonal wavenumber spectra (QD_SPECTRA=1), host side of csrc/qd_spectra.hip.

Nothing the reference has built: its plan for the scale-selective filters asks for a high-wavenumber variance ratio and KE
spectra, and built neither.  On every sampled step of the device loop each selected field is transformed on the device, row by row,
to its one-sided zonal variance spectrum

    P_j(k) = c_k |X_j(k)|^2 / n^2,   X_j(k) = sum_i x[j][i] exp(-2 pi i ik / n),   k = 0 .. kN = n // 2,   n = n_lon,
    c_k = 1 for k = 0 and for k = n / 2 of an even n, 2 otherwise                  (Parseval: sum_k P_j(k) = mean_i x[j][i]^2)

and the rows are combined with the weights w_j = max(cos lat_j, 0) (series.row_weights) to P(k) = sum_j w_j P_j(k) / sum_j w_j.  A
row that holds a non-finite value is NaN in every bin, makes P NaN in every bin, and is counted.  One record per sampled step --
per entry P(0 .. kN) and the count of non-finite rows -- stays in the lane's device log until the span ends (a span lane without a
flag bit, like the series); under QD_SPECTRA_LAT=1 (the default) the P_j(k) are also added into resident sum planes, read when a
window ends.  span_deliver drains the records into the open window, and behind a window's last step the window is written to
<QD_OUTPUT_DIR, default output>/spectra/spectra_day_{a}_{b}.nc.  The window clock and the labels are history's: window k is the
steps [k S, (k + 1) S) of the run-local step index, S = max(1, int(QD_SPECTRA_EVERY_DAYS * day / dt + 0.5)), every
QD_SPECTRA_EVERY-th step of a window is sampled, counted from the window's first step.

dft_reference is the definition in extended precision; combine_reference is the NumPy restatement of the device's cross-row order
(the top of csrc/qd_spectra.hip), bit for bit; hi_frac is the high-band variance share of the window file.  Nothing here touches
the device at import.
"""
from __future__ import annotations

import functools
import math

import numpy as np

from . import history, order, series
from ._lib import SPECTRA_STATS
from .window_lane import LogWindowLane, env_days, env_dt, env_every, env_int, i8_code, window_file_name

FIELDS_VAR = "QD_SPECTRA_FIELDS"
DEFAULT_FIELDS = ("U", "V", "H", "Q", "CLOUD")     # what the hyperdiffusion acts on
EVERY_DAYS, EVERY, LAT = 10.0, 24, 1


def n_bins(n_lon):
    return int(n_lon) // 2 + 1


def bin_weights(n_lon):
    """c_k: 1 for k = 0 and for k = n / 2 of an even n, 2 otherwise."""
    n = int(n_lon)
    c = np.full(n_bins(n), 2.0)
    c[0] = 1.0
    if n % 2 == 0:
        c[-1] = 1.0
    return c


# ------------------------------------------------------------------------------------- the definition, in extended precision
def _wide():
    return np.finfo(np.longdouble).nmant > np.finfo(np.float64).nmant


@functools.lru_cache(maxsize=8)
def _twiddles_longdouble(n):
    """cos / sin(2 pi t / n), t = 0 .. n - 1, as longdouble, with the octant symmetries exact: arguments are folded into
    [0, pi / 4], so cos(2 pi m t / n) sampled from this table is exactly +-1, 0 or +-1/2 where the true value is."""
    ld = np.longdouble
    pi = ld(4) * np.arctan(ld(1))
    c, s = np.empty(n, dtype=ld), np.empty(n, dtype=ld)
    for t in range(n):
        # angle = 2 pi t / n = (pi / 4) * (8 t / n): octant o, remainder r / n of an octant
        o, r = divmod(8 * t, n)
        if o % 2 == 0:
            a = pi * ld(r) / ld(4 * n)
        else:
            a = pi * ld(n - r) / ld(4 * n)
        ca, sa = np.cos(a), np.sin(a)
        if r == 0 and o % 2 == 0:
            ca, sa = ld(1), ld(0)
        cc, ss = [(ca, sa), (sa, ca), (-sa, ca), (-ca, sa), (-ca, -sa), (-sa, -ca), (sa, -ca), (ca, -sa)][o]
        c[t], s[t] = cc, ss
    return c, s


def _dft_longdouble(x):
    n_lat, n = x.shape
    kN = n // 2
    c, s = _twiddles_longdouble(n)
    xl = x.astype(np.longdouble)
    i = np.arange(n, dtype=np.int64)
    re = np.empty((n_lat, kN + 1), dtype=np.longdouble)
    im = np.empty((n_lat, kN + 1), dtype=np.longdouble)
    for k in range(kN + 1):
        idx = (i * k) % n
        re[:, k] = xl @ c[idx]
        im[:, k] = -(xl @ s[idx])
    return re, im


def _dft_mpmath(x):
    import mpmath
    mpmath.mp.prec = 80
    n_lat, n = x.shape
    kN = n // 2
    tw = [mpmath.expjpi(mpmath.mpf(-2 * t) / n) for t in range(n)]
    re = np.empty((n_lat, kN + 1), dtype=object)
    im = np.empty((n_lat, kN + 1), dtype=object)
    for j in range(n_lat):
        row = [mpmath.mpf(float(v)) for v in x[j]]
        for k in range(kN + 1):
            z = mpmath.fsum(row[i] * tw[(i * k) % n] for i in range(n))
            re[j, k], im[j, k] = z.real, z.imag
    return re, im


def dft_reference(plane, parts=False):
    """The definition at the top of this file for a plane [n_lat][n_lon] (or one row [n_lon]) in extended precision ->
    P [n_lat][n_bins] as f64 (the extended result rounded once), or with parts=True (P, Re X, Im X), all f64.  np.longdouble where
    it is wider than f64 (x87: a 63-bit fraction), mpmath at 80 bits elsewhere.  A row that holds a non-finite value is NaN in
    every bin."""
    x = np.asarray(plane, dtype=np.float64)
    one = x.ndim == 1
    x = np.ascontiguousarray(x.reshape(1, -1) if one else x)
    n = x.shape[1]
    bad = ~np.isfinite(x).all(axis=1)
    xs = np.where(bad[:, None], 0.0, x)
    with np.errstate(all="ignore"):
        if _wide():
            re, im = _dft_longdouble(xs)
            P = (re * re + im * im) * bin_weights(n).astype(np.longdouble) / (np.longdouble(n) * np.longdouble(n))
        else:
            import mpmath
            re, im = _dft_mpmath(xs)
            c = bin_weights(n)
            P = np.array([[(re[j, k] ** 2 + im[j, k] ** 2) * mpmath.mpf(c[k]) / (n * n) for k in range(re.shape[1])] for j in range(len(re))],
                         dtype=object)
        P, re, im = (np.array(a, dtype=np.float64) for a in (P, re, im))
    for a in (P, re, im):
        a[bad] = np.nan
    if one:
        P, re, im = P[0], re[0], im[0]
    return (P, re, im) if parts else P


# ------------------------------------------------------------------------------------- the kernel's cross-row order, in NumPy
def combine_reference(P_rows, lat):
    """The global spectrum in the device's order: P_rows [n_lat][n_bins] per-row powers, lat [n_lat] degrees -> P [n_bins].
    Per bin, lane l of 64 takes the rows l, l + 64, ... in ascending order, num += w_j * P_j(k) (the product rounded), W += w_j,
    both from +0.0; then the five halvings of csrc/qd_blockred.h; P(k) = num / W.  This is the second stage of
    series.reduce_reference applied per bin.  (A row past the end is no add on the device and an add of +0.0 here: an accumulator
    that starts at +0.0 and takes non-negative or NaN terms never holds -0.0.)"""
    P = np.ascontiguousarray(P_rows, dtype=np.float64)
    w = series.row_weights(lat)
    if P.ndim != 2 or w.size != P.shape[0]:
        raise ValueError("combine_reference: P_rows is [n_lat][n_bins], lat holds one latitude per row")
    with np.errstate(invalid="ignore", over="ignore"):
        prod = (w[:, None] * P).T                                             # [bin][row]
        rows_p = order.lanes(prod, 64, 0.0)                                 # [bin][round][lane]
        rows_w = order.lanes(w, 64, 0.0)                                    # [round][lane]
        num, W = np.zeros((P.shape[1], 64)), np.zeros(64)
        for k in range(rows_w.shape[0]):
            num = num + rows_p[:, k, :]
            W = W + rows_w[k]
        return order.wave(num, np.add) / order.wave(W, np.add)


def hi_frac(P):
    """The high-band variance share of spectra P [..., n_bins]: sum_{k >= ceil(0.75 kN)} P(k) / sum_{k >= 1} P(k), the
    "upper-quartile band" ratio of the reference's plan for its filters; NaN where the denominator is 0 (or kN = 0)."""
    P = np.asarray(P, dtype=np.float64)
    kN = P.shape[-1] - 1
    k0 = max(1, int(math.ceil(0.75 * kN)))
    with np.errstate(invalid="ignore", divide="ignore"):
        den = P[..., 1:].sum(axis=-1)
        num = P[..., k0:].sum(axis=-1)
        return np.where(den == 0.0, np.nan, num / np.where(den == 0.0, 1.0, den))


def record_width(n_entries, n_lon):
    return int(n_entries) * (n_bins(n_lon) + SPECTRA_STATS)


def split_records(recs, n_entries, n_lon):
    """[n][width] records -> (power [n][n_entries][n_bins], bad_rows [n][n_entries])."""
    nb = n_bins(n_lon)
    r = np.asarray(recs, dtype=np.float64).reshape(-1, int(n_entries), nb + SPECTRA_STATS)
    return r[:, :, :nb], r[:, :, nb]


# ------------------------------------------------------------------------------------- environment
def read_env(env):
    """-> dict: enabled (QD_SPECTRA, default 0), every (QD_SPECTRA_EVERY, default 24: ten samples per planet-day at the default
    300 s step; unparsable or < 1 -> 24), lat (QD_SPECTRA_LAT, default 1), every_days (QD_SPECTRA_EVERY_DAYS, default 10;
    unparsable or <= 0 -> 10), fields (QD_SPECTRA_FIELDS through history's parser, or None = U,V,H,Q,CLOUD)."""
    enabled = env_int(env, "QD_SPECTRA", 0) == 1
    text = env.get(FIELDS_VAR)
    fields = history.parse_fields(text, var=FIELDS_VAR) if (enabled and text is not None and str(text).strip()) else None
    return {"enabled": enabled, "every": env_every(env, "QD_SPECTRA_EVERY", EVERY), "lat": env_int(env, "QD_SPECTRA_LAT", LAT) != 0,
            "every_days": env_days(env, "QD_SPECTRA_EVERY_DAYS", EVERY_DAYS), "fields": fields}


def resolve_fields(fields, with_ocean):
    """The run's entry names: U,V,H,Q,CLOUD, or the named ones under history's ocean-only rule."""
    if fields is None:
        return list(DEFAULT_FIELDS)
    return history.resolve_fields(fields, with_ocean, var=FIELDS_VAR)


def file_name(a_days, b_days, decimals=1):
    return window_file_name("spectra", a_days, b_days, decimals)


def window_variables(names, recs, times, steps, lat, n_lon, dt, every, complete, sums=None, count=0):
    """One window as ncio.write_nc takes it -> (dims, variables).  recs [n][width], times [n] s, steps [n] run-local indices;
    sums [n_entries][n_lat][n_bins] with their sample count under QD_SPECTRA_LAT=1, else None."""
    lat = np.asarray(lat, dtype=np.float64).reshape(-1)
    n, nb = int(np.shape(recs)[0]), n_bins(n_lon)
    power, bad = split_records(recs, len(names), n_lon)
    v = {"time_seconds": ("f8", ("time",), np.asarray(times, dtype=np.float64).reshape(n)),
         "step": (i8_code(), ("time",), np.asarray(steps, dtype=np.int64).reshape(n)),
         "wavenumber": ("f8", ("k",), np.arange(nb, dtype=np.float64)),
         "lat": ("f8", ("lat",), lat)}
    for q, name in enumerate(names):
        low = name.lower()
        v[f"{low}_power"] = ("f8", ("time", "k"), np.ascontiguousarray(power[:, q, :]))
        v[f"{low}_bad_rows"] = ("i4", ("time",), bad[:, q].astype(np.int32))
        v[f"{low}_hi_frac"] = ("f8", ("time",), np.ascontiguousarray(hi_frac(power[:, q, :])))
        if sums is not None:
            with np.errstate(invalid="ignore", divide="ignore"):
                v[f"{low}_power_lat"] = ("f8", ("lat", "k"), np.asarray(sums[q], dtype=np.float64) / np.float64(count))
    if "U" in names and "V" in names:
        v["ke_power"] = ("f8", ("time", "k"), 0.5 * (power[:, names.index("U"), :] + power[:, names.index("V"), :]))
    v.update(dt_seconds=("f8", (), float(dt)), sample_every=("i4", (), int(every)), lat_resolved=("i4", (), 1 if sums is not None else 0),
             n_samples=("i4", (), n), complete=("i4", (), 1 if complete else 0))
    return {"time": n, "k": nb, "lat": int(lat.size)}, v


class Spectra(LogWindowLane):
    """The lane's participant in Device.step_n (like Series): the clock and the span protocol are window_lane's, flush() writes the
    window's file.  drop() forgets the delivered records, _pending, and on the device the log, the sums and their sample count."""
    NAME, TAG = "spectra", "Spectra"

    def __init__(self, dev, grid, cfg, with_ocean=True, dt=300.0, day=None, out=print, output_dir=None):
        self.names = resolve_fields(cfg.get("fields"), with_ocean)
        self.lat_resolved = bool(cfg["lat"])
        self.lat = np.asarray(grid.lat, dtype=np.float64).reshape(-1)
        self.n_lon = int(np.asarray(grid.lon).size)
        super().__init__(dev, grid, cfg, out, dt, day, cfg["every_days"], cfg["every"], record_width(len(self.names), self.n_lon), output_dir)
        dev.spectra_configure(history.entries_for(self.names), self.lat_resolved, series.row_weights(self.lat))

    def key(self):
        """The lane's part of a checkpoint's subsystem set."""
        return f"{','.join(self.names)}|every={int(self.every)}|lat={int(self.lat_resolved)}"

    def _upload(self, flags):
        self.dev.spectra_schedule(flags)

    def _drain(self, want):
        return self.dev.spectra_log(want)

    def sums(self):
        """The lat-resolved sum planes as they stand on the device -> (sums [n_entries][n_lat][n_bins], count), or (None, 0)."""
        return self.dev.spectra_sums() if self.lat_resolved else (None, 0)

    def restore_window(self, recs, times, steps, i, sums=None, count=0):
        """The inverse of window(), sums() and the clock, for an exact resume (checkpoint.py)."""
        super().restore_window(recs, times, steps, i)
        if self.lat_resolved and sums is not None:
            self.dev.spectra_sums_set(sums, int(count))

    def _window_file(self, complete):
        recs, times, steps = self.window()
        if len(recs) == 0:
            return None
        sums, count = self.sums()
        a, b = float(times[0]) / self.day, float(times[-1]) / self.day
        dims, variables = window_variables(self.names, recs, times, steps, self.lat, self.n_lon, self.dt, self.every, complete,
                                           sums=sums, count=count)
        d = self.decimals
        power, _ = split_records(recs, len(self.names), self.n_lon)
        hf = hi_frac(power)                                                   # [time][entry]
        line = (f"[Spectra] day {a:.{d}f}–{b:.{d}f}: {len(recs)} samples | " +
                " ".join(f"{n} hi={hf[0, k]:.6g}→{hf[-1, k]:.6g}" for k, n in list(enumerate(self.names))[:6]))
        return a, b, dims, variables, line

    def drop(self):
        super().drop()
        self._pending = []
        self.dev.spectra_reset()


def from_env(dev, grid, env, with_ocean=True, dt=None, day=None, out=print):
    """QD_SPECTRA (default 0) -> a Spectra on this handle, or None: at 0 nothing is configured, allocated, scheduled or launched."""
    cfg = read_env(env)
    if not cfg["enabled"]:
        return None
    return Spectra(dev, grid, cfg, with_ocean=with_ocean, dt=env_dt(env, dt), day=day, out=out)
