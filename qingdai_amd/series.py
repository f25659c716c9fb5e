"""
qingdai_amd/series.py -- per-step time series and zonal means (QD_SERIES=1), host side of csrc/qd_series.hip.

Nothing the reference has.  On every sampled step of the device loop each selected field is reduced on the device to a record --
a cos-latitude-weighted global mean, a minimum, a maximum, a NaN count and (QD_SERIES_ZONAL=1, the default) the zonal mean of every
latitude row -- in a span lane without a flag bit, like the history accumulators: a schedule given before a span turns it on.  The
records stay in the lane's device log until the span ends; span_deliver drains them into the open window, and behind a window's last
step the window is written to <QD_OUTPUT_DIR, default output>/series/series_day_{a}_{b}.nc, a and b the start times over `day` of
the window's first and last sampled step.  The window clock is history's: windows are counted on the run-local step index, window k
is the steps [k S, (k + 1) S) with S = max(1, int(QD_SERIES_EVERY_DAYS * day / dt + 0.5)), and every QD_SERIES_EVERY-th step of a
window is sampled, counted from the window's first step.  A record of a field for step i is the reduction of what Device.get
returns after a span that ends with step i.

reduce_reference is the NumPy restatement of the kernel's summation order (the top of csrc/qd_series.hip), bit for bit: the only
definition of that order outside the .hip.  Nothing here touches the device at import.
"""
from __future__ import annotations

import math
import os

import numpy as np

from . import history, ncio
from ._lib import SERIES_STATS

FIELDS_VAR = "QD_SERIES_FIELDS"
EVERY_DAYS, EVERY, ZONAL = 10.0, 1, 1
STATS = ("mean", "min", "max", "nan")          # the four leading doubles of an entry's part of a record


# ------------------------------------------------------------------------------------- the kernel's order, in NumPy
def _wave(x, op):
    """The five-halving wave reduction of csrc/qd_blockred.h over the last axis (64 lanes) -> what lane 0 holds."""
    x = np.array(x, copy=True)
    o = 32
    while o > 0:
        x[..., :o] = op(x[..., :o], x[..., o:2 * o])
        o >>= 1
    return x[..., 0]


def _lanes(v, width, fill):
    """[..., m] -> [..., rounds, width]: element k * width + l is lane l's k-th; `fill` where the plane ends."""
    m = v.shape[-1]
    rounds = max(1, -(-m // width))
    out = np.full(v.shape[:-1] + (rounds * width,), fill, dtype=np.float64)
    out[..., :m] = v
    return out.reshape(v.shape[:-1] + (rounds, width))


def reduce_reference(plane, lat, n_lon=None):
    """One entry's part of a record, in the device's order -> (mean, min, max, nan_count, zonal[n_lat]).
    plane [n_lat][n_lon] f64 (for an op-1 entry: np.sqrt(a * a + b * b)); lat [n_lat] degrees, w_j = max(cos lat_j, 0).
      row stage     lane l of a row's wave owns the cells 128 k + 2 l and 128 k + 2 l + 1 and adds them in ascending order into one
                    accumulator that starts at +0.0; then the five halvings.  (A cell past the row's end is no add on the device;
                    here it is an add of +0.0, which changes no bit: an accumulator that starts at +0.0 never holds -0.0.)
      second stage  lane l takes the rows l, l + 64, ... in ascending order: num += w_j * S_j (the product rounded), W += w_j; then
                    the five halvings; mean = num / (n_lon * W).
    min and max are fmin / fmax over the same ownership; as values they do not depend on the order (the sign of a zero result
    among zeros of both signs is the hardware's choice and no part of the contract)."""
    x = np.ascontiguousarray(plane, dtype=np.float64)
    n_lat, m = x.shape
    if n_lon is not None and int(n_lon) != m:
        raise ValueError(f"reduce_reference: the plane has {m} columns, n_lon is {n_lon}")
    w = np.maximum(np.cos(np.deg2rad(np.asarray(lat, dtype=np.float64).reshape(-1))), 0.0)
    if w.size != n_lat:
        raise ValueError("reduce_reference: lat holds one latitude per row")
    with np.errstate(invalid="ignore", over="ignore"):
        cells = _lanes(x, 128, 0.0).reshape(n_lat, -1, 64, 2)             # [row][round k][lane][the lane's two cells]
        acc = np.zeros((n_lat, 64))
        for k in range(cells.shape[1]):
            acc = acc + cells[:, k, :, 0]
            acc = acc + cells[:, k, :, 1]
        S = _wave(acc, np.add)                                            # [n_lat]
        zonal = S / np.float64(m)
        rows_w, rows_p = _lanes(w, 64, 0.0), _lanes(w * S, 64, 0.0)       # [round][lane]; a row past the end adds +0.0
        num, W = np.zeros(64), np.zeros(64)
        for k in range(rows_w.shape[0]):
            num = num + rows_p[k]
            W = W + rows_w[k]
        mean = _wave(num, np.add) / (np.float64(m) * _wave(W, np.add))
    nan = np.isnan(x)
    some = not nan.all()
    return (float(mean), float(np.nanmin(x)) if some else float("nan"), float(np.nanmax(x)) if some else float("nan"),
            int(nan.sum()), zonal)


def row_weights(lat):
    """The row weights the device gets at configure time: max(cos lat, 0), history.global_mean's."""
    return np.maximum(np.cos(np.deg2rad(np.asarray(lat, dtype=np.float64).reshape(-1))), 0.0)


def record_width(n_entries, n_lat, zonal):
    return int(n_entries) * (SERIES_STATS + (int(n_lat) if zonal else 0))


def split_records(recs, n_entries, n_lat, zonal):
    """[n][width] records -> (stats [n][n_entries][4], zonal [n][n_entries][n_lat] or None)."""
    r = np.asarray(recs, dtype=np.float64).reshape(-1, int(n_entries), SERIES_STATS + (int(n_lat) if zonal else 0))
    return r[:, :, :SERIES_STATS], (r[:, :, SERIES_STATS:] if zonal else None)


# ------------------------------------------------------------------------------------- environment
def _int(env, name, default):
    try:
        return int(env.get(name, str(default)))
    except (TypeError, ValueError):
        return default


def read_env(env):
    """-> dict: enabled (QD_SERIES, default 0), every (QD_SERIES_EVERY, default 1; unparsable or < 1 -> 1), zonal (QD_SERIES_ZONAL,
    default 1), every_days (QD_SERIES_EVERY_DAYS, default 10; unparsable or <= 0 -> 10), fields (QD_SERIES_FIELDS through history's
    parser, or None = history's default list)."""
    enabled = _int(env, "QD_SERIES", 0) == 1
    every = _int(env, "QD_SERIES_EVERY", EVERY)
    if every < 1:
        every = EVERY
    try:
        days = float(env.get("QD_SERIES_EVERY_DAYS", str(EVERY_DAYS)))
    except (TypeError, ValueError):
        days = EVERY_DAYS
    if not (days > 0.0) or not math.isfinite(days):
        days = EVERY_DAYS
    text = env.get(FIELDS_VAR)
    fields = history.parse_fields(text, var=FIELDS_VAR) if (enabled and text is not None and str(text).strip()) else None
    return {"enabled": enabled, "every": every, "zonal": _int(env, "QD_SERIES_ZONAL", ZONAL) != 0, "every_days": days, "fields": fields}


def file_name(a_days, b_days, decimals=1):
    w = decimals + 3
    return f"series_day_{a_days:0{w}.{decimals}f}_{b_days:0{w}.{decimals}f}.nc"


def _i8():
    """Classic NetCDF (the scipy back end) has no 64-bit integer: the step indices, far below 2^53, are then written as f8."""
    return "i8" if ncio.backend() == "netCDF4" else "f8"


def window_variables(names, recs, times, steps, lat, zonal, dt, every, complete):
    """One window as ncio.write_nc takes it -> (dims, variables).  recs [n][width], times [n] s, steps [n] run-local indices."""
    lat = np.asarray(lat, dtype=np.float64).reshape(-1)
    n = int(np.shape(recs)[0])
    stats, zon = split_records(recs, len(names), lat.size, zonal)
    v = {"time_seconds": ("f8", ("time",), np.asarray(times, dtype=np.float64).reshape(n)),
         "step": (_i8(), ("time",), np.asarray(steps, dtype=np.int64).reshape(n)),
         "lat": ("f8", ("lat",), lat)}
    for k, name in enumerate(names):
        low = name.lower()
        for q, stat in enumerate(STATS[:3]):
            v[f"{low}_{stat}"] = ("f8", ("time",), np.ascontiguousarray(stats[:, k, q]))
        v[f"{low}_nan"] = ("i4", ("time",), stats[:, k, 3].astype(np.int32))
        if zonal:
            v[f"{low}_zonal"] = ("f8", ("time", "lat"), np.ascontiguousarray(zon[:, k, :]))
    v.update(dt_seconds=("f8", (), float(dt)), sample_every=("i4", (), int(every)), zonal=("i4", (), 1 if zonal else 0),
             complete=("i4", (), 1 if complete else 0))
    return {"time": n, "lat": int(lat.size)}, v


class Series:
    """The lane's participant in Device.step_n (like History): the run-local step index is its clock, span_schedule uploads the
    span's sample flags, span_deliver drains the span's records into the open window, flush() writes the window's file."""

    def __init__(self, dev, grid, cfg, with_ocean=True, dt=300.0, day=None, out=print, output_dir=None):
        self.dev, self.grid, self.cfg, self.out = dev, grid, dict(cfg), out
        self.dt = float(dt)
        self.day = float(2.0 * np.pi / dev.params.omega) if day is None else float(day)
        self.names = history.resolve_fields(cfg.get("fields"), with_ocean, var=FIELDS_VAR)
        self.S = history.steps_per_window(cfg["every_days"], self.day, self.dt)
        self.every = int(cfg["every"])
        self.zonal = bool(cfg["zonal"])
        self.decimals = history.label_decimals(self.S * self.dt / self.day)
        self.output_dir = output_dir
        self.lat = np.asarray(grid.lat, dtype=np.float64).reshape(-1)
        self.width = record_width(len(self.names), self.lat.size, self.zonal)
        self.i = 0                                   # run-local index of the next step
        self._pending = []                           # (times, steps) of spans that ran and whose records are still in the device log
        self.drop()
        self.files = []
        dev.series_configure(history.entries_for(self.names), self.zonal, row_weights(self.lat))

    # -- the span protocol of Device.step_n
    def span_clock(self):
        return (self.i, len(self._pending))

    def span_restore(self, clock):
        self.i = clock[0]
        del self._pending[clock[1]:]

    def span_schedule(self, t0, dt, n):
        flags = history.schedule(self.i, n, self.S, self.every)
        self.dev.series_schedule(flags)              # (more than QD_SERIES_LOG_CAP samples between two drains: qd_step_n refuses the span)
        if t0 is None:
            times = (self.i + np.arange(int(n))) * float(dt)
        elif np.ndim(t0) == 0:
            times = float(t0) + float(dt) * np.arange(int(n))
        else:
            times = np.asarray(t0, dtype=np.float64)
        hit = np.flatnonzero(flags)
        return (int(n), np.asarray(times, dtype=np.float64)[hit].copy(), (self.i + hit).astype(np.int64))

    def _fired(self, k):
        n, times, steps = k
        self.i += n
        if len(times):
            self._pending.append((times, steps))

    def span_deliver(self, dt):
        """Drain the device log into the open window -> the records [n][width] that came."""
        want = sum(len(t) for t, _ in self._pending)
        if want == 0:
            return np.empty((0, self.width))
        recs = self.dev.series_log(want)
        if len(recs) != want:
            raise RuntimeError(f"Series: the device log held {len(recs)} records where the schedule says {want}")
        self.recs.append(recs)
        for t, s in self._pending:
            self.times.append(t)
            self.steps.append(s)
        self._pending = []
        return recs

    # -- windows
    def steps_to_window_end(self, i=None):
        """Steps from step i (default: the next step) up to and including its window's last step."""
        i = self.i if i is None else int(i)
        return self.S - (i % self.S)

    def window_closed(self):
        """The last step that ran was a window's last step."""
        return self.i > 0 and self.i % self.S == 0

    def window(self):
        """The open window as delivered so far -> (recs [n][width], times [n], steps [n])."""
        if not self.recs:
            return np.empty((0, self.width)), np.empty(0), np.empty(0, dtype=np.int64)
        return np.concatenate(self.recs), np.concatenate(self.times), np.concatenate(self.steps)

    def restore_window(self, recs, times, steps, i):
        """The inverse of window() and the clock, for an exact resume (checkpoint.py)."""
        self.drop()
        recs = np.asarray(recs, dtype=np.float64).reshape(-1, self.width)
        if len(recs):
            self.recs, self.times = [recs.copy()], [np.asarray(times, dtype=np.float64).reshape(-1).copy()]
            self.steps = [np.asarray(steps).reshape(-1).astype(np.int64)]
        self.i = int(i)

    def path(self, a_days, b_days):
        out = self.output_dir if self.output_dir is not None else os.environ.get("QD_OUTPUT_DIR", "output")
        return os.path.join(out, "series", file_name(a_days, b_days, self.decimals))

    def flush(self, complete=1):
        """Write the open window's file, print one line, start the next window -> the path, or None when it holds no record."""
        recs, times, steps = self.window()
        if len(recs) == 0:
            return None
        a, b = float(times[0]) / self.day, float(times[-1]) / self.day
        path = self.path(a, b)
        dims, variables = window_variables(self.names, recs, times, steps, self.lat, self.zonal, self.dt, self.every, complete)
        os.makedirs(os.path.dirname(path), exist_ok=True)
        tmp = path + ".part"
        try:
            ncio.write_nc(tmp, dims, variables)
            os.replace(tmp, path)
        finally:
            if os.path.exists(tmp):
                os.remove(tmp)
        d = self.decimals
        stats, _ = split_records(recs, len(self.names), self.lat.size, self.zonal)
        self.out(f"[Series] day {a:.{d}f}–{b:.{d}f}: {len(recs)} samples | " +
                 " ".join(f"{n}={stats[0, k, 0]:.6g}→{stats[-1, k, 0]:.6g}" for k, n in list(enumerate(self.names))[:6]))
        self.drop()
        self.files.append(path)
        return path

    def drop(self):
        """Forget the open window's delivered records; the next sample starts the next file."""
        self.recs, self.times, self.steps = [], [], []


def from_env(dev, grid, env, with_ocean=True, dt=None, day=None, out=print):
    """QD_SERIES (default 0) -> a Series on this handle, or None: at 0 nothing is configured, allocated, scheduled or launched."""
    cfg = read_env(env)
    if not cfg["enabled"]:
        return None
    if dt is None:
        dt = float(env.get("QD_DT_SECONDS", "300"))
    return Series(dev, grid, cfg, with_ocean=with_ocean, dt=dt, day=day, out=out)
