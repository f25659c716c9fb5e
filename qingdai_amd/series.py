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

import numpy as np

from . import history, order
from ._lib import SERIES_STATS
from .window_lane import LogWindowLane, env_days, env_dt, env_every, env_int, i8_code, window_file_name

FIELDS_VAR = "QD_SERIES_FIELDS"
EVERY_DAYS, EVERY, ZONAL = 10.0, 1, 1
STATS = ("mean", "min", "max", "nan")          # the four leading doubles of an entry's part of a record


# ------------------------------------------------------------------------------------- the kernel's order, in NumPy (order.py)
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
        cells = order.lanes(x, 128, 0.0).reshape(n_lat, -1, 64, 2)             # [row][round k][lane][the lane's two cells]
        acc = np.zeros((n_lat, 64))
        for k in range(cells.shape[1]):
            acc = acc + cells[:, k, :, 0]
            acc = acc + cells[:, k, :, 1]
        S = order.wave(acc, np.add)                                            # [n_lat]
        zonal = S / np.float64(m)
        rows_w, rows_p = order.lanes(w, 64, 0.0), order.lanes(w * S, 64, 0.0)       # [round][lane]; a row past the end adds +0.0
        num, W = np.zeros(64), np.zeros(64)
        for k in range(rows_w.shape[0]):
            num = num + rows_p[k]
            W = W + rows_w[k]
        mean = order.wave(num, np.add) / (np.float64(m) * order.wave(W, np.add))
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
def read_env(env):
    """-> dict: enabled (QD_SERIES, default 0), every (QD_SERIES_EVERY, default 1; unparsable or < 1 -> 1), zonal (QD_SERIES_ZONAL,
    default 1), every_days (QD_SERIES_EVERY_DAYS, default 10; unparsable or <= 0 -> 10), fields (QD_SERIES_FIELDS through history's
    parser, or None = history's default list)."""
    enabled = env_int(env, "QD_SERIES", 0) == 1
    text = env.get(FIELDS_VAR)
    fields = history.parse_fields(text, var=FIELDS_VAR) if (enabled and text is not None and str(text).strip()) else None
    return {"enabled": enabled, "every": env_every(env, "QD_SERIES_EVERY", EVERY), "zonal": env_int(env, "QD_SERIES_ZONAL", ZONAL) != 0,
            "every_days": env_days(env, "QD_SERIES_EVERY_DAYS", EVERY_DAYS), "fields": fields}


def file_name(a_days, b_days, decimals=1):
    return window_file_name("series", a_days, b_days, decimals)


def window_variables(names, recs, times, steps, lat, zonal, dt, every, complete):
    """One window as ncio.write_nc takes it -> (dims, variables).  recs [n][width], times [n] s, steps [n] run-local indices."""
    lat = np.asarray(lat, dtype=np.float64).reshape(-1)
    n = int(np.shape(recs)[0])
    stats, zon = split_records(recs, len(names), lat.size, zonal)
    v = {"time_seconds": ("f8", ("time",), np.asarray(times, dtype=np.float64).reshape(n)),
         "step": (i8_code(), ("time",), np.asarray(steps, dtype=np.int64).reshape(n)),
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


class Series(LogWindowLane):
    """The lane's participant in Device.step_n (like History): the clock and the span protocol are window_lane's, flush() writes the
    window's file.  drop() forgets the delivered records only: _pending and the device log stay as they are."""
    NAME, TAG = "series", "Series"

    def __init__(self, dev, grid, cfg, with_ocean=True, dt=300.0, day=None, out=print, output_dir=None):
        self.names = history.resolve_fields(cfg.get("fields"), with_ocean, var=FIELDS_VAR)
        self.zonal = bool(cfg["zonal"])
        self.lat = np.asarray(grid.lat, dtype=np.float64).reshape(-1)
        super().__init__(dev, grid, cfg, out, dt, day, cfg["every_days"], cfg["every"], record_width(len(self.names), self.lat.size, self.zonal),
                         output_dir)
        dev.series_configure(history.entries_for(self.names), self.zonal, row_weights(self.lat))

    def key(self):
        """The lane's part of a checkpoint's subsystem set."""
        return f"{','.join(self.names)}|zonal={int(self.zonal)}|every={int(self.every)}"

    def _upload(self, flags):
        self.dev.series_schedule(flags)

    def _drain(self, want):
        return self.dev.series_log(want)

    def _window_file(self, complete):
        recs, times, steps = self.window()
        if len(recs) == 0:
            return None
        a, b = float(times[0]) / self.day, float(times[-1]) / self.day
        dims, variables = window_variables(self.names, recs, times, steps, self.lat, self.zonal, self.dt, self.every, complete)
        d = self.decimals
        stats, _ = split_records(recs, len(self.names), self.lat.size, self.zonal)
        line = (f"[Series] day {a:.{d}f}–{b:.{d}f}: {len(recs)} samples | " +
                " ".join(f"{n}={stats[0, k, 0]:.6g}→{stats[-1, k, 0]:.6g}" for k, n in list(enumerate(self.names))[:6]))
        return a, b, dims, variables, line


def from_env(dev, grid, env, with_ocean=True, dt=None, day=None, out=print):
    """QD_SERIES (default 0) -> a Series on this handle, or None: at 0 nothing is configured, allocated, scheduled or launched."""
    cfg = read_env(env)
    if not cfg["enabled"]:
        return None
    return Series(dev, grid, cfg, with_ocean=with_ocean, dt=env_dt(env, dt), day=day, out=out)
