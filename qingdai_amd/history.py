"""
qingdai_amd/history.py -- time-mean history files (QD_HISTORY=1), host side of csrc/qd_history.hip.

The reference leaves PNG snapshots, budget lines and one restart file; it has no time-mean output, so there is no reference format.
Here every selected field is added into a resident accumulator on every sampled step of the device loop (a span lane without a
flag bit, like the budget diagnostics: a schedule given before a span turns it on), and at the end of each window of
QD_HISTORY_EVERY_DAYS planet-days the sums are read, divided by the sample count once, and written to
<QD_OUTPUT_DIR, default output>/history/history_day_{a}_{b}.nc, a and b the start times over `day` of the window's first and last
sampled step.  Windows are counted on the run-local step index, which starts where the lane is enabled: window k is the steps
[k S, (k + 1) S) with S = max(1, int(days * day / dt + 0.5)), and every QD_HISTORY_SAMPLE_EVERY-th step of a window is sampled,
counted from the window's first step.  A sample of a field for step i is what Device.get returns after a span that ends with step i.

Nothing here touches the device at import; the clock and the file writing are plain NumPy (tests/test_history_cpu.py).
"""
from __future__ import annotations

import numpy as np

from ._lib import FIELDS, HISTORY_MAX_ENTRIES
from .window_lane import (SumWindowLane, env_days, env_dt, env_every, env_int, label_decimals, schedule,      # noqa: F401  (the clock's
                          steps_per_window, window_file_name)                                               # functions are re-exported)

DEFAULT_FIELDS = ("TS", "H", "U", "V", "Q", "CLOUD", "HICE", "PRECIP", "ALBEDO", "ISR", "OLR", "EFLUX", "PCOND", "W_LAND", "S_SNOW",
                  "RUNOFF", "WIND_SPEED")
DEFAULT_OCEAN_FIELDS = ("SST", "UO", "VO", "ETA", "QNET", "CURRENT_SPEED")
DERIVED = {"WIND_SPEED": ("U", "V"), "CURRENT_SPEED": ("UO", "VO")}        # sqrt(a*a + b*b)
OCEAN_ONLY = frozenset(DEFAULT_OCEAN_FIELDS)
EVERY_DAYS, SAMPLE_EVERY = 10.0, 1


def parse_fields(text, var="QD_HISTORY_FIELDS"):
    """QD_HISTORY_FIELDS (or the variable `var` names: the series lane reads its own list with this parser) -> upper-cased names,
    in order; an unknown name, or more than 32, raises a ValueError that names it."""
    names = [s.strip().upper() for s in str(text).split(",") if s.strip()]
    for n in names:
        if n not in FIELDS and n not in DERIVED:
            raise ValueError(f"{var}: unknown field '{n}' (an f64 plane as Device.get takes it, WIND_SPEED or CURRENT_SPEED)")
    if len(names) > HISTORY_MAX_ENTRIES:
        raise ValueError(f"{var}: {len(names)} entries, at most {HISTORY_MAX_ENTRIES}")
    return names


def read_env(env):
    """-> dict: enabled (QD_HISTORY, default 0), every_days (QD_HISTORY_EVERY_DAYS, default 10; unparsable or <= 0 -> 10),
    sample_every (QD_HISTORY_SAMPLE_EVERY, default 1; unparsable or < 1 -> 1), fields (QD_HISTORY_FIELDS parsed, or None = default)."""
    enabled = env_int(env, "QD_HISTORY", 0) == 1
    text = env.get("QD_HISTORY_FIELDS")
    fields = parse_fields(text) if (enabled and text is not None and str(text).strip()) else None
    return {"enabled": enabled, "every_days": env_days(env, "QD_HISTORY_EVERY_DAYS", EVERY_DAYS),
            "sample_every": env_every(env, "QD_HISTORY_SAMPLE_EVERY", SAMPLE_EVERY), "fields": fields}


def resolve_fields(fields, with_ocean, var="QD_HISTORY_FIELDS"):
    """The run's entry names: the default list (ocean fields only with the ocean) or the named ones, among which a field of a
    subsystem that is off is refused."""
    if fields is None:
        return list(DEFAULT_FIELDS) + (list(DEFAULT_OCEAN_FIELDS) if with_ocean else [])
    for n in fields:
        if n in OCEAN_ONLY and not with_ocean:
            raise ValueError(f"{var}: field '{n}' needs the ocean, which is off in this run (QD_USE_OCEAN)")
    return list(fields)


def entries_for(names):
    """names -> [(op, a, b)] as Device.history_configure takes them."""
    return [(1,) + DERIVED[n] if n in DERIVED else (0, n, None) for n in names]


def file_name(a_days, b_days, decimals=1):
    return window_file_name("history", a_days, b_days, decimals)


def global_mean(plane, lat_mesh):
    """cos-latitude-weighted mean of a map: sum(max(cos lat, 0) x) / sum(max(cos lat, 0))."""
    w = np.maximum(np.cos(np.deg2rad(lat_mesh)), 0.0)
    return float(np.sum(w * plane) / np.sum(w))


class History(SumWindowLane):
    """The lane's participant in Device.step_n (like BudgetDiag): the clock and the span protocol are window_lane's, flush() turns
    the resident sums into one file.  drop() zeroes the device's sums and count and forgets the labels."""
    NAME, TAG = "history", "History"

    def __init__(self, dev, grid, cfg, with_ocean=True, dt=300.0, day=None, out=print, output_dir=None):
        super().__init__(dev, grid, cfg, out, dt, day, cfg["every_days"], cfg["sample_every"], output_dir)
        self.names = resolve_fields(cfg.get("fields"), with_ocean)
        dev.history_configure(entries_for(self.names))

    def key(self):
        """The lane's part of a checkpoint's subsystem set."""
        return ",".join(self.names)

    def _upload(self, flags):
        self.dev.history_schedule(flags)

    def flush(self, t_first_days=None, t_last_days=None, complete=1):
        """Read the sums, divide by the sample count, write the file, print one line, reset -> the path, or None when the window
        holds no sample.  The labels default to the start times of the window's first and last sampled step."""
        return super().flush(complete, t_first_days=t_first_days, t_last_days=t_last_days)

    def _window_file(self, complete, t_first_days=None, t_last_days=None):
        sums, count = self.dev.history_read()
        if count <= 0:
            return None
        t0s = self.t_first if t_first_days is None else float(t_first_days) * self.day
        t1s = self.t_last if t_last_days is None else float(t_last_days) * self.day
        t0s, t1s = (0.0 if t0s is None else float(t0s)), (0.0 if t1s is None else float(t1s))
        a, b = t0s / self.day, t1s / self.day
        means = np.asarray(sums, dtype=np.float64) / np.float64(count)
        variables = {"lat": ("f8", ("lat",), np.asarray(self.grid.lat, dtype=np.float64)),
                     "lon": ("f8", ("lon",), np.asarray(self.grid.lon, dtype=np.float64))}
        for name, plane in zip(self.names, means):
            variables[name.lower()] = ("f8", ("lat", "lon"), plane)
        variables.update(n_samples=("i4", (), int(count)), t_start_seconds=("f8", (), t0s), t_end_seconds=("f8", (), t1s),
                         dt_seconds=("f8", (), self.dt), sample_every=("i4", (), self.sample_every), complete=("i4", (), 1 if complete else 0))
        d = self.decimals
        line = (f"[History] day {a:.{d}f}–{b:.{d}f}: {count} samples | " +
                " ".join(f"{n}={global_mean(m, self.grid.lat_mesh):.6g}" for n, m in list(zip(self.names, means))[:6]))
        return a, b, {"lat": int(self.grid.n_lat), "lon": int(self.grid.n_lon)}, variables, line

    def drop(self):
        self.dev.history_reset()
        super().drop()


def from_env(dev, grid, env, with_ocean=True, dt=None, day=None, out=print):
    """QD_HISTORY (default 0) -> a History on this handle, or None: at 0 nothing is configured, allocated, scheduled or launched."""
    cfg = read_env(env)
    if not cfg["enabled"]:
        return None
    return History(dev, grid, cfg, with_ocean=with_ocean, dt=env_dt(env, dt), day=day, out=out)
