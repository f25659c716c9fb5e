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

import math
import os

import numpy as np

from . import ncio
from ._lib import FIELDS, HISTORY_MAX_ENTRIES

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
    try:
        enabled = int(env.get("QD_HISTORY", "0")) == 1
    except ValueError:
        enabled = False
    try:
        days = float(env.get("QD_HISTORY_EVERY_DAYS", str(EVERY_DAYS)))
    except ValueError:
        days = EVERY_DAYS
    if not (days > 0.0) or not math.isfinite(days):
        days = EVERY_DAYS
    try:
        k = int(env.get("QD_HISTORY_SAMPLE_EVERY", str(SAMPLE_EVERY)))
    except ValueError:
        k = SAMPLE_EVERY
    if k < 1:
        k = SAMPLE_EVERY
    text = env.get("QD_HISTORY_FIELDS")
    fields = parse_fields(text) if (enabled and text is not None and str(text).strip()) else None
    return {"enabled": enabled, "every_days": days, "sample_every": k, "fields": fields}


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


def steps_per_window(every_days, day, dt):
    return max(1, int(float(every_days) * float(day) / float(dt) + 0.5))


def schedule(i0, n, S, sample_every=1):
    """The next n steps, the first with run-local index i0 -> int32 [n]: 1 where the step's position in its window [k S, (k + 1) S)
    is a multiple of sample_every (the phase restarts with every window)."""
    pos = (int(i0) + np.arange(int(n), dtype=np.int64)) % int(S)
    return (pos % int(sample_every) == 0).astype(np.int32)


def label_decimals(window_days):
    """Decimals of the day labels in a file name: 1, the frames' convention (`{t:05.1f}`), and as many as a window shorter than
    0.1 day needs for its labels to differ from the next window's."""
    return max(1, int(math.ceil(-math.log10(float(window_days)) - 1e-12)))


def file_name(a_days, b_days, decimals=1):
    w = decimals + 3
    return f"history_day_{a_days:0{w}.{decimals}f}_{b_days:0{w}.{decimals}f}.nc"


def global_mean(plane, lat_mesh):
    """cos-latitude-weighted mean of a map: sum(max(cos lat, 0) x) / sum(max(cos lat, 0))."""
    w = np.maximum(np.cos(np.deg2rad(lat_mesh)), 0.0)
    return float(np.sum(w * plane) / np.sum(w))


class History:
    """The lane's participant in Device.step_n (like BudgetDiag): the run-local step index is its clock, span_schedule uploads the
    span's sample flags, flush() turns the resident sums into one file."""

    def __init__(self, dev, grid, cfg, with_ocean=True, dt=300.0, day=None, out=print, output_dir=None):
        self.dev, self.grid, self.cfg, self.out = dev, grid, dict(cfg), out
        self.dt = float(dt)
        self.day = float(2.0 * np.pi / dev.params.omega) if day is None else float(day)
        self.names = resolve_fields(cfg.get("fields"), with_ocean)
        self.S = steps_per_window(cfg["every_days"], self.day, self.dt)
        self.sample_every = int(cfg["sample_every"])
        self.decimals = label_decimals(self.S * self.dt / self.day)
        self.output_dir = output_dir
        self.i = 0                                   # run-local index of the next step
        self.t_first = self.t_last = None            # start times (s) of the open window's first and last sampled step
        self.n_open = 0                              # samples the host has scheduled into the open window
        self.files = []
        dev.history_configure(entries_for(self.names))

    # -- the span protocol of Device.step_n
    def span_clock(self):
        return (self.i, self.t_first, self.t_last, self.n_open)

    def span_restore(self, clock):
        self.i, self.t_first, self.t_last, self.n_open = clock

    def span_schedule(self, t0, dt, n):
        flags = schedule(self.i, n, self.S, self.sample_every)
        self.dev.history_schedule(flags)
        if t0 is None:
            times = (self.i + np.arange(int(n))) * float(dt)
        elif np.ndim(t0) == 0:
            times = float(t0) + float(dt) * np.arange(int(n))
        else:
            times = np.asarray(t0, dtype=np.float64)
        hit = np.flatnonzero(flags)
        return (int(n), (float(times[hit[0]]), float(times[hit[-1]])) if hit.size else None, int(hit.size))

    def _fired(self, k):
        n, span, count = k
        self.i += n
        if span is not None:
            if self.t_first is None:
                self.t_first = span[0]
            self.t_last = span[1]
            self.n_open += count

    def span_deliver(self, dt):
        pass                                         # the samples went into the resident sums: nothing to drain behind a span

    # -- windows
    def steps_to_window_end(self, i=None):
        """Steps from step i (default: the next step) up to and including its window's last step."""
        i = self.i if i is None else int(i)
        return self.S - (i % self.S)

    def window_closed(self):
        """The last step that ran was a window's last step."""
        return self.i > 0 and self.i % self.S == 0

    def path(self, a_days, b_days):
        out = self.output_dir if self.output_dir is not None else os.environ.get("QD_OUTPUT_DIR", "output")
        return os.path.join(out, "history", file_name(a_days, b_days, self.decimals))

    def flush(self, t_first_days=None, t_last_days=None, complete=1):
        """Read the sums, divide by the sample count, write the file, print one line, reset -> the path, or None when the window
        holds no sample.  The labels default to the start times of the window's first and last sampled step."""
        sums, count = self.dev.history_read()
        if count <= 0:
            return None
        t0s = self.t_first if t_first_days is None else float(t_first_days) * self.day
        t1s = self.t_last if t_last_days is None else float(t_last_days) * self.day
        t0s, t1s = (0.0 if t0s is None else float(t0s)), (0.0 if t1s is None else float(t1s))
        a, b = t0s / self.day, t1s / self.day
        means = np.asarray(sums, dtype=np.float64) / np.float64(count)
        path = self.path(a, b)
        variables = {"lat": ("f8", ("lat",), np.asarray(self.grid.lat, dtype=np.float64)),
                     "lon": ("f8", ("lon",), np.asarray(self.grid.lon, dtype=np.float64))}
        for name, plane in zip(self.names, means):
            variables[name.lower()] = ("f8", ("lat", "lon"), plane)
        variables.update(n_samples=("i4", (), int(count)), t_start_seconds=("f8", (), t0s), t_end_seconds=("f8", (), t1s),
                         dt_seconds=("f8", (), self.dt), sample_every=("i4", (), self.sample_every), complete=("i4", (), 1 if complete else 0))
        os.makedirs(os.path.dirname(path), exist_ok=True)
        tmp = path + ".part"
        try:
            ncio.write_nc(tmp, {"lat": int(self.grid.n_lat), "lon": int(self.grid.n_lon)}, variables)
            os.replace(tmp, path)
        finally:
            if os.path.exists(tmp):
                os.remove(tmp)
        d = self.decimals
        self.out(f"[History] day {a:.{d}f}–{b:.{d}f}: {count} samples | " +
                 " ".join(f"{n}={global_mean(m, self.grid.lat_mesh):.6g}" for n, m in list(zip(self.names, means))[:6]))
        self.drop()
        self.files.append(path)
        return path

    def drop(self):
        """Forget the open window: sums and count to zero, the labels start with the next sample."""
        self.dev.history_reset()
        self.t_first = self.t_last = None
        self.n_open = 0


def from_env(dev, grid, env, with_ocean=True, dt=None, day=None, out=print):
    """QD_HISTORY (default 0) -> a History on this handle, or None: at 0 nothing is configured, allocated, scheduled or launched."""
    cfg = read_env(env)
    if not cfg["enabled"]:
        return None
    if dt is None:
        dt = float(env.get("QD_DT_SECONDS", "300"))
    return History(dev, grid, cfg, with_ocean=with_ocean, dt=dt, day=day, out=out)
