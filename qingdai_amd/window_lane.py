"""
qingdai_amd/window_lane.py -- the host side that the windowed diagnostics share: history, series, spectra, drifters, flow, spharm,
eddy and extremes.  The one statement of their window clock and of their part in the span protocol of Device.step_n.

The window clock: windows are counted on the run-local step index, which starts where the lane is enabled.  Window k is the steps
[k S, (k + 1) S) with S = max(1, int(every_days * day / dt + 0.5)), and every `every`-th step of a window is sampled, counted from the
window's first step (the phase restarts with every window).  A window's file is <QD_OUTPUT_DIR, default output>/NAME/
NAME_day_{a}_{b}.nc, a and b the start times over `day` of the window's first and last sampled step.

Two concrete bases for the two forms a lane's open window takes:
  SumWindowLane   the samples go into resident planes on the device; the host keeps the labels (t_first, t_last) and a count
                  (n_open).  History, Eddy, Extremes.
  LogWindowLane   every sample leaves a record in the lane's device log; span_deliver drains it behind each span into recs, times
                  and steps.  Series, Spectra, Drifters, Flow, Spharm.
A lane overrides: _upload(flags) (its dev.<x>_schedule), _drain(want) (log lanes: its dev.<x>_log), _window_file(complete) -> None
for an empty window or (a_days, b_days, dims, variables, line), drop() (what forgetting the open window means for it) and key() (its
part of a checkpoint's subsystem set).

Nothing here touches the device; everything is plain NumPy (tests/test_window_lane_cpu.py).
"""
from __future__ import annotations

import math
import os

import numpy as np

from . import ncio


# ------------------------------------------------------------------------------------- environment
def env_int(env, name, default):
    """env[name] as an int; the default where it is unset or does not parse (a value that is no text included)."""
    try:
        return int(env.get(name, str(default)))
    except (TypeError, ValueError):
        return default


def env_every(env, name, default):
    """A cadence in steps: an int >= 1, else the default."""
    k = env_int(env, name, default)
    return k if k >= 1 else default


def env_days(env, name, default=10.0):
    """A window length in planet-days: a finite float > 0, else the default."""
    try:
        days = float(env.get(name, str(default)))
    except (TypeError, ValueError):
        return default
    return days if days > 0.0 and math.isfinite(days) else default


def env_dt(env, dt=None):
    """The step a lane built from the environment runs at: the caller's, else QD_DT_SECONDS (default 300)."""
    return float(env.get("QD_DT_SECONDS", "300")) if dt is None else dt


# ------------------------------------------------------------------------------------- the clock
def steps_per_window(every_days, day, dt):
    return max(1, int(float(every_days) * float(day) / float(dt) + 0.5))


def schedule(i0, n, S, sample_every=1):
    """The next n steps, the first with run-local index i0 -> int32 [n]: 1 where the step's position in its window [k S, (k + 1) S)
    is a multiple of sample_every (the phase restarts with every window)."""
    pos = (int(i0) + np.arange(int(n), dtype=np.int64)) % int(S)
    return (pos % int(sample_every) == 0).astype(np.int32)


def span_times(i, t0, dt, n):
    """The start times of a span's n steps as Device.step_n names them: t0 None -> the run-local index i times dt; a scalar -> t0 + dt
    * arange(n); an array -> the n times themselves."""
    if t0 is None:
        return (i + np.arange(int(n))) * float(dt)
    if np.ndim(t0) == 0:
        return float(t0) + float(dt) * np.arange(int(n))
    return np.asarray(t0, dtype=np.float64)


# ------------------------------------------------------------------------------------- files
def label_decimals(window_days):
    """Decimals of the day labels in a file name: 1, the frames' convention (`{t:05.1f}`), and as many as a window shorter than
    0.1 day needs for its labels to differ from the next window's."""
    return max(1, int(math.ceil(-math.log10(float(window_days)) - 1e-12)))


def window_file_name(prefix, a_days, b_days, decimals=1):
    w = decimals + 3
    return f"{prefix}_day_{a_days:0{w}.{decimals}f}_{b_days:0{w}.{decimals}f}.nc"


def write_atomic(path, dims, variables):
    """ncio.write_nc to `path` + ".part", then os.replace: a failure in the middle leaves no part file and an earlier `path` as it
    was."""
    os.makedirs(os.path.dirname(path), exist_ok=True)
    tmp = path + ".part"
    try:
        ncio.write_nc(tmp, dims, variables)
        os.replace(tmp, path)
    finally:
        if os.path.exists(tmp):
            os.remove(tmp)


def i8_code():
    """Classic NetCDF (the scipy back end) has no 64-bit integer: step indices and counts, far below 2^53, are then written as f8."""
    return "i8" if ncio.backend() == "netCDF4" else "f8"


# ------------------------------------------------------------------------------------- the lanes
class WindowLane:
    """What the eight lanes share: the window clock on the run-local step index `i`, span_schedule, the window's path and the
    skeleton of flush.  NAME is the directory, the file prefix and the lane's name in driver and checkpoint; TAG the bracketed word
    of its printed line."""
    NAME = TAG = None

    def __init__(self, dev, grid, cfg, out, dt, day, every_days, every, output_dir=None):
        self.dev, self.grid, self.cfg, self.out = dev, grid, dict(cfg), out
        self.dt = float(dt)
        self.day = float(2.0 * np.pi / dev.params.omega) if day is None else float(day)
        self.S = steps_per_window(every_days, self.day, self.dt)
        self.every = int(every)
        self.decimals = label_decimals(self.S * self.dt / self.day)
        self.output_dir = output_dir
        self.i = 0                                   # run-local index of the next step
        self.files = []

    # -- the span protocol of Device.step_n (span_clock, span_restore, _fired and span_deliver are the two bases')
    def span_schedule(self, t0, dt, n):
        flags = schedule(self.i, n, self.S, self.every)
        self._upload(flags)                          # (more samples than a log holds between two drains: qd_step_n refuses the span)
        return self._span_result(span_times(self.i, t0, dt, n), np.flatnonzero(flags), n)

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
        return os.path.join(out, self.NAME, window_file_name(self.NAME, a_days, b_days, self.decimals))

    def flush(self, complete=1, **labels):
        """Write the open window's file, print one line, start the next window -> the path, or None when the window is empty."""
        window = self._window_file(complete, **labels)
        if window is None:
            return None
        a, b, dims, variables, line = window
        path = self.path(a, b)
        write_atomic(path, dims, variables)
        self.out(line)
        self.drop()
        self.files.append(path)
        return path


class SumWindowLane(WindowLane):
    """A lane whose samples go into resident planes: the host's part of the open window is its labels and its sample count."""

    def __init__(self, dev, grid, cfg, out, dt, day, every_days, every, output_dir=None):
        super().__init__(dev, grid, cfg, out, dt, day, every_days, every, output_dir)
        self.sample_every = self.every
        self.t_first = self.t_last = None            # start times (s) of the open window's first and last sampled step
        self.n_open = 0                              # samples the host has scheduled into the open window

    def span_clock(self):
        return (self.i, self.t_first, self.t_last, self.n_open)

    def span_restore(self, clock):
        self.i, self.t_first, self.t_last, self.n_open = clock

    def _span_result(self, times, hit, n):
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
        pass                                         # the samples went into the resident planes: nothing to drain behind a span

    def window_labels(self):
        """(t_first, t_last) in seconds, 0 where the window has none."""
        return (0.0 if self.t_first is None else float(self.t_first)), (0.0 if self.t_last is None else float(self.t_last))

    def drop(self):
        """Forget the open window, the host's half: the labels start with the next sample.  A lane resets its planes first."""
        self.t_first = self.t_last = None
        self.n_open = 0


class LogWindowLane(WindowLane):
    """A lane whose samples leave records of `width` doubles in a device log: _pending holds the (times, steps) of spans that ran
    and whose records are still there, recs / times / steps the open window as delivered."""

    def __init__(self, dev, grid, cfg, out, dt, day, every_days, every, width, output_dir=None):
        super().__init__(dev, grid, cfg, out, dt, day, every_days, every, output_dir)
        self.width = int(width)
        self._pending = []
        self.recs, self.times, self.steps = [], [], []

    def span_clock(self):
        return (self.i, len(self._pending))

    def span_restore(self, clock):
        self.i = clock[0]
        del self._pending[clock[1]:]

    def _span_result(self, times, hit, n):
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
        recs = self._drain(want)
        if len(recs) != want:
            raise RuntimeError(f"{type(self).__name__}: the device log held {len(recs)} records where the schedule says {want}")
        self.recs.append(recs)
        for t, s in self._pending:
            self.times.append(t)
            self.steps.append(s)
        self._pending = []
        return recs

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

    def drop(self):
        """Forget the open window's delivered records; the next sample starts the next file.  _pending and the device log stay: a
        lane whose drop() also forgets those says so."""
        self.recs, self.times, self.steps = [], [], []
