"""
qingdai_amd/extremes.py -- extremes, spells and distributions (QD_EXTREMES=1), host side of csrc/qd_extremes.hip.

Nothing the reference has.  The other statistics lanes give means, per-step global numbers, second moments and spectra; none says
what the tails look like.  On every sampled step of the device loop this lane updates, per cell, each selected entry's maximum and
minimum with the sample they occurred in and a count of NaNs; per threshold (TS<273.15, PRECIP>1 mm/day) how often it held, how
many spells there were and how long the longest was; and per binned entry and latitude row a histogram -- a span lane without a
flag bit and without a log, like the history accumulators, sampled at history's two places (PRECIP in front of the ocean step).
Behind a window's last step the state becomes <QD_OUTPUT_DIR, default output>/extremes/extremes_day_{a}_{b}.nc, labelled like the
history files.  The window clock is history's: window k is the steps [k S, (k + 1) S) with S = max(1, int(QD_EXTREMES_EVERY_DAYS *
day / dt + 0.5)), and every QD_EXTREMES_SAMPLE_EVERY-th step of a window is sampled, counted from the window's first step.

The definition of a sample is the top of csrc/qd_extremes.hip; accumulate_reference restates it bit for bit and is the only other
statement.  Every number of the state is a selection among stored values or an integer count.  Everything is reset at a window's
start, the running spell included: a spell is cut at a window boundary (the file carries the run at the window's end as
{label}_open, so a reader can see a cut; stitching windows is not done here).

The default thresholds, bin ranges and cadence are guesses: nobody has measured this planet's tails.  The file carries each
histogram's under, over and NaN shares, so a range that misses the distribution shows.

Nothing here touches the device at import; the parsers, the clock, the arithmetic and the file writing are plain NumPy
(tests/test_extremes_cpu.py).
"""
from __future__ import annotations

import math
import zlib

import numpy as np

from . import history
from ._lib import C as _C
from .window_lane import SumWindowLane, env_days, env_dt, env_every, env_int, i8_code, window_file_name

FIELDS_VAR, THRESHOLDS_VAR, BINS_VAR = "QD_EXTREMES_FIELDS", "QD_EXTREMES_THRESHOLDS", "QD_EXTREMES_BINS"
DEFAULT_FIELDS = ("TS", "PRECIP", "WIND_SPEED", "H")
DEFAULT_OCEAN_FIELDS = ("SST",)
DEFAULT_THRESHOLDS = "TS<273.15,PRECIP>1.1574e-5"         # freezing; 1 mm/day (the state frame shows PRECIP * 86400 as mm/day)
DEFAULT_BINS = "PRECIP:log:1e-8:1e-2:60,TS:lin:150:350:100,WIND_SPEED:lin:0:100:100"
MAX_ENTRIES, MAX_THRESHOLDS = _C["QD_EXTREMES_MAX_ENTRIES"], _C["QD_EXTREMES_MAX_THRESHOLDS"]
MAX_HISTS, MAX_BINS = _C["QD_EXTREMES_MAX_HISTS"], _C["QD_EXTREMES_MAX_BINS"]
EVERY_DAYS = 10.0
SAMPLE_EVERY = 4          # a guess, like the ranges above: one sample moves of the order of 200 bytes per cell at the defaults (derived)
QUANTILE_LEVELS = (0.5, 0.9, 0.99, 0.999)


# ------------------------------------------------------------------------------------- the lists
def parse_fields(text, var=FIELDS_VAR):
    """History's parser with this lane's entry limit."""
    names = history.parse_fields(text, var=var)
    if len(names) > MAX_ENTRIES:
        raise ValueError(f"{var}: {len(names)} entries, at most {MAX_ENTRIES}")
    for n in names:
        if names.count(n) > 1:
            raise ValueError(f"{var}: field '{n}' is named twice")
    return names


def _number(text, var, item):
    try:
        v = float(text)
    except (TypeError, ValueError):
        raise ValueError(f"{var}: '{item}': '{text}' is not a number") from None
    if not math.isfinite(v):
        raise ValueError(f"{var}: '{item}': '{text}' is not finite")
    return v


def parse_thresholds(text, fields, var=THRESHOLDS_VAR):
    """'TS<273.15,PRECIP>1e-5' -> [(name, '<' or '>', value)], names upper-cased.  Refused with a ValueError that names the item: an
    item that is not NAME<value or NAME>value, a value that is no finite number, a name that is not among `fields`, a threshold
    named twice, more than 16."""
    out = []
    for item in (s.strip() for s in str(text).split(",")):
        if not item:
            continue
        cmp = "<" if "<" in item else ">" if ">" in item else None
        name, _, value = item.partition(cmp) if cmp else (item, "", "")
        name = name.strip().upper()
        if cmp is None or not name or not value.strip() or "<" in value or ">" in value:
            raise ValueError(f"{var}: '{item}' is not NAME<value or NAME>value")
        v = _number(value.strip(), var, item)
        if name not in fields:
            raise ValueError(f"{var}: '{item}': '{name}' is not among the lane's fields ({', '.join(fields)})")
        if (name, cmp, v) in out:
            raise ValueError(f"{var}: the threshold '{item}' is named twice")
        out.append((name, cmp, v))
    if len(out) > MAX_THRESHOLDS:
        raise ValueError(f"{var}: {len(out)} thresholds, at most {MAX_THRESHOLDS}")
    return out


def make_edges(kind, lo, hi, n):
    """n + 1 edges in f64 from lo to hi: 'lin' evenly spaced, 'log' evenly spaced in log10; the end points are lo and hi exactly."""
    if kind == "lin":
        e = np.linspace(lo, hi, n + 1)
    else:
        e = np.power(10.0, np.linspace(math.log10(lo), math.log10(hi), n + 1))
    e[0], e[-1] = lo, hi
    return e


def check_edges(edges, what):
    """-> the edges as a 1D f64 array; refused: fewer than 2, more than 257, not finite, not strictly increasing."""
    e = np.array(edges, dtype=np.float64).reshape(-1)
    if e.size < 2:
        raise ValueError(f"{what}: fewer than 2 edges")
    if e.size - 1 > MAX_BINS:
        raise ValueError(f"{what}: {e.size - 1} bins, at most {MAX_BINS}")
    if not np.all(np.isfinite(e)) or not np.all(e[1:] > e[:-1]):
        raise ValueError(f"{what}: the edges are not finite and strictly increasing")
    return e


def parse_bins(text, fields, var=BINS_VAR):
    """'PRECIP:log:1e-8:1e-2:60,TS:lin:150:350:100' -> [(name, edges)].  Refused with a ValueError that names the item: an item that is
    not NAME:lin:lo:hi:n or NAME:log:lo:hi:n, numbers that are none, log with lo <= 0, hi <= lo, n outside 1 .. 256, a name that is
    not among `fields`, a name binned twice, more than 8."""
    out = []
    for item in (s.strip() for s in str(text).split(",")):
        if not item:
            continue
        part = [s.strip() for s in item.split(":")]
        if len(part) != 5 or not part[0] or part[1].lower() not in ("lin", "log"):
            raise ValueError(f"{var}: '{item}' is not NAME:lin:lo:hi:n or NAME:log:lo:hi:n")
        name, kind = part[0].upper(), part[1].lower()
        lo, hi = _number(part[2], var, item), _number(part[3], var, item)
        try:
            n = int(part[4])
        except ValueError:
            raise ValueError(f"{var}: '{item}': '{part[4]}' is not a bin count") from None
        if kind == "log" and lo <= 0.0:
            raise ValueError(f"{var}: '{item}': log bins need lo > 0")
        if hi <= lo:
            raise ValueError(f"{var}: '{item}': hi is not above lo")
        if n < 1 or n > MAX_BINS:
            raise ValueError(f"{var}: '{item}': {n} bins, 1 to {MAX_BINS}")
        if name not in fields:
            raise ValueError(f"{var}: '{item}': '{name}' is not among the lane's fields ({', '.join(fields)})")
        if name in [o[0] for o in out]:
            raise ValueError(f"{var}: '{item}': '{name}' is binned twice")
        out.append((name, check_edges(make_edges(kind, lo, hi, n), f"{var}: '{item}'")))
    if len(out) > MAX_HISTS:
        raise ValueError(f"{var}: {len(out)} histograms, at most {MAX_HISTS}")
    return out


def threshold_label(name, cmp, value):
    """('TS', '<', 273.15) -> 'TS_lt_273p15': the value as %g, made safe for a variable name."""
    text = ("%g" % value).replace("+", "").replace("-", "m").replace(".", "p")
    return f"{name}_{'lt' if cmp == '<' else 'gt'}_{text}"


def read_env(env):
    """-> dict: enabled (QD_EXTREMES, default 0), fields (QD_EXTREMES_FIELDS parsed, or None = the default list), thresholds and bins
    (the texts of QD_EXTREMES_THRESHOLDS and QD_EXTREMES_BINS, or None = the defaults that name a field of the run), sample_every
    (QD_EXTREMES_SAMPLE_EVERY, default 4; unparsable or < 1 -> 4), every_days (QD_EXTREMES_EVERY_DAYS, default 10; unparsable or
    <= 0 -> 10).  The lists are parsed -- and refused -- only when the lane is on."""
    enabled = env_int(env, "QD_EXTREMES", 0) == 1

    def text(var):
        t = env.get(var)
        return None if t is None or not str(t).strip() else str(t)
    fields = text(FIELDS_VAR)
    cfg = {"enabled": enabled, "fields": None, "thresholds": text(THRESHOLDS_VAR), "bins": text(BINS_VAR),
           "sample_every": env_every(env, "QD_EXTREMES_SAMPLE_EVERY", SAMPLE_EVERY), "every_days": env_days(env, "QD_EXTREMES_EVERY_DAYS", EVERY_DAYS)}
    if enabled:
        cfg["fields"] = parse_fields(fields) if fields is not None else None
        names = cfg["fields"] if cfg["fields"] is not None else list(DEFAULT_FIELDS + DEFAULT_OCEAN_FIELDS)
        if cfg["thresholds"] is not None:
            parse_thresholds(cfg["thresholds"], names)
        if cfg["bins"] is not None:
            parse_bins(cfg["bins"], names)
    return cfg


def resolve_fields(fields, with_ocean, var=FIELDS_VAR):
    """The run's entry names: the default list (SST only with the ocean) or the named ones, among which a field of a subsystem that
    is off is refused (history's rule)."""
    if fields is None:
        return list(DEFAULT_FIELDS) + (list(DEFAULT_OCEAN_FIELDS) if with_ocean else [])
    return history.resolve_fields(fields, with_ocean, var=var)


def file_name(a_days, b_days, decimals=1):
    return window_file_name("extremes", a_days, b_days, decimals)


# ------------------------------------------------------------------------------------- the definition, in NumPy
def entry_values(names, get):
    """[E][n_lat][n_lon]: the entries' values from get(field name) -> plane; a derived entry is np.sqrt(a*a + b*b)."""
    out = []
    with np.errstate(invalid="ignore", over="ignore"):
        for n in names:
            if n in history.DERIVED:
                a, b = (np.asarray(get(f), dtype=np.float64) for f in history.DERIVED[n])
                out.append(np.sqrt(a * a + b * b))
            else:
                out.append(np.asarray(get(n), dtype=np.float64))
    return np.stack(out)


def bin_columns(x, edges):
    """The histogram column of every value, 0 .. nb + 2 in [under, bin 0 .. bin nb - 1, over, nan]."""
    x, e = np.asarray(x, dtype=np.float64), np.asarray(edges, dtype=np.float64)
    nb = e.size - 1
    is_nan = np.isnan(x)
    with np.errstate(invalid="ignore"):
        under, over = x < e[0], x >= e[nb]
    inside = ~(is_nan | under | over)
    col = np.searchsorted(e, np.where(inside, x, e[0]), side="right")        # bin + 1
    return np.where(is_nan, nb + 2, np.where(under, 0, np.where(over, nb + 1, col))).astype(np.int64)


def accumulate_reference(samples, thresholds=(), hists=(), state=None):
    """The lane's state after the samples, bit for bit -> {vmax, vmin [E][n_lat][n_lon] f64; tmax, tmin, nan [E][n_lat][n_lon] i32;
    thr [T][n_lat][n_lon][4] u32 (count, run, longest, spells); hist: a list of [n_lat][nb + 3] i64; n: the sample count}.
    samples: an iterable of [E][n_lat][n_lon] f64 arrays of entry values, one per sample, in step order; thresholds: [(entry index,
    '<' or '>', value)]; hists: [(entry index, edges)]; state: what an earlier call returned, to go on from (None: a window's
    start).  k is the sample's 0-based index in the window.  Per cell:
        if (x > vmax) { vmax = x; tmax = k; }    if (x < vmin) { vmin = x; tmin = k; }    nan += (x != x)
        hit = x cmp value;  spells += hit && run == 0;  run = hit ? run + 1 : 0;  count += hit;  longest = max(longest, run)
    and per row hist[column of x] += 1 (bin_columns)."""
    st = None
    if state is not None:
        st = {k: np.array(state[k]) for k in ("vmax", "vmin", "tmax", "tmin", "nan", "thr")}
        st["hist"] = [np.array(h, dtype=np.int64) for h in state["hist"]]
        st["n"] = int(state["n"])
    with np.errstate(invalid="ignore"):
        for x in samples:
            x = np.asarray(x, dtype=np.float64)
            if st is None:
                shape = x.shape
                st = {"vmax": np.full(shape, -np.inf), "vmin": np.full(shape, np.inf), "tmax": np.full(shape, -1, dtype=np.int32),
                      "tmin": np.full(shape, -1, dtype=np.int32), "nan": np.zeros(shape, dtype=np.int32),
                      "thr": np.zeros((len(thresholds),) + shape[1:] + (4,), dtype=np.uint32),
                      "hist": [np.zeros((shape[1], np.size(e) - 1 + 3), dtype=np.int64) for _, e in hists], "n": 0}
            k = np.int32(st["n"])
            up, down = x > st["vmax"], x < st["vmin"]
            st["vmax"], st["tmax"] = np.where(up, x, st["vmax"]), np.where(up, k, st["tmax"]).astype(np.int32)
            st["vmin"], st["tmin"] = np.where(down, x, st["vmin"]), np.where(down, k, st["tmin"]).astype(np.int32)
            st["nan"] = st["nan"] + (x != x).astype(np.int32)
            for t, (e, cmp, value) in enumerate(thresholds):
                hit = (x[e] > np.float64(value)) if cmp in (">", ord(">")) else (x[e] < np.float64(value))
                count, run, longest, spells = (st["thr"][t][..., i] for i in range(4))
                spells = spells + (hit & (run == 0)).astype(np.uint32)
                run = np.where(hit, run + np.uint32(1), np.uint32(0)).astype(np.uint32)
                count = count + hit.astype(np.uint32)
                longest = np.maximum(longest, run)
                st["thr"][t] = np.stack([count, run, longest, spells], axis=-1)
            for h, (e, edges) in enumerate(hists):
                w = np.size(edges) - 1 + 3
                col = bin_columns(x[e], edges)
                rows = np.arange(col.shape[0], dtype=np.int64)[:, None] * w
                st["hist"][h] = st["hist"][h] + np.bincount((rows + col).ravel(), minlength=col.shape[0] * w).reshape(col.shape[0], w)
            st["n"] += 1
    if st is None:
        raise ValueError("accumulate_reference: no sample and no state")
    return st


# ------------------------------------------------------------------------------------- what a file says of the state
def row_weights(lat):
    return np.maximum(np.cos(np.deg2rad(np.asarray(lat, dtype=np.float64))), 0.0)


def hist_summary(hist, edges, lat, levels=QUANTILE_LEVELS):
    """One table [n_lat][nb + 3] -> {pdf [nb], under_frac, over_frac, nan_frac, quantiles [len(levels)]}, rows weighted by
    max(cos lat, 0).  pdf: the share of in-range samples per bin (NaN without any).  The three shares are of all samples.  A
    quantile is a level of the samples that are not NaN: linear interpolation inside the bin the level falls into, NaN when it
    falls into under or over (or there is no sample)."""
    e = np.asarray(edges, dtype=np.float64)
    nb = e.size - 1
    w = row_weights(lat)
    cols = np.sum(w[:, None] * np.asarray(hist, dtype=np.float64), axis=0)
    total, inside = float(np.sum(cols)), float(np.sum(cols[1:nb + 1]))
    nan = float("nan")
    out = {"pdf": cols[1:nb + 1] / inside if inside > 0.0 else np.full(nb, nan),
           "under_frac": cols[0] / total if total > 0.0 else nan, "over_frac": cols[nb + 1] / total if total > 0.0 else nan,
           "nan_frac": cols[nb + 2] / total if total > 0.0 else nan}
    valid = total - float(cols[nb + 2])
    cum = np.cumsum(cols[:nb + 1])                      # behind under, behind bin 0, ..., behind bin nb - 1
    q = []
    for level in levels:
        target = float(level) * valid
        if not (valid > 0.0) or target <= cum[0] or target > cum[nb]:
            q.append(nan)
            continue
        i = int(np.searchsorted(cum[1:], target, side="left"))          # the first bin behind which the level is reached
        q.append(float(e[i] + (target - cum[i]) / cols[1 + i] * (e[i + 1] - e[i])))
    out["quantiles"] = np.array(q, dtype=np.float64)
    return out


def threshold_summary(thr, n, step_seconds):
    """One threshold's items [n_lat][n_lon][4] and the sample count -> {count, spells, open (i4), freq, longest_seconds,
    mean_spell_seconds (f8; NaN where there are no spells)}; step_seconds: the time between two samples."""
    count, run, longest, spells = (np.asarray(thr[..., i], dtype=np.int64) for i in range(4))
    with np.errstate(invalid="ignore", divide="ignore"):
        mean = np.where(spells > 0, count / np.maximum(spells, 1), np.nan) * float(step_seconds)
    return {"count": count.astype(np.int32), "spells": spells.astype(np.int32), "open": run.astype(np.int32),
            "freq": count / np.float64(n), "longest_seconds": longest * float(step_seconds), "mean_spell_seconds": mean}


def window_variables(state, names, thresholds, hists, lat, lon, t_first, step_seconds):
    """The state of a window -> (dims, variables) of its file, without the scalars.  thresholds: [(name, cmp, value)]; hists:
    [(name, edges)]; t_first: the start time (s) of sample 0; step_seconds: sample_every * dt."""
    lat, lon = np.asarray(lat, dtype=np.float64), np.asarray(lon, dtype=np.float64)
    dims = {"lat": lat.size, "lon": lon.size, "quantile": len(QUANTILE_LEVELS)}
    v = {"lat": ("f8", ("lat",), lat), "lon": ("f8", ("lon",), lon),
         "quantile_levels": ("f8", ("quantile",), np.array(QUANTILE_LEVELS, dtype=np.float64))}
    for e, name in enumerate(names):
        n = name.lower()
        for side, val, t in (("max", state["vmax"][e], state["tmax"][e]), ("min", state["vmin"][e], state["tmin"][e])):
            v[f"{n}_{side}"] = ("f8", ("lat", "lon"), np.where(t >= 0, val, np.nan))
            v[f"{n}_t{side}_seconds"] = ("f8", ("lat", "lon"), np.where(t >= 0, float(t_first) + t.astype(np.float64) * float(step_seconds), np.nan))
        v[f"{n}_nan"] = ("i4", ("lat", "lon"), np.asarray(state["nan"][e], dtype=np.int32))
    for t, (name, cmp, value) in enumerate(thresholds):
        label = threshold_label(name, cmp, value).lower()
        s = threshold_summary(state["thr"][t], state["n"], step_seconds)
        for key in ("count", "spells", "open"):
            v[f"{label}_{key}"] = ("i4", ("lat", "lon"), s[key])
        for key in ("freq", "longest_seconds", "mean_spell_seconds"):
            v[f"{label}_{key}"] = ("f8", ("lat", "lon"), s[key])
    for h, (name, edges) in enumerate(hists):
        n, nb = name.lower(), np.size(edges) - 1
        dims[f"{n}_edge"], dims[f"{n}_bin"], dims[f"{n}_col"] = nb + 1, nb, nb + 3
        s = hist_summary(state["hist"][h], edges, lat)
        v[f"{n}_edges"] = ("f8", (f"{n}_edge",), np.asarray(edges, dtype=np.float64))
        v[f"{n}_hist"] = (i8_code(), ("lat", f"{n}_col"), np.asarray(state["hist"][h], dtype=np.int64))
        v[f"{n}_pdf"] = ("f8", (f"{n}_bin",), s["pdf"])
        for key in ("under_frac", "over_frac", "nan_frac"):
            v[f"{n}_{key}"] = ("f8", (), float(s[key]))
        v[f"{n}_quantiles"] = ("f8", ("quantile",), s["quantiles"])
    return dims, v


# ------------------------------------------------------------------------------------- the lane
class Extremes(SumWindowLane):
    """The lane's participant in Device.step_n: the clock and the span protocol are window_lane's, flush() turns the resident state
    into one file.  drop() puts the device's state back to its start values, the count to zero, and forgets the labels.

    Extremes(sim, fields=..., thresholds=..., bins={name: edges}) configures it on a driver.Simulation with the caller's own lists:
    fields a list of names or a comma-separated text, thresholds a text like QD_EXTREMES_THRESHOLDS or [(name, cmp, value)], bins a
    text like QD_EXTREMES_BINS or {name: edges} with the edges as they are to be used.  Extremes(dev, grid, cfg, ...) is what
    from_env builds.  What is None comes from cfg, and then from the defaults that name a field of the run."""

    NAME, TAG = "extremes", "Extremes"

    def __init__(self, dev, grid=None, cfg=None, with_ocean=None, dt=None, day=None, out=print, output_dir=None,
                 fields=None, thresholds=None, bins=None):
        sim = dev if hasattr(dev, "dev") else None
        if sim is not None:
            dev, grid = sim.dev, sim.grid if grid is None else grid
            with_ocean = (sim.ocean is not None) if with_ocean is None else with_ocean
            dt = float(sim.dt) if dt is None else dt
            day = getattr(sim, "day_seconds", None) if day is None else day
        cfg = dict(cfg or {})
        super().__init__(dev, grid, cfg, out, 300.0 if dt is None else dt, day, cfg.get("every_days", EVERY_DAYS),
                         cfg.get("sample_every", SAMPLE_EVERY), output_dir)
        with_ocean = True if with_ocean is None else bool(with_ocean)
        fields = cfg.get("fields") if fields is None else fields
        if isinstance(fields, str):
            fields = parse_fields(fields)
        elif fields is not None:
            fields = parse_fields(",".join(fields))
        self.names = resolve_fields(fields, with_ocean)
        thresholds = cfg.get("thresholds") if thresholds is None else thresholds
        if thresholds is None:                       # the defaults, as far as the run has their fields
            thresholds = ",".join(s for s in DEFAULT_THRESHOLDS.split(",") if s.replace(">", "<").split("<")[0] in self.names)
        self.thresholds = (parse_thresholds(thresholds, self.names) if isinstance(thresholds, str) else
                           parse_thresholds(",".join(f"{n}{'<' if c in ('<', ord('<')) else '>'}{float(x)!r}" for n, c, x in thresholds), self.names))
        bins = cfg.get("bins") if bins is None else bins
        if bins is None:
            bins = ",".join(s for s in DEFAULT_BINS.split(",") if s.split(":")[0] in self.names)
        if isinstance(bins, str):
            self.hists = parse_bins(bins, self.names)
        else:
            self.hists = []
            for n, e in dict(bins).items():
                n = str(n).strip().upper()
                if n not in self.names:
                    raise ValueError(f"{BINS_VAR}: '{n}' is not among the lane's fields ({', '.join(self.names)})")
                self.hists.append((n, check_edges(e, f"{BINS_VAR}: '{n}'")))
            if len(self.hists) > MAX_HISTS:
                raise ValueError(f"{BINS_VAR}: {len(self.hists)} histograms, at most {MAX_HISTS}")
        dev.extremes_configure(history.entries_for(self.names), [(self.names.index(n), c, x) for n, c, x in self.thresholds],
                               [(self.names.index(n), e) for n, e in self.hists])

    def key(self):
        """The lane's part of a checkpoint's subsystem set."""
        thr = ",".join(threshold_label(*t) for t in self.thresholds)
        bins = ",".join(f"{n}:{e.size - 1}:{float(e[0])!r}:{float(e[-1])!r}:{zlib.crc32(e.tobytes()):08x}" for n, e in self.hists)
        return f"{','.join(self.names)}|{thr}|{bins}|every={self.sample_every}"

    def _upload(self, flags):
        self.dev.extremes_schedule(flags)

    def _window_file(self, complete):
        state = self.dev.extremes_read()
        count = state["n"]
        if count <= 0:
            return None
        t0s, t1s = self.window_labels()
        a, b = t0s / self.day, t1s / self.day
        lat = np.asarray(self.grid.lat, dtype=np.float64)
        lon = np.asarray(self.grid.lon, dtype=np.float64)
        dims, variables = window_variables(state, self.names, self.thresholds, self.hists, lat, lon, t0s, self.sample_every * self.dt)
        variables.update(n_samples=("i4", (), int(count)), t_start_seconds=("f8", (), t0s), t_end_seconds=("f8", (), t1s),
                         dt_seconds=("f8", (), self.dt), sample_every=("i4", (), self.sample_every),
                         complete=("i4", (), 1 if complete else 0))
        d = self.decimals
        top = np.where(state["tmax"][0] >= 0, state["vmax"][0], -np.inf)
        j, i = np.unravel_index(int(np.argmax(top)), top.shape)
        line = (f"[Extremes] day {a:.{d}f}–{b:.{d}f}: {count} samples | {self.names[0]} max={float(top[j, i]):.6g} at "
                f"({float(lat[j]):.2f}, {float(lon[i]):.2f})")
        if self.hists:
            n = self.hists[0][0]
            line += f" | {n} p99={float(variables[n.lower() + '_quantiles'][2][2]):.6g}"
        if self.thresholds:
            label = threshold_label(*self.thresholds[0])
            freq = variables[label.lower() + "_freq"][2]
            line += f"{' |' if not self.hists else ''} {label} freq={history.global_mean(freq, self.grid.lat_mesh):.6g}"
        return a, b, dims, variables, line

    def drop(self):
        self.dev.extremes_reset()
        super().drop()


def from_env(dev, grid, env, with_ocean=True, dt=None, day=None, out=print):
    """QD_EXTREMES (default 0) -> an Extremes on this handle, or None: at 0 nothing is configured, allocated, scheduled, launched,
    written or read."""
    cfg = read_env(env)
    if not cfg["enabled"]:
        return None
    return Extremes(dev, grid, cfg, with_ocean=with_ocean, dt=env_dt(env, dt), day=day, out=out)
