"""
qingdai_amd/eddy.py -- eddy statistics: covariances and transports (QD_EDDY=1), host side of csrc/qd_eddy.hip.

Nothing the reference has.  Climate is described by first and second moments, and the mean of a product is not the product of the
means: on every sampled step of the device loop the lane adds, per cell, the deviation of each selected field from an anchor and the
products of the selected pairs of deviations into resident planes (a span lane without a flag bit and without a log, like the
history accumulators).  Behind a window's last step the sums become, per pair (A, B) and latitude row, the zonal-mean transport
[A B] and its three parts -- mean meridional, stationary waves, transient eddies -- and, with QD_EDDY_MAPS=1, maps of the transient
covariance and of the time means, in <QD_OUTPUT_DIR, default output>/eddy/eddy_day_{a}_{b}.nc, labelled like the history files.
The window clock is history's: window k is the steps [k S, (k + 1) S) with S = max(1, int(QD_EDDY_EVERY_DAYS * day / dt + 0.5)),
and every QD_EDDY_SAMPLE_EVERY-th step of a window is sampled, counted from the window's first step.  A sample of a field for step
i is what Device.get returns after a span that ends with step i.

The definition of a sample is the top of csrc/qd_eddy.hip; accumulate_reference restates it bit for bit and is the only other
statement.  zonal_reference restates k_eddy_zonal's summation order (the row stage of series.reduce_reference).

The decomposition (decompose), per pair (p, q) and row, with N samples, n = n_lon columns, [.] the zonal and an overbar the time mean,
abar = r + S / N per cell, x* = x - [x]:
    total       [mean(a b)]         = mean + stationary + transient, DEFINED as that sum, so the identity is exact
    mean        [abar][bbar]          the mean meridional part
    stationary  [abar* bbar*]       = sum(abar* bbar*) / n, from the deviations themselves (two passes over a row, on the host)
    transient   [mean(a' b')]       = sum(C) / (n N) - sum(S_p S_q) / (n N^2)
The transient part is a covariance in time, cell by cell: it does not change when an anchor is taken from each cell's series and
needs only two of the four row sums of k_eddy_zonal.  The mean and the stationary part are about the time means themselves, which
need the anchors -- an anchor is a value per CELL, so the zonal covariance of S_p / N and S_q / N is the stationary part of
abar - r, not of abar (with the anchor at the first sample it is the covariance of the first sample's eddies).  The host therefore
forms [abar] and [abar* bbar*] from the anchor and sum planes it downloads at the window's end, maps on or off (the choice among the
two forms the design allows for the anchor terms: one code path, and 2 F planes once per window are nothing beside the samples).
qd_eddy_zonal still delivers all four sums; sum(S_p) and sum(S_q) are there for a caller who wants the zonal means of the
deviations.

Nothing here touches the device at import; the parser, the clock, the arithmetic and the file writing are plain NumPy
(tests/test_eddy_cpu.py).
"""
from __future__ import annotations

import numpy as np

from . import history, order
from ._lib import C as _C, FIELDS
from .window_lane import SumWindowLane, env_days, env_dt, env_every, env_int, window_file_name

PAIRS_VAR = "QD_EDDY_PAIRS"
DEFAULT_PAIRS = "U*V,V*TS,V*Q,V*H,U*U,V*V,H*H,TS*TS"
MAX_FIELDS, MAX_PAIRS = _C["QD_EDDY_MAX_FIELDS"], _C["QD_EDDY_MAX_PAIRS"]
EVERY_DAYS, MAPS = 10.0, 1
# A guess at a cost of a few percent of a step: one sample moves 288 bytes per cell at the default pairs (derived from the sizes).
# Nobody has measured which cadence the statistics need; DESIGN.md section 7 holds what a sample costs.
SAMPLE_EVERY = 4
PARTS = ("total", "mean", "stationary", "transient")


# ------------------------------------------------------------------------------------- the pair list
def parse_pairs(text, var=PAIRS_VAR):
    """'U*V,V*TS,U*U' -> (fields, pairs, labels): the distinct field names in order of first appearance, [(p, q)] indices into them,
    [(A, B)] the names as written.  Names go through history's field table.  Refused with a ValueError that names the item: an
    item that is not A*B, an unknown field, a derived entry (WIND_SPEED, CURRENT_SPEED), PRECIP, a pair named twice in either
    order, an empty list, more than 16 fields or 32 pairs."""
    fields, pairs, labels = [], [], []
    for item in (s.strip().upper() for s in str(text).split(",")):
        if not item:
            continue
        ab = [s.strip() for s in item.split("*")]
        if len(ab) != 2 or not all(ab):
            raise ValueError(f"{var}: '{item}' is not a pair A*B")
        for n in ab:
            if n in history.DERIVED:
                raise ValueError(f"{var}: '{n}' is a derived entry; a pair takes f64 planes only")
            if n not in FIELDS:
                raise ValueError(f"{var}: unknown field '{n}' (an f64 plane as Device.get takes it)")
            if n == "PRECIP":
                raise ValueError(f"{var}: PRECIP is sampled in front of the ocean step, every other field behind the step's last "
                                 f"launch: a product across the two places has no meaning")
            if n not in fields:
                fields.append(n)
        pq = (fields.index(ab[0]), fields.index(ab[1]))
        if pq in pairs or pq[::-1] in pairs:
            raise ValueError(f"{var}: the pair '{item}' is named twice (the order of the two fields does not count)")
        pairs.append(pq)
        labels.append((ab[0], ab[1]))
    if not pairs:
        raise ValueError(f"{var}: no pair")
    if len(fields) > MAX_FIELDS:
        raise ValueError(f"{var}: {len(fields)} fields, at most {MAX_FIELDS}")
    if len(pairs) > MAX_PAIRS:
        raise ValueError(f"{var}: {len(pairs)} pairs, at most {MAX_PAIRS}")
    return fields, pairs, labels


def read_env(env):
    """-> dict: enabled (QD_EDDY, default 0), pairs (QD_EDDY_PAIRS as text, upper-cased; the default list when unset or empty;
    parsed -- and refused -- only when the lane is on), sample_every (QD_EDDY_SAMPLE_EVERY, default 4; unparsable or < 1 -> 4),
    every_days (QD_EDDY_EVERY_DAYS, default 10; unparsable or <= 0 -> 10), maps (QD_EDDY_MAPS, default 1)."""
    enabled = env_int(env, "QD_EDDY", 0) == 1
    text = env.get(PAIRS_VAR)
    text = DEFAULT_PAIRS if text is None or not str(text).strip() else ",".join(s.strip().upper() for s in str(text).split(",") if s.strip())
    if enabled:
        parse_pairs(text)
    return {"enabled": enabled, "pairs": text, "sample_every": env_every(env, "QD_EDDY_SAMPLE_EVERY", SAMPLE_EVERY),
            "every_days": env_days(env, "QD_EDDY_EVERY_DAYS", EVERY_DAYS), "maps": env_int(env, "QD_EDDY_MAPS", MAPS) != 0}


def file_name(a_days, b_days, decimals=1):
    return window_file_name("eddy", a_days, b_days, decimals)


# ------------------------------------------------------------------------------------- the definition, in NumPy
def accumulate_reference(samples, pairs, state=None):
    """The lane's state after the samples, bit for bit -> (r [F][...], S [F][...], C [P][...], N).
    samples: an iterable of [F][...] f64 arrays, one per sample, in step order; pairs: [(p, q)]; state: what an earlier call
    returned, to go on from (None: a window's start).  Per cell, every operation rounded on its own:
        the first sample of a window       r_f = a_f
        every sample (the first included)  d_f = a_f - r_f;  S_f = S_f + d_f;  C_k = C_k + (d_p * d_q)
    No compensation, no special case for a non-finite value (inf - inf is NaN and stays)."""
    r, S, Cs, N = (None, None, None, 0) if state is None else state
    if state is not None:
        r, S, Cs = np.array(r, dtype=np.float64), np.array(S, dtype=np.float64), np.array(Cs, dtype=np.float64)
    with np.errstate(invalid="ignore", over="ignore"):
        for a in samples:
            a = np.asarray(a, dtype=np.float64)
            if N == 0:
                r = a.copy()
                S = np.zeros_like(a)
                Cs = np.zeros((len(pairs),) + a.shape[1:])
            d = a - r
            S = S + d
            for k, (p, q) in enumerate(pairs):
                Cs[k] = Cs[k] + (d[p] * d[q])
            N += 1
    return r, S, Cs, N


def _row_sums(x):
    """[..., n_lon] -> [...]: k_eddy_zonal's order, the row stage of series.reduce_reference: lane l of a row's wave owns the cells
    128 m + 2 l and 128 m + 2 l + 1 and adds them in ascending order into one accumulator that starts at +0.0; then the five
    halvings.  (A cell past the row's end is no add on the device and an add of +0.0 here, which changes no bit.)"""
    x = np.ascontiguousarray(x, dtype=np.float64)
    cells = order.lanes(x, 128, 0.0)
    cells = cells.reshape(x.shape[:-1] + (cells.shape[-2], 64, 2))
    acc = np.zeros(x.shape[:-1] + (64,))
    for m in range(cells.shape[-3]):
        acc = acc + cells[..., m, :, 0]
        acc = acc + cells[..., m, :, 1]
    return order.wave(acc, np.add)


def zonal_reference(S, Cs, pairs):
    """qd_eddy_zonal, bit for bit -> [P][4][n_lat]: per pair and row the sums over all columns of S_p, S_q, C_k and S_p * S_q
    (the product rounded)."""
    S, Cs = np.asarray(S, dtype=np.float64), np.asarray(Cs, dtype=np.float64)
    out = np.empty((len(pairs), 4, S.shape[1]))
    with np.errstate(invalid="ignore", over="ignore"):
        for k, (p, q) in enumerate(pairs):
            out[k] = _row_sums(np.stack([S[p], S[q], Cs[k], S[p] * S[q]]))
    return out


def time_means(anchors, sums, count):
    """abar = r + S / N per field and cell."""
    with np.errstate(invalid="ignore", over="ignore", divide="ignore"):
        return np.asarray(anchors, dtype=np.float64) + np.asarray(sums, dtype=np.float64) / np.float64(count)


def decompose(zonal, count, abar, pairs):
    """The four parts per pair and row, in f64 -> {total, mean, stationary, transient}, each [P][n_lat].
    zonal [P][4][n_lat]: qd_eddy_zonal's sums; count: N; abar [F][n_lat][n_lon]: the fields' time means (time_means); pairs:
    [(p, q)].  [x] is np.sum over the columns / n_lon.  total is defined as (mean + stationary) + transient: the identity holds
    exactly."""
    z = np.asarray(zonal, dtype=np.float64)
    abar = np.asarray(abar, dtype=np.float64)
    n, N = np.float64(abar.shape[-1]), np.float64(count)
    sc, sx = z[:, 2], z[:, 3]
    with np.errstate(invalid="ignore", over="ignore", divide="ignore"):
        zm = np.sum(abar, axis=-1) / n                              # [F][n_lat]
        star = abar - zm[..., None]
        mean = np.stack([zm[p] * zm[q] for p, q in pairs])
        stationary = np.stack([np.sum(star[p] * star[q], axis=-1) / n for p, q in pairs])
        transient = sc / (n * N) - sx / (n * N * N)
        total = (mean + stationary) + transient
    return {"total": total, "mean": mean, "stationary": stationary, "transient": transient}


def covariance_maps(sums, pair_sums, pairs, count):
    """The transient covariance per cell, C / N - (S_p / N)(S_q / N) -> [P][n_lat][n_lon]"""
    N = np.float64(count)
    with np.errstate(invalid="ignore", over="ignore", divide="ignore"):
        return np.stack([pair_sums[k] / N - (sums[p] / N) * (sums[q] / N) for k, (p, q) in enumerate(pairs)])


# ------------------------------------------------------------------------------------- the lane
class Eddy(SumWindowLane):
    """The lane's participant in Device.step_n: the clock and the span protocol are window_lane's, flush() turns the resident sums
    into one file.  drop() zeroes the device's planes and count and forgets the labels."""
    NAME, TAG = "eddy", "Eddy"

    def __init__(self, dev, grid, cfg, with_ocean=True, dt=300.0, day=None, out=print, output_dir=None):
        super().__init__(dev, grid, cfg, out, dt, day, cfg["every_days"], cfg["sample_every"], output_dir)
        self.text = str(cfg.get("pairs") or DEFAULT_PAIRS)
        self.fields, self.pairs, self.labels = parse_pairs(self.text)
        history.resolve_fields(self.fields, with_ocean, var=PAIRS_VAR)     # a field of a subsystem that is off is refused
        self.maps = bool(cfg.get("maps", True))
        dev.eddy_configure(self.fields, self.pairs)

    def key(self):
        """The lane's part of a checkpoint's subsystem set."""
        return f"{self.text}|every={self.sample_every}|maps={int(self.maps)}"

    def _upload(self, flags):
        self.dev.eddy_schedule(flags)

    def _window_file(self, complete):
        """Reduce the rows on the device, read the planes, decompose -> the window's file, or None when it holds no sample."""
        anchors, sums, pair_sums, count = self.dev.eddy_read()
        if count <= 0:
            return None
        zonal = self.dev.eddy_zonal()
        t0s, t1s = self.window_labels()
        a, b = t0s / self.day, t1s / self.day
        abar = time_means(anchors, sums, count)
        parts = decompose(zonal, count, abar, self.pairs)
        lat = np.asarray(self.grid.lat, dtype=np.float64)
        variables = {"lat": ("f8", ("lat",), lat), "lon": ("f8", ("lon",), np.asarray(self.grid.lon, dtype=np.float64))}
        for k, (A, B) in enumerate(self.labels):
            for part in PARTS:
                variables[f"{A}_{B}_{part}".lower()] = ("f8", ("lat",), parts[part][k])
        if self.maps:
            for k, cov in enumerate(covariance_maps(sums, pair_sums, self.pairs, count)):
                variables["{}_{}_cov".format(*self.labels[k]).lower()] = ("f8", ("lat", "lon"), cov)
            for name, plane in zip(self.fields, abar):
                variables[f"{name}_mean".lower()] = ("f8", ("lat", "lon"), plane)
        variables.update(n_samples=("i4", (), int(count)), t_start_seconds=("f8", (), t0s), t_end_seconds=("f8", (), t1s),
                         dt_seconds=("f8", (), self.dt), sample_every=("i4", (), self.sample_every), maps=("i4", (), int(self.maps)),
                         complete=("i4", (), 1 if complete else 0))
        tr = parts["transient"][0]
        if np.isnan(tr).all():
            where, value = float("nan"), float("nan")
        else:
            j = int(np.nanargmax(np.abs(tr)))
            where, value = float(lat[j]), float(tr[j])
        d = self.decimals
        line = (f"[Eddy] day {a:.{d}f}–{b:.{d}f}: {count} samples | {self.labels[0][0]}*{self.labels[0][1]} transient "
                f"max |.| at lat {where:.2f}: {value:.6g}")
        return a, b, {"lat": int(self.grid.n_lat), "lon": int(self.grid.n_lon)}, variables, line

    def drop(self):
        self.dev.eddy_reset()
        super().drop()


def from_env(dev, grid, env, with_ocean=True, dt=None, day=None, out=print):
    """QD_EDDY (default 0) -> an Eddy on this handle, or None: at 0 nothing is configured, allocated, scheduled or launched."""
    cfg = read_env(env)
    if not cfg["enabled"]:
        return None
    return Eddy(dev, grid, cfg, with_ocean=with_ocean, dt=env_dt(env, dt), day=day, out=out)
