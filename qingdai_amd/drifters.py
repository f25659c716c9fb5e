"""
qingdai_amd/drifters.py -- Lagrangian drifters (QD_DRIFTERS=1), host side of csrc/qd_drift.hip.

Nothing the reference has.  Two populations of particles live on the device: `atm` follows the winds (U, V), `ocn` the currents
(UO, VO; needs the ocean).  The lane is the one span lane whose resident state moves: EVERY step of a span it takes part in advances
every live particle by one midpoint step on the planes as the step leaves them, and the scheduled steps also leave a record --
positions, status, the ocn population's blocked counts and the bilinear values of the sampled planes (QD_DRIFT_SAMPLE_ATM, default
TS,H; QD_DRIFT_SAMPLE_OCN, default SST) at the new positions -- in the lane's device log.  span_deliver drains the log into the open
window, and behind a window's last step the window is written to <QD_OUTPUT_DIR, default output>/drifters/drifters_day_{a}_{b}.nc.
The window clock and the labels are history's: window k is the steps [k S, (k + 1) S) of the run-local step index,
S = max(1, int(QD_DRIFT_EVERY_DAYS * day / dt + 0.5)), and every QD_DRIFT_EVERY-th step of a window records, counted from the
window's first step.  A record is large (it holds every particle), so the log holds few of them (Drifters.cap, what
qd_drift_configure returns): steps_to_window_end also ends a chunk where the log would be full.

advance_reference is the NumPy restatement of the device's step (the top of csrc/qd_drift.hip), bit for bit: the only definition
of the step outside the .hip.  Nothing here touches the device at import.
"""
from __future__ import annotations

import math

import numpy as np

from . import history
from ._lib import DRIFT_MAX, DRIFT_MAX_SAMPLES
from .window_lane import LogWindowLane, env_days, env_every, env_int, i8_code, window_file_name

SAMPLE_VARS = ("QD_DRIFT_SAMPLE_ATM", "QD_DRIFT_SAMPLE_OCN")
N_ATM, N_OCN, EVERY, EVERY_DAYS = 4096, 4096, 24, 10.0
DEFAULT_SAMPLES = (("TS", "H"), ("SST",))
POPS = ("atm", "ocn")


# ------------------------------------------------------------------------------------- the device's step, in NumPy
def sec_table(lat):
    """The row table of the zonal metric the device gets at configure time: S_j = 1 / max(cos lat_j, sin(dlat / 2)), lat in
    degrees.  The floor is the cosine half a row from the pole: the table stays finite there and a particle on the pole row moves
    zonally as one half a row away would."""
    lat = np.asarray(lat, dtype=np.float64).reshape(-1)
    dphi = np.deg2rad(lat[1] - lat[0])
    return 1.0 / np.maximum(np.cos(np.deg2rad(lat)), np.sin(dphi / 2.0))


def _cell(r, c, n_lat, n_lon):
    r0f, c0f = np.floor(r), np.floor(c)
    tr, tc = r - r0f, c - c0f
    r0 = np.clip(r0f.astype(np.int64), 0, n_lat - 1)
    c0 = np.clip(c0f.astype(np.int64), 0, n_lon - 2)
    return r0, np.minimum(r0 + 1, n_lat - 1), c0, c0 + 1, 1.0 - tr, tr, 1.0 - tc, tc


def _mix(f, K):
    r0, r1, c0, c1, wr0, wr1, wc0, wc1 = K
    t = np.zeros(r0.shape, dtype=np.float64)
    t = t + f[r0, c0] * wr0 * wc0
    t = t + f[r0, c1] * wr0 * wc1
    t = t + f[r1, c0] * wr1 * wc0
    t = t + f[r1, c1] * wr1 * wc1
    return t


def sample_reference(f, r, c):
    """The bilinear value of the plane f [n_lat][n_lon] at (r, c), r in [0, n_lat - 1], c in [0, n_lon - 1): the corner order of
    oracle numerics.bilinear_wrap, as the device takes it on a recording step."""
    f = np.asarray(f, dtype=np.float64)
    r, c = np.asarray(r, dtype=np.float64).reshape(-1), np.asarray(c, dtype=np.float64).reshape(-1)
    with np.errstate(all="ignore"):
        return _mix(f, _cell(r, c, *f.shape))


def fold(r, c, n_lat, n_lon):
    """One reflection at a pole (with half a turn in longitude), then the column into [0, P), P = n_lon - 1 -> (r, c, ok); ok is
    False where a coordinate is non-finite or the row is still outside [0, n_lat - 1] (r and c are then meaningless)."""
    r, c = np.array(r, dtype=np.float64), np.array(c, dtype=np.float64)
    rmax, P = np.float64(n_lat - 1), np.float64(n_lon - 1)
    with np.errstate(all="ignore"):
        ok = np.isfinite(r) & np.isfinite(c)
        south, north = r < 0.0, r > rmax
        r = np.where(south, -r, np.where(north, 2.0 * rmax - r, r))
        c = np.where(south | north, c + P / 2.0, c)
        ok = ok & (r >= 0.0) & (r <= rmax) & np.isfinite(c)
        c = c - P * np.floor(c / P)
        c = np.where((c >= 0.0) & (c < P), c, 0.0)
    return r, c, ok


def advance_reference(r, c, status, blocked, U, V, land, lat, dt, a, ocean):
    """One step of one population, as the device takes it -> (r, c, status, blocked), new arrays.  r, c, status, blocked [n] f64
    (blocked is carried unchanged when ocean is false); U, V [n_lat][n_lon] the two velocity planes; land [n_lat][n_lon], non-zero
    = land, read only when ocean; lat [n_lat] degrees; dt seconds; a the planet's radius."""
    U, V = np.asarray(U, dtype=np.float64), np.asarray(V, dtype=np.float64)
    n_lat, n_lon = U.shape
    lat = np.asarray(lat, dtype=np.float64).reshape(-1)
    S = sec_table(lat)
    dt, a = np.float64(dt), np.float64(a)
    adlat = a * np.deg2rad(lat[1] - lat[0])
    adlon = a * np.deg2rad(np.float64(360.0) / np.float64(n_lon - 1))
    r, c = np.array(r, dtype=np.float64).reshape(-1), np.array(c, dtype=np.float64).reshape(-1)
    status, blocked = np.array(status, dtype=np.float64).reshape(-1), np.array(blocked, dtype=np.float64).reshape(-1)
    live = status == 0.0

    def stage(rr, cc):
        K = _cell(rr, cc, n_lat, n_lon)
        u, v = _mix(U, K), _mix(V, K)
        sec = S[K[0]] * K[4] + S[K[1]] * K[5]
        dr, dc = v * dt / adlat, u * dt * sec / adlon
        return dr, dc, np.isfinite(u) & np.isfinite(v) & np.isfinite(dr) & np.isfinite(dc)

    with np.errstate(all="ignore"):
        dr0, dc0, ok = stage(r, c)
        rm, cm, okf = fold(r + dr0 / 2.0, c + dc0 / 2.0, n_lat, n_lon)
        ok = ok & okf
        rm, cm = np.where(ok, rm, r), np.where(ok, cm, c)           # (a failed particle's midpoint is never used)
        dr1, dc1, ok1 = stage(rm, cm)
        rn, cn, okf = fold(r + dr1, c + dc1, n_lat, n_lon)
        ok = ok & ok1 & okf
        move = live & ok
        if ocean:
            jr = np.clip(np.floor(np.where(ok, rn, 0.0) + 0.5).astype(np.int64), 0, n_lat - 1)
            jc = np.clip(np.floor(np.where(ok, cn, 0.0) + 0.5).astype(np.int64), 0, n_lon - 1)
            jc = np.where(jc == n_lon - 1, 0, jc)
            wet = np.asarray(land)[jr, jc] == 0
            blocked = np.where(move & ~wet, blocked + 1.0, blocked)
            move = move & wet
    status = np.where(live & ~ok, 1.0, status)
    return np.where(move, rn, r), np.where(move, cn, c), status, blocked


# ------------------------------------------------------------------------------------- coordinates and seeds
def to_index(lat_deg, lon_deg, grid):
    """Degrees -> (r, c): r = (lat + 90) / dlat, clipped to [0, n_lat - 1]; c = lon / dlon taken into [0, n_lon - 1)."""
    n_lat, n_lon = int(grid.n_lat), int(grid.n_lon)
    lat = np.asarray(lat_deg, dtype=np.float64).reshape(-1)
    lon = np.asarray(lon_deg, dtype=np.float64).reshape(-1)
    if lat.shape != lon.shape:
        raise ValueError("drifters: a seed list holds one longitude per latitude")
    if not (np.isfinite(lat).all() and np.isfinite(lon).all()):
        raise ValueError("drifters: a seed coordinate is not finite")
    P = np.float64(n_lon - 1)
    r = np.clip((lat + 90.0) / (180.0 / (n_lat - 1)), 0.0, np.float64(n_lat - 1))
    c = lon / (360.0 / P)
    c = c - P * np.floor(c / P)
    return r, np.where((c >= 0.0) & (c < P), c, 0.0)


def to_degrees(r, c, n_lat, n_lon):
    """(r, c) -> (lat, lon) in degrees: -90 + r dlat, c dlon."""
    return -90.0 + np.asarray(r, dtype=np.float64) * (180.0 / (n_lat - 1)), np.asarray(c, dtype=np.float64) * (360.0 / (n_lon - 1))


def nearest_cell(r, c, n_lon):
    """The cell nearest to (r, c): (floor(r + 0.5), floor(c + 0.5)), column n_lon - 1 taken as column 0."""
    jr = np.floor(np.asarray(r) + 0.5).astype(np.int64)
    jc = np.floor(np.asarray(c) + 0.5).astype(np.int64)
    return jr, np.where(jc == n_lon - 1, 0, jc)


def seed_fibonacci(n, grid, land_mask=None):
    """n points of the Fibonacci sphere lattice (point i at sin lat = 1 - (2 i + 1) / n, lon = i * the golden angle), as (r, c);
    with a land mask only those whose nearest cell is ocean (so fewer than n).  Deterministic: no generator."""
    n = int(n)
    if n <= 0:
        return np.empty(0), np.empty(0)
    i = np.arange(n, dtype=np.float64)
    lat = np.rad2deg(np.arcsin(np.clip(1.0 - (2.0 * i + 1.0) / n, -1.0, 1.0)))
    golden = 180.0 * (3.0 - math.sqrt(5.0))                       # degrees
    r, c = to_index(lat, np.mod(i * golden, 360.0), grid)
    if land_mask is not None:
        jr, jc = nearest_cell(r, c, int(grid.n_lon))
        keep = np.asarray(land_mask)[jr, jc] == 0
        r, c = r[keep], c[keep]
    return r, c


# ------------------------------------------------------------------------------------- environment
def parse_samples(text, var):
    """A sample list through history's parser: f64 planes only (no derived speed), at most 4, never PRECIP."""
    names = history.parse_fields(text, var=var)
    for n in names:
        if n in history.DERIVED:
            raise ValueError(f"{var}: '{n}' is no plane (the drifters sample f64 planes)")
        if n == "PRECIP":
            raise ValueError(f"{var}: PRECIP cannot be sampled: inside a span the hoisted precipitation block has overwritten it with "
                             f"the next step's before the lane reads")
    if len(names) > DRIFT_MAX_SAMPLES:
        raise ValueError(f"{var}: {len(names)} fields, at most {DRIFT_MAX_SAMPLES}")
    return names


def read_env(env):
    """-> dict: enabled (QD_DRIFTERS, default 0), n_atm / n_ocn (QD_DRIFT_N_ATM / QD_DRIFT_N_OCN, default 4096 each; unparsable ->
    the default; outside [0, 2^20] raises), every (QD_DRIFT_EVERY, default 24; unparsable or < 1 -> 24), every_days
    (QD_DRIFT_EVERY_DAYS, default 10; unparsable or <= 0 -> 10), sample_atm / sample_ocn (QD_DRIFT_SAMPLE_ATM, default TS,H;
    QD_DRIFT_SAMPLE_OCN, default SST; an empty value samples nothing), log_cap (QD_DRIFT_LOG_CAP: fewer records per chunk than the
    device log holds, for tests; None = the device's)."""
    enabled = env_int(env, "QD_DRIFTERS", 0) == 1
    counts = []
    for name, default in (("QD_DRIFT_N_ATM", N_ATM), ("QD_DRIFT_N_OCN", N_OCN)):
        k = env_int(env, name, default)
        if enabled and not 0 <= k <= DRIFT_MAX:
            raise ValueError(f"{name}: {k} particles, a population holds 0 to {DRIFT_MAX}")
        counts.append(k)
    samples = []
    for var, default in zip(SAMPLE_VARS, DEFAULT_SAMPLES):
        text = env.get(var)
        samples.append(list(default) if text is None else (parse_samples(text, var) if enabled else []))
    cap = env_int(env, "QD_DRIFT_LOG_CAP", 0)
    return {"enabled": enabled, "n_atm": counts[0], "n_ocn": counts[1], "every": env_every(env, "QD_DRIFT_EVERY", EVERY),
            "every_days": env_days(env, "QD_DRIFT_EVERY_DAYS", EVERY_DAYS),
            "sample_atm": samples[0], "sample_ocn": samples[1], "log_cap": cap if cap >= 1 else None}


def default_config(**over):
    cfg = read_env({})
    cfg["enabled"] = True
    cfg.update(over)
    return cfg


# ------------------------------------------------------------------------------------- records and the window file
def block_rows(pop, n_samples):
    """Rows of [n] doubles a population has in a record: r | c | status [| blocked] | samples."""
    return (4 if pop == "ocn" else 3) + int(n_samples)


def record_width(n_atm, ns_atm, n_ocn, ns_ocn):
    return int(n_atm) * block_rows("atm", ns_atm) + int(n_ocn) * block_rows("ocn", ns_ocn)


def log_capacity(width):
    """Records the device log holds between two drains: max(1, min(16, floor(256 MiB / record bytes)))."""
    return max(1, min(16, (256 << 20) // max(1, 8 * int(width))))


def split_records(recs, n_atm, ns_atm, n_ocn, ns_ocn):
    """[k][width] records -> {"atm": [k][3 + ns_atm][n_atm], "ocn": [k][4 + ns_ocn][n_ocn]}."""
    recs = np.asarray(recs, dtype=np.float64).reshape(-1, record_width(n_atm, ns_atm, n_ocn, ns_ocn))
    cut = int(n_atm) * block_rows("atm", ns_atm)
    return {"atm": recs[:, :cut].reshape(len(recs), block_rows("atm", ns_atm), int(n_atm)),
            "ocn": recs[:, cut:].reshape(len(recs), block_rows("ocn", ns_ocn), int(n_ocn))}


def file_name(a_days, b_days, decimals=1):
    return window_file_name("drifters", a_days, b_days, decimals)


def window_variables(parts, samples, times, steps, shape, dt, every, complete):
    """One window as ncio.write_nc takes it -> (dims, variables).  parts: split_records' dict; samples: {"atm": names, "ocn":
    names}; shape (n_lat, n_lon).  A population without particles has no variables."""
    n = int(len(times))
    dims = {"time": n}
    v = {"time_seconds": ("f8", ("time",), np.asarray(times, dtype=np.float64).reshape(n)),
         "step": (i8_code(), ("time",), np.asarray(steps, dtype=np.int64).reshape(n))}
    for pop in POPS:
        b = parts[pop]
        if b.shape[2] == 0:
            continue
        dim = f"particle_{pop}"
        dims[dim] = int(b.shape[2])
        lat, lon = to_degrees(b[:, 0, :], b[:, 1, :], *shape)
        v[f"{pop}_lat"] = ("f8", ("time", dim), np.ascontiguousarray(lat))
        v[f"{pop}_lon"] = ("f8", ("time", dim), np.ascontiguousarray(lon))
        v[f"{pop}_status"] = ("i4", ("time", dim), b[:, 2, :].astype(np.int32))
        first = 3
        if pop == "ocn":
            v["ocn_blocked"] = ("i4", ("time", dim), b[:, 3, :].astype(np.int32))
            first = 4
        for k, name in enumerate(samples[pop]):
            v[f"{pop}_{name.lower()}"] = ("f8", ("time", dim), np.ascontiguousarray(b[:, first + k, :]))
    v.update(dt_seconds=("f8", (), float(dt)), sample_every=("i4", (), int(every)), complete=("i4", (), 1 if complete else 0))
    return dims, v


class Drifters(LogWindowLane):
    """The lane's participant in Device.step_n: the clock and the span protocol are window_lane's (the flags name the steps that
    record; every step of the span advances), flush() writes the window's file.  drop() forgets the delivered records only: _pending
    and the device log stay as they are.  `sim` gives dev, grid, ocean (None = off), dt, day_seconds and land_mask.  Seeds:
    atm=(lat, lon) and / or ocn=(lat, lon) in degrees, the caller's own; with neither, cfg's counts of Fibonacci lattice points (ocn:
    those over ocean)."""
    NAME, TAG = "drifters", "Drifters"

    def __init__(self, sim, atm=None, ocn=None, cfg=None, out=print, output_dir=None):
        cfg = default_config() if cfg is None else dict(cfg)
        dev, grid = sim.dev, sim.grid
        self.with_ocean = getattr(sim, "ocean", None) is not None
        self.shape = (int(grid.n_lat), int(grid.n_lon))
        land = np.asarray(sim.land_mask)
        if atm is None and ocn is None:
            seeds = {"atm": seed_fibonacci(cfg["n_atm"], grid),
                     "ocn": seed_fibonacci(cfg["n_ocn"], grid, land) if self.with_ocean else (np.empty(0), np.empty(0))}
        else:
            seeds = {p: to_index(*s, grid) if s is not None else (np.empty(0), np.empty(0)) for p, s in (("atm", atm), ("ocn", ocn))}
        if len(seeds["ocn"][0]) and not self.with_ocean:
            raise ValueError("drifters: the ocn population needs the ocean, which is off in this run (QD_USE_OCEAN)")
        for p in POPS:
            if len(seeds[p][0]) > DRIFT_MAX:
                raise ValueError(f"drifters: {len(seeds[p][0])} {p} particles, a population holds at most {DRIFT_MAX}")
        self.n = {p: int(len(seeds[p][0])) for p in POPS}
        self.samples = {"atm": list(cfg["sample_atm"]) if self.n["atm"] else [], "ocn": list(cfg["sample_ocn"]) if self.n["ocn"] else []}
        for p, var in zip(POPS, SAMPLE_VARS):
            for name in self.samples[p]:
                if name in history.OCEAN_ONLY and not self.with_ocean:
                    raise ValueError(f"{var}: field '{name}' needs the ocean, which is off in this run (QD_USE_OCEAN)")
        width = record_width(self.n["atm"], len(self.samples["atm"]), self.n["ocn"], len(self.samples["ocn"]))
        super().__init__(dev, grid, cfg, out, sim.dt, sim.day_seconds, cfg["every_days"], cfg["every"], width, output_dir)
        self.device_cap = dev.drift_configure(seeds["atm"], seeds["ocn"], self.samples["atm"], self.samples["ocn"],
                                              sec_table(grid.lat))
        self.cap = self.device_cap if cfg.get("log_cap") is None else max(1, min(self.device_cap, int(cfg["log_cap"])))

    def key(self):
        """The lane's place in a checkpoint's subsystem set."""
        return "|".join(f"{p}={self.n[p]}:{','.join(self.samples[p])}" for p in POPS) + f"|every={self.every}"

    def _upload(self, flags):
        self.dev.drift_schedule(flags)

    def _drain(self, want):
        return self.dev.drift_log(want)

    def steps_to_window_end(self, i=None):
        """Steps from step i (default: the next step) up to and including the earlier of its window's last step and the step whose
        record fills the device log (self.cap records since the last drain, and every span is drained)."""
        i = self.i if i is None else int(i)
        pos = i % self.S
        first = -(-pos // self.every) * self.every                 # the next recording position of the window
        room = first + (self.cap - 1) * self.every - pos + 1       # steps up to and including the cap-th record from here
        return min(self.S - pos, room)

    def split(self, recs):
        return split_records(recs, self.n["atm"], len(self.samples["atm"]), self.n["ocn"], len(self.samples["ocn"]))

    def state(self):
        """The particles as they stand -> {"atm": [3][n_atm] r | c | status, "ocn": [4][n_ocn] r | c | status | blocked}."""
        atm, ocn = self.dev.drift_state()
        return {"atm": atm, "ocn": ocn}

    def restore_state(self, atm, ocn):
        self.dev.drift_state_set(atm, ocn)

    def _window_file(self, complete):
        recs, times, steps = self.window()
        if len(recs) == 0:
            return None
        a, b = float(times[0]) / self.day, float(times[-1]) / self.day
        parts = self.split(recs)
        dims, variables = window_variables(parts, self.samples, times, steps, self.shape, self.dt, self.every, complete)
        d = self.decimals
        dead = {p: int(parts[p][-1, 2, :].sum()) for p in POPS}
        line = (f"[Drifters] day {a:.{d}f}–{b:.{d}f}: {len(recs)} records | atm {self.n['atm'] - dead['atm']}/{dead['atm']} | "
                f"ocn {self.n['ocn'] - dead['ocn']}/{dead['ocn']}/{int(parts['ocn'][-1, 3, :].sum()) if self.n['ocn'] else 0}")
        return a, b, dims, variables, line


def from_env(sim, env, out=print):
    """QD_DRIFTERS (default 0) -> a Drifters on the run's handle, or None: at 0 nothing is configured, allocated, scheduled or
    launched."""
    cfg = read_env(env)
    if not cfg["enabled"]:
        return None
    return Drifters(sim, cfg=cfg, out=out)
