"""
qingdai_amd/checkpoint.py -- bit-for-bit checkpoint and resume of the whole resident state (QD_CHECKPOINT), checked by the device
state digest (include/qingdai_hip.h: qd_state_digest).  Nothing the reference has: its restart file holds 14 planes as f4 and
t_seconds, and a run resumed from it does not continue the run that was stopped.  A run cut in two by `save` and `load` here equals
the uncut run, bit for bit, in every plane `Device.get` returns.

The file (one NetCDF file through ncio.write_nc, f8 / u1 / i8 only; written to a temporary name and moved into place):
  f_<NAME>            every f64 field of _lib.FIELDS as f8 (a map the ecology keeps as f32 is saved as the f8 image of its f32 values)
  m_LAND_MASK, m_ICE_MASK   u1
  phyto_C             the tracers [species, lat, lon]; PHYTO_N, KD490 and WATER_ALPHA are fields
  route_buffer, route_flow, route_lakes, route_clock {t_accum, steps, an event has happened}
  hist_sums, hist_clock {i, t_first, t_last, n_open, count}       an open history window continues
  series_records, series_times, series_steps, series_clock {i, records}   an open series window continues (QD_SERIES=1 only; host
                      data: the records were reduced on the device and enter no digest)
  spectra_records, spectra_times, spectra_steps, spectra_clock {i, records, count}, spectra_sums   an open spectra window continues
                      (QD_SPECTRA=1 only); the lat-resolved sum planes (QD_SPECTRA_LAT=1) are resident and digested as SPECTRA_SUMS
  qd_*                the ecology's own exact-resume variables (ecology.py: EcologyAdapter._extension_variables), not restated here
  flow_records, flow_times, flow_steps, flow_clock {i, records, count}, flow_sums   an open flow window continues (QD_FLOW=1 only);
                      the four sum planes are resident and digested as FLOW_SUMS
  spharm_records, spharm_times, spharm_steps, spharm_clock {i, records, count}, spharm_sums   an open spherical-harmonic window
                      continues (QD_SPHARM=1 only); the 2D sum planes (QD_SPHARM_2D=1) are resident and digested as SPHARM_SUMS
  eddy_anchors, eddy_sums, eddy_pair_sums, eddy_clock {i, t_first, t_last, n_open, count}   an open eddy window continues (QD_EDDY=1
                      only); the planes are resident and digested as EDDY_ANCHORS and EDDY_SUMS (sums and pair sums as one plane)
  extremes_values [2][E] (vmax, vmin), extremes_counts [3][E] (tmax, tmin, nan; i4), extremes_thresholds [T][lat][lon][4] (i4: the
                      u32 words), extremes_hist (every table, one behind the other), extremes_clock {i, t_first, t_last, n_open,
                      count}   an open extremes window continues (QD_EXTREMES=1 only); digested as EXTREMES_VALUES,
                      EXTREMES_COUNTS (thresholds, then counts, as one plane of 4-byte words) and EXTREMES_HIST
  drift_atm, drift_ocn, drift_records, drift_times, drift_steps, drift_clock {i, records}   the drifters' particle state (r | c |
                      status [| blocked], f8) and their open window (QD_DRIFTERS=1 only)
  atm_counter, ocn_counter, step_index, span_mark {step index, atm counter at the last span's end}, t_seconds, t_origin {t0, steps
  since, their dt}, diversity_next_day,
  phyto_clock {phyto_next_time, daily steps}, state_scalars (qd_state_scalars_get: cloud_eff_valid, the ecology sub-step's clock and
  cache flags, the individuals' sub-step accumulator, the daily lanes' firing counts, the last energy-budget means), qnet_lw
  {qnet_lw_eps0, qnet_lw_kc as the autotuner left them}, params_bytes (the qd_params struct)
  attributes          abi_version, n_lat, n_lon, code_hash, subsystems, digest_<plane> and run_digest as hex strings (classic NetCDF
                      has no 64-bit unsigned type)
Not carried, because each is documented as bit-identical either way or is no state of the run: the median predictors, the tail-fix
form and its probe clock; the closure memory of the budget diagnostics (the first firing after a resume prints without its d/dt
part, as at start); the timing tables; the band stack of the daily phytoplankton step (an output of every daily step that only the
true-colour frame reads); the event and diagnostic logs, which every span drains.
"""
from __future__ import annotations

import ctypes
import os

import numpy as np

from . import _lib, ncio
from ._lib import FIELDS
from .window_lane import env_int as _int, i8_code as _i8

KEYED_LANES = ("series", "spectra", "flow", "spharm", "eddy", "extremes", "drifters")     # the order check_subsystems tests them in

ABI_VERSION = 1                      # QD_ABI_VERSION as of this module (tests/test_state_digest_cpu.py holds it to the header); a handle's
                                     # own library is asked where there is one (abi_version)
DEFAULT_NAME = "checkpoint.nc"
F32_MAPS = ("ECO_LAI", "ECO_LAI_SNAP", "ECO_F", "ECO_ALPHA", "ECO_ALPHA_BANDED")      # qd_eco_params.map_f32
_GOLD, _M1, _M2 = np.uint64(0x9E3779B97F4A7C15), np.uint64(0xBF58476D1CE4E5B9), np.uint64(0x94D049BB133111EB)
_MASK = (1 << 64) - 1


class CheckpointRefused(RuntimeError):
    """The file does not fit this run; nothing of the run has been touched.  str() is the reason of the [Checkpoint] refused line."""


class CheckpointInconsistent(RuntimeError):
    """The run is not at a span boundary -- the device is ahead of the host clocks, as right behind a qd_step_n call whose
    bookkeeping has not run (a signal handler, an error inside a span): nothing is written and the last good file stays."""


def abi_version(dev=None):
    """QD_ABI_VERSION of the library the handle runs on (this module's constant for a handle without one)."""
    lib = getattr(dev, "lib", None)
    return int(lib.qd_abi_version()) if lib is not None else ABI_VERSION


def span_consistent(sim):
    """-> None when the host clocks and the device agree, else the reason.  Simulation keeps `_span_mark` = (step index, device atm
    counter) as they stood when the bookkeeping of the last span was done (or at the load, or at construction), and `_in_span` while
    one is in flight."""
    if getattr(sim, "_in_span", False):
        return "a span is in flight: the device is ahead of the host clocks"
    mark = getattr(sim, "_span_mark", None)
    if mark is None:
        return None
    atm = int(sim.dev.counters()[0])
    if int(mark[0]) != int(sim._step_index) or int(mark[1]) != atm:
        return (f"the device is not where the host clocks are (step index {int(sim._step_index)}, device counter {atm}; at the last "
                f"span's end {int(mark[0])} and {int(mark[1])})")
    return None


# ------------------------------------------------------------------------------------- environment
def read_env(env=None, data_dir=None):
    """QD_CHECKPOINT (default 0), QD_CHECKPOINT_PATH (default <QD_DATA_DIR>/checkpoint.nc), QD_CHECKPOINT_STRICT (default 1)."""
    env = os.environ if env is None else env
    data_dir = env.get("QD_DATA_DIR", "data") if data_dir is None else data_dir
    path = env.get("QD_CHECKPOINT_PATH") or os.path.join(data_dir, DEFAULT_NAME)
    return {"enabled": _int(env, "QD_CHECKPOINT", 0) == 1, "path": path, "strict": _int(env, "QD_CHECKPOINT_STRICT", 1) != 0}


def startup_refusal(sim, env=None):
    """What QD_CHECKPOINT=1 does not run with -> one line naming the reason, or None."""
    env = os.environ if env is None else env
    if not getattr(sim.dev, "whole_globe", True):
        return "QD_CHECKPOINT=1 needs a whole-globe handle: the state of latitude bands is not carried"
    if _int(env, "QD_ECO_SPECIATION", 0) == 1 or getattr(sim, "speciation", None) is not None:
        return ("QD_CHECKPOINT=1 does not run with QD_ECO_SPECIATION=1: the draws made ahead and the state of the global generator "
                "are not carried; unset one of the two")
    if getattr(sim, "daily_hook", None) is not None:
        return "QD_CHECKPOINT=1 does not run with a daily_hook: its state is host state this package does not own"
    return None


# ------------------------------------------------------------------------------------- the digest on the host
def _mix64(z):
    with np.errstate(over="ignore"):
        z = z ^ (z >> np.uint64(30))
        z = z * _M1
        z = z ^ (z >> np.uint64(27))
        z = z * _M2
        return z ^ (z >> np.uint64(31))


def host_digest(a):
    """include/qingdai_hip.h: qd_state_digest of a host array (8-, 4- or 1-byte elements) -> int.  Used to check a file before
    anything of it reaches the device; the device's own digest checks the upload."""
    a = np.ascontiguousarray(a)
    w = a.reshape(-1).view({8: np.uint64, 4: np.uint32, 1: np.uint8}[a.dtype.itemsize]).astype(np.uint64)
    with np.errstate(over="ignore"):
        i1 = np.arange(1, w.size + 1, dtype=np.uint64)
        return int(np.sum(_mix64(w + i1 * _GOLD), dtype=np.uint64))


def fnv1a64(name):
    h = 0xCBF29CE484222325
    for b in str(name).encode("utf-8"):
        h = ((h ^ b) * 0x100000001B3) & _MASK
    return h


def run_digest(digests):
    """{plane: D} -> sum_e mix64(D_e ^ fnv1a64(name_e)) mod 2^64."""
    total = 0
    for name, d in digests.items():
        total = (total + int(_mix64(np.uint64(int(d) ^ fnv1a64(name))))) & _MASK
    return total


# ------------------------------------------------------------------------------------- what the run holds
def _eco_f32(sim):
    return bool(sim.eco is not None and int(sim.eco.params.map_f32))


def subsystems(sim):
    """The subsystem set a file must share with the run that loads it, as one string per item.  A keyed lane's item (its key()) is
    there only when the lane is on: a file without it says "off", as every file written before the lane existed does.  The history
    item is older than the keys: it is always there, "-" when the lane is off."""
    pop = sim.eco.pop if sim.eco is not None else None
    items = {"ocean": str(int(sim.ocean is not None)), "routing": str(int(sim.routing is not None)),
             "phyto": str(int(sim.phyto is not None)), "phyto_transport": str(int(bool(getattr(sim, "phyto_transport", False)))),
             "phyto_daily": str(int(sim.phyto_daily is not None)),
             "ecology": str(int(sim.eco is not None)), "population": str(int(pop is not None)), "eco_f32": str(int(_eco_f32(sim))),
             "eco_daily": str(int(sim.eco_daily is not None)), "individuals": str(int(sim.indiv is not None)),
             "indiv_daily": str(int(sim.indiv_daily is not None)),
             "history": ",".join(sim.history.names) if sim.history is not None else "-"}
    for name in ("series", "spectra", "drifters", "flow", "spharm", "eddy", "extremes"):      # (the order the files have held them in)
        lane = getattr(sim, name, None)
        if lane is not None:
            items[name] = lane.key()
    return items


def plane_names(sim):
    """The checkpoint set: every resident plane that a digest covers, as Device.digest names them."""
    names = list(FIELDS) + ["LAND_MASK", "ICE_MASK"]
    if sim.phyto is not None:
        names += [f"PHYTO_TRACER:{s}" for s in range(int(sim.phyto.S))]
    if sim.routing is not None:
        names += ["ROUTE_BUFFER", "ROUTE_FLOW"] + (["ROUTE_LAKES"] if sim.routing.n_lakes > 0 else [])
    if sim.eco_daily is not None:
        names.append("ECO_LAI_STACK")
    if sim.indiv is not None and sim.indiv.n_indiv > 0:
        names += ["INDIV_E_DAY", "INDIV_STRESS"]
    if sim.history is not None:
        names += [f"HISTORY_SUM:{k}" for k in range(len(sim.history.names))]
    spc = getattr(sim, "spectra", None)
    if spc is not None and spc.lat_resolved:
        names.append("SPECTRA_SUMS")
    if getattr(sim, "flow", None) is not None:
        names.append("FLOW_SUMS")
    sph = getattr(sim, "spharm", None)
    if sph is not None and sph.two_d:
        names.append("SPHARM_SUMS")
    if getattr(sim, "eddy", None) is not None:
        names += ["EDDY_SUMS", "EDDY_ANCHORS"]
    ext = getattr(sim, "extremes", None)
    if ext is not None:
        names += ["EXTREMES_VALUES", "EXTREMES_COUNTS"] + (["EXTREMES_HIST"] if ext.hists else [])
    return names


def simulation_digest(sim):
    """{plane: int} for the checkpoint set, taken on the device in one call, plus "run"."""
    names = plane_names(sim)
    d = {n: int(v) for n, v in zip(names, sim.dev.digest(names))}
    d["run"] = run_digest(d)
    return d


def _attr_key(name):
    return "digest_" + name.replace(":", "_")


def _code_hash():
    from ._codehash import fatbin_sha, LIB
    return fatbin_sha(LIB) or "unknown"


def _nan(x):
    return float("nan") if x is None else float(x)


def _none(x):
    return None if np.isnan(x) else float(x)


def collect(sim):
    """Everything of the run, read in one sequence with nothing stepping in between: the digests first, then the planes they cover
    -> (dims, variables, attrs) as ncio.write_nc takes them."""
    dev = sim.dev
    why = span_consistent(sim)
    if why:
        raise CheckpointInconsistent(why)
    dev.flush()
    digests = simulation_digest(sim)
    n_lat, n_lon = dev.shape
    dims = {"lat": n_lat, "lon": n_lon, "three": 3, "five": 5, "two": 2, "scalars": _lib.STATE_SCALARS_N}
    v = {}
    for name in FIELDS:
        dev._host.pop(name, None)
        v["f_" + name] = ("f8", ("lat", "lon"), dev.get(name).copy())
        dev._host.pop(name, None)
    for name in ("LAND_MASK", "ICE_MASK"):
        dev._host.pop(name, None)
        v["m_" + name] = ("u1", ("lat", "lon"), dev.get(name).copy())
        dev._host.pop(name, None)
    a, o = dev.counters()
    i8 = _i8()
    v["atm_counter"], v["ocn_counter"], v["step_index"] = (i8, (), int(a)), (i8, (), int(o)), (i8, (), int(sim._step_index))
    t0, k, dt = sim._t_origin
    v["t_seconds"] = ("f8", (), float(sim.t))
    v["t_origin"] = ("f8", ("three",), np.array([float(t0), float(k), _nan(dt)]))
    mark = getattr(sim, "_span_mark", None) or (sim._step_index, a)        # as recorded behind the last span's bookkeeping
    v["span_mark"] = ("f8", ("two",), np.array([float(mark[0]), float(mark[1])]))       # what a load holds the counters against
    v["diversity_next_day"] = ("f8", (), float(sim.diversity_next_day))
    v["state_scalars"] = ("f8", ("scalars",), dev.state_scalars())
    v["qnet_lw"] = ("f8", ("two",), np.array([float(dev.params.qnet_lw_eps0), float(dev.params.qnet_lw_kc)]))
    ps = dev.params.to_struct()
    raw = np.frombuffer(ctypes.string_at(ctypes.addressof(ps), ctypes.sizeof(ps)), dtype=np.uint8).copy()
    dims["params_bytes"] = int(raw.size)
    v["params_bytes"] = ("u1", ("params_bytes",), raw)
    if sim.phyto is not None:
        dims["phyto_species"] = int(sim.phyto.S)
        v["phyto_C"] = ("f8", ("phyto_species", "lat", "lon"), dev.phyto_download())
        pd = sim.phyto_daily
        v["phyto_clock"] = ("f8", ("two",), np.array([float(pd.phyto_next_time), float(pd.n_steps)] if pd is not None else [0.0, 0.0]))
    if sim.routing is not None:
        r = sim.routing
        v["route_buffer"] = ("f8", ("lat", "lon"), dev.route_download("BUFFER").reshape(dev.shape))
        v["route_flow"] = ("f8", ("lat", "lon"), dev.route_download("FLOW").reshape(dev.shape))
        if r.n_lakes > 0:
            dims["lake"] = int(r.n_lakes)
            v["route_lakes"] = ("f8", ("lake",), dev.route_download("LAKES"))
        v["route_clock"] = ("f8", ("three",), np.array([float(r.t_accum), float(r._steps), 1.0 if r._have_event else 0.0]))
    if sim.history is not None:
        h = sim.history
        sums, count = dev.history_read()
        dims["hist"] = int(sums.shape[0])
        v["hist_sums"] = ("f8", ("hist", "lat", "lon"), sums)
        v["hist_clock"] = ("f8", ("five",), np.array([float(h.i), _nan(h.t_first), _nan(h.t_last), float(h.n_open), float(count)]))
    ser = getattr(sim, "series", None)
    if ser is not None:                                        # (a span boundary: every record of the log has been delivered)
        _save_log_window(dims, v, ser, "series")
    spc = getattr(sim, "spectra", None)
    if spc is not None:
        sums, count = spc.sums()
        _save_log_window(dims, v, spc, "spectra", count)
        if sums is not None:
            dims["spectra_entry"], dims["spectra_k"] = int(sums.shape[0]), int(sums.shape[2])
            v["spectra_sums"] = ("f8", ("spectra_entry", "lat", "spectra_k"), sums)
    flw = getattr(sim, "flow", None)
    if flw is not None:
        sums, count = flw.sums()
        _save_log_window(dims, v, flw, "flow", count)
        dims["flow_plane"] = int(sums.shape[0])
        v["flow_sums"] = ("f8", ("flow_plane", "lat", "lon"), sums)
    sph = getattr(sim, "spharm", None)
    if sph is not None:
        sums, count = sph.sums()
        _save_log_window(dims, v, sph, "spharm", count)
        if sums is not None:
            dims["spharm_entry"], dims["spharm_degree"] = int(sums.shape[0]), int(sums.shape[1])
            v["spharm_sums"] = ("f8", ("spharm_entry", "spharm_degree", "spharm_degree"), sums)
    edd = getattr(sim, "eddy", None)
    if edd is not None:
        anchors, sums, pair_sums, count = dev.eddy_read()
        dims["eddy_field"], dims["eddy_pair"] = int(sums.shape[0]), int(pair_sums.shape[0])
        v["eddy_anchors"] = ("f8", ("eddy_field", "lat", "lon"), anchors)
        v["eddy_sums"] = ("f8", ("eddy_field", "lat", "lon"), sums)
        v["eddy_pair_sums"] = ("f8", ("eddy_pair", "lat", "lon"), pair_sums)
        v["eddy_clock"] = ("f8", ("five",), np.array([float(edd.i), _nan(edd.t_first), _nan(edd.t_last), float(edd.n_open), float(count)]))
    ext = getattr(sim, "extremes", None)
    if ext is not None:
        st = dev.extremes_read()
        hist = np.concatenate([h.reshape(-1) for h in st["hist"]]) if st["hist"] else np.zeros(1, dtype=np.int64)
        dims["extremes_entry"], dims["extremes_threshold"], dims["extremes_hist"] = int(st["vmax"].shape[0]), max(1, int(st["thr"].shape[0])), int(hist.size)
        dims["four"] = 4
        thr = st["thr"].view(np.int32) if st["thr"].shape[0] else np.zeros((1,) + st["thr"].shape[1:], dtype=np.int32)
        v["extremes_values"] = ("f8", ("two", "extremes_entry", "lat", "lon"), np.stack([st["vmax"], st["vmin"]]))
        v["extremes_counts"] = ("i4", ("three", "extremes_entry", "lat", "lon"), np.stack([st["tmax"], st["tmin"], st["nan"]]))
        v["extremes_thresholds"] = ("i4", ("extremes_threshold", "lat", "lon", "four"), thr)
        v["extremes_hist"] = (_i8(), ("extremes_hist",), hist)
        v["extremes_clock"] = ("f8", ("five",), np.array([float(ext.i), _nan(ext.t_first), _nan(ext.t_last), float(ext.n_open), float(st["n"])]))
    dri = getattr(sim, "drifters", None)
    if dri is not None:                                        # the particles as they stand, and the open window's records so far
        _save_log_window(dims, v, dri, "drift")
        for pop, state in dri.state().items():
            if state.shape[1]:
                dims[f"drift_{pop}_rows"], dims[f"drift_{pop}_n"] = int(state.shape[0]), int(state.shape[1])
                v[f"drift_{pop}"] = ("f8", (f"drift_{pop}_rows", f"drift_{pop}_n"), state)
    if sim.eco is not None and sim.eco.pop is not None:
        xd, xv = sim.eco._extension_variables(sim.indiv)
        dims["species"] = int(sim.eco.pop.Ns)
        dims.update(xd)
        v.update(xv)
        if sim.eco_daily is not None:      # drawn at start-up (from OS entropy without QD_ECO_RAND_SEED): the run's identity, not its state
            v["eco_species_modes"] = ("u1", ("species",), np.array([1 if str(m).lower() == "seed" else 0 for m in sim.eco_daily.species_modes], dtype=np.uint8))
    attrs = {"title": "Qingdai exact-resume checkpoint", "creator": "qingdai_amd", "format": "qd-checkpoint-1",
             "abi_version": float(abi_version(dev)), "n_lat": float(n_lat), "n_lon": float(n_lon), "code_hash": _code_hash(),
             "subsystems": ";".join(f"{k}={val}" for k, val in subsystems(sim).items())}
    for name, d in digests.items():
        attrs["run_digest" if name == "run" else _attr_key(name)] = f"0x{d:016x}"
    return dims, v, attrs


def _save_log_window(dims, v, lane, prefix, count=None):
    """A LogWindowLane's open window as <prefix>_records / _times / _steps, padded to one row where it is empty (classic NetCDF
    reads a dimension of size 0 as the unlimited one), and <prefix>_clock {i, records[, count: the sample count of the lane's sums]}."""
    recs, times, steps = lane.window()
    n = int(len(recs))
    pad = max(n, 1)
    t, w = prefix + "_time", prefix + "_width"
    dims[t], dims[w] = pad, max(1, int(lane.width))
    v[prefix + "_records"] = ("f8", (t, w), np.concatenate([recs, np.zeros((pad - n, lane.width))]).reshape(pad, -1))
    v[prefix + "_times"] = ("f8", (t,), np.concatenate([times, np.zeros(pad - n)]))
    v[prefix + "_steps"] = ("f8", (t,), np.concatenate([np.asarray(steps, dtype=np.float64), np.zeros(pad - n)]))
    clock = [float(lane.i), float(n)] + ([] if count is None else [float(count)])
    v[prefix + "_clock"] = ("f8", ("two" if count is None else "three",), np.array(clock))


def _restore_log_window(v, lane, prefix, **sums):
    """The inverse of _save_log_window, through the lane's restore_window (which takes `sums`, where the lane has some)."""
    clock = np.asarray(v[prefix + "_clock"], dtype=np.float64)
    n = int(clock[1])
    lane.restore_window(np.asarray(v[prefix + "_records"], dtype=np.float64)[:n], np.asarray(v[prefix + "_times"])[:n],
                        np.asarray(v[prefix + "_steps"])[:n], int(clock[0]), **sums)


def write_atomic(path, dims, variables, attrs):
    """ncio.write_nc to a temporary name beside `path`, then os.replace: a failure in the middle leaves the old file."""
    path = str(path)
    d, base = os.path.split(os.path.abspath(path))
    tmp = os.path.join(d, f".{base}.{os.getpid()}.part")         # two runs that share a data directory do not share the name
    try:
        ncio.write_nc(tmp, dims, variables, attrs)
        _fsync(tmp)                                            # the data before the name: a crash leaves the old file or the new
        os.replace(tmp, path)
        _fsync(d)
    finally:
        if os.path.exists(tmp):
            os.remove(tmp)


def _fsync(path):
    try:
        fd = os.open(path, os.O_RDONLY)
    except OSError:
        return
    try:
        os.fsync(fd)
    except OSError:
        pass                                                   # (a file system that cannot sync a directory)
    finally:
        os.close(fd)


def save(sim, path, reason=None, out=print):
    """Write the checkpoint -> the run digest.  One [Checkpoint] line when `reason` is given."""
    dims, v, attrs = collect(sim)
    write_atomic(path, dims, v, attrs)
    run = int(attrs["run_digest"], 16)
    if reason is not None:
        out(f"[Checkpoint] ({reason}) wrote '{path}' at t={sim.t:.1f} s, step {sim._step_index}, run digest 0x{run:016x}")
    return run


# ------------------------------------------------------------------------------------- reading and checking a file
class CheckpointFile:
    def __init__(self, path, variables, attrs):
        self.path, self.v, self.attrs = str(path), variables, attrs
        self.verified = False

    def plane(self, name):
        """The host array whose stored bits the digest of `name` covers, in the element size the device keeps it in."""
        v = self.v
        base, _, idx = name.partition(":")
        if name in ("LAND_MASK", "ICE_MASK"):
            return np.asarray(v["m_" + name]).astype(np.uint8)
        if name in FIELDS:
            a = np.asarray(v["f_" + name], dtype=np.float64)
            return a.astype(np.float32) if (self.subsystems().get("eco_f32") == "1" and name in F32_MAPS) else a
        if name in ("EDDY_SUMS", "EDDY_ANCHORS"):                  # the device keeps each plane at an even stride: a cell of +0.0 behind an odd one
            keys = ("eddy_sums", "eddy_pair_sums") if name == "EDDY_SUMS" else ("eddy_anchors",)
            planes = np.concatenate([np.asarray(v[k], dtype=np.float64).reshape(np.shape(v[k])[0], -1) for k in keys])
            return np.pad(planes, ((0, 0), (0, planes.shape[1] & 1)))
        if name == "EXTREMES_VALUES":
            return np.asarray(v["extremes_values"], dtype=np.float64)
        if name == "EXTREMES_COUNTS":                              # every 4-byte plane as one: the thresholds (as far as there are any), then the counts
            n_thr = len([t for t in self.subsystems().get("extremes", "||").split("|")[1].split(",") if t])
            thr = np.asarray(v["extremes_thresholds"]).astype(np.int32)[:n_thr]
            return np.concatenate([thr.reshape(-1), np.asarray(v["extremes_counts"]).astype(np.int32).reshape(-1)])
        if name == "EXTREMES_HIST":
            return np.asarray(v["extremes_hist"]).astype(np.int64)
        key = {"PHYTO_TRACER": "phyto_C", "HISTORY_SUM": "hist_sums"}.get(base)
        if key is not None:
            return np.asarray(v[key], dtype=np.float64)[int(idx)]
        key = {"ROUTE_BUFFER": "route_buffer", "ROUTE_FLOW": "route_flow", "ROUTE_LAKES": "route_lakes", "ECO_LAI_STACK": "qd_LAI_layers_SK",
               "INDIV_E_DAY": "qd_indiv_E_day", "INDIV_STRESS": "qd_indiv_stress_days", "SPECTRA_SUMS": "spectra_sums",
               "FLOW_SUMS": "flow_sums", "SPHARM_SUMS": "spharm_sums"}[name]
        return np.asarray(v[key], dtype=np.float64)

    def subsystems(self):
        return dict(item.split("=", 1) for item in str(self.attrs.get("subsystems", "")).split(";") if "=" in item)

    def digests(self):
        """{plane name: int} as stored (the attribute keys hold '_' for ':')."""
        return {k[len("digest_"):]: int(str(val), 16) for k, val in self.attrs.items() if k.startswith("digest_")}

    def scalar(self, name):
        return float(np.asarray(self.v[name]).reshape(-1)[0])


def read(path):
    if not os.path.exists(path):
        raise CheckpointRefused("the file does not exist")
    try:
        v, attrs = ncio.read_nc(str(path))
    except Exception as e:      # noqa: BLE001
        raise CheckpointRefused(f"the file cannot be read ({e})") from None
    if attrs.get("format") != "qd-checkpoint-1":
        raise CheckpointRefused("the file is not a checkpoint of this package (no format = qd-checkpoint-1)")
    return CheckpointFile(path, v, attrs)


def check_grid_and_abi(f, shape, dev=None):
    got = (int(float(f.attrs.get("n_lat", -1))), int(float(f.attrs.get("n_lon", -1))))
    if got != tuple(int(x) for x in shape):
        raise CheckpointRefused(f"the grid shape differs: the file holds {got[0]}x{got[1]}, the run is {shape[0]}x{shape[1]}")
    abi = int(float(f.attrs.get("abi_version", -1)))
    if abi != abi_version(dev):
        raise CheckpointRefused(f"the ABI version differs: the file was written by version {abi}, this build is version {abi_version(dev)}")
    if "span_mark" in f.v:
        mark = np.asarray(f.v["span_mark"], dtype=np.float64).reshape(-1)
        if int(mark[0]) != int(f.scalar("step_index")) or int(mark[1]) != int(f.scalar("atm_counter")):
            raise CheckpointRefused(f"the file was not written at a span boundary: step index {int(f.scalar('step_index'))} and device counter "
                                    f"{int(f.scalar('atm_counter'))} against {int(mark[0])} and {int(mark[1])} at the last span's end")
    else:
        raise CheckpointRefused("the file holds no span mark")


def check_subsystems(f, sim):
    want, got = subsystems(sim), f.subsystems()
    onoff = lambda s: {"0": "off", "1": "on"}.get(s, f"'{s}'")
    for name in KEYED_LANES:
        if got.get(name, "-") != want.get(name, "-"):
            raise CheckpointRefused(f"the subsystem set differs: the {name} lane is '{got.get(name, '-')}' in the file and "
                                    f"'{want.get(name, '-')}' in this run")
    for k in want:
        if got.get(k) != want[k]:
            if k == "history":
                raise CheckpointRefused(f"the subsystem set differs: the history fields are '{got.get(k, '-')}' in the file and '{want[k]}' in this run")
            raise CheckpointRefused(f"the subsystem set differs: {k} is {onoff(got.get(k, '0'))} in the file and {onoff(want[k])} in this run")


def verify_file(f):
    """Every stored digest against the host digest of the plane as the file holds it: a changed byte, a truncated variable."""
    stored = f.digests()
    if not stored or "run_digest" not in f.attrs:
        raise CheckpointRefused("the file holds no digests")
    by_key = {}
    for name in _file_plane_names(f):
        key = name.replace(":", "_")
        if key not in stored:
            raise CheckpointRefused(f"the file holds no digest of {name}")
        try:
            d = host_digest(f.plane(name))
        except Exception as e:      # noqa: BLE001
            raise CheckpointRefused(f"plane {name} cannot be read from the file ({e})") from None
        if d != stored[key]:
            raise CheckpointRefused(f"the digest of {name} does not match: the file's plane gives 0x{d:016x}, the file says 0x{stored[key]:016x}")
        by_key[name] = d
    if len(by_key) != len(stored):
        raise CheckpointRefused("the file holds digests of planes it does not hold")
    run = run_digest(by_key)
    if run != int(str(f.attrs["run_digest"]), 16):
        raise CheckpointRefused(f"the run digest does not match: the planes give 0x{run:016x}, the file says {f.attrs['run_digest']}")
    f.verified = True
    return run


def _file_plane_names(f):
    v = f.v
    names = [n for n in FIELDS if "f_" + n in v] + [n for n in ("LAND_MASK", "ICE_MASK") if "m_" + n in v]
    if "phyto_C" in v:
        names += [f"PHYTO_TRACER:{s}" for s in range(np.shape(v["phyto_C"])[0])]
    names += [n for n, k in (("ROUTE_BUFFER", "route_buffer"), ("ROUTE_FLOW", "route_flow"), ("ROUTE_LAKES", "route_lakes")) if k in v]
    if "qd_LAI_layers_SK" in v and f.subsystems().get("eco_daily") == "1":
        names.append("ECO_LAI_STACK")
    names += [n for n, k in (("INDIV_E_DAY", "qd_indiv_E_day"), ("INDIV_STRESS", "qd_indiv_stress_days")) if k in v]
    if "hist_sums" in v:
        names += [f"HISTORY_SUM:{k}" for k in range(np.shape(v["hist_sums"])[0])]
    if "spectra_sums" in v:
        names.append("SPECTRA_SUMS")
    if "flow_sums" in v:
        names.append("FLOW_SUMS")
    if "spharm_sums" in v:
        names.append("SPHARM_SUMS")
    if "eddy_sums" in v:
        names += ["EDDY_SUMS", "EDDY_ANCHORS"]
    if "extremes_values" in v:
        names += ["EXTREMES_VALUES", "EXTREMES_COUNTS"] + (["EXTREMES_HIST"] if "digest_EXTREMES_HIST" in f.attrs else [])
    return names


def param_differences(f, params):
    """Field names of qd_params whose saved bytes differ from the run's (NaN compares by bits, like everything here)."""
    from .params import qd_params
    raw = np.asarray(f.v["params_bytes"]).astype(np.uint8).tobytes()
    if len(raw) != ctypes.sizeof(qd_params):
        return ["<the struct size>"]
    saved, now = qd_params.from_buffer_copy(raw), params.to_struct()
    out = []
    for name, ctype in qd_params._fields_:
        a, b = ctype(getattr(saved, name)), ctype(getattr(now, name))
        if bytes(a) != bytes(b):
            out.append(name)
    return out


# ------------------------------------------------------------------------------------- load
def load(sim, path, env=None, out=print):
    """Put a checkpoint back into a freshly built Simulation that has the file's subsystems enabled.  Every refusal is raised
    before anything of the run is touched (CheckpointRefused); the device then digests every plane again and a difference from the
    stored digests is an error (RuntimeError: the state is then neither the file's nor a fresh one).  -> the run digest."""
    env = os.environ if env is None else env
    f = path if isinstance(path, CheckpointFile) else read(path)
    dev = sim.dev
    why = startup_refusal(sim, env)
    if why:
        raise CheckpointRefused(why)
    check_grid_and_abi(f, dev.shape, dev)
    check_subsystems(f, sim)
    if not f.verified:
        verify_file(f)
    if not np.array_equal(f.plane("LAND_MASK"), np.asarray(sim.land_mask).astype(np.uint8)):
        raise CheckpointRefused("the land mask differs from the run's topography")
    if sim.phyto is not None and np.shape(f.v["phyto_C"])[0] != int(sim.phyto.S):
        raise CheckpointRefused(f"the subsystem set differs: the file holds {np.shape(f.v['phyto_C'])[0]} tracer species, the run {int(sim.phyto.S)}")
    if sim.routing is not None and int(np.size(f.v.get("route_lakes", ()))) != int(sim.routing.n_lakes):
        raise CheckpointRefused("the subsystem set differs: the routing network of the file has another lake count")
    diff = param_differences(f, dev.params)
    autotune = _int(env, "QD_ENERGY_AUTOTUNE", 0) == 1
    if autotune:
        diff = [n for n in diff if n not in ("qnet_lw_eps0", "qnet_lw_kc")]
    if diff:
        out("[Checkpoint] note: parameters differ from the saved run: " + ", ".join(diff))
    v = f.v
    # 1. the ecology's own exact-resume variables, through the ecology's own code (it configures the daily lane again)
    pop = sim.eco.pop if sim.eco is not None else None
    own_modes = list(sim.eco_daily.species_modes) if sim.eco_daily is not None else None
    if own_modes is not None and "eco_species_modes" in v and np.size(v["eco_species_modes"]) == len(own_modes):
        # the spread modes the saved run drew at its start-up; the lane is configured with them by the restore below
        sim.eco_daily.species_modes = ["seed" if int(m) else "diffusion" for m in np.asarray(v["eco_species_modes"]).reshape(-1)]
    if pop is not None and not sim.eco._restore_extended(v, sim.indiv):      # checks every shape first and touches nothing when one misfits
        if own_modes is not None:
            sim.eco_daily.species_modes = own_modes
        raise CheckpointRefused("the ecology variables of the file do not fit this run (species, layers or individuals differ)")
    # 2. the planes.  LAND_MASK is the run's own (checked above); an elevation map only where the run has one (an upload marks it present)
    dev._host.clear()
    for name in FIELDS:
        if name == "ELEVATION" and sim.elevation is None:
            continue
        dev.upload_now(name, np.asarray(v["f_" + name], dtype=np.float64))
    dev.upload_now("ICE_MASK", f.plane("ICE_MASK"))
    if sim.phyto is not None:
        dev.phyto_upload(np.asarray(v["phyto_C"], dtype=np.float64))
        if sim.phyto_daily is not None:
            sim.phyto_daily.phyto_next_time, sim.phyto_daily.n_steps = float(v["phyto_clock"][0]), int(v["phyto_clock"][1])
    if sim.routing is not None:
        r, clock = sim.routing, np.asarray(v["route_clock"], dtype=np.float64)
        dev.route_restore(v["route_buffer"], v["route_flow"], v.get("route_lakes"), int(clock[1]))
        r.t_accum, r._steps, r._have_event, r._last = float(clock[0]), int(clock[1]), bool(clock[2]), None
    if sim.history is not None:
        h, clock = sim.history, np.asarray(v["hist_clock"], dtype=np.float64)
        dev.history_restore(np.asarray(v["hist_sums"], dtype=np.float64), int(clock[4]))
        h.i, h.t_first, h.t_last, h.n_open = int(clock[0]), _none(clock[1]), _none(clock[2]), int(clock[3])
    if getattr(sim, "series", None) is not None:
        _restore_log_window(v, sim.series, "series")
        dev.series_reset()
    if getattr(sim, "spectra", None) is not None:
        _restore_log_window(v, sim.spectra, "spectra", sums=np.asarray(v["spectra_sums"], dtype=np.float64) if "spectra_sums" in v else None,
                            count=int(v["spectra_clock"][2]))
    if getattr(sim, "flow", None) is not None:
        _restore_log_window(v, sim.flow, "flow", sums=np.asarray(v["flow_sums"], dtype=np.float64), count=int(v["flow_clock"][2]))
    if getattr(sim, "spharm", None) is not None:
        _restore_log_window(v, sim.spharm, "spharm", sums=np.asarray(v["spharm_sums"], dtype=np.float64) if "spharm_sums" in v else None,
                            count=int(v["spharm_clock"][2]))
    if getattr(sim, "eddy", None) is not None:
        e, clock = sim.eddy, np.asarray(v["eddy_clock"], dtype=np.float64)
        dev.eddy_restore(np.asarray(v["eddy_anchors"], dtype=np.float64), np.asarray(v["eddy_sums"], dtype=np.float64),
                         np.asarray(v["eddy_pair_sums"], dtype=np.float64), int(clock[4]))
        e.i, e.t_first, e.t_last, e.n_open = int(clock[0]), _none(clock[1]), _none(clock[2]), int(clock[3])
    if getattr(sim, "extremes", None) is not None:
        x, clock = sim.extremes, np.asarray(v["extremes_clock"], dtype=np.float64)
        values, counts = np.asarray(v["extremes_values"], dtype=np.float64), np.asarray(v["extremes_counts"]).astype(np.int32)
        thr = np.ascontiguousarray(np.asarray(v["extremes_thresholds"]).astype(np.int32)[:len(x.thresholds)]).view(np.uint32)
        flat, tables, o = np.asarray(v["extremes_hist"]).astype(np.int64), [], 0
        for _, edges in x.hists:
            w = edges.size - 1 + 3
            tables.append(flat[o:o + values.shape[2] * w].reshape(values.shape[2], w))
            o += values.shape[2] * w
        dev.extremes_restore({"vmax": values[0], "vmin": values[1], "tmax": counts[0], "tmin": counts[1], "nan": counts[2],
                              "thr": thr, "hist": tables, "n": int(clock[4])})
        x.i, x.t_first, x.t_last, x.n_open = int(clock[0]), _none(clock[1]), _none(clock[2]), int(clock[3])
    dri = getattr(sim, "drifters", None)
    if dri is not None:
        _restore_log_window(v, dri, "drift")
        dri.restore_state(np.asarray(v["drift_atm"], dtype=np.float64) if "drift_atm" in v else np.empty((3, 0)),
                          np.asarray(v["drift_ocn"], dtype=np.float64) if "drift_ocn" in v else np.empty((4, 0)))
        dev.drift_reset()
    # 3. counters, parameters, the host-side scalars (last: the uploads above set some of the flags they carry)
    dev.set_counters(int(f.scalar("atm_counter")), int(f.scalar("ocn_counter")))
    if autotune:
        dev.params.qnet_lw_eps0, dev.params.qnet_lw_kc = float(v["qnet_lw"][0]), float(v["qnet_lw"][1])
        dev.push_params()
    dev.set_state_scalars(np.asarray(v["state_scalars"], dtype=np.float64))
    if pop is not None:                                        # the firing counts moved: the host copies are current as of now
        if sim.eco_daily is not None:
            sim.eco_daily.n_firings = int(np.asarray(v["state_scalars"])[_lib.STATE_SCALAR_SLOT["eco_daily_fired"]])
        pop.LAI_layers_SK = pop._layers
        pop.species_weights = pop._weights
    # 4. the host clocks
    t0, k, dt = (float(x) for x in np.asarray(v["t_origin"], dtype=np.float64))
    sim.t = f.scalar("t_seconds")
    sim._t_origin = (t0, int(k), _none(dt))
    sim._step_index = sim._index_base = int(f.scalar("step_index"))      # the plot clock and the budget cadence count on from here
    if getattr(sim, "budget", None) is not None:
        sim.budget.i = sim._step_index
    sim._span_mark = (sim._step_index, int(f.scalar("atm_counter")))
    sim.diversity_next_day = f.scalar("diversity_next_day")
    # 5. what the device now holds against what the file says
    stored = f.digests()
    now = simulation_digest(sim)
    for name, d in now.items():
        if name != "run" and d != stored.get(name.replace(":", "_")):
            raise RuntimeError(f"[Checkpoint] after the upload the device digest of {name} is 0x{d:016x}, the file says "
                               f"0x{stored.get(name.replace(':', '_'), 0):016x}: the state is not the saved run's")
    out(f"[Checkpoint] loaded '{f.path}' at t={sim.t:.1f} s, step {sim._step_index}, run digest 0x{now['run']:016x}")
    return now["run"]
