"""
qingdai_amd/device.py -- one resident device context (qd_handle) per grid.

The reference keeps atmosphere and ocean state in two Python objects that exchange
NumPy arrays every step (run_simulation.py:2194-2253).  Here both live in one device
context so the coupling never leaves HBM; `SpectralModel` and `WindDrivenSlabOcean`
are views onto it.  Attribute reads download, attribute writes upload lazily
(DoubleBufferingArray contract, numerics/double_buffer.py:47-184).
"""
from __future__ import annotations

import ctypes

import numpy as np

from . import _lib
from ._lib import F, OUT, QdError
from .params import QdParams


def _c(a, dtype=np.float64):
    return np.ascontiguousarray(a, dtype=dtype)


class Device:
    _history_n = 0            # entries of the last history_configure
    _series_width = 0         # doubles per record of the last series_configure
    _spectra_n = 0            # entries of the last spectra_configure
    _spectra_lat = False      # ... and whether it keeps the lat-resolved sum planes
    _spharm_n = _spharm_N = 0 # entries and truncation of the last spharm_configure
    _spharm_2d = False        # ... and whether it keeps the 2D sum planes
    _eddy = (0, 0)            # fields and pairs of the last eddy_configure
    _extremes = (0, 0, ())    # entries, thresholds and the bin counts of the histograms of the last extremes_configure
    _drift = (0, 0, 0, 0)     # n_atm, n_ocn, record width and log capacity of the last drift_configure
    _tiles_n = 1              # tiles of the last tile configuration
    _div_shape = None         # [S, lat, lon] of the last eco_diversity call

    def __init__(self, grid, params: QdParams | None = None, device=0, row0=0, n_rows=None, halo=0, rank=0, world=1):
        self.lib = _lib.load()
        self.grid = grid
        self.params = params or QdParams.from_env()
        self.shape = (grid.n_lat, grid.n_lon)
        n_rows = grid.n_lat if n_rows is None else n_rows
        self.whole_globe = row0 == 0 and n_rows == grid.n_lat and halo == 0 and world == 1     # not a latitude band
        desc = _lib.qd_grid_desc(grid.n_lat, grid.n_lon, row0, n_rows, halo, device, rank, world)
        h = ctypes.c_void_p()
        ps = self.params.to_struct()
        rc = self.lib.qd_create(ctypes.byref(desc), ctypes.byref(ps), float(self.params.q_init_rh), ctypes.byref(h))
        if rc != 0:
            raise QdError("qd_create failed: " + (self.lib.qd_last_error(None) or b"?").decode())
        self.h = h
        self._host = {}           # field -> ndarray handed to the caller (may have been mutated)
        grid._device = self

    # ---- the call seam: every symbol goes through _lib.call, marshalled by its declaration in include/qingdai_hip.h
    def call(self, symbol, *args, error=QdError, what=None):
        """symbol(self.h, *args), checked -> the values of its OUT arguments (_lib.call)."""
        return _lib.call(self.lib, symbol, (self.h,) + args, last_error=lambda: self.lib.qd_last_error(self.h), error=error, what=what)

    def _chk(self, rc, what):
        """For callers that reach self.lib themselves (tests, the benchmark)."""
        if rc != 0:
            raise QdError(f"{what} failed: " + (self.lib.qd_last_error(self.h) or b"?").decode())

    def close(self):
        if getattr(self, "h", None):
            self.lib.qd_destroy(self.h)
            self.h = None

    def __del__(self):
        try:
            self.close()
        except Exception:
            pass

    # ---- parameters
    def push_params(self):
        ps = self.params.to_struct()
        self.call("qd_set_params", ps, ctypes.sizeof(ps))

    # ---- attribute surface
    def get(self, name):
        """Download (or return the cached host copy of) a field."""
        if name in self._host:
            return self._host[name]
        out = np.empty(self.shape, dtype=np.uint8 if name in ("LAND_MASK", "ICE_MASK") else np.float64)
        self.call("qd_download", F[name], out, out.nbytes, what=f"qd_download({name})")
        self._host[name] = out
        return out

    def set(self, name, arr):
        if name in ("LAND_MASK", "ICE_MASK"):
            a = _c(arr, np.uint8)
        else:
            a = _c(np.broadcast_to(np.asarray(arr, dtype=np.float64), self.shape))
            if not a.flags.writeable:
                a = a.copy()
        if a.shape != self.shape:
            raise ValueError(f"{name}: expected shape {self.shape}, got {a.shape}")
        self._host[name] = a

    def flush(self):
        """Send every host-side copy that may differ from the device (anything written, or
        read and possibly mutated in place) before device work starts."""
        for name in list(self._host):
            a = self._host[name]
            self.call("qd_upload", F[name], a, a.nbytes, what=f"qd_upload({name})")
        self._host.clear()

    def upload_now(self, name, arr):
        self.set(name, arr)
        a = self._host.pop(name)
        self.call("qd_upload", F[name], a, a.nbytes, what=f"qd_upload({name})")

    # ---- the path
    def forcing(self, star_a, star_b, theta, with_teq=True):
        self.flush()
        self.call("qd_forcing", _c(star_a).reshape(3), _c(star_b).reshape(3), theta, bool(with_teq))

    def simple_albedo(self, ocean_albedo=0.08):
        self.flush()
        self.call("qd_simple_albedo", ocean_albedo)

    def atmos_step(self, dt, has_albedo):
        self.flush()
        self.call("qd_atmos_step", dt, bool(has_albedo))

    def ocean_step(self, dt, compute_qnet, use_ice_mask, inject_sst):
        self.flush()
        self.call("qd_ocean_step", dt, compute_qnet, use_ice_mask, inject_sst)

    def driver_physics(self, dt):
        self.flush()
        self.call("qd_driver_physics", dt)

    def hydrology_commit(self, dt):
        self.flush()
        self.call("qd_hydrology_commit", dt)

    def step_n(self, stars, dt, with_ocean=False, with_physics=False, pass_albedo=True, with_hydrology=False, energy_diag=False,
               ecology=False, phyto=False, routing=None, phyto_daily=None, t0=None, eco_daily=None, budget=None, history=None,
               series=None, spectra=None, drifters=None, flow=None, spharm=None, eddy=None, extremes=None):
        """benchmark_jax.py:124-158 as one resident loop (qd_step_n).  `stars`: [n][7] host
        scalars from ThermalForcing.star_table().  The span lanes, each a participant on this handle whose records stay in its
        device log until the caller has it deliver them: `routing`, a RiverRouting -- bit7, after the hydrology commit (which it
        needs); its t_accum names the event steps.  `phyto_daily`, a phyto.PhytoDaily -- bit8; its firing clock turns the span's
        times (t0 + dt * arange(n), or t0 itself when it is the n times) into the schedule.  `eco_daily`, an
        ecology.PopulationDaily -- bit9 (needs `ecology`); its day accumulator names the firing steps.  `budget`, a
        budget_diag.BudgetDiag -- no flag bit: its schedule (run-local step index, the ocean's step count) turns the lane on for
        the span.  `history`, a history.History -- no flag bit either: its window clock names the sampled steps, whose fields are
        added to the resident sums (history_read).  `series`, a series.Series -- no flag bit: its window clock names the sampled
        steps, each of which leaves one record of reduced fields in the lane's log (series_log).  `spectra`, a spectra.Spectra -- no flag bit:
        likewise, one record of zonal wavenumber spectra per sampled step (spectra_log).  `drifters`, a drifters.Drifters -- no flag bit, and the
        one lane whose state moves: every step of the span advances the particles, its window clock names the steps that also leave a
        record (drift_log).  `flow`, a flow.Flow -- no flag bit: one record of flow kinematics per sampled step (flow_log), and the
        sampled psi, chi, zeta, delta in resident sum planes (flow_sums).  `spharm`, a spharm.Spharm -- no flag bit: one record of
        spherical-harmonic power spectra per sampled step (spharm_log), the 2D terms in resident sum planes (spharm_sums).  `eddy`, an
        eddy.Eddy -- no flag bit and no log: a sampled step adds the fields' deviations from their anchors and the products of
        pairs of them to resident planes (eddy_read).  `extremes`, an extremes.Extremes -- no flag bit and no log: a sampled step
        updates per-cell extremes, threshold counts and spells, and per-row histograms in resident planes (extremes_read)."""
        self.flush()
        st = _c(stars)
        assert st.ndim == 2 and st.shape[1] == 7
        n = int(st.shape[0])
        # The span's participants (csrc/qd_span.h), one protocol for all of them:
        #   dev                       the handle the lane is configured on
        #   span_clock()              -> the host clock as it stands before the span
        #   span_schedule(t0, dt, n)  advance that clock over the n steps, upload their schedule -> what _fired is to be told
        #   span_restore(clock)       nothing ran (an upload or qd_step_n raised): the clock back to what span_clock gave
        #   _fired(k)                 the span ran: k is what span_schedule returned
        #   span_deliver(dt)          drain the lane's device log and deliver it (print, keep); the caller's move, once per span
        lanes = [p for p in (phyto_daily, routing, eco_daily, budget, history, series, spectra, drifters, flow, spharm, eddy, extremes) if p is not None]
        for p in lanes:
            if p.dev is not self:
                raise ValueError(f"step_n: the {type(p).__name__} runs on another device handle")
        if phyto_daily is not None and t0 is None:
            raise ValueError("step_n: phyto_daily needs the span's start time t0")
        flags = _lib.step_flags(with_ocean=with_ocean, with_physics=with_physics, pass_albedo=pass_albedo, with_hydrology=with_hydrology,
                                energy_diag=energy_diag, ecology=ecology, phyto=phyto, routing=routing is not None, phyto_daily=phyto_daily is not None,
                                eco_daily=eco_daily is not None)
        clocks = [p.span_clock() for p in lanes]
        try:
            fired = [p.span_schedule(t0, float(dt), n) for p in lanes]      # each uploads its schedule for this span
            self.call("qd_step_n", n, dt, flags, st)
        except Exception:
            for p, clock in zip(lanes, clocks):                               # nothing ran: every host clock back to before the call
                p.span_restore(clock)
            raise
        for p, k in zip(lanes, fired):
            p._fired(k)

    def sync(self):
        self.call("qd_sync")

    # ---- river routing (qd_route.hip): plan upload, class seam, results
    ROUTE_WHICH = {"FLOW": 0, "LAKES": 1, "BUFFER": 2}

    def route_configure(self, plan):
        """Upload a routing.RoutingPlan (whole-globe handles only)."""
        keep = [np.ascontiguousarray(a) for a in (plan.cflags, plan.area_row, plan.code, plan.seg_start, plan.seg_cells,
                                                  plan.level_start, plan.jp_start, plan.jp_cells, plan.lake_start,
                                                  plan.lake_cells, plan.lake_frac)]
        ptr = [a.ctypes.data for a in keep]
        ps = _lib.qd_route_plan(plan.n_lat * plan.n_lon, len(plan.seg_start) - 1, len(plan.seg_cells), plan.n_levels,
                                len(plan.jp_cells), plan.n_lakes, plan.pe_lakes, 0, *ptr)
        self.call("qd_route_configure", ps, ctypes.sizeof(ps))
        self._route_n = (plan.n_lat * plan.n_lon, plan.n_lakes)
        self._route_last = None

    def route_free(self):
        self.call("qd_route_free")

    def route_reset(self):
        self.call("qd_route_reset")
        self._route_last = None

    def route_accumulate(self, dt):
        self.flush()
        self.call("qd_route_accumulate", dt)

    def route_event(self, event_dt, with_pe):
        self.flush()
        self.call("qd_route_event", event_dt, bool(with_pe))

    def route_download(self, which):
        out = np.zeros(self._route_n[1] if which == "LAKES" else self._route_n[0], dtype=np.float64)
        self.call("qd_route_download", self.ROUTE_WHICH[which], out, out.size)
        return out

    def route_schedule(self, event_dt):
        self.call("qd_route_schedule", np.size(event_dt), event_dt)

    @staticmethod
    def _records(drained, width):
        """What a span lane's drain (csrc/qd_span.h) handed back, (buffer, n) -> [n][width] records, oldest first; the device log
        is empty afterwards."""
        buf, n = drained
        return buf.reshape(-1, width)[:n].copy()

    def route_events(self):
        """Drain the device event log -> list of dicts (routing.LOG_KEYS), oldest first."""
        from .routing import LOG_KEYS
        rows = self._records(self.call("qd_route_events", OUT(_lib.SPAN_LOG_CAP * _lib.ROUTE_LOG_W), _lib.SPAN_LOG_CAP, OUT), _lib.ROUTE_LOG_W)
        out = [dict(zip(LOG_KEYS, (float(x) for x in row))) for row in rows]
        if out:
            self._route_last = out[-1]
        return out

    def route_last_event(self):
        return self._route_last

    # ---- periodic budget diagnostics (qd_budget_diag.hip)
    def budget_diag_configure(self, lines, polar_row):
        if np.size(polar_row) != self.shape[0]:
            raise ValueError("budget_diag_configure: polar_row holds one flag per latitude row")
        self.call("qd_budget_diag_configure", lines, polar_row)

    def budget_diag_schedule(self, fire):
        self.call("qd_budget_diag_schedule", np.size(fire), fire)

    def budget_diag_log(self):
        """Drain the records -> [n][BUDGET_LOG_W] (budget_diag.REC names the slots), oldest first."""
        return self._records(self.call("qd_budget_diag_log", OUT(_lib.SPAN_LOG_CAP * _lib.BUDGET_LOG_W), _lib.SPAN_LOG_CAP, OUT), _lib.BUDGET_LOG_W)

    def budget_diag_reset(self):
        self.call("qd_budget_diag_reset")

    # ---- time-mean history accumulators (qd_history.hip)
    def history_configure(self, entries):
        """entries: [(op, a, b)] with a, b field names as `get` takes them (b None for op 0): op 0 = the plane a,
        1 = sqrt(a*a + b*b).  An empty list releases the accumulators."""
        self.call("qd_history_configure", len(entries), [e[0] for e in entries], [F[e[1]] for e in entries],
                  [F[e[2]] if e[2] is not None else -1 for e in entries])
        self._history_n = len(entries)

    def history_schedule(self, sample):
        self.call("qd_history_schedule", np.size(sample), sample)

    def history_sample(self):
        """One sample of every entry from the fields as they stand (the class seam)."""
        self.flush()
        self.call("qd_history_sample")

    def history_read(self):
        """-> (sums [n][n_lat][n_lon], sample count)"""
        out = np.empty((self._history_n,) + self.shape, dtype=np.float64)
        return out, self.call("qd_history_read", out, OUT)

    def history_reset(self):
        self.call("qd_history_reset")

    # ---- extremes, spells and distributions (qd_extremes.hip)
    def extremes_configure(self, entries, thresholds=(), hists=()):
        """entries: [(op, a, b)] as history_configure takes them; thresholds: [(entry index, '<' or '>', value)]; hists: [(entry
        index, edges)], nb + 1 strictly increasing finite edges each.  An empty entry list releases the lane."""
        if not len(entries):
            self.call("qd_extremes_configure", 0, None, None, None, 0, None, None, None, 0, None, None, None)
            self._extremes = (0, 0, ())
            return
        cmp = [ord(c) if isinstance(c, str) and len(c) == 1 else int(c) for _, c, _ in thresholds]
        edges = [np.asarray(e, dtype=np.float64).reshape(-1) for _, e in hists]
        self.call("qd_extremes_configure", len(entries), [e[0] for e in entries], [F[e[1]] for e in entries],
                  [F[e[2]] if e[2] is not None else -1 for e in entries],
                  len(thresholds), [int(t[0]) for t in thresholds] or None, cmp or None, [float(t[2]) for t in thresholds] or None,
                  len(hists), [int(h[0]) for h in hists] or None, [e.size - 1 for e in edges] or None,
                  np.concatenate(edges) if edges else None)
        self._extremes = (len(entries), len(thresholds), tuple(e.size - 1 for e in edges))

    def extremes_schedule(self, sample):
        self.call("qd_extremes_schedule", np.size(sample), sample)

    def extremes_sample(self):
        """One sample of every entry from the fields as they stand (the class seam); k is the lane's own count."""
        self.flush()
        self.call("qd_extremes_sample")

    def extremes_read(self):
        """-> the lane's state as extremes.accumulate_reference returns it: {vmax, vmin [E][n_lat][n_lon] f64; tmax, tmin, nan
        [E][n_lat][n_lon] i32; thr [T][n_lat][n_lon][4] u32 (count, run, longest, spells); hist: a list of [n_lat][nb + 3] i64;
        n: the sample count}"""
        ne, nt, nbs = self._extremes
        nlat = self.shape[0]
        values = np.empty((2, ne) + self.shape, dtype=np.float64)
        counts = np.empty((3, ne) + self.shape, dtype=np.int32)
        thr = np.empty((nt,) + self.shape + (4,), dtype=np.int32)
        hist = np.empty(sum(nlat * (nb + 3) for nb in nbs), dtype=np.int64)
        n = self.call("qd_extremes_read", values, counts, thr if nt else None, hist if nbs else None, OUT)
        tables, o = [], 0
        for nb in nbs:
            tables.append(hist[o:o + nlat * (nb + 3)].reshape(nlat, nb + 3).copy())
            o += nlat * (nb + 3)
        return {"vmax": values[0], "vmin": values[1], "tmax": counts[0], "tmin": counts[1], "nan": counts[2],
                "thr": thr.view(np.uint32), "hist": tables, "n": int(n)}

    def extremes_restore(self, state):
        """The inverse of extremes_read, for an exact resume."""
        ne, nt, nbs = self._extremes
        nlat = self.shape[0]
        for name in ("vmax", "vmin", "tmax", "tmin", "nan"):
            if np.shape(state[name]) != (ne,) + self.shape:
                raise ValueError(f"extremes_restore: expected {name} of shape {(ne,) + self.shape}, got {np.shape(state[name])}")
        if np.shape(state["thr"]) != (nt,) + self.shape + (4,):
            raise ValueError(f"extremes_restore: expected thr of shape {(nt,) + self.shape + (4,)}, got {np.shape(state['thr'])}")
        if [np.shape(h) for h in state["hist"]] != [(nlat, nb + 3) for nb in nbs]:
            raise ValueError("extremes_restore: the histogram tables do not have the configured shapes")
        values = np.stack([np.asarray(state["vmax"], dtype=np.float64), np.asarray(state["vmin"], dtype=np.float64)])
        counts = np.stack([np.asarray(state[k], dtype=np.int32) for k in ("tmax", "tmin", "nan")])
        thr = np.ascontiguousarray(state["thr"], dtype=np.uint32).view(np.int32)
        hist = np.concatenate([np.asarray(h, dtype=np.int64).reshape(-1) for h in state["hist"]]) if nbs else None
        self.call("qd_extremes_restore", values, counts, thr if nt else None, hist, int(state["n"]))

    def extremes_reset(self):
        self.call("qd_extremes_reset")

    # ---- per-step series (qd_series.hip)
    def series_configure(self, entries, zonal, w_row):
        """entries: [(op, a, b)] as history_configure takes them; zonal: the records carry every row's zonal mean; w_row [n_lat]:
        the row weights of the mean, max(cos lat, 0).  An empty list releases the lane."""
        if len(entries) and (w_row is None or np.size(w_row) != self.shape[0]):
            raise ValueError("series_configure: w_row holds one weight per latitude row")
        self.call("qd_series_configure", len(entries), [e[0] for e in entries], [F[e[1]] for e in entries],
                  [F[e[2]] if e[2] is not None else -1 for e in entries], int(bool(zonal)), None if w_row is None else _c(w_row).reshape(-1))
        self._series_width = len(entries) * (_lib.SERIES_STATS + (self.shape[0] if zonal else 0))

    def series_schedule(self, sample):
        self.call("qd_series_schedule", np.size(sample), sample)

    def series_sample(self):
        """One record of every entry from the fields as they stand (the class seam)."""
        self.flush()
        self.call("qd_series_sample")

    def series_log(self, max_records=None):
        """Drain the records -> [n][width], oldest first; width = entries * (SERIES_STATS + (n_lat if zonal else 0)), per entry
        mean, min, max, nan_count and then the zonal means.  max_records: what the caller knows to be queued at most."""
        room = _lib.SERIES_LOG_CAP if max_records is None else max(0, min(int(max_records), _lib.SERIES_LOG_CAP))
        w = max(1, self._series_width)
        buf = np.empty(max(1, room) * w, dtype=np.float64)      # a record is large: no zero-filled ctypes buffer here
        return self._records((buf, self.call("qd_series_log", buf, room, OUT)), w)

    def series_reset(self):
        self.call("qd_series_reset")

    # ---- zonal wavenumber spectra (qd_spectra.hip)
    def spectra_configure(self, entries, lat_resolved, w_row):
        """entries: [(op, a, b)] as history_configure takes them; lat_resolved: the per-row powers are also summed in resident
        planes (spectra_sums); w_row [n_lat]: the row weights of the global spectrum, max(cos lat, 0).  An empty list releases the
        lane.  QD_SPECTRA_FORM=direct in the environment of this call forces the direct DFT."""
        if len(entries) and (w_row is None or np.size(w_row) != self.shape[0]):
            raise ValueError("spectra_configure: w_row holds one weight per latitude row")
        self.call("qd_spectra_configure", len(entries), [e[0] for e in entries], [F[e[1]] for e in entries],
                  [F[e[2]] if e[2] is not None else -1 for e in entries], int(bool(lat_resolved)), None if w_row is None else _c(w_row).reshape(-1))
        self._spectra_n, self._spectra_lat = len(entries), bool(lat_resolved) and len(entries) > 0

    @property
    def spectra_bins(self):
        return self.shape[1] // 2 + 1

    def spectra_schedule(self, sample):
        self.call("qd_spectra_schedule", np.size(sample), sample)

    def spectra_sample(self):
        """One record of every entry from the fields as they stand (the class seam)."""
        self.flush()
        self.call("qd_spectra_sample")

    def spectra_log(self, max_records=None):
        """Drain the records -> [n][width], oldest first; width = entries * (n_bins + SPECTRA_STATS), per entry the global spectrum
        P(0 .. n_lon // 2) and then the count of non-finite rows.  max_records: what the caller knows to be queued at most."""
        room = _lib.SPECTRA_LOG_CAP if max_records is None else max(0, min(int(max_records), _lib.SPECTRA_LOG_CAP))
        w = max(1, self._spectra_n * (self.spectra_bins + _lib.SPECTRA_STATS))
        buf = np.empty(max(1, room) * w, dtype=np.float64)      # a record is large: no zero-filled ctypes buffer here
        return self._records((buf, self.call("qd_spectra_log", buf, room, OUT)), w)

    def spectra_sums(self):
        """-> (sums [n][n_lat][n_bins] of the per-row powers, sample count); lat-resolved configurations only."""
        out = np.empty((self._spectra_n, self.shape[0], self.spectra_bins), dtype=np.float64)
        return out, self.call("qd_spectra_sums_get", out, OUT)

    def spectra_sums_set(self, sums, count):
        """The inverse of spectra_sums, for an exact resume."""
        want = (self._spectra_n, self.shape[0], self.spectra_bins)
        if np.shape(sums) != want:
            raise ValueError(f"spectra_sums_set: expected sums of shape {want}, got {np.shape(sums)}")
        self.call("qd_spectra_sums_set", _c(sums), count)

    def spectra_reset(self):
        self.call("qd_spectra_reset")

    # ---- spherical-harmonic power spectra (qd_spharm.hip)
    def spharm_configure(self, entries, two_d, tables, flow_tables=None):
        """entries: [(op, a, b)] as history_configure takes them, or (QD_SPHARM_OP_VORT / _DIV, None, None); two_d: the terms
        c_m |x_n^m|^2 are also summed in resident planes (spharm_sums); tables: spharm.tables(n_lat, n_lon); flow_tables:
        flow.grid_tables(grid, radius), needed when an entry is VORT or DIV.  An empty list (or tables None) releases the lane.
        QD_SPHARM_FORM=direct in the environment of this call forces the direct row sums."""
        if not len(entries) or tables is None:
            self.call("qd_spharm_configure", 0, None, None, None, 0, 0, None, None, None, None, None, None, None)
            self._spharm_n, self._spharm_2d, self._spharm_N = 0, False, 0
            return
        if (tables.n_lat, tables.n_lon) != self.shape:
            raise ValueError(f"spharm_configure: the tables are for a {tables.n_lat} x {tables.n_lon} grid, the handle's is {self.shape}")
        own = (_lib.C["QD_SPHARM_OP_VORT"], _lib.C["QD_SPHARM_OP_DIV"])
        if flow_tables is None and any(e[0] in own for e in entries):
            raise ValueError("spharm_configure: a VORT or DIV entry needs the flow lane's grid tables (flow.grid_tables)")
        self.call("qd_spharm_configure", len(entries), [e[0] for e in entries], [F[e[1]] if e[1] is not None else -1 for e in entries],
                  [F[e[2]] if e[2] is not None else -1 for e in entries], int(bool(two_d)), tables.N, tables.w, tables.mu,
                  tables.seed_pairs, tables.A, tables.B, None if flow_tables is None else flow_tables.tab,
                  None if flow_tables is None else flow_tables.geom)
        self._spharm_n, self._spharm_2d, self._spharm_N = len(entries), bool(two_d), int(tables.N)

    def spharm_schedule(self, sample):
        self.call("qd_spharm_schedule", np.size(sample), sample)

    def spharm_sample(self):
        """One record of every entry from the fields as they stand, added to the 2D sums (the class seam)."""
        self.flush()
        self.call("qd_spharm_sample")

    def spharm_log(self, max_records=None):
        """Drain the records -> [n][width], oldest first; width = entries * (N + 1 + QD_SPHARM_STATS), per entry P(0 .. N), the mean
        square and the count of bad rows.  max_records: what the caller knows to be queued at most."""
        cap = _lib.C["QD_SPHARM_LOG_CAP"]
        room = cap if max_records is None else max(0, min(int(max_records), cap))
        w = max(1, self._spharm_n * (self._spharm_N + 1 + _lib.C["QD_SPHARM_STATS"]))
        buf = np.empty(max(1, room) * w, dtype=np.float64)
        return self._records((buf, self.call("qd_spharm_log", buf, room, OUT)), w)

    def spharm_sums(self):
        """-> (sums [n][N + 1 (n)][N + 1 (m)] of c_m |x_n^m|^2, sample count); 2D configurations only."""
        out = np.empty((self._spharm_n, self._spharm_N + 1, self._spharm_N + 1), dtype=np.float64)
        return out, self.call("qd_spharm_sums_get", out, OUT)

    def spharm_sums_set(self, sums, count):
        """The inverse of spharm_sums, for an exact resume."""
        want = (self._spharm_n, self._spharm_N + 1, self._spharm_N + 1)
        if np.shape(sums) != want:
            raise ValueError(f"spharm_sums_set: expected sums of shape {want}, got {np.shape(sums)}")
        self.call("qd_spharm_sums_set", _c(sums), count)

    def spharm_reset(self):
        self.call("qd_spharm_reset")

    def spharm_analyse(self, plane):
        """The kernels of one entry on a host plane (the class seam, outside any span) -> (coef [m][n] complex, rec
        [N + 1 + QD_SPHARM_STATS]); the log and the 2D sums stay as they are."""
        x = _c(plane)
        if x.shape != self.shape:
            raise ValueError(f"spharm_analyse: the plane is of shape {self.shape}")
        n1 = self._spharm_N + 1
        re, im, rec = np.empty((n1, n1)), np.empty((n1, n1)), np.empty(n1 + _lib.C["QD_SPHARM_STATS"])
        self.call("qd_spharm_analyse", x, re, im, rec)
        return re + 1j * im, rec

    # ---- eddy statistics (qd_eddy.hip)
    def eddy_configure(self, fields, pairs):
        """fields: names of distinct f64 planes; pairs: [(p, q)] indices into them (p == q: a variance).  An empty field list
        releases the lane."""
        if not len(fields):
            self.call("qd_eddy_configure", 0, None, 0, None, None)
            self._eddy = (0, 0)
            return
        self.call("qd_eddy_configure", len(fields), [F[n] for n in fields], len(pairs), [int(a) for a, _ in pairs], [int(b) for _, b in pairs])
        self._eddy = (len(fields), len(pairs))

    def eddy_schedule(self, sample):
        self.call("qd_eddy_schedule", np.size(sample), sample)

    def eddy_sample(self):
        """One sample of every field and pair from the planes as they stand (the class seam)."""
        self.flush()
        self.call("qd_eddy_sample")

    def eddy_read(self):
        """-> (anchors [F][n_lat][n_lon], sums [F][n_lat][n_lon], pair sums [P][n_lat][n_lon], sample count)"""
        nf, npair = self._eddy
        r, s, c = (np.empty((n,) + self.shape, dtype=np.float64) for n in (nf, nf, npair))
        return r, s, c, self.call("qd_eddy_read", r, s, c, OUT)

    def eddy_restore(self, anchors, sums, pair_sums, count):
        """The inverse of eddy_read, for an exact resume."""
        nf, npair = self._eddy
        for name, a, n in (("anchors", anchors, nf), ("sums", sums, nf), ("pair_sums", pair_sums, npair)):
            if np.shape(a) != (n,) + self.shape:
                raise ValueError(f"eddy_restore: expected {name} of shape {(n,) + self.shape}, got {np.shape(a)}")
        self.call("qd_eddy_restore", anchors, sums, pair_sums, count)

    def eddy_zonal(self):
        """-> [P][4][n_lat]: per pair and row the sums over the columns of S_p, S_q, C and S_p * S_q (k_eddy_zonal)"""
        out = np.empty((self._eddy[1], _lib.C["QD_EDDY_ZONAL_SUMS"], self.shape[0]), dtype=np.float64)
        self.call("qd_eddy_zonal", out)
        return out

    def eddy_reset(self):
        self.call("qd_eddy_reset")

    # ---- Lagrangian drifters (qd_drift.hip)
    def drift_configure(self, atm, ocn, sample_atm, sample_ocn, sec_row):
        """atm, ocn: (r, c) index coordinates of the two populations' particles (r in [0, n_lat - 1], c in [0, n_lon - 1)), or None;
        sample_atm, sample_ocn: up to DRIFT_MAX_SAMPLES field names each; sec_row [n_lat]: drifters.sec_table.  Two empty populations
        release the lane.  -> the records the lane's log holds between two drains."""
        pops = [(np.empty(0), np.empty(0)) if p is None else (_c(p[0]).reshape(-1), _c(p[1]).reshape(-1)) for p in (atm, ocn)]
        for r, c in pops:
            if r.shape != c.shape:
                raise ValueError("drift_configure: a population holds one column coordinate per row coordinate")
        n = [int(r.size) for r, _ in pops]
        if sum(n) and (sec_row is None or np.size(sec_row) != self.shape[0]):
            raise ValueError("drift_configure: sec_row holds one value per latitude row")
        names = [list(s or []) if k else [] for s, k in zip((sample_atm, sample_ocn), n)]
        cap = self.call("qd_drift_configure", n[0], pops[0][0], pops[0][1], n[1], pops[1][0], pops[1][1], len(names[0]),
                        [F[x] for x in names[0]] or None, len(names[1]), [F[x] for x in names[1]] or None,
                        None if sec_row is None else _c(sec_row).reshape(-1), OUT)
        width = n[0] * (3 + len(names[0])) + n[1] * (4 + len(names[1]))
        self._drift = (n[0], n[1], width, int(cap))
        return int(cap)

    def drift_schedule(self, record):
        self.call("qd_drift_schedule", np.size(record), record)

    def drift_advance(self, dt, record=False):
        """One step of every live particle on the planes as they stand (the class seam); record: it also leaves a record."""
        self.flush()
        self.call("qd_drift_advance", dt, bool(record))

    def drift_log(self, max_records=None):
        """Drain the records -> [n][width], oldest first: [atm: r | c | status | samples][ocn: r | c | status | blocked | samples],
        each block one double per particle."""
        cap = max(1, self._drift[3])
        room = cap if max_records is None else max(0, min(int(max_records), cap))
        w = max(1, self._drift[2])
        buf = np.empty(max(1, room) * w, dtype=np.float64)      # a record is large: no zero-filled ctypes buffer here
        return self._records((buf, self.call("qd_drift_log", buf, room, OUT)), w)

    def drift_state(self):
        """-> (atm [3][n_atm] = r | c | status, ocn [4][n_ocn] = r | c | status | blocked) as the particles stand."""
        atm, ocn = np.empty((3, self._drift[0])), np.empty((4, self._drift[1]))
        self.call("qd_drift_state_get", atm if atm.size else None, ocn if ocn.size else None)
        return atm, ocn

    def drift_state_set(self, atm, ocn):
        """The inverse of drift_state, for an exact resume."""
        atm, ocn = _c(atm).reshape(3, -1), _c(ocn).reshape(4, -1)
        if (atm.shape[1], ocn.shape[1]) != self._drift[:2]:
            raise ValueError(f"drift_state_set: expected {self._drift[0]} atm and {self._drift[1]} ocn particles, got {atm.shape[1]} and {ocn.shape[1]}")
        self.call("qd_drift_state_set", atm if atm.size else None, ocn if ocn.size else None)

    def drift_reset(self):
        self.call("qd_drift_reset")

    # ---- streamfunction and velocity potential (qd_flow.hip)
    def flow_configure(self, tables):
        """tables: flow.grid_tables(grid, radius), the grid quantities of the discrete system; None releases the lane.
        QD_FLOW_FORM=direct in the environment of this call forces the direct row transforms."""
        if tables is None:
            self.call("qd_flow_configure", None, None, None)
        else:
            if (tables.n_lat, tables.n_lon) != self.shape:
                raise ValueError(f"flow_configure: the tables are for a {tables.n_lat} x {tables.n_lon} grid, the handle's is {self.shape}")
            self.call("qd_flow_configure", tables.tab, tables.lam, tables.geom)
        self._flow = tables is not None

    def flow_schedule(self, sample):
        self.call("qd_flow_schedule", np.size(sample), sample)

    def flow_sample(self):
        """One record from the resident U, V as they stand, added to the sum planes (the class seam)."""
        self.flush()
        self.call("qd_flow_sample")

    def flow_log(self, max_records=None):
        """Drain the records -> [n][QD_FLOW_REC_W] (flow.REC), oldest first.  max_records: what the caller knows to be queued at most."""
        room = _lib.C["QD_FLOW_LOG_CAP"] if max_records is None else max(0, min(int(max_records), _lib.C["QD_FLOW_LOG_CAP"]))
        w = _lib.C["QD_FLOW_REC_W"]
        buf = np.empty(max(1, room) * w, dtype=np.float64)
        return self._records((buf, self.call("qd_flow_log", buf, room, OUT)), w)

    def flow_sums(self):
        """-> (sums [4][n_lat][n_lon] of psi, chi, zeta, delta over the samples of the window, sample count)."""
        out = np.empty((_lib.C["QD_FLOW_PLANES"],) + self.shape, dtype=np.float64)
        return out, self.call("qd_flow_sums_get", out, OUT)

    def flow_sums_set(self, sums, count):
        """The inverse of flow_sums, for an exact resume."""
        want = (_lib.C["QD_FLOW_PLANES"],) + self.shape
        if np.shape(sums) != want:
            raise ValueError(f"flow_sums_set: expected sums of shape {want}, got {np.shape(sums)}")
        self.call("qd_flow_sums_set", _c(sums), count)

    def flow_reset(self):
        self.call("qd_flow_reset")

    def flow_solve(self, u, v):
        """The kernels of a sample on host planes (the class seam, outside any span) -> (zeta, delta, psi, chi); the record goes
        to the log (flow_log), the sum planes stay as they are."""
        u, v = (_c(x) for x in (u, v))
        if u.shape != self.shape or v.shape != self.shape:
            raise ValueError(f"flow_solve: u and v are planes of shape {self.shape}")
        zeta, delta, psi, chi = (np.empty(self.shape, dtype=np.float64) for _ in range(4))
        self.call("qd_flow_solve", u, v, zeta, delta, psi, chi)
        return zeta, delta, psi, chi

    # ---- daily phytoplankton step (qd_phyto_daily.hip)
    def phyto_daily_configure(self, params, band_tab, species_tab, shape):
        self.call("qd_phyto_daily_configure", params, ctypes.sizeof(params), band_tab, species_tab, shape)

    def phyto_daily(self, star_row, use_sst):
        self.flush()
        self.call("qd_phyto_daily", _c(star_row).reshape(7), bool(use_sst))

    def phyto_daily_schedule(self, fire):
        self.call("qd_phyto_daily_schedule", np.size(fire), fire)

    def phyto_daily_log(self):
        """Drain the [PhytoDiag] records -> [n][4] (daily steps so far, <C_tot>, <Kd490>, <alpha_water>)."""
        return self._records(self.call("qd_phyto_daily_log", OUT(_lib.SPAN_LOG_CAP * _lib.PHYTO_DAILY_LOG_W), _lib.SPAN_LOG_CAP, OUT),
                             _lib.PHYTO_DAILY_LOG_W)

    def phyto_daily_bands(self, nb):
        out = np.empty((nb,) + self.shape, dtype=np.float64)
        self.call("qd_phyto_daily_download_bands", out, out.size)
        return out

    def phyto_daily_steps(self):
        return self.call("qd_phyto_daily_state", OUT)

    # ---- daily vegetation step (qd_eco_daily.hip)
    def eco_daily_configure(self, params, species_mode, species_weights):
        self.call("qd_eco_daily_configure", params, ctypes.sizeof(params), species_mode, species_weights)

    def eco_daily_set_layers(self, layers):
        a = _c(layers)
        self.call("qd_eco_daily_set_layers", a, np.prod(a.shape[:-2]))

    def eco_daily_get_layers(self, n_species, n_layers):
        out = np.empty((n_species, n_layers) + self.shape, dtype=np.float64)
        self.call("qd_eco_daily_get_layers", out, n_species * n_layers)
        return out

    def _soil(self, soil_index):
        return None if soil_index is None else np.broadcast_to(np.asarray(soil_index, dtype=np.float64), self.shape)

    def eco_daily_step(self, soil_index=None):
        """One firing now; soil_index None = from the resident W_LAND and GLACIER, as inside a span."""
        self.flush()
        self.call("qd_eco_daily_step", self._soil(soil_index))
        for k in ("ECO_LAI", "ECO_EDAY", "ECO_AGE", "ECO_SEEDBANK", "ECO_GATE"):
            self._host.pop(k, None)

    def eco_daily_schedule(self, fire):
        self.call("qd_eco_daily_schedule", np.size(fire), fire)

    def eco_daily_log(self):
        """Drain the daily vegetation records -> [n][4] (firings so far, LAI_min, LAI_mean, LAI_max over land)."""
        return self._records(self.call("qd_eco_daily_log", OUT(_lib.SPAN_LOG_CAP * _lib.ECO_DAILY_LOG_W), _lib.SPAN_LOG_CAP, OUT),
                             _lib.ECO_DAILY_LOG_W)

    def eco_daily_firings(self):
        return self.call("qd_eco_daily_state", OUT)

    def eco_daily_speciate(self, parent, frac, n_species):
        """One speciation event on the resident stack of n_species species (qd_eco_speciate.hip) -> species_weights [n_species + 1]."""
        self.flush()
        out = self.call("qd_eco_daily_speciate", parent, frac, OUT(int(n_species) + 1))
        self._host.pop("ECO_LAI", None)
        return out

    # ---- restore from an ecology autosave (qd_eco_state.hip)
    def eco_state_restore(self, lai, weights, n_layers, lai_max):
        """adapter.py:742-757 on the device: lai [lat, lon] float32 (the arithmetic is then float32, as the reference's NetCDF
        branch runs it) or float64; weights [S] as the reference leaves them.  Writes the resident stack of the daily lane when it
        exists, and ECO_LAI."""
        self.flush()
        f32 = np.asarray(lai).dtype == np.float32
        a = _c(lai, np.float32 if f32 else np.float64)
        if a.shape != self.shape:
            raise ValueError(f"eco_state_restore: expected a [{self.shape[0]}, {self.shape[1]}] LAI plane, got {a.shape}")
        self.call("qd_eco_state_restore", a, f32, weights, np.size(weights), n_layers, lai_max)
        self._host.pop("ECO_LAI", None)

    # ---- daily step of the individuals (qd_indiv_daily.hip)
    def indiv_daily_configure(self, params, species_id, level):
        self.call("qd_indiv_daily_configure", params, ctypes.sizeof(params), species_id, level)

    def indiv_daily_step(self, soil_index=None):
        """One firing now; soil_index None = from the resident W_LAND and GLACIER, as inside a span."""
        self.flush()
        self.call("qd_indiv_daily_step", self._soil(soil_index))
        for k in ("ECO_LAI", "ECO_SEEDBANK"):
            self._host.pop(k, None)

    def indiv_daily_log(self):
        """Drain the individuals' daily records -> [n][4] (firings so far, beta_hint, n_cells, levels)."""
        return self._records(self.call("qd_indiv_daily_log", OUT(_lib.SPAN_LOG_CAP * _lib.INDIV_DAILY_LOG_W), _lib.SPAN_LOG_CAP, OUT),
                             _lib.INDIV_DAILY_LOG_W)

    def indiv_daily_weights(self, n_species):
        return self.call("qd_indiv_daily_weights", OUT(n_species), n_species)

    def indiv_daily_firings(self):
        return self.call("qd_indiv_daily_state", OUT)

    # ---- diversity diagnostics (qd_eco_div.hip)
    def eco_diversity(self, w_norm_row, layers=None, n_species=None, n_layers=None, land_mask=None):
        """pygcm/ecology/diversity.py on the device -> {alpha_mean, gamma_eff, beta_whittaker}; the maps stay resident
        (eco_diversity_get).  layers None: the resident stack of eco_daily_configure (n_species, n_layers name its shape); else a host
        [S, K, lat, lon] stack.  land_mask None: the ecology's land mask on the handle's grid; else the caller's mask, whose shape
        is the grid of the call (layers is then required)."""
        w = _c(w_norm_row)
        a = None
        if layers is not None:
            a = _c(layers)
            if a.ndim != 4:
                raise ValueError(f"eco_diversity: layers must be [S, K, lat, lon], got {a.shape}")
            n_species, n_layers = a.shape[:2]
        if land_mask is not None:
            m = _c(land_mask, np.uint8)
            if a is None or a.shape[2:] != m.shape or w.shape != (m.shape[0],):
                raise ValueError("eco_diversity: a land mask of the caller's needs a host stack and a weight row of its shape")
            out = self.call("qd_eco_diversity_on", m.shape[0], m.shape[1], m, a, n_species, n_layers, w, OUT(3))
            self._div_shape = (int(n_species),) + m.shape
        else:
            if w.shape != (self.shape[0],) or (a is not None and a.shape[2:] != self.shape):
                raise ValueError(f"eco_diversity: expected [S, K, {self.shape[0]}, {self.shape[1]}] layers and {self.shape[0]} row weights")
            out = self.call("qd_eco_diversity", a, n_species, n_layers, w, OUT(3))
            self._div_shape = (int(n_species),) + self.shape
        return dict(zip(("alpha_mean", "gamma_eff", "beta_whittaker"), out.tolist()))

    def eco_diversity_get(self, name):
        """A result of the last eco_diversity call: "ECO_DIV_LS" [S, lat, lon], "ECO_DIV_ALPHA", "ECO_DIV_BC" [lat, lon],
        "ECO_DIV_SUMMARY" [3]."""
        shp = self._div_shape
        shape = (3,) if name == "ECO_DIV_SUMMARY" else (None if shp is None else (shp if name == "ECO_DIV_LS" else shp[1:]))
        out = np.empty(shape if shape is not None else (1,), dtype=np.float64)
        self.call("qd_eco_diversity_download", F[name], out, out.size)
        return out

    # ---- true-colour frame (qd_truecolor.hip)
    def truecolor_configure(self, params, eco_tab=None, phyto_tab=None, phyto_bands=None, lake_mask=None):
        """params: a _lib.qd_truecolor_params; eco_tab [7, nb_eco], phyto_tab [6, nb_phyto] (include/qingdai_hip.h); phyto_bands None =
        the resident stack of the daily phytoplankton step, else a host [nb_phyto, lat, lon] stack; lake_mask [lat, lon] or None."""
        if eco_tab is not None and np.shape(eco_tab) != (7, params.nb_eco) or phyto_tab is not None and np.shape(phyto_tab) != (6, params.nb_phyto):
            raise ValueError("truecolor_configure: eco_tab must be [7, nb_eco] and phyto_tab [6, nb_phyto]")
        if phyto_bands is not None and np.shape(phyto_bands) != (params.nb_phyto,) + self.shape or lake_mask is not None and np.shape(lake_mask) != self.shape:
            raise ValueError("truecolor_configure: phyto_bands must be [nb_phyto, lat, lon] and lake_mask [lat, lon]")
        self.call("qd_truecolor_configure", params, ctypes.sizeof(params), eco_tab, phyto_tab, phyto_bands, lake_mask)

    def truecolor_render(self, want_f64=False, flow=None):
        """One frame from the resident state -> (sea_ice_area, mean_h_ice); the image stays resident (truecolor_image / truecolor_rgb).
        flow None: the routing state's flow map; else a host [lat, lon] map."""
        self.flush()
        if flow is not None and np.shape(flow) != self.shape:
            raise ValueError(f"truecolor_render: flow must be {self.shape}, got {np.shape(flow)}")
        return tuple(self.call("qd_truecolor_render", bool(want_f64), flow, OUT(2)).tolist())

    def truecolor_image(self):
        """The u8 image [lat, lon, 3] of the last render, northernmost row first."""
        out = np.empty(self.shape + (3,), dtype=np.uint8)
        self.call("qd_truecolor_download", 0, out, out.size)
        return out

    def truecolor_rgb(self):
        """The unquantised f64 rgb [lat, lon, 3] in grid order of the last render (want_f64=True)."""
        out = np.empty(self.shape + (3,), dtype=np.float64)
        self.call("qd_truecolor_download", 1, out, out.size)
        return out

    # ---- 15-panel state frame (qd_stateframe.hip)
    def stateframe_configure(self, params, lake_mask=None):
        """params: a _lib.qd_stateframe_params; lake_mask [lat, lon] or None."""
        if lake_mask is not None and np.shape(lake_mask) != self.shape:
            raise ValueError(f"stateframe_configure: lake_mask must be {self.shape}, got {np.shape(lake_mask)}")
        self.call("qd_stateframe_configure", params, ctypes.sizeof(params), lake_mask)

    def stateframe_scan(self):
        """The extremes and the two argmax cells the level rules need, from the state as it stands -> (the STATEFRAME_SCAN_N doubles
        include/qingdai_hip.h names, [cell of star A, cell of star B]).  Also fills the vorticity plane the render reads."""
        self.flush()
        out, marks = self.call("qd_stateframe_scan", OUT(_lib.STATEFRAME_SCAN_N), OUT(2))
        return out, marks.tolist()

    def stateframe_render(self, table, flow=None, want_stacks=False):
        """table: a _lib.qd_stateframe_table.  flow None: the routing state's flow map; else a host [lat, lon] map.  The mosaic stays
        resident (stateframe_image / stateframe_bands / stateframe_fields)."""
        self.flush()
        if flow is not None and np.shape(flow) != self.shape:
            raise ValueError(f"stateframe_render: flow must be {self.shape}, got {np.shape(flow)}")
        self.call("qd_stateframe_render", table, ctypes.sizeof(table), flow, bool(want_stacks))

    def stateframe_image(self):
        """The u8 mosaic [5 lat + 6 gutters, 3 lon + 4 gutters, 3] of the last render."""
        g = _lib.STATEFRAME_GUTTER
        out = np.empty((5 * self.shape[0] + 6 * g, 3 * self.shape[1] + 4 * g, 3), dtype=np.uint8)
        self.call("qd_stateframe_download", 0, out, out.size)
        return out

    def stateframe_bands(self):
        """The int8 band indices [15, lat, lon] in grid order of the last render (want_stacks=True); -1 = white."""
        out = np.empty((_lib.STATEFRAME_PANELS,) + self.shape, dtype=np.int8)
        self.call("qd_stateframe_download", 1, out, out.size)
        return out

    def stateframe_fields(self):
        """The f64 fields [15, lat, lon] handed to the band search by the last render (want_stacks=True)."""
        out = np.empty((_lib.STATEFRAME_PANELS,) + self.shape, dtype=np.float64)
        self.call("qd_stateframe_download", 2, out, out.size)
        return out

    # ---- tiles of the ecology / plankton / ISR figures (qd_tiles.hip)
    def tiles_configure(self, height_scale=10.0, layers=None):
        """height_scale: QD_ECO_HEIGHT_SCALE_M.  layers None: the stack sources read the resident stack of eco_daily_configure; else a
        host [S, K, lat, lon] stack, uploaded here."""
        shp = (0, 0) if layers is None else np.shape(layers)
        if layers is not None and (len(shp) != 4 or shp[2:] != self.shape):
            raise ValueError(f"tiles_configure: layers must be [S, K, {self.shape[0]}, {self.shape[1]}], got {shp}")
        self.call("qd_tiles_configure", height_scale, layers, shp[0], shp[1])

    def tiles_set_plane(self, plane):
        """A host [lat, lon] map for the tile source "HOST_PLANE" (kept until the next tiles_configure)."""
        if np.shape(plane) != self.shape:
            raise ValueError(f"tiles_set_plane: plane must be {self.shape}, got {np.shape(plane)}")
        self.call("qd_tiles_set_plane", plane)

    def tiles_available(self):
        """-> (an LAI map, a scalar alpha map, a banded alpha map) are on the device."""
        return tuple(bool(x) for x in self.call("qd_tiles_available", OUT(3)))

    @staticmethod
    def _tile_refs(refs):
        arr = (_lib.qd_tile_ref * max(1, len(refs)))()
        for k, (src, idx) in enumerate(refs):
            arr[k].source, arr[k].index = (_lib.TILE[src] if isinstance(src, str) else int(src)), int(idx)
        return arr

    def tiles_scan(self, refs):
        """refs: up to 8 (source, index), source a name of _lib.TILE_SOURCES or its id -> per plane {"min", "max" over the finite values,
        "nan" (the plane holds one), "argmax" (np.argmax's flat cell), "argmax_value"}."""
        self.flush()
        n = len(refs)
        out, cells = self.call("qd_tiles_scan", self._tile_refs(refs), n, OUT(4 * max(1, n)), OUT(max(1, n)))
        out = out.reshape(-1, 4)
        return [{"min": float(out[k, 0]), "max": float(out[k, 1]), "nan": bool(out[k, 2] > 0.0), "argmax": int(cells[k]),
                 "argmax_value": float(out[k, 3])} for k in range(n)]

    def tiles_order_stats(self, source, index, ranks):
        """-> (count of non-NaN cells, [the ranks[k]-th smallest of them, 0-based]); NaN for a rank that is not below the count."""
        self.flush()
        vals = np.full(max(1, len(ranks)), np.nan, dtype=np.float64)
        count = self.call("qd_tiles_order_stats", _lib.TILE[source] if isinstance(source, str) else source, index,
                          ranks if len(ranks) else [0], len(ranks), vals, OUT)
        return count, vals[:len(ranks)]

    def tiles_render(self, tiles, want_stacks=False):
        """tiles: a sequence of _lib.qd_tile_desc (one row, at most 8).  The mosaic stays resident (tiles_image / tiles_bands /
        tiles_planes)."""
        self.flush()
        n = len(tiles)
        self.call("qd_tiles_render", (_lib.qd_tile_desc * max(1, n))(*tiles), ctypes.sizeof(_lib.qd_tile_desc), n, bool(want_stacks))
        self._tiles_n = n

    def tiles_image(self):
        """The u8 mosaic [lat + 2 gutters, n lon + (n + 1) gutters, 3] of the last render."""
        g, n = _lib.STATEFRAME_GUTTER, self._tiles_n
        out = np.empty((self.shape[0] + 2 * g, n * self.shape[1] + (n + 1) * g, 3), dtype=np.uint8)
        self.call("qd_tiles_download", 0, out, out.size)
        return out

    def tiles_bands(self):
        """The int8 band indices [n, lat, lon] of the last render (want_stacks=True); -1 = white."""
        out = np.empty((self._tiles_n,) + self.shape, dtype=np.int8)
        self.call("qd_tiles_download", 1, out, out.size)
        return out

    def tiles_planes(self):
        """The f64 planes [n, lat, lon] handed to the band search by the last render (want_stacks=True)."""
        out = np.empty((self._tiles_n,) + self.shape, dtype=np.float64)
        self.call("qd_tiles_download", 2, out, out.size)
        return out

    # ---- phytoplankton tracers carried by the ocean currents (pygcm/ecology/phyto.py:496-547), resident
    def phyto_configure(self, n_species, K_h, adv_alpha):
        self.call("qd_phyto_configure", n_species, K_h, adv_alpha)
        self._phyto_S = int(n_species)

    def phyto_upload(self, C_s):
        C_s = _c(C_s)
        assert C_s.ndim == 3 and C_s.shape[0] == getattr(self, "_phyto_S", -1) and C_s.shape[1:] == self.shape
        for s in range(C_s.shape[0]):
            self.call("qd_phyto_upload", s, C_s[s])

    def phyto_download(self):
        self.flush()
        out = np.zeros((self._phyto_S,) + self.shape, dtype=np.float64)
        for s in range(self._phyto_S):
            self.call("qd_phyto_download", s, out[s])
        return out

    def phyto_advect_diffuse(self, dt_seconds):
        """PhytoManager.advect_diffuse on the resident tracers and the resident uo / vo (three launches for all species)."""
        self.flush()
        self.call("qd_phyto_advect_diffuse", dt_seconds)

    def last_ocean_nsub(self):
        return self.call("qd_last_ocean_nsub", OUT)

    def step_scalars(self):
        """The device scalars a step's launches hand to each other (include/qingdai_hip.h: qd_step_scalars), by name."""
        return dict(zip(("PREF", "ETA_MEAN", "MED_OUT", "PSCALE", "RENORM", "BLEND_W", "TMP0", "TMP1"), self.call("qd_step_scalars", OUT(8))))

    def ocean_mean_next_count(self):
        """Ocean sub-steps since create whose eta mean the next momentum launch finished (QD_MEAN_IN_MOMENTUM)."""
        return self.call("qd_ocean_mean_next_count", OUT)

    def step_forms(self):
        """Which form of the step kernels this handle takes and what the last step chose (include/qingdai_hip.h: qd_step_forms,
        enum qd_step_form), by the enumerators' lower-case names: dyn_stream, ocn_ntc, tile_tr, tail_kernel, last_mean_form, ...;
        cnt_* / max_*: tallies since the handle was created of the launch-by-launch decisions a latitude band makes"""
        out = self.call("qd_step_forms", OUT(_lib.C["QD_SF_N"]))
        return {k[len("QD_SF_"):].lower(): int(out[v]) for k, v in _lib.C.items() if k.startswith("QD_SF_") and k != "QD_SF_N"}

    def counters(self):
        return self.call("qd_get_step_counter", OUT, OUT)

    def set_counters(self, a, o):
        self.call("qd_set_step_counter", a, o)

    # ---- state digest and the scalars of an exact resume (qd_digest.hip)
    def digest(self, names):
        """The 64-bit digests of resident planes (include/qingdai_hip.h: qd_state_digest), one launch per 64 of them -> np.uint64[n].
        names: what _lib.state_ref takes -- field names, LAND_MASK, ICE_MASK, ROUTE_BUFFER, ROUTE_FLOW, ROUTE_LAKES, ECO_LAI_STACK,
        INDIV_E_DAY, INDIV_STRESS, SPECTRA_SUMS, FLOW_SUMS, SPHARM_SUMS, EDDY_SUMS, EDDY_ANCHORS, EXTREMES_VALUES, EXTREMES_COUNTS, EXTREMES_HIST, "PHYTO_TRACER:s", "HISTORY_SUM:k".  A plane whose subsystem is not configured raises."""
        self.flush()
        refs = [_lib.state_ref(n) for n in names]
        out = np.zeros(len(refs), dtype=np.uint64)
        for k in range(0, len(refs), _lib.STATE_DIGEST_MAX):
            r, o = refs[k:k + _lib.STATE_DIGEST_MAX], out[k:k + _lib.STATE_DIGEST_MAX]
            self.call("qd_state_digest", len(r), r, o)
        return out

    def state_scalars(self):
        """The host-side scalars a step reads besides the planes and the step counters -> float64[STATE_SCALARS_N]."""
        return self.call("qd_state_scalars_get", OUT(_lib.STATE_SCALARS_N), _lib.STATE_SCALARS_N)

    def set_state_scalars(self, values):
        self.call("qd_state_scalars_set", values, np.size(values))

    def route_restore(self, buffer, flow, lakes, steps):
        """The inverse of route_download("BUFFER" / "FLOW" / "LAKES") plus the accumulation count."""
        lk = None if lakes is None or np.size(lakes) == 0 else lakes
        if np.size(buffer) != self._route_n[0] or np.size(flow) != self._route_n[0] or (0 if lk is None else np.size(lk)) != self._route_n[1]:
            raise ValueError("route_restore: the arrays do not have the configured network's cell and lake counts")
        self.call("qd_route_restore", buffer, flow, lk, steps)

    def history_restore(self, sums, count):
        """The inverse of history_read: an open window's sums [n][n_lat][n_lon] and its sample count."""
        if np.shape(sums) != (self._history_n,) + self.shape:
            raise ValueError(f"history_restore: expected sums of shape {(self._history_n,) + self.shape}, got {np.shape(sums)}")
        self.call("qd_history_restore", sums, count)

    def reduce(self, name, op):
        self.flush()
        return self.call("qd_reduce", F[name], op, OUT)

    # ---- timing hooks
    def timing(self, on=True, select=None):
        if select:
            self.call("qd_timing_select", select)
        else:
            self.call("qd_timing_enable", bool(on))
        self.call("qd_timing_reset")

    def timing_get(self, name):
        return self.call("qd_timing_get", name, OUT, OUT)

    # ---- operator seam (jax_compat.py:111-216): host in, host out
    def _out(self):
        return np.empty(self.shape, dtype=np.float64)

    def op_laplacian(self, Fh, ocean=False):
        out = self._out()
        self.call("qd_op_laplacian", Fh, bool(ocean), out)
        return out

    def op_hyperdiffuse(self, Fh, k4, dt, n_substeps=1, ocean=False):
        out, k = self._out(), None
        if not np.isscalar(k4):
            k = np.asarray(k4, dtype=np.float64)
            if k.ndim == 2:          # the reference's maps are constant along longitude
                if not np.all(k == k[:, :1]):
                    raise ValueError("k4 map must be a function of latitude only")
                k = k[:, 0]
        self.call("qd_op_hyperdiffuse", Fh, k, 0.0 if k is not None else k4, dt, n_substeps, bool(ocean), out)
        return out

    def op_advect(self, field, u, v, dt, ocean=False):
        out = self._out()
        self.call("qd_op_advect", field, u, v, dt, bool(ocean), out)
        return out

    def op_shapiro(self, Fh, n=2):
        out = self._out()
        self.call("qd_op_shapiro", Fh, n, out)
        return out

    ENERGY_DIAG_KEYS = ("TOA_net", "SFC_net", "ATM_net", "I_mean", "R_mean", "OLR_mean", "SW_sfc_mean", "LW_sfc_mean",
                        "SH_mean", "LH_mean")

    def energy_diagnostics(self):
        """energy.compute_energy_diagnostics (energy.py:494-538) of the resident state -> dict of global means."""
        self.flush()
        return dict(zip(self.ENERGY_DIAG_KEYS, self.call("qd_energy_diagnostics", OUT(10)).tolist()))

    def copy_ceiling(self, nbytes=1 << 30, reps=8):
        """Measured device-to-device streaming rate in GB/s (read + written bytes), past the Infinity Cache by default."""
        return self.call("qd_copy_ceiling", nbytes, reps, OUT)

    def energy_diagnostics_last(self):
        """The means taken inside the last step_n(..., energy_diag=True): first step, after time_step, before the ocean."""
        return dict(zip(self.ENERGY_DIAG_KEYS, self.call("qd_energy_diagnostics_last", OUT(10)).tolist()))

    def op_zonal_filter(self, Fh, cutoff=0.75, damp=0.5):
        """SpectralModel._spectral_zonal_filter (dynamics.py:233-258)."""
        out = self._out()
        self.call("qd_op_zonal_filter", Fh, cutoff, damp, out)
        return out

    def op_divvort(self, u, v, vort=False):
        out = self._out()
        if vort:
            self.call("qd_op_vorticity", u, v, out, what="qd_op_div/vort")
        else:
            self.call("qd_op_divergence", u, v, out, what="qd_op_div/vort")
        return out

    def op_gaussian(self, Fh, sigma, mode="reflect"):
        out = self._out()
        self.call("qd_op_gaussian", Fh, sigma, mode == "wrap", out)
        return out

    def op_median_positive(self, x, default):
        return self.call("qd_op_median_positive", x, default, OUT)

    def op_median_at(self, x, default, transform=0, tparam=0.0, site=0):
        """The exact median of the positives of x (transform 0) or of max(0, -(x - tparam)) (transform 1) at call site `site`
        (0..3: keeps a window on the device; -1: none)."""
        return self.call("qd_op_median_at", x, default, transform, tparam, site, OUT)

    def op_median_pair(self, x0, default0, transform0, tparam0, site0, x1, default1, transform1, tparam1, site1):
        """Two medians through the step's pair chain -> (median 0, median 1); refused unless both sites have a window."""
        out = self.call("qd_op_median_pair", x0, default0, transform0, tparam0, site0, x1, default1, transform1, tparam1, site1, OUT(2))
        return float(out[0]), float(out[1])

    def median_state(self):
        """qd_median_state as one dict per call site: the form report of the last median there.  `lo_bits` / `hi_bits` are the bit
        patterns of the published bracket."""
        st = np.ascontiguousarray(self.call("qd_median_state", OUT(64))).reshape(4, 16)
        bits = st.view(np.uint64)
        return [dict(centre=float(s[0]), valid=bool(s[3]), hits=int(s[4]), misses=int(s[5]), list_len=int(s[6]), count=int(s[7]),
                     lo_bits=int(b[8]), hi_bits=int(b[9]), calls=int(s[12])) for s, b in zip(st, bits)]
