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
from ._lib import F, QdError
from .params import QdParams


def _c(a, dtype=np.float64):
    return np.ascontiguousarray(a, dtype=dtype)


class Device:
    _history_n = 0            # entries of the last history_configure
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
        self._dirty = set()       # fields whose host copy is newer than the device copy
        grid._device = self

    # ---- errors
    def _chk(self, rc, what):
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
        self._chk(self.lib.qd_set_params(self.h, ctypes.byref(ps), ctypes.sizeof(ps)), "qd_set_params")

    # ---- attribute surface
    def get(self, name):
        """Download (or return the cached host copy of) a field."""
        if name in self._host:
            return self._host[name]
        if name in ("LAND_MASK", "ICE_MASK"):
            out = np.empty(self.shape, dtype=np.uint8)
        else:
            out = np.empty(self.shape, dtype=np.float64)
        self._chk(self.lib.qd_download(self.h, F[name], out.ctypes.data, out.nbytes), f"qd_download({name})")
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
        self._dirty.add(name)

    def flush(self):
        """Send every host-side copy that may differ from the device (anything written, or
        read and possibly mutated in place) before device work starts."""
        for name in list(self._host):
            a = self._host[name]
            self._chk(self.lib.qd_upload(self.h, F[name], a.ctypes.data, a.nbytes), f"qd_upload({name})")
        self._host.clear()
        self._dirty.clear()

    def upload_now(self, name, arr):
        self.set(name, arr)
        a = self._host.pop(name)
        self._dirty.discard(name)
        self._chk(self.lib.qd_upload(self.h, F[name], a.ctypes.data, a.nbytes), f"qd_upload({name})")

    # ---- the path
    def forcing(self, star_a, star_b, theta, with_teq=True):
        self.flush()
        A = (ctypes.c_double * 3)(*star_a)
        B = (ctypes.c_double * 3)(*star_b)
        self._chk(self.lib.qd_forcing(self.h, A, B, float(theta), 1 if with_teq else 0), "qd_forcing")

    def simple_albedo(self, ocean_albedo=0.08):
        self.flush()
        self._chk(self.lib.qd_simple_albedo(self.h, float(ocean_albedo)), "qd_simple_albedo")

    def atmos_step(self, dt, has_albedo):
        self.flush()
        self._chk(self.lib.qd_atmos_step(self.h, float(dt), 1 if has_albedo else 0), "qd_atmos_step")

    def ocean_step(self, dt, compute_qnet, use_ice_mask, inject_sst):
        self.flush()
        self._chk(self.lib.qd_ocean_step(self.h, float(dt), int(compute_qnet), int(use_ice_mask), int(inject_sst)),
                  "qd_ocean_step")

    def driver_physics(self, dt):
        self.flush()
        self._chk(self.lib.qd_driver_physics(self.h, float(dt)), "qd_driver_physics")

    def hydrology_commit(self, dt):
        self.flush()
        self._chk(self.lib.qd_hydrology_commit(self.h, float(dt)), "qd_hydrology_commit")

    def step_n(self, stars, dt, with_ocean=False, with_physics=False, pass_albedo=True, with_hydrology=False, energy_diag=False,
               ecology=False, phyto=False, routing=None, phyto_daily=None, t0=None, eco_daily=None, budget=None, history=None):
        """benchmark_jax.py:124-158 as one resident loop (qd_step_n).  `stars`: [n][7] host
        scalars from ThermalForcing.star_table().  The span lanes, each a participant on this handle whose records stay in its
        device log until the caller has it deliver them: `routing`, a RiverRouting -- bit7, after the hydrology commit (which it
        needs); its t_accum names the event steps.  `phyto_daily`, a phyto.PhytoDaily -- bit8; its firing clock turns the span's
        times (t0 + dt * arange(n), or t0 itself when it is the n times) into the schedule.  `eco_daily`, an
        ecology.PopulationDaily -- bit9 (needs `ecology`); its day accumulator names the firing steps.  `budget`, a
        budget_diag.BudgetDiag -- no flag bit: its schedule (run-local step index, the ocean's step count) turns the lane on for
        the span.  `history`, a history.History -- no flag bit either: its window clock names the sampled steps, whose fields are
        added to the resident sums (history_read)."""
        self.flush()
        st = np.ascontiguousarray(stars, dtype=np.float64)
        assert st.ndim == 2 and st.shape[1] == 7
        n = int(st.shape[0])
        # The span's participants (csrc/qd_span.h), one protocol for all of them:
        #   dev                       the handle the lane is configured on
        #   span_clock()              -> the host clock as it stands before the span
        #   span_schedule(t0, dt, n)  advance that clock over the n steps, upload their schedule -> what _fired is to be told
        #   span_restore(clock)       nothing ran (an upload or qd_step_n raised): the clock back to what span_clock gave
        #   _fired(k)                 the span ran: k is what span_schedule returned
        #   span_deliver(dt)          drain the lane's device log and deliver it (print, keep); the caller's move, once per span
        lanes = [p for p in (phyto_daily, routing, eco_daily, budget, history) if p is not None]
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
            self._chk(self.lib.qd_step_n(self.h, n, float(dt), flags, st.ctypes.data_as(ctypes.POINTER(ctypes.c_double))), "qd_step_n")
        except Exception:
            for p, clock in zip(lanes, clocks):                               # nothing ran: every host clock back to before the call
                p.span_restore(clock)
            raise
        for p, k in zip(lanes, fired):
            p._fired(k)

    def sync(self):
        self._chk(self.lib.qd_sync(self.h), "qd_sync")

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
        self._chk(self.lib.qd_route_configure(self.h, ctypes.byref(ps), ctypes.sizeof(ps)), "qd_route_configure")
        self._route_n = (plan.n_lat * plan.n_lon, plan.n_lakes)
        self._route_last = None

    def route_free(self):
        self._chk(self.lib.qd_route_free(self.h), "qd_route_free")

    def route_reset(self):
        self._chk(self.lib.qd_route_reset(self.h), "qd_route_reset")
        self._route_last = None

    def route_accumulate(self, dt):
        self.flush()
        self._chk(self.lib.qd_route_accumulate(self.h, float(dt)), "qd_route_accumulate")

    def route_event(self, event_dt, with_pe):
        self.flush()
        self._chk(self.lib.qd_route_event(self.h, float(event_dt), 1 if with_pe else 0), "qd_route_event")

    def route_download(self, which):
        n = self._route_n[1] if which == "LAKES" else self._route_n[0]
        out = np.zeros(n, dtype=np.float64)
        self._chk(self.lib.qd_route_download(self.h, self.ROUTE_WHICH[which], out.ctypes.data_as(ctypes.POINTER(ctypes.c_double)), n),
                  "qd_route_download")
        return out

    def route_schedule(self, event_dt):
        ev = _c(event_dt)
        self._chk(self.lib.qd_route_schedule(self.h, int(ev.size), ev.ctypes.data_as(ctypes.POINTER(ctypes.c_double))), "qd_route_schedule")

    def _drain(self, fn, width, what):
        """A span lane's device log (csrc/qd_span.h) -> [n][width] records, oldest first; the log is empty afterwards."""
        buf = np.empty((_lib.SPAN_LOG_CAP, width), dtype=np.float64)
        n = ctypes.c_int32(0)
        self._chk(fn(self.h, buf.ctypes.data_as(ctypes.POINTER(ctypes.c_double)), _lib.SPAN_LOG_CAP, ctypes.byref(n)), what)
        return buf[:n.value].copy()

    def route_events(self):
        """Drain the device event log -> list of dicts (routing.LOG_KEYS), oldest first."""
        from .routing import LOG_KEYS
        out = [dict(zip(LOG_KEYS, (float(x) for x in row))) for row in self._drain(self.lib.qd_route_events, _lib.ROUTE_LOG_W, "qd_route_events")]
        if out:
            self._route_last = out[-1]
        return out

    def route_last_event(self):
        return self._route_last

    # ---- periodic budget diagnostics (qd_budget_diag.hip)
    def budget_diag_configure(self, lines, polar_row):
        pr = _c(polar_row, np.uint8)
        if pr.size != self.shape[0]:
            raise ValueError("budget_diag_configure: polar_row holds one flag per latitude row")
        self._chk(self.lib.qd_budget_diag_configure(self.h, int(lines), pr.ctypes.data_as(ctypes.POINTER(ctypes.c_uint8))),
                  "qd_budget_diag_configure")

    def budget_diag_schedule(self, fire):
        f = _c(fire, np.int32)
        self._chk(self.lib.qd_budget_diag_schedule(self.h, int(f.size), f.ctypes.data_as(ctypes.POINTER(ctypes.c_int32))), "qd_budget_diag_schedule")

    def budget_diag_log(self):
        """Drain the records -> [n][BUDGET_LOG_W] (budget_diag.REC names the slots), oldest first."""
        return self._drain(self.lib.qd_budget_diag_log, _lib.BUDGET_LOG_W, "qd_budget_diag_log")

    def budget_diag_reset(self):
        self._chk(self.lib.qd_budget_diag_reset(self.h), "qd_budget_diag_reset")

    # ---- time-mean history accumulators (qd_history.hip)
    def history_configure(self, entries):
        """entries: [(op, a, b)] with a, b field names as `get` takes them (b None for op 0): op 0 = the plane a,
        1 = sqrt(a*a + b*b).  An empty list releases the accumulators."""
        ip = ctypes.POINTER(ctypes.c_int32)
        op = _c([e[0] for e in entries], np.int32)
        a = _c([F[e[1]] for e in entries], np.int32)
        b = _c([F[e[2]] if e[2] is not None else -1 for e in entries], np.int32)
        self._chk(self.lib.qd_history_configure(self.h, len(entries), op.ctypes.data_as(ip), a.ctypes.data_as(ip), b.ctypes.data_as(ip)),
                  "qd_history_configure")
        self._history_n = len(entries)

    def history_schedule(self, sample):
        f = _c(sample, np.int32)
        self._chk(self.lib.qd_history_schedule(self.h, int(f.size), f.ctypes.data_as(ctypes.POINTER(ctypes.c_int32))), "qd_history_schedule")

    def history_sample(self):
        """One sample of every entry from the fields as they stand (the class seam)."""
        self.flush()
        self._chk(self.lib.qd_history_sample(self.h), "qd_history_sample")

    def history_read(self):
        """-> (sums [n][n_lat][n_lon], sample count)"""
        out = np.empty((self._history_n,) + self.shape, dtype=np.float64)
        n = ctypes.c_int64(0)
        self._chk(self.lib.qd_history_read(self.h, out.ctypes.data_as(ctypes.POINTER(ctypes.c_double)), ctypes.byref(n)), "qd_history_read")
        return out, int(n.value)

    def history_reset(self):
        self._chk(self.lib.qd_history_reset(self.h), "qd_history_reset")

    # ---- daily phytoplankton step (qd_phyto_daily.hip)
    def phyto_daily_configure(self, params, band_tab, species_tab, shape):
        keep = [np.ascontiguousarray(a, dtype=np.float64) for a in (band_tab, species_tab, shape)]
        dp = ctypes.POINTER(ctypes.c_double)
        self._chk(self.lib.qd_phyto_daily_configure(self.h, ctypes.byref(params), ctypes.sizeof(params),
                                                    *[a.ctypes.data_as(dp) for a in keep]), "qd_phyto_daily_configure")

    def phyto_daily(self, star_row, use_sst):
        self.flush()
        row = np.ascontiguousarray(star_row, dtype=np.float64).reshape(7)
        self._chk(self.lib.qd_phyto_daily(self.h, row.ctypes.data_as(ctypes.POINTER(ctypes.c_double)), 1 if use_sst else 0),
                  "qd_phyto_daily")

    def phyto_daily_schedule(self, fire):
        f = _c(fire, np.int32)
        self._chk(self.lib.qd_phyto_daily_schedule(self.h, int(f.size), f.ctypes.data_as(ctypes.POINTER(ctypes.c_int32))), "qd_phyto_daily_schedule")

    def phyto_daily_log(self):
        """Drain the [PhytoDiag] records -> [n][4] (daily steps so far, <C_tot>, <Kd490>, <alpha_water>)."""
        return self._drain(self.lib.qd_phyto_daily_log, _lib.PHYTO_DAILY_LOG_W, "qd_phyto_daily_log")

    def phyto_daily_bands(self, nb):
        out = np.empty((nb,) + self.shape, dtype=np.float64)
        self._chk(self.lib.qd_phyto_daily_download_bands(self.h, out.ctypes.data_as(ctypes.POINTER(ctypes.c_double)), out.size),
                  "qd_phyto_daily_download_bands")
        return out

    def phyto_daily_steps(self):
        n = ctypes.c_int64(0)
        self._chk(self.lib.qd_phyto_daily_state(self.h, ctypes.byref(n)), "qd_phyto_daily_state")
        return int(n.value)

    # ---- daily vegetation step (qd_eco_daily.hip)
    def eco_daily_configure(self, params, species_mode, species_weights):
        m, w = _c(species_mode, np.int32), _c(species_weights)
        self._chk(self.lib.qd_eco_daily_configure(self.h, ctypes.byref(params), ctypes.sizeof(params),
                                                  m.ctypes.data_as(ctypes.POINTER(ctypes.c_int32)),
                                                  w.ctypes.data_as(ctypes.POINTER(ctypes.c_double))), "qd_eco_daily_configure")

    def eco_daily_set_layers(self, layers):
        a = _c(layers)
        self._chk(self.lib.qd_eco_daily_set_layers(self.h, a.ctypes.data, int(np.prod(a.shape[:-2]))), "qd_eco_daily_set_layers")

    def eco_daily_get_layers(self, n_species, n_layers):
        out = np.empty((n_species, n_layers) + self.shape, dtype=np.float64)
        self._chk(self.lib.qd_eco_daily_get_layers(self.h, out.ctypes.data, n_species * n_layers), "qd_eco_daily_get_layers")
        return out

    def eco_daily_step(self, soil_index=None):
        """One firing now; soil_index None = from the resident W_LAND and GLACIER, as inside a span."""
        self.flush()
        a = None if soil_index is None else _c(np.broadcast_to(np.asarray(soil_index, dtype=np.float64), self.shape))
        self._chk(self.lib.qd_eco_daily_step(self.h, None if a is None else a.ctypes.data), "qd_eco_daily_step")
        for k in ("ECO_LAI", "ECO_EDAY", "ECO_AGE", "ECO_SEEDBANK", "ECO_GATE"):
            self._host.pop(k, None)

    def eco_daily_schedule(self, fire):
        f = _c(fire, np.int32)
        self._chk(self.lib.qd_eco_daily_schedule(self.h, int(f.size), f.ctypes.data_as(ctypes.POINTER(ctypes.c_int32))), "qd_eco_daily_schedule")

    def eco_daily_log(self):
        """Drain the daily vegetation records -> [n][4] (firings so far, LAI_min, LAI_mean, LAI_max over land)."""
        return self._drain(self.lib.qd_eco_daily_log, _lib.ECO_DAILY_LOG_W, "qd_eco_daily_log")

    def eco_daily_firings(self):
        n = ctypes.c_int64(0)
        self._chk(self.lib.qd_eco_daily_state(self.h, ctypes.byref(n)), "qd_eco_daily_state")
        return int(n.value)

    def eco_daily_speciate(self, parent, frac, n_species):
        """One speciation event on the resident stack of n_species species (qd_eco_speciate.hip) -> species_weights [n_species + 1]."""
        self.flush()
        out = np.empty(int(n_species) + 1, dtype=np.float64)
        self._chk(self.lib.qd_eco_daily_speciate(self.h, int(parent), float(frac), out.ctypes.data_as(ctypes.POINTER(ctypes.c_double))),
                  "qd_eco_daily_speciate")
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
        w = _c(weights)
        self._chk(self.lib.qd_eco_state_restore(self.h, a.ctypes.data, 1 if f32 else 0, w.ctypes.data_as(ctypes.POINTER(ctypes.c_double)),
                                                int(w.size), int(n_layers), float(lai_max)), "qd_eco_state_restore")
        self._host.pop("ECO_LAI", None)

    # ---- daily step of the individuals (qd_indiv_daily.hip)
    def indiv_daily_configure(self, params, species_id, level):
        s, l = _c(species_id, np.int32), _c(level, np.int32)
        ip = ctypes.POINTER(ctypes.c_int32)
        self._chk(self.lib.qd_indiv_daily_configure(self.h, ctypes.byref(params), ctypes.sizeof(params), s.ctypes.data_as(ip),
                                                    l.ctypes.data_as(ip)), "qd_indiv_daily_configure")

    def indiv_daily_step(self, soil_index=None):
        """One firing now; soil_index None = from the resident W_LAND and GLACIER, as inside a span."""
        self.flush()
        a = None if soil_index is None else _c(np.broadcast_to(np.asarray(soil_index, dtype=np.float64), self.shape))
        self._chk(self.lib.qd_indiv_daily_step(self.h, None if a is None else a.ctypes.data), "qd_indiv_daily_step")
        for k in ("ECO_LAI", "ECO_SEEDBANK"):
            self._host.pop(k, None)

    def indiv_daily_log(self):
        """Drain the individuals' daily records -> [n][4] (firings so far, beta_hint, n_cells, levels)."""
        return self._drain(self.lib.qd_indiv_daily_log, _lib.INDIV_DAILY_LOG_W, "qd_indiv_daily_log")

    def indiv_daily_weights(self, n_species):
        out = np.empty(int(n_species), dtype=np.float64)
        self._chk(self.lib.qd_indiv_daily_weights(self.h, out.ctypes.data_as(ctypes.POINTER(ctypes.c_double)), int(n_species)),
                  "qd_indiv_daily_weights")
        return out

    def indiv_daily_firings(self):
        n = ctypes.c_int64(0)
        self._chk(self.lib.qd_indiv_daily_state(self.h, ctypes.byref(n)), "qd_indiv_daily_state")
        return int(n.value)

    # ---- diversity diagnostics (qd_eco_div.hip)
    def eco_diversity(self, w_norm_row, layers=None, n_species=None, n_layers=None, land_mask=None):
        """pygcm/ecology/diversity.py on the device -> {alpha_mean, gamma_eff, beta_whittaker}; the maps stay resident
        (eco_diversity_get).  layers None: the resident stack of eco_daily_configure (n_species, n_layers name its shape); else a host
        [S, K, lat, lon] stack.  land_mask None: the ecology's land mask on the handle's grid; else the caller's mask, whose shape
        is the grid of the call (layers is then required)."""
        dp = ctypes.POINTER(ctypes.c_double)
        w = _c(w_norm_row)
        out = (ctypes.c_double * 3)()
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
            self._chk(self.lib.qd_eco_diversity_on(self.h, m.shape[0], m.shape[1], m.ctypes.data_as(ctypes.POINTER(ctypes.c_uint8)),
                                                   a.ctypes.data, int(n_species), int(n_layers), w.ctypes.data_as(dp), out),
                      "qd_eco_diversity_on")
            self._div_shape = (int(n_species),) + m.shape
        else:
            if w.shape != (self.shape[0],) or (a is not None and a.shape[2:] != self.shape):
                raise ValueError(f"eco_diversity: expected [S, K, {self.shape[0]}, {self.shape[1]}] layers and {self.shape[0]} row weights")
            self._chk(self.lib.qd_eco_diversity(self.h, None if a is None else a.ctypes.data, int(n_species), int(n_layers),
                                                w.ctypes.data_as(dp), out), "qd_eco_diversity")
            self._div_shape = (int(n_species),) + self.shape
        return {"alpha_mean": float(out[0]), "gamma_eff": float(out[1]), "beta_whittaker": float(out[2])}

    def eco_diversity_get(self, name):
        """A result of the last eco_diversity call: "ECO_DIV_LS" [S, lat, lon], "ECO_DIV_ALPHA", "ECO_DIV_BC" [lat, lon],
        "ECO_DIV_SUMMARY" [3]."""
        shp = self._div_shape
        shape = (3,) if name == "ECO_DIV_SUMMARY" else (None if shp is None else (shp if name == "ECO_DIV_LS" else shp[1:]))
        out = np.empty(shape if shape is not None else (1,), dtype=np.float64)
        self._chk(self.lib.qd_eco_diversity_download(self.h, F[name], out.ctypes.data_as(ctypes.POINTER(ctypes.c_double)), out.size),
                  "qd_eco_diversity_download")
        return out

    # ---- true-colour frame (qd_truecolor.hip)
    def truecolor_configure(self, params, eco_tab=None, phyto_tab=None, phyto_bands=None, lake_mask=None):
        """params: a _lib.qd_truecolor_params; eco_tab [7, nb_eco], phyto_tab [6, nb_phyto] (include/qingdai_hip.h); phyto_bands None =
        the resident stack of the daily phytoplankton step, else a host [nb_phyto, lat, lon] stack; lake_mask [lat, lon] or None."""
        dp, u8p = ctypes.POINTER(ctypes.c_double), ctypes.POINTER(ctypes.c_uint8)
        e = None if eco_tab is None else _c(eco_tab)
        t = None if phyto_tab is None else _c(phyto_tab)
        b = None if phyto_bands is None else _c(phyto_bands)
        m = None if lake_mask is None else _c(lake_mask, np.uint8)
        if e is not None and e.shape != (7, params.nb_eco) or t is not None and t.shape != (6, params.nb_phyto):
            raise ValueError("truecolor_configure: eco_tab must be [7, nb_eco] and phyto_tab [6, nb_phyto]")
        if b is not None and b.shape != (params.nb_phyto,) + self.shape or m is not None and m.shape != self.shape:
            raise ValueError("truecolor_configure: phyto_bands must be [nb_phyto, lat, lon] and lake_mask [lat, lon]")
        self._chk(self.lib.qd_truecolor_configure(self.h, ctypes.byref(params), ctypes.sizeof(params),
                                                  None if e is None else e.ctypes.data_as(dp), None if t is None else t.ctypes.data_as(dp),
                                                  None if b is None else b.ctypes.data_as(dp), None if m is None else m.ctypes.data_as(u8p)),
                  "qd_truecolor_configure")

    def truecolor_render(self, want_f64=False, flow=None):
        """One frame from the resident state -> (sea_ice_area, mean_h_ice); the image stays resident (truecolor_image / truecolor_rgb).
        flow None: the routing state's flow map; else a host [lat, lon] map."""
        self.flush()
        f = None if flow is None else _c(flow)
        if f is not None and f.shape != self.shape:
            raise ValueError(f"truecolor_render: flow must be {self.shape}, got {f.shape}")
        out = (ctypes.c_double * 2)()
        self._chk(self.lib.qd_truecolor_render(self.h, 1 if want_f64 else 0,
                                               None if f is None else f.ctypes.data_as(ctypes.POINTER(ctypes.c_double)), out), "qd_truecolor_render")
        return float(out[0]), float(out[1])

    def truecolor_image(self):
        """The u8 image [lat, lon, 3] of the last render, northernmost row first."""
        out = np.empty(self.shape + (3,), dtype=np.uint8)
        self._chk(self.lib.qd_truecolor_download(self.h, 0, out.ctypes.data, out.size), "qd_truecolor_download")
        return out

    def truecolor_rgb(self):
        """The unquantised f64 rgb [lat, lon, 3] in grid order of the last render (want_f64=True)."""
        out = np.empty(self.shape + (3,), dtype=np.float64)
        self._chk(self.lib.qd_truecolor_download(self.h, 1, out.ctypes.data, out.size), "qd_truecolor_download")
        return out

    # ---- 15-panel state frame (qd_stateframe.hip)
    def stateframe_configure(self, params, lake_mask=None):
        """params: a _lib.qd_stateframe_params; lake_mask [lat, lon] or None."""
        m = None if lake_mask is None else _c(lake_mask, np.uint8)
        if m is not None and m.shape != self.shape:
            raise ValueError(f"stateframe_configure: lake_mask must be {self.shape}, got {m.shape}")
        self._chk(self.lib.qd_stateframe_configure(self.h, ctypes.byref(params), ctypes.sizeof(params),
                                                   None if m is None else m.ctypes.data_as(ctypes.POINTER(ctypes.c_uint8))),
                  "qd_stateframe_configure")

    def stateframe_scan(self):
        """The extremes and the two argmax cells the level rules need, from the state as it stands -> (the STATEFRAME_SCAN_N doubles
        include/qingdai_hip.h names, [cell of star A, cell of star B]).  Also fills the vorticity plane the render reads."""
        self.flush()
        out = np.empty(_lib.STATEFRAME_SCAN_N, dtype=np.float64)
        marks = (ctypes.c_int64 * 2)()
        self._chk(self.lib.qd_stateframe_scan(self.h, out.ctypes.data_as(ctypes.POINTER(ctypes.c_double)), marks), "qd_stateframe_scan")
        return out, [int(marks[0]), int(marks[1])]

    def stateframe_render(self, table, flow=None, want_stacks=False):
        """table: a _lib.qd_stateframe_table.  flow None: the routing state's flow map; else a host [lat, lon] map.  The mosaic stays
        resident (stateframe_image / stateframe_bands / stateframe_fields)."""
        self.flush()
        f = None if flow is None else _c(flow)
        if f is not None and f.shape != self.shape:
            raise ValueError(f"stateframe_render: flow must be {self.shape}, got {f.shape}")
        self._chk(self.lib.qd_stateframe_render(self.h, ctypes.byref(table), ctypes.sizeof(table),
                                                None if f is None else f.ctypes.data_as(ctypes.POINTER(ctypes.c_double)),
                                                1 if want_stacks else 0), "qd_stateframe_render")

    def stateframe_image(self):
        """The u8 mosaic [5 lat + 6 gutters, 3 lon + 4 gutters, 3] of the last render."""
        g = _lib.STATEFRAME_GUTTER
        out = np.empty((5 * self.shape[0] + 6 * g, 3 * self.shape[1] + 4 * g, 3), dtype=np.uint8)
        self._chk(self.lib.qd_stateframe_download(self.h, 0, out.ctypes.data, out.size), "qd_stateframe_download")
        return out

    def stateframe_bands(self):
        """The int8 band indices [15, lat, lon] in grid order of the last render (want_stacks=True); -1 = white."""
        out = np.empty((_lib.STATEFRAME_PANELS,) + self.shape, dtype=np.int8)
        self._chk(self.lib.qd_stateframe_download(self.h, 1, out.ctypes.data, out.size), "qd_stateframe_download")
        return out

    def stateframe_fields(self):
        """The f64 fields [15, lat, lon] handed to the band search by the last render (want_stacks=True)."""
        out = np.empty((_lib.STATEFRAME_PANELS,) + self.shape, dtype=np.float64)
        self._chk(self.lib.qd_stateframe_download(self.h, 2, out.ctypes.data, out.size), "qd_stateframe_download")
        return out

    # ---- tiles of the ecology / plankton / ISR figures (qd_tiles.hip)
    def tiles_configure(self, height_scale=10.0, layers=None):
        """height_scale: QD_ECO_HEIGHT_SCALE_M.  layers None: the stack sources read the resident stack of eco_daily_configure; else a
        host [S, K, lat, lon] stack, uploaded here."""
        a = None if layers is None else _c(layers)
        if a is not None and (a.ndim != 4 or a.shape[2:] != self.shape):
            raise ValueError(f"tiles_configure: layers must be [S, K, {self.shape[0]}, {self.shape[1]}], got {a.shape}")
        self._chk(self.lib.qd_tiles_configure(self.h, float(height_scale), None if a is None else a.ctypes.data_as(ctypes.POINTER(ctypes.c_double)),
                                              0 if a is None else a.shape[0], 0 if a is None else a.shape[1]), "qd_tiles_configure")

    def tiles_set_plane(self, plane):
        """A host [lat, lon] map for the tile source "HOST_PLANE" (kept until the next tiles_configure)."""
        a = _c(plane)
        if a.shape != self.shape:
            raise ValueError(f"tiles_set_plane: plane must be {self.shape}, got {a.shape}")
        self._chk(self.lib.qd_tiles_set_plane(self.h, a.ctypes.data_as(ctypes.POINTER(ctypes.c_double))), "qd_tiles_set_plane")

    def tiles_available(self):
        """-> (an LAI map, a scalar alpha map, a banded alpha map) are on the device."""
        out = (ctypes.c_int32 * 3)()
        self._chk(self.lib.qd_tiles_available(self.h, out), "qd_tiles_available")
        return bool(out[0]), bool(out[1]), bool(out[2])

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
        out = np.empty((max(1, n), 4), dtype=np.float64)
        cells = (ctypes.c_int64 * max(1, n))()
        self._chk(self.lib.qd_tiles_scan(self.h, self._tile_refs(refs), n, out.ctypes.data_as(ctypes.POINTER(ctypes.c_double)), cells), "qd_tiles_scan")
        return [{"min": float(out[k, 0]), "max": float(out[k, 1]), "nan": bool(out[k, 2] > 0.0), "argmax": int(cells[k]),
                 "argmax_value": float(out[k, 3])} for k in range(n)]

    def tiles_order_stats(self, source, index, ranks):
        """-> (count of non-NaN cells, [the ranks[k]-th smallest of them, 0-based]); NaN for a rank that is not below the count."""
        self.flush()
        r = (ctypes.c_int64 * max(1, len(ranks)))(*[int(x) for x in ranks])
        vals = np.full(max(1, len(ranks)), np.nan, dtype=np.float64)
        count = ctypes.c_int64(-1)
        self._chk(self.lib.qd_tiles_order_stats(self.h, _lib.TILE[source] if isinstance(source, str) else int(source), int(index), r, len(ranks),
                                                vals.ctypes.data_as(ctypes.POINTER(ctypes.c_double)), ctypes.byref(count)), "qd_tiles_order_stats")
        return int(count.value), vals[:len(ranks)]

    def tiles_render(self, tiles, want_stacks=False):
        """tiles: a sequence of _lib.qd_tile_desc (one row, at most 8).  The mosaic stays resident (tiles_image / tiles_bands /
        tiles_planes)."""
        self.flush()
        n = len(tiles)
        arr = (_lib.qd_tile_desc * max(1, n))(*tiles)
        self._chk(self.lib.qd_tiles_render(self.h, arr, ctypes.sizeof(_lib.qd_tile_desc), n, 1 if want_stacks else 0), "qd_tiles_render")
        self._tiles_n = n

    def tiles_image(self):
        """The u8 mosaic [lat + 2 gutters, n lon + (n + 1) gutters, 3] of the last render."""
        g, n = _lib.STATEFRAME_GUTTER, self._tiles_n
        out = np.empty((self.shape[0] + 2 * g, n * self.shape[1] + (n + 1) * g, 3), dtype=np.uint8)
        self._chk(self.lib.qd_tiles_download(self.h, 0, out.ctypes.data, out.size), "qd_tiles_download")
        return out

    def tiles_bands(self):
        """The int8 band indices [n, lat, lon] of the last render (want_stacks=True); -1 = white."""
        out = np.empty((self._tiles_n,) + self.shape, dtype=np.int8)
        self._chk(self.lib.qd_tiles_download(self.h, 1, out.ctypes.data, out.size), "qd_tiles_download")
        return out

    def tiles_planes(self):
        """The f64 planes [n, lat, lon] handed to the band search by the last render (want_stacks=True)."""
        out = np.empty((self._tiles_n,) + self.shape, dtype=np.float64)
        self._chk(self.lib.qd_tiles_download(self.h, 2, out.ctypes.data, out.size), "qd_tiles_download")
        return out

    # ---- phytoplankton tracers carried by the ocean currents (pygcm/ecology/phyto.py:496-547), resident
    def phyto_configure(self, n_species, K_h, adv_alpha):
        self._chk(self.lib.qd_phyto_configure(self.h, int(n_species), float(K_h), float(adv_alpha)), "qd_phyto_configure")
        self._phyto_S = int(n_species)

    def phyto_upload(self, C_s):
        C_s = np.ascontiguousarray(C_s, dtype=np.float64)
        assert C_s.ndim == 3 and C_s.shape[0] == getattr(self, "_phyto_S", -1) and C_s.shape[1:] == self.shape
        for s in range(C_s.shape[0]):
            self._chk(self.lib.qd_phyto_upload(self.h, s, C_s[s].ctypes.data), "qd_phyto_upload")

    def phyto_download(self):
        self.flush()
        out = np.zeros((self._phyto_S,) + self.shape, dtype=np.float64)
        for s in range(self._phyto_S):
            self._chk(self.lib.qd_phyto_download(self.h, s, out[s].ctypes.data), "qd_phyto_download")
        return out

    def phyto_advect_diffuse(self, dt_seconds):
        """PhytoManager.advect_diffuse on the resident tracers and the resident uo / vo (three launches for all species)."""
        self.flush()
        self._chk(self.lib.qd_phyto_advect_diffuse(self.h, float(dt_seconds)), "qd_phyto_advect_diffuse")

    def last_ocean_nsub(self):
        n = ctypes.c_int(0)
        self.lib.qd_last_ocean_nsub(self.h, ctypes.byref(n))
        return n.value

    def step_scalars(self):
        """The device scalars a step's launches hand to each other (include/qingdai_hip.h: qd_step_scalars), by name."""
        out = np.zeros(8)
        self._chk(self.lib.qd_step_scalars(self.h, out.ctypes.data_as(ctypes.POINTER(ctypes.c_double))), "qd_step_scalars")
        return dict(zip(("PREF", "ETA_MEAN", "MED_OUT", "PSCALE", "RENORM", "BLEND_W", "TMP0", "TMP1"), out))

    def ocean_mean_next_count(self):
        """Ocean sub-steps since create whose eta mean the next momentum launch finished (QD_MEAN_IN_MOMENTUM)."""
        n = ctypes.c_int64(0)
        self._chk(self.lib.qd_ocean_mean_next_count(self.h, ctypes.byref(n)), "qd_ocean_mean_next_count")
        return n.value

    def counters(self):
        a, o = ctypes.c_int64(0), ctypes.c_int64(0)
        self.lib.qd_get_step_counter(self.h, ctypes.byref(a), ctypes.byref(o))
        return a.value, o.value

    def set_counters(self, a, o):
        self.lib.qd_set_step_counter(self.h, int(a), int(o))

    # ---- state digest and the scalars of an exact resume (qd_digest.hip)
    def digest(self, names):
        """The 64-bit digests of resident planes (include/qingdai_hip.h: qd_state_digest), one launch per 64 of them -> np.uint64[n].
        names: what _lib.state_ref takes -- field names, LAND_MASK, ICE_MASK, ROUTE_BUFFER, ROUTE_FLOW, ROUTE_LAKES, ECO_LAI_STACK,
        INDIV_E_DAY, INDIV_STRESS, "PHYTO_TRACER:s", "HISTORY_SUM:k".  A plane whose subsystem is not configured raises."""
        self.flush()
        refs = _c([_lib.state_ref(n) for n in names], np.int32)
        out = np.zeros(refs.size, dtype=np.uint64)
        for k in range(0, int(refs.size), _lib.STATE_DIGEST_MAX):
            r, o = refs[k:k + _lib.STATE_DIGEST_MAX], out[k:k + _lib.STATE_DIGEST_MAX]
            self._chk(self.lib.qd_state_digest(self.h, int(r.size), r.ctypes.data_as(ctypes.POINTER(ctypes.c_int32)),
                                               o.ctypes.data_as(ctypes.POINTER(ctypes.c_uint64))), "qd_state_digest")
        return out

    def state_scalars(self):
        """The host-side scalars a step reads besides the planes and the step counters -> float64[STATE_SCALARS_N]."""
        out = np.zeros(_lib.STATE_SCALARS_N, dtype=np.float64)
        self._chk(self.lib.qd_state_scalars_get(self.h, out.ctypes.data_as(ctypes.POINTER(ctypes.c_double)), int(out.size)), "qd_state_scalars_get")
        return out

    def set_state_scalars(self, values):
        v = _c(values)
        self._chk(self.lib.qd_state_scalars_set(self.h, v.ctypes.data_as(ctypes.POINTER(ctypes.c_double)), int(v.size)), "qd_state_scalars_set")

    def route_restore(self, buffer, flow, lakes, steps):
        """The inverse of route_download("BUFFER" / "FLOW" / "LAKES") plus the accumulation count."""
        dp = ctypes.POINTER(ctypes.c_double)
        b, f = _c(buffer).ravel(), _c(flow).ravel()
        lk = None if lakes is None or np.size(lakes) == 0 else _c(lakes).ravel()
        if b.size != self._route_n[0] or f.size != self._route_n[0] or (0 if lk is None else lk.size) != self._route_n[1]:
            raise ValueError("route_restore: the arrays do not have the configured network's cell and lake counts")
        self._chk(self.lib.qd_route_restore(self.h, b.ctypes.data_as(dp), f.ctypes.data_as(dp), None if lk is None else lk.ctypes.data_as(dp),
                                            int(steps)), "qd_route_restore")

    def history_restore(self, sums, count):
        """The inverse of history_read: an open window's sums [n][n_lat][n_lon] and its sample count."""
        a = _c(sums)
        if a.shape != (self._history_n,) + self.shape:
            raise ValueError(f"history_restore: expected sums of shape {(self._history_n,) + self.shape}, got {a.shape}")
        self._chk(self.lib.qd_history_restore(self.h, a.ctypes.data_as(ctypes.POINTER(ctypes.c_double)), int(count)), "qd_history_restore")

    def reduce(self, name, op):
        self.flush()
        out = ctypes.c_double(0.0)
        self._chk(self.lib.qd_reduce(self.h, F[name], int(op), ctypes.byref(out)), "qd_reduce")
        return out.value

    # ---- timing hooks
    def timing(self, on=True, select=None):
        if select:
            self.lib.qd_timing_select(self.h, select.encode())
        else:
            self.lib.qd_timing_enable(self.h, 1 if on else 0)
        self.lib.qd_timing_reset(self.h)

    def timing_get(self, name):
        ms, n = ctypes.c_double(0), ctypes.c_int64(0)
        self.lib.qd_timing_get(self.h, name.encode(), ctypes.byref(ms), ctypes.byref(n))
        return ms.value, n.value

    # ---- operator seam (jax_compat.py:111-216): host in, host out
    def _out(self):
        return np.empty(self.shape, dtype=np.float64)

    def op_laplacian(self, Fh, ocean=False):
        a, out = _c(Fh), self._out()
        self._chk(self.lib.qd_op_laplacian(self.h, a.ctypes.data, 1 if ocean else 0, out.ctypes.data), "qd_op_laplacian")
        return out

    def op_hyperdiffuse(self, Fh, k4, dt, n_substeps=1, ocean=False):
        a, out = _c(Fh), self._out()
        if np.isscalar(k4):
            rc = self.lib.qd_op_hyperdiffuse(self.h, a.ctypes.data, None, float(k4), float(dt), int(n_substeps),
                                             1 if ocean else 0, out.ctypes.data)
        else:
            k = np.asarray(k4, dtype=np.float64)
            if k.ndim == 2:          # the reference's maps are constant along longitude
                if not np.all(k == k[:, :1]):
                    raise ValueError("k4 map must be a function of latitude only")
                k = k[:, 0]
            k = _c(k)
            rc = self.lib.qd_op_hyperdiffuse(self.h, a.ctypes.data, k.ctypes.data, 0.0, float(dt), int(n_substeps),
                                             1 if ocean else 0, out.ctypes.data)
        self._chk(rc, "qd_op_hyperdiffuse")
        return out

    def op_advect(self, field, u, v, dt, ocean=False):
        a, uu, vv, out = _c(field), _c(u), _c(v), self._out()
        self._chk(self.lib.qd_op_advect(self.h, a.ctypes.data, uu.ctypes.data, vv.ctypes.data, float(dt),
                                        1 if ocean else 0, out.ctypes.data), "qd_op_advect")
        return out

    def op_shapiro(self, Fh, n=2):
        a, out = _c(Fh), self._out()
        self._chk(self.lib.qd_op_shapiro(self.h, a.ctypes.data, int(n), out.ctypes.data), "qd_op_shapiro")
        return out

    ENERGY_DIAG_KEYS = ("TOA_net", "SFC_net", "ATM_net", "I_mean", "R_mean", "OLR_mean", "SW_sfc_mean", "LW_sfc_mean",
                        "SH_mean", "LH_mean")

    def energy_diagnostics(self):
        """energy.compute_energy_diagnostics (energy.py:494-538) of the resident state -> dict of global means."""
        self.flush()
        out = (ctypes.c_double * 10)()
        self._chk(self.lib.qd_energy_diagnostics(self.h, out), "qd_energy_diagnostics")
        return dict(zip(self.ENERGY_DIAG_KEYS, [float(x) for x in out]))

    def copy_ceiling(self, nbytes=1 << 30, reps=8):
        """Measured device-to-device streaming rate in GB/s (read + written bytes), past the Infinity Cache by default."""
        out = ctypes.c_double(0.0)
        self._chk(self.lib.qd_copy_ceiling(self.h, int(nbytes), int(reps), ctypes.byref(out)), "qd_copy_ceiling")
        return out.value

    def energy_diagnostics_last(self):
        """The means taken inside the last step_n(..., energy_diag=True): first step, after time_step, before the ocean."""
        out = (ctypes.c_double * 10)()
        self._chk(self.lib.qd_energy_diagnostics_last(self.h, out), "qd_energy_diagnostics_last")
        return dict(zip(self.ENERGY_DIAG_KEYS, [float(x) for x in out]))

    def op_zonal_filter(self, Fh, cutoff=0.75, damp=0.5):
        """SpectralModel._spectral_zonal_filter (dynamics.py:233-258)."""
        a, out = _c(Fh), self._out()
        self._chk(self.lib.qd_op_zonal_filter(self.h, a.ctypes.data, float(cutoff), float(damp), out.ctypes.data), "qd_op_zonal_filter")
        return out

    def op_divvort(self, u, v, vort=False):
        uu, vv, out = _c(u), _c(v), self._out()
        fn = self.lib.qd_op_vorticity if vort else self.lib.qd_op_divergence
        self._chk(fn(self.h, uu.ctypes.data, vv.ctypes.data, out.ctypes.data), "qd_op_div/vort")
        return out

    def op_gaussian(self, Fh, sigma, mode="reflect"):
        a, out = _c(Fh), self._out()
        self._chk(self.lib.qd_op_gaussian(self.h, a.ctypes.data, float(sigma), 1 if mode == "wrap" else 0,
                                          out.ctypes.data), "qd_op_gaussian")
        return out

    def op_median_positive(self, x, default):
        a = _c(x)
        out = ctypes.c_double(0.0)
        self._chk(self.lib.qd_op_median_positive(self.h, a.ctypes.data, float(default), ctypes.byref(out)),
                  "qd_op_median_positive")
        return out.value
