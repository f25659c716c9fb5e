"""
qingdai_amd/routing.py -- river routing (P014, pygcm/routing.py) on the device.

The reference routes the land runoff along an offline D8 network with a sequential loop over `flow_order`
(routing.py:226-278).  That loop is a forest accumulation, and it is scheduled here without changing one f64
addition:

  * every cell gets its position p in `flow_order` and a target (a land cell, OCEAN, LAKE k, VOID, or DEAD:
    a delivery that ends as residual).  An edge u -> t is LIVE only when t is processed later, p(t) > p(u);
    everything else the sequential loop leaves in `acc` as residual (or, for t == u, wipes).  Live edges point
    forward in p, so they form a forest.
  * pull form: m(c) = (buf(c) + m(u1)) + m(u2) + ... over the live predecessors sorted by p, counting only
    those with m > 0 -- the reference's own additions in its own order, so the flow map is bit-identical.
  * the forest is cut into SEGMENTS (chains in which every cell but the head has exactly one live predecessor)
    ordered by junction level: one lane walks a segment at register speed, one barrier per junction level.

`build_plan` runs once per network (NumPy); `RiverRouting` uploads the plan to a device handle and runs the
accumulation and the events there (qingdai_amd/csrc/qd_route.hip).  Networks the reference cannot run (it would
raise) and networks with duplicate `flow_order` entries are refused with ValueError.
"""
from __future__ import annotations

import os
from dataclasses import dataclass
from typing import Dict, Optional

import numpy as np

from .params import PLANET_RADIUS

# target codes (qd_route.hip): >= 0 a live edge to that cell
T_OCEAN, T_VOID, T_DEAD, T_NOTPROC, T_LAKE0 = -1, -2, -3, -4, -5

LOG_KEYS = ("step", "event_dt", "ocean_inflow_kgps", "mass_closure_error_kg", "mass_input_kg", "ocean_kg", "residual_kg",
            "lake_delta_kg")                   # one event record of the device log: _lib.ROUTE_LOG_W doubles


@dataclass
class RoutingNetwork:
    """What pygcm/routing.py:108-163 makes of a network file, validated."""
    shape: tuple
    land_mask: np.ndarray            # (n_lat, n_lon) uint8
    flow_to_index: np.ndarray        # (n_cells,) int64
    flow_order: np.ndarray           # (n_order,) int64
    lake_mask: Optional[np.ndarray]
    lake_id: Optional[np.ndarray]
    lake_outlet_index: Optional[np.ndarray]
    n_lakes: int

    @property
    def has_lakes(self):
        return self.lake_mask is not None and self.lake_id is not None and self.n_lakes > 0


def network_from_vars(v: Dict[str, np.ndarray], shape) -> RoutingNetwork:
    """The reference constructor's reading of the variables (routing.py:108-163): the fallback order, the two
    outlet forms and the n_lakes coercion.  Raises ValueError for what the reference could not run."""
    n_lat, n_lon = shape
    n_cells = n_lat * n_lon
    if v.get("land_mask") is None:
        raise ValueError("hydrology network: missing 'land_mask' variable")
    land_mask = (np.asarray(v["land_mask"]) > 0).astype(np.uint8)
    if land_mask.shape != tuple(shape):
        raise ValueError(f"hydrology network: land_mask shape {land_mask.shape} != grid shape {tuple(shape)}")
    flow_to = v.get("flow_to_index")
    if flow_to is None:
        raise ValueError("hydrology network: missing 'flow_to_index' variable")
    flow_to = np.asarray(flow_to)
    if flow_to.shape != tuple(shape):
        raise ValueError(f"hydrology network: flow_to_index shape {flow_to.shape} != grid shape {tuple(shape)}")
    flow_to = flow_to.astype(np.int64).ravel()
    order = v.get("flow_order")
    if order is None:
        order = np.where(land_mask.ravel() == 1)[0].astype(np.int64)        # routing.py:125-129
    else:
        order = np.asarray(order).astype(np.int64).ravel()
    if order.size and (order.min() < 0 or order.max() >= n_cells):
        raise ValueError("hydrology network: flow_order holds indices outside the grid")
    if np.unique(order).size != order.size:
        raise ValueError("hydrology network: flow_order holds duplicate cells")
    lake_mask = v.get("lake_mask")
    lake_id = v.get("lake_id")
    for name, a in (("lake_mask", lake_mask), ("lake_id", lake_id)):
        if a is not None and np.asarray(a).shape != tuple(shape):
            raise ValueError(f"hydrology network: {name} shape {np.asarray(a).shape} != grid shape {tuple(shape)}")
    outlet = v.get("lake_outlet_index")
    if outlet is None and v.get("lake_outlet_i") is not None and v.get("lake_outlet_j") is not None:
        outlet = np.asarray(v["lake_outlet_j"]).astype(np.int64) * n_lon + np.asarray(v["lake_outlet_i"]).astype(np.int64)
    if outlet is not None:
        outlet = np.asarray(outlet).astype(np.int64).ravel()
    n_lakes = 0
    if lake_id is not None:
        lake_id = np.asarray(lake_id)
        if not np.all(np.isfinite(lake_id)):
            raise ValueError("hydrology network: lake_id holds non-finite values")
        n_lakes = int(np.max(lake_id))
    if n_lakes > 0 and outlet is not None and outlet.shape[0] != n_lakes:
        n_lakes = min(n_lakes, outlet.shape[0])                              # routing.py:158-162
        outlet = outlet[:n_lakes]
    return RoutingNetwork(tuple(shape), land_mask, flow_to, order, None if lake_mask is None else np.asarray(lake_mask),
                          lake_id, outlet, n_lakes)


def cell_area_rows(grid) -> np.ndarray:
    """routing.py:168-196: A = R^2 dlam (sin phi+ - sin phi-) per row, in the reference's operation order."""
    n_lat, n_lon = int(grid.n_lat), int(grid.n_lon)
    R = float(PLANET_RADIUS)
    lats = np.asarray(grid.lat, dtype=float)
    lons = np.asarray(grid.lon, dtype=float)
    dphi = np.deg2rad(abs(lats[1] - lats[0])) if n_lat > 1 else np.deg2rad(1.5)
    dlam = np.deg2rad(abs(lons[1] - lons[0])) if n_lon > 1 else np.deg2rad(1.5)
    phi_cent = np.deg2rad(np.asarray(grid.lat_mesh)[:, 0])
    phi_plus = np.clip(phi_cent + 0.5 * dphi, -0.5 * np.pi, 0.5 * np.pi)
    phi_minus = np.clip(phi_cent - 0.5 * dphi, -0.5 * np.pi, 0.5 * np.pi)
    return (R * R) * dlam * (np.sin(phi_plus) - np.sin(phi_minus))


@dataclass
class RoutingPlan:
    """The device plan: everything qd_route_configure uploads."""
    n_lat: int
    n_lon: int
    cflags: np.ndarray        # (n_cells,) uint8: bit0 network land, bit1 lake cell of the P-E update (lake_mask != 0)
    area_row: np.ndarray      # (n_lat,) f64
    code: np.ndarray          # (n_cells,) int32: live target cell, or T_* (LAKE k = T_LAKE0 - k)
    seg_start: np.ndarray     # (n_seg + 1,) int32 into seg_cells; segments ordered by junction level
    seg_cells: np.ndarray     # int32, each segment head first
    level_start: np.ndarray   # (n_levels + 1,) int32 into the segments
    jp_start: np.ndarray      # (n_seg + 1,) int32 into jp_cells: the live predecessors of each segment's head, sorted by p
    jp_cells: np.ndarray      # int32
    lake_start: np.ndarray    # (n_lakes + 1,) int32 into lake_cells: the cells that drain into lake storage k, sorted by p
    lake_cells: np.ndarray    # int32
    lake_frac: np.ndarray     # (n_lakes,) f64: the P-E split (routing.py:289-296)
    n_lakes: int              # lake storages (0: lake_volume_kg is None)
    pe_lakes: int             # 1: the lake P-E update runs when P and E are given

    @property
    def n_levels(self):
        return len(self.level_start) - 1


def _targets(net: RoutingNetwork):
    """-> (pos, target) per cell: pos = position in flow_order (-1: never processed); target a cell index or T_*."""
    n_cells = net.land_mask.size
    land_flat = net.land_mask.ravel() == 1
    order = net.flow_order
    pos = np.full(n_cells, -1, dtype=np.int64)
    pos[order] = np.arange(order.size, dtype=np.int64)
    tgt = np.full(n_cells, T_NOTPROC, dtype=np.int64)
    # normal land cells (routing.py:266-276)
    dn = net.flow_to_index[order]
    if np.any(dn >= n_cells):
        bad = dn >= n_cells
        is_lake = np.zeros(order.size, bool)
        if net.has_lakes:
            is_lake = net.lake_mask.ravel()[order] > 0
        if np.any(bad & ~is_lake):
            raise ValueError("hydrology network: flow_to_index points outside the grid for a routed cell")
    dn_c = np.clip(dn, 0, n_cells - 1)
    t = np.where((dn < 0) | ~land_flat[dn_c], T_OCEAN, dn)
    if net.has_lakes:
        lake_is = net.lake_mask.ravel()[order] > 0
        lid = np.trunc(np.asarray(net.lake_id, dtype=float).ravel()[order]).astype(np.int64)
        out = net.lake_outlet_index
        has_out = (lid > 0) & (out is not None) & (lid <= (0 if out is None else out.shape[0]))
        o = np.full(order.size, -1, dtype=np.int64)
        if out is not None and out.size:
            o[has_out] = out[lid[has_out] - 1]
        o_c = np.clip(o, 0, n_cells - 1)
        to_cell = has_out & (o >= 0) & (o < n_cells) & land_flat[o_c]
        lt = np.where(to_cell, o, T_OCEAN)                                       # routing.py:245-256
        store = ~has_out & (lid > 0)                                             # routing.py:257-260
        if np.any(lake_is & store & (lid > net.n_lakes)):
            raise ValueError("hydrology network: a lake cell names a lake id beyond the lake storages (the reference "
                             "would index lake_volume out of range)")
        lt = np.where(store, T_LAKE0 - (lid - 1), lt)
        lt = np.where(~has_out & ~store, T_VOID, lt)
        t = np.where(lake_is, lt, t)
    # a delivery to the cell itself is wiped (acc[idx] = 0 follows acc[dn] += m); one to a cell processed
    # earlier, or never, stays there as residual
    cell = t >= 0
    tc = np.clip(t, 0, n_cells - 1)
    t = np.where(cell & (tc == order), T_VOID, t)
    cell = t >= 0
    t = np.where(cell & (pos[tc] <= np.arange(order.size)), T_DEAD, t)
    tgt[order] = t
    return pos, tgt


def build_plan(net: RoutingNetwork, area_row: np.ndarray) -> RoutingPlan:
    n_lat, n_lon = net.shape
    n_cells = n_lat * n_lon
    pos, tgt = _targets(net)
    order = net.flow_order
    live = tgt >= 0
    npred = np.bincount(tgt[live], minlength=n_cells)
    # live predecessors of every cell, sorted by p (CSR over cells); flow_order is already p order
    src = order[live[order]]
    dst = tgt[src]
    k = np.argsort(dst, kind="stable")           # stable: predecessors of a cell stay in p order
    pred_cells = src[k]
    pred_start = np.zeros(n_cells + 1, dtype=np.int64)
    np.cumsum(np.bincount(dst, minlength=n_cells), out=pred_start[1:])
    # segments: heads are processed cells with != 1 live predecessor, walked in p order
    heads = order[npred[order] != 1]
    seg_of = np.full(n_cells, -1, dtype=np.int64)
    tgt_l = tgt.tolist()
    npred_l = npred.tolist()
    seg_cells, seg_start, seg_level = [], [0], []
    ps, pc = pred_start.tolist(), pred_cells.tolist()
    seg_of_l = seg_of.tolist()
    for h in heads.tolist():
        s = len(seg_level)
        lev = 0
        for i in range(ps[h], ps[h + 1]):
            lev = max(lev, seg_level[seg_of_l[pc[i]]] + 1)
        seg_level.append(lev)
        c = h
        while True:
            seg_cells.append(c)
            seg_of_l[c] = s
            t = tgt_l[c]
            if t < 0 or npred_l[t] != 1:
                break
            c = t
        seg_start.append(len(seg_cells))
    if len(seg_cells) != order.size:
        raise AssertionError("routing plan: segments do not cover flow_order")
    seg_level = np.asarray(seg_level, dtype=np.int64)
    seg_start = np.asarray(seg_start, dtype=np.int64)
    seg_cells = np.asarray(seg_cells, dtype=np.int64)
    n_seg = seg_level.size
    # order the segments by level (stable), lay their cells out contiguously
    so = np.argsort(seg_level, kind="stable")
    lens = np.diff(seg_start)
    new_start = np.zeros(n_seg + 1, dtype=np.int64)
    np.cumsum(lens[so], out=new_start[1:])
    new_cells = np.concatenate([seg_cells[seg_start[s]:seg_start[s + 1]] for s in so]) if n_seg else np.zeros(0, np.int64)
    n_levels = int(seg_level.max()) + 1 if n_seg else 0
    level_start = np.zeros(n_levels + 1, dtype=np.int64)
    np.cumsum(np.bincount(seg_level, minlength=n_levels), out=level_start[1:])
    heads_sorted = new_cells[new_start[:-1]] if n_seg else np.zeros(0, np.int64)
    jl = pred_start[heads_sorted + 1] - pred_start[heads_sorted]
    jp_start = np.zeros(n_seg + 1, dtype=np.int64)
    np.cumsum(jl, out=jp_start[1:])
    jp_cells = (np.concatenate([pred_cells[pred_start[h]:pred_start[h + 1]] for h in heads_sorted])
                if n_seg else np.zeros(0, np.int64))
    # lake storages, the P-E split
    n_store = max(net.n_lakes, 0)
    lk = (tgt <= T_LAKE0)
    lake_src = order[lk[order]]
    lake_k = T_LAKE0 - tgt[lake_src]
    kk = np.argsort(lake_k, kind="stable")
    lake_cells = lake_src[kk]
    lake_start = np.zeros(n_store + 1, dtype=np.int64)
    if n_store:
        np.cumsum(np.bincount(lake_k, minlength=n_store), out=lake_start[1:])
    cflags = (net.land_mask.ravel() == 1).astype(np.uint8)
    lake_frac = np.zeros(n_store, dtype=np.float64)
    pe = 0
    if net.has_lakes:
        A = np.repeat(np.asarray(area_row, dtype=float)[:, None], n_lon, axis=1)
        lake_mask_bool = net.lake_mask.astype(bool)
        cflags |= (lake_mask_bool.ravel().astype(np.uint8) << 1)
        pe = 1
        # routing.py:291-295 (per lake a pass over the grid there; one pass here, summed in another order: last bits only)
        ids = np.asarray(net.lake_id).ravel()
        sel = (ids == np.trunc(ids)) & (ids >= 1) & (ids <= net.n_lakes)
        lake_area = np.bincount(ids[sel].astype(np.int64) - 1, weights=A.ravel()[sel], minlength=net.n_lakes)[:net.n_lakes]
        total = np.sum(np.where(lake_mask_bool, A, 0.0))
        with np.errstate(divide="ignore", invalid="ignore"):
            lake_frac[:] = np.where(lake_area <= 0, 0.0, lake_area / total)
    i32 = lambda a: np.ascontiguousarray(a, dtype=np.int32)
    return RoutingPlan(n_lat, n_lon, np.ascontiguousarray(cflags), np.ascontiguousarray(area_row, dtype=np.float64),
                       i32(tgt), i32(new_start), i32(new_cells), i32(level_start), i32(jp_start), i32(jp_cells),
                       i32(lake_start), i32(lake_cells), lake_frac, n_store, pe)


@dataclass
class RoutingDiagnostics:
    flow_accum_kgps: np.ndarray
    ocean_inflow_kgps: float
    mass_closure_error_kg: float
    lake_volume_kg: Optional[np.ndarray] = None


class RiverRouting:
    """pygcm/routing.py:RiverRouting with the accumulation and the events on the device.

    `dev`: the Device (qd_handle) to run on -- a whole-globe handle of the same grid; by default the one the grid
    already carries (its model's), else a fresh one.  `step` uploads its arguments into that handle's RUNOFF /
    PRECIP / EFLUX fields (the class seam); the resident loop passes `routing=` to Device.step_n instead.
    """

    def __init__(self, grid, network_nc_path, dt_hydro_hours=6.0, treat_lake_as_water=True, alpha_lake=None, diag=True,
                 dev=None, _vars=None):
        if _vars is None:
            if not os.path.exists(network_nc_path):
                raise FileNotFoundError(f"Hydrology network file not found: {network_nc_path}")
            from .ncio import read_nc
            _vars, _ = read_nc(network_nc_path, ["land_mask", "flow_to_index", "flow_order", "lake_mask", "lake_id",
                                                  "lake_outlet_index", "lake_outlet_i", "lake_outlet_j"])
        self.grid = grid
        self.dt_hydro_seconds = float(dt_hydro_hours) * 3600.0
        self.treat_lake_as_water = bool(treat_lake_as_water)
        self.alpha_lake = alpha_lake
        self.diag_enabled = bool(diag)
        self.n_lat, self.n_lon = int(grid.n_lat), int(grid.n_lon)
        self.shape = (self.n_lat, self.n_lon)
        self.n_cells = self.n_lat * self.n_lon
        self.net = network_from_vars(_vars, self.shape)
        self.land_mask = self.net.land_mask
        self.flow_order = self.net.flow_order
        self.n_lakes = self.net.n_lakes
        self.cell_area = np.repeat(cell_area_rows(grid)[:, None], self.n_lon, axis=1)
        self.plan = build_plan(self.net, self.cell_area[:, 0])
        if dev is None:
            dev = getattr(grid, "_device", None)
            if dev is None:
                from .device import Device
                dev = Device(grid)
        self.dev = dev
        dev.route_configure(self.plan)
        self.t_accum = 0.0
        self._steps = 0
        self._have_event = False
        self._last = None
        if self.diag_enabled:
            print(f"[Routing] Loaded network: land={int(self.land_mask.sum())} cells, "
                  f"n_lakes={self.n_lakes}, dt_hydro={self.dt_hydro_seconds/3600.0:.1f} h")

    @classmethod
    def from_arrays(cls, grid, land_mask, flow_to_index, flow_order=None, lake_mask=None, lake_id=None,
                    lake_outlet_index=None, lake_outlet_i=None, lake_outlet_j=None, **kw):
        v = dict(land_mask=land_mask, flow_to_index=flow_to_index, flow_order=flow_order, lake_mask=lake_mask,
                 lake_id=lake_id, lake_outlet_index=lake_outlet_index, lake_outlet_i=lake_outlet_i, lake_outlet_j=lake_outlet_j)
        return cls(grid, None, _vars={k: a for k, a in v.items() if a is not None}, **kw)

    def close(self):
        if getattr(self, "dev", None) is not None and getattr(self.dev, "h", None):
            self.dev.route_free()
        self.dev = None

    # ---- the host's event schedule (routing.py:214-219, the reference's float test)
    def schedule(self, dt_seconds, n):
        """-> per-step event_dt (0: no event) for n steps of dt, advancing t_accum as the reference does."""
        ev = np.zeros(n, dtype=np.float64)
        for s in range(n):
            self.t_accum += float(dt_seconds)
            if not (self.t_accum + 1e-9 < self.dt_hydro_seconds):
                ev[s] = self.t_accum
                self.t_accum = 0.0
        self._steps += n
        return ev

    # ---- span participant (the protocol is stated in Device.step_n)
    def span_clock(self):
        return self.t_accum, self._steps

    def span_schedule(self, t0, dt, n):
        self.dev.route_schedule(self.schedule(dt, n))

    def span_restore(self, clock):
        self.t_accum, self._steps = clock

    def _fired(self, k):
        pass                                   # schedule() has already counted the span's steps

    def span_deliver(self, dt):
        self.take_events(self.dev.route_events())      # the span's events, oldest first

    def step(self, R_land_flux, dt_seconds, precip_flux=None, evap_flux=None):
        """routing.py:199-312 on host arrays: upload, accumulate on the device, route when the window is full."""
        R = np.asarray(R_land_flux, dtype=float)
        if R.shape != self.shape:
            raise ValueError(f"R_land_flux shape {R.shape} != grid shape {self.shape}")
        d = self.dev
        d.upload_now("RUNOFF", R)
        ev = self.schedule(dt_seconds, 1)[0]
        d.route_accumulate(dt_seconds)
        if ev == 0.0:
            return
        with_pe = precip_flux is not None and evap_flux is not None
        if with_pe:
            d.upload_now("PRECIP", np.asarray(precip_flux, dtype=float))
            d.upload_now("EFLUX", np.asarray(evap_flux, dtype=float))
        d.route_event(ev, with_pe)
        self.take_events(d.route_events())

    def take_events(self, log):
        """Records drained from the device log (Device.route_events): the reference's per-event line for each, and the
        newest becomes what diagnostics() reports."""
        if self.diag_enabled:
            for e in log:
                print(f"[HydroRouting] ocean_inflow={e['ocean_inflow_kgps']:.3e} kg/s | "
                      f"mass_error={e['mass_closure_error_kg']:.3e} kg")
        if len(log):
            self._have_event = True
            self._last = None

    def reset(self):
        self.t_accum = 0.0
        self._have_event = False
        self._last = None
        self.dev.route_reset()

    def buffer_kg(self):
        return self.dev.route_download("BUFFER").reshape(self.shape)

    def diagnostics(self) -> Dict[str, object]:
        if not self._have_event:
            return {"flow_accum_kgps": np.zeros(self.shape, dtype=float), "ocean_inflow_kgps": 0.0,
                    "mass_closure_error_kg": 0.0,
                    "lake_volume_kg": (np.zeros(self.n_lakes, dtype=float) if self.n_lakes > 0 else None)}
        if self._last is None:
            e = self.dev.route_last_event()
            self._last = RoutingDiagnostics(
                self.dev.route_download("FLOW").reshape(self.shape), float(e["ocean_inflow_kgps"]),
                float(e["mass_closure_error_kg"]), self.dev.route_download("LAKES") if self.n_lakes > 0 else None)
        L = self._last
        return {"flow_accum_kgps": L.flow_accum_kgps, "ocean_inflow_kgps": L.ocean_inflow_kgps,
                "mass_closure_error_kg": L.mass_closure_error_kg, "lake_volume_kg": L.lake_volume_kg}
