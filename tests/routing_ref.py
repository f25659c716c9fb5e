"""Test-side restatements for river routing (qingdai_amd/routing.py, qd_route.hip).

`SeqRouting`: pygcm/routing.py's accumulation and sequential event loop restated on a RoutingNetwork -- the
yardstick the device schedule is held against.  `emulate_event`: the device's segment / junction schedule
(k_route_walk, k_route_levels, k_route_reduce, k_route_final) in NumPy, to check the plan on a CPU.
"""
import numpy as np

from qingdai_amd.routing import T_DEAD, T_LAKE0, T_NOTPROC, T_OCEAN


class SeqRouting:
    def __init__(self, net, area_row, dt_hydro_seconds):
        self.net = net
        self.shape = net.shape
        self.area = np.repeat(np.asarray(area_row, float)[:, None], net.shape[1], axis=1)
        self.dt_hydro = float(dt_hydro_seconds)
        self.buffer = np.zeros(net.land_mask.size)
        self.t_accum = 0.0
        self.lake_vol = np.zeros(net.n_lakes) if net.n_lakes > 0 else None
        self.events = []

    def step(self, R, dt, P=None, E=None, step_index=None):
        net = self.net
        land = net.land_mask == 1
        self.buffer += np.where(land, np.asarray(R, float) * self.area * float(dt), 0.0).ravel()
        self.t_accum += float(dt)
        if self.t_accum + 1e-9 < self.dt_hydro:
            return None
        event_dt = self.t_accum
        self.t_accum = 0.0
        acc = self.buffer.copy()
        self.buffer.fill(0.0)
        n_cells = acc.size
        flow = np.zeros(n_cells)
        ocean = 0.0
        mass_input = float(np.sum(acc))
        land_flat = net.land_mask.ravel() == 1
        has = net.has_lakes
        lake_is = net.lake_mask.ravel() > 0 if has else None
        lid_f = net.lake_id.ravel() if has else None
        out = net.lake_outlet_index if has else None
        ft = net.flow_to_index
        for idx in net.flow_order.tolist():
            m = acc[idx]
            if m <= 0.0:
                continue
            flow[idx] += m
            if has and lake_is[idx]:
                lid = int(lid_f[idx])
                if lid > 0 and out is not None and lid <= out.shape[0]:
                    o = int(out[lid - 1])
                    if o < 0:
                        ocean += m
                    elif 0 <= o < n_cells and land_flat[o]:
                        acc[o] += m
                    else:
                        ocean += m
                else:
                    if self.lake_vol is not None and lid > 0:
                        self.lake_vol[lid - 1] += m
                acc[idx] = 0.0
                continue
            dn = int(ft[idx])
            if dn < 0 or not land_flat[dn]:
                ocean += m
                acc[idx] = 0.0
            else:
                acc[dn] += m
                acc[idx] = 0.0
        residual = float(np.sum(acc))
        lake_delta = 0.0
        if has and self.lake_vol is not None and P is not None and E is not None:
            lm = net.lake_mask.astype(bool)
            lake_add = float(np.sum(np.where(lm, (np.asarray(P, float) - np.asarray(E, float)) * self.area * event_dt, 0.0)))
            if lake_add != 0.0 and net.n_lakes > 0:
                with np.errstate(divide="ignore", invalid="ignore"):
                    for k in range(1, net.n_lakes + 1):
                        la = np.sum(np.where(net.lake_id == k, self.area, 0.0))
                        frac = 0.0 if la <= 0 else la / np.sum(np.where(lm, self.area, 0.0))
                        self.lake_vol[k - 1] += frac * lake_add
                lake_delta = lake_add
        closure = mass_input - (ocean + lake_delta + residual)
        ev = dict(step=step_index, event_dt=event_dt, flow=(flow / max(event_dt, 1e-9)).reshape(self.shape),
                  ocean_inflow_kgps=ocean / max(event_dt, 1e-9), mass_closure_error_kg=closure, mass_input_kg=mass_input,
                  lake_volume_kg=None if self.lake_vol is None else self.lake_vol.copy())
        self.events.append(ev)
        return ev


def emulate_accumulate(plan, buf, R, dt):
    A = np.repeat(plan.area_row[:, None], plan.n_lon, axis=1).ravel()
    buf += np.where(plan.cflags & 1, np.asarray(R, float).ravel() * A * float(dt), 0.0)


def emulate_event(plan, buf, lake_vol, event_dt, P=None, E=None):
    """One event of the device schedule on a plan (buf is cleared, lake_vol updated in place) -> record dict."""
    n_cells = buf.size
    M = np.zeros(n_cells)
    ss, sc, js, jc = plan.seg_start, plan.seg_cells, plan.jp_start, plan.jp_cells
    for L in range(plan.n_levels):                          # level order; lanes of a level are independent
        for s in range(plan.level_start[L], plan.level_start[L + 1]):
            h = sc[ss[s]]
            m = buf[h]
            for k in range(js[s], js[s + 1]):
                mu = M[jc[k]]
                if not (mu <= 0.0):
                    m = m + mu
            M[h] = m
            for i in range(ss[s] + 1, ss[s + 1]):
                c = sc[i]
                m = buf[c] if m <= 0.0 else buf[c] + m
                M[c] = m
    dt_den = max(event_dt, 1e-9)
    code = plan.code.astype(np.int64)
    proc = code != T_NOTPROC
    pos = proc & ~(M <= 0.0)
    flow = np.where(pos, M / dt_den, 0.0)
    mass_input = float(np.sum(buf))
    ocean = float(np.sum(np.where(pos & (code == T_OCEAN), M, 0.0)))
    residual = float(np.sum(np.where(~proc, buf, 0.0)) + np.sum(np.where(proc & (M <= 0.0), M, 0.0))
                     + np.sum(np.where(pos & (code == T_DEAD), M, 0.0)))
    with_pe = P is not None and E is not None and plan.pe_lakes and plan.n_lakes > 0
    lake_add = 0.0
    if with_pe:
        A = np.repeat(plan.area_row[:, None], plan.n_lon, axis=1).ravel()
        lake_add = float(np.sum(np.where(plan.cflags & 2, (np.asarray(P, float).ravel() - np.asarray(E, float).ravel()) * A * event_dt, 0.0)))
    pe = with_pe and lake_add != 0.0
    for k in range(plan.n_lakes):
        v = lake_vol[k]
        for c in plan.lake_cells[plan.lake_start[k]:plan.lake_start[k + 1]]:
            if not (M[c] <= 0.0):
                v += M[c]
        if pe:
            v += plan.lake_frac[k] * lake_add
        lake_vol[k] = v
    lake_delta = lake_add if pe else 0.0
    buf.fill(0.0)
    return dict(event_dt=event_dt, flow=flow.reshape(plan.n_lat, plan.n_lon), ocean_inflow_kgps=ocean / dt_den,
                mass_closure_error_kg=mass_input - ((ocean + lake_delta) + residual), mass_input_kg=mass_input)


def case_inputs(z, k):
    """Step k's (R, P, E) of a golden: base fields combined in f64."""
    R = z["R0"] + k * z["R1"]
    P = z["P0"] + k * z["P1"]
    E = z["E0"]
    return R, P, E


def case_vars(z):
    return {n[4:]: z[n] for n in z.files if n.startswith("net_")}
