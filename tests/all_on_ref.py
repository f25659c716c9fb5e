"""The CPU twin of the all-on driver loop (test infrastructure, a plain helper module): ocean, ecology with individuals, tracers,
river routing and the two daily steps in one iteration, composed of parts that each pin one lane elsewhere --
  DriverOracle + OceanOracle                         the physics step (oracle/qd_oracle/driver.py)
  EcoCoupling(EcoAdapter(CanopyPopulation)), IndividualSubstep   the sub-daily ecology (oracle/qd_oracle/ecology.py)
  phyto_daily_ref.step_daily                         PhytoManager.step_daily, fired inside the coupling; its alpha becomes ocean_alpha
  qd_oracle.phyto.advect_diffuse                     the tracer transport after the ocean step
  eco_daily_ref.step_daily                           PopulationManager.step_daily at the top of its firing steps, soil index from the
                                                     twin's own W_land and glacier of the step before
  routing_ref.SeqRouting                             fed with the twin's own runoff, precipitation and evaporation
in the reference driver's order (run_simulation.py:1785-1810 daily vegetation, 2021-2046 individuals, 2051-2061 daily phytoplankton,
2075-2128 albedo blend, 2194-2258 dynamics, ocean, transport, 2290-2348 hydrology commit and routing)."""
import numpy as np

import eco_daily_ref
import phyto_daily_ref
from routing_ref import SeqRouting


class _Coupling:
    """An EcoCoupling whose apply first runs the daily phytoplankton step on its firing steps (this step's insolation, the ocean
    temperature and the tracers as the step before left them) and hands its scalar alpha to the blend as ocean_alpha."""

    def __init__(self, twin, base, couple):
        self.twin, self.base, self.couple = twin, base, couple

    def apply(self, base_in, land, glacier, isr, dt):
        w = self.twin
        if w.phyto_fire is not None and w.phyto_fire[w.k]:
            d = w.drv
            r = phyto_daily_ref.step_daily(w.C, w.N, d.atm.isr_A, d.atm.isr_B, d.ocean.Ts, w.tab, w.mask)
            w.C, w.N, w.kd490, w.water_alpha = r["C"], r["N"], r["kd490"], r["alpha_scalar"]
            w.phyto_log.append([float(len(w.phyto_log) + 1)] + [float(x) for x in r["means"]])
            if self.couple:
                self.base.ocean_alpha = r["alpha_scalar"]
        return self.base.apply(base_in, land, glacier, isr, dt)


class AllOnTwin:
    def __init__(self, sim, init, env, network=None, dt_hydro_seconds=None, phyto_fire=None, eco_fire=None, couple=True):
        """sim: the device Simulation BEFORE its first step (configuration is read off it); init: dict(h, T_s, S_snow, W_land, layers,
        bank, C, N); env: the QD_ECO_* strings of the run; network: the synthetic_network dict or None; *_fire: per-step firing
        schedules (None = the lane is absent)."""
        import qd_oracle as qo
        from qd_oracle import ecology as oeco, spectral as osp
        from qd_oracle.driver import DriverOracle
        from qingdai_amd.routing import cell_area_rows, network_from_vars
        nlat, nlon = sim.grid.n_lat, sim.grid.n_lon
        self.mask = sim.land_mask
        land = self.land = sim.land_mask == 1
        self.g, P = qo.Grid(nlat, nlon), qo.defaults()
        m = self.m = qo.AtmosOracle(self.g, sim.friction, sim.land_mask, P, C_s_map=np.where(land, 3e6, P.Cs_ocean).astype(float))
        m.h, m.T_s = init["h"].copy(), init["T_s"].copy()
        self.oc = qo.OceanOracle(self.g, sim.land_mask, P, init_Ts=np.full((nlat, nlon), 288.0))
        drv = self.drv = DriverOracle(self.g, m, self.oc, qo.Forcing(self.g), sim.land_mask, sim.base_albedo, P)
        drv.S_snow, drv.W_land = init["S_snow"].copy(), init["W_land"].copy()
        drv.glacier = np.zeros((nlat, nlon), dtype=bool)
        ep = sim.eco.params
        ob = osp.make_bands(16, 380.0, 780.0)
        assert sim.eco.bands.nbands == 16 and abs(oeco.leaf_scalar(ob) - ep.leaf_scalar) < 1e-15
        self.pop = oeco.CanopyPopulation(sim.land_mask, init["layers"].copy(), k_canopy=ep.k_canopy, light_update_every_hours=ep.light_update_hours,
                                         recompute_lai_delta=ep.recompute_lai_delta)
        adapter = oeco.EcoAdapter(self.pop, oeco.leaf_scalar(ob), soil_ref=ep.soil_ref, substep_every_nphys=ep.substep_every_nphys)
        self.base = oeco.EcoCoupling(adapter, w_lai=ep.w_lai)
        drv.eco = _Coupling(self, self.base, couple)
        if sim.indiv is not None:
            pool = sim.indiv
            drv.indiv = oeco.IndividualSubstep(pool.sample_j, pool.sample_i, pool.indiv_cell_index, pool.indiv_Ab, pool.indiv_tol,
                                               pool.substeps_per_day)
            drv.indiv_bands, drv.indiv_day, drv.soil_cap = ob, pool.day_seconds, pool.soil_cap
        # daily phytoplankton + transport
        self.C, self.N = init["C"].copy(), init["N"].copy()
        self.kd490 = self.water_alpha = None
        self.phyto_fire, self.phyto_log = (None if phyto_fire is None else list(phyto_fire)), []
        self.tab = phyto_daily_ref.tables_from_host(sim.phyto_daily.t) if sim.phyto_daily is not None else None
        self.K_h, self.adv_alpha = sim.phyto.K_h, sim.phyto.adv_alpha
        # daily vegetation
        self.eco_fire, self.eco_log = (None if eco_fire is None else list(eco_fire)), []
        if eco_fire is not None:
            self.veg = eco_daily_ref.State(land, None, None, np.zeros(land.shape), init["bank"].copy(), land.astype(float))
            self.veg_cfg = eco_daily_ref.Cfg.from_env(env, sim.eco_daily.species_modes, sim.eco.pop.species_weights)
        # routing
        self.seq = None
        if network is not None:
            self.seq = SeqRouting(network_from_vars(network, (nlat, nlon)), cell_area_rows(sim.grid), dt_hydro_seconds)
        self.k = 0

    def step(self, dt):
        from qd_oracle import phyto as ophyto
        drv = self.drv
        if self.eco_fire is not None:
            for _ in range(int(self.eco_fire[self.k])):
                v = self.veg
                v.layers, v.E_day = self.pop.layers, self.pop.E_day
                eco_daily_ref.step_daily(v, self.veg_cfg, eco_daily_ref.soil_index(drv.W_land, drv.glacier, self.veg_cfg.soil_cap))
                self.pop.layers, self.pop.E_day = v.layers, v.E_day
                s = v.summary()
                self.eco_log.append([float(len(self.eco_log) + 1), s["LAI_min"], s["LAI_mean"], s["LAI_max"]])
        drv.step(self.k * dt, dt)
        self.C = ophyto.advect_diffuse(self.C, self.oc.uo, self.oc.vo, dt, self.g, self.mask, K_h=self.K_h, adv_alpha=self.adv_alpha)
        if self.seq is not None:
            self.seq.step(drv.R_flux, dt, drv.precip, self.m.E_flux_last, step_index=self.k + 1)
        self.k += 1

    def fields(self):
        m, d, oc = self.m, self.drv, self.oc
        f = self.pop.f_cached
        out = {"U": m.u, "V": m.v, "H": m.h, "TS": m.T_s, "Q": m.q, "CLOUD": m.cloud_cover, "HICE": m.h_ice, "W_LAND": d.W_land,
               "S_SNOW": d.S_snow, "ALBEDO": d.albedo, "UO": oc.uo, "VO": oc.vo, "ETA": oc.eta, "SST": oc.Ts,
               "ECO_LAI": self.pop.total_LAI(), "ECO_EDAY": self.pop.E_day, "ECO_ALPHA": self.base.last_alpha,
               "ECO_F": np.where(self.land, f, np.nan), "tracers": self.C, "layers": self.pop.layers}
        if self.phyto_fire is not None:
            out.update({"WATER_ALPHA": self.water_alpha, "KD490": self.kd490, "PHYTO_N": self.N})
        if self.eco_fire is not None:
            out.update({"age": self.veg.age, "bank": self.veg.bank})
        if d.indiv is not None:
            out.update({"indiv_E_day": d.indiv.E_day, "indiv_stress": d.indiv.stress_days})
        if self.seq is not None and self.seq.events:
            out.update({"route_flow": self.seq.events[-1]["flow"], "route_buffer": self.seq.buffer.reshape(self.land.shape)})
            if self.seq.lake_vol is not None:
                out["route_lakes"] = self.seq.lake_vol
        return out
