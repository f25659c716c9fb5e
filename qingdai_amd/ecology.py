"""
qingdai_amd/ecology.py -- the per-physics-step ecology on the device (stages 2-4; BASELINE config 5).

Mirrors, with the reference's names and call signatures, the part of pygcm/ecology the driver touches every step:

  EcologyAdapter(grid, land_mask).step_subdaily(I_total, cloud_eff, dt)      adapter.py:33-186
      .get_surface_albedo_bands()                                             adapter.py:519-545
  PopulationCanopy  -- the sub-daily face of PopulationManager               population.py:48-122,252-294,831-915
      E_day, LAI_layers_SK, total_LAI(), canopy_reflectance_factor(), step_subdaily()
  IndividualPool(grid, land_mask, eco).try_substep(isr_A, isr_B, eco, soil, dt, day)   individuals.py:37-191

State lives in the grid's Device (qd_eco_* / qd_indiv_* of include/qingdai_hip.h); inside a fused loop
(`Device.step_n(..., ecology=True)`) none of these methods is called at all.  The deterministic, grid-shaped part of the daily
population dynamics (PopulationManager.step_daily with its spread, seed bank and age, population.py:389-828) runs on the device
too: `PopulationDaily` configures it from the reference's environment variables, `PopulationCanopy.step_daily` is its class
seam, and `Device.step_n(..., eco_daily=...)` fires it inside a span (QD_ECO_DAILY=1 in the driver).  The diversity diagnostics
(pygcm/ecology/diversity.py) run on the device as well: `PopulationCanopy.diversity()` (qd_eco_diversity) with the clock, the line
and the file writer the driver uses under QD_ECO_DIVERSITY_ENABLE=1.  IndividualPool.step_daily
(individuals.py:193-361) runs on the device behind every firing of that daily step: `IndividualDaily` reads its variables, plans
the levels of the cell loop (`plan_levels`) and configures it, `IndividualPool.step_daily` is its class seam
(QD_ECO_INDIV_DAILY=1 in the driver).  Mutation and genes are host code outside this package: `Simulation` hands `E_day` to a
caller-supplied daily hook and takes the new LAI layers back.
"""
from __future__ import annotations

import ctypes
import os
from dataclasses import dataclass

import numpy as np

from . import spectral as sp
from ._lib import qd_eco_params, qd_eco_daily_params, qd_indiv_daily_params

_dp = ctypes.POINTER(ctypes.c_double)
_ip = ctypes.POINTER(ctypes.c_int32)


def _envf(name, default):
    try:
        return float(os.getenv(name, str(default)))
    except ValueError:
        return float(default)


def _envi(name, default):
    try:
        return int(os.getenv(name, str(default)))
    except ValueError:
        return int(default)


def _peaks_from_env(prefix):
    """`<prefix>PEAKS="450:40:0.6, 680:30:0.8"` (genes.py:53-67); the default is that two-peak absorber."""
    out = []
    for part in os.getenv(prefix + "PEAKS", "").split(","):
        try:
            c, w, h = part.strip().split(":")
            out.append((float(c), float(w), float(h)))
        except ValueError:
            continue
    return out or [(450.0, 40.0, 0.6), (680.0, 30.0, 0.8)]


class PopulationCanopy:
    """LAI layers + daily energy buffer + canopy cache of PopulationManager, resident on the device."""

    def __init__(self, dev, land_mask, diag=False):
        self._dev = dev
        self.land = (np.asarray(land_mask) == 1)
        self.shape = self.land.shape
        self.K = max(1, _envi("QD_ECO_COHORT_K", 1))
        w_env = os.getenv("QD_ECO_SPECIES_WEIGHTS", "").strip()
        ns_default = max(1, _envi("QD_ECO_NS", 20))
        if w_env:
            try:
                w = [float(x) for x in w_env.split(",") if x.strip() != ""]
            except ValueError:
                w = [1.0]
        else:
            w = [1.0 / float(ns_default)] * ns_default
        tot = sum(w) if w else 1.0
        if tot <= 0:
            self.species_weights = np.full((ns_default,), 1.0 / float(ns_default))
        else:
            self.species_weights = np.asarray([max(0.0, x) for x in w], dtype=float)
            self.species_weights /= tot
        self.Ns = int(self.species_weights.shape[0])
        lai0 = np.zeros(self.shape)
        lai0[self.land] = _envf("QD_ECO_LAI_INIT", 0.2)
        self.LAI_layers_SK = np.zeros((self.Ns, self.K) + self.shape)
        for s in range(self.Ns):
            for k in range(self.K):
                self.LAI_layers_SK[s, k] = float(self.species_weights[s]) * (lai0 / float(self.K))
        self._species_R_leaf = None
        self.daily = None                  # a PopulationDaily once the daily step runs on the device
        self.indiv_daily = None            # an IndividualDaily once the individuals' daily step runs on the device
        self.push_layers(init=True)

    def _stack_clock(self):
        """What has changed the resident stack so far: firings of the vegetation step and of the individuals' step."""
        return (self._dev.eco_daily_firings(), self._dev.indiv_daily_firings())

    # -- species weights: recomputed on the device by every firing of the individuals' daily step (population.py:343-359)
    @property
    def species_weights(self):
        if getattr(self, "indiv_daily", None) is not None:
            fired = self._dev.indiv_daily_firings()
            if fired and fired != self._weights_at:
                self._weights, self._weights_at = self._dev.indiv_daily_weights(self._weights.size), fired
        return self._weights

    @species_weights.setter
    def species_weights(self, w):
        self._weights = w
        self._weights_at = self._dev.indiv_daily_firings() if getattr(self, "indiv_daily", None) is not None else 0

    # -- LAI
    @property
    def LAI_layers_SK(self):
        """[S, K, lat, lon]; with a device daily step the resident stack is the truth and is downloaded."""
        if getattr(self, "daily", None) is not None:
            fired = self._stack_clock()                        # the device's own counts: firings of a span or of a direct call alike
            if fired != self._layers_at:
                self._layers, self._layers_at = self._dev.eco_daily_get_layers(self.Ns, self.K), fired
        return self._layers

    @LAI_layers_SK.setter
    def LAI_layers_SK(self, layers):
        self._layers = layers
        self._layers_at = self._stack_clock() if getattr(self, "daily", None) is not None else 0

    def push_layers(self, layers=None, init=False):
        """Hand the (changed) [S, K, lat, lon] stack to the device: what the daily step does once per planet-day."""
        if layers is not None:
            self.LAI_layers_SK = np.asarray(layers, dtype=np.float64)
        a = np.ascontiguousarray(self.LAI_layers_SK, dtype=np.float64)
        if a.shape[-2:] != self.shape:
            raise ValueError(f"LAI layers: expected [..., {self.shape[0]}, {self.shape[1]}], got {a.shape}")
        n = int(np.prod(a.shape[:-2]))
        self._dev._chk(self._dev.lib.qd_eco_set_lai_layers(self._dev.h, a.ctypes.data, n, 1 if init else 0), "qd_eco_set_lai_layers")
        if self.daily is not None:
            self._dev.eco_daily_set_layers(a.reshape((-1,) + self.shape))

    # -- daily step (population.py:389-596) on the device
    def step_daily(self, soil_water_index):
        """One firing of the device daily step with the reference's argument: None = dry (zeros), a scalar, or a [lat, lon] map
        (any other shape falls back to its nanmean, population.py:408-416)."""
        if self.daily is None:
            PopulationDaily(self)
        if soil_water_index is None:
            soil = np.zeros(self.shape)
        elif np.isscalar(soil_water_index):
            soil = np.full(self.shape, float(soil_water_index))
        else:
            soil = np.asarray(soil_water_index, dtype=float)
            if soil.shape != self.shape:
                soil = np.full(self.shape, float(np.nanmean(soil)))
        self._dev.eco_daily_step(soil)
        self.daily._fired(1)

    @property
    def age_days(self):
        self._dev._host.pop("ECO_AGE", None)
        return self._dev.get("ECO_AGE").copy()

    @property
    def seed_bank(self):
        self._dev._host.pop("ECO_SEEDBANK", None)
        return self._dev.get("ECO_SEEDBANK").copy()

    @seed_bank.setter
    def seed_bank(self, arr):
        self._dev.upload_now("ECO_SEEDBANK", np.broadcast_to(np.asarray(arr, dtype=np.float64), self.shape))

    @property
    def _spread_gate(self):
        self._dev._host.pop("ECO_GATE", None)
        return self._dev.get("ECO_GATE").copy()

    def total_LAI(self):
        self._dev._host.pop("ECO_LAI", None)
        return self._dev.get("ECO_LAI").copy()

    # -- daily energy buffer
    @property
    def E_day(self):
        self._dev._host.pop("ECO_EDAY", None)
        return self._dev.get("ECO_EDAY").copy()

    @E_day.setter
    def E_day(self, arr):
        self._dev.upload_now("ECO_EDAY", np.broadcast_to(np.asarray(arr, dtype=np.float64), self.shape))

    # -- canopy
    def canopy_reflectance_factor(self):
        """f(LAI) on land, NaN elsewhere (population.py:831-842); needs a canopy cache (any sub-step or banded call builds it)."""
        self._dev._host.pop("ECO_F", None)
        out = np.full(self.shape, np.nan)
        f = self._dev.get("ECO_F")
        out[self.land] = f[self.land]
        return out

    def set_species_reflectance_bands(self, R):
        R = np.asarray(R, dtype=float)
        self._species_R_leaf = np.clip(R, 0.0, 1.0) if R.ndim == 2 else None

    def effective_leaf_reflectance_bands(self, nb):
        """R_eff[b] = clip(sum_i w_i R_i[b]) with the reference's fallbacks (population.py:856-873)."""
        R = self._species_R_leaf
        if R is None:
            return np.full((nb,), 0.5)
        if R.shape[1] != nb:
            return np.full((nb,), float(np.nanmean(R)))
        w = self.species_weights if self.species_weights.size == R.shape[0] else np.full((R.shape[0],), 1.0 / max(1, R.shape[0]))
        return np.clip(np.tensordot(w, R, axes=(0, 0)), 0.0, 1.0)

    # -- diversity diagnostics (pygcm/ecology/diversity.py) on the device
    def diversity(self):
        """compute_alpha_eff_map, compute_local_bray_curtis and compute_whittaker_beta of the current community ->
        (alpha_map, bc_local, L_s [S, lat, lon], {alpha_mean, gamma_eff, beta_whittaker}).  With a device daily step the
        resident stack is used where it lies; otherwise the host LAI_layers_SK is handed over.  Changes no state."""
        d = self._dev
        w_row = diversity_weights(d.grid.lat_mesh, self.land)
        if self.daily is not None:
            summary = d.eco_diversity(w_row, n_species=self.Ns, n_layers=self.K)
        else:
            summary = d.eco_diversity(w_row, layers=np.asarray(self.LAI_layers_SK, dtype=np.float64))
        return d.eco_diversity_get("ECO_DIV_ALPHA"), d.eco_diversity_get("ECO_DIV_BC"), d.eco_diversity_get("ECO_DIV_LS"), summary

    def state(self):
        out = (ctypes.c_double * 5)()
        self._dev._chk(self._dev.lib.qd_eco_get_state(self._dev.h, out), "qd_eco_get_state")
        return {"hours": out[0], "next_recompute_hours": out[1], "step_count": int(out[2]), "n_recompute": int(out[3]),
                "alpha_cached": bool(out[4])}

    def summary(self):
        L = self.total_LAI()[self.land]
        if L.size == 0:
            return {"LAI_min": 0.0, "LAI_mean": 0.0, "LAI_max": 0.0}
        return {"LAI_min": float(np.min(L)), "LAI_mean": float(np.mean(L)), "LAI_max": float(np.max(L))}


def diversity_weights(lat_mesh, land):
    """The static factor of compute_whittaker_beta (diversity.py:28-31,69-72): w_norm = max(cos(deg2rad(lat)), 0) / (its sum over
    land + 1e-15), evaluated on the mesh as the reference does -> the per-row table [n_lat] the device takes."""
    w = np.maximum(np.cos(np.deg2rad(np.asarray(lat_mesh, dtype=float))), 0.0)
    w_sum_land = float(np.sum(w[np.asarray(land, dtype=bool)])) + 1e-15
    return np.ascontiguousarray((w / w_sum_land)[:, 0])


def diversity_env(env):
    """-> (enabled, every_days) from QD_ECO_DIVERSITY_ENABLE (default 0) and QD_ECO_DIVERSITY_EVERY_DAYS (default 10, and 10 on a
    parse error; run_simulation.py reads them the same way)."""
    try:
        enabled = int(env.get("QD_ECO_DIVERSITY_ENABLE", "0")) == 1
    except ValueError:
        enabled = False
    try:
        every = float(env.get("QD_ECO_DIVERSITY_EVERY_DAYS", "10"))
    except ValueError:
        every = 10.0
    return enabled, every


def diversity_firings(times, day_seconds, next_day, every_days):
    """The reference's clock (run_simulation.py:2404-2411) over the step START times `times` (float64, as Simulation._span_times
    holds them): the step whose t / day >= next fires and sets next = t / day + every -> (indices of the firing steps, next)."""
    fired = []
    for i, t in enumerate(np.asarray(times, dtype=np.float64)):
        t_days = float(t) / day_seconds
        if t_days >= next_day:
            fired.append(i)
            next_day = t_days + every_days
    return fired, next_day


def diversity_summary_text(t_days, summary):
    """The four lines of diversity_summary_day_*.txt (diversity.py:168-172), character for character."""
    return (f"Day: {t_days:.2f}\n"
            f"Whittaker beta (\u03b2 = \u03b3/\u03b1\u0304): {summary['beta_whittaker']:.4f}\n"
            f"  alpha_mean (\u03b1\u0304): {summary['alpha_mean']:.4f}\n"
            f"  gamma_eff  (\u03b3 ): {summary['gamma_eff']:.4f}\n")


def diversity_line(t_days, summary):
    """The driver's line per firing under QD_ECO_DIAG=1."""
    return (f"[Diversity] day {t_days:.2f}: alpha_mean={summary['alpha_mean']:.4f} gamma_eff={summary['gamma_eff']:.4f} "
            f"beta_whittaker={summary['beta_whittaker']:.4f}")


def write_diversity_files(base_output_dir, t_days, alpha_map, bc_local, L_s, summary, land_mask):
    """The reference's files under <base_output_dir>/ecology/ (diversity.py:138-186, 197): the text summary and
    community_day_*.npz (L_s as float32, land_mask as int8) as they are; the two PNG maps become diversity_maps_day_*.npz with
    alpha_map and bc_local (no matplotlib here) -> the three paths."""
    outdir = os.path.join(base_output_dir, "ecology")
    os.makedirs(outdir, exist_ok=True)
    tag = f"{t_days:05.1f}"
    paths = (os.path.join(outdir, f"diversity_summary_day_{tag}.txt"), os.path.join(outdir, f"community_day_{tag}.npz"),
             os.path.join(outdir, f"diversity_maps_day_{tag}.npz"))
    with open(paths[0], "w", encoding="utf-8") as f:
        f.write(diversity_summary_text(t_days, summary))
    np.savez(paths[1], L_s=np.asarray(L_s).astype(np.float32), land_mask=np.asarray(land_mask).astype(np.int8))
    np.savez(paths[2], alpha_map=np.asarray(alpha_map), bc_local=np.asarray(bc_local))
    return paths


def _envf_any(name, default):
    """float(os.getenv(name, default)) with the reference's `except Exception` fallback to the default."""
    try:
        return float(os.getenv(name, str(default)))
    except Exception:      # noqa: BLE001
        return float(default)


def species_modes_from_env(n_species, species_weights, weights_from_env):
    """PopulationManager._init_species_modes (population.py:177-229): QD_ECO_SPECIES_{i}_MODE where it names 'seed' or 'diffusion';
    the rest from np.random.default_rng(QD_ECO_RAND_SEED) -- with QD_ECO_SPECIES_WEIGHTS set ONE draw by weight picks the single
    seed species, otherwise one uniform draw per unspecified species in index order (< 0.5 = seed).  Same generator calls in the
    same order as the reference, so a given seed yields its modes."""
    S = int(n_species)
    modes = []
    for i in range(S):
        m = os.getenv(f"QD_ECO_SPECIES_{i}_MODE", "").strip().lower()
        modes.append(m if m in ("seed", "diffusion") else "")
    try:
        seed_val = os.getenv("QD_ECO_RAND_SEED")
        rng = np.random.default_rng(int(seed_val)) if seed_val not in (None, "") else np.random.default_rng()
    except Exception:      # noqa: BLE001
        rng = np.random.default_rng()
    unspec = [i for i in range(S) if modes[i] == ""]
    if not unspec:
        return modes
    if weights_from_env:
        try:
            w = np.clip(np.asarray(species_weights, dtype=float), 0.0, None)
            w = w / (np.sum(w) + 1e-12)
            chosen = int(rng.choice(np.arange(S), p=w))
        except Exception:      # noqa: BLE001
            chosen = 1 if S > 1 else 0
        for i in unspec:
            modes[i] = "seed" if i == chosen else "diffusion"
    else:
        for i in unspec:
            modes[i] = "seed" if rng.random() < 0.5 else "diffusion"
    return modes


def daily_counts(accum, dt, n, day):
    """The reference's day accumulator over n steps (run_simulation.py:1784-1789, float64): accum += dt; while accum >= day:
    accum -= day, one firing -> (firings per step [n] int32, the accumulator afterwards)."""
    fire = np.zeros(int(n), dtype=np.int32)
    a, dt, day = np.float64(accum), np.float64(dt), np.float64(day)
    for s in range(int(n)):
        a = a + dt
        while a >= day:
            a = a - day
            fire[s] += 1
    return fire, float(a)


def eco_daily_line(rec):
    """The adapter's diagnostic line (adapter.py:434-436) from a record {firings, LAI_min, LAI_mean, LAI_max}."""
    return f"[Ecology] daily: LAI(min/mean/max)={rec[1]:.2f}/{rec[2]:.2f}/{rec[3]:.2f}"


class PopulationDaily:
    """The device daily step of a PopulationCanopy: parameters from the reference's environment variables with its defaults and
    parse fallbacks (LAIParams.from_env, QD_ECO_SPREAD_*, QD_ECO_REPRO_FRACTION, QD_ECO_SEED_*, QD_ECO_SEEDLING_LAI,
    QD_ECO_LAYER_UPFRAC, QD_ECO_SOIL_WATER_CAP), the per-species spread modes, and the span participant of Device.step_n: a day
    accumulator on the host names the firing steps, rolled back when the span does not run."""

    def __init__(self, pop, day_seconds=None, species_modes=None):
        self.pop, self.dev = pop, pop._dev
        self.shape = pop.shape
        from .forcing import PLANET_OMEGA
        self.day_seconds = float(day_seconds) if day_seconds else 2 * np.pi / PLANET_OMEGA
        self.accum_day = 0.0
        self.n_firings = 0
        try:
            enable = int(os.getenv("QD_ECO_SPREAD_ENABLE", "0")) == 1
        except Exception:      # noqa: BLE001
            enable = False
        self.spread_enable = enable
        self.spread_rate = _envf_any("QD_ECO_SPREAD_RATE", 0.0)
        self.spread_neighbors = os.getenv("QD_ECO_SPREAD_NEIGHBORS", "vonNeumann").strip().lower()
        self.repro_fraction = _envf_any("QD_ECO_REPRO_FRACTION", 0.2)
        gate_soil, soil_exp = 1, 1.0
        try:                               # population.py:423-431: any parse failure here means the land-mask gate
            gate_soil = 1 if int(os.getenv("QD_ECO_SPREAD_GATE_SOIL", "1")) == 1 else 0
            if gate_soil:
                soil_exp = float(os.getenv("QD_ECO_SPREAD_SOIL_EXP", "1.0"))
        except Exception:      # noqa: BLE001
            gate_soil = 0
        cap_env = os.getenv("QD_ECO_SOIL_WATER_CAP")
        try:
            soil_cap = float(cap_env) if cap_env is not None else 50.0
        except Exception:      # noqa: BLE001
            soil_cap = 50.0
        self.species_modes = list(species_modes) if species_modes is not None else species_modes_from_env(
            pop.Ns, pop.species_weights, bool(os.getenv("QD_ECO_SPECIES_WEIGHTS", "").strip()))
        rate = float(max(0.0, min(0.5, self.spread_rate)))
        self.params = qd_eco_daily_params(
            n_species=pop.Ns, n_layers=pop.K, spread=1 if (self.spread_enable and self.spread_rate > 0.0) else 0,
            moore=1 if self.spread_neighbors in ("moore", "8", "8n") else 0, gate_soil=gate_soil, reserved=0,
            lai_max=_envf_any("QD_ECO_LAI_MAX", 5.0), k_canopy=_envf_any("QD_ECO_LAI_K", 0.5),
            growth_per_j=_envf_any("QD_ECO_LAI_GROWTH", 2.0e-5), senesce_per_day=_envf_any("QD_ECO_LAI_SENESCENCE", 0.01),
            stress_thresh=_envf_any("QD_ECO_SOIL_STRESS_THRESH", 0.3), stress_strength=_envf_any("QD_ECO_SOIL_STRESS_GAIN", 1.0),
            soil_cap=soil_cap, repro_frac=float(np.clip(self.repro_fraction, 0.0, 0.95)), spread_rate=rate, soil_exp=soil_exp,
            upfrac=_envf_any("QD_ECO_LAYER_UPFRAC", 0.1), dlai_max=_envf_any("QD_ECO_SPREAD_DLAI_MAX", 0.02),
            seed_energy=float(max(1e-12, _envf_any("QD_ECO_SEED_ENERGY", 1.0))),
            seed_scale=float(max(1e-12, _envf_any("QD_ECO_SEED_SCALE", 1.0))),
            seedling_lai=_envf_any("QD_ECO_SEEDLING_LAI", 0.02), retain=_envf_any("QD_ECO_SEED_BANK_RETAIN", 0.2),
            bank_max=_envf_any("QD_ECO_SEED_BANK_MAX", 1000.0), seed_dlai_max=_envf_any("QD_ECO_SEED_DLAI_MAX", 0.01),
            germ_frac=_envf_any("QD_ECO_SEED_GERMINATE_FRAC", 0.10), bank_decay=_envf_any("QD_ECO_SEED_BANK_DECAY", 0.02))
        self.configure()

    def configure(self):
        """(Re)configure the device: parameters, modes, weights, the current layers; age, seed bank, log and firing count to zero."""
        pop = self.pop
        layers = np.ascontiguousarray(pop.LAI_layers_SK, dtype=np.float64)
        w = np.asarray(pop.species_weights, dtype=float)
        w = w / (np.sum(w) + 1e-12)                                                     # population.py:571-572
        mode = [1 if str(m).lower() == "seed" else 0 for m in self.species_modes]
        self.dev.eco_daily_configure(self.params, mode, w)
        self.n_firings = 0
        pop.daily = self
        pop.LAI_layers_SK = layers
        self.dev.eco_daily_set_layers(layers.reshape((-1,) + self.shape))
        self.dev.upload_now("ECO_GATE", pop.land.astype(float))                         # population.py:171
        if getattr(pop, "indiv_daily", None) is not None:                               # the device dropped it with the old stack
            pop.indiv_daily.configure()

    def _fired(self, n):
        self.n_firings += int(n)

    def schedule(self, dt, n):
        fire, self.accum_day = daily_counts(self.accum_day, dt, n, self.day_seconds)
        return fire

    # ---- span participant (Device.step_n)
    def span_clock(self):
        return self.accum_day

    def span_schedule(self, t0, dt, n):
        fire = self.schedule(dt, n)
        self.dev.eco_daily_schedule(fire)
        return int(fire.sum())

    def span_restore(self, clock):
        self.accum_day = clock

    def log(self):
        """Drain the device log -> list of summary() dicts, oldest first."""
        return [{"step": int(r[0]), "LAI_min": float(r[1]), "LAI_mean": float(r[2]), "LAI_max": float(r[3])}
                for r in self.dev.eco_daily_log()]


def spill_targets(j, i, H, W):
    """The four grid cells the cell loop of IndividualPool.step_daily adds recruits to, in its order (individuals.py:296-299):
    `zip(jn, in_)` of jn = [max(0, j-1), min(H-1, j+1), j, j] and in_ = [(i-1) % W, (i+1) % W, i, i] -- as written that pairs the
    row neighbours with the column neighbours: the north-west and south-east cells, then the cell itself twice."""
    jn = [max(0, j - 1), min(H - 1, j + 1), j, j]
    in_ = [(i - 1) % W, (i + 1) % W, i, i]
    return list(zip(jn, in_))


def footprint(j, i, H, W):
    """The set of grid cells a sampled cell reads or writes in the cell loop: itself and its spill targets."""
    return {(j, i), *spill_targets(j, i, H, W)}


def plan_levels(sample_j, sample_i, H, W):
    """Levels of the cell loop (individuals.py:259-306): level(c) = 1 + max(level of the earlier cells whose footprint meets
    c's), 1 without one -> int32 [C].  Cells of one level touch disjoint grid cells and may run together; running the levels in
    ascending order keeps every conflicting pair (read-write and write-write alike: f64 addition does not commute in its
    rounding) in the order of the sequential loop."""
    top = {}                                     # grid cell -> the highest level of a cell so far whose footprint holds it
    levels = np.zeros(len(sample_j), dtype=np.int32)
    for c, (j, i) in enumerate(zip(np.asarray(sample_j).tolist(), np.asarray(sample_i).tolist())):
        f = footprint(j, i, H, W)
        lv = 1 + max(top.get(g, 0) for g in f)
        for g in f:
            top[g] = lv
        levels[c] = lv
    return levels


def indiv_daily_line(n_cells, per_cell, beta_hint):
    """The reference's diagnostic line (individuals.py:360-361)."""
    return (f"[EcoIndiv] daily applied to {int(n_cells)} cells \u00d7 {int(per_cell)} indiv; "
            f"mean max species share per cell ~ {beta_hint:.2f} (lower\u2192more even).")


class IndividualDaily:
    """The device daily step of an IndividualPool (individuals.py:193-361) on the stack of a PopulationDaily: parameters from the
    reference's variables with its defaults, the species id of every individual, the level plan of the cell loop.  A value that
    does not parse is an error here (the reference raises inside step_daily and its driver skips the step every day), except
    in the seed-coupling block, whose `except Exception: pass` switches the coupling off."""

    def __init__(self, pool, pop):
        if pop is None or getattr(pop, "daily", None) is None:
            raise ValueError("IndividualDaily needs a population whose daily step runs on the device (PopulationDaily)")
        self.pool, self.pop, self.dev = pool, pop, pop._dev
        strict = lambda name, default: float(os.getenv(name, default))
        couple, repro, seed_energy, retain, bank_max = 0, 0.2, 1.0, 0.2, 1000.0
        try:                                                                           # individuals.py:315-337
            couple = 1 if int(os.getenv("QD_ECO_INDIV_SEED_COUPLE", "1")) == 1 else 0
            repro = float(pop.daily.repro_fraction)
            seed_energy = _envf_any("QD_ECO_SEED_ENERGY", 1.0)                          # pop.seed_energy (population.py:154-157)
            retain = float(os.getenv("QD_ECO_SEED_BANK_RETAIN", "0.2"))
            bank_max = float(os.getenv("QD_ECO_SEED_BANK_MAX", "1000.0"))
        except Exception:      # noqa: BLE001
            couple = 0
        self.params = qd_indiv_daily_params(
            n_species=pop.Ns, n_layers=pop.K, per_cell=int(pool.per_cell), seed_couple=couple,
            stress_penalty=strict("QD_ECO_INDIV_STRESS_PENALTY", "0.2"), lai_grow=strict("QD_ECO_LAI_GROWTH_RATE", "0.002"),
            lai_decay=strict("QD_ECO_LAI_DECAY_RATE", "0.001"), recruit_frac=strict("QD_ECO_LAI_RECRUIT_FRAC", "0.2"),
            stress_decay=strict("QD_ECO_INDIV_STRESS_DECAY", "0.5"), repro_frac=repro, seed_energy=seed_energy, retain=retain,
            bank_max=bank_max, lai_max=float(pop.daily.params.lai_max))
        self.levels = plan_levels(pool.sample_j, pool.sample_i, pool.h, pool.w)
        self.n_levels = int(self.levels.max()) if self.levels.size else 0
        self.configure()

    def configure(self):
        self.dev.indiv_daily_configure(self.params, self.pool.indiv_species_id, self.levels)
        self.pool.daily = self
        self.pop.indiv_daily = self
        self.pop.species_weights = self.pop._weights                                    # the firing count starts again at zero

    def log(self):
        """Drain the device log -> list of dicts, oldest first."""
        return [{"step": int(r[0]), "beta_hint": float(r[1]), "n_cells": int(r[2]), "levels": int(r[3])} for r in self.dev.indiv_daily_log()]

    def lines(self, records=None):
        """The reference's line per firing."""
        return [indiv_daily_line(r["n_cells"], self.pool.per_cell, r["beta_hint"]) for r in (self.log() if records is None else records)]


@dataclass
class AdapterConfig:
    substep_every_nphys: int = 1
    lai_albedo_weight: float = 1.0


class EcologyAdapter:
    def __init__(self, grid, land_mask, dev=None, albedo_couple=None, f32_maps=None):
        """f32_maps: None = QD_ECO_F32 (0) -- store the canopy maps (LAI_tot, snapshot, f, alpha, banded alpha) as f32 on the device
        (BASELINE configs[4] "f32 mixed precision"); arithmetic, reductions and E_day stay f64."""
        self.grid = grid
        self._dev = dev if dev is not None else getattr(grid, "_device", None)
        if self._dev is None:
            raise RuntimeError("EcologyAdapter needs the grid's Device (create the SpectralModel first, or pass dev=)")
        self.land_mask = (np.asarray(land_mask) == 1)
        self.cfg = AdapterConfig(_envi("QD_ECO_SUBSTEP_EVERY_NPHYS", 1), _envf("QD_ECO_LAI_ALBEDO_WEIGHT", 1.0))
        self.bands = sp.make_bands()
        self.w_b = sp.band_weights_from_mode(self.bands)
        self.R_leaf = sp.default_leaf_reflectance(self.bands)
        self.alpha_leaf_scalar = float(np.sum(self.R_leaf * self.w_b))
        if albedo_couple is None:
            albedo_couple = _envi("QD_ECO_SUBDAILY_ENABLE", 1) == 1 and _envi("QD_ECO_ALBEDO_COUPLE", 1) == 1
        self.params = qd_eco_params(
            k_canopy=_envf("QD_ECO_LAI_K", 0.5), leaf_scalar=float(np.clip(self.alpha_leaf_scalar, 0.0, 1.0)),
            soil_ref=_envf("QD_ECO_SOIL_REFLECT", 0.20), w_lai=self.cfg.lai_albedo_weight,
            light_update_hours=_envf("QD_ECO_LIGHT_UPDATE_EVERY_HOURS", 6.0),
            recompute_lai_delta=_envf("QD_ECO_LIGHT_RECOMPUTE_LAI_DELTA", 0.05),
            substep_every_nphys=max(1, self.cfg.substep_every_nphys), albedo_couple=1 if albedo_couple else 0,
            bands_couple=1 if _envi("QD_ECO_BANDS_COUPLE", 0) == 1 else 0,
            water_couple=1 if (_envi("QD_PHYTO_ENABLE", 0) == 1 and _envi("QD_PHYTO_ALBEDO_COUPLE", 1) == 1) else 0,
            use_lai=1 if _envi("QD_ECO_USE_LAI", 1) == 1 else 0,
            map_f32=1 if ((_envi("QD_ECO_F32", 0) == 1) if f32_maps is None else bool(f32_maps)) else 0)
        self.configure()
        self._count = 0
        self.pop = None
        if not self.params.use_lai:        # M1 branch (adapter.py:79-80,162-166): no population, scalar leaf alpha on land
            self.species_drought_tolerance = None
            return
        self.pop = PopulationCanopy(self._dev, self.land_mask.astype(int))
        # per-species leaf reflectance and drought tolerance from the QD_ECO_SPECIES_{i}_* genes (adapter.py:90-116, genes.py:45-90)
        R, tol = species_tables(self.bands, self.pop.Ns)
        self.pop.set_species_reflectance_bands(R)
        self.species_drought_tolerance = tol

    def configure(self):
        self._dev._chk(self._dev.lib.qd_eco_configure(self._dev.h, ctypes.byref(self.params), ctypes.sizeof(self.params)),
                       "qd_eco_configure")

    def step_subdaily(self, I_total=None, cloud_eff=None, dt_seconds=300.0):
        """adapter.py:140-186.  With I_total=None the resident ISR is used (the usual case); returns the land-only alpha map
        on a sub-step boundary (downloaded), None otherwise."""
        d = self._dev
        if I_total is not None:
            d.set("ISR", I_total)
        d.flush()
        d._chk(d.lib.qd_eco_substep(d.h, float(dt_seconds)), "qd_eco_substep")
        out = (ctypes.c_double * 5)()
        d._chk(d.lib.qd_eco_get_state(d.h, out), "qd_eco_get_state")
        if int(out[2]) % max(1, self.cfg.substep_every_nphys) != 0:
            return None
        d._host.pop("ECO_ALPHA", None)
        return d.get("ECO_ALPHA").copy()

    def banded_alpha(self):
        """The driver's daily reduction (run_simulation.py:1839-1844) computed on the device and left resident in
        ECO_ALPHA_BANDED: clip(nansum_b A_b w_b, 0, 1).  Returns the host copy."""
        d = self._dev
        nb = int(self.bands.nbands)
        r = np.ascontiguousarray(self.pop.effective_leaf_reflectance_bands(nb), dtype=np.float64)
        w = np.ascontiguousarray(self.w_b, dtype=np.float64)
        d.flush()
        d._chk(d.lib.qd_eco_banded_alpha(d.h, nb, r.ctypes.data_as(_dp), w.ctypes.data_as(_dp)), "qd_eco_banded_alpha")
        d._host.pop("ECO_ALPHA_BANDED", None)
        return d.get("ECO_ALPHA_BANDED").copy()

    def get_surface_albedo_bands(self):
        """(A_b [NB, lat, lon], w_b) like adapter.py:519-545, rebuilt on the host from the resident canopy factor."""
        nb = int(self.bands.nbands)
        R_eff = self.pop.effective_leaf_reflectance_bands(nb)
        f = self.pop.canopy_reflectance_factor()
        A = np.full((nb,) + self.pop.shape, np.nan)
        land = self.land_mask
        for b in range(nb):
            A[b][land] = np.clip(R_eff[b] * f[land] + (1.0 - f[land]) * self.params.soil_ref, 0.0, 1.0)
        return A, self.w_b.copy()


def sample_pool(land_mask, species_weights, R_species, drought_tol, nb, sample_frac, per_cell):
    """The arrays IndividualPool.__init__ draws (individuals.py:63-131), as a pure host function: sampled cells without
    replacement from default_rng(42), the cell index of every individual, species by weight, per-band coefficients = species
    leaf reflectance + N(0, 0.02) jitter clipped to [0, 1], drought tolerance by species.  Same generator calls in the same
    order as the reference, so the same land mask and species table give the same pool."""
    land = (np.asarray(land_mask) == 1)
    width = land.shape[1]
    w = np.asarray(species_weights, dtype=float)
    if w.ndim != 1 or w.size <= 0:
        w = np.asarray([1.0])
    ns = int(w.size)
    spw = w / w.sum() if w.sum() > 0 else np.full((ns,), 1.0 / ns)
    rng = np.random.default_rng(seed=42)
    land_idx = np.flatnonzero(land.ravel())
    want = max(1, int(sample_frac * land_idx.size))
    picked = land_idx if want >= land_idx.size else rng.choice(land_idx, size=want, replace=False)
    sample_j = np.asarray(picked // width, dtype=np.int32)
    sample_i = np.asarray(picked % width, dtype=np.int32)
    n_cells = int(sample_j.size)
    n_indiv = n_cells * int(per_cell)
    cell = np.repeat(np.arange(n_cells, dtype=np.int32), int(per_cell))
    species_id = rng.choice(np.arange(ns, dtype=np.int32), size=n_indiv, p=spw)
    R = R_species
    if R is None or R.shape[0] != ns:
        R = np.full((ns, nb), 0.5)
    if R.shape[1] > nb:
        R = R[:, :nb]
    elif R.shape[1] < nb:
        R = np.pad(R, ((0, 0), (0, nb - R.shape[1])), mode="edge")
    Ab = np.clip(R[species_id, :] + rng.normal(0.0, 0.02, size=(n_indiv, nb)), 0.0, 1.0)
    tol = np.full((ns,), 0.5) if drought_tol is None or len(drought_tol) != ns else np.asarray(drought_tol, dtype=float)
    return {"sp_weights": spw, "sample_j": sample_j, "sample_i": sample_i, "indiv_cell_index": cell, "indiv_species_id": species_id,
            "indiv_Ab": Ab, "indiv_tol": np.clip(tol, 0.0, 1.0)[species_id]}


def species_tables(bands, n_species):
    """Per-species leaf reflectance [Ns, NB] and drought tolerance [Ns] from the QD_ECO_SPECIES_{i}_* genes
    (adapter.py:90-116, genes.py:45-111)."""
    R, tol = [], []
    for i in range(n_species):
        pre = f"QD_ECO_SPECIES_{i}_"
        R.append(np.clip(1.0 - sp.absorbance_from_peaks(bands, _peaks_from_env(pre)), 0.0, 1.0))
        tol.append(_envf(pre + "DROUGHT_TOL", 0.3))
    return np.stack(R, axis=0), np.asarray(tol, dtype=float)


class IndividualPool:
    """Sampled individuals (individuals.py:37-191).  The sampling uses the same generator calls in the same order as the
    reference (default_rng(42): cells without replacement, species by weight, N(0, 0.02) jitter), so a given land mask yields
    the same pool."""

    def __init__(self, grid, land_mask, eco_adapter, *, sample_frac=0.02, per_cell=100, substeps_per_day=10, day_seconds=None,
                 soil_cap=None, diag=False, f32_storage=None):
        if getattr(eco_adapter, "pop", None) is None:
            raise RuntimeError("IndividualPool requires EcologyAdapter.pop (QD_ECO_USE_LAI=1)")     # individuals.py:67-69
        self._dev = eco_adapter._dev
        self.land_mask = (np.asarray(land_mask) == 1)
        self.h, self.w = self.land_mask.shape
        self.bands = eco_adapter.bands
        self.nb = int(self.bands.nbands)
        pop = eco_adapter.pop
        frac = _envf("QD_ECO_INDIV_SAMPLE_FRAC", sample_frac)
        self.per_cell = _envi("QD_ECO_INDIV_PER_CELL", per_cell)
        self.substeps_per_day = max(1, _envi("QD_ECO_INDIV_SUBSTEPS_PER_DAY", substeps_per_day))
        arr = sample_pool(self.land_mask, pop.species_weights, pop._species_R_leaf,
                          getattr(eco_adapter, "species_drought_tolerance", None), self.nb, frac, self.per_cell)
        for k, v in arr.items():
            setattr(self, k, v)
        self.ns = int(self.sp_weights.size)
        self.n_cells = int(self.sample_j.size)
        self.n_indiv = self.n_cells * self.per_cell
        from .forcing import PLANET_OMEGA
        self.day_seconds = float(day_seconds) if day_seconds else 2 * np.pi / PLANET_OMEGA
        self.soil_cap = float(soil_cap) if soil_cap is not None else _envf("QD_ECO_SOIL_WATER_CAP", 50.0)
        # QD_ECO_F32=1: keep the [N, NB] coefficient table as f32 on the device (BASELINE configs[4] "f32 mixed precision")
        self.f32_storage = (_envi("QD_ECO_F32", 0) == 1) if f32_storage is None else bool(f32_storage)
        self.daily = None                  # an IndividualDaily once step_daily runs on the device
        self.configure()

    def configure(self, **star_kw):
        d = self._dev
        specA, specB, tray = (np.ascontiguousarray(a, dtype=np.float64) for a in sp.star_band_weights(self.bands, **star_kw))
        sj, si, ci = (np.ascontiguousarray(a, dtype=np.int32) for a in (self.sample_j, self.sample_i, self.indiv_cell_index))
        Ab = np.ascontiguousarray(self.indiv_Ab, dtype=np.float64)
        tol = np.ascontiguousarray(self.indiv_tol, dtype=np.float64)
        d._chk(d.lib.qd_indiv_configure(d.h, self.n_cells, sj.ctypes.data_as(_ip), si.ctypes.data_as(_ip), self.n_indiv,
                                        ci.ctypes.data_as(_ip), Ab.ctypes.data, tol.ctypes.data, self.nb, specA.ctypes.data_as(_dp),
                                        specB.ctypes.data_as(_dp), tray.ctypes.data_as(_dp), self.substeps_per_day,
                                        self.day_seconds, self.soil_cap, 1 if self.f32_storage else 0), "qd_indiv_configure")
        if self.daily is not None:                                                      # the device dropped it with the old pool
            self.daily.configure()

    def step_daily(self, eco_adapter, soil_W_land, Ts_map=None, day_length_hours=24.0):
        """individuals.py:193-361 on the device, with the reference's arguments (Ts_map and day_length_hours are unused there
        too): soil_W_land None = zeros, a scalar, or a [lat, lon] soil index (another shape falls back to its nanmean)."""
        pop = getattr(eco_adapter, "pop", None)
        if pop is None:
            self.reset()
            return
        if self.daily is None:
            IndividualDaily(self, pop)
        shape = (self.h, self.w)
        if soil_W_land is None:
            soil = np.zeros(shape)
        elif np.isscalar(soil_W_land):
            soil = np.full(shape, float(soil_W_land))
        else:
            soil = np.asarray(soil_W_land, dtype=float)
            if soil.shape != shape:
                soil = np.full(shape, float(np.nanmean(soil)))
        self._dev.indiv_daily_step(soil)

    def try_substep(self, isr_A=None, isr_B=None, eco_adapter=None, soil_W_land=None, dt_seconds=300.0, day_length_seconds=None):
        """individuals.py:142-191 on the resident ISR_A / ISR_B / W_LAND (arrays given here are uploaded first; `soil_W_land`
        is the soil INDEX the reference driver passes, so it is uploaded scaled back by the cap).  Returns True when a
        sub-step fired."""
        d = self._dev
        if isr_A is not None:
            d.set("ISR_A", isr_A)
        if isr_B is not None:
            d.set("ISR_B", isr_B)
        if soil_W_land is not None:
            d.set("W_LAND", np.asarray(soil_W_land, dtype=np.float64) * max(1e-6, self.soil_cap))
        d.flush()
        fired = ctypes.c_int32(0)
        d._chk(d.lib.qd_indiv_substep(d.h, float(dt_seconds), ctypes.byref(fired)), "qd_indiv_substep")
        return bool(fired.value)

    def _pull(self):
        E, S = np.empty(self.n_indiv), np.empty(self.n_indiv)
        self._dev._chk(self._dev.lib.qd_indiv_download(self._dev.h, E.ctypes.data, S.ctypes.data), "qd_indiv_download")
        return E, S

    @property
    def indiv_E_day(self):
        return self._pull()[0]

    @property
    def indiv_water_stress_days(self):
        return self._pull()[1]

    def reset(self, E_day=None, stress_days=None):
        """What the daily step does to the buffers (individuals.py:207-208 and the end of step_daily)."""
        E = np.zeros(self.n_indiv) if E_day is None else np.ascontiguousarray(E_day, dtype=np.float64)
        S = np.zeros(self.n_indiv) if stress_days is None else np.ascontiguousarray(stress_days, dtype=np.float64)
        self._dev._chk(self._dev.lib.qd_indiv_upload(self._dev.h, E.ctypes.data, S.ctypes.data), "qd_indiv_upload")
