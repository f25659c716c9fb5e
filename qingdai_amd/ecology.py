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
(QD_ECO_INDIV_DAILY=1 in the driver).  The state survives a restart through the reference's files (adapter.py:284-426, 574-777;
QD_ECO_PERSIST in the driver): `EcologyAdapter.save_autosave` / `load_autosave` write and read ecology.nc (or its NPZ form),
`save_genes_json` / `load_genes_json` genes.json from a small host gene table (`Gene`), and the load rebuilds the LAI stack from the
file's one plane on the device (qd_eco_state_restore).  Speciation (adapter.py:437-515; QD_ECO_SPECIATION=1 in the driver): `Speciation`
holds the reference's draws and limits, `Gene.mutated` restates _mutate_genes draw for draw, and the split of the parent's LAI into
the new species runs on the resident stack (`PopulationCanopy.add_species_from_parent`, qd_eco_daily_speciate);
`EcologyAdapter.export_genes` writes the reference's genes_day_*.json.
"""
from __future__ import annotations

import ctypes
import glob
import json
import os
import shutil
import time
from dataclasses import dataclass, field

import numpy as np

from . import ncio
from . import spectral as sp
from ._lib import OUT, QdError, qd_eco_params, qd_eco_daily_params, qd_indiv_daily_params
from .device import Device     # Device.call(dev, symbol, ...): the classes here take whatever has a handle `h` on a library `lib` for a device


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
    daily = None                           # a PopulationDaily once the daily step runs on the device
    indiv_daily = None                     # an IndividualDaily once the individuals' daily step runs on the device

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
        self.push_layers(init=True)

    def _stack_clock(self):
        """What has changed the resident stack so far: firings of the vegetation step and of the individuals' step."""
        return (self._dev.eco_daily_firings(), self._dev.indiv_daily_firings())

    # -- species weights: recomputed on the device by every firing of the individuals' daily step (population.py:343-359)
    @property
    def species_weights(self):
        if self.indiv_daily is not None:
            fired = self._dev.indiv_daily_firings()
            if fired and fired != self._weights_at:
                self._weights, self._weights_at = self._dev.indiv_daily_weights(self._weights.size), fired
        return self._weights

    @species_weights.setter
    def species_weights(self, w):
        self._weights = w
        self._weights_at = self._dev.indiv_daily_firings() if self.indiv_daily is not None else 0

    # -- LAI
    @property
    def LAI_layers_SK(self):
        """[S, K, lat, lon]; with a device daily step the resident stack is the truth and is downloaded."""
        if self.daily is not None:
            fired = self._stack_clock()                        # the device's own counts: firings of a span or of a direct call alike
            if fired != self._layers_at:
                self._layers, self._layers_at = self._dev.eco_daily_get_layers(self.Ns, self.K), fired
        return self._layers

    @LAI_layers_SK.setter
    def LAI_layers_SK(self, layers):
        self._layers = layers
        self._layers_at = self._stack_clock() if self.daily is not None else 0

    def push_layers(self, layers=None, init=False):
        """Hand the (changed) [S, K, lat, lon] stack to the device: what the daily step does once per planet-day."""
        if layers is not None:
            self.LAI_layers_SK = np.asarray(layers, dtype=np.float64)
        a = np.ascontiguousarray(self.LAI_layers_SK, dtype=np.float64)
        if a.shape[-2:] != self.shape:
            raise ValueError(f"LAI layers: expected [..., {self.shape[0]}, {self.shape[1]}], got {a.shape}")
        Device.call(self._dev, "qd_eco_set_lai_layers", a, np.prod(a.shape[:-2]), bool(init))
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

    # -- one speciation event (population.py:361-387) on the resident stack
    def add_species_from_parent(self, parent_idx, frac=0.02):
        """Split clip(frac, 0, 0.5) of the parent's LAI into a new last species on the device (qd_eco_daily_speciate) and follow
        it on the host: Ns, species_weights (recomputed from the land sums), the lane's parameters and mode list -- the new index
        gets what population.py:511 gives an index the list does not hold -- and the host copy of the stack counts as stale.
        Returns the index of the new species."""
        if self.daily is None:
            raise RuntimeError("add_species_from_parent needs the device daily step (PopulationDaily): the event runs on its resident stack")
        w = self._dev.eco_daily_speciate(int(parent_idx), float(frac), self.Ns)
        self.Ns += 1
        self.species_weights = w
        self.daily.params.n_species = self.Ns
        self.daily.species_modes.append(new_species_mode(self.Ns - 1))
        self._layers_at = None
        return self.Ns - 1

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
        out = Device.call(self._dev, "qd_eco_get_state", OUT(5)).tolist()
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


def new_species_mode(index):
    """The spread mode of a species index the mode list does not hold (population.py:511)."""
    return "seed" if int(index) == 1 else "diffusion"


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

    struck = 0                             # firings of the next span's first step the host has already run through the class seam
    diag = False                           # QD_ECO_DIAG: print the line of every firing a span delivers (the driver sets it)
    indiv_daily = None                     # the IndividualDaily whose line per firing follows this lane's (the driver sets it)

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

    def configure(self, stack=True):
        """(Re)configure the device: parameters, modes, weights, the current layers; age, seed bank, log and firing count to zero.
        stack=False leaves the resident stack as the device holds it (zeros after a change of the plane count): the caller fills it,
        and the host copy counts as stale."""
        pop = self.pop
        layers = np.ascontiguousarray(pop.LAI_layers_SK, dtype=np.float64) if stack else None
        w = np.asarray(pop.species_weights, dtype=float)
        w = w / (np.sum(w) + 1e-12)                                                     # population.py:571-572
        mode = [1 if str(m).lower() == "seed" else 0 for m in self.species_modes]
        self.dev.eco_daily_configure(self.params, mode, w)
        self.n_firings = 0
        pop.daily = self
        if stack:
            pop.LAI_layers_SK = layers
            self.dev.eco_daily_set_layers(layers.reshape((-1,) + self.shape))
        else:
            pop._layers_at = None
        self.dev.upload_now("ECO_GATE", pop.land.astype(float))                         # population.py:171
        if getattr(pop, "indiv_daily", None) is not None:                               # the device dropped it with the old stack
            pop.indiv_daily.configure()

    def resize(self, n_species, stack=True):
        """An autosave file with another species count (adapter.py:745-752): the lane is configured again for it.  The reference
        keeps the mode list it drew for the run's own species and never extends it: an index beyond it spreads by population.py:511
        (new_species_mode), which is also what a species born from a speciation event has -- so a run resumes with the modes it was
        saved with.  The caller has already given pop.Ns and pop.species_weights."""
        n = int(n_species)
        self.params.n_species = n
        self.species_modes = list(self.species_modes[:n]) + [new_species_mode(i) for i in range(len(self.species_modes), n)]
        self.configure(stack=stack)

    def _fired(self, n):
        self.n_firings += int(n)

    def schedule(self, dt, n):
        fire, self.accum_day = daily_counts(self.accum_day, dt, n, self.day_seconds)
        return fire

    # ---- span participant (Device.step_n)
    def span_clock(self):
        return (self.accum_day, self.struck)

    def span_schedule(self, t0, dt, n):
        fire = self.schedule(dt, n)
        if self.struck:                    # run by the host before this span: the accumulator moved as always, the lane stays idle
            if self.struck > fire[0]:
                raise ValueError(f"PopulationDaily: {self.struck} firings struck out of a step that has {int(fire[0])}")
            fire[0] -= self.struck
            self.struck = 0
        self.dev.eco_daily_schedule(fire)
        return int(fire.sum())

    def span_restore(self, clock):
        self.accum_day, self.struck = clock

    def span_deliver(self, dt):
        """-> the records of the span's firings, oldest first; under `diag` their lines (adapter.py:434-436) and, behind them, the
        individuals' line per firing (individuals.py:358-361): they fire together."""
        recs = self.dev.eco_daily_log()
        lines = [eco_daily_line(rec) for rec in recs] + (self.indiv_daily.lines() if self.indiv_daily is not None else [])
        if self.diag:
            for line in lines:
                print(line)
        return recs

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
class Gene:
    """One row of the host gene table: the fields the reference's Genes carries (genes.py:19-41); peaks are (center_nm, width_nm,
    height) tuples.  Only the peaks and the drought tolerance act on the run; the rest travels through genes.json."""
    identity: str = "grass"
    alloc_root: float = 0.3
    alloc_stem: float = 0.2
    alloc_leaf: float = 0.5
    leaf_area_per_energy: float = 2.0e-3
    peaks: list = field(default_factory=list)
    drought_tolerance: float = 0.3
    gdd_germinate: float = 80.0
    lifespan_days: int = 365
    provenance: str | None = None

    @staticmethod
    def from_env(prefix="QD_ECO_GENE_"):
        """Genes.from_env (genes.py:45-92): <prefix>IDENTITY, ALLOC_ROOT / _STEM / _LEAF (normalised; 0.3 / 0.2 / 0.5 when their
        sum is not positive), LEAF_AREA_PER_EN, PEAKS, DROUGHT_TOL, GDD_GERMINATE, LIFESPAN_DAYS, each with its default on a
        parse error."""
        def f(name, default):
            try:
                return float(os.getenv(prefix + name, str(default)))
            except Exception:      # noqa: BLE001
                return default
        g = Gene(identity=os.getenv(prefix + "IDENTITY", "grass").strip(), alloc_root=f("ALLOC_ROOT", 0.3),
                 alloc_stem=f("ALLOC_STEM", 0.2), alloc_leaf=f("ALLOC_LEAF", 0.5), leaf_area_per_energy=f("LEAF_AREA_PER_EN", 2.0e-3),
                 peaks=_peaks_from_env(prefix), drought_tolerance=f("DROUGHT_TOL", 0.3), gdd_germinate=f("GDD_GERMINATE", 80.0),
                 lifespan_days=int(f("LIFESPAN_DAYS", 365)))
        s = g.alloc_root + g.alloc_stem + g.alloc_leaf
        if s <= 0:
            g.alloc_root, g.alloc_stem, g.alloc_leaf = 0.3, 0.2, 0.5
        else:
            g.alloc_root /= s
            g.alloc_stem /= s
            g.alloc_leaf /= s
        g.provenance = f"env:{prefix}"
        return g

    def reflectance(self, bands):
        """reflectance_from_genes (genes.py:114-120) on `bands`."""
        return np.clip(1.0 - sp.absorbance_from_peaks(bands, self.peaks), 0.0, 1.0)

    def mutated(self, rng, bands, w_b, drift=None):
        """EcologyAdapter._mutate_genes (adapter.py:471-515), draw for draw from `rng` (None = the numpy.random module, the global
        legacy generator the reference uses): three uniform(-0.05, 0.05) for the allocations, clipped to [0.05, 0.90] and
        renormalised; per peak normal(0, 8), normal(0, 5), normal(0, 0.05) for centre, width and height with their clips; normal
        draws for drought tolerance, GDD, lifespan (int(np.clip(...))) and leaf area (multiplicative); then every centre is
        nudged by drift (None = QD_ECO_MUT_LAMBDA_DRIFT, 0.1; not a number: no nudge, like the reference's `except: pass`) towards
        the weighted band centre.  Identity <parent>_mut, no provenance."""
        rng = np.random if rng is None else rng
        root = float(np.clip(self.alloc_root + rng.uniform(-0.05, 0.05), 0.05, 0.90))
        stem = float(np.clip(self.alloc_stem + rng.uniform(-0.05, 0.05), 0.05, 0.90))
        leaf = float(np.clip(self.alloc_leaf + rng.uniform(-0.05, 0.05), 0.05, 0.90))
        tot = root + stem + leaf
        peaks = []
        for (c, w, h) in self.peaks:
            c = float(np.clip(c + rng.normal(0.0, 8.0), 380.0, 780.0))
            w = float(np.clip(w + rng.normal(0.0, 5.0), 10.0, 120.0))
            h = float(np.clip(h + rng.normal(0.0, 0.05), 0.05, 0.98))
            peaks.append((c, w, h))
        g = Gene(identity=self.identity + "_mut", alloc_root=root / tot, alloc_stem=stem / tot, alloc_leaf=leaf / tot,
                 leaf_area_per_energy=self.leaf_area_per_energy, peaks=peaks, drought_tolerance=self.drought_tolerance,
                 gdd_germinate=self.gdd_germinate, lifespan_days=self.lifespan_days)
        g.drought_tolerance = float(np.clip(g.drought_tolerance + rng.normal(0.0, 0.03), 0.05, 0.95))
        g.gdd_germinate = float(np.clip(g.gdd_germinate + rng.normal(0.0, 5.0), 10.0, 500.0))
        g.lifespan_days = int(np.clip(g.lifespan_days + rng.normal(0.0, 30.0), 30, 365 * 5))
        g.leaf_area_per_energy = float(np.clip(g.leaf_area_per_energy * (1.0 + rng.normal(0.0, 0.1)), 1e-5, 5e-2))
        try:
            lam, wb = np.asarray(bands.lambda_centers, dtype=float), np.asarray(w_b, dtype=float)
            lam_w = float(np.sum(lam * wb) / (np.sum(wb) + 1e-12))
            alpha = float(os.getenv("QD_ECO_MUT_LAMBDA_DRIFT", "0.1")) if drift is None else float(drift)
            g.peaks = [(float(np.clip(c + alpha * (lam_w - c), 380.0, 780.0)), w, h) for (c, w, h) in g.peaks]
        except Exception:      # noqa: BLE001
            pass
        return g


def genes_from_env(bands, n_species, species_modes=None):
    """The adapter's genes_list (adapter.py:84-138): one gene per species from QD_ECO_SPECIES_{i}_*, the template gene QD_ECO_GENE_*
    where that one's reflectance is not finite; identities from the spread modes ('seed' -> tree, 'diffusion' -> grass; without
    modes species 1 is the tree) unless QD_ECO_SPECIES_{i}_IDENTITY names one."""
    out = []
    for i in range(int(n_species)):
        try:
            g = Gene.from_env(f"QD_ECO_SPECIES_{i}_")
            if not np.all(np.isfinite(g.reflectance(bands))):
                raise ValueError("non-finite R_leaf")
        except Exception:      # noqa: BLE001
            g = Gene.from_env("QD_ECO_GENE_")
        out.append(g)
    modes = list(species_modes) if species_modes is not None else []
    for i, g in enumerate(out):
        if os.getenv(f"QD_ECO_SPECIES_{i}_IDENTITY"):
            continue
        mode = modes[i] if (i < len(modes) and modes[i] in ("seed", "diffusion")) else ("seed" if i == 1 else "diffusion")
        g.identity = "tree" if mode == "seed" else "grass"
    return out


def genes_document(genes, bands, w_b, species_weights, day_value=None):
    """The schema-3 document of save_genes_json (adapter.py:300-346)."""
    table = []
    for i, g in enumerate(genes):
        table.append({
            "index": i, "identity": g.identity, "provenance": g.provenance, "alloc_root": float(g.alloc_root),
            "alloc_stem": float(g.alloc_stem), "alloc_leaf": float(g.alloc_leaf), "leaf_area_per_energy": float(g.leaf_area_per_energy),
            "drought_tolerance": float(g.drought_tolerance), "gdd_germinate": float(g.gdd_germinate),
            "lifespan_days": int(g.lifespan_days), "peaks_model": "gaussian",
            "peaks": [{"center_nm": float(c), "sigma_nm": float(w), "variance_nm2": float(float(w) * float(w)), "height": float(h)}
                      for (c, w, h) in g.peaks]})
    doc = {"schema_version": 3, "source": "PyGCM.EcologyAdapter.save_genes_json",
           "day": float(day_value) if day_value is not None else None,
           "bands": {"nbands": int(bands.nbands), "band_weights": [float(x) for x in np.asarray(w_b, dtype=float).tolist()]},
           "genes": table}
    weights = [float(x) for x in np.asarray(species_weights, dtype=float).tolist()] if species_weights is not None else []
    if weights:
        doc["species_weights"] = weights
    return doc


def genes_from_document(doc):
    """The gene table of load_genes_json (adapter.py:370-401): sigma_nm where it is positive, else sqrt(max(0, variance_nm2));
    allocations normalised; a peak that does not parse is dropped."""
    out = []
    for rec in doc.get("genes", []):
        peaks = []
        for pk in rec.get("peaks", []) or []:
            try:
                sigma = float(pk.get("sigma_nm", 0.0))
                if sigma <= 0 and "variance_nm2" in pk:
                    sigma = float(np.sqrt(max(0.0, float(pk.get("variance_nm2", 0.0)))))
                peaks.append((float(pk.get("center_nm", 0.0)), sigma, float(pk.get("height", 0.0))))
            except Exception:      # noqa: BLE001
                continue
        g = Gene(identity=str(rec.get("identity", "sp")), alloc_root=float(rec.get("alloc_root", 0.3)),
                 alloc_stem=float(rec.get("alloc_stem", 0.2)), alloc_leaf=float(rec.get("alloc_leaf", 0.5)),
                 leaf_area_per_energy=float(rec.get("leaf_area_per_energy", 2.0e-3)), peaks=peaks,
                 drought_tolerance=float(rec.get("drought_tolerance", 0.3)), gdd_germinate=float(rec.get("gdd_germinate", 80.0)),
                 lifespan_days=int(rec.get("lifespan_days", 365)), provenance="autosave:genes_json")
        s = g.alloc_root + g.alloc_stem + g.alloc_leaf
        if s > 0:
            g.alloc_root /= s
            g.alloc_stem /= s
            g.alloc_leaf /= s
        out.append(g)
    return out


def genes_export_document(genes, bands, w_b, species_weights, day_value):
    """The schema-3 document of export_genes (adapter.py:188-281): every gene entry carries the three band arrays and, where the
    weight list reaches it, its `weight`; no top-level species_weights."""
    doc = genes_document(genes, bands, w_b, None, day_value)
    doc["source"] = "PyGCM.EcologyAdapter.export_genes"
    doc["day"] = float(day_value)
    weights = None if species_weights is None else [float(x) for x in np.asarray(species_weights, dtype=float).tolist()]
    arrays = {k: [float(x) for x in np.asarray(getattr(bands, a), dtype=float).tolist()]
              for k, a in (("lambda_centers_nm", "lambda_centers"), ("delta_lambda_nm", "delta_lambda"), ("lambda_edges_nm", "lambda_edges"))}
    for i, entry in enumerate(doc["genes"]):
        entry.update(arrays)
        if weights is not None and i < len(weights):
            entry["weight"] = weights[i]
    return doc


def genes_export_path(out_dir, day_value):
    return os.path.join(out_dir, f"genes_day_{day_value:05.1f}.json")


class Speciation:
    """The stochastic tail of EcologyAdapter.step_daily (adapter.py:437-466): after every daily firing one rand() against
    QD_ECO_MUT_RATE; on a hit below QD_ECO_SPECIES_MAX a parent drawn by species weight, the split of QD_ECO_MUT_EPS of its LAI
    into a new species on the device, the mutated gene, the new reflectance table.  rng None = the numpy.random module (the
    global legacy generator the reference draws from); np.random.RandomState(seed) gives the reference's numbers under
    np.random.seed(seed).  The rand() of a firing can be drawn ahead (`hit_ahead`) and is kept until its firing is taken, so
    looking ahead twice never draws twice; nothing else is drawn ahead."""

    def __init__(self, mut_rate=None, mut_eps=None, species_max=None, rng=None, env=None):
        env = os.environ if env is None else env

        def read(name, default, kind):
            try:
                return kind(env.get(name, str(default)))
            except Exception:      # noqa: BLE001  (adapter.py:42-53)
                return default
        self.mut_rate = read("QD_ECO_MUT_RATE", 0.0, float) if mut_rate is None else float(mut_rate)
        self.mut_eps = read("QD_ECO_MUT_EPS", 0.02, float) if mut_eps is None else float(mut_eps)
        self.species_max = read("QD_ECO_SPECIES_MAX", 8, int) if species_max is None else int(species_max)
        self.rng = rng
        self.n_done = 0                    # firings taken so far
        self._draws = {}                   # firing number (1-based) -> its rand(), drawn ahead and not yet taken
        self.n_events = 0

    def _rng(self):
        return np.random if self.rng is None else self.rng

    def hit_ahead(self, k):
        """Is the k-th firing from now (k >= 1) a hit?  Draws its rand() once.  The caller asks in firing order and stops at the
        first hit, so the generator never runs past the draws the reference has made by then."""
        if not self.mut_rate > 0.0:
            return False
        f = self.n_done + int(k)
        if f not in self._draws:
            self._draws[f] = float(self._rng().rand())
        return self._draws[f] < self.mut_rate

    def passed(self, n):
        """n firings ran inside a span; none of them was a hit (the driver ends a chunk before one)."""
        for _ in range(int(n)):
            self.n_done += 1
            if self.mut_rate > 0.0 and self._draws.pop(self.n_done, 1.0) < self.mut_rate:
                raise RuntimeError("Speciation: a firing that was drawn as a hit ran inside a span")

    def event(self, adapter):
        """What follows one daily firing -> the index of the new species, or None."""
        self.n_done += 1
        if not self.mut_rate > 0.0:
            return None
        u = self._draws.pop(self.n_done, None)
        if u is None:
            u = float(self._rng().rand())
        if not u < self.mut_rate:
            return None
        pop, rng = adapter.pop, self._rng()
        S_now = int(pop.Ns)
        if not S_now < self.species_max:
            if adapter._diag:
                print(f"[Ecology] mutation skipped: species_max={self.species_max} reached.")
            return None
        genes = adapter.genes_list                                  # (read from the environment on first use: before Ns moves)
        try:
            w = np.asarray(pop.species_weights, dtype=float)
            w = w / (np.sum(w) + 1e-12)
            parent = int(rng.choice(np.arange(S_now), p=w))
        except Exception:      # noqa: BLE001
            parent = int(rng.randint(0, max(1, S_now)))
        idx_new = pop.add_species_from_parent(parent, frac=self.mut_eps)
        try:
            g_parent = genes[parent] if parent < len(genes) else Gene.from_env()
            g_new = g_parent.mutated(rng, adapter.bands, adapter.w_b)
        except Exception:      # noqa: BLE001
            g_new = Gene.from_env()
        if idx_new >= len(genes):
            genes.append(g_new)
        else:
            genes = (genes + [g_new])[:idx_new + 1]
        adapter.genes_list = genes
        pop.set_species_reflectance_bands(np.stack([g.reflectance(adapter.bands) for g in genes], axis=0))
        self.n_events += 1
        if adapter._diag:
            print(f"[Ecology] mutation: parent={parent} \u2192 new species idx={idx_new}; Ns={len(genes)}")
        return idx_new


def persist_level(env=None):
    """QD_ECO_PERSIST (default 0): 1 writes and reads ecology.nc and genes.json with the reference's variable set; 2 adds the qd_*
    extension variables, with which the ecology lanes resume bit for bit.  A value that does not parse counts as 0."""
    env = os.environ if env is None else env
    try:
        return max(0, min(2, int(env.get("QD_ECO_PERSIST", "0"))))
    except ValueError:
        return 0


def restore_weights(w):
    """The species weights load_autosave leaves (adapter.py:748-750): clipped at 0 and divided by their sum -- in the dtype they
    arrive in, float32 from a NetCDF file -- or uniform float64 when the sum is 0."""
    w = np.clip(np.asarray(w), 0.0, None)
    ssum = float(np.sum(w))
    return (w / ssum) if ssum > 0 else np.full((int(w.size),), 1.0 / float(max(int(w.size), 1)), dtype=float)


def restore_layers(lai, weights, n_layers, lai_max):
    """The host form of qd_eco_state_restore (adapter.py:744-756), for a population whose stack lives on the host: NumPy keeps the
    dtype of `lai` through the clip, the division and the product; the store into the float64 stack widens."""
    K = max(1, int(n_layers))
    L = np.clip(lai, 0.0, lai_max)
    out = np.zeros((len(weights), K) + L.shape, dtype=float)
    for s in range(len(weights)):
        for k in range(K):
            out[s, k] = float(weights[s]) * (L / float(K))
    return out


# the [lat, lon] planes among the qd_* variables, in the order they are put back (ECO_LAI behind the stack's plane sum: after a
# firing of the individuals' step the map is summed layer by layer, which the plane-after-plane sum does not reproduce in the last bit)
EXT_PLANES = (("qd_LAI", "ECO_LAI"), ("qd_age_days", "ECO_AGE"), ("qd_seed_bank", "ECO_SEEDBANK"), ("qd_E_day", "ECO_EDAY"))


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
        self._diag = _envi("QD_ECO_DIAG", 1) == 1
        self._genes = None                 # the host gene table, built when genes.json is first written or read
        if not self.params.use_lai:        # M1 branch (adapter.py:79-80,162-166): no population, scalar leaf alpha on land
            self.species_drought_tolerance = None
            return
        self.pop = PopulationCanopy(self._dev, self.land_mask.astype(int))
        # per-species leaf reflectance and drought tolerance from the QD_ECO_SPECIES_{i}_* genes (adapter.py:90-116, genes.py:45-90)
        R, tol = species_tables(self.bands, self.pop.Ns)
        self.pop.set_species_reflectance_bands(R)
        self.species_drought_tolerance = tol

    # -- genes.json (adapter.py:284-426)
    @property
    def genes_list(self):
        """The gene table (adapter.py:84-138), read from the QD_ECO_SPECIES_{i}_* / QD_ECO_GENE_* variables on first use.  The
        identities follow the spread modes of the daily lane; without one they are drawn as the reference's population draws them."""
        if self._genes is None:
            n = self.pop.Ns if self.pop is not None else 1
            daily = getattr(self.pop, "daily", None) if self.pop is not None else None
            if daily is not None:
                modes = daily.species_modes
            elif self.pop is not None:
                modes = species_modes_from_env(n, self.pop.species_weights, bool(os.getenv("QD_ECO_SPECIES_WEIGHTS", "").strip()))
            else:
                modes = None
            self._genes = genes_from_env(self.bands, n, modes)
        return self._genes

    @genes_list.setter
    def genes_list(self, genes):
        self._genes = list(genes)

    def save_genes_json(self, path, day_value=None):
        try:
            os.makedirs(os.path.dirname(path) or ".", exist_ok=True)
        except Exception:      # noqa: BLE001
            pass
        try:
            try:
                weights = np.asarray(getattr(self.pop, "species_weights", []), dtype=float)
            except Exception:      # noqa: BLE001
                weights = None
            doc = genes_document(self.genes_list, self.bands, self.w_b, weights, day_value)
            with open(path, "w", encoding="utf-8") as f:
                json.dump(doc, f, ensure_ascii=False, indent=2)
            if self._diag:
                print(f"[Ecology] Genes autosave written: {path} (Ns={len(doc['genes'])})")
            return True
        except Exception as e:      # noqa: BLE001
            if self._diag:
                print(f"[Ecology] Genes autosave save failed: {e}")
            return False

    def export_genes(self, out_dir, day_value):
        """adapter.py:188-281: <out_dir>/genes_day_{day:05.1f}.json with the current gene table and weights; never raises."""
        try:
            os.makedirs(out_dir, exist_ok=True)
            path = genes_export_path(out_dir, day_value)
            try:
                weights = np.asarray(getattr(self.pop, "species_weights", []), dtype=float)
            except Exception:      # noqa: BLE001
                weights = None
            doc = genes_export_document(self.genes_list, self.bands, self.w_b, weights, day_value)
            with open(path, "w", encoding="utf-8") as f:
                json.dump(doc, f, ensure_ascii=False, indent=2)
            if self._diag:
                print(f"[Ecology] Genes exported: {path} (Ns={len(doc['genes'])}, schema=3)")
        except Exception as e:      # noqa: BLE001
            if self._diag:
                print(f"[Ecology] Genes export failed: {e}")

    def load_genes_json(self, path, *, on_mismatch="keep"):
        try:
            with open(path, "r", encoding="utf-8") as f:
                doc = json.load(f)
        except Exception as e:      # noqa: BLE001
            if self._diag:
                print(f"[Ecology] Genes autosave load failed: {e}")
            return False
        try:
            genes_in = genes_from_document(doc)
            if len(genes_in) == 0:
                if self._diag:
                    print("[Ecology] Genes autosave contains no genes; keeping current.")
                return False
            self.genes_list = genes_in
            try:
                R = np.stack([g.reflectance(self.bands) for g in genes_in], axis=0)
                if self.pop is not None:
                    self.pop.set_species_reflectance_bands(R)
            except Exception as e:      # noqa: BLE001
                if self._diag:
                    print(f"[Ecology] Genes reflectance rebuild failed: {e}")
            if self._diag:
                print(f"[Ecology] Genes autosave loaded: Ns={len(genes_in)} (band nb={self.bands.nbands})")
            return True
        except Exception as e:      # noqa: BLE001
            if self._diag:
                print(f"[Ecology] Genes autosave parse failed: {e}")
            return False

    # -- ecology.nc (adapter.py:574-777)
    @property
    def lai_max(self):
        daily = getattr(self.pop, "daily", None)
        return float(daily.params.lai_max) if daily is not None else _envf_any("QD_ECO_LAI_MAX", 5.0)

    def _extension_variables(self, indiv=None):
        """The qd_* variables of QD_ECO_PERSIST=2, all f8, read through the getters: -> (dims, variables)."""
        pop, d = self.pop, self._dev
        stack = np.asarray(pop.LAI_layers_SK, dtype=np.float64)
        dims = {"layer": int(stack.shape[1]), "qd_clock": 3}
        v = {"qd_LAI_layers_SK": ("f8", ("species", "layer", "lat", "lon"), stack)}
        for name, fid in EXT_PLANES:
            d._host.pop(fid, None)
            v[name] = ("f8", ("lat", "lon"), d.get(fid).copy())
        v["qd_species_weights"] = ("f8", ("species",), np.asarray(pop.species_weights, dtype=np.float64))
        v["qd_accum_day"] = ("f8", (), float(pop.daily.accum_day) if pop.daily is not None else 0.0)
        st = pop.state()
        v["qd_eco_clock"] = ("f8", ("qd_clock",), np.array([st["hours"], st["next_recompute_hours"], float(st["step_count"])]))
        if indiv is not None and indiv.n_indiv > 0:
            E, S = indiv._pull()
            dims["qd_indiv"] = int(indiv.n_indiv)
            v["qd_indiv_E_day"] = ("f8", ("qd_indiv",), E)
            v["qd_indiv_stress_days"] = ("f8", ("qd_indiv",), S)
        return dims, v

    def save_autosave(self, path_npz, day_value=None, *, extended=None, indiv=None):
        """adapter.py:574-710: `.nc` -> the reference's NetCDF layout through ncio.write_nc, anything else -> its NPZ; written to
        .<name>.tmp<ext> and moved onto the target, then copied to <name>_<UTC stamp><ext>, the copies pruned by mtime to
        QD_ECO_AUTOSAVE_KEEP (default 4), genes.json written beside it.  LAI is ECO_LAI.  extended (None = QD_ECO_PERSIST == 2)
        adds the qd_* variables to a `.nc` file; indiv names the IndividualPool whose buffers go with them."""
        try:
            out_dir = os.path.dirname(path_npz) or "."
            name, ext = os.path.splitext(os.path.basename(path_npz))
            os.makedirs(out_dir, exist_ok=True)
            ts = time.strftime("%Y%m%dT%H%M%SZ", time.gmtime())
            backup_path = os.path.join(out_dir, f"{name}_{ts}{ext}")
            tmp_path = os.path.join(out_dir, f".{name}.tmp{ext}")
            pop = self.pop
            LAI = species_w = R = None
            if pop is not None:
                LAI = pop.total_LAI()
                species_w = np.asarray(pop.species_weights, dtype=float)
                if pop._species_R_leaf is not None:
                    R = np.asarray(pop._species_R_leaf, dtype=float)
            if ext.lower() == ".nc":
                g = self.grid
                dims = {"lat": g.n_lat, "lon": g.n_lon}
                if species_w is not None:
                    dims["species"] = int(species_w.size)
                dims["band"] = int(self.bands.nbands)
                v = {"lat": ("f4", ("lat",), np.asarray(g.lat, np.float32)), "lon": ("f4", ("lon",), np.asarray(g.lon, np.float32))}
                if LAI is not None:
                    v["LAI"] = ("f4", ("lat", "lon"), np.asarray(LAI, dtype=np.float32))
                if species_w is not None:
                    v["species_weights"] = ("f4", ("species",), species_w.astype(np.float32))
                v["bands_lambda_centers"] = ("f4", ("band",), np.asarray(self.bands.lambda_centers, dtype=np.float32))
                v["bands_delta_lambda"] = ("f4", ("band",), np.asarray(self.bands.delta_lambda, dtype=np.float32))
                v["w_b"] = ("f4", ("band",), np.asarray(self.w_b, dtype=np.float32))
                if R is not None and species_w is not None:
                    v["R_species_nb"] = ("f4", ("species", "band"), R.astype(np.float32))
                if day_value is not None:
                    v["day_value"] = ("f4", (), float(day_value))
                if (persist_level() == 2 if extended is None else bool(extended)) and pop is not None:
                    xd, xv = self._extension_variables(indiv)
                    dims.update(xd)
                    v.update(xv)
                ncio.write_nc(tmp_path, dims, v, {"title": "Qingdai Ecology State", "schema_version": 1,
                                                  "source": "EcologyAdapter.save_autosave"})
                os.replace(tmp_path, path_npz)
            else:
                data = {"schema_version": np.int32(1)}
                if LAI is not None:
                    data["LAI"] = np.asarray(LAI, dtype=float)
                if species_w is not None:
                    data["species_weights"] = species_w
                data["bands_lambda_centers"] = np.asarray(self.bands.lambda_centers, dtype=float)
                data["bands_delta_lambda"] = np.asarray(self.bands.delta_lambda, dtype=float)
                data["w_b"] = np.asarray(self.w_b, dtype=float)
                if R is not None:
                    data["R_species_nb"] = R
                if day_value is not None:
                    data["day_value"] = float(day_value)
                with open(tmp_path, "wb") as f:
                    np.savez(f, **data)
                    f.flush()
                    os.fsync(f.fileno())
                os.replace(tmp_path, path_npz)
            try:
                shutil.copy2(path_npz, backup_path)
            except Exception:      # noqa: BLE001
                backup_path = None
            try:
                keep = int(os.getenv("QD_ECO_AUTOSAVE_KEEP", "4"))
                files = sorted(glob.glob(os.path.join(out_dir, f"{name}_*{ext}")), key=os.path.getmtime, reverse=True)
                for old in files[keep:]:
                    try:
                        os.remove(old)
                    except Exception:      # noqa: BLE001
                        pass
            except Exception:      # noqa: BLE001
                pass
            try:
                self.save_genes_json(os.path.join(out_dir, "genes.json"), day_value=day_value)
            except Exception:      # noqa: BLE001
                pass
            if self._diag:
                print(f"[Ecology] Autosave written: {path_npz}" + (f"; backup={backup_path}" if backup_path else ""))
            return True
        except Exception as e:      # noqa: BLE001
            if self._diag:
                print(f"[Ecology] Autosave+ load failed: {e}")          # (the reference's wording, adapter.py:709)
            return False

    def _read_autosave(self, path):
        """-> {name: array} of an autosave file: the `.nc` branch through ncio.read_nc (arrays arrive float32, as netCDF4 hands them
        to the reference), anything else through np.load."""
        if os.path.splitext(path)[1].lower() == ".nc":
            v, _ = ncio.read_nc(path)
            return v
        with np.load(path) as data:
            return {k: data[k] for k in data.files}

    def _restore_extended(self, v, indiv):
        """The qd_* variables when every shape fits -> True; touches nothing otherwise."""
        pop, d = self.pop, self._dev
        need = ("qd_LAI_layers_SK", "qd_species_weights", "qd_accum_day", "qd_eco_clock") + tuple(n for n, _ in EXT_PLANES)
        if any(n not in v for n in need):
            return False
        stack, w = np.ascontiguousarray(v["qd_LAI_layers_SK"], dtype=np.float64), np.asarray(v["qd_species_weights"], dtype=np.float64)
        if stack.ndim != 4 or stack.shape[1:] != (pop.K,) + pop.shape or w.shape != (stack.shape[0],) or np.size(v["qd_eco_clock"]) != 3:
            return False
        if any(np.shape(v[n]) != pop.shape for n, _ in EXT_PLANES):
            return False
        with_indiv = indiv is not None and indiv.n_indiv > 0
        if with_indiv != ("qd_indiv_E_day" in v) or (with_indiv and (np.shape(v["qd_indiv_E_day"]) != (indiv.n_indiv,) or
                                                                     np.shape(v.get("qd_indiv_stress_days")) != (indiv.n_indiv,))):
            return False
        self._resize(int(w.size), w)
        if pop.daily is not None:
            d.eco_daily_set_layers(stack.reshape((-1,) + pop.shape))
            pop.LAI_layers_SK = stack
            pop.daily.accum_day = float(v["qd_accum_day"])
            Device.call(d, "qd_eco_set_lai_layers", stack, stack.shape[0] * stack.shape[1], 0)
            d._host.pop("ECO_LAI", None)
        else:
            pop.push_layers(stack)
        for name, fid in EXT_PLANES:
            d.upload_now(fid, np.asarray(v[name], dtype=np.float64))
        Device.call(d, "qd_eco_set_state", np.ravel(v["qd_eco_clock"]))
        if with_indiv:
            indiv.reset(np.asarray(v["qd_indiv_E_day"], dtype=np.float64), np.asarray(v["qd_indiv_stress_days"], dtype=np.float64))
        return True

    def _resize(self, n_species, weights):
        """Give the population the file's species count and weights.  A daily lane is configured again for them -- the reference reads
        pop.species_weights in every step_daily, the device holds its own copy -- with ECO_AGE and ECO_SEEDBANK put back behind the
        configure; its resident stack is left for the caller to fill."""
        pop, d = self.pop, self._dev
        changed = int(n_species) != pop.Ns
        if pop.daily is not None:
            age, bank = pop.age_days, pop.seed_bank
        pop.Ns = int(n_species)
        pop.species_weights = weights
        if pop.daily is not None:
            if changed:
                pop.daily.resize(pop.Ns, stack=False)
            else:
                pop.daily.configure(stack=False)
            d.upload_now("ECO_AGE", age)
            d.upload_now("ECO_SEEDBANK", bank)

    def load_autosave(self, path_npz, *, on_mismatch="fallback", indiv=None, extended=None):
        """adapter.py:712-777 with the restore on the device (qd_eco_state_restore): LAI and species_weights rebuild the stack by
        the reference's rule, in the precision the file's arrays arrive in; bands and R_species_nb are taken when their band count
        is the run's.  The qd_* variables of QD_ECO_PERSIST=2, when present and fitting, win over that rule (extended=False ignores
        them).  A file whose species count differs from a run with the individuals' daily step raises (the pool was sampled for the
        run's species), and so does a latitude-band handle."""
        pop = self.pop
        if pop is None:
            return False
        try:
            v = self._read_autosave(path_npz)
            LAI, w = v.get("LAI"), v.get("species_weights")
            if LAI is None or np.ndim(LAI) != 2 or w is None or np.ndim(w) != 1:
                if self._diag:
                    print("[Ecology] Autosave+ malformed: require LAI (2D) and species_weights (1D).")
                return False
            LAI, w = np.asarray(LAI), np.asarray(w)
            if LAI.shape != pop.shape:
                raise ValueError(f"LAI is {LAI.shape}, the grid is {pop.shape}")
        except Exception as e:      # noqa: BLE001
            if self._diag:
                print(f"[Ecology] Autosave+ load failed: {e}")
            return False
        if getattr(pop, "indiv_daily", None) is not None and int(w.size) != pop.Ns:
            raise ValueError(f"the file holds {int(w.size)} species, the run {pop.Ns}, and the individuals of QD_ECO_INDIV_DAILY=1 were "
                             "sampled for the run's; starting fresh")
        try:
            has_ext = (extended is None or bool(extended)) and any(k.startswith("qd_") for k in v)
            exact = has_ext and self._restore_extended(v, indiv)
            if not exact:
                if has_ext and self._diag:
                    print("[Ecology] Autosave+: the qd_* extension variables do not fit this run -- restored by the reference rule.")
                if LAI.dtype != np.float32:                                 # float32 stays float32 (NumPy's rule); the rest is float64
                    LAI = LAI.astype(np.float64)
                weights = restore_weights(w)
                self._resize(int(weights.size), weights)
                self._dev.eco_state_restore(LAI, np.asarray(weights, dtype=np.float64), pop.K, self.lai_max)
                if pop.daily is not None:
                    pop._layers_at = None                                   # the resident stack is the truth: downloaded on the next read
                else:
                    pop.LAI_layers_SK = restore_layers(LAI, weights, pop.K, self.lai_max)
            centers, R = v.get("bands_lambda_centers"), v.get("R_species_nb")
            ok_adv = (centers is not None and len(centers) == self.bands.nbands and R is not None and np.ndim(R) == 2 and
                      R.shape[1] == self.bands.nbands)
            if ok_adv:
                pop.set_species_reflectance_bands(np.asarray(R, dtype=float))
            elif self._diag and on_mismatch != "ignore":
                print("[Ecology] Autosave+: advanced fields (bands/R_species) mismatched – restored base LAI/weights only.")
            if self._diag:
                s = pop.summary()
                print(f"[Ecology] Autosave+ loaded: LAI(min/mean/max)={s['LAI_min']:.2f}/{s['LAI_mean']:.2f}/{s['LAI_max']:.2f}; "
                      f"S={pop.Ns}, K={pop.K}, advanced={'OK' if ok_adv else 'NO'}")
                if exact:
                    print("[Ecology] Autosave+: exact resume from the qd_* extension variables.")
            return True
        except QdError:
            raise
        except Exception as e:      # noqa: BLE001
            if self._diag:
                print(f"[Ecology] Autosave+ load failed: {e}")
            return False

    def configure(self):
        Device.call(self._dev, "qd_eco_configure", self.params, ctypes.sizeof(self.params))

    def step_subdaily(self, I_total=None, cloud_eff=None, dt_seconds=300.0):
        """adapter.py:140-186.  With I_total=None the resident ISR is used (the usual case); returns the land-only alpha map
        on a sub-step boundary (downloaded), None otherwise."""
        d = self._dev
        if I_total is not None:
            d.set("ISR", I_total)
        d.flush()
        Device.call(d, "qd_eco_substep", dt_seconds)
        out = Device.call(d, "qd_eco_get_state", OUT(5))
        if int(out[2]) % max(1, self.cfg.substep_every_nphys) != 0:
            return None
        d._host.pop("ECO_ALPHA", None)
        return d.get("ECO_ALPHA").copy()

    def banded_alpha(self):
        """The driver's daily reduction (run_simulation.py:1839-1844) computed on the device and left resident in
        ECO_ALPHA_BANDED: clip(nansum_b A_b w_b, 0, 1).  Returns the host copy."""
        d = self._dev
        nb = int(self.bands.nbands)
        r = self.pop.effective_leaf_reflectance_bands(nb)
        d.flush()
        Device.call(d, "qd_eco_banded_alpha", nb, r, self.w_b)
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
        specA, specB, tray = sp.star_band_weights(self.bands, **star_kw)
        Device.call(d, "qd_indiv_configure", self.n_cells, self.sample_j, self.sample_i, self.n_indiv, self.indiv_cell_index, self.indiv_Ab,
                    self.indiv_tol, self.nb, specA, specB, tray, self.substeps_per_day, self.day_seconds, self.soil_cap, self.f32_storage)
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
        return bool(Device.call(d, "qd_indiv_substep", dt_seconds, OUT))

    def _pull(self):
        E, S = np.empty(self.n_indiv), np.empty(self.n_indiv)
        Device.call(self._dev, "qd_indiv_download", E, S)
        return E, S

    @property
    def indiv_E_day(self):
        return self._pull()[0]

    @property
    def indiv_water_stress_days(self):
        return self._pull()[1]

    def reset(self, E_day=None, stress_days=None):
        """What the daily step does to the buffers (individuals.py:207-208 and the end of step_daily)."""
        E = np.zeros(self.n_indiv) if E_day is None else E_day
        S = np.zeros(self.n_indiv) if stress_days is None else stress_days
        Device.call(self._dev, "qd_indiv_upload", E, S)
