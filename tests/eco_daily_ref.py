"""NumPy restatement of the daily vegetation step (test infrastructure), written from its description -- growth and senescence,
the layered Beer-Lambert allocation, per-species neighbour / seed spread in species order, age, germination from the seed bank
and its decay -- in the operation order the device kernels (qingdai_amd/csrc/qd_eco_daily.hip) follow.  The goldens
tests/golden/eco_daily_*_19x36.npz, made by the reference's own class, pin it bitwise.

`State` holds layers [S, K, lat, lon], E_day, age, bank, gate and the land mask; `Cfg.from_env(env)` reads a dict of QD_ECO_*
strings with the reference's defaults; `step_daily(state, cfg, soil, probe=None)` advances the state in place.  `probe`, when a
dict, collects for every branch of the step the smallest distance of a compared quantity from its threshold (see `_near`)."""
from dataclasses import dataclass, field

import numpy as np

VON_NEUMANN = [(-1, 0), (0, -1), (0, 1), (1, 0)]
MOORE = [(-1, -1), (-1, 0), (-1, 1), (0, -1), (0, 1), (1, -1), (1, 0), (1, 1)]


@dataclass
class Cfg:
    lai_max: float = 5.0
    k_canopy: float = 0.5
    growth_per_j: float = 2.0e-5
    senesce_per_day: float = 0.01
    stress_thresh: float = 0.3
    stress_strength: float = 1.0
    soil_cap: float = 50.0
    repro_fraction: float = 0.2
    spread_enable: bool = False
    spread_rate: float = 0.0
    moore: bool = False
    gate_soil: bool = True
    soil_exp: float = 1.0
    upfrac: float = 0.1
    dlai_max: float = 0.02
    seed_energy: float = 1.0
    seed_scale: float = 1.0
    seedling_lai: float = 0.02
    retain: float = 0.2
    bank_max: float = 1000.0
    seed_dlai_max: float = 0.01
    germ_frac: float = 0.10
    bank_decay: float = 0.02
    modes: list = field(default_factory=list)          # per species 'seed' | 'diffusion'
    weights: np.ndarray = None                         # species_weights (sum 1)

    @staticmethod
    def from_env(env, modes, weights):
        f = lambda k, d: float(env.get(k, d))
        return Cfg(f("QD_ECO_LAI_MAX", 5.0), f("QD_ECO_LAI_K", 0.5), f("QD_ECO_LAI_GROWTH", 2.0e-5), f("QD_ECO_LAI_SENESCENCE", 0.01),
                   f("QD_ECO_SOIL_STRESS_THRESH", 0.3), f("QD_ECO_SOIL_STRESS_GAIN", 1.0), f("QD_ECO_SOIL_WATER_CAP", 50.0),
                   f("QD_ECO_REPRO_FRACTION", 0.2), int(env.get("QD_ECO_SPREAD_ENABLE", "0")) == 1, f("QD_ECO_SPREAD_RATE", 0.0),
                   env.get("QD_ECO_SPREAD_NEIGHBORS", "vonNeumann").strip().lower() in ("moore", "8", "8n"),
                   int(env.get("QD_ECO_SPREAD_GATE_SOIL", "1")) == 1, f("QD_ECO_SPREAD_SOIL_EXP", 1.0), f("QD_ECO_LAYER_UPFRAC", 0.1),
                   f("QD_ECO_SPREAD_DLAI_MAX", 0.02), f("QD_ECO_SEED_ENERGY", 1.0), f("QD_ECO_SEED_SCALE", 1.0),
                   f("QD_ECO_SEEDLING_LAI", 0.02), f("QD_ECO_SEED_BANK_RETAIN", 0.2), f("QD_ECO_SEED_BANK_MAX", 1000.0),
                   f("QD_ECO_SEED_DLAI_MAX", 0.01), f("QD_ECO_SEED_GERMINATE_FRAC", 0.10), f("QD_ECO_SEED_BANK_DECAY", 0.02),
                   [str(m) for m in modes], np.asarray(weights, dtype=float))


@dataclass
class State:
    land: np.ndarray           # bool [lat, lon]
    layers: np.ndarray         # [S, K, lat, lon]
    E_day: np.ndarray
    age: np.ndarray
    bank: np.ndarray
    gate: np.ndarray

    def total(self):
        return np.sum(self.layers, axis=(0, 1))

    def summary(self):
        L = self.total()[self.land]
        if L.size == 0:
            return {"LAI_min": 0.0, "LAI_mean": 0.0, "LAI_max": 0.0}
        return {"LAI_min": float(np.min(L)), "LAI_mean": float(np.mean(L)), "LAI_max": float(np.max(L))}


def soil_index(W_land, glacier, cap):
    """The driver's soil index: clip(W_land / max(1e-6, cap), 0, 1), zero on ice sheets."""
    return np.clip(W_land / max(1e-6, cap), 0.0, 1.0) * (~(np.asarray(glacier) != 0))


def _near(probe, name, q, t, where=None, scale=1.0):
    """Record the smallest distance of q from the threshold t, relative to max(|q|, |t|) -- or, for t == 0, to `scale`, the
    quantity's natural size.  Values exactly on a zero threshold (zeros by construction: ocean, no light, no change) do not count."""
    if probe is None:
        return
    q = np.asarray(q, dtype=float)
    if where is not None:
        q = q[where]
    q = q[np.isfinite(q)]
    if t == 0.0:
        q = q[q != 0.0]
        d = np.abs(q) / scale
    else:
        d = np.abs(q - t) / np.maximum(np.abs(q), abs(t))
    if d.size:
        probe[name] = min(probe.get(name, np.inf), float(np.min(d)))


def _neighbour_sum(x, offsets, scale=None):
    out = np.zeros(x.shape, dtype=float)
    for dy, dx in offsets:
        r = np.roll(x, shift=(dy, dx), axis=(0, 1))
        out += r if scale is None else scale * r
    return out


def step_daily(st, c, soil, probe=None):
    land = st.land
    S, K = st.layers.shape[:2]
    soil = np.asarray(soil, dtype=float)
    sc = np.clip(soil, 0.0, 1.0)
    rf = float(np.clip(c.repro_fraction, 0.0, 0.95))
    E = np.nan_to_num(st.E_day)
    growth = np.where(land, c.growth_per_j * ((1.0 - rf) * E), 0.0)
    _near(probe, "soil_vs_stress_thresh", sc, c.stress_thresh, land)
    sen = np.where(land, c.senesce_per_day * c.stress_strength * np.maximum(0.0, c.stress_thresh - sc), 0.0)
    st.gate = np.where(land, sc ** c.soil_exp, 0.0) if c.gate_soil else land.astype(float)

    if K > 1:
        prev = np.maximum(st.layers, 0.0)
        by_k = np.sum(prev, axis=0)
        I_in = E
        cap = np.zeros((K,) + land.shape)
        for k in range(K):
            T = np.exp(-c.k_canopy * by_k[k])
            cap[k] = I_in * (1.0 - T)
            I_in = I_in * T
        cap_sum = np.sum(cap, axis=0)
        _near(probe, "cap_sum_vs_0", cap_sum, 0.0)
        tot = np.sum(prev, axis=(0, 1))
        _near(probe, "LAI_vs_0", by_k, 0.0, scale=c.lai_max)
        with np.errstate(invalid="ignore", divide="ignore"):
            w_sk = np.where(by_k[None] > 0.0, prev / (by_k[None] + 1e-12), 1.0 / float(S))
            wcap = cap / (cap_sum[None] + 1e-12)
            wsen = np.where(tot[None, None] > 0.0, prev / (tot[None, None] + 1e-12), 1.0 / float(S * K))
        no_cap = cap_sum <= 0.0
        g = np.zeros_like(prev)
        eq = growth / float(K) / float(S)
        for s in range(S):
            for k in range(K):
                g[s, k] = np.where(no_cap, eq, w_sk[s, k] * wcap[k] * growth)
        raw = prev + g - wsen * sen[None, None]
        _near(probe, "LAI_vs_0", raw, 0.0, scale=c.lai_max)
        _near(probe, "LAI_vs_lai_max", raw, c.lai_max)
        st.layers = np.clip(raw, 0.0, c.lai_max)
        if c.upfrac > 0.0:
            for s in range(S):
                for k in range(K - 1, 0, -1):
                    d = c.upfrac * np.maximum(0.0, st.layers[s, k] - st.layers[s, k - 1])
                    st.layers[s, k] -= d
                    st.layers[s, k - 1] += d
    # K == 1: growth and senescence move only an aggregate that the refresh below overwrites from the unchanged layers

    rate = float(max(0.0, min(0.5, c.spread_rate)))
    if c.spread_enable and c.spread_rate > 0.0 and rate > 0.0:
        offsets = MOORE if c.moore else VON_NEUMANN
        nv = np.zeros(land.shape)
        for dy, dx in offsets:
            nv += np.roll(land, shift=(-dy, -dx), axis=(0, 1)).astype(float)
        for s in range(S):
            gate = np.where(land, np.clip(st.gate, 0.0, 1.0), 0.0)
            Ls = np.maximum(np.sum(st.layers[s], axis=0), 0.0)
            if s < len(c.modes) and c.modes[s] == "seed":
                tot = np.maximum(np.sum(st.layers, axis=(0, 1)), 0.0)
                with np.errstate(invalid="ignore", divide="ignore"):
                    sh = np.where(tot > 0.0, Ls / (tot + 1e-12), 0.0)
                seeds = np.maximum((rf * E * sh) / max(1e-12, c.seed_energy), 0.0) * land.astype(float)
                r_eff = rate * (1.0 - np.exp(-seeds / max(1e-12, c.seed_scale)))
                _near(probe, "seed_bank_vs_bank_max", st.bank + c.retain * seeds, c.bank_max)
                st.bank = np.clip(st.bank + c.retain * seeds, 0.0, c.bank_max)
                r_eff = r_eff * gate
                with np.errstate(invalid="ignore", divide="ignore"):
                    share = np.where(nv > 0.0, r_eff * seeds / (nv + 1e-12), 0.0)
                add = _neighbour_sum(share, offsets, scale=max(0.0, c.seedling_lai))
                _near(probe, "increment_vs_dmax_seed", add, c.seed_dlai_max)
                _near(probe, "increment_vs_0", add, 0.0, scale=c.seed_dlai_max)
                add = np.minimum(add, c.seed_dlai_max)
                seeded = (add > 0.0) & land
                _near(probe, "LAI_vs_lai_max", st.layers[s, 0] + add, c.lai_max, seeded)
                st.layers[s, 0][seeded] = np.clip(st.layers[s, 0][seeded] + add[seeded], 0.0, c.lai_max)
                st.age[seeded] = 0.0
            else:
                out = rate * Ls * gate
                with np.errstate(invalid="ignore", divide="ignore"):
                    share = np.where(nv > 0.0, out / (nv + 1e-12), 0.0)
                inflow = _neighbour_sum(share, offsets)
                inc = (Ls - out + inflow) - Ls
                _near(probe, "increment_vs_dmax", inc, c.dlai_max)
                _near(probe, "increment_vs_0", inc, 0.0, scale=c.dlai_max)
                capped = Ls + np.minimum(np.maximum(inc, 0.0), c.dlai_max) + np.minimum(inc, 0.0)
                _near(probe, "LAI_vs_lai_max", capped, c.lai_max, land)
                _near(probe, "LAI_vs_0", capped, 0.0, land, scale=c.lai_max)
                new = np.where(land, np.clip(capped, 0.0, c.lai_max), 0.0)
                with np.errstate(invalid="ignore", divide="ignore"):
                    fac = np.where(Ls > 0.0, new / (Ls + 1e-12), 0.0)
                st.layers[s] = np.clip(st.layers[s] * fac[None], 0.0, c.lai_max)

    tot = st.total()
    _near(probe, "LAI_vs_0", tot, 0.0, land, scale=c.lai_max)
    st.age[(np.maximum(tot, 0.0) > 0.0) & land] += 1.0
    gate = np.where(land, np.clip(st.gate, 0.0, 1.0), 0.0)
    germ = max(0.0, c.germ_frac) * st.bank * gate
    add_total = c.seedling_lai * germ
    w = c.weights / (np.sum(c.weights) + 1e-12)
    for s in range(S):
        _near(probe, "LAI_vs_lai_max", st.layers[s, 0] + w[s] * add_total, c.lai_max, land)
        st.layers[s, 0][land] = np.clip(st.layers[s, 0][land] + (w[s] * add_total)[land], 0.0, c.lai_max)
    st.bank = np.maximum(0.0, st.bank - germ)
    st.bank *= max(0.0, 1.0 - c.bank_decay)
    st.E_day = np.zeros_like(st.E_day)
    return st
