"""NumPy restatement of the individuals' daily step (test infrastructure) in the stages the device kernels
(qingdai_amd/csrc/qd_indiv_daily.hip) run: per-cell tables, the exact median, the cell loop level by level, the stack pass with
the species weights, the seed bank, the individuals' buffers.  The goldens tests/golden/indiv_daily_*_19x36.npz, made by the
reference's own IndividualPool.step_daily behind its PopulationManager.step_daily, pin it bitwise -- which is the proof that running
the levels of `plan_levels` in ascending order is the sequential cell loop.

`Cfg.from_env(env, lai_max)` reads a dict of QD_ECO_* strings with the reference's defaults; `step_daily(st, cfg, soil, levels)`
advances a `State` in place and returns {beta_hint, medE, denom}.  `levels=None` runs the cells one after the other (the loop as
written); `probe`, when a dict, collects the smallest distance of every compared quantity from its threshold."""
from dataclasses import dataclass

import numpy as np

from eco_daily_ref import _near


def np_sum(a):
    """np.sum over a contiguous run of n <= 128 doubles, spelled out: fewer than eight terms one after the other from 0, else
    eight interleaved partial sums combined as a tree and the n mod 8 last terms one by one."""
    a = [np.float64(x) for x in a]
    n = len(a)
    if n < 8:
        r = np.float64(0.0)
        for x in a:
            r = r + x
        return r
    r = a[:8]
    n8 = n - n % 8
    for i in range(8, n8, 8):
        for q in range(8):
            r[q] = r[q] + a[i + q]
    res = ((r[0] + r[1]) + (r[2] + r[3])) + ((r[4] + r[5]) + (r[6] + r[7]))
    for i in range(n8, n):
        res = res + a[i]
    return res


def pymax(a, b):
    """Python's max(a, b): b only when b > a."""
    return b if b > a else a


def spill_targets(j, i, H, W):
    jn = [max(0, j - 1), min(H - 1, j + 1), j, j]
    in_ = [(i - 1) % W, (i + 1) % W, i, i]
    return list(zip(jn, in_))


@dataclass
class Cfg:
    stress_penalty: float = 0.2
    lai_grow: float = 0.002
    lai_decay: float = 0.001
    recruit_frac: float = 0.2
    seed_couple: bool = True
    stress_decay: float = 0.5
    repro_frac: float = 0.2
    seed_energy: float = 1.0
    retain: float = 0.2
    bank_max: float = 1000.0
    lai_max: float = 5.0

    @staticmethod
    def from_env(env):
        f = lambda k, d: float(env.get(k, d))
        return Cfg(f("QD_ECO_INDIV_STRESS_PENALTY", 0.2), f("QD_ECO_LAI_GROWTH_RATE", 0.002), f("QD_ECO_LAI_DECAY_RATE", 0.001),
                   f("QD_ECO_LAI_RECRUIT_FRAC", 0.2), int(env.get("QD_ECO_INDIV_SEED_COUPLE", "1")) == 1,
                   f("QD_ECO_INDIV_STRESS_DECAY", 0.5), f("QD_ECO_REPRO_FRACTION", 0.2), f("QD_ECO_SEED_ENERGY", 1.0),
                   f("QD_ECO_SEED_BANK_RETAIN", 0.2), f("QD_ECO_SEED_BANK_MAX", 1000.0), f("QD_ECO_LAI_MAX", 5.0))


@dataclass
class State:
    land: np.ndarray           # bool [lat, lon]
    layers: np.ndarray         # [S, K, lat, lon]
    bank: np.ndarray           # [lat, lon]
    sample_j: np.ndarray
    sample_i: np.ndarray
    per_cell: int
    species: np.ndarray        # [N]
    tol: np.ndarray            # [N]
    E: np.ndarray              # [N]
    stress: np.ndarray         # [N]
    LAI: np.ndarray = None
    weights: np.ndarray = None


def cell_tables(st, c):
    """Stage 1 -> (W [C, S], mean_stress [C, S], denom [C]).  The tables are built [S, C] as the reference lays them out, so
    that np.sum(axis=0) runs in its order: over s one after the other -- except for C == 1, where the [S, 1] table is one
    contiguous run and the sum takes np_sum's order."""
    S, C, pc = st.layers.shape[0], len(st.sample_j), st.per_cell
    Es, Ss, Nn = np.zeros((S, C)), np.zeros((S, C)), np.zeros((S, C))
    cell = np.repeat(np.arange(C), pc)
    np.add.at(Es, (st.species, cell), st.E)                    # sequential: a cell's individuals in their order
    np.add.at(Ss, (st.species, cell), st.stress)
    np.add.at(Nn, (st.species, cell), 1.0)
    with np.errstate(invalid="ignore", divide="ignore", over="ignore"):
        denom = np.sum(Es, axis=0) + 1e-12
        Wt = Es / denom[None, :]
        mean = np.zeros((S, C))
        if c.stress_penalty > 0.0:
            mean = np.divide(Ss, Nn, out=np.zeros_like(Ss), where=Nn > 0)
            Wt = Wt * (1.0 / (1.0 + c.stress_penalty * mean))
            Wt = Wt / (np.sum(Wt, axis=0) + 1e-12)[None, :]
    return np.ascontiguousarray(Wt.T), np.ascontiguousarray(mean.T), denom


def median_positive(denom):
    """Stage 2: np.median(denom[denom > 0]) by the two middle order statistics, 1.0 when none."""
    d = np.sort(denom[denom > 0])
    if d.size == 0:
        return 1.0
    return float(d[(d.size - 1) // 2]) if d.size % 2 else float((d[d.size // 2 - 1] + d[d.size // 2]) / 2.0)


def one_cell(L, ci, j, i, wk, ms, denom_c, medE, c, probe=None):
    """Stage 3 for one sampled cell on the stack L (np.maximum(stack, 0) applied where a value is read or added to)."""
    S, K, H, W = L.shape
    with np.errstate(invalid="ignore", divide="ignore", over="ignore"):
        col = np.maximum(L[:, :, j, i], 0.0)
        total_k = [np_sum(col[:, 0])] if K == 1 else [sum((col[s, k] for s in range(S)), np.float64(0.0)) for k in range(K)]
        total_old = np_sum(total_k)
        e_scaled = denom_c / (medE + 1e-12)
        msc = np_sum(ms * wk) if c.stress_penalty > 0.0 else 0.0
        dLAI = c.lai_grow * (e_scaled - 1.0) - c.lai_decay * msc
        dLAI = dLAI * pymax(total_old, 1.0)
        raw = total_old + dLAI
        _near(probe, "total_vs_lai_max", raw, c.lai_max)
        _near(probe, "total_vs_0", raw, 0.0, scale=c.lai_max)
        new_total = float(np.clip(raw, 0.0, c.lai_max))
        scale = new_total / (total_old + 1e-12) if total_old > 0.0 else new_total / pymax(c.lai_max, 1.0)
        for k in range(K):
            new_k = total_k[k] * scale
            L[:, k, j, i] = 0.0 if new_k <= 0.0 else wk * new_k
        _near(probe, "growth_vs_0", new_total - total_old, 0.0, scale=c.lai_max)
        recruit = pymax(0.0, new_total - total_old) * c.recruit_frac
        if recruit > 0.0:
            add = (recruit / 4.0) / float(max(K, 1))
            for jj, ii in spill_targets(j, i, H, W):
                for k in range(K):
                    L[:, k, jj, ii] = np.maximum(L[:, k, jj, ii], 0.0) + wk * add


def step_daily(st, c, soil, levels=None, probe=None):
    S, K, H, W = st.layers.shape
    C = len(st.sample_j)
    Wt, mean, denom = cell_tables(st, c)
    medE = median_positive(denom)
    order = range(C) if levels is None else np.argsort(np.asarray(levels), kind="stable")
    L = st.layers
    for ci in order:
        one_cell(L, ci, int(st.sample_j[ci]), int(st.sample_i[ci]), Wt[ci], mean[ci], denom[ci], medE, c, probe)
    # stage 4: the whole stack
    _near(probe, "layer_vs_lai_max", L, c.lai_max)
    st.layers = np.clip(np.maximum(L, 0.0), 0.0, c.lai_max)
    st.LAI = np.sum(np.sum(st.layers, axis=0), axis=0)
    L_s = np.sum(np.maximum(st.layers, 0.0), axis=1)
    totals = np.array([float(np.nansum(L_s[s][st.land])) for s in range(S)])
    ssum = float(np.sum(totals))
    with np.errstate(invalid="ignore", divide="ignore"):
        st.weights = np.full((S,), 1.0 / float(S)) if ssum <= 0 else np.clip(totals / ssum, 0.0, 1.0)
    # stage 5: the seed bank
    if c.seed_couple:
        with np.errstate(invalid="ignore", over="ignore"):
            seeds = c.retain * (np.maximum(0.0, c.repro_frac) * np.maximum(0.0, denom) / max(c.seed_energy, 1e-12))
            for ci in range(C):
                j, i = int(st.sample_j[ci]), int(st.sample_i[ci])
                _near(probe, "bank_vs_bank_max", st.bank[j, i] + seeds[ci], c.bank_max)
                st.bank[j, i] = np.clip(st.bank[j, i] + seeds[ci], 0.0, c.bank_max)
    # stage 6: the individuals
    soil = np.asarray(soil, dtype=float)
    soil_n = np.repeat(soil[st.sample_j, st.sample_i], st.per_cell)
    _near(probe, "soil_vs_tol", soil_n - st.tol, 0.0)
    ok = soil_n >= st.tol
    st.E = np.zeros_like(st.E)
    _near(probe, "stress_vs_365", st.stress[~ok] + 1.0, 365.0)
    st.stress = np.where(ok, st.stress * c.stress_decay, np.minimum(st.stress + 1.0, 365.0))
    with np.errstate(invalid="ignore"):
        beta = float(np.mean(np.max(Wt, axis=1))) if C else 0.0
    return {"beta_hint": beta, "medE": medE, "denom": denom}
