"""Plain NumPy restatement of what qd_topogen_build computes from qingdai_amd.topogen.build_inputs -- the stages of
pygcm/topography.py:90-276 from the same host tables, with NumPy's own (pairwise) means and the fixed-point weighted select --
so that the host side of the device path is checked against the reference's goldens without a GPU."""
import json

import numpy as np

W_BITS = 38


def case(z):
    """-> (shape, seed, params, target_land_frac) of a tests/golden/topogen_*.npz"""
    return tuple(int(x) for x in z["shape"]), int(z["seed"]), json.loads(str(z["params"])), float(z["target_land_frac"])


def _half_filter(F, w, axis, mode):
    r = len(w) - 1
    n = F.shape[axis]
    base = np.arange(n)
    ext = (lambda i: np.mod(i, n)) if mode == "wrap" else (lambda i: np.clip(i, 0, n - 1))
    out = np.take(F, base, axis=axis) * w[r]
    for k in range(r, 0, -1):
        out = out + (np.take(F, ext(base - k), axis=axis) + np.take(F, ext(base + k), axis=axis)) * w[r - k]
    return out


def _norm(x):
    return x.mean(), x.std() + 1e-8


def weighted_select(elev, area_w, target_land_frac):
    """the device's sea level: the smallest value whose cumulative fixed-point weight reaches ceil(q * total)"""
    n_lat, n_lon = elev.shape
    wfix = [int(round(float(w) * 2 ** W_BITS)) for w in area_w]
    total = sum(wfix) * n_lon
    q = 1.0 - float(target_land_frac)
    thr = 0 if q <= 0.0 else (total if q >= 1.0 else min(total, int(np.ceil(q * float(total)))))
    v = (elev + 0.0).ravel()
    order = np.argsort(v, kind="stable")
    cum = 0
    for k in order:
        cum += wfix[k // n_lon]
        if cum >= thr:
            return float(v[k])
    return float(v[order[-1]])


def build(a, shape):
    """elevation, sea level, mask from a build_inputs dict"""
    n_lat, n_lon = shape
    par, radii, weights = a["par"], a["radii"], a["weights"]
    off = np.concatenate([[0], np.cumsum(radii + 1)])
    half = lambda f: weights[off[f]:off[f + 1]]
    smooth = lambda f, F: _half_filter(_half_filter(F, half(2 * f), 0, "nearest"), half(2 * f + 1), 1, "wrap")
    h1 = np.zeros(shape)
    for (s0, c0, amp), cl in zip(a["cont"], a["cont_coslon"]):
        cosd = np.clip(a["sin_lat"][:, None] * s0 + a["cos_lat"][:, None] * c0 * cl[None, :], -1.0, 1.0)
        h1 += amp * np.exp(-(np.arccos(cosd) / par[0]) ** float(par[1]))
    m0, s0 = _norm(h1)
    vlf = smooth(0, a["noise"][0])
    m1, s1 = _norm(vlf)
    h1 = par[2] * ((h1 - m0) / s0) + par[3] * ((vlf - m1) / s1)
    m2, s2 = _norm(h1)
    fbm = np.zeros(shape)
    for o, amp in enumerate(a["oct_amp"]):
        layer = smooth(1 + o, a["noise"][1 + o])
        m, s = _norm(layer)
        fbm = fbm + amp * ((layer - m) / s)
    m4, s4 = _norm(fbm)
    comb = par[4] * ((h1 - m2) / s2) + par[5] * ((fbm - m4) / s4)
    m5, s5 = _norm(comb)
    elev = smooth(len(a["oct_amp"]) + 1, par[6] * ((comb - m5) / s5))
    sea = weighted_select(elev, a["area_w"], par[7])
    return elev, sea, (elev >= sea).astype(np.uint8)
