"""NumPy restatement of PhytoManager.step_daily (pygcm/ecology/phyto.py:339-435) for the daily-step tests.

Pinned to the reference by tests/golden/phyto_daily_*.npz (test_phyto_daily_cpu.py); the GPU tests use it where no golden exists
(721 x 1440, the resident loop).  `tab` holds the reference's tables under the golden's names without the "tab_" prefix
(`tables_from_golden`, `tables_from_host`).
"""
import numpy as np


def insolation(star, lat_deg, lon_deg):
    """Per-star insolation of one 7-scalar star row (forcing.py:85-103)."""
    lat = np.deg2rad(np.asarray(lat_deg, dtype=float))[:, None]
    lon = np.deg2rad(np.asarray(lon_deg, dtype=float))[None, :]
    sl, cl = np.sin(lat), np.cos(lat)
    out = []
    for k in (0, 3):
        cz = np.maximum(0.0, sl * np.sin(star[k + 1]) + cl * np.cos(star[k + 1]) * np.cos(star[6] + lon - star[k + 2]))
        out.append(star[k] * cz)
    return out


def tables_from_golden(z):
    return {k[4:]: (z[k].item() if z[k].ndim == 0 else np.asarray(z[k])) for k in z.files if k.startswith("tab_")}


def tables_from_host(t):
    """qingdai_amd.phyto.daily_tables -> the golden's names."""
    return dict(Kd0_b=t["Kd0_b"], kchl_b=t["kchl_b"], Apure_b=t["Apure_b"], shape_sb=t["shape_sb"], c_reflect_s=t["c_reflect_s"],
                p_reflect_s=t["p_reflect_s"], mu_max_s=t["mu_max_s"], m0_s=t["m0_s"], KN_s=t["KN_s"], Y_s=t["Y_s"], w_b=t["w_b"],
                idx_490=t["idx_490"], H_mld=t["H_mld"], lambda_centers=t["bands"].lambda_centers,
                delta_lambda=t["bands"].delta_lambda, specA=t["specA"], specB=t["specB"], T_ray=t["T_ray"], alpha_P=t["alpha_P"],
                Q10=t["Q10"], T_ref=t["T_ref"], kd_exp_m=t["kd_exp_m"], lambda_sink=t["lambda_sink_m_per_day"],
                R_remin=t["R_remin"], enable_N=int(t["enable_N"]), alpha_clip_min=t["alpha_clip_min"],
                alpha_clip_max=t["alpha_clip_max"])


def band_split(insA, insB, tab):
    """dual_star_insolation_to_bands (spectral.py:397-426)."""
    NB = len(tab["specA"])
    S_b = np.stack([(tab["specA"][b] * insA + tab["specB"][b] * insB) * tab["T_ray"][b] for b in range(NB)])
    tot = insA + insB
    ssum = np.sum(S_b, axis=0)
    pos = (ssum > 1e-12) & (tot > 1e-12)
    I_b = np.zeros_like(S_b)
    for b in range(NB):
        I_b[b][pos] = (S_b[b][pos] / ssum[pos]) * tot[pos]
    return np.nan_to_num(I_b, nan=0.0, posinf=0.0, neginf=0.0)


def step_daily(C, N, insA, insB, T_w, tab, land_mask, dt_days=1.0, lat_deg=None):
    """-> dict(C, N, alpha_bands, alpha_scalar, kd490, means) after one daily step; C / N are not modified."""
    ocean = np.asarray(land_mask) == 0
    H = float(tab["H_mld"])
    I_b = band_split(insA, insB, tab)
    C_tot = np.sum(C, axis=0)
    Kd = np.clip(tab["Kd0_b"][:, None, None] + tab["kchl_b"][:, None, None] * np.power(np.maximum(C_tot, 0.0), tab["kd_exp_m"])[None],
                 1e-6, np.inf)
    x = Kd * H
    fac = np.where(x < 1e-6, 1.0 - 0.5 * x + (x ** 2) / 6.0, (1.0 - np.exp(-x)) / np.clip(x, 1e-12, None))
    Ibar = np.clip(I_b * fac, 0.0, np.inf)
    E = np.tensordot(tab["shape_sb"], Ibar * tab["delta_lambda"][:, None, None], axes=(1, 0))
    mu_max = tab["mu_max_s"][:, None, None]
    muL = np.tanh(tab["alpha_P"] * E / np.maximum(mu_max, 1e-6))
    fT = np.power(tab["Q10"], (np.asarray(T_w, dtype=float) - tab["T_ref"]) / 10.0)
    sink = float(tab["lambda_sink"]) / max(1e-6, H) if tab["lambda_sink"] > 0.0 else 0.0
    if tab["enable_N"]:
        fN = N[None] / (np.maximum(tab["KN_s"][:, None, None], 1e-12) + N[None])
        mu_grow = mu_max * muL * fT[None] * np.clip(fN, 0.0, 1.0)
    else:
        mu_grow = mu_max * muL * fT[None]
    mu = mu_grow - (tab["m0_s"][:, None, None] + sink)
    Cn = np.clip(C + mu * C * float(dt_days), 0.0, np.inf)
    Cn[:, ~ocean] = 0.0
    Nn = np.array(N, dtype=float, copy=True)
    if tab["enable_N"]:
        upt = np.sum((mu_grow * Cn) / np.maximum(tab["Y_s"][:, None, None], 1e-12), axis=0)
        Nn = np.clip(Nn + (-upt + float(tab["R_remin"])) * float(dt_days), 0.0, np.inf)
        Nn[~ocean] = 0.0
    A = np.broadcast_to(tab["Apure_b"][:, None, None], Kd.shape).astype(float)
    for s in range(C.shape[0]):
        chl = np.maximum(Cn[s], 0.0)
        p = float(tab["p_reflect_s"][s])
        term = chl if p == 1.0 else np.power(chl, p)
        A = A + (float(tab["c_reflect_s"][s]) * tab["shape_sb"][s][:, None, None]) * term[None]
    A = np.clip(A, tab["alpha_clip_min"], tab["alpha_clip_max"])
    a_s = np.clip(np.sum(A * tab["w_b"][:, None, None], axis=0), tab["alpha_clip_min"], tab["alpha_clip_max"])
    kd490 = Kd[int(tab["idx_490"])]
    n_lat = C.shape[1]
    lat = np.linspace(-90.0, 90.0, n_lat) if lat_deg is None else np.asarray(lat_deg)
    w = np.broadcast_to(np.maximum(np.cos(np.deg2rad(lat)), 0.0)[:, None], C.shape[1:])
    ws = float(np.sum(w)) + 1e-15
    means = [float(np.sum(np.nan_to_num(f) * w) / ws) for f in (np.sum(Cn, axis=0), kd490, a_s)]
    return dict(C=Cn, N=Nn, alpha_bands=A, alpha_scalar=a_s, kd490=kd490, means=np.array(means))
