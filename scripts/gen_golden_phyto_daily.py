"""Regenerate tests/golden/phyto_daily_*.npz from the reference's PhytoManager.step_daily (pygcm/ecology/phyto.py:339-435).

Needs a checkout of the reference project (default ../reference next to this repository, or --reference DIR).

Each golden holds the case's environment (env_keys / env_vals), the grid shape, the land mask, one star row per day (the 7 scalars
of qd_step_n: flux, declination, right ascension of each star and the rotation angle theta) with the insolation insA / insB the
forcing evaluates from it, the water temperature T_w per day, the initial C_phyto_s and N, the reference's tables, the outputs after
the FIRST and the LAST daily step (C, N, alpha_water_bands, alpha_water_scalar, Kd_490), the full-precision [PhytoDiag] means of
every day and the printed lines.
"""
import argparse
import contextlib
import io
import os
import sys
import zlib

import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))
OUT = os.path.join(HERE, "..", "tests", "golden")


def insolation(star, lat_deg, lon_deg):
    """forcing.py:85-103 for one star row (qd_star_insolation): per-star flux * max(0, cos zenith)."""
    lat = np.deg2rad(lat_deg)[:, None]
    lon = np.deg2rad(lon_deg)[None, :]
    sl, cl = np.sin(lat), np.cos(lat)
    out = []
    for k in (0, 3):
        flux, decl, ra = star[k], star[k + 1], star[k + 2]
        cz = np.maximum(0.0, sl * np.sin(decl) + cl * np.cos(decl) * np.cos(star[6] + lon - ra))
        out.append(flux * cz)
    return out


CASES = {
    # name: (n_lat, n_lon, n_days, H, env, zero-chlorophyll ocean fraction, flux B scale)
    "defaults_19x36": (19, 36, 4, 50.0, {}, 0.0, 1.0),
    "s3_custom_19x36": (19, 36, 3, 50.0, {
        "QD_PHYTO_NSPECIES": "3", "QD_PHYTO_SPEC_MU_NM": "450,560,650", "QD_PHYTO_SPEC_SIGMA_NM": "40,80,60",
        "QD_PHYTO_SPEC_C_REFLECT": "0.03,0.01,0.05", "QD_PHYTO_SPEC_P_REFLECT": "1.0,0.5,0.7",
        "QD_PHYTO_SPEC_MU_MAX": "2.0,1.2,0.8", "QD_PHYTO_SPEC_M0": "0.04,0.06,0.02", "QD_PHYTO_KN": "0.3,0.8,1.2",
        "QD_PHYTO_YIELD": "0.8,1.5,1.0", "QD_PHYTO_LAMBDA_SINK": "2.5", "QD_PHYTO_KD0": "0.03,0.05",
        "QD_PHYTO_APURE": "0.05,0.07,0.065"}, 0.0, 1.0),
    "no_n_19x36": (19, 36, 3, 50.0, {"QD_PHYTO_ENABLE_N": "0", "QD_PHYTO_NSPECIES": "4"}, 0.0, 1.0),
    # H = 0.1 m (the floor) and Kd0 = 0: cells without chlorophyll have Kd = 1e-6 and x = 1e-7 < 1e-6 (the series branch);
    # star B switched off; the night side has no light at all
    "tiny_kd_night_19x36": (19, 36, 3, 0.05, {"QD_PHYTO_KD0_DEFAULT": "0", "QD_PHYTO_NSPECIES": "3"}, 0.35, 0.0),
    "nb7_rayleigh_19x36": (19, 36, 3, 30.0, {"QD_ECO_SPECTRAL_BANDS": "7", "QD_ECO_TOA_TO_SURF_MODE": "rayleigh",
                                             "QD_PHYTO_NSPECIES": "5"}, 0.0, 1.0),
}


def S_guess(env):
    return int(env.get("QD_PHYTO_NSPECIES", "10"))


def make_case(name, ref_root):
    n_lat, n_lon, n_days, H, env, zero_frac, fluxB = CASES[name]
    keep = {k: os.environ.get(k) for k in env}
    os.environ.update(env)
    try:
        sys.path.insert(0, ref_root)
        from pygcm.ecology.phyto import PhytoManager
        from pygcm.ecology import spectral as rsp
        from pygcm.grid import SphericalGrid
        grid = SphericalGrid(n_lat, n_lon)
        rng = np.random.default_rng(zlib.crc32(name.encode()))
        lat, lon = np.deg2rad(grid.lat_mesh), np.deg2rad(grid.lon_mesh)
        # (the default case's larger continents keep its file near 200 KB: ten species and 16 bands per ocean cell)
        thr = 0.05 if S_guess(env) >= 10 else 0.45
        mask = ((np.sin(2 * lon + 0.3) * np.cos(lat) + 0.4 * np.sin(3 * lat) + 0.2 * rng.standard_normal(lat.shape)) > thr)
        mask = mask.astype(np.uint8)
        pm = PhytoManager(grid, mask, H_mld_m=H, diag=True)
        ocean = mask == 0
        S = pm.S
        C0 = np.abs(rng.lognormal(np.log(0.05 / S), 0.8, (S, n_lat, n_lon)))
        if zero_frac > 0:
            C0[:, rng.random((n_lat, n_lon)) < zero_frac] = 0.0
        C0[:, ~ocean] = 0.0
        N0 = np.where(ocean, rng.uniform(0.0, 2.0, (n_lat, n_lon)), 0.0)
        pm.C_phyto_s = C0.copy()
        pm.N = N0.copy()
        stars, insA, insB, Tw = [], [], [], []
        for d in range(n_days):
            st = np.array([1361.0 * (0.9 + 0.05 * d), 0.35 - 0.1 * d, 0.4 + 0.3 * d,
                           fluxB * 420.0 * (1.0 + 0.1 * d), -0.2 + 0.05 * d, 2.5 - 0.2 * d, 1.1 + 0.7 * d])
            a, b = insolation(st, grid.lat, grid.lon)
            stars.append(st); insA.append(a); insB.append(b)
            Tw.append(288.0 + 12.0 * np.cos(lat) ** 2 + 0.5 * rng.standard_normal(lat.shape) - 3.0 * d)
        out = {}
        means, lines = [], []
        w = np.maximum(np.cos(np.deg2rad(grid.lat_mesh)), 0.0)
        wsum = float(np.sum(w)) + 1e-15
        for d in range(n_days):
            buf = io.StringIO()
            with contextlib.redirect_stdout(buf):
                pm.step_daily(insA[d], insB[d], Tw[d], dt_days=1.0)
            lines.append(buf.getvalue().strip())
            wm = [float(np.sum(np.nan_to_num(x) * w) / wsum) for x in (np.sum(pm.C_phyto_s, axis=0), pm.Kd_490, pm.alpha_water_scalar)]
            means.append(wm)
            if d in (0, n_days - 1):
                tag = "first" if d == 0 else "last"
                out[f"{tag}_C"] = pm.C_phyto_s.copy()
                out[f"{tag}_N"] = np.asarray(pm.N, dtype=float).copy()
                out[f"{tag}_alpha_bands"] = pm.alpha_water_bands.copy()
                out[f"{tag}_alpha_scalar"] = pm.alpha_water_scalar.copy()
                out[f"{tag}_kd490"] = pm.Kd_490.copy()
        # the reference's band split weights (dual_star_insolation_to_bands with the constants' L / M ratios)
        from pygcm import constants as const
        jA, jB = float(os.getenv("QD_STAR_A_J", "0.8")), float(os.getenv("QD_STAR_B_J", "0.8"))
        TA = rsp.estimate_teff_from_LM(const.L_A / const.L_SUN, const.M_A / const.M_SUN, j=jA)
        TB = rsp.estimate_teff_from_LM(const.L_B / const.L_SUN, const.M_B / const.M_SUN, j=jB)
        data = dict(
            env_keys=np.array(list(env.keys()), dtype="U64"), env_vals=np.array(list(env.values()), dtype="U128"),
            n_lat=n_lat, n_lon=n_lon, n_days=n_days, H_arg=H, land_mask=mask, stars=np.array(stars), insA=np.array(insA),
            insB=np.array(insB), T_w=np.array(Tw), C0=C0, N0=N0, means=np.array(means), lines=np.array(lines, dtype="U256"),
            tab_Kd0_b=pm.Kd0_b, tab_kchl_b=pm.kchl_b, tab_Apure_b=pm.Apure_b, tab_shape_sb=pm.shape_sb,
            tab_c_reflect_s=pm.c_reflect_s, tab_p_reflect_s=pm.p_reflect_s, tab_mu_max_s=pm.mu_max_s, tab_m0_s=pm.m0_s,
            tab_KN_s=pm.KN_s, tab_Y_s=pm.Y_s, tab_w_b=pm.w_b, tab_idx_490=pm._idx_490, tab_H_mld=pm.H_mld,
            tab_lambda_centers=pm.bands.lambda_centers, tab_delta_lambda=pm.bands.delta_lambda,
            tab_specA=rsp.blackbody_band_weights(TA, pm.bands), tab_specB=rsp.blackbody_band_weights(TB, pm.bands),
            tab_T_ray=np.clip(rsp._rayleigh_band_factor(pm.bands), 0.0, np.inf),
            tab_alpha_P=pm.params.alpha_P, tab_Q10=pm.params.Q10, tab_T_ref=pm.params.T_ref, tab_kd_exp_m=pm.params.kd_exp_m,
            tab_lambda_sink=pm.params.lambda_sink_m_per_day, tab_R_remin=pm.R_remin, tab_enable_N=int(pm.enable_N),
            tab_alpha_clip_min=pm.alpha_clip_min, tab_alpha_clip_max=pm.alpha_clip_max, **out)
        path = os.path.join(OUT, f"phyto_daily_{name}.npz")
        np.savez_compressed(path, **data)
        print(f"{path}: {os.path.getsize(path) / 1024:.0f} KB, S={S}, NB={pm.bands.nbands}")
    finally:
        for k, v in keep.items():
            if v is None:
                os.environ.pop(k, None)
            else:
                os.environ[k] = v


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reference", default=os.path.join(HERE, "..", "..", "reference"))
    ap.add_argument("cases", nargs="*", default=list(CASES))
    a = ap.parse_args()
    for name in a.cases:
        make_case(name, os.path.abspath(a.reference))


if __name__ == "__main__":
    main()
