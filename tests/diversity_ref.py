"""NumPy restatement of the diversity diagnostics (the reference's pygcm/ecology/diversity.py), written for the tests: the checker
of the device kernels at shapes the goldens do not cover, and -- with `wrap` / `pole_clip` switched off -- the proof that the
goldens notice a wrong neighbourhood.  tests/test_diversity_cpu.py holds it against every golden: L_s and the Bray-Curtis map bit
for bit, alpha and the summary to 1e-15."""
import numpy as np

SHIFTS = ((-1, 0), (1, 0), (0, -1), (0, 1))          # up, down, west, east: the order the mean accumulates in


def species_lai(stack):
    """[S, K, lat, lon] -> L_s [S, lat, lon]: negative layers count as 0, planes added in k order."""
    return np.sum(np.maximum(np.asarray(stack, dtype=np.float64), 0.0), axis=1)


def alpha_map(L_s, land_mask):
    """exp(Shannon entropy) of the species shares on land cells that carry any LAI; NaN elsewhere."""
    total = np.sum(L_s, axis=0)
    where = (np.asarray(land_mask) == 1) & (total > 0)
    out = np.full(total.shape, np.nan)
    if where.any():
        share = np.ascontiguousarray(L_s[:, where]) / (total[where] + 1e-15)[None, :]      # [S, cells], C order: the sum below runs in s order
        out[where] = np.exp(-np.sum(share * np.log(share + 1e-15), axis=0))
    return out


def bray_curtis(L_s, land_mask, wrap=True, pole_clip=True):
    """Mean Bray-Curtis dissimilarity to the 4 neighbours that are land; NaN off land.  Rows stop at the poles (a pole cell is its
    own neighbour), columns are periodic.  wrap=False clips the columns instead, pole_clip=False lets the rows wrap: the two wrong
    neighbourhoods the goldens must tell from the right one."""
    S, H, W = L_s.shape
    land = np.asarray(land_mask) == 1
    total = np.sum(L_s, axis=0)
    rows, cols = np.arange(H), np.arange(W)
    acc, cnt = np.zeros((H, W)), np.zeros((H, W))
    for dr, dc in SHIFTS:
        rr = (np.clip(rows + dr, 0, H - 1) if pole_clip else (rows + dr) % H)[:, None]
        cc = ((cols + dc) % W if wrap else np.clip(cols + dc, 0, W - 1))[None, :]
        other = L_s[:, rr, cc]                      # gathered with index arrays: NumPy lays it out species-contiguous, and the sum
                                                    # over s below therefore runs in its pairwise order, as in the reference
        shared = np.sum(np.minimum(L_s, other), axis=0)
        bc = 1.0 - 2.0 * (shared / ((total + np.sum(other, axis=0)) + 1e-15))
        both = land & land[rr, cc]
        acc[both] += bc[both]
        cnt[both] += 1.0
    with np.errstate(invalid="ignore", divide="ignore"):
        out = np.where(cnt > 0, acc / cnt, np.nan)
    out[~land] = np.nan
    return out


def area_weights(lat_mesh, land_mask):
    """max(cos lat, 0) divided by its sum over land (+ 1e-15) -> [lat, lon]."""
    w = np.maximum(np.cos(np.deg2rad(lat_mesh)), 0.0)
    return w / (float(np.sum(w[np.asarray(land_mask) == 1])) + 1e-15)


def whittaker(L_s, land_mask, lat_mesh, alpha=None):
    """-> (alpha_mean, gamma_eff, beta_whittaker): the area-weighted mean alpha over land, exp(entropy) of the area-weighted
    species totals, their ratio."""
    land = np.asarray(land_mask) == 1
    alpha = alpha_map(L_s, land_mask) if alpha is None else alpha
    w = area_weights(lat_mesh, land_mask)
    alpha_mean = float(np.nansum(alpha[land] * w[land]))
    T = np.array([float(np.nansum(L_s[s][land] * w[land])) for s in range(L_s.shape[0])])
    share = T / (float(np.sum(T)) + 1e-15)
    gamma = float(np.exp(float(-np.sum(share * np.log(share + 1e-15)))))
    return alpha_mean, gamma, float(gamma / max(alpha_mean, 1e-12))


def diversity(stack, land_mask, lat_mesh):
    L_s = species_lai(stack)
    a = alpha_map(L_s, land_mask)
    return {"L_s": L_s, "alpha_map": a, "bc_local": bray_curtis(L_s, land_mask),
            "summary": np.array(whittaker(L_s, land_mask, lat_mesh, a))}


def lat_mesh(n_lat, n_lon):
    return np.repeat(np.linspace(-90.0, 90.0, n_lat)[:, None], n_lon, axis=1)
