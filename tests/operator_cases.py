"""Case tables and seeded inputs of the isolated-operator tests (test infrastructure; not a conftest).

tests/test_operator_refs_cpu.py pins the oracle's restatements at these cases without a GPU; tests/test_gpu_operator_seam.py runs
the device operators at the same cases against the oracle.  The shapes are the ones at which a kernel changes form or its last
block / strip / lane is ragged; every earlier operator test used odd n_lat and an n_lon that is a multiple of 12.
"""
import numpy as np

# point stencils (one thread per cell, QD_BLOCK = 256 columns per workgroup): the minimum grid; even n_lat (no equator row); one
# column short of a block, exactly one block, one column past it; a third block
POINT_SHAPES = ((5, 4), (6, 9), (8, 255), (9, 256), (6, 257), (10, 600))

# Shapiro: k_shapiro_stream<NP> owns strips of 64 - 2 NP columns x 12 rows and runs when n_lon >= 64 and n <= 3
#   (6, 63)    below the threshold: k_shapiro_pass for every n
#   (5, 64)    the whole grid shorter than the cascade plus its eight-row prefetch; the last column strip owns 2 (NP = 1) lanes
#   (12, 116)  NP = 3: exactly two column strips of 58; exactly one row strip
#   (13, 120)  NP = 2: exactly two column strips of 60; the second row strip is one row tall
#   (25, 124)  NP = 1: exactly two column strips of 62; the third row strip is one row tall
#   (13, 125)  NP = 1: the third column strip owns one lane
SHAPIRO_SHAPES = ((6, 63), (5, 64), (12, 116), (13, 120), (25, 124), (13, 125))
SHAPIRO_N = (1, 2, 3, 4)            # 4: k_shapiro_pass at every shape

# Gaussian blur: radius int(4 sigma + 0.5) = 0, 1, 2, 3, 4, 5, 24
#   r = 1, 2, 4 k_gauss_rows<r> (owns 256 - 2 r columns x 8 rows); other r <= 24, r = 0 included, k_gauss_fused; n_lon <= 2 r, or
#   QD_FUSED=0, k_gauss_axis; sigma <= 1e-15 a copy and r > 24 a refusal, both decided on the host
#   (5, 8)     n_lon <= 2 r from r = 4 on; n_lat < r: the reflect / wrap extension runs over several periods
#   (9, 249)   rows<4>: second column block owns one column; second row block has one valid row
#   (24, 252)  rows<2>: exactly one column block; three full row blocks
#   (17, 254)  rows<1>: exactly one column block; third row block has one valid row
#   (8, 255)   rows<1>: second column block owns one column; exactly one row block
#   (9, 257)   fused: second column block owns one column
GAUSS_SHAPES = ((5, 8), (9, 249), (24, 252), (17, 254), (8, 255), (9, 257))
GAUSS_SIGMAS = (0.1, 0.2, 0.5, 0.75, 1.0, 1.3, 6.0)
GAUSS_MODES = ("reflect", "wrap")
GAUSS_SIGMA_REFUSED = 6.2           # r = 25 > 24
GAUSS_SIGMA_COPY = 0.0              # the exit in front of the weight table (scipy itself divides by zero here: GPU test only)

# zonal filter: even and odd n_lon (odd: no Nyquist bin), below / at / above one block of bins and columns
ZONAL_SHAPES = ((5, 4), (5, 5), (6, 63), (7, 64), (5, 255), (5, 257), (5, 600))
# (cutoff, damp): the default; kcut clamped up to 1, full damping; kcut = kN (only the last bin); cutoff and damp beyond 1;
# the two scrub-only exits
ZONAL_PARAMS = ((0.75, 0.5), (0.01, 1.0), (1.0, 0.3), (2.0, 2.0), (0.5, 0.0), (0.0, 0.5))
ZONAL_SCRUB_ONLY = ((0.5, 0.0), (0.0, 0.5))
ZONAL_TOO_LONG = (5, 6000)          # 3 n + 2 nb doubles exceed the 150 KB of LDS the kernel may ask for

# qd_reduce: stage 1 strides columns beyond 256, stage 2 strides the row partials beyond 256
REDUCE_SHAPES = ((5, 4), (7, 255), (7, 256), (9, 257), (257, 8), (257, 520))


# the kernel-group names under which the launcher times each form (qd_timing_get), and the form each case is written for: the
# launch rules of qd_shapiro_fields / qd_gaussian / qd_zonal_filter_fields restated
FORM_GROUPS = ("k_shapiro_stream", "k_shapiro_pass", "k_gauss_rows1", "k_gauss_rows2", "k_gauss_rows4", "k_gauss_fused", "k_gauss_axis",
               "k_zonal_filter", "k_scrub_field")


def shapiro_form(n_lon, n, stream=True):
    return "k_shapiro_stream" if (stream and n <= 3 and n_lon >= 64) else "k_shapiro_pass"


def gauss_radius(sigma):
    return int(4.0 * sigma + 0.5)


def gauss_form(n_lon, sigma, fused=True):
    if not sigma > 1e-15:
        return None                                            # the sigma = 0 exit: a copy, no kernel
    r = gauss_radius(sigma)                                    # r = 0 (sigma 0.1) is no exit: the general forms run with no taps
    if fused and n_lon > 2 * r:
        return f"k_gauss_rows{r}" if r in (1, 2, 4) else "k_gauss_fused"
    return "k_gauss_axis"


def zonal_form(cutoff, damp):
    return "k_zonal_filter" if (damp > 0.0 and cutoff > 0.0) else "k_scrub_field"


def seed_of(shape, salt=0):
    return 100003 * int(shape[0]) + 17 * int(shape[1]) + int(salt)


def field(shape, salt=0):
    """A smooth part plus unit noise: stencil results do not cancel to nothing, and no two columns or rows are alike."""
    n_lat, n_lon = shape
    r = np.random.default_rng(seed_of(shape, salt))
    lat = np.linspace(-0.5 * np.pi, 0.5 * np.pi, n_lat)[:, None]
    lon = np.linspace(0.0, 2.0 * np.pi, n_lon)[None, :]
    smooth = 8.0 * np.sin(lat) * np.cos(2.0 * lon) + 3.0 * np.cos(3.0 * lat) * np.sin(lon) + 5.0
    return smooth + r.normal(0.0, 1.0, shape)


def winds(shape, scale=20.0, salt=100):
    """(u, v) = scale * normal: 20 for the advection cases, 3e4 for the 'storm' that folds pole rows many times round."""
    r = np.random.default_rng(seed_of(shape, salt))
    return scale * r.normal(0.0, 1.0, shape), scale * r.normal(0.0, 1.0, shape)


def poisoned(shape, salt=0):
    """field() with one NaN and one inf, for the operators whose reference scrubs (the zonal filter)."""
    F = field(shape, salt)
    F[1, shape[1] - 1] = np.nan
    F[shape[0] - 1, 0] = np.inf
    return F


def gauss_weights_mirror(sigma):
    """NumPy restatement of qd_gauss_weights (qd_stencil.hip): phi over -r..r, the sum as numpy's pairwise sum forms it for fewer
    than 128 elements -- a plain loop below 8 elements, else eight running accumulators over the whole blocks of eight, combined
    ((0+1)+(2+3))+((4+5)+(6+7)), then the tail one by one.  Returns the full symmetric kernel phi / total."""
    r = int(4.0 * float(sigma) + 0.5)
    x = np.arange(-r, r + 1)
    phi = np.exp(-0.5 / (sigma * sigma) * x ** 2)
    m = 2 * r + 1
    if m < 8:
        tot = np.float64(0.0)
        for k in range(m):
            tot = tot + phi[k]
    else:
        acc = [phi[k] for k in range(8)]
        k = 8
        while k < m - (m % 8):
            for t in range(8):
                acc[t] = acc[t] + phi[k + t]
            k += 8
        tot = ((acc[0] + acc[1]) + (acc[2] + acc[3])) + ((acc[4] + acc[5]) + (acc[6] + acc[7]))
        while k < m:
            tot = tot + phi[k]
            k += 1
    return phi / tot


def reduce_fields(shape):
    """name -> (field, ops it is meant for).  Every field is finite; qd_reduce's behaviour on NaN / inf is not specified."""
    n_lat, n_lon = shape
    r = np.random.default_rng(seed_of(shape, 7))
    wide = r.normal(0.0, 1.0, shape) * np.exp(r.normal(0.0, 1.0, shape) * 5.0)
    neg = -np.exp(r.normal(0.0, 2.0, shape))                  # MAX / MAXABS: the -DBL_MAX identity must not come back
    pos = np.exp(r.normal(0.0, 2.0, shape))                   # MIN (as max of -x)
    last_hi = r.normal(0.0, 1.0, shape); last_hi[-1, -1] = 50.0        # the single extreme in the last column of the last row
    last_lo = r.normal(0.0, 1.0, shape); last_lo[-1, -1] = -60.0
    out = {"wide": wide, "negative": neg, "positive": pos, "last_hi": last_hi, "last_lo": last_lo}
    if n_lat > 256 and n_lon > 256:                           # column 256 of row 256: the first cell of both second strides
        s_hi = r.normal(0.0, 1.0, shape); s_hi[256, 256] = 70.0
        s_lo = r.normal(0.0, 1.0, shape); s_lo[256, 256] = -80.0
        out["stride_hi"] = s_hi; out["stride_lo"] = s_lo
    return out
