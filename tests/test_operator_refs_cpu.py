"""CPU: the references of tests/test_gpu_operator_seam.py, pinned at its cases (tests/operator_cases.py) without a GPU.

The GPU test compares the device operators with the oracle's restatements where no golden file exists; this module shows that the
restatements are themselves sound at those ragged shapes: bit for bit against scipy.ndimage for the Gaussian blur and the Shapiro
filter, to rounding against a long-double direct DFT for the zonal filter.  It also pins the host-side weight table of the device
blur (qd_gauss_weights) and states the reduction reference and its bound.
"""
import math

import numpy as np
import pytest

import operator_cases as oc
from qd_oracle import atmos as oat, numerics as onx

EPS = float(np.finfo(np.float64).eps)


@pytest.mark.parametrize("shape", oc.GAUSS_SHAPES)
def test_oracle_gaussian_equals_scipy(shape):
    from scipy.ndimage import gaussian_filter
    F = oc.field(shape)
    for sigma in oc.GAUSS_SIGMAS:
        for mode in oc.GAUSS_MODES:
            assert np.array_equal(onx.gaussian_filter(F, sigma, mode), gaussian_filter(F, sigma=sigma, mode=mode)), (sigma, mode)


@pytest.mark.parametrize("shape", oc.SHAPIRO_SHAPES)
def test_oracle_shapiro_equals_scipy(shape):
    from scipy.ndimage import convolve
    F = oc.field(shape)
    k1 = np.array([0.25, 0.5, 0.25])
    for n in oc.SHAPIRO_N:
        want = F.copy()
        for _ in range(n):
            want = convolve(want, k1[np.newaxis, :], mode="wrap")
            want = convolve(want, k1[:, np.newaxis], mode="nearest")
        assert np.array_equal(onx.shapiro(F, n), want), n


def zonal_filter_longdouble(F, cutoff, damp):
    """The zonal filter as a direct DFT in long double: F - (1 - s) * (the part of F in the bins kcut .. kN).  pi is a long double;
    the phase 2 pi (j k mod n) / n is reduced in integers first."""
    ld = np.longdouble
    x = np.nan_to_num(F).astype(ld)
    n = x.shape[1]
    if damp <= 0.0 or cutoff <= 0.0 or n // 2 < 1:
        return x
    kN = n // 2
    kcut = int(max(1, min(kN, int(cutoff * kN))))
    s = max(0.0, 1.0 - min(1.0, damp))
    pi = ld(4) * np.arctan(ld(1))
    j = np.arange(n)
    high = np.zeros_like(x)
    for k in range(kcut, kN + 1):
        ang = (ld(2) * pi) * ((j * k) % n).astype(ld) / ld(n)
        c, sn = np.cos(ang), np.sin(ang)
        Xr, Xi = x @ c, -(x @ sn)
        if n % 2 == 0 and k == kN:
            high += np.outer(Xr, c)                               # Nyquist: real part only, weight 1
        else:
            high += ld(2) * (np.outer(Xr, c) - np.outer(Xi, sn))
    return x - ld(1.0 - s) * (high / ld(n))


def zonal_row_error(got, want):
    """max |got - want| per row, in units of eps * the row's max-norm of `want`."""
    want = np.asarray(want)
    d = np.max(np.abs(np.asarray(got).astype(want.dtype) - want), axis=1)
    return np.asarray(d / np.maximum(np.max(np.abs(want), axis=1), 1e-300) / EPS, dtype=float)


@pytest.mark.parametrize("shape", oc.ZONAL_SHAPES)
def test_oracle_zonal_filter_vs_longdouble_dft(shape):
    """np.fft's rfft / irfft against the long-double direct DFT: <= 64 eps of each row's max-norm.  Measured worst case over the
    table: 4.6 eps ((5, 257), cutoff 2.0, damp 2.0).  The input holds one NaN, which both scrub to 0.  The +inf of the GPU test's
    input is left out of the filtering cases here: scrubbed to DBL_MAX it overflows an f64 transform, so np.fft's own result on that
    row is a pattern of +-DBL_MAX and zeros decided by its order of summation -- no reference value exists for it.  The scrub-only
    parameter pairs keep it: there the result is nan_to_num(F) exactly."""
    assert np.finfo(np.longdouble).eps < 1e-18, "this check needs an extended-precision long double"
    F = oc.field(shape)
    F[1, shape[1] - 1] = np.nan
    worst = 0.0
    for cutoff, damp in oc.ZONAL_PARAMS:
        if (cutoff, damp) in oc.ZONAL_SCRUB_ONLY:
            P = oc.poisoned(shape)
            assert np.array_equal(oat.spectral_zonal_filter(P.copy(), cutoff, damp, shape[1]), np.nan_to_num(P))
            continue
        got = oat.spectral_zonal_filter(F.copy(), cutoff, damp, shape[1])
        e = float(zonal_row_error(got, zonal_filter_longdouble(F, cutoff, damp)).max())
        print(shape, cutoff, damp, f"{e:.2f} eps")
        worst = max(worst, e)
        assert e <= 64.0, (cutoff, damp, e)
    print("worst", worst)


def test_gauss_weights_mirror_equals_numpy_sum():
    """qd_gauss_weights divides phi by a sum it forms with eight accumulators, claiming numpy's pairwise order; the restatement of
    that sum (operator_cases.gauss_weights_mirror) equals phi / phi.sum() bit for bit for every kernel length 2 r + 1 = 1 .. 49 and
    for every sigma of the table."""
    seen = set()
    sigmas = list(oc.GAUSS_SIGMAS) + [(r + 0.1) / 4.0 for r in range(25)]           # r = 0 .. 24, each once more
    for sigma in sigmas:
        want = onx.gaussian_kernel1d(sigma)
        got = oc.gauss_weights_mirror(sigma)
        seen.add(len(want))
        assert np.array_equal(got, want), sigma
    assert seen == set(range(1, 50, 2))


def reduce_sum_bound(x):
    """The reference of QD_R_SUM is math.fsum(x), the correctly rounded sum.  The device adds in a fixed tree (qd_reduce.hip): per
    row and thread a running sum over the columns j, j + 256, ... (at most 3 additions at n_lon <= 768), 6 shuffle levels, 3 LDS
    additions by thread 0; then per thread a running sum over the row partials k, k + 256 (at most 2 at n_lat <= 512), 6 shuffle
    levels and 3 LDS additions again: no element passes through more than 23 additions, so
        |got - sum| <= 23 (eps / 2) sum|x| (1 + O(eps)).
    The tests use 64 eps sum|x|, that figure rounded up generously; it is still 1e3 to 1e5 times below the error of dropping or
    doubling a single typical element."""
    return 64.0 * EPS * math.fsum(np.abs(np.asarray(x, dtype=float)).ravel())


@pytest.mark.parametrize("shape", oc.REDUCE_SHAPES)
def test_reduce_reference_and_bound(shape):
    """The bound is meaningful: numpy's own pairwise sum sits inside it, and a sum that loses one element does not."""
    for name, x in oc.reduce_fields(shape).items():
        ref = math.fsum(x.ravel())
        b = reduce_sum_bound(x)
        assert abs(float(x.sum()) - ref) <= b, name
        flat = x.ravel()
        k = int(np.argsort(np.abs(flat))[flat.size // 2])         # a median-magnitude element
        assert abs(math.fsum(np.delete(flat, k)) - ref) > b, name


def test_tables_reach_every_form():
    want = set(oc.FORM_GROUPS)
    got = {oc.shapiro_form(s[1], n) for s in oc.SHAPIRO_SHAPES for n in oc.SHAPIRO_N}
    got |= {oc.gauss_form(s[1], sg) for s in oc.GAUSS_SHAPES for sg in oc.GAUSS_SIGMAS}
    got |= {oc.zonal_form(c, d) for c, d in oc.ZONAL_PARAMS}
    assert got == want
    assert oc.gauss_form(8, oc.GAUSS_SIGMA_COPY) is None and oc.gauss_radius(oc.GAUSS_SIGMA_REFUSED) > 24     # the two host-side exits
    # the ragged conditions the shapes were chosen for
    assert any(n_lon >= 64 and n_lat < 8 for n_lat, n_lon in oc.SHAPIRO_SHAPES)                    # shorter than the prefetch
    for npass in (1, 2, 3):
        w = 64 - 2 * npass
        assert any(n_lon >= 64 and n_lon % w == 0 for _, n_lon in oc.SHAPIRO_SHAPES), npass        # exact multiple of the strip
    assert any(n_lon >= 64 and n_lon % 62 in (1, 2) for _, n_lon in oc.SHAPIRO_SHAPES)             # last strip owns 1 or 2 lanes
    assert any(n_lon >= 64 and n_lat % 12 == 1 for n_lat, n_lon in oc.SHAPIRO_SHAPES)              # a row strip one row tall
    for r in (1, 2):
        assert any(n_lon == 256 - 2 * r for _, n_lon in oc.GAUSS_SHAPES), r                          # exactly one column block
    assert any(n_lon % 254 == 1 for _, n_lon in oc.GAUSS_SHAPES) and any(n_lon % 248 == 1 for _, n_lon in oc.GAUSS_SHAPES)
    assert any(n_lon % 256 == 1 for _, n_lon in oc.GAUSS_SHAPES)                                   # fused: one owned column
    assert any(n_lat > 8 and n_lat % 8 in range(1, 8) for n_lat, _ in oc.GAUSS_SHAPES)             # second row block, nvalid < 8
    assert any(n_lat < 24 for n_lat, _ in oc.GAUSS_SHAPES)                                         # reflect over several periods
