"""GPU (-m gpu): every public operator of the seam (qd_op_*, and qd_reduce) in isolation against the oracle, at the shapes and
parameters where the launcher picks another kernel form or the last block / strip / lane is ragged (tests/operator_cases.py).
No time stepping: nothing amplifies rounding, so the bounds are the a-priori ones.

The oracle's restatements are pinned at the same cases, without a GPU, by tests/test_operator_refs_cpu.py.

Which form ran is not guessed from the shape: the handles run with kernel-group timing on, and every case asserts the launch counts
of the groups k_shapiro_stream / k_shapiro_pass, k_gauss_rows1 / 2 / 4 / k_gauss_fused / k_gauss_axis, k_zonal_filter /
k_scrub_field against the form the case was written for (operator_cases.shapiro_form / gauss_form / zonal_form).
tests/test_operator_refs_cpu.py::test_tables_reach_every_form checks that the tables, through those expectations, cover every form.

  operator family   bound (relative to the max-norm; zonal filter: per row)           worst measured (MI355X)
  point stencils    1e-13  (storm advection 1e-10)                                    0: bit-equal at every shape
  Shapiro           1e-13; stream == pass bit for bit                                 0: bit-equal
  Gaussian          1e-13; fused forms == two-launch form bit for bit                 4.9e-16  ((9, 249), sigma 6.0, wrap)
  zonal filter      4 n_lon eps                                                       0.73 n_lon eps  ((5, 5), cutoff 0.01, damp 1)
  qd_reduce         MAX / MIN / MAXABS exact; SUM / COSWEIGHTED_MEAN 64 eps sum|x|    SUM 0.77, mean 0.90 eps sum|x|
"""
import math

import numpy as np
import pytest

import operator_cases as oc
from util import relerr

pytestmark = pytest.mark.gpu

OP_TOL = 1e-13
STORM_TOL = 1e-10
EPS = float(np.finfo(np.float64).eps)
DT = 300.0
SWITCHES = ("QD_FUSED", "QD_SHAPIRO_STREAM")
GROUPS = oc.FORM_GROUPS

_HANDLES = {}          # (shape, switch or None) -> Device


@pytest.fixture(scope="module", autouse=True)
def _close_handles():
    yield
    for dev in _HANDLES.values():
        dev.close()
    _HANDLES.clear()


def handle(monkeypatch, shape, switch=None):
    """One handle per (shape, switch).  The switches are read in qd_create: the environment is set before the handle is built."""
    key = (tuple(shape), switch)
    if key not in _HANDLES:
        import qingdai_amd as qa
        for s in SWITCHES:
            monkeypatch.delenv(s, raising=False)
        if switch:
            monkeypatch.setenv(switch, "0")
        dev = qa.SphericalGrid(*shape)._ops()
        dev.timing(on=True)
        _HANDLES[key] = dev
    return _HANDLES[key]


def launches(dev):
    """{group: brackets since the last call} of the operator forms; resets the counters."""
    out = {g: dev.timing_get(g)[1] for g in GROUPS}
    dev.timing(on=True)
    return {g: n for g, n in out.items() if n}


# ---------------------------------------------------------------- point stencils
@pytest.mark.parametrize("shape", oc.POINT_SHAPES)
def test_point_stencils_vs_oracle(gpu, monkeypatch, shape):
    """laplacian atm / ocn, hyperdiffuse (row map, scalar, n_sub = 2), divergence, vorticity, advect atm / ocn / storm."""
    import qingdai_amd as qa
    import qd_oracle as qo
    from qd_oracle import atmos as oat
    dev = handle(monkeypatch, shape)
    og = qo.Grid(*shape)
    P = qa.QdParams()
    a = P.a
    cos = np.cos(np.deg2rad(og.lat_mesh))
    c02, c05, c6 = np.maximum(cos, 0.2), np.maximum(cos, 0.5), np.maximum(1e-6, cos)
    dl, dn = og.dlat_rad, og.dlon_rad
    F, T = oc.field(shape), oc.field(shape, salt=1)
    u, v = oc.winds(shape, 20.0)
    us, vs = oc.winds(shape, 3.0e4, salt=200)
    # the project's own row map: sigma4 * min(a dphi, a dlam cos)^4 / dt, cos floored at 1e-3 (qd_build_k4_tables)
    k4 = P.sigma4 * np.minimum(a * dl, a * dn * np.maximum(cos, 1e-3)) ** 4 / DT
    k4s = float(np.median(k4[:, 0]))
    want = dict(
        lap_atm=oat.laplacian_sphere(F.copy(), dl, dn, c02, a), lap_ocn=oat.laplacian_sphere(F.copy(), dl, dn, c05, a),
        hyper_row=oat.hyperdiffuse(F.copy(), k4, DT, 1, dl, dn, c02, a),
        hyper_nsub2=oat.hyperdiffuse(F.copy(), 0.5 * k4, DT, 2, dl, dn, c02, a),
        hyper_scalar=oat.hyperdiffuse(F.copy(), k4s, DT, 1, dl, dn, c02, a),
        hyper_ocn=oat.hyperdiffuse(F.copy(), k4, DT, 1, dl, dn, c05, a),
        div=og.divergence(u, v), vort=og.vorticity(u, v),
        advect_atm=oat.advect_semilag(T, u, v, DT, a, dl, dn, c6), advect_ocn=oat.advect_semilag(T, u, v, DT, a, dl, dn, c05),
    )
    got = dict(
        lap_atm=dev.op_laplacian(F), lap_ocn=dev.op_laplacian(F, ocean=True),
        hyper_row=dev.op_hyperdiffuse(F, k4, DT, 1), hyper_nsub2=dev.op_hyperdiffuse(F, 0.5 * k4, DT, 2),
        hyper_scalar=dev.op_hyperdiffuse(F, k4s, DT, 1), hyper_ocn=dev.op_hyperdiffuse(F, k4, DT, 1, ocean=True),
        div=dev.op_divvort(u, v), vort=dev.op_divvort(u, v, vort=True),
        advect_atm=dev.op_advect(T, u, v, DT), advect_ocn=dev.op_advect(T, u, v, DT, ocean=True),
    )
    worst = {k: relerr(got[k], want[k]) for k in want}
    storm = relerr(dev.op_advect(T, us, vs, DT), oat.advect_semilag(T, us, vs, DT, a, dl, dn, c6))
    print("point", shape, {k: f"{e:.2e}" for k, e in worst.items()}, f"storm {storm:.2e}")
    for k in want:
        assert float(np.max(np.abs(want[k]))) > 0.0, k          # the reference is not degenerate
    for k, e in worst.items():
        assert e < OP_TOL, (k, e)
    assert storm < STORM_TOL, storm


# ---------------------------------------------------------------- what the call seam does to an input
@pytest.mark.parametrize("shape", ((19, 36), (5, 130)))
def test_inputs_of_any_layout_equal_their_contiguous_f64_copy(gpu, monkeypatch, shape):
    """float32, Fortran-ordered and strided inputs: each operator's result is, bit for bit, the one for
    np.ascontiguousarray(x, dtype=np.float64) -- the conversion every caller of the seam used to write out by hand."""
    dev = handle(monkeypatch, shape)
    fields = (oc.field(shape), *oc.winds(shape))
    forms = {"float32": lambda x: x.astype(np.float32), "fortran": np.asfortranarray, "strided": lambda x: np.repeat(x, 2, axis=1)[:, ::2]}
    for name, form in forms.items():
        f, u, v = (form(x) for x in fields)
        assert f.dtype != np.float64 or not f.flags.c_contiguous, name
        cf, cu, cv = (np.ascontiguousarray(x, dtype=np.float64) for x in (f, u, v))
        got = (dev.op_laplacian(f), dev.op_laplacian(f, ocean=True), dev.op_advect(f, u, v, DT), dev.op_advect(f, u, v, DT, ocean=True),
               dev.op_divvort(u, v), dev.op_divvort(u, v, vort=True))
        want = (dev.op_laplacian(cf), dev.op_laplacian(cf, ocean=True), dev.op_advect(cf, cu, cv, DT), dev.op_advect(cf, cu, cv, DT, ocean=True),
                dev.op_divvort(cu, cv), dev.op_divvort(cu, cv, vort=True))
        for k, (g, w) in enumerate(zip(got, want)):
            assert np.all(np.isfinite(w)) and float(np.max(np.abs(w))) > 0.0, (name, k)
            assert np.array_equal(g, w), (name, k)
        assert f.dtype == form(fields[0]).dtype and np.array_equal(f, form(fields[0])), name      # the caller's array is left alone


# ---------------------------------------------------------------- Shapiro
@pytest.mark.parametrize("shape", oc.SHAPIRO_SHAPES)
def test_shapiro_vs_oracle_and_pass_form(gpu, monkeypatch, shape):
    from qd_oracle import numerics as onx
    dev = handle(monkeypatch, shape)
    ref = handle(monkeypatch, shape, "QD_SHAPIRO_STREAM")
    F = oc.field(shape)
    launches(dev), launches(ref)
    for n in oc.SHAPIRO_N:
        got, got_pass = dev.op_shapiro(F, n), ref.op_shapiro(F, n)
        assert launches(dev) == {oc.shapiro_form(shape[1], n): 1}, n
        assert launches(ref) == {"k_shapiro_pass": 1}, n
        e = relerr(got, onx.shapiro(F, n))
        print("shapiro", shape, n, oc.shapiro_form(shape[1], n), f"{e:.2e}", f"pass form {relerr(got_pass, onx.shapiro(F, n)):.2e}")
        assert e < OP_TOL, (n, e)
        assert np.array_equal(got, got_pass), n                  # the streaming form claims bit identity with the pass form


# ---------------------------------------------------------------- Gaussian
@pytest.mark.parametrize("shape", oc.GAUSS_SHAPES)
def test_gaussian_vs_oracle_and_two_launch_form(gpu, monkeypatch, shape):
    from qd_oracle import numerics as onx
    dev = handle(monkeypatch, shape)
    ref = handle(monkeypatch, shape, "QD_FUSED")
    F = oc.field(shape)
    launches(dev), launches(ref)
    for sigma in oc.GAUSS_SIGMAS:
        for mode in oc.GAUSS_MODES:
            got, got_axis = dev.op_gaussian(F, sigma, mode), ref.op_gaussian(F, sigma, mode)
            form, form_ref = oc.gauss_form(shape[1], sigma), oc.gauss_form(shape[1], sigma, fused=False)
            assert launches(dev) == ({form: 1} if form else {}), (sigma, mode)
            assert launches(ref) == ({form_ref: 1} if form_ref else {}), (sigma, mode)
            e = relerr(got, onx.gaussian_filter(F, sigma, mode))
            print("gauss", shape, sigma, mode, form, f"{e:.2e}")
            assert e < OP_TOL, (sigma, mode, e)
            assert np.array_equal(got, got_axis), (sigma, mode)  # every form: the same taps in the same order
            if oc.gauss_radius(sigma) == 0:
                assert np.array_equal(got, F), (sigma, mode)     # no taps: w[0] = 1
    for d in (dev, ref):                                         # sigma = 0: a device copy, no kernel
        assert np.array_equal(d.op_gaussian(F, oc.GAUSS_SIGMA_COPY), F)
        assert launches(d) == {}


@pytest.mark.parametrize("shape", (oc.GAUSS_SHAPES[0], oc.GAUSS_SHAPES[-1]))
def test_gaussian_radius_beyond_table_is_refused(gpu, monkeypatch, shape):
    """sigma = 6.2 gives r = 25 > 24: refused on the host (nothing is launched), and the handle goes on working."""
    from qingdai_amd._lib import QdError
    from qd_oracle import numerics as onx
    dev = handle(monkeypatch, shape)
    F = oc.field(shape)
    assert oc.gauss_radius(oc.GAUSS_SIGMA_REFUSED) == 25
    launches(dev)
    with pytest.raises(QdError, match="radius too large"):
        dev.op_gaussian(F, oc.GAUSS_SIGMA_REFUSED)
    assert launches(dev) == {}
    assert relerr(dev.op_gaussian(F, 1.0), onx.gaussian_filter(F, 1.0)) < OP_TOL


# ---------------------------------------------------------------- zonal filter
def zonal_check(dev, shape):
    """Bound: an n-term direct DFT has an a-priori error of n eps per phase; two phases, and a factor 2 for the rounding of the
    twiddles: 4 n_lon eps of the row's max-norm (5.3e-13 at n_lon = 600).
    The input holds one NaN and one +inf; the reference scrubs both (0, DBL_MAX).  The row with the NaN is held to the bound like
    every other row.  The row with DBL_MAX is compared exactly where the filter only scrubs; where it transforms, an f64 DFT of
    that row overflows -- np.fft's own result there is a pattern of +-DBL_MAX and zeros that its order of summation decides
    (tests/test_operator_refs_cpu.py), so no reference value exists -- and the row is only required to come back finite."""
    from qd_oracle import atmos as oat
    n_lat, n_lon = shape
    F = oc.poisoned(shape)
    inf_row = n_lat - 1
    fin = np.arange(n_lat) != inf_row
    worst = 0.0
    launches(dev)
    for cutoff, damp in oc.ZONAL_PARAMS:
        with np.errstate(all="ignore"):
            want = oat.spectral_zonal_filter(F.copy(), cutoff, damp, n_lon)
        got = dev.op_zonal_filter(F, cutoff, damp)
        assert launches(dev) == {oc.zonal_form(cutoff, damp): 1}, (cutoff, damp)
        assert np.all(np.isfinite(got)), (cutoff, damp)
        if (cutoff, damp) in oc.ZONAL_SCRUB_ONLY:
            assert np.array_equal(got, np.nan_to_num(F)), (cutoff, damp)
            assert np.array_equal(want, np.nan_to_num(F))
            continue
        rows = np.max(np.abs(want[fin]), axis=1)
        err = np.max(np.abs(got[fin] - want[fin]), axis=1) / rows
        e = float(err.max()) / (n_lon * EPS)
        print("zonal", shape, cutoff, damp, f"{float(err.max()):.2e} = {e:.2f} n eps")
        worst = max(worst, e)
        assert np.all(err <= 4.0 * n_lon * EPS), (cutoff, damp, float(err.max()))
    return worst


@pytest.mark.parametrize("shape", oc.ZONAL_SHAPES)
def test_zonal_filter_vs_oracle(gpu, monkeypatch, shape):
    zonal_check(handle(monkeypatch, shape), shape)


def test_zonal_filter_row_too_long_is_refused(gpu, monkeypatch):
    """(5, 6000): 3 n + 2 nb doubles exceed the 150 KB of LDS the kernel may ask for.  Refused on the host; the handle stays usable."""
    from qingdai_amd._lib import QdError
    from qd_oracle import numerics as onx
    shape = oc.ZONAL_TOO_LONG
    dev = handle(monkeypatch, shape)
    F = oc.poisoned(shape)
    launches(dev)
    with pytest.raises(QdError, match="row too long"):
        dev.op_zonal_filter(F, 0.75, 0.5)
    assert launches(dev) == {}
    assert np.array_equal(dev.op_zonal_filter(F, 0.5, 0.0), np.nan_to_num(F))
    G = oc.field(shape)
    assert relerr(dev.op_shapiro(G, 1), onx.shapiro(G, 1)) < OP_TOL


# ---------------------------------------------------------------- qd_reduce
def warea_tables(shape):
    """The row weights and their total as qd_api.hip's table set-up forms them: lat = linspace(-90, 90, n_lat) (start + i * step, the
    last sample forced), w[i] = max(cos(lat[i] * (pi / 180)), 0), wsum = the running sum of w[i] * n_lon in row order."""
    n_lat, n_lon = shape
    step = (90.0 - (-90.0)) / float(n_lat - 1)
    lat = np.array([-90.0 + float(i) * step for i in range(n_lat)])
    lat[-1] = 90.0
    w = np.maximum(np.cos(lat * (math.pi / 180.0)), 0.0)
    ws = 0.0
    for i in range(n_lat):
        ws += float(w[i]) * n_lon
    return w, ws


@pytest.mark.parametrize("shape", oc.REDUCE_SHAPES)
def test_reduce_all_ops(gpu, monkeypatch, shape):
    """MAX, MIN, MAXABS: exactly NumPy's.  SUM: |got - fsum(x)| <= 64 eps fsum|x| -- no element passes through more than 23
    additions of the device's fixed tree at these shapes (test_operator_refs_cpu.reduce_sum_bound has the count).
    COSWEIGHTED_MEAN: the same bound on fsum(x w) / (wsum + 1e-15)."""
    from qingdai_amd import _lib
    dev = handle(monkeypatch, shape)
    w, wsum = warea_tables(shape)
    worst_sum = worst_mean = 0.0
    for name, x in oc.reduce_fields(shape).items():
        dev.upload_now("H", x)
        assert dev.reduce("H", _lib.R_MAX) == float(x.max()), name
        assert dev.reduce("H", _lib.R_MIN) == float(x.min()), name
        assert dev.reduce("H", _lib.R_MAXABS) == float(np.abs(x).max()), name
        ref, scale = math.fsum(x.ravel()), math.fsum(np.abs(x).ravel())
        e = abs(dev.reduce("H", _lib.R_SUM) - ref) / (EPS * scale)
        xw = x * w[:, None]
        refm, scalem = math.fsum(xw.ravel()) / (wsum + 1e-15), math.fsum(np.abs(xw).ravel()) / (wsum + 1e-15)
        em = abs(dev.reduce("H", _lib.R_COSMEAN) - refm) / (EPS * scalem)
        print("reduce", shape, name, f"sum {e:.2f} eps sum|x|, cos-weighted mean {em:.2f} eps sum|x w| / wsum")
        worst_sum, worst_mean = max(worst_sum, e), max(worst_mean, em)
        assert e <= 64.0, (name, e)
        assert em <= 64.0, (name, em)
    assert np.array_equal(dev.get("H"), x)                        # the reductions read the field and leave it alone
