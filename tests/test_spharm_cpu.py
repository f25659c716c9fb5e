"""CPU: the definition of the spherical-harmonic lane (qingdai_amd/spharm.py) and its host side, without a device.

  the Clenshaw-Curtis weights; orthonormality of the f64 Legendre tables under them; the Legendre functions against scipy.special;
  a single harmonic, and a field just beyond the truncation; the round trip synthesise -> analyse_reference at seven shapes, in f64
  and in extended precision; the kinetic-energy formula on solid-body rotation; the environment parser, the refusals, the
  truncation rule, the window's variable set and the file-name rule."""
import math

import numpy as np
import pytest

SHAPES = [(5, 8), (7, 12), (19, 36), (9, 45), (20, 36), (33, 24), (131, 12)]
EPS = float(np.finfo(np.float64).eps)
RECOVERY_MEASURED = 4.3e-15          # the largest f64 recovery error measured over SHAPES when the lane was specified
A = 6.371e6


def coefficients(g, seed=1):
    """Random triangular coefficients x_n^m at [m][n], real for m = 0."""
    r = np.random.default_rng(seed)
    c = np.triu(r.normal(size=(g.N + 1, g.N + 1)) + 1j * r.normal(size=(g.N + 1, g.N + 1)))
    c[0] = c[0].real
    return c


@pytest.mark.parametrize("n_lat", [5, 6, 19, 20, 131, 721])
def test_weights_sum_to_two(n_lat):
    from qingdai_amd import spharm
    g = spharm.tables(n_lat, 12)
    assert g.w.shape == (n_lat,) and (g.w > 0).all()
    assert abs(math.fsum(g.w) - 2.0) <= 4 * EPS * 2.0
    assert np.array_equal(g.w, g.w[::-1]) and np.array_equal(g.mu, -g.mu[::-1])      # the hemispheres mirror exactly
    assert g.mu[0] == -1.0 and g.mu[-1] == 1.0 and (n_lat % 2 == 0 or g.mu[n_lat // 2] == 0.0)


@pytest.mark.parametrize("shape", [(19, 36), (20, 36), (33, 24)])
def test_gram_matrices_of_the_f64_tables(shape):
    from qingdai_amd import spharm
    g = spharm.tables(*shape)
    assert g.N == min((shape[0] - 1) // 2, (shape[1] - 1) // 2)
    for m in (0, g.N // 2):
        P = spharm.legendre(g, m)[m:]
        gram = 0.5 * (P * g.w).dot(P.T)
        err = float(np.abs(gram - np.eye(len(P))).max())
        print(f"spharm gram {shape[0]}x{shape[1]} m={m}: {err:.3e} (bound {64 * EPS * (g.N + 1):.3e})")
        assert err <= 64 * EPS * (g.N + 1), (shape, m, err)


def test_legendre_against_scipy():
    from scipy.special import lpmv
    from qingdai_amd import spharm
    g = spharm.tables(19, 36)
    assert g.N == 9
    for m in range(g.N + 1):
        P = spharm.legendre(g, m)
        for n in range(m, g.N + 1):
            # lpmv carries the Condon-Shortley phase (-1)^m; Pbar_n^m = sqrt((2n + 1) (n - m)! / (n + m)!) P_n^m without it
            norm = math.sqrt((2 * n + 1) * math.factorial(n - m) / math.factorial(n + m))
            want = (-1) ** m * norm * lpmv(m, n, g.mu)
            assert np.abs(P[n] - want).max() <= 1e-13, (m, n)
        assert not P[:m].any()


def test_a_single_harmonic_and_one_beyond_the_truncation():
    """Re Y_5^3 at 19 x 36 (N = 9): all power in bin 5 and sum P = ms.  A field at n = N + 1 = 10, m = 1 cannot be carried, and on
    this grid none of it aliases into the bins n <= 9 either (against n = 9 it is odd about the equator, against n <= 8 the product
    is a polynomial of degree <= 18 = n_lat - 1, which the weights integrate exactly): the run gives resid = 1.000000 with
    ms = 0.500839 (the quadrature of a degree-20 polynomial whose integral is 1/2); the test asks for resid >= 0.99."""
    from scipy.special import lpmv
    from qingdai_amd import spharm
    g = spharm.tables(19, 36)
    c = np.zeros((g.N + 1, g.N + 1), dtype=complex)
    c[3, 5] = 1.0
    x = spharm.synthesise(c, g)
    P, ms, bad = spharm.power_reference(spharm.analyse_reference(x, g), x, g)
    assert bad == 0 and abs(P[5] - 2.0) <= 1e-13 and np.delete(P, 5).max() <= 1e-26
    assert abs(P.sum() - ms) <= 1e-13 * ms
    assert abs(float(spharm.resid(P, ms))) <= 1e-13
    n, m = g.N + 1, 1
    pbar = -math.sqrt((2 * n + 1) * math.factorial(n - m) / math.factorial(n + m)) * lpmv(m, n, g.mu)
    x = pbar[:, None] * np.cos(2 * np.pi * np.arange(36) / 36)[None, :]
    P, ms, bad = spharm.power_reference(spharm.analyse_reference(x, g), x, g)
    r = float(spharm.resid(P, ms))
    print(f"spharm resid of a field at n = N + 1: {r:.6f} (ms {ms:.6f})")
    assert abs(ms - 0.5) <= 0.01 and r >= 0.99


@pytest.mark.parametrize("shape", SHAPES, ids=[f"{a}x{b}" for a, b in SHAPES])
def test_round_trip(shape):
    from qingdai_amd import spharm
    g = spharm.tables(*shape)
    c = coefficients(g)
    x = spharm.synthesise(c, g, extended=True)
    e64 = float(np.abs(spharm.analyse_reference(x, g) - c).max())
    ext = float(np.abs(spharm.analyse_reference(x, g, extended=True) - c).max())
    print(f"spharm round trip {shape[0]}x{shape[1]} (N = {g.N}): f64 {e64:.3e} extended {ext:.3e}")
    assert e64 <= 8 * RECOVERY_MEASURED and ext < e64, (shape, e64, ext)
    P, ms, bad = spharm.power_reference(c, x, g)                  # Parseval on the exact coefficients
    assert bad == 0 and abs(P.sum() - ms) <= 64 * EPS * ms


def test_a_non_finite_cell_makes_every_coefficient_nan():
    from qingdai_amd import spharm
    g = spharm.tables(9, 45)
    x = spharm.synthesise(coefficients(g), g)
    x[4, 7] = np.inf
    c = spharm.analyse_reference(x, g)
    P, ms, bad = spharm.power_reference(c, x, g)
    assert np.isnan(c.real).all() and np.isnan(c.imag).all() and np.isnan(P).all() and np.isnan(ms) and bad == 1


def test_ke_of_solid_body_rotation():
    from qingdai_amd import spharm
    g = spharm.tables(33, 24)
    omega = 7.292e-5
    zeta = 2.0 * omega * g.mu[:, None] * np.ones((1, 24))         # u = a omega cos(phi): zeta = 2 omega sin(phi)
    P = spharm.power_reference(spharm.analyse_reference(zeta, g))
    ke, rot, div = spharm.ke_spectra(P, np.zeros_like(P), A)
    assert abs(rot[1] - A * A * omega * omega / 3.0) <= 1e-13 * rot[1]
    assert np.delete(rot, 1).max() <= 1e-26 * rot[1] and not div.any() and np.array_equal(ke, rot) and ke[0] == 0.0


def test_ke_slope():
    from qingdai_amd import spharm
    n = np.arange(41, dtype=np.float64)
    ke = np.zeros(41)
    ke[1:] = 3.0 * n[1:] ** -3.0
    assert abs(spharm.ke_slope(ke)[0] + 3.0) <= 1e-12                # 8 <= n <= 20
    assert np.isnan(spharm.ke_slope(ke[:21])[0])                     # 8 <= n <= 10: three bins
    ke[9:12] = 0.0
    assert np.isfinite(spharm.ke_slope(ke)[0])


def test_environment_and_refusals():
    from qingdai_amd import spharm
    from qingdai_amd._lib import C
    d = spharm.read_env({})
    assert d == {"enabled": False, "every": 24, "two_d": True, "every_days": 10.0, "fields": None}
    d = spharm.read_env({"QD_SPHARM": "1", "QD_SPHARM_EVERY": "0", "QD_SPHARM_EVERY_DAYS": "nan", "QD_SPHARM_2D": "0", "QD_SPHARM_FIELDS": " vort, h ,precip"})
    assert d == {"enabled": True, "every": 24, "two_d": False, "every_days": 10.0, "fields": ["VORT", "H", "PRECIP"]}
    d = spharm.read_env({"QD_SPHARM": "x", "QD_SPHARM_EVERY": "x", "QD_SPHARM_EVERY_DAYS": "-1", "QD_SPHARM_FIELDS": "NOPE"})
    assert d["enabled"] is False and d["every"] == 24 and d["every_days"] == 10.0 and d["fields"] is None      # off: the list is not read
    assert spharm.resolve_fields(None, False) == ["VORT", "DIV", "H"]
    with pytest.raises(ValueError, match="QD_SPHARM_FIELDS: unknown field 'NOPE'"):
        spharm.read_env({"QD_SPHARM": "1", "QD_SPHARM_FIELDS": "H,NOPE"})
    with pytest.raises(ValueError, match="QD_SPHARM_FIELDS: field 'SST' needs the ocean"):
        spharm.resolve_fields(["H", "SST"], False)
    assert spharm.resolve_fields(["H", "SST"], True) == ["H", "SST"]
    with pytest.raises(ValueError, match="at most 32"):
        spharm.parse_fields(",".join(["H"] * 33))
    # history's entries, PRECIP among them (sampled in front of the ocean step by the device, as history's), and the lane's own two
    assert spharm.entries_for(["PRECIP", "VORT", "WIND_SPEED", "DIV"]) == [(0, "PRECIP", None), (C["QD_SPHARM_OP_VORT"], None, None),
                                                                          (1, "U", "V"), (C["QD_SPHARM_OP_DIV"], None, None)]
    assert spharm.truncation(721, 1440) == 360 and spharm.truncation(5, 8) == 2 and spharm.truncation(3, 8) == 1
    for shape in ((2, 8), (9, 2), (1, 1)):
        with pytest.raises(ValueError, match="N >= 1 is needed"):
            spharm.truncation(*shape)
    assert spharm.file_name(0.0, 9.9) == "spharm_day_00.0_09.9.nc" and spharm.file_name(0.5, 0.55, 2) == "spharm_day_00.50_00.55.nc"


def test_window_variables():
    from qingdai_amd import spharm
    N, names = 4, ["VORT", "DIV", "H"]
    r = np.random.default_rng(3)
    recs = r.random((2, spharm.record_width(3, N)))
    recs.reshape(2, 3, N + 3)[:, :, N + 2] = [[0, 1, 0], [0, 0, 2]]
    sums = r.random((3, N + 1, N + 1))
    dims, v = spharm.window_variables(names, recs, [0.0, 600.0], [0, 2], N, 300.0, 2, 1, A, sums=sums, count=2)
    per = {f"{n.lower()}_{s}" for n in names for s in ("power", "meansq", "resid", "bad_rows", "power_nm")}
    assert set(v) == per | {"time_seconds", "step", "degree", "ke_power", "ke_rot_power", "ke_div_power", "ke_slope", "truncation",
                            "dt_seconds", "sample_every", "n_samples", "complete"}
    assert dims == {"time": 2, "n": N + 1, "m": N + 1} and v["truncation"][2] == N and v["n_samples"][2] == 2
    power, ms, bad = spharm.split_records(recs, 3, N)
    assert np.array_equal(v["h_power"][2], power[:, 2]) and np.array_equal(v["h_meansq"][2], ms[:, 2])
    assert v["div_bad_rows"][2].tolist() == [1, 0] and v["h_bad_rows"][2].tolist() == [0, 2]
    assert np.allclose(v["h_resid"][2], 1.0 - power[:, 2].sum(axis=1) / ms[:, 2]) and np.array_equal(v["h_power_nm"][2], sums[2] / 2.0)
    assert np.array_equal(v["ke_power"][2], v["ke_rot_power"][2] + v["ke_div_power"][2]) and not v["ke_power"][2][:, 0].any()
    assert np.isnan(v["ke_slope"][2]).all()                       # N / 2 < 8: no bins to fit
    _, v = spharm.window_variables(["H"], recs[:, :N + 3], [0.0, 600.0], [0, 2], N, 300.0, 2, 0, A)
    assert set(v) == {"h_power", "h_meansq", "h_resid", "h_bad_rows", "time_seconds", "step", "degree", "truncation", "dt_seconds",
                      "sample_every", "n_samples", "complete"} and v["complete"][2] == 0
