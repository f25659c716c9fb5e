"""CPU: the hostile-terrain cases of the network generator (tests/hydronet_cases.py) without a GPU -- the restatements
(tests/hydronet_ref.py) against each case's golden of the reference's generator, the plain model of the kernel's chunked sweep
against the restatement, and the condition each case is there for: a case that misses it is a wrong case.

The flow order's `placed < n_land` branch has no case: D8 cannot produce a cycle through the public entry (hydronet_cases)."""
import os

import numpy as np
import pytest

import qingdai_amd as qa
import hydronet_cases as hc
import hydronet_ref as hr
from qingdai_amd.hydronet import host_tables

HERE = os.path.dirname(os.path.abspath(__file__))


def _bits(a):
    return np.ascontiguousarray(a, dtype=np.float64).view(np.uint64)


def _golden(name):
    return np.load(os.path.join(HERE, "golden", f"hydronet_{name}.npz"))


@pytest.mark.parametrize("name", list(hc.GOLDENED))
def test_restatements_reproduce_case_golden(name):
    """All five stages, bit for bit, from the builder's field (the golden stores none)."""
    z = _golden(name)
    assert str(z["elev_src"]) == f"case:{name}" and "elevation" not in z.files
    assert os.path.getsize(os.path.join(HERE, "golden", f"hydronet_{name}.npz")) < 450 * 1024
    shape, land, elev, eps, max_iters = hr.case_inputs(z)
    r = hc.restated(name)
    assert shape == r["elevation"].shape and eps == r["eps"] and max_iters == r["max_iters"]
    assert np.array_equal(_bits(elev), _bits(r["elevation"])) and np.array_equal(land, r["land"])
    assert r["sweeps"] == int(z["sweeps"])
    assert np.array_equal(_bits(r["elevation_filled"]), _bits(hr.golden_filled(z, elev)))
    for k in ("flow_to_index", "lake_mask", "lake_id", "lake_outlet_index", "flow_order"):
        assert np.array_equal(r[k], z[k]), k
    assert r["n_lakes"] == int(z["n_lakes"])
    lat, lon, cp = host_tables(qa.SphericalGrid(*shape))
    for got, want in ((lat, z["lat_rad"]), (lon, z["lon_rad"]), (cp, z["cos_pair"])):
        assert np.array_equal(_bits(got), _bits(want))


_MODEL = {}


def _model(name):
    if name not in _MODEL:
        r = hc.restated(name)
        _MODEL[name] = hc.chunk_model(r["elevation"], r["land"], r["eps"], r["max_iters"])
    return _MODEL[name]


def _never_runs(name):
    """-> [(longest run of never-merged chunks, it ends in the last chunk)] per row visit."""
    return [hc.longest_never_run(never) for _, _, never in _model(name)[2]]


@pytest.mark.parametrize("name", list(hc.CASES))
def test_chunk_model_equals_the_plain_sweeps(name):
    r = hc.restated(name)
    filled, sweeps, visits = _model(name)
    assert sweeps == r["sweeps"]
    assert np.array_equal(_bits(filled), _bits(r["elevation_filled"]))
    assert (len(visits) > 0) == (r["max_iters"] > 0)


def test_every_size_edge_has_a_case():
    shapes = {hc.restated(n)["elevation"].shape for n in hc.GOLDENED}
    assert {(5, 4), (5, 5), (6, 17), (5, 16), (7, 33), (32, 64), (64, 96)} <= shapes
    assert 32 * 64 == hc.SCAN_TILE and 64 * 96 == 3 * hc.SCAN_TILE
    assert min(s[0] for s in shapes) == 5 and min(s[1] for s in shapes) == 4                   # qd_create's minima
    assert {hc.restated(n)["max_iters"] for n in hc.GOLDENED} >= {0, 3, 5, 30, 50, 80}
    assert all(hc.restated(n)["elevation"].size <= 10000 for n in hc.GOLDENED)
    assert int(hc.restated("ring_7x50")["sweeps"]) == 80                                        # the flat ring never settles
    assert set(hc.RESTATED) == {"vplane_13x4320"} | {f"wide_13x{n}" for n in (1940, 1941, 2880, 4097, 4846)}


def test_seam_valley_reaches_the_carry_walk_at_the_last_chunk():
    rise = _never_runs("seam_valley_rise_9x272")
    assert max((n for n, at_end in rise if at_end), default=0) >= 8
    assert max(n for n, _ in _never_runs("seam_valley_fall_9x272")) <= 1
    for name in ("seam_valley_rise_9x272", "seam_valley_fall_9x272"):
        assert hc.restated(name)["sweeps"] == 30


def test_widest_case_gives_a_lane_two_chunks():
    n_lon = 4846
    nch = -(-n_lon // hc.PF_CHUNK)
    assert nch > hc.PF_THREADS and -(-4097 // hc.PF_CHUNK) > hc.PF_THREADS >= -(-4096 // hc.PF_CHUNK)
    assert max(n for n, _ in _never_runs("wide_13x4846")) >= 256
    assert max(n for n, _ in _never_runs("wide_13x2880")) >= 150


def test_lds_thresholds_sit_where_the_cases_are():
    assert hc.pitfill_lds_bytes(13, 1940) <= hc.LDS_DEFAULT < hc.pitfill_lds_bytes(13, 1941)
    assert hc.pitfill_lds_bytes(13, 4853) == 163823 and hc.pitfill_lds_bytes(13, 4854) == 163856   # either side of 160 KiB,
    # but the kernel's static LDS comes out of the same 160 KiB, so the widest row is seven columns narrower
    assert hc.LDS_LIMIT + hc.LDS_STATIC == 160 * 1024
    assert hc.pitfill_lds_bytes(13, 4846) <= hc.LDS_LIMIT < hc.pitfill_lds_bytes(13, 4847)
    assert hc.LDS_DEFAULT < hc.pitfill_lds_bytes(13, 4320) <= hc.LDS_LIMIT                     # the V-plane's row fits
    src = open(os.path.join(os.path.dirname(HERE), "qingdai_amd", "csrc", "qd_hydronet.hip")).read()
    for text in ("#define HN_PF_T 256", "#define HN_PF_C 16", "#define HN_SCAN_PER 8", "#define HN_ORDER_T 1024",
                 "lds + fa.sharedSizeBytes > 160 * 1024", "lds > 64 * 1024"):
        assert text in src, text                                                                # the constants restated above


def test_vplane_runs_long_and_wide_generations():
    r = hc.restated("vplane_13x4320")
    sizes = hc.kahn_generations(r["flow_to_index"], r["land"])
    assert sum(sizes) == int((r["land"] == 1).sum()) == r["flow_order"].size
    assert len(sizes) >= 1000 and max(sizes) > 4096 > hc.ORDER_SLICE


def test_cone_has_a_confluence_of_eight():
    r = hc.restated("cone_9x12")
    f = r["flow_to_index"].ravel()
    assert np.bincount(f[f >= 0], minlength=f.size).max() == 8


def test_serpentine_is_one_long_lake():
    r = hc.restated("serpentine_33x64")
    assert r["n_lakes"] == 1 and int(r["lake_mask"].sum()) > 900
    # the snake does not close across the seam: no lake cell on the last column
    assert not r["lake_mask"][:, -1].any() and r["lake_mask"][0, 0] == 1 and r["lake_mask"][-1, 0] == 1


def test_all_land_flat_lake_has_no_outlet():
    r = hc.restated("all_land_flat_5x12")
    assert r["n_lakes"] == 1 and r["lake_mask"].all() and (r["land"] == 1).all()
    assert r["lake_outlet_index"].tolist() == [-1]


def test_seam_pole_lake_wraps_and_touches_both_poles():
    r = hc.restated("seam_pole_lake_9x40")
    lm = r["lake_mask"]
    assert r["n_lakes"] == 1 and lm[:, 0].any() and lm[:, -1].any() and lm[0].any() and lm[-1].any()
    assert int(r["lake_outlet_index"][0]) >= 0


def test_signed_zero_lake_candidates_have_both_signs():
    r = hc.restated("signed_zero_it0_9x24")
    ef, lm, land = r["elevation_filled"], r["lake_mask"], r["land"]
    n_lat, n_lon = land.shape
    j, i = hc.SIGNED_ZERO_PITS[0]
    assert lm[j, i] == 1 and int((r["lake_id"] == r["lake_id"][j, i]).sum()) == 1               # a lake of the pit alone
    cand = [ef[jj, ii] for jj, ii in hr.neighbours(j, i, n_lat, n_lon) if lm[jj, ii] == 0 and land[jj, ii] == 1]
    assert len(cand) == 8 and all(v == 0.0 for v in cand)
    signs = [bool(np.signbit(v)) for v in cand]
    assert signs[0] is False and True in signs[1:]          # +0.0 first, a -0.0 later: the first is the outlet
    assert int(r["lake_outlet_index"][r["lake_id"][j, i] - 1]) == (j - 1) * n_lon + i - 1


def test_eps_below_half_an_ulp_changes_nothing():
    r = hc.restated("eps_tiny_37x72")
    land, elev = r["land"] == 1, r["elevation"]
    assert r["eps"] == 1e-14 and bool(np.all(elev[land] + 1e-14 == elev[land]))
    assert r["sweeps"] == 1 and np.array_equal(_bits(r["elevation_filled"]), _bits(elev))
    # and the guard is what holds them: cells level with their lowest neighbour
    n_lat, n_lon = elev.shape
    level = sum(1 for j, i in zip(*np.nonzero(land))
                if elev[j, i] == min(elev[jj, ii] for jj, ii in hr.neighbours(j, i, n_lat, n_lon)))
    assert level > 100
    big = hc.restated("eps_large_37x72")
    assert big["eps"] == 0.5 and big["sweeps"] == 5 and int((big["elevation_filled"] != big["elevation"]).sum()) > 500
