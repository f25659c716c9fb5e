"""CPU: the table of median edges (tests/median_cases.py) itself.  Every case lands on the edge it is named for -- the list is 4096
long and then 4097, a band holds 4092 candidates and then 4093, a rank's bin is 0 or 2047 and its neighbour just outside -- the model's
value is numpy's median bit for bit, and every form of the table of forms is reached by at least one case."""
from fractions import Fraction

import numpy as np
import pytest

import median_cases as mc


def check_edge(cid, k, P, edge):
    """the named expectations of one call against the model's prediction"""
    derived = dict(P)
    derived["isinf"] = bool(np.isinf(P["value"]))
    if "band_M" in P and P["band_M"]:
        derived["band_max"] = max(P["band_M"])
    for key, want in edge.items():
        if key == "wg_top":
            wg = P["wg"]
            assert wg[:len(want)] == want and all(c == 0 for c in wg[len(want):]), (cid, k, wg[:4], want)
            continue
        got = derived[key]
        if callable(want):
            assert want(got), (cid, k, key, got)
        elif key == "value":
            assert mc.same(got, want), (cid, k, got, want)
        else:
            assert got == want, (cid, k, key, got, want)


@pytest.mark.parametrize("cid", sorted(mc.CASES))
def test_case_sits_on_its_edge(cid):
    C = mc.CASES[cid]
    calls, preds = mc.predict_case(C)
    assert len(calls) >= 2 and C["why"]
    n_lat, n_lon = C["shape"]
    assert n_lat * n_lon <= 12800                                # the largest: (40, 320), the band capacity on three bands
    for k, (c, ps) in enumerate(zip(calls, preds)):
        jobs = [c] if c["op"] == "single" else list(c["jobs"])
        edges = [c["edge"]] if c["op"] == "single" else list(c["edges"])
        for j, P, e in zip(jobs, ps, edges):
            assert np.shape(j["x"]) == C["shape"]
            want = mc.expected(j["x"], j["dflt"], j["transform"], j["tparam"])
            assert mc.same(P["value"], want), (cid, k, P["value"], want)          # the model's two order statistics == np.median
            assert e, (cid, k, "a call without a named expectation")
            check_edge(cid, k, P, e)
    # the same calls with QD_MEDIAN_PREDICT=0: form 1 (bands: six passes) throughout
    _, off = mc.predict_case(C, calls=[c for c in calls if c["op"] == "single"], predict=False)
    assert all(P[0]["form"] in ("1", "4-first") and P[0]["report"] is None for P in off)


def test_fields_are_functions_of_seed_and_shape():
    for cid in ("geometry/5x2051", "capacity/stage_600_600", "bands3/total_4097", "pair/transforms"):
        a, b = mc.CASES[cid]["build"](), mc.CASES[cid]["build"]()
        for x, y in zip(a, b):
            xs = [x["x"]] if x["op"] == "single" else [j["x"] for j in x["jobs"]]
            ys = [y["x"]] if y["op"] == "single" else [j["x"] for j in y["jobs"]]
            assert all(np.array_equal(p, q, equal_nan=True) for p, q in zip(xs, ys))


def test_every_form_is_reached():
    reached = {f: [] for f in mc.FORMS}
    for cid in sorted(mc.CASES):
        _, preds = mc.predict_case(mc.CASES[cid])
        got = set().union(*(mc.forms_of(P) for ps in preds for P in ps))
        for f in got:
            reached[f].append(cid)
    print({f: len(v) for f, v in reached.items()})
    assert all(reached[f] for f in mc.FORMS), {f: v for f, v in reached.items() if not v}
    # the combinations the issue names: the pair chain with each finisher, transform 1 on a windowed and on a band call
    combos = set()
    for cid in sorted(mc.CASES):
        _, preds = mc.predict_case(mc.CASES[cid])
        combos |= {(P["chain"], P["form"], P["transform"]) for ps in preds for P in ps}
    for want in (("pair", "2a", 0), ("pair", "2b", 0), ("pair", "2c", 0), ("pair", "none", 0), ("pair", "2a", 1), ("single", "2a", 1),
                 ("single", "4a", 1), ("single", "4-first", 1), ("single", "1", 1)):
        assert want in combos, want


def test_the_named_edges_come_in_neighbouring_pairs():
    """M = 4096 and 4097; a band at 4092 and 4093; 512 and 513 in a workgroup; bins 0 / -1 and 2047 / 2048"""
    def second(cid, key):
        _, preds = mc.predict_case(mc.CASES[cid])
        return preds[1][0][key]
    assert [second(f"capacity/list_{m}_odd", "M") for m in (4095, 4096, 4097)] == [4095, 4096, 4097]
    assert [second(f"capacity/list_{m}_even", "form") for m in (4095, 4096, 4097)] == ["2a", "2a", "2b"]
    assert [second(f"capacity/stage_{n}", "wg")[0] for n in (511, 512, 513, 600)] == [511, 512, 513, 600]
    assert mc.WG_STAGE == 512 and second("capacity/stage_600_600", "wg")[:3] == [600, 600, 0]
    for w in (2, 3):
        assert max(second(f"bands{w}/band_4092", "band_M")) == mc.BAND_CAP and not second(f"bands{w}/band_4092", "miss")
        assert max(second(f"bands{w}/band_4093", "band_M")) == mc.BAND_CAP + 1 and second(f"bands{w}/band_4093", "miss")
        assert [second(f"bands{w}/total_{m}", "form") for m in (4096, 4097)] == ["4a", "4b"]
    assert [second(f"window/{c}", "k1_bin") for c in ("below1", "div16", "bin0", "bin2047", "times16")] == [-1, 0, 0, 2047, 2048]
    base, top = mc._wbase(mc.WCENTRE)
    assert mc.bits(mc.WCENTRE / 16.0) == base and mc.bits(mc.WCENTRE * 16.0) == top          # x 16 and / 16 are the window's two ends


def test_transform_restatements_agree():
    """qd_med_value's max(0, -(x - tparam)) and physics.py:296's, bit for bit on the cases' inputs; the subtraction rounds there"""
    n = 0
    for cid, C in mc.CASES.items():
        for c in C["build"]() if "transform" in cid else ():
            jobs = [c] if c["op"] == "single" else list(c["jobs"])
            for j in jobs:
                if j["transform"] != 1:
                    continue
                a, b = mc.med_value_kernel(j["x"], 1, j["tparam"]), mc.med_value_physics(j["x"], j["tparam"])
                assert np.array_equal(a.view(np.uint64), b.view(np.uint64))
                assert not (a[j["x"] == j["tparam"]] > 0).any()                       # entries equal to tparam do not count
                x = j["x"][np.isfinite(j["x"])]
                if np.ptp(x) > 0:
                    tp = Fraction(j["tparam"])                                        # x - tparam is not exact
                    assert tp == 0 or any(Fraction(float(v)) - tp != Fraction(float(v - j["tparam"])) for v in x.ravel()[:200])
                    n += 1
    assert n >= 6


def test_band_ranges_restated():
    from qingdai_amd.bands import band_ranges
    for n_lat in (40, 41, 91):
        for w in (2, 3, 4):
            assert mc.band_ranges(n_lat, w) == band_ranges(n_lat, w)
