"""CPU: the band geometries of tests/band_form_cases.py before any of them goes to a GPU.  The library's own planner runs without a
device (qd_plansim_*, as tests/test_bands_cpu.py drives it): every row's bands are accepted, a coupled step's chain of radii never
asks for more than the halo (in a BandGroup one rank that fails alone leaves the others waiting at the barrier), every row's `why`
holds on the segments the planner returns, the rows together claim every threshold the table is built around -- each row at least
one that no other row claims, so that dropping a row fails here --, and the oracle sensitivities behind the coupled bounds are
recomputed."""
import ctypes
import types

import numpy as np
import pytest

import band_form_cases as bc
import step_form_cases as sc

I = ctypes.c_int32


class Plan:
    """A planner-only handle of one band of a row; fresh handles are valid on their whole halo (qd_create)"""

    def __init__(self, cid, halo, rank):
        from qingdai_amd import _lib
        self.lib, self.F = _lib.load(), _lib.F
        self.nlat, self.nlon = bc.CASES[cid]["shape"]
        rr = bc.ranges_of(cid)
        self.row0, self.nrows = rr[rank]
        self.halo = halo
        desc = _lib.qd_grid_desc(self.nlat, self.nlon, self.row0, self.nrows, halo, 0, rank, len(rr))
        self.h = ctypes.c_void_p()
        assert self.lib.qd_plansim_create(ctypes.byref(desc), ctypes.byref(self.h)) == 0, (cid, halo, rank)
        every = list(range(_lib.C["QD_F_COUNT_F64"]))
        assert self.lib.qd_plansim_mark(self.h, (I * len(every))(*every), len(every), halo) == 0

    def close(self):
        assert self.lib.qd_plansim_destroy(self.h) == 0

    def margin(self, field):
        return self.lib.qd_plansim_margin(self.h, self.F[field])

    def plan(self, ins):
        f, r = [self.F[k] for k, _ in ins], [x for _, x in ins]
        m = self.lib.qd_plansim_plan(self.h, (I * len(f))(*f), (I * len(f))(*r), len(f), -1)
        fl, geo, n_ex = (I * 16)(), (I * 4)(), 0
        while self.lib.qd_plansim_pop_exchange(self.h, fl, 16, geo) > 0:
            n_ex += 1
        return m, n_ex

    def mark(self, outs, m):
        assert self.lib.qd_plansim_mark(self.h, (I * len(outs))(*[self.F[k] for k in outs]), len(outs), m) == 0

    def segments(self, m):
        seg = (I * 6)()
        ns = self.lib.qd_plansim_segments(self.h, m, seg)
        assert 1 <= ns <= 3
        return [(seg[2 * k], seg[2 * k + 1]) for k in range(ns)]

    def segments_rows(self, vr0, cnt):
        seg = (I * 12)()
        ns = self.lib.qd_plansim_segments_rows(self.h, vr0, cnt, seg)
        assert 0 <= ns <= 6
        return [(seg[2 * k], seg[2 * k + 1]) for k in range(ns)]

    def stream_ok(self, segs, ocean):
        """qd_stream_ok / qd_ocn_stream_ok(_list) on explicit segments"""
        if self.nlon < 64 or self.nlat < 12 or not segs:
            return False
        for r0, n in segs:
            if not bc.seg_ok(r0, n, self.nlat):
                return False
            if ocean and (r0 == 0 or r0 + n == self.nlat) and not (bc.on_slab(0, self.row0, self.nrows, self.halo, self.nlat) and
                                                                  bc.on_slab(self.nlat - 1, self.row0, self.nrows, self.halo, self.nlat)):
                return False
        return True

    def polar(self):
        return self.row0 == 0 or self.row0 + self.nrows == self.nlat


def run_chain(cid, halo, rank, nsteps=2):
    """bc.plan_chain for `nsteps` steps -> [(tag, margin, exchanges, what the narrow ocean plan could do before the exchange)]"""
    c = bc.CASES[cid]
    P = Plan(cid, halo, rank)
    out = []
    narrow = [("ETA", 5), ("UO", 4), ("VO", 4), ("ISR_A", 4), ("ISR_B", 4)]
    for _ in range(nsteps):
        for tag, ins, outs in bc.plan_chain(c["shape"], halo, with_atm="atm" in c["runs"]):
            assert all(r <= halo for _, r in ins), (cid, halo, tag, ins)
            m_old = min(P.margin(f) - r for f, r in narrow)
            m, n_ex = P.plan(ins)
            assert m >= 0, (cid, halo, rank, tag, m)                       # -1: a radius wider than the halo
            assert n_ex <= 1
            if outs:
                P.mark(outs, m)
            out.append((tag, m, n_ex, m_old))
    return P, out


def all_bands(cid):
    for halo in bc.halos_of(cid):
        for rank in range(len(bc.ranges_of(cid))):
            P, chain = run_chain(cid, halo, rank)
            yield halo, rank, P, chain
            P.close()


def margins(chain, tag):
    return sorted({m for t, m, _, _ in chain if t == tag})


# ---------------------------------------------------------------- no refusal
@pytest.mark.parametrize("cid", bc.IDS)
def test_every_band_is_accepted_and_the_chain_stays_inside_the_halo(cid):
    from qingdai_amd.bands import required_halo
    c = bc.CASES[cid]
    nlat, nlon = c["shape"]
    assert nlat <= 97 and nlon <= 130 and set(c["runs"]) <= {"atm", "ocean", "coupled"} and set(c["claims"]) <= set(bc.CLAIMS)
    rr = bc.ranges_of(cid)
    assert rr[0][0] == 0 and sum(n for _, n in rr) == nlat and all(rr[k][0] + rr[k][1] == rr[k + 1][0] for k in range(len(rr) - 1))
    for halo in bc.halos_of(cid):
        assert halo >= 5                                                   # qd_create
        if "atm" in c["runs"]:
            assert halo >= required_halo(nlat, bc.DT) == 12
        for r0, n in rr:
            assert n >= halo and n + 2 * halo <= nlat, (cid, halo, r0, n)  # qd_exchange, qd_create
    n = 0
    for halo, rank, P, chain in all_bands(cid):                             # run_chain asserts on every plan
        n += 1
        for tag, m, _, _ in chain:
            rows = sorted(r for r0, k in P.segments(m) for r in range(r0, r0 + k))
            assert rows == sorted((P.row0 - m + k) % nlat for k in range(P.nrows + 2 * m)), (cid, halo, rank, tag, m)
    assert n == len(rr) * len(bc.halos_of(cid))


def test_no_segment_starts_within_four_rows_of_a_pole():
    """own_nrows >= halo and a momentum margin <= halo - 5: the first / last row of a launch segment is a pole or >= 5 rows from it,
    for every row, band and margin the chain gives (and for every margin up to halo - 5)"""
    for cid in bc.IDS:
        for halo, rank, P, chain in all_bands(cid):
            ms = set(margins(chain, "dyn") + margins(chain, "ocn")) | set(range(0, max(0, halo - 5) + 1))
            assert max(margins(chain, "dyn") + margins(chain, "ocn")) <= halo - 5
            for m in ms:
                for r0, n in P.segments(m):
                    assert not (0 < r0 < 5) and not (P.nlat - 5 < r0 + n < P.nlat), (cid, halo, rank, m, r0, n)


# ---------------------------------------------------------------- the geometric claim of every row
def _claim_holds(claim, cid):
    bands = []
    try:
        for halo in bc.halos_of(cid):
            for rank in range(len(bc.ranges_of(cid))):
                P, chain = run_chain(cid, halo, rank)
                bands.append((halo, rank, P, chain))
        return _claim_on(claim, cid, bands)
    finally:
        for _, _, P, _ in bands:
            P.close()


def _claim_on(claim, cid, bands):
    """bands: (halo, rank, open planner handle, chain).  Segments come from the library: qd_plansim_segments for a launch at a margin,
    qd_plansim_segments_rows for the interior rows and the boundary strips of a split launch."""
    c = bc.CASES[cid]
    nlat, nlon = c["shape"]
    rr = bc.ranges_of(cid)
    halos = bc.halos_of(cid)
    w58, w60, _ = sc.last_widths(nlon)
    TR = 6                                                                  # qd_pick_tile at these sizes; the GPU evidence asserts tile_tr == 6

    def segs(P, m):
        return P.segments(m)

    def own(P, m):
        return [s for s in segs(P, m) if s[0] <= P.row0 < s[0] + s[1]][0]

    def wrap(P, m):
        return [s for s in segs(P, m) if s != own(P, m)]

    def tiles(P, seg):
        return [bc.fast_tile(TR, seg, i0, nlat, nlon, P.row0 - P.halo, P.nrows + 2 * P.halo) for i0 in range(seg[0], seg[0] + seg[1], TR)]

    def poles_on_slab(P):
        return bc.on_slab(0, P.row0, P.nrows, P.halo, nlat) and bc.on_slab(nlat - 1, P.row0, P.nrows, P.halo, nlat)

    if claim == "fast_tile_plane_shifted":
        per_band, low, high = [], False, False                              # every polar band has one; both clamps occur in the row
        for _, _, P, ch in bands:
            if not P.polar():
                continue
            for m in margins(ch, "ocn"):
                s = own(P, m)
                lo, hi = (0 if s[0] == 0 else s[0] - 5), (nlat if sum(s) == nlat else sum(s) + 5)
                t = [x for x in tiles(P, s) if x["fits"] and x["shifted"]]
                low |= any(x["p0"] == lo for x in t)
                high |= any(x["p0"] == hi - (TR + 10) for x in t)
                per_band.append(bool(t) and not P.stream_ok(segs(P, m), True))
        return bool(per_band) and all(per_band) and low and high
    if claim == "fast_tile_slab_edge":
        return any(m == halo - 5 and any(x["fits"] and x["slab_edge"] for x in tiles(P, own(P, m))) and not P.stream_ok(segs(P, m), True)
                   for halo, _, P, ch in bands for m in margins(ch, "ocn"))
    if claim == "wrap_tile_exact":
        got = [x["fits"] for _, _, P, ch in bands if P.polar() for m in margins(ch, "dyn") + margins(ch, "ocn") for w in wrap(P, m) for x in tiles(P, w)]
        return bool(got) and not any(got)
    if claim == "pole_tile_without_other_pole":
        return any(not P.polar() and not poles_on_slab(P) and any(x["fits"] and not x["interior"] for x in tiles(P, own(P, m))) and
                   any(x["fits"] and x["interior"] for x in tiles(P, own(P, m))) for _, _, P, ch in bands for m in margins(ch, "ocn"))
    if claim == "slab_is_whole_ring":
        return any(n + 2 * halos[0] == nlat for _, n in rr)
    if claim == "wrap_segment_short":
        return all(0 < len(wrap(P, m)) and all(n < 10 for _, n in wrap(P, m)) and not P.stream_ok(segs(P, m), True)
                   for _, _, P, ch in bands if P.polar() for m in margins(ch, "dyn") + margins(ch, "ocn"))
    if claim == "nlon_below_64":
        return nlon < 64 and all(not P.stream_ok(segs(P, 0), False) for _, _, P, _ in bands)
    if claim == "own_equals_halo":
        return any(n == halos[0] for _, n in rr) and any(n > halos[0] for _, n in rr)
    if claim == "own_equals_halo_everywhere":
        return all(n == halos[0] for _, n in rr)
    if claim == "one_column_tail_group":
        return w60 == 1
    if claim == "one_column_momentum_strip":
        return w58 == 1
    if claim == "interior_band_streams":
        return any(not P.polar() and all(len(segs(P, m)) == 1 and segs(P, m)[0][0] >= 5 and sum(segs(P, m)[0]) <= nlat - 5 and
                                         P.stream_ok(segs(P, m), True) for m in range(0, halo + 1)) for halo, _, P, _ in bands)
    if claim == "tail_on_one_segment":
        return any(all(len(segs(P, m)) == 1 for m in margins(ch, "tail")) and margins(ch, "tail") for _, _, P, ch in bands)
    if claim == "segment_at_row_5":
        hit = [(s[0] == 5, s[0] + s[1] == nlat - 5) for _, _, P, ch in bands if not P.polar() for m in margins(ch, "ocn") for s in segs(P, m)
               if P.stream_ok(segs(P, m), True)]
        return any(a for a, _ in hit) and any(b for _, b in hit)
    if claim == "world_of_5_uneven":
        return len(rr) == 5 and len({n for _, n in rr}) == 2
    if claim in ("deep_halo_pair", "boundary_strips_thin"):
        found = []
        for _, _, P, ch in bands:
            for k, (tag, _, n_ex, m_old) in enumerate(ch):
                if tag != "wide" or not n_ex:
                    continue
                m = ch[k + 1][1]                                            # the momentum launch behind the exchange
                m_int = m_old if m_old >= 0 else -12
                inner = P.segments_rows(P.row0 - m_int, P.nrows + 2 * m_int) if P.nrows + 2 * m_int > 0 else []
                split = P.nrows + 2 * m_int >= 12 and P.stream_ok(inner, True) and P.nrows >= P.halo
                if not split or m <= m_int:
                    continue
                strips = P.segments_rows(P.row0 - m, m - m_int) + P.segments_rows(P.row0 + P.nrows + m_int, m - m_int)
                found.append((len(strips), m - m_int, P.stream_ok(strips, True)))
        if claim == "deep_halo_pair":
            return any(n == 2 and rows >= 10 and ok for n, rows, ok in found)
        return bool(found) and all(rows < 10 and not ok for _, rows, ok in found)
    if claim in ("form_flips_within_a_step", "wrap_segment_streams"):
        per_band = [[P.stream_ok(segs(P, m), True) for m in margins(ch, "ocn") if wrap(P, m)] for _, _, P, ch in bands if P.polar()]
        if claim == "wrap_segment_streams":
            return any(any(b) for b in per_band)
        return any(any(b) and not all(b) for b in per_band)
    if claim == "band_tail_halo_threshold":
        need = max(7, bc.ocn_reach(c["shape"]) + 2)
        return need - 1 in halos and need in halos and min(halos) == 5 and max(halos) > need
    raise KeyError(claim)


@pytest.mark.parametrize("cid", bc.IDS)
def test_the_geometry_of_a_row_is_what_its_why_says(cid):
    for claim in bc.CASES[cid]["claims"]:
        assert _claim_holds(claim, cid), (cid, claim, bc.CLAIMS[claim])


def test_claims_are_not_vacuous():
    """Each predicate can fail: a claim a row does not make is false for a row built the other way"""
    assert not _claim_holds("wrap_segment_short", "deep3_97x70") and not _claim_holds("deep_halo_pair", "polar2_48x65")
    assert not _claim_holds("interior_band_streams", "polar2_48x65") and not _claim_holds("segment_at_row_5", "interior3_61x117")
    assert not _claim_holds("boundary_strips_thin", "deep3_97x70") and not _claim_holds("form_flips_within_a_step", "polar2_48x65")
    assert not _claim_holds("nlon_below_64", "five_61x64") and not _claim_holds("tail_on_one_segment", "polar2_48x65")
    assert not _claim_holds("fast_tile_plane_shifted", "narrow2_48x63") and not _claim_holds("fast_tile_slab_edge", "deep3_97x70")
    assert not _claim_holds("pole_tile_without_other_pole", "polar2_48x65") and not _claim_holds("pole_tile_without_other_pole", "interior3_61x117")


# ---------------------------------------------------------------- coverage
def test_the_table_claims_every_threshold_and_no_row_is_spare():
    claimed = {}
    for cid in bc.IDS:
        for k in bc.CASES[cid]["claims"]:
            claimed.setdefault(k, []).append(cid)
    assert set(claimed) == set(bc.CLAIMS), set(bc.CLAIMS) ^ set(claimed)
    for cid in bc.IDS:                                                      # dropping the row would leave a threshold unclaimed
        assert any(claimed[k] == [cid] for k in bc.CASES[cid]["claims"]), cid
    # the transports and switches of the issue are crossed somewhere
    crossed = {s for cid in bc.IDS for s in bc.CASES[cid]["switches"]}
    assert crossed == {"QD_STREAM_NO_PAIR=1", "QD_PEER_ONE_LAUNCH=0", "QD_PEER_FOLD=0", "QD_BAND_TAIL=0", "QD_NO_HOST_RING=1", "QD_FUSED_FAST=0",
                       "QD_FUSED_FAST=3"}
    # QD_FUSED_FAST=0 is crossed on a row whose tile launches have FAST tiles (else the cross compares EXACT with EXACT)
    assert any("QD_FUSED_FAST=0" in bc.CASES[cid]["switches"] and "fast_tile_plane_shifted" in bc.CASES[cid]["claims"] for cid in bc.IDS)
    assert set(bc.TRANSPORTS) == {"host", "peer0", "peer1", "peer2"}
    for cid in bc.IDS:
        assert bc.CASES[cid].get("evidence"), cid
        assert ("coupled" in bc.CASES[cid]["runs"]) != bool(bc.CASES[cid].get("no_coupled")), cid      # a coupled run, or the reason for none


def test_band_group_refuses_ranges_that_do_not_tile_the_globe():
    """BandGroup(ranges=) checks its argument before it creates a handle"""
    from qingdai_amd.bands import BandGroup
    grid = types.SimpleNamespace(n_lat=50)
    for bad in ([(0, 12), (12, 26), (38, 11)], [(0, 12), (13, 25), (38, 12)], [(0, 50)], [(0, 12), (12, 0), (12, 38)], [(1, 11), (12, 26), (38, 12)]):
        with pytest.raises(ValueError):
            BandGroup(grid, 3, ranges=bad)


# ---------------------------------------------------------------- the oracle's own sensitivity
def test_band_sensitivities_have_not_drifted():
    assert set(bc.BAND_SENS) == set(bc.COUPLED_IDS)
    for cid in bc.COUPLED_IDS:
        ocn, atm = bc.band_sensitivity(cid)
        print(cid, "ocean", ocn, "atmosphere", atm)
        assert bc.BAND_SENS[cid] / 10.0 <= ocn <= bc.BAND_SENS[cid] * 10.0, (cid, ocn, bc.BAND_SENS[cid])
        assert atm < 1e-11                                                  # 100 x below STEP_TOL, as tests/test_step_form_cases_cpu.py asks
        assert bc.band_bound(cid) == max(1e-12, 1000.0 * bc.BAND_SENS[cid]) and bc.oracle_bound(cid) == bc.STEP_TOL
