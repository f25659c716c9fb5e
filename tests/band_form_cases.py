"""The latitude-band geometries at which the band step path makes a form decision of its own, what each row is there for, and the
tallies (Device.step_forms: cnt_* / max_* of enum qd_step_form) each one must leave on the named band.  Shared by
tests/test_gpu_band_forms.py (bands against the whole globe, against the oracle, form against form) and
tests/test_band_form_cases_cpu.py (the planner accepts every row, the geometric claim of every row, coverage of the table, oracle
sensitivities).  Test infrastructure only.

The band-only decisions the table is built around (qingdai_amd/csrc):
  qs_segments_ok / qs_seg_ok      a launch at margin m streams only if every row segment has >= 10 rows and starts / ends at a pole or
                                  >= 5 rows from it; else qd_launch_dyn_hyper / qd_launch_ocn_hyper take the tile kernels for THAT launch
  qd_segments                     a polar band at margin m > 0 has a wrap segment of m rows beyond the pole
  qd_ocn_stream_ok / QD_OCN_WRAP_OK   a pole segment / pole tile needs the other pole's eta row on the slab
  qd_fast_tile                    a tile takes the FAST path if its plane of TR + 10 rows, shifted to stay on the segment +- 5 rows, fits
                                  there and on the slab (qd_lrow(p0) + RA <= lrows); the tallies cnt_*_tile_fast / cnt_tile_exact /
                                  cnt_tile_shift / cnt_tile_slab_edge ask the kernels' own test on the host beside every tile launch
  band_tail                       n_lon >= 64 and halo >= max(7, Ro + 2); else the round-2 sub-step
  the split sub-step              peer exchange with QD_PEER_OVERLAP >= 1: interior rows between push and unpack if they are >= 12 rows and
                                  pass qd_ocn_stream_ok_list; boundary strips as k_ocn_stream_pair, or the whole launch redone when thin
  the band tail                   one qd_launch_ocn_tail per segment; the fix list only on one segment

What the planner makes of a step (plan_chain below, run through qd_plansim_* by the CPU test): with the required halo of 12 rows the
atmosphere's momentum launch runs at margin 5 to 7 and the ocean's at margin 7 after an exchange in EVERY sub-step, so a polar band's
wrap segment has 5 to 7 rows (< 10: tiles on every launch) and a split's boundary strips have 7 rows (< 10: redone).  Only a deeper halo
(24 rows: margins 19, 12, 5 over three sub-steps, one exchange) streams a wrap segment, flips form inside a step and has boundary
strips of >= 10 rows.

A band is never thinner than its halo (qd_exchange refuses it) and a momentum launch never runs beyond margin halo - 5, so a launch
segment of a valid band group starts at a pole or >= 5 rows from it: the `1..4 rows from a pole` clause of qs_seg_ok cannot be reached
through qd_launch_*_hyper (test_no_segment_starts_within_four_rows_of_a_pole holds that for every row); bands of 12 rows next to a
polar band of 12 reach its accepting edge, a segment that starts at row 5 / ends at n_lat - 5.
"""
import numpy as np

import step_form_cases as sc

STEP_TOL = sc.STEP_TOL
NSTEPS, DT = sc.NSTEPS, sc.DT                # 3 steps of 300 s
BAND_TOL = 1e-12                             # tests/test_gpu_bands.py: only the band-wise order of the global sums differs

# transport -> environment (read in qd_comm_init_local / qd_peer_init_group)
TRANSPORTS = {
    "host": {},                                                                  # host copies, eta sums through the in-process host ring
    "peer0": {"QD_PEER_EXCHANGE": "1", "QD_PEER_OVERLAP": "0"},                  # device mailboxes, exchange then compute
    "peer1": {"QD_PEER_EXCHANGE": "1", "QD_PEER_OVERLAP": "1"},                  # interior rows between push and unpack
    "peer2": {"QD_PEER_EXCHANGE": "1", "QD_PEER_OVERLAP": "2"},                  # the push carried by the interior launch
}
SWITCH_NAMES = ("QD_PEER_EXCHANGE", "QD_PEER_OVERLAP", "QD_STREAM_NO_PAIR", "QD_PEER_ONE_LAUNCH", "QD_PEER_FOLD", "QD_BAND_TAIL",
                "QD_NO_HOST_RING", "QD_HOST_RING", "QD_FUSED_FAST", "QD_FUSED", "QD_OCN_TAIL", "QD_TAIL_V", "QD_OCN_FUSED", "QD_BAND_HALO",
                "QD_TAIL_FIX", "QD_TAIL_GENERAL", "QD_MEAN_IN_MOMENTUM", "QD_PEER_HOOKS")

# what each threshold named in the module text asks of a row's geometry; tests/test_band_form_cases_cpu.py evaluates every claim of
# every row on the segments qd_plansim_segments / qd_plansim_segments_rows return, and asks that every key here is claimed
CLAIMS = {
    "slab_is_whole_ring": "a band with n_rows + 2 halo == n_lat: the slab holds every row of the globe once",
    "wrap_segment_short": "a polar band's wrap segment has < 10 rows at every momentum margin: tiles on every launch",
    "nlon_below_64": "n_lon < 64 on bands: tile kernels, the round-2 sub-step, Shapiro one launch per pass",
    "own_equals_halo": "a band with n_rows == halo",
    "own_equals_halo_everywhere": "every band has n_rows == halo",
    "one_column_tail_group": "n_lon = 60 k + 1: a one-column last group of k_ocn_tail_fast on every segment",
    "one_column_momentum_strip": "n_lon = 58 k + 1: a one-column last strip of the momentum kernels on every segment",
    "interior_band_streams": "a band that is one segment, >= 5 rows from both poles, at every momentum margin: streams on every launch",
    "segment_at_row_5": "a segment that starts at row 5 or ends at n_lat - 5 at the ocean's momentum margin: the accepting edge of qs_seg_ok",
    "world_of_5_uneven": "five bands, uneven split",
    "deep_halo_pair": "at the sub-step that exchanges, the interior rows own -+ 12 are >= 12 and the boundary strips >= 10 rows: k_ocn_stream_pair",
    "boundary_strips_thin": "boundary strips of < 10 rows: the split launch is redone as a whole",
    "form_flips_within_a_step": "a polar band whose wrap segment has >= 10 rows at one ocean momentum margin and < 10 at another",
    "wrap_segment_streams": "a polar band's wrap segment of >= 10 rows with the other pole's eta row on the slab",
    "band_tail_halo_threshold": "halos on both sides of max(7, Ro + 2)",
    "fast_tile_plane_shifted": "qd_fast_tile on a polar band's own segment at the ocean's momentum margin: FAST tiles whose plane is clamped at "
                               "the pole (p0 = 0, not o0 - 5) and at the segment's other end (p0 = s1 + 5 - RA)",
    "fast_tile_slab_edge": "a FAST tile whose plane ends on the slab's last row, qd_lrow(p0) + RA == lrows: the margin is halo - 5",
    "wrap_tile_exact": "the tiles of a wrap segment of < 10 rows never fit the FAST plane (m + 5 < RA): EXACT",
    "pole_tile_without_other_pole": "QD_OCN_WRAP_OK refuses: a FAST-fitting tile of a non-polar band whose plane starts within 2 rows of a pole "
                                    "while the other pole's eta row is off the slab (k_ocn_hyper EXACT, k_dyn_hyper FAST)",
    "tail_on_one_segment": "a band whose tail runs on one segment: the only place the band tail takes the fix list",
}


def EQ(v):
    return ("==", v)


def GT(v):
    return (">", v)


# with the required halo the atmosphere's momentum launch runs at margin 5: a polar band's wrap segment has 5 rows (tiles on each of
# the 3 steps), a band away from the poles is one segment (streams)
POLAR_DYN = dict(cnt_dyn_tile=EQ(3), cnt_dyn_stream=EQ(0), max_mom_segs=EQ(2))
INNER_DYN = dict(cnt_dyn_stream=EQ(3), cnt_dyn_tile=EQ(0), max_mom_segs=EQ(1))

# id -> grid, world or hand-made ranges, halo(s), the runs (atm / ocean / coupled), the switches to cross, claims (keys of CLAIMS),
# evidence: {(run, transport[, halo or None[, switches]]): {band: {tally: (op, value)}}} -- the tallies of that band's handle after the run ("collective":
# host copies without the host ring; 9 = 3 steps of 3 sub-steps), and what the row is for.
# Beside each row: the worst measured error / bound on an MI355X, from test_gpu_band_forms' print-out (nothing is tightened to it).
CASES = {
    "polar2_48x65": dict(
        shape=(48, 65), world=2, halo=12, runs=("atm", "ocean", "coupled"),
        switches=("QD_FUSED_FAST=0", "QD_PEER_FOLD=0", "QD_BAND_TAIL=0", "QD_NO_HOST_RING=1"),
        claims=("slab_is_whole_ring", "wrap_segment_short", "boundary_strips_thin", "fast_tile_plane_shifted", "fast_tile_slab_edge", "wrap_tile_exact"),
        # measured (error / bound): atmosphere vs oracle 2.1e-6; ocean vs globe 8.9e-5, vs oracle 3.3e-5; coupled vs globe 3.6e-4, vs oracle 1.5e-6
        evidence={("atm", "host"): {0: POLAR_DYN, 1: POLAR_DYN},
                  ("ocean", "host"): {0: dict(cnt_sub_round2=EQ(9), cnt_sub_band_tail=EQ(0)), 1: dict(cnt_sub_round2=EQ(9))},
                  ("ocean", "collective"): {0: dict(cnt_sub_band_tail=EQ(9), cnt_sub_round2=EQ(0), cnt_split=EQ(0), max_tail_segs=EQ(2))},
                  ("ocean", "peer0"): {0: dict(cnt_split=EQ(0), cnt_ocn_tile=EQ(9), cnt_ocn_stream=EQ(0), max_tail_segs=EQ(2), cnt_tail_fix=EQ(0),
                                               tile_tr=EQ(6), cnt_ocn_tile_fast=GT(0), cnt_dyn_tile_fast=EQ(0), cnt_tile_exact=GT(0), cnt_tile_shift=GT(0),
                                               cnt_tile_slab_edge=GT(0)),
                                       1: dict(tile_tr=EQ(6), cnt_ocn_tile_fast=GT(0), cnt_tile_exact=GT(0), cnt_tile_shift=GT(0))},
                  ("ocean", "peer2", None, ("QD_FUSED_FAST=0",)): {b: dict(cnt_ocn_tile=EQ(9), cnt_ocn_tile_fast=EQ(0), cnt_tile_exact=GT(0), cnt_tile_shift=EQ(0))
                                                                   for b in (0, 1)},
                  ("atm", "peer0"): {0: dict(cnt_dyn_tile_fast=GT(0), cnt_tile_shift=GT(0), cnt_tile_exact=GT(0))},
                  ("ocean", "peer1"): {b: dict(cnt_split=GT(0), cnt_split_redo=GT(0), cnt_stream_pair=EQ(0), cnt_stream_push=EQ(0), cnt_ocn_tile=EQ(9),
                                               cnt_ocn_stream=EQ(0), max_mom_segs=EQ(2)) for b in (0, 1)},
                  ("ocean", "peer2"): {b: dict(cnt_split_redo=GT(0), cnt_stream_push=GT(0)) for b in (0, 1)},
                  ("coupled", "peer2"): {0: dict(cnt_dyn_tile=EQ(3), cnt_split_redo=GT(0), max_tail_segs=EQ(2))}},
        why="both bands polar, 24 + 24 rows, n_rows + 2 halo == n_lat; wrap segments of 5 to 7 rows on every launch (tiles, pole tiles "
            "reading the other pole's eta row from the slab); tail on two segments; last column strip 58 + 7"),
    "narrow2_48x63": dict(
        shape=(48, 63), world=2, halo=12, runs=("atm", "ocean"), switches=(),
        claims=("nlon_below_64",),
        no_coupled="the coupled span adds nothing to the row's branches: below 64 columns every launch is a tile launch and every sub-step the round-2 "
                   "one, which the atmosphere span and the ocean step already run; polar2_48x65 is the coupled run of this band layout",
        # measured: atmosphere vs oracle 4.2e-6; ocean vs globe 1.8e-4, vs oracle 1.7e-3
        evidence={("atm", "peer2"): {0: POLAR_DYN, 1: POLAR_DYN},
                  ("ocean", "peer2"): {b: dict(cnt_sub_round2=EQ(9), cnt_sub_band_tail=EQ(0), cnt_ocn_tile=EQ(9), cnt_ocn_stream=EQ(0), cnt_split=EQ(0))
                                       for b in (0, 1)},
                  ("ocean", "collective"): {0: dict(cnt_sub_round2=EQ(9), cnt_sub_band_tail=EQ(0))}},
        why="n_lon < 64 on bands: tile kernels only (EXACT), the round-2 band sub-step, Shapiro one launch per pass"),
    "thin3_37x121": dict(
        shape=(37, 121), world=3, halo=12, runs=("atm", "ocean"), switches=("QD_PEER_ONE_LAUNCH=0",),
        claims=("own_equals_halo", "one_column_tail_group"),
        no_coupled="the oracle itself answers the 1e-15 perturbation with 2.6e-10 there: 1000 x that bounds nothing",
        # measured: atmosphere vs oracle 4.6e-6; ocean vs globe 3.6e-4, vs oracle 3.8e-7
        evidence={("atm", "host"): {0: POLAR_DYN, 1: INNER_DYN, 2: POLAR_DYN},
                  ("ocean", "peer1"): {1: dict(cnt_split=GT(0), cnt_split_redo=GT(0), cnt_ocn_stream=EQ(9), cnt_ocn_tile=EQ(0), max_tail_segs=EQ(1),
                                               cnt_tail_fix=GT(0)),
                                       2: dict(cnt_split=GT(0), cnt_split_redo=GT(0), cnt_ocn_tile=EQ(9), max_tail_segs=EQ(2), cnt_tail_fix=EQ(0))},
                  ("ocean", "peer0"): {1: dict(cnt_split=EQ(0), cnt_ocn_stream=EQ(9))}},
        why="13 + 12 + 12 rows: own_nrows == halo on two bands (the split's own_nrows >= halo test at equality); 2 x 60 + 1 columns: "
            "a one-column last tail group on every segment; the middle band rows 13..24 streams (segment 6..31 at margin 7)"),
    "interior3_61x117": dict(
        shape=(61, 117), world=3, halo=12, runs=("atm", "ocean"), switches=("QD_FUSED_FAST=0",),
        claims=("interior_band_streams", "one_column_momentum_strip", "tail_on_one_segment"),
        no_coupled="five_61x64 is the coupled run of a layout with polar and interior bands at the same grid height; this row adds the column count",
        # measured: atmosphere vs oracle 4.7e-6; ocean vs globe 1.5e-4, vs oracle 1.6e-4
        evidence={("atm", "peer0"): {0: POLAR_DYN, 1: INNER_DYN, 2: POLAR_DYN},
                  ("ocean", "peer0"): {1: dict(cnt_ocn_stream=EQ(9), cnt_ocn_tile=EQ(0), max_mom_segs=EQ(1), max_tail_segs=EQ(1), cnt_tail_fix=GT(0))},
                  ("ocean", "collective"): {1: dict(cnt_ocn_stream=EQ(9), max_tail_segs=EQ(1), cnt_tail_fix=EQ(0))}},   # no fix statistics outside the mailboxes
        why="21 + 20 + 20 rows: the middle band is never near a pole (one segment: the band tail's fix list); 2 x 58 + 1 columns: a "
            "one-column last momentum strip"),
    "even4_48x125": dict(
        shape=(48, 125), world=4, halo=12, runs=("atm", "ocean"), switches=("QD_PEER_FOLD=0", "QD_FUSED_FAST=3"),
        claims=("own_equals_halo_everywhere", "segment_at_row_5", "pole_tile_without_other_pole"),
        no_coupled="the oracle itself answers the 1e-15 perturbation with 1.1e-5 there (a branch of the coupled physics flips): 1000 x that bounds nothing",
        # measured: atmosphere vs oracle 3.2e-6; ocean vs globe 1.8e-4, vs oracle 9.9e-6
        evidence={("atm", "host"): {0: POLAR_DYN, 1: INNER_DYN, 2: INNER_DYN, 3: POLAR_DYN},
                  ("ocean", "peer2"): {0: dict(cnt_ocn_tile=EQ(9), cnt_split=GT(0)), 3: dict(cnt_ocn_tile=EQ(9), cnt_split=GT(0)),
                                       1: dict(cnt_ocn_stream=EQ(9), cnt_ocn_tile=EQ(0), cnt_split=GT(0), cnt_split_redo=GT(0), cnt_stream_push=GT(0)),
                                       2: dict(cnt_ocn_stream=EQ(9), cnt_ocn_tile=EQ(0), cnt_split=GT(0), cnt_split_redo=GT(0), cnt_stream_push=GT(0))},
                  # the tile kernels with their FAST path on bands that would stream: the middle bands' first / last tile starts at a pole row
                  # (band 1's last tile ends on its slab's last row; band 2's slab ends at the pole, where its last tile is the EXACT one)
                  ("ocean", "peer2", None, ("QD_FUSED_FAST=3",)): {1: dict(tile_tr=EQ(6), cnt_ocn_stream=EQ(0), cnt_ocn_tile=EQ(9), cnt_ocn_tile_fast=GT(0),
                                                                           cnt_tile_exact=GT(0), cnt_tile_slab_edge=GT(0), cnt_split=EQ(0)),
                                                                   2: dict(tile_tr=EQ(6), cnt_ocn_stream=EQ(0), cnt_ocn_tile=EQ(9), cnt_ocn_tile_fast=GT(0),
                                                                           cnt_tile_exact=GT(0), cnt_tile_slab_edge=EQ(0), cnt_split=EQ(0))}},
        why="12 rows each: every band at own_nrows == halo; the two middle bands' segments start at row 5 / end at n_lat - 5 at margin 7; "
            "2 x 62 + 1 columns"),
    "five_61x64": dict(
        shape=(61, 64), world=5, halo=12, runs=("atm", "ocean", "coupled"), switches=("QD_BAND_TAIL=0", "QD_NO_HOST_RING=1"),
        claims=("world_of_5_uneven",),
        # measured: atmosphere vs oracle 5.7e-6; ocean vs globe 1.6e-4, vs oracle 1.3e-4; coupled vs globe 4.9e-4, vs oracle 3.4e-6
        evidence={("atm", "peer1"): {0: POLAR_DYN, 1: INNER_DYN, 2: INNER_DYN, 3: INNER_DYN, 4: POLAR_DYN},
                  ("coupled", "peer2"): {**{b: dict(cnt_ocn_stream=GT(0), cnt_ocn_tile=EQ(0), cnt_split_redo=GT(0), max_tail_segs=EQ(1), cnt_tail_fix=GT(0))
                                            for b in (1, 2, 3)},
                                         **{b: dict(cnt_ocn_tile=GT(0), cnt_ocn_stream=EQ(0), max_tail_segs=EQ(2), cnt_tail_fix=EQ(0)) for b in (0, 4)}},
                  ("coupled", "host"): {2: dict(cnt_sub_round2=GT(0), cnt_sub_band_tail=EQ(0))}},
        why="13 + 12 + 12 + 12 + 12 rows: an odd world with an uneven split at the smallest streaming width (column strips 58 + 6)"),
    "deep3_97x70": dict(
        shape=(97, 70), ranges=((0, 30), (30, 37), (67, 30)), halo=24, runs=("atm", "ocean", "coupled"),
        switches=("QD_STREAM_NO_PAIR=1", "QD_PEER_ONE_LAUNCH=0", "QD_FUSED_FAST=0"),
        claims=("deep_halo_pair", "form_flips_within_a_step", "wrap_segment_streams"),
        # measured: atmosphere vs oracle 6.9e-6; ocean vs globe 8.9e-3, vs oracle 9.6e-5; coupled vs globe 7.9e-4, vs oracle 1.1e-5
        evidence={("atm", "host"): {0: dict(cnt_dyn_stream=EQ(2), cnt_dyn_tile=EQ(1), max_mom_segs=EQ(2)), 1: INNER_DYN,
                                    2: dict(cnt_dyn_stream=EQ(2), cnt_dyn_tile=EQ(1))},
                  ("ocean", "peer0"): {0: dict(cnt_ocn_stream=EQ(6), cnt_ocn_tile=EQ(3), max_mom_segs=EQ(2), max_tail_segs=EQ(2)),
                                       1: dict(cnt_ocn_stream=EQ(9), cnt_split=EQ(0)), 2: dict(cnt_ocn_stream=EQ(6), cnt_ocn_tile=EQ(3))},
                  ("ocean", "peer1"): {0: dict(cnt_split=EQ(0)),                                   # 30 - 24 = 6 interior rows: not split
                                       1: dict(cnt_split=GT(0), cnt_split_redo=EQ(0), cnt_stream_pair=GT(0), cnt_stream_push=EQ(0))},
                  ("ocean", "peer2"): {1: dict(cnt_split=GT(0), cnt_split_redo=EQ(0), cnt_stream_pair=GT(0), cnt_stream_push=GT(0))}},
        why="hand-made ranges 30 + 37 + 30, halo 24: one exchange per three sub-steps, ocean momentum at margins 19 / 12 / 5 -- a polar "
            "band's wrap segment streams at 19 and 12 rows (the other pole's eta row is on its slab) and falls to tiles at 5; the middle "
            "band's split has an interior of 37 - 24 = 13 rows and boundary strips of 31 rows each (k_ocn_stream_pair, k_ocn_stream_push); "
            "an even split of 97 rows leaves no band both tall enough for that interior and short enough for its slab"),
    "thinhalo3_40x64": dict(
        shape=(40, 64), world=3, halo=(5, 6, 7, 9), runs=("ocean",), switches=(),
        claims=("band_tail_halo_threshold",),
        no_coupled="the atmosphere needs a halo of 12 rows: these halos carry the ocean step alone",
        # measured: ocean vs globe 1.7e-4, vs oracle 3.0e-5
        evidence={("ocean", "peer0", 5): {b: dict(cnt_sub_round2=EQ(9), cnt_sub_band_tail=EQ(0), cnt_ocn_stream=EQ(9), max_mom_segs=EQ(1)) for b in (0, 1, 2)},
                  ("ocean", "peer0", 6): {0: dict(cnt_sub_round2=EQ(9), cnt_ocn_tile=EQ(9), max_mom_segs=EQ(2)), 1: dict(cnt_ocn_stream=EQ(9))},
                  ("ocean", "peer0", 7): {0: dict(cnt_sub_band_tail=EQ(9), cnt_sub_round2=EQ(0), cnt_ocn_tile=EQ(9), max_tail_segs=EQ(1))},
                  ("ocean", "peer0", 9): {0: dict(cnt_sub_band_tail=EQ(9), max_tail_segs=EQ(2)), 1: dict(max_tail_segs=EQ(1))},
                  ("ocean", "collective", 6): {0: dict(cnt_sub_round2=EQ(9))}, ("ocean", "collective", 7): {0: dict(cnt_sub_band_tail=EQ(9))}},
        why="14 + 13 + 13 rows, ocean step only, halos around max(7, Ro + 2) = 7: 5 and 6 take the round-2 sub-step, 7 and 9 the band tail "
            "(tests/test_gpu_bands.py's thin-halo test at the smallest width that takes the one-launch tail)"),
}
IDS = tuple(CASES)
COUPLED_IDS = tuple(k for k in IDS if "coupled" in CASES[k]["runs"])

# DriverOracle against itself, initial zonal wind scaled by 1 + 1e-15, NSTEPS steps at run_cfl (3 sub-steps an ocean step): the largest
# deviation of uo, vo, eta relative to each field's max-norm.  Measured on the CPU by band_sensitivity() below and recomputed by
# tests/test_band_form_cases_cpu.py (it fails when one has drifted by more than 10 x).
# (three rows have a coupled run; each of the other five says why not under `no_coupled`)
BAND_SENS = {"polar2_48x65": 6.5e-16, "five_61x64": 5.5e-16, "deep3_97x70": 2.7e-15}


def band_bound(cid):
    """Bands against the whole globe (and transport against transport where only the order of the eta sum differs):
    max(1e-12, 1000 x the oracle's own sensitivity) -- a rounding difference of a few hundred ulp entering at each step"""
    return max(BAND_TOL, 1000.0 * BAND_SENS.get(cid, 0.0))


def oracle_bound(cid):
    """uo, vo, eta of a coupled band run against DriverOracle: step_form_cases.coupled_bound with this table's sensitivities"""
    return min(1e-7, max(STEP_TOL, 1000.0 * BAND_SENS[cid]))


def ranges_of(cid):
    from qingdai_amd.bands import band_ranges
    c = CASES[cid]
    return [tuple(r) for r in c["ranges"]] if "ranges" in c else band_ranges(c["shape"][0], c["world"])


def halos_of(cid):
    h = CASES[cid]["halo"]
    return tuple(h) if isinstance(h, tuple) else (h,)


def env_of(switches):
    return dict(s.split("=") for s in switches)


# ---------------------------------------------------------------- the launchers' geometry, restated for the CPU test
def seg_ok(row0, nrows, nlat):
    """qs_seg_ok (qd_stream.hip)"""
    s1 = row0 + nrows
    return not ((0 < row0 < 5) or (nlat - 5 < s1 < nlat) or nrows < 10)


def on_slab(row, row0, nrows, halo, nlat):
    """host_lrow(G, row) < G.lrows_ : the global row is one of the band's slab rows"""
    return (row - (row0 - halo)) % nlat < nrows + 2 * halo


def fast_tile(tr, seg, i0, nlat, nlon, lbase, lrows):
    """qd_fast_tile<TR> (qd_fused.hip) for the tile that owns rows from i0 of the launch segment `seg` = (row0, nrows) on a slab whose
    first row is global row lbase -> dict(p0, fits, interior, shifted, slab_edge)"""
    ra = tr + 10
    s0, s1 = seg[0], seg[0] + seg[1]
    lo, hi = (0 if s0 == 0 else s0 - 5), (nlat if s1 == nlat else s1 + 5)
    x = i0 - 5
    p0 = lo if x < lo else (hi - ra if x > hi - ra else x)              # qd_clampi(i0 - 5, lo, hi - RA)
    lrow = (p0 - lbase) % nlat
    fits = hi - lo >= ra and lo >= 0 and hi <= nlat and lrow + ra <= lrows and nlon >= 64
    return dict(p0=p0, fits=fits, interior=p0 >= 2 and p0 + ra <= nlat - 2, shifted=p0 != i0 - 5, slab_edge=lrow + ra == lrows)


def ocn_reach(shape, n_sub=3):
    """qd_adv_reach(sub_dt, 4 m/s)"""
    import qd_oracle as qo
    return int(np.ceil(4.0 * (DT / n_sub) / (qo.defaults().a * np.pi / (shape[0] - 1)))) + 1


def plan_chain(shape, halo, with_atm=True, n_sub=3, nlon=None):
    """One coupled step as the planner sees it: (tag, inputs [(field, radius)], outputs) in launch order, the radii of qd_atmos.hip /
    qd_ocean.hip.  tag 'dyn' / 'ocn' / 'tail': the launches whose margin decides a form; 'wide' plans without a launch.  TAUX / TAUY /
    T1 are scratch slabs of the library: ISR_A / ISR_B / TEQ stand in for them."""
    from qingdai_amd.bands import adv_reach
    R, Ro = adv_reach(shape[0], DT), ocn_reach(shape, n_sub)
    band_tail = (nlon if nlon is not None else shape[1]) >= 64 and halo >= max(7, Ro + 2)
    ops = []
    if with_atm:
        ops += [("column", [("U", 0), ("V", 0), ("H", 0), ("TS", 0), ("Q", 0)], ["H", "TS", "Q"]),
                ("gather", [("TS", R), ("Q", R), ("U", 0), ("V", 0)], ["TS", "Q"]),
                ("dyn", [("H", 5), ("U", 4), ("V", 4), ("Q", 4), ("CLOUD", 4)], ["U", "V", "H", "Q", "CLOUD"]),
                ("shapiro", [("U", 2), ("V", 2), ("H", 2)], ["U", "V", "H"]),
                ("cloud", [("CLOUD", R), ("U", 0), ("V", 0), ("H", 0)], ["U", "V", "H", "TS", "Q", "CLOUD"])]
    ops += [("stress", [("U", 0), ("V", 0), ("UO", 0), ("VO", 0)], ["ISR_A", "ISR_B"])]
    for _ in range(n_sub):
        if band_tail:
            ops += [("wide", [("ETA", 7), ("UO", 6), ("VO", 6), ("ISR_A", 6), ("ISR_B", 6), ("SST", Ro + 2)], [])]
        ops += [("ocn", [("ETA", 5), ("UO", 4), ("VO", 4), ("ISR_A", 4), ("ISR_B", 4)], ["UO", "VO", "ETA"])]
        if band_tail:
            ops += [("tail", [("UO", 2), ("VO", 2), ("ETA", 0), ("SST", Ro + 2), ("QNET", 0)], ["ETA", "SST", "UO", "VO"])]
        else:
            ops += [("cont", [("UO", 1), ("VO", 1), ("ETA", 0), ("SST", Ro)], ["TEQ", "ETA"]),
                    ("sst", [("TEQ", 2), ("QNET", 0), ("UO", 1), ("VO", 1), ("ETA", 0)], ["SST", "UO", "VO"])]
    return ops


# ---------------------------------------------------------------- states
def seed_of(cid):
    return 300 + IDS.index(cid)


def atm_state(cid):
    """step_form_cases.perturbed_state, wet / cloudy / icy, as the device's field names"""
    st = sc.perturbed_state(CASES[cid]["shape"], seed_of(cid), wet=True, cloudy=True, icy=True)
    return {"U": st["u"], "V": st["v"], "H": st["h"], "TS": st["T_s"], "Q": st["q"], "CLOUD": st["cloud_cover"], "HICE": st["h_ice"]}


def ocean_state(cid):
    """step_form_cases.fast_ocean_state (currents at the 3 m/s cap with fast pole rows, eta inside its clip, an ice mask) with the wind
    slowed to 15 m/s, so that the gravity-wave speed sets the sub-step count (3 at run_cfl)"""
    mask, s = sc.fast_ocean_state(CASES[cid]["shape"])
    s = dict(s)
    s["u_atm"] = s["u_atm"] * (15.0 / 250.0); s["v_atm"] = s["v_atm"] * (15.0 / 250.0)
    return mask, s


def coupled_oracle(cid, land_mask, base_albedo, friction, scale=1.0):
    """step_form_cases.coupled_oracle at ocean_cfl = run_cfl (3 sub-steps an ocean step); returns (atmosphere, ocean, driver)"""
    import qd_oracle as qo
    from qd_oracle.driver import DriverOracle
    shape = CASES[cid]["shape"]
    nlat, nlon = shape
    st = sc.coupled_state(shape, land_mask)
    g = qo.Grid(nlat, nlon)
    P = qo.defaults(ocean_cfl=sc.run_cfl(shape))
    m = qo.AtmosOracle(g, friction, land_mask, P, C_s_map=np.where(land_mask == 1, 3e6, P.Cs_ocean).astype(float))
    m.h, m.T_s, m.u, m.v = st["h"].copy(), st["T_s"].copy(), st["u"] * scale, st["v"].copy()
    oc = qo.OceanOracle(g, land_mask, P, init_Ts=np.full((nlat, nlon), 288.0))
    d = DriverOracle(g, m, oc, qo.Forcing(g), land_mask, base_albedo, P)
    d.S_snow = st["S_snow"].copy()
    for i in range(NSTEPS):
        d.step(i * DT, DT)
    return m, oc, d


def band_sensitivity(cid):
    """step_form_cases.coupled_sensitivity for a row of this table -> (ocean, atmosphere / surface)"""
    from util import surface, relerr
    _, mask, alb, fric = surface(*CASES[cid]["shape"])
    a = coupled_oracle(cid, mask, alb, fric)
    b = coupled_oracle(cid, mask, alb, fric, scale=1.0 + 1e-15)
    ocn = max(relerr(getattr(a[1], k), getattr(b[1], k)) for k in ("uo", "vo", "eta"))
    atm = max(relerr(getattr(a[0], k), getattr(b[0], k)) for k in ("u", "v", "h", "T_s", "q", "cloud_cover"))
    return ocn, atm
