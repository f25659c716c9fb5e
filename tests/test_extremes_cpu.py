"""CPU: the host side of the extremes lane (qingdai_amd/extremes.py) -- switches, the three parsers and their refusals, labels and
file names, the header constants, and accumulate_reference against an independent, deliberately slow statement (per-cell Python
loops, spells by itertools.groupby, the histogram from a sort plus edge comparisons) on hostile values, bit for bit."""
import itertools
import os
import re

import numpy as np
import pytest

from qingdai_amd import extremes as ex

HERE = os.path.dirname(os.path.abspath(__file__))
FIELDS = ["TS", "PRECIP", "WIND_SPEED", "H"]


# ---------------------------------------------------------------- switches
def test_switches_and_fallbacks():
    off = ex.read_env({})
    assert off == {"enabled": False, "fields": None, "thresholds": None, "bins": None, "sample_every": 4, "every_days": 10.0}
    on = ex.read_env({"QD_EXTREMES": "1", "QD_EXTREMES_FIELDS": " ts , precip ", "QD_EXTREMES_THRESHOLDS": "ts<250",
                      "QD_EXTREMES_BINS": "precip:log:1e-9:1e-3:8", "QD_EXTREMES_SAMPLE_EVERY": "3", "QD_EXTREMES_EVERY_DAYS": "0.5"})
    assert on == {"enabled": True, "fields": ["TS", "PRECIP"], "thresholds": "ts<250", "bins": "precip:log:1e-9:1e-3:8",
                  "sample_every": 3, "every_days": 0.5}
    for bad in ("0", "-2", "x", ""):
        assert ex.read_env({"QD_EXTREMES_SAMPLE_EVERY": bad})["sample_every"] == 4
    for bad in ("0", "-1", "nan", "inf", "x"):
        assert ex.read_env({"QD_EXTREMES_EVERY_DAYS": bad})["every_days"] == 10.0
    assert not ex.read_env({"QD_EXTREMES": "2"})["enabled"] and not ex.read_env({"QD_EXTREMES": "yes"})["enabled"]
    assert ex.read_env({"QD_EXTREMES": "1", "QD_EXTREMES_BINS": "  "})["bins"] is None
    # lists that would be refused are not looked at while the lane is off
    assert ex.read_env({"QD_EXTREMES_THRESHOLDS": "NOPE<1"})["thresholds"] == "NOPE<1"
    with pytest.raises(ValueError, match="QD_EXTREMES_THRESHOLDS: 'NOPE<1': 'NOPE' is not among the lane's fields"):
        ex.read_env({"QD_EXTREMES": "1", "QD_EXTREMES_THRESHOLDS": "NOPE<1"})
    with pytest.raises(ValueError, match="QD_EXTREMES_FIELDS: unknown field 'NOPE'"):
        ex.read_env({"QD_EXTREMES": "1", "QD_EXTREMES_FIELDS": "TS,NOPE"})
    # the defaults parse against the default fields
    assert [t[:2] for t in ex.parse_thresholds(ex.DEFAULT_THRESHOLDS, FIELDS)] == [("TS", "<"), ("PRECIP", ">")]
    assert [(n, e.size) for n, e in ex.parse_bins(ex.DEFAULT_BINS, FIELDS)] == [("PRECIP", 61), ("TS", 101), ("WIND_SPEED", 101)]
    assert ex.resolve_fields(None, True) == FIELDS + ["SST"] and ex.resolve_fields(None, False) == FIELDS
    with pytest.raises(ValueError, match="QD_EXTREMES_FIELDS: field 'SST' needs the ocean"):
        ex.resolve_fields(["SST"], False)
    with pytest.raises(ValueError, match="QD_EXTREMES_FIELDS: 17 entries, at most 16"):
        ex.parse_fields(",".join(["TS"] * 17))


def test_threshold_parser_and_refusals():
    assert ex.parse_thresholds(" ts<273.15 , PRECIP>1.1574e-5,TS<-3", FIELDS) == [("TS", "<", 273.15), ("PRECIP", ">", 1.1574e-5), ("TS", "<", -3.0)]
    for bad, why in (("TS=3", "'TS=3' is not NAME<value or NAME>value"), ("<3", "is not NAME<value"), ("TS<", "is not NAME<value"),
                     ("TS<1<2", "is not NAME<value"), ("TS<abc", "'abc' is not a number"), ("TS<inf", "is not finite"),
                     ("TS<nan", "is not finite"), ("SST<280", "'SST' is not among the lane's fields"),
                     ("TS<273.15,TS<273.15", "the threshold 'TS<273.15' is named twice")):
        with pytest.raises(ValueError, match="QD_EXTREMES_THRESHOLDS: .*" + re.escape(why)):
            ex.parse_thresholds(bad, FIELDS)
    with pytest.raises(ValueError, match="17 thresholds, at most 16"):
        ex.parse_thresholds(",".join(f"TS<{k}" for k in range(17)), FIELDS)


def test_bin_parser_and_refusals():
    (name, e), = ex.parse_bins("ts:lin:150:350:100", FIELDS)
    assert name == "TS" and e.size == 101 and e[0] == 150.0 and e[-1] == 350.0 and np.all(np.diff(e) > 0)
    (_, e), = ex.parse_bins("PRECIP:log:1e-8:1e-2:60", FIELDS)
    assert e.size == 61 and e[0] == 1e-8 and e[-1] == 1e-2 and np.allclose(np.diff(np.log10(e)), 0.1)
    for bad, why in (("TS:lin:1:2", "is not NAME:lin:lo:hi:n or NAME:log:lo:hi:n"), ("TS:cube:1:2:3", "is not NAME:lin:lo:hi:n"),
                     ("TS:lin:a:2:3", "'a' is not a number"), ("TS:lin:1:2:x", "'x' is not a bin count"),
                     ("TS:log:0:2:3", "log bins need lo > 0"), ("TS:log:-1:2:3", "log bins need lo > 0"),
                     ("TS:lin:2:2:3", "hi is not above lo"), ("TS:lin:3:2:3", "hi is not above lo"), ("TS:lin:1:2:0", "0 bins, 1 to 256"),
                     ("TS:lin:1:2:257", "257 bins, 1 to 256"), ("SST:lin:1:2:3", "'SST' is not among the lane's fields"),
                     ("TS:lin:1:2:3,TS:lin:1:2:4", "'TS' is binned twice"), ("TS:lin:1:inf:3", "is not finite")):
        with pytest.raises(ValueError, match="QD_EXTREMES_BINS: .*" + re.escape(why)):
            ex.parse_bins(bad, FIELDS)
    for bad, why in (([1.0], "fewer than 2 edges"), ([1.0, 1.0], "not finite and strictly increasing"), ([2.0, 1.0], "strictly increasing"),
                     ([1.0, np.nan], "not finite"), ([0.0, np.inf], "not finite"), (np.arange(258.0), "257 bins, at most 256")):
        with pytest.raises(ValueError, match=why):
            ex.check_edges(bad, "x")
    assert ex.check_edges(np.arange(257.0), "x").size == 257


def test_labels_and_file_names():
    assert ex.threshold_label("TS", "<", 273.15) == "TS_lt_273p15"
    assert ex.threshold_label("PRECIP", ">", 1.1574e-5) == "PRECIP_gt_1p1574em05"
    assert ex.threshold_label("TS", "<", -3.0) == "TS_lt_m3"
    assert ex.file_name(0.0, 9.9) == "extremes_day_00.0_09.9.nc" and ex.file_name(0.0, 0.05, 2) == "extremes_day_00.00_00.05.nc"


def test_header_surface():
    from qingdai_amd import _lib
    from qingdai_amd.device import Device
    C = _lib.C
    assert C["QD_ABI_VERSION"] == 1
    assert (C["QD_EXTREMES_MAX_ENTRIES"], C["QD_EXTREMES_MAX_THRESHOLDS"], C["QD_EXTREMES_MAX_HISTS"], C["QD_EXTREMES_MAX_BINS"]) == (16, 16, 8, 256)
    assert (C["QD_EXTREMES_CMP_LT"], C["QD_EXTREMES_CMP_GT"]) == (ord("<"), ord(">"))
    assert [_lib.state_ref(n) for n in ("EXTREMES_VALUES", "EXTREMES_COUNTS", "EXTREMES_HIST")] == [505, 506, 507]
    for n in ("qd_extremes_configure", "qd_extremes_schedule", "qd_extremes_sample", "qd_extremes_read", "qd_extremes_restore", "qd_extremes_reset"):
        assert n in _lib.SYMBOLS and hasattr(Device, n[3:]), n
    assert [s[0] for s in _lib.SIGNATURES["qd_extremes_configure"]] == ["h", "n_entries", "op", "a", "b", "n_thresholds", "thr_entry", "thr_cmp",
                                                                       "thr_value", "n_hists", "hist_entry", "hist_nb", "edges"]
    assert [(s[0], s[2]) for s in _lib.SIGNATURES["qd_extremes_read"]] == [("h", "qd_handle"), ("values", "double"), ("counts", "int32_t"),
                                                                          ("thresholds", "int32_t"), ("hist", "int64_t"), ("count", "int64_t")]
    assert [s[0] for s in _lib.SIGNATURES["qd_extremes_restore"]] == ["h", "values", "counts", "thresholds", "hist", "count"]
    assert [s[0] for s in _lib.SIGNATURES["qd_extremes_schedule"]] == ["h", "steps", "sample"]
    assert "extremes" not in " ".join(_lib.STEP_BITS)            # no flag bit: a schedule turns the lane on
    src = open(os.path.join(HERE, "..", "qingdai_amd", "csrc", "qd_span.h")).read()
    assert re.search(r"QD_LANE_HISTORY, QD_LANE_EXTREMES,", src) and re.search(r"QD_LANE_EDDY, QD_N_LANES", src)


# ---------------------------------------------------------------- the slow statement
def slow_state(samples, thresholds, hists):
    """Per-cell Python loops over the whole series of a window."""
    samples = [np.asarray(s, dtype=np.float64) for s in samples]
    E, nlat, nlon = samples[0].shape
    N = len(samples)
    st = {"vmax": np.empty((E, nlat, nlon)), "vmin": np.empty((E, nlat, nlon)), "tmax": np.empty((E, nlat, nlon), dtype=np.int32),
          "tmin": np.empty((E, nlat, nlon), dtype=np.int32), "nan": np.empty((E, nlat, nlon), dtype=np.int32),
          "thr": np.empty((len(thresholds), nlat, nlon, 4), dtype=np.uint32), "hist": [], "n": N}
    for e in range(E):
        for j in range(nlat):
            for i in range(nlon):
                xs = [float(s[e, j, i]) for s in samples]
                vmax, vmin, tmax, tmin = -np.inf, np.inf, -1, -1
                for k, x in enumerate(xs):
                    if x > vmax:
                        vmax, tmax = x, k
                    if x < vmin:
                        vmin, tmin = x, k
                st["vmax"][e, j, i], st["vmin"][e, j, i], st["tmax"][e, j, i], st["tmin"][e, j, i] = vmax, vmin, tmax, tmin
                st["nan"][e, j, i] = sum(1 for x in xs if x != x)
    for t, (e, cmp, value) in enumerate(thresholds):
        for j in range(nlat):
            for i in range(nlon):
                hits = [(float(s[e, j, i]) > value) if cmp == ">" else (float(s[e, j, i]) < value) for s in samples]
                groups = [(key, len(list(g))) for key, g in itertools.groupby(hits)]
                runs = [n for key, n in groups if key]
                st["thr"][t, j, i] = (sum(hits), groups[-1][1] if groups and groups[-1][0] else 0, max(runs, default=0), len(runs))
    for e, edges in hists:
        edges = [float(x) for x in edges]
        nb = len(edges) - 1
        table = np.zeros((nlat, nb + 3), dtype=np.int64)
        for j in range(nlat):
            xs = sorted(float(s[e, j, i]) for s in samples for i in range(nlon) if s[e, j, i] == s[e, j, i])
            table[j, nb + 2] = N * nlon - len(xs)
            table[j, 0] = sum(1 for x in xs if x < edges[0])
            table[j, nb + 1] = sum(1 for x in xs if x >= edges[nb])
            for b in range(nb):
                table[j, 1 + b] = sum(1 for x in xs if edges[b] <= x < edges[b + 1])
        st["hist"].append(table)
    return st


def same_state(a, b):
    for k in ("vmax", "vmin"):
        assert np.array_equal(np.asarray(a[k]).view(np.int64), np.asarray(b[k]).view(np.int64)), k
    for k in ("tmax", "tmin", "nan", "thr"):
        assert np.asarray(a[k]).dtype == np.asarray(b[k]).dtype and np.array_equal(a[k], b[k]), k
    assert len(a["hist"]) == len(b["hist"]) and all(np.array_equal(x, y) for x, y in zip(a["hist"], b["hist"]))
    assert a["n"] == b["n"]


EDGES = np.array([-1.0, 0.0, 0.5, 1.0, 2.5, 7.0])


def hostile(shape, N, seed):
    """[N][2][n_lat][n_lon]: entry 0 gaussian around the edges with every hostile value planted, entry 1 lognormal"""
    rng = np.random.default_rng(seed)
    nlat, nlon = shape
    s = np.stack([rng.normal(0.8, 1.5, (N, nlat, nlon)), np.exp(rng.normal(-12.0, 3.0, (N, nlat, nlon)))], axis=1)
    a = s[:, 0]
    a[0, 0, 0] = np.nan; a[N // 2, 0, 1] = np.nan; a[N - 1, 0, 2] = np.nan       # NaN in the first, a middle and the last sample
    a[:, 0, 3] = np.nan                                                          # NaN throughout: t = -1
    a[2, 1, 0] = np.inf; a[3, 1, 1] = -np.inf; a[1, 1, 2] = np.inf; a[4, 1, 2] = np.inf
    a[:, 1, 3] = 0.25; a[1, 1, 3] = -0.0; a[2, 1, 3] = 0.0; a[3, 1, 3] = -0.0     # -0.0 then +0.0 as the minimum: the earlier one stays
    a[:, 2, 0] = 0.3; a[2, 2, 0] = 5.0; a[5, 2, 0] = 5.0; a[1, 2, 0] = -4.0; a[min(7, N - 1), 2, 0] = -4.0     # ties: the earliest is kept
    vals = list(EDGES) + [np.nextafter(x, -np.inf) for x in EDGES] + [np.nextafter(x, np.inf) for x in EDGES]     # on and beside every edge
    vals += [5e-324, -5e-324, 2.2e-308, -0.0]                                    # subnormals, and -0.0 against the edge at 0.0
    for n, x in enumerate(vals):
        a[n % N, 2, 1 + (n // N) % (nlon - 1)] = x
    a[:, 2, nlon - 1] = EDGES[-1]                                                # x == e_nb throughout: over
    return s


THRESHOLDS = [(0, "<", 0.5), (0, ">", 0.5), (1, ">", 1.1574e-5), (0, ">", EDGES[-1])]
HISTS = [(0, EDGES), (1, ex.make_edges("log", 1e-8, 1e-2, 12)), (0, np.array([0.0, 1.0]))]


@pytest.mark.parametrize("shape, N", [((3, 4), 12), ((5, 7), 13)])
def test_reference_equals_the_slow_statement(shape, N):
    s = hostile(shape, N, 7)
    got, want = ex.accumulate_reference(s, THRESHOLDS, HISTS), slow_state(s, THRESHOLDS, HISTS)
    same_state(got, want)
    a = s[:, 0]
    # the planted cases, spelled out
    assert got["tmax"][0, 0, 3] == -1 and got["tmin"][0, 0, 3] == -1 and got["nan"][0, 0, 3] == N and np.isneginf(got["vmax"][0, 0, 3])
    assert got["nan"][0, 0, 0] == 1 and got["tmax"][0, 0, 0] >= 1
    assert got["vmax"][0, 1, 0] == np.inf and got["tmax"][0, 1, 0] == 2 and got["vmin"][0, 1, 1] == -np.inf and got["tmin"][0, 1, 1] == 3
    assert got["tmax"][0, 1, 2] == 1                                             # +inf twice: the earliest
    assert got["tmin"][0, 1, 3] == 1 and np.signbit(got["vmin"][0, 1, 3])         # -0.0 came first and +0.0 does not displace it
    assert (got["tmax"][0, 2, 0], got["tmin"][0, 2, 0]) == (2, 1)
    h = got["hist"][0]
    assert h[2, -2] >= N                                                         # x == e_nb went to over
    # closure: every row's columns sum to n_lon * N
    for e, table in zip(HISTS, got["hist"]):
        assert np.array_equal(table.sum(axis=1), np.full(shape[0], shape[1] * N))
    # -0.0 with an edge at 0.0 lands in the bin that starts there; the value below every edge in under
    assert ex.bin_columns(np.array([-0.0, 0.0, -5e-324, np.nextafter(1.0, 0.0), 1.0, np.nan]), [0.0, 1.0]).tolist() == [1, 1, 0, 1, 2, 3]
    # the file's view of the cell without a sample
    _, v = ex.window_variables(got, ["A", "B"], [("A", "<", 0.5)], [("A", EDGES)], np.linspace(-60, 60, shape[0]), np.arange(shape[1]) * 1.0, 100.0, 1200.0)
    assert np.isnan(v["a_max"][2][0, 3]) and np.isnan(v["a_tmax_seconds"][2][0, 3]) and v["a_nan"][2][0, 3] == N
    assert v["a_tmax_seconds"][2][1, 0] == 100.0 + 2 * 1200.0
    assert a.shape == (N,) + shape


def test_continuation_from_a_state():
    s = hostile((5, 7), 13, 11)
    whole = ex.accumulate_reference(s, THRESHOLDS, HISTS)
    for cut in (1, 6, 12):
        first = ex.accumulate_reference(s[:cut], THRESHOLDS, HISTS)
        keep = {k: (np.array(v, copy=True) if k not in ("hist", "n") else v) for k, v in first.items()}
        same_state(ex.accumulate_reference(s[cut:], THRESHOLDS, HISTS, state=first), whole)
        same_state(first, keep)                                                  # the state handed in is left as it was
    with pytest.raises(ValueError):
        ex.accumulate_reference([], THRESHOLDS, HISTS)


def test_threshold_summary():
    s = np.zeros((8, 1, 1, 2))
    s[:, 0, 0, 0] = [1, 1, 0, 1, 1, 1, 0, 1]                                     # spells 2, 3 and an open one of 1
    st = ex.accumulate_reference(s, [(0, ">", 0.5)], [])
    assert st["thr"][0, 0, 0].tolist() == [6, 1, 3, 3] and st["thr"][0, 0, 1].tolist() == [0, 0, 0, 0]
    t = ex.threshold_summary(st["thr"][0], st["n"], 1200.0)
    assert t["count"][0, 0] == 6 and t["spells"][0, 0] == 3 and t["open"][0, 0] == 1 and t["freq"][0, 0] == 6 / 8
    assert t["longest_seconds"][0, 0] == 3600.0 and t["mean_spell_seconds"][0, 0] == 2400.0 and np.isnan(t["mean_spell_seconds"][0, 1])
    assert t["count"].dtype == np.int32 and t["freq"].dtype == np.float64


def test_quantiles_lie_in_numpys_bin():
    """hist_summary's quantile and np.quantile of the same values under the same weights (the inverted CDF) fall into the same bin of
    the table, so they differ by at most that bin's width: the levels and the sample are chosen so that no level's cumulative weight
    comes near a bin's boundary (checked below), hence the bound is derived, not tuned."""
    rng = np.random.default_rng(3)
    nlat, nlon, N = 9, 16, 25
    lat = np.linspace(-80.0, 80.0, nlat)
    x = rng.gamma(2.0, 1.5, (N, 1, nlat, nlon))
    edges = np.linspace(0.0, 30.0, 121)
    st = ex.accumulate_reference(x, [], [(0, edges)])
    got = ex.hist_summary(st["hist"][0], edges, lat)
    assert got["under_frac"] == 0.0 and got["over_frac"] == 0.0 and got["nan_frac"] == 0.0 and abs(got["pdf"].sum() - 1.0) < 1e-12
    w = np.broadcast_to(ex.row_weights(lat)[None, :, None], (N, nlat, nlon)).ravel()
    vals = x[:, 0].ravel()
    order = np.argsort(vals)
    cw = np.cumsum(w[order]) / np.sum(w)
    for level, q in zip(ex.QUANTILE_LEVELS, got["quantiles"]):
        want = float(np.quantile(vals, level, weights=w, method="inverted_cdf"))
        b = int(np.searchsorted(edges, want, side="right")) - 1
        # strictly inside: the cumulative weight behind either edge of the bin is away from the level
        below, above = cw[vals[order] < edges[b]], cw[vals[order] < edges[b + 1]]
        assert (below[-1] if below.size else 0.0) < level - 1e-9 and above[-1] > level + 1e-9
        assert edges[b] <= q <= edges[b + 1], (level, q, want)
        assert abs(q - want) <= edges[b + 1] - edges[b]
    # a level that falls into under or over is NaN; so is everything without a sample
    x2 = np.concatenate([np.full(30, -1.0), np.full(40, 0.5), np.full(30, 9.0)]).reshape(1, 1, 1, 100)
    s2 = ex.hist_summary(ex.accumulate_reference(x2, [], [(0, [0.0, 1.0])])["hist"][0], [0.0, 1.0], [0.0], levels=(0.1, 0.3, 0.5, 0.7, 0.71, 0.99))
    assert np.isnan(s2["quantiles"][[0, 1, 4, 5]]).all() and s2["quantiles"][2] == 0.5 and s2["quantiles"][3] == 1.0
    assert (s2["under_frac"], s2["over_frac"]) == (0.3, 0.3)
    empty = ex.hist_summary(np.zeros((1, 4), dtype=np.int64), [0.0, 1.0], [0.0])
    assert np.isnan(empty["quantiles"]).all() and np.isnan(empty["pdf"]).all() and np.isnan(empty["under_frac"])


# ---------------------------------------------------------------- the lane through a stand-in device
class FakeDevice:
    class params:
        omega = 2.0 * np.pi / 72000.0

    def __init__(self, shape):
        self.shape, self.calls, self.state, self.cfg = shape, [], None, None

    def extremes_configure(self, entries, thresholds, hists):
        self.cfg = (entries, thresholds, hists)

    def extremes_schedule(self, flags):
        self.calls.append(("schedule", np.asarray(flags).tolist()))

    def extremes_read(self):
        return self.state

    def extremes_reset(self):
        self.calls.append(("reset",))
        self.state = dict(self.state, n=0)


class Grid:
    def __init__(self, nlat, nlon):
        self.n_lat, self.n_lon = nlat, nlon
        self.lat, self.lon = np.linspace(-80.0, 80.0, nlat), np.arange(nlon) * (360.0 / nlon)
        self.lat_mesh = np.repeat(self.lat[:, None], nlon, axis=1)


def test_lane_file_and_line(tmp_path):
    from qingdai_amd import ncio
    nlat, nlon, N = 5, 7, 6
    dev, lines = FakeDevice((nlat, nlon)), []
    lane = ex.Extremes(dev, Grid(nlat, nlon), {"every_days": 0.1, "sample_every": 4}, with_ocean=False, dt=300.0, day=72000.0,
                       out=lines.append, output_dir=str(tmp_path), fields=["TS", "WIND_SPEED"], thresholds="TS<0.5",
                       bins={"ts": EDGES})
    assert lane.names == ["TS", "WIND_SPEED"] and lane.S == 24
    assert dev.cfg[0] == [(0, "TS", None), (1, "U", "V")] and dev.cfg[1] == [(0, "<", 0.5)] and dev.cfg[2][0][0] == 0
    assert re.fullmatch(r"TS,WIND_SPEED\|TS_lt_0p5\|TS:5:-1\.0:7\.0:[0-9a-f]{8}\|every=4", lane.key()), lane.key()
    k = lane.span_schedule(None, 300.0, 24)
    assert dev.calls[-1] == ("schedule", [1, 0, 0, 0] * 6) and k == (24, (0.0, 6000.0), 6)
    lane._fired(k)
    assert lane.window_closed() and lane.steps_to_window_end() == 24
    dev.state = ex.accumulate_reference(hostile((nlat, nlon), N, 5), [(0, "<", 0.5)], [(0, EDGES)])
    path = lane.flush()
    assert os.path.basename(path) == "extremes_day_00.0_00.1.nc" and dev.calls[-1] == ("reset",) and lane.t_first is None
    v, _ = ncio.read_nc(path)
    for name, shape in (("ts_max", (nlat, nlon)), ("wind_speed_tmin_seconds", (nlat, nlon)), ("ts_nan", (nlat, nlon)),
                        ("ts_lt_0p5_count", (nlat, nlon)), ("ts_lt_0p5_freq", (nlat, nlon)), ("ts_lt_0p5_open", (nlat, nlon)),
                        ("ts_lt_0p5_spells", (nlat, nlon)), ("ts_lt_0p5_longest_seconds", (nlat, nlon)),
                        ("ts_lt_0p5_mean_spell_seconds", (nlat, nlon)), ("ts_edges", (6,)), ("ts_hist", (nlat, 8)), ("ts_pdf", (5,)),
                        ("ts_quantiles", (4,)), ("quantile_levels", (4,))):
        assert v[name].shape == shape, name
    assert int(v["n_samples"]) == N and int(v["complete"]) == 1 and int(v["sample_every"]) == 4 and float(v["dt_seconds"]) == 300.0
    assert np.array_equal(v["ts_lt_0p5_freq"], v["ts_lt_0p5_count"] / N) and np.array_equal(v["ts_hist"].sum(axis=1), np.full(nlat, nlon * N))
    assert np.isnan(v["ts_max"][0, 3]) and np.array_equal(v["ts_edges"], EDGES)
    assert re.fullmatch(r"\[Extremes\] day 0\.0–0\.1: 6 samples \| TS max=inf at \(-40\.00, 0\.00\) \| TS p99=\S+ TS_lt_0p5 freq=\S+", lines[0]), lines
    # an empty window writes nothing
    assert lane.flush() is None and len(lines) == 1
    # refusals of the caller's own lists
    with pytest.raises(ValueError, match="'SST' is not among the lane's fields"):
        ex.Extremes(dev, Grid(nlat, nlon), {}, fields=["TS"], thresholds="", bins={"SST": [0.0, 1.0]})
    with pytest.raises(ValueError, match="strictly increasing"):
        ex.Extremes(dev, Grid(nlat, nlon), {}, fields=["TS"], thresholds="", bins={"TS": [0.0, 0.0]})
    # the defaults keep what names a field of the run
    lane = ex.Extremes(dev, Grid(nlat, nlon), {}, with_ocean=False, fields=["TS", "H"])
    assert [t[0] for t in lane.thresholds] == ["TS"] and [h[0] for h in lane.hists] == ["TS"]
    assert ex.from_env(dev, Grid(nlat, nlon), {}) is None and ex.from_env(dev, Grid(nlat, nlon), {"QD_EXTREMES": "0"}) is None
