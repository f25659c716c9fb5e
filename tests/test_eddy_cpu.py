"""CPU: the host side of the eddy lane (qingdai_amd/eddy.py) -- switches, the pair parser, the clock, the file and the line through
a stand-in device, the header constants, the decomposition against an analytic field, and accumulate_reference against exact
rational arithmetic (with the raw form sum(ab)/N - sum(a)sum(b)/N^2 missing the same bound: the reason for the anchor)."""
import os
import re
from fractions import Fraction

import numpy as np
import pytest

from qingdai_amd import eddy, history as hs

HERE = os.path.dirname(os.path.abspath(__file__))
DAY, DT = 72000.0, 300.0


# ---------------------------------------------------------------- switches
def test_switches_and_fallbacks():
    off = eddy.read_env({})
    assert off == {"enabled": False, "pairs": "U*V,V*TS,V*Q,V*H,U*U,V*V,H*H,TS*TS", "sample_every": 4, "every_days": 10.0, "maps": True}
    on = eddy.read_env({"QD_EDDY": "1", "QD_EDDY_PAIRS": " u*v , ts*ts ", "QD_EDDY_SAMPLE_EVERY": "3", "QD_EDDY_EVERY_DAYS": "0.5",
                        "QD_EDDY_MAPS": "0"})
    assert on == {"enabled": True, "pairs": "U*V,TS*TS", "sample_every": 3, "every_days": 0.5, "maps": False}
    for bad in ("0", "-2", "x", ""):
        assert eddy.read_env({"QD_EDDY_SAMPLE_EVERY": bad})["sample_every"] == 4
    for bad in ("0", "-1", "nan", "inf", "x"):
        assert eddy.read_env({"QD_EDDY_EVERY_DAYS": bad})["every_days"] == 10.0
    assert not eddy.read_env({"QD_EDDY": "2"})["enabled"] and not eddy.read_env({"QD_EDDY": "yes"})["enabled"]
    assert eddy.read_env({"QD_EDDY": "1", "QD_EDDY_PAIRS": "  "})["pairs"] == eddy.DEFAULT_PAIRS
    # a list that would be refused is not looked at while the lane is off
    assert eddy.read_env({"QD_EDDY_PAIRS": "NOPE*U"})["pairs"] == "NOPE*U"
    with pytest.raises(ValueError, match="QD_EDDY_PAIRS: unknown field 'NOPE'"):
        eddy.read_env({"QD_EDDY": "1", "QD_EDDY_PAIRS": "NOPE*U"})


def test_pair_parser_and_refusals():
    fields, pairs, labels = eddy.parse_pairs(eddy.DEFAULT_PAIRS)
    assert fields == ["U", "V", "TS", "Q", "H"]
    assert pairs == [(0, 1), (1, 2), (1, 3), (1, 4), (0, 0), (1, 1), (4, 4), (2, 2)]
    assert labels[0] == ("U", "V") and labels[-1] == ("TS", "TS")
    assert eddy.parse_pairs("vo*sst, ,Sst*SST") == (["VO", "SST"], [(0, 1), (1, 1)], [("VO", "SST"), ("SST", "SST")])
    for text, why in (("U", "'U' is not a pair A\\*B"), ("U*V*H", "is not a pair"), ("U*", "is not a pair"), ("U*NOPE", "unknown field 'NOPE'"),
                      ("WIND_SPEED*U", "'WIND_SPEED' is a derived entry"), ("V*PRECIP", "PRECIP is sampled in front of the ocean step"),
                      ("U*V,V*U", "the pair 'V\\*U' is named twice"), ("U*U,U*U", "named twice"), ("", "no pair"), (" , ", "no pair")):
        with pytest.raises(ValueError, match="QD_EDDY_PAIRS: .*" + why):
            eddy.parse_pairs(text)
    from qingdai_amd._lib import FIELDS
    names = [n for n in FIELDS if n != "PRECIP"]
    with pytest.raises(ValueError, match="QD_EDDY_PAIRS: 17 fields, at most 16"):
        eddy.parse_pairs(",".join(f"{n}*{n}" for n in names[:17]))
    many = [f"{names[i]}*{names[j]}" for i in range(8) for j in range(i, 8)]
    assert len(eddy.parse_pairs(",".join(many[:32]))[1]) == 32
    with pytest.raises(ValueError, match="QD_EDDY_PAIRS: 33 pairs, at most 32"):
        eddy.parse_pairs(",".join(many[:33]))


# ---------------------------------------------------------------- a stand-in device
class StandIn:
    def __init__(self, state=None):
        self.calls = []
        self.state = state                      # (r, S, C, N)
        self.params = None

    def eddy_configure(self, fields, pairs):
        self.calls.append(("configure", list(fields), list(pairs)))
        self.pairs = list(pairs)

    def eddy_schedule(self, flags):
        self.calls.append(("schedule", np.asarray(flags).tolist()))

    def eddy_read(self):
        return self.state

    def eddy_zonal(self):
        return eddy.zonal_reference(self.state[1], self.state[2], self.pairs)

    def eddy_reset(self):
        self.calls.append(("reset",))
        self.state = self.state[:3] + (0,) if self.state is not None else None


def make(tmp_path, state=None, pairs="U*V,TS*TS", every="0.05", k="1", maps="1", with_ocean=False, shape=(5, 6)):
    import qingdai_amd as qa
    grid = qa.SphericalGrid(*shape)
    dev = StandIn(state)
    lines = []
    cfg = eddy.read_env({"QD_EDDY": "1", "QD_EDDY_PAIRS": pairs, "QD_EDDY_EVERY_DAYS": every, "QD_EDDY_SAMPLE_EVERY": k, "QD_EDDY_MAPS": maps})
    e = eddy.Eddy(dev, grid, cfg, with_ocean=with_ocean, dt=DT, day=DAY, out=lines.append, output_dir=str(tmp_path))
    return e, dev, grid, lines


def test_clock_is_historys(tmp_path):
    e, dev, _, _ = make(tmp_path, every="0.05", k="3")
    assert e.S == 12 == hs.steps_per_window(0.05, DAY, DT)
    assert dev.calls[0] == ("configure", ["U", "V", "TS"], [(0, 1), (2, 2)])
    assert [e.steps_to_window_end(i) for i in (0, 5, 11, 12, 23)] == [12, 7, 1, 12, 1]
    clock = e.span_clock()
    k = e.span_schedule(None, DT, 5)
    assert dev.calls[-1] == ("schedule", hs.schedule(0, 5, 12, 3).tolist()) == ("schedule", [1, 0, 0, 1, 0]) and k == (5, (0.0, 3 * DT), 2)
    e.span_restore(clock)
    assert e.i == 0 and e.n_open == 0 and e.t_first is None
    e._fired(e.span_schedule(1000.0, DT, 5))
    assert (e.i, e.t_first, e.t_last, e.n_open) == (5, 1000.0, 1000.0 + 3 * DT, 2) and not e.window_closed()
    e._fired(e.span_schedule(1000.0 + DT * np.arange(5, 12), DT, 7))
    assert dev.calls[-1] == ("schedule", hs.schedule(5, 7, 12, 3).tolist())        # the phase restarts with the window
    assert (e.i, e.t_first, e.t_last, e.n_open) == (12, 1000.0, 1000.0 + 9 * DT, 4) and e.window_closed()
    e._fired(e.span_schedule(None, DT, 2))
    assert dev.calls[-1] == ("schedule", [1, 0])
    assert e.key() == "U*V,TS*TS|every=3|maps=1"
    with pytest.raises(ValueError, match="QD_EDDY_PAIRS: field 'VO' needs the ocean"):
        make(tmp_path, pairs="VO*SST")
    assert make(tmp_path, pairs="VO*SST", with_ocean=True)[0].fields == ["VO", "SST"]


def _state(shape, pairs, n_fields, N=6, seed=3):
    r = np.random.default_rng(seed)
    samples = [np.stack([280.0 + 5.0 * f + r.normal(size=shape) for f in range(n_fields)]) for _ in range(N)]
    return eddy.accumulate_reference(samples, pairs), samples


@pytest.mark.parametrize("maps", ["1", "0"])
def test_file_and_line(tmp_path, maps):
    from qingdai_amd import ncio
    state, samples = _state((5, 6), [(0, 1), (2, 2)], 3)
    e, dev, grid, lines = make(tmp_path, state, maps=maps, k="2")
    e.t_first, e.t_last, e.n_open = 600.0, 4200.0, 6
    path = e.flush(complete=0)
    a, b = 600.0 / DAY, 4200.0 / DAY
    assert os.path.basename(path) == f"eddy_day_{a:05.2f}_{b:05.2f}.nc" and os.path.dirname(path) == os.path.join(str(tmp_path), "eddy")
    assert os.listdir(os.path.dirname(path)) == [os.path.basename(path)]                # no temporary file is left
    v, _ = ncio.read_nc(path)
    per = {f"{p}_{part}" for p in ("u_v", "ts_ts") for part in eddy.PARTS}
    mapped = {"u_v_cov", "ts_ts_cov", "u_mean", "v_mean", "ts_mean"} if maps == "1" else set()
    assert set(v) == per | mapped | {"lat", "lon", "n_samples", "t_start_seconds", "t_end_seconds", "dt_seconds", "sample_every", "maps", "complete"}
    assert (int(v["n_samples"]), int(v["sample_every"]), int(v["complete"]), int(v["maps"])) == (6, 2, 0, int(maps))
    x = np.stack(samples)                                       # [N][F][lat][lon]: the plain two-pass answer
    mean = x.mean(axis=0)
    dev_ = x - mean
    for name, (p, q) in (("u_v", (0, 1)), ("ts_ts", (2, 2))):
        assert v[f"{name}_total"].shape == (5,) and v[f"{name}_total"].dtype == np.float64
        assert np.array_equal(v[f"{name}_total"], (v[f"{name}_mean"] + v[f"{name}_stationary"]) + v[f"{name}_transient"])
        np.testing.assert_allclose(v[f"{name}_total"], (x[:, p] * x[:, q]).mean(axis=(0, 2)), rtol=1e-12)
        np.testing.assert_allclose(v[f"{name}_mean"], mean[p].mean(axis=1) * mean[q].mean(axis=1), rtol=1e-13)
        np.testing.assert_allclose(v[f"{name}_transient"], (dev_[:, p] * dev_[:, q]).mean(axis=(0, 2)), rtol=1e-9)
        zp, zq = mean[p] - mean[p].mean(axis=1, keepdims=True), mean[q] - mean[q].mean(axis=1, keepdims=True)
        np.testing.assert_allclose(v[f"{name}_stationary"], (zp * zq).mean(axis=1), rtol=1e-9)
        if maps == "1":
            np.testing.assert_allclose(v[f"{name}_cov"], (dev_[:, p] * dev_[:, q]).mean(axis=0), rtol=1e-9, atol=1e-13)
    if maps == "1":
        np.testing.assert_allclose(v["ts_mean"], mean[2], rtol=1e-14)
    tr = v["u_v_transient"]
    j = int(np.argmax(np.abs(tr)))
    assert lines == [f"[Eddy] day {a:.2f}–{b:.2f}: 6 samples | U*V transient max |.| at lat {grid.lat[j]:.2f}: {tr[j]:.6g}"]
    assert dev.calls[-1] == ("reset",) and e.n_open == 0 and e.t_first is None and e.files == [path]
    assert e.flush() is None and len(lines) == 1                # an empty window writes nothing


def test_failed_write_leaves_nothing_behind(tmp_path, monkeypatch):
    from qingdai_amd import ncio
    state, _ = _state((5, 6), [(0, 1), (2, 2)], 3)
    e, dev, _, lines = make(tmp_path, state)
    e.t_first, e.t_last, e.n_open = 0.0, 300.0, 6

    def broken(path, dims, variables, attrs=None):
        open(path, "w").write("half a file")
        raise OSError("disk full")
    monkeypatch.setattr(ncio, "write_nc", broken)
    with pytest.raises(OSError, match="disk full"):
        e.flush()
    assert os.listdir(tmp_path / "eddy") == [] and lines == [] and e.files == []
    assert e.n_open == 6 and ("reset",) not in dev.calls       # the window is still there for the caller to decide
    e.drop()
    assert dev.calls[-1] == ("reset",) and e.n_open == 0 and e.t_first is None and e.t_last is None


def test_a_window_of_nans_still_prints(tmp_path):
    state, _ = _state((5, 6), [(0, 1), (2, 2)], 3)
    state[1][:] = np.nan
    e, _, _, lines = make(tmp_path, state)
    e.flush()
    assert lines[0].endswith("U*V transient max |.| at lat nan: nan")


# ---------------------------------------------------------------- ABI
def test_header_constants_and_surface():
    from qingdai_amd import _lib
    from qingdai_amd.device import Device
    C = _lib.C
    assert (C["QD_EDDY_MAX_FIELDS"], C["QD_EDDY_MAX_PAIRS"], C["QD_EDDY_ZONAL_SUMS"]) == (16, 32, 4)
    assert (C["QD_STATE_REF_EDDY_SUMS"], C["QD_STATE_REF_EDDY_ANCHORS"]) == (503, 504)
    assert (C["QD_STATE_REF_SPECTRA_SUMS"], C["QD_STATE_REF_FLOW_SUMS"], C["QD_STATE_REF_SPHARM_SUMS"]) == (500, 501, 502)     # the others keep theirs
    assert _lib.state_ref("EDDY_SUMS") == 503 and _lib.state_ref("EDDY_ANCHORS") == 504
    for n in ("qd_eddy_configure", "qd_eddy_schedule", "qd_eddy_sample", "qd_eddy_read", "qd_eddy_restore", "qd_eddy_zonal", "qd_eddy_reset"):
        assert n in _lib.SYMBOLS and hasattr(Device, n[3:]), n
    assert [s[0] for s in _lib.SIGNATURES["qd_eddy_configure"]] == ["h", "n_fields", "fields", "n_pairs", "p", "q"]
    assert [s[0] for s in _lib.SIGNATURES["qd_eddy_read"]] == ["h", "anchors", "sums", "pair_sums", "count"]
    assert "eddy" not in " ".join(_lib.STEP_BITS)               # no flag bit: a schedule turns the lane on
    src = open(os.path.join(HERE, "..", "qingdai_amd", "csrc", "qd_span.h")).read()
    assert re.search(r"QD_LANE_SPHARM, QD_LANE_EDDY, QD_N_LANES", src)


# ---------------------------------------------------------------- the decomposition
def synthetic(n_lat=7, n_lon=48, N=40, k=3, periods=2):
    """a = A(phi) + B cos(k lambda) + C cos(omega t + k lambda), columns periodic by index, an integer number of periods sampled"""
    lam = 2.0 * np.pi * np.arange(n_lon) / n_lon
    phi = np.linspace(-1.2, 1.2, n_lat)[:, None]
    A = (280.0 + 20.0 * np.cos(phi), 5.0 + 3.0 * np.sin(phi))
    B, Cc = (2.0, -1.5), (0.75, 1.25)
    samples = []
    for t in range(N):
        wt = 2.0 * np.pi * periods * t / N
        samples.append(np.stack([A[f] + B[f] * np.cos(k * lam)[None, :] + Cc[f] * np.cos(wt + k * lam)[None, :] for f in range(2)]))
    return samples, A, B, Cc


def test_decompose_against_the_analytic_answer():
    samples, A, B, Cc = synthetic()
    pairs = [(0, 1), (0, 0), (1, 1)]
    r, S, Cs, N = eddy.accumulate_reference(samples, pairs)
    parts = eddy.decompose(eddy.zonal_reference(S, Cs, pairs), N, eddy.time_means(r, S, N), pairs)
    for k, (p, q) in enumerate(pairs):
        np.testing.assert_allclose(parts["mean"][k], (A[p] * A[q])[:, 0], rtol=1e-12)
        np.testing.assert_allclose(parts["stationary"][k], np.full(7, B[p] * B[q] / 2.0), rtol=1e-12)
        np.testing.assert_allclose(parts["transient"][k], np.full(7, Cc[p] * Cc[q] / 2.0), rtol=1e-12)
        # the identity, exactly: the total is defined as the sum
        assert np.array_equal(parts["total"][k], (parts["mean"][k] + parts["stationary"][k]) + parts["transient"][k])
        np.testing.assert_allclose(parts["total"][k], (A[p] * A[q])[:, 0] + B[p] * B[q] / 2.0 + Cc[p] * Cc[q] / 2.0, rtol=1e-12)


def test_accumulate_reference_can_go_on_from_a_state():
    samples, *_ = synthetic(N=6)
    pairs = [(0, 1), (1, 1)]
    whole = eddy.accumulate_reference(samples, pairs)
    cut = eddy.accumulate_reference(samples[2:], pairs, state=eddy.accumulate_reference(samples[:2], pairs))
    assert whole[3] == cut[3] == 6 and all(a.tobytes() == b.tobytes() for a, b in zip(whole[:3], cut[:3]))
    first = eddy.accumulate_reference(samples[:1], pairs)
    assert not first[1].any() and not first[2].any() and np.array_equal(first[0], samples[0])


def test_zonal_reference_is_the_series_row_stage():
    from qingdai_amd import series
    r = np.random.default_rng(11)
    for shape in ((5, 5), (6, 63), (7, 64), (9, 130), (9, 257)):
        S, Cs = r.normal(size=(2,) + shape) * 1e3, r.normal(size=(1,) + shape)
        z = eddy.zonal_reference(S, Cs, [(0, 1)])
        lat = np.linspace(-90, 90, shape[0])
        for t, plane in enumerate((S[0], S[1], Cs[0], S[0] * S[1])):
            zonal = series.reduce_reference(plane, lat)[4]          # S_j / n_lon, the division exact enough to undo: compare sums
            assert np.array_equal(z[0, t] / np.float64(shape[1]), zonal), (shape, t)


# ---------------------------------------------------------------- accuracy: why there is an anchor
def test_anchored_sums_meet_the_bound_the_raw_form_misses():
    """Fields with mean 300 and spread 1e-3, N = 500 samples, four cells.  With d the exact differences a - r, every covariance of
    accumulate_reference lies within gamma_{2N+8} (mean|d_p d_q| + mean|d_p| mean|d_q|) of the exact one, gamma_k = k u / (1 - k u):
    two roundings in the factors, one in the product, N - 1 adds, and the division.  The raw form on the same data does not."""
    N, cells = 500, 4
    rng = np.random.default_rng(2024)
    a = 300.0 + 1e-3 * rng.normal(size=(N, 2, cells))
    pairs = [(0, 1), (0, 0), (1, 1)]
    r, S, Cs, n = eddy.accumulate_reference(list(a), pairs)
    assert n == N
    cov = Cs / np.float64(N) - (S / np.float64(N))[[p for p, _ in pairs]] * (S / np.float64(N))[[q for _, q in pairs]]
    with np.errstate(all="ignore"):
        raw = np.stack([(a[:, p] * a[:, q]).sum(axis=0) / N - (a[:, p].sum(axis=0) / N) * (a[:, q].sum(axis=0) / N) for p, q in pairs])
    u = Fraction(1, 2 ** 53)
    gamma = (2 * N + 8) * u / (1 - (2 * N + 8) * u)
    missed = 0
    for c in range(cells):
        fa = [[Fraction(float(a[t, f, c])) for t in range(N)] for f in range(2)]
        d = [[x - fa[f][0] for x in fa[f]] for f in range(2)]
        for k, (p, q) in enumerate(pairs):
            exact = sum(x * y for x, y in zip(d[p], d[q])) / N - (sum(d[p]) / N) * (sum(d[q]) / N)
            bound = gamma * (sum(abs(x * y) for x, y in zip(d[p], d[q])) / N + (sum(map(abs, d[p])) / N) * (sum(map(abs, d[q])) / N))
            err = abs(Fraction(float(cov[k, c])) - exact)
            print(f"cell {c} pair {k}: anchored error {float(err):.3e}, bound {float(bound):.3e}, raw error "
                  f"{float(abs(Fraction(float(raw[k, c])) - exact)):.3e}, covariance {float(exact):.3e}")
            assert err <= bound, (c, k, float(err), float(bound))
            missed += abs(Fraction(float(raw[k, c])) - exact) > bound
    assert missed == cells * len(pairs)                         # the raw form misses it everywhere
