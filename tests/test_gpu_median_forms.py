"""GPU (-m gpu): every form of the exact median of positives (qingdai_amd/csrc/qd_reduce.hip) at the edges of tests/median_cases.py.

Each call of a case is compared with np.median(t(x)[t(x) > 0]) in float64 BIT FOR BIT (no tolerance: the contract is equality),
and the device's form report (Device.median_state: centre, valid, hits, misses, list length, count, bracket patterns; bands: the
all-reduce count and with it the miss flag) with the table's prediction -- a case named for the LDS list must have been served from
it.  Whole-globe cases repeat their fields on a handle with QD_MEDIAN_PREDICT=0; pair cases repeat theirs as single calls on a
fresh handle.  One fresh handle (or band group) per case: a handle carries predictor state, the order of calls is part of a case.

+inf as the upper middle rank (values/inf_upper_middle, bands*/inf_rank, the pair chain's miss jobs): qd_med_final_body started
its search for the upper middle at DBL_MAX, which +inf can never undercut; the windowed call returned (v1 + DBL_MAX) / 2 where
numpy, the first call and QD_MEDIAN_PREDICT=0 return inf.  It starts at +inf now.
"""
import numpy as np
import pytest

import median_cases as mc

pytestmark = pytest.mark.gpu

SWITCHES = ("QD_MEDIAN_PREDICT", "QD_MED_BLOCKS", "QD_PEER_EXCHANGE", "QD_PEER_HOOKS", "QD_MED_PAIR", "QD_MED_SIDE", "QD_MEDIAN_DEBUG")
WHOLE = sorted(cid for cid, C in mc.CASES.items() if not C["world"])
BANDS = sorted((cid, t) for cid, C in mc.CASES.items() if C["world"] for t in C["transports"])
REPORT_KEYS = ("valid", "hits", "misses", "list_len", "count", "lo_bits", "hi_bits", "calls")


def _switches(monkeypatch, env, transport=None):
    for k in SWITCHES:
        monkeypatch.delenv(k, raising=False)
    for k, v in env.items():
        monkeypatch.setenv(k, v)
    if transport in ("peer", "peer_nohooks"):
        monkeypatch.setenv("QD_PEER_EXCHANGE", "1")
    if transport == "peer_nohooks":
        monkeypatch.setenv("QD_PEER_HOOKS", "0")


def _handle(shape):
    import qingdai_amd as qa
    from qingdai_amd.device import Device
    return Device(qa.SphericalGrid(*shape), qa.QdParams())


def _check_report(where, got, want):
    assert not want["valid"] or mc.same(got["centre"], want["centre"]), (where, got, want)      # (a dropped centre is not read)
    for k in REPORT_KEYS:
        assert got[k] == want[k], (where, k, got, want)


def _check_value(where, got, j):
    want = mc.expected(j["x"], j["dflt"], j["transform"], j["tparam"])
    print(where, "device", repr(got), "numpy", repr(want))
    assert mc.same(got, want), (where, got, want)


def _jobs(c):
    return [c] if c["op"] == "single" else list(c["jobs"])


def _run_whole(dev, calls, preds, cid, as_singles=False):
    """the calls of a case on one whole-globe handle -> [[value, ...]] per call, checked against numpy and the prediction"""
    out = []
    for k, (c, ps) in enumerate(zip(calls, preds)):
        if c["op"] == "single" or as_singles:
            got = [dev.op_median_at(j["x"], j["dflt"], j["transform"], j["tparam"], j["site"]) for j in _jobs(c)]
        else:
            a, b = c["jobs"]
            got = list(dev.op_median_pair(a["x"], a["dflt"], a["transform"], a["tparam"], a["site"],
                                          b["x"], b["dflt"], b["transform"], b["tparam"], b["site"]))
        state = dev.median_state()
        for j, g, P in zip(_jobs(c), got, ps):
            _check_value((cid, k, P["form"]), g, j)
            if P["report"] is not None:
                _check_report((cid, k, P["form"], j["site"]), state[j["site"]], P["report"])
        out.append(got)
    return out


@pytest.mark.parametrize("cid", WHOLE)
def test_whole_globe_case(gpu, monkeypatch, cid):
    C = mc.CASES[cid]
    calls, preds = mc.predict_case(C)
    _switches(monkeypatch, C["env"])
    dev = _handle(C["shape"])
    try:
        got = _run_whole(dev, calls, preds, cid)
        state = dev.median_state()
    finally:
        dev.close()
    if any(c["op"] == "pair" for c in calls):
        # every job of a pair equals the same call made singly, and leaves its site as the single call does: nothing leaks between
        # the two buffer sets
        dev = _handle(C["shape"])
        try:
            singly = _run_whole(dev, calls, preds, cid + " singly", as_singles=True)
            again = dev.median_state()
        finally:
            dev.close()
        assert all(mc.same(a, b) for x, y in zip(got, singly) for a, b in zip(x, y)), (cid, got, singly)
        for s in range(mc.SITES):
            _check_report((cid, "pair against singles", s), state[s], again[s])
    if C["three_way"]:
        # the digit-by-digit select on the same fields (QD_MEDIAN_PREDICT=0) agrees with the first call and the windowed call
        monkeypatch.setenv("QD_MEDIAN_PREDICT", "0")
        dev = _handle(C["shape"])
        try:
            for k, c in enumerate(calls):
                for j, g in zip(_jobs(c), got[k]):
                    off = dev.op_median_at(j["x"], j["dflt"], j["transform"], j["tparam"], j["site"])
                    assert mc.same(off, g), (cid, k, "QD_MEDIAN_PREDICT=0", off, g)
            assert all(s["calls"] == 0 and not s["valid"] for s in dev.median_state())
        finally:
            dev.close()


@pytest.mark.parametrize("cid,transport", BANDS)
def test_band_case(gpu, monkeypatch, cid, transport):
    import qingdai_amd as qa
    from qingdai_amd.bands import BandGroup
    C = mc.CASES[cid]
    calls, preds = mc.predict_case(C)
    _switches(monkeypatch, C["env"], transport)
    world = C["world"]
    grp = BandGroup(qa.SphericalGrid(*C["shape"]), world, qa.QdParams(), halo=mc.BAND_HALO)
    try:
        for k, (c, (P,)) in enumerate(zip(calls, preds)):
            before = grp.allreduces()
            got = [None] * world

            def work(dev, rank, c=c, got=got):
                got[rank] = dev.op_median_at(c["x"], c["dflt"], c["transform"], c["tparam"], c["site"])
            grp.run(work)
            for rank in range(world):                               # every band returns numpy's bits on the whole field
                _check_value((cid, transport, k, P["form"], rank), got[rank], c)
            delta = [int(a - b) for a, b in zip(grp.allreduces(), before)]
            assert delta == [P["allreduces"]] * world, (cid, transport, k, P["form"], delta, P["allreduces"])      # 2, 2 + 6 on a miss
            if P["report"] is not None:
                for rank, dev in enumerate(grp.devs):
                    _check_report((cid, transport, k, P["form"], rank), dev.median_state()[c["site"]], P["report"])
    finally:
        grp.close()


def test_seam_refusals(gpu, monkeypatch):
    """the refusals of the two entry points return before any launch, with a message; qd_op_median_positive is site 0, transform 0"""
    import qingdai_amd as qa
    from qingdai_amd import _lib
    from qingdai_amd.bands import BandGroup
    _switches(monkeypatch, {})
    shape = (7, 65)
    x = mc.field(shape, 1, mc.spread(1, 300, 2.0))
    dev = _handle(shape)
    try:
        a = (x, 1e-6, 0, 0.0, 2)
        b = (x * 3.0, 1e-6, 0, 0.0, 3)
        with pytest.raises(_lib.QdError, match="not ready"):
            dev.op_median_pair(*a, *b)                             # no window yet: must not fall back to two single calls
        assert all(s["calls"] == 0 and not s["valid"] for s in dev.median_state())
        with pytest.raises(_lib.QdError, match="different sites"):
            dev.op_median_pair(*a, *a)
        for bad in (-2, 4):
            with pytest.raises(_lib.QdError, match="site"):
                dev.op_median_at(x, 1e-6, 0, 0.0, bad)
        with pytest.raises(_lib.QdError, match="sites"):
            dev.op_median_pair(x, 1e-6, 0, 0.0, -1, *b)
        with pytest.raises(_lib.QdError, match="transform"):
            dev.op_median_at(x, 1e-6, 2, 0.0, 0)
        want = mc.expected(x, 1e-6)
        assert dev.op_median_positive(x, 1e-6) == want and dev.op_median_positive(x * 1.01, 1e-6) == mc.expected(x * 1.01, 1e-6)
        s0 = dev.median_state()[0]
        assert s0["hits"] == 1 and s0["calls"] == 1 and s0["valid"] and s0["centre"] == mc.expected(x * 1.01, 1e-6)
    finally:
        dev.close()
    monkeypatch.setenv("QD_MEDIAN_PREDICT", "0")
    dev = _handle(shape)
    try:
        assert dev.op_median_at(x, 1e-6, 0, 0.0, 2) == want and dev.op_median_at(x, 1e-6, 0, 0.0, 3) == want
        with pytest.raises(_lib.QdError, match="not ready"):
            dev.op_median_pair(*a, *b)
    finally:
        dev.close()
    monkeypatch.delenv("QD_MEDIAN_PREDICT")
    grp = BandGroup(qa.SphericalGrid(*mc.BSHAPE), 2, qa.QdParams(), halo=mc.BAND_HALO)
    try:
        y = mc.field(mc.BSHAPE, 2, mc.spread(2, 300, 2.0))
        with pytest.raises(_lib.QdError, match="whole-globe"):
            grp.devs[0].op_median_pair(y, 1e-6, 0, 0.0, 2, y, 1e-6, 0, 0.0, 3)
    finally:
        grp.close()
