"""GPU (-m gpu): the latitude-band step path against the whole-globe handle and against the oracle at the band geometries where the
band path makes a form decision of its own (tests/band_form_cases.py): polar bands whose slab is the whole ring, wrap segments that
are too short to stream and ones that stream, n_lon < 64 on bands, own_nrows == halo, a world of 5, one-column last strips and groups
on every segment, halos around the band tail's threshold, a deep halo whose split sub-step has boundary strips of >= 10 rows and the
required halo whose strips are thin (the whole launch redone).  One device, in-process band groups (host copies with the host ring or
collectives, device mailboxes with QD_PEER_OVERLAP 0 / 1 / 2); every grid has at most 97 x 125 cells; 3 steps of 300 s, an ocean step
of 3 sub-steps (step_form_cases.run_cfl).

Which branch ran is not guessed from the geometry: every handle's tallies (Device.step_forms: cnt_* / max_*) are read before it closes,
each row's evidence is asserted on the named band, and test_table_reaches_every_form asserts that every tally is non-zero somewhere.

  family                      reference and bound (relative to the field's max-norm)                         worst measured (MI355X)
  atmosphere span, 3 steps    the whole-globe handle: np.array_equal on U, V, H, TS, Q, CLOUD, HICE (no       0: bit-equal
                              global sum on the path)
                              util.run_oracle_time_step: STEP_TOL = 1e-9                                     6.9e-15  U, deep3_97x70
  ocean step x 3              the whole-globe handle: band_bound = max(1e-12, 1000 x BAND_SENS) (only the     2.4e-14  of 2.7e-12, deep3_97x70;
                              band-wise order of the eta sums differs)                                       <= 3.6e-16 of 1e-12 on the other rows
                              OceanOracle: STEP_TOL                                                          1.7e-12  eta, narrow2_48x63
  coupled loop, 3 steps       the whole-globe handle: band_bound                                             2.1e-15  eta, of 2.7e-12, deep3_97x70
                              DriverOracle: atmosphere / surface STEP_TOL, uo / vo / eta                     1.1e-14  eta, deep3_97x70
                              min(1e-7, max(STEP_TOL, 1000 x BAND_SENS)) = 1e-9 on all three rows
  form against form           bit for bit (the same arithmetic on the same rows, the eta sum formed in the    0: bit-equal
                              same order): QD_PEER_OVERLAP 0 / 1 / 2 (so the redone split against the
                              unsplit launch), QD_STREAM_NO_PAIR, QD_PEER_ONE_LAUNCH, QD_FUSED_FAST=0,
                              QD_PEER_FOLD=0, host copies (collectives) against mailboxes
                              band_bound (the eta sum per row instead of per strip): QD_BAND_TAIL=0, host     2.4e-14  of 2.7e-12, deep3_97x70
                              ring against collective
  non-finite values           the whole-globe handle, one sub-step: np.array_equal with equal_nan; one step   0: bit-equal
                              of 300 s: the same sub-step count and NaN placement

"""
import numpy as np
import pytest

import band_form_cases as bc
import step_form_cases as sc
from util import relerr, surface, run_oracle_time_step

pytestmark = pytest.mark.gpu

STEP_TOL = bc.STEP_TOL
ATM_FIELDS = ("U", "V", "H", "TS", "Q", "CLOUD", "HICE")
OCN_FIELDS = ("UO", "VO", "ETA", "SST")
TALLIES = ("cnt_dyn_stream", "cnt_dyn_tile", "cnt_ocn_stream", "cnt_ocn_tile", "cnt_split", "cnt_split_redo", "cnt_stream_pair",
           "cnt_stream_push", "cnt_sub_band_tail", "cnt_sub_round2", "max_tail_segs", "max_mom_segs", "cnt_tail_fix", "cnt_dyn_tile_fast",
           "cnt_ocn_tile_fast", "cnt_tile_exact", "cnt_tile_shift", "cnt_tile_slab_edge")
COLLECTIVE = ("QD_NO_HOST_RING=1",)

_RUNS = {}          # (cid, kind, transport, switches, halo) -> (fields, [form report per band], n_sub)
_ORACLE = {}


def _params(kind, shape):
    """QdParams as util.run_device_time_step (atm) / WindDrivenSlabOcean (ocean) / driver.Simulation (coupled) leave them"""
    import qingdai_amd as qa
    p = qa.QdParams(energy_w=1.0) if kind == "atm" else qa.QdParams(ocean_cfl=sc.run_cfl(shape))
    if kind != "ocean":
        p.update(g=9.81, H=8000.0, tau_rad=10.0 * 24 * 3600, greenhouse_factor=0.40)
        p.Cs_ocean, p.Cs_land, p.Cs_ice, p.has_csmap = 1000.0 * 4200.0 * 50.0, 3e6, 5e6, 1
    p.H_ocean = 50.0
    return p


def _inputs(cid, kind):
    """({field: array} to upload, the per-step work as fn(dev), the fields to read back)"""
    import qingdai_amd as qa
    shape = bc.CASES[cid]["shape"]
    nlat, nlon = shape
    _, mask, alb, fric = surface(nlat, nlon)
    csmap = np.where(mask == 1, 3e6, 1000.0 * 4200.0 * 50.0).astype(float)
    forcing = qa.ThermalForcing(qa.SphericalGrid(nlat, nlon), qa.OrbitalSystem())
    if kind == "atm":
        up = {"LAND_MASK": mask, "FRICTION": fric, "CSMAP": csmap, "ALBEDO": np.where(mask == 0, 0.08, alb), **bc.atm_state(cid)}
        stars = [forcing.star_scalars(i * bc.DT) for i in range(bc.NSTEPS)]

        def work(dev):
            for a, b, th in stars:
                dev.forcing(a, b, th, True)
                dev.atmos_step(bc.DT, True)
        return up, work, ATM_FIELDS
    if kind in ("ocean", "nan", "nan300"):
        _, s = bc.ocean_state(cid)
        up = {"LAND_MASK": mask, "SST": s["sst"], "UO": s["uo"].copy(), "VO": s["vo"], "ETA": s["eta"].copy(), "U": s["u_atm"], "V": s["v_atm"],
              "QNET": s["qnet"], "ICE_MASK": s["ice"].astype(np.uint8)}
        if kind in ("nan", "nan300"):
            for (i, j), (f, v) in nonfinite_cells(cid).items():
                up[f][i, j] = v
        nsteps, dt = (1, 20.0) if kind == "nan" else (1, bc.DT) if kind == "nan300" else (bc.NSTEPS, bc.DT)

        def work(dev):
            for _ in range(nsteps):
                dev.ocean_step(dt, 0, True, 0)
        return up, work, OCN_FIELDS
    assert kind == "coupled"
    st = sc.coupled_state(shape, mask)
    up = {"LAND_MASK": mask, "FRICTION": fric, "CSMAP": csmap, "BASE_ALBEDO": alb, "SST": np.full(shape, 288.0), "H": st["h"], "TS": st["T_s"],
          "U": st["u"], "V": st["v"], "S_SNOW": st["S_snow"]}
    table = forcing.star_table([i * bc.DT for i in range(bc.NSTEPS)])

    def work(dev):
        dev.step_n(table, bc.DT, with_ocean=True, with_physics=True, pass_albedo=False, with_hydrology=True)
    return up, work, ATM_FIELDS + OCN_FIELDS + ("PRECIP", "ALBEDO", "S_SNOW", "W_LAND")


def nonfinite_cells(cid):
    """One NaN in uo and a huge eta in an owned row next to the halo of the first interior band (or the second band) and of band 0"""
    rr = bc.ranges_of(cid)
    nlon = bc.CASES[cid]["shape"][1]
    r1, n1 = rr[1]
    return {(r1, nlon // 3): ("UO", np.nan), (r1 + n1 - 1, nlon - 1): ("ETA", 1e30),
            (rr[0][1] - 1, 0): ("UO", np.nan), (1, nlon // 2): ("ETA", -1e30)}


def run(monkeypatch, cid, kind, transport=None, switches=(), halo=None):
    """transport None: the whole-globe handle.  The environment is read in qd_create / qd_comm_init_local: set before either."""
    halo = halo if halo is not None else bc.halos_of(cid)[0]
    key = (cid, kind, transport, tuple(switches), halo if transport else None)
    if key in _RUNS:
        return _RUNS[key]
    import qingdai_amd as qa
    from qingdai_amd.bands import BandGroup
    from qingdai_amd.device import Device
    for k in bc.SWITCH_NAMES:
        monkeypatch.delenv(k, raising=False)
    for k, v in {**(bc.TRANSPORTS[transport] if transport else {}), **bc.env_of(switches)}.items():
        monkeypatch.setenv(k, v)
    shape = bc.CASES[cid]["shape"]
    grid = qa.SphericalGrid(*shape)
    up, work, names = _inputs(cid, kind)
    p = _params(kind, shape)
    if transport is None:
        dev = Device(grid, p)
        for k, v in up.items():
            dev.upload_now(k, v)
        work(dev)
        out = {k: dev.get(k).copy() for k in names}
        res = (out, [dev.step_forms()], dev.last_ocean_nsub())
        dev.close()
    else:
        rr = bc.ranges_of(cid)
        grp = BandGroup(grid, len(rr), p, halo=halo, ranges=rr)
        for k, v in up.items():
            grp.set(k, v)
        grp.run(lambda d, r: work(d))
        out = {k: grp.get(k) for k in names}
        res = (out, [d.step_forms() for d in grp.devs], grp.devs[0].last_ocean_nsub())
        grp.close()
    _RUNS[key] = res
    return res


def _tallies(forms):
    return [{k: f[k] for k in TALLIES if f[k]} for f in forms]


def _worst(errs):
    k = max(errs, key=errs.get)
    return f"{errs[k]:.1e} {k}"


# ---------------------------------------------------------------- (a) atmosphere span
@pytest.mark.parametrize("cid", [c for c in bc.IDS if "atm" in bc.CASES[c]["runs"]])
def test_atmosphere_bands_equal_the_globe_bit_for_bit_and_the_oracle(gpu, monkeypatch, cid):
    """No global sum on the atmosphere's path: every transport equals the whole-globe handle bit for bit; the band run itself is held
    to the oracle (the reference is then not only the code under test)."""
    shape = bc.CASES[cid]["shape"]
    ref, _, _ = run(monkeypatch, cid, "atm")
    if cid not in _ORACLE:
        st = bc.atm_state(cid)
        d = {"init_u": st["U"], "init_v": st["V"], "init_h": st["H"], "init_T_s": st["TS"], "init_q": st["Q"], "init_cloud_cover": st["CLOUD"],
             "init_h_ice": st["HICE"]}
        meta = dict(nlat=shape[0], nlon=shape[1], nsteps=bc.NSTEPS, dt=bc.DT, over={"energy_w": 1.0}, with_albedo=True)
        _ORACLE[cid] = run_oracle_time_step(meta, d)
    o = _ORACLE[cid]
    want = {"U": o.u, "V": o.v, "H": o.h, "TS": o.T_s, "Q": o.q, "CLOUD": o.cloud_cover, "HICE": o.h_ice}
    for transport in bc.TRANSPORTS:
        got, forms, _ = run(monkeypatch, cid, "atm", transport)
        errs = {k: relerr(got[k], want[k]) for k in ATM_FIELDS}
        print("atmosphere", cid, transport, "vs oracle", _worst(errs), "ratio", f"{max(errs.values()) / STEP_TOL:.1e}", _tallies(forms))
        for k in ATM_FIELDS:
            assert np.array_equal(got[k], ref[k]), (cid, transport, k, relerr(got[k], ref[k]), np.argwhere(got[k] != ref[k])[:4])
            assert errs[k] < STEP_TOL, (cid, transport, k, errs[k])


# ---------------------------------------------------------------- (b) ocean step and coupled loop
def _ocean_oracle(cid):
    if ("ocean", cid) not in _ORACLE:
        import qd_oracle as qo
        shape = bc.CASES[cid]["shape"]
        mask, s = bc.ocean_state(cid)
        oo = qo.OceanOracle(qo.Grid(*shape), mask, qo.defaults(ocean_cfl=sc.run_cfl(shape)), init_Ts=s["sst"].copy())
        oo.uo, oo.vo, oo.eta = s["uo"].copy(), s["vo"].copy(), s["eta"].copy()
        for _ in range(bc.NSTEPS):
            oo.step(bc.DT, s["u_atm"], s["v_atm"], Q_net=s["qnet"], ice_mask=s["ice"])
        _ORACLE[("ocean", cid)] = ({"UO": oo.uo, "VO": oo.vo, "ETA": oo.eta, "SST": oo.Ts}, oo.last_n_sub)
    return _ORACLE[("ocean", cid)]


OCEAN_CASES = [(c, h) for c in bc.IDS if "ocean" in bc.CASES[c]["runs"] for h in bc.halos_of(c)]


@pytest.mark.parametrize("cid,halo", OCEAN_CASES, ids=[f"{c}-halo{h}" for c, h in OCEAN_CASES])
def test_ocean_step_bands_vs_globe_and_oracle(gpu, monkeypatch, cid, halo):
    """Three full ocean steps of three sub-steps from the fast state (currents at the cap, fast pole rows, an ice mask)"""
    ref, _, nsub = run(monkeypatch, cid, "ocean")
    want, o_nsub = _ocean_oracle(cid)
    assert nsub == o_nsub == 3, (nsub, o_nsub)
    bound = bc.band_bound(cid)
    for transport, sw in [(t, ()) for t in bc.TRANSPORTS] + [("host", COLLECTIVE)]:
        got, forms, b_nsub = run(monkeypatch, cid, "ocean", transport, sw, halo)
        assert b_nsub == nsub
        e_ref = {k: relerr(got[k], ref[k]) for k in OCN_FIELDS}
        e_orc = {k: relerr(got[k], want[k]) for k in OCN_FIELDS}
        print("ocean", cid, halo, transport, sw, "vs globe", _worst(e_ref), "ratio", f"{max(e_ref.values()) / bound:.1e}", "vs oracle", _worst(e_orc),
              "ratio", f"{max(e_orc.values()) / STEP_TOL:.1e}", _tallies(forms))
        for k in OCN_FIELDS:
            assert e_ref[k] < bound, (cid, halo, transport, sw, k, e_ref[k])
            assert e_orc[k] < STEP_TOL, (cid, halo, transport, sw, k, e_orc[k])


@pytest.mark.parametrize("cid", bc.COUPLED_IDS)
def test_coupled_loop_bands_vs_globe_and_driver_oracle(gpu, monkeypatch, cid):
    """driver.Simulation's span (atmosphere, driver physics, hydrology, ocean with Q_net and the ice mask from the device) on bands"""
    shape = bc.CASES[cid]["shape"]
    ref, _, nsub = run(monkeypatch, cid, "coupled")
    if ("coupled", cid) not in _ORACLE:
        _, mask, alb, fric = surface(*shape)
        _ORACLE[("coupled", cid)] = bc.coupled_oracle(cid, mask, alb, fric)
    m, oc, d = _ORACLE[("coupled", cid)]
    want = {"U": m.u, "V": m.v, "H": m.h, "TS": m.T_s, "Q": m.q, "CLOUD": m.cloud_cover, "HICE": m.h_ice, "UO": oc.uo, "VO": oc.vo, "ETA": oc.eta,
            "SST": oc.Ts, "PRECIP": d.precip, "ALBEDO": d.albedo, "S_SNOW": d.S_snow, "W_LAND": d.W_land}
    assert nsub == oc.last_n_sub and nsub >= 3, (nsub, oc.last_n_sub)          # (the state's own winds set the count: 12 at run_cfl)
    assert (d.S_snow > 0).sum() > 0
    bound, obound = bc.band_bound(cid), bc.oracle_bound(cid)
    for transport, sw in [(None, ())] + [(t, ()) for t in bc.TRANSPORTS] + [("host", COLLECTIVE)]:
        got, forms, _ = run(monkeypatch, cid, "coupled", transport, sw)
        e_orc = {k: relerr(got[k], want[k]) / (obound if k in ("UO", "VO", "ETA") else STEP_TOL) for k in want}
        e_ref = {k: relerr(got[k], ref[k]) / bound for k in want}
        print("coupled", cid, transport, sw, "vs globe ratio", _worst(e_ref), "vs oracle ratio", _worst(e_orc), _tallies(forms))
        for k in want:
            assert e_orc[k] < 1.0, (cid, transport, sw, k, "vs oracle", e_orc[k])
            assert e_ref[k] < 1.0, (cid, transport, sw, k, "vs globe", e_ref[k])


# ---------------------------------------------------------------- (c) form against form on the same band group
def _bit_equal(a, b, what):
    for k in a:
        assert np.array_equal(a[k], b[k], equal_nan=True), (what, k, relerr(np.nan_to_num(a[k]), np.nan_to_num(b[k])))


def _within(a, b, bound, what):
    errs = {k: relerr(a[k], b[k]) for k in a}
    for k, e in errs.items():
        assert e < bound, (what, k, e)
    return max(errs.values())


@pytest.mark.parametrize("cid", bc.IDS)
def test_band_forms_agree(gpu, monkeypatch, cid):
    """On the row's ocean run (and its coupled run where it has one).
    Bit for bit: QD_PEER_OVERLAP 0 / 1 / 2 -- the rows of a launch do not depend on the piece they are computed in, the eta sum is the
    tail's, which the split does not touch; with the required halo overlap 1 / 2 split every sub-step and redo the launch as a whole
    (thin strips), so this is also the redo branch against the unsplit launch.  QD_STREAM_NO_PAIR (two launches instead of one),
    QD_PEER_ONE_LAUNCH (where the exchange's kernels are cut), QD_FUSED_FAST=0 (tile EXACT path: the same arithmetic in the same order;
    asserted to cross tile launches that HAD FAST tiles) and QD_FUSED_FAST=3 (the tile FAST path on bands that stream by default).
    Also bit for bit, because the eta sum is formed in the same order: QD_PEER_FOLD=0 (the band's share reduced by a launch of its own
    instead of the tail's finishing wave: both add the ranks' slots in rank order, qd_peer.hip OP 0 / qd_peer_dev.h) and host copies
    without the host ring against the mailboxes (qd_allreduce_f64's in-process form adds stage[0], stage[1], ... -- rank order too --
    and both run the same band-tail kernels).
    Band bound: QD_BAND_TAIL=0 (the round-2 kernels sum eta per row, the tail per strip) and host ring against collective (the ring
    takes the round-2 kernels with the mean deferred and reduced on the host)."""
    c = bc.CASES[cid]
    halo = bc.halos_of(cid)[-1]
    note = {}
    for kind in [k for k in ("ocean", "coupled") if k in c["runs"]]:
        bound = bc.band_bound(cid)
        peer = {t: run(monkeypatch, cid, kind, t, (), halo)[0] for t in ("peer0", "peer1", "peer2")}
        _bit_equal(peer["peer1"], peer["peer0"], (cid, kind, "QD_PEER_OVERLAP=1"))
        _bit_equal(peer["peer2"], peer["peer0"], (cid, kind, "QD_PEER_OVERLAP=2"))
        host = run(monkeypatch, cid, kind, "host", (), halo)[0]
        coll = run(monkeypatch, cid, kind, "host", COLLECTIVE, halo)[0]
        note[kind, "ring/collective"] = _within(host, coll, bound, (cid, kind, "host ring against collective"))
        _bit_equal(coll, peer["peer0"], (cid, kind, "host copies against mailboxes"))
        for sw in c["switches"]:
            if sw in ("QD_STREAM_NO_PAIR=1", "QD_PEER_ONE_LAUNCH=0"):
                got, forms, _ = run(monkeypatch, cid, kind, "peer2", (sw,), halo)
                _bit_equal(got, peer["peer2"], (cid, kind, sw))
                if sw == "QD_STREAM_NO_PAIR=1":                            # the switch took the pair launch away, not the split
                    assert any(f["cnt_split"] > 0 for f in forms) and all(f["cnt_stream_pair"] == 0 for f in forms), _tallies(forms)
            elif sw in ("QD_FUSED_FAST=0", "QD_FUSED_FAST=3"):
                got, forms, _ = run(monkeypatch, cid, kind, "peer2", (sw,), halo)
                _bit_equal(got, peer["peer2"], (cid, kind, sw, "peer2"))
                _bit_equal(run(monkeypatch, cid, kind, "host", (sw,), halo)[0], host, (cid, kind, sw, "host"))
                base = run(monkeypatch, cid, kind, "peer2", (), halo)[1]
                if sw == "QD_FUSED_FAST=0":                                # FAST tiles against EXACT tiles, not EXACT against EXACT
                    assert any(f["cnt_ocn_tile_fast"] > 0 for f in base), _tallies(base)
                    assert all(f["cnt_ocn_tile_fast"] == 0 and f["cnt_dyn_tile_fast"] == 0 and f["cnt_ocn_stream"] == 0 for f in forms), _tallies(forms)
                    assert any(f["cnt_tile_exact"] > 0 for f in forms)
                else:                                                      # the tile FAST path on the bands that stream by default
                    assert all(f["cnt_ocn_stream"] == 0 for f in forms) and any(f["cnt_ocn_tile_fast"] > b["cnt_ocn_tile_fast"]
                                                                                for f, b in zip(forms, base)), _tallies(forms)
            elif sw == "QD_PEER_FOLD=0":
                _bit_equal(run(monkeypatch, cid, kind, "peer2", (sw,), halo)[0], peer["peer2"], (cid, kind, sw))
            elif sw == "QD_BAND_TAIL=0":
                note[kind, sw] = _within(run(monkeypatch, cid, kind, "peer2", (sw,), halo)[0], peer["peer2"], bound, (cid, kind, sw, "peer2"))
                note[kind, sw + " collective"] = _within(run(monkeypatch, cid, kind, "host", COLLECTIVE + (sw,), halo)[0], coll, bound,
                                                         (cid, kind, sw, "collective"))
            else:
                assert sw == "QD_NO_HOST_RING=1", sw                       # crossed above
    print("band forms", cid, "bound", f"{bc.band_bound(cid):.1e}", {k: f"{v:.1e}" for k, v in note.items()})


# ---------------------------------------------------------------- (d) which branch ran
def _all_reports(monkeypatch):
    """Every (row, run, transport, switch) of the tests above with the report of every band: cached runs, nothing is launched twice"""
    seen = []
    for cid in bc.IDS:
        c = bc.CASES[cid]
        for kind in c["runs"]:
            for halo in bc.halos_of(cid):
                combos = [(t, ()) for t in bc.TRANSPORTS]
                if kind != "atm":
                    combos += [("host", COLLECTIVE)]
                for transport, sw in combos:
                    seen.append((cid, kind, transport, sw, halo, run(monkeypatch, cid, kind, transport, sw, halo)[1]))
    return seen


def test_table_reaches_every_form(gpu, monkeypatch):
    """Every tally of qd_step_forms is non-zero on some band of some row; if a launcher threshold moves, this fails instead of the
    table silently losing a branch."""
    seen = _all_reports(monkeypatch)
    for t in TALLIES:
        where = [(cid, kind, tr, sw, halo, b) for cid, kind, tr, sw, halo, forms in seen for b, f in enumerate(forms) if f[t] > 0]
        print(t, len(where), where[:3])
        assert where, t
    def any_band(pred):
        return any(pred(f) for *_, forms in seen for f in forms)
    assert any_band(lambda f: f["max_tail_segs"] == 1) and any_band(lambda f: f["max_tail_segs"] == 2)
    assert any_band(lambda f: f["max_mom_segs"] == 1) and any_band(lambda f: f["max_mom_segs"] == 2)
    # one handle took both momentum forms (the margin shrinks from launch to launch)
    assert any_band(lambda f: f["cnt_ocn_stream"] > 0 and f["cnt_ocn_tile"] > 0)
    assert any_band(lambda f: f["cnt_split"] > 0 and f["cnt_split_redo"] == 0) and any_band(lambda f: f["cnt_split_redo"] > 0)


def _holds(value, op, want):
    return {"==": value == want, ">": value > want}[op]


@pytest.mark.parametrize("cid", bc.IDS)
def test_row_reaches_its_branch(gpu, monkeypatch, cid):
    """The row's evidence on the named band: {(run, transport[, halo or None[, switches]]): {band: {tally: (op, value)}}}.  A row that
    does not reach its branch is a wrong row."""
    ev = bc.CASES[cid].get("evidence", {})
    halo = bc.halos_of(cid)
    for (kind, transport, *rest), bands in ev.items():
        h = rest[0] if rest and rest[0] is not None else halo[0]
        sw = (COLLECTIVE if transport == "collective" else ()) + (tuple(rest[1]) if len(rest) > 1 else ())
        forms = run(monkeypatch, cid, kind, "host" if transport == "collective" else transport, sw, h)[1]
        for band, want in bands.items():
            bad = {k: (forms[band][k], op, v) for k, (op, v) in want.items() if not _holds(forms[band][k], op, v)}
            assert not bad, (cid, kind, transport, h, "band", band, "got, want:", bad)
    assert ev, cid


# ---------------------------------------------------------------- (e) non-finite values on a band
@pytest.mark.parametrize("cid", ["interior3_61x117", "polar2_48x65"])
def test_nonfinite_values_on_a_band(gpu, monkeypatch, cid):
    """A NaN in uo and an eta of +-1e30 in owned rows next to the halo of a polar band and of the next band.  The EXACT re-run of a FAST
    tile or wave and the outlier / fix cells must be the same whichever segment (own rows or a neighbour's halo) computed them.
    One ocean step of 20 s, which is ONE sub-step: the band-wise order of the eta sum then reaches eta alone, once, at the end of the
    step (with more sub-steps it enters the next momentum launch, and bit-equality with the whole globe is not implied), so bands
    must equal the whole globe bit for bit, NaN placement included.  The interior band under the mailboxes must have taken the fix list.
    One step of 300 s besides: the poisoned cells must not change the sub-step count a band computes (NaN never wins the CFL
    maxima, on a band's segments as on the globe) nor where the NaNs end up."""
    ref, _, nsub = run(monkeypatch, cid, "nan")
    assert nsub == 1
    print("non-finite", cid, "whole globe: NaN cells", {k: int(np.isnan(ref[k]).sum()) for k in OCN_FIELDS})
    ref300, _, nsub300 = run(monkeypatch, cid, "nan300")
    print("non-finite", cid, "300 s: sub-steps", nsub300)
    for transport, sw in [(t, ()) for t in bc.TRANSPORTS] + [("host", COLLECTIVE)]:
        got, forms, b_nsub = run(monkeypatch, cid, "nan", transport, sw)
        assert b_nsub == 1, (cid, transport, sw, b_nsub)
        diff = {k: (int(np.sum(~((got[k] == ref[k]) | (np.isnan(got[k]) & np.isnan(ref[k]))))), relerr(np.nan_to_num(got[k]), np.nan_to_num(ref[k])))
                for k in OCN_FIELDS}
        print("non-finite", cid, transport, sw, "cells that differ, rel. error:", diff, _tallies(forms))
        for k in OCN_FIELDS:
            assert np.array_equal(got[k], ref[k], equal_nan=True), (cid, transport, sw, k, diff[k])
        if cid == "interior3_61x117" and transport.startswith("peer"):
            assert forms[1]["cnt_tail_fix"] == 1 and forms[1]["max_tail_segs"] == 1, _tallies(forms)
        got300, _, b_nsub300 = run(monkeypatch, cid, "nan300", transport, sw)
        assert b_nsub300 == nsub300, (cid, transport, sw, b_nsub300, nsub300)
        for k in OCN_FIELDS:
            assert np.array_equal(np.isnan(got300[k]), np.isnan(ref300[k])), (cid, transport, sw, k, "300 s")
