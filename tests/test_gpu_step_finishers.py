"""The one-workgroup finishers that moved into their consumers (qd_physics.hip, qd_stencil.hip).

On a whole-globe handle the precipitation k_gauss_pair reduces the row partials of k_precip_raw in every workgroup (no
k_precip_scalars launch), k_precip_raw reads the divergence slab k_divvort stored for the median instead of forming the divergence
again, and pos = max(0, -(div - D_crit)) is never stored: the blur of the fallback blend forms it from the same slab on load.  The
same operations on the same operands in the same order, so every field and both scalars must equal the unfolded launches
(QD_MERGE_POINTWISE=0: k_precip_raw<false>, k_precip_scalars, k_gauss_rows x 2, k_precip_blend) bit for bit.
"""
import numpy as np
import pytest

from test_gpu_bands import _seed_state, _setup

pytestmark = pytest.mark.gpu

FIELDS = ("PRECIP", "CLOUD", "CLOUD_FROM_P", "ALBEDO", "U", "H", "Q", "TS")
SCALARS = ("RENORM", "BLEND_W", "PSCALE")

# what the state has to exercise: the usual step (fallback blend off: pass B of the blur does not run), no cell with positive
# convergence (anypos false: the median writes its default, F_div is 0), and the fallback blend on (<Pq> < pq_min: pass B reads the
# divergence slab and forms pos on load)
CASES = {
    "usual": dict(),
    "no_positive_convergence": dict(D_crit=-1e30),            # (the pole rows' 1 / cos factor makes |div| of order 1 there)
    "fallback_blend": dict(p_hybrid_fallback=1, pq_min=1e3),
}


def _run(monkeypatch, gpu, nlat, nlon, over, merged, nsteps=3):
    from qingdai_amd.device import Device
    monkeypatch.setenv("QD_MERGE_POINTWISE", "1" if merged else "0")
    qa, grid, mask, alb, fric, p = _setup(nlat, nlon, dict(energy_w=1.0, **over))
    forcing = qa.ThermalForcing(qa.SphericalGrid(nlat, nlon), qa.OrbitalSystem())
    dev = Device(grid, p)
    st = _seed_state(nlat, nlon, 11)
    # a state that condenses (P_cond > 0, so <Pq> >= pq_min and the fallback blend is off unless the case asks for it): h is the
    # anomaly the air temperature 288 + g / c_p h is taken from, and q is above saturation at 288 K
    st["H"] = st["H"] - 8000.0
    st["Q"] = 3.0 * st["Q"]
    for k, v in {"LAND_MASK": mask, "FRICTION": fric, "BASE_ALBEDO": alb, **st}.items():
        dev.upload_now(k, v)
    # one step at a time as well as a span: the hoisted precipitation block of the next step runs inside the span only
    dev.step_n(forcing.star_table([0.0]), 300.0, with_ocean=True, with_physics=True, pass_albedo=True)
    dev.step_n(forcing.star_table([300.0 * (1 + i) for i in range(nsteps - 1)]), 300.0, with_ocean=True, with_physics=True, pass_albedo=True)
    out = {k: np.array(dev.get(k)) for k in FIELDS}
    sc = dev.step_scalars()
    dev.close()
    return out, sc


@pytest.mark.parametrize("case", sorted(CASES))
@pytest.mark.parametrize("shape", [(19, 36), (91, 130)])
def test_folded_precipitation_finishers_equal_the_unfolded_launches(gpu, monkeypatch, shape, case):
    nlat, nlon = shape
    ref, ref_sc = _run(monkeypatch, gpu, nlat, nlon, CASES[case], merged=False)
    got, got_sc = _run(monkeypatch, gpu, nlat, nlon, CASES[case], merged=True)
    for k in SCALARS:
        print(case, shape, k, got_sc[k], ref_sc[k])
    # the case is what its name says (on the reference run, which does not contain the code under test)
    if case == "fallback_blend":
        assert ref_sc["BLEND_W"] == 0.6
    else:
        assert ref_sc["BLEND_W"] == 0.0 and ref_sc["RENORM"] > 0.0
    if case == "no_positive_convergence":
        assert ref_sc["PSCALE"] == 1e-12                      # the median's default: no positive entry
    else:
        assert ref_sc["PSCALE"] > 1e-12
    assert np.isfinite(ref["PRECIP"]).all() and ref["PRECIP"].max() > 0.0
    for k in SCALARS:
        assert got_sc[k] == ref_sc[k], (k, got_sc[k], ref_sc[k])
    for k in FIELDS:
        assert np.array_equal(got[k], ref[k], equal_nan=True), k


# ------------------------------------------------------------------ the eta mean of an ocean sub-step, finished by the next launch
# (qd_wave.h: qd_acc_add / qd_acc_read; qd_stream.h: qs_mean_handover).  QD_MEAN_IN_MOMENTUM=0 is the same code with every tail launch
# finishing its own mean behind tickets: same adds, same reduction, so the ocean must not differ by a bit.
OCEAN = ("UO", "VO", "ETA", "SST", "TS")


def _ocean_run(monkeypatch, nlat, nlon, cfl, on, spans=(4,), poison=False, fix_list=False):
    from qingdai_amd.device import Device
    monkeypatch.setenv("QD_MEAN_IN_MOMENTUM", "1" if on else "0")
    # the reference runs the storing form of the tail kernel in every step, like the new path (fix_list: the handle's own threshold,
    # i.e. the fix-list form while its lists are short, which keeps its finishing wave)
    if fix_list:
        monkeypatch.delenv("QD_TAIL_FIX_DENSE", raising=False)
    else:
        monkeypatch.setenv("QD_TAIL_FIX_DENSE", "-1")
    qa, grid, mask, alb, fric, p = _setup(nlat, nlon, dict(energy_w=1.0, ocean_cfl=cfl))
    forcing = qa.ThermalForcing(qa.SphericalGrid(nlat, nlon), qa.OrbitalSystem())
    dev = Device(grid, p)
    st = _seed_state(nlat, nlon, 7)
    r = np.random.default_rng(17)
    lat = np.linspace(-np.pi / 2, np.pi / 2, nlat)[:, None]
    st["UO"] = np.where(mask == 0, 0.3 * np.cos(lat) + 0.05 * r.normal(size=(nlat, nlon)), 0.0)
    st["VO"] = np.where(mask == 0, 0.05 * r.normal(size=(nlat, nlon)), 0.0)
    st["ETA"] = np.where(mask == 0, 0.2 * r.normal(size=(nlat, nlon)), 0.0)
    if poison:                                                # a partial sum that is not representable: the flagged fallback
        oc = np.argwhere(mask == 0)
        a, b = oc[len(oc) // 3], oc[2 * len(oc) // 3]
        st["ETA"][a[0], a[1]] = np.nan
        st["ETA"][b[0], b[1]] = 1e300
    for k, v in {"LAND_MASK": mask, "FRICTION": fric, "BASE_ALBEDO": alb, **st}.items():
        dev.upload_now(k, v)
    t, nsub = 0.0, []
    for n in spans:
        dev.step_n(forcing.star_table([t + 300.0 * i for i in range(n)]), 300.0, with_ocean=True, with_physics=True, pass_albedo=True)
        t += 300.0 * n
        nsub.append(dev.last_ocean_nsub())
    out = {k: np.array(dev.get(k)) for k in OCEAN}
    left = dev.ocean_mean_next_count()
    dev.close()
    return out, nsub, left


# one column strip of the tail kernel with the longitude wrap inside one wave; ragged strips; more tail workgroups than slots
@pytest.mark.parametrize("shape,cfl", [((46, 72), 0.05), ((46, 72), 0.04), ((91, 130), 0.05), ((181, 360), 0.05), ((181, 360), 0.04)])
def test_eta_mean_finished_by_the_next_momentum_launch_changes_nothing(gpu, monkeypatch, shape, cfl):
    nlat, nlon = shape
    ref, ref_nsub, ref_left = _ocean_run(monkeypatch, nlat, nlon, cfl, on=False)
    got, nsub, left = _ocean_run(monkeypatch, nlat, nlon, cfl, on=True)
    print(shape, cfl, "n_sub", nsub, "left to the next launch", left)
    assert nsub == ref_nsub and nsub[-1] >= 3
    assert ref_left == 0 and left >= (nsub[-1] - 1)           # the new path really ran (every sub-step but the last of a step)
    for k in OCEAN:
        assert np.array_equal(got[k], ref[k], equal_nan=True), k


def test_eta_mean_by_the_next_launch_with_nan_and_huge_eta(gpu, monkeypatch):
    """A NaN and a 1e300 in eta: their strips raise the slot flag, and the reader adds the stored partials in the finisher's order."""
    ref, _, _ = _ocean_run(monkeypatch, 91, 130, 0.05, on=False, poison=True, spans=(2,))
    got, nsub, left = _ocean_run(monkeypatch, 91, 130, 0.05, on=True, poison=True, spans=(2,))
    assert left > 0
    for k in OCEAN:
        assert np.array_equal(got[k], ref[k], equal_nan=True), k


def test_two_spans_leave_the_slot_sets_clean(gpu, monkeypatch):
    ref, _, _ = _ocean_run(monkeypatch, 91, 130, 0.05, on=False, spans=(2, 2))
    got, nsub, left = _ocean_run(monkeypatch, 91, 130, 0.05, on=True, spans=(2, 2))
    assert left > 0
    for k in OCEAN:
        assert np.array_equal(got[k], ref[k], equal_nan=True), k


def test_the_fix_list_form_of_the_old_path_equals_the_new_default(gpu, monkeypatch):
    """A step that leaves its means to the next launch no longer takes the fix-list form; with the switch off the handle does, from
    rest, as before: same ocean, bit for bit."""
    ref, _, ref_left = _ocean_run(monkeypatch, 91, 130, 0.05, on=False, fix_list=True)
    got, nsub, left = _ocean_run(monkeypatch, 91, 130, 0.05, on=True, fix_list=True)
    assert ref_left == 0 and left > 0
    for k in OCEAN:
        assert np.array_equal(got[k], ref[k], equal_nan=True), k
