"""CPU: the table of tests/step_form_cases.py and its fixtures (tests/golden/ts_*_forms.npz, ocean_*_forms.npz).  The fixtures exist and
are small, the ocean ones really have 2-6 sub-steps, the oracle is not chaotic over the steps the GPU tests compare (so a GPU failure
there cannot be blamed on amplified rounding), and the recorded coupled-loop sensitivities reproduce."""
import glob
import os

import numpy as np
import pytest

import step_form_cases as sc
from util import GOLD, STATE, DIAG, load_golden, relerr, run_oracle_time_step

CHAOS_TOL = 1e-11          # 100 x below STEP_TOL


def _names(shape):
    return f"ts_{shape[0]}x{shape[1]}_forms", f"ocean_{shape[0]}x{shape[1]}_forms"


def test_every_fixture_shape_has_its_files_and_they_are_small():
    new = [os.path.join(GOLD, n + ".npz") for s in sc.FIXTURE_SHAPES for n in _names(s)]
    for p in new:
        assert os.path.exists(p), p
    old = [p for p in glob.glob(os.path.join(GOLD, "*")) if p not in new]
    assert max(os.path.getsize(p) for p in new) < max(os.path.getsize(p) for p in old)
    assert sorted(glob.glob(os.path.join(GOLD, "*_forms.npz"))) == sorted(new)          # and no fixture the table does not know


@pytest.mark.parametrize("shape", sc.FIXTURE_SHAPES)
def test_fixture_is_the_table_row(shape):
    """The fixture's inputs are the case module's restated states (what the GPU tests feed the shapes without a fixture), its ocean
    run has 2-6 sub-steps a step, and the table's column widths are the shape's."""
    seed, cfl = sc.CASES[shape]["fixture"]
    ts, ocn = _names(shape)
    meta, d = load_golden(ts)
    assert (meta["nlat"], meta["nlon"], meta["nsteps"], meta["over"], meta["with_albedo"], meta["seed"]) == (*shape, sc.ATM_NSTEPS, {"energy_w": 1.0}, True, seed)
    m2, d2 = sc.ts_case(shape)
    for k in STATE:
        assert np.array_equal(d["init_" + k], d2["init_" + k]), k
    meta, d = load_golden(ocn)
    assert meta["over"] == {"ocean_cfl": cfl} == {"ocean_cfl": sc.CASES[shape]["cfl"]} and meta["nsteps"] == 3
    assert all(2 <= n <= 6 for n in meta["n_sub"]), meta["n_sub"]
    _, o2 = sc.ocean_case(shape)
    for k in ("u_atm", "v_atm", "Q_net", "init_uo", "init_vo", "init_eta", "init_Ts"):
        assert np.array_equal(d[k], o2[k]), k
    assert np.array_equal(d["ice_mask"].astype(bool), o2["ice_mask"])


def test_table_columns():
    for shape, row in sc.CASES.items():
        w58, w60, w62 = sc.last_widths(shape[1])
        assert row["last_strip"] == w58 and row["last_group"] == (w60 if shape[1] >= 64 else None), shape
        assert set(row["switches"]) <= set(sc.SWITCH_FORMS)
    widths = {sc.last_widths(s[1]) for s in sc.SHAPES}
    assert {w[0] for w in widths} >= {1, 3} and {w[1] for w in widths} >= {1} and (1, 5, 1)[2] in {w[2] for w in widths}
    assert {s[1] for s in sc.SHAPES} >= {63, 64, 65} and {s[0] for s in sc.SHAPES} >= {11, 12, 13, 37, 38}
    assert set(sc.COUPLED_SHAPES) <= set(sc.SHAPES) and set(sc.MODE_SHAPES) <= set(sc.SHAPES)


@pytest.mark.parametrize("shape", sc.SHAPES)
def test_oracle_is_not_chaotic_over_the_compared_steps(shape):
    """Inputs perturbed by 1e-15 (relative): every compared field of the atmosphere step and of the three ocean steps moves by
    <= 1e-11 of its max-norm."""
    import qd_oracle as qo
    meta, d = sc.ts_case(shape)
    a = run_oracle_time_step(meta, d)
    d1 = dict(d)
    d1["init_u"] = d["init_u"] * (1.0 + 1e-15)                 # the wind, as tests/test_oracle_polar_noise_cpu.py perturbs it
    b = run_oracle_time_step(meta, d1)
    errs = {k: relerr(getattr(a, k), getattr(b, k)) for k in STATE + DIAG + ("cloud_eff_last",)}
    mask, o = sc.ocean_case(shape)
    runs = []
    for scale in (1.0, 1.0 + 1e-15):
        oo = qo.OceanOracle(qo.Grid(*shape), mask, qo.defaults(ocean_cfl=sc.CASES[shape]["cfl"]), init_Ts=o["init_Ts"].copy())
        oo.uo, oo.vo, oo.eta = o["init_uo"] * scale, o["init_vo"].copy(), o["init_eta"] * scale
        for _ in range(sc.NSTEPS):
            oo.step(sc.DT, o["u_atm"] * scale, o["v_atm"], Q_net=o["Q_net"], ice_mask=o["ice_mask"])
        assert 2 <= oo.last_n_sub <= 6
        runs.append(oo)
    errs.update({"ocean " + k: relerr(getattr(runs[0], k), getattr(runs[1], k)) for k in ("uo", "vo", "eta", "Ts")})
    print(shape, {k: f"{e:.1e}" for k, e in errs.items()})
    for k, e in errs.items():
        assert e <= CHAOS_TOL, (shape, k, e)


@pytest.mark.parametrize("shape", sc.COUPLED_SHAPES)
def test_recorded_coupled_sensitivity_reproduces(shape):
    """step_form_cases.COUPLED_SENS is what coupled_sensitivity measures here, within 10 x (2e-16, one rounding, counts as the floor);
    the atmosphere and surface fields of the same pair of runs stay 100 x below STEP_TOL."""
    ocn, atm = sc.coupled_sensitivity(shape)
    rec = sc.COUPLED_SENS[shape]
    print(shape, "uo / vo / eta", ocn, "recorded", rec, "atmosphere", atm, "bound", sc.coupled_bound(shape))
    assert max(ocn, 2e-16) <= 10.0 * rec and rec <= 10.0 * max(ocn, 2e-16), (shape, ocn, rec)
    assert atm <= CHAOS_TOL
    assert sc.STEP_TOL <= sc.coupled_bound(shape) <= 1e-7
