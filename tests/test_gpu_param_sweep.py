"""GPU (-m gpu): every run-time parameter of `qd_params`, one at a time, through the device path and the oracle.

One case per row of tests/param_sweep_cases.py: QdParams(**companions, **{param: value}), the row's scenario at 37 x 72 through the
C-ABI (SpectralModel.time_step, WindDrivenSlabOcean.step, Simulation.run_steps -> Device.step_n, Device.driver_physics), the
oracle on the same inputs, and -- where the row has one -- the reference's own digest of that run (tests/golden/param_sweep_*).
tests/test_param_sweep_cpu.py shows without a GPU that every row moves the oracle's result by at least 1000 x the bound below, so
a kernel with the default baked in, a table built from the wrong field or two swapped struct members fails its row here.
The rows marked `unfused` (their parameter reaches the fused dynamics / ocean kernels) run a second time with QD_FUSED=0: the
reference-order kernels read their parameters separately.

  scenario      compared                                      bound     worst measured (MI355X), fused / QD_FUSED=0
  column        u v h T_s q cloud h_ice + 5 diagnostics +     1e-9      7.3e-12 / 7.3e-12  (filter_type=spectral: cloud_eff_last)
  column_init   cloud_eff, 7 (2) time_steps with albedo       1e-9      1.2e-13  (H=7500: v)
  ocean         uo vo eta Ts, 3 steps of 7 sub-steps          1e-9      5.3e-13 (ocean_k4_u: eta) / 1.4e-11 (ocean_cfl=0.03: eta)
  driver        state + precip albedo snow bucket runoff SST  1e-9      1.3e-13  (alpha_cloud: v)
                uo vo eta of the coupled run, 4 steps         1e-7      2.4e-15  (alpha_cloud: vo)
                step-1 precipitation and albedo               1e-11     2.6e-16  (lapse_k_kpm: albedo)
  orog          precipitation of one driver_physics call      1e-11     4.3e-16  (orog_enable=0)
  DEAD          perturbed run == baseline, bit for bit
(worst over the rows of the scenario, against the oracle and against the reference's digest, whichever is larger)

The bounds are the project's existing ones (tests/test_gpu_parity.py: STEP_TOL, the coupled ocean's 1e-7 after 4 steps,
the step-1 diagnostics' 1e-11).  A row may carry a looser bound only as 100 x the oracle's own noise under a 1e-15 perturbation
of one input (param_sweep_cases.R: `noise`, `tol`), measured on the CPU -- never from the device's error.
"""
import numpy as np
import pytest

import param_sweep_cases as C
from util import load_golden

pytestmark = pytest.mark.gpu

_ORACLE = {}           # (scenario, companions) -> oracle baseline
_DEVICE = {}           # (scenario, companions, fused) -> device baseline
_GOLD = {}


def _key(scenario, comp):
    return (scenario, tuple(sorted(comp.items())))


def _set_fused(monkeypatch, fused):
    """QD_FUSED is read in qd_create: set before any handle of the run is built."""
    monkeypatch.delenv("QD_FUSED", raising=False)
    if not fused:
        monkeypatch.setenv("QD_FUSED", "0")


def oracle_run(scenario, over):
    with np.errstate(all="ignore"):
        return C.run_oracle(scenario, over)


def oracle_baseline(scenario, comp):
    k = _key(scenario, comp)
    if k not in _ORACLE:
        _ORACLE[k] = oracle_run(scenario, comp)
    return _ORACLE[k]


def device_baseline(monkeypatch, scenario, comp, fused=True):
    k = _key(scenario, comp) + (fused,)
    if k not in _DEVICE:
        _set_fused(monkeypatch, fused)
        _DEVICE[k] = C.run_device(scenario, comp)
    return _DEVICE[k]


def gold(scenario):
    if scenario not in _GOLD:
        _GOLD[scenario] = load_golden(C.fixture_name(scenario))
    return _GOLD[scenario]


def check_row(monkeypatch, row, fused):
    scn = row["scenario"]
    over = {**row["comp"], row["param"]: row["value"]}
    _set_fused(monkeypatch, fused)
    got = C.run_device(scn, over)
    want = oracle_run(scn, over)
    tol = C.row_tol(row)
    errs = {k: C.relerr(got[k], want[k]) for k in tol}
    ref_errs = {}
    if row["fixture"]:
        meta, d = gold(scn)
        ri = meta["rows"].index(row["id"])
        for fi, k in enumerate(meta["fields"]):
            scale = max(float(d["maxs"][ri, fi]), 1e-300)
            vals, s, _ = C.digest(got[k], d["cells"])
            ref_errs[k] = max(float(np.max(np.abs(vals - d["vals"][ri, fi]))) / scale,
                              abs(s - float(d["sums"][ri, fi])) / (got[k].size * scale))
    print(f"sweep {scn} {row['id']} fused={int(fused)} oracle:", {k: f"{e:.1e}" for k, e in errs.items()},
          "reference:", {k: f"{e:.1e}" for k, e in ref_errs.items()})
    if "n_sub" in want:
        assert got["n_sub"] == want["n_sub"]
    # the baseline of the same companions: the device, too, responds to the parameter (and is right at the baseline)
    base = device_baseline(monkeypatch, scn, row["comp"], fused)
    obase = oracle_baseline(scn, row["comp"])
    for k in tol:
        assert C.relerr(base[k], obase[k]) < tol[k], ("baseline", k)
    assert any(C.relerr(got[k], base[k]) >= 0.5 * C.live_threshold(tol[k]) for k in tol)
    for k in tol:
        assert errs[k] < tol[k], (row["id"], k, errs[k], "vs oracle")
    for k, e in ref_errs.items():
        assert e < tol[k], (row["id"], k, e, "vs reference digest")


@pytest.mark.parametrize("row", C.ROWS, ids=[r["id"] for r in C.ROWS])
def test_parameter_reaches_the_device(gpu, monkeypatch, row):
    check_row(monkeypatch, row, fused=True)


UNFUSED = [r for r in C.ROWS if r["unfused"]]


@pytest.mark.parametrize("row", UNFUSED, ids=[r["id"] for r in UNFUSED])
def test_parameter_reaches_the_unfused_kernels(gpu, monkeypatch, row):
    check_row(monkeypatch, row, fused=False)


@pytest.mark.parametrize("name", sorted(C.DEAD))
def test_dead_parameter_changes_nothing_on_the_device(gpu, monkeypatch, name):
    scn, value, _ = C.DEAD[name]
    base = device_baseline(monkeypatch, scn, {})
    _set_fused(monkeypatch, True)
    got = C.run_device(scn, {name: value})
    for k in C.SCENARIOS[scn]["fields"]:
        assert np.array_equal(got[k], base[k]), k
