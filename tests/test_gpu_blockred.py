"""GPU (-m gpu): the reduced quantities of the five modules that share csrc/qd_blockred.h -- the routing event record, the
[PhytoDiag] means, the vegetation summary, the Whittaker summary and the two sea-ice numbers -- against the NumPy restatements the
project keeps (routing_ref, phyto_daily_ref, eco_daily_ref, diversity_ref, truecolor_ref), on the scenario of
scripts/reduction_fingerprint.py (one routing event, two daily phytoplankton steps, two vegetation firings with spread on, one
diversity call, one true-colour render).

Shapes: 23 x 300 (two x-blocks per row, the second with 44 live threads; 46 row-blocks, fewer than a wave) and 131 x 300 (262
row-blocks: the block-strided second stage loops twice, the lane-strided one five times with a ragged tail; 154 true-colour
blocks); 23 x 300 once more with a mask that leaves whole workgroups (and whole waves of others) without land, so that the
vegetation minimum and maximum meet their identity elements in both stages.

Tolerances are the ones the modules' own tests hold for the same quantities: 1e-12 relative on the routing record (test_gpu_routing
_close), rtol 1e-10 on the [PhytoDiag] means (test_gpu_phyto_daily, the resident loop), 1e-12 on the vegetation summary
(test_gpu_eco_daily, the 721 x 1440 firing), test_gpu_diversity.BOUND on the Whittaker summary, truecolor_ref.BOUND on the sea-ice
numbers."""
import importlib.util
import os

import numpy as np
import pytest

import diversity_ref
import eco_daily_ref
import phyto_daily_ref
import truecolor_ref
from routing_ref import SeqRouting
from test_gpu_diversity import BOUND as DIV_BOUND, deviation as div_deviation
from util import relerr

pytestmark = pytest.mark.gpu

HERE = os.path.dirname(os.path.abspath(__file__))
_spec = importlib.util.spec_from_file_location("reduction_fingerprint", os.path.join(HERE, "..", "scripts", "reduction_fingerprint.py"))
fp = importlib.util.module_from_spec(_spec)
_spec.loader.exec_module(fp)


def sparse_land(shape):
    """Land only in rows 9.. and there only in columns 70..249: the second x-block of every row, the first x-block of rows 0..8, the
    four diversity row-blocks 0..1 and the first wave of every first x-block hold no land."""
    land = np.zeros(shape, dtype=np.uint8)
    r = np.random.default_rng(5)
    land[9:, 70:250] = r.uniform(size=(shape[0] - 9, 180)) < 0.6
    return land


CASES = {"23x300": ((23, 300), None), "131x300": ((131, 300), None), "23x300-sparse": ((23, 300), sparse_land)}


def expected(shape, inp, got):
    """The five reduced quantities from the restatements (the insolation, the species modes and weights are the device run's)."""
    import qingdai_amd as qa
    from qingdai_amd.phyto import daily_tables
    from qingdai_amd.routing import cell_area_rows, network_from_vars
    grid = qa.SphericalGrid(*shape)
    land = inp["land"]
    want = {}
    seq = SeqRouting(network_from_vars(fp.south_network(land), shape), cell_area_rows(grid), fp.DT)
    want["route"] = seq.step(inp["R"], fp.DT, inp["P"], inp["E"])
    tab = phyto_daily_ref.tables_from_host(daily_tables(inp["C0"].shape[0], H_mld_m=50.0))
    C, N, means = inp["C0"], inp["N0"], []
    for d in range(2):
        r = phyto_daily_ref.step_daily(C, N, got["phyto_insolation"][d, 0], got["phyto_insolation"][d, 1], inp["Tw"], tab, land)
        C, N = r["C"], r["N"]
        means.append(r["means"])
    want["phyto_means"] = np.array(means)
    lm = land == 1
    st = eco_daily_ref.State(lm, inp["L0"].copy(), None, np.zeros(shape), inp["bank0"].copy(), lm.astype(float))
    cfg = eco_daily_ref.Cfg.from_env(fp.ENV, ["seed" if m else "diffusion" for m in got["eco_modes"]], got["eco_weights"])
    summ = []
    for d in range(2):
        st.E_day = inp["E_days"][d].copy()
        eco_daily_ref.step_daily(st, cfg, inp["soil"][d])
        s = st.summary()
        summ.append([s["LAI_min"], s["LAI_mean"], s["LAI_max"]])
    want["eco_summary"], want["eco_layers"] = np.array(summ), st.layers
    want["div"] = diversity_ref.diversity(got["eco_layers"], land, grid.lat_mesh)
    tc = {k[3:]: v for k, v in inp.items() if k.startswith("tc_")}
    tc["land_mask"] = land
    want["tc"] = truecolor_ref.render(tc, inp["tc"], inp["tc_eco_tab"], inp["tc_phyto_tab"], inp["tc_bands"], inp["tc_lake"], inp["tc_flow"],
                                      lat=grid.lat)
    return want


@pytest.mark.parametrize("case", list(CASES))
def test_reduced_quantities_vs_restatements(gpu, case, monkeypatch):
    shape, mask = CASES[case]
    for k in [k for k in os.environ if k.startswith(("QD_ECO_", "QD_PHYTO_", "QD_STAR_", "QD_PLOT_", "QD_TRUECOLOR_"))]:
        monkeypatch.delenv(k)
    for k, v in fp.ENV.items():
        monkeypatch.setenv(k, v)
    inp = fp.build_inputs(shape, land=None if mask is None else mask(shape))
    got = fp.run_device(shape, inp)
    want = expected(shape, inp, got)
    # routing: step, event_dt, ocean_kgps, closure, input, ocean_kg, residual, lake_delta
    rec, w = got["route_log"], want["route"]
    assert rec[0] == 1.0 and rec[1] == fp.DT and w["mass_input_kg"] != 0.0
    e_ocean = abs(rec[2] - w["ocean_inflow_kgps"]) / max(abs(w["ocean_inflow_kgps"]), 1e-300)
    e_close = abs(rec[3] - w["mass_closure_error_kg"]) / max(abs(w["mass_input_kg"]), 1e-300)
    assert np.array_equal(got["route_flow"].reshape(shape), w["flow"]) and not got["route_buffer"].any()
    # phytoplankton: the three area-weighted means of both days
    assert got["phyto_log"].shape == (2, 4) and list(got["phyto_log"][:, 0]) == [1.0, 2.0]
    e_phyto = float(np.max(np.abs(got["phyto_log"][:, 1:] - want["phyto_means"]) / np.abs(want["phyto_means"])))
    # vegetation: min, mean, max over land after both firings
    assert got["eco_log"].shape == (2, 4) and list(got["eco_log"][:, 0]) == [1.0, 2.0]
    e_eco = max(relerr(got["eco_log"][d, 1:], want["eco_summary"][d]) for d in range(2))
    e_layers = relerr(got["eco_layers"], want["eco_layers"])
    # diversity and true colour
    e_div = div_deviation(got["div_summary"], want["div"]["summary"])
    e_ice = float(np.max(np.abs(got["tc_sea_ice"] - want["tc"]["sea_ice"])))
    print(f"{case}: route ocean {e_ocean:.2e} closure {e_close:.2e} | phyto {e_phyto:.2e} | eco summary {e_eco:.2e} "
          f"layers {e_layers:.2e} | diversity {e_div:.2e} | sea ice {e_ice:.2e}")
    assert max(e_ocean, e_close) <= 1e-12
    assert np.allclose(got["phyto_log"][:, 1:], want["phyto_means"], rtol=1e-10)
    assert e_eco <= 1e-12
    assert np.array_equal(got["div_Ls"], want["div"]["L_s"], equal_nan=True)
    assert e_div <= DIV_BOUND
    assert e_ice <= truecolor_ref.BOUND
    # not vacuous: every reduction saw land and ocean, ice and open water, and the vegetation moved
    assert got["eco_log"][1, 1] < got["eco_log"][1, 2] < got["eco_log"][1, 3] and np.abs(want["eco_layers"] - inp["L0"]).max() > 0.01
    assert got["tc_sea_ice"][0] > 0.0 and got["tc_sea_ice"][1] > 0.0 and np.isfinite(got["div_summary"]).all()
