#!/usr/bin/env python3
"""Bit-for-bit fingerprint of the five feature modules whose kernels end in a workgroup reduction (csrc/qd_blockred.h): one
routing event, two daily phytoplankton steps, two vegetation firings with spread on, one diversity call and one true-colour
render on a whole-globe handle, from seeded inputs.

    reduction_fingerprint.py --out F.npz           run on the GPU, store every output (logs, summaries, maps, images, fields)
    reduction_fingerprint.py --compare A.npz B.npz  np.array_equal(..., equal_nan=True) on every key, exit status 1 on a difference

Run it on two builds of the library (PYTHONPATH picks the package) and compare: a change that is meant to keep every summation
order keeps every key.  Shapes: 23 x 300 (two x-blocks per row, the second with 44 live threads; 46 row-blocks, fewer than a wave)
and 131 x 300 (262 row-blocks: the block-strided second stage loops twice, the lane-strided one five times with a ragged tail; 154
true-colour blocks).  tests/test_gpu_blockred.py checks the same runs against the NumPy restatements."""
import argparse
import os
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
if ROOT not in sys.path:
    sys.path.insert(0, ROOT)

SHAPES = ((23, 300), (131, 300))
DT = 3600.0
ENV = {"QD_ECO_NS": "5", "QD_ECO_COHORT_K": "2", "QD_ECO_SPREAD_ENABLE": "1", "QD_ECO_SPREAD_RATE": "0.1", "QD_ECO_RAND_SEED": "7",
       "QD_ECO_SEED_ENERGY": "500", "QD_ECO_SPREAD_SOIL_EXP": "1.5", "QD_PHYTO_NSPECIES": "4"}
TC_FIELDS = {"HICE": "h_ice", "C_SNOW": "C_snow", "CLOUD": "cloud", "TS": "T_s", "ISR": "isr", "ISR_A": "isr_A", "ISR_B": "isr_B", "ECO_F": "eco_f"}
NB_TC = 16


def set_env():
    """The environment the five modules read their parameters from: nothing inherited, ENV on top."""
    for k in [k for k in os.environ if k.startswith(("QD_ECO_", "QD_PHYTO_", "QD_STAR_", "QD_PLOT_", "QD_TRUECOLOR_"))]:
        del os.environ[k]
    os.environ.update(ENV)


def south_network(land):
    """Every land cell drains into the land cell south of it, the southernmost of a column into the ocean; no lakes."""
    n_lat, n_lon = land.shape
    idx = np.arange(n_lat * n_lon, dtype=np.int64).reshape(n_lat, n_lon)
    ft = np.full((n_lat, n_lon), -1, dtype=np.int64)
    ft[1:] = np.where((land[1:] == 1) & (land[:-1] == 1), idx[:-1], -1)
    ft[land != 1] = -1
    order = idx[::-1][land[::-1] == 1]                          # northern rows first: a cell comes before its target
    return dict(land_mask=land.astype(np.uint8), flow_to_index=ft, flow_order=np.ascontiguousarray(order))


def build_inputs(shape, seed=11, land=None):
    """Seeded inputs of the whole scenario -> dict of arrays (and the true-colour parameter tuple under "tc")."""
    from qingdai_amd import _lib
    n_lat, n_lon = shape
    r = np.random.default_rng(seed + 1000 * n_lat + n_lon)
    if land is None:
        land = (r.uniform(size=shape) < 0.45).astype(np.uint8)
    land = np.ascontiguousarray(land, dtype=np.uint8)
    lm, oc = land == 1, land == 0
    S, K, SP = int(ENV["QD_ECO_NS"]), int(ENV["QD_ECO_COHORT_K"]), int(ENV["QD_PHYTO_NSPECIES"])
    inp = {"land": land,
           "R": r.uniform(-1e-6, 2e-5, shape), "P": r.uniform(0.0, 4e-5, shape), "E": r.uniform(0.0, 3e-5, shape),
           "C0": np.abs(r.lognormal(np.log(0.3), 0.5, (SP,) + shape)) * oc, "N0": np.where(oc, r.uniform(0.2, 2.0, shape), 0.0),
           "Tw": 275.0 + 25.0 * r.uniform(size=shape), "star_t": np.array([3.0e6, 3.0e6 + 86400.0]),
           "L0": r.uniform(0.0, 0.15, (S, K) + shape) * lm, "bank0": r.uniform(0.0, 3.0, shape) * lm,
           "E_days": r.uniform(0.0, 2.0e4, (2,) + shape), "soil": r.uniform(0.0, 0.9, (2,) + shape)}
    tc = {"h_ice": np.where(r.uniform(size=shape) < 0.5, 0.0, r.uniform(0.2, 2.0, shape)), "C_snow": r.uniform(-0.2, 1.4, shape),
          "cloud": r.uniform(0.0, 1.0, shape), "T_s": r.uniform(250.0, 300.0, shape), "isr_A": r.uniform(0.0, 700.0, shape),
          "isr_B": r.uniform(0.0, 300.0, shape), "eco_f": r.uniform(-0.1, 1.1, shape)}
    tc["isr_A"][:, : n_lon // 3] = 0.0
    tc["isr_B"][:, : n_lon // 2] = 0.0                          # a night side
    tc["isr"] = tc["isr_A"] + tc["isr_B"]
    inp.update({"tc_" + k: v for k, v in tc.items()})

    def tab(rows):
        t = r.uniform(0.05, 1.0, (rows, NB_TC))
        t[-6:-3] /= t[-6:-3].sum(axis=1, keepdims=True)          # the channel weights are normalised
        return t
    inp["tc_eco_tab"], inp["tc_phyto_tab"] = tab(7), tab(6)
    bands = r.uniform(0.0, 0.3, (NB_TC,) + shape)
    bands[:, lm] = np.nan
    inp["tc_bands"], inp["tc_flow"] = bands, 10.0 ** r.uniform(4.0, 8.0, shape)
    inp["tc_lake"] = (r.uniform(size=shape) < 0.2).astype(np.uint8)
    inp["tc"] = _lib.qd_truecolor_params(1, 1, 0, 1, 1, 1, 1, NB_TC, NB_TC, 0, 0.5, 0.15, 0.2, 0.6, 1.8, 1.35, 0.2, 2.2, 0.85, 262.0, 0.6,
                                         0.95, 1e6, 0.45, 0.4)
    return inp


def run_device(shape, inp):
    """The scenario on a fresh whole-globe handle -> dict of every output.  set_env() first."""
    import ctypes
    import qingdai_amd as qa
    from qingdai_amd.device import Device
    from qingdai_amd.ecology import EcologyAdapter, PopulationDaily
    from qingdai_amd.phyto import PhytoDaily, PhytoTracers
    from qingdai_amd.routing import RiverRouting
    grid = qa.SphericalGrid(*shape)
    land = inp["land"]
    dev = Device(grid)
    dev.upload_now("LAND_MASK", land)
    out = {}
    # one routing event: the accumulation of one step, then the event with the lake P - E term requested
    rr = RiverRouting.from_arrays(grid, dt_hydro_hours=DT / 3600.0, diag=False, dev=dev, **south_network(land))
    rr.step(inp["R"], DT, precip_flux=inp["P"], evap_flux=inp["E"])
    out["route_log"] = np.array(list(dev.route_last_event().values()), dtype=np.float64)
    out["route_flow"], out["route_buffer"] = dev.route_download("FLOW"), dev.route_download("BUFFER")
    # two daily phytoplankton steps
    tr = PhytoTracers(grid, land, dev=dev)
    dev.phyto_upload(inp["C0"])
    pd = PhytoDaily(tr, H_mld_m=50.0, diag=False, dev=dev)
    pd.N = inp["N0"]
    dev.upload_now("SST", inp["Tw"])
    stars = np.ascontiguousarray(qa.ThermalForcing(grid, qa.OrbitalSystem()).star_table(inp["star_t"]))
    dp = ctypes.POINTER(ctypes.c_double)
    ins = np.empty((2, 2) + shape)
    for d in range(2):
        dev._chk(dev.lib.qd_phyto_daily_insolation(dev.h, stars[d].ctypes.data_as(dp), ins[d, 0].ctypes.data_as(dp),
                                                    ins[d, 1].ctypes.data_as(dp)), "qd_phyto_daily_insolation")
        dev.phyto_daily(stars[d], True)
        pd._fired(1)
    out["phyto_log"], out["phyto_insolation"] = dev.phyto_daily_log(), ins
    bands, scalar = pd.get_alpha_maps()
    out.update({"phyto_C": tr.C_phyto_s, "phyto_N": pd.N, "phyto_bands": bands, "WATER_ALPHA": scalar, "KD490": pd.get_kd490()})
    # two vegetation firings, spread on
    pop = EcologyAdapter(grid, land, dev=dev, albedo_couple=True).pop
    daily = PopulationDaily(pop)
    pop.push_layers(inp["L0"], init=True)
    pop.seed_bank = inp["bank0"]
    for d in range(2):
        pop.E_day = inp["E_days"][d]
        pop.step_daily(inp["soil"][d])
    out["eco_log"] = dev.eco_daily_log()
    out["eco_modes"] = np.array([1 if m == "seed" else 0 for m in daily.species_modes])
    out["eco_weights"] = np.asarray(pop.species_weights, dtype=np.float64)
    out["eco_layers"] = pop.LAI_layers_SK.copy()
    for k in ("ECO_LAI", "ECO_EDAY", "ECO_AGE", "ECO_SEEDBANK", "ECO_GATE"):
        dev._host.pop(k, None)
        out[k] = np.array(dev.get(k), copy=True)
    # one diversity call on the resident stack
    alpha, bc, L_s, s = pop.diversity()
    out.update({"div_alpha": alpha, "div_bc": bc, "div_Ls": L_s, "div_summary": np.array([s["alpha_mean"], s["gamma_eff"], s["beta_whittaker"]])})
    # one true-colour render with every overlay on
    for fid, key in TC_FIELDS.items():
        dev.upload_now(fid, inp["tc_" + key])
    dev.truecolor_configure(inp["tc"], inp["tc_eco_tab"], inp["tc_phyto_tab"], inp["tc_bands"], inp["tc_lake"])
    area, mean_h = dev.truecolor_render(want_f64=True, flow=inp["tc_flow"])
    out.update({"tc_img": dev.truecolor_image(), "tc_rgb": dev.truecolor_rgb(), "tc_sea_ice": np.array([area, mean_h])})
    dev.close()
    return out


def compare(a_path, b_path):
    a, b = np.load(a_path), np.load(b_path)
    bad = sorted(set(a.files) ^ set(b.files))
    for k in sorted(set(a.files) & set(b.files)):
        if not (a[k].shape == b[k].shape and np.array_equal(a[k], b[k], equal_nan=a[k].dtype.kind == "f")):
            bad.append(k)
    print(f"{len(a.files)} keys, {len(bad)} differ" + (": " + ", ".join(bad) if bad else ""))
    return 1 if bad else 0


def main(argv=None):
    ap = argparse.ArgumentParser(description=__doc__.split("\n\n")[0])
    ap.add_argument("--out")
    ap.add_argument("--compare", nargs=2, metavar=("A", "B"))
    a = ap.parse_args(argv)
    if a.compare:
        return compare(*a.compare)
    if not a.out:
        ap.error("--out F.npz or --compare A.npz B.npz")
    set_env()
    store = {}
    for shape in SHAPES:
        for k, v in run_device(shape, build_inputs(shape)).items():
            store[f"{shape[0]}x{shape[1]}/{k}"] = v
    np.savez(a.out, **store)
    print(f"{a.out}: {len(store)} keys")
    return 0


if __name__ == "__main__":
    sys.exit(main())
