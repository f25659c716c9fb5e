"""Cost and accuracy of the spherical-harmonic lane (QD_SPHARM=1) at 721 x 1440 (T360).

    python scripts/spharm_cost.py [--out profiles/spharm_cost.json] [--bench-parent a,b,c --bench-tree a,b,c]

Runs the driver's flag set with full physics and the ocean (no ecology, tracers or routing) from the bench's resting state, prints
one JSON line and writes it to --out:
  * ms per step with the lane off and with the lane sampling every step (the default fields VORT, DIV, H, the 2D sums on) -- medians
    over `reps` x `rounds` = 15 spans of `n` = 20 steps after a warm-up span, every span ending in a synchronise, the cases
    interleaved `rounds` times; the difference to "off" is one sample's cost;
  * the device time of each launch of a sample (timing groups spharm_vortdiv, spharm_rows, spharm_leg, spharm_record), taken from
    the dispatches themselves (HIP events attached to the launch); spharm_leg is the Legendre stage alone;
  * the amortised cost per step at the default cadence (one sample in 24 steps), next to the flow lane's sample for scale;
  * accuracy: at the shapes of tests/test_gpu_spharm.py the error against the extended-precision analysis, over the largest
    coefficient, of the f64 NumPy restatement and of the device (the pairs DESIGN.md lists);
  * the same pair at the full size, through the handle's seam: the device's coefficients of a 721 x 1440 plane against the f64 and the
    extended analysis, and Parseval's residual of a band-limited plane;
  * bench: `bench.py --gpus 1` ms per step with the lane off, parent commit and this tree alternating, as handed in on the command
    line (the runs are made by hand: two checkouts).
DESIGN.md quotes the result."""
import argparse
import json
import os
import sys
import time

import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, os.path.join(HERE, ".."))

SHAPES = [(5, 8), (3, 8), (19, 36), (9, 45), (20, 36), (33, 24), (7, 26), (131, 12), (256, 8), (257, 8), (768, 8), (769, 8)]
GROUPS = ("spharm_vortdiv", "spharm_rows", "spharm_leg", "spharm_record")
FLOW_SAMPLE_MS = 0.375                  # the flow lane's sample at the same grid (profiles/flow_cost.json), for scale


def accuracy():
    """The (f64 restatement, device) error pairs of the test shapes, with the test's plane."""
    from qingdai_amd import spharm
    out = {}
    for shape in SHAPES + [(19, 36)]:
        direct = f"{shape[0]}x{shape[1]}" in out
        if direct:
            os.environ["QD_SPHARM_FORM"] = "direct"
        try:
            g = spharm.tables(*shape)
            r = np.random.default_rng(shape[0] * 10000 + shape[1])
            lat = np.deg2rad(np.linspace(-90, 90, shape[0]))[:, None]
            x = 8.0 * np.cos(lat) + 10.0 * r.normal(size=shape)
            c64, ext, dev = spharm.analyse_reference(x, g), spharm.analyse_reference(x, g, extended=True), spharm.analyse_grid(shape[0], shape[1], x)
        finally:
            os.environ.pop("QD_SPHARM_FORM", None)
        rel = lambda c, ref: float(np.abs(c - ref).max() / np.abs(ref).max())
        out[f"{shape[0]}x{shape[1]}" + ("_direct" if direct else "")] = {"N": g.N, "f64": rel(c64, ext), "device": rel(dev.coef, ext)}
    return out


def full_size(dev, g):
    """The error pair at the handle's own grid, the lane configured: the test's kind of plane, and a band-limited one."""
    from qingdai_amd import spharm
    r = np.random.default_rng(7)
    lat = np.deg2rad(np.linspace(-90, 90, g.n_lat))[:, None]
    x = 8.0 * np.cos(lat) + 10.0 * r.normal(size=(g.n_lat, g.n_lon))
    c64, ext = spharm.analyse_reference(x, g), spharm.analyse_reference(x, g, extended=True)
    coef, rec = dev.spharm_analyse(x)
    rel = lambda c, ref: float(np.abs(c - ref).max() / np.abs(ref).max())
    P, ms, bad = spharm.power_reference(coef, x, g)
    c = np.triu(r.normal(size=(g.N + 1, g.N + 1)) + 1j * r.normal(size=(g.N + 1, g.N + 1))) / (1.0 + np.arange(g.N + 1))[None, :]
    c[0] = c[0].real
    y = spharm.synthesise(c, g)
    back, rec_y = dev.spharm_analyse(y)
    return {"f64": rel(c64, ext), "device": rel(coef, ext), "record_is_the_restatement": bool(np.array_equal(rec[:g.N + 1], P) and rec[g.N + 1] == ms),
            "resid_of_white_noise_plane": float(spharm.resid(rec[:g.N + 1], rec[g.N + 1])),
            "round_trip": {"f64": float(np.abs(spharm.analyse_reference(y, g) - c).max()), "device": float(np.abs(back - c).max())},
            "parseval_resid_band_limited": float(spharm.resid(rec_y[:g.N + 1], rec_y[g.N + 1]))}


def main():
    import qingdai_amd as qa
    from qingdai_amd import spharm
    from qingdai_amd.driver import Simulation
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=os.path.join(HERE, "..", "profiles", "spharm_cost.json"))
    ap.add_argument("--grid", default="721x1440")
    ap.add_argument("--bench-parent", default="", help="ms per step of the parent commit's bench runs, comma-separated")
    ap.add_argument("--bench-tree", default="", help="... and of this tree's, in the order they alternated")
    args = ap.parse_args()
    n_lat, n_lon = (int(x) for x in args.grid.split("x"))
    n, reps, rounds = 20, 5, 3
    out = {"accuracy": accuracy()}
    sim = Simulation(n_lat, n_lon, params=qa.QdParams(), use_ocean=True, quiet=True, ecology=False, individuals=False, phyto=False)
    sim.routing = None
    quiet = lambda s: None
    cfg = {"enabled": True, "every": 1, "every_days": 1e6, "two_d": True, "fields": None}

    def new_lane():
        return spharm.Spharm(sim.dev, sim.grid, cfg, with_ocean=True, dt=float(sim.dt), day=sim.day_seconds, out=quiet)

    def span_ms():
        sim.dev.sync()
        t0 = time.perf_counter()
        sim.run_steps(n)
        sim.dev.sync()
        if sim.spharm is not None:
            sim.spharm.drop()                                   # the records were delivered; this run keeps none
        return 1e3 * (time.perf_counter() - t0) / n
    sim.run_steps(40)                                           # spin-up: past the first steps' transients
    t = {"off": [], "on": []}
    for _ in range(rounds):
        for name in t:
            sim.spharm = new_lane() if name == "on" else None
            span_ms()
            t[name] += [span_ms() for _ in range(reps)]
            if sim.spharm is not None:
                sim.dev.spharm_configure([], False, None)
                sim.spharm = None
    out.update({name: {"median_ms_per_step": float(np.median(v)), "min": float(np.min(v)), "max": float(np.max(v))} for name, v in t.items()})
    out["one_sample_ms"] = out["on"]["median_ms_per_step"] - out["off"]["median_ms_per_step"]
    sim.spharm = new_lane()
    out["truncation"], out["fields"] = sim.spharm.N, list(sim.spharm.names)
    out["full_size"] = full_size(sim.dev, sim.spharm.tables)
    sim.run_steps(n)
    sim.spharm.drop()
    got = {g: [] for g in GROUPS}
    for _ in range(rounds):
        for group in got:
            sim.dev.timing(select=group)
            sim.run_steps(n)
            sim.dev.sync()
            sim.spharm.drop()
            mean_ms, launches = sim.dev.timing_get(group)
            assert launches == n, (group, launches)
            got[group].append(mean_ms)
    sim.dev.timing(on=False)
    out["launches_ms"] = {g: float(np.median(v)) for g, v in got.items()}
    out["launches_ms"]["sum"] = float(sum(out["launches_ms"].values()))
    out["legendre_stage_ms"] = out["launches_ms"]["spharm_leg"]
    sim.dev.spharm_configure([], False, None)
    sim.spharm = None
    out["default_cadence"] = {"every": spharm.EVERY, "amortised_ms_per_step": out["one_sample_ms"] / spharm.EVERY}
    out["flow_lane_sample_ms_for_scale"] = FLOW_SAMPLE_MS
    out["grid"] = [n_lat, n_lon]
    out["bench_ms_per_step"] = {"parent": [float(x) for x in args.bench_parent.split(",") if x], "tree": [float(x) for x in args.bench_tree.split(",") if x]}
    text = json.dumps(out)
    print(text)
    os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
    with open(args.out, "w", encoding="utf-8") as f:
        f.write(text + "\n")


if __name__ == "__main__":
    main()
