"""Cost and accuracy of the flow lane (QD_FLOW=1): streamfunction and velocity potential at 721 x 1440.

    python scripts/flow_cost.py [--out profiles/flow_cost.json] [--bench-parent a,b,c --bench-tree a,b,c]

Runs the driver's flag set with full physics and the ocean (no ecology, tracers or routing) from the bench's resting state, prints
one JSON line and writes it to --out:
  * ms per step with the lane off and with the lane sampling every step -- medians over `reps` x `rounds` = 15 spans of `n` = 20
    steps after a warm-up span, every span ending in a synchronise, the cases interleaved `rounds` times -- for the default form (the
    FFT) and for QD_FLOW_FORM=direct; the difference to "off" is one sample's cost;
  * the device time of each of the six launches of a sample (timing groups flow_vortdiv, flow_fwd, flow_lat, flow_inv,
    flow_finish, flow_record), taken from the dispatches themselves, per form;
  * the amortised cost per step at the default cadence (one sample in 24 steps);
  * accuracy: at the shapes of tests/test_gpu_flow.py the max-relative error against the extended-precision solve of the f64 NumPy
    restatement and of the device, for psi and chi (the pairs DESIGN.md lists);
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

SHAPES = [(3, 4), (5, 4), (19, 36), (9, 45), (7, 35), (7, 26), (5, 600), (131, 12)]
GROUPS = ("flow_vortdiv", "flow_fwd", "flow_lat", "flow_inv", "flow_finish", "flow_record")


def accuracy():
    """The (f64 restatement, device) error pairs of the test shapes, with the test's winds."""
    import qingdai_amd as qa
    from qingdai_amd import flow
    out = {}
    a = qa.QdParams().a
    for shape in SHAPES + [(19, 36)]:
        direct = f"{shape[0]}x{shape[1]}" in out
        if direct:
            os.environ["QD_FLOW_FORM"] = "direct"
        try:
            grid = qa.SphericalGrid(*shape)
            g = flow.grid_tables(grid, a)
            r = np.random.default_rng(shape[0] * 10000 + shape[1])
            lat = np.deg2rad(np.linspace(-90, 90, shape[0]))[:, None]
            u, v = 8.0 * np.cos(lat) + 10.0 * r.normal(size=shape), 5.0 * r.normal(size=shape)
            r64, ext, dev = flow.helmholtz_reference(u, v, g), flow.helmholtz_reference(u, v, g, extended=True), flow.solve_grid(grid, a, u, v)
        finally:
            os.environ.pop("QD_FLOW_FORM", None)
        rel = lambda x, ref: float(np.abs(x - ref).max() / np.abs(ref).max())
        out[f"{shape[0]}x{shape[1]}" + ("_direct" if direct else "")] = {
            "psi": {"f64": rel(r64.psi, ext.psi), "device": rel(dev.psi, ext.psi)}, "chi": {"f64": rel(r64.chi, ext.chi), "device": rel(dev.chi, ext.chi)}}
    return out


def main():
    import qingdai_amd as qa
    from qingdai_amd import flow
    from qingdai_amd.driver import Simulation
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=os.path.join(HERE, "..", "profiles", "flow_cost.json"))
    ap.add_argument("--grid", default="721x1440")
    ap.add_argument("--skip-direct", action="store_true", help="leave the direct form out (a quick look)")
    ap.add_argument("--bench-parent", default="", help="ms per step of the parent commit's bench runs, comma-separated")
    ap.add_argument("--bench-tree", default="", help="... and of this tree's, in the order they alternated")
    args = ap.parse_args()
    n_lat, n_lon = (int(x) for x in args.grid.split("x"))
    n, reps, rounds = 20, 5, 3
    out = {"accuracy": accuracy()}
    sim = Simulation(n_lat, n_lon, params=qa.QdParams(), use_ocean=True, quiet=True, ecology=False, individuals=False, phyto=False)
    sim.routing = None
    quiet = lambda s: None

    def new_flow(form):
        """The form is read by the configure call, once."""
        if form == "direct":
            os.environ["QD_FLOW_FORM"] = "direct"
        else:
            os.environ.pop("QD_FLOW_FORM", None)
        try:
            return flow.Flow(sim.dev, sim.grid, {"enabled": True, "every": 1, "every_days": 1e6}, dt=float(sim.dt), day=sim.day_seconds, out=quiet)
        finally:
            os.environ.pop("QD_FLOW_FORM", None)

    def span_ms():
        sim.dev.sync()
        t0 = time.perf_counter()
        sim.run_steps(n)
        sim.dev.sync()
        if sim.flow is not None:
            sim.flow.drop()                                     # the records were delivered; this run keeps none
        return 1e3 * (time.perf_counter() - t0) / n
    sim.run_steps(40)                                           # spin-up: past the first steps' transients
    forms = ("fft",) if args.skip_direct else ("fft", "direct")
    cases = [("off", None)] + [(form, form) for form in forms]
    t = {name: [] for name, _ in cases}
    for _ in range(rounds):
        for name, form in cases:
            sim.flow = new_flow(form) if form else None
            span_ms()
            t[name] += [span_ms() for _ in range(reps)]
            if sim.flow is not None:
                sim.dev.flow_configure(None)
                sim.flow = None
    out.update({name: {"median_ms_per_step": float(np.median(v)), "min": float(np.min(v)), "max": float(np.max(v))} for name, v in t.items()})
    off = out["off"]["median_ms_per_step"]
    out["one_sample_ms"] = {name: out[name]["median_ms_per_step"] - off for name in t if name != "off"}
    out["launches_ms"] = {}
    for form in forms:
        sim.flow = new_flow(form)
        sim.run_steps(n)
        sim.flow.drop()
        got = {g: [] for g in GROUPS}
        for _ in range(rounds):
            for group in got:
                sim.dev.timing(select=group)
                sim.run_steps(n)
                sim.dev.sync()
                sim.flow.drop()
                mean_ms, launches = sim.dev.timing_get(group)
                assert launches == n, (group, launches)
                got[group].append(mean_ms)
        sim.dev.timing(on=False)
        out["launches_ms"][form] = {g: float(np.median(v)) for g, v in got.items()}
        out["launches_ms"][form]["sum"] = float(sum(out["launches_ms"][form].values()))
        sim.dev.flow_configure(None)
        sim.flow = None
    out["default_cadence"] = {"every": flow.EVERY, "amortised_ms_per_step": out["one_sample_ms"]["fft"] / flow.EVERY}
    if "direct" in forms:
        out["fft_is_faster"] = bool(out["launches_ms"]["fft"]["sum"] < out["launches_ms"]["direct"]["sum"])
    out["grid"] = [n_lat, n_lon]
    out["bench_ms_per_step"] = {"parent": [float(x) for x in args.bench_parent.split(",") if x], "tree": [float(x) for x in args.bench_tree.split(",") if x]}
    text = json.dumps(out)
    print(text)
    os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
    with open(args.out, "w", encoding="utf-8") as f:
        f.write(text + "\n")


if __name__ == "__main__":
    main()
