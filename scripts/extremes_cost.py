"""Cost of the extremes lane (QD_EXTREMES=1) at 721 x 1440, next to the step it rides on and to history's accumulate launches.

    python scripts/extremes_cost.py [--out profiles/extremes_cost.json]

Runs the driver's flag set with full physics and the ocean (no ecology, tracers or routing) from the bench's resting state, the
default lists (5 entries with SST, 2 thresholds, 3 histograms), and prints one JSON line (and writes it to --out):
  * ms per step with the lane off, with every step sampled and at the default cadence (every fourth step) -- medians over 15 spans of
    20 steps (5 per round, the three cases interleaved three times in one process), every span ending in a synchronise;
  * the device time of k_ext_accum from the library's timing group "extremes" (taken from the dispatches themselves; two launches per
    sampled step: PRECIP's early one and the rest) in a run of its own, and the bytes a sample LOADS in steady state (per cell: 8 per
    source plane, 16 for vmax and vmin per entry, 16 per threshold) with the GB/s that gives -- stores go out only where a value
    changed and are not counted, so the figure is a lower bound of the traffic;
  * the yardstick, in the same process: history's k_hist_accum launches (group "history", default field list, every step sampled)
    with their bytes (8 per source read, 16 per sum) and GB/s;
  * the device's copy ceiling (qd_copy_ceiling);
  * the resource usage of the kernel, as the compiler reports it (-Rpass-analysis=kernel-resource-usage).
profiles/README.md and DESIGN.md section 7 quote the result."""
import argparse
import json
import os
import sys
import time

import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, os.path.join(HERE, ".."))

# k_ext_accum; hipcc for gfx950, ROCm 7
RESOURCES = {"kernel": "k_ext_accum", "vgprs": 36, "sgprs": 53, "scratch_bytes": 0, "lds_bytes": 24736, "waves_per_simd": 6}


def main():
    import qingdai_amd as qa
    from qingdai_amd import extremes as ex, history as hs
    from qingdai_amd.driver import Simulation
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=None)
    args = ap.parse_args()
    n_lat, n_lon, n, reps, rounds = 721, 1440, 20, 5, 3
    sim = Simulation(n_lat, n_lon, params=qa.QdParams(), use_ocean=True, quiet=True, ecology=False, individuals=False, phyto=False)
    sim.routing = None

    def lane(k):
        cfg = {"enabled": True, "every_days": 1e6, "sample_every": k}       # one window: nothing is written
        return ex.Extremes(sim.dev, sim.grid, cfg, with_ocean=True, dt=float(sim.dt), day=sim.day_seconds, out=lambda s: None)

    def span_ms():
        sim.dev.sync()
        t0 = time.perf_counter()
        sim.run_steps(n)
        sim.dev.sync()
        return 1e3 * (time.perf_counter() - t0) / n
    sim.run_steps(40)                                           # spin-up: past the first steps' transients
    t = {"off": [], "every_step": [], "every_4th": []}
    for _ in range(rounds):
        for name, k in (("off", None), ("every_step", 1), ("every_4th", 4)):
            sim.extremes = lane(k) if k else None               # a fresh configure: the state at its start values, the window starts here
            span_ms()
            t[name] += [span_ms() for _ in range(reps)]
            if k:
                sim.dev.extremes_configure([])
    sim.extremes = None
    out = {name: {"median_ms_per_step": float(np.median(v)), "min": float(np.min(v)), "max": float(np.max(v)), "spans": len(v)}
           for name, v in t.items()}
    out["one_sample_ms"] = out["every_step"]["median_ms_per_step"] - out["off"]["median_ms_per_step"]
    out["default_cadence_ms_per_step"] = out["every_4th"]["median_ms_per_step"] - out["off"]["median_ms_per_step"]
    out["default_cadence_share_of_step"] = out["default_cadence_ms_per_step"] / out["off"]["median_ms_per_step"]
    cells = n_lat * n_lon

    def launches_of(group, bytes_per_sample):
        sim.run_steps(n)
        sim.dev.timing(select=group)
        sim.run_steps(2 * n)
        sim.dev.sync()
        mean_ms, launches = sim.dev.timing_get(group)
        sim.dev.timing(on=False)
        total_ms = mean_ms * launches
        return {"per_sampled_step": launches / (2.0 * n), "mean_ms": mean_ms, "ms_per_sampled_step": total_ms / (2.0 * n),
                "bytes_per_sample": bytes_per_sample, "GBps": bytes_per_sample * 2.0 * n / (total_ms * 1e-3) / 1e9 if total_ms > 0 else None}
    # the launches alone, from the dispatches: this lane's, then the yardstick's
    sim.extremes = lane(1)
    names, nt, nh = sim.extremes.names, len(sim.extremes.thresholds), len(sim.extremes.hists)
    loads = sum((16 if e[0] == 1 else 8) + 16 for e in hs.entries_for(names)) + 16 * nt
    out["extremes_launches"] = launches_of("extremes", loads * cells)
    out["extremes_launches"]["bytes_are"] = "steady-state loads only (a lower bound: stores where a value changed are not counted)"
    state = sim.dev.extremes_read()
    out["closure"] = bool(all((h.sum(axis=1) == n_lon * state["n"]).all() for h in state["hist"]))
    sim.dev.extremes_configure([])
    sim.extremes = None
    cfg = {"enabled": True, "every_days": 1e6, "sample_every": 1, "fields": None}
    sim.history = hs.History(sim.dev, sim.grid, cfg, with_ocean=True, dt=float(sim.dt), day=sim.day_seconds, out=lambda s: None)
    per_sample = sum((16 + 16) if e[0] == 1 else (8 + 16) for e in hs.entries_for(sim.history.names)) * cells
    out["history_launches"] = launches_of("history", per_sample)
    sim.dev.history_configure([])
    sim.history = None
    out["copy_ceiling_GBps"] = sim.dev.copy_ceiling()
    out["entries"], out["thresholds"], out["histograms"], out["grid"], out["resources"] = len(names), nt, nh, [n_lat, n_lon], RESOURCES
    line = json.dumps(out)
    print(line)
    if args.out:
        with open(args.out, "w") as f:
            f.write(line + "\n")


if __name__ == "__main__":
    main()
