"""Cost of the drifter lane (QD_DRIFTERS=1) at 721 x 1440 (BASELINE.json configs[2]): the step with the lane off and on.

    python scripts/drifters_cost.py [--out profiles/drifters_cost.json]

Runs the driver's flag set with full physics and the ocean (no ecology, tracers or routing) from the bench's resting state, prints
one JSON line and writes it to --out.  For the default counts (4096 + 4096 seeds, the ocean's over ocean cells) and for 2^20 + 2^20
particles, with the default samples (TS, H / SST) and the default cadence (a record every 24th step):
  * ms per step with the lane off and with it on, in the same process -- medians over `reps` spans of `n` steps after a warm-up
    span, every span ending in a synchronise and (lane on) the drain of its records, the two cases interleaved `rounds` times;
  * the device time of the lane's launch (timing group "drifters") from the dispatches themselves, and the launches per step:
    the one structural condition is exactly one launch per step with the lane on and none with it off.
DESIGN.md quotes the result."""
import argparse
import json
import os
import sys
import time

import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, os.path.join(HERE, ".."))


def main():
    import qingdai_amd as qa
    from qingdai_amd import drifters as dr
    from qingdai_amd.driver import Simulation
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=os.path.join(HERE, "..", "profiles", "drifters_cost.json"))
    ap.add_argument("--grid", default="721x1440")
    args = ap.parse_args()
    n_lat, n_lon = (int(x) for x in args.grid.split("x"))
    n, reps, rounds = 24, 5, 3
    sim = Simulation(n_lat, n_lon, params=qa.QdParams(), use_ocean=True, quiet=True, ecology=False, individuals=False, phyto=False)
    sim.routing = None
    quiet = lambda s: None
    cfg = dr.default_config(every_days=1e6)                       # one window: nothing is written
    big = 1 << 20
    wet = dr.seed_fibonacci(2 * big, sim.grid, sim.land_mask)
    seeds = {"default": None,
             "2^20+2^20": (dr.to_degrees(*dr.seed_fibonacci(big, sim.grid), n_lat, n_lon),
                           dr.to_degrees(wet[0][:big], wet[1][:big], n_lat, n_lon))}

    def new_lane(case):
        s = seeds[case]
        return dr.Drifters(sim, cfg=cfg, out=quiet) if s is None else dr.Drifters(sim, atm=s[0], ocn=s[1], cfg=cfg, out=quiet)

    def release():
        sim.dev.drift_configure(None, None, [], [], None)
        sim.drifters = None

    def span_ms():
        sim.dev.sync()
        t0 = time.perf_counter()
        sim.run_steps(n)
        sim.dev.sync()
        ms = 1e3 * (time.perf_counter() - t0) / n
        if sim.drifters is not None:
            sim.drifters.drop()                                 # the records were delivered; this run keeps none
        return ms
    sim.run_steps(40)                                           # spin-up: past the first steps' transients
    out = {"grid": [n_lat, n_lon], "steps_per_span": n, "record_every": int(cfg["every"])}
    for case in seeds:
        t = {"off": [], "on": []}
        for _ in range(rounds):
            for name in ("off", "on"):
                sim.drifters = new_lane(case) if name == "on" else None
                span_ms()
                t[name] += [span_ms() for _ in range(reps)]
                if sim.drifters is not None:
                    counts, width, cap = dict(sim.drifters.n), sim.drifters.width, sim.drifters.device_cap
                    release()
        res = {name: {"median_ms_per_step": float(np.median(v)), "min": float(np.min(v)), "max": float(np.max(v))} for name, v in t.items()}
        res["lane_ms_per_step"] = res["on"]["median_ms_per_step"] - res["off"]["median_ms_per_step"]
        res["particles"], res["record_doubles"], res["log_cap"] = counts, width, cap
        # the launch alone, from the dispatches; and the launch count with the lane off
        sim.dev.timing(select="drifters")
        sim.run_steps(n)
        sim.dev.sync()
        before = sim.dev.timing_get("drifters")[1]
        sim.drifters = new_lane(case)
        sim.run_steps(2 * n)
        sim.dev.sync()
        sim.drifters.drop()
        mean_ms, launches = sim.dev.timing_get("drifters")
        sim.dev.timing(on=False)
        release()
        res["kernel"] = {"launches_per_step_off": before / float(n), "launches_per_step_on": (launches - before) / (2.0 * n),
                         "mean_ms_per_launch": float(mean_ms)}
        res["one_launch_per_step"] = bool(before == 0 and launches == 2 * n)
        out[case] = res
    text = json.dumps(out)
    print(text)
    os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
    with open(args.out, "w", encoding="utf-8") as f:
        f.write(text + "\n")


if __name__ == "__main__":
    main()
