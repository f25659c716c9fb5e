"""Cost of the time-mean history lane (QD_HISTORY=1) at 721 x 1440, next to the step it rides on.

    python scripts/history_cost.py

Runs the driver's flag set with full physics and the ocean (no ecology, tracers or routing) from the bench's resting state, the
default field list (23 entries with the ocean), and prints one JSON line:
  * ms per step with the lane off, with every step sampled and with every fourth step sampled -- medians over `reps` spans of `n`
    steps after a warm-up span, every span ending in a synchronise, the three cases interleaved `rounds` times;
  * the device time of the accumulate launches from the library's timing group "history" (taken from the dispatches themselves) in a
    run of its own, and their achieved GB/s, counting 8 bytes per source read and 16 per sum (read and written);
  * the device's copy ceiling (qd_copy_ceiling, what `bench.py --full` reports), and the ratio.
profiles/README.md and DESIGN.md section 7 quote the result."""
import json
import os
import sys
import time

import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, os.path.join(HERE, ".."))


def main():
    import qingdai_amd as qa
    from qingdai_amd import history as hs
    from qingdai_amd.driver import Simulation
    n_lat, n_lon, n, reps, rounds = 721, 1440, 20, 5, 3
    sim = Simulation(n_lat, n_lon, params=qa.QdParams(), use_ocean=True, quiet=True, ecology=False, individuals=False, phyto=False)
    sim.routing = None
    lanes = {}
    for k in (1, 4):
        cfg = {"enabled": True, "every_days": 1e6, "sample_every": k, "fields": None}       # one window: nothing is written
        lanes[k] = lambda cfg=cfg: hs.History(sim.dev, sim.grid, cfg, with_ocean=True, dt=float(sim.dt), day=sim.day_seconds, out=lambda s: None)

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
            sim.history = lanes[k]() if k else None             # a fresh configure: sums zeroed, the window starts here
            span_ms()
            t[name] += [span_ms() for _ in range(reps)]
            if k:
                sim.dev.history_configure([])
    out = {name: {"median_ms_per_step": float(np.median(v)), "min": float(np.min(v)), "max": float(np.max(v))} for name, v in t.items()}
    out["one_sample_ms"] = out["every_step"]["median_ms_per_step"] - out["off"]["median_ms_per_step"]
    # the launches alone, from the dispatches
    sim.history = lanes[1]()
    names = sim.history.names
    sim.run_steps(n)
    sim.dev.timing(select="history")
    sim.run_steps(2 * n)
    sim.dev.sync()
    mean_ms, launches = sim.dev.timing_get("history")
    sim.dev.timing(on=False)
    cells = n_lat * n_lon
    per_sample = sum((16 + 16) if e[0] == 1 else (8 + 16) for e in hs.entries_for(names)) * cells
    total_ms = mean_ms * launches
    out["launches"] = {"per_sampled_step": launches / (2.0 * n), "mean_ms": mean_ms, "ms_per_sampled_step": total_ms / (2.0 * n),
                       "bytes_per_sample": per_sample, "GBps": per_sample * 2.0 * n / (total_ms * 1e-3) / 1e9 if total_ms > 0 else None}
    out["copy_ceiling_GBps"] = sim.dev.copy_ceiling()
    if out["launches"]["GBps"]:
        out["fraction_of_copy_ceiling"] = out["launches"]["GBps"] / out["copy_ceiling_GBps"]
    out["entries"], out["grid"] = len(names), [n_lat, n_lon]
    print(json.dumps(out))


if __name__ == "__main__":
    main()
