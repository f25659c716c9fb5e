"""Cost of one firing of the budget diagnostics lane (QD_BUDGET_DIAG=1) at 721 x 1440, next to the step it rides on.

    python scripts/budget_diag_cost.py

Runs the driver's flag set (ocean, driver physics, hydrology commit; no ecology, tracers or routing) from the bench's resting
state and prints one JSON line: ms per step of spans in which no step fires, ms per step of equally long spans in which EVERY step
fires both cadences (all six positions: ten extra launches and the un-hoisted precipitation block), and their difference = the
cost of one firing.  Each figure is the median over `reps` spans of `n` steps after a warm-up span; every span ends in a
synchronise.  profiles/README.md and DESIGN.md section 7 quote the result."""
import json
import os
import sys
import time

import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, os.path.join(HERE, ".."))


def main():
    import qingdai_amd as qa
    from qingdai_amd import budget_diag as bd
    from qingdai_amd.driver import Simulation
    n_lat, n_lon, n, reps = 721, 1440, 20, 7
    sim = Simulation(n_lat, n_lon, params=qa.QdParams(), use_ocean=True, quiet=True, ecology=False, individuals=False, phyto=False)
    sim.routing = None
    fire = {"v": 0}

    class Every(bd.BudgetDiag):
        def span_schedule(self, t0, dt, k):
            f = np.full(k, fire["v"], dtype=np.int32)
            self.dev.budget_diag_schedule(f)
            return [(self.i + s, int(f[s])) for s in np.flatnonzero(f)], int(k)
    sim.budget = Every(sim.dev, sim.grid, {}, with_ocean=True, routed=False, out=lambda s: None)

    def span_ms():
        sim.dev.sync()
        t0 = time.perf_counter()
        sim.run_steps(n)
        sim.dev.sync()
        return 1e3 * (time.perf_counter() - t0) / n
    sim.run_steps(40)                                           # spin-up: past the first steps' transients
    out = {}
    for name, v in (("off", 0), ("firing", 3), ("off_again", 0)):
        fire["v"] = v
        span_ms()
        t = [span_ms() for _ in range(reps)]
        out[name] = {"median_ms_per_step": float(np.median(t)), "min": float(np.min(t)), "max": float(np.max(t))}
    out["one_firing_ms"] = out["firing"]["median_ms_per_step"] - 0.5 * (out["off"]["median_ms_per_step"] + out["off_again"]["median_ms_per_step"])
    out["amortised_over_200_steps_ms_per_step"] = out["one_firing_ms"] / 200.0
    out["grid"] = [n_lat, n_lon]
    print(json.dumps(out))


if __name__ == "__main__":
    main()
