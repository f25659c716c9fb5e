"""Cost of the per-step series lane (QD_SERIES=1) at 721 x 1440, next to the history launch for the same entries and the step.

    python scripts/series_cost.py [--out profiles/series_cost.json]

Runs the driver's flag set with full physics and the ocean (no ecology, tracers or routing) from the bench's resting state with the
default field list (23 entries with the ocean), prints one JSON line and writes it to --out:
  * ms per step with both lanes off and with the series lane sampling every step -- medians over `reps` spans of `n` steps after a
    warm-up span, every span ending in a synchronise, the two cases interleaved `rounds` times;
  * the device time of the series launches (timing group "series") and of k_hist_accum (group "history") for the same entries, taken
    from the dispatches themselves with both lanes sampling every step of the same run, the two groups selected in turn `rounds`
    times; the series' achieved read GB/s, counting 8 bytes per source plane and cell (an op-1 entry reads two);
  * the device's copy ceiling (qd_copy_ceiling, what `bench.py --full` reports), and the ratio;
  * series_not_slower_than_history: the one structural condition -- the series launch reads each plane once where the history launch
    moves three planes' worth of bytes per entry, so it must not take longer.
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
    from qingdai_amd import history as hs, series as sr
    from qingdai_amd.driver import Simulation
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=os.path.join(HERE, "..", "profiles", "series_cost.json"))
    ap.add_argument("--grid", default="721x1440")
    args = ap.parse_args()
    n_lat, n_lon = (int(x) for x in args.grid.split("x"))
    n, reps, rounds = 20, 5, 3
    sim = Simulation(n_lat, n_lon, params=qa.QdParams(), use_ocean=True, quiet=True, ecology=False, individuals=False, phyto=False)
    sim.routing = None
    quiet = lambda s: None
    s_cfg = {"enabled": True, "every": 1, "zonal": True, "every_days": 1e6, "fields": None}        # one window: nothing is written
    h_cfg = {"enabled": True, "every_days": 1e6, "sample_every": 1, "fields": None}
    new_series = lambda: sr.Series(sim.dev, sim.grid, s_cfg, with_ocean=True, dt=float(sim.dt), day=sim.day_seconds, out=quiet)
    new_history = lambda: hs.History(sim.dev, sim.grid, h_cfg, with_ocean=True, dt=float(sim.dt), day=sim.day_seconds, out=quiet)

    def span_ms():
        sim.dev.sync()
        t0 = time.perf_counter()
        sim.run_steps(n)
        sim.dev.sync()
        if sim.series is not None:
            sim.series.drop()                                   # the records were delivered; this run keeps none
        return 1e3 * (time.perf_counter() - t0) / n
    sim.run_steps(40)                                           # spin-up: past the first steps' transients
    t = {"off": [], "every_step": []}
    for _ in range(rounds):
        for name in ("off", "every_step"):
            sim.series = new_series() if name == "every_step" else None
            span_ms()
            t[name] += [span_ms() for _ in range(reps)]
            if sim.series is not None:
                sim.dev.series_configure([], 0, None)
                sim.series = None
    out = {name: {"median_ms_per_step": float(np.median(v)), "min": float(np.min(v)), "max": float(np.max(v))} for name, v in t.items()}
    out["one_sample_ms"] = out["every_step"]["median_ms_per_step"] - out["off"]["median_ms_per_step"]
    # the launches alone, from the dispatches: both lanes on the same entries in the same run, the two groups timed in turn
    sim.series, sim.history = new_series(), new_history()
    names = sim.series.names
    assert names == sim.history.names
    sim.run_steps(n)
    sim.series.drop()
    got = {"series": [], "history": []}
    for _ in range(rounds):
        for group in ("series", "history"):
            sim.dev.timing(select=group)
            sim.run_steps(2 * n)
            sim.dev.sync()
            sim.series.drop()
            mean_ms, launches = sim.dev.timing_get(group)
            got[group].append((mean_ms * launches / (2.0 * n), launches / (2.0 * n)))
    sim.dev.timing(on=False)
    cells = n_lat * n_lon
    read_bytes = sum(16 if e[0] == 1 else 8 for e in hs.entries_for(names)) * cells
    for group in got:
        ms = [a for a, _ in got[group]]
        out[group + "_launches"] = {"per_sampled_step": got[group][0][1], "ms_per_sampled_step": float(np.median(ms)),
                                    "min": float(np.min(ms)), "max": float(np.max(ms))}
    s_ms, h_ms = out["series_launches"]["ms_per_sampled_step"], out["history_launches"]["ms_per_sampled_step"]
    out["series_launches"]["read_bytes_per_sample"] = read_bytes
    out["series_launches"]["read_GBps"] = read_bytes / (s_ms * 1e-3) / 1e9 if s_ms > 0 else None
    out["history_launches"]["bytes_per_sample"] = read_bytes + 16 * len(names) * cells       # the sources, and every sum read and written
    out["series_not_slower_than_history"] = bool(0 < s_ms <= h_ms)
    out["copy_ceiling_GBps"] = sim.dev.copy_ceiling()
    if out["series_launches"]["read_GBps"]:
        out["fraction_of_copy_ceiling"] = out["series_launches"]["read_GBps"] / out["copy_ceiling_GBps"]
    out["entries"], out["grid"], out["record_doubles"] = len(names), [n_lat, n_lon], sim.series.width
    text = json.dumps(out)
    print(text)
    os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
    with open(args.out, "w", encoding="utf-8") as f:
        f.write(text + "\n")


if __name__ == "__main__":
    main()
