"""Cost of the procedural planet at 721 x 1440 (and, with --big, 1441 x 2880): the host recipe it can replace, the device build end
to end, and what the device build is made of.

    python scripts/topogen_cost.py [--big] [--big-host] [--reps N] [--out profiles/topogen_cost.json]

Per grid, three times:
  host_s        qingdai_amd.topography.create_land_sea_mask -- the NumPy tap loop every driver start paid (one run; at
                1441 x 2880 only with --big-host: it takes minutes)
  device_s      qingdai_amd.topogen.generate end to end on an existing handle: the host draws, the tables and weights, the
                uploads, the kernels, the downloads (median of `reps` after a warm-up)
  kernels_ms    the kernels alone, by events around them (qd_topogen_last_ms), next to draws_s, the host random draws alone
The draws are unchanged host work and are the floor of the device path.  Also recorded: whether the device mask equals the
host's and the largest elevation difference.  Writes the JSON and prints the rows of the DESIGN.md table."""
import argparse
import json
import os
import sys
import time

import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, os.path.join(HERE, ".."))


def measure(n_lat, n_lon, reps, host):
    import qingdai_amd as qa
    from qingdai_amd import topogen
    from qingdai_amd.device import Device
    from qingdai_amd.topography import create_land_sea_mask
    grid = qa.SphericalGrid(n_lat, n_lon)
    dev = Device(grid)
    timing = {}
    topogen.generate(grid, dev=dev, timing=timing)                     # warm-up: code objects, first allocations
    wall, kern, draws = [], [], []
    for _ in range(reps):
        t0 = time.perf_counter()
        out = topogen.generate(grid, dev=dev, timing=timing)
        wall.append(time.perf_counter() - t0)
        kern.append(timing["kernels_ms"])
        t0 = time.perf_counter()
        topogen.draw(grid, 42)
        draws.append(time.perf_counter() - t0)
    dev.close()
    rec = {"grid": [n_lat, n_lon], "reps": reps, "device_s": float(np.median(wall)), "device_s_min_max": [min(wall), max(wall)],
           "kernels_ms": float(np.median(kern)), "kernels_ms_min_max": [min(kern), max(kern)], "draws_s": float(np.median(draws)),
           "sea_level_m": out["sea_level_m"], "land_frac": out["land_frac"]}
    if host:
        t0 = time.perf_counter()
        mask, elev = create_land_sea_mask(grid, return_elevation=True)
        rec["host_s"] = time.perf_counter() - t0
        rec["mask_equal_host"] = bool(np.array_equal(mask, out["land_mask"]))
        rec["max_abs_elevation_diff_m"] = float(np.max(np.abs(elev - out["elevation"])))
        rec["speedup_end_to_end"] = rec["host_s"] / rec["device_s"]
    rec["kernels_below_draws"] = bool(rec["kernels_ms"] * 1e-3 < rec["draws_s"])
    return rec


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--big", action="store_true", help="also 1441 x 2880 (device side)")
    ap.add_argument("--big-host", action="store_true", help="with --big: time the host recipe there too (minutes)")
    ap.add_argument("--reps", type=int, default=5)
    ap.add_argument("--out", default=os.path.join(HERE, "..", "profiles", "topogen_cost.json"))
    a = ap.parse_args()
    recs = [measure(721, 1440, a.reps, True)]
    if a.big:
        recs.append(measure(1441, 2880, max(2, a.reps // 2), a.big_host))
    os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
    with open(a.out, "w") as fh:
        json.dump({"what": "scripts/topogen_cost.py", "grids": recs}, fh, indent=1)
        fh.write("\n")
    print("| grid | host recipe | device build, end to end | host draws alone | kernels alone (events) | speed-up |")
    print("|---|---|---|---|---|---|")
    for r in recs:
        host = f"{r['host_s']:.2f} s" if "host_s" in r else "not run"
        up = f"{r['speedup_end_to_end']:.0f}x" if "host_s" in r else "-"
        print(f"| {r['grid'][0]}x{r['grid'][1]} | {host} | {r['device_s']:.3f} s | {r['draws_s']:.3f} s | {r['kernels_ms']:.2f} ms | {up} |")
    print(json.dumps(recs))


if __name__ == "__main__":
    main()
