"""Cost of saving and restoring the vegetation state at 721 x 1440 with the default population (Ns = 20, K = 1).

    python scripts/eco_state_cost.py

Prints one JSON line: the wall time of one periodic autosave (Simulation.save_autosave) with QD_ECO_PERSIST at 0 -- the autosave as
it was before the switch existed --, 1 and 2, the size of the ecology file each level writes, and the wall time of one restore of the
resident stack from the file's one LAI plane through qd_eco_state_restore next to the host route it stands in for (the NumPy rule
of ecology.restore_layers, then the upload of the whole stack), with the bytes each route moves over the host link and on the
device, by arithmetic ("Saving and resuming the vegetation state")."""
import json
import os
import sys
import tempfile
import time

import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, os.path.join(HERE, ".."))


def best(fn, reps=3):
    out = []
    for _ in range(reps):
        t0 = time.perf_counter()
        fn()
        out.append(time.perf_counter() - t0)
    return 1e3 * min(out)


def main():
    from qingdai_amd.driver import Simulation
    from qingdai_amd.ecology import restore_layers, restore_weights
    for k in [k for k in os.environ if k.startswith("QD_ECO_")]:
        del os.environ[k]
    os.environ.update({"QD_ECO_DAILY": "1", "QD_ECO_DIAG": "0", "QD_ECO_INDIV_ENABLE": "0", "QD_PHYTO_ENABLE": "0", "QD_USE_OCEAN": "0"})
    n_lat, n_lon = 721, 1440
    sim = Simulation(n_lat=n_lat, n_lon=n_lon, quiet=True)
    pop, dev = sim.eco.pop, sim.dev
    S, K, cells = pop.Ns, pop.K, n_lat * n_lon
    res = {"grid": [n_lat, n_lon], "n_species": S, "n_layers": K}
    times = {0: [], 1: [], 2: []}
    with tempfile.TemporaryDirectory() as tmp:
        for rep in range(6):                                    # the three levels in turn, so that a busy host hits them alike
            for level in (0, 1, 2):
                os.environ["QD_ECO_PERSIST"] = str(level)
                out = os.path.join(tmp, f"level{level}")
                t0 = time.perf_counter()
                sim.save_autosave(out)
                times[level].append(1e3 * (time.perf_counter() - t0))
        for level in (0, 1, 2):
            p = os.path.join(tmp, f"level{level}", "ecology.nc")
            res[f"autosave_ms_persist{level}"] = min(times[level][1:])                # (the first round creates the directories)
            res[f"autosave_ms_persist{level}_median"] = float(np.median(times[level][1:]))
            res[f"ecology_nc_bytes_persist{level}"] = os.path.getsize(p) if os.path.exists(p) else 0
    res["autosave_added_ms_persist1"] = res["autosave_ms_persist1"] - res["autosave_ms_persist0"]
    res["autosave_added_ms_persist2"] = res["autosave_ms_persist2"] - res["autosave_ms_persist0"]
    # the restore: the file's f32 plane and weights
    rng = np.random.default_rng(2)
    lai = rng.uniform(0.0, 4.0, (n_lat, n_lon)).astype(np.float32)
    w = restore_weights(rng.uniform(0.1, 1.0, S).astype(np.float32))
    w64 = np.asarray(w, dtype=np.float64)
    dev.eco_state_restore(lai, w64, K, 5.0)
    n = 200                                                     # a window of many calls, each ending in a device synchronise
    t0 = time.perf_counter()
    for _ in range(n):
        dev.eco_state_restore(lai, w64, K, 5.0)
        dev.sync()
    res["restore_kernel_ms"] = 1e3 * (time.perf_counter() - t0) / n
    on_device = dev.eco_daily_get_layers(S, K)

    def host_route():
        stack = restore_layers(lai, w, K, 5.0)
        pop.push_layers(stack)
        dev.sync()
        return stack
    res["restore_host_route_ms"] = best(host_route)
    res["restore_host_rule_alone_ms"] = best(lambda: restore_layers(lai, w, K, 5.0))
    res["bitwise_equal_routes"] = bool(np.array_equal(on_device, dev.eco_daily_get_layers(S, K)))
    res["kernel_route_bytes_host_link"] = 4 * cells
    res["kernel_route_bytes_device"] = cells * (4 + 8 * S * K + 8)
    res["host_route_bytes_host_link"] = 2 * 8 * S * K * cells            # the plane-sum staging and the resident stack
    print(json.dumps(res))
    dev.close()


if __name__ == "__main__":
    main()
