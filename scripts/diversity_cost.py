"""Cost of one diversity firing at 721 x 1440, Ns = 20, K = 2 on the resident stack, next to the path it replaces.

    rocprofv3 --kernel-trace --stats -d <dir> -- python scripts/diversity_cost.py        # kernel times: k_div_alpha, k_div_bc, k_div_final
    python scripts/diversity_cost.py                                                     # wall times only

Prints one JSON line: the wall time of PopulationCanopy.diversity() (three launches + the download of the two maps and L_s), of the
device call alone (no map download), and of the old way to look at the community -- qd_eco_daily_get_layers (332 MB over the host
link) followed by the NumPy restatement tests/diversity_ref.py -- plus the bytes each kernel moves, by arithmetic (DESIGN.md
section 7, "Diversity diagnostics")."""
import json
import os
import sys
import time

import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, os.path.join(HERE, ".."))
sys.path.insert(0, os.path.join(HERE, "..", "tests"))


def main():
    import qingdai_amd as qa
    import diversity_ref as ref
    from qingdai_amd.device import Device
    from qingdai_amd.ecology import EcologyAdapter, PopulationDaily, diversity_weights
    from qingdai_amd.topography import create_land_sea_mask
    n_lat, n_lon, S, K = 721, 1440, 20, 2
    os.environ.update({"QD_ECO_NS": str(S), "QD_ECO_COHORT_K": str(K)})
    grid = qa.SphericalGrid(n_lat, n_lon)
    mask = create_land_sea_mask(grid).astype(np.uint8)
    dev = Device(grid)
    dev.upload_now("LAND_MASK", mask)
    pop = EcologyAdapter(grid, mask, dev=dev, albedo_couple=True).pop
    PopulationDaily(pop)
    stack = np.random.default_rng(1).uniform(0.0, 0.3, (S, K, n_lat, n_lon)) * (mask == 1)
    pop.push_layers(stack, init=True)
    w = diversity_weights(grid.lat_mesh, mask == 1)
    dev.eco_diversity(w, n_species=S, n_layers=K)              # first use allocates
    reps = 5
    t0 = time.perf_counter()
    for _ in range(reps):
        summary = dev.eco_diversity(w, n_species=S, n_layers=K)
    t_call = (time.perf_counter() - t0) / reps
    t0 = time.perf_counter()
    alpha, bc, L_s, summary = pop.diversity()
    t_full = time.perf_counter() - t0
    t0 = time.perf_counter()
    layers = dev.eco_daily_get_layers(S, K)
    t_get = time.perf_counter() - t0
    t0 = time.perf_counter()
    want = ref.diversity(layers, mask, grid.lat_mesh)
    t_ref = time.perf_counter() - t0
    same = bool(np.array_equal(want["L_s"], L_s) and np.array_equal(want["bc_local"], bc, equal_nan=True))
    cells = n_lat * n_lon
    rs, tc = 8, 62                                              # QD_DIV_RS, QD_DIV_TC of qd_eco_div.hip
    print(json.dumps({
        "grid": [n_lat, n_lon], "n_species": S, "n_layers": K, "bitwise_L_s_and_bc": same,
        "wall_ms_device_call": 1e3 * t_call, "wall_ms_diversity_with_downloads": 1e3 * t_full,
        "wall_ms_get_layers": 1e3 * t_get, "wall_ms_numpy_restatement": 1e3 * t_ref,
        "bytes_k_div_alpha": cells * (8 * S * K + 8 * S + 8 + 1), "bytes_k_div_bc": int(cells * (8 * S * (rs + 2) / rs * 64 / tc + 8 + 1)),
        "summary": summary}))
    dev.close()


if __name__ == "__main__":
    main()
