#!/usr/bin/env python3
"""Drop-in for the reference's `python scripts/generate_topography.py` (P004): the procedural elevation, the land-sea mask
at the target land fraction and the base surface properties, built on the MI355X (qingdai_amd.topogen) and written to
data/topography_qingdai_{n_lat}x{n_lon}_seed{seed}_{UTC stamp}.nc with the reference's variables and attributes -- the file
QD_TOPO_NC loads.

Environment (the reference's names and defaults): QD_N_LAT 181, QD_N_LON 360, QD_SEED 42, QD_TARGET_LAND_FRAC 0.40,
QD_N_CONTINENTS 3, QD_CONT_SIGMA_DEG 30, QD_CONT_SHAPE_P 2, QD_CONT_MIN_DIST_DEG 40, QD_W_VLF 0.35, QD_FBM_OCTAVES 5,
QD_HURST_H 0.8, QD_W1 1.0, QD_W3 0.6, QD_SCALE_M 4500.  A value that does not parse is its default."""
import os
import sys
from datetime import datetime, timezone

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))

from qingdai_amd import topogen  # noqa: E402
from qingdai_amd.grid import SphericalGrid  # noqa: E402


def main(env=None):
    env = os.environ if env is None else env
    n_lat = topogen._env_value(env, "QD_N_LAT", int, 181)
    n_lon = topogen._env_value(env, "QD_N_LON", int, 360)
    seed, target, params = topogen.params_from_env(env)
    print(f"[Topo] Grid {n_lat}x{n_lon}, seed={seed}, target_land_frac={target}")
    print(f"[Topo] Params: {params}")
    grid = SphericalGrid(n_lat, n_lon)
    out = topogen.generate(grid, seed=seed, params=params, target_land_frac=target)
    print(f"[Topography] Target land fraction={target:.3f}, achieved={out['land_frac']:.3f}, sea_level={out['sea_level_m']:.1f} m")
    albedo, friction = topogen.base_properties(out["land_mask"], out["elevation"], grid)
    stamp = datetime.now(timezone.utc).strftime("%Y%m%dT%H%M%SZ")
    path = os.path.join("data", f"topography_qingdai_{n_lat}x{n_lon}_seed{seed}_{stamp}.nc")
    print(f"[Topo] Exporting to NetCDF: {path}")
    topogen.write_topography(path, grid, out["elevation"], out["land_mask"], albedo, friction, out["sea_level_m"])
    print("[Topo] Done.")
    return 0


if __name__ == "__main__":
    try:
        sys.exit(main())
    except Exception as e:      # noqa: BLE001
        print(f"[Topo] ERROR: {e}", file=sys.stderr)
        sys.exit(1)
