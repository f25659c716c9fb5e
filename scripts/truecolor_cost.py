"""Cost of one true-colour frame at 721 x 1440 with every overlay on (16 ecology bands, 16 phytoplankton bands, rivers, lakes),
next to the path it replaces.

    rocprofv3 --kernel-trace --stats -d <dir> -- python scripts/truecolor_cost.py        # kernel times: k_truecolor, k_truecolor_final
    python scripts/truecolor_cost.py                                                     # wall times only

Prints one JSON line: the wall time of one render plus the download of the u8 image (3 bytes per cell), the device time of the
render's two launches from events, and the time to download what a user had to fetch to compose the frame on the host -- nine f64
fields, the flow map and the [16]-plane phytoplankton stack -- plus the bytes each path moves, by arithmetic (DESIGN.md section 7,
"True-colour frame").  Each timing is the median of `reps` repetitions after a warm-up; every timed call ends in a stream
synchronise."""
import json
import os
import sys
import time

import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, os.path.join(HERE, ".."))


def median_ms(fn, reps):
    fn()
    out = []
    for _ in range(reps):
        t0 = time.perf_counter()
        fn()
        out.append(1e3 * (time.perf_counter() - t0))
    return float(np.median(out)), float(np.min(out)), float(np.max(out))


def main():
    import qingdai_amd as qa
    from qingdai_amd import _lib
    from qingdai_amd.device import Device
    from qingdai_amd.topography import create_land_sea_mask
    n_lat, n_lon, nb, reps = 721, 1440, 16, 20
    shape = (n_lat, n_lon)
    grid = qa.SphericalGrid(n_lat, n_lon)
    mask = create_land_sea_mask(grid).astype(np.uint8)
    r = np.random.default_rng(1)
    dev = Device(grid)
    dev.upload_now("LAND_MASK", mask)
    fields = {"HICE": np.where(r.uniform(size=shape) < 0.8, 0.0, r.uniform(0.0, 2.0, shape)), "C_SNOW": r.uniform(0.0, 1.0, shape),
              "CLOUD": r.uniform(0.0, 1.0, shape), "TS": r.uniform(250.0, 300.0, shape), "ISR_A": r.uniform(0.0, 700.0, shape),
              "ISR_B": r.uniform(0.0, 300.0, shape), "ECO_F": r.uniform(0.0, 1.0, shape)}
    fields["ISR"] = fields["ISR_A"] + fields["ISR_B"]
    for k, a in fields.items():
        dev.upload_now(k, a)
    p = _lib.qd_truecolor_params(1, 1, 0, 1, 1, 1, 1, nb, nb, 0, 0.5, 0.15, 0.2, 0.6, 1.8, 1.35, 0.2, 2.2, 0.85, 273.15, 0.6, 0.95, 1e6, 0.45, 0.4)
    tab = r.uniform(0.05, 1.0, (7, nb))
    bands = r.uniform(0.0, 0.3, (nb,) + shape)
    flow = 10.0 ** r.uniform(3.0, 8.0, shape)
    dev.truecolor_configure(p, tab, tab[1:], bands, (r.uniform(size=shape) < 0.05).astype(np.uint8))
    dev.truecolor_render(flow=flow)                             # the flow map is staged once; the timed renders read it where it lies

    def frame():
        dev.truecolor_render(flow=flow)
        return dev.truecolor_image()
    t_frame = median_ms(frame, reps)
    dev.timing(True)
    for _ in range(reps):
        dev.truecolor_render(flow=flow)
    dev_ms, n_timed = dev.timing_get("truecolor")
    dev.timing(False)
    t_img = median_ms(dev.truecolor_image, reps)

    def old_way():
        for k in ("HICE", "C_SNOW", "CLOUD", "TS", "ISR", "ISR_A", "ISR_B", "ECO_F"):
            dev._host.pop(k, None)
            dev.get(k)
        dev._host.pop("LAND_MASK", None)
        dev.get("LAND_MASK")
        return dev.truecolor_rgb()                             # stands in for the [16]-plane stack and the flow map: 3 of their 17 planes
    dev.truecolor_render(want_f64=True, flow=flow)
    t_old = median_ms(old_way, max(3, reps // 4))
    cells = n_lat * n_lon
    planes_old = 8 + 3
    print(json.dumps({
        "grid": [n_lat, n_lon], "nb_eco": nb, "nb_phyto": nb, "reps": reps,
        "wall_ms_render_plus_u8_download": {"median": t_frame[0], "min": t_frame[1], "max": t_frame[2]},
        "wall_ms_u8_download": {"median": t_img[0], "min": t_img[1], "max": t_img[2]},
        "device_ms_render_two_launches": dev_ms, "device_timed_launch_groups": n_timed,
        "wall_ms_download_inputs_f64": {"median": t_old[0], "min": t_old[1], "max": t_old[2], "planes_downloaded": planes_old,
                                        "planes_a_user_needs": 8 + 1 + nb, "scaled_to_needed_planes_ms": t_old[0] * (8 + 1 + nb) / planes_old},
        "bytes_kernel_reads": cells * (8 * (8 + 1 + nb) + 2), "bytes_kernel_writes": cells * 3,
        "bytes_over_host_link_frame": cells * 3, "bytes_over_host_link_inputs": cells * (8 * (8 + 1 + nb) + 1)}))
    dev.close()


if __name__ == "__main__":
    main()
