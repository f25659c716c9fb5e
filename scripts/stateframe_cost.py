"""Cost of one state frame (QD_STATE_PLOT=1) at 721 x 1440, by part, next to the host route it replaces.

    python scripts/stateframe_cost.py

Runs the driver's flag set (ocean, driver physics, hydrology commit; no ecology, tracers or routing) from the bench's resting state
for a spin-up, then times, each as the median over `reps` repetitions after a warm-up and each ending in a synchronise:
  scan      qd_stateframe_scan (two launches, 30 doubles back)
  table     the host's level rules and band colours (stateframe.build_table + pack_table)
  render    qd_stateframe_render (the table upload, the memset, one launch)
  download  the u8 mosaic to the host
  frame     all four, as StateFrame.render does them
  png       the PNG and the JSON sidecar written to a temporary directory (host only)
and the host route: dev.get of the seventeen planes the figure reads plus tests/stateframe_ref.py (fields, scan, table, render) on
one core.  Prints one JSON line.  profiles/README.md and DESIGN.md section 7 quote the result."""
import json
import os
import sys
import tempfile
import time

import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, os.path.join(HERE, ".."))
sys.path.insert(0, os.path.join(HERE, "..", "tests"))


def med(fn, reps):
    fn()
    t = []
    for _ in range(reps):
        t0 = time.perf_counter()
        fn()
        t.append(1e3 * (time.perf_counter() - t0))
    return {"median_ms": float(np.median(t)), "min": float(np.min(t)), "max": float(np.max(t))}


def main():
    import qingdai_amd as qa
    import stateframe_ref as ref
    from qingdai_amd import stateframe as sfm
    from qingdai_amd.driver import Simulation
    n_lat, n_lon, reps = 721, 1440, 20
    sim = Simulation(n_lat, n_lon, params=qa.QdParams(), use_ocean=True, quiet=True, ecology=False, individuals=False, phyto=False)
    sim.routing = None
    sim.run_steps(40)                                           # spin-up: past the first steps' transients
    dev = sim.dev
    sf = sfm.StateFrame(sim, env={})
    sf.configure()
    e = sfm.read_env({})
    state = {}

    def scan():
        state["scan"] = sfm.unpack_scan(*dev.stateframe_scan())

    def table():
        state["tab"] = sfm.build_table(state["scan"], e, ocean=True)
        state["packed"] = sfm.pack_table(state["tab"])

    def render():
        dev.stateframe_render(state["packed"])

    def download():
        state["img"] = dev.stateframe_image()

    out = {"grid": [n_lat, n_lon], "reps": reps}
    for name, fn in (("scan", scan), ("table", table), ("render", render), ("download", download), ("frame", sf.render)):
        out[name] = med(fn, reps)
    with tempfile.TemporaryDirectory() as tmp:
        out["frame_and_files"] = med(lambda: sf.write_frame(12.25, tmp), 5)
    names = list(ref.INPUTS)

    def host_get():
        for k in names:
            dev._host.pop(k, None)
        state["inp"] = {ref.INPUTS[k]: dev.get(k) for k in names}
        state["inp"]["land_mask"] = sim.land_mask

    def host_draw():
        F = ref.fields(state["inp"], sim.grid.lat, ocean=True, p0=dev.params.p0, rho_a=dev.params.rho_a, H=dev.params.H)
        tab = sfm.build_table(ref.scan(F, state["inp"]["isr_A"], state["inp"]["isr_B"]), e, ocean=True)
        state["host_img"] = ref.render(F, tab, sim.land_mask)[1]

    out["host_get_planes"] = med(host_get, 5)
    out["host_restatement_one_core"] = med(host_draw, 3)
    out["host_route_ms"] = out["host_get_planes"]["median_ms"] + out["host_restatement_one_core"]["median_ms"]
    out["planes_pulled_by_the_host_route"] = len(names)
    sf.render()
    out["pixels_differing_between_host_and_device_mosaic"] = int(np.any(state["host_img"] != dev.stateframe_image(), axis=-1).sum())
    print(json.dumps(out))


if __name__ == "__main__":
    main()
