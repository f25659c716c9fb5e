"""Cost of one firing of the ecology, plankton and ISR figures (QD_FIGURES=1) at 181 x 360 and 721 x 1440, next to one state frame.

    python scripts/figures_cost.py

Runs the driver with the daily vegetation and plankton lanes (QD_ECO_DAILY=1, QD_PHYTO_DAILY=1; the LAI stack and the tracers are
resident) from its start-up state for a short spin-up, then times one firing of each figure up to, and without, the download of its
mosaic.  Two numbers per figure, each the median over `reps` repetitions after a warm-up:
  device_ms   the library's event pairs around its kernel groups (qd_timing: tiles_scan, tiles_select, tiles_render;
              stateframe_scan, stateframe_render for the yardstick), summed over the launches of one firing
  call_ms     wall time of the same calls from Python, each ending in a synchronise: the device time plus launches, the small
              result copies and the host's level rules
The plankton figure is species 0 and species 1 (two selects of two passes each: the count, then the two ranks).  Prints one JSON
line.  profiles/README.md and DESIGN.md section 7 quote the result."""
import json
import os
import sys
import time

import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, os.path.join(HERE, ".."))

ENV = {"QD_ECO_ENABLE": "1", "QD_ECO_DAILY": "1", "QD_ECO_DIAG": "0", "QD_PHYTO_ENABLE": "1", "QD_PHYTO_DAILY": "1", "QD_PHYTO_DIAG": "0",
       "QD_HYDRO_ENABLE": "0", "QD_AUTOSAVE_LOAD": "0"}
GROUPS = ("tiles_scan", "tiles_select", "tiles_render", "stateframe_scan", "stateframe_render")


def measure(dev, fn, reps):
    """-> {"device_ms", "call_ms"} of fn: medians over reps after two warm-up calls."""
    fn(), fn()
    dev.timing(True)
    ev, wall = [], []
    for _ in range(reps):
        dev.timing(True)                                        # resets the groups' totals
        t0 = time.perf_counter()
        fn()
        wall.append(1e3 * (time.perf_counter() - t0))
        ev.append(sum(ms * n for ms, n in (dev.timing_get(g) for g in GROUPS)))      # qd_timing_get: the mean per group and its count
    dev.timing(False)
    return {"device_ms": float(np.median(ev)), "call_ms": float(np.median(wall)), "call_min": float(np.min(wall)), "call_max": float(np.max(wall))}


def one_grid(n_lat, n_lon, reps):
    import qingdai_amd as qa
    from qingdai_amd import figures as fgm, stateframe as sfm
    from qingdai_amd.driver import Simulation
    sim = Simulation(n_lat, n_lon, params=qa.QdParams(), use_ocean=True, quiet=True)
    sim.bootstrap_ecology()
    sim.run_steps(12)
    sim.eco.banded_alpha()                                      # as a run past its first day boundary: the panel's host fallback is not timed
    dev = sim.dev
    fg = fgm.Figures(sim, env=dict(ENV))
    sf = sfm.StateFrame(sim, env={})
    sf.configure()
    e = sfm.read_env({})

    def ecology():
        _no_download(fg, "ecology")

    def plankton():
        _no_download(fg, "plankton0"), _no_download(fg, "plankton1")

    def isr():
        _no_download(fg, "isr")

    def state():
        scan = sfm.unpack_scan(*dev.stateframe_scan())
        dev.stateframe_render(sfm.pack_table(sfm.build_table(scan, e, ocean=True)))
    out = {"grid": [n_lat, n_lon], "species": int(sim.eco.pop.Ns), "layers": int(sim.eco.pop.K), "tracers": int(sim.phyto.S)}
    for name, fn in (("ecology", ecology), ("plankton", plankton), ("isr", isr), ("state_frame", state)):
        out[name] = measure(dev, fn, reps)
    dev.close()
    return out


def _no_download(fg, what):
    """One figure up to the render, without the download of the mosaic."""
    real = fg.dev.tiles_image
    fg.dev.tiles_image = lambda: None
    try:
        if what == "ecology":
            fg.ecology(1.0)
        elif what == "isr":
            fg.isr(1.0)
        else:
            fg.plankton(1.0, int(what[-1]))
    finally:
        fg.dev.tiles_image = real


def main():
    os.environ.update(ENV)
    out = {"reps": 20, "grids": [one_grid(181, 360, 20), one_grid(721, 1440, 20)]}
    print(json.dumps(out))


if __name__ == "__main__":
    main()
