"""Cost of the zonal spectra lane (QD_SPECTRA=1) at 721 x 1440, next to the step and to a series sample.

    python scripts/spectra_cost.py [--out profiles/spectra_cost.json]

Runs the driver's flag set with full physics and the ocean (no ecology, tracers or routing) from the bench's resting state with the
default field list (U, V, H, Q, CLOUD), prints one JSON line and writes it to --out:
  * ms per step with the lane off and with the lane sampling every step -- medians over `reps` x `rounds` = 15 spans of `n` = 20
    steps after a warm-up span, every span ending in a synchronise, the cases interleaved `rounds` times -- for the default form
    (the FFT) and for QD_SPECTRA_FORM=direct, each with QD_SPECTRA_LAT on and off; the difference to "off" is one sample's cost;
  * the device time of k_spectra_rows (timing group "spectra") and of k_spectra_combine (group "spectra_combine"), taken from the
    dispatches themselves, per form; the rows kernel's achieved read GB/s, counting 8 bytes per source plane and cell, against the
    device's copy ceiling (qd_copy_ceiling, what `bench.py --full` reports) of the same run;
  * the amortised cost per step at the default cadence (one sample in 24 steps), beside a series sample (profiles/series_cost.json);
  * fft_is_faster: the structural condition -- the default form must be the faster of the two at this grid.
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
    from qingdai_amd import history as hs, spectra as sp
    from qingdai_amd.driver import Simulation
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=os.path.join(HERE, "..", "profiles", "spectra_cost.json"))
    ap.add_argument("--grid", default="721x1440")
    ap.add_argument("--skip-direct", action="store_true", help="leave the direct form out (a quick look)")
    args = ap.parse_args()
    n_lat, n_lon = (int(x) for x in args.grid.split("x"))
    n, reps, rounds = 20, 5, 3
    sim = Simulation(n_lat, n_lon, params=qa.QdParams(), use_ocean=True, quiet=True, ecology=False, individuals=False, phyto=False)
    sim.routing = None
    quiet = lambda s: None

    def new_spectra(form, lat):
        """The form is read by the configure call, once."""
        if form == "direct":
            os.environ["QD_SPECTRA_FORM"] = "direct"
        else:
            os.environ.pop("QD_SPECTRA_FORM", None)
        cfg = {"enabled": True, "every": 1, "lat": lat, "every_days": 1e6, "fields": None}      # one window: nothing is written
        try:
            return sp.Spectra(sim.dev, sim.grid, cfg, with_ocean=True, dt=float(sim.dt), day=sim.day_seconds, out=quiet)
        finally:
            os.environ.pop("QD_SPECTRA_FORM", None)

    def span_ms():
        sim.dev.sync()
        t0 = time.perf_counter()
        sim.run_steps(n)
        sim.dev.sync()
        if sim.spectra is not None:
            sim.spectra.drop()                                  # the records were delivered; this run keeps none
        return 1e3 * (time.perf_counter() - t0) / n
    sim.run_steps(40)                                           # spin-up: past the first steps' transients
    forms = ("fft",) if args.skip_direct else ("fft", "direct")
    cases = [("off", None, None)] + [(f"{form}_lat{lat}", form, bool(lat)) for form in forms for lat in (1, 0)]
    t = {name: [] for name, _, _ in cases}
    for _ in range(rounds):
        for name, form, lat in cases:
            sim.spectra = new_spectra(form, lat) if form else None
            span_ms()
            t[name] += [span_ms() for _ in range(reps)]
            if sim.spectra is not None:
                sim.dev.spectra_configure([], 0, None)
                sim.spectra = None
    out = {name: {"median_ms_per_step": float(np.median(v)), "min": float(np.min(v)), "max": float(np.max(v))} for name, v in t.items()}
    off = out["off"]["median_ms_per_step"]
    out["one_sample_ms"] = {name: out[name]["median_ms_per_step"] - off for name in t if name != "off"}
    # the launches alone, from the dispatches, per form
    names = list(sp.DEFAULT_FIELDS)
    cells = n_lat * n_lon
    read_bytes = sum(16 if e[0] == 1 else 8 for e in hs.entries_for(names)) * cells
    out["launches"] = {}
    for form in forms:
        sim.spectra = new_spectra(form, True)
        sim.run_steps(n)
        sim.spectra.drop()
        got = {"spectra": [], "spectra_combine": []}
        for _ in range(rounds):
            for group in got:
                sim.dev.timing(select=group)
                sim.run_steps(n)
                sim.dev.sync()
                sim.spectra.drop()
                mean_ms, launches = sim.dev.timing_get(group)
                got[group].append((mean_ms * launches / float(n), launches / float(n)))
        sim.dev.timing(on=False)
        rows_ms = float(np.median([a for a, _ in got["spectra"]]))
        comb_ms = float(np.median([a for a, _ in got["spectra_combine"]]))
        out["launches"][form] = {"k_spectra_rows_ms": rows_ms, "k_spectra_combine_ms": comb_ms, "per_sampled_step": got["spectra"][0][1] +
                                 got["spectra_combine"][0][1], "read_bytes_per_sample": read_bytes,
                                 "rows_read_GBps": read_bytes / (rows_ms * 1e-3) / 1e9 if rows_ms > 0 else None}
        sim.dev.spectra_configure([], 0, None)
        sim.spectra = None
    out["copy_ceiling_GBps"] = sim.dev.copy_ceiling()
    for form in forms:
        g = out["launches"][form]["rows_read_GBps"]
        if g:
            out["launches"][form]["fraction_of_copy_ceiling"] = g / out["copy_ceiling_GBps"]
    out["default_cadence"] = {"every": sp.EVERY, "amortised_ms_per_step": out["one_sample_ms"]["fft_lat1"] / sp.EVERY,
                              "series_sample_ms": 0.067}
    if "direct" in forms:
        out["fft_is_faster"] = bool(out["launches"]["fft"]["k_spectra_rows_ms"] < out["launches"]["direct"]["k_spectra_rows_ms"])
    out["entries"], out["grid"], out["record_doubles"] = len(names), [n_lat, n_lon], sp.record_width(len(names), n_lon)
    text = json.dumps(out)
    print(text)
    os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
    with open(args.out, "w", encoding="utf-8") as f:
        f.write(text + "\n")


if __name__ == "__main__":
    main()
