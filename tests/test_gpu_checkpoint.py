"""GPU (-m gpu): a run cut in two by save_checkpoint and load_checkpoint equals the uncut run, bit for bit.

Scenario at 19 x 36, dt = 300 s (240 steps per planet-day): ocean, hydrology, river routing on a network generated on the device,
phytoplankton transport with the daily step, ecology with the daily vegetation step and the individuals' daily step, time-mean
history with 120-step windows.  Run A is 350 steps; run B is 175 steps, save_checkpoint, a NEW Simulation, load_checkpoint, 175
steps.  175 is not a multiple of 6 (the Shapiro cadence reads the step counter), lies inside the routing interval 144..216, inside
a day, inside the history window [120, 240) and inside a sub-step period of the individuals; the second half holds the routing events
of the steps 216 and 288, the day boundary of step 240 for every daily lane, and the window end at 240.  Every comparison is
np.array_equal on raw bits.  QD_ECO_RAND_SEED fixes the spread modes a run draws at start-up, so that A and B are the same run; the
Simulation that resumes is built under another seed and must take the saved run's modes from the file.  The control takes the same split through the reference's f4 restart and must differ.
A third case (37 x 72, no ocean, spectral filter every 4th step, 50 + 51 steps) covers the other counter-driven cadence and the
subsystem bookkeeping; the last runs main() twice in one data directory against main() once."""
import os
import re

import numpy as np
import pytest

pytestmark = pytest.mark.gpu

SPLIT, TOTAL = 175, 350


def _set_env(monkeypatch, env):
    for k in [k for k in os.environ if k.startswith("QD_")]:
        monkeypatch.delenv(k)
    for k, v in env.items():
        monkeypatch.setenv(k, str(v))


def _full_env(tmp_path):
    return {"QD_N_LAT": "19", "QD_N_LON": "36", "QD_DT_SECONDS": "300", "QD_USE_OCEAN": "1", "QD_HYDRO_ENABLE": "1", "QD_HYDRO_AUTOGEN": "1",
            "QD_HYDRO_NETCDF": str(tmp_path / "hydrology.nc"), "QD_HYDRO_DIAG": "0", "QD_PHYTO_ENABLE": "1", "QD_PHYTO_DAILY": "1",
            "QD_PHYTO_DIAG": "0", "QD_ECO_ENABLE": "1", "QD_ECO_DAILY": "1", "QD_ECO_INDIV_DAILY": "1", "QD_ECO_DIAG": "0", "QD_ECO_NS": "4",
            "QD_ECO_COHORT_K": "2", "QD_ECO_RAND_SEED": "3", "QD_ECO_SPREAD_ENABLE": "1", "QD_ECO_SPREAD_RATE": "0.1", "QD_HISTORY": "1",
            "QD_HISTORY_EVERY_DAYS": "0.5", "QD_OUTPUT_DIR": str(tmp_path / "unused")}


def _build(out_dir, fresh=True):
    """A Simulation from the environment with its lanes enabled; `fresh` runs the bootstrap a run has before its first step."""
    from qingdai_amd.driver import Simulation
    sim = Simulation(quiet=True)
    sim.enable_routing()
    sim.enable_history()
    if sim.history is not None:
        sim.history.output_dir = str(out_dir)
    if fresh:
        sim.bootstrap_ecology()
    return sim


def _bits(a):
    a = np.ascontiguousarray(a)
    return a.view({8: np.uint64, 1: np.uint8}[a.dtype.itemsize]).copy()


def _state(sim):
    """Raw bits of every resident plane the run has, by name."""
    from qingdai_amd import _lib
    d = sim.dev
    out = {}
    for name in _lib.FIELDS + ["LAND_MASK", "ICE_MASK"]:
        d._host.pop(name, None)
        out[name] = _bits(d.get(name))
        d._host.pop(name, None)
    if sim.phyto is not None:
        out["tracers"] = _bits(d.phyto_download())
    if sim.eco_daily is not None:
        out["lai_stack"] = _bits(d.eco_daily_get_layers(sim.eco.pop.Ns, sim.eco.pop.K))
    if sim.indiv is not None:
        E, S = sim.indiv._pull()
        out["indiv_E_day"], out["indiv_stress"] = _bits(E), _bits(S)
    if sim.routing is not None:
        for which in ("BUFFER", "FLOW") + (("LAKES",) if sim.routing.n_lakes > 0 else ()):
            out["route_" + which] = _bits(d.route_download(which))
    return out


def _finish(sim):
    if sim.history is not None:
        sim.flush_history(complete=0)
    res = {"state": _state(sim), "counters": sim.dev.counters(), "digest": sim.digest(), "t": sim.t, "step": sim._step_index,
           "files": list(sim.history.files) if sim.history is not None else []}
    sim.dev.close()
    return res


@pytest.fixture(scope="module")
def full_run(gpu, tmp_path_factory):
    """Run A, once for the module: 350 uncut steps of the full configuration, and its state after step 175."""
    tmp = tmp_path_factory.mktemp("ckpt_full")
    mp = pytest.MonkeyPatch()
    try:
        _set_env(mp, _full_env(tmp))
        sim = _build(tmp / "A")
        assert sim.routing is not None and sim.phyto_daily is not None and sim.eco_daily is not None and sim.indiv_daily is not None
        assert sim.history is not None and sim.history.S == 120 and sim.routing.dt_hydro_seconds == 72 * 300.0
        sim.run_steps(SPLIT)
        mid = _state(sim)
        sim.run_steps(TOTAL - SPLIT)
        res = _finish(sim)
        res["mid"] = mid
    finally:
        mp.undo()
    return tmp, res


def _compare(a, b):
    assert a["counters"] == b["counters"] and a["step"] == b["step"] and a["t"] == b["t"]
    assert a["state"].keys() == b["state"].keys()
    differ = [k for k in a["state"] if not np.array_equal(a["state"][k], b["state"][k])]
    assert not differ, differ
    assert a["digest"] == b["digest"]


def test_split_run_equals_the_uncut_run(gpu, full_run, monkeypatch, capsys):
    from qingdai_amd import ncio
    tmp, A = full_run
    _set_env(monkeypatch, _full_env(tmp))
    b1 = _build(tmp / "B")
    b1.run_steps(SPLIT)
    path = str(tmp / "ck" / "checkpoint.nc")
    run1 = b1.save_checkpoint(path, reason="test")
    assert run1 == b1.digest()["run"]
    assert b1.dev.counters()[0] == SPLIT and SPLIT % 6 != 0 and 144 < SPLIT < 216 and 120 < SPLIT < 240
    assert b1.routing.t_accum == (SPLIT - 144) * 300.0 and b1.history.n_open == SPLIT - 120 and b1.eco_daily.n_firings == 0
    mid = _state(b1)
    assert all(np.array_equal(mid[k], A["mid"][k]) for k in mid)             # the first halves are the same run
    modes = list(b1.eco_daily.species_modes)
    b1.dev.close()
    # a NEW Simulation, at its start values -- and with spread modes of its own draw, as a new process without QD_ECO_RAND_SEED has
    monkeypatch.setenv("QD_ECO_RAND_SEED", "12")
    b2 = _build(tmp / "B", fresh=False)
    assert b2.eco_daily.species_modes != modes and "seed" in modes and "diffusion" in modes
    assert b2.dev.counters() == (0, 0) and not np.array_equal(_state(b2)["TS"], mid["TS"])
    assert b2.load_checkpoint(path) == run1
    out = capsys.readouterr().out
    assert f"[Checkpoint] (test) wrote '{path}' at t={SPLIT * 300.0:.1f} s, step {SPLIT}, run digest 0x{run1:016x}" in out
    assert f"[Checkpoint] loaded '{path}' at t={SPLIT * 300.0:.1f} s, step {SPLIT}, run digest 0x{run1:016x}" in out
    assert b2.eco_daily.species_modes == modes
    loaded = _state(b2)
    assert not [k for k in mid if not np.array_equal(loaded[k], mid[k])]     # equal after resume means every field
    b2.run_steps(TOTAL - SPLIT)
    assert b2.eco_daily.n_firings == 1 and b2.phyto_daily.n_steps >= 1 and b2.routing._steps == TOTAL
    B = _finish(b2)
    _compare(A, B)
    # the history files written after the split: the window that was open at the save, and the one open at the end
    names = lambda files: [os.path.basename(p) for p in files]
    assert len(A["files"]) == 3 and names(B["files"]) == names(A["files"][1:])
    for pa, pb in zip(A["files"][1:], B["files"]):
        va, vb = ncio.read_nc(pa)[0], ncio.read_nc(pb)[0]
        assert va.keys() == vb.keys()
        for k in va:
            assert np.asarray(va[k]).tobytes() == np.asarray(vb[k]).tobytes(), (os.path.basename(pa), k)


def test_control_the_f4_restart_does_not_continue_the_run(gpu, full_run, monkeypatch):
    """The same split through sim.save / sim.load: the scenario sees a lossy resume."""
    tmp, A = full_run
    _set_env(monkeypatch, _full_env(tmp))
    c1 = _build(tmp / "C")
    c1.run_steps(SPLIT)
    path = str(tmp / "restart_f4.nc")
    c1.save(path)
    c1.dev.close()
    c2 = _build(tmp / "C", fresh=False)
    c2.load(path)
    c2.run_steps(TOTAL - SPLIT)
    C = _finish(c2)
    differ = [k for k in ("U", "V", "H", "TS", "Q", "CLOUD", "SST", "UO", "VO", "ETA", "W_LAND") if not np.array_equal(C["state"][k], A["state"][k])]
    assert differ, "the f4 restart reproduced the uncut run: the scenario cannot see a lossy resume"
    assert C["digest"]["run"] != A["digest"]["run"] and C["counters"] != A["counters"]


def test_no_ocean_spectral_cadence_and_subsystem_bookkeeping(gpu, tmp_path, monkeypatch):
    from qingdai_amd import checkpoint
    env = {"QD_N_LAT": "37", "QD_N_LON": "72", "QD_DT_SECONDS": "300", "QD_USE_OCEAN": "0", "QD_HYDRO_ENABLE": "0", "QD_PHYTO_ENABLE": "0",
           "QD_ECO_ENABLE": "0", "QD_FILTER_TYPE": "spectral", "QD_SPEC_EVERY": "4"}
    _set_env(monkeypatch, env)
    a = _build(tmp_path)
    assert a.ocean is None and a.routing is None and a.phyto is None and a.eco is None and a.history is None
    a.run_steps(101)
    A = _finish(a)
    b1 = _build(tmp_path)
    b1.run_steps(50)                                            # 50 is no multiple of 4: the filter cadence depends on the counter
    path = str(tmp_path / "checkpoint.nc")
    b1.save_checkpoint(path)
    b1.dev.close()
    b2 = _build(tmp_path, fresh=False)
    b2.load_checkpoint(path)
    assert b2.dev.counters()[0] == 50 and b2._step_index == 50
    b2.run_steps(51)
    _compare(A, _finish(b2))
    # without the counter the cadence shifts: a run that loads the planes alone is another run
    c = _build(tmp_path, fresh=False)
    c.load_checkpoint(path)
    c.dev.set_counters(0, 0)
    c.run_steps(51)
    assert _finish(c)["digest"]["run"] != A["digest"]["run"]
    # another subsystem set is refused, with nothing touched
    _set_env(monkeypatch, {**env, "QD_USE_OCEAN": "1"})
    d = _build(tmp_path, fresh=False)
    before = d.digest()
    with pytest.raises(checkpoint.CheckpointRefused, match="the subsystem set differs: ocean is off in the file and on in this run"):
        d.load_checkpoint(path)
    assert d.digest() == before
    d.dev.close()
    _set_env(monkeypatch, {**env, "QD_N_LAT": "19", "QD_N_LON": "36"})
    e = _build(tmp_path, fresh=False)
    with pytest.raises(checkpoint.CheckpointRefused, match="the grid shape differs: the file holds 37x72, the run is 19x36"):
        e.load_checkpoint(path)
    e.dev.close()


def test_f32_maps_and_autotuned_pair(gpu, tmp_path, monkeypatch, capsys):
    """QD_ECO_F32=1 (five maps live as f32 slabs and travel as the f8 images of their values) with QD_ENERGY_AUTOTUNE=1 (every 7th
    step runs alone, and the nudged qnet_lw pair acts from the next step on): 30 + 31 steps against 61.  30 is no multiple of 7, the
    second half holds the tuning steps 35 .. 56, and the light update of the canopy falls into both halves."""
    from qingdai_amd import checkpoint
    env = {"QD_N_LAT": "19", "QD_N_LON": "36", "QD_DT_SECONDS": "300", "QD_USE_OCEAN": "1", "QD_HYDRO_ENABLE": "0", "QD_PHYTO_ENABLE": "0",
           "QD_ECO_ENABLE": "1", "QD_ECO_F32": "1", "QD_ECO_DIAG": "0", "QD_ECO_NS": "3", "QD_ECO_LIGHT_UPDATE_EVERY_HOURS": "0.5",
           "QD_ENERGY_AUTOTUNE": "1", "QD_GH_LOCK": "0", "QD_ENERGY_TUNE_EVERY": "7", "QD_ENERGY_AUTOTUNE_DIAG": "0"}
    _set_env(monkeypatch, env)
    pair = lambda sim: np.array([sim.dev.params.qnet_lw_eps0, sim.dev.params.qnet_lw_kc]).view(np.uint64).tolist()
    a = _build(tmp_path)
    assert a.eco is not None and int(a.eco.params.map_f32) == 1 and a.indiv is not None and np.isnan(a.dev.params.qnet_lw_eps0)
    a.run_steps(61)
    pair_a = pair(a)
    assert not np.isnan(a.dev.params.qnet_lw_eps0)
    A = _finish(a)
    b1 = _build(tmp_path)
    b1.run_steps(30)
    pair_mid = pair(b1)
    path = str(tmp_path / "checkpoint.nc")
    # not at a span boundary: nothing is written
    b1._in_span = True
    with pytest.raises(checkpoint.CheckpointInconsistent, match="a span is in flight"):
        b1.save_checkpoint(path)
    b1._in_span = False
    b1.dev.set_counters(31, 31)
    with pytest.raises(checkpoint.CheckpointInconsistent, match="step index 30, device counter 31; at the last span's end 30 and 30"):
        b1.save_checkpoint(path)
    assert not os.path.exists(path)
    b1.dev.set_counters(30, 30)
    b1.save_checkpoint(path)
    b1.dev.close()
    f = checkpoint.read(path)
    assert f.subsystems()["eco_f32"] == "1" and f.plane("ECO_F").dtype == np.float32 and f.plane("TS").dtype == np.float64
    assert np.array_equal(f.plane("ECO_F").astype(np.float64), np.asarray(f.v["f_ECO_F"]))         # f8 images of f32 values
    b2 = _build(tmp_path, fresh=False)
    assert np.isnan(b2.dev.params.qnet_lw_eps0)
    b2.load_checkpoint(path)
    assert pair(b2) == pair_mid and "parameters differ" not in capsys.readouterr().out
    b2.run_steps(31)
    assert pair(b2) == pair_a and pair_a != pair_mid
    _compare(A, _finish(b2))
    # the same file in a run that keeps the maps as f64: another subsystem set
    _set_env(monkeypatch, {**env, "QD_ECO_F32": "0"})
    c = _build(tmp_path, fresh=False)
    with pytest.raises(checkpoint.CheckpointRefused, match="the subsystem set differs: eco_f32 is on in the file and off in this run"):
        c.load_checkpoint(path)
    c.dev.close()


def _main_env(tmp_path, data, days, **extra):
    env = {"QD_N_LAT": "19", "QD_N_LON": "36", "QD_DT_SECONDS": "300", "QD_SIM_DAYS": str(days), "QD_DYN_DIAG_PRINT": "0",
           "QD_DATA_DIR": str(tmp_path / data), "QD_OUTPUT_DIR": str(tmp_path / ("out_" + data)), "QD_HYDRO_AUTOGEN": "1",
           "QD_HYDRO_NETCDF": str(tmp_path / "hydrology.nc"), "QD_HYDRO_DIAG": "0", "QD_PHYTO_DAILY": "1", "QD_PHYTO_DIAG": "0",
           "QD_ECO_DAILY": "1", "QD_ECO_DIAG": "0", "QD_ECO_NS": "3", "QD_HISTORY": "1", "QD_HISTORY_EVERY_DAYS": "0.5", "QD_CHECKPOINT": "1"}
    env.update(extra)
    return env


def _run_digest_of(path):
    from qingdai_amd import ncio
    return ncio.read_nc(path, ["t_seconds"])[1]["run_digest"]


def test_main_twice_equals_main_once(gpu, tmp_path, monkeypatch, capsys):
    from qingdai_amd import driver, ncio
    monkeypatch.chdir(tmp_path)
    _set_env(monkeypatch, _main_env(tmp_path, "whole", 1.2))
    assert driver.main() == 0
    whole = capsys.readouterr().out
    assert "[Checkpoint] loaded" not in whole and "[Checkpoint] (final) wrote" in whole and " 288 steps" in whole
    assert "[Checkpoint] ecology.nc and genes.json are written and read as under QD_ECO_PERSIST=2." in whole
    want = _run_digest_of(str(tmp_path / "whole" / "checkpoint.nc"))
    _set_env(monkeypatch, _main_env(tmp_path, "cut", 0.6))
    assert driver.main() == 0
    first = capsys.readouterr().out
    assert " 144 steps" in first and "[Checkpoint] (final) wrote" in first and "[Checkpoint] loaded" not in first
    assert driver.main() == 0
    second = capsys.readouterr().out
    ck_path = str(tmp_path / "cut" / "checkpoint.nc")
    assert f"[Checkpoint] loaded '{ck_path}' at t=43200.0 s, step 144, run digest 0x" in second and "[Autosave] loaded" not in second
    assert re.search(r"\[Checkpoint\] \(final\) wrote '" + re.escape(ck_path) + r"' at t=86400\.0 s, step 288, run digest (0x[0-9a-f]{16})", second).group(1) == want
    assert _run_digest_of(ck_path) == want
    # the window that was open at the cut is written once, complete, under the uncut run's name
    hist = lambda d: sorted(os.listdir(tmp_path / ("out_" + d) / "history"))
    assert hist("cut") == hist("whole") and len(hist("whole")) == 2
    for name in hist("whole"):
        va, vb = ncio.read_nc(str(tmp_path / "out_whole" / "history" / name))[0], ncio.read_nc(str(tmp_path / "out_cut" / "history" / name))[0]
        assert all(np.asarray(va[k]).tobytes() == np.asarray(vb[k]).tobytes() for k in va), name
    # the reference's files are there as before
    assert {"atmosphere.nc", "ocean.nc", "topography.nc", "plankton.nc", "ecology.nc", "genes.json", "checkpoint.nc"} <= set(os.listdir(tmp_path / "cut"))
    # one byte of one plane changed: refused with the digest line, a non-zero exit, the file left alone
    dims, v, attrs = ncio.read_nc_full(ck_path)
    code, vd, arr = v["f_H"]
    arr = arr.copy()
    arr.view(np.uint8).flat[5] ^= 1
    v["f_H"] = (code, vd, arr)
    ncio.write_nc(ck_path, dims, v, attrs)
    stamp = open(ck_path, "rb").read()
    assert driver.main() == 2
    out = capsys.readouterr().out
    assert f"[Checkpoint] refused '{ck_path}': the digest of H does not match" in out and "Simulation Finished" not in out
    assert open(ck_path, "rb").read() == stamp
    # QD_CHECKPOINT_STRICT=0 falls back to atmosphere.nc
    _set_env(monkeypatch, _main_env(tmp_path, "cut", 0.05, QD_CHECKPOINT_STRICT="0"))
    assert driver.main() == 0
    out = capsys.readouterr().out
    assert f"[Checkpoint] refused '{ck_path}': the digest of H does not match" in out
    assert f"[Autosave] loaded '{tmp_path / 'cut' / 'atmosphere.nc'}' at t=86400.0 s" in out and "--- Simulation Finished ---" in out
