"""CPU: the file layer of qingdai_amd/checkpoint.py against a fake device (planes in a dict, the digest through the host reference
tests/state_digest_ref.py): the round trip of every variable kind through both ncio back ends, the atomic write, every refusal and
its text, the parameter note, the environment, and main()'s strict / non-strict start-up order against a fake Simulation."""
import os
import types

import numpy as np
import pytest

import state_digest_ref as ref
from qingdai_amd import _lib, checkpoint as ck, ncio
from qingdai_amd.params import QdParams

SHAPE = (7, 10)


def _backends():
    out = ["scipy"]
    try:
        import netCDF4  # noqa: F401
        out.append("netCDF4")
    except Exception:      # noqa: BLE001
        pass
    return out


class FakeDev:
    whole_globe = True

    def __init__(self, seed=0, f32=False):
        rng = np.random.default_rng(seed)
        self.shape, self.params, self.f32 = SHAPE, QdParams(), f32
        self._host = {}
        bits = lambda *s: rng.integers(0, 2**64, s, dtype=np.uint64).view(np.float64)
        self.planes = {n: bits(*SHAPE) for n in _lib.FIELDS}
        for n in ck.F32_MAPS:                                  # what a download of an f32 slab hands out: f8 images of f32 values
            if f32:
                self.planes[n] = rng.standard_normal(SHAPE).astype(np.float32).astype(np.float64)
        self.planes["ELEVATION"] = np.zeros(SHAPE)
        self.planes["LAND_MASK"] = (rng.random(SHAPE) < 0.4).astype(np.uint8)
        self.planes["ICE_MASK"] = (rng.random(SHAPE) < 0.2).astype(np.uint8)
        self.tracers, self.route = bits(3, *SHAPE), {"BUFFER": bits(*SHAPE), "FLOW": bits(*SHAPE), "LAKES": bits(4)}
        self.route_steps = 0
        self.hist, self.hist_count = bits(2, *SHAPE), 5
        self.ctr = (175, 175)
        self.scalars = rng.random(_lib.STATE_SCALARS_N)
        self.pushed = 0

    def flush(self):
        pass

    def get(self, name):
        return self.planes[name]

    def upload_now(self, name, arr):
        self.planes[name] = np.array(arr, dtype=np.uint8 if name.endswith("_MASK") else np.float64)

    def counters(self):
        return self.ctr

    def set_counters(self, a, o):
        self.ctr = (a, o)

    def state_scalars(self):
        return self.scalars.copy()

    def set_state_scalars(self, v):
        self.scalars = np.array(v, dtype=np.float64)

    def push_params(self):
        self.pushed += 1

    def phyto_download(self):
        return self.tracers.copy()

    def phyto_upload(self, C):
        self.tracers = np.array(C)

    def route_download(self, which):
        return self.route[which].reshape(-1).copy()

    def route_restore(self, buf, flow, lakes, steps):
        self.route = {"BUFFER": np.array(buf).reshape(SHAPE), "FLOW": np.array(flow).reshape(SHAPE), "LAKES": np.array(lakes)}
        self.route_steps = steps

    def history_read(self):
        return self.hist.copy(), self.hist_count

    def history_restore(self, sums, count):
        self.hist, self.hist_count = np.array(sums), count

    def _plane(self, name):
        base, _, idx = name.partition(":")
        if base == "PHYTO_TRACER":
            return self.tracers[int(idx)]
        if base == "HISTORY_SUM":
            return self.hist[int(idx)]
        if name.startswith("ROUTE_"):
            return self.route[name[6:]]
        a = self.planes[name]
        return a.astype(np.float32) if (self.f32 and name in ck.F32_MAPS) else a

    def digest(self, names):
        return np.array([ref.digest(self._plane(n)) for n in names], dtype=np.uint64)


def _sim(seed=0, routing=True, history=("TS", "U"), f32=False):
    dev = FakeDev(seed, f32=f32)
    eco = types.SimpleNamespace(pop=None, params=types.SimpleNamespace(map_f32=1)) if f32 else None
    sim = types.SimpleNamespace(
        dev=dev, eco=eco, indiv=None, eco_daily=None, indiv_daily=None, ocean=object(), speciation=None, daily_hook=None, budget=None,
        phyto=types.SimpleNamespace(S=3), phyto_transport=True, phyto_daily=types.SimpleNamespace(phyto_next_time=72000.0, n_steps=2),
        routing=types.SimpleNamespace(n_lakes=4, t_accum=9300.0, _steps=175, _have_event=True, _last="x") if routing else None,
        history=types.SimpleNamespace(names=list(history), i=175, t_first=36000.0, t_last=None, n_open=55) if history else None,
        land_mask=dev.planes["LAND_MASK"].copy(), elevation=None, t=52500.0, _t_origin=(0.0, 175, 300.0), _step_index=175,
        diversity_next_day=10.5, _index_base=0)
    return sim


def _fresh(like, **kw):
    """A run that starts over: other planes and clocks, the same topography."""
    sim = _sim(seed=99, **kw)
    sim.dev.planes["LAND_MASK"] = like.land_mask.copy()
    sim.land_mask = like.land_mask.copy()
    sim.t, sim._t_origin, sim._step_index, sim.diversity_next_day = 0.0, (0.0, 0, None), 0, 0.0
    if sim.routing is not None:
        sim.routing.t_accum, sim.routing._steps, sim.routing._have_event = 0.0, 0, False
    if sim.history is not None:
        sim.history.i, sim.history.t_first, sim.history.n_open = 0, None, 0
    sim.phyto_daily.phyto_next_time, sim.phyto_daily.n_steps = 0.0, 0
    sim.dev.ctr = (0, 0)
    return sim


def _bits(a):
    a = np.ascontiguousarray(a)
    return a.view({8: np.uint64, 1: np.uint8}[a.dtype.itemsize])


@pytest.mark.parametrize("backend", _backends())
@pytest.mark.parametrize("f32", [False, True], ids=["f64maps", "f32maps"])
def test_round_trip_of_every_variable_kind_cpu(tmp_path, monkeypatch, capsys, backend, f32):
    monkeypatch.setattr(ncio, "backend", lambda: backend)
    a = _sim(f32=f32)
    path = str(tmp_path / "sub" / "checkpoint.nc")
    run = ck.save(a, path, reason="periodic")
    out = capsys.readouterr().out
    assert out.startswith(f"[Checkpoint] (periodic) wrote '{path}' at t=52500.0 s, step 175, run digest 0x{run:016x}")
    assert run == ck.simulation_digest(a)["run"] == ref.run_digest({n: ref.digest(a.dev._plane(n)) for n in ck.plane_names(a)})
    v, attrs = ncio.read_nc(path)
    assert attrs["format"] == "qd-checkpoint-1" and int(attrs["abi_version"]) == 1 and attrs["run_digest"] == f"0x{run:016x}"
    assert v["f_U"].dtype == np.float64 and v["m_ICE_MASK"].dtype.itemsize == 1 and v["hist_sums"].shape == (2,) + SHAPE
    assert attrs["digest_PHYTO_TRACER_2"] == f"0x{ref.digest(a.dev.tracers[2]):016x}"
    assert [f for f in os.listdir(tmp_path / "sub")] == ["checkpoint.nc"]          # no temporary file left
    b = _fresh(a, f32=f32)
    assert ck.load(b, path) == run
    assert f"[Checkpoint] loaded '{path}' at t=52500.0 s, step 175, run digest 0x{run:016x}" in capsys.readouterr().out
    for n in _lib.FIELDS + ["ICE_MASK"]:
        assert np.array_equal(_bits(b.dev.planes[n]), _bits(a.dev.planes[n])), n       # raw bits: NaN payloads, signed zeros
    assert np.array_equal(_bits(b.dev.tracers), _bits(a.dev.tracers)) and np.array_equal(_bits(b.dev.hist), _bits(a.dev.hist))
    for k in ("BUFFER", "FLOW", "LAKES"):
        assert np.array_equal(_bits(b.dev.route[k]), _bits(a.dev.route[k])), k
    assert b.dev.ctr == (175, 175) and b.dev.route_steps == 175 and b.dev.hist_count == 5
    assert np.array_equal(b.dev.scalars, a.dev.scalars)
    assert (b.t, b._t_origin, b._step_index, b._index_base, b.diversity_next_day, b._span_mark) == (52500.0, (0.0, 175, 300.0), 175, 175, 10.5, (175, 175))
    assert (b.routing.t_accum, b.routing._steps, b.routing._have_event, b.routing._last) == (9300.0, 175, True, None)
    assert (b.history.i, b.history.t_first, b.history.t_last, b.history.n_open) == (175, 36000.0, None, 55)
    assert (b.phyto_daily.phyto_next_time, b.phyto_daily.n_steps) == (72000.0, 2)
    assert ck.simulation_digest(b) == ck.simulation_digest(a)


def test_atomic_write_cpu(tmp_path, monkeypatch):
    a = _sim()
    path = str(tmp_path / "checkpoint.nc")
    ck.save(a, path)
    before = open(path, "rb").read()
    real = ncio.write_nc

    def dies(p, dims, variables, attrs=None):
        real(p, dims, {k: variables[k] for k in list(variables)[:5]}, attrs)          # half a file is on disk ...
        raise OSError("disk full")
    monkeypatch.setattr(ncio, "write_nc", dies)
    a.dev.planes["U"] = a.dev.planes["U"] + 1.0
    with pytest.raises(OSError, match="disk full"):
        ck.save(a, path)
    assert open(path, "rb").read() == before and os.listdir(tmp_path) == ["checkpoint.nc"]      # ... and the old one is what stays
    monkeypatch.setattr(ncio, "write_nc", real)
    assert ck.load(_fresh(a), path, out=lambda s: None) == int(ncio.read_nc(path)[1]["run_digest"], 16)


def _rewrite(path, change):
    dims, v, attrs = ncio.read_nc_full(path)
    change(v, attrs)
    ncio.write_nc(path, dims, v, attrs)


def test_every_refusal_and_its_text_cpu(tmp_path):
    a = _sim()
    path = str(tmp_path / "checkpoint.nc")
    ck.save(a, path)
    quiet = lambda s: None

    def refused(sim, p=path, env=None):
        before = {n: x.copy() for n, x in sim.dev.planes.items()}
        with pytest.raises(ck.CheckpointRefused) as e:
            ck.load(sim, p, env=env or {}, out=quiet)
        assert all(np.array_equal(_bits(before[n]), _bits(sim.dev.planes[n])) for n in before) and sim._step_index == 0     # nothing touched
        return str(e.value)
    assert refused(_fresh(a), str(tmp_path / "none.nc")) == "the file does not exist"
    other = str(tmp_path / "other.nc")
    ncio.write_nc(other, {"x": 2}, {"x": ("f8", ("x",), np.zeros(2))}, {"title": "something else"})
    assert "is not a checkpoint of this package" in refused(_fresh(a), other)
    # the subsystem set
    assert refused(_fresh(a, routing=False)) == "the subsystem set differs: routing is on in the file and off in this run"
    assert refused(_fresh(a, history=("TS", "H"))) == "the subsystem set differs: the history fields are 'TS,U' in the file and 'TS,H' in this run"
    assert refused(_fresh(a, history=None)) == "the subsystem set differs: the history fields are 'TS,U' in the file and '-' in this run"
    assert refused(_fresh(a, f32=True)) == "the subsystem set differs: ecology is off in the file and on in this run"
    b = _fresh(a)
    b.ocean = None
    assert refused(b) == "the subsystem set differs: ocean is on in the file and off in this run"
    b = _fresh(a)
    b.phyto_daily = None
    assert refused(b) == "the subsystem set differs: phyto_daily is on in the file and off in this run"
    # the topography
    b = _fresh(a)
    b.land_mask = 1 - b.land_mask
    assert refused(b) == "the land mask differs from the run's topography"
    # start-up refusals reach a load too
    b = _fresh(a)
    b.daily_hook = lambda *x: None
    assert "does not run with a daily_hook" in refused(b)
    assert "does not run with QD_ECO_SPECIATION=1" in refused(_fresh(a), env={"QD_ECO_SPECIATION": "1"})
    b = _fresh(a)
    b.dev.whole_globe = False
    assert "latitude bands" in refused(b)
    # grid shape and ABI version
    p2 = str(tmp_path / "grid.nc")
    ck.save(a, p2)
    _rewrite(p2, lambda v, at: at.update(n_lat=9.0))
    assert refused(_fresh(a), p2) == "the grid shape differs: the file holds 9x10, the run is 7x10"
    ck.save(a, p2)
    _rewrite(p2, lambda v, at: at.update(abi_version=2.0))
    assert refused(_fresh(a), p2) == "the ABI version differs: the file was written by version 2, this build is version 1"
    # one changed byte of one plane; a truncated variable; a plane mapped to another slab
    ck.save(a, p2)

    def flip(v, at):
        code, dims, arr = v["f_TS"]
        arr = arr.copy()
        arr.view(np.uint8).flat[13] ^= 1
        v["f_TS"] = (code, dims, arr)
    _rewrite(p2, flip)
    msg = refused(_fresh(a), p2)
    assert msg.startswith("the digest of TS does not match: the file's plane gives 0x") and msg.endswith(f"the file says 0x{ref.digest(a.dev.planes['TS']):016x}")
    ck.save(a, p2)
    _rewrite(p2, lambda v, at: v.pop("f_Q"))
    assert refused(_fresh(a), p2) == "the file holds digests of planes it does not hold"
    ck.save(a, p2)

    def swap(v, at):
        v["f_U"], v["f_V"] = v["f_V"], v["f_U"]
    _rewrite(p2, swap)
    assert refused(_fresh(a), p2).startswith("the digest of U does not match")
    ck.save(a, p2)
    _rewrite(p2, lambda v, at: at.update(run_digest="0x0000000000000001"))
    assert refused(_fresh(a), p2).startswith("the run digest does not match")


def test_saved_only_at_a_span_boundary_cpu(tmp_path, capsys):
    """Right behind the device call of a span the device is ahead of the host clocks (that is where a signal handler runs): no
    file is written and the last good one stays; a file whose counters disagree with its span mark is refused by a load."""
    a = _sim()
    a._span_mark, a._in_span = (175, 175), False
    path = str(tmp_path / "checkpoint.nc")
    ck.save(a, path)
    good = open(path, "rb").read()
    a.dev.ctr = (190, 190)                                      # qd_step_n has returned, _run_lanes has not moved the clocks yet
    a._in_span = True
    with pytest.raises(ck.CheckpointInconsistent, match="a span is in flight"):
        ck.save(a, path)
    a._in_span = False                                          # an error inside a span: the flag is down, the device moved on
    with pytest.raises(ck.CheckpointInconsistent, match="step index 175, device counter 190; at the last span's end 175 and 175"):
        ck.save(a, path)
    assert open(path, "rb").read() == good and os.listdir(tmp_path) == ["checkpoint.nc"]
    a._step_index, a._span_mark = 190, (190, 190)               # the bookkeeping is done
    ck.save(a, path)
    # a file written without the guard: planes and counter of step 190, clocks of step 175
    bad = str(tmp_path / "bad.nc")
    ck.save(a, bad)
    _rewrite(bad, lambda v, at: v.update(step_index=(v["step_index"][0], (), 175)))
    b = _fresh(a)
    with pytest.raises(ck.CheckpointRefused, match="the file was not written at a span boundary: step index 175 and device counter 190 "
                                                   "against 190 and 190"):
        ck.load(b, bad, out=lambda s: None)
    assert b._step_index == 0 and b.dev.ctr == (0, 0)
    _rewrite(bad, lambda v, at: v.pop("span_mark"))
    with pytest.raises(ck.CheckpointRefused, match="the file holds no span mark"):
        ck.load(_fresh(a), bad, out=lambda s: None)


def test_device_digest_after_the_upload_is_checked_cpu(tmp_path):
    """A device that stores a plane in another slab than the one it digests: the file is fine, the upload is not."""
    a = _sim()
    path = str(tmp_path / "checkpoint.nc")
    ck.save(a, path)
    b = _fresh(a)
    up = b.dev.upload_now
    b.dev.upload_now = lambda name, arr: up("V" if name == "U" else name, arr)
    with pytest.raises(RuntimeError, match="after the upload the device digest of U is 0x"):
        ck.load(b, path, out=lambda s: None)


def test_parameter_difference_note_cpu(tmp_path, capsys):
    a = _sim()
    path = str(tmp_path / "checkpoint.nc")
    a.dev.params.qnet_lw_eps0, a.dev.params.qnet_lw_kc = 0.71, 0.23
    ck.save(a, path)
    b = _fresh(a)
    b.dev.params.update(tau_rad=1.0e6, shapiro_every=4)
    ck.load(b, path, env={})
    out = capsys.readouterr().out
    assert out.count("[Checkpoint] note: parameters differ from the saved run: ") == 1
    names = out.split("parameters differ from the saved run: ")[1].splitlines()[0].split(", ")
    assert set(names) == {"tau_rad", "shapiro_every", "qnet_lw_eps0", "qnet_lw_kc"}
    assert np.isnan(b.dev.params.qnet_lw_eps0) and b.dev.pushed == 0           # without the autotuner the run's own pair stays
    # QD_ENERGY_AUTOTUNE=1: the autotuned pair comes from the file and is not a difference
    c = _fresh(a)
    ck.load(c, path, env={"QD_ENERGY_AUTOTUNE": "1"})
    assert "parameters differ" not in capsys.readouterr().out
    assert (c.dev.params.qnet_lw_eps0, c.dev.params.qnet_lw_kc, c.dev.pushed) == (0.71, 0.23, 1)


def test_env_parsing_cpu():
    assert ck.read_env({}) == {"enabled": False, "path": os.path.join("data", "checkpoint.nc"), "strict": True}
    assert ck.read_env({"QD_CHECKPOINT": "1", "QD_DATA_DIR": "/x/y"}) == {"enabled": True, "path": "/x/y/checkpoint.nc", "strict": True}
    assert ck.read_env({"QD_CHECKPOINT": "1", "QD_CHECKPOINT_PATH": "/z/c.nc", "QD_CHECKPOINT_STRICT": "0"}, "d") == \
        {"enabled": True, "path": "/z/c.nc", "strict": False}
    assert ck.read_env({"QD_CHECKPOINT": "yes", "QD_CHECKPOINT_STRICT": "?"})["enabled"] is False
    assert ck.read_env({"QD_CHECKPOINT": "2"})["enabled"] is False and ck.read_env({"QD_CHECKPOINT_STRICT": "?"})["strict"] is True
    from qingdai_amd.driver import eco_persist_level
    assert eco_persist_level({}) == 0 and eco_persist_level({"QD_ECO_PERSIST": "1"}) == 1
    assert eco_persist_level({"QD_CHECKPOINT": "1"}) == 2 and eco_persist_level({"QD_CHECKPOINT": "1", "QD_ECO_PERSIST": "1"}) == 2


def test_host_digest_is_the_reference_cpu():
    rng = np.random.default_rng(2)
    for a in (rng.integers(0, 2**64, (5, 7), dtype=np.uint64).view(np.float64), rng.standard_normal(11).astype(np.float32),
              rng.integers(0, 256, 9, dtype=np.uint8), np.zeros(0)):
        assert ck.host_digest(a) == ref.digest(a)
    assert ck.fnv1a64("run") == ref.fnv1a64("run") and ck.run_digest({"U": 5, "X:1": 9}) == ref.run_digest({"U": 5, "X:1": 9})


# ------------------------------------------------------------------ main()'s start-up order against a fake Simulation
class MainSim:
    """What driver.main asks of a Simulation, with a fake device; every call that matters is recorded."""
    made = []

    def __init__(self):
        s = _fresh(_sim())
        self.__dict__.update(s.__dict__)
        self.calls = []
        self.grid = types.SimpleNamespace(n_lat=SHAPE[0], n_lon=SHAPE[1])
        self.forcing = types.SimpleNamespace(orbital_system=types.SimpleNamespace(T_planet=3.0e7))
        self.dt = 300
        self.routing = self.history = None
        MainSim.made.append(self)

    def load(self, path):
        self.calls.append(("load", os.path.basename(path)))
        self.t = 600.0

    def load_ocean_override(self, path):
        return False

    def load_ecology(self, data_dir, env):
        self.calls.append(("load_ecology",))

    def enable_routing(self, env):
        self.calls.append(("enable_routing",))
        self.routing = types.SimpleNamespace(n_lakes=4, t_accum=0.0, _steps=0, _have_event=False, _last=None)

    def enable_budget_diag(self, env):
        pass

    def enable_history(self, env):
        self.history = types.SimpleNamespace(names=["TS", "U"], i=0, t_first=None, t_last=None, n_open=0)

    def enable_stateframe(self, env):
        return None

    enable_truecolor = enable_figures = enable_stateframe

    def bootstrap_ecology(self):
        self.calls.append(("bootstrap",))

    def load_checkpoint(self, f, env=None):
        self.calls.append(("load_checkpoint",))
        return ck.load(self, f, env=env)

    def save_checkpoint(self, path, reason=None):
        self.calls.append(("save_checkpoint", reason))
        return ck.save(self, path, reason=reason)

    def run_loop(self, n_total, next_autosave_t, after_chunk):
        self.calls.append(("run_loop", n_total))
        self.t += n_total * self.dt
        self._step_index += n_total

    def save_autosave(self, data_dir):
        self.calls.append(("save_autosave",))
        open(os.path.join(data_dir, "atmosphere.nc"), "wb").write(b"x")

    def save(self, path):
        pass

    def flush_history(self, complete=1):
        self.calls.append(("flush_history", complete))


def _main(monkeypatch, tmp_path, **env):
    from qingdai_amd import driver
    for k in [k for k in os.environ if k.startswith("QD_")]:
        monkeypatch.delenv(k)
    base = {"QD_DATA_DIR": str(tmp_path / "data"), "QD_SIM_DAYS": "0.01", "QD_DYN_DIAG_PRINT": "0", "QD_ECO_AUTOSAVE_EVERY_HOURS": "0"}
    for k, v in {**base, **env}.items():
        monkeypatch.setenv(k, v)
    monkeypatch.setattr(driver, "Simulation", MainSim)
    monkeypatch.setattr(driver.atexit, "register", lambda fn: None)
    monkeypatch.setattr(driver.signal, "signal", lambda *a: None)
    os.makedirs(tmp_path / "data", exist_ok=True)
    MainSim.made.clear()
    rc = driver.main()
    return rc, MainSim.made[-1]


def test_main_start_up_order_cpu(tmp_path, monkeypatch, capsys):
    path = str(tmp_path / "data" / "checkpoint.nc")
    # 1. switch off: nothing of the checkpoint is called, written or printed
    rc, sim = _main(monkeypatch, tmp_path)
    assert rc == 0 and not os.path.exists(path) and "[Checkpoint]" not in capsys.readouterr().out
    assert [c[0] for c in sim.calls] == ["load_ecology", "enable_routing", "bootstrap", "run_loop", "flush_history", "save_autosave"]
    # 2. switch on, no file yet: a fresh start that writes one behind the reference's files
    rc, sim = _main(monkeypatch, tmp_path, QD_CHECKPOINT="1", QD_AUTOSAVE_LOAD="0")
    out = capsys.readouterr().out
    assert rc == 0 and os.path.exists(path) and f"[Checkpoint] (final) wrote '{path}'" in out
    assert [c[0] for c in sim.calls] == ["load_ecology", "enable_routing", "bootstrap", "run_loop", "save_autosave", "save_checkpoint"]
    saved_t, saved_i = sim.t, sim._step_index
    # 3. the checkpoint wins over atmosphere.nc: loaded behind the lanes, no legacy load, no bootstrap; the clock goes on
    rc, sim = _main(monkeypatch, tmp_path, QD_CHECKPOINT="1")
    out = capsys.readouterr().out
    assert rc == 0 and f"[Checkpoint] loaded '{path}' at t={saved_t:.1f} s, step {saved_i}" in out and "[Autosave] loaded" not in out
    assert [c[0] for c in sim.calls] == ["enable_routing", "load_checkpoint", "run_loop", "save_autosave", "save_checkpoint"]
    assert sim._step_index == 2 * saved_i
    # 4. QD_RESTART_IN or QD_AUTOSAVE_LOAD=0: the checkpoint is not looked at
    rc, sim = _main(monkeypatch, tmp_path, QD_CHECKPOINT="1", QD_RESTART_IN=str(tmp_path / "data" / "atmosphere.nc"))
    assert rc == 0 and ("load", "atmosphere.nc") in sim.calls and ("load_checkpoint",) not in sim.calls
    capsys.readouterr()
    # 5. one byte of one plane changed: refused with the digest line; strict -> 2, nothing run, nothing written
    ck.save(_sim(), path)

    def flip(v, at):
        code, dims, arr = v["f_TS"]
        arr = arr.copy()
        arr.view(np.uint8).flat[3] ^= 1
        v["f_TS"] = (code, dims, arr)
    _rewrite(path, flip)
    stamp = open(path, "rb").read()
    rc, sim = _main(monkeypatch, tmp_path, QD_CHECKPOINT="1")
    out = capsys.readouterr().out
    assert rc == 2 and f"[Checkpoint] refused '{path}': the digest of TS does not match" in out and sim.calls == []
    assert open(path, "rb").read() == stamp
    # 6. ... and QD_CHECKPOINT_STRICT=0 takes the old load order
    rc, sim = _main(monkeypatch, tmp_path, QD_CHECKPOINT="1", QD_CHECKPOINT_STRICT="0")
    out = capsys.readouterr().out
    assert rc == 0 and f"[Checkpoint] refused '{path}': the digest of TS does not match" in out and "[Autosave] loaded" in out
    assert [c[0] for c in sim.calls][:4] == ["load", "load_ecology", "enable_routing", "bootstrap"]
    # 7. a file of another subsystem set is refused behind the lanes: strict -> 2; else the old order, late
    a = _sim(history=("TS", "H"))
    a.land_mask = sim.land_mask.copy()
    a.dev.planes["LAND_MASK"] = sim.land_mask.copy()
    ck.save(a, path)
    rc, sim = _main(monkeypatch, tmp_path, QD_CHECKPOINT="1")
    assert rc == 2 and "refused" in capsys.readouterr().out and [c[0] for c in sim.calls] == ["enable_routing", "load_checkpoint"]
    rc, sim = _main(monkeypatch, tmp_path, QD_CHECKPOINT="1", QD_CHECKPOINT_STRICT="0")
    assert rc == 0 and [c[0] for c in sim.calls][:5] == ["enable_routing", "load_checkpoint", "load", "load_ecology", "bootstrap"]
    # 8. refused at start-up
    rc, sim = _main(monkeypatch, tmp_path, QD_CHECKPOINT="1", QD_ECO_SPECIATION="1")
    assert rc == 2 and "[Checkpoint] QD_CHECKPOINT=1 does not run with QD_ECO_SPECIATION=1" in capsys.readouterr().out and sim.calls == []


class LoopSim(MainSim):
    """MainSim with the real run_loop; its run_steps is a span: the device call, then -- where a signal handler runs -- the handler,
    then the bookkeeping."""
    from qingdai_amd import driver as _driver
    run_loop, request_stop = _driver.Simulation.run_loop, _driver.Simulation.request_stop
    _in_chunk, _stop_request, _in_span = False, None, False
    handlers, fire_at = {}, None

    def __init__(self):
        super().__init__()
        self._span_mark = (0, 0)

    def outputs_due(self, i0, n_max):
        return []

    def run_steps(self, n):
        import signal as _signal
        self._in_span = True
        self.dev.ctr = (self.dev.ctr[0] + n, self.dev.ctr[1] + n)          # qd_step_n has returned
        self.calls.append(("device", self.dev.ctr[0]))
        if LoopSim.fire_at is not None and self.dev.ctr[0] >= LoopSim.fire_at:
            LoopSim.fire_at = None
            LoopSim.handlers[_signal.SIGTERM](_signal.SIGTERM, None)       # ... and Python runs the handler here
        self.t += n * self.dt
        self._step_index += n
        self._span_mark, self._in_span = (self._step_index, self.dev.ctr[0]), False
        self.calls.append(("bookkeeping", self._step_index))


def test_signal_between_the_device_call_and_the_bookkeeping_cpu(tmp_path, monkeypatch, capsys):
    from qingdai_amd import driver
    for k in [k for k in os.environ if k.startswith("QD_")]:
        monkeypatch.delenv(k)

    def run(**env):
        base = {"QD_DATA_DIR": str(tmp_path / "data"), "QD_SIM_DAYS": "0.02", "QD_DYN_DIAG_PRINT": "0", "QD_ECO_AUTOSAVE_EVERY_HOURS": "0.04",
                "QD_AUTOSAVE_LOAD": "0"}
        for k in [k for k in os.environ if k.startswith("QD_")]:
            monkeypatch.delenv(k)
        for k, v in {**base, **env}.items():
            monkeypatch.setenv(k, v)
        monkeypatch.setattr(driver, "Simulation", LoopSim)
        monkeypatch.setattr(driver.atexit, "register", lambda fn: None)
        monkeypatch.setattr(driver.signal, "signal", lambda sig, fn: LoopSim.handlers.__setitem__(sig, fn))
        os.makedirs(tmp_path / "data", exist_ok=True)
        MainSim.made.clear()
        LoopSim.fire_at = 2
        with pytest.raises(SystemExit) as e:
            driver.main()
        return e.value.code, MainSim.made[-1], capsys.readouterr().out
    # 0.04 planetary hours = 120 s: chunks of 1 step (the autosave threshold), 5 steps in all; SIGTERM behind the device call of step 2
    code, sim, out = run(QD_CHECKPOINT="1")
    names = [c[0] for c in sim.calls]
    assert code == 143 and ("device", 2) in sim.calls
    at = sim.calls.index(("device", 2))
    assert sim.calls[at + 1] == ("bookkeeping", 2)              # nothing was saved in between: the stop waited
    assert names.count("device") == 2 and sim.calls[-1] == ("save_checkpoint", "signal") and sim.calls[-2] == ("save_autosave",)
    assert "[Checkpoint] (signal) wrote" in out and "skipped" not in out
    f = ck.read(str(tmp_path / "data" / "checkpoint.nc"))
    assert int(f.scalar("step_index")) == 2 == int(f.scalar("atm_counter")) and list(f.v["span_mark"]) == [2.0, 2.0]
    ck.check_grid_and_abi(f, SHAPE)
    # without the switch the handler acts at once, as it always did
    code, sim, out = run()
    at = sim.calls.index(("device", 2))
    assert code == 143 and sim.calls[at + 1] == ("save_autosave",) and ("bookkeeping", 2) not in sim.calls and "[Checkpoint]" not in out
    # a handler that did act inside a span (request_stop not taken): the f4 files are written, the checkpoint is skipped and kept
    monkeypatch.setattr(LoopSim, "request_stop", lambda self, stop: False)
    code, sim, out = run(QD_CHECKPOINT="1")
    assert code == 143 and "[Checkpoint] (signal) skipped: a span is in flight" in out and ("save_autosave",) in sim.calls
    kept = ck.read(str(tmp_path / "data" / "checkpoint.nc"))      # the periodic file of step 1, the last consistent state of this run
    assert int(kept.scalar("step_index")) == 1 == int(kept.scalar("atm_counter")) and "[Checkpoint] (periodic) wrote" in out
