"""CPU: the three host clocks that name the steps on which the device fires inside a qd_step_n span -- RiverRouting.schedule,
phyto.daily_schedule driven by Simulation.t, ecology.daily_counts -- around a stub library (no GPU, no libqingdai_hip.so).

Partition invariance: however N steps are cut into spans, the concatenated schedules, the times handed to the forcing table and
the clocks afterwards are those of the one whole span, and both are those of a literal step-by-step transcription of the
reference driver's loop:
  t              `time_steps = np.arange(t0_seconds, t0_seconds + sim_duration_seconds, dt)`, `for i, t in enumerate(...)`
                 (run_simulation.py:1639, 1746-1760): NumPy fills it as t0 + i * ((t0 + dt) - t0)
  vegetation     `accum_t_day += dt; while accum_t_day >= day_in_seconds: ... accum_t_day -= day_in_seconds` (run_simulation.py:1785-1789)
  phytoplankton  `if t >= phyto_next_time: ... phyto_next_time = t + day_in_seconds` (run_simulation.py:1738, 2053-2061)
  routing        `self.t_accum += float(dt_seconds); if self.t_accum + 1e-9 < self.dt_hydro_seconds: return;
                 event_dt = self.t_accum; self.t_accum = 0.0` (pygcm/routing.py:236-243)
The spans are driven through Simulation._run_chunk and Device.step_n themselves, so what is compared is what reaches
qd_*_schedule and ThermalForcing.star_table."""
import ctypes

import numpy as np
import pytest

from qingdai_amd.device import Device
from qingdai_amd.driver import Simulation
from qingdai_amd.ecology import PopulationDaily, daily_counts
from qingdai_amd.phyto import PhytoDaily, daily_schedule
from qingdai_amd.routing import RiverRouting

PLANET_DAY = 2 * np.pi / 8.726646259971648e-5
N = 97
SCHEDULES = {"qd_route_schedule": ctypes.c_double, "qd_phyto_daily_schedule": ctypes.c_int32, "qd_eco_daily_schedule": ctypes.c_int32}
LOGS = ("qd_route_events", "qd_phyto_daily_log", "qd_eco_daily_log")


class StubLib:
    """Keeps every schedule a span uploads; the logs are empty."""

    def __init__(self):
        self.sched = {k: [] for k in SCHEDULES}
        self.spans = []

    def __getattr__(self, name):
        if name in SCHEDULES:
            def fn(h, n, ptr):
                self.sched[name] += list(np.ctypeslib.as_array(ptr, shape=(n,))) if n else []
                return 0
            return fn
        if name in LOGS:
            return lambda h, buf, cap, n: 0
        if name == "qd_step_n":
            def step(h, n, dt, flags, stars):
                self.spans.append(n)
                return 0
            return step
        raise AttributeError(name)

    def qd_destroy(self, h):
        return 0


class StubForcing:
    def __init__(self):
        self.times = []

    def star_table(self, times):
        self.times += [float(t) for t in times]
        return np.zeros((len(times), 7))


def make_sim(t0, dt, day_phyto, day_eco, dt_hydro):
    dev = object.__new__(Device)
    dev.lib, dev.h, dev._host = StubLib(), ctypes.c_void_p(1), {}
    sim = object.__new__(Simulation)
    sim.dev, sim.dt, sim._step_index, sim.forcing = dev, dt, 0, StubForcing()
    sim.t = t0
    sim.ocean, sim.eco, sim.phyto_transport, sim.daily_hook, sim.eco_diag = None, object(), False, None, False
    r = object.__new__(RiverRouting)
    r.dev, r.dt_hydro_seconds, r.t_accum, r._steps, r.diag_enabled = dev, dt_hydro, 0.0, 0, False
    p = object.__new__(PhytoDaily)
    p.dev, p.day_seconds, p.phyto_next_time, p.n_steps, p.diag = dev, day_phyto, 0.0, 0, False
    e = object.__new__(PopulationDaily)
    e.dev, e.day_seconds, e.accum_day, e.n_firings = dev, day_eco, 0.0, 0
    sim.routing, sim.phyto_daily, sim.eco_daily = r, p, e
    return sim


def reference_loop(t0, dt, n, day_phyto, day_eco, dt_hydro):
    """The reference driver's loop, statement by statement (the lines of the module docstring)."""
    time_steps = np.arange(t0, t0 + (n - 0.5) * dt, dt)
    assert len(time_steps) == n
    accum_t_day, phyto_next_time, t_accum = 0.0, 0.0, 0.0
    eco, phy, ev = [], [], []
    for i, t in enumerate(time_steps):
        accum_t_day += dt
        k = 0
        while accum_t_day >= day_eco:
            accum_t_day -= day_eco
            k += 1
        eco.append(k)
        if t >= phyto_next_time:
            phy.append(1)
            phyto_next_time = t + day_phyto
        else:
            phy.append(0)
        t_accum += float(dt)
        if t_accum + 1e-9 < dt_hydro:
            ev.append(0.0)
        else:
            ev.append(t_accum)
            t_accum = 0.0
    return dict(times=[float(t) for t in time_steps], eco=eco, phyto=phy, route=ev, accum_day=accum_t_day, next_time=phyto_next_time,
                t_accum=t_accum)


def run(cuts, t0, dt, day_phyto, day_eco, dt_hydro):
    sim = make_sim(t0, dt, day_phyto, day_eco, dt_hydro)
    for n in cuts:
        sim._run_chunk(n)
    lib = sim.dev.lib
    assert lib.spans == list(cuts) and sim._step_index == sum(cuts)
    assert sim.phyto_daily.n_steps == sum(lib.sched["qd_phyto_daily_schedule"]) and sim.eco_daily.n_firings == sum(lib.sched["qd_eco_daily_schedule"])
    return dict(times=sim.forcing.times, eco=[int(x) for x in lib.sched["qd_eco_daily_schedule"]],
                phyto=[int(x) for x in lib.sched["qd_phyto_daily_schedule"]], route=[float(x) for x in lib.sched["qd_route_schedule"]],
                accum_day=sim.eco_daily.accum_day, next_time=sim.phyto_daily.phyto_next_time, t_accum=sim.routing.t_accum), sim.t


def partitions(n, seed, count=6):
    rng = np.random.default_rng(seed)
    out = [[n], [1] * n, [1, n - 1], [n - 1, 1]]
    for _ in range(count):
        cuts = np.sort(rng.choice(np.arange(1, n), size=int(rng.integers(1, 12)), replace=False))
        out.append([int(x) for x in np.diff(np.concatenate([[0], cuts, [n]]))])
    return out


# dt, then in units of dt: the phytoplankton day, the vegetation day (clocks of their own), the routing window
CLOCKS = {
    "dt300": (300.0, 11.37, 8.0, 7.0),
    "dt3600_planet_day": (3600.0, PLANET_DAY / 3600.0, PLANET_DAY / 3600.0, 6.0),
    "dt123.4_not_binary": (123.4, 7.3, 9.0, 2.7),
    "dt123.4_equal_to_the_day": (123.4, 1.0, 1.0, 1.0),
    "dt300_equal_to_the_day": (300.0, 1.0, 1.0, 3.0),
    "dt123.4_is_2.5_days": (123.4, 0.4, 0.4, 0.4),
    "dt3600_is_2.5_days": (3600.0, 0.4, 0.4, 0.7),
}
EPOCHS = {"t0_zero": 0.0, "t0_epoch": 1234.5678 * PLANET_DAY, "t0_small": 0.1}


@pytest.mark.parametrize("epoch", EPOCHS)
@pytest.mark.parametrize("clock", CLOCKS)
def test_any_partition_gives_the_reference_loops_schedules_cpu(clock, epoch):
    dt, day_phyto, day_eco, dt_hydro = CLOCKS[clock][0], *(m * CLOCKS[clock][0] for m in CLOCKS[clock][1:])
    t0 = EPOCHS[epoch]
    want = reference_loop(t0, dt, N, day_phyto, day_eco, dt_hydro)
    assert sum(want["eco"]) >= 2 and sum(want["phyto"]) >= 2 and np.count_nonzero(want["route"]) >= 2
    if day_eco < dt:
        assert max(want["eco"]) >= 2                              # dt > day: more than one firing in a step
    t_end = float(np.arange(t0, t0 + (N + 0.5) * dt, dt)[N])
    for cuts in partitions(N, seed=sum(map(ord, clock + epoch))):
        got, t = run(cuts, t0, dt, day_phyto, day_eco, dt_hydro)
        for k in want:
            assert got[k] == want[k], (cuts, k)
        assert t == t_end, (cuts, t, t_end)


def test_the_three_functions_alone_cpu():
    """The same, on the bare functions: each continues from the clock it returned."""
    dt, day = 123.4, 7.3 * 123.4
    want = reference_loop(0.0, dt, N, day, day, 2.7 * dt)
    for cuts in partitions(N, seed=5):
        a, nt, k0, eco, phy = 0.0, 0.0, 0, [], []
        r = object.__new__(RiverRouting)
        r.dt_hydro_seconds, r.t_accum, r._steps = 2.7 * dt, 0.0, 0
        ev = []
        for n in cuts:
            f, a = daily_counts(a, dt, n, day)
            eco += [int(x) for x in f]
            f, nt = daily_schedule(nt, np.asarray(want["times"][k0:k0 + n]), dt, n, day)
            phy += [int(x) for x in f]
            ev += [float(x) for x in r.schedule(dt, n)]
            k0 += n
        assert (eco, phy, ev, a, nt, r.t_accum) == (want["eco"], want["phyto"], want["route"], want["accum_day"], want["next_time"], want["t_accum"])
        assert r._steps == N
    # a scalar t0 is the span's first time, the rest follows as t0 + dt * arange(n)
    f, nt = daily_schedule(0.0, 0.0, 300.0, 20, 1500.0)
    assert list(f) == [1, 0, 0, 0, 0] * 4 and nt == 4500.0 + 1500.0


def test_time_is_settable_and_restarts_the_count_cpu():
    """Assigning Simulation.t (a restart, QD_ORBIT_EPOCH_*) makes that value the origin of the following steps."""
    sim = make_sim(0.0, 123.4, 1e9, 1e9, 1e9)
    sim._run_chunk(5)
    sim.t = 1000.25
    sim._run_chunk(3)
    sim._run_chunk(2)
    assert sim.forcing.times[5:] == [float(x) for x in np.arange(1000.25, 1000.25 + 4.5 * 123.4, 123.4)]
    sim.dt = 300.0                                              # a changed step restarts the count from the current time as well
    t = sim.t
    sim._run_chunk(2)
    assert sim.forcing.times[10:] == [t, t + 300.0] and sim.t == t + 600.0
