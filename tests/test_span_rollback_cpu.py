"""Device.step_n with span participants (river routing, the daily phytoplankton step) around a stub library: no GPU, no
libqingdai_hip.so.  A failing schedule upload or a failing span leaves every participant's host clock where it was before the call;
a span that ran advances the clocks exactly as schedule() alone does and reaches qd_step_n once."""
import ctypes

import numpy as np
import pytest

from qingdai_amd._lib import QdError
from qingdai_amd.device import Device
from qingdai_amd.phyto import PhytoDaily
from qingdai_amd.routing import RiverRouting

N, DT, T0 = 30, 300.0, 500.0
CALLS = ("qd_phyto_daily_schedule", "qd_route_schedule", "qd_step_n")


class StubLib:
    """The three entry points step_n reaches, each returning the code programmed for it."""

    def __init__(self, fail=None):
        self.fail = fail
        self.calls = []

    def _entry(self, name):
        def fn(h, *args):
            self.calls.append((name, args))
            return -1 if name == self.fail else 0
        return fn

    def __getattr__(self, name):
        if name in CALLS:
            return self._entry(name)
        raise AttributeError(name)

    def qd_last_error(self, h):
        return b"programmed failure"

    def qd_destroy(self, h):
        return 0


def make_device(fail=None):
    dev = object.__new__(Device)
    dev.lib, dev.h, dev._host = StubLib(fail), ctypes.c_void_p(1), {}
    return dev


def make_routing(dev):
    r = object.__new__(RiverRouting)
    r.dev, r.dt_hydro_seconds, r.t_accum, r._steps = dev, 3600.0, 1200.0, 5
    return r


def make_daily(dev):
    d = object.__new__(PhytoDaily)
    d.dev, d.day_seconds, d.phyto_next_time, d.n_steps = dev, 3000.0, 1000.0, 2
    return d


def run(dev, routing, daily):
    dev.step_n(np.zeros((N, 7)), DT, with_ocean=True, with_physics=True, with_hydrology=True, routing=routing, phyto_daily=daily, t0=T0)


def participants(who, dev):
    return (make_routing(dev) if who in ("routing", "both") else None, make_daily(dev) if who in ("daily", "both") else None)


@pytest.mark.parametrize("who,fail", [("routing", "qd_route_schedule"), ("routing", "qd_step_n"),
                                      ("daily", "qd_phyto_daily_schedule"), ("daily", "qd_step_n"),
                                      ("both", "qd_phyto_daily_schedule"), ("both", "qd_route_schedule"), ("both", "qd_step_n")])
def test_failure_restores_every_clock_cpu(who, fail):
    dev = make_device(fail)
    routing, daily = participants(who, dev)
    with pytest.raises(QdError, match=fail):
        run(dev, routing, daily)
    if routing is not None:
        assert (routing.t_accum, routing._steps) == (1200.0, 5)
    if daily is not None:
        assert daily.phyto_next_time == 1000.0
        assert daily.n_steps == 2
    assert [c[0] for c in dev.lib.calls].count("qd_step_n") == (1 if fail == "qd_step_n" else 0)


@pytest.mark.parametrize("who", ["none", "routing", "daily", "both"])
def test_success_advances_as_schedule_alone_cpu(who):
    dev = make_device()
    routing, daily = participants(who, dev)
    run(dev, routing, daily)
    steps = [args for name, args in dev.lib.calls if name == "qd_step_n"]
    assert len(steps) == 1
    n, dt, flags = steps[0][:3]
    assert (n, dt) == (N, DT)
    assert bool(flags & 128) == (routing is not None) and bool(flags & 256) == (daily is not None)
    assert flags & ~(128 | 256) == 1 | 2 | 4 | 8                      # pass_albedo is step_n's default
    if routing is not None:
        twin = make_routing(None)
        ev = twin.schedule(DT, N)
        assert np.count_nonzero(ev) > 0
        assert (routing.t_accum, routing._steps) == (twin.t_accum, twin._steps)
    if daily is not None:
        twin = make_daily(None)
        fire = twin.schedule(T0, DT, N)
        assert int(fire.sum()) > 1
        assert daily.phyto_next_time == twin.phyto_next_time
        assert daily.n_steps == 2 + int(fire.sum())


def test_foreign_handle_and_missing_t0_cpu():
    dev = make_device()
    with pytest.raises(ValueError, match="step_n: the RiverRouting runs on another device handle"):
        run(dev, make_routing(make_device()), None)
    with pytest.raises(ValueError, match="step_n: the PhytoDaily runs on another device handle"):
        run(dev, None, make_daily(make_device()))
    daily = make_daily(dev)
    with pytest.raises(ValueError, match="step_n: phyto_daily needs the span's start time t0"):
        dev.step_n(np.zeros((N, 7)), DT, with_physics=True, phyto_daily=daily)
    assert daily.phyto_next_time == 1000.0 and dev.lib.calls == []
