"""GPU (-m gpu): the network generator (qd_hydronet.hip) on the hostile-terrain cases of tests/hydronet_cases.py -- every
goldened case bit for bit against the reference's generator, the wide cases (pit-fill LDS beyond 64 KiB and up to the limit, a lane with two chunks, a thousand Kahn generations) against the restatements of tests/hydronet_ref.py, determinism
across the enlarged-LDS launch, the refusal one column past the limit, and the device-built network handed to the device router
(qd_route.hip) against the sequential restatement of tests/routing_ref.py.

The flow order's `placed < n_land` branch has no case: D8 cannot produce a cycle through the public entry (hydronet_cases)."""
import os

import numpy as np
import pytest

import qingdai_amd as qa
import hydronet_cases as hc
import hydronet_ref as hr
from qingdai_amd.device import Device
from qingdai_amd.hydronet import HydroNetError, generate_network, host_tables
from qingdai_amd.routing import RiverRouting, cell_area_rows, network_from_vars
from routing_ref import SeqRouting

pytestmark = pytest.mark.gpu

HERE = os.path.dirname(os.path.abspath(__file__))
STAGES = ("flow_to_index", "flow_order", "lake_mask", "lake_id", "lake_outlet_index")
ROUTED = ("land_mask", "flow_to_index", "flow_order", "lake_mask", "lake_id", "lake_outlet_index")


def _bits(a):
    return np.ascontiguousarray(a, dtype=np.float64).view(np.uint64)


def _golden(name):
    return np.load(os.path.join(HERE, "golden", f"hydronet_{name}.npz"))


def _build(name, dev=None):
    r = hc.restated(name)
    grid = qa.SphericalGrid(*r["elevation"].shape)
    own = dev is None
    if own:
        dev = Device(grid)
    net = generate_network(grid, r["land"], r["elevation"], eps=r["eps"], max_iters=r["max_iters"], dev=dev)
    if own:
        dev.close()
    return net


def _assert_dtypes(net):
    assert net["flow_to_index"].dtype == np.int64 and net["flow_order"].dtype == np.int64
    assert net["lake_mask"].dtype == np.uint8 and net["lake_id"].dtype == np.int32 and net["lake_outlet_index"].dtype == np.int32


@pytest.mark.parametrize("name", list(hc.GOLDENED))
def test_case_golden_bitwise(gpu, name):
    z = _golden(name)
    shape, land, elev, eps, max_iters = hr.case_inputs(z)
    grid = qa.SphericalGrid(*shape)
    dev = Device(grid)
    net = generate_network(grid, land, elev, eps=eps, max_iters=max_iters, dev=dev)
    dev.close()
    assert net["sweeps"] == int(z["sweeps"])
    assert np.array_equal(_bits(net["elevation_filled"]), _bits(hr.golden_filled(z, elev)))
    for k in STAGES:
        assert np.array_equal(net[k], z[k]), k
    _assert_dtypes(net)
    assert np.array_equal(net["land_mask"], land) and net["n_lakes"] == int(z["n_lakes"])


def _assert_equals_restated(net, r):
    assert net["sweeps"] == r["sweeps"]
    assert np.array_equal(_bits(net["elevation_filled"]), _bits(r["elevation_filled"]))
    for k in STAGES:
        assert np.array_equal(net[k], r[k]), k
    _assert_dtypes(net)
    assert net["n_lakes"] == r["n_lakes"]


@pytest.mark.parametrize("name", list(hc.RESTATED))
def test_wide_case_equals_restatements(gpu, name):
    """13 rows are accepted by the handle, so no shape had to move for that; the V-plane is 4320 columns wide (hydronet_cases)."""
    _assert_equals_restated(_build(name), hc.restated(name))


def test_widest_row_twice_then_a_small_grid(gpu):
    """The widest launch (160 KiB of LDS but 4 B) twice on one handle is bit-identical, and a fresh handle's build within the
    default LDS is right after it."""
    name = "wide_13x4846"
    r = hc.restated(name)
    dev = Device(qa.SphericalGrid(*r["elevation"].shape))
    a = _build(name, dev)
    b = _build(name, dev)
    dev.close()
    for k in ("elevation_filled",) + STAGES:
        assert np.array_equal(np.asarray(a[k]).view(np.uint8), np.asarray(b[k]).view(np.uint8)), k
    assert a["sweeps"] == b["sweeps"] and a["n_lakes"] == b["n_lakes"]
    _assert_equals_restated(b, r)
    z = np.load(os.path.join(HERE, "golden", "hydronet_zero_19x36.npz"))
    shape, land, elev, eps, max_iters = hr.case_inputs(z)
    grid = qa.SphericalGrid(*shape)
    dev = Device(grid)
    net = generate_network(grid, land, elev, eps=eps, max_iters=max_iters, dev=dev)
    dev.close()
    assert net["sweeps"] == int(z["sweeps"])
    assert np.array_equal(_bits(net["elevation_filled"]), _bits(hr.golden_filled(z, elev)))
    for k in STAGES:
        assert np.array_equal(net[k], z[k]), k


def test_one_column_past_the_lds_limit_is_refused(gpu):
    """13 x 4847 needs 163 613 B of LDS rows, 29 B more than the kernel's static LDS leaves of 160 KiB, and is refused on the
    host, before any launch.  A handle builds its own grid only, so no build of that handle can succeed: it must go on
    answering (the next call gets the refusal that is due to it, not a stale one), and the next build, of the widest accepted
    row on a handle of its own, succeeds."""
    n_lat, n_lon = 13, 4847
    assert hc.pitfill_lds_bytes(n_lat, n_lon) > hc.LDS_LIMIT >= hc.pitfill_lds_bytes(n_lat, n_lon - 1)
    grid = qa.SphericalGrid(n_lat, n_lon)
    dev = Device(grid)
    land = np.ones((n_lat, n_lon), np.uint8)
    land[0] = 0
    elev = np.tile(10.0 * np.arange(n_lat)[:, None], (1, n_lon))
    with pytest.raises(HydroNetError, match="too large"):
        generate_network(grid, land, elev, max_iters=2, dev=dev)
    with pytest.raises(HydroNetError, match="non-finite"):
        generate_network(grid, land, np.full((n_lat, n_lon), np.nan), dev=dev)
    with pytest.raises(HydroNetError, match="too large"):
        generate_network(grid, land, elev, max_iters=2, dev=dev)
    dev.close()
    n_lon -= 1
    grid = qa.SphericalGrid(n_lat, n_lon)
    dev = Device(grid)
    net = generate_network(grid, land[:, 1:], elev[:, 1:], max_iters=2, dev=dev)
    dev.close()
    # a plane that falls to the ocean row: nothing to fill, and row 1 is one lake on the shore
    assert net["sweeps"] == 1 and np.array_equal(net["elevation_filled"], elev[:, 1:])
    assert net["n_lakes"] == 1 and net["lake_outlet_index"].tolist() == [-1] and net["lake_mask"][1].all()
    flow = hr.d8(*host_tables(grid), land[:, 1:], elev[:, 1:])
    assert np.array_equal(net["flow_to_index"], flow) and np.array_equal(net["flow_order"], hr.flow_order(flow, land[:, 1:]))


def _close(got, want, scale):
    assert abs(got - want) <= 1e-12 * max(abs(scale), 1e-300), (got, want)


@pytest.mark.parametrize("name", ["seam_valley_rise_9x272", "inland_37x72", "vplane_13x4320"])
def test_generated_network_routes_like_the_sequential_router(gpu, name):
    """The generator's own arrays (lakes of many cells, outlets it chose) into RiverRouting.from_arrays on the same handle,
    two routing events, against SeqRouting with the tolerances of test_gpu_routing.test_fullsize_network_two_events."""
    if name in hc.CASES:
        r = hc.restated(name)
        land, elev, eps, max_iters = r["land"], r["elevation"], r["eps"], r["max_iters"]
    else:
        _, land, elev, eps, max_iters = hr.case_inputs(_golden(name))
    n_lat, n_lon = elev.shape
    grid = qa.SphericalGrid(n_lat, n_lon)
    dev = Device(grid)
    net = generate_network(grid, land, elev, eps=eps, max_iters=max_iters, dev=dev)
    v = {k: net[k] for k in ROUTED}
    assert net["n_lakes"] > 0
    rr = RiverRouting.from_arrays(grid, dt_hydro_hours=1.0, diag=False, dev=dev, **v)
    seq = SeqRouting(network_from_vars(v, (n_lat, n_lon)), cell_area_rows(grid), rr.dt_hydro_seconds)
    rng = np.random.default_rng(3)
    n_ev = 0
    for k in range(8):
        R = rng.uniform(-1e-6, 2e-5, (n_lat, n_lon))
        P = rng.uniform(0, 4e-5, (n_lat, n_lon))
        E = rng.uniform(0, 3e-5, (n_lat, n_lon))
        rr.step(R, 900.0, precip_flux=P, evap_flux=E)
        want = seq.step(R, 900.0, P, E)
        if want is None:
            continue
        n_ev += 1
        d = rr.diagnostics()
        np.testing.assert_array_equal(d["flow_accum_kgps"], want["flow"])
        _close(d["ocean_inflow_kgps"], want["ocean_inflow_kgps"], want["ocean_inflow_kgps"])
        _close(d["mass_closure_error_kg"], want["mass_closure_error_kg"], want["mass_input_kg"])
        np.testing.assert_allclose(d["lake_volume_kg"], want["lake_volume_kg"], rtol=1e-12, atol=1e-12 * want["mass_input_kg"])
    assert n_ev == 2
    rr.close()
    dev.close()
