"""GPU (-m gpu): the daily phytoplankton step (P017, PhytoManager.step_daily, pygcm/ecology/phyto.py:339-435) on the resident
tracers (qd_phyto_daily_*): stand-alone against the reference's goldens, its in-kernel insolation against k_forcing's, 721 x 1440
against the NumPy restatement, inside qd_step_n (bit8) against DriverOracle, the driver's [PhytoDiag] lines, a configured but
unused daily state, and the refusal on a banded handle."""
import ctypes
import glob
import os

import numpy as np
import pytest

import phyto_daily_ref as ref
from util import relerr

pytestmark = pytest.mark.gpu

HERE = os.path.dirname(os.path.abspath(__file__))
GOLDENS = sorted(glob.glob(os.path.join(HERE, "golden", "phyto_daily_*.npz")))


def _clean_env(monkeypatch):
    for k in [k for k in os.environ if k.startswith(("QD_PHYTO_", "QD_ECO_", "QD_STAR_"))]:
        monkeypatch.delenv(k)


def _daily_on(dev, grid, mask, S, H, C0=None, N0=None, **kw):
    from qingdai_amd.phyto import PhytoDaily, PhytoTracers
    tr = PhytoTracers(grid, mask, dev=dev)
    if C0 is not None:
        dev.phyto_upload(C0)
    pd = PhytoDaily(tr, H_mld_m=H, diag=False, dev=dev, **kw)
    if N0 is not None:
        pd.N = N0
    assert pd.S == S
    return tr, pd


@pytest.mark.parametrize("path", GOLDENS, ids=lambda p: os.path.basename(p)[12:-4])
def test_standalone_vs_reference_goldens(gpu, path, monkeypatch):
    import qingdai_amd as qa
    from qingdai_amd.device import Device
    z = np.load(path)
    _clean_env(monkeypatch)
    for k, v in zip(z["env_keys"], z["env_vals"]):
        monkeypatch.setenv(str(k), str(v))
    nlat, nlon, n = int(z["n_lat"]), int(z["n_lon"]), int(z["n_days"])
    grid = qa.SphericalGrid(nlat, nlon)
    mask = z["land_mask"]
    dev = Device(grid)
    dev.upload_now("LAND_MASK", mask)
    S = z["C0"].shape[0]
    tr, pd = _daily_on(dev, grid, mask, S, float(z["H_arg"]), C0=z["C0"], N0=z["N0"])
    land = mask == 1
    errs = {}
    for d in range(n):
        dev.upload_now("SST", z["T_w"][d])
        pd.step_daily(z["stars"][d], use_sst=True)
        for tag, day, tol in (("first", 0, 1e-12), ("last", n - 1, 1e-10)):
            if d != day:
                continue
            bands, scalar = pd.get_alpha_maps()
            got = {"C": tr.C_phyto_s, "N": pd.N, "alpha_bands": bands, "alpha_scalar": scalar, "kd490": pd.get_kd490()}
            for k, v in got.items():
                e = relerr(v, z[f"{tag}_{k}"])
                errs[(tag, k)] = e
                assert e < tol, (tag, k, e)
            assert np.all(got["C"][:, land] == 0.0) and np.all(got["N"][land] == 0.0)
    print(os.path.basename(path), {f"{a}/{b}": f"{e:.1e}" for (a, b), e in errs.items()})
    assert pd.n_steps == n and dev.phyto_daily_steps() == n
    dev.close()


def test_in_kernel_insolation_is_bitwise_k_forcing(gpu):
    import qingdai_amd as qa
    from qingdai_amd.device import Device
    grid = qa.SphericalGrid(91, 180)
    dev = Device(grid)
    forcing = qa.ThermalForcing(grid, qa.OrbitalSystem())
    dp = ctypes.POINTER(ctypes.c_double)
    for t in (0.0, 12345.0 * 300.0, 7.7e7):
        st = np.ascontiguousarray(forcing.star_table([t])[0])
        dev.forcing(st[0:3], st[3:6], st[6], with_teq=False)
        isrA, isrB = dev.get("ISR_A").copy(), dev.get("ISR_B").copy()
        a = np.empty(dev.shape); b = np.empty(dev.shape)
        dev._chk(dev.lib.qd_phyto_daily_insolation(dev.h, st.ctypes.data_as(dp), a.ctypes.data_as(dp), b.ctypes.data_as(dp)),
                 "qd_phyto_daily_insolation")
        assert np.array_equal(a, isrA) and np.array_equal(b, isrB)
        assert np.count_nonzero(a) > 0 and np.count_nonzero(a == 0.0) > 0
        # the host restatement agrees to rounding (NumPy's cos vs the device's)
        ra, rb = ref.insolation(st, grid.lat, grid.lon)
        assert relerr(a, ra) < 1e-13 and relerr(b, rb) < 1e-13
    dev.close()


def test_full_size_one_day_vs_restatement(gpu, monkeypatch):
    import qingdai_amd as qa
    from qingdai_amd.device import Device
    from qingdai_amd.phyto import daily_tables
    from qingdai_amd.topography import create_land_sea_mask
    _clean_env(monkeypatch)
    grid = qa.SphericalGrid(721, 1440)
    mask = create_land_sea_mask(grid)
    dev = Device(grid)
    dev.upload_now("LAND_MASK", mask)
    r = np.random.default_rng(7)
    S = 10
    C0 = np.abs(r.lognormal(np.log(0.005), 0.7, (S, 721, 1440))) * (mask == 0)
    N0 = np.where(mask == 0, r.uniform(0.0, 2.0, (721, 1440)), 0.0)
    Tw = 285.0 + 15.0 * np.cos(np.deg2rad(grid.lat_mesh)) ** 2
    tr, pd = _daily_on(dev, grid, mask, S, 50.0, C0=C0, N0=N0)
    dev.upload_now("TS", Tw)
    forcing = qa.ThermalForcing(grid, qa.OrbitalSystem())
    st = forcing.star_table([3.0e6])[0]
    dev.timing(True, select="phyto_daily")
    pd.step_daily(st, use_sst=False)
    dev.sync()
    a = np.empty(dev.shape); b = np.empty(dev.shape)
    dp = ctypes.POINTER(ctypes.c_double)
    stc = np.ascontiguousarray(st)
    dev._chk(dev.lib.qd_phyto_daily_insolation(dev.h, stc.ctypes.data_as(dp), a.ctypes.data_as(dp), b.ctypes.data_as(dp)), "insolation")
    tab = ref.tables_from_host(daily_tables(S, H_mld_m=50.0))
    want = ref.step_daily(C0, N0, a, b, Tw, tab, mask)
    bands, scalar = pd.get_alpha_maps()
    got = {"C": tr.C_phyto_s, "N": pd.N, "alpha_bands": bands, "alpha_scalar": scalar, "kd490": pd.get_kd490()}
    errs = {k: relerr(v, want[k]) for k, v in got.items()}
    print("721x1440 one day:", {k: f"{e:.1e}" for k, e in errs.items()}, "kernel ms", dev.timing_get("phyto_daily"))
    assert max(errs.values()) < 1e-12, errs
    land = mask == 1
    assert np.all(got["C"][:, land] == 0.0) and np.all(got["N"][land] == 0.0)
    dev.close()


class _DailyCoupling:
    """An EcoCoupling whose apply runs the restatement on the firing steps (atm.isr_A / isr_B, T_w = ocean.Ts or atm.T_s, C before
    this step's transport) and then overrides the ocean base albedo with the result, as run_simulation.py:2051-2061,2121-2128 do."""

    def __init__(self, d, tab, mask, C, N, fire, couple=True):
        from qd_oracle.ecology import EcoCoupling
        self.base = EcoCoupling(None)
        self.d, self.tab, self.mask, self.C, self.N = d, tab, mask, C, N
        self.fire, self.k, self.couple = list(fire), 0, couple
        self.means = []

    def apply(self, base_in, land, glacier, isr, dt):
        d = self.d
        if self.fire[self.k]:
            Tw = d.ocean.Ts if d.ocean is not None else d.atm.T_s
            r = ref.step_daily(self.C, self.N, d.atm.isr_A, d.atm.isr_B, Tw, self.tab, self.mask)
            self.C, self.N = r["C"], r["N"]
            self.means.append(r["means"])
            if self.couple:
                self.base.ocean_alpha = r["alpha_scalar"]
        self.k += 1
        return self.base.apply(base_in, land, glacier, isr, dt)


@pytest.mark.parametrize("with_ocean,transport", [(True, True), (True, False), (False, False)])
def test_inside_the_resident_loop_vs_oracle(gpu, with_ocean, transport, monkeypatch):
    import qd_oracle as qo
    from qd_oracle.driver import DriverOracle
    from qd_oracle import phyto as ophyto
    import qingdai_amd as qa
    from qingdai_amd.phyto import daily_tables
    from qingdai_amd.topography import create_land_sea_mask, generate_base_properties
    _clean_env(monkeypatch)
    monkeypatch.setenv("QD_PHYTO_NSPECIES", "4")
    nlat, nlon, S, nsteps, dt = 37, 72, 4, 14, 300.0
    over = dict(energy_w=1.0, cloud_couple=1)
    grid = qa.SphericalGrid(nlat, nlon)
    mask = create_land_sea_mask(grid)
    base_albedo, friction = generate_base_properties(mask)
    Cs_ocean = 1000.0 * 4200.0 * 50.0
    csmap = np.where(mask == 1, 3e6, Cs_ocean).astype(float)
    m = qa.SpectralModel(grid, friction, H=8000, tau_rad=10 * 24 * 3600, greenhouse_factor=0.40, C_s_map=csmap, land_mask=mask,
                         Cs_ocean=Cs_ocean, Cs_land=3e6, Cs_ice=5e6, params=qa.QdParams(**over))
    if with_ocean:
        qa.WindDrivenSlabOcean(grid, mask, 50.0, init_Ts=np.full((nlat, nlon), 288.0))
    dev = m._dev
    dev.upload_now("BASE_ALBEDO", base_albedo)
    r = np.random.default_rng(3)
    C0 = np.abs(r.lognormal(np.log(0.3), 0.5, (S, nlat, nlon))) * (mask == 0)
    N0 = np.where(mask == 0, r.uniform(0.2, 2.0, (nlat, nlon)), 0.0)
    tr, pd = _daily_on(dev, grid, mask, S, 50.0, C0=C0, N0=N0, day_seconds=5 * dt)
    forcing = qa.ThermalForcing(grid, qa.OrbitalSystem())
    times = [i * dt for i in range(nsteps)]
    from qingdai_amd.phyto import daily_schedule
    fire, _ = daily_schedule(0.0, 0.0, dt, nsteps, 5 * dt)
    assert list(np.nonzero(fire)[0]) == [0, 5, 10]
    # two spans, the second one starting inside a day
    k = 7
    dev.step_n(forcing.star_table(times[:k]), dt, with_ocean=with_ocean, with_physics=True, pass_albedo=True, phyto=transport,
               phyto_daily=pd, t0=0.0)
    log1 = dev.phyto_daily_log()
    dev.step_n(forcing.star_table(times[k:]), dt, with_ocean=with_ocean, with_physics=True, pass_albedo=True, phyto=transport,
               phyto_daily=pd, t0=times[k])
    log = np.concatenate([log1, dev.phyto_daily_log()])
    g = qo.Grid(nlat, nlon)
    P = qo.defaults(**over)
    om = qo.AtmosOracle(g, friction, mask, P, C_s_map=csmap)
    oo = qo.OceanOracle(g, mask, P, init_Ts=np.full((nlat, nlon), 288.0)) if with_ocean else None
    d = DriverOracle(g, om, oo, qo.Forcing(g), mask, base_albedo, P)
    tab = ref.tables_from_host(daily_tables(S, H_mld_m=50.0))
    cpl = _DailyCoupling(d, tab, mask, C0, N0, fire)
    d.eco = cpl
    for i in range(nsteps):
        d.step(times[i], dt, pass_albedo=True, commit=False)
        if transport:
            cpl.C = ophyto.advect_diffuse(cpl.C, oo.uo, oo.vo, dt, g, mask, K_h=5.0e3, adv_alpha=0.7)
    errs = {"albedo": relerr(dev.get("ALBEDO"), d.albedo), "T_s": relerr(dev.get("TS"), om.T_s),
            "C": relerr(tr.C_phyto_s, cpl.C), "N": relerr(pd.N, cpl.N)}
    if with_ocean:
        errs["SST"] = relerr(dev.get("SST"), oo.Ts)
    print(f"ocean={with_ocean} transport={transport}:", {k: f"{e:.1e}" for k, e in errs.items()})
    assert max(errs.values()) < 1e-9, errs
    assert log.shape == (3, 4) and list(log[:, 0]) == [1.0, 2.0, 3.0]
    assert np.allclose(log[:, 1:], np.array(cpl.means), rtol=1e-10)
    ocean = mask == 0
    assert relerr(cpl.C, C0) > 1e-3
    # the ocean base albedo follows the daily alpha (ocean cells without ice and cloud would show it)
    assert relerr(dev.get("WATER_ALPHA"), cpl.base.ocean_alpha) < 1e-12 and np.all(np.isfinite(dev.get("ALBEDO")[ocean]))
    dev.close()


def test_configured_but_unused_is_bit_identical(gpu, monkeypatch):
    import qingdai_amd as qa
    from qingdai_amd.topography import create_land_sea_mask, generate_base_properties
    _clean_env(monkeypatch)
    monkeypatch.setenv("QD_PHYTO_NSPECIES", "3")
    nlat, nlon, dt = 37, 72, 300.0
    grid = qa.SphericalGrid(nlat, nlon)
    mask = create_land_sea_mask(grid)
    base_albedo, friction = generate_base_properties(mask)
    forcing = qa.ThermalForcing(grid, qa.OrbitalSystem())
    stars = forcing.star_table([i * dt for i in range(6)])
    out = []
    for configure in (False, True):
        m = qa.SpectralModel(grid, friction, H=8000, tau_rad=10 * 24 * 3600, greenhouse_factor=0.40, land_mask=mask,
                             params=qa.QdParams(energy_w=1.0, cloud_couple=1))
        qa.WindDrivenSlabOcean(grid, mask, 50.0, init_Ts=np.full((nlat, nlon), 288.0))
        dev = m._dev
        dev.upload_now("BASE_ALBEDO", base_albedo)
        if configure:
            _daily_on(dev, grid, mask, 3, 50.0)
            dev.upload_now("WATER_ALPHA", np.full((nlat, nlon), 0.5))     # would change the albedo if it were blended
        else:
            from qingdai_amd.phyto import PhytoTracers
            PhytoTracers(grid, mask, dev=dev)
        dev.step_n(stars, dt, with_ocean=True, with_physics=True, pass_albedo=False, with_hydrology=True, phyto=True)
        out.append({f: dev.get(f).copy() for f in ("ALBEDO", "TS", "SST", "U", "H", "Q", "CLOUD", "W_LAND")})
        dev.close()
    for f in out[0]:
        assert np.array_equal(out[0][f], out[1][f]), f


def test_driver_prints_phytodiag_lines(gpu, monkeypatch, capsys, tmp_path):
    from qingdai_amd.driver import Simulation
    _clean_env(monkeypatch)
    monkeypatch.setenv("QD_PHYTO_DAILY", "1")
    monkeypatch.setenv("QD_PHYTO_NSPECIES", "4")
    monkeypatch.setenv("QD_DT_SECONDS", "3600")           # 20 steps per planet-day
    monkeypatch.setenv("QD_ECO_ENABLE", "0")
    sim = Simulation(n_lat=37, n_lon=72, quiet=True)
    assert sim.phyto_daily is not None and sim.phyto_transport
    out = capsys.readouterr().out
    assert "[Phyto] NB=16 bands, H_mld=50.0 m | S=4" in out and "[Phyto] Manager initialized." in out
    for n in (13, 13, 13, 2):                              # steps 0 .. 40: fires on 0, 20, 40
        sim.run_steps(n)
    out = capsys.readouterr().out
    lines = [ln for ln in out.splitlines() if ln.startswith("[PhytoDiag] S=4 | ⟨Chl_tot⟩=")]
    assert len(lines) == 3, out
    assert sim.phyto_daily.n_steps == 3
    sim.save_autosave(str(tmp_path))
    from qingdai_amd import ncio
    v, attrs = ncio.read_nc(str(tmp_path / "plankton.nc"))
    assert {"C_phyto_s", "alpha_water_bands", "alpha_water_scalar", "Kd_490", "N", "bands_lambda_centers"} <= set(v)
    assert int(attrs["NB"]) == 16 and float(attrs["H_mld_m"]) == 50.0
    # without the ocean the daily step still runs (on T_s), the transport does not
    monkeypatch.setenv("QD_USE_OCEAN", "0")
    sim2 = Simulation(n_lat=19, n_lon=36, quiet=True)
    assert sim2.phyto_daily is not None and not sim2.phyto_transport
    sim2.run_steps(3)
    assert sim2.phyto_daily.n_steps == 1
    sim.dev.close(); sim2.dev.close()


def test_banded_handle_refuses(gpu, monkeypatch):
    import qingdai_amd as qa
    from qingdai_amd.device import Device
    from qingdai_amd.phyto import PhytoDaily, PhytoTracers
    _clean_env(monkeypatch)
    grid = qa.SphericalGrid(73, 144)
    mask = np.zeros((73, 144), dtype=np.uint8)
    dev = Device(grid, row0=20, n_rows=30, halo=6)
    tr = PhytoTracers(grid, mask, dev=dev)
    with pytest.raises(qa._lib.QdError, match="whole-globe"):
        PhytoDaily(tr, diag=False, dev=dev)
    st = np.zeros(7)
    dp = ctypes.POINTER(ctypes.c_double)
    assert dev.lib.qd_phyto_daily(dev.h, st.ctypes.data_as(dp), 1) != 0
    assert b"whole-globe" in dev.lib.qd_last_error(dev.h)
    stars = np.zeros((1, 7))
    rc = dev.lib.qd_step_n(dev.h, 1, 300.0, 2 | 256, stars.ctypes.data_as(dp))
    assert rc != 0 and b"whole-globe" in dev.lib.qd_last_error(dev.h)
    dev.close()
