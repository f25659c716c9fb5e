"""CPU: the diversity diagnostics' host side.  The NumPy restatement (tests/diversity_ref.py, the GPU tests' checker) against every
golden of the reference; two wrong neighbourhoods that the goldens must notice; the driver's firing clock and chunking against a
literal replay of the reference's loop; the writer's files; the environment switches; the ABI names."""
import glob
import os

import numpy as np
import pytest

import diversity_ref as ref
from qingdai_amd import _lib
from qingdai_amd.driver import Simulation

HERE = os.path.dirname(os.path.abspath(__file__))
GOLDENS = sorted(glob.glob(os.path.join(HERE, "golden", "diversity_*_19x36.npz")))
DAY = 2 * np.pi / 8.726646259971648e-5


def _case(path):
    return os.path.basename(path)[10:-10]


def _rel(got, want):
    got, want = np.asarray(got, dtype=float), np.asarray(want, dtype=float)
    assert np.array_equal(np.isnan(got), np.isnan(want)), "NaN positions differ"
    ok = np.isfinite(want) & (want != 0)
    assert np.array_equal(got[~ok], want[~ok], equal_nan=True)
    return float(np.max(np.abs(got[ok] - want[ok]) / np.abs(want[ok]), initial=0.0))


def test_the_six_cases_exist():
    assert [_case(p) for p in GOLDENS] == ["mixed", "noland", "nonfinite", "seam", "single", "wide"]
    shapes = {_case(p): np.load(p)["stack"].shape[:2] for p in GOLDENS}
    assert shapes["mixed"] == (20, 2) and shapes["seam"] == (3, 8) and shapes["single"] == (1, 1) and shapes["wide"][0] == 64


@pytest.mark.parametrize("path", GOLDENS, ids=_case)
def test_restatement_vs_reference_goldens(path):
    z = np.load(path)
    with np.errstate(all="ignore"):
        got = ref.diversity(z["stack"], z["land_mask"], ref.lat_mesh(19, 36))
    assert np.array_equal(got["L_s"], z["L_s"], equal_nan=True)                  # no transcendental: bit for bit
    assert np.array_equal(got["bc_local"], z["bc_local"], equal_nan=True)
    assert _rel(got["alpha_map"], z["alpha_map"]) <= 1e-15 and _rel(got["summary"], z["summary"]) <= 1e-15


def test_what_the_cases_cover():
    z = {_case(p): np.load(p) for p in GOLDENS}
    m = z["mixed"]
    land = m["land_mask"] == 1
    bare = land & (m["L_s"].sum(axis=0) == 0)
    assert land[0].any() and land[-1].any() and bare.sum() >= 9 and (~land).sum() > 100
    assert np.isnan(m["alpha_map"][bare]).all() and np.isfinite(m["alpha_map"][land & ~bare]).all()
    assert (m["bc_local"] == 1.0).any() and ((m["L_s"] == 0) & land & ~bare).any()
    s = z["seam"]["land_mask"]
    assert all(s[r, c] == 1 for r in (0, -1) for c in (0, -1)) and ((s[:, 0] == 1) & (s[:, -1] == 1)).sum() >= 9
    assert _rel(z["single"]["summary"], [1.0, 1.0, 1.0]) < 1e-12
    assert np.nanmax(np.abs(z["single"]["alpha_map"] - 1.0)) < 1e-12
    n = z["nonfinite"]
    assert (n["stack"] < 0).any() and np.isnan(n["stack"]).any() and np.isinf(n["stack"]).any() and (n["L_s"][np.isfinite(n["L_s"])] >= 0).all()
    nl = n["land_mask"] == 1
    assert np.isnan(n["bc_local"][nl]).sum() > np.isnan(z["mixed"]["bc_local"][land]).sum() and np.isnan(n["summary"][1:]).all()
    o = z["noland"]
    assert np.isnan(o["alpha_map"]).all() and np.isnan(o["bc_local"]).all() and o["summary"].tolist() == [0.0, 1.0, 1e12]


def test_the_goldens_notice_a_wrong_neighbourhood():
    z = {_case(p): np.load(p) for p in GOLDENS}
    for case in ("seam", "mixed"):
        L_s, land, want = z[case]["L_s"], z[case]["land_mask"], z[case]["bc_local"]
        assert np.array_equal(ref.bray_curtis(L_s, land), want, equal_nan=True)
        flags = {"seam": dict(wrap=False), "mixed": dict(pole_clip=False)}[case]
        assert not np.array_equal(ref.bray_curtis(L_s, land, **flags), want, equal_nan=True), case
    # and each of the two is missed where it should be: the seam columns, the pole rows
    d = ref.bray_curtis(z["seam"]["L_s"], z["seam"]["land_mask"], wrap=False)
    bad = ~((d == z["seam"]["bc_local"]) | (np.isnan(d) & np.isnan(z["seam"]["bc_local"])))
    assert bad[:, [0, -1]].any() and not bad[:, 1:-1].any()
    d = ref.bray_curtis(z["mixed"]["L_s"], z["mixed"]["land_mask"], pole_clip=False)
    bad = ~((d == z["mixed"]["bc_local"]) | (np.isnan(d) & np.isnan(z["mixed"]["bc_local"])))
    assert bad[[0, -1]].any() and not bad[1:-1].any()


def test_weight_row_is_the_reference_factor():
    from qingdai_amd.ecology import diversity_weights
    z = np.load(GOLDENS[0])
    mesh = ref.lat_mesh(19, 36)
    w = ref.area_weights(mesh, z["land_mask"])
    row = diversity_weights(mesh, z["land_mask"] == 1)
    assert row.shape == (19,) and np.array_equal(np.repeat(row[:, None], 36, axis=1), w)


# ------------------------------------------------------------------ the driver's clock
def _reference_loop(t0, n_steps, dt, every):
    """run_simulation.py:1639,1741,2404-2411, literally: time_steps = np.arange(t0, t0 + duration, dt); per step t_days = t / day;
    the diagnostics run when t_days >= next and set next = t_days + every -> [(step, t_days)]."""
    time_steps = np.arange(t0, t0 + n_steps * dt, dt)[:n_steps]
    fired, diversity_next_day = [], [0.0]
    for i, t in enumerate(time_steps):
        t_days = t / DAY
        if t_days >= diversity_next_day[0]:
            fired.append((i, t_days))
            diversity_next_day[0] = t_days + every
    return fired


class _Sim(Simulation):
    """driver.Simulation with the device taken out: a chunk only advances the clock, a firing only moves the threshold."""
    def __init__(self, t0, dt, on, every):
        self.dt, self.day_seconds = dt, DAY
        self.diversity_on, self.diversity_every = on, every
        self.t = t0
        self.chunks, self.fired = [], []

    def run_steps(self, n):
        _, self._t = self._span_times(n)
        self.chunks.append(n)

    def run_diversity(self, t_days):
        self.fired.append((sum(self.chunks) - 1, t_days))
        self.diversity_next_day = t_days + self.diversity_every


def _drive(t0, n_total, dt, on, every, next_autosave=None):
    """The driver's own loop (Simulation.run_loop) -> (chunk lengths, [(step, t_days)] of the firings)."""
    sim = _Sim(t0, dt, on, every)
    sim.run_loop(n_total, next_autosave)
    return sim.chunks, sim.fired


@pytest.mark.parametrize("every", [10.0, 0.5, 0.0, 1.0 / 3.0, -1.0])
@pytest.mark.parametrize("t0", [0.0, 1234.5, 3.7 * DAY + 17.0])
def test_clock_and_chunks_vs_reference_loop(every, t0):
    n_total, dt = 700, 300.0                                    # 2.9 planet-days
    want = _reference_loop(t0, n_total, dt, every)
    chunks, fired = _drive(t0, n_total, dt, True, every)
    assert fired == want                                        # the same steps, the same float64 t_days (the file names' source)
    assert want[0][0] == 0                                      # the first step always fires, after a restart too
    if every <= 0:
        assert [i for i, _ in want] == list(range(n_total)) and chunks == [1] * n_total
    ends = set(np.cumsum(chunks) - 1)
    assert {i for i, _ in want} <= ends and sum(chunks) == n_total and max(chunks) <= 200
    names = [f"diversity_summary_day_{t:05.1f}.txt" for _, t in fired]
    assert names == [f"diversity_summary_day_{t:05.1f}.txt" for _, t in want]


def test_chunks_unchanged_when_disabled():
    from qingdai_amd.driver import chunk_until
    for t0, thr in ((0.0, None), (0.0, 18000.0), (777.0, 5000.0)):
        chunks, fired = _drive(t0, 700, 300.0, False, 0.5, next_autosave=thr)
        assert fired == []
        t, done, old = t0, 0, []
        while done < 700:                                       # the loop as it was: no fire_in argument
            n = chunk_until(t, 300.0, thr, 700 - done)
            old.append(n)
            done += n
            t += n * 300.0
        assert chunks == old
    assert chunk_until(0.0, 300.0, None, 1000) == 200 and chunk_until(0.0, 300.0, None, 1000, fire_in=None) == 200
    assert chunk_until(0.0, 300.0, None, 1000, fire_in=7) == 7 and chunk_until(0.0, 300.0, 900.0, 1000, fire_in=7) == 3
    assert chunk_until(0.0, 300.0, 3000.0, 1000, fire_in=1) == 1


def test_firings_function_vs_reference_loop():
    from qingdai_amd.ecology import diversity_firings
    times = 1234.5 + np.arange(500) * ((1234.5 + 300.0) - 1234.5)
    fired, nxt = diversity_firings(times, DAY, 0.0, 1.0 / 3.0)
    want = _reference_loop(1234.5, 500, 300.0, 1.0 / 3.0)
    assert fired == [i for i, _ in want] and nxt == want[-1][1] + 1.0 / 3.0


# ------------------------------------------------------------------ files, environment, ABI
def test_writer_files(tmp_path):
    from qingdai_amd.ecology import write_diversity_files
    z = np.load([p for p in GOLDENS if "mixed" in p][0])
    summary = dict(zip(("alpha_mean", "gamma_eff", "beta_whittaker"), z["summary"]))
    paths = write_diversity_files(str(tmp_path / "out"), 12.3456, z["alpha_map"], z["bc_local"], z["L_s"], summary, z["land_mask"].astype(np.int64))
    eco = tmp_path / "out" / "ecology"
    assert sorted(os.listdir(eco)) == ["community_day_012.3.npz", "diversity_maps_day_012.3.npz", "diversity_summary_day_012.3.txt"]
    assert [os.path.basename(p) for p in paths] == ["diversity_summary_day_012.3.txt", "community_day_012.3.npz", "diversity_maps_day_012.3.npz"]
    raw = open(eco / "diversity_summary_day_012.3.txt", "rb").read()
    a, g, b = z["summary"]
    abar = "\u03b1\u0304"                                       # the reference writes alpha + a combining macron, not a precomposed letter
    want = (f"Day: 12.35\n" + f"Whittaker beta (\u03b2 = \u03b3/{abar}): {b:.4f}\n" + f"  alpha_mean ({abar}): {a:.4f}\n" +
            f"  gamma_eff  (\u03b3 ): {g:.4f}\n")
    assert raw == want.encode("utf-8") and raw.count(b"\n") == 4
    assert "16.5885" in want and "19.9151" in want and "1.2005" in want
    c = np.load(eco / "community_day_012.3.npz")
    assert sorted(c.files) == ["L_s", "land_mask"] and c["L_s"].dtype == np.float32 and c["land_mask"].dtype == np.int8
    assert np.array_equal(c["L_s"], z["L_s"].astype(np.float32)) and np.array_equal(c["land_mask"], z["land_mask"])
    m = np.load(eco / "diversity_maps_day_012.3.npz")
    assert sorted(m.files) == ["alpha_map", "bc_local"] and m["alpha_map"].dtype == np.float64
    assert np.array_equal(m["alpha_map"], z["alpha_map"], equal_nan=True) and np.array_equal(m["bc_local"], z["bc_local"], equal_nan=True)
    write_diversity_files(str(tmp_path / "out"), 0.0, z["alpha_map"], z["bc_local"], z["L_s"], summary, z["land_mask"])
    assert os.path.exists(eco / "diversity_summary_day_000.0.txt")


def test_diag_line():
    from qingdai_amd.ecology import diversity_line
    line = diversity_line(0.05, {"alpha_mean": 16.58853543, "gamma_eff": 19.91508564, "beta_whittaker": 1.20053309})
    assert line == "[Diversity] day 0.05: alpha_mean=16.5885 gamma_eff=19.9151 beta_whittaker=1.2005"


def test_env_parsing():
    from qingdai_amd.ecology import diversity_env
    assert diversity_env({}) == (False, 10.0)
    assert diversity_env({"QD_ECO_DIVERSITY_ENABLE": "1"}) == (True, 10.0)
    assert diversity_env({"QD_ECO_DIVERSITY_ENABLE": "0", "QD_ECO_DIVERSITY_EVERY_DAYS": "2.5"}) == (False, 2.5)
    assert diversity_env({"QD_ECO_DIVERSITY_ENABLE": "1", "QD_ECO_DIVERSITY_EVERY_DAYS": "often"}) == (True, 10.0)
    assert diversity_env({"QD_ECO_DIVERSITY_ENABLE": "1", "QD_ECO_DIVERSITY_EVERY_DAYS": "-3"}) == (True, -3.0)
    assert diversity_env({"QD_ECO_DIVERSITY_ENABLE": "yes"}) == (False, 10.0)


def test_abi_names():
    # that the header declares the symbols and the ids are the compiler's: tests/test_abi_cpu.py
    assert {k: v for k, v in _lib.F.items() if k.startswith("ECO_DIV_")} == {"ECO_DIV_LS": 110, "ECO_DIV_ALPHA": 111, "ECO_DIV_BC": 112,
                                                                            "ECO_DIV_SUMMARY": 113}
    assert _lib.FIELDS[-1] == "KD490" and _lib.F["LAND_MASK"] == 100 and _lib.F["ICE_MASK"] == 101      # nothing renumbered
    from qingdai_amd.device import Device
    from qingdai_amd.ecology import PopulationCanopy
    assert callable(Device.eco_diversity) and callable(Device.eco_diversity_get) and callable(PopulationCanopy.diversity)
