"""CPU: the ecology autosave's host side and its NumPy restatement, no GPU and no libqingdai_hip.so.  The restatement against the
reference's goldens (bitwise, both load rules' spellings); around a stub device: the `.nc` layout through ncio.read_nc_full, the f32
cast of LAI, tmp + replace, the backups and QD_ECO_AUTOSAVE_KEEP, the path rules of QD_ECO_AUTOSAVE_PATH, genes.json against the
reference's document, load_genes_json's three branches, the mismatch branches with the reference's lines, the refusal under
QD_ECO_INDIV_DAILY, the silence of QD_ECO_PERSIST unset, the new ABI name."""
import contextlib
import ctypes
import glob
import io
import json
import os
import re

import numpy as np
import pytest

import eco_state_ref as ref
from qingdai_amd import ncio
from qingdai_amd import SphericalGrid

HERE = os.path.dirname(os.path.abspath(__file__))
GOLD = os.path.join(HERE, "golden")
GOLDENS = sorted(p for p in glob.glob(os.path.join(GOLD, "eco_state_*_f*_*x*.npz")) if "mismatch" not in p)
CASES = ["k8_f32", "k8_f64", "mixed_f32", "mixed_f64", "noland_f32", "ns20_f32", "ns20_f64", "wide_f32", "wide_f64"]
CLOCK = (7.5, 12.0, 90.0)


def _case(p):
    return "_".join(os.path.basename(p).split("_")[2:4])


def _env_of(z):
    return {str(k): str(v) for k, v in zip(z["env_keys"], z["env_vals"])}


def _clean_env(monkeypatch, env=None):
    for k in [k for k in os.environ if k.startswith(("QD_ECO_", "QD_AUTOSAVE", "QD_DATA_DIR"))]:
        monkeypatch.delenv(k)
    for k, v in (env or {}).items():
        monkeypatch.setenv(k, v)


# ------------------------------------------------------------------ the restatement against the reference
def test_every_case_has_a_golden_cpu():
    assert [_case(p) for p in GOLDENS] == CASES
    assert os.path.exists(os.path.join(GOLD, "eco_state_mismatch_f32_19x36.npz")) and os.path.exists(os.path.join(GOLD, "genes_eco_state_mixed.json"))


@pytest.mark.parametrize("path", GOLDENS, ids=_case)
def test_restatement_matches_reference_bitwise_cpu(path):
    z = np.load(path)
    K, lai_max = int(z["K"]), float(z["lai_max"])
    got = ref.load_rule(z["file_LAI"], z["file_species_weights"], K, lai_max)
    want = [z["load_LAI"], z["load_species_weights"], z["load_LAI_layers_SK"], z["load_total_LAI"]]
    for a, b, what in zip(got, want, ("LAI", "weights", "stack", "total")):
        assert a.dtype == b.dtype and np.array_equal(a, b, equal_nan=True), what
    if z["file_LAI"].dtype == np.float32:
        for a, b, what in zip(ref.load_rule_f32(z["file_LAI"], z["file_species_weights"], K, lai_max), want, ("LAI", "weights", "stack", "total")):
            assert np.array_equal(a, b, equal_nan=True), what
        f64 = ref.load_rule(z["file_LAI"].astype(np.float64), z["file_species_weights"].astype(np.float64), K, lai_max)[2]
        assert not np.array_equal(f64, z["load_LAI_layers_SK"], equal_nan=True)          # f64 arithmetic is NOT what the reference does
    assert z["load_LAI_layers_SK"].dtype == np.float64
    assert np.array_equal(np.clip(z["file_R_species_nb"].astype(float), 0, 1), z["load_R_leaf"])


def test_goldens_cover_what_they_claim_cpu():
    z = {c: np.load(p) for c, p in zip(CASES, GOLDENS)}
    assert z["mixed_f32"]["load_LAI_layers_SK"].shape == (3, 2, 19, 36) and z["ns20_f64"]["load_LAI_layers_SK"].shape == (20, 1, 19, 36)
    assert z["k8_f32"]["load_LAI_layers_SK"].shape == (1, 8, 19, 36) and z["wide_f32"]["load_LAI_layers_SK"].shape == (3, 2, 5, 130)
    assert sorted(set(map(str, z["mixed_f32"]["modes"]))) == ["diffusion", "seed"] and not z["noland_f32"]["land_mask"].any()
    for c in ("mixed_f32", "mixed_f64", "ns20_f32", "wide_f64"):
        L, land = z[c]["file_LAI"], z[c]["land_mask"] == 1
        assert (L < 0).any() and (L > 5.0).any() and np.isnan(L).any() and np.isposinf(L).any() and (L == 0).any()
        assert land[0].any() and land[-1].any()
        meta = json.loads(str(z[c]["meta"]))
        assert meta["ocean_cells_nonzero"] > 10                  # no land mask in the load: ocean cells keep their values
        assert meta["LAI_vs_total_LAI"] > 0                      # pop.LAI and the plane sum differ after a load
        assert (z[c]["load_species_weights"] == 0).any()         # a species clipped to weight 0
    sub = z["mixed_f32"]["file_LAI"][0, 3]
    assert sub.dtype == np.float32 and 0 < sub < np.finfo(np.float32).tiny and z["mixed_f32"]["load_LAI_layers_SK"][0, 0, 0, 3] > 0


# ------------------------------------------------------------------ a stub device
class StubLib:
    def __init__(self):
        self.calls, self.clock = [], list(CLOCK)

    def __getattr__(self, name):
        if not name.startswith("qd_"):
            raise AttributeError(name)

        def fn(h, *args):
            self.calls.append((name, args))
            return 0
        return fn

    def qd_eco_get_state(self, h, out):
        for i, v in enumerate(self.clock + [2.0, 1.0]):
            out[i] = v
        return 0

    def qd_eco_set_state(self, h, clock):
        self.clock = [clock[0], clock[1], clock[2]]
        self.calls.append(("qd_eco_set_state", tuple(self.clock)))
        return 0


class StubDev:
    """What the ecology classes ask of a Device, on the host: planes in a dict, the restore through the restatement."""
    def __init__(self, grid):
        self.grid, self.shape, self.lib, self.h, self._host, self.planes = grid, (grid.n_lat, grid.n_lon), StubLib(), ctypes.c_void_p(1), {}, {}
        self.restores, self.stack, self.fired = [], None, 0

    def _chk(self, rc, what):
        assert rc == 0, what

    def flush(self):
        pass

    def get(self, name):
        return self.planes.setdefault(name, np.zeros(self.shape))

    def upload_now(self, name, arr):
        self.planes[name] = np.array(np.broadcast_to(np.asarray(arr, dtype=np.float64), self.shape))

    def eco_state_restore(self, lai, weights, n_layers, lai_max):
        self.restores.append((np.asarray(lai).dtype, np.array(weights), int(n_layers), float(lai_max)))
        q = np.clip(lai, 0.0, lai_max) / float(n_layers)         # the weights arrive as the reference leaves them: no second division
        self.planes["ECO_LAI"] = np.sum([(float(w) * q).astype(np.float64) for w in weights for _ in range(n_layers)], axis=0)

    def eco_daily_firings(self):
        return self.fired

    def indiv_daily_firings(self):
        return 0


def _adapter(monkeypatch, env, shape=(19, 36), land=None):
    from qingdai_amd.ecology import EcologyAdapter
    _clean_env(monkeypatch, env)
    grid = SphericalGrid(*shape)
    dev = StubDev(grid)
    land = np.ones(shape, dtype=np.uint8) if land is None else land
    return EcologyAdapter(grid, land, dev=dev), dev


MIXED = os.path.join(GOLD, "eco_state_mixed_f32_19x36.npz")


def _mixed(monkeypatch, extra=None):
    z = np.load(MIXED)
    eco, dev = _adapter(monkeypatch, {**_env_of(z), **(extra or {})}, land=z["land_mask"])
    return z, eco, dev


def _write_nc(path, z, prefix="file_"):
    """A NetCDF file of the reference's layout from a golden's file arrays."""
    S, NB = z[prefix + "R_species_nb"].shape
    ncio.write_nc(path, {"lat": z[prefix + "LAI"].shape[0], "lon": z[prefix + "LAI"].shape[1], "species": S, "band": NB},
                  {"LAI": ("f4", ("lat", "lon"), z[prefix + "LAI"]), "species_weights": ("f4", ("species",), z[prefix + "species_weights"]),
                   "bands_lambda_centers": ("f4", ("band",), z[prefix + "bands_lambda_centers"]),
                   "R_species_nb": ("f4", ("species", "band"), z[prefix + "R_species_nb"])}, dict(ref.NC_ATTRS))


# ------------------------------------------------------------------ save
@pytest.mark.parametrize("level", [1, 2])
def test_nc_layout_cpu(tmp_path, monkeypatch, level):
    z, eco, dev = _mixed(monkeypatch, {"QD_ECO_PERSIST": str(level), "QD_ECO_DIAG": "1"})
    plane = np.random.default_rng(1).uniform(0, 3, dev.shape) * (1 + 1e-9)
    dev.planes["ECO_LAI"] = plane
    path = str(tmp_path / "data" / "ecology.nc")
    buf = io.StringIO()
    with contextlib.redirect_stdout(buf):
        assert eco.save_autosave(path, day_value=1.5) is True
    dims, v, attrs = ncio.read_nc_full(path)
    want_dims, want = ref.nc_layout(3, eco.bands.nbands, dev.shape, level=level, K=2)
    assert dims == want_dims and {k: (c, d) for k, (c, d, _) in v.items()} == want
    assert attrs["title"] == ref.NC_ATTRS["title"] and attrs["source"] == ref.NC_ATTRS["source"] and int(attrs["schema_version"]) == 1
    assert np.array_equal(v["LAI"][2], plane.astype(np.float32)) and not np.array_equal(v["LAI"][2].astype(float), plane)      # the f32 cast
    assert np.array_equal(v["species_weights"][2], eco.pop.species_weights.astype(np.float32)) and float(v["day_value"][2]) == 1.5
    assert np.array_equal(v["R_species_nb"][2], eco.pop._species_R_leaf.astype(np.float32))
    assert np.array_equal(v["lat"][2], eco.grid.lat.astype(np.float32)) and np.array_equal(v["w_b"][2], eco.w_b.astype(np.float32))
    if level == 2:
        assert np.array_equal(v["qd_LAI_layers_SK"][2], eco.pop.LAI_layers_SK) and tuple(v["qd_eco_clock"][2]) == CLOCK
        assert np.array_equal(v["qd_species_weights"][2], eco.pop.species_weights) and float(v["qd_accum_day"][2]) == 0.0
    # tmp + replace: nothing but the file, one backup and genes.json; the reference's line
    names = sorted(os.listdir(tmp_path / "data"))
    assert len(names) == 3 and names[0] == "ecology.nc" and re.fullmatch(r"ecology_\d{8}T\d{6}Z\.nc", names[1]) and names[2] == "genes.json"
    assert not [n for n in os.listdir(tmp_path / "data") if ".tmp" in n]
    line = [l for l in buf.getvalue().splitlines() if l.startswith("[Ecology] Autosave written: ")]
    assert line == [f"[Ecology] Autosave written: {path}; backup={os.path.join(os.path.dirname(path), names[1])}"]


def test_npz_branch_cpu(tmp_path, monkeypatch):
    z, eco, dev = _mixed(monkeypatch)
    dev.planes["ECO_LAI"] = np.full(dev.shape, 0.25)
    path = str(tmp_path / "eco.npz")
    assert eco.save_autosave(path, day_value=2.0)
    with np.load(path) as d:
        assert sorted(d.files) == sorted(["schema_version", "LAI", "species_weights", "bands_lambda_centers", "bands_delta_lambda", "w_b",
                                          "R_species_nb", "day_value"])
        assert d["LAI"].dtype == np.float64 and int(d["schema_version"]) == 1 and float(d["day_value"]) == 2.0
    assert not [n for n in os.listdir(tmp_path) if ".tmp" in n]


@pytest.mark.parametrize("keep", [0, 1, 4])
def test_backups_and_keep_cpu(tmp_path, monkeypatch, keep):
    import qingdai_amd.ecology as E
    z, eco, dev = _mixed(monkeypatch, {"QD_ECO_AUTOSAVE_KEEP": str(keep), "QD_ECO_DIAG": "0"})
    stamps = iter(f"20300101T0000{n:02d}Z" for n in range(60))
    monkeypatch.setattr(E.time, "strftime", lambda fmt, t=None: next(stamps))
    for _ in range(6):
        assert eco.save_autosave(str(tmp_path / "ecology.nc"))
    backups = sorted(n for n in os.listdir(tmp_path) if re.fullmatch(r"ecology_.*\.nc", n))
    assert len(backups) == keep and "ecology.nc" in os.listdir(tmp_path) and "genes.json" in os.listdir(tmp_path)
    if keep == 0:
        return
    os.makedirs(tmp_path / "other")
    assert eco.save_autosave(str(tmp_path / "other" / "state.npz"))      # another name and extension: its own backups, the first ones stay
    assert sorted(n for n in os.listdir(tmp_path) if re.fullmatch(r"ecology_.*\.nc", n)) == backups


# ------------------------------------------------------------------ the driver's path rules
def _sim(eco, indiv=None):
    from qingdai_amd.driver import Simulation
    sim = object.__new__(Simulation)
    sim.eco, sim.indiv = eco, indiv
    return sim


def test_autosave_path_rules_cpu(tmp_path, monkeypatch, capsys):
    z, eco, dev = _mixed(monkeypatch, {"QD_ECO_DIAG": "1"})
    sim, data = _sim(eco), str(tmp_path / "data")
    custom = str(tmp_path / "elsewhere" / "Veg.NC")
    assert sim.save_ecology(data, 1.0, {"QD_ECO_PERSIST": "1", "QD_ECO_AUTOSAVE_PATH": custom}) == custom           # `.nc`, any case
    assert os.path.exists(custom) and os.path.exists(os.path.join(data, "genes.json")) and not os.path.exists(os.path.join(data, "ecology.nc"))
    npz = str(tmp_path / "elsewhere" / "veg.npz")
    assert sim.save_ecology(data, 1.0, {"QD_ECO_PERSIST": "1", "QD_ECO_AUTOSAVE_PATH": npz}) == os.path.join(data, "ecology.nc")
    assert not os.path.exists(npz) and os.path.exists(os.path.join(data, "ecology.nc"))                             # not `.nc`: ignored on save
    # on load any extension is taken
    np.savez(npz, LAI=z["file_LAI"].astype(np.float64), species_weights=z["file_species_weights"].astype(np.float64),
             bands_lambda_centers=z["file_bands_lambda_centers"], R_species_nb=z["file_R_species_nb"])
    capsys.readouterr()
    assert sim.load_ecology(data, {"QD_ECO_PERSIST": "1", "QD_ECO_AUTOSAVE_PATH": npz, "QD_ECO_GENES_JSON_PATH": str(tmp_path / "none.json")})
    out = capsys.readouterr().out.splitlines()
    assert out[-1] == f"[Ecology] autosave load OK from '{npz}'" and out[-2].startswith("[Ecology] Autosave+ loaded: LAI(min/mean/max)=")
    assert dev.restores[-1][0] == np.float64
    assert not sim.load_ecology(data, {"QD_ECO_PERSIST": "1", "QD_AUTOSAVE_LOAD": "0"})
    # a failing save prints the reference's line and goes on
    monkeypatch.setattr(type(eco), "save_autosave", lambda *a, **k: (_ for _ in ()).throw(OSError("disk full")))
    assert sim.save_ecology(data, 1.0, {"QD_ECO_PERSIST": "1"}) is None
    assert "[Autosave] Ecology extended save failed: disk full" in capsys.readouterr().out


def test_persist_unset_calls_nothing_cpu(tmp_path, monkeypatch, capsys):
    from qingdai_amd.driver import eco_persist_level
    z, eco, dev = _mixed(monkeypatch)

    def boom(*a, **k):
        raise AssertionError("the persistence code ran without QD_ECO_PERSIST")
    for name in ("save_autosave", "load_autosave", "save_genes_json", "load_genes_json"):
        monkeypatch.setattr(type(eco), name, boom)
    sim, data = _sim(eco), str(tmp_path / "data")
    os.makedirs(data)
    open(os.path.join(data, "ecology.nc"), "w").close()
    open(os.path.join(data, "genes.json"), "w").close()
    for env in ({}, {"QD_ECO_PERSIST": "0"}, {"QD_ECO_PERSIST": "junk"}):
        assert eco_persist_level(env) == 0 and sim.save_ecology(data, 1.0, env) is None and sim.load_ecology(data, env) is False
    assert (eco_persist_level({"QD_ECO_PERSIST": "1"}), eco_persist_level({"QD_ECO_PERSIST": "2"}), eco_persist_level({"QD_ECO_PERSIST": "7"})) == (1, 2, 2)
    assert capsys.readouterr().out == "" and dev.restores == []


# ------------------------------------------------------------------ genes.json
def test_genes_json_equals_the_reference_document_cpu(tmp_path, monkeypatch):
    z = np.load(os.path.join(GOLD, "eco_state_mixed_f64_19x36.npz"))
    eco, dev = _adapter(monkeypatch, _env_of(z), land=z["land_mask"])
    from qingdai_amd.ecology import PopulationDaily
    eco.pop.species_weights = z["load_species_weights"]
    path = str(tmp_path / "genes.json")
    assert eco.save_genes_json(path, day_value=9.0)
    got, want = json.load(open(path)), json.load(open(os.path.join(GOLD, "genes_eco_state_mixed.json")))
    ref.check_genes_document(got, 3, eco.bands.nbands)
    ref.check_genes_document(want, 3, eco.bands.nbands)
    assert got["day"] == 9.0 and want["day"] == 1.25
    got.pop("day"), want.pop("day")
    assert got == want and list(got) == list(want)
    assert [g["identity"] for g in got["genes"]] == ["tree", "grass", "shrub"]          # by mode, and the named one
    assert open(path).read().startswith('{\n  "schema_version": 3,')


def test_load_genes_json_branches_cpu(tmp_path, monkeypatch, capsys):
    z, eco, dev = _mixed(monkeypatch, {"QD_ECO_DIAG": "1"})
    doc = json.load(open(os.path.join(GOLD, "genes_eco_state_mixed.json")))
    lam = eco.bands.lambda_centers
    R0 = eco.pop._species_R_leaf.copy()
    # sigma_nm wins over variance_nm2
    for rec in doc["genes"]:
        for pk in rec["peaks"]:
            pk["variance_nm2"] = 1.0
    doc["genes"] = doc["genes"][:2]
    p = str(tmp_path / "g.json")
    json.dump(doc, open(p, "w"))
    assert eco.load_genes_json(p) is True and len(eco.genes_list) == 2
    want = np.stack([ref.gene_reflectance(lam, ref.peaks_of(r)) for r in doc["genes"]])
    assert np.array_equal(eco.pop._species_R_leaf, want) and [g.provenance for g in eco.genes_list] == ["autosave:genes_json"] * 2
    assert "[Ecology] Genes autosave loaded: Ns=2 (band nb=%d)" % eco.bands.nbands in capsys.readouterr().out
    # variance_nm2 only
    for rec in doc["genes"]:
        for pk in rec["peaks"]:
            pk["variance_nm2"] = 4.0 * pk.pop("sigma_nm") ** 2
    json.dump(doc, open(p, "w"))
    assert eco.load_genes_json(p) is True
    wide = np.stack([ref.gene_reflectance(lam, [(c, 2.0 * s, h) for c, s, h in pk]) for pk in
                     [[(q["center_nm"], np.sqrt(q["variance_nm2"]) / 2.0, q["height"]) for q in r["peaks"]] for r in doc["genes"]]])
    assert np.array_equal(eco.pop._species_R_leaf, wide) and not np.array_equal(wide, want)
    s = sum((eco.genes_list[1].alloc_root, eco.genes_list[1].alloc_stem, eco.genes_list[1].alloc_leaf))
    assert abs(s - 1.0) < 1e-15
    # no genes: False, everything kept
    kept, table = eco.pop._species_R_leaf.copy(), eco.genes_list
    json.dump({"schema_version": 3, "genes": []}, open(p, "w"))
    assert eco.load_genes_json(p) is False and np.array_equal(eco.pop._species_R_leaf, kept) and eco.genes_list is table
    assert "[Ecology] Genes autosave contains no genes; keeping current." in capsys.readouterr().out
    assert eco.load_genes_json(str(tmp_path / "missing.json")) is False
    assert R0.shape == (3, eco.bands.nbands)


# ------------------------------------------------------------------ load
def test_load_nc_is_float32_and_npz_float64_cpu(tmp_path, monkeypatch):
    z, eco, dev = _mixed(monkeypatch)
    path = str(tmp_path / "ecology.nc")
    _write_nc(path, z)
    assert eco.load_autosave(path) is True
    dt, w, K, lai_max = dev.restores[-1]
    assert dt == np.float32 and K == 2 and lai_max == 5.0 and np.array_equal(w, z["load_species_weights"].astype(np.float64))
    assert eco.pop.species_weights.dtype == np.float32 and np.array_equal(eco.pop.species_weights, z["load_species_weights"])
    assert np.array_equal(eco.pop.LAI_layers_SK, z["load_LAI_layers_SK"], equal_nan=True)         # the host form of the rule, no daily lane
    assert np.array_equal(eco.pop.total_LAI(), z["load_total_LAI"], equal_nan=True) and np.array_equal(eco.pop._species_R_leaf, z["load_R_leaf"])
    z64 = np.load(os.path.join(GOLD, "eco_state_mixed_f64_19x36.npz"))
    eco, dev = _adapter(monkeypatch, _env_of(z64), land=z64["land_mask"])
    npz = str(tmp_path / "ecology.npz")
    np.savez(npz, **{k[5:]: z64[k] for k in z64.files if k.startswith("file_")})
    assert eco.load_autosave(npz) is True and dev.restores[-1][0] == np.float64
    assert np.array_equal(eco.pop.LAI_layers_SK, z64["load_LAI_layers_SK"], equal_nan=True)
    assert np.array_equal(eco.pop.species_weights, z64["load_species_weights"])


def test_mismatch_branches_and_lines_cpu(tmp_path, monkeypatch, capsys):
    m = np.load(os.path.join(GOLD, "eco_state_mismatch_f32_19x36.npz"))
    env = {**_env_of(m), "QD_ECO_DIAG": "1"}

    def load(tag, **kw):
        eco, dev = _adapter(monkeypatch, env, land=m["land_mask"])
        path = str(tmp_path / (tag + ".npz"))
        np.savez(path, **{k[len(tag) + 6:]: m[k] for k in m.files if k.startswith(tag + "_file_")})
        before = (eco.pop.LAI_layers_SK.copy(), eco.pop.species_weights.copy(), eco.pop._species_R_leaf.copy())
        capsys.readouterr()
        ok = eco.load_autosave(path, **kw)
        lines = capsys.readouterr().out.splitlines()
        assert ok == bool(m[tag + "_ok"]) and lines == [str(l) for l in m[tag + "_lines"]], (tag, lines)
        return eco, dev, before
    eco, dev, _ = load("species4")                              # another species count: the population follows the file
    assert eco.pop.Ns == 4 and np.array_equal(eco.pop.LAI_layers_SK, m["species4_load_LAI_layers_SK"], equal_nan=True)
    assert np.array_equal(eco.pop.species_weights, m["species4_load_species_weights"]) and np.array_equal(eco.pop._species_R_leaf, m["species4_load_R_leaf"])
    eco, dev, before = load("bands")                            # another band count: base fields only, and the note
    assert np.array_equal(eco.pop._species_R_leaf, before[2]) and np.array_equal(eco.pop.LAI_layers_SK, m["bands_load_LAI_layers_SK"], equal_nan=True)
    load("bands_ignore", on_mismatch="ignore")                  # ... without the note
    eco, dev, before = load("malformed")                        # LAI not 2-D: False, state untouched
    assert dev.restores == [] and all(np.array_equal(a, b) for a, b in zip(before, (eco.pop.LAI_layers_SK, eco.pop.species_weights, eco.pop._species_R_leaf)))


def test_species_mismatch_reconfigures_the_lane_and_keeps_age_and_bank_cpu(tmp_path, monkeypatch):
    from qingdai_amd.ecology import PopulationDaily
    m = np.load(os.path.join(GOLD, "eco_state_mismatch_f32_19x36.npz"))
    eco, dev = _adapter(monkeypatch, {**_env_of(m), "QD_ECO_DIAG": "0", "QD_ECO_RAND_SEED": "5"}, land=m["land_mask"])
    dev.eco_daily_configure = lambda p, mode, w: (dev.lib.calls.append(("configure", p.n_species, list(mode), np.array(w))),
                                                  dev.planes.update(ECO_AGE=np.zeros(dev.shape), ECO_SEEDBANK=np.zeros(dev.shape)))
    dev.eco_daily_set_layers = lambda a: setattr(dev, "stack", np.array(a))
    dev.eco_daily_get_layers = lambda S, K: dev.stack.reshape((S, K) + dev.shape)
    daily = PopulationDaily(eco.pop, day_seconds=100.0)
    age, bank = np.random.default_rng(0).uniform(0, 9, (2,) + dev.shape)
    dev.planes.update(ECO_AGE=age.copy(), ECO_SEEDBANK=bank.copy())
    path = str(tmp_path / "s4.npz")
    np.savez(path, **{k[14:]: m[k] for k in m.files if k.startswith("species4_file_")})
    assert eco.load_autosave(path) is True
    conf = [c for c in dev.lib.calls if c[0] == "configure"]
    assert [c[1] for c in conf] == [3, 4] and len(daily.species_modes) == 4 and daily.params.n_species == 4
    assert np.array_equal(dev.planes["ECO_AGE"], age) and np.array_equal(dev.planes["ECO_SEEDBANK"], bank)        # put back behind the configure
    assert dev.restores[-1][1].size == 4 and dev.stack.shape[0] == 6          # the stack is the kernel's to fill, not uploaded again
    # the same species count: the lane still gets the file's weights (the reference reads pop.species_weights in every step_daily)
    w4 = np.array([0.0, 0.2, 0.7, 0.1])
    np.savez(path, LAI=m["species4_file_LAI"].astype(np.float64), species_weights=w4 * 3.0)
    assert eco.load_autosave(path) is True
    conf = [c for c in dev.lib.calls if c[0] == "configure"]
    assert len(conf) == 3 and conf[-1][1] == 4 and np.allclose(conf[-1][3], w4, rtol=0, atol=1e-12) and not np.allclose(conf[-2][3], w4, atol=1e-3)
    assert np.array_equal(dev.planes["ECO_AGE"], age) and np.array_equal(dev.planes["ECO_SEEDBANK"], bank)


def test_indiv_daily_refuses_another_species_count_cpu(tmp_path, monkeypatch, capsys):
    m = np.load(os.path.join(GOLD, "eco_state_mismatch_f32_19x36.npz"))
    eco, dev = _adapter(monkeypatch, {**_env_of(m), "QD_ECO_DIAG": "1"}, land=m["land_mask"])
    eco.pop.indiv_daily = object()                              # the individuals' daily step is configured
    eco.pop._weights_at = 0
    data = tmp_path / "data"
    os.makedirs(data)
    path = str(data / "ecology.npz")
    np.savez(path, **{k[14:]: m[k] for k in m.files if k.startswith("species4_file_")})
    before = eco.pop.LAI_layers_SK.copy()
    with pytest.raises(ValueError, match="the file holds 4 species, the run 3"):
        eco.load_autosave(path)
    capsys.readouterr()
    assert _sim(eco).load_ecology(str(data), {"QD_ECO_PERSIST": "1", "QD_ECO_AUTOSAVE_PATH": path}) is False      # the driver goes on fresh
    out = capsys.readouterr().out.splitlines()
    assert len(out) == 1 and out[0].startswith("[Ecology] autosave load skipped: the file holds 4 species, the run 3")
    assert dev.restores == [] and np.array_equal(eco.pop.LAI_layers_SK, before) and eco.pop.Ns == 3


def test_exact_variables_round_trip_and_misfit_cpu(tmp_path, monkeypatch, capsys):
    z, eco, dev = _mixed(monkeypatch, {"QD_ECO_DIAG": "1"})
    rng = np.random.default_rng(3)
    stack = rng.uniform(0, 1, (3, 2) + dev.shape)
    eco.pop.LAI_layers_SK = stack
    for k in ("ECO_AGE", "ECO_SEEDBANK", "ECO_EDAY"):
        dev.planes[k] = rng.uniform(0, 5, dev.shape)
    dev.planes["ECO_LAI"] = np.nextafter(stack.sum(axis=(0, 1)), np.inf)      # (summed in another order by the individuals' step)
    saved = {k: v.copy() for k, v in dev.planes.items()}
    path = str(tmp_path / "ecology.nc")
    assert eco.save_autosave(path, 3.0, extended=True)
    _, v, _ = ncio.read_nc_full(path)
    assert ref.fits({k: a for k, (_, _, a) in v.items()}, 3, 2, dev.shape, 0)
    eco2, dev2 = _adapter(monkeypatch, {**_env_of(z), "QD_ECO_DIAG": "1"}, land=z["land_mask"])
    capsys.readouterr()
    assert eco2.load_autosave(path) is True
    assert "[Ecology] Autosave+: exact resume from the qd_* extension variables." in capsys.readouterr().out
    assert dev2.restores == [] and np.array_equal(eco2.pop.LAI_layers_SK, stack) and tuple(dev2.lib.clock) == CLOCK
    for k in ("ECO_LAI", "ECO_AGE", "ECO_SEEDBANK", "ECO_EDAY"):
        assert np.array_equal(dev2.planes[k], saved[k]), k
    # extended=False (QD_ECO_PERSIST=1 in the driver) and a run with another K ignore them: the reference rule, and one line for the misfit
    eco3, dev3 = _adapter(monkeypatch, {**_env_of(z), "QD_ECO_DIAG": "1"}, land=z["land_mask"])
    assert eco3.load_autosave(path, extended=False) is True and len(dev3.restores) == 1
    eco4, dev4 = _adapter(monkeypatch, {**_env_of(z), "QD_ECO_DIAG": "1", "QD_ECO_COHORT_K": "3"}, land=z["land_mask"])
    capsys.readouterr()
    assert eco4.load_autosave(path) is True and len(dev4.restores) == 1 and dev4.restores[0][2] == 3
    assert capsys.readouterr().out.count("extension variables do not fit this run") == 1


def test_abi_name_cpu():
    h = open(os.path.join(HERE, "..", "include", "qingdai_hip.h")).read()
    assert re.search(r"\bint qd_eco_state_restore\(qd_handle h, const void\* lai, int lai_is_f32,", h)
    assert "adapter.py:742-757" in h
    mk = open(os.path.join(HERE, "..", "qingdai_amd", "csrc", "Makefile")).read()
    assert "qd_eco_state.hip" in mk and "ftz" not in mk.lower() and "denormals" not in mk.lower() and "fast-math" not in mk.replace("-fno-fast-math", "")
