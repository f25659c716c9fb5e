"""CPU: the parameter sweep's table (tests/param_sweep_cases.py) is complete, every row is live in the oracle, the oracle agrees
with the reference's digest of every row that has one, and the environment layer maps every QD_* name onto its field.

Liveness is a condition, not a measurement: a row whose perturbed oracle run does not move a compared field by 1000 x the bound
that field is held to on the device (1e-6 at least) would pass on the device whatever the kernel does with the parameter."""
import math

import numpy as np
import pytest

import qd_oracle as qo
import param_sweep_cases as C
from qingdai_amd import params as qp
from util import load_golden

ALL = [n for n, _, _ in qp._DOUBLES + qp._INTS]
_BASE = {}


def oracle_baseline(scenario, comp):
    key = (scenario, tuple(sorted(comp.items())))
    if key not in _BASE:
        with np.errstate(all="ignore"):
            _BASE[key] = C.run_oracle(scenario, comp)
    return _BASE[key]


def test_every_parameter_is_in_exactly_one_list():
    rows = {r["param"] for r in C.ROWS}
    for n in ALL:
        where = [n in rows, n in C.DEAD, n in C.EXEMPT]
        assert sum(where) == 1, (n, where)
    assert rows | set(C.DEAD) | set(C.EXEMPT) == set(ALL)                  # and nothing in them that is no parameter
    assert set(vars(qo.defaults())) - {"q_init_rh"} == set(ALL) - {"has_csmap"}
    assert len({r["id"] for r in C.ROWS}) == len(C.ROWS)
    for n, (scn, value, where) in C.DEAD.items():                          # a DEAD entry cites the reference's file:line
        assert scn in C.SCENARIOS and "pygcm/" in where and ".py:" in where, n
    for n, why in C.EXEMPT.items():
        assert why.strip(), n
    for v in ("combo", "hyper4", "shapiro", "spectral"):                   # every filter_type: combo is the baseline
        assert v == "combo" or any(r["param"] == "filter_type" and r["value"] == v for r in C.ROWS), v
    for r in C.ROWS:
        assert r["fixture"] or r["pin"], r["id"]                           # a reference digest, or the name of the existing pin
        assert set(r["comp"]) <= set(ALL) and r["param"] not in r["comp"], r["id"]
        if r["tol"]:                                                       # a loosened bound is 100 x the oracle's own noise
            assert r["noise"], r["id"]
            for k, t in r["tol"].items():
                assert t <= 100.0 * r["noise"][k] * (1 + 1e-12), (r["id"], k)


LIVE_ROWS = C.ROWS + C.PIN_ROWS


@pytest.mark.parametrize("row", LIVE_ROWS, ids=[f"{r['scenario']}-{r['id']}" for r in LIVE_ROWS])
def test_row_is_live_in_the_oracle(row):
    base = oracle_baseline(row["scenario"], row["comp"])
    with np.errstate(all="ignore"):
        got = C.run_oracle(row["scenario"], {**row["comp"], row["param"]: row["value"]})
    tol = C.row_tol(row)
    moved = {k: C.relerr(got[k], base[k]) for k in tol}
    assert any(moved[k] >= C.live_threshold(tol[k]) for k in tol), moved


@pytest.mark.parametrize("name", sorted(C.DEAD))
def test_dead_parameter_changes_nothing_in_the_oracle(name):
    scn, value, _ = C.DEAD[name]
    base = oracle_baseline(scn, {})
    with np.errstate(all="ignore"):
        got = C.run_oracle(scn, {name: value})
    for k in C.SCENARIOS[scn]["fields"]:
        assert np.array_equal(got[k], base[k]), k


FIXTURE_ROWS = [r for r in C.ROWS + C.PIN_ROWS if r["fixture"]]


@pytest.mark.parametrize("row", FIXTURE_ROWS, ids=[f"{r['scenario']}-{r['id']}" for r in FIXTURE_ROWS])
def test_oracle_matches_the_reference_digest(row):
    """The bound of tests/test_oracle_golden.py for the family (time_step 1e-11, ocean 1e-14, orographic precipitation bit for
    bit); the sums scaled as in test_driver_known_answers: |delta sum| <= tol * N * max|field|."""
    scn = row["scenario"]
    meta, d = load_golden(C.fixture_name(scn))
    ri = meta["rows"].index(row["id"])
    tol = C.SCENARIOS[scn]["ref_tol"]
    with np.errstate(all="ignore"):
        got = C.run_oracle(scn, {**row["comp"], row["param"]: row["value"]})
    cells = d["cells"]
    assert {0, C.SHAPE[0] - 1} <= set((cells // C.SHAPE[1]).tolist()) and {0, C.SHAPE[1] - 1} <= set((cells % C.SHAPE[1]).tolist())
    for fi, k in enumerate(meta["fields"]):
        scale = float(d["maxs"][ri, fi])
        vals, s, mx = C.digest(got[k], cells)
        assert np.max(np.abs(vals - d["vals"][ri, fi])) <= tol * max(scale, 1e-300), (k, "cells")
        assert abs(s - float(d["sums"][ri, fi])) <= tol * got[k].size * max(scale, 1e-300), (k, "sum")
        assert abs(mx - scale) <= tol * max(scale, 1e-300), (k, "max")


def test_fixtures_hold_exactly_the_table_rows():
    for scn, sc in C.SCENARIOS.items():
        rows = C.fixture_rows(scn)
        if sc["ref_tol"] is None:
            assert not rows
            continue
        meta, d = load_golden(C.fixture_name(scn))
        assert meta["rows"] == [r["id"] for r in rows] and meta["fields"] == list(sc["fields"])
        assert np.array_equal(d["cells"], C.sample_cells()) and d["cells"].size == C.N_SAMPLE


def _same(a, b):
    return all((x == y) or (isinstance(x, float) and isinstance(y, float) and math.isnan(x) and math.isnan(y))
               for x, y in ((getattr(a, n), getattr(b, n)) for n in ALL))


def _clean_env(monkeypatch):
    import os
    for k in [k for k in os.environ if k.startswith("QD_")]:
        monkeypatch.delenv(k)


ENV_CASES = [(r["param"], r["value"]) for r in C.ROWS if C.env_name(r["param"])] + \
            [(n, v) for n, (_, v, _) in C.DEAD.items() if C.env_name(n)]


@pytest.mark.parametrize("param,value", ENV_CASES, ids=[f"{p}={v}" for p, v in ENV_CASES])
def test_env_name_sets_its_field(monkeypatch, param, value):
    _clean_env(monkeypatch)
    name = C.env_name(param)
    monkeypatch.setenv(name, C.env_value(param, value))
    want = qp.QdParams(**{param: value})
    if name == "QD_RHO_A":                     # one variable, two readers (humidity.py:65 and ocean.py:55)
        want = qp.QdParams(rho_a=value, rho_a_ocean=value)
    assert _same(qp.QdParams.from_env(), want)


def test_env_words_and_unset_spellings(monkeypatch):
    _clean_env(monkeypatch)
    for name, word, field, code in (("QD_MOM_SCHEME", "primitive", "mom_scheme", 1), ("QD_MOM_SCHEME", "geos", "mom_scheme", 0),
                                    ("QD_FILTER_TYPE", "combo", "filter_type", 0), ("QD_FILTER_TYPE", "hyper4", "filter_type", 1),
                                    ("QD_FILTER_TYPE", "Shapiro", "filter_type", 2), ("QD_FILTER_TYPE", "spectral", "filter_type", 3),
                                    ("QD_FILTER_TYPE", "none", "filter_type", 4),
                                    ("QD_OCEAN_OUTLIER", "mean4", "ocean_outlier", 0), ("QD_OCEAN_OUTLIER", "clamp", "ocean_outlier", 1),
                                    ("QD_SNOW_MELT_MODE", "degree_day", "snow_melt_mode", 0),
                                    ("QD_SNOW_MELT_MODE", "constant", "snow_melt_mode", 1)):
        monkeypatch.setenv(name, word)
        assert getattr(qp.QdParams.from_env(), field) == code, (name, word)
        monkeypatch.delenv(name)
    # the words the table's rows use are the ones the reference was given when the fixtures were made
    assert qp.QdParams(filter_type="spectral").filter_type == 3 and qp.QdParams(ocean_outlier="clamp").ocean_outlier == 1
    # "unset": the NaN-default parameters stay NaN, the others keep their default
    for n, env, dflt in qp._DOUBLES:
        if env is None:
            continue
        for spelling in ("", "None", "null"):
            monkeypatch.setenv(env, spelling)
            got = getattr(qp.QdParams.from_env(), n)
            assert (math.isnan(got) and math.isnan(dflt)) or got == dflt, (env, spelling, got)
        monkeypatch.delenv(env)
