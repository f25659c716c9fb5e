"""NumPy restatement of the ecology autosave (test infrastructure), written from its description: the two load rules, the layout of
the saved file and the genes document.  The goldens tests/golden/eco_state_*.npz and genes_eco_state_mixed.json, made by the
reference's own EcologyAdapter and PopulationManager, pin it bitwise.

The reference rule (`load_rule`): L = clip(LAI, 0, lai_max); w = clip(w, 0) / sum, or uniform when the sum is 0; every plane
[s][k] = float(w_s) * (L / float(K)).  NumPy carries the dtype of the file's arrays through all of it -- float32 from a NetCDF file,
float64 from an NPZ -- and only the store into the float64 stack widens; np.clip passes NaN and there is no land mask.  total_LAI()
afterwards is the sum of the planes, which differs from L in the last bit.
The exact rule: the qd_* variables are put back as saved, when every shape fits (`fits`).
"""
import numpy as np

NC_CORE = {  # name -> (dtype code, dims) of the reference's variable set (adapter.py:608-652)
    "lat": ("f4", ("lat",)), "lon": ("f4", ("lon",)), "LAI": ("f4", ("lat", "lon")), "species_weights": ("f4", ("species",)),
    "bands_lambda_centers": ("f4", ("band",)), "bands_delta_lambda": ("f4", ("band",)), "w_b": ("f4", ("band",)),
    "R_species_nb": ("f4", ("species", "band")), "day_value": ("f4", ()),
}
NC_EXT = {  # the qd_* extension variables of QD_ECO_PERSIST=2, all f8
    "qd_LAI_layers_SK": ("f8", ("species", "layer", "lat", "lon")), "qd_LAI": ("f8", ("lat", "lon")), "qd_age_days": ("f8", ("lat", "lon")),
    "qd_seed_bank": ("f8", ("lat", "lon")), "qd_E_day": ("f8", ("lat", "lon")), "qd_species_weights": ("f8", ("species",)),
    "qd_accum_day": ("f8", ()), "qd_eco_clock": ("f8", ("qd_clock",)),
}
NC_EXT_INDIV = {"qd_indiv_E_day": ("f8", ("qd_indiv",)), "qd_indiv_stress_days": ("f8", ("qd_indiv",))}
NC_ATTRS = {"title": "Qingdai Ecology State", "schema_version": 1, "source": "EcologyAdapter.save_autosave"}
GENE_FIELDS = ("index", "identity", "provenance", "alloc_root", "alloc_stem", "alloc_leaf", "leaf_area_per_energy", "drought_tolerance",
               "gdd_germinate", "lifespan_days", "peaks_model", "peaks")
PEAK_FIELDS = ("center_nm", "sigma_nm", "variance_nm2", "height")


def load_weights(w):
    w = np.clip(np.asarray(w), 0.0, None)
    ssum = float(np.sum(w))
    return (w / ssum) if ssum > 0 else np.full((w.size,), 1.0 / float(max(w.size, 1)), dtype=float)


def load_rule(LAI, w, K, lai_max):
    """-> (L = pop.LAI, species_weights, LAI_layers_SK [S, K, lat, lon] float64, total_LAI) in the dtypes NumPy gives them."""
    L = np.clip(np.asarray(LAI), 0.0, lai_max)
    sw = load_weights(w)
    K = max(1, int(K))
    stack = np.zeros((sw.size, K) + L.shape, dtype=float)
    for s in range(sw.size):
        for k in range(K):
            stack[s, k] = float(sw[s]) * (L / float(K))
    return L, sw, stack, np.sum(stack, axis=(0, 1))


def load_rule_f32(LAI, w, K, lai_max):
    """The same rule spelled out in float32 scalars, cell by cell operation by operation (what the device kernel does)."""
    f = np.float32
    L = np.asarray(LAI, dtype=f)
    with np.errstate(invalid="ignore"):
        L = np.where(np.isnan(L), L, np.minimum(np.maximum(L, f(0.0)), f(lai_max)))
    sw = load_weights(np.asarray(w, dtype=f))
    q = L / f(max(1, int(K)))
    stack = np.stack([np.stack([(f(ws) * q).astype(np.float64)] * max(1, int(K))) for ws in sw])
    return L, sw, stack, np.sum(stack, axis=(0, 1))


def fits(v, S, K, shape, n_indiv):
    """Do the qd_* variables of a file fit a run with S species, K layers, the grid `shape` and n_indiv individuals (0: none)?"""
    if any(n not in v for n in NC_EXT):
        return False
    if np.shape(v["qd_LAI_layers_SK"])[1:] != (K,) + tuple(shape) or np.shape(v["qd_species_weights"]) != (np.shape(v["qd_LAI_layers_SK"])[0],):
        return False
    if any(np.shape(v[n]) != tuple(shape) for n in ("qd_LAI", "qd_age_days", "qd_seed_bank", "qd_E_day")) or np.size(v["qd_eco_clock"]) != 3:
        return False
    if (n_indiv > 0) != ("qd_indiv_E_day" in v):
        return False
    return n_indiv == 0 or (np.shape(v["qd_indiv_E_day"]) == (n_indiv,) and np.shape(v.get("qd_indiv_stress_days")) == (n_indiv,))


def nc_layout(S, NB, shape, with_R=True, with_day=True, level=1, K=1, n_indiv=0):
    """-> (dims, {name: (code, dims)}) of the file save_autosave writes."""
    dims = {"lat": shape[0], "lon": shape[1], "species": S, "band": NB}
    names = dict(NC_CORE)
    if not with_R:
        del names["R_species_nb"]
    if not with_day:
        del names["day_value"]
    if level == 2:
        names.update(NC_EXT)
        dims.update({"layer": K, "qd_clock": 3})
        if n_indiv > 0:
            names.update(NC_EXT_INDIV)
            dims["qd_indiv"] = n_indiv
    return dims, names


def gene_reflectance(lambda_centers, peaks):
    """R = clip(1 - clip(sum_p h exp(-(lam - c)^2 / (2 sigma^2)), 0, 1), 0, 1); peaks with sigma <= 0 or h <= 0 are skipped."""
    lam = np.asarray(lambda_centers, dtype=float)
    A = np.zeros_like(lam)
    for c, s, h in peaks:
        if s <= 0 or h <= 0:
            continue
        A += h * np.exp(-((lam - c) ** 2) / (2 * (s ** 2)))
    return np.clip(1.0 - np.clip(A, 0.0, 1.0), 0.0, 1.0)


def peaks_of(rec):
    """The (center, sigma, height) list of one genes.json record: sigma_nm where positive, else sqrt(max(0, variance_nm2))."""
    out = []
    for pk in rec.get("peaks", []) or []:
        sigma = float(pk.get("sigma_nm", 0.0))
        if sigma <= 0 and "variance_nm2" in pk:
            sigma = float(np.sqrt(max(0.0, float(pk.get("variance_nm2", 0.0)))))
        out.append((float(pk.get("center_nm", 0.0)), sigma, float(pk.get("height", 0.0))))
    return out


def check_genes_document(doc, S, NB):
    """Schema 3 (adapter.py:320-346): raises AssertionError where the document is not of it."""
    assert doc["schema_version"] == 3 and doc["source"] == "PyGCM.EcologyAdapter.save_genes_json"
    assert doc["bands"]["nbands"] == NB and len(doc["bands"]["band_weights"]) == NB
    assert len(doc["genes"]) == S and len(doc["species_weights"]) == S
    for i, rec in enumerate(doc["genes"]):
        assert tuple(rec) == GENE_FIELDS and rec["index"] == i and rec["peaks_model"] == "gaussian"
        for pk in rec["peaks"]:
            assert tuple(pk) == PEAK_FIELDS and pk["variance_nm2"] == pk["sigma_nm"] * pk["sigma_nm"]
