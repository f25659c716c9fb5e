"""NumPy restatement of one speciation event on the LAI stack (test infrastructure), written from its description: a fraction
f = clip(frac, 0, 0.5) of the parent species' LAI moves, layer by layer, into a new last species; every plane is clipped to
[0, lai_max]; the total LAI is the sum over species within a layer, then over the layers; the species weights are the land sums
of sum_k max(x, 0) per species (NaN skipped), divided by their sum and clipped to [0, 1] -- uniform when that sum is not positive.
The goldens tests/golden/speciation_*.npz, made by the reference's own classes, pin it bitwise.

`replay(z)` runs a golden's whole sequence -- firings through tests/eco_daily_ref.py, events through `split` -- and yields the
state after every stage (LAI: the layer-wise total, what an event leaves in ECO_LAI; total_LAI: np.sum(axis=(0, 1)), what a plain
firing leaves there); the mode of a species born from an event is `new_mode(index)`."""
import numpy as np

import eco_daily_ref as pref


def split(layers, parent, frac, lai_max):
    """[S, K, lat, lon] -> [S + 1, K, lat, lon]; transfer is one multiply, the parent's remainder one subtract."""
    S = layers.shape[0]
    p = int(np.clip(parent, 0, S - 1))
    f = float(np.clip(frac, 0.0, 0.5))
    new = np.zeros((S + 1,) + layers.shape[1:], dtype=float)
    new[:S] = layers
    with np.errstate(invalid="ignore"):                         # inf - f * inf is NaN, and stays
        transfer = f * layers[p]
        new[p] = layers[p] - transfer
        new[S] = transfer
        return np.clip(new, 0.0, lai_max)


def total(layers):
    """The total LAI an event leaves: species summed within a layer, then the layers (a plain firing's is np.sum(axis=(0, 1)))."""
    return np.sum(np.sum(layers, axis=0), axis=0)


def weights(layers, land):
    S = layers.shape[0]
    L_s = np.sum(np.maximum(layers, 0.0), axis=1)
    totals = np.array([float(np.nansum(L_s[s][land])) for s in range(S)])
    ssum = float(np.sum(totals))
    if ssum <= 0:
        return np.full((S,), 1.0 / float(S))
    return np.clip(totals / ssum, 0.0, 1.0)


def new_mode(index):
    return "seed" if index == 1 else "diffusion"


def env_of(z):
    return dict(zip((str(k) for k in z["env_keys"]), (str(v) for v in z["env_vals"])))


def replay(z):
    """-> [(tag, state dict)] after every stage of the golden's sequence, the parents taken from the golden."""
    env = env_of(z)
    land = z["land_mask"] == 1
    cfg = pref.Cfg.from_env(env, [str(m) for m in z["modes"]], z["species_weights0"])
    st = pref.State(land, z["L0"].copy(), None, np.zeros(land.shape), z["bank0"].copy(), land.astype(float))
    frac, smax = float(env.get("QD_ECO_MUT_EPS", "0.02")), int(env.get("QD_ECO_SPECIES_MAX", "8"))
    w = cfg.weights
    out, hit = [], 0
    for d in range(int(z["n_firings"])):
        st.E_day = z["E_days"][d].copy()
        pref.step_daily(st, cfg, z["soil"][d])
        if d in z["hit_firings"].tolist():
            hit += 1
            if st.layers.shape[0] < smax:
                st.layers = split(st.layers, int(z[f"hit{hit}_parent"]), frac, cfg.lai_max)
                w = weights(st.layers, land)
                cfg.weights = w
                cfg.modes = cfg.modes + [new_mode(len(cfg.modes))]
        out.append((f"s{d + 1}", {"stack": st.layers.copy(), "LAI": total(st.layers), "total_LAI": st.total(), "weights": np.array(w, dtype=float), "age": st.age.copy(),
                                  "bank": st.bank.copy()}))
    return out
