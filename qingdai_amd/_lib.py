"""
qingdai_amd/_lib.py -- ctypes binding of libqingdai_hip.so (include/qingdai_hip.h).

There is no CPU fallback: if the HIP library is missing or no GPU is visible the
product raises.  (The oracle under oracle/ is test infrastructure and is never
imported from here.)
"""
from __future__ import annotations

import ctypes
import os

from .params import qd_params

_HERE = os.path.dirname(os.path.abspath(__file__))
LIB_PATH = os.environ.get("QD_LIB_PATH") or os.path.join(_HERE, "libqingdai_hip.so")     # QD_LIB_PATH: developer A/B builds

# field ids (enum qd_field)
FIELDS = ["U", "V", "H", "TS", "Q", "CLOUD", "HICE", "ISR", "ISR_A", "ISR_B", "TEQ", "ALBEDO",
          "OLR", "EFLUX", "PCOND", "LH", "LHREL", "CLOUD_EFF", "FRICTION", "CSMAP", "BASE_ALBEDO", "ELEVATION",
          "UO", "VO", "ETA", "SST", "QNET", "PRECIP", "CLOUD_FROM_P", "CLOUD_SRC", "W_LAND", "S_SNOW", "C_SNOW",
          "S_SNOW_NEXT", "MELT", "P_RAIN", "GLACIER", "RUNOFF",
          "ECO_LAI", "ECO_LAI_SNAP", "ECO_F", "ECO_EDAY", "ECO_ALPHA", "ECO_ALPHA_BANDED", "WATER_ALPHA",
          "ECO_AGE", "ECO_SEEDBANK", "ECO_GATE", "PHYTO_N", "KD490"]
F = {n: i for i, n in enumerate(FIELDS)}
F["LAND_MASK"] = 100
F["ICE_MASK"] = 101
# results of the last qd_eco_diversity call (qd_eco_diversity_download; ids behind the masks, the f64 slab list above is unchanged)
F.update({"ECO_DIV_LS": 110, "ECO_DIV_ALPHA": 111, "ECO_DIV_BC": 112, "ECO_DIV_SUMMARY": 113})
R_SUM, R_COSMEAN, R_MAX, R_MIN, R_MAXABS = 0, 1, 2, 3, 4

# every symbol include/qingdai_hip.h declares
SYMBOLS = [
    "qd_abi_version", "qd_device_count", "qd_create", "qd_destroy", "qd_last_error", "qd_upload", "qd_download", "qd_set_params",
    "qd_get_step_counter", "qd_set_step_counter", "qd_forcing", "qd_simple_albedo", "qd_atmos_step",
    "qd_ocean_step", "qd_driver_physics", "qd_hydrology_commit", "qd_step_n", "qd_last_ocean_nsub", "qd_sync",
    "qd_op_laplacian", "qd_op_hyperdiffuse", "qd_op_advect", "qd_op_shapiro", "qd_op_zonal_filter", "qd_op_divergence",
    "qd_op_vorticity", "qd_op_gaussian", "qd_op_median_positive", "qd_median_state", "qd_step_scalars", "qd_ocean_mean_next_count", "qd_reduce", "qd_energy_diagnostics", "qd_energy_diagnostics_last", "qd_band_insolation",
    "qd_comm_unique_id", "qd_comm_init", "qd_comm_init_local", "qd_comm_stats", "qd_comm_allreduce_count", "qd_comm_grouped_sum_count", "qd_comm_init_shm", "qd_comm_host_allreduce_count", "qd_hostring_open", "qd_hostring_allreduce",
    "qd_hostring_close", "qd_comm_barrier", "qd_comm_allreduce_max", "qd_peer_export", "qd_peer_connect", "qd_comm_peer_stats", "qd_comm_peer_carried", "qd_peer_selftest", "qd_peer_disable", "qd_tune_reload",
    "qd_plansim_create", "qd_plansim_destroy", "qd_plansim_plan", "qd_plansim_mark", "qd_plansim_margin", "qd_plansim_segments",
    "qd_plansim_pop_exchange", "qd_plansim_segments_rows",
    "qd_eco_configure", "qd_eco_set_lai_layers", "qd_eco_substep", "qd_eco_banded_alpha", "qd_eco_get_state", "qd_eco_set_state",
    "qd_indiv_configure", "qd_indiv_substep", "qd_indiv_download", "qd_indiv_upload",
    "qd_phyto_configure", "qd_phyto_upload", "qd_phyto_download", "qd_phyto_advect_diffuse",
    "qd_phyto_daily_configure", "qd_phyto_daily", "qd_phyto_daily_schedule", "qd_phyto_daily_log", "qd_phyto_daily_download_bands",
    "qd_phyto_daily_state", "qd_phyto_daily_insolation",
    "qd_eco_daily_configure", "qd_eco_daily_set_layers", "qd_eco_daily_get_layers", "qd_eco_daily_step", "qd_eco_daily_schedule",
    "qd_eco_daily_log", "qd_eco_daily_state", "qd_eco_daily_speciate",
    "qd_eco_state_restore",
    "qd_indiv_daily_configure", "qd_indiv_daily_step", "qd_indiv_daily_log", "qd_indiv_daily_weights", "qd_indiv_daily_state",
    "qd_eco_diversity", "qd_eco_diversity_on", "qd_eco_diversity_download",
    "qd_truecolor_configure", "qd_truecolor_render", "qd_truecolor_download",
    "qd_stateframe_configure", "qd_stateframe_scan", "qd_stateframe_render", "qd_stateframe_download",
    "qd_tiles_configure", "qd_tiles_set_plane", "qd_tiles_available", "qd_tiles_scan", "qd_tiles_order_stats", "qd_tiles_render", "qd_tiles_download",
    "qd_budget_diag_configure", "qd_budget_diag_schedule", "qd_budget_diag_log", "qd_budget_diag_reset",
    "qd_history_configure", "qd_history_schedule", "qd_history_sample", "qd_history_read", "qd_history_reset", "qd_history_restore",
    "qd_state_digest", "qd_state_scalars_get", "qd_state_scalars_set",
    "qd_route_configure", "qd_route_free", "qd_route_reset", "qd_route_accumulate", "qd_route_event", "qd_route_schedule",
    "qd_route_download", "qd_route_events", "qd_route_restore",
    "qd_hydronet_build", "qd_hydronet_sweeps",
    "qd_topogen_smooth", "qd_topogen_build", "qd_topogen_last_ms",
    "qd_copy_ceiling", "qd_timing_enable", "qd_timing_select", "qd_timing_get", "qd_timing_reset",
]


class qd_eco_params(ctypes.Structure):
    """include/qingdai_hip.h: qd_eco_params"""
    _fields_ = ([(n, ctypes.c_double) for n in ("k_canopy", "leaf_scalar", "soil_ref", "w_lai", "light_update_hours",
                                                 "recompute_lai_delta")] +
                [(n, ctypes.c_int32) for n in ("substep_every_nphys", "albedo_couple", "bands_couple", "water_couple", "use_lai", "map_f32")])


class qd_phyto_daily_params(ctypes.Structure):
    """include/qingdai_hip.h: qd_phyto_daily_params"""
    _fields_ = ([(n, ctypes.c_int32) for n in ("n_species", "n_bands", "idx_490", "enable_N", "couple", "reserved")] +
                [(n, ctypes.c_double) for n in ("H_mld", "alpha_P", "Q10", "T_ref", "kd_exp_m", "sink", "R_remin", "alpha_clip_min",
                                                 "alpha_clip_max", "dt_days")])


class qd_eco_daily_params(ctypes.Structure):
    """include/qingdai_hip.h: qd_eco_daily_params"""
    _fields_ = ([(n, ctypes.c_int32) for n in ("n_species", "n_layers", "spread", "moore", "gate_soil", "reserved")] +
                [(n, ctypes.c_double) for n in ("lai_max", "k_canopy", "growth_per_j", "senesce_per_day", "stress_thresh", "stress_strength",
                                                 "soil_cap", "repro_frac", "spread_rate", "soil_exp", "upfrac", "dlai_max", "seed_energy",
                                                 "seed_scale", "seedling_lai", "retain", "bank_max", "seed_dlai_max", "germ_frac",
                                                 "bank_decay")])


class qd_indiv_daily_params(ctypes.Structure):
    """include/qingdai_hip.h: qd_indiv_daily_params"""
    _fields_ = ([(n, ctypes.c_int32) for n in ("n_species", "n_layers", "per_cell", "seed_couple")] +
                [(n, ctypes.c_double) for n in ("stress_penalty", "lai_grow", "lai_decay", "recruit_frac", "stress_decay", "repro_frac",
                                                 "seed_energy", "retain", "bank_max", "lai_max")])


class qd_truecolor_params(ctypes.Structure):
    """include/qingdai_hip.h: qd_truecolor_params"""
    _fields_ = ([(n, ctypes.c_int32) for n in ("snow_by_swe", "veg", "veg_f_one", "oceancolor", "snow_by_ts", "rivers", "lakes", "nb_eco",
                                                "nb_phyto", "reserved")] +
                [(n, ctypes.c_double) for n in ("h_ice_ref", "ice_frac_thr", "snow_cover_frac", "snow_vis_alpha", "veg_gamma", "veg_sat",
                                                 "soil_ref", "oc_gamma", "oc_blend", "snow_thresh", "cloud_alpha", "cloud_white",
                                                 "river_min", "river_alpha", "lake_alpha")])


TRUECOLOR_MAX_BANDS = 16     # QD_TRUECOLOR_MAX_BANDS

STATEFRAME_PANELS = 15       # QD_STATEFRAME_PANELS
STATEFRAME_MAX_LEVELS = 32   # QD_STATEFRAME_MAX_LEVELS
STATEFRAME_GUTTER = 4        # QD_STATEFRAME_GUTTER
STATEFRAME_SCAN_N = 28       # QD_STATEFRAME_SCAN_N


class qd_stateframe_params(ctypes.Structure):
    """include/qingdai_hip.h: qd_stateframe_params"""
    _fields_ = ([(n, ctypes.c_int32) for n in ("ps_abs", "ocean", "rivers", "lakes")] +
                [(n, ctypes.c_double) for n in ("p0", "rho_a", "H", "river_min", "river_alpha", "lake_alpha")])


class qd_stateframe_panel(ctypes.Structure):
    """include/qingdai_hip.h: qd_stateframe_panel"""
    _fields_ = ([(n, ctypes.c_int32) for n in ("n_levels", "extend_max", "constant", "coast")] +
                [("levels", ctypes.c_double * STATEFRAME_MAX_LEVELS), ("rgb", (ctypes.c_double * 3) * STATEFRAME_MAX_LEVELS)])


class qd_stateframe_table(ctypes.Structure):
    """include/qingdai_hip.h: qd_stateframe_table"""
    _fields_ = [("panel", qd_stateframe_panel * STATEFRAME_PANELS), ("mark_cell", ctypes.c_int64 * 2)]


TILES_MAX = 8                # QD_TILES_MAX
TILES_MAX_RANKS = 4          # QD_TILES_MAX_RANKS
# enum qd_tile_source
TILE_SOURCES = ("LAI", "ALPHA", "ALPHA_BANDED", "CANOPY_HEIGHT", "SPECIES_DENSITY", "PLANKTON", "ISR_A", "ISR_B", "HOST_PLANE")
TILE = {n: i for i, n in enumerate(TILE_SOURCES)}


class qd_tile_ref(ctypes.Structure):
    """include/qingdai_hip.h: qd_tile_ref"""
    _fields_ = [("source", ctypes.c_int32), ("index", ctypes.c_int32)]


class qd_tile_desc(ctypes.Structure):
    """include/qingdai_hip.h: qd_tile_desc"""
    _fields_ = ([(n, ctypes.c_int32) for n in ("source", "index", "n_levels", "extend_max", "constant", "unavailable", "coast", "mark_kind")] +
                [("mark_cell", ctypes.c_int64), ("levels", ctypes.c_double * STATEFRAME_MAX_LEVELS),
                 ("rgb", (ctypes.c_double * 3) * STATEFRAME_MAX_LEVELS)])


SPAN_LOG_CAP = 4096          # records a span lane's device log holds between two drains (csrc/qd_span.h: QD_SPAN_LOG_CAP is the same number)
PHYTO_DAILY_LOG_W = 4        # doubles per [PhytoDiag] record
ECO_DAILY_LOG_W = 4          # doubles per daily vegetation record {firings, LAI_min, LAI_mean, LAI_max}
INDIV_DAILY_LOG_W = 4        # doubles per record of the individuals' daily step {firings, beta_hint, n_cells, levels}
BUDGET_LOG_W = 40           # doubles per budget diagnostics record (QD_BUDGET_LOG_W; budget_diag.REC names the slots)
HISTORY_MAX_ENTRIES = 32     # QD_HISTORY_MAX_ENTRIES
ROUTE_LOG_W = 8              # doubles per routing event record (routing.LOG_KEYS)
STATE_DIGEST_MAX = 64        # QD_STATE_DIGEST_MAX: refs per qd_state_digest call
STATE_SCALARS_N = 32         # QD_STATE_SCALARS_N
# the slots of qd_state_scalars_get / set the host reads by name (csrc/qd_digest.hip lists all of them)
STATE_SCALAR_SLOT = {"cloud_eff_valid": 0, "has_elevation": 1, "phyto_daily_steps": 17, "eco_daily_fired": 18, "indiv_daily_fired": 19, "last_nsub": 20}
# enum qd_state_ref: the resident planes without a field id, as Device.digest names them ("PHYTO_TRACER:3", "HISTORY_SUM:0")
STATE_REFS = {"PHYTO_TRACER": 200, "ROUTE_BUFFER": 300, "ROUTE_FLOW": 301, "ROUTE_LAKES": 302, "ECO_LAI_STACK": 310,
              "INDIV_E_DAY": 320, "INDIV_STRESS": 321, "HISTORY_SUM": 400}
STATE_REF_COUNT = {"PHYTO_TRACER": 64, "HISTORY_SUM": 32}     # the indexed ones: name:k with k below this


def state_ref(name):
    """A plane's name -> the ref qd_state_digest takes: a field name of F (f64 fields and the two masks), a name of STATE_REFS, or
    an indexed one, "PHYTO_TRACER:s" / "HISTORY_SUM:k"."""
    if name in FIELDS or name in ("LAND_MASK", "ICE_MASK"):
        return F[name]
    base, _, idx = str(name).partition(":")
    if base in STATE_REF_COUNT and idx.isdigit() and int(idx) < STATE_REF_COUNT[base]:
        return STATE_REFS[base] + int(idx)
    if base in STATE_REFS and base not in STATE_REF_COUNT and not idx:
        return STATE_REFS[base]
    raise KeyError(f"'{name}' names no resident plane (a field of FIELDS, LAND_MASK, ICE_MASK, {', '.join(STATE_REFS)})")

# qd_step_n flags (include/qingdai_hip.h): bit k switches STEP_BITS[k], named as Device.step_n's keywords
STEP_BITS = ("with_ocean", "with_physics", "pass_albedo", "with_hydrology", "energy_diag", "ecology", "phyto", "routing", "phyto_daily", "eco_daily")


def step_flags(**on):
    return sum(1 << STEP_BITS.index(k) for k, v in on.items() if v)


class qd_route_plan(ctypes.Structure):
    """include/qingdai_hip.h: qd_route_plan"""
    _fields_ = ([(n, ctypes.c_int32) for n in ("n_cells", "n_seg", "n_seg_cells", "n_levels", "n_jp", "n_lakes", "pe_lakes",
                                                "reserved")] +
                [("cflags", ctypes.c_void_p), ("area_row", ctypes.c_void_p), ("code", ctypes.c_void_p),
                 ("seg_start", ctypes.c_void_p), ("seg_cells", ctypes.c_void_p), ("level_start", ctypes.c_void_p),
                 ("jp_start", ctypes.c_void_p), ("jp_cells", ctypes.c_void_p), ("lake_start", ctypes.c_void_p),
                 ("lake_cells", ctypes.c_void_p), ("lake_frac", ctypes.c_void_p)])


class qd_grid_desc(ctypes.Structure):
    _fields_ = [(n, ctypes.c_int32) for n in ("n_lat", "n_lon", "row0", "n_rows", "halo", "device", "rank", "world")]


_lib = None


class QdError(RuntimeError):
    pass


def load():
    """Load the HIP library; fail loudly when it is absent (no fallback path exists)."""
    global _lib
    if _lib is not None:
        return _lib
    if not os.path.exists(LIB_PATH):
        raise QdError(f"{LIB_PATH} not found: build it with `python -c 'import __graft_entry__ as g; g.build()'` "
                      f"or `make -C qingdai_amd/csrc` (hipcc, gfx950). There is no CPU fallback.")
    lib = ctypes.CDLL(LIB_PATH, mode=ctypes.RTLD_GLOBAL)
    vp, dp, i32, i64, dbl, sz = (ctypes.c_void_p, ctypes.POINTER(ctypes.c_double), ctypes.c_int, ctypes.c_int64,
                                 ctypes.c_double, ctypes.c_size_t)
    ip, u8p = ctypes.POINTER(i32), ctypes.POINTER(ctypes.c_uint8)
    lib.qd_create.argtypes = [ctypes.POINTER(qd_grid_desc), ctypes.POINTER(qd_params), dbl, ctypes.POINTER(vp)]
    lib.qd_destroy.argtypes = [vp]
    lib.qd_last_error.argtypes = [vp]
    lib.qd_upload.argtypes = [vp, i32, vp, sz]
    lib.qd_download.argtypes = [vp, i32, vp, sz]
    lib.qd_set_params.argtypes = [vp, ctypes.POINTER(qd_params), sz]
    lib.qd_get_step_counter.argtypes = [vp, ctypes.POINTER(i64), ctypes.POINTER(i64)]
    lib.qd_set_step_counter.argtypes = [vp, i64, i64]
    lib.qd_forcing.argtypes = [vp, dp, dp, dbl, i32]
    lib.qd_simple_albedo.argtypes = [vp, dbl]
    lib.qd_atmos_step.argtypes = [vp, dbl, i32]
    lib.qd_ocean_step.argtypes = [vp, dbl, i32, i32, i32]
    lib.qd_driver_physics.argtypes = [vp, dbl]
    lib.qd_hydrology_commit.argtypes = [vp, dbl]
    lib.qd_step_n.argtypes = [vp, i32, dbl, i32, dp]
    lib.qd_last_ocean_nsub.argtypes = [vp, ctypes.POINTER(i32)]
    lib.qd_sync.argtypes = [vp]
    lib.qd_op_laplacian.argtypes = [vp, vp, i32, vp]
    lib.qd_op_hyperdiffuse.argtypes = [vp, vp, vp, dbl, dbl, i32, i32, vp]
    lib.qd_op_advect.argtypes = [vp, vp, vp, vp, dbl, i32, vp]
    lib.qd_op_shapiro.argtypes = [vp, vp, i32, vp]
    lib.qd_op_zonal_filter.argtypes = [vp, vp, dbl, dbl, vp]
    lib.qd_op_divergence.argtypes = [vp, vp, vp, vp]
    lib.qd_op_vorticity.argtypes = [vp, vp, vp, vp]
    lib.qd_op_gaussian.argtypes = [vp, vp, dbl, i32, vp]
    lib.qd_op_median_positive.argtypes = [vp, vp, dbl, dp]
    lib.qd_reduce.argtypes = [vp, i32, i32, dp]
    lib.qd_energy_diagnostics.argtypes = [vp, dp]
    lib.qd_energy_diagnostics_last.argtypes = [vp, dp]
    lib.qd_copy_ceiling.argtypes = [vp, sz, i32, dp]
    lib.qd_band_insolation.argtypes = [vp, i32, dp, dp, dp, vp]
    lib.qd_eco_configure.argtypes = [vp, ctypes.POINTER(qd_eco_params), sz]
    lib.qd_eco_set_lai_layers.argtypes = [vp, vp, i32, i32]
    lib.qd_eco_substep.argtypes = [vp, dbl]
    lib.qd_eco_banded_alpha.argtypes = [vp, i32, dp, dp]
    lib.qd_eco_get_state.argtypes = [vp, dp]
    lib.qd_eco_set_state.argtypes = [vp, dp]
    lib.qd_indiv_configure.argtypes = [vp, i32, ip, ip, i32, ip, vp, vp, i32, dp, dp, dp, i32, dbl, dbl, i32]
    lib.qd_indiv_substep.argtypes = [vp, dbl, ip]
    lib.qd_indiv_download.argtypes = [vp, vp, vp]
    lib.qd_indiv_upload.argtypes = [vp, vp, vp]
    lib.qd_phyto_configure.argtypes = [vp, i32, dbl, dbl]
    lib.qd_phyto_upload.argtypes = [vp, i32, vp]
    lib.qd_phyto_download.argtypes = [vp, i32, vp]
    lib.qd_phyto_advect_diffuse.argtypes = [vp, dbl]
    lib.qd_phyto_daily_configure.argtypes = [vp, ctypes.POINTER(qd_phyto_daily_params), sz, dp, dp, dp]
    lib.qd_phyto_daily.argtypes = [vp, dp, i32]
    lib.qd_phyto_daily_schedule.argtypes = [vp, i32, ip]
    lib.qd_phyto_daily_log.argtypes = [vp, dp, i32, ip]
    lib.qd_phyto_daily_download_bands.argtypes = [vp, dp, sz]
    lib.qd_phyto_daily_state.argtypes = [vp, ctypes.POINTER(i64)]
    lib.qd_phyto_daily_insolation.argtypes = [vp, dp, dp, dp]
    lib.qd_eco_daily_configure.argtypes = [vp, ctypes.POINTER(qd_eco_daily_params), sz, ip, dp]
    lib.qd_eco_daily_set_layers.argtypes = [vp, vp, i32]
    lib.qd_eco_daily_get_layers.argtypes = [vp, vp, i32]
    lib.qd_eco_state_restore.argtypes = [vp, vp, i32, dp, i32, i32, ctypes.c_double]
    lib.qd_eco_daily_step.argtypes = [vp, vp]
    lib.qd_eco_daily_schedule.argtypes = [vp, i32, ip]
    lib.qd_eco_daily_log.argtypes = [vp, dp, i32, ip]
    lib.qd_eco_daily_state.argtypes = [vp, ctypes.POINTER(i64)]
    lib.qd_eco_daily_speciate.argtypes = [vp, i32, ctypes.c_double, dp]
    lib.qd_indiv_daily_configure.argtypes = [vp, ctypes.POINTER(qd_indiv_daily_params), sz, ip, ip]
    lib.qd_indiv_daily_step.argtypes = [vp, vp]
    lib.qd_indiv_daily_log.argtypes = [vp, dp, i32, ip]
    lib.qd_indiv_daily_weights.argtypes = [vp, dp, i32]
    lib.qd_indiv_daily_state.argtypes = [vp, ctypes.POINTER(i64)]
    lib.qd_eco_diversity.argtypes = [vp, vp, i32, i32, dp, dp]
    lib.qd_eco_diversity_on.argtypes = [vp, i32, i32, u8p, vp, i32, i32, dp, dp]
    lib.qd_eco_diversity_download.argtypes = [vp, i32, dp, sz]
    lib.qd_truecolor_configure.argtypes = [vp, ctypes.POINTER(qd_truecolor_params), sz, dp, dp, dp, u8p]
    lib.qd_truecolor_render.argtypes = [vp, i32, dp, dp]
    lib.qd_truecolor_download.argtypes = [vp, i32, vp, sz]
    lib.qd_stateframe_configure.argtypes = [vp, ctypes.POINTER(qd_stateframe_params), sz, u8p]
    lib.qd_stateframe_scan.argtypes = [vp, dp, ctypes.POINTER(i64)]
    lib.qd_stateframe_render.argtypes = [vp, ctypes.POINTER(qd_stateframe_table), sz, dp, i32]
    lib.qd_stateframe_download.argtypes = [vp, i32, vp, sz]
    lib.qd_tiles_configure.argtypes = [vp, dbl, dp, i32, i32]
    lib.qd_tiles_set_plane.argtypes = [vp, dp]
    lib.qd_tiles_available.argtypes = [vp, ip]
    lib.qd_tiles_scan.argtypes = [vp, ctypes.POINTER(qd_tile_ref), i32, dp, ctypes.POINTER(i64)]
    lib.qd_tiles_order_stats.argtypes = [vp, i32, i32, ctypes.POINTER(i64), i32, dp, ctypes.POINTER(i64)]
    lib.qd_tiles_render.argtypes = [vp, ctypes.POINTER(qd_tile_desc), sz, i32, i32]
    lib.qd_tiles_download.argtypes = [vp, i32, vp, sz]
    lib.qd_budget_diag_configure.argtypes = [vp, i32, u8p]
    lib.qd_budget_diag_schedule.argtypes = [vp, i32, ip]
    lib.qd_budget_diag_log.argtypes = [vp, dp, i32, ip]
    lib.qd_budget_diag_reset.argtypes = [vp]
    lib.qd_history_configure.argtypes = [vp, i32, ip, ip, ip]
    lib.qd_history_schedule.argtypes = [vp, i32, ip]
    lib.qd_history_sample.argtypes = [vp]
    lib.qd_history_read.argtypes = [vp, dp, ctypes.POINTER(i64)]
    lib.qd_history_reset.argtypes = [vp]
    lib.qd_history_restore.argtypes = [vp, dp, i64]
    lib.qd_state_digest.argtypes = [vp, i32, ip, ctypes.POINTER(ctypes.c_uint64)]
    lib.qd_state_scalars_get.argtypes = [vp, dp, i32]
    lib.qd_state_scalars_set.argtypes = [vp, dp, i32]
    lib.qd_comm_unique_id.argtypes = [vp, sz]
    lib.qd_comm_init.argtypes = [vp, vp, sz]
    lib.qd_comm_barrier.argtypes = [vp]
    lib.qd_comm_init_local.argtypes = [ctypes.POINTER(vp), i32]
    lib.qd_median_state.argtypes = [vp, dp]
    lib.qd_step_scalars.argtypes = [vp, dp]
    lib.qd_ocean_mean_next_count.argtypes = [vp, ctypes.POINTER(i64)]
    lib.qd_comm_stats.argtypes = [vp, ctypes.POINTER(i32)]
    lib.qd_comm_allreduce_count.argtypes = [vp, ctypes.POINTER(i32)]
    lib.qd_comm_grouped_sum_count.argtypes = [vp, ctypes.POINTER(i32)]
    lib.qd_comm_init_shm.argtypes = [vp, ctypes.c_char_p]
    lib.qd_comm_host_allreduce_count.argtypes = [vp, ctypes.POINTER(i32)]
    lib.qd_hostring_open.argtypes = [ctypes.c_char_p, i32, i32, ctypes.POINTER(vp)]
    lib.qd_hostring_allreduce.argtypes = [vp, dp, i32, i32]
    lib.qd_hostring_close.argtypes = [vp]
    lib.qd_comm_allreduce_max.argtypes = [vp, dp, i32]
    lib.qd_tune_reload.argtypes = [vp]
    lib.qd_peer_export.argtypes = [vp, vp, sz]
    lib.qd_peer_connect.argtypes = [vp, vp, sz, i32]
    lib.qd_peer_selftest.argtypes = [vp, i32, ctypes.POINTER(ctypes.c_longlong)]
    lib.qd_peer_disable.argtypes = [vp]
    lib.qd_comm_peer_stats.argtypes = [vp, ctypes.POINTER(i32), ctypes.POINTER(i32)]
    lib.qd_comm_peer_carried.argtypes = [vp]
    lib.qd_plansim_create.argtypes = [ctypes.POINTER(qd_grid_desc), ctypes.POINTER(vp)]
    lib.qd_plansim_destroy.argtypes = [vp]
    lib.qd_plansim_plan.argtypes = [vp, ip, ip, i32, i32]
    lib.qd_plansim_mark.argtypes = [vp, ip, i32, i32]
    lib.qd_plansim_margin.argtypes = [vp, i32]
    lib.qd_plansim_segments.argtypes = [vp, i32, ip]
    lib.qd_plansim_pop_exchange.argtypes = [vp, ip, i32, ip]
    lib.qd_plansim_segments_rows.argtypes = [vp, i32, i32, ip]
    lib.qd_route_configure.argtypes = [vp, ctypes.POINTER(qd_route_plan), sz]
    lib.qd_route_free.argtypes = [vp]
    lib.qd_route_reset.argtypes = [vp]
    lib.qd_route_accumulate.argtypes = [vp, dbl]
    lib.qd_route_event.argtypes = [vp, dbl, i32]
    lib.qd_route_schedule.argtypes = [vp, i32, dp]
    lib.qd_route_download.argtypes = [vp, i32, dp, sz]
    lib.qd_route_events.argtypes = [vp, dp, i32, ip]
    lib.qd_route_restore.argtypes = [vp, dp, dp, dp, i64]
    lib.qd_hydronet_build.argtypes = [vp, i32, i32, u8p, dp, dbl, i32, dp, dp, dp, dbl, dp, ip, ip, u8p, ip, ip, i32,
                                      ip, ip]
    lib.qd_hydronet_sweeps.argtypes = [vp, ip]
    lib.qd_topogen_smooth.argtypes = [vp, i32, i32, dp, dp, i32, dp, i32, i32, dp]
    lib.qd_topogen_build.argtypes = [vp, i32, i32, dp, i32, dp, dp, i32, dp, dp, dp, dp, dp, ip, dp, dp, u8p, dp]
    lib.qd_topogen_last_ms.argtypes = [vp, dp]
    lib.qd_timing_enable.argtypes = [vp, i32]
    lib.qd_timing_select.argtypes = [vp, ctypes.c_char_p]
    lib.qd_timing_get.argtypes = [vp, ctypes.c_char_p, dp, ctypes.POINTER(i64)]
    lib.qd_timing_reset.argtypes = [vp]
    for s in SYMBOLS:
        getattr(lib, s).restype = i32
    lib.qd_last_error.restype = ctypes.c_char_p
    _lib = lib
    return lib
