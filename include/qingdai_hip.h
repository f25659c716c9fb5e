/*
 * include/qingdai_hip.h -- C-ABI of libqingdai_hip.so (MI355X / gfx950).
 *
 * Drop-in boundary for the per-timestep lat-lon grid update of PyGCM-for-Qingdai.
 * The reference has no FFI for this path: its seam is Python level
 *  --
 *   (1) the class surface  pygcm/dynamics.py:22-23,260  SpectralModel(...).time_step(Teq, dt, albedo=None)
 *                          pygcm/ocean.py:28-34,265     WindDrivenSlabOcean(...).step(dt, u, v, Q_net, ice_mask)
 *                          + the free functions of physics/energy/humidity/forcing the driver calls
 *                            (scripts/run_simulation.py:25,36), and
 *   (2) the operator seam  pygcm/jax_compat.py:111,135,190
 *                          laplacian_sphere / hyperdiffuse / advect_semilag gated by is_enabled().
 * Every entry point below names the reference interface it replaces.  Plain C:
 * handles, pointers, sizes; no C++ or torch types.  All arrays are C-order
 * float64 [n_lat][n_lon] (uint8 for masks) in HOST memory, borrowed for the call.
 * The library owns all device memory.  Return 0 = OK, negative = error (see
 * qd_last_error); nothing throws or aborts.  One HIP stream per handle; a handle
 * is not thread-safe.  Steps are asynchronous: qd_download / qd_sync / qd_reduce
 * synchronise.
 */
#ifndef QINGDAI_HIP_H
#define QINGDAI_HIP_H

#include <stddef.h>
#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

#define QD_ABI_VERSION 1

typedef struct qd_ctx* qd_handle;

/* Grid + latitude-band descriptor.  Single GPU: row0 = 0, n_rows = n_lat, halo = 0.
 * Multi GPU (one process per GPU): rows [row0, row0 + n_rows) of the global grid are
 * owned; `halo` extra rows are kept on each side and refreshed by qd_halo_* (RCCL). */
typedef struct qd_grid_desc {
    int32_t n_lat, n_lon;
    int32_t row0, n_rows, halo;
    int32_t device;            /* HIP device ordinal */
    int32_t rank, world;       /* band index / number of bands */
} qd_grid_desc;

/* Field ids: one per array attribute of the reference classes (+ static maps). */
enum qd_field {
    /* SpectralModel prognostic state (dynamics.py:56-66,84) */
    QD_F_U = 0, QD_F_V, QD_F_H, QD_F_TS, QD_F_Q, QD_F_CLOUD, QD_F_HICE,
    /* per-step inputs assigned by the driver (run_simulation.py:1943-1944,2191) */
    QD_F_ISR, QD_F_ISR_A, QD_F_ISR_B, QD_F_TEQ, QD_F_ALBEDO,
    /* diagnostics written by time_step (dynamics.py:294-297,353,411) */
    QD_F_OLR, QD_F_EFLUX, QD_F_PCOND, QD_F_LH, QD_F_LHREL, QD_F_CLOUD_EFF,
    /* static maps (dynamics.py:25-31; topography.py:295-346) */
    QD_F_FRICTION, QD_F_CSMAP, QD_F_BASE_ALBEDO, QD_F_ELEVATION,
    /* WindDrivenSlabOcean state + forcing (ocean.py:86-94,265-270) */
    QD_F_UO, QD_F_VO, QD_F_ETA, QD_F_SST, QD_F_QNET,
    /* driver-side diagnostics (run_simulation.py:1778,1876,1884,2144) */
    QD_F_PRECIP, QD_F_CLOUD_FROM_P, QD_F_CLOUD_SRC,
    /* land hydrology reservoirs (run_simulation.py:1289-1290; hydrology.py) */
    QD_F_W_LAND, QD_F_S_SNOW, QD_F_C_SNOW,
    /* P019 provisional snow / land bucket working fields (run_simulation.py:1946-2019, 2290-2339) */
    QD_F_S_SNOW_NEXT, QD_F_MELT, QD_F_P_RAIN, QD_F_GLACIER, QD_F_RUNOFF,
    /* ecology, per physics step (population.py:252-294,831-915; adapter.py:140-186; run_simulation.py:2075-2128):
     * total LAI, its snapshot at the last canopy recompute, cached canopy factor f, daily energy buffer, land-only
     * ecology alpha (NaN elsewhere), daily banded alpha, ocean-colour alpha of the phytoplankton coupling */
    QD_F_ECO_LAI, QD_F_ECO_LAI_SNAP, QD_F_ECO_F, QD_F_ECO_EDAY, QD_F_ECO_ALPHA, QD_F_ECO_ALPHA_BANDED, QD_F_WATER_ALPHA,
    /* daily vegetation step (population.py:389-596): age_days, seed_bank, _spread_gate */
    QD_F_ECO_AGE, QD_F_ECO_SEEDBANK, QD_F_ECO_GATE,
    /* daily phytoplankton step (phyto.py:339-435): nutrient pool N (mmol m^-3), Kd(490) (m^-1) */
    QD_F_PHYTO_N, QD_F_KD490,
    QD_F_COUNT_F64,
    /* uint8 masks */
    QD_F_LAND_MASK = 100, QD_F_ICE_MASK = 101,
    /* results of the last qd_eco_diversity call, read with qd_eco_diversity_download (not slabs: no qd_upload / qd_download):
     * L_s [n_species][n_lat][n_lon], alpha map, local Bray-Curtis map [n_lat][n_lon], {alpha_mean, gamma_eff, beta_whittaker} */
    QD_F_ECO_DIV_LS = 110, QD_F_ECO_DIV_ALPHA = 111, QD_F_ECO_DIV_BC = 112, QD_F_ECO_DIV_SUMMARY = 113
};

/* Every env-derived scalar the reference reads inside the step,
 * as one POD.  NaN in a double = "environment variable unset".  Field names equal
 * qingdai_amd.params.QdParams and oracle/qd_oracle/params.py. */
typedef struct qd_params {
    /* SpectralModel ctor: dynamics.py:22-41 */
    double g, H, tau_rad, greenhouse_factor, a, omega;
    double t_freeze, rho_i, L_f, Cs_ocean, Cs_land, Cs_ice;
    /* humidity.py:58-82 */
    double C_E, rho_a, h_mbl, L_v, p0, ocean_evap_scale, land_evap_scale, ice_evap_scale, tau_cond;
    /* energy.py:55-74; dynamics.py:316-386 */
    double sw_a0, sw_kc, lw_eps0, lw_kc, t_floor, c_sfc;
    double energy_w, rh0, k_q, k_p, pcond_ref, hice_ref, eps_default, ch, cp_a;
    double atm_h, gh_factor_lw, eps_ocean, eps_land, eps_ice, lw_tau0, lw_ktau;
    /* dynamics.py:534-658 */
    double sigma4, k4_u, k4_v, k4_h, k4_q, k4_cloud, spec_cutoff, spec_damp, diff_factor;
    /* ocean.py:49-75,380-443,519-533 */
    double H_ocean, rho_w, cp_w, g_ocean, CD, r_bot, rho_a_ocean, vcap, tau_scale;
    double polar_sponge_lat, polar_sponge_gain, K_h, sigma4_ocean, ocean_cfl, ocean_max_u;
    double ocean_k4_u, ocean_k4_v, ocean_k4_eta, ocean_adv_alpha, ocean_ice_qfac, eta_cap, ts_min, ts_max;
    /* driver physics: run_simulation.py:1605-1613,1777,1866-1934 */
    double D_crit, k_precip, alpha_water, alpha_ice, alpha_cloud, p_betadiv, pq_min, p_blend;
    double pref, cmax, w_mem, w_p, w_src, cloud_from_p_floor, cloud_adv_alpha, cloud_smooth_sigma;
    /* land hydrology + P019 lapse / snow: hydrology.py:27-80, run_simulation.py:1616-1627 */
    double runoff_tau_days, wland_cap_mm, snow_thresh_K, snow_melt_rate_mm_day, snow_t_band_K;
    double snow_ddf_mm_per_k_day, snow_melt_tref_K, swe_ref_mm, swe_max_mm, snow_albedo_fresh;
    double lapse_k_kpm, land_elev_max_m, polar_ice_thick_max_m, polar_lat_thresh, rho_snow, glacier_frac, glacier_swe_mm;
    /* orographic precipitation factor: physics.py:116-161, run_simulation.py:1612-1613,1769-1775 */
    double orog_k;
    /* the driver's own EnergyParams copy, nudged by autotune_greenhouse_params (energy.py:544-579,
     * run_simulation.py:1245-1257,2242-2246); NaN = same as lw_eps0 / lw_kc.  Only the coupling block (Q_net,
     * energy diagnostics) reads them, never time_step. */
    double qnet_lw_eps0, qnet_lw_kc;
    /* integer switches */
    int32_t seaice_enabled, cloud_couple, lw_v2, gh_lock, polar_freeze_fix_s, polar_freeze_fix_n;
    int32_t mom_scheme;        /* 0 geos, 1 primitive (QD_MOM_SCHEME) */
    int32_t diff_enable, filter_type; /* 0 combo, 1 hyper4, 2 shapiro, 3 spectral, 4 other */
    int32_t diff_every, k4_nsub, diff_q, diff_cloud, shapiro_every, shapiro_n, spec_every;
    int32_t ocean_k4_nsub, ocean_diff_every, ocean_shapiro_n, ocean_shapiro_every;
    int32_t ocean_outlier;     /* 0 mean4, 1 clamp */
    int32_t ocean_use_qnet, ocean_polar_fix;
    int32_t p_hybrid_fallback, cloud_advect, use_topo_albedo, has_csmap;
    int32_t snow_melt_mode;    /* 0 degree_day, 1 constant (QD_SNOW_MELT_MODE) */
    int32_t swe_enable, lapse_enable;
    int32_t orog_enable;       /* QD_OROG; takes effect once an ELEVATION field has been uploaded */
} qd_params;

/* ---- lifetime ------------------------------------------------------------------ */
int qd_abi_version(void);
int qd_device_count(void);   /* visible HIP devices (0 when none): what jax_compat.is_enabled() asks of its backend */
/* SpectralModel.__init__ / WindDrivenSlabOcean.__init__ (dynamics.py:22-88, ocean.py:28-97):
 * allocates every field on `desc->device`, fills the reference's initial state
 * (u=v=0, h=H+300 sin^2, T_s=288, q=RH0*q_sat(T_s), ocean at rest, SST=288). */
int qd_create(const qd_grid_desc* desc, const qd_params* params, double q_init_rh, qd_handle* out);
int qd_destroy(qd_handle h);
const char* qd_last_error(qd_handle h);   /* h may be NULL: error of the last failed qd_create */

/* ---- attribute surface: `gcm.u = arr` / `arr = gcm.u` (run_simulation.py:1441-1447,1900,2253) */
int qd_upload(qd_handle h, int field, const void* host_global, size_t bytes);
int qd_download(qd_handle h, int field, void* host_global, size_t bytes);
/* the reference re-reads its env every step (dynamics.py:330-650); callers re-send on change */
int qd_set_params(qd_handle h, const qd_params* params, size_t sizeof_params);
int qd_get_step_counter(qd_handle h, int64_t* atmos_counter, int64_t* ocean_counter);
int qd_set_step_counter(qd_handle h, int64_t atmos_counter, int64_t ocean_counter);

/* ---- the path ------------------------------------------------------------------- */
/* forcing.py:78-103,138-165: isr_A, isr_B, isr (and Teq from the ALBEDO field when with_teq)
 * from ten host scalars: per star (flux, declination, right ascension) + theta (+ sigma). */
int qd_forcing(qd_handle h, const double star_a[3], const double star_b[3], double theta, int with_teq);
/* benchmark_jax.py:129: albedo = where(land == 0, ocean_albedo, base_albedo) */
int qd_simple_albedo(qd_handle h, double ocean_albedo);
/* SpectralModel.time_step(Teq, dt, albedo) (dynamics.py:260-667); Teq/ISR/ALBEDO fields must be current */
int qd_atmos_step(qd_handle h, double dt, int has_albedo);
/* run_simulation.py:2197-2253 + ocean.py:265-533: Q_net from SW/LW/SH/LH, ice mask from h_ice,
 * WindDrivenSlabOcean.step, then T_s <- SST over open ocean.  compute_qnet=0 uses the QNET field
 * and ICE_MASK as uploaded; inject_sst=0 skips the write-back. */
int qd_ocean_step(qd_handle h, double dt, int compute_qnet, int use_ice_mask, int inject_sst);
/* run_simulation.py:1766-1934,2063-2146: hybrid precipitation, cloud-from-precip, cloud source,
 * cloud blend + advection, dynamic albedo (physics.py:12-354). */
int qd_driver_physics(qd_handle h, double dt);
/* run_simulation.py:2290-2339: commit the provisional snowpack, update the land bucket (hydrology.py:219-260) */
int qd_hydrology_commit(qd_handle h, double dt);
/* benchmark_jax.py:124-158 as one resident loop of n steps: forcing -> albedo -> time_step [-> ocean
 * coupling] [-> hydrology commit].  `flags` is a mask of enum qd_step_flag.  `stars` holds n rows of 7 host scalars
 * (flux_A, decl_A, ra_A, flux_B, decl_B, ra_B, theta), evaluated by the caller as forcing.py:85-125 does. */
enum qd_step_flag {
    QD_STEP_WITH_OCEAN = 1,        /* bit0: the ocean coupling */
    QD_STEP_WITH_PHYSICS = 2,      /* bit1: the driver physics (else the simple ocean/land albedo of benchmark_jax.py:129) */
    QD_STEP_PASS_ALBEDO = 4,       /* bit2: pass albedo to time_step */
    QD_STEP_WITH_HYDROLOGY = 8,    /* bit3: hydrology commit */
    QD_STEP_ENERGY_DIAG = 16,      /* bit4: energy diagnostics on the first step (qd_energy_diagnostics_last) */
    QD_STEP_ECOLOGY = 32,          /* bit5: ecology sub-step (qd_eco_substep, and qd_indiv_substep when a pool is configured; needs bit1) */
    QD_STEP_PHYTO = 64,            /* bit6: tracer transport after the ocean step (qd_phyto_advect_diffuse; needs bit0 and qd_phyto_configure) */
    QD_STEP_ROUTING = 128,         /* bit7: river routing after the hydrology commit (qd_route_accumulate, and qd_route_event on the steps a
                                      qd_route_schedule of n entries names; needs bit3 and qd_route_configure) */
    QD_STEP_PHYTO_DAILY = 256,     /* bit8: daily phytoplankton step at the top of the steps a qd_phyto_daily_schedule of n entries names
                                      (SST with bit0, else TS; needs bit1 and qd_phyto_daily_configure) */
    QD_STEP_ECO_DAILY = 512        /* bit9: daily vegetation step at the top of the steps a qd_eco_daily_schedule of n entries names (needs
                                      bit5 and qd_eco_daily_configure) */
};
int qd_step_n(qd_handle h, int n, double dt, int flags, const double* stars);
int qd_last_ocean_nsub(qd_handle h, int* n_sub);
int qd_sync(qd_handle h);

/* ---- operator seam: jax_compat.py:111-216 (host in, host out; global arrays) ------ */
/* cos floor kinds: 0 = max(cos,0.2) atmosphere, 1 = max(cos,0.5) ocean */
int qd_op_laplacian(qd_handle h, const double* F, int cos_kind, double* out);
/* k4_row: n_lat per-row coefficients, or NULL with scalar k4 */
int qd_op_hyperdiffuse(qd_handle h, const double* F, const double* k4_row, double k4_scalar, double dt,
                       int n_substeps, int cos_kind, double* out);
/* cos floor kinds: 0 = max(1e-6,cos) atmosphere, 1 = max(cos,0.5) ocean / driver cloud */
int qd_op_advect(qd_handle h, const double* field, const double* u, const double* v, double dt,
                 int cos_kind, double* out);
int qd_op_shapiro(qd_handle h, const double* F, int n, double* out);                /* dynamics.py:215-231 */
int qd_op_zonal_filter(qd_handle h, const double* F, double cutoff, double damp, double* out); /* dynamics.py:233-258 */
int qd_op_divergence(qd_handle h, const double* u, const double* v, double* out);   /* grid.py:41-68 */
int qd_op_vorticity(qd_handle h, const double* u, const double* v, double* out);    /* grid.py:70-88 */
int qd_op_gaussian(qd_handle h, const double* F, double sigma, int mode_wrap, double* out); /* physics.py:44 */
int qd_op_median_positive(qd_handle h, const double* x, double dflt, double* out);  /* dynamics.py:344-348 */
/* (new, diagnostics) the same median by the arguments the step's own call sites pass: transform 0 = x, 1 = max(0, -(x - tparam))
 * (physics.py:296); site 0..3 keeps a window on the device between calls, site -1 has none.  qd_op_median_positive is the call
 * with (0, 0.0, 0). */
int qd_op_median_at(qd_handle h, const double* x, double dflt, int transform, double tparam, int site, double* out);
/* (new, diagnostics) two medians through the step's pair chain (one set of three launches, two buffer sets): out2 = {median 0,
 * median 1}.  Whole-globe handles, two different sites that both have a window already; anything else is refused. */
int qd_op_median_pair(qd_handle h, const double* x0, double dflt0, int tr0, double tp0, int site0,
                      const double* x1, double dflt1, int tr1, double tp1, int site1, double* out2);
/* (new, diagnostics) the per-call-site state of the three in-step medians (dynamics.py:344-348, run_simulation.py:1740-1747,
 * 1866-1874): 4 sites x 16 doubles {last median, -, -, valid, hits, misses, candidates of the last call, positives of the last
 * call, bracket lo, hi, -, ok, calls, last miss: call, centre, result}; site 1 = P_cond, 2 = convergence, 3 = precipitation */
int qd_median_state(qd_handle h, double* out64);
/* (new, diagnostics) the device scalars the launches of a step hand to each other: {P_ref of P_cond, eta mean of the last ocean
 * sub-step, precipitation median, convergence scale (median of pos > 0), renormalisation s = <Pq> / <P_raw>, blend weight of the
 * legacy precipitation, 2 x scratch} */
int qd_step_scalars(qd_handle h, double* out8);
/* (new, diagnostics) ocean sub-steps since create whose eta mean was left to the next momentum launch (QD_MEAN_IN_MOMENTUM) */
int qd_ocean_mean_next_count(qd_handle h, int64_t* out);
/* (new, diagnostics) which form of the step kernels this handle takes: out[QD_SF_N].  The timing groups k_dyn_hyper / k_ocn_hyper are
 * shared by the row-streaming and the LDS-tile launchers and ocean_tail by three kernels; this says which.  Read-only, no launch, no
 * wait.  The geometry entries are what the launchers' own shape functions return for the handle's rows (margin 0); the QD_SF_LAST_*
 * entries are what the last atmosphere / ocean step noted where it decided (0 before the first step); the QD_SF_CNT_* / QD_SF_MAX_*
 * entries are host-side tallies since qd_create of the launch-by-launch decisions a latitude band makes (a band's margin shrinks from
 * launch to launch, so the LAST_* notes keep only the last of several forms): written beside the notes, never read by a launch. */
enum qd_step_form {
    QD_SF_DYN_STREAM,       /* momentum + del^4 of the atmosphere: 1 = k_dyn_stream, 0 = k_dyn_hyper<TR> (LDS tiles) */
    QD_SF_OCN_STREAM,       /* the same of the ocean sub-step: 1 = k_ocn_stream, 0 = k_ocn_hyper<TR> */
    QD_SF_DYN_NTC,          /* streaming form, atmosphere: column strips (58 owned columns each), */
    QD_SF_DYN_NRS,          /*   row strips, */
    QD_SF_DYN_R,            /*   rows of a strip, */
    QD_SF_DYN_VB,           /*   virtual rows that trim the north-pole strip */
    QD_SF_OCN_NTC,          /* streaming form, ocean: the same four */
    QD_SF_OCN_NRS,
    QD_SF_OCN_R,
    QD_SF_OCN_VB,
    QD_SF_TILE_TR,          /* tile form: owned rows of a tile, */
    QD_SF_TILE_NTR,         /*   row tiles, */
    QD_SF_TILE_NTC,         /*   column tiles (58 owned columns each), */
    QD_SF_TILE_DYN_FAST,    /*   row tiles of k_dyn_hyper whose workgroups take the FAST path (0: every tile EXACT), */
    QD_SF_TILE_OCN_FAST,    /*   the same of k_ocn_hyper */
    QD_SF_TAIL_KERNEL,      /* one-launch ocean tail this handle's launcher picks: 0 refuses (two launches), 1 k_ocn_tail_fast, 2 k_ocn_tail_stream */
    QD_SF_TAIL_NTC,         /*   column groups (60 owned columns each; k_ocn_tail_stream: 62), */
    QD_SF_TAIL_POLE,        /*   pole strips (k_ocn_tail_fast), */
    QD_SF_TAIL_MID,         /*   strips between them (k_ocn_tail_stream: all strips), */
    QD_SF_TAIL_R,           /*   rows of such a strip, */
    QD_SF_TAIL_RP,          /*   rows of a pole strip, */
    QD_SF_TAIL_GENERAL,     /*   1: every wave takes the general form (QD_TAIL_GENERAL) */
    QD_SF_FUSED_OK,         /* k_ocn_fused (QD_OCN_FUSED=1) accepts the grid; its column groups, middle strips, their rows, QD_FUSED_SEQ */
    QD_SF_FUSED_NTC,
    QD_SF_FUSED_NMID,
    QD_SF_FUSED_R,
    QD_SF_FUSED_SEQ,
    QD_SF_LAST_NSUB,        /* the last ocean step: sub-steps, */
    QD_SF_LAST_USE_TAIL,    /*   the rest of a sub-step was one launch, */
    QD_SF_LAST_TAIL_ACC,    /*   that launch reduced its own strip sums, */
    QD_SF_LAST_USE_FUSED1,  /*   the whole sub-step was one launch (k_ocn_fused), */
    QD_SF_LAST_MEAN_FORM,   /*   the eta mean of a sub-step was left to the next momentum launch (mean_form_ok), */
    QD_SF_LAST_FIX_NOW,     /*   the currents were patched in place through the fix list (fix_now), */
    QD_SF_LAST_TAIL_KERNEL, /*   last tail launch: 0 none, 1 k_ocn_tail_fast<false>, 2 k_ocn_tail_fast<true>, 3 k_ocn_tail_stream, 4 k_ocn_fused */
    QD_SF_LAST_DYN_FORM,    /* the last momentum launch of the atmosphere: 0 none (QD_FUSED=0), 1 streaming, 2 tiles */
    QD_SF_LAST_OCN_FORM,    /* the last momentum launch of the ocean: the same */
    QD_SF_CNT_DYN_STREAM,   /* since qd_create: calls of qd_launch_dyn_hyper that took k_dyn_stream, */
    QD_SF_CNT_DYN_TILE,     /*   that took k_dyn_hyper<TR>, */
    QD_SF_CNT_OCN_STREAM,   /*   calls of qd_launch_ocn_hyper that took k_ocn_stream -- the interior and boundary launches of a split sub-step go
                             *   past that launcher and are not among them; a split whose boundary is REDONE calls it and is counted, here or as a tile, */
    QD_SF_CNT_OCN_TILE,     /*   that took k_ocn_hyper<TR>, */
    QD_SF_CNT_SPLIT,        /*   ocean sub-steps whose interior rows were launched between the halo push and the unpack, */
    QD_SF_CNT_SPLIT_REDO,   /*   of those, the ones whose boundary strips were too thin: the whole launch redone in the other form, */
    QD_SF_CNT_STREAM_PAIR,  /*   k_ocn_stream_pair launches (the two boundary strips in one launch), */
    QD_SF_CNT_STREAM_PUSH,  /*   k_ocn_stream_push launches (a row segment with the halo push in front), */
    QD_SF_CNT_SUB_BAND_TAIL, /*  ocean sub-steps of a band on the band_tail path (one tail launch per row segment), */
    QD_SF_CNT_SUB_ROUND2,   /*   ocean sub-steps of a band on the round-2 path (k_cont_sstadv + k_sst_outlier_fused), */
    QD_SF_MAX_TAIL_SEGS,    /*   the most row segments a band tail ran on, */
    QD_SF_MAX_MOM_SEGS,     /*   the most row segments a call of qd_launch_dyn_hyper / qd_launch_ocn_hyper ran on, */
    QD_SF_CNT_TAIL_FIX,     /*   band tails that were handed the fix list (one segment, fix_now; the launcher still drops it when the kernel
                             *   it picks has no finishing wave), */
    QD_SF_CNT_DYN_TILE_FAST, /*  row tiles of the k_dyn_hyper launches that passed the kernel's own test for the FAST path (qd_fast_tile), */
    QD_SF_CNT_OCN_TILE_FAST, /*  the same of k_ocn_hyper (qd_fast_tile and QD_OCN_WRAP_OK), */
    QD_SF_CNT_TILE_EXACT,   /*   row tiles of either that did not (a segment shorter than the plane, an off-slab plane or pole row, QD_FUSED_FAST=0), */
    QD_SF_CNT_TILE_SHIFT,   /*   FAST row tiles whose plane was shifted to stay on the segment +- 5 rows (p0 != o0 - 5), */
    QD_SF_CNT_TILE_SLAB_EDGE, /* FAST row tiles whose plane ends on the last row of the slab (qd_lrow(p0) + RA == lrows) */
    QD_SF_N
};
int qd_step_forms(qd_handle h, int32_t* out);

/* ---- ecology spectral sub-step, first stage (pygcm/ecology/spectral.py:304-426) --------------------
 * dual_star_insolation_to_bands on the resident ISR_A / ISR_B: specA/specB/tray are the NB host-computed band weights of the
 * two stars and the Rayleigh factor; the result [nb][n_lat][n_lon] f64 stays resident and is also copied to `out_host_or_null`. */
int qd_band_insolation(qd_handle h, int nb, const double* specA, const double* specB, const double* tray, double* out_host_or_null);

/* ---- ecology, the per-physics-step part (BASELINE config 5; SURVEY.md 8(f)3 stages 2-4) --------------------------------
 * The daily population dynamics (population.py:389-830, individuals.py:193-361) stay host code that runs once per
 * planet-day; it hands the device the LAI layers and takes the energy buffers back. */
typedef struct qd_eco_params {
    double k_canopy;             /* QD_ECO_LAI_K (0.5): f = 1 - exp(-k max(LAI_tot, 0)), population.py:911-915 */
    double leaf_scalar;          /* adapter.py:61: sum_b R_leaf[b] w_b */
    double soil_ref;             /* QD_ECO_SOIL_REFLECT (0.20), adapter.py:170 */
    double w_lai;                /* QD_ECO_LAI_ALBEDO_WEIGHT (1.0), run_simulation.py:2089-2100 */
    double light_update_hours;   /* QD_ECO_LIGHT_UPDATE_EVERY_HOURS (6), population.py:62-65,900 */
    double recompute_lai_delta;  /* QD_ECO_LIGHT_RECOMPUTE_LAI_DELTA (0.05), population.py:66-69,903-907 */
    int32_t substep_every_nphys; /* QD_ECO_SUBSTEP_EVERY_NPHYS (1), adapter.py:156 */
    int32_t albedo_couple;       /* QD_ECO_SUBDAILY_ENABLE && QD_ECO_ALBEDO_COUPLE: run_simulation.py:2075 */
    int32_t bands_couple;        /* QD_ECO_BANDS_COUPLE: land base albedo <- clip(ECO_ALPHA_BANDED), run_simulation.py:2107-2112 */
    int32_t water_couple;        /* QD_PHYTO_ENABLE && QD_PHYTO_ALBEDO_COUPLE: ocean base albedo <- clip(WATER_ALPHA), :2121-2128 */
    int32_t use_lai;             /* QD_ECO_USE_LAI (1).  0 = the adapter's M1 branch (adapter.py:162-166): no population, no E_day,
                                    alpha = clip(leaf_scalar) on land */
    int32_t map_f32;             /* QD_ECO_F32 (0): store the canopy maps ECO_LAI, ECO_LAI_SNAP, ECO_F, ECO_ALPHA, ECO_ALPHA_BANDED as f32
                                    (arithmetic, the LAI plane sum, the lai-delta reduction and E_day stay f64); qd_upload /
                                    qd_download of these fields still exchange f64 with the host.  Fixed once the maps hold data. */
} qd_eco_params;
int qd_eco_configure(qd_handle h, const qd_eco_params* p, size_t sizeof_params);
/* PopulationManager.total_LAI (population.py:288-294): layers = [n_planes][n_lat][n_lon] host f64 (the flattened
 * [S][K] planes of LAI_layers_SK), summed plane after plane like np.sum(axis=(0,1)) into the resident ECO_LAI.
 * init != 0 also takes the constructor's snapshot (population.py:71). */
int qd_eco_set_lai_layers(qd_handle h, const double* layers, int n_planes, int init);
/* EcologyAdapter.step_subdaily (adapter.py:140-186) on the resident ISR: E_day += nan_to_num(isr) dt, canopy clock and
 * recompute policy (population.py:252-280,895-915), land-only alpha map on sub-step boundaries.  qd_step_n with flags
 * bit5 runs the same inside its loop, where the driver does (run_simulation.py:2075-2104). */
int qd_eco_substep(qd_handle h, double dt);
/* population.get_surface_albedo_bands + the driver's daily reduction (population.py:875-893, run_simulation.py:1843-1844):
 * ECO_ALPHA_BANDED <- clip(nansum_b clip(R_eff[b] f + (1 - f) soil, 0, 1) w_b, 0, 1); nb <= 32 */
int qd_eco_banded_alpha(qd_handle h, int nb, const double* r_eff, const double* w_b);
/* clock state for restarts / inspection: out[0] hours accumulated, [1] next time-based recompute, [2] step count,
 * [3] canopy recomputes so far, [4] 1 when an alpha map is cached */
int qd_eco_get_state(qd_handle h, double out[5]);
int qd_eco_set_state(qd_handle h, const double in[3]);        /* hours, next recompute, step count */

/* IndividualPool (individuals.py:37-191): n_cells sampled land cells (row j, column i), n_indiv individuals each bound to
 * one sampled cell, with a per-band coefficient row Ab[n_indiv][nb] and a drought tolerance; band tables as in
 * qd_band_insolation.  State (E_day, water-stress days) stays resident.  ab_f32 != 0 keeps the coefficient table -- the
 * only large array of the sub-step -- as f32 in HBM (the "f32 mixed precision" of BASELINE configs[4]); all arithmetic and
 * the state stay f64, so results move by the f32 rounding of Ab (<= 6e-8 relative). */
int qd_indiv_configure(qd_handle h, int n_cells, const int32_t* sample_j, const int32_t* sample_i, int n_indiv,
                       const int32_t* cell_index, const double* Ab, const double* tol, int nb, const double* specA,
                       const double* specB, const double* tray, int substeps_per_day, double day_seconds, double soil_cap,
                       int ab_f32);
/* IndividualPool.try_substep (individuals.py:142-191) on the resident ISR_A / ISR_B and the soil index
 * clip(W_LAND / max(1e-6, soil_cap), 0, 1) of run_simulation.py:2025-2033; *fired = 1 when a sub-step was consumed.
 * The band intensities are evaluated per sampled cell and never materialised as [NB][n_lat][n_lon]. */
int qd_indiv_substep(qd_handle h, double dt, int* fired_or_null);
int qd_indiv_download(qd_handle h, double* E_day, double* stress_days);   /* each [n_indiv]; band handles: own cells, 0 elsewhere */
int qd_indiv_upload(qd_handle h, const double* E_day, const double* stress_days);   /* daily reset / restart */

/* ---- phytoplankton tracers carried by the ocean currents (pygcm/ecology/phyto.py:496-547) ------------
 * PhytoManager.advect_diffuse on resident state: C_phyto_s [S][n_lat][n_lon] lives on the device next to the ocean's
 * uo / vo; the driver calls it once per step after the SST write-back (scripts/run_simulation.py:2254-2258).
 * K_h = QD_PHYTO_KH (phyto.py:123), adv_alpha = QD_PHYTO_ADV_ALPHA (phyto.py:517).  n_species = 0 frees the stack. */
int qd_phyto_configure(qd_handle h, int n_species, double K_h, double adv_alpha);
int qd_phyto_upload(qd_handle h, int species, const double* host);      /* [n_lat][n_lon] f64 */
int qd_phyto_download(qd_handle h, int species, double* host);
int qd_phyto_advect_diffuse(qd_handle h, double dt_seconds);             /* all species, three launches */

/* ---- daily phytoplankton step (P017, PhytoManager.step_daily, pygcm/ecology/phyto.py:339-435), whole-globe handles -------
 * One pointwise launch per planet-day on the resident tracers of qd_phyto_configure (n_species must match): the cell's two-star
 * insolation from the step's star row (7 scalars as in qd_step_n), the band split, Kd, mixed-layer light, growth, the nutrient
 * pool, the band reflectances and their scalar reduction.  Writes the tracers, PHYTO_N, KD490, WATER_ALPHA and a resident
 * [n_bands][n_lat][n_lon] band stack, and appends one record of QD_PHYTO_DAILY_LOG_W = 4 doubles to a device log:
 * {daily steps so far, <C_tot>, <Kd490>, <alpha_water>} with the max(cos lat, 0)-weighted means of the [PhytoDiag] line.
 * With `couple` set, the albedo launches override the ocean base albedo with clip(WATER_ALPHA, 0, 1) from the first daily step on
 * (run_simulation.py:2121-2128). */
#define QD_PHYTO_DAILY_LOG_W 4
#define QD_SPAN_LOG_CAP 4096          /* records the device log of a span lane (this one, the daily vegetation and individuals' steps, routing,
                                         the budget diagnostics) holds between two drains */
typedef struct qd_phyto_daily_params {
    int32_t n_species, n_bands;
    int32_t idx_490;             /* band nearest 490 nm */
    int32_t enable_N;            /* QD_PHYTO_ENABLE_N */
    int32_t couple;              /* QD_PHYTO_ALBEDO_COUPLE */
    int32_t reserved;
    double H_mld;                /* max(0.1, H) */
    double alpha_P, Q10, T_ref, kd_exp_m;
    double sink;                 /* lambda_sink / max(1e-6, H_mld) when lambda_sink > 0, else 0 */
    double R_remin;
    double alpha_clip_min, alpha_clip_max;
    double dt_days;              /* 1 in the driver */
} qd_phyto_daily_params;
/* band_tab [8][n_bands] rows: Kd0, k_chl, A_pure, delta_lambda, w (scalar reduction weights), specA, specB, T_ray (the band split
 * of qd_band_insolation); species_tab [6][n_species] rows: c_reflect, p_reflect, mu_max, m0, KN, Y; shape [n_species][n_bands].
 * The first call, and a call that changes n_bands, zeroes the band stack, KD490 and the step count. */
int qd_phyto_daily_configure(qd_handle h, const qd_phyto_daily_params* p, size_t sizeof_params, const double* band_tab,
                             const double* species_tab, const double* shape);
int qd_phyto_daily(qd_handle h, const double* star_row, int use_sst);   /* one daily step now (T_w = SST or TS) */
int qd_phyto_daily_schedule(qd_handle h, int n, const int32_t* fire);   /* the next qd_step_n span: 1 = the step fires */
int qd_phyto_daily_log(qd_handle h, double* out, int max, int* n);      /* drains the log: *n records of 4 doubles */
int qd_phyto_daily_download_bands(qd_handle h, double* host, size_t n); /* [n_bands][n_lat][n_lon] */
int qd_phyto_daily_state(qd_handle h, int64_t* n_steps);                /* daily steps run since the configure */
/* the two per-star insolation maps [n_lat][n_lon] the daily kernel evaluates for a star row (checks against qd_forcing) */
int qd_phyto_daily_insolation(qd_handle h, const double* star_row, double* insA, double* insB);

/* ---- daily vegetation step (PopulationManager.step_daily, pygcm/ecology/population.py:389-828), whole-globe handles --------
 * One firing: growth from E_day and senescence under soil-water stress, the layered Beer-Lambert allocation (K > 1), per-species
 * neighbour / seed spread in species order, age, soil-gated germination from the seed bank, its decay, ECO_LAI = sum of the
 * layers, E_day = 0; all f64 in the reference's operation order.  The [n_species][K][n_lat][n_lon] LAI stack is resident
 * (qd_eco_daily_set_layers / _get_layers); ECO_AGE, ECO_SEEDBANK and ECO_GATE are ordinary fields.  A firing leaves the canopy
 * state as qd_eco_set_lai_layers(h, layers, n, 0) does (snapshot and recompute clock untouched) and appends one record of
 * QD_ECO_DAILY_LOG_W = 4 doubles to a device log: {firings so far, LAI_min, LAI_mean, LAI_max} over land (summary(),
 * population.py:947-957; zeros without land).  The individuals' daily step runs behind it once configured (below); a speciation
 * event is qd_eco_daily_speciate; the gene table and the mutation's draws stay on the host. */
#define QD_ECO_DAILY_LOG_W 4
#define QD_ECO_DAILY_MAX_K 8
typedef struct qd_eco_daily_params {
    int32_t n_species, n_layers;      /* Ns (1..64), QD_ECO_COHORT_K (1..8) */
    int32_t spread;                   /* QD_ECO_SPREAD_ENABLE == 1 and QD_ECO_SPREAD_RATE > 0 */
    int32_t moore;                    /* QD_ECO_SPREAD_NEIGHBORS in moore / 8 / 8n, else von Neumann */
    int32_t gate_soil;                /* QD_ECO_SPREAD_GATE_SOIL */
    int32_t reserved;
    double lai_max, k_canopy, growth_per_j, senesce_per_day, stress_thresh, stress_strength;   /* LAIParams */
    double soil_cap;                  /* QD_ECO_SOIL_WATER_CAP: soil = clip(W_LAND / max(1e-6, cap), 0, 1), 0 on GLACIER */
    double repro_frac;                /* clip(QD_ECO_REPRO_FRACTION, 0, 0.95) */
    double spread_rate;               /* clip(QD_ECO_SPREAD_RATE, 0, 0.5) */
    double soil_exp, upfrac, dlai_max;
    double seed_energy, seed_scale;   /* max(1e-12, .) */
    double seedling_lai, retain, bank_max, seed_dlai_max, germ_frac, bank_decay;
} qd_eco_daily_params;
/* species_mode [n_species]: 0 diffusion, 1 seed; species_weights [n_species]: already divided by (their sum + 1e-12).
 * The first call, and a call that changes n_species * n_layers, allocates the stack; every call zeroes ECO_AGE and ECO_SEEDBANK,
 * the firing count and the log.  Refused on latitude bands. */
int qd_eco_daily_configure(qd_handle h, const qd_eco_daily_params* p, size_t sizeof_params, const int32_t* species_mode,
                           const double* species_weights);
int qd_eco_daily_set_layers(qd_handle h, const double* layers, int n_planes);   /* [n_species * n_layers][n_lat][n_lon] */
int qd_eco_daily_get_layers(qd_handle h, double* layers, int n_planes);
/* one firing now.  soil_index NULL: from the resident W_LAND and GLACIER, as inside a span; else a host [n_lat][n_lon] map,
 * the soil_water_index argument of step_daily */
int qd_eco_daily_step(qd_handle h, const double* soil_index);
int qd_eco_daily_schedule(qd_handle h, int n, const int32_t* fire);   /* the next qd_step_n span: firings at the top of each step */
int qd_eco_daily_log(qd_handle h, double* out, int max, int* n);      /* drains the log: *n records of 4 doubles */
int qd_eco_daily_state(qd_handle h, int64_t* n_firings);              /* firings since the configure */
/* one speciation event on the resident stack (PopulationManager.add_species_from_parent, population.py:361-387): a new
 * [(n_species + 1) * K] stack is allocated, one pass over the cells fills it from the old one -- transfer = f * x_p with
 * f = clip(frac, 0, 0.5) and p = clip(parent, 0, n_species - 1), the parent plane x_p - transfer, the new (last) species transfer,
 * every plane clipped to [0, lai_max] (NaN passes), all bit for bit -- and the stacks are swapped.  The same pass writes ECO_LAI
 * (species summed within a layer, then the layers) and the per-species land sums, from which one workgroup derives
 * species_weights (totals / their sum clipped to [0, 1]; 1 / (n_species + 1) when the sum is <= 0) -> weights_out
 * [n_species + 1] and the lane's germination weights w / (sum(w) + 1e-12).  The weights differ from NumPy's by the blocked order
 * of the land sums.  The mode table grows by the mode the reference gives an index its list does not hold (seed for index 1,
 * else diffusion); n_species grows by one.  ECO_AGE, ECO_SEEDBANK, ECO_EDAY, ECO_GATE, the firing count, the log and a pending
 * schedule are untouched; the canopy state is left as by qd_eco_set_lai_layers(h, stack, n, 0).  Refused: latitude bands, no
 * qd_eco_daily_configure, n_species + 1 > 64, a configured qd_indiv_daily (its pool was sampled for the old species), frac <= 0
 * (the reference adds no species then). */
int qd_eco_daily_speciate(qd_handle h, int parent, double frac, double* weights_out);

/* ---- restore of the vegetation state from an ecology autosave (EcologyAdapter.load_autosave, pygcm/ecology/adapter.py:742-757),
 * whole-globe handles ---------------------------------------------------------------------------------------------------------
 * lai: the file's [n_lat][n_lon] LAI plane, float32 (lai_is_f32 != 0: what a NetCDF file hands the reference) or float64 (its NPZ
 * branch).  w [n_species]: the species weights as the reference leaves them -- clipped at 0 and divided by their sum, or uniform
 * when the sum is 0.  One launch over the cells: L = np.clip(LAI, 0, lai_max) (NaN passes, +inf -> lai_max, no land mask: ocean
 * cells keep their values), q = L / n_layers, plane[s][k] = w_s * q for all n_species * n_layers planes -- with lai_is_f32 the
 * clip, the IEEE divide and the multiply are float32 (subnormals kept) and only the store widens, as NumPy >= 2 runs it; else all
 * f64.  The planes go into the resident stack of qd_eco_daily_configure when that exists (n_species / n_layers must be its);
 * ECO_LAI receives their sum in np.sum(axis=(0,1))'s order, f64 -- total_LAI() after the load, which differs from the clipped
 * plane pop.LAI in the last bit.  Leaves the canopy state as qd_eco_set_lai_layers(h, stack, n, 0) does; ECO_AGE, ECO_SEEDBANK,
 * E_day and the clocks are untouched, as in the reference.  Refused: latitude bands, no qd_eco_configure, n_species outside
 * 1..64, n_layers outside 1..8, a shape that is not the resident stack's. */
int qd_eco_state_restore(qd_handle h, const void* lai, int lai_is_f32, const double* w, int n_species, int n_layers,
                         double lai_max);

/* ---- daily step of the sampled individuals (IndividualPool.step_daily, pygcm/ecology/individuals.py:193-361; driver call
 * scripts/run_simulation.py:1818-1835), whole-globe handles ----------------------------------------------------------------------
 * Needs qd_indiv_configure (the pool, per_cell consecutive individuals per sampled cell) and qd_eco_daily_configure (the resident
 * stack).  One firing, f64 in the reference's operation order, no atomics:
 *   1 per sampled cell   E, stress days and counts per species in individual order (np.add.at, :219-235), denom, the weights, the
 *                        stress penalty and the renormalisation (:224-243) into per-cell tables; the seed bank (:316-335)
 *   2 one workgroup      medE = np.median(denom[denom > 0]) or 1.0 (:252), exact; beta_hint = mean_c max_s W (:359)
 *   3 per level          the cell loop (:259-306): cells of one level of the host's plan write disjoint grid cells and run in one
 *                        launch, levels in ascending order -- the sequential loop, bit for bit
 *   4 whole stack        clip to [0, lai_max], ECO_LAI (:308-310), per-species land sums -> species_weights (population.py:343-359)
 *                        and the daily lane's normalised germination weights
 *   6 per individual     E_day = 0, stress relief / decay / +1 capped at 365 (:340-356)
 * Once configured, every firing of the bit9 lane inside qd_step_n runs this step directly behind the vegetation step, on the
 * same soil index.  A firing appends {firings so far, beta_hint, n_cells, levels} to a log of its own (QD_SPAN_LOG_CAP records). */
#define QD_INDIV_DAILY_LOG_W 4
typedef struct qd_indiv_daily_params {
    int32_t n_species, n_layers;      /* must be the stack's */
    int32_t per_cell;                 /* QD_ECO_INDIV_PER_CELL: individuals c * per_cell .. belong to sampled cell c */
    int32_t seed_couple;              /* QD_ECO_INDIV_SEED_COUPLE == 1 (default 1) */
    double stress_penalty;            /* QD_ECO_INDIV_STRESS_PENALTY 0.2; <= 0: no penalty and the cell's mean stress is 0 */
    double lai_grow, lai_decay;       /* QD_ECO_LAI_GROWTH_RATE 0.002, QD_ECO_LAI_DECAY_RATE 0.001 */
    double recruit_frac;              /* QD_ECO_LAI_RECRUIT_FRAC 0.2 */
    double stress_decay;              /* QD_ECO_INDIV_STRESS_DECAY 0.5 */
    double repro_frac, seed_energy;   /* pop.repro_fraction, pop.seed_energy as read (individuals.py:319-320) */
    double retain, bank_max;          /* QD_ECO_SEED_BANK_RETAIN 0.2, QD_ECO_SEED_BANK_MAX 1000 */
    double lai_max;                   /* pop.params.lai_max */
} qd_indiv_daily_params;
/* species_id [n_indiv]: 0 .. n_species-1.  level [n_cells]: the 1-based level of every sampled cell, level(c) = 1 + max(level of
 * the earlier cells that write a grid cell c writes); checked here (two cells of a level share no grid cell, a later cell that
 * shares one has the higher level).  Refused: latitude bands, no qd_indiv_configure / qd_eco_daily_configure, n_species or n_layers
 * that differ from the stack's, n_cells * per_cell != n_indiv or a cell index that is not i / per_cell.  A later
 * qd_indiv_configure or qd_eco_daily_configure drops this configuration. */
int qd_indiv_daily_configure(qd_handle h, const qd_indiv_daily_params* p, size_t sizeof_params, const int32_t* species_id,
                             const int32_t* level);
/* one firing now (the class seam).  soil_index as in qd_eco_daily_step: NULL = from the resident W_LAND and GLACIER */
int qd_indiv_daily_step(qd_handle h, const double* soil_index);
int qd_indiv_daily_log(qd_handle h, double* out, int max, int* n);    /* drains the log: *n records of 4 doubles */
int qd_indiv_daily_weights(qd_handle h, double* w, int n_species);    /* species_weights after the last firing */
int qd_indiv_daily_state(qd_handle h, int64_t* n_firings);            /* firings since the configure; 0 when not configured */

/* ---- diversity diagnostics (pygcm/ecology/diversity.py:8-135; scripts/run_simulation.py:2406-2414), whole-globe handles ------
 * From a [n_species][n_layers][n_lat][n_lon] LAI stack and the ecology's land mask (land == 1), f64 in the reference's operation
 * order: L_s = sum_k max(stack, 0) (plane after plane), the alpha map exp(-sum_s p log(p + 1e-15)) with p = L_s / (L_tot + 1e-15)
 * on land with L_tot > 0 (NaN elsewhere), the mean Bray-Curtis dissimilarity to the up / down / west / east neighbours that are land
 * (rows clipped at the poles, columns periodic; NaN off land), and the Whittaker summary {alpha_mean, gamma_eff, beta_whittaker}
 * from nansum(alpha w_norm) and nansum(L_s w_norm) over land.  w_norm_row [n_lat] is the reference's
 * max(cos(deg2rad(lat)), 0) / (sum over land + 1e-15), computed by the caller.  layers NULL: the resident stack of
 * qd_eco_daily_configure (n_species / n_layers must be its); else a host stack, uploaded to a scratch buffer allocated on first
 * use.  L_s and the Bray-Curtis map equal NumPy's bit for bit; alpha and the summary differ by the device log / exp and by the
 * blocked order of the two global sums (per-workgroup partials, one-workgroup finish, fixed order, no atomics).  The results stay
 * resident until the next call (qd_eco_diversity_download); summary3 (may be NULL) also receives the three doubles.  The call
 * changes nothing else: no field, no canopy version, no snapshot, no clock, no lane log.  Refused: latitude bands, n_species
 * outside 1..64, n_layers outside 1..QD_ECO_DAILY_MAX_K, layers NULL without a configured stack of that shape. */
int qd_eco_diversity(qd_handle h, const double* layers, int n_species, int n_layers, const double* w_norm_row, double* summary3);
/* the same kernels on a grid and land mask of the caller's (host [n_lat][n_lon] uint8, land == 1; layers a host stack): a saved
 * community at another resolution.  n_lat >= 2, n_lon >= 3.  The handle lends its device and stream. */
int qd_eco_diversity_on(qd_handle h, int n_lat, int n_lon, const uint8_t* land_mask, const double* layers, int n_species,
                        int n_layers, const double* w_norm_row, double* summary3);
/* field: QD_F_ECO_DIV_LS (n = n_species * cells), _ALPHA, _BC (n = cells), _SUMMARY (n = 3) of the last call on this handle */
int qd_eco_diversity_download(qd_handle h, int field, double* host, size_t n);

/* ---- true-colour frame (scripts/run_simulation.py:539-778, plot_true_color), whole-globe handles ----------------------------
 * The reference's rgb_map[n_lat][n_lon][3] and the two numbers of its [TrueColor] line, composed in one launch from the resident
 * HICE, C_SNOW, CLOUD, TS, ISR, ISR_A, ISR_B, ECO_F, the land mask, the phytoplankton band stack and the routing flow map, f64 in
 * the reference's operation order: base colours -> sea ice (1 - exp(-max(h_ice, 0) / max(1e-6, h_ice_ref)) >= ice_frac_thr on the
 * ocean) -> land snow blend -> vegetation overlay -> ocean-colour overlay (open ocean only) -> snow by T_s -> clouds -> rivers ->
 * lakes -> clip.  The per-band irradiance of the two overlays is recomputed per cell from ISR_A / ISR_B with the rule of
 * qd_band_insolation; no [NB]-plane stack of it is read.  The only operations that are not exactly NumPy's are exp and pow. */
#define QD_TRUECOLOR_MAX_BANDS 16
typedef struct qd_truecolor_params {
    int32_t snow_by_swe;              /* QD_TRUECOLOR_SNOW_BY_SWE == 1 */
    int32_t veg;                      /* QD_ECO_TRUECOLOR_VEG == 1 and an ecology adapter exists */
    int32_t veg_f_one;                /* no population (QD_ECO_USE_LAI=0): f = 1 on land, R_eff = R_leaf */
    int32_t oceancolor;               /* QD_PLOT_OCEANCOLOR == 1 and a daily phytoplankton manager exists */
    int32_t snow_by_ts;               /* QD_TRUECOLOR_SNOW_BY_TS == 1 */
    int32_t rivers;                   /* routing exists and QD_PLOT_RIVERS == 1 */
    int32_t lakes;                    /* routing exists and its lake mask has a set cell */
    int32_t nb_eco, nb_phyto;         /* bands of the two overlays, 0..QD_TRUECOLOR_MAX_BANDS */
    int32_t reserved;
    double h_ice_ref, ice_frac_thr;   /* QD_HICE_REF, QD_TRUECOLOR_ICE_FRAC */
    double snow_cover_frac, snow_vis_alpha;   /* QD_SNOW_COVER_FRAC, QD_SNOW_VIS_ALPHA */
    double veg_gamma, veg_sat, soil_ref;      /* QD_ECO_TRUECOLOR_GAMMA, QD_ECO_TRUECOLOR_SAT, QD_ECO_SOIL_REFLECT */
    double oc_gamma, oc_blend;        /* QD_OC_GAMMA, QD_OC_BLEND */
    double snow_thresh;               /* QD_SNOW_THRESH */
    double cloud_alpha, cloud_white;  /* QD_TRUECOLOR_CLOUD_ALPHA, QD_TRUECOLOR_CLOUD_WHITE */
    double river_min, river_alpha, lake_alpha;   /* QD_RIVER_MIN_KGPS, QD_RIVER_ALPHA, QD_LAKE_ALPHA */
} qd_truecolor_params;
/* eco_tab [7][nb_eco]: R_eff, the channel weights wr, wg, wb, the star spectra specA, specB and the Rayleigh factor T_ray of the
 * ecology's bands (NULL when nb_eco == 0); phyto_tab [6][nb_phyto]: wr, wg, wb, specA, specB, T_ray of the phytoplankton's bands.
 * phyto_bands: NULL = the resident band stack of the daily phytoplankton step (the overlay is skipped until its first step has
 * run, as the reference skips it while alpha_water_bands is None); else a host [nb_phyto][n_lat][n_lon] stack, kept in a buffer of
 * the renderer's.  lake_mask: host [n_lat][n_lon] uint8 or NULL.  Refused on latitude bands. */
int qd_truecolor_configure(qd_handle h, const qd_truecolor_params* p, size_t sizeof_params, const double* eco_tab,
                           const double* phyto_tab, const double* phyto_bands, const uint8_t* lake_mask);
/* One frame from the state as it stands.  flow: NULL = the routing state's flow map; else a host [n_lat][n_lon] map (kg/s).
 * want_f64 != 0 also keeps the unquantised rgb.  out2 (may be NULL) = {sea_ice_area, mean_h_ice}: sum(w mask) / (sum(w) + 1e-15)
 * with w = max(cos lat, 0), and the mean of h_ice over the sea-ice mask (0 for an empty mask), from per-workgroup partials combined
 * in a fixed order.  Reads the state and changes none of it. */
int qd_truecolor_render(qd_handle h, int want_f64, const double* flow, double* out2);
/* which 0: the u8 image [n_lat][n_lon][3], northernmost row first, min(255, floor(x * 255 + 0.5)), NaN -> 0 (n = bytes);
 * which 1: the f64 rgb [n_lat][n_lon][3] in grid order of a render with want_f64 (n = doubles) */
int qd_truecolor_download(qd_handle h, int which, void* host, size_t n);

/* ---- 15-panel state frame (scripts/run_simulation.py:330-537, plot_state), whole-globe handles ----------------------------
 * A frame is a mosaic of 5 rows x 3 columns of tiles in the reference's panel order, each tile n_lat x n_lon pixels (one per cell,
 * northernmost row on top), with a white gutter of QD_STATEFRAME_GUTTER pixels between the tiles and around the mosaic:
 * width 3 n_lon + 4 gutters, height 5 n_lat + 6 gutters.  A tile is the reference's contourf sampled at the cell centres: a cell
 * takes the colour of the band i with levels[i] <= z < levels[i + 1]; the last band is closed above; a non-finite z or a z outside
 * every band is white; with extend_max a z above the top level takes the colour with the index n_levels - 1.  The fields are f64 in
 * the reference's operation order (:345-498); panels 7 and 8 fill the speed the reference colours its streamlines with. */
#define QD_STATEFRAME_PANELS 15
#define QD_STATEFRAME_MAX_LEVELS 32
#define QD_STATEFRAME_GUTTER 4
#define QD_STATEFRAME_SCAN_N 28
typedef struct qd_stateframe_params {
    int32_t ps_abs;                   /* QD_PLOT_PS_MODE == "abs" (:373-379) */
    int32_t ocean;                    /* an ocean exists: panel 4 is SST, panel 8 the current speed; else T_s and h - H (:348, :418-427) */
    int32_t rivers;                   /* routing exists and QD_PLOT_RIVERS == 1 (:513) */
    int32_t lakes;                    /* routing exists and its lake mask has a set cell (:525-526) */
    double p0, rho_a;                 /* the humidity parameters of the model (:368-369) */
    double H;                         /* the model's mean depth (:425) */
    double river_min, river_alpha, lake_alpha;   /* QD_RIVER_MIN_KGPS, QD_RIVER_ALPHA, QD_LAKE_ALPHA (:517-527) */
} qd_stateframe_params;
typedef struct qd_stateframe_panel {
    int32_t n_levels;                 /* 2..QD_STATEFRAME_MAX_LEVELS; ignored when constant */
    int32_t extend_max;               /* contourf(extend="max"), panel 5 (:396) */
    int32_t constant;                 /* no usable range: the tile stays white apart from its overlays */
    int32_t coast;                    /* 0 none (panel 10), 1 black, 2 white (panel 12) (:356 ... :500) */
    double levels[QD_STATEFRAME_MAX_LEVELS];
    double rgb[QD_STATEFRAME_MAX_LEVELS][3];    /* colour of band i; [n_levels - 1] the extended band */
} qd_stateframe_panel;
typedef struct qd_stateframe_table {
    qd_stateframe_panel panel[QD_STATEFRAME_PANELS];
    int64_t mark_cell[2];             /* flat cells of the star A (cyan x) and star B (yellow +) marks of panel 10, -1 = none (:444-449) */
} qd_stateframe_table;
/* Allocates the u8 mosaic, the vorticity plane and the partials.  lake_mask: host [n_lat][n_lon] uint8 or NULL.  Refused on
 * latitude bands. */
int qd_stateframe_configure(qd_handle h, const qd_stateframe_params* p, size_t sizeof_params, const uint8_t* lake_mask);
/* One launch over the grid plus a one-workgroup finish (replaces the host reductions of :349-350, :433, :444-445 and contourf's
 * zmin / zmax): writes the vorticity plane (the arithmetic of qd_op_vorticity) and out[QD_STATEFRAME_SCAN_N]:
 *   [0..2] min, [3..5] max of nan_to_num(T_s - 273.15), T_a - 273.15, nan_to_num(SST - 273.15) -- T_a over its non-NaN cells, with
 *   [25] = 1 when T_a holds a NaN (np.min then gives NaN and np.nanmin skips the field);
 *   [6..14] min, [15..23] max over the FINITE values of the panels 3, 7, 8, 9, 10, 12, 13, 14, 15 (+inf / -inf when there is none);
 *   [24] nanmax |vort| (-inf when every cell is NaN); [26], [27] isr_A, isr_B at their np.argmax cells, which go to mark_cells[2]
 *   (a NaN beats every number, ties go to the lowest flat index).
 * min, max and this argmax do not depend on the order of combination: the results are exact and repeatable. */
int qd_stateframe_scan(qd_handle h, double* out, int64_t* mark_cells);
/* One launch, one thread per (panel, cell), behind a memset of the mosaic to white (replaces the fifteen contourf calls, the coast
 * contours and the river / lake / star overlays of :355-530).  Needs a scan on this state (the vorticity plane): a render
 * after the handle's step counters have moved since the scan is refused.  The table is one constant-memory object per device; the
 * library serialises the renders of all handles on it.  flow: NULL = the
 * routing state's flow map; else a host [n_lat][n_lon] map (kg/s).  want_stacks != 0 also keeps the int8 band indices and the f64
 * fields.  Refuses a panel with more than QD_STATEFRAME_MAX_LEVELS levels.  Reads the state and changes none of it. */
int qd_stateframe_render(qd_handle h, const qd_stateframe_table* table, size_t sizeof_table, const double* flow, int want_stacks);
/* which 0: the u8 mosaic [5 n_lat + 24][3 n_lon + 16][3], min(255, floor(x * 255 + 0.5)) (n = bytes); which 1: the int8 band
 * indices [15][n_lat][n_lon] in grid order, -1 = white (n = bytes); which 2: the f64 fields [15][n_lat][n_lon] (n = doubles);
 * 1 and 2 only after a render with want_stacks (replaces plt.savefig, :535-536) */
int qd_stateframe_download(qd_handle h, int which, void* host, size_t n);

/* ---- tile renderer of the ecology, plankton and ISR figures (scripts/run_simulation.py:828-1060), whole-globe handles --------
 * A figure is one row of up to QD_TILES_MAX tiles with the state frame's geometry (one pixel per cell, northernmost row on top,
 * QD_STATEFRAME_GUTTER white pixels between and around): width n n_lon + (n + 1) gutters, height n_lat + 2 gutters.  A tile is
 * contourf sampled at the cell centres with the state frame's band, coast and u8 rules.  Every source plane equals the array the
 * reference hands to contourf bit for bit (no exp, log or pow is involved; stacks are reduced plane after plane, as NumPy does).
 * Every call reads the state and changes none of it. */
#define QD_TILES_MAX 8
#define QD_TILES_MAX_RANKS 4
typedef enum qd_tile_source {
    QD_TILE_LAI = 0,                  /* nan_to_num(QD_F_ECO_LAI) (:978) */
    QD_TILE_ALPHA = 1,                /* nan_to_num(QD_F_ECO_ALPHA) (:989) */
    QD_TILE_ALPHA_BANDED = 2,         /* nan_to_num(QD_F_ECO_ALPHA_BANDED) (:1000) */
    QD_TILE_CANOPY_HEIGHT = 3,        /* nan_to_num(canopy_height_map()) (:1009; pygcm/ecology/population.py:296-320, layered branch) */
    QD_TILE_SPECIES_DENSITY = 4,      /* nan_to_num(species_density_maps()[index]) (:1019; population.py:322-341, layered branch) */
    QD_TILE_PLANKTON = 5,             /* C_phyto_s[index], NaN where land_mask == 1 (:852-854), the resident tracer stack */
    QD_TILE_ISR_A = 6,                /* QD_F_ISR_A (:906) */
    QD_TILE_ISR_B = 7,                /* QD_F_ISR_B (:914) */
    QD_TILE_HOST_PLANE = 8            /* nan_to_num of the plane of qd_tiles_set_plane: the panel's banded-alpha fallback (:2458-2466) */
} qd_tile_source;
typedef struct qd_tile_ref { int32_t source, index; } qd_tile_ref;   /* index: the species of the sources 4 and 5, else 0 */
typedef struct qd_tile_desc {
    int32_t source, index;
    int32_t n_levels;                 /* 2..QD_STATEFRAME_MAX_LEVELS; ignored when constant or unavailable */
    int32_t extend_max;               /* contourf(extend="max") */
    int32_t constant;                 /* no usable range (contourf would raise): the tile stays white under its coast */
    int32_t unavailable;              /* the reference's "... not available" placeholder: white under its coast, the source is not read */
    int32_t coast;                    /* 0 none, 1 black, 2 white */
    int32_t mark_kind;                /* 0 none, 1 a cyan x (:928), 2 a yellow + (:929), at mark_cell */
    int64_t mark_cell;                /* flat cell, -1 = none */
    double levels[QD_STATEFRAME_MAX_LEVELS];
    double rgb[QD_STATEFRAME_MAX_LEVELS][3];
} qd_tile_desc;
/* height_scale: QD_ECO_HEIGHT_SCALE_M (population.py:302).  layers: NULL = the stack sources read the resident stack of
 * qd_eco_daily_configure; else a host [n_species][n_layers][n_lat][n_lon] stack, uploaded to a scratch buffer here (the convention
 * of qd_eco_diversity).  Allocates the select state.  Refused on latitude bands. */
int qd_tiles_configure(qd_handle h, double height_scale, const double* layers, int n_species, int n_layers);
/* plane: host [n_lat][n_lon], kept for QD_TILE_HOST_PLANE until the next qd_tiles_configure.  The reference computes its panel's
 * banded-alpha fallback into a local (:2464); this is the way to draw such a map without writing it into the resident state. */
int qd_tiles_set_plane(qd_handle h, const double* plane);
/* out3: is there an LAI map (eco.pop.LAI), a scalar alpha map (last_alpha_ecology_map, :1851) and a banded one
 * (last_alpha_banded, :1844) on the device? */
int qd_tiles_available(qd_handle h, int32_t* out3);
/* One launch over the grid plus a one-workgroup finish, for n <= QD_TILES_MAX planes (replaces contourf's zmin / zmax, np.max of
 * :903 and np.argmax of :924-925): out[k][4] = {min, max over the FINITE values (+inf / -inf when there is none), 1 when the plane
 * holds a NaN, the value at the np.argmax cell}, argmax_cell[k] that cell (a NaN beats every number, ties go to the lowest flat
 * index).  Total-order selections: exact, whatever the launch shape. */
int qd_tiles_scan(qd_handle h, const qd_tile_ref* refs, int n, double* out, int64_t* argmax_cell);
/* Exact order statistics of one plane (replaces the sort inside np.nanpercentile, :862): *count = the number of non-NaN cells;
 * values[k] = the ranks[k]-th smallest of them (0-based; +inf is a value, as in np.sort; either zero may stand for a zero), NaN for
 * a rank that is not below *count -- every rank of an empty plane.  A radix select on the order-preserving 64-bit key, 8 bits a
 * pass, all n_ranks <= QD_TILES_MAX_RANKS ranks narrowed in the same 8 passes. */
int qd_tiles_order_stats(qd_handle h, int source, int index, const int64_t* ranks, int n_ranks, double* values, int64_t* count);
/* One launch, one thread per (tile, cell), behind a memset of the mosaic to white (replaces the contourf and coast-contour calls of
 * :871-873, :906-929, :978-1021).  want_stacks != 0 also keeps the int8 band indices and the f64 planes.  Refuses n > QD_TILES_MAX,
 * more than QD_STATEFRAME_MAX_LEVELS levels, a species out of range and a stack source without a stack. */
int qd_tiles_render(qd_handle h, const qd_tile_desc* tiles, size_t sizeof_tile, int n, int want_stacks);
/* which 0: the u8 mosaic [n_lat + 8][n n_lon + 4 (n + 1)][3] (n = bytes); which 1: the int8 band indices [n][n_lat][n_lon], -1 =
 * white (n = bytes); which 2: the f64 planes [n][n_lat][n_lon], NaN for an unavailable tile (n = doubles); 1 and 2 only after a
 * render with want_stacks (replaces plt.savefig, :880, :950, :1059) */
int qd_tiles_download(qd_handle h, int which, void* host, size_t n);

/* ---- river routing (P014, pygcm/routing.py), whole-globe handles ----------------------------------
 * The host plans the network once (qingdai_amd/routing.py: build_plan): per cell a target code (>= 0 a live edge to that
 * cell; -1 ocean, -2 void, -3 residual, -4 never processed, -5 - k lake storage k) and the reference's sequential loop cut into
 * segments ordered by junction level.  The buffer accumulates RUNOFF every step; an event routes it with at most seven launches,
 * fills the flow map and appends one record of QD_ROUTE_LOG_W = 8 doubles to a device event log:
 * {step, event_dt, ocean_inflow_kgps, mass_closure_error_kg, mass_input_kg, ocean_kg, residual_kg, lake_delta_kg}. */
#define QD_ROUTE_LOG_W 8
typedef struct qd_route_plan {
    int32_t n_cells;                    /* n_lat * n_lon */
    int32_t n_seg, n_seg_cells, n_levels, n_jp, n_lakes;
    int32_t pe_lakes;                   /* 1: the lake P - E update runs on events that come with P and E */
    int32_t reserved;
    const uint8_t* cflags;              /* [n_cells] bit0 network land, bit1 lake cell of the P - E update */
    const double* area_row;             /* [n_lat] cell area per row (m^2) */
    const int32_t* code;                /* [n_cells] */
    const int32_t* seg_start;           /* [n_seg + 1] into seg_cells */
    const int32_t* seg_cells;           /* [n_seg_cells] head first */
    const int32_t* level_start;         /* [n_levels + 1] into the segments */
    const int32_t* jp_start;            /* [n_seg + 1] into jp_cells */
    const int32_t* jp_cells;            /* [n_jp] live predecessors of each head, in flow_order position */
    const int32_t* lake_start;          /* [n_lakes + 1] into lake_cells */
    const int32_t* lake_cells;          /* cells that drain into each lake storage, in flow_order position */
    const double* lake_frac;            /* [n_lakes] lake-area fraction of the P - E update */
} qd_route_plan;
int qd_route_configure(qd_handle h, const qd_route_plan* plan, size_t plan_bytes);   /* uploads the plan; zeroes the state */
int qd_route_free(qd_handle h);
int qd_route_reset(qd_handle h);                             /* buffer, flow map, lake volumes, log and step count to zero */
int qd_route_accumulate(qd_handle h, double dt);             /* buffer += where(land, (RUNOFF * area) * dt, 0) */
int qd_route_event(qd_handle h, double event_dt, int with_pe);   /* route the buffer (P, E: the PRECIP / EFLUX fields) */
int qd_route_schedule(qd_handle h, int n, const double* event_dt);   /* the next qd_step_n span: event_dt per step, 0 = none */
int qd_route_download(qd_handle h, int which, double* host, size_t n);   /* 0 flow map kg/s [n_cells], 1 lake volumes [n_lakes], 2 buffer */
int qd_route_events(qd_handle h, double* out, int max, int* n);   /* drains the event log: *n records of 8 doubles */
/* the inverse of qd_route_download, for an exact resume (QD_CHECKPOINT; the reference's restart does not carry the buffer): buffer
 * and flow map [n_cells], lake volumes [n_lakes] (null without lakes), the accumulations so far; log and schedule are left alone */
int qd_route_restore(qd_handle h, const double* buffer, const double* flow, const double* lakes, int64_t steps);

/* ---- river network generation (P014, scripts/generate_hydrology_maps.py:64-311), whole-globe handles ------------------
 * pit_fill(elevation, land_mask, max_iters, eps), compute_flow_to_index, identify_lakes, compute_lake_outlets and
 * topo_sort_flow_order on the handle's stream, every output bit-identical to the reference's.  land_mask and elevation are
 * [n_lat][n_lon] (the handle's grid); the host tables are the reference's spherical_distance operands: lat_rad [n_lat] and
 * lon_rad [n_lon] (np.deg2rad of the grid's axes) and cos_pair [n_lat][3] = cos(0.5 (lat_rad[j] + lat_rad[j + dj])) for
 * dj = -1, 0, 1 (unused entries at the poles are ignored); radius is PLANET_RADIUS.  Outputs: elevation_filled [n_lat][n_lon],
 * flow_to_index [n_lat][n_lon] (-1: ocean, sink), flow_order [*n_land], lake_mask, lake_id [n_lat][n_lon] and
 * lake_outlet_index [*n_lakes] (room for lake_outlet_cap).  Refused (nonzero): a shape that is not the handle's, n_lat < 2 or
 * n_lon < 3, land_mask values other than 0 / 1, and non-finite elevation on a land cell or a neighbour of one (NaN comparisons
 * make the reference depend on its visiting order). */
int qd_hydronet_build(qd_handle h, int n_lat, int n_lon, const uint8_t* land_mask, const double* elevation, double eps, int max_iters,
                      const double* lat_rad, const double* lon_rad, const double* cos_pair, double radius,
                      double* elevation_filled, int32_t* flow_to_index, int32_t* flow_order, uint8_t* lake_mask, int32_t* lake_id,
                      int32_t* lake_outlet_index, int lake_outlet_cap, int* n_land, int* n_lakes);
int qd_hydronet_sweeps(qd_handle h, int* sweeps);   /* pit-fill sweeps the last qd_hydronet_build on this handle ran */

/* ---- procedural topography (P004, pygcm/topography.py:58-83, 90-276), whole-globe handles ---------------------------------
 * The elevation recipe of generate_elevation_map and the sea level of create_land_sea_mask_from_elevation on the handle's
 * stream, all f64.  The random draws stay on the host (NumPy's default_rng stream); the host also makes the Gaussian weights.
 *
 * qd_topogen_smooth: gaussian_filter(field, sigma, mode=("nearest", "wrap")) (:164, :194, :245) as two separable passes, axis 0
 * clamped, then axis 1 periodic.  w_lat [r_lat + 1] and w_lon [r_lon + 1] are the first half of the normalised kernel, centre
 * last (w[r] is the centre weight; r = int(4 sigma + 0.5), r = 0 is the identity); a radius may exceed its axis.  The sum runs
 * centre first, then the pairs (F[i-k] + F[i+k]) * w[r-k] from k = r down to 1: bit-identical to scipy's correlate1d.
 * lds_bytes: the LDS a workgroup may use for a staged row / column strip (0: 64 KiB); a line that does not fit is read from
 * global memory instead (same sums).
 *
 * qd_topogen_build: the whole recipe.  par[QD_TOPOGEN_NPAR] = {sigma_rad, shape_p, 1 - W_VLF, W_VLF, W1, W3, SCALE_M,
 * target_land_frac}; oct_amp [n_oct] = 2 ** (-H k) as the reference accumulates it; noise [(1 + n_oct)][n_lat][n_lon]: the VLF
 * field, then the octaves (:162, :193); cont [n_cont][3] = {sin lat0, cos lat0, A} and cont_coslon [n_cont][n_lon] =
 * cos(lon - lon0) (:42-48); sin_lat, cos_lat, area_w [n_lat] (area_w = max(cos lat, 0), :262-264); radii [2 (n_oct + 2)] =
 * (r_lat, r_lon) of the VLF filter, the octaves' and the final 0.5-sigma one, and weights: their half kernels one after the
 * other in that order (lat, then lon, r + 1 entries each).  Every (x - mean) / (std + 1e-8) (:157-170, :195-202, :240) is two
 * passes (mean, then centred squares) with the block reduction of qd_blockred.h.  The sea level (_weighted_quantile, :58-83) is
 * a weighted MSB-first radix select over the f64 bit patterns with fixed-point row weights: one of the field's own values.
 * Outputs: elevation [n_lat][n_lon], land_mask (u8, elevation >= sea level), *sea_level_m.
 * Refused (nonzero): a band handle, a shape that is not the handle's, n_oct > QD_TOPOGEN_MAX_OCTAVES, n_cont >
 * QD_TOPOGEN_MAX_CONTINENTS, a radius > QD_TOPOGEN_MAX_RADIUS, non-finite noise, tables, weights or parameters, and an
 * elevation that comes out non-finite. */
#define QD_TOPOGEN_NPAR 8
#define QD_TOPOGEN_MAX_OCTAVES 16
#define QD_TOPOGEN_MAX_CONTINENTS 64
#define QD_TOPOGEN_MAX_RADIUS 65536
int qd_topogen_smooth(qd_handle h, int n_lat, int n_lon, const double* field, const double* w_lat, int r_lat, const double* w_lon,
                      int r_lon, int lds_bytes, double* out);
int qd_topogen_build(qd_handle h, int n_lat, int n_lon, const double* par, int n_oct, const double* oct_amp, const double* noise,
                     int n_cont, const double* cont, const double* cont_coslon, const double* sin_lat, const double* cos_lat,
                     const double* area_w, const int32_t* radii, const double* weights, double* elevation, uint8_t* land_mask,
                     double* sea_level_m);
int qd_topogen_last_ms(qd_handle h, double* ms);   /* event time of the kernels of the last qd_topogen_build on this handle */

/* ---- periodic budget diagnostics (QD_BUDGET_DIAG), whole-globe handles --------------------------------------------------
 * The reference driver prints [EnergyDiag], [OceanDiag], [HumidityDiag], [WaterDiag] and [HydroRoutingDiag] on steps i % 200 == 0
 * (run_simulation.py:2148-2188, 2263-2287, 2349-2398) and its ocean prints [OceanE] on its own step count (pygcm/ocean.py:446-516).
 * Here they are a span lane without a flag bit: a schedule given before a qd_step_n span turns it on for that span.  On a
 * scheduled step qd_step_n reduces on the device at the reference's positions in the step and leaves ONE record of
 * QD_BUDGET_LOG_W doubles; a step that is not scheduled launches nothing extra.  The record holds fixed-order SUMS and extrema
 * (w = max(cos lat, 0)); dividing by the weight sums and formatting is the host's (qingdai_amd/budget_diag.py):
 *    0.. 4  [EnergyDiag]   sum w TOA_net, sum w SFC_net, sum w ATM_net (energy.py:515-525), sum and count of the non-NaN T_s
 *    5..12  [OceanE]       sum w eff_Q, sum w dT ocean, sum w ocean, the same three over the polar ocean, its cell count,
 *                          1 when an earlier firing had left an SST snapshot (else the dT sums are 0)
 *   13..16  [OceanDiag]    sum w KE, max speed, eta min, eta max (ocean.py:539-545)
 *   17..20  [HumidityDiag] sum w of E, P_cond, LH, LH_release
 *   21..27  [WaterDiag]    sum w of E, precip, runoff, rho_a h_mbl q, rho_i h_ice, W_land, S_snow (hydrology.py:304-321)
 *   28..30  [HydroRoutingDiag] np.nanmax of the flow map, the last event's ocean inflow (kg/s) and mass closure error (kg)
 *   32..36  1 when the position ran (energy, ocean energy, ocean, humidity, water)     37  the step's schedule value
 * Lines that need the ocean step, the hydrology commit or routing run only in spans whose flags bring them. */
enum { QD_BD_LINE_ENERGY = 1, QD_BD_LINE_OCEAN = 2, QD_BD_LINE_OCEAN_ENERGY = 4, QD_BD_LINE_HUMIDITY = 8, QD_BD_LINE_WATER = 16 };
#define QD_BUDGET_LOG_W 40
/* lines: mask of QD_BD_LINE_*; polar_row[n_lat]: 1 where the reference's |lat| >= QD_OCEAN_POLAR_LAT test holds (ocean.py:488-489).
 * Allocates the log, the row partials and one SST snapshot; forgets an earlier configuration. */
int qd_budget_diag_configure(qd_handle h, int lines, const uint8_t* polar_row);
/* the next qd_step_n span: per step 0 = nothing, bit0 = the driver's cadence (run_simulation.py:2150 `i % 200 == 0`), bit1 = the
 * ocean's (ocean.py:452 `self._step % every == 0`) */
int qd_budget_diag_schedule(qd_handle h, int n, const int32_t* fire);
int qd_budget_diag_log(qd_handle h, double* out, int max, int* n);   /* drains the log: *n records of QD_BUDGET_LOG_W doubles */
int qd_budget_diag_reset(qd_handle h);                                /* log, schedule and the SST snapshot (ocean.py:476-479) forgotten */

/* ---- time-mean history accumulators (QD_HISTORY), whole-globe handles ----------------------------------------------------
 * Nothing the reference has: its loop leaves snapshots, no time means.  A span lane without a flag bit and without a log, like the
 * budget diagnostics: a schedule given before a qd_step_n span turns it on for that span, and on every sampled step each entry's
 * value is added to its resident sum plane, sum = sum + x in f64, in step order (no compensation; a NaN sample makes the cell
 * NaN).  The value of a field for step s is what qd_download returns after a span that ends with step s: the entries that read
 * PRECIP are sampled in front of the ocean step, inside which the next step's precipitation block may already run, every other
 * entry behind the step's last launch -- at most two launches per sampled step, none on the others.  When an entry reads one of
 * the lazily stored diagnostics (P_RAIN, S_SNOW_NEXT, MELT, C_SNOW, GLACIER, ISR_A, ISR_B, EFLUX, LHREL, OLR) a sampled step stores
 * them.  The host divides the sums by the sample count (qingdai_amd/history.py). */
#define QD_HISTORY_MAX_ENTRIES 32
/* n entries: op[k] 0 = the f64 plane a[k]; 1 = sqrt(a*a + b*b) of the planes a[k], b[k], rounded as np.sqrt(u*u + v*v).  Allocates
 * [n][n_lat][n_lon] sums, zeroed, and zeroes the sample count; forgets an earlier configuration; n == 0 only releases.  Refused:
 * latitude bands, n > 32, an unknown op, a field id that is not an f64 plane (masks, maps the ecology keeps as f32), op 1 without
 * b, op 1 that pairs PRECIP with another field. */
int qd_history_configure(qd_handle h, int n, const int32_t* op, const int32_t* a, const int32_t* b);
int qd_history_schedule(qd_handle h, int steps, const int32_t* sample);   /* the next qd_step_n span: non-zero = the step is sampled */
int qd_history_sample(qd_handle h);                                      /* one sample of every entry now, outside a span (one launch) */
int qd_history_read(qd_handle h, double* sums, int64_t* count);          /* the sums [n][n_lat][n_lon] and the samples in them */
int qd_history_reset(qd_handle h);                                       /* sums and count back to zero */
/* the inverse of qd_history_read, for an exact resume (QD_CHECKPOINT): an open window's sums and sample count put back */
int qd_history_restore(qd_handle h, const double* sums, int64_t count);

/* ---- per-step time series and zonal means (QD_SERIES), whole-globe handles ------------------------------------------------
 * Nothing the reference has.  A span lane without a flag bit, like the history accumulators, and with a device log, like the budget
 * diagnostics: a schedule given before a qd_step_n span turns it on for that span, and on every sampled step each entry (an entry
 * is a history entry: op 0 = an f64 plane, 1 = sqrt(a*a + b*b)) is reduced on the device to
 *     mean, min, max, nan_count [, zonal[n_lat]]
 * with w_j = w_row[j] (the host's max(cos lat_j, 0)), S_j the sum of row j, zonal[j] = S_j / n_lon, mean = (sum_j w_j S_j) /
 * (n_lon sum_j w_j), min / max over the non-NaN cells (NaN when there is none), nan_count exact; a NaN cell makes its row's zonal
 * and the mean NaN.  The n entries' results in configure order are ONE record of n * (QD_SERIES_STATS + (zonal ? n_lat : 0))
 * doubles; the log holds QD_SERIES_LOG_CAP records between two drains.  The summation order is fixed (csrc/qd_series.hip,
 * qingdai_amd/series.py: reduce_reference): a record depends on the planes' values and the grid shape alone.  Entries that read
 * PRECIP are reduced in front of the ocean step, the others behind the step's last launch, as in the history lane: at most two
 * launches per sampled step, none on the others; a sampled step stores the lazily stored diagnostics when an entry reads one. */
#define QD_SERIES_MAX_ENTRIES 32                         /* entries of one configuration */
#define QD_SERIES_LOG_CAP 256                            /* records the series log holds between two drains */
#define QD_SERIES_STATS 4                                /* mean, min, max, nan_count in front of an entry's zonal means */
/* n entries as qd_history_configure takes them, zonal != 0: the records carry the zonal means, w_row[n_lat]: the row weights.
 * Allocates the log; forgets an earlier configuration; n == 0 only releases.  Refused as in qd_history_configure. */
int qd_series_configure(qd_handle h, int n, const int32_t* op, const int32_t* a, const int32_t* b, int zonal, const double* w_row); /* n == 0 releases */
int qd_series_schedule(qd_handle h, int steps, const int32_t* sample);  /* the next qd_step_n span: non-zero = the step is sampled */
int qd_series_sample(qd_handle h);                                   /* class seam: one record now, outside a span */
int qd_series_log(qd_handle h, double* out, int max, int* n);        /* drain: *n records of width doubles, oldest first */
int qd_series_reset(qd_handle h);                                    /* log and schedule forgotten */

/* ---- zonal wavenumber spectra (QD_SPECTRA), whole-globe handles ----------------------------------------------------------
 * Nothing the reference has built (its plan for the dissipation filters asks for them).  A span lane without a flag bit and with a
 * device log, like the series: a schedule given before a qd_step_n span turns it on for that span, and on every sampled step each
 * entry (a history entry: op 0 = an f64 plane, 1 = sqrt(a*a + b*b)) is transformed row by row: with n = n_lon,
 * X_j(k) = sum_i x[j][i] exp(-2 pi i ik / n) for k = 0 .. n / 2 (n_bins = n / 2 + 1),
 *     P_j(k) = c_k |X_j(k)|^2 / n^2      c_k = 1 for k = 0 and for k = n / 2 of an even n, else 2      (sum_k P_j(k) = mean_i x^2)
 *     P(k) = sum_j w_j P_j(k) / sum_j w_j                                with w_j = w_row[j] (the host's max(cos lat_j, 0)).
 * A row that holds a non-finite value is NaN in every bin, makes every bin of P NaN, and is counted.  The n entries' results in
 * configure order are ONE record of n * (n_bins + QD_SPECTRA_STATS) doubles -- per entry P(0 .. n / 2), then the count of non-finite
 * rows; the log holds QD_SPECTRA_LOG_CAP records between two drains.  With lat_resolved the P_j(k) are also added into resident sum
 * planes [n][n_lat][n_bins] (qd_spectra_sums_get / _set).  Rows of length 2^a 3^b 5^c take a mixed-radix FFT in LDS, every other
 * length a direct DFT (QD_SPECTRA_FORM=direct in the environment of the configure call: the direct form everywhere); the order of
 * every sum is fixed (csrc/qd_spectra.hip, qingdai_amd/spectra.py: combine_reference).  Entries that read PRECIP are sampled in
 * front of the ocean step, the others behind the step's last launch: two launches per sampling position, none on unsampled steps;
 * a sampled step stores the lazily stored diagnostics when an entry reads one. */
#define QD_SPECTRA_MAX_ENTRIES 32                        /* entries of one configuration */
#define QD_SPECTRA_LOG_CAP 256                           /* records the spectra log holds between two drains */
#define QD_SPECTRA_STATS 1                               /* the count of non-finite rows behind an entry's n_bins powers */
/* n entries as qd_history_configure takes them, lat_resolved != 0: the sum planes are kept, w_row[n_lat]: the row weights.
 * Allocates the log, the twiddle table and the planes; forgets an earlier configuration; n == 0 only releases.  Refused as in
 * qd_history_configure, and with one line when a row's working set does not fit the LDS a workgroup may take. */
int qd_spectra_configure(qd_handle h, int n, const int32_t* op, const int32_t* a, const int32_t* b, int lat_resolved, const double* w_row); /* n == 0 releases */
int qd_spectra_schedule(qd_handle h, int steps, const int32_t* sample); /* the next qd_step_n span: non-zero = the step is sampled */
int qd_spectra_sample(qd_handle h);                                  /* class seam: one record now, outside a span */
int qd_spectra_log(qd_handle h, double* out, int max, int* n);       /* drain: *n records of width doubles, oldest first */
int qd_spectra_sums_get(qd_handle h, double* sums, int64_t* count);  /* lat_resolved: the sums [n][n_lat][n_bins] and the samples in them */
int qd_spectra_sums_set(qd_handle h, const double* sums, int64_t count);   /* its inverse, for an exact resume (QD_CHECKPOINT) */
int qd_spectra_reset(qd_handle h);                                   /* log and schedule forgotten, sums and count zeroed */

/* ---- Lagrangian drifters (QD_DRIFTERS), whole-globe handles ----------------------------------------------------------------
 * Nothing the reference has.  Two populations of particles, `atm` on (U, V) and `ocn` on (UO, VO), resident on the device as f64
 * structures of arrays (r, c, status [, blocked]: row coordinate in [0, n_lat - 1], column coordinate in [0, n_lon - 1), 1 = dead,
 * rejected moves onto land).  A span lane without a flag bit whose state MOVES: a schedule given before a qd_step_n span turns the
 * lane on for that span, EVERY step of the span then advances every live particle by one midpoint step of the span's dt on the
 * planes as the step leaves them (behind the step's last launch: what qd_download returns after a span that ends there), and a
 * step whose schedule value is non-zero also leaves ONE record in the lane's log:
 *     [atm: r | c | status | sample 0 | ...][ocn: r | c | status | blocked | sample 0 | ...]     each block n_pop doubles
 * the samples being the bilinear values, at the particle's new position, of up to QD_DRIFT_MAX_SAMPLES f64 planes per population.
 * One launch per advanced step, with or without a record; none while the lane is not scheduled.  The step itself -- index space,
 * no transcendental on the device, fold at the poles, wrap at the seam, dead and blocked particles -- is stated at the top of
 * csrc/qd_drift.hip and restated bit for bit by qingdai_amd/drifters.py: advance_reference.  When a sampled plane is one of the
 * lazily stored diagnostics a recording step stores them.  A span with an ocn population needs the ocean step (bit0). */
#define QD_DRIFT_MAX 1048576                             /* particles of one population */
#define QD_DRIFT_MAX_SAMPLES 4                           /* sampled planes of one population */
#define QD_DRIFT_LOG_MIB 256                             /* the log holds as many records as fit into this many MiB ... */
#define QD_DRIFT_LOG_CAP_MAX 16                          /* ... at most this many and at least one */
/* n_pop particles at (r_pop[i], c_pop[i]), status 0, blocked 0; ns_pop sampled planes (field ids); sec_row[n_lat]: the metric table
 * 1 / max(cos lat_j, sin(dlat / 2)) of the zonal displacement.  *log_cap: the records the log holds between two drains,
 * max(1, min(QD_DRIFT_LOG_CAP_MAX, floor(QD_DRIFT_LOG_MIB MiB / record bytes))).  Forgets an earlier configuration; n_atm == 0 &&
 * n_ocn == 0 only releases.  Refused: latitude bands, a count below 0 or above QD_DRIFT_MAX, an initial coordinate that is
 * non-finite or outside its interval, more than QD_DRIFT_MAX_SAMPLES planes, a sampled field that is not an f64 plane, PRECIP as a
 * sampled plane (inside a span the hoisted precipitation block has overwritten it with the next step's before the lane reads). */
int qd_drift_configure(qd_handle h, int n_atm, const double* r_atm, const double* c_atm, int n_ocn, const double* r_ocn,
                       const double* c_ocn, int ns_atm, const int32_t* planes_atm, int ns_ocn, const int32_t* planes_ocn,
                       const double* sec_row, int* log_cap);
int qd_drift_schedule(qd_handle h, int steps, const int32_t* record);  /* the next qd_step_n span advances; non-zero = the step records */
int qd_drift_advance(qd_handle h, double dt, int record);            /* class seam: one step now, outside a span (one launch) */
int qd_drift_log(qd_handle h, double* out, int max, int* n);         /* drain: *n records of width doubles, oldest first */
/* the particle state, for an exact resume: atm [3][n_atm] = r | c | status, ocn [4][n_ocn] = r | c | status | blocked; set refuses
 * what configure refuses of a position, a status that is neither 0 nor 1 and a blocked count that is negative or non-finite */
int qd_drift_state_get(qd_handle h, double* atm, double* ocn);
int qd_drift_state_set(qd_handle h, const double* atm, const double* ocn);
int qd_drift_reset(qd_handle h);                                     /* log and schedule forgotten; the particles stay */

/* ---- streamfunction and velocity potential (QD_FLOW), whole-globe handles ------------------------------------------------
 * Nothing the reference has (it defines vorticity and divergence and stops there).  A span lane without a flag bit and with a
 * device log, like the spectra: on every sampled step the resident (U, V) give
 *     zeta, delta   SphericalGrid.vorticity / .divergence on the rows 1 .. n_lat - 2, bit for bit; on the two pole rows the
 *                   circulation and the outflow of the polar cap of radius dlat / 2, constant along the row
 *     psi, chi      the solutions of L psi = zeta - mean(zeta), L chi = delta - mean(delta) with the finite-volume Laplacian L
 *                   stated in qingdai_amd/flow.py (helmholtz_reference, the definition), both of weighted mean zero: a row FFT,
 *                   one tridiagonal solve in latitude per zonal wavenumber (two prefix sums for wavenumber 0), an inverse row FFT
 * and ONE record of QD_FLOW_REC_W doubles (enum qd_flow_rec) in the lane's log, which holds QD_FLOW_LOG_CAP records between two
 * drains; psi, chi, zeta, delta are added into four resident sum planes [4][n_lat][n_lon] (qd_flow_sums_get / _set).  A
 * non-finite value anywhere in U or V makes psi and chi NaN in every cell, and the rows that hold one are counted.  Row lengths
 * 2^a 3^b 5^c take the FFT form, every other length the direct form (QD_FLOW_FORM=direct in the environment of the configure
 * call: the direct form everywhere).  Six launches on a sampled step, behind the step's last launch; none on any other step. */
#define QD_FLOW_LOG_CAP 256                              /* records the flow log holds between two drains */
#define QD_FLOW_TAB 6                                    /* rows of the grid table: flow.py: grid_tables */
#define QD_FLOW_PLANES 4                                 /* the sum planes: psi, chi, zeta, delta */
enum qd_flow_rec {
    QD_FLOW_ZETA_MEAN = 0, QD_FLOW_DIV_MEAN, QD_FLOW_ZETA_RMS, QD_FLOW_DIV_RMS, QD_FLOW_ZETA_MAXABS, QD_FLOW_DIV_MAXABS,
    QD_FLOW_PSI_MIN, QD_FLOW_PSI_MAX, QD_FLOW_CHI_MIN, QD_FLOW_CHI_MAX, QD_FLOW_KE, QD_FLOW_KE_ROT, QD_FLOW_KE_DIV, QD_FLOW_BAD,
    QD_FLOW_REC_W
};
/* tab [QD_FLOW_TAB][n_lat], lam [n_lon / 2 + 1], geom [3] = {a, dlat, dlon}: the grid quantities of the discrete system as
 * flow.grid_tables forms them (the host is their one source).  Allocates the log, the twiddle table, the work and the sum planes;
 * forgets an earlier configuration; tab == NULL only releases.  Refused: latitude bands, a row whose working set does not fit the
 * LDS a workgroup may take. */
int qd_flow_configure(qd_handle h, const double* tab, const double* lam, const double* geom);
int qd_flow_schedule(qd_handle h, int steps, const int32_t* sample);   /* the next qd_step_n span: non-zero = the step is sampled */
int qd_flow_sample(qd_handle h);                                     /* class seam: one record now from the resident U, V, outside a span */
int qd_flow_log(qd_handle h, double* out, int max, int* n);          /* drain: *n records of QD_FLOW_REC_W doubles, oldest first */
int qd_flow_sums_get(qd_handle h, double* sums, int64_t* count);     /* the sums [QD_FLOW_PLANES][n_lat][n_lon] and the samples in them */
int qd_flow_sums_set(qd_handle h, const double* sums, int64_t count);   /* its inverse, for an exact resume (QD_CHECKPOINT) */
int qd_flow_reset(qd_handle h);                                      /* log and schedule forgotten, sums and count zeroed */
/* class seam on host planes [n_lat][n_lon], outside a span: the kernels of a sample on (u, v) instead of the resident winds; the
 * record goes to the log, the sums and their count stay as they are */
int qd_flow_solve(qd_handle h, const double* u, const double* v, double* zeta, double* delta, double* psi, double* chi);
/* the same kernels without a handle, on a grid of any n_lat >= 3, n_lon >= 4 (qd_create needs five rows): rec [QD_FLOW_REC_W] */
int qd_flow_solve_grid(int n_lat, int n_lon, int device, const double* tab, const double* lam, const double* geom, const double* u,
                       const double* v, double* zeta, double* delta, double* psi, double* chi, double* rec);

/* ---- spherical-harmonic power spectra (QD_SPHARM), whole-globe handles ----------------------------------------------------
 * Nothing the reference has.  A span lane without a flag bit and with a device log, like the spectra: on every sampled step each
 * entry's plane is analysed into spherical-harmonic coefficients x_n^m, 0 <= m <= n <= N, N the triangular truncation
 * min((n_lat - 1) / 2, (n_lon - 1) / 2), as qingdai_amd/spharm.py defines them (analyse_reference): a row transform (the row FFT
 * of the spectra and flow lanes for n_lon = 2^a 3^b 5^c, direct sums otherwise or under QD_SPHARM_FORM=direct in the environment
 * of the configure call), then per (entry, m) the Legendre recurrence in n fused with the Clenshaw-Curtis quadrature over the
 * latitude rows, all f64 and in a fixed order.  An entry is a history entry (op 0: the f64 plane a; op 1: sqrt(a*a + b*b)) or one
 * of this lane's own: QD_SPHARM_OP_VORT / _DIV, the flow lane's relative vorticity and divergence of the resident (U, V), produced
 * by the flow lane's kernel (qd_flow_configure is not needed).  The entries' results, in configure order, are ONE record of
 * n * (N + 1 + QD_SPHARM_STATS) doubles -- per entry P(0 .. N), P(n) = sum_m c_m |x_n^m|^2, then the mean square (1/2) sum_j w_j
 * mean_i x^2 and the count of rows that hold a non-finite value (one of those makes every coefficient and every bin of the entry
 * NaN) -- in the lane's log, which holds QD_SPHARM_LOG_CAP records between two drains.  With two_d the terms c_m |x_n^m|^2 are also
 * added into resident sum planes [entry][N + 1 (n)][N + 1 (m)] (qd_spharm_sums_get / _set).  Sampling places are history's: the
 * entries that read PRECIP in front of the ocean step, every other entry behind the step's last launch. */
#define QD_SPHARM_LOG_CAP 256                            /* records the lane's log holds between two drains */
#define QD_SPHARM_MAX_ENTRIES 32                         /* entries of one configuration */
#define QD_SPHARM_STATS 2                                /* the mean square and the bad-row count behind an entry's N + 1 powers */
#define QD_SPHARM_OP_VORT 2                              /* entry ops beside history's 0 and 1 */
#define QD_SPHARM_OP_DIV 3
#define QD_SPHARM_MAX_LAT 1535                           /* rows the Legendre kernel's widest form takes (12 latitude pairs per lane) */
/* n entries (op, a, b as qd_history_configure takes them; a and b are ignored for QD_SPHARM_OP_VORT / _DIV), trunc = N, and the
 * host's tables as spharm.tables forms them (the host is their one source): w, mu [n_lat], seed [N + 1][(n_lat + 1) / 2] =
 * Pbar_m^m(mu_j) on the rows of the southern half, A, B [N + 1][N + 1] indexed [m][n]; flow_tab [QD_FLOW_TAB][n_lat] and flow_geom
 * [3] as qd_flow_configure takes them, needed when an entry is VORT or DIV.  Allocates the log, the work planes and, with two_d,
 * the sum planes; forgets an earlier configuration; n == 0 or w == NULL only releases.  Refused: latitude bands, N < 1 or not the
 * grid's truncation, more than QD_SPHARM_MAX_LAT rows, a row whose working set does not fit the LDS a workgroup may take. */
int qd_spharm_configure(qd_handle h, int n, const int32_t* op, const int32_t* a, const int32_t* b, int two_d, int trunc, const double* w,
                        const double* mu, const double* seed, const double* A, const double* B, const double* flow_tab,
                        const double* flow_geom);
int qd_spharm_schedule(qd_handle h, int steps, const int32_t* sample);   /* the next qd_step_n span: non-zero = the step is sampled */
int qd_spharm_sample(qd_handle h);                                   /* class seam: one record now from the resident fields, outside a span */
int qd_spharm_log(qd_handle h, double* out, int max, int* n);        /* drain: *n records, oldest first */
int qd_spharm_sums_get(qd_handle h, double* sums, int64_t* count);   /* the 2D sums [n][N + 1][N + 1] and the samples in them */
int qd_spharm_sums_set(qd_handle h, const double* sums, int64_t count);   /* its inverse, for an exact resume (QD_CHECKPOINT) */
int qd_spharm_reset(qd_handle h);                                    /* log and schedule forgotten, sums and count zeroed */
/* class seam on a host plane [n_lat][n_lon], outside a span: the kernels of one entry on the plane -> coef_re, coef_im
 * [N + 1 (m)][N + 1 (n)] (zero for n < m) and rec [N + 1 + QD_SPHARM_STATS]; the log, the sums and their count stay as they are */
int qd_spharm_analyse(qd_handle h, const double* plane, double* coef_re, double* coef_im, double* rec);
/* the same kernels without a handle, on any grid with N >= 1 (qd_create needs five rows) */
int qd_spharm_analyse_grid(int n_lat, int n_lon, int device, int trunc, const double* w, const double* mu, const double* seed,
                           const double* A, const double* B, const double* plane, double* coef_re, double* coef_im, double* rec);

/* ---- eddy statistics: time sums of products of two fields (QD_EDDY), whole-globe handles --------------------------------------
 * Nothing the reference has.  A span lane without a flag bit and without a log, like the history accumulators: a configuration names
 * F <= QD_EDDY_MAX_FIELDS distinct f64 planes and P <= QD_EDDY_MAX_PAIRS pairs (p, q) of indices into that list (p == q: a variance).
 * Resident: anchors r[F], first-moment sums S[F] and pair sums C[P], each [n_lat][n_lon] f64.  One sample, per cell, behind the
 * step's last launch (history's late group): the first sample of a window stores r_f = a_f; then d_f = a_f - r_f, S_f = S_f + d_f,
 * C_k = C_k + (d_p * d_q), every operation rounded on its own, no compensation, non-finite values as they come (the top of
 * qingdai_amd/csrc/qd_eddy.hip is the definition, eddy.accumulate_reference its restatement).  One launch per sample. */
#define QD_EDDY_MAX_FIELDS 16
#define QD_EDDY_MAX_PAIRS 32
#define QD_EDDY_ZONAL_SUMS 4                             /* row sums per pair of qd_eddy_zonal: S_p, S_q, C_k, S_p * S_q */
/* fields[n_fields]: qd_field ids; p, q [n_pairs]: indices into fields.  Allocates and zeroes the planes; forgets an earlier
 * configuration; n_fields == 0 only releases.  Refused, each with one line that begins "eddy:": latitude bands, more fields or pairs
 * than the limits or no pair, an unknown plane or one that is not f64, PRECIP (sampled in front of the ocean step, every other field
 * behind the step's last launch: a product across the two places has no meaning), a field named twice, a pair index out of range, a
 * pair named twice in either order. */
int qd_eddy_configure(qd_handle h, int n_fields, const int32_t* fields, int n_pairs, const int32_t* p, const int32_t* q);
int qd_eddy_schedule(qd_handle h, int steps, const int32_t* sample);     /* the next qd_step_n span: non-zero = the step is sampled */
int qd_eddy_sample(qd_handle h);                                        /* class seam: one sample now from the resident fields, outside a span */
/* anchors [F][n_lat][n_lon], sums [F][n_lat][n_lon], pair_sums [P][n_lat][n_lon] and the samples in them */
int qd_eddy_read(qd_handle h, double* anchors, double* sums, double* pair_sums, int64_t* count);
int qd_eddy_restore(qd_handle h, const double* anchors, const double* sums, const double* pair_sums, int64_t count);   /* its inverse (QD_CHECKPOINT) */
/* out [P][QD_EDDY_ZONAL_SUMS][n_lat]: per pair and row the sums over all n_lon columns of S_p, S_q, C_k and S_p * S_q (the product
 * rounded), one wavefront per (pair, row) in the order of the series lane's row stage */
int qd_eddy_zonal(qd_handle h, double* out);
int qd_eddy_reset(qd_handle h);                                         /* sums and count zeroed, schedule forgotten: the next sample is a window's first */

/* ---- extremes, spells and distributions (QD_EXTREMES), whole-globe handles -----------------------------------------------------
 * Nothing the reference has.  A span lane of history's kind (no flag bit, no log, early and late sampling places): a configuration
 * names E <= QD_EXTREMES_MAX_ENTRIES entries (op, a, b) as the history accumulators take them, T <= QD_EXTREMES_MAX_THRESHOLDS
 * thresholds (entry, cmp, value) and B <= QD_EXTREMES_MAX_HISTS binned entries, each with nb + 1 strictly increasing finite edges,
 * 1 <= nb <= QD_EXTREMES_MAX_BINS.  Resident, reset at a window's start; k is the 0-based index of the sample in its window:
 *   per entry and cell      vmax, vmin (f64, -inf / +inf), tmax, tmin (i32, -1), nan (i32, 0):
 *                           if (x > vmax) { vmax = x; tmax = k; }  if (x < vmin) { vmin = x; tmin = k; }  nan += (x != x)
 *   per threshold and cell  one 16-byte item {count, run, longest, spells} (u32, 0): hit = x cmp value (false for a NaN);
 *                           spells += hit && run == 0; run = hit ? run + 1 : 0; count += hit; longest = max(longest, run)
 *   per binned entry, row   hist[nb + 3] (i64, 0), columns [under, bin 0 .. bin nb - 1, over, nan]: a NaN to nan, x < e_0 to under,
 *                           x >= e_nb to over, anything else to the bin np.searchsorted(edges, x, side="right") - 1
 * Selections and integer counts only: the state does not depend on the launch geometry (the top of qingdai_amd/csrc/qd_extremes.hip
 * is the definition, extremes.accumulate_reference its restatement).  At most two launches on a sampled step, none otherwise. */
#define QD_EXTREMES_MAX_ENTRIES 16
#define QD_EXTREMES_MAX_THRESHOLDS 16
#define QD_EXTREMES_MAX_HISTS 8
#define QD_EXTREMES_MAX_BINS 256
#define QD_EXTREMES_CMP_LT 60                            /* '<' */
#define QD_EXTREMES_CMP_GT 62                            /* '>' */
/* op, a, b [n_entries]: as qd_history_configure; thr_entry, thr_cmp, thr_value [n_thresholds]: an index into the entries, one of
 * QD_EXTREMES_CMP_*, a finite value; hist_entry, hist_nb [n_hists]: an index into the entries and the bin count; edges: the
 * sum(nb + 1) edges of all tables, one behind the other.  Allocates the state at its start values; forgets an earlier configuration;
 * n_entries == 0 only releases.  Refused, each with one line that begins "extremes:": latitude bands, more entries, thresholds,
 * histograms or bins than the limits, what the entry table refuses, a threshold or histogram whose entry index is out of range, a cmp
 * that is neither, a non-finite threshold, fewer than 2 edges, edges that are not finite and strictly increasing. */
int qd_extremes_configure(qd_handle h, int n_entries, const int32_t* op, const int32_t* a, const int32_t* b, int n_thresholds,
                          const int32_t* thr_entry, const int32_t* thr_cmp, const double* thr_value, int n_hists,
                          const int32_t* hist_entry, const int32_t* hist_nb, const double* edges);
int qd_extremes_schedule(qd_handle h, int steps, const int32_t* sample);   /* the next qd_step_n span: non-zero = the step is sampled */
int qd_extremes_sample(qd_handle h);                                    /* class seam: one sample of every entry now, k = the lane's count */
/* values [2][E][n_lat][n_lon] (vmax, vmin); counts [3][E][n_lat][n_lon] (tmax, tmin, nan); thresholds [T][n_lat][n_lon][4] (count, run,
 * longest, spells; u32 carried as int32); hist: per binned entry [n_lat][nb + 3], one behind the other; and the samples in them */
int qd_extremes_read(qd_handle h, double* values, int32_t* counts, int32_t* thresholds, int64_t* hist, int64_t* count);
int qd_extremes_restore(qd_handle h, const double* values, const int32_t* counts, const int32_t* thresholds, const int64_t* hist,
                        int64_t count);                                   /* its inverse (QD_CHECKPOINT) */
int qd_extremes_reset(qd_handle h);                                     /* start values, count 0, schedule forgotten: the next sample is a window's first */

/* ---- state digest and exact resume (QD_CHECKPOINT), whole-globe handles ---------------------------------------------------
 * Nothing the reference has: its restart file holds 14 planes as f4 and a resumed run does not continue the run that was stopped.
 * qd_state_digest: a 64-bit digest of resident planes, all of them in ONE launch.  The digest of a plane of n elements is
 *     D = sum_{i = 0 .. n-1} mix64(w_i + (i + 1) * 0x9E3779B97F4A7C15)  mod 2^64
 * with w_i the element's stored bits zero-extended to 64 (f64 8 bytes, f32 4, u8 1; NaN payloads and the sign of zero count; a map
 * the ecology keeps as f32 is digested as the f32 slab it is), i the element's row-major index in the global plane, and mix64 the
 * splitmix64 finaliser (z ^= z >> 30; z *= 0xBF58476D1CE4E5B9; z ^= z >> 27; z *= 0x94D049BB133111EB; z ^= z >> 31).  Integer
 * addition is associative: the value does not depend on the launch shape or on the order in which the workgroups finish.
 * A ref is a qd_field id (every f64 field, QD_F_LAND_MASK, QD_F_ICE_MASK) or one of the resident planes that have no field id: */
enum qd_state_ref {
    QD_SR_PHYTO_TRACER = 200,      /* + s: the tracer of species s (< QD_STATE_REF_TRACERS), [n_lat][n_lon] */
    QD_SR_ROUTE_BUFFER = 300, QD_SR_ROUTE_FLOW = 301,   /* what qd_route keeps: the buffer and the flow map [n_lat][n_lon] ... */
    QD_SR_ROUTE_LAKES = 302,       /* ... and the lake volumes [n_lakes] */
    QD_SR_ECO_LAI_STACK = 310,     /* the LAI stack of the daily vegetation step, [n_species * n_layers][n_lat][n_lon] as ONE plane */
    QD_SR_INDIV_E_DAY = 320, QD_SR_INDIV_STRESS = 321,   /* the individuals' buffers [n_indiv] */
    QD_SR_HISTORY_SUM = 400        /* + k: the sum plane of history entry k (< QD_STATE_REF_HISTORY_SUMS) */
};
#define QD_STATE_REF_TRACERS 64                         /* index range of QD_SR_PHYTO_TRACER */
#define QD_STATE_REF_HISTORY_SUMS QD_HISTORY_MAX_ENTRIES   /* index range of QD_SR_HISTORY_SUM */
#define QD_STATE_REF_SPECTRA_SUMS 500                   /* one more ref: the lat-resolved sums of the spectra lane, [n][n_lat][n_bins] as ONE plane */
#define QD_STATE_REF_FLOW_SUMS 501                      /* and the sum planes of the flow lane, [QD_FLOW_PLANES][n_lat][n_lon] as ONE plane */
#define QD_STATE_REF_SPHARM_SUMS 502                    /* and the 2D sums of the spherical-harmonic lane, [n][N + 1][N + 1] as ONE plane */
#define QD_STATE_REF_EDDY_SUMS 503                      /* and the eddy lane's first-moment and pair sums, [F + P] planes of even stride as ONE plane */
#define QD_STATE_REF_EDDY_ANCHORS 504                   /* and its anchors, [F] planes of even stride as ONE plane */
#define QD_STATE_REF_EXTREMES_VALUES 505                /* and the extremes lane's vmax and vmin, [2][E] f64 planes as ONE plane */
#define QD_STATE_REF_EXTREMES_COUNTS 506                /* and every 4-byte plane of it, [T][cells][4] thresholds then [3][E] tmax / tmin / nan, as ONE plane */
#define QD_STATE_REF_EXTREMES_HIST 507                  /* and its histograms, the i64 tables one behind the other, as ONE plane */
#define QD_STATE_DIGEST_MAX 64
/* n <= 64 refs -> out[n].  Refused: latitude bands, an unknown ref, a ref whose subsystem is not configured (the line names it). */
int qd_state_digest(qd_handle h, int n, const int32_t* refs, uint64_t* out);
/* The host-side scalars a step reads besides the planes and the two step counters, as n = QD_STATE_SCALARS_N doubles in the slots
 * of enum qd_state_scalar; set puts them back on a fresh handle that was configured like the one they were read from. */
enum qd_state_scalar {
    QD_SS_CLOUD_EFF_VALID = 0,
    QD_SS_HAS_ELEVATION = 1,          /* read only: the elevation map is the run's own */
    QD_SS_ECO_HOURS = 2, QD_SS_ECO_NEXT_H = 3, QD_SS_ECO_COUNT = 4,   /* the ecology sub-step's clock */
    QD_SS_HAVE_LAI = 5, QD_SS_F_VALID = 6, QD_SS_ALPHA_VALID = 7, QD_SS_ALPHA_DIRTY = 8, QD_SS_BANDED_VALID = 9, QD_SS_WATER_VALID = 10,
    QD_SS_LAI_VERSION = 11, QD_SS_SNAP_VERSION = 12, QD_SS_N_RECOMPUTE = 13,
    QD_SS_INDIV_PERIOD = 14,          /* the individuals' sub-step period (-1: not begun) */
    QD_SS_INDIV_ACCUM = 15, QD_SS_INDIV_FIRED = 16,   /* its accumulator, its firings */
    QD_SS_PHYTO_DAILY_STEPS = 17, QD_SS_ECO_DAILY_FIRED = 18, QD_SS_INDIV_DAILY_FIRED = 19,   /* the counts of the daily lanes */
    QD_SS_LAST_NSUB = 20,
    QD_SS_LAST_DIAG = 21              /* .. 30: the energy-budget means of the last span that took them; 31 reserved (0) */
};
#define QD_STATE_SCALARS_N 32
int qd_state_scalars_get(qd_handle h, double* out, int n);
int qd_state_scalars_set(qd_handle h, const double* in, int n);

/* ---- reductions for diagnostics (energy.py:494-538, ocean.py:535-561) -------------- */
/* compute_energy_diagnostics (energy.py:494-538) from the resident state, with the flux formulas of the driver's
 * coupling block (run_simulation.py:2199-2239): out[10] = cos-weighted global means of
 * TOA_net, SFC_net, ATM_net, I, R, OLR, SW_sfc, LW_sfc, SH, LH. */
int qd_energy_diagnostics(qd_handle h, double out[10]);
/* the same ten means as taken INSIDE the last qd_step_n call that had flags bit4 set: on its first step, after time_step and
 * before the ocean step, i.e. exactly where run_simulation.py:2242-2246 evaluates them for the autotuner */
int qd_energy_diagnostics_last(qd_handle h, double out[10]);
enum qd_reduce_op { QD_R_SUM = 0, QD_R_COSWEIGHTED_MEAN = 1, QD_R_MAX = 2, QD_R_MIN = 3, QD_R_MAXABS = 4 };
/* NaN / inf: SUM and COSWEIGHTED_MEAN add them like any value (IEEE: NaN, or inf - inf = NaN, reaches the result); MAX, MIN and MAXABS compare (v > acc), so a NaN cell is skipped and +-inf counts as a value, from the identity -DBL_MAX (MIN: +DBL_MAX), which is what comes back when nothing beats it (every cell NaN; MAX of all -inf) */
int qd_reduce(qd_handle h, int field, int op, double* out);

/* ---- multi-GPU: latitude bands, RCCL halo exchange ------------------ */
int qd_comm_unique_id(void* id128, size_t bytes);                 /* rank 0: ncclGetUniqueId */
int qd_comm_init(qd_handle h, const void* id128, size_t bytes);   /* all ranks: ncclCommInitRank */
/* in-process group of band handles on ONE device, one host thread per handle: exercises the band
 * logic (margins, ring halos, reductions) without RCCL; handles[] ordered by rank */
int qd_comm_init_local(qd_handle* handles, int n);
int qd_comm_stats(qd_handle h, int* halo_exchanges);
int qd_comm_allreduce_count(qd_handle h, int* allreduces);        /* all-reduce collectives issued so far (statistics) */
/* of those, the eta sums of ocean sub-steps that went out INSIDE the ncclGroup of the following halo exchange instead of as a
 * collective launch of their own (round 3; WindDrivenSlabOcean.step removes the global mean of eta once per sub-step,
 * pygcm/ocean.py:369-377 -- the reference has no counterpart for the transport) */
int qd_comm_grouped_sum_count(qd_handle h, int* grouped);
/* host ring: the ranks of ONE node all-reduce the few host-visible scalars of a step (eta sum per ocean sub-step, CFL maxima)
 * through a POSIX shared-memory segment instead of an RCCL launch each; every rank passes the same `name` (unique per launch).
 * Optional: without it those scalars go through RCCL like everything else. */
int qd_comm_init_shm(qd_handle h, const char* name);
int qd_comm_host_allreduce_count(qd_handle h, int* n);
/* the ring by itself (no handle, no GPU): what tests/test_bands_cpu.py drives from several processes */
int qd_hostring_open(const char* name, int rank, int world, void** ring_out);
int qd_hostring_allreduce(void* ring, double* vals, int n, int op_max);   /* n <= 8; op_max 0 = sum in rank order, 1 = max */
int qd_hostring_close(void* ring);

/* Planner simulation (host only, no device is touched): the latitude-band planner of SURVEY.md 8(e) -- validity margins, launch
 * segments, the decision WHEN to exchange halos and WHICH rows move where -- on a handle that owns no memory.  Exchanges are
 * logged instead of performed; tests/test_bands_cpu.py performs them with torch.distributed (gloo) on NumPy slabs.
 * The reference has no counterpart (single process, np.roll on whole arrays: pygcm/ocean.py:306-310, dynamics.py:144-173). */
int qd_plansim_create(const qd_grid_desc* desc, qd_handle* out);
int qd_plansim_destroy(qd_handle h);
int qd_plansim_plan(qd_handle h, const int* fields, const int* radii, int n, int want);      /* -> margin of the outputs */
int qd_plansim_mark(qd_handle h, const int* fields, int n, int margin);
int qd_plansim_margin(qd_handle h, int field);
int qd_plansim_segments(qd_handle h, int margin, int* row0_nrows_pairs);                    /* -> number of segments (<= 3) */
int qd_plansim_pop_exchange(qd_handle h, int* fields_out, int max_fields, int* geom4);      /* geom4 = {H, owned rows, up, dn} */
int qd_plansim_segments_rows(qd_handle h, int vr0, int cnt, int* row0_nrows_pairs);          /* ring rows [vr0, vr0 + cnt) -> segments (<= 6) */
int qd_comm_barrier(qd_handle h);
/* Device-side exchange over the peer mapping (round 4; QD_PEER_EXCHANGE=1): halo rows and global sums are STORED into the
 * neighbours' memory by small kernels on the handle's own stream and polled there -- no collective launch, no host.  Every rank
 * exports the IPC handle of its mailbox (64 bytes), the host side hands every rank all handles in rank order, qd_peer_connect
 * maps them; from then on qd_comm_init is not needed.  In-process groups (qd_comm_init_local) switch to it through the environment
 * variable.  Replaces nothing in the reference (single process: np.roll on whole arrays, pygcm/ocean.py:306-310,369-377). */
int qd_peer_export(qd_handle h, void* handle64, size_t bytes);
int qd_peer_connect(qd_handle h, const void* handles, size_t bytes_each, int world);
int qd_comm_peer_stats(qd_handle h, int* halo_exchanges, int* reductions);   /* operations that went through the mailboxes */
int qd_comm_peer_carried(qd_handle h);   /* of those halo exchanges: pushes that went out INSIDE a compute launch (QD_PEER_OVERLAP=2); < 0: bad handle */
/* self-test of a freshly connected transport: `iters` ring exchanges of rows whose values encode (sender, iteration, position) and
 * all-reduces of rank-dependent numbers with known results; *wrong = values this rank found wrong (stale data would show here, not as
 * an error).  qd_peer_disable: leave the mailboxes (all ranks together, when any rank's self-test failed) -- the host then calls
 * qd_comm_init. */
int qd_peer_selftest(qd_handle h, int iters, long long* wrong);
int qd_peer_disable(qd_handle h);
int qd_comm_allreduce_max(qd_handle h, double* inout, int n);     /* bench timing: max over ranks */

/* ---- profiling hooks ----------------------------------------------------------------- */
/* mean device time (ms) of the kernels tagged `name` since the last reset, measured with
 * hipEvents on the handle's stream when timing is enabled. */
/* measured streaming ceiling of the device ("also report a measured device-copy ceiling"): a device-to-device copy of
 * `bytes` (choose > 256 MiB to get past the Infinity Cache), `reps` times; *gbs = (read + written bytes) / time. */
int qd_copy_ceiling(qd_handle h, size_t bytes, int reps, double* gbs);
/* Launcher tuning switches (QD_STREAM_R*, QD_TAIL_R / _RP / _V / _GENERAL, QD_MED_BLOCKS, QD_SHAPIRO_R, QD_TILE_TR: README.md) are
 * read from the environment once, in qd_create; the developer scripts that sweep one of them on a live handle call this to have
 * them read again.  Nothing the reference has (it re-reads its own QD_* variables every step: pygcm/dynamics.py:330-348). */
int qd_tune_reload(qd_handle h);
int qd_timing_enable(qd_handle h, int on);           /* 0 off, 1 every kernel group */
int qd_timing_select(qd_handle h, const char* name); /* time only the groups "name[:stride],..." (implies on); with a stride
                                                       * only every stride-th launch of the group is bracketed */
/* the operator seam's groups name the form that ran: k_shapiro_stream / k_shapiro_pass, k_gauss_rows1 / 2 / 4, k_gauss_fused, k_gauss_axis,
 * k_zonal_filter / k_scrub_field (one bracket per call of the form, however many launches it takes) */
int qd_timing_get(qd_handle h, const char* name, double* mean_ms, int64_t* launches);
int qd_timing_reset(qd_handle h);

#ifdef __cplusplus
}
#endif
#endif /* QINGDAI_HIP_H */
