// qd_phyto_daily.hip -- the daily phytoplankton step (P017) on the resident tracers, gfx950.
//
// PhytoManager.step_daily (pygcm/ecology/phyto.py:339-435), called by the reference driver once per planet-day after the step's
// insolation (scripts/run_simulation.py:2051-2061), per cell:
//     I_b    = dual_star_insolation_to_bands(insA, insB)                                   spectral.py:397-426
//     Kd_b   = clip(Kd0_b + kchl_b max(C_tot, 0)^m, 1e-6, inf)                              phyto.py:285-299
//     Ibar_b = clip(I_b (1 - e^-x) / x, 0, inf), x = Kd_b H (series below 1e-6)             phyto.py:301-315
//     E_s    = sum_b shape_sb Ibar_b dlam_b;  muL_s = tanh(alpha_P E_s / max(mu_max_s, 1e-6)) phyto.py:361-375
//     mu_grow_s = mu_max_s muL_s Q10^((T_w - T_ref)/10) [clip(N / (KN_s + N), 0, 1)]        phyto.py:376-392
//     C_s    = clip(C_s + (mu_grow_s - m0_s - sink) C_s dt, 0, inf), land 0                 phyto.py:394-400
//     N      = clip(N + (R - sum_s mu_grow_s C_s_new / Y_s) dt, 0, inf), land 0             phyto.py:402-411
//     A_b    = clip(Apure_b + sum_s c_s shape_sb max(C_s, 0)^p_s, lo, hi); alpha = clip(sum_b A_b w_b, lo, hi)   phyto.py:317-337,413-419
// One thread per cell, one launch per day.  The step's two-star insolation is evaluated in registers from the star row with the
// forcing kernels' own arithmetic (qd_star_insolation): the ISR_A / ISR_B of the step are not stored yet when this runs at the top
// of a qd_step_n step.  The band loops are unrolled over a register array of 16 (or 32) bands and guarded by n_bands; species are
// a runtime loop (their planes are read twice: once for C_tot, once for the update).  The per-block cos-weighted partial sums of
// the [PhytoDiag] line are finished by one workgroup into a device log the host drains after the span.
#include "qd_span.h"
#include "qd_pointwise.h"
#include "qd_blockred.h"
#include <algorithm>

struct QdPhytoDaily {
    qd_phyto_daily_params p{};
    double* tab = nullptr;            // band_tab [8][NB] | species_tab [6][S] | shape [S][NB]
    double* bands = nullptr;          // [NB][cells] alpha_water_bands
    int nb_alloc = 0;
    QdPartials partial;               // [3][nblk]
    int64_t n_steps = 0;
    QdSpanLane lane;                  // qd_phyto_daily_schedule: 1 per firing step of the next span; the [PhytoDiag] log
};

struct QdPDArgs {
    QdGeom G; QdTabs T; QdStar A, B; double theta;
    qd_phyto_daily_params p;
    const double* tab;
    double* C; size_t stride;
    double* N; const double* Tw; const uint8_t* land;
    double* kd490; double* walpha; double* bands; size_t plane;
    double* partial;
};

// x^p for x >= 0 (or NaN): sqrt when p == 0.5, the default of both exponents -- correctly rounded, like the C library's pow that
// NumPy calls, and several times cheaper than a general f64 pow
__device__ __forceinline__ double qd_pd_pow(double x, double p) { return p == 0.5 ? sqrt(x) : pow(x, p); }

template <int NBR>
__global__ void __launch_bounds__(QD_BLOCK)
k_phyto_daily(QdPDArgs K) {
    const QdGeom& G = K.G;
    const qd_phyto_daily_params& P = K.p;
    const int j = blockIdx.x * QD_BLOCK + threadIdx.x;
    const int i = G.row0 + blockIdx.y;
    double d[3] = {0.0, 0.0, 0.0};
    if (j < G.nlon) {
        const size_t o = (size_t)qd_lrow(G, i) * G.nlon + j;
        const int NB = P.n_bands, S = P.n_species;
        const double* __restrict__ kd0 = K.tab;
        const double* __restrict__ kchl = kd0 + NB;
        const double* __restrict__ apure = kd0 + 2 * NB;
        const double* __restrict__ dlam = kd0 + 3 * NB;
        const double* __restrict__ wb = kd0 + 4 * NB;
        const double* __restrict__ spA = kd0 + 5 * NB;
        const double* __restrict__ spB = kd0 + 6 * NB;
        const double* __restrict__ tray = kd0 + 7 * NB;
        const double* __restrict__ c_ref = kd0 + 8 * NB;
        const double* __restrict__ p_ref = c_ref + S;
        const double* __restrict__ mu_max = c_ref + 2 * S;
        const double* __restrict__ m0 = c_ref + 3 * S;
        const double* __restrict__ KN = c_ref + 4 * S;
        const double* __restrict__ Y = c_ref + 5 * S;
        const double* __restrict__ shape = c_ref + 6 * S;
        const bool land = K.land[o] != 0;

        // 1) the band split of the cell's two-star insolation (spectral.py:397-426, as k_indiv_substep)
        double a_, b_;
        qd_star_insolation(K.T, K.A, K.B, K.theta, i, j, a_, b_);
        const double tot = a_ + b_;
        double sum = 0.0;
#pragma unroll
        for (int b = 0; b < NBR; ++b)
            if (b < NB) sum += (spA[b] * a_ + spB[b] * b_) * tray[b];
        const bool pos = (sum > 1e-12) && (tot > 1e-12);

        // 2) Kd from the total chlorophyll before the update, 3) mixed-layer light per band times the band width
        double Ct = 0.0;
        for (int s = 0; s < S; ++s) Ct += K.C[(size_t)s * K.stride + o];
        const double chl_pow = qd_pd_pow(qd_max(Ct, 0.0), P.kd_exp_m);
        double Ibd[NBR];
        double kd490 = 0.0;
#pragma unroll
        for (int b = 0; b < NBR; ++b) {
            Ibd[b] = 0.0;
            if (b < NB) {
                double Ib = pos ? (((spA[b] * a_ + spB[b] * b_) * tray[b]) / sum) * tot : 0.0;
                if (!(fabs(Ib) <= DBL_MAX)) Ib = 0.0;
                const double Kd = qd_clip(kd0[b] + kchl[b] * chl_pow, 1e-6, INFINITY);
                if (b == P.idx_490) kd490 = Kd;
                const double x = Kd * P.H_mld;
                const double fac = (x < 1e-6) ? (1.0 - 0.5 * x) + (x * x) / 6.0 : (1.0 - exp(-x)) / qd_max(x, 1e-12);
                Ibd[b] = qd_clip(Ib * fac, 0.0, INFINITY) * dlam[b];
            }
        }

        // 4-7) growth per species, the tracer update, the nutrient uptake and the band reflectances
        const double fT = pow(P.Q10, (K.Tw[o] - P.T_ref) / 10.0);
        const double Nv = K.N[o];
        double Ab[NBR];
#pragma unroll
        for (int b = 0; b < NBR; ++b) Ab[b] = (b < NB) ? apure[b] : 0.0;
        double upt = 0.0, Cnow = 0.0;
        for (int s = 0; s < S; ++s) {
            const double* __restrict__ sh = shape + (size_t)s * NB;
            double E = 0.0;
#pragma unroll
            for (int b = 0; b < NBR; ++b)
                if (b < NB) E = (b == 0) ? sh[0] * Ibd[0] : E + sh[b] * Ibd[b];
            const double muL = tanh(P.alpha_P * E / qd_max(mu_max[s], 1e-6));
            double mg = mu_max[s] * muL * fT;
            if (P.enable_N) mg = mg * qd_clip(Nv / (qd_max(KN[s], 1e-12) + Nv), 0.0, 1.0);
            const double mu = mg - (m0[s] + P.sink);
            double* __restrict__ Cs = K.C + (size_t)s * K.stride;
            const double C0 = Cs[o];
            double Cn = qd_clip(C0 + (mu * C0) * P.dt_days, 0.0, INFINITY);
            if (land) Cn = 0.0;
            Cs[o] = Cn;
            const double u = (mg * Cn) / qd_max(Y[s], 1e-12);
            upt = (s == 0) ? u : upt + u;
            Cnow = (s == 0) ? Cn : Cnow + Cn;
            const double chl = qd_max(Cn, 0.0);
            const double term = (p_ref[s] == 1.0) ? chl : qd_pd_pow(chl, p_ref[s]);
            const double cs = c_ref[s];
#pragma unroll
            for (int b = 0; b < NBR; ++b)
                if (b < NB) Ab[b] = Ab[b] + (cs * sh[b]) * term;
        }
        if (P.enable_N) {
            double Nn = qd_clip(Nv + (-upt + P.R_remin) * P.dt_days, 0.0, INFINITY);
            K.N[o] = land ? 0.0 : Nn;
        }

        // 8) band reflectances, their scalar reduction, Kd(490)
        double as = 0.0;
#pragma unroll
        for (int b = 0; b < NBR; ++b)
            if (b < NB) {
                const double ab = qd_clip(Ab[b], P.alpha_clip_min, P.alpha_clip_max);
                K.bands[(size_t)b * K.plane + o] = ab;
                const double t = ab * wb[b];
                as = (b == 0) ? t : as + t;
            }
        as = qd_clip(as, P.alpha_clip_min, P.alpha_clip_max);
        K.walpha[o] = as;
        K.kd490[o] = kd490;

        // 9) the [PhytoDiag] sums: nan_to_num(x) max(cos lat, 0)
        const double w = K.T.warea[i];
        d[0] = qd_nn(Cnow) * w; d[1] = qd_nn(kd490) * w; d[2] = qd_nn(as) * w;
    }
    qd_block_partials(d, 3, nullptr, K.partial, (size_t)gridDim.x * gridDim.y, (size_t)blockIdx.y * gridDim.x + blockIdx.x);
}

// one workgroup: the three weighted sums over the blocks in a fixed order, divided by sum(max(cos lat, 0)) + 1e-15
__global__ void __launch_bounds__(QD_BLOCK)
k_phyto_daily_finish(const double* __restrict__ partial, int nblk, const double* __restrict__ warea, int nlat, int nlon, double seq,
                     double* __restrict__ rec) {
    double t[4] = {0.0, 0.0, 0.0, 0.0};
    qd_planes_strided(partial, nblk, 3, nullptr, t);
    for (int r = threadIdx.x; r < nlat; r += QD_BLOCK) t[3] += warea[r] * (double)nlon;
    qd_block_totals(t, nullptr);
    if (threadIdx.x == 0) {
        const double ws = t[3] + 1e-15;
        rec[0] = seq; rec[1] = t[0] / ws; rec[2] = t[1] / ws; rec[3] = t[2] / ws;
    }
}

// the cell insolation exactly as k_phyto_daily evaluates it (same device function, same host-side star scalars): what the checks
// compare bit for bit with the ISR_A / ISR_B of k_forcing
__global__ void __launch_bounds__(QD_BLOCK)
k_phyto_daily_insolation(QdGeom G, QdTabs T, QdStar A, QdStar B, double theta, double* __restrict__ outA, double* __restrict__ outB) {
    const int j = blockIdx.x * QD_BLOCK + threadIdx.x;
    if (j >= G.nlon) return;
    const int i = G.row0 + blockIdx.y;
    const size_t o = (size_t)qd_lrow(G, i) * G.nlon + j;
    double a_, b_;
    qd_star_insolation(T, A, B, theta, i, j, a_, b_);
    outA[o] = a_; outB[o] = b_;
}

// ------------------------------------------------------------------ host side
static void pd_free(QdPhytoDaily* d) {
    if (!d) return;
    void* p[] = {d->tab, d->bands, d->partial.p, d->lane.log};
    for (void* q : p) if (q) hipFree(q);
    delete d;
}
void qd_phyto_daily_release(qd_ctx* c) { pd_free(c->pdaily); c->pdaily = nullptr; }

bool qd_phyto_daily_couples(const qd_ctx* c) { return c->pdaily && c->pdaily->p.couple && c->pdaily->n_steps > 0; }

static QdStar pd_star(const double* s) { return QdStar{s[0], std::sin(s[1]), std::cos(s[1]), s[2]}; }   // as qd_forcing_impl

extern "C" int qd_phyto_daily_insolation(qd_handle c, const double* st, double* insA, double* insB) {
    if (!c || !st || !insA || !insB) return -1;
    if (!qd_whole_globe(c)) return qd_fail(c, "qd_phyto_daily_insolation: needs a whole-globe handle");
    hipSetDevice(c->desc.device);
    const QdGeom G = qd_segments(c, 0).g[0];
    const dim3 grid((G.nlon + QD_BLOCK - 1) / QD_BLOCK, G.nrows);
    double* a = c->scratch[10]; double* b = c->scratch[11];
    hipLaunchKernelGGL(k_phyto_daily_insolation, grid, dim3(QD_BLOCK), 0, c->stream, G, c->tabs, pd_star(st), pd_star(st + 3), st[6], a, b);
    const size_t bytes = (size_t)G.nlat * G.nlon * sizeof(double);
    QD_HIP(c, hipMemcpyAsync(insA, a, bytes, hipMemcpyDeviceToHost, c->stream));
    QD_HIP(c, hipMemcpyAsync(insB, b, bytes, hipMemcpyDeviceToHost, c->stream));
    QD_HIP(c, hipStreamSynchronize(c->stream));
    return 0;
}

extern "C" int qd_phyto_daily_configure(qd_handle c, const qd_phyto_daily_params* p, size_t sz, const double* band_tab,
                                        const double* species_tab, const double* shape) {
    if (!c || !p || !band_tab || !species_tab || !shape) return -1;
    if (sz != sizeof(qd_phyto_daily_params)) return qd_fail(c, "qd_phyto_daily_configure: struct size mismatch (ABI)");
    if (!qd_whole_globe(c))
        return qd_fail(c, "qd_phyto_daily_configure: the daily phytoplankton step needs a whole-globe handle (world == 1, n_rows == n_lat); "
                          "latitude bands are not supported");
    const int S = p->n_species, NB = p->n_bands;
    if (S < 1 || S > QD_MAX_SPECIES) return qd_fail(c, "qd_phyto_daily_configure: n_species out of range (1..64)");
    if (NB < 1 || NB > QD_MAXBANDS) return qd_fail(c, "qd_phyto_daily_configure: n_bands out of range (1..32)");
    if (p->idx_490 < 0 || p->idx_490 >= NB) return qd_fail(c, "qd_phyto_daily_configure: idx_490 out of range");
    if (c->phyto.S != S) return qd_fail(c, "qd_phyto_daily_configure: n_species differs from the resident tracers (qd_phyto_configure first)");
    hipSetDevice(c->desc.device);
    QdPhytoDaily* d = c->pdaily;
    const bool first = d == nullptr;
    if (first) d = c->pdaily = new QdPhytoDaily();
    QD_HIP(c, hipStreamSynchronize(c->stream));
    const size_t cells = c->geo.cells();
    const size_t ntab = (size_t)8 * NB + (size_t)6 * S + (size_t)S * NB;
    if (d->tab) { hipFree(d->tab); d->tab = nullptr; }
    QD_HIP(c, hipMalloc(&d->tab, ntab * sizeof(double)));
    std::vector<double> h(ntab);
    std::copy(band_tab, band_tab + (size_t)8 * NB, h.begin());
    std::copy(species_tab, species_tab + (size_t)6 * S, h.begin() + (size_t)8 * NB);
    std::copy(shape, shape + (size_t)S * NB, h.begin() + (size_t)8 * NB + (size_t)6 * S);
    QD_HIP(c, hipMemcpy(d->tab, h.data(), ntab * sizeof(double), hipMemcpyHostToDevice));
    if (first || d->nb_alloc != NB) {
        if (d->bands) { hipFree(d->bands); d->bands = nullptr; }
        QD_HIP(c, hipMalloc(&d->bands, (size_t)NB * cells * sizeof(double)));
        QD_HIP(c, hipMemsetAsync(d->bands, 0, (size_t)NB * cells * sizeof(double), c->stream));
        QD_HIP(c, hipMemsetAsync(c->f[QD_F_KD490], 0, cells * sizeof(double), c->stream));
        d->nb_alloc = NB;
        d->n_steps = 0;
    }
    if (int rc = d->partial.ensure(c, 3, ((c->geo.nlon + QD_BLOCK - 1) / QD_BLOCK) * c->geo.nrows)) return rc;
    d->lane.width = QD_PHYTO_DAILY_LOG_W;
    if (!d->lane.log) QD_HIP(c, hipMalloc(&d->lane.log, d->lane.log_doubles() * sizeof(double)));
    d->p = *p;
    QD_HIP(c, hipStreamSynchronize(c->stream));
    return 0;
}

int qd_phyto_daily_step_impl(qd_ctx* c, const double* st, int use_sst) {
    QdPhytoDaily* d = c->pdaily;
    if (c->phyto.S != d->p.n_species) return qd_fail(c, "qd_phyto_daily: the resident tracers changed their species count since the configure");
    if (d->lane.full()) return qd_fail(c, "qd_phyto_daily: diagnostic log full (drain it with qd_phyto_daily_log)");
    QdScope sc(c, "phyto_daily");
    QdPDArgs K;
    K.G = qd_segments(c, 0).g[0];
    K.T = c->tabs;
    K.A = pd_star(st);
    K.B = pd_star(st + 3);
    K.theta = st[6];
    K.p = d->p;
    K.tab = d->tab;
    K.C = c->phyto.stack[0]; K.stride = c->phyto.stride;
    K.N = c->f[QD_F_PHYTO_N]; K.Tw = use_sst ? c->f[QD_F_SST] : c->f[QD_F_TS]; K.land = c->land;
    K.kd490 = c->f[QD_F_KD490]; K.walpha = c->f[QD_F_WATER_ALPHA]; K.bands = d->bands; K.plane = c->geo.cells();
    K.partial = d->partial.p;
    const dim3 grid((K.G.nlon + QD_BLOCK - 1) / QD_BLOCK, K.G.nrows);
    if (d->p.n_bands <= 16) hipLaunchKernelGGL(k_phyto_daily<16>, grid, dim3(QD_BLOCK), 0, c->stream, K);
    else hipLaunchKernelGGL(k_phyto_daily<32>, grid, dim3(QD_BLOCK), 0, c->stream, K);
    d->n_steps += 1;
    hipLaunchKernelGGL(k_phyto_daily_finish, dim3(1), dim3(QD_BLOCK), 0, c->stream, d->partial.p, (int)(grid.x * grid.y), c->tabs.warea,
                       c->geo.nlat, c->geo.nlon, (double)d->n_steps, d->lane.next());
    for (int k = 0; k < c->phyto.S; ++k) qd_mark(c, {c->phyto.cur[k]}, 0);
    qd_mark(c, {c->f[QD_F_PHYTO_N], c->f[QD_F_KD490], c->f[QD_F_WATER_ALPHA]}, 0);
    return 0;
}

extern "C" int qd_phyto_daily(qd_handle c, const double* star_row, int use_sst) {
    if (!c || !star_row) return -1;
    if (!qd_whole_globe(c)) return qd_fail(c, "qd_phyto_daily: the daily phytoplankton step needs a whole-globe handle; latitude bands are not supported");
    if (!c->pdaily) return qd_fail(c, "qd_phyto_daily: qd_phyto_daily_configure has not been called");
    hipSetDevice(c->desc.device);
    if (int rc = qd_phyto_daily_step_impl(c, star_row, use_sst ? 1 : 0)) return rc;
    return qd_launch_check(c, "qd_phyto_daily");
}

static QdSpanLane* pd_lane(qd_ctx* c) { return c && c->pdaily ? &c->pdaily->lane : nullptr; }
static const char* const PD_MISSING = "qd_phyto_daily_configure has not been called";

extern "C" int qd_phyto_daily_schedule(qd_handle c, int n, const int32_t* fire) {
    return qd_lane_schedule(c, pd_lane(c), n, fire, "qd_phyto_daily_schedule", PD_MISSING);
}

QdSpanLane* qd_phyto_daily_span_begin(qd_ctx* c, int n, int with_phys) {
    static const QdSpanTexts T = {
        "qd_step_n: the daily phytoplankton step (bit8) needs a whole-globe handle; latitude bands are not supported",
        "qd_step_n: bit8 set but qd_phyto_daily_configure has not been called",
        "qd_step_n: bit8 needs a qd_phyto_daily_schedule of exactly n steps before the span",
        "qd_step_n: the span's daily steps would overflow the diagnostic log (drain it first)"};
    const bool stale = c->pdaily && c->phyto.S != c->pdaily->p.n_species;
    return qd_lane_span_begin(c, pd_lane(c), n, T,
                              with_phys ? nullptr : "qd_step_n: the daily phytoplankton step (bit8) needs the driver physics (bit1)",
                              stale ? "qd_step_n: the resident tracers changed their species count since qd_phyto_daily_configure" : nullptr);
}

extern "C" int qd_phyto_daily_log(qd_handle c, double* out, int max, int* n) {
    return qd_lane_drain(c, pd_lane(c), out, max, n, "qd_phyto_daily_log", PD_MISSING);
}

bool qd_phyto_daily_bands(const qd_ctx* c, const double** bands, int* n_bands, int64_t* n_steps) {
    const QdPhytoDaily* d = c->pdaily;
    if (!d || !d->bands) return false;
    *bands = d->bands; *n_bands = d->nb_alloc; *n_steps = d->n_steps;
    return true;
}

extern "C" int qd_phyto_daily_download_bands(qd_handle c, double* host, size_t n) {
    if (!c || !host) return -1;
    QdPhytoDaily* d = c->pdaily;
    if (!d) return qd_fail(c, "qd_phyto_daily_download_bands: qd_phyto_daily_configure has not been called");
    const size_t plane = (size_t)c->geo.nlat * c->geo.nlon;
    if (n != (size_t)d->nb_alloc * plane) return qd_fail(c, "qd_phyto_daily_download_bands: element count does not match n_bands * n_lat * n_lon");
    hipSetDevice(c->desc.device);
    for (int b = 0; b < d->nb_alloc; ++b)
        QD_HIP(c, hipMemcpyAsync(host + (size_t)b * plane, d->bands + (size_t)b * c->geo.cells(), plane * sizeof(double),
                                 hipMemcpyDeviceToHost, c->stream));
    QD_HIP(c, hipStreamSynchronize(c->stream));
    return 0;
}

int64_t qd_phyto_daily_steps(qd_ctx* c, int64_t set) {
    if (!c->pdaily) return 0;
    if (set >= 0) c->pdaily->n_steps = set;
    return c->pdaily->n_steps;
}

extern "C" int qd_phyto_daily_state(qd_handle c, int64_t* n_steps) {
    if (!c || !n_steps) return -1;
    *n_steps = c->pdaily ? c->pdaily->n_steps : 0;
    return 0;
}
