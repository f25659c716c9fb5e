// qd_eco_div.hip -- the diversity diagnostics on a [S][K][lat][lon] LAI stack, gfx950 (qd_eco_diversity).
//
// pygcm/ecology/diversity.py: _get_species_lai_SK (:8-25), compute_alpha_eff_map (:34-58), compute_whittaker_beta (:61-88),
// compute_local_bray_curtis (:91-135); the reference driver runs them every QD_ECO_DIVERSITY_EVERY_DAYS (run_simulation.py:2406-2414).
//   k_div_alpha<SMAX>   pointwise, QD_DIV_R rows per thread: the S * K planes are read once; L_s = sum_k max(plane, 0) (plane after
//                       plane, np.sum(axis=1)) stays in registers and is written once; L_tot = sum_s L_s in s order; on land with
//                       L_tot > 0 alpha = exp(-sum_s p log(p + 1e-15)), p = L_s / (L_tot + 1e-15), NaN elsewhere; the thread's
//                       nansum terms alpha w_norm and L_s w_norm (land only) -> one partial per workgroup and quantity.
//   k_div_bc            one wave per strip of QD_DIV_RS rows x 62 columns (lanes 1..62; lanes 0 and 63 hold the wrapped neighbour
//                       columns): species after species the strip's RS + 2 rows of L_s pass through registers, north / south come
//                       from the neighbouring row registers, west / east by DPP lane shifts (qd_wave.h), so L_s is read
//                       (RS + 2) / RS * 64 / 62 = 1.29 times.  Per shift sum_s min(a_s, b_s) in s order, sum_a = L_tot in s order;
//                       bc = 1 - 2 (min_sum / ((sum_a + sum_b) + 1e-15)), accumulated in the order up, down, west, east over the
//                       shifts whose both cells are land, divided by their count.  Rows are clipped at the poles (a pole cell is
//                       its own neighbour, as in the reference), columns wrap.
//                       sum_b is NOT the neighbour's L_tot bit for bit: the reference gathers the neighbour stack with index
//                       arrays (L_s[:, j_nbr, i_nbr]), NumPy lays that result out with the species axis contiguous, and np.sum
//                       over a contiguous axis runs its pairwise loop -- for n < 128 terms eight interleaved partial sums r[q] +=
//                       a[8 m + q], combined as ((r0 + r1) + (r2 + r3)) + ((r4 + r5) + (r6 + r7)), the n mod 8 last terms added one
//                       by one (n < 8: 0 + a0 + a1 ...).  k_div_alpha forms that sum of every cell from the L_s in its registers
//                       and stores it as one more plane (L_pair); k_div_bc reads the neighbours' values of it.
//   k_div_final         one workgroup: the partials in a fixed order -> T_s, alpha_mean, gamma_eff, beta_whittaker.
// np.maximum / np.minimum propagate NaN: qd_max / qd_min (qd_internal.h), not fmax / fmin.  f64, contraction off (Makefile), no
// atomics.  No transcendental touches L_s or the Bray-Curtis map: both equal NumPy's bit for bit.
#include "qd_internal.h"
#include "qd_wave.h"
#include "qd_blockred.h"
#include <algorithm>

#define QD_DIV_R 4                // rows per thread of k_div_alpha
#define QD_DIV_RS 8               // rows per strip of k_div_bc
#define QD_DIV_TC 62              // owned columns per strip of k_div_bc

struct QdEcoDiv {
    int nlat = 0, nlon = 0, S = 0;            // shape of the results held
    int valid = 0;
    double* Ls = nullptr;  size_t ls_cap = 0;         // [S][cells]
    double* alpha = nullptr; double* bc = nullptr; double* lpair = nullptr; size_t map_cap = 0;   // [cells]; lpair: L_tot in NumPy's pairwise order
    double* stage = nullptr; size_t stage_cap = 0;    // a host-passed stack
    uint8_t* land = nullptr; size_t land_cap = 0;     // a caller's land mask (qd_eco_diversity_on)
    double* wrow = nullptr; int wrow_cap = 0;         // [nlat]
    QdPartials partial;                               // [1 + S][nblk]: alpha, then L_s
    double* out3 = nullptr;                           // device {alpha_mean, gamma_eff, beta_whittaker}
    double summary[3] = {0, 0, 0};
};

struct QdDivArgs {
    int nlat, nlon, S, K;
    const double* L; size_t plane;
    const uint8_t* land;
    const double* wrow;
    double* Ls; double* alpha; double* bc; double* lpair;
    double* partial;
};

__device__ __forceinline__ int qd_dv_east_i(int x) { return __builtin_amdgcn_update_dpp(0, x, 0x130, 0xf, 0xf, true); }   // lane + 1
__device__ __forceinline__ int qd_dv_west_i(int x) { return __builtin_amdgcn_update_dpp(0, x, 0x138, 0xf, 0xf, true); }   // lane - 1

// ------------------------------------------------------------------ L_s, alpha map, nansum partials
template <int SMAX>
__global__ void __launch_bounds__(QD_BLOCK)
k_div_alpha(QdDivArgs A) {
    const int j = blockIdx.x * QD_BLOCK + threadIdx.x;
    const int S = A.S, K = A.K;
    double acc[SMAX + 1];                                      // [0] alpha, [1 + s] L_s
#pragma unroll
    for (int s = 0; s <= SMAX; ++s) acc[s] = 0.0;
    if (j < A.nlon) {
        for (int rr = 0; rr < QD_DIV_R; ++rr) {
            const int row = blockIdx.y * QD_DIV_R + rr;
            if (row >= A.nlat) break;
            const size_t o = (size_t)row * A.nlon + j;
            const bool land = A.land[o] == 1;
            const double wn = A.wrow[row];
            double ls[SMAX];
            double ltot = 0.0;
#pragma unroll
            for (int s = 0; s < SMAX; ++s)
                if (s < S) {
                    double x = 0.0;
                    for (int k = 0; k < K; ++k) {
                        const double v = qd_max(A.L[(size_t)(s * K + k) * A.plane + o], 0.0);
                        x = (k == 0) ? v : x + v;
                    }
                    ls[s] = x;
                    A.Ls[(size_t)s * A.plane + o] = x;
                    ltot = (s == 0) ? x : ltot + x;
                }
            {                                                  // the same total in np.sum's order over a contiguous axis (header)
                const int s8 = S & ~7;
                double r[8];
#pragma unroll
                for (int q = 0; q < 8; ++q) r[q] = 0.0;
#pragma unroll
                for (int s = 0; s < SMAX; ++s)
                    if (s < s8) r[s & 7] = (s < 8) ? ls[s] : r[s & 7] + ls[s];
                double lp = (S >= 8) ? ((r[0] + r[1]) + (r[2] + r[3])) + ((r[4] + r[5]) + (r[6] + r[7])) : 0.0;
#pragma unroll
                for (int s = 0; s < SMAX; ++s)
                    if (s >= s8 && s < S) lp += ls[s];
                A.lpair[o] = lp;
            }
            double alpha = NAN;
            if (land && ltot > 0.0) {
                const double denom = ltot + 1e-15;
                double h = 0.0;
#pragma unroll
                for (int s = 0; s < SMAX; ++s)
                    if (s < S) {
                        const double p = ls[s] / denom;
                        const double t = p * log(p + 1e-15);
                        h = (s == 0) ? t : h + t;
                    }
                alpha = exp(-h);
            }
            A.alpha[o] = alpha;
            if (land) {                                        // np.nansum: NaN terms count as 0
                const double ta = alpha * wn;
                if (ta == ta) acc[0] += ta;
#pragma unroll
                for (int s = 0; s < SMAX; ++s)
                    if (s < S) {
                        const double t = ls[s] * wn;
                        if (t == t) acc[s + 1] += t;
                    }
            }
        }
    }
    qd_block_partials(acc, S + 1, nullptr, A.partial, (size_t)gridDim.x * gridDim.y, (size_t)blockIdx.y * gridDim.x + blockIdx.x);
}

// ------------------------------------------------------------------ local Bray-Curtis map
__global__ void __launch_bounds__(QD_BLOCK)
k_div_bc(QdDivArgs A, int ncs, int nstrips) {
    const int lane = threadIdx.x & 63;
    const int strip = blockIdx.x * (QD_BLOCK / 64) + (threadIdx.x >> 6);
    if (strip >= nstrips) return;                              // wave-uniform
    const int rs = strip / ncs, cs = strip - rs * ncs;
    const int r0 = rs * QD_DIV_RS;
    const int j = cs * QD_DIV_TC + lane - 1;                   // lane 0: the column west of the strip, lane 63: east of it
    int jw = j % A.nlon;                                       // the column this lane loads (periodic)
    if (jw < 0) jw += A.nlon;
    const bool owned = lane >= 1 && lane <= QD_DIV_TC && j < A.nlon;
    size_t off[QD_DIV_RS + 2];                                 // rows r0 - 1 .. r0 + RS, clipped at the poles
    int lm[QD_DIV_RS + 2];
#pragma unroll
    for (int t = 0; t < QD_DIV_RS + 2; ++t) {
        off[t] = (size_t)qd_clampi(r0 - 1 + t, 0, A.nlat - 1) * A.nlon + jw;
        lm[t] = A.land[off[t]] == 1 ? 1 : 0;
    }
    double mU[QD_DIV_RS], mD[QD_DIV_RS], mW[QD_DIV_RS], mE[QD_DIV_RS], tot[QD_DIV_RS], lp[QD_DIV_RS + 2];
#pragma unroll
    for (int r = 0; r < QD_DIV_RS; ++r) { mU[r] = 0.0; mD[r] = 0.0; mW[r] = 0.0; mE[r] = 0.0; tot[r] = 0.0; }
#pragma unroll
    for (int t = 0; t < QD_DIV_RS + 2; ++t) lp[t] = A.lpair[off[t]];
    for (int s = 0; s < A.S; ++s) {
        const double* P = A.Ls + (size_t)s * A.plane;
        double v[QD_DIV_RS + 2];
#pragma unroll
        for (int t = 0; t < QD_DIV_RS + 2; ++t) v[t] = P[off[t]];
#pragma unroll
        for (int r = 0; r < QD_DIV_RS; ++r) {
            const double a = v[r + 1];
            tot[r] += a;
            mU[r] += qd_min(a, v[r]);
            mD[r] += qd_min(a, v[r + 2]);
            mW[r] += qd_min(a, qd_west(a));
            mE[r] += qd_min(a, qd_east(a));
        }
    }
#pragma unroll
    for (int r = 0; r < QD_DIV_RS; ++r) {
        const double sa = tot[r];
        const double sw = qd_west(lp[r + 1]), se = qd_east(lp[r + 1]);      // every lane takes part in the shifts
        const int lw = qd_dv_west_i(lm[r + 1]), le = qd_dv_east_i(lm[r + 1]);
        const int row = r0 + r;
        double accum = 0.0, count = 0.0;
        if (lm[r + 1]) {
            if (lm[r])     { accum += 1.0 - 2.0 * (mU[r] / ((sa + lp[r]) + 1e-15));     count += 1.0; }
            if (lm[r + 2]) { accum += 1.0 - 2.0 * (mD[r] / ((sa + lp[r + 2]) + 1e-15)); count += 1.0; }
            if (lw)        { accum += 1.0 - 2.0 * (mW[r] / ((sa + sw) + 1e-15));         count += 1.0; }
            if (le)        { accum += 1.0 - 2.0 * (mE[r] / ((sa + se) + 1e-15));         count += 1.0; }
        }
        if (owned && row < A.nlat)
            A.bc[(size_t)row * A.nlon + j] = (lm[r + 1] && count > 0.0) ? accum / count : NAN;
    }
}

// ------------------------------------------------------------------ Whittaker summary from the partials
__global__ void __launch_bounds__(QD_BLOCK)
k_div_final(const double* __restrict__ partial, int nblk, int S, double* __restrict__ out3) {
    __shared__ double tot[QD_MAX_SPECIES + 1];
    qd_planes_by_wave(partial, nblk, S + 1, tot);
    if (threadIdx.x == 0) {
        const double alpha_mean = tot[0];
        double tsum = 0.0;
        for (int s = 0; s < S; ++s) tsum = (s == 0) ? tot[1] : tsum + tot[s + 1];
        tsum = tsum + 1e-15;
        double h = 0.0;
        for (int s = 0; s < S; ++s) {
            const double p = tot[s + 1] / tsum;
            const double t = p * log(p + 1e-15);
            h = (s == 0) ? t : h + t;
        }
        const double gamma = exp(-h);
        const double am = (1e-12 > alpha_mean) ? 1e-12 : alpha_mean;    // Python's max(alpha_mean, 1e-12)
        out3[0] = alpha_mean; out3[1] = gamma; out3[2] = gamma / am;
    }
}

// ------------------------------------------------------------------ host side
void qd_eco_div_release(qd_ctx* c) {
    QdEcoDiv* d = c->ediv;
    if (!d) return;
    void* p[] = {d->Ls, d->alpha, d->bc, d->lpair, d->stage, d->land, d->wrow, d->partial.p, d->out3};
    for (void* q : p) if (q) hipFree(q);
    delete d;
    c->ediv = nullptr;
}

template <class T> static hipError_t div_grow(T** p, size_t* cap, size_t n) {
    if (*p && *cap >= n) return hipSuccess;
    if (*p) { hipFree(*p); *p = nullptr; *cap = 0; }
    const hipError_t e = hipMalloc((void**)p, n * sizeof(T));
    if (e == hipSuccess) *cap = n;
    return e;
}

// land_host != nullptr: the caller's grid and mask; else the handle's.  layers_host == nullptr: L_dev (the resident stack).
static int div_run(qd_ctx* c, const char* who, int nlat, int nlon, const uint8_t* land_host, const double* layers_host,
                   const double* L_dev, int S, int K, const double* w_norm_row, double* summary3) {
    hipSetDevice(c->desc.device);
    QdEcoDiv* d = c->ediv;
    if (!d) d = c->ediv = new QdEcoDiv();
    d->valid = 0;
    const size_t cells = (size_t)nlat * nlon;
    QD_HIP(c, hipStreamSynchronize(c->stream));                // buffers may be regrown: nothing of an earlier call is in flight
    QD_HIP(c, div_grow(&d->Ls, &d->ls_cap, (size_t)S * cells));
    if (!d->alpha || d->map_cap < cells) {
        if (d->alpha) { hipFree(d->alpha); d->alpha = nullptr; }
        if (d->bc) { hipFree(d->bc); d->bc = nullptr; }
        if (d->lpair) { hipFree(d->lpair); d->lpair = nullptr; }
        d->map_cap = 0;
        QD_HIP(c, hipMalloc(&d->alpha, cells * sizeof(double)));
        QD_HIP(c, hipMalloc(&d->bc, cells * sizeof(double)));
        QD_HIP(c, hipMalloc(&d->lpair, cells * sizeof(double)));
        d->map_cap = cells;
    }
    { size_t cap = (size_t)d->wrow_cap; QD_HIP(c, div_grow(&d->wrow, &cap, (size_t)nlat)); d->wrow_cap = (int)cap; }
    const dim3 grid_a((nlon + QD_BLOCK - 1) / QD_BLOCK, (nlat + QD_DIV_R - 1) / QD_DIV_R), block(QD_BLOCK);
    if (int rc = d->partial.ensure(c, S + 1, (int)(grid_a.x * grid_a.y))) return rc;
    if (!d->out3) QD_HIP(c, hipMalloc(&d->out3, 3 * sizeof(double)));
    if (layers_host) {
        QD_HIP(c, div_grow(&d->stage, &d->stage_cap, (size_t)S * K * cells));
        QD_HIP(c, hipMemcpyAsync(d->stage, layers_host, (size_t)S * K * cells * sizeof(double), hipMemcpyHostToDevice, c->stream));
        L_dev = d->stage;
    }
    const uint8_t* land = c->land;
    if (land_host) {
        QD_HIP(c, div_grow(&d->land, &d->land_cap, cells));
        QD_HIP(c, hipMemcpyAsync(d->land, land_host, cells, hipMemcpyHostToDevice, c->stream));
        land = d->land;
    }
    QD_HIP(c, hipMemcpyAsync(d->wrow, w_norm_row, (size_t)nlat * sizeof(double), hipMemcpyHostToDevice, c->stream));
    QD_HIP(c, hipStreamSynchronize(c->stream));                // the host buffers are only borrowed for the call
    QdDivArgs A;
    A.nlat = nlat; A.nlon = nlon; A.S = S; A.K = K;
    A.L = L_dev; A.plane = cells; A.land = land; A.wrow = d->wrow;
    A.Ls = d->Ls; A.alpha = d->alpha; A.bc = d->bc; A.lpair = d->lpair; A.partial = d->partial.p;
    {
        QdScope sc(c, "eco_diversity");
        if (S <= 8) hipLaunchKernelGGL(k_div_alpha<8>, grid_a, block, 0, c->stream, A);
        else if (S <= 24) hipLaunchKernelGGL(k_div_alpha<24>, grid_a, block, 0, c->stream, A);
        else hipLaunchKernelGGL(k_div_alpha<QD_MAX_SPECIES>, grid_a, block, 0, c->stream, A);
        const int ncs = (nlon + QD_DIV_TC - 1) / QD_DIV_TC, nrs = (nlat + QD_DIV_RS - 1) / QD_DIV_RS;
        const int nstrips = ncs * nrs, wpb = QD_BLOCK / 64;
        hipLaunchKernelGGL(k_div_bc, dim3((nstrips + wpb - 1) / wpb), block, 0, c->stream, A, ncs, nstrips);
        hipLaunchKernelGGL(k_div_final, dim3(1), block, 0, c->stream, d->partial.p, d->partial.nblk, S, d->out3);
    }
    QD_HIP(c, hipMemcpyAsync(d->summary, d->out3, 3 * sizeof(double), hipMemcpyDeviceToHost, c->stream));
    QD_HIP(c, hipStreamSynchronize(c->stream));
    const hipError_t e = hipGetLastError();
    if (e != hipSuccess) return qd_fail(c, (std::string(who) + ": kernel").c_str(), e);
    d->nlat = nlat; d->nlon = nlon; d->S = S; d->valid = 1;
    if (summary3) for (int k = 0; k < 3; ++k) summary3[k] = d->summary[k];
    return 0;
}

static int div_sizes(qd_ctx* c, const char* who, int S, int K) {
    if (S < 1 || S > QD_MAX_SPECIES) return qd_fail(c, (std::string(who) + ": n_species out of range (1..64)").c_str());
    if (K < 1 || K > QD_ECO_DAILY_MAX_K) return qd_fail(c, (std::string(who) + ": n_layers out of range (1..8)").c_str());
    return 0;
}

extern "C" int qd_eco_diversity(qd_handle c, const double* layers, int n_species, int n_layers, const double* w_norm_row, double* summary3) {
    if (!c || !w_norm_row) return -1;
    const char* who = "qd_eco_diversity";
    if (!qd_whole_globe(c))
        return qd_fail(c, "qd_eco_diversity: the diversity diagnostics need a whole-globe handle (world == 1, n_rows == n_lat); "
                          "latitude bands are not supported");
    if (int rc = div_sizes(c, who, n_species, n_layers)) return rc;
    const double* L = nullptr;
    if (!layers) {
        int S = 0, K = 0;
        if (!qd_eco_daily_stack(c, &L, &S, &K))
            return qd_fail(c, "qd_eco_diversity: layers is NULL and there is no resident stack (qd_eco_daily_configure has not been called)");
        if (S != n_species || K != n_layers)
            return qd_fail(c, "qd_eco_diversity: n_species / n_layers are not those of the resident stack");
    }
    return div_run(c, who, c->geo.nlat, c->geo.nlon, nullptr, layers, L, n_species, n_layers, w_norm_row, summary3);
}

extern "C" int qd_eco_diversity_on(qd_handle c, int n_lat, int n_lon, const uint8_t* land_mask, const double* layers, int n_species,
                                   int n_layers, const double* w_norm_row, double* summary3) {
    if (!c || !land_mask || !layers || !w_norm_row) return -1;
    const char* who = "qd_eco_diversity_on";
    if (n_lat < 2 || n_lon < 3) return qd_fail(c, "qd_eco_diversity_on: the grid needs n_lat >= 2 and n_lon >= 3");
    if ((size_t)n_lat * (size_t)n_lon > (size_t)INT_MAX) return qd_fail(c, "qd_eco_diversity_on: grid too large");
    if (int rc = div_sizes(c, who, n_species, n_layers)) return rc;
    return div_run(c, who, n_lat, n_lon, land_mask, layers, nullptr, n_species, n_layers, w_norm_row, summary3);
}

extern "C" int qd_eco_diversity_download(qd_handle c, int field, double* host, size_t n) {
    if (!c || !host) return -1;
    const QdEcoDiv* d = c->ediv;
    if (!d || !d->valid) return qd_fail(c, "qd_eco_diversity_download: no diversity results on this handle (call qd_eco_diversity first)");
    const size_t cells = (size_t)d->nlat * d->nlon;
    const double* src = nullptr; size_t want = cells;
    switch (field) {
        case QD_F_ECO_DIV_LS: src = d->Ls; want = (size_t)d->S * cells; break;
        case QD_F_ECO_DIV_ALPHA: src = d->alpha; break;
        case QD_F_ECO_DIV_BC: src = d->bc; break;
        case QD_F_ECO_DIV_SUMMARY: want = 3; break;
        default: return qd_fail(c, "qd_eco_diversity_download: unknown field");
    }
    if (n != want) return qd_fail(c, "qd_eco_diversity_download: size mismatch");
    if (!src) { for (int k = 0; k < 3; ++k) host[k] = d->summary[k]; return 0; }
    hipSetDevice(c->desc.device);
    QD_HIP(c, hipMemcpyAsync(host, src, want * sizeof(double), hipMemcpyDeviceToHost, c->stream));
    QD_HIP(c, hipStreamSynchronize(c->stream));
    return 0;
}
