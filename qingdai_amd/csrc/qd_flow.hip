// qd_flow.hip -- flow kinematics of the resident winds: relative vorticity zeta, divergence delta, streamfunction psi and velocity
// potential chi, one record of scalars per sampled step and four resident sum planes, as a span lane, gfx950 (QD_FLOW).
//
// The definition is qingdai_amd/flow.py: helmholtz_reference (grid quantities, the pole rule, the finite-volume Laplacian L, the
// solve L psi = zeta - mean(zeta), L chi = delta - mean(delta)); the host forms the grid table tab [QD_FLOW_TAB][n_lat] =
// c_j | c_{j+1/2} | w_j | c_{j+1/2} / dphi | dphi / c_j | a^2 w_j and lam [K] (K = n_lon / 2 + 1) once and hands them to configure.
// A sample is six launches, every one with a workgroup of QD_BLOCK threads per latitude row unless said otherwise:
//   k_flow_vortdiv   zeta, delta planes from (U, V): SphericalGrid.vorticity / .divergence in the reference's operation order on the
//                    rows 1 .. N - 2; on a pole row the lane-order row sum of the cap's mean tangential / normal wind (below), the
//                    value constant along the row.  Also the row partials of the first reduction stage: sum, sum of squares and
//                    max |.| of zeta and delta, sum of (u^2 + v^2) / 2 (0 on pole rows), 1.0 when the row of U or V holds a
//                    non-finite value.
//   k_flow_fwd       the row DFT of zeta and delta in ONE complex transform of length n = n_lon, y = zeta + i delta, separated by
//                    Z(k) = (Y(k) + conj Y(n - k)) / 2, D(k) = (Y(k) - conj Y(n - k)) / (2i), k < K; spectral planes [row][k], Re and
//                    Im apart.  fft (n = 2^a 3^b 5^c): qd_rowfft.h; direct (any n, QD_FLOW_FORM=direct): row and table in LDS,
//                    thread k adds x[i] cos / sin(2 pi ((i k) mod n) / n) for i ascending.
//   k_flow_lat       one thread per (field, k): first every workgroup combines the row partials across rows (it needs the two
//                    means; workgroup 0 writes the record's first-stage scalars and the count of bad rows).  k >= 1: Thomas
//                    elimination over the rows 1 .. N - 2 of the system scaled by w_j, lower c_{j-1/2} / dphi, upper
//                    c_{j+1/2} / dphi, diagonal -(upper + lower) + lam_k dphi / c_j, right side a^2 w_j Z_j(k), Re and Im carried
//                    together, one reciprocal per row, the modified upper coefficients kept in a plane of their own, the solution
//                    written over the right side; the pole rows are 0.  k = 0: F_j = sum_{l <= j} a^2 w_l (Z_l(0) - n mean),
//                    psi_{j+1} = psi_j + F_j / (c_{j+1/2} / dphi) from psi_0 = 0, then sum_j w_j psi_j / sum_j w_j is removed; all
//                    sums ascending in j.  The coefficients are derived in the kernel from the row tables, which every workgroup
//                    stages in LDS once.  The walk over the rows is a latency chain: rows are taken in batches of QF_LAT_B whose
//                    loads are issued together, one batch ahead of the arithmetic, so the chain waits for no memory; the two
//                    k = 0 walks have the last workgroup to themselves (in a wave shared with k >= 1 the two paths would run
//                    one after the other).
//   k_flow_inv       the inverse row transform of psi^ + i chi^ (Hermitian extension, conj - forward FFT - conj, / n; or the direct
//                    sum over k ascending) -> psi, chi planes; NaN in every cell when a row was bad.
//   k_flow_finish    rotational and divergent wind by centred differences on the rows 1 .. N - 2 (u_psi = -(dpsi / dphi) / a,
//                    v_psi = (dpsi / dlam) / (a c_j), u_chi = (dchi / dlam) / (a c_j), v_chi = (dchi / dphi) / a), the row partials of
//                    their kinetic energies and of min / max of psi and chi, and sum = sum + x on the four sum planes.
//   k_flow_record    one workgroup: the second-stage scalars.
// REDUCTION ORDER (series.reduce_reference's, restated by flow.scalars_reference bit for bit): a row sum is taken by ONE wave, lane
// l owning the cells 128 k + 2 l and 128 k + 2 l + 1, added in ascending order from +0.0, then the five halvings of
// qd_blockred.h; across rows lane l takes the rows l, l + 64, ... ascending, num = num + w_j S_j (the product rounded),
// W = W + w_j, the five halvings, mean = num / (n W).  min / max are fmin / fmax (order-free as values), max |.| starts at 0.
// Pole rule: with S the lane-order row sum of (x[pole row][i] + x[next row][i]) / 2, val = (c_half S) / ((a w_P) n); zeta_N = +val(u),
// zeta_S = -val(u), delta_N = -val(v), delta_S = +val(v).
// No atomics, no scratch: the same planes give the same bits, run after run.  Whole-globe handles only; qd_flow_solve_grid runs
// the same kernels without a handle (qd_create needs five rows, the solve three).
#include "qd_span.h"
#include "qd_blockred.h"
#include "qd_rowfft.h"
#include <algorithm>
#include <cmath>
#include <cstdlib>
#include <cstring>

#define QF_LDS_LIMIT (150 * 1024)     // bytes of the CU's 160 KB LDS one workgroup may take here (k_spectra_rows' limit)
#define QF_NROW1 8                    // row partials of k_flow_vortdiv
#define QF_NROW2 6                    // row partials of k_flow_finish
#define QF_LAT_B 24                   // rows of k_flow_lat whose loads are in flight together (and as many again one batch ahead)
#define QF_FINITE(x) (fabs(x) <= 1.7976931348623157e308)
static_assert(QD_BLOCK / 64 == 4, "k_flow_*: four waves share the reductions of a row");
static_assert(QD_FLOW_TAB == 6 && QD_FLOW_PLANES == 4 && QD_FLOW_REC_W == 14, "the public header's flow constants");

struct QdFlowGrid {
    int nlat, nlon, K;
    double a, dlat, dlon;
    const double* tab;                // [QD_FLOW_TAB][nlat]
    const double* lam;                // [K]
    const double* tw;                 // [2][nlon] cos / sin(2 pi t / nlon)
    __device__ __forceinline__ double c(int j) const { return tab[j]; }
    __device__ __forceinline__ double ch(int j) const { return tab[nlat + j]; }
    __device__ __forceinline__ double w(int j) const { return tab[2 * nlat + j]; }
    __device__ __forceinline__ double chd(int j) const { return tab[3 * nlat + j]; }
    __device__ __forceinline__ double e(int j) const { return tab[4 * nlat + j]; }
    __device__ __forceinline__ double aw(int j) const { return tab[5 * nlat + j]; }
};

// ---- the fixed-order reductions (one wave each; results valid in lane 0)
__device__ __forceinline__ double qf_row_sum(const double* x, int n, int lane) {
    double acc = 0.0;
    for (int i = 2 * lane; i < n; i += 128) { acc = acc + x[i]; if (i + 1 < n) acc = acc + x[i + 1]; }
    return qd_wave_sum(acc);
}
__device__ __forceinline__ double qf_row_sumsq(const double* x, int n, int lane) {
    double acc = 0.0;
    for (int i = 2 * lane; i < n; i += 128) { acc = acc + x[i] * x[i]; if (i + 1 < n) acc = acc + x[i + 1] * x[i + 1]; }
    return qd_wave_sum(acc);
}
__device__ __forceinline__ double qf_row_maxabs(const double* x, int n, int lane) {
    double acc = 0.0;
    for (int i = lane; i < n; i += 64) acc = fmax(acc, fabs(x[i]));
    return qd_wave_fmax(acc);
}
__device__ __forceinline__ double qf_cross_mean(const QdFlowGrid& G, const double* __restrict__ S, int lane) {
    double num = 0.0, W = 0.0;
    for (int j = lane; j < G.nlat; j += 64) { const double w = G.w(j); num = num + w * S[j]; W = W + w; }
    num = qd_wave_sum(num); W = qd_wave_sum(W);
    return num / ((double)G.nlon * W);
}
__device__ __forceinline__ double qf_cross(const double* __restrict__ S, int nlat, int lane, QdRedOp op) {      // sum, fmin or fmax over rows
    double a = op == QD_RED_SUM ? 0.0 : (op == QD_RED_MIN ? INFINITY : -INFINITY);
    for (int j = lane; j < nlat; j += 64) a = qd_red_join(a, S[j], op);
    return qd_red_wave(a, op);
}

// ------------------------------------------------------------------ zeta, delta and the first row partials
// dynamic LDS: zr[n], dr[n], ke[n]
__global__ void __launch_bounds__(QD_BLOCK)
k_flow_vortdiv(QdFlowGrid G, const double* __restrict__ u, const double* __restrict__ v, double* __restrict__ Z, double* __restrict__ D,
               double* __restrict__ rowstat) {
    extern __shared__ double qf_lds[];
    __shared__ int s_bad;
    __shared__ double s_pole[2];
    const int n = G.nlon, N = G.nlat, j = blockIdx.x, lane = threadIdx.x & 63, wv = threadIdx.x >> 6;
    double* zr = qf_lds; double* dr = zr + n; double* ke = dr + n;
    const bool pole = j == 0 || j == N - 1;
    const size_t row = (size_t)j * n;
    if (threadIdx.x == 0) s_bad = 0;
    __syncthreads();
    int nonfinite = 0;
    if (!pole) {
        const double cn = G.c(j + 1), cs = G.c(j - 1), pre = 1 / (G.a * fmax(G.c(j), 1e-6));
        const double* un = u + row + n; const double* us = u + row - n;
        const double* vn = v + row + n; const double* vs = v + row - n;
        for (int i = threadIdx.x; i < n; i += QD_BLOCK) {
            const int ip = i + 1 == n ? 0 : i + 1, im = i == 0 ? n - 1 : i - 1;
            const double u0 = u[row + i], v0 = v[row + i];
            nonfinite |= (!QF_FINITE(u0) || !QF_FINITE(v0)) ? 1 : 0;
            const double dv_dlon = (v[row + ip] - v[row + im]) / (2 * G.dlon);
            const double du_dlon = (u[row + ip] - u[row + im]) / (2 * G.dlon);
            const double ducos = (un[i] * cn - us[i] * cs) / (2 * G.dlat);
            const double dvcos = (vn[i] * cn - vs[i] * cs) / (2 * G.dlat);
            zr[i] = pre * (dv_dlon - ducos);
            dr[i] = pre * (du_dlon + dvcos);
            ke[i] = 0.5 * (u0 * u0 + v0 * v0);
        }
    } else {
        const size_t nb = j == 0 ? row + n : row - n;      // the neighbouring row
        for (int i = threadIdx.x; i < n; i += QD_BLOCK) {
            const double u0 = u[row + i], v0 = v[row + i];
            nonfinite |= (!QF_FINITE(u0) || !QF_FINITE(v0)) ? 1 : 0;
            zr[i] = 0.5 * (u0 + u[nb + i]);
            dr[i] = 0.5 * (v0 + v[nb + i]);
        }
    }
    if (nonfinite) s_bad = 1;                               // (every writer stores the same value)
    __syncthreads();
    if (pole) {
        if (wv < 2) {
            const double S = qf_row_sum(wv == 0 ? zr : dr, n, lane);
            if (lane == 0) s_pole[wv] = S;
        }
        __syncthreads();
        const double chalf = G.ch(j == 0 ? 0 : N - 2), den = (G.a * G.w(j)) * (double)n;
        const double vu = (chalf * s_pole[0]) / den, vv = (chalf * s_pole[1]) / den;
        const double zp = j == 0 ? -vu : vu, dp = j == 0 ? vv : -vv;
        for (int i = threadIdx.x; i < n; i += QD_BLOCK) { zr[i] = zp; dr[i] = dp; }
        __syncthreads();
    }
    for (int i = threadIdx.x; i < n; i += QD_BLOCK) { Z[row + i] = zr[i]; D[row + i] = dr[i]; }
    double r0, r1, r2 = 0.0;
    if (wv < 2) {
        const double* x = wv == 0 ? zr : dr;
        r0 = qf_row_sum(x, n, lane); r1 = qf_row_sumsq(x, n, lane); r2 = qf_row_maxabs(x, n, lane);
        if (lane == 0) { rowstat[(3 * wv + 0) * N + j] = r0; rowstat[(3 * wv + 1) * N + j] = r1; rowstat[(3 * wv + 2) * N + j] = r2; }
    } else if (wv == 2) {
        r0 = pole ? 0.0 : qf_row_sum(ke, n, lane);
        if (lane == 0) rowstat[6 * N + j] = r0;
    } else if (lane == 0) {
        rowstat[7 * N + j] = s_bad ? 1.0 : 0.0;
    }
}

// ------------------------------------------------------------------ the forward row transform
// FORM 0: fft, dynamic LDS 4 (QS_SK(n) + 1) doubles; 1: direct, 4 n doubles
template <int FORM>
__global__ void __launch_bounds__(QD_BLOCK)
k_flow_fwd(QdFlowGrid G, QdSpecPlan F, const double* __restrict__ Z, const double* __restrict__ D, double* __restrict__ spec) {
    extern __shared__ double qf_lds[];
    const int n = G.nlon, N = G.nlat, K = G.K, j = blockIdx.x;
    const size_t row = (size_t)j * n, plane = (size_t)N * K, out = (size_t)j * K;
    if (FORM == 0) {
        const int mp = QS_SK(n) + 1;
        double* Ar = qf_lds; double* Ai = Ar + mp; double* Br = Ai + mp; double* Bi = Br + mp;
        for (int t = threadIdx.x; t < n; t += QD_BLOCK) qs_st(Ar, Ai, t, {Z[row + t], D[row + t]});
        __syncthreads();
        double *Xr, *Xi, *Yr, *Yi;
        qs_run(F, n, G.tw, Ar, Ai, Br, Bi, &Xr, &Xi, &Yr, &Yi);
        for (int k = threadIdx.x; k < K; k += QD_BLOCK) {
            const qs_cx y = qs_ld(Xr, Xi, k), c = qs_ld(Xr, Xi, k == 0 ? 0 : n - k);
            spec[out + k] = 0.5 * (y.r + c.r);
            spec[plane + out + k] = 0.5 * (y.i - c.i);
            spec[2 * plane + out + k] = 0.5 * (y.i + c.i);
            spec[3 * plane + out + k] = -0.5 * (y.r - c.r);
        }
    } else {
        double* x0 = qf_lds; double* x1 = x0 + n; double* tc = x1 + n; double* ts = tc + n;
        for (int t = threadIdx.x; t < n; t += QD_BLOCK) { x0[t] = Z[row + t]; x1[t] = D[row + t]; tc[t] = G.tw[t]; ts[t] = G.tw[n + t]; }
        __syncthreads();
        for (int k = threadIdx.x; k < K; k += QD_BLOCK) {
            double zr = 0.0, zi = 0.0, dr = 0.0, di = 0.0;
            int idx = 0;
            for (int i = 0; i < n; ++i) {
                const double cc = tc[idx], ss = ts[idx];
                zr += x0[i] * cc; zi -= x0[i] * ss;
                dr += x1[i] * cc; di -= x1[i] * ss;
                idx += k; if (idx >= n) idx -= n;
            }
            spec[out + k] = zr; spec[plane + out + k] = zi; spec[2 * plane + out + k] = dr; spec[3 * plane + out + k] = di;
        }
    }
}

// ------------------------------------------------------------------ the latitude solve, one thread per (field, k)
__global__ void __launch_bounds__(QD_BLOCK)
k_flow_lat(QdFlowGrid G, const double* __restrict__ rowstat, double* __restrict__ spec, double* __restrict__ cp, double* __restrict__ scal,
           double* __restrict__ rec) {
    extern __shared__ double qf_lds[];
    __shared__ double s_tot[QF_NROW1];
    const int N = G.nlat, K = G.K, lane = threadIdx.x & 63, wv = threadIdx.x >> 6;
    // the first reduction stage across rows: wave 0 zeta (mean, rms, max), 1 delta, 2 the kinetic energy, 3 the bad rows
    if (wv < 2) {
        const double m = qf_cross_mean(G, rowstat + (size_t)(3 * wv) * N, lane), q = qf_cross_mean(G, rowstat + (size_t)(3 * wv + 1) * N, lane);
        const double x = qf_cross(rowstat + (size_t)(3 * wv + 2) * N, N, lane, QD_RED_MAX);
        if (lane == 0) { s_tot[3 * wv] = m; s_tot[3 * wv + 1] = sqrt(q); s_tot[3 * wv + 2] = x; }
    } else if (wv == 2) {
        const double m = qf_cross_mean(G, rowstat + (size_t)6 * N, lane);
        if (lane == 0) s_tot[6] = m;
    } else {
        const double b = qf_cross(rowstat + (size_t)7 * N, N, lane, QD_RED_SUM);
        if (lane == 0) s_tot[7] = b;
    }
    __syncthreads();
    if (blockIdx.x == 0 && threadIdx.x == 0) {
        rec[QD_FLOW_ZETA_MEAN] = s_tot[0]; rec[QD_FLOW_ZETA_RMS] = s_tot[1]; rec[QD_FLOW_ZETA_MAXABS] = s_tot[2];
        rec[QD_FLOW_DIV_MEAN] = s_tot[3]; rec[QD_FLOW_DIV_RMS] = s_tot[4]; rec[QD_FLOW_DIV_MAXABS] = s_tot[5];
        rec[QD_FLOW_KE] = s_tot[6]; rec[QD_FLOW_BAD] = s_tot[7];
        scal[0] = s_tot[7];
    }
    // the row tables of the elimination, once per workgroup: chd | aw | e (dynamic LDS, 3 N doubles)
    double* t_chd = qf_lds; double* t_aw = t_chd + N; double* t_e = t_aw + N;
    for (int j = threadIdx.x; j < N; j += QD_BLOCK) { t_chd[j] = G.chd(j); t_aw[j] = G.aw(j); t_e[j] = G.e(j); }
    __syncthreads();
    const size_t plane = (size_t)N * K;
    if (blockIdx.x == gridDim.x - 1) {
        // k = 0, the last workgroup: lane 0 of wave 0 takes zeta, lane 0 of wave 1 delta.  Three passes in batches of QF_LAT_B rows
        // whose loads are issued together; the chain of a pass is one addition per row (the divisions do not depend on it).
        if (lane != 0 || wv > 1) return;
        const int f = wv;
        double* R = spec + (size_t)(2 * f) * plane;
        double* I = R + plane;
        const double shift = (double)G.nlon * s_tot[3 * f];
        double Fa = 0.0, psi = 0.0, num = 0.0, W = 0.0;
        for (int j0 = 0; j0 < N; j0 += QF_LAT_B) {
            double r[QF_LAT_B];
#pragma unroll
            for (int b = 0; b < QF_LAT_B; ++b) r[b] = j0 + b < N ? R[(size_t)(j0 + b) * K] : 0.0;
#pragma unroll
            for (int b = 0; b < QF_LAT_B; ++b) {
                const int j = j0 + b;
                if (j < N) {
                    Fa = Fa + t_aw[j] * (r[b] - shift);
                    R[(size_t)j * K] = psi; I[(size_t)j * K] = 0.0;
                    const double w = G.w(j);
                    num = num + w * psi; W = W + w;
                    if (j < N - 1) psi = psi + Fa / t_chd[j];
                }
            }
        }
        const double m = num / W;
        for (int j0 = 0; j0 < N; j0 += QF_LAT_B) {
            double r[QF_LAT_B];
#pragma unroll
            for (int b = 0; b < QF_LAT_B; ++b) r[b] = j0 + b < N ? R[(size_t)(j0 + b) * K] : 0.0;
#pragma unroll
            for (int b = 0; b < QF_LAT_B; ++b) if (j0 + b < N) R[(size_t)(j0 + b) * K] = r[b] - m;
        }
        return;
    }
    // k >= 1: Thomas elimination in batches of QF_LAT_B rows; a batch's right sides are loaded while the batch before it is
    // worked on, so the chain (a subtraction, a reciprocal, three multiplies per row) never waits for memory
    const int t = blockIdx.x * QD_BLOCK + threadIdx.x, K1 = K - 1;
    if (t >= 2 * K1) return;
    const int f = t / K1, k = 1 + (t - f * K1);
    double* R = spec + (size_t)(2 * f) * plane + k;
    double* I = R + plane;
    double* C = cp + (size_t)f * plane + k;
    const double lamk = G.lam[k];
    double cpv = 0.0, dr = 0.0, di = 0.0;
    double ar[QF_LAT_B], ai[QF_LAT_B], nr[QF_LAT_B], ni[QF_LAT_B];
#pragma unroll
    for (int b = 0; b < QF_LAT_B; ++b) {
        const int j = 1 + b;
        ar[b] = j < N - 1 ? R[(size_t)j * K] : 0.0; ai[b] = j < N - 1 ? I[(size_t)j * K] : 0.0;
    }
    for (int j0 = 1; j0 < N - 1; j0 += QF_LAT_B) {
#pragma unroll
        for (int b = 0; b < QF_LAT_B; ++b) {
            const int j = j0 + QF_LAT_B + b;
            nr[b] = j < N - 1 ? R[(size_t)j * K] : 0.0; ni[b] = j < N - 1 ? I[(size_t)j * K] : 0.0;
        }
#pragma unroll
        for (int b = 0; b < QF_LAT_B; ++b) {
            const int j = j0 + b;
            if (j < N - 1) {
                const size_t o = (size_t)j * K;
                const double lo = t_chd[j - 1], up = t_chd[j], aw = t_aw[j];
                const double diag = -(up + lo) + t_e[j] * lamk;
                const double inv = 1.0 / (diag - lo * cpv);
                cpv = up * inv;
                dr = (aw * ar[b] - lo * dr) * inv;
                di = (aw * ai[b] - lo * di) * inv;
                C[o] = cpv; R[o] = dr; I[o] = di;
            }
        }
#pragma unroll
        for (int b = 0; b < QF_LAT_B; ++b) { ar[b] = nr[b]; ai[b] = ni[b]; }
    }
    R[(size_t)(N - 1) * K] = 0.0; I[(size_t)(N - 1) * K] = 0.0;
    R[0] = 0.0; I[0] = 0.0;
    double xr = 0.0, xi = 0.0;
    double ac[QF_LAT_B], nc[QF_LAT_B];
#pragma unroll
    for (int b = 0; b < QF_LAT_B; ++b) {
        const int j = N - 2 - b;
        ar[b] = j >= 1 ? R[(size_t)j * K] : 0.0; ai[b] = j >= 1 ? I[(size_t)j * K] : 0.0; ac[b] = j >= 1 ? C[(size_t)j * K] : 0.0;
    }
    for (int j0 = N - 2; j0 >= 1; j0 -= QF_LAT_B) {
#pragma unroll
        for (int b = 0; b < QF_LAT_B; ++b) {
            const int j = j0 - QF_LAT_B - b;
            nr[b] = j >= 1 ? R[(size_t)j * K] : 0.0; ni[b] = j >= 1 ? I[(size_t)j * K] : 0.0; nc[b] = j >= 1 ? C[(size_t)j * K] : 0.0;
        }
#pragma unroll
        for (int b = 0; b < QF_LAT_B; ++b) {
            const int j = j0 - b;
            if (j >= 1) {
                xr = ar[b] - ac[b] * xr; xi = ai[b] - ac[b] * xi;
                R[(size_t)j * K] = xr; I[(size_t)j * K] = xi;
            }
        }
#pragma unroll
        for (int b = 0; b < QF_LAT_B; ++b) { ar[b] = nr[b]; ai[b] = ni[b]; ac[b] = nc[b]; }
    }
}

// ------------------------------------------------------------------ the inverse row transform
// FORM 0: fft, dynamic LDS 4 (QS_SK(n) + 1) doubles; 1: direct, 4 K + 2 n doubles
template <int FORM>
__global__ void __launch_bounds__(QD_BLOCK)
k_flow_inv(QdFlowGrid G, QdSpecPlan F, const double* __restrict__ spec, const double* __restrict__ scal, double* __restrict__ P,
           double* __restrict__ X) {
    extern __shared__ double qf_lds[];
    const int n = G.nlon, N = G.nlat, K = G.K, j = blockIdx.x;
    const size_t row = (size_t)j * n, plane = (size_t)N * K, in = (size_t)j * K;
    const bool bad = scal[0] != 0.0;
    const double dn = (double)n;
    if (FORM == 0) {
        const int mp = QS_SK(n) + 1;
        double* Ar = qf_lds; double* Ai = Ar + mp; double* Br = Ai + mp; double* Bi = Br + mp;
        for (int k = threadIdx.x; k < K; k += QD_BLOCK) {
            const double pr = spec[in + k], pi = spec[plane + in + k], xr = spec[2 * plane + in + k], xi = spec[3 * plane + in + k];
            qs_st(Ar, Ai, k, {pr - xi, -(pi + xr)});                      // conj(psi^ + i chi^)
            if (k > 0 && 2 * k != n) qs_st(Ar, Ai, n - k, {pr + xi, -(xr - pi)});      // ... of the Hermitian partner
        }
        __syncthreads();
        double *Xr, *Xi, *Yr, *Yi;
        qs_run(F, n, G.tw, Ar, Ai, Br, Bi, &Xr, &Xi, &Yr, &Yi);
        for (int i = threadIdx.x; i < n; i += QD_BLOCK) {
            const qs_cx y = qs_ld(Xr, Xi, i);
            P[row + i] = bad ? NAN : y.r / dn;
            X[row + i] = bad ? NAN : -y.i / dn;
        }
    } else {
        double* pr = qf_lds; double* pi = pr + K; double* xr = pi + K; double* xi = xr + K; double* tc = xi + K; double* ts = tc + n;
        for (int k = threadIdx.x; k < K; k += QD_BLOCK) {
            pr[k] = spec[in + k]; pi[k] = spec[plane + in + k]; xr[k] = spec[2 * plane + in + k]; xi[k] = spec[3 * plane + in + k];
        }
        for (int t = threadIdx.x; t < n; t += QD_BLOCK) { tc[t] = G.tw[t]; ts[t] = G.tw[n + t]; }
        __syncthreads();
        for (int i = threadIdx.x; i < n; i += QD_BLOCK) {
            double ap = pr[0], ax = xr[0];
            int idx = 0;
            for (int k = 1; k < K; ++k) {
                idx += i; if (idx >= n) idx -= n;
                const double f = 2 * k == n ? 1.0 : 2.0, cc = tc[idx], ss = ts[idx];
                ap += f * (pr[k] * cc - pi[k] * ss);
                ax += f * (xr[k] * cc - xi[k] * ss);
            }
            P[row + i] = bad ? NAN : ap / dn;
            X[row + i] = bad ? NAN : ax / dn;
        }
    }
}

// ------------------------------------------------------------------ winds, second row partials, sum planes
// dynamic LDS: kr[n], kd[n]
__global__ void __launch_bounds__(QD_BLOCK)
k_flow_finish(QdFlowGrid G, const double* __restrict__ Z, const double* __restrict__ D, const double* __restrict__ P,
              const double* __restrict__ X, double* __restrict__ sums, double* __restrict__ rowstat2) {
    extern __shared__ double qf_lds[];
    __shared__ double sm[4][QD_BLOCK / 64];
    const int n = G.nlon, N = G.nlat, j = blockIdx.x, lane = threadIdx.x & 63, wv = threadIdx.x >> 6;
    double* kr = qf_lds; double* kd = kr + n;
    const bool pole = j == 0 || j == N - 1;
    const size_t row = (size_t)j * n, cells = (size_t)N * n;
    const double ac = G.a * G.c(j);
    double v[4] = {INFINITY, -INFINITY, INFINITY, -INFINITY};
    for (int i = threadIdx.x; i < n; i += QD_BLOCK) {
        const double p = P[row + i], x = X[row + i];
        v[0] = fmin(v[0], p); v[1] = fmax(v[1], p); v[2] = fmin(v[2], x); v[3] = fmax(v[3], x);
        if (!pole) {
            const int ip = i + 1 == n ? 0 : i + 1, im = i == 0 ? n - 1 : i - 1;
            const double dp_dphi = (P[row + n + i] - P[row - n + i]) / (2 * G.dlat), dp_dlam = (P[row + ip] - P[row + im]) / (2 * G.dlon);
            const double dx_dphi = (X[row + n + i] - X[row - n + i]) / (2 * G.dlat), dx_dlam = (X[row + ip] - X[row + im]) / (2 * G.dlon);
            const double ur = -(dp_dphi / G.a), vr = dp_dlam / ac, ud = dx_dlam / ac, vd = dx_dphi / G.a;
            kr[i] = 0.5 * (ur * ur + vr * vr);
            kd[i] = 0.5 * (ud * ud + vd * vd);
        }
        if (sums) {
            sums[row + i] = sums[row + i] + p;
            sums[cells + row + i] = sums[cells + row + i] + x;
            sums[2 * cells + row + i] = sums[2 * cells + row + i] + Z[row + i];
            sums[3 * cells + row + i] = sums[3 * cells + row + i] + D[row + i];
        }
    }
    const QdRedOp ops[4] = {QD_RED_MIN, QD_RED_MAX, QD_RED_MIN, QD_RED_MAX};
    qd_block_gather(sm, v, 4, ops);                         // (its barrier also publishes kr, kd)
    if (threadIdx.x < 4) rowstat2[(size_t)threadIdx.x * N + j] = qd_block_total(sm, threadIdx.x, ops[threadIdx.x]);
    if (wv < 2) {
        const double S = pole ? 0.0 : qf_row_sum(wv == 0 ? kr : kd, n, lane);
        if (lane == 0) rowstat2[(size_t)(4 + wv) * N + j] = S;
    }
}

// one workgroup: wave q takes min / max plane q; waves 0 and 1 then the two energies
__global__ void __launch_bounds__(QD_BLOCK)
k_flow_record(QdFlowGrid G, const double* __restrict__ rowstat2, double* __restrict__ rec) {
    const int N = G.nlat, lane = threadIdx.x & 63, wv = threadIdx.x >> 6;
    const double x = qf_cross(rowstat2 + (size_t)wv * N, N, lane, (wv & 1) ? QD_RED_MAX : QD_RED_MIN);
    if (lane == 0) rec[QD_FLOW_PSI_MIN + wv] = x;
    if (wv < 2) {
        const double m = qf_cross_mean(G, rowstat2 + (size_t)(4 + wv) * N, lane);
        if (lane == 0) rec[QD_FLOW_KE_ROT + wv] = m;
    }
}

// ------------------------------------------------------------------ host side
struct QdFlow {
    int nlat = 0, nlon = 0, K = 0, direct = 0, device = 0;
    double geom[3] = {0, 0, 0};
    QdSpecPlan plan{};
    size_t lds_tr = 0, lds_inv = 0;   // dynamic LDS of k_flow_fwd, k_flow_inv
    double* tab = nullptr;            // [QD_FLOW_TAB][nlat]
    double* lam = nullptr;            // [K]
    double* tw = nullptr;             // [2][nlon]
    double* work = nullptr;           // Z, D, P, X [4][nlat][nlon]
    double* spec = nullptr;           // [4][nlat][K], and behind them the modified upper coefficients [2][nlat][K]
    double* rows = nullptr;           // [QF_NROW1 + QF_NROW2][nlat], then the scalars [8] and a record outside the log [QD_FLOW_REC_W]
    double* sums = nullptr;           // [QD_FLOW_PLANES][nlat][nlon] (handles only)
    double* uv = nullptr;             // [2][nlat][nlon] the host planes of qd_flow_solve, allocated at its first call
    int64_t count = 0;                // samples in the sums
    QdSpanLane lane;
    size_t cells() const { return (size_t)nlat * nlon; }
    double* scal() const { return rows + (size_t)(QF_NROW1 + QF_NROW2) * nlat; }
    double* rec_out() const { return scal() + 8; }
    QdFlowGrid grid() const { return QdFlowGrid{nlat, nlon, K, geom[0], geom[1], geom[2], tab, lam, tw}; }
};

static QdSpanLane* flow_lane(qd_ctx* c) { return c && c->flow ? &c->flow->lane : nullptr; }

static void flow_free(QdFlow* s) {
    void* p[] = {s->tab, s->lam, s->tw, s->work, s->spec, s->rows, s->sums, s->uv, s->lane.log};
    for (void* q : p) if (q) hipFree(q);
    delete s;
}

void qd_flow_release(qd_ctx* c) {
    if (!c->flow) return;
    if (c->stream) hipStreamSynchronize(c->stream);
    flow_free(c->flow);
    c->flow = nullptr;
}

// -> the tables and work planes of a grid on the current device, or nullptr with *why set; with_lane: the log and the sum planes too
static QdFlow* flow_build(int nlat, int nlon, const double* tab, const double* lam, const double* geom, bool with_lane, hipStream_t st,
                          std::string* why) {
    QdFlow* s = new QdFlow();
    s->nlat = nlat; s->nlon = nlon; s->K = nlon / 2 + 1;
    std::memcpy(s->geom, geom, sizeof s->geom);
    const char* form = std::getenv("QD_FLOW_FORM");                   // read here, once, never on the step path
    s->direct = (form && std::strcmp(form, "direct") == 0) || !qd_rowfft_plan(nlon, 1, s->plan) ? 1 : 0;
    s->lds_tr = sizeof(double) * (s->direct ? 4 * (size_t)nlon : 4 * (size_t)(QS_SK(nlon) + 1));
    s->lds_inv = sizeof(double) * (s->direct ? 4 * (size_t)s->K + 2 * (size_t)nlon : 4 * (size_t)(QS_SK(nlon) + 1));
    if (std::max(s->lds_tr, s->lds_inv) > QF_LDS_LIMIT || 3 * (size_t)nlat * sizeof(double) > QF_LDS_LIMIT) {
        *why = "a grid of " + std::to_string(nlat) + " x " + std::to_string(nlon) + " needs " +
               std::to_string(std::max(std::max(s->lds_tr, s->lds_inv), 3 * (size_t)nlat * sizeof(double))) +
               " bytes of LDS, a workgroup may take " + std::to_string(QF_LDS_LIMIT) + " of the CU's 163840";
        delete s;
        return nullptr;
    }
    s->lane.width = QD_FLOW_REC_W;
    s->lane.cap = QD_FLOW_LOG_CAP;
    const std::vector<double> tw = qd_rowfft_table(nlon);
    const size_t cells = s->cells(), sp = (size_t)nlat * s->K;
    const size_t tabb = (size_t)QD_FLOW_TAB * nlat * sizeof(double), lamb = (size_t)s->K * sizeof(double), twb = tw.size() * sizeof(double),
                 workb = 4 * cells * sizeof(double), specb = 6 * sp * sizeof(double),
                 rowsb = ((size_t)(QF_NROW1 + QF_NROW2) * nlat + 8 + QD_FLOW_REC_W) * sizeof(double),
                 logb = s->lane.log_doubles() * sizeof(double), sumb = QD_FLOW_PLANES * cells * sizeof(double);
    bool ok = hipMalloc(&s->tab, tabb) == hipSuccess && hipMalloc(&s->lam, lamb) == hipSuccess && hipMalloc(&s->tw, twb) == hipSuccess &&
              hipMalloc(&s->work, workb) == hipSuccess && hipMalloc(&s->spec, specb) == hipSuccess && hipMalloc(&s->rows, rowsb) == hipSuccess &&
              (!with_lane || (hipMalloc(&s->lane.log, logb) == hipSuccess && hipMalloc(&s->sums, sumb) == hipSuccess));
    ok = ok && hipMemcpyAsync(s->tab, tab, tabb, hipMemcpyHostToDevice, st) == hipSuccess &&
         hipMemcpyAsync(s->lam, lam, lamb, hipMemcpyHostToDevice, st) == hipSuccess &&
         hipMemcpyAsync(s->tw, tw.data(), twb, hipMemcpyHostToDevice, st) == hipSuccess &&
         hipMemsetAsync(s->work, 0, workb, st) == hipSuccess && hipMemsetAsync(s->spec, 0, specb, st) == hipSuccess &&
         hipMemsetAsync(s->rows, 0, rowsb, st) == hipSuccess &&
         (!with_lane || (hipMemsetAsync(s->lane.log, 0, logb, st) == hipSuccess && hipMemsetAsync(s->sums, 0, sumb, st) == hipSuccess)) &&
         hipStreamSynchronize(st) == hipSuccess;          // (tw and the caller's tables are only borrowed)
    // a workgroup may take more than the default 64 KB of dynamic LDS (k_spectra_rows does the same)
    ok = ok && hipFuncSetAttribute((const void*)k_flow_fwd<0>, hipFuncAttributeMaxDynamicSharedMemorySize, QF_LDS_LIMIT) == hipSuccess &&
         hipFuncSetAttribute((const void*)k_flow_fwd<1>, hipFuncAttributeMaxDynamicSharedMemorySize, QF_LDS_LIMIT) == hipSuccess &&
         hipFuncSetAttribute((const void*)k_flow_inv<0>, hipFuncAttributeMaxDynamicSharedMemorySize, QF_LDS_LIMIT) == hipSuccess &&
         hipFuncSetAttribute((const void*)k_flow_inv<1>, hipFuncAttributeMaxDynamicSharedMemorySize, QF_LDS_LIMIT) == hipSuccess &&
         hipFuncSetAttribute((const void*)k_flow_vortdiv, hipFuncAttributeMaxDynamicSharedMemorySize, QF_LDS_LIMIT) == hipSuccess &&
         hipFuncSetAttribute((const void*)k_flow_lat, hipFuncAttributeMaxDynamicSharedMemorySize, QF_LDS_LIMIT) == hipSuccess &&
         hipFuncSetAttribute((const void*)k_flow_finish, hipFuncAttributeMaxDynamicSharedMemorySize, QF_LDS_LIMIT) == hipSuccess;
    if (!ok) { *why = "device allocation or upload failed"; flow_free(s); return nullptr; }
    return s;
}

// QD_LAUNCH_TIMED with dynamic LDS, and without a handle (c == nullptr) a plain launch
#define QF_LAUNCH(c, name, kernel, grid, lds, stream, ...) do { \
    if (c) { QdScope sc(c, name, true); \
        if (sc.on) { sc.used = true; hipExtLaunchKernelGGL((kernel), grid, dim3(QD_BLOCK), lds, stream, sc.e0, sc.e1, 0, __VA_ARGS__); } \
        else hipLaunchKernelGGL((kernel), grid, dim3(QD_BLOCK), lds, stream, __VA_ARGS__); } \
    else hipLaunchKernelGGL((kernel), grid, dim3(QD_BLOCK), lds, stream, __VA_ARGS__); } while (0)

// the six launches of a sample on the device planes (U, V); rec: where the record goes; sums: the sum planes or nullptr
static void flow_run(QdFlow* s, qd_ctx* c, hipStream_t st, const double* U, const double* V, double* rec, double* sums) {
    const QdFlowGrid G = s->grid();
    const size_t cells = s->cells(), sp = (size_t)s->nlat * s->K;
    double *Z = s->work, *D = Z + cells, *P = D + cells, *X = P + cells;
    double *cp = s->spec + 4 * sp, *row1 = s->rows, *row2 = s->rows + (size_t)QF_NROW1 * s->nlat;
    const dim3 rows(s->nlat);
    QF_LAUNCH(c, "flow_vortdiv", k_flow_vortdiv, rows, 3 * (size_t)s->nlon * sizeof(double), st, G, U, V, Z, D, row1);
    if (s->direct) QF_LAUNCH(c, "flow_fwd", k_flow_fwd<1>, rows, s->lds_tr, st, G, s->plan, (const double*)Z, (const double*)D, s->spec);
    else QF_LAUNCH(c, "flow_fwd", k_flow_fwd<0>, rows, s->lds_tr, st, G, s->plan, (const double*)Z, (const double*)D, s->spec);
    QF_LAUNCH(c, "flow_lat", k_flow_lat, dim3((2 * (s->K - 1) + QD_BLOCK - 1) / QD_BLOCK + 1), 3 * (size_t)s->nlat * sizeof(double), st, G, (const double*)row1, s->spec, cp, s->scal(), rec);
    if (s->direct) QF_LAUNCH(c, "flow_inv", k_flow_inv<1>, rows, s->lds_inv, st, G, s->plan, (const double*)s->spec, (const double*)s->scal(), P, X);
    else QF_LAUNCH(c, "flow_inv", k_flow_inv<0>, rows, s->lds_inv, st, G, s->plan, (const double*)s->spec, (const double*)s->scal(), P, X);
    QF_LAUNCH(c, "flow_finish", k_flow_finish, rows, 2 * (size_t)s->nlon * sizeof(double), st, G, (const double*)Z, (const double*)D,
              (const double*)P, (const double*)X, sums, row2);
    QF_LAUNCH(c, "flow_record", k_flow_record, dim3(1), 0, st, G, (const double*)row2, rec);
}

extern "C" int qd_flow_configure(qd_handle c, const double* tab, const double* lam, const double* geom) {
    if (!c || (tab && (!lam || !geom))) return -1;
    if (!qd_whole_globe(c))
        return qd_fail(c, "qd_flow_configure: the flow lane needs a whole-globe handle (world == 1, n_rows == n_lat); "
                          "latitude bands are not supported");
    hipSetDevice(c->desc.device);
    qd_flow_release(c);
    if (!tab) return 0;
    std::string why;
    QdFlow* s = flow_build(c->geo.nlat, c->geo.nlon, tab, lam, geom, true, c->stream, &why);
    if (!s) return qd_fail(c, ("qd_flow_configure: " + why).c_str());
    s->device = c->desc.device;
    c->flow = s;
    return 0;
}

extern "C" int qd_flow_schedule(qd_handle c, int steps, const int32_t* sample) {
    return qd_lane_schedule(c, flow_lane(c), steps, sample, "qd_flow_schedule", "not configured (qd_flow_configure first)");
}
extern "C" int qd_flow_log(qd_handle c, double* out, int max, int* n) {
    return qd_lane_drain(c, flow_lane(c), out, max, n, "qd_flow_log", "not configured (qd_flow_configure first)");
}
extern "C" int qd_flow_reset(qd_handle c) {
    if (!c) return -1;
    QdFlow* s = c->flow;
    if (!s) return qd_fail(c, "qd_flow_reset: not configured (qd_flow_configure first)");
    hipSetDevice(c->desc.device);
    QD_HIP(c, hipMemsetAsync(s->sums, 0, QD_FLOW_PLANES * s->cells() * sizeof(double), c->stream));
    s->count = 0;
    s->lane.reset();
    return 0;
}

extern "C" int qd_flow_sums_get(qd_handle c, double* sums, int64_t* count) {
    if (!c || !count || !sums) return -1;
    QdFlow* s = c->flow;
    if (!s) return qd_fail(c, "qd_flow_sums_get: not configured (qd_flow_configure first)");
    hipSetDevice(c->desc.device);
    QD_HIP(c, hipMemcpyAsync(sums, s->sums, QD_FLOW_PLANES * s->cells() * sizeof(double), hipMemcpyDeviceToHost, c->stream));
    QD_HIP(c, hipStreamSynchronize(c->stream));
    const hipError_t e = hipGetLastError();
    if (e != hipSuccess) return qd_fail(c, "qd_flow_sums_get: kernel", e);
    *count = s->count;
    return 0;
}

extern "C" int qd_flow_sums_set(qd_handle c, const double* sums, int64_t count) {
    if (!c || !sums) return -1;
    QdFlow* s = c->flow;
    if (!s) return qd_fail(c, "qd_flow_sums_set: not configured (qd_flow_configure first)");
    if (count < 0) return qd_fail(c, "qd_flow_sums_set: negative sample count");
    hipSetDevice(c->desc.device);
    QD_HIP(c, hipMemcpyAsync(s->sums, sums, QD_FLOW_PLANES * s->cells() * sizeof(double), hipMemcpyHostToDevice, c->stream));
    QD_HIP(c, hipStreamSynchronize(c->stream));                // the host buffer is only borrowed for the call
    s->count = count;
    return 0;
}

bool qd_flow_planes(const qd_ctx* c, const double** sums, size_t* n) {
    const QdFlow* s = c->flow;
    if (!s) return false;
    *sums = s->sums; *n = QD_FLOW_PLANES * s->cells();
    return true;
}

bool qd_flow_scheduled(const qd_ctx* c) { return c->flow && !c->flow->lane.sched.empty(); }

QdSpanLane* qd_flow_span_begin(qd_ctx* c, int n) {
    static const QdSpanTexts T = {
        "qd_step_n: the flow lane needs a whole-globe handle; latitude bands are not supported",
        "qd_step_n: qd_flow_configure has not been called",
        "qd_step_n: a qd_flow_schedule must cover exactly the n steps of the span",
        "qd_step_n: the span's flow records would overflow the log of QD_FLOW_LOG_CAP (drain it with qd_flow_log first)"};
    QdSpanLane* l = qd_lane_span_begin(c, flow_lane(c), n, T);
    if (!l && c->flow) c->flow->lane.clear_schedule();        // refused: the span guard never sees this lane, and a schedule serves one span
    return l;
}

// a sampled step: U, V as the step leaves them
int qd_flow_step(qd_ctx* c) {
    QdFlow* s = c->flow;
    if (s->lane.full()) return qd_fail(c, "qd_step_n: flow log full (drain it with qd_flow_log)");
    s->count++;
    flow_run(s, c, c->stream, c->f[QD_F_U], c->f[QD_F_V], s->lane.next(), s->sums);
    return 0;
}

extern "C" int qd_flow_sample(qd_handle c) {
    if (!c) return -1;
    if (!c->flow) return qd_fail(c, "qd_flow_sample: not configured (qd_flow_configure first)");
    if (c->flow->lane.full()) return qd_fail(c, "qd_flow_sample: flow log full (drain it with qd_flow_log)");
    hipSetDevice(c->desc.device);
    if (int rc = qd_flow_step(c)) return rc;
    return qd_launch_check(c, "qd_flow_sample");
}

// upload (u, v), run, download the four planes (and the record when rec is a host pointer)
static int flow_solve(QdFlow* s, qd_ctx* c, hipStream_t st, const char* who, const double* u, const double* v, double* const out[4],
                      double* rec_dev, double* rec_host) {
    const size_t cells = s->cells(), pb = cells * sizeof(double);
    if (!s->uv) QD_HIP(c, hipMalloc(&s->uv, 2 * pb));
    QD_HIP(c, hipMemcpyAsync(s->uv, u, pb, hipMemcpyHostToDevice, st));
    QD_HIP(c, hipMemcpyAsync(s->uv + cells, v, pb, hipMemcpyHostToDevice, st));
    flow_run(s, c, st, s->uv, s->uv + cells, rec_dev, nullptr);
    const hipError_t le = hipGetLastError();
    if (le != hipSuccess) return qd_fail(c, (std::string(who) + ": launch").c_str(), le);
    for (int q = 0; q < 4; ++q)                               // the work planes Z, D, P, X are zeta, delta, psi, chi
        QD_HIP(c, hipMemcpyAsync(out[q], s->work + (size_t)q * cells, pb, hipMemcpyDeviceToHost, st));
    if (rec_host) QD_HIP(c, hipMemcpyAsync(rec_host, rec_dev, QD_FLOW_REC_W * sizeof(double), hipMemcpyDeviceToHost, st));
    QD_HIP(c, hipStreamSynchronize(st));
    const hipError_t e = hipGetLastError();
    if (e != hipSuccess) return qd_fail(c, (std::string(who) + ": kernel").c_str(), e);
    return 0;
}

extern "C" int qd_flow_solve(qd_handle c, const double* u, const double* v, double* zeta, double* delta, double* psi, double* chi) {
    if (!c || !u || !v || !zeta || !delta || !psi || !chi) return -1;
    QdFlow* s = c->flow;
    if (!s) return qd_fail(c, "qd_flow_solve: not configured (qd_flow_configure first)");
    if (s->lane.full()) return qd_fail(c, "qd_flow_solve: flow log full (drain it with qd_flow_log)");
    hipSetDevice(c->desc.device);
    double* const out[4] = {zeta, delta, psi, chi};
    return flow_solve(s, c, c->stream, "qd_flow_solve", u, v, out, s->lane.next(), nullptr);
}

extern "C" int qd_flow_solve_grid(int n_lat, int n_lon, int device, const double* tab, const double* lam, const double* geom, const double* u,
                                  const double* v, double* zeta, double* delta, double* psi, double* chi, double* rec) {
    if (!tab || !lam || !geom || !u || !v || !zeta || !delta || !psi || !chi || !rec) return qd_fail(nullptr, "qd_flow_solve_grid: null argument");
    if (n_lat < 3 || n_lon < 4) return qd_fail(nullptr, "qd_flow_solve_grid: grid too small (need n_lat>=3, n_lon>=4)");
    int ndev = 0;
    if (hipGetDeviceCount(&ndev) != hipSuccess || ndev == 0) return qd_fail(nullptr, "qd_flow_solve_grid: no HIP device visible");
    if (device < 0 || device >= ndev) return qd_fail(nullptr, "qd_flow_solve_grid: bad device ordinal");
    hipError_t e;
    if ((e = hipSetDevice(device)) != hipSuccess) return qd_fail(nullptr, "qd_flow_solve_grid: hipSetDevice", e);
    hipStream_t st = nullptr;
    if ((e = hipStreamCreate(&st)) != hipSuccess) return qd_fail(nullptr, "qd_flow_solve_grid: hipStreamCreate", e);
    std::string why;
    QdFlow* s = flow_build(n_lat, n_lon, tab, lam, geom, false, st, &why);
    int rc = s ? 0 : qd_fail(nullptr, ("qd_flow_solve_grid: " + why).c_str());
    if (s) {
        double* const out[4] = {zeta, delta, psi, chi};
        rc = flow_solve(s, nullptr, st, "qd_flow_solve_grid", u, v, out, s->rec_out(), rec);
        hipStreamSynchronize(st);
        flow_free(s);
    }
    hipStreamDestroy(st);
    return rc;
}

// ---- the vorticity / divergence launch for another lane (qd_spharm.hip: its VORT and DIV entries), on that lane's own buffers: tab
// [QD_FLOW_TAB][nlat] on the device, geom {a, dlat, dlon}, Z and D [nlat][nlon], rowstat [QF_NROW1][nlat].  prepare: once, at that
// lane's configure time (a row of 3 nlon doubles may need more than the default 64 KB of dynamic LDS).
bool qd_flow_vortdiv_prepare(size_t lds_limit) {
    return hipFuncSetAttribute((const void*)k_flow_vortdiv, hipFuncAttributeMaxDynamicSharedMemorySize, (int)lds_limit) == hipSuccess;
}
void qd_flow_vortdiv_launch(qd_ctx* c, hipStream_t st, int nlat, int nlon, const double* tab, const double* geom, const double* U, const double* V,
                            double* Z, double* D, double* rowstat) {
    const QdFlowGrid G{nlat, nlon, nlon / 2 + 1, geom[0], geom[1], geom[2], tab, nullptr, nullptr};
    QF_LAUNCH(c, "spharm_vortdiv", k_flow_vortdiv, dim3(nlat), 3 * (size_t)nlon * sizeof(double), st, G, U, V, Z, D, rowstat);
}
