// qd_blockred.h -- the wave and workgroup reductions of the QD_BLOCK kernels, defined once (device side, gfx950: 64 lanes).
//
// SUMMATION ORDER IS THE INVARIANT.  Every result below is a fixed function of its inputs and of the launch shape:
//   wave       five __shfl_down halvings (32, 16, 8, 4, 2, 1); the result is valid in lane 0
//   workgroup  lane 0 of every wave -> LDS, one barrier, the QD_BLOCK / 64 wave results combined one after the other from wave 0
//   stage 2    a plane of per-workgroup partials either block-strided (k = tid, tid + QD_BLOCK, ...; then the workgroup tail) or
//              with one wave per plane (k = lane, lane + 64, ...; then the wave sum)
// A kernel that moves from one form to another changes its bits.  Not shared on purpose: qr_block_sum (qd_route.hip: its own block
// size and LDS tree), qd_pd_pow (qd_phyto_daily.hip: only the 0.5 shortcut) and the multi-value shuffle loops written inline.
#pragma once
#include "qd_internal.h"

__device__ __forceinline__ double qd_wave_sum(double x) {
#pragma unroll
    for (int o = 32; o > 0; o >>= 1) x += __shfl_down(x, o, 64);
    return x;
}
__device__ __forceinline__ double qd_wave_max(double x) {        // compare form: a NaN never replaces x
#pragma unroll
    for (int o = 32; o > 0; o >>= 1) { double y = __shfl_down(x, o, 64); x = (y > x) ? y : x; }
    return x;
}
__device__ __forceinline__ double qd_wave_fmin(double x) {       // fmin / fmax form: a NaN operand is dropped
#pragma unroll
    for (int o = 32; o > 0; o >>= 1) x = fmin(x, __shfl_down(x, o, 64));
    return x;
}
__device__ __forceinline__ double qd_wave_fmax(double x) {
#pragma unroll
    for (int o = 32; o > 0; o >>= 1) x = fmax(x, __shfl_down(x, o, 64));
    return x;
}

// ---- the integer family (qd_digest.hip): sums mod 2^64.  Integer addition is associative, so unlike everything above the result
// does NOT depend on the form, the launch shape or the order in which workgroups arrive.
//   wave       the same five halvings, the 64-bit value moved as its two 32-bit halves (a DPP / permute lane move is 32 bits wide)
//   workgroup  lane 0 of every wave -> LDS, one barrier, thread 0 adds the QD_BLOCK / 64 wave results; valid in thread 0
__device__ __forceinline__ unsigned long long qd_wave_sum_u64(unsigned long long x) {
#pragma unroll
    for (int o = 32; o > 0; o >>= 1) {
        const unsigned int lo = __shfl_down((unsigned int)x, o, 64), hi = __shfl_down((unsigned int)(x >> 32), o, 64);
        x += ((unsigned long long)hi << 32) | (unsigned long long)lo;
    }
    return x;
}
__device__ __forceinline__ unsigned long long qd_block_sum_u64(unsigned long long x) {      // every thread of the workgroup calls it
    __shared__ unsigned long long sm[QD_BLOCK / 64];
    const int lane = threadIdx.x & 63, wv = threadIdx.x >> 6;
    x = qd_wave_sum_u64(x);
    if (lane == 0) sm[wv] = x;
    __syncthreads();
    if (threadIdx.x == 0)
        for (int k = 1; k < QD_BLOCK / 64; ++k) x += sm[k];
    return x;
}

// x ** e as NumPy evaluates it for a scalar exponent: 1, 2 and 0.5 take its exact fast paths
__device__ __forceinline__ double qd_pow_np(double x, double e) {
    return e == 1.0 ? x : (e == 2.0 ? x * x : (e == 0.5 ? sqrt(x) : pow(x, e)));
}

// ---- N quantities of one workgroup, each a sum, an fmin or an fmax.  `op`: one entry per quantity, nullptr = all sums
enum QdRedOp { QD_RED_SUM = 0, QD_RED_MIN, QD_RED_MAX };
__device__ __forceinline__ QdRedOp qd_red_op(const QdRedOp* op, int q) { return op ? op[q] : QD_RED_SUM; }
__device__ __forceinline__ double qd_red_identity(QdRedOp op) { return op == QD_RED_SUM ? 0.0 : (op == QD_RED_MIN ? INFINITY : -INFINITY); }
__device__ __forceinline__ double qd_red_join(double a, double b, QdRedOp op) {
    return op == QD_RED_SUM ? a + b : (op == QD_RED_MIN ? fmin(a, b) : fmax(a, b));
}
__device__ __forceinline__ double qd_red_wave(double x, QdRedOp op) {
    return op == QD_RED_SUM ? qd_wave_sum(x) : (op == QD_RED_MIN ? qd_wave_fmin(x) : qd_wave_fmax(x));
}

// the tail every form shares: wave-reduce v[0 .. count), lane 0 -> sm[q][wave], barrier.  Every thread of the workgroup calls it.
template <int N>
__device__ __forceinline__ void qd_block_gather(double (&sm)[N][QD_BLOCK / 64], const double (&v)[N], int count, const QdRedOp* op) {
    const int lane = threadIdx.x & 63, wv = threadIdx.x >> 6;
#pragma unroll
    for (int q = 0; q < N; ++q)
        if (q < count) {
            const double r = qd_red_wave(v[q], qd_red_op(op, q));
            if (lane == 0) sm[q][wv] = r;
        }
    __syncthreads();
}
template <int N>
__device__ __forceinline__ double qd_block_total(const double (&sm)[N][QD_BLOCK / 64], int q, QdRedOp op) {
    double r = sm[q][0];
    for (int k = 1; k < QD_BLOCK / 64; ++k) r = qd_red_join(r, sm[q][k], op);
    return r;
}

// stage 1: thread q < count stores the workgroup's value of quantity q to partial[q * nblk + b] (b: this workgroup of nblk)
template <int N>
__device__ __forceinline__ void qd_block_partials(const double (&v)[N], int count, const QdRedOp* op, double* __restrict__ partial,
                                                  size_t nblk, size_t b) {
    __shared__ double sm[N][QD_BLOCK / 64];
    qd_block_gather(sm, v, count, op);
    const int q = threadIdx.x;
    if (q < count) partial[(size_t)q * nblk + b] = qd_block_total(sm, q, qd_red_op(op, q));
}

// stage 2, block-strided: v[q] = this thread's share of plane q < planes (a one-workgroup kernel; the caller may add quantities of
// its own behind them); then qd_block_totals leaves the N workgroup totals in thread 0's v
template <int N>
__device__ __forceinline__ void qd_planes_strided(const double* __restrict__ partial, int nblk, int planes, const QdRedOp* op, double (&v)[N]) {
#pragma unroll
    for (int q = 0; q < N; ++q)
        if (q < planes) {
            const QdRedOp o = qd_red_op(op, q);
            double a = qd_red_identity(o);
            for (int k = threadIdx.x; k < nblk; k += QD_BLOCK) a = qd_red_join(a, partial[(size_t)q * nblk + k], o);
            v[q] = a;
        }
}
template <int N>
__device__ __forceinline__ void qd_block_totals(double (&v)[N], const QdRedOp* op) {
    __shared__ double sm[N][QD_BLOCK / 64];
    qd_block_gather(sm, v, N, op);
    if (threadIdx.x == 0)
        for (int q = 0; q < N; ++q) v[q] = qd_block_total(sm, q, qd_red_op(op, q));
}

// stage 2, one wave per plane: tot[q] (LDS, [planes]) = the sum of plane q, lanes strided over its nblk partials; every thread of
// the workgroup may read tot on return
__device__ __forceinline__ void qd_planes_by_wave(const double* __restrict__ partial, int nblk, int planes, double* tot) {
    const int lane = threadIdx.x & 63, wv = threadIdx.x >> 6;
    for (int q = wv; q < planes; q += QD_BLOCK / 64) {
        double a = 0.0;
        for (int k = lane; k < nblk; k += 64) a += partial[(size_t)q * nblk + k];
        a = qd_wave_sum(a);
        if (lane == 0) tot[q] = a;
    }
    __syncthreads();
}

// ---- the two scalars of the precipitation renormalisation from the row partials of k_precip_raw (partial[0 .. n) = sum Pq w,
// partial[n .. 2n) = sum P_raw w): out[0] = s = num / den, out[1] = blend weight of the legacy field (p_blend when <Pq> < pq_min and
// the fallback is on, else 0).  One workgroup of QD_BLOCK threads; block-strided shares, wave sums, thread 0 adds the wave results
// from wave 0 on.  k_precip_scalars (one workgroup) and the precipitation k_gauss_pair (every workgroup for itself) both call it:
// one order, one result.  out: LDS or global; every thread may read an LDS out on return.
__device__ __forceinline__ void qd_precip_scalars_wg(const double* __restrict__ partial, int n, double wsum, double pq_min, double p_blend,
                                                     int use_fb, double* out) {
    __shared__ double sm[2][QD_BLOCK / 64];
    double a = 0.0, b = 0.0;
    for (int k = threadIdx.x; k < n; k += QD_BLOCK) { a += partial[k]; b += partial[n + k]; }
    a = qd_wave_sum(a); b = qd_wave_sum(b);
    const int lane = threadIdx.x & 63, wv = threadIdx.x >> 6;
    if (lane == 0) { sm[0][wv] = a; sm[1][wv] = b; }
    __syncthreads();
    if (threadIdx.x == 0) {
        for (int k = 1; k < QD_BLOCK / 64; ++k) { a += sm[0][k]; b += sm[1][k]; }
        const double den = b + 1e-20;
        out[0] = den > 0 ? a / den : 1.0;
        const double pq_mean = a / (wsum + 1e-15);
        out[1] = (use_fb && pq_mean < pq_min) ? p_blend : 0.0;
    }
    __syncthreads();
}
