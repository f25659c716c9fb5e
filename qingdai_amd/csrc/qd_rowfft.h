// qd_rowfft.h -- the f64 row FFT in LDS that the spectra lane (qd_spectra.hip) and the flow lane (qd_flow.hip) share, gfx950.
//
// A complex sequence of length m = 2^a 3^b 5^c is transformed (forward: exp(-2 pi i ...)) by a Stockham autosort FFT with radix
// 4 / 2 / 3 / 5 passes between two LDS buffers: the pass with radix r, sub-length L and stride s = m / L has butterfly b = p s + q
// read src[b + t m / r], t < r, and write dst[q + s (r p + u)] = (sum_t a_t w_r^(t u)) w_L^(p u); one barrier per pass, which the
// caller places.  Re and Im live in arrays of their own (8-byte elements) and element i sits at QS_SK(i) = i + (i >> 5), one pad
// per 32 (the conflict analysis and the measurement behind the pad: the top of qd_spectra.hip).  The twiddles come from ONE table
// cos / sin(2 pi t / n), t = 0 .. n - 1, of a length n = m step, built on the host in extended precision.  An inverse transform is
// the forward one between two conjugations.  The order of every sum is fixed: the same input gives the same bits, run after run.
#pragma once
#include "qd_internal.h"
#include <cmath>
#include <vector>

#define QD_SPEC_MAX_PASSES 16
struct QdSpecPlan { int m, step, even, nf; int r[QD_SPEC_MAX_PASSES]; };               // fft: length, table step n / m, n even, the passes

#ifndef QD_SPEC_SKEW_SHIFT
#define QD_SPEC_SKEW_SHIFT 5          // one 8-byte pad per 32 elements
#endif
#define QS_SK(i) ((i) + ((i) >> QD_SPEC_SKEW_SHIFT))

struct qs_cx { double r, i; };
__device__ __forceinline__ qs_cx qs_add(qs_cx a, qs_cx b) { return {a.r + b.r, a.i + b.i}; }
__device__ __forceinline__ qs_cx qs_sub(qs_cx a, qs_cx b) { return {a.r - b.r, a.i - b.i}; }
__device__ __forceinline__ qs_cx qs_mul(qs_cx a, qs_cx w) { return {a.r * w.r - a.i * w.i, a.r * w.i + a.i * w.r}; }
__device__ __forceinline__ qs_cx qs_mji(qs_cx a) { return {a.i, -a.r}; }               // a * (-i)
__device__ __forceinline__ qs_cx qs_scale(qs_cx a, double f) { return {a.r * f, a.i * f}; }
__device__ __forceinline__ qs_cx qs_tw(const double* __restrict__ tw, int n, int idx) { return {tw[idx], -tw[n + idx]}; }   // exp(-2 pi i idx / n)
__device__ __forceinline__ qs_cx qs_ld(const double* re, const double* im, int i) { const int k = QS_SK(i); return {re[k], im[k]}; }
__device__ __forceinline__ void qs_st(double* re, double* im, int i, qs_cx v) { const int k = QS_SK(i); re[k] = v.r; im[k] = v.i; }

// one Stockham pass of radix R over the whole sequence (every thread of the workgroup; the caller's barrier follows)
template <int R>
__device__ __forceinline__ void qs_pass(const double* sr, const double* si, double* dr, double* di, int m, int s, int step, int n,
                                        const double* __restrict__ tw) {
    const int nb = m / R;                                   // butterflies; the sub-length is L = m / s, L / R = nb / s
    const bool last = nb == s;                              // L == R: p == 0 everywhere, every twiddle is 1
    for (int b = threadIdx.x; b < nb; b += QD_BLOCK) {
        const int p = b / s, q = b - p * s;
        qs_cx a[R], y[R];
#pragma unroll
        for (int t = 0; t < R; ++t) a[t] = qs_ld(sr, si, b + t * nb);
        if (R == 2) {
            y[0] = qs_add(a[0], a[1]); y[1] = qs_sub(a[0], a[1]);
        } else if (R == 4) {
            const qs_cx t0 = qs_add(a[0], a[2]), t1 = qs_sub(a[0], a[2]), t2 = qs_add(a[1], a[3]), t3 = qs_mji(qs_sub(a[1], a[3]));
            y[0] = qs_add(t0, t2); y[1] = qs_add(t1, t3); y[2] = qs_sub(t0, t2); y[3] = qs_sub(t1, t3);
        } else if (R == 3) {
            const double h = 0.86602540378443864676;        // sin(2 pi / 3)
            const qs_cx sm = qs_add(a[1], a[2]), d = qs_scale(qs_mji(qs_sub(a[1], a[2])), h);
            const qs_cx md = qs_sub(a[0], qs_scale(sm, 0.5));
            y[0] = qs_add(a[0], sm); y[1] = qs_add(md, d); y[2] = qs_sub(md, d);
        } else {
            const double c1 = 0.30901699437494742410, c2 = -0.80901699437494742410;     // cos(2 pi / 5), cos(4 pi / 5)
            const double s1 = 0.95105651629515357212, s2 = 0.58778525229247312917;      // sin(2 pi / 5), sin(4 pi / 5)
            const qs_cx s14 = qs_add(a[1], a[4]), d14 = qs_sub(a[1], a[4]), s23 = qs_add(a[2], a[3]), d23 = qs_sub(a[2], a[3]);
            const qs_cx m1 = qs_add(a[0], qs_add(qs_scale(s14, c1), qs_scale(s23, c2)));
            const qs_cx m2 = qs_add(a[0], qs_add(qs_scale(s14, c2), qs_scale(s23, c1)));
            const qs_cx n1 = qs_mji(qs_add(qs_scale(d14, s1), qs_scale(d23, s2)));
            const qs_cx n2 = qs_mji(qs_sub(qs_scale(d14, s2), qs_scale(d23, s1)));
            y[0] = qs_add(a[0], qs_add(s14, s23));
            y[1] = qs_add(m1, n1); y[4] = qs_sub(m1, n1); y[2] = qs_add(m2, n2); y[3] = qs_sub(m2, n2);
        }
        const int o = q + s * R * p, base = p * s * step;   // u base < m step = n: no wrap
        qs_st(dr, di, o, y[0]);
#pragma unroll
        for (int u = 1; u < R; ++u) qs_st(dr, di, o + s * u, last ? y[u] : qs_mul(y[u], qs_tw(tw, n, u * base)));
    }
}

// every pass of the plan, each behind a barrier of its own, from (ar, ai) with (br, bi) as the second buffer; the caller has
// synchronised the loads.  -> the transform sits in (*xr, *xi), the other buffer in (*yr, *yi).  Every thread of the workgroup.
__device__ __forceinline__ void qs_run(const QdSpecPlan& F, int n, const double* __restrict__ tw, double* ar, double* ai, double* br,
                                       double* bi, double** xr, double** xi, double** yr, double** yi) {
    double *sr = ar, *si = ai, *dr = br, *di = bi;
    int s = 1;
    for (int f = 0; f < F.nf; ++f) {
        const int r = F.r[f];
        if (r == 4) qs_pass<4>(sr, si, dr, di, F.m, s, F.step, n, tw);
        else if (r == 2) qs_pass<2>(sr, si, dr, di, F.m, s, F.step, n, tw);
        else if (r == 3) qs_pass<3>(sr, si, dr, di, F.m, s, F.step, n, tw);
        else qs_pass<5>(sr, si, dr, di, F.m, s, F.step, n, tw);
        __syncthreads();
        double* t0 = sr; sr = dr; dr = t0;
        t0 = si; si = di; di = t0;
        s *= r;
    }
    *xr = sr; *xi = si; *yr = dr; *yi = di;
}

// host: m = 2^a 3^b 5^c -> the radix list of the length-m transform (4s first) on a table of m * step entries, or false
inline bool qd_rowfft_plan(int m, int step, QdSpecPlan& F) {
    F.m = m; F.step = step; F.nf = 0;
    const int radix[] = {4, 2, 3, 5};
    for (int r : radix)
        while (m % r == 0) { if (F.nf == QD_SPEC_MAX_PASSES) return false; F.r[F.nf++] = r; m /= r; }
    return m == 1;
}

// host: cos / sin(2 pi t / n), t = 0 .. n - 1, as [2][n], rounded once from long double
inline std::vector<double> qd_rowfft_table(int n) {
    std::vector<double> tw(2 * (size_t)n);
    for (int k = 0; k < n; ++k) {
        const long double ang = 2.0L * 3.14159265358979323846264338327950288L * (long double)k / (long double)n;
        tw[k] = (double)cosl(ang); tw[n + k] = (double)sinl(ang);
    }
    return tw;
}
