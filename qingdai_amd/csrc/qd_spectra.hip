// qd_spectra.hip -- zonal wavenumber spectra: the one-sided variance spectrum of every latitude row of selected fields, one record
// per sampled step, as a span lane, gfx950 (QD_SPECTRA).
//
// An entry is what a history entry is (qd_entry.h): an f64 plane (op 0) or sqrt(a*a + b*b) of two planes (op 1).  For a row x[i],
// i = 0 .. n - 1 (n = n_lon), X(k) = sum_i x[i] exp(-2 pi i ik / n) for k = 0 .. kN = n / 2 (n_bins = kN + 1) and
//     P_j(k) = c_k (Re X(k)^2 + Im X(k)^2) / n^2        c_k = 1 for k = 0 and for k = n / 2 of an even n, 2 otherwise
// (Parseval: sum_k P_j(k) is the zonal mean of x^2).  The global spectrum is P(k) = sum_j w_j P_j(k) / sum_j w_j with the host's
// w_j = max(cos lat_j, 0).  A row that holds a non-finite value gives NaN in every bin of the row and of P, and is counted.  The n
// entries' results, in configure order, are ONE record of n (n_bins + QD_SPECTRA_STATS) doubles -- per entry P(0 .. kN), then the
// count of non-finite rows -- in the lane's device log, which holds QD_SPECTRA_LOG_CAP records between two drains (qd_spectra_log).
// With lat_resolved the per-row powers are also added into resident sum planes [entry][n_lat][n_bins] (sum = sum + P, one thread
// per cell, from +0.0), which the host reads with their sample count (qd_spectra_sums_get) and divides.  No flag bit: a schedule
// given before the span turns the lane on.  Groups and sampling places are history's: the entries that read PRECIP in front of the
// ocean step, every other entry behind the step's last launch.  A sampling position is two launches, k_spectra_rows and
// k_spectra_combine; an unsampled step launches nothing.  Whole-globe handles only.
//
// k_spectra_rows: ONE workgroup of QD_BLOCK threads per (entry, row), the row read once and staged in LDS; the twiddles come from
// the one table cos / sin(2 pi t / n), t = 0 .. n - 1, built at configure time in extended precision (as c->zonal_tw is built).
//   fft     n = 2^a 3^b 5^c.  An even n is packed as the complex sequence z[t] = x[2t] + i x[2t + 1] of length m = n / 2 (an odd n
//           as z[t] = x[t], m = n), transformed by a Stockham autosort FFT with radix 4 / 2 / 3 / 5 passes between two LDS buffers
//           (pass with radix r, sub-length L, stride s = m / L: butterfly b = p s + q reads src[b + t m / r], t < r, and writes
//           dst[q + s (r p + u)] = (sum_t a_t w_r^(t u)) w_L^(p u); one barrier per pass), and an even n is separated by
//           X(k) = (Z(k) + conj Z(m - k)) / 2 + w_n^k (Z(k) - conj Z(m - k)) / (2i).  Re and Im live in arrays of their own (8-byte
//           elements) and element i sits at i + (i >> 5), one pad per 32.  The reads of a pass are unit-stride (conflict-free but
//           where a group of lanes crosses a pad).  An 8-byte LDS store is served 16 lanes at a time over 16 eight-byte slots: the
//           stride-4 stores of a first radix-4 pass (s = 1) are a four-way conflict unpadded and two-way with the pad, stride 2 is
//           two-way either way, strides 3 and 5 are conflict-free; the second pass (s = r) stores runs of r and is up to four-way,
//           passes with s >= 16 store whole runs of 16 and are conflict-free.  Measured at 721 x 1440 (4 4 3 3 5), the kernel
//           takes 0.0458 ms with this pad, 0.0459 ms with one pad per 16 and 0.0456 ms with none (-DQD_SPEC_SKEW_SHIFT=4 / 30):
//           the LDS conflicts that remain do not bound it, so no finer layout was built.  LDS: 32 (m + m / 32 + 1) + 8 bytes.
//   direct  any n (and every n under QD_SPECTRA_FORM=direct, read once at configure time): the row and the table in LDS (24 n
//           bytes), thread k takes the bins k, k + QD_BLOCK, ... and adds x[i] cos / sin(2 pi ((i k) mod n) / n) for i ascending.
// Several rows are in flight per CU by occupancy (n = 1440: 23.8 KB of LDS, six workgroups per CU; n = 2880: 47.6 KB, three).
// No scratch, no atomics: the same planes give the same bits in either form, run after run.
// k_spectra_combine: per (entry, bin) lane l of 64 takes the rows l, l + 64, ... in ascending order, num = num + w_j P_j(k) (the
// product rounded), W = W + w_j, both from +0.0; then the five halvings of qd_blockred.h (here through LDS, x[l] = x[l] + x[l + o]
// for l < o, o = 32 .. 1: what lane 0 of the shuffle form holds) and P(k) = num / W.  A workgroup is 64 lanes x 4 neighbouring
// bins, so a wave reads 32-byte runs of 16 rows.  spectra.combine_reference restates it in NumPy, bit for bit.
#include "qd_span.h"
#include "qd_entry.h"
#include "qd_blockred.h"
#include "qd_rowfft.h"
#include <algorithm>
#include <cmath>
#include <cstdlib>
#include <cstring>

#define QD_SPEC_NSTAT 1                 // the count of non-finite rows behind an entry's bins (include/qingdai_hip.h: QD_SPECTRA_STATS)
#define QD_SPEC_LDS_LIMIT (150 * 1024)  // bytes of the CU's 160 KB LDS one workgroup may take here (k_zonal_filter's limit)
#define QD_SPEC_CBINS 4                 // bins per k_spectra_combine workgroup
#define QD_SPEC_CROUNDS 4               // rows per lane whose loads are in flight together
static_assert(QD_SPECTRA_MAX_ENTRIES == QD_ENTRY_MAX, "the spectra table is the shared entry table");
static_assert(QD_SPECTRA_STATS == QD_SPEC_NSTAT, "the record's trailing statistics");
static_assert(QD_BLOCK == 64 * QD_SPEC_CBINS, "k_spectra_combine: 64 lanes x QD_SPEC_CBINS bins");

struct QdSpecEntry { const double* a; const double* b; int slot; int pad_; };          // b == nullptr: op 0; slot: the entry's place in the record
struct QdSpecTab { QdSpecEntry e[QD_ENTRY_MAX]; int n; };

// qs_cx, QS_SK, qs_ld / qs_st, qs_pass and QdSpecPlan: qd_rowfft.h, shared with the flow lane

// FORM 0: fft, 1: direct.  Dynamic LDS: one flag word of 8 bytes, then the form's arrays.
template <int FORM>
__global__ void __launch_bounds__(QD_BLOCK)
k_spectra_rows(QdSpecTab T, QdSpecPlan F, int nlat, int n, const double* __restrict__ tw, double* __restrict__ rows,
               double* __restrict__ bad, double* __restrict__ sums) {
    extern __shared__ double qs_lds[];
    int* flag = reinterpret_cast<int*>(qs_lds);
    const int q = blockIdx.x / nlat, j = blockIdx.x - q * nlat, kN = n / 2, nbins = kN + 1;
    const QdSpecEntry E = T.e[q];
    const bool pair = E.b != nullptr;
    const size_t row = (size_t)j * n;
    const double* pa = E.a + row;
    const double* pb = pair ? E.b + row : pa;
    if (threadIdx.x == 0) *flag = 0;
    __syncthreads();
    int nonfinite = 0;
    const double* Xr;
    const double* Xi;
    double *xr, *xi;
    if (FORM == 0) {
        const int m = F.m, mp = QS_SK(m) + 1;
        double* Ar = qs_lds + 1; double* Ai = Ar + mp; double* Br = Ai + mp; double* Bi = Br + mp;
        if (F.even) {                                       // the row starts 16-byte aligned: every plane is an allocation of its own
            for (int t = threadIdx.x; t < m; t += QD_BLOCK) {
                const double2 u = *reinterpret_cast<const double2*>(pa + 2 * t);
                double2 v = u;
                if (pair) v = *reinterpret_cast<const double2*>(pb + 2 * t);
                const double x0 = hist_value(u.x, v.x, pair), x1 = hist_value(u.y, v.y, pair);
                nonfinite |= (!(fabs(x0) <= 1.7976931348623157e308) || !(fabs(x1) <= 1.7976931348623157e308)) ? 1 : 0;
                qs_st(Ar, Ai, t, {x0, x1});
            }
        } else {
            for (int t = threadIdx.x; t < m; t += QD_BLOCK) {
                const double x0 = hist_value(pa[t], pb[t], pair);
                nonfinite |= !(fabs(x0) <= 1.7976931348623157e308) ? 1 : 0;
                qs_st(Ar, Ai, t, {x0, 0.0});
            }
        }
        if (nonfinite) *flag = 1;                           // (every writer stores the same value)
        __syncthreads();
        double *sr = Ar, *si = Ai, *dr = Br, *di = Bi;
        int s = 1;
        for (int f = 0; f < F.nf; ++f) {
            const int r = F.r[f];
            if (r == 4) qs_pass<4>(sr, si, dr, di, m, s, F.step, n, tw);
            else if (r == 2) qs_pass<2>(sr, si, dr, di, m, s, F.step, n, tw);
            else if (r == 3) qs_pass<3>(sr, si, dr, di, m, s, F.step, n, tw);
            else qs_pass<5>(sr, si, dr, di, m, s, F.step, n, tw);
            __syncthreads();
            double* t0 = sr; sr = dr; dr = t0;
            t0 = si; si = di; di = t0;
            s *= r;
        }
        Xr = sr; Xi = si; xr = dr; xi = di;
    } else {
        double* x = qs_lds + 1; double* tc = x + n; double* ts = tc + n;
        for (int t = threadIdx.x; t < n; t += QD_BLOCK) {
            const double x0 = hist_value(pa[t], pb[t], pair);
            nonfinite |= !(fabs(x0) <= 1.7976931348623157e308) ? 1 : 0;
            x[t] = x0; tc[t] = tw[t]; ts[t] = tw[n + t];
        }
        if (nonfinite) *flag = 1;
        __syncthreads();
        Xr = x; Xi = tc; xr = ts; xi = nullptr;
    }
    const bool isbad = *flag != 0;                          // workgroup-uniform
    const double nn = (double)n * (double)n;
    const size_t out = ((size_t)E.slot * nlat + j) * nbins;     // rows, bad and sums are indexed by the entry's place in the record
    for (int k = threadIdx.x; k < nbins; k += QD_BLOCK) {
        double re, im;
        if (FORM == 0) {
            if (F.even) {
                const int m = F.m, k0 = k == m ? 0 : k, k1 = k == 0 ? 0 : m - k;
                const qs_cx z = qs_ld(Xr, Xi, k0), c = qs_ld(Xr, Xi, k1);       // conj Z(m - k) = (c.r, -c.i)
                const double er = 0.5 * (z.r + c.r), ei = 0.5 * (z.i - c.i), orr = 0.5 * (z.i + c.i), oi = -0.5 * (z.r - c.r);
                const double wc = tw[k], ws = tw[n + k];                          // w_n^k = wc - i ws
                re = er + (wc * orr + ws * oi);
                im = ei + (wc * oi - ws * orr);
            } else {
                const qs_cx z = qs_ld(Xr, Xi, k);
                re = z.r; im = z.i;
            }
        } else {
            const double *x = Xr, *tc = Xi, *ts = xr;
            double ar = 0.0, ai = 0.0;
            int idx = 0;
            for (int i = 0; i < n; ++i) {
                const double v = x[i];
                ar += v * tc[idx];
                ai -= v * ts[idx];
                idx += k; if (idx >= n) idx -= n;
            }
            re = ar; im = ai;
        }
        const double ck = (k == 0 || 2 * k == n) ? 1.0 : 2.0;
        const double P = isbad ? NAN : ck * (re * re + im * im) / nn;
        rows[out + k] = P;
        if (sums) sums[out + k] = sums[out + k] + P;
    }
    if (threadIdx.x == 0) bad[(size_t)E.slot * nlat + j] = isbad ? 1.0 : 0.0;
    (void)xi;
}

// the cross-row combination: one workgroup per (entry, 4 neighbouring bins); thread = (lane l, bin kk) with kk the fast index
__global__ void __launch_bounds__(QD_BLOCK)
k_spectra_combine(QdSpecTab T, int nlat, int nbins, const double* __restrict__ wrow, const double* __restrict__ rows,
                  const double* __restrict__ bad, double* __restrict__ rec) {
    __shared__ double s_num[64][QD_SPEC_CBINS], s_w[64][QD_SPEC_CBINS], s_cnt[64];
    const int kblocks = (nbins + QD_SPEC_CBINS - 1) / QD_SPEC_CBINS;
    const int q = blockIdx.x / kblocks, kb = blockIdx.x - q * kblocks;
    const int kk = threadIdx.x & (QD_SPEC_CBINS - 1), l = threadIdx.x / QD_SPEC_CBINS, k = kb * QD_SPEC_CBINS + kk;
    const bool live = k < nbins, counts = kb == 0 && kk == 0;
    const int slot = T.e[q].slot;
    const double* R = rows + (size_t)slot * nlat * nbins + (live ? k : 0);
    const double* B = bad + (size_t)slot * nlat;
    double num = 0.0, W = 0.0, cnt = 0.0;
    for (int j0 = l; j0 < nlat; j0 += 64 * QD_SPEC_CROUNDS) {
        double w[QD_SPEC_CROUNDS], v[QD_SPEC_CROUNDS], bd[QD_SPEC_CROUNDS];
#pragma unroll
        for (int r = 0; r < QD_SPEC_CROUNDS; ++r) {
            const int jr = j0 + 64 * r;
            w[r] = v[r] = bd[r] = 0.0;
            if (jr < nlat) {
                w[r] = wrow[jr];
                if (live) v[r] = R[(size_t)jr * nbins];
                if (counts) bd[r] = B[jr];
            }
        }
#pragma unroll
        for (int r = 0; r < QD_SPEC_CROUNDS; ++r)
            if (j0 + 64 * r < nlat) { num = num + w[r] * v[r]; W = W + w[r]; cnt = cnt + bd[r]; }
    }
    s_num[l][kk] = num; s_w[l][kk] = W;
    if (kk == 0) s_cnt[l] = cnt;
    __syncthreads();
    for (int o = 32; o > 0; o >>= 1) {
        if (l < o) {
            s_num[l][kk] = s_num[l][kk] + s_num[l + o][kk];
            s_w[l][kk] = s_w[l][kk] + s_w[l + o][kk];
            if (kk == 0) s_cnt[l] = s_cnt[l] + s_cnt[l + o];
        }
        __syncthreads();
    }
    if (l == 0) {
        double* out = rec + (size_t)slot * (nbins + QD_SPEC_NSTAT);
        if (live) out[k] = s_num[0][kk] / s_w[0][kk];
        if (counts) out[nbins] = s_cnt[0];
    }
}

// ------------------------------------------------------------------ host side
struct QdSpectra : QdEntrySel {       // the entry table (qd_entry.h)
    int lat = 0, direct = 0, nbins = 0;
    QdSpecPlan plan{};
    size_t lds = 0;                   // dynamic LDS of k_spectra_rows
    double* tw = nullptr;             // [2][n_lon] cos / sin(2 pi t / n_lon)
    double* wrow = nullptr;           // [n_lat] the host's max(cos lat, 0)
    double* rows = nullptr;           // [n][n_lat][n_bins] the per-row powers of the sample in flight
    double* bad = nullptr;            // [n][n_lat] 1.0: the row holds a non-finite value
    double* sums = nullptr;           // [n][n_lat][n_bins] lat_resolved: the sums of the per-row powers
    int64_t count = 0;                // samples in the sums
    double* rec = nullptr;            // the record of the step in progress
    QdSpanLane lane;
    size_t plane_doubles(const qd_ctx* c) const { return (size_t)n * c->geo.nlat * nbins; }
};

static QdSpanLane* spectra_lane(qd_ctx* c) { return c && c->spectra ? &c->spectra->lane : nullptr; }

void qd_spectra_release(qd_ctx* c) {
    QdSpectra* s = c->spectra;
    if (!s) return;
    if (c->stream) hipStreamSynchronize(c->stream);
    void* p[] = {s->tw, s->wrow, s->rows, s->bad, s->sums, s->lane.log};
    for (void* q : p) if (q) hipFree(q);
    delete s;
    c->spectra = nullptr;
}

// n = 2^a 3^b 5^c -> the radix list of the length-m transform (qd_rowfft.h), or false
static bool spectra_plan(int n, QdSpecPlan& F) {
    F = QdSpecPlan{};
    F.even = (n % 2 == 0) ? 1 : 0;
    return qd_rowfft_plan(F.even ? n / 2 : n, F.even ? 2 : 1, F);
}

extern "C" int qd_spectra_configure(qd_handle c, int n, const int32_t* op, const int32_t* a, const int32_t* b, int lat_resolved, const double* w_row) {
    if (!c || n < 0 || (n && (!op || !a || !w_row))) return -1;
    if (!qd_whole_globe(c))
        return qd_fail(c, "qd_spectra_configure: the spectra need a whole-globe handle (world == 1, n_rows == n_lat); "
                          "latitude bands are not supported");
    QdSpectra t;
    if (qd_entries_parse(c, "qd_spectra_configure", n, op, a, b, t)) return -1;
    hipSetDevice(c->desc.device);
    qd_spectra_release(c);
    if (n == 0) return 0;
    const int nlat = c->geo.nlat, nlon = c->geo.nlon;
    const char* form = std::getenv("QD_SPECTRA_FORM");                // read here, once, never on the step path
    t.direct = (form && std::strcmp(form, "direct") == 0) || !spectra_plan(nlon, t.plan) ? 1 : 0;
    t.lds = sizeof(double) * (t.direct ? 1 + 3 * (size_t)nlon : 1 + 4 * (size_t)(QS_SK(t.plan.m) + 1));
    if (t.lds > QD_SPEC_LDS_LIMIT)
        return qd_fail(c, ("qd_spectra_configure: a row of n_lon = " + std::to_string(nlon) + " needs " + std::to_string(t.lds) +
                           " bytes of LDS, a workgroup may take " + std::to_string(QD_SPEC_LDS_LIMIT) + " of the CU's 163840").c_str());
    QdSpectra* s = new QdSpectra(t);
    s->lat = lat_resolved ? 1 : 0;
    s->nbins = nlon / 2 + 1;
    s->lane.width = n * (s->nbins + QD_SPEC_NSTAT);
    s->lane.cap = QD_SPECTRA_LOG_CAP;
    const std::vector<double> tw = qd_rowfft_table(nlon);
    const size_t logb = s->lane.log_doubles() * sizeof(double), planeb = s->plane_doubles(c) * sizeof(double),
                 badb = (size_t)n * nlat * sizeof(double), twb = tw.size() * sizeof(double);
    bool ok = hipMalloc(&s->tw, twb) == hipSuccess && hipMalloc(&s->wrow, (size_t)nlat * sizeof(double)) == hipSuccess &&
              hipMalloc(&s->rows, planeb) == hipSuccess && hipMalloc(&s->bad, badb) == hipSuccess && hipMalloc(&s->lane.log, logb) == hipSuccess &&
              (!s->lat || hipMalloc(&s->sums, planeb) == hipSuccess);
    ok = ok && hipMemcpyAsync(s->tw, tw.data(), twb, hipMemcpyHostToDevice, c->stream) == hipSuccess &&
         hipMemcpyAsync(s->wrow, w_row, (size_t)nlat * sizeof(double), hipMemcpyHostToDevice, c->stream) == hipSuccess &&
         hipMemsetAsync(s->rows, 0, planeb, c->stream) == hipSuccess && hipMemsetAsync(s->bad, 0, badb, c->stream) == hipSuccess &&
         hipMemsetAsync(s->lane.log, 0, logb, c->stream) == hipSuccess &&
         (!s->lat || hipMemsetAsync(s->sums, 0, planeb, c->stream) == hipSuccess) && hipStreamSynchronize(c->stream) == hipSuccess;
    // a workgroup may take more than the default 64 KB of dynamic LDS (k_zonal_filter does the same)
    ok = ok && hipFuncSetAttribute((const void*)k_spectra_rows<0>, hipFuncAttributeMaxDynamicSharedMemorySize, QD_SPEC_LDS_LIMIT) == hipSuccess &&
         hipFuncSetAttribute((const void*)k_spectra_rows<1>, hipFuncAttributeMaxDynamicSharedMemorySize, QD_SPEC_LDS_LIMIT) == hipSuccess;
    c->spectra = s;
    if (!ok) { qd_spectra_release(c); return qd_fail(c, "qd_spectra_configure: device allocation or upload failed"); }
    return 0;
}

extern "C" int qd_spectra_schedule(qd_handle c, int steps, const int32_t* sample) {
    return qd_lane_schedule(c, spectra_lane(c), steps, sample, "qd_spectra_schedule", "not configured (qd_spectra_configure first)");
}
extern "C" int qd_spectra_log(qd_handle c, double* out, int max, int* n) {
    return qd_lane_drain(c, spectra_lane(c), out, max, n, "qd_spectra_log", "not configured (qd_spectra_configure first)");
}
extern "C" int qd_spectra_reset(qd_handle c) {
    if (!c) return -1;
    QdSpectra* s = c->spectra;
    if (!s) return qd_fail(c, "qd_spectra_reset: not configured (qd_spectra_configure first)");
    hipSetDevice(c->desc.device);
    if (s->sums) QD_HIP(c, hipMemsetAsync(s->sums, 0, s->plane_doubles(c) * sizeof(double), c->stream));
    s->count = 0;
    s->lane.reset();
    return 0;
}

extern "C" int qd_spectra_sums_get(qd_handle c, double* sums, int64_t* count) {
    if (!c || !count) return -1;
    QdSpectra* s = c->spectra;
    if (!s) return qd_fail(c, "qd_spectra_sums_get: not configured (qd_spectra_configure first)");
    if (!s->sums) return qd_fail(c, "qd_spectra_sums_get: the configuration is not lat-resolved");
    if (!sums) return -1;
    hipSetDevice(c->desc.device);
    QD_HIP(c, hipMemcpyAsync(sums, s->sums, s->plane_doubles(c) * sizeof(double), hipMemcpyDeviceToHost, c->stream));
    QD_HIP(c, hipStreamSynchronize(c->stream));
    const hipError_t e = hipGetLastError();
    if (e != hipSuccess) return qd_fail(c, "qd_spectra_sums_get: kernel", e);
    *count = s->count;
    return 0;
}

extern "C" int qd_spectra_sums_set(qd_handle c, const double* sums, int64_t count) {
    if (!c) return -1;
    QdSpectra* s = c->spectra;
    if (!s) return qd_fail(c, "qd_spectra_sums_set: not configured (qd_spectra_configure first)");
    if (!s->sums) return qd_fail(c, "qd_spectra_sums_set: the configuration is not lat-resolved");
    if (!sums) return -1;
    if (count < 0) return qd_fail(c, "qd_spectra_sums_set: negative sample count");
    hipSetDevice(c->desc.device);
    QD_HIP(c, hipMemcpyAsync(s->sums, sums, s->plane_doubles(c) * sizeof(double), hipMemcpyHostToDevice, c->stream));
    QD_HIP(c, hipStreamSynchronize(c->stream));                // the host buffer is only borrowed for the call
    s->count = count;
    return 0;
}

bool qd_spectra_planes(const qd_ctx* c, const double** sums, size_t* n) {
    const QdSpectra* s = c->spectra;
    if (!s || !s->sums) return false;
    *sums = s->sums; *n = s->plane_doubles(c);
    return true;
}

bool qd_spectra_scheduled(const qd_ctx* c) { return c->spectra && !c->spectra->lane.sched.empty(); }
bool qd_spectra_reads_lazy(const qd_ctx* c) { return c->spectra && c->spectra->lazy; }

QdSpanLane* qd_spectra_span_begin(qd_ctx* c, int n) {
    static const QdSpanTexts T = {
        "qd_step_n: the spectra need a whole-globe handle; latitude bands are not supported",
        "qd_step_n: qd_spectra_configure has not been called",
        "qd_step_n: a qd_spectra_schedule must cover exactly the n steps of the span",
        "qd_step_n: the span's spectra records would overflow the log of QD_SPECTRA_LOG_CAP (drain it with qd_spectra_log first)"};
    const bool stale = c->spectra && c->spectra->stale(c);
    QdSpanLane* l = qd_lane_span_begin(c, spectra_lane(c), n, T, nullptr,
                                       stale ? "qd_step_n: a spectra field is no longer an f64 plane (qd_spectra_configure again)" : nullptr);
    if (!l && c->spectra) c->spectra->lane.clear_schedule();      // refused: the span guard never sees this lane, and a schedule serves one span
    return l;
}

// a sampled step begins: its record slot, which the step's groups fill between them (every entry is in one of the two)
int qd_spectra_begin_step(qd_ctx* c) {
    QdSpectra* s = c->spectra;
    if (s->lane.full()) return qd_fail(c, "qd_step_n: spectra log full (drain it with qd_spectra_log)");
    s->rec = s->lane.next();
    return 0;
}

// QD_LAUNCH_TIMED with dynamic LDS
#define QS_LAUNCH_TIMED(sc, kernel, grid, block, lds, stream, ...) do { \
    if ((sc).on && (sc).attach) { (sc).used = true; hipExtLaunchKernelGGL((kernel), grid, block, lds, stream, (sc).e0, (sc).e1, 0, __VA_ARGS__); } \
    else hipLaunchKernelGGL((kernel), grid, block, lds, stream, __VA_ARGS__); } while (0)

// group 0: the early entries, 1: the late entries (the sample count moves on with them), 2: all of them (the class seam)
int qd_spectra_transform(qd_ctx* c, int group) {
    QdSpectra* s = c->spectra;
    QdSpecTab T;
    T.n = 0;
    for (int k = 0; k < s->n; ++k) {
        if (group != 2 && s->early[k] != (group == 0)) continue;
        T.e[T.n++] = QdSpecEntry{c->f[s->a[k]], s->op[k] == 1 ? c->f[s->b[k]] : (const double*)nullptr, k, 0};
    }
    for (int k = T.n; k < QD_ENTRY_MAX; ++k) T.e[k] = QdSpecEntry{nullptr, nullptr, 0, 0};
    if (group != 0) s->count++;
    if (T.n == 0) return 0;
    const int nlat = c->geo.nlat, nlon = c->geo.nlon;
    {
        QdScope sc(c, "spectra", true);                       // k_spectra_rows: timed from the dispatch itself
        if (s->direct)
            QS_LAUNCH_TIMED(sc, k_spectra_rows<1>, dim3(T.n * nlat), dim3(QD_BLOCK), s->lds, c->stream, T, s->plan, nlat, nlon,
                            (const double*)s->tw, s->rows, s->bad, s->sums);
        else
            QS_LAUNCH_TIMED(sc, k_spectra_rows<0>, dim3(T.n * nlat), dim3(QD_BLOCK), s->lds, c->stream, T, s->plan, nlat, nlon,
                            (const double*)s->tw, s->rows, s->bad, s->sums);
    }
    QdScope sc(c, "spectra_combine", true);
    const int kblocks = (s->nbins + QD_SPEC_CBINS - 1) / QD_SPEC_CBINS;
    QS_LAUNCH_TIMED(sc, k_spectra_combine, dim3(T.n * kblocks), dim3(QD_BLOCK), 0, c->stream, T, nlat, s->nbins, (const double*)s->wrow,
                    (const double*)s->rows, (const double*)s->bad, s->rec);
    return 0;
}

extern "C" int qd_spectra_sample(qd_handle c) {
    if (!c) return -1;
    if (!c->spectra) return qd_fail(c, "qd_spectra_sample: not configured (qd_spectra_configure first)");
    if (c->spectra->stale(c)) return qd_fail(c, "qd_spectra_sample: a spectra field is no longer an f64 plane (qd_spectra_configure again)");
    if (c->spectra->lane.full()) return qd_fail(c, "qd_spectra_sample: spectra log full (drain it with qd_spectra_log)");
    hipSetDevice(c->desc.device);
    c->spectra->rec = c->spectra->lane.next();
    if (int rc = qd_spectra_transform(c, 2)) return rc;
    return qd_launch_check(c, "qd_spectra_sample");
}
