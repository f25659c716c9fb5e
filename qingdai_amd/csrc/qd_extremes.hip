// qd_extremes.hip -- extremes, spells and distributions: per-cell selections and integer counts, per-row histograms, accumulated as
// a span lane, gfx950 (QD_EXTREMES).
//
// THE DEFINITION (qingdai_amd/extremes.py: accumulate_reference restates it bit for bit; there is no third statement).
// A configuration names E <= QD_EXTREMES_MAX_ENTRIES entries of the entry table (qd_entry.h: op 0 a plane, op 1 sqrt(a*a + b*b)),
// T <= QD_EXTREMES_MAX_THRESHOLDS thresholds (entry, cmp, value), cmp '<' or '>', value a finite f64, and B <= QD_EXTREMES_MAX_HISTS
// binned entries, each with nb + 1 strictly increasing finite f64 edges e_0 .. e_nb, 1 <= nb <= QD_EXTREMES_MAX_BINS.  Resident state,
// reset at a window's start; k is the 0-based index of the sample in its window, a host integer that comes with the launch; x is the
// entry's value in the cell:
//     per entry and cell       vmax, vmin  f64, start -inf, +inf       if (x > vmax) { vmax = x; tmax = k; }
//                              tmax, tmin  i32, start -1               if (x < vmin) { vmin = x; tmin = k; }
//                              nan         i32, start 0                nan += (x != x)
//     per threshold and cell   count, run, longest, spells  u32, 0     hit = x cmp value (false for a NaN)
//                                                                      spells += hit && run == 0;  run = hit ? run + 1 : 0
//                                                                      count += hit;  longest = max(longest, run)
//     per binned entry, row    hist[nb + 3]  i64, start 0              columns [under, bin 0 .. bin nb - 1, over, nan]: a NaN adds to nan,
//                                                                      x < e_0 to under, x >= e_nb to over, anything else to bin
//                                                                      np.searchsorted(edges, x, side="right") - 1
// The comparisons are strict: the earliest of equal values keeps its time, a NaN never enters, -0.0 does not displace +0.0.  run is
// reset with everything else: a spell is cut at a window boundary.  One rule for every table of edges; no log and no division on the
// device.  Every number is a selection among stored values or an integer count, so the state does not depend on the launch
// geometry, on how a run is cut into spans, nor on span lane or class seam (qd_extremes_sample).
//
// A sample of step s is what qd_download returns after a span that ends with step s: the entries that read PRECIP are sampled in
// front of the ocean step, every other entry behind the step's last launch (history's early and late groups, qd_entry.h).  A sampled
// step adds at most these two launches, an unsampled step none.
//
// k_ext_accum: one workgroup per QD_BLOCK consecutive cells of a latitude row (blockIdx.y the row, blockIdx.x the segment), one cell
// per thread, one launch for a whole group.  The table -- sources, and per entry of the launch the slots of its thresholds and
// histograms -- comes by value in the kernel arguments and is rebuilt from c->f[] at every launch (the step swaps field pointers);
// thresholds and histograms are listed by entry, so every index into the table is a loop counter, wave-uniform, and x stays in a
// register (no per-thread array indexed by a run-time value: it would live in scratch, qd_eddy.hip).  Per cell and entry: the
// source(s), vmax and vmin are read; stores go out only where a value changed (tmax, tmin are written, never read; nan is read and
// written only for a NaN).  A threshold is one 16-byte load and at most one 16-byte store.  Histograms: the edges and one u32
// counter per column of every table are in LDS (static, 24.7 KiB); a NaN, under and over are counted per wave by ballot and
// population count and added by one lane; an in-range cell finds its bin by bisection on the LDS edges and adds 1 with an LDS
// integer atomic.  A row is split across workgroups (one workgroup per row left a device of 256 CUs three workgroups each, and
// every thread six dependent passes: 0.088 against 0.068 ms per sampled step at 721 x 1440): behind a barrier a workgroup adds its
// non-zero counters into the row's i64 columns with 64-bit integer atomics, so the table does not depend on the order of arrival.
// No float atomics.  Whole-globe handles only.
#include "qd_span.h"
#include "qd_entry.h"
#include <algorithm>
#include <cmath>
#include <string>
#include <vector>

#define QD_EXT_E QD_EXTREMES_MAX_ENTRIES
#define QD_EXT_T QD_EXTREMES_MAX_THRESHOLDS
#define QD_EXT_H QD_EXTREMES_MAX_HISTS
#define QD_EXT_EDGES (QD_EXT_H * (QD_EXTREMES_MAX_BINS + 1))
#define QD_EXT_COLS (QD_EXT_H * (QD_EXTREMES_MAX_BINS + 3))
static_assert(QD_EXT_E <= QD_ENTRY_MAX, "the entry table holds the lane's entries");

struct QdExtTab {
    const double* a[QD_EXT_E];               // the sources of the launch's entries, as c->f[] stands at this launch
    const double* b[QD_EXT_E];               // nullptr: op 0
    double* val;                             // [2][E][cells]: vmax, vmin
    int* cnt;                                // [3][E][cells]: tmax, tmin, nan
    uint4* thr;                              // [T][cells]: {count, run, longest, spells}
    long long* hist;                         // the tables [n_lat][nb + 3], one behind the other
    const double* edges;                     // the edges of all tables, one behind the other
    size_t cells;
    int E, n, k;                             // configured entries (the plane count of val and cnt), entries of this launch, the sample's index
    int n_edges, n_cols;                     // edges and columns of all tables
    int ent[QD_EXT_E];                       // launch entry j -> its index in the state
    int tb[QD_EXT_E + 1];                    // launch entry j's thresholds: the slots [tb[j], tb[j + 1])
    int tix[QD_EXT_T];                       // slot -> the threshold's index in the state | (cmp is '>') << 8
    double tv[QD_EXT_T];                     // slot -> value
    int hb[QD_EXT_E + 1];                    // launch entry j's histograms: the slots [hb[j], hb[j + 1])
    int hix[QD_EXT_H];                       // slot -> the table's index
    int nb[QD_EXT_H], eo[QD_EXT_H], bo[QD_EXT_H];    // by table: bins, its first edge in `edges`, its first column among all columns
    long long ho[QD_EXT_H];                  // by table: its first element in `hist`
};

__global__ void __launch_bounds__(QD_BLOCK)
k_ext_accum(QdExtTab T, int nlon) {
    __shared__ double s_edge[QD_EXT_EDGES];
    __shared__ unsigned int s_col[QD_EXT_COLS];
    const int tid = threadIdx.x, row = blockIdx.y, c0 = blockIdx.x * QD_BLOCK;
    const bool binned = T.hb[T.n] > 0;                   // wave-uniform: the barriers below are taken by all or none
    if (binned) {
        for (int i = tid; i < T.n_edges; i += QD_BLOCK) s_edge[i] = T.edges[i];
        for (int i = tid; i < T.n_cols; i += QD_BLOCK) s_col[i] = 0u;
        __syncthreads();
    }
    const size_t r0 = (size_t)row * nlon, cells = T.cells;
    {
        const bool valid = c0 + tid < nlon;              // a lane past the row's end stays to the end: the ballots see whole waves
        const size_t i = r0 + (valid ? c0 + tid : 0);
        for (int j = 0; j < T.n; ++j) {
            const int e = T.ent[j];
            double x = 0.0;
            if (valid) {
                const double* B = T.b[j];
                double* pmax = T.val + (size_t)e * cells + i;
                double* pmin = T.val + (size_t)(T.E + e) * cells + i;
                const double xa = T.a[j][i], xb = B ? B[i] : 0.0, vmax = *pmax, vmin = *pmin;
                x = hist_value(xa, xb, B != nullptr);
                if (x > vmax) { *pmax = x; T.cnt[(size_t)e * cells + i] = T.k; }
                if (x < vmin) { *pmin = x; T.cnt[(size_t)(T.E + e) * cells + i] = T.k; }
                if (x != x) T.cnt[(size_t)(2 * T.E + e) * cells + i] += 1;
            }
            for (int s = T.tb[j]; s < T.tb[j + 1]; ++s) {
                if (valid) {
                    uint4* p = T.thr + (size_t)(T.tix[s] & 255) * cells + i;
                    uint4 w = *p;                        // x count, y run, z longest, w spells
                    const double v = T.tv[s];
                    const bool hit = (T.tix[s] >> 8) ? x > v : x < v;
                    if (hit) {
                        w.w += w.y == 0u ? 1u : 0u;
                        w.y += 1u;
                        w.x += 1u;
                        w.z = w.z > w.y ? w.z : w.y;
                        *p = w;
                    } else if (w.y != 0u) {
                        w.y = 0u;
                        *p = w;
                    }
                }
            }
            for (int s = T.hb[j]; s < T.hb[j + 1]; ++s) {
                const int h = T.hix[s], nb = T.nb[h];
                const double* ed = s_edge + T.eo[h];
                unsigned int* col = s_col + T.bo[h];
                const bool is_nan = valid && x != x;
                const bool under = valid && x < ed[0];
                const bool over = valid && x >= ed[nb];
                const unsigned int n_nan = (unsigned int)__popcll(__ballot(is_nan));
                const unsigned int n_under = (unsigned int)__popcll(__ballot(under));
                const unsigned int n_over = (unsigned int)__popcll(__ballot(over));
                if ((tid & 63) == 0) {
                    if (n_under) atomicAdd(col, n_under);
                    if (n_over) atomicAdd(col + nb + 1, n_over);
                    if (n_nan) atomicAdd(col + nb + 2, n_nan);
                }
                if (valid && !is_nan && !under && !over) {
                    int lo = 0, hi = nb;                 // e[lo] <= x < e[hi]
                    while (hi - lo > 1) {
                        const int mid = (lo + hi) >> 1;
                        if (ed[mid] <= x) lo = mid; else hi = mid;
                    }
                    atomicAdd(col + 1 + lo, 1u);
                }
            }
        }
    }
    if (binned) {
        __syncthreads();
        for (int s = 0; s < T.hb[T.n]; ++s) {
            const int h = T.hix[s], w = T.nb[h] + 3;
            unsigned long long* g = reinterpret_cast<unsigned long long*>(T.hist + T.ho[h] + (size_t)row * w);
            const unsigned int* col = s_col + T.bo[h];
            for (int i = tid; i < w; i += QD_BLOCK) {
                const unsigned int v = col[i];
                if (v) atomicAdd(g + i, (unsigned long long)v);
            }
        }
    }
}

// the start values of the f64 planes: [0, half) -inf, [half, 2 half) +inf
__global__ void __launch_bounds__(QD_BLOCK)
k_ext_fill(double* __restrict__ val, size_t half) {
    const size_t stride = (size_t)gridDim.x * QD_BLOCK;
    for (size_t i = (size_t)blockIdx.x * QD_BLOCK + threadIdx.x; i < 2 * half; i += stride) val[i] = i < half ? -INFINITY : INFINITY;
}

struct QdExtremes : QdEntrySel {      // the entry table (qd_entry.h)
    int T = 0, B = 0;
    int t_entry[QD_EXT_T], t_gt[QD_EXT_T];
    double t_value[QD_EXT_T];
    int h_entry[QD_EXT_H], h_nb[QD_EXT_H], h_eo[QD_EXT_H], h_bo[QD_EXT_H];
    long long h_ho[QD_EXT_H];
    int n_edges = 0, n_cols = 0;
    size_t cells = 0, hist_n = 0;     // cells of a plane; elements of all histogram tables
    double* val = nullptr;            // [2][E][cells]
    unsigned int* words = nullptr;    // every 4-byte plane: [T][cells][4] thresholds (16-byte aligned: they come first), then [3][E][cells]
    long long* hist = nullptr;        // hist_n elements (nullptr without a histogram)
    double* edges = nullptr;          // n_edges (likewise)
    int64_t count = 0;                // samples in the state
    QdSpanLane lane;                  // width 0: no log

    size_t thr_words() const { return (size_t)4 * T * cells; }
    size_t cnt_words() const { return (size_t)3 * n * cells; }
    int* cnt() const { return reinterpret_cast<int*>(words + thr_words()); }
};

static const char* const EXT_MISSING = "extremes: not configured (qd_extremes_configure first)";
static const char* const EXT_STALE = "extremes: a field is no longer an f64 plane (qd_extremes_configure again)";
static QdSpanLane* ext_lane(qd_ctx* c) { return c && c->extremes ? &c->extremes->lane : nullptr; }

void qd_extremes_release(qd_ctx* c) {
    QdExtremes* x = c->extremes;
    if (!x) return;
    if (c->stream) hipStreamSynchronize(c->stream);
    if (x->val) hipFree(x->val);
    if (x->words) hipFree(x->words);
    if (x->hist) hipFree(x->hist);
    if (x->edges) hipFree(x->edges);
    delete x;
    c->extremes = nullptr;
}

// the state at its start values, on the stream
static hipError_t ext_clear(qd_ctx* c, QdExtremes* x) {
    const size_t half = (size_t)x->n * x->cells;
    const int blocks = (int)std::min<size_t>(std::max<size_t>(1, (2 * half + QD_BLOCK - 1) / QD_BLOCK), (size_t)std::max(1, c->n_cu) * 8);
    hipLaunchKernelGGL(k_ext_fill, dim3(blocks), dim3(QD_BLOCK), 0, c->stream, x->val, half);
    hipError_t e = hipGetLastError();
    if (e == hipSuccess && x->T) e = hipMemsetAsync(x->words, 0, x->thr_words() * 4, c->stream);
    if (e == hipSuccess) e = hipMemsetAsync(x->cnt(), 0xFF, 2 * half * 4, c->stream);                 // tmax, tmin: -1
    if (e == hipSuccess) e = hipMemsetAsync(x->cnt() + 2 * half, 0, half * 4, c->stream);             // nan
    if (e == hipSuccess && x->hist) e = hipMemsetAsync(x->hist, 0, x->hist_n * sizeof(long long), c->stream);
    return e;
}

extern "C" int qd_extremes_configure(qd_handle c, int n_entries, const int32_t* op, const int32_t* a, const int32_t* b, int n_thresholds,
                                     const int32_t* thr_entry, const int32_t* thr_cmp, const double* thr_value, int n_hists,
                                     const int32_t* hist_entry, const int32_t* hist_nb, const double* edges) {
    if (!c || n_entries < 0 || n_thresholds < 0 || n_hists < 0 || (n_entries && (!op || !a))) return -1;
    if (n_entries && ((n_thresholds && (!thr_entry || !thr_cmp || !thr_value)) || (n_hists && (!hist_entry || !hist_nb || !edges)))) return -1;
    if (!qd_whole_globe(c))
        return qd_fail(c, "extremes: the extremes lane needs a whole-globe handle (world == 1, n_rows == n_lat); latitude bands are not supported");
    QdExtremes t;
    if (n_entries > QD_EXT_E) return qd_fail(c, "extremes: at most 16 entries");
    if (n_thresholds > QD_EXT_T) return qd_fail(c, "extremes: at most 16 thresholds");
    if (n_hists > QD_EXT_H) return qd_fail(c, "extremes: at most 8 histograms");
    if (qd_entries_parse(c, "extremes", n_entries, op, a, b, t)) return -1;
    std::vector<double> host_edges;
    for (int k = 0; k < n_thresholds && n_entries; ++k) {
        const std::string w = "extremes: threshold " + std::to_string(k);
        if (thr_entry[k] < 0 || thr_entry[k] >= n_entries) return qd_fail(c, (w + " has an entry index outside the " + std::to_string(n_entries) + " entries").c_str());
        if (thr_cmp[k] != QD_EXTREMES_CMP_LT && thr_cmp[k] != QD_EXTREMES_CMP_GT) return qd_fail(c, (w + ": cmp is neither '<' (60) nor '>' (62)").c_str());
        if (!std::isfinite(thr_value[k])) return qd_fail(c, (w + ": the value is not finite").c_str());
        t.t_entry[k] = thr_entry[k]; t.t_gt[k] = thr_cmp[k] == QD_EXTREMES_CMP_GT ? 1 : 0; t.t_value[k] = thr_value[k];
    }
    const size_t nlat = (size_t)c->geo.nlat;
    for (int h = 0; h < n_hists && n_entries; ++h) {
        const std::string w = "extremes: histogram " + std::to_string(h);
        if (hist_entry[h] < 0 || hist_entry[h] >= n_entries) return qd_fail(c, (w + " has an entry index outside the " + std::to_string(n_entries) + " entries").c_str());
        if (hist_nb[h] < 1) return qd_fail(c, (w + ": fewer than 2 edges").c_str());
        if (hist_nb[h] > QD_EXTREMES_MAX_BINS) return qd_fail(c, (w + ": at most 256 bins").c_str());
        const double* e = edges + t.n_edges;
        for (int i = 0; i <= hist_nb[h]; ++i)
            if (!std::isfinite(e[i]) || (i && !(e[i] > e[i - 1]))) return qd_fail(c, (w + ": the edges are not finite and strictly increasing").c_str());
        t.h_entry[h] = hist_entry[h]; t.h_nb[h] = hist_nb[h]; t.h_eo[h] = t.n_edges; t.h_bo[h] = t.n_cols; t.h_ho[h] = (long long)t.hist_n;
        host_edges.insert(host_edges.end(), e, e + hist_nb[h] + 1);
        t.n_edges += hist_nb[h] + 1; t.n_cols += hist_nb[h] + 3; t.hist_n += nlat * (size_t)(hist_nb[h] + 3);
    }
    hipSetDevice(c->desc.device);
    qd_extremes_release(c);
    if (n_entries == 0) return 0;
    t.T = n_thresholds; t.B = n_hists; t.cells = c->geo.cells();
    QdExtremes* x = new QdExtremes(t);
    c->extremes = x;
    bool ok = hipMalloc(&x->val, (size_t)2 * x->n * x->cells * sizeof(double)) == hipSuccess &&
              hipMalloc(&x->words, (x->thr_words() + x->cnt_words()) * 4) == hipSuccess;
    if (ok && x->B)
        ok = hipMalloc(&x->hist, x->hist_n * sizeof(long long)) == hipSuccess && hipMalloc(&x->edges, (size_t)x->n_edges * sizeof(double)) == hipSuccess &&
             hipMemcpyAsync(x->edges, host_edges.data(), (size_t)x->n_edges * sizeof(double), hipMemcpyHostToDevice, c->stream) == hipSuccess;
    ok = ok && ext_clear(c, x) == hipSuccess && hipStreamSynchronize(c->stream) == hipSuccess;      // host_edges is only borrowed
    if (!ok) { qd_extremes_release(c); return qd_fail(c, "extremes: device allocation failed"); }
    return 0;
}

extern "C" int qd_extremes_schedule(qd_handle c, int steps, const int32_t* sample) {
    return qd_lane_schedule(c, ext_lane(c), steps, sample, "extremes", "not configured (qd_extremes_configure first)");
}

bool qd_extremes_scheduled(const qd_ctx* c) { return c->extremes && !c->extremes->lane.sched.empty(); }
bool qd_extremes_reads_lazy(const qd_ctx* c) { return c->extremes && c->extremes->lazy; }

QdSpanLane* qd_extremes_span_begin(qd_ctx* c, int n) {
    static const QdSpanTexts T = {
        "extremes: qd_step_n: the extremes lane needs a whole-globe handle; latitude bands are not supported",
        "extremes: qd_step_n: qd_extremes_configure has not been called",
        "extremes: qd_step_n: a qd_extremes_schedule must cover exactly the n steps of the span",
        "extremes: qd_step_n: a span samples the extremes at most QD_SPAN_LOG_CAP times"};
    QdSpanLane* l = qd_lane_span_begin(c, ext_lane(c), n, T, nullptr, c->extremes && c->extremes->stale(c) ? EXT_STALE : nullptr);
    if (!l && c->extremes) c->extremes->lane.clear_schedule();    // refused: the span guard never sees this lane, and a schedule serves one span
    return l;
}

// group 0: the early entries, 1: the late entries (the sample count moves on with them), 2: all of them (the class seam)
int qd_extremes_accumulate(qd_ctx* c, int group) {
    QdExtremes* x = c->extremes;
    QdExtTab T = {};
    T.val = x->val; T.cnt = x->cnt(); T.thr = reinterpret_cast<uint4*>(x->words); T.hist = x->hist; T.edges = x->edges;
    T.cells = x->cells; T.E = x->n; T.k = (int)x->count; T.n_edges = x->n_edges; T.n_cols = x->n_cols;
    for (int h = 0; h < x->B; ++h) { T.nb[h] = x->h_nb[h]; T.eo[h] = x->h_eo[h]; T.bo[h] = x->h_bo[h]; T.ho[h] = x->h_ho[h]; }
    int nt = 0, nh = 0;
    for (int k = 0; k < x->n; ++k) {
        if (group != 2 && x->early[k] != (group == 0)) continue;
        const int j = T.n++;
        T.a[j] = c->f[x->a[k]]; T.b[j] = x->op[k] == 1 ? c->f[x->b[k]] : (const double*)nullptr;
        T.ent[j] = k; T.tb[j] = nt; T.hb[j] = nh;
        for (int t = 0; t < x->T; ++t) if (x->t_entry[t] == k) { T.tix[nt] = t | (x->t_gt[t] << 8); T.tv[nt] = x->t_value[t]; ++nt; }
        for (int h = 0; h < x->B; ++h) if (x->h_entry[h] == k) T.hix[nh++] = h;
    }
    for (int j = T.n; j <= QD_EXT_E; ++j) { T.tb[j] = nt; T.hb[j] = nh; }
    if (group != 0) x->count++;
    if (T.n == 0) return 0;
    QdScope sc(c, "extremes", true);                      // one launch: timed from the dispatch itself
    QD_LAUNCH_TIMED(sc, k_ext_accum, dim3((unsigned)((c->geo.nlon + QD_BLOCK - 1) / QD_BLOCK), (unsigned)c->geo.nlat), dim3(QD_BLOCK), c->stream, T,
                    c->geo.nlon);
    return 0;
}

extern "C" int qd_extremes_sample(qd_handle c) {
    if (!c) return -1;
    if (!c->extremes) return qd_fail(c, EXT_MISSING);
    if (c->extremes->stale(c)) return qd_fail(c, EXT_STALE);
    hipSetDevice(c->desc.device);
    if (int rc = qd_extremes_accumulate(c, 2)) return rc;
    return qd_launch_check(c, "extremes: qd_extremes_sample");
}

extern "C" int qd_extremes_read(qd_handle c, double* values, int32_t* counts, int32_t* thresholds, int64_t* hist, int64_t* count) {
    if (!c) return -1;
    QdExtremes* x = c->extremes;
    if (!x) return qd_fail(c, EXT_MISSING);
    if (!values || !counts || !count || (x->T && !thresholds) || (x->B && !hist)) return -1;
    hipSetDevice(c->desc.device);
    QD_HIP(c, hipMemcpyAsync(values, x->val, (size_t)2 * x->n * x->cells * sizeof(double), hipMemcpyDeviceToHost, c->stream));
    QD_HIP(c, hipMemcpyAsync(counts, x->cnt(), x->cnt_words() * 4, hipMemcpyDeviceToHost, c->stream));
    if (x->T) QD_HIP(c, hipMemcpyAsync(thresholds, x->words, x->thr_words() * 4, hipMemcpyDeviceToHost, c->stream));
    if (x->B) QD_HIP(c, hipMemcpyAsync(hist, x->hist, x->hist_n * sizeof(long long), hipMemcpyDeviceToHost, c->stream));
    QD_HIP(c, hipStreamSynchronize(c->stream));               // a host buffer is only borrowed for the call
    const hipError_t err = hipGetLastError();
    if (err != hipSuccess) return qd_fail(c, "extremes: qd_extremes_read: kernel", err);
    *count = x->count;
    return 0;
}

extern "C" int qd_extremes_restore(qd_handle c, const double* values, const int32_t* counts, const int32_t* thresholds, const int64_t* hist,
                                   int64_t count) {
    if (!c) return -1;
    QdExtremes* x = c->extremes;
    if (!x) return qd_fail(c, EXT_MISSING);
    if (!values || !counts || (x->T && !thresholds) || (x->B && !hist)) return -1;
    if (count < 0 || count > INT32_MAX) return qd_fail(c, "extremes: qd_extremes_restore: the sample count is negative or no int32");
    hipSetDevice(c->desc.device);
    QD_HIP(c, hipMemcpyAsync(x->val, values, (size_t)2 * x->n * x->cells * sizeof(double), hipMemcpyHostToDevice, c->stream));
    QD_HIP(c, hipMemcpyAsync(x->cnt(), counts, x->cnt_words() * 4, hipMemcpyHostToDevice, c->stream));
    if (x->T) QD_HIP(c, hipMemcpyAsync(x->words, thresholds, x->thr_words() * 4, hipMemcpyHostToDevice, c->stream));
    if (x->B) QD_HIP(c, hipMemcpyAsync(x->hist, hist, x->hist_n * sizeof(long long), hipMemcpyHostToDevice, c->stream));
    QD_HIP(c, hipStreamSynchronize(c->stream));
    x->count = count;
    return 0;
}

bool qd_extremes_planes(const qd_ctx* c, int which, const void** p, size_t* n) {
    const QdExtremes* x = c->extremes;
    if (!x) return false;
    if (which == 0) { *p = x->val; *n = (size_t)2 * x->n * x->cells; }
    else if (which == 1) { *p = x->words; *n = x->thr_words() + x->cnt_words(); }
    else { *p = x->hist; *n = x->hist_n; }
    return true;
}

extern "C" int qd_extremes_reset(qd_handle c) {
    if (!c) return -1;
    QdExtremes* x = c->extremes;
    if (!x) return qd_fail(c, EXT_MISSING);
    hipSetDevice(c->desc.device);
    const hipError_t e = ext_clear(c, x);
    if (e != hipSuccess) return qd_fail(c, "extremes: qd_extremes_reset", e);
    x->count = 0;
    x->lane.clear_schedule();
    return 0;
}
