// qd_history.hip -- time-mean history files: per-step accumulation of selected fields as a span lane, gfx950 (QD_HISTORY).
//
// An entry is an f64 plane (op 0) or sqrt(a*a + b*b) of two planes (op 1); its sum plane receives sum = sum + x on every sampled step
// of a qd_step_n span (qd_history_schedule: one value per step, non-zero = sampled).  The lane has no flag bit and no log: a schedule
// given before the span turns it on, the sums stay resident until the host reads them (qd_history_read) and divides by the sample
// count, once (qingdai_amd/history.py).  A cell of a sum has one writer and the adds of a window come in step order, so the sums do
// not depend on how a run is cut into spans: ((0 + x_1) + x_2) + ..., f64, no compensation, a NaN sample makes the cell NaN.
//
// A sample of step s is what qd_download returns after a span that ends with step s.  With the precipitation block of step s + 1
// queued inside the ocean step of step s (QD_HOIST_PRECIP, qd_api.hip) PRECIP is overwritten before step s is over, so the entries
// that read PRECIP -- the only field that block stores -- form the EARLY group, accumulated in front of the ocean step; every other
// entry is in the LATE group, accumulated behind the last launch of the step.  A sampled step adds at most these two launches, an
// unsampled step none.
//
// k_hist_accum: one launch for a whole group.  The table of (a, b, sum) pointers comes by value in the kernel arguments (32 x 24
// bytes).  Grid-stride over PAIRS of cells, 16-byte loads and stores per lane (every plane starts 16-byte aligned: the fields are
// allocations of their own, the sum planes have an even stride); an odd cell count leaves one cell to a scalar tail.  The entry loop
// is unrolled by four: the loads of four entries are in flight before the first add.  The grid is sized from the CU count.  No LDS,
// no atomics.  Whole-globe handles only.
#include "qd_span.h"
#include "qd_entry.h"
#include <algorithm>

#define QD_HISTORY_MAX QD_ENTRY_MAX    // entries (include/qingdai_hip.h: QD_HISTORY_MAX_ENTRIES)
#define QD_HIST_UNROLL 4

struct QdHistEntry { const double* a; const double* b; double* sum; };        // b == nullptr: op 0
struct QdHistTab { QdHistEntry e[QD_HISTORY_MAX]; int n; };

__global__ void __launch_bounds__(QD_BLOCK)
k_hist_accum(QdHistTab T, size_t npairs, size_t cells) {
    const size_t stride = (size_t)gridDim.x * QD_BLOCK;
    for (size_t p = (size_t)blockIdx.x * QD_BLOCK + threadIdx.x; p < npairs; p += stride) {
        for (int e0 = 0; e0 < T.n; e0 += QD_HIST_UNROLL) {
            double2 x[QD_HIST_UNROLL], y[QD_HIST_UNROLL], s[QD_HIST_UNROLL];
#pragma unroll
            for (int k = 0; k < QD_HIST_UNROLL; ++k) {
                if (e0 + k < T.n) {
                    const QdHistEntry E = T.e[e0 + k];
                    x[k] = reinterpret_cast<const double2*>(E.a)[p];
                    y[k] = E.b ? reinterpret_cast<const double2*>(E.b)[p] : make_double2(0.0, 0.0);
                    s[k] = reinterpret_cast<const double2*>(E.sum)[p];
                }
            }
#pragma unroll
            for (int k = 0; k < QD_HIST_UNROLL; ++k) {
                if (e0 + k < T.n) {
                    const QdHistEntry E = T.e[e0 + k];
                    const bool pair = E.b != nullptr;
                    double2 r;
                    r.x = s[k].x + hist_value(x[k].x, y[k].x, pair);
                    r.y = s[k].y + hist_value(x[k].y, y[k].y, pair);
                    reinterpret_cast<double2*>(E.sum)[p] = r;
                }
            }
        }
    }
    // odd cell count: the last cell, one thread per entry
    if ((cells & 1) && blockIdx.x == 0 && (int)threadIdx.x < T.n) {
        const QdHistEntry E = T.e[threadIdx.x];
        const size_t o = cells - 1;
        E.sum[o] = E.sum[o] + hist_value(E.a[o], E.b ? E.b[o] : 0.0, E.b != nullptr);
    }
}

struct QdHistory : QdEntrySel {       // the entry table (qd_entry.h)
    double* sums = nullptr;           // [n][stride]
    size_t stride = 0;                // cells rounded up to even: every sum plane starts 16-byte aligned
    int64_t count = 0;                // samples in the sums
    QdSpanLane lane;                  // width 0: no log
};

static QdSpanLane* hist_lane(qd_ctx* c) { return c && c->history ? &c->history->lane : nullptr; }

void qd_history_release(qd_ctx* c) {
    QdHistory* h = c->history;
    if (!h) return;
    if (c->stream) hipStreamSynchronize(c->stream);
    if (h->sums) hipFree(h->sums);
    delete h;
    c->history = nullptr;
}

extern "C" int qd_history_configure(qd_handle c, int n, const int32_t* op, const int32_t* a, const int32_t* b) {
    if (!c || n < 0 || (n && (!op || !a))) return -1;
    if (!qd_whole_globe(c))
        return qd_fail(c, "qd_history_configure: the history accumulators need a whole-globe handle (world == 1, n_rows == n_lat); "
                          "latitude bands are not supported");
    QdHistory t;
    if (qd_entries_parse(c, "qd_history_configure", n, op, a, b, t)) return -1;
    hipSetDevice(c->desc.device);
    qd_history_release(c);
    if (n == 0) return 0;
    QdHistory* h = new QdHistory(t);
    h->stride = (c->geo.cells() + 1) & ~(size_t)1;
    const size_t bytes = (size_t)n * h->stride * sizeof(double);
    const bool ok = hipMalloc(&h->sums, bytes) == hipSuccess && hipMemsetAsync(h->sums, 0, bytes, c->stream) == hipSuccess &&
                    hipStreamSynchronize(c->stream) == hipSuccess;
    c->history = h;
    if (!ok) { qd_history_release(c); return qd_fail(c, "qd_history_configure: device allocation failed"); }
    return 0;
}

extern "C" int qd_history_schedule(qd_handle c, int steps, const int32_t* sample) {
    return qd_lane_schedule(c, hist_lane(c), steps, sample, "qd_history_schedule", "not configured (qd_history_configure first)");
}

bool qd_history_scheduled(const qd_ctx* c) { return c->history && !c->history->lane.sched.empty(); }
bool qd_history_reads_lazy(const qd_ctx* c) { return c->history && c->history->lazy; }

static bool hist_stale(const qd_ctx* c) { return c->history && c->history->stale(c); }

QdSpanLane* qd_history_span_begin(qd_ctx* c, int n) {
    static const QdSpanTexts T = {
        "qd_step_n: the history accumulators need a whole-globe handle; latitude bands are not supported",
        "qd_step_n: qd_history_configure has not been called",
        "qd_step_n: a qd_history_schedule must cover exactly the n steps of the span",
        "qd_step_n: a span samples the history at most QD_SPAN_LOG_CAP times"};
    QdSpanLane* l = qd_lane_span_begin(c, hist_lane(c), n, T, nullptr,
                                       hist_stale(c) ? "qd_step_n: a history field is no longer an f64 plane (qd_history_configure again)" : nullptr);
    if (!l && c->history) c->history->lane.clear_schedule();      // refused: the span guard never sees this lane, and a schedule serves one span
    return l;
}

// group 0: the early entries, 1: the late entries (the sample count moves on with them), 2: all of them (the class seam)
int qd_history_accumulate(qd_ctx* c, int group) {
    QdHistory* h = c->history;
    QdHistTab T;
    T.n = 0;
    for (int k = 0; k < h->n; ++k) {
        if (group != 2 && h->early[k] != (group == 0)) continue;
        T.e[T.n++] = QdHistEntry{c->f[h->a[k]], h->op[k] == 1 ? c->f[h->b[k]] : (const double*)nullptr, h->sums + (size_t)k * h->stride};
    }
    for (int k = T.n; k < QD_HISTORY_MAX; ++k) T.e[k] = QdHistEntry{nullptr, nullptr, nullptr};
    if (group != 0) h->count++;
    if (T.n == 0) return 0;
    QdScope sc(c, "history", true);                       // one launch: timed from the dispatch itself
    const size_t cells = c->geo.cells(), npairs = cells / 2;
    const size_t want = std::max<size_t>(1, (npairs + QD_BLOCK - 1) / QD_BLOCK);
    const int blocks = (int)std::min<size_t>(want, (size_t)std::max(1, c->n_cu) * 8);
    QD_LAUNCH_TIMED(sc, k_hist_accum, dim3(blocks), dim3(QD_BLOCK), c->stream, T, npairs, cells);
    return 0;
}

extern "C" int qd_history_sample(qd_handle c) {
    if (!c) return -1;
    if (!c->history) return qd_fail(c, "qd_history_sample: not configured (qd_history_configure first)");
    if (hist_stale(c)) return qd_fail(c, "qd_history_sample: a history field is no longer an f64 plane (qd_history_configure again)");
    hipSetDevice(c->desc.device);
    if (int rc = qd_history_accumulate(c, 2)) return rc;
    return qd_launch_check(c, "qd_history_sample");
}

extern "C" int qd_history_read(qd_handle c, double* sums, int64_t* count) {
    if (!c || !sums || !count) return -1;
    QdHistory* h = c->history;
    if (!h) return qd_fail(c, "qd_history_read: not configured (qd_history_configure first)");
    hipSetDevice(c->desc.device);
    const size_t row = c->geo.cells() * sizeof(double);
    QD_HIP(c, hipMemcpy2DAsync(sums, row, h->sums, h->stride * sizeof(double), row, (size_t)h->n, hipMemcpyDeviceToHost, c->stream));
    QD_HIP(c, hipStreamSynchronize(c->stream));
    const hipError_t e = hipGetLastError();
    if (e != hipSuccess) return qd_fail(c, "qd_history_read: kernel", e);
    *count = h->count;
    return 0;
}

bool qd_history_planes(const qd_ctx* c, const double** sums, size_t* stride, int* n) {
    const QdHistory* h = c->history;
    if (!h) return false;
    *sums = h->sums; *stride = h->stride; *n = h->n;
    return true;
}

// the inverse of qd_history_read for an exact resume: an open window's sums [n][n_lat][n_lon] and its sample count
extern "C" int qd_history_restore(qd_handle c, const double* sums, int64_t count) {
    if (!c || !sums) return -1;
    QdHistory* h = c->history;
    if (!h) return qd_fail(c, "qd_history_restore: not configured (qd_history_configure first)");
    if (count < 0) return qd_fail(c, "qd_history_restore: negative sample count");
    hipSetDevice(c->desc.device);
    const size_t row = c->geo.cells() * sizeof(double);
    QD_HIP(c, hipMemcpy2DAsync(h->sums, h->stride * sizeof(double), sums, row, row, (size_t)h->n, hipMemcpyHostToDevice, c->stream));
    QD_HIP(c, hipStreamSynchronize(c->stream));                // the host buffer is only borrowed for the call
    h->count = count;
    return 0;
}

extern "C" int qd_history_reset(qd_handle c) {
    if (!c) return -1;
    QdHistory* h = c->history;
    if (!h) return qd_fail(c, "qd_history_reset: not configured (qd_history_configure first)");
    hipSetDevice(c->desc.device);
    QD_HIP(c, hipMemsetAsync(h->sums, 0, (size_t)h->n * h->stride * sizeof(double), c->stream));
    h->count = 0;
    return 0;
}
