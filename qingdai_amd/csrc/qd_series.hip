// qd_series.hip -- per-step time series and zonal means: selected fields reduced to one record per sampled step, as a span lane,
// gfx950 (QD_SERIES).
//
// An entry is what a history entry is (qd_entry.h): an f64 plane (op 0) or sqrt(a*a + b*b) of two planes (op 1).  On every sampled
// step of a qd_step_n span (qd_series_schedule: one value per step, non-zero = sampled) every entry is reduced to
//     mean, min, max, nan_count [, zonal[n_lat]]
// and the n entries' results, in configure order, are ONE record of width = n (4 + (zonal ? n_lat : 0)) doubles in the lane's device
// log, which holds QD_SERIES_LOG_CAP records between two drains (qd_series_log).  No flag bit: a schedule given before the span turns
// the lane on.  Groups and sampling places are history's: the entries that read PRECIP are reduced in front of the ocean step, every
// other entry behind the step's last launch; both launches write into the one record slot the step reserved.  A sampled step adds at
// most these two launches (one per group), an unsampled step none.  Whole-globe handles only.
//
// ORDER IS THE INVARIANT (qd_blockred.h).  A record is a function of the planes' values and (n_lat, n_lon) alone -- not of the CU
// count, the grid size, the number or order of the other entries, zonal on or off, how a run is cut into spans, span lane or class
// seam.  x: the entry's value in a cell; w_j = max(cos lat_j, 0) as the host uploaded it (qd_series_configure: w_row).
//   row stage     ONE wavefront per (entry, row j).  Lane l owns the cells 128 k + 2 l and 128 k + 2 l + 1, k = 0, 1, ..., and takes
//                 them in ascending order into ONE accumulator each of: acc (from +0.0: acc = acc + x), mn (from NaN: fmin), mx (from
//                 NaN: fmax), cnt (x != x, an integer).  Then the five-halving wave reductions of qd_blockred.h (qd_wave_sum /
//                 qd_wave_fmin / qd_wave_fmax; the integer count the same way) -> S_j, mn_j, mx_j, cnt_j in lane 0.
//                 Loads are 16 bytes per lane where the row starts 16-byte aligned (even n_lon; every plane is an allocation of its
//                 own), 8 bytes otherwise; a lane owns the same cells in both forms, so the bits are the same.  Four rounds k are in
//                 flight before the first add.
//                 zonal[j] = S_j / n_lon.
//   second stage  ONE wavefront per entry, over the rows: lane l takes j = l, l + 64, ... in ascending order into num (+0.0: num =
//                 num + w_j * S_j, the product rounded, no FMA), W (+0.0: W = W + w_j), mn, mx (from NaN: fmin / fmax), cnt; then
//                 the same wave reductions (the qd_planes_by_wave form).
//                 mean = num / ((double)n_lon * W)        min = mn, max = mx (NaN when every cell is NaN)        nan_count = cnt
//   A NaN cell makes its row's zonal and the mean NaN; +-inf propagates as IEEE gives it.  min and max are exact VALUES: the sign
//   of a zero result among zeros of both signs is the hardware's fmin / fmax choice and is not part of the contract.
//
// ONE launch per group.  QD_BLOCK threads = 4 row waves per workgroup, ceil(n_lat / 4) workgroups per entry (a workgroup's rows are
// one entry's); each wave's lane 0 stores its four row results write-through (agent-scope stores) into `part` and drains them, the
// workgroup meets at ONE barrier behind its row work (none inside it), thread 0 takes a ticket of its ENTRY; wave 0 of the workgroup
// that draws an entry's last ticket runs that entry's second stage on agent-scope loads of `part` and puts the ticket back to 0 (the
// hand-off of k_cont_sstadv's eta mean, qd_ocean.hip).  So the entries' second stages run beside one another and beside the other
// entries' row waves, not one after the other in a single workgroup behind everything else.  LDS: the one flag.
// qingdai_amd/series.py: reduce_reference is the NumPy restatement of this order, the only one outside this file.
#include "qd_span.h"
#include "qd_entry.h"
#include "qd_blockred.h"
#include <algorithm>

#define QD_SERIES_ROUNDS 4         // rounds of 128 cells whose loads are in flight together
#define QD_SERIES_NSTAT 4          // mean, min, max, nan_count (include/qingdai_hip.h: QD_SERIES_STATS)
#define QD_SERIES_TICKET_STRIDE 32 // 64-bit words between two entries' tickets: 256 bytes, no two in one cache line
#define QD_SERIES_TICKET_BYTES ((size_t)QD_ENTRY_MAX * QD_SERIES_TICKET_STRIDE * sizeof(unsigned long long))
static_assert(QD_SERIES_MAX_ENTRIES == QD_ENTRY_MAX, "the series table is the shared entry table");
static_assert(QD_SERIES_STATS == QD_SERIES_NSTAT, "the record's leading statistics");

struct QdSeriesEntry { const double* a; const double* b; int slot; int pad_; };       // b == nullptr: op 0; slot: the entry's place in the record
struct QdSeriesTab { QdSeriesEntry e[QD_ENTRY_MAX]; int n; };

__device__ __forceinline__ int qs_wave_sum_int(int x) {
#pragma unroll
    for (int o = 32; o > 0; o >>= 1) x += __shfl_down(x, o, 64);
    return x;
}

// one lane's two cells of round k (cells c0 = 128 k + 2 lane and c0 + 1 of the row that starts at p), in order
__device__ __forceinline__ void qs_take(double x0, double x1, bool v0, bool v1, double& acc, double& mn, double& mx, int& cnt) {
    if (v0) { acc = acc + x0; mn = fmin(mn, x0); mx = fmax(mx, x0); cnt += (x0 != x0) ? 1 : 0; }
    if (v1) { acc = acc + x1; mn = fmin(mn, x1); mx = fmax(mx, x1); cnt += (x1 != x1) ? 1 : 0; }
}

__global__ void __launch_bounds__(QD_BLOCK)
k_series(QdSeriesTab T, int nlat, int nlon, int zonal, const double* __restrict__ wrow, double* part, unsigned long long* ticket,
         double* __restrict__ rec) {
    __shared__ int s_last;
    const int lane = threadIdx.x & 63, wv = threadIdx.x >> 6;
    const int wpe = (nlat + QD_BLOCK / 64 - 1) / (QD_BLOCK / 64);      // workgroups per entry: a workgroup's rows are one entry's
    const int q = blockIdx.x / wpe, j = (blockIdx.x - q * wpe) * (QD_BLOCK / 64) + wv;       // this wave's (entry, row)
    const int stride = QD_SERIES_NSTAT + (zonal ? nlat : 0);
    const QdSeriesEntry E = T.e[q];
    if (j < nlat) {                                             // wave-uniform
        const bool pair = E.b != nullptr;
        const size_t row = (size_t)j * nlon;
        const double* pa = E.a + row;
        const double* pb = pair ? E.b + row : pa;
        double acc = 0.0, mn = NAN, mx = NAN;
        int cnt = 0;
        const bool wide = (nlon & 1) == 0;                      // the row starts 16-byte aligned
        for (int c0 = 2 * lane; c0 < nlon; c0 += 128 * QD_SERIES_ROUNDS) {
            double xa[QD_SERIES_ROUNDS][2], xb[QD_SERIES_ROUNDS][2];
#pragma unroll
            for (int r = 0; r < QD_SERIES_ROUNDS; ++r) {
                const int c = c0 + 128 * r;
                xa[r][0] = xa[r][1] = xb[r][0] = xb[r][1] = 0.0;
                if (wide) {
                    if (c < nlon) {                             // even n_lon: c + 1 < n_lon as well
                        const double2 u = *reinterpret_cast<const double2*>(pa + c);
                        xa[r][0] = u.x; xa[r][1] = u.y;
                        if (pair) { const double2 v = *reinterpret_cast<const double2*>(pb + c); xb[r][0] = v.x; xb[r][1] = v.y; }
                    }
                } else {
                    if (c < nlon) { xa[r][0] = pa[c]; if (pair) xb[r][0] = pb[c]; }
                    if (c + 1 < nlon) { xa[r][1] = pa[c + 1]; if (pair) xb[r][1] = pb[c + 1]; }
                }
            }
#pragma unroll
            for (int r = 0; r < QD_SERIES_ROUNDS; ++r) {
                const int c = c0 + 128 * r;
                qs_take(hist_value(xa[r][0], xb[r][0], pair), hist_value(xa[r][1], xb[r][1], pair), c < nlon, c + 1 < nlon, acc, mn, mx, cnt);
            }
        }
        acc = qd_wave_sum(acc); mn = qd_wave_fmin(mn); mx = qd_wave_fmax(mx); cnt = qs_wave_sum_int(cnt);
        if (lane == 0) {
            double* P = part + (size_t)q * QD_SERIES_NSTAT * nlat + j;
            __hip_atomic_store(P, acc, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
            __hip_atomic_store(P + nlat, mn, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
            __hip_atomic_store(P + 2 * (size_t)nlat, mx, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
            __hip_atomic_store(P + 3 * (size_t)nlat, (double)cnt, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
            if (zonal) rec[(size_t)E.slot * stride + QD_SERIES_NSTAT + j] = acc / (double)nlon;
        }
        asm volatile("s_waitcnt vmcnt(0)" ::: "memory");        // every storing wave drains its write-through stores ...
    }
    __syncthreads();                                            // ... before the workgroup's one ticket, its entry's
    unsigned long long* tk = ticket + (size_t)q * QD_SERIES_TICKET_STRIDE;
    if (threadIdx.x == 0) {
        const unsigned long long t = atomicAdd(tk, 1ull);
        s_last = (t == (unsigned long long)wpe - 1ull) ? 1 : 0;
    }
    __syncthreads();
    if (!s_last || wv != 0) return;
    // second stage: wave 0 of the entry's last workgroup to arrive.  Lane l takes the rows l, l + 64, ... in ascending order; the
    // loads of QD_SERIES_ROUNDS rows per lane are in flight before the first add (a chain of single loads would be a chain of
    // memory latencies)
    const double* P = part + (size_t)q * QD_SERIES_NSTAT * nlat;
    double num = 0.0, W = 0.0, mn = NAN, mx = NAN, cnt = 0.0;
    for (int j0 = lane; j0 < nlat; j0 += 64 * QD_SERIES_ROUNDS) {
        double w[QD_SERIES_ROUNDS], v[QD_SERIES_ROUNDS][QD_SERIES_NSTAT];
#pragma unroll
        for (int r = 0; r < QD_SERIES_ROUNDS; ++r) {
            const int jr = j0 + 64 * r;
            w[r] = 0.0;
#pragma unroll
            for (int k = 0; k < QD_SERIES_NSTAT; ++k) v[r][k] = 0.0;
            if (jr < nlat) {
                w[r] = wrow[jr];
#pragma unroll
                for (int k = 0; k < QD_SERIES_NSTAT; ++k)
                    v[r][k] = __hip_atomic_load(P + (size_t)k * nlat + jr, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
            }
        }
#pragma unroll
        for (int r = 0; r < QD_SERIES_ROUNDS; ++r)
            if (j0 + 64 * r < nlat) {
                num = num + w[r] * v[r][0]; W = W + w[r];
                mn = fmin(mn, v[r][1]); mx = fmax(mx, v[r][2]); cnt = cnt + v[r][3];
            }
    }
    num = qd_wave_sum(num); W = qd_wave_sum(W); mn = qd_wave_fmin(mn); mx = qd_wave_fmax(mx); cnt = qd_wave_sum(cnt);
    if (lane == 0) {
        double* R = rec + (size_t)E.slot * stride;
        R[0] = num / ((double)nlon * W); R[1] = mn; R[2] = mx; R[3] = cnt;
        __hip_atomic_store(tk, 0ull, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
    }
}

// ------------------------------------------------------------------ host side
struct QdSeries : QdEntrySel {        // the entry table (qd_entry.h)
    int zonal = 0;
    double* wrow = nullptr;           // [n_lat] the host's max(cos lat, 0)
    double* part = nullptr;           // [n][4][n_lat] row results of the launch in flight
    unsigned long long* ticket = nullptr;   // [QD_ENTRY_MAX][QD_SERIES_TICKET_STRIDE], one live word per entry, 0 between launches
    double* rec = nullptr;            // the record of the step in progress
    QdSpanLane lane;
};

static QdSpanLane* series_lane(qd_ctx* c) { return c && c->series ? &c->series->lane : nullptr; }

void qd_series_release(qd_ctx* c) {
    QdSeries* s = c->series;
    if (!s) return;
    if (c->stream) hipStreamSynchronize(c->stream);
    void* p[] = {s->wrow, s->part, s->ticket, s->lane.log};
    for (void* q : p) if (q) hipFree(q);
    delete s;
    c->series = nullptr;
}

extern "C" int qd_series_configure(qd_handle c, int n, const int32_t* op, const int32_t* a, const int32_t* b, int zonal, const double* w_row) {
    if (!c || n < 0 || (n && (!op || !a || !w_row))) return -1;
    if (!qd_whole_globe(c))
        return qd_fail(c, "qd_series_configure: the series need a whole-globe handle (world == 1, n_rows == n_lat); "
                          "latitude bands are not supported");
    QdSeries t;
    if (qd_entries_parse(c, "qd_series_configure", n, op, a, b, t)) return -1;
    hipSetDevice(c->desc.device);
    qd_series_release(c);
    if (n == 0) return 0;
    QdSeries* s = new QdSeries(t);
    const int nlat = c->geo.nlat;
    s->zonal = zonal ? 1 : 0;
    s->lane.width = n * (QD_SERIES_NSTAT + (s->zonal ? nlat : 0));
    s->lane.cap = QD_SERIES_LOG_CAP;
    const size_t logb = s->lane.log_doubles() * sizeof(double), partb = (size_t)n * QD_SERIES_NSTAT * nlat * sizeof(double);
    const bool ok = hipMalloc(&s->wrow, (size_t)nlat * sizeof(double)) == hipSuccess && hipMalloc(&s->part, partb) == hipSuccess &&
                    hipMalloc(&s->ticket, QD_SERIES_TICKET_BYTES) == hipSuccess && hipMalloc(&s->lane.log, logb) == hipSuccess &&
                    hipMemcpyAsync(s->wrow, w_row, (size_t)nlat * sizeof(double), hipMemcpyHostToDevice, c->stream) == hipSuccess &&
                    hipMemsetAsync(s->part, 0, partb, c->stream) == hipSuccess && hipMemsetAsync(s->ticket, 0, QD_SERIES_TICKET_BYTES, c->stream) == hipSuccess &&
                    hipMemsetAsync(s->lane.log, 0, logb, c->stream) == hipSuccess && hipStreamSynchronize(c->stream) == hipSuccess;
    c->series = s;
    if (!ok) { qd_series_release(c); return qd_fail(c, "qd_series_configure: device allocation or upload failed"); }
    return 0;
}

extern "C" int qd_series_schedule(qd_handle c, int steps, const int32_t* sample) {
    return qd_lane_schedule(c, series_lane(c), steps, sample, "qd_series_schedule", "not configured (qd_series_configure first)");
}
extern "C" int qd_series_log(qd_handle c, double* out, int max, int* n) {
    return qd_lane_drain(c, series_lane(c), out, max, n, "qd_series_log", "not configured (qd_series_configure first)");
}
extern "C" int qd_series_reset(qd_handle c) {
    if (!c) return -1;
    if (!c->series) return qd_fail(c, "qd_series_reset: not configured (qd_series_configure first)");
    c->series->lane.reset();
    return 0;
}

bool qd_series_scheduled(const qd_ctx* c) { return c->series && !c->series->lane.sched.empty(); }
bool qd_series_reads_lazy(const qd_ctx* c) { return c->series && c->series->lazy; }

QdSpanLane* qd_series_span_begin(qd_ctx* c, int n) {
    static const QdSpanTexts T = {
        "qd_step_n: the series need a whole-globe handle; latitude bands are not supported",
        "qd_step_n: qd_series_configure has not been called",
        "qd_step_n: a qd_series_schedule must cover exactly the n steps of the span",
        "qd_step_n: the span's series records would overflow the log of QD_SERIES_LOG_CAP (drain it with qd_series_log first)"};
    const bool stale = c->series && c->series->stale(c);
    QdSpanLane* l = qd_lane_span_begin(c, series_lane(c), n, T, nullptr,
                                       stale ? "qd_step_n: a series field is no longer an f64 plane (qd_series_configure again)" : nullptr);
    if (!l && c->series) c->series->lane.clear_schedule();        // refused: the span guard never sees this lane, and a schedule serves one span
    return l;
}

// a sampled step begins: its record slot, which the step's groups fill between them (every entry is in one of the two)
int qd_series_begin_step(qd_ctx* c) {
    QdSeries* s = c->series;
    if (s->lane.full()) return qd_fail(c, "qd_step_n: series log full (drain it with qd_series_log)");
    s->rec = s->lane.next();
    return 0;
}

// group 0: the early entries, 1: the late entries, 2: all of them (the class seam) -> the open record slot
int qd_series_reduce(qd_ctx* c, int group) {
    QdSeries* s = c->series;
    QdSeriesTab T;
    T.n = 0;
    for (int k = 0; k < s->n; ++k) {
        if (group != 2 && s->early[k] != (group == 0)) continue;
        T.e[T.n++] = QdSeriesEntry{c->f[s->a[k]], s->op[k] == 1 ? c->f[s->b[k]] : (const double*)nullptr, k, 0};
    }
    for (int k = T.n; k < QD_ENTRY_MAX; ++k) T.e[k] = QdSeriesEntry{nullptr, nullptr, 0, 0};
    if (T.n == 0) return 0;
    QdScope sc(c, "series", true);                        // one launch: timed from the dispatch itself
    const int nlat = c->geo.nlat, blocks = T.n * ((nlat + QD_BLOCK / 64 - 1) / (QD_BLOCK / 64));
    QD_LAUNCH_TIMED(sc, k_series, dim3(blocks), dim3(QD_BLOCK), c->stream, T, nlat, c->geo.nlon, s->zonal, (const double*)s->wrow, s->part,
                    s->ticket, s->rec);
    return 0;
}

extern "C" int qd_series_sample(qd_handle c) {
    if (!c) return -1;
    if (!c->series) return qd_fail(c, "qd_series_sample: not configured (qd_series_configure first)");
    if (c->series->stale(c)) return qd_fail(c, "qd_series_sample: a series field is no longer an f64 plane (qd_series_configure again)");
    if (c->series->lane.full()) return qd_fail(c, "qd_series_sample: series log full (drain it with qd_series_log)");
    hipSetDevice(c->desc.device);
    c->series->rec = c->series->lane.next();
    if (int rc = qd_series_reduce(c, 2)) return rc;
    return qd_launch_check(c, "qd_series_sample");
}
