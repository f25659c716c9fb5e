// qd_route.hip -- river routing (P014, pygcm/routing.py) on the device.
//
// Per step (routing.py:206-212):   buf += where(net_land, (R * cell_area) * dt, 0)           k_route_accum
// Per event (routing.py:214-312), at most seven launches whatever the network:
//   k_route_walk    level-0 segments, one lane each (wide); levels 1..3 too while they hold >= 2048 segments
//   k_route_levels  the segments of the remaining junction levels, ONE workgroup, one barrier per level
//   k_route_reduce  flow map, the per-cell shares of input / ocean / residual / lake P-E into per-block partials; clears buf
//   k_route_final   ONE workgroup: the partials in a fixed order, the lake storages, the event record
//
// The plan (qingdai_amd/routing.py: build_plan) turns the reference's sequential loop over flow_order into a forest of live
// edges u -> t (t processed after u).  A segment is a chain whose cells after the head have exactly one live predecessor; a
// lane walks it with
//     m(head) = buf(head) (+ m(u)) ... over the head's live predecessors in flow_order position, skipping m(u) <= 0
//     m(next) = m <= 0 ? buf(next) : buf(next) + m
// -- the reference's own f64 additions in its own order, so the flow map is bit-identical.  There are no atomics on the
// accumulation path and every reduction has a fixed order: the results do not depend on scheduling.
// Whole-globe handles only (the network is global; routing across latitude bands is not built).
#include "qd_span.h"

#define QD_ROUTE_BLOCK 256
#define QD_ROUTE_LVL_BLOCK 1024
#define QD_ROUTE_RED_BLOCKS 1024
#define QD_ROUTE_WIDE_LEVELS 4    // at most this many levels go out as wide launches ...
#define QD_ROUTE_WIDE_MIN 2048    // ... and beyond level 0 only while a level holds this many segments
// QD_ROUTE_LOG_W (include/qingdai_hip.h): step, event_dt, ocean_kgps, closure, input, ocean_kg, residual, lake_delta

enum { QR_OCEAN = -1, QR_VOID = -2, QR_DEAD = -3, QR_NOTPROC = -4, QR_LAKE0 = -5 };

struct QdRoute {
    int nlat = 0, nlon = 0; size_t cells = 0;
    int n_seg = 0, n_seg_cells = 0, n_levels = 0, n_jp = 0, n_lakes = 0, pe_lakes = 0;
    std::vector<int> lvl;                 // host copy of level_start
    uint8_t* cflags = nullptr; double* area_row = nullptr; int32_t* code = nullptr;
    int32_t* seg_start = nullptr; int32_t* seg_cells = nullptr; int32_t* level_start = nullptr;
    int32_t* jp_start = nullptr; int32_t* jp_cells = nullptr;
    int32_t* lake_start = nullptr; int32_t* lake_cells = nullptr; double* lake_frac = nullptr;
    double* buf = nullptr; double* M = nullptr; double* flow = nullptr; double* lake_vol = nullptr;
    double* partial = nullptr;
    int red_blocks = 0;
    int64_t steps = 0;                    // accumulations since configure / reset
    const double* last_rec = nullptr;     // the last event's record in the log (a drain leaves it in place)
    QdSpanLane lane;                      // qd_route_schedule: event_dt per step of the next span (0: none); the event log
};

// ------------------------------------------------------------------ kernels
__global__ void __launch_bounds__(QD_ROUTE_BLOCK)
k_route_accum(int nlon, const double* __restrict__ R, const uint8_t* __restrict__ cflags, const double* __restrict__ area_row,
              double dt, double* __restrict__ buf) {
    const int j = blockIdx.x * QD_ROUTE_BLOCK + threadIdx.x;
    if (j >= nlon) return;
    const int i = blockIdx.y;
    const size_t o = (size_t)i * nlon + j;
    const double inc = (R[o] * area_row[i]) * dt;
    buf[o] += (cflags[o] & 1) ? inc : 0.0;
}

// the handed-off m of another lane of the level kernel: an L1-bypassing load (its store was waited for before the barrier)
__device__ __forceinline__ double qr_load_l2(const double* p) {
    const unsigned long long u = __hip_atomic_load((const unsigned long long*)p, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
    return __longlong_as_double((long long)u);
}

__device__ __forceinline__ void qr_walk(int s, const int32_t* __restrict__ seg_start, const int32_t* __restrict__ seg_cells,
                                        const int32_t* __restrict__ jp_start, const int32_t* __restrict__ jp_cells,
                                        const double* __restrict__ buf, double* M) {
    const int a = seg_start[s], b = seg_start[s + 1];
    const int h = seg_cells[a];
    double m = buf[h];
    for (int k = jp_start[s], e = jp_start[s + 1]; k < e; ++k) {
        const double mu = qr_load_l2(M + jp_cells[k]);
        if (!(mu <= 0.0)) m = m + mu;
    }
    M[h] = m;
    // the chain: its cells and their buffers are known in advance -- eight loads in flight, then eight dependent adds
    for (int i = a + 1; i < b; i += 8) {
        const int n = min(8, b - i);
        int cc[8]; double bb[8];
#pragma unroll
        for (int k = 0; k < 8; ++k) cc[k] = k < n ? seg_cells[i + k] : h;
#pragma unroll
        for (int k = 0; k < 8; ++k) bb[k] = buf[cc[k]];
#pragma unroll
        for (int k = 0; k < 8; ++k)
            if (k < n) { m = (m <= 0.0) ? bb[k] : bb[k] + m; M[cc[k]] = m; }
    }
}

__global__ void __launch_bounds__(QD_ROUTE_BLOCK)
k_route_walk(int s0, int n, const int32_t* __restrict__ seg_start, const int32_t* __restrict__ seg_cells, const int32_t* __restrict__ jp_start,
             const int32_t* __restrict__ jp_cells, const double* __restrict__ buf, double* M) {
    const int s = blockIdx.x * QD_ROUTE_BLOCK + threadIdx.x;
    if (s < n) qr_walk(s0 + s, seg_start, seg_cells, jp_start, jp_cells, buf, M);
}

__global__ void __launch_bounds__(QD_ROUTE_LVL_BLOCK)
k_route_levels(int L0, int n_levels, const int32_t* __restrict__ level_start, const int32_t* __restrict__ seg_start,
               const int32_t* __restrict__ seg_cells, const int32_t* __restrict__ jp_start, const int32_t* __restrict__ jp_cells,
               const double* __restrict__ buf, double* M) {
    for (int L = L0; L < n_levels; ++L) {
        const int lo = level_start[L], hi = level_start[L + 1];
        for (int s = lo + (int)threadIdx.x; s < hi; s += QD_ROUTE_LVL_BLOCK) qr_walk(s, seg_start, seg_cells, jp_start, jp_cells, buf, M);
        asm volatile("s_waitcnt vmcnt(0)" ::: "memory");
        __syncthreads();
    }
}

__device__ __forceinline__ double qr_block_sum(double v, double* sh) {
    sh[threadIdx.x] = v;
    __syncthreads();
    for (int w = QD_ROUTE_BLOCK / 2; w > 0; w >>= 1) {
        if ((int)threadIdx.x < w) sh[threadIdx.x] += sh[threadIdx.x + w];
        __syncthreads();
    }
    const double r = sh[0];
    __syncthreads();
    return r;
}

__global__ void __launch_bounds__(QD_ROUTE_BLOCK)
k_route_reduce(int nlon, size_t cells, const int32_t* __restrict__ code, const uint8_t* __restrict__ cflags,
               const double* __restrict__ area_row, const double* __restrict__ M, double* __restrict__ buf, double* __restrict__ flow,
               const double* __restrict__ P, const double* __restrict__ E, int with_pe, double event_dt, double dt_den,
               double* __restrict__ partial) {
    __shared__ double sh[QD_ROUTE_BLOCK];
    double in = 0.0, oc = 0.0, res = 0.0, la = 0.0;
    const size_t stride = (size_t)gridDim.x * QD_ROUTE_BLOCK;
    for (size_t c = (size_t)blockIdx.x * QD_ROUTE_BLOCK + threadIdx.x; c < cells; c += stride) {
        const double b = buf[c];
        const int t = code[c];
        in += b;
        double fl = 0.0;
        if (t == QR_NOTPROC) res += b;
        else {
            const double m = M[c];
            if (m <= 0.0) res += m;                   // skipped: stays in acc
            else {
                fl = m / dt_den;
                if (t == QR_OCEAN) oc += m;
                else if (t == QR_DEAD) res += m;      // delivered to a cell already processed, or never
            }
        }
        flow[c] = fl;
        buf[c] = 0.0;
        if (with_pe && (cflags[c] & 2)) {
            const int i = (int)(c / (size_t)nlon);
            la += ((P[c] - E[c]) * area_row[i]) * event_dt;
        }
    }
    in = qr_block_sum(in, sh); oc = qr_block_sum(oc, sh); res = qr_block_sum(res, sh); la = qr_block_sum(la, sh);
    if (threadIdx.x == 0) {
        double* p = partial + 4 * (size_t)blockIdx.x;
        p[0] = in; p[1] = oc; p[2] = res; p[3] = la;
    }
}

__global__ void __launch_bounds__(QD_ROUTE_BLOCK)
k_route_final(int nb, const double* __restrict__ partial, int n_lakes, const int32_t* __restrict__ lake_start,
              const int32_t* __restrict__ lake_cells, const double* __restrict__ lake_frac, const double* __restrict__ M,
              double* __restrict__ lake_vol, int with_pe, double event_dt, double dt_den, double step, double* __restrict__ rec) {
    __shared__ double sh[QD_ROUTE_BLOCK];
    double s4[4] = {0.0, 0.0, 0.0, 0.0};
    for (int b = threadIdx.x; b < nb; b += QD_ROUTE_BLOCK)
#pragma unroll
        for (int k = 0; k < 4; ++k) s4[k] += partial[4 * (size_t)b + k];
    for (int k = 0; k < 4; ++k) s4[k] = qr_block_sum(s4[k], sh);
    const double lake_add = s4[3];
    const bool pe = with_pe && lake_add != 0.0 && n_lakes > 0;
    // lake storages: the inflow in flow_order position (routing.py:257-260), then the P-E share (routing.py:289-297)
    for (int k = threadIdx.x; k < n_lakes; k += QD_ROUTE_BLOCK) {
        double v = lake_vol[k];
        for (int q = lake_start[k], e = lake_start[k + 1]; q < e; ++q) {
            const double m = M[lake_cells[q]];
            if (!(m <= 0.0)) v += m;
        }
        if (pe) v += lake_frac[k] * lake_add;
        lake_vol[k] = v;
    }
    if (threadIdx.x == 0) {
        const double lake_delta = pe ? lake_add : 0.0;
        const double mass_out = (s4[1] + lake_delta) + s4[2];
        rec[0] = step; rec[1] = event_dt; rec[2] = s4[1] / dt_den; rec[3] = s4[0] - mass_out;
        rec[4] = s4[0]; rec[5] = s4[1]; rec[6] = s4[2]; rec[7] = lake_delta;
    }
}

// ------------------------------------------------------------------ host side
static void qr_free(QdRoute* r) {
    void* ptrs[] = {r->cflags, r->area_row, r->code, r->seg_start, r->seg_cells, r->level_start, r->jp_start, r->jp_cells,
                    r->lake_start, r->lake_cells, r->lake_frac, r->buf, r->M, r->flow, r->lake_vol, r->partial, r->lane.log};
    for (void* p : ptrs) if (p) hipFree(p);
    delete r;
}

void qd_route_release(qd_ctx* c) {
    if (!c->route) return;
    if (c->stream) hipStreamSynchronize(c->stream);
    qr_free(c->route);
    c->route = nullptr;
}

extern "C" int qd_route_free(qd_handle c) {
    if (!c) return -1;
    hipSetDevice(c->desc.device);
    qd_route_release(c);
    return 0;
}

template <class T>
static bool qr_up(qd_ctx* c, T** dst, const T* src, size_t n) {
    const size_t bytes = std::max<size_t>(n, 1) * sizeof(T);
    if (hipMalloc(dst, bytes) != hipSuccess) return false;
    if (n && hipMemcpyAsync(*dst, src, n * sizeof(T), hipMemcpyHostToDevice, c->stream) != hipSuccess) return false;
    return true;
}
template <class T>
static bool qr_zero(qd_ctx* c, T** dst, size_t n) {
    const size_t bytes = std::max<size_t>(n, 1) * sizeof(T);
    return hipMalloc(dst, bytes) == hipSuccess && hipMemsetAsync(*dst, 0, bytes, c->stream) == hipSuccess;
}

// every index the kernels follow is checked here, once: a bad plan is refused, never launched
static const char* qr_check(const qd_route_plan* p, size_t cells) {
    if (p->n_seg < 0 || p->n_seg_cells < 0 || p->n_levels < 0 || p->n_jp < 0 || p->n_lakes < 0) return "negative count";
    if (!p->cflags || !p->area_row || !p->code) return "missing cell arrays";
    if ((p->n_seg > 0) != (p->n_levels > 0)) return "segments without levels";
    if (p->n_seg && (!p->seg_start || !p->seg_cells || !p->level_start || !p->jp_start)) return "missing segment arrays";
    if (p->n_jp && !p->jp_cells) return "missing junction list";
    if (p->n_lakes && (!p->lake_start || !p->lake_frac)) return "missing lake arrays";
    if (p->n_seg_cells > (long long)cells) return "more segment cells than grid cells";
    for (size_t k = 0; k < cells; ++k) {
        const int t = p->code[k];
        if (t >= (long long)cells || t < QR_LAKE0 - (p->n_lakes - 1) || (t <= QR_LAKE0 && p->n_lakes == 0)) return "target code out of range";
    }
    if (p->n_seg) {
        if (p->seg_start[0] != 0 || p->seg_start[p->n_seg] != p->n_seg_cells) return "segment offsets do not span the cell list";
        if (p->jp_start[0] != 0 || p->jp_start[p->n_seg] != p->n_jp) return "junction offsets do not span the list";
        for (int s = 0; s < p->n_seg; ++s)
            if (p->seg_start[s + 1] <= p->seg_start[s] || p->jp_start[s + 1] < p->jp_start[s]) return "segment offsets not increasing";
        if (p->level_start[0] != 0 || p->level_start[p->n_levels] != p->n_seg) return "level offsets do not span the segments";
        for (int L = 0; L < p->n_levels; ++L) if (p->level_start[L + 1] < p->level_start[L]) return "level offsets not increasing";
        for (int k = 0; k < p->n_seg_cells; ++k) if (p->seg_cells[k] < 0 || p->seg_cells[k] >= (long long)cells) return "segment cell out of range";
        for (int k = 0; k < p->n_jp; ++k) if (p->jp_cells[k] < 0 || p->jp_cells[k] >= (long long)cells) return "junction cell out of range";
    }
    if (p->n_lakes) {
        if (p->lake_start[0] != 0) return "lake offsets do not start at 0";
        for (int k = 0; k < p->n_lakes; ++k) if (p->lake_start[k + 1] < p->lake_start[k]) return "lake offsets not increasing";
        const int nl = p->lake_start[p->n_lakes];
        if (nl && !p->lake_cells) return "missing lake cell list";
        for (int k = 0; k < nl; ++k) if (p->lake_cells[k] < 0 || p->lake_cells[k] >= (long long)cells) return "lake cell out of range";
    }
    return nullptr;
}

extern "C" int qd_route_configure(qd_handle c, const qd_route_plan* p, size_t plan_bytes) {
    if (!c || !p) return -1;
    if (plan_bytes != sizeof(qd_route_plan)) return qd_fail(c, "qd_route_configure: plan struct size mismatch");
    if (!qd_whole_globe(c))
        return qd_fail(c, "qd_route_configure: river routing needs a whole-globe handle (world == 1, n_rows == n_lat); "
                          "routing across latitude bands is not supported");
    const size_t cells = (size_t)c->geo.nlat * c->geo.nlon;
    if (p->n_cells != (long long)cells) return qd_fail(c, "qd_route_configure: the plan's cell count is not the grid's");
    if (const char* why = qr_check(p, cells)) {
        static thread_local char msg[160];
        snprintf(msg, sizeof(msg), "qd_route_configure: bad plan (%s)", why);
        return qd_fail(c, msg);
    }
    hipSetDevice(c->desc.device);
    qd_route_release(c);
    QdRoute* r = new QdRoute();
    r->nlat = c->geo.nlat; r->nlon = c->geo.nlon; r->cells = cells;
    r->n_seg = p->n_seg; r->n_seg_cells = p->n_seg_cells; r->n_levels = p->n_levels; r->n_jp = p->n_jp;
    r->n_lakes = p->n_lakes; r->pe_lakes = p->pe_lakes; r->lane.width = QD_ROUTE_LOG_W;
    r->lvl.assign(p->level_start, p->level_start + (p->n_levels ? p->n_levels + 1 : 0));
    r->red_blocks = (int)std::min<size_t>(QD_ROUTE_RED_BLOCKS, (cells + QD_ROUTE_BLOCK - 1) / QD_ROUTE_BLOCK);
    const int nlk = p->n_lakes ? p->lake_start[p->n_lakes] : 0;
    bool ok = qr_up(c, &r->cflags, p->cflags, cells) && qr_up(c, &r->area_row, p->area_row, (size_t)r->nlat) &&
              qr_up(c, &r->code, p->code, cells) &&
              qr_up(c, &r->seg_start, p->seg_start, p->n_seg ? (size_t)p->n_seg + 1 : 0) &&
              qr_up(c, &r->seg_cells, p->seg_cells, (size_t)p->n_seg_cells) &&
              qr_up(c, &r->level_start, p->level_start, p->n_levels ? (size_t)p->n_levels + 1 : 0) &&
              qr_up(c, &r->jp_start, p->jp_start, p->n_seg ? (size_t)p->n_seg + 1 : 0) &&
              qr_up(c, &r->jp_cells, p->jp_cells, (size_t)p->n_jp) &&
              qr_up(c, &r->lake_start, p->lake_start, p->n_lakes ? (size_t)p->n_lakes + 1 : 0) &&
              qr_up(c, &r->lake_cells, p->lake_cells, (size_t)nlk) &&
              qr_up(c, &r->lake_frac, p->lake_frac, (size_t)p->n_lakes) &&
              qr_zero(c, &r->buf, cells) && qr_zero(c, &r->M, cells) && qr_zero(c, &r->flow, cells) &&
              qr_zero(c, &r->lake_vol, (size_t)p->n_lakes) && qr_zero(c, &r->partial, 4 * (size_t)r->red_blocks) &&
              qr_zero(c, &r->lane.log, r->lane.log_doubles());
    // the host arrays are the caller's: the copies finish before this returns
    ok = ok && hipStreamSynchronize(c->stream) == hipSuccess;
    if (!ok) { hipStreamSynchronize(c->stream); qr_free(r); return qd_fail(c, "qd_route_configure: device allocation or upload failed"); }
    c->route = r;
    return 0;
}

extern "C" int qd_route_reset(qd_handle c) {
    if (!c) return -1;
    QdRoute* r = c->route;
    if (!r) return qd_fail(c, "qd_route_reset: no network configured (qd_route_configure first)");
    hipSetDevice(c->desc.device);
    QD_HIP(c, hipMemsetAsync(r->buf, 0, r->cells * sizeof(double), c->stream));
    QD_HIP(c, hipMemsetAsync(r->flow, 0, r->cells * sizeof(double), c->stream));
    if (r->n_lakes) QD_HIP(c, hipMemsetAsync(r->lake_vol, 0, r->n_lakes * sizeof(double), c->stream));
    QD_HIP(c, hipStreamSynchronize(c->stream));
    r->steps = 0; r->lane.reset(); r->last_rec = nullptr;
    return 0;
}

static int qr_accumulate(qd_ctx* c, double dt) {
    QdRoute* r = c->route;
    QdScope sc(c, "route_accum");
    hipLaunchKernelGGL(k_route_accum, dim3((r->nlon + QD_ROUTE_BLOCK - 1) / QD_ROUTE_BLOCK, r->nlat), dim3(QD_ROUTE_BLOCK), 0, c->stream,
                       r->nlon, (const double*)c->f[QD_F_RUNOFF], (const uint8_t*)r->cflags, (const double*)r->area_row, dt, r->buf);
    r->steps += 1;
    return 0;
}

static int qr_event(qd_ctx* c, double event_dt, int with_pe) {
    QdRoute* r = c->route;
    if (r->lane.full()) return qd_fail(c, "qd_route: event log full (drain it with qd_route_events)");
    QdScope sc(c, "route_event");
    const double dt_den = std::max(event_dt, 1e-9);
    const int pe = (with_pe && r->pe_lakes && r->n_lakes > 0) ? 1 : 0;
    int L = 0;
    for (; L < r->n_levels && L < QD_ROUTE_WIDE_LEVELS; ++L) {
        const int s0 = r->lvl[L], ns = r->lvl[L + 1] - r->lvl[L];
        if (L > 0 && ns < QD_ROUTE_WIDE_MIN) break;
        hipLaunchKernelGGL(k_route_walk, dim3((ns + QD_ROUTE_BLOCK - 1) / QD_ROUTE_BLOCK), dim3(QD_ROUTE_BLOCK), 0, c->stream,
                           s0, ns, (const int32_t*)r->seg_start, (const int32_t*)r->seg_cells, (const int32_t*)r->jp_start,
                           (const int32_t*)r->jp_cells, (const double*)r->buf, r->M);
    }
    if (L < r->n_levels)
        hipLaunchKernelGGL(k_route_levels, dim3(1), dim3(QD_ROUTE_LVL_BLOCK), 0, c->stream, L, r->n_levels, (const int32_t*)r->level_start,
                           (const int32_t*)r->seg_start, (const int32_t*)r->seg_cells, (const int32_t*)r->jp_start,
                           (const int32_t*)r->jp_cells, (const double*)r->buf, r->M);
    hipLaunchKernelGGL(k_route_reduce, dim3(r->red_blocks), dim3(QD_ROUTE_BLOCK), 0, c->stream, r->nlon, r->cells,
                       (const int32_t*)r->code, (const uint8_t*)r->cflags, (const double*)r->area_row, (const double*)r->M, r->buf,
                       r->flow, (const double*)c->f[QD_F_PRECIP], (const double*)c->f[QD_F_EFLUX], pe, event_dt, dt_den, r->partial);
    double* rec = r->lane.next();
    hipLaunchKernelGGL(k_route_final, dim3(1), dim3(QD_ROUTE_BLOCK), 0, c->stream, r->red_blocks, (const double*)r->partial, r->n_lakes,
                       (const int32_t*)r->lake_start, (const int32_t*)r->lake_cells, (const double*)r->lake_frac, (const double*)r->M,
                       r->lake_vol, pe, event_dt, dt_den, (double)r->steps, rec);
    r->last_rec = rec;
    return 0;
}

extern "C" int qd_route_accumulate(qd_handle c, double dt) {
    if (!c) return -1;
    if (!c->route) return qd_fail(c, "qd_route_accumulate: no network configured (qd_route_configure first)");
    hipSetDevice(c->desc.device);
    qr_accumulate(c, dt);
    return qd_launch_check(c, "qd_route_accumulate");
}

extern "C" int qd_route_event(qd_handle c, double event_dt, int with_pe) {
    if (!c) return -1;
    if (!c->route) return qd_fail(c, "qd_route_event: no network configured (qd_route_configure first)");
    hipSetDevice(c->desc.device);
    if (int rc = qr_event(c, event_dt, with_pe)) return rc;
    return qd_launch_check(c, "qd_route_event");
}

static QdSpanLane* qr_lane(qd_ctx* c) { return c && c->route ? &c->route->lane : nullptr; }

extern "C" int qd_route_schedule(qd_handle c, int n, const double* event_dt) {
    return qd_lane_schedule(c, qr_lane(c), n, event_dt, "qd_route_schedule", "no network configured (qd_route_configure first)");
}

QdSpanLane* qd_route_span_begin(qd_ctx* c, int n) {
    static const QdSpanTexts T = {
        "qd_step_n: river routing (bit7) needs a whole-globe handle; routing across latitude bands is not supported",
        "qd_step_n: bit7 set but qd_route_configure has not been called",
        "qd_step_n: bit7 needs a qd_route_schedule of exactly n steps before the span",
        "qd_step_n: the span's routing events would overflow the event log (drain it first)"};
    return qd_lane_span_begin(c, qr_lane(c), n, T);
}

int qd_route_step_impl(qd_ctx* c, double dt, int s) {
    qr_accumulate(c, dt);
    const double ev = c->route->lane.at(s);
    return ev != 0.0 ? qr_event(c, ev, 1) : 0;
}

bool qd_route_planes(const qd_ctx* c, const double** buf, const double** flow, const double** lakes, int* n_lakes) {
    const QdRoute* r = c->route;
    if (!r) return false;
    *buf = r->buf; *flow = r->flow; *lakes = r->lake_vol; *n_lakes = r->n_lakes;
    return true;
}

// the inverse of qd_route_download for an exact resume: buffer and flow map [cells], lake volumes [n_lakes] (may be null without
// lakes), the accumulations so far.  The event log and the schedule are left alone
extern "C" int qd_route_restore(qd_handle c, const double* buffer, const double* flow, const double* lakes, int64_t steps) {
    if (!c || !buffer || !flow) return -1;
    QdRoute* r = c->route;
    if (!r) return qd_fail(c, "qd_route_restore: no network configured (qd_route_configure first)");
    if (r->n_lakes > 0 && !lakes) return qd_fail(c, "qd_route_restore: the network has lakes and no lake volumes were given");
    if (steps < 0) return qd_fail(c, "qd_route_restore: negative step count");
    hipSetDevice(c->desc.device);
    QD_HIP(c, hipMemcpyAsync(r->buf, buffer, r->cells * sizeof(double), hipMemcpyHostToDevice, c->stream));
    QD_HIP(c, hipMemcpyAsync(r->flow, flow, r->cells * sizeof(double), hipMemcpyHostToDevice, c->stream));
    if (r->n_lakes > 0) QD_HIP(c, hipMemcpyAsync(r->lake_vol, lakes, (size_t)r->n_lakes * sizeof(double), hipMemcpyHostToDevice, c->stream));
    QD_HIP(c, hipStreamSynchronize(c->stream));                // the host buffers are only borrowed for the call
    r->steps = steps;
    return 0;
}

const double* qd_route_flow(const qd_ctx* c) { return c->route ? c->route->flow : nullptr; }
const double* qd_route_last_record(const qd_ctx* c) { return c->route ? c->route->last_rec : nullptr; }

extern "C" int qd_route_download(qd_handle c, int which, double* host, size_t n) {
    if (!c || !host) return -1;
    QdRoute* r = c->route;
    if (!r) return qd_fail(c, "qd_route_download: no network configured");
    const double* src = which == 0 ? r->flow : which == 1 ? r->lake_vol : which == 2 ? r->buf : nullptr;
    const size_t want = which == 1 ? (size_t)r->n_lakes : r->cells;
    if (!src) return qd_fail(c, "qd_route_download: which is 0 (flow map), 1 (lake volumes) or 2 (buffer)");
    if (n != want) return qd_fail(c, "qd_route_download: element count does not match");
    hipSetDevice(c->desc.device);
    if (n) QD_HIP(c, hipMemcpyAsync(host, src, n * sizeof(double), hipMemcpyDeviceToHost, c->stream));
    QD_HIP(c, hipStreamSynchronize(c->stream));
    return 0;
}

extern "C" int qd_route_events(qd_handle c, double* out, int max, int* n) {
    return qd_lane_drain(c, qr_lane(c), out, max, n, "qd_route_events", "no network configured");
}
