// qd_eddy.hip -- eddy statistics: time sums of products of two fields, accumulated as a span lane, gfx950 (QD_EDDY).
//
// THE DEFINITION (qingdai_amd/eddy.py: accumulate_reference restates it bit for bit; there is no third statement).
// A configuration names F <= QD_EDDY_MAX_FIELDS distinct f64 planes a_0 .. a_{F-1} and P <= QD_EDDY_MAX_PAIRS pairs (p_k, q_k) of
// indices into that list; p == q is a variance.  Resident state, every plane [n_lat][n_lon] f64: anchors r[F], first-moment sums
// S[F], pair sums C[P]; the sample count is a host integer.  One sample, per cell, all in f64, every operation rounded on its own
// (this build has contraction off: no fused multiply-add):
//     the first sample of a window       r_f = a_f                       for every field
//     every sample (the first included)  d_f = a_f - r_f                 one rounding
//                                        S_f = S_f + d_f
//                                        C_k = C_k + (d_p * d_q)         the product rounded, then the add
// No compensation and no special case for a non-finite value: inf - inf is NaN and stays.  The first sample adds exact zeros to
// finite cells.  The anchor is there for accuracy: a covariance does not change when a constant is taken from a field, and sums of
// deviations from a nearby value do not cancel the way sum(ab) - sum(a) sum(b) / N does for a field with mean 288 and variance 1.
// A cell of a plane has one writer and the adds of a window come in step order, so the state does not depend on how a run is cut
// into spans, nor on span lane or class seam (qd_eddy_sample).
//
// A sample of step s is what qd_download returns after a span that ends with step s: the lane samples behind the step's last launch,
// where history's late group is sampled.  PRECIP, the one field sampled in front of the ocean step, is refused: a product across the
// two places has no meaning.  One launch per sampled step, none otherwise.
//
// k_eddy_accum: grid-stride over PAIRS of cells, 16-byte loads and stores per lane (every source is an allocation of its own, the
// lane's planes have an even stride), a scalar tail for the last cell of an odd grid.  Every source and every anchor is loaded once
// per cell and sample; the deviations d_f are staged in LDS as [field][thread] -- a thread reads back only what it wrote, so there
// is no barrier in the main loop -- and the pair loop, whose (p, q) are run-time values, reads them from there (a register array
// indexed by a run-time value would live in scratch).  The table of pointers and pair indices comes by value in the kernel arguments
// and is rebuilt from c->f[] at every launch: the step swaps field pointers.  Up to QD_EDDY_UNROLL fields (their source, anchor and
// sum: 12 loads, k_hist_accum's depth) and then up to QD_EDDY_UNROLL pair sums are in flight before the first use.  The kernel is instantiated for F
// rounded up to 2, 4, 8, 16, which sizes the LDS (16 fields: 128 threads per workgroup, 32 KiB).  No atomics.
//
// k_eddy_zonal (a window's end, not on the step path): per pair k and row j the sums over all n_lon columns of S_p, S_q, C_k and
// S_p * S_q (the product rounded), one wavefront per (pair, row): lane l owns the cells 128 m + 2 l and 128 m + 2 l + 1, m = 0, 1, ...,
// and adds them in ascending order into accumulators that start at +0.0; then the five halvings of qd_blockred.h -- the row stage of
// qd_series.hip, so series.reduce_reference's order is this one's.
#include "qd_span.h"
#include "qd_entry.h"
#include "qd_blockred.h"
#include <algorithm>
#include <string>

#define QD_EDDY_UNROLL 4

struct QdEddyTab {
    const double* a[QD_EDDY_MAX_FIELDS];     // the sources, as c->f[] stands at this launch
    double* r; double* S; double* C;         // [F][stride], [F][stride], [P][stride]
    size_t stride;                           // cells rounded up to even
    int F, P, first;                         // first != 0: the window's first sample stores the anchors
    int pq[QD_EDDY_MAX_PAIRS];               // p | q << 8: whole dwords, which a wave-uniform index reads with a scalar load
    __host__ __device__ int p(int k) const { return pq[k] & 255; }
    __host__ __device__ int q(int k) const { return pq[k] >> 8; }
};

template <int FT, int BLK>
__global__ void __launch_bounds__(BLK)
k_eddy_accum(QdEddyTab T, size_t npairs, size_t cells) {
    __shared__ double2 sd[FT][BLK];                      // d_f of this thread's cell pair
    const int tid = threadIdx.x;
    const size_t gstride = (size_t)gridDim.x * BLK, half = T.stride / 2;
    constexpr int UF = FT < QD_EDDY_UNROLL ? FT : QD_EDDY_UNROLL;
    for (size_t i = (size_t)blockIdx.x * BLK + tid; i < npairs; i += gstride) {
        for (int f0 = 0; f0 < T.F; f0 += UF) {
            double2 a[UF], r[UF], s[UF];
#pragma unroll
            for (int k = 0; k < UF; ++k) {
                if (f0 + k < T.F) {
                    a[k] = reinterpret_cast<const double2*>(T.a[f0 + k])[i];
                    r[k] = reinterpret_cast<const double2*>(T.r)[(size_t)(f0 + k) * half + i];
                    s[k] = reinterpret_cast<const double2*>(T.S)[(size_t)(f0 + k) * half + i];
                }
            }
#pragma unroll
            for (int k = 0; k < UF; ++k) {
                if (f0 + k < T.F) {
                    // (the anchor is loaded on a window's first sample too and dropped here: a choice between a register and a
                    // load would put the register array into scratch)
                    const double2 rr = T.first ? a[k] : r[k];
                    double2 d;
                    d.x = a[k].x - rr.x;
                    d.y = a[k].y - rr.y;
                    sd[f0 + k][tid] = d;
                    s[k].x = s[k].x + d.x;
                    s[k].y = s[k].y + d.y;
                    reinterpret_cast<double2*>(T.S)[(size_t)(f0 + k) * half + i] = s[k];
                    if (T.first) reinterpret_cast<double2*>(T.r)[(size_t)(f0 + k) * half + i] = a[k];
                }
            }
        }
        for (int k0 = 0; k0 < T.P; k0 += QD_EDDY_UNROLL) {
            double2 cs[QD_EDDY_UNROLL];
#pragma unroll
            for (int k = 0; k < QD_EDDY_UNROLL; ++k)
                if (k0 + k < T.P) cs[k] = reinterpret_cast<const double2*>(T.C)[(size_t)(k0 + k) * half + i];
#pragma unroll
            for (int k = 0; k < QD_EDDY_UNROLL; ++k) {
                if (k0 + k < T.P) {
                    const double2 dp = sd[T.p(k0 + k)][tid], dq = sd[T.q(k0 + k)][tid];
                    cs[k].x = cs[k].x + dp.x * dq.x;
                    cs[k].y = cs[k].y + dp.y * dq.y;
                    reinterpret_cast<double2*>(T.C)[(size_t)(k0 + k) * half + i] = cs[k];
                }
            }
        }
    }
    // odd cell count: the last cell; thread f takes field f, then thread k pair k (both below BLK), d in the first LDS column.  The
    // loops keep the table's index wave-uniform: a per-thread index into the kernel arguments would copy them to scratch
    if ((cells & 1) && blockIdx.x == 0) {
        const size_t o = cells - 1;
        __syncthreads();                                 // the main loop's reads of column 0 are over
        for (int f = 0; f < T.F; ++f) {
            if (tid == f) {
                double* S = T.S + (size_t)f * T.stride + o;
                double* R = T.r + (size_t)f * T.stride + o;
                const double a = T.a[f][o], r0 = *R;
                const double r = T.first ? a : r0;
                const double d = a - r;
                sd[f][0].x = d;
                *S = *S + d;
                if (T.first) *R = a;
            }
        }
        __syncthreads();
        for (int k = 0; k < T.P; ++k) {
            if (tid == k) {
                double* C = T.C + (size_t)k * T.stride + o;
                *C = *C + sd[T.p(k)][0].x * sd[T.q(k)][0].x;
            }
        }
    }
}

// one wavefront per (pair, row); QD_BLOCK / 64 of them in a workgroup
__global__ void __launch_bounds__(QD_BLOCK)
k_eddy_zonal(QdEddyTab T, int nlat, int nlon, double* __restrict__ out) {
    const int lane = threadIdx.x & 63;
    const size_t w = (size_t)blockIdx.x * (QD_BLOCK / 64) + (threadIdx.x >> 6);
    if (w >= (size_t)T.P * nlat) return;                 // whole waves leave: no barrier follows
    const int k = (int)(w / nlat), j = (int)(w % nlat);
    const double* __restrict__ sp = T.S + (size_t)T.p(k) * T.stride + (size_t)j * nlon;
    const double* __restrict__ sq = T.S + (size_t)T.q(k) * T.stride + (size_t)j * nlon;
    const double* __restrict__ ck = T.C + (size_t)k * T.stride + (size_t)j * nlon;
    double ap = 0.0, aq = 0.0, ac = 0.0, ax = 0.0;
    for (int c0 = 2 * lane; c0 < nlon; c0 += 128) {
        const bool two = c0 + 1 < nlon;
        const double p0 = sp[c0], q0 = sq[c0], x0 = ck[c0];
        const double p1 = two ? sp[c0 + 1] : 0.0, q1 = two ? sq[c0 + 1] : 0.0, x1 = two ? ck[c0 + 1] : 0.0;
        ap = ap + p0; aq = aq + q0; ac = ac + x0; ax = ax + p0 * q0;
        if (two) { ap = ap + p1; aq = aq + q1; ac = ac + x1; ax = ax + p1 * q1; }
    }
    ap = qd_wave_sum(ap); aq = qd_wave_sum(aq); ac = qd_wave_sum(ac); ax = qd_wave_sum(ax);
    if (lane == 0) {
        double* o = out + (size_t)k * QD_EDDY_ZONAL_SUMS * nlat + j;
        o[0] = ap; o[(size_t)nlat] = aq; o[(size_t)2 * nlat] = ac; o[(size_t)3 * nlat] = ax;
    }
}

struct QdEddy {
    int F = 0, P = 0;
    int field[QD_EDDY_MAX_FIELDS];
    unsigned char p[QD_EDDY_MAX_PAIRS], q[QD_EDDY_MAX_PAIRS];
    bool lazy = false;                // a field is one of the lazily stored diagnostics (QD_LAZY_DIAG)
    double* planes = nullptr;         // [F anchors][F sums][P pair sums], each of `stride` doubles
    double* zonal = nullptr;          // [P][QD_EDDY_ZONAL_SUMS][n_lat], the result of k_eddy_zonal
    size_t stride = 0;                // cells rounded up to even: every plane starts 16-byte aligned
    int64_t count = 0;                // samples in the sums
    QdSpanLane lane;                  // width 0: no log

    double* anchors() const { return planes; }
    double* sums() const { return planes + (size_t)F * stride; }
    double* pair_sums() const { return planes + (size_t)2 * F * stride; }
    size_t doubles() const { return (size_t)(2 * F + P) * stride; }
    // the ecology may have turned a selected map into an f32 slab since the configure (qd_eco_params.map_f32)
    bool stale(const qd_ctx* c) const {
        for (int f = 0; f < F; ++f) if (!hist_plane(c, field[f])) return true;
        return false;
    }
};

static const char* const EDDY_MISSING = "eddy: not configured (qd_eddy_configure first)";
static const char* const EDDY_STALE = "eddy: a field is no longer an f64 plane (qd_eddy_configure again)";
static QdSpanLane* eddy_lane(qd_ctx* c) { return c && c->eddy ? &c->eddy->lane : nullptr; }

void qd_eddy_release(qd_ctx* c) {
    QdEddy* e = c->eddy;
    if (!e) return;
    if (c->stream) hipStreamSynchronize(c->stream);
    if (e->planes) hipFree(e->planes);
    if (e->zonal) hipFree(e->zonal);
    delete e;
    c->eddy = nullptr;
}

extern "C" int qd_eddy_configure(qd_handle c, int n_fields, const int32_t* fields, int n_pairs, const int32_t* p, const int32_t* q) {
    if (!c || n_fields < 0 || n_pairs < 0 || (n_fields && (!fields || (n_pairs && (!p || !q))))) return -1;
    if (!qd_whole_globe(c))
        return qd_fail(c, "eddy: the eddy statistics need a whole-globe handle (world == 1, n_rows == n_lat); latitude bands are not supported");
    QdEddy t;
    if (n_fields > QD_EDDY_MAX_FIELDS) return qd_fail(c, "eddy: at most 16 fields");
    if (n_pairs > QD_EDDY_MAX_PAIRS) return qd_fail(c, "eddy: at most 32 pairs");
    if (n_fields && n_pairs == 0) return qd_fail(c, "eddy: no pair (fields without a pair accumulate nothing)");
    for (int f = 0; f < n_fields; ++f) {
        if (!hist_plane(c, fields[f])) return qd_fail(c, ("eddy: field " + std::to_string(f) + " is not an f64 plane").c_str());
        if (fields[f] == QD_F_PRECIP)
            return qd_fail(c, "eddy: PRECIP is sampled in front of the ocean step, every other field behind the step's last launch: "
                              "a product across the two places has no meaning");
        for (int g = 0; g < f; ++g) if (fields[g] == fields[f]) return qd_fail(c, ("eddy: field " + std::to_string(f) + " is named twice").c_str());
        t.field[f] = fields[f];
        t.lazy = t.lazy || hist_lazy_field(fields[f]);
    }
    for (int k = 0; k < n_pairs && n_fields; ++k) {
        if (p[k] < 0 || p[k] >= n_fields || q[k] < 0 || q[k] >= n_fields)
            return qd_fail(c, ("eddy: pair " + std::to_string(k) + " has an index outside the " + std::to_string(n_fields) + " fields").c_str());
        for (int m = 0; m < k; ++m)
            if ((p[m] == p[k] && q[m] == q[k]) || (p[m] == q[k] && q[m] == p[k]))
                return qd_fail(c, ("eddy: pair " + std::to_string(k) + " is pair " + std::to_string(m) + " again (the order of the two fields does not count)").c_str());
        t.p[k] = (unsigned char)p[k]; t.q[k] = (unsigned char)q[k];
    }
    hipSetDevice(c->desc.device);
    qd_eddy_release(c);
    if (n_fields == 0) return 0;
    t.F = n_fields; t.P = n_pairs;
    QdEddy* e = new QdEddy(t);
    e->stride = (c->geo.cells() + 1) & ~(size_t)1;
    const size_t bytes = e->doubles() * sizeof(double), zb = (size_t)e->P * QD_EDDY_ZONAL_SUMS * c->geo.nlat * sizeof(double);
    const bool ok = hipMalloc(&e->planes, bytes) == hipSuccess && hipMalloc(&e->zonal, zb) == hipSuccess &&
                    hipMemsetAsync(e->planes, 0, bytes, c->stream) == hipSuccess && hipStreamSynchronize(c->stream) == hipSuccess;
    c->eddy = e;
    if (!ok) { qd_eddy_release(c); return qd_fail(c, "eddy: device allocation failed"); }
    return 0;
}

extern "C" int qd_eddy_schedule(qd_handle c, int steps, const int32_t* sample) {
    return qd_lane_schedule(c, eddy_lane(c), steps, sample, "eddy", "not configured (qd_eddy_configure first)");
}

bool qd_eddy_scheduled(const qd_ctx* c) { return c->eddy && !c->eddy->lane.sched.empty(); }
bool qd_eddy_reads_lazy(const qd_ctx* c) { return c->eddy && c->eddy->lazy; }

QdSpanLane* qd_eddy_span_begin(qd_ctx* c, int n) {
    static const QdSpanTexts T = {
        "eddy: qd_step_n: the eddy statistics need a whole-globe handle; latitude bands are not supported",
        "eddy: qd_step_n: qd_eddy_configure has not been called",
        "eddy: qd_step_n: a qd_eddy_schedule must cover exactly the n steps of the span",
        "eddy: qd_step_n: a span samples the eddy statistics at most QD_SPAN_LOG_CAP times"};
    QdSpanLane* l = qd_lane_span_begin(c, eddy_lane(c), n, T, nullptr, c->eddy && c->eddy->stale(c) ? EDDY_STALE : nullptr);
    if (!l && c->eddy) c->eddy->lane.clear_schedule();            // refused: the span guard never sees this lane, and a schedule serves one span
    return l;
}

static QdEddyTab eddy_table(const qd_ctx* c, const QdEddy* e) {
    QdEddyTab T;
    for (int f = 0; f < QD_EDDY_MAX_FIELDS; ++f) T.a[f] = f < e->F ? c->f[e->field[f]] : nullptr;
    T.r = e->anchors(); T.S = e->sums(); T.C = e->pair_sums();
    T.stride = e->stride; T.F = e->F; T.P = e->P; T.first = e->count == 0 ? 1 : 0;
    for (int k = 0; k < QD_EDDY_MAX_PAIRS; ++k) T.pq[k] = k < e->P ? (int)e->p[k] | ((int)e->q[k] << 8) : 0;
    return T;
}

template <int FT, int BLK>
static void eddy_launch(qd_ctx* c, QdScope& sc, const QdEddyTab& T, size_t npairs, size_t cells) {
    const size_t want = std::max<size_t>(1, (npairs + BLK - 1) / BLK);
    const int blocks = (int)std::min<size_t>(want, (size_t)std::max(1, c->n_cu) * 8 * (QD_BLOCK / BLK));
    QD_LAUNCH_TIMED(sc, (k_eddy_accum<FT, BLK>), dim3(blocks), dim3(BLK), c->stream, T, npairs, cells);
}

// one sample of every field and pair from the planes as they stand (the span's late position, and the class seam)
int qd_eddy_accumulate(qd_ctx* c) {
    QdEddy* e = c->eddy;
    const QdEddyTab T = eddy_table(c, e);
    e->count++;
    QdScope sc(c, "eddy", true);                          // one launch: timed from the dispatch itself
    const size_t cells = c->geo.cells(), npairs = cells / 2;
    if (e->F <= 2) eddy_launch<2, QD_BLOCK>(c, sc, T, npairs, cells);
    else if (e->F <= 4) eddy_launch<4, QD_BLOCK>(c, sc, T, npairs, cells);
    else if (e->F <= 8) eddy_launch<8, QD_BLOCK>(c, sc, T, npairs, cells);
    else eddy_launch<16, QD_BLOCK / 2>(c, sc, T, npairs, cells);
    return 0;
}

extern "C" int qd_eddy_sample(qd_handle c) {
    if (!c) return -1;
    if (!c->eddy) return qd_fail(c, EDDY_MISSING);
    if (c->eddy->stale(c)) return qd_fail(c, EDDY_STALE);
    hipSetDevice(c->desc.device);
    if (int rc = qd_eddy_accumulate(c)) return rc;
    return qd_launch_check(c, "eddy: qd_eddy_sample");
}

// the three groups of planes between the device (stride) and the host (cells), either way
static int eddy_copy(qd_ctx* c, QdEddy* e, double* anchors, double* sums, double* pair_sums, bool to_host) {
    const size_t row = c->geo.cells() * sizeof(double), pitch = e->stride * sizeof(double);
    struct { double* host; double* dev; int n; } part[3] = {{anchors, e->anchors(), e->F}, {sums, e->sums(), e->F}, {pair_sums, e->pair_sums(), e->P}};
    for (auto& g : part) {
        if (to_host) QD_HIP(c, hipMemcpy2DAsync(g.host, row, g.dev, pitch, row, (size_t)g.n, hipMemcpyDeviceToHost, c->stream));
        else QD_HIP(c, hipMemcpy2DAsync(g.dev, pitch, g.host, row, row, (size_t)g.n, hipMemcpyHostToDevice, c->stream));
    }
    QD_HIP(c, hipStreamSynchronize(c->stream));               // a host buffer is only borrowed for the call
    return 0;
}

extern "C" int qd_eddy_read(qd_handle c, double* anchors, double* sums, double* pair_sums, int64_t* count) {
    if (!c) return -1;
    QdEddy* e = c->eddy;
    if (!e) return qd_fail(c, EDDY_MISSING);
    if (!anchors || !sums || !pair_sums || !count) return -1;
    hipSetDevice(c->desc.device);
    if (int rc = eddy_copy(c, e, anchors, sums, pair_sums, true)) return rc;
    const hipError_t err = hipGetLastError();
    if (err != hipSuccess) return qd_fail(c, "eddy: qd_eddy_read: kernel", err);
    *count = e->count;
    return 0;
}

extern "C" int qd_eddy_restore(qd_handle c, const double* anchors, const double* sums, const double* pair_sums, int64_t count) {
    if (!c) return -1;
    QdEddy* e = c->eddy;
    if (!e) return qd_fail(c, EDDY_MISSING);
    if (!anchors || !sums || !pair_sums) return -1;
    if (count < 0) return qd_fail(c, "eddy: qd_eddy_restore: negative sample count");
    hipSetDevice(c->desc.device);
    if (int rc = eddy_copy(c, e, const_cast<double*>(anchors), const_cast<double*>(sums), const_cast<double*>(pair_sums), false)) return rc;
    e->count = count;
    return 0;
}

extern "C" int qd_eddy_zonal(qd_handle c, double* out) {
    if (!c) return -1;
    QdEddy* e = c->eddy;
    if (!e) return qd_fail(c, EDDY_MISSING);
    if (!out) return -1;
    hipSetDevice(c->desc.device);
    const int nlat = c->geo.nlat, nlon = c->geo.nlon;
    const size_t waves = (size_t)e->P * nlat, per = QD_BLOCK / 64;
    {
        QdScope sc(c, "eddy_zonal", true);
        QD_LAUNCH_TIMED(sc, k_eddy_zonal, dim3((unsigned)((waves + per - 1) / per)), dim3(QD_BLOCK), c->stream, eddy_table(c, e), nlat, nlon, e->zonal);
    }
    QD_HIP(c, hipMemcpyAsync(out, e->zonal, waves * QD_EDDY_ZONAL_SUMS * sizeof(double), hipMemcpyDeviceToHost, c->stream));
    QD_HIP(c, hipStreamSynchronize(c->stream));
    return qd_launch_check(c, "eddy: qd_eddy_zonal");
}

bool qd_eddy_planes(const qd_ctx* c, const double** anchors, size_t* n_anchors, const double** sums, size_t* n_sums) {
    const QdEddy* e = c->eddy;
    if (!e) return false;
    *anchors = e->anchors(); *n_anchors = (size_t)e->F * e->stride;
    *sums = e->sums(); *n_sums = (size_t)(e->F + e->P) * e->stride;
    return true;
}

extern "C" int qd_eddy_reset(qd_handle c) {
    if (!c) return -1;
    QdEddy* e = c->eddy;
    if (!e) return qd_fail(c, EDDY_MISSING);
    hipSetDevice(c->desc.device);
    QD_HIP(c, hipMemsetAsync(e->planes, 0, e->doubles() * sizeof(double), c->stream));
    e->count = 0;
    e->lane.clear_schedule();
    return 0;
}
