// qd_digest.hip -- a 64-bit digest of every resident plane in one launch, and the host-side scalars an exact resume has to carry
// (QD_CHECKPOINT, qingdai_amd/checkpoint.py), gfx950.  Nothing the reference has.
//
// The digest of a plane of n elements is
//     D = sum_{i = 0 .. n-1} mix64(w_i + (i + 1) * 0x9E3779B97F4A7C15)   mod 2^64
// w_i: the element's stored bits, zero-extended to 64 (f64: 8 bytes, f32: 4, u8: 1 -- NaN payloads and the sign of zero count); i: the
// element's row-major index in the GLOBAL plane; mix64: the splitmix64 finaliser.  The terms are added as integers, so the value does
// not depend on the grid shape, the wave order or the order in which the workgroups' atomics arrive.
//
// k_state_digest: one launch for a table of up to 64 planes, {pointer, element count, element size} by value in the kernel arguments
// (64 x 16 bytes; k_hist_accum takes its table the same way).  blockIdx.y is the entry; the workgroups of a row walk their entry with
// a grid stride -- f64 planes as PAIRS through 16-byte loads, with one leading element when the plane starts 8 bytes off a 16-byte
// boundary and one trailing element when what is left is odd, both taken by thread 0 of workgroup 0.  Each lane keeps a u64 partial,
// the wave and the workgroup reduce it (qd_blockred.h: qd_block_sum_u64), and thread 0 issues ONE 64-bit atomicAdd per workgroup
// into out[entry], which the launcher zeroes on the stream in front of the launch.  The grid is sized from the CU count.  Every load
// is inside [0, n) of its entry; the kernel stores nothing but the atomic.  Whole-globe handles only.
#include "qd_blockred.h"
#include <algorithm>

#define QD_DIGEST_MAX 64          // entries per call (include/qingdai_hip.h: QD_STATE_DIGEST_MAX)
#define QD_DIGEST_GOLD 0x9E3779B97F4A7C15ull

struct QdDigestEntry { const void* p; unsigned long long n_esz; };       // n_esz: element count << 4 | element size (8, 4, 1)
struct QdDigestTab { QdDigestEntry e[QD_DIGEST_MAX]; };

__host__ __device__ __forceinline__ unsigned long long qd_mix64(unsigned long long z) {
    z ^= z >> 30; z *= 0xBF58476D1CE4E5B9ull;
    z ^= z >> 27; z *= 0x94D049BB133111EBull;
    z ^= z >> 31;
    return z;
}
__device__ __forceinline__ unsigned long long qd_digest_term(unsigned long long w, unsigned long long i) {
    return qd_mix64(w + (i + 1ull) * QD_DIGEST_GOLD);
}

__global__ void __launch_bounds__(QD_BLOCK)
k_state_digest(QdDigestTab T, unsigned long long* __restrict__ out) {
    const QdDigestEntry E = T.e[blockIdx.y];
    const unsigned long long n = E.n_esz >> 4;
    const unsigned int esz = (unsigned int)(E.n_esz & 15ull);
    const unsigned long long stride = (unsigned long long)gridDim.x * QD_BLOCK;
    const unsigned long long t0 = (unsigned long long)blockIdx.x * QD_BLOCK + threadIdx.x;
    unsigned long long acc = 0ull;
    if (esz == 8) {
        const unsigned long long* __restrict__ w = (const unsigned long long*)E.p;
        const unsigned long long head = (n > 0 && ((unsigned long long)(uintptr_t)E.p & 15ull)) ? 1ull : 0ull;
        const unsigned long long npairs = (n - head) >> 1;
        const ulonglong2* __restrict__ w2 = (const ulonglong2*)(w + head);
        for (unsigned long long p = t0; p < npairs; p += stride) {
            const ulonglong2 v = w2[p];
            const unsigned long long i = head + 2ull * p;
            acc += qd_digest_term(v.x, i) + qd_digest_term(v.y, i + 1ull);
        }
        if (t0 == 0) {
            if (head) acc += qd_digest_term(w[0], 0ull);
            if (head + 2ull * npairs < n) acc += qd_digest_term(w[n - 1ull], n - 1ull);
        }
    } else if (esz == 4) {
        const unsigned int* __restrict__ w = (const unsigned int*)E.p;
        for (unsigned long long i = t0; i < n; i += stride) acc += qd_digest_term((unsigned long long)w[i], i);
    } else {
        const unsigned char* __restrict__ w = (const unsigned char*)E.p;
        for (unsigned long long i = t0; i < n; i += stride) acc += qd_digest_term((unsigned long long)w[i], i);
    }
    acc = qd_block_sum_u64(acc);
    if (threadIdx.x == 0) atomicAdd(out + blockIdx.y, acc);
}

// ------------------------------------------------------------------ refs -> planes
static const char* dg_ref_name(int ref, char* buf, size_t nb) {
    if (ref >= QD_SR_PHYTO_TRACER && ref < QD_SR_PHYTO_TRACER + QD_MAX_SPECIES) snprintf(buf, nb, "PHYTO_TRACER + %d", ref - QD_SR_PHYTO_TRACER);
    else if (ref >= QD_SR_HISTORY_SUM && ref < QD_SR_HISTORY_SUM + QD_HISTORY_MAX_ENTRIES) snprintf(buf, nb, "HISTORY_SUM + %d", ref - QD_SR_HISTORY_SUM);
    else snprintf(buf, nb, "%s", ref == QD_SR_ROUTE_BUFFER ? "ROUTE_BUFFER" : ref == QD_SR_ROUTE_FLOW ? "ROUTE_FLOW" : ref == QD_SR_ROUTE_LAKES ? "ROUTE_LAKES" :
                                 ref == QD_SR_ECO_LAI_STACK ? "ECO_LAI_STACK" : ref == QD_SR_INDIV_E_DAY ? "INDIV_E_DAY" :
                                 ref == QD_SR_INDIV_STRESS ? "INDIV_STRESS" : ref == QD_STATE_REF_SPECTRA_SUMS ? "SPECTRA_SUMS" :
                                 ref == QD_STATE_REF_FLOW_SUMS ? "FLOW_SUMS" : ref == QD_STATE_REF_SPHARM_SUMS ? "SPHARM_SUMS" :
                                 ref == QD_STATE_REF_EDDY_SUMS ? "EDDY_SUMS" : ref == QD_STATE_REF_EDDY_ANCHORS ? "EDDY_ANCHORS" :
                                 ref == QD_STATE_REF_EXTREMES_VALUES ? "EXTREMES_VALUES" : ref == QD_STATE_REF_EXTREMES_COUNTS ? "EXTREMES_COUNTS" :
                                 ref == QD_STATE_REF_EXTREMES_HIST ? "EXTREMES_HIST" : "?");
    return buf;
}

// -> 0 and the plane of `ref`, or the error set
static int dg_resolve(qd_ctx* c, int ref, QdDigestEntry* e) {
    const size_t cells = c->geo.cells();
    const void* p = nullptr; size_t n = cells; unsigned int esz = 8;
    const char* why = nullptr;
    char name[48];
    if (ref == QD_F_LAND_MASK || ref == QD_F_ICE_MASK) { p = ref == QD_F_LAND_MASK ? c->land : c->icemask; esz = 1; }
    else if (ref >= 0 && ref < QD_F_COUNT_F64) { p = c->f[ref]; esz = qd_eco_is_f32(c, ref) ? 4 : 8; }
    else if (ref >= QD_SR_PHYTO_TRACER && ref < QD_SR_PHYTO_TRACER + QD_MAX_SPECIES) {
        const int s = ref - QD_SR_PHYTO_TRACER;
        if (c->phyto.S == 0) why = "the phytoplankton tracers are not configured (qd_phyto_configure)";
        else if (s >= c->phyto.S) why = "the species index is not below the tracer count";
        else p = c->phyto.cur[s];
    } else if (ref == QD_SR_ROUTE_BUFFER || ref == QD_SR_ROUTE_FLOW || ref == QD_SR_ROUTE_LAKES) {
        const double *buf, *flow, *lakes; int n_lakes;
        if (!qd_route_planes(c, &buf, &flow, &lakes, &n_lakes)) why = "river routing is not configured (qd_route_configure)";
        else if (ref == QD_SR_ROUTE_LAKES) { p = lakes; n = (size_t)n_lakes; if (n_lakes <= 0) why = "the routing network has no lakes"; }
        else p = ref == QD_SR_ROUTE_BUFFER ? buf : flow;
    } else if (ref == QD_SR_ECO_LAI_STACK) {
        const double* L; int S, K;
        if (!qd_eco_daily_stack(c, &L, &S, &K)) why = "the daily vegetation step is not configured (qd_eco_daily_configure)";
        else { p = L; n = (size_t)S * K * cells; }
    } else if (ref == QD_SR_INDIV_E_DAY || ref == QD_SR_INDIV_STRESS) {
        if (c->eco.n_indiv <= 0) why = "the individuals are not configured (qd_indiv_configure)";
        else { p = ref == QD_SR_INDIV_E_DAY ? c->eco.E_day : c->eco.stress; n = (size_t)c->eco.n_indiv; }
    } else if (ref >= QD_SR_HISTORY_SUM && ref < QD_SR_HISTORY_SUM + QD_HISTORY_MAX_ENTRIES) {
        const double* sums; size_t stride; int ne;
        const int k = ref - QD_SR_HISTORY_SUM;
        if (!qd_history_planes(c, &sums, &stride, &ne)) why = "the history accumulators are not configured (qd_history_configure)";
        else if (k >= ne) why = "the entry index is not below the entry count";
        else p = sums + (size_t)k * stride;
    } else if (ref == QD_STATE_REF_SPECTRA_SUMS) {
        const double* sums;
        if (!qd_spectra_planes(c, &sums, &n)) { why = "the lat-resolved spectra sums are not configured (qd_spectra_configure)"; n = cells; }
        else p = sums;
    } else if (ref == QD_STATE_REF_FLOW_SUMS) {
        const double* sums;
        if (!qd_flow_planes(c, &sums, &n)) { why = "the flow lane is not configured (qd_flow_configure)"; n = cells; }
        else p = sums;
    } else if (ref == QD_STATE_REF_SPHARM_SUMS) {
        const double* sums;
        if (!qd_spharm_planes(c, &sums, &n)) { why = "the 2D sums of the spherical-harmonic lane are not configured (qd_spharm_configure)"; n = cells; }
        else p = sums;
    } else if (ref == QD_STATE_REF_EDDY_SUMS || ref == QD_STATE_REF_EDDY_ANCHORS) {
        const double *anchors, *sums; size_t na, ns;
        if (!qd_eddy_planes(c, &anchors, &na, &sums, &ns)) { why = "the eddy statistics are not configured (qd_eddy_configure)"; n = cells; }
        else if (ref == QD_STATE_REF_EDDY_SUMS) { p = sums; n = ns; }
        else { p = anchors; n = na; }
    } else if (ref == QD_STATE_REF_EXTREMES_VALUES || ref == QD_STATE_REF_EXTREMES_COUNTS || ref == QD_STATE_REF_EXTREMES_HIST) {
        const int which = ref - QD_STATE_REF_EXTREMES_VALUES;
        if (!qd_extremes_planes(c, which, &p, &n)) { why = "the extremes lane is not configured (qd_extremes_configure)"; n = cells; }
        else if (!p) why = "the extremes lane has no histogram";
        else esz = which == 1 ? 4 : 8;
    } else {
        return qd_fail(c, ("qd_state_digest: unknown ref " + std::to_string(ref)).c_str());
    }
    if (why) return qd_fail(c, (std::string("qd_state_digest: ref ") + dg_ref_name(ref, name, sizeof name) + ": " + why).c_str());
    if (!p) return qd_fail(c, ("qd_state_digest: ref " + std::to_string(ref) + " has no plane on this handle").c_str());
    e->p = p; e->n_esz = ((unsigned long long)n << 4) | (unsigned long long)esz;
    return 0;
}

extern "C" int qd_state_digest(qd_handle c, int n, const int32_t* refs, uint64_t* out) {
    if (!c || n < 0 || (n && (!refs || !out))) return -1;
    if (!qd_whole_globe(c))
        return qd_fail(c, "qd_state_digest: the state digest needs a whole-globe handle (world == 1, n_rows == n_lat); latitude bands are not supported");
    if (n > QD_DIGEST_MAX) return qd_fail(c, "qd_state_digest: at most 64 refs per call");
    if (n == 0) return 0;
    QdDigestTab T;
    unsigned long long most = 0;
    for (int k = 0; k < n; ++k) {
        if (int rc = dg_resolve(c, refs[k], &T.e[k])) return rc;
        const unsigned long long ne = T.e[k].n_esz >> 4;
        most = std::max(most, (T.e[k].n_esz & 15ull) == 8 ? (ne + 1) / 2 : ne);        // work items of the longest entry
    }
    for (int k = n; k < QD_DIGEST_MAX; ++k) T.e[k] = QdDigestEntry{nullptr, 0ull};
    hipSetDevice(c->desc.device);
    if (!c->digest_out) QD_HIP(c, hipMalloc(&c->digest_out, (size_t)QD_DIGEST_MAX * sizeof(unsigned long long)));   // first use; qd_destroy frees it
    unsigned long long* dout = c->digest_out;
    int rc = 0;
    {
        QdScope sc(c, "state_digest", true);                  // one launch: timed from the dispatch itself
        const unsigned long long want = std::max<unsigned long long>(1ull, (most + QD_BLOCK - 1) / QD_BLOCK);
        const unsigned long long per_entry = std::max<unsigned long long>(1ull, ((unsigned long long)std::max(1, c->n_cu) * 8ull + n - 1) / n);
        const int gx = (int)std::min(want, per_entry);
        hipError_t e = hipMemsetAsync(dout, 0, (size_t)QD_DIGEST_MAX * sizeof(unsigned long long), c->stream);
        if (e == hipSuccess) {
            QD_LAUNCH_TIMED(sc, k_state_digest, dim3(gx, n), dim3(QD_BLOCK), c->stream, T, dout);
            e = hipMemcpyAsync(out, dout, (size_t)n * sizeof(unsigned long long), hipMemcpyDeviceToHost, c->stream);
        }
        if (e == hipSuccess) e = hipStreamSynchronize(c->stream);
        if (e == hipSuccess) e = hipGetLastError();
        if (e != hipSuccess) rc = qd_fail(c, "qd_state_digest: launch", e);
    }
    return rc;
}

// ------------------------------------------------------------------ the host-side scalars of an exact resume
// What a step reads from the context besides the planes and the two step counters (qd_internal.h: qd_ctx, QdEco), as doubles (the
// counts stay far below 2^53).  The QD_STATE_SCALARS_N = 32 slots are enum qd_state_scalar of the public header, which the code
// below uses by name; what they hold:
//   0 cloud_eff_valid   1 has_elevation (read only: the elevation map is the run's own)   2 eco.hours   3 eco.next_h   4 eco.count
//   5 have_lai   6 f_valid   7 alpha_valid   8 alpha_dirty   9 banded_valid   10 water_valid   11 lai_version   12 snap_version
//   13 n_recompute   14 the individuals' sub-step period (-1: not begun)   15 its accumulator   16 its firings
//   17 daily phytoplankton steps   18 daily vegetation firings   19 firings of the individuals' daily step   20 last_nsub
//   21 .. 30 the energy-budget means of the last span that took them   31 reserved (0)
static_assert(QD_STATE_REF_TRACERS == QD_MAX_SPECIES, "the public index range of QD_SR_PHYTO_TRACER is the species cap");
static_assert(QD_SS_LAST_DIAG + 10 < QD_STATE_SCALARS_N, "the ten energy-budget means and the reserved slot end the table");
extern "C" int qd_state_scalars_get(qd_handle c, double* out, int n) {
    if (!c || !out) return -1;
    if (n != QD_STATE_SCALARS_N) return qd_fail(c, "qd_state_scalars_get: n is not QD_STATE_SCALARS_N (ABI drift)");
    const QdEco& E = c->eco;
    std::fill(out, out + QD_STATE_SCALARS_N, 0.0);
    out[QD_SS_CLOUD_EFF_VALID] = (double)c->cloud_eff_valid; out[QD_SS_HAS_ELEVATION] = (double)c->has_elevation;
    out[QD_SS_ECO_HOURS] = E.hours; out[QD_SS_ECO_NEXT_H] = E.next_h; out[QD_SS_ECO_COUNT] = (double)E.count;
    out[QD_SS_HAVE_LAI] = (double)E.have_lai; out[QD_SS_F_VALID] = (double)E.f_valid; out[QD_SS_ALPHA_VALID] = (double)E.alpha_valid;
    out[QD_SS_ALPHA_DIRTY] = (double)E.alpha_dirty; out[QD_SS_BANDED_VALID] = (double)E.banded_valid;
    out[QD_SS_WATER_VALID] = (double)E.water_valid;
    out[QD_SS_LAI_VERSION] = (double)E.lai_version; out[QD_SS_SNAP_VERSION] = (double)E.snap_version;
    out[QD_SS_N_RECOMPUTE] = (double)E.n_recompute;
    out[QD_SS_INDIV_PERIOD] = E.period; out[QD_SS_INDIV_ACCUM] = E.accum; out[QD_SS_INDIV_FIRED] = (double)E.n_fired;
    out[QD_SS_PHYTO_DAILY_STEPS] = (double)qd_phyto_daily_steps(c, -1); out[QD_SS_ECO_DAILY_FIRED] = (double)qd_eco_daily_fired(c, -1);
    out[QD_SS_INDIV_DAILY_FIRED] = (double)qd_indiv_daily_fired(c, -1); out[QD_SS_LAST_NSUB] = (double)c->last_nsub;
    std::copy(c->last_diag, c->last_diag + 10, out + QD_SS_LAST_DIAG);
    return 0;
}

extern "C" int qd_state_scalars_set(qd_handle c, const double* in, int n) {
    if (!c || !in) return -1;
    if (n != QD_STATE_SCALARS_N) return qd_fail(c, "qd_state_scalars_set: n is not QD_STATE_SCALARS_N (ABI drift)");
    if (!qd_whole_globe(c)) return qd_fail(c, "qd_state_scalars_set: an exact resume needs a whole-globe handle; latitude bands are not supported");
    QdEco& E = c->eco;
    c->cloud_eff_valid = in[QD_SS_CLOUD_EFF_VALID] != 0.0;      // QD_SS_HAS_ELEVATION is read only
    E.hours = in[QD_SS_ECO_HOURS]; E.next_h = in[QD_SS_ECO_NEXT_H]; E.count = (int64_t)in[QD_SS_ECO_COUNT];
    E.have_lai = in[QD_SS_HAVE_LAI] != 0.0; E.f_valid = in[QD_SS_F_VALID] != 0.0; E.alpha_valid = in[QD_SS_ALPHA_VALID] != 0.0;
    E.alpha_dirty = in[QD_SS_ALPHA_DIRTY] != 0.0; E.banded_valid = in[QD_SS_BANDED_VALID] != 0.0;
    E.water_valid = in[QD_SS_WATER_VALID] != 0.0;
    E.lai_version = (int)in[QD_SS_LAI_VERSION]; E.snap_version = (int)in[QD_SS_SNAP_VERSION];
    E.n_recompute = (int)in[QD_SS_N_RECOMPUTE];
    E.period = in[QD_SS_INDIV_PERIOD]; E.accum = in[QD_SS_INDIV_ACCUM]; E.n_fired = (int64_t)in[QD_SS_INDIV_FIRED];
    qd_phyto_daily_steps(c, (int64_t)in[QD_SS_PHYTO_DAILY_STEPS]); qd_eco_daily_fired(c, (int64_t)in[QD_SS_ECO_DAILY_FIRED]);
    qd_indiv_daily_fired(c, (int64_t)in[QD_SS_INDIV_DAILY_FIRED]);
    c->last_nsub = (int)in[QD_SS_LAST_NSUB];
    std::copy(in + QD_SS_LAST_DIAG, in + QD_SS_LAST_DIAG + 10, c->last_diag);
    return 0;
}
