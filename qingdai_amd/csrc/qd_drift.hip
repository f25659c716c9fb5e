// qd_drift.hip -- Lagrangian drifters: particles that follow the resident winds and currents, advanced on EVERY step of a qd_step_n
// span and recorded on the scheduled ones, as a span lane, gfx950 (QD_DRIFTERS).
//
// THE STEP IS THE CONTRACT.  It is stated here and restated in NumPy by qingdai_amd/drifters.py: advance_reference, bit for bit, and
// nowhere else.  Two populations share it: `atm` follows (U, V), `ocn` follows (UO, VO).  A particle is (r, c, status) and, for
// ocn, a blocked count: r the row coordinate in [0, n_lat - 1], c the column coordinate in [0, P), P = n_lon - 1 (the grid's last
// column repeats the first meridian: the period of oracle/qd_oracle/numerics.py: wrap_coord).  All of it is f64, a structure of arrays.
// One step of length dt reads the two velocity planes as the model's step leaves them (what qd_download returns after a span that
// ends with that step):
//   sample(f, r, c)  r0 = floor(r), c0 = floor(c), tr = r - r0, tc = c - c0, r1 = min(r0 + 1, n_lat - 1), c1 = c0 + 1 (<= n_lon - 1,
//                    since c < P), wr0 = 1 - tr, wr1 = tr, wc0 = 1 - tc, wc1 = tc, and in the corner order of numerics.bilinear_wrap
//                        t = 0; t = t + f[r0][c0] * wr0 * wc0; t = t + f[r0][c1] * wr0 * wc1; t = t + f[r1][c0] * wr1 * wc0;
//                        t = t + f[r1][c1] * wr1 * wc1                      (every product left to right, every operation rounded)
//   sec(r)           S[r0] * wr0 + S[r1] * wr1 with the row table S_j = 1 / max(cos lat_j, sin(dlat / 2)) the HOST computed
//                    (drifters.sec_table) and qd_drift_configure uploaded.  No sin, cos or other transcendental runs on the
//                    device for this lane: + - * /, floor and comparisons only, under -ffp-contract=off.
//   stage 0          (u0, v0) = sample at (r, c);  dr0 = v0 * dt / (a * dlat);  dc0 = u0 * dt * sec(r) / (a * dlon)
//                    (rm, cm) = fold(r + dr0 / 2, c + dc0 / 2)
//   stage 1          (u1, v1) = sample at (rm, cm), the SAME planes;  dr1 = v1 * dt / (a * dlat);  dc1 = u1 * dt * sec(rm) / (a * dlon)
//                    (r', c') = fold(r + dr1, c + dc1)
//   fold(r, c)       r < 0: r = -r, c = c + P / 2;  r > n_lat - 1: r = 2 (n_lat - 1) - r, c = c + P / 2 -- once; an r still outside
//                    [0, n_lat - 1] fails.  Then c = c - P * floor(c / P), any number of wraps; a result == P becomes 0 (and so does
//                    one the rounding of c / P left below 0 or above P, which can only happen within a rounding error of the seam
//                    or where ulp(c) > P: the column stays inside [0, P) whatever comes in).
//   dead             a non-finite u, v, dr, dc or folded coordinate at either stage, or a fold that fails, sets status = 1: the
//                    particle keeps the position it had and is never touched again.  A NaN in a corner of weight 0 kills too:
//                    0 * NaN is NaN -- that is the arithmetic, and deliberate.
//   blocked (ocn)    the cell nearest to (r', c') is (floor(r' + 0.5), floor(c' + 0.5)), column n_lon - 1 taken as column 0; where
//                    the handle's land mask holds land there the move is rejected: the position stays, blocked = blocked + 1.
// On a recording step every particle, dead or alive, also takes sample(f, r, c) at the position it then has of up to
// QD_DRIFT_MAX_SAMPLES planes per population, and ONE record goes to the lane's log:
//     [atm: r | c | status | sample 0 | ...][ocn: r | c | status | blocked | sample 0 | ...]       each block [n] doubles, contiguous
//
// ONE launch per advanced step, with or without a record (timing scope "drifters"), none while the lane is off.  One thread per
// particle, QD_BLOCK threads per workgroup; the first ceil(n_atm / QD_BLOCK) workgroups are atm's, the others ocn's.  No LDS, no
// atomics, no cross-lane traffic.  The kernel is a latency chain of two gathers (8 corners + 2 table rows each), not a bandwidth
// load: the eight corner loads of a stage are independent and are issued before the first of them is used, and nothing limits the
// occupancy (no LDS; the register count is far below the 128 that would halve it).
#include "qd_span.h"
#include "qd_entry.h"
#include <cmath>
#include <vector>

static_assert(QD_DRIFT_MAX_SAMPLES == 4, "the sample table of a population");

struct QdDriftPop {
    double* st;                                   // [3 (atm) or 4 (ocn)][n]: r | c | status [| blocked]
    const double* pu; const double* pv;           // the two velocity planes
    const double* samp[QD_DRIFT_MAX_SAMPLES];     // the sampled planes of a recording step
    double* rec;                                  // this population's block of the open record; nullptr: the step does not record
    int n, ns, ocean, blocks;                     // particles, sampled planes, 1: the land test and the blocked count, workgroups
};
struct QdDriftArgs {
    QdDriftPop pop[2];
    const double* sec;                            // [n_lat] the row table S
    const uint8_t* land;                          // [n_lat][n_lon]
    int nlat, nlon;
    double dt, adlat, adlon;                      // a * dlat, a * dlon
};

struct QdDriftCell { size_t i00, i01, i10, i11; int r0, r1; double wr0, wr1, wc0, wc1; };

__device__ __forceinline__ bool dr_fin(double x) { return fabs(x) <= DBL_MAX; }          // false for NaN and +-inf

// (r, c) inside [0, n_lat - 1] x [0, P): the clamps change nothing there and keep every index inside the plane whatever comes in
__device__ __forceinline__ QdDriftCell dr_cell(double r, double c, int nlat, int nlon) {
    QdDriftCell K;
    const double r0f = floor(r), c0f = floor(c);
    const double tr = r - r0f, tc = c - c0f;
    int r0 = (int)r0f, c0 = (int)c0f;
    r0 = min(max(r0, 0), nlat - 1); c0 = min(max(c0, 0), nlon - 2);
    const int r1 = min(r0 + 1, nlat - 1), c1 = c0 + 1;
    K.r0 = r0; K.r1 = r1;
    K.i00 = (size_t)r0 * nlon + c0; K.i01 = (size_t)r0 * nlon + c1; K.i10 = (size_t)r1 * nlon + c0; K.i11 = (size_t)r1 * nlon + c1;
    K.wr0 = 1.0 - tr; K.wr1 = tr; K.wc0 = 1.0 - tc; K.wc1 = tc;
    return K;
}
__device__ __forceinline__ double dr_mix(double f00, double f01, double f10, double f11, const QdDriftCell& K) {
    double t = 0.0;
    t = t + f00 * K.wr0 * K.wc0;
    t = t + f01 * K.wr0 * K.wc1;
    t = t + f10 * K.wr1 * K.wc0;
    t = t + f11 * K.wr1 * K.wc1;
    return t;
}
// one stage's velocities and metric: ten independent loads, all issued before the first use
__device__ __forceinline__ void dr_stage(const double* __restrict__ pu, const double* __restrict__ pv, const double* __restrict__ S,
                                         const QdDriftCell& K, double& u, double& v, double& sec) {
    const double u00 = pu[K.i00], u01 = pu[K.i01], u10 = pu[K.i10], u11 = pu[K.i11];
    const double v00 = pv[K.i00], v01 = pv[K.i01], v10 = pv[K.i10], v11 = pv[K.i11];
    const double s0 = S[K.r0], s1 = S[K.r1];
    u = dr_mix(u00, u01, u10, u11, K);
    v = dr_mix(v00, v01, v10, v11, K);
    sec = s0 * K.wr0 + s1 * K.wr1;
}
__device__ __forceinline__ bool dr_fold(double& r, double& c, double rmax, double P) {
    if (!dr_fin(r) || !dr_fin(c)) return false;
    if (r < 0.0) { r = -r; c = c + P / 2.0; }
    else if (r > rmax) { r = 2.0 * rmax - r; c = c + P / 2.0; }
    if (!(r >= 0.0 && r <= rmax) || !dr_fin(c)) return false;
    c = c - P * floor(c / P);
    if (!(c >= 0.0 && c < P)) c = 0.0;
    return true;
}

__global__ void __launch_bounds__(QD_BLOCK) k_drift(QdDriftArgs A) {
    const int q = (int)blockIdx.x < A.pop[0].blocks ? 0 : 1;                    // workgroup-uniform
    const QdDriftPop& Q = A.pop[q];
    const int i = ((int)blockIdx.x - (q ? A.pop[0].blocks : 0)) * QD_BLOCK + (int)threadIdx.x;
    if (i >= Q.n) return;
    const size_t n = (size_t)Q.n;
    const int nlat = A.nlat, nlon = A.nlon;
    const double rmax = (double)(nlat - 1), P = (double)(nlon - 1);
    double r = Q.st[i], c = Q.st[n + i], dead = Q.st[2 * n + i];
    double blocked = Q.ocean ? Q.st[3 * n + i] : 0.0;
    if (dead == 0.0) {
        double u, v, sec, rn = r, cn = c;
        const QdDriftCell K0 = dr_cell(r, c, nlat, nlon);
        dr_stage(Q.pu, Q.pv, A.sec, K0, u, v, sec);
        const double dr0 = v * A.dt / A.adlat, dc0 = u * A.dt * sec / A.adlon;
        bool ok = dr_fin(u) && dr_fin(v) && dr_fin(dr0) && dr_fin(dc0);
        double rm = r + dr0 / 2.0, cm = c + dc0 / 2.0;
        ok = ok && dr_fold(rm, cm, rmax, P);
        if (ok) {
            const QdDriftCell K1 = dr_cell(rm, cm, nlat, nlon);
            dr_stage(Q.pu, Q.pv, A.sec, K1, u, v, sec);
            const double dr1 = v * A.dt / A.adlat, dc1 = u * A.dt * sec / A.adlon;
            ok = dr_fin(u) && dr_fin(v) && dr_fin(dr1) && dr_fin(dc1);
            rn = r + dr1; cn = c + dc1;
            ok = ok && dr_fold(rn, cn, rmax, P);
        }
        if (!ok) {
            dead = 1.0;
            Q.st[2 * n + i] = dead;
        } else {
            bool move = true;
            if (Q.ocean) {
                int jr = (int)floor(rn + 0.5), jc = (int)floor(cn + 0.5);
                jr = min(max(jr, 0), nlat - 1); jc = min(max(jc, 0), nlon - 1);
                if (jc == nlon - 1) jc = 0;
                move = A.land[(size_t)jr * nlon + jc] == 0;
                if (!move) { blocked = blocked + 1.0; Q.st[3 * n + i] = blocked; }
            }
            if (move) { r = rn; c = cn; Q.st[i] = r; Q.st[n + i] = c; }
        }
    }
    if (Q.rec) {
        double* R = Q.rec;
        R[i] = r; R[n + i] = c; R[2 * n + i] = dead;
        int b = 3;
        if (Q.ocean) { R[3 * n + i] = blocked; b = 4; }
        const QdDriftCell K = dr_cell(r, c, nlat, nlon);
        double f[QD_DRIFT_MAX_SAMPLES][4];
#pragma unroll
        for (int k = 0; k < QD_DRIFT_MAX_SAMPLES; ++k)
            if (k < Q.ns) { const double* p = Q.samp[k]; f[k][0] = p[K.i00]; f[k][1] = p[K.i01]; f[k][2] = p[K.i10]; f[k][3] = p[K.i11]; }
#pragma unroll
        for (int k = 0; k < QD_DRIFT_MAX_SAMPLES; ++k)
            if (k < Q.ns) R[(size_t)(b + k) * n + i] = dr_mix(f[k][0], f[k][1], f[k][2], f[k][3], K);
    }
}

// ------------------------------------------------------------------ host side
struct QdDrift {
    int n[2] = {0, 0}, ns[2] = {0, 0};
    int planes[2][QD_DRIFT_MAX_SAMPLES];
    double* st[2] = {nullptr, nullptr};           // [3][n_atm], [4][n_ocn]
    double* sec = nullptr;                        // [n_lat]
    bool lazy = false;                            // a sampled plane is one of the lazily stored diagnostics
    QdSpanLane lane;
    static int rows(int q) { return q ? 4 : 3; }
    size_t block(int q) const { return (size_t)n[q] * (rows(q) + ns[q]); }       // doubles of a population's part of a record
    bool stale(const qd_ctx* c) const {
        for (int q = 0; q < 2; ++q) for (int k = 0; k < ns[q]; ++k) if (!hist_plane(c, planes[q][k])) return true;
        return false;
    }
};
static const char* const DRIFT_MISSING = "not configured (qd_drift_configure first)";
static const char* const DRIFT_STALE = "a sampled field is no longer an f64 plane (qd_drift_configure again)";

static QdSpanLane* drift_lane(qd_ctx* c) { return c && c->drift ? &c->drift->lane : nullptr; }

void qd_drift_release(qd_ctx* c) {
    QdDrift* d = c->drift;
    if (!d) return;
    if (c->stream) hipStreamSynchronize(c->stream);
    void* p[] = {d->st[0], d->st[1], d->sec, d->lane.log};
    for (void* q : p) if (q) hipFree(q);
    delete d;
    c->drift = nullptr;
}

// a population's state as the host hands it over: every coordinate finite and inside its interval, status 0 or 1, blocked >= 0
static const char* drift_state_check(const qd_ctx* c, int n, const double* r, const double* col, const double* status, const double* blocked) {
    const double rmax = (double)(c->geo.nlat - 1), P = (double)(c->geo.nlon - 1);
    for (int i = 0; i < n; ++i) {
        if (!(r[i] >= 0.0 && r[i] <= rmax)) return "a row coordinate is non-finite or outside [0, n_lat - 1]";
        if (!(col[i] >= 0.0 && col[i] < P)) return "a column coordinate is non-finite or outside [0, n_lon - 1)";
        if (status && status[i] != 0.0 && status[i] != 1.0) return "a status is neither 0 nor 1";
        if (blocked && !(blocked[i] >= 0.0 && blocked[i] <= DBL_MAX)) return "a blocked count is negative or non-finite";
    }
    return nullptr;
}

extern "C" int qd_drift_configure(qd_handle c, int n_atm, const double* r_atm, const double* c_atm, int n_ocn, const double* r_ocn,
                                  const double* c_ocn, int ns_atm, const int32_t* planes_atm, int ns_ocn, const int32_t* planes_ocn,
                                  const double* sec_row, int* log_cap) {
    if (!c) return -1;
    const std::string w = "qd_drift_configure: ";
    if (!qd_whole_globe(c))
        return qd_fail(c, (w + "the drifters need a whole-globe handle (world == 1, n_rows == n_lat); latitude bands are not supported").c_str());
    if (n_atm < 0 || n_ocn < 0 || n_atm > QD_DRIFT_MAX || n_ocn > QD_DRIFT_MAX)
        return qd_fail(c, (w + "a population holds 0 to QD_DRIFT_MAX (1048576) particles").c_str());
    const int nn[2] = {n_atm, n_ocn}, nsv[2] = {n_atm ? ns_atm : 0, n_ocn ? ns_ocn : 0};
    const double* rr[2] = {r_atm, r_ocn};
    const double* cc[2] = {c_atm, c_ocn};
    const int32_t* pl[2] = {planes_atm, planes_ocn};
    QdDrift t;
    for (int q = 0; q < 2; ++q) {
        if (nn[q] && (!rr[q] || !cc[q] || !sec_row)) return -1;
        if (nsv[q] < 0 || nsv[q] > QD_DRIFT_MAX_SAMPLES) return qd_fail(c, (w + "at most 4 sampled planes per population").c_str());
        if (nsv[q] && !pl[q]) return -1;
        for (int k = 0; k < nsv[q]; ++k) {
            if (pl[q][k] == QD_F_PRECIP)
                return qd_fail(c, (w + "PRECIP cannot be sampled: the lane reads behind a step's last launch, and inside a span the hoisted "
                                       "precipitation block has by then overwritten it with the next step's").c_str());
            if (!hist_plane(c, pl[q][k])) return qd_fail(c, (w + "a sampled field is not an f64 plane").c_str());
            t.planes[q][k] = pl[q][k];
            t.lazy = t.lazy || hist_lazy_field(pl[q][k]);
        }
        if (const char* why = drift_state_check(c, nn[q], rr[q], cc[q], nullptr, nullptr)) return qd_fail(c, (w + "initial position: " + why).c_str());
        t.n[q] = nn[q]; t.ns[q] = nsv[q];
    }
    hipSetDevice(c->desc.device);
    qd_drift_release(c);
    if (log_cap) *log_cap = 0;
    if (n_atm == 0 && n_ocn == 0) return 0;
    QdDrift* d = new QdDrift(t);
    const int nlat = c->geo.nlat;
    const size_t width = d->block(0) + d->block(1), recb = width * sizeof(double);
    d->lane.width = (int)width;                   // <= 2 * 2^20 * 8
    d->lane.cap = (int)std::max<size_t>(1, std::min<size_t>(QD_DRIFT_LOG_CAP_MAX, ((size_t)QD_DRIFT_LOG_MIB << 20) / recb));
    bool ok = hipMalloc(&d->sec, (size_t)nlat * sizeof(double)) == hipSuccess &&
              hipMalloc(&d->lane.log, d->lane.log_doubles() * sizeof(double)) == hipSuccess &&
              hipMemcpyAsync(d->sec, sec_row, (size_t)nlat * sizeof(double), hipMemcpyHostToDevice, c->stream) == hipSuccess &&
              hipMemsetAsync(d->lane.log, 0, d->lane.log_doubles() * sizeof(double), c->stream) == hipSuccess;
    for (int q = 0; q < 2 && ok; ++q) {
        if (!nn[q]) continue;
        const size_t nb = (size_t)nn[q] * sizeof(double);
        ok = hipMalloc(&d->st[q], QdDrift::rows(q) * nb) == hipSuccess &&
             hipMemsetAsync(d->st[q], 0, QdDrift::rows(q) * nb, c->stream) == hipSuccess &&         // status 0, blocked 0
             hipMemcpyAsync(d->st[q], rr[q], nb, hipMemcpyHostToDevice, c->stream) == hipSuccess &&
             hipMemcpyAsync(d->st[q] + nn[q], cc[q], nb, hipMemcpyHostToDevice, c->stream) == hipSuccess;
    }
    ok = ok && hipStreamSynchronize(c->stream) == hipSuccess;          // the host arrays are the caller's again
    c->drift = d;
    if (!ok) { qd_drift_release(c); return qd_fail(c, (w + "device allocation or upload failed").c_str()); }
    if (log_cap) *log_cap = d->lane.cap;
    return 0;
}

extern "C" int qd_drift_schedule(qd_handle c, int steps, const int32_t* record) {
    return qd_lane_schedule(c, drift_lane(c), steps, record, "qd_drift_schedule", DRIFT_MISSING);
}
extern "C" int qd_drift_log(qd_handle c, double* out, int max, int* n) {
    return qd_lane_drain(c, drift_lane(c), out, max, n, "qd_drift_log", DRIFT_MISSING);
}
extern "C" int qd_drift_reset(qd_handle c) {
    if (!c) return -1;
    if (!c->drift) return qd_fail(c, (std::string("qd_drift_reset: ") + DRIFT_MISSING).c_str());
    c->drift->lane.reset();
    return 0;
}

extern "C" int qd_drift_state_get(qd_handle c, double* atm, double* ocn) {
    if (!c) return -1;
    QdDrift* d = c->drift;
    if (!d) return qd_fail(c, (std::string("qd_drift_state_get: ") + DRIFT_MISSING).c_str());
    double* out[2] = {atm, ocn};
    hipSetDevice(c->desc.device);
    for (int q = 0; q < 2; ++q) {
        if (!d->n[q]) continue;
        if (!out[q]) return -1;
        QD_HIP(c, hipMemcpyAsync(out[q], d->st[q], (size_t)QdDrift::rows(q) * d->n[q] * sizeof(double), hipMemcpyDeviceToHost, c->stream));
    }
    QD_HIP(c, hipStreamSynchronize(c->stream));
    return 0;
}
extern "C" int qd_drift_state_set(qd_handle c, const double* atm, const double* ocn) {
    if (!c) return -1;
    QdDrift* d = c->drift;
    if (!d) return qd_fail(c, (std::string("qd_drift_state_set: ") + DRIFT_MISSING).c_str());
    const double* in[2] = {atm, ocn};
    for (int q = 0; q < 2; ++q) {
        if (!d->n[q]) continue;
        if (!in[q]) return -1;
        const size_t n = (size_t)d->n[q];
        if (const char* why = drift_state_check(c, d->n[q], in[q], in[q] + n, in[q] + 2 * n, q ? in[q] + 3 * n : nullptr))
            return qd_fail(c, (std::string("qd_drift_state_set: ") + why).c_str());
    }
    hipSetDevice(c->desc.device);
    for (int q = 0; q < 2; ++q)
        if (d->n[q])
            QD_HIP(c, hipMemcpyAsync(d->st[q], in[q], (size_t)QdDrift::rows(q) * d->n[q] * sizeof(double), hipMemcpyHostToDevice, c->stream));
    QD_HIP(c, hipStreamSynchronize(c->stream));
    return 0;
}

bool qd_drift_scheduled(const qd_ctx* c) { return c->drift && !c->drift->lane.sched.empty(); }
bool qd_drift_reads_lazy(const qd_ctx* c) { return c->drift && c->drift->lazy; }

QdSpanLane* qd_drift_span_begin(qd_ctx* c, int n, int with_ocean) {
    static const QdSpanTexts T = {
        "qd_step_n: the drifters need a whole-globe handle; latitude bands are not supported",
        "qd_step_n: qd_drift_configure has not been called",
        "qd_step_n: a qd_drift_schedule must cover exactly the n steps of the span",
        "qd_step_n: the span's drifter records would overflow the lane's log (drain it with qd_drift_log first)"};
    const bool dry = c->drift && c->drift->n[1] > 0 && !with_ocean;
    const bool stale = c->drift && c->drift->stale(c);
    QdSpanLane* l = qd_lane_span_begin(c, drift_lane(c), n, T, dry ? "qd_step_n: the ocn drifters need the ocean step (bit0)" : nullptr,
                                       stale ? "qd_step_n: a sampled drifter field is no longer an f64 plane (qd_drift_configure again)" : nullptr);
    if (!l && c->drift) c->drift->lane.clear_schedule();          // refused: the span guard never sees this lane, and a schedule serves one span
    return l;
}

// one step of both populations on the planes as they stand; record: the step also fills the lane's next record
int qd_drift_step(qd_ctx* c, double dt, int record) {
    QdDrift* d = c->drift;
    double* rec = nullptr;
    if (record) {
        if (d->lane.full()) return qd_fail(c, "qd_step_n: drifter log full (drain it with qd_drift_log)");
        rec = d->lane.next();
    }
    QdDriftArgs A;
    const int fu[2] = {QD_F_U, QD_F_UO}, fv[2] = {QD_F_V, QD_F_VO};
    for (int q = 0; q < 2; ++q) {
        QdDriftPop& Q = A.pop[q];
        Q.st = d->st[q]; Q.pu = c->f[fu[q]]; Q.pv = c->f[fv[q]];
        for (int k = 0; k < QD_DRIFT_MAX_SAMPLES; ++k) Q.samp[k] = k < d->ns[q] ? c->f[d->planes[q][k]] : nullptr;
        Q.rec = rec ? rec + (q ? d->block(0) : 0) : nullptr;
        Q.n = d->n[q]; Q.ns = d->ns[q]; Q.ocean = q; Q.blocks = (d->n[q] + QD_BLOCK - 1) / QD_BLOCK;
    }
    A.sec = d->sec; A.land = c->land; A.nlat = c->geo.nlat; A.nlon = c->geo.nlon;
    A.dt = dt; A.adlat = c->p.a * c->dlat; A.adlon = c->p.a * c->dlon;
    QdScope sc(c, "drifters", true);                      // one launch: timed from the dispatch itself
    QD_LAUNCH_TIMED(sc, k_drift, dim3(A.pop[0].blocks + A.pop[1].blocks), dim3(QD_BLOCK), c->stream, A);
    return 0;
}

extern "C" int qd_drift_advance(qd_handle c, double dt, int record) {
    if (!c) return -1;
    if (!c->drift) return qd_fail(c, (std::string("qd_drift_advance: ") + DRIFT_MISSING).c_str());
    if (c->drift->stale(c)) return qd_fail(c, (std::string("qd_drift_advance: ") + DRIFT_STALE).c_str());
    if (record && c->drift->lane.full()) return qd_fail(c, "qd_drift_advance: drifter log full (drain it with qd_drift_log)");
    hipSetDevice(c->desc.device);
    if (int rc = qd_drift_step(c, dt, record)) return rc;
    return qd_launch_check(c, "qd_drift_advance");
}
