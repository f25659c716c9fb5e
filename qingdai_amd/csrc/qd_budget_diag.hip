// qd_budget_diag.hip -- the reference driver's periodic budget lines as a span lane, gfx950 (QD_BUDGET_DIAG).
//
// On a scheduled step of a qd_step_n span (qd_budget_diag_schedule: bit0 = the driver's i % 200 cadence, bit1 = the ocean's own
// [OceanE] cadence) qd_step_n runs up to five reductions at the reference's positions in the step; each is ONE multi-accumulator
// launch (one workgroup per row, every field read once) and one finishing workgroup that writes its sums into the step's record:
//   1 k_bd_energy        in front of time_step (run_simulation.py:2150-2185): the flux function of the coupling block
//                        (qd_surface_fluxes) on isr, the current albedo, cloud_for_rad, T_s, h, u, v and the previous step's LH
//                        -> sum w TOA_net, sum w SFC_net, sum w ATM_net (energy.py:515-525), and np.nanmean(T_s) as sum / count
//   2 k_bd_ocean_energy  inside the ocean step, behind the last sub-step and in front of the polar fill (ocean.py:446-516): eff_Q
//                        with the under-ice factor, (SST - SST at the previous firing) / dt, over the ocean and over the polar
//                        ocean; the kernel also takes the new snapshot
//   3 k_bd_ocean         behind the ocean step (ocean.py:535-545): sum w KE, max speed, eta min / max
//   4 k_bd_humidity      behind time_step (run_simulation.py:2276-2283): sum w of E, P_cond, LH, LH_release
//   5 k_bd_water         behind the snow commit, bucket and routing (run_simulation.py:2350-2394, hydrology.py:304-321): sum w of E,
//                        hybrid precip, R_flux_land_total, rho_a h_mbl q, rho_i h_ice, W_land, S_snow; np.nanmax of the routing
//                        flow map; the last routing event's ocean inflow and closure error are copied behind them
// The record holds SUMS and extrema; the host (qingdai_amd/budget_diag.py) divides by its own weight sums and formats, so that the
// last few scalar operations are the reference's own Python expressions.  Sums: wave shuffle, workgroup, then the rows in a fixed
// order (qd_blockred.h) -- no atomics, a record does not depend on scheduling or on how a run is cut into spans.
// Whole-globe handles only.  A step that does not fire launches nothing of this file.
#include "qd_span.h"
#include "qd_fluxes.h"
#include "qd_blockred.h"
#include <algorithm>

QdColP qd_make_colp_driver(const qd_ctx* c, double dt);   // qd_ocean.hip
const double* qd_route_last_record(const qd_ctx* c);      // qd_route.hip

#define QD_BD_NQ 8                 // accumulators per launch (at most)
// record slots (qingdai_amd/budget_diag.py: REC)
enum { BD_E_TOA = 0, BD_OE_Q = 5, BD_O_KE = 13, BD_H_E = 17, BD_W_E = 21, BD_W_FLOW = 28, BD_W_INFLOW = 29, BD_RAN = 32, BD_FIRE = 37 };

struct QdBdOps { QdRedOp op[QD_BD_NQ]; };
static QdBdOps bd_ops(std::initializer_list<QdRedOp> l) {
    QdBdOps o; int k = 0;
    for (int q = 0; q < QD_BD_NQ; ++q) o.op[q] = QD_RED_SUM;
    for (QdRedOp x : l) o.op[k++] = x;
    return o;
}

struct QdBudget {
    int lines = 0;                    // QD_BD_LINE_* the host enabled
    uint8_t* polar_row = nullptr;     // [nlat] the reference's |lat| >= QD_OCEAN_POLAR_LAT test, evaluated by the host
    double* sst_prev = nullptr;       // [cells] SST at the previous [OceanE] firing
    int have_prev = 0;
    double* partial = nullptr;        // [QD_BD_NQ][nlat]
    double* rec = nullptr;            // the record of the step in progress
    QdSpanLane lane;
};

// ------------------------------------------------------------------ stage 1: one workgroup per row
__global__ void __launch_bounds__(QD_BLOCK)
k_bd_energy(QdGeom G, QdTabs T, QdColP P, QdBdOps O, const double* __restrict__ isr, const double* __restrict__ albedo,
            const double* __restrict__ cloud, const double* __restrict__ Ts, const double* __restrict__ h,
            const double* __restrict__ u, const double* __restrict__ v, const uint8_t* __restrict__ land,
            const double* __restrict__ hice, const double* __restrict__ LH, double* __restrict__ partial) {
    const int i = blockIdx.x;
    const size_t b = (size_t)i * G.nlon;
    const double w = T.warea[i];
    double acc[QD_BD_NQ] = {0, 0, 0, 0, 0, 0, 0, 0};
    for (int j = threadIdx.x; j < G.nlon; j += QD_BLOCK) {
        const size_t o = b + j;
        const double ts = Ts[o], I = isr[o];
        const QdFlux F = qd_surface_fluxes(P, I, albedo[o], cloud[o], ts, 288.0 + P.ga * h[o], u[o], v[o], land[o] == 1, hice[o]);
        const double toa = I - F.R - F.OLR, sfc = F.SW_sfc - F.LW_sfc - F.SH - LH[o];
        acc[0] += toa * w; acc[1] += sfc * w; acc[2] += (toa - sfc) * w;
        if (ts == ts) { acc[3] += ts; acc[4] += 1.0; }
    }
    qd_block_partials(acc, 5, O.op, partial, gridDim.x, blockIdx.x);
}

struct QdBdOceanE { double inv_dt, ice_qfac; int use_ice, have_prev; };
__global__ void __launch_bounds__(QD_BLOCK)
k_bd_ocean_energy(QdGeom G, QdTabs T, QdBdOceanE K, QdBdOps O, const double* __restrict__ sst, const double* __restrict__ qnet,
                  const uint8_t* __restrict__ land, const uint8_t* __restrict__ ice, const uint8_t* __restrict__ polar_row,
                  double* __restrict__ prev, double* __restrict__ partial) {
    const int i = blockIdx.x;
    const size_t b = (size_t)i * G.nlon;
    const double w = T.warea[i];
    const bool prow = polar_row[i] != 0;
    double acc[QD_BD_NQ] = {0, 0, 0, 0, 0, 0, 0, 0};
    for (int j = threadIdx.x; j < G.nlon; j += QD_BLOCK) {
        const size_t o = b + j;
        const bool ocean = land[o] == 0, iced = K.use_ice && ice[o] != 0;
        const double t = qd_nn(sst[o]), q = qnet[o];
        // eff_Q: Q_net over open ocean, ice_qfac Q_net under ice (only when ice_qfac > 0), 0 on land
        const double eq = !ocean ? 0.0 : (!iced ? q : (K.ice_qfac > 0.0 ? K.ice_qfac * q : 0.0));
        const double m = ocean ? 1.0 : 0.0;
        const double dT = K.have_prev ? (t - prev[o]) * K.inv_dt : 0.0;
        acc[0] += eq * w; acc[1] += (dT * w) * m; acc[2] += w * m;
        if (prow && ocean) { acc[3] += eq * w; acc[4] += dT * w; acc[5] += w; acc[6] += 1.0; }
        prev[o] = t;
    }
    acc[7] = K.have_prev ? 1.0 : 0.0;
    qd_block_partials(acc, 8, O.op, partial, gridDim.x, blockIdx.x);
}

__global__ void __launch_bounds__(QD_BLOCK)
k_bd_ocean(QdGeom G, QdTabs T, QdBdOps O, const double* __restrict__ uo, const double* __restrict__ vo, const double* __restrict__ eta,
           double* __restrict__ partial) {
    const int i = blockIdx.x;
    const size_t b = (size_t)i * G.nlon;
    const double w = T.warea[i];
    double acc[QD_BD_NQ] = {0, -INFINITY, INFINITY, -INFINITY, 0, 0, 0, 0};
    for (int j = threadIdx.x; j < G.nlon; j += QD_BLOCK) {
        const size_t o = b + j;
        const double a = uo[o], c = vo[o], e = eta[o];
        const double s2 = a * a + c * c;
        acc[0] += (0.5 * s2) * w;
        acc[1] = fmax(acc[1], sqrt(s2)); acc[2] = fmin(acc[2], e); acc[3] = fmax(acc[3], e);
    }
    qd_block_partials(acc, 4, O.op, partial, gridDim.x, blockIdx.x);
}

__global__ void __launch_bounds__(QD_BLOCK)
k_bd_humidity(QdGeom G, QdTabs T, QdBdOps O, const double* __restrict__ E, const double* __restrict__ Pc, const double* __restrict__ LH,
              const double* __restrict__ LHrel, double* __restrict__ partial) {
    const int i = blockIdx.x;
    const size_t b = (size_t)i * G.nlon;
    const double w = T.warea[i];
    double acc[QD_BD_NQ] = {0, 0, 0, 0, 0, 0, 0, 0};
    for (int j = threadIdx.x; j < G.nlon; j += QD_BLOCK) {
        const size_t o = b + j;
        acc[0] += E[o] * w; acc[1] += Pc[o] * w; acc[2] += LH[o] * w; acc[3] += LHrel[o] * w;
    }
    qd_block_partials(acc, 4, O.op, partial, gridDim.x, blockIdx.x);
}

__global__ void __launch_bounds__(QD_BLOCK)
k_bd_water(QdGeom G, QdTabs T, QdBdOps O, double cwv_fac, double rho_i, const double* __restrict__ E, const double* __restrict__ P,
           const double* __restrict__ R, const double* __restrict__ q, const double* __restrict__ hice, const double* __restrict__ W,
           const double* __restrict__ S, const double* __restrict__ flow, double* __restrict__ partial) {
    const int i = blockIdx.x;
    const size_t b = (size_t)i * G.nlon;
    const double w = T.warea[i];
    double acc[QD_BD_NQ] = {0, 0, 0, 0, 0, 0, 0, -INFINITY};
    for (int j = threadIdx.x; j < G.nlon; j += QD_BLOCK) {
        const size_t o = b + j;
        acc[0] += E[o] * w; acc[1] += P[o] * w; acc[2] += R[o] * w;
        acc[3] += (cwv_fac * q[o]) * w; acc[4] += (rho_i * hice[o]) * w; acc[5] += W[o] * w; acc[6] += S[o] * w;
        if (flow) acc[7] = fmax(acc[7], flow[o]);              // np.nanmax: fmax drops a NaN operand
    }
    qd_block_partials(acc, flow ? 8 : 7, O.op, partial, gridDim.x, blockIdx.x);
}

// ------------------------------------------------------------------ stage 2: the rows in a fixed order -> the record
__global__ void __launch_bounds__(QD_BLOCK)
k_bd_finish(const double* __restrict__ partial, int nrows, int nq, QdBdOps O, double* __restrict__ rec, int slot0,
            const double* __restrict__ extra, int extra_slot, int ran_slot, double fire) {
    double v[QD_BD_NQ];
#pragma unroll
    for (int q = 0; q < QD_BD_NQ; ++q) v[q] = 0.0;
    qd_planes_strided(partial, nrows, nq, O.op, v);
    qd_block_totals(v, O.op);
    if (threadIdx.x == 0) {
#pragma unroll
        for (int q = 0; q < QD_BD_NQ; ++q)
            if (q < nq) rec[slot0 + q] = v[q];
        if (extra) { rec[extra_slot] = extra[0]; rec[extra_slot + 1] = extra[1]; }
        rec[ran_slot] = 1.0; rec[BD_FIRE] = fire;
    }
}

// ------------------------------------------------------------------ host side
static QdSpanLane* bd_lane(qd_ctx* c) { return c && c->budget ? &c->budget->lane : nullptr; }

void qd_budget_release(qd_ctx* c) {
    QdBudget* b = c->budget;
    if (!b) return;
    if (c->stream) hipStreamSynchronize(c->stream);
    void* p[] = {b->polar_row, b->sst_prev, b->partial, b->lane.log};
    for (void* q : p) if (q) hipFree(q);
    delete b;
    c->budget = nullptr;
}

extern "C" int qd_budget_diag_configure(qd_handle c, int lines, const uint8_t* polar_row) {
    if (!c || !polar_row) return -1;
    if (!qd_whole_globe(c))
        return qd_fail(c, "qd_budget_diag_configure: the budget diagnostics need a whole-globe handle (world == 1, n_rows == n_lat); "
                          "latitude bands are not supported");
    if (lines < 0 || lines > 31) return qd_fail(c, "qd_budget_diag_configure: lines is a mask of QD_BD_LINE_* (0..31)");
    hipSetDevice(c->desc.device);
    qd_budget_release(c);
    QdBudget* b = new QdBudget();
    b->lines = lines; b->lane.width = QD_BUDGET_LOG_W;
    const size_t cells = c->geo.cells();
    const int nlat = c->geo.nlat;
    const bool ok = hipMalloc(&b->polar_row, (size_t)nlat) == hipSuccess && hipMalloc(&b->sst_prev, cells * sizeof(double)) == hipSuccess &&
                    hipMalloc(&b->partial, (size_t)QD_BD_NQ * nlat * sizeof(double)) == hipSuccess &&
                    hipMalloc(&b->lane.log, b->lane.log_doubles() * sizeof(double)) == hipSuccess &&
                    hipMemcpyAsync(b->polar_row, polar_row, (size_t)nlat, hipMemcpyHostToDevice, c->stream) == hipSuccess &&
                    hipMemsetAsync(b->sst_prev, 0, cells * sizeof(double), c->stream) == hipSuccess &&
                    hipMemsetAsync(b->lane.log, 0, b->lane.log_doubles() * sizeof(double), c->stream) == hipSuccess &&
                    hipStreamSynchronize(c->stream) == hipSuccess;
    c->budget = b;
    if (!ok) { qd_budget_release(c); return qd_fail(c, "qd_budget_diag_configure: device allocation or upload failed"); }
    return 0;
}

extern "C" int qd_budget_diag_schedule(qd_handle c, int n, const int32_t* fire) {
    if (c && fire) for (int s = 0; s < n; ++s) if (fire[s] < 0 || fire[s] > 3) return qd_fail(c, "qd_budget_diag_schedule: a step's value is 0..3");
    return qd_lane_schedule(c, bd_lane(c), n, fire, "qd_budget_diag_schedule", "not configured (qd_budget_diag_configure first)");
}
extern "C" int qd_budget_diag_log(qd_handle c, double* out, int max, int* n) {
    return qd_lane_drain(c, bd_lane(c), out, max, n, "qd_budget_diag_log", "not configured (qd_budget_diag_configure first)");
}
extern "C" int qd_budget_diag_reset(qd_handle c) {
    if (!c) return -1;
    if (!c->budget) return qd_fail(c, "qd_budget_diag_reset: not configured (qd_budget_diag_configure first)");
    c->budget->lane.reset(); c->budget->have_prev = 0;
    return 0;
}

bool qd_budget_scheduled(const qd_ctx* c) { return c->budget && !c->budget->lane.sched.empty(); }
int qd_budget_lines(const qd_ctx* c) { return c->budget ? c->budget->lines : 0; }

QdSpanLane* qd_budget_span_begin(qd_ctx* c, int n) {
    static const QdSpanTexts T = {
        "qd_step_n: the budget diagnostics need a whole-globe handle; latitude bands are not supported",
        "qd_step_n: qd_budget_diag_configure has not been called",
        "qd_step_n: a qd_budget_diag_schedule must cover exactly the n steps of the span",
        "qd_step_n: the span's budget records would overflow the log (drain it with qd_budget_diag_log first)"};
    return qd_lane_span_begin(c, bd_lane(c), n, T);
}

// a firing step begins: its record, zeroed (a position that does not run leaves zeros and no ran flag)
int qd_budget_begin_step(qd_ctx* c) {
    QdBudget* b = c->budget;
    if (b->lane.full()) return qd_fail(c, "qd_step_n: budget log full (drain it with qd_budget_diag_log)");
    b->rec = b->lane.next();
    QD_HIP(c, hipMemsetAsync(b->rec, 0, QD_BUDGET_LOG_W * sizeof(double), c->stream));
    return 0;
}

static void bd_finish(qd_ctx* c, int nq, const QdBdOps& O, int slot0, int pos, double fire, const double* extra = nullptr, int extra_slot = 0) {
    QdBudget* b = c->budget;
    hipLaunchKernelGGL(k_bd_finish, dim3(1), dim3(QD_BLOCK), 0, c->stream, (const double*)b->partial, c->geo.nlat, nq, O, b->rec, slot0,
                       extra, extra_slot, BD_RAN + pos, fire);
}

int qd_budget_energy(qd_ctx* c, double fire) {
    QdBudget* b = c->budget;
    double** F = c->f;
    QdScope sc(c, "budget_diag");
    const QdColP P = qd_make_colp_driver(c, 0.0);
    const double* cl = c->cloud_eff_valid ? F[QD_F_CLOUD_EFF] : F[QD_F_CLOUD];
    const QdBdOps O = bd_ops({});
    hipLaunchKernelGGL(k_bd_energy, dim3(c->geo.nlat), dim3(QD_BLOCK), 0, c->stream, c->geo, c->tabs, P, O, (const double*)F[QD_F_ISR],
                       (const double*)F[QD_F_ALBEDO], cl, (const double*)F[QD_F_TS], (const double*)F[QD_F_H], (const double*)F[QD_F_U],
                       (const double*)F[QD_F_V], (const uint8_t*)c->land, (const double*)F[QD_F_HICE], (const double*)F[QD_F_LH], b->partial);
    bd_finish(c, 5, O, BD_E_TOA, 0, fire);
    return 0;
}

int qd_budget_ocean_energy(qd_ctx* c, double dt, int use_ice_mask) {
    QdBudget* b = c->budget;
    double** F = c->f;
    QdScope sc(c, "budget_diag");
    const QdBdOceanE K{1.0 / std::max(1e-12, dt), c->p.ocean_ice_qfac, use_ice_mask ? 1 : 0, b->have_prev};
    const QdBdOps O = bd_ops({QD_RED_SUM, QD_RED_SUM, QD_RED_SUM, QD_RED_SUM, QD_RED_SUM, QD_RED_SUM, QD_RED_SUM, QD_RED_MAX});
    hipLaunchKernelGGL(k_bd_ocean_energy, dim3(c->geo.nlat), dim3(QD_BLOCK), 0, c->stream, c->geo, c->tabs, K, O, (const double*)F[QD_F_SST],
                       (const double*)F[QD_F_QNET], (const uint8_t*)c->land, (const uint8_t*)c->icemask, (const uint8_t*)b->polar_row,
                       b->sst_prev, b->partial);
    bd_finish(c, 8, O, BD_OE_Q, 1, c->budget_fire);
    b->have_prev = 1;
    return 0;
}

int qd_budget_ocean(qd_ctx* c, double fire) {
    QdBudget* b = c->budget;
    double** F = c->f;
    QdScope sc(c, "budget_diag");
    const QdBdOps O = bd_ops({QD_RED_SUM, QD_RED_MAX, QD_RED_MIN, QD_RED_MAX});
    hipLaunchKernelGGL(k_bd_ocean, dim3(c->geo.nlat), dim3(QD_BLOCK), 0, c->stream, c->geo, c->tabs, O, (const double*)F[QD_F_UO],
                       (const double*)F[QD_F_VO], (const double*)F[QD_F_ETA], b->partial);
    bd_finish(c, 4, O, BD_O_KE, 2, fire);
    return 0;
}

int qd_budget_humidity(qd_ctx* c, double fire) {
    QdBudget* b = c->budget;
    double** F = c->f;
    QdScope sc(c, "budget_diag");
    const QdBdOps O = bd_ops({});
    hipLaunchKernelGGL(k_bd_humidity, dim3(c->geo.nlat), dim3(QD_BLOCK), 0, c->stream, c->geo, c->tabs, O, (const double*)F[QD_F_EFLUX],
                       (const double*)F[QD_F_PCOND], (const double*)F[QD_F_LH], (const double*)F[QD_F_LHREL], b->partial);
    bd_finish(c, 4, O, BD_H_E, 3, fire);
    return 0;
}

int qd_budget_water(qd_ctx* c, double fire, int with_route) {
    QdBudget* b = c->budget;
    double** F = c->f;
    QdScope sc(c, "budget_diag");
    const double* flow = with_route ? qd_route_flow(c) : nullptr;
    const double* last = with_route ? qd_route_last_record(c) : nullptr;      // {.., .., ocean_kgps, closure, ..}: nullptr before the first event
    const QdBdOps O = bd_ops({QD_RED_SUM, QD_RED_SUM, QD_RED_SUM, QD_RED_SUM, QD_RED_SUM, QD_RED_SUM, QD_RED_SUM, QD_RED_MAX});
    hipLaunchKernelGGL(k_bd_water, dim3(c->geo.nlat), dim3(QD_BLOCK), 0, c->stream, c->geo, c->tabs, O, c->p.rho_a * c->p.h_mbl, c->p.rho_i,
                       (const double*)F[QD_F_EFLUX], (const double*)F[QD_F_PRECIP], (const double*)F[QD_F_RUNOFF], (const double*)F[QD_F_Q],
                       (const double*)F[QD_F_HICE], (const double*)F[QD_F_W_LAND], (const double*)F[QD_F_S_SNOW], flow, b->partial);
    bd_finish(c, flow ? 8 : 7, O, BD_W_E, 4, fire, last ? last + 2 : nullptr, BD_W_INFLOW);
    return 0;
}
