// qd_stateframe.hip -- the reference's 15-panel status figure from the resident state, gfx950 (qd_stateframe_*).
//
// plot_state (scripts/run_simulation.py:330-537) hands fifteen derived maps to contourf.  Here a frame is a mosaic of 5 x 3 tiles
// of n_lat x n_lon pixels (one pixel per cell, northernmost row on top, a white gutter of QD_STATEFRAME_GUTTER pixels), each tile
// the reference's contourf sampled at the cell centres: a cell takes the colour of the band i with levels[i] <= z < levels[i + 1],
// the last band closed above; non-finite z and z outside every band are white; extend="max" (panel 5) colours z above the top.
//   k_sf_scan          one thread per cell: the fifteen fields in f64 in the reference's operation order, the vorticity plane
//                      (qd_divvort_point, the arithmetic of qd_op_vorticity), and per workgroup one partial of every extreme a level
//                      rule needs -- min / max of T_s, T_a, SST (Celsius; a NaN of T_a is flagged, np.min propagates it), min / max
//                      over the FINITE values of the panels 3, 7, 8, 9, 10, 12, 13, 14, 15, nanmax |vort| -- and of the two argmax
//                      cells of isr_A / isr_B as np.argmax finds them (a NaN beats every number, ties go to the lowest flat index).
//   k_sf_final         one workgroup: the partials -> QD_STATEFRAME_SCAN_N doubles and the two cells.
//                      min, max and this argmax are a total-order selection: the result does not depend on the order in which the
//                      partials are combined, so it is exact and repeatable whatever the launch shape.
//   k_sf_render<WANT>  one thread per (panel, cell): blockIdx.y is the panel, consecutive lanes are consecutive longitudes.  The
//                      field again (or the vorticity plane), an upper-bound search in at most 32 levels of the table in constant
//                      memory, the overlays in the reference's order -- coast (a land cell with an ocean 4-neighbour, longitude
//                      periodic, latitude clipped), rivers and lakes on the panels 1 and 8, the two star marks on panel 10 -- and the
//                      u8 store min(255, floor(x 255 + 0.5)).  WANT also keeps the band index (int8, -1 = white) and the f64 field.
// The gutters are a memset of the mosaic to white in front of the launch.  f64, contraction off (Makefile), no atomics, vector
// stores only; sqrt is the only rounded library operation and it is correctly rounded.
#include "qd_internal.h"
#include "qd_blockred.h"
#include "qd_contour.h"
#include "qd_device.h"
#include <mutex>

#define QD_SF_NP QD_STATEFRAME_PANELS
#define QD_SF_ML QD_STATEFRAME_MAX_LEVELS
#define QD_SF_G QD_STATEFRAME_GUTTER
#define QD_SF_NRED 26                  // quantities reduced through qd_block_partials: QD_STATEFRAME_SCAN_N less the two argmax values

// One table per module and device, shared by every handle: qd_stateframe_render holds g_sf_table_lock from the upload until its
// launch has drained, so renders of handles on other host threads take turns and none draws with another's table.
__constant__ qd_stateframe_table g_sf_table;
static std::mutex g_sf_table_lock;

struct QdStateFrame {
    qd_stateframe_params p{};
    int configured = 0, have_scan = 0, have_img = 0, have_stacks = 0;
    long long scan_atm = -1, scan_ocn = -1;   // the handle's step counters when the scan ran: a render on a stepped state is refused
    size_t cells = 0, mosaic = 0;      // mosaic: bytes
    int mw = 0, mh = 0;
    uint8_t* img = nullptr;            // [mh][mw][3]
    int8_t* band = nullptr;            // [15][cells], allocated by the first render that wants it
    double* fields = nullptr;          // [15][cells], likewise
    double* vort = nullptr;            // [cells]
    QdPartials partial;                // [QD_SF_NRED + 6][nblk]
    double* out = nullptr;             // device [QD_STATEFRAME_SCAN_N + 2]
    double* flow = nullptr;            // a caller's flow map (qd_stateframe_render)
    uint8_t* lake = nullptr;
    qd_stateframe_table table{};       // the host copy the constant-memory upload reads
    double last[QD_STATEFRAME_SCAN_N + 2] = {0};
};

struct QdSfArgs {
    QdGeom G; QdTabs T;
    int nlat, nlon, cells;
    qd_stateframe_params p;
    double a, dlat, dlon;
    const uint8_t* land;
    const double *ts, *h, *sst, *precip, *cloud, *u, *v, *uo, *vo, *isr, *isrA, *isrB, *albedo, *olr, *q, *eflux, *pcond;
    const double* flow; const uint8_t* lake;
    double* vort;
    double* partial;
    uint8_t* img; int mw; int8_t* band; double* fields;
};

// the field of panel p (0-based) at cell o (run_simulation.py:345-498); panel 8 (the vorticity) is read from its plane
__device__ __forceinline__ double sf_field(const QdSfArgs& K, int p, int o) {
    const double g = 9.81;
    switch (p) {
    case 0: return qd_nn(K.ts[o] - 273.15);
    case 1: return (288.0 + (g / 1004.0) * K.h[o]) - 273.15;
    case 2: return K.p.ps_abs ? (K.p.p0 + (K.p.rho_a * g) * K.h[o]) * 1e-2 : ((K.p.rho_a * g) * K.h[o]) * 1e-2;
    case 3: return qd_nn((K.p.ocean ? K.sst[o] : K.ts[o]) - 273.15);
    case 4: return qd_nn(K.precip[o]) * 86400.0;
    case 5: return K.cloud[o];
    case 6: { const double a = qd_nn(K.u[o]), b = qd_nn(K.v[o]); return sqrt(a * a + b * b); }
    case 7: {
        if (!K.p.ocean) return K.h[o] - K.p.H;
        const double a = qd_nn(K.uo[o]), b = qd_nn(K.vo[o]);
        return sqrt(a * a + b * b);
    }
    case 8: return K.vort[o];
    case 9: return K.isr[o];
    case 10: return K.albedo[o];
    case 11: return K.olr[o];
    case 12: return 1e3 * qd_nn(K.q[o]);
    case 13: return qd_nn(K.eflux[o]) * 86400.0;
    default: return qd_nn(K.pcond[o]) * 86400.0;
    }
}

// slots of the scan result (QD_STATEFRAME_SCAN_N doubles; include/qingdai_hip.h names them): 0..2 the minima of T_s, T_a, SST, 3..5
// their maxima, 6..14 the nine auto panels' minima, 15..23 their maxima, 24 |vort|, 25 the NaN flag of T_a.  The table lives in device
// memory: a lane indexes it by its own id (sf_block_reduce), which a table built in registers could only serve from scratch.
#define QD_SF_MIN9 QD_RED_MIN, QD_RED_MIN, QD_RED_MIN, QD_RED_MIN, QD_RED_MIN, QD_RED_MIN, QD_RED_MIN, QD_RED_MIN, QD_RED_MIN
#define QD_SF_MAX9 QD_RED_MAX, QD_RED_MAX, QD_RED_MAX, QD_RED_MAX, QD_RED_MAX, QD_RED_MAX, QD_RED_MAX, QD_RED_MAX, QD_RED_MAX
__device__ const QdRedOp g_sf_ops[QD_SF_NRED] = {QD_RED_MIN, QD_RED_MIN, QD_RED_MIN, QD_RED_MAX, QD_RED_MAX, QD_RED_MAX, QD_SF_MIN9,
                                                 QD_SF_MAX9, QD_RED_MAX, QD_RED_MAX};
__device__ __forceinline__ constexpr bool sf_slot_is_min(int k) { return k < 3 || (k >= 6 && k < 15); }
__device__ __forceinline__ double sf_join(int k, double a, double b) { return sf_slot_is_min(k) ? fmin(a, b) : fmax(a, b); }

// the workgroup's value of every slot -> dst[q * stride + b], by thread q: the wave step of qd_blockred.h with the operation of each
// slot known at compile time (every v[] index is a constant: the array stays in registers), then its LDS step
__device__ __forceinline__ void sf_block_reduce(const double (&v)[QD_SF_NRED], double* __restrict__ dst, size_t stride, size_t b) {
    __shared__ double sm[QD_SF_NRED][QD_BLOCK / 64];
    const int lane = threadIdx.x & 63, wv = threadIdx.x >> 6;
#pragma unroll
    for (int q = 0; q < QD_SF_NRED; ++q) {
        const double r = sf_slot_is_min(q) ? qd_wave_fmin(v[q]) : qd_wave_fmax(v[q]);
        if (lane == 0) sm[q][wv] = r;
    }
    __syncthreads();
    const int q = threadIdx.x;
    if (q < QD_SF_NRED) dst[(size_t)q * stride + b] = qd_block_total(sm, q, g_sf_ops[q]);
}

__global__ void __launch_bounds__(QD_BLOCK)
k_sf_scan(QdSfArgs K) {
    const int o = blockIdx.x * QD_BLOCK + threadIdx.x;
    double v[QD_SF_NRED];
#pragma unroll
    for (int k = 0; k < QD_SF_NRED; ++k) v[k] = sf_slot_is_min(k) ? INFINITY : -INFINITY;
    QdSfBest bA = sf_none(), bB = sf_none();
    if (o < K.cells) {
        const int row = o / K.nlon, col = o - row * K.nlon;
        const double w = qd_divvort_point(K.G, K.T, K.v, K.u, row, col, K.a, K.dlat, K.dlon, 1);
        K.vort[o] = w;
        const double ts = sf_field(K, 0, o), ta = sf_field(K, 1, o), sst = sf_field(K, 3, o);
        v[0] = ts; v[3] = ts; v[2] = sst; v[5] = sst;
        if (ta == ta) { v[1] = ta; v[4] = ta; v[25] = 0.0; } else v[25] = 1.0;
        const int auto_panel[9] = {2, 6, 7, 8, 9, 11, 12, 13, 14};
#pragma unroll
        for (int k = 0; k < 9; ++k) {
            const double z = auto_panel[k] == 8 ? w : sf_field(K, auto_panel[k], o);
            if (sf_finite(z)) { v[6 + k] = z; v[15 + k] = z; }
        }
        const double aw = fabs(w);
        if (aw == aw) v[24] = aw;                               // np.nanmax(np.abs(vort))
        const double A = K.isrA[o], B = K.isrB[o];
        bA.v = A; bA.i = (double)o; bA.nan = A != A;
        bB.v = B; bB.i = (double)o; bB.nan = B != B;
    }
    sf_block_reduce(v, K.partial, (size_t)gridDim.x, (size_t)blockIdx.x);
    // the two argmax candidates of this workgroup: wave shuffles, then one small LDS step
    __shared__ double sv[2][QD_BLOCK / 64], si[2][QD_BLOCK / 64];
    __shared__ int sn[2][QD_BLOCK / 64];
    bA = sf_wave_best(bA); bB = sf_wave_best(bB);
    const int lane = threadIdx.x & 63, wv = threadIdx.x >> 6;
    if (lane == 0) { sv[0][wv] = bA.v; si[0][wv] = bA.i; sn[0][wv] = bA.nan; sv[1][wv] = bB.v; si[1][wv] = bB.i; sn[1][wv] = bB.nan; }
    __syncthreads();
    if (threadIdx.x < 2) {
        const int s = threadIdx.x;
        QdSfBest b; b.v = sv[s][0]; b.i = si[s][0]; b.nan = sn[s][0];
        for (int k = 1; k < QD_BLOCK / 64; ++k) { QdSfBest y; y.v = sv[s][k]; y.i = si[s][k]; y.nan = sn[s][k]; b = sf_better(b, y); }
        double* q = K.partial + (size_t)(QD_SF_NRED + 3 * s) * gridDim.x + blockIdx.x;
        q[0] = b.v; q[(size_t)gridDim.x] = b.i; q[2 * (size_t)gridDim.x] = b.nan ? 1.0 : 0.0;
    }
}

__global__ void __launch_bounds__(QD_BLOCK)
k_sf_final(const double* __restrict__ partial, int nblk, double* __restrict__ out) {
    double v[QD_SF_NRED];
#pragma unroll
    for (int q = 0; q < QD_SF_NRED; ++q) {                     // block-strided over the plane of slot q
        double a = sf_slot_is_min(q) ? INFINITY : -INFINITY;
        for (int k = threadIdx.x; k < nblk; k += QD_BLOCK) a = sf_join(q, a, partial[(size_t)q * nblk + k]);
        v[q] = a;
    }
    sf_block_reduce(v, out, 1, 0);                             // one workgroup: its values are the totals, out[q] by thread q
    const int lane = threadIdx.x & 63, wv = threadIdx.x >> 6;
    if (wv < 2) {                                               // wave 0: star A, wave 1: star B
        const double* q = partial + (size_t)(QD_SF_NRED + 3 * wv) * nblk;
        QdSfBest b = sf_none();
        for (int k = lane; k < nblk; k += 64) {
            QdSfBest y; y.v = q[k]; y.i = q[(size_t)nblk + k]; y.nan = q[2 * (size_t)nblk + k] != 0.0;
            b = sf_better(b, y);
        }
        b = sf_wave_best(b);
        if (lane == 0) { out[26 + wv] = b.v; out[QD_STATEFRAME_SCAN_N + wv] = b.i; }
    }
}

// the band of z in the panel's levels: -1 = white; the extended band has the index n_levels - 1 (qd_contour.h)
__device__ __forceinline__ int sf_band(const qd_stateframe_panel& P, double z) {
    return sf_band_of(P.levels, P.n_levels, P.constant != 0, P.extend_max != 0, z);
}

template <bool WANT>
__global__ void __launch_bounds__(QD_BLOCK)
k_sf_render(QdSfArgs K) {
    const int o = blockIdx.x * QD_BLOCK + threadIdx.x;
    const int p = blockIdx.y;
    if (o >= K.cells) return;
    const qd_stateframe_panel& P = g_sf_table.panel[p];
    const int row = o / K.nlon, col = o - row * K.nlon;
    const double z = sf_field(K, p, o);
    const int bi = sf_band(P, z);
    double r = 1.0, g = 1.0, b = 1.0;
    if (bi >= 0) { r = P.rgb[bi][0]; g = P.rgb[bi][1]; b = P.rgb[bi][2]; }
    const bool land = K.land[o] == 1;
    if (P.coast && land && sf_on_coast(K.land, K.nlat, K.nlon, row, col)) {
        const double c = P.coast == 2 ? 1.0 : 0.0;
        r = c; g = c; b = c;
    }
    if (p == 0 || p == 7) {
        if (K.flow && land && K.flow[o] >= K.p.river_min) {     // deepskyblue
            const double al = K.p.river_alpha;
            r = r * (1.0 - al) + 0.0 * al; g = g * (1.0 - al) + 0.749 * al; b = b * (1.0 - al) + 1.0 * al;
        }
        if (K.lake && K.lake[o]) {                              // dodgerblue
            const double al = K.p.lake_alpha;
            r = r * (1.0 - al) + 0.118 * al; g = g * (1.0 - al) + 0.565 * al; b = b * (1.0 - al) + 1.0 * al;
        }
    }
    if (p == 9) {
#pragma unroll
        for (int s = 0; s < 2; ++s) {                           // star A: a cyan x; then star B: a yellow +
            const long long m = g_sf_table.mark_cell[s];
            if (m < 0 || m >= K.cells) continue;
            const bool hit = sf_mark_hit(s == 1, m, K.nlon, row, col);
            if (hit) { r = s == 0 ? 0.0 : 1.0; g = 1.0; b = s == 0 ? 1.0 : 0.0; }
        }
    }
    if (WANT) {
        K.band[(size_t)p * K.cells + o] = (int8_t)bi;
        K.fields[(size_t)p * K.cells + o] = z;
    }
    const int tr = p / 3, tc = p - 3 * tr;
    const size_t y = (size_t)QD_SF_G + (size_t)tr * (K.nlat + QD_SF_G) + (size_t)(K.nlat - 1 - row);
    const size_t x = (size_t)QD_SF_G + (size_t)tc * (K.nlon + QD_SF_G) + (size_t)col;
    uint8_t* q8 = K.img + (y * (size_t)K.mw + x) * 3;
    q8[0] = sf_u8(r); q8[1] = sf_u8(g); q8[2] = sf_u8(b);
}

// ------------------------------------------------------------------ host side
void qd_stateframe_release(qd_ctx* c) {
    QdStateFrame* d = c->sframe;
    if (!d) return;
    void* p[] = {d->img, d->band, d->fields, d->vort, d->partial.p, d->out, d->flow, d->lake};
    for (void* q : p) if (q) hipFree(q);
    delete d;
    c->sframe = nullptr;
}

static const char* SF_BANDS = "the state frame needs a whole-globe handle (world == 1, n_rows == n_lat); latitude bands are not supported";

extern "C" int qd_stateframe_configure(qd_handle c, const qd_stateframe_params* p, size_t sz, const uint8_t* lake_mask) {
    if (!c || !p) return -1;
    if (sz != sizeof(qd_stateframe_params)) return qd_fail(c, "qd_stateframe_configure: struct size mismatch (ABI)");
    if (!qd_whole_globe(c)) return qd_fail(c, (std::string("qd_stateframe_configure: ") + SF_BANDS).c_str());
    if (p->lakes && !lake_mask) return qd_fail(c, "qd_stateframe_configure: lakes set without a lake mask");
    const size_t cells = (size_t)c->geo.nlat * (size_t)c->geo.nlon;
    if (cells > (size_t)INT_MAX / 64) return qd_fail(c, "qd_stateframe_configure: grid too large");
    hipSetDevice(c->desc.device);
    QdStateFrame* d = c->sframe;
    if (!d) d = c->sframe = new QdStateFrame();
    d->configured = d->have_scan = d->have_img = d->have_stacks = 0;
    QD_HIP(c, hipStreamSynchronize(c->stream));
    d->cells = cells;
    d->mw = QD_SF_NP / 5 * c->geo.nlon + (QD_SF_NP / 5 + 1) * QD_SF_G;
    d->mh = 5 * c->geo.nlat + 6 * QD_SF_G;
    d->mosaic = (size_t)d->mw * d->mh * 3;
    if (!d->img) QD_HIP(c, hipMalloc(&d->img, d->mosaic));
    if (!d->vort) QD_HIP(c, hipMalloc(&d->vort, cells * sizeof(double)));
    if (!d->out) QD_HIP(c, hipMalloc(&d->out, (QD_STATEFRAME_SCAN_N + 2) * sizeof(double)));
    if (int rc = d->partial.ensure(c, QD_SF_NRED + 6, (int)((cells + QD_BLOCK - 1) / QD_BLOCK))) return rc;
    if (lake_mask) {
        if (!d->lake) QD_HIP(c, hipMalloc(&d->lake, cells));
        QD_HIP(c, hipMemcpy(d->lake, lake_mask, cells, hipMemcpyHostToDevice));
    }
    d->p = *p;
    d->configured = 1;
    return 0;
}

static void sf_args(qd_ctx* c, QdStateFrame* d, QdSfArgs& K) {
    double** F = c->f;
    K.G = c->geo; K.T = c->tabs;
    K.nlat = c->geo.nlat; K.nlon = c->geo.nlon; K.cells = (int)d->cells;
    K.p = d->p;
    K.a = c->p.a; K.dlat = c->dlat; K.dlon = c->dlon;
    K.land = c->land;
    K.ts = F[QD_F_TS]; K.h = F[QD_F_H]; K.sst = F[QD_F_SST]; K.precip = F[QD_F_PRECIP]; K.cloud = F[QD_F_CLOUD];
    K.u = F[QD_F_U]; K.v = F[QD_F_V]; K.uo = F[QD_F_UO]; K.vo = F[QD_F_VO];
    K.isr = F[QD_F_ISR]; K.isrA = F[QD_F_ISR_A]; K.isrB = F[QD_F_ISR_B];
    K.albedo = F[QD_F_ALBEDO]; K.olr = F[QD_F_OLR]; K.q = F[QD_F_Q]; K.eflux = F[QD_F_EFLUX]; K.pcond = F[QD_F_PCOND];
    K.flow = nullptr; K.lake = nullptr;
    K.vort = d->vort; K.partial = d->partial.p;
    K.img = d->img; K.mw = d->mw; K.band = nullptr; K.fields = nullptr;
}

extern "C" int qd_stateframe_scan(qd_handle c, double* out, int64_t* mark_cells) {
    if (!c || !out || !mark_cells) return -1;
    if (!qd_whole_globe(c)) return qd_fail(c, (std::string("qd_stateframe_scan: ") + SF_BANDS).c_str());
    QdStateFrame* d = c->sframe;
    if (!d || !d->configured) return qd_fail(c, "qd_stateframe_scan: qd_stateframe_configure has not been called");
    hipSetDevice(c->desc.device);
    d->have_scan = 0;
    QdSfArgs K;
    sf_args(c, d, K);
    {
        QdScope sc(c, "stateframe_scan");
        const dim3 block(QD_BLOCK);
        hipLaunchKernelGGL(k_sf_scan, dim3(d->partial.nblk), block, 0, c->stream, K);
        hipLaunchKernelGGL(k_sf_final, dim3(1), block, 0, c->stream, d->partial.p, d->partial.nblk, d->out);
    }
    QD_HIP(c, hipMemcpyAsync(d->last, d->out, sizeof(d->last), hipMemcpyDeviceToHost, c->stream));
    QD_HIP(c, hipStreamSynchronize(c->stream));
    const hipError_t e = hipGetLastError();
    if (e != hipSuccess) return qd_fail(c, "qd_stateframe_scan: kernel", e);
    for (int k = 0; k < QD_STATEFRAME_SCAN_N; ++k) out[k] = d->last[k];
    for (int s = 0; s < 2; ++s) {
        const double i = d->last[QD_STATEFRAME_SCAN_N + s];
        mark_cells[s] = (i >= 0.0 && i < (double)d->cells) ? (int64_t)i : -1;
    }
    d->scan_atm = (long long)c->atm_counter; d->scan_ocn = (long long)c->ocn_counter;
    d->have_scan = 1;
    return 0;
}

extern "C" int qd_stateframe_render(qd_handle c, const qd_stateframe_table* table, size_t sz, const double* flow, int want_stacks) {
    if (!c || !table) return -1;
    if (sz != sizeof(qd_stateframe_table)) return qd_fail(c, "qd_stateframe_render: struct size mismatch (ABI)");
    if (!qd_whole_globe(c)) return qd_fail(c, (std::string("qd_stateframe_render: ") + SF_BANDS).c_str());
    QdStateFrame* d = c->sframe;
    if (!d || !d->configured) return qd_fail(c, "qd_stateframe_render: qd_stateframe_configure has not been called");
    if (!d->have_scan) return qd_fail(c, "qd_stateframe_render: qd_stateframe_scan has not been called (the vorticity plane is its output)");
    if (d->scan_atm != (long long)c->atm_counter || d->scan_ocn != (long long)c->ocn_counter)
        return qd_fail(c, "qd_stateframe_render: the state has been stepped since qd_stateframe_scan (its vorticity plane and extremes are stale); scan again");
    for (int p = 0; p < QD_SF_NP; ++p) {
        const qd_stateframe_panel& P = table->panel[p];
        if (P.n_levels > QD_SF_ML) return qd_fail(c, "qd_stateframe_render: a panel has more than QD_STATEFRAME_MAX_LEVELS (32) levels");
        if (P.n_levels < 0 || (!P.constant && P.n_levels < 2)) return qd_fail(c, "qd_stateframe_render: a panel that is not constant needs at least 2 levels");
        if (P.coast < 0 || P.coast > 2) return qd_fail(c, "qd_stateframe_render: coast must be 0 (none), 1 (black) or 2 (white)");
    }
    hipSetDevice(c->desc.device);
    const size_t cells = d->cells;
    d->have_img = d->have_stacks = 0;
    QdSfArgs K;
    sf_args(c, d, K);
    if (d->p.rivers) {
        if (flow) {
            QD_HIP(c, hipStreamSynchronize(c->stream));        // an earlier render may still read the staging buffer
            if (!d->flow) QD_HIP(c, hipMalloc(&d->flow, cells * sizeof(double)));
            QD_HIP(c, hipMemcpy(d->flow, flow, cells * sizeof(double), hipMemcpyHostToDevice));
            K.flow = d->flow;
        } else {
            K.flow = qd_route_flow(c);
            if (!K.flow) return qd_fail(c, "qd_stateframe_render: rivers are on, flow is NULL and no routing network is configured");
        }
    }
    K.lake = (d->p.lakes && d->lake) ? d->lake : nullptr;
    if (want_stacks && !d->band) {
        QD_HIP(c, hipStreamSynchronize(c->stream));
        QD_HIP(c, hipMalloc(&d->band, (size_t)QD_SF_NP * cells));
        QD_HIP(c, hipMalloc(&d->fields, (size_t)QD_SF_NP * cells * sizeof(double)));
    }
    K.band = want_stacks ? d->band : nullptr; K.fields = want_stacks ? d->fields : nullptr;
    QD_HIP(c, hipStreamSynchronize(c->stream));                // the previous upload of the table has been consumed
    d->table = *table;
    std::lock_guard<std::mutex> turn(g_sf_table_lock);         // released behind the synchronise below, on every return path
    QD_HIP(c, hipMemcpyToSymbolAsync(HIP_SYMBOL(g_sf_table), &d->table, sizeof(qd_stateframe_table), 0, hipMemcpyHostToDevice, c->stream));
    QD_HIP(c, hipMemsetAsync(d->img, 255, d->mosaic, c->stream));      // the gutters
    {
        QdScope sc(c, "stateframe_render");
        const dim3 grid(d->partial.nblk, QD_SF_NP), block(QD_BLOCK);
        if (want_stacks) hipLaunchKernelGGL(k_sf_render<true>, grid, block, 0, c->stream, K);
        else hipLaunchKernelGGL(k_sf_render<false>, grid, block, 0, c->stream, K);
    }
    QD_HIP(c, hipStreamSynchronize(c->stream));
    const hipError_t e = hipGetLastError();
    if (e != hipSuccess) return qd_fail(c, "qd_stateframe_render: kernel", e);
    d->have_img = 1; d->have_stacks = want_stacks ? 1 : 0;
    return 0;
}

extern "C" int qd_stateframe_download(qd_handle c, int which, void* host, size_t n) {
    if (!c || !host) return -1;
    const QdStateFrame* d = c->sframe;
    if (!d || !d->have_img) return qd_fail(c, "qd_stateframe_download: no frame on this handle (call qd_stateframe_render first)");
    if (which < 0 || which > 2) return qd_fail(c, "qd_stateframe_download: which must be 0 (u8 mosaic), 1 (int8 band indices) or 2 (f64 fields)");
    if (which != 0 && !d->have_stacks) return qd_fail(c, "qd_stateframe_download: the last render did not keep the stacks (want_stacks)");
    if (n != (which == 0 ? d->mosaic : (size_t)QD_SF_NP * d->cells)) return qd_fail(c, "qd_stateframe_download: size mismatch");
    hipSetDevice(c->desc.device);
    const void* src = which == 0 ? (const void*)d->img : (which == 1 ? (const void*)d->band : (const void*)d->fields);
    QD_HIP(c, hipMemcpyAsync(host, src, which == 2 ? n * sizeof(double) : n, hipMemcpyDeviceToHost, c->stream));
    QD_HIP(c, hipStreamSynchronize(c->stream));
    return 0;
}
