// qd_tiles.hip -- the ecology, plankton and ISR figures from the resident state, gfx950 (qd_tiles_*).
//
// plot_plankton_species (scripts/run_simulation.py:828-889), plot_isr_components (:891-951) and plot_ecology (:954-1060) hand up
// to five planes each to contourf.  Here a figure is one row of up to QD_TILES_MAX tiles with the state frame's geometry, band rule,
// coast rule, marks and u8 store (qd_contour.h); what a tile shows is a (source, index) pair, tl_value below.
//   k_tl_scan / k_tl_scan_final   one thread per (plane, cell), then one workgroup: min / max over the finite values, a NaN flag and
//                      the np.argmax cell of up to 8 planes.  Total-order selections: exact whatever the launch shape.
//   k_tl_hist / k_tl_narrow       the order statistics np.nanpercentile sorts for: a radix select on the order-preserving 64-bit key
//                      of the double (sign bit flipped for a positive, every bit for a negative), most significant digit first.
//                      DIGIT WIDTH 8 BITS, 8 PASSES.  Per pass k_tl_hist (at most QD_TL_SEL_BLOCKS workgroups, grid-strided) counts,
//                      for each requested rank, the digits of the cells whose key matches that rank's prefix so far: one 256-bin
//                      histogram per rank in LDS (4 x 256 x 4 B = 4 KiB of the 160 KiB; integer LDS atomics, so the counts do not
//                      depend on the order of arrival), stored as one partial per workgroup; k_tl_narrow (one workgroup, thread b
//                      = bin b) adds the partials and walks the 256 totals to the bin that holds the rank.  All ranks share the
//                      passes.  A wider digit would save passes -- 11 bits: 6 passes, 32 KiB, 16 bits does not fit -- but the
//                      finish is bins x workgroups x ranks additions in one workgroup and the plane (8 MB at 721 x 1440) stays in
//                      the L2 / MALL between the passes, so a pass costs about its two launches either way; 8 bits keeps the
//                      finish at one bin per thread.  The result is a value of the plane: exact and repeatable.
//   k_tl_render<WANT>  one thread per (tile, cell): the plane again, the band search in the tile's levels (a device buffer, one table
//                      per handle: nothing is shared between handles), coast, mark, u8 store.  WANT keeps band indices and planes.
// Stack sources reduce the [S][K] LAI planes plane after plane in NumPy's order (np.sum over a leading axis); np.maximum propagates
// NaN (qd_max).  f64, contraction off (Makefile), no floating-point atomics, vector stores only.  Reads the state, changes none.
#include "qd_internal.h"
#include "qd_blockred.h"
#include "qd_contour.h"
#include <cstring>
#include <string>

#define QD_TL_G QD_STATEFRAME_GUTTER
#define QD_TL_ML QD_STATEFRAME_MAX_LEVELS
#define QD_TL_BINS 256
#define QD_TL_SEL_BLOCKS 256
#define QD_TL_NR QD_TILES_MAX_RANKS
#define QD_TL_SCAN_PLANES 6            // per plane of the scan: min, max, NaN flag, best value, best index, best is-NaN

typedef unsigned long long tl_u64;

struct QdTlSel {                       // the select's state on the device
    tl_u64 prefix[QD_TL_NR];           // the digits found so far, in place; the lower bits are zero
    tl_u64 rank[QD_TL_NR];             // the rank among the cells that match the prefix
    tl_u64 n;                          // non-NaN cells (the first pass counts them)
    int bad[QD_TL_NR];                 // the rank is not below n
};

struct QdTlSrc {                       // what tl_value reads
    int nlat, nlon, cells;
    const uint8_t* land;
    const void *lai, *alpha, *banded; int lai32, alpha32, banded32;      // eco slabs, f32 under qd_eco_params.map_f32
    const double* L; int S, K;         // the LAI stack [S][K][cells] or nullptr
    double hscale;
    const double* phyto; size_t phyto_stride; int phyto_S;               // the tracer stack or nullptr
    const double *isrA, *isrB;
    const double* host;                // a caller's plane (qd_tiles_set_plane) or nullptr
};

struct QdTiles {
    int configured = 0, have_img = 0, have_stacks = 0, n_tiles = 0;
    double hscale = 10.0;
    size_t cells = 0;
    double* stage = nullptr; size_t stage_cap = 0; int hS = 0, hK = 0;   // a host-passed stack
    double* hplane = nullptr; int have_hplane = 0;                       // a host-passed plane [cells]
    uint8_t* img = nullptr; size_t img_cap = 0; int mw = 0, mh = 0;      // [mh][mw][3]
    int8_t* band = nullptr; double* planes = nullptr;                    // [QD_TILES_MAX][cells], allocated by the first render that wants them
    qd_tile_desc* table = nullptr;          // device [QD_TILES_MAX]
    qd_tile_ref* refs = nullptr;       // device [QD_TILES_MAX]
    QdPartials partial;                // [QD_TILES_MAX * QD_TL_SCAN_PLANES][nblk]
    double* out = nullptr;             // device [QD_TILES_MAX][5]
    unsigned int* hist = nullptr;      // [QD_TL_SEL_BLOCKS][QD_TL_NR][QD_TL_BINS]
    QdTlSel* sel = nullptr;
    int nblk = 0;
};

__device__ __forceinline__ double tl_slab(const void* p, int f32, int o) {
    return f32 ? (double)((const float*)p)[o] : ((const double*)p)[o];
}

// the plane of (source, index) at cell o, as the reference hands it to contourf.  The host has checked that the source can be read.
__device__ __forceinline__ double tl_value(const QdTlSrc& A, int source, int index, int o) {
    switch (source) {
    case QD_TILE_LAI: return qd_nn(tl_slab(A.lai, A.lai32, o));
    case QD_TILE_ALPHA: return qd_nn(tl_slab(A.alpha, A.alpha32, o));
    case QD_TILE_ALPHA_BANDED: return qd_nn(tl_slab(A.banded, A.banded32, o));
    case QD_TILE_CANOPY_HEIGHT: {
        // population.py:310-319: LAI_by_k = sum_s max(L, 0); num = sum_k ((k + 1) / K) LAI_by_k; den = sum_k LAI_by_k + 1e-12
        if (A.land[o] != 1) return 0.0;                         // NaN over the ocean, then nan_to_num
        double num = 0.0, den = 0.0;
        for (int k = 0; k < A.K; ++k) {
            double by_k = 0.0;
            for (int s = 0; s < A.S; ++s) {
                const double v = qd_max(A.L[(size_t)(s * A.K + k) * A.cells + o], 0.0);
                by_k = (s == 0) ? v : by_k + v;
            }
            const double t = ((double)(k + 1) / (double)A.K) * by_k;
            num = (k == 0) ? t : num + t;
            den = (k == 0) ? by_k : den + by_k;
        }
        return qd_nn(A.hscale * (num / (den + 1e-12)));
    }
    case QD_TILE_SPECIES_DENSITY: {
        if (A.land[o] != 1) return 0.0;                         // population.py:336-339
        double x = 0.0;
        for (int k = 0; k < A.K; ++k) {
            const double v = qd_max(A.L[(size_t)(index * A.K + k) * A.cells + o], 0.0);
            x = (k == 0) ? v : x + v;
        }
        return qd_nn(x);
    }
    case QD_TILE_PLANKTON: return A.land[o] == 1 ? NAN : A.phyto[(size_t)index * A.phyto_stride + o];
    case QD_TILE_ISR_A: return A.isrA[o];
    case QD_TILE_ISR_B: return A.isrB[o];
    default: return qd_nn(A.host[o]);
    }
}

// ------------------------------------------------------------------ scan
__global__ void __launch_bounds__(QD_BLOCK)
k_tl_scan(QdTlSrc A, const qd_tile_ref* __restrict__ refs, double* __restrict__ partial) {
    const int o = blockIdx.x * QD_BLOCK + threadIdx.x;
    const int t = blockIdx.y;
    double lo = INFINITY, hi = -INFINITY, flag = 0.0;
    QdSfBest best = sf_none();
    if (o < A.cells) {
        const double z = tl_value(A, refs[t].source, refs[t].index, o);
        if (sf_finite(z)) { lo = z; hi = z; }
        if (z != z) flag = 1.0;
        best.v = z; best.i = (double)o; best.nan = z != z;
    }
    __shared__ double sm[5][QD_BLOCK / 64];
    __shared__ int sn[QD_BLOCK / 64];
    lo = qd_wave_fmin(lo); hi = qd_wave_fmax(hi); flag = qd_wave_fmax(flag); best = sf_wave_best(best);
    const int lane = threadIdx.x & 63, wv = threadIdx.x >> 6;
    if (lane == 0) { sm[0][wv] = lo; sm[1][wv] = hi; sm[2][wv] = flag; sm[3][wv] = best.v; sm[4][wv] = best.i; sn[wv] = best.nan; }
    __syncthreads();
    if (threadIdx.x == 0) {
        QdSfBest b; b.v = sm[3][0]; b.i = sm[4][0]; b.nan = sn[0];
        for (int k = 1; k < QD_BLOCK / 64; ++k) {
            lo = fmin(lo, sm[0][k]); hi = fmax(hi, sm[1][k]); flag = fmax(flag, sm[2][k]);
            QdSfBest y; y.v = sm[3][k]; y.i = sm[4][k]; y.nan = sn[k];
            b = sf_better(b, y);
        }
        const size_t nblk = gridDim.x;
        double* q = partial + (size_t)t * QD_TL_SCAN_PLANES * nblk + blockIdx.x;
        q[0] = lo; q[nblk] = hi; q[2 * nblk] = flag; q[3 * nblk] = b.v; q[4 * nblk] = b.i; q[5 * nblk] = b.nan ? 1.0 : 0.0;
    }
}

// one workgroup, one wave per plane (4 waves take the planes in turn): out[t] = {min, max, flag, best value, best index}
__global__ void __launch_bounds__(QD_BLOCK)
k_tl_scan_final(const double* __restrict__ partial, int nblk, int n, double* __restrict__ out) {
    const int lane = threadIdx.x & 63, wv = threadIdx.x >> 6;
    for (int t = wv; t < n; t += QD_BLOCK / 64) {
        const double* q = partial + (size_t)t * QD_TL_SCAN_PLANES * nblk;
        double lo = INFINITY, hi = -INFINITY, flag = 0.0;
        QdSfBest b = sf_none();
        for (int k = lane; k < nblk; k += 64) {
            lo = fmin(lo, q[k]); hi = fmax(hi, q[(size_t)nblk + k]); flag = fmax(flag, q[2 * (size_t)nblk + k]);
            QdSfBest y; y.v = q[3 * (size_t)nblk + k]; y.i = q[4 * (size_t)nblk + k]; y.nan = q[5 * (size_t)nblk + k] != 0.0;
            b = sf_better(b, y);
        }
        lo = qd_wave_fmin(lo); hi = qd_wave_fmax(hi); flag = qd_wave_fmax(flag); b = sf_wave_best(b);
        if (lane == 0) { double* r = out + 5 * t; r[0] = lo; r[1] = hi; r[2] = flag; r[3] = b.v; r[4] = b.i; }
    }
}

// ------------------------------------------------------------------ order statistics
// the order-preserving key: x < y  <=>  key(x) < key(y) for every pair of non-NaN doubles but (-0, +0), which NumPy calls equal
__device__ __forceinline__ tl_u64 tl_key(double x) {
    const tl_u64 b = (tl_u64)__double_as_longlong(x);
    return (b >> 63) ? ~b : (b | 0x8000000000000000ull);
}
__device__ __forceinline__ double tl_unkey(tl_u64 k) {
    const tl_u64 b = (k >> 63) ? (k & 0x7fffffffffffffffull) : ~k;
    return __longlong_as_double((long long)b);
}

// pass `pass` (0 = the top byte): hist[blk][q][d] = this workgroup's cells whose key agrees with prefix[q] above the digit and has d there
__global__ void __launch_bounds__(QD_BLOCK)
k_tl_hist(QdTlSrc A, int source, int index, int n_ranks, int pass, const QdTlSel* __restrict__ sel, unsigned int* __restrict__ hist) {
    __shared__ unsigned int h[QD_TL_NR][QD_TL_BINS];
    for (int k = threadIdx.x; k < QD_TL_NR * QD_TL_BINS; k += QD_BLOCK) (&h[0][0])[k] = 0u;
    const int shift = 56 - 8 * pass;
    const tl_u64 mask = pass == 0 ? 0ull : (~0ull << (shift + 8));
    tl_u64 pre[QD_TL_NR];
#pragma unroll
    for (int q = 0; q < QD_TL_NR; ++q) pre[q] = (q < n_ranks && pass > 0) ? sel->prefix[q] : 0ull;
    __syncthreads();
    for (int o = blockIdx.x * QD_BLOCK + threadIdx.x; o < A.cells; o += gridDim.x * QD_BLOCK) {
        const double z = tl_value(A, source, index, o);
        if (z != z) continue;
        const tl_u64 key = tl_key(z);
        const int d = (int)((key >> shift) & 0xffull);
#pragma unroll
        for (int q = 0; q < QD_TL_NR; ++q)
            if (q < n_ranks && (key & mask) == pre[q]) atomicAdd(&h[q][d], 1u);
    }
    __syncthreads();
    unsigned int* dst = hist + (size_t)blockIdx.x * QD_TL_NR * QD_TL_BINS;
    for (int k = threadIdx.x; k < QD_TL_NR * QD_TL_BINS; k += QD_BLOCK) dst[k] = (&h[0][0])[k];
}

// one workgroup of QD_TL_BINS threads: thread b adds bin b of every partial; thread 0 walks the totals to the bin of each rank
__global__ void __launch_bounds__(QD_TL_BINS)
k_tl_narrow(const unsigned int* __restrict__ hist, int nblk, int n_ranks, int pass, QdTlSel* __restrict__ sel) {
    __shared__ tl_u64 tot[QD_TL_NR][QD_TL_BINS];
    const int b = threadIdx.x;
    for (int q = 0; q < n_ranks; ++q) {
        tl_u64 a = 0;
        for (int k = 0; k < nblk; ++k) a += hist[((size_t)k * QD_TL_NR + q) * QD_TL_BINS + b];
        tot[q][b] = a;
    }
    __syncthreads();
    if (b == 0) {
        const int shift = 56 - 8 * pass;
        if (pass == 0) {
            tl_u64 n = 0;
            for (int d = 0; d < QD_TL_BINS; ++d) n += tot[0][d];
            sel->n = n;
        }
        for (int q = 0; q < n_ranks; ++q) {
            if (pass > 0 && sel->bad[q]) continue;
            tl_u64 r = sel->rank[q], cum = 0;
            int found = -1;
            for (int d = 0; d < QD_TL_BINS; ++d) {
                const tl_u64 c = tot[q][d];
                if (r < cum + c) { found = d; break; }
                cum += c;
            }
            if (found < 0) { sel->bad[q] = 1; continue; }
            sel->bad[q] = 0;
            sel->prefix[q] = (pass == 0 ? 0ull : sel->prefix[q]) | ((tl_u64)found << shift);
            sel->rank[q] = r - cum;
        }
    }
}

// ------------------------------------------------------------------ render
template <bool WANT>
__global__ void __launch_bounds__(QD_BLOCK)
k_tl_render(QdTlSrc A, const qd_tile_desc* __restrict__ table, uint8_t* __restrict__ img, int mw, int8_t* __restrict__ band,
            double* __restrict__ planes) {
    const int o = blockIdx.x * QD_BLOCK + threadIdx.x;
    const int t = blockIdx.y;
    if (o >= A.cells) return;
    const qd_tile_desc& P = table[t];
    const int row = o / A.nlon, col = o - row * A.nlon;
    const double z = P.unavailable ? NAN : tl_value(A, P.source, P.index, o);
    const int bi = sf_band_of(P.levels, P.n_levels, P.constant != 0 || P.unavailable != 0, P.extend_max != 0, z);
    double r = 1.0, g = 1.0, b = 1.0;
    if (bi >= 0) { r = P.rgb[bi][0]; g = P.rgb[bi][1]; b = P.rgb[bi][2]; }
    if (P.coast && A.land[o] == 1 && sf_on_coast(A.land, A.nlat, A.nlon, row, col)) {
        const double c = P.coast == 2 ? 1.0 : 0.0;
        r = c; g = c; b = c;
    }
    if (P.mark_kind && P.mark_cell >= 0 && P.mark_cell < A.cells && sf_mark_hit(P.mark_kind == 2, P.mark_cell, A.nlon, row, col)) {
        r = P.mark_kind == 2 ? 1.0 : 0.0; g = 1.0; b = P.mark_kind == 2 ? 0.0 : 1.0;      // yellow +, cyan x
    }
    if (WANT) {
        band[(size_t)t * A.cells + o] = (int8_t)bi;
        planes[(size_t)t * A.cells + o] = z;
    }
    const size_t y = (size_t)QD_TL_G + (size_t)(A.nlat - 1 - row);
    const size_t x = (size_t)QD_TL_G + (size_t)t * (A.nlon + QD_TL_G) + (size_t)col;
    uint8_t* q8 = img + (y * (size_t)mw + x) * 3;
    q8[0] = sf_u8(r); q8[1] = sf_u8(g); q8[2] = sf_u8(b);
}

// ------------------------------------------------------------------ host side
void qd_tiles_release(qd_ctx* c) {
    QdTiles* d = c->tiles;
    if (!d) return;
    void* p[] = {d->stage, d->hplane, d->img, d->band, d->planes, d->table, d->refs, d->partial.p, d->out, d->hist, d->sel};
    for (void* q : p) if (q) hipFree(q);
    delete d;
    c->tiles = nullptr;
}

static const char* TL_BANDS = "the figure tiles need a whole-globe handle (world == 1, n_rows == n_lat); latitude bands are not supported";

extern "C" int qd_tiles_configure(qd_handle c, double height_scale, const double* layers, int n_species, int n_layers) {
    if (!c) return -1;
    if (!qd_whole_globe(c)) return qd_fail(c, (std::string("qd_tiles_configure: ") + TL_BANDS).c_str());
    if (layers) {
        if (n_species < 1 || n_species > QD_MAX_SPECIES) return qd_fail(c, "qd_tiles_configure: n_species out of range (1..64)");
        if (n_layers < 1 || n_layers > QD_ECO_DAILY_MAX_K) return qd_fail(c, "qd_tiles_configure: n_layers out of range (1..8)");
    }
    const size_t cells = (size_t)c->geo.nlat * (size_t)c->geo.nlon;
    if (cells > (size_t)INT_MAX / 64) return qd_fail(c, "qd_tiles_configure: grid too large");
    hipSetDevice(c->desc.device);
    QdTiles* d = c->tiles;
    if (!d) d = c->tiles = new QdTiles();
    d->configured = d->have_img = d->have_stacks = 0;
    QD_HIP(c, hipStreamSynchronize(c->stream));
    d->cells = cells;
    d->nblk = (int)((cells + QD_BLOCK - 1) / QD_BLOCK);
    if (!d->table) QD_HIP(c, hipMalloc(&d->table, QD_TILES_MAX * sizeof(qd_tile_desc)));
    if (!d->refs) QD_HIP(c, hipMalloc(&d->refs, QD_TILES_MAX * sizeof(qd_tile_ref)));
    if (!d->out) QD_HIP(c, hipMalloc(&d->out, QD_TILES_MAX * 5 * sizeof(double)));
    if (!d->hist) QD_HIP(c, hipMalloc(&d->hist, (size_t)QD_TL_SEL_BLOCKS * QD_TL_NR * QD_TL_BINS * sizeof(unsigned int)));
    if (!d->sel) QD_HIP(c, hipMalloc(&d->sel, sizeof(QdTlSel)));
    if (int rc = d->partial.ensure(c, QD_TILES_MAX * QD_TL_SCAN_PLANES, d->nblk)) return rc;
    d->hS = d->hK = 0; d->have_hplane = 0;
    if (layers) {
        const size_t n = (size_t)n_species * n_layers * cells;
        if (!d->stage || d->stage_cap < n) {
            if (d->stage) { hipFree(d->stage); d->stage = nullptr; d->stage_cap = 0; }
            QD_HIP(c, hipMalloc(&d->stage, n * sizeof(double)));
            d->stage_cap = n;
        }
        QD_HIP(c, hipMemcpy(d->stage, layers, n * sizeof(double), hipMemcpyHostToDevice));
        d->hS = n_species; d->hK = n_layers;
    }
    d->hscale = height_scale;
    d->configured = 1;
    return 0;
}

extern "C" int qd_tiles_set_plane(qd_handle c, const double* plane) {
    if (!c || !plane) return -1;
    QdTiles* d = c->tiles;
    if (!qd_whole_globe(c)) return qd_fail(c, (std::string("qd_tiles_set_plane: ") + TL_BANDS).c_str());
    if (!d || !d->configured) return qd_fail(c, "qd_tiles_set_plane: qd_tiles_configure has not been called");
    hipSetDevice(c->desc.device);
    QD_HIP(c, hipStreamSynchronize(c->stream));                // an earlier render may still read the plane
    if (!d->hplane) QD_HIP(c, hipMalloc(&d->hplane, d->cells * sizeof(double)));
    QD_HIP(c, hipMemcpy(d->hplane, plane, d->cells * sizeof(double), hipMemcpyHostToDevice));
    d->have_hplane = 1;
    return 0;
}

extern "C" int qd_tiles_available(qd_handle c, int32_t* out3) {
    if (!c || !out3) return -1;
    const QdEco& E = c->eco;
    out3[0] = E.have_lai ? 1 : 0; out3[1] = E.alpha_valid ? 1 : 0; out3[2] = E.banded_valid ? 1 : 0;
    return 0;
}

// fills the sources and checks that (source, index) can be read on this handle
static int tl_src(qd_ctx* c, const char* who, QdTiles* d, QdTlSrc& A, const int* source, const int* index, int n, int stride) {
    double** F = c->f;
    A.nlat = c->geo.nlat; A.nlon = c->geo.nlon; A.cells = (int)d->cells;
    A.land = c->land;
    A.lai = F[QD_F_ECO_LAI]; A.alpha = F[QD_F_ECO_ALPHA]; A.banded = F[QD_F_ECO_ALPHA_BANDED];
    A.lai32 = qd_eco_is_f32(c, QD_F_ECO_LAI) ? 1 : 0; A.alpha32 = qd_eco_is_f32(c, QD_F_ECO_ALPHA) ? 1 : 0;
    A.banded32 = qd_eco_is_f32(c, QD_F_ECO_ALPHA_BANDED) ? 1 : 0;
    A.L = nullptr; A.S = A.K = 0;
    if (d->hS) { A.L = d->stage; A.S = d->hS; A.K = d->hK; }
    else if (!qd_eco_daily_stack(c, &A.L, &A.S, &A.K)) { A.L = nullptr; A.S = A.K = 0; }
    A.hscale = d->hscale;
    A.phyto = c->phyto.S ? c->phyto.stack[0] + (size_t)c->geo.halo * c->geo.nlon : nullptr;
    A.phyto_stride = c->phyto.stride; A.phyto_S = c->phyto.S;
    A.isrA = F[QD_F_ISR_A]; A.isrB = F[QD_F_ISR_B];
    A.host = d->have_hplane ? d->hplane : nullptr;
    for (int k = 0; k < n; ++k) {
        const int s = source[(size_t)k * stride], i = index[(size_t)k * stride];
        if (s < QD_TILE_LAI || s > QD_TILE_HOST_PLANE) return qd_fail(c, (std::string(who) + ": unknown tile source").c_str());
        if (s == QD_TILE_CANOPY_HEIGHT || s == QD_TILE_SPECIES_DENSITY) {
            if (!A.L)
                return qd_fail(c, (std::string(who) + ": a stack source needs the resident stack of qd_eco_daily_configure or a host stack "
                                   "(qd_tiles_configure); there is neither").c_str());
            if (s == QD_TILE_SPECIES_DENSITY && (i < 0 || i >= A.S))
                return qd_fail(c, (std::string(who) + ": species index out of range").c_str());
        }
        if (s == QD_TILE_HOST_PLANE && !A.host) return qd_fail(c, (std::string(who) + ": no host plane on this handle (qd_tiles_set_plane first)").c_str());
        if (s == QD_TILE_PLANKTON) {
            if (!A.phyto) return qd_fail(c, (std::string(who) + ": no tracers on this handle (qd_phyto_configure first)").c_str());
            if (i < 0 || i >= A.phyto_S) return qd_fail(c, (std::string(who) + ": species index out of range").c_str());
        }
    }
    return 0;
}

static QdTiles* tl_ready(qd_ctx* c, const char* who) {
    if (!qd_whole_globe(c)) { qd_fail(c, (std::string(who) + ": " + TL_BANDS).c_str()); return nullptr; }
    QdTiles* d = c->tiles;
    if (!d || !d->configured) { qd_fail(c, (std::string(who) + ": qd_tiles_configure has not been called").c_str()); return nullptr; }
    return d;
}

extern "C" int qd_tiles_scan(qd_handle c, const qd_tile_ref* refs, int n, double* out, int64_t* argmax_cell) {
    if (!c || !refs || !out || !argmax_cell) return -1;
    const char* who = "qd_tiles_scan";
    QdTiles* d = tl_ready(c, who);
    if (!d) return -1;
    if (n < 1 || n > QD_TILES_MAX) return qd_fail(c, "qd_tiles_scan: the list holds 1..QD_TILES_MAX (8) planes");
    hipSetDevice(c->desc.device);
    QdTlSrc A;
    if (int rc = tl_src(c, who, d, A, &refs[0].source, &refs[0].index, n, 2)) return rc;
    QD_HIP(c, hipMemcpyAsync(d->refs, refs, (size_t)n * sizeof(qd_tile_ref), hipMemcpyHostToDevice, c->stream));
    {
        QdScope sc(c, "tiles_scan");
        hipLaunchKernelGGL(k_tl_scan, dim3(d->nblk, n), dim3(QD_BLOCK), 0, c->stream, A, d->refs, d->partial.p);
        hipLaunchKernelGGL(k_tl_scan_final, dim3(1), dim3(QD_BLOCK), 0, c->stream, d->partial.p, d->nblk, n, d->out);
    }
    double host[QD_TILES_MAX * 5];
    QD_HIP(c, hipMemcpyAsync(host, d->out, (size_t)n * 5 * sizeof(double), hipMemcpyDeviceToHost, c->stream));
    QD_HIP(c, hipStreamSynchronize(c->stream));
    const hipError_t e = hipGetLastError();
    if (e != hipSuccess) return qd_fail(c, "qd_tiles_scan: kernel", e);
    for (int k = 0; k < n; ++k) {
        for (int j = 0; j < 4; ++j) out[4 * k + j] = host[5 * k + j];
        const double i = host[5 * k + 4];
        argmax_cell[k] = (i >= 0.0 && i < (double)d->cells) ? (int64_t)i : -1;
    }
    return 0;
}

extern "C" int qd_tiles_order_stats(qd_handle c, int source, int index, const int64_t* ranks, int n_ranks, double* values, int64_t* count) {
    if (!c || !count || (n_ranks > 0 && (!ranks || !values))) return -1;
    const char* who = "qd_tiles_order_stats";
    QdTiles* d = tl_ready(c, who);
    if (!d) return -1;
    if (n_ranks < 0 || n_ranks > QD_TL_NR) return qd_fail(c, "qd_tiles_order_stats: at most QD_TILES_MAX_RANKS (4) ranks a call");
    for (int q = 0; q < n_ranks; ++q)
        if (ranks[q] < 0) return qd_fail(c, "qd_tiles_order_stats: a rank is negative");
    hipSetDevice(c->desc.device);
    QdTlSrc A;
    if (int rc = tl_src(c, who, d, A, &source, &index, 1, 1)) return rc;
    QdTlSel h{};
    const int nr = n_ranks > 0 ? n_ranks : 1;                  // the count alone: one rank, whose value is dropped
    for (int q = 0; q < n_ranks; ++q) h.rank[q] = (tl_u64)ranks[q];
    QD_HIP(c, hipMemcpyAsync(d->sel, &h, sizeof(h), hipMemcpyHostToDevice, c->stream));
    const int nblk = d->nblk < QD_TL_SEL_BLOCKS ? d->nblk : QD_TL_SEL_BLOCKS;
    {
        QdScope sc(c, "tiles_select");
        const int passes = n_ranks > 0 ? 8 : 1;               // the count alone is the total of the first pass
        for (int pass = 0; pass < passes; ++pass) {
            hipLaunchKernelGGL(k_tl_hist, dim3(nblk), dim3(QD_BLOCK), 0, c->stream, A, source, index, nr, pass, d->sel, d->hist);
            hipLaunchKernelGGL(k_tl_narrow, dim3(1), dim3(QD_TL_BINS), 0, c->stream, d->hist, nblk, nr, pass, d->sel);
        }
    }
    QD_HIP(c, hipMemcpyAsync(&h, d->sel, sizeof(h), hipMemcpyDeviceToHost, c->stream));
    QD_HIP(c, hipStreamSynchronize(c->stream));
    const hipError_t e = hipGetLastError();
    if (e != hipSuccess) return qd_fail(c, "qd_tiles_order_stats: kernel", e);
    *count = (int64_t)h.n;
    for (int q = 0; q < n_ranks; ++q) {
        if (h.bad[q] || (tl_u64)ranks[q] >= h.n) { values[q] = NAN; continue; }
        const tl_u64 b = (h.prefix[q] >> 63) ? (h.prefix[q] & 0x7fffffffffffffffull) : ~h.prefix[q];
        std::memcpy(&values[q], &b, sizeof(double));
    }
    return 0;
}

extern "C" int qd_tiles_render(qd_handle c, const qd_tile_desc* tiles, size_t sz, int n, int want_stacks) {
    if (!c || !tiles) return -1;
    const char* who = "qd_tiles_render";
    if (sz != sizeof(qd_tile_desc)) return qd_fail(c, "qd_tiles_render: struct size mismatch (ABI)");
    QdTiles* d = tl_ready(c, who);
    if (!d) return -1;
    if (n < 1 || n > QD_TILES_MAX) return qd_fail(c, "qd_tiles_render: a figure holds 1..QD_TILES_MAX (8) tiles");
    hipSetDevice(c->desc.device);
    QdTlSrc A;
    qd_tile_ref live[QD_TILES_MAX];
    int n_live = 0;
    for (int t = 0; t < n; ++t) {
        const qd_tile_desc& P = tiles[t];
        const bool dead = P.constant || P.unavailable;
        if (P.n_levels > QD_TL_ML) return qd_fail(c, "qd_tiles_render: a tile has more than QD_STATEFRAME_MAX_LEVELS (32) levels");
        if (P.n_levels < 0 || (!dead && P.n_levels < 2))
            return qd_fail(c, "qd_tiles_render: a tile that is neither constant nor unavailable needs at least 2 levels");
        if (P.coast < 0 || P.coast > 2) return qd_fail(c, "qd_tiles_render: coast must be 0 (none), 1 (black) or 2 (white)");
        if (P.mark_kind < 0 || P.mark_kind > 2) return qd_fail(c, "qd_tiles_render: mark_kind must be 0 (none), 1 (cyan x) or 2 (yellow +)");
        if (!P.unavailable) { live[n_live].source = P.source; live[n_live].index = P.index; ++n_live; }
    }
    if (int rc = tl_src(c, who, d, A, &live[0].source, &live[0].index, n_live, 2)) return rc;
    const size_t cells = d->cells;
    d->have_img = d->have_stacks = 0;
    QD_HIP(c, hipStreamSynchronize(c->stream));                // an earlier render may still read the table and the mosaic
    const int mw = n * c->geo.nlon + (n + 1) * QD_TL_G, mh = c->geo.nlat + 2 * QD_TL_G;
    const size_t bytes = (size_t)mw * mh * 3;
    if (!d->img || d->img_cap < bytes) {
        if (d->img) { hipFree(d->img); d->img = nullptr; d->img_cap = 0; }
        QD_HIP(c, hipMalloc(&d->img, bytes));
        d->img_cap = bytes;
    }
    if (want_stacks && !d->band) {
        QD_HIP(c, hipMalloc(&d->band, (size_t)QD_TILES_MAX * cells));
        QD_HIP(c, hipMalloc(&d->planes, (size_t)QD_TILES_MAX * cells * sizeof(double)));
    }
    QD_HIP(c, hipMemcpy(d->table, tiles, (size_t)n * sizeof(qd_tile_desc), hipMemcpyHostToDevice));
    QD_HIP(c, hipMemsetAsync(d->img, 255, bytes, c->stream));  // the gutters
    {
        QdScope sc(c, "tiles_render");
        const dim3 grid(d->nblk, n), block(QD_BLOCK);
        if (want_stacks) hipLaunchKernelGGL(k_tl_render<true>, grid, block, 0, c->stream, A, d->table, d->img, mw, d->band, d->planes);
        else hipLaunchKernelGGL(k_tl_render<false>, grid, block, 0, c->stream, A, d->table, d->img, mw, (int8_t*)nullptr, (double*)nullptr);
    }
    QD_HIP(c, hipStreamSynchronize(c->stream));
    const hipError_t e = hipGetLastError();
    if (e != hipSuccess) return qd_fail(c, "qd_tiles_render: kernel", e);
    d->mw = mw; d->mh = mh; d->n_tiles = n;
    d->have_img = 1; d->have_stacks = want_stacks ? 1 : 0;
    return 0;
}

extern "C" int qd_tiles_download(qd_handle c, int which, void* host, size_t n) {
    if (!c || !host) return -1;
    const QdTiles* d = c->tiles;
    if (!d || !d->have_img) return qd_fail(c, "qd_tiles_download: no figure on this handle (call qd_tiles_render first)");
    if (which < 0 || which > 2) return qd_fail(c, "qd_tiles_download: which must be 0 (u8 mosaic), 1 (int8 band indices) or 2 (f64 planes)");
    if (which != 0 && !d->have_stacks) return qd_fail(c, "qd_tiles_download: the last render did not keep the stacks (want_stacks)");
    if (n != (which == 0 ? (size_t)d->mw * d->mh * 3 : (size_t)d->n_tiles * d->cells)) return qd_fail(c, "qd_tiles_download: size mismatch");
    hipSetDevice(c->desc.device);
    const void* src = which == 0 ? (const void*)d->img : (which == 1 ? (const void*)d->band : (const void*)d->planes);
    QD_HIP(c, hipMemcpyAsync(host, src, which == 2 ? n * sizeof(double) : n, hipMemcpyDeviceToHost, c->stream));
    QD_HIP(c, hipStreamSynchronize(c->stream));
    return 0;
}
