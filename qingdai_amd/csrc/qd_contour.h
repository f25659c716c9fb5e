// qd_contour.h -- what the two contour-band renderers share (qd_stateframe.hip, qd_tiles.hip), device side, gfx950.
//
// A tile is matplotlib's contourf sampled at the cell centres: sf_band_of finds the band of a value, sf_on_coast the reference's
// coast contour (ax.contour(land_mask, levels=[0.5])) as a cell rule, sf_mark_hit the two star marks, sf_u8 the store.  QdSfBest /
// sf_better are np.argmax as a total-order selection.  All of it is integer logic or comparisons: nothing here rounds.
#pragma once
#include "qd_internal.h"

__device__ __forceinline__ bool sf_finite(double x) { return fabs(x) <= DBL_MAX; }

// np.argmax as a selection: a NaN beats every number, a larger value beats a smaller one, the lower flat index breaks ties
struct QdSfBest { double v, i; int nan; };
__device__ __forceinline__ QdSfBest sf_better(const QdSfBest& a, const QdSfBest& b) {
    const bool take_a = (a.nan != b.nan) ? (a.nan != 0) : ((!a.nan && a.v != b.v) ? (a.v > b.v) : (a.i <= b.i));
    QdSfBest r;                                                 // field by field: a select of whole structs goes through scratch
    r.v = take_a ? a.v : b.v; r.i = take_a ? a.i : b.i; r.nan = take_a ? a.nan : b.nan;
    return r;
}
__device__ __forceinline__ QdSfBest sf_wave_best(QdSfBest x) {
#pragma unroll
    for (int o = 32; o > 0; o >>= 1) {
        QdSfBest y;
        y.v = __shfl_down(x.v, o, 64); y.i = __shfl_down(x.i, o, 64); y.nan = __shfl_down(x.nan, o, 64);
        x = sf_better(x, y);
    }
    return x;
}
__device__ __forceinline__ QdSfBest sf_none() { QdSfBest b; b.v = -INFINITY; b.i = INFINITY; b.nan = 0; return b; }

// the band of z in n levels: -1 = white; the extended band has the index n - 1.  dead: the tile has no usable range.
__device__ __forceinline__ int sf_band_of(const double* __restrict__ levels, int n, bool dead, bool extend_max, double z) {
    if (n < 2 || dead || !sf_finite(z)) return -1;
    int lo = 0, hi = n;                                         // the number of levels <= z
    while (lo < hi) {
        const int mid = (lo + hi) >> 1;
        if (levels[mid] <= z) lo = mid + 1; else hi = mid;
    }
    if (lo == 0) return -1;
    if (lo < n) return lo - 1;
    if (z == levels[n - 1]) return n - 2;                       // the last band is closed above
    return extend_max ? n - 1 : -1;
}

__device__ __forceinline__ uint8_t sf_u8(double x) {
    const double q = floor(x * 255.0 + 0.5);
    return (x == x) ? (uint8_t)(q > 255.0 ? 255.0 : (q < 0.0 ? 0.0 : q)) : (uint8_t)0;
}

// a land cell with an ocean 4-neighbour: longitude periodic, latitude clipped (the caller has found land[row][col] == 1)
__device__ __forceinline__ bool sf_on_coast(const uint8_t* __restrict__ land, int nlat, int nlon, int row, int col) {
    const int rn = row + 1 < nlat ? row + 1 : row, rs = row > 0 ? row - 1 : row;
    const int ce = qd_wrapc(col + 1, nlon), cw = qd_wrapc(col - 1, nlon);
    return land[(size_t)rn * nlon + col] == 0 || land[(size_t)rs * nlon + col] == 0 || land[(size_t)row * nlon + ce] == 0 ||
           land[(size_t)row * nlon + cw] == 0;
}

// does the mark at the flat cell m cover (row, col)?  plus == false: an x (the centre and its four diagonal neighbours); plus ==
// true: a + (the centre and its four edge neighbours).  Columns wrap, rows do not.
__device__ __forceinline__ bool sf_mark_hit(bool plus, long long m, int nlon, int row, int col) {
    const int mr = (int)(m / nlon), mc = (int)(m - (long long)mr * nlon);
    const int dr = row - mr;
    int dc = col - mc; if (dc < 0) dc += nlon;
    const int adc = dc == 0 ? 0 : ((dc == 1 || dc == nlon - 1) ? 1 : 2);
    const int adr = dr < 0 ? -dr : dr;
    const bool centre = adr == 0 && adc == 0;
    return plus ? (centre || (adr == 0 && adc == 1) || (adr == 1 && adc == 0)) : (centre || (adr == 1 && adc == 1));
}
