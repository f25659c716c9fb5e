// qd_hydronet.hip -- the offline river network (P014, scripts/generate_hydrology_maps.py:84-311) built on the device.
//
// Five stages, every output bit-identical to the reference's generator:
//   k_hn_pitfill      pit_fill (:84-109): the row-major Gauss-Seidel sweeps in ONE persistent workgroup
//   k_hn_d8           compute_flow_to_index (:112-150): one lane per cell, distances from host tables
//   k_hn_lake_*       identify_lakes (:174-207): min-label propagation with pointer jumping, ids by a rank of the roots
//   k_hn_outlet_*     compute_lake_outlets (:210-262): two atomic-min passes (elevation key, then candidate ordinal)
//   k_hn_order_*      topo_sort_flow_order (:153-171): Kahn's FIFO order one generation at a time in ONE workgroup
//
// Pit fill.  A sweep visits the rows in order; row j sees row j-1 as updated in this sweep and row j+1, and the cells east of
// each cell, as left by the last sweep.  Cell 0 sees cell n-1 of the last sweep; cell n-1 sees the new cell 0.  So cell 0 is
// computed first, and then every cell i >= 1 is x_i = f_i(x_{i-1}) with
//     f_i(x) = (land && e_i <= m && m + eps > e_i) ? m + eps : e_i,   m = min(x, A_i),
// A_i the min of the non-west neighbours.  f_i is monotone in x, rounding included, so per chunk of HN_PF_C cells a lane runs
// the trajectories from x = -inf and x = +inf; from the first cell where they meet, the chunk no longer depends on its input.
// Only the unmerged prefixes take the true carry from the west: from the nearest merged chunk, walked serially (a long
// east-west valley is that serial walk).  A row is swept only when it can change: row j in sweep s needs row j-1 changed in
// sweep s, or row j or j+1 changed in sweep s-1.  The rows j-1, j, j+1 live in an LDS cache of three rows.
// Whole-globe handles only (the network is global).
#include "qd_internal.h"
#include <cmath>
#include <vector>

#define HN_PF_T 256          // threads of the pit-fill workgroup
#define HN_PF_C 16           // cells per chunk of the in-row chain
#define HN_T 256             // wide kernels and the scan tiles
#define HN_SCAN_PER 8        // elements per thread of a scan tile
#define HN_SCAN_TILE (HN_T * HN_SCAN_PER)
#define HN_SCAN_TOP_T 1024   // the top level of the scan: one workgroup
#define HN_ORDER_T 1024      // the flow-order workgroup
#define HN_NOPICK 0x7f7f7f7f  // the outlet pick before any candidate (a byte memset)
#define HN_MAX_CELLS (HN_SCAN_TILE * HN_SCAN_TOP_T * HN_SCAN_PER)

// loads of data another lane of the same workgroup stored (behind a barrier): L1-bypassing
__device__ __forceinline__ double hn_ld(const double* p) {
    const unsigned long long u = __hip_atomic_load((const unsigned long long*)p, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
    return __longlong_as_double((long long)u);
}
__device__ __forceinline__ int hn_ldi(const int* p) { return __hip_atomic_load(p, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT); }
__device__ __forceinline__ double hn_min(double a, double b) { return b < a ? b : a; }

// ------------------------------------------------------------------ pit fill
__device__ __forceinline__ double hn_f(bool land, double e, double m, double eps) {
    const double me = m + eps;
    return (land && e <= m && me > e) ? me : e;
}

// min of the non-west neighbours of cell i >= 1 of the row (east of n-1 is the new cell 0)
__device__ __forceinline__ double hn_A(int i, int n, const double* up, const double* cur, const double* dn, double x0) {
    const int ip = i + 1 == n ? 0 : i + 1;
    double A = i + 1 == n ? x0 : cur[ip];
    if (up) A = hn_min(hn_min(hn_min(A, up[i - 1]), up[i]), up[ip]);
    if (dn) A = hn_min(hn_min(hn_min(A, dn[i - 1]), dn[i]), dn[ip]);
    return A;
}

__global__ void __launch_bounds__(HN_PF_T)
k_hn_pitfill(int nlat, int nlon, const uint8_t* __restrict__ land, double* e, double eps, int max_iters, int* __restrict__ sweeps_out) {
    extern __shared__ double hn_lds[];
    const int n = nlon, nch = (nlon + HN_PF_C - 1) / HN_PF_C, tid = threadIdx.x;
    double* nv = hn_lds + 3 * n;                       // the row's new values (slots 0..2: the row cache)
    double* tail = hn_lds + 4 * n;                     // [nch] a merged chunk's last value
    int* mrg = (int*)(tail + nch);                     // [nch] cells of the chunk before its trajectories met
    uint8_t* lrow = (uint8_t*)(mrg + nch);             // [n] the row's land flags
    uint8_t* chg_prev = lrow + n;                      // [nlat] changed in the last sweep
    uint8_t* chg_cur = chg_prev + nlat;                // [nlat] changed in this sweep
    int t0 = -1, t1 = -1, t2 = -1;                     // the row each cache slot holds (uniform)
    int s = 0;
    for (int it = 1; it <= max_iters; ++it) {
        s = it;
        bool any = false, prev_changed = false;
        for (int j = 0; j < nlat; ++j) {
            const bool dirty = it == 1 || prev_changed || chg_prev[j] || (j + 1 < nlat && chg_prev[j + 1]);
            bool row_changed = false;
            if (dirty) {
                // rows j-1 (new), j, j+1 into the cache; a missing row goes to a slot that holds none of the three
                const int need[3] = {j - 1, j, j + 1 < nlat ? j + 1 : -1};
                int sl[3];
#pragma unroll
                for (int a = 0; a < 3; ++a)
                    sl[a] = need[a] < 0 ? -1 : t0 == need[a] ? 0 : t1 == need[a] ? 1 : t2 == need[a] ? 2 : -1;
#pragma unroll
                for (int a = 0; a < 3; ++a) {
                    if (need[a] < 0 || sl[a] >= 0) continue;
                    const int b = (sl[0] != 0 && sl[1] != 0 && sl[2] != 0) ? 0 : (sl[0] != 1 && sl[1] != 1 && sl[2] != 1) ? 1 : 2;
                    sl[a] = b;
                    if (b == 0) t0 = need[a]; else if (b == 1) t1 = need[a]; else t2 = need[a];
                    const double* src = e + (size_t)need[a] * n;
                    for (int i = tid; i < n; i += HN_PF_T) hn_lds[b * n + i] = hn_ld(src + i);
                }
                for (int i = tid; i < n; i += HN_PF_T) lrow[i] = land[(size_t)j * n + i] == 1;
                __syncthreads();
                const double* up = sl[0] >= 0 ? hn_lds + sl[0] * n : nullptr;
                double* cur = hn_lds + sl[1] * n;
                const double* dn = sl[2] >= 0 ? hn_lds + sl[2] * n : nullptr;
                // cell 0: every neighbour as the last sweep left it (row j-1: this sweep's)
                double A0 = hn_min(cur[n - 1], cur[1]);
                if (up) A0 = hn_min(hn_min(hn_min(A0, up[n - 1]), up[0]), up[1]);
                if (dn) A0 = hn_min(hn_min(hn_min(A0, dn[n - 1]), dn[0]), dn[1]);
                const double x0 = hn_f(lrow[0], cur[0], A0, eps);
                // per chunk: the trajectories from -inf and +inf until they meet
                for (int k = tid; k < nch; k += HN_PF_T) {
                    const int i0 = k * HN_PF_C, i1 = min(i0 + HN_PF_C, n);
                    double lo = -INFINITY, hi = INFINITY, x = 0.0;
                    int p = i1 - i0;
                    bool met = false;
                    for (int i = i0; i < i1; ++i) {
                        if (i == 0) { x = x0; met = true; p = 0; nv[0] = x0; continue; }
                        const double A = hn_A(i, n, up, cur, dn, x0);
                        const bool l = lrow[i];
                        const double ei = cur[i];
                        if (met) { x = hn_f(l, ei, hn_min(x, A), eps); nv[i] = x; continue; }
                        lo = hn_f(l, ei, hn_min(lo, A), eps);
                        hi = hn_f(l, ei, hn_min(hi, A), eps);
                        if (__double_as_longlong(lo) == __double_as_longlong(hi)) { met = true; p = i - i0; x = lo; nv[i] = x; }
                    }
                    mrg[k] = p;
                    tail[k] = x;
                }
                __syncthreads();
                // unmerged prefixes: the true carry from the nearest merged chunk to the west (chunk 0 always is)
                for (int k = tid; k < nch; k += HN_PF_T) {
                    const int i0 = k * HN_PF_C;
                    if (mrg[k] == 0) continue;
                    int q = k - 1;
                    while (mrg[q] == min(HN_PF_C, n - q * HN_PF_C)) --q;
                    double x = tail[q];
                    for (int i = (q + 1) * HN_PF_C, iend = i0 + mrg[k]; i < iend; ++i) {
                        x = hn_f(lrow[i], cur[i], hn_min(x, hn_A(i, n, up, cur, dn, x0)), eps);
                        if (i >= i0) nv[i] = x;
                    }
                }
                __syncthreads();
                bool ch = false;
                double* dst = e + (size_t)j * n;
                for (int i = tid; i < n; i += HN_PF_T) {
                    const double v = nv[i];
                    if (__double_as_longlong(v) != __double_as_longlong(cur[i])) { ch = true; cur[i] = v; dst[i] = v; }
                }
                asm volatile("s_waitcnt vmcnt(0)" ::: "memory");     // the row is in L2 before any lane reloads it
                row_changed = __syncthreads_or(ch) != 0;
            }
            if (tid == 0) chg_cur[j] = row_changed;
            prev_changed = row_changed;
            any |= row_changed;
        }
        __syncthreads();
        if (!any) break;
        for (int j = tid; j < nlat; j += HN_PF_T) chg_prev[j] = chg_cur[j];
        __syncthreads();
    }
    if (tid == 0) *sweeps_out = s;
}

// ------------------------------------------------------------------ D8 directions
// spherical_distance (:64-81) with the reference's operations in its order; lat / lon in radians and the row-pair cosines
// cos(0.5 (lat_j + lat_jj)) come from the host (NumPy), the rest is IEEE f64 (contraction off, correctly rounded sqrt)
__global__ void __launch_bounds__(HN_T)
k_hn_d8(int nlat, int nlon, const uint8_t* __restrict__ land, const double* __restrict__ z, const double* __restrict__ lat,
        const double* __restrict__ lon, const double* __restrict__ cosp, double R, int* __restrict__ flow) {
    const int i = blockIdx.x * HN_T + threadIdx.x, j = blockIdx.y;
    if (i >= nlon) return;
    const size_t c = (size_t)j * nlon + i;
    if (land[c] != 1) { flow[c] = -1; return; }
    const double z0 = z[c];
    double best = -INFINITY;
    int bi = -1;
    for (int dj = -1; dj <= 1; ++dj) {
        const int jj = j + dj;
        if (jj < 0 || jj >= nlat) continue;
        const double cs = cosp[j * 3 + dj + 1];
        const double dlat = lat[jj] - lat[j];
        for (int di = -1; di <= 1; ++di) {
            if (di == 0 && dj == 0) continue;
            const int ii = (i + di + nlon) % nlon;
            double dlon = lon[ii] - lon[i];
            if (dlon > M_PI) dlon -= 2.0 * M_PI;
            else if (dlon < -M_PI) dlon += 2.0 * M_PI;
            const double x = dlon * cs;
            const double dist = R * sqrt(x * x + dlat * dlat);
            if (dist <= 0.0) continue;
            const int n = jj * nlon + ii;
            const double slope = (z0 - z[n]) / dist;
            if (slope > best) { best = slope; bi = n; }
        }
    }
    flow[c] = (best > 0.0 && bi >= 0 && land[bi] == 1) ? bi : -1;
}

// ------------------------------------------------------------------ exclusive scan of int32 (three launches)
__device__ __forceinline__ int hn_block_excl(int v, int* sh, int T, int* total) {
    const int t = threadIdx.x;
    sh[t] = v;
    __syncthreads();
    for (int o = 1; o < T; o <<= 1) {
        const int a = t >= o ? sh[t - o] : 0;
        __syncthreads();
        sh[t] += a;
        __syncthreads();
    }
    const int incl = sh[t];
    *total = sh[T - 1];
    __syncthreads();
    return incl - v;
}

__global__ void __launch_bounds__(HN_T) k_hn_scan_tile(int n, const int* __restrict__ in, int* __restrict__ out, int* __restrict__ bsum) {
    __shared__ int sh[HN_T];
    const size_t base = (size_t)blockIdx.x * HN_SCAN_TILE + (size_t)threadIdx.x * HN_SCAN_PER;
    int v[HN_SCAN_PER], s = 0;
#pragma unroll
    for (int k = 0; k < HN_SCAN_PER; ++k) { v[k] = base + k < (size_t)n ? in[base + k] : 0; s += v[k]; }
    int total;
    int x = hn_block_excl(s, sh, HN_T, &total);
#pragma unroll
    for (int k = 0; k < HN_SCAN_PER; ++k) { if (base + k < (size_t)n) out[base + k] = x; x += v[k]; }
    if (threadIdx.x == 0) bsum[blockIdx.x] = total;
}

__global__ void __launch_bounds__(HN_SCAN_TOP_T) k_hn_scan_top(int nb, int* __restrict__ bsum, int* __restrict__ tot) {
    __shared__ int sh[HN_SCAN_TOP_T];
    const int base = threadIdx.x * HN_SCAN_PER;
    int v[HN_SCAN_PER], s = 0;
#pragma unroll
    for (int k = 0; k < HN_SCAN_PER; ++k) { v[k] = base + k < nb ? bsum[base + k] : 0; s += v[k]; }
    int total;
    int x = hn_block_excl(s, sh, HN_SCAN_TOP_T, &total);
#pragma unroll
    for (int k = 0; k < HN_SCAN_PER; ++k) { if (base + k < nb) bsum[base + k] = x; x += v[k]; }
    if (threadIdx.x == 0) *tot = total;
}

__global__ void __launch_bounds__(HN_T) k_hn_scan_add(int n, int* __restrict__ out, const int* __restrict__ bsum) {
    const size_t k = (size_t)blockIdx.x * HN_T + threadIdx.x;
    if (k < (size_t)n) out[k] += bsum[k / HN_SCAN_TILE];
}

// ------------------------------------------------------------------ lakes
// label = the component's smallest cell index; labels only fall and always name a cell of the component with a label <= its
// own, so stale reads of a neighbour's label are harmless and the fixed point does not depend on scheduling
__global__ void __launch_bounds__(HN_T)
k_hn_lake_init(int cells, const uint8_t* __restrict__ land, const int* __restrict__ flow, int* __restrict__ lab) {
    const int c = blockIdx.x * HN_T + threadIdx.x;
    if (c < cells) lab[c] = (land[c] == 1 && flow[c] == -1) ? c : -1;
}

__global__ void __launch_bounds__(HN_T) k_hn_lake_prop(int nlat, int nlon, int* lab, int* __restrict__ changed) {
    const int i = blockIdx.x * HN_T + threadIdx.x, j = blockIdx.y;
    if (i >= nlon) return;
    const int c = j * nlon + i;
    const int l0 = lab[c];
    if (l0 < 0) return;
    int m = l0;
    for (int dj = -1; dj <= 1; ++dj) {
        const int jj = j + dj;
        if (jj < 0 || jj >= nlat) continue;
        for (int di = -1; di <= 1; ++di) {
            if (di == 0 && dj == 0) continue;
            const int ln = lab[jj * nlon + (i + di + nlon) % nlon];
            if (ln >= 0 && ln < m) m = ln;
        }
    }
    m = min(m, lab[m]);                          // pointer jump
    if (m < l0) { lab[c] = m; *changed = 1; }
}

__global__ void __launch_bounds__(HN_T) k_hn_lake_roots(int cells, const int* __restrict__ lab, int* __restrict__ flag) {
    const int c = blockIdx.x * HN_T + threadIdx.x;
    if (c < cells) flag[c] = lab[c] == c;
}

__global__ void __launch_bounds__(HN_T)
k_hn_lake_ids(int cells, const int* __restrict__ lab, const int* __restrict__ rank, uint8_t* __restrict__ lake_mask,
              int* __restrict__ lake_id) {
    const int c = blockIdx.x * HN_T + threadIdx.x;
    if (c >= cells) return;
    const int l = lab[c];
    lake_mask[c] = l >= 0;
    lake_id[c] = l >= 0 ? rank[l] + 1 : 0;
}

// ------------------------------------------------------------------ lake outlets
// The reference keeps, per lake, the first strict minimum of the f64 filled elevation over the non-lake land neighbours in
// (lake cell row-major, neighbour) order, and -1 when a lake cell has an ocean neighbour.  Two passes: the minimum of an
// order-preserving key of the elevation (and an ocean flag), then the minimum (cell, neighbour) ordinal among the neighbours
// at that key.  atomicMin / atomicOr give the same result in any order.
__device__ __forceinline__ unsigned long long hn_key(double z) {
    if (z == 0.0) z = 0.0;                       // -0 and +0 compare equal in the reference
    const unsigned long long u = (unsigned long long)__double_as_longlong(z);
    return (u >> 63) ? ~u : (u | 0x8000000000000000ull);
}

__global__ void __launch_bounds__(HN_T)
k_hn_outlet_key(int nlat, int nlon, const uint8_t* __restrict__ land, const uint8_t* __restrict__ lake_mask,
                const int* __restrict__ lake_id, const double* __restrict__ z, unsigned long long* __restrict__ zkey,
                int* __restrict__ ocean) {
    const int i = blockIdx.x * HN_T + threadIdx.x, j = blockIdx.y;
    if (i >= nlon) return;
    const int c = j * nlon + i;
    if (!lake_mask[c]) return;
    const int k = lake_id[c] - 1;
    unsigned long long best = ~0ull;
    bool oc = false;
    for (int dj = -1; dj <= 1; ++dj) {
        const int jj = j + dj;
        if (jj < 0 || jj >= nlat) continue;
        for (int di = -1; di <= 1; ++di) {
            if (di == 0 && dj == 0) continue;
            const int n = jj * nlon + (i + di + nlon) % nlon;
            if (lake_mask[n]) continue;
            if (land[n] == 0) { oc = true; continue; }
            best = min(best, hn_key(z[n]));
        }
    }
    if (oc) atomicOr(ocean + k, 1);
    if (best != ~0ull) atomicMin(zkey + k, best);
}

__global__ void __launch_bounds__(HN_T)
k_hn_outlet_pick(int nlat, int nlon, const uint8_t* __restrict__ land, const uint8_t* __restrict__ lake_mask,
                 const int* __restrict__ lake_id, const double* __restrict__ z, const unsigned long long* __restrict__ zkey,
                 int* __restrict__ pick) {
    const int i = blockIdx.x * HN_T + threadIdx.x, j = blockIdx.y;
    if (i >= nlon) return;
    const int c = j * nlon + i;
    if (!lake_mask[c]) return;
    const int k = lake_id[c] - 1;
    const unsigned long long want = zkey[k];
    for (int dj = -1; dj <= 1; ++dj) {
        const int jj = j + dj;
        if (jj < 0 || jj >= nlat) continue;
        for (int di = -1; di <= 1; ++di) {
            if (di == 0 && dj == 0) continue;
            const int n = jj * nlon + (i + di + nlon) % nlon;
            if (lake_mask[n] || land[n] == 0 || hn_key(z[n]) != want) continue;
            atomicMin(pick + k, c * 9 + (dj + 1) * 3 + (di + 1));   // the first candidate is this cell's first such neighbour
            return;
        }
    }
}

__global__ void __launch_bounds__(HN_T)
k_hn_outlet_final(int n_lakes, int nlat, int nlon, const int* __restrict__ ocean, const int* __restrict__ pick, int* __restrict__ out) {
    const int k = blockIdx.x * HN_T + threadIdx.x;
    if (k >= n_lakes) return;
    const int p = pick[k];
    if (ocean[k] || p == HN_NOPICK) { out[k] = -1; return; }
    const int c = p / 9, t = p % 9, j = c / nlon + t / 3 - 1, i = (c % nlon + t % 3 - 1 + nlon) % nlon;
    out[k] = j * nlon + i;
}

// ------------------------------------------------------------------ flow order
// Kahn's algorithm with a FIFO queue, one generation at a time: block 0 is the land cells of in-degree 0 in index order; block g
// is block g-1 walked in order, emitting flow_to[u] when u is the last of that cell's predecessors to be placed and the cell's
// remaining in-degree reaches 0 -- exactly the cells the FIFO queue appends while it pops block g-1.
__global__ void __launch_bounds__(HN_T)
k_hn_order_indeg(int cells, const uint8_t* __restrict__ land, const int* __restrict__ flow, int* __restrict__ rem, int* __restrict__ last) {
    const int c = blockIdx.x * HN_T + threadIdx.x;
    if (c >= cells) return;
    last[c] = -1;
    if (land[c] != 1) return;
    const int d = flow[c];
    if (d >= 0 && land[d] == 1) atomicAdd(rem + d, 1);
}

__global__ void __launch_bounds__(HN_T)
k_hn_order_flag(int cells, int mode, const uint8_t* __restrict__ land, const int* __restrict__ rem, int* __restrict__ flag) {
    const int c = blockIdx.x * HN_T + threadIdx.x;
    if (c < cells) flag[c] = land[c] == 1 && (mode == 0 ? rem[c] == 0 : rem[c] > 0);   // 0: block 0, 1: never placed
}

__global__ void __launch_bounds__(HN_T)
k_hn_order_scatter(int cells, const int* __restrict__ flag, const int* __restrict__ pos, int off, int* __restrict__ order) {
    const int c = blockIdx.x * HN_T + threadIdx.x;
    if (c < cells && flag[c]) order[off + pos[c]] = c;
}

__global__ void __launch_bounds__(HN_ORDER_T)
k_hn_order_gen(int n0, const uint8_t* __restrict__ land, const int* __restrict__ flow, int* order, int* rem, int* last,
               int* __restrict__ placed) {
    __shared__ int wsum[HN_ORDER_T / 64];
    __shared__ int s_tot;
    const int tid = threadIdx.x, lane = tid & 63, w = tid >> 6;
    int b0 = 0, b1 = n0;
    while (b1 > b0) {
        for (int p = b0 + tid; p < b1; p += HN_ORDER_T) {
            const int d = flow[hn_ldi(order + p)];
            if (d >= 0 && land[d] == 1) { atomicSub(rem + d, 1); atomicMax(last + d, p); }
        }
        asm volatile("s_waitcnt vmcnt(0)" ::: "memory");
        __syncthreads();
        int out = b1;
        for (int base = b0; base < b1; base += HN_ORDER_T) {
            const int p = base + tid;
            int d = -1;
            bool emit = false;
            if (p < b1) {
                d = flow[hn_ldi(order + p)];
                emit = d >= 0 && land[d] == 1 && hn_ldi(rem + d) == 0 && hn_ldi(last + d) == p;
            }
            const unsigned long long m = __ballot(emit);
            const int before = __popcll(m & ((1ull << lane) - 1ull));
            if (lane == 0) wsum[w] = __popcll(m);
            __syncthreads();
            if (tid == 0) {
                int acc = 0;
                for (int q = 0; q < HN_ORDER_T / 64; ++q) { const int t = wsum[q]; wsum[q] = acc; acc += t; }
                s_tot = acc;
            }
            __syncthreads();
            if (emit) order[out + wsum[w] + before] = d;
            out += s_tot;
            asm volatile("s_waitcnt vmcnt(0)" ::: "memory");
            __syncthreads();
        }
        b0 = b1;
        b1 = out;
    }
    if (tid == 0) *placed = b1;
}

// ------------------------------------------------------------------ entry points
namespace {
struct HnBuf {
    std::vector<void*> p;
    template <class T> T* get(size_t n) {
        void* q = nullptr;
        if (hipMalloc(&q, std::max<size_t>(n, 1) * sizeof(T)) != hipSuccess) return nullptr;
        p.push_back(q);
        return (T*)q;
    }
    ~HnBuf() { for (void* q : p) hipFree(q); }
};
}  // namespace

// exclusive scan of in[0..n) into out, the total to *host_total (synchronises)
static int hn_scan(qd_ctx* c, int n, const int* in, int* out, int* bsum, int* dtot, int* host_total) {
    const int nb = (n + HN_SCAN_TILE - 1) / HN_SCAN_TILE;
    hipLaunchKernelGGL(k_hn_scan_tile, dim3(nb), dim3(HN_T), 0, c->stream, n, in, out, bsum);
    hipLaunchKernelGGL(k_hn_scan_top, dim3(1), dim3(HN_SCAN_TOP_T), 0, c->stream, nb, bsum, dtot);
    hipLaunchKernelGGL(k_hn_scan_add, dim3((n + HN_T - 1) / HN_T), dim3(HN_T), 0, c->stream, n, out, (const int*)bsum);
    QD_HIP(c, hipMemcpyAsync(host_total, dtot, sizeof(int), hipMemcpyDeviceToHost, c->stream));
    QD_HIP(c, hipStreamSynchronize(c->stream));
    return 0;
}

static size_t hn_pitfill_lds(int nlat, int nlon) {
    const int nch = (nlon + HN_PF_C - 1) / HN_PF_C;
    return (size_t)4 * nlon * sizeof(double) + (size_t)nch * (sizeof(double) + sizeof(int)) + (size_t)nlon + 2 * (size_t)nlat;
}

extern "C" int qd_hydronet_build(qd_handle c, int n_lat, int n_lon, const uint8_t* land_mask, const double* elevation, double eps,
                                 int max_iters, const double* lat_rad, const double* lon_rad, const double* cos_pair, double radius,
                                 double* elevation_filled, int32_t* flow_to_index, int32_t* flow_order, uint8_t* lake_mask,
                                 int32_t* lake_id, int32_t* lake_outlet_index, int lake_outlet_cap, int* n_land_out, int* n_lakes_out) {
    if (!c) return -1;
    c->hydronet_sweeps = -1;
    if (!c->geo.full || c->desc.world > 1)
        return qd_fail(c, "qd_hydronet_build: network generation needs a whole-globe handle (world == 1, n_rows == n_lat); "
                          "latitude bands are not supported");
    if (n_lat != c->geo.nlat || n_lon != c->geo.nlon) return qd_fail(c, "qd_hydronet_build: shape is not the handle's grid");
    if (n_lat < 2 || n_lon < 3) return qd_fail(c, "qd_hydronet_build: the grid needs n_lat >= 2 and n_lon >= 3");
    const size_t cells = (size_t)n_lat * n_lon;
    if (cells > (size_t)HN_MAX_CELLS) return qd_fail(c, "qd_hydronet_build: grid too large");
    if (!land_mask || !elevation || !lat_rad || !lon_rad || !cos_pair || !elevation_filled || !flow_to_index || !flow_order ||
        !lake_mask || !lake_id || !n_land_out || !n_lakes_out || (lake_outlet_cap > 0 && !lake_outlet_index) || lake_outlet_cap < 0)
        return qd_fail(c, "qd_hydronet_build: missing array");
    if (max_iters < 0) return qd_fail(c, "qd_hydronet_build: max_iters < 0");
    // NaN comparisons make the reference depend on its visiting order: refused where a land cell reads them
    int n_land = 0;
    for (size_t k = 0; k < cells; ++k) {
        const int l = land_mask[k];
        if (l > 1) return qd_fail(c, "qd_hydronet_build: land_mask holds values other than 0 and 1");
        if (l != 1) continue;
        ++n_land;
        const int j = (int)(k / n_lon), i = (int)(k % n_lon);
        for (int dj = -1; dj <= 1; ++dj) {
            const int jj = j + dj;
            if (jj < 0 || jj >= n_lat) continue;
            for (int di = -1; di <= 1; ++di)
                if (!std::isfinite(elevation[(size_t)jj * n_lon + (i + di + n_lon) % n_lon]))
                    return qd_fail(c, "qd_hydronet_build: non-finite elevation on a land cell or next to one");
        }
    }
    // a workgroup has 160 KiB of LDS, and the kernel's static part (the scratch of __syncthreads_or's workgroup reduction)
    // comes out of it: the runtime refuses a dynamic size beyond the rest
    const size_t lds = hn_pitfill_lds(n_lat, n_lon);
    hipSetDevice(c->desc.device);
    hipFuncAttributes fa;
    QD_HIP(c, hipFuncGetAttributes(&fa, (const void*)k_hn_pitfill));
    if (lds + fa.sharedSizeBytes > 160 * 1024) return qd_fail(c, "qd_hydronet_build: n_lon too large for the pit fill's LDS rows");
    if (lds > 64 * 1024)
        QD_HIP(c, hipFuncSetAttribute((const void*)k_hn_pitfill, hipFuncAttributeMaxDynamicSharedMemorySize, (int)lds));
    const int N = (int)cells;
    HnBuf B;
    uint8_t* d_land = B.get<uint8_t>(cells);
    double* d_e = B.get<double>(cells);
    double* d_tab = B.get<double>((size_t)n_lat + n_lon + 3 * (size_t)n_lat);
    int* d_flow = B.get<int>(cells);
    int* d_a = B.get<int>(cells);       // labels, then the remaining in-degree
    int* d_b = B.get<int>(cells);       // flags
    int* d_pos = B.get<int>(cells);     // scan output
    int* d_last = B.get<int>(cells);
    int* d_order = B.get<int>(cells);
    uint8_t* d_lmask = B.get<uint8_t>(cells);
    int* d_lid = B.get<int>(cells);
    int* d_bsum = B.get<int>((size_t)HN_SCAN_TOP_T * HN_SCAN_PER);
    int* d_small = B.get<int>(4);       // sweeps, changed, scan total, placed
    if (!d_land || !d_e || !d_tab || !d_flow || !d_a || !d_b || !d_pos || !d_last || !d_order || !d_lmask || !d_lid || !d_bsum || !d_small)
        return qd_fail(c, "qd_hydronet_build: device allocation failed");
    hipStream_t s = c->stream;
    QD_HIP(c, hipMemcpyAsync(d_land, land_mask, cells, hipMemcpyHostToDevice, s));
    QD_HIP(c, hipMemcpyAsync(d_e, elevation, cells * sizeof(double), hipMemcpyHostToDevice, s));
    QD_HIP(c, hipMemcpyAsync(d_tab, lat_rad, n_lat * sizeof(double), hipMemcpyHostToDevice, s));
    QD_HIP(c, hipMemcpyAsync(d_tab + n_lat, lon_rad, n_lon * sizeof(double), hipMemcpyHostToDevice, s));
    QD_HIP(c, hipMemcpyAsync(d_tab + n_lat + n_lon, cos_pair, 3 * n_lat * sizeof(double), hipMemcpyHostToDevice, s));
    const dim3 g1((N + HN_T - 1) / HN_T), g2((n_lon + HN_T - 1) / HN_T, n_lat);

    // 1. pit fill
    hipLaunchKernelGGL(k_hn_pitfill, dim3(1), dim3(HN_PF_T), lds, s, n_lat, n_lon, (const uint8_t*)d_land, d_e, eps, max_iters, d_small);
    int h_small[4] = {0, 0, 0, 0};
    QD_HIP(c, hipMemcpyAsync(h_small, d_small, sizeof(int), hipMemcpyDeviceToHost, s));
    // 2. D8
    hipLaunchKernelGGL(k_hn_d8, g2, dim3(HN_T), 0, s, n_lat, n_lon, (const uint8_t*)d_land, (const double*)d_e, (const double*)d_tab,
                       (const double*)(d_tab + n_lat), (const double*)(d_tab + n_lat + n_lon), radius, d_flow);
    // 3. lakes
    hipLaunchKernelGGL(k_hn_lake_init, g1, dim3(HN_T), 0, s, N, (const uint8_t*)d_land, (const int*)d_flow, d_a);
    for (int it = 0;; ++it) {
        if (it > N) return qd_fail(c, "qd_hydronet_build: lake labels did not converge");
        QD_HIP(c, hipMemsetAsync(d_small + 1, 0, sizeof(int), s));
        hipLaunchKernelGGL(k_hn_lake_prop, g2, dim3(HN_T), 0, s, n_lat, n_lon, d_a, d_small + 1);
        int ch = 0;
        QD_HIP(c, hipMemcpyAsync(&ch, d_small + 1, sizeof(int), hipMemcpyDeviceToHost, s));
        QD_HIP(c, hipStreamSynchronize(s));
        if (!ch) break;
    }
    hipLaunchKernelGGL(k_hn_lake_roots, g1, dim3(HN_T), 0, s, N, (const int*)d_a, d_b);
    int n_lakes = 0;
    if (hn_scan(c, N, d_b, d_pos, d_bsum, d_small + 2, &n_lakes)) return -1;
    if (n_lakes > lake_outlet_cap) return qd_fail(c, "qd_hydronet_build: more lakes than lake_outlet_cap");
    hipLaunchKernelGGL(k_hn_lake_ids, g1, dim3(HN_T), 0, s, N, (const int*)d_a, (const int*)d_pos, d_lmask, d_lid);
    // 4. outlets (the scratch of the order stage, before it is used: zkey in d_pos / d_last, the ocean flag in d_b, pick in d_order)
    if (n_lakes > 0) {
        unsigned long long* d_zkey = (unsigned long long*)d_pos;      // n_lakes <= cells / 2: the keys fit in cells ints
        int* d_ocean = d_b; int* d_pick = d_order; int* d_out = d_last;
        if ((size_t)n_lakes * 2 > cells) return qd_fail(c, "qd_hydronet_build: lake count beyond the scratch");
        QD_HIP(c, hipMemsetAsync(d_zkey, 0xff, (size_t)n_lakes * sizeof(unsigned long long), s));
        QD_HIP(c, hipMemsetAsync(d_ocean, 0, (size_t)n_lakes * sizeof(int), s));
        QD_HIP(c, hipMemsetAsync(d_pick, 0x7f, (size_t)n_lakes * sizeof(int), s));
        hipLaunchKernelGGL(k_hn_outlet_key, g2, dim3(HN_T), 0, s, n_lat, n_lon, (const uint8_t*)d_land, (const uint8_t*)d_lmask,
                           (const int*)d_lid, (const double*)d_e, d_zkey, d_ocean);
        hipLaunchKernelGGL(k_hn_outlet_pick, g2, dim3(HN_T), 0, s, n_lat, n_lon, (const uint8_t*)d_land, (const uint8_t*)d_lmask,
                           (const int*)d_lid, (const double*)d_e, (const unsigned long long*)d_zkey, d_pick);
        hipLaunchKernelGGL(k_hn_outlet_final, dim3((n_lakes + HN_T - 1) / HN_T), dim3(HN_T), 0, s, n_lakes, n_lat, n_lon,
                           (const int*)d_ocean, (const int*)d_pick, d_out);
        QD_HIP(c, hipMemcpyAsync(lake_outlet_index, d_out, (size_t)n_lakes * sizeof(int), hipMemcpyDeviceToHost, s));
        QD_HIP(c, hipStreamSynchronize(s));
    }
    // 5. flow order
    QD_HIP(c, hipMemsetAsync(d_a, 0, cells * sizeof(int), s));
    hipLaunchKernelGGL(k_hn_order_indeg, g1, dim3(HN_T), 0, s, N, (const uint8_t*)d_land, (const int*)d_flow, d_a, d_last);
    hipLaunchKernelGGL(k_hn_order_flag, g1, dim3(HN_T), 0, s, N, 0, (const uint8_t*)d_land, (const int*)d_a, d_b);
    int n0 = 0;
    if (hn_scan(c, N, d_b, d_pos, d_bsum, d_small + 2, &n0)) return -1;
    hipLaunchKernelGGL(k_hn_order_scatter, g1, dim3(HN_T), 0, s, N, (const int*)d_b, (const int*)d_pos, 0, d_order);
    hipLaunchKernelGGL(k_hn_order_gen, dim3(1), dim3(HN_ORDER_T), 0, s, n0, (const uint8_t*)d_land, (const int*)d_flow, d_order, d_a,
                       d_last, d_small + 3);
    QD_HIP(c, hipMemcpyAsync(h_small + 3, d_small + 3, sizeof(int), hipMemcpyDeviceToHost, s));
    QD_HIP(c, hipStreamSynchronize(s));
    const int placed = h_small[3];
    if (placed < n_land) {     // the reference appends the cells Kahn never placed, in index order (none on a D8 network)
        hipLaunchKernelGGL(k_hn_order_flag, g1, dim3(HN_T), 0, s, N, 1, (const uint8_t*)d_land, (const int*)d_a, d_b);
        int nr = 0;
        if (hn_scan(c, N, d_b, d_pos, d_bsum, d_small + 2, &nr)) return -1;
        hipLaunchKernelGGL(k_hn_order_scatter, g1, dim3(HN_T), 0, s, N, (const int*)d_b, (const int*)d_pos, placed, d_order);
    }
    // results
    QD_HIP(c, hipMemcpyAsync(elevation_filled, d_e, cells * sizeof(double), hipMemcpyDeviceToHost, s));
    QD_HIP(c, hipMemcpyAsync(flow_to_index, d_flow, cells * sizeof(int), hipMemcpyDeviceToHost, s));
    QD_HIP(c, hipMemcpyAsync(flow_order, d_order, (size_t)n_land * sizeof(int), hipMemcpyDeviceToHost, s));
    QD_HIP(c, hipMemcpyAsync(lake_mask, d_lmask, cells, hipMemcpyDeviceToHost, s));
    QD_HIP(c, hipMemcpyAsync(lake_id, d_lid, cells * sizeof(int), hipMemcpyDeviceToHost, s));
    QD_HIP(c, hipStreamSynchronize(s));
    hipError_t e = hipGetLastError();
    if (e != hipSuccess) return qd_fail(c, "qd_hydronet_build: kernel", e);
    if (placed > n_land) return qd_fail(c, "qd_hydronet_build: flow order placed more cells than there is land");
    c->hydronet_sweeps = h_small[0];
    *n_land_out = n_land;
    *n_lakes_out = n_lakes;
    return 0;
}

extern "C" int qd_hydronet_sweeps(qd_handle c, int* sweeps) {
    if (!c || !sweeps) return -1;
    if (c->hydronet_sweeps < 0) return qd_fail(c, "qd_hydronet_sweeps: no network built on this handle");
    *sweeps = c->hydronet_sweeps;
    return 0;
}
