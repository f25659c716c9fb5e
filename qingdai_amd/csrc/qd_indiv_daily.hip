// qd_indiv_daily.hip -- the daily step of the sampled individuals on the resident LAI stack, gfx950: runs behind every firing of
// the daily vegetation lane (bit9) once configured.
//
// IndividualPool.step_daily (pygcm/ecology/individuals.py:193-361), called by the reference driver directly behind
// eco.step_daily with the same soil index (scripts/run_simulation.py:1818-1835).  One firing:
//   k_ind_cells    per sampled cell: E, stress days and counts per species in individual order (np.add.at is sequential and a
//                  cell's individuals are consecutive), denom = sum_s E + 1e-12, W = E / denom, the stress penalty with
//                  mean_stress = 0 where no individual, the renormalisation (:219-243) -> tables [C][S]; max_s W; the seed bank
//                  clip(bank + retain (max(0, repro) max(0, denom) / max(seed_energy, 1e-12)), 0, bank_max) at the cell (:316-335;
//                  `'soil_idx' in locals()` is false there, so no soil gate)
//   k_ind_median   one workgroup: medE = np.median(denom[denom > 0]) (the mean of the two middle order statistics; 1.0 when none),
//                  by a bitwise search on the keys with counted ranks -- exact, no sort, no atomics; beta_hint = mean_c max_s W as
//                  a blocked sum; the firing's record
//   k_ind_level    the cell loop (:259-306), the only order-dependent part.  A cell reads its own column and writes itself and the
//                  targets of `zip(jn, in_)` -- as written that is (max(0, j-1), (i-1) % W), (min(H-1, j+1), (i+1) % W) and the cell
//                  itself twice.  The host plans levels (ecology.plan_levels): cells of a level write disjoint grid cells and run
//                  in one launch, one thread per cell, levels ascending: the sequential loop bit for bit.  Kept literally: scale
//                  for total_old == 0, `new_k <= 0.0` (false for NaN), dLAI *= max(total_old, 1.0) with Python's max, the
//                  unused tot_nb (not computed).  np.sum over a contiguous run of n >= 8 takes NumPy's eight-accumulator order
//                  (qd_np_sum): np.sum(total_k) for K = 8, np.sum(mean_stress[:, ci] * wk) for S >= 8, and the strided
//                  np.sum(LAI_SK[:, :, j, i], axis=0) when K == 1 (the reduction is then the inner loop)
//   k_ind_stack    the one HBM-sized pass: clip(max(L, 0), 0, lai_max) on every plane, ECO_LAI = sum over s within a layer, then
//                  over the layers (:308-310), per-workgroup partials of nansum_land sum_k max(L, 0) per species
//   k_ind_weights  one workgroup: the partials in a fixed order -> species_weights (population.py:343-359, 1 / S when all zero)
//                  and w / (sum(w) + 1e-12) into the daily lane's germination weights
//   k_ind_reset    per individual: E_day = 0; soil >= tol: stress *= decay, else min(stress + 1, 365) (:340-356)
// f64 throughout, contraction off (Makefile), no atomics.  The only reordering against NumPy is the blocked land sum of
// k_ind_stack / k_ind_weights (NumPy's nansum is pairwise) and the blocked mean of beta_hint.
#include "qd_span.h"
#include "qd_blockred.h"
#include <algorithm>

struct QdIndivDaily {
    qd_indiv_daily_params p{};
    int C = 0, n_indiv = 0, n_levels = 0;
    int32_t* species = nullptr;       // [n_indiv]
    int32_t* order = nullptr;         // [C] sampled cells sorted by level, stable
    std::vector<int> level_start;     // [n_levels + 1] into order
    double* tabW = nullptr;           // [C][S] E -> W
    double* tabM = nullptr;           // [C][S] stress days -> mean stress
    double* tabN = nullptr;           // [C][S] counts
    double* denom = nullptr;          // [C]
    double* wmax = nullptr;           // [C] max_s W
    double* scal = nullptr;           // [2] medE, beta_hint
    double* wout = nullptr;           // [S] species_weights
    QdPartials partial;               // [S][nblk]
    int64_t n_fired = 0;
    QdSpanLane lane;                  // the log; its schedule is the daily lane's, copied at the span's begin
};

// np.sum over a run of n <= 64 doubles (qd_eco_div.hip has the same order for its pairwise total): n < 8 one after the other from
// 0, else eight interleaved partial sums combined as a tree, the n mod 8 last terms one by one
template <class F>
__device__ __forceinline__ double qd_np_sum(int n, F at) {
    if (n < 8) { double r = 0.0; for (int i = 0; i < n; ++i) r = r + at(i); return r; }
    double r[8];
#pragma unroll
    for (int q = 0; q < 8; ++q) r[q] = at(q);
    const int n8 = n & ~7;
    for (int i = 8; i < n8; i += 8)
#pragma unroll
        for (int q = 0; q < 8; ++q) r[q] = r[q] + at(i + q);
    double res = ((r[0] + r[1]) + (r[2] + r[3])) + ((r[4] + r[5]) + (r[6] + r[7]));
    for (int i = n8; i < n; ++i) res = res + at(i);
    return res;
}
// Python's max(a, b): b only when b > a (a NaN first argument stays)
__device__ __forceinline__ double qd_pymax(double a, double b) { return b > a ? b : a; }

struct QdIDArgs {
    int nlat, nlon, S, K, C, per_cell, n_indiv;
    qd_indiv_daily_params p;
    double* L; size_t plane;
    const uint8_t* land;
    const int32_t *sj, *si, *species;
    double *E, *stress; const double* tol;
    double *tabW, *tabM, *tabN, *denom, *wmax, *scal;
    double *bank, *lai; int lai_f32;
    const double *wland, *glacier; double soil_cap;
    double* partial;
    int pair_cells;                   // C == 1: np.sum(axis=0) of a [S, 1] table runs over a contiguous run
};

// ------------------------------------------------------------------ 1: per-cell tables, seed bank
__global__ void __launch_bounds__(QD_BLOCK)
k_ind_cells(QdIDArgs A) {
    const int c = blockIdx.x * QD_BLOCK + threadIdx.x;
    if (c >= A.C) return;
    const int S = A.S;
    const qd_indiv_daily_params& P = A.p;
    double* Es = A.tabW + (size_t)c * S;
    double* St = A.tabM + (size_t)c * S;
    double* Nn = A.tabN + (size_t)c * S;
    for (int s = 0; s < S; ++s) { Es[s] = 0.0; St[s] = 0.0; Nn[s] = 0.0; }
    const int n0 = c * A.per_cell;
    for (int n = n0; n < n0 + A.per_cell; ++n) {
        const int s = A.species[n];
        Es[s] = Es[s] + A.E[n];
        St[s] = St[s] + A.stress[n];
        Nn[s] = Nn[s] + 1.0;
    }
    const bool pair = A.pair_cells != 0;
    double den = pair ? qd_np_sum(S, [&](int s) { return Es[s]; }) : 0.0;
    if (!pair) for (int s = 0; s < S; ++s) den = den + Es[s];
    den = den + 1e-12;
    A.denom[c] = den;
    for (int s = 0; s < S; ++s) Es[s] = Es[s] / den;
    if (P.stress_penalty > 0.0) {
        for (int s = 0; s < S; ++s) {
            const double m = Nn[s] > 0.0 ? St[s] / Nn[s] : 0.0;
            St[s] = m;
            Es[s] = Es[s] * (1.0 / (1.0 + P.stress_penalty * m));
        }
        double d2 = pair ? qd_np_sum(S, [&](int s) { return Es[s]; }) : 0.0;
        if (!pair) for (int s = 0; s < S; ++s) d2 = d2 + Es[s];
        d2 = d2 + 1e-12;
        for (int s = 0; s < S; ++s) Es[s] = Es[s] / d2;
    } else {
        for (int s = 0; s < S; ++s) St[s] = 0.0;
    }
    double mx = Es[0];
    for (int s = 1; s < S; ++s) mx = qd_max(mx, Es[s]);                 // np.max: NaN propagates
    A.wmax[c] = mx;
    if (P.seed_couple) {
        const size_t o = (size_t)A.sj[c] * A.nlon + A.si[c];
        double seeds = (qd_max(0.0, P.repro_frac) * qd_max(0.0, den)) / qd_pymax(P.seed_energy, 1e-12);
        seeds = P.retain * seeds;
        A.bank[o] = qd_clip(A.bank[o] + seeds, 0.0, P.bank_max);
    }
}

// ------------------------------------------------------------------ 2: median of the positive denominators, beta_hint, record
__device__ __forceinline__ void id_block_count2(unsigned& a, unsigned& b, unsigned (*sm)[QD_BLOCK / 64]) {
#pragma unroll
    for (int o = 32; o > 0; o >>= 1) { a += __shfl_down(a, o, 64); b += __shfl_down(b, o, 64); }
    const int lane = threadIdx.x & 63, wv = threadIdx.x >> 6;
    __syncthreads();                                                    // the previous round's readers are done
    if (lane == 0) { sm[0][wv] = a; sm[1][wv] = b; }
    __syncthreads();
    a = 0; b = 0;
    for (int k = 0; k < QD_BLOCK / 64; ++k) { a += sm[0][k]; b += sm[1][k]; }
}

__global__ void __launch_bounds__(QD_BLOCK)
k_ind_median(int C, const double* __restrict__ denom, const double* __restrict__ wmax, double seq, int levels,
             double* __restrict__ scal, double* __restrict__ rec) {
    __shared__ unsigned sm[2][QD_BLOCK / 64];
    // positive doubles (+inf included) order as their bit patterns; NaN and values <= 0 do not take part
    unsigned n = 0, dummy = 0;
    for (int k = threadIdx.x; k < C; k += QD_BLOCK) n += denom[k] > 0.0 ? 1u : 0u;
    id_block_count2(n, dummy, sm);
    double med = 1.0;
    if (n > 0) {
        const unsigned k1 = (n - 1) / 2, k2 = n / 2;
        unsigned long long p1 = 0, p2 = 0;                              // the largest keys with count(key < p) <= k
        for (int bit = 62; bit >= 0; --bit) {                           // bit 63 is the sign: clear for every key
            const unsigned long long c1 = p1 | (1ull << bit), c2 = p2 | (1ull << bit);
            unsigned a = 0, b = 0;
            for (int k = threadIdx.x; k < C; k += QD_BLOCK) {
                const double v = denom[k];
                if (v > 0.0) {
                    const unsigned long long key = (unsigned long long)__double_as_longlong(v);
                    a += key < c1 ? 1u : 0u;
                    b += key < c2 ? 1u : 0u;
                }
            }
            id_block_count2(a, b, sm);
            if (a <= k1) p1 = c1;
            if (b <= k2) p2 = c2;
        }
        const double lo = __longlong_as_double((long long)p1), hi = __longlong_as_double((long long)p2);
        med = (k1 == k2) ? lo : (lo + hi) / 2.0;                        // np.mean of the two middle values
    }
    double t[1] = {0.0};
    for (int k = threadIdx.x; k < C; k += QD_BLOCK) t[0] += wmax[k];
    qd_block_totals(t, nullptr);
    if (threadIdx.x == 0) {
        const double beta = t[0] / (double)C;
        scal[0] = med; scal[1] = beta;
        rec[0] = seq; rec[1] = beta; rec[2] = (double)C; rec[3] = (double)levels;
    }
}

// ------------------------------------------------------------------ 3: the cell loop, one level
__global__ void __launch_bounds__(QD_BLOCK)
k_ind_level(QdIDArgs A, const int32_t* __restrict__ order, int first, int count) {
    const int t = blockIdx.x * QD_BLOCK + threadIdx.x;
    if (t >= count) return;
    const int ci = order[first + t];
    const int S = A.S, K = A.K, H = A.nlat, W = A.nlon;
    const qd_indiv_daily_params& P = A.p;
    const int j = A.sj[ci], i = A.si[ci];
    const size_t o = (size_t)j * W + i;
    const double* wk = A.tabW + (size_t)ci * S;
    const double* ms = A.tabM + (size_t)ci * S;
    double totk[QD_ECO_DAILY_MAX_K];
#pragma unroll
    for (int k = 0; k < QD_ECO_DAILY_MAX_K; ++k)
        if (k < K) {
            auto at = [&](int s) { return qd_max(A.L[(size_t)(s * K + k) * A.plane + o], 0.0); };
            if (K == 1) totk[k] = qd_np_sum(S, at);                     // [S, 1]: the reduction is the (strided) inner loop
            else { double r = 0.0; for (int s = 0; s < S; ++s) r = r + at(s); totk[k] = r; }
        }
    double total_old;
    if (K < 8) { total_old = 0.0;
#pragma unroll
        for (int k = 0; k < QD_ECO_DAILY_MAX_K; ++k) if (k < K) total_old = total_old + totk[k];
    } else total_old = ((totk[0] + totk[1]) + (totk[2] + totk[3])) + ((totk[4] + totk[5]) + (totk[6] + totk[7]));
    const double medE = A.scal[0];
    const double e_scaled = A.denom[ci] / (medE + 1e-12);
    const double msc = P.stress_penalty > 0.0 ? qd_np_sum(S, [&](int s) { return ms[s] * wk[s]; }) : 0.0;
    double dLAI = P.lai_grow * (e_scaled - 1.0) - P.lai_decay * msc;
    dLAI = dLAI * qd_pymax(total_old, 1.0);
    const double new_total = qd_clip(total_old + dLAI, 0.0, P.lai_max);
    const double scale = total_old > 0.0 ? new_total / (total_old + 1e-12) : new_total / qd_pymax(P.lai_max, 1.0);
#pragma unroll
    for (int k = 0; k < QD_ECO_DAILY_MAX_K; ++k)
        if (k < K) {
            const double new_k = totk[k] * scale;
            const bool zero = new_k <= 0.0;
            for (int s = 0; s < S; ++s) A.L[(size_t)(s * K + k) * A.plane + o] = zero ? 0.0 : wk[s] * new_k;
        }
    const double recruit = qd_pymax(0.0, new_total - total_old) * P.recruit_frac;
    if (recruit > 0.0) {
        const double share = recruit / 4.0;
        const double add = share / (double)(K > 1 ? K : 1);
        const int jm = j - 1 < 0 ? 0 : j - 1, jp = j + 1 > H - 1 ? H - 1 : j + 1;
        const int im = i - 1 < 0 ? i - 1 + W : i - 1, ip = i + 1 >= W ? i + 1 - W : i + 1;
        // zip(jn, in_) as written: jn = [j-1, j+1, j, j] against in_ = [i-1, i+1, i, i]
        const size_t nb[4] = {(size_t)jm * W + im, (size_t)jp * W + ip, o, o};
        for (int q = 0; q < 4; ++q)
            for (int k = 0; k < K; ++k)
                for (int s = 0; s < S; ++s) {
                    double* l = A.L + (size_t)(s * K + k) * A.plane + nb[q];
                    *l = qd_max(*l, 0.0) + wk[s] * add;                 // the loop works on np.maximum(stack, 0)
                }
    }
}

// ------------------------------------------------------------------ 4: the whole stack
template <int SMAX>
__global__ void __launch_bounds__(QD_BLOCK)
k_ind_stack(QdIDArgs A) {
    const int j = blockIdx.x * QD_BLOCK + threadIdx.x;
    const int S = A.S, K = A.K;
    double d[SMAX];
#pragma unroll
    for (int s = 0; s < SMAX; ++s) d[s] = 0.0;
    if (j < A.nlon) {
        const size_t o = (size_t)blockIdx.y * A.nlon + j;
        const bool land = A.land[o] == 1;
        double lay[QD_ECO_DAILY_MAX_K];
#pragma unroll
        for (int s = 0; s < SMAX; ++s)
            if (s < S) {
                double ls = 0.0;
#pragma unroll
                for (int k = 0; k < QD_ECO_DAILY_MAX_K; ++k)
                    if (k < K) {
                        double* l = A.L + (size_t)(s * K + k) * A.plane + o;
                        const double v = qd_clip(qd_max(*l, 0.0), 0.0, A.p.lai_max);
                        *l = v;
                        lay[k] = (s == 0) ? 0.0 + v : lay[k] + v;
                        ls = ls + qd_max(v, 0.0);
                    }
                d[s] = (land && ls == ls) ? ls : 0.0;                   // nansum over land
            }
        double tot = 0.0;
#pragma unroll
        for (int k = 0; k < QD_ECO_DAILY_MAX_K; ++k) if (k < K) tot = tot + lay[k];
        if (A.lai_f32) reinterpret_cast<float*>(A.lai)[o] = (float)tot; else A.lai[o] = tot;
    }
    qd_block_partials(d, S, nullptr, A.partial, (size_t)gridDim.x * gridDim.y, (size_t)blockIdx.y * gridDim.x + blockIdx.x);
}

// one workgroup: totals[s] in a fixed order, then population.py:355-359 and :571-572 with np.sum's order over [S]
__global__ void __launch_bounds__(QD_BLOCK)
k_ind_weights(const double* __restrict__ partial, int nblk, int S, double* __restrict__ wout, double* __restrict__ wnorm) {
    __shared__ double tot[QD_MAX_SPECIES];
    qd_planes_by_wave(partial, nblk, S, tot);
    if (threadIdx.x == 0) {
        const double ssum = qd_np_sum(S, [&](int s) { return tot[s]; });
        for (int s = 0; s < S; ++s) tot[s] = ssum <= 0.0 ? 1.0 / (double)S : qd_clip(tot[s] / ssum, 0.0, 1.0);
        const double wsum = qd_np_sum(S, [&](int s) { return tot[s]; }) + 1e-12;
        for (int s = 0; s < S; ++s) { wout[s] = tot[s]; wnorm[s] = tot[s] / wsum; }
    }
}

void qd_species_weights_launch(qd_ctx* c, const double* partial, int nblk, int S, double* wout, double* wnorm) {
    hipLaunchKernelGGL(k_ind_weights, dim3(1), dim3(QD_BLOCK), 0, c->stream, partial, nblk, S, wout, wnorm);
}

// ------------------------------------------------------------------ 6: the individuals' buffers
__global__ void __launch_bounds__(QD_BLOCK)
k_ind_reset(QdIDArgs A, const double* __restrict__ soil_in) {
    const int n = blockIdx.x * QD_BLOCK + threadIdx.x;
    if (n >= A.n_indiv) return;
    const int c = n / A.per_cell;
    const size_t o = (size_t)A.sj[c] * A.nlon + A.si[c];
    double soil;
    if (soil_in) soil = soil_in[o];
    else soil = qd_clip(A.wland[o] / qd_max(1e-6, A.soil_cap), 0.0, 1.0) * (A.glacier[o] != 0.0 ? 0.0 : 1.0);
    A.E[n] = 0.0;
    const double st = A.stress[n];
    A.stress[n] = soil >= A.tol[n] ? st * A.p.stress_decay : qd_min(st + 1.0, 365.0);
}

// ------------------------------------------------------------------ host side
void qd_indiv_daily_release(qd_ctx* c) {
    QdIndivDaily* d = c->idaily;
    if (!d) return;
    hipStreamSynchronize(c->stream);
    void* p[] = {d->species, d->order, d->tabW, d->tabM, d->tabN, d->denom, d->wmax, d->scal, d->wout, d->partial.p, d->lane.log};
    for (void* q : p) if (q) hipFree(q);
    delete d;
    c->idaily = nullptr;
}

// the grid cells a sampled cell writes: itself and the two targets of zip(jn, in_) that are not itself
static inline void id_footprint(int j, int i, int H, int W, size_t* f) {
    const int jm = std::max(0, j - 1), jp = std::min(H - 1, j + 1);
    f[0] = (size_t)j * W + i; f[1] = (size_t)jm * W + (i - 1 + W) % W; f[2] = (size_t)jp * W + (i + 1) % W;
}

extern "C" int qd_indiv_daily_configure(qd_handle c, const qd_indiv_daily_params* p, size_t sz, const int32_t* species_id,
                                        const int32_t* level) {
    if (!c || !p || !species_id || !level) return -1;
    if (sz != sizeof(qd_indiv_daily_params)) return qd_fail(c, "qd_indiv_daily_configure: struct size mismatch (ABI)");
    if (!qd_whole_globe(c))
        return qd_fail(c, "qd_indiv_daily_configure: the individuals' daily step needs a whole-globe handle (world == 1, n_rows == n_lat); "
                          "latitude bands are not supported");
    const QdEco& E = c->eco;
    if (E.n_indiv <= 0) return qd_fail(c, "qd_indiv_daily_configure: qd_indiv_configure has not been called");
    const double* L; int S, K;
    if (!qd_eco_daily_stack(c, &L, &S, &K)) return qd_fail(c, "qd_indiv_daily_configure: qd_eco_daily_configure has not been called");
    if (p->n_species != S || p->n_layers != K) return qd_fail(c, "qd_indiv_daily_configure: n_species / n_layers are not the stack's");
    const int C = E.n_cells, N = E.n_indiv, H = c->geo.nlat, W = c->geo.nlon;
    if (p->per_cell < 1 || (int64_t)C * p->per_cell != (int64_t)N) return qd_fail(c, "qd_indiv_daily_configure: n_cells * per_cell is not n_indiv");
    for (int n = 0; n < N; ++n)
        if (species_id[n] < 0 || species_id[n] >= S) return qd_fail(c, "qd_indiv_daily_configure: species id outside 0 .. n_species-1");
    hipSetDevice(c->desc.device);
    QD_HIP(c, hipStreamSynchronize(c->stream));
    std::vector<int32_t> sj(C), si(C), cell(N);
    QD_HIP(c, hipMemcpy(sj.data(), E.sample_j, (size_t)C * sizeof(int32_t), hipMemcpyDeviceToHost));
    QD_HIP(c, hipMemcpy(si.data(), E.sample_i, (size_t)C * sizeof(int32_t), hipMemcpyDeviceToHost));
    QD_HIP(c, hipMemcpy(cell.data(), E.cell, (size_t)N * sizeof(int32_t), hipMemcpyDeviceToHost));
    for (int n = 0; n < N; ++n)
        if (cell[n] != n / p->per_cell) return qd_fail(c, "qd_indiv_daily_configure: the individuals of a cell are not consecutive (cell index != i / per_cell)");
    // the plan: a cell's level lies above that of every earlier cell that writes one of its grid cells
    std::vector<int32_t> seen((size_t)H * W, 0);
    int n_levels = 0;
    for (int k = 0; k < C; ++k) {
        size_t f[3];
        id_footprint(sj[k], si[k], H, W, f);
        if (level[k] < 1 || level[k] > C) return qd_fail(c, "qd_indiv_daily_configure: level outside 1 .. n_cells");
        for (size_t q : f) if (level[k] <= seen[q]) return qd_fail(c, "qd_indiv_daily_configure: the level plan does not keep the order of two cells that write the same grid cell");
        for (size_t q : f) seen[q] = level[k];
        n_levels = std::max(n_levels, (int)level[k]);
    }
    std::vector<int> start(n_levels + 2, 0);
    for (int k = 0; k < C; ++k) start[level[k] + 1]++;
    for (int l = 1; l <= n_levels + 1; ++l) start[l] += start[l - 1];
    std::vector<int32_t> order(C);
    { std::vector<int> at(start.begin(), start.end()); for (int k = 0; k < C; ++k) order[at[level[k]]++] = k; }

    qd_indiv_daily_release(c);
    QdIndivDaily* d = c->idaily = new QdIndivDaily();
    d->p = *p; d->C = C; d->n_indiv = N; d->n_levels = n_levels;
    d->level_start.assign(start.begin() + 1, start.end());             // [n_levels + 1]
    d->lane.width = QD_INDIV_DAILY_LOG_W;
    d->lane.counts = true;
    const auto allocate = [&]() -> int {
        const size_t tab = (size_t)C * S * sizeof(double);
        QD_HIP(c, hipMalloc(&d->species, (size_t)N * sizeof(int32_t)));
        QD_HIP(c, hipMalloc(&d->order, (size_t)C * sizeof(int32_t)));
        QD_HIP(c, hipMalloc(&d->tabW, tab)); QD_HIP(c, hipMalloc(&d->tabM, tab)); QD_HIP(c, hipMalloc(&d->tabN, tab));
        QD_HIP(c, hipMalloc(&d->denom, (size_t)C * sizeof(double)));
        QD_HIP(c, hipMalloc(&d->wmax, (size_t)C * sizeof(double)));
        QD_HIP(c, hipMalloc(&d->scal, 2 * sizeof(double)));
        QD_HIP(c, hipMalloc(&d->wout, (size_t)S * sizeof(double)));
        QD_HIP(c, hipMemcpy(d->species, species_id, (size_t)N * sizeof(int32_t), hipMemcpyHostToDevice));
        QD_HIP(c, hipMemcpy(d->order, order.data(), (size_t)C * sizeof(int32_t), hipMemcpyHostToDevice));
        QD_HIP(c, hipMemset(d->wout, 0, (size_t)S * sizeof(double)));
        if (int rc = d->partial.ensure(c, S, ((W + QD_BLOCK - 1) / QD_BLOCK) * H)) return rc;
        QD_HIP(c, hipMalloc(&d->lane.log, d->lane.log_doubles() * sizeof(double)));
        return 0;
    };
    if (int rc = allocate()) { qd_indiv_daily_release(c); return rc; }  // never a half-built configuration
    d->lane.reset();
    return 0;
}

// soil_dev as in qd_eco_daily_step_impl
int qd_indiv_daily_step_impl(qd_ctx* c, const double* soil_dev) {
    QdIndivDaily* d = c->idaily;
    const QdEco& E = c->eco;
    const double* Lc; int S, K;
    if (!qd_eco_daily_stack(c, &Lc, &S, &K) || S != d->p.n_species || K != d->p.n_layers || E.n_indiv != d->n_indiv || E.n_cells != d->C)
        return qd_fail(c, "qd_indiv_daily: the pool or the stack changed since qd_indiv_daily_configure");
    if (d->lane.full()) return qd_fail(c, "qd_indiv_daily: log full (drain it with qd_indiv_daily_log)");
    QdScope sc(c, "indiv_daily");
    QdIDArgs A;
    A.nlat = c->geo.nlat; A.nlon = c->geo.nlon; A.S = S; A.K = K; A.C = d->C; A.per_cell = d->p.per_cell; A.n_indiv = d->n_indiv;
    A.p = d->p;
    A.L = const_cast<double*>(Lc); A.plane = c->geo.cells();
    A.land = c->land;
    A.sj = E.sample_j; A.si = E.sample_i; A.species = d->species;
    A.E = E.E_day; A.stress = E.stress; A.tol = E.tol;
    A.tabW = d->tabW; A.tabM = d->tabM; A.tabN = d->tabN; A.denom = d->denom; A.wmax = d->wmax; A.scal = d->scal;
    A.bank = c->f[QD_F_ECO_SEEDBANK]; A.lai = c->f[QD_F_ECO_LAI]; A.lai_f32 = c->eco.p.map_f32 ? 1 : 0;
    A.wland = c->f[QD_F_W_LAND]; A.glacier = c->f[QD_F_GLACIER]; A.soil_cap = qd_eco_daily_soil_cap(c);
    A.partial = d->partial.p;
    A.pair_cells = d->C == 1 ? 1 : 0;
    const dim3 block(QD_BLOCK);
    const auto flat = [](int n) { return dim3((unsigned)((n + QD_BLOCK - 1) / QD_BLOCK)); };
    hipLaunchKernelGGL(k_ind_cells, flat(A.C), block, 0, c->stream, A);
    d->n_fired += 1;
    hipLaunchKernelGGL(k_ind_median, dim3(1), block, 0, c->stream, A.C, (const double*)d->denom, (const double*)d->wmax, (double)d->n_fired,
                       d->n_levels, d->scal, d->lane.next());
    for (int l = 0; l < d->n_levels; ++l) {
        const int first = d->level_start[l], count = d->level_start[l + 1] - first;
        if (count > 0) hipLaunchKernelGGL(k_ind_level, flat(count), block, 0, c->stream, A, (const int32_t*)d->order, first, count);
    }
    const dim3 grid((A.nlon + QD_BLOCK - 1) / QD_BLOCK, A.nlat);
    if (S <= 8) hipLaunchKernelGGL(k_ind_stack<8>, grid, block, 0, c->stream, A);
    else if (S <= 24) hipLaunchKernelGGL(k_ind_stack<24>, grid, block, 0, c->stream, A);
    else hipLaunchKernelGGL(k_ind_stack<QD_MAX_SPECIES>, grid, block, 0, c->stream, A);
    qd_species_weights_launch(c, d->partial.p, (int)(grid.x * grid.y), S, d->wout, qd_eco_daily_weights_dev(c));
    hipLaunchKernelGGL(k_ind_reset, flat(A.n_indiv), block, 0, c->stream, A, soil_dev);
    // the canopy state qd_eco_daily_step_impl leaves: new layers, snapshot and recompute clock untouched
    c->eco.have_lai = 1; c->eco.lai_version++;
    qd_mark(c, {c->f[QD_F_ECO_LAI], c->f[QD_F_ECO_SEEDBANK]}, 0);
    return 0;
}

extern "C" int qd_indiv_daily_step(qd_handle c, const double* soil_index) {
    if (!c) return -1;
    if (!qd_whole_globe(c)) return qd_fail(c, "qd_indiv_daily_step: the individuals' daily step needs a whole-globe handle; latitude bands are not supported");
    if (!c->idaily) return qd_fail(c, "qd_indiv_daily_step: qd_indiv_daily_configure has not been called");
    hipSetDevice(c->desc.device);
    double* stage = qd_eco_daily_share_plane(c);                        // free between two vegetation steps: stage the host map there
    if (soil_index) {
        if (!stage) return qd_fail(c, "qd_indiv_daily_step: qd_eco_daily_configure has not been called");
        QD_HIP(c, hipMemcpyAsync(stage, soil_index, c->geo.cells() * sizeof(double), hipMemcpyHostToDevice, c->stream));
        QD_HIP(c, hipStreamSynchronize(c->stream));                     // the host buffer is only borrowed for the call
    }
    if (int rc = qd_indiv_daily_step_impl(c, soil_index ? stage : nullptr)) return rc;
    return qd_launch_check(c, "qd_indiv_daily_step");
}

static QdSpanLane* id_lane(qd_ctx* c) { return c && c->idaily ? &c->idaily->lane : nullptr; }

// qd_step_n, before work: the individuals fire with the daily lane, so its schedule is theirs -> the lane (for the span guard),
// or nullptr with the error set when the span's firings would overflow the log
QdSpanLane* qd_indiv_daily_span_begin(qd_ctx* c, const QdSpanLane* daily) {
    QdSpanLane* l = id_lane(c);
    l->sched = daily->sched;
    if (!l->fits()) {
        l->clear_schedule();
        qd_fail(c, "qd_step_n: the span's daily steps of the individuals would overflow their log (drain it with qd_indiv_daily_log)");
        return nullptr;
    }
    return l;
}

extern "C" int qd_indiv_daily_log(qd_handle c, double* out, int max, int* n) {
    return qd_lane_drain(c, id_lane(c), out, max, n, "qd_indiv_daily_log", "qd_indiv_daily_configure has not been called");
}

extern "C" int qd_indiv_daily_weights(qd_handle c, double* w, int n_species) {
    if (!c || !w) return -1;
    QdIndivDaily* d = c->idaily;
    if (!d) return qd_fail(c, "qd_indiv_daily_weights: qd_indiv_daily_configure has not been called");
    if (n_species != d->p.n_species) return qd_fail(c, "qd_indiv_daily_weights: n_species is not the configured one");
    if (d->n_fired == 0) return qd_fail(c, "qd_indiv_daily_weights: no firing yet");
    hipSetDevice(c->desc.device);
    QD_HIP(c, hipMemcpyAsync(w, d->wout, (size_t)n_species * sizeof(double), hipMemcpyDeviceToHost, c->stream));
    QD_HIP(c, hipStreamSynchronize(c->stream));
    return 0;
}

int64_t qd_indiv_daily_fired(qd_ctx* c, int64_t set) {
    if (!c->idaily) return 0;
    if (set >= 0) c->idaily->n_fired = set;
    return c->idaily->n_fired;
}

extern "C" int qd_indiv_daily_state(qd_handle c, int64_t* n_firings) {
    if (!c || !n_firings) return -1;
    *n_firings = c->idaily ? c->idaily->n_fired : 0;
    return 0;
}
