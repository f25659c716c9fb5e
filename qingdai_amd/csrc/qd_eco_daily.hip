// qd_eco_daily.hip -- the daily vegetation step on the resident LAI stack, gfx950: the third span lane (bit9).
//
// PopulationManager.step_daily (pygcm/ecology/population.py:389-596), called by the reference driver at every planet-day boundary
// with soil = clip(W_land / max(1e-6, cap), 0, 1) * !glacier (scripts/run_simulation.py:1786-1810).  One firing, per cell:
//   front    growth = growth_per_j (1 - repro) nan_to_num(E_day), sen = senesce gain max(0, thresh - clip(soil)), both 0 off land;
//            gate = clip(soil)^exp on land (or the land mask); K > 1: top-down capture cap_k, growth by cap_k / cap_sum and the LAI
//            share within the layer (equal split where cap_sum <= 0), senescence by the share of the total, clip to [0, lai_max],
//            species-wise upward transfer k = K-1 .. 1.  K == 1: the layers do not change (the reference updates only an aggregate
//            that its later refresh overwrites from the layers).
//   spread   species after species (s sees what 0..s-1 left): k_ecod_share writes the per-neighbour share of every source cell from
//            its own pre-update values (diffusion: rate LAI_s gate / n_land_neighbours; seed: r_eff Seeds / n_land_neighbours, and the
//            retained seeds into the bank), k_ecod_apply gathers the 4 / 8 neighbours' shares in the reference's offset order and
//            updates its own cell (population.py:663-700, 736-827).  np.roll wraps both axes: row 0 and row n_lat-1 are neighbours.
//   finish   age += 1 where total LAI > 0 on land, germination into layer 0 by species weight, seed-bank decay, ECO_LAI = sum of
//            the planes (s outer, k inner: np.sum(axis=(0,1))), E_day = 0, per-block {sum, count, min, max} of the land LAI;
//            k_ecod_final reduces them in a fixed order into the lane's record {firings, LAI_min, LAI_mean, LAI_max}.
// All pointwise or 5 / 9-point, row-major coalesced, HBM-bound; f64 throughout, contraction off (Makefile), no atomics.
#include "qd_span.h"
#include "qd_blockred.h"
#include <algorithm>

struct QdEcoDaily {
    qd_eco_daily_params p{};
    std::vector<int32_t> mode;        // [S] 0 diffusion, 1 seed
    double* w = nullptr;              // [S] normalised species weights
    double* L = nullptr;              // [S * K][cells] LAI_layers_SK
    int planes = 0;
    double* share = nullptr;          // [cells] per-neighbour share of the species being spread (and the staged soil index of a seam call)
    QdPartials partial;               // [4][nblk]: sum, count, min, max of the land LAI
    int64_t n_fired = 0;
    QdSpanLane lane;                  // qd_eco_daily_schedule: firings per step of the next span; the summary log
};

struct QdEDArgs {
    int nlat, nlon;
    qd_eco_daily_params p;
    double* L; size_t plane;
    const uint8_t* land;
    const double* w;
    double* eday; double* age; double* bank; double* gate; double* share; double* lai;
    const double* wland; const double* glacier;
    double* partial;
    int lai_f32;
};

__constant__ const QdRedOp qd_ed_ops[4] = {QD_RED_SUM, QD_RED_SUM, QD_RED_MIN, QD_RED_MAX};

// ------------------------------------------------------------------ front: soil, gate, growth / senescence into the layers
__global__ void __launch_bounds__(QD_BLOCK)
k_ecod_front(QdEDArgs A, const double* __restrict__ soil_in) {
    const int j = blockIdx.x * QD_BLOCK + threadIdx.x;
    if (j >= A.nlon) return;
    const size_t o = (size_t)blockIdx.y * A.nlon + j;
    const qd_eco_daily_params& P = A.p;
    const bool land = A.land[o] == 1;
    double soil;
    if (soil_in) soil = soil_in[o];
    else soil = qd_clip(A.wland[o] / qd_max(1e-6, P.soil_cap), 0.0, 1.0) * (A.glacier[o] != 0.0 ? 0.0 : 1.0);
    const double sc = qd_clip(soil, 0.0, 1.0);
    const double E = qd_nn(A.eday[o]);
    const double growth = land ? P.growth_per_j * ((1.0 - P.repro_frac) * E) : 0.0;
    const double sen = land ? (P.senesce_per_day * P.stress_strength) * qd_max(0.0, P.stress_thresh - sc) : 0.0;
    A.gate[o] = land ? (P.gate_soil ? qd_pow_np(sc, P.soil_exp) : 1.0) : 0.0;
    const int S = P.n_species, K = P.n_layers;
    if (K <= 1) return;                                        // population.py:499-501: only the aggregate moves, and it is overwritten

    // 1) totals per layer (species summed in index order) and of the column (s outer, k inner)
    double totk[QD_ECO_DAILY_MAX_K];
    double tot = 0.0;
    for (int s = 0; s < S; ++s)
#pragma unroll
        for (int k = 0; k < QD_ECO_DAILY_MAX_K; ++k)
            if (k < K) {
                const double v = qd_max(A.L[(size_t)(s * K + k) * A.plane + o], 0.0);
                totk[k] = (s == 0) ? v : totk[k] + v;
                tot = (s == 0 && k == 0) ? v : tot + v;
            }
    // 2) top-down Beer-Lambert capture
    double capk[QD_ECO_DAILY_MAX_K];
    double I_in = E, cap_sum = 0.0;
#pragma unroll
    for (int k = 0; k < QD_ECO_DAILY_MAX_K; ++k)
        if (k < K) {
            const double T = exp(-P.k_canopy * totk[k]);
            capk[k] = I_in * (1.0 - T);
            I_in = I_in * T;
            cap_sum = (k == 0) ? capk[0] : cap_sum + capk[k];
        }
    const bool no_cap = cap_sum <= 0.0;
    const double eq = (growth / (double)K) / (double)S;
    const double inv_s = 1.0 / (double)S, inv_sk = 1.0 / (double)(S * K);
    // 3) growth and senescence shares, clip, upward transfer, species by species
    for (int s = 0; s < S; ++s) {
        double l[QD_ECO_DAILY_MAX_K];
#pragma unroll
        for (int k = 0; k < QD_ECO_DAILY_MAX_K; ++k)
            if (k < K) {
                const double v = qd_max(A.L[(size_t)(s * K + k) * A.plane + o], 0.0);
                const double wsk = totk[k] > 0.0 ? v / (totk[k] + 1e-12) : inv_s;
                const double g = no_cap ? eq : (wsk * (capk[k] / (cap_sum + 1e-12))) * growth;
                const double ws = tot > 0.0 ? v / (tot + 1e-12) : inv_sk;
                l[k] = qd_clip((v + g) - ws * sen, 0.0, P.lai_max);
            }
        if (P.upfrac > 0.0) {
#pragma unroll
            for (int k = QD_ECO_DAILY_MAX_K - 1; k >= 1; --k)
                if (k < K) {
                    const double d = P.upfrac * qd_max(0.0, l[k] - l[k - 1]);
                    l[k] = l[k] - d;
                    l[k - 1] = l[k - 1] + d;
                }
        }
#pragma unroll
        for (int k = 0; k < QD_ECO_DAILY_MAX_K; ++k)
            if (k < K) A.L[(size_t)(s * K + k) * A.plane + o] = l[k];
    }
}

// ------------------------------------------------------------------ spread
__device__ __forceinline__ int qd_ed_up(int i, int n) { return i + 1 >= n ? i + 1 - n : i + 1; }
__device__ __forceinline__ int qd_ed_dn(int i, int n) { return i - 1 < 0 ? i - 1 + n : i - 1; }

// the neighbours of (i, j) in the reference's offset order, as sources of np.roll(x, shift=(dy, dx)): x[i - dy][j - dx]
//   von Neumann (-1,0) (0,-1) (0,1) (1,0);  Moore (-1,-1) (-1,0) (-1,1) (0,-1) (0,1) (1,-1) (1,0) (1,1)
__device__ __forceinline__ int qd_ed_neigh(int moore, int i, int j, int nlat, int nlon, size_t* idx) {
    const size_t rp = (size_t)qd_ed_up(i, nlat) * nlon, r0 = (size_t)i * nlon, rm = (size_t)qd_ed_dn(i, nlat) * nlon;
    const int jp = qd_ed_up(j, nlon), jm = qd_ed_dn(j, nlon);
    if (!moore) { idx[0] = rp + j; idx[1] = r0 + jp; idx[2] = r0 + jm; idx[3] = rm + j; return 4; }
    idx[0] = rp + jp; idx[1] = rp + j; idx[2] = rp + jm; idx[3] = r0 + jp; idx[4] = r0 + jm; idx[5] = rm + jp; idx[6] = rm + j; idx[7] = rm + jm;
    return 8;
}

// what one source cell hands to EACH of its neighbours, from its own values before species s is updated
__global__ void __launch_bounds__(QD_BLOCK)
k_ecod_share(QdEDArgs A, int s, int seed) {
    const int j = blockIdx.x * QD_BLOCK + threadIdx.x;
    if (j >= A.nlon) return;
    const int i = blockIdx.y;
    const size_t o = (size_t)i * A.nlon + j;
    const qd_eco_daily_params& P = A.p;
    const int S = P.n_species, K = P.n_layers;
    const bool land = A.land[o] == 1;
    size_t nb[8];
    const int nn = qd_ed_neigh(P.moore, i, j, A.nlat, A.nlon, nb);
    double nv = 0.0;                                           // land cells among the neighbours (the count is symmetric in the offsets)
    for (int q = 0; q < nn; ++q) nv += (A.land[nb[q]] == 1) ? 1.0 : 0.0;
    const double g = land ? qd_clip(A.gate[o], 0.0, 1.0) : 0.0;
    double share;
    if (!seed) {
        double Ls = 0.0;
        for (int k = 0; k < K; ++k) { const double v = A.L[(size_t)(s * K + k) * A.plane + o]; Ls = (k == 0) ? v : Ls + v; }
        Ls = qd_max(Ls, 0.0);
        const double out = (P.spread_rate * Ls) * g;
        share = nv > 0.0 ? out / (nv + 1e-12) : 0.0;
    } else {
        double Ls = 0.0, tot = 0.0;
        for (int t = 0; t < S; ++t)
            for (int k = 0; k < K; ++k) {
                const double v = A.L[(size_t)(t * K + k) * A.plane + o];
                tot = (t == 0 && k == 0) ? v : tot + v;
                if (t == s) Ls = (k == 0) ? v : Ls + v;
            }
        Ls = qd_max(Ls, 0.0); tot = qd_max(tot, 0.0);
        const double sh = tot > 0.0 ? Ls / (tot + 1e-12) : 0.0;
        const double Er = (P.repro_frac * qd_nn(A.eday[o])) * sh;
        const double seeds = qd_max(Er / P.seed_energy, 0.0) * (land ? 1.0 : 0.0);
        double r = P.spread_rate * (1.0 - exp(-seeds / P.seed_scale));
        A.bank[o] = qd_clip(A.bank[o] + P.retain * seeds, 0.0, P.bank_max);
        r = r * g;
        share = nv > 0.0 ? (r * seeds) / (nv + 1e-12) : 0.0;
    }
    A.share[o] = share;
}

__global__ void __launch_bounds__(QD_BLOCK)
k_ecod_apply(QdEDArgs A, int s, int seed) {
    const int j = blockIdx.x * QD_BLOCK + threadIdx.x;
    if (j >= A.nlon) return;
    const int i = blockIdx.y;
    const size_t o = (size_t)i * A.nlon + j;
    const qd_eco_daily_params& P = A.p;
    const int K = P.n_layers;
    const bool land = A.land[o] == 1;
    size_t nb[8];
    const int nn = qd_ed_neigh(P.moore, i, j, A.nlat, A.nlon, nb);
    if (seed) {
        const double sl = qd_max(0.0, P.seedling_lai);
        double add = 0.0;
        for (int q = 0; q < nn; ++q) add += sl * A.share[nb[q]];
        add = qd_min(add, P.seed_dlai_max);
        if (add > 0.0 && land) {
            double* l0 = A.L + (size_t)(s * K) * A.plane + o;
            *l0 = qd_clip(*l0 + add, 0.0, P.lai_max);
            A.age[o] = 0.0;
        }
        return;
    }
    double inflow = 0.0;
    for (int q = 0; q < nn; ++q) inflow += A.share[nb[q]];
    double prev = 0.0;
    for (int k = 0; k < K; ++k) { const double v = A.L[(size_t)(s * K + k) * A.plane + o]; prev = (k == 0) ? v : prev + v; }
    prev = qd_max(prev, 0.0);
    const double g = land ? qd_clip(A.gate[o], 0.0, 1.0) : 0.0;
    const double out = (P.spread_rate * prev) * g;
    const double raw = (prev - out) + inflow;
    const double inc = raw - prev;
    const double capped = (prev + qd_min(qd_max(inc, 0.0), P.dlai_max)) + qd_min(inc, 0.0);
    const double nw = land ? qd_clip(capped, 0.0, P.lai_max) : 0.0;
    const double fac = prev > 0.0 ? nw / (prev + 1e-12) : 0.0;
    for (int k = 0; k < K; ++k) {
        double* l = A.L + (size_t)(s * K + k) * A.plane + o;
        *l = qd_clip(*l * fac, 0.0, P.lai_max);
    }
}

// ------------------------------------------------------------------ finish: age, germination, bank decay, ECO_LAI, E_day, partials
__global__ void __launch_bounds__(QD_BLOCK)
k_ecod_finish(QdEDArgs A) {
    const int j = blockIdx.x * QD_BLOCK + threadIdx.x;
    double d[4] = {0.0, 0.0, INFINITY, -INFINITY};             // sum, count, min, max
    if (j < A.nlon) {
        const size_t o = (size_t)blockIdx.y * A.nlon + j;
        const qd_eco_daily_params& P = A.p;
        const int S = P.n_species, K = P.n_layers;
        const bool land = A.land[o] == 1;
        const double g = land ? qd_clip(A.gate[o], 0.0, 1.0) : 0.0;
        const double bank = A.bank[o];
        const double germ = (qd_max(0.0, P.germ_frac) * bank) * g;
        const double add_total = P.seedling_lai * germ;
        double pre = 0.0, post = 0.0;
        for (int s = 0; s < S; ++s)
            for (int k = 0; k < K; ++k) {
                double* l = A.L + (size_t)(s * K + k) * A.plane + o;
                double v = *l;
                pre = (s == 0 && k == 0) ? v : pre + v;
                if (k == 0 && land) { v = qd_clip(v + A.w[s] * add_total, 0.0, P.lai_max); *l = v; }
                post = (s == 0 && k == 0) ? v : post + v;
            }
        if (land && qd_max(pre, 0.0) > 0.0) A.age[o] = A.age[o] + 1.0;
        A.bank[o] = qd_max(0.0, bank - germ) * qd_max(0.0, 1.0 - P.bank_decay);
        if (A.lai_f32) reinterpret_cast<float*>(A.lai)[o] = (float)post; else A.lai[o] = post;
        A.eday[o] = 0.0;
        if (land) { d[0] = post; d[1] = 1.0; d[2] = post; d[3] = post; }
    }
    qd_block_partials(d, 4, qd_ed_ops, A.partial, (size_t)gridDim.x * gridDim.y, (size_t)blockIdx.y * gridDim.x + blockIdx.x);
}

// one workgroup: the block partials in a fixed order -> {firings, LAI_min, LAI_mean, LAI_max} (zeros without land)
__global__ void __launch_bounds__(QD_BLOCK)
k_ecod_final(const double* __restrict__ partial, int nblk, double seq, double* __restrict__ rec) {
    double t[4];
    qd_planes_strided(partial, nblk, 4, qd_ed_ops, t);
    qd_block_totals(t, qd_ed_ops);
    if (threadIdx.x == 0) {
        const double a = t[0], n = t[1], lo = t[2], hi = t[3];
        rec[0] = seq;
        rec[1] = n > 0.0 ? lo : 0.0; rec[2] = n > 0.0 ? a / n : 0.0; rec[3] = n > 0.0 ? hi : 0.0;
    }
}

// ------------------------------------------------------------------ host side
void qd_eco_daily_release(qd_ctx* c) {
    QdEcoDaily* d = c->edaily;
    if (!d) return;
    void* p[] = {d->w, d->L, d->share, d->partial.p, d->lane.log};
    for (void* q : p) if (q) hipFree(q);
    delete d;
    c->edaily = nullptr;
}

bool qd_eco_daily_stack(const qd_ctx* c, const double** L, int* n_species, int* n_layers) {
    const QdEcoDaily* d = c->edaily;
    if (!d || !d->L) return false;
    *L = d->L; *n_species = d->p.n_species; *n_layers = d->p.n_layers;
    return true;
}

double* qd_eco_daily_share_plane(qd_ctx* c) { return c->edaily ? c->edaily->share : nullptr; }
double* qd_eco_daily_weights_dev(qd_ctx* c) { return c->edaily ? c->edaily->w : nullptr; }
double qd_eco_daily_soil_cap(const qd_ctx* c) { return c->edaily ? c->edaily->p.soil_cap : 50.0; }
double qd_eco_daily_lai_max(const qd_ctx* c) { return c->edaily ? c->edaily->p.lai_max : 5.0; }

// qd_eco_speciate.hip: the stack grown by one species.  Takes L1 [(S + 1) * K][cells] and w1 [S + 1] and frees the old ones (the
// caller has synchronised the stream).  The new index gets the mode population.py:511 gives an index the mode list does not hold
// (the reference never extends species_modes).  Age, seed bank, E_day, gate, firing count, log and schedule stay.
void qd_eco_daily_adopt(qd_ctx* c, double* L1, double* w1) {
    QdEcoDaily* d = c->edaily;
    hipFree(d->L); hipFree(d->w);
    d->L = L1; d->w = w1;
    d->mode.push_back(d->p.n_species == 1 ? 1 : 0);
    d->p.n_species += 1;
    d->planes = d->p.n_species * d->p.n_layers;
}

extern "C" int qd_eco_daily_configure(qd_handle c, const qd_eco_daily_params* p, size_t sz, const int32_t* mode, const double* w) {
    if (!c || !p || !mode || !w) return -1;
    if (sz != sizeof(qd_eco_daily_params)) return qd_fail(c, "qd_eco_daily_configure: struct size mismatch (ABI)");
    if (!qd_whole_globe(c))
        return qd_fail(c, "qd_eco_daily_configure: the daily vegetation step needs a whole-globe handle (world == 1, n_rows == n_lat); "
                          "latitude bands are not supported");
    const int S = p->n_species, K = p->n_layers;
    if (S < 1 || S > QD_MAX_SPECIES) return qd_fail(c, "qd_eco_daily_configure: n_species out of range (1..64)");
    if (K < 1 || K > QD_ECO_DAILY_MAX_K) return qd_fail(c, "qd_eco_daily_configure: n_layers out of range (1..8)");
    for (int s = 0; s < S; ++s) if (mode[s] != 0 && mode[s] != 1) return qd_fail(c, "qd_eco_daily_configure: species_mode is 0 (diffusion) or 1 (seed)");
    hipSetDevice(c->desc.device);
    qd_indiv_daily_release(c);                                  // its tables and weights belong to the stack configured before
    QdEcoDaily* d = c->edaily;
    if (!d) d = c->edaily = new QdEcoDaily();
    QD_HIP(c, hipStreamSynchronize(c->stream));
    const size_t cells = c->geo.cells();
    if (d->planes != S * K) {
        if (d->L) { hipFree(d->L); d->L = nullptr; }
        d->planes = 0;
        QD_HIP(c, hipMalloc(&d->L, (size_t)S * K * cells * sizeof(double)));
        QD_HIP(c, hipMemsetAsync(d->L, 0, (size_t)S * K * cells * sizeof(double), c->stream));
        d->planes = S * K;
    }
    if (d->w) { hipFree(d->w); d->w = nullptr; }
    QD_HIP(c, hipMalloc(&d->w, (size_t)S * sizeof(double)));
    QD_HIP(c, hipMemcpy(d->w, w, (size_t)S * sizeof(double), hipMemcpyHostToDevice));
    if (!d->share) QD_HIP(c, hipMalloc(&d->share, cells * sizeof(double)));
    if (int rc = d->partial.ensure(c, 4, ((c->geo.nlon + QD_BLOCK - 1) / QD_BLOCK) * c->geo.nrows)) return rc;
    d->lane.width = QD_ECO_DAILY_LOG_W;
    d->lane.counts = true;                                      // a step may fire more than once (dt > day)
    if (!d->lane.log) QD_HIP(c, hipMalloc(&d->lane.log, d->lane.log_doubles() * sizeof(double)));
    d->lane.reset();
    QD_HIP(c, hipMemsetAsync(c->f[QD_F_ECO_AGE], 0, cells * sizeof(double), c->stream));
    QD_HIP(c, hipMemsetAsync(c->f[QD_F_ECO_SEEDBANK], 0, cells * sizeof(double), c->stream));
    d->mode.assign(mode, mode + S);
    d->p = *p;
    d->n_fired = 0;
    QD_HIP(c, hipStreamSynchronize(c->stream));
    return 0;
}

static int ed_layers_check(qd_ctx* c, const char* who, const void* host, int n_planes) {
    if (!c || !host) return -1;
    if (!c->edaily) return qd_fail(c, (std::string(who) + ": qd_eco_daily_configure has not been called").c_str());
    if (n_planes != c->edaily->planes) return qd_fail(c, (std::string(who) + ": plane count is not n_species * n_layers").c_str());
    hipSetDevice(c->desc.device);
    return 0;
}
extern "C" int qd_eco_daily_set_layers(qd_handle c, const double* layers, int n_planes) {
    if (int rc = ed_layers_check(c, "qd_eco_daily_set_layers", layers, n_planes)) return rc;
    QD_HIP(c, hipMemcpyAsync(c->edaily->L, layers, (size_t)n_planes * c->geo.cells() * sizeof(double), hipMemcpyHostToDevice, c->stream));
    QD_HIP(c, hipStreamSynchronize(c->stream));
    return 0;
}
extern "C" int qd_eco_daily_get_layers(qd_handle c, double* layers, int n_planes) {
    if (int rc = ed_layers_check(c, "qd_eco_daily_get_layers", layers, n_planes)) return rc;
    QD_HIP(c, hipMemcpyAsync(layers, c->edaily->L, (size_t)n_planes * c->geo.cells() * sizeof(double), hipMemcpyDeviceToHost, c->stream));
    QD_HIP(c, hipStreamSynchronize(c->stream));
    const hipError_t e = hipGetLastError();
    if (e != hipSuccess) return qd_fail(c, "qd_eco_daily_get_layers: kernel", e);
    return 0;
}

// soil_dev: a device [cells] soil index, or nullptr = from W_LAND and GLACIER
int qd_eco_daily_step_impl(qd_ctx* c, const double* soil_dev) {
    QdEcoDaily* d = c->edaily;
    if (d->lane.full()) return qd_fail(c, "qd_eco_daily: summary log full (drain it with qd_eco_daily_log)");
    QdScope sc(c, "eco_daily");
    QdEDArgs A;
    A.nlat = c->geo.nlat; A.nlon = c->geo.nlon;
    A.p = d->p;
    A.L = d->L; A.plane = c->geo.cells();
    A.land = c->land; A.w = d->w;
    A.eday = c->f[QD_F_ECO_EDAY]; A.age = c->f[QD_F_ECO_AGE]; A.bank = c->f[QD_F_ECO_SEEDBANK]; A.gate = c->f[QD_F_ECO_GATE];
    A.share = d->share; A.lai = c->f[QD_F_ECO_LAI];
    A.wland = c->f[QD_F_W_LAND]; A.glacier = c->f[QD_F_GLACIER];
    A.partial = d->partial.p;
    A.lai_f32 = c->eco.p.map_f32 ? 1 : 0;
    const dim3 grid((A.nlon + QD_BLOCK - 1) / QD_BLOCK, A.nlat), block(QD_BLOCK);
    hipLaunchKernelGGL(k_ecod_front, grid, block, 0, c->stream, A, soil_dev);
    if (d->p.spread && d->p.spread_rate > 0.0)
        for (int s = 0; s < d->p.n_species; ++s) {
            hipLaunchKernelGGL(k_ecod_share, grid, block, 0, c->stream, A, s, (int)d->mode[s]);
            hipLaunchKernelGGL(k_ecod_apply, grid, block, 0, c->stream, A, s, (int)d->mode[s]);
        }
    hipLaunchKernelGGL(k_ecod_finish, grid, block, 0, c->stream, A);
    d->n_fired += 1;
    hipLaunchKernelGGL(k_ecod_final, dim3(1), block, 0, c->stream, d->partial.p, (int)(grid.x * grid.y), (double)d->n_fired, d->lane.next());
    // the canopy state of qd_eco_set_lai_layers(h, layers, n, 0): new layers, snapshot and recompute clock untouched
    c->eco.have_lai = 1; c->eco.lai_version++;
    qd_mark(c, {c->f[QD_F_ECO_LAI], c->f[QD_F_ECO_EDAY], c->f[QD_F_ECO_AGE], c->f[QD_F_ECO_SEEDBANK], c->f[QD_F_ECO_GATE]}, 0);
    return 0;
}

extern "C" int qd_eco_daily_step(qd_handle c, const double* soil_index) {
    if (!c) return -1;
    if (!qd_whole_globe(c)) return qd_fail(c, "qd_eco_daily_step: the daily vegetation step needs a whole-globe handle; latitude bands are not supported");
    QdEcoDaily* d = c->edaily;
    if (!d) return qd_fail(c, "qd_eco_daily_step: qd_eco_daily_configure has not been called");
    hipSetDevice(c->desc.device);
    if (soil_index) {                                           // the share plane is free until the spread: stage the host map there
        QD_HIP(c, hipMemcpyAsync(d->share, soil_index, c->geo.cells() * sizeof(double), hipMemcpyHostToDevice, c->stream));
        QD_HIP(c, hipStreamSynchronize(c->stream));             // the host buffer is only borrowed for the call
    }
    if (int rc = qd_eco_daily_step_impl(c, soil_index ? d->share : nullptr)) return rc;
    return qd_launch_check(c, "qd_eco_daily_step");
}

static QdSpanLane* ed_lane(qd_ctx* c) { return c && c->edaily ? &c->edaily->lane : nullptr; }
static const char* const ED_MISSING = "qd_eco_daily_configure has not been called";

extern "C" int qd_eco_daily_schedule(qd_handle c, int n, const int32_t* fire) {
    return qd_lane_schedule(c, ed_lane(c), n, fire, "qd_eco_daily_schedule", ED_MISSING);
}

QdSpanLane* qd_eco_daily_span_begin(qd_ctx* c, int n, int with_eco) {
    static const QdSpanTexts T = {
        "qd_step_n: the daily vegetation step (bit9) needs a whole-globe handle; latitude bands are not supported",
        "qd_step_n: bit9 set but qd_eco_daily_configure has not been called",
        "qd_step_n: bit9 needs a qd_eco_daily_schedule of exactly n steps before the span",
        "qd_step_n: the span's daily vegetation steps would overflow the summary log (drain it first)"};
    return qd_lane_span_begin(c, ed_lane(c), n, T,
                              with_eco ? nullptr : "qd_step_n: the daily vegetation step (bit9) needs the ecology sub-step (bit5)");
}

extern "C" int qd_eco_daily_log(qd_handle c, double* out, int max, int* n) {
    return qd_lane_drain(c, ed_lane(c), out, max, n, "qd_eco_daily_log", ED_MISSING);
}

int64_t qd_eco_daily_fired(qd_ctx* c, int64_t set) {
    if (!c->edaily) return 0;
    if (set >= 0) c->edaily->n_fired = set;
    return c->edaily->n_fired;
}

extern "C" int qd_eco_daily_state(qd_handle c, int64_t* n_firings) {
    if (!c || !n_firings) return -1;
    *n_firings = c->edaily ? c->edaily->n_fired : 0;
    return 0;
}
