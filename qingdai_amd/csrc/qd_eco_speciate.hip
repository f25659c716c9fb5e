// qd_eco_speciate.hip -- one speciation event on the resident LAI stack of the daily vegetation lane, gfx950.
//
// PopulationManager.add_species_from_parent (pygcm/ecology/population.py:361-387), called by EcologyAdapter.step_daily on a hit of
// its mutation draw (adapter.py:437-466).  The stack grows from [S][K] to [S + 1][K] planes:
//   k_spec_split   the one HBM-sized pass, old stack -> new stack: transfer = f x_p (one multiply), parent plane x_p - transfer (one
//                  subtract), new plane transfer, EVERY plane np.clip(., 0, lai_max) (NaN passes); ECO_LAI = sum over s within a
//                  layer, then over the layers (:383-384); per-workgroup partials of nansum_land sum_k max(x, 0) per species
//                  (recompute_species_weights_from_LAI, :343-359) in the layout of k_ind_stack.  Reads S K + K planes, writes
//                  (S + 1) K + 1; a thread keeps K layer sums and S + 1 species sums in registers
//   weights        k_ind_weights (qd_indiv_daily.hip), one workgroup: species_weights and w / (sum(w) + 1e-12) into the lane's
//                  germination weights
// f64 throughout, contraction off (Makefile), no atomics.  The only reordering against NumPy is the blocked land sum behind the
// weights (NumPy's nansum is pairwise).  The lane's mode table gets the mode population.py:511 gives an index it does not hold.
#include "qd_span.h"
#include "qd_blockred.h"

struct QdSpArgs {
    int nlon, S, K, parent;           // S: species before the split
    double frac, lai_max;
    const double* L0; double* L1; size_t plane;
    const uint8_t* land;
    double* lai; int lai_f32;
    double* partial;
};

template <int SMAX>
__global__ void __launch_bounds__(QD_BLOCK)
k_spec_split(QdSpArgs A) {
    const int j = blockIdx.x * QD_BLOCK + threadIdx.x;
    const int S1 = A.S + 1, K = A.K;
    double d[SMAX];
#pragma unroll
    for (int s = 0; s < SMAX; ++s) d[s] = 0.0;
    if (j < A.nlon) {
        const size_t o = (size_t)blockIdx.y * A.nlon + j;
        const bool land = A.land[o] == 1;
        double lay[QD_ECO_DAILY_MAX_K];
#pragma unroll
        for (int s = 0; s < SMAX; ++s)
            if (s < S1) {
                const int src = s < A.S ? s : A.parent;
                double ls = 0.0;
#pragma unroll
                for (int k = 0; k < QD_ECO_DAILY_MAX_K; ++k)
                    if (k < K) {
                        const double x = A.L0[(size_t)(src * K + k) * A.plane + o];
                        double v = x;
                        if (src == A.parent) {
                            const double transfer = A.frac * x;
                            v = (s == A.S) ? transfer : x - transfer;
                        }
                        v = qd_clip(v, 0.0, A.lai_max);
                        A.L1[(size_t)(s * K + k) * A.plane + o] = v;
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
    qd_block_partials(d, S1, nullptr, A.partial, (size_t)gridDim.x * gridDim.y, (size_t)blockIdx.y * gridDim.x + blockIdx.x);
}

namespace {
struct SpBuffers {                    // what the event allocates; the stack and the weights leave with qd_eco_daily_adopt
    double *L1 = nullptr, *w1 = nullptr, *wout = nullptr;
    QdPartials partial;
    ~SpBuffers() { for (void* q : {(void*)L1, (void*)w1, (void*)wout}) if (q) hipFree(q); partial.free(); }
};
}

extern "C" int qd_eco_daily_speciate(qd_handle c, int parent, double frac, double* weights_out) {
    if (!c || !weights_out) return -1;
    if (!qd_whole_globe(c))
        return qd_fail(c, "qd_eco_daily_speciate: the daily vegetation step needs a whole-globe handle (world == 1, n_rows == n_lat); "
                          "latitude bands are not supported");
    const double* L0; int S, K;
    if (!qd_eco_daily_stack(c, &L0, &S, &K)) return qd_fail(c, "qd_eco_daily_speciate: qd_eco_daily_configure has not been called");
    if (S + 1 > QD_MAX_SPECIES) return qd_fail(c, "qd_eco_daily_speciate: n_species + 1 out of range (1..64)");
    if (c->idaily)
        return qd_fail(c, "qd_eco_daily_speciate: qd_indiv_daily_configure is in force -- the individuals were sampled for the stack's species");
    const double f = frac < 0.0 ? 0.0 : (frac > 0.5 ? 0.5 : frac);           // np.clip(frac, 0, 0.5); NaN stays
    if (!(f > 0.0)) return qd_fail(c, "qd_eco_daily_speciate: frac <= 0 splits nothing (population.py:371-372 adds no species then)");
    hipSetDevice(c->desc.device);
    QD_HIP(c, hipStreamSynchronize(c->stream));
    const size_t cells = c->geo.cells();
    const int S1 = S + 1, nlat = c->geo.nlat, nlon = c->geo.nlon;
    const dim3 grid((nlon + QD_BLOCK - 1) / QD_BLOCK, nlat), block(QD_BLOCK);
    const int nblk = (int)(grid.x * grid.y);
    SpBuffers B;
    QD_HIP(c, hipMalloc(&B.L1, (size_t)S1 * K * cells * sizeof(double)));
    QD_HIP(c, hipMalloc(&B.w1, (size_t)S1 * sizeof(double)));
    QD_HIP(c, hipMalloc(&B.wout, (size_t)S1 * sizeof(double)));
    if (int rc = B.partial.ensure(c, S1, nblk)) return rc;
    QdSpArgs A;
    A.nlon = nlon; A.S = S; A.K = K;
    A.parent = parent < 0 ? 0 : (parent > S - 1 ? S - 1 : parent);
    A.frac = f; A.lai_max = qd_eco_daily_lai_max(c);
    A.L0 = L0; A.L1 = B.L1; A.plane = cells;
    A.land = c->land;
    A.lai = c->f[QD_F_ECO_LAI]; A.lai_f32 = c->eco.p.map_f32 ? 1 : 0;
    A.partial = B.partial.p;
    {
        QdScope sc(c, "eco_speciate");
        if (S1 <= 8) hipLaunchKernelGGL(k_spec_split<8>, grid, block, 0, c->stream, A);
        else if (S1 <= 24) hipLaunchKernelGGL(k_spec_split<24>, grid, block, 0, c->stream, A);
        else hipLaunchKernelGGL(k_spec_split<QD_MAX_SPECIES>, grid, block, 0, c->stream, A);
        qd_species_weights_launch(c, B.partial.p, nblk, S1, B.wout, B.w1);
    }
    QD_HIP(c, hipMemcpyAsync(weights_out, B.wout, (size_t)S1 * sizeof(double), hipMemcpyDeviceToHost, c->stream));
    QD_HIP(c, hipStreamSynchronize(c->stream));                         // the old stack is read until here; the host buffer is borrowed
    if (int rc = qd_launch_check(c, "qd_eco_daily_speciate")) return rc;
    qd_eco_daily_adopt(c, B.L1, B.w1);
    B.L1 = nullptr; B.w1 = nullptr;
    // the canopy state of qd_eco_set_lai_layers(h, layers, n, 0): new layers, snapshot and recompute clock untouched
    c->eco.have_lai = 1; c->eco.lai_version++;
    qd_mark(c, {c->f[QD_F_ECO_LAI]}, 0);
    return 0;
}
