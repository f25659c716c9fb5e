// qd_eco_state.hip -- the restore of the vegetation state from an ecology autosave file, gfx950.
//
// EcologyAdapter.load_autosave (pygcm/ecology/adapter.py:742-757): from the file's one LAI plane and its species weights
//   L = np.clip(LAI, 0, lai_max);  LAI_layers_SK[s][k] = float(w_s) * (L / float(K))  for every species s and layer k.
// One launch over the cells reads the plane once and writes the S * K planes where they live -- the resident stack of the daily
// lane -- together with ECO_LAI.  Nothing of it is on the per-step path; the point is that the stack (20 planes by default) never
// crosses the host link.
//
// The arithmetic restates NumPy's, in the precision the reference runs it in:
//   * a NetCDF file hands the reference float32 arrays, and NumPy keeps float32 through the clip, the division by the Python float
//     K and the product with the Python float w_s; only the store into the f64 stack widens.  lai_is_f32 selects that chain: one
//     correctly rounded f32 divide (never a multiply by 1 / K), one f32 multiply, subnormals kept;
//   * the NPZ branch hands it float64: the same chain in f64.
//   * np.clip passes NaN through (fmin / fmax would not), and the reference does not mask by land: ocean cells keep their values.
// ECO_LAI receives the sum of the planes in np.sum(axis=(0,1))'s order (s outer, k inner, f64), which is what total_LAI() -- the
// reader of the canopy factor, the recompute policy and summary() -- sees after a load; pop.LAI itself (the clipped plane) differs
// from it in the last bit and has no reader on the device.
#include "qd_internal.h"

template <typename T>
__device__ __forceinline__ T qd_es_clip(T x, T lo, T hi) {       // np.clip: min(max(x, lo), hi), NaN passes
    if (x != x) return x;
    const T a = x > lo ? x : lo;
    return a < hi ? a : hi;
}

struct QdESArgs {
    size_t cells;
    const void* lai;                  // [cells] the file's plane, f32 or f64
    double* L;                        // [S * K][cells] the resident stack, or nullptr
    double* lai_out;                  // ECO_LAI
    int lai_out_f32;
    int S, K;
    double lai_max;
    double w[QD_MAX_SPECIES];
};

template <typename T>
__global__ void __launch_bounds__(QD_BLOCK)
k_eco_state_restore(QdESArgs A) {
    const size_t o = (size_t)blockIdx.x * QD_BLOCK + threadIdx.x;
    if (o >= A.cells) return;
    const T x = reinterpret_cast<const T*>(A.lai)[o];
    const T Lc = qd_es_clip<T>(x, (T)0, (T)A.lai_max);
    const T q = Lc / (T)A.K;                                    // IEEE divide in T
    double tot = 0.0;
    for (int s = 0; s < A.S; ++s) {
        const double v = (double)((T)A.w[s] * q);
        for (int k = 0; k < A.K; ++k) {
            if (A.L) A.L[(size_t)(s * A.K + k) * A.cells + o] = v;
            tot = (s == 0 && k == 0) ? v : tot + v;
        }
    }
    if (A.lai_out_f32) reinterpret_cast<float*>(A.lai_out)[o] = (float)tot; else A.lai_out[o] = tot;
}

extern "C" int qd_eco_state_restore(qd_handle c, const void* lai, int lai_is_f32, const double* w, int n_species, int n_layers,
                                    double lai_max) {
    if (!c || !lai || !w) return -1;
    if (!qd_whole_globe(c))
        return qd_fail(c, "qd_eco_state_restore: the restore needs a whole-globe handle (world == 1, n_rows == n_lat); latitude bands are "
                          "not supported");
    if (!c->eco.configured) return qd_fail(c, "qd_eco_state_restore: qd_eco_configure has not been called");
    if (n_species < 1 || n_species > QD_MAX_SPECIES) return qd_fail(c, "qd_eco_state_restore: n_species out of range (1..64)");
    if (n_layers < 1 || n_layers > QD_ECO_DAILY_MAX_K) return qd_fail(c, "qd_eco_state_restore: n_layers out of range (1..8)");
    const double* stack = nullptr;
    int S = 0, K = 0;
    if (qd_eco_daily_stack(c, &stack, &S, &K) && (S != n_species || K != n_layers))
        return qd_fail(c, "qd_eco_state_restore: n_species / n_layers are not the resident stack's (configure the daily lane for the "
                          "file's species count first)");
    hipSetDevice(c->desc.device);
    QdESArgs A;
    A.cells = c->geo.cells();
    double* stage = c->scratch[10];                             // one slab of cells doubles: holds either form of the plane
    QD_HIP(c, hipMemcpyAsync(stage, lai, A.cells * (lai_is_f32 ? sizeof(float) : sizeof(double)), hipMemcpyHostToDevice, c->stream));
    QD_HIP(c, hipStreamSynchronize(c->stream));                 // the host buffer is only borrowed for the call
    A.lai = stage;
    A.L = const_cast<double*>(stack);
    A.lai_out = c->f[QD_F_ECO_LAI];
    A.lai_out_f32 = c->eco.p.map_f32 ? 1 : 0;
    A.S = n_species; A.K = n_layers;
    A.lai_max = lai_max;
    for (int s = 0; s < QD_MAX_SPECIES; ++s) A.w[s] = s < n_species ? w[s] : 0.0;
    const dim3 grid((unsigned)((A.cells + QD_BLOCK - 1) / QD_BLOCK)), block(QD_BLOCK);
    if (lai_is_f32) hipLaunchKernelGGL(k_eco_state_restore<float>, grid, block, 0, c->stream, A);
    else hipLaunchKernelGGL(k_eco_state_restore<double>, grid, block, 0, c->stream, A);
    // the canopy state of qd_eco_set_lai_layers(h, stack, n, 0): new layers, snapshot and recompute clock untouched
    c->eco.have_lai = 1; c->eco.lai_version++;
    qd_mark(c, {c->f[QD_F_ECO_LAI]}, c->geo.halo);
    return qd_launch_check(c, "qd_eco_state_restore");
}
