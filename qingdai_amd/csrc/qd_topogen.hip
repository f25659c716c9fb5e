// qd_topogen.hip -- the procedural planet (P004, pygcm/topography.py:58-83, 90-276) built on the device.
//
// Stages, in the reference's order (the random draws and the Gaussian weights come from the host):
//   k_tg_continents   _generate_L1_continents (:148-154): per cell the sum over the centres of A exp(-(d / sigma) ** p),
//                     d = arccos(clip(sin lat sin lat0 + cos lat cos lat0 cos(lon - lon0))) from host tables
//   k_tg_filter       gaussian_filter(mode=("nearest", "wrap")) (:164, :194, :245): two separable passes, bit-identical
//   k_tg_sum/_fin     every (x - mean) / (std + 1e-8) (:157, :165, :170, :195, :202, :240): mean, then centred squares
//   k_tg_lin          the normalisations fused with the blends (:168, :196, :237) and the scaling (:242)
//   k_tg_hist/_pick   _weighted_quantile (:58-83): a weighted MSB-first radix select over the f64 bit patterns
//   k_tg_mask         elevation >= sea level (:271)
//
// The filter.  One line is a row (axis 1, periodic) or a column (axis 0, clamped).  A workgroup stages TG lines in LDS -- one
// row, or a strip of C <= 32 neighbouring columns as [row][C] -- and every lane owns TG_M = 5 neighbouring outputs of one line.
// For tap distance k an output p needs F[p - k] and F[p + k]; the five outputs of a lane need five neighbouring values on each
// side, and going from k to k - 1 shifts both windows by one: ONE new LDS read per side and tap serves all five outputs.  The
// windows are register rings (the k loop is unrolled by TG_M, so every ring slot is a fixed register).  A lane's reads are
// TG_M * C doubles apart from its neighbour's: with TG_M = 5 and C a power of two the 32 lanes of a ds_read_b64 group fall on
// 32 different bank pairs.  The accumulation is scipy's symmetric correlate1d, as topography._filter_axis restates it: the
// centre tap first, then (F[p - k] + F[p + k]) * w[r - k] from k = r down to 1, no FMA (-ffp-contract=off).  Indices wrap by
// true modulo / clamp, so a radius larger than the axis is fine.  A line that does not fit the LDS budget takes the same
// kernel with the reads going to global memory (LDS = false).
//
// The select.  Cells of a row share the weight max(cos lat, 0); it is held as a 38-bit fixed-point integer, so that a bucket's
// weight is an integer sum: the same for any order of the atomics.  Eight passes of eight bits over the order-preserving key of
// the bit pattern pick, from the top byte down, the first non-empty bucket at which the cumulative weight reaches
// ceil(q * total); the result is one of the field's values (-0.0 counts as +0.0).
// Whole-globe handles only.
#include "qd_blockred.h"
#include <cmath>
#include <vector>

#define TG_M 5                 // neighbouring outputs of one lane
#define TG_CMAX 32             // columns of a latitude strip
#define TG_LDS_MAX (64 * 1024) // a workgroup's LDS budget
#define TG_NB_MAX 1024         // workgroups of a reduction: one partial each
#define TG_BINS 256            // an 8-bit digit of the select
#define TG_WBITS 38            // fixed-point bits of a row weight: cells <= 2^24 and weight <= 2^38 keep every sum below 2^62
#define TG_MAX_CELLS (1 << 24)

// ------------------------------------------------------------------ continents
__global__ void __launch_bounds__(QD_BLOCK)
k_tg_continents(int nlat, int nlon, int ncont, const double* __restrict__ cont, const double* __restrict__ coslon,
                const double* __restrict__ sin_lat, const double* __restrict__ cos_lat, double sigma, double p, double* __restrict__ out) {
    const int i = blockIdx.x * QD_BLOCK + threadIdx.x, j = blockIdx.y;
    if (i >= nlon) return;
    const double sl = sin_lat[j], cl = cos_lat[j];
    double h = 0.0;
    for (int c = 0; c < ncont; ++c) {
        double cd = sl * cont[3 * c] + cl * cont[3 * c + 1] * coslon[(size_t)c * nlon + i];
        cd = cd < -1.0 ? -1.0 : (cd > 1.0 ? 1.0 : cd);
        h += cont[3 * c + 2] * exp(-qd_pow_np(acos(cd) / sigma, p));
    }
    out[(size_t)j * nlon + i] = h;
}

// ------------------------------------------------------------------ filter
// lines: line l of nlines starts at in + l * sline and steps by spos; n positions.  Workgroup b holds the lines [b C, b C + C).
template <bool WRAP, bool LDS>
__global__ void __launch_bounds__(QD_BLOCK)
k_tg_filter(const double* __restrict__ in, double* __restrict__ out, int n, int nlines, int C, size_t spos, size_t sline,
            const double* __restrict__ w, int r) {
    extern __shared__ __align__(16) double tg_sm[];
    const int line0 = blockIdx.x * C;
    if (LDS) {
        for (int e = threadIdx.x; e < n * C; e += blockDim.x) {
            const int pos = e / C, c = e - pos * C;
            tg_sm[e] = line0 + c < nlines ? in[(size_t)(line0 + c) * sline + (size_t)pos * spos] : 0.0;
        }
        __syncthreads();
    }
    const int nchunk = (n + TG_M - 1) / TG_M;
    const double wc = w[r];
    for (int it = threadIdx.x; it < nchunk * C; it += blockDim.x) {
        const int q = it / C, c = it - q * C;
        if (line0 + c >= nlines) continue;
        const int p0 = q * TG_M;
        const double* src = in + (size_t)(line0 + c) * sline;
        auto rd = [&](int pos) -> double { return LDS ? tg_sm[pos * C + c] : src[(size_t)pos * spos]; };
        auto ext = [&](int x) -> int {       // WRAP: x is kept in [0, n) by its owner; clamp otherwise
            return WRAP ? x : (x < 0 ? 0 : (x > n - 1 ? n - 1 : x));
        };
        auto mod = [&](int x) -> int { if (!WRAP) return x; x %= n; return x < 0 ? x + n : x; };
        double acc[TG_M], L[TG_M], R[TG_M];
        int xl = mod(p0 - r), xr = mod(p0 + r);
#pragma unroll
        for (int m = 0; m < TG_M; ++m) {
            const int pc = p0 + m < n ? p0 + m : n - 1;
            acc[m] = rd(pc) * wc;
            L[m] = rd(ext(xl));
            R[m] = rd(ext(xr));
            ++xl; ++xr;
            if (WRAP) { if (xl == n) xl = 0; if (xr == n) xr = 0; }
        }
        // xl: the position entering the left window next (p0 + TG_M - k); the right window is entered from below (p0 + k - 1)
        xr = mod(p0 + r - 1);
        for (int k = r; k >= 1; k -= TG_M) {
#pragma unroll
            for (int t = 0; t < TG_M; ++t) {
                if (k - t >= 1) {
                    const double wk = w[r - (k - t)];
#pragma unroll
                    for (int m = 0; m < TG_M; ++m) acc[m] = acc[m] + (L[(m + t) % TG_M] + R[(m - t + TG_M) % TG_M]) * wk;
                    L[t] = rd(ext(xl));
                    R[TG_M - 1 - t] = rd(ext(xr));
                    ++xl; --xr;
                    if (WRAP) { if (xl == n) xl = 0; if (xr < 0) xr = n - 1; }
                }
            }
        }
        double* dst = out + (size_t)(line0 + c) * sline;
#pragma unroll
        for (int m = 0; m < TG_M; ++m)
            if (p0 + m < n) dst[(size_t)(p0 + m) * spos] = acc[m];
    }
}

// ------------------------------------------------------------------ mean and std
// stat = {mean, std + 1e-8}.  SQ = 0: partial sums of x.  SQ = 1: every workgroup folds the nb partial sums (the same order in
// each) into the mean, then partial sums of (x - mean)^2.  k_tg_fin: std = sqrt(sum / N) (the population std of np.std).
template <int SQ>
__global__ void __launch_bounds__(QD_BLOCK)
k_tg_sum(const double* __restrict__ x, int N, int nb, const double* __restrict__ part_in, double* __restrict__ part_out, double* stat) {
    __shared__ double s_mean;
    double mean = 0.0;
    if (SQ) {
        double v[1];
        qd_planes_strided<1>(part_in, nb, 1, nullptr, v);
        qd_block_totals<1>(v, nullptr);
        if (threadIdx.x == 0) {
            s_mean = v[0] / (double)N;
            if (blockIdx.x == 0) stat[0] = s_mean;
        }
        __syncthreads();
        mean = s_mean;
    }
    double a = 0.0;
    for (size_t k = (size_t)blockIdx.x * QD_BLOCK + threadIdx.x; k < (size_t)N; k += (size_t)nb * QD_BLOCK) {
        const double d = x[k] - mean;
        a += SQ ? d * d : d;
    }
    const double v[1] = {a};
    qd_block_partials<1>(v, 1, nullptr, part_out, (size_t)nb, (size_t)blockIdx.x);
}

__global__ void __launch_bounds__(QD_BLOCK) k_tg_fin(int N, int nb, const double* __restrict__ part, double* stat) {
    double v[1];
    qd_planes_strided<1>(part, nb, 1, nullptr, v);
    qd_block_totals<1>(v, nullptr);
    if (threadIdx.x == 0) stat[1] = sqrt(v[0] / (double)N) + 1e-8;
}

// out = a * ((x - sx[0]) / sx[1]) [+ b * ((y - sy[0]) / sy[1])]: the normalisations fused with the blend that reads them
__global__ void __launch_bounds__(QD_BLOCK)
k_tg_lin(int N, double a, const double* x, const double* __restrict__ sx, double b, const double* __restrict__ y,
         const double* __restrict__ sy, double* out) {       // out may be x
    const size_t k = (size_t)blockIdx.x * QD_BLOCK + threadIdx.x;
    if (k >= (size_t)N) return;
    double v = a * ((x[k] - sx[0]) / sx[1]);
    if (y) v = v + b * ((y[k] - sy[0]) / sy[1]);
    out[k] = v;
}

// ------------------------------------------------------------------ weighted select
__device__ __forceinline__ unsigned long long tg_key(double x) {       // ascending in x; -0.0 and +0.0 share a key
    const unsigned long long u = x == 0.0 ? 0ull : (unsigned long long)__double_as_longlong(x);
    return (u >> 63) ? ~u : (u | 0x8000000000000000ull);
}
__device__ __forceinline__ double tg_unkey(unsigned long long k) {
    const unsigned long long u = (k >> 63) ? (k & 0x7fffffffffffffffull) : ~k;
    return __longlong_as_double((long long)u);
}

// sel = {key bits found so far, the weight still to reach inside them}; hw / hc: bucket weight and count of this digit
__global__ void __launch_bounds__(QD_BLOCK)
k_tg_hist(const double* __restrict__ x, int N, int nlon, int nb, const unsigned long long* __restrict__ wfix,
          const unsigned long long* __restrict__ sel, int shift, unsigned long long* hw, unsigned int* hc) {
    __shared__ unsigned long long sw[TG_BINS];
    __shared__ unsigned int sc[TG_BINS];
    for (int k = threadIdx.x; k < TG_BINS; k += QD_BLOCK) { sw[k] = 0ull; sc[k] = 0u; }
    __syncthreads();
    const unsigned long long pre = sel[0];
    for (size_t k = (size_t)blockIdx.x * QD_BLOCK + threadIdx.x; k < (size_t)N; k += (size_t)nb * QD_BLOCK) {
        const unsigned long long key = tg_key(x[k]);
        if (shift < 56 && (key >> (shift + 8)) != (pre >> (shift + 8))) continue;
        const unsigned int d = (unsigned int)((key >> shift) & (TG_BINS - 1));
        atomicAdd(&sw[d], wfix[k / (size_t)nlon]);
        atomicAdd(&sc[d], 1u);
    }
    __syncthreads();
    for (int k = threadIdx.x; k < TG_BINS; k += QD_BLOCK)
        if (sc[k]) { atomicAdd(&hw[k], sw[k]); atomicAdd(&hc[k], sc[k]); }
}

// one workgroup: the first non-empty bucket at which the cumulative weight reaches sel[1] (the last non-empty one if none does),
// the histogram cleared for the next digit; after the last digit the value itself
__global__ void __launch_bounds__(TG_BINS)
k_tg_pick(unsigned long long* hw, unsigned int* hc, unsigned long long* sel, int shift, double* sea) {
    __shared__ unsigned long long sw[TG_BINS];
    __shared__ unsigned int sc[TG_BINS];
    const int t = threadIdx.x;
    sw[t] = hw[t]; sc[t] = hc[t];
    hw[t] = 0ull; hc[t] = 0u;
    __syncthreads();
    if (t != 0) return;
    const unsigned long long T = sel[1];
    unsigned long long cum = 0ull, rest = ~0ull;
    int pick = -1, last = 0;
    for (int b = 0; b < TG_BINS; ++b) {
        if (!sc[b]) continue;
        last = b;
        if (cum + sw[b] >= T) { pick = b; rest = T - cum; break; }
        cum += sw[b];
    }
    if (pick < 0) pick = last;           // never reached (rounding of the threshold): the largest value, as np.clip(idx) does
    const unsigned long long key = sel[0] | ((unsigned long long)pick << shift);
    sel[0] = key;
    sel[1] = rest;
    if (shift == 0) *sea = tg_unkey(key);
}

__global__ void __launch_bounds__(QD_BLOCK) k_tg_mask(const double* __restrict__ x, int N, const double* __restrict__ sea, uint8_t* __restrict__ m) {
    const size_t k = (size_t)blockIdx.x * QD_BLOCK + threadIdx.x;
    if (k < (size_t)N) m[k] = x[k] >= sea[0] ? 1 : 0;
}

// ------------------------------------------------------------------ host side
namespace {
struct TgBuf {
    std::vector<void*> p;
    template <class T> T* get(size_t n) {
        void* q = nullptr;
        if (hipMalloc(&q, std::max<size_t>(n, 1) * sizeof(T)) != hipSuccess) return nullptr;
        p.push_back(q);
        return (T*)q;
    }
    ~TgBuf() { for (void* q : p) hipFree(q); }
};

bool tg_finite(const double* a, size_t n) {
    for (size_t k = 0; k < n; ++k)
        if (!std::isfinite(a[k])) return false;
    return true;
}

int tg_threads(int items) { return std::min(QD_BLOCK, std::max(64, (items + 63) / 64 * 64)); }

// one separable pass over device memory; w: device half kernel [r + 1]
void tg_pass(qd_ctx* c, bool lat, const double* in, double* out, int nlat, int nlon, const double* w, int r, int lds_bytes) {
    const int n = lat ? nlat : nlon, nlines = lat ? nlon : nlat;
    const size_t spos = lat ? (size_t)nlon : 1, sline = lat ? 1 : (size_t)nlon;
    int C = 1;
    bool lds = (size_t)n * sizeof(double) <= (size_t)lds_bytes;
    if (lat) {
        if (lds) while (C < TG_CMAX && C * 2 <= nlines && (size_t)n * (C * 2) * sizeof(double) <= (size_t)lds_bytes) C *= 2;
        else C = std::min(TG_CMAX, nlines);        // global reads: neighbouring lanes on neighbouring columns
    }
    const int items = (n + TG_M - 1) / TG_M * C, nblk = (nlines + C - 1) / C;
    const dim3 g(nblk), b(tg_threads(items));
    const size_t sm = lds ? (size_t)n * C * sizeof(double) : 0;
    if (lat) {
        if (lds) hipLaunchKernelGGL((k_tg_filter<false, true>), g, b, sm, c->stream, in, out, n, nlines, C, spos, sline, w, r);
        else hipLaunchKernelGGL((k_tg_filter<false, false>), g, b, 0, c->stream, in, out, n, nlines, C, spos, sline, w, r);
    } else {
        if (lds) hipLaunchKernelGGL((k_tg_filter<true, true>), g, b, sm, c->stream, in, out, n, nlines, C, spos, sline, w, r);
        else hipLaunchKernelGGL((k_tg_filter<true, false>), g, b, 0, c->stream, in, out, n, nlines, C, spos, sline, w, r);
    }
}

int tg_nb(int N) { return std::min(TG_NB_MAX, (N + QD_BLOCK - 1) / QD_BLOCK); }

// stat <- {mean, std + 1e-8} of x[0 .. N)
void tg_stats(qd_ctx* c, const double* x, int N, double* part, double* stat) {
    const int nb = tg_nb(N);
    hipLaunchKernelGGL((k_tg_sum<0>), dim3(nb), dim3(QD_BLOCK), 0, c->stream, x, N, nb, (const double*)nullptr, part, stat);
    hipLaunchKernelGGL((k_tg_sum<1>), dim3(nb), dim3(QD_BLOCK), 0, c->stream, x, N, nb, (const double*)part, part + TG_NB_MAX, stat);
    hipLaunchKernelGGL(k_tg_fin, dim3(1), dim3(QD_BLOCK), 0, c->stream, N, nb, (const double*)(part + TG_NB_MAX), stat);
}

int tg_check_handle(qd_ctx* c, const char* who, int n_lat, int n_lon) {
    if (!c->geo.full || c->desc.world > 1)
        return qd_fail(c, (std::string(who) + ": topography generation needs a whole-globe handle (world == 1, n_rows == n_lat); "
                                              "latitude bands are not supported").c_str());
    if (n_lat != c->geo.nlat || n_lon != c->geo.nlon) return qd_fail(c, (std::string(who) + ": shape is not the handle's grid").c_str());
    if (n_lat < 1 || n_lon < 1 || n_lat > 65535 || (size_t)n_lat * n_lon > (size_t)TG_MAX_CELLS)
        return qd_fail(c, (std::string(who) + ": grid too large (more than 65535 rows or 2^24 cells)").c_str());
    return 0;
}

int tg_check_kernel(qd_ctx* c, const char* who, const double* w, int r) {
    if (r < 0 || r > QD_TOPOGEN_MAX_RADIUS) return qd_fail(c, (std::string(who) + ": filter radius outside [0, QD_TOPOGEN_MAX_RADIUS]").c_str());
    if (!w || !tg_finite(w, (size_t)r + 1)) return qd_fail(c, (std::string(who) + ": missing or non-finite filter weights").c_str());
    return 0;
}

int tg_lds_budget(int lds_bytes) { return lds_bytes <= 0 ? TG_LDS_MAX : std::min(lds_bytes, TG_LDS_MAX); }
}  // namespace

extern "C" int qd_topogen_smooth(qd_handle c, int n_lat, int n_lon, const double* field, const double* w_lat, int r_lat,
                                 const double* w_lon, int r_lon, int lds_bytes, double* out) {
    if (!c) return -1;
    if (tg_check_handle(c, "qd_topogen_smooth", n_lat, n_lon)) return -1;
    if (!field || !out) return qd_fail(c, "qd_topogen_smooth: missing array");
    if (tg_check_kernel(c, "qd_topogen_smooth", w_lat, r_lat) || tg_check_kernel(c, "qd_topogen_smooth", w_lon, r_lon)) return -1;
    const size_t cells = (size_t)n_lat * n_lon;
    if (!tg_finite(field, cells)) return qd_fail(c, "qd_topogen_smooth: non-finite field");
    hipSetDevice(c->desc.device);
    TgBuf B;
    double* d_a = B.get<double>(cells);
    double* d_b = B.get<double>(cells);
    double* d_w = B.get<double>((size_t)r_lat + r_lon + 2);
    if (!d_a || !d_b || !d_w) return qd_fail(c, "qd_topogen_smooth: device allocation failed");
    hipStream_t s = c->stream;
    QD_HIP(c, hipMemcpyAsync(d_a, field, cells * sizeof(double), hipMemcpyHostToDevice, s));
    QD_HIP(c, hipMemcpyAsync(d_w, w_lat, ((size_t)r_lat + 1) * sizeof(double), hipMemcpyHostToDevice, s));
    QD_HIP(c, hipMemcpyAsync(d_w + r_lat + 1, w_lon, ((size_t)r_lon + 1) * sizeof(double), hipMemcpyHostToDevice, s));
    const int lds = tg_lds_budget(lds_bytes);
    tg_pass(c, true, d_a, d_b, n_lat, n_lon, d_w, r_lat, lds);
    tg_pass(c, false, d_b, d_a, n_lat, n_lon, d_w + r_lat + 1, r_lon, lds);
    QD_HIP(c, hipMemcpyAsync(out, d_a, cells * sizeof(double), hipMemcpyDeviceToHost, s));
    QD_HIP(c, hipStreamSynchronize(s));
    const hipError_t e = hipGetLastError();
    if (e != hipSuccess) return qd_fail(c, "qd_topogen_smooth: kernel", e);
    return 0;
}

extern "C" int qd_topogen_build(qd_handle c, int n_lat, int n_lon, const double* par, int n_oct, const double* oct_amp,
                                const double* noise, int n_cont, const double* cont, const double* cont_coslon, const double* sin_lat,
                                const double* cos_lat, const double* area_w, const int32_t* radii, const double* weights,
                                double* elevation, uint8_t* land_mask, double* sea_level_m) {
    if (!c) return -1;
    c->topogen_ms = -1.0;
    if (tg_check_handle(c, "qd_topogen_build", n_lat, n_lon)) return -1;
    if (n_oct < 0 || n_oct > QD_TOPOGEN_MAX_OCTAVES) return qd_fail(c, "qd_topogen_build: octave count outside [0, QD_TOPOGEN_MAX_OCTAVES = 16]");
    if (n_cont < 0 || n_cont > QD_TOPOGEN_MAX_CONTINENTS)
        return qd_fail(c, "qd_topogen_build: continent count outside [0, QD_TOPOGEN_MAX_CONTINENTS = 64]");
    if (!par || !noise || !sin_lat || !cos_lat || !area_w || !radii || !weights || !elevation || !land_mask || !sea_level_m ||
        (n_oct > 0 && !oct_amp) || (n_cont > 0 && (!cont || !cont_coslon)))
        return qd_fail(c, "qd_topogen_build: missing array");
    const size_t cells = (size_t)n_lat * n_lon;
    const int N = (int)cells, nfilt = n_oct + 2;
    if (!tg_finite(par, QD_TOPOGEN_NPAR) || !tg_finite(oct_amp, (size_t)n_oct)) return qd_fail(c, "qd_topogen_build: non-finite parameter");
    if (!(par[0] > 0.0)) return qd_fail(c, "qd_topogen_build: the continent width must be positive");
    if (!tg_finite(cont, (size_t)n_cont * 3) || !tg_finite(cont_coslon, (size_t)n_cont * n_lon) || !tg_finite(sin_lat, n_lat) ||
        !tg_finite(cos_lat, n_lat) || !tg_finite(area_w, n_lat))
        return qd_fail(c, "qd_topogen_build: non-finite table");
    if (!tg_finite(noise, (size_t)(1 + n_oct) * cells)) return qd_fail(c, "qd_topogen_build: non-finite noise");
    std::vector<size_t> woff(2 * (size_t)nfilt);
    size_t wlen = 0;
    for (int f = 0; f < 2 * nfilt; ++f) {
        if (radii[f] < 0 || radii[f] > QD_TOPOGEN_MAX_RADIUS) return qd_fail(c, "qd_topogen_build: filter radius outside [0, QD_TOPOGEN_MAX_RADIUS]");
        woff[f] = wlen;
        wlen += (size_t)radii[f] + 1;
    }
    if (!tg_finite(weights, wlen)) return qd_fail(c, "qd_topogen_build: non-finite filter weights");
    // fixed-point row weights and the threshold: total <= 2^24 cells * 2^38 < 2^62, exact in 64 bits
    std::vector<unsigned long long> wfix(n_lat);
    unsigned long long total = 0;
    for (int j = 0; j < n_lat; ++j) {
        const double wj = area_w[j];
        if (wj < 0.0 || wj > 1.0) return qd_fail(c, "qd_topogen_build: area weight outside [0, 1]");
        wfix[j] = (unsigned long long)std::llround(std::ldexp(wj, TG_WBITS));
        total += wfix[j] * (unsigned long long)n_lon;
    }
    const double q = 1.0 - par[7];
    unsigned long long thr = 0;
    if (q > 0.0) thr = q >= 1.0 ? total : std::min(total, (unsigned long long)std::ceil(q * (double)total));

    hipSetDevice(c->desc.device);
    TgBuf B;
    double* d_noise = B.get<double>((size_t)(1 + n_oct) * cells);
    double* d_tmp = B.get<double>(cells);
    double* d_sm = B.get<double>(cells);
    double* d_h1 = B.get<double>(cells);
    double* d_fbm = B.get<double>(cells);
    double* d_w = B.get<double>(wlen);
    double* d_tab = B.get<double>((size_t)2 * n_lat + (size_t)n_cont * 3 + (size_t)n_cont * n_lon);
    double* d_part = B.get<double>(2 * TG_NB_MAX);
    double* d_stat = B.get<double>(16);          // six {mean, std + 1e-8}, the identity {0, 1}, the sea level
    unsigned long long* d_wfix = B.get<unsigned long long>(n_lat);
    unsigned long long* d_sel = B.get<unsigned long long>(2 + TG_BINS);
    unsigned int* d_hc = B.get<unsigned int>(TG_BINS);
    uint8_t* d_mask = B.get<uint8_t>(cells);
    hipEvent_t ev0 = nullptr, ev1 = nullptr;
    if (!d_noise || !d_tmp || !d_sm || !d_h1 || !d_fbm || !d_w || !d_tab || !d_part || !d_stat || !d_wfix || !d_sel || !d_hc || !d_mask)
        return qd_fail(c, "qd_topogen_build: device allocation failed");
    hipStream_t s = c->stream;
    double* d_sinlat = d_tab; double* d_coslat = d_tab + n_lat; double* d_cont = d_tab + 2 * n_lat; double* d_cl = d_cont + (size_t)n_cont * 3;
    unsigned long long* d_hw = d_sel + 2;
    const double ident[2] = {0.0, 1.0};
    const unsigned long long sel0[2] = {0ull, thr};
    QD_HIP(c, hipMemcpyAsync(d_noise, noise, (size_t)(1 + n_oct) * cells * sizeof(double), hipMemcpyHostToDevice, s));
    QD_HIP(c, hipMemcpyAsync(d_w, weights, wlen * sizeof(double), hipMemcpyHostToDevice, s));
    QD_HIP(c, hipMemcpyAsync(d_sinlat, sin_lat, n_lat * sizeof(double), hipMemcpyHostToDevice, s));
    QD_HIP(c, hipMemcpyAsync(d_coslat, cos_lat, n_lat * sizeof(double), hipMemcpyHostToDevice, s));
    if (n_cont > 0) {
        QD_HIP(c, hipMemcpyAsync(d_cont, cont, (size_t)n_cont * 3 * sizeof(double), hipMemcpyHostToDevice, s));
        QD_HIP(c, hipMemcpyAsync(d_cl, cont_coslon, (size_t)n_cont * n_lon * sizeof(double), hipMemcpyHostToDevice, s));
    }
    QD_HIP(c, hipMemcpyAsync(d_stat + 12, ident, sizeof(ident), hipMemcpyHostToDevice, s));
    QD_HIP(c, hipMemcpyAsync(d_wfix, wfix.data(), n_lat * sizeof(unsigned long long), hipMemcpyHostToDevice, s));
    QD_HIP(c, hipMemcpyAsync(d_sel, sel0, sizeof(sel0), hipMemcpyHostToDevice, s));
    QD_HIP(c, hipMemsetAsync(d_hw, 0, TG_BINS * sizeof(unsigned long long), s));
    QD_HIP(c, hipMemsetAsync(d_hc, 0, TG_BINS * sizeof(unsigned int), s));
    QD_HIP(c, hipStreamSynchronize(s));           // the host arrays above go out of scope; the events time kernels only
    QD_HIP(c, hipEventCreate(&ev0));
    if (hipEventCreate(&ev1) != hipSuccess) { hipEventDestroy(ev0); return qd_fail(c, "qd_topogen_build: hipEventCreate"); }
    hipEventRecord(ev0, s);

    const int lds = TG_LDS_MAX;
    const dim3 g1((N + QD_BLOCK - 1) / QD_BLOCK), g2((n_lon + QD_BLOCK - 1) / QD_BLOCK, n_lat), blk(QD_BLOCK);
    auto smooth = [&](int f, const double* in, double* out) {
        tg_pass(c, true, in, d_tmp, n_lat, n_lon, d_w + woff[2 * f], radii[2 * f], lds);
        tg_pass(c, false, d_tmp, out, n_lat, n_lon, d_w + woff[2 * f + 1], radii[2 * f + 1], lds);
    };
    double* st = d_stat; const double* st_id = d_stat + 12; double* d_sea = d_stat + 14;
    // L1: continents, normalised; the VLF field, normalised; their blend (topography.py:148-170)
    hipLaunchKernelGGL(k_tg_continents, g2, blk, 0, s, n_lat, n_lon, n_cont, (const double*)d_cont, (const double*)d_cl,
                       (const double*)d_sinlat, (const double*)d_coslat, par[0], par[1], d_h1);
    tg_stats(c, d_h1, N, d_part, st + 0);
    smooth(0, d_noise, d_sm);
    tg_stats(c, d_sm, N, d_part, st + 2);
    hipLaunchKernelGGL(k_tg_lin, g1, blk, 0, s, N, par[2], (const double*)d_h1, (const double*)(st + 0), par[3], (const double*)d_sm,
                       (const double*)(st + 2), d_h1);
    tg_stats(c, d_h1, N, d_part, st + 4);
    // L3: fbm += amp * normalised octave (:192-202)
    hipMemsetAsync(d_fbm, 0, cells * sizeof(double), s);
    for (int o = 0; o < n_oct; ++o) {
        smooth(1 + o, d_noise + (size_t)(1 + o) * cells, d_sm);
        tg_stats(c, d_sm, N, d_part, st + 6);
        hipLaunchKernelGGL(k_tg_lin, g1, blk, 0, s, N, 1.0, (const double*)d_fbm, st_id, oct_amp[o], (const double*)d_sm,
                           (const double*)(st + 6), d_fbm);
    }
    tg_stats(c, d_fbm, N, d_part, st + 8);
    // W1 * H_l1 + W3 * H_l3, normalised and scaled, the last gentle filter (:237-245)
    hipLaunchKernelGGL(k_tg_lin, g1, blk, 0, s, N, par[4], (const double*)d_h1, (const double*)(st + 4), par[5], (const double*)d_fbm,
                       (const double*)(st + 8), d_sm);
    tg_stats(c, d_sm, N, d_part, st + 10);
    hipLaunchKernelGGL(k_tg_lin, g1, blk, 0, s, N, par[6], (const double*)d_sm, (const double*)(st + 10), 0.0, (const double*)nullptr,
                       (const double*)nullptr, d_h1);
    double* d_elev = d_fbm;
    smooth(nfilt - 1, d_h1, d_elev);
    // sea level and mask (:58-83, :262-271)
    const int nb = tg_nb(N);
    for (int shift = 56; shift >= 0; shift -= 8) {
        hipLaunchKernelGGL(k_tg_hist, dim3(nb), blk, 0, s, (const double*)d_elev, N, n_lon, nb, (const unsigned long long*)d_wfix,
                           (const unsigned long long*)d_sel, shift, d_hw, d_hc);
        hipLaunchKernelGGL(k_tg_pick, dim3(1), dim3(TG_BINS), 0, s, d_hw, d_hc, d_sel, shift, d_sea);
    }
    hipLaunchKernelGGL(k_tg_mask, g1, blk, 0, s, (const double*)d_elev, N, (const double*)d_sea, d_mask);
    hipEventRecord(ev1, s);
    hipError_t e = hipMemcpyAsync(elevation, d_elev, cells * sizeof(double), hipMemcpyDeviceToHost, s);
    if (e == hipSuccess) e = hipMemcpyAsync(land_mask, d_mask, cells, hipMemcpyDeviceToHost, s);
    double sea = 0.0;
    if (e == hipSuccess) e = hipMemcpyAsync(&sea, d_sea, sizeof(double), hipMemcpyDeviceToHost, s);
    if (e == hipSuccess) e = hipStreamSynchronize(s);
    if (e == hipSuccess) e = hipGetLastError();
    float ms = -1.0f;
    if (e == hipSuccess) e = hipEventElapsedTime(&ms, ev0, ev1);
    hipEventDestroy(ev0);
    hipEventDestroy(ev1);
    if (e != hipSuccess) return qd_fail(c, "qd_topogen_build: kernel", e);
    if (!std::isfinite(sea) || !tg_finite(elevation, cells))
        return qd_fail(c, "qd_topogen_build: the elevation came out non-finite (the inputs overflow the normalisations)");
    *sea_level_m = sea;
    c->topogen_ms = (double)ms;
    return 0;
}

extern "C" int qd_topogen_last_ms(qd_handle c, double* ms) {
    if (!c || !ms) return -1;
    if (c->topogen_ms < 0.0) return qd_fail(c, "qd_topogen_last_ms: no topography built on this handle");
    *ms = c->topogen_ms;
    return 0;
}
