// qd_spharm.hip -- spherical-harmonic power spectra: the coefficients x_n^m of selected fields up to a triangular truncation N,
// their power per total wavenumber n, one record per sampled step, as a span lane, gfx950 (QD_SPHARM).
//
// The definition is qingdai_amd/spharm.py (analyse_reference): rows j = 0 .. L = n_lat - 1 at mu_j = sin(-pi / 2 + j pi / L), the
// Chebyshev extreme points, with Clenshaw-Curtis weights w_j -- exact quadrature for N = min((n_lat - 1) / 2, (n_lon - 1) / 2) --
//     X_j(m) = (1 / n) sum_i x[j][i] exp(-2 pi i im / n)        x_n^m = (1 / 2) sum_j w_j Pbar_n^m(mu_j) X_j(m)
//     Pbar_n^m = A_n^m (mu Pbar_{n-1}^m - B_n^m Pbar_{n-2}^m) from the seed Pbar_m^m and Pbar_{m-1}^m = 0
//     P(n) = sum_{m <= n} c_m |x_n^m|^2 (c_0 = 1, else 2)       ms = (1 / 2) sum_j w_j mean_i x[j][i]^2
// w, mu, the seeds and A, B [m][n] are the host's tables (extended precision, rounded once); the recurrence runs in f64 here.  An
// entry is a history entry (qd_entry.h) or VORT / DIV: the flow lane's zeta, delta of the resident (U, V), made by the flow lane's
// own kernel (qd_flow_vortdiv_launch) into two planes of this lane.  Per sampling position:
//   k_flow_vortdiv     when VORT or DIV is selected (qd_flow.hip)
//   k_spharm_rows      ONE workgroup of QD_BLOCK threads per (entry, row): the row staged in LDS, transformed as the complex sequence
//                      x + 0 i of length n by the Stockham passes of qd_rowfft.h (n = 2^a 3^b 5^c), or by direct sums for any other n
//                      and under QD_SPHARM_FORM=direct (thread m adds x[i] cos / sin(2 pi ((i m) mod n) / n) for i ascending); the
//                      bins 0 .. N divided by n and stored m-major, [entry][Re | Im][m][j], so the next stage reads along j.  Wave 0
//                      takes ms_j = (sum_i x^2) / n in the lane order of the series and flow lanes (lane l owns the cells
//                      128 k + 2 l and 128 k + 2 l + 1, ascending from +0.0, then the five halvings of qd_blockred.h).  A row that
//                      holds a non-finite value is NaN in every bin and in ms_j, and is flagged.
//   k_spharm_leg<NP>   the Legendre stage, ONE wave (a workgroup of 64) per (entry, m), no LDS, no barrier.  Lane l owns the
//                      latitude pairs (p, L - p), p = l, l + 64, ... (NP of them, in registers): mu_p, Pbar_{n-1}, Pbar_{n-2} and the
//                      symmetric / antisymmetric sums E = w_p (X_p + X_{L-p}), O = w_p (X_p - X_{L-p}), Re and Im; the equator row of
//                      an odd n_lat is taken once, E = w X, O = 0.  Pbar_n^m(-mu) = (-1)^(n+m) Pbar_n^m(mu), so the walk n = m .. N
//                      touches each pair once: acc = acc + Pbar E for n - m even, Pbar O for n - m odd, pairs in ascending p from
//                      +0.0, then the five halvings, and x_n^m = 0.5 acc.  A_n^m and B_n^m are wave-uniform loads.  NP is 2, 6 or 12
//                      (n_lat <= 255, 767, 1535 = QD_SPHARM_MAX_LAT): a pair past the end holds zeros and adds +0.0.  A plane with a
//                      flagged row gives NaN in every coefficient.
//   k_spharm_record    one workgroup per entry: thread n adds c_m (re re + im im) for m = 0 .. n ascending from +0.0 -> P(n), and with
//                      two_d sum[n][m] = sum[n][m] + term; wave 0: lane l takes the rows l, l + 64, ... ascending, acc = acc + w_j
//                      ms_j, the five halvings, ms = 0.5 acc; wave 1 counts the flagged rows likewise.
// The Legendre form built is the plain one of the lane's design: at 721 rows a lane holds 6 pairs, at 1441 rows 12.  Neither of
// the two heavier candidates -- the pairs of one m split over the waves of a workgroup with an LDS combine, or m paired with
// N - m to even out the trip counts -- was built: at T360 and the default three entries the stage takes the time DESIGN.md
// section 7 states, next to the other lanes' samples, at the default cadence of one sample in 24 steps, and it keeps the project's
// habit of one wave per unit of work without LDS or barriers.  A Pbar table is not the way (about 190 MB at T360).
// No atomics, no scratch: the same planes give the same bits, run after run.  spharm.power_reference restates k_spharm_record bit
// for bit.  Whole-globe handles only; qd_spharm_analyse_grid runs the same kernels without a handle.
#include "qd_span.h"
#include "qd_entry.h"
#include "qd_blockred.h"
#include "qd_rowfft.h"
#include <algorithm>
#include <cmath>
#include <cstdlib>
#include <cstring>

#define QH_LDS_LIMIT (150 * 1024)     // bytes of the CU's 160 KB LDS one workgroup may take here (k_spectra_rows' limit)
#define QH_NSTAT 2                    // ms and the bad-row count behind an entry's powers (include/qingdai_hip.h: QD_SPHARM_STATS)
#define QH_FLOW_ROWSTAT 8             // row partials k_flow_vortdiv writes (qd_flow.hip: QF_NROW1)
#define QH_FINITE(x) (fabs(x) <= 1.7976931348623157e308)
static_assert(QD_SPHARM_MAX_ENTRIES == QD_ENTRY_MAX, "the spharm table is the shared entry table");
static_assert(QD_SPHARM_STATS == QH_NSTAT, "the record's trailing statistics");
static_assert(QD_SPHARM_MAX_LAT == 2 * 12 * 64 - 1, "k_spharm_leg<12>: 768 latitude pairs");

struct QdShGrid {
    int nlat, nlon, N, npairs;
    const double *w, *mu, *seed, *A, *B, *tw;      // [nlat], [nlat], [N + 1][npairs], [N + 1][N + 1] x 2, [2][nlon]
};
struct QdShEntry { const double* a; const double* b; int slot; int pad_; };            // b == nullptr: op 0; slot: the entry's place in the record
struct QdShTab { QdShEntry e[QD_ENTRY_MAX]; int n; };

// ------------------------------------------------------------------ the row stage
// FORM 0: fft, dynamic LDS 8 + 32 (QS_SK(n) + 1) bytes; 1: direct, 8 + 24 n bytes.  spec: [slot][Re | Im][N + 1][nlat]
template <int FORM>
__global__ void __launch_bounds__(QD_BLOCK)
k_spharm_rows(QdShTab T, QdSpecPlan F, QdShGrid G, double* __restrict__ spec, double* __restrict__ rowms, double* __restrict__ rowbad) {
    extern __shared__ double qh_lds[];
    int* flag = reinterpret_cast<int*>(qh_lds);
    const int nlat = G.nlat, n = G.nlon, N1 = G.N + 1;
    const int q = blockIdx.x / nlat, j = blockIdx.x - q * nlat, lane = threadIdx.x & 63, wv = threadIdx.x >> 6;
    const QdShEntry E = T.e[q];
    const bool pair = E.b != nullptr;
    const size_t row = (size_t)j * n;
    const double* pa = E.a + row;
    const double* pb = pair ? E.b + row : pa;
    if (threadIdx.x == 0) *flag = 0;
    __syncthreads();
    const int mp = QS_SK(n) + 1;
    double* Ar = qh_lds + 1; double* Ai = Ar + mp; double* Br = Ai + mp; double* Bi = Br + mp;      // fft
    double* x = qh_lds + 1; double* tc = x + n; double* ts = tc + n;                                // direct
    int nonfinite = 0;
    for (int t = threadIdx.x; t < n; t += QD_BLOCK) {
        const double x0 = hist_value(pa[t], pb[t], pair);
        nonfinite |= !QH_FINITE(x0) ? 1 : 0;
        if (FORM == 0) qs_st(Ar, Ai, t, {x0, 0.0});
        else { x[t] = x0; tc[t] = G.tw[t]; ts[t] = G.tw[n + t]; }
    }
    if (nonfinite) *flag = 1;                               // (every writer stores the same value)
    __syncthreads();
    const bool isbad = *flag != 0;                          // workgroup-uniform
    if (wv == 0) {                                          // ms_j, before any pass overwrites the staged row (the first pass only reads it)
        double acc = 0.0;
        for (int i = 2 * lane; i < n; i += 128) {
            const double v0 = FORM == 0 ? Ar[QS_SK(i)] : x[i];
            acc = acc + v0 * v0;
            if (i + 1 < n) { const double v1 = FORM == 0 ? Ar[QS_SK(i + 1)] : x[i + 1]; acc = acc + v1 * v1; }
        }
        acc = qd_wave_sum(acc);
        if (lane == 0) {
            rowms[(size_t)E.slot * nlat + j] = isbad ? NAN : acc / (double)n;
            rowbad[(size_t)E.slot * nlat + j] = isbad ? 1.0 : 0.0;
        }
    }
    double* SR = spec + ((size_t)(2 * E.slot) * N1) * nlat + j;
    double* SI = SR + (size_t)N1 * nlat;
    const double dn = (double)n;
    if (FORM == 0) {
        double *Xr, *Xi, *Yr, *Yi;
        qs_run(F, n, G.tw, Ar, Ai, Br, Bi, &Xr, &Xi, &Yr, &Yi);
        for (int m = threadIdx.x; m < N1; m += QD_BLOCK) {
            const qs_cx y = qs_ld(Xr, Xi, m);
            SR[(size_t)m * nlat] = isbad ? NAN : y.r / dn;
            SI[(size_t)m * nlat] = isbad ? NAN : y.i / dn;
        }
    } else {
        for (int m = threadIdx.x; m < N1; m += QD_BLOCK) {
            double ar = 0.0, ai = 0.0;
            int idx = 0;
            for (int i = 0; i < n; ++i) {
                const double v = x[i];
                ar += v * tc[idx];
                ai -= v * ts[idx];
                idx += m; if (idx >= n) idx -= n;
            }
            SR[(size_t)m * nlat] = isbad ? NAN : ar / dn;
            SI[(size_t)m * nlat] = isbad ? NAN : ai / dn;
        }
    }
}

// ------------------------------------------------------------------ the Legendre stage
template <int NP>
__device__ __forceinline__ void qh_advance(double a, double b, const double (&mu)[NP], double (&p1)[NP], double (&p2)[NP]) {
#pragma unroll
    for (int k = 0; k < NP; ++k) { const double p = a * (mu[k] * p1[k] - b * p2[k]); p2[k] = p1[k]; p1[k] = p; }
}
template <int NP>
__device__ __forceinline__ void qh_emit(const double (&p)[NP], const double (&sr)[NP], const double (&si)[NP], int lane, double* cr, double* ci) {
    double ar = 0.0, ai = 0.0;
#pragma unroll
    for (int k = 0; k < NP; ++k) { ar = ar + p[k] * sr[k]; ai = ai + p[k] * si[k]; }
    ar = qd_wave_sum(ar); ai = qd_wave_sum(ai);
    if (lane == 0) { *cr = 0.5 * ar; *ci = 0.5 * ai; }
}

// coef: [slot][Re | Im][N + 1 (m)][N + 1 (n)]
template <int NP>
__global__ void __launch_bounds__(64)
k_spharm_leg(QdShTab T, QdShGrid G, const double* __restrict__ spec, const double* __restrict__ rowbad, double* __restrict__ coef) {
    const int N = G.N, N1 = N + 1, nlat = G.nlat, L = nlat - 1, lane = threadIdx.x;
    const int q = blockIdx.x / N1, m = blockIdx.x - q * N1, slot = T.e[q].slot;
    const double* XR = spec + ((size_t)(2 * slot) * N1 + m) * nlat;
    const double* XI = XR + (size_t)N1 * nlat;
    const double* BAD = rowbad + (size_t)slot * nlat;
    double* CR = coef + ((size_t)(2 * slot) * N1 + m) * N1;
    double* CI = CR + (size_t)N1 * N1;
    double mu[NP], p1[NP], p2[NP], er[NP], ei[NP], orr[NP], oi[NP];
    int bad = 0;
#pragma unroll
    for (int k = 0; k < NP; ++k) {
        const int p = lane + 64 * k;
        mu[k] = p1[k] = p2[k] = er[k] = ei[k] = orr[k] = oi[k] = 0.0;
        if (p < G.npairs) {
            const int jn = L - p;
            const double w = G.w[p], ar = XR[p], ai = XI[p];
            mu[k] = G.mu[p];
            p1[k] = G.seed[(size_t)m * G.npairs + p];
            bad |= (BAD[p] != 0.0 || BAD[jn] != 0.0) ? 1 : 0;
            if (jn == p) { er[k] = w * ar; ei[k] = w * ai; }                  // the equator row: once, in the even part only
            else {
                const double br = XR[jn], bi = XI[jn];
                er[k] = w * (ar + br); ei[k] = w * (ai + bi);
                orr[k] = w * (ar - br); oi[k] = w * (ai - bi);
            }
        }
    }
    if (__any(bad)) {                                       // wave-uniform: the transform couples every cell
        for (int n = lane; n < N1; n += 64) { CR[n] = NAN; CI[n] = NAN; }
        return;
    }
    for (int n = lane; n < m; n += 64) { CR[n] = 0.0; CI[n] = 0.0; }
    const double* Am = G.A + (size_t)m * N1;
    const double* Bm = G.B + (size_t)m * N1;
    qh_emit<NP>(p1, er, ei, lane, CR + m, CI + m);
    int n = m + 1;
    for (; n + 1 <= N; n += 2) {
        qh_advance<NP>(Am[n], Bm[n], mu, p1, p2);
        qh_emit<NP>(p1, orr, oi, lane, CR + n, CI + n);
        qh_advance<NP>(Am[n + 1], Bm[n + 1], mu, p1, p2);
        qh_emit<NP>(p1, er, ei, lane, CR + n + 1, CI + n + 1);
    }
    if (n <= N) {
        qh_advance<NP>(Am[n], Bm[n], mu, p1, p2);
        qh_emit<NP>(p1, orr, oi, lane, CR + n, CI + n);
    }
}

// ------------------------------------------------------------------ power, mean square, bad rows, the 2D sums
// one workgroup per entry; rec: the record in progress; sums: [slot][N + 1 (n)][N + 1 (m)] or nullptr
__global__ void __launch_bounds__(QD_BLOCK)
k_spharm_record(QdShTab T, QdShGrid G, const double* __restrict__ coef, const double* __restrict__ rowms, const double* __restrict__ rowbad,
                double* __restrict__ rec, double* __restrict__ sums) {
    const int N1 = G.N + 1, nlat = G.nlat, slot = T.e[blockIdx.x].slot, lane = threadIdx.x & 63, wv = threadIdx.x >> 6;
    const double* CR = coef + (size_t)(2 * slot) * N1 * N1;
    const double* CI = CR + (size_t)N1 * N1;
    double* out = rec + (size_t)slot * (N1 + QH_NSTAT);
    double* S = sums ? sums + (size_t)slot * N1 * N1 : nullptr;
    for (int n = threadIdx.x; n < N1; n += QD_BLOCK) {
        double acc = 0.0;
        for (int m = 0; m <= n; ++m) {
            const double re = CR[(size_t)m * N1 + n], im = CI[(size_t)m * N1 + n];
            const double t = (m == 0 ? 1.0 : 2.0) * (re * re + im * im);
            acc = acc + t;
            if (S) S[(size_t)n * N1 + m] = S[(size_t)n * N1 + m] + t;
        }
        out[n] = acc;
    }
    if (wv == 0) {
        double acc = 0.0;
        for (int j = lane; j < nlat; j += 64) acc = acc + G.w[j] * rowms[(size_t)slot * nlat + j];
        acc = qd_wave_sum(acc);
        if (lane == 0) out[N1] = 0.5 * acc;
    } else if (wv == 1) {
        double acc = 0.0;
        for (int j = lane; j < nlat; j += 64) acc = acc + rowbad[(size_t)slot * nlat + j];
        acc = qd_wave_sum(acc);
        if (lane == 0) out[N1 + 1] = acc;
    }
}

// ------------------------------------------------------------------ host side
enum { QH_KIND_FIELD = 0, QH_KIND_VORT, QH_KIND_DIV };

struct QdSpharm {
    int nlat = 0, nlon = 0, N = 0, npairs = 0, np = 0, direct = 0, two_d = 0;
    int n = 0;                        // entries
    int kind[QD_ENTRY_MAX];           // QH_KIND_* per entry
    QdEntrySel sel;                   // the field entries' table, at the entries' own places (VORT / DIV places hold a = U: never read)
    bool uses_flow = false;
    QdSpecPlan plan{};
    size_t lds = 0;                   // dynamic LDS of k_spharm_rows
    double* tabs = nullptr;           // w | mu | seed | A | B | tw, one allocation
    QdShGrid G{};
    double* spec = nullptr;           // [n][2][N + 1][nlat]
    double* coef = nullptr;           // [n][2][N + 1][N + 1]
    double* rows = nullptr;           // ms_j [n][nlat], bad_j [n][nlat], then a record outside the log [N + 1 + QH_NSTAT]
    double* sums = nullptr;           // [n][N + 1][N + 1] (two_d)
    double* ftab = nullptr;           // the flow lane's grid table [QD_FLOW_TAB][nlat], Z and D [2][nlat][nlon], its row partials
    double fgeom[3] = {0, 0, 0};
    double* hplane = nullptr;         // [nlat][nlon] the host plane of qd_spharm_analyse, allocated at its first call
    int64_t count = 0;                // samples in the sums
    double* rec = nullptr;            // the record of the step in progress
    QdSpanLane lane;
    int N1() const { return N + 1; }
    size_t cells() const { return (size_t)nlat * nlon; }
    size_t sum_doubles() const { return (size_t)n * N1() * N1(); }
    double* rowms() const { return rows; }
    double* rowbad() const { return rows + (size_t)n * nlat; }
    double* rec_out() const { return rows + 2 * (size_t)n * nlat; }
    double* Z() const { return ftab + (size_t)QD_FLOW_TAB * nlat; }
    double* D() const { return Z() + cells(); }
    double* fstat() const { return D() + cells(); }
};

static QdSpanLane* spharm_lane(qd_ctx* c) { return c && c->spharm ? &c->spharm->lane : nullptr; }

static void spharm_free(QdSpharm* s) {
    void* p[] = {s->tabs, s->spec, s->coef, s->rows, s->sums, s->ftab, s->hplane, s->lane.log};
    for (void* q : p) if (q) hipFree(q);
    delete s;
}

void qd_spharm_release(qd_ctx* c) {
    if (!c->spharm) return;
    if (c->stream) hipStreamSynchronize(c->stream);
    spharm_free(c->spharm);
    c->spharm = nullptr;
}

struct QdShHostTables { const double *w, *mu, *seed, *A, *B, *flow_tab, *flow_geom; };

// -> the tables and work planes of t (its entry table filled in) on the current device, or nullptr with *why set; with_lane: the
// log and, with two_d, the sum planes too
static QdSpharm* spharm_build(const QdSpharm& t, int nlat, int nlon, int trunc, const QdShHostTables& H, bool with_lane, hipStream_t st,
                              std::string* why) {
    const int N = std::min((nlat - 1) / 2, (nlon - 1) / 2);
    if (N < 1 || trunc != N) {
        *why = "a grid of " + std::to_string(nlat) + " x " + std::to_string(nlon) + " has the truncation N = " + std::to_string(N) +
               (N < 1 ? "; N >= 1 is needed" : ", the tables are for N = " + std::to_string(trunc));
        return nullptr;
    }
    if (nlat > QD_SPHARM_MAX_LAT) {
        *why = "n_lat = " + std::to_string(nlat) + ": the Legendre kernel takes at most QD_SPHARM_MAX_LAT = " + std::to_string(QD_SPHARM_MAX_LAT) + " rows";
        return nullptr;
    }
    QdSpharm* s = new QdSpharm(t);
    s->nlat = nlat; s->nlon = nlon; s->N = N; s->npairs = (nlat + 1) / 2;
    const int per_lane = (s->npairs + 63) / 64;
    s->np = per_lane <= 2 ? 2 : (per_lane <= 6 ? 6 : 12);
    const char* form = std::getenv("QD_SPHARM_FORM");                 // read here, once, never on the step path
    s->direct = (form && std::strcmp(form, "direct") == 0) || !qd_rowfft_plan(nlon, 1, s->plan) ? 1 : 0;
    s->lds = sizeof(double) * (s->direct ? 1 + 3 * (size_t)nlon : 1 + 4 * (size_t)(QS_SK(nlon) + 1));
    const size_t flow_lds = s->uses_flow ? 3 * (size_t)nlon * sizeof(double) : 0;
    if (std::max(s->lds, flow_lds) > QH_LDS_LIMIT) {
        *why = "a row of n_lon = " + std::to_string(nlon) + " needs " + std::to_string(std::max(s->lds, flow_lds)) +
               " bytes of LDS, a workgroup may take " + std::to_string(QH_LDS_LIMIT) + " of the CU's 163840";
        delete s;
        return nullptr;
    }
    const int N1 = N + 1, n = s->n;
    s->lane.width = n * (N1 + QH_NSTAT);
    s->lane.cap = QD_SPHARM_LOG_CAP;
    const std::vector<double> tw = qd_rowfft_table(nlon);
    // the tables, one allocation: w | mu | seed | A | B | tw
    const size_t o_mu = nlat, o_seed = o_mu + nlat, o_A = o_seed + (size_t)N1 * s->npairs, o_B = o_A + (size_t)N1 * N1, o_tw = o_B + (size_t)N1 * N1,
                 tabd = o_tw + tw.size();
    std::vector<double> host(tabd);
    std::memcpy(host.data(), H.w, nlat * sizeof(double));
    std::memcpy(host.data() + o_mu, H.mu, nlat * sizeof(double));
    std::memcpy(host.data() + o_seed, H.seed, (size_t)N1 * s->npairs * sizeof(double));
    std::memcpy(host.data() + o_A, H.A, (size_t)N1 * N1 * sizeof(double));
    std::memcpy(host.data() + o_B, H.B, (size_t)N1 * N1 * sizeof(double));
    std::memcpy(host.data() + o_tw, tw.data(), tw.size() * sizeof(double));
    const size_t cells = s->cells();
    const size_t tabb = tabd * sizeof(double), specb = (size_t)n * 2 * N1 * nlat * sizeof(double), coefb = (size_t)n * 2 * N1 * N1 * sizeof(double),
                 rowsb = (2 * (size_t)n * nlat + N1 + QH_NSTAT) * sizeof(double), sumb = s->sum_doubles() * sizeof(double),
                 logb = s->lane.log_doubles() * sizeof(double),
                 ftabd = (size_t)QD_FLOW_TAB * nlat, flowb = (ftabd + 2 * cells + (size_t)QH_FLOW_ROWSTAT * nlat) * sizeof(double);
    bool ok = hipMalloc(&s->tabs, tabb) == hipSuccess && hipMalloc(&s->spec, specb) == hipSuccess && hipMalloc(&s->coef, coefb) == hipSuccess &&
              hipMalloc(&s->rows, rowsb) == hipSuccess && (!s->uses_flow || hipMalloc(&s->ftab, flowb) == hipSuccess) &&
              (!with_lane || hipMalloc(&s->lane.log, logb) == hipSuccess) && (!(with_lane && s->two_d) || hipMalloc(&s->sums, sumb) == hipSuccess);
    ok = ok && hipMemcpyAsync(s->tabs, host.data(), tabb, hipMemcpyHostToDevice, st) == hipSuccess &&
         hipMemsetAsync(s->spec, 0, specb, st) == hipSuccess && hipMemsetAsync(s->coef, 0, coefb, st) == hipSuccess &&
         hipMemsetAsync(s->rows, 0, rowsb, st) == hipSuccess &&
         (!s->uses_flow || (hipMemsetAsync(s->ftab, 0, flowb, st) == hipSuccess &&
                            hipMemcpyAsync(s->ftab, H.flow_tab, ftabd * sizeof(double), hipMemcpyHostToDevice, st) == hipSuccess)) &&
         (!s->lane.log || hipMemsetAsync(s->lane.log, 0, logb, st) == hipSuccess) &&
         (!s->sums || hipMemsetAsync(s->sums, 0, sumb, st) == hipSuccess) && hipStreamSynchronize(st) == hipSuccess;      // (host tables are only borrowed)
    if (s->uses_flow) std::memcpy(s->fgeom, H.flow_geom, sizeof s->fgeom);
    // a workgroup may take more than the default 64 KB of dynamic LDS (k_spectra_rows does the same)
    ok = ok && hipFuncSetAttribute((const void*)k_spharm_rows<0>, hipFuncAttributeMaxDynamicSharedMemorySize, QH_LDS_LIMIT) == hipSuccess &&
         hipFuncSetAttribute((const void*)k_spharm_rows<1>, hipFuncAttributeMaxDynamicSharedMemorySize, QH_LDS_LIMIT) == hipSuccess &&
         (!s->uses_flow || qd_flow_vortdiv_prepare(QH_LDS_LIMIT));
    if (!ok) { *why = "device allocation or upload failed"; spharm_free(s); return nullptr; }
    s->G = QdShGrid{nlat, nlon, N, s->npairs, s->tabs, s->tabs + o_mu, s->tabs + o_seed, s->tabs + o_A, s->tabs + o_B, s->tabs + o_tw};
    return s;
}

// QD_LAUNCH_TIMED with dynamic LDS and a block size, and without a handle (c == nullptr) a plain launch
#define QH_LAUNCH(c, name, kernel, grid, block, lds, stream, ...) do { \
    if (c) { QdScope sc(c, name, true); \
        if (sc.on) { sc.used = true; hipExtLaunchKernelGGL((kernel), grid, block, lds, stream, sc.e0, sc.e1, 0, __VA_ARGS__); } \
        else hipLaunchKernelGGL((kernel), grid, block, lds, stream, __VA_ARGS__); } \
    else hipLaunchKernelGGL((kernel), grid, block, lds, stream, __VA_ARGS__); } while (0)

// the three launches of a sampling position on the entries of T; rec: where the record goes; sums: the sum planes or nullptr
static void spharm_run(QdSpharm* s, qd_ctx* c, hipStream_t st, const QdShTab& T, double* rec, double* sums) {
    const QdShGrid G = s->G;
    const dim3 rows(T.n * s->nlat), waves(T.n * s->N1());
    if (s->direct) QH_LAUNCH(c, "spharm_rows", k_spharm_rows<1>, rows, dim3(QD_BLOCK), s->lds, st, T, s->plan, G, s->spec, s->rowms(), s->rowbad());
    else QH_LAUNCH(c, "spharm_rows", k_spharm_rows<0>, rows, dim3(QD_BLOCK), s->lds, st, T, s->plan, G, s->spec, s->rowms(), s->rowbad());
    if (s->np == 2) QH_LAUNCH(c, "spharm_leg", k_spharm_leg<2>, waves, dim3(64), 0, st, T, G, (const double*)s->spec, (const double*)s->rowbad(), s->coef);
    else if (s->np == 6) QH_LAUNCH(c, "spharm_leg", k_spharm_leg<6>, waves, dim3(64), 0, st, T, G, (const double*)s->spec, (const double*)s->rowbad(), s->coef);
    else QH_LAUNCH(c, "spharm_leg", k_spharm_leg<12>, waves, dim3(64), 0, st, T, G, (const double*)s->spec, (const double*)s->rowbad(), s->coef);
    QH_LAUNCH(c, "spharm_record", k_spharm_record, dim3(T.n), dim3(QD_BLOCK), 0, st, T, G, (const double*)s->coef, (const double*)s->rowms(),
              (const double*)s->rowbad(), rec, sums);
}

static void spharm_tab_clear(QdShTab& T) {
    T.n = 0;
    for (int k = 0; k < QD_ENTRY_MAX; ++k) T.e[k] = QdShEntry{nullptr, nullptr, 0, 0};
}

extern "C" int qd_spharm_configure(qd_handle c, int n, const int32_t* op, const int32_t* a, const int32_t* b, int two_d, int trunc, const double* w,
                                   const double* mu, const double* seed, const double* A, const double* B, const double* flow_tab,
                                   const double* flow_geom) {
    if (!c || n < 0) return -1;
    if (n == 0 || !w) n = 0;
    if (n && (!op || !a || !mu || !seed || !A || !B)) return -1;
    if (!qd_whole_globe(c))
        return qd_fail(c, "qd_spharm_configure: the spherical-harmonic spectra need a whole-globe handle (world == 1, n_rows == n_lat); "
                          "latitude bands are not supported");
    if (n > QD_ENTRY_MAX) return qd_fail(c, "qd_spharm_configure: at most 32 entries");
    QdSpharm t;
    // the field entries go through the shared parser at their own places; a VORT / DIV place holds the plane U there, which is never read
    int32_t fop[QD_ENTRY_MAX], fa[QD_ENTRY_MAX], fb[QD_ENTRY_MAX];
    for (int k = 0; k < n; ++k) {
        const bool own = op[k] == QD_SPHARM_OP_VORT || op[k] == QD_SPHARM_OP_DIV;
        t.kind[k] = op[k] == QD_SPHARM_OP_VORT ? QH_KIND_VORT : (op[k] == QD_SPHARM_OP_DIV ? QH_KIND_DIV : QH_KIND_FIELD);
        t.uses_flow = t.uses_flow || own;
        fop[k] = own ? 0 : op[k]; fa[k] = own ? QD_F_U : a[k]; fb[k] = own || !b ? -1 : b[k];
    }
    if (qd_entries_parse(c, "qd_spharm_configure", n, fop, fa, b ? fb : nullptr, t.sel)) return -1;
    if (t.uses_flow && (!flow_tab || !flow_geom))
        return qd_fail(c, "qd_spharm_configure: a VORT or DIV entry needs the flow lane's grid table and geometry");
    hipSetDevice(c->desc.device);
    qd_spharm_release(c);
    if (n == 0) return 0;
    t.n = n; t.two_d = two_d ? 1 : 0;
    std::string why;
    const QdShHostTables H{w, mu, seed, A, B, flow_tab, flow_geom};
    QdSpharm* s = spharm_build(t, c->geo.nlat, c->geo.nlon, trunc, H, true, c->stream, &why);
    if (!s) return qd_fail(c, ("qd_spharm_configure: " + why).c_str());
    c->spharm = s;
    return 0;
}

extern "C" int qd_spharm_schedule(qd_handle c, int steps, const int32_t* sample) {
    return qd_lane_schedule(c, spharm_lane(c), steps, sample, "qd_spharm_schedule", "not configured (qd_spharm_configure first)");
}
extern "C" int qd_spharm_log(qd_handle c, double* out, int max, int* n) {
    return qd_lane_drain(c, spharm_lane(c), out, max, n, "qd_spharm_log", "not configured (qd_spharm_configure first)");
}
extern "C" int qd_spharm_reset(qd_handle c) {
    if (!c) return -1;
    QdSpharm* s = c->spharm;
    if (!s) return qd_fail(c, "qd_spharm_reset: not configured (qd_spharm_configure first)");
    hipSetDevice(c->desc.device);
    if (s->sums) QD_HIP(c, hipMemsetAsync(s->sums, 0, s->sum_doubles() * sizeof(double), c->stream));
    s->count = 0;
    s->lane.reset();
    return 0;
}

extern "C" int qd_spharm_sums_get(qd_handle c, double* sums, int64_t* count) {
    if (!c || !count) return -1;
    QdSpharm* s = c->spharm;
    if (!s) return qd_fail(c, "qd_spharm_sums_get: not configured (qd_spharm_configure first)");
    if (!s->sums) return qd_fail(c, "qd_spharm_sums_get: the configuration keeps no 2D sums");
    if (!sums) return -1;
    hipSetDevice(c->desc.device);
    QD_HIP(c, hipMemcpyAsync(sums, s->sums, s->sum_doubles() * sizeof(double), hipMemcpyDeviceToHost, c->stream));
    QD_HIP(c, hipStreamSynchronize(c->stream));
    const hipError_t e = hipGetLastError();
    if (e != hipSuccess) return qd_fail(c, "qd_spharm_sums_get: kernel", e);
    *count = s->count;
    return 0;
}

extern "C" int qd_spharm_sums_set(qd_handle c, const double* sums, int64_t count) {
    if (!c) return -1;
    QdSpharm* s = c->spharm;
    if (!s) return qd_fail(c, "qd_spharm_sums_set: not configured (qd_spharm_configure first)");
    if (!s->sums) return qd_fail(c, "qd_spharm_sums_set: the configuration keeps no 2D sums");
    if (!sums) return -1;
    if (count < 0) return qd_fail(c, "qd_spharm_sums_set: negative sample count");
    hipSetDevice(c->desc.device);
    QD_HIP(c, hipMemcpyAsync(s->sums, sums, s->sum_doubles() * sizeof(double), hipMemcpyHostToDevice, c->stream));
    QD_HIP(c, hipStreamSynchronize(c->stream));                // the host buffer is only borrowed for the call
    s->count = count;
    return 0;
}

bool qd_spharm_planes(const qd_ctx* c, const double** sums, size_t* n) {
    const QdSpharm* s = c->spharm;
    if (!s || !s->sums) return false;
    *sums = s->sums; *n = s->sum_doubles();
    return true;
}

bool qd_spharm_scheduled(const qd_ctx* c) { return c->spharm && !c->spharm->lane.sched.empty(); }
bool qd_spharm_reads_lazy(const qd_ctx* c) { return c->spharm && c->spharm->sel.lazy; }

static bool spharm_stale(const QdSpharm* s, const qd_ctx* c) {
    for (int k = 0; k < s->n; ++k)
        if (s->kind[k] == QH_KIND_FIELD && (!hist_plane(c, s->sel.a[k]) || (s->sel.op[k] == 1 && !hist_plane(c, s->sel.b[k])))) return true;
    return false;
}

QdSpanLane* qd_spharm_span_begin(qd_ctx* c, int n) {
    static const QdSpanTexts T = {
        "qd_step_n: the spherical-harmonic spectra need a whole-globe handle; latitude bands are not supported",
        "qd_step_n: qd_spharm_configure has not been called",
        "qd_step_n: a qd_spharm_schedule must cover exactly the n steps of the span",
        "qd_step_n: the span's spharm records would overflow the log of QD_SPHARM_LOG_CAP (drain it with qd_spharm_log first)"};
    const bool stale = c->spharm && spharm_stale(c->spharm, c);
    QdSpanLane* l = qd_lane_span_begin(c, spharm_lane(c), n, T, nullptr,
                                       stale ? "qd_step_n: a spharm field is no longer an f64 plane (qd_spharm_configure again)" : nullptr);
    if (!l && c->spharm) c->spharm->lane.clear_schedule();        // refused: the span guard never sees this lane, and a schedule serves one span
    return l;
}

// a sampled step begins: its record slot, which the step's groups fill between them (every entry is in one of the two)
int qd_spharm_begin_step(qd_ctx* c) {
    QdSpharm* s = c->spharm;
    if (s->lane.full()) return qd_fail(c, "qd_step_n: spharm log full (drain it with qd_spharm_log)");
    s->rec = s->lane.next();
    return 0;
}

// group 0: the early entries, 1: the late entries (VORT and DIV among them; the sample count moves on with them), 2: all of them
int qd_spharm_transform(qd_ctx* c, int group) {
    QdSpharm* s = c->spharm;
    QdShTab T;
    spharm_tab_clear(T);
    bool flow = false;
    for (int k = 0; k < s->n; ++k) {
        const bool early = s->kind[k] == QH_KIND_FIELD && s->sel.early[k];
        if (group != 2 && early != (group == 0)) continue;
        if (s->kind[k] == QH_KIND_FIELD)
            T.e[T.n++] = QdShEntry{c->f[s->sel.a[k]], s->sel.op[k] == 1 ? c->f[s->sel.b[k]] : (const double*)nullptr, k, 0};
        else { T.e[T.n++] = QdShEntry{s->kind[k] == QH_KIND_VORT ? s->Z() : s->D(), nullptr, k, 0}; flow = true; }
    }
    if (group != 0) s->count++;
    if (T.n == 0) return 0;
    if (flow) qd_flow_vortdiv_launch(c, c->stream, s->nlat, s->nlon, s->ftab, s->fgeom, c->f[QD_F_U], c->f[QD_F_V], s->Z(), s->D(), s->fstat());
    spharm_run(s, c, c->stream, T, s->rec, s->sums);
    return 0;
}

extern "C" int qd_spharm_sample(qd_handle c) {
    if (!c) return -1;
    QdSpharm* s = c->spharm;
    if (!s) return qd_fail(c, "qd_spharm_sample: not configured (qd_spharm_configure first)");
    if (spharm_stale(s, c)) return qd_fail(c, "qd_spharm_sample: a spharm field is no longer an f64 plane (qd_spharm_configure again)");
    if (s->lane.full()) return qd_fail(c, "qd_spharm_sample: spharm log full (drain it with qd_spharm_log)");
    hipSetDevice(c->desc.device);
    s->rec = s->lane.next();
    if (int rc = qd_spharm_transform(c, 2)) return rc;
    return qd_launch_check(c, "qd_spharm_sample");
}

// upload the plane, run one entry in slot 0 of the work planes, download its coefficients and its record
static int spharm_analyse(QdSpharm* s, qd_ctx* c, hipStream_t st, const char* who, const double* plane, double* coef_re, double* coef_im,
                          double* rec) {
    const size_t pb = s->cells() * sizeof(double), cb = (size_t)s->N1() * s->N1() * sizeof(double);
    if (!s->hplane) QD_HIP(c, hipMalloc(&s->hplane, pb));
    QD_HIP(c, hipMemcpyAsync(s->hplane, plane, pb, hipMemcpyHostToDevice, st));
    QdShTab T;
    spharm_tab_clear(T);
    T.e[T.n++] = QdShEntry{s->hplane, nullptr, 0, 0};
    spharm_run(s, c, st, T, s->rec_out(), nullptr);
    const hipError_t le = hipGetLastError();
    if (le != hipSuccess) return qd_fail(c, (std::string(who) + ": launch").c_str(), le);
    QD_HIP(c, hipMemcpyAsync(coef_re, s->coef, cb, hipMemcpyDeviceToHost, st));
    QD_HIP(c, hipMemcpyAsync(coef_im, s->coef + (size_t)s->N1() * s->N1(), cb, hipMemcpyDeviceToHost, st));
    QD_HIP(c, hipMemcpyAsync(rec, s->rec_out(), (size_t)(s->N1() + QH_NSTAT) * sizeof(double), hipMemcpyDeviceToHost, st));
    QD_HIP(c, hipStreamSynchronize(st));
    const hipError_t e = hipGetLastError();
    if (e != hipSuccess) return qd_fail(c, (std::string(who) + ": kernel").c_str(), e);
    return 0;
}

extern "C" int qd_spharm_analyse(qd_handle c, const double* plane, double* coef_re, double* coef_im, double* rec) {
    if (!c || !plane || !coef_re || !coef_im || !rec) return -1;
    QdSpharm* s = c->spharm;
    if (!s) return qd_fail(c, "qd_spharm_analyse: not configured (qd_spharm_configure first)");
    hipSetDevice(c->desc.device);
    return spharm_analyse(s, c, c->stream, "qd_spharm_analyse", plane, coef_re, coef_im, rec);
}

extern "C" int qd_spharm_analyse_grid(int n_lat, int n_lon, int device, int trunc, const double* w, const double* mu, const double* seed,
                                      const double* A, const double* B, const double* plane, double* coef_re, double* coef_im, double* rec) {
    if (!w || !mu || !seed || !A || !B || !plane || !coef_re || !coef_im || !rec) return qd_fail(nullptr, "qd_spharm_analyse_grid: null argument");
    int ndev = 0;
    if (hipGetDeviceCount(&ndev) != hipSuccess || ndev == 0) return qd_fail(nullptr, "qd_spharm_analyse_grid: no HIP device visible");
    if (device < 0 || device >= ndev) return qd_fail(nullptr, "qd_spharm_analyse_grid: bad device ordinal");
    hipError_t e;
    if ((e = hipSetDevice(device)) != hipSuccess) return qd_fail(nullptr, "qd_spharm_analyse_grid: hipSetDevice", e);
    hipStream_t st = nullptr;
    if ((e = hipStreamCreate(&st)) != hipSuccess) return qd_fail(nullptr, "qd_spharm_analyse_grid: hipStreamCreate", e);
    QdSpharm t;
    t.n = 1; t.kind[0] = QH_KIND_FIELD;
    std::string why;
    const QdShHostTables H{w, mu, seed, A, B, nullptr, nullptr};
    QdSpharm* s = spharm_build(t, n_lat, n_lon, trunc, H, false, st, &why);
    int rc = s ? 0 : qd_fail(nullptr, ("qd_spharm_analyse_grid: " + why).c_str());
    if (s) {
        rc = spharm_analyse(s, nullptr, st, "qd_spharm_analyse_grid", plane, coef_re, coef_im, rec);
        hipStreamSynchronize(st);
        spharm_free(s);
    }
    hipStreamDestroy(st);
    return rc;
}
