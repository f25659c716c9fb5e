// qd_truecolor.hip -- the reference's pseudo-true-colour frame from the resident state, gfx950 (qd_truecolor_render).
//
// plot_true_color (scripts/run_simulation.py:539-778) builds rgb_map[n_lat][n_lon][3] with pointwise array arithmetic, hands it to
// imshow and prints a [TrueColor] line with two sea-ice numbers.  Here:
//   k_truecolor<WANT64>  one thread per cell, f64, the reference's stages in its order of operations (:548-757):
//                        base colours by land mask -> sea ice where 1 - exp(-max(h_ice, 0) / max(1e-6, H_ref)) >= thr on the ocean ->
//                        land snow blend from nan_to_num(C_snow) -> vegetation overlay (A_b = clip(R_eff[b] f + (1 - f) soil_ref, 0, 1)
//                        on land, NaN elsewhere; channel sums nansum_b A_b (w_c[b] w_rel[b]) in b order; clip, gamma, saturation;
//                        blended by clip(nan_to_num(f), 0, 1) on land) -> ocean-colour overlay (the same sums over the phytoplankton
//                        band stack, its own gamma, blended into the ocean cells that are not sea ice) -> snow by T_s -> clouds ->
//                        rivers -> lakes -> clip.  w_rel[b] = I_b / (I_tot + 1e-12) where I_tot = max(ISR, 0) > 1e-12, else 0; I_b is
//                        recomputed per cell from ISR_A / ISR_B and the band tables with the rule of k_band_insolation
//                        (qd_physics.hip), so no [NB]-plane irradiance stack is read.  The band loops are unrolled over 16 register
//                        slots and guarded by the runtime band count; the tables travel in the kernel arguments.
//                        Output: the u8 image, row-flipped (northernmost row first, imshow's origin='lower'),
//                        min(255, floor(x 255 + 0.5)), NaN -> 0; with WANT64 also the unquantised rgb in grid order.  Per workgroup
//                        one partial of sum w mask, sum w, sum h_ice mask, sum mask (w = max(cos lat, 0)): wave shuffles, then LDS.
//   k_truecolor_final    one workgroup: the partials in a fixed order -> sea_ice_area = sum(w mask) / (sum(w) + 1e-15), mean_h_ice.
// np.maximum / np.clip propagate NaN (qd_max / qd_clip), np.nansum counts a NaN term as 0.  x ** e follows NumPy's scalar-exponent
// shortcuts (e == 1: x, e == 0.5: sqrt, e == 2: x x), else pow.  f64, contraction off (Makefile), no atomics, vector stores only.
// exp and pow are the only operations whose rounding may differ from NumPy's.
#include "qd_internal.h"
#include "qd_blockred.h"
#include <algorithm>

#define QD_TC_NB QD_TRUECOLOR_MAX_BANDS

struct QdTcTab { double reff[QD_TC_NB], wr[QD_TC_NB], wg[QD_TC_NB], wb[QD_TC_NB], sa[QD_TC_NB], sb[QD_TC_NB], tr[QD_TC_NB]; };

struct QdTrueColor {
    qd_truecolor_params p{};
    int configured = 0;
    QdTcTab eco{}, ph{};
    size_t cells = 0;
    uint8_t* img = nullptr;            // [nlat][nlon][3], row-flipped
    double* rgb = nullptr;             // [nlat][nlon][3], allocated by the first render that wants it
    QdPartials partial;                // [4][nblk]
    double* out2 = nullptr;            // device {sea_ice_area, mean_h_ice}
    double* pbands = nullptr; int pbands_nb = 0;   // a caller's phytoplankton band stack (qd_truecolor_configure)
    double* flow = nullptr;            // a caller's flow map (qd_truecolor_render)
    uint8_t* lake = nullptr;
    int have_img = 0, have_rgb = 0;
    double last2[2] = {0, 0};
};

struct QdTcArgs {
    int nlat, nlon; int cells;
    qd_truecolor_params p;
    int veg, oc, rivers, lakes, ecof_f32;
    const uint8_t* land;
    const double *hice, *csnow, *cloud, *ts, *isr, *isrA, *isrB;
    const void* ecof;
    const double* pbands; size_t pplane;
    const double* flow; const uint8_t* lake; const double* warea;
    QdTcTab eco, ph;
    uint8_t* img; double* rgb; double* partial;
};

// w_rel[b] = I_b / (I_tot + 1e-12) of one cell (run_simulation.py:610-620 over spectral.py:397-426)
__device__ __forceinline__ void qd_tc_wrel(const QdTcTab& T, int nb, double A, double B, double isr, double* wrel) {
    const double tot = A + B;
    double S[QD_TC_NB];
    double sum = 0.0;
#pragma unroll
    for (int b = 0; b < QD_TC_NB; ++b)
        if (b < nb) { S[b] = (T.sa[b] * A + T.sb[b] * B) * T.tr[b]; sum += S[b]; }
    const bool pos = (sum > 1e-12) && (tot > 1e-12);
    const double itot = qd_max(isr, 0.0);
    const bool lit = itot > 1e-12;
    const double den = itot + 1e-12;
#pragma unroll
    for (int b = 0; b < QD_TC_NB; ++b)
        if (b < nb) {
            double v = pos ? (S[b] / sum) * tot : 0.0;
            if (!(fabs(v) <= DBL_MAX)) v = 0.0;                // nan_to_num(nan=0, posinf=0, neginf=0)
            wrel[b] = lit ? v / den : 0.0;
        }
}

__device__ __forceinline__ void qd_tc_add(double& acc, int b, double t) {      // np.nansum over axis 0: NaN terms count as 0
    if (t != t) t = 0.0;
    acc = (b == 0) ? t : acc + t;
}

template <bool WANT64>
__global__ void __launch_bounds__(QD_BLOCK)
k_truecolor(QdTcArgs K) {
    const qd_truecolor_params& P = K.p;
    const int o = blockIdx.x * QD_BLOCK + threadIdx.x;
    double acc[4] = {0.0, 0.0, 0.0, 0.0};                      // w mask, w, h_ice mask, mask
    if (o < K.cells) {
        const int row = o / K.nlon, col = o - row * K.nlon;
        const uint8_t lm = K.land[o];
        const bool ocean = lm == 0, land = lm == 1;
        const double ice_r = 0.90, ice_g = 0.90, ice_b = 0.95;
        double r = 0.0, g = 0.0, b = 0.0;
        if (ocean) { r = 0.10; g = 0.20; b = 0.50; }
        if (land) { r = 0.40; g = 0.30; b = 0.20; }
        // sea ice from thickness
        const double h = K.hice[o];
        const double href = (1e-6 > P.h_ice_ref) ? 1e-6 : P.h_ice_ref;      // Python's max(1e-6, H_ice_ref)
        const double ice_frac = 1.0 - exp(-qd_max(h, 0.0) / href);
        const bool sea_ice = ocean && (ice_frac >= P.ice_frac_thr);
        if (sea_ice) { r = ice_r; g = ice_g; b = ice_b; }
        const double w = K.warea[row];
        acc[1] = w;
        if (sea_ice) { acc[0] = w; acc[2] = h; acc[3] = 1.0; }
        // land snow from the cover fraction
        if (P.snow_by_swe) {
            const double C = qd_nn(K.csnow[o]);
            if (land && C >= P.snow_cover_frac) {
                const double al = P.snow_vis_alpha * qd_clip(C, 0.0, 1.0);
                r = r * (1.0 - al) + ice_r * al;
                g = g * (1.0 - al) + ice_g * al;
                b = b * (1.0 - al) + ice_b * al;
            }
        }
        const double insA = K.isrA[o], insB = K.isrB[o], isr = K.isr[o];
        // vegetation overlay
        if (K.veg) {
            double fraw;                                       // canopy_reflectance_factor(): the cache on land, NaN elsewhere
            if (P.veg_f_one) fraw = land ? 1.0 : NAN;
            else fraw = land ? (K.ecof_f32 ? (double)((const float*)K.ecof)[o] : ((const double*)K.ecof)[o]) : NAN;
            const double fn = P.veg_f_one ? (land ? 1.0 : 0.0) : qd_nn(fraw);
            double wrel[QD_TC_NB];
            qd_tc_wrel(K.eco, P.nb_eco, insA, insB, isr, wrel);
            double Rr = 0.0, Rg = 0.0, Rb = 0.0;
#pragma unroll
            for (int k = 0; k < QD_TC_NB; ++k)
                if (k < P.nb_eco) {
                    const double Ab = land ? qd_clip(K.eco.reff[k] * fraw + (1.0 - fraw) * P.soil_ref, 0.0, 1.0) : NAN;
                    qd_tc_add(Rr, k, Ab * (K.eco.wr[k] * wrel[k]));
                    qd_tc_add(Rg, k, Ab * (K.eco.wg[k] * wrel[k]));
                    qd_tc_add(Rb, k, Ab * (K.eco.wb[k] * wrel[k]));
                }
            double vr = qd_clip(Rr, 0.0, 1.0), vg = qd_clip(Rg, 0.0, 1.0), vb = qd_clip(Rb, 0.0, 1.0);
            if (P.veg_gamma > 0.0) {
                const double e = 1.0 / P.veg_gamma;
                vr = qd_pow_np(vr, e); vg = qd_pow_np(vg, e); vb = qd_pow_np(vb, e);
            }
            if (P.veg_sat != 1.0) {
                const double m = ((vr + vg) + vb) / 3.0;
                vr = qd_clip(m + P.veg_sat * (vr - m), 0.0, 1.0);
                vg = qd_clip(m + P.veg_sat * (vg - m), 0.0, 1.0);
                vb = qd_clip(m + P.veg_sat * (vb - m), 0.0, 1.0);
            }
            if (land) {
                const double f = qd_clip(fn, 0.0, 1.0);
                r = r * (1.0 - f) + vr * f;
                g = g * (1.0 - f) + vg * f;
                b = b * (1.0 - f) + vb * f;
            }
        }
        // ocean colour on the open ocean
        if (K.oc && ocean && !sea_ice) {
            double wrel[QD_TC_NB];
            qd_tc_wrel(K.ph, P.nb_phyto, insA, insB, isr, wrel);
            double Rr = 0.0, Rg = 0.0, Rb = 0.0;
#pragma unroll
            for (int k = 0; k < QD_TC_NB; ++k)
                if (k < P.nb_phyto) {
                    const double Ab = K.pbands[(size_t)k * K.pplane + o];
                    qd_tc_add(Rr, k, Ab * (K.ph.wr[k] * wrel[k]));
                    qd_tc_add(Rg, k, Ab * (K.ph.wg[k] * wrel[k]));
                    qd_tc_add(Rb, k, Ab * (K.ph.wb[k] * wrel[k]));
                }
            double vr = qd_clip(Rr, 0.0, 1.0), vg = qd_clip(Rg, 0.0, 1.0), vb = qd_clip(Rb, 0.0, 1.0);
            if (P.oc_gamma > 0.0) {
                const double e = 1.0 / P.oc_gamma;
                vr = qd_pow_np(vr, e); vg = qd_pow_np(vg, e); vb = qd_pow_np(vb, e);
            }
            r = r * (1.0 - P.oc_blend) + vr * P.oc_blend;
            g = g * (1.0 - P.oc_blend) + vg * P.oc_blend;
            b = b * (1.0 - P.oc_blend) + vb * P.oc_blend;
        }
        // snow by surface temperature
        if (P.snow_by_ts && land && K.ts[o] <= P.snow_thresh) { r = 0.97 * ice_r; g = 0.97 * ice_g; b = 0.97 * ice_b; }
        // clouds
        {
            const double ca = P.cloud_alpha * K.cloud[o];
            r = r * (1.0 - ca) + ca * P.cloud_white;
            g = g * (1.0 - ca) + ca * P.cloud_white;
            b = b * (1.0 - ca) + ca * P.cloud_white;
        }
        const double land_f = land ? 1.0 : 0.0;
        if (K.rivers) {
            const double m = ((K.flow[o] >= P.river_min) ? 1.0 : 0.0) * land_f;
            const double am = P.river_alpha * m;
            r = r * (1.0 - am) + 0.05 * am;
            g = g * (1.0 - am) + 0.35 * am;
            b = b * (1.0 - am) + 0.90 * am;
        }
        if (K.lakes) {
            const double m = (double)K.lake[o] * land_f;
            const double am = P.lake_alpha * m;
            r = r * (1.0 - am) + 0.15 * am;
            g = g * (1.0 - am) + 0.55 * am;
            b = b * (1.0 - am) + 0.95 * am;
        }
        r = qd_clip(r, 0.0, 1.0); g = qd_clip(g, 0.0, 1.0); b = qd_clip(b, 0.0, 1.0);
        if (WANT64) {
            double* q = K.rgb + (size_t)o * 3;
            q[0] = r; q[1] = g; q[2] = b;
        }
        uint8_t* q8 = K.img + ((size_t)(K.nlat - 1 - row) * K.nlon + col) * 3;
        const double qr = floor(r * 255.0 + 0.5), qg = floor(g * 255.0 + 0.5), qb = floor(b * 255.0 + 0.5);
        q8[0] = (r == r) ? (uint8_t)(qr > 255.0 ? 255.0 : qr) : (uint8_t)0;
        q8[1] = (g == g) ? (uint8_t)(qg > 255.0 ? 255.0 : qg) : (uint8_t)0;
        q8[2] = (b == b) ? (uint8_t)(qb > 255.0 ? 255.0 : qb) : (uint8_t)0;
    }
    qd_block_partials(acc, 4, nullptr, K.partial, (size_t)gridDim.x, (size_t)blockIdx.x);
}

__global__ void __launch_bounds__(QD_BLOCK)
k_truecolor_final(const double* __restrict__ partial, int nblk, double* __restrict__ out2) {
    __shared__ double tot[4];
    qd_planes_by_wave(partial, nblk, 4, tot);
    if (threadIdx.x == 0) {
        out2[0] = tot[0] / (tot[1] + 1e-15);
        out2[1] = tot[3] > 0.0 ? tot[2] / tot[3] : 0.0;
    }
}

// ------------------------------------------------------------------ host side
void qd_truecolor_release(qd_ctx* c) {
    QdTrueColor* d = c->tcol;
    if (!d) return;
    void* p[] = {d->img, d->rgb, d->partial.p, d->out2, d->pbands, d->flow, d->lake};
    for (void* q : p) if (q) hipFree(q);
    delete d;
    c->tcol = nullptr;
}

static void tc_fill(double* dst, const double* src, int nb) {
    for (int b = 0; b < QD_TC_NB; ++b) dst[b] = b < nb ? src[b] : 0.0;
}

extern "C" int qd_truecolor_configure(qd_handle c, const qd_truecolor_params* p, size_t sz, const double* eco_tab,
                                      const double* phyto_tab, const double* phyto_bands, const uint8_t* lake_mask) {
    if (!c || !p) return -1;
    if (sz != sizeof(qd_truecolor_params)) return qd_fail(c, "qd_truecolor_configure: struct size mismatch (ABI)");
    if (!qd_whole_globe(c))
        return qd_fail(c, "qd_truecolor_configure: the true-colour frame needs a whole-globe handle (world == 1, n_rows == n_lat); "
                          "latitude bands are not supported");
    if (p->nb_eco < 0 || p->nb_eco > QD_TC_NB || p->nb_phyto < 0 || p->nb_phyto > QD_TC_NB)
        return qd_fail(c, "qd_truecolor_configure: band counts out of range (0..16)");
    if (p->veg && (p->nb_eco < 1 || !eco_tab)) return qd_fail(c, "qd_truecolor_configure: the vegetation overlay needs nb_eco >= 1 and eco_tab");
    if (p->oceancolor && (p->nb_phyto < 1 || !phyto_tab)) return qd_fail(c, "qd_truecolor_configure: the ocean-colour overlay needs nb_phyto >= 1 and phyto_tab");
    if (p->lakes && !lake_mask) return qd_fail(c, "qd_truecolor_configure: lakes set without a lake mask");
    if ((size_t)c->geo.nlat * (size_t)c->geo.nlon > (size_t)INT_MAX / 4) return qd_fail(c, "qd_truecolor_configure: grid too large");
    hipSetDevice(c->desc.device);
    QdTrueColor* d = c->tcol;
    if (!d) d = c->tcol = new QdTrueColor();
    d->configured = 0; d->have_img = d->have_rgb = 0;
    QD_HIP(c, hipStreamSynchronize(c->stream));
    const size_t cells = (size_t)c->geo.nlat * c->geo.nlon;
    d->cells = cells;
    if (!d->img) QD_HIP(c, hipMalloc(&d->img, cells * 3));
    if (int rc = d->partial.ensure(c, 4, (int)((cells + QD_BLOCK - 1) / QD_BLOCK))) return rc;
    if (!d->out2) QD_HIP(c, hipMalloc(&d->out2, 2 * sizeof(double)));
    d->eco = QdTcTab{}; d->ph = QdTcTab{};
    if (eco_tab && p->nb_eco > 0) {
        const int nb = p->nb_eco;
        double* dst[7] = {d->eco.reff, d->eco.wr, d->eco.wg, d->eco.wb, d->eco.sa, d->eco.sb, d->eco.tr};
        for (int k = 0; k < 7; ++k) tc_fill(dst[k], eco_tab + (size_t)k * nb, nb);
    }
    if (phyto_tab && p->nb_phyto > 0) {
        const int nb = p->nb_phyto;
        double* dst[6] = {d->ph.wr, d->ph.wg, d->ph.wb, d->ph.sa, d->ph.sb, d->ph.tr};
        for (int k = 0; k < 6; ++k) tc_fill(dst[k], phyto_tab + (size_t)k * nb, nb);
    }
    if (d->pbands) { hipFree(d->pbands); d->pbands = nullptr; d->pbands_nb = 0; }
    if (phyto_bands && p->nb_phyto > 0) {
        const size_t n = (size_t)p->nb_phyto * cells * sizeof(double);
        QD_HIP(c, hipMalloc(&d->pbands, n));
        QD_HIP(c, hipMemcpy(d->pbands, phyto_bands, n, hipMemcpyHostToDevice));
        d->pbands_nb = p->nb_phyto;
    }
    if (lake_mask) {
        if (!d->lake) QD_HIP(c, hipMalloc(&d->lake, cells));
        QD_HIP(c, hipMemcpy(d->lake, lake_mask, cells, hipMemcpyHostToDevice));
    }
    d->p = *p;
    d->configured = 1;
    return 0;
}

extern "C" int qd_truecolor_render(qd_handle c, int want_f64, const double* flow, double* out2) {
    if (!c) return -1;
    if (!qd_whole_globe(c))
        return qd_fail(c, "qd_truecolor_render: the true-colour frame needs a whole-globe handle; latitude bands are not supported");
    QdTrueColor* d = c->tcol;
    if (!d || !d->configured) return qd_fail(c, "qd_truecolor_render: qd_truecolor_configure has not been called");
    hipSetDevice(c->desc.device);
    const size_t cells = d->cells;
    d->have_img = d->have_rgb = 0;
    QdTcArgs K;
    K.nlat = c->geo.nlat; K.nlon = c->geo.nlon; K.cells = (int)cells;
    K.p = d->p;
    K.veg = d->p.veg ? 1 : 0;
    K.rivers = d->p.rivers ? 1 : 0;
    K.lakes = (d->p.lakes && d->lake) ? 1 : 0;
    K.flow = nullptr;
    if (K.rivers) {
        if (flow) {
            QD_HIP(c, hipStreamSynchronize(c->stream));        // an earlier render may still read the staging buffer
            if (!d->flow) QD_HIP(c, hipMalloc(&d->flow, cells * sizeof(double)));
            QD_HIP(c, hipMemcpy(d->flow, flow, cells * sizeof(double), hipMemcpyHostToDevice));
            K.flow = d->flow;
        } else {
            K.flow = qd_route_flow(c);
            if (!K.flow) return qd_fail(c, "qd_truecolor_render: rivers are on, flow is NULL and no routing network is configured");
        }
    }
    K.oc = 0; K.pbands = nullptr; K.pplane = c->geo.cells();
    if (d->p.oceancolor) {
        if (d->pbands) { K.oc = 1; K.pbands = d->pbands; K.pplane = cells; }
        else {
            const double* pb = nullptr; int nb = 0; int64_t steps = 0;
            if (qd_phyto_daily_bands(c, &pb, &nb, &steps)) {
                if (nb != d->p.nb_phyto) return qd_fail(c, "qd_truecolor_render: nb_phyto is not the band count of the resident stack");
                if (steps > 0) { K.oc = 1; K.pbands = pb; }    // before the first daily step the reference has no band maps
            }
        }
    }
    double** F = c->f;
    K.ecof_f32 = qd_eco_is_f32(c, QD_F_ECO_F) ? 1 : 0;
    K.land = c->land;
    K.hice = F[QD_F_HICE]; K.csnow = F[QD_F_C_SNOW]; K.cloud = F[QD_F_CLOUD]; K.ts = F[QD_F_TS];
    K.isr = F[QD_F_ISR]; K.isrA = F[QD_F_ISR_A]; K.isrB = F[QD_F_ISR_B]; K.ecof = F[QD_F_ECO_F];
    K.lake = d->lake; K.warea = c->tabs.warea;
    K.eco = d->eco; K.ph = d->ph;
    if (want_f64 && !d->rgb) {
        QD_HIP(c, hipStreamSynchronize(c->stream));
        QD_HIP(c, hipMalloc(&d->rgb, cells * 3 * sizeof(double)));
    }
    K.img = d->img; K.rgb = want_f64 ? d->rgb : nullptr; K.partial = d->partial.p;
    {
        QdScope sc(c, "truecolor");
        const dim3 grid(d->partial.nblk), block(QD_BLOCK);
        if (want_f64) hipLaunchKernelGGL(k_truecolor<true>, grid, block, 0, c->stream, K);
        else hipLaunchKernelGGL(k_truecolor<false>, grid, block, 0, c->stream, K);
        hipLaunchKernelGGL(k_truecolor_final, dim3(1), block, 0, c->stream, d->partial.p, d->partial.nblk, d->out2);
    }
    QD_HIP(c, hipMemcpyAsync(d->last2, d->out2, 2 * sizeof(double), hipMemcpyDeviceToHost, c->stream));
    QD_HIP(c, hipStreamSynchronize(c->stream));
    const hipError_t e = hipGetLastError();
    if (e != hipSuccess) return qd_fail(c, "qd_truecolor_render: kernel", e);
    d->have_img = 1; d->have_rgb = want_f64 ? 1 : 0;
    if (out2) { out2[0] = d->last2[0]; out2[1] = d->last2[1]; }
    return 0;
}

extern "C" int qd_truecolor_download(qd_handle c, int which, void* host, size_t n) {
    if (!c || !host) return -1;
    const QdTrueColor* d = c->tcol;
    if (!d || !d->have_img) return qd_fail(c, "qd_truecolor_download: no frame on this handle (call qd_truecolor_render first)");
    if (which != 0 && which != 1) return qd_fail(c, "qd_truecolor_download: which must be 0 (u8 image) or 1 (f64 rgb)");
    if (which == 1 && !d->have_rgb) return qd_fail(c, "qd_truecolor_download: the last render did not keep the f64 rgb (want_f64)");
    if (n != d->cells * 3) return qd_fail(c, "qd_truecolor_download: size mismatch");
    hipSetDevice(c->desc.device);
    const size_t bytes = which == 0 ? n : n * sizeof(double);
    QD_HIP(c, hipMemcpyAsync(host, which == 0 ? (const void*)d->img : (const void*)d->rgb, bytes, hipMemcpyDeviceToHost, c->stream));
    QD_HIP(c, hipStreamSynchronize(c->stream));
    return 0;
}
