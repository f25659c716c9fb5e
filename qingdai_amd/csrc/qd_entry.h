// qd_entry.h -- the entry table the history accumulators (qd_history.hip) and the per-step series (qd_series.hip) share: what an
// entry is, what it is worth in a cell, where in a step it is sampled and which fields make a sampled step store its diagnostics.
//   op 0   the f64 plane a                         op 1   sqrt(a*a + b*b) of the planes a and b, rounded as np.sqrt(u*u + v*v)
// An entry that reads PRECIP is EARLY: sampled in front of the ocean step, inside which the next step's precipitation block may
// already run (QD_HOIST_PRECIP, qd_api.hip); every other entry is LATE, sampled behind the step's last launch.
#pragma once
#include "qd_internal.h"
#include <algorithm>
#include <string>

#define QD_ENTRY_MAX 32            // entries of one table (include/qingdai_hip.h: QD_HISTORY_MAX_ENTRIES, QD_SERIES_MAX_ENTRIES)

__device__ __forceinline__ double hist_value(double a, double b, bool pair) { return pair ? sqrt(a * a + b * b) : a; }

// the fields nothing inside a span reads and only a span's last step stores (qd_internal.h: lazy_diag)
static inline bool hist_lazy_field(int f) {
    static const int L[] = {QD_F_P_RAIN, QD_F_S_SNOW_NEXT, QD_F_MELT, QD_F_C_SNOW, QD_F_GLACIER, QD_F_ISR_A, QD_F_ISR_B, QD_F_EFLUX, QD_F_LHREL, QD_F_OLR};
    return std::find(std::begin(L), std::end(L), f) != std::end(L);
}
static inline bool hist_plane(const qd_ctx* c, int f) { return f >= 0 && f < QD_F_COUNT_F64 && !qd_eco_is_f32(c, f); }

struct QdEntrySel {
    int n = 0;
    int op[QD_ENTRY_MAX], a[QD_ENTRY_MAX], b[QD_ENTRY_MAX];
    bool early[QD_ENTRY_MAX];         // the entry reads PRECIP: sampled in front of the ocean step
    bool lazy = false;                // an entry reads one of the lazily stored diagnostics (QD_LAZY_DIAG)

    // the ecology may have turned a selected map into an f32 slab since the configure (qd_eco_params.map_f32)
    bool stale(const qd_ctx* c) const {
        for (int k = 0; k < n; ++k)
            if (!hist_plane(c, a[k]) || (op[k] == 1 && !hist_plane(c, b[k]))) return true;
        return false;
    }
};

// the checks of a qd_X_configure on its (op, a, b) lists, in their order, with "<who>: " in front -> 0 and t filled (t.n = n), or
// -1 with the error set
static inline int qd_entries_parse(qd_ctx* c, const char* who, int n, const int32_t* op, const int32_t* a, const int32_t* b, QdEntrySel& t) {
    const std::string w = std::string(who) + ": ";
    if (n > QD_ENTRY_MAX) return qd_fail(c, (w + "at most 32 entries").c_str());
    for (int k = 0; k < n; ++k) {
        if (op[k] != 0 && op[k] != 1) return qd_fail(c, (w + "unknown op (0 = field a, 1 = sqrt(a*a + b*b))").c_str());
        if (!hist_plane(c, a[k])) return qd_fail(c, (w + "field a is not an f64 plane").c_str());
        if (op[k] == 1 && !b) return qd_fail(c, (w + "op 1 needs a second field b").c_str());
        if (op[k] == 1 && !hist_plane(c, b[k])) return qd_fail(c, (w + "field b is not an f64 plane").c_str());
        t.op[k] = op[k]; t.a[k] = a[k]; t.b[k] = op[k] == 1 ? b[k] : -1;
        t.early[k] = a[k] == QD_F_PRECIP || t.b[k] == QD_F_PRECIP;
        if (t.early[k] && op[k] == 1 && a[k] != b[k])
            return qd_fail(c, (w + "op 1 cannot pair PRECIP with another field (they are sampled at different places of a step)").c_str());
        t.lazy = t.lazy || hist_lazy_field(a[k]) || (op[k] == 1 && hist_lazy_field(b[k]));
    }
    t.n = n;
    return 0;
}
