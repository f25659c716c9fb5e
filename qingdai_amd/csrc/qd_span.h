// qd_span.h -- the span lane: something that fires on scheduled steps of a qd_step_n span and leaves one record per firing in a
// device log the host drains afterwards.  Three lanes: river routing (bit7, qd_route.hip), the daily phytoplankton step (bit8,
// qd_phyto_daily.hip), the daily vegetation step (bit9, qd_eco_daily.hip); the individuals' daily step
// (qd_indiv_daily.hip) fires with bit9 and keeps a log of its own; the budget diagnostics (qd_budget_diag.hip) have no flag bit:
// a schedule given before the span turns them on; so it is with the history accumulators (qd_history.hip), which keep sum planes
// instead of a log (width 0), and with the per-step series (qd_series.hip), whose records are large and come every sampled step: its
// lane holds QD_SERIES_LOG_CAP of them (cap), the zonal spectra (qd_spectra.hip), a lane of the same kind, QD_SPECTRA_LOG_CAP, every
// other lane QD_SPAN_LOG_CAP.  The drifters (qd_drift.hip) are the one lane whose resident state moves: EVERY step of a span it is
// scheduled for advances the particles, and the schedule value says whether the step also leaves a record; its cap follows the
// record size.  The flow lane (qd_flow.hip: streamfunction and velocity potential) is a lane of the spectra's kind, QD_FLOW_LOG_CAP,
// and so are the spherical-harmonic spectra (qd_spharm.hip), QD_SPHARM_LOG_CAP.  The eddy statistics (qd_eddy.hip) are a lane of
// history's kind: resident sum planes, no log (width 0); so are the extremes, spells and distributions (qd_extremes.hip), whose
// resident planes hold selections and integer counts, sampled at history's two places.
//   qd_X_schedule           qd_lane_schedule: one value per step of the NEXT span, 0 = the step does not fire
//   qd_step_n, before work  qd_lane_span_begin: exactly n steps scheduled, and their firings fit into the log behind the cursor
//   qd_step_n, step s       at(s) != 0: X runs (not when full()) and writes its record at next()
//   qd_step_n, any exit     clear_schedule() (the span guard): a schedule serves one span
//   qd_X_events / qd_X_log  qd_lane_drain: the records so far, oldest first, to the host; the cursor returns to 0
// Host side only, no allocation and no getenv on the qd_step_n path.  The error texts are the subsystem's.
#pragma once
#include "qd_internal.h"

// QD_SPAN_LOG_CAP, the records a lane holds between two drains, is the public header's (the host sizes its drain buffers by it)
enum { QD_LANE_ROUTE = 0, QD_LANE_PHYTO_DAILY, QD_LANE_ECO_DAILY, QD_LANE_INDIV_DAILY, QD_LANE_BUDGET, QD_LANE_HISTORY, QD_LANE_EXTREMES, QD_LANE_SERIES, QD_LANE_SPECTRA, QD_LANE_DRIFT, QD_LANE_FLOW, QD_LANE_SPHARM, QD_LANE_EDDY, QD_N_LANES };

struct QdSpanLane {
    double* log = nullptr;          // device, [cap][width]; the subsystem sets width (and cap), allocates and frees it
    int width = 0, n = 0;           // doubles per record; records queued since the last drain (the cursor)
    int cap = QD_SPAN_LOG_CAP;      // records the log holds between two drains
    bool counts = false;            // a schedule value is the step's number of firings (>= 0); else any non-zero value is one firing
    std::vector<double> sched;      // the next span's value per step

    size_t log_doubles() const { return (size_t)cap * width; }     // what the subsystem allocates
    double at(int s) const { return s >= 0 && s < (int)sched.size() ? sched[s] : 0.0; }
    void clear_schedule() { sched.clear(); }
    void reset() { n = 0; sched.clear(); }
    bool scheduled(int steps) const { return (int)sched.size() == steps; }
    bool fits() const { double ev = 0.0; for (double x : sched) ev += counts ? x : (x != 0.0 ? 1.0 : 0.0); return n + ev <= cap; }
    bool full() const { return n >= cap; }
    double* next() { return log + (size_t)(n++) * width; }                     // where the next record goes; the cursor moves on
};

// The bodies of qd_X_schedule and qd_X_log / qd_X_events.  l: the subsystem's lane, nullptr while it is not configured ->
// "<who>: <missing>"
template <class T> inline int qd_lane_schedule(qd_ctx* c, QdSpanLane* l, int steps, const T* v, const char* who, const char* missing) {
    if (!c || steps < 0 || (steps && !v)) return -1;
    if (!l) return qd_fail(c, (std::string(who) + ": " + missing).c_str());
    if (l->counts) for (int s = 0; s < steps; ++s) if (v[s] < 0) return qd_fail(c, (std::string(who) + ": negative firing count").c_str());
    l->sched.assign(v, v + steps);
    return 0;
}
inline int qd_lane_drain(qd_ctx* c, QdSpanLane* l, double* out, int max, int* count, const char* who, const char* missing) {
    if (!c || !count) return -1;
    const std::string w(who);
    if (!l) return qd_fail(c, (w + ": " + missing).c_str());
    if (l->n > max) return qd_fail(c, (w + ": more records than room").c_str());
    hipSetDevice(c->desc.device);
    if (l->n && !out) return -1;
    if (l->n) QD_HIP(c, hipMemcpyAsync(out, l->log, (size_t)l->n * l->width * sizeof(double), hipMemcpyDeviceToHost, c->stream));
    QD_HIP(c, hipStreamSynchronize(c->stream));
    const hipError_t e = hipGetLastError();
    if (e != hipSuccess) return qd_fail(c, (w + ": kernel").c_str(), e);
    *count = l->n; l->n = 0;
    return 0;
}

// The checks every qd_X_span_begin makes, in their order, with the subsystem's texts; `needs` (a flag of the span the lane depends
// on is missing) and `stale` (the configuration no longer matches the handle) are the subsystem's own findings, or nullptr.
// -> the lane, or nullptr with the error set.
struct QdSpanTexts { const char *globe, *missing, *unscheduled, *overflow; };
inline QdSpanLane* qd_lane_span_begin(qd_ctx* c, QdSpanLane* l, int steps, const QdSpanTexts& t, const char* needs = nullptr,
                                      const char* stale = nullptr) {
    const char* why = !qd_whole_globe(c) ? t.globe : !l ? t.missing : needs ? needs : !l->scheduled(steps) ? t.unscheduled
                    : stale ? stale : !l->fits() ? t.overflow : nullptr;
    if (why) qd_fail(c, why);
    return why ? nullptr : l;
}
