// qd_span.h -- the span lane: something that fires on scheduled steps of a qd_step_n span and leaves one record per firing in a
// device log the host drains afterwards: river routing (bit7, qd_route.hip), the daily phytoplankton step (bit8, qd_phyto_daily.hip).
//   qd_X_schedule           set():   one value per step of the NEXT span, 0 = the step does not fire
//   qd_step_n, before work  scheduled(n) && fits(): exactly n steps, and their firings fit into the log behind the cursor
//   qd_step_n, step s       at(s) != 0: X runs (not when full()) and writes its record at next()
//   qd_step_n, any exit     clear_schedule() (the span guard): a schedule serves one span
//   qd_X_events / qd_X_log  drain(): the records so far, oldest first, to the host; the cursor returns to 0
// Host side only, no allocation and no getenv on the qd_step_n path.  The error texts are the subsystem's.
#pragma once
#include "qd_internal.h"

#define QD_SPAN_LOG_CAP 4096        // records a lane holds between two drains (qingdai_amd/_lib.py: SPAN_LOG_CAP is the same number)

struct QdSpanLane {
    double* log = nullptr;          // device, [QD_SPAN_LOG_CAP][width]; the subsystem sets width, allocates and frees it
    int width = 0, n = 0;           // doubles per record; records queued since the last drain (the cursor)
    std::vector<double> sched;      // the next span's value per step

    size_t log_doubles() const { return (size_t)QD_SPAN_LOG_CAP * width; }     // what the subsystem allocates
    template <class T> void set(const T* v, int steps) { sched.assign(v, v + steps); }
    double at(int s) const { return s >= 0 && s < (int)sched.size() ? sched[s] : 0.0; }
    void clear_schedule() { sched.clear(); }
    void reset() { n = 0; sched.clear(); }
    bool scheduled(int steps) const { return (int)sched.size() == steps; }
    bool fits() const { int ev = 0; for (double x : sched) ev += x != 0.0; return n + ev <= QD_SPAN_LOG_CAP; }
    bool full() const { return n >= QD_SPAN_LOG_CAP; }
    double* next() { return log + (size_t)(n++) * width; }                     // where the next record goes; the cursor moves on
    int drain(qd_ctx* c, const std::string& who, double* out, int max, int* count) {
        if (n > max) return qd_fail(c, (who + ": more records than room").c_str());
        hipSetDevice(c->desc.device);
        if (n && !out) return -1;
        if (n) QD_HIP(c, hipMemcpyAsync(out, log, (size_t)n * width * sizeof(double), hipMemcpyDeviceToHost, c->stream));
        QD_HIP(c, hipStreamSynchronize(c->stream));
        const hipError_t e = hipGetLastError();
        if (e != hipSuccess) return qd_fail(c, (who + ": kernel").c_str(), e);
        *count = n; n = 0;
        return 0;
    }
};
