// Event slots of the library's three live profilers (mvs_profile_dominant / _layers / _stages, include/mvsnet_hip.h): up to
// CALLS calls, EVENTS HIP events each, created on first use and kept.  A call claims a slot, marks events on its stream and
// commits the slot once it shall count; the read-out waits for the events and averages intervals over the committed calls.
// Not for hipGraph capture.  The instances live in library.hip; regnet.hip claims and marks.
#pragma once
#include "common.h"

template <int CALLS, int EVENTS>
struct EventSlots {
    bool on = false;
    int used = 0, created = 0;
    hipEvent_t ev[CALLS][EVENTS];
    bool hit[CALLS][EVENTS];       // recorded by the call that holds the slot

    void enable(bool e) { on = e; used = 0; }
    // slot of this call, or -1 (off, full, or no events to be had)
    int claim() {
        if (!on || used >= CALLS) return -1;
        const int s = used;
        if (s >= created) {
            for (int k = 0; k < EVENTS; ++k) if (hipEventCreate(&ev[s][k]) != hipSuccess) return -1;
            created = s + 1;
        }
        for (int k = 0; k < EVENTS; ++k) hit[s][k] = false;
        return s;
    }
    void commit(int s) { if (s >= 0) used = s + 1; }
    int mark(int s, int k, hipStream_t st) {
        if (s < 0) return 0;
        const hipError_t e = hipEventRecord(ev[s][k], st);
        if (e == hipSuccess) hit[s][k] = true;
        return (int)e;
    }
    // avg_ms[l] = mean over the committed calls of the time from event l * stride to event l * stride + 1 (0 where an end was
    // never recorded); *count = committed calls.  Starts a new series.
    int read(double* avg_ms, int n, int stride, int* count) {
        for (int l = 0; l < n; ++l) avg_ms[l] = 0.0;
        for (int i = 0; i < used; ++i)
            for (int l = 0; l < n; ++l) {
                const int k = l * stride;
                if (!hit[i][k] || !hit[i][k + 1]) continue;
                hipError_t e = hipEventSynchronize(ev[i][k + 1]);
                float ms = 0.f;
                if (e == hipSuccess) e = hipEventElapsedTime(&ms, ev[i][k], ev[i][k + 1]);
                if (e != hipSuccess) return (int)e;
                avg_ms[l] += ms;
            }
        *count = used;
        if (used) for (int l = 0; l < n; ++l) avg_ms[l] /= used;
        used = 0;
        return 0;
    }
};

// capacities: 64, 32 and 32 calls
extern __attribute__((visibility("hidden"))) EventSlots<64, 2> mvs_prof_dominant;      // [begin, end] of the fused 3dconv0_1 + 1_0 pass
extern __attribute__((visibility("hidden"))) EventSlots<32, 22> mvs_prof_layers;       // [begin, end] per layer, weight order
extern __attribute__((visibility("hidden"))) EventSlots<32, 4> mvs_prof_stages;        // boundaries of the three stages of mvs_depth_from_features_f32
