// The stream sets of the recurrent sweep (mvs_gru_prepare / mvs_gru_release): calibration, slots, lookup.
// Cell 1 (the recurrent chain) runs on the CALLER's stream; cell 2, cell 3 (+ WTA) and the per-batch producer (cost slices +
// hoisted x-part of cell 1) run on three library-owned streams.  WHICH streams matters (round 3, profiles/r03_gru_bisect*.log,
// r03_pipe_probe.txt): the runtime binds a stream to a hardware queue on its first use, hardware queues are dealt round-robin
// over the FOUR compute pipes of the command processor in creation order (queue ids k and k + 4 share a pipe), and a queue
// that is stalled on an event wait -- or busy with the chain's ~8 dispatches per plane -- slows the dispatches of the other
// queue of its pipe 3-19x (a chain of 200 dependent empty kernels: 0.31 ms alone, 0.59 ms with any other queue stalled,
// 1.6-5.8 ms with the stalled queue on the same pipe).  Round 2 created three side streams on first use and took whatever
// queue ids came: with the caller's queue created first and nothing else in the process they were k+1..k+3 (23 ms per c3
// depth map); with ONE unrelated stream used in between (any torch.cuda.Stream that ran a kernel) the producer or cell 3
// landed on the chain's pipe and the same sweep took 44 ms.  Now: eight candidate streams per caller stream, four of the high
// and four of the low priority class, hardware queues created back to back (ids k..k+7: the candidates of a class sit on four
// different pipes, high[m] and low[m] on the same one), and ONE calibration on first use finds the candidate pipe the
// caller's queue lives on by measurement (pipe_of_caller): cells 2 / 3 take two high-priority candidates and the producer a
// low-priority one on the three OTHER pipes.
#include "conv_common.h"      // mvs_stream_set_side
#include "gru_common.h"
#include <cstdio>
#include <mutex>

namespace {
__global__ void gru_probe_empty_kernel() {}
__global__ void gru_probe_spin_kernel(long long ticks) {       // bounded: leaves after `ticks` of the 100 MHz wall clock or 2^26 polls
    const long long t0 = wall_clock64();
    for (int i = 0; i < (1 << 26); ++i)
        if (wall_clock64() - t0 > ticks) break;
}

// Index m (0..3) of the candidate pair (high[m], low[m]) that shares a compute pipe with `caller`, or -1.  While the caller
// waits on an event (as it does at the end of every sweep) a chain of 100 dependent empty kernels runs on each candidate in
// turn: the candidate on the caller's pipe takes several times as long as the others.  One-off, ~10 ms, synchronises.
int pipe_of_caller(hipStream_t caller, GruStreams& g) {
    hipEvent_t t0, t1, gate;
    if (hipEventCreate(&t0) != hipSuccess || hipEventCreate(&t1) != hipSuccess ||
        hipEventCreateWithFlags(&gate, hipEventDisableTiming) != hipSuccess) return -1;
    auto slowest = [&](const float* t) {                         // the one of four that stands out (> 1.7 x the median), or -1
        int m = 0;
        for (int i = 1; i < 4; ++i) if (t[i] > t[m]) m = i;
        float o[3]; int n = 0;
        for (int i = 0; i < 4; ++i) if (i != m) o[n++] = t[i];
        const float med = o[0] > o[1] ? (o[1] > o[2] ? o[1] : (o[0] > o[2] ? o[2] : o[0])) : (o[0] > o[2] ? o[0] : (o[1] > o[2] ? o[2] : o[1]));
        return t[m] > 1.7f * med ? m : -1;
    };
    // high[m] and low[m] share a pipe by construction, so the two classes must name the same m: a measurement disturbed by other
    // work on the GPU (another process, the application's own streams) is repeated, up to three times
    int mh = -1, ml = -1;
    bool ok = true;
    for (int attempt = 0; attempt < 3 && ok; ++attempt) {
        ok = hipStreamSynchronize(caller) == hipSuccess;         // the caller must be idle, or it would not be stalled on OUR wait
        for (int j = 0; ok && j < 8; ++j) {
            hipStream_t sj = g.cand[j], sg = g.cand[(j + 1) & 7];    // the gate holds the chain back while the host enqueues it
            gru_probe_spin_kernel<<<1, 64, 0, sg>>>(60000);          // 0.6 ms
            ok = ok && hipEventRecord(gate, sg) == hipSuccess && hipStreamWaitEvent(sj, gate, 0) == hipSuccess &&
                 hipEventRecord(t0, sj) == hipSuccess;
            for (int k = 0; k < 100; ++k) gru_probe_empty_kernel<<<1, 64, 0, sj>>>();
            ok = ok && hipEventRecord(t1, sj) == hipSuccess && hipStreamWaitEvent(caller, t1, 0) == hipSuccess &&
                 hipEventSynchronize(t1) == hipSuccess && hipStreamSynchronize(sg) == hipSuccess;
            float ms = 0.f;
            ok = ok && hipEventElapsedTime(&ms, t0, t1) == hipSuccess;
            g.probe_us[j] = ms * 1e3f;
        }
        if (!ok) break;
        mh = slowest(g.probe_us); ml = slowest(g.probe_us + 4);
        if (mh == ml && mh >= 0) break;                          // both classes agree
    }
    (void)hipEventDestroy(t0); (void)hipEventDestroy(t1); (void)hipEventDestroy(gate);
    if (!ok) return -1;
    if (mh >= 0 && ml >= 0 && mh != ml) return g.probe_us[mh] / g.probe_us[(mh + 1) & 3] > g.probe_us[4 + ml] / g.probe_us[4 + ((ml + 1) & 3)] ? mh : ml;
    return mh >= 0 ? mh : ml;                                    // the same pipe by construction; either measurement will do
}

// One set per (device, caller stream) -- sweeps of different reference views in flight on different caller streams must not
// share side streams, or they would serialise behind each other.  Sets are created and calibrated by mvs_gru_prepare() ONLY
// (round 4: the sweep itself used to do this on first use, i.e. create streams and synchronise inside an entry point whose
// header promises neither, and invalidate a hipGraph capture it was first called under); the sweep looks its set up and never
// creates one; mvs_gru_release() gives a slot back.
struct GruSlot { int dev; hipStream_t caller; GruStreams g; int state; };      // state: 0 free, 1 ready
constexpr int GRU_SLOTS = 16;
GruSlot g_slots[GRU_SLOTS];
std::mutex g_slots_mu;

void gru_destroy(GruStreams& g) {                       // whatever of a set exists (also a half-built one)
    for (int i = 0; i < 8; ++i) if (g.cand[i]) { (void)hipStreamSynchronize(g.cand[i]); (void)hipStreamDestroy(g.cand[i]); g.cand[i] = nullptr; }
    auto ev = [](hipEvent_t& e) { if (e) { (void)hipEventDestroy(e); e = nullptr; } };
    ev(g.fork);
    for (int i = 0; i < 2; ++i) { ev(g.xready[i]); ev(g.xdone[i]); for (int j = 0; j < RG; ++j) { ev(g.ready[i][j]); ev(g.read[i][j]); } }
    for (int i = 0; i < 3; ++i) { ev(g.join[i]); g.s[i] = nullptr; }
}

// Creates and calibrates the set of `caller` on the current device (idempotent).  Synchronises `caller` and the new streams.
int gru_prepare(hipStream_t caller) {
    int dev = 0;
    hipError_t e = hipGetDevice(&dev);
    if (e != hipSuccess) return (int)e;
    if (mvs_is_capturing(caller)) return MVS_E_NOT_PREPARED;   // prepare synchronises
    std::lock_guard<std::mutex> lock(g_slots_mu);
    int free_slot = -1;
    for (int i = 0; i < GRU_SLOTS; ++i) {
        if (g_slots[i].state == 1 && g_slots[i].dev == dev && g_slots[i].caller == caller) return 0;
        if (g_slots[i].state == 0 && free_slot < 0) free_slot = i;
    }
    if (free_slot < 0) return MVS_E_NO_SLOT;               // GRU_SLOTS caller streams hold a set: release one first
    GruSlot& sl = g_slots[free_slot];
    sl = GruSlot{};
    sl.dev = dev; sl.caller = caller;
    GruStreams& g = sl.g;
    int lo = 0, hi = 0;
    if (hipDeviceGetStreamPriorityRange(&lo, &hi) != hipSuccess) lo = hi = 0;   // lo = least urgent: the batch producer yields to the cells
    e = hipSuccess;
    for (int i = 0; e == hipSuccess && i < 8; ++i) e = hipStreamCreateWithPriority(&g.cand[i], hipStreamNonBlocking, i < 4 ? hi : lo);
    // first use = hardware queue creation: touch the eight candidates now, in order, with nothing in between
    for (int i = 0; e == hipSuccess && i < 8; ++i) {
        gru_probe_empty_kernel<<<1, 64, 0, g.cand[i]>>>();
        e = hipStreamSynchronize(g.cand[i]);
    }
    auto ev = [&](hipEvent_t* ep) { if (e == hipSuccess) e = hipEventCreateWithFlags(ep, hipEventDisableTiming); };
    ev(&g.fork);
    for (int i = 0; i < 2; ++i) { ev(&g.xready[i]); ev(&g.xdone[i]); for (int j = 0; j < RG; ++j) { ev(&g.ready[i][j]); ev(&g.read[i][j]); } }
    for (int i = 0; i < 3; ++i) ev(&g.join[i]);
    if (e != hipSuccess) { gru_destroy(g); return (int)e; }
    g.pipe_of_caller = pipe_of_caller(caller, g);
    if (g.pipe_of_caller < 0) {
        // no candidate pipe stood out (other work on the GPU during the ~10 ms measurement, or a runtime that deals queues
        // differently): the sweep still runs as a wavefront, but one of its side streams may share the caller's compute
        // pipe -- the 2x slow layout of round 2 (profiles/r03_gru_bisect*.log).  Say so, once per process.
        static bool told = false;
        if (!told) { told = true; fprintf(stderr, "mvsnet_hip: mvs_gru_prepare: the stream-layout calibration was inconclusive (chains %.0f %.0f %.0f %.0f | %.0f %.0f %.0f %.0f us); "
                                                  "the recurrent sweep may run up to 2x slower on this stream -- call mvs_gru_release + mvs_gru_prepare again on an idle GPU\n",
                                          g.probe_us[0], g.probe_us[1], g.probe_us[2], g.probe_us[3], g.probe_us[4], g.probe_us[5], g.probe_us[6], g.probe_us[7]); }
    }
    int pick[3], n = 0;                                  // the three candidate pipes the caller's queue is NOT on
    for (int m = 0; m < 4 && n < 3; ++m) if (m != g.pipe_of_caller) pick[n++] = m;
    g.s[0] = g.cand[pick[0]]; g.s[1] = g.cand[pick[1]]; g.s[2] = g.cand[4 + pick[2]];
    for (int i = 0; i < 8; ++i)                          // the five candidates that lost go back (their hardware queues with them)
        if (g.cand[i] != g.s[0] && g.cand[i] != g.s[1] && g.cand[i] != g.s[2]) { (void)hipStreamDestroy(g.cand[i]); g.cand[i] = nullptr; }
    sl.state = 1;
    return 0;
}

int gru_release(hipStream_t caller) {
    int dev = 0;
    hipError_t e = hipGetDevice(&dev);
    if (e != hipSuccess) return (int)e;
    std::lock_guard<std::mutex> lock(g_slots_mu);
    for (int i = 0; i < GRU_SLOTS; ++i)
        if (g_slots[i].state == 1 && g_slots[i].dev == dev && g_slots[i].caller == caller) {
            gru_destroy(g_slots[i].g);                   // waits for the side streams' work
            g_slots[i].state = 0;
            return 0;
        }
    return MVS_E_BADARG;
}

}  // namespace

GruStreams* mvs_gru_find(hipStream_t caller) {
    int dev = 0;
    if (hipGetDevice(&dev) != hipSuccess) return nullptr;
    std::lock_guard<std::mutex> lock(g_slots_mu);
    for (int i = 0; i < GRU_SLOTS; ++i)
        if (g_slots[i].state == 1 && g_slots[i].dev == dev && g_slots[i].caller == caller) return &g_slots[i].g;
    return nullptr;
}

// One side stream (and a fork / join event pair) of the set mvs_gru_prepare made for `caller`, for other users of the library's
// stream sets (regnet.hip: a branch layer beside the low-resolution chain); false without a set.
bool mvs_stream_set_side(hipStream_t caller, hipStream_t* side, hipEvent_t* fork, hipEvent_t* join) {
    GruStreams* g = mvs_gru_find(caller);
    if (!g) return false;
    *side = g->s[0]; *fork = g->fork; *join = g->join[0];
    return true;
}

extern "C" int mvs_gru_prepare(void* stream) { return gru_prepare(mvs_stream(stream)); }
extern "C" int mvs_gru_release(void* stream) { return gru_release(mvs_stream(stream)); }

extern "C" int mvs_gru_stream_layout(void* stream, int* pipe_of_caller_out, float* probe_us_out) {
    GruStreams* gs = mvs_gru_find(mvs_stream(stream));
    if (!gs) return MVS_E_NOT_PREPARED;
    if (pipe_of_caller_out) *pipe_of_caller_out = gs->pipe_of_caller;
    if (probe_us_out) for (int i = 0; i < 8; ++i) probe_us_out[i] = gs->probe_us[i];
    return 0;
}
