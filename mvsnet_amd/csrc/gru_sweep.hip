// The recurrent sweep's orchestration: routing, the fused pipeline's and the four-stream wavefront's enqueue order, the join.
// No kernel and no launch here: the kernels and their launchers are in gru.hip, gru_mfma.hip and gru_fused.hip, the stream
// sets in gru_streams.hip, what they share in gru_common.h.
#include "gru_common.h"
#include <cstdio>

// shape part of the routing decision of mvs_gru_wta*_f32 (exported for the CPU-side routing test; tests/test_abi_and_io.py)
extern "C" int mvs_gru_fused_route(int C, int f1, int f2, int f3, size_t view_block_bytes) {
    return C == 32 && f1 == 16 && f2 == 4 && f3 == 2 && view_block_bytes < ((size_t)1 << 31);
}

extern "C" size_t mvs_gru_workspace_bytes(int H, int W, int C, int f1, int f2, int f3) {
    return carve(nullptr, H, W, C, f1, f2, f3).bytes;
}

// Formulation of cell 1 on the MFMA kernels: 1 = hoisted x-part (its own batched launches on the producer stream + per-plane
// kernels over the 16 state channels), 2 = full 48-channel per-plane kernels, 0 = by view count (hoisted for one view: the
// chain's latency paces a single sweep; full for two or more: B x 950 tiles per launch hide it, and the hoisted form's px
// tensor -- 46 MB of traffic per plane and view -- and its producer competing for the matrix pipes are what is left to save).
// Both give the same bits (gru_mfma.hip, SPLIT accumulators).
static std::atomic<int> g_gru_form{0};                 // read ONCE per sweep (a sweep in flight keeps the formulation it started with)
extern "C" int mvs_gru_set_formulation(int form) {
    if (form < 0 || form > 3) return MVS_E_BADARG;
    g_gru_form.store(form);
    return 0;
}

namespace {

// One sweep: what the caller passed, the carved workspace and the routing decision.  Filled by mvs_gru_wta_batch_f32.
struct Sweep {
    int view_num, depth_num, H, W, C, F[3];
    size_t hw;
    Views vw;                                        // reference views per launch; byte stride between their workspace blocks
    char* base; GruWs ws;                            // view 0's workspace block and its carving; view v's tensors are v * ws.bytes further
    const float* const* params; const float* depth_values;
    const float* const* ref; const float* const* src; const float* const* transforms;
    hipStream_t st;                                  // the caller's stream carries cell 1, the recurrent chain
    bool fused, mfma1, hoist;
    int route[3];                                    // wavefront, per cell: 0 generic, 1 MFMA (cell 1), 2 small-cell kernels
    GruStreams* gs;                                  // the stream set this sweep uses, or null: everything on the caller's stream
    bool forked;                                     // side streams wait on gs->fork: join_side_streams() has work to do
};

template <class T> T* vp(const Sweep& sw, T* p, int v) { return (T*)((char*)p + (size_t)v * sw.vw.stride); }     // host-side view pointer
int zero(const Sweep& sw, float* p, size_t nfloat) { return mvs_gru_zero_views(p, nfloat, sw.vw, sw.st); }

// The routing decision, made before anything of the sweep proper is enqueued.
void route_sweep(Sweep& sw) {
    const int C = sw.C, f1 = sw.F[0];
    // cell 1 (90 % of the MACs) runs on the fp32-MFMA kernels when its shape fits their tiling
    sw.mfma1 = (mvs_get_conv_impl() != MVS_CONV_IMPL_SCALAR) && C == 32 && f1 == 16;
    const int form = g_gru_form.load();
    // The fused sweep (gru_fused.hip): the reference's filter counts (model.py:641-660, 'normal' mode) at 32 feature channels --
    // all three cells, prob_conv and the winner-take-all update in two launches per plane on the caller's stream alone.
    // Formulation 0 takes it whenever the shape fits -- also for ONE eager view on a stream that has a stream set, where the round-4
    // wavefront with the hoisted x-part (formulation 1) is still 3-4 % faster (c3, same box: 21.8 against 22.6 ms): a batch of views
    // must give the single view's bits, and from two views per sweep on, and under hipGraph capture (23.4 against 37 ms), the fused
    // sweep is the faster or equal one (profiles/r05_gru_ab_forms.txt).
    // The fused kernels address a whole view's workspace block through one buffer resource with 32-bit byte offsets: blocks of
    // 2 GiB and more (~10.2 KB per pixel: feature maps above ~210 k pixels, e.g. 576 x 384) take the wavefront route, which
    // addresses every tensor by itself -- decided HERE, before anything is enqueued.
    sw.fused = mvs_gru_fused_route(C, f1, sw.F[1], sw.F[2], sw.vw.stride) && sw.mfma1 && (form == 0 || form == 3);
    if (sw.fused) {
        // The -variance cost slices (model.py:680-693,698) come in batches of XB planes from one depth-sweep launch per view.  With a
        // stream set (mvs_gru_prepare) the producer runs ONE BATCH AHEAD on the set's low-priority stream, into the other half of
        // a two-batch buffer (the px tensor of the wavefront formulations, unused here): its waves fill the issue slots the
        // recurrent launches leave idle instead of standing in line with them (31 of 287 us per plane at four views).  Without a
        // set, and under hipGraph capture, everything stays on the caller's stream.
        sw.gs = (!mvs_is_capturing(sw.st) && sw.depth_num > XB && !mvs_hook(MVS_HOOK_GRU_ONE_STREAM)) ? mvs_gru_find(sw.st) : nullptr;
        return;
    }
    sw.hoist = sw.mfma1 && (form == 1 || (form == 0 && sw.vw.n == 1));
    // which kernels each cell gets; the generic conv + gates route shares rh / u and stays on one stream
    const int cins[3] = {C, f1, sw.F[1]};
    for (int k = 0; k < 3; ++k) sw.route[k] = (k == 0 && sw.mfma1) ? 1 : mvs_gru_small_covers(cins[k], sw.F[k]) ? 2 : 0;
    const bool wavefront = sw.route[0] && sw.route[1] && sw.route[2] && sw.depth_num > 2 * PG &&
                           !mvs_hook(MVS_HOOK_GRU_ONE_STREAM);      // test hook (parity of the one-stream sweep), read per sweep
    // Under hipGraph capture the WAVEFRONT formulations go to the caller's stream alone.  Root cause of the round-4 host crash
    // (profiles/r05_capture_wavefront_root_cause.txt): hip::Stream::EndCapture() of the HIP runtime the PyTorch wheel bundles
    // (libamdhip64 7.0.70002, the runtime every Python process of this library runs on) recurses without bound once two captured
    // streams wait on each other's events in BOTH directions -- which the ring's backward waits (`read`) do from the fifth group on;
    // tools/capture_wavefront_repro.hip reproduces it with empty kernels (stack overflow from 40 planes on with that runtime, clean
    // with /opt/rocm 7.2's; stream flags, priorities, event re-use and capture mode do not matter).  Nothing in this event graph is
    // illegal.  The default formulation (gru_fused.hip) has no cross-stream pattern and is captured at full speed.
    const bool capturing = mvs_is_capturing(sw.st);
    // (tools/capture_wavefront_repro.hip is the standalone evidence; the library has no switch that re-enables the crashing path)
    sw.gs = (wavefront && !capturing) ? mvs_gru_find(sw.st) : nullptr;
    if (wavefront && !capturing && !sw.gs) {
        // no side streams for this caller stream: this entry point creates none (mvs_gru_prepare does) -- run the sweep on the
        // caller's stream alone (same results, ~1.7x the time at 400 x 300) and say so once.
        static std::atomic<bool> told{false};
        if (!told.exchange(true))
            fprintf(stderr, "mvsnet_hip: mvs_gru_wta*_f32 on a stream without mvs_gru_prepare(): the recurrent sweep runs on this stream "
                            "alone (same results, slower); call mvs_gru_prepare(stream) once per caller stream\n");
    }
}

// Join on EVERY exit after the fork: also when a launch failed half-way the caller's stream must stay ordered
// after whatever the side streams were given -- the caller frees or re-uses the feature maps and the workspace in stream order.
// The streams that were forked: the producer's in the fused sweep, all three in the wavefront.
int join_side_streams(const Sweep& sw, int rc) {
    if (!sw.forked) return rc;
    for (int i = sw.fused ? 2 : 0; i < 3; ++i) {
        hipError_t e1 = hipEventRecord(sw.gs->join[i], sw.gs->s[i]);
        if (e1 == hipSuccess) e1 = hipStreamWaitEvent(sw.st, sw.gs->join[i], 0);
        if (e1 != hipSuccess && rc == 0) rc = (int)e1;
    }
    return rc;
}

// the WTA operands of plane dd (cell 3's prob_conv, the planes' depths per view, the accumulators); dd = -1: no plane
WtaFold wta_of_plane(const Sweep& sw, int dd) {
    WtaFold w = {sw.params[30], sw.params[31], {}, sw.ws.max_prob, sw.ws.depth, sw.ws.exp_sum};
    for (int v = 0; v < sw.vw.n; ++v) w.depth_value[v] = dd >= 0 ? sw.depth_values[(size_t)v * sw.depth_num + dd] : 0.f;
    return w;
}

// ---- the fused sweep: two launches per plane on the caller's stream, the cost slices one batch ahead on the producer's ----------

// the cost slices of batch bidx: with a producer stream, the halves of a two-batch buffer (the px tensor) in turn
float* fused_x_batch(const Sweep& sw, int bidx) { return sw.gs ? sw.ws.px + (size_t)(bidx & 1) * XB * sw.hw * sw.C : sw.ws.x; }

int fused_produce(const Sweep& sw, int bidx, hipStream_t s, int threads) {
    const int t0 = bidx * XB, nb = sw.depth_num - t0 < XB ? sw.depth_num - t0 : XB;
    for (int v = 0; v < sw.vw.n; ++v) {
        const int r = mvs_cost_volume_threads_f32(sw.ref[v], sw.src[v], sw.transforms[v], sw.view_num, sw.depth_num, t0, nb, sw.H, sw.W, sw.C,
                                                  /*variant*/ 1, /*negate*/ 1, /*border*/ 0, vp(sw, fused_x_batch(sw, bidx), v), threads, s);
        if (r) return r;
    }
    return 0;
}

int fused_sweep(Sweep& sw) {
    const GruWs& ws = sw.ws;
    const hipStream_t st = sw.st;
    GruStreams* pg = sw.gs;
    const int depth_num = sw.depth_num;
    int rc;
    hipError_t e0;
    if ((rc = mvs_gru1_full_weights(sw.params[0], sw.params[6], sw.C, sw.F[0], ws.wfg, ws.wfo, st))) return rc;
    if ((rc = mvs_gru_fused_prepare_weights(sw.params, ws, st))) return rc;
    for (int k = 0; k < 3; ++k) if ((rc = zero(sw, ws.h[k][1], sw.hw * sw.F[k]))) return rc;      // s(-1) = 0 lives in h[k][1]; h[k][0] zeroed by the caller
    if ((rc = zero(sw, (float*)ws.fstats, (size_t)GRU_FUSED_RING * GRU_FUSED_ROW * 2))) return rc;
    const hipStream_t sx = pg ? pg->s[2] : st;
    // (on the producer stream: 128-thread workgroups, 16 KB of LDS -- they fit beside a fused workgroup)
    const int small_wg = mvs_hook(MVS_HOOK_GRU_PRODUCER_THREADS);      // A/B hook, validated by mvs_set_test_hook (64 / 128 / 192 / 256)
    if (pg) {
        if ((e0 = hipEventRecord(pg->fork, st)) != hipSuccess) return (int)e0;
        sw.forked = true;
        if ((e0 = hipStreamWaitEvent(sx, pg->fork, 0)) != hipSuccess) return (int)e0;
        if ((rc = fused_produce(sw, 0, sx, small_wg))) return rc;
        if ((e0 = hipEventRecord(pg->xready[0], sx)) != hipSuccess) return (int)e0;
    }
    for (int t = 0; t < depth_num + 3; ++t) {
        if (t % XB == 0) {
            const int bidx = t / XB;
            if (t < depth_num) {
                if (!pg) { if ((rc = fused_produce(sw, bidx, st, 256))) return rc; }
                else {
                    if ((e0 = hipStreamWaitEvent(st, pg->xready[bidx & 1], 0)) != hipSuccess) return (int)e0;
                    if ((bidx + 1) * XB < depth_num) {       // the next batch into the other half, once its readers (batch bidx - 1) are done
                        if (bidx >= 1 && ((e0 = hipEventRecord(pg->xdone[(bidx + 1) & 1], st)) != hipSuccess ||
                                          (e0 = hipStreamWaitEvent(sx, pg->xdone[(bidx + 1) & 1], 0)) != hipSuccess)) return (int)e0;
                        if ((rc = fused_produce(sw, bidx + 1, sx, small_wg))) return rc;
                        if ((e0 = hipEventRecord(pg->xready[(bidx + 1) & 1], sx)) != hipSuccess) return (int)e0;
                    }
                }
            }
            // LayerNorm-sum rows of planes t + XB .. t + 2 XB - 1 (their previous users, planes 64 earlier, are long done)
            if (t > 0 && (rc = zero(sw, (float*)gru_fused_row(ws, t + XB), (size_t)XB * GRU_FUSED_ROW * 2))) return rc;
        }
        const int tx = t < depth_num ? t : depth_num - 1;
        if ((rc = mvs_gru_fused_step(ws, sw.base, sw.params, t, depth_num, fused_x_batch(sw, tx / XB) + (size_t)(tx % XB) * sw.hw * sw.C,
                                     sw.H, sw.W, sw.vw.n, sw.vw.stride, sw.depth_values, st))) return rc;
    }
    return 0;
}

// ---- the wavefront: cell 1 on the caller's stream, cells 2 / 3 and the per-batch producer on the set's three ----------------

// the wavefront's LayerNorm sums of cell k, plane d: [gates: 2 groups x 2 | out: 1 x 2] in a ring of SB + 1 batches
double* plane_stats(const Sweep& sw, int d, int k) { return sw.ws.stats + (size_t)(((d / XB) % (SB + 1)) * XB + d % XB) * 18 + 6 * k; }

// The cost slices of the batch that holds plane d.  Hoisted form: one buffer -- the x-part launches that read it follow the
// slices' launch on the producer stream, and what the chain reads (px) has two halves.  Full form: the chain reads the
// slices themselves while the producer writes the next batch, so they alternate between two halves too (the memory of
// the unused px tensor: 2 * XB * 48 floats per pixel against the 2 * XB * C needed).
float* wave_x_batch(const Sweep& sw, int d) {
    return (sw.mfma1 && !sw.hoist && sw.gs) ? sw.ws.px + (size_t)((d / XB) & 1) * XB * sw.hw * sw.C : sw.ws.x;
}

// Per batch: x = -variance cost slices (model.py:680-693,698) and, for the MFMA cell 1, the x halves of
// its two convolutions for the whole batch (gru_mfma.hip: x-part hoisting).
int produce_batch(const Sweep& sw, int d0, hipStream_t s) {
    const GruWs& ws = sw.ws;
    const int H = sw.H, W = sw.W, C = sw.C, f1 = sw.F[0];
    const int nb = sw.depth_num - d0 < XB ? sw.depth_num - d0 : XB;
    for (int v = 0; v < sw.vw.n; ++v) {
        int r2 = mvs_cost_volume_f32(sw.ref[v], sw.src[v], sw.transforms[v], sw.view_num, sw.depth_num, d0, nb, H, W, C, /*variant*/ 1,
                                     /*negate*/ 1, /*border*/ 0, vp(sw, wave_x_batch(sw, d0), v), s);
        if (r2) return r2;
        if (sw.hoist && (r2 = mvs_gru1_xpart_mfma(vp(sw, wave_x_batch(sw, d0), v), ws.wx, ws.wx + (size_t)9 * C * 2 * f1, sw.params[1], sw.params[7], H, W, nb,
                                                  vp(sw, ws.px, v) + (size_t)((d0 / XB) & 1) * XB * sw.hw * 3 * f1, s))) return r2;
    }
    return 0;
}

// start of a batch of XB planes (on cell 1's stream, before its first plane of the batch)
int batch_start(const Sweep& sw, int d) {
    GruStreams* gs = sw.gs;
    const hipStream_t st = sw.st;
    const int half = (d / XB) & 1;
    // LayerNorm sums of this batch (other slots of the ring may still be in use by cells 2 / 3 of earlier planes: cell 3
    // lags cell 1 by fewer than 2 * RG groups = at most SB batches)
    int r;
    hipError_t e;
    if ((r = zero(sw, (float*)plane_stats(sw, d, 0), (size_t)XB * 18 * 2))) return r;
    if (!(gs && sw.mfma1)) return produce_batch(sw, d, st);
    // the producer runs one batch ahead on its own (low-priority) stream: 2/3 of cell 1's MACs leave the
    // recurrent chain
    hipStream_t sx = gs->s[2];
    if (d == 0) {
        if ((r = produce_batch(sw, 0, sx))) return r;
        if ((e = hipEventRecord(gs->xready[0], sx)) != hipSuccess) return (int)e;
    }
    if ((e = hipStreamWaitEvent(st, gs->xready[half], 0)) != hipSuccess) return (int)e;
    if (d + XB < sw.depth_num) {                     // next batch into the other half, once its readers are done
        if (d >= XB && (e = hipStreamWaitEvent(sx, gs->xdone[half ^ 1], 0)) != hipSuccess) return (int)e;
        if ((r = produce_batch(sw, d + XB, sx))) return r;
        if ((e = hipEventRecord(gs->xready[half ^ 1], sx)) != hipSuccess) return (int)e;
    }
    return 0;
}

// Cell k of plane d as its kernels see it.  `prev` (non-null: plane d-1 left its blend to this plane's gate convolution) points
// into the struct: pass it by reference.
struct CellPlane {
    int k, d, cin, f;
    const float* const* p;                           // the cell's 10 parameter tensors
    const float* xin; float* h; float* g; float* c; double* sg; double* so;
    PrevPlane prev_in; const PrevPlane* prev;
};

// cell 1 on the full 48-channel MFMA kernels
int cell1_full(const Sweep& sw, const CellPlane& cp, hipStream_t s) {
    const GruWs& ws = sw.ws; const float* const* p = cp.p;
    int r;
    if (cp.prev)
        r = mvs_gru1_gates_full_blend_mfma(cp.xin, cp.prev->h_before, cp.c, cp.prev->g, cp.prev->so, cp.prev->sg + 2, p[8], p[9], p[4], p[5], cp.h,
                                           ws.wfg, p[1], sw.H, sw.W, cp.g, cp.sg, sw.vw.n, sw.vw.stride, s);
    else
        r = mvs_gru1_gates_full_mfma(cp.xin, cp.h, ws.wfg, p[1], sw.H, sw.W, cp.g, cp.sg, sw.vw.n, sw.vw.stride, s);
    if (r) return r;
    return mvs_gru1_out_full_mfma(cp.xin, cp.h, cp.g, cp.sg, p[2], p[3], ws.wfo, p[7], sw.H, sw.W, cp.c, cp.so, sw.vw.n, sw.vw.stride, s);
}

// cell 1 with the hoisted x-part: per-plane MFMA kernels over the 16 state channels
int cell1_hoisted(const Sweep& sw, const CellPlane& cp, hipStream_t s) {
    const GruWs& ws = sw.ws; const float* const* p = cp.p;
    const float* px_d = ws.px + ((size_t)((cp.d / XB) & 1) * XB + cp.d % XB) * sw.hw * 3 * sw.F[0];
    int r;
    if (cp.prev)
        r = mvs_gru1_gates_h_blend_mfma(cp.prev->h_before, cp.c, cp.prev->g, cp.prev->so, cp.prev->sg + 2, p[8], p[9], p[4], p[5], cp.h,
                                        ws.wgh, px_d, sw.H, sw.W, cp.g, cp.sg, sw.vw.n, sw.vw.stride, s);
    else
        r = mvs_gru1_gates_h_mfma(cp.h, ws.wgh, px_d, sw.H, sw.W, cp.g, cp.sg, sw.vw.n, sw.vw.stride, s);
    if (r) return r;
    return mvs_gru1_out_h_mfma(cp.h, cp.g, cp.sg, p[2], p[3], ws.woh, px_d, sw.H, sw.W, cp.c, cp.so, sw.vw.n, sw.vw.stride, s);
}

// shape-generic route: one view per launch
int cell_generic(const Sweep& sw, const CellPlane& cp, hipStream_t s) {
    const GruWs& ws = sw.ws; const float* const* p = cp.p;
    const int H = sw.H, W = sw.W, k = cp.k, f = cp.f;
    int r;
    for (int v = 0; v < sw.vw.n; ++v) {
        if ((r = mvs_gru_conv2d(vp(sw, cp.xin, v), cp.cin, vp(sw, cp.h, v), f, p[0], p[1], H, W, 2 * f, vp(sw, ws.g[k], v), vp(sw, cp.sg, v), 2, s))) return r;
        if ((r = mvs_gru_gates_f32(vp(sw, ws.g[k], v), vp(sw, cp.sg, v), p[2], p[3], p[4], p[5], vp(sw, cp.h, v), H, W, f, vp(sw, ws.rh, v), vp(sw, ws.u, v), s))) return r;
        if ((r = mvs_gru_conv2d(vp(sw, cp.xin, v), cp.cin, vp(sw, ws.rh, v), f, p[6], p[7], H, W, f, vp(sw, cp.c, v), vp(sw, cp.so, v), 1, s))) return r;
    }
    return 0;
}

// cell k of plane d on stream s: gate conv, candidate conv, blend (+ prob / WTA after cell 3)
int cell_plane(const Sweep& sw, int k, int d, hipStream_t s) {
    const GruWs& ws = sw.ws;
    GruStreams* gs = sw.gs;
    const int ring = RG * PG, slot = d % XB, depth_num = sw.depth_num;
    // On the wavefront: the blend of a plane is folded into the NEXT plane's gate convolution (its
    // staging forms the state it convolves) except at the end of a synchronisation group, where the next cell
    // (and the WTA update) are about to read the state: 3 of 4 blend launches disappear.  The gate buffer
    // alternates, a folded gate convolution still reads the previous plane's update gate while it writes its own.
    const bool fold = sw.route[k] != 0 && gs != nullptr;           // (the MFMA cell 1 folds its blend the same way)
    const bool fused_in = fold && d % PG != 0;               // plane d-1 left its blend to this plane
    const bool blend_now = !fold || d % PG == PG - 1 || d == depth_num - 1;
    CellPlane cp = {};
    cp.k = k; cp.d = d; cp.cin = k == 0 ? sw.C : sw.F[k - 1]; cp.f = sw.F[k];
    cp.p = sw.params + 10 * k;
    cp.sg = plane_stats(sw, d, k); cp.so = cp.sg + 4;
    cp.h = ws.h[k][d % ring];
    float* hn = ws.h[k][(d + 1) % ring];
    cp.g = (fold && (d & 1)) ? ws.g2[k] : ws.g[k];
    cp.c = ws.c[k];
    if (fused_in) {
        const int dp = d - 1;
        double* sgp = plane_stats(sw, dp, k);
        cp.prev_in = {ws.h[k][dp % ring], (dp & 1) ? ws.g2[k] : ws.g[k], sgp, sgp + 4};
        cp.prev = &cp.prev_in;
    }
    cp.xin = k == 0 ? wave_x_batch(sw, d) + (size_t)slot * sw.hw * sw.C : ws.h[k - 1][(d + 1) % ring];
    const float* const* p = cp.p;
    int r;
    hipError_t e;
    bool wta_folded = false;
    if (sw.route[k] == 1) {
        if ((r = sw.hoist ? cell1_hoisted(sw, cp, s) : cell1_full(sw, cp, s))) return r;
        if (gs && (slot == XB - 1 || d == depth_num - 1) && (e = hipEventRecord(gs->xdone[(d / XB) & 1], s)) != hipSuccess) return (int)e;
    } else if (sw.route[k] == 2) {
        // cell 3: the previous plane's prob_conv + winner-take-all update rides in this plane's gate convolution, which forms
        // that plane's final state in its tile anyway
        const WtaFold wfold = wta_of_plane(sw, d - 1);
        wta_folded = k == 2 && fused_in;
        if ((r = mvs_gru_small_cell(cp.cin, cp.f, cp.xin, cp.h, p, sw.H, sw.W, cp.g, cp.c, cp.sg, cp.so, cp.prev, sw.vw, s, wta_folded ? &wfold : nullptr))) return r;
    } else if ((r = cell_generic(sw, cp, s))) return r;
    // plane d-1's state exists since this plane's gate convolution
    if (k == 2 && fused_in && !wta_folded && (r = mvs_gru_prob_wta_views(cp.h, sw.F[2], wta_of_plane(sw, d - 1), ws.reg, sw.H, sw.W, sw.vw, s))) return r;
    if (blend_now) {
        if ((r = mvs_gru_blend_views(cp.c, cp.so, p[8], p[9], cp.g, cp.sg + 2, p[4], p[5], sw.H, sw.W, cp.f, cp.h, hn, sw.vw, s))) return r;
        if (k == 2 && (r = mvs_gru_prob_wta_views(hn, sw.F[2], wta_of_plane(sw, d), ws.reg, sw.H, sw.W, sw.vw, s))) return r;
    }
    return (int)hipGetLastError();
}

// Wavefront over (plane, cell): cell k of plane d needs cell k-1 of plane d and cell k of plane d-1, so
// the three cells run on three streams, cell 1 of the next planes alongside cell 2 of these and cell 3 of
// the previous ones; the small kernels of cells 2 / 3 (launch-latency bound, a few workgroups per CU) then
// fill the machine under cell 1's kernels instead of serialising behind them.  A cross-stream dependency
// costs tens of microseconds of signal latency, as much as a cell's kernels for one plane, so the streams
// synchronise per GROUP of PG planes: states live in a ring of RG*PG planes (plane d reads h[k][d % ring], writes
// h[k][(d+1) % ring]); per group j, ready[k][j % RG] = cell k has written its states of group j, read[k][j % RG] =
// cell k+1 is done reading them (cell k may overwrite those ring slots in group j+RG).
// Several reference views (views > 1) ride in the SAME launches: every kernel of the sweep takes a view index from its
// grid, so the ~7 launches per plane, their ~5 us floors and the cross-stream waits are shared by `views` depth maps.
int wavefront_groups(const Sweep& sw) {
    GruStreams* gs = sw.gs;
    // (cells 2 and 3 sharing ONE side stream, round 4: 28.6 against 22.5 ms at one view, 74.4 against 71.5 ms per 4-view sweep)
    const hipStream_t sk[3] = {sw.st, gs->s[0], gs->s[1]};
    int rc;
    hipError_t e;
    for (int j = 0, d0 = 0; d0 < sw.depth_num; ++j, d0 += PG) {
        const int d1 = d0 + PG < sw.depth_num ? d0 + PG : sw.depth_num, jp = j % RG;
        for (int k = 0; k < 3; ++k) {
            hipStream_t s = sk[k];
            // the states cell k wrote in this group ...
            if (k > 0 && (e = hipStreamWaitEvent(s, gs->ready[k - 1][jp], 0)) != hipSuccess) return (int)e;
            // ... and the ring slots this cell is about to overwrite were read by cell k+1 RG groups ago
            if (k < 2 && j >= RG && (e = hipStreamWaitEvent(s, gs->read[k][jp], 0)) != hipSuccess) return (int)e;
            for (int d = d0; d < d1; ++d) {
                if (k == 0 && d % XB == 0 && (rc = batch_start(sw, d))) return rc;
                if ((rc = cell_plane(sw, k, d, s))) return rc;
            }
            if (k < 2 && (e = hipEventRecord(gs->ready[k][jp], s)) != hipSuccess) return (int)e;
            if (k > 0 && (e = hipEventRecord(gs->read[k - 1][jp], s)) != hipSuccess) return (int)e;
        }
    }
    return 0;
}

int wavefront_sweep(Sweep& sw) {
    const GruWs& ws = sw.ws;
    GruStreams* gs = sw.gs;
    int rc;
    hipError_t e;
    if (sw.mfma1) {                                      // prepared weights, shared by the views
        if (sw.hoist) rc = mvs_gru1_split_weights(sw.params[0], sw.params[6], sw.C, sw.F[0], ws.wx, ws.wgh, ws.woh, sw.st);
        else rc = mvs_gru1_full_weights(sw.params[0], sw.params[6], sw.C, sw.F[0], ws.wfg, ws.wfo, sw.st);
        if (rc) return rc;
    }
    if (!gs) {
        // one stream: planes in order, cells in order
        for (int d = 0; d < sw.depth_num; ++d) {
            if (d % XB == 0 && (rc = batch_start(sw, d))) return rc;
            for (int k = 0; k < 3; ++k) if ((rc = cell_plane(sw, k, d, sw.st))) return rc;
        }
        return 0;
    }
    if ((e = hipEventRecord(gs->fork, sw.st)) != hipSuccess) return (int)e;
    sw.forked = true;
    for (int i = 0; i < 3; ++i) if ((e = hipStreamWaitEvent(gs->s[i], gs->fork, 0)) != hipSuccess) return (int)e;
    return wavefront_groups(sw);
}

}  // namespace

extern "C" int mvs_gru_wta_batch_f32(const float* const* ref, const float* const* src, const float* const* transforms,
                                     int views, int view_num, int depth_num, int H, int W, int C, int f1, int f2,
                                     int f3, const float* const* params, const float* depth_values,
                                     void* workspace, size_t workspace_bytes, float* depth_out,
                                     float* prob_out, void* stream) {
    MVS_CHECK_ARG(ref && src && transforms && params && depth_values && workspace && depth_out && prob_out);
    MVS_CHECK_ARG(views >= 1 && views <= MVS_GRU_MAX_VIEWS);
    MVS_CHECK_ARG(view_num >= 2 && depth_num >= 1 && H > 0 && W > 0 && C > 0 && f1 > 0 && f2 > 0 && f3 > 0);
    if (f1 > 64 || f2 > 64 || f3 > 64) return MVS_E_SHAPE;     // gru_blend_fused_kernel keeps 2 x F LayerNorm affines in LDS ('fat': 32)
    for (int v = 0; v < views; ++v) MVS_CHECK_ARG(ref[v] && src[v] && transforms[v]);
    Sweep sw = {};
    sw.base = (char*)workspace;
    sw.ws = carve(sw.base, H, W, C, f1, f2, f3);
    if (workspace_bytes < sw.ws.bytes * (size_t)views) return MVS_E_WORKSPACE;
    sw.view_num = view_num; sw.depth_num = depth_num; sw.H = H; sw.W = W; sw.C = C;
    sw.F[0] = f1; sw.F[1] = f2; sw.F[2] = f3;
    sw.hw = (size_t)H * W;
    sw.vw = {views, sw.ws.bytes};
    sw.params = params; sw.depth_values = depth_values;
    sw.ref = ref; sw.src = src; sw.transforms = transforms;
    sw.st = mvs_stream(stream);
    int rc;
    // zero initial states and WTA accumulators (model.py:649-654, 737-739)
    for (int k = 0; k < 3; ++k) if ((rc = zero(sw, sw.ws.h[k][0], sw.hw * sw.F[k]))) return rc;
    if ((rc = zero(sw, sw.ws.max_prob, sw.hw)) || (rc = zero(sw, sw.ws.exp_sum, sw.hw)) || (rc = zero(sw, sw.ws.depth, sw.hw))) return rc;
    route_sweep(sw);
    rc = sw.fused ? fused_sweep(sw) : wavefront_sweep(sw);
    rc = join_side_streams(sw, rc);
    if (rc) return rc;
    return mvs_gru_finish_views(sw.ws, H, W, sw.vw, depth_out, prob_out, sw.st);
}

extern "C" int mvs_gru_wta_f32(const float* ref, const float* src, const float* transforms,
                               int view_num, int depth_num, int H, int W, int C, int f1, int f2,
                               int f3, const float* const* params, const float* depth_values,
                               void* workspace, size_t workspace_bytes, float* depth_out,
                               float* prob_out, void* stream) {
    return mvs_gru_wta_batch_f32(&ref, &src, &transforms, 1, view_num, depth_num, H, W, C, f1, f2, f3, params, depth_values,
                                 workspace, workspace_bytes, depth_out, prob_out, stream);
}
