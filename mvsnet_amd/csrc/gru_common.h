// What the files of the recurrent path share: gru.hip (kernels, stage entry points, launchers), gru_mfma.hip (cell 1 on the
// matrix pipe), gru_fused.hip (the two-launches-per-plane sweep), gru_streams.hip (stream sets) and gru_sweep.hip (orchestration).
// Host-side declarations only; structs that are kernel arguments stay next to their kernels.
#pragma once
#include "common.h"

constexpr int MVS_GRU_MAX_VIEWS = 8;     // reference views per sweep launch (mvs_gru_wta_batch_f32)
// Planes per cost-volume batch of the recurrent sweep: the -variance slices of XB consecutive planes
// come from ONE depth-sweep launch (register tap reuse along depth, cost_volume.hip) into a ring of
// XB slices, instead of one single-plane launch per step (26 -> ~6 us per plane at 400 x 300).
constexpr int XB = 16;
// Planes per synchronisation group of the wavefront (see wavefront_sweep, gru_sweep.hip); the state ring holds RG groups of PG planes.
// (round 4, same box: PG = 2 / 4 / 8 measured 23.40 / 22.47 / 22.49 ms at one view and 72.65 / 71.52 / 70.79 ms per 4-view sweep)
constexpr int PG = 4;
// Ring depth in groups.  A cell may run RG groups ahead of the cell that consumes its states.  Round 1 used 2: the kernel
// trace showed every stream stalling ~100-200 us at EVERY group boundary -- cell k can start group j only when cell k+1
// has finished group j-2, i.e. one group time + two cross-stream signal latencies after cell k finished it, and the signal
// latency (tens of microseconds) exceeds the slack.  With 4 groups the wait is already satisfied when it is reached.
constexpr int RG = 4;
constexpr int SB = 4;          // LayerNorm-sum ring in batches of XB planes: cell 3 lags cell 1 by fewer than 2 * RG groups <= SB batches

// ---- the fused sweep's rings and tables (gru_fused.hip) ----------------------------------------------------------------
constexpr int GRU_FUSED_RING = 64;       // LayerNorm-sum rows of the fused sweep: plane p uses row p % 64 (the sweep zeroes them a batch ahead)
// Copies of a plane's LayerNorm sums: every workgroup of a launch adds its partial sums with float64 atomics, and atomics on one
// cache line are performed one after the other by the L2 -- 256 workgroups x 3 cells on the same 144 bytes were 6 us of every
// plane (round 6: a build without these atomics ran the c3 sweep in 20.87 instead of 22.41 ms; tools/r6_gru_nostat_diag.patch).
// A workgroup adds to copy blockIdx.x % 8 (256 bytes apart: other lines); the next launch's prologue adds the copies up.
constexpr int GRU_FUSED_SLOTS = 8;
constexpr int GRU_FUSED_SLOT_STRIDE = 32;                  // doubles between copies: every copy on cache lines of its own (18 used)
constexpr int GRU_FUSED_ROW = GRU_FUSED_SLOT_STRIDE * GRU_FUSED_SLOTS;      // doubles per row: [slot][cell][6]
// Small-cell tables of the two fused launches, [tap][quad][m][4] floats per table (gru_small_table_kernel): a 20-channel input
// takes 9 * 5 * 16 floats, a 6-channel input 9 * 2 * 16.
constexpr int GRU_FUSED_T20 = 9 * 5 * 16, GRU_FUSED_T6 = 9 * 2 * 16;
// gates launch: cell 2 gates (20 -> 8) as two output-channel quads | cell 3 gates (6 -> 4) | prob_conv (18 weights, bias, pad)
constexpr int GRU_FUSED_WSG_C2HI = GRU_FUSED_T20, GRU_FUSED_WSG_C3 = 2 * GRU_FUSED_T20, GRU_FUSED_WSG_PROB = 2 * GRU_FUSED_T20 + GRU_FUSED_T6;
constexpr int GRU_FUSED_WSG_FLOATS = GRU_FUSED_WSG_PROB + 20;
// output launch: cell 2 candidate (20 -> 4) | cell 3 candidate (6 -> 2)
constexpr int GRU_FUSED_WSC_C3 = GRU_FUSED_T20, GRU_FUSED_WSC_FLOATS = GRU_FUSED_T20 + GRU_FUSED_T6;

// ---- workspace of one view ------------------------------------------------------------------------------------------------
// The fused sweep uses h[k][0..1] as its state ping-pong (s(q) in h[k][q & 1]), {g[k], g2[k]} as its gate ping-pong, c[k], fstats,
// wfg / wfo (cell-1 weights of the gates / output launch), wsg / wsc and x, and addresses them by 32-bit offsets from the block's base.
struct GruWs {
    float *x, *g[3], *g2[3], *c[3], *rh, *u, *h[3][8 * 4], *reg, *max_prob, *exp_sum, *depth;   // h: ring of RG*PG states (RG <= 8); g2: the gate buffer of odd planes (cells whose blend is folded into the next plane's gate convolution)
    float *px, *wx, *wgh, *woh;        // hoisted x-part of cell 1: (2, XB, H, W, 3*f1) and its prepared weights
    float *wfg, *wfo;                  // cell 1 unhoisted: prepared weights of the full 48-channel convolutions
    float *wsg, *wsc;                  // fused sweep: small-cell tables of the gates / output launch (gru_fused.hip)
    double* fstats;                    // fused sweep: GRU_FUSED_RING planes x GRU_FUSED_SLOTS copies x 3 cells x 6 LayerNorm sums
    double* stats;     // per plane of a batch: 3 cells x (gates: 2 groups x 2, out: 1 x 2) = 3 x 6 doubles
    size_t bytes;
};
inline size_t align256(size_t b) { return (b + 255) & ~(size_t)255; }
inline GruWs carve(char* base, int H, int W, int C, int f1, int f2, int f3) {
    size_t hw = (size_t)H * W, off = 0;
    auto take = [&](size_t nfloat) { char* p = base ? base + off : nullptr; off += align256(nfloat * 4); return (float*)p; };
    GruWs w;
    const int F[3] = {f1, f2, f3};
    int fmax = f1 > f2 ? (f1 > f3 ? f1 : f3) : (f2 > f3 ? f2 : f3);
    w.x = take(hw * C * XB);
    // every cell has its own gate / candidate buffers and a ring of states: the three cells of
    // consecutive planes run concurrently (see wavefront_sweep, gru_sweep.hip)
    for (int k = 0; k < 3; ++k) {
        w.g[k] = take(hw * 2 * F[k]); w.g2[k] = take(hw * 2 * F[k]); w.c[k] = take(hw * F[k]);
        for (int r = 0; r < RG * PG; ++r) w.h[k][r] = take(hw * F[k]);
    }
    w.rh = take(hw * fmax); w.u = take(hw * fmax);
    w.reg = take(hw); w.max_prob = take(hw); w.exp_sum = take(hw); w.depth = take(hw);
    w.px = take((size_t)2 * XB * hw * 3 * f1);
    w.wx = take((size_t)9 * C * 3 * f1); w.wgh = take((size_t)9 * f1 * 2 * f1); w.woh = take((size_t)9 * f1 * f1);
    w.wfg = take((size_t)9 * (C + f1) * 2 * f1); w.wfo = take((size_t)9 * (C + f1) * f1);
    w.stats = (double*)(base ? base + off : nullptr); off += align256((size_t)(SB + 1) * XB * 18 * 8);   // SB + 1 batches deep
    w.wsg = take(GRU_FUSED_WSG_FLOATS); w.wsc = take(GRU_FUSED_WSC_FLOATS);
    w.fstats = (double*)(base ? base + off : nullptr); off += align256((size_t)GRU_FUSED_RING * GRU_FUSED_ROW * 8);
    w.bytes = off;
    return w;
}
// the fused sweep's LayerNorm-sum row of plane p
inline double* gru_fused_row(const GruWs& ws, int p) { return ws.fstats + (size_t)(p % GRU_FUSED_RING) * GRU_FUSED_ROW; }

// ---- stream sets (gru_streams.hip) ------------------------------------------------------------------------------------------
struct GruStreams { hipStream_t cand[8], s[3]; int pipe_of_caller; float probe_us[8];
                    hipEvent_t fork, join[3], ready[2][RG], read[2][RG], xready[2], xdone[2]; };
inline bool mvs_is_capturing(hipStream_t s) {
    hipStreamCaptureStatus cs = hipStreamCaptureStatusNone;
    return hipStreamIsCapturing(s, &cs) == hipSuccess && cs != hipStreamCaptureStatusNone;
}
// the set mvs_gru_prepare made for `caller` on the current device, or null: the sweep looks its set up and never creates one
GruStreams* mvs_gru_find(hipStream_t caller);
// (mvs_stream_set_side, the set's interface for the rest of the library, is declared in conv_common.h, which its user includes)

// ---- launchers of gru.hip the sweep calls -----------------------------------------------------------------------------------
// `prev`: the previous plane's blend has not been launched -- its inputs; h then RECEIVES the state entering this plane
// (formed from h_before, the state that entered the previous plane) in the gate convolution's staging
struct PrevPlane { const float* h_before; const float* g; const double* sg; const double* so; };
// `wta` (cell 3, with `prev`): prob_conv + winner-take-all update of the previous plane inside the gate convolution
struct WtaFold { const float* pw; const float* pbias; float depth_value[MVS_GRU_MAX_VIEWS]; float *max_prob, *depth_image, *exp_sum; };
struct Views { int n; size_t stride; };              // views per launch, byte stride between their tensors
// cells 2 / 3 on the small-cell kernels: gate conv then candidate conv (reset gate folded in); MVS_E_SHAPE if the shape has no instance
bool mvs_gru_small_covers(int cin, int f);
int mvs_gru_small_cell(int cin, int f, const float* xin, float* h, const float* const* p, int H, int W, float* g, float* c,
                       double* sg, double* so, const PrevPlane* prev, Views vw, hipStream_t st, const WtaFold* wta);
// h_out = u*h + (1-u)*tanh(LN(c)), u = sigmoid(LN(g_u)), every view in one launch (gru_blend_fused_kernel)
int mvs_gru_blend_views(const float* c, const double* stats_c, const float* og, const float* ob, const float* g, const double* stats_u,
                        const float* ug, const float* ub, int H, int W, int F, const float* h, float* h_out, Views vw, hipStream_t st);
// prob_conv + exp + winner-take-all update (model.py:701-731) of the plane whose final state is `hs` and whose depths are w.depth_value
int mvs_gru_prob_wta_views(const float* hs, int f3, const WtaFold& w, float* reg, int H, int W, Views vw, hipStream_t st);
int mvs_gru_conv2d(const float* xa, int Ca, const float* xb, int Cb, const float* w, const float* bias, int H, int W, int Cout,
                  float* y, double* stats, int groups, hipStream_t st);
// the same tensor of every view := 0 (sizes are multiples of 4 floats: 256-byte carving)
int mvs_gru_zero_views(float* p, size_t nfloat, Views vw, hipStream_t st);
// max_prob / (exp_sum + 1e-7) and the depth image of every view -> (views, H, W) outputs
int mvs_gru_finish_views(const GruWs& ws, int H, int W, Views vw, float* depth_out, float* prob_out, hipStream_t st);

// ---- cell-1 MFMA convolutions (gru_mfma.hip); MVS_E_SHAPE outside their tiling -------------------------------------------
int mvs_gru1_split_weights(const float* w_gates, const float* w_out, int CA, int F, float* wx, float* wgh, float* woh,
                           hipStream_t st);
int mvs_gru1_xpart_mfma(const float* x, const float* wxg, const float* wxo, const float* bias_g, const float* bias_o,
                        int H, int W, int planes, float* px, hipStream_t st);
int mvs_gru1_gates_h_mfma(const float* h, const float* wgh, const float* px, int H, int W, float* g, double* stats,
                          int views, size_t vstride, hipStream_t st);
int mvs_gru1_gates_h_blend_mfma(const float* h_before, const float* c_prev, const float* g_prev, const double* stats_c,
                                const double* stats_u, const float* o_gamma, const float* o_beta, const float* u_gamma,
                                const float* u_beta, float* h_out, const float* wgh, const float* px, int H, int W,
                                float* g, double* stats, int views, size_t vstride, hipStream_t st);
int mvs_gru1_out_h_mfma(const float* h, const float* g, const double* g_stats, const float* r_gamma, const float* r_beta,
                        const float* woh, const float* px, int H, int W, float* c, double* stats, int views, size_t vstride,
                        hipStream_t st);
int mvs_gru1_full_weights(const float* w_gates, const float* w_out, int CA, int F, float* wg, float* wo, hipStream_t st);
int mvs_gru1_gates_full_mfma(const float* x, const float* h, const float* wg, const float* bias, int H, int W, float* g,
                             double* stats, int views, size_t vstride, hipStream_t st);
int mvs_gru1_gates_full_blend_mfma(const float* x, const float* h_before, const float* c_prev, const float* g_prev,
                                   const double* stats_c, const double* stats_u, const float* o_gamma, const float* o_beta,
                                   const float* u_gamma, const float* u_beta, float* h_out, const float* wg,
                                   const float* bias, int H, int W, float* g, double* stats, int views, size_t vstride,
                                   hipStream_t st);
int mvs_gru1_out_full_mfma(const float* x, const float* h, const float* g, const double* g_stats, const float* r_gamma,
                           const float* r_beta, const float* wo, const float* bias, int H, int W, float* c, double* stats,
                           int views, size_t vstride, hipStream_t st);
int mvs_cost_volume_threads_f32(const float* ref, const float* src, const float* transforms, int view_num, int depth_total, int d_begin,
                                int d_count, int H, int W, int C, int variant, int negate, int border, float* cost, int threads, void* stream);
// ---- the fused two-launches-per-plane sweep (gru_fused.hip); `base` = view 0's workspace block, which `ws` was carved from ----
int mvs_gru_fused_prepare_weights(const float* const* params, const GruWs& ws, hipStream_t st);
int mvs_gru_fused_step(const GruWs& ws, char* base, const float* const* params, int t, int depth_num, const float* x_t, int H, int W,
                       int views, size_t vstride, const float* depth_values, hipStream_t st);
