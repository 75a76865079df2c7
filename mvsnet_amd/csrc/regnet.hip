// Host-side composition: the single-layer entry points (scalar vs MFMA), the RegNetUS0 3D U-Net as a layer table plus its
// launch sequence (mvsnet/cnn_wrapper/mvsnetworks.py:122-158), its workspace and weight preparation, and features -> depth in
// one call.  One small fold kernel here; every launch goes to the caller's stream and nothing allocates or syncs.
#include "conv_common.h"
#include "profile.h"
#include <initializer_list>

extern "C" int mvs_conv3d_f32(const float* x, const float* xs, const float* xb, const float* x2,
                              const float* x2s, const float* x2b, const float* w, int D, int H,
                              int W, int Cin, int Cout, int stride, float* y, double* stats,
                              void* stream) {
    MVS_CHECK_ARG(x && w && y && D > 0 && H > 0 && W > 0 && Cin > 0 && Cout > 0);
    MVS_CHECK_ARG((xs == nullptr) == (xb == nullptr) && (x2s == nullptr) == (x2b == nullptr));
    MVS_CHECK_ARG(stride == 1 || stride == 2);
    hipStream_t st = mvs_stream(stream);
    const int impl = mvs_get_conv_impl();
    if (impl != MVS_CONV_IMPL_SCALAR) {
        ConvArgs a = conv_args(x, w, y, stats, D, H, W, Cout);
        a.xs = xs; a.xb = xb; a.x2 = x2; a.x2s = x2s; a.x2b = x2b;
        int rc = mvs_conv3d_dispatch(a, Cin, Cout, stride, st);
        if (rc != MVS_E_SHAPE || impl == MVS_CONV_IMPL_MFMA) return rc;
    }
    return mvs_conv3d_scalar(x, xs, xb, x2, x2s, x2b, w, D, H, W, Cin, Cout, stride, y, stats, st);
}

extern "C" int mvs_deconv3d_f32(const float* x, const float* xs, const float* xb, const float* x2,
                                const float* x2s, const float* x2b, const float* w, int D, int H,
                                int W, int Cin, int Cout, float* y, double* stats, void* stream) {
    MVS_CHECK_ARG(x && w && y && D > 0 && H > 0 && W > 0 && Cin > 0 && Cout > 0);
    MVS_CHECK_ARG((xs == nullptr) == (xb == nullptr) && (x2s == nullptr) == (x2b == nullptr));
    hipStream_t st = mvs_stream(stream);
    const int impl = mvs_get_conv_impl();
    if (impl != MVS_CONV_IMPL_SCALAR) {
        ConvArgs a = conv_args(x, w, y, stats, D, H, W, Cout);
        a.xs = xs; a.xb = xb; a.x2 = x2; a.x2s = x2s; a.x2b = x2b;
        int rc = mvs_deconv3d_mfma_launch(a, Cin, Cout, st);
        if (rc != MVS_E_SHAPE || impl == MVS_CONV_IMPL_MFMA) return rc;
    }
    return mvs_deconv3d_scalar(x, xs, xb, x2, x2s, x2b, w, D, H, W, Cin, Cout, y, stats, st);
}

extern "C" int mvs_conv3d_pair_f32(const float* x, const float* w1, const float* w2, int D, int H, int W,
                                   int Cin, int Cout1, int Cout2, float* y1, double* stats1,
                                   float* y2, double* stats2, void* stream) {
    MVS_CHECK_ARG(x && w1 && w2 && y1 && y2 && D > 0 && H > 0 && W > 0);
    if (Cin != 32 || Cout1 != 8 || Cout2 != 16 || mvs_get_conv_impl() == MVS_CONV_IMPL_SCALAR) return MVS_E_SHAPE;
    return mvs_conv3d_c8_s2_launch(conv_args(x, w1, y1, stats1, D, H, W, Cout1), w2, y2, stats2, mvs_stream(stream));
}

// ---- RegNetUS0 -----------------------------------------------------------------------------------

// Share (1/1000) of 3dconv2_1's blocks that ride as filler workgroups in the launches of 3dconv3_0 and 3dconv3_1 (the rest in
// 3dconv4_0's).  Measured at the metric workload (profiles/r04_filler_ab.txt, depth maps/s): layers apart 912-915; 250/500
// 920-923; 200/400 916; 300/550 913; 0/600 913; 330/340 905.
constexpr int FILL_3_0 = 250, FILL_3_1 = 500;

extern "C" int mvs_regnet_filler_shares(int* permille3) {
    MVS_CHECK_ARG(permille3);
    permille3[0] = FILL_3_0; permille3[1] = FILL_3_1; permille3[2] = 1000 - FILL_3_0 - FILL_3_1;
    return 0;
}

namespace {

// ---- the layer table: everything else about the network's shape is derived from it ----------------
constexpr int N_LAYERS = 11, N_BN = 10;      // all layers but the output conv have BatchNorm
enum { L10, L20, L30, L01, L11, L21, L31, L40, L50, L60, L62 };      // order of the weights array
enum { S1 = 0, S2 = 1, UP = 2 };             // stride 1, stride 2, transposed: conv_coutg's kinds
constexpr int COST = 0, ONE = 0;             // ci: the cost volume's cin;  co: the single output channel
struct LayerRow {
    int kind;
    int level;       // resolution of the input: (D, H, W) >> level
    int ci, co;      // channels in multiples of base (or COST / ONE)
    int p1, p2;      // producers: in = BN+ReLU(p1) [+ BN+ReLU(p2)]; -1 = the raw cost volume / none
};
constexpr LayerRow NET[N_LAYERS] = {
    // encoder (mvsnetworks.py:130-136)
    /* 3dconv1_0 */ {S2, 0, COST, 2, -1, -1},
    /* 3dconv2_0 */ {S2, 1, 2, 4, L10, -1},
    /* 3dconv3_0 */ {S2, 2, 4, 8, L20, -1},
    // same-resolution branches, only needed by the decoder (mvsnetworks.py:138-141)
    /* 3dconv0_1 */ {S1, 0, COST, 1, -1, -1},
    /* 3dconv1_1 */ {S1, 1, 2, 2, L10, -1},
    /* 3dconv2_1 */ {S1, 2, 4, 4, L20, -1},
    /* 3dconv3_1 */ {S1, 3, 8, 8, L30, -1},
    // decoder with additive skips (mvsnetworks.py:146-157)
    /* 3dconv4_0 */ {UP, 3, 8, 4, L31, -1},
    /* 3dconv5_0 */ {UP, 2, 4, 2, L40, L21},
    /* 3dconv6_0 */ {UP, 1, 2, 1, L50, L11},
    // output conv, no BN / ReLU / bias (mvsnetworks.py:158)
    /* 3dconv6_2 */ {S1, 0, 1, ONE, L60, L01},
};
constexpr int out_level(int i) { return NET[i].level + (NET[i].kind == S2) - (NET[i].kind == UP); }
constexpr int widest() { int m = 0; for (const LayerRow& r : NET) m = r.co > m ? r.co : m; return m; }
constexpr int CMAX = widest();               // widest layer, in multiples of base

// doubles of the BatchNorm sums: N_BN x MVS_BN_SLOTS_MAX x 2 x cmax (partial rows per layer, conv_common.h: conv_stats_row)
size_t stats_doubles(int b) { return (size_t)N_BN * MVS_BN_SLOTS_MAX * 2 * CMAX * b; }

// the table at one (cin, base): channel counts, and where each layer's pre-laid-out weights live
struct Net {
    int ci[N_LAYERS], co[N_LAYERS];
    size_t woff[N_LAYERS], wtotal;           // floats; the bf16 hi|lo layouts follow the fp32 ones at wtotal + woff
    bool ok[N_LAYERS], bf[N_LAYERS];         // has an MFMA weight layout / a bf16x3 one
};
Net net_of(int cin, int b) {
    Net n;
    size_t off = 0;
    for (int i = 0; i < N_LAYERS; ++i) {
        const int kind = NET[i].kind, ci = NET[i].ci == COST ? cin : NET[i].ci * b, co = NET[i].co == ONE ? 1 : NET[i].co * b;
        n.ci[i] = ci; n.co[i] = co; n.woff[i] = off;
        n.ok[i] = (i != L62) && (ci % 4 == 0) && conv_coutg(kind, ci, co) != 0;
        n.bf[i] = n.ok[i] && kind == S1 && mvs_conv3d_bf16x3_supported(ci, co);
        off += (size_t)27 * ci * co;
    }
    n.wtotal = off;
    return n;
}

struct RegnetWs {
    float* y[N_BN];        // raw (pre-BN) outputs
    float* scale[N_BN];
    float* shift[N_BN];
    double* stats;         // stats_doubles(b)
    size_t bytes;
};

size_t align256(size_t b) { return (b + 255) & ~(size_t)255; }

// 3dconv0_1's transformed weights for the fused pair's Winograd kernel (conv3d_c8_wino.hip) live behind the other layouts, where the
// layer has the shape that kernel is built for
size_t wino_floats(const Net& n) { return (n.ci[L01] == 32 && n.co[L01] == 8) ? (size_t)MVS_CONV_WINO_FLOATS : 0; }

RegnetWs carve(char* base, int D, int H, int W, int b) {
    const size_t v0 = (size_t)D * H * W;
    size_t off = 0;
    RegnetWs w;
    for (int i = 0; i < N_BN; ++i) {
        w.y[i] = (float*)(base ? base + off : nullptr);
        off += align256((v0 >> (3 * out_level(i))) * NET[i].co * b * sizeof(float));
    }
    for (int i = 0; i < N_BN; ++i) {
        w.scale[i] = (float*)(base ? base + off : nullptr); off += align256(CMAX * b * sizeof(float));
        w.shift[i] = (float*)(base ? base + off : nullptr); off += align256(CMAX * b * sizeof(float));
    }
    w.stats = (double*)(base ? base + off : nullptr);
    off += align256(stats_doubles(b) * sizeof(double));
    w.bytes = off;
    return w;
}

}  // namespace

extern "C" size_t mvs_regnet_workspace_bytes(int D, int H, int W, int cin, int base) {
    if (D <= 0 || H <= 0 || W <= 0 || cin <= 0 || base <= 0) return 0;
    return carve(nullptr, D, H, W, base).bytes;
}

extern "C" size_t mvs_regnet_prepared_floats(int cin, int base) {
    if (cin <= 0 || base <= 0) return 0;
    const Net n = net_of(cin, base);
    return 2 * n.wtotal + wino_floats(n);      // fp32 layouts, then bf16 hi|lo layouts, then 3dconv0_1's Winograd layout
}

extern "C" int mvs_regnet_prepare_f32(const float* const* weights, int cin, int base, float* prepared,
                                      void* stream) {
    MVS_CHECK_ARG(weights && prepared && cin > 0 && base > 0);
    const Net n = net_of(cin, base);
    for (int i = 0; i < N_LAYERS; ++i) {
        if (!n.ok[i]) continue;
        int rc = mvs_conv_weight_layout(weights[i], NET[i].kind, n.ci[i], n.co[i], prepared + n.woff[i], mvs_stream(stream));
        if (rc) return rc;
        if (n.bf[i]) {
            rc = mvs_conv_weight_split(weights[i], n.ci[i], n.co[i],
                                       reinterpret_cast<unsigned short*>(prepared + n.wtotal + n.woff[i]), mvs_stream(stream));
            if (rc) return rc;
        }
    }
    if (wino_floats(n)) return mvs_conv_wino_weight_layout(weights[L01], prepared + 2 * n.wtotal, mvs_stream(stream));
    return 0;
}

namespace {

// (nslot, n) partial rows of BatchNorm sums -> row 0 holds the total, the other rows zero
__global__ void bn_fold_rows_kernel(double* stats, int nslot, int n) {
    for (int j = threadIdx.x; j < n; j += blockDim.x) {
        double t = stats[j];
        for (int r = 1; r < nslot; ++r) { t += stats[(size_t)r * n + j]; stats[(size_t)r * n + j] = 0.0; }
        stats[j] = t;
    }
}

// partial rows per layer: only where EVERY layer has an MFMA kernel (the scalar fallback finalises one row)
// More rows shorten the producers' tails of same-address float64 atomics; a consumer workgroup folds the rows once (conv_common.h,
// bn_sum1: one thread per channel, every row requested before the first is added).  Depth maps/s at the metric workload:
//   BN_SLOTS                          1       2       4       8
//   every consumer thread folds     858     864     860     848     (round 2: each row cost the consumers ~3 us per depth map)
//   one fold per workgroup          945.6   958.8   961.8   969.1   (one run each, PAIR_SLOTS = 2; the parent build 954.0 .. 954.9)
//   same, medians of three            --      --    984.0   986.3   (another machine: the parent build 967.7 .. 969.7)
// (MVS_HOOK_BN_SLOTS; profiles/r07_tail_ab.txt).  8 is the workspace's row count, MVS_BN_SLOTS_MAX.
constexpr int BN_SLOTS = 8;
// the fused pass over the cost volume spreads its sums over partial rows too (conv3d_c8.hip, FuseArgs)
//   PAIR_SLOTS                        1       2       4       8
//   every consumer thread folds     870     869     869     864     (round 1 .. 2)
//   one fold per workgroup          960.2   958.8   957.3   958.2   (one run each, BN_SLOTS = 2)
//   same at BN_SLOTS = 8, medians     --    986.3   987.1   985.1   (of three; the runs of one setting spread over 1 .. 9)
// no difference outside the spread: the count stays (240 workgroups finish together and add 48 sums each).
constexpr int PAIR_SLOTS = 2;
static_assert(BN_SLOTS <= MVS_BN_SLOTS_MAX && PAIR_SLOTS <= MVS_BN_SLOTS_MAX, "rows beyond the workspace's slab");
static_assert(MVS_BN_SLOTS_MAX == 8, "mvs_set_test_hook admits 1..8 rows");
// test / measurement hooks: another row count for one call (tests compare the defaults with one row)
int bn_slots() { const int hk = mvs_hook(MVS_HOOK_BN_SLOTS); return hk ? hk : BN_SLOTS; }
int pair_slots() { const int hk = mvs_hook(MVS_HOOK_PAIR_SLOTS); return hk ? hk : PAIR_SLOTS; }

// One call of the regulariser: what the steps below share.
struct Run {
    const float* cost; int batch, D, H, W, b;
    const float* const* weights; const float* prepared; const float* const* gammas; const float* const* betas;
    float eps; float* reg; hipStream_t hs;
    int impl;
    Net net;
    RegnetWs ws;
    size_t ws_floats1;           // a sample's workspace region (regions are 256-byte aligned)
    bool all_mfma;
    int SL;                      // partial rows of every layer's sums
    int PS;                      // partial rows of the fused pair's sums
    int lp;                      // per-layer event slot of this call (mvs_profile_layers), or -1
    bool pair_done = false;
    bool finalised[N_BN] = {};

    double* st(int i) const { return ws.stats + (size_t)i * MVS_BN_SLOTS_MAX * 2 * CMAX * b; }
    int nslot_of(int i) const { return (pair_done && (i == L01 || i == L10)) ? PS : SL; }
    BnSrc bn_of(int i) const {   // producer i's raw BatchNorm sums (i < 0: raw input, no BN)
        if (i < 0) return BnSrc{nullptr, nullptr, nullptr, 1.0, eps, 0, 1};
        return BnSrc{st(i), gammas[i], betas[i], count(i), eps, net.co[i], nslot_of(i)};
    }
    double count(int i) const { return ((double)batch * D * H * W) / (double)(1 << (3 * out_level(i))); }   // voxels behind a statistic
    const float* wprep(int i) const { return (prepared && net.ok[i]) ? prepared + net.woff[i] : nullptr; }
    const float* wprep_wino() const { return (prepared && wino_floats(net)) ? prepared + 2 * net.wtotal : nullptr; }
    int mark(int l, int k, hipStream_t s) const { return mvs_prof_layers.mark(lp, 2 * l + k, s); }
};

// layer `out` of sample bi as its MFMA launcher takes it: in = BN+ReLU(p1) [+ BN+ReLU(p2)] from the producers' raw sums
ConvArgs layer_args(const Run& r, int bi, int out) {
    const LayerRow& row = NET[out];
    const size_t wo = (size_t)bi * r.ws_floats1;
    const size_t v0 = (size_t)r.D * r.H * r.W;
    ConvArgs a = conv_args(row.p1 >= 0 ? r.ws.y[row.p1] + wo : r.cost + (size_t)bi * v0 * r.net.ci[out], r.weights[out],
                           out == L62 ? r.reg + (size_t)bi * v0 : r.ws.y[out] + wo, out == L62 ? nullptr : r.st(out),
                           r.D >> row.level, r.H >> row.level, r.W >> row.level, r.net.co[out]);
    a.x2 = row.p2 >= 0 ? r.ws.y[row.p2] + wo : nullptr;
    a.bn = r.bn_of(row.p1); a.bn2 = r.bn_of(row.p2);
    a.wprep = r.wprep(out);
    // opt-in split-precision path: bf16 hi|lo weights live behind the fp32 layouts
    // (the opt-in split-precision mode keeps every fused / filled fp32 launch of the default mode and uses its bf16 kernel for the one
    //  layer where it is faster, 3dconv0_1: 32 -> 8 over the whole volume -- round 5; before, it ran all eleven layers apart)
    if (r.prepared && r.impl == MVS_CONV_IMPL_BF16X3 && r.net.bf[out] && (!r.all_mfma || out == L01))
        a.wprep_bf = reinterpret_cast<const unsigned short*>(r.prepared + r.net.wtotal + r.net.woff[out]);
    a.stats_slots = r.SL;
    return a;
}

int ensure_final(Run& r, int i) {        // (scale, shift) of producer i for the scalar kernels, once per producer and call
    if (i < 0 || r.finalised[i]) return 0;
    r.finalised[i] = true;
    // the producer may have spread its sums over partial rows: fold them into row 0 (the other rows become zero, so an MFMA
    // consumer that adds the rows up again still gets the total)
    if (r.nslot_of(i) > 1) {
        bn_fold_rows_kernel<<<1, 256, 0, r.hs>>>(r.st(i), r.nslot_of(i), 2 * r.net.co[i]);
        hipError_t e = hipGetLastError();
        if (e != hipSuccess) return (int)e;
    }
    return mvs_bn_finalize_f32(r.st(i), r.net.co[i], r.count(i), r.gammas[i], r.betas[i], r.eps, r.ws.scale[i], r.ws.shift[i], r.hs);
}

int layer_one(Run& r, int bi, int out, hipStream_t s) {
    const LayerRow& row = NET[out];
    ConvArgs a = layer_args(r, bi, out);
    const int ci = r.net.ci[out], co = r.net.co[out];
    if (r.impl != MVS_CONV_IMPL_SCALAR) {
        int rc = row.kind == UP ? mvs_deconv3d_mfma_launch(a, ci, co, s) : mvs_conv3d_dispatch(a, ci, co, row.kind == S2 ? 2 : 1, s);
        // a (D, H, W) outside a layer's MFMA tiling falls back to the shape-generic kernel for THAT layer (AUTO only)
        if (rc != MVS_E_SHAPE || r.impl != MVS_CONV_IMPL_AUTO) return rc;
    }
    int rc;
    if ((rc = ensure_final(r, row.p1)) || (rc = ensure_final(r, row.p2))) return rc;
    const float* s1 = row.p1 >= 0 ? r.ws.scale[row.p1] : nullptr; const float* t1 = row.p1 >= 0 ? r.ws.shift[row.p1] : nullptr;
    const float* s2 = row.p2 >= 0 ? r.ws.scale[row.p2] : nullptr; const float* t2 = row.p2 >= 0 ? r.ws.shift[row.p2] : nullptr;
    return row.kind == UP ? mvs_deconv3d_scalar(a.x, s1, t1, a.x2, s2, t2, a.w, a.D, a.H, a.W, ci, co, a.y, a.stats, s)
                          : mvs_conv3d_scalar(a.x, s1, t1, a.x2, s2, t2, a.w, a.D, a.H, a.W, ci, co, row.kind == S2 ? 2 : 1, a.y, a.stats, s);
}

// a plain layer on stream s: for all samples of the batch before any consumer is launched
int layer(Run& r, int out, hipStream_t s) {
    int rc = r.mark(out, 0, s);
    for (int bi = 0; bi < r.batch && !rc; ++bi) rc = layer_one(r, bi, out, s);
    return rc ? rc : r.mark(out, 1, s);
}

// ---- fused forms.  Each answers APART when it does not apply -- its precondition fails, or its first launch answers
// MVS_E_SHAPE -- and or_apart() then runs its layers one by one; any other code is the call's. ----------------------------
constexpr int APART = -1000;      // no MVS_E_* code and no hipError_t

int or_apart(Run& r, int rc, std::initializer_list<int> layers) {
    if (rc != APART) return rc;
    for (int l : layers) if ((rc = layer(r, l, r.hs))) return rc;
    return 0;
}

// 3dconv1_0 and 3dconv0_1 read the same volume, the raw cost volume: one fused pass when the shape is the one conv3d_c8.hip is
// built for.  (Its launcher answers MVS_E_SHAPE for volumes of 2 GB and more, so a pair that ran implies all_mfma.)
// Reports under 3dconv0_1; the dominant-kernel profiler (mvs_profile_dominant) brackets it and counts it once its end is recorded.
int fused_pair(Run& r) {
    if (!((r.impl == MVS_CONV_IMPL_AUTO || r.impl == MVS_CONV_IMPL_MFMA) && r.net.ci[L01] == 32 && r.b == 8)) return APART;
    const int slot = mvs_prof_dominant.claim();
    int rc;
    if ((rc = mvs_prof_dominant.mark(slot, 0, r.hs)) || (rc = r.mark(L01, 0, r.hs))) return rc;
    for (int bi = 0; bi < r.batch; ++bi) {
        const size_t wo = (size_t)bi * r.ws_floats1;
        ConvArgs a = conv_args(r.cost + (size_t)bi * r.D * r.H * r.W * r.net.ci[L01], r.weights[L01], r.ws.y[L01] + wo, r.st(L01),
                               r.D, r.H, r.W, r.net.co[L01]);
        a.wprep = r.wprep(L01);
        rc = mvs_conv3d_c8_s2_launch(a, r.weights[L10], r.ws.y[L10] + wo, r.st(L10), r.hs, r.PS, r.PS, r.wprep_wino());
        if (rc) return rc == MVS_E_SHAPE ? APART : rc;
    }
    if ((rc = r.mark(L01, 1, r.hs)) || (rc = mvs_prof_dominant.mark(slot, 1, r.hs))) return rc;
    mvs_prof_dominant.commit(slot);
    r.pair_done = true;
    return 0;
}

// 3dconv1_1 (stride 1) and 3dconv2_0 (stride 2) read the same tensor, BN + ReLU of 3dconv1_0: one fused pass when the
// shape is the one conv3d_mfma.hip builds it for (round 4), as for the two consumers of the cost volume above.
// Reports under 3dconv1_1.
int fuse2(Run& r) {
    const int D1 = r.D >> 1, H1 = r.H >> 1, W1 = r.W >> 1;
    if (!r.all_mfma || (D1 & 1) || (H1 & 1) || (W1 & 1)) return APART;
    int rc = r.mark(L11, 0, r.hs);
    for (int bi = 0; bi < r.batch && !rc; ++bi) {
        const size_t wo = (size_t)bi * r.ws_floats1;
        ConvArgs a = conv_args(r.ws.y[L10] + wo, r.weights[L11], r.ws.y[L11] + wo, r.st(L11), D1, H1, W1, r.net.co[L11]);
        a.bn = r.bn_of(L10); a.wprep = r.wprep(L11); a.stats_slots = r.SL;
        rc = mvs_conv3d_s1_fuse2_launch(a, r.weights[L20], r.ws.y[L20] + wo, r.st(L20), r.hs);
    }
    if (rc) return rc == MVS_E_SHAPE ? APART : rc;
    return r.mark(L11, 1, r.hs);
}

// Round 6 experiment (MVS_HOOK_REGNET_SIDE_BRANCH): 3dconv1_1 is only read by 3dconv6_0, three launches of the latency-bound
// low-resolution chain later -- on a side stream of the caller's stream set (mvs_gru_prepare) it runs BESIDE 3dconv2_0 and the
// chain instead of in front of them; 3dconv2_0 then runs apart from it.  MEASURED: 986.5-987.8 against 982.4-983.7 depth maps/s
// (+0.4 %, profiles/r06_regnet_side_branch.txt) -- the chain's launches stretch by nearly what the branch hides, as in round 1.
// (Round 1 ran the same-resolution branches on a side stream beside the encoder's tail; with the block kernels of conv3d_os.hip a
// layer running beside the chain slows it by more than it hides -- 826 depth maps/s with the fork, 837 without -- so the product
// is one stream.)  Stays a measurement hook.  The caller's stream joins the side stream on every exit after the fork.
struct SideBranch {
    hipStream_t hs = nullptr, side = nullptr;
    hipEvent_t ev_fork = nullptr, ev_join = nullptr;
    enum { NONE, FORKED, BRANCH_RECORDED } state = NONE;
    int fork() {
        hipError_t e = hipEventRecord(ev_fork, hs);
        if (e == hipSuccess) e = hipStreamWaitEvent(side, ev_fork, 0);
        if (e == hipSuccess) state = FORKED;
        return (int)e;
    }
    int branch_end() {
        const hipError_t e = hipEventRecord(ev_join, side);
        if (e == hipSuccess) state = BRANCH_RECORDED;
        return (int)e;
    }
    int join() {      // no-op when no branch is open
        if (state == NONE) return 0;
        hipError_t e = state == FORKED ? hipEventRecord(ev_join, side) : hipSuccess;
        if (e == hipSuccess) e = hipStreamWaitEvent(hs, ev_join, 0);
        state = NONE;
        return (int)e;
    }
    ~SideBranch() { join(); }
};
int side_branch(Run& r, SideBranch& sb) {
    int rc;
    if ((rc = sb.fork()) || (rc = layer(r, L11, sb.side)) || (rc = sb.branch_end())) return rc;
    return layer(r, L20, r.hs);
}

// 3dconv2_1 (only the decoder's 3dconv5_0 reads it) rides as filler blocks in the launches of the 1/8-resolution chain
// 3dconv3_0 -> 3_1 -> 4_0 (conv3d_os.hip, conv3d_os_filled_kernel; round 4) when every layer has its block kernel: needs
// prepared weights.  A filled launch reports under its chain layer.  MVS_E_SHAPE from the second or third launch is an error.
int filled_chain(Run& r) {
    if (!(r.all_mfma && r.prepared && r.net.ok[L21] && r.net.ok[L30] && r.net.ok[L31] && r.net.ok[L40])) return APART;
    const int nfill = mvs_conv3d_os_filler_blocks(r.D >> 2, r.H >> 2, r.W >> 2);
    // share of 3dconv2_1's blocks per chain launch, in 1/1000 (multiples of 8 blocks: one per XCD)
    const int f0 = (nfill * FILL_3_0 / 1000) & ~7, f1 = (nfill * FILL_3_1 / 1000) & ~7;
    const int chain[3] = {L30, L31, L40}, first[3] = {0, f0, f0 + f1}, count[3] = {f0, f1, nfill - f0 - f1};
    for (int k = 0; k < 3; ++k) {
        const int out = chain[k];
        int rc = r.mark(out, 0, r.hs);
        for (int bi = 0; bi < r.batch && !rc; ++bi)
            rc = mvs_conv3d_os_filled_launch(layer_args(r, bi, out), NET[out].kind, r.net.ci[out], r.net.co[out],
                                             layer_args(r, bi, L21), first[k], count[k], r.hs);
        if (!rc) rc = r.mark(out, 1, r.hs);
        if (rc) return (rc == MVS_E_SHAPE && k == 0) ? APART : rc;
    }
    return 0;
}

// `batch` samples share every BatchNorm layer's statistics (the reference normalises over (B,D,H,W), network.py:496-506):
// each layer runs for all samples -- their float64 sums land in the same slab -- before any consumer reads them.
// cost (B,D,H,W,cin), reg (B,D,H,W), workspace = B consecutive per-sample regions (the sums live in the first).
// stats_zeroed: the caller has cleared the sums already (mvs_depth_from_features_f32: in its homography launch).
int regnet_run(const float* cost, int batch, int D, int H, int W, int cin, int base,
               const float* const* weights, const float* prepared, const float* const* gammas,
               const float* const* betas, float eps, void* workspace, size_t workspace_bytes,
               float* reg, void* stream, bool stats_zeroed = false) {
    MVS_CHECK_ARG(cost && weights && gammas && betas && workspace && reg);
    MVS_CHECK_ARG(batch > 0 && D > 0 && H > 0 && W > 0 && cin > 0 && base > 0);
    if ((D % 8) || (H % 8) || (W % 8)) return MVS_E_SHAPE;
    const RegnetWs ws = carve((char*)workspace, D, H, W, base);
    if (workspace_bytes < ws.bytes * (size_t)batch) return MVS_E_WORKSPACE;
    int rc;
    if (!stats_zeroed && (rc = mvs_zero_f64(ws.stats, stats_doubles(base), stream))) return rc;
    const int impl = mvs_get_conv_impl();
    // 2 rows per layer only where every layer has its MFMA kernel
    // (volumes of 2 GB and more leave the 32-bit-offset MFMA kernels for the generic ones: one row there)
    const bool all_mfma = impl != MVS_CONV_IMPL_SCALAR && cin == 32 && base == 8 && (long long)D * H * W * cin * 4 < (1LL << 31);
    Run r{cost, batch, D, H, W, base, weights, prepared, gammas, betas, eps, reg, mvs_stream(stream), impl,
          net_of(cin, base), ws, ws.bytes / sizeof(float), all_mfma, all_mfma ? bn_slots() : 1, pair_slots(), mvs_prof_layers.claim()};
    mvs_prof_layers.commit(r.lp);

    SideBranch sb;
    bool side = false;
    if (mvs_hook(MVS_HOOK_REGNET_SIDE_BRANCH) && all_mfma && batch == 1 && r.lp < 0) {
        hipStreamCaptureStatus cs = hipStreamCaptureStatusNone;
        const bool capturing = hipStreamIsCapturing(r.hs, &cs) == hipSuccess && cs != hipStreamCaptureStatusNone;
        sb.hs = r.hs;
        side = !capturing && mvs_stream_set_side(r.hs, &sb.side, &sb.ev_fork, &sb.ev_join);
    }
    if ((rc = or_apart(r, fused_pair(r), {L10, L01}))) return rc;
    if ((rc = or_apart(r, side ? side_branch(r, sb) : fuse2(r), {L11, L20}))) return rc;
    if ((rc = or_apart(r, filled_chain(r), {L21, L30, L31, L40}))) return rc;
    if ((rc = layer(r, L50, r.hs))) return rc;
    if ((rc = sb.join())) return rc;                       // 3dconv6_0 reads 3dconv1_1
    if ((rc = layer(r, L60, r.hs))) return rc;
    return layer(r, L62, r.hs);
}

}  // namespace

extern "C" int mvs_regnet_us0_f32(const float* cost, int D, int H, int W, int cin, int base,
                                  const float* const* weights, const float* const* gammas,
                                  const float* const* betas, float eps, void* workspace,
                                  size_t workspace_bytes, float* reg, void* stream) {
    return regnet_run(cost, 1, D, H, W, cin, base, weights, nullptr, gammas, betas, eps, workspace,
                      workspace_bytes, reg, stream);
}

extern "C" int mvs_regnet_us0_prepared_f32(const float* cost, int D, int H, int W, int cin, int base,
                                           const float* const* weights, const float* prepared,
                                           const float* const* gammas, const float* const* betas,
                                           float eps, void* workspace, size_t workspace_bytes,
                                           float* reg, void* stream) {
    MVS_CHECK_ARG(prepared);
    return regnet_run(cost, 1, D, H, W, cin, base, weights, prepared, gammas, betas, eps, workspace,
                      workspace_bytes, reg, stream);
}

extern "C" int mvs_regnet_us0_batch_f32(const float* cost, int batch, int D, int H, int W, int cin, int base,
                                        const float* const* weights, const float* prepared,
                                        const float* const* gammas, const float* const* betas,
                                        float eps, void* workspace, size_t workspace_bytes,
                                        float* reg, void* stream) {
    return regnet_run(cost, batch, D, H, W, cin, base, weights, prepared, gammas, betas, eps, workspace,
                      workspace_bytes, reg, stream);
}

// ---- features -> depth in one call (model.py:374-502 after the towers) ---------------------------------------------
extern "C" int mvs_depth_from_features_f32(const float* features, const float* cams, int view_num, int depth_num,
                                           int H, int W, int C, int base, float depth_start, float depth_interval,
                                           float depth_end, int inverse_depth, int variant,
                                           const float* const* weights, const float* prepared,
                                           const float* const* gammas, const float* const* betas, float eps,
                                           float* transforms, float* cost, void* workspace, size_t workspace_bytes,
                                           float* reg, float* depth, float* prob, void* stream) {
    MVS_CHECK_ARG(features && cams && weights && gammas && betas && transforms && cost && workspace && reg && depth && prob);
    MVS_CHECK_ARG(view_num >= 2 && depth_num >= 1 && H > 0 && W > 0 && C > 0 && base > 0);
    if ((depth_num % 8) || (H % 8) || (W % 8)) return MVS_E_SHAPE;
    RegnetWs ws = carve((char*)workspace, depth_num, H, W, base);
    if (workspace_bytes < ws.bytes) return MVS_E_WORKSPACE;
    int rc;
    const int sp = mvs_prof_stages.claim();          // stage event slot of this call (mvs_profile_stages)
    mvs_prof_stages.commit(sp);
    auto mark = [&](int k) { return mvs_prof_stages.mark(sp, k, mvs_stream(stream)); };
    if ((rc = mark(0))) return rc;
    // plane homographies -> 8-vectors, and the zero-fill of this depth map's BatchNorm sums, in one launch
    if ((rc = mvs_homography_transforms_zero(cams, view_num, depth_num, depth_start, depth_interval, depth_end, inverse_depth,
                                             transforms, ws.stats, (int)stats_doubles(base), mvs_stream(stream)))) return rc;
    if ((rc = mvs_cost_volume_f32(features, features + (size_t)H * W * C, transforms, view_num, depth_num, 0, depth_num,
                                  H, W, C, variant, 0, 0, cost, stream))) return rc;
    if ((rc = mark(1))) return rc;
    if ((rc = regnet_run(cost, 1, depth_num, H, W, C, base, weights, prepared, gammas, betas, eps, workspace,
                         workspace_bytes, reg, stream, true))) return rc;
    if ((rc = mark(2))) return rc;
    if ((rc = mvs_softargmin_prob_f32(reg, depth_num, H, W, depth_start, depth_interval, inverse_depth, depth, prob, stream))) return rc;
    return mark(3);
}
