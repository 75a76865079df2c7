// ConvGRU regulariser (R-MVSNet) and winner-take-all depth sweep (R8, R9, K10, K11).
// Reference behaviour: ConvGRUCell.__call__ (mvsnet/convgru.py:82-122) with group_norm reducing
// to tf.contrib.layers.layer_norm for every filter count on the path (convgru.py:24-31), and the
// while_loop body / tail of inference_winner_take_all (mvsnet/model.py:676-751).
//
// v1 kernels: shape-generic VALU convolution over the channel concatenation [xa | xb] (no concat
// is materialised), LayerNorm moments accumulated by the producing convolution, gate / blend
// element-wise stages, WTA update.  The sweep keeps all state resident in HBM/L2; only the
// current cost slice (H*W*C) exists, never the (D,H,W,C) volume.
#include "gru_common.h"

namespace {

template <int CO>
__global__ void __launch_bounds__(256)
conv2d_cat_kernel(const float* __restrict__ xa, int Ca, const float* __restrict__ xb, int Cb,
                  const float* __restrict__ w, const float* __restrict__ bias, int H, int W,
                  float* __restrict__ y, double* __restrict__ stats, int groups) {
    __shared__ float red[4][2][2];
    const int pix = blockIdx.x * blockDim.x + threadIdx.x;
    const int HW = H * W;
    const bool valid = pix < HW;
    const int Ct = Ca + Cb;
    float acc[CO];
#pragma unroll
    for (int j = 0; j < CO; ++j) acc[j] = bias ? bias[j] : 0.f;
    if (valid) {
        const int py = pix / W, px = pix - py * W;
        for (int kh = 0; kh < 3; ++kh) {
            int iy = py + kh - 1; if (iy < 0 || iy >= H) continue;
            for (int kw = 0; kw < 3; ++kw) {
                int ix = px + kw - 1; if (ix < 0 || ix >= W) continue;
                const size_t p = (size_t)iy * W + ix;
                const float* wt = w + (size_t)(kh * 3 + kw) * Ct * CO;
                for (int ci = 0; ci < Ca; ++ci) {
                    float xv = xa[p * Ca + ci];
#pragma unroll
                    for (int j = 0; j < CO; ++j) acc[j] += xv * wt[(size_t)ci * CO + j];
                }
                for (int ci = 0; ci < Cb; ++ci) {
                    float xv = xb[p * Cb + ci];
#pragma unroll
                    for (int j = 0; j < CO; ++j) acc[j] += xv * wt[(size_t)(Ca + ci) * CO + j];
                }
            }
        }
#pragma unroll
        for (int j = 0; j < CO; ++j) y[(size_t)pix * CO + j] = acc[j];
    }
    if (stats) {
        const int per = CO / groups;
        const int lane = threadIdx.x & 63, wv = threadIdx.x >> 6;
        for (int g = 0; g < groups; ++g) {
            float s = 0.f, q = 0.f;
            if (valid) {
#pragma unroll
                for (int j = 0; j < CO; ++j)
                    if (j / per == g) { s += acc[j]; q += acc[j] * acc[j]; }
            }
            s = wave_sum(s); q = wave_sum(q);
            if (lane == 0) { red[wv][g][0] = s; red[wv][g][1] = q; }
        }
        __syncthreads();
        if (threadIdx.x < groups * 2) {
            int g = threadIdx.x >> 1, k = threadIdx.x & 1;
            double t = (double)red[0][g][k] + (double)red[1][g][k] + (double)red[2][g][k] + (double)red[3][g][k];
            atomicAdd(&stats[g * 2 + k], t);
        }
    }
}

typedef float f32x4 __attribute__((ext_vector_type(4)));
struct LN { float inv_r, mean_r; };

// LayerNorm affine from accumulated moments: y = x*inv[c] + (beta[c] - mean*inv[c]),
// inv[c] = gamma[c] / sqrt(var + 1e-12)   (tf.contrib.layers.layer_norm)
__device__ __forceinline__ void ln_affine(const double* st, double n, float gamma, float beta,
                                          float& a, float& b) {
    double mean = st[0] / n;
    double var = st[1] / n - mean * mean;
    if (var < 0.0) var = 0.0;
    double inv = (double)gamma / sqrt(var + 1e-12);
    a = (float)inv;
    b = (float)((double)beta - mean * inv);
}

__device__ __forceinline__ float sigmoidf(float x) { return 1.0f / (1.0f + expf(-x)); }

__global__ void __launch_bounds__(256)
gru_gates_kernel(const float* __restrict__ g, const double* __restrict__ stats,
                 const float* __restrict__ rg, const float* __restrict__ rb,
                 const float* __restrict__ ug, const float* __restrict__ ub,
                 const float* __restrict__ h, int HW, int F, float* __restrict__ rh,
                 float* __restrict__ u) {
    long long i = (long long)blockIdx.x * blockDim.x + threadIdx.x;
    if (i >= (long long)HW * F) return;
    int f = (int)(i % F);
    long long pix = i / F;
    double n = (double)HW * F;
    float a, b;
    ln_affine(stats, n, rg[f], rb[f], a, b);
    float r = sigmoidf(g[pix * 2 * F + f] * a + b);               // convgru.py:97,101
    ln_affine(stats + 2, n, ug[f], ub[f], a, b);
    float uu = sigmoidf(g[pix * 2 * F + F + f] * a + b);          // convgru.py:98,102
    rh[i] = r * h[i];                                             // convgru.py:107
    u[i] = uu;
}

__global__ void __launch_bounds__(256)
gru_blend_kernel(const float* __restrict__ c, const double* __restrict__ stats,
                 const float* __restrict__ og, const float* __restrict__ ob,
                 const float* __restrict__ u, int HW, int F, float* __restrict__ h) {
    long long i = (long long)blockIdx.x * blockDim.x + threadIdx.x;
    if (i >= (long long)HW * F) return;
    int f = (int)(i % F);
    float a, b;
    ln_affine(stats, (double)HW * F, og[f], ob[f], a, b);
    float yv = tanhf(c[i] * a + b);                               // convgru.py:114,117
    float uu = u[i];
    h[i] = uu * h[i] + (1.0f - uu) * yv;                          // convgru.py:120
}

__global__ void __launch_bounds__(256)
wta_update_kernel(const float* __restrict__ reg, float depth_value, int HW,
                  float* __restrict__ max_prob, float* __restrict__ depth_image,
                  float* __restrict__ exp_sum) {
    int i = blockIdx.x * blockDim.x + threadIdx.x;
    if (i >= HW) return;
    float p = expf(reg[i]);                                       // model.py:703
    float mp = max_prob[i];
    if (mp < p) { max_prob[i] = p; depth_image[i] = depth_value; }  // :721-728 (strict <)
    exp_sum[i] += p;                                              // :731
}

__global__ void __launch_bounds__(256)
wta_finish_kernel(const float* __restrict__ max_prob, const float* __restrict__ exp_sum, int HW,
                  float* __restrict__ prob) {
    int i = blockIdx.x * blockDim.x + threadIdx.x;
    if (i < HW) prob[i] = max_prob[i] / (exp_sum[i] + 1e-7f);     // model.py:749-751
}

template <int N>
__device__ __forceinline__ void load_vec(const float* __restrict__ p, float (&o)[N]) {
    if constexpr (N % 4 == 0) {
#pragma unroll
        for (int i = 0; i < N / 4; ++i) { float4 t = *(const float4*)(p + 4 * i); o[4*i] = t.x; o[4*i+1] = t.y; o[4*i+2] = t.z; o[4*i+3] = t.w; }
    } else if constexpr (N % 2 == 0) {
#pragma unroll
        for (int i = 0; i < N / 2; ++i) { float2 t = *(const float2*)(p + 2 * i); o[2*i] = t.x; o[2*i+1] = t.y; }
    } else {
#pragma unroll
        for (int i = 0; i < N; ++i) o[i] = p[i];
    }
}

// Small-channel 3x3 convolution over [xa | xb] for ConvGRU cells 2 and 3 (20 -> 8/4, 6 -> 4/2
// channels).  A workgroup owns a 16 x 16 pixel tile: the 18 x 18 neighbourhood of the concatenation is
// staged once in LDS (MODE 1 folds the reset gate into xb there: xb = sigmoid(LayerNorm(g_r)) * h,
// convgru.py:97,101,107 -- evaluated once per staged element, not once per tap), every thread then
// reads its 9 taps from LDS; weights come through the scalar cache.
// MODE 2: what the previous plane's blend needs, evaluated while staging xb (see conv2d_small_kernel)
// View v of a multi-view launch: every tensor of the sweep lives `vstride` bytes after view v-1's (one workspace block per
// view); weights, biases and LayerNorm parameters are shared.
template <class T> __device__ __forceinline__ T* view_ptr(T* p, size_t vo) { return p ? (T*)((char*)p + vo) : p; }
template <class T> __device__ __forceinline__ const T* view_ptr(const T* p, size_t vo) { return p ? (const T*)((const char*)p + vo) : p; }

struct BlendIn {
    const float* c; const float* g;                   // previous plane: raw candidate (H,W,F) and gate (H,W,2F) convolutions
    const double* stats_c; const double* stats_u;     // their LayerNorm moments [sum, sumsq]
    const float *og, *ob, *ug, *ub;                   // candidate / update LayerNorm gamma, beta
    float* h_out;                                     // receives the blended state (the tile's own pixels)
    // cell 3 only (pw != null): prob_conv + exp + winner-take-all update of the PREVIOUS plane, whose final state is the
    // state just formed in the tile (model.py:701-703, 721-731): one launch less per plane
    const float* pw; const float* pbias; float depth_value[MVS_GRU_MAX_VIEWS];      // per view: the planes' depths differ between views
    float *max_prob, *depth_image, *exp_sum;
};

// MODE 2 folds the PREVIOUS plane's blend into the staging of xb: xb holds the state that entered the previous plane
// and the state entering this one, u*h + (1-u)*tanh(LN c) (convgru.py:98,102,114-120), is formed on load (halo
// positions are recomputed by the neighbouring tiles), written out for the tile's own pixels -- the candidate
// convolution, the next cell and the WTA update read it -- and convolved: one launch less per plane and cell.
struct SmallArgs {
    const float* xa; const float* xb; const float* g; const double* g_stats; const float* r_gamma; const float* r_beta;
    const float* w; const float* bias; int H, W; float* y; double* stats; int groups; BlendIn bl;
    size_t vstride;                                   // blockIdx.y = view
};

template <int CA, int CB, int CO, int MODE, bool MATRIX>
__device__ __forceinline__ void conv2d_small_body(const SmallArgs& sa, const int bid) {
    const int view = blockIdx.y;
    const size_t vo = (size_t)view * sa.vstride;
    const float* __restrict__ xa = view_ptr(sa.xa, vo); const float* __restrict__ xb = view_ptr(sa.xb, vo);
    const float* __restrict__ g = view_ptr(sa.g, vo); const double* __restrict__ g_stats = view_ptr(sa.g_stats, vo);
    const float* __restrict__ r_gamma = sa.r_gamma; const float* __restrict__ r_beta = sa.r_beta;
    const float* __restrict__ w = sa.w; const float* __restrict__ bias = sa.bias;
    const int H = sa.H, W = sa.W, groups = sa.groups;
    float* __restrict__ y = view_ptr(sa.y, vo); double* __restrict__ stats = view_ptr(sa.stats, vo);
    // (no local copy of sa.bl: its per-view depth array would be indexed dynamically in registers, i.e. put into scratch memory)
    const BlendIn& bl = sa.bl;
    const float* __restrict__ bl_c = view_ptr(bl.c, vo); const float* __restrict__ bl_g = view_ptr(bl.g, vo);
    const double* __restrict__ bl_stats_c = view_ptr(bl.stats_c, vo); const double* __restrict__ bl_stats_u = view_ptr(bl.stats_u, vo);
    float* __restrict__ bl_h_out = view_ptr(bl.h_out, vo); float* __restrict__ bl_max_prob = view_ptr(bl.max_prob, vo);
    float* __restrict__ bl_depth_image = view_ptr(bl.depth_image, vo); float* __restrict__ bl_exp_sum = view_ptr(bl.exp_sum, vo);
    constexpr int CT = CA + CB;
    constexpr int TS = 16, PS = TS + 2;
    typedef const __attribute__((address_space(4))) float cfloat;      // wave-uniform -> s_load into SGPRs
    cfloat* wsh = (cfloat*)w;
    __shared__ __attribute__((aligned(16))) float tile[PS * PS * CT];
    __shared__ float red[4][2][2];
    // Round 4: the convolution itself on v_mfma_f32_4x4x1_16B_f32 -- 16 blocks of (4 output channels x 4 pixels), K = 1: a lane
    // stays one pixel, its B operand is the staged input value it already holds, its four result registers are 4 output
    // channels of that pixel, and the A operand (lane m: weight of output channel m & 3) is one LDS read per (tap, channel).
    // Exactly the fused multiply-add chain of the vector form, in the same order: the same bits (tools/small_cell_probe.hip
    // checks it).  The probe (profiles/r04_small_cell_probe.txt) measured the 20 -> 8 convolution at 82.7 TFLOP/s on this
    // form against 48.0 on v_pk_fma_f32 with SGPR weights -- the packed FMA issues at half rate on gfx950, so the matrix
    // instruction is twice the vector ALU's real fp32 rate, without padding for 4- and 8-channel outputs (2 channels: half).
    // MATRIX is chosen by the launcher: the matrix form for ONE reference view per sweep (same-box A/B, c3: 22.49 -> 22.06 ms),
    // the vector form for several views per launch (72.4 against 73.1 ms per 4-view sweep: there the kernels are bound by memory
    // and the sweep by the matrix pipe cell 1 keeps busy; the 5.8 KB weight table costs the 20-channel instances one of their
    // six workgroups per CU).  Both forms give the same bits.
    constexpr bool MFMA44 = MATRIX && (CO == 8 || CO == 4 || CO == 2);
    constexpr int NGRP = CO > 4 ? 2 : 1;               // matrix instructions per (tap, input channel)
    __shared__ __attribute__((aligned(16))) float wl[MFMA44 ? 9 * CT * 4 * NGRP : 4];      // [tap * CT + ci][m & 3][group]
    if (MFMA44) {
        for (int i = threadIdx.x; i < 9 * CT * 4 * NGRP; i += 256) {
            const int g_ = i % NGRP, r_ = (i / NGRP) & 3, k_ = i / (4 * NGRP), co = r_ + 4 * g_;
            wl[i] = co < CO ? w[k_ * CO + co] : 0.f;     // visible to the convolution after the staging barrier below
        }
    }
    // LayerNorm moments -> (mean, 1 / sqrt(var + eps)) ONCE per workgroup (two lanes, then LDS): every thread used to run the
    // float64 divisions and square roots itself, per channel -- ~1000 instruction slots per wave at the head of a kernel whose
    // own work is a few hundred (round 3: the four small-cell kernels 43 / 30 / 27 / 15 us per 4-view plane before)
    // Round 4: the per-channel (scale, shift) pairs too -- CB (MODE 2: 2 * CB) lanes do the float64 arithmetic, everybody reads
    // the float results back as LDS broadcasts (every thread used to redo 4 * CB float64 multiplies and conversions)
    __shared__ float lna[2][CB][2];
    if (MODE != 0) {
        if (threadIdx.x < (MODE == 2 ? 2 * CB : CB)) {
            const int k = threadIdx.x / CB, f = threadIdx.x - k * CB;       // k = 0: reset (MODE 1) / update (MODE 2) gate, 1: candidate
            const double cnt = (double)H * W * CB;
            const double* st = MODE == 1 ? g_stats : (k == 0 ? bl_stats_u : bl_stats_c);
            const double mean = st[0] / cnt;
            double var = st[1] / cnt - mean * mean;
            if (var < 0.0) var = 0.0;
            const double rstd = 1.0 / sqrt(var + 1e-12);              // tf.contrib.layers.layer_norm, eps 1e-12
            const float gamma = MODE == 1 ? r_gamma[f] : (k == 0 ? bl.ug[f] : bl.og[f]);
            const float beta = MODE == 1 ? r_beta[f] : (k == 0 ? bl.ub[f] : bl.ob[f]);
            const double inv = (double)gamma * rstd;
            lna[k][f][0] = (float)inv; lna[k][f][1] = (float)((double)beta - mean * inv);
        }
        __syncthreads();
    }
    float ra[CB], rb[CB];
    if (MODE == 1) {
#pragma unroll
        for (int f = 0; f < CB; ++f) { ra[f] = lna[0][f][0]; rb[f] = lna[0][f][1]; }
    }
    float ua[CB], ub_[CB], ca[CB], cb_[CB];
    if (MODE == 2) {
#pragma unroll
        for (int f = 0; f < CB; ++f) { ua[f] = lna[0][f][0]; ub_[f] = lna[0][f][1]; ca[f] = lna[1][f][0]; cb_[f] = lna[1][f][1]; }
    }
    const int tiles_x = (W + TS - 1) / TS;
    const int ty = bid / tiles_x, tx = bid - ty * tiles_x;
    const int y0 = ty * TS, x0 = tx * TS;
    for (int f = threadIdx.x; f < PS * PS; f += 256) {
        const int r = f / PS, c = f - r * PS;
        const int gy = y0 - 1 + r, gx = x0 - 1 + c;
        float va[CA], vb[CB];
#pragma unroll
        for (int i = 0; i < CA; ++i) va[i] = 0.f;
#pragma unroll
        for (int i = 0; i < CB; ++i) vb[i] = 0.f;
        if (gy >= 0 && gy < H && gx >= 0 && gx < W) {
            const size_t p = (size_t)gy * W + gx;
            load_vec<CA>(xa + p * CA, va);
            load_vec<CB>(xb + p * CB, vb);
            if (MODE == 1) {
                float gr[CB];
                load_vec<CB>(g + p * 2 * CB, gr);
#pragma unroll
                for (int i = 0; i < CB; ++i) vb[i] *= mvs_sigmoid_fast(gr[i] * ra[i] + rb[i]);
            }
            if (MODE == 2) {
                float cv[CB], gu[CB];
                load_vec<CB>(bl_c + p * CB, cv);
                load_vec<CB>(bl_g + p * 2 * CB + CB, gu);
#pragma unroll
                for (int i = 0; i < CB; ++i) {
                    const float uu = mvs_sigmoid_fast(gu[i] * ua[i] + ub_[i]);
                    vb[i] = uu * vb[i] + (1.0f - uu) * mvs_tanh_fast(cv[i] * ca[i] + cb_[i]);
                }
                if (r >= 1 && r <= TS && c >= 1 && c <= TS) {
#pragma unroll
                    for (int i = 0; i < CB; ++i) bl_h_out[p * CB + i] = vb[i];
                }
            }
        }
        float* d = tile + f * CT;
#pragma unroll
        for (int i = 0; i < CA; ++i) d[i] = va[i];
#pragma unroll
        for (int i = 0; i < CB; ++i) d[CA + i] = vb[i];
    }
    __syncthreads();
    const int ly = threadIdx.x >> 4, lx = threadIdx.x & 15;
    const int py = y0 + ly, px = x0 + lx;
    const bool valid = py < H && px < W;
    if (MODE == 2 && bl.pw != nullptr && valid) {     // as prob_wta_kernel: taps outside the image are staged zeros
        float pacc = bl.pbias ? bl.pbias[0] : 0.f;
#pragma unroll
        for (int kh = 0; kh < 3; ++kh)
#pragma unroll
            for (int kw = 0; kw < 3; ++kw) {
                const int gy = py + kh - 1, gx = px + kw - 1;
                if (gy < 0 || gy >= H || gx < 0 || gx >= W) continue;
                const float* tp = tile + ((ly + kh) * PS + lx + kw) * CT + CA;
#pragma unroll
                for (int ci = 0; ci < CB; ++ci) pacc += tp[ci] * bl.pw[(kh * 3 + kw) * CB + ci];
            }
        const float pr = expf(pacc);
        const int pix = py * W + px;
        const float mp = bl_max_prob[pix];
        if (mp < pr) { bl_max_prob[pix] = pr; bl_depth_image[pix] = bl.depth_value[view]; }     // kernarg array, uniform index: s_load
        bl_exp_sum[pix] += pr;
    }
    float acc[CO];
#pragma unroll
    for (int j = 0; j < CO; ++j) acc[j] = bias ? bias[j] : 0.f;
    if constexpr (MFMA44) {
        f32x4 a0 = {0.f, 0.f, 0.f, 0.f}, a1 = a0;
#pragma unroll
        for (int j = 0; j < 4; ++j) { if (j < CO) a0[j] = acc[j]; if (NGRP == 2) a1[j] = acc[CO > 4 ? 4 + j : 0]; }
        const float* wa = wl + (threadIdx.x & 3) * NGRP;
#pragma unroll
        for (int kh = 0; kh < 3; ++kh) {
#pragma unroll
            for (int kw = 0; kw < 3; ++kw) {
                float v[CT];
                load_vec<CT>(tile + ((ly + kh) * PS + lx + kw) * CT, v);
                const float* wt = wa + (kh * 3 + kw) * CT * 4 * NGRP;
#pragma unroll
                for (int ci = 0; ci < CT; ++ci) {
                    if constexpr (NGRP == 2) {
                        const float2 wv = *(const float2*)(wt + ci * 8);
                        a0 = __builtin_amdgcn_mfma_f32_4x4x1f32(wv.x, v[ci], a0, 0, 0, 0);
                        a1 = __builtin_amdgcn_mfma_f32_4x4x1f32(wv.y, v[ci], a1, 0, 0, 0);
                    } else {
                        a0 = __builtin_amdgcn_mfma_f32_4x4x1f32(wt[ci * 4], v[ci], a0, 0, 0, 0);
                    }
                }
            }
        }
#pragma unroll
        for (int j = 0; j < 4; ++j) { if (j < CO) acc[j] = a0[j]; if (NGRP == 2) acc[CO > 4 ? 4 + j : 0] = a1[j]; }
    } else {
#pragma unroll
        for (int kh = 0; kh < 3; ++kh) {
#pragma unroll
            for (int kw = 0; kw < 3; ++kw) {
                float v[CT];
                load_vec<CT>(tile + ((ly + kh) * PS + lx + kw) * CT, v);
                cfloat* wt = wsh + (kh * 3 + kw) * CT * CO;
#pragma unroll
                for (int ci = 0; ci < CT; ++ci)
#pragma unroll
                    for (int j = 0; j < CO; ++j) acc[j] = __builtin_fmaf(v[ci], wt[ci * CO + j], acc[j]);
                // (explicitly fused: written as acc += v * w the 20 -> 4 instance came out with part of its products on
                // v_pk_mul_f32 + v_add_f32, i.e. rounded twice -- legal under -ffp-contract=fast, but not the matrix form's
                // multiply-add chain, and the two forms must give the same bits)
            }
        }
    }
    if (valid) {
        float* dst = y + ((size_t)py * W + px) * CO;
#pragma unroll
        for (int j = 0; j < CO; ++j) dst[j] = acc[j];
    }
    if (stats) {
        const int per = CO / groups;
        const int lane = threadIdx.x & 63, wv = threadIdx.x >> 6;
        for (int gi = 0; gi < groups; ++gi) {
            float sv = 0.f, qv = 0.f;
            if (valid) {
#pragma unroll
                for (int j = 0; j < CO; ++j)      // explicit fused multiply-add: left to -ffp-contract the matrix and the vector
                    if (j / per == gi) { sv += acc[j]; qv = __builtin_fmaf(acc[j], acc[j], qv); }      // form of this kernel came out differently (1 ulp in the moments)
            }
            sv = wave_sum(sv); qv = wave_sum(qv);
            if (lane == 0) { red[wv][gi][0] = sv; red[wv][gi][1] = qv; }
        }
        __syncthreads();
        if (threadIdx.x < groups * 2) {
            int gi = threadIdx.x >> 1, k = threadIdx.x & 1;
            double t = (double)red[0][gi][k] + (double)red[1][gi][k] + (double)red[2][gi][k] + (double)red[3][gi][k];
            atomicAdd(&stats[gi * 2 + k], t);
        }
    }
}

template <int CA, int CB, int CO, int MODE, bool MATRIX>
__global__ void __launch_bounds__(256)
conv2d_small_kernel(SmallArgs a) { conv2d_small_body<CA, CB, CO, MODE, MATRIX>(a, blockIdx.x); }

// cells 2 / 3: gate conv then candidate conv (reset gate folded in)
template <int CA, int F>
void launch_small_cell(const float* xin, float* h, const float* const* p, int H, int W, float* g, float* c,
                       double* sg, double* so, const PrevPlane* prev, Views vw, hipStream_t st, const WtaFold* wta) {
    const dim3 grid(((H + 15) / 16) * ((W + 15) / 16), vw.n);     // 16 x 16 pixel tiles x views
    BlendIn none = {};
    const bool mg = vw.n == 1, mc = vw.n == 1;                      // matrix form for one view per sweep, vector form for several (conv2d_small_body)
    if (prev) {
        BlendIn bl = {c, prev->g, prev->so, prev->sg + 2, p[8], p[9], p[4], p[5], h, nullptr, nullptr, {}, nullptr, nullptr, nullptr};
        if (wta) {
            bl.pw = wta->pw; bl.pbias = wta->pbias; bl.max_prob = wta->max_prob; bl.depth_image = wta->depth_image; bl.exp_sum = wta->exp_sum;
            for (int v = 0; v < MVS_GRU_MAX_VIEWS; ++v) bl.depth_value[v] = wta->depth_value[v];
        }
        const SmallArgs ga{xin, prev->h_before, nullptr, nullptr, nullptr, nullptr, p[0], p[1], H, W, g, sg, 2, bl, vw.stride};
        if (mg) conv2d_small_kernel<CA, F, 2 * F, 2, true><<<grid, 256, 0, st>>>(ga);
        else conv2d_small_kernel<CA, F, 2 * F, 2, false><<<grid, 256, 0, st>>>(ga);
    } else {
        const SmallArgs ga{xin, h, nullptr, nullptr, nullptr, nullptr, p[0], p[1], H, W, g, sg, 2, none, vw.stride};
        if (mg) conv2d_small_kernel<CA, F, 2 * F, 0, true><<<grid, 256, 0, st>>>(ga);
        else conv2d_small_kernel<CA, F, 2 * F, 0, false><<<grid, 256, 0, st>>>(ga);
    }
    const SmallArgs ca{xin, h, g, sg, p[2], p[3], p[6], p[7], H, W, c, so, 1, none, vw.stride};
    if (mc) conv2d_small_kernel<CA, F, F, 1, true><<<grid, 256, 0, st>>>(ca);
    else conv2d_small_kernel<CA, F, F, 1, false><<<grid, 256, 0, st>>>(ca);
}

// the shapes launch_small_cell is instantiated for: the routing predicate and the dispatch read this one table
typedef void (*SmallCellFn)(const float*, float*, const float* const*, int, int, float*, float*, double*, double*, const PrevPlane*,
                            Views, hipStream_t, const WtaFold*);
struct SmallShape { int cin, f; SmallCellFn launch; };
const SmallShape SMALL_SHAPES[] = {{16, 4, launch_small_cell<16, 4>}, {4, 2, launch_small_cell<4, 2>},
                                   {8, 2, launch_small_cell<8, 2>}, {2, 1, launch_small_cell<2, 1>}};
const SmallShape* small_shape(int cin, int f) {
    for (const SmallShape& s : SMALL_SHAPES) if (s.cin == cin && s.f == f) return &s;
    return nullptr;
}

// blend with the update gate evaluated in place: h = u*h + (1-u)*tanh(LN(c)), u = sigmoid(LN(g_u))
// (convgru.py:98,102,114-120); g holds the raw gate convolution (reset | update).  One thread handles
// VEC consecutive channels of a pixel (VEC | F), so the float64 LayerNorm statistics are folded into
// (scale, shift) once per thread instead of once per element.
template <int VEC>
__global__ void __launch_bounds__(256)
gru_blend_fused_kernel(const float* __restrict__ c, const double* __restrict__ stats_c,
                       const float* __restrict__ og, const float* __restrict__ ob,
                       const float* __restrict__ g, const double* __restrict__ stats_u,
                       const float* __restrict__ ug, const float* __restrict__ ub, int HW, int F,
                       const float* h, float* h_out,         // may alias (non-pipelined sweep)
                       size_t vstride) {                     // blockIdx.y = view
    const long long i = ((long long)blockIdx.x * blockDim.x + threadIdx.x) * VEC;
    const size_t vo = (size_t)blockIdx.y * vstride;
    c = view_ptr(c, vo); stats_c = view_ptr(stats_c, vo); g = view_ptr(g, vo); stats_u = view_ptr(stats_u, vo);
    h = view_ptr(h, vo); h_out = view_ptr(h_out, vo);
    // the (scale, shift) pairs of both LayerNorms once per workgroup (2F lanes in float64, then LDS broadcasts): every thread
    // used to run two float64 square roots and 4 * VEC float64 multiplies (F <= 64: the launcher checks)
    __shared__ float aff[2][64][2];
    if (threadIdx.x < 2 * F) {
        const int k = threadIdx.x / F, f = threadIdx.x - k * F;             // k = 0: update gate, 1: candidate
        const double n = (double)HW * F;
        const double* st = k == 0 ? stats_u : stats_c;
        const double mean = st[0] / n;
        double var = st[1] / n - mean * mean; if (var < 0.0) var = 0.0;
        const double inv = (double)(k == 0 ? ug[f] : og[f]) * (1.0 / sqrt(var + 1e-12));
        aff[k][f][0] = (float)inv; aff[k][f][1] = (float)((double)(k == 0 ? ub[f] : ob[f]) - mean * inv);
    }
    __syncthreads();
    if (i >= (long long)HW * F) return;
    const int f = (int)(i % F);
    const long long pix = i / F;
    float cv[VEC], gv[VEC], hv[VEC];
#pragma unroll
    for (int k = 0; k < VEC; ++k) { cv[k] = c[i + k]; gv[k] = g[pix * 2 * F + F + f + k]; hv[k] = h[i + k]; }
#pragma unroll
    for (int k = 0; k < VEC; ++k) {
        const float uu = mvs_sigmoid_fast(gv[k] * aff[0][f + k][0] + aff[0][f + k][1]);
        const float yv = mvs_tanh_fast(cv[k] * aff[1][f + k][0] + aff[1][f + k][1]);
        h_out[i + k] = uu * hv[k] + (1.0f - uu) * yv;
    }
}

// prob_conv (3x3, F3 -> 1, bias) + exp + winner-take-all update in one pass
// (model.py:701-703, 721-731); strict '<' keeps the first maximum.
struct DepthVals { float v[MVS_GRU_MAX_VIEWS]; };
template <int F3>
__global__ void __launch_bounds__(256)
prob_wta_kernel(const float* __restrict__ h3, const float* __restrict__ w, const float* __restrict__ bias,
                DepthVals dv, int H, int W, float* __restrict__ max_prob,
                float* __restrict__ depth_image, float* __restrict__ exp_sum, size_t vstride) {
    int pix = blockIdx.x * blockDim.x + threadIdx.x;
    if (pix >= H * W) return;
    const float depth_value = dv.v[blockIdx.y];
    const size_t vo = (size_t)blockIdx.y * vstride;
    h3 = view_ptr(h3, vo); max_prob = view_ptr(max_prob, vo); depth_image = view_ptr(depth_image, vo); exp_sum = view_ptr(exp_sum, vo);
    int py = pix / W, px = pix - py * W;
    float acc = bias ? bias[0] : 0.f;
#pragma unroll
    for (int kh = 0; kh < 3; ++kh) {
        int iy = py + kh - 1; if (iy < 0 || iy >= H) continue;
#pragma unroll
        for (int kw = 0; kw < 3; ++kw) {
            int ix = px + kw - 1; if (ix < 0 || ix >= W) continue;
            const float* p = h3 + ((size_t)iy * W + ix) * F3;
#pragma unroll
            for (int ci = 0; ci < F3; ++ci) acc += p[ci] * w[(kh * 3 + kw) * F3 + ci];
        }
    }
    float pr = expf(acc);
    float mp = max_prob[pix];
    if (mp < pr) { max_prob[pix] = pr; depth_image[pix] = depth_value; }
    exp_sum[pix] += pr;
}

__global__ void __launch_bounds__(256)
zero_views_kernel(float4* p, size_t n4, size_t vstride) {       // blockIdx.y = view
    size_t i = (size_t)blockIdx.x * blockDim.x + threadIdx.x;
    if (i < n4) view_ptr(p, (size_t)blockIdx.y * vstride)[i] = make_float4(0.f, 0.f, 0.f, 0.f);
}
__global__ void __launch_bounds__(256)
wta_finish_views_kernel(const float* max_prob, const float* exp_sum, const float* depth, int HW, size_t vstride,
                        float* __restrict__ depth_out, float* __restrict__ prob_out) {      // outputs (views, H, W)
    int i = blockIdx.x * blockDim.x + threadIdx.x;
    if (i >= HW) return;
    const size_t vo = (size_t)blockIdx.y * vstride, o = (size_t)blockIdx.y * HW + i;
    prob_out[o] = view_ptr(max_prob, vo)[i] / (view_ptr(exp_sum, vo)[i] + 1e-7f);          // model.py:749-751
    depth_out[o] = view_ptr(depth, vo)[i];
}
}  // namespace

int mvs_gru_conv2d(const float* xa, int Ca, const float* xb, int Cb, const float* w,
                  const float* bias, int H, int W, int Cout, float* y, double* stats, int groups,
                  hipStream_t st) {
    int grid = mvs_cdiv((long long)H * W, 256);
#define MVS_C2D(CO) case CO: conv2d_cat_kernel<CO><<<grid, 256, 0, st>>>(xa, Ca, xb, Cb, w, bias, H, W, y, stats, groups); break;
    switch (Cout) {
        MVS_C2D(1) MVS_C2D(2) MVS_C2D(4) MVS_C2D(8) MVS_C2D(16) MVS_C2D(32)
        // filter counts off the reference's powers of two, and the 'fat' variant's 32-filter cell 1 (a 64-channel gate convolution):
        // mvs_gru_wta*_f32 accepts every f <= 64, and these were MVS_E_SHAPE half-way into its first plane
        MVS_C2D(3) MVS_C2D(6) MVS_C2D(12) MVS_C2D(24) MVS_C2D(64)
        default: return MVS_E_SHAPE;
    }
#undef MVS_C2D
    return (int)hipGetLastError();
}

bool mvs_gru_small_covers(int cin, int f) { return small_shape(cin, f) != nullptr; }
int mvs_gru_small_cell(int cin, int f, const float* xin, float* h, const float* const* p, int H, int W, float* g, float* c,
                       double* sg, double* so, const PrevPlane* prev, Views vw, hipStream_t st, const WtaFold* wta) {
    const SmallShape* s = small_shape(cin, f);
    if (!s) return MVS_E_SHAPE;
    s->launch(xin, h, p, H, W, g, c, sg, so, prev, vw, st, wta);
    return 0;
}

int mvs_gru_blend_views(const float* c, const double* stats_c, const float* og, const float* ob, const float* g, const double* stats_u,
                        const float* ug, const float* ub, int H, int W, int F, const float* h, float* h_out, Views vw, hipStream_t st) {
    const int vec = F % 4 == 0 ? 4 : F % 2 == 0 ? 2 : 1;
    const dim3 grid(mvs_cdiv((long long)H * W * F / vec, 256), vw.n);
    if (vec == 4)
        gru_blend_fused_kernel<4><<<grid, 256, 0, st>>>(c, stats_c, og, ob, g, stats_u, ug, ub, H * W, F, h, h_out, vw.stride);
    else if (vec == 2)
        gru_blend_fused_kernel<2><<<grid, 256, 0, st>>>(c, stats_c, og, ob, g, stats_u, ug, ub, H * W, F, h, h_out, vw.stride);
    else
        gru_blend_fused_kernel<1><<<grid, 256, 0, st>>>(c, stats_c, og, ob, g, stats_u, ug, ub, H * W, F, h, h_out, vw.stride);
    return (int)hipGetLastError();
}

int mvs_gru_zero_views(float* p, size_t nfloat, Views vw, hipStream_t st) {
    const size_t n4 = (nfloat + 3) / 4;
    zero_views_kernel<<<dim3(mvs_cdiv((long long)n4, 256), vw.n), 256, 0, st>>>((float4*)p, n4, vw.stride);
    return (int)hipGetLastError();
}

int mvs_gru_finish_views(const GruWs& ws, int H, int W, Views vw, float* depth_out, float* prob_out, hipStream_t st) {
    wta_finish_views_kernel<<<dim3(mvs_cdiv((long long)H * W, 256), vw.n), 256, 0, st>>>(ws.max_prob, ws.exp_sum, ws.depth, H * W, vw.stride,
                                                                                       depth_out, prob_out);
    return (int)hipGetLastError();
}

extern "C" int mvs_conv2d_cat_f32(const float* xa, int Ca, const float* xb, int Cb, const float* w,
                                  const float* bias, int H, int W, int Cout, float* y,
                                  double* stats, int groups, void* stream) {
    MVS_CHECK_ARG(xa && w && y && Ca > 0 && Cb >= 0 && H > 0 && W > 0 && Cout > 0);
    MVS_CHECK_ARG(Cb == 0 || xb);
    if (stats) { MVS_CHECK_ARG(groups == 1 || groups == 2); if (Cout % groups) return MVS_E_SHAPE; }
    else groups = 1;
    return mvs_gru_conv2d(xa, Ca, xb, Cb, w, bias, H, W, Cout, y, stats, groups, mvs_stream(stream));
}

extern "C" int mvs_gru_gates_f32(const float* g, const double* stats, const float* reset_gamma,
                                 const float* reset_beta, const float* update_gamma,
                                 const float* update_beta, const float* h, int H, int W, int F,
                                 float* rh, float* u, void* stream) {
    MVS_CHECK_ARG(g && stats && reset_gamma && reset_beta && update_gamma && update_beta && h && rh && u);
    MVS_CHECK_ARG(H > 0 && W > 0 && F > 0);
    long long n = (long long)H * W * F;
    gru_gates_kernel<<<mvs_cdiv(n, 256), 256, 0, mvs_stream(stream)>>>(
        g, stats, reset_gamma, reset_beta, update_gamma, update_beta, h, H * W, F, rh, u);
    MVS_LAUNCH_RET();
}

extern "C" int mvs_gru_blend_f32(const float* c, const double* stats, const float* out_gamma,
                                 const float* out_beta, const float* u, int H, int W, int F,
                                 float* h, void* stream) {
    MVS_CHECK_ARG(c && stats && out_gamma && out_beta && u && h && H > 0 && W > 0 && F > 0);
    long long n = (long long)H * W * F;
    gru_blend_kernel<<<mvs_cdiv(n, 256), 256, 0, mvs_stream(stream)>>>(c, stats, out_gamma, out_beta,
                                                                     u, H * W, F, h);
    MVS_LAUNCH_RET();
}

extern "C" int mvs_wta_update_f32(const float* reg, float depth_value, int H, int W,
                                  float* max_prob, float* depth_image, float* exp_sum,
                                  void* stream) {
    MVS_CHECK_ARG(reg && max_prob && depth_image && exp_sum && H > 0 && W > 0);
    wta_update_kernel<<<mvs_cdiv((long long)H * W, 256), 256, 0, mvs_stream(stream)>>>(
        reg, depth_value, H * W, max_prob, depth_image, exp_sum);
    MVS_LAUNCH_RET();
}

extern "C" int mvs_wta_finish_f32(const float* max_prob, const float* exp_sum, int H, int W,
                                  float* prob_out, void* stream) {
    MVS_CHECK_ARG(max_prob && exp_sum && prob_out && H > 0 && W > 0);
    wta_finish_kernel<<<mvs_cdiv((long long)H * W, 256), 256, 0, mvs_stream(stream)>>>(
        max_prob, exp_sum, H * W, prob_out);
    MVS_LAUNCH_RET();
}

int mvs_gru_prob_wta_views(const float* hs, int f3, const WtaFold& w, float* reg, int H, int W, Views vw, hipStream_t st) {
    const dim3 grid(mvs_cdiv((long long)H * W, 256), vw.n);
    auto vp = [&](auto* p, int v) { return (decltype(p))((char*)p + (size_t)v * vw.stride); };     // host-side view pointer
    DepthVals dv = {};
    for (int v = 0; v < vw.n; ++v) dv.v[v] = w.depth_value[v];
    int r;
    switch (f3) {
        case 1: prob_wta_kernel<1><<<grid, 256, 0, st>>>(hs, w.pw, w.pbias, dv, H, W, w.max_prob, w.depth_image, w.exp_sum, vw.stride); break;
        case 2: prob_wta_kernel<2><<<grid, 256, 0, st>>>(hs, w.pw, w.pbias, dv, H, W, w.max_prob, w.depth_image, w.exp_sum, vw.stride); break;
        case 4: prob_wta_kernel<4><<<grid, 256, 0, st>>>(hs, w.pw, w.pbias, dv, H, W, w.max_prob, w.depth_image, w.exp_sum, vw.stride); break;
        default:
            for (int v = 0; v < vw.n; ++v) {
                if ((r = mvs_gru_conv2d(vp(hs, v), f3, nullptr, 0, w.pw, w.pbias, H, W, 1, vp(reg, v), nullptr, 1, st))) return r;
                if ((r = mvs_wta_update_f32(vp(reg, v), dv.v[v], H, W, vp(w.max_prob, v), vp(w.depth_image, v), vp(w.exp_sum, v), st))) return r;
            }
    }
    return (int)hipGetLastError();
}
