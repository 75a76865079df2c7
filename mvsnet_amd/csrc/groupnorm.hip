// GroupNorm (+ReLU) of the 2D towers for training (Network.conv_gn / deconv_gn, network.py:217-276,350-409: groups of 8
// channels, biased variance, eps 1e-5): forward and backward passes, and the converter from the inference kernels' GroupNorm
// partial sums to the per-channel statistics these passes read.
#include "common.h"

namespace {

__device__ __forceinline__ float4 ld4(const float* p) { return *reinterpret_cast<const float4*>(p); }
__device__ __forceinline__ void st4(float* p, float4 v) { *reinterpret_cast<float4*>(p) = v; }

// torch's group_norm spends ~0.4 ms per layer in its moments kernel on channel-last tensors (12 of the towers' 14.5 ms
// forward); these are plain HBM passes.
// x (V, HW, C) channel-last; stats (V, 2, C) float64 per-channel [sum, sumsq] (group moments are folded from
// the 8 channel sums of a group wherever they are needed); sums (V, 2, C) float64 [sum gz, sum gz*xhat].
constexpr int GN_CH = 8;
constexpr int GN_BWD_SLOTS = 8;        // copies of the backward sums the workgroups spread their float64 atomics over

// Moments of view v's 8-channel group starting at channel c0, folded from its channels' float64 [sum, sumsq]: the mean and
// 1 / sqrt(biased variance + eps) formed in float64 and rounded once.
__device__ __forceinline__ void gn_group_moments(const double* __restrict__ stats, int v, int c0, int C, size_t hw, float eps,
                                                 float& mean, float& inv) {
    double s = 0.0, q = 0.0;
    for (int k = 0; k < GN_CH; ++k) { s += stats[((size_t)v * 2) * C + c0 + k]; q += stats[((size_t)v * 2 + 1) * C + c0 + k]; }
    const double nn = (double)hw * GN_CH, mu = s / nn;
    double var = q / nn - mu * mu; if (var < 0.0) var = 0.0;
    mean = (float)mu; inv = (float)(1.0 / sqrt(var + (double)eps));
}

// mode 0: stats += [x, x^2];  mode 1: sums += [gz, gz*xhat], gz = g * [gamma*xhat+beta > 0] (when relu)
template <int MODE>
__global__ void __launch_bounds__(256)
gn_reduce_kernel(const float* __restrict__ x, const float* __restrict__ g, const double* __restrict__ stats,
                 const float* __restrict__ gamma, const float* __restrict__ beta, float eps, int relu,
                 size_t hw, int cq, double* __restrict__ out) {
    __shared__ float red[4 * 32][8];                       // [wave][channel quad <= 32][sum, weighted sum]
    const int tid = threadIdx.x, v = blockIdx.y;
    const int c = (tid % cq) * 4, C = cq * 4;
    const size_t n4 = hw * cq;
    const float* xv = x + (size_t)v * n4 * 4;
    const float* gv = MODE ? g + (size_t)v * n4 * 4 : nullptr;
    float mean = 0.f, inv = 1.f, ga[4] = {1, 1, 1, 1}, be[4] = {0, 0, 0, 0};
    if (MODE) {
        gn_group_moments(stats, v, c & ~(GN_CH - 1), C, hw, eps, mean, inv);
        for (int k = 0; k < 4; ++k) { ga[k] = gamma[c + k]; be[k] = beta[c + k]; }
    }
    float a[4] = {0.f, 0.f, 0.f, 0.f}, b[4] = {0.f, 0.f, 0.f, 0.f};
    auto fold = [&](const float4 xx, const float4 g4) {
        const float vv[4] = {xx.x, xx.y, xx.z, xx.w};
        if (MODE == 0) {
#pragma unroll
            for (int k = 0; k < 4; ++k) { a[k] += vv[k]; b[k] += vv[k] * vv[k]; }
        } else {
            const float gg[4] = {g4.x, g4.y, g4.z, g4.w};
#pragma unroll
            for (int k = 0; k < 4; ++k) {
                const float xh = (vv[k] - mean) * inv;
                const float gz = (!relu || ga[k] * xh + be[k] > 0.f) ? gg[k] : 0.f;
                a[k] += gz; b[k] += gz * xh;
            }
        }
    };
    // four elements per trip, their loads issued together: with one per trip a full-resolution layer was ~19 dependent trips of
    // two loads per thread on 384 workgroups -- latency-bound at 38 us per launch on average (round 6's trace of the training step)
    const size_t stride = (size_t)gridDim.x * 256;
    size_t i = (size_t)blockIdx.x * 256 + tid;
    for (; i + 3 * stride < n4; i += 4 * stride) {
        float4 xx[4], g4[4];
#pragma unroll
        for (int u = 0; u < 4; ++u) {
            xx[u] = ld4(xv + 4 * (i + u * stride));
            g4[u] = MODE ? ld4(gv + 4 * (i + u * stride)) : make_float4(0.f, 0.f, 0.f, 0.f);
        }
#pragma unroll
        for (int u = 0; u < 4; ++u) fold(xx[u], g4[u]);
    }
    for (; i < n4; i += stride) fold(ld4(xv + 4 * i), MODE ? ld4(gv + 4 * i) : make_float4(0.f, 0.f, 0.f, 0.f));
    // lanes l, l + cq, l + 2 cq, ... of a wave hold the same channel quad (cq divides 64): butterfly over the offsets >= cq, then
    // the four waves' rows through LDS (with 8 channels the old tree had TWO threads walk 128 rows each: +5 us per launch)
#pragma unroll
    for (int k = 0; k < 4; ++k)
        for (int o = 32; o >= cq; o >>= 1) { a[k] += __shfl_xor(a[k], o, 64); b[k] += __shfl_xor(b[k], o, 64); }
    if ((tid & 63) < cq) {
#pragma unroll
        for (int k = 0; k < 4; ++k) { red[(tid >> 6) * 32 + (tid & 63)][k] = a[k]; red[(tid >> 6) * 32 + (tid & 63)][4 + k] = b[k]; }
    }
    __syncthreads();
    if (tid < cq) {
        double sa[4] = {0, 0, 0, 0}, sb[4] = {0, 0, 0, 0};
        for (int w = 0; w < 4; ++w)
#pragma unroll
            for (int k = 0; k < 4; ++k) { sa[k] += red[w * 32 + tid][k]; sb[k] += red[w * 32 + tid][4 + k]; }
        // MODE 1: the partial sums go to one of GN_BWD_SLOTS copies of `out`, which the apply pass adds up as it reads them.
        // Atomics on ONE address are performed one after the other by the L2, ~40 ns each (tools/r6_gn_reduce_probe.py: a
        // launch of 384 workgroups cost 15 us more than one of 128 whatever the tensor's size): round 6 first let every
        // workgroup add to per-layer totals as well, then take a ticket so that the last one would fold -- either way 384
        // serialised atomics, 30-52 us per launch in the training step against 5-23 us for the element-wise pass over the
        // same tensors.  No cross-workgroup step is left here: 16 atomics per address and slot.
        double* dst = out + (MODE ? (size_t)(blockIdx.x % GN_BWD_SLOTS) * gridDim.y * 2 * C : 0);
#pragma unroll
        for (int k = 0; k < 4; ++k) {
            atomicAdd(dst + ((size_t)v * 2) * C + c + k, sa[k]);
            atomicAdd(dst + ((size_t)v * 2 + 1) * C + c + k, sb[k]);
        }
    }
}

// mode 0: y = act(gamma*xhat + beta);  mode 1: dx = inv * (gamma*gz - mean_g(gamma*gz) - xhat * mean_g(gamma*gz*xhat))
template <int MODE>
__global__ void __launch_bounds__(256)
gn_apply_kernel(const float* __restrict__ x, const float* __restrict__ g, const double* __restrict__ stats,
                const double* __restrict__ sums, const float* __restrict__ gamma, const float* __restrict__ beta,
                float eps, int relu, size_t hw, int cq, float* __restrict__ out, double* __restrict__ tot = nullptr) {
    const int tid = threadIdx.x, v = blockIdx.y;
    const int c = (tid % cq) * 4, C = cq * 4;
    const size_t n4 = hw * cq;
    const int c0 = c & ~(GN_CH - 1);
    const size_t plane = (size_t)gridDim.y * 2 * C;       // one slot of the backward sums: (V, 2, C)
    if (MODE && tot && blockIdx.x == 0 && blockIdx.y == 0) {
        // (2, C) over all views and slots: d beta, d gamma -- one workgroup, one thread per (statistic, channel); C <= 128
        if (tid < 2 * C) {
            double acc = 0.0;
            for (unsigned vv = 0; vv < gridDim.y; ++vv)
#pragma unroll
                for (int sl = 0; sl < GN_BWD_SLOTS; ++sl) acc += sums[sl * plane + (size_t)vv * 2 * C + tid];
            tot[tid] += acc;
        }
    }
    // the slots of this view's backward sums, added up ONCE per workgroup (one thread per (statistic, channel), C <= 128), not by
    // every thread for its own group (128 float64 loads per thread: the pass took 37 instead of 15 us on a 240 x 320 x 16 layer)
    __shared__ double folded[2 * 128];
    if (MODE) {
        if (tid < 2 * C) {
            double acc = 0.0;
#pragma unroll
            for (int sl = 0; sl < GN_BWD_SLOTS; ++sl) acc += sums[sl * plane + (size_t)v * 2 * C + tid];
            folded[tid] = acc;
        }
        __syncthreads();
    }
    float mean, inv;
    gn_group_moments(stats, v, c0, C, hw, eps, mean, inv);
    double ta = 0.0, tb = 0.0;
    if (MODE)
        for (int k = 0; k < GN_CH; ++k) {
            ta += (double)gamma[c0 + k] * folded[c0 + k];
            tb += (double)gamma[c0 + k] * folded[C + c0 + k];
        }
    const double nn = (double)hw * GN_CH;
    const float m1 = (float)(ta / nn), m2 = (float)(tb / nn);
    float ga[4], be[4];
#pragma unroll
    for (int k = 0; k < 4; ++k) { ga[k] = gamma[c + k]; be[k] = beta[c + k]; }
    const float* xv = x + (size_t)v * n4 * 4;
    const float* gv = MODE ? g + (size_t)v * n4 * 4 : nullptr;
    float* ov = out + (size_t)v * n4 * 4;
    for (size_t i = (size_t)blockIdx.x * 256 + tid; i < n4; i += (size_t)gridDim.x * 256) {
        const float4 xx = ld4(xv + 4 * i);
        const float vv[4] = {xx.x, xx.y, xx.z, xx.w};
        float o[4];
        if (MODE == 0) {
#pragma unroll
            for (int k = 0; k < 4; ++k) {
                const float z = ga[k] * ((vv[k] - mean) * inv) + be[k];
                o[k] = relu ? fmaxf(z, 0.f) : z;
            }
        } else {
            const float4 g4 = ld4(gv + 4 * i);
            const float gg[4] = {g4.x, g4.y, g4.z, g4.w};
#pragma unroll
            for (int k = 0; k < 4; ++k) {
                const float xh = (vv[k] - mean) * inv;
                const float gz = (!relu || ga[k] * xh + be[k] > 0.f) ? gg[k] : 0.f;
                o[k] = inv * (ga[k] * gz - m1 - xh * m2);
            }
        }
        st4(ov + 4 * i, make_float4(o[0], o[1], o[2], o[3]));
    }
}

}  // namespace

// The inference kernels' GroupNorm sums -- (V, C/8, slots, 2) float64 partial [sum, sumsq] per 8-channel group (csrc/unet2d*.hip) --
// in the per-channel layout of the kernels above: every channel of a group carries an eighth of the group's totals, so the
// group moments folded from "the 8 channel sums" are the forward's own.  The training towers need no second pass over the
// activations for statistics the forward convolution already produced (round 6: 31 launches and 0.6 ms of a 6 ms step).
// All layers of a tower in one launch: layer i's slots start `slot_off[i]` float64 behind `slots`, its (V, 2, C_i) statistics
// `stat_off[i]` behind `stats` (the jobs ride in the kernel arguments; blockIdx.y = layer).
constexpr int GN_MANY_MAX = 64;
struct GnManyJobs { long long slot_off[GN_MANY_MAX], stat_off[GN_MANY_MAX]; int C[GN_MANY_MAX]; };

__global__ void gn_slots_to_channel_sums_many_kernel(const double* __restrict__ slots, int V, int nslot, double* __restrict__ stats,
                                                     GnManyJobs jobs) {
    const int C = jobs.C[blockIdx.y];
    const double* sl = slots + jobs.slot_off[blockIdx.y];
    double* out = stats + jobs.stat_off[blockIdx.y];
    for (int i = blockIdx.x * blockDim.x + threadIdx.x; i < V * 2 * C; i += gridDim.x * blockDim.x) {
        const int c = i % C, k = (i / C) & 1, v = i / (2 * C);
        const double* p = sl + (((size_t)v * (C / GN_CH) + c / GN_CH) * nslot) * 2 + k;
        double t = 0.0;
        for (int s_ = 0; s_ < nslot; ++s_) t += p[2 * s_];
        out[i] = t * 0.125;
    }
}

extern "C" int mvs_gn_slots_to_channel_sums_many_f64(int n, const double* slots, const long long* slot_off, const int* C, int V,
                                                     int nslot, double* stats, const long long* stat_off, void* stream) {
    MVS_CHECK_ARG(n > 0 && slots && slot_off && C && stats && stat_off && V > 0 && nslot > 0);
    for (int i = 0; i < n; ++i) {
        MVS_CHECK_ARG(C[i] > 0 && slot_off[i] >= 0 && stat_off[i] >= 0);
        if (C[i] % GN_CH) return MVS_E_SHAPE;
    }
    for (int first = 0; first < n; first += GN_MANY_MAX) {
        const int m = n - first < GN_MANY_MAX ? n - first : GN_MANY_MAX;
        GnManyJobs jobs;
        int cmax = 1;
        for (int k = 0; k < m; ++k) {
            jobs.slot_off[k] = slot_off[first + k]; jobs.stat_off[k] = stat_off[first + k]; jobs.C[k] = C[first + k];
            if (C[first + k] > cmax) cmax = C[first + k];
        }
        hipLaunchKernelGGL(gn_slots_to_channel_sums_many_kernel, dim3(mvs_cdiv((long long)V * 2 * cmax, 256), m), dim3(256), 0,
                           mvs_stream(stream), slots, V, nslot, stats, jobs);
    }
    MVS_LAUNCH_RET();
}

extern "C" int mvs_gn_slots_to_channel_sums_f64(const double* slots, int V, int C, int nslot, double* stats, void* stream) {
    const long long off = 0;                                   // one layer: a one-job call of the launch above
    return mvs_gn_slots_to_channel_sums_many_f64(1, slots, &off, &C, V, nslot, stats, &off, stream);
}

// GroupNorm entry points: mode selects the pass (see the kernels above).
static int gn_check(const void* x, int V, size_t hw, int C) {
    if (!x || V <= 0 || hw == 0 || C <= 0) return MVS_E_BADARG;
    if (C % GN_CH || 256 % (C / 4) || C > 128) return MVS_E_SHAPE;     // a wave's lanes cover whole rows of C / 4 quads; LDS rows for <= 32 quads
    return 0;
}
// Workgroups per view of the reductions (each ends with float64 atomics on shared cache lines: see GN_BWD_SLOTS).
#ifndef GN_REDUCE_BLOCKS
#define GN_REDUCE_BLOCKS 128
#endif

static dim3 gn_grid(size_t hw, int C, int V, int cap) {
    size_t b = (hw * (size_t)(C / 4) + 255) / 256;
    return dim3((unsigned)(b < (size_t)cap ? (b ? b : 1) : cap), V);
}

extern "C" int mvs_gn_stats_f32(const float* x, int V, size_t hw, int C, double* stats, void* stream) {
    int rc = gn_check(x, V, hw, C); if (rc) return rc;
    MVS_CHECK_ARG(stats);
    gn_reduce_kernel<0><<<gn_grid(hw, C, V, GN_REDUCE_BLOCKS), 256, 0, mvs_stream(stream)>>>(x, nullptr, nullptr, nullptr, nullptr, 0.f, 0,
                                                                                hw, C / 4, stats);
    MVS_LAUNCH_RET();
}

extern "C" int mvs_gn_apply_f32(const float* x, const double* stats, const float* gamma, const float* beta, float eps,
                                int relu, int V, size_t hw, int C, float* y, void* stream) {
    int rc = gn_check(x, V, hw, C); if (rc) return rc;
    MVS_CHECK_ARG(stats && gamma && beta && y);
    gn_apply_kernel<0><<<gn_grid(hw, C, V, 2048), 256, 0, mvs_stream(stream)>>>(x, nullptr, stats, nullptr, gamma, beta, eps, relu,
                                                                                hw, C / 4, y);
    MVS_LAUNCH_RET();
}

// `sums`: mvs_gn_bwd_sums_doubles(V, C) float64, zeroed by the caller: mvs_gn_bwd_sum_slots() copies of (V, 2, C) that the
// workgroups spread their atomics over; the apply pass (and whoever wants d gamma / d beta) adds the copies up.
extern "C" int mvs_gn_bwd_sum_slots(void) { return GN_BWD_SLOTS; }
extern "C" size_t mvs_gn_bwd_sums_doubles(int V, int C) {
    return (V > 0 && C > 0) ? (size_t)GN_BWD_SLOTS * V * 2 * C : 0;
}

extern "C" int mvs_gn_bwd_reduce_f32(const float* x, const double* stats, const float* gamma, const float* beta, float eps,
                                     int relu, const float* g, int V, size_t hw, int C, double* sums, void* stream) {
    int rc = gn_check(x, V, hw, C); if (rc) return rc;
    MVS_CHECK_ARG(stats && gamma && beta && g && sums);
    gn_reduce_kernel<1><<<gn_grid(hw, C, V, GN_REDUCE_BLOCKS), 256, 0, mvs_stream(stream)>>>(x, g, stats, gamma, beta, eps, relu, hw, C / 4, sums);
    MVS_LAUNCH_RET();
}

extern "C" int mvs_gn_bwd_apply_f32(const float* x, const double* stats, const float* gamma, const float* beta, float eps,
                                    int relu, const float* g, const double* sums, int V, size_t hw, int C, float* dx,
                                    void* stream) {
    int rc = gn_check(x, V, hw, C); if (rc) return rc;
    MVS_CHECK_ARG(stats && gamma && beta && g && sums && dx);
    gn_apply_kernel<1><<<gn_grid(hw, C, V, 2048), 256, 0, mvs_stream(stream)>>>(x, g, stats, sums, gamma, beta, eps, relu,
                                                                                hw, C / 4, dx);
    MVS_LAUNCH_RET();
}

// The same, and the sums over ALL views and slots ADDED to totals (2, C) float64 [d beta, d gamma] by the first workgroup: the
// parameter gradients without a reduction launch per layer.  C <= 128.
extern "C" int mvs_gn_bwd_apply_tot_f32(const float* x, const double* stats, const float* gamma, const float* beta, float eps,
                                        int relu, const float* g, const double* sums, double* totals, int V, size_t hw, int C,
                                        float* dx, void* stream) {
    int rc = gn_check(x, V, hw, C); if (rc) return rc;
    MVS_CHECK_ARG(stats && gamma && beta && g && sums && totals && dx);
    gn_apply_kernel<1><<<gn_grid(hw, C, V, 2048), 256, 0, mvs_stream(stream)>>>(x, g, stats, sums, gamma, beta, eps, relu,
                                                                                hw, C / 4, dx, totals);
    MVS_LAUNCH_RET();
}
