// The optimiser steps of training (the reference picks one in mvsnet/train.py:257-266): each is one elementwise launch over
// the flat parameter buffer (all variables of the model are views into it), with the gradient scale folded in.
#include "common.h"

namespace {

// tf.train.RMSPropOptimizer (decay 0.9, momentum 0, epsilon 1e-10, not centered; its `rms` slot starts
// at ONE):  ms += (g*g - ms) * (1 - decay);  mom = momentum*mom + lr * g / sqrt(ms + eps);  w -= mom.
// One launch over the flat parameter buffer (all variables of the model are views into it).
__global__ void __launch_bounds__(256)
rmsprop_kernel(float* __restrict__ w, const float* __restrict__ g, float* __restrict__ ms,
               float* __restrict__ mom, size_t n, float lr, float decay, float momentum, float eps,
               float grad_scale) {
    for (size_t i = (size_t)blockIdx.x * 256 + threadIdx.x; i < n; i += (size_t)gridDim.x * 256) {
        float gi = g[i] * grad_scale;
        float m = ms[i] + (gi * gi - ms[i]) * (1.0f - decay);
        float mo = momentum * mom[i] + lr * gi / sqrtf(m + eps);
        ms[i] = m; mom[i] = mo; w[i] -= mo;
    }
}

// tf.train.MomentumOptimizer (train.py:262-263): accum = momentum*accum + g; w -= lr*accum.
__global__ void __launch_bounds__(256)
momentum_kernel(float* __restrict__ w, const float* __restrict__ g, float* __restrict__ accum, size_t n, float lr,
                float momentum, float grad_scale) {
    for (size_t i = (size_t)blockIdx.x * 256 + threadIdx.x; i < n; i += (size_t)gridDim.x * 256) {
        float a = momentum * accum[i] + g[i] * grad_scale;
        accum[i] = a; w[i] -= lr * a;
    }
}

// tf.train.AdamOptimizer (train.py:266): m, v moments; w -= lr_t * m / (sqrt(v) + eps) with
// lr_t = lr * sqrt(1 - beta2^t) / (1 - beta1^t) formed by the caller.
__global__ void __launch_bounds__(256)
adam_kernel(float* __restrict__ w, const float* __restrict__ g, float* __restrict__ m, float* __restrict__ v,
            size_t n, float lr_t, float beta1, float beta2, float eps, float grad_scale) {
    for (size_t i = (size_t)blockIdx.x * 256 + threadIdx.x; i < n; i += (size_t)gridDim.x * 256) {
        float gi = g[i] * grad_scale;
        float mi = m[i] + (gi - m[i]) * (1.0f - beta1);
        float vi = v[i] + (gi * gi - v[i]) * (1.0f - beta2);
        m[i] = mi; v[i] = vi; w[i] -= lr_t * mi / (sqrtf(vi) + eps);
    }
}

inline int grid_for(size_t n4) { size_t b = (n4 + 255) / 256; return (int)(b < 4096 ? (b ? b : 1) : 4096); }

}  // namespace

extern "C" int mvs_rmsprop_step_f32(float* w, const float* g, float* ms, float* mom, size_t n, float lr,
                                    float decay, float momentum, float eps, float grad_scale, void* stream) {
    MVS_CHECK_ARG(w && g && ms && mom && n > 0);
    rmsprop_kernel<<<grid_for(n), 256, 0, mvs_stream(stream)>>>(w, g, ms, mom, n, lr, decay, momentum, eps, grad_scale);
    MVS_LAUNCH_RET();
}

extern "C" int mvs_momentum_step_f32(float* w, const float* g, float* accum, size_t n, float lr, float momentum,
                                     float grad_scale, void* stream) {
    MVS_CHECK_ARG(w && g && accum && n > 0);
    momentum_kernel<<<grid_for(n), 256, 0, mvs_stream(stream)>>>(w, g, accum, n, lr, momentum, grad_scale);
    MVS_LAUNCH_RET();
}

extern "C" int mvs_adam_step_f32(float* w, const float* g, float* m, float* v, size_t n, float lr_t, float beta1,
                                 float beta2, float eps, float grad_scale, void* stream) {
    MVS_CHECK_ARG(w && g && m && v && n > 0);
    adam_kernel<<<grid_for(n), 256, 0, mvs_stream(stream)>>>(w, g, m, v, n, lr_t, beta1, beta2, eps, grad_scale);
    MVS_LAUNCH_RET();
}
