// Rasterisation of a triangle mesh into per-view depth maps (mvs_raster_mesh_f32) and interpolation of vertex attributes
// over the result (mvs_raster_interpolate_f32).  The semantics are normative in mvsnet_amd/render_mesh.py;
// tests/raster_reference.py restates them in numpy.
//
//   clear     the 8-byte keys of all V*H*W pixels are set to all ones (empty), the queue counter to 0;
//   small     one lane per face, taken in `order`; the three vertices are read once and the view loop runs inside the lane,
//             RS_VIEWS views at a time.  Per view the three float32 projections (P_v's twelve floats in scalar registers),
//             the snap to 1/256 pixel, the int64 area and the clipped bounding box.  A lane walks its RS_VIEWS boxes in
//             step: per step one pixel of each, the three int64 edge functions, and for a covered pixel the float64 depth
//             and key = bits(z) << 32 | face index: one plain load of the pixel's current key, and only when the lane's key
//             is smaller one 64-bit unsigned atomic min at agent scope.  Keys only decrease, so a stale load can only cost
//             an atomic, never an answer.  A (face, view) pair whose box holds more than large_pixels pixels is appended
//             to the queue instead (one 64-bit add on the counter, one 8-byte store); when the queue is full the lane
//             walks the box itself;
//   large     a fixed grid of workgroups reads the counter (the kernel boundary makes it and the entries visible) and
//             takes the entries blockIdx.x, + gridDim.x, ...: every lane repeats the setup, then the 64 x 4 lanes stride over
//             the box, rows of 64 pixels side by side;
//   resolve   keys -> depth (0 where empty) and index (-1 where empty).
//   interpolate   one lane per pixel: the setup of the face its index names, the edge functions at the pixel, and per
//             channel ((t_a A_a + t_b A_b) + t_c A_c) / ((t_a + t_b) + t_c) in float64.
// Every float operation is rounded on its own (contraction off); the only atomics on the output are unsigned minima, so no
// byte depends on the order of execution, the grid, the processing order, large_pixels or queue_capacity.
#include "geom_common.h"

namespace {

constexpr int RS_THREADS = 256;
constexpr int RS_BLOCKS = 2048;                 // fixed grid of the small kernel: 8 workgroups per CU
constexpr int RS_LARGE_BLOCKS = 1024;           // fixed grid of the large kernel
constexpr int RS_VIEWS = 4;                     // views a lane works on at once (loads in flight)
constexpr int RS_MAX_AXIS = 1 << 20;            // H, W: 256 x stays inside the guard band
constexpr int RS_MAX_CHANNELS = 8;
constexpr float RS_GUARD = 268435456.f;         // 2^28, in 1/256 pixel
constexpr size_t RS_HEAD_BYTES = 256;           // the queue counter, in a block of its own at the workspace's start

// One face in one view after the setup: corners in 1/256 pixel, their depths, sign of the area, clipped bounding box.
struct RsTri {
    int xa, ya, xb, yb, xc, yc;
    float wa, wb, wc;
    int sgn;
    long long area;                             // |area2|
    int x0, x1, y0, y1;
};

// Projects and snaps one vertex; false when it is unusable in this view (then qx = qy = 0).
__device__ __forceinline__ bool rs_vertex(const float* __restrict__ P, const float* p, float min_depth, int& qx, int& qy, float& w) {
#pragma clang fp contract(off)
    const float u = geo_row(P, p[0], p[1], p[2]), v = geo_row(P + 4, p[0], p[1], p[2]);
    w = geo_row(P + 8, p[0], p[1], p[2]);
    const float fx = floorf(__fdiv_rn(u, w) * 256.f + 0.5f), fy = floorf(__fdiv_rn(v, w) * 256.f + 0.5f);
    // compared in float32, before any conversion; a NaN fails every comparison
    const bool ok = __builtin_isfinite(w) && w > min_depth && fabsf(fx) <= RS_GUARD && fabsf(fy) <= RS_GUARD;
    qx = ok ? (int)fx : 0;
    qy = ok ? (int)fy : 0;
    return ok;
}

// The nine coordinates of face f -> p[9]; false for a face or vertex index outside its range (nothing is dereferenced then).
__device__ __forceinline__ bool rs_load_face(const float* __restrict__ vertices, int M, const int* __restrict__ faces, int F, int f,
                                             float* p, int* abc) {
    if ((unsigned)f >= (unsigned)F) return false;
    const int a = faces[3 * (size_t)f], b = faces[3 * (size_t)f + 1], c = faces[3 * (size_t)f + 2];
    if ((unsigned)a >= (unsigned)M || (unsigned)b >= (unsigned)M || (unsigned)c >= (unsigned)M) return false;
    abc[0] = a, abc[1] = b, abc[2] = c;
#pragma unroll
    for (int k = 0; k < 3; ++k) {
        p[k] = vertices[3 * (size_t)a + k];
        p[3 + k] = vertices[3 * (size_t)b + k];
        p[6 + k] = vertices[3 * (size_t)c + k];
    }
    return true;
}

// The setup of one face in one view; false when the face is dropped there.  The bounding box may still be empty.
__device__ __forceinline__ bool rs_setup(const float* __restrict__ P, const float* p, float min_depth, int cull, int H, int W, RsTri& t) {
    bool ok = rs_vertex(P, p, min_depth, t.xa, t.ya, t.wa);
    ok &= rs_vertex(P, p + 3, min_depth, t.xb, t.yb, t.wb);
    ok &= rs_vertex(P, p + 6, min_depth, t.xc, t.yc, t.wc);
    // |q| <= 2^28: differences fit 30 bits, products 59
    const long long area2 = (long long)(t.xb - t.xa) * (t.yc - t.ya) - (long long)(t.yb - t.ya) * (t.xc - t.xa);
    t.sgn = area2 > 0 ? 1 : -1;
    t.area = area2 > 0 ? area2 : -area2;
    ok &= area2 != 0 && !(cull > 0 && area2 > 0) && !(cull < 0 && area2 < 0);
    // [ceil(min / 256), floor(max / 256)] by arithmetic shifts, clipped to the image
    t.x0 = max((min(t.xa, min(t.xb, t.xc)) + 255) >> 8, 0);
    t.x1 = min(max(t.xa, max(t.xb, t.xc)) >> 8, W - 1);
    t.y0 = max((min(t.ya, min(t.yb, t.yc)) + 255) >> 8, 0);
    t.y1 = min(max(t.ya, max(t.yb, t.yc)) >> 8, H - 1);
    return ok;
}

// sgn [(xe - xs)(py - ys) - (ye - ys)(px - xs)] and whether p is inside the edge or on it while the edge owns its points.
__device__ __forceinline__ bool rs_edge(int sgn, int xs, int ys, int xe, int ye, int px, int py, long long& e) {
    const int dx = xe - xs, dy = ye - ys;
    e = sgn * ((long long)dx * (py - ys) - (long long)dy * (px - xs));
    const int ox = sgn * dx, oy = sgn * dy;
    return e > 0 || (e == 0 && (oy > 0 || (oy == 0 && ox < 0)));
}

// The three edge functions at pixel (x, y), 0 <= x, y <= 2^20 -> covered.
__device__ __forceinline__ bool rs_cover(const RsTri& t, int x, int y, long long& ea, long long& eb, long long& ec) {
    const int px = x << 8, py = y << 8;
    const bool a = rs_edge(t.sgn, t.xb, t.yb, t.xc, t.yc, px, py, ea);
    const bool b = rs_edge(t.sgn, t.xc, t.yc, t.xa, t.ya, px, py, eb);
    const bool c = rs_edge(t.sgn, t.xa, t.ya, t.xb, t.yb, px, py, ec);
    return a && b && c;
}

// t_k = double(e_k) (1 / double(w_k)); -> the sum (t_a + t_b) + t_c.  hipcc's float64 division is correctly rounded.
__device__ __forceinline__ double rs_weights(const RsTri& t, long long ea, long long eb, long long ec, double& ta, double& tb, double& tc) {
#pragma clang fp contract(off)
    ta = (double)ea * (1.0 / (double)t.wa);
    tb = (double)eb * (1.0 / (double)t.wb);
    tc = (double)ec * (1.0 / (double)t.wc);
    return (ta + tb) + tc;
}

__device__ __forceinline__ unsigned long long rs_key(const RsTri& t, long long ea, long long eb, long long ec, int f) {
#pragma clang fp contract(off)
    double ta, tb, tc;
    const double s = rs_weights(t, ea, eb, ec, ta, tb, tc);
    const float z = (float)((double)t.area / s);
    return geo_key(z, f);
}

// grid (blocks over the faces, chunks of views): lane L of a row of blocks takes faces order[L], order[L + lanes], ...
__global__ __launch_bounds__(RS_THREADS) void rs_small_kernel(const float* __restrict__ vertices, int M, const int* __restrict__ faces,
                                                               int F, const int* __restrict__ order, const float* __restrict__ proj,
                                                               int V, int views_per_chunk, int H, int W, float min_depth, int cull,
                                                               long long large_pixels, int queue_capacity,
                                                               unsigned long long* __restrict__ keys,
                                                               unsigned long long* __restrict__ counter,
                                                               unsigned long long* __restrict__ queue) {
    const int v0 = blockIdx.y * views_per_chunk, v1 = min(V, v0 + views_per_chunk);
    const size_t plane = (size_t)H * W;
    for (long long i = (long long)blockIdx.x * RS_THREADS + threadIdx.x; i < F; i += (long long)gridDim.x * RS_THREADS) {
        const int f = order ? order[i] : (int)i;
        float p[9];
        int abc[3];
        if (!rs_load_face(vertices, M, faces, F, f, p, abc)) continue;     // a bad face or order entry: dropped, nothing read
        for (int vb = v0; vb < v1; vb += RS_VIEWS) {
            RsTri t[RS_VIEWS];
            int cx[RS_VIEWS], cy[RS_VIEWS];
            bool act[RS_VIEWS];
#pragma unroll
            for (int k = 0; k < RS_VIEWS; ++k) {
                const int v = min(vb + k, v1 - 1);                         // wave-uniform: P arrives by scalar loads
                bool ok = rs_setup(proj + 12 * (size_t)v, p, min_depth, cull, H, W, t[k]);
                ok = ok && vb + k < v1 && t[k].x0 <= t[k].x1 && t[k].y0 <= t[k].y1;
                if (ok && (long long)(t[k].x1 - t[k].x0 + 1) * (t[k].y1 - t[k].y0 + 1) > large_pixels && queue_capacity > 0) {
                    const unsigned long long slot = atomicAdd(counter, 1ull);
                    if (slot < (unsigned long long)queue_capacity) {       // a full queue: the lane walks the box itself
                        queue[slot] = ((unsigned long long)(unsigned)(vb + k) << 32) | (unsigned)f;
                        ok = false;
                    }
                }
                act[k] = ok;
                cx[k] = t[k].x0;
                cy[k] = t[k].y0;
            }
            while (act[0] || act[1] || act[2] || act[3]) {
                // one pixel of each view's box per step: all loads before the first atomic, so a lane keeps RS_VIEWS gathers
                // in flight (an atomic stays counted in vmcnt for hundreds of cycles)
                size_t at[RS_VIEWS];
                unsigned long long key[RS_VIEWS], cur[RS_VIEWS];
#pragma unroll
                for (int k = 0; k < RS_VIEWS; ++k) {
                    long long ea, eb, ec;
                    const bool hit = act[k] && rs_cover(t[k], cx[k], cy[k], ea, eb, ec);
                    key[k] = GEO_EMPTY;
                    if (hit) key[k] = rs_key(t[k], ea, eb, ec, f);
                    // a lane without a hit loads key 0 of the buffer and masks it to 0: no key is smaller, no atomic follows
                    at[k] = hit ? (size_t)(vb + k) * plane + (size_t)cy[k] * W + cx[k] : (size_t)0;
                    cur[k] = keys[at[k]] & (hit ? ~0ull : 0ull);
                }
                static_assert(RS_VIEWS == 4, "the loop condition above and the barrier below name four values");
                asm volatile("" : "+v"(cur[0]), "+v"(cur[1]), "+v"(cur[2]), "+v"(cur[3]));
#pragma unroll
                for (int k = 0; k < RS_VIEWS; ++k) {
                    if (key[k] < cur[k]) __hip_atomic_fetch_min(keys + at[k], key[k], __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
                    if (act[k] && ++cx[k] > t[k].x1) {
                        cx[k] = t[k].x0;
                        if (++cy[k] > t[k].y1) act[k] = false;
                    }
                }
            }
        }
    }
}

// One workgroup per queue entry at a time; 64 lanes along x, 4 rows.
__global__ __launch_bounds__(RS_THREADS) void rs_large_kernel(const float* __restrict__ vertices, int M, const int* __restrict__ faces,
                                                               int F, const float* __restrict__ proj, int V, int H, int W,
                                                               float min_depth, int cull, int queue_capacity,
                                                               unsigned long long* __restrict__ keys,
                                                               const unsigned long long* __restrict__ counter,
                                                               const unsigned long long* __restrict__ queue) {
    const unsigned long long n = min(counter[0], (unsigned long long)queue_capacity);
    const size_t plane = (size_t)H * W;
    const int lx = threadIdx.x & 63, ly = threadIdx.x >> 6;
    for (unsigned long long e = blockIdx.x; e < n; e += gridDim.x) {
        const unsigned long long q = queue[e];
        const int f = (int)(unsigned)q, v = (int)(q >> 32);
        float p[9];
        int abc[3];
        RsTri t;
        if ((unsigned)v >= (unsigned)V || !rs_load_face(vertices, M, faces, F, f, p, abc)) continue;
        if (!rs_setup(proj + 12 * (size_t)v, p, min_depth, cull, H, W, t)) continue;
        for (int y = t.y0 + ly; y <= t.y1; y += RS_THREADS / 64)
            for (int x = t.x0 + lx; x <= t.x1; x += 64) {
                long long ea, eb, ec;
                if (!rs_cover(t, x, y, ea, eb, ec)) continue;
                const unsigned long long key = rs_key(t, ea, eb, ec, f);
                unsigned long long* at = keys + (size_t)v * plane + (size_t)y * W + x;
                if (key < *at) __hip_atomic_fetch_min(at, key, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
            }
    }
}

// One lane per pixel of all views: C channels of the face its index names, 0 for an empty pixel, an index outside 0..F-1
// or a face that is dropped in the view.
__global__ __launch_bounds__(RS_THREADS) void rs_interpolate_kernel(const float* __restrict__ vertices, int M,
                                                                     const int* __restrict__ faces, int F,
                                                                     const float* __restrict__ proj, long long pixels, int H, int W,
                                                                     float min_depth, const int* __restrict__ index,
                                                                     const float* __restrict__ attr, int C, float* __restrict__ out) {
#pragma clang fp contract(off)
    const long long pix = (long long)blockIdx.x * RS_THREADS + threadIdx.x;
    if (pix >= pixels) return;
    const long long plane = (long long)H * W;
    const int v = (int)(pix / plane), r = (int)(pix % plane);
    float res[RS_MAX_CHANNELS];
#pragma unroll
    for (int c = 0; c < RS_MAX_CHANNELS; ++c) res[c] = 0.f;
    float p[9];
    int abc[3];
    RsTri t;
    if (rs_load_face(vertices, M, faces, F, index[pix], p, abc) && rs_setup(proj + 12 * (size_t)v, p, min_depth, 0, H, W, t)) {
        long long ea, eb, ec;
        rs_cover(t, r % W, r / W, ea, eb, ec);
        double ta, tb, tc;
        const double s = rs_weights(t, ea, eb, ec, ta, tb, tc);
#pragma unroll
        for (int c = 0; c < RS_MAX_CHANNELS; ++c)
            if (c < C) {
                const double A = attr[(size_t)abc[0] * C + c], B = attr[(size_t)abc[1] * C + c], G = attr[(size_t)abc[2] * C + c];
                res[c] = (float)(((ta * A + tb * B) + tc * G) / s);
            }
    }
#pragma unroll
    for (int c = 0; c < RS_MAX_CHANNELS; ++c)
        if (c < C) out[(size_t)pix * C + c] = res[c];
}

// [counter block | keys | queue]
struct RsLayout { size_t counter, keys, queue, total; };

RsLayout rs_layout(long long pixels, int queue_capacity) {
    GeoCarver c;
    return {c.take(RS_HEAD_BYTES), c.take((size_t)pixels * sizeof(unsigned long long)),
            c.take((size_t)queue_capacity * sizeof(unsigned long long)), c.off};
}

}  // namespace

extern "C" size_t mvs_raster_workspace_bytes(int V, int H, int W, int queue_capacity) {
    if (V <= 0 || H <= 0 || W <= 0 || queue_capacity < 0 || !geo_pixels_ok(V, H, W, RS_MAX_AXIS)) return 0;
    return rs_layout((long long)V * H * W, queue_capacity).total;
}

extern "C" int mvs_raster_mesh_f32(const float* vertices, int M, const int* faces, int F, const int* order, const float* proj, int V,
                                   int H, int W, float min_depth, int cull, int large_pixels, int queue_capacity, float* depth,
                                   int* index, void* workspace, size_t workspace_bytes, void* stream) {
    MVS_CHECK_ARG(vertices && faces && proj && depth && workspace);
    MVS_CHECK_ARG(M > 0 && F > 0 && V > 0 && H > 0 && W > 0);
    MVS_CHECK_ARG(min_depth >= 0.f && __builtin_isfinite(min_depth));
    MVS_CHECK_ARG(cull >= -1 && cull <= 1 && large_pixels >= 0 && queue_capacity >= 0);
    if (!geo_pixels_ok(V, H, W, RS_MAX_AXIS)) return MVS_E_SHAPE;
    const long long pixels = (long long)V * H * W;
    const RsLayout L = rs_layout(pixels, queue_capacity);
    if (workspace_bytes < L.total) return MVS_E_WORKSPACE;
    hipStream_t st = mvs_stream(stream);
    char* ws = static_cast<char*>(workspace);
    unsigned long long* counter = reinterpret_cast<unsigned long long*>(ws + L.counter);
    unsigned long long* keys = reinterpret_cast<unsigned long long*>(ws + L.keys);
    unsigned long long* queue = reinterpret_cast<unsigned long long*>(ws + L.queue);

    hipError_t e = hipMemsetAsync(counter, 0, RS_HEAD_BYTES, st);
    if (e != hipSuccess) return (int)e;
    e = hipMemsetAsync(keys, 0xff, (size_t)pixels * sizeof(unsigned long long), st);
    if (e != hipSuccess) return (int)e;
    const GeoViewGrid g = geo_view_grid(F, V, RS_THREADS, RS_BLOCKS);
    hipLaunchKernelGGL(rs_small_kernel, dim3(g.blocks, g.chunks), dim3(RS_THREADS), 0, st, vertices, M, faces, F, order, proj, V,
                       g.per, H, W, min_depth, cull, (long long)large_pixels, queue_capacity, keys, counter, queue);
    if (queue_capacity > 0)
        hipLaunchKernelGGL(rs_large_kernel, dim3(std::min(RS_LARGE_BLOCKS, queue_capacity)), dim3(RS_THREADS), 0, st, vertices, M, faces,
                           F, proj, V, H, W, min_depth, cull, queue_capacity, keys, counter, queue);
    hipLaunchKernelGGL(geo_resolve_kernel<RS_THREADS>, dim3(mvs_cdiv(pixels, RS_THREADS)), dim3(RS_THREADS), 0, st, keys, pixels, depth, index);
    MVS_LAUNCH_RET();
}

extern "C" int mvs_raster_interpolate_f32(const float* vertices, int M, const int* faces, int F, const float* proj, int V, int H,
                                          int W, float min_depth, const int* index, const float* attr, int C, float* out,
                                          void* stream) {
    MVS_CHECK_ARG(vertices && faces && proj && index && attr && out);
    MVS_CHECK_ARG(M > 0 && F > 0 && V > 0 && H > 0 && W > 0);
    MVS_CHECK_ARG(min_depth >= 0.f && __builtin_isfinite(min_depth));
    MVS_CHECK_ARG(C >= 1 && C <= RS_MAX_CHANNELS);
    if (!geo_pixels_ok(V, H, W, RS_MAX_AXIS)) return MVS_E_SHAPE;
    const long long pixels = (long long)V * H * W;
    hipLaunchKernelGGL(rs_interpolate_kernel, dim3(mvs_cdiv(pixels, RS_THREADS)), dim3(RS_THREADS), 0, mvs_stream(stream), vertices,
                       M, faces, F, proj, pixels, H, W, min_depth, index, attr, C, out);
    MVS_LAUNCH_RET();
}
