// Rendering of a point cloud into per-view depth maps (mvs_render_points_f32): every point is projected into every view and
// a z-buffer keeps, per pixel, the nearest point.  The semantics are normative in mvsnet_amd/render.py;
// tests/render_reference.py restates them in numpy.
//
//   clear     the 8-byte keys of all V*H*W pixels are set to all ones (empty);
//   splat     one lane per point, taken in `order`; the view loop runs inside the lane, so a point is read once.  Per view
//             the float32 projection (u, v, w) with P_v's twelve floats in scalar registers, the pixel
//             (floor(u/w + 1/2), floor(v/w + 1/2)) by an IEEE division, the (2 splat + 1)^2 covered pixels culled in float
//             against the image, and per surviving pixel key = bits(w) << 32 | point index: one plain load of the pixel's
//             current key, and only when the lane's key is smaller one 64-bit unsigned atomic min at agent scope.  Keys
//             only decrease, so a stale load can only cost an atomic, never an answer.  w is positive and finite, so its
//             bits order as unsigned integers: smallest depth, exact ties to the smallest index, whatever the order.
//             A lane works on RD_VIEWS views at once, so that it keeps that many loads in flight;
//   resolve   keys -> depth (0 where empty) and index (-1 where empty);
//   filter    optional hidden-point removal: resolve writes the raw map into the workspace, and a second kernel reads a
//             32 x 8 tile of it with a halo of k pixels into LDS, counts per pixel the window pixels in front of it
//             (raw[q] > 0 and raw[q] < z * ratio) and writes depth / index; the raw map is only read, so this is order-free.
#include "geom_common.h"

namespace {

constexpr int RD_THREADS = 256;
constexpr int RD_BLOCKS = 2048;                 // fixed grid of the splat kernel: 8 workgroups per CU
constexpr int RD_VIEWS = 4;                     // views a lane works on at once (loads in flight)
constexpr int RD_MAX_SPLAT = 32;
constexpr int RD_MAX_OCCL_RADIUS = 16;
constexpr int RD_MAX_AXIS = 1 << 24;            // H, W: every pixel coordinate is an exact float32
constexpr int RD_TILE_W = 32, RD_TILE_H = 8;    // filter tile = one workgroup

// grid (blocks over the points, chunks of views): lane L of a row of blocks takes points order[L], order[L + lanes], ...
__global__ __launch_bounds__(RD_THREADS) void rd_splat_kernel(const float* __restrict__ xyz, int n, const int* __restrict__ order,
                                                               const float* __restrict__ proj, int V, int views_per_chunk,
                                                               int H, int W, int splat, float min_depth,
                                                               unsigned long long* __restrict__ keys) {
    const int v0 = blockIdx.y * views_per_chunk, v1 = min(V, v0 + views_per_chunk);
    const float wmax = (float)(W - 1), hmax = (float)(H - 1);
    const size_t plane = (size_t)H * W;
    for (long long i = (long long)blockIdx.x * RD_THREADS + threadIdx.x; i < n; i += (long long)gridDim.x * RD_THREADS) {
        const int s = order ? order[i] : (int)i;
        if (s < 0 || s >= n) continue;                        // not a permutation: the point is left out, nothing is read
        const float x = xyz[3 * (size_t)s], y = xyz[3 * (size_t)s + 1], z = xyz[3 * (size_t)s + 2];
        for (int vb = v0; vb < v1; vb += RD_VIEWS) {
            // RD_VIEWS views at a time: their projections first, then per covered offset all their loads before the first
            // atomic, so a lane keeps RD_VIEWS gathers in flight instead of one
            float fx[RD_VIEWS], fy[RD_VIEWS];
            unsigned long long key[RD_VIEWS];
            bool ok[RD_VIEWS];
#pragma unroll
            for (int k = 0; k < RD_VIEWS; ++k) {
                const int v = min(vb + k, v1 - 1);                     // wave-uniform: P arrives by scalar loads
                const float* __restrict__ P = proj + 12 * (size_t)v;
                const float w = geo_row(P + 8, x, y, z);
                fx[k] = geo_pixel(geo_row(P, x, y, z), w);
                fy[k] = geo_pixel(geo_row(P + 4, x, y, z), w);
                ok[k] = vb + k < v1 && GEO_USABLE(w, fx[k], fy[k], min_depth);
                key[k] = geo_key(w, s);
            }
            for (int dy = -splat; dy <= splat; ++dy)
                for (int dx = -splat; dx <= splat; ++dx) {
                    size_t at[RD_VIEWS];
                    unsigned long long cur[RD_VIEWS];
#pragma unroll
                    for (int k = 0; k < RD_VIEWS; ++k) {
                        const float px = fx[k] + (float)dx, py = fy[k] + (float)dy;
                        // in float, before any conversion: a huge coordinate is never converted
                        const bool in = ok[k] && GEO_INSIDE(px, py, wmax, hmax);
                        // a culled lane loads key 0 of the buffer instead (a load without a branch) and masks it to 0: no
                        // key is smaller than 0, so no atomic follows
                        at[k] = in ? (size_t)(vb + k) * plane + (size_t)(int)py * W + (int)px : (size_t)0;
                        cur[k] = keys[at[k]] & (in ? ~0ull : 0ull);
                    }
                    // every load has arrived before the first atomic is issued: an atomic stays counted in vmcnt for hundreds
                    // of cycles, and a load's wait placed behind one would wait for it too
                    static_assert(RD_VIEWS == 4, "the barrier below names four values");
                    asm volatile("" : "+v"(cur[0]), "+v"(cur[1]), "+v"(cur[2]), "+v"(cur[3]));
#pragma unroll
                    for (int k = 0; k < RD_VIEWS; ++k)
                        if (key[k] < cur[k]) __hip_atomic_fetch_min(keys + at[k], key[k], __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
                }
        }
    }
}

// One workgroup per 32 x 8 tile of one view; tile (tx + k2) x (ty + k2) of the raw map in LDS, 0 outside the image (a zero
// is never "in front").  Removed pixels get depth 0 and index -1; the others keep the raw depth (index was resolved before).
__global__ __launch_bounds__(RD_THREADS) void rd_filter_kernel(const float* __restrict__ raw, int H, int W, int tiles_x, int tiles_y,
                                                                int k, float ratio, int count, float* __restrict__ depth,
                                                                int* __restrict__ index) {
    extern __shared__ float rd_tile[];
    const int t = blockIdx.x;
    const int v = t / (tiles_x * tiles_y), ty = (t / tiles_x) % tiles_y, tx = t % tiles_x;
    const int x0 = tx * RD_TILE_W, y0 = ty * RD_TILE_H;
    const int tw = RD_TILE_W + 2 * k, th = RD_TILE_H + 2 * k;
    const float* __restrict__ rv = raw + (size_t)v * H * W;
    for (int e = threadIdx.x; e < tw * th; e += RD_THREADS) {
        const int gy = y0 - k + e / tw, gx = x0 - k + e % tw;
        rd_tile[e] = (gy >= 0 && gy < H && gx >= 0 && gx < W) ? rv[(size_t)gy * W + gx] : 0.f;
    }
    __syncthreads();
    const int lx = threadIdx.x % RD_TILE_W, ly = threadIdx.x / RD_TILE_W;
    const int x = x0 + lx, y = y0 + ly;
    if (x >= W || y >= H) return;
    const float z = rd_tile[(ly + k) * tw + lx + k];
    const float limit = z * ratio;
    int c = 0;
    for (int dy = -k; dy <= k; ++dy)
        for (int dx = -k; dx <= k; ++dx) {
            const float q = rd_tile[(ly + k + dy) * tw + lx + k + dx];
            c += ((dx | dy) != 0 && q > 0.f && q < limit) ? 1 : 0;
        }
    const bool removed = z > 0.f && c >= count;
    const size_t p = ((size_t)v * H + y) * W + x;
    depth[p] = removed ? 0.f : z;
    if (index && removed) index[p] = -1;
}

// [keys | raw map of the filter]
struct RdLayout { size_t keys, raw, total; };

RdLayout rd_layout(long long pixels, bool occlusion) {
    GeoCarver c;
    return {c.take((size_t)pixels * sizeof(unsigned long long)), c.take(occlusion ? (size_t)pixels * sizeof(float) : 0), c.off};
}

}  // namespace

extern "C" size_t mvs_render_workspace_bytes(int V, int H, int W, int occlusion) {
    if (V <= 0 || H <= 0 || W <= 0 || !geo_pixels_ok(V, H, W, RD_MAX_AXIS)) return 0;
    return rd_layout((long long)V * H * W, occlusion != 0).total;
}

extern "C" int mvs_render_points_f32(const float* xyz, int n, const int* order, const float* proj, int V, int H, int W, int splat,
                                     float min_depth, int occl_radius, float occl_ratio, int occl_count, float* depth, int* index,
                                     void* workspace, size_t workspace_bytes, void* stream) {
    MVS_CHECK_ARG(xyz && proj && depth && workspace);
    MVS_CHECK_ARG(n > 0 && V > 0 && H > 0 && W > 0);
    MVS_CHECK_ARG(splat >= 0 && splat <= RD_MAX_SPLAT);
    MVS_CHECK_ARG(min_depth >= 0.f && __builtin_isfinite(min_depth));
    MVS_CHECK_ARG(occl_radius >= 0 && occl_radius <= RD_MAX_OCCL_RADIUS);
    const bool occlusion = occl_radius > 0;
    if (occlusion) MVS_CHECK_ARG(occl_ratio > 0.f && occl_ratio < 1.f && occl_count >= 1);
    if (!geo_pixels_ok(V, H, W, RD_MAX_AXIS)) return MVS_E_SHAPE;
    const long long pixels = (long long)V * H * W;
    const RdLayout L = rd_layout(pixels, occlusion);
    if (workspace_bytes < L.total) return MVS_E_WORKSPACE;
    hipStream_t st = mvs_stream(stream);
    char* ws = static_cast<char*>(workspace);
    unsigned long long* keys = reinterpret_cast<unsigned long long*>(ws + L.keys);
    float* raw = reinterpret_cast<float*>(ws + L.raw);

    hipError_t e = hipMemsetAsync(keys, 0xff, (size_t)pixels * sizeof(unsigned long long), st);
    if (e != hipSuccess) return (int)e;
    const GeoViewGrid g = geo_view_grid(n, V, RD_THREADS, RD_BLOCKS);
    hipLaunchKernelGGL(rd_splat_kernel, dim3(g.blocks, g.chunks), dim3(RD_THREADS), 0, st, xyz, n, order, proj, V, g.per, H, W,
                       splat, min_depth, keys);
    hipLaunchKernelGGL(geo_resolve_kernel<RD_THREADS>, dim3(mvs_cdiv(pixels, RD_THREADS)), dim3(RD_THREADS), 0, st, keys, pixels,
                       occlusion ? raw : depth, index);
    if (occlusion) {
        const int tiles_x = mvs_cdiv(W, RD_TILE_W), tiles_y = mvs_cdiv(H, RD_TILE_H);
        const size_t lds = (size_t)(RD_TILE_W + 2 * occl_radius) * (RD_TILE_H + 2 * occl_radius) * sizeof(float);
        hipLaunchKernelGGL(rd_filter_kernel, dim3((unsigned)((long long)V * tiles_x * tiles_y)), dim3(RD_THREADS), lds, st, raw, H, W,
                           tiles_x, tiles_y, occl_radius, occl_ratio, occl_count, depth, index);
    }
    MVS_LAUNCH_RET();
}
