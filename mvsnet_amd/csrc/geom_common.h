// One copy of what the geometry kernels share (fusion, pointcloud, render, view_selection, tsdf, raster, mesh_components):
// the float32 projection and its visibility test, the 64-bit z-buffer key, the depth / probability filter, the block scan
// with the compaction kernels built on it, and the host-side alignment, shape check, launch shape and workspace carver.
// These are the normative arithmetic the numpy restatements under tests/ hold the kernels to: a new geometry kernel takes
// its projection, key and scan from here.  Everything is safe in several translation units: forceinline device functions,
// static inline host functions, and kernels that are templates in an anonymous namespace (instantiated only where used).
#pragma once
#include "common.h"

// Wave-uniform, read-only data through the scalar unit: a load from the constant address space at a uniform address is an
// s_load (a plain global pointer would be loaded per lane: the compiler cannot prove the memory unclobbered).
typedef __attribute__((address_space(4))) const float geo_cfloat;

// ------------------------------------------------------------------------------------------------ projection
// ((P0 x + P1 y) + P2 z) + P3 in float32, every product and sum rounded.  F: const float, or geo_cfloat for a row that is
// read through the constant address space.
template <typename F>
__device__ __forceinline__ float geo_row(F* r, float x, float y, float z) {
#pragma clang fp contract(off)
    return ((r[0] * x + r[1] * y) + r[2] * z) + r[3];
}

// floor(a / b + 1/2): correctly rounded division, then one rounded sum.
__device__ __forceinline__ float geo_pixel(float a, float b) {
#pragma clang fp contract(off)
    return floorf(__fdiv_rn(a, b) + 0.5f);
}

// The visibility test, compared in float32 before any conversion, so a huge coordinate is never converted and a NaN fails:
// GEO_USABLE (depth w above min_depth, w and the pixel (fx, fy) finite), GEO_INSIDE ((px, py) in [0, wmax] x [0, hmax]) and
// GEO_VISIBLE, both of the same pixel.  Macros, not functions: as functions, by value or by reference, the chains compile to
// other code in the callers than they do standing in the kernel (ts_integrate_kernel measured 1.5 .. 3 % slower); the order
// of the terms is each caller's own from before the header, for the same reason.  As they stand, the callers' ISA is unchanged.
#define GEO_USABLE(w, fx, fy, min_depth) \
    ((w) > (min_depth) && __builtin_isfinite(w) && __builtin_isfinite(fx) && __builtin_isfinite(fy))
#define GEO_INSIDE(px, py, wmax, hmax) ((px) >= 0.f && (px) <= (wmax) && (py) >= 0.f && (py) <= (hmax))
#define GEO_VISIBLE(w, fx, fy, min_depth, wmax, hmax) \
    (__builtin_isfinite(w) && (w) > (min_depth) && __builtin_isfinite(fx) && __builtin_isfinite(fy) && (fx) >= 0.f && (fx) <= (wmax) && \
     (fy) >= 0.f && (fy) <= (hmax))

// ------------------------------------------------------------------------------------------------ z-buffer key
// bits(depth) << 32 | id.  A positive finite depth's bits order as unsigned integers, so an unsigned minimum keeps the
// smallest depth and, among exact ties, the smallest id; all ones is the empty pixel.
constexpr unsigned long long GEO_EMPTY = ~0ull;
__device__ __forceinline__ unsigned long long geo_key(float depth, int id) {
    return ((unsigned long long)__float_as_uint(depth) << 32) | (unsigned)id;
}
__device__ __forceinline__ float geo_key_depth(unsigned long long k) { return k == GEO_EMPTY ? 0.f : __uint_as_float((unsigned)(k >> 32)); }
__device__ __forceinline__ int geo_key_index(unsigned long long k) { return k == GEO_EMPTY ? -1 : (int)(unsigned)k; }

// ------------------------------------------------------------------------------------------------ scan and compaction
constexpr int GEO_COMPACT_PER = 4;              // elements per thread of a compaction block

// Exclusive scan of one value per thread over a block of THREADS threads (Hillis-Steele in LDS); returns the thread's prefix.
template <int THREADS>
__device__ int geo_block_exclusive_scan(int v, int* sh, int& total) {
    const int t = threadIdx.x;
    sh[t] = v;
    __syncthreads();
    for (int o = 1; o < THREADS; o <<= 1) {
        const int add = t >= o ? sh[t - o] : 0;
        __syncthreads();
        sh[t] += add;
        __syncthreads();
    }
    total = sh[THREADS - 1];
    const int incl = sh[t];
    __syncthreads();
    return incl - v;
}

// Sum of one int per thread over a workgroup of THREADS threads: a wave sum by shuffles, then THREADS / 64 words of LDS.  The
// total is returned in thread 0 (other threads get a partial sum).  Every thread calls it; `sh` holds THREADS / 64 ints, and
// a second call on the same `sh` needs a __syncthreads() in between.  A kernel that counts into a status word adds thread
// 0's total with ONE atomic per workgroup (a wave, an atomic measured 0.37 -> 0.045 ms on 2 M faces: DESIGN 4.17).
template <int THREADS>
__device__ __forceinline__ int geo_block_sum(int v, int* sh) {
#pragma unroll
    for (int o = 32; o > 0; o >>= 1) v += __shfl_xor(v, o, 64);
    if ((threadIdx.x & 63) == 0) sh[threadIdx.x >> 6] = v;
    __syncthreads();
    int total = 0;
    if (threadIdx.x == 0) {
#pragma unroll
        for (int w = 0; w < THREADS / 64; ++w) total += sh[w];
    }
    return total;
}

// ------------------------------------------------------------------------------------------------ sorted keys
// The first position in the ascending keys[0..n) whose key is >= want: a binary search of at most 32 steps inside 0..n-1, no
// atomics.  Keys of the form int64(owner) << 31 | item sort the items of one owner into a run, bounded by the lower bounds
// of owner << 31 and (owner + 1) << 31.
__device__ __forceinline__ long long geo_lower_bound(const long long* __restrict__ keys, long long n, long long want) {
    long long lo = 0, hi = n;
    while (lo < hi) {
        const long long mid = (lo + hi) >> 1;
        if (keys[mid] < want) lo = mid + 1;
        else hi = mid;
    }
    return lo;
}

namespace {

// One lane per pixel of all views: keys -> depth (0 where empty) and index (-1 where empty).  index may be NULL.
template <int THREADS>
__global__ __launch_bounds__(THREADS) void geo_resolve_kernel(const unsigned long long* __restrict__ keys, long long pixels,
                                                              float* __restrict__ depth, int* __restrict__ index) {
    const long long p = (long long)blockIdx.x * THREADS + threadIdx.x;
    if (p >= pixels) return;
    const unsigned long long k = keys[p];
    depth[p] = geo_key_depth(k);
    if (index) index[p] = geo_key_index(k);
}

// df = D where D > 0, finite and P >= thr, else 0.
template <int THREADS>
__global__ __launch_bounds__(THREADS) void geo_filter_kernel(const float* __restrict__ depth, const float* __restrict__ prob,
                                                             size_t n, float thr, float* __restrict__ df) {
    const size_t i = (size_t)blockIdx.x * THREADS + threadIdx.x;
    if (i >= n) return;
    const float d = depth[i], p = prob[i];
    df[i] = (d > 0.f && __builtin_isfinite(d) && p >= thr) ? d : 0.f;
}

// counts[block] = the number of set keep flags among the block's GEO_COMPACT_PER * THREADS elements.
template <int THREADS>
__global__ __launch_bounds__(THREADS) void geo_compact_count_kernel(const uint8_t* __restrict__ keep, size_t n,
                                                                    int* __restrict__ counts) {
    __shared__ int sh[THREADS];
    const size_t e0 = ((size_t)blockIdx.x * THREADS + threadIdx.x) * GEO_COMPACT_PER;
    int c = 0;
    for (int i = 0; i < GEO_COMPACT_PER; ++i) c += (e0 + i < n && keep[e0 + i]) ? 1 : 0;
    int total;
    geo_block_exclusive_scan<THREADS>(c, sh, total);
    if (threadIdx.x == 0) counts[blockIdx.x] = total;
}

// One workgroup per array (grid.y arrays, `stride` ints apart): exclusive scan of the nb block totals counts -> offs, which
// may be the same array; the grand total -> total[array] unless total is NULL.
template <int THREADS>
__global__ __launch_bounds__(THREADS) void geo_scan_top_kernel(const int* counts, int nb, int stride, int* offs, int* total) {
    __shared__ int sh[THREADS];
    const int* in = counts + blockIdx.y * stride;
    int* out = offs + blockIdx.y * stride;
    int carry = 0;
    for (int b0 = 0; b0 < nb; b0 += THREADS) {
        const int b = b0 + threadIdx.x;
        const int c = b < nb ? in[b] : 0;
        int sum;
        const int ex = geo_block_exclusive_scan<THREADS>(c, sh, sum);
        if (b < nb) out[b] = carry + ex;
        carry += sum;
    }
    if (total && threadIdx.x == 0) total[blockIdx.y] = carry;
}

}  // namespace

// ------------------------------------------------------------------------------------------------ host side
static inline size_t geo_align256(size_t b) { return (b + 255) & ~(size_t)255; }

// V maps of H x W: every pixel coordinate below max_axis, every pixel index an int.
static inline bool geo_pixels_ok(int V, int H, int W, int max_axis) {
    return H <= max_axis && W <= max_axis && (long long)V * H * W <= 0x7fffffffLL;
}

// A fixed grid of at most max_blocks workgroups striding over the items; a small set of items leaves blocks over, which then
// share the views: grid (blocks, chunks), a row of blocks taking `per` views.
struct GeoViewGrid { int blocks, chunks, per; };

static inline GeoViewGrid geo_view_grid(long long items, int V, int threads, int max_blocks) {
    GeoViewGrid g;
    g.blocks = (int)std::min<long long>(max_blocks, mvs_cdiv(items, threads));
    g.per = mvs_cdiv(V, std::min(V, std::max(1, max_blocks / g.blocks)));
    g.chunks = mvs_cdiv(V, g.per);
    return g;
}

// Bump carver of a workspace: take(bytes) returns the offset of the next piece and moves on by the aligned size.
struct GeoCarver {
    size_t off = 0;
    size_t take(size_t bytes) {
        const size_t at = off;
        off += geo_align256(bytes);
        return at;
    }
};
