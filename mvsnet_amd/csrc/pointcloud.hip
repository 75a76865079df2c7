// Point-cloud evaluation (accuracy, completeness, F-score of a predicted cloud against a ground-truth cloud): exact,
// distance-capped nearest neighbours between two clouds, per-cloud voxel downsampling and the distance statistics.  The
// semantics are normative in mvsnet_amd/evaluate.py; tests/pointcloud_reference.py restates them in float64.
//
// Nearest neighbour of every query point in a target cloud (mvs_nn_f32), all on the caller's stream, nothing allocated:
//   count     per point of the target and of the queries its cell c = clamp(floor((x - o) / cell)) of the target's uniform
//             grid (gx, gy, gz) and its rank inside the cell (an integer atomicAdd on the cell's counter);
//   scan      exclusive scan of both per-cell counters (multi-block: chunk totals, one workgroup over the totals, apply);
//   scatter   cell-ordered float4 copies (x, y, z, input index as bits) of the target and of the queries;
//   query     one lane per query in cell order (the lanes of a wave share cells): the query's own cell, then balls of
//             radius cell, 2 cell, 4 cell, ... (starting at the distance to the grid's box for a query outside it) up to
//             max_dist.  A ball is one contiguous range of the sorted target per (y, z) row, the x-range clipped to the ball
//             and every row pruned by the best distance so far; the search ends after the first ball that holds the best
//             point.  Exact ties of the float32 d^2 go to the smallest input index, so the result does not depend on the
//             order in which candidates are visited.  Written back in input order.
//             (A first form walked Chebyshev rings of cells; a query far from the target then re-read the two end cells of
//             every row once per ring, ~10x the start-array reads of the balls: DESIGN 4.9.)
// The bounds are deflated by a small multiple of the coordinate scale (PC_EPS_REL) so that float32 rounding of cell
// coordinates can never exclude the true nearest point; that costs at most a few extra cells, never an answer.
//
// Statistics (mvs_dist_stats_f32): fixed grid of blocks, per-thread sums in a fixed order, fixed trees inside a block, float64
// partial sums and integer counts per block, one workgroup reduces them in block order: bitwise reproducible, no float atomics.
//
// Voxel downsampling (mvs_voxel_keys_f32, then a stable key sort by the caller, then mvs_voxel_select_f32): float64 keys,
// "first of run" marks on the sorted keys set the keep flag of the run's first point in input order, ordered compaction.
//
// ICP registration (mvsnet_amd/register.py is normative): mvs_nn_target_build_f32 is count / scan / scatter for a target that
// does not move, once; mvs_icp_step_f32 is one pass per iteration, one lane per source point: transform in float64, the
// query above, the eighteen float64 moments of the correspondences, reduced as the statistics are.  Nothing per point
// goes to memory unless the caller asks for dist / index.
#include "geom_common.h"

namespace {

constexpr int PC_THREADS = 256;
constexpr int PC_SCAN_PER = 16;                           // elements per thread of a scan chunk
constexpr int PC_SCAN_CHUNK = PC_THREADS * PC_SCAN_PER;   // 4096
constexpr long long PC_MAX_CELLS = 1LL << 24;
constexpr int PC_MAX_THRESHOLDS = 16;
constexpr int PC_STATS_BLOCKS = 1024;
constexpr int PC_COMPACT_CHUNK = PC_THREADS * GEO_COMPACT_PER;   // 1024 points per compaction block
constexpr float PC_EPS_REL = 8e-6f;                       // bound deflation, relative to the coordinate scale
constexpr float PC_SHRINK = 1.0f - 1e-5f;                 // bound deflation of squared distances (float32 d^2 rounding)

__device__ __forceinline__ int pc_cell_axis(float x, float o, float cell, int g) {
    float f = floorf((x - o) / cell);
    f = fminf(fmaxf(f, 0.f), (float)(g - 1));
    return (int)f;
}

__global__ __launch_bounds__(PC_THREADS) void pc_cell_count_kernel(const float* __restrict__ pts, int n, float ox, float oy,
                                                                    float oz, float cell, int gx, int gy, int gz,
                                                                    int* __restrict__ cellid, int* __restrict__ rank,
                                                                    int* __restrict__ count) {
    const int i = blockIdx.x * PC_THREADS + threadIdx.x;
    if (i >= n) return;
    const float x = pts[3 * (size_t)i], y = pts[3 * (size_t)i + 1], z = pts[3 * (size_t)i + 2];
    const int c = (pc_cell_axis(z, oz, cell, gz) * gy + pc_cell_axis(y, oy, cell, gy)) * gx + pc_cell_axis(x, ox, cell, gx);
    cellid[i] = c;
    rank[i] = atomicAdd(&count[c], 1);
}

__global__ __launch_bounds__(PC_THREADS) void pc_scatter_kernel(const float* __restrict__ pts, int n, const int* __restrict__ cellid,
                                                                 const int* __restrict__ rank, const int* __restrict__ start,
                                                                 float4* __restrict__ sorted) {
    const int i = blockIdx.x * PC_THREADS + threadIdx.x;
    if (i >= n) return;
    const float x = pts[3 * (size_t)i], y = pts[3 * (size_t)i + 1], z = pts[3 * (size_t)i + 2];
    sorted[start[cellid[i]] + rank[i]] = make_float4(x, y, z, __int_as_float(i));
}

// ------------------------------------------------------------------ multi-block exclusive scan of int arrays, in place
// grid (chunks, arrays): array y at data + y * stride (m entries), its chunk totals at bsum + y * bstride.

__global__ __launch_bounds__(PC_THREADS) void pc_scan_reduce_kernel(const int* __restrict__ data, int m, size_t stride,
                                                                     int* __restrict__ bsum, int bstride) {
    __shared__ int sh[PC_THREADS];
    const int* d = data + blockIdx.y * stride;
    const long long e0 = (long long)blockIdx.x * PC_SCAN_CHUNK + (long long)threadIdx.x * PC_SCAN_PER;
    int s = 0;
    for (int k = 0; k < PC_SCAN_PER; ++k) s += e0 + k < m ? d[e0 + k] : 0;
    int total;
    geo_block_exclusive_scan<PC_THREADS>(s, sh, total);
    if (threadIdx.x == 0) bsum[blockIdx.y * bstride + blockIdx.x] = total;
}

__global__ __launch_bounds__(PC_THREADS) void pc_scan_apply_kernel(int* __restrict__ data, int m, size_t stride,
                                                                    const int* __restrict__ bsum, int bstride) {
    __shared__ int sh[PC_THREADS];
    int* d = data + blockIdx.y * stride;
    const long long e0 = (long long)blockIdx.x * PC_SCAN_CHUNK + (long long)threadIdx.x * PC_SCAN_PER;
    int v[PC_SCAN_PER];
    int s = 0;
#pragma unroll
    for (int k = 0; k < PC_SCAN_PER; ++k) {
        v[k] = e0 + k < m ? d[e0 + k] : 0;
        s += v[k];
    }
    int total;
    int o = bsum[blockIdx.y * bstride + blockIdx.x] + geo_block_exclusive_scan<PC_THREADS>(s, sh, total);
#pragma unroll
    for (int k = 0; k < PC_SCAN_PER; ++k) {
        if (e0 + k < m) d[e0 + k] = o;
        o += v[k];
    }
}

// ------------------------------------------------------------------ nearest-neighbour query

__device__ __forceinline__ float pc_slab_gap(float q, float lo, float hi, float eps) {
    const float g = fmaxf(fmaxf(lo - q, q - hi), 0.f);
    return fmaxf(g - eps, 0.f);
}

// Cells [a, b] of one axis that can hold a point within rho of coordinate q (one cell of slack on each side for rounding).
__device__ __forceinline__ void pc_axis_range(float q, float rho, float o, float cell, int g, int& a, int& b) {
    const float fa = floorf((q - rho - o) / cell) - 1.f, fb = floorf((q + rho - o) / cell) + 1.f;
    a = (int)fminf(fmaxf(fa, 0.f), (float)(g - 1));
    b = (int)fminf(fmaxf(fb, 0.f), (float)(g - 1));
    if (fb < 0.f) b = -1;                                 // the whole range is below the grid
    if (fa > (float)(g - 1)) a = g;                       // ... or above it
}

__device__ __forceinline__ void pc_consider(float4 p, float qx, float qy, float qz, float& best2, int& bi) {
    const float dx = qx - p.x, dy = qy - p.y, dz = qz - p.z;
    const float d2 = dx * dx + dy * dy + dz * dz;
    const int j = __float_as_int(p.w);
    if (d2 < best2 || (d2 == best2 && j < bi)) {
        best2 = d2;
        bi = j;
    }
}

// Candidates k0 .. k1-1, four loads in flight per lane (the loop is bound by the latency of its gathers).
__device__ __forceinline__ void pc_scan_range(const float4* __restrict__ ts, int k0, int k1, float qx, float qy, float qz,
                                              float& best2, int& bi, int& seen) {
    seen += k1 - k0;
    int k = k0;
    for (; k + 4 <= k1; k += 4) {
        const float4 p0 = ts[k], p1 = ts[k + 1], p2 = ts[k + 2], p3 = ts[k + 3];
        pc_consider(p0, qx, qy, qz, best2, bi);
        pc_consider(p1, qx, qy, qz, best2, bi);
        pc_consider(p2, qx, qy, qz, best2, bi);
        pc_consider(p3, qx, qy, qz, best2, bi);
    }
    for (; k < k1; ++k) pc_consider(ts[k], qx, qy, qz, best2, bi);
}

// Every target point within sqrt(R2) of q (cells whose deflated gap is inside the ball, one range per (y, z) row), pruned
// by the best distance so far.  The limit is inflated by 1 / PC_SHRINK so that device ties with `best` are still visited.
__device__ __forceinline__ void pc_visit_ball(const float4* __restrict__ ts, const int* __restrict__ tstart, float4 q, float R2,
                                              float ox, float oy, float oz, float cell, int gx, int gy, int gz, float eps,
                                              float& best2, int& bi, int& seen) {
    int za, zb;
    pc_axis_range(q.z, sqrtf(fminf(R2, best2 / PC_SHRINK)), oz, cell, gz, za, zb);
    for (int z = za; z <= zb; ++z) {
        const float gzp = pc_slab_gap(q.z, oz + (float)z * cell, oz + (float)(z + 1) * cell, eps);
        const float rz2 = fminf(R2, best2 / PC_SHRINK) - gzp * gzp;
        if (rz2 < 0.f) continue;
        int ya, yb;
        pc_axis_range(q.y, sqrtf(rz2), oy, cell, gy, ya, yb);
        for (int y = ya; y <= yb; ++y) {
            const float gyp = pc_slab_gap(q.y, oy + (float)y * cell, oy + (float)(y + 1) * cell, eps);
            const float rx2 = fminf(R2, best2 / PC_SHRINK) - gzp * gzp - gyp * gyp;
            if (rx2 < 0.f) continue;
            int xa, xb;
            pc_axis_range(q.x, sqrtf(rx2), ox, cell, gx, xa, xb);
            if (xa > xb) continue;
            const int row = (z * gy + y) * gx;
            pc_scan_range(ts, tstart[row + xa], tstart[row + xb + 1], q.x, q.y, q.z, best2, bi, seen);
        }
    }
}

// The query loop: the nearest target point of q within max_dist -> best2 (float32 d^2, +inf when the grid's box is beyond
// max_dist), bi (its input index), seen (candidates compared).  The caller applies the cap best2 <= max_dist^2.
__device__ __forceinline__ void pc_query(const float4* __restrict__ ts, const int* __restrict__ tstart, float4 q, float ox,
                                         float oy, float oz, float cell, int gx, int gy, int gz, float max_dist, float& best2,
                                         int& bi, int& seen) {
    const int cx = pc_cell_axis(q.x, ox, cell, gx), cy = pc_cell_axis(q.y, oy, cell, gy), cz = pc_cell_axis(q.z, oz, cell, gz);
    const int gmax = max(gx, max(gy, gz));
    const float scale = fmaxf(fabsf(q.x), fmaxf(fabsf(q.y), fabsf(q.z))) + fmaxf(fabsf(ox), fmaxf(fabsf(oy), fabsf(oz))) +
                        (float)gmax * cell;
    const float eps = PC_EPS_REL * scale;
    const float hx = ox + (float)gx * cell, hy = oy + (float)gy * cell, hz = oz + (float)gz * cell;
    // distance outside the grid's box per axis (every target point lies inside it)
    const float outx = pc_slab_gap(q.x, ox, hx, eps), outy = pc_slab_gap(q.y, oy, hy, eps), outz = pc_slab_gap(q.z, oz, hz, eps);
    const float md2 = max_dist * max_dist;
    best2 = __builtin_inff();
    bi = 0x7fffffff;
    seen = 0;
    const float box2 = outx * outx + outy * outy + outz * outz;
    if (box2 * PC_SHRINK <= md2) {
        // the query's own cell first: a good first `best` prunes the rows of the first ball
        const int own = (cz * gy + cy) * gx + cx;
        pc_scan_range(ts, tstart[own], tstart[own + 1], q.x, q.y, q.z, best2, bi, seen);
        for (float R = fmaxf(cell, sqrtf(box2) + cell);; R *= 2.f) {
            const bool last = R >= max_dist;
            const float Rs = last ? max_dist * (1.f + 1e-5f) + eps : R;
            pc_visit_ball(ts, tstart, q, Rs * Rs, ox, oy, oz, cell, gx, gy, gz, eps, best2, bi, seen);
            const float inner = fmaxf(R - eps, 0.f);
            if (last || best2 < inner * inner * PC_SHRINK) break;   // the nearest point lies inside the searched ball
        }
    }
}

__global__ __launch_bounds__(PC_THREADS) void pc_nn_query_kernel(
        const float4* __restrict__ qs, int nq, const float4* __restrict__ ts, const int* __restrict__ tstart, float ox, float oy,
        float oz, float cell, int gx, int gy, int gz, float max_dist, float* __restrict__ dist, int* __restrict__ index,
        int* __restrict__ visited) {
    const int i = blockIdx.x * PC_THREADS + threadIdx.x;
    if (i >= nq) return;
    const float4 q = qs[i];
    const int qi = __float_as_int(q.w);
    float best2;
    int bi, seen;
    pc_query(ts, tstart, q, ox, oy, oz, cell, gx, gy, gz, max_dist, best2, bi, seen);
    const bool in = best2 <= max_dist * max_dist;
    dist[qi] = in ? sqrtf(best2) : __builtin_inff();
    index[qi] = in ? bi : -1;
    if (visited) visited[qi] = seen;
}

// ------------------------------------------------------------------ distance statistics

struct PcThresholds { float t[PC_MAX_THRESHOLDS]; };

template <typename T>
__device__ T pc_block_sum(T v, T* sh) {
#pragma unroll
    for (int o = 32; o > 0; o >>= 1) v += __shfl_xor(v, o, 64);
    const int w = threadIdx.x >> 6;
    __syncthreads();
    if ((threadIdx.x & 63) == 0) sh[w] = v;
    __syncthreads();
    T s = sh[0];
    for (int k = 1; k < PC_THREADS / 64; ++k) s += sh[k];
    return s;
}

// partials per block: psum[b] (float64 inlier sum), pcnt[b * (1 + PC_MAX_THRESHOLDS) + 0] inlier count, + 1 + t below tau_t
__global__ __launch_bounds__(PC_THREADS) void pc_stats_partial_kernel(const float* __restrict__ dist, int n, float max_dist,
                                                                       PcThresholds thr, int n_thr, double* __restrict__ psum,
                                                                       int* __restrict__ pcnt) {
    __shared__ double shd[PC_THREADS / 64];
    __shared__ int shi[PC_THREADS / 64];
    double s = 0.0;
    int c = 0;
    int ct[PC_MAX_THRESHOLDS];
#pragma unroll
    for (int t = 0; t < PC_MAX_THRESHOLDS; ++t) ct[t] = 0;
    for (long long i = (long long)blockIdx.x * PC_THREADS + threadIdx.x; i < n; i += (long long)gridDim.x * PC_THREADS) {
        const float d = dist[i];
        if (d < max_dist) { s += (double)d; ++c; }
#pragma unroll
        for (int t = 0; t < PC_MAX_THRESHOLDS; ++t) ct[t] += (t < n_thr && d < thr.t[t]) ? 1 : 0;
    }
    const double bs = pc_block_sum(s, shd);
    const int bc = pc_block_sum(c, shi);
    int* out = pcnt + (size_t)blockIdx.x * (1 + PC_MAX_THRESHOLDS);
    if (threadIdx.x == 0) { psum[blockIdx.x] = bs; out[0] = bc; }
#pragma unroll
    for (int t = 0; t < PC_MAX_THRESHOLDS; ++t) {
        const int v = pc_block_sum(ct[t], shi);
        if (threadIdx.x == 0) out[1 + t] = v;
    }
}

// One workgroup: the nb partials in block order -> out = inlier sum, inlier count, count below tau_t (as float64).
__global__ __launch_bounds__(PC_THREADS) void pc_stats_final_kernel(const double* __restrict__ psum, const int* __restrict__ pcnt,
                                                                     int nb, int n_thr, double* __restrict__ out) {
    __shared__ double shd[PC_THREADS / 64];
    __shared__ long long shl[PC_THREADS / 64];
    double s = 0.0;
    for (int b = threadIdx.x; b < nb; b += PC_THREADS) s += psum[b];
    const double total = pc_block_sum(s, shd);
    if (threadIdx.x == 0) out[0] = total;
    for (int k = 0; k <= n_thr; ++k) {
        long long c = 0;
        for (int b = threadIdx.x; b < nb; b += PC_THREADS) c += pcnt[(size_t)b * (1 + PC_MAX_THRESHOLDS) + k];
        const long long v = pc_block_sum(c, shl);
        if (threadIdx.x == 0) out[1 + k] = (double)v;
    }
}

// ------------------------------------------------------------------ one ICP registration step (mvs_icp_step_f32)
// moments = [count, sum |r|^2, sum a (3), sum b (3), sum a b^T (9, row-major), sum |a|^2] over the source points p that have
// a target point q within max_corr_dist of fl32(T p): a = p - cp, b = q - cq, r = T p - q in float64 (T p unrounded).
// mvsnet_amd/register.py is normative.

constexpr int PC_ICP_MOMENTS = 18;
constexpr int PC_ICP_BLOCKS = 2048;

struct PcIcpParams { double T[12], cp[3], cq[3]; };

// T[i,0] x + T[i,1] y + T[i,2] z + T[i,3], left to right, every product and sum rounded (no fused multiply-add), as
// evaluate._transform evaluates it.
__device__ __forceinline__ double pc_affine_row(const double* __restrict__ r, double x, double y, double z) {
#pragma clang fp contract(off)
    return ((x * r[0] + y * r[1]) + z * r[2]) + r[3];
}

// One lane per source point in processing order (order[i], or i): blocks sweep the cloud in strides of the grid, so lane L of
// the grid sums points L, L + lanes, ... in that order.  tpos: the target's per-point cell and rank, which with tstart give
// the position of target point j in the cell-ordered copy.  partial: PC_ICP_MOMENTS doubles per block.
__global__ __launch_bounds__(PC_THREADS) void pc_icp_step_kernel(
        const float* __restrict__ src, int n, const int* __restrict__ order, PcIcpParams P, const float4* __restrict__ ts,
        const int* __restrict__ tstart, const int* __restrict__ tcell, const int* __restrict__ trank, float ox, float oy, float oz,
        float cell, int gx, int gy, int gz, float max_dist, double* __restrict__ partial, float* __restrict__ dist,
        int* __restrict__ index) {
    __shared__ double shd[PC_THREADS / 64];
    double m[PC_ICP_MOMENTS];
#pragma unroll
    for (int k = 0; k < PC_ICP_MOMENTS; ++k) m[k] = 0.0;
    for (long long i = (long long)blockIdx.x * PC_THREADS + threadIdx.x; i < n; i += (long long)gridDim.x * PC_THREADS) {
        const int s = order ? order[i] : (int)i;
        if (s < 0 || s >= n) continue;                       // not a permutation: the point is left out, nothing is read
        const double px = (double)src[3 * (size_t)s], py = (double)src[3 * (size_t)s + 1], pz = (double)src[3 * (size_t)s + 2];
        const double tx = pc_affine_row(P.T, px, py, pz), ty = pc_affine_row(P.T + 4, px, py, pz),
                     tz = pc_affine_row(P.T + 8, px, py, pz);
        const float4 q = make_float4((float)tx, (float)ty, (float)tz, 0.f);
        float best2;
        int bi, seen;
        pc_query(ts, tstart, q, ox, oy, oz, cell, gx, gy, gz, max_dist, best2, bi, seen);
        const bool in = best2 <= max_dist * max_dist;
        if (dist) dist[s] = in ? sqrtf(best2) : __builtin_inff();
        if (index) index[s] = in ? bi : -1;
        if (!in) continue;
        const float4 t = ts[tstart[tcell[bi]] + trank[bi]];
        const double a0 = px - P.cp[0], a1 = py - P.cp[1], a2 = pz - P.cp[2];
        const double b0 = (double)t.x - P.cq[0], b1 = (double)t.y - P.cq[1], b2 = (double)t.z - P.cq[2];
        const double r0 = tx - (double)t.x, r1 = ty - (double)t.y, r2 = tz - (double)t.z;
        m[0] += 1.0;
        m[1] += (r0 * r0 + r1 * r1) + r2 * r2;
        m[2] += a0;  m[3] += a1;  m[4] += a2;
        m[5] += b0;  m[6] += b1;  m[7] += b2;
        m[8] += a0 * b0;   m[9] += a0 * b1;   m[10] += a0 * b2;
        m[11] += a1 * b0;  m[12] += a1 * b1;  m[13] += a1 * b2;
        m[14] += a2 * b0;  m[15] += a2 * b1;  m[16] += a2 * b2;
        m[17] += (a0 * a0 + a1 * a1) + a2 * a2;
    }
#pragma unroll
    for (int k = 0; k < PC_ICP_MOMENTS; ++k) {
        const double v = pc_block_sum(m[k], shd);
        if (threadIdx.x == 0) partial[(size_t)blockIdx.x * PC_ICP_MOMENTS + k] = v;
    }
}

// One workgroup: the nb partials in block order.
__global__ __launch_bounds__(PC_THREADS) void pc_icp_final_kernel(const double* __restrict__ partial, int nb,
                                                                   double* __restrict__ out) {
    __shared__ double shd[PC_THREADS / 64];
    for (int k = 0; k < PC_ICP_MOMENTS; ++k) {
        double s = 0.0;
        for (int b = threadIdx.x; b < nb; b += PC_THREADS) s += partial[(size_t)b * PC_ICP_MOMENTS + k];
        const double total = pc_block_sum(s, shd);
        if (threadIdx.x == 0) out[k] = total;
    }
}

// ------------------------------------------------------------------ voxel downsampling

__global__ __launch_bounds__(PC_THREADS) void pc_voxel_keys_kernel(const float* __restrict__ xyz, int n, double mx, double my,
                                                                    double mz, double cell, long long* __restrict__ keys) {
    const int i = blockIdx.x * PC_THREADS + threadIdx.x;
    if (i >= n) return;
    const double lim = (double)((1 << 21) - 1);
    const double kx = fmin(fmax(floor(((double)xyz[3 * (size_t)i] - mx) / cell), 0.0), lim);
    const double ky = fmin(fmax(floor(((double)xyz[3 * (size_t)i + 1] - my) / cell), 0.0), lim);
    const double kz = fmin(fmax(floor(((double)xyz[3 * (size_t)i + 2] - mz) / cell), 0.0), lim);
    keys[i] = (long long)kx | ((long long)ky << 21) | ((long long)kz << 42);
}

// keep[order[i]] = 1 when sorted position i starts a run of equal keys (the stable sort puts the run's first point in input
// order first), else 0.  Every point is written once.
__global__ __launch_bounds__(PC_THREADS) void pc_voxel_mark_kernel(const long long* __restrict__ keys, const long long* __restrict__ order,
                                                                    int n, uint8_t* __restrict__ keep) {
    const int i = blockIdx.x * PC_THREADS + threadIdx.x;
    if (i >= n) return;
    const long long o = order[i];
    if (o < 0 || o >= n) return;
    keep[o] = (i == 0 || keys[i] != keys[i - 1]) ? 1 : 0;
}

__global__ __launch_bounds__(PC_THREADS) void pc_compact_write_kernel(const uint8_t* __restrict__ keep, const float* __restrict__ xyz,
                                                                       int n, const int* __restrict__ offs, int nb,
                                                                       float* __restrict__ out, int* __restrict__ count) {
    __shared__ int sh[PC_THREADS];
    const long long e0 = (long long)blockIdx.x * PC_COMPACT_CHUNK + GEO_COMPACT_PER * threadIdx.x;
    int c = 0;
    for (int k = 0; k < GEO_COMPACT_PER; ++k) c += (e0 + k < n && keep[e0 + k]) ? 1 : 0;
    int total;
    int o = offs[blockIdx.x] + geo_block_exclusive_scan<PC_THREADS>(c, sh, total);
    if (blockIdx.x == 0 && threadIdx.x == 0) *count = offs[nb];
    for (int k = 0; k < GEO_COMPACT_PER; ++k) {
        const long long e = e0 + k;
        if (e >= n || !keep[e]) continue;
        out[3 * (size_t)o] = xyz[3 * e];
        out[3 * (size_t)o + 1] = xyz[3 * e + 1];
        out[3 * (size_t)o + 2] = xyz[3 * e + 2];
        ++o;
    }
}

// ------------------------------------------------------------------ host side

int pc_scan_chunks(long long m) { return (int)((m + PC_SCAN_CHUNK - 1) / PC_SCAN_CHUNK); }

// Exclusive scan of `arrays` int arrays of m entries each, `stride` apart, in place; bsum: arrays * (chunks + 1) ints.
hipError_t pc_scan(int* data, long long m, size_t stride, int arrays, int* bsum, hipStream_t st) {
    const int nb = pc_scan_chunks(m);
    const int bstride = nb + 1;
    hipLaunchKernelGGL(pc_scan_reduce_kernel, dim3(nb, arrays), dim3(PC_THREADS), 0, st, data, (int)m, stride, bsum, bstride);
    hipLaunchKernelGGL(geo_scan_top_kernel<PC_THREADS>, dim3(1, arrays), dim3(PC_THREADS), 0, st, bsum, nb, bstride, bsum, (int*)nullptr);
    hipLaunchKernelGGL(pc_scan_apply_kernel, dim3(nb, arrays), dim3(PC_THREADS), 0, st, data, (int)m, stride, bsum, bstride);
    return hipGetLastError();
}

struct NnLayout {
    size_t starts, bsum, tcell, trank, qcell, qrank, tsorted, qsorted, total;
    size_t stride;           // ints between the target's and the queries' per-cell arrays
};

NnLayout nn_layout(int nq, int nt, long long ncell) {
    NnLayout L{};
    const long long m = ncell + 1;
    L.stride = geo_align256((size_t)m * sizeof(int)) / sizeof(int);
    GeoCarver c;
    L.starts = c.take(2 * L.stride * sizeof(int));
    L.bsum = c.take(2 * ((size_t)pc_scan_chunks(m) + 1) * sizeof(int));
    L.tcell = c.take((size_t)nt * sizeof(int));
    L.trank = c.take((size_t)nt * sizeof(int));
    L.qcell = c.take((size_t)nq * sizeof(int));
    L.qrank = c.take((size_t)nq * sizeof(int));
    L.tsorted = c.take((size_t)nt * sizeof(float4));
    L.qsorted = c.take((size_t)nq * sizeof(float4));
    L.total = c.off;
    return L;
}

bool nn_grid_ok(int gx, int gy, int gz) {
    return gx > 0 && gy > 0 && gz > 0 && (long long)gx * gy * gz <= PC_MAX_CELLS;
}

int stats_blocks(int n) { return (int)std::min<long long>(PC_STATS_BLOCKS, ((long long)n + PC_THREADS * 8 - 1) / (PC_THREADS * 8)); }

size_t stats_bytes(int n) {
    const size_t nb = (size_t)stats_blocks(n);
    return geo_align256(nb * sizeof(double)) + geo_align256(nb * (1 + PC_MAX_THRESHOLDS) * sizeof(int));
}

int compact_blocks(int n) { return (int)(((long long)n + PC_COMPACT_CHUNK - 1) / PC_COMPACT_CHUNK); }

size_t voxel_select_bytes(int n) {
    const int nb = compact_blocks(n);
    return geo_align256((size_t)n) + geo_align256(((size_t)nb + 1) * sizeof(int)) + geo_align256(((size_t)pc_scan_chunks(nb + 1) + 1) * sizeof(int));
}

// The target alone: per-cell starts, scan scratch, per-point cell and rank (kept: they locate a point in the sorted copy), sorted copy.
struct TargetLayout { size_t starts, bsum, tcell, trank, tsorted, total; };

TargetLayout target_layout(int nt, long long ncell) {
    TargetLayout L{};
    const long long m = ncell + 1;
    GeoCarver c;
    L.starts = c.take((size_t)m * sizeof(int));
    L.bsum = c.take(((size_t)pc_scan_chunks(m) + 1) * sizeof(int));
    L.tcell = c.take((size_t)nt * sizeof(int));
    L.trank = c.take((size_t)nt * sizeof(int));
    L.tsorted = c.take((size_t)nt * sizeof(float4));
    L.total = c.off;
    return L;
}

int icp_blocks(int n) { return (int)std::min<long long>(PC_ICP_BLOCKS, ((long long)n + PC_THREADS - 1) / PC_THREADS); }

size_t icp_bytes(int n) { return geo_align256((size_t)icp_blocks(n) * PC_ICP_MOMENTS * sizeof(double)); }

}  // namespace

extern "C" size_t mvs_nn_workspace_bytes(int n_query, int n_target, int gx, int gy, int gz) {
    if (n_query <= 0 || n_target <= 0 || !nn_grid_ok(gx, gy, gz)) return 0;
    return nn_layout(n_query, n_target, (long long)gx * gy * gz).total;
}

extern "C" int mvs_nn_f32(const float* query, int n_query, const float* target, int n_target, float ox, float oy, float oz,
                          float cell, int gx, int gy, int gz, float max_dist, float* dist, int* index, void* workspace,
                          size_t workspace_bytes, void* stream) {
    MVS_CHECK_ARG(query && target && dist && index && workspace);
    MVS_CHECK_ARG(n_query > 0 && n_target > 0 && gx > 0 && gy > 0 && gz > 0);
    MVS_CHECK_ARG(__builtin_isfinite(ox) && __builtin_isfinite(oy) && __builtin_isfinite(oz));
    MVS_CHECK_ARG(cell > 0.f && __builtin_isfinite(cell) && max_dist > 0.f && __builtin_isfinite(max_dist * max_dist));
    if (!nn_grid_ok(gx, gy, gz)) return MVS_E_SHAPE;
    const long long ncell = (long long)gx * gy * gz;
    const NnLayout L = nn_layout(n_query, n_target, ncell);
    if (workspace_bytes < L.total) return MVS_E_WORKSPACE;
    hipStream_t st = mvs_stream(stream);
    char* ws = static_cast<char*>(workspace);
    int* tstart = reinterpret_cast<int*>(ws + L.starts);
    int* qstart = tstart + L.stride;
    int* bsum = reinterpret_cast<int*>(ws + L.bsum);
    int* tcell = reinterpret_cast<int*>(ws + L.tcell);
    int* trank = reinterpret_cast<int*>(ws + L.trank);
    int* qcell = reinterpret_cast<int*>(ws + L.qcell);
    int* qrank = reinterpret_cast<int*>(ws + L.qrank);
    float4* tsorted = reinterpret_cast<float4*>(ws + L.tsorted);
    float4* qsorted = reinterpret_cast<float4*>(ws + L.qsorted);

    hipError_t e = hipMemsetAsync(tstart, 0, 2 * L.stride * sizeof(int), st);
    if (e != hipSuccess) return (int)e;
    hipLaunchKernelGGL(pc_cell_count_kernel, dim3(mvs_cdiv(n_target, PC_THREADS)), dim3(PC_THREADS), 0, st, target, n_target,
                       ox, oy, oz, cell, gx, gy, gz, tcell, trank, tstart);
    hipLaunchKernelGGL(pc_cell_count_kernel, dim3(mvs_cdiv(n_query, PC_THREADS)), dim3(PC_THREADS), 0, st, query, n_query,
                       ox, oy, oz, cell, gx, gy, gz, qcell, qrank, qstart);
    e = pc_scan(tstart, ncell + 1, L.stride, 2, bsum, st);
    if (e != hipSuccess) return (int)e;
    hipLaunchKernelGGL(pc_scatter_kernel, dim3(mvs_cdiv(n_target, PC_THREADS)), dim3(PC_THREADS), 0, st, target, n_target,
                       tcell, trank, tstart, tsorted);
    hipLaunchKernelGGL(pc_scatter_kernel, dim3(mvs_cdiv(n_query, PC_THREADS)), dim3(PC_THREADS), 0, st, query, n_query,
                       qcell, qrank, qstart, qsorted);
    hipLaunchKernelGGL(pc_nn_query_kernel, dim3(mvs_cdiv(n_query, PC_THREADS)), dim3(PC_THREADS), 0, st, qsorted, n_query,
                       tsorted, tstart, ox, oy, oz, cell, gx, gy, gz, max_dist, dist, index, (int*)nullptr);
    MVS_LAUNCH_RET();
}

extern "C" int mvs_nn_query_f32(int n_query, int n_target, float ox, float oy, float oz, float cell, int gx, int gy, int gz,
                                float max_dist, float* dist, int* index, int* visited, const void* workspace,
                                size_t workspace_bytes, void* stream) {
    MVS_CHECK_ARG(dist && index && workspace && n_query > 0 && n_target > 0 && gx > 0 && gy > 0 && gz > 0);
    MVS_CHECK_ARG(__builtin_isfinite(ox) && __builtin_isfinite(oy) && __builtin_isfinite(oz));
    MVS_CHECK_ARG(cell > 0.f && __builtin_isfinite(cell) && max_dist > 0.f && __builtin_isfinite(max_dist * max_dist));
    if (!nn_grid_ok(gx, gy, gz)) return MVS_E_SHAPE;
    const NnLayout L = nn_layout(n_query, n_target, (long long)gx * gy * gz);
    if (workspace_bytes < L.total) return MVS_E_WORKSPACE;
    const char* ws = static_cast<const char*>(workspace);
    hipLaunchKernelGGL(pc_nn_query_kernel, dim3(mvs_cdiv(n_query, PC_THREADS)), dim3(PC_THREADS), 0, mvs_stream(stream),
                       reinterpret_cast<const float4*>(ws + L.qsorted), n_query, reinterpret_cast<const float4*>(ws + L.tsorted),
                       reinterpret_cast<const int*>(ws + L.starts), ox, oy, oz, cell, gx, gy, gz, max_dist, dist, index, visited);
    MVS_LAUNCH_RET();
}

extern "C" size_t mvs_nn_target_workspace_bytes(int n_target, int gx, int gy, int gz) {
    if (n_target <= 0 || !nn_grid_ok(gx, gy, gz)) return 0;
    return target_layout(n_target, (long long)gx * gy * gz).total;
}

extern "C" int mvs_nn_target_build_f32(const float* target, int n_target, float ox, float oy, float oz, float cell, int gx, int gy,
                                       int gz, void* workspace, size_t workspace_bytes, void* stream) {
    MVS_CHECK_ARG(target && workspace && n_target > 0 && gx > 0 && gy > 0 && gz > 0);
    MVS_CHECK_ARG(__builtin_isfinite(ox) && __builtin_isfinite(oy) && __builtin_isfinite(oz));
    MVS_CHECK_ARG(cell > 0.f && __builtin_isfinite(cell));
    if (!nn_grid_ok(gx, gy, gz)) return MVS_E_SHAPE;
    const long long ncell = (long long)gx * gy * gz;
    const TargetLayout L = target_layout(n_target, ncell);
    if (workspace_bytes < L.total) return MVS_E_WORKSPACE;
    hipStream_t st = mvs_stream(stream);
    char* ws = static_cast<char*>(workspace);
    int* tstart = reinterpret_cast<int*>(ws + L.starts);
    int* tcell = reinterpret_cast<int*>(ws + L.tcell);
    int* trank = reinterpret_cast<int*>(ws + L.trank);
    hipError_t e = hipMemsetAsync(tstart, 0, (size_t)(ncell + 1) * sizeof(int), st);
    if (e != hipSuccess) return (int)e;
    hipLaunchKernelGGL(pc_cell_count_kernel, dim3(mvs_cdiv(n_target, PC_THREADS)), dim3(PC_THREADS), 0, st, target, n_target,
                       ox, oy, oz, cell, gx, gy, gz, tcell, trank, tstart);
    e = pc_scan(tstart, ncell + 1, 0, 1, reinterpret_cast<int*>(ws + L.bsum), st);
    if (e != hipSuccess) return (int)e;
    hipLaunchKernelGGL(pc_scatter_kernel, dim3(mvs_cdiv(n_target, PC_THREADS)), dim3(PC_THREADS), 0, st, target, n_target,
                       tcell, trank, tstart, reinterpret_cast<float4*>(ws + L.tsorted));
    MVS_LAUNCH_RET();
}

extern "C" size_t mvs_icp_step_workspace_bytes(int n_source) {
    return n_source > 0 ? icp_bytes(n_source) : 0;
}

extern "C" int mvs_icp_step_f32(const float* source, int n_source, const int* order, const double* T, const double* cp,
                                const double* cq, float ox, float oy, float oz, float cell, int gx, int gy, int gz, int n_target,
                                const void* target_workspace, size_t target_workspace_bytes, float max_corr_dist,
                                double* moments, float* dist, int* index, void* workspace, size_t workspace_bytes,
                                void* stream) {
    MVS_CHECK_ARG(source && T && cp && cq && target_workspace && moments && workspace);
    MVS_CHECK_ARG(n_source > 0 && n_target > 0 && gx > 0 && gy > 0 && gz > 0);
    MVS_CHECK_ARG(__builtin_isfinite(ox) && __builtin_isfinite(oy) && __builtin_isfinite(oz));
    MVS_CHECK_ARG(cell > 0.f && __builtin_isfinite(cell));
    MVS_CHECK_ARG(max_corr_dist > 0.f && __builtin_isfinite(max_corr_dist * max_corr_dist));
    PcIcpParams P;
    for (int k = 0; k < 12; ++k) {
        MVS_CHECK_ARG(__builtin_isfinite(T[k]));
        P.T[k] = T[k];
    }
    for (int k = 0; k < 3; ++k) {
        MVS_CHECK_ARG(__builtin_isfinite(cp[k]) && __builtin_isfinite(cq[k]));
        P.cp[k] = cp[k];
        P.cq[k] = cq[k];
    }
    if (!nn_grid_ok(gx, gy, gz)) return MVS_E_SHAPE;
    const TargetLayout L = target_layout(n_target, (long long)gx * gy * gz);
    if (target_workspace_bytes < L.total || workspace_bytes < icp_bytes(n_source)) return MVS_E_WORKSPACE;
    hipStream_t st = mvs_stream(stream);
    const char* tw = static_cast<const char*>(target_workspace);
    double* partial = static_cast<double*>(workspace);
    const int nb = icp_blocks(n_source);
    hipLaunchKernelGGL(pc_icp_step_kernel, dim3(nb), dim3(PC_THREADS), 0, st, source, n_source, order, P,
                       reinterpret_cast<const float4*>(tw + L.tsorted), reinterpret_cast<const int*>(tw + L.starts),
                       reinterpret_cast<const int*>(tw + L.tcell), reinterpret_cast<const int*>(tw + L.trank), ox, oy, oz, cell,
                       gx, gy, gz, max_corr_dist, partial, dist, index);
    hipLaunchKernelGGL(pc_icp_final_kernel, dim3(1), dim3(PC_THREADS), 0, st, partial, nb, moments);
    MVS_LAUNCH_RET();
}

extern "C" size_t mvs_dist_stats_workspace_bytes(int n, int n_thresholds) {
    if (n <= 0 || n_thresholds < 0 || n_thresholds > PC_MAX_THRESHOLDS) return 0;
    return stats_bytes(n);
}

extern "C" int mvs_dist_stats_f32(const float* dist, int n, float max_dist, const float* thresholds, int n_thresholds,
                                  double* out, void* workspace, size_t workspace_bytes, void* stream) {
    MVS_CHECK_ARG(dist && out && workspace && n > 0 && n_thresholds >= 0 && (n_thresholds == 0 || thresholds));
    MVS_CHECK_ARG(max_dist > 0.f && __builtin_isfinite(max_dist));
    if (n_thresholds > PC_MAX_THRESHOLDS) return MVS_E_SHAPE;
    PcThresholds thr{};
    for (int t = 0; t < n_thresholds; ++t) {
        MVS_CHECK_ARG(thresholds[t] > 0.f && thresholds[t] <= max_dist);
        thr.t[t] = thresholds[t];
    }
    if (workspace_bytes < stats_bytes(n)) return MVS_E_WORKSPACE;
    hipStream_t st = mvs_stream(stream);
    const int nb = stats_blocks(n);
    char* ws = static_cast<char*>(workspace);
    double* psum = reinterpret_cast<double*>(ws);
    int* pcnt = reinterpret_cast<int*>(ws + geo_align256((size_t)nb * sizeof(double)));
    hipLaunchKernelGGL(pc_stats_partial_kernel, dim3(nb), dim3(PC_THREADS), 0, st, dist, n, max_dist, thr, n_thresholds, psum, pcnt);
    hipLaunchKernelGGL(pc_stats_final_kernel, dim3(1), dim3(PC_THREADS), 0, st, psum, pcnt, nb, n_thresholds, out);
    MVS_LAUNCH_RET();
}

extern "C" int mvs_voxel_keys_f32(const float* xyz, int n, double min_x, double min_y, double min_z, double cell,
                                  long long* keys, void* stream) {
    MVS_CHECK_ARG(xyz && keys && n > 0 && cell > 0.0 && __builtin_isfinite(cell));
    MVS_CHECK_ARG(__builtin_isfinite(min_x) && __builtin_isfinite(min_y) && __builtin_isfinite(min_z));
    hipLaunchKernelGGL(pc_voxel_keys_kernel, dim3(mvs_cdiv(n, PC_THREADS)), dim3(PC_THREADS), 0, mvs_stream(stream), xyz, n,
                       min_x, min_y, min_z, cell, keys);
    MVS_LAUNCH_RET();
}

extern "C" size_t mvs_voxel_select_workspace_bytes(int n) {
    return n > 0 ? voxel_select_bytes(n) : 0;
}

extern "C" int mvs_voxel_select_f32(const float* xyz, int n, const long long* sorted_keys, const long long* order, float* out,
                                    int* count, void* workspace, size_t workspace_bytes, void* stream) {
    MVS_CHECK_ARG(xyz && sorted_keys && order && out && count && workspace && n > 0);
    if (workspace_bytes < voxel_select_bytes(n)) return MVS_E_WORKSPACE;
    hipStream_t st = mvs_stream(stream);
    const int nb = compact_blocks(n);
    char* ws = static_cast<char*>(workspace);
    uint8_t* keep = reinterpret_cast<uint8_t*>(ws);
    int* offs = reinterpret_cast<int*>(ws + geo_align256((size_t)n));
    int* bsum = reinterpret_cast<int*>(ws + geo_align256((size_t)n) + geo_align256(((size_t)nb + 1) * sizeof(int)));
    hipError_t e = hipMemsetAsync(offs + nb, 0, sizeof(int), st);
    if (e != hipSuccess) return (int)e;
    hipLaunchKernelGGL(pc_voxel_mark_kernel, dim3(mvs_cdiv(n, PC_THREADS)), dim3(PC_THREADS), 0, st, sorted_keys, order, n, keep);
    hipLaunchKernelGGL(geo_compact_count_kernel<PC_THREADS>, dim3(nb), dim3(PC_THREADS), 0, st, keep, (size_t)n, offs);
    e = pc_scan(offs, (long long)nb + 1, 0, 1, bsum, st);
    if (e != hipSuccess) return (int)e;
    hipLaunchKernelGGL(pc_compact_write_kernel, dim3(nb), dim3(PC_THREADS), 0, st, keep, xyz, n, offs, nb, out, count);
    MVS_LAUNCH_RET();
}
