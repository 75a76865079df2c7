// TSDF fusion of depth maps into a volume (mvs_tsdf_integrate_f32) and extraction of its zero surface by naive surface nets
// (mvs_surface_nets_count_f32, mvs_surface_nets_write_f32).  The semantics are normative in mvsnet_amd/mesh.py;
// tests/mesh_reference.py restates them in numpy, and the kernels equal its float32 statement byte for byte.
//
//   filter     df = D where D > 0, finite and P >= prob_threshold, else 0 (all views of the call; the gathers read df only);
//   integrate  a gather per node: a workgroup owns a brick of 64 x 4 x 4 nodes, lanes of a wave along x, so the 64 taps of a
//              wave fall on neighbouring pixels of a view.  A lane takes its four nodes one after the other; per node sum
//              and count are read once, the views are taken TS_VIEWS at a time (their TS_VIEWS gathers in flight together,
//              P_v by scalar loads), added in ascending order, and sum and count are written once.  No atomics: a node has
//              one owner.  (Leaving out, per brick, the views whose frustum the brick's bounding sphere cannot reach was
//              built and measured: it never gained, DESIGN 4.13, and is not here);
//   classify   one lane per cell: valid (8 corners observed) and active (valid, corners not all on one side);
//   edges      one lane per node: the number of triangles its three edges give (0, 2, 4 or 6);
//   write      one lane per node: the vertex of its cell when active, at rank - 1 of the inclusive scan of the active flags,
//              and its triangles at the inclusive scan of the counts minus its own count.  The scans are the caller's.
#include "geom_common.h"

// every product and sum below is rounded on its own: the numpy statement has no fused multiply-add
#pragma clang fp contract(off)

namespace {

constexpr int TS_THREADS = 256;
constexpr int TS_BX = 64, TS_BY = 4, TS_BZ = 4;    // brick: a wave is one x-row of 64 nodes, a workgroup 4 rows, 4 slices in turn
constexpr int TS_VIEWS = 4;                        // views a lane works on at once (loads in flight)
constexpr int TS_MAX_AXIS = 1 << 24;               // H, W, image sizes: every pixel coordinate is an exact float32
constexpr int TS_CELL_VALID = 1, TS_CELL_ACTIVE = 2;

// o + s float(i): a rounded product, then a rounded sum.
__device__ __forceinline__ float ts_coord(float o, float s, float i) {
    return o + s * i;
}

template <bool COLOUR>
__global__ __launch_bounds__(TS_THREADS) void ts_integrate_kernel(const float* __restrict__ df, int V, int H, int W,
                                                                   const float* __restrict__ proj,
                                                                   const unsigned char* __restrict__ images, int img_h, int img_w,
                                                                   float ox, float oy, float oz, float voxel, int nx, int ny, int nz,
                                                                   int bricks_x, int bricks_y, float trunc,
                                                                   float* __restrict__ sum, int* __restrict__ count,
                                                                   unsigned int* __restrict__ rgb_sum, int* __restrict__ rgb_count) {
    const int b = blockIdx.x;
    const int i0 = (b % bricks_x) * TS_BX, j0 = ((b / bricks_x) % bricks_y) * TS_BY, k0 = (b / (bricks_x * bricks_y)) * TS_BZ;
    const int lane = threadIdx.x & 63;
    const int i = i0 + lane, j = j0 + (threadIdx.x >> 6);
    const bool column = i < nx && j < ny;
    const float x = ts_coord(ox, voxel, (float)i), y = ts_coord(oy, voxel, (float)j);
    const float wmax = (float)(W - 1), hmax = (float)(H - 1);
    const size_t plane = (size_t)H * W;
    const float neg_trunc = -trunc;

    for (int kz = 0; kz < TS_BZ; ++kz) {
        const int k = k0 + kz;
        if (k >= nz) break;                                                    // uniform over the workgroup
        const float z = ts_coord(oz, voxel, (float)k);
        const size_t node = ((size_t)k * ny + j) * nx + i;
        float s = 0.f;
        int c = 0;
        unsigned int cr = 0, cg = 0, cb = 0;
        int cn = 0;
        if (column) {
            s = sum[node];
            c = count[node];
            if constexpr (COLOUR) {
                cr = rgb_sum[3 * node]; cg = rgb_sum[3 * node + 1]; cb = rgb_sum[3 * node + 2];
                cn = rgb_count[node];
            }
        }
        for (int vb = 0; vb < V; vb += TS_VIEWS) {
            float w[TS_VIEWS], d[TS_VIEWS], fx[TS_VIEWS], fy[TS_VIEWS];
            int view[TS_VIEWS];
#pragma unroll
            for (int t = 0; t < TS_VIEWS; ++t) {
                const int v = min(vb + t, V - 1);                              // wave-uniform: P arrives by scalar loads
                view[t] = v;
                geo_cfloat* P = (geo_cfloat*)proj + 12 * (size_t)v;                // the constant space: scalar loads
                w[t] = geo_row(P + 8, x, y, z);
                fx[t] = geo_pixel(geo_row(P, x, y, z), w[t]);
                fy[t] = geo_pixel(geo_row(P + 4, x, y, z), w[t]);
                // in float, before any conversion: a huge or non-finite coordinate is never converted
                const bool in = column && vb + t < V && GEO_VISIBLE(w[t], fx[t], fy[t], 0.f, wmax, hmax);
                // a culled lane loads element 0 instead (a load without a branch) and masks it to 0, which is "no depth"
                const size_t at = in ? (size_t)v * plane + (size_t)(int)fy[t] * W + (int)fx[t] : (size_t)0;
                const float g = df[at];
                d[t] = in ? g : 0.f;
            }
#pragma unroll
            for (int t = 0; t < TS_VIEWS; ++t) {
                if (!(d[t] > 0.f)) continue;
                const float sdf = d[t] - w[t];
                if (sdf < neg_trunc) continue;
                s = s + fminf(__fdiv_rn(sdf, trunc), 1.0f);
                c += 1;
                if constexpr (COLOUR) {
                    if (sdf <= trunc) {
                        const long long px = ((2LL * (long long)(int)fx[t] + 1) * img_w) / (2LL * W);
                        const long long py = ((2LL * (long long)(int)fy[t] + 1) * img_h) / (2LL * H);
                        const unsigned char* q = images + (((size_t)view[t] * img_h + (size_t)py) * img_w + (size_t)px) * 3;
                        cr += q[0]; cg += q[1]; cb += q[2];
                        cn += 1;
                    }
                }
            }
        }
        if (column) {
            sum[node] = s;
            count[node] = c;
            if constexpr (COLOUR) {
                rgb_sum[3 * node] = cr; rgb_sum[3 * node + 1] = cg; rgb_sum[3 * node + 2] = cb;
                rgb_count[node] = cn;
            }
        }
    }
}

// ------------------------------------------------------------------------------------------------ surface nets

struct TsNode { bool observed, inside; float f; };

__device__ __forceinline__ TsNode ts_node(const float* __restrict__ sum, const int* __restrict__ count, size_t node, int min_count) {
    const int c = count[node];
    TsNode r;
    r.observed = c >= min_count;
    r.f = r.observed ? __fdiv_rn(sum[node], (float)c) : 0.f;
    r.inside = r.observed && r.f < 0.f;
    return r;
}

// One lane per cell, cells in linear order (k (ny-1) + j) (nx-1) + i.
__global__ __launch_bounds__(TS_THREADS) void ts_classify_kernel(const float* __restrict__ sum, const int* __restrict__ count, int nx,
                                                                  int ny, int nz, int min_count, long long cells,
                                                                  int* __restrict__ cell_flags, int* __restrict__ totals) {
    const long long cidx = (long long)blockIdx.x * TS_THREADS + threadIdx.x;
    int active = 0;
    if (cidx < cells) {
        const int i = (int)(cidx % (nx - 1)), j = (int)((cidx / (nx - 1)) % (ny - 1)), k = (int)(cidx / ((long long)(nx - 1) * (ny - 1)));
        bool valid = true;
        int inside = 0;
#pragma unroll
        for (int o = 0; o < 8; ++o) {
            const TsNode nd = ts_node(sum, count, ((size_t)(k + (o >> 2)) * ny + (j + ((o >> 1) & 1))) * nx + (i + (o & 1)), min_count);
            valid &= nd.observed;
            inside += nd.inside ? 1 : 0;
        }
        active = (valid && inside > 0 && inside < 8) ? 1 : 0;
        cell_flags[cidx] = (valid ? TS_CELL_VALID : 0) | (active ? TS_CELL_ACTIVE : 0);
    }
    const int m = __popcll(__ballot(active));
    if ((threadIdx.x & 63) == 0 && m) atomicAdd(totals, m);              // an integer total: the same in any order
}

// Cell (ci, cj, ck) exists and is valid.
__device__ __forceinline__ bool ts_cell_valid(const int* __restrict__ cell_flags, int nx, int ny, int nz, int ci, int cj, int ck) {
    if (ci < 0 || cj < 0 || ck < 0 || ci >= nx - 1 || cj >= ny - 1 || ck >= nz - 1) return false;
    return (cell_flags[((size_t)ck * (ny - 1) + cj) * (nx - 1) + ci] & TS_CELL_VALID) != 0;
}

// Does the node edge from q = (i, j, k) along axis a give its two triangles?  *inside_q: whether q is inside.
__device__ __forceinline__ bool ts_edge_faces(const float* __restrict__ sum, const int* __restrict__ count,
                                              const int* __restrict__ cell_flags, int nx, int ny, int nz, int min_count, int i, int j,
                                              int k, int a, const TsNode& q) {
    const int ea[3] = {a == 0, a == 1, a == 2}, b = (a + 1) % 3, c = (a + 2) % 3;
    const int eb[3] = {b == 0, b == 1, b == 2}, ec[3] = {c == 0, c == 1, c == 2};
    const int dims[3] = {nx, ny, nz}, at[3] = {i, j, k};
    if (at[a] + 1 >= dims[a] || !q.observed) return false;
    const TsNode p = ts_node(sum, count, ((size_t)(k + ea[2]) * ny + (j + ea[1])) * nx + (i + ea[0]), min_count);
    if (!p.observed || p.inside == q.inside) return false;
    return ts_cell_valid(cell_flags, nx, ny, nz, i - eb[0] - ec[0], j - eb[1] - ec[1], k - eb[2] - ec[2]) &&
           ts_cell_valid(cell_flags, nx, ny, nz, i - ec[0], j - ec[1], k - ec[2]) &&
           ts_cell_valid(cell_flags, nx, ny, nz, i, j, k) &&
           ts_cell_valid(cell_flags, nx, ny, nz, i - eb[0], j - eb[1], k - eb[2]);
}

// One lane per node: the number of its triangles.
__global__ __launch_bounds__(TS_THREADS) void ts_edges_kernel(const float* __restrict__ sum, const int* __restrict__ count,
                                                               const int* __restrict__ cell_flags, int nx, int ny, int nz,
                                                               int min_count, long long nodes, int* __restrict__ face_count,
                                                               int* __restrict__ totals) {
    const long long q = (long long)blockIdx.x * TS_THREADS + threadIdx.x;
    int faces = 0;
    if (q < nodes) {
        const int i = (int)(q % nx), j = (int)((q / nx) % ny), k = (int)(q / ((long long)nx * ny));
        const TsNode nd = ts_node(sum, count, (size_t)q, min_count);
#pragma unroll
        for (int a = 0; a < 3; ++a) faces += ts_edge_faces(sum, count, cell_flags, nx, ny, nz, min_count, i, j, k, a, nd) ? 2 : 0;
        face_count[q] = faces;
    }
    int t = faces;
#pragma unroll
    for (int o = 32; o > 0; o >>= 1) t += __shfl_xor(t, o, 64);
    if ((threadIdx.x & 63) == 0 && t) atomicAdd(totals + 1, t);
}

template <bool COLOUR>
__global__ __launch_bounds__(TS_THREADS) void ts_write_kernel(const float* __restrict__ sum, const int* __restrict__ count,
                                                               const unsigned int* __restrict__ rgb_sum,
                                                               const int* __restrict__ rgb_count, float ox, float oy, float oz,
                                                               float voxel, int nx, int ny, int nz, int min_count, long long nodes,
                                                               const int* __restrict__ cell_flags, const int* __restrict__ face_count,
                                                               const int* __restrict__ cell_rank, const int* __restrict__ face_end,
                                                               int M, int F, float* __restrict__ vertices,
                                                               unsigned char* __restrict__ colours, int* __restrict__ faces) {
    const long long q = (long long)blockIdx.x * TS_THREADS + threadIdx.x;
    if (q >= nodes) return;
    const int i = (int)(q % nx), j = (int)((q / nx) % ny), k = (int)(q / ((long long)nx * ny));
    auto cell_index = [&](int ci, int cj, int ck) { return ((size_t)ck * (ny - 1) + cj) * (nx - 1) + ci; };

    if (i < nx - 1 && j < ny - 1 && k < nz - 1) {
        const size_t cidx = cell_index(i, j, k);
        const int id = cell_rank[cidx] - 1;
        if ((cell_flags[cidx] & TS_CELL_ACTIVE) && id >= 0 && id < M) {
            TsNode nd[8];
#pragma unroll
            for (int o = 0; o < 8; ++o)
                nd[o] = ts_node(sum, count, ((size_t)(k + (o >> 2)) * ny + (j + ((o >> 1) & 1))) * nx + (i + (o & 1)), min_count);
            float acc[3] = {0.f, 0.f, 0.f};
            int m = 0;
#pragma unroll
            for (int a = 0; a < 3; ++a) {
                const int b = (a + 1) % 3, c = (a + 2) % 3;
#pragma unroll
                for (int e = 0; e < 4; ++e) {
                    const int off_c = e >> 1, off_b = e & 1;
                    const int lo = (off_b << b) | (off_c << c), hi = lo | (1 << a);
                    if (nd[lo].inside != nd[hi].inside) {
                        const float tau = __fdiv_rn(nd[lo].f, nd[lo].f - nd[hi].f);
                        acc[a] = acc[a] + tau;
                        acc[b] = acc[b] + (float)off_b;
                        acc[c] = acc[c] + (float)off_c;
                        m += 1;
                    }
                }
            }
            const float fm = (float)m;
            const float o3[3] = {ox, oy, oz};
            const int at[3] = {i, j, k};
#pragma unroll
            for (int a = 0; a < 3; ++a) {
                const float local = __fdiv_rn(acc[a], fm);
                const float g = (float)at[a] + local;
                vertices[3 * (size_t)id + a] = o3[a] + voxel * g;
            }
            unsigned long long R[3] = {0, 0, 0}, cn = 0;
            if constexpr (COLOUR) {
#pragma unroll
                for (int o = 0; o < 8; ++o) {
                    const size_t node = ((size_t)(k + (o >> 2)) * ny + (j + ((o >> 1) & 1))) * nx + (i + (o & 1));
                    R[0] += rgb_sum[3 * node]; R[1] += rgb_sum[3 * node + 1]; R[2] += rgb_sum[3 * node + 2];
                    cn += (unsigned long long)(unsigned int)rgb_count[node];
                }
            }
#pragma unroll
            for (int a = 0; a < 3; ++a) colours[3 * (size_t)id + a] = cn ? (unsigned char)((2 * R[a] + cn) / (2 * cn)) : 0;
        }
    }

    const int mine = face_count[q];
    if (mine == 0) return;
    int at_face = face_end[q] - mine;
    const TsNode nq = ts_node(sum, count, (size_t)q, min_count);
#pragma unroll
    for (int a = 0; a < 3; ++a) {
        if (!ts_edge_faces(sum, count, cell_flags, nx, ny, nz, min_count, i, j, k, a, nq)) continue;
        const int b = (a + 1) % 3, c = (a + 2) % 3;
        const int eb[3] = {b == 0, b == 1, b == 2}, ec[3] = {c == 0, c == 1, c == 2};
        const int c0 = cell_rank[cell_index(i - eb[0] - ec[0], j - eb[1] - ec[1], k - eb[2] - ec[2])] - 1;
        const int c1 = cell_rank[cell_index(i - ec[0], j - ec[1], k - ec[2])] - 1;
        const int c2 = cell_rank[cell_index(i, j, k)] - 1;
        const int c3 = cell_rank[cell_index(i - eb[0], j - eb[1], k - eb[2])] - 1;
        if (at_face >= 0 && at_face + 2 <= F) {
            int* f = faces + 3 * (size_t)at_face;
            f[0] = c0; f[1] = nq.inside ? c1 : c2; f[2] = nq.inside ? c2 : c1;
            f[3] = c0; f[4] = nq.inside ? c2 : c3; f[5] = nq.inside ? c3 : c2;
        }
        at_face += 2;
    }
}

bool ts_volume_ok(int nx, int ny, int nz) { return (long long)nx * ny * nz <= 0x7fffffffLL; }

long long ts_cells(int nx, int ny, int nz) { return (long long)(nx - 1) * (ny - 1) * (nz - 1); }

}  // namespace

extern "C" size_t mvs_tsdf_integrate_workspace_bytes(int V, int H, int W) {
    if (V <= 0 || H <= 0 || W <= 0 || !geo_pixels_ok(V, H, W, TS_MAX_AXIS)) return 0;
    return geo_align256((size_t)V * H * W * sizeof(float));
}

extern "C" int mvs_tsdf_integrate_f32(const float* depth, const float* prob, int V, int H, int W, const float* proj,
                                      const unsigned char* images, int img_h, int img_w, const float* origin, float voxel, int nx,
                                      int ny, int nz, float trunc, float prob_threshold, int flags, float* sum, int* count,
                                      unsigned int* rgb_sum, int* rgb_count, void* workspace, size_t workspace_bytes, void* stream) {
    MVS_CHECK_ARG(depth && prob && proj && origin && sum && count && workspace);
    MVS_CHECK_ARG(V > 0 && H > 0 && W > 0 && nx > 0 && ny > 0 && nz > 0);
    MVS_CHECK_ARG(__builtin_isfinite(origin[0]) && __builtin_isfinite(origin[1]) && __builtin_isfinite(origin[2]));
    MVS_CHECK_ARG(voxel > 0.f && __builtin_isfinite(voxel) && trunc > 0.f && __builtin_isfinite(trunc));
    MVS_CHECK_ARG(!__builtin_isnan(prob_threshold) && flags == 0);
    const bool colour = images != nullptr;
    if (colour) MVS_CHECK_ARG(rgb_sum && rgb_count && img_h > 0 && img_w > 0);
    if (!ts_volume_ok(nx, ny, nz) || !geo_pixels_ok(V, H, W, TS_MAX_AXIS)) return MVS_E_SHAPE;
    if (colour && (img_h > TS_MAX_AXIS || img_w > TS_MAX_AXIS)) return MVS_E_SHAPE;
    const size_t pixels = (size_t)V * H * W;
    if (workspace_bytes < geo_align256(pixels * sizeof(float))) return MVS_E_WORKSPACE;
    hipStream_t st = mvs_stream(stream);
    float* df = static_cast<float*>(workspace);
    hipLaunchKernelGGL(geo_filter_kernel<TS_THREADS>, dim3(mvs_cdiv((long long)pixels, TS_THREADS)), dim3(TS_THREADS), 0, st, depth, prob, pixels,
                       prob_threshold, df);
    const int bx = mvs_cdiv(nx, TS_BX), by = mvs_cdiv(ny, TS_BY), bz = mvs_cdiv(nz, TS_BZ);
    const dim3 grid((unsigned)((long long)bx * by * bz));
    if (colour)
        hipLaunchKernelGGL(ts_integrate_kernel<true>, grid, dim3(TS_THREADS), 0, st, df, V, H, W, proj, images, img_h, img_w, origin[0],
                           origin[1], origin[2], voxel, nx, ny, nz, bx, by, trunc, sum, count, rgb_sum, rgb_count);
    else
        hipLaunchKernelGGL(ts_integrate_kernel<false>, grid, dim3(TS_THREADS), 0, st, df, V, H, W, proj, images, img_h, img_w, origin[0],
                           origin[1], origin[2], voxel, nx, ny, nz, bx, by, trunc, sum, count, rgb_sum, rgb_count);
    MVS_LAUNCH_RET();
}

extern "C" size_t mvs_surface_nets_workspace_bytes(int nx, int ny, int nz) {
    if (nx <= 0 || ny <= 0 || nz <= 0 || !ts_volume_ok(nx, ny, nz)) return 0;
    const long long cells = (nx > 1 && ny > 1 && nz > 1) ? ts_cells(nx, ny, nz) : 0;
    return geo_align256((size_t)std::max(cells, 1LL) * sizeof(int)) + geo_align256((size_t)nx * ny * nz * sizeof(int));
}

extern "C" int mvs_surface_nets_count_f32(const float* sum, const int* count, int nx, int ny, int nz, int min_count, int* totals,
                                          void* workspace, size_t workspace_bytes, void* stream) {
    MVS_CHECK_ARG(sum && count && totals && workspace);
    MVS_CHECK_ARG(nx > 0 && ny > 0 && nz > 0 && min_count >= 1);
    if (!ts_volume_ok(nx, ny, nz)) return MVS_E_SHAPE;
    if (workspace_bytes < mvs_surface_nets_workspace_bytes(nx, ny, nz)) return MVS_E_WORKSPACE;
    hipStream_t st = mvs_stream(stream);
    const long long nodes = (long long)nx * ny * nz;
    const long long cells = (nx > 1 && ny > 1 && nz > 1) ? ts_cells(nx, ny, nz) : 0;
    int* cell_flags = static_cast<int*>(workspace);
    int* face_count = reinterpret_cast<int*>(static_cast<char*>(workspace) + geo_align256((size_t)std::max(cells, 1LL) * sizeof(int)));
    hipError_t e = hipMemsetAsync(totals, 0, 2 * sizeof(int), st);
    if (e != hipSuccess) return (int)e;
    if (cells == 0) {                                                          // an axis of one node: no cells, no faces
        e = hipMemsetAsync(cell_flags, 0, sizeof(int), st);
        if (e != hipSuccess) return (int)e;
        e = hipMemsetAsync(face_count, 0, (size_t)nodes * sizeof(int), st);
        return (int)e;
    }
    hipLaunchKernelGGL(ts_classify_kernel, dim3(mvs_cdiv(cells, TS_THREADS)), dim3(TS_THREADS), 0, st, sum, count, nx, ny, nz,
                       min_count, cells, cell_flags, totals);
    hipLaunchKernelGGL(ts_edges_kernel, dim3(mvs_cdiv(nodes, TS_THREADS)), dim3(TS_THREADS), 0, st, sum, count, cell_flags, nx, ny, nz,
                       min_count, nodes, face_count, totals);
    MVS_LAUNCH_RET();
}

extern "C" int mvs_surface_nets_write_f32(const float* sum, const int* count, const unsigned int* rgb_sum, const int* rgb_count,
                                          const float* origin, float voxel, int nx, int ny, int nz, int min_count,
                                          const int* cell_rank, const int* face_end, int M, int F, float* vertices,
                                          unsigned char* colours, int* faces, void* workspace, size_t workspace_bytes, void* stream) {
    MVS_CHECK_ARG(sum && count && origin && cell_rank && face_end && workspace);
    MVS_CHECK_ARG((rgb_sum == nullptr) == (rgb_count == nullptr));
    MVS_CHECK_ARG(nx > 0 && ny > 0 && nz > 0 && min_count >= 1 && M >= 0 && F >= 0);
    MVS_CHECK_ARG((M == 0 || (vertices && colours)) && (F == 0 || faces));
    MVS_CHECK_ARG(__builtin_isfinite(origin[0]) && __builtin_isfinite(origin[1]) && __builtin_isfinite(origin[2]));
    MVS_CHECK_ARG(voxel > 0.f && __builtin_isfinite(voxel));
    if (!ts_volume_ok(nx, ny, nz)) return MVS_E_SHAPE;
    if (workspace_bytes < mvs_surface_nets_workspace_bytes(nx, ny, nz)) return MVS_E_WORKSPACE;
    if (M == 0 || nx < 2 || ny < 2 || nz < 2) return 0;                        // no vertex, so no face either
    const long long nodes = (long long)nx * ny * nz;
    const int* cell_flags = static_cast<const int*>(workspace);
    const int* face_count = reinterpret_cast<const int*>(static_cast<const char*>(workspace) +
                                                         geo_align256((size_t)ts_cells(nx, ny, nz) * sizeof(int)));
    hipStream_t st = mvs_stream(stream);
    const dim3 grid(mvs_cdiv(nodes, TS_THREADS));
    if (rgb_sum)
        hipLaunchKernelGGL(ts_write_kernel<true>, grid, dim3(TS_THREADS), 0, st, sum, count, rgb_sum, rgb_count, origin[0], origin[1],
                           origin[2], voxel, nx, ny, nz, min_count, nodes, cell_flags, face_count, cell_rank, face_end, M, F, vertices,
                           colours, faces);
    else
        hipLaunchKernelGGL(ts_write_kernel<false>, grid, dim3(TS_THREADS), 0, st, sum, count, rgb_sum, rgb_count, origin[0], origin[1],
                           origin[2], voxel, nx, ny, nz, min_count, nodes, cell_flags, face_count, cell_rank, face_end, M, F, vertices,
                           colours, faces);
    MVS_LAUNCH_RET();
}
