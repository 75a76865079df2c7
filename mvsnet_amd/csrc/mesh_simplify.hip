// Mesh simplification by vertex clustering on a uniform grid of cells (mvs_mesh_cluster_keys_f32, mvs_mesh_cluster_heads_i64,
// mvs_mesh_cluster_sums_f32, mvs_mesh_cluster_faces_i32, mvs_mesh_cluster_mark_i32).  The semantics are normative in
// mvsnet_amd/mesh_simplify.py; tests/mesh_simplify_reference.py restates them in numpy, and the kernels equal it byte for byte.
// The caller (torch) owns the memory, the stable sorts and the prefix sums between the calls; the last step is
// mesh_components.hip's mvs_mesh_compact_write_f32 on the clusters.
//
//   keys       cell: one lane per vertex, the cell of the vertex in float64 (every operation rounded on its own): keys[v] = the
//              63-bit key of a clusterable vertex, else -1, and its three 20-bit offsets inside the cell;
//              use: one lane per face: a face is valid when its three indices lie in 0..M-1 and keys[] is >= 0 at all three;
//              a valid face stores 1 to used[] at its vertices (several writers, one value);
//              drop: keys[v] = -1 where used[v] is 0: only vertices that a valid face names contribute;
//   heads      on the sorted keys: head[i] = 1 where a run of equal keys >= 0 starts; the caller's inclusive scan of head
//              ranks the clusters in ascending key order;
//   sums       one lane per sorted position: vertex_cluster[order[i]] = rank - 1 (-1 for key -1), and n, the offsets and the
//              colour bytes are summed per cluster.  The input is sorted, so the lanes of a wave that share a cluster are
//              neighbours: a segmented sum over them (six steps of shuffles, in 32 bits: 64 lanes of 20 bits) leaves every
//              run's sum in its first lane, which issues the one 64-bit atomic per (wave, cluster) and word.  Integer sums: the
//              bytes do not depend on the order;
//              finish: one lane per cluster: position and colour from the sums;
//   faces      one lane per face: its three clusters, -1 -1 -1 for an invalid face; the sort key of a valid face with three
//              different clusters is their ascending triple (one int64 of 3 x 21 bits, or two int64), INT64_MAX otherwise;
//   mark       on the sorted face keys: the first face of a run stays (the sort is stable: the smallest input index);
//              face_keep for all F, plain stores of 1 to vertex_keep at the clusters of a kept face.
#include "geom_common.h"

#pragma clang fp contract(off)

namespace {

constexpr int MS_THREADS = 256;
constexpr int MS_STATUS_WORDS = 64;                 // 256 bytes at the start of the workspace
constexpr int MS_INVALID = 0, MS_UNCLUSTERABLE = 1, MS_DEGENERATE = 2, MS_DUPLICATE = 3;
constexpr int MS_ACC_WORDS = 8;                     // per cluster: n, S[3], C[3], key
constexpr long long MS_MAX = 0x7fffffffLL;
constexpr long long MS_CELLS = 1LL << 21;           // cells per axis
constexpr double MS_QUANTUM = 1048576.0;            // offsets are multiples of 2^-20 of a cell
constexpr long long MS_DEAD = 0x7fffffffffffffffLL;

constexpr int MS_MAX_BLOCKS = 2048;                 // of the kernel that strides over the faces

struct MsGrid { double o[3], cell; };

// Adds the workgroup's sum of `mine` to *word with one atomic, none when the sum is 0.  Every thread of the workgroup calls it,
// once.  (A wave, an atomic was measured on the degenerate faces, which are most faces of a mesh that is being simplified:
// 31 000 atomics on one word took 0.33 of the 0.37 ms of the faces launch at 2 M faces)
__device__ __forceinline__ void ms_block_count(int mine, int* word) {
    __shared__ int s_n[MS_THREADS / MVS_WAVE];
    int n = mine;
#pragma unroll
    for (int o = 32; o > 0; o >>= 1) n += __shfl_xor(n, o, 64);
    if ((threadIdx.x & 63) == 0) s_n[threadIdx.x >> 6] = n;
    __syncthreads();
    if (threadIdx.x == 0) {
        int total = 0;
#pragma unroll
        for (int w = 0; w < MS_THREADS / MVS_WAVE; ++w) total += s_n[w];
        if (total) atomicAdd(word, total);
    }
}

__global__ __launch_bounds__(MS_THREADS) void ms_cell_kernel(const float* __restrict__ vertices, long long M, MsGrid g,
                                                              long long* __restrict__ keys, int* __restrict__ offsets,
                                                              int* status) {
    const long long v = (long long)blockIdx.x * MS_THREADS + threadIdx.x;
    bool bad = false;
    if (v < M) {
        bool ok = true;
        long long key = 0;
        int q[3] = {0, 0, 0};
#pragma unroll
        for (int a = 0; a < 3; ++a) {
            const float x = vertices[3 * (size_t)v + a];
            const double u = ((double)x - g.o[a]) / g.cell;
            const double k = floor(u);
            const bool in = __builtin_isfinite(x) && k >= 0.0 && k <= (double)(MS_CELLS - 1);   // NaN and inf fail
            ok = ok && in;
            if (in) {
                key |= (long long)k << (21 * a);
                q[a] = (int)floor((u - k) * MS_QUANTUM);                       // u - k and the product are exact
            }
        }
        keys[v] = ok ? key : -1;
#pragma unroll
        for (int a = 0; a < 3; ++a) offsets[3 * (size_t)v + a] = ok ? q[a] : 0;
        bad = !ok;
    }
    ms_block_count(bad ? 1 : 0, status + MS_UNCLUSTERABLE);
}

__global__ __launch_bounds__(MS_THREADS) void ms_use_kernel(const int* __restrict__ faces, long long M, long long F,
                                                             const long long* __restrict__ keys, int* __restrict__ used,
                                                             int* status) {
    const long long f = (long long)blockIdx.x * MS_THREADS + threadIdx.x;
    bool invalid = false;
    if (f < F) {
        const int a = faces[3 * (size_t)f], b = faces[3 * (size_t)f + 1], c = faces[3 * (size_t)f + 2];
        bool valid = a >= 0 && a < M && b >= 0 && b < M && c >= 0 && c < M;
        valid = valid && keys[a] >= 0 && keys[b] >= 0 && keys[c] >= 0;
        if (valid) used[a] = used[b] = used[c] = 1;                            // several writers, one value
        invalid = !valid;
    }
    ms_block_count(invalid ? 1 : 0, status + MS_INVALID);
}

__global__ __launch_bounds__(MS_THREADS) void ms_drop_kernel(const int* __restrict__ used, long long M,
                                                              long long* __restrict__ keys) {
    const long long v = (long long)blockIdx.x * MS_THREADS + threadIdx.x;
    if (v < M && used[v] == 0) keys[v] = -1;
}

__global__ __launch_bounds__(MS_THREADS) void ms_heads_kernel(const long long* __restrict__ sorted_keys, long long M,
                                                               int* __restrict__ head) {
    const long long i = (long long)blockIdx.x * MS_THREADS + threadIdx.x;
    if (i >= M) return;
    const long long k = sorted_keys[i];
    head[i] = (k >= 0 && (i == 0 || sorted_keys[i - 1] != k)) ? 1 : 0;
}

template <bool COLOUR>
__global__ __launch_bounds__(MS_THREADS) void ms_sums_kernel(const long long* __restrict__ sorted_keys,
                                                              const long long* __restrict__ order, const int* __restrict__ head_rank,
                                                              const int* __restrict__ offsets, const unsigned char* __restrict__ colours,
                                                              long long M, int* __restrict__ vertex_cluster,
                                                              unsigned long long* __restrict__ acc) {
    const long long i = (long long)blockIdx.x * MS_THREADS + threadIdx.x;
    constexpr int W = COLOUR ? 7 : 4;
    int cid = -1;
    int s[7] = {0, 0, 0, 0, 0, 0, 0};
    bool head = false;
    long long key = -1;
    if (i < M) {
        key = sorted_keys[i];
        const long long o = order[i];
        const long long id = (long long)head_rank[i] - 1;
        if (o >= 0 && o < M) {                                                 // the order and the ranks are the caller's
            if (key >= 0 && id >= 0 && id < M) {
                cid = (int)id;
                head = i == 0 || sorted_keys[i - 1] != key;
                s[0] = 1;
#pragma unroll
                for (int a = 0; a < 3; ++a) {
                    s[1 + a] = offsets[3 * (size_t)o + a];
                    if constexpr (COLOUR) s[4 + a] = colours[3 * (size_t)o + a];
                }
            }
            vertex_cluster[o] = cid;
        }
    }
    if (head) acc[(size_t)cid * MS_ACC_WORDS + 7] = (unsigned long long)key;   // one writer: the run's first position
#ifdef MS_NO_WAVE_REDUCE                                                       // measurement build: a lane, its atomics
    if (cid >= 0) {
#pragma unroll
        for (int w = 0; w < W; ++w) atomicAdd(acc + (size_t)cid * MS_ACC_WORDS + w, (unsigned long long)s[w]);
    }
#else
    // segmented sum over the runs of equal cid inside the wave: after the step with offset o, a lane holds the sum over itself
    // and the up to 2 o - 1 lanes above it that share its cid; runs are contiguous, so lane + o in the run means all between are
    const int lane = threadIdx.x & 63;
#pragma unroll
    for (int o = 1; o < 64; o <<= 1) {
        const int other = __shfl_down(cid, o, 64);
        const bool take = lane + o < 64 && other == cid;
#pragma unroll
        for (int w = 0; w < W; ++w) {
            const int t = __shfl_down(s[w], o, 64);
            if (take) s[w] += t;
        }
    }
    const int before = __shfl_up(cid, 1, 64);
    if (cid >= 0 && (lane == 0 || before != cid)) {
#pragma unroll
        for (int w = 0; w < W; ++w) atomicAdd(acc + (size_t)cid * MS_ACC_WORDS + w, (unsigned long long)s[w]);
    }
#endif
}

// One lane per cluster slot; K = the last rank.  a = S / (n 2^20); b = k + a; c = b cell; d = o + c; float32(d).
template <bool COLOUR>
__global__ __launch_bounds__(MS_THREADS) void ms_finish_kernel(const unsigned long long* __restrict__ acc,
                                                                const int* __restrict__ head_rank, long long M, MsGrid g,
                                                                float* __restrict__ cluster_vertices,
                                                                unsigned char* __restrict__ cluster_colours) {
    const long long c = (long long)blockIdx.x * MS_THREADS + threadIdx.x;
    if (c >= M || c >= (long long)head_rank[M - 1]) return;
    const unsigned long long* w = acc + (size_t)c * MS_ACC_WORDS;
    const long long n = (long long)w[0], key = (long long)w[7];
    if (n <= 0) return;                                                        // every ranked cluster has a member
    const double den = (double)(n * (1LL << 20));
#pragma unroll
    for (int a = 0; a < 3; ++a) {
        const double k = (double)((key >> (21 * a)) & (MS_CELLS - 1));
        const double mean = (double)(long long)w[1 + a] / den;
        const double b = k + mean;
        const double d = g.o[a] + b * g.cell;                                  // contraction is off: a rounded product, a rounded sum
        cluster_vertices[3 * (size_t)c + a] = (float)d;
        if constexpr (COLOUR) cluster_colours[3 * (size_t)c + a] = (unsigned char)((2 * (long long)w[4 + a] + n) / (2 * n));
    }
}

__global__ __launch_bounds__(MS_THREADS) void ms_faces_kernel(const int* __restrict__ faces, long long M, long long F,
                                                               const int* __restrict__ vertex_cluster, int* __restrict__ cluster_faces,
                                                               long long* __restrict__ key_lo, long long* __restrict__ key_hi,
                                                               int* status) {
    int degenerates = 0;                                                       // of this thread: it strides over the faces
    for (long long f = (long long)blockIdx.x * MS_THREADS + threadIdx.x; f < F; f += (long long)gridDim.x * MS_THREADS) {
        const int a = faces[3 * (size_t)f], b = faces[3 * (size_t)f + 1], c = faces[3 * (size_t)f + 2];
        int ca = -1, cb = -1, cc = -1;
        if (a >= 0 && a < M && b >= 0 && b < M && c >= 0 && c < M) {
            ca = vertex_cluster[a];
            cb = vertex_cluster[b];
            cc = vertex_cluster[c];
        }
        const bool valid = ca >= 0 && cb >= 0 && cc >= 0 && ca < M && cb < M && cc < M;
        if (!valid) ca = cb = cc = -1;
        const bool degenerate = valid && (ca == cb || cb == cc || ca == cc);
        degenerates += degenerate ? 1 : 0;
        cluster_faces[3 * (size_t)f] = ca;
        cluster_faces[3 * (size_t)f + 1] = cb;
        cluster_faces[3 * (size_t)f + 2] = cc;
        long long lo = MS_DEAD, hi = MS_DEAD;
        if (valid && !degenerate) {
            const long long x = min(ca, min(cb, cc)), z = max(ca, max(cb, cc));
            const long long y = (long long)ca + cb + cc - x - z;
            if (key_hi) { hi = x; lo = (y << 32) | z; }
            else lo = (x << 42) | (y << 21) | z;                               // the launcher saw M <= 2^21
        }
        key_lo[f] = lo;
        if (key_hi) key_hi[f] = hi;
    }
    ms_block_count(degenerates, status + MS_DEGENERATE);
}

__device__ __forceinline__ bool ms_live(const int* __restrict__ cluster_faces, long long f, long long M, int* c) {
    c[0] = cluster_faces[3 * (size_t)f];
    c[1] = cluster_faces[3 * (size_t)f + 1];
    c[2] = cluster_faces[3 * (size_t)f + 2];
    return c[0] >= 0 && c[1] >= 0 && c[2] >= 0 && c[0] < M && c[1] < M && c[2] < M && c[0] != c[1] && c[1] != c[2] && c[0] != c[2];
}

__global__ __launch_bounds__(MS_THREADS) void ms_mark_kernel(const int* __restrict__ cluster_faces, long long M, long long F,
                                                              const long long* __restrict__ sorted_lo, const long long* __restrict__ sorted_hi,
                                                              const long long* __restrict__ order, int* __restrict__ face_keep,
                                                              int* __restrict__ vertex_keep, int* status) {
    const long long i = (long long)blockIdx.x * MS_THREADS + threadIdx.x;
    bool duplicate = false;
    if (i < F) {
        const long long f = order[i];
        if (f >= 0 && f < F) {                                                 // the order is the caller's
            int c[3];
            const bool live = ms_live(cluster_faces, f, M, c);
            const bool first = i == 0 || sorted_lo[i - 1] != sorted_lo[i] || (sorted_hi && sorted_hi[i - 1] != sorted_hi[i]);
            const bool keep = live && first;
            duplicate = live && !first;
            face_keep[f] = keep ? 1 : 0;
            if (keep) vertex_keep[c[0]] = vertex_keep[c[1]] = vertex_keep[c[2]] = 1;      // several writers, one value
        }
    }
    ms_block_count(duplicate ? 1 : 0, status + MS_DUPLICATE);
}

// [status words | used | sums]
struct MsLayout { size_t status, used, acc, total; };

MsLayout ms_layout(long long M) {
    GeoCarver c;
    const size_t m = (size_t)std::max(M, 1LL);
    return {c.take(MS_STATUS_WORDS * sizeof(int)), c.take(m * sizeof(int)), c.take(m * MS_ACC_WORDS * sizeof(unsigned long long)), c.off};
}

int ms_sizes(long long M, long long F) {
    if (M < 0 || F < 0) return MVS_E_BADARG;
    if (M > MS_MAX || F > MS_MAX) return MVS_E_SHAPE;
    return 0;
}

bool ms_grid(float ox, float oy, float oz, float cell, MsGrid* g) {
    if (!(__builtin_isfinite(ox) && __builtin_isfinite(oy) && __builtin_isfinite(oz) && __builtin_isfinite(cell) && cell > 0.f)) return false;
    *g = {{(double)ox, (double)oy, (double)oz}, (double)cell};
    return true;
}

}  // namespace

extern "C" size_t mvs_mesh_cluster_workspace_bytes(long long M, long long F) {
    if (ms_sizes(M, F) != 0) return 0;
    return ms_layout(M).total;
}

extern "C" int mvs_mesh_cluster_keys_f32(const float* vertices, long long M, const int* faces, long long F, float origin_x,
                                         float origin_y, float origin_z, float cell, long long* keys, int* offsets,
                                         void* workspace, size_t workspace_bytes, void* stream) {
    MVS_CHECK_ARG(workspace);
    if (int rc = ms_sizes(M, F)) return rc;
    MsGrid g;
    MVS_CHECK_ARG(ms_grid(origin_x, origin_y, origin_z, cell, &g));
    MVS_CHECK_ARG((M == 0 || (vertices && keys && offsets)) && (F == 0 || faces));
    const MsLayout L = ms_layout(M);
    if (workspace_bytes < L.total) return MVS_E_WORKSPACE;
    hipStream_t st = mvs_stream(stream);
    char* ws = static_cast<char*>(workspace);
    int* status = reinterpret_cast<int*>(ws + L.status);
    int* used = reinterpret_cast<int*>(ws + L.used);
    hipError_t e = hipMemsetAsync(status, 0, MS_STATUS_WORDS * sizeof(int), st);
    if (e != hipSuccess) return (int)e;
    if (M) {
        e = hipMemsetAsync(used, 0, (size_t)M * sizeof(int), st);
        if (e != hipSuccess) return (int)e;
    }
    const dim3 gm(mvs_cdiv(M, MS_THREADS)), gf(mvs_cdiv(F, MS_THREADS)), block(MS_THREADS);
    if (M) hipLaunchKernelGGL(ms_cell_kernel, gm, block, 0, st, vertices, M, g, keys, offsets, status);
    if (F) hipLaunchKernelGGL(ms_use_kernel, gf, block, 0, st, faces, M, F, keys, used, status);
    if (M) hipLaunchKernelGGL(ms_drop_kernel, gm, block, 0, st, used, M, keys);
    MVS_LAUNCH_RET();
}

extern "C" int mvs_mesh_cluster_heads_i64(const long long* sorted_keys, long long M, int* head, void* stream) {
    if (int rc = ms_sizes(M, 0)) return rc;
    MVS_CHECK_ARG(M == 0 || (sorted_keys && head));
    if (M == 0) return 0;
    hipLaunchKernelGGL(ms_heads_kernel, dim3(mvs_cdiv(M, MS_THREADS)), dim3(MS_THREADS), 0, mvs_stream(stream), sorted_keys, M, head);
    MVS_LAUNCH_RET();
}

extern "C" int mvs_mesh_cluster_sums_f32(const long long* sorted_keys, const long long* order, const int* head_rank,
                                         const int* offsets, const unsigned char* colours, long long M, float origin_x,
                                         float origin_y, float origin_z, float cell, int* vertex_cluster, float* cluster_vertices,
                                         unsigned char* cluster_colours, void* workspace, size_t workspace_bytes, void* stream) {
    MVS_CHECK_ARG(workspace);
    if (int rc = ms_sizes(M, 0)) return rc;
    MsGrid g;
    MVS_CHECK_ARG(ms_grid(origin_x, origin_y, origin_z, cell, &g));
    MVS_CHECK_ARG(M == 0 || (sorted_keys && order && head_rank && offsets && vertex_cluster && cluster_vertices));
    MVS_CHECK_ARG((colours == nullptr) == (cluster_colours == nullptr) || M == 0);
    const MsLayout L = ms_layout(M);
    if (workspace_bytes < L.total) return MVS_E_WORKSPACE;
    if (M == 0) return 0;
    hipStream_t st = mvs_stream(stream);
    unsigned long long* acc = reinterpret_cast<unsigned long long*>(static_cast<char*>(workspace) + L.acc);
    hipError_t e = hipMemsetAsync(acc, 0, (size_t)M * MS_ACC_WORDS * sizeof(unsigned long long), st);
    if (e != hipSuccess) return (int)e;
    const dim3 gm(mvs_cdiv(M, MS_THREADS)), block(MS_THREADS);
    if (colours) {
        hipLaunchKernelGGL(ms_sums_kernel<true>, gm, block, 0, st, sorted_keys, order, head_rank, offsets, colours, M, vertex_cluster, acc);
        hipLaunchKernelGGL(ms_finish_kernel<true>, gm, block, 0, st, acc, head_rank, M, g, cluster_vertices, cluster_colours);
    } else {
        hipLaunchKernelGGL(ms_sums_kernel<false>, gm, block, 0, st, sorted_keys, order, head_rank, offsets, colours, M, vertex_cluster, acc);
        hipLaunchKernelGGL(ms_finish_kernel<false>, gm, block, 0, st, acc, head_rank, M, g, cluster_vertices, cluster_colours);
    }
    MVS_LAUNCH_RET();
}

extern "C" int mvs_mesh_cluster_faces_i32(const int* faces, long long M, long long F, const int* vertex_cluster, int* cluster_faces,
                                          long long* key_lo, long long* key_hi, void* workspace, size_t workspace_bytes,
                                          void* stream) {
    MVS_CHECK_ARG(workspace);
    if (int rc = ms_sizes(M, F)) return rc;
    if (key_hi == nullptr && M > MS_CELLS) return MVS_E_SHAPE;                 // three cluster indices no longer fit one key
    MVS_CHECK_ARG((M == 0 || vertex_cluster) && (F == 0 || (faces && cluster_faces && key_lo)));
    const MsLayout L = ms_layout(M);
    if (workspace_bytes < L.total) return MVS_E_WORKSPACE;
    hipStream_t st = mvs_stream(stream);
    int* status = reinterpret_cast<int*>(static_cast<char*>(workspace) + L.status);
    hipError_t e = hipMemsetAsync(status + MS_DEGENERATE, 0, sizeof(int), st);
    if (e != hipSuccess) return (int)e;
    if (F) hipLaunchKernelGGL(ms_faces_kernel, dim3(std::min(mvs_cdiv(F, MS_THREADS), MS_MAX_BLOCKS)), dim3(MS_THREADS), 0, st, faces, M, F, vertex_cluster,
                              cluster_faces, key_lo, key_hi, status);
    MVS_LAUNCH_RET();
}

extern "C" int mvs_mesh_cluster_mark_i32(const int* cluster_faces, long long M, long long F, const long long* sorted_lo,
                                         const long long* sorted_hi, const long long* order, int* face_keep, int* vertex_keep,
                                         void* workspace, size_t workspace_bytes, void* stream) {
    MVS_CHECK_ARG(workspace);
    if (int rc = ms_sizes(M, F)) return rc;
    MVS_CHECK_ARG((M == 0 || vertex_keep) && (F == 0 || (cluster_faces && sorted_lo && order && face_keep)));
    const MsLayout L = ms_layout(M);
    if (workspace_bytes < L.total) return MVS_E_WORKSPACE;
    hipStream_t st = mvs_stream(stream);
    int* status = reinterpret_cast<int*>(static_cast<char*>(workspace) + L.status);
    hipError_t e = hipMemsetAsync(status + MS_DUPLICATE, 0, sizeof(int), st);
    if (e != hipSuccess) return (int)e;
    if (M) {
        e = hipMemsetAsync(vertex_keep, 0, (size_t)M * sizeof(int), st);
        if (e != hipSuccess) return (int)e;
    }
    if (F) hipLaunchKernelGGL(ms_mark_kernel, dim3(mvs_cdiv(F, MS_THREADS)), dim3(MS_THREADS), 0, st, cluster_faces, M, F, sorted_lo,
                              sorted_hi, order, face_keep, vertex_keep, status);
    MVS_LAUNCH_RET();
}
