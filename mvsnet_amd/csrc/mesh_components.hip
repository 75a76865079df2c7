// Connected components of a triangle mesh, their face counts and bounding boxes, and the compaction of a selection of them
// (mvs_mesh_components_label_i32, mvs_mesh_components_measure_f32, mvs_mesh_compact_mark_i32, mvs_mesh_compact_write_f32).
// The semantics are normative in mvsnet_amd/mesh_clean.py; tests/mesh_clean_reference.py restates them in numpy, and the
// kernels equal it byte for byte (boxes by value).
//
//   init       parent[v] = v, root_min[v] = INT32_MAX;
//   link       one lane per face: the face is valid when its three indices lie in 0..M-1 and its nine coordinates are
//              finite; a valid face joins (a, b) and (b, c) by mesh_link.h's find-and-hook, whose roots are the vertices of
//              lowest rank (a fixed scramble of the index).  In this launch every read of parent is a relaxed agent-scope
//              atomic load and every write an agent-scope atomic (a compare-and-swap for a hook, an atomic store for a
//              shortening), so no argument about stale lines in an XCD's L2 or a CU's L1 is needed.  No lane waits for
//              another; a lane past MC_BUDGET walk steps and retries sets the error word and returns;
//   roots      vertex_labels[v] = root(v), by plain loads: parent is only read here, behind a kernel boundary; and
//              root_min[root] = the smallest v: the lanes of a wave run over ascending v, so the first lane of each root in
//              the wave holds the wave's minimum and issues the one atomic minimum;
//   faces      face_labels[f] = root_min[root of the first vertex], -1 for an invalid face;
//   labels     vertex_labels[v] = root_min[vertex_labels[v]]: the smallest vertex index of the component;
//   count      one lane per face, counts[label] += 1; box: one lane per vertex whose component has a face (counts[label] > 0,
//              which is the same as "a valid face names it"), six ordered-unsigned minima and maxima.  Both reduce before
//              they touch memory: the lanes of a wave that share the first remaining lane's label combine by cross-lane
//              operations, label after label; the first label of each wave goes through LDS, where the workgroup's waves
//              combine once more; then one atomic per (workgroup, label) and word.  Integer sums, minima and maxima: the
//              bytes do not depend on the order;
//   mark       face_keep[f] = keep_label[face_labels[f]] != 0, and plain stores of 1 to vertex_keep at its three vertices;
//   write      one lane per index: a kept vertex (and its colour) goes to vertex_rank - 1, a kept face to face_rank - 1 with
//              its indices replaced by vertex_rank - 1.  The two inclusive scans are the caller's.
#include "geom_common.h"

#define MC_HD __device__ __forceinline__
#include "mesh_link.h"

namespace {

constexpr int MC_THREADS = 256;
constexpr int MC_WAVES = MC_THREADS / MVS_WAVE;
constexpr int MC_STATUS_WORDS = 64;                 // 256 bytes at the start of the workspace: error, invalid, unreferenced
constexpr int MC_ERROR = 0, MC_INVALID = 1, MC_UNREFERENCED = 2;
// Walk steps plus retries one edge, or one root walk, may take.  Path halving keeps walks short (tens of steps on meshes of
// millions of faces); the cap only turns a mistake into an error word instead of a kernel that never ends.
constexpr int MC_BUDGET = 1 << 22;
constexpr long long MC_MAX = 0x7fffffffLL;

struct McDeviceOps {
    static __device__ __forceinline__ int load(int* p) { return __hip_atomic_load(p, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT); }
    static __device__ __forceinline__ void shorten(int* p, int v) {
        __hip_atomic_store(p, v, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
    }
    static __device__ __forceinline__ bool hook(int* p, int expected, int desired) {
        return __hip_atomic_compare_exchange_strong(p, &expected, desired, __ATOMIC_RELAXED, __ATOMIC_RELAXED,
                                                    __HIP_MEMORY_SCOPE_AGENT);
    }
};

__device__ __forceinline__ bool mc_finite3(const float* __restrict__ vertices, int v) {
    const float* p = vertices + 3 * (size_t)v;
    return __builtin_isfinite(p[0]) && __builtin_isfinite(p[1]) && __builtin_isfinite(p[2]);
}

// bits -> an unsigned word that orders as the float does (-0.0 just below +0.0)
__device__ __forceinline__ unsigned int mc_ordered(float x) {
    const unsigned int b = __float_as_uint(x);
    return (b & 0x80000000u) ? ~b : (b ^ 0x80000000u);
}

__global__ __launch_bounds__(MC_THREADS) void mc_init_kernel(int* __restrict__ parent, int* __restrict__ root_min, long long M) {
    const long long v = (long long)blockIdx.x * MC_THREADS + threadIdx.x;
    if (v >= M) return;
    parent[v] = (int)v;
    root_min[v] = 0x7fffffff;
}

__global__ __launch_bounds__(MC_THREADS) void mc_link_kernel(const float* __restrict__ vertices, long long M,
                                                              const int* __restrict__ faces, long long F, int* parent,
                                                              int* __restrict__ face_labels, int* status) {
    const long long f = (long long)blockIdx.x * MC_THREADS + threadIdx.x;
    bool invalid = false;
    if (f < F) {
        const int a = faces[3 * (size_t)f], b = faces[3 * (size_t)f + 1], c = faces[3 * (size_t)f + 2];
        bool valid = a >= 0 && a < M && b >= 0 && b < M && c >= 0 && c < M;
        valid = valid && mc_finite3(vertices, a) && mc_finite3(vertices, b) && mc_finite3(vertices, c);
        invalid = !valid;
        face_labels[f] = valid ? 0 : -1;                                        // the faces launch completes it
        if (valid && !(mc_link<McDeviceOps>(parent, a, b, MC_BUDGET) && mc_link<McDeviceOps>(parent, b, c, MC_BUDGET)))
            __hip_atomic_store(status + MC_ERROR, 1, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
    }
    const int n = __popcll(__ballot(invalid));
    if ((threadIdx.x & 63) == 0 && n) atomicAdd(status + MC_INVALID, n);
}

// vertex_labels[v] = root(v) for now, and root_min[root] = the smallest v under it.
__global__ __launch_bounds__(MC_THREADS) void mc_roots_kernel(const int* __restrict__ parent, long long M,
                                                               int* __restrict__ vertex_labels, int* __restrict__ root_min,
                                                               int* status) {
    const long long v = (long long)blockIdx.x * MC_THREADS + threadIdx.x;
    int r = -1;
    if (v < M) {
        r = (int)v;
        int steps = MC_BUDGET;
        for (int p = parent[r]; p != r; p = parent[r]) {
            r = p;
            if (--steps < 0) {
                __hip_atomic_store(status + MC_ERROR, 1, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
                break;
            }
        }
        vertex_labels[v] = r;
    }
    // lanes hold ascending v: the first lane of each root in the wave has the wave's smallest v of that root
    const int lane = threadIdx.x & 63;
    unsigned long long todo = __ballot(r >= 0);
    while (todo) {                                                             // wave-uniform
        const int leader = __ffsll((long long)todo) - 1;
        const int R = __shfl(r, leader, 64);
        if (lane == leader) atomicMin(root_min + R, (int)v);
        todo &= ~__ballot(r == R);
    }
}

__global__ __launch_bounds__(MC_THREADS) void mc_face_labels_kernel(const int* __restrict__ faces, long long F,
                                                                     const int* __restrict__ vertex_roots,
                                                                     const int* __restrict__ root_min,
                                                                     int* __restrict__ face_labels) {
    const long long f = (long long)blockIdx.x * MC_THREADS + threadIdx.x;
    if (f >= F) return;
    if (face_labels[f] >= 0) face_labels[f] = root_min[vertex_roots[faces[3 * (size_t)f]]];   // valid: link checked the index
}

__global__ __launch_bounds__(MC_THREADS) void mc_vertex_labels_kernel(const int* __restrict__ root_min, long long M,
                                                                       int* __restrict__ vertex_labels) {
    const long long v = (long long)blockIdx.x * MC_THREADS + threadIdx.x;
    if (v < M) vertex_labels[v] = root_min[vertex_labels[v]];
}

// ------------------------------------------------------------------------------------------------ measures

__global__ __launch_bounds__(MC_THREADS) void mc_measure_init_kernel(int* __restrict__ counts, unsigned int* __restrict__ boxes,
                                                                      long long M, int* status) {
    const long long v = (long long)blockIdx.x * MC_THREADS + threadIdx.x;
    if (v == 0) status[MC_UNREFERENCED] = 0;
    if (v >= M) return;
    counts[v] = 0;
    unsigned int* b = boxes + 6 * (size_t)v;
    b[0] = b[1] = b[2] = 0xffffffffu;
    b[3] = b[4] = b[5] = 0u;
}

// Sums n over the lanes of a wave that share a label (label < 0: the lane has nothing) and adds each sum to counts[label]
// with one atomic.  With SLOT, the first label's sum goes to *slot_label, *slot_n instead (slot_label -1: the wave had none).
// Every lane of the wave calls it.
template <bool SLOT>
__device__ __forceinline__ void mc_reduce_count(int label, int n, int* __restrict__ counts, int* slot_label, int* slot_n) {
    const int lane = threadIdx.x & 63;
    unsigned long long todo = __ballot(label >= 0);
    bool first = SLOT;
    if (SLOT && todo == 0 && lane == 0) *slot_label = -1;
    while (todo) {                                                             // wave-uniform
        const int leader = __ffsll((long long)todo) - 1;
        const int L = __shfl(label, leader, 64);
        const bool mine = label == L;
        int s = mine ? n : 0;
#pragma unroll
        for (int o = 32; o > 0; o >>= 1) s += __shfl_xor(s, o, 64);
        if (lane == leader) {
            if (first) { *slot_label = L; *slot_n = s; }
            else atomicAdd(counts + L, s);
        }
        first = false;
        todo &= ~__ballot(mine);
    }
}

__global__ __launch_bounds__(MC_THREADS) void mc_count_kernel(const int* __restrict__ face_labels, long long M, long long F,
                                                               int* __restrict__ counts) {
    const long long f = (long long)blockIdx.x * MC_THREADS + threadIdx.x;
    int label = f < F ? face_labels[f] : -1;
    if (label >= M) label = -1;                                                // the labels are the caller's: never outside counts
#ifdef MC_NO_WAVE_REDUCE                                                       // measurement build: a lane, an atomic
    if (label >= 0) atomicAdd(counts + label, 1);
#else
    __shared__ int s_label[MC_WAVES], s_n[MC_WAVES];
    const int wave = threadIdx.x >> 6;
    mc_reduce_count<true>(label, 1, counts, s_label + wave, s_n + wave);
    __syncthreads();
    if (wave == 0) {
        const bool have = threadIdx.x < MC_WAVES;
        mc_reduce_count<false>(have ? s_label[have ? threadIdx.x : 0] : -1, have ? s_n[threadIdx.x] : 0, counts, nullptr, nullptr);
    }
#endif
}

struct McBox { unsigned int lo[3], hi[3]; };

__device__ __forceinline__ void mc_box_atomics(unsigned int* __restrict__ boxes, int L, const McBox& b) {
    unsigned int* d = boxes + 6 * (size_t)L;
#pragma unroll
    for (int a = 0; a < 3; ++a) {
        atomicMin(d + a, b.lo[a]);
        atomicMax(d + 3 + a, b.hi[a]);
    }
}

// mc_reduce_count for boxes: minima and maxima over the lanes of a wave that share a label.
template <bool SLOT>
__device__ __forceinline__ void mc_reduce_box(int label, const McBox& mine_box, unsigned int* __restrict__ boxes, int* slot_label,
                                              McBox* slot_box) {
    const int lane = threadIdx.x & 63;
    unsigned long long todo = __ballot(label >= 0);
    bool first = SLOT;
    if (SLOT && todo == 0 && lane == 0) *slot_label = -1;
    while (todo) {
        const int leader = __ffsll((long long)todo) - 1;
        const int L = __shfl(label, leader, 64);
        const bool mine = label == L;
        McBox r;
#pragma unroll
        for (int a = 0; a < 3; ++a) {
            r.lo[a] = mine ? mine_box.lo[a] : 0xffffffffu;
            r.hi[a] = mine ? mine_box.hi[a] : 0u;
#pragma unroll
            for (int o = 32; o > 0; o >>= 1) {
                r.lo[a] = min(r.lo[a], (unsigned int)__shfl_xor((int)r.lo[a], o, 64));
                r.hi[a] = max(r.hi[a], (unsigned int)__shfl_xor((int)r.hi[a], o, 64));
            }
        }
        if (lane == leader) {
            if (first) { *slot_label = L; *slot_box = r; }
            else mc_box_atomics(boxes, L, r);
        }
        first = false;
        todo &= ~__ballot(mine);
    }
}

__global__ __launch_bounds__(MC_THREADS) void mc_box_kernel(const float* __restrict__ vertices, long long M,
                                                             const int* __restrict__ vertex_labels, const int* __restrict__ counts,
                                                             unsigned int* __restrict__ boxes, int* status) {
    const long long v = (long long)blockIdx.x * MC_THREADS + threadIdx.x;
    int label = -1;
    bool unreferenced = false;
    McBox b;
#pragma unroll
    for (int a = 0; a < 3; ++a) { b.lo[a] = 0xffffffffu; b.hi[a] = 0u; }
    if (v < M) {
        const int L = vertex_labels[v];
        if (L >= 0 && L < M && counts[L] > 0) {                                // its component has a face: a valid face names v
            label = L;
#pragma unroll
            for (int a = 0; a < 3; ++a) b.lo[a] = b.hi[a] = mc_ordered(vertices[3 * (size_t)v + a]);
        } else {
            unreferenced = true;
        }
    }
    const int n = __popcll(__ballot(unreferenced));
    if ((threadIdx.x & 63) == 0 && n) atomicAdd(status + MC_UNREFERENCED, n);
#ifdef MC_NO_WAVE_REDUCE
    if (label >= 0) mc_box_atomics(boxes, label, b);
#else
    __shared__ int s_label[MC_WAVES];
    __shared__ McBox s_box[MC_WAVES];
    const int wave = threadIdx.x >> 6;
    mc_reduce_box<true>(label, b, boxes, s_label + wave, s_box + wave);
    __syncthreads();
    if (wave == 0) {
        const bool have = threadIdx.x < MC_WAVES;
        const int slot = have ? threadIdx.x : 0;
        mc_reduce_box<false>(have ? s_label[slot] : -1, s_box[slot], boxes, nullptr, nullptr);
    }
#endif
}

// ------------------------------------------------------------------------------------------------ compaction

__global__ __launch_bounds__(MC_THREADS) void mc_mark_kernel(const int* __restrict__ faces, long long M, long long F,
                                                              const int* __restrict__ face_labels, const int* __restrict__ keep_label,
                                                              int* __restrict__ face_keep, int* __restrict__ vertex_keep) {
    const long long f = (long long)blockIdx.x * MC_THREADS + threadIdx.x;
    if (f >= F) return;
    const int L = face_labels[f];
    const int a = faces[3 * (size_t)f], b = faces[3 * (size_t)f + 1], c = faces[3 * (size_t)f + 2];
    // a labelled face is valid, so its indices are inside; they are checked again because the labels are the caller's
    const bool keep = L >= 0 && L < M && keep_label[L] != 0 && a >= 0 && a < M && b >= 0 && b < M && c >= 0 && c < M;
    face_keep[f] = keep ? 1 : 0;
    if (keep) vertex_keep[a] = vertex_keep[b] = vertex_keep[c] = 1;            // several writers, one value
}

template <bool COLOUR>
__global__ __launch_bounds__(MC_THREADS) void mc_write_kernel(const float* __restrict__ vertices, const unsigned char* __restrict__ colours,
                                                               long long M, const int* __restrict__ faces, long long F,
                                                               const int* __restrict__ face_keep, const int* __restrict__ face_rank,
                                                               const int* __restrict__ vertex_keep, const int* __restrict__ vertex_rank,
                                                               long long M_out, long long F_out, float* __restrict__ out_vertices,
                                                               unsigned char* __restrict__ out_colours, int* __restrict__ out_faces) {
    const long long i = (long long)blockIdx.x * MC_THREADS + threadIdx.x;
    if (i < M && vertex_keep[i]) {
        const long long id = (long long)vertex_rank[i] - 1;
        if (id >= 0 && id < M_out) {
#pragma unroll
            for (int a = 0; a < 3; ++a) {
                out_vertices[3 * (size_t)id + a] = vertices[3 * (size_t)i + a];
                if constexpr (COLOUR) out_colours[3 * (size_t)id + a] = colours[3 * (size_t)i + a];
            }
        }
    }
    if (i < F && face_keep[i]) {
        const long long id = (long long)face_rank[i] - 1;
        if (id >= 0 && id < F_out) {
#pragma unroll
            for (int a = 0; a < 3; ++a) {
                const int v = faces[3 * (size_t)i + a];
                out_faces[3 * (size_t)id + a] = (v >= 0 && v < M) ? vertex_rank[v] - 1 : -1;
            }
        }
    }
}

// [status words | parent | root_min]
struct McLayout { size_t status, parent, root_min, total; };

McLayout mc_layout(long long M) {
    GeoCarver c;
    const size_t ints = (size_t)std::max(M, 1LL) * sizeof(int);
    return {c.take(MC_STATUS_WORDS * sizeof(int)), c.take(ints), c.take(ints), c.off};
}

int mc_sizes(long long M, long long F) {
    if (M < 0 || F < 0) return MVS_E_BADARG;
    if (M > MC_MAX || F > MC_MAX) return MVS_E_SHAPE;
    return 0;
}

}  // namespace

extern "C" size_t mvs_mesh_components_workspace_bytes(long long M, long long F) {
    if (mc_sizes(M, F) != 0) return 0;
    return mc_layout(M).total;
}

extern "C" int mvs_mesh_components_label_i32(const float* vertices, long long M, const int* faces, long long F, int* vertex_labels,
                                             int* face_labels, void* workspace, size_t workspace_bytes, void* stream) {
    MVS_CHECK_ARG(workspace);
    if (int rc = mc_sizes(M, F)) return rc;
    MVS_CHECK_ARG((M == 0 || (vertices && vertex_labels)) && (F == 0 || (faces && face_labels)));
    const McLayout L = mc_layout(M);
    if (workspace_bytes < L.total) return MVS_E_WORKSPACE;
    hipStream_t st = mvs_stream(stream);
    char* ws = static_cast<char*>(workspace);
    int* status = reinterpret_cast<int*>(ws + L.status);
    int* parent = reinterpret_cast<int*>(ws + L.parent);
    int* root_min = reinterpret_cast<int*>(ws + L.root_min);
    hipError_t e = hipMemsetAsync(status, 0, MC_STATUS_WORDS * sizeof(int), st);
    if (e != hipSuccess) return (int)e;
    const dim3 gm(mvs_cdiv(M, MC_THREADS)), gf(mvs_cdiv(F, MC_THREADS)), block(MC_THREADS);
    if (M) hipLaunchKernelGGL(mc_init_kernel, gm, block, 0, st, parent, root_min, M);
    if (F) hipLaunchKernelGGL(mc_link_kernel, gf, block, 0, st, vertices, M, faces, F, parent, face_labels, status);
    if (M) hipLaunchKernelGGL(mc_roots_kernel, gm, block, 0, st, parent, M, vertex_labels, root_min, status);
    if (F) hipLaunchKernelGGL(mc_face_labels_kernel, gf, block, 0, st, faces, F, vertex_labels, root_min, face_labels);
    if (M) hipLaunchKernelGGL(mc_vertex_labels_kernel, gm, block, 0, st, root_min, M, vertex_labels);
    MVS_LAUNCH_RET();
}

extern "C" int mvs_mesh_components_measure_f32(const float* vertices, long long M, long long F, const int* vertex_labels,
                                               const int* face_labels, int* counts, unsigned int* boxes, void* workspace,
                                               size_t workspace_bytes, void* stream) {
    MVS_CHECK_ARG(workspace);
    if (int rc = mc_sizes(M, F)) return rc;
    MVS_CHECK_ARG((M == 0 || (vertices && vertex_labels && counts && boxes)) && (F == 0 || face_labels));
    const McLayout L = mc_layout(M);
    if (workspace_bytes < L.total) return MVS_E_WORKSPACE;
    hipStream_t st = mvs_stream(stream);
    int* status = reinterpret_cast<int*>(static_cast<char*>(workspace) + L.status);
    const dim3 gm(mvs_cdiv(std::max(M, 1LL), MC_THREADS)), gf(mvs_cdiv(F, MC_THREADS)), block(MC_THREADS);
    hipLaunchKernelGGL(mc_measure_init_kernel, gm, block, 0, st, counts, boxes, M, status);
    if (M && F) hipLaunchKernelGGL(mc_count_kernel, gf, block, 0, st, face_labels, M, F, counts);
    if (M) hipLaunchKernelGGL(mc_box_kernel, gm, block, 0, st, vertices, M, vertex_labels, counts, boxes, status);
    MVS_LAUNCH_RET();
}

extern "C" int mvs_mesh_compact_mark_i32(const int* faces, long long M, long long F, const int* face_labels, const int* keep_label,
                                         int* face_keep, int* vertex_keep, void* stream) {
    if (int rc = mc_sizes(M, F)) return rc;
    MVS_CHECK_ARG((M == 0 || (keep_label && vertex_keep)) && (F == 0 || (faces && face_labels && face_keep)));
    hipStream_t st = mvs_stream(stream);
    if (M) {
        hipError_t e = hipMemsetAsync(vertex_keep, 0, (size_t)M * sizeof(int), st);
        if (e != hipSuccess) return (int)e;
    }
    if (F) hipLaunchKernelGGL(mc_mark_kernel, dim3(mvs_cdiv(F, MC_THREADS)), dim3(MC_THREADS), 0, st, faces, M, F, face_labels, keep_label,
                              face_keep, vertex_keep);
    MVS_LAUNCH_RET();
}

extern "C" int mvs_mesh_compact_write_f32(const float* vertices, const unsigned char* colours, long long M, const int* faces,
                                          long long F, const int* face_keep, const int* face_rank, const int* vertex_keep,
                                          const int* vertex_rank, long long M_out, long long F_out, float* out_vertices,
                                          unsigned char* out_colours, int* out_faces, void* stream) {
    if (int rc = mc_sizes(M, F)) return rc;
    MVS_CHECK_ARG(M_out >= 0 && M_out <= M && F_out >= 0 && F_out <= F);
    MVS_CHECK_ARG((colours == nullptr) == (out_colours == nullptr) || M_out == 0);
    MVS_CHECK_ARG((M == 0 || (vertices && vertex_keep && vertex_rank)) && (F == 0 || (faces && face_keep && face_rank)));
    MVS_CHECK_ARG((M_out == 0 || out_vertices) && (F_out == 0 || out_faces));
    if (M_out == 0) return 0;                                                  // no vertex, so no face either
    hipStream_t st = mvs_stream(stream);
    const dim3 grid(mvs_cdiv(std::max(M, F), MC_THREADS)), block(MC_THREADS);
    if (colours && out_colours)
        hipLaunchKernelGGL(mc_write_kernel<true>, grid, block, 0, st, vertices, colours, M, faces, F, face_keep, face_rank, vertex_keep,
                           vertex_rank, M_out, F_out, out_vertices, out_colours, out_faces);
    else
        hipLaunchKernelGGL(mc_write_kernel<false>, grid, block, 0, st, vertices, colours, M, faces, F, face_keep, face_rank,
                           vertex_keep, vertex_rank, M_out, F_out, out_vertices, out_colours, out_faces);
    MVS_LAUNCH_RET();
}
