// Taubin smoothing of a triangle mesh (mvs_mesh_smooth_edges_i64, mvs_mesh_smooth_heads_i64, mvs_mesh_smooth_rows_i32,
// mvs_mesh_smooth_step_f32).  The semantics are normative in mvsnet_amd/mesh_smooth.py; tests/mesh_smooth_reference.py restates
// them in numpy, and the kernels equal it byte for byte.  The caller (torch) owns the memory, the sort of the edge keys and the
// inclusive scan of the heads; the workspace holds the status words alone.
//
//   edges      one lane per vertex counts the vertices that are not finite; one lane per face: a face is valid when its three
//              indices lie in 0..M-1 (only then are its vertices read); a valid face stores its six directed edges
//              a>b b>a b>c c>b c>a a>c as int64(s) << 31 | t where s != t and both ends are finite, INT64_MAX otherwise; an
//              invalid face stores six times INT64_MAX;
//   heads      on the sorted keys: head[i] = 1 where a run of a live key starts.  A head whose successor differs is a boundary
//              edge, one whose second successor is equal a non-manifold edge; both are counted where s < t, which counts an
//              undirected edge once;
//   rows       entries: one lane per sorted position: the head of rank k (the caller's scan, minus one) stores
//              neighbours[k] = t | boundary << 31;
//              starts: one lane per vertex 0..M: row_start[v] = the scan before the lower bound of v << 31 in the sorted keys
//              (a binary search: at most 32 steps, no atomics);
//              classes: one lane per vertex walks its row once: 0 fixed, 1 curve, 2 interior;
//   step       one lane per vertex: a fixed vertex copies its row of X; every other walks its row of neighbours in order and
//              sums their positions in float64, one after the other, then m = s / n, d = m - x, e = f d, y = x + e, the clamp
//              to V0 +- r, float32(y); a result that is not finite keeps X[v] on all three axes.  Jacobi: X is read, Y written.
// Every index read from an array (faces, ranks, row bounds, targets) is compared with its range before it is used as an index.
#include "geom_common.h"

#pragma clang fp contract(off)

namespace {

constexpr int SM_THREADS = 256;
constexpr int SM_STATUS_WORDS = 64;                 // 256 bytes: the whole workspace
constexpr int SM_INVALID = 0, SM_NON_FINITE = 1, SM_BOUNDARY_EDGES = 2, SM_NON_MANIFOLD = 3, SM_BOUNDARY_VERTICES = 4, SM_FIXED = 5;
constexpr long long SM_MAX = 0x7fffffffLL;
constexpr long long SM_DEAD = 0x7fffffffffffffffLL;
constexpr int SM_FIXED_CLASS = 0, SM_CURVE_CLASS = 1, SM_INTERIOR_CLASS = 2;
constexpr int SM_MODE_FIXED = 0, SM_MODE_CURVE = 1, SM_MODE_FREE = 2;
constexpr unsigned SM_TARGET = 0x7fffffffu;         // bits 0..30 of a neighbours entry; bit 31: a boundary edge

__device__ __forceinline__ void sm_count(int mine, int* word) {
    __shared__ int sh[SM_THREADS / MVS_WAVE];
    const int total = geo_block_sum<SM_THREADS>(mine, sh);
    if (threadIdx.x == 0 && total) atomicAdd(word, total);
}

__device__ __forceinline__ bool sm_finite(const float* __restrict__ vertices, long long v) {
    const float* p = vertices + 3 * (size_t)v;
    return __builtin_isfinite(p[0]) && __builtin_isfinite(p[1]) && __builtin_isfinite(p[2]);
}

__global__ __launch_bounds__(SM_THREADS) void sm_finite_kernel(const float* __restrict__ vertices, long long M, int* status) {
    const long long v = (long long)blockIdx.x * SM_THREADS + threadIdx.x;
    sm_count(v < M && !sm_finite(vertices, v) ? 1 : 0, status + SM_NON_FINITE);
}

__device__ __forceinline__ long long sm_key(int s, int t, bool s_ok, bool t_ok) {
    return (s != t && s_ok && t_ok) ? (((long long)s << 31) | (long long)t) : SM_DEAD;
}

__global__ __launch_bounds__(SM_THREADS) void sm_edges_kernel(const float* __restrict__ vertices, long long M,
                                                               const int* __restrict__ faces, long long F,
                                                               long long* __restrict__ keys, int* status) {
    const long long f = (long long)blockIdx.x * SM_THREADS + threadIdx.x;
    bool invalid = false;
    if (f < F) {
        const int a = faces[3 * (size_t)f], b = faces[3 * (size_t)f + 1], c = faces[3 * (size_t)f + 2];
        const bool valid = a >= 0 && a < M && b >= 0 && b < M && c >= 0 && c < M;
        long long* k = keys + 6 * (size_t)f;
        if (valid) {
            const bool fa = sm_finite(vertices, a), fb = sm_finite(vertices, b), fc = sm_finite(vertices, c);
            k[0] = sm_key(a, b, fa, fb);
            k[1] = sm_key(b, a, fb, fa);
            k[2] = sm_key(b, c, fb, fc);
            k[3] = sm_key(c, b, fc, fb);
            k[4] = sm_key(c, a, fc, fa);
            k[5] = sm_key(a, c, fa, fc);
        } else {
#pragma unroll
            for (int e = 0; e < 6; ++e) k[e] = SM_DEAD;
        }
        invalid = !valid;
    }
    sm_count(invalid ? 1 : 0, status + SM_INVALID);
}

__device__ __forceinline__ bool sm_live(long long k) { return k >= 0 && k != SM_DEAD; }

__global__ __launch_bounds__(SM_THREADS) void sm_heads_kernel(const long long* __restrict__ sorted_keys, long long E,
                                                               int* __restrict__ head, int* status) {
    const long long i = (long long)blockIdx.x * SM_THREADS + threadIdx.x;
    int boundary = 0, non_manifold = 0;
    if (i < E) {
        const long long k = sorted_keys[i];
        const bool first = sm_live(k) && (i == 0 || sorted_keys[i - 1] != k);
        head[i] = first ? 1 : 0;
        if (first && (k >> 31) < (k & SM_MAX)) {                               // s < t: an undirected edge counts once
            boundary = (i + 1 == E || sorted_keys[i + 1] != k) ? 1 : 0;
            non_manifold = (i + 2 < E && sorted_keys[i + 2] == k) ? 1 : 0;
        }
    }
    __shared__ int sh[2][SM_THREADS / MVS_WAVE];
    const int nb = geo_block_sum<SM_THREADS>(boundary, sh[0]);
    const int nm = geo_block_sum<SM_THREADS>(non_manifold, sh[1]);
    if (threadIdx.x == 0) {
        if (nb) atomicAdd(status + SM_BOUNDARY_EDGES, nb);
        if (nm) atomicAdd(status + SM_NON_MANIFOLD, nm);
    }
}

__global__ __launch_bounds__(SM_THREADS) void sm_entries_kernel(const long long* __restrict__ sorted_keys,
                                                                 const int* __restrict__ head, const int* __restrict__ head_rank,
                                                                 long long M, long long E, int* __restrict__ neighbours) {
    const long long i = (long long)blockIdx.x * SM_THREADS + threadIdx.x;
    if (i >= E || head[i] != 1) return;
    const long long k = sorted_keys[i];
    const long long rank = (long long)head_rank[i] - 1;                        // the head and the ranks are the caller's
    if (!sm_live(k) || rank < 0 || rank >= E) return;
    const long long s = k >> 31, t = k & SM_MAX;
    if (s >= M || t >= M) return;
    const bool boundary = i + 1 == E || sorted_keys[i + 1] != k;
    neighbours[rank] = (int)((unsigned)t | (boundary ? 0x80000000u : 0u));
}

// row_start[v] for v = 0..M: the number of unique edges whose source is below v.
__global__ __launch_bounds__(SM_THREADS) void sm_starts_kernel(const long long* __restrict__ sorted_keys,
                                                                const int* __restrict__ head_rank, long long M, long long E,
                                                                int* __restrict__ row_start) {
    const long long v = (long long)blockIdx.x * SM_THREADS + threadIdx.x;
    if (v > M) return;
    const long long lo = geo_lower_bound(sorted_keys, E, v << 31);             // the first position whose key is >= v << 31
    row_start[v] = lo > 0 ? head_rank[lo - 1] : 0;
}

__global__ __launch_bounds__(SM_THREADS) void sm_class_kernel(const int* __restrict__ row_start, const int* __restrict__ neighbours,
                                                               long long M, long long E, int mode,
                                                               unsigned char* __restrict__ vertex_class, int* status) {
    const long long v = (long long)blockIdx.x * SM_THREADS + threadIdx.x;
    int on_boundary = 0, fixed = 0;
    if (v < M) {
        const long long a = row_start[v], b = row_start[v + 1];
        const bool rows_ok = a >= 0 && a <= b && b <= E;
        if (rows_ok) {
            for (long long e = a; e < b; ++e) on_boundary |= (unsigned)neighbours[e] >> 31;
        }
        int cls = SM_INTERIOR_CLASS;
        if (!rows_ok || a == b || (on_boundary && mode == SM_MODE_FIXED)) cls = SM_FIXED_CLASS;
        else if (on_boundary && mode == SM_MODE_CURVE) cls = SM_CURVE_CLASS;
        vertex_class[v] = (unsigned char)cls;
        fixed = cls == SM_FIXED_CLASS ? 1 : 0;
    }
    __shared__ int sh[2][SM_THREADS / MVS_WAVE];
    const int nb = geo_block_sum<SM_THREADS>(on_boundary, sh[0]);
    const int nf = geo_block_sum<SM_THREADS>(fixed, sh[1]);
    if (threadIdx.x == 0) {
        if (nb) atomicAdd(status + SM_BOUNDARY_VERTICES, nb);
        if (nf) atomicAdd(status + SM_FIXED, nf);
    }
}

// A position: ROW floats apart, three of them used.  ROW = 4 rows are 16-byte aligned and move as one float4, the fourth
// float travelling from X to Y as it is.
template <int ROW> struct SmRow;
template <> struct SmRow<3> {
    float x, y, z;
    __device__ __forceinline__ static SmRow load(const float* __restrict__ p, long long v) {
        const float* q = p + 3 * (size_t)v;
        return {q[0], q[1], q[2]};
    }
    __device__ __forceinline__ void store(float* __restrict__ p, long long v, float a, float b, float c) const {
        float* q = p + 3 * (size_t)v;
        q[0] = a; q[1] = b; q[2] = c;
    }
};
template <> struct SmRow<4> {
    float x, y, z, w;
    __device__ __forceinline__ static SmRow load(const float* __restrict__ p, long long v) {
        const float4 q = reinterpret_cast<const float4*>(p)[v];
        return {q.x, q.y, q.z, q.w};
    }
    __device__ __forceinline__ void store(float* __restrict__ p, long long v, float a, float b, float c) const {
        reinterpret_cast<float4*>(p)[v] = make_float4(a, b, c, w);
    }
};

__device__ __forceinline__ bool sm_move(double s, int n, float x, float x0, double f, double r, bool clamp, float* out) {
    const double m = s / (double)n;
    const double d = m - (double)x;
    const double e = f * d;
    double y = (double)x + e;
    if (clamp) {
        const double lo = (double)x0 - r, hi = (double)x0 + r;
        y = y < lo ? lo : y;
        y = y > hi ? hi : y;
    }
    *out = (float)y;
    return __builtin_isfinite(*out);
}

template <int ROW>
__global__ __launch_bounds__(SM_THREADS) void sm_step_kernel(const float* __restrict__ X, const float* __restrict__ V0,
                                                              const int* __restrict__ row_start, const int* __restrict__ neighbours,
                                                              const unsigned char* __restrict__ vertex_class, long long M,
                                                              long long N, double f, double r, bool clamp, float* __restrict__ Y) {
    const long long v = (long long)blockIdx.x * SM_THREADS + threadIdx.x;
    if (v >= M) return;
    const SmRow<ROW> x = SmRow<ROW>::load(X, v);
    float ox = x.x, oy = x.y, oz = x.z;
    const int cls = vertex_class[v];
    if (cls == SM_CURVE_CLASS || cls == SM_INTERIOR_CLASS) {
        const long long a = row_start[v], b = row_start[v + 1];
        if (a >= 0 && a <= b && b <= N) {
            double sx = 0.0, sy = 0.0, sz = 0.0;
            int n = 0;
            for (long long e = a; e < b; ++e) {
                const unsigned w = (unsigned)neighbours[e];
                const long long j = w & SM_TARGET;
                if ((cls == SM_CURVE_CLASS && !(w >> 31)) || j >= M) continue;
                const SmRow<ROW> p = SmRow<ROW>::load(X, j);
                sx += (double)p.x;
                sy += (double)p.y;
                sz += (double)p.z;
                ++n;
            }
            if (n > 0) {
                const SmRow<ROW> x0 = clamp ? SmRow<ROW>::load(V0, v) : x;
                float nx, ny, nz;
                const bool okx = sm_move(sx, n, x.x, x0.x, f, r, clamp, &nx);
                const bool oky = sm_move(sy, n, x.y, x0.y, f, r, clamp, &ny);
                const bool okz = sm_move(sz, n, x.z, x0.z, f, r, clamp, &nz);
                if (okx && oky && okz) { ox = nx; oy = ny; oz = nz; }
            }
        }
    }
    x.store(Y, v, ox, oy, oz);
}

int sm_sizes(long long M, long long F) {
    if (M < 0 || F < 0) return MVS_E_BADARG;
    if (M > SM_MAX || F > SM_MAX / 6) return MVS_E_SHAPE;
    return 0;
}

constexpr size_t SM_WORKSPACE = SM_STATUS_WORDS * sizeof(int);

// Clears `count` status words from `first` on.
hipError_t sm_clear(int* status, int first, int count, hipStream_t st) {
    return hipMemsetAsync(status + first, 0, count * sizeof(int), st);
}

}  // namespace

extern "C" size_t mvs_mesh_smooth_workspace_bytes(long long M, long long F) {
    if (sm_sizes(M, F) != 0) return 0;
    return SM_WORKSPACE;
}

extern "C" int mvs_mesh_smooth_edges_i64(const float* vertices, long long M, const int* faces, long long F, long long* keys,
                                         void* workspace, size_t workspace_bytes, void* stream) {
    MVS_CHECK_ARG(workspace);
    if (int rc = sm_sizes(M, F)) return rc;
    MVS_CHECK_ARG((M == 0 || vertices) && (F == 0 || (faces && keys)));
    if (workspace_bytes < SM_WORKSPACE) return MVS_E_WORKSPACE;
    hipStream_t st = mvs_stream(stream);
    int* status = static_cast<int*>(workspace);
    hipError_t e = sm_clear(status, 0, SM_STATUS_WORDS, st);
    if (e != hipSuccess) return (int)e;
    const dim3 block(SM_THREADS);
    if (M) hipLaunchKernelGGL(sm_finite_kernel, dim3(mvs_cdiv(M, SM_THREADS)), block, 0, st, vertices, M, status);
    if (F) hipLaunchKernelGGL(sm_edges_kernel, dim3(mvs_cdiv(F, SM_THREADS)), block, 0, st, vertices, M, faces, F, keys, status);
    MVS_LAUNCH_RET();
}

extern "C" int mvs_mesh_smooth_heads_i64(const long long* sorted_keys, long long F, int* head, void* workspace,
                                         size_t workspace_bytes, void* stream) {
    MVS_CHECK_ARG(workspace);
    if (int rc = sm_sizes(0, F)) return rc;
    MVS_CHECK_ARG(F == 0 || (sorted_keys && head));
    if (workspace_bytes < SM_WORKSPACE) return MVS_E_WORKSPACE;
    hipStream_t st = mvs_stream(stream);
    int* status = static_cast<int*>(workspace);
    hipError_t e = sm_clear(status, SM_BOUNDARY_EDGES, 2, st);
    if (e != hipSuccess) return (int)e;
    const long long E = 6 * F;
    if (E) hipLaunchKernelGGL(sm_heads_kernel, dim3(mvs_cdiv(E, SM_THREADS)), dim3(SM_THREADS), 0, st, sorted_keys, E, head, status);
    MVS_LAUNCH_RET();
}

extern "C" int mvs_mesh_smooth_rows_i32(const long long* sorted_keys, const int* head, const int* head_rank, long long M,
                                        long long F, int boundary, int* neighbours, int* row_start, unsigned char* vertex_class,
                                        void* workspace, size_t workspace_bytes, void* stream) {
    MVS_CHECK_ARG(workspace);
    if (int rc = sm_sizes(M, F)) return rc;
    MVS_CHECK_ARG(boundary == SM_MODE_FIXED || boundary == SM_MODE_CURVE || boundary == SM_MODE_FREE);
    MVS_CHECK_ARG((F == 0 || (sorted_keys && head && head_rank && neighbours)) && row_start && (M == 0 || vertex_class));
    if (workspace_bytes < SM_WORKSPACE) return MVS_E_WORKSPACE;
    hipStream_t st = mvs_stream(stream);
    int* status = static_cast<int*>(workspace);
    hipError_t e = sm_clear(status, SM_BOUNDARY_VERTICES, 2, st);
    if (e != hipSuccess) return (int)e;
    const long long E = 6 * F;
    const dim3 block(SM_THREADS);
    if (E) hipLaunchKernelGGL(sm_entries_kernel, dim3(mvs_cdiv(E, SM_THREADS)), block, 0, st, sorted_keys, head, head_rank, M, E, neighbours);
    hipLaunchKernelGGL(sm_starts_kernel, dim3(mvs_cdiv(M + 1, SM_THREADS)), block, 0, st, sorted_keys, head_rank, M, E, row_start);
    if (M) hipLaunchKernelGGL(sm_class_kernel, dim3(mvs_cdiv(M, SM_THREADS)), block, 0, st, row_start, neighbours, M, E, boundary, vertex_class, status);
    MVS_LAUNCH_RET();
}

extern "C" int mvs_mesh_smooth_step_f32(const float* X, const float* V0, const int* row_start, const int* neighbours,
                                        const unsigned char* vertex_class, long long M, long long N, int row_floats, float factor,
                                        float max_displacement, float* Y, void* stream) {
    if (M < 0 || N < 0) return MVS_E_BADARG;
    if (M > SM_MAX || N > SM_MAX) return MVS_E_SHAPE;
    MVS_CHECK_ARG(row_floats == 3 || row_floats == 4);
    MVS_CHECK_ARG(__builtin_isfinite(factor) && !__builtin_isnan(max_displacement) && max_displacement != __builtin_inff());
    MVS_CHECK_ARG(M == 0 || (X && V0 && row_start && vertex_class && Y && X != Y && (N == 0 || neighbours)));
    if (row_floats == 4) MVS_CHECK_ARG((((uintptr_t)X | (uintptr_t)V0 | (uintptr_t)Y) & 15) == 0);
    if (M == 0) return 0;
    const bool clamp = max_displacement >= 0.f;                                // negative: no bound
    const dim3 grid(mvs_cdiv(M, SM_THREADS)), block(SM_THREADS);
    hipStream_t st = mvs_stream(stream);
    if (row_floats == 3)
        hipLaunchKernelGGL(sm_step_kernel<3>, grid, block, 0, st, X, V0, row_start, neighbours, vertex_class, M, N, (double)factor,
                           (double)max_displacement, clamp, Y);
    else
        hipLaunchKernelGGL(sm_step_kernel<4>, grid, block, 0, st, X, V0, row_start, neighbours, vertex_class, M, N, (double)factor,
                           (double)max_displacement, clamp, Y);
    MVS_LAUNCH_RET();
}
