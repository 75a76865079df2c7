// Vertex normals and per-vertex colour from the full-resolution images (mvs_mesh_normals_keys_i64, mvs_mesh_normals_f32,
// mvs_mesh_colour_accumulate_f32, mvs_mesh_colour_finish_u8).  The semantics are normative in mvsnet_amd/mesh_colour.py;
// tests/mesh_colour_reference.py restates them in numpy, and the kernels equal it byte for byte.  The caller (torch) owns the
// memory, the sort of the incidence keys and the depth maps of the rasteriser; the workspace holds the status words alone.
//
//   keys        one lane per face: a face is valid when its three indices lie in 0..M-1 (only then are its vertices read), are
//               pairwise different and its nine coordinates are finite; a valid face stores int64(vertex) << 31 | f for its three
//               corners, an invalid one three times INT64_MAX;
//   normals     one lane per vertex: two lower-bound searches in the sorted keys bound its run of faces, ascending; the face
//               normals (b - a) x (c - a) are summed in float64 one after the other and the sum is normalised;
//   accumulate  one lane per vertex loops over the views of the call: the projection rows and the camera centre of a view are
//               the same in every lane and come through the scalar unit; the lane tests the vertex against the rasterised depth
//               map, weights the view by the cosine between its normal and the ray to the camera, and takes a bilinear sample
//               of the uint8 image.  The four sums of the vertex stay in registers over the views: acc and seen are read once
//               and written once, and only by the vertex's own lane, so there are no atomics and the order is the views';
//   finish      one lane per vertex: the weighted mean, rounded to a byte, or the input colour where nothing was seen.
// Every index read from an array (faces, the face of a key) is compared with its range before it is used as an index; the
// pixel of a vertex is compared with the image in float32 before it is converted.
#include "geom_common.h"

#pragma clang fp contract(off)

namespace {

constexpr int MC_THREADS = 256;
constexpr int MC_STATUS_WORDS = 64;                 // 256 bytes: the whole workspace
constexpr int MC_INVALID = 0, MC_ZERO_NORMALS = 1, MC_UNSEEN = 2;
constexpr long long MC_MAX = 0x7fffffffLL;
constexpr long long MC_DEAD = 0x7fffffffffffffffLL;
constexpr int MC_MAX_AXIS = 1 << 20;
constexpr int MC_MAX_POWER = 8;
constexpr size_t MC_WORKSPACE = MC_STATUS_WORDS * sizeof(int);

__device__ __forceinline__ void mc_count(int mine, int* word) {
    __shared__ int sh[MC_THREADS / MVS_WAVE];
    const int total = geo_block_sum<MC_THREADS>(mine, sh);
    if (threadIdx.x == 0 && total) atomicAdd(word, total);
}

__device__ __forceinline__ bool mc_finite(const float* __restrict__ vertices, long long v) {
    const float* p = vertices + 3 * (size_t)v;
    return __builtin_isfinite(p[0]) && __builtin_isfinite(p[1]) && __builtin_isfinite(p[2]);
}

__global__ __launch_bounds__(MC_THREADS) void mc_keys_kernel(const float* __restrict__ vertices, long long M,
                                                              const int* __restrict__ faces, long long F,
                                                              long long* __restrict__ keys, int* status) {
    const long long f = (long long)blockIdx.x * MC_THREADS + threadIdx.x;
    bool invalid = false;
    if (f < F) {
        const int a = faces[3 * (size_t)f], b = faces[3 * (size_t)f + 1], c = faces[3 * (size_t)f + 2];
        bool valid = a >= 0 && a < M && b >= 0 && b < M && c >= 0 && c < M && a != b && b != c && c != a;
        if (valid) valid = mc_finite(vertices, a) && mc_finite(vertices, b) && mc_finite(vertices, c);
        long long* k = keys + 3 * (size_t)f;
        k[0] = valid ? (((long long)a << 31) | f) : MC_DEAD;
        k[1] = valid ? (((long long)b << 31) | f) : MC_DEAD;
        k[2] = valid ? (((long long)c << 31) | f) : MC_DEAD;
        invalid = !valid;
    }
    mc_count(invalid ? 1 : 0, status + MC_INVALID);
}

__global__ __launch_bounds__(MC_THREADS) void mc_normals_kernel(const float* __restrict__ vertices, long long M,
                                                                 const int* __restrict__ faces, long long F,
                                                                 const long long* __restrict__ sorted_keys,
                                                                 float* __restrict__ normals, int* status) {
    const long long v = (long long)blockIdx.x * MC_THREADS + threadIdx.x;
    int zero = 0;
    if (v < M) {
        const long long E = 3 * F;
        const long long first = geo_lower_bound(sorted_keys, E, v << 31), last = geo_lower_bound(sorted_keys, E, (v + 1) << 31);
        double sx = 0.0, sy = 0.0, sz = 0.0;
        for (long long e = first; e < last; ++e) {
            const long long f = sorted_keys[e] & MC_MAX;
            if (f >= F) continue;
            const int a = faces[3 * (size_t)f], b = faces[3 * (size_t)f + 1], c = faces[3 * (size_t)f + 2];
            if (a < 0 || a >= M || b < 0 || b >= M || c < 0 || c >= M) continue;
            const float *pa = vertices + 3 * (size_t)a, *pb = vertices + 3 * (size_t)b, *pc = vertices + 3 * (size_t)c;
            const double ax = pa[0], ay = pa[1], az = pa[2];
            const double ux = (double)pb[0] - ax, uy = (double)pb[1] - ay, uz = (double)pb[2] - az;
            const double wx = (double)pc[0] - ax, wy = (double)pc[1] - ay, wz = (double)pc[2] - az;
            sx += uy * wz - uz * wy;
            sy += uz * wx - ux * wz;
            sz += ux * wy - uy * wx;
        }
        const double len = sqrt((sx * sx + sy * sy) + sz * sz);
        float nx = 0.f, ny = 0.f, nz = 0.f;
        if (first < last && len > 0.0 && __builtin_isfinite(len)) {
            nx = (float)(sx / len);
            ny = (float)(sy / len);
            nz = (float)(sz / len);
        } else {
            zero = 1;
        }
        float* n = normals + 3 * (size_t)v;
        n[0] = nx; n[1] = ny; n[2] = nz;
    }
    mc_count(zero, status + MC_ZERO_NORMALS);
}

// (1 - t) a + t b in float32, every product and sum rounded; `s` is 1 - t.
__device__ __forceinline__ float mc_mix(float s, float t, float a, float b) { return s * a + t * b; }

__global__ __launch_bounds__(MC_THREADS) void mc_accumulate_kernel(const float* __restrict__ vertices, const float* __restrict__ normals,
                                                                    long long M, const float* __restrict__ proj,
                                                                    const float* __restrict__ centres, int V, int H, int W,
                                                                    const float* __restrict__ depth,
                                                                    const unsigned char* __restrict__ images, float min_depth,
                                                                    float ratio, float min_cos, int power,
                                                                    double* __restrict__ acc, int* __restrict__ seen) {
    const long long j = (long long)blockIdx.x * MC_THREADS + threadIdx.x;
    if (j >= M) return;
    const float x = vertices[3 * (size_t)j], y = vertices[3 * (size_t)j + 1], z = vertices[3 * (size_t)j + 2];
    const float nx = normals[3 * (size_t)j], ny = normals[3 * (size_t)j + 1], nz = normals[3 * (size_t)j + 2];
    if (!(__builtin_isfinite(x) && __builtin_isfinite(y) && __builtin_isfinite(z)) || (nx == 0.f && ny == 0.f && nz == 0.f)) return;
    const float wmax = (float)(W - 1), hmax = (float)(H - 1);
    const double cut = (double)min_cos;
    // The sums start from the stored ones, so that a later call continues an earlier one in the order one call over all views
    // has: acc is read here and written below, once each (rows of 32 bytes: two 16-byte moves).
    double2* row = reinterpret_cast<double2*>(acc + 4 * (size_t)j);
    const double2 lo = row[0], hi = row[1];
    double s0 = lo.x, s1 = lo.y, s2 = hi.x, sg = hi.y;
    int count = 0;
    for (int v = 0; v < V; ++v) {
        geo_cfloat* P = (geo_cfloat*)proj + 12 * (size_t)v;                    // the constant space: scalar loads, once per view
        geo_cfloat* C = (geo_cfloat*)centres + 3 * (size_t)v;
        const float w = geo_row(P + 8, x, y, z);
        if (!(__builtin_isfinite(w) && w > min_depth)) continue;
        const float sx = __fdiv_rn(geo_row(P, x, y, z), w), sy = __fdiv_rn(geo_row(P + 4, x, y, z), w);
        if (!(__builtin_isfinite(sx) && __builtin_isfinite(sy))) continue;
        const float px = floorf(sx + 0.5f), py = floorf(sy + 0.5f);
        if (!GEO_INSIDE(px, py, wmax, hmax)) continue;                         // in float32, before any conversion
        const float zb = depth[((size_t)v * H + (size_t)(int)py) * W + (size_t)(int)px];
        if (!(zb > 0.f)) continue;
        const float reach = zb * ratio;
        if (!(w <= reach)) continue;
        const double dx = (double)C[0] - (double)x, dy = (double)C[1] - (double)y, dz = (double)C[2] - (double)z;
        const double q = (dx * dx + dy * dy) + dz * dz;
        if (!(q > 0.0)) continue;
        const double c = (((double)nx * dx + (double)ny * dy) + (double)nz * dz) / sqrt(q);
        if (!(c >= cut)) continue;
        double g = 1.0;
        if (power > 0) {
            g = c;
            for (int k = 1; k < power; ++k) g = g * c;
        }
        // the bilinear sample: px, py inside the image bound floor(sx), floor(sy) to -1 .. W-1, -1 .. H-1
        const float x0 = floorf(sx), y0 = floorf(sy);
        const float fx = sx - x0, fy = sy - y0, gx = 1.f - fx, gy = 1.f - fy;
        const int xa = (int)fminf(fmaxf(x0, 0.f), wmax), xb = (int)fminf(fmaxf(x0 + 1.f, 0.f), wmax);
        const int ya = (int)fminf(fmaxf(y0, 0.f), hmax), yb = (int)fminf(fmaxf(y0 + 1.f, 0.f), hmax);
        const unsigned char* top = images + (((size_t)v * H + (size_t)ya) * W) * 3;         // byte offsets in 64 bits
        const unsigned char* bot = images + (((size_t)v * H + (size_t)yb) * W) * 3;
        const size_t oa = 3 * (size_t)xa, ob = 3 * (size_t)xb;
        float s[3];
#pragma unroll
        for (int k = 0; k < 3; ++k) {
            const float t = mc_mix(gx, fx, (float)top[oa + k], (float)top[ob + k]);
            const float b = mc_mix(gx, fx, (float)bot[oa + k], (float)bot[ob + k]);
            s[k] = mc_mix(gy, fy, t, b);
        }
        s0 += g * (double)s[0];
        s1 += g * (double)s[1];
        s2 += g * (double)s[2];
        sg += g;
        ++count;
    }
    if (count == 0) return;                                                    // nothing was added: the sums stay as they are
    row[0] = make_double2(s0, s1);
    row[1] = make_double2(s2, sg);
    seen[j] += count;
}

__device__ __forceinline__ unsigned char mc_byte(double sum, double weight) {
    const double r = floor(sum / weight + 0.5);
    return (unsigned char)(r >= 255.0 ? 255 : r >= 0.0 ? (int)r : 0);         // a NaN gives 0
}

__global__ __launch_bounds__(MC_THREADS) void mc_finish_kernel(const unsigned char* __restrict__ colours, const double* __restrict__ acc,
                                                                const int* __restrict__ seen, long long M,
                                                                unsigned char* __restrict__ out, int* status) {
    const long long j = (long long)blockIdx.x * MC_THREADS + threadIdx.x;
    int unseen = 0;
    if (j < M) {
        const double* a = acc + 4 * (size_t)j;
        const double weight = a[3];
        unsigned char* o = out + 3 * (size_t)j;
        if (seen[j] > 0 && weight > 0.0) {
            o[0] = mc_byte(a[0], weight);
            o[1] = mc_byte(a[1], weight);
            o[2] = mc_byte(a[2], weight);
        } else {
            const unsigned char* c = colours + 3 * (size_t)j;
            o[0] = colours ? c[0] : 0;
            o[1] = colours ? c[1] : 0;
            o[2] = colours ? c[2] : 0;
            unseen = 1;
        }
    }
    mc_count(unseen, status + MC_UNSEEN);
}

int mc_sizes(long long M, long long F) {
    if (M < 0 || F < 0) return MVS_E_BADARG;
    if (M > MC_MAX || F > MC_MAX / 3) return MVS_E_SHAPE;
    return 0;
}

}  // namespace

extern "C" size_t mvs_mesh_colour_workspace_bytes(long long M, long long F) {
    if (mc_sizes(M, F) != 0) return 0;
    return MC_WORKSPACE;
}

extern "C" int mvs_mesh_normals_keys_i64(const float* vertices, long long M, const int* faces, long long F, long long* keys,
                                         void* workspace, size_t workspace_bytes, void* stream) {
    MVS_CHECK_ARG(workspace);
    if (int rc = mc_sizes(M, F)) return rc;
    MVS_CHECK_ARG((M == 0 || vertices) && (F == 0 || (faces && keys)));
    MVS_CHECK_ARG(F == 0 || ((const void*)keys != (const void*)vertices && (const void*)keys != (const void*)faces));
    if (workspace_bytes < MC_WORKSPACE) return MVS_E_WORKSPACE;
    hipStream_t st = mvs_stream(stream);
    int* status = static_cast<int*>(workspace);
    hipError_t e = hipMemsetAsync(status, 0, MC_WORKSPACE, st);                // every word: the first call of a mesh
    if (e != hipSuccess) return (int)e;
    if (F) hipLaunchKernelGGL(mc_keys_kernel, dim3(mvs_cdiv(F, MC_THREADS)), dim3(MC_THREADS), 0, st, vertices, M, faces, F, keys, status);
    MVS_LAUNCH_RET();
}

extern "C" int mvs_mesh_normals_f32(const float* vertices, long long M, const int* faces, long long F, const long long* sorted_keys,
                                    float* normals, void* workspace, size_t workspace_bytes, void* stream) {
    MVS_CHECK_ARG(workspace);
    if (int rc = mc_sizes(M, F)) return rc;
    MVS_CHECK_ARG((M == 0 || (vertices && normals)) && (F == 0 || (faces && sorted_keys)));
    MVS_CHECK_ARG(M == 0 || ((const void*)normals != (const void*)vertices && (const void*)normals != (const void*)faces &&
                             (const void*)normals != (const void*)sorted_keys));
    if (workspace_bytes < MC_WORKSPACE) return MVS_E_WORKSPACE;
    hipStream_t st = mvs_stream(stream);
    int* status = static_cast<int*>(workspace);
    hipError_t e = hipMemsetAsync(status + MC_ZERO_NORMALS, 0, sizeof(int), st);
    if (e != hipSuccess) return (int)e;
    if (M) hipLaunchKernelGGL(mc_normals_kernel, dim3(mvs_cdiv(M, MC_THREADS)), dim3(MC_THREADS), 0, st, vertices, M, faces, F, sorted_keys,
                              normals, status);
    MVS_LAUNCH_RET();
}

extern "C" int mvs_mesh_colour_accumulate_f32(const float* vertices, const float* normals, long long M, const float* proj,
                                              const float* centres, int V, int H, int W, const float* depth,
                                              const unsigned char* images, float min_depth, float ratio, float min_cos, int power,
                                              double* acc, int* seen, void* stream) {
    if (M < 0 || V < 0 || H < 0 || W < 0) return MVS_E_BADARG;
    MVS_CHECK_ARG(power >= 0 && power <= MC_MAX_POWER);
    MVS_CHECK_ARG(min_depth >= 0.f && __builtin_isfinite(min_depth) && ratio > 0.f && __builtin_isfinite(ratio) &&
                  min_cos >= -1.f && min_cos <= 1.f);                          // a NaN fails each of them
    if (M > MC_MAX || (V > 0 && !geo_pixels_ok(V, H, W, MC_MAX_AXIS))) return MVS_E_SHAPE;
    MVS_CHECK_ARG(V == 0 || (H >= 1 && W >= 1));
    MVS_CHECK_ARG(M == 0 || (vertices && normals && acc && seen));
    MVS_CHECK_ARG(V == 0 || (proj && centres && depth && images));
    const void* in[] = {vertices, normals, proj, centres, depth, images};
    for (const void* p : in) MVS_CHECK_ARG(p == nullptr || (p != (const void*)acc && p != (const void*)seen));
    MVS_CHECK_ARG(M == 0 || (const void*)acc != (const void*)seen);
    MVS_CHECK_ARG((((uintptr_t)acc) & 15) == 0);
    if (M == 0 || V == 0) return 0;
    hipLaunchKernelGGL(mc_accumulate_kernel, dim3(mvs_cdiv(M, MC_THREADS)), dim3(MC_THREADS), 0, mvs_stream(stream), vertices, normals, M,
                       proj, centres, V, H, W, depth, images, min_depth, ratio, min_cos, power, acc, seen);
    MVS_LAUNCH_RET();
}

extern "C" int mvs_mesh_colour_finish_u8(const unsigned char* colours, const double* acc, const int* seen, long long M,
                                         unsigned char* out, void* workspace, size_t workspace_bytes, void* stream) {
    MVS_CHECK_ARG(workspace);
    if (int rc = mc_sizes(M, 0)) return rc;
    MVS_CHECK_ARG(M == 0 || (acc && seen && out));
    MVS_CHECK_ARG(M == 0 || ((const void*)out != (const void*)colours && (const void*)out != (const void*)acc &&
                             (const void*)out != (const void*)seen));
    if (workspace_bytes < MC_WORKSPACE) return MVS_E_WORKSPACE;
    hipStream_t st = mvs_stream(stream);
    int* status = static_cast<int*>(workspace);
    hipError_t e = hipMemsetAsync(status + MC_UNSEEN, 0, sizeof(int), st);
    if (e != hipSuccess) return (int)e;
    if (M) hipLaunchKernelGGL(mc_finish_kernel, dim3(mvs_cdiv(M, MC_THREADS)), dim3(MC_THREADS), 0, st, colours, acc, seen, M, out, status);
    MVS_LAUNCH_RET();
}
