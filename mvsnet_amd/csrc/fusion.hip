// Geometric-consistency fusion of a session's depth maps into one coloured point cloud (the step the
// reference hands to the external CUDA program fusibile, mvsnet/depthfusion.py:194-214).  The algorithm is this project's own
// and fully specified in mvsnet_amd/fusion.py; it is NOT bit-compatible with fusibile (no disparity criterion; normals are
// this project's own finite-difference estimate, see below).
//
// Per reference pixel p = (x, y) of view r with filtered depth d > 0 and every source s of r's list (ascending):
//   (u, v, w)    = M[r][s] (x d, y d, d, 1)          project into s; w > 0
//   q            = (floor(u/w + 1/2), floor(v/w + 1/2)) inside s and valid there (filtered depth ds > 0)
//   (u', v', w') = M[s][r] (qx ds, qy ds, ds, 1)     back into r; w' > 0
//   consistent   : |(u'/w', v'/w') - (x, y)|^2 < reproj^2 and |w' - d| < depth_rel d
// M[a][b] = P_b o B_a (3x4, float32 on the device, composed in float64 on the host): B_a maps (x d, y d, d, 1) to the world
// point, P_b = K_b [R_b | t_b].  A (pixel, source) pair is two 3x4 products, two IEEE reciprocals and one gather of the
// source's filtered depth; a consistent pair adds a third 3x4 product (its world point).
//
// Launches (all on the caller's stream; nothing allocated, nothing synchronised -- the whole call captures into a hipGraph):
//   filter    df = D where D > 0, finite and P >= prob_threshold, else 0 (all views; the gathers read df only);
//   pairs     one lane per reference pixel, the wave's sources a contiguous chunk ("slice") of r's list: source indices and
//             table entries are wave-uniform scalar loads (constant address space + readfirstlane; checked in the ISA).  Per
//             slice a partial sum of (X_s - X) and the consistent count, SoA planes;
//   finalize  slices summed in slice order (fixed: results are bitwise reproducible), keep = n >= num_consistent, fused point
//             X + sum / (n + 1); in dedupe mode the witnesses q of a kept pixel are marked used (uint8 stores of 1);
//   compact   per-1024-pixel counts, one exclusive scan, ordered writes: view ascending, then row-major pixel order.
// dedupe = 0: pairs + finalize once over all views.  dedupe = 1: views in ascending order, pairs + finalize per view (the marks
// of view r land only in views != r, so a view's pixels run in parallel); its 20 480 pixels at 160 x 128 are 320 waves, so the
// sources of a pixel are spread over up to 16 slices (grid.z) to fill the 256 CUs.
// Normals (mvs_depth_normals_f32, mvs_fusion_normals_f32; the NRM = true instantiations of pairs, finalize and write):
//   normal map  one lane per pixel, all views in one launch: a 5-point stencil on the filtered depth, tangents
//             tx = a(x+1, y) - a(x-1, y), ty = a(x, y+1) - a(x, y-1) with a = (x d, y d, d) over the usable neighbours (valid and
//             |dq - d| < jump d; one-sided when one is usable), n = A ty x A tx normalised and turned towards the camera, A =
//             the first three columns of B_v (scalar loads); (0, 0, 0) = no normal.  Inside the fusion the map is kept in
//             the workspace, FU_NSTRIDE floats per pixel (4: one 16-byte gather per consistent pair, word 3 = 1 when the
//             pixel has a normal; 3: packed); the public map is (V, H, W, 3);
//   pairs     a consistent pair gathers its source's normal AFTER the geometric tests and adds it to three more partial-sum
//             planes per slice; with a cosine threshold > -1 a pixel without a normal is invalid (as reference pixel and as
//             witness) and the pair must also satisfy n_r . n_s > cos;
//   finalize  N = n_r + sum over slices (slice order), normalised, (0, 0, 0) when |N| = 0;  write compacts it like the points.
// The NRM = false instantiations are the kernels of mvs_fusion_f32, instruction for instruction what they were without the
// template parameter.
// The compiler merges some neighbouring stores into wide ones; tools/store_hazard_scan.py (run by the CPU suite) finds none of
// them with its data registers overwritten too early.
#include "geom_common.h"

namespace {

constexpr int FU_THREADS = 256;
constexpr int FU_TABLE = 12;          // floats per 3x4 matrix
constexpr int FU_MAX_SLICES = 16;
constexpr int FU_CHUNK = FU_THREADS * GEO_COMPACT_PER;   // 1024 pixels per compaction block
#ifndef FU_NSTRIDE
#define FU_NSTRIDE 4                  // floats per pixel of the internal normal map (EXPERIMENTS.md: 4 padded, 3 packed)
#endif
static_assert(FU_NSTRIDE == 3 || FU_NSTRIDE == 4, "internal normal map: 3 (packed) or 4 (padded, validity word) floats per pixel");

__device__ __forceinline__ void fu_apply(const float* __restrict__ m, float a0, float a1, float a2, float& o0, float& o1, float& o2) {
    o0 = fmaf(m[0], a0, fmaf(m[1], a1, fmaf(m[2], a2, m[3])));
    o1 = fmaf(m[4], a0, fmaf(m[5], a1, fmaf(m[6], a2, m[7])));
    o2 = fmaf(m[8], a0, fmaf(m[9], a1, fmaf(m[10], a2, m[11])));
}

typedef __attribute__((address_space(4))) const int fu_cint;       // geo_cfloat's sibling: scalar loads of uniform ints

struct FuMat { float m[FU_TABLE]; };

// Matrix `index` (wave-uniform; readfirstlane states it to the compiler) of a table of 3x4 matrices.
__device__ __forceinline__ FuMat fu_load_mat(const float* table, int index) {
    const geo_cfloat* c = (const geo_cfloat*)table + (size_t)__builtin_amdgcn_readfirstlane(index) * FU_TABLE;
    FuMat t;
#pragma unroll
    for (int i = 0; i < FU_TABLE; ++i) t.m[i] = c[i];
    return t;
}

// Ties the loaded values to this point in the program: the compiler cannot sink the scalar loads into the (divergent)
// branches that use them, so a whole iteration's tables arrive in one round trip.
__device__ __forceinline__ void fu_pin(const FuMat& t) {
#pragma unroll
    for (int i = 0; i < FU_TABLE; ++i) asm volatile("" ::"s"(t.m[i]));
}

__device__ __forceinline__ int fu_load_uniform(const int* p, int i) {
    return ((const fu_cint*)p)[__builtin_amdgcn_readfirstlane(i)];
}

// Normal of element e of a map of STRIDE floats per pixel; false when the pixel has none (then the normal is (0, 0, 0)).
template <int STRIDE>
__device__ __forceinline__ bool fu_normal_load(const float* __restrict__ nmap, size_t e, float& n0, float& n1, float& n2) {
    if constexpr (STRIDE == 4) {
        const float4 t = reinterpret_cast<const float4*>(nmap)[e];
        n0 = t.x; n1 = t.y; n2 = t.z;
        return t.w != 0.f;
    } else {
        n0 = nmap[3 * e]; n1 = nmap[3 * e + 1]; n2 = nmap[3 * e + 2];
        return n0 != 0.f || n1 != 0.f || n2 != 0.f;
    }
}

// The one extra kernel argument of the NRM instantiations of pairs, finalize and write.  It is a parameter pack that is empty
// for NRM = false, so that those keep the parameter list (and with it the kernarg layout and the code) they had.
struct FuNrm {
    const float* nmap;      // (V, HW, FU_NSTRIDE) normal maps
    float cos_thr;          // > -1: normal test on
    float* fnrm;            // (V, HW, 3) fused normals before compaction
    float* normals;         // (count, 3) output
};
__device__ __forceinline__ const FuNrm& fu_nrm(const FuNrm& a) { return a; }

// Filtered depth of element i: from df, or (RAW) from depth and prob by the rule of geo_filter_kernel.
template <bool RAW>
__device__ __forceinline__ float fu_filtered(const float* __restrict__ depth, const float* __restrict__ prob, float thr, size_t i) {
    const float d = depth[i];
    if constexpr (RAW) return (d > 0.f && __builtin_isfinite(d) && prob[i] >= thr) ? d : 0.f;
    return d;
}

// grid (cdiv(HW, 256), V).  nmap (V, HW, STRIDE) floats.  RAW: depth / prob are the caller's maps, else depth = df (prob unused).
// The view is wave-uniform: A_v (and C_v, which cancels: X - C_v = A_v a) arrives as scalar loads.
template <int STRIDE, bool RAW>
__global__ __launch_bounds__(FU_THREADS) void fusion_normal_map_kernel(const float* __restrict__ depth, const float* __restrict__ prob,
                                                                        float thr, const float* __restrict__ B, int H, int W,
                                                                        float jump, float* __restrict__ nmap) {
    const int HW = H * W;
    const int v = blockIdx.y;
    const int p = blockIdx.x * FU_THREADS + threadIdx.x;
    if (p >= HW) return;
    const FuMat A = fu_load_mat(B, v);
    const int x = p % W, y = p / W;
    const size_t e = (size_t)v * HW + p;
    const float d = fu_filtered<RAW>(depth, prob, thr, e);
    float n0 = 0.f, n1 = 0.f, n2 = 0.f;
    bool has = false;
    if (d > 0.f) {
        const float lim = jump * d;
        const float dl = x > 0 ? fu_filtered<RAW>(depth, prob, thr, e - 1) : 0.f;
        const float dr = x + 1 < W ? fu_filtered<RAW>(depth, prob, thr, e + 1) : 0.f;
        const float du = y > 0 ? fu_filtered<RAW>(depth, prob, thr, e - W) : 0.f;
        const float dd = y + 1 < H ? fu_filtered<RAW>(depth, prob, thr, e + W) : 0.f;
        const bool ul = dl > 0.f && fabsf(dl - d) < lim, ur = dr > 0.f && fabsf(dr - d) < lim;
        const bool uu = du > 0.f && fabsf(du - d) < lim, ud = dd > 0.f && fabsf(dd - d) < lim;
        if ((ul || ur) && (uu || ud)) {
            const float fx = (float)x, fy = (float)y;
            // tangent = a(high end) - a(low end), an unusable end replaced by the pixel itself
            const float xh = ur ? fx + 1.f : fx, dxh = ur ? dr : d, xl = ul ? fx - 1.f : fx, dxl = ul ? dl : d;
            const float yh = ud ? fy + 1.f : fy, dyh = ud ? dd : d, yl = uu ? fy - 1.f : fy, dyl = uu ? du : d;
            const float tx0 = xh * dxh - xl * dxl, tx1 = fy * dxh - fy * dxl, tx2 = dxh - dxl;
            const float ty0 = fx * dyh - fx * dyl, ty1 = yh * dyh - yl * dyl, ty2 = dyh - dyl;
            const float* m = A.m;
            const float q0 = fmaf(m[0], tx0, fmaf(m[1], tx1, m[2] * tx2)), q1 = fmaf(m[4], tx0, fmaf(m[5], tx1, m[6] * tx2)),
                        q2 = fmaf(m[8], tx0, fmaf(m[9], tx1, m[10] * tx2));
            const float p0 = fmaf(m[0], ty0, fmaf(m[1], ty1, m[2] * ty2)), p1 = fmaf(m[4], ty0, fmaf(m[5], ty1, m[6] * ty2)),
                        p2 = fmaf(m[8], ty0, fmaf(m[9], ty1, m[10] * ty2));
            const float c0 = p1 * q2 - p2 * q1, c1 = p2 * q0 - p0 * q2, c2 = p0 * q1 - p1 * q0;      // A ty x A tx
            const float len2 = c0 * c0 + c1 * c1 + c2 * c2;
            if (len2 > 0.f && __builtin_isfinite(len2)) {
                const float a0 = fx * d, a1 = fy * d;
                const float g0 = fmaf(m[0], a0, fmaf(m[1], a1, m[2] * d)), g1 = fmaf(m[4], a0, fmaf(m[5], a1, m[6] * d)),
                            g2 = fmaf(m[8], a0, fmaf(m[9], a1, m[10] * d));                             // X - C_v
                float inv = 1.0f / sqrtf(len2);
                if (c0 * g0 + c1 * g1 + c2 * g2 > 0.f) inv = -inv;                                      // face the camera
                n0 = c0 * inv; n1 = c1 * inv; n2 = c2 * inv;
                has = true;
            }
        }
    }
    if constexpr (STRIDE == 4) {
        reinterpret_cast<float4*>(nmap)[e] = make_float4(n0, n1, n2, has ? 1.f : 0.f);
    } else {
        nmap[3 * e] = n0; nmap[3 * e + 1] = n1; nmap[3 * e + 2] = n2;
    }
}

// grid (cdiv(HW, 256), views of this launch, slices).  part: (slices, 4, nview, HW) floats = sum of (X_s - X) x/y/z, count;
// NRM: (slices, 7, nview, HW), planes 4..6 the sum of the consistent sources' normals (nmap: (V, HW, FU_NSTRIDE)).
// witness (dedupe only): (max_src, HW) int32, view * HW + q of the consistent source at list position j, else -1.
// The reference view r, its source list and the source s of an iteration are wave-uniform (they depend on blockIdx and the
// loop counter only): the list and the three 3x4 tables of a pair (M[r][s], M[s][r], B_s) are scalar loads, one iteration
// ahead.  The only vector-memory access of an iteration is the gather of the source's filtered depth (plus the witness store
// in dedupe mode).
template <bool NRM, typename... NA>
__global__ __launch_bounds__(FU_THREADS) void fusion_pairs_kernel(
        const float* __restrict__ df, const uint8_t* used, const float* __restrict__ M, const float* __restrict__ B,
        const int* __restrict__ src_off, const int* __restrict__ src_idx, int max_src, int V, int H, int W, int v0, int chunk,
        float reproj2, float depth_rel, float* __restrict__ part, int* __restrict__ witness, NA... na) {
    constexpr int PLANES = NRM ? 7 : 4;
    const float* __restrict__ nmap = nullptr;
    float cos_thr = -1.f;
    if constexpr (NRM) { nmap = fu_nrm(na...).nmap; cos_thr = fu_nrm(na...).cos_thr; }
    const int HW = H * W;
    const int vl = blockIdx.y, r = v0 + vl, nview = gridDim.y;
    const int slice = blockIdx.z;
    const int p = blockIdx.x * FU_THREADS + threadIdx.x;
    const bool inside = p < HW;
    const int x = inside ? p % W : 0, y = inside ? p / W : 0;
    float d = inside ? df[(size_t)r * HW + p] : 0.f;
    if (used && inside && used[(size_t)r * HW + p]) d = 0.f;
    float r0 = 0.f, r1 = 0.f, r2 = 0.f, m0 = 0.f, m1 = 0.f, m2 = 0.f;
    if constexpr (NRM) {
        // threshold on: a pixel without a normal is no reference pixel
        if (cos_thr > -1.f && !(inside && fu_normal_load<FU_NSTRIDE>(nmap, (size_t)r * HW + p, r0, r1, r2))) d = 0.f;
    }
    const bool ref = d > 0.f;
    const int beg = fu_load_uniform(src_off, r);
    int cnt = fu_load_uniform(src_off, r + 1) - beg;
    cnt = cnt < 0 ? 0 : (cnt > max_src ? max_src : cnt);
    const int j0 = min(slice * chunk, cnt), j1 = min(j0 + chunk, cnt);
    const float fx = (float)x, fy = (float)y;
    const float a0 = fx * d, a1 = fy * d;
    float X0, X1, X2;
    const FuMat Br = fu_load_mat(B, r);
    fu_apply(Br.m, a0, a1, d, X0, X1, X2);
    float s0 = 0.f, s1 = 0.f, s2 = 0.f, n = 0.f;
    // one-iteration software pipeline: the tables of source j+1 and the index of source j+2 are requested at the top of
    // iteration j and waited for at its bottom, so an iteration waits on its own gather only.  An out-of-range source
    // loads view r's tables instead (never used) so that every address stays inside the tables.
    const auto safe = [&](int src) { return (src >= 0 && src < V) ? src : r; };
    int s_cur = j0 < j1 ? fu_load_uniform(src_idx, beg + j0) : r;
    int s_nxt = j0 + 1 < j1 ? fu_load_uniform(src_idx, beg + j0 + 1) : s_cur;
    FuMat Mrs = fu_load_mat(M, r * V + safe(s_cur)), Msr = fu_load_mat(M, safe(s_cur) * V + r), Bs = fu_load_mat(B, safe(s_cur));
    fu_pin(Mrs); fu_pin(Msr); fu_pin(Bs);
    for (int j = j0; j < j1; ++j) {
        const int s = s_cur, sn = s_nxt;
        const FuMat nMrs = fu_load_mat(M, r * V + safe(sn)), nMsr = fu_load_mat(M, safe(sn) * V + r), nBs = fu_load_mat(B, safe(sn));
        const int snn = j + 2 < j1 ? fu_load_uniform(src_idx, beg + j + 2) : sn;
        int wit = -1;
        if (s >= 0 && s < V && s != r) {                  // uniform branch
            float u, v, w;
            fu_apply(Mrs.m, a0, a1, d, u, v, w);
            if (ref && w > 0.f) {
                const float iw = 1.0f / w;
                const float qxf = floorf(u * iw + 0.5f), qyf = floorf(v * iw + 0.5f);
                if (qxf >= 0.f && qxf < (float)W && qyf >= 0.f && qyf < (float)H) {
                    const int q = (int)qyf * W + (int)qxf;
                    const float ds = df[(size_t)s * HW + q];
                    if (ds > 0.f) {
                        const float b0 = qxf * ds, b1 = qyf * ds;
                        float u2, v2, w2;
                        fu_apply(Msr.m, b0, b1, ds, u2, v2, w2);
                        if (w2 > 0.f) {
                            const float iw2 = 1.0f / w2;
                            const float ex = u2 * iw2 - fx, ey = v2 * iw2 - fy;
                            if (ex * ex + ey * ey < reproj2 && fabsf(w2 - d) < depth_rel * d) {
                                float Y0, Y1, Y2;
                                if constexpr (NRM) {
                                    float t0, t1, t2;
                                    const bool has = fu_normal_load<FU_NSTRIDE>(nmap, (size_t)s * HW + q, t0, t1, t2);
                                    if (!(cos_thr > -1.f) || (has && r0 * t0 + r1 * t1 + r2 * t2 > cos_thr)) {
                                        fu_apply(Bs.m, b0, b1, ds, Y0, Y1, Y2);
                                        s0 += Y0 - X0; s1 += Y1 - X1; s2 += Y2 - X2; n += 1.f;
                                        m0 += t0; m1 += t1; m2 += t2;
                                        wit = s * HW + q;
                                    }
                                } else {
                                    fu_apply(Bs.m, b0, b1, ds, Y0, Y1, Y2);
                                    s0 += Y0 - X0; s1 += Y1 - X1; s2 += Y2 - X2; n += 1.f;
                                    wit = s * HW + q;
                                }
                            }
                        }
                    }
                }
            }
        }
        if (witness && inside) witness[(size_t)j * HW + p] = wit;
        fu_pin(nMrs); fu_pin(nMsr); fu_pin(nBs);
        Mrs = nMrs; Msr = nMsr; Bs = nBs;
        s_cur = sn; s_nxt = snn;
    }
    if (!inside) return;
    const size_t plane = (size_t)nview * HW, base = (size_t)slice * PLANES * plane + (size_t)vl * HW + p;
    part[base] = s0;
    part[base + plane] = s1;
    part[base + 2 * plane] = s2;
    part[base + 3 * plane] = n;
    if constexpr (NRM) {
        part[base + 4 * plane] = m0;
        part[base + 5 * plane] = m1;
        part[base + 6 * plane] = m2;
    }
}

// grid (cdiv(HW, 256), views of this launch).  keep (V, HW) uint8, fxyz (V, HW, 3) float32; NRM: fnrm (V, HW, 3) float32.
template <bool NRM, typename... NA>
__global__ __launch_bounds__(FU_THREADS) void fusion_finalize_kernel(
        const float* __restrict__ df, uint8_t* used, const float* __restrict__ B, const float* __restrict__ part, int slices,
        const int* __restrict__ src_off, const int* __restrict__ witness, int max_src, int H, int W, int v0, float num_consistent,
        uint8_t* __restrict__ keep, float* __restrict__ fxyz, NA... na) {
    constexpr int PLANES = NRM ? 7 : 4;
    const float* __restrict__ nmap = nullptr;
    float* __restrict__ fnrm = nullptr;
    float cos_thr = -1.f;
    if constexpr (NRM) { nmap = fu_nrm(na...).nmap; cos_thr = fu_nrm(na...).cos_thr; fnrm = fu_nrm(na...).fnrm; }
    const int HW = H * W;
    const int vl = blockIdx.y, r = v0 + vl, nview = gridDim.y;
    const int p = blockIdx.x * FU_THREADS + threadIdx.x;
    if (p >= HW) return;
    const size_t e = (size_t)r * HW + p;
    float d = df[e];
    if (used && used[e]) d = 0.f;
    float N0 = 0.f, N1 = 0.f, N2 = 0.f;
    if constexpr (NRM) {
        if (!fu_normal_load<FU_NSTRIDE>(nmap, e, N0, N1, N2) && cos_thr > -1.f) d = 0.f;
    }
    const float fx = (float)(p % W), fy = (float)(p / W);
    float X0, X1, X2;
    fu_apply(B + (size_t)r * FU_TABLE, fx * d, fy * d, d, X0, X1, X2);
    const size_t plane = (size_t)nview * HW;
    float s0 = 0.f, s1 = 0.f, s2 = 0.f, n = 0.f, m0 = 0.f, m1 = 0.f, m2 = 0.f;
    for (int sl = 0; sl < slices; ++sl) {
        const size_t base = (size_t)sl * PLANES * plane + (size_t)vl * HW + p;
        s0 += part[base]; s1 += part[base + plane]; s2 += part[base + 2 * plane]; n += part[base + 3 * plane];
        if constexpr (NRM) { m0 += part[base + 4 * plane]; m1 += part[base + 5 * plane]; m2 += part[base + 6 * plane]; }
    }
    const bool k = d > 0.f && n >= num_consistent;
    keep[e] = k ? 1 : 0;
    const float inv = 1.0f / (n + 1.f);
    fxyz[3 * e] = X0 + s0 * inv;
    fxyz[3 * e + 1] = X1 + s1 * inv;
    fxyz[3 * e + 2] = X2 + s2 * inv;
    if constexpr (NRM) {
        N0 += m0; N1 += m1; N2 += m2;
        const float len2 = N0 * N0 + N1 * N1 + N2 * N2;
        const float ninv = (len2 > 0.f && __builtin_isfinite(len2)) ? 1.0f / sqrtf(len2) : 0.f;
        fnrm[3 * e] = N0 * ninv;
        fnrm[3 * e + 1] = N1 * ninv;
        fnrm[3 * e + 2] = N2 * ninv;
    }
    if (k && witness) {
        int cnt = src_off[r + 1] - src_off[r];
        cnt = cnt < 0 ? 0 : (cnt > max_src ? max_src : cnt);
        for (int j = 0; j < cnt; ++j) {
            const int w = witness[(size_t)j * HW + p];
            if (w >= 0) used[w] = 1;        // always another view: idempotent stores, the race between writers is harmless
        }
    }
}

template <bool NRM, typename... NA>
__global__ __launch_bounds__(FU_THREADS) void fusion_write_kernel(
        const uint8_t* __restrict__ keep, const float* __restrict__ fxyz, size_t n, int HW, int W, const int* __restrict__ offs,
        const uint8_t* __restrict__ images, int img_h, int img_w, int H, float* __restrict__ xyz, uint8_t* __restrict__ rgb,
        int* __restrict__ view_index, int* __restrict__ pixel_index, NA... na) {
    const float* __restrict__ fnrm = nullptr;
    float* __restrict__ normals = nullptr;
    if constexpr (NRM) { fnrm = fu_nrm(na...).fnrm; normals = fu_nrm(na...).normals; }
    __shared__ int sh[FU_THREADS];
    const size_t e0 = (size_t)blockIdx.x * FU_CHUNK + GEO_COMPACT_PER * threadIdx.x;
    int c = 0;
    for (int i = 0; i < GEO_COMPACT_PER; ++i) c += (e0 + i < n && keep[e0 + i]) ? 1 : 0;
    int total;
    int o = offs[blockIdx.x] + geo_block_exclusive_scan<FU_THREADS>(c, sh, total);
    for (int i = 0; i < GEO_COMPACT_PER; ++i) {
        const size_t e = e0 + i;
        if (e >= n || !keep[e]) continue;
        xyz[3 * (size_t)o] = fxyz[3 * e];
        xyz[3 * (size_t)o + 1] = fxyz[3 * e + 1];
        xyz[3 * (size_t)o + 2] = fxyz[3 * e + 2];
        if constexpr (NRM) {
            normals[3 * (size_t)o] = fnrm[3 * e];
            normals[3 * (size_t)o + 1] = fnrm[3 * e + 1];
            normals[3 * (size_t)o + 2] = fnrm[3 * e + 2];
        }
        const int v = (int)(e / HW), p = (int)(e % HW);
        view_index[o] = v;
        if (pixel_index) pixel_index[o] = p;
        uint8_t c0 = 0, c1 = 0, c2 = 0;
        if (images) {
            const long long x = p % W, y = p / W;
            const long long ix = (2 * x + 1) * img_w / (2 * (long long)W), iy = (2 * y + 1) * img_h / (2 * (long long)H);
            const uint8_t* px = images + (((size_t)v * img_h + iy) * img_w + ix) * 3;
            c0 = px[0]; c1 = px[1]; c2 = px[2];
        }
        rgb[3 * (size_t)o] = c0;
        rgb[3 * (size_t)o + 1] = c1;
        rgb[3 * (size_t)o + 2] = c2;
        ++o;
    }
}

int fusion_slices(int HW, int max_src, int dedupe) {
    if (!dedupe || max_src <= 1) return 1;
    int s = mvs_cdiv(4096, mvs_cdiv(HW, 64));          // about 4096 waves per view launch
    if (s > FU_MAX_SLICES) s = FU_MAX_SLICES;
    if (s > max_src) s = max_src;
    return s < 1 ? 1 : s;
}

struct FuLayout {
    size_t df, used, part, witness, keep, fxyz, counts, offs, nmap, fnrm, total;
    int slices, nb;
};

FuLayout fusion_layout(int V, int H, int W, int max_src, int dedupe, bool normals = false) {
    FuLayout L{};
    const size_t px = (size_t)V * H * W, HW = (size_t)H * W;
    L.slices = fusion_slices((int)HW, max_src, dedupe);
    L.nb = (int)((px + FU_CHUNK - 1) / FU_CHUNK);
    const size_t nview = dedupe ? 1 : (size_t)V;
    GeoCarver c;
    L.df = c.take(px * sizeof(float));
    L.used = c.take(dedupe ? px : 0);
    L.part = c.take((size_t)L.slices * (normals ? 7 : 4) * nview * HW * sizeof(float));
    L.witness = c.take(dedupe ? (size_t)max_src * HW * sizeof(int) : 0);
    L.keep = c.take(px);
    L.fxyz = c.take(px * 3 * sizeof(float));
    L.counts = c.take((size_t)L.nb * sizeof(int));
    L.offs = c.take((size_t)L.nb * sizeof(int));
    L.nmap = c.take(normals ? px * FU_NSTRIDE * sizeof(float) : 0);
    L.fnrm = c.take(normals ? px * 3 * sizeof(float) : 0);
    L.total = c.off;
    return L;
}

bool fusion_shape_ok(int V, int H, int W, int max_src) {
    if (V > 65535 || max_src > 65535) return false;
    return (long long)V * H * W <= 0x7fffffffLL;
}

}  // namespace

extern "C" size_t mvs_fusion_workspace_bytes(int V, int H, int W, int max_sources, int dedupe) {
    if (V <= 0 || H <= 0 || W <= 0 || max_sources < 0 || !fusion_shape_ok(V, H, W, max_sources)) return 0;
    return fusion_layout(V, H, W, max_sources, dedupe != 0).total;
}

namespace {

// The launches of one fusion.  NRM: normal map into the workspace first, then the normal-carrying instantiations.
template <bool NRM>
int fusion_launch(const float* depth, const float* prob, int V, int H, int W, const float* tables, const int* src_offsets,
                  const int* src_index, int max_sources, float prob_threshold, float reproj_threshold, float depth_rel_threshold,
                  float num_consistent, int dedupe, float jump_threshold, float cos_threshold, const uint8_t* images, int img_h,
                  int img_w, float* xyz, uint8_t* rgb, float* normals, int* view_index, int* pixel_index, int* count,
                  void* workspace, size_t workspace_bytes, void* stream) {
    MVS_CHECK_ARG(depth && prob && tables && src_offsets && xyz && rgb && view_index && count && workspace);
    MVS_CHECK_ARG(V > 0 && H > 0 && W > 0 && max_sources >= 0 && (max_sources == 0 || src_index));
    MVS_CHECK_ARG(!images || (img_h > 0 && img_w > 0));
    MVS_CHECK_ARG(!__builtin_isnan(prob_threshold) && reproj_threshold > 0.f && depth_rel_threshold >= 0.f &&
                  !__builtin_isnan(num_consistent));
    if (NRM) MVS_CHECK_ARG(normals && jump_threshold >= 0.f && !__builtin_isnan(cos_threshold) && cos_threshold < 1.f);
    if (!fusion_shape_ok(V, H, W, max_sources)) return MVS_E_SHAPE;
    if (images && (long long)img_h * img_w * 3 * V > 0x7fffffffffffLL) return MVS_E_SHAPE;
    const int dd = dedupe != 0;
    const FuLayout L = fusion_layout(V, H, W, max_sources, dd, NRM);
    if (workspace_bytes < L.total) return MVS_E_WORKSPACE;
    hipStream_t st = mvs_stream(stream);
    char* ws = static_cast<char*>(workspace);
    float* df = reinterpret_cast<float*>(ws + L.df);
    uint8_t* used = dd ? reinterpret_cast<uint8_t*>(ws + L.used) : nullptr;
    float* part = reinterpret_cast<float*>(ws + L.part);
    int* witness = dd ? reinterpret_cast<int*>(ws + L.witness) : nullptr;
    uint8_t* keep = reinterpret_cast<uint8_t*>(ws + L.keep);
    float* fxyz = reinterpret_cast<float*>(ws + L.fxyz);
    int* counts = reinterpret_cast<int*>(ws + L.counts);
    int* offs = reinterpret_cast<int*>(ws + L.offs);
    float* nmap = NRM ? reinterpret_cast<float*>(ws + L.nmap) : nullptr;
    float* fnrm = NRM ? reinterpret_cast<float*>(ws + L.fnrm) : nullptr;
    const int HW = H * W;
    const size_t px = (size_t)V * HW;
    const float* M = tables;
    const float* B = tables + (size_t)V * V * FU_TABLE;
    const int chunk = max_sources > 0 ? mvs_cdiv(max_sources, L.slices) : 0;
    const float reproj2 = reproj_threshold * reproj_threshold;
    const unsigned gx = (unsigned)mvs_cdiv(HW, FU_THREADS);

    hipLaunchKernelGGL(geo_filter_kernel<FU_THREADS>, dim3((unsigned)((px + FU_THREADS - 1) / FU_THREADS)), dim3(FU_THREADS), 0, st,
                       depth, prob, px, prob_threshold, df);
    if (NRM)
        hipLaunchKernelGGL((fusion_normal_map_kernel<FU_NSTRIDE, false>), dim3(gx, V), dim3(FU_THREADS), 0, st, df,
                           (const float*)nullptr, 0.f, B, H, W, jump_threshold, nmap);
    const FuNrm na{nmap, cos_threshold, fnrm, normals};
    const auto pairs = [&](dim3 grid, const uint8_t* u, int v0, int* wit) {
        if constexpr (NRM)
            hipLaunchKernelGGL((fusion_pairs_kernel<true, FuNrm>), grid, dim3(FU_THREADS), 0, st, df, u, M, B, src_offsets, src_index,
                               max_sources, V, H, W, v0, chunk, reproj2, depth_rel_threshold, part, wit, na);
        else
            hipLaunchKernelGGL((fusion_pairs_kernel<false>), grid, dim3(FU_THREADS), 0, st, df, u, M, B, src_offsets, src_index,
                               max_sources, V, H, W, v0, chunk, reproj2, depth_rel_threshold, part, wit);
    };
    const auto finalize = [&](dim3 grid, uint8_t* u, int slices, const int* wit, int v0) {
        if constexpr (NRM)
            hipLaunchKernelGGL((fusion_finalize_kernel<true, FuNrm>), grid, dim3(FU_THREADS), 0, st, df, u, B, part, slices,
                               src_offsets, wit, max_sources, H, W, v0, num_consistent, keep, fxyz, na);
        else
            hipLaunchKernelGGL((fusion_finalize_kernel<false>), grid, dim3(FU_THREADS), 0, st, df, u, B, part, slices, src_offsets,
                               wit, max_sources, H, W, v0, num_consistent, keep, fxyz);
    };
    if (dd) {
        hipError_t e = hipMemsetAsync(used, 0, px, st);
        if (e != hipSuccess) return (int)e;
        for (int r = 0; r < V; ++r) {
            pairs(dim3(gx, 1, L.slices), used, r, witness);
            finalize(dim3(gx, 1), used, L.slices, witness, r);
        }
    } else {
        pairs(dim3(gx, V, 1), nullptr, 0, nullptr);
        finalize(dim3(gx, V), nullptr, 1, nullptr, 0);
    }
    hipLaunchKernelGGL(geo_compact_count_kernel<FU_THREADS>, dim3(L.nb), dim3(FU_THREADS), 0, st, keep, px, counts);
    hipLaunchKernelGGL(geo_scan_top_kernel<FU_THREADS>, dim3(1), dim3(FU_THREADS), 0, st, counts, L.nb, 0, offs, count);
    if constexpr (NRM)
        hipLaunchKernelGGL((fusion_write_kernel<true, FuNrm>), dim3(L.nb), dim3(FU_THREADS), 0, st, keep, fxyz, px, HW, W, offs, images,
                           img_h, img_w, H, xyz, rgb, view_index, pixel_index, na);
    else
        hipLaunchKernelGGL((fusion_write_kernel<false>), dim3(L.nb), dim3(FU_THREADS), 0, st, keep, fxyz, px, HW, W, offs, images,
                           img_h, img_w, H, xyz, rgb, view_index, pixel_index);
    MVS_LAUNCH_RET();
}

}  // namespace

extern "C" int mvs_fusion_f32(const float* depth, const float* prob, int V, int H, int W, const float* tables,
                              const int* src_offsets, const int* src_index, int max_sources, float prob_threshold,
                              float reproj_threshold, float depth_rel_threshold, float num_consistent, int dedupe,
                              const uint8_t* images, int img_h, int img_w, float* xyz, uint8_t* rgb, int* view_index, int* pixel_index,
                              int* count, void* workspace, size_t workspace_bytes, void* stream) {
    return fusion_launch<false>(depth, prob, V, H, W, tables, src_offsets, src_index, max_sources, prob_threshold,
                                reproj_threshold, depth_rel_threshold, num_consistent, dedupe, 0.f, -1.f, images, img_h, img_w,
                                xyz, rgb, nullptr, view_index, pixel_index, count, workspace, workspace_bytes, stream);
}

extern "C" size_t mvs_fusion_normals_workspace_bytes(int V, int H, int W, int max_sources, int dedupe) {
    if (V <= 0 || H <= 0 || W <= 0 || max_sources < 0 || !fusion_shape_ok(V, H, W, max_sources)) return 0;
    return fusion_layout(V, H, W, max_sources, dedupe != 0, true).total;
}

extern "C" int mvs_fusion_normals_f32(const float* depth, const float* prob, int V, int H, int W, const float* tables,
                                      const int* src_offsets, const int* src_index, int max_sources, float prob_threshold,
                                      float reproj_threshold, float depth_rel_threshold, float num_consistent, int dedupe,
                                      float jump_threshold, float normal_cos_threshold, const uint8_t* images, int img_h,
                                      int img_w, float* xyz, uint8_t* rgb, float* normals, int* view_index, int* pixel_index,
                                      int* count, void* workspace, size_t workspace_bytes, void* stream) {
    return fusion_launch<true>(depth, prob, V, H, W, tables, src_offsets, src_index, max_sources, prob_threshold,
                               reproj_threshold, depth_rel_threshold, num_consistent, dedupe, jump_threshold,
                               normal_cos_threshold <= -1.f ? -1.f : normal_cos_threshold, images, img_h, img_w, xyz, rgb, normals,
                               view_index, pixel_index, count, workspace, workspace_bytes, stream);
}

extern "C" int mvs_depth_normals_f32(const float* depth, const float* prob, int V, int H, int W, const float* tables,
                                     float prob_threshold, float jump_threshold, float* normals, void* stream) {
    MVS_CHECK_ARG(depth && prob && tables && normals && V > 0 && H > 0 && W > 0);
    MVS_CHECK_ARG(!__builtin_isnan(prob_threshold) && jump_threshold >= 0.f);
    if (!fusion_shape_ok(V, H, W, 0)) return MVS_E_SHAPE;
    hipLaunchKernelGGL((fusion_normal_map_kernel<3, true>), dim3((unsigned)mvs_cdiv(H * W, FU_THREADS), V), dim3(FU_THREADS), 0,
                       mvs_stream(stream), depth, prob, prob_threshold, tables + (size_t)V * V * FU_TABLE, H, W, jump_threshold,
                       normals);
    MVS_LAUNCH_RET();
}
