// Winograd F(2,3) variant of the fused pass over the cost volume (conv3d_c8.hip: 3dconv0_1, 32 -> 8 stride 1, and 3dconv1_0,
// 32 -> 16 stride 2, from one staging of the volume).  3dconv0_1 is 80 % of that launch's matrix work; along w its three taps
// become four products per PAIR of output columns instead of six:
//
//   staged columns d0..d3 = 2p-1 .. 2p+2 of output columns 2p, 2p+1        weights g0..g2 = w[kw = 0..2]
//   t0 = d0 - d2   t1 = d1 + d2   t2 = d2 - d1   t3 = d1 - d3              U0 = g0   U1 = (g0 + g1 + g2) / 2
//   m_i = U_i * t_i (summed over kd, kh, ci)                               U2 = (g0 - g1 + g2) / 2   U3 = g2
//   y[2p] = m0 + m1 + m2          y[2p+1] = m1 - m2 - m3
//
// The kernel is conv3d_c8_kernel<true, false, SPAN> with the tap index kw = 0..2 replaced by the point index 0..3:
//
//   * An MFMA column is a pair of output columns, so the workgroup's tile is 8 x 32 (h x w), 10 x 34 staged positions per plane.
//     Two raw slabs are 87 KB and the 12 (kh, point) weight blocks 36.9 KB: one workgroup per CU.
//   * The workgroup has eight waves, two per SIMD, in two roles that move no arithmetic between waves: waves 0-3 carry 3dconv0_1
//     (the Winograd sweep and retire(), 320 MFMAs per interior plane), wave 4 + w carries what wave w carried of 3dconv1_0 (input
//     channels 8w .. 8w + 7; 72 or 144 MFMAs per plane) and fills the matrix pipe behind its SIMD partner's operand reads,
//     transforms, stores and barrier waits.  All 512 threads stage the planes, six pieces each.  The role is a scalar branch
//     around the whole march, so each role's registers are allocated by themselves (at most 256 per wave).  One barrier per
//     plane joins all eight.  MVS_HOOK_PAIR_WAVES4 = 1 takes the four-wave instantiation (<SPAN, false>): every wave carries both
//     layers, one wave per SIMD with the whole register file; same bits.
//   * The slab keeps RAW planes -- the stride-2 part reads them as before.  The B operand of (point, ci group, staged row) is
//     formed in registers from two ds_read_b128 and one vector add / subtract per k-step.  Even staged columns are stored in
//     front of odd ones (physical column (c & 1) * 17 + (c >> 1)): the 16 lanes of a read sit at columns 2n + const, which are
//     then neighbours, and a rotation of the 16-B channel slot by the column pair keeps them on 16 distinct slots (slab_off).
//   * Every accumulator tile is four, one per point; row packing over kh is unchanged.  Per wave and interior plane
//     4 points x 2 ci groups x (2 + 3 + 3 + 2) tiles x 4 k-steps = 320 MFMAs for 2 rows x 32 columns (240 for 2 x 16 before).
//     retire() forms y[2p], y[2p+1] in the order above, stores both and adds both to the BatchNorm sums.
//   * Stride-2 part: direct, K split by ci across the waves as before, over a 4 x 16 patch of outputs (four column tiles).
//
// U is computed in float64 from the float32 weights and rounded once, by the pre-layout (mvs_conv_wino_weight_layout) and by the
// in-kernel path alike: same bits.  A voxel's arithmetic does not depend on the range, chunk or segment that computes it.
#include "conv_common.h"
#include <cstdlib>
#include <cstdio>

namespace {

constexpr int TW = 32;                        // output columns of a tile = 16 MFMA columns
constexpr int TH = 8;
constexpr int PW = TW + 2;                     // 34 staged columns
constexpr int HP = PW / 2;                     // even columns in front, odd columns behind
constexpr int CIN = 32, COUT = 8, CQ = CIN / 4;
constexpr int COUT2 = 16;                      // stride-2 layer
constexpr int NPOS = (TH + 2) * PW;            // 340 staged positions
constexpr int NF4 = NPOS * CQ;                 // 2720 float4
constexpr int NROWS = 3 * COUT;                // 24
constexpr int WROW = NROWS * 4;                // floats per (tap, ci-quad)
constexpr int NPT = 4;                         // Winograd points
constexpr int W_FLOATS = 3 * NPT * CQ * WROW;  // 9216
constexpr int SP = CIN;                        // slab pitch (floats), swizzled
constexpr int ROWP = PW * SP;                  // floats per staged row
constexpr int SLAB_FLOATS = NPOS * SP;         // 10880
constexpr int KH_FLOATS = NPT * CQ * WROW;     // weight floats per kh
constexpr int NCT = 4;                         // stride-2 column tiles: (row pair, column half)
constexpr int RED_FLOATS = 3 * NCT * 64 * 4;   // partial stride-2 tiles of waves 1..3
constexpr int LDS_FLOATS = 2 * SLAB_FLOATS + W_FLOATS + 4 + RED_FLOATS;   // + zero block
constexpr int SLOTS = 256;                     // workgroups resident at once: one per CU

typedef float f32x2 __attribute__((ext_vector_type(2)));
typedef unsigned int u32x4_t __attribute__((ext_vector_type(4)));
constexpr int OOB = (int)0x80000000u;

// float offset of 16-B channel slot `slot` at staged (row, col).  Positions keep a 128-B pitch; the slot is rotated by twice the
// physical column pair.  A ds_read_b128 is served in groups of 16 lanes that hold 16 neighbouring physical columns, eight with
// k-quad a and eight with a + 1 (lanes 0-3, 12-15 | 4-11 of two quads): of the eight with the same column parity -- the same
// half of the 256-B bank row -- four carry a and four a + 1, and 2 x (column pair) puts the former on even and the latter on odd
// slots wherever the group starts (conv3d_c8.hip's XOR by the column pair is conflict-free only for groups that start on an even
// column, which half of this kernel's reads do not).  slot + 4 is still slot ^ 4: the second ci group stays an XOR of the offset.
__device__ __forceinline__ int slab_off(int row, int col, int slot) {
    const int pc = (col & 1) * HP + (col >> 1);
    return (row * PW + pc) * SP + (((slot + 2 * (pc >> 1)) & 7) << 2);
}

// point `pt` of the transformed weights of one (kd, kh, ci, co): float64, rounded once
__device__ __forceinline__ float wino_u(float g0, float g1, float g2, int pt) {
    if (pt == 0) return g0;
    if (pt == 3) return g2;
    const double s = (double)g0 + (double)g2;
    return (float)(0.5 * (pt == 1 ? s + (double)g1 : s - (double)g1));
}
// element i of the kernel's weight block [kh * 4 + point][ci / 4][kd][co][ci % 4] from TensorFlow's (3, 3, 3, 32, 8)
__device__ __forceinline__ float wino_weight(const float* __restrict__ w, int i) {
    const int j = i & 3;
    const int r = (i >> 2) % NROWS;
    const int g = (i >> 2) / NROWS;
    const int ciq = g % CQ, tap = g / CQ;
    const int kh = tap >> 2, pt = tap & 3;
    const int kd = r / COUT, co = r - kd * COUT;
    const float* p = w + ((size_t)((kd * 3 + kh) * 3) * CIN + ciq * 4 + j) * COUT + co;
    return wino_u(p[0], p[CIN * COUT], p[2 * CIN * COUT], pt);
}

__global__ void wino_weight_layout_kernel(const float* __restrict__ w, float* __restrict__ out) {
    const int i = blockIdx.x * blockDim.x + threadIdx.x;
    if (i < W_FLOATS) out[i] = wino_weight(w, i);
}

struct WinoArgs {
    const float* wprep;   // the 3dconv0_1 weights as wino_weight_layout_kernel leaves them, or null (then from a.w)
    const float* w2;      // stride-2 weights, TensorFlow layout (3,3,3,32,16)
    float* y2;            // (D/2, H/2, W/2, 16) raw output
    double* stats2;       // (2,16) float64 sums or null
    int slots1, slots2;   // partial rows of the two layers' sums (conv3d_c8.hip, FuseArgs)
    int span_g, span_m;   // SPAN schedule, as in conv3d_c8.hip
    int span_b[17];
    int full_sweeps;      // test hook MVS_HOOK_CONV_FULL_SWEEPS, as in conv3d_c8.hip
};

// W8: eight waves, two per SIMD, in two roles (the header comment); false: four waves that each carry both roles
template <bool SPAN, bool W8>
__global__ void __launch_bounds__(W8 ? 512 : 256, 1)
conv3d_c8_wino_kernel(ConvArgs a, WinoArgs fa) {
    extern __shared__ __attribute__((aligned(16))) float smem[];
    float* slab = smem;                            // [2][NPOS][SP]
    float* wl = smem + 2 * SLAB_FLOATS;            // [3 kh x 4 points][CQ][3 kd][8 co][4], then 4 zeros
    float* red = wl + W_FLOATS + 4;                // [3 waves][4 tiles][64 lanes][4]
    constexpr int ZOFF = W_FLOATS;

    const int tid = threadIdx.x;
    const int lane = tid & 63, wave = __builtin_amdgcn_readfirstlane(tid >> 6);   // scalar
    const int rw = W8 ? wave & 3 : wave;           // the wave's index inside its role: row pair (stride 1), ci quarter (stride 2)
    const int n = lane & 15, kq = lane >> 4;

    const int tiles_w = (a.W + TW - 1) / TW;
    // What this workgroup marches: one (tile, plane range), or with SPAN up to two -- the end of one tile's depth and the
    // start of the next tile's.
    int seg_tile[2], seg_d0[2], seg_d1[2], nseg = 1;
    if (SPAN) {
        // workgroup w -> XCD w % 8 (round-robin dispatch): an XCD works through consecutive groups, i.e. neighbouring tiles
        const int per_xcd = gridDim.x >> 3, j = blockIdx.x >> 3, x = blockIdx.x & 7;
        const int lin = (gridDim.x & 7) ? (int)blockIdx.x : x * per_xcd + j;
        const int grp = lin / fa.span_m, k = lin - grp * fa.span_m;
        const int lo = fa.span_b[k], hi_ = fa.span_b[k + 1];
        const int t0 = lo / a.D, t1 = (hi_ - 1) / a.D;
        seg_tile[0] = grp * fa.span_g + t0; seg_d0[0] = lo - t0 * a.D; seg_d1[0] = min(hi_, (t0 + 1) * a.D) - t0 * a.D;
        seg_tile[1] = grp * fa.span_g + t1; seg_d0[1] = 0; seg_d1[1] = hi_ - t1 * a.D;
        nseg = t1 != t0 ? 2 : 1;
    } else {
        seg_tile[0] = xcd_swizzle(blockIdx.x, gridDim.x);
        seg_d0[0] = blockIdx.z * a.planes_per_wg;
        seg_d1[0] = min(seg_d0[0] + a.planes_per_wg, a.D);
        seg_tile[1] = 0; seg_d0[1] = 0; seg_d1[1] = 0;
    }
    int h0 = (seg_tile[0] / tiles_w) * TH, w0 = (seg_tile[0] % tiles_w) * TW;
    int d0 = seg_d0[0], d1 = seg_d1[0];
    int T = d1 - d0 + 2;                           // input planes d0-1 .. d1

    // (by the 256 threads of the stride-1 role: W8's other half fetches its wS fragments and stages the first plane meanwhile)
    auto init_weights = [&]() __attribute__((always_inline)) {
        if (fa.wprep) copy_weights_to_lds(wl, fa.wprep, W_FLOATS);
        else for (int i = tid; i < W_FLOATS; i += 256) wl[i] = wino_weight(a.w, i);
        if (tid < 4) wl[ZOFF + tid] = 0.f;
    };

    // ---- staging ---------------------------------------------------------------------------------
    // every thread of the workgroup stages: 11 pieces of a plane with four waves, 6 with eight
    constexpr int NTH = W8 ? 512 : 256, NITW = (NF4 + NTH - 1) / NTH;
    const int c4 = tid % CQ;
    float4 pre[NITW];
    int goff[NITW], loff[NITW];
    auto set_goff = [&]() __attribute__((always_inline)) {
#pragma unroll
        for (int i = 0; i < NITW; ++i) {
            int f = tid + NTH * i;
            if (f >= NF4) f -= NTH;                // spare threads of the last piece redo their previous one
            int pos = f / CQ;
            int r = pos / PW, c = pos - r * PW;
            int gh = h0 - 1 + r, gw = w0 - 1 + c;
            bool inb = gh >= 0 && gh < a.H && gw >= 0 && gw < a.W;
            goff[i] = inb ? ((gh * a.W + gw) * CIN + 4 * c4) * 4 : OOB;      // byte offset inside a plane
            loff[i] = slab_off(r, c, c4);
        }
    };
    // Buffer addressing (the launcher guarantees < 2 GB tensors): 32-bit byte offsets, and an offset
    // with bit 31 set is out of range -> loads return 0 (= SAME padding), stores are dropped.
    const int plane_bytes = a.H * a.W * CIN * 4;
    const auto xrsrc = __builtin_amdgcn_make_buffer_rsrc((void*)a.x, 0, a.D * plane_bytes, 0x00020000);
    const auto yrsrc = __builtin_amdgcn_make_buffer_rsrc((void*)a.y, 0, a.D * a.H * a.W * COUT * 4, 0x00020000);

    // piece i of a plane's staging: global -> registers (load_piece), registers -> LDS (stage_piece)
    // (branch-free: these run between the MFMAs of the sweep)
    auto load_piece = [&](int i, int q) __attribute__((always_inline)) {
        const bool plane_ok = (q >= 0) && (q < a.D);
        u32x4_t v = __builtin_amdgcn_raw_buffer_load_b128(xrsrc, goff[i] | (plane_ok ? 0 : OOB),
                                                           plane_ok ? q * plane_bytes : 0, 0);
        pre[i] = make_float4(__uint_as_float(v[0]), __uint_as_float(v[1]), __uint_as_float(v[2]), __uint_as_float(v[3]));
    };
    auto stage_piece = [&](int i, float* buf) __attribute__((always_inline)) {
        *(float4*)(buf + loff[i]) = pre[i];
    };

    // ---- stride-1 accumulators, per point: [0],[1] = blocks 0|1 (rows 0-7 | 8-15) of output rows r, r+1;
    // [2] = block 2 of row r (rows 0-7) and of row r+1 (rows 8-15).  Block b carries kd = (P-b) mod 3.
    f32x4 acc[NPT][3];
#pragma unroll
    for (int p = 0; p < NPT; ++p)
#pragma unroll
        for (int i = 0; i < 3; ++i) acc[p][i] = (f32x4){0.f, 0.f, 0.f, 0.f};
    double st_s[4] = {0.0, 0.0, 0.0, 0.0}, st_q[4] = {0.0, 0.0, 0.0, 0.0};      // doubles: E[x^2] - E[x]^2 multiplies a float32 run's rounding by (mean / deviation)^2

    // raw operand d_c: staged row 2*rw + i (i = 0..3, an immediate), column 2n + c, slot kq (s = 1 is ^16)
    int bcol[4];
#pragma unroll
    for (int c = 0; c < 4; ++c) bcol[c] = slab_off(2 * rw, 2 * n + c, kq);
    const int hi = n >> 3;                         // 0: tile rows 0-7, 1: rows 8-15
    const int a_lane = (kq * NROWS + (n & 7)) * 4;

    // `extra(G)` is called once per step: the plane march hangs the next plane's staging on it so
    // that those VALU / LDS-write / global-load instructions issue in the shadow of the MFMAs.
    // TM (bit t = the tiles acc[.][t] are issued) is 7 on every plane but a range's first and last, whose other blocks retire() drops.
    auto sweep = [&](auto Pc, auto Mc, const float* buf, auto&& extra) __attribute__((always_inline)) {
        constexpr int P = decltype(Pc)::value, TM = decltype(Mc)::value;
        constexpr int KD_B0 = P % 3, KD_B1 = (P + 2) % 3, KD_B2 = (P + 1) % 3;
        const int a0 = a_lane + (hi ? KD_B1 : KD_B0) * COUT * 4;          // blocks 0|1
        const int ap = a_lane + KD_B2 * COUT * 4 - hi * KH_FLOATS;        // block 2: kh = i - hi
        f32x4 da[2], db[2], pv[2], av[3];
        // step G = ((pt*2 + s)*4 + i): staged row i against the weights of (point pt, ci group s)
        auto load_grp = [&](int G, int r) __attribute__((always_inline)) {
            const int i = G & 3, pt = G >> 3, s = (G >> 2) & 1;
            const int wconst = (pt * CQ + 4 * s) * WROW;
            if (r == 0) {
                // t_pt = d_ca -/+ d_cb
                const int ca = pt == 0 ? 0 : pt == 2 ? 2 : 1, cb = pt == 0 ? 2 : pt == 1 ? 2 : pt == 2 ? 1 : 3;
                da[G & 1] = *(const f32x4*)(buf + (bcol[ca] ^ (16 * s)) + i * ROWP);
                db[G & 1] = *(const f32x4*)(buf + (bcol[cb] ^ (16 * s)) + i * ROWP);
            } else if (r == 1) {
                int off = ap + i * KH_FLOATS + wconst;
                if (i == 0) off = hi ? ZOFF : off;       // rows 8-15 would need kh = -1
                if (i == 3) off = hi ? off : ZOFF;       // rows 0-7 would need kh = 3
                pv[G & 1] = *(const f32x4*)(wl + off);
            } else if (i < 3) av[i] = *(const f32x4*)(wl + a0 + i * KH_FLOATS + wconst);
        };
        constexpr int NG = 8 * NPT;
        f32x4 bt[2];
        auto form = [&](int G) __attribute__((always_inline)) {
            bt[G & 1] = (G >> 3) == 1 ? da[G & 1] + db[G & 1] : da[G & 1] - db[G & 1];
        };
#pragma unroll
        for (int r = 0; r < 3; ++r) load_grp(0, r);
        form(0);
        // Four waves: nothing else fills the matrix pipe while this wave issues anything but an MFMA (with eight, the SIMD's
        // stride-2 wave does).  So the next step's operand reads, its add / subtract and the staging piece are spread over the four k-steps of the current one, each
        // behind a group of 2-3 MFMAs (64-96 clocks of matrix work): raw operands after k-step 0, weights after k-step 1, the
        // transformed operand (its reads are two MFMA groups old by then) after k-step 2, staging after k-step 3.
#pragma unroll
        for (int G = 0; G < NG; ++G) {
            const int i = G & 3, pt = G >> 3;
            const int NC = (i == 0 || i == 3) ? 2 : 3;      // MFMA tiles of this step
#pragma unroll
            for (int j = 0; j < 4; ++j) {
#pragma unroll
                for (int c = 0; c < NC; ++c) {
                    // i = 0: row r kh 0 | packed;  i = 1,2: row r+1 kh i-1 | row r kh i | packed;  i = 3: row r+1 kh 2 | packed
                    int t; float aval;
                    if (c == NC - 1) { t = 2; aval = pv[G & 1][j]; }
                    else if (i == 0) { t = 0; aval = av[0][j]; }
                    else if (c == 0) { t = 1; aval = av[i - 1][j]; }
                    else { t = 0; aval = av[i][j]; }
                    if ((TM >> t) & 1) acc[pt][t] = __builtin_amdgcn_mfma_f32_16x16x4f32(aval, bt[G & 1][j], acc[pt][t], 0, 0, 0);
                }
                if (G + 1 < NG) {
                    if (j == 0) load_grp(G + 1, 0);
                    if (j == 1) { load_grp(G + 1, 1); load_grp(G + 1, 2); }
                    if (j == 2) form(G + 1);
                }
                if (j == 3) extra(G);
                __builtin_amdgcn_sched_barrier(0);
            }
        }
    };

    // store + zero the block that has just received kd = 2 (block (P+1)%3), output plane o
    // per-lane byte offsets inside an output plane, of column w0 + 2n (its neighbour 2n + 1 follows 32 bytes behind; W is even):
    // rows r, r+1 (blocks 0|1) and r + (kq>>1) (block 2)
    int yoff[3];
    auto set_yoff = [&]() __attribute__((always_inline)) {
        const int w = w0 + 2 * n, co = 4 * (kq & 1);
        const int hs[3] = {h0 + 2 * rw, h0 + 2 * rw + 1, h0 + 2 * rw + (kq >> 1)};
#pragma unroll
        for (int i = 0; i < 3; ++i)
            yoff[i] = (hs[i] < a.H && w < a.W) ? ((hs[i] * a.W + w) * COUT + co) * 4 : OOB;
    };
    const int yplane_bytes = a.H * a.W * COUT * 4;
    auto retire = [&](auto Pc, int o) __attribute__((always_inline)) {
        constexpr int P = decltype(Pc)::value;
        constexpr int B = (P + 1) % 3;
        const bool plane_ok = (o >= d0) && (o < d1);
        auto emit = [&](int t, int yo) __attribute__((always_inline)) {
            // (the squares are explicit fused multiply-adds: left to the compiler, one inlined copy of this code contracted them and
            //  another did not, and the float32 partial sums then depended on which plane body retired a block)
            if (plane_ok) {
                const f32x4 m0 = acc[0][t], m1 = acc[1][t], m2 = acc[2][t], m3 = acc[3][t];
                f32x4 y[2];
                y[0] = (m0 + m1) + m2;
                y[1] = (m1 - m2) - m3;
#pragma unroll
                for (int e = 0; e < 2; ++e) {
                    u32x4_t v = {__float_as_uint(y[e][0]), __float_as_uint(y[e][1]), __float_as_uint(y[e][2]), __float_as_uint(y[e][3])};
                    __builtin_amdgcn_raw_buffer_store_b128(v, yrsrc, yo + e * COUT * 4 + o * yplane_bytes, 0, 0);
                    if (yo >= 0) {
#pragma unroll
                        for (int k = 0; k < 4; ++k) { const double v = (double)y[e][k]; st_s[k] += v; st_q[k] = fma(v, v, st_q[k]); }
                    }
                }
            }
#pragma unroll
            for (int p = 0; p < NPT; ++p) acc[p][t] = (f32x4){0.f, 0.f, 0.f, 0.f};
        };
        if (B < 2) {
            if ((kq >> 1) == B) { emit(0, yoff[0]); emit(1, yoff[1]); }
        } else {
            emit(2, yoff[2]);
        }
    };

    // ---- stride-2 part ---------------------------------------------------------------------------
    // Column tile ct = (rt, wt), lane column n: output (oh, ow) = (h0/2 + 2rt + (n>>3), w0/2 + 8wt + (n&7)); input tap
    // (kh, kw) sits at staged (row 4rt + 2(n>>3) + kh + 1, col 16wt + 2(n&7) + kw + 1).  This wave's k index
    // kq of step j is input channel 8*rw + 2kq + j (one ds_read_b64 per tap and tile).
    float wS[3][9][2];
    f32x4 cur[NCT], prv[NCT];                      // output planes od_cur / od_cur - 1, per column tile
    int s2b[3][2];
    double st2_s[4] = {0.0, 0.0, 0.0, 0.0}, st2_q[4] = {0.0, 0.0, 0.0, 0.0};
    int fin_od = -1;                               // output plane whose partial tiles wait in `red`
    const int Ho = a.H / 2, Wo = a.W / 2;
    auto init_s2 = [&]() __attribute__((always_inline)) {
#pragma unroll
        for (int kd = 0; kd < 3; ++kd)
#pragma unroll
            for (int tap = 0; tap < 9; ++tap)
#pragma unroll
                for (int j = 0; j < 2; ++j)
                    wS[kd][tap][j] = fa.w2[((size_t)(kd * 9 + tap) * CIN + 8 * rw + 2 * kq + j) * COUT2 + n];
#pragma unroll
        for (int kw = 0; kw < 3; ++kw)
#pragma unroll
            for (int wt = 0; wt < 2; ++wt)
                s2b[kw][wt] = slab_off(2 * (n >> 3), 16 * wt + 2 * (n & 7) + kw + 1, 2 * rw + (kq >> 1)) + 2 * (kq & 1);
#pragma unroll
        for (int ct = 0; ct < NCT; ++ct) { cur[ct] = (f32x4){0.f, 0.f, 0.f, 0.f}; prv[ct] = cur[ct]; }
    };

    // `extra2(tap)` is called once per tap: with eight waves the plane staging hangs on it, as it hangs on the sweep's extra(G)
    // with four
    auto s2_sweep = [&](auto Ec, const float* buf, auto&& extra2) __attribute__((always_inline)) {
        // 0: odd plane, kd 1 -> cur;  1: even plane, kd 0 -> cur, kd 2 -> prv;  2: the even plane that ends a range, kd 2 -> prv
        // only (the output plane it would start belongs to the next range)
        constexpr int MODE = decltype(Ec)::value;
        f32x2 b2[2][NCT];
        auto ld = [&](int tap, f32x2 (&b)[NCT]) __attribute__((always_inline)) {
            const int kh = tap / 3, kw = tap % 3;
#pragma unroll
            for (int ct = 0; ct < NCT; ++ct) b[ct] = *(const f32x2*)(buf + s2b[kw][ct & 1] + (4 * (ct >> 1) + kh + 1) * ROWP);
        };
        ld(0, b2[0]);
#pragma unroll
        for (int tap = 0; tap < 9; ++tap) {
            if (tap + 1 < 9) ld(tap + 1, b2[(tap + 1) & 1]);
#pragma unroll
            for (int j = 0; j < 2; ++j)
#pragma unroll
                for (int ct = 0; ct < NCT; ++ct) {
                    const float bval = b2[tap & 1][ct][j];
                    if (MODE) {
                        if (MODE == 1) cur[ct] = __builtin_amdgcn_mfma_f32_16x16x4f32(wS[0][tap][j], bval, cur[ct], 0, 0, 0);
                        prv[ct] = __builtin_amdgcn_mfma_f32_16x16x4f32(wS[2][tap][j], bval, prv[ct], 0, 0, 0);
                    } else {
                        cur[ct] = __builtin_amdgcn_mfma_f32_16x16x4f32(wS[1][tap][j], bval, cur[ct], 0, 0, 0);
                    }
                }
            extra2(tap);
            __builtin_amdgcn_sched_barrier(0);
        }
    };
    // the waves' K-quarters of the output plane that has just completed -> `red`, summed by the role's first wave after the next
    // barrier
    auto s2_park = [&](int od) __attribute__((always_inline)) {
        if (rw > 0) {
#pragma unroll
            for (int ct = 0; ct < NCT; ++ct)
                *(f32x4*)(red + (((rw - 1) * NCT + ct) * 64 + lane) * 4) = prv[ct];
        }
        fin_od = od;
    };
    // the role's first wave: sum the four K-quarters of output plane fin_od, store, BatchNorm sums
    auto s2_finish = [&]() __attribute__((always_inline)) {
        if (fin_od >= 0 && rw == 0) {
#pragma unroll
            for (int ct = 0; ct < NCT; ++ct) {
                f32x4 r = prv[ct];
#pragma unroll
                for (int w = 0; w < 3; ++w) {
                    f32x4 p = *(const f32x4*)(red + ((w * NCT + ct) * 64 + lane) * 4);
                    r[0] += p[0]; r[1] += p[1]; r[2] += p[2]; r[3] += p[3];
                }
                const int oh = h0 / 2 + 2 * (ct >> 1) + (n >> 3), ow = w0 / 2 + 8 * (ct & 1) + (n & 7);
                if (oh < Ho && ow < Wo) {
                    float* dst = fa.y2 + ((((size_t)fin_od * Ho + oh) * Wo) + ow) * COUT2 + 4 * kq;
                    *(float4*)dst = make_float4(r[0], r[1], r[2], r[3]);
#pragma unroll
                    for (int k = 0; k < 4; ++k) { const double v = (double)r[k]; st2_s[k] += v; st2_q[k] = fma(v, v, st2_q[k]); }
                }
            }
        }
        fin_od = -1;
    };

    // ---- plane march (conv3d_c8.hip: same steps, same halo-plane rules) ---------------------------
    // Plane q is swept while plane q+1 moves registers -> LDS (steps 4..14 with four waves) and plane q+2 is requested from global
    // memory (steps 16..26).  A range [d0, d1) stages the input planes d0 - 1 .. d1 (t = 0 .. T - 1, P = t % 3); its first plane issues
    // only the tiles acc[.][0] | acc[.][1] (kd = 0 of output d0), its last only the block that retires (kd = 2 of output d1 - 1)
    // and the kd = 2 half of the stride-2 part; planes outside the volume issue nothing.  fa.full_sweeps = 1 runs plane() on all
    // T planes, 2 on all inside the volume.
    //
    // The whole march is written once per ROLE: 0 = both layers in every wave (four waves), 1 = the stride-1 layer alone (waves
    // 0-3 of eight), 2 = the stride-2 layer alone (waves 4-7 of eight).  Every role passes the same barriers: the prologue's and
    // one per plane.  Every thread stages its NITW pieces of a plane in every role (all of them on waves 4-7 took 256 registers
    // and 29-44 spilled ones).  Roles 0 and 1 hang them on the sweep's extra(G); role 2 hangs them between the stride-2 taps
    // (extra2), and on a plane without a stride-2 sweep -- outside the volume, before the range's first stride-2 plane, a
    // first_plane -- it stages them in a row.
    auto march = [&](auto Rc) __attribute__((always_inline)) {
        constexpr int ROLE = decltype(Rc)::value;
        constexpr bool S1 = ROLE != 2, S2 = ROLE != 1;
        if (S1) {
            init_weights();
            set_yoff();      // (a raised issue priority for role 1 from here on measured a tie: EXPERIMENTS, pair-roles addendum)
        }
        set_goff();
        if (S2) init_s2();

        auto prologue = [&](int t0) __attribute__((always_inline)) {
            float* buf = slab + (t0 & 1) * SLAB_FLOATS;
#pragma unroll
            for (int i = 0; i < NITW; ++i) load_piece(i, d0 - 1 + t0);
#pragma unroll
            for (int i = 0; i < NITW; ++i) stage_piece(i, buf);
#pragma unroll
            for (int i = 0; i < NITW; ++i) load_piece(i, d0 + t0);
            __syncthreads();
        };
        // staging of the plane after the one being swept: item k < NITW moves piece k registers -> LDS, item NITW + k requests
        // piece k of the plane after that (past the last plane these stage / request planes nobody reads: harmless, and branch-free)
        auto stage_item = [&](int k, float* nxt, int q) __attribute__((always_inline)) {
            if (k < NITW) stage_piece(k, nxt); else load_piece(k - NITW, q + 2);
        };
        auto stage_all = [&](float* nxt, int q) __attribute__((always_inline)) {
#pragma unroll
            for (int k = 0; k < 2 * NITW; ++k) stage_item(k, nxt, q);
        };

        auto plane = [&](auto Pc, int t) __attribute__((always_inline)) {
            const int q = d0 - 1 + t;
            float* cur_buf = slab + (t & 1) * SLAB_FLOATS;
            float* nxt = slab + ((t + 1) & 1) * SLAB_FLOATS;
            const bool in_vol = (q >= 0) && (q < a.D);
            auto extra = [&](int G) __attribute__((always_inline)) {
                if (S1) {
                    if (G >= 4 && G < 4 + NITW) stage_piece(G - 4, nxt);
                    if (G >= 16 && G < 16 + NITW) load_piece(G - 16, q + 2);
                }
            };
            // role 2: the 12 items over the nine taps, 1-2 behind each tap's 8 or 16 MFMAs
            auto extra2 = [&](int tap) __attribute__((always_inline)) {
                if (ROLE == 2) {
#pragma unroll
                    for (int k = 0; k < 2 * NITW; ++k)
                        if (k >= tap * 2 * NITW / 9 && k < (tap + 1) * 2 * NITW / 9) stage_item(k, nxt, q);
                }
            };
            if (S2) s2_finish();
            if (S1) sweep(Pc, std::integral_constant<int, 7>{}, cur_buf, extra);      // planes outside the volume are staged as zeros
            if (S2) {
                const bool even = q >= d0 && !(q & 1);
                const bool swept = q >= d0 && in_vol;
                if (even) {
                    // plane q = 2*od_cur: od_cur starts (kd 0), od_cur - 1 completes (kd 2)
#pragma unroll
                    for (int ct = 0; ct < NCT; ++ct) { prv[ct] = cur[ct]; cur[ct] = (f32x4){0.f, 0.f, 0.f, 0.f}; }
                }
                if (swept) {
                    if (q & 1) s2_sweep(std::false_type{}, cur_buf, extra2);
                    else s2_sweep(std::true_type{}, cur_buf, extra2);
                } else if (ROLE == 2) {
                    stage_all(nxt, q);
                }
                if (even) {
                    const int od_prev = q / 2 - 1;
                    if (2 * od_prev >= d0) s2_park(od_prev);
                }
            }
            if (S1) retire(Pc, q - 1);
            __syncthreads();
        };
        // t = 0 of a range that starts inside the volume (P = 0)
        auto first_plane = [&]() __attribute__((always_inline)) {
            const int q = d0 - 1;
            float* nxt = slab + SLAB_FLOATS;
            auto extra = [&](int G) __attribute__((always_inline)) {
                if (S1) {
                    if (G >= 4 && G < 4 + NITW) stage_piece(G - 4, nxt);
                    if (G >= 16 && G < 16 + NITW) load_piece(G - 16, q + 2);
                }
            };
            if (S1) {
                sweep(std::integral_constant<int, 0>{}, std::integral_constant<int, 3>{}, slab, extra);
                retire(std::integral_constant<int, 0>{}, q - 1);      // (zeroes what block 1 took)
            }
            if (ROLE == 2) stage_all(nxt, q);
            __syncthreads();
        };
        // t = T - 1, plane d1
        auto last_plane = [&](auto Pc) __attribute__((always_inline)) {
            constexpr int P = decltype(Pc)::value;
            const int q = d1;
            const float* cur_buf = slab + ((T - 1) & 1) * SLAB_FLOATS;
            const bool in_vol = q < a.D;
            if (S2) s2_finish();
            if (S1 && in_vol) sweep(Pc, std::integral_constant<int, (P + 1) % 3 == 2 ? 4 : 3>{}, cur_buf, [](int) {});
            if (S2) {
                // plane q = 2*od_cur completes od_cur - 1 (kd 2); od_cur is another range's
#pragma unroll
                for (int ct = 0; ct < NCT; ++ct) { prv[ct] = cur[ct]; cur[ct] = (f32x4){0.f, 0.f, 0.f, 0.f}; }
                if (in_vol) s2_sweep(std::integral_constant<int, 2>{}, cur_buf, [](int) {});
                const int od_prev = q / 2 - 1;
                if (2 * od_prev >= d0) s2_park(od_prev);
            }
            if (S1) retire(Pc, q - 1);
            __syncthreads();
        };
        for (int sg = 0; sg < (SPAN ? nseg : 1); ++sg) {
            if (SPAN && sg > 0) {
                // second segment: another tile, its first planes.  Whatever the first march left in the accumulators belongs to
                // planes past its range; the last stride-2 plane of the first range is flushed before its partials are
                // overwritten.  Each role resets its own state.
                if (S2) s2_finish();
                h0 = (seg_tile[1] / tiles_w) * TH; w0 = (seg_tile[1] % tiles_w) * TW;
                d0 = seg_d0[1]; d1 = seg_d1[1]; T = d1 - d0 + 2;
                set_goff();
                if (S1) {
                    set_yoff();
#pragma unroll
                    for (int p = 0; p < NPT; ++p)
#pragma unroll
                        for (int i = 0; i < 3; ++i) acc[p][i] = (f32x4){0.f, 0.f, 0.f, 0.f};
                }
                if (S2) {
#pragma unroll
                    for (int ct = 0; ct < NCT; ++ct) { cur[ct] = (f32x4){0.f, 0.f, 0.f, 0.f}; prv[ct] = cur[ct]; }
                }
            }
            // planes [t_lo, t_hi) run plane(); T >= 3, so the first and the last plane are two planes
            const bool trim_first = fa.full_sweeps == 0 || (fa.full_sweeps == 2 && d0 == 0);
            const bool trim_last = fa.full_sweeps == 0 || (fa.full_sweeps == 2 && d1 == a.D);
            const int t_lo = trim_first ? 1 : 0, t_hi = trim_last ? T - 1 : T;
            prologue(trim_first && d0 == 0 ? 1 : 0);
            if (trim_first && d0 > 0) first_plane();
            for (int t = 0; t < t_hi; t += 3) {
                if (t >= t_lo) plane(std::integral_constant<int, 0>{}, t);
                if (t + 1 < t_hi) plane(std::integral_constant<int, 1>{}, t + 1);
                if (t + 2 < t_hi) plane(std::integral_constant<int, 2>{}, t + 2);
            }
            if (trim_last) {
                const int pl = (T - 1) % 3;
                if (pl == 0) last_plane(std::integral_constant<int, 0>{});
                else if (pl == 1) last_plane(std::integral_constant<int, 1>{});
                else last_plane(std::integral_constant<int, 2>{});
            }
        }
        if (S2) {
            s2_finish();
            // 3dconv1_0's sums stay on the wave that finished the tiles
            if (fa.stats2 && rw == 0) {
#pragma unroll
                for (int k = 0; k < 4; ++k) {
                    double sv = st2_s[k], qv = st2_q[k];
#pragma unroll
                    for (int o = 8; o > 0; o >>= 1) { sv += __shfl_xor(sv, o, 64); qv += __shfl_xor(qv, o, 64); }
                    if (n == 0) {
                        double* s2p = fa.stats2 + (size_t)((blockIdx.x + gridDim.x * blockIdx.z) % fa.slots2) * 2 * COUT2;
                        atomicAdd(&s2p[4 * kq + k], sv);
                        atomicAdd(&s2p[COUT2 + 4 * kq + k], qv);
                    }
                }
            }
        }
    };
    // (a scalar branch: each role's registers are allocated by themselves, the kernel takes the larger set)
    if (!W8) march(std::integral_constant<int, 0>{});
    else if (wave < 4) march(std::integral_constant<int, 1>{});
    else march(std::integral_constant<int, 2>{});

    // every lane's st_* are the sums of channels 4*(kq&1) .. +3: fold lanes l and l^32.  stats_commit adds the rows of waves 0-3;
    // with eight waves the other four pass zeros into rows 4-7 (8 x 32 floats of the slab, which is dead by now)
    if (a.stats) stats_commit<COUT>(st_s, st_q, true, slab,
                                    a.stats + (size_t)((blockIdx.x + gridDim.x * blockIdx.z) % fa.slots1) * 2 * COUT,
                                    a.cout_total, 0);
}

}  // namespace

int mvs_conv_wino_weight_layout(const float* w, float* out, hipStream_t st) {
    wino_weight_layout_kernel<<<mvs_cdiv(W_FLOATS, 256), 256, 0, st>>>(w, out);
    return (int)hipGetLastError();
}

// The schedule is launch_c8<true>'s (conv3d_c8.hip) at this kernel's tile and residency: 8 x 32 tiles, one workgroup per CU.
// At the metric workload 80 tiles x 192 planes meet 256 slots: SPAN takes 5 tiles / 16 workgroups, ranges of 60 planes.
int mvs_conv3d_c8_wino_s2_launch(const ConvArgs& a0, const float* wprep_wino, const float* w2, float* y2, double* stats2,
                                 hipStream_t st, int slots1, int slots2) {
    ConvArgs a = a0;
    WinoArgs fa = {wprep_wino, w2, y2, stats2, slots1 > 1 ? slots1 : 1, slots2 > 1 ? slots2 : 1};
    fa.full_sweeps = mvs_hook(MVS_HOOK_CONV_FULL_SWEEPS) & 3;
    // test hooks: planes per workgroup (whole chunks then, no SPAN), or SPAN with a given (G, M)
    const int hk_planes = mvs_hook(MVS_HOOK_PAIR_PLANES), hk_span = mvs_hook(MVS_HOOK_SPAN_FORCE);
    if (a.x2 || a.xs || a.bn.stats || a.cout_total != COUT || (a.D & 1) || (a.H & 1) || (a.W & 1)) return MVS_E_SHAPE;
    if ((long long)a.D * a.H * a.W * CIN * 4 >= (1LL << 31)) return MVS_E_SHAPE;   // 32-bit buffer offsets
    const int tiles = ((a.H + TH - 1) / TH) * ((a.W + TW - 1) / TW);
    {
        // chunks start on even planes so that stride-2 output planes never straddle workgroups
        int best = 2; long long best_cost = 1LL << 60;
        for (int dr = 2; dr <= a.D; dr += 2) {
            long long wgs = (long long)tiles * ((a.D + dr - 1) / dr);
            long long cost = ((wgs + SLOTS - 1) / SLOTS) * (dr + 3);
            if (cost < best_cost) { best_cost = cost; best = dr; }
        }
        a.planes_per_wg = best;
    }
    if (hk_planes) a.planes_per_wg = hk_planes < a.D ? hk_planes : a.D;
    dim3 grid(tiles, 1, (a.D + a.planes_per_wg - 1) / a.planes_per_wg);
    const size_t smem = (size_t)LDS_FLOATS * sizeof(float);
    static bool attr_done = false;
    if (!attr_done) {
        const void* kernels[4] = {(const void*)conv3d_c8_wino_kernel<false, false>, (const void*)conv3d_c8_wino_kernel<true, false>,
                                  (const void*)conv3d_c8_wino_kernel<false, true>, (const void*)conv3d_c8_wino_kernel<true, true>};
        for (const void* k : kernels) {
            hipError_t e = hipFuncSetAttribute(k, hipFuncAttributeMaxDynamicSharedMemorySize, (int)smem);
            if (e != hipSuccess) return (int)e;
        }
        attr_done = true;
    }
    // eight waves in two roles unless the test hook asks for the four-wave instantiation (same bits)
    const bool w8 = !mvs_hook(MVS_HOOK_PAIR_WAVES4);
    // SPAN schedule: groups of G tiles share M workgroups that cut the tiles' concatenated depth into M equal ranges; a range may
    // cross one tile boundary.  Taken when it costs fewer plane steps than whole chunks.
    if (!mvs_hook(MVS_HOOK_CONV_NO_SPAN) && !hk_planes) {      // (test hook: whole depth chunks, the schedule SPAN replaces)
        const long long chunk_cost = (((long long)tiles * grid.z + SLOTS - 1) / SLOTS) * (a.planes_per_wg + 3);
        int bg = 0, bm = 0; long long bcost = chunk_cost;
        // MVS_HOOK_SPAN_FORCE = G << 8 | M: that pair alone is looked at, at any range length and whatever it costs (tests
        // reach ranges that cross a tile boundary at small sizes); a pair that breaks the other rules falls back to chunks
        const int fg = hk_span >> 8, fm = hk_span & 255;
        for (int G = 1; G <= 8; ++G) {
            if (tiles % G || (hk_span && G != fg)) continue;
            for (int M = G; M <= 16; ++M) {
                if (hk_span && M != fm) continue;
                const int total = G * a.D;
                if (total % M || (long long)(tiles / G) * M > SLOTS) continue;
                const int L = total / M;
                if ((L & 1) || (L < 32 && !hk_span) || L > a.D) continue;      // even starts (stride-2 planes), at most one boundary per range
                const long long cost = L + 3 + ((a.D % L) ? 2 : 0);
                if (cost < bcost || hk_span) { bcost = cost; bg = G; bm = M; }
            }
        }
        if (bg) {
            fa.span_g = bg; fa.span_m = bm;
            for (int k = 0; k <= bm; ++k) fa.span_b[k] = k * (bg * a.D / bm);
            if (w8) conv3d_c8_wino_kernel<true, true><<<dim3((tiles / bg) * bm), 512, smem, st>>>(a, fa);
            else conv3d_c8_wino_kernel<true, false><<<dim3((tiles / bg) * bm), 256, smem, st>>>(a, fa);
            return (int)hipGetLastError();
        }
    }
    if (w8) conv3d_c8_wino_kernel<false, true><<<grid, 512, smem, st>>>(a, fa);
    else conv3d_c8_wino_kernel<false, false><<<grid, 256, smem, st>>>(a, fa);
    return (int)hipGetLastError();
}
