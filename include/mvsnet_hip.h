/* mvsnet_hip.h -- C ABI of libmvsnet_hip.so (MI355X / gfx950 plane-sweep depth inference).
 *
 * The reference (ubiquity6/MVSNet) has NO plugin / operator / FFI interface: its seam is a set of
 * Python functions building one TensorFlow graph.  This header is therefore the new
 * drop-in boundary: one entry point per reference function on the hot path, cited below.  The
 * Python host side (mvsnet_amd/model.py, same names and argument meaning as mvsnet/model.py) binds
 * these through ctypes; INTEGRATION.md shows the stub a reference maintainer would add.
 *
 * Conventions (all entry points):
 *   - every pointer is a DEVICE pointer owned by the caller unless marked [host];
 *   - tensors are float32, channel-last, contiguous: images (H,W,C), volumes (D,H,W,C);
 *   - functions enqueue kernels on `stream` (a hipStream_t passed as void*; NULL = default
 *     stream); they never allocate, never free, never synchronise, never create streams or events -- so a
 *     whole pass captures into a hipGraph.  The exceptions are named where they are declared and are all set-up /
 *     tear-down / diagnostic calls, never compute calls: mvs_gru_prepare and mvs_gru_release (create / destroy the
 *     recurrent sweep's side streams and events, synchronise), and the profiling read-outs mvs_profile_dominant_ms /
 *     mvs_profile_layers_ms (wait for their timing events);
 *   - return value: 0 on success, a positive hipError_t on a HIP failure, a negative
 *     MVS_E_* code on an argument error.  Nothing throws.
 *
 * Memory contract of the hot path (homographies, warp, cost volume, the 3-D convolutions, RegNetUS0, soft-argmin, the ConvGRU
 * stages and the recurrent sweep, the 2-D tower layers and the training kernels; tests/test_gpu_arena.py runs each of them with
 * every operand in one poisoned, guarded arena, tests/device_arena.py):
 *   - alignment: 16 bytes for every tensor, statistics, prepared-weight and workspace pointer is enough for every entry point
 *     (the kernels move channel quads as 16-byte packets and float64 sums as 8-byte words).  Nothing needs more: a workspace is
 *     carved at 256-byte multiples of ITS OWN start, whatever that is, and no kernel assumes the 256 or 512 bytes an allocator
 *     usually gives.  Only mvs_center_images_u8_f32 checks its pointers (images 4 bytes, out4 16: MVS_E_SHAPE);
 *   - every element of every output is written by the call, whatever the output held before -- except where an argument is
 *     documented as an accumulator the caller clears (the float64 `stats` / `sums` / `stats_out`, the gradients of
 *     mvs_cost_volume_bwd_f32, the running maps of mvs_wta_update_f32) or as updated in place (`h` of mvs_gru_blend_f32);
 *   - scratch holds anything on entry: workspaces (exactly mvs_*_workspace_bytes() bytes suffice), and the transforms / cost /
 *     reg buffers of mvs_depth_from_features_f32, are written before they are read, so one workspace may serve calls of
 *     changing shape back to back on a stream, and NaN or stale values left in it change nothing;
 *   - nothing outside the stated extents is written: not a byte before or after an output or a workspace, and inputs, weights
 *     and affines are never modified.  A call refused with MVS_E_WORKSPACE has enqueued nothing and written nothing;
 *   - the result does not depend on what lies outside the inputs: SAME padding and out-of-image taps are zeros (or clamped
 *     taps) formed by the kernels, and no load leaves a tensor's extent.
 *
 * Memory contract of the geometry entry points (everything declared from mvs_fusion_workspace_bytes to the end of this header:
 * fusion, point cloud, render, view selection, TSDF and surface nets, raster, mesh components; tests/test_gpu_arena_geometry.py
 * runs each of them in the same arena and lists, piece by piece, what first writes every workspace word).  The five rules above
 * hold for them as well, with these particulars:
 *   - alignment: 16 bytes for every pointer is enough in every family, workspaces included (they are carved at 256-byte
 *     multiples of their own start; the widest accesses are the 16-byte points and normals of the sorted copies and the normal
 *     map, and 8-byte keys, masks, queue entries and sums).  No entry point checks alignment and none needs more;
 *   - accumulators the caller clears before the first call, and which a later call continues: sum, count, rgb_sum and rgb_count
 *     of mvs_tsdf_integrate_f32 (every node is read, added to and stored back), and the mask of mvs_view_visibility_f32 (bits are
 *     ORed in; bits the call's views do not name are kept).  Nothing else has to be cleared by the caller;
 *   - outputs that the call stores whatever they held (none of them is added to): count of mvs_fusion_f32 / mvs_fusion_normals_f32
 *     and of mvs_voxel_select_f32, moments of mvs_icp_step_f32, out of mvs_dist_stats_f32 (2 + n_thresholds doubles), totals of
 *     mvs_surface_nets_count_f32, score_sum and shared of mvs_view_scores_f32 (all V x V entries, zeros where a >= b), hist of
 *     mvs_view_depth_hist_f32 (all V x (pass + 1) x 65536 bins), vertex_keep of mvs_mesh_compact_mark_i32, counts and boxes of
 *     mvs_mesh_components_measure_f32, depth and index of the two z-buffer calls;
 *   - capacity outputs are written up to what is produced and not a byte further: xyz, rgb, normals, view_index and pixel_index
 *     of the fusion calls and out of mvs_voxel_select_f32 hold *count entries and are untouched from entry *count on; vertices,
 *     colours and faces of mvs_surface_nets_write_f32 are untouched beyond the totals of the count call when M or F is larger
 *     (and not written at all when an axis has one node); out_vertices, out_colours and out_faces of mvs_mesh_compact_write_f32
 *     are untouched beyond the last rank when M_out or F_out is larger;
 *   - workspaces hold anything on entry and every word a call reads was written earlier in that call (counters, cell starts,
 *     used / keep flags, the z-buffer keys, the raster queue's counter and the 64 status words are cleared by the call), so
 *     one workspace serves calls of changing shape back to back.  Four workspaces carry state to a LATER call, which reads
 *     them as the earlier call left them and needs the same sizes and grid: mvs_nn_f32 -> mvs_nn_query_f32 and
 *     mvs_nn_target_build_f32 -> mvs_icp_step_f32 (both readers take the workspace as const and do not write it),
 *     mvs_mesh_components_label_i32 -> mvs_mesh_components_measure_f32 (which stores status word 2), and
 *     mvs_surface_nets_count_f32 -> the caller's two scans -> mvs_surface_nets_write_f32 (which only reads it);
 *   - a call that returns MVS_E_BADARG, MVS_E_SHAPE or MVS_E_WORKSPACE has enqueued nothing: outputs, accumulators and the
 *     workspace hold what they held.  mvs_*_workspace_bytes() is exact: one byte less is refused.
 */
#ifndef MVSNET_HIP_H_
#define MVSNET_HIP_H_

#include <stddef.h>
#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

#define MVS_ABI_VERSION 1

#define MVS_E_BADARG   (-1)   /* null pointer / non-positive size                         */
#define MVS_E_SHAPE    (-2)   /* shape not supported by this build (see function comment) */
#define MVS_E_WORKSPACE (-3)  /* workspace too small                                      */
#define MVS_E_NOT_PREPARED (-4) /* mvs_gru_prepare on a stream under hipGraph capture (it synchronises);
                                   mvs_gru_stream_layout on a stream without a set */
#define MVS_E_NO_SLOT  (-5)   /* mvs_gru_prepare: all 16 stream sets of the process are in use (mvs_gru_release frees one).
                                   Not fatal for the sweep: without a set it runs on the caller's stream alone */

/* Regulariser implementation selector (mvs_set_conv_impl): the MFMA path is the product;
 * the scalar path is a slow, shape-generic HIP cross-check (never a CPU fallback). */
#define MVS_CONV_IMPL_AUTO   0
#define MVS_CONV_IMPL_SCALAR 1
#define MVS_CONV_IMPL_MFMA   2
/* opt-in: stride-1 MFMA layers evaluate fp32 products as three bf16 MFMAs (x = hi + lo split,
 * fp32 accumulate, ~1.5e-5 relative error per product); only through mvs_regnet_us0_prepared_f32 */
#define MVS_CONV_IMPL_BF16X3 3

int mvs_abi_version(void);
/* Static description of a return code (never NULL). */
const char* mvs_error_string(int code);
int mvs_set_conv_impl(int impl);
int mvs_get_conv_impl(void);

/* Test / measurement hooks.  The library reads NOTHING from the environment: every switch that lets a test reach a schedule the
 * launchers would not pick by themselves is one of these process-wide integers (atomic; read at launch time, so set them while
 * no call of the library is in flight).  Results never depend on them except where stated; 0 (or the stated default) = the
 * product behaviour.  mvs_set_test_hook returns MVS_E_BADARG for an unknown id or a value outside the hook's range and leaves
 * the hook unchanged; mvs_get_test_hook returns the current value (or MVS_E_BADARG). */
#define MVS_HOOK_CV_TILE_ROWS_LOG2    0  /* warp + variance: force the wave tile to 2^v rows (v = 0..3); -1 (default) = voted from the transforms.  Same bits */
#define MVS_HOOK_CONV_NO_SPAN         1  /* 1: 3dconv0_1 + 1_0 launch walks whole depth chunks instead of SPAN ranges.  Same bits */
#define MVS_HOOK_CONV_NO_FUSE2        2  /* 1: 3dconv1_1 and 2_0 run as two launches instead of the fused one.  Same bits */
#define MVS_HOOK_S2_PLANES            3  /* >= 1: output planes per workgroup of the stride-2 plane-march kernel; 0 = the launcher's choice.  Same bits */
#define MVS_HOOK_GRU_ONE_STREAM       4  /* 1: the wavefront formulations of the recurrent sweep stay on the caller's stream.  Same bits */
#define MVS_HOOK_GRU_PRODUCER_THREADS 5  /* threads per workgroup of the wavefront's producer launches: 64, 128 (default), 192 or 256.  Same bits */
#define MVS_HOOK_UNET_PERSISTENT       6  /* 1 (default): tower layers with a persistent instance (csrc/unet2d_p.hip) take it; 0: the one-tile-per-workgroup kernels.  Sums differ in the last float64 bits */
#define MVS_HOOK_UNET_GRID            7  /* >= 1: persistent workgroups per launch (per cout group; capped at the tile count) -- tests reach multi-tile ranges at small sizes, measurements vary the residency; 0 (default) = the launcher's choice */
#define MVS_HOOK_FUSE2_PLANES          8  /* even, >= 2: planes per workgroup of the fused 3dconv1_1 + 2_0 launch (measurement); 0 (default) = the launcher's choice.  BatchNorm sums arrive in another order: last bits */
#define MVS_HOOK_REGNET_SIDE_BRANCH    9  /* 1: RegNetUS0's 3dconv1_1 on a side stream of the caller's stream set (mvs_gru_prepare) beside 3dconv2_0 and the low-resolution chain (measurement; needs a set, no capture); 0 (default): fused with 3dconv2_0 in line */
#define MVS_HOOK_OUT_PLANES           10  /* >= 1: planes per workgroup of 3dconv6_2 (tests reach several chunks and both march directions at small sizes; measurement); 0 (default) = the launcher's choice.  Chunks march in alternating directions: last bits */
#define MVS_HOOK_BN_SLOTS             11  /* 1..8: partial rows of RegNetUS0's BatchNorm sums (every layer but the fused pair); 0 (default) = the built-in count.  The sums arrive in another order: last bits */
#define MVS_HOOK_PAIR_SLOTS           12  /* 1..8: partial rows of the fused 3dconv0_1 + 1_0 pass's sums; 0 (default) = the built-in count.  Last bits, as above */
#define MVS_HOOK_CONV_FULL_SWEEPS     13  /* a + 4 * b, a for the 32 -> 8 kernels (conv3d_c8.hip), b for conv3d_s1_kernel (conv3d_mfma.hip), each 0..2.  1: every staged plane of a workgroup's range is swept in full, the halo planes d0 - 1 and d1 included; 2: but for halo planes outside the volume (A/B measurements, bit-equality tests); 0 (default): halo planes issue only the tiles whose result is kept, planes outside the volume none.  Same bits (an exact zero may change sign) */
#define MVS_HOOK_PAIR_PLANES          14  /* even, >= 2: planes per workgroup of the fused 3dconv0_1 + 1_0 launch, in whole chunks (no SPAN); 0 (default) = the launcher's choice.  BatchNorm sums arrive in another order: last bits */
#define MVS_HOOK_S1_PLANES            15  /* >= 1: planes per workgroup of the stride-1 plane-march kernels (conv3d_s1_kernel and the unfused 32 -> 8 kernel); 0 (default) = the launcher's choice.  Last bits, as above */
#define MVS_HOOK_SPAN_FORCE           16  /* G << 8 | M (G = 1..8 tiles per group, M = G..16 ranges): the fused 3dconv0_1 + 1_0 launch takes the SPAN schedule with that pair at any size, if the launcher's other rules allow it (whole chunks if not); 0 (default) = the launcher's choice.  Last bits, as above */
#define MVS_HOOK_PAIR_DIRECT          17  /* 1: the fused 3dconv0_1 + 1_0 launch takes the direct kernel (conv3d_c8.hip) for 3dconv0_1; 0 (default): Winograd F(2,3) along w (conv3d_c8_wino.hip).  3dconv0_1 differs in the last bits (another formula), 3dconv1_0 is the same bits */
#define MVS_HOOK_PAIR_WAVES4          18  /* 1: the Winograd pair kernel runs as four waves per workgroup, each carrying both layers; 0 (default): eight waves, two per SIMD -- waves 0-3 carry 3dconv0_1, waves 4-7 carry 3dconv1_0 and the plane staging.  Same bits */
#define MVS_HOOK_COUNT                19
int mvs_set_test_hook(int id, int value);
int mvs_get_test_hook(int id);

/* ---------------------------------------------------------------------------------------------
 * R1/R1' + R2 prep: plane-induced homographies and their tf.contrib.image.transform 8-vectors.
 * Replaces get_homographies (mvsnet/homography_warping.py:10-58), get_homographies_inv_depth
 * (:60-106) and the coefficient algebra of tf_transform_homography (:216-250).
 *   cams          (view_num,2,4,4)  reference layout, view 0 = reference view
 *   inverse_depth 0: depth_d = depth_start + d*depth_interval          (depth_end ignored)
 *                 1: depth_d = 1/linspace(1/depth_start, 1/depth_end, D) (depth_interval ignored)
 *   homographies  (view_num-1, depth_num, 3, 3)   may be NULL
 *   transforms    (view_num-1, depth_num, 8)      a0 a1 a2 b0 b1 b2 c0 c1, normalised by c2'
 */
int mvs_homography_transforms_f32(const float* cams, int view_num, int depth_num,
                                  float depth_start, float depth_interval, float depth_end,
                                  int inverse_depth, float* homographies, float* transforms,
                                  void* stream);

/* ---------------------------------------------------------------------------------------------
 * R2 + R3: fused projective bilinear warp (zero fill per tap) + cross-view variance.
 * Replaces tf_transform_homography (mvsnet/homography_warping.py:251-252) and the cost loop of
 * inference_mem (mvsnet/model.py:422-463) / inference (:315-334) / the GRU body (:680-693).
 *   ref        (H,W,C)            reference-view feature map
 *   src        (view_num-1,H,W,C) source-view feature maps
 *   transforms (view_num-1,depth_total,8)
 *   d_begin,d_count   planes [d_begin, d_begin+d_count) are produced (d_count = depth_total for the
 *                     3D-CNN path, 1 per step for the recurrent path)
 *   variant    0: cost = Q/N - S*S/(N*N)   (inference_mem, model.py:458-461)
 *              1: cost = Q/N - (S/N)^2     (inference / GRU, model.py:330-332)
 *   negate     1: writes -cost (the GRU consumes -cost, model.py:698)
 *   border     0: zero fill per tap (reference behaviour)   1: clamp taps to the border
 *              (the reference's dead homography_warping path, homography_warping.py:146-149)
 *   cost       (d_count,H,W,C)
 * C must be a multiple of 4.
 * A sample point that leaves the image, however far (beyond int32 included), contributes 0 for that view and leaves the
 * other views alone.  Where proj = t6 x + t7 y + 1 is exactly 0 at a pixel, both device routes -- the depth sweep and the
 * per-plane kernel, chosen by view count, channel count and image size -- and mvs_warp_f32 behave alike:
 *   numerator != 0   the coordinate is +-inf: outside the image, the view contributes 0 and the voxel stays finite
 *                    (tf.contrib.image.transform blends the zero taps with inf - inf weights and gives NaN here; the
 *                    depth sweep's out-of-range weights are literal zeros, and making them carry the NaN cost 1 % of a
 *                    depth map at the metric workload, so the sweep's behaviour is the contract and the per-plane kernel
 *                    and the oracle follow it)
 *   numerator == 0   the coordinate is 0 / 0 = NaN and the voxel is NaN on both routes
 * (tests/test_gpu_forward_cameras.py, the exact_zero transforms of tests/forward_warp_reference.py).
 */
int mvs_cost_volume_f32(const float* ref, const float* src, const float* transforms,
                        int view_num, int depth_total, int d_begin, int d_count,
                        int H, int W, int C, int variant, int negate, int border,
                        float* cost, void* stream);

/* Stand-alone warp of one feature map by one transform (tf_transform_homography,
 * mvsnet/homography_warping.py:211-253); used by the parity tests.  image/out (H,W,C). */
int mvs_warp_f32(const float* image, const float* transform8, int H, int W, int C, int border,
                 float* out, void* stream);

/* ---------------------------------------------------------------------------------------------
 * R4: 3x3x3 convolution / transposed convolution with TensorFlow SAME padding, no bias, and the
 * batch-statistics BatchNorm of the PRODUCER fused into the consumer's load:
 *      in(v,c) = act(x(v,c)*x_scale[c] + x_shift[c]) [ + act(x2(v,c)*x2_scale[c] + x2_shift[c]) ]
 * with act = ReLU when a scale pointer is given, identity (scale=1, shift=0) when it is NULL.
 * Replaces Network.conv / conv_bn / deconv / deconv_bn / batch_normalization / add
 * (mvsnet/cnn_wrapper/network.py:171-215,278-348,457-459,492-509).
 *   x, x2     (D,H,W,Cin)        x2 may be NULL (no skip connection)
 *   w         conv:   (3,3,3,Cin,Cout)  TensorFlow conv3d kernel layout
 *             deconv: (3,3,3,Cout,Cin)  TensorFlow conv3d_transpose kernel layout
 *   stride    conv: 1 or 2 (out = ceil(n/stride)); deconv: 2 (out = 2n)
 *   y         raw (pre-BN) output, (Do,Ho,Wo,Cout)
 *   stats     NULL, or (2,Cout) float64 accumulators [sum, sum of squares] over all output voxels;
 *             must be zeroed by the caller before the launch (mvs_zero_f64)
 */
int mvs_conv3d_f32(const float* x, const float* x_scale, const float* x_shift,
                   const float* x2, const float* x2_scale, const float* x2_shift,
                   const float* w, int D, int H, int W, int Cin, int Cout, int stride,
                   float* y, double* stats, void* stream);
int mvs_deconv3d_f32(const float* x, const float* x_scale, const float* x_shift,
                     const float* x2, const float* x2_scale, const float* x2_shift,
                     const float* w, int D, int H, int W, int Cin, int Cout,
                     float* y, double* stats, void* stream);

/* The two consumers of the cost volume in ONE pass over it: y1 = conv3d(x, w1, stride 1) and
 * y2 = conv3d(x, w2, stride 2), i.e. 3dconv0_1 and 3dconv1_0 of RegNetUS0
 * (mvsnet/cnn_wrapper/mvsnetworks.py:130-134), each with the semantics of mvs_conv3d_f32 (raw input,
 * no producer BatchNorm).  Only the shape of that layer pair is implemented: Cin = 32, Cout1 = 8,
 * Cout2 = 16, even D, H, W; anything else returns MVS_E_SHAPE (call mvs_conv3d_f32 twice instead).
 *   x (D,H,W,32)   w1 (3,3,3,32,8)   w2 (3,3,3,32,16)   y1 (D,H,W,8)   y2 (D/2,H/2,W/2,16)
 *   stats1 / stats2: NULL or zeroed (2,8) / (2,16) float64 accumulators as in mvs_conv3d_f32 */
int mvs_conv3d_pair_f32(const float* x, const float* w1, const float* w2, int D, int H, int W,
                        int Cin, int Cout1, int Cout2, float* y1, double* stats1,
                        float* y2, double* stats2, void* stream);

/* BatchNorm (training-mode statistics, biased variance; network.py:496-506) folded to an affine:
 *   mean = sum/count; var = sumsq/count - mean^2; scale = gamma/sqrt(var+eps); shift = beta-mean*scale
 * stats (2,C) float64 as produced above; scale/shift (C). */
int mvs_bn_finalize_f32(const double* stats, int C, double count, const float* gamma,
                        const float* beta, float eps, float* scale, float* shift, void* stream);
int mvs_zero_f64(double* p, size_t n, void* stream);

/* ---------------------------------------------------------------------------------------------
 * R5: the whole RegNetUS0 3D U-Net (mvsnet/cnn_wrapper/mvsnetworks.py:122-158).
 *   cost      (D,H,W,Cin) with D,H,W divisible by 8
 *   weights   [host] array of 11 device pointers in the order
 *             1_0, 2_0, 3_0, 0_1, 1_1, 2_1, 3_1, 4_0, 5_0, 6_0, 6_2   (TensorFlow layouts)
 *   gammas, betas  [host] arrays of 10 device pointers (same order, no entry for 6_2)
 *   base      base_filter (8 for network_mode 'normal'); Cin of the volume = cin
 *   workspace device scratch of at least mvs_regnet_workspace_bytes() bytes
 *   reg       (D,H,W) filtered cost volume (the squeezed 3dconv6_2 output)
 */
size_t mvs_regnet_workspace_bytes(int D, int H, int W, int cin, int base);
/* Optional one-off weight pre-layout: re-orders the 10 MFMA layers' kernels into the order the
 * kernels keep them in LDS, so that a workgroup uploads its weights with coalesced 16-byte lanes.
 * `prepared` holds mvs_regnet_prepared_floats() floats; pass it to mvs_regnet_us0_prepared_f32
 * together with the original weights (still used by layers outside the MFMA tiling). */
size_t mvs_regnet_prepared_floats(int cin, int base);
int mvs_regnet_prepare_f32(const float* const* weights, int cin, int base, float* prepared,
                           void* stream);
int mvs_regnet_us0_prepared_f32(const float* cost, int D, int H, int W, int cin, int base,
                                const float* const* weights, const float* prepared,
                                const float* const* gammas, const float* const* betas, float eps,
                                void* workspace, size_t workspace_bytes, float* reg, void* stream);

/* ---------------------------------------------------------------------------------------------
 * the 2D convolutions of the UNetDS2GN feature extractor (mvsnet/cnn_wrapper/
 * mvsnetworks.py:53-115; Network.conv_gn / deconv_gn / conv, network.py:171-276,350-409), batched
 * over the V views of a cluster (GroupNorm is per view).  As in the 3D stack a layer stores its RAW
 * output plus float64 group sums, and the consumer applies the producer's GroupNorm (eps 1e-5,
 * 8 channels per group, biased variance) while loading:
 *      in(v,p,c) = act(x(v,p,c) * s(v,c) + t(v,c)),  s, t from stats (V, C/8, S, 2) [sum, sumsq], gamma, beta
 * where S = mvs_gn_stat_slots() partial accumulators per (view, group) that consumers add up (they keep
 * the float64 atomics of ~10^4 workgroups from serialising on one address).
 * (stats == NULL: identity, e.g. the image; relu != 0 for conv_gn producers, 0 for deconv_gn).
 *   mvs_conv2d_gn_f32     k x k (3 or 5) SAME convolution, stride 1 or 2, no bias, of the channel
 *                         concatenation of one or two sources; weights pre-laid-out by
 *                         mvs_conv2d_prepare_f32 (from the TensorFlow (k,k,Cin,Cout) layout, same
 *                         cin1/cin2/cout); channel counts multiples of 4 (image: pad 3 -> 4), Cout of 8
 *   mvs_deconv2d_gn_f32   3x3 stride-2 SAME transposed convolution (out = 2H x 2W): MFMA path when
 *                         `prepared` (mvs_deconv2d_prepare_f32, Cin a multiple of 16) is given, else a
 *                         VALU gather on `w` in the TensorFlow (3,3,Cout,Cin) layout
 *   stats_out             NULL or zeroed (V, Cout/8, S, 2) float64 accumulators of the raw output
 */
int mvs_gn_stat_slots(void);
size_t mvs_conv2d_prepared_floats(int ks, int cin1, int cin2, int cout);
int mvs_conv2d_prepare_f32(const float* w, int ks, int cin1, int cin2, int cout, float* prepared, void* stream);
/* Prepared weights of the stride-1 convolution that computes a layer's INPUT gradient, from the layer's forward kernel
 * w (k,k,cin_fwd,cout_fwd): consumer and buffer size as mvs_conv2d_prepare_f32(ks, cout_fwd, 0, cin_fwd). */
int mvs_conv2d_prepare_dgrad_f32(const float* w, int ks, int cin_fwd, int cout_fwd, float* prepared, void* stream);
int mvs_conv2d_gn_f32(const float* x1, const double* stats1, const float* gamma1, const float* beta1, int c1, int relu1,
                      const float* x2, const double* stats2, const float* gamma2, const float* beta2, int c2, int relu2,
                      const float* prepared, int V, int H, int W, int cout, int ks, int stride,
                      float* y, double* stats_out, void* stream);
/* n weight preparations in one launch (the training towers: every layer's forward and input-gradient kernel once per step).
 * Job i: kind 0 = mvs_conv2d_prepare_f32(w, ks, c1, c2, cout) with cin_src channels actually in `w` (the image layer: c1 = 4,
 * cin_src = 3, the fourth laid out as zeros; otherwise c1 + c2); kind 1 = mvs_conv2d_prepare_dgrad_f32(w, ks, cin_fwd = c1,
 * cout_fwd = cout); kind 2 = mvs_deconv2d_prepare_f32(w, cin = c1, cout); into prepared[i], sized as for the single calls.
 * All array arguments are host arrays of n entries. */
int mvs_unet_prepare_many_f32(int n, const int* kind, const float* const* w, const int* ks, const int* c1, const int* c2,
                              const int* cin_src, const int* cout, float* const* prepared, void* stream);
size_t mvs_deconv2d_prepared_floats(int cin, int cout);
int mvs_deconv2d_prepare_f32(const float* w, int cin, int cout, float* prepared, void* stream);
int mvs_deconv2d_gn_f32(const float* x, const double* stats, const float* gamma, const float* beta, int cin, int relu,
                        const float* w, const float* prepared, int V, int H, int W, int cout, float* y,
                        double* stats_out, void* stream);

/* The towers' input side: per-image, per-channel standardisation of decoded uint8 images on the device, replacing the host
 * call mvs_data_generation/utils.py:33-38 center_image (applied per image by cluster_generator before the graph sees it):
 *   images     (V, H, W, 3) uint8, 4-byte aligned, H*W a multiple of 4
 *   out4       (V, H, W, 4) float32, 16-byte aligned: (x - mean_c) / (sqrt(var_c) + 1e-8) per image and channel, channel 3 = 0
 *              (the layout mvs_conv2d_gn_f32 reads the image in: 3 channels padded to 4)
 *   workspace  mvs_center_images_workspace_bytes(V) bytes (zeroed by the call): exact uint64 sums and sums of squares
 * mean and biased variance come from exact integer totals in float64; the output expression is evaluated in float32 as the
 * reference's.  MVS_E_SHAPE for sizes / alignments outside the above. */
size_t mvs_center_images_workspace_bytes(int V);
int mvs_center_images_u8_f32(const uint8_t* images, int V, int H, int W, float* out4, void* workspace, void* stream);

/* Live timing of the dominant kernel for bench.py's `roofline` object: while enabled, every
 * mvs_regnet_us0_*_f32 call brackets its first launch (the fused 3dconv0_1 + 3dconv1_0 pass over the
 * cost volume, conv3d_c8_kernel) with HIP events on the caller's stream (up to 64 calls).
 * mvs_profile_dominant_ms waits for those events, returns their average duration in milliseconds and
 * the number of samples, and clears them.  Do not enable during hipGraph capture. */
int mvs_profile_dominant(int enable);
int mvs_profile_dominant_ms(double* avg_ms, int* count);
/* Per-layer timing inside a depth map (bench.py's `roofline_kernels` rows of the low-resolution layers): while
 * enabled, every mvs_regnet_us0_*_f32 call brackets EACH of its layer launches with HIP events on the stream that
 * launch goes to (the branch layers' side stream included), up to 32 calls.  mvs_profile_layers_ms waits for the
 * events and returns, for the 11 layers in weight order (3dconv1_0 2_0 3_0 0_1 1_1 2_1 3_1 4_0 5_0 6_0 6_2), the
 * average duration in milliseconds (the fused 3dconv0_1 + 3dconv1_0 pass reports its time under 3dconv0_1 and 0 under
 * 3dconv1_0) and the number of calls sampled.  Every event costs a few microseconds of device idle time: use it
 * outside timed regions; not during hipGraph capture. */
/* The same for the three stages of mvs_depth_from_features_f32 -- [0] homographies + warp + variance, [1] the RegNetUS0 stack
 * (its 11 launches), [2] softmax / soft-argmin / probability -- so that bench.py's stage rows describe the timed path itself (one
 * library call per depth map) and sum to its duration, plus the ~1-2 us of device idle time each event record costs. */
int mvs_profile_stages(int enable);
int mvs_profile_stages_ms(double* avg_ms3, int* count);
int mvs_profile_layers(int enable);
int mvs_profile_layers_ms(double* avg_ms11, int* count);
/* Launch plan of the 1/8-resolution chain.  With prepared weights and the metric's channel widths 3dconv2_1 (read only by
 * the decoder's 3dconv5_0, mvsnetworks.py:139,148-150) has no launch of its own: its blocks ride as filler workgroups behind
 * the blocks of 3dconv3_0, 3dconv3_1 and 3dconv4_0 (240 workgroups each, half of their time fixed cost with the matrix pipe
 * idle).  [host] permille3 receives the share of 3dconv2_1's blocks in each of those three launches, in 1/1000
 * (compile-time constants); mvs_profile_layers_ms then reports 0 under 3dconv2_1.  Without prepared weights, or for other
 * channel widths / volumes of 2 GB and more, the four layers are launched apart whatever this call says. */
int mvs_regnet_filler_shares(int* permille3);
/* The whole 3D-CNN path after the feature towers in ONE call (inference_mem, model.py:408-502): plane homographies ->
 * fused warp + variance cost volume -> RegNetUS0 -> softmax / soft-argmin / probability map; 14 launches, none of them for
 * bookkeeping (the BatchNorm sums are cleared by the homography launch).
 *   features (view_num,H,W,C): the reference view first; cams (view_num,2,4,4); depth samples as in
 *   mvs_homography_transforms_f32; variant as in mvs_cost_volume_f32;
 *   caller-owned scratch: transforms (view_num-1,D,8), cost (D,H,W,C), workspace (mvs_regnet_workspace_bytes), reg (D,H,W);
 *   outputs depth, prob (H,W).  prepared: mvs_regnet_prepare_f32's buffer or NULL. */
int mvs_depth_from_features_f32(const float* features, const float* cams, int view_num, int depth_num,
                                int H, int W, int C, int base, float depth_start, float depth_interval,
                                float depth_end, int inverse_depth, int variant,
                                const float* const* weights, const float* prepared,
                                const float* const* gammas, const float* const* betas, float eps,
                                float* transforms, float* cost, void* workspace, size_t workspace_bytes,
                                float* reg, float* depth, float* prob, void* stream);
/* RegNetUS0 on a batch (FLAGS.batch_size > 1, model.py:466-469): the reference's BatchNorm layers normalise with
 * the statistics of the whole batch (B,D,H,W) (network.py:496-506), so samples are coupled through every layer's sums.
 *   cost (B,D,H,W,cin) contiguous; reg (B,D,H,W); workspace >= B * mvs_regnet_workspace_bytes(D,H,W,cin,base);
 *   prepared: the buffer of mvs_regnet_prepare_f32 or NULL. */
int mvs_regnet_us0_batch_f32(const float* cost, int batch, int D, int H, int W, int cin, int base,
                             const float* const* weights, const float* prepared,
                             const float* const* gammas, const float* const* betas, float eps,
                             void* workspace, size_t workspace_bytes, float* reg, void* stream);
int mvs_regnet_us0_f32(const float* cost, int D, int H, int W, int cin, int base,
                       const float* const* weights, const float* const* gammas,
                       const float* const* betas, float eps, void* workspace,
                       size_t workspace_bytes, float* reg, void* stream);

/* ---------------------------------------------------------------------------------------------
 * R6 + R7: softmax(-reg) over depth, soft-argmin depth, 4-bucket probability map.
 * Replaces mvsnet/model.py:471-498 and get_probability_map_slice (:45-144).
 *   reg (D,H,W); depth, prob (H,W); depth samples as in mvs_homography_transforms_f32 with
 *   depth_end = depth_start + (D-1)*depth_interval.
 */
int mvs_softargmin_prob_f32(const float* reg, int D, int H, int W, float depth_start,
                            float depth_interval, int inverse_depth, float* depth, float* prob,
                            void* stream);

/* ---------------------------------------------------------------------------------------------
 * R8: 3x3 SAME 2D convolution over the channel concatenation [xa | xb] with bias, used by the
 * ConvGRU cell (mvsnet/convgru.py:89-93,107-111) and prob_conv (mvsnet/model.py:701-702).
 *   xa (H,W,Ca), xb (H,W,Cb) (xb may be NULL with Cb = 0); w (3,3,Ca+Cb,Cout); bias (Cout)
 *   y  (H,W,Cout)
 *   stats  NULL or (groups,2) float64 [sum,sumsq] over (H,W, Cout/groups channels) per group,
 *          zeroed by the caller: the LayerNorm moments of convgru.py:30-31 (groups = 2 for the
 *          gate convolution: reset | update; 1 for the output convolution).
 */
int mvs_conv2d_cat_f32(const float* xa, int Ca, const float* xb, int Cb, const float* w,
                       const float* bias, int H, int W, int Cout, float* y, double* stats,
                       int groups, void* stream);

/* ConvGRU element-wise stages (mvsnet/convgru.py:97-102,114-120); LayerNorm = tf.contrib.layers
 * layer_norm: moments over (H,W,F), eps 1e-12, per-channel gamma/beta.
 *   gates: g (H,W,2F) raw gate conv; stats (2,2) f64 -> r*h (H,W,F) and u (H,W,F)
 *   blend: c (H,W,F) raw output conv; stats (1,2) f64; h updated in place:
 *          h = u*h + (1-u)*tanh(LN(c))
 */
int mvs_gru_gates_f32(const float* g, const double* stats, const float* reset_gamma,
                      const float* reset_beta, const float* update_gamma, const float* update_beta,
                      const float* h, int H, int W, int F, float* rh, float* u, void* stream);
int mvs_gru_blend_f32(const float* c, const double* stats, const float* out_gamma,
                      const float* out_beta, const float* u, int H, int W, int F, float* h,
                      void* stream);

/* R9: winner-take-all update (mvsnet/model.py:703-731): prob = exp(reg); strict '<' keeps the first
 * maximum.  All maps (H,W).  mvs_wta_finish: prob_out = max_prob / (exp_sum + 1e-7) (:749-751). */
int mvs_wta_update_f32(const float* reg, float depth_value, int H, int W, float* max_prob,
                       float* depth_image, float* exp_sum, void* stream);
int mvs_wta_finish_f32(const float* max_prob, const float* exp_sum, int H, int W, float* prob_out,
                       void* stream);

/* R9 composed: the whole recurrent sweep of inference_winner_take_all (mvsnet/model.py:601-751)
 * after the feature towers.
 *   params [host] array of 32 device pointers: for cell i in 1..3:
 *            gates_w, gates_b, reset_gamma, reset_beta, update_gamma, update_beta,
 *            out_w, out_b, out_gamma, out_beta   (10 each), then prob_w, prob_b
 *   depth_values [host] depth_num floats (depth of plane d, model.py:706-715)
 *   filters (f1,f2,f3): ConvGRU filter counts (16,4,2 for 'normal')
 * The sweep is a wavefront over (plane, cell) on library-owned side streams forked from / joined to `stream`: the set
 * mvs_gru_prepare(stream) created for this caller stream.  The sweep itself creates nothing and never synchronises:
 *   - default formulation at the reference's shape (mvs_gru_set_formulation 0 / 3): the fused sweep, two launches per plane on
 *     `stream` alone, with or without a set, eagerly or under hipGraph capture -- the same bits every time;
 *   - wavefront formulations (1 / 2) on a prepared stream: four streams; on a stream without a set: the same sweep on `stream`
 *     alone (same winning planes, ~1.7x the time at 400 x 300), one note on stderr per process;
 *   - wavefront formulations under hipGraph capture: always the one-stream form -- hip::Stream::EndCapture of the HIP runtime the
 *     PyTorch wheel bundles (7.0.70002) recurses without bound when captured streams wait on each other in both directions (root
 *     cause, native backtrace and a stand-alone reproducer: profiles/r05_capture_wavefront_root_cause.txt,
 *     tools/capture_wavefront_repro.hip; ROCm 7.2's own runtime does not have the defect);
 *   - every exit after the fork, error returns included, first makes `stream` wait for the side streams.
 * The workspace holds a batch of 16 cost slices, two batches of the hoisted x-part of cell 1 and 16-plane state rings:
 * ~1.0 GB at 400 x 300, C = 32 (mvs_gru_workspace_bytes).
 */
size_t mvs_gru_workspace_bytes(int H, int W, int C, int f1, int f2, int f3);
int mvs_gru_wta_f32(const float* ref, const float* src, const float* transforms, int view_num,
                    int depth_num, int H, int W, int C, int f1, int f2, int f3,
                    const float* const* params, const float* depth_values, void* workspace,
                    size_t workspace_bytes, float* depth_out, float* prob_out, void* stream);

/* The same sweep for `views` (1..8) INDEPENDENT reference views of one size in the same launches -- how config 3 shards
 * (mvsnet/inference.py:105-119 loops over ~135 reference views per GPU): every kernel of the wavefront takes a view index
 * from its grid, so the ~7 launches per plane, their latency floors and the cross-stream waits are shared by `views` depth
 * maps.  Per-view results equal the single-view call's (same tiles, same arithmetic; the LayerNorm sums are float per tile
 * and double across tiles, so they do not depend on how tiles are dealt to workgroups).
 *   ref / src / transforms [host] arrays of `views` device pointers (as in mvs_gru_wta_f32, one entry per view)
 *   depth_values [host] views x depth_num floats
 *   workspace    views x mvs_gru_workspace_bytes(...) bytes (one block per view)
 *   depth_out / prob_out (views, H, W)
 * Shape limits (both entry points): f1, f2, f3 <= 64, MVS_E_SHAPE otherwise (the blend kernels keep 2 x F LayerNorm affines per
 * cell in LDS and the staging code is written for at most 64 state channels; the reference uses 16 / 4 / 2, the 'fat' variant
 * 32 / 8 / 4); views in 1..8 (MVS_E_BADARG); C as mvs_cost_volume_f32 accepts it.  The fused two-launch sweep covers C = 32 with 16 / 4 / 2 while a view's
 * workspace block (mvs_gru_workspace_bytes, ~10.2 KB per pixel) stays below 2 GiB -- its kernels address the block with 32-bit
 * byte offsets -- i.e. feature maps up to ~210 k pixels; larger maps (e.g. 576 x 384) and every other accepted shape run the
 * wavefront kernels.  mvs_gru_fused_route is that predicate (1 = fused), decided before anything is enqueued.
 */
int mvs_gru_fused_route(int C, int f1, int f2, int f3, size_t view_block_bytes);
int mvs_gru_wta_batch_f32(const float* const* ref, const float* const* src, const float* const* transforms,
                          int views, int view_num, int depth_num, int H, int W, int C, int f1, int f2,
                          int f3, const float* const* params, const float* depth_values, void* workspace,
                          size_t workspace_bytes, float* depth_out, float* prob_out, void* stream);

/* Set-up of the recurrent sweep for caller stream `stream` on the current device: three side streams, ~30 events, and ONE
 * ~10-30 ms calibration that finds the compute pipe the caller's hardware queue lives on (csrc/gru_streams.hip) so that the
 * side streams avoid it.  THE call of this header that creates resources and synchronises (`stream` and the new streams):
 * call it once per caller stream at start-up (DepthPlan(..., "GRU") does), never inside a latency-critical region or under
 * hipGraph capture (returns MVS_E_NOT_PREPARED there).  Idempotent.  An inconclusive calibration is reported once on stderr and
 * the set is still usable.  At most 16 sets per process (MVS_E_NO_SLOT beyond; mvs_gru_release frees one).  Thread-safe.
 * Optional since round 5: without a set the sweep runs as the fused two-launches-per-plane pipeline on the caller's stream alone
 * (csrc/gru_fused.hip), which needs none; the round-4 four-stream wavefront (mvs_gru_set_formulation 1 / 2) still does. */
int mvs_gru_prepare(void* stream);
/* Tear-down: waits for the set's side streams, destroys them and their events (MVS_E_BADARG: no set for this stream).  Call it
 * before destroying `stream` -- a later stream may receive the same handle on another hardware queue. */
int mvs_gru_release(void* stream);

/* Formulation of the recurrent sweep at the reference's shape (32 feature channels, filters 16 / 4 / 2):
 *   0 (default) = 3 = the FUSED sweep (csrc/gru_fused.hip): two launches per plane on the caller's stream alone carry all three
 *       cells, prob_conv and the winner-take-all update; no stream set needed, captures into a hipGraph;
 *   1 = the round-4 wavefront over a stream set (mvs_gru_prepare) with cell 1's x-part hoisted into batched producer launches,
 *   2 = the same wavefront with full 48-channel per-plane kernels.
 * 1 and 2 give the same bits as each other; the fused sweep runs the same multiply-add chains for cell 1 and differs from them
 * in the last bits (LayerNorm partial sums, the small cells' four partial chains).  Within a formulation a batch of views gives
 * the single view's bits.  Other shapes take the wavefront / generic routes whatever is set.  A tuning / test switch: process-wide
 * atomic, read once at the start of each sweep -- a sweep keeps the formulation it started with. */
int mvs_gru_set_formulation(int form);

/* Diagnostic (csrc/gru_fused.hip): per-workgroup time stamps of the fused two-launches-per-plane sweep.  `buffer` = caller-owned
 * device memory of (1 + 8 * capacity) int64, zeroed by the caller; every workgroup of every fused launch appends one record
 * [launch << 32 | phase << 16 | workgroup, entry, first tile staged, first tile done, loop done, exit (100 MHz ticks), tiles,
 * HW_ID].  null switches it off (the default).  Not thread-safe; tools/gru_fused_trace.py. */
int mvs_gru_fused_trace(void* buffer, int capacity);

/* Diagnostic: the side-stream layout of the set mvs_gru_prepare made for `stream` (MVS_E_NOT_PREPARED without one):
 * *pipe_of_caller = which of the four candidate pipes the caller's hardware queue was measured on (-1: none stood out),
 * probe_us[8] = the calibration chain times of the eight candidate streams (4 high-, 4 low-priority). */
int mvs_gru_stream_layout(void* stream, int* pipe_of_caller, float* probe_us);

/* ---------------------------------------------------------------------------------------------
 * backward passes of the plane-sweep path for training (csrc/backward.hip, conv3d_wgrad.hip; the
 * optimiser steps: csrc/optimizer.hip).  The reference has no such
 * functions: TensorFlow differentiates the graph of `inference` (mvsnet/model.py:257-372) inside
 * opt.compute_gradients (mvsnet/train.py:428-429).  Input gradients of the 3D convolutions need no
 * entry point of their own: a stride-2 convolution's input gradient is mvs_deconv3d_f32 with the SAME
 * kernel array, a transposed convolution's is mvs_conv3d_f32 (stride 2) with the same array, and a
 * stride-1 convolution's is mvs_conv3d_f32 with the kernel flipped along kd,kh,kw and Cin/Cout swapped.
 *
 * mvs_softargmin_bwd_f32   g_reg(d) = -g_depth * P_d * (z_d - depth) - g_prob * P_d * (m_d - prob), P = softmax(-reg),
 *                          m_d = number of the four probability buckets equal to plane d (model.py:343-366, 45-144;
 *                          the bucket indices carry no gradient); g_depth or g_prob may be NULL
 * mvs_bn_relu_f32          out = act(y*scale+shift) [+ act(y2*scale2+shift2)], act = ReLU when the scale
 *                          is given: the normalised layer input the forward kernels form on load
 * mvs_bn_bwd_reduce_f32    BatchNorm(batch statistics)+ReLU backward, pass 1: sums (S,2,C) float64 (zeroed
 *                          by the caller; S = mvs_bn_bwd_sum_slots() partial rows that pass 2 folds, so that
 *                          the float64 atomics of ~1000 workgroups do not serialise) += [sum gz, sum gz*xhat], gz = (g1 [+ g2]) * [y*scale+shift > 0],
 *                          xhat from `stats` (the forward's (2,C) sums) / count / eps (network.py:492-509)
 * mvs_bn_bwd_apply_f32     pass 2: g_y = gamma/std * (gz - mean(gz) - xhat*mean(gz*xhat));
 *                          g_gamma = sum gz*xhat, g_beta = sum gz (either may be NULL)
 * mvs_conv3d_wgrad_f32     dW(tap,cb,cs) = sum_o big(stride*o + tap - pad, cb) * small(o, cs); big (D,H,W,Cbig),
 *                          small (D/s,H/s,W/s,Csmall); convolution: big = layer input, small = output
 *                          gradient -> dW in the conv3d layout; transposed convolution (stride 2): big =
 *                          output gradient, small = layer input -> dW in the conv3d_transpose layout.
 *                          Deterministic (per-workgroup partials in `workspace`, fixed-order float64 sum).
 *                          Built for the channel pairs of RegNetUS0 'normal' (else MVS_E_SHAPE).
 * mvs_cost_volume_bwd_f32  gradient of mvs_cost_volume_f32 (either variant) w.r.t. the feature maps:
 *                          g_ref (H,W,C) and g_src (view_num-1,H,W,C), zeroed by the caller, are
 *                          accumulated with float atomics; g2 may be NULL (second consumer of the volume)
 * mvs_rmsprop_step_f32     tf.train.RMSPropOptimizer update over a flat parameter buffer (train.py:259):
 *                          ms += (g^2-ms)(1-decay); mom = momentum*mom + lr*g/sqrt(ms+eps); w -= mom,
 *                          g = grad * grad_scale (1/world_size after a sum all-reduce)
 */
int mvs_softargmin_bwd_f32(const float* reg, const float* g_depth, const float* g_prob, int D, int H, int W,
                           float depth_start, float depth_interval, int inverse_depth,
                           float* g_reg, void* stream);
int mvs_bn_relu_f32(const float* y, const float* scale, const float* shift, const float* y2,
                    const float* scale2, const float* shift2, size_t voxels, int C, float* out,
                    void* stream);
int mvs_bn_bwd_sum_slots(void);
int mvs_bn_bwd_reduce_f32(const float* y, const double* stats, double count, float eps,
                          const float* scale, const float* shift, const float* g1,
                          const float* g2, size_t voxels, int C, double* sums, void* stream);
int mvs_bn_bwd_apply_f32(const float* y, const double* stats, double count, float eps,
                         const float* scale, const float* shift, const float* gamma,
                         const float* g1, const float* g2, const double* sums, size_t voxels,
                         int C, float* g_y, float* g_gamma, float* g_beta, void* stream);
size_t mvs_conv3d_wgrad_workspace_bytes(int D, int H, int W, int Cbig, int Csmall, int stride);
int mvs_conv3d_wgrad_f32(const float* big, const float* small, int D, int H, int W, int Cbig,
                         int Csmall, int stride, void* workspace, size_t workspace_bytes,
                         float* dw, void* stream);
int mvs_cost_volume_bwd_f32(const float* ref, const float* src, const float* transforms,
                            int view_num, int depth_num, int H, int W, int C, const float* g1,
                            const float* g2, float* g_ref, float* g_src, void* stream);
/* Atomic-free, bit-reproducible variant of mvs_cost_volume_bwd_f32 (C = 32 or 16): stores the per-view
 * warped-sample gradients in `workspace` (mvs_cost_volume_bwd_workspace_bytes: (N-1)*D*H*W*C floats plus
 * chunk rows) and gathers them in the source frame through the inverse plane homographies.  g_ref / g_src
 * are overwritten (no zeroing needed).  Planes that minify a source view more than ~8x fall outside its
 * candidate search; use the scatter version for such geometry. */
size_t mvs_cost_volume_bwd_workspace_bytes(int view_num, int depth_num, int H, int W, int C);
int mvs_cost_volume_bwd_gather_f32(const float* ref, const float* src, const float* transforms,
                                   int view_num, int depth_num, int H, int W, int C, const float* g1,
                                   const float* g2, void* workspace, size_t workspace_bytes,
                                   float* g_ref, float* g_src, void* stream);
int mvs_rmsprop_step_f32(float* w, const float* g, float* ms, float* mom, size_t n, float lr,
                         float decay, float momentum, float eps, float grad_scale, void* stream);
/* GroupNorm (+ReLU) of the 2D towers for TRAINING (csrc/groupnorm.hip; Network.conv_gn / deconv_gn, network.py:217-276, 350-409:
 * groups of 8 channels, biased variance; inference fuses GroupNorm into mvs_conv2d_gn_f32 instead).
 *   x, y, g, dx   (V, hw, C) channel-last, C a multiple of 8
 *   stats         (V, 2, C) float64 per-channel [sum, sum of squares] of x, zeroed by the caller before
 *                 mvs_gn_stats_f32 (group moments are folded from a group's 8 channel sums where needed)
 *   sums          mvs_gn_bwd_sums_doubles(V, C) float64 = mvs_gn_bwd_sum_slots() copies of (V, 2, C) [sum gz, sum gz*xhat],
 *                 zeroed by the caller before mvs_gn_bwd_reduce_f32: the workgroups spread their float64 atomics over the
 *                 copies (atomics on one address are performed one after the other), mvs_gn_bwd_apply_f32 adds them up;
 *                 g_beta(c) = sum over slots and views of sums(s,v,0,c), g_gamma(c) likewise of sums(s,v,1,c)
 *   relu          1: y = ReLU(gamma*xhat+beta) (conv_gn), 0: no activation (deconv_gn) */
int mvs_gn_stats_f32(const float* x, int V, size_t hw, int C, double* stats, void* stream);
/* The same statistics from the sums the tower convolutions already wrote: slots (V, C/8, nslot, 2) float64 partial [sum, sumsq]
 * per 8-channel group (mvs_conv2d_gn_f32 / mvs_deconv2d_gn_f32, nslot = mvs_gn_stat_slots()) -> stats (V, 2, C), every channel
 * carrying an eighth of its group's totals (the group moments the kernels below fold from 8 channel sums are then the forward's). */
int mvs_gn_slots_to_channel_sums_f64(const double* slots, int V, int C, int nslot, double* stats, void* stream);
/* ... for n layers in one launch: layer i's slots start slot_off[i] float64 behind `slots`, its (V, 2, C[i]) statistics
 * stat_off[i] behind `stats` (host arrays of n entries). */
int mvs_gn_slots_to_channel_sums_many_f64(int n, const double* slots, const long long* slot_off, const int* C, int V, int nslot,
                                          double* stats, const long long* stat_off, void* stream);
int mvs_gn_apply_f32(const float* x, const double* stats, const float* gamma, const float* beta, float eps,
                     int relu, int V, size_t hw, int C, float* y, void* stream);
int mvs_gn_bwd_sum_slots(void);
size_t mvs_gn_bwd_sums_doubles(int V, int C);
int mvs_gn_bwd_reduce_f32(const float* x, const double* stats, const float* gamma, const float* beta, float eps,
                          int relu, const float* g, int V, size_t hw, int C, double* sums, void* stream);
int mvs_gn_bwd_apply_f32(const float* x, const double* stats, const float* gamma, const float* beta, float eps,
                         int relu, const float* g, const double* sums, int V, size_t hw, int C, float* dx,
                         void* stream);
/* ... with g_beta / g_gamma ADDED to totals (2, C) float64 by the launch's first workgroup (the parameter gradients without a
 * reduction launch per layer); C <= 128. */
int mvs_gn_bwd_apply_tot_f32(const float* x, const double* stats, const float* gamma, const float* beta, float eps,
                             int relu, const float* g, const double* sums, double* totals, int V, size_t hw, int C, float* dx,
                             void* stream);
/* The other two optimisers of setup_optimizer (csrc/optimizer.hip; train.py:248-271): tf.train.MomentumOptimizer
 * (accum = momentum*accum + g; w -= lr*accum) and tf.train.AdamOptimizer (lr_t = lr*sqrt(1-beta2^t)/
 * (1-beta1^t) formed by the caller; w -= lr_t*m/(sqrt(v)+eps)). */
int mvs_momentum_step_f32(float* w, const float* g, float* accum, size_t n, float lr, float momentum,
                          float grad_scale, void* stream);
int mvs_adam_step_f32(float* w, const float* g, float* m, float* v, size_t n, float lr_t, float beta1,
                      float beta2, float eps, float grad_scale, void* stream);

/* Many small tensors in one launch (the end of the towers' backward, replacing a permute-copy and an autograd accumulation
 * launch per parameter -- average_gradients' inputs, train.py:155-187, land in the flat gradient buffer directly):
 *   mvs_transpose_add_many_f32   job i: dst_i (KK, keep, B) += src_i (B, A, KK) with the axes reversed, rows a >= keep dropped
 *                                (ATen's (Cout, Cin, k, k) weight gradient into TensorFlow's (k, k, Cin, Cout) variable);
 *                                dims = n x 4 host ints [B, A, KK, keep], src / dst host arrays of n device pointers
 *   mvs_add_f64_many_f32         job i: dst_i[0..counts_i) += (float)src_i[..]  (GroupNorm gamma / beta gradients accumulated
 *                                in float64 by mvs_gn_bwd_apply_tot_f32)
 * Any n (the jobs travel in the kernel arguments, 48 / 96 per launch). */
int mvs_transpose_add_many_f32(int n, const float* const* src, float* const* dst, const int* dims, void* stream);
int mvs_add_f64_many_f32(int n, const double* const* src, float* const* dst, const int* counts, void* stream);
/*   mvs_add_many_f32             job i: dst_i[0..counts_i) += src_i[..] (the regulariser's parameter gradients, already in the
 *                                variables' layouts, into the flat gradient buffer) */
int mvs_add_many_f32(int n, const float* const* src, float* const* dst, const long long* counts, void* stream);

/* Training of the recurrent regulariser (inference_prob_recurrent, mvsnet/model.py:505-599; ConvGRUCell,
 * mvsnet/convgru.py:82-122): the plane-sequential part of back-propagation through time of ONE cell over all D
 * planes (csrc/gru_train.hip).  px (D,H,W,3F) holds the x parts of the cell's two convolutions with their biases,
 * channels [reset | update | candidate]; wgh (3,3,F,2F) / woh (3,3,F,F) are the h parts of the two kernels;
 * ln (6,F) = reset gamma, reset beta, update gamma, update beta, candidate gamma, candidate beta.
 * Forward keeps g (D,H,W,2F), c (D,H,W,F) (raw convolutions), rh (D,H,W,F) = r*h, h (D+1,H,W,F) with h[0] the initial
 * state set by the caller, and the LayerNorm moments stats (D, forward_slots, 6) float64, zeroed by the caller.
 * Backward takes gh (D,H,W,F), the gradient reaching every state from outside the recurrence, the flipped /
 * transposed kernels wgh_t (3,3,2F,F), woh_t (3,3,F,F), and returns gpx (D,H,W,3F), the gradient w.r.t. px (from
 * which the host forms every input, weight and bias gradient with batched convolutions), and
 * part (D,3,backward_slots,2,F) float64 (zeroed by the caller): per plane and LayerNorm the sums over pixels of
 * dz and dz*xhat, i.e. the gradients of beta and gamma once summed over planes and slots.
 * scratch: 6*H*W*F floats.  dh_in (H,W,F): gradient w.r.t. the state LEAVING the last plane that arrives from
 * planes above this call's range (null: none, and then the caller zeroes `scratch`); dh_out (H,W,F), optional:
 * receives the gradient w.r.t. h[0], the state entering plane 0 -- so a sweep can be run in chunks of planes (forward
 * in ascending chunks with h carried through the (D+1)-plane buffer, backward in descending chunks with dh_out of
 * one call as dh_in of the next), which is what lets the three cells run as a wavefront on three streams.
 * F in {16, 8, 4, 2, 1}. */
int mvs_gru_train_slots(int* forward_slots, int* backward_slots);
int mvs_gru_train_cell_fwd_f32(const float* px, const float* wgh, const float* woh, const float* ln, int D, int H,
                               int W, int F, float* g, float* c, float* rh, float* h, double* stats, void* stream);
int mvs_gru_train_cell_bwd_f32(const float* gh, const float* g, const float* c, const float* h, const double* stats,
                               const float* wgh_t, const float* woh_t, const float* ln, int D, int H, int W, int F,
                               float* gpx, double* part, float* scratch, const float* dh_in, float* dh_out,
                               void* stream);

/* Weight gradient of a 3x3 SAME stride-1 2D convolution over a batch of planes (csrc/conv2d_wgrad.hip; in the
 * reference: TensorFlow's Conv2DBackpropFilter of the tf.layers.conv2d calls of mvsnet/convgru.py:92,110 behind
 * opt.compute_gradients, train.py:428-429):  dw (3,3,Cin,Cout) = sum over n,y,x of x[n,y+kh-1,x+kw-1,ci] * g[n,y,x,co].
 * x (N,H,W,Cin); g (N,H,W,g_stride) of which channels [g_off, g_off+Cout) are used (g_stride, g_off multiples of 4).
 * Deterministic (per-workgroup partials in `workspace`, fixed-order float64 sum).  Built for (Cin, Cout) in
 * {16,32} x {16,32,48}; anything else returns MVS_E_SHAPE. */
size_t mvs_conv2d_wgrad_workspace_bytes(int N, int H, int W, int Cin, int Cout);
int mvs_conv2d_wgrad_f32(const float* x, const float* g, int g_stride, int g_off, int N, int H, int W, int Cin,
                         int Cout, void* workspace, size_t workspace_bytes, float* dw, void* stream);

/* Geometric-consistency fusion of V depth maps into one coloured point cloud (csrc/fusion.hip; replaces the external
 * fusibile run of mvsnet/depthfusion.py:194-214 with this project's own algorithm, specified in mvsnet_amd/fusion.py --
 * not bit-compatible with fusibile):
 *   depth, prob   (V,H,W) float32; a pixel is valid when depth > 0, finite and prob >= prob_threshold
 *   tables        V*V*12 + V*12 floats: M[a][b] (3x4, row-major) = P_b o B_a at [(a*V + b)*12], then B_v at [V*V*12 + v*12];
 *                 B_v maps (x d, y d, d, 1) of view v's pixel (x, y) at depth d to the world point, P_b = K_b [R_b | t_b]
 *   src_offsets   V+1 int32, src_index: view r's sources are src_index[src_offsets[r] .. src_offsets[r+1]), ascending,
 *                 r itself excluded (entries out of range or equal to r are skipped); at most max_sources are used per view
 *   num_consistent  a pixel is kept when its count of consistent sources n >= num_consistent (compared as float)
 *   dedupe        1: views in ascending order, witnesses of kept pixels are never reference pixels later; 0: views independent
 *   images        (V,img_h,img_w,3) uint8 or NULL (colours 0); nearest pixel ((x+1/2) img_w / W, (y+1/2) img_h / H)
 *   xyz (V*H*W,3) float32, rgb (V*H*W,3) uint8, view_index (V*H*W) int32, pixel_index (V*H*W) int32 or NULL (row-major
 *                 y*W + x of the point's reference pixel): capacity for every pixel; the first *count entries (count: one
 *                 int32 on the device) are the points, by view ascending then row-major pixel order
 *   workspace     mvs_fusion_workspace_bytes(V, H, W, max_sources, dedupe) bytes (MVS_E_WORKSPACE when smaller)
 * Deterministic: integer counts and fixed-order float32 sums, no float atomics (two runs give the same bytes).
 * MVS_E_SHAPE when V*H*W exceeds 2^31-1 or V or max_sources exceeds 65535. */
size_t mvs_fusion_workspace_bytes(int V, int H, int W, int max_sources, int dedupe);
int mvs_fusion_f32(const float* depth, const float* prob, int V, int H, int W, const float* tables, const int* src_offsets,
                   const int* src_index, int max_sources, float prob_threshold, float reproj_threshold,
                   float depth_rel_threshold, float num_consistent, int dedupe, const uint8_t* images, int img_h, int img_w,
                   float* xyz, uint8_t* rgb, int* view_index, int* pixel_index, int* count, void* workspace,
                   size_t workspace_bytes, void* stream);

/* Surface normals from depth maps, and the fusion that carries them (csrc/fusion.hip; semantics in mvsnet_amd/fusion.py):
 *   mvs_depth_normals_f32   per-view normal maps: depth, prob (V,H,W) and tables as for mvs_fusion_f32 (only the B_v part is
 *                 read); normals (V,H,W,3) float32 in the world frame, unit length and facing the camera, (0,0,0) where a
 *                 pixel has no normal (invalid, or no usable neighbour along x or along y: a neighbour is usable when it is
 *                 valid and |d_q - d| < jump_threshold d).  One launch, nothing allocated, nothing synchronised.
 *   mvs_fusion_normals_f32  mvs_fusion_f32 with normals; the arguments of mvs_fusion_f32 plus
 *     jump_threshold        the depth-jump limit of the normal maps
 *     normal_cos_threshold  <= -1: off -- points, order and colours are those of mvs_fusion_f32, bit for bit; otherwise a
 *                 pixel without a normal is not valid (neither reference pixel nor witness) and a geometrically consistent
 *                 pair is consistent only when n_r . n_s > normal_cos_threshold (must be < 1)
 *     normals     (V*H*W,3) float32, capacity as xyz: per point the normalised sum of its reference pixel's normal and its
 *                 consistent sources' normals (fixed slice order: bitwise reproducible), (0,0,0) when that sum is zero
 *     workspace   mvs_fusion_normals_workspace_bytes(V, H, W, max_sources, dedupe) bytes (it also holds the normal maps, 16
 *                 bytes per pixel)
 * Error codes as mvs_fusion_f32. */
int mvs_depth_normals_f32(const float* depth, const float* prob, int V, int H, int W, const float* tables, float prob_threshold,
                          float jump_threshold, float* normals, void* stream);
size_t mvs_fusion_normals_workspace_bytes(int V, int H, int W, int max_sources, int dedupe);
int mvs_fusion_normals_f32(const float* depth, const float* prob, int V, int H, int W, const float* tables,
                           const int* src_offsets, const int* src_index, int max_sources, float prob_threshold,
                           float reproj_threshold, float depth_rel_threshold, float num_consistent, int dedupe,
                           float jump_threshold, float normal_cos_threshold, const uint8_t* images, int img_h, int img_w,
                           float* xyz, uint8_t* rgb, float* normals, int* view_index, int* pixel_index, int* count,
                           void* workspace, size_t workspace_bytes, void* stream);

/* Point-cloud evaluation (csrc/pointcloud.hip; semantics in mvsnet_amd/evaluate.py).  Points are (n,3) float32, n >= 1.
 *
 * Nearest neighbour of every query point in the target cloud, capped at max_dist:
 *   grid          the target's uniform grid: origin (ox, oy, oz), cubic cells of side `cell`, gx * gy * gz cells
 *                 (MVS_E_SHAPE beyond 2^24); points outside it are clamped into its border cells, any grid gives exact results
 *   dist, index   (n_query) float32 / int32, in query input order: d = min over the target of |q - t| (d^2 in float32 from
 *                 float32 differences) and the target index of the minimiser when d^2 <= max_dist^2, else +inf and -1; exact
 *                 ties of d^2 go to the smallest target index
 *   workspace     mvs_nn_workspace_bytes(n_query, n_target, gx, gy, gz) bytes (0 for invalid sizes)
 * Deterministic: the only atomics are integer ranks inside a cell, and the answer does not depend on them. */
size_t mvs_nn_workspace_bytes(int n_query, int n_target, int gx, int gy, int gz);
int mvs_nn_f32(const float* query, int n_query, const float* target, int n_target, float ox, float oy, float oz, float cell,
               int gx, int gy, int gz, float max_dist, float* dist, int* index, void* workspace, size_t workspace_bytes,
               void* stream);
/* The query step of mvs_nn_f32 alone, over the grid and the sorted copies that the last mvs_nn_f32 call with the same sizes,
 * grid and workspace left there (for another max_dist, or to time the query apart from the grid builds); visited (n_query)
 * int32 or NULL receives the number of candidate target points each query compared (a measurement). */
int mvs_nn_query_f32(int n_query, int n_target, float ox, float oy, float oz, float cell, int gx, int gy, int gz,
                     float max_dist, float* dist, int* index, int* visited, const void* workspace, size_t workspace_bytes,
                     void* stream);
/* The target's grid alone, built once for many queries against a target that does not move (count / scan / scatter of
 * mvs_nn_f32 for the target only):
 *   workspace     mvs_nn_target_workspace_bytes(n_target, gx, gy, gz) bytes (0 for invalid sizes); after the call it holds the
 *                 per-cell starts, the cell-ordered float4 copy (x, y, z, input index) and each point's place in that copy */
size_t mvs_nn_target_workspace_bytes(int n_target, int gx, int gy, int gz);
int mvs_nn_target_build_f32(const float* target, int n_target, float ox, float oy, float oz, float cell, int gx, int gy, int gz,
                            void* workspace, size_t workspace_bytes, void* stream);
/* One step of point-to-point ICP, fused: transform, nearest neighbour and the float64 moments the host solves from
 * (mvsnet_amd/register.py is normative):
 *   source        (n_source,3) float32, read only
 *   order         NULL or (n_source) int32, a permutation of the source: the order in which lanes take the points (points that
 *                 share a target cell side by side run faster); NULL = input order.  It never changes which neighbour a
 *                 point gets, only the order of the float64 sums
 *   T, cp, cq     [host] row-major 3x4 float64 transform (finite) and the two float64 centres, passed to the kernel by value
 *   grid, n_target, target_workspace: exactly what mvs_nn_target_build_f32 was called with and what it left behind
 *   moments       [device] 18 doubles over the source points p whose p' = fl32(T p) (rows left to right in float64, rounded
 *                 once) has a target point q with float32 d^2 <= max_corr_dist^2 (nearest, ties to the smallest index):
 *                 count, sum |r|^2, sum a (3), sum b (3), sum a b^T (9, row-major), sum |a|^2 with a = p - cp, b = q - cq,
 *                 r = T p - q in float64 (T p unrounded)
 *   dist, index   NULL or (n_source) float32 / int32 in input order, as mvs_nn_f32 writes them for the queries p'
 *   workspace     mvs_icp_step_workspace_bytes(n_source) bytes
 * Per-lane sums in a fixed order, fixed trees inside a block, float64 partials per block reduced in block order by one
 * workgroup; no float atomics: the same inputs, order and sizes give the same 18 x 8 bytes on every run. */
size_t mvs_icp_step_workspace_bytes(int n_source);
int mvs_icp_step_f32(const float* source, int n_source, const int* order, const double* T, const double* cp, const double* cq,
                     float ox, float oy, float oz, float cell, int gx, int gy, int gz, int n_target,
                     const void* target_workspace, size_t target_workspace_bytes, float max_corr_dist, double* moments,
                     float* dist, int* index, void* workspace, size_t workspace_bytes, void* stream);
/* Statistics of a distance array (inf = beyond):
 *   thresholds    [host] n_thresholds floats, each 0 < tau <= max_dist (MVS_E_BADARG otherwise); at most 16 (MVS_E_SHAPE)
 *   out           2 + n_thresholds doubles: sum of d over d < max_dist, count of d < max_dist, count of d < tau_t per threshold
 *   workspace     mvs_dist_stats_workspace_bytes(n, n_thresholds) bytes
 * float64 partial sums per block reduced in block order, integer counts: the same input gives the same bytes. */
size_t mvs_dist_stats_workspace_bytes(int n, int n_thresholds);
int mvs_dist_stats_f32(const float* dist, int n, float max_dist, const float* thresholds, int n_thresholds, double* out,
                       void* workspace, size_t workspace_bytes, void* stream);
/* Voxel downsampling, first point in input order per occupied voxel, in two calls around a stable sort of the keys:
 *   mvs_voxel_keys_f32    keys (n) int64 = kx | ky << 21 | kz << 42, k = floor((x - min) / cell) per axis in float64; the
 *                         caller guarantees k < 2^21 (larger values are clamped)
 *   mvs_voxel_select_f32  sorted_keys (n) int64 and order (n) int64, the keys after a STABLE ascending sort and the input
 *                         index of each; out (n,3) float32 receives the kept points in input order, count (one int32) their
 *                         number; workspace mvs_voxel_select_workspace_bytes(n) bytes */
int mvs_voxel_keys_f32(const float* xyz, int n, double min_x, double min_y, double min_z, double cell, long long* keys,
                       void* stream);
size_t mvs_voxel_select_workspace_bytes(int n);
int mvs_voxel_select_f32(const float* xyz, int n, const long long* sorted_keys, const long long* order, float* out, int* count,
                         void* workspace, size_t workspace_bytes, void* stream);

/* Rendering of a point cloud into per-view depth maps with a z-buffer (csrc/render.hip; semantics in mvsnet_amd/render.py):
 *   xyz           (n,3) float32, read only; non-finite coordinates are allowed (such a point covers no pixel)
 *   order         NULL or (n) int32, a permutation of the points: the order in which lanes take them (points that fall on
 *                 neighbouring pixels side by side run faster); NULL = input order.  It never changes a byte of the output
 *   proj          [device] V*12 floats: P_v = K_v [R_v | t_v] (3x4, row-major) at [v*12], composed in float64, rounded once
 *   splat         s in 0..32: a point covers the (2 s + 1)^2 pixels around its own, clipped to the image
 *   min_depth     >= 0, finite: a point is a candidate in a view only when its depth w > min_depth
 *   occl_radius   0: no hidden-point removal.  k in 1..16: a pixel of raw depth z > 0 is removed when at least occl_count
 *                 (>= 1) other pixels q of its (2 k + 1)^2 window have 0 < raw[q] < z * occl_ratio (0 < occl_ratio < 1)
 *   depth         (V,H,W) float32: per pixel the smallest w of the points that cover it, 0 where empty (or removed)
 *   index         NULL or (V,H,W) int32: the input index of that point (exact ties of w: the smallest), -1 where empty
 *   workspace     mvs_render_workspace_bytes(V, H, W, occlusion) bytes (0 for invalid sizes): the 8-byte keys
 *                 bits(w) << 32 | index of all pixels, which the call clears itself, plus the raw map when occlusion != 0
 * Only enqueues on `stream`: nothing is allocated, nothing synchronised.  The only atomics are 64-bit unsigned minima, so
 * the same inputs give the same bytes in any order and grid.  Every argument is checked before the first GPU call:
 * MVS_E_BADARG for a null pointer or an option outside the ranges above, MVS_E_SHAPE when V*H*W exceeds 2^31-1 or H or W
 * exceeds 2^24 (pixel coordinates are compared as float32), MVS_E_WORKSPACE. */
size_t mvs_render_workspace_bytes(int V, int H, int W, int occlusion);
int mvs_render_points_f32(const float* xyz, int n, const int* order, const float* proj, int V, int H, int W, int splat,
                          float min_depth, int occl_radius, float occl_ratio, int occl_count, float* depth, int* index,
                          void* workspace, size_t workspace_bytes, void* stream);

/* View selection from cameras and a cloud (csrc/view_selection.hip; semantics in mvsnet_amd/select_views.py).  Common to the
 * three calls:
 *   xyz           (n,3) float32, read only; non-finite coordinates are allowed
 *   mask          (n, mask_words) 64-bit words, mask_words >= ceil(V / 64): view position p of point i is bit p % 64 of word
 *                 p / 64 of row i.  Bits at positions >= V are ignored by the readers
 *   proj          [device] 12 floats per view, as mvs_render_points_f32 takes them
 * mvs_view_visibility_f32: the V views of one size H x W; sets, never clears, the bit view_bits[v] of every point visible
 * in view v (the caller zeroes the mask before the first call; a view_bits entry outside 0 .. 64 mask_words - 1 is left out).
 *   view_bits     [device] (V) int32: the bit position of each of the call's views
 *   min_depth     >= 0, finite: visible only when w > min_depth
 *   zbuf          NULL (frustum) or (V,H,W) float32 depth maps of the call's views: visible only when the map is > 0 at the
 *                 point's pixel and w <= map * z_tol (z_tol >= 1, a float32 product)
 * mvs_view_scores_f32: over all pairs a < b < V of view positions, shared[a V + b] = the number of points with both bits set
 * and score_sum[a V + b] = the sum of table[k] over them (select_views.py, "pair score"); both (V,V) int64, cleared by the
 * call, entries with a >= b stay 0.
 *   order         NULL or (n) int32, a permutation of the points: which lane takes which point, never an output byte
 *   centres       [device] (V,3) float32 camera centres by view position
 *   table         [device] 8192 uint16 weights
 *   workspace     mvs_view_scores_workspace_bytes(n, V) bytes (0 for invalid sizes): the work counters, cleared by the call
 * mvs_view_depth_hist_f32: histograms of the float32 bits of w = row 2 of proj[v] applied to the point, over the points with
 * bit v set; proj holds all V views by position.  The call clears hist.
 *   pass 0        prefixes NULL; hist (V, 65536) uint32 counts of bits(w) >> 16
 *   pass 1        prefixes [device] (V,2) int32; hist (V, 2, 65536) uint32: hist[v][j] counts bits(w) & 0xffff over the points
 *                 with bits(w) >> 16 == prefixes[v][j]
 * All three only enqueue on `stream`: nothing is allocated, nothing synchronised, and every accumulation is an integer, so
 * the same inputs give the same bytes in any order and grid.  Every argument is checked before the first GPU call:
 * MVS_E_BADARG for a null pointer or an option outside the ranges above, MVS_E_SHAPE for V > 512, n < 1,
 * mask_words < ceil(V / 64), H or W beyond 2^24 or V*H*W beyond 2^31-1, MVS_E_WORKSPACE. */
int mvs_view_visibility_f32(const float* xyz, int n, const float* proj, const int* view_bits, int V, int H, int W,
                            float min_depth, const float* zbuf, float z_tol, unsigned long long* mask, int mask_words,
                            void* stream);
size_t mvs_view_scores_workspace_bytes(int n, int V);
int mvs_view_scores_f32(const float* xyz, int n, const int* order, const unsigned long long* mask, int mask_words,
                        const float* centres, int V, const unsigned short* table, long long* score_sum, long long* shared,
                        void* workspace, size_t workspace_bytes, void* stream);
int mvs_view_depth_hist_f32(const float* xyz, int n, const float* proj, int V, const unsigned long long* mask, int mask_words,
                            int pass, const int* prefixes, unsigned int* hist, void* stream);

/* TSDF fusion of depth maps into a volume and surface-nets extraction of a triangle mesh (csrc/tsdf.hip; semantics in
 * mvsnet_amd/mesh.py).  The volume has nx x ny x nz nodes, node (i, j, k) at linear index (k ny + j) nx + i and at
 * origin + voxel (i, j, k); at most 2^31-1 nodes (MVS_E_SHAPE beyond).
 *   origin        [host] 3 finite floats;  voxel > 0 and trunc > 0, finite
 *   sum, count    (nz,ny,nx) float32 / int32: the truncated signed distances added so far and their number
 *   rgb_sum       NULL or (nz,ny,nx,3) uint32, with rgb_count (nz,ny,nx) int32: colour sums and their number
 * mvs_tsdf_integrate_f32 adds the V views of one size H x W, in ascending order, to sum and count (and, when images is not
 * NULL, to rgb_sum and rgb_count, which are then required); a later call continues the same sums.
 *   depth, prob   (V,H,W) float32; a pixel counts when depth > 0, finite and prob >= prob_threshold (not NaN)
 *   proj          [device] V*12 floats, as mvs_render_points_f32 takes them
 *   images        NULL or (V,img_h,img_w,3) uint8
 *   flags         reserved, must be 0
 *   workspace     mvs_tsdf_integrate_workspace_bytes(V, H, W) bytes (0 for invalid sizes): the filtered depth maps
 * MVS_E_SHAPE for H, W, img_h or img_w beyond 2^24 or V*H*W beyond 2^31-1.
 * mvs_surface_nets_count_f32 classifies cells and node edges (a node is observed when count >= min_count >= 1):
 *   totals        [device] 2 int32, cleared by the call: the number of vertices M and of triangles F
 *   workspace     mvs_surface_nets_workspace_bytes(nx, ny, nz) bytes: per cell, in linear cell order
 *                 (k (ny-1) + j) (nx-1) + i, an int32 with bit 0 = valid and bit 1 = active (one zero when an axis has one
 *                 node), then, 256-byte aligned, per node an int32 triangle count.  The caller scans both
 * mvs_surface_nets_write_f32 writes the mesh from the same volume, min_count and workspace as the count call left them:
 *   cell_rank     [device] per cell int32: the inclusive scan of the active bits (a cell's vertex id is its rank - 1)
 *   face_end      [device] per node int32: the inclusive scan of the triangle counts
 *   M, F          capacities of the outputs; a vertex or triangle beyond them is not written
 *   vertices      (M,3) float32;  colours (M,3) uint8 (0 without rgb_sum);  faces (F,3) int32, ordered by node, then axis
 * All three only enqueue on `stream`: nothing is allocated, nothing synchronised, a node or cell has one writer and the only
 * atomics are the two integer totals, so the same inputs give the same bytes.  Every argument is checked before the first
 * GPU call (MVS_E_BADARG, MVS_E_SHAPE, MVS_E_WORKSPACE) and the outputs are untouched on error. */
size_t mvs_tsdf_integrate_workspace_bytes(int V, int H, int W);
int mvs_tsdf_integrate_f32(const float* depth, const float* prob, int V, int H, int W, const float* proj,
                           const unsigned char* images, int img_h, int img_w, const float* origin, float voxel, int nx, int ny,
                           int nz, float trunc, float prob_threshold, int flags, float* sum, int* count, unsigned int* rgb_sum,
                           int* rgb_count, void* workspace, size_t workspace_bytes, void* stream);
size_t mvs_surface_nets_workspace_bytes(int nx, int ny, int nz);
int mvs_surface_nets_count_f32(const float* sum, const int* count, int nx, int ny, int nz, int min_count, int* totals,
                               void* workspace, size_t workspace_bytes, void* stream);
int mvs_surface_nets_write_f32(const float* sum, const int* count, const unsigned int* rgb_sum, const int* rgb_count,
                               const float* origin, float voxel, int nx, int ny, int nz, int min_count, const int* cell_rank,
                               const int* face_end, int M, int F, float* vertices, unsigned char* colours, int* faces,
                               void* workspace, size_t workspace_bytes, void* stream);

/* Rasterisation of a triangle mesh into per-view depth maps with a z-buffer, and interpolation of vertex attributes over
 * the result (csrc/raster.hip; semantics in mvsnet_amd/render_mesh.py).
 *   vertices      (M,3) float32, read only; non-finite coordinates are allowed (their faces are dropped)
 *   faces         (F,3) int32; a face that names a vertex outside 0..M-1 is dropped and never dereferenced
 *   order         NULL or (F) int32, a permutation of the faces: the order in which lanes take them; NULL = input order
 *   proj          [device] 12 floats per view, as mvs_render_points_f32 takes them
 *   min_depth     >= 0 and finite: a vertex at or below it makes its faces drop out of that view (nothing is clipped)
 *   cull          0 keeps every face, +1 drops those of positive screen area (the back faces of an outward-wound mesh),
 *                 -1 those of negative
 *   large_pixels  a (face, view) pair whose clipped bounding box holds more pixels goes through the queue to the second
 *                 kernel, where a workgroup strides over the box; queue_capacity entries of 8 bytes, and a pair that finds
 *                 the queue full is drawn by its lane.  Neither changes a byte of the output
 *   depth         (V,H,W) float32: per pixel the smallest perspective-correct depth of the faces that cover it, 0 where empty
 *   index         NULL or (V,H,W) int32: that face (exact ties of depth: the smallest index), -1 where empty
 *   workspace     mvs_raster_workspace_bytes(V, H, W, queue_capacity) bytes (0 for invalid sizes): the queue counter, the
 *                 8-byte keys bits(z) << 32 | face of all pixels and the queue; the call clears what it needs
 * mvs_raster_interpolate_f32: index (V,H,W) int32 as the mesh call wrote it, attr (M,C) float32 with 1 <= C <= 8 ->
 * out (V,H,W,C) float32, perspective-correct in float64; 0 where the pixel is empty, its index is outside 0..F-1 or its face
 * is dropped in that view.
 * Both only enqueue on `stream`: nothing is allocated, nothing synchronised.  The only atomics on the output are 64-bit
 * unsigned minima, so the same inputs give the same bytes in any order and grid.  Every argument is checked before the
 * first GPU call: MVS_E_BADARG for a null pointer or an option outside the ranges above, MVS_E_SHAPE when V*H*W exceeds
 * 2^31-1 or H or W exceeds 2^20 (256 x stays inside the guard band of 2^28), MVS_E_WORKSPACE; outputs are untouched on error. */
size_t mvs_raster_workspace_bytes(int V, int H, int W, int queue_capacity);
int mvs_raster_mesh_f32(const float* vertices, int M, const int* faces, int F, const int* order, const float* proj, int V,
                        int H, int W, float min_depth, int cull, int large_pixels, int queue_capacity, float* depth,
                        int* index, void* workspace, size_t workspace_bytes, void* stream);
int mvs_raster_interpolate_f32(const float* vertices, int M, const int* faces, int F, const float* proj, int V, int H, int W,
                               float min_depth, const int* index, const float* attr, int C, float* out, void* stream);

/* Connected components of a triangle mesh, their measures, and the compaction of a selection of them (csrc/mesh_components.hip;
 * semantics in mvsnet_amd/mesh_clean.py).  M vertices and F faces, each 0..2^31-1 (negative: MVS_E_BADARG, beyond: MVS_E_SHAPE);
 * a pointer to an array of M or F entries may be NULL when that size is 0.
 *   vertices      (M,3) float32, read only; a face with a non-finite vertex is invalid
 *   faces         (F,3) int32; a face that names a vertex outside 0..M-1 is invalid and never dereferenced
 *   workspace     mvs_mesh_components_workspace_bytes(M, F) bytes (0 for invalid sizes): 64 int32 status words, then the
 *                 union-find parents and the smallest index under each root.  Status word 0 is the error word (non-zero: a lane ran past the cap on walk steps and
 *                 retries, the result is void), word 1 the number of invalid faces, word 2 the number of unreferenced vertices
 * mvs_mesh_components_label_i32 clears the status words and writes
 *   vertex_labels (M) int32: the smallest vertex index of the vertex's component
 *   face_labels   (F) int32: the label of the face's first vertex, -1 for an invalid face
 * mvs_mesh_components_measure_f32 takes the labels and the workspace as the label call left them and writes
 *   counts        (M) int32: at index L the number of faces of label L (0 where L is no label, or that of an unreferenced vertex)
 *   boxes         (M,6) uint32: at row L the minima (x, y, z) and maxima (x, y, z) over the vertices of component L as ordered
 *                 images of their float32 bits (bits ^ 0x80000000 for a clear sign bit, ~bits otherwise); 0xffffffff and 0 where
 *                 the component has no face
 * mvs_mesh_compact_mark_i32: keep_label (M) int32, non-zero at the labels to keep ->
 *   face_keep     (F) int32: 1 for a face whose label is kept, else 0
 *   vertex_keep   (M) int32: 1 for a vertex that a kept face names, else 0
 * mvs_mesh_compact_write_f32: face_rank and vertex_rank are the inclusive prefix sums of face_keep and vertex_keep, F_out and
 * M_out their last entries -> out_vertices (M_out,3), out_colours (M_out,3) (colours and out_colours NULL together),
 * out_faces (F_out,3) re-indexed, all in input order.
 * All four only enqueue on `stream`: nothing is allocated, nothing synchronised.  The only atomics on outputs are integer sums,
 * minima and maxima, so the same inputs give the same bytes in any order and grid.  Every argument is checked before the first
 * GPU call (MVS_E_BADARG, MVS_E_SHAPE, MVS_E_WORKSPACE) and the outputs are untouched on error. */
size_t mvs_mesh_components_workspace_bytes(long long M, long long F);
int mvs_mesh_components_label_i32(const float* vertices, long long M, const int* faces, long long F, int* vertex_labels,
                                  int* face_labels, void* workspace, size_t workspace_bytes, void* stream);
int mvs_mesh_components_measure_f32(const float* vertices, long long M, long long F, const int* vertex_labels,
                                    const int* face_labels, int* counts, unsigned int* boxes, void* workspace,
                                    size_t workspace_bytes, void* stream);
int mvs_mesh_compact_mark_i32(const int* faces, long long M, long long F, const int* face_labels, const int* keep_label,
                              int* face_keep, int* vertex_keep, void* stream);
int mvs_mesh_compact_write_f32(const float* vertices, const unsigned char* colours, long long M, const int* faces, long long F,
                               const int* face_keep, const int* face_rank, const int* vertex_keep, const int* vertex_rank,
                               long long M_out, long long F_out, float* out_vertices, unsigned char* out_colours, int* out_faces,
                               void* stream);

/* Mesh simplification by vertex clustering on a uniform grid of cells (csrc/mesh_simplify.hip; semantics in
 * mvsnet_amd/mesh_simplify.py).  M vertices and F faces, each 0..2^31-1 (negative: MVS_E_BADARG, beyond: MVS_E_SHAPE); a pointer
 * to an array of M or F entries may be NULL when that size is 0.  origin and cell are float32, finite, cell > 0 (else
 * MVS_E_BADARG); the kernels widen them to float64.  The caller sorts and scans between the calls:
 *   mvs_mesh_cluster_keys_f32   vertices (M,3) float32, faces (F,3) int32 -> keys (M) int64: the cell key kx | ky << 21 | kz << 42
 *                 of a vertex that a valid face names, else -1; offsets (M,3) int32: floor(fraction of the cell * 2^20), 0 for a
 *                 vertex that is not clusterable.  Clears the status words; counts words 0 and 1
 *   (a stable ascending sort of keys -> sorted_keys, order (M) int64)
 *   mvs_mesh_cluster_heads_i64  -> head (M) int32: 1 where a run of equal sorted keys >= 0 starts, else 0
 *   (an inclusive scan of head -> head_rank (M) int32; its last entry is the number of clusters K)
 *   mvs_mesh_cluster_sums_f32   colours NULL or (M,3) uint8 -> vertex_cluster (M) int32: the cluster (rank - 1, ascending key
 *                 order) of a contributing vertex, else -1; cluster_vertices (M,3) float32 and cluster_colours (M,3) uint8
 *                 (NULL together with colours): rows 0..K-1 are written, the rest is left alone
 *   mvs_mesh_cluster_faces_i32  -> cluster_faces (F,3) int32: the three clusters, -1 -1 -1 for an invalid face; key_lo (F) int64
 *                 and key_hi (F) int64 or NULL: the sort key of a valid face with three different clusters x < y < z is
 *                 x << 42 | y << 21 | z in key_lo when key_hi is NULL (M <= 2^21, else MVS_E_SHAPE), otherwise key_hi = x,
 *                 key_lo = y << 32 | z; INT64_MAX in both for every other face.  Counts status word 2
 *   (a stable ascending sort by (key_hi, key_lo) -> sorted_lo, sorted_hi or NULL, order (F) int64)
 *   mvs_mesh_cluster_mark_i32   -> face_keep (F) int32: 1 for the first face of a run of equal keys if it is valid and not
 *                 degenerate, else 0; vertex_keep (M) int32: 1 for a cluster that a kept face names, else 0.  Counts word 3
 *   (inclusive scans of both, then mvs_mesh_compact_write_f32 on cluster_vertices, cluster_colours and cluster_faces with M = K)
 *   workspace     mvs_mesh_cluster_workspace_bytes(M, F) bytes (0 for invalid sizes), one for all calls of a mesh: 64 int32
 *                 status words (0 invalid faces, 1 unclusterable vertices, 2 degenerate faces, 3 duplicate faces), the use
 *                 marks of the vertices, and 8 int64 per cluster slot (n, the offset sums, the colour sums, the key)
 * All five only enqueue on `stream`: nothing is allocated, nothing synchronised.  The only atomics are integer sums, so the
 * same inputs give the same bytes in any order and grid.  Every argument is checked before the first GPU call (MVS_E_BADARG,
 * MVS_E_SHAPE, MVS_E_WORKSPACE) and the outputs are untouched on error.  Indices that the caller computed (order, head_rank,
 * vertex_cluster, cluster_faces) are range-checked before they are used. */
size_t mvs_mesh_cluster_workspace_bytes(long long M, long long F);
int mvs_mesh_cluster_keys_f32(const float* vertices, long long M, const int* faces, long long F, float origin_x, float origin_y,
                              float origin_z, float cell, long long* keys, int* offsets, void* workspace, size_t workspace_bytes,
                              void* stream);
int mvs_mesh_cluster_heads_i64(const long long* sorted_keys, long long M, int* head, void* stream);
int mvs_mesh_cluster_sums_f32(const long long* sorted_keys, const long long* order, const int* head_rank, const int* offsets,
                              const unsigned char* colours, long long M, float origin_x, float origin_y, float origin_z,
                              float cell, int* vertex_cluster, float* cluster_vertices, unsigned char* cluster_colours,
                              void* workspace, size_t workspace_bytes, void* stream);
int mvs_mesh_cluster_faces_i32(const int* faces, long long M, long long F, const int* vertex_cluster, int* cluster_faces,
                               long long* key_lo, long long* key_hi, void* workspace, size_t workspace_bytes, void* stream);
int mvs_mesh_cluster_mark_i32(const int* cluster_faces, long long M, long long F, const long long* sorted_lo,
                              const long long* sorted_hi, const long long* order, int* face_keep, int* vertex_keep,
                              void* workspace, size_t workspace_bytes, void* stream);

/* Sampling of a triangle mesh's surface into a point cloud (csrc/mesh_sample.hip; semantics in mvsnet_amd/mesh_sample.py).
 * M vertices, 0..2^31-1, and F faces, 0..2^26 (negative: MVS_E_BADARG, beyond: MVS_E_SHAPE); a pointer to an array of M or F
 * entries may be NULL when that size is 0.
 *   mvs_mesh_sample_quota_f32   vertices (M,3) float32, faces (F,3) int32, density (samples per unit area, finite and > 0, else
 *                 MVS_E_BADARG) -> quota (F) int64: floor(area * density * 2^16), 0 for a face that is invalid (an index outside
 *                 0..M-1 or a vertex that is not finite), has no area or is saturated (2^36 or more).  Clears the status words
 *                 and counts words 0 (invalid), 1 (zero area) and 2 (saturated)
 *   (an inclusive int64 scan of quota -> sums (F); the number of samples is N = sums[F - 1] >> 16)
 *   mvs_mesh_sample_write_f32   colours NULL or (M,3) uint8; sums (F) int64; N samples, 0..2^31-1; seed, any 64 bits ->
 *                 out_xyz (N,3) float32 and, each unless NULL, out_face (N) int32, out_colours (N,3) uint8 (needs colours, else
 *                 MVS_E_BADARG) and out_normals (N,3) float32.  Sample g lies in the first face f with (sums[f] >> 16) > g.  Sums
 *                 that are not the scan of the quota give zeros and face -1 for the samples that find no face with indices
 *                 inside 0..M-1: every index read from sums or faces is range-checked before it is used
 *   workspace     mvs_mesh_sample_workspace_bytes(M, F) bytes (0 for invalid sizes): 64 int32 status words
 * Both only enqueue on `stream`: nothing is allocated, nothing synchronised.  The only atomics are integer counts, and a sample
 * depends on (seed, g) and its face alone: the same inputs give the same bytes on any grid.  Every argument is checked before
 * the first GPU call and the outputs are untouched on error. */
size_t mvs_mesh_sample_workspace_bytes(long long M, long long F);
int mvs_mesh_sample_quota_f32(const float* vertices, long long M, const int* faces, long long F, double density, long long* quota,
                              void* workspace, size_t workspace_bytes, void* stream);
int mvs_mesh_sample_write_f32(const float* vertices, const unsigned char* colours, long long M, const int* faces, long long F,
                              const long long* sums, long long N, unsigned long long seed, float* out_xyz, int* out_face,
                              unsigned char* out_colours, float* out_normals, void* stream);

/* Taubin smoothing of a triangle mesh: Jacobi passes over a sorted adjacency structure (csrc/mesh_smooth.hip; semantics in
 * mvsnet_amd/mesh_smooth.py).  M vertices, 0..2^31-1, and F faces with 6 F <= 2^31-1 (negative: MVS_E_BADARG, beyond:
 * MVS_E_SHAPE); E = 6 F.  A pointer to an array of M, F or E entries may be NULL when that size is 0.  The caller sorts and
 * scans between the calls:
 *   mvs_mesh_smooth_edges_i64   vertices (M,3) float32, faces (F,3) int32 -> keys (E) int64: per face the directed edges a>b b>a
 *                 b>c c>b c>a a>c as int64(s) << 31 | t; INT64_MAX for an edge with s == t or an end that is not finite, and for
 *                 all six of a face with an index outside 0..M-1.  Clears the status words; counts words 0 and 1
 *   (an ascending sort of keys -> sorted_keys (E) int64)
 *   mvs_mesh_smooth_heads_i64   -> head (E) int32: 1 where a run of equal live keys starts, else 0.  Counts words 2 and 3
 *   (an inclusive scan of head -> head_rank (E) int32; its last entry is the number of unique directed edges U)
 *   mvs_mesh_smooth_rows_i32    boundary 0 fixed, 1 curve, 2 free (else MVS_E_BADARG) -> neighbours (E) int32: entries 0..U-1
 *                 are written, the target in bits 0..30 and bit 31 set on a boundary edge, the rest is left alone; row_start
 *                 (M + 1) int32: the unique edges whose source is below v; vertex_class (M) uint8: 0 fixed, 1 curve, 2 interior.
 *                 Counts words 4 and 5
 *   mvs_mesh_smooth_step_f32    one pass X -> Y (never the same array: MVS_E_BADARG) with the float32 factor (finite) over the
 *                 rows; V0 the positions the bound is taken from, max_displacement r >= 0 or negative for none (NaN, +inf:
 *                 MVS_E_BADARG); N the entries of neighbours, 0..2^31-1, against which the row bounds are checked.  X, V0 and Y
 *                 are (M, row_floats) float32 with row_floats 3, or 4 with 16-byte aligned arrays, where the fourth float
 *                 travels from X to Y as it is
 *   workspace     mvs_mesh_smooth_workspace_bytes(M, F) bytes (0 for invalid sizes): 64 int32 status words (0 invalid faces,
 *                 1 vertices that are not finite, 2 boundary edges, 3 non-manifold edges, 4 boundary vertices, 5 fixed vertices);
 *                 each call clears the words it counts
 * All four only enqueue on `stream`: nothing is allocated, nothing synchronised.  The only atomics are integer counts, and the
 * sums of a pass run in one order, so the same inputs give the same bytes on any grid.  Every argument is checked before the
 * first GPU call and the outputs are untouched on error.  Every index read from an array (faces, head_rank, row_start,
 * neighbours) is range-checked before it is used. */
size_t mvs_mesh_smooth_workspace_bytes(long long M, long long F);
int mvs_mesh_smooth_edges_i64(const float* vertices, long long M, const int* faces, long long F, long long* keys, void* workspace,
                              size_t workspace_bytes, void* stream);
int mvs_mesh_smooth_heads_i64(const long long* sorted_keys, long long F, int* head, void* workspace, size_t workspace_bytes,
                              void* stream);
int mvs_mesh_smooth_rows_i32(const long long* sorted_keys, const int* head, const int* head_rank, long long M, long long F,
                             int boundary, int* neighbours, int* row_start, unsigned char* vertex_class, void* workspace,
                             size_t workspace_bytes, void* stream);
int mvs_mesh_smooth_step_f32(const float* X, const float* V0, const int* row_start, const int* neighbours,
                             const unsigned char* vertex_class, long long M, long long N, int row_floats, float factor,
                             float max_displacement, float* Y, void* stream);

/* Vertex normals and per-vertex colour from the full-resolution images (csrc/mesh_colour.hip; semantics in
 * mvsnet_amd/mesh_colour.py).  M vertices, 0..2^31-1, and F faces with 3 F <= 2^31-1 (negative: MVS_E_BADARG, beyond:
 * MVS_E_SHAPE); E = 3 F.  A pointer to an array of M, F, E or V entries may be NULL when that size is 0.  The caller sorts
 * between the first two calls and rasterises the depth maps (mvs_raster_mesh_f32, cull 0) before the third:
 *   mvs_mesh_normals_keys_i64   vertices (M,3) float32, faces (F,3) int32 -> keys (E) int64: per valid face (indices in 0..M-1
 *                 and pairwise different, nine finite coordinates) int64(vertex) << 31 | f for its three corners, INT64_MAX
 *                 three times otherwise.  Clears the status words; counts word 0
 *   (an ascending sort of keys -> sorted_keys (E) int64)
 *   mvs_mesh_normals_f32        -> normals (M,3) float32: per vertex the float64 sum of (b - a) x (c - a) over its run of
 *                 faces, ascending, normalised and rounded once; (0,0,0) where the run is empty or the length is 0 or not
 *                 finite.  Counts word 1
 *   mvs_mesh_colour_accumulate_f32  V views of H x W (H, W <= 2^20, V H W <= 2^31-1: else MVS_E_SHAPE), in ascending order: proj
 *                 (V,12) float32 as render.projection_tables gives it, centres (V,3) float32, depth (V,H,W) float32, images
 *                 (V,H,W,3) uint8 (byte offsets in 64 bits); min_depth >= 0 and ratio > 0 finite, min_cos in [-1, 1], power
 *                 0..8 (else MVS_E_BADARG).  Every vertex a view sees adds its weighted bilinear sample to acc (M,4) float64
 *                 (16-byte aligned: three channel sums and the weight) and 1 to seen (M) int32; both continue what they hold,
 *                 so the caller zeroes them before the first call of a mesh.  acc and seen must not be one of the inputs
 *   mvs_mesh_colour_finish_u8   colours (M,3) uint8 or NULL, acc, seen -> out (M,3) uint8 (never one of the inputs): the byte
 *                 floor(acc[k] / acc[3] + 1/2) clamped to 0..255 where seen > 0 and acc[3] > 0, else the input colour, or 0
 *                 without one.  Counts word 2
 *   workspace     mvs_mesh_colour_workspace_bytes(M, F) bytes (0 for invalid sizes): 64 int32 status words (0 invalid faces,
 *                 1 vertices with a zero normal, 2 vertices no view saw); each call clears the words it counts.  The
 *                 accumulation counts nothing and takes no workspace
 * All four only enqueue on `stream`: nothing is allocated, nothing synchronised.  The only atomics are integer counts; a
 * vertex's sums run in one lane in the order of the views, so the same inputs give the same bytes on any grid, and two calls
 * over two halves of the views give the bytes of one call over all.  Every argument is checked before the first GPU call and
 * the outputs are untouched on error.  Every index read from an array (faces, the face of a key) is range-checked before it
 * is used, and a pixel is compared with the image in float32 before it is converted. */
size_t mvs_mesh_colour_workspace_bytes(long long M, long long F);
int mvs_mesh_normals_keys_i64(const float* vertices, long long M, const int* faces, long long F, long long* keys, void* workspace,
                              size_t workspace_bytes, void* stream);
int mvs_mesh_normals_f32(const float* vertices, long long M, const int* faces, long long F, const long long* sorted_keys,
                         float* normals, void* workspace, size_t workspace_bytes, void* stream);
int mvs_mesh_colour_accumulate_f32(const float* vertices, const float* normals, long long M, const float* proj,
                                   const float* centres, int V, int H, int W, const float* depth, const unsigned char* images,
                                   float min_depth, float ratio, float min_cos, int power, double* acc, int* seen, void* stream);
int mvs_mesh_colour_finish_u8(const unsigned char* colours, const double* acc, const int* seen, long long M, unsigned char* out,
                              void* workspace, size_t workspace_bytes, void* stream);

#ifdef __cplusplus
}
#endif
#endif /* MVSNET_HIP_H_ */
