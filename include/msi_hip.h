/*
 * msi_hip.h -- C ABI of libmsi_hip.so: the MI355X (gfx950) native kernels of the
 * multi-sphere-image infer -> render hot path.
 *
 * The reference (brownvc/matryodshka) has no native code and no FFI: its only
 * seam is the Python class matryodshka.msi.MSI called from test.py:127-159.
 * Each entry point below therefore cites the reference *Python function* whose
 * arithmetic it replaces (file:line inside the reference checkout); the Python
 * class matryodshka_amd.msi.MSI keeps the reference's method signatures and is
 * the only caller (INTEGRATION.md shows the ctypes binding).
 *
 * Conventions
 *   - plain pointers and sizes only; no C++ or torch types cross this boundary;
 *   - the CALLER owns every buffer (device pointers unless the name ends in
 *     `_host`); the library never allocates persistent device memory; scratch
 *     is passed in, sized by the matching `*_workspace_bytes` query;
 *   - every launch is asynchronous on `stream` (a hipStream_t passed as void*;
 *     NULL = the default stream); no hidden synchronisation;
 *   - return value: MSI_OK (0) or a negative MSI_E_* code; never a C++
 *     exception; msi_last_error_string() gives the thread-local detail;
 *   - re-entrant: no mutable global state besides the thread-local error text;
 *   - all tensors are contiguous fp32 in the documented layout, dims int32.
 *
 * Layouts
 *   image        [B,H,W,3]     preprocessed, range [-1,1]
 *   psv          [B,H,W,C]     C = 6*D for the two-source ODS volume; channel
 *                              = src*3D + d*3 + c (projector.py:164-169,
 *                              msi.py:1124-1129)
 *   pred         [B,H,W,2*D]   tanh output of the CNN (blend weights | alphas)
 *   rgba_native  [B,D,H,W,4]   the layer stack, D-major (what msi.py:422
 *                              transposes to before warping); float4 texels
 *   out          [B,H,W,3]
 *   trig         [2W+2H]       cosS[W] sinS[W] cosT[H] sinT[H] of the lat-long
 *                              grid (spherical.py:42-44), host-built
 */
#ifndef MSI_HIP_H
#define MSI_HIP_H

#include <stddef.h>
#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

#define MSI_OK 0
#define MSI_E_BADARG (-1)
#define MSI_E_LAUNCH (-2)
#define MSI_E_UNSUPPORTED (-3)
#define MSI_E_WORKSPACE (-4)
#define MSI_E_RANGE (-5) /* msi_net_plan_status: a LayerNorm statistic left the range the kernels resolve */

typedef void *msi_stream_t; /* hipStream_t */

const char *msi_version(void);
/* ABI version of this header: bumped whenever a struct of this file grows or changes layout, an entry point changes
 * its signature, or the PACKED weight blob (msi_net_pack_weights_host) changes format.  A caller compares
 * msi_abi_version() of the library it loaded with the MSI_ABI_VERSION it was compiled against and refuses to run on
 * a mismatch; packed blobs are not portable across versions (re-pack from the parameter blob).
 *   3: msi_layer_info.ln_scale_offset; LayerNorm window doubles in the packed blob (round 3)
 *   4: msi_net_plan_layer_kernel; render status word (msi_render_status_*); sweep volume takes shared poses (round 4)
 *   5: packed blob carries the fp16-split (x2) block; MSI_NET_OPT_F32_SPLIT_F16, MSI_NET_STATUS_F16_SPLIT_RANGE (round 4)
 *   6: msi_net_plan_calibrate; MSI_NET_OPT_X3_TILE8 (round 5)
 *   7: MSI_NET_OPT_X3_ROWPAR (round 5)
 *   8: msi_probe_matrix_rate (round 6)
 *   9: msi_perspective_sweep_volume_bf16
 *      (additions since, no bump: msi_mpi_render_views; msi_score_workspace_bytes, msi_score_images; msi_cube_render_views,
 *      msi_equirect_to_cube_f32; msi_sparse_index_tiles, msi_sparse_gather_tiles, msi_sparse_expand, msi_render_views_sparse;
 *      msi_hres_index_tiles, msi_hres_layers_sparse; msi_sparse_index_tiles_edge, msi_mpi_render_views_sparse,
 *      msi_cube_render_views_sparse; msi_pp_hres_layers, msi_hres_index_tiles_edge, msi_pp_hres_layers_sparse;
 *      msi_cube_plane_sweep_f32, msi_cube_sweep_volume_bf16, msi_cube_hres_layers, msi_cube_hres_layers_sparse;
 *      msi_cube_render_views_seamless, MSI_RENDER_STATUS_NOT_CUBE_CAMERA; msi_cube_render_ods_views,
 *      msi_cube_render_ods_views_sparse; msi_render_views_factored; msi_build_mips, msi_render_views_mip; msi_render_views_aniso) */
#define MSI_ABI_VERSION 9
int32_t msi_abi_version(void);
const char *msi_last_error_string(void);
/* CRC-32C (Castagnoli) of a host buffer, continuing from `crc` (0 for a new message): the per-tensor checksum of
 * the TensorFlow checkpoints test.py:191-202 restores (matryodshka_amd/tf_checkpoint.py verifies it on load). */
uint32_t msi_crc32c_host(const void *data_host, size_t n, uint32_t crc);

/* Measurement aid (round 6; bench.py's `roofline.frac_of_sustained`; no reference counterpart): `num_workgroups` workgroups of four waves issue
 * `iterations` x 12 v_mfma_f32_32x32x16_bf16 back to back per wave -- no memory or LDS traffic -- on operands that change between consecutive instructions
 * (changing_operands = 1) or stay constant (0).  Dense bf16 flops = num_workgroups x 4 x iterations x 12 x 2 x 32 x 32 x 16; time it with events on `stream`.
 * ticks_device (may be NULL): [num_workgroups][2] = per-workgroup deltas of s_memtime (shader-clock cycles) and s_memrealtime (100 MHz).  sink_device: one float. */
int32_t msi_probe_matrix_rate(int32_t changing_operands, int64_t iterations, int32_t num_workgroups, uint64_t *ticks_device, float *sink_device,
                              msi_stream_t stream);

/* ---- geometry tables (host) -------------------------------------------------
 * spherical.lat_long_grid (spherical.py:42-44) is separable; the kernels take
 * cos/sin of its two axes as a table.  tf.linspace fp32 semantics, then the
 * correctly rounded fp32 cos/sin of each fp32 angle (DESIGN.md "trig tables"). */
size_t msi_trig_table_floats(int32_t height, int32_t width);
int msi_build_trig_tables_host(int32_t height, int32_t width, float *out_host);

/* ---- pre / de-process -------------------------------------------------------
 * MSI.preprocess_image (msi.py:1163-1171): uint8 -> x*(1/255), then x*2-1. */
int msi_preprocess_u8_f32(const uint8_t *in, float *out, size_t n, msi_stream_t stream);
int msi_preprocess_f32(const float *in, float *out, size_t n, msi_stream_t stream);
/* both images of a frame (raw_src_image, raw_ref_image of infer_msi, msi.py:73-75) in one launch */
int msi_preprocess_pair_u8_f32(const uint8_t *in0, const uint8_t *in1, float *out0, float *out1, size_t n,
                               msi_stream_t stream);
/* MSI.deprocess_image (msi.py:1173-1181): trunc(((x+1)/2)*255.5) -> uint8;
 * is_depth != 0: MSI.deprocess_depth_image (msi.py:1186-1194): trunc(x*255.5).
 * Values are clamped to [0,255] before the cast. */
int msi_deprocess_f32_u8(const float *in, uint8_t *out, size_t n, int32_t is_depth,
                         msi_stream_t stream);
/* deprocess_image(rgb) and deprocess_depth_image(depth) of test.py:149-159 in one launch (n elements each) */
int msi_deprocess_pair_f32_u8(const float *rgb, const float *depth, uint8_t *out_rgb, uint8_t *out_depth, size_t n,
                              msi_stream_t stream);

/* out[b] = lhs[b] @ rhs[b] for [B,4,4] row-major poses, terms summed k = 0..3 without fma:
 * curr_pose = psv_src_pose @ ref_pose_inv (msi.py:1125), tgt_pose @ interp_pose_inv (msi.py:644-646).
 * One 16-thread-per-sample launch instead of a BLAS call in the frame loop. */
int msi_compose_poses_f32(const float *lhs, const float *rhs, float *out, int32_t batch,
                          msi_stream_t stream);

/* ---- K1: ODS sphere sweep -----------------------------------------------------
 * pj.ods_sphere_sweep -> sweep_one (projector.py:209-211, 129-170) with
 * backproject_spherical (spherical.py:116-129), apply_pose (projector.py:275-291),
 * project_ods (spherical.py:170-233) and the wrap-around bilinear gather
 * sampling.resample (sampling.py:135-197), fused; nothing is materialised but
 * the output.  The part of project_ods that decides its branches (up to the discriminant) is IEEE fp32 op for op;
 * the continuous remainder (root, angles, pixel coordinates) uses 1-ulp primitives (<= 2e-5 px).  Writes channels [channel_offset, channel_offset+3*D) of psv.
 *   pose [B,4,4] (curr_pose = src_pose @ ref_pose_inv, msi.py:1125),
 *   intrinsics [B,3,3] (ODS baseline in [b,0,0], data_loader.py:160),
 *   depths [D], order = +1 (ref) / -1 (src) (msi.py:1127). */
int msi_ods_sphere_sweep_f32(const float *image, const float *pose, const float *intrinsics,
                             const float *depths, const float *trig, int32_t batch,
                             int32_t height, int32_t width, int32_t num_depths, int32_t order,
                             float *psv, int32_t psv_channels, int32_t channel_offset,
                             msi_stream_t stream);

/* Same sweep with a bf16 volume (round to nearest even): the network input of BASELINE
 * configs[2]; everything up to the final store is the fp32 arithmetic above. */
int msi_ods_sphere_sweep_bf16(const float *image, const float *pose, const float *intrinsics,
                              const float *depths, const float *trig, int32_t batch,
                              int32_t height, int32_t width, int32_t num_depths, int32_t order,
                              void *psv_bf16, int32_t psv_channels, int32_t channel_offset,
                              msi_stream_t stream);

/* The whole double volume of MSI.format_network_input (msi.py:1124-1129) in one launch: ref_image with order +1
 * into channels [0,3D), src_image with order -1 into [3D,6D) of psv [B,H,W,6D] (fp32, or bf16 when psv_is_bf16 != 0).
 * The poses are the two curr_pose = pose @ ref_pose_inv (msi_compose_pose_pair_f32).  When they are equal per
 * sample (test path: identity poses) the branch-deciding quadratic of project_ods is evaluated once for both
 * sources; results are identical to two msi_ods_sphere_sweep_* calls. */
int msi_ods_sweep_volume(const float *ref_image, const float *src_image, const float *ref_curr_pose,
                         const float *src_curr_pose, const float *intrinsics, const float *depths, const float *trig,
                         int32_t batch, int32_t height, int32_t width, int32_t num_depths, void *psv, int32_t psv_is_bf16,
                         msi_stream_t stream);
/* out0[b] = lhs0[b] @ rhs[b], out1[b] = lhs1[b] @ rhs[b] (one launch for both curr_pose, msi.py:1125). */
int msi_compose_pose_pair_f32(const float *lhs0, const float *lhs1, const float *rhs, float *out0, float *out1,
                              int32_t batch, msi_stream_t stream);

/* ---- K3: RGBA layer assembly ----------------------------------------------------
 * infer_msi "layer_prediction", which_color_pred = blend_psv (msi.py:130-147):
 * w=(pred[..,d]+1)/2, a=(pred[..,D+d]+1)/2, rgb = w*psv_ref_d + (1-w)*psv_src_d.
 * Writes rgba_native [B,D,H,W,4]; blend_weights / alphas ([B,H,W,D]) may be NULL
 * (the optional extra outputs of msi.py:281-287). */
int msi_assemble_rgba_f32(const float *psv, const float *pred, float *rgba_native,
                          float *blend_weights, float *alphas, int32_t batch, int32_t height,
                          int32_t width, int32_t num_planes, msi_stream_t stream);

/* msi_assemble_rgba_f32 reading the bf16 PSV of the bf16 path (pred, outputs fp32). */
int msi_assemble_rgba_bf16psv_f32(const void *psv_bf16, const float *pred, float *rgba_native,
                                  float *blend_weights, float *alphas, int32_t batch, int32_t height,
                                  int32_t width, int32_t num_planes, msi_stream_t stream);

/* The other colour schemes of infer_msi (FLAGS.which_color_pred, test.py:55-56; msi.py:166-275).  pred holds
 *   MSI_COLOR_BLEND_PSV    [w | alpha]                2D   channels  (= msi_assemble_rgba_f32)
 *   MSI_COLOR_BLEND_BG     [w | alpha | bg rgb]       2D+3           rgb = w psv_ref + (1-w) bg          (msi.py:177-188)
 *   MSI_COLOR_BLEND_BG_PSV [w | alpha | bw | bg rgb]  3D+3           rgb = bw (w psv_ref + (1-w) psv_src) + (1-bw) bg
 *   MSI_COLOR_ALPHA_ONLY   [alpha]                    D              rgb = psv_ref                       (msi.py:258-268)
 * with w, alpha, bw = (x+1)/2 and bg the raw tanh output.  psv [B,H,W,6D] fp32, or bf16 when psv_is_bf16 != 0;
 * blend_weights / alphas / bg_blend_weights [B,H,W,D] may be NULL (msi.py:276-289). */
#define MSI_COLOR_BLEND_PSV 0
#define MSI_COLOR_BLEND_BG 1
#define MSI_COLOR_BLEND_BG_PSV 2
#define MSI_COLOR_ALPHA_ONLY 3
int msi_assemble_rgba_color_f32(const void *psv, int32_t psv_is_bf16, const float *pred, int32_t which_color_pred,
                                float *rgba_native, float *blend_weights, float *alphas, float *bg_blend_weights,
                                int32_t batch, int32_t height, int32_t width, int32_t num_planes, msi_stream_t stream);

/* High-res re-render (test.py:283-394): the per-plane loop there is (a) the high-res sphere
 * sweep (msi_ods_sphere_sweep_f32 at the high resolution), (b) tf.image.resize(BILINEAR,
 * align_corners=True) of the low-res blend weights / alphas (test.py:319-325), (c) the blend of
 * test.py:327-334 and (d) the warp + over-composite of test.py:337-382.  (b) and (c) are: */
int msi_resize_bilinear_f32(const float *in, float *out, int32_t batch, int32_t in_h, int32_t in_w,
                            int32_t channels, int32_t out_h, int32_t out_w, msi_stream_t stream);
/* as msi_assemble_rgba_f32, but `weights_alphas` [B,H,W,2*D] already holds blend weights | alphas
 * in (0,1) (i.e. after the (x+1)/2 of msi.py:132-133). */
int msi_assemble_rgba_scaled_f32(const float *psv, const float *weights_alphas, float *rgba_native,
                                 int32_t batch, int32_t height, int32_t width, int32_t num_planes,
                                 msi_stream_t stream);
/* (a) + (b) + (c) in ONE launch (MSI.hres_layers): the high-res layer stack straight from the two high-res images and the
 * low-res blend weights / alphas, as fp32, in a compact format (see msi_pack_layers), or both.  Neither the [B,Hh,Wh,6D] sweep
 * volume nor the [B,Hh,Wh,2D] upsampled tensor exists: a texel is computed from two image gathers, eight low-res taps and one
 * blend, and stored once.
 *   ref_image, src_image   [B,Hh,Wh,3] preprocessed; ref_curr_pose, src_curr_pose [B,4,4], intrinsics [B,3,3], depths [D] and
 *                          trig (the table of (Hh, Wh) = (height, width)) as msi_ods_sweep_volume takes them
 *   blend_weights, alphas  [B,h,w,D] each ((h, w) = (low_height, low_width)), already in (0,1), 16-byte aligned
 *   rgba_native            [B,D,Hh,Wh,4] fp32, 16-byte aligned, or NULL
 *   layers_out             [B,D,Hh,Wh] texels of `format`, 16-byte aligned, or NULL.  `format` must be MSI_LAYERS_RGBA8 or
 *                          MSI_LAYERS_RGBA16F when layers_out is non-NULL and is ignored when it is NULL.
 * At least one output is non-NULL; with both, one launch writes both.
 * CONTRACT: rgba_native is bit-identical to msi_ods_sweep_volume (fp32) -> msi_resize_bilinear_f32 of [blend_weights | alphas]
 * (concatenated along the channels) -> msi_assemble_rgba_scaled_f32, and layers_out is bit-identical to
 * msi_pack_layers(format) of that stack (the kernel runs the same device functions in the same order; the geometry units are
 * compiled without contraction).
 * Argument checks, in this order: unknown format with a non-NULL layers_out -> MSI_E_BADARG ("unknown format"); both outputs
 * NULL -> MSI_E_BADARG ("null pointer"); any other NULL pointer; non-positive dims (batch < 0) -> MSI_E_BADARG ("bad dims");
 * num_planes % 4 != 0 -> MSI_E_UNSUPPORTED; then the size limits of the kernels it replaces, MSI_E_BADARG: Hh * Wh < 2^24
 * (24-bit pixel offsets), Hh <= 65535 and B <= 65535 (grid dimensions), h * w * D < 2^31.  Error texts name hres_layers.
 * batch = 0 returns MSI_OK without a launch.  Batch rides on the grid (no frame loop): high-res is a batch-1 workload. */
int msi_hres_layers(const float *ref_image, const float *src_image, const float *ref_curr_pose, const float *src_curr_pose,
                    const float *intrinsics, const float *depths, const float *trig, const float *blend_weights,
                    const float *alphas, int32_t batch, int32_t low_height, int32_t low_width, int32_t height, int32_t width,
                    int32_t num_planes, float *rgba_native, void *layers_out, int32_t format, msi_stream_t stream);

/* ---- K4: target-view reprojection + over-composite -------------------------------
 * MSI.msi_render_equirect_view / _depth (msi.py:407-429, 384-405):
 * pj.projective_forward_sphere (projector.py:34-62) = spherical.intersect_sphere
 * (spherical.py:268-326) -> project_spherical (:235-246) -> theta_phi_to_pixels
 * (:54-68) -> sampling.resample per layer, then pj.over_composite
 * (projector.py:246-265) and/or pj.over_composite_depth (:225-244), fused in one
 * pass: neither the pixel coordinates nor the warped layers are materialised,
 * and RGB + depth share the warp.  out_rgb / out_depth may be NULL (not both).
 *   tgt_pose_rt [B,4,4], tgt_pos [B,3], depths [D] (far -> near).
 * status_device (all four render entry points; may be NULL): one int32 in DEVICE memory the kernel ORs
 * MSI_RENDER_STATUS_ORIGIN_OUTSIDE into when a sample's ray origin (pose @ tgt_pos, or the ODS viewing circle) is not
 * strictly inside every sphere it is intersected with.  There spherical.py:316-318 takes the square root of a negative
 * number and the int cast of the NaN pixel coordinate is undefined; the kernel clamps the discriminant (finite pixels,
 * not reference-defined) and reports it here instead of failing silently.  The caller zeroes the word and reads it back
 * when it wants to know (the MSI class checks host-side inputs before the launch and device-side ones through this). */
#define MSI_RENDER_STATUS_ORIGIN_OUTSIDE 1
/* msi_cube_render_views_seamless only: a sample's stack camera is not fx = fy = cx = cy = S/2; it was rendered with the clamp rule. */
#define MSI_RENDER_STATUS_NOT_CUBE_CAMERA 2
int msi_render_equirect_f32(const float *rgba_native, const float *tgt_pose_rt,
                            const float *tgt_pos, const float *depths, const float *trig,
                            int32_t batch, int32_t height, int32_t width, int32_t num_planes,
                            float *out_rgb, float *out_depth, int32_t *status_device, msi_stream_t stream);
/* Many views of one MSI per launch (MSI.render_views; no reference counterpart -- the reference's player was not
 * released): V target cameras per sample, each rendered as msi_render_equirect_f32 renders its one view.
 *   rgba_native [B,D,H,W,4], depths [D] (far -> near), tgt_pose_rt [B*V,4,4], tgt_pos [B*V,3] (view v of sample b at
 *   index b*V + v; it samples stack b only).  The ray direction is rotated by pose[:3,:3], the ray origin is
 *   pose @ (tgt_pos[2], tgt_pos[1], tgt_pos[0], 1) (the x<->z swap of the equirect render).  Rays before the pose:
 *   MSI_CAMERA_EQUIRECT  the lat-long grid of the OUTPUT size: trig = the msi_build_trig_tables_host table of
 *                        (out_height, out_width) (required); intrinsics unused.  At out size == (H, W) every view is
 *                        bit-identical to msi_render_equirect_f32 with that pose.
 *   MSI_CAMERA_PINHOLE   pixel (i, j) -> (1, (i + 0.5 - cy) / fy, (j + 0.5 - cx) / fx): forward +x, image-down +y,
 *                        image-right +z, so with an identity pose the centre pixel looks where the centre of an equirect
 *                        render looks, with the same orientation.  intrinsics [B*V,3,3] row-major in pixels
 *                        (fx, cx in row 0; fy, cy in row 1) (required); trig unused.  out size >= 2 x 2.
 *   out_rgb [B,V,out_height,out_width,3], out_depth [B,V,out_height,out_width] (ONE channel: the composited i / D of
 *   over_composite_depth); either may be NULL, not both.  status_device as above (may be NULL).
 * The grid runs sample -> view -> row: the views of one stack are rendered one after another.
 * Argument checks before any launch, in this order (the one order of every *_render_views entry point; each lists its own
 * instance), MSI_E_BADARG: both outputs NULL; a NULL stack / pose / position / depths; unknown format (msi_render_views_packed);
 * unknown camera; a NULL trig (equirect) / intrinsics (pinhole); batch < 0 or a non-positive height / width / num_planes ("bad
 * dims"); views < 1; an output size below 1 x 1 (2 x 2 pinhole); H * W >= 2^24 (24-bit texel offsets); more than 2^31 - 8
 * workgroups (64 output pixels of a row each).  batch = 0 then returns MSI_OK without a launch. */
#define MSI_CAMERA_EQUIRECT 0
#define MSI_CAMERA_PINHOLE 1
int msi_render_views_f32(const float *rgba_native, const float *tgt_pose_rt, const float *tgt_pos,
                         const float *intrinsics, const float *depths, const float *trig,
                         int32_t batch, int32_t views, int32_t height, int32_t width, int32_t num_planes,
                         int32_t camera, int32_t out_height, int32_t out_width,
                         float *out_rgb, float *out_depth, int32_t *status_device, msi_stream_t stream);

/* Compact layer stacks (MSI.pack_layers / unpack_layers / render_views on a PackedLayers; no reference counterpart beyond
 * test.py:271-276, which stores an MSI as 8-bit colour and alpha PNGs -- the 256 levels of MSI_LAYERS_RGBA8).  The layout
 * is the native one, [B,D,H,W] texels, with a smaller texel:
 *   MSI_LAYERS_F32      16 bytes: four floats (rgba_native itself; not a format of pack / unpack)
 *   MSI_LAYERS_RGBA8     4 bytes: r, g, b, a in this byte order.  fp32 arithmetic, one rounding per operation, no fused
 *                        multiply-add; rint = round half to even:
 *                          encode colour  q = rint((min(max(x, -1), 1) + 1) * 127.5)
 *                          encode alpha   q = rint(min(max(x, 0), 1) * 255)
 *                          decode colour  x = (float(q) - 127.5) * kc,  kc = fl32(1 / 127.5) = 0x1.010102p-7
 *                          decode alpha   x = float(q) * ka,            ka = fl32(1 / 255)   = 0x1.010102p-8
 *                        Codes 0 / 255 decode to exactly -1 / +1 (colour) and 0 / 1 (alpha); decode(255 - q) = -decode(q)
 *                        for colour; both tables increase strictly and encode(decode(q)) = q.  Round-trip error <= half a
 *                        step: 1/255 (colour), 1/510 (alpha).  A NaN input is outside the contract: it does not fault and
 *                        encodes as code 0 (max / min return their other operand).
 *   MSI_LAYERS_RGBA16F   8 bytes: four IEEE halves, r, g, b, a.  Encode = round-to-nearest-even of the fp32 value, no
 *                        clamp; decode is exact.
 * msi_pack_layers / msi_unpack_layers convert `texels` (= B*D*H*W) texels between rgba_native and `packed`; the two buffers
 * must not overlap and are 16-byte aligned.  msi_render_views_packed is msi_render_views_f32 reading a stack of `format`
 * (MSI_LAYERS_F32 forwards to msi_render_views_f32): every tap is decoded by the rule above and composited with the fp32
 * kernel's arithmetic, so the outputs are bit-identical to msi_render_views_f32 on the msi_unpack_layers of the stack.
 * texels = 0 and batch = 0 return MSI_OK without a launch. */
#define MSI_LAYERS_F32 0
#define MSI_LAYERS_RGBA8 1
#define MSI_LAYERS_RGBA16F 2
int msi_pack_layers(const float *rgba_native, int32_t format, void *packed, int64_t texels, msi_stream_t stream);
int msi_unpack_layers(const void *packed, int32_t format, float *rgba_native, int64_t texels, msi_stream_t stream);
int msi_render_views_packed(const void *layers, int32_t format, const float *tgt_pose_rt, const float *tgt_pos,
                            const float *intrinsics, const float *depths, const float *trig,
                            int32_t batch, int32_t views, int32_t height, int32_t width, int32_t num_planes,
                            int32_t camera, int32_t out_height, int32_t out_width,
                            float *out_rgb, float *out_depth, int32_t *status_device, msi_stream_t stream);
/* The ODS stereo camera of the viewer (MSI.render_views(camera='ods'), MSI.render_ods_pair; no reference counterpart): V ODS
 * views of each MSI per launch -- both eyes of a stereo 360 frame are V = 2 -- from a stack of any `format` (MSI_LAYERS_*),
 * at any output size, rgb and one-channel depth.  It is the MSI_CAMERA_EQUIRECT camera of msi_render_views_f32 with the ray
 * origin moved onto the viewing circle (it is an entry point of its own, not a camera code: the codes of the three
 * *_render_views functions stay 0 and 1).  Pixel (i, j) of the lat-long grid of the OUTPUT size, before the pose:
 *     direction  r = (cos S_j cos T_i, sin T_i, sin S_j cos T_i)                               -- the equirect camera's
 *     origin     c = (tgt_pos[2] + sin S_j * e, tgt_pos[1], tgt_pos[0] + (-cos S_j) * e)       -- e = eye_radius[b*V + v]
 *   then r <- pose[:3,:3] r, c <- pose (c, 1) and the per-layer arithmetic of msi_render_views_f32, op for op.
 *   (sin S, 0, -cos S) . r = 0: the ray is tangent to the circle of radius |e| around the head position.  e is SIGNED:
 *   e = +baseline is the left eye (the reference's order = +1, its ref image), e = -baseline the right eye (the src image).
 *   layers [B,D,H,W] texels of `format`, depths [D] (far -> near), tgt_pose_rt [B*V,4,4], tgt_pos [B*V,3], eye_radius [B*V]
 *   (view v of sample b at index b*V + v), trig = the msi_build_trig_tables_host table of (out_height, out_width);
 *   out_rgb [B,V,out_height,out_width,3], out_depth [B,V,out_height,out_width]; either may be NULL, not both.
 * Three facts fix the convention (tests/test_ods_views_cpu.py holds the composed CPU reference to them, the GPU tests the kernel):
 *   1. e = 0 is the equirect camera: the outputs are bit-identical to msi_render_views_f32 / msi_render_views_packed with
 *      MSI_CAMERA_EQUIRECT for the same poses, positions and size.
 *   2. Output column j is column W-1-j of msi_render_ods_f32 (which keeps the reference's order, mirrored against its inputs):
 *      at the stack's size with tgt_pos = 0, e = order * intrinsics[b,0,0] and the same pose the two agree to rounding (the
 *      trig table is not exactly symmetric, so not bit for bit).
 *   3. It is upright and the eye sign is the sweep's: an image swept with msi_ods_sphere_sweep_f32 (order, one depth) and
 *      rendered back as a single opaque layer with e = order * baseline reproduces the image unflipped; e = -order * baseline
 *      does not.
 * status_device (may be NULL): the origin differs from pixel to pixel here, so MSI_RENDER_STATUS_ORIGIN_OUTSIDE is set when ANY
 * rendered pixel's origin is not strictly inside every sphere it is intersected with, or is NaN -- also when only a part of
 * the circle leaves the innermost sphere (every lane tests its own origin; one atomic OR per wavefront).  Pixels stay finite
 * (clamped discriminant), as in the other renders.
 * Argument checks before any launch, in this order, MSI_E_BADARG: both outputs NULL; a NULL input (every pointer but the outputs
 * and status_device is required); unknown format; bad dims; views < 1; an output size below 1 x 1; H * W >= 2^24; the grid limit
 * of msi_render_views_f32.  batch = 0 then returns MSI_OK without a launch. */
int msi_render_ods_views(const void *layers, int32_t format, const float *tgt_pose_rt, const float *tgt_pos,
                         const float *eye_radius, const float *depths, const float *trig,
                         int32_t batch, int32_t views, int32_t height, int32_t width, int32_t num_planes,
                         int32_t out_height, int32_t out_width,
                         float *out_rgb, float *out_depth, int32_t *status_device, msi_stream_t stream);
/* Sparse layer stacks (MSI.sparsify_layers / densify_layers / render_views on a SparseLayers; no reference counterpart): a packed
 * stack (MSI_LAYERS_RGBA8 or MSI_LAYERS_RGBA16F; fp32 pools are not built) that stores only the tiles a sphere render can see.
 * matryodshka_amd/sparse.py holds the same rule in numpy (sparsify_np / expand_np); the kernels are tested against it bit for bit.
 *   tile         4 rows x 16 columns of texels; H % 4 == 0 and W % 16 == 0, otherwise MSI_E_UNSUPPORTED.
 *   empty texel  its alpha DECODES to zero: code 0 (rgba8), +0 or -0 (rgba16f).
 *   keep         tile (ty, tx) of layer d of sample b is kept iff d == 0 (the composite takes layer 0's colour whatever its alpha)
 *                or any texel within Chebyshev distance 1 of the tile -- its 6 x 18 window, x modulo W and y modulo H, as the
 *                bilinear taps of the sphere renders wrap -- is not empty.  Consequence: a bilinear footprint with ANY of its
 *                four taps in a dropped tile has four zero alphas, so the layer contributes nothing to that pixel.
 *   table        int32 [B,D,H/4,W/16]: the tile's index among the kept tiles of its own layer, in row-major tile order, or -1
 *   layer_start  int64 [B*D+1]: exclusive prefix sum of the kept tiles per layer; layer_start[B*D] = T
 *   pool         [T][4][16] texels; tile k of layer (b, d) is pool[layer_start[b*D+d] + k].  16-byte aligned.
 * msi_sparse_index_tiles applies the rule to a dense packed stack: it writes the final table and counts_out [B*D], the kept tiles per
 * layer (two launches; no atomic decides an index: the result is the same bytes every time).  The prefix sum of the counts and the
 * allocation of the pool are the caller's.  msi_sparse_gather_tiles copies the kept tiles into pool_out; msi_sparse_expand writes
 * the dense stack back, all-zero bytes in dropped tiles.  table, layer_start and the pool must belong together (the entry points
 * trust them: they address the pool through them).
 * msi_render_views_sparse is msi_render_views_packed (eye_radius == NULL; camera = MSI_CAMERA_EQUIRECT or MSI_CAMERA_PINHOLE) and
 * msi_render_ods_views (eye_radius [B*V] non-NULL with MSI_CAMERA_EQUIRECT: the same origin formula, the same per-lane status
 * vote) reading a sparse stack: per layer a lane looks its tap tiles up in the table; with all four present it loads and blends
 * exactly as the dense kernels do, otherwise the layer's step is skipped (and when no lane of a wavefront has a present
 * footprint the texel loads are not issued).  CONTRACT: colours are finite in texels whose alpha is zero (always true for rgba8;
 * an rgba16f inf / NaN colour under a zero alpha is outside it: the dense render turns it into NaN, this one skips it).  Then
 * every output element compares == to msi_render_views_packed / msi_render_ods_views on the original dense stack and on
 * msi_sparse_expand's output: the same bits, except that a zero may differ in sign (a skipped step does not add c * 0).  The
 * status word is the dense kernels' (qc_max sees every layer).
 * Argument checks before any HIP call, in this order, MSI_E_BADARG unless noted.  Tile entry points: a NULL pointer; unknown
 * format (MSI_LAYERS_F32 included); non-positive dims (batch < 0); H % 4 or W % 16 -> MSI_E_UNSUPPORTED; H * W >= 2^24.
 * msi_render_views_sparse: both outputs NULL; a NULL pool / table / layer_start / pose / position / depths; unknown format;
 * unknown camera; a NULL trig (equirect) / intrinsics (pinhole); eye_radius with the pinhole camera; bad dims; the tile
 * divisibility -> MSI_E_UNSUPPORTED; views < 1; output size below 1 x 1 (2 x 2 pinhole); H * W >= 2^24; the grid limit of the
 * other views renders.  batch = 0 returns MSI_OK after validation, without a launch. */
int msi_sparse_index_tiles(const void *layers, int32_t format, int32_t batch, int32_t num_planes, int32_t height, int32_t width,
                           int32_t *table_out, int32_t *counts_out, msi_stream_t stream);
int msi_sparse_gather_tiles(const void *layers, int32_t format, const int32_t *table, const int64_t *layer_start, int32_t batch,
                            int32_t num_planes, int32_t height, int32_t width, void *pool_out, msi_stream_t stream);
int msi_sparse_expand(const void *pool, const int32_t *table, const int64_t *layer_start, int32_t format, int32_t batch,
                      int32_t num_planes, int32_t height, int32_t width, void *layers_out, msi_stream_t stream);
int msi_render_views_sparse(const void *pool, const int32_t *table, const int64_t *layer_start, int32_t format,
                            const float *tgt_pose_rt, const float *tgt_pos, const float *intrinsics, const float *eye_radius,
                            const float *depths, const float *trig, int32_t batch, int32_t views, int32_t height, int32_t width,
                            int32_t num_planes, int32_t camera, int32_t out_height, int32_t out_width, float *out_rgb,
                            float *out_depth, int32_t *status_device, msi_stream_t stream);
/* Sparse stacks for surfaces that do not wrap (MSI.sparsify_layers(border='edge'); MSI.mpi_render_views / cube_render_views on a
 * SparseLayers): the planar render zero-pads -- a tap outside [0,W) x [0,H) is masked to zero -- and the cube render clamps to the
 * edge of the chosen face; neither ever reads the opposite border.  So the EDGE keep rule is the rule above with the tile's 6 x 18
 * window CLIPPED to the image instead of wrapped: tile (ty, tx) of layer d is kept iff d == 0 or some texel of the clipped window is
 * not empty.  Then a footprint with any in-range tap in a dropped tile has all in-range alphas zero.  Tile, "empty", table,
 * layer_start, pool and layer 0 kept whole are unchanged; the kept set is a subset of the wrap rule's.  A stack records the rule
 * it was made with: the sphere renders are correct on wrap-rule stacks only, these two read edge-rule stacks (the Python layer
 * refuses a mismatch; the C entry points trust their caller).
 *   msi_sparse_index_tiles_edge   msi_sparse_index_tiles with the edge rule: the same arguments, checks, launches and outputs.
 *                                 msi_sparse_gather_tiles and msi_sparse_expand do not depend on the rule.
 *   msi_mpi_render_views_sparse   msi_mpi_render_views with (pool, table, layer_start, format) in place of the stack.  Per layer a
 *                                 lane looks up the tiles of its IN-RANGE taps only (a masked tap is never absent; its value is zero);
 *                                 a pixel that samples outside (-1, W) x (-1, H) is present with every tap masked.
 *   msi_cube_render_views_sparse  msi_cube_render_views likewise; table [6B,D,S/4,S/16].  S % 16 == 0 is required
 *                                 (MSI_E_UNSUPPORTED).  Clamped taps never leave the face: all four are looked up.  The status word
 *                                 is msi_cube_render_views'.  A sample's six DENSE face stacks must stay below 2^31 bytes, as there
 *                                 (they bound its kept tiles, which one descriptor addresses).
 * Both follow msi_render_views_sparse's contract: with every tap tile present a lane loads and blends exactly as the dense kernel
 * does, otherwise the layer's step is skipped (and when no lane of a wavefront is present the texel loads are not issued); with
 * finite colours under zero alphas every output element compares == to msi_mpi_render_views / msi_cube_render_views on the dense
 * packed stack and on msi_sparse_expand's output (a zero may differ in sign).
 * Argument checks before any HIP call, in this order, MSI_E_BADARG unless noted.  msi_sparse_index_tiles_edge: the tile entry
 * points'.  msi_mpi_render_views_sparse: both outputs NULL; a NULL input; unknown format (MSI_LAYERS_F32 included); bad dims; more
 * than 128 planes, then H % 4 or W % 16 -> MSI_E_UNSUPPORTED; views < 1; output size below 1 x 1; H * W >= 2^24; the grid limit.
 * msi_cube_render_views_sparse: both outputs NULL; a NULL pool / table / layer_start / pose / position / stack_intrinsics / depths;
 * unknown format; unknown camera; a NULL trig (equirect) / tgt_intrinsics (pinhole); bad dims; more than 128 planes, then S % 16 ->
 * MSI_E_UNSUPPORTED; views < 1; output size below 1 x 1 (2 x 2 pinhole); the 2^31-byte limit; the grid limit.  batch = 0 returns
 * MSI_OK after validation, without a launch. */
int msi_sparse_index_tiles_edge(const void *layers, int32_t format, int32_t batch, int32_t num_planes, int32_t height, int32_t width,
                                int32_t *table_out, int32_t *counts_out, msi_stream_t stream);
int msi_mpi_render_views_sparse(const void *pool, const int32_t *table, const int64_t *layer_start, int32_t format,
                                const float *tgt_pose, const float *intrinsics, const float *tgt_intrinsics_inv, const float *depths,
                                int32_t batch, int32_t views, int32_t height, int32_t width, int32_t num_planes,
                                int32_t out_height, int32_t out_width, float *out_rgb, float *out_depth, msi_stream_t stream);
int msi_cube_render_views_sparse(const void *pool, const int32_t *table, const int64_t *layer_start, int32_t format,
                                 const float *tgt_pose_rt, const float *tgt_pos, const float *tgt_intrinsics,
                                 const float *stack_intrinsics, const float *depths, const float *trig,
                                 int32_t batch, int32_t views, int32_t face_size, int32_t num_planes, int32_t camera,
                                 int32_t out_height, int32_t out_width, float *out_rgb, float *out_depth, int32_t *status_device,
                                 msi_stream_t stream);
/* The high-res stack of msi_hres_layers built sparse (MSI.hres_layers_sparse): the dense stack is never written.
 * RULE: msi_hres_layers stores a texel's alpha as the align-corners bilinear resize of the low-res alphas, encoded; it does not
 * depend on the images.  So the keep rule above is applied to the alphas the dense stack WOULD hold -- the same resize
 * expression and the same encoder, in the geometry units compiled without contraction -- and the table is known before any texel
 * is computed: a NaN, a negative, a > 1, a too-small (rgba8: rounds to code 0; rgba16f: underflows to +-0) or a -0.0 alpha
 * lands on the side the stored code would put it.
 *   msi_hres_index_tiles    alphas [B,h,w,D] -> table_out [B,D,Hh/4,Wh/16] (final: index or -1) and counts_out [B*D], equal to
 *                           msi_sparse_index_tiles of msi_hres_layers' codes of `format` (two launches, the second is
 *                           msi_sparse_index_tiles' scan).  The prefix sum and the allocation of the pool are the caller's.
 *   msi_hres_layers_sparse  msi_hres_layers' inputs, the table and layer_start -> pool_out: every texel of every kept tile,
 *                           the empty ones too, with the bits of the dense stack (the one texel definition both kernels
 *                           call); for a dropped tile no sample position is computed, no image memory is read and nothing is
 *                           stored.  The result equals msi_sparse_gather_tiles of msi_hres_layers' stack.  One launch.  The
 *                           pool's bytes decide between plain and non-temporal stores, as msi_hres_layers decides for its
 *                           stack: where the DENSE stack would exceed 256 MiB (a smaller one bounds the pool), one 8-byte read
 *                           of layer_start[B*D] and a wait for `stream` come first.  Pool offsets are 64-bit.
 * Argument checks before any HIP call, in this order: msi_hres_layers' (a NULL pointer -> MSI_E_BADARG, bad dims,
 * num_planes % 4 -> MSI_E_UNSUPPORTED, Hh * Wh >= 2^24 / Hh or B > 65535, h * w * D >= 2^31), then the tile entry points'
 * (unknown format, MSI_LAYERS_F32 included -> MSI_E_BADARG; Hh % 4 or Wh % 16 -> MSI_E_UNSUPPORTED).  Error texts name
 * hres_index_tiles / hres_layers_sparse.  batch = 0 returns MSI_OK after validation.  table, layer_start and the pool must
 * belong together; msi_hres_layers_sparse refuses a layer_start that ends beyond the table's tiles. */
int msi_hres_index_tiles(const float *alphas, int32_t format, int32_t batch, int32_t low_height, int32_t low_width,
                         int32_t height, int32_t width, int32_t num_planes,
                         int32_t *table_out, int32_t *counts_out, msi_stream_t stream);
int msi_hres_layers_sparse(const float *ref_image, const float *src_image, const float *ref_curr_pose, const float *src_curr_pose,
                           const float *intrinsics, const float *depths, const float *trig, const float *blend_weights,
                           const float *alphas, int32_t batch, int32_t low_height, int32_t low_width, int32_t height, int32_t width,
                           int32_t num_planes, const int32_t *table, const int64_t *layer_start, void *pool_out, int32_t format,
                           msi_stream_t stream);
/* Views straight from the FACTORS of a high-res stack (MSI.hres_factors -> FactoredLayers -> MSI.render_views / render_ods_pair): the stack
 * msi_hres_layers would build is never allocated; every tap of a render evaluates that stack's texel from msi_hres_layers' own inputs.
 * Arguments: msi_hres_layers' inputs and sizes in its order (trig: the table of the STACK size, height x width), then the view arguments
 * of msi_render_views_sparse: tgt_pose_rt [B*V][4][4], tgt_pos [B*V][3], view_intrinsics [B*V][3][3] (pinhole) or NULL, eye_radius
 * [B*V] (the ODS camera; with MSI_CAMERA_EQUIRECT only) or NULL, view_trig (the table of the OUTPUT size; equirect and ODS) or NULL,
 * views, camera, the output size, out_rgb [B,V,h,w,3] / out_depth [B,V,h,w] (either may be NULL), the status word.
 * Every output element compares == to msi_render_views_f32 (eye_radius == NULL) / msi_render_ods_views (non-NULL) on the fp32 stack
 * msi_hres_layers writes from the same arguments: the same bits, except that a zero may differ in sign -- where no lane of a
 * wavefront sees a layer (blended alpha == 0, layer 0 excepted) its colour is not computed and the step adds nothing (CONTRACT as
 * for the sparse viewer: image values are finite).  The status word is the dense kernels'.
 * Argument checks before any HIP call, in this order, MSI_E_BADARG unless noted.  msi_hres_layers': a NULL input of the stack; bad
 * dims; num_planes % 4 -> MSI_E_UNSUPPORTED; H * W >= 2^24 (H, B > 65535); h * w * D >= 2^31.  Then the views': both outputs NULL; a
 * NULL pose / position; unknown camera; a NULL view_trig (equirect) / view_intrinsics (pinhole); eye_radius with the pinhole camera;
 * views < 1; output size below 1 x 1 (2 x 2 pinhole); the grid limit of the other views renders.  batch = 0 returns MSI_OK after
 * validation, without a launch. */
int msi_render_views_factored(const float *ref_image, const float *src_image, const float *ref_curr_pose, const float *src_curr_pose,
                              const float *intrinsics, const float *depths, const float *trig, const float *blend_weights,
                              const float *alphas, int32_t batch, int32_t low_height, int32_t low_width, int32_t height, int32_t width,
                              int32_t num_planes, const float *tgt_pose_rt, const float *tgt_pos, const float *view_intrinsics,
                              const float *eye_radius, const float *view_trig, int32_t views, int32_t camera, int32_t out_height,
                              int32_t out_width, float *out_rgb, float *out_depth, int32_t *status_device, msi_stream_t stream);
/* Mip-mapped layer stacks (MSI.build_mips -> MipLayers -> MSI.render_views / render_ods_pair with lod_bias; no reference counterpart):
 * the viewers above take four bilinear taps at the stack's own resolution, which aliases wherever an output pixel covers more than
 * one texel (a thumbnail of a large stack, a wide field of view, the poles, the far side of a translated viewpoint).  A stack gets
 * the levels of a pyramid, and the view kernel blends the two levels that bracket each pixel's footprint (trilinear filtering).
 * matryodshka_amd/mips.py holds the pyramid rule in numpy (build_mips_np; the kernel is tested against it bit for bit) and
 * tests/mip_reference.py the view rule in fp64.
 *
 * msi_build_mips: layers [B,D,H,W] texels of `format` (any MSI_LAYERS_*), levels = L in 1 .. MSI_MIP_MAX_LEVELS, H and W multiples
 * of 2^(L-1), the top level (H >> (L-1)) x (W >> (L-1)) at least 2 x 2.  mips_out holds the levels 1 .. L-1, consecutive, level l
 * [B,D,H>>l,W>>l] texels of the same format, 16-byte aligned (about a third of the base's bytes); level 0 is the base, untouched.
 * One launch: the base is read once, a workgroup reduces 32 x 32 base texels of one (sample, layer) through every level.
 *   THE PYRAMID RULE (fp32, one rounding per operation, no fused multiply-add), on DECODED texels (a, c_0..c_2) = (alpha, colour):
 *     level 1   texel (y, x) owns the base block rows 2y, 2y+1 x columns 2x, 2x+1 = tl, tr, bl, br.  Its partial sums are
 *                 A = sum a,   P_k = sum fl(a * c_k),   Q_k = sum c_k,   each summed as (tl + tr) + (bl + br).
 *     level l   the partials of texel (y, x) are the sums of the four partials of level l-1 at (2y, 2y+1) x (2x, 2x+1), in the
 *               same order.  Partials are never quantised: only the texel that is stored is.
 *     texel     with n = 4^l:  alpha = A * (1/n);  colour_k = P_k / A (IEEE divide) where the layer d != 0 and A > 0, else
 *               colour_k = Q_k * (1/n).  Layer 0 always takes the plain mean: over-compositing ignores its alpha.
 *     store     encoded with the format's encoder above (rgba8 / rgba16f); MSI_LAYERS_F32 stores the four floats.
 *   A transparent texel's colour therefore never bleeds into a coarser level.
 * Argument checks before any HIP call, in this order, MSI_E_BADARG: a NULL layers (a NULL mips_out with L > 1); unknown format;
 * non-positive dims (batch < 0); L outside 1 .. MSI_MIP_MAX_LEVELS; H or W not a multiple of 2^(L-1); a top level below 2 x 2;
 * 2^31 or more workgroups.  batch = 0 and L = 1 (nothing to write) return MSI_OK without a launch.
 *
 * msi_render_views_mip: msi_render_views_packed's arguments with, after `format`, mips (msi_build_mips' buffer for the same
 * sizes and format; may be NULL when levels = 1), levels, lod_bias, and -- as in msi_render_views_sparse -- eye_radius [B*V] after
 * intrinsics: non-NULL (with MSI_CAMERA_EQUIRECT only) selects the ODS camera of msi_render_ods_views.  Cameras, pose, ray / sphere
 * quadratic, pixel coordinates, over-composite, segment combine, outputs and the status word are those renders', op for op; only the
 * blended texel (r, g, b, alpha) of a layer changes:
 *   THE TEXEL RULE.  (u, v) is the layer's hit of pixel (i, j), in pixel coordinates of the H x W base.  (u_x, v_x) is the hit
 *   of the column neighbour (i, j'), j' = j + 1 if j + 1 < out_width else j - 1; (u_y, v_y) that of the row neighbour (i', j), i'
 *   chosen the same way.  A neighbour is the WHOLE ray of that pixel (for the ODS camera its origin moves too).  An axis of one
 *   pixel has no neighbour: its differences are 0.
 *     du_x = u_x - u, du_x -= W * rint(du_x / W)   (u wraps: the nearer way round);   dv_x = v_x - v   (v does not wrap);  same for y
 *     rho    = max(hypot(du_x, dv_x), hypot(du_y, dv_y))                  texels per output pixel, isotropic
 *     lambda = min(max(log2(rho) + lod_bias, 0), L - 1);  rho = 0 or a NaN gives 0
 *     l0 = floor(lambda),  f = lambda - l0,  l1 = min(l0 + 1, L - 1)
 *     at level l the hit is  u_l = (u + 0.5) * 2^-l - 0.5,  v_l = (v + 0.5) * 2^-l - 0.5   (l = 0: u and v themselves)
 *     t_l    = the viewers' wrap-around bilinear lookup (four taps, both axes wrap, weights from the unwrapped corners, summed
 *              a, b, c, d) of level l at (u_l, v_l) with the level's size (W >> l, H >> l)
 *     texel  = t_l0 + f * (t_l1 - t_l0) per component  (f = 0: t_l0 itself; level l1 is then not read)
 *   The kernel evaluates log2, the reciprocal of W and the hits with the continuous-tail primitives of the other renders (1 ulp);
 *   nothing here branches on them discontinuously: the rule is continuous in the ray.
 *   Properties: a pixel with lambda = 0 on every layer has the bits of msi_render_views_packed / msi_render_ods_views; so has the
 *   whole image when levels = 1 or lod_bias <= -64.  lod_bias >= 64 reads the top level alone.
 *   The footprint is isotropic: near the stack's poles, where du_x is large while dv_x is small, lambda follows du_x and the image
 *   is blurred along v as well (msi_render_views_aniso below filters along the footprint's major axis instead).
 * Argument checks before any HIP call, in this order, MSI_E_BADARG: both outputs NULL; a NULL layers / pose / position / depths
 * (a NULL mips with L > 1); unknown format; unknown camera; a NULL trig (equirect) / intrinsics (pinhole); eye_radius with the
 * pinhole camera; bad dims; a NaN lod_bias; L outside 1 .. MSI_MIP_MAX_LEVELS; H or W not a multiple of 2^(L-1); a top level below
 * 2 x 2; views < 1; output size below 1 x 1 (2 x 2 pinhole); H * W >= 2^24; the grid limit of the other views renders.  batch = 0
 * returns MSI_OK after validation, without a launch.
 *
 * msi_render_views_aniso (MSI.render_views / render_ods_pair with max_anisotropy > 1): msi_render_views_mip's arguments with
 * max_anisotropy = A in [1, MSI_ANISO_MAX] after lod_bias.  An equirect stack's texel rows near a pole span the whole circle: a view
 * that does not share the stack's poles (an eye looking up or down, a tilted head, a translated viewpoint) has footprints there that
 * are many texels long and about one wide, which the isotropic rule above answers with a coarse level, smeared both ways.  Here the
 * level follows the MINOR axis of the footprint and several trilinear samples are taken along the MAJOR axis.  Everything but the
 * blended texel of a layer is msi_render_views_mip's, op for op; tests/aniso_reference.py holds the rule in fp64.
 *   THE ANISOTROPIC TEXEL RULE.  (u, v), the two neighbours (their choice at the image border included) and du_x, dv_x, du_y, dv_y
 *   as in THE TEXEL RULE above (du wrapped the nearer way round, dv not wrapped).  Per layer, in this fp32 operation order (one
 *   rounding per operation, no fused multiply-add; sqrt, the quotients marked /~, the reciprocal square root and log2 are the
 *   1-ulp continuous-tail primitives of the other renders):
 *     E = du_x du_x + du_y du_y,   G = dv_x dv_x + dv_y dv_y,   Fm = du_x dv_x + du_y dv_y        (J J^T of the 2 x 2 footprint Jacobian)
 *     h = 0.5 (E - G),   R = sqrt(h h + Fm Fm)
 *     s_max = sqrt(0.5 (E + G) + R)                  texels per pixel along the major axis of the footprint ellipse
 *     s_min = |du_x dv_y - du_y dv_x| /~ s_max       ... along the minor axis
 *     ratio = 1 unless s_max > 1 (so also for s_max = 0 or a NaN), else min(max(s_max /~ max(s_min, 1), 1), A)
 *             (the inner max(., 1) only absorbs the rounding of the quotients: the exact value is >= 1 already)
 *     step  = s_max /~ ratio                         base texels between samples
 *     lambda = min(max(log2(step) + lod_bias, 0), L - 1);  step = 0 or a NaN gives 0;   l0, f, l1 as above
 *     axis  (a_u, a_v) = (h + R, Fm) if h >= 0 else (Fm, R - h);  n2 = a_u a_u + a_v a_v;
 *           (mu_u, mu_v) = (a_u, a_v) * rsqrt(n2) if n2 > 0 else (1, 0)        unit major axis, texel space
 *     s_u = step * mu_u,  s_v = step * mu_v
 *     M = ceil(0.5 (ratio - 1));   samples m = -M .. M at (u + m s_u, v + m s_v); for m != 0 each coordinate is then wrapped by whole
 *           sizes, u -= W floor((u + 0.5) (1 / W)), v -= H floor((v + 0.5) (1 / H)), the sample of m = 0 is the hit itself
 *     w_m = min(max(0.5 ratio - (|m| - 0.5), 0), 1) * (1 / ratio)   (IEEE reciprocal)   a box of length `ratio` cut into unit cells
 *           around the samples: the cells of |m| < M are whole, the outermost two are what is left; sum of w_m = 1
 *     t_m = the trilinear texel of THE TEXEL RULE at sample m (per-level hit transform, wrap-around bilinear lookup, lerp by f)
 *     texel = w_0 t_0, then + w_1 t_1, + w_1 t_-1, + w_2 t_2, + w_2 t_-2, ..  in this order, per component
 *   Properties: the outermost weights go to 0 exactly where M changes (ratio = 2M + 1), the axis only matters where ratio > 1 and
 *   its sign not at all (the samples are symmetric), so nothing is discontinuous in the ray.  ratio = 1 gives ONE trilinear sample
 *   with weight 1 -- its own bits -- whose lambda comes from s_max: that is not rho of THE TEXEL RULE (the longer COLUMN of the
 *   Jacobian, where s_max is its larger singular value), so A = 1 is not bit-identical to msi_render_views_mip (MSI.render_views
 *   calls that entry point for max_anisotropy = 1).  A pixel with s_max <= 1 on every layer has the bits of the plain render
 *   (msi_render_views_packed / msi_render_ods_views), and lod_bias <= -64 is the plain render bit for bit: that shortcut alone
 *   skips the filter.  A stack of one level (mips NULL) is still filtered along the major axis at level 0 -- a view magnified in
 *   v and minified in u.  At most 2 ceil((A - 1) / 2) + 1 samples per layer: 17 at A = 16.  The samples wrap on BOTH axes, as the
 *   viewers' lookup does: a sample that leaves the stack over a pole comes back in at the opposite pole (near a pole the major
 *   axis runs along u, where wrapping is the geometry; the wrap in v is the lookup's, not the sphere's).
 * Argument checks: msi_render_views_mip's, in its order, with one more after the NaN lod_bias: max_anisotropy NaN or outside
 * [1, MSI_ANISO_MAX].  batch = 0 returns MSI_OK after validation, without a launch. */
#define MSI_MIP_MAX_LEVELS 6
#define MSI_ANISO_MAX 16
int msi_build_mips(const void *layers, int32_t format, int32_t batch, int32_t num_planes, int32_t height, int32_t width,
                   int32_t levels, void *mips_out, msi_stream_t stream);
int msi_render_views_mip(const void *layers, int32_t format, const void *mips, int32_t levels, float lod_bias,
                         const float *tgt_pose_rt, const float *tgt_pos, const float *intrinsics, const float *eye_radius,
                         const float *depths, const float *trig, int32_t batch, int32_t views, int32_t height, int32_t width,
                         int32_t num_planes, int32_t camera, int32_t out_height, int32_t out_width, float *out_rgb,
                         float *out_depth, int32_t *status_device, msi_stream_t stream);
int msi_render_views_aniso(const void *layers, int32_t format, const void *mips, int32_t levels, float lod_bias,
                           float max_anisotropy, const float *tgt_pose_rt, const float *tgt_pos, const float *intrinsics,
                           const float *eye_radius, const float *depths, const float *trig, int32_t batch, int32_t views,
                           int32_t height, int32_t width, int32_t num_planes, int32_t camera, int32_t out_height,
                           int32_t out_width, float *out_rgb, float *out_depth, int32_t *status_device, msi_stream_t stream);
/* MSI.msi_render_equirect_view_single (msi.py:431-452): the warped, un-composited
 * layers, out_layers [D,B,H,W,4]. */
int msi_project_layers_f32(const float *rgba_native, const float *tgt_pose_rt,
                           const float *tgt_pos, const float *depths, const float *trig,
                           int32_t batch, int32_t height, int32_t width, int32_t num_planes,
                           float *out_layers, int32_t *status_device, msi_stream_t stream);

/* MSI.msi_render_ods_view (msi.py:502-525): pj.projective_forward_ods (projector.py:100-127) =
 * spherical.intersect_ods (spherical.py:328-365; eye rays tangent to the viewing circle of radius
 * intrinsics[b,0,0], order +1 left / -1 right, transformed by pose [B,4,4]) -> resample ->
 * over_composite.  out_rgb [B,H,W,3]. */
int msi_render_ods_f32(const float *rgba_native, const float *pose, const float *intrinsics,
                       const float *depths, const float *trig, int32_t batch, int32_t height,
                       int32_t width, int32_t num_planes, int32_t order, float *out_rgb,
                       int32_t *status_device, msi_stream_t stream);
/* MSI.msi_render_perspective_view (msi.py:475-500): pj.projective_forward_sphere_to_perspective
 * (projector.py:64-98) = spherical.intersect_perspective (spherical.py:367-401; hard-coded
 * 0.1/0.05 intrinsics) -> resample -> over_composite.  `pose` [B,4,4] is the crop rotation the
 * caller builds from viewing_window (projector.py:78-86); out_rgb [B,tgt_height,tgt_width,3]. */
int msi_render_perspective_f32(const float *rgba_native, const float *pose, const float *tgt_pos,
                               const float *depths, int32_t batch, int32_t height, int32_t width,
                               int32_t num_planes, int32_t tgt_height, int32_t tgt_width, float *out_rgb,
                               int32_t *status_device, msi_stream_t stream);

/* ---- PP (perspective cube-face) path, BASELINE configs[4] ------------------------------------
 * pj.perspective_plane_sweep (projector.py:221-223): sweep_one with spherical.uv_grid (:46-48),
 * backproject_planar (:131-149), apply_pose (projector.py:275-291), project_perspective
 * (spherical.py:248-266) and the wrap-around sampler.  intrinsics [B,3,3] = fx,cx / fy,cy. */
int msi_perspective_plane_sweep_f32(const float *image, const float *pose, const float *intrinsics,
                                    const float *depths, int32_t batch, int32_t height, int32_t width,
                                    int32_t num_depths, float *psv, int32_t psv_channels,
                                    int32_t channel_offset, msi_stream_t stream);
/* The whole bf16 double volume of MSI.format_network_input for input_type PP (msi.py:1157-1161) in one launch:
 * pj.perspective_plane_sweep (projector.py:221-223) of ref_image into channels [0,3D) and of src_image into [3D,6D) of
 * psv_bf16 [B,H,W,6D].  The poses are the two curr_pose = pose @ ref_pose_inv (msi_compose_pose_pair_f32).  Every value
 * is the round to nearest even of what two msi_perspective_plane_sweep_f32 calls compute, bit for bit. */
int msi_perspective_sweep_volume_bf16(const float *ref_image, const float *src_image, const float *ref_curr_pose,
                                      const float *src_curr_pose, const float *intrinsics, const float *depths,
                                      int32_t batch, int32_t height, int32_t width, int32_t num_depths,
                                      void *psv_bf16, msi_stream_t stream);
/* The high-res layer stack of the PP path in ONE launch (MSI.mpi_hres_layers): msi_hres_layers for perspective images.  Two
 * msi_perspective_plane_sweep_f32 of the high-res images (ref = foreground, src = background; poses as
 * msi_perspective_sweep_volume_bf16, intrinsics [B,3,3] those of the HIGH-RES images), msi_resize_bilinear_f32 of the low-res
 * blend_weights / alphas [B,h,w,D] and msi_assemble_rgba_scaled_f32, without the [B,Hh,Wh,6D] volume or the upsampled tensor:
 * rgba_native [B,D,Hh,Wh,4] has the bits of those launches, layers_out those of msi_pack_layers of it.  Parameters, outputs
 * (either may be NULL, not both), formats, store policy and checks are msi_hres_layers' without `trig`; in addition Hh > 1,
 * Wh > 1 and Hh * Wh * 12 < 2^31 (MSI_E_BADARG), the sweep's own.  Error texts name pp_hres_layers.  batch = 0 returns MSI_OK
 * after validation. */
int msi_pp_hres_layers(const float *ref_image, const float *src_image, const float *ref_curr_pose, const float *src_curr_pose,
                       const float *intrinsics, const float *depths, const float *blend_weights, const float *alphas, int32_t batch,
                       int32_t low_height, int32_t low_width, int32_t height, int32_t width, int32_t num_planes, float *rgba_native,
                       void *layers_out, int32_t format, msi_stream_t stream);
/* msi_pp_hres_layers' packed stack built sparse for the viewers that never read the opposite border (MSI.mpi_hres_layers_sparse;
 * msi_mpi_render_views_sparse, msi_cube_render_views_sparse), as msi_hres_index_tiles / msi_hres_layers_sparse build the sphere's:
 *   msi_hres_index_tiles_edge  msi_hres_index_tiles with msi_sparse_index_tiles_edge's keep rule (a tile's 6 x 18 window clipped
 *                              to the image): equal to msi_sparse_index_tiles_edge of msi_pp_hres_layers' codes of `format`.
 *   msi_pp_hres_layers_sparse  msi_hres_layers_sparse without `trig`, with msi_pp_hres_layers' texel: equal to
 *                              msi_sparse_gather_tiles of msi_pp_hres_layers' stack.
 * Checks: their siblings', then Hh > 1, Wh > 1 and Hh * Wh * 12 < 2^31 ahead of the tile entry points' checks.  Error texts
 * name hres_index_tiles_edge / pp_hres_layers_sparse. */
int msi_hres_index_tiles_edge(const float *alphas, int32_t format, int32_t batch, int32_t low_height, int32_t low_width,
                              int32_t height, int32_t width, int32_t num_planes,
                              int32_t *table_out, int32_t *counts_out, msi_stream_t stream);
int msi_pp_hres_layers_sparse(const float *ref_image, const float *src_image, const float *ref_curr_pose, const float *src_curr_pose,
                              const float *intrinsics, const float *depths, const float *blend_weights, const float *alphas,
                              int32_t batch, int32_t low_height, int32_t low_width, int32_t height, int32_t width, int32_t num_planes,
                              const int32_t *table, const int64_t *layer_start, void *pool_out, int32_t format, msi_stream_t stream);
/* MSI.mpi_render_view (msi.py:527-548): pj.projective_forward_homography (projector.py:343-373) ->
 * homography.planar_transform (homography.py:35-157) -> tf.contrib.resampler (zero padding) ->
 * pj.over_composite.  intrinsics_inv [B,3,3] replaces the hidden graph input `intrinsics_inv:0`
 * (homography.py:52). */
int msi_mpi_render_f32(const float *rgba_native, const float *tgt_pose, const float *intrinsics,
                       const float *intrinsics_inv, const float *depths, int32_t batch, int32_t height,
                       int32_t width, int32_t num_planes, float *out_rgb, msi_stream_t stream);
/* Many views of one MPI per launch (MSI.mpi_render_views; no reference counterpart): V target cameras per stack, each rendered
 * as msi_mpi_render_f32 renders its one view, at any output size, from an fp32 or a packed stack.
 *   layers             [B,D,H,W] texels of `format`: MSI_LAYERS_F32 (rgba_native), MSI_LAYERS_RGBA8 or MSI_LAYERS_RGBA16F
 *   tgt_pose           [B*V,4,4]  view v of sample b at index b*V + v; it samples stack b only
 *   intrinsics         [B,3,3]    the SOURCE camera K of stack b
 *   tgt_intrinsics_inv [B*V,3,3]  the inverse of the TARGET camera of view (b, v), in pixels of the output size
 *   depths             [D] (far -> near), D <= 128
 *   out_rgb [B,V,out_height,out_width,3], out_depth [B,V,out_height,out_width]; either may be NULL, not both.
 * Contract:
 *   rgb    Pixel (i, j) of the output is the point (j, i, 1) of meshgrid_abs at the OUTPUT size, taken through the inverse
 *          homography K_s (R^T + R^T t n^T R^T / (-depth - n^T R^T t)) K_t^-1 of each plane, sampled with the zero-padding
 *          bilinear resampler and over-composited far to near, with msi_mpi_render_f32's operations in its order.  With
 *          (out_height, out_width) = (H, W) and tgt_intrinsics_inv = its intrinsics_inv, every view is BIT-IDENTICAL to
 *          msi_mpi_render_f32 with that view's pose.
 *   depth  pj.over_composite_depth (projector.py:225-244) of the same warped layers, ONE channel: 0 at the farthest layer,
 *          then (d / D) * alpha + out * (1 - alpha) with d / D the fp32 rounding of the fp64 quotient -- the composited plane
 *          index / D as in msi_render_views_f32, not a physical depth.
 *   zero padding  A sample outside (-1, W) x (-1, H) contributes (0, 0, 0, 0) for that layer, a corner outside the layer
 *          contributes zeros with its weight (no wrap-around): where every layer samples outside, rgb and depth are 0.
 *   packed stacks  Every tap is decoded by the rule of msi_unpack_layers, so the outputs are bit-identical to the same call
 *          on the msi_unpack_layers of the stack with MSI_LAYERS_F32.
 * Argument checks before any launch, in this order, MSI_E_BADARG unless noted: both outputs NULL; a NULL input; an unknown
 * format; batch < 0 or a non-positive height / width / num_planes ("bad dims"); num_planes > 128 -> MSI_E_UNSUPPORTED;
 * views < 1; an output size below 1 x 1; H * W >= 2^24 (24-bit texel offsets); more than 2^31 - 8 workgroups (64 x 4
 * output pixels each).  batch = 0 then returns MSI_OK without a launch. */
int msi_mpi_render_views(const void *layers, int32_t format, const float *tgt_pose, const float *intrinsics,
                         const float *tgt_intrinsics_inv, const float *depths, int32_t batch, int32_t views, int32_t height,
                         int32_t width, int32_t num_planes, int32_t out_height, int32_t out_width, float *out_rgb,
                         float *out_depth, msi_stream_t stream);

/* ---- cube-map viewer of the PP path (MSI.cube_render_views / MSI.equirect_to_cube; no reference counterpart) ----------
 * The cube frame is the camera frame of face 0: x right, y down, z forward.  Face f has orientation R_f, whose columns are
 * the face camera's x, y, z axes in the cube frame:
 *   f  0 front (+z)  1 right (+x)  2 back (-z)   3 left (-x)   4 up (-y)     5 down (+y)
 *   x  (1,0,0)       (0,0,-1)      (-1,0,0)      (0,0,1)       (1,0,0)       (1,0,0)
 *   y  (0,1,0)       (0,1,0)       (0,1,0)       (0,1,0)       (0,0,1)       (0,0,-1)
 *   z  (0,0,1)       (1,0,0)       (0,0,-1)      (-1,0,0)      (0,-1,0)      (0,1,0)
 * A cube stack is the native stack [6B,D,S,S] of square faces, face f of sample b at entry 6 b + f (what the PP network
 * writes for a batch of 6B faces); texel (ix, iy) of layer d of face f is the cube-frame point R_f depths[d] K^-1 (ix, iy, 1)
 * with the sample's stack camera K (integer-pixel convention of the MPI path), so layer d of the six faces is a cube shell
 * of half-side depths[d].
 *
 * msi_cube_render_views: V views per sample in one launch, msi_render_views_f32's cameras, pose model and outputs.
 *   layers            [6B,D,S,S] texels of `format` (MSI_LAYERS_F32, _RGBA8 or _RGBA16F), depths [D] far -> near, D <= 128
 *   tgt_pose_rt       [B*V,4,4], tgt_pos [B*V,3]: direction rotated by pose[:3,:3], origin pose @ (tgt_pos[2], tgt_pos[1],
 *                     tgt_pos[0], 1); this render frame (forward +x, down +y, right +z) maps to the cube frame by swapping x
 *                     and z, so the centre of an equirect output looks at the centre of face 0
 *   tgt_intrinsics    [B*V,3,3] (MSI_CAMERA_PINHOLE; trig unused), trig = the table of (out_height, out_width)
 *                     (MSI_CAMERA_EQUIRECT; tgt_intrinsics unused)
 *   stack_intrinsics  [B,3,3] the camera K shared by a sample's six faces
 *   out_rgb [B,V,out_height,out_width,3], out_depth [B,V,out_height,out_width] (the composited d / D); either may be NULL
 * Per shell, for origin o and direction r in the cube frame and h = depths[d]: t = min over the axes with r_k != 0 of
 * (h sign(r_k) - o_k) / r_k, P = o + t r; the face is the axis of the largest |P_k| with its sign (ties: z, x, y);
 * p = R_f^T P, u = fx p_x / h + cx, v = fy p_y / h + cy, both CLAMPED to [0, S-1], bilinear over the four texels of THAT face
 * (clamp to edge: no zero padding, no fetch from the neighbouring face -- with fx = cx = S/2 a face covers [-1, 1 - 2/S] in
 * tan space; fx = cx = (S-1)/2 makes it symmetric); composite strictly far to near: layer 0 replaces, then c a + acc (1 - a).
 * A packed stack is decoded by the rule of msi_unpack_layers: the outputs are bit-identical to the same call on the unpacked
 * stack.  status_device as in msi_render_views_f32: MSI_RENDER_STATUS_ORIGIN_OUTSIDE when a view's origin is not strictly
 * inside the innermost shell (max |o_k| >= min depths, or NaN); its pixels are finite for finite inputs.  Every texel address
 * is in range by construction for any input.
 * Argument checks before any launch, in this order, MSI_E_BADARG unless noted: both outputs NULL; a NULL stack / pose /
 * position / stack_intrinsics / depths; unknown format; unknown camera; a NULL trig (equirect) / tgt_intrinsics (pinhole);
 * batch < 0 or non-positive face_size / num_planes ("bad dims"); num_planes > 128 -> MSI_E_UNSUPPORTED; views < 1; an output
 * size below 1 x 1 (2 x 2 for the pinhole camera); a sample whose six face stacks reach 2^31 bytes (32-bit per-lane offsets);
 * more than 2^31 - 8 workgroups.  batch = 0 returns MSI_OK, no launch. */
int msi_cube_render_views(const void *layers, int32_t format, const float *tgt_pose_rt, const float *tgt_pos,
                          const float *tgt_intrinsics, const float *stack_intrinsics, const float *depths, const float *trig,
                          int32_t batch, int32_t views, int32_t face_size, int32_t num_planes, int32_t camera,
                          int32_t out_height, int32_t out_width, float *out_rgb, float *out_depth, int32_t *status_device,
                          msi_stream_t stream);
/* msi_cube_render_views with the SEAMLESS filter (MSI.cube_render_views(filtering='seamless')): the same arguments, checks, codes,
 * cameras, outputs and composite; only the taps differ.  With the cube camera fx = fy = cx = cy = S/2 a face stores tan = -1 ..
 * 1 - 2/S and nothing on its +x and +y edges, so the clamp rule repeats the last texel over a one-texel band along cube edges;
 * the neighbouring face usually stores a sample at exactly the missing point (its column 0 or row 0 lies on the shared edge).
 * The rule is defined for that camera only (the cube point of lattice point (x, y), 0 <= x, y <= S, of a face is then a lattice
 * point of every other face containing it).  Ray, shell hit, face choice and p = R_f^T P are msi_cube_render_views', op for op.
 *   1. u and v are clamped to [0, S] instead of [0, S-1] (fmaxf first: a NaN still becomes 0).
 *   2. x0 = min(floor(u), S-1), x1 = x0 + 1 <= S, du = u - x0 in [0, 1]; y0, y1, dv likewise.
 *   3. The four taps are bilinear with msi_cube_render_views' weights and summation order.
 *   4. A tap with x < S and y < S is the face's own texel.
 *   5. A tap with x = S or y = S is a VIRTUAL texel at the cube point P of that lattice point (an edge point; a cube corner when
 *      the other coordinate is 0 or S).  The other faces that contain P -- one for an edge point, two for a corner -- are taken
 *      in ascending face index; the first whose lattice coordinates of P lie in [0, S-1]^2 supplies its texel (one fetch).  When
 *      no face stores P the virtual texel is the mean of the clamped texels (each face's coordinates of P clamped to [0, S-1])
 *      of all faces meeting at P, own face first, then the others in ascending face index: (a + b) * 0.5f for two faces,
 *      ((a + b) + c) * (1.0f / 3.0f) for three; per channel, alpha included, on decoded fp32 values (a packed render keeps the
 *      bits of the render of the unpacked stack).
 * The three classes of the 12 cube edges under this rule:
 *   8 are stored by ONE face (the ring front -> right -> back -> left -> front; front/up, front/down, up/right, down/left): the
 *     filter is continuous across them;
 *   2 have NO stored sample (right/down, back/down): the mean rule makes the filter continuous over a two-texel span;
 *   2 are stored TWICE (up/back, up/left: row 0 of both faces): each face keeps its own texel, so a step in the CONTENT of the
 *     two faces remains there.  That is not a filtering artefact; in-range texels are never overridden.
 * The +x/+y corner square of a face reaches a cube corner: the three-face rule makes every face that sees it agree on its value.
 * A sample whose stack_intrinsics are not exactly (S/2, S/2, S/2, S/2) is rendered with the clamp rule, the bits of
 * msi_cube_render_views, and MSI_RENDER_STATUS_NOT_CUBE_CAMERA is ORed into *status_device.  Every texel address is in range by
 * construction for any input.  Not supported: sparse stacks (msi_cube_render_views_sparse has no seamless twin). */
int msi_cube_render_views_seamless(const void *layers, int32_t format, const float *tgt_pose_rt, const float *tgt_pos,
                                   const float *tgt_intrinsics, const float *stack_intrinsics, const float *depths, const float *trig,
                                   int32_t batch, int32_t views, int32_t face_size, int32_t num_planes, int32_t camera,
                                   int32_t out_height, int32_t out_width, float *out_rgb, float *out_depth, int32_t *status_device,
                                   msi_stream_t stream);
/* The ODS stereo camera of the cube viewer (MSI.cube_render_views(camera='ods'), MSI.cube_render_ods_pair): V eye panoramas of each
 * cube per launch -- both eyes of a stereo 360 frame are V = 2 -- from dense stacks with either filter (msi_cube_render_ods_views:
 * filtering 0 = the clamp taps of msi_cube_render_views, 1 = the seamless taps of msi_cube_render_views_seamless) or from an
 * edge-rule sparse stack with the clamp taps (msi_cube_render_ods_views_sparse: (pool, table, layer_start, format) in place of
 * the stack, msi_cube_render_views_sparse's contract).  As msi_render_ods_views beside msi_render_views_f32, they are entry
 * points of their own, not a camera code: the codes of the *_render_views functions stay 0 and 1.  Pixel (i, j) of the lat-long
 * grid of the OUTPUT size, before the pose:
 *     direction  r = (cos S_j cos T_i, sin T_i, sin S_j cos T_i)                               -- the equirect camera's
 *     origin     c = (tgt_pos[2] + sin S_j * e, tgt_pos[1], tgt_pos[0] + (-cos S_j) * e)       -- e = eye_radius[b*V + v]
 *   then r <- pose[:3,:3] r, c <- pose (c, 1), the swap of x and z into the cube frame, and from there the arithmetic of the
 *   entry point named above, op for op: shell hit, face choice and its tie rule, p = R_f^T P, the taps, the bilinear sum order,
 *   the far-to-near composite.  (sin S, 0, -cos S) . r = 0: the ray is tangent to the circle of radius |e| around the head
 *   position.  e is SIGNED as in msi_render_ods_views: e = +baseline is the left eye, e = -baseline the right eye.
 *   eye_radius [B*V] (view v of sample b at index b*V + v), trig = the msi_build_trig_tables_host table of (out_height,
 *   out_width); both required.  Every other argument as in msi_cube_render_views.
 * Facts that fix the convention (tests/test_cube_ods_cpu.py holds the fp64 reference to them, tests/test_gpu_cube_ods.py the kernels):
 *   1. e = 0 is the equirect camera: outputs and status word are bit-identical to msi_cube_render_views / _seamless / _sparse
 *      with MSI_CAMERA_EQUIRECT for the same poses, positions and size.
 *   2. The eye sign is the sphere camera's: for content mirror-symmetric under the render frame's right axis (z -> -z), head at
 *      the origin and identity pose, the right-eye image is the left-eye image flipped left to right.
 *   3. The parallax vanishes with distance: the render of a shell of half-side h converges to the equirect render as h / |e| grows.
 * status_device (may be NULL): the origin differs from pixel to pixel here, so MSI_RENDER_STATUS_ORIGIN_OUTSIDE is set when ANY
 * rendered pixel's origin is not strictly inside the innermost shell (max_k |o_k| >= min depths, or NaN) -- also when only a part
 * of the circle leaves it (every lane tests its own origin; one atomic OR per wavefront that has such a lane).  Pixels stay finite
 * for finite inputs.  MSI_RENDER_STATUS_NOT_CUBE_CAMERA (filtering 1) is msi_cube_render_views_seamless'.
 * Argument checks before any HIP call, in this order, MSI_E_BADARG unless noted.  msi_cube_render_ods_views: both outputs NULL; a
 * NULL input (every pointer but the outputs and status_device is required, eye_radius and trig included); unknown format; batch < 0
 * or non-positive face_size / num_planes ("bad dims"); unknown filtering; num_planes > 128 -> MSI_E_UNSUPPORTED; views < 1; an
 * output size below 1 x 1; a sample whose six face stacks reach 2^31 bytes; more than 2^31 - 8 workgroups.
 * msi_cube_render_ods_views_sparse: both outputs NULL; a NULL input; unknown format (MSI_LAYERS_F32 included); bad dims; more than
 * 128 planes, then S % 16 -> MSI_E_UNSUPPORTED; views < 1; an output size below 1 x 1; the 2^31-byte limit (of the DENSE stacks);
 * the grid limit.  batch = 0 then returns MSI_OK without a launch. */
int msi_cube_render_ods_views(const void *layers, int32_t format, const float *tgt_pose_rt, const float *tgt_pos,
                              const float *eye_radius, const float *stack_intrinsics, const float *depths, const float *trig,
                              int32_t batch, int32_t views, int32_t face_size, int32_t num_planes, int32_t filtering,
                              int32_t out_height, int32_t out_width, float *out_rgb, float *out_depth, int32_t *status_device,
                              msi_stream_t stream);
int msi_cube_render_ods_views_sparse(const void *pool, const int32_t *table, const int64_t *layer_start, int32_t format,
                                     const float *tgt_pose_rt, const float *tgt_pos, const float *eye_radius,
                                     const float *stack_intrinsics, const float *depths, const float *trig,
                                     int32_t batch, int32_t views, int32_t face_size, int32_t num_planes,
                                     int32_t out_height, int32_t out_width, float *out_rgb, float *out_depth, int32_t *status_device,
                                     msi_stream_t stream);
/* Panorama -> six face images: image [B,H,W,C] fp32 (C in 1..4) -> out [B,6,S,S,C].  Texel (ix, iy) of face f looks along
 * R_f K^-1 (ix, iy, 1) with intrinsics [B,3,3]; with x and z swapped that is a direction of the render frame, sampled at
 * u = (atan2(z, x) + pi) / 2pi W - 0.5, v = (asin(y / |dir|) + pi/2) / pi H - 0.5 (the inverse of the lat-long grid of
 * msi_build_trig_tables_host), bilinear, wrapping in u and clamping in v. */
int msi_equirect_to_cube_f32(const float *image, const float *intrinsics, int32_t batch, int32_t height, int32_t width,
                             int32_t channels, int32_t face_size, float *out, msi_stream_t stream);

/* ---- cube path, source half sampled from the source PANORAMA (MSI.format_cube_input; src_sampling='panorama' of
 * MSI.infer_cube / MSI.hres_cube_layers; no reference counterpart) --------------------------------------------------------
 * The face-wise cube path sweeps each face's own source image with the wrap-around sampler: a plane point that projects past
 * the face's border gets texels from the opposite side of the SAME face.  These entry points take the source panorama itself
 * and look every plane point up along its own direction, so such a point gets the neighbouring face's content.  They are the
 * face-wise twins with that one change; `batch` is the number of CUBES B, every per-face array has 6 B entries (face f of cube
 * b at 6 b + f, faces in the table above), faces are square (face_size = S).
 * The sample position, shared by all four (one device function): for face f = n % 6 of entry n, pixel (i, j), plane depth d,
 * P = face_pose[n] and K = intrinsics[n]:
 *   X = backproject_planar and a = apply_pose(P, X) exactly as msi_perspective_plane_sweep_f32 computes them; Y = apply_pose(P, a)
 *   (the reference applies the pose twice -- once in apply_pose, once inside project_perspective through K4 @ pose -- so the
 *   face sweep samples K Y: Y is the direction it looks along wherever its (u, v) falls inside the face; no K enters Y);
 *   dir = R_f Y (a signed permutation); lon = atan2(dir_x + 0, dir_z + 0), lat = asin(dir_y / |dir|) (the sweep's and render's
 *   angle helpers, 1.3e-7 rad; libm with -DMSI_FAST_TAIL=0); u = (lon + pi) / 2pi Wp - 0.5, v = (lat + pi/2) / pi Hp - 0.5;
 *   u clamped to [-0.5, Wp - 0.5] and wrapped, v clamped to [0, Hp - 1] (msi_equirect_to_cube_f32's sampler, its weights and
 *   sum order).  A NaN coordinate (Y = 0, a non-finite pose) becomes the lower bound before the float -> int conversion:
 *   every texel address lies inside the cube's own panorama for any input.
 *
 * msi_cube_plane_sweep_f32   msi_perspective_plane_sweep_f32 of one source: writes channels [channel_offset, channel_offset +
 *                            3 D) of psv [6B,S,S,psv_channels] and nothing else.  panorama [B,Hp,Wp,3], face_pose [6B,4,4],
 *                            intrinsics [6B,3,3], depths [D].  Both kernel forms and the store policy are the twin's, chosen by
 *                            the twin's conditions.
 * msi_cube_sweep_volume_bf16 msi_perspective_sweep_volume_bf16: the whole bf16 network input [6B,S,S,6D] in one launch.  The ref
 *                            half [0,3D) comes from ref_faces [6B,S,S,3] with ref_face_pose and has that entry point's bits;
 *                            the src half [3D,6D) is the round to nearest even of msi_cube_plane_sweep_f32 with
 *                            src_face_pose, bit for bit.
 * msi_cube_hres_layers       msi_pp_hres_layers with the background taps from the panorama: the bits of
 *                            msi_perspective_plane_sweep_f32 (ref faces) + msi_cube_plane_sweep_f32 (panorama) at face_size ->
 *                            msi_resize_bilinear_f32 of blend_weights / alphas [6B,s,s,D] (s = low_size) ->
 *                            msi_assemble_rgba_scaled_f32; rgba_native [6B,D,S,S,4] and / or layers_out (msi_pack_layers of
 *                            it); outputs, formats and store policy as msi_pp_hres_layers.
 * msi_cube_hres_layers_sparse  msi_pp_hres_layers_sparse likewise: equal to msi_sparse_gather_tiles of msi_cube_hres_layers'
 *                            stack; the table is msi_hres_index_tiles_edge's (batch 6B): alphas do not depend on the sweep.
 * Checks before any launch, MSI_E_BADARG unless noted: (hres: unknown format, both outputs NULL;) a NULL pointer; (sweeps:
 * num_depths < 1;) batch < 0 or face_size < 2; Hp < 2 or Wp < 2; Hp * Wp * 12 >= 2^31; 6 * batch or face_size above 65535;
 * S * S * 12 >= 2^31; then the twin's own (the channel window; msi_hres_layers' checks with batch 6B, num_planes % 4 ->
 * MSI_E_UNSUPPORTED; the tile entry points' checks).  batch = 0 then returns MSI_OK without a launch.  Error texts name
 * cube_plane_sweep / cube_sweep_volume_bf16 / cube_hres_layers / cube_hres_layers_sparse. */
int msi_cube_plane_sweep_f32(const float *panorama, const float *face_pose, const float *intrinsics, const float *depths,
                             int32_t batch, int32_t pano_height, int32_t pano_width, int32_t face_size, int32_t num_depths,
                             float *psv, int32_t psv_channels, int32_t channel_offset, msi_stream_t stream);
int msi_cube_sweep_volume_bf16(const float *ref_faces, const float *src_panorama, const float *ref_face_pose,
                               const float *src_face_pose, const float *intrinsics, const float *depths, int32_t batch,
                               int32_t pano_height, int32_t pano_width, int32_t face_size, int32_t num_depths, void *psv_bf16,
                               msi_stream_t stream);
int msi_cube_hres_layers(const float *ref_faces, const float *src_panorama, const float *ref_face_pose, const float *src_face_pose,
                         const float *intrinsics, const float *depths, const float *blend_weights, const float *alphas,
                         int32_t batch, int32_t pano_height, int32_t pano_width, int32_t low_size, int32_t face_size,
                         int32_t num_planes, float *rgba_native, void *layers_out, int32_t format, msi_stream_t stream);
int msi_cube_hres_layers_sparse(const float *ref_faces, const float *src_panorama, const float *ref_face_pose,
                                const float *src_face_pose, const float *intrinsics, const float *depths,
                                const float *blend_weights, const float *alphas, int32_t batch, int32_t pano_height,
                                int32_t pano_width, int32_t low_size, int32_t face_size, int32_t num_planes, const int32_t *table,
                                const int64_t *layer_start, void *pool_out, int32_t format, msi_stream_t stream);

/* ---- image scores --------------------------------------------------------------------
 * eval.py:127-174 (tf.image.ssim, tf.image.psnr with max_val 255; the mean absolute difference of consecutive frames) for
 * images that are already on the device; matryodshka_amd/evaluate.py is the host statement of the same numbers.  Per pair p
 * of n_pairs: pred image p against target image p / group (group = 1: one to one; group = V: [B,V,...] renders against
 * [B,...] ground truth; group = n_pairs: everything against one image).
 *   pred    [n_pairs, H, W, C]          C in 1..4; both fp32 (MSI_SCORE_F32) or both uint8 (MSI_SCORE_U8)
 *   target  [n_pairs / group, H, W, C]
 *   transform, applied to both images as a pixel is read (fp64 from there on):
 *     MSI_SCORE_RAW    the value as it is (the only transform of uint8 images)
 *     MSI_SCORE_IMAGE  ((double)x + 1) / 2 * 255;  MSI_SCORE_DEPTH  (double)x * 255
 *     quantize = 1 (IMAGE or DEPTH, fp32 only): the 8-bit level msi_deprocess_f32_u8 stores, op for op in fp32 (NaN -> 0)
 *   row_weights  [H] doubles on the device or NULL (all ones): one weight per image row, e.g. the solid angle of an
 *     equirectangular row (WS-PSNR)
 *   metrics  MSI_SCORE_MSE | MSI_SCORE_MAE | MSI_SCORE_SSIM
 *   out  [n_pairs][4] doubles = mse, mae, ssim, psnr; NaN where not requested (psnr comes with MSI_SCORE_MSE):
 *     mse  = sum_r w_r sum_{c,ch} d^2 / (sum_r w_r * W * C), mae the same with |d|
 *     psnr = 20 log10(max_val) - 10 log10(mse), +inf when mse = 0
 *     ssim = tf.image.ssim: 11 x 11 softmax-normalised Gaussian (sigma 1.5) applied separably at VALID positions, k1 = 0.01,
 *            k2 = 0.03, the mean of the lum * cs map, a map row weighted with the weight of its window's centre row:
 *            sum_i w_{i+5} sum_{j,ch} map / (sum_i w_{i+5} * (W - 10) * C)
 *   workspace  msi_score_workspace_bytes(n_pairs, H, W, C) bytes (0 and an error text for dims it refuses); it may arrive
 *     uninitialised.
 * fp64 arithmetic, no atomics: a pair's four numbers are bit-reproducible from call to call and do not depend on how many other
 * pairs share the call.  Sums of integer levels (uint8 or quantised images, no weights) are exact.
 * Argument checks before any HIP call: MSI_E_BADARG for a NULL pred / target / out / workspace, n_pairs < 1, group < 1 or not a
 * divisor of n_pairs, a non-positive height / width, C outside 1..4, an unknown dtype / transform, quantize or a non-RAW
 * transform with uint8, quantize with RAW, an empty or unknown metrics mask, SSIM with min(H, W) < 11, max_val <= 0;
 * MSI_E_UNSUPPORTED for more than 2^31 - 1 workgroups (16 x 32 map positions each); MSI_E_WORKSPACE for a workspace that is too small. */
#define MSI_SCORE_F32 0
#define MSI_SCORE_U8 1
#define MSI_SCORE_RAW 0
#define MSI_SCORE_IMAGE 1
#define MSI_SCORE_DEPTH 2
#define MSI_SCORE_MSE 1u
#define MSI_SCORE_MAE 2u
#define MSI_SCORE_SSIM 4u
size_t msi_score_workspace_bytes(int32_t n_pairs, int32_t height, int32_t width, int32_t channels);
int msi_score_images(const void *pred, const void *target, int32_t dtype, int32_t transform, int32_t quantize, int32_t n_pairs,
                     int32_t group, int32_t height, int32_t width, int32_t channels, const double *row_weights, double max_val,
                     uint32_t metrics, double *out, void *workspace, size_t workspace_bytes, msi_stream_t stream);

/* ---- K2: encoder-decoder CNN -------------------------------------------------------
 * nets.msi_coord_train_net (nets.py:471-515; coord_net=1) and nets.msi_train_net
 * (nets.py:387-450; coord_net=0): 14x conv3x3 (+|sin(lat)| coordinate channel,
 * nets.py:260-270), 3x conv-transpose 4x4 s2, LayerNorm over (H,W,C) + ReLU after
 * each, 1x1 tanh head with bias.  Implicit-GEMM on fp32 MFMA; LayerNorm sums are produced by the conv
 * epilogue -- order-independent 64-bit fixed-point accumulation (one word per sum, every wave's share rounded to one
 * unit) inside a per-layer window whose exponent the packer derives from the weights; a forward whose statistics leave
 * that window reports it through msi_net_plan_status instead of returning silently wrong values -- and applied with
 * the ReLU by the consumer while it stages its input (halo-patch kernels, head) or by one in-place pass per layer.  msi_train_net's conv-transposes are normalised over their uncropped
 * (2H+10) x (2W+10) VALID output, as nets.py:423-435 does, before the [5:-5] crop. */
typedef struct msi_net_desc {
  int32_t batch, height, width; /* height, width multiples of 8 */
  int32_t in_channels;          /* 6*D */
  int32_t num_outputs;          /* 2*D for blend_psv */
  int32_t ngf;                  /* 64 in the reference */
  int32_t coord_net;            /* 1: msi_coord_train_net, 0: msi_train_net */
  int32_t dtype;                /* MSI_DTYPE_F32 (0) or MSI_DTYPE_BF16 (1): operand type of the convolutions */
} msi_net_desc;

#define MSI_DTYPE_F32 0
#define MSI_DTYPE_BF16 1

#define MSI_NET_NUM_LAYERS 18

typedef struct msi_layer_info {
  char name[16];          /* TF scope name: conv1_1 ... conv8_2, color_pred */
  int32_t kind;           /* 0 conv3x3, 1 convT4x4s2, 2 head 1x1 */
  int32_t cin, cout;      /* cin without the coordinate channel */
  int32_t has_coord;
  int32_t stride, rate;
  int32_t in_h, in_w, out_h, out_w;
  uint64_t param_offset;  /* float offset of `weights` in the parameter blob   */
  uint64_t param_floats;  /* weights + gamma + beta (or + biases)              */
  uint64_t raw_offset;    /* BYTE offset of the raw (pre-LayerNorm) output in  */
                          /* the workspace; (uint64)-1 for the head.  fp32     */
                          /* plans: fp32 [B,H,W,cout]; bf16 plans: fp16 of     */
                          /* x * 2^-e, e = the layer's LayerNorm window (below) */
  uint64_t affine_offset; /* BYTE offset of scale[cout] shift[cout] in the ws  */
  uint64_t ln_scale_offset; /* FLOAT offset in the PACKED blob of four doubles */
                          /* {S1, S2, 1/S1, 1/S2}, S1 = 2^(24 - e), S2 =       */
                          /* 2^(16 - 2e): the fixed-point window of the layer's */
                          /* LayerNorm sums; 2^e = 2^24 / S1                    */
} msi_layer_info;

/* Parameter blob ("reference layout"), fp32, layers in graph order; per layer
 *   conv3x3 : weights [3,3,cin+has_coord,cout], gamma [cout], beta [cout]
 *   convT   : weights [4,4,cout,cin],           gamma [cout], beta [cout]
 *   head    : weights [1,1,cin,cout],           biases [cout]
 * i.e. the TF variables net/<name>/weights, .../LayerNorm/gamma, .../LayerNorm/beta,
 * net/color_pred/{weights,biases} (test.py:191-202 restores exactly these). */
int msi_net_layer_info(const msi_net_desc *desc, int32_t layer, msi_layer_info *out);
size_t msi_net_param_floats(const msi_net_desc *desc);
size_t msi_net_packed_floats(const msi_net_desc *desc);
int msi_net_pack_weights_host(const msi_net_desc *desc, const float *params_host,
                              float *packed_host);
size_t msi_net_workspace_bytes(const msi_net_desc *desc);

/* A plan resolves everything about a descriptor that does not depend on the buffers -- layer table, tile
 * choice and work decomposition per layer, workspace layout, the CU count of the current device
 * (hipDeviceProp.multiProcessorCount) -- once, so that msi_net_plan_forward does no allocation and no
 * per-layer set-up arithmetic.  The plan is host memory owned by the caller (create / destroy); forward takes
 * it const and keeps all per-call state on the stack: concurrent forwards on one plan (different streams,
 * different workspaces) are safe.  Options replace what used to be environment variables; they are per plan,
 * never process-global, and changing one re-plans (query msi_net_plan_workspace_bytes again afterwards). */
typedef struct msi_net_plan msi_net_plan;
#define MSI_NET_OPT_FIXUP_KERNEL 0 /* 0 (default): split tiles are summed inside the conv launch (last arriver);  */
                                   /* 1: by a separate conv_fixup_kernel launch (bitwise-identical results)       */
#define MSI_NET_OPT_TAILSPLIT 1    /* cut the tiles of the partial last round along K: 1 (default) whole tiles in multiples of   */
                                   /* the CU count, 2 in multiples of a full residency (5 workgroups x CUs; measured slower), 0 never */
#define MSI_NET_OPT_BIGTILE 2      /* bf16 tile choice: 0 never 128x128 / 128x64, 1 (default) by grid size, 2 always */
#define MSI_NET_OPT_HEAD_FUSE_LN 3 /* 1 (default): the fp32 head applies its source's LayerNorm while loading      */
#define MSI_NET_OPT_NUM_CUS 4      /* CUs the work decomposition balances over (default: the device's count)      */
#define MSI_NET_OPT_F32_TILE 5     /* retired (were: the fp32 128x64 / 64x128 tap-kernel tiles and their per-layer mask, measured   */
#define MSI_NET_OPT_F32_TILE_MASK 6 /* slower): 0 is accepted and does nothing, anything else is MSI_E_UNSUPPORTED (F32_TILE outside 0..2: MSI_E_BADARG) */
#define MSI_NET_OPT_APPLY_AHEAD 7   /* retired (was: a layer's LayerNorm + ReLU applied by the first workgroups of its consumer's    */
                                   /* launch, measured slower: DESIGN.md): 0 is accepted and does nothing, anything else is MSI_E_UNSUPPORTED */
#define MSI_NET_OPT_HALO 8          /* default 5.  bit 0: the stride-1 3x3 layers run the halo-patch kernels (conv_halo_kernel fp32,   */
                                   /* conv_halo_bf16_kernel: one LDS-stationary halo patch per workgroup and input chunk, the          */
                                   /* producer's LayerNorm applied while staging it) and the bf16 conv-transposes                      */
                                   /* convt_halo_bf16_kernel; bit 1 (measured slower: opt-in): the fp32 SAME conv-transposes run       */
                                   /* convt_halo_kernel (the two classes of one output-row parity per workgroup, either source's       */
                                   /* LayerNorm applied while staging); bit 2: the fp32 stride-2 3x3 layers run conv_halo_s2_kernel    */
                                   /* (four parity-plane patches per 32-channel group, the producer's LayerNorm applied while staging);*/
                                   /* 0: tap-DMA kernel everywhere.  With F32_SPLIT3 on for a layer (the default) ANY non-zero HALO    */
                                   /* value lets that layer take its split halo kernel: the conv-transposes run convt_halo_x3_kernel    */
                                   /* without bit 1 and the stride-2 layers conv_halo_s2_x3_kernel whatever their grid size (the native */
                                   /* stride-2 form is only chosen at >= 3 tiles per CU); set F32_SPLIT3 = 0 to get the bit-by-bit      */
                                   /* selection described above                                                                         */
#define MSI_NET_OPT_HALO_SKIP 9     /* bit i = layer i (graph order) does NOT take a halo kernel although it qualifies (tuning)          */
#define MSI_NET_OPT_UNIFORM_SPLIT 10 /* s >= 2: layers with one to two 64x64 tiles per CU cut EVERY tile into s equal K-ranges (tuning; 0 = default split) */
#define MSI_NET_OPT_BF16_STAGE_RAW 11 /* bf16 plans: bit 0 the 256x64 conv tile (conv8_2), bit 1 the 128x64 conv-transpose tile (conv8_1) read their  */
                                      /* sources RAW (fp16) and apply the producer's LayerNorm while staging (default 1: bit 1 measured slower); 0: from ln_apply's bf16 copies */
#define MSI_NET_OPT_SPLIT_OVERHEAD 12 /* k-steps of prologue + epilogue a K-range visit is charged in the tail-split cost model (tuning; 0 = r01 rule) */
#define MSI_NET_OPT_BF16_WAVES 13 /* waves per workgroup of the bf16 halo-patch conv kernel's 128x128 tile: 8 (default; 4 x 2 waves of 32 pixels x 64 channels: */
                                  /* four waves per SIMD with two workgroups per CU, so that a workgroup's prologue / epilogue has neighbours to hide behind) */
                                  /* or 4 (r02 shape).  The 256x64 tile always runs four (eight measured slower) */
#define MSI_NET_OPT_F32_SPLIT3 14 /* fp32 plans, bit i = layer i (graph order): a 3x3 layer (stride 1 or 2, rate 1 or 2) or conv-transpose (SAME, or msi_train_net's */
                                  /* wrap_pad + VALID form) that qualifies for a halo-patch kernel (MSI_NET_OPT_HALO != 0) computes its fp32 convolution as a 3-way */
                                  /* bf16 split of both operands with SIX products (h.h, h.m, m.h, h.l, l.h, m.m; exact products, fp32 accumulation; */
                                  /* dropped terms <= 2^-26 of a product: fp32-grade, NOT the 3-product TF32-grade split) on the 16x faster bf16 MFMA */
                                  /* (conv_halo_x3_kernel).  Default 0x3ffff (every layer that qualifies); 0 = native fp32 MFMA (v_mfma_f32_32x32x2_f32) everywhere */
#define MSI_NET_OPT_F32_SPLIT_F16 15 /* fp32 plans, bit i = layer i: a layer that runs the split (F32_SPLIT3) uses its fp16 form -- x = h + m' 2^-11 with fp16 */
                                     /* parts (22 significand bits), THREE products h.h + (h.m' + m'.h) 2^-11, fp32 accumulation: half the matrix work of the */
                                     /* six-product bf16 form at the same measured error (profiles/r04_split_numerics.txt), but the operands must lie in */
                                     /* the fp16 RANGE: |x| > 65504 (weights or normalised activations) poisons the layer and sets MSI_NET_STATUS_F16_SPLIT_RANGE. */
                                     /* The 22 bits hold for |x| >= 2^-14 only: below that h, and below 2^-25 m' too, are fp16 subnormals (absolute resolution 2^-24 and */
                                     /* 2^-35) -- LayerNorm'd activations and slim-initialised weights sit far above; nothing flags an operand that small.  NaN operands */
                                     /* set the status bit like |x| > 65504. */
                                     /* Default 0 (opt-in: 22-bit operands are narrower than fp32's 24 -- the default fp32 arithmetic stays the six-product bf16 form); */
                                     /* 0x3ffff = every layer that runs the split, msi_train_net's conv-transposes included (until r05 those ignored the bit: the r04 */
                                     /* finding that kept them on the bf16 form is closed, DESIGN.md section 4 "the wobble") */
#define MSI_NET_OPT_X3_TILE8 16 /* fp32 plans, bit i = layer i: a stride-1, rate-1 layer on the six-product split (F32_SPLIT3 without F32_SPLIT_F16) whose input height is a  */
                                /* multiple of 8 runs conv_halo8_x3_kernel: 8 x 16-pixel x 64-channel tiles, two accumulators per wave sharing the weight fragments -- half */
                                /* the weight bytes L2 -> LDS, half the prologues / patch swaps per output, 0.75 fragment reads per MFMA, two workgroups per CU.  Same        */
                                /* arithmetic and per-accumulator summation order as the 4-row tile.  Applied only where the layer's grid stays >= 3 such tiles per CU       */
                                /* (smaller grids are cut into K-ranges either way and lose); bit 30 forces it on every eligible layer (tests).  Default 0x3ffff.            */
                                /* The conv-transposes and the stride-2 layers take the 8 x 16-pixel tile under the same bit and rule (convt_halo8_x3_kernel: four            */
                                /* accumulators per wave; conv_halo8_s2_x3_kernel: 9 x 17-pixel unit patches)                                                               */
#define MSI_NET_OPT_X3_ROWPAR 17 /* fp32 plans, bit i = layer i: a stride-1, RATE-2 layer on the split (F32_SPLIT3) whose input height is a multiple of 8 runs on ROW-PARITY  */
                                 /* tiles: a tile's four rows are every other image row (tile row t = 2 t' + parity -> rows 8 t' + parity + 2 r), so along H a dilation-2 tap */
                                 /* is the NEXT tile row -- a 6 x 20-pixel patch instead of 8 x 20, the two-stage weight ring and three workgroups per CU instead of two.      */
                                 /* Same arithmetic and summation order per output element (bit-identical to the plain rate-2 tile).  Default 0x3ffff                         */
#define MSI_NET_OPT_COUNT 18
int msi_net_plan_create(const msi_net_desc *desc, msi_net_plan **out_plan);
void msi_net_plan_destroy(msi_net_plan *plan);
int msi_net_plan_set_option(msi_net_plan *plan, int32_t option, int32_t value);
size_t msi_net_plan_workspace_bytes(const msi_net_plan *plan);
/* After a forward, does workspace[raw_offset of `layer`] hold the layer's LayerNorm + ReLU'd activation (1) or its raw
 * convolution output (0: every consumer applies the LayerNorm itself while loading -- the head, halo-patch layers)?
 * -1: bad arguments.  (Tests / debugging; the frame loop does not need it.) */
int32_t msi_net_plan_layer_is_normalized(const msi_net_plan *plan, int32_t layer);
/* Which kernel instantiation the plan launches for `layer` (0 .. MSI_NET_NUM_LAYERS-1), written to name[name_bytes] as
 * rocprofv3 spells it without the namespace -- e.g. "conv_halo_s2_kernel<1>", "conv_halo_bf16_kernel<128, 128, 1, 1, 8>",
 * "conv_igemm_kernel<64, 64, 1, 0>" (<BM, BN, MODE 0 conv / 1 conv-transpose / 2 head, BF16>); *nblocks = workgroups of the
 * launch, *nsplit_tiles = tiles cut into K-ranges (both optional).  The choice depends on batch x tiles against the CU
 * count, so a parity test at a bench batch asserts with this that the variants it checked are the ones the bench times
 * (color_pred reports the stand-alone head; msi_net_plan_forward_rgba replaces it by head_assemble_kernel). */
int32_t msi_net_plan_layer_kernel(const msi_net_plan *plan, int32_t layer, char *name, size_t name_bytes, int32_t *nblocks,
                                  int32_t *nsplit_tiles);
/* The launch parameters the plan holds for `layer`, as opaque bytes (tests of the planner hash them: a refactor of the planner
 * must leave them unchanged): the kernel argument with its pointers null, then inlaunch, fuse_ln, skip_apply, ln_blocks as four
 * int32.  *needed = their size (optional); out may be NULL to ask for it, else out[bytes] must hold them.  The layout is the
 * library's own and may change between builds. */
int32_t msi_net_plan_layer_params(const msi_net_plan *plan, int32_t layer, void *out, size_t bytes, size_t *needed);
/* Health of the LAST forward that ran with `workspace` on `stream` (synchronises the stream: call it after a frame,
 * not inside the frame loop's hot path): MSI_OK, or MSI_E_RANGE with the reason in msi_last_error_string when a
 * LayerNorm sum overflowed its fixed-point window (bit 1 of *status_bits: raw outputs > ~3000x the scale the weights
 * predict, or non-finite input; bf16 plans also set it when a raw output may have left the range of the fp16 it is
 * stored in -- some |x 2^-e - pivot| of a wave's 1 024 values above 32 752, i.e. > ~1000x that scale) or a variance fell below its resolution (bit 2: < ~1e-3 of that scale, or a constant
 * layer).  status_bits may be NULL.  The word is reset by the next forward. */
#define MSI_NET_STATUS_APPLY_AHEAD_TIMEOUT 1 /* bit 0: no kernel sets it any more (the number stays taken) */
#define MSI_NET_STATUS_LN_OVERFLOW 2
#define MSI_NET_STATUS_LN_UNDERFLOW 4
#define MSI_NET_STATUS_F16_SPLIT_RANGE 8 /* an operand of a layer on the fp16 split (F32_SPLIT_F16) exceeded 65504: rerun with that option 0 */
int32_t msi_net_plan_status(const msi_net_plan *plan, const void *workspace, msi_stream_t stream, int32_t *status_bits);
/* LayerNorm window calibration (round 5).  The fixed-point window of a layer's LayerNorm sums (MSI_NET_STATUS_LN_*) follows an exponent the packer
 * estimates from the weights; a checkpoint whose trained gamma / beta / weights put a layer's raw output far from that estimate would end every forward in
 * MSI_E_RANGE.  msi_net_plan_calibrate measures instead: layer by layer it runs the network on `net_input` (a representative frame, device memory, the
 * forward's layout), moves / centres each layer's window on the measured raw rms and rewrites the four scale doubles at ln_scale_offset of `packed`
 * (DEVICE memory, modified in place; every plan that shares the blob sees the new windows).  Blocking (it synchronises `stream` several times per layer),
 * a one-off of a few dozen forwards; *layers_changed (may be NULL) = layers whose exponent moved.  MSI_E_RANGE if a layer has no finite, non-constant output.
 * ALL OR NOTHING (round 6): on ANY error return every window is written back as it was on entry.  Within a batch the window is centred on the samples it
 * resolves; a constant sample among others is left out (a forward flags it itself). */
int32_t msi_net_plan_calibrate(const msi_net_plan *plan, float *packed, const void *net_input, void *workspace, size_t workspace_bytes,
                               msi_stream_t stream, int32_t *layers_changed);
/* net_input [B,H,W,in_channels] (fp32, or bf16 when desc.dtype = MSI_DTYPE_BF16) -> pred [B,H,W,num_outputs] fp32. */
int msi_net_plan_forward(const msi_net_plan *plan, const float *packed, const void *net_input, float *pred,
                         void *workspace, size_t workspace_bytes, msi_stream_t stream);

/* The network followed by infer_msi's layer_prediction for which_color_pred = blend_psv (msi.py:130-147) with the
 * 1x1 head, its source's LayerNorm and the RGBA assembly fused into ONE kernel: `pred` never exists in HBM.
 * net_input [B,H,W,6D] (fp32, or bf16 for a bf16 plan) is both the network input and the sweep volume the layers are
 * blended from; rgba_native [B,D,H,W,4] fp32; blend_weights / alphas [B,H,W,D] and pred [B,H,W,2D] (the tanh output)
 * are optional (NULL).  fp32 plans: bit-identical to msi_net_plan_forward + msi_assemble_rgba_f32.  bf16 plans: the
 * head runs on the fp32 MFMA over the same bf16-rounded operands (activation rounded where ln_apply rounds it, weights
 * rounded at pack time), so it equals the two-step bf16 path up to the fp32 summation order; conv8_2 then has no
 * ln_apply launch and no bf16 copy.  event_after_convs: optional hipEvent_t recorded on `stream` between the last
 * convolution and the fused tail (bench.py times the MFMA-bound and the HBM-bound part separately).
 * MSI_E_UNSUPPORTED for other colour schemes / ngf > 64 / D > 64 / HEAD_FUSE_LN = 0: use msi_net_plan_forward +
 * msi_assemble_rgba_color_f32 there. */
int msi_net_plan_forward_rgba(const msi_net_plan *plan, const float *packed, const void *net_input, float *rgba_native,
                              float *blend_weights, float *alphas, float *pred, void *workspace, size_t workspace_bytes,
                              msi_stream_t stream, void *event_after_convs);

/* msi_net_plan_forward_rgba with the layer stack emitted in a compact format (MSI_LAYERS_RGBA8 / MSI_LAYERS_RGBA16F, see
 * msi_pack_layers) straight from the fused tail: the kernel encodes the fp32 texel it has just blended and stores 4 or 8
 * bytes instead of 16, so a consumer that keeps, stores or renders packed stacks (msi_render_views_packed) never has an
 * fp32 stack in memory and runs no msi_pack_layers pass.
 *   layers_out   [B,D,H,W] texels of `format`, 16-byte aligned, or NULL.  `format` must be MSI_LAYERS_RGBA8 or
 *                MSI_LAYERS_RGBA16F when layers_out is non-NULL and is ignored when it is NULL.
 *   rgba_native  [B,D,H,W,4] fp32, or NULL.  At least one of rgba_native and layers_out is non-NULL; with both, ONE launch
 *                writes both stacks.
 *   every other argument as in msi_net_plan_forward_rgba.
 * CONTRACT: layers_out is bit-identical to msi_pack_layers(format) applied to the rgba_native that
 * msi_net_plan_forward_rgba writes for the same plan and input, for fp32 plans and for bf16 plans; rgba_native,
 * blend_weights, alphas and pred, when requested, are bit-identical to msi_net_plan_forward_rgba's.
 * Argument checks, in this order: unknown format with a non-NULL layers_out -> MSI_E_BADARG ("unknown format"); both
 * outputs NULL -> MSI_E_BADARG ("null pointer") -- neither needs a plan or a device; then the checks of
 * msi_net_plan_forward_rgba (NULL plan -> MSI_E_BADARG, MSI_E_UNSUPPORTED under exactly its conditions: assemble the fp32
 * stack with msi_assemble_rgba_color_f32 and pack it with msi_pack_layers there).  Error texts name net_forward_layers.
 * A plan of batch 0 returns MSI_OK without a launch.  With layers_out = NULL the call IS msi_net_plan_forward_rgba (the
 * same kernel, head_assemble_kernel); with a layers_out the tail runs as head_assemble_packed_kernel<BF16, format>. */
int msi_net_plan_forward_layers(const msi_net_plan *plan, const float *packed, const void *net_input, float *rgba_native,
                                void *layers_out, int32_t format, float *blend_weights, float *alphas, float *pred,
                                void *workspace, size_t workspace_bytes, msi_stream_t stream, void *event_after_convs);

/* Descriptor-level convenience: the two calls below build a transient plan per call (set-up time, tests); the
 * frame loop uses msi_net_plan_forward.
 * net_input [B,H,W,in_channels] -> pred [B,H,W,num_outputs]. */
int msi_net_forward_f32(const msi_net_desc *desc, const float *packed, const float *net_input,
                        float *pred, void *workspace, size_t workspace_bytes,
                        msi_stream_t stream);
/* BASELINE configs[2] (bf16): desc->dtype = MSI_DTYPE_BF16.  net_input [B,H,W,in_channels] bf16
 * (msi_ods_sphere_sweep_bf16 writes it), weights and activations bf16 (round to nearest even),
 * products accumulated in fp32 on v_mfma_f32_32x32x16_bf16, LayerNorm statistics and affine in
 * fp32 on the fp32 accumulators, pred [B,H,W,num_outputs] fp32.  in_channels and ngf must be
 * multiples of 8.  The packed blob (same size query / packer, keyed by desc->dtype) holds bf16
 * weights and fp32 gamma / beta / bias. */
int msi_net_forward_bf16(const msi_net_desc *desc, const float *packed, const void *net_input_bf16,
                         float *pred, void *workspace, size_t workspace_bytes,
                         msi_stream_t stream);

#ifdef __cplusplus
}
#endif
#endif /* MSI_HIP_H */
