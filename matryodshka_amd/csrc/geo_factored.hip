// The viewer of a FACTORED high-res stack: msi_render_views_factored -- K4, the sphere render of geometry_device.h (sphere_views_body: the body of
// render_views_kernel, geo_render.hip, and of render_ods_views_kernel, geo_ods.hip), reading each tap of the [B,D,H,W,4] stack msi_hres_layers
// would have built from that stack's inputs instead (FactoredSphereStack, geometry_device.h).  No stack is allocated, written or read: a frame is
// the two high-res images and the two low-res [B,h,w,D] tensors -- at 4096 x 2048 x 32 over 640 x 320, 254 MB against 4.3 GB -- and every output
// element compares == to msi_render_views_f32 / msi_render_ods_views on the stack msi_hres_layers writes from the same arguments.
// The price is arithmetic: a tap is two ODS projections and eight image loads where the stack render has one 16-byte load, four taps per layer.
#include "geometry_device.h"

namespace {

// One kernel per output mode and camera (view_ray's three).  Grid and block are render_views_launch's: a workgroup is 64 pixels of one target row x
// RENDER_SEGS layer segments.  K: the constants of the STACK size -- the render's (sphere_uv) and the sweep's (ods_tail) are the same struct.
// Registers: the four taps of a layer keep up to 32 image texels in flight; the allocation is the compiler's unless MSI_FACTORED_WAVES asks for an
// occupancy (profiles/hres_factored_isa.txt, profiles/hres_factored_timing.txt).
#ifndef MSI_FACTORED_WAVES   // (tuning: -DMSI_FACTORED_WAVES=3 / 4 waves per SIMD; 0: the compiler's choice)
#define MSI_FACTORED_WAVES 0
#endif
#if MSI_FACTORED_WAVES
#define MSI_FACTORED_OCCUPANCY __attribute__((amdgpu_waves_per_eu(MSI_FACTORED_WAVES, MSI_FACTORED_WAVES)))
#else
#define MSI_FACTORED_OCCUPANCY
#endif
template <int MODE, int CAMERA>
__global__ void __launch_bounds__(256) MSI_FACTORED_OCCUPANCY
render_views_factored_kernel(const float *__restrict__ image0, const float *__restrict__ image1, const float *__restrict__ pose0,
                             const float *__restrict__ pose1, const float *__restrict__ stack_intrinsics, const float *__restrict__ depths,
                             const float *__restrict__ stack_trig, const float *__restrict__ blend_weights, const float *__restrict__ alphas,
                             int low_h, int low_w, float sy, float sx, const float *__restrict__ pose_rt, const float *__restrict__ tgt_pos,
                             const float *__restrict__ intrinsics, const float *__restrict__ eye_radius, const float *__restrict__ trig,
                             int batch, int views, int height, int width, int nd, int out_h, int out_w, float *__restrict__ out_rgb,
                             float *__restrict__ out_depth, PixConsts K, DepthFrac F, int *__restrict__ status) {
  const auto stack = [&](int b) {
    const size_t low_base = (size_t)b * low_h * low_w * nd;          // (h * w * D < 2^31: checked on the host)
    return FactoredSphereStack{image0, image1, pose0, pose1, stack_intrinsics, depths, stack_trig, blend_weights + low_base, alphas + low_base,
                               b, nd, height, width, low_h, low_w, sy, sx};
  };
  sphere_views_body<MODE, CAMERA>(stack, pose_rt, tgt_pos, intrinsics, eye_radius, trig, batch, views, nd, out_h, out_w, out_rgb, out_depth, K, F,
                                  status);
}

}  // namespace

extern "C" {

int msi_render_views_factored(const float *ref_image, const float *src_image, const float *ref_curr_pose, const float *src_curr_pose,
                              const float *intrinsics, const float *depths, const float *trig, const float *blend_weights, const float *alphas,
                              int32_t batch, int32_t low_height, int32_t low_width, int32_t height, int32_t width, int32_t num_planes,
                              const float *tgt_pose_rt, const float *tgt_pos, const float *view_intrinsics, const float *eye_radius,
                              const float *view_trig, int32_t views, int32_t camera, int32_t out_height, int32_t out_width, float *out_rgb,
                              float *out_depth, int32_t *status_device, msi_stream_t stream) {
  const char *who = "render_views_factored";
  if (const int e = hres_check(who, ref_image && src_image && ref_curr_pose && src_curr_pose && intrinsics && depths && trig && blend_weights &&
                               alphas, batch, low_height, low_width, height, width, num_planes)) return e;
  const ViewArgs a = {who, out_rgb, out_depth, tgt_pose_rt && tgt_pos, MSI_LAYERS_F32, ANY_FORMAT, "", &camera, view_trig, view_intrinsics,
                      eye_radius, true, (long)height * width, views, batch, out_height, out_width, 1};
  unsigned grid;
  if (const int e = check_views(a, no_check, no_check, &grid)) return e;
  if (batch == 0) return MSI_OK;
  const float sy = hres_scale(low_height, height), sx = hres_scale(low_width, width);
  const PixConsts K = make_consts(height, width);
  const DepthFrac F = depth_fractions(num_planes);
  hipStream_t s = msi::as_stream(stream);
  const auto launch = [&](auto M, auto CAM, auto) {   // (no texel format: the factors are fp32)
    hipLaunchKernelGGL((render_views_factored_kernel<decltype(M)::value, decltype(CAM)::value>), dim3(grid), dim3(64, RENDER_SEGS), 0, s, ref_image,
                       src_image, ref_curr_pose, src_curr_pose, intrinsics, depths, trig, blend_weights, alphas, low_height, low_width, sy, sx,
                       tgt_pose_rt, tgt_pos, view_intrinsics, eye_radius, view_trig, batch, views, height, width, num_planes, out_height, out_width,
                       out_rgb, out_depth, K, F, status_device);
  };
  for_view_kernel(render_mode(out_rgb, out_depth), MSI_LAYERS_F32, eye_radius != nullptr, camera, launch);
  return msi::check_launch(who);
}

}  // extern "C"
