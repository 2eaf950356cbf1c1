// K4 with the ODS stereo camera (msi_render_ods_views): render_ods_views_kernel, the many-views sphere render of geometry_device.h
// (render_views_body, the body of render_views_kernel too) with view_ray's CAMERA_ODS -- the ray origin on the viewing circle instead of at one
// point per view; the convention is stated there.  The kernel first, its C ABI entry point below.
#include "geometry_device.h"

namespace {

// K4, both eyes (or any V ODS views) of one stack per launch, from an fp32 or a packed stack.
template <int MODE, int FMT>
__global__ void __launch_bounds__(256)
render_ods_views_kernel(const void *__restrict__ layers, const float *__restrict__ pose_rt, const float *__restrict__ tgt_pos,
                        const float *__restrict__ eye_radius, const float *__restrict__ depths, const float *__restrict__ trig,
                        int batch, int views, int height, int width, int nd, int out_h, int out_w, float *__restrict__ out_rgb,
                        float *__restrict__ out_depth, PixConsts K, DepthFrac F, int *__restrict__ status) {
  render_views_body<MODE, CAMERA_ODS, FMT>(layers, pose_rt, tgt_pos, nullptr, eye_radius, depths, trig, batch, views, height, width, nd, out_h,
                                           out_w, out_rgb, out_depth, K, F, status);
}

}  // namespace

extern "C" {

int msi_render_ods_views(const void *layers, int32_t format, const float *tgt_pose_rt, const float *tgt_pos,
                         const float *eye_radius, const float *depths, const float *trig,
                         int32_t batch, int32_t views, int32_t height, int32_t width, int32_t num_planes,
                         int32_t out_height, int32_t out_width,
                         float *out_rgb, float *out_depth, int32_t *status_device, msi_stream_t stream) {
  const ViewArgs a = {"render_ods_views", out_rgb, out_depth, layers && tgt_pose_rt && tgt_pos && eye_radius && depths && trig, format, ANY_FORMAT,
                      "", nullptr, nullptr, nullptr, nullptr, batch >= 0 && height > 0 && width > 0 && num_planes > 0, (long)height * width,
                      views, batch, out_height, out_width, 1};
  unsigned grid;
  if (const int e = check_views(a, no_check, no_check, &grid)) return e;
  if (batch == 0) return MSI_OK;
  const dim3 block(64, RENDER_SEGS);
  const PixConsts K = make_consts(height, width);
  const DepthFrac F = depth_fractions(num_planes);
  hipStream_t s = msi::as_stream(stream);
  for_mode(render_mode(out_rgb, out_depth), [&](auto M) { for_format(format, [&](auto FMT) {
    hipLaunchKernelGGL((render_ods_views_kernel<decltype(M)::value, decltype(FMT)::value>), dim3(grid), block, 0, s, layers, tgt_pose_rt, tgt_pos,
                       eye_radius, depths, trig, batch, views, height, width, num_planes, out_height, out_width, out_rgb, out_depth, K, F,
                       status_device);
  }); });
  return msi::check_launch("render_ods_views");
}

}  // extern "C"
