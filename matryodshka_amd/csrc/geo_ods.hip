// K4 with the ODS stereo camera (msi_render_ods_views): render_ods_views_kernel, the sphere render of geometry_device.h (the body of
// render_views_kernel, geo_render.hip) with the ray origin on the viewing circle instead of at one point per view; the kernel first, its C ABI
// entry point below.
#include "geometry_device.h"

namespace {

// K4, both eyes (or any V ODS views) of one stack per launch.  The camera is render_views_kernel's equirect camera with the ray
// origin moved onto the viewing circle of the view: on the lat-long grid of the OUTPUT size (trig = its table), before the pose,
//   direction  r = (cos S cos T, sin T, sin S cos T)                                       -- the equirect camera's
//   origin     c = (tgt_pos[2] + sin S * e, tgt_pos[1], tgt_pos[0] + (-cos S) * e)         -- e = eye_radius[b*V + v], signed:
//                                                                                             e > 0 the left eye (the reference's order = +1)
// (sin S, 0, -cos S) . r = 0: the ray is tangent to the circle of radius |e| around the head position.  Then as every view:
// apply_pose and the per-layer step of every sphere render -- with e = 0 the origin is tgt_pos + (+-0) and the render has the bits of the equirect camera.
// Column j is column W-1-j of render_kernel<RAY_ODS>'s image (msi_render_ods_f32 keeps the reference's mirrored order), i.e. this
// one is upright like every other render here.  What differs from render_views_kernel: e is one scalar load, but the origin -- and
// with it cc, qb and qc -- is per lane, so NO lane can speak for the wave in the status word: every lane tests its own origin, the
// wave votes, and lane 0 issues the one atomicOr.
template <int MODE, int FMT>
__global__ void __launch_bounds__(256)
render_ods_views_kernel(const void *__restrict__ layers, const float *__restrict__ pose_rt, const float *__restrict__ tgt_pos,
                        const float *__restrict__ eye_radius, const float *__restrict__ depths, const float *__restrict__ trig,
                        int batch, int views, int height, int width, int nd, int out_h, int out_w, float *__restrict__ out_rgb,
                        float *__restrict__ out_depth, PixConsts K, DepthFrac F, int *__restrict__ status) {
  SphereBlock s(out_h, out_w, views, batch);
  if (s.past_end()) return;
  s.decode(views, out_w);
  const unsigned bv = s.bv;
  const int i = s.i, j = s.j;

  const float cs = trig[j], ss = trig[out_w + j];
  const float ct = trig[2 * out_w + i], st = trig[2 * out_w + out_h + i];
  ViewRay r;
  r.rx = cs * ct; r.ry = st; r.rz = ss * ct;
  const float *tp = tgt_pos + (size_t)bv * 3;
  const float e = eye_radius[bv];
  r.cx = tp[2] + ss * e; r.cy = tp[1]; r.cz = tp[0] + (-cs) * e;
  apply_pose(pose_rt + (size_t)bv * 16, r);
  const SphereQuad q = sphere_quad(r);
  const SphereStack<FMT> S(layers, depths, s.b, nd, height, width);
  const size_t pix = (size_t)bv * out_h * out_w + (size_t)i * out_w + j;
  float o0 = 0.f, o1 = 0.f, o2 = 0.f, od = 0.f, tr = 1.f;
  float qc_max = -1.0f;
#pragma unroll 4
  for (int d = S.first(s.seg); d < S.end(s.seg); ++d) {
    const auto t = S.layer(d, r, q, K, qc_max);
    qc_max = t.qc_max;
    const Composite n = over_step<MODE>(o0, o1, o2, od, tr, d, t.c, [&] { return depth_frac(F, d, nd); });
    o0 = n.o0; o1 = n.o1; o2 = n.o2; od = n.od; tr = n.tr;
  }
  // The origin is a property of the LANE here (a point of the viewing circle): a circle that crosses the innermost sphere is
  // outside the domain for some columns only, so every lane tests its own, the wave votes, and one lane issues one atomicOr per
  // wave.  (Lanes past the row end vote with the last pixel's origin, which a stored lane of this row has too.)
  if (status != nullptr) {
    const bool any = __builtin_amdgcn_ballot_w64(!(qc_max < 0.0f) || q.cc != q.cc) != 0;   // (wave-uniform)
    if (any && threadIdx.x == 0) atomicOr(status, MSI_RENDER_STATUS_ORIGIN_OUTSIDE);
  }
  sphere_combine(s, o0, o1, o2, od, tr,
                 [&](float o0, float o1, float o2, float od) { store_pixel<MODE>(out_rgb, out_depth, pix, o0, o1, o2, od); });
}

}  // namespace

extern "C" {

int msi_render_ods_views(const void *layers, int32_t format, const float *tgt_pose_rt, const float *tgt_pos,
                         const float *eye_radius, const float *depths, const float *trig,
                         int32_t batch, int32_t views, int32_t height, int32_t width, int32_t num_planes,
                         int32_t out_height, int32_t out_width,
                         float *out_rgb, float *out_depth, int32_t *status_device, msi_stream_t stream) {
  MSI_REQUIRE(out_rgb || out_depth, "render_ods_views: both outputs are NULL");
  MSI_REQUIRE(layers && tgt_pose_rt && tgt_pos && eye_radius && depths && trig, "render_ods_views: null pointer");
  MSI_REQUIRE(format == MSI_LAYERS_F32 || format == MSI_LAYERS_RGBA8 || format == MSI_LAYERS_RGBA16F,
              "render_ods_views: unknown format %d", format);
  MSI_REQUIRE(batch >= 0 && height > 0 && width > 0 && num_planes > 0, "render_ods_views: bad dims");
  MSI_REQUIRE(views >= 1, "render_ods_views: views must be >= 1 (got %d)", views);
  MSI_REQUIRE(out_height >= 1 && out_width >= 1, "render_ods_views: bad output size %d x %d", out_height, out_width);
  MSI_REQUIRE((long)height * width < (1L << 24), "render_ods_views: layers of more than 2^24 texels (24-bit texel offsets)");
  unsigned grid;
  if (const int e = view_grid("render_ods_views", (long)((out_width + 63) / 64) * out_height, views, batch, &grid)) return e;
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
