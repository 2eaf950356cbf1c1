// K4 of the geometry side, fused reprojection + wrap-around bilinear gather + over-composite: render_kernel (one view per sample: equirect, ODS,
// perspective crop), render_views_kernel (many views of one stack per launch) and render_views_packed_kernel (the same from an rgba8 / rgba16f
// stack; the decoders are in geometry_device.h, shared with unpack_layers_kernel); kernels first, their C ABI entry points below.
#include "geometry_device.h"

namespace {

// ------------------------------------------------------------------------ K4
// The kernels are built from the sphere-render pieces of geometry_device.h (SphereBlock: the workgroup shape and the XCD-aware grid; apply_pose,
// sphere_quad, sphere_uv: the per-layer geometry; SphereStack::layer: the per-layer step; over_step; sphere_combine: the segment combine).
// ray model of the TARGET view: equirect (spherical.intersect_sphere, spherical.py:268-326),
// ODS eye (intersect_ods, :328-365) or the hard-coded perspective crop (intersect_perspective, :367-401)
enum RayModel { RAY_EQUIRECT = 0, RAY_ODS = 1, RAY_PERSPECTIVE = 2 };

struct RayParams {
  int out_h, out_w;        // target image size (== layer size except for RAY_PERSPECTIVE)
  float order;             // RAY_ODS: +1 left eye / -1 right eye
  float s0, sstep, t0, tstep;  // RAY_PERSPECTIVE: uv_grid = tf.linspace(-1+1/n, 1-1/n, n) (spherical.py:46-48)
};

// One view per sample, with the reference's three ray models; besides the composite (rgb and the reference's three-channel depth, [B,h,w,3]
// each) it can write every reprojected layer instead (RENDER_LAYERS: out_layers [D,B,h,w,4], nothing to combine).
template <int MODE, int RAY>
__global__ void __launch_bounds__(256)
render_kernel(const float4 *__restrict__ rgba, const float *__restrict__ pose_rt,
              const float *__restrict__ tgt_pos, const float *__restrict__ intrinsics,
              const float *__restrict__ depths, const float *__restrict__ trig, int batch, int height,
              int width, int nd, float *__restrict__ out_rgb, float *__restrict__ out_depth,
              float4 *__restrict__ out_layers, PixConsts K, RayParams R, DepthFrac F, int *__restrict__ status) {
  SphereBlock s(R.out_h, R.out_w, 1, batch);
  if (s.past_end()) return;                       // (grid rounded up to a multiple of 8; whole workgroups leave)
  s.decode(1, R.out_w);
  const int b = s.b, i = s.i, j = s.j;

  ViewRay r;
  if (RAY == RAY_PERSPECTIVE) {
    // spherical.py:381-392: rx = S*0.1, ry = T*0.05, rz = -0.05; centre (c0, c1, -c2)
    const float S = R.s0 + R.sstep * (float)j, T = R.t0 + R.tstep * (float)i;
    r.rx = S * 0.1f; r.ry = T * 0.05f; r.rz = -1.0f * 0.05f;
    const float *tp = tgt_pos + (size_t)b * 3;
    r.cx = tp[0]; r.cy = tp[1]; r.cz = -tp[2];
  } else {
    const float cs = trig[j], ss = trig[width + j];
    const float ct = trig[2 * width + i], st = trig[2 * width + height + i];
    if (RAY == RAY_ODS) {
      // spherical.py:349-358: ray (cosS cosT, sinT, -sinS cosT) from the viewing circle
      const float bl = intrinsics[(size_t)b * 9];
      r.rx = cs * ct; r.ry = st; r.rz = (-ss) * ct;
      r.cx = ((-ss) * bl) * R.order; r.cy = 0.0f; r.cz = ((-cs) * bl) * R.order;
    } else {
      // spherical.py:280-288: ray (cosS cosT, sinT, sinS cosT); origin = tgt_pos with x<->z swapped
      r.rx = cs * ct; r.ry = st; r.rz = ss * ct;
      const float *tp = tgt_pos + (size_t)b * 3;
      r.cx = tp[2]; r.cy = tp[1]; r.cz = tp[0];
    }
  }
  apply_pose(pose_rt + (size_t)b * 16, r);
  const SphereQuad q = sphere_quad(r);

  // The gathers and the over-composite step are this kernel's own text (SphereStack::layer's and over_step's arithmetic): written with them, not
  // every instantiation keeps the instruction stream that bench.py times (profiles/shared_render_pieces_isa.txt).
  const size_t hw = (size_t)height * width;             // source layer size
  const int layer_bytes = (int)(hw * 16);                // (H * W < 2^24, checked on the host)
  const size_t ohw = (size_t)R.out_h * R.out_w;          // target size
  const size_t pix = (size_t)i * R.out_w + j;
  float o0 = 0.f, o1 = 0.f, o2 = 0.f, od = 0.f, tr = 1.f;
  float qc_max = -1.0f;                                  // max over this thread's layers of |origin|^2 - radius^2 (>= 0: origin not inside that sphere)
  const int d_lo = (s.seg * nd) / RENDER_SEGS, d_hi = ((s.seg + 1) * nd) / RENDER_SEGS;

#pragma unroll 4
  for (int d = d_lo; d < d_hi; ++d) {
    const SphereUv p = sphere_uv(depths[d], r, q, K);
    qc_max = fmaxf(qc_max, p.qc);
    const TapsR tp4 = make_taps_ranged(p.u, p.v, width, height);
    const __amdgpu_buffer_rsrc_t L = __builtin_amdgcn_make_buffer_rsrc((void *)(rgba + ((size_t)b * nd + d) * hw), 0, layer_bytes, 0x00020000);
    typedef unsigned u32x4_g __attribute__((ext_vector_type(4)));
    const float4 A = __builtin_bit_cast(float4, (u32x4_g)__builtin_amdgcn_raw_buffer_load_b128(L, tp4.oa << 4, 0, 0));
    const float4 Bv = __builtin_bit_cast(float4, (u32x4_g)__builtin_amdgcn_raw_buffer_load_b128(L, tp4.ob << 4, 0, 0));
    const float4 C = __builtin_bit_cast(float4, (u32x4_g)__builtin_amdgcn_raw_buffer_load_b128(L, tp4.oc << 4, 0, 0));
    const float4 Dv = __builtin_bit_cast(float4, (u32x4_g)__builtin_amdgcn_raw_buffer_load_b128(L, tp4.od << 4, 0, 0));
    const float al = blend4(tp4, A.w, Bv.w, C.w, Dv.w);
    if (MODE & RENDER_LAYERS) {
      float4 o;
      o.x = blend4(tp4, A.x, Bv.x, C.x, Dv.x);
      o.y = blend4(tp4, A.y, Bv.y, C.y, Dv.y);
      o.z = blend4(tp4, A.z, Bv.z, C.z, Dv.z);
      o.w = al;
      if (s.valid) out_layers[((size_t)d * batch + b) * ohw + pix] = o;
    }
    if (MODE & RENDER_RGB) {
      const float cr = blend4(tp4, A.x, Bv.x, C.x, Dv.x);
      const float cg = blend4(tp4, A.y, Bv.y, C.y, Dv.y);
      const float cb = blend4(tp4, A.z, Bv.z, C.z, Dv.z);
      if (d == 0) {
        o0 = cr; o1 = cg; o2 = cb;
      } else {
        const float om = 1.0f - al;
        o0 = cr * al + o0 * om;
        o1 = cg * al + o1 * om;
        o2 = cb * al + o2 * om;
      }
    }
    if (MODE & RENDER_DEPTH) {
      if (d == 0) {
        od = 0.0f;
      } else {
        const float frac = nd <= DEPTH_FRAC_MAX ? F.f[d] : (float)((double)d / (double)nd);
        od = frac * al + od * (1.0f - al);
      }
    }
    tr = tr * (1.0f - al);
  }
  // (one lane per wave; the origin is a property of the sample, so all lanes agree)
  if (status != nullptr && threadIdx.x == 0 && (!(qc_max < 0.0f) || q.cc != q.cc)) atomicOr(status, MSI_RENDER_STATUS_ORIGIN_OUTSIDE);
  if (MODE & RENDER_LAYERS) return;            // (nothing to combine)
  sphere_combine(s, o0, o1, o2, od, tr, [&](float o0, float o1, float o2, float od) {
    if (MODE & RENDER_RGB) {
      float *o = out_rgb + ((size_t)b * ohw + pix) * 3;
      o[0] = o0; o[1] = o1; o[2] = o2;
    }
    if (MODE & RENDER_DEPTH) {
      float *o = out_depth + ((size_t)b * ohw + pix) * 3;
      o[0] = od; o[1] = od; o[2] = od;
    }
  });
}

// Many views of one stack per launch (msi_render_views_f32 / msi_render_views_packed): render_views_body (geometry_device.h) under two kernel
// names; the fp32 kernel keeps the name the profiles know it by.
template <int MODE, int CAMERA>
__global__ void __launch_bounds__(256)
render_views_kernel(const float4 *__restrict__ rgba, const float *__restrict__ pose_rt, const float *__restrict__ tgt_pos,
                    const float *__restrict__ intrinsics, const float *__restrict__ depths, const float *__restrict__ trig,
                    int batch, int views, int height, int width, int nd, int out_h, int out_w, float *__restrict__ out_rgb,
                    float *__restrict__ out_depth, PixConsts K, DepthFrac F, int *__restrict__ status) {
  render_views_body<MODE, CAMERA, MSI_LAYERS_F32>(rgba, pose_rt, tgt_pos, intrinsics, nullptr, depths, trig, batch, views, height, width, nd, out_h,
                                                  out_w, out_rgb, out_depth, K, F, status);
}

// FMT = MSI_LAYERS_RGBA8 or MSI_LAYERS_RGBA16F (the formats and their exact rule are in msi_hip.h)
template <int MODE, int CAMERA, int FMT>
__global__ void __launch_bounds__(256)
render_views_packed_kernel(const void *__restrict__ layers, const float *__restrict__ pose_rt, const float *__restrict__ tgt_pos,
                           const float *__restrict__ intrinsics, const float *__restrict__ depths, const float *__restrict__ trig,
                           int batch, int views, int height, int width, int nd, int out_h, int out_w, float *__restrict__ out_rgb,
                           float *__restrict__ out_depth, PixConsts K, DepthFrac F, int *__restrict__ status) {
  render_views_body<MODE, CAMERA, FMT>(layers, pose_rt, tgt_pos, intrinsics, nullptr, depths, trig, batch, views, height, width, nd, out_h, out_w,
                                       out_rgb, out_depth, K, F, status);
}

}  // namespace

extern "C" {

static int render_common(int mode, int ray, const float *rgba_native, const float *pose, const float *tgt_pos,
                         const float *intrinsics, const float *depths, const float *trig, int32_t batch,
                         int32_t height, int32_t width, int32_t num_planes, RayParams R, float *out_rgb,
                         float *out_depth, float *out_layers, int32_t *status, msi_stream_t stream) {
  MSI_REQUIRE(rgba_native && pose && depths, "render: null pointer");
  MSI_REQUIRE(batch >= 0 && height > 0 && width > 0 && num_planes > 0 && R.out_h > 0 && R.out_w > 0,
              "render: bad dims");
  MSI_REQUIRE((long)height * width < (1L << 24), "render: layers of more than 2^24 texels (24-bit texel offsets)");
  if (batch == 0) return MSI_OK;
  unsigned grid;
  if (const int e = view_grid("render", (long)((R.out_w + 63) / 64) * R.out_h, 1, batch, &grid)) return e;
  const dim3 block(64, RENDER_SEGS);
  const PixConsts K = make_consts(height, width);
  const float4 *src = reinterpret_cast<const float4 *>(rgba_native);
  float4 *lay = reinterpret_cast<float4 *>(out_layers);
  hipStream_t s = msi::as_stream(stream);
  const DepthFrac F = depth_fractions(num_planes);
  auto launch = [&](auto M, auto RY) {
    hipLaunchKernelGGL((render_kernel<decltype(M)::value, decltype(RY)::value>), dim3(grid), block, 0, s, src, pose, tgt_pos, intrinsics, depths,
                       trig, batch, height, width, num_planes, out_rgb, out_depth, lay, K, R, F, status);
  };
  if (ray == RAY_EQUIRECT) {
    if (mode == RENDER_LAYERS) launch(Const<RENDER_LAYERS>{}, Const<RAY_EQUIRECT>{});
    else if (mode == RENDER_RGB || mode == RENDER_DEPTH || mode == (RENDER_RGB | RENDER_DEPTH)) for_mode(mode, [&](auto M) { launch(M, Const<RAY_EQUIRECT>{}); });
    else return msi::fail(MSI_E_BADARG, "render: bad mode %d", mode);
  } else if (ray == RAY_ODS) {
    launch(Const<RENDER_RGB>{}, Const<RAY_ODS>{});
  } else {
    launch(Const<RENDER_RGB>{}, Const<RAY_PERSPECTIVE>{});
  }
  return msi::check_launch("render");
}

static RayParams same_size(int32_t height, int32_t width) {
  RayParams R;
  R.out_h = height; R.out_w = width; R.order = 1.0f;
  R.s0 = R.sstep = R.t0 = R.tstep = 0.0f;
  return R;
}

int msi_render_equirect_f32(const float *rgba_native, const float *tgt_pose_rt,
                            const float *tgt_pos, const float *depths, const float *trig,
                            int32_t batch, int32_t height, int32_t width, int32_t num_planes,
                            float *out_rgb, float *out_depth, int32_t *status_device, msi_stream_t stream) {
  MSI_REQUIRE(out_rgb || out_depth, "render_equirect: both outputs are NULL");
  MSI_REQUIRE(tgt_pos && trig, "render_equirect: null pointer");
  return render_common(render_mode(out_rgb, out_depth), RAY_EQUIRECT, rgba_native, tgt_pose_rt, tgt_pos, nullptr, depths, trig, batch, height,
                       width, num_planes, same_size(height, width), out_rgb, out_depth, nullptr, status_device, stream);
}

// msi_render_views_f32 and msi_render_views_packed: one launch table behind the checks of every many-views entry point (`who` names the entry
// point in the error text).
static int render_views_launch(const char *who, const void *layers, int32_t format, const float *tgt_pose_rt, const float *tgt_pos,
                               const float *intrinsics, const float *depths, const float *trig,
                               int32_t batch, int32_t views, int32_t height, int32_t width, int32_t num_planes,
                               int32_t camera, int32_t out_height, int32_t out_width,
                               float *out_rgb, float *out_depth, int32_t *status_device, msi_stream_t stream) {
  const ViewArgs a = {who, out_rgb, out_depth, layers && tgt_pose_rt && tgt_pos && depths, format, ANY_FORMAT, "", &camera, trig, intrinsics, nullptr,
                      batch >= 0 && height > 0 && width > 0 && num_planes > 0, (long)height * width, views, batch, out_height, out_width, 1};
  unsigned grid;
  if (const int e = check_views(a, no_check, no_check, &grid)) return e;
  if (batch == 0) return MSI_OK;
  const dim3 block(64, RENDER_SEGS);
  const PixConsts K = make_consts(height, width);
  const DepthFrac F = depth_fractions(num_planes);
  hipStream_t s = msi::as_stream(stream);
  for_mode(render_mode(out_rgb, out_depth), [&](auto M) { for_camera(camera, [&](auto CAM) { for_format(format, [&](auto FMT) {
    constexpr int m = decltype(M)::value, cam = decltype(CAM)::value, fmt = decltype(FMT)::value;
    if constexpr (fmt == MSI_LAYERS_F32)
      hipLaunchKernelGGL((render_views_kernel<m, cam>), dim3(grid), block, 0, s, static_cast<const float4 *>(layers), tgt_pose_rt, tgt_pos, intrinsics,
                         depths, trig, batch, views, height, width, num_planes, out_height, out_width, out_rgb, out_depth, K, F, status_device);
    else
      hipLaunchKernelGGL((render_views_packed_kernel<m, cam, fmt>), dim3(grid), block, 0, s, layers, tgt_pose_rt, tgt_pos, intrinsics, depths, trig,
                         batch, views, height, width, num_planes, out_height, out_width, out_rgb, out_depth, K, F, status_device);
  }); }); });
  return msi::check_launch(who);
}

int msi_render_views_f32(const float *rgba_native, const float *tgt_pose_rt, const float *tgt_pos,
                         const float *intrinsics, const float *depths, const float *trig,
                         int32_t batch, int32_t views, int32_t height, int32_t width, int32_t num_planes,
                         int32_t camera, int32_t out_height, int32_t out_width,
                         float *out_rgb, float *out_depth, int32_t *status_device, msi_stream_t stream) {
  return render_views_launch("render_views", rgba_native, MSI_LAYERS_F32, tgt_pose_rt, tgt_pos, intrinsics, depths, trig, batch, views,
                             height, width, num_planes, camera, out_height, out_width, out_rgb, out_depth, status_device, stream);
}

int msi_render_views_packed(const void *layers, int32_t format, const float *tgt_pose_rt, const float *tgt_pos,
                            const float *intrinsics, const float *depths, const float *trig,
                            int32_t batch, int32_t views, int32_t height, int32_t width, int32_t num_planes,
                            int32_t camera, int32_t out_height, int32_t out_width,
                            float *out_rgb, float *out_depth, int32_t *status_device, msi_stream_t stream) {
  return render_views_launch("render_views_packed", layers, format, tgt_pose_rt, tgt_pos, intrinsics, depths, trig, batch, views,
                             height, width, num_planes, camera, out_height, out_width, out_rgb, out_depth, status_device, stream);
}

int msi_project_layers_f32(const float *rgba_native, const float *tgt_pose_rt,
                           const float *tgt_pos, const float *depths, const float *trig,
                           int32_t batch, int32_t height, int32_t width, int32_t num_planes,
                           float *out_layers, int32_t *status_device, msi_stream_t stream) {
  MSI_REQUIRE(out_layers && tgt_pos && trig, "project_layers: null pointer");
  return render_common(RENDER_LAYERS, RAY_EQUIRECT, rgba_native, tgt_pose_rt, tgt_pos, nullptr, depths, trig, batch,
                       height, width, num_planes, same_size(height, width), nullptr, nullptr, out_layers, status_device, stream);
}

int msi_render_ods_f32(const float *rgba_native, const float *pose, const float *intrinsics,
                       const float *depths, const float *trig, int32_t batch, int32_t height,
                       int32_t width, int32_t num_planes, int32_t order, float *out_rgb, int32_t *status_device,
                       msi_stream_t stream) {
  MSI_REQUIRE(out_rgb && intrinsics && trig, "render_ods: null pointer");
  MSI_REQUIRE(order == 1 || order == -1, "render_ods: order must be +1 or -1");
  RayParams R = same_size(height, width);
  R.order = (float)order;
  return render_common(RENDER_RGB, RAY_ODS, rgba_native, pose, nullptr, intrinsics, depths, trig, batch, height,
                       width, num_planes, R, out_rgb, nullptr, nullptr, status_device, stream);
}

int msi_render_perspective_f32(const float *rgba_native, const float *pose, const float *tgt_pos,
                               const float *depths, int32_t batch, int32_t height, int32_t width,
                               int32_t num_planes, int32_t tgt_height, int32_t tgt_width, float *out_rgb,
                               int32_t *status_device, msi_stream_t stream) {
  MSI_REQUIRE(out_rgb && tgt_pos, "render_perspective: null pointer");
  MSI_REQUIRE(tgt_height > 1 && tgt_width > 1, "render_perspective: bad target size");
  RayParams R = same_size(tgt_height, tgt_width);
  const UvGrid gs = uv_grid(tgt_width), gt = uv_grid(tgt_height);
  R.s0 = gs.start; R.sstep = gs.step;
  R.t0 = gt.start; R.tstep = gt.step;
  return render_common(RENDER_RGB, RAY_PERSPECTIVE, rgba_native, pose, tgt_pos, nullptr, depths, nullptr, batch,
                       height, width, num_planes, R, out_rgb, nullptr, nullptr, status_device, stream);
}

}  // extern "C"
