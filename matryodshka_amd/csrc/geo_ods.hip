// K4 with the ODS stereo camera (msi_render_ods_views): render_ods_views_kernel, a sibling of render_views_kernel and
// render_views_packed_kernel (geo_render.hip, which stays as it is, instruction for instruction) whose ray origin sits on the
// viewing circle instead of at one point per view; the kernel first, its C ABI entry point below.
#include "geometry_device.h"

namespace {

constexpr int RENDER_SEGS = 4;   // layer segments per pixel (threads in y), as geo_render.hip

// One texel format for the three stacks render_views reads: the fp32 stack through layer_rsrc / layer_tap, the compact ones
// through their packed_ forms (geometry_device.h: ONE way to address and decode a texel for every render family).
template <int FMT> struct OdsTexel {
  static constexpr int shift = TexelShift<FMT>::value;
  static __device__ __forceinline__ __amdgpu_buffer_rsrc_t rsrc(const void *layers, int b, int nd, int d, size_t hw, int layer_bytes) {
    return packed_layer_rsrc<FMT>(layers, b, nd, d, hw, layer_bytes);
  }
  static __device__ __forceinline__ float4 tap(__amdgpu_buffer_rsrc_t L, unsigned texel) { return packed_layer_tap<FMT>(L, texel); }
};
template <> struct OdsTexel<MSI_LAYERS_F32> {
  static constexpr int shift = 4;
  static __device__ __forceinline__ __amdgpu_buffer_rsrc_t rsrc(const void *layers, int b, int nd, int d, size_t hw, int layer_bytes) {
    return layer_rsrc(static_cast<const float4 *>(layers), b, nd, d, hw, layer_bytes);
  }
  static __device__ __forceinline__ float4 tap(__amdgpu_buffer_rsrc_t L, unsigned texel) { return layer_tap(L, texel); }
};

// K4, both eyes (or any V ODS views) of one stack per launch.  The camera is render_views_kernel's equirect camera with the ray
// origin moved onto the viewing circle of the view: on the lat-long grid of the OUTPUT size (trig = its table), before the pose,
//   direction  r = (cos S cos T, sin T, sin S cos T)                                       -- the equirect camera's
//   origin     c = (tgt_pos[2] + sin S * e, tgt_pos[1], tgt_pos[0] + (-cos S) * e)         -- e = eye_radius[b*V + v], signed:
//                                                                                             e > 0 the left eye (the reference's order = +1)
// (sin S, 0, -cos S) . r = 0: the ray is tangent to the circle of radius |e| around the head position.  Then as every view:
// r <- pose[:3,:3] r, c <- pose (c, 1), and render_views_kernel's per-layer arithmetic, op for op -- with e = 0 the origin is
// tgt_pos + (+-0) and the render has the bits of the equirect camera.  Column j is column W-1-j of render_kernel<RAY_ODS>'s image
// (msi_render_ods_f32 keeps the reference's mirrored order), i.e. this one is upright like every other render here.
// Same 64 x RENDER_SEGS workgroup, same XCD-aware 1-D grid in sample -> view -> row -> block order, same segment combine and
// stores.  What differs: e is one scalar load, but the origin -- and with it cc, qb and qc -- is per lane, so NO lane can speak
// for the wave in the status word: every lane tests its own origin, the wave votes, and lane 0 issues the one atomicOr.
template <int MODE, int FMT>
__global__ void __launch_bounds__(256)
render_ods_views_kernel(const void *__restrict__ layers, const float *__restrict__ pose_rt, const float *__restrict__ tgt_pos,
                        const float *__restrict__ eye_radius, const float *__restrict__ depths, const float *__restrict__ trig,
                        int batch, int views, int height, int width, int nd, int out_h, int out_w, float *__restrict__ out_rgb,
                        float *__restrict__ out_depth, PixConsts K, DepthFrac F, int *__restrict__ status) {
  const unsigned gx = (unsigned)(out_w + 63) >> 6;
  const unsigned nblk = gx * (unsigned)out_h * (unsigned)views * (unsigned)batch, per = gridDim.x >> 3;
  const unsigned lin = (blockIdx.x & 7u) * per + (blockIdx.x >> 3);
  if (lin >= nblk) return;
  const unsigned rowb = lin / gx;
  const int j_raw = (int)(lin - rowb * gx) * 64 + threadIdx.x;
  const unsigned bv = rowb / (unsigned)out_h;           // sample * views + view
  const int i = (int)(rowb - bv * (unsigned)out_h);
  const int b = (int)(bv / (unsigned)views);
  const int seg = __builtin_amdgcn_readfirstlane(threadIdx.y);
  const bool valid = j_raw < out_w;
  const int j = valid ? j_raw : out_w - 1;              // (lanes past the row end: duplicates of the last pixel, no store)
  __shared__ float s_part[RENDER_SEGS][64][5];

  const float cs = trig[j], ss = trig[out_w + j];
  const float ct = trig[2 * out_w + i], st = trig[2 * out_w + out_h + i];
  float rx = cs * ct, ry = st, rz = ss * ct;
  const float *tp = tgt_pos + (size_t)bv * 3;
  const float e = eye_radius[bv];
  float cx = tp[2] + ss * e, cy = tp[1], cz = tp[0] + (-cs) * e;
  const float *P = pose_rt + (size_t)bv * 16;
  {
    const float x = (P[0] * rx + P[1] * ry) + P[2] * rz;
    const float y = (P[4] * rx + P[5] * ry) + P[6] * rz;
    const float z = (P[8] * rx + P[9] * ry) + P[10] * rz;
    rx = x; ry = y; rz = z;
  }
  {
    const float x = ((P[0] * cx + P[1] * cy) + P[2] * cz) + P[3] * 1.0f;
    const float y = ((P[4] * cx + P[5] * cy) + P[6] * cz) + P[7] * 1.0f;
    const float z = ((P[8] * cx + P[9] * cy) + P[10] * cz) + P[11] * 1.0f;
    cx = x; cy = y; cz = z;
  }
  const float qa = (rx * rx + ry * ry) + rz * rz;
  const float qb = 2.0f * ((rx * cx + ry * cy) + rz * cz);
  const float cc = (cx * cx + cy * cy) + cz * cz;
  const float qb2 = qb * qb;
  const float fa = 4.0f * qa, ta = 2.0f * qa;
  const float inv_ta = __builtin_amdgcn_rcpf(ta);

  const size_t hw = (size_t)height * width;
  const int layer_bytes = (int)(hw << OdsTexel<FMT>::shift);   // (H * W < 2^24, checked on the host)
  const size_t pix = (size_t)bv * out_h * out_w + (size_t)i * out_w + j;
  float o0 = 0.f, o1 = 0.f, o2 = 0.f, od = 0.f, tr = 1.f;
  float qc_max = -1.0f;                                  // max over this thread's layers of |origin|^2 - radius^2
  const int d_lo = (seg * nd) / RENDER_SEGS, d_hi = ((seg + 1) * nd) / RENDER_SEGS;

#pragma unroll 4
  for (int d = d_lo; d < d_hi; ++d) {
    const float radius = depths[d];
    const float qc = cc - radius * radius;
    qc_max = fmaxf(qc_max, qc);
    const float disc = qb2 - fa * qc;
#if MSI_FAST_TAIL
    const float num = t_sqrt(fmaxf(disc, 0.0f)) - qb;
    const float tq = num * inv_ta;
    const float t = __builtin_fmaf(__builtin_fmaf(-tq, ta, num), inv_ta, tq);
#else
    const float t = t_div(-qb + t_sqrt(fmaxf(disc, 0.0f)), ta);
#endif
    const float x = cx + t * rx;
    const float y = cy + t * ry;
    const float z = cz + t * rz;
    float theta, phi;
    t_angles(x, y, z, radius, theta, phi);
#if MSI_FAST_TAIL
    const float u = ((theta + K.pi) - K.pi_over_w) * K.u_scale;
    const float v = ((phi + K.half_pi) - K.half_pi_over_h) * K.v_scale;
#else
    const float u = (((theta + K.pi) - K.pi_over_w) / K.u_den) * K.wm1;
    const float v = (((phi + K.half_pi) - K.half_pi_over_h) / K.v_den) * K.hm1;
#endif
    const TapsR tp4 = make_taps_ranged(u, v, width, height);
    const __amdgpu_buffer_rsrc_t L = OdsTexel<FMT>::rsrc(layers, b, nd, d, hw, layer_bytes);
    const float4 A = OdsTexel<FMT>::tap(L, tp4.oa), Bv = OdsTexel<FMT>::tap(L, tp4.ob), C = OdsTexel<FMT>::tap(L, tp4.oc), Dv = OdsTexel<FMT>::tap(L, tp4.od);
    const float al = blend4(tp4, A.w, Bv.w, C.w, Dv.w);
    if (MODE & RENDER_RGB) {
      const float r = blend4(tp4, A.x, Bv.x, C.x, Dv.x);
      const float g = blend4(tp4, A.y, Bv.y, C.y, Dv.y);
      const float bl = blend4(tp4, A.z, Bv.z, C.z, Dv.z);
      if (d == 0) {
        o0 = r; o1 = g; o2 = bl;
      } else {
        const float om = 1.0f - al;
        o0 = r * al + o0 * om;
        o1 = g * al + o1 * om;
        o2 = bl * al + o2 * om;
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
  // The origin is a property of the LANE here (a point of the viewing circle): a circle that crosses the innermost sphere is
  // outside the domain for some columns only, so every lane tests its own -- not strictly inside every sphere it met, or NaN
  // (fmaxf drops NaNs: a NaN origin leaves qc_max at -1) -- the wave votes, and one lane issues one atomicOr per wave.  (Lanes
  // past the row end vote with the last pixel's origin, which a stored lane of this row has too.)
  if (status != nullptr) {
    const bool outside = !(qc_max < 0.0f) || cc != cc;
    const bool any = __builtin_amdgcn_ballot_w64(outside) != 0;   // (wave-uniform)
    if (any && threadIdx.x == 0) atomicOr(status, MSI_RENDER_STATUS_ORIGIN_OUTSIDE);
  }
  s_part[seg][threadIdx.x][0] = o0; s_part[seg][threadIdx.x][1] = o1; s_part[seg][threadIdx.x][2] = o2;
  s_part[seg][threadIdx.x][3] = od; s_part[seg][threadIdx.x][4] = tr;
  __syncthreads();
  if (seg != 0 || !valid) return;
#pragma unroll
  for (int sg = 1; sg < RENDER_SEGS; ++sg) {    // back to front: segment 0 holds the farthest layers
    const float *q = s_part[sg][threadIdx.x];
    o0 = q[0] + q[4] * o0; o1 = q[1] + q[4] * o1; o2 = q[2] + q[4] * o2;
    od = q[3] + q[4] * od;
  }
  if (MODE & RENDER_RGB) {
    float *o = out_rgb + pix * 3;
    o[0] = o0; o[1] = o1; o[2] = o2;
  }
  if (MODE & RENDER_DEPTH) out_depth[pix] = od;
}

}  // namespace

extern "C" {

int msi_render_ods_views(const void *layers, int32_t format, const float *tgt_pose_rt, const float *tgt_pos,
                         const float *eye_radius, const float *depths, const float *trig,
                         int32_t batch, int32_t views, int32_t height, int32_t width, int32_t num_planes,
                         int32_t out_height, int32_t out_width,
                         float *out_rgb, float *out_depth, int32_t *status_device, msi_stream_t stream) {
  // (the checks of render_views_launch, geo_render.hip)
  MSI_REQUIRE(out_rgb || out_depth, "render_ods_views: both outputs are NULL");
  MSI_REQUIRE(layers && tgt_pose_rt && tgt_pos && eye_radius && depths && trig, "render_ods_views: null pointer");
  MSI_REQUIRE(format == MSI_LAYERS_F32 || format == MSI_LAYERS_RGBA8 || format == MSI_LAYERS_RGBA16F,
              "render_ods_views: unknown format %d", format);
  MSI_REQUIRE(batch >= 0 && height > 0 && width > 0 && num_planes > 0, "render_ods_views: bad dims");
  MSI_REQUIRE(views >= 1, "render_ods_views: views must be >= 1 (got %d)", views);
  MSI_REQUIRE(out_height >= 1 && out_width >= 1, "render_ods_views: bad output size %d x %d", out_height, out_width);
  MSI_REQUIRE((long)height * width < (1L << 24), "render_ods_views: layers of more than 2^24 texels (24-bit texel offsets)");
  const long lim = (1L << 31) - 8;
  long nblk = (long)((out_width + 63) / 64) * out_height;     // (each factor < 2^31: checked before every product)
  MSI_REQUIRE(nblk < lim, "render_ods_views: too many target pixels for one launch");
  nblk *= views;
  MSI_REQUIRE(nblk < lim, "render_ods_views: too many target pixels for one launch");
  nblk *= batch;
  MSI_REQUIRE(nblk < lim, "render_ods_views: too many target pixels for one launch");
  if (batch == 0) return MSI_OK;
  const dim3 grid((unsigned)((nblk + 7) / 8 * 8)), block(64, RENDER_SEGS);
  const PixConsts K = make_consts(height, width);
  DepthFrac F;
  for (int d = 0; d < DEPTH_FRAC_MAX; ++d) F.f[d] = d < num_planes ? (float)((double)d / (double)num_planes) : 0.0f;
  const int mode = (out_rgb ? RENDER_RGB : 0) | (out_depth ? RENDER_DEPTH : 0);
  hipStream_t s = msi::as_stream(stream);
#define MSI_LAUNCH_ODS(M, FMT)                                                                                                        \
  hipLaunchKernelGGL((render_ods_views_kernel<M, FMT>), grid, block, 0, s, layers, tgt_pose_rt, tgt_pos, eye_radius, depths, trig,   \
                     batch, views, height, width, num_planes, out_height, out_width, out_rgb, out_depth, K, F, status_device)
#define MSI_LAUNCH_ODS_M(FMT)                                                \
  switch (mode) {                                                            \
    case RENDER_RGB: MSI_LAUNCH_ODS(RENDER_RGB, FMT); break;                 \
    case RENDER_DEPTH: MSI_LAUNCH_ODS(RENDER_DEPTH, FMT); break;             \
    default: MSI_LAUNCH_ODS(RENDER_RGB | RENDER_DEPTH, FMT); break;          \
  }
  switch (format) {
    case MSI_LAYERS_RGBA8: MSI_LAUNCH_ODS_M(MSI_LAYERS_RGBA8) break;
    case MSI_LAYERS_RGBA16F: MSI_LAUNCH_ODS_M(MSI_LAYERS_RGBA16F) break;
    default: MSI_LAUNCH_ODS_M(MSI_LAYERS_F32) break;
  }
#undef MSI_LAUNCH_ODS_M
#undef MSI_LAUNCH_ODS
  return msi::check_launch("render_ods_views");
}

}  // extern "C"
