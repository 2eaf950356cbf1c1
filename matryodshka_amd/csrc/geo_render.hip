// K4 of the geometry side, fused reprojection + wrap-around bilinear gather + over-composite: render_kernel (one view per sample: equirect, ODS,
// perspective crop), render_views_kernel (many views of one stack per launch) and render_views_packed_kernel (the same from an rgba8 / rgba16f
// stack; the decoders are in geometry_device.h, shared with unpack_layers_kernel); kernels first, their C ABI entry points below.
#include "geometry_device.h"

namespace {

// ------------------------------------------------------------------------ K4
// One thread per target pixel, 64x4-pixel tiles (a wavefront = 64 consecutive
// columns, so each tap row is a ~1 KiB coalesced float4 segment and vertically
// adjacent waves share tap rows in L1).  The ray/sphere quadratic's a and b do
// not depend on the layer, so per layer only sqrt, one divide and the two atan2
// remain; the running composite lives in registers and every texel of the
// D x H x W x 4 stack is fetched from HBM once.  (RenderMode, DepthFrac and the layer descriptors / taps: geometry_device.h, shared with the MPI render.)
constexpr int RENDER_SEGS = 4;   // layer segments per pixel (threads in y)
// ray model of the TARGET view: equirect (spherical.intersect_sphere, spherical.py:268-326),
// ODS eye (intersect_ods, :328-365) or the hard-coded perspective crop (intersect_perspective, :367-401)
enum RayModel { RAY_EQUIRECT = 0, RAY_ODS = 1, RAY_PERSPECTIVE = 2 };

struct RayParams {
  int out_h, out_w;        // target image size (== layer size except for RAY_PERSPECTIVE)
  float order;             // RAY_ODS: +1 left eye / -1 right eye
  float s0, sstep, t0, tstep;  // RAY_PERSPECTIVE: uv_grid = tf.linspace(-1+1/n, 1-1/n, n) (spherical.py:46-48)
};

template <int MODE, int RAY>
__global__ void __launch_bounds__(256)
render_kernel(const float4 *__restrict__ rgba, const float *__restrict__ pose_rt,
              const float *__restrict__ tgt_pos, const float *__restrict__ intrinsics,
              const float *__restrict__ depths, const float *__restrict__ trig, int batch, int height,
              int width, int nd, float *__restrict__ out_rgb, float *__restrict__ out_depth,
              float4 *__restrict__ out_layers, PixConsts K, RayParams R, DepthFrac F, int *__restrict__ status) {
  // block = 64 pixels of one target row x RENDER_SEGS layer segments: a pixel's D layers are split over RENDER_SEGS
  // threads (same lane, different waves), each compositing its contiguous range of layers from transparent black,
  //   C <- rgb a + C (1-a),   T <- T (1-a),
  // and the segments are combined back to front, out = C_3 + T_3 (C_2 + T_2 (C_1 + T_1 C_0)) (the over operator is
  // associative; rounding differs from the strictly sequential form by ~1e-7).  One thread per pixel left the chip with
  // 3 200 wavefronts for 8 192 wave slots and a 32-deep chain of dependent-latency gathers per thread.
  // 1-D grid, XCD-aware: workgroup ids go round-robin over the 8 XCDs and each XCD has its own L2, so XCD x takes the
  // x-th eighth of the (sample, row, 64-pixel block) sequence, in order: vertically adjacent target rows -- which share
  // their bilinear tap rows -- are gathered through the SAME L2 (with rows dealt round-robin every tap row was fetched
  // by two XCDs: 2.3x the stack's bytes at D = 64, batch 16; 1.43x at the BASELINE size)
  const unsigned gx = (unsigned)(R.out_w + 63) >> 6;
  const unsigned nblk = gx * (unsigned)R.out_h * (unsigned)batch, per = gridDim.x >> 3;
  const unsigned lin = (blockIdx.x & 7u) * per + (blockIdx.x >> 3);
  if (lin >= nblk) return;                        // (grid rounded up to a multiple of 8; whole workgroups leave)
  const unsigned rowb = lin / gx;
  const int j_raw = (int)(lin - rowb * gx) * 64 + threadIdx.x;
  const int b = (int)(rowb / (unsigned)R.out_h);
  const int i = (int)(rowb - (unsigned)b * (unsigned)R.out_h);
  // (a wavefront is one threadIdx.y: telling the compiler keeps the layer index -- and with it the per-layer buffer
  // descriptor -- in SGPRs; without it every gather sat in a readfirstlane waterfall loop, ~12 instructions each)
  const int seg = __builtin_amdgcn_readfirstlane(threadIdx.y);
  const bool valid = j_raw < R.out_w;
  const int j = valid ? j_raw : R.out_w - 1;      // (lanes past the row end compute a duplicate and store nothing: no early return before the barrier)
  __shared__ float s_part[RENDER_SEGS][64][5];

  float rx, ry, rz, cx, cy, cz;
  if (RAY == RAY_PERSPECTIVE) {
    // spherical.py:381-392: rx = S*0.1, ry = T*0.05, rz = -0.05; centre (c0, c1, -c2)
    const float S = R.s0 + R.sstep * (float)j, T = R.t0 + R.tstep * (float)i;
    rx = S * 0.1f; ry = T * 0.05f; rz = -1.0f * 0.05f;
    const float *tp = tgt_pos + (size_t)b * 3;
    cx = tp[0]; cy = tp[1]; cz = -tp[2];
  } else {
    const float cs = trig[j], ss = trig[width + j];
    const float ct = trig[2 * width + i], st = trig[2 * width + height + i];
    if (RAY == RAY_ODS) {
      // spherical.py:349-358: ray (cosS cosT, sinT, -sinS cosT) from the viewing circle
      const float bl = intrinsics[(size_t)b * 9];
      rx = cs * ct; ry = st; rz = (-ss) * ct;
      cx = ((-ss) * bl) * R.order; cy = 0.0f; cz = ((-cs) * bl) * R.order;
    } else {
      // spherical.py:280-288: ray (cosS cosT, sinT, sinS cosT); origin = tgt_pos with x<->z swapped
      rx = cs * ct; ry = st; rz = ss * ct;
      const float *tp = tgt_pos + (size_t)b * 3;
      cx = tp[2]; cy = tp[1]; cz = tp[0];
    }
  }
  const float *P = pose_rt + (size_t)b * 16;
  {
    const float x = (P[0] * rx + P[1] * ry) + P[2] * rz;
    const float y = (P[4] * rx + P[5] * ry) + P[6] * rz;
    const float z = (P[8] * rx + P[9] * ry) + P[10] * rz;
    rx = x; ry = y; rz = z;
  }
  // ray origin through the full 4x4 (spherical.py:303-310 / transform_ray :70-94)
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

  const size_t hw = (size_t)height * width;             // source layer size
  const int layer_bytes = (int)(hw * 16);                // (H * W < 2^24, checked on the host)
  const size_t ohw = (size_t)R.out_h * R.out_w;          // target size
  const size_t pix = (size_t)i * R.out_w + j;
  float o0 = 0.f, o1 = 0.f, o2 = 0.f, od = 0.f, tr = 1.f;
  float qc_max = -1.0f;                                  // max over this thread's layers of |origin|^2 - radius^2 (>= 0: origin not inside that sphere)
  const int d_lo = (seg * nd) / RENDER_SEGS, d_hi = ((seg + 1) * nd) / RENDER_SEGS;

#pragma unroll 4
  for (int d = d_lo; d < d_hi; ++d) {
    const float radius = depths[d];
    const float qc = cc - radius * radius;
    qc_max = fmaxf(qc_max, qc);
    const float disc = qb2 - fa * qc;
    // disc >= 0 whenever the ray origin is inside the sphere (the documented domain; the host-side guard of the MSI class
    // enforces it for host inputs).  Outside it the reference takes sqrt of a negative number and casts NaN to int
    // (undefined); the clamp keeps device-side inputs finite and changes nothing inside the domain.
    // (no branch of the reference depends on these values: the whole chain is continuous -> 1-ulp primitives)
#if MSI_FAST_TAIL
    const float num = t_sqrt(fmaxf(disc, 0.0f)) - qb;           // t = num / ta with the pixel's 1 / ta (one correction step: <= 1 ulp)
    const float tq = num * inv_ta;
    const float t = __builtin_fmaf(__builtin_fmaf(-tq, ta, num), inv_ta, tq);
#else
    const float t = t_div(-qb + t_sqrt(fmaxf(disc, 0.0f)), ta);
#endif
    const float x = cx + t * rx;
    const float y = cy + t * ry;
    const float z = cz + t * rz;
    // project_spherical (spherical.py:243-246) + theta_phi_to_pixels (:54-68); the point lies on the layer's sphere: |P| = radius
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
    // one descriptor per layer (scalar work): 32-bit texel offsets also for stacks beyond 2 GiB
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
      if (valid) out_layers[((size_t)d * batch + b) * ohw + pix] = o;
    }
    if (MODE & RENDER_RGB) {
      const float r = blend4(tp4, A.x, Bv.x, C.x, Dv.x);
      const float g = blend4(tp4, A.y, Bv.y, C.y, Dv.y);
      const float bl = blend4(tp4, A.z, Bv.z, C.z, Dv.z);
      if (d == 0) {  // projector.py:259-260: the farthest layer's alpha is ignored
        o0 = r; o1 = g; o2 = bl;
      } else {       // projector.py:262-263
        const float om = 1.0f - al;
        o0 = r * al + o0 * om;
        o1 = g * al + o1 * om;
        o2 = bl * al + o2 * om;
      }
    }
    if (MODE & RENDER_DEPTH) {
      if (d == 0) {
        od = 0.0f;   // projector.py:239-240
      } else {       // projector.py:242: (i / len) * alpha + output * (1 - alpha)
        const float frac = nd <= DEPTH_FRAC_MAX ? F.f[d] : (float)((double)d / (double)nd);
        od = frac * al + od * (1.0f - al);
      }
    }
    tr = tr * (1.0f - al);
  }
  // the ray origin of this sample is not inside every sphere it was intersected with: outside the reference's domain
  // (spherical.py:316-318 takes the square root of a negative number there); the clamp above kept the pixels finite, the
  // status word says so (one lane per wave; the origin is a property of the sample, so all lanes agree)
  // (fmaxf drops NaNs: a NaN pose / target position makes cc NaN and leaves qc_max at -1 -- tested separately)
  if (status != nullptr && threadIdx.x == 0 && (!(qc_max < 0.0f) || cc != cc)) atomicOr(status, MSI_RENDER_STATUS_ORIGIN_OUTSIDE);
  if (MODE & RENDER_LAYERS) return;            // (nothing to combine)
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
    float *o = out_rgb + ((size_t)b * ohw + pix) * 3;
    o[0] = o0; o[1] = o1; o[2] = o2;
  }
  if (MODE & RENDER_DEPTH) {
    float *o = out_depth + ((size_t)b * ohw + pix) * 3;
    o[0] = od; o[1] = od; o[2] = od;
  }
}

// K4, many views of one stack per launch (msi_render_views_f32): render_kernel's per-layer arithmetic, op for op, for V target
// cameras per sample.  A workgroup is one (sample, view, target row, 64-pixel block); the 1-D grid runs sample -> view -> row
// -> block with render_kernel's XCD-aware mapping, so the V views of one stack follow each other (its texels stay in the
// Infinity Cache while they render) and adjacent rows of one view share an XCD's L2.  The pose, origin and K of a view are
// wave-uniform (scalar loads).  Rays before the pose:
//   MSI_CAMERA_EQUIRECT  (cos S cos T, sin T, sin S cos T) on the lat-long grid of the OUTPUT size (trig = its table)
//   MSI_CAMERA_PINHOLE   (1, (i + 0.5 - cy) / fy, (j + 0.5 - cx) / fx): forward +x, image-down +y, image-right +z -- the
//                        orientation of the equirect render around its centre pixel
// and the origin is pose @ (tgt_pos[2], tgt_pos[1], tgt_pos[0], 1) for both.  Outputs rgb [B,V,h,w,3] and depth [B,V,h,w].
template <int MODE, int CAMERA>
__global__ void __launch_bounds__(256)
render_views_kernel(const float4 *__restrict__ rgba, const float *__restrict__ pose_rt, const float *__restrict__ tgt_pos,
                    const float *__restrict__ intrinsics, const float *__restrict__ depths, const float *__restrict__ trig,
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
  const int j = valid ? j_raw : out_w - 1;
  __shared__ float s_part[RENDER_SEGS][64][5];

  float rx, ry, rz;
  if (CAMERA == MSI_CAMERA_PINHOLE) {
    const float *Kv = intrinsics + (size_t)bv * 9;      // fx . cx / . fy cy
    rx = 1.0f;
    ry = (((float)i + 0.5f) - Kv[5]) / Kv[4];            // (IEEE divides: per pixel, not per layer)
    rz = (((float)j + 0.5f) - Kv[2]) / Kv[0];
  } else {
    const float cs = trig[j], ss = trig[out_w + j];
    const float ct = trig[2 * out_w + i], st = trig[2 * out_w + out_h + i];
    rx = cs * ct; ry = st; rz = ss * ct;
  }
  const float *tp = tgt_pos + (size_t)bv * 3;
  float cx = tp[2], cy = tp[1], cz = tp[0];
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
  const int layer_bytes = (int)(hw * 16);
  const size_t pix = (size_t)bv * out_h * out_w + (size_t)i * out_w + j;
  float o0 = 0.f, o1 = 0.f, o2 = 0.f, od = 0.f, tr = 1.f;
  float qc_max = -1.0f;
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
    const __amdgpu_buffer_rsrc_t L = layer_rsrc(rgba, b, nd, d, hw, layer_bytes);
    const float4 A = layer_tap(L, tp4.oa), Bv = layer_tap(L, tp4.ob), C = layer_tap(L, tp4.oc), Dv = layer_tap(L, tp4.od);
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
  // (as render_kernel: the origin of this view is not inside every sphere, or is NaN)
  if (status != nullptr && threadIdx.x == 0 && (!(qc_max < 0.0f) || cc != cc)) atomicOr(status, MSI_RENDER_STATUS_ORIGIN_OUTSIDE);
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
  // (a wave's 64 pixels are one contiguous 768-byte rgb run and one 256-byte depth run)
  if (MODE & RENDER_RGB) {
    float *o = out_rgb + pix * 3;
    o[0] = o0; o[1] = o1; o[2] = o2;
  }
  if (MODE & RENDER_DEPTH) out_depth[pix] = od;
}

// K4 from a compact stack (msi_render_views_packed; the formats and their exact rule are in msi_hip.h): a sibling of
// render_views_kernel with the texel format of the stack as FMT (MSI_LAYERS_RGBA8 or MSI_LAYERS_RGBA16F; the fp32 kernel above
// stays as it is, instruction for instruction).  A tap is ONE 4-byte (rgba8: buffer_load_dword) or 8-byte (rgba16f:
// buffer_load_dwordx2) load through the same per-layer descriptor, with layer_bytes and the texel shift scaled to the format,
// decoded to the four fp32 values msi_unpack_layers writes for that texel (rgba8: 11 VALU per tap -- four v_cvt_f32_ubyte, three
// subtracts, four multiplies; rgba16f: four v_cvt_f32_f16).  Everything after the decode is render_views_kernel's arithmetic,
// op for op, so a render from a packed stack is bit-identical to msi_render_views_f32 on the unpacked one.
template <int MODE, int CAMERA, int FMT>
__global__ void __launch_bounds__(256)
render_views_packed_kernel(const void *__restrict__ layers, const float *__restrict__ pose_rt, const float *__restrict__ tgt_pos,
                           const float *__restrict__ intrinsics, const float *__restrict__ depths, const float *__restrict__ trig,
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
  const int j = valid ? j_raw : out_w - 1;
  __shared__ float s_part[RENDER_SEGS][64][5];

  float rx, ry, rz;
  if (CAMERA == MSI_CAMERA_PINHOLE) {
    const float *Kv = intrinsics + (size_t)bv * 9;      // fx . cx / . fy cy
    rx = 1.0f;
    ry = (((float)i + 0.5f) - Kv[5]) / Kv[4];            // (IEEE divides: per pixel, not per layer)
    rz = (((float)j + 0.5f) - Kv[2]) / Kv[0];
  } else {
    const float cs = trig[j], ss = trig[out_w + j];
    const float ct = trig[2 * out_w + i], st = trig[2 * out_w + out_h + i];
    rx = cs * ct; ry = st; rz = ss * ct;
  }
  const float *tp = tgt_pos + (size_t)bv * 3;
  float cx = tp[2], cy = tp[1], cz = tp[0];
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
  const int layer_bytes = (int)(hw << TexelShift<FMT>::value);
  const size_t pix = (size_t)bv * out_h * out_w + (size_t)i * out_w + j;
  float o0 = 0.f, o1 = 0.f, o2 = 0.f, od = 0.f, tr = 1.f;
  float qc_max = -1.0f;
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
    const __amdgpu_buffer_rsrc_t L = packed_layer_rsrc<FMT>(layers, b, nd, d, hw, layer_bytes);
    const float4 A = packed_layer_tap<FMT>(L, tp4.oa), Bv = packed_layer_tap<FMT>(L, tp4.ob), C = packed_layer_tap<FMT>(L, tp4.oc), Dv = packed_layer_tap<FMT>(L, tp4.od);
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
  // (as render_kernel: the origin of this view is not inside every sphere, or is NaN)
  if (status != nullptr && threadIdx.x == 0 && (!(qc_max < 0.0f) || cc != cc)) atomicOr(status, MSI_RENDER_STATUS_ORIGIN_OUTSIDE);
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
  // (a wave's 64 pixels are one contiguous 768-byte rgb run and one 256-byte depth run)
  if (MODE & RENDER_RGB) {
    float *o = out_rgb + pix * 3;
    o[0] = o0; o[1] = o1; o[2] = o2;
  }
  if (MODE & RENDER_DEPTH) out_depth[pix] = od;
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
  const long nblk = (long)((R.out_w + 63) / 64) * R.out_h * batch;
  MSI_REQUIRE(nblk < (1L << 31) - 8, "render: too many target pixels for one launch");
  const dim3 grid((unsigned)((nblk + 7) / 8 * 8)), block(64, RENDER_SEGS);
  const PixConsts K = make_consts(height, width);
  const float4 *src = reinterpret_cast<const float4 *>(rgba_native);
  float4 *lay = reinterpret_cast<float4 *>(out_layers);
  hipStream_t s = msi::as_stream(stream);
  DepthFrac F;
  for (int d = 0; d < DEPTH_FRAC_MAX; ++d) F.f[d] = d < num_planes ? (float)((double)d / (double)num_planes) : 0.0f;
#define MSI_LAUNCH_RENDER(M, RY)                                                                       \
  hipLaunchKernelGGL((render_kernel<M, RY>), grid, block, 0, s, src, pose, tgt_pos, intrinsics, depths, \
                     trig, batch, height, width, num_planes, out_rgb, out_depth, lay, K, R, F, status)
  if (ray == RAY_EQUIRECT) {
    switch (mode) {
      case RENDER_RGB: MSI_LAUNCH_RENDER(RENDER_RGB, RAY_EQUIRECT); break;
      case RENDER_DEPTH: MSI_LAUNCH_RENDER(RENDER_DEPTH, RAY_EQUIRECT); break;
      case RENDER_RGB | RENDER_DEPTH: MSI_LAUNCH_RENDER(RENDER_RGB | RENDER_DEPTH, RAY_EQUIRECT); break;
      case RENDER_LAYERS: MSI_LAUNCH_RENDER(RENDER_LAYERS, RAY_EQUIRECT); break;
      default: return msi::fail(MSI_E_BADARG, "render: bad mode %d", mode);
    }
  } else if (ray == RAY_ODS) {
    MSI_LAUNCH_RENDER(RENDER_RGB, RAY_ODS);
  } else {
    MSI_LAUNCH_RENDER(RENDER_RGB, RAY_PERSPECTIVE);
  }
#undef MSI_LAUNCH_RENDER
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
  const int mode = (out_rgb ? RENDER_RGB : 0) | (out_depth ? RENDER_DEPTH : 0);
  return render_common(mode, RAY_EQUIRECT, rgba_native, tgt_pose_rt, tgt_pos, nullptr, depths, trig, batch, height,
                       width, num_planes, same_size(height, width), out_rgb, out_depth, nullptr, status_device, stream);
}

// msi_render_views_f32 and msi_render_views_packed: one set of checks and one launch table (`who` names the entry point in the
// error text; `format` is one of MSI_LAYERS_*, already validated by the caller).
static int render_views_launch(const char *who, const void *layers, int32_t format, const float *tgt_pose_rt, const float *tgt_pos,
                               const float *intrinsics, const float *depths, const float *trig,
                               int32_t batch, int32_t views, int32_t height, int32_t width, int32_t num_planes,
                               int32_t camera, int32_t out_height, int32_t out_width,
                               float *out_rgb, float *out_depth, int32_t *status_device, msi_stream_t stream) {
  MSI_REQUIRE(out_rgb || out_depth, "%s: both outputs are NULL", who);
  MSI_REQUIRE(layers && tgt_pose_rt && tgt_pos && depths, "%s: null pointer", who);
  MSI_REQUIRE(camera == MSI_CAMERA_EQUIRECT || camera == MSI_CAMERA_PINHOLE, "%s: unknown camera %d", who, camera);
  MSI_REQUIRE(camera != MSI_CAMERA_EQUIRECT || trig, "%s: null pointer (equirect camera needs trig)", who);
  MSI_REQUIRE(camera != MSI_CAMERA_PINHOLE || intrinsics, "%s: null pointer (pinhole camera needs intrinsics)", who);
  MSI_REQUIRE(batch >= 0 && height > 0 && width > 0 && num_planes > 0, "%s: bad dims", who);
  MSI_REQUIRE(views >= 1, "%s: views must be >= 1 (got %d)", who, views);
  const int min_out = camera == MSI_CAMERA_PINHOLE ? 2 : 1;
  MSI_REQUIRE(out_height >= min_out && out_width >= min_out, "%s: bad output size %d x %d", who, out_height, out_width);
  MSI_REQUIRE((long)height * width < (1L << 24), "%s: layers of more than 2^24 texels (24-bit texel offsets)", who);
  const long lim = (1L << 31) - 8;
  long nblk = (long)((out_width + 63) / 64) * out_height;     // (each factor < 2^31: checked before every product)
  MSI_REQUIRE(nblk < lim, "%s: too many target pixels for one launch", who);
  nblk *= views;
  MSI_REQUIRE(nblk < lim, "%s: too many target pixels for one launch", who);
  nblk *= batch;
  MSI_REQUIRE(nblk < lim, "%s: too many target pixels for one launch", who);
  if (batch == 0) return MSI_OK;
  const dim3 grid((unsigned)((nblk + 7) / 8 * 8)), block(64, RENDER_SEGS);
  const PixConsts K = make_consts(height, width);
  DepthFrac F;
  for (int d = 0; d < DEPTH_FRAC_MAX; ++d) F.f[d] = d < num_planes ? (float)((double)d / (double)num_planes) : 0.0f;
  const int mode = (out_rgb ? RENDER_RGB : 0) | (out_depth ? RENDER_DEPTH : 0);
  hipStream_t s = msi::as_stream(stream);
#define MSI_VIEWS_ARGS tgt_pose_rt, tgt_pos, intrinsics, depths, trig, batch, views, height, width, num_planes, out_height, out_width, \
                       out_rgb, out_depth, K, F, status_device
#define MSI_LAUNCH_VIEWS(M, CAM)                                                                                                        \
  switch (format) {                                                                                                                     \
    case MSI_LAYERS_RGBA8:                                                                                                              \
      hipLaunchKernelGGL((render_views_packed_kernel<M, CAM, MSI_LAYERS_RGBA8>), grid, block, 0, s, layers, MSI_VIEWS_ARGS); break;     \
    case MSI_LAYERS_RGBA16F:                                                                                                            \
      hipLaunchKernelGGL((render_views_packed_kernel<M, CAM, MSI_LAYERS_RGBA16F>), grid, block, 0, s, layers, MSI_VIEWS_ARGS); break;   \
    default:                                                                                                                            \
      hipLaunchKernelGGL((render_views_kernel<M, CAM>), grid, block, 0, s, static_cast<const float4 *>(layers), MSI_VIEWS_ARGS); break; \
  }
#define MSI_LAUNCH_VIEWS_M(CAM)                                                     \
  switch (mode) {                                                                   \
    case RENDER_RGB: MSI_LAUNCH_VIEWS(RENDER_RGB, CAM); break;                      \
    case RENDER_DEPTH: MSI_LAUNCH_VIEWS(RENDER_DEPTH, CAM); break;                  \
    default: MSI_LAUNCH_VIEWS(RENDER_RGB | RENDER_DEPTH, CAM); break;               \
  }
  if (camera == MSI_CAMERA_PINHOLE) {
    MSI_LAUNCH_VIEWS_M(MSI_CAMERA_PINHOLE)
  } else {
    MSI_LAUNCH_VIEWS_M(MSI_CAMERA_EQUIRECT)
  }
#undef MSI_LAUNCH_VIEWS_M
#undef MSI_LAUNCH_VIEWS
#undef MSI_VIEWS_ARGS
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
  MSI_REQUIRE(format == MSI_LAYERS_F32 || format == MSI_LAYERS_RGBA8 || format == MSI_LAYERS_RGBA16F,
              "render_views_packed: unknown format %d", format);
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
