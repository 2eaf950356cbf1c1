// The cube conventions and the cube PIXEL, once, for the three cube viewers: cube_render_views_kernel and cube_render_views_seamless_kernel (geo_cube.hip) and
// cube_render_views_sparse_kernel (geo_sparse_views.hip).  Include after geometry_device.h.
//
// Conventions (include/msi_hip.h states them for callers).  The cube frame is the camera frame of face 0 (x right, y down, z forward).  Face f of
// sample b is entry 6 b + f of the native [6B,D,S,S] stack; its camera axes in the cube frame are the columns of R_f:
//   f      0 front   1 right    2 back     3 left     4 up       5 down
//   x      (1,0,0)   (0,0,-1)   (-1,0,0)   (0,0,1)    (1,0,0)    (1,0,0)
//   y      (0,1,0)   (0,1,0)    (0,1,0)    (0,1,0)    (0,0,1)    (0,0,-1)
//   z      (0,0,1)   (1,0,0)    (0,0,-1)   (-1,0,0)   (0,-1,0)   (0,1,0)
// Texel (ix, iy) of layer d of face f is the cube-frame point R_f planes[d] K^-1 (ix, iy, 1): layer d of the six faces is a cube shell of
// half-side planes[d].
//
// The pixel, in the order a kernel runs it.  Every piece takes and returns VALUES; the layer loop, the composite's accumulators, hmin, the early
// returns and the tap stage (plain, seamless, sparse) are each kernel's own (accumulators by reference or in a struct, and a loop inside a callee,
// change the instruction streams: profiles/shared_render_pieces_isa.txt, profiles/cube_pixel_pieces_isa.txt).
//   rays    cube_ray: render_views_kernel's (view_ray and apply_pose, geometry_device.h): (cos S cos T, sin T, sin S cos T) on the lat-long grid of the
//           output or (1, (i + 0.5 - cy) / fy, (j + 0.5 - cx) / fx), rotated by pose[:3,:3]; origin pose @ (tgt_pos[2], tgt_pos[1], tgt_pos[0], 1).
//           That render frame (forward +x, down +y, right +z) becomes the cube frame by swapping x and z.  Pose, origin and both cameras are
//           wave-uniform (scalar loads).  CAMERA_ODS is the equirect camera with view_ray's origin on the viewing circle, (tgt_pos[2] + sin S_j e,
//           tgt_pos[1], tgt_pos[0] - cos S_j e) before the pose, e = eye_radius[bv] read through the kernels' `intrinsics` argument (the pinhole
//           table's place: no kernel argument is added).  Its origin, and with it ox, oy, oz and bx, by, bz, is per LANE (vector registers); the
//           pose and e stay scalar.
//   shell   cube_hit.  For origin o, direction r and half-side h: t = min over the axes of (h sign(r_k) - o_k) / r_k, evaluated as
//           h / |r_k| - o_k / r_k with the two quotients per pixel (cube_ray: IEEE divides; an axis with r_k = 0 is given +inf, and fminf drops a
//           NaN), P = o + t r.  The face is the axis of the largest |P_k| with its sign (ties: z, x, y; a NaN point compares false everywhere:
//           a y face); p = R_f^T P is two selects; u = fx p_x / h + cx, v = fy p_y / h + cy with the stack camera (CubeCamera), clamped to
//           [0, hi] with fmaxf FIRST: a NaN becomes 0 BEFORE any float -> int conversion.  hi is S-1 (clamp to the edge of the chosen face) or,
//           for the seamless filter with the cube camera, S.
//   blend   cube_blend: bilinear over the four taps A (y0,x0) B (y0,x1) C (y1,x0) D (y1,x1), ((wa A + wb B) + wc C) + wd D per channel.
//   status  cube_origin_outside: the origin is not strictly inside the innermost shell (max |o_k| >= min planes) or is NaN (fmaxf drops a NaN, so
//           it is tested by itself).  Such a view ORs MSI_RENDER_STATUS_ORIGIN_OUTSIDE into *status; its pixels are finite for finite inputs (t may
//           be negative, the taps are clamped).  Who speaks is the caller's text: the origin of an equirect or pinhole view is a property of the
//           view, every lane agrees and one lane per workgroup tests; under CAMERA_ODS it is a property of the lane, every lane tests its own,
//           the wave votes and lane 0 issues one atomicOr (render_views_body's form).
#pragma once

namespace {

struct CubeRay { float dx, dy, dz, ox, oy, oz, ax, bx, ay, by, az, bz; };   // direction, origin, 1 / |r_k| and o_k / r_k: t_k = h a_k - b_k

template <int CAMERA>
__device__ __forceinline__ CubeRay cube_ray(const float *intrinsics, const float *trig, const float *tgt_pos, const float *pose_rt, unsigned bv, int i,
                                            int j, int out_h, int out_w) {
  ViewRay r = view_ray<CAMERA>(intrinsics, intrinsics, trig, tgt_pos, bv, i, j, out_h, out_w);   // (CAMERA_ODS: `intrinsics` is eye_radius)
  apply_pose(pose_rt + (size_t)bv * 16, r);
  const float dx = r.rz, dy = r.ry, dz = r.rx;           // render frame -> cube frame: x <-> z
  const float ox = r.cz, oy = r.cy, oz = r.cx;
  const float inf = __builtin_inff();
  const float ax = dx != 0.0f ? 1.0f / fabsf(dx) : inf, bx = dx != 0.0f ? ox / dx : 0.0f;
  const float ay = dy != 0.0f ? 1.0f / fabsf(dy) : inf, by = dy != 0.0f ? oy / dy : 0.0f;
  const float az = dz != 0.0f ? 1.0f / fabsf(dz) : inf, bz = dz != 0.0f ? oz / dz : 0.0f;
  return CubeRay{dx, dy, dz, ox, oy, oz, ax, bx, ay, by, az, bz};
}

struct CubeCamera { float fx, cx, fy, cy; };             // the six faces' camera of sample b: fx . cx / . fy cy of stack_intrinsics + 9 b

__device__ __forceinline__ CubeCamera cube_stack_camera(const float *stack_intrinsics, int b) {
  const float *Ks = stack_intrinsics + (size_t)b * 9;
  return CubeCamera{Ks[0], Ks[2], Ks[4], Ks[5]};
}

struct CubeHit { unsigned f; float u, v; };              // the face and the texel coordinates in it, in [0, hi]

__device__ __forceinline__ CubeHit cube_hit(const CubeRay &r, const CubeCamera &k, float h, float hi) {
  const float t = fminf(fminf(__builtin_fmaf(h, r.ax, -r.bx), __builtin_fmaf(h, r.ay, -r.by)), __builtin_fmaf(h, r.az, -r.bz));
  const float px = __builtin_fmaf(t, r.dx, r.ox), py = __builtin_fmaf(t, r.dy, r.oy), pz = __builtin_fmaf(t, r.dz, r.oz);
  const float mx = fabsf(px), my = fabsf(py), mz = fabsf(pz);
  const bool zf = mz >= mx && mz >= my;                 // ties: z, x, y
  const bool xf = !zf && mx >= my;
  const bool neg = (zf ? pz : (xf ? px : py)) < 0.0f;
  CubeHit c;
  c.f = zf ? (neg ? 2u : 0u) : (xf ? (neg ? 3u : 1u) : (neg ? 4u : 5u));
  const float qx = zf ? (neg ? -px : px) : (xf ? (neg ? pz : -pz) : px);   // p = R_f^T P
  const float qy = (zf || xf) ? py : (neg ? pz : -pz);
  const float inv_h = t_div(1.0f, h);
  c.u = fminf(fmaxf(__builtin_fmaf(qx, k.fx * inv_h, k.cx), 0.0f), hi);   // fmaxf(NaN, 0) = 0
  c.v = fminf(fmaxf(__builtin_fmaf(qy, k.fy * inv_h, k.cy), 0.0f), hi);
  return c;
}

// du, dv: the fractions of u, v above (x0, y0)
__device__ __forceinline__ float4 cube_blend(float du, float dv, const float4 &A, const float4 &B, const float4 &C, const float4 &D) {
  const float du1 = 1.0f - du, dv1 = 1.0f - dv;
  const float wa = dv1 * du1, wb = dv1 * du, wc = dv * du1, wd = dv * du;
  float4 c;
  c.w = ((wa * A.w + wb * B.w) + wc * C.w) + wd * D.w;
  c.x = ((wa * A.x + wb * B.x) + wc * C.x) + wd * D.x;
  c.y = ((wa * A.y + wb * B.y) + wc * C.y) + wd * D.y;
  c.z = ((wa * A.z + wb * B.z) + wc * C.z) + wd * D.z;
  return c;
}

// hmin: the smallest half-side the ray was intersected with (each caller's fminf over its layers)
__device__ __forceinline__ bool cube_origin_outside(const CubeRay &r, float hmin) {
  const float omax = fmaxf(fmaxf(fabsf(r.ox), fabsf(r.oy)), fabsf(r.oz));
  return !(omax < hmin) || r.ox != r.ox || r.oy != r.oy || r.oz != r.oz;
}

// msi_cube_render_views* and msi_cube_render_views_sparse*: the per-sample descriptor addresses the six faces' stacks (sparse: the sample's kept
// tiles, which are no more than its dense stacks) with one 32-bit byte offset per lane
inline int cube_sample_bytes_check(const char *who, int format, int face_size, int num_planes) {
  const int texel_bytes = format == MSI_LAYERS_F32 ? 16 : format == MSI_LAYERS_RGBA16F ? 8 : 4;
  MSI_REQUIRE(face_size < (1 << 15) && (long)face_size * face_size * 6 * num_planes * texel_bytes < (1L << 31),   // (< 2^30 * 6 * 128 * 16)
              "%s: a sample's six face stacks (6 x %d x %d x %d texels of %d bytes) reach 2^31 bytes (32-bit offsets)", who, num_planes, face_size,
              face_size, texel_bytes);
  return MSI_OK;
}

}  // namespace
