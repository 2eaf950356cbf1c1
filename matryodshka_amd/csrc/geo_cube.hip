// The cube-map viewer of the PP path (no reference counterpart): cube_render_views_kernel renders V views per sample from SIX face stacks in one
// launch, equirect_to_cube_kernel cuts a panorama into the six face images the PP network takes; kernels first, their C ABI entry points below.
//
// Conventions (include/msi_hip.h states them for callers).  The cube frame is the camera frame of face 0 (x right, y down, z forward).  Face f of
// sample b is entry 6 b + f of the native [6B,D,S,S] stack; its camera axes in the cube frame are the columns of R_f:
//   f      0 front   1 right    2 back     3 left     4 up       5 down
//   x      (1,0,0)   (0,0,-1)   (-1,0,0)   (0,0,1)    (1,0,0)    (1,0,0)
//   y      (0,1,0)   (0,1,0)    (0,1,0)    (0,1,0)    (0,0,1)    (0,0,-1)
//   z      (0,0,1)   (1,0,0)    (0,0,-1)   (-1,0,0)   (0,-1,0)   (0,1,0)
// Texel (ix, iy) of layer d of face f is the cube-frame point R_f planes[d] K^-1 (ix, iy, 1): layer d of the six faces is a cube shell of
// half-side planes[d].
#include "geometry_device.h"

namespace {

// One thread per target pixel, the whole far-to-near composite in that thread (strictly sequential, as mpi_render_views_kernel: layer 0
// replaces, then c a + acc (1 - a)); a workgroup is 64 x 4 pixels of one (sample, view), a wave one row.
//   grid    1-D, sample -> view -> 4-row group -> 64-pixel block with the XCD-aware mapping of every many-views render (ViewBlock, geometry_device.h): the views of one cube follow each
//           other through the Infinity Cache and adjacent row groups share an XCD's L2.
//   rays    render_views_kernel's (view_ray and apply_pose, geometry_device.h): (cos S cos T, sin T, sin S cos T) on the lat-long grid of the output or (1, (i + 0.5 - cy) / fy,
//           (j + 0.5 - cx) / fx), rotated by pose[:3,:3]; origin pose @ (tgt_pos[2], tgt_pos[1], tgt_pos[0], 1).  That render frame (forward +x,
//           down +y, right +z) becomes the cube frame by swapping x and z.  Pose, origin and both cameras are wave-uniform (scalar loads).
//   shell   For origin o, direction r and half-side h: t = min over the axes of (h sign(r_k) - o_k) / r_k, evaluated as h / |r_k| - o_k / r_k
//           with the two quotients per pixel (IEEE divides; an axis with r_k = 0 is given +inf, and fminf drops a NaN), P = o + t r.  The face
//           is the axis of the largest |P_k| with its sign (ties: z, x, y); p = R_f^T P is two selects; u = fx p_x / h + cx, v = fy p_y / h + cy.
//   taps    u, v are clamped to [0, S-1] (fmaxf first: a NaN becomes 0 BEFORE the float -> int conversion), then bilinear over (x0, y0) ..
//           (min(x0+1, S-1), min(y0+1, S-1)): clamp to the edge of the chosen face, no zero padding, no fetch from the neighbouring face.
//           The face index differs per lane, so the descriptor is per SAMPLE (scalar: the six faces' 6 D S^2 texels) and the face and layer
//           are in the 32-bit per-lane offset ((f D + d) S^2 + y S + x) << log2(texel bytes); the host refuses a sample of 2^31 bytes or more.
//           Every index is in [0, S-1] and f in [0, 5] by construction, whatever the inputs; the descriptor's range check is a second line.
//           One 16-, 8- or 4-byte load per tap, decoded by geometry_device.h's decoders: a packed render has the bits of the render of the
//           unpacked stack.
//   loop    unrolled by 4: a shell's taps do not depend on the running composite, so several shells' taps are in flight under the blend.
//   status  a view whose origin is not strictly inside the innermost shell (max |o_k| >= min planes, or NaN) ORs MSI_RENDER_STATUS_ORIGIN_OUTSIDE
//           into *status (one lane per workgroup); its pixels are finite for finite inputs (t may be negative, the taps are clamped).
template <int MODE, int CAMERA, int FMT>
__global__ void __launch_bounds__(256)
cube_render_views_kernel(const void *__restrict__ layers, const float *__restrict__ pose_rt, const float *__restrict__ tgt_pos,
                         const float *__restrict__ intrinsics, const float *__restrict__ stack_intrinsics,
                         const float *__restrict__ depths, const float *__restrict__ trig, int batch, int views, int face, int nd,
                         int out_h, int out_w, float *__restrict__ out_rgb, float *__restrict__ out_depth, DepthFrac F,
                         int *__restrict__ status) {
  ViewBlock<4> k(out_h, out_w, views, batch);
  if (k.past_end()) return;                             // (grid rounded up to a multiple of 8; whole workgroups leave)
  k.decode(views);
  const unsigned bv = k.bv;
  const int i = k.i, j = k.j, b = k.b;
  if (j >= out_w || i >= out_h) return;                 // (no barrier below; lane (0, 0) of a workgroup is always inside)

  ViewRay r = view_ray<CAMERA>(intrinsics, nullptr, trig, tgt_pos, bv, i, j, out_h, out_w);
  apply_pose(pose_rt + (size_t)bv * 16, r);
  // render frame -> cube frame: x <-> z
  const float dx = r.rz, dy = r.ry, dz = r.rx;
  const float ox = r.cz, oy = r.cy, oz = r.cx;
  // t_k = h / |r_k| - o_k / r_k
  const float inf = __builtin_inff();
  const float ax = dx != 0.0f ? 1.0f / fabsf(dx) : inf, bx = dx != 0.0f ? ox / dx : 0.0f;
  const float ay = dy != 0.0f ? 1.0f / fabsf(dy) : inf, by = dy != 0.0f ? oy / dy : 0.0f;
  const float az = dz != 0.0f ? 1.0f / fabsf(dz) : inf, bz = dz != 0.0f ? oz / dz : 0.0f;

  const float *Ks = stack_intrinsics + (size_t)b * 9;   // the six faces' camera: fx . cx / . fy cy
  const float kfx = Ks[0], kcx = Ks[2], kfy = Ks[4], kcy = Ks[5];
  const float sm1 = (float)(face - 1);
  const unsigned ss2 = (unsigned)face * (unsigned)face, fstride = ss2 * (unsigned)nd;     // texels of a layer / of a face's stack
  const size_t sample_bytes = ((size_t)6 * fstride) << StackTexel<FMT>::shift;          // (< 2^31, checked on the host)
  const __amdgpu_buffer_rsrc_t L =
      __builtin_amdgcn_make_buffer_rsrc((void *)(static_cast<const char *>(layers) + (size_t)b * sample_bytes), 0, (int)sample_bytes, 0x00020000);
  float o0 = 0.f, o1 = 0.f, o2 = 0.f, od = 0.f;
  float hmin = inf;

#pragma unroll 4
  for (int d = 0; d < nd; ++d) {
    const float h = depths[d];
    hmin = fminf(hmin, h);
    const float t = fminf(fminf(__builtin_fmaf(h, ax, -bx), __builtin_fmaf(h, ay, -by)), __builtin_fmaf(h, az, -bz));
    const float px = __builtin_fmaf(t, dx, ox), py = __builtin_fmaf(t, dy, oy), pz = __builtin_fmaf(t, dz, oz);
    const float mx = fabsf(px), my = fabsf(py), mz = fabsf(pz);
    const bool zf = mz >= mx && mz >= my;               // ties: z, x, y (a NaN point compares false everywhere: a y face, clamped taps)
    const bool xf = !zf && mx >= my;
    const bool neg = (zf ? pz : (xf ? px : py)) < 0.0f;
    const unsigned f = zf ? (neg ? 2u : 0u) : (xf ? (neg ? 3u : 1u) : (neg ? 4u : 5u));
    const float qx = zf ? (neg ? -px : px) : (xf ? (neg ? pz : -pz) : px);   // p = R_f^T P
    const float qy = (zf || xf) ? py : (neg ? pz : -pz);
    const float inv_h = t_div(1.0f, h);
    const float u = fminf(fmaxf(__builtin_fmaf(qx, kfx * inv_h, kcx), 0.0f), sm1);   // fmaxf(NaN, 0) = 0
    const float v = fminf(fmaxf(__builtin_fmaf(qy, kfy * inv_h, kcy), 0.0f), sm1);
    const float fx0 = floorf(u), fy0 = floorf(v);
    const float dx0 = u - fx0, dy0 = v - fy0, dx1 = 1.0f - dx0, dy1 = 1.0f - dy0;
    const int x0 = (int)fx0, y0 = (int)fy0;             // in [0, S-1]
    const int x1 = min(x0 + 1, face - 1), y1 = min(y0 + 1, face - 1);
    const unsigned base = f * fstride + (unsigned)d * ss2;
    const unsigned r0 = base + (unsigned)y0 * (unsigned)face, r1 = base + (unsigned)y1 * (unsigned)face;
    const float4 A = StackTexel<FMT>::tap(L, r0 + (unsigned)x0), Bv = StackTexel<FMT>::tap(L, r0 + (unsigned)x1);
    const float4 C = StackTexel<FMT>::tap(L, r1 + (unsigned)x0), Dv = StackTexel<FMT>::tap(L, r1 + (unsigned)x1);
    const float wa = dy1 * dx1, wb = dy1 * dx0, wc = dy0 * dx1, wd = dy0 * dx0;
    float4 c;
    c.w = ((wa * A.w + wb * Bv.w) + wc * C.w) + wd * Dv.w;
    c.x = ((wa * A.x + wb * Bv.x) + wc * C.x) + wd * Dv.x;
    c.y = ((wa * A.y + wb * Bv.y) + wc * C.y) + wd * Dv.y;
    c.z = ((wa * A.z + wb * Bv.z) + wc * C.z) + wd * Dv.z;
    const float al = c.w;
    if (MODE & RENDER_RGB) {
      if (d == 0) {
        o0 = c.x; o1 = c.y; o2 = c.z;
      } else {
        const float om = 1.0f - al;
        o0 = c.x * al + o0 * om;
        o1 = c.y * al + o1 * om;
        o2 = c.z * al + o2 * om;
      }
    }
    if (MODE & RENDER_DEPTH) {   // over_composite_depth: 0 at layer 0, then (d / D) a + out (1 - a)
      if (d == 0) od = 0.0f;
      else od = F.f[d] * al + od * (1.0f - al);
    }
  }
  // the origin is a property of the view: every lane agrees (fmaxf drops a NaN, so it is tested by itself)
  if (status != nullptr && threadIdx.x == 0 && threadIdx.y == 0) {
    const float omax = fmaxf(fmaxf(fabsf(ox), fabsf(oy)), fabsf(oz));
    if (!(omax < hmin) || ox != ox || oy != oy || oz != oz) atomicOr(status, MSI_RENDER_STATUS_ORIGIN_OUTSIDE);
  }
  store_pixel<MODE>(out_rgb, out_depth, ((size_t)bv * out_h + i) * out_w + j, o0, o1, o2, od);
}

// Panorama -> six face images: image [B,H,W,C] (C <= 4) -> out [B,6,S,S,C].  Texel (ix, iy) of face f looks along R_f K^-1 (ix, iy, 1) in the
// cube frame; with x and z swapped that is a direction of the render frame, whose longitude atan2(z, x) and latitude asin(y / |dir|) sit at
// u = (lon + pi) / 2pi W - 0.5, v = (lat + pi/2) / pi H - 0.5 of the lat-long grid.  Bilinear, wrapping in u and clamping in v.  One thread per
// output texel; libm's atan2f / asinf (the kernel moves a few hundred KB).  The coordinates are clamped (fmaxf first: NaN -> lower bound) before
// the float -> int conversion, so every index is in range for any input.
__global__ void __launch_bounds__(256)
equirect_to_cube_kernel(const float *__restrict__ image, const float *__restrict__ intrinsics, int batch, int height, int width,
                        int channels, int face, float *__restrict__ out) {
  const size_t n = (size_t)batch * 6 * face * face;
  for (size_t idx = (size_t)blockIdx.x * blockDim.x + threadIdx.x; idx < n; idx += (size_t)gridDim.x * blockDim.x) {
    const int ix = (int)(idx % face), iy = (int)((idx / face) % face);
    const int bf = (int)(idx / ((size_t)face * face));
    const int b = bf / 6, f = bf - b * 6;
    const float *K = intrinsics + (size_t)b * 9;
    const float qx = ((float)ix - K[2]) / K[0], qy = ((float)iy - K[5]) / K[4];   // K^-1 (ix, iy, 1), z = 1
    float x, y, z;                                                                  // R_f q
    switch (f) {
      case 0: x = qx; y = qy; z = 1.0f; break;
      case 1: x = 1.0f; y = qy; z = -qx; break;
      case 2: x = -qx; y = qy; z = -1.0f; break;
      case 3: x = -1.0f; y = qy; z = qx; break;
      case 4: x = qx; y = -1.0f; z = qy; break;
      default: x = qx; y = 1.0f; z = -qy; break;
    }
    // render frame = (z, y, x): lon = atan2(render z, render x) = atan2(x, z); "+ 0.0f" turns -0 into +0, so a face centre that looks straight
    // at a pole has ONE longitude (atan2(+0, +0) = 0) whichever face it is on
    const float lon = atan2f(x + 0.0f, z + 0.0f);
    const float lat = asinf(y / sqrtf((x * x + y * y) + z * z));
    const float PI = 3.14159265358979323846f;
    float u = ((lon + PI) / (2.0f * PI)) * (float)width - 0.5f;
    float v = ((lat + 0.5f * PI) / PI) * (float)height - 0.5f;
    u = fminf(fmaxf(u, -0.5f), (float)width - 0.5f);
    v = fminf(fmaxf(v, 0.0f), (float)(height - 1));
    const float fx0 = floorf(u), fy0 = floorf(v);
    const float du = u - fx0, dv = v - fy0;
    int x0 = (int)fx0, y0 = (int)fy0;                   // x0 in [-1, W-1], y0 in [0, H-1]
    int x1 = x0 + 1;
    const int y1 = min(y0 + 1, height - 1);
    x0 = x0 < 0 ? x0 + width : x0;
    x1 = x1 >= width ? x1 - width : x1;
    const float *img = image + (size_t)b * height * width * channels;
    const float *a = img + ((size_t)y0 * width + x0) * channels, *bb = img + ((size_t)y0 * width + x1) * channels;
    const float *c = img + ((size_t)y1 * width + x0) * channels, *dd = img + ((size_t)y1 * width + x1) * channels;
    const float wa = (1.0f - dv) * (1.0f - du), wb = (1.0f - dv) * du, wc = dv * (1.0f - du), wd = dv * du;
    float *o = out + idx * channels;
    for (int ch = 0; ch < channels; ++ch) o[ch] = ((wa * a[ch] + wb * bb[ch]) + wc * c[ch]) + wd * dd[ch];
  }
}

}  // namespace

extern "C" {

int msi_cube_render_views(const void *layers, int32_t format, const float *tgt_pose_rt, const float *tgt_pos,
                          const float *tgt_intrinsics, const float *stack_intrinsics, const float *depths, const float *trig,
                          int32_t batch, int32_t views, int32_t face_size, int32_t num_planes, int32_t camera,
                          int32_t out_height, int32_t out_width, float *out_rgb, float *out_depth, int32_t *status_device,
                          msi_stream_t stream) {
  const ViewArgs a = {"cube_render_views", out_rgb, out_depth, layers && tgt_pose_rt && tgt_pos && stack_intrinsics && depths, format, ANY_FORMAT, "",
                      &camera, trig, tgt_intrinsics, nullptr, batch >= 0 && face_size > 0 && num_planes > 0, 0, views, batch, out_height, out_width, 4};
  const auto planes = [&] {
    return num_planes <= DEPTH_FRAC_MAX ? (int)MSI_OK : msi::fail(MSI_E_UNSUPPORTED, "cube_render_views: at most %d planes", DEPTH_FRAC_MAX);
  };
  // the per-sample descriptor: the six faces' stacks are addressed with one 32-bit byte offset per lane
  const auto sample_bytes = [&] {
    const int texel_bytes = format == MSI_LAYERS_F32 ? 16 : format == MSI_LAYERS_RGBA16F ? 8 : 4;
    MSI_REQUIRE(face_size < (1 << 15) && (long)face_size * face_size * 6 * num_planes * texel_bytes < (1L << 31),   // (< 2^30 * 6 * 128 * 16)
                "cube_render_views: a sample's six face stacks (6 x %d x %d x %d texels of %d bytes) reach 2^31 bytes (32-bit offsets)",
                num_planes, face_size, face_size, texel_bytes);
    return (int)MSI_OK;
  };
  unsigned grid;
  if (const int e = check_views(a, planes, sample_bytes, &grid)) return e;
  if (batch == 0) return MSI_OK;
  const DepthFrac F = depth_fractions(num_planes);
  hipStream_t s = msi::as_stream(stream);
  for_mode(render_mode(out_rgb, out_depth), [&](auto M) { for_camera(camera, [&](auto CAM) { for_format(format, [&](auto FMT) {
    hipLaunchKernelGGL((cube_render_views_kernel<decltype(M)::value, decltype(CAM)::value, decltype(FMT)::value>), dim3(grid), dim3(64, 4), 0, s,
                       layers, tgt_pose_rt, tgt_pos, tgt_intrinsics, stack_intrinsics, depths, trig, batch, views, face_size, num_planes,
                       out_height, out_width, out_rgb, out_depth, F, status_device);
  }); }); });
  return msi::check_launch("cube_render_views");
}

int msi_equirect_to_cube_f32(const float *image, const float *intrinsics, int32_t batch, int32_t height, int32_t width,
                             int32_t channels, int32_t face_size, float *out, msi_stream_t stream) {
  MSI_REQUIRE(image && intrinsics && out, "equirect_to_cube: null pointer");
  MSI_REQUIRE(batch >= 0 && height > 0 && width > 0 && face_size > 0, "equirect_to_cube: bad dims");
  MSI_REQUIRE(channels >= 1 && channels <= 4, "equirect_to_cube: channels must be 1..4 (got %d)", channels);
  MSI_REQUIRE((long)height * width < (1L << 24) && face_size < (1 << 12), "equirect_to_cube: image of 2^24 pixels or faces of 4096 or more");
  if (batch == 0) return MSI_OK;
  const size_t n = (size_t)batch * 6 * face_size * face_size;
  hipLaunchKernelGGL(equirect_to_cube_kernel, dim3(grid_1d(n)), dim3(256), 0, msi::as_stream(stream), image, intrinsics, batch, height,
                     width, channels, face_size, out);
  return msi::check_launch("equirect_to_cube");
}

}  // extern "C"
