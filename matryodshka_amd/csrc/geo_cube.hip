// The cube-map viewer of the PP path (no reference counterpart): cube_render_views_kernel renders V views per sample from SIX face stacks in one
// launch, equirect_to_cube_kernel cuts a panorama into the six face images the PP network takes; kernels first, their C ABI entry points below.
// The cube conventions and the pixel's pieces (ray, shell hit, blend, origin test) are geo_cube.h's.
//
// The SEAMLESS filter (cube_render_views_seamless_kernel, msi_cube_render_views_seamless; include/msi_hip.h and cubemap.virtual_texel state the
// same rule).  It is defined for the cube camera fx = fy = cx = cy = S/2 only: a face then stores tan = -1 .. 1 - 2/S, nothing on its +x and +y
// edges, and the cube point of lattice point (x, y), 0 <= x, y <= S, of a face is a lattice point of every other face that contains it.  Ray,
// shell hit, face choice and p = R_f^T P are geo_cube.h's pieces, the clamp kernel's too.  Then
//   1. u, v are clamped to [0, S] (fmaxf first); 2. x0 = min(floor(u), S-1), x1 = x0 + 1 <= S, du = u - x0 in [0, 1], likewise y0, y1, dv;
//   3. four bilinear taps with the clamp kernel's weights and sum order; 4. a tap with x < S and y < S is the face's own texel;
//   5. a tap with x = S or y = S is a VIRTUAL texel at the cube point P (an edge point; a cube corner when the other coordinate is 0 or S).
//      The other faces containing P (one on an edge, two at a corner) are tried in ascending face index: the first whose lattice coordinates
//      of P lie in [0, S-1]^2 supplies its texel (one fetch).  When none stores P, the virtual texel is the mean of the clamped texels
//      (coordinates clamped to [0, S-1]) of all faces meeting at P: own face first, then the others in ascending index, (a + b) * 0.5f or
//      ((a + b) + c) * (1.0f / 3.0f), per channel (alpha included) on decoded fp32 values.
// The neighbour across each side in closed form (t = the running coordinate; cube_side_px .. cube_corner_nx below), lattice coordinates in the
// neighbour g:
//   f        +x side (x = S, t = y)     +y side (y = S, t = x)     third face at corner (S, 0)     third face at corner (0, S)
//   0 front  g 1 (0, t)                 g 5 (t, 0)                 g 4 (S, S)                      g 3 (S, S)
//   1 right  g 2 (0, t)                 g 5 (S, t)      *          g 4 (S, 0)                      g 0 (S, S)
//   2 back   g 3 (0, t)                 g 5 (S - t, S)  *          g 4 (0, 0)                      g 1 (S, S)
//   3 left   g 0 (0, t)                 g 5 (0, S - t)             g 4 (0, S)                      g 2 (S, S)
//   4 up     g 1 (S - t, 0)             g 0 (t, 0)                 g 2 (0, 0)                      g 3 (S, 0)
//   5 down   g 1 (t, S)      *          g 2 (S - t, S)  *          g 0 (S, S)                      g 3 (0, S)
// (* a coordinate S: the neighbour does not store the edge either.)  Of the 12 cube edges 8 are stored by one face (the ring front -> right ->
// back -> left -> front, front/up, front/down, up/right, down/left): the filter is continuous across them.  2 have no stored sample
// (right/down, back/down): the mean rule makes them continuous over a two-texel span.  2 are stored twice (up/back, up/left: row 0 of both
// faces): each face keeps its own texel, so a step in CONTENT between the two faces remains there; in-range texels are never overridden.
#include "geometry_device.h"
#include "geo_cube.h"

namespace {

// One thread per target pixel, the whole far-to-near composite in that thread (strictly sequential, as mpi_render_views_kernel: layer 0
// replaces, then c a + acc (1 - a)); a workgroup is 64 x 4 pixels of one (sample, view), a wave one row.
//   grid    1-D, sample -> view -> 4-row group -> 64-pixel block with the XCD-aware mapping of every many-views render (ViewBlock, geometry_device.h): the views of one cube follow each
//           other through the Infinity Cache and adjacent row groups share an XCD's L2.
//   pixel   ray, shell hit, blend and origin test are geo_cube.h's pieces (cube_ray, cube_hit with hi = S-1, cube_blend, cube_origin_outside);
//           CAMERA_ODS is msi_cube_render_ods_views.
//   taps    bilinear over (x0, y0) .. (min(x0+1, S-1), min(y0+1, S-1)) of u, v in [0, S-1]: clamp to the edge of the chosen face, no zero padding,
//           no fetch from the neighbouring face.
//           The face index differs per lane, so the descriptor is per SAMPLE (scalar: the six faces' 6 D S^2 texels) and the face and layer
//           are in the 32-bit per-lane offset ((f D + d) S^2 + y S + x) << log2(texel bytes); the host refuses a sample of 2^31 bytes or more.
//           Every index is in [0, S-1] and f in [0, 5] by construction, whatever the inputs; the descriptor's range check is a second line.
//           One 16-, 8- or 4-byte load per tap, decoded by geometry_device.h's decoders: a packed render has the bits of the render of the
//           unpacked stack.
//   loop    unrolled by 4: a shell's taps do not depend on the running composite, so several shells' taps are in flight under the blend.  The
//           composite is this kernel's own text (over_step grows its depth-only instantiations: profiles/shared_render_pieces_isa.txt).
//   status  one lane per workgroup; CAMERA_ODS: every lane tests its own origin, one atomicOr per wavefront with a set lane.
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

  const CubeRay r = cube_ray<CAMERA>(intrinsics, trig, tgt_pos, pose_rt, bv, i, j, out_h, out_w);
  const CubeCamera cam = cube_stack_camera(stack_intrinsics, b);
  const float sm1 = (float)(face - 1);
  const unsigned ss2 = (unsigned)face * (unsigned)face, fstride = ss2 * (unsigned)nd;     // texels of a layer / of a face's stack
  const size_t sample_bytes = ((size_t)6 * fstride) << StackTexel<FMT>::shift;          // (< 2^31, checked on the host)
  const __amdgpu_buffer_rsrc_t L =
      __builtin_amdgcn_make_buffer_rsrc((void *)(static_cast<const char *>(layers) + (size_t)b * sample_bytes), 0, (int)sample_bytes, 0x00020000);
  float o0 = 0.f, o1 = 0.f, o2 = 0.f, od = 0.f;
  float hmin = __builtin_inff();

#pragma unroll 4
  for (int d = 0; d < nd; ++d) {
    const float h = depths[d];
    hmin = fminf(hmin, h);
    const CubeHit p = cube_hit(r, cam, h, sm1);
    const float fx0 = floorf(p.u), fy0 = floorf(p.v);
    const float dx0 = p.u - fx0, dy0 = p.v - fy0, dx1 = 1.0f - dx0, dy1 = 1.0f - dy0;
    const int x0 = (int)fx0, y0 = (int)fy0;             // in [0, S-1]
    const int x1 = min(x0 + 1, face - 1), y1 = min(y0 + 1, face - 1);
    const unsigned base = p.f * fstride + (unsigned)d * ss2;
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
  if constexpr (CAMERA == CAMERA_ODS) {                 // (every lane tests its own origin, the wave votes, lane 0 issues the atomicOr)
    if (status != nullptr) {
      const bool any = __builtin_amdgcn_ballot_w64(cube_origin_outside(r, hmin)) != 0;   // (wave-uniform)
      if (any && threadIdx.x == 0) atomicOr(status, MSI_RENDER_STATUS_ORIGIN_OUTSIDE);
    }
  } else {                                              // (the origin is a property of the view: every lane agrees)
    if (status != nullptr && threadIdx.x == 0 && threadIdx.y == 0) {
      if (cube_origin_outside(r, hmin)) atomicOr(status, MSI_RENDER_STATUS_ORIGIN_OUTSIDE);
    }
  }
  store_pixel<MODE>(out_rgb, out_depth, ((size_t)bv * out_h + i) * out_w + j, o0, o1, o2, od);
}

// ---- the seamless filter: the neighbour tables in closed form (integer selects on the face and the side; no memory table)
struct CubeTexel { unsigned f; int x, y; };              // lattice coordinates in [0, S] for t in [0, S]
__device__ __forceinline__ CubeTexel cube_side_px(unsigned f, int t, int S) {      // across x = S, t = y
  CubeTexel r;
  r.f = f < 4u ? ((f + 1u) & 3u) : 1u;
  r.x = f < 4u ? 0 : (f == 4u ? S - t : t);
  r.y = f < 4u ? t : (f == 4u ? 0 : S);
  return r;
}
__device__ __forceinline__ CubeTexel cube_side_py(unsigned f, int t, int S) {      // across y = S, t = x
  const bool keep = f == 0u || f == 4u;
  CubeTexel r;
  r.f = f < 4u ? 5u : (f == 4u ? 0u : 2u);
  r.x = keep ? t : (f == 1u ? S : (f == 3u ? 0 : S - t));
  r.y = keep ? 0 : (f == 1u ? t : (f == 3u ? S - t : S));
  return r;
}
__device__ __forceinline__ CubeTexel cube_corner_ny(unsigned f, int S) {           // the third face at corner (S, 0): across y = 0
  CubeTexel r;
  r.f = f < 4u ? 4u : (f == 4u ? 2u : 0u);
  r.x = (f <= 1u || f == 5u) ? S : 0;
  r.y = (f == 0u || f == 3u || f == 5u) ? S : 0;
  return r;
}
__device__ __forceinline__ CubeTexel cube_corner_nx(unsigned f, int S) {           // the third face at corner (0, S): across x = 0
  CubeTexel r;
  r.f = f < 4u ? ((f + 3u) & 3u) : 3u;
  r.x = f == 5u ? 0 : S;
  r.y = f == 4u ? 0 : S;
  return r;
}
// The virtual texel of lattice point (x, y) of face f with x == S or y == S (x, y in [0, S]): n = 1 -> the texel at o0 (another face's); n = 2 ->
// (o0 + o1) * 0.5f; n = 3 -> ((o0 + o1) + o2) * (1/3), o0 the own face's clamped texel.  Offsets are texels from the sample's base; every
// coordinate goes through min(., S-1) and every face through the selects above: in range for any f in [0, 5], x, y in [0, S].
struct VirtualTexel { unsigned n, o0, o1, o2; };
__device__ __forceinline__ VirtualTexel cube_virtual_texel(unsigned f, int x, int y, int S, unsigned fstride, unsigned dbase) {
  const bool xs = x == S, ys = y == S;
  const bool corner = (xs && ys) || (xs && y == 0) || (ys && x == 0);
  CubeTexel a = xs ? cube_side_px(f, y, S) : cube_side_py(f, x, S);
  CubeTexel b = (xs && ys) ? cube_side_py(f, x, S) : (xs ? cube_corner_ny(f, S) : cube_corner_nx(f, S));   // (meaningful at a corner only)
  if (corner && b.f < a.f) { const CubeTexel c = a; a = b; b = c; }                  // ascending face index
  const bool ia = a.x < S && a.y < S, ib = corner && b.x < S && b.y < S;
  const int m = S - 1;
  const auto at = [&](unsigned g, int tx, int ty) { return g * fstride + dbase + (unsigned)min(ty, m) * (unsigned)S + (unsigned)min(tx, m); };
  const unsigned oa = at(a.f, a.x, a.y), ob = at(b.f, b.x, b.y);
  VirtualTexel v;
  v.n = (ia || ib) ? 1u : (corner ? 3u : 2u);
  v.o0 = ia ? oa : (ib ? ob : at(f, x, y));
  v.o1 = oa;
  v.o2 = ob;
  return v;
}
__device__ __forceinline__ float4 cube_select(bool c, float4 a, float4 b) {
  float4 r;
  r.x = c ? a.x : b.x; r.y = c ? a.y : b.y; r.z = c ? a.z : b.z; r.w = c ? a.w : b.w;
  return r;
}
__device__ __forceinline__ float4 cube_mean(unsigned n, float4 a, float4 b, float4 c) {
  float4 r;
  if (n == 3u) {
    const float third = 1.0f / 3.0f;
    r.x = ((a.x + b.x) + c.x) * third; r.y = ((a.y + b.y) + c.y) * third; r.z = ((a.z + b.z) + c.z) * third; r.w = ((a.w + b.w) + c.w) * third;
  } else {
    r.x = (a.x + b.x) * 0.5f; r.y = (a.y + b.y) * 0.5f; r.z = (a.z + b.z) * 0.5f; r.w = (a.w + b.w) * 0.5f;
  }
  return r;
}

// The same table for an EDGE point (no corner), where nearly all strip lanes are: the neighbour's texel is affine in the running coordinate,
// texel = (g D + d) S^2 + c0 + t k for t in [1, S-1] (t is clamped to that range: in the neighbour's face for any input, S >= 2).  Where the
// neighbour does not store the edge (!stored) it is the neighbour's CLAMPED texel, the second term of the two-face mean.
//   +x side  f < 4: g = f + 1 & 3, (0, t): c0 = 0, k = S     f = 4: g = 1, (S - t, 0): c0 = S, k = -1      f = 5: g = 1, (t, S-1): c0 = S^2 - S, k = 1, !stored
//   +y side  f = 0, 4: g = 5, 0, (t, 0): c0 = 0, k = 1       f = 1: g = 5, (S-1, t): c0 = S - 1, k = S, !stored
//            f = 3: g = 5, (0, S - t): c0 = S^2, k = -S      f = 2, 5: g = 5, 2, (S - t, S-1): c0 = S^2, k = -1, !stored
struct CubeEdge { unsigned n0, n1; bool stored; };         // the neighbour's texels at t and t + 1
__device__ __forceinline__ CubeEdge cube_edge(unsigned f, bool xside, int t, int S, unsigned ss2, unsigned fstride, unsigned dbase) {
  const bool ring = f < 4u;
  const unsigned gx = ring ? ((f + 1u) & 3u) : 1u, gy = ring ? 5u : (f == 4u ? 0u : 2u);
  const int cx0 = ring ? 0 : (f == 4u ? S : (int)ss2 - S), kx = ring ? S : (f == 4u ? -1 : 1);
  const bool keep = f == 0u || f == 4u;
  const int cy0 = keep ? 0 : (f == 1u ? S - 1 : (int)ss2), ky = keep ? 1 : (f == 1u ? S : (f == 3u ? -S : -1));
  const unsigned g = xside ? gx : gy;
  const int c0 = xside ? cx0 : cy0, k = xside ? kx : ky;
  const int ta = min(max(t, 1), S - 1), tb = min(max(t + 1, 1), S - 1);
  const unsigned base = g * fstride + dbase;
  CubeEdge e;
  e.n0 = base + (unsigned)(c0 + ta * k);
  e.n1 = base + (unsigned)(c0 + tb * k);
  e.stored = xside ? f != 5u : (keep || f == 3u);
  return e;
}

// cube_render_views_kernel with the seamless filter (the rule: this file's header).  Grid and composite are that kernel's, the pixel's pieces
// geo_cube.h's (cube_hit with hi = S for the cube camera); what differs is the tap stage.
//   camera  the rule holds for fx = fy = cx = cy = S/2 only: the sample's stack camera is compared with S/2 (scalar, uniform per workgroup).  Any
//           other camera renders with the clamp rule (hi = S-1 below: the clamp kernel's values op for op) and ORs MSI_RENDER_STATUS_NOT_CUBE_CAMERA.
//   taps    four unconditional loads per shell, as the clamp kernel: A is always the own texel; B, C, D are the own texel, the neighbour's texel (8 of
//           the 12 edges: the offset is replaced, no extra fetch) or the own CLAMPED texel, the first term of a mean.  Only lanes in the strip
//           (x1 == S or y1 == S, about 2/S of the rays) run the integer selects of cube_edge, and only lanes on the two unstored edges (the mean's
//           second term) or in a corner square (cube_virtual_texel, the general rule) fetch again, in the blend pass;
//           each is under a branch a wavefront with no such lane skips (s_cbranch_execz).
//   loop    groups of four shells: first the four shells' taps are issued, then the four blends run, so up to 16 taps are in flight under the blend
//           (the clamp kernel's unroll by 4, written out because the strip branch sits between the shells).
//   bounds  x0, y0 in [0, S-1] by the clamps (a NaN is 0), x1, y1 in [0, S]; every fetched coordinate passes min(., S-1) (cube_edge: its running coordinate is clamped
//           to [1, S-1], which keeps c0 + t k inside the neighbour's S^2 texels), every face is a select with values in [0, 5]: all offsets lie inside the sample's 6 D S^2 texels for any input; the descriptor's range check is a second line.
template <int FMT> struct CubeShellTaps {
  float4 A, B, C, D;
  float du, dv;
  unsigned key;            // f | x0 << 3 | again << 31 (x0 < 2^15); y0 below
  int y0;
};

template <int MODE, int CAMERA, int FMT>
__global__ void __launch_bounds__(256)
cube_render_views_seamless_kernel(const void *__restrict__ layers, const float *__restrict__ pose_rt, const float *__restrict__ tgt_pos,
                                  const float *__restrict__ intrinsics, const float *__restrict__ stack_intrinsics,
                                  const float *__restrict__ depths, const float *__restrict__ trig, int batch, int views, int face, int nd,
                                  int out_h, int out_w, float *__restrict__ out_rgb, float *__restrict__ out_depth, DepthFrac F,
                                  int *__restrict__ status) {
  ViewBlock<4> k(out_h, out_w, views, batch);
  if (k.past_end()) return;
  k.decode(views);
  const unsigned bv = k.bv;
  const int i = k.i, j = k.j, b = k.b;
  if (j >= out_w || i >= out_h) return;

  const CubeRay r = cube_ray<CAMERA>(intrinsics, trig, tgt_pos, pose_rt, bv, i, j, out_h, out_w);
  const CubeCamera cam = cube_stack_camera(stack_intrinsics, b);
  const float half = 0.5f * (float)face;
  const bool cube_camera = cam.fx == half && cam.fy == half && cam.cx == half && cam.cy == half;    // (a NaN camera: false)
  const int m = face - 1, hi = cube_camera ? face : m;
  const float sm1 = (float)m, fhi = (float)hi;
  const unsigned ss2 = (unsigned)face * (unsigned)face, fstride = ss2 * (unsigned)nd;
  const size_t sample_bytes = ((size_t)6 * fstride) << StackTexel<FMT>::shift;
  const __amdgpu_buffer_rsrc_t L =
      __builtin_amdgcn_make_buffer_rsrc((void *)(static_cast<const char *>(layers) + (size_t)b * sample_bytes), 0, (int)sample_bytes, 0x00020000);
  float o0 = 0.f, o1 = 0.f, o2 = 0.f, od = 0.f;
  float hmin = __builtin_inff();

  const auto fetch = [&](int d, CubeShellTaps<FMT> &T) {
    const float h = depths[d];
    hmin = fminf(hmin, h);
    const CubeHit p = cube_hit(r, cam, h, fhi);
    const unsigned f = p.f;
    const float fx0 = fminf(floorf(p.u), sm1), fy0 = fminf(floorf(p.v), sm1);
    const int x0 = (int)fx0, y0 = (int)fy0;             // in [0, S-1]
    const int x1 = min(x0 + 1, hi), y1 = min(y0 + 1, hi);   // in [0, S]; S only with the cube camera
    const unsigned dbase = (unsigned)d * ss2, base = f * fstride + dbase;
    const unsigned r0 = base + (unsigned)y0 * (unsigned)face, r1 = base + (unsigned)min(y1, m) * (unsigned)face;
    unsigned oB = r0 + (unsigned)min(x1, m), oC = r1 + (unsigned)x0, oD = r1 + (unsigned)min(x1, m);
    unsigned again = 0u;                                // an unstored edge or a corner square: the blend pass fetches again
    if (x1 == face || y1 == face) {                     // the strip: B, C, D may be virtual texels
      const bool xs = x1 == face, ys = y1 == face;
      if (!((xs && (ys || y0 == 0)) || (ys && x0 == 0))) {   // an edge: B and D across x = S (t = y0, y0 + 1) or C and D across y = S (t = x0, x0 + 1)
        const CubeEdge e = cube_edge(f, xs, xs ? y0 : x0, face, ss2, fstride, dbase);
        if (e.stored) {
          oB = xs ? e.n0 : oB; oC = xs ? oC : e.n0; oD = e.n1;
        } else {
          again = 1u;
        }
      } else {                                          // a corner square (a few lanes): the blend pass fetches its virtual texels
        again = 1u;
      }
    }
    T.A = StackTexel<FMT>::tap(L, r0 + (unsigned)x0); T.B = StackTexel<FMT>::tap(L, oB);
    T.C = StackTexel<FMT>::tap(L, oC); T.D = StackTexel<FMT>::tap(L, oD);
    T.du = p.u - fx0; T.dv = p.v - fy0;
    T.key = f | ((unsigned)x0 << 3) | (again << 31);
    T.y0 = y0;
  };
  const auto blend = [&](int d, CubeShellTaps<FMT> &T) {
    if (T.key >> 31) {                                  // an unstored edge (the other face's clamped texels for the means) or a corner square
      const unsigned f = T.key & 7u, dbase = (unsigned)d * ss2;
      const int x0 = (int)((T.key >> 3) & 0x7fffu), y0 = T.y0, x1 = x0 + 1, y1 = y0 + 1;   // (set with the cube camera only: hi = S)
      const bool xs = x1 == face, ys = y1 == face;
      if (!((xs && (ys || y0 == 0)) || (ys && x0 == 0))) {   // an unstored edge: the two-face mean of both virtual texels
        const CubeEdge e = cube_edge(f, xs, xs ? y0 : x0, face, ss2, fstride, dbase);
        const float4 n0 = StackTexel<FMT>::tap(L, e.n0), n1 = StackTexel<FMT>::tap(L, e.n1);
        const float4 own = cube_select(xs, T.B, T.C), m0 = cube_mean(2u, own, n0, n0);       // (selects, not two stores: the shells stay in registers)
        T.B = cube_select(xs, m0, T.B);
        T.C = cube_select(xs, T.C, m0);
        T.D = cube_mean(2u, T.D, n1, n1);
      } else {                                          // a corner square: its virtual texels through the general rule
        const auto corner_tap = [&](int tx, int ty) {
          const VirtualTexel vt = cube_virtual_texel(f, tx, ty, face, fstride, dbase);
          const float4 a = StackTexel<FMT>::tap(L, vt.o0), b = StackTexel<FMT>::tap(L, vt.o1), c = StackTexel<FMT>::tap(L, vt.o2);
          float4 r = a;
          if (vt.n > 1u) r = cube_mean(vt.n, a, b, c);
          return r;
        };
        if (xs) T.B = corner_tap(x1, y0);
        __builtin_amdgcn_sched_barrier(0);              // (one tap's loads at a time: these few lanes must not cost every lane registers)
        if (ys) T.C = corner_tap(x0, y1);
        __builtin_amdgcn_sched_barrier(0);
        T.D = corner_tap(x1, y1);
      }
    }
    const float4 c = cube_blend(T.du, T.dv, T.A, T.B, T.C, T.D);
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
    if (MODE & RENDER_DEPTH) {
      if (d == 0) od = 0.0f;
      else od = F.f[d] * al + od * (1.0f - al);
    }
  };

  for (int d0 = 0; d0 < nd; d0 += 4) {                  // (four named shells)
    CubeShellTaps<FMT> T0, T1, T2, T3;
    const bool s1 = d0 + 1 < nd, s2 = d0 + 2 < nd, s3 = d0 + 3 < nd;
    fetch(d0, T0);
    if (s1) fetch(d0 + 1, T1);
    if (s2) fetch(d0 + 2, T2);
    if (s3) fetch(d0 + 3, T3);
    blend(d0, T0);
    if (s1) blend(d0 + 1, T1);
    if (s2) blend(d0 + 2, T2);
    if (s3) blend(d0 + 3, T3);
  }
  if constexpr (CAMERA == CAMERA_ODS) {                 // (the wave votes on its lanes' origins; the stack camera is uniform)
    if (status != nullptr) {
      const bool any = __builtin_amdgcn_ballot_w64(cube_origin_outside(r, hmin)) != 0;
      const int bits = (cube_camera ? 0 : MSI_RENDER_STATUS_NOT_CUBE_CAMERA) | (any ? MSI_RENDER_STATUS_ORIGIN_OUTSIDE : 0);
      if (bits && threadIdx.x == 0) atomicOr(status, bits);
    }
  } else if (status != nullptr && threadIdx.x == 0 && threadIdx.y == 0) {
    int bits = cube_camera ? 0 : MSI_RENDER_STATUS_NOT_CUBE_CAMERA;
    if (cube_origin_outside(r, hmin)) bits |= MSI_RENDER_STATUS_ORIGIN_OUTSIDE;
    if (bits) atomicOr(status, bits);
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

// the viewers share their argument checks and grid; `seamless` picks the kernel family.  ods: the ODS camera's entry point -- no camera code, every
// table required, `camera_table` is eye_radius [B*V] (it travels in the kernels' `intrinsics` argument) and `filtering` is the caller's code, checked here.
static int cube_views_launch(const char *who, bool ods, int32_t filtering, const void *layers, int32_t format, const float *tgt_pose_rt,
                             const float *tgt_pos, const float *camera_table, const float *stack_intrinsics, const float *depths, const float *trig,
                             int32_t batch, int32_t views, int32_t face_size, int32_t num_planes, int32_t camera,
                             int32_t out_height, int32_t out_width, float *out_rgb, float *out_depth, int32_t *status_device,
                             msi_stream_t stream) {
  const bool inputs = layers && tgt_pose_rt && tgt_pos && stack_intrinsics && depths && (!ods || (camera_table && trig));
  const ViewArgs a = {who, out_rgb, out_depth, inputs, format, ANY_FORMAT, "", ods ? nullptr : &camera, trig, camera_table, nullptr,
                      batch >= 0 && face_size > 0 && num_planes > 0, 0, views, batch, out_height, out_width, 4};
  const auto planes = [&] {
    MSI_REQUIRE(filtering == 0 || filtering == 1, "%s: unknown filtering %d (0 clamp, 1 seamless)", who, filtering);
    return num_planes <= DEPTH_FRAC_MAX ? (int)MSI_OK : msi::fail(MSI_E_UNSUPPORTED, "%s: at most %d planes", who, DEPTH_FRAC_MAX);
  };
  const auto sample_bytes = [&] { return cube_sample_bytes_check(who, format, face_size, num_planes); };
  unsigned grid;
  if (const int e = check_views(a, planes, sample_bytes, &grid)) return e;
  if (batch == 0) return MSI_OK;
  const DepthFrac F = depth_fractions(num_planes);
  hipStream_t s = msi::as_stream(stream);
  const auto launch = [&](auto M, auto CAM, auto FMT) {
    const auto go = [&](auto kernel) {
      hipLaunchKernelGGL(kernel, dim3(grid), dim3(64, 4), 0, s, layers, tgt_pose_rt, tgt_pos, camera_table, stack_intrinsics, depths, trig, batch,
                         views, face_size, num_planes, out_height, out_width, out_rgb, out_depth, F, status_device);
    };
    if (filtering) go(cube_render_views_seamless_kernel<decltype(M)::value, decltype(CAM)::value, decltype(FMT)::value>);
    else go(cube_render_views_kernel<decltype(M)::value, decltype(CAM)::value, decltype(FMT)::value>);
  };
  for_view_kernel(render_mode(out_rgb, out_depth), format, ods, camera, launch);
  return msi::check_launch(who);
}

int msi_cube_render_views(const void *layers, int32_t format, const float *tgt_pose_rt, const float *tgt_pos,
                          const float *tgt_intrinsics, const float *stack_intrinsics, const float *depths, const float *trig,
                          int32_t batch, int32_t views, int32_t face_size, int32_t num_planes, int32_t camera,
                          int32_t out_height, int32_t out_width, float *out_rgb, float *out_depth, int32_t *status_device,
                          msi_stream_t stream) {
  return cube_views_launch("cube_render_views", false, 0, layers, format, tgt_pose_rt, tgt_pos, tgt_intrinsics, stack_intrinsics, depths, trig, batch,
                           views, face_size, num_planes, camera, out_height, out_width, out_rgb, out_depth, status_device, stream);
}

int msi_cube_render_views_seamless(const void *layers, int32_t format, const float *tgt_pose_rt, const float *tgt_pos,
                                   const float *tgt_intrinsics, const float *stack_intrinsics, const float *depths, const float *trig,
                                   int32_t batch, int32_t views, int32_t face_size, int32_t num_planes, int32_t camera,
                                   int32_t out_height, int32_t out_width, float *out_rgb, float *out_depth, int32_t *status_device,
                                   msi_stream_t stream) {
  return cube_views_launch("cube_render_views", false, 1, layers, format, tgt_pose_rt, tgt_pos, tgt_intrinsics, stack_intrinsics, depths, trig, batch,
                           views, face_size, num_planes, camera, out_height, out_width, out_rgb, out_depth, status_device, stream);
}

int msi_cube_render_ods_views(const void *layers, int32_t format, const float *tgt_pose_rt, const float *tgt_pos, const float *eye_radius,
                              const float *stack_intrinsics, const float *depths, const float *trig, int32_t batch, int32_t views,
                              int32_t face_size, int32_t num_planes, int32_t filtering, int32_t out_height, int32_t out_width, float *out_rgb,
                              float *out_depth, int32_t *status_device, msi_stream_t stream) {
  return cube_views_launch("cube_render_ods_views", true, filtering, layers, format, tgt_pose_rt, tgt_pos, eye_radius, stack_intrinsics, depths, trig,
                           batch, views, face_size, num_planes, MSI_CAMERA_EQUIRECT, out_height, out_width, out_rgb, out_depth, status_device, stream);
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
