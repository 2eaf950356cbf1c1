// Shared by the translation units of the geometry-side kernels of the MSI infer->render path for gfx950 (HBM-bound), one unit per kernel family:
//   geo_prep.hip    K5 pre/deprocess (single and pair), pose composition, the host-built trig tables
//   geo_sweep.hip   K1 ODS sphere sweep: ods_sweep_kernel, ods_sweep_lds_kernel
//   geo_layers.hip  K3 RGBA assembly, bilinear resize, the fused high-res layer stack, pack / unpack of the compact stacks
//   geo_render.hip  K4 fused reprojection + wrap-around bilinear gather + over-composite: render_kernel, render_views_kernel and its packed form
//   geo_ods.hip     K4 with the ODS stereo camera: render_ods_views_kernel (both eyes of a stack per launch, fp32 or packed stacks)
//   geo_sparse.hip  the sparse layer stacks' format: the tile index (both keep rules) / gather / expand kernels.  geo_sparse.h: what the three sparse units share
//   geo_sparse_hres.hip   the high-res stack built sparse (hres_keep_kernel, hres_layers_sparse_kernel)
//   geo_sparse_views.hip  K4 from a sparse stack: render_views_sparse_kernel (the cameras of render and ods); the planar and cube renders from one
//   geo_factored.hip      K4 from the FACTORS of a high-res stack, no stack in memory: render_views_factored_kernel
//   geo_mip.hip           mip-mapped stacks: build_mips_kernel (the pyramid of a stack in one launch) and K4 with a trilinear texel, render_views_mip_kernel
//   geo_planar.hip  the PP path: perspective plane sweeps, the MPI render and its many-views form (fp32 or packed stacks)
//   geo_planar_hres.hip   the PP high-res stack in one pass, dense or sparse: pp_hres_layers_kernel, pp_hres_layers_sparse_kernel
//   geo_cube.hip    the cube-map viewer of the PP path: cube_render_views_kernel (six face stacks as one panorama or headset view), equirect_to_cube_kernel
//                   (geo_cube.h: the cube conventions and the pieces of the cube pixel, for this unit and geo_sparse_views.hip's cube kernel)
//   geo_cube_sweep.hip    the cube path's source half sampled from the source PANORAMA, across face edges: cube_sweep_kernel, cube_sweep_volume_bf16_kernel,
//                         cube_hres_layers_kernel, cube_hres_layers_sparse_kernel
// Here: ONLY what more than one family uses (anonymous namespace: every unit inlines its own copy); each block says who shares it and why the
// sharing is a contract.  What a single family uses lives in that family's unit.
//
// Every unit that includes this header is compiled with -ffp-contract=off (build.py GEO_UNITS): the reference evaluates every
// elementwise TF op separately in fp32 (no FMA contraction), and project_ods'
// discriminant is ill-conditioned enough that a contracted
// multiply-add flips the `disc >= 0` branch on ~1% of far-plane pixels.  With the
// reference's operation order, IEEE sqrt/div (hipcc default) and the host-built
// trig tables, every branch below is bit-reproducible against the CPU oracle.
#pragma once
#include <cmath>
#include <cstdint>
#include <cstdlib>
#include <type_traits>

#include "msi_common.h"

namespace {

// ---- sweep, layers (hres_layers_kernel), render, planar: the pixel-coordinate constants, the wrap-around bilinear taps and the fast continuous tail.
// Contract: a sample position and its four corner weights have the same bits in every kernel that resamples an image or a layer.
// fp32 constants the reference folds from Python doubles (spherical.py:54-68,
// :222-223), rounded once on the host.
struct PixConsts {
  float pi, pi_over_w, u_den, wm1;          // u = ((theta + pi) - pi/W) / (2pi - 2pi/W) * (W-1)
  float half_pi, half_pi_over_h, v_den, hm1;  // v = ((phi + pi/2) - (pi/2)/H) / (pi - pi/H) * (H-1)
  float u_scale, v_scale;                   // (W-1) / u_den, (H-1) / v_den, rounded once from fp64 (fast tail)
};

PixConsts make_consts(int height, int width) {
  const double PI = 3.14159265358979323846;
  PixConsts k;
  k.pi = (float)PI;
  k.pi_over_w = (float)(PI / width);
  k.u_den = (float)(2 * PI - 2 * PI / width);
  k.wm1 = (float)(width - 1);
  k.half_pi = (float)(0.5 * PI);
  k.half_pi_over_h = (float)(0.5 * PI / height);
  k.v_den = (float)(PI - PI / height);
  k.hm1 = (float)(height - 1);
  k.u_scale = (float)((double)(width - 1) / (2 * PI - 2 * PI / width));
  k.v_scale = (float)((double)(height - 1) / (PI - PI / height));
  return k;
}

// tf.mod on int32 = floor-mod.  Pixel coordinates that come out of the angle formulas lie in
// [-1, n], so the index (a = x + n) is in [n-1, 2n]: one conditional subtract; anything else (only
// reachable through NaN/inf garbage) takes the generic integer-division path (~20 instructions,
// which used to be paid 4x per bilinear lookup).
__device__ __forceinline__ int floor_mod(int a, int n) {
  if (a >= 0 && a < 2 * n) return a >= n ? a - n : a;
  int m = a % n;
  return m < 0 ? m + n : m;
}

// Corner indices and area weights of sampling.resample (sampling.py:150-165,
// 187-190): weights from the UNWRAPPED corners, indices wrapped in both axes.
struct Taps {
  int x0, x1, y0, y1;
  float wa, wb, wc, wd;
};

__device__ __forceinline__ Taps make_taps(float x, float y, int width, int height) {
  Taps t;
  const float fx0 = floorf(x), fy0 = floorf(y);
  const int x0 = (int)fx0, y0 = (int)fy0;
  const int x1 = x0 + 1, y1 = y0 + 1;
  const float dx0 = x - (float)x0, dy0 = y - (float)y0;
  const float dx1 = (float)x1 - x, dy1 = (float)y1 - y;
  t.x0 = floor_mod(x0 + width, width);
  t.y0 = floor_mod(y0 + height, height);
  t.x1 = floor_mod(x1 + width, width);
  t.y1 = floor_mod(y1 + height, height);
  t.wa = dy1 * dx1;
  t.wb = dy1 * dx0;
  t.wc = dy0 * dx1;
  t.wd = dy0 * dx0;
  return t;
}

// make_taps for coordinates that lie in [-1, n] by construction -- the sweep and the render derive them from angles
// (theta in [-pi, pi], phi clamped / in [-pi/2, pi/2]  =>  u in [-0.5, W-0.5], v in [-0.5, H-0.5]) -- so the floor-mod
// is one unsigned min per corner, nothing branches, and the corner positions are 24-bit pixel offsets (row * W + col,
// full-rate v_mul_u32_u24; the host checks H * W < 2^24) for 32-bit buffer addressing: the generic form above spent
// a quarter of these VALU-bound kernels in 64-bit address multiplies and exec-masked division fall-backs.
// Weights as above (unwrapped corners; (float)(int)floor(x) == floor(x) in this range); garbage inputs (NaN -> 0, inf)
// are clamped into the image instead of taking the reference's undefined int cast.
// The ONE definition of the clamp and the wrap is make_taps_xy: the wrapped corner COORDINATES and the weights, for the renders that address a
// texel by (row, column) -- the sparse viewer's tiles (geo_sparse_views.hip), the factored viewer's texel function (FactoredSphereStack below);
// make_taps_ranged folds them into flat texel offsets.
struct TapsXY {
  unsigned x0, x1, y0, y1;
  float wa, wb, wc, wd;
};

__device__ __forceinline__ TapsXY make_taps_xy(float x, float y, int width, int height) {
  TapsXY t;
  const float fx0 = floorf(x), fy0 = floorf(y);
  const float dx0 = x - fx0, dy0 = y - fy0;
  const float dx1 = (fx0 + 1.0f) - x, dy1 = (fy0 + 1.0f) - y;
  t.wa = dy1 * dx1;
  t.wb = dy1 * dx0;
  t.wc = dy0 * dx1;
  t.wd = dy0 * dx0;
  const int x0 = max(-1, min((int)fx0, width - 1)), y0 = max(-1, min((int)fy0, height - 1));
  const unsigned ax = (unsigned)(x0 + width), ay = (unsigned)(y0 + height);
  t.x0 = min(ax, ax - (unsigned)width); t.y0 = min(ay, ay - (unsigned)height);   // -1 -> n-1
  const unsigned bx = (unsigned)(x0 + 1), by = (unsigned)(y0 + 1);
  t.x1 = min(bx, bx - (unsigned)width); t.y1 = min(by, by - (unsigned)height);   // n -> 0
  return t;
}

struct TapsR {
  unsigned oa, ob, oc, od;   // pixel offsets of (y0,x0) (y0,x1) (y1,x0) (y1,x1)
  float wa, wb, wc, wd;
};

__device__ __forceinline__ TapsR make_taps_ranged(float x, float y, int width, int height) {
  const TapsXY c = make_taps_xy(x, y, width, height);
  TapsR t;
  t.wa = c.wa; t.wb = c.wb; t.wc = c.wc; t.wd = c.wd;
  const unsigned r0 = __umul24(c.y0, (unsigned)width), r1 = __umul24(c.y1, (unsigned)width);
  t.oa = r0 + c.x0; t.ob = r0 + c.x1; t.oc = r1 + c.x0; t.od = r1 + c.x1;
  return t;
}

__device__ __forceinline__ float blend4(const TapsR &t, float a, float b, float c, float d) {
  return ((t.wa * a + t.wb * b) + t.wc * c) + t.wd * d;
}

__device__ __forceinline__ float blend4(const TapsXY &t, float a, float b, float c, float d) {
  return ((t.wa * a + t.wb * b) + t.wc * c) + t.wd * d;
}

__device__ __forceinline__ float blend4(const Taps &t, float a, float b, float c, float d) {
  // tf.add_n([area_a*A, area_b*B, area_c*C, area_d*D]) summed in list order.
  return ((t.wa * a + t.wb * b) + t.wc * c) + t.wd * d;
}

// ---- the CONTINUOUS tail of the angle math ----------------------------------------------------------
// Everything that feeds a branch of the reference (|z| > |x|, sign(pz), disc >= 0: the quadratic of project_ods up
// to `disc`) is evaluated op for op in IEEE fp32 above / below.  What follows the branches -- the root, the direction,
// the two angles and the pixel coordinates -- is a continuous function of its inputs, so 1-ulp primitives
// (v_rcp_f32 + one Newton step, v_sqrt_f32, a degree-7 odd minimax atan, 1.3e-7 rad) move a sample by <= 2e-5 px,
// i.e. the bilinear result by ~1e-5 of the image range (tolerance 1e-3), and cost a third of the IEEE sequences
// (the sweep and the render are VALU-bound: ~470 / ~260 instructions per sample with libm atan2f and IEEE
// divide / sqrt, profiles/r01_*).  -DMSI_FAST_TAIL=0 restores the IEEE / libm tail.
#ifndef MSI_FAST_TAIL
#define MSI_FAST_TAIL 1
#endif

__device__ __forceinline__ float t_sqrt(float x) {
#if MSI_FAST_TAIL
  return __builtin_amdgcn_sqrtf(x);
#else
  return sqrtf(x);
#endif
}

__device__ __forceinline__ float t_div(float a, float b) {
#if MSI_FAST_TAIL
  const float r = __builtin_amdgcn_rcpf(b);
  const float q = a * r;
  return __builtin_fmaf(__builtin_fmaf(-q, b, a), r, q);   // one correction step: <= 1 ulp for normal operands
#else
  return a / b;
#endif
}

// atan on [-1, 1] (an odd polynomial of degree 15, 1.3e-7 rad) and the two angles of a point (x, y, z) with
// horizontal distance h = sqrt(x^2 + z^2) and norm R through half-angle forms, tan(a / 2) = sin a / (1 + cos a):
//   atan2(y, h) = 2 atan(y / (h + R))                       (|phi| <= pi/2: the argument is in [-1, 1] as it is)
//   atan2(z, x) = 2 atan(z / (h + x))            for x >= 0,
//               = copysign(pi, z) - 2 atan(z / (h - x))  for x < 0   (both arguments in [-1, 1])
// -- no min / max / swap range reduction, no quadrant fix-ups, one shared square root: ~14 instead of ~30 instructions
// per angle in the render kernel, which is bound by its VALU stream.  Same 1.3e-7 rad polynomial (doubled: 2.6e-7 rad =
// 3e-5 px at W = 640); atan2(+-0, +-0) = +-0 like libm's for (+0, +0).  Used by the render kernel (no data-dependent reference
// branch in its chain, finite inputs) and, since r04, by the sweep's continuous tail (ods_tail): there the angles feed floor() of
// the pixel coordinates, so a sample within 3e-5 px of an integer may take the neighbouring tap pair -- with weights (1 - eps, eps)
// against (eps', 1 - eps') on the same two texels, i.e. the bilinear value moves by <= 3e-5 of a texel difference (the resample is
// continuous across tap boundaries); the reference's branch-deciding values (disc, |z| > |x|, sign(pz)) are computed before this,
// IEEE op for op.  NaN inputs (disc < 0 pixels) produce NaN / garbage angles that ods_tail overrides as the reference does.
__device__ __forceinline__ float t_atan_unit(float a) {
  const float s = a * a;
  float p = -0.0040545277297496796f;
  p = __builtin_fmaf(p, s, 0.021862812340259552f);
  p = __builtin_fmaf(p, s, -0.05591211095452309f);
  p = __builtin_fmaf(p, s, 0.09642180800437927f);
  p = __builtin_fmaf(p, s, -0.13908623158931732f);
  p = __builtin_fmaf(p, s, 0.19946564733982086f);
  p = __builtin_fmaf(p, s, -0.33329859375953674f);
  p = __builtin_fmaf(p, s, 0.9999993443489075f);
  return p * a;
}

__device__ __forceinline__ void t_angles(float x, float y, float z, float R, float &theta_neg, float &phi) {
#if MSI_FAST_TAIL
  const float h = __builtin_amdgcn_sqrtf(x * x + z * z);
  const float den = fmaxf(h + fabsf(x), 1.17549435e-38f);               // (x = z = 0: 0 / tiny = 0)
  const float a2 = 2.0f * t_atan_unit(z * __builtin_amdgcn_rcpf(den));
  const float th = __builtin_signbitf(x) ? __builtin_copysignf(3.14159265358979324f, z) - a2 : a2;
  theta_neg = -th;
  phi = 2.0f * t_atan_unit(y * __builtin_amdgcn_rcpf(h + R));
#else
  theta_neg = -atan2f(z, x);
  phi = atan2f(y, sqrtf(x * x + z * z));
#endif
}

// ---- sweep, layers (assemble_kernel reads the bf16 volume), planar: ONE bf16 rounding for every kernel that writes or reads a bf16 volume.
// fp32 <-> bf16 (round to nearest even; the values stored here are finite)
__device__ __forceinline__ unsigned short f32_to_bf16(float f) {
  const unsigned u = __builtin_bit_cast(unsigned, f);
  return (unsigned short)((u + 0x7fffu + ((u >> 16) & 1u)) >> 16);
}
__device__ __forceinline__ float bf16_to_f32(unsigned short h) {
  return __builtin_bit_cast(float, (unsigned)h << 16);
}
__device__ __forceinline__ void store_elem(float *p, size_t i, float v) { p[i] = v; }
__device__ __forceinline__ void store_elem(unsigned short *p, size_t i, float v) { p[i] = f32_to_bf16(v); }

// ---- sweep and layers: hres_layers_kernel must produce the bits of ods_sweep_kernel -> resize -> assemble, so it runs THESE functions, op for op.
// ------------------------------------------------------------------------ K1
// project_ods (spherical.py:181-229) in two parts.
// (1) ods_quad: everything up to the discriminant, op for op in IEEE fp32 (no contraction: every unit that includes this header is compiled with
//     -ffp-contract=off) -- it decides the reference's three branches (|z| > |x|, sign(pz), disc >= 0), and `disc` is
//     ill conditioned, so not one rounding may differ from the oracle here.
// (2) ods_tail: root, ray direction, angles, pixel coordinates -- continuous in (a, bq, f, px, pz, disc), evaluated
//     with the 1-ulp primitives above.  It is the only part that depends on `order`, so when both sources of the sweep
//     volume have the same pose (the test path: identity poses, msi.py:1125) they share (1).
struct OdsQuad {
  float f, px, pz, a, bq, disc, y;
  bool zlx;
};

__device__ __forceinline__ OdsQuad ods_quad(const float *__restrict__ P, float r, float depth, float csct, float st, float ssct) {
  OdsQuad q;
  // backproject_spherical (spherical.py:125-128)
  float x = depth * csct;
  float y = depth * st;
  float z = depth * ssct;
  // apply_pose (projector.py:275-291): pose @ [x,y,z,1], terms summed left to right
  const float px_ = ((P[0] * x + P[1] * y) + P[2] * z) + P[3] * 1.0f;
  const float py_ = ((P[4] * x + P[5] * y) + P[6] * z) + P[7] * 1.0f;
  const float pz_ = ((P[8] * x + P[9] * y) + P[10] * z) + P[11] * 1.0f;
  x = px_;
  y = py_;
  z = pz_;
  // project_ods (spherical.py:181-192)
  q.f = r * r - (x * x + z * z);
  q.zlx = fabsf(z) > fabsf(x);
  q.px = q.zlx ? x : z;
  q.pz = q.zlx ? z : x;
  const float pz2 = q.pz * q.pz;
  q.a = 1.0f + (q.px * q.px) / pz2;
  q.bq = ((-2.0f * q.f) * q.px) / pz2;
  const float c = q.f + (q.f * q.f) / pz2;
  q.disc = q.bq * q.bq - (4.0f * q.a) * c;
  q.y = y;
  return q;
}

// (spherical.py:195-229) -> pixel coordinates (u, v); (1, 1) where disc < 0 or NaN
__device__ __forceinline__ void ods_tail(const OdsQuad &q, float order, const PixConsts &K, float &u, float &v) {
  const float sgn = (q.pz > 0.0f) ? 1.0f : ((q.pz < 0.0f) ? -1.0f : q.pz);
  float s = ((-order) * sgn) * t_sqrt(q.disc);
  s = q.zlx ? s : -s;
  float dx = t_div(-q.bq + s, 2.0f * q.a);
  float dz = t_div(q.f - q.px * dx, q.pz);
  const float dxf = q.zlx ? -dx : -dz;
  const float dzf = q.zlx ? -dz : -dx;
  dx = dxf;
  dz = dzf;
#if MSI_FAST_TAIL
  // (r04: the render kernel's half-angle forms -- one square root more, two range reductions less than two atan2; where disc < 0 everything
  // here is NaN or garbage and the override below applies, as before)
  float theta, phi;
  t_angles(dx, q.y, dz, t_sqrt((dx * dx + dz * dz) + q.y * q.y), theta, phi);
#else
  const float theta = -atan2f(dz, dx);
  float phi = atan2f(q.y, t_sqrt(dx * dx + dz * dz));
#endif
  if (phi != phi) phi = 1.0f;
  phi = (phi <= K.half_pi) ? phi : K.half_pi;
  phi = (phi >= -K.half_pi) ? phi : -K.half_pi;
#if MSI_FAST_TAIL
  u = ((theta + K.pi) - K.pi_over_w) * K.u_scale;
  v = ((phi + K.half_pi) - K.half_pi_over_h) * K.v_scale;
#else
  u = (((theta + K.pi) - K.pi_over_w) / K.u_den) * K.wm1;
  v = (((phi + K.half_pi) - K.half_pi_over_h) / K.v_den) * K.hm1;
#endif
  if (!(q.disc >= 0.0f)) {
    u = 1.0f;
    v = 1.0f;
  }
}

// resample (sampling.py:135-197) of one RGB texel; `img` = buffer descriptor of one sample's [H,W,3] image.
// The four corners as BYTE offsets (pixel offset x 12, 24-bit multiply) + area weights: everything of a sample that does
// not depend on the image -- kept in registers while the frames of a batch that share (pose, baseline) are gathered.
typedef unsigned u32x3_g __attribute__((ext_vector_type(3)));
typedef float f32x3_g __attribute__((ext_vector_type(3)));
struct TapsB {
  unsigned oa, ob, oc, od;
  float wa, wb, wc, wd;
};
__device__ __forceinline__ TapsB make_taps_bytes(float u, float v, int width, int height) {
  const TapsR t = make_taps_ranged(u, v, width, height);
  TapsB r;
  r.oa = __umul24(t.oa, 12u); r.ob = __umul24(t.ob, 12u); r.oc = __umul24(t.oc, 12u); r.od = __umul24(t.od, 12u);
  r.wa = t.wa; r.wb = t.wb; r.wc = t.wc; r.wd = t.wd;
  return r;
}
__device__ __forceinline__ float blend4(const TapsB &t, float a, float b, float c, float d) {
  return ((t.wa * a + t.wb * b) + t.wc * c) + t.wd * d;   // tf.add_n order (sampling.py:187-190)
}
// (the four loads and the three blends apart: hres_layers_sparse_kernel keeps the loads of one layer in flight while it blends another)
struct Rgb4 { f32x3_g a, b, c, d; };
__device__ __forceinline__ Rgb4 gather3_load(__amdgpu_buffer_rsrc_t img, const TapsB &t) {
  Rgb4 g;
  g.a = __builtin_bit_cast(f32x3_g, (u32x3_g)__builtin_amdgcn_raw_buffer_load_b96(img, t.oa, 0, 0));
  g.b = __builtin_bit_cast(f32x3_g, (u32x3_g)__builtin_amdgcn_raw_buffer_load_b96(img, t.ob, 0, 0));
  g.c = __builtin_bit_cast(f32x3_g, (u32x3_g)__builtin_amdgcn_raw_buffer_load_b96(img, t.oc, 0, 0));
  g.d = __builtin_bit_cast(f32x3_g, (u32x3_g)__builtin_amdgcn_raw_buffer_load_b96(img, t.od, 0, 0));
  return g;
}
__device__ __forceinline__ void gather3_blend(const TapsB &t, const Rgb4 &g, float *out) {
  out[0] = blend4(t, g.a.x, g.b.x, g.c.x, g.d.x);
  out[1] = blend4(t, g.a.y, g.b.y, g.c.y, g.d.y);
  out[2] = blend4(t, g.a.z, g.b.z, g.c.z, g.d.z);
}
__device__ __forceinline__ void gather3(__amdgpu_buffer_rsrc_t img, const TapsB &t, float *out) { gather3_blend(t, gather3_load(img, t), out); }

// ---- sweep, layers (pack / unpack / hres) and planar: the 16-byte store of every streaming kernel; its host side is beyond_infinity_cache below.
// The 16-byte pieces of a wave's whole-pixel strip.  nt != 0 (block-uniform; the host sets it when the volume is larger than the 256-MB Infinity Cache): non-temporal
// stores -- a volume that cannot stay cached until conv1_1 reads it should not evict what can (r06, same-box A/B at configs[2]: sweep 1.07 -> 0.98 ms per 16 frames;
// configs[3] -1 %; at batch 1 the 157-MB volume stays cached and keeps plain stores).
__device__ __forceinline__ void sweep_store16(uint4 *dst, const uint4 &v, int nt) {
  if (nt) {
    __builtin_nontemporal_store(v.x, &dst->x); __builtin_nontemporal_store(v.y, &dst->y); __builtin_nontemporal_store(v.z, &dst->z); __builtin_nontemporal_store(v.w, &dst->w);
  } else {
    *dst = v;
  }
}

// ---- layers (hres_layers_kernel) and sparse (hres_keep_kernel, hres_layers_sparse_kernel): ONE definition of a texel of the high-res stack, so the
// tiles a sparse stack keeps and the codes in them are the dense stack's, bit for bit.  The texel is the sweep's functions above, the resize's
// expression and the assembly's blend in the order of the three launches the dense kernel replaced (geo_layers.hip tells that story).
// Layers per group (one G-float vector per low-res corner; the group is unrolled) and the waves per SIMD the register allocation aims at.  What hides the gathers'
// latency is the independent samples a lane has in flight, not the wave count (same-box A/B, DESIGN.md section 4, profiles/hres_layers_variants.txt): G = 4 at four waves
// (101-103 VGPRs) 2.3 ms at 4096x2048x32, G = 2 at five waves the same there and 1.9 x slower at 1280x640, G = 1 at six waves 1.7 x / 2.8 x slower; G = 4 at five waves spills.
#ifndef MSI_HRES_GROUP   // (tuning: -DMSI_HRES_GROUP=1 / 2 / 4)
#define MSI_HRES_GROUP 4
#endif
#ifndef MSI_HRES_WAVES   // (tuning: -DMSI_HRES_WAVES=4 / 5)
#define MSI_HRES_WAVES 4
#endif

// tf.image.resize(..., BILINEAR, align_corners=True) [TF-knowledge: resize_bilinear_op]:
// src = dst * (in-1)/(out-1); lower = floor(src), upper = min(ceil(src), in-1), lerp = src - lower;
// top = tl + (tr - tl)*xl; bottom = bl + (br - bl)*xl; out = top + (bottom - top)*yl.
// Used by the high-res re-render to upsample blend weights / alphas (test.py:319-325).
// The ONE definition of that expression, for a float (resize_bilinear_kernel, per component) or a vector of layers (the hres kernels, elementwise).
template <typename T>
__device__ __forceinline__ T lerp2(T tl, T tr, T bl, T br, float xl, float yl) {
  const T top = tl + (tr - tl) * xl;
  const T bot = bl + (br - bl) * xl;
  return top + (bot - top) * yl;
}

constexpr int HRES_G = MSI_HRES_GROUP;
typedef float hres_vec __attribute__((ext_vector_type(HRES_G)));

// the resize's corners (element offsets of layer 0 in a [h,w,D] low-res tensor) and fractions of high-res pixel (i, j) (resize_bilinear_kernel; sy, sx
// from the host as in msi_resize_bilinear_f32)
struct HresAxis {   // along one axis: the two low-res coordinates a high-res coordinate lies between (both non-decreasing in it) and the fraction
  int lo, hi;
  float frac;
};
__device__ __forceinline__ HresAxis hres_axis(int i, float s, int low_n) {
  HresAxis a;
  const float f = (float)i * s;
  a.lo = (int)floorf(f);
  a.hi = min((int)ceilf(f), low_n - 1);
  a.frac = f - (float)a.lo;
  return a;
}
struct HresCorners {
  unsigned tl, tr, bl, br;
  float xl, yl;
};
__device__ __forceinline__ HresCorners hres_corners(int i, int j, float sy, float sx, int low_h, int low_w, int nd) {
  HresCorners c;
  const HresAxis y = hres_axis(i, sy, low_h), x = hres_axis(j, sx, low_w);
  c.yl = y.frac; c.xl = x.frac;
  c.tl = (unsigned)(y.lo * low_w + x.lo) * (unsigned)nd; c.tr = (unsigned)(y.lo * low_w + x.hi) * (unsigned)nd;      // (h * w * D < 2^31: checked on the host)
  c.bl = (unsigned)(y.hi * low_w + x.lo) * (unsigned)nd; c.br = (unsigned)(y.hi * low_w + x.hi) * (unsigned)nd;
  return c;
}
// HRES_G layers of a low-res tensor (p = its sample + the group's first layer) at those corners
__device__ __forceinline__ hres_vec hres_lerp(const float *__restrict__ p, const HresCorners &k) {
  const hres_vec a = *reinterpret_cast<const hres_vec *>(p + k.tl), b = *reinterpret_cast<const hres_vec *>(p + k.tr);
  const hres_vec c = *reinterpret_cast<const hres_vec *>(p + k.bl), d = *reinterpret_cast<const hres_vec *>(p + k.br);
  return lerp2(a, b, c, d, k.xl, k.yl);         // (elementwise: the resize's expression)
}

template <int FMT, int NT>
__device__ __forceinline__ void hres_store_packed(void *__restrict__ base, size_t texel, const float4 &t) {
  if constexpr (FMT == MSI_LAYERS_RGBA8) {
    unsigned *p = static_cast<unsigned *>(base) + texel;
    const unsigned q = rgba8_encode(t);
    if (NT) __builtin_nontemporal_store(q, p); else *p = q;
  } else {
    u32x2_g *p = static_cast<u32x2_g *>(base) + texel;
    const u32x2_g q = rgba16f_encode(t);
    if (NT) __builtin_nontemporal_store(q, p); else *p = q;
  }
}

// A texel in three steps, each a function of the one before: where its two samples lie (taps), their eight texels (fetch: gather3_load x 2), and the
// blend (hres_blend: gather3_blend; assemble_kernel, COLOR_BLEND_PSV with pred_scaled).  The first two belong to the SOURCE of the stack -- the ODS
// pair, the PP pair, a cube face and its panorama -- and every source is one type of the same shape:
//   its members       what pixel (b, i, j) of an [B,D,height,width] stack has for all its layers (computed once, by the function that returns it)
//   taps(depth)       the sample positions of the texel at that depth, as byte offsets and weights; a source's own shortcuts live here
//   fetch(taps)       the eight 12-byte loads
// hres_texel is the three in a row, the dense builders' texel; the sparse builders call the steps.
struct HresTaps { TapsB fg, bg; };
struct HresRgb { Rgb4 fg, bg; };

// The ODS source (hres_layers_kernel, hres_layers_sparse_kernel): the sweep's per-pixel constants (ods_sweep_kernel), the two images, the two poses;
// taps = ods_quad / ods_tail / make_taps_bytes per image.
struct OdsHres {
  int b, i, j, height, width;
  const PixConsts &K;                           // the kernel's own argument (a copy moves its loads): K must outlive the source
  const float *P0, *P1;
  __amdgpu_buffer_rsrc_t img0, img1;
  float r, csct, st, ssct;
  bool same;                                    // both sources share the quadratic when their poses are equal
  __device__ __forceinline__ HresTaps taps(float depth) const {
    HresTaps t;
    float u, v;
    const OdsQuad q0 = ods_quad(P0, r, depth, csct, st, ssct);
    ods_tail(q0, 1.0f, K, u, v);
    t.fg = make_taps_bytes(u, v, width, height);
    if (same) {
      ods_tail(q0, -1.0f, K, u, v);
    } else {
      const OdsQuad q1 = ods_quad(P1, r, depth, csct, st, ssct);
      ods_tail(q1, -1.0f, K, u, v);
    }
    t.bg = make_taps_bytes(u, v, width, height);
    return t;
  }
  __device__ __forceinline__ HresRgb fetch(const HresTaps &t) const {
    HresRgb g;
    g.fg = gather3_load(img0, t.fg);
    g.bg = gather3_load(img1, t.bg);
    return g;
  }
};
__device__ __forceinline__ OdsHres ods_hres(const float *__restrict__ image0, const float *__restrict__ image1, const float *__restrict__ pose0,
                                            const float *__restrict__ pose1, const float *__restrict__ intrinsics, const float *__restrict__ trig,
                                            const PixConsts &K, int b, int i, int j, int height, int width) {
  OdsHres p{b, i, j, height, width, K};
  const float cs = trig[j], ss = trig[width + j];
  const float ct = trig[2 * width + i];
  p.st = trig[2 * width + height + i];
  p.csct = cs * ct; p.ssct = ss * ct;
  const int img_bytes = height * width * 12;
  p.P0 = pose0 + (size_t)b * 16; p.P1 = pose1 + (size_t)b * 16;
  p.img0 = __builtin_amdgcn_make_buffer_rsrc((void *)(image0 + (size_t)b * height * width * 3), 0, img_bytes, 0x00020000);
  p.img1 = __builtin_amdgcn_make_buffer_rsrc((void *)(image1 + (size_t)b * height * width * 3), 0, img_bytes, 0x00020000);
  p.r = intrinsics[(size_t)b * 9];
  p.same = true;
#pragma unroll
  for (int k = 0; k < 12; ++k) p.same = p.same && (p.P0[k] == p.P1[k]);
  return p;
}

__device__ __forceinline__ float4 hres_blend(const HresTaps &t, const HresRgb &g, float w, float alpha) {
  float fg[3], bg[3];
  gather3_blend(t.fg, g.fg, fg);
  gather3_blend(t.bg, g.bg, bg);
  const float omw = 1.0f - w;
  float4 o;
  o.x = w * fg[0] + omw * bg[0];
  o.y = w * fg[1] + omw * bg[1];
  o.z = w * fg[2] + omw * bg[2];
  o.w = alpha;
  return o;
}
template <class Source>
__device__ __forceinline__ float4 hres_texel(const Source &src, float depth, float w, float alpha) {
  const HresTaps t = src.taps(depth);
  return hres_blend(t, src.fetch(t), w, alpha);
}


// ---- planar (pp_sweep_kernel, pp_sweep_volume_bf16_kernel), planar-hres and cube-sweep: the steps of pj.perspective_plane_sweep (projector.py:221-223),
// each written ONCE, so that the fp32 sweeps, the bf16 volumes and the high-res builders of the PP and the cube path agree bit for bit.  No reciprocal,
// no fused multiply-add, no reassociation: the parentheses are the reference's order of operations.
struct Vec3 { float x, y, z; };
// backproject_planar (spherical.py:146-148): x = depth*S*cx/fx, y = depth*T*cy/fy, z = depth*1.  One axis (the bf16 sweeps stage y per plane) and the point.
__device__ __forceinline__ float backproject_axis(float depth, float s, float c, float f) { return ((depth * s) * c) / f; }
__device__ __forceinline__ Vec3 backproject_planar(float depth, float S, float T, float fx, float fy, float cx, float cy) {
  return Vec3{backproject_axis(depth, S, cx, fx), backproject_axis(depth, T, cy, fy), depth * 1.0f};
}
// apply_pose (projector.py:275-291): rows 0..2 of pose @ (x, y, z, 1), terms summed left to right
__device__ __forceinline__ Vec3 apply_pose(const float *P, const Vec3 &a) {
  return Vec3{((P[0] * a.x + P[1] * a.y) + P[2] * a.z) + P[3] * 1.0f, ((P[4] * a.x + P[5] * a.y) + P[6] * a.z) + P[7] * 1.0f,
              ((P[8] * a.x + P[9] * a.y) + P[10] * a.z) + P[11] * 1.0f};
}
// project_perspective (spherical.py:248-266): entry (r, c), r < 3, of M = K4 @ pose -- the 3x3 intrinsics Kb are zero-padded to 4x4 (projector.py:145-148),
// so the padded column contributes 0 * pose[3][c] -- and (u, v) = (pr0 / pr2, pr1 / pr2) of pr = M (x, y, z, 1) from rows 0..2 of M (m[12], registers or LDS)
__device__ __forceinline__ float k4_pose(const float *Kb, const float *P, int r, int c) {
  return ((Kb[r * 3 + 0] * P[c] + Kb[r * 3 + 1] * P[4 + c]) + Kb[r * 3 + 2] * P[8 + c]) + 0.0f * P[12 + c];
}
struct Uv { float u, v; };
__device__ __forceinline__ Uv project_rows(const float *m, const Vec3 &a) {
  float pr[3];
#pragma unroll
  for (int r = 0; r < 3; ++r) pr[r] = ((m[r * 4 + 0] * a.x + m[r * 4 + 1] * a.y) + m[r * 4 + 2] * a.z) + m[r * 4 + 3] * 1.0f;
  return Uv{pr[0] / pr[2], pr[1] / pr[2]};
}
// make_taps' four corners as byte offsets into one [H,W,3] image (H * W * 12 < 2^31: checked on the host), for gather3
__device__ __forceinline__ TapsB taps_bytes(const Taps &t, int width) {
  TapsB r;
  r.oa = (unsigned)(t.y0 * width + t.x0) * 12u; r.ob = (unsigned)(t.y0 * width + t.x1) * 12u;
  r.oc = (unsigned)(t.y1 * width + t.x0) * 12u; r.od = (unsigned)(t.y1 * width + t.x1) * 12u;
  r.wa = t.wa; r.wb = t.wb; r.wc = t.wc; r.wd = t.wd;
  return r;
}
// (the form without staged rows: M computed by the thread that uses it)
__device__ __forceinline__ Uv project_k4_pose(const float *Kb, const float *P, const Vec3 &a) {
  float m[12];
#pragma unroll
  for (int e = 0; e < 12; ++e) m[e] = k4_pose(Kb, P, e >> 2, e & 3);
  return project_rows(m, a);
}

// ---- planar and cube-sweep: what the plane sweeps of an image and of a cube's panorama share around their samplers -- a thread is sample idx = j * nd + d of
// row blockIdx.y of image blockIdx.z, grid = (ceil(W * D / 256), H, B) -- the decode and the stores.  FAST forms: full waves of complete pixels (the host decides).
struct PixelPlane { int j, d; };
// FAST: idx / nd by multiply-high with nd_magic = udiv_magic32(nd) (+ one correction); 32-bit index math only (64-bit div / mod are emulated in ~100 VALU
// instructions each and used to dominate the sweep)
template <int FAST> __device__ __forceinline__ PixelPlane sweep_pixel_plane(int idx, int nd, unsigned nd_magic) {
  int j;
  if (FAST) {
    unsigned jq = __umulhi((unsigned)idx, nd_magic);
    if ((unsigned)idx - jq * (unsigned)nd >= (unsigned)nd) ++jq;
    j = (int)jq;
  } else {
    j = idx / nd;
  }
  return PixelPlane{j, idx - j * nd};
}
// The fp32 sweeps' FAST store: whole-pixel runs through the wave's strip.  lane = (pixel of the wave, depth); the wave's 64 / D pixels are consecutive from
// row0 (the row's first pixel) + the wave's first, each owns 3 D contiguous floats at + coff: the strip IS the pixels' runs back to back, and lanes 0..47
// store 16 bytes each (non-temporal when the volume exceeds the Infinity Cache: sweep_store16).
__device__ __forceinline__ void sweep_strip_store(const float *o, long row0, int nd, float *__restrict__ psv, int channels, int coff, int nt) {
  __shared__ __attribute__((aligned(16))) float s_out[4][192];
  const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
  float *w = s_out[wave];
  __builtin_amdgcn_wave_barrier();
  w[lane * 3 + 0] = o[0]; w[lane * 3 + 1] = o[1]; w[lane * 3 + 2] = o[2];
  __builtin_amdgcn_wave_barrier();
  if (lane < 48) {
    const int vpp = (3 * nd) >> 2;                                         // 16-byte vectors per pixel run
    unsigned plq = __umulhi((unsigned)lane, 0xffffffffu / (unsigned)vpp + 1u);
    if ((unsigned)lane - plq * (unsigned)vpp >= (unsigned)vpp) --plq;      // (lane < 48, vpp >= 3: the estimate is exact or one too large)
    const int pl = (int)plq, k = lane - pl * vpp;
    const long pw0 = row0 + (long)((blockIdx.x * 256 + wave * 64) / nd);
    uint4 *dst = reinterpret_cast<uint4 *>(psv + (size_t)(pw0 + pl) * channels + coff) + k;
    sweep_store16(dst, reinterpret_cast<const uint4 *>(w)[lane], nt);
  }
}
// The bf16 volumes' store of pixel p, plane d: out[0] into channels [0, 3D), out[1] into [3D, 6D) of psv [.,6D].  FAST: the wave's 64 / D pixels are
// consecutive and each owns 6 D contiguous channels: lane = pl * D + d writes its two triples into a wave-private fp32 strip at pl * 6 D + {0, 3 D} + 3 d, then
// lanes 0..47 each pack 8 of the 384 values (v_cvt_pk_bf16_f32: round to nearest even, what f32_to_bf16 computes for the finite values stored here) into one
// 16-byte store.  Generic: six bf16 halves per thread.  NT is a template argument, not sweep_store16's runtime flag: with the packed value computed
// ahead of the branch, hipcc merges the two stores into one plain store.
template <int FAST, int NT>
__device__ __forceinline__ void sweep_volume_store_bf16(const float (&out)[2][3], long p, int d, int nd, int nd_shift, unsigned short *__restrict__ psv) {
  if (FAST) {
    __shared__ __attribute__((aligned(16))) float s_out[4][384];
    const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
    const int pl = lane >> nd_shift;
    float *w = s_out[wave];
    __builtin_amdgcn_wave_barrier();
    const int e0 = pl * 6 * nd + 3 * d;
#pragma unroll
    for (int c = 0; c < 3; ++c) {
      w[e0 + c] = out[0][c];
      w[e0 + 3 * nd + c] = out[1][c];
    }
    __builtin_amdgcn_wave_barrier();
    if (lane < 48) {
      const float4 lo = reinterpret_cast<const float4 *>(w)[2 * lane], hi = reinterpret_cast<const float4 *>(w)[2 * lane + 1];
      uint4 pk;
      asm("v_cvt_pk_bf16_f32 %0, %1, %2" : "=v"(pk.x) : "v"(lo.x), "v"(lo.y));
      asm("v_cvt_pk_bf16_f32 %0, %1, %2" : "=v"(pk.y) : "v"(lo.z), "v"(lo.w));
      asm("v_cvt_pk_bf16_f32 %0, %1, %2" : "=v"(pk.z) : "v"(hi.x), "v"(hi.y));
      asm("v_cvt_pk_bf16_f32 %0, %1, %2" : "=v"(pk.w) : "v"(hi.z), "v"(hi.w));
      uint4 *dst = reinterpret_cast<uint4 *>(psv + (size_t)(p - pl) * (6 * nd)) + lane;   // (p - pl: the wave's first pixel)
      sweep_store16(dst, pk, NT);
    }
    return;
  }
  unsigned short *o = psv + (size_t)p * (6 * nd) + 3 * d;
#pragma unroll
  for (int c = 0; c < 3; ++c) {
    o[c] = f32_to_bf16(out[0][c]);
    o[3 * nd + c] = f32_to_bf16(out[1][c]);
  }
}
// image b of an [B,H,W,3] batch as a range-checked buffer with 32-bit byte offsets (H * W * 12 < 2^31: checked on the host)
__device__ __forceinline__ __amdgpu_buffer_rsrc_t image_rsrc(const float *__restrict__ images, int b, int height, int width) {
  return __builtin_amdgcn_make_buffer_rsrc((void *)(images + (size_t)b * height * width * 3), 0, height * width * 12, 0x00020000);
}
// the sample of an image at pixel coordinates p through the reference's wrap-around sampler: one 12-byte buffer load per corner
__device__ __forceinline__ void wrap_gather3(__amdgpu_buffer_rsrc_t img, const Uv &p, int width, int height, float *out) {
  gather3(img, taps_bytes(make_taps(p.u, p.v, width, height), width), out);
}

// The fp32 plane sweep of one source into its 3 D channel window of psv [B,H,W,C] (pp_sweep_kernel: geo_planar.hip, which tells the story;
// cube_sweep_kernel: geo_cube_sweep.hip) is ONE body around the source's sampler: src.sample<FAST>(Kb, a, o) = the RGB of the source where the posed plane
// point a lands (its own pose src.P applied once already).  FAST: whole pixels through the wave's strip.
template <int FAST, class Source>
__device__ __forceinline__ void sweep_body(const Source &src, const float *intrinsics, const float *depths, int height, int width, int nd, float s0,
                                           float sstep, float t0, float tstep, float *psv, int channels, int coff, unsigned nd_magic, int nt) {
  const int idx = blockIdx.x * 256 + threadIdx.x;
  if (!FAST && idx >= width * nd) return;
  const PixelPlane q = sweep_pixel_plane<FAST>(idx, nd, nd_magic);
  const int i = blockIdx.y, b = blockIdx.z;
  const float *Kb = intrinsics + (size_t)b * 9;
  const long row0 = ((long)b * height + i) * width;
  const float S = s0 + sstep * (float)q.j, T = t0 + tstep * (float)i;
  float o[3];
  src.template sample<FAST>(Kb, apply_pose(src.P, backproject_planar(depths[q.d], S, T, Kb[0], Kb[4], Kb[2], Kb[5])), o);
  if (FAST) {
    sweep_strip_store(o, row0, nd, psv, channels, coff, nt);
    return;
  }
  float *dst = psv + (size_t)(row0 + q.j) * channels + coff + q.d * 3;
  dst[0] = o[0]; dst[1] = o[1]; dst[2] = o[2];
}

// The whole bf16 network input of a pair in one launch (pp_sweep_volume_bf16_kernel: geo_planar.hip, which tells the story;
// cube_sweep_volume_bf16_kernel: geo_cube_sweep.hip): ONE body.  The ref half is image0 through its own camera; the src half is Src's -- Src::CAMERA: a
// second image of the same camera (src.image, src.P: its M is staged next to the ref half's), else src.sample(a, o) as in sweep_body.  FAST
// (64 % D == 0, (W * D) % 64 == 0): M per face and camera source and backproject_planar's y per plane of this row are staged in LDS.
template <int FAST, int NT, class Src>
__device__ __forceinline__ void sweep_volume_bf16_body(const float *image0, const float *P0, const Src &src,
                                                       const float *intrinsics, const float *depths, int height, int width,
                                                       int nd, int nd_shift, float s0, float sstep, float t0, float tstep,
                                                       unsigned short *psv) {
  constexpr int NM = Src::CAMERA ? 2 : 1;
  const int idx = blockIdx.x * 256 + threadIdx.x;
  const int i = blockIdx.y, b = blockIdx.z;
  const float *Kb = intrinsics + (size_t)b * 9;
  const float fx = Kb[0], fy = Kb[4], cx = Kb[2], cy = Kb[5];
  const float T = t0 + tstep * (float)i;
  __shared__ float s_m[NM][12];
  __shared__ float s_y[64];
  if (FAST) {
    const int tid = threadIdx.x;
    if (tid < 12 * NM) {
      const int s = tid / 12, e = tid - s * 12;
      s_m[s][e] = k4_pose(Kb, s ? src.P : P0, e >> 2, e & 3);
    } else if (tid >= 64 && tid < 64 + nd) {
      s_y[tid - 64] = backproject_axis(depths[tid - 64], T, cy, fy);
    }
    __syncthreads();
    if (idx >= width * nd) return;   // (W * D) % 64 == 0: whole waves
  } else {
    if (idx >= width * nd) return;
  }
  const int j = FAST ? idx >> nd_shift : idx / nd;
  const int d = FAST ? idx & (nd - 1) : idx - j * nd;
  const float S = s0 + sstep * (float)j;
  const float depth = depths[d];
  // backproject_planar, shared by both halves
  const Vec3 point = Vec3{backproject_axis(depth, S, cx, fx), FAST ? s_y[d] : backproject_axis(depth, T, cy, fy), depth * 1.0f};
  float out[2][3];
  const auto camera = [&](int s, const float *image, const float *P) {
    const Vec3 a = apply_pose(P, point);
    wrap_gather3(image_rsrc(image, b, height, width), FAST ? project_rows(s_m[s], a) : project_k4_pose(Kb, P, a), width, height, out[s]);
  };
  camera(0, image0, P0);
  if constexpr (Src::CAMERA) camera(1, src.image, src.P);
  else src.template sample<FAST>(Kb, apply_pose(src.P, point), out[1]);
  sweep_volume_store_bf16<FAST, NT>(out, ((long)b * height + i) * width + j, d, nd, nd_shift, psv);
}

// ---- planar-hres (pp_hres_layers_kernel, pp_hres_layers_sparse_kernel: geo_planar_hres.hip): ONE definition of a texel of the PP high-res stack.  It is
// pp_sweep_kernel's arithmetic (geo_planar.hip), the steps above -- S and T of uv_grid, backproject_planar with its two divides, apply_pose, M = K4 @ pose,
// u = pr0 / pr2, v = pr1 / pr2, make_taps, blend4 -- once per source image (ref = foreground, src = background), then the steps every source ends with
// (hres_corners / hres_lerp, hres_blend, hres_store_packed): the bits of msi_perspective_plane_sweep_f32 x 2 -> msi_resize_bilinear_f32 ->
// msi_assemble_rgba_scaled_f32.
// K, both poses and both M depend on the sample alone: they are made wave-uniform (pp_uniform) so that they live in SGPRs, not in 60 VGPRs of every lane.
__device__ __forceinline__ float pp_uniform(float v) {   // (v is the same in every lane: a function of blockIdx.z)
  return __builtin_bit_cast(float, __builtin_amdgcn_readfirstlane(__builtin_bit_cast(int, v)));
}
struct PpHresSource {
  __amdgpu_buffer_rsrc_t img;
  const float *P;      // pose [4,4] of this source
  float m[12];         // rows 0..2 of K4 @ pose
};
__device__ __forceinline__ PpHresSource pp_hres_source(const float *__restrict__ image, const float *__restrict__ pose, const float *Kb, int b, int height,
                                                       int width) {
  PpHresSource s;
  s.P = pose + (size_t)b * 16;
  s.img = image_rsrc(image, b, height, width);
#pragma unroll
  for (int r = 0; r < 3; ++r)
#pragma unroll
    for (int c = 0; c < 4; ++c) s.m[r * 4 + c] = pp_uniform(k4_pose(Kb, s.P, r, c));
  return s;
}
// where the plane point of backproject_planar lands in one source: apply_pose, project_perspective, the wrap-around taps as byte offsets
__device__ __forceinline__ TapsB pp_hres_source_taps(const PpHresSource &s, const Vec3 &point, int width, int height) {
  const Uv p = project_rows(s.m, apply_pose(s.P, point));
  return taps_bytes(make_taps(p.u, p.v, width, height), width);      // (wrapped indices lie inside the image whatever u and v are)
}
// what the PP and the cube source share: pixel (b, i, j) of a stack of `height` x `width` images, its point S, T of uv_grid, the camera of sample b and
// the foreground image (ref image, ref pose)
struct PlanarHresPixel {
  int b, i, j, height, width;
  PpHresSource s0;
  float S, T, fx, fy, cx, cy;
  __device__ __forceinline__ Vec3 plane_point(float depth) const { return backproject_planar(depth, S, T, fx, fy, cx, cy); }
};
__device__ __forceinline__ PlanarHresPixel planar_hres_pixel(const float *__restrict__ image0, const float *__restrict__ pose0,
                                                             const float *__restrict__ intrinsics, int b, int i, int j, int height, int width, float s0,
                                                             float sstep, float t0, float tstep) {
  PlanarHresPixel p;
  p.b = b; p.i = i; p.j = j; p.height = height; p.width = width;
  const float *Kb = intrinsics + (size_t)b * 9;
  p.fx = Kb[0]; p.fy = Kb[4]; p.cx = Kb[2]; p.cy = Kb[5];
  p.S = s0 + sstep * (float)j; p.T = t0 + tstep * (float)i;
  p.s0 = pp_hres_source(image0, pose0, Kb, b, height, width);
  return p;
}
// The PP source (pp_hres_layers_kernel, pp_hres_layers_sparse_kernel): the background is a second image of the same camera.  Equal poses: both sample
// the same position, and the taps are copied.
struct PpHres : PlanarHresPixel {
  PpHresSource s1;
  bool same;
  __device__ __forceinline__ HresTaps taps(float depth) const {
    HresTaps t;
    const Vec3 point = plane_point(depth);
    t.fg = pp_hres_source_taps(s0, point, width, height);
    if (same) t.bg = t.fg;
    else t.bg = pp_hres_source_taps(s1, point, width, height);
    return t;
  }
  __device__ __forceinline__ HresRgb fetch(const HresTaps &t) const {
    HresRgb g;
    g.fg = gather3_load(s0.img, t.fg);
    g.bg = gather3_load(s1.img, t.bg);
    return g;
  }
};
__device__ __forceinline__ PpHres pp_hres(const float *__restrict__ image0, const float *__restrict__ image1, const float *__restrict__ pose0,
                                          const float *__restrict__ pose1, const float *__restrict__ intrinsics, int b, int i, int j, int height, int width,
                                          float s0, float sstep, float t0, float tstep) {
  PpHres p{planar_hres_pixel(image0, pose0, intrinsics, b, i, j, height, width, s0, sstep, t0, tstep)};
  p.s1 = pp_hres_source(image1, pose1, intrinsics + (size_t)b * 9, b, height, width);
  p.same = true;
#pragma unroll
  for (int k = 0; k < 16; ++k) p.same = p.same && (p.s0.P[k] == p.s1.P[k]);   // (row 3 too: M has 0 * pose[3][c], which is NaN for an infinite entry)
  return p;
}

// ---- cube-sweep (cube_sweep_kernel, cube_sweep_volume_bf16_kernel, cube_hres_layers_kernel, cube_hres_layers_sparse_kernel: geo_cube_sweep.hip): ONE definition
// of where a plane point of a cube face lies in the source PANORAMA, so that the fp32 sweep, the bf16 volume and the high-res builders agree bit for bit.
// a is apply_pose(P, backproject_planar) as pp_sweep_kernel has it; the face sweep goes on to pr = (K4 @ P) (a, 1) = K Y with
// Y = apply_pose(P, a) -- the reference's doubled pose (geo_planar.hip) -- so Y is the direction the face sweep samples wherever its (u, v) falls
// inside the face.  Here Y is looked up in the panorama along itself: R_f Y with equirect_to_cube_kernel's face table (a signed permutation; f is
// workgroup-uniform), that kernel's lat-long mapping lon = atan2(x + 0, z + 0), lat = asin(y / |dir|) through t_angles (atan2(y, hypot(x, z)) is that
// arcsine; -DMSI_FAST_TAIL=0: libm), u = (lon + pi) / 2pi W - 0.5, v = (lat + pi/2) / pi H - 0.5, and its sampler: u clamped to [-0.5, W - 0.5] and
// wrapped, v clamped to [0, H - 1], fmaxf first so that a NaN (Y = 0, a non-finite pose) is the lower bound BEFORE the float -> int conversion; the
// weights and blend4's order are that kernel's.  Every offset lies inside one sample's [H,W,3] panorama for any input (H * W * 12 < 2^31, checked on
// the host); the range-checked descriptor is a second line.
__device__ __forceinline__ TapsB cube_pano_taps(const float *__restrict__ P, int f, const Vec3 &a, int pano_h, int pano_w) {
  const Vec3 Y = apply_pose(P, a);                                              // the pose once more
  const float yx = Y.x, yy = Y.y, yz = Y.z;
  float cx, cy, cz;                                                             // R_f Y
  switch (f) {
    case 0: cx = yx; cy = yy; cz = yz; break;
    case 1: cx = yz; cy = yy; cz = -yx; break;
    case 2: cx = -yx; cy = yy; cz = -yz; break;
    case 3: cx = -yz; cy = yy; cz = yx; break;
    case 4: cx = yx; cy = -yz; cz = yy; break;
    default: cx = yx; cy = yz; cz = -yy; break;
  }
  // t_angles' (x, z) are the render frame's: cube (z, x); "+ 0.0f" turns -0 into +0 (one longitude at a pole, as equirect_to_cube_kernel)
  float lon_neg, lat;
  t_angles(cz + 0.0f, cy, cx + 0.0f, t_sqrt((cx * cx + cy * cy) + cz * cz), lon_neg, lat);
  const float PI = 3.14159265358979323846f;
  float u = ((PI - lon_neg) * ((float)pano_w * 0.15915494309189535f)) - 0.5f;   // (W / 2pi and H / pi: wave-uniform)
  float v = ((lat + 0.5f * PI) * ((float)pano_h * 0.31830988618379069f)) - 0.5f;
  u = fminf(fmaxf(u, -0.5f), (float)pano_w - 0.5f);
  v = fminf(fmaxf(v, 0.0f), (float)(pano_h - 1));
  const float fx0 = floorf(u), fy0 = floorf(v);
  const float du = u - fx0, dv = v - fy0;
  int x0 = min((int)fx0, pano_w - 1);                   // in [-1, W-1] ((float)W - 0.5f is W itself from 2^24 on)
  const int y0 = min((int)fy0, pano_h - 1);             // in [0, H-1]
  int x1 = x0 + 1;
  const int y1 = min(y0 + 1, pano_h - 1);
  x0 = x0 < 0 ? x0 + pano_w : x0;
  x1 = x1 >= pano_w ? x1 - pano_w : x1;
  TapsB t;
  t.oa = (unsigned)(y0 * pano_w + x0) * 12u; t.ob = (unsigned)(y0 * pano_w + x1) * 12u;
  t.oc = (unsigned)(y1 * pano_w + x0) * 12u; t.od = (unsigned)(y1 * pano_w + x1) * 12u;
  t.wa = (1.0f - dv) * (1.0f - du); t.wb = (1.0f - dv) * du; t.wc = dv * (1.0f - du); t.wd = dv * du;
  return t;
}

// The texel of the cube high-res stack: the PP texel above with its background taken from the source panorama.  Entry n of the [6B,...] batch is face
// n % 6 of sample n / 6 (b = n here); the foreground (ref face, ref pose) is PlanarHresPixel's, unchanged, and there is no equal-poses shortcut: the two
// sources are different images.
struct CubeHres : PlanarHresPixel {
  __amdgpu_buffer_rsrc_t pano;     // the source panorama of this cube
  const float *P1;                 // the face's source pose
  int f, pano_h, pano_w;
  __device__ __forceinline__ HresTaps taps(float depth) const {
    HresTaps t;
    const Vec3 point = plane_point(depth);
    t.fg = pp_hres_source_taps(s0, point, width, height);
    t.bg = cube_pano_taps(P1, f, apply_pose(P1, point), pano_h, pano_w);
    return t;
  }
  __device__ __forceinline__ HresRgb fetch(const HresTaps &t) const {
    HresRgb g;
    g.fg = gather3_load(s0.img, t.fg);
    g.bg = gather3_load(pano, t.bg);
    return g;
  }
};
__device__ __forceinline__ CubeHres cube_hres(const float *__restrict__ ref_faces, const float *__restrict__ panorama, const float *__restrict__ pose0,
                                              const float *__restrict__ pose1, const float *__restrict__ intrinsics, int n, int i, int j, int face,
                                              int pano_h, int pano_w, float s0, float sstep) {
  CubeHres p{planar_hres_pixel(ref_faces, pose0, intrinsics, n, i, j, face, face, s0, sstep, s0, sstep)};
  const int sample = n / 6;
  p.f = n - sample * 6; p.pano_h = pano_h; p.pano_w = pano_w;
  p.pano = image_rsrc(panorama, sample, pano_h, pano_w);
  p.P1 = pose1 + (size_t)n * 16;
  return p;
}

// ---- render (render_views_packed_kernel) and layers (unpack_layers_kernel): ONE decode rule, so a render from a packed stack is bit-identical to
// msi_render_views_f32 on the unpacked one.
constexpr float RGBA8_KC = 0x1.010102p-7f;   // fl32(1 / 127.5)
constexpr float RGBA8_KA = 0x1.010102p-8f;   // fl32(1 / 255)
// (half4_g, u32x2_g and the encoders rgba8_encode / rgba16f_encode: msi_common.h, shared with the fused tail of cnn_tail.hip)

__device__ __forceinline__ float4 rgba8_decode(unsigned q) {   // (the byte picks compile to v_cvt_f32_ubyte0..3)
  float4 t;
  t.x = ((float)(q & 0xffu) - 127.5f) * RGBA8_KC;
  t.y = ((float)((q >> 8) & 0xffu) - 127.5f) * RGBA8_KC;
  t.z = ((float)((q >> 16) & 0xffu) - 127.5f) * RGBA8_KC;
  t.w = (float)(q >> 24) * RGBA8_KA;
  return t;
}

__device__ __forceinline__ float4 rgba16f_decode(u32x2_g q) {
  const half4_g h = __builtin_bit_cast(half4_g, q);
  float4 t;
  t.x = (float)h.x; t.y = (float)h.y; t.z = (float)h.z; t.w = (float)h.w;
  return t;
}

// ---- render, ods, planar (mpi_render_views_kernel) and cube: the output modes, the layer fraction of over_composite_depth, ONE way to address and load a
// texel of a layer stack, fp32 or packed, so the many-views renders of every family read the same bits from the same stack, and the pieces those
// renders are made of (block decode, rays and pose, the sphere renders' per-layer step and segment combine, the pixel store).  The pieces take and
// return VALUES: a piece that updates a kernel's accumulators through references changes the order in which the compiler promotes them to registers,
// and with it the instruction stream (profiles/shared_render_pieces_isa.txt has what each form did).
enum RenderMode { RENDER_RGB = 1, RENDER_DEPTH = 2, RENDER_LAYERS = 4 };

// (i / len) of projector.py:242 per layer: a Python double division converted to an fp32 tensor constant.  Tabulated on the
// host (kernel argument, read with a scalar load: the layer index is wave-uniform) -- as an expression in the kernel it was an
// emulated fp64 division, ~25 half-rate instructions per (thread, layer), a fifth of the render kernel's VALU time.
constexpr int DEPTH_FRAC_MAX = 128;
struct DepthFrac { float f[DEPTH_FRAC_MAX]; };

// ONE texel policy for every render that reads a [B,D,H,W,4] stack -- fp32 (a 16-byte load) or packed (rgba16f: 8 bytes, rgba8: 4, decoded by the
// rule above): shift = log2 of the bytes per texel, layer = the buffer resource of layer d of sample b (32-bit texel offsets also for stacks beyond
// 2 GiB; layer_bytes = hw << shift, H * W < 2^24 checked on the host), tap = the four fp32 values of one texel of that resource.  A tap of a packed
// stack is ONE load decoded to what msi_unpack_layers writes for that texel (rgba8: 11 VALU per tap -- four v_cvt_f32_ubyte, three subtracts, four
// multiplies; rgba16f: four v_cvt_f32_f16), so a render from a packed stack is bit-identical to the render of the unpacked one.
template <int FMT> struct StackTexel {
  static_assert(FMT == MSI_LAYERS_F32 || FMT == MSI_LAYERS_RGBA8 || FMT == MSI_LAYERS_RGBA16F, "a texel format of msi_hip.h");
  static constexpr int shift = FMT == MSI_LAYERS_F32 ? 4 : FMT == MSI_LAYERS_RGBA16F ? 3 : 2;
  static __device__ __forceinline__ __amdgpu_buffer_rsrc_t layer(const void *layers, int b, int nd, int d, size_t hw, int layer_bytes) {
    if constexpr (FMT == MSI_LAYERS_F32)
      return __builtin_amdgcn_make_buffer_rsrc((void *)(static_cast<const float4 *>(layers) + ((size_t)b * nd + d) * hw), 0, layer_bytes, 0x00020000);
    else
      return __builtin_amdgcn_make_buffer_rsrc((void *)(static_cast<const char *>(layers) + ((((size_t)b * nd + d) * hw) << shift)), 0, layer_bytes, 0x00020000);
  }
  static __device__ __forceinline__ float4 tap(__amdgpu_buffer_rsrc_t L, unsigned texel) {
    if constexpr (FMT == MSI_LAYERS_F32) {
      typedef unsigned u32x4_g __attribute__((ext_vector_type(4)));
      return __builtin_bit_cast(float4, (u32x4_g)__builtin_amdgcn_raw_buffer_load_b128(L, texel << 4, 0, 0));
    } else if constexpr (FMT == MSI_LAYERS_RGBA8) {
      return rgba8_decode(__builtin_amdgcn_raw_buffer_load_b32(L, texel << 2, 0, 0));
    } else {
      return rgba16f_decode((u32x2_g)__builtin_amdgcn_raw_buffer_load_b64(L, texel << 3, 0, 0));
    }
  }
};

// ---- the many-views renders (render, ods, cube, planar): which pixel a thread renders.  A workgroup is 64 consecutive pixels of ROWS target rows of
// one (sample, view); the 1-D grid runs sample -> view -> row group -> 64-pixel block.
// XCD-aware: workgroup ids go round-robin over the 8 XCDs and each XCD has its own L2, so XCD x takes the x-th eighth of that sequence, in order:
// vertically adjacent target rows -- which share their bilinear tap rows -- are gathered through the SAME L2 (with rows dealt round-robin every tap
// row was fetched by two XCDs: 2.3x the stack's bytes at D = 64, batch 16; 1.43x at the BASELINE size), and the V views of one stack follow each other
// (its texels stay in the Infinity Cache while they render).  The host rounds the grid up to a multiple of 8 (view_grid below): whole workgroups
// past the end (past_end()) leave before decode().  ROWS = 1: the row is the group and threadIdx.y is free (the sphere renders' layer segments); ROWS = 4: a
// wave is one row.  j may lie past the row end.
template <int ROWS> struct ViewBlock {
  unsigned gx, gy, nblk, lin;
  unsigned bv;   // sample * views + view
  int b, i, j;
  __device__ __forceinline__ ViewBlock(int out_h, int out_w, int views, int batch) {
    gx = (unsigned)(out_w + 63) >> 6, gy = ROWS == 1 ? (unsigned)out_h : (unsigned)(out_h + ROWS - 1) / ROWS;
    nblk = gx * gy * (unsigned)views * (unsigned)batch;
    const unsigned per = gridDim.x >> 3;
    lin = (blockIdx.x & 7u) * per + (blockIdx.x >> 3);
  }
  __device__ __forceinline__ bool past_end() const { return lin >= nblk; }
  __device__ __forceinline__ void decode(int views) {   // (after past_end)
    const unsigned rowb = lin / gx;
    j = (int)(lin - rowb * gx) * 64 + threadIdx.x;
    bv = rowb / gy;
    i = ROWS == 1 ? (int)(rowb - bv * gy) : (int)(rowb - bv * gy) * ROWS + threadIdx.y;
    b = (int)(bv / (unsigned)views);
  }
};

// A ray of a target view: direction r, origin c.  view_ray gives both BEFORE the pose for the cameras of the many-views renders (pose, origin,
// K and e of a view are wave-uniform: scalar loads; a camera reads its own table only, the others may be nullptr):
//   MSI_CAMERA_EQUIRECT  (cos S cos T, sin T, sin S cos T) on the lat-long grid of the OUTPUT size (trig = its table)
//   MSI_CAMERA_PINHOLE   (1, (i + 0.5 - cy) / fy, (j + 0.5 - cx) / fx): forward +x, image-down +y, image-right +z -- the
//                        orientation of the equirect render around its centre pixel (IEEE divides: per pixel, not per layer)
// with the origin (tgt_pos[2], tgt_pos[1], tgt_pos[0]) for both, and
//   CAMERA_ODS           the equirect camera with the origin moved onto the viewing circle of the view:
//                          direction  r = (cos S cos T, sin T, sin S cos T)
//                          origin     c = (tgt_pos[2] + sin S * e, tgt_pos[1], tgt_pos[0] + (-cos S) * e)   -- e = eye_radius[b*V + v], signed:
//                                                                                             e > 0 the left eye (the reference's order = +1)
//                        (sin S, 0, -cos S) . r = 0: the ray is tangent to the circle of radius |e| around the head position.  With e = 0 the
//                        origin is tgt_pos + (+-0) and the render has the bits of the equirect camera.  Column j is column W-1-j of
//                        render_kernel<RAY_ODS>'s image (msi_render_ods_f32 keeps the reference's mirrored order), i.e. this one is upright
//                        like every other render here.  The origin -- and with it cc, qb and qc -- is per LANE: see the status word below.
// apply_pose is r <- pose[:3,:3] r, c <- pose (c, 1) of every render (spherical.py:303-310 / transform_ray :70-94), terms summed left to right.
constexpr int CAMERA_ODS = 2;   // (the kernels' third camera, chosen by a non-NULL eye_radius: not a camera code of the ABI)
struct ViewRay { float rx, ry, rz, cx, cy, cz; };

template <int CAMERA>
__device__ __forceinline__ ViewRay view_ray(const float *intrinsics, const float *eye_radius, const float *trig, const float *tgt_pos, unsigned bv,
                                            int i, int j, int out_h, int out_w) {
  ViewRay r;
  if (CAMERA == MSI_CAMERA_PINHOLE) {
    const float *Kv = intrinsics + (size_t)bv * 9;      // fx . cx / . fy cy
    r.rx = 1.0f;
    r.ry = (((float)i + 0.5f) - Kv[5]) / Kv[4];
    r.rz = (((float)j + 0.5f) - Kv[2]) / Kv[0];
  } else {
    const float cs = trig[j], ss = trig[out_w + j];
    const float ct = trig[2 * out_w + i], st = trig[2 * out_w + out_h + i];
    r.rx = cs * ct; r.ry = st; r.rz = ss * ct;
    if constexpr (CAMERA == CAMERA_ODS) {
      const float *tp = tgt_pos + (size_t)bv * 3;
      const float e = eye_radius[bv];
      r.cx = tp[2] + ss * e; r.cy = tp[1]; r.cz = tp[0] + (-cs) * e;
      return r;
    }
  }
  const float *tp = tgt_pos + (size_t)bv * 3;
  r.cx = tp[2]; r.cy = tp[1]; r.cz = tp[0];
  return r;
}

__device__ __forceinline__ void apply_pose(const float *P, ViewRay &r) {
  {
    const float x = (P[0] * r.rx + P[1] * r.ry) + P[2] * r.rz;
    const float y = (P[4] * r.rx + P[5] * r.ry) + P[6] * r.rz;
    const float z = (P[8] * r.rx + P[9] * r.ry) + P[10] * r.rz;
    r.rx = x; r.ry = y; r.rz = z;
  }
  {
    const float x = ((P[0] * r.cx + P[1] * r.cy) + P[2] * r.cz) + P[3] * 1.0f;
    const float y = ((P[4] * r.cx + P[5] * r.cy) + P[6] * r.cz) + P[7] * 1.0f;
    const float z = ((P[8] * r.cx + P[9] * r.cy) + P[10] * r.cz) + P[11] * 1.0f;
    r.cx = x; r.cy = y; r.cz = z;
  }
}

// The running far-to-near composite of a pixel (pj.over_composite, projector.py:259-263, and over_composite_depth, :239-242) and its step for layer d
// with the blended texel c = (r, g, b, alpha): layer 0 replaces (the farthest layer's alpha is ignored; depth 0), every other layer is
// c a + out (1 - a) for the colour and frac a + out (1 - a) for the depth, frac() = (d / D) as an fp32 constant (DepthFrac).  tr is the
// transmittance of the layers so far, for renders that combine partial composites.
struct Composite { float o0, o1, o2, od, tr; };

template <int MODE, class Frac>
__device__ __forceinline__ Composite over_step(float o0, float o1, float o2, float od, float tr, int d, const float4 &c, Frac frac) {
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
    else od = frac() * al + od * (1.0f - al);
  }
  tr = tr * (1.0f - al);
  return Composite{o0, o1, o2, od, tr};
}

// rgb [B,V,h,w,3] and one-channel depth [B,V,h,w] of the many-views renders (a wave's 64 pixels are one contiguous 768-byte rgb run and one
// 256-byte depth run)
template <int MODE>
__device__ __forceinline__ void store_pixel(float *out_rgb, float *out_depth, size_t pix, float o0, float o1, float o2, float od) {
  if (MODE & RENDER_RGB) {
    float *p = out_rgb + pix * 3;
    p[0] = o0; p[1] = o1; p[2] = o2;
  }
  if (MODE & RENDER_DEPTH) out_depth[pix] = od;
}

// ---- K4, the sphere renders (render_kernel, render_views_kernel, render_views_packed_kernel: geo_render.hip; render_ods_views_kernel: geo_ods.hip):
// fused reprojection + wrap-around bilinear gather + over-composite, built from ONE set of pieces.  One thread per target pixel and layer segment, block = 64 pixels of
// one target row x RENDER_SEGS layer segments (a wavefront = 64 consecutive columns, so each tap row is a ~1 KiB coalesced float4 segment and
// vertically adjacent rows share tap rows in L2): a pixel's D layers are split over RENDER_SEGS threads (same lane, different waves), each
// compositing its contiguous range of layers from transparent black,
//   C <- rgb a + C (1-a),   T <- T (1-a),
// and the segments are combined back to front, out = C_3 + T_3 (C_2 + T_2 (C_1 + T_1 C_0)) (the over operator is associative; rounding differs
// from the strictly sequential form by ~1e-7).  One thread per pixel left the chip with 3 200 wavefronts for 8 192 wave slots and a 32-deep chain
// of dependent-latency gathers per thread.  The ray/sphere quadratic's a and b do not depend on the layer, so per layer only sqrt, one divide
// and the two angles remain; every texel of the D x H x W x 4 stack is fetched from HBM once.
// The many-views kernels of the three units are ONE body, render_views_body below, for view_ray's three cameras and a stack in any texel format;
// render_views_sparse_kernel (geo_sparse_views.hip) runs the same pieces around its own layer loop.  render_kernel keeps its three ray models, its
// stores and its own text of the gathers and the over step (as pieces they change some of its instantiations: profiles/shared_render_pieces_isa.txt).
constexpr int RENDER_SEGS = 4;   // layer segments per pixel (threads in y)

struct SphereBlock : ViewBlock<1> {
  int seg;
  bool valid;    // j < out_w; decode clamps j into the row
  using ViewBlock<1>::ViewBlock;
  __device__ __forceinline__ void decode(int views, int out_w) {
    ViewBlock<1>::decode(views);
    // (a wavefront is one threadIdx.y: telling the compiler keeps the layer index -- and with it the per-layer buffer
    // descriptor -- in SGPRs; without it every gather sat in a readfirstlane waterfall loop, ~12 instructions each)
    seg = __builtin_amdgcn_readfirstlane(threadIdx.y);
    valid = j < out_w;
    j = valid ? j : out_w - 1;      // (lanes past the row end compute a duplicate and store nothing: no early return before the barrier)
  }
};

// The status word of a sphere render: qc_max, the max over a thread's layers of |origin|^2 - radius^2, is >= 0 when the ray origin (cc = |origin|^2)
// is not inside every sphere it was intersected with, and cc is NaN for a NaN pose / target position (fmaxf drops NaNs and leaves qc_max at -1 --
// tested separately): outside the reference's domain (spherical.py:316-318 takes the square root of a negative number there).  The clamp
// in sphere_uv kept the pixels finite; each kernel ORs MSI_RENDER_STATUS_ORIGIN_OUTSIDE into *status on `!(qc_max < 0.0f) || cc != cc`, one
// atomicOr per wave at the most.  Who speaks for the wave depends on the camera: the origin of an equirect or pinhole view is a property of the
// view, so all lanes agree and lane 0 tests its own.  The origin of an ODS view is a property of the LANE (a point of the viewing circle): a
// circle that crosses the innermost sphere is outside the domain for some columns only, so every lane tests its own, the wave votes, and lane 0
// issues the atomicOr.  (Lanes past the row end vote with the last pixel's origin, which a stored lane of this row has too.)  The choice is two
// lines under `if constexpr (CAMERA == CAMERA_ODS)` in render_views_body and in render_views_sparse_kernel: as one function it changes the
// instruction counts of both (profiles/ods_camera_pieces_isa.txt).

// the layer-independent part of the ray/sphere quadratic |c + t r|^2 = radius^2 of ray r (after the pose)
struct SphereQuad { float qb, cc, qb2, fa, ta, inv_ta; };

__device__ __forceinline__ SphereQuad sphere_quad(const ViewRay &r) {
  SphereQuad q;
  const float qa = (r.rx * r.rx + r.ry * r.ry) + r.rz * r.rz;
  q.qb = 2.0f * ((r.rx * r.cx + r.ry * r.cy) + r.rz * r.cz);
  q.cc = (r.cx * r.cx + r.cy * r.cy) + r.cz * r.cz;
  q.qb2 = q.qb * q.qb;
  q.fa = 4.0f * qa; q.ta = 2.0f * qa;
  q.inv_ta = __builtin_amdgcn_rcpf(q.ta);
  return q;
}

// The per-layer geometry of every sphere render: where ray r meets the sphere of this radius, as pixel coordinates (u, v) of the layer, and
// qc = |origin|^2 - radius^2 for the caller's qc_max (the status word above).
struct SphereUv { float u, v, qc; };

__device__ __forceinline__ SphereUv sphere_uv(float radius, const ViewRay &r, const SphereQuad &q, const PixConsts &K) {
  SphereUv p;
  p.qc = q.cc - radius * radius;
  const float disc = q.qb2 - q.fa * p.qc;
  // disc >= 0 whenever the ray origin is inside the sphere (the documented domain; the host-side guard of the MSI class
  // enforces it for host inputs).  Outside it the reference takes sqrt of a negative number and casts NaN to int
  // (undefined); the clamp keeps device-side inputs finite and changes nothing inside the domain.
  // (no branch of the reference depends on these values: the whole chain is continuous -> 1-ulp primitives)
#if MSI_FAST_TAIL
  const float num = t_sqrt(fmaxf(disc, 0.0f)) - q.qb;           // t = num / ta with the pixel's 1 / ta (one correction step: <= 1 ulp)
  const float tq = num * q.inv_ta;
  const float t = __builtin_fmaf(__builtin_fmaf(-tq, q.ta, num), q.inv_ta, tq);
#else
  const float t = t_div(-q.qb + t_sqrt(fmaxf(disc, 0.0f)), q.ta);
#endif
  const float x = r.cx + t * r.rx;
  const float y = r.cy + t * r.ry;
  const float z = r.cz + t * r.rz;
  // project_spherical (spherical.py:243-246) + theta_phi_to_pixels (:54-68); the point lies on the layer's sphere: |P| = radius
  float theta, phi;
  t_angles(x, y, z, radius, theta, phi);
#if MSI_FAST_TAIL
  p.u = ((theta + K.pi) - K.pi_over_w) * K.u_scale;
  p.v = ((phi + K.half_pi) - K.half_pi_over_h) * K.v_scale;
#else
  p.u = (((theta + K.pi) - K.pi_over_w) / K.u_den) * K.wm1;
  p.v = (((phi + K.half_pi) - K.half_pi_over_h) / K.v_den) * K.hm1;
#endif
  return p;
}

// (i / len) of projector.py:242 for layer d, tabulated up to DEPTH_FRAC_MAX layers
__device__ __forceinline__ float depth_frac(const DepthFrac &F, int d, int nd) {
  return nd <= DEPTH_FRAC_MAX ? F.f[d] : (float)((double)d / (double)nd);
}

// The layers of sample b as a sphere render sees them: layer(d, ...) is the per-layer step, from the quadratic to the four taps to the blended
// texel (r, g, b, alpha) of layer d along ray r; the layers first(seg) .. end(seg) are segment seg's.
template <int FMT> struct SphereStack {
  const void *layers;
  const float *depths;
  int b, nd, height, width;
  size_t hw;          // source layer size
  int layer_bytes;    // (H * W < 2^24, checked on the host)
  __device__ __forceinline__ SphereStack(const void *layers_, const float *depths_, int b_, int nd_, int height_, int width_)
      : layers(layers_), depths(depths_), b(b_), nd(nd_), height(height_), width(width_), hw((size_t)height_ * width_),
        layer_bytes((int)(hw << StackTexel<FMT>::shift)) {}
  static constexpr int UNROLL = 4;   // of the layer loop of sphere_views_body
  __device__ __forceinline__ int first(int seg) const { return (seg * nd) / RENDER_SEGS; }
  __device__ __forceinline__ int end(int seg) const { return ((seg + 1) * nd) / RENDER_SEGS; }

  struct Step { float4 c; float qc_max; };
  __device__ __forceinline__ Step layer(int d, const ViewRay &r, const SphereQuad &q, const PixConsts &K, float qc_max) const {
    Step s;
    const SphereUv p = sphere_uv(depths[d], r, q, K);
    s.qc_max = fmaxf(qc_max, p.qc);
    const TapsR tp4 = make_taps_ranged(p.u, p.v, width, height);
    // one descriptor per layer (scalar work)
    const __amdgpu_buffer_rsrc_t L = StackTexel<FMT>::layer(layers, b, nd, d, hw, layer_bytes);
    const float4 A = StackTexel<FMT>::tap(L, tp4.oa), Bv = StackTexel<FMT>::tap(L, tp4.ob), C = StackTexel<FMT>::tap(L, tp4.oc), Dv = StackTexel<FMT>::tap(L, tp4.od);
    s.c.w = blend4(tp4, A.w, Bv.w, C.w, Dv.w);
    s.c.x = blend4(tp4, A.x, Bv.x, C.x, Dv.x);
    s.c.y = blend4(tp4, A.y, Bv.y, C.y, Dv.y);
    s.c.z = blend4(tp4, A.z, Bv.z, C.z, Dv.z);
    return s;
  }
};

// The sibling of SphereStack for a high-res stack that was never built (render_views_factored_kernel, geo_factored.hip): the "layers" are the
// FACTORS of msi_hres_layers -- the two images, the two poses, the intrinsics, the stack-size trig table and the low-res blend_weights / alphas --
// and a tap is the texel function itself, hres_texel(ods_hres(.., y, x), depth, w, a) with w, a the resize at (y, x), evaluated at the four wrapped
// corners make_taps_xy names.  Every step is the builders' device function, in a unit compiled without contraction, so a tap has the bits
// hres_layers_kernel stores and layer() returns what SphereStack<MSI_LAYERS_F32>::layer returns from that stack (blend4 in its order w, x, y, z).
// Alpha first: its four taps are sixteen low-res loads and no image gather.  Where no lane of the wavefront can see the layer -- the blended alpha
// compares == 0 and the layer is not layer 0, whose colour the composite takes whatever its alpha -- the colour is not computed and the step
// returns colour 0: over_step is then 0 * 0 + o * 1, the dense step up to the sign of a zero (colours finite, as in the sparse viewer's contract).
// qc_max sees every layer.  The four taps share two rows and two columns: the trig lookups and hres_axis of a row / column are common
// subexpressions of the four ods_hres / hres_corners calls, the pose comparison (OdsHres::same) is the same for every tap of a sample.
#ifndef MSI_FACTORED_SKIP   // (measurement: -DMSI_FACTORED_SKIP=0 computes every layer's colour, tools/hres_factored_bench.py)
#define MSI_FACTORED_SKIP 1
#endif
struct FactoredSphereStack {
  const float *image0, *image1, *pose0, *pose1, *intrinsics, *depths, *trig;   // msi_hres_layers' inputs; trig: the table of the STACK size
  const float *bw, *al;                                                        // sample b's low-res tensors [h,w,D]
  int b, nd, height, width, low_h, low_w;
  float sy, sx;                                                                // hres_scale of the two axes
  static constexpr int UNROLL = 1;   // (a layer step is ~3 500 instructions, and the wave's vote below cannot be unrolled with a remainder loop)
  __device__ __forceinline__ int first(int seg) const { return (seg * nd) / RENDER_SEGS; }
  __device__ __forceinline__ int end(int seg) const { return ((seg + 1) * nd) / RENDER_SEGS; }

  // the resize of layer d of a low-res tensor at corners k: lerp2<float>, elementwise what hres_lerp computes for a group of layers
  __device__ __forceinline__ float low(const float *p, int d, const HresCorners &k) const {
    return lerp2(p[k.tl + d], p[k.tr + d], p[k.bl + d], p[k.br + d], k.xl, k.yl);
  }
  __device__ __forceinline__ float4 texel(int d, unsigned y, unsigned x, const HresCorners &k, float alpha, const PixConsts &K) const {
    return hres_texel(ods_hres(image0, image1, pose0, pose1, intrinsics, trig, K, b, (int)y, (int)x, height, width), depths[d], low(bw, d, k), alpha);
  }

  struct Step { float4 c; float qc_max; };
  __device__ __forceinline__ Step layer(int d, const ViewRay &r, const SphereQuad &q, const PixConsts &K, float qc_max) const {
    Step s;
    const SphereUv p = sphere_uv(depths[d], r, q, K);
    s.qc_max = fmaxf(qc_max, p.qc);
    const TapsXY t = make_taps_xy(p.u, p.v, width, height);
    const HresCorners ka = hres_corners((int)t.y0, (int)t.x0, sy, sx, low_h, low_w, nd), kb = hres_corners((int)t.y0, (int)t.x1, sy, sx, low_h, low_w, nd);
    const HresCorners kc = hres_corners((int)t.y1, (int)t.x0, sy, sx, low_h, low_w, nd), kd = hres_corners((int)t.y1, (int)t.x1, sy, sx, low_h, low_w, nd);
    const float aa = low(al, d, ka), ab = low(al, d, kb), ac = low(al, d, kc), ad = low(al, d, kd);
    s.c.w = blend4(t, aa, ab, ac, ad);
    s.c.x = 0.0f; s.c.y = 0.0f; s.c.z = 0.0f;
    if (MSI_FACTORED_SKIP && __builtin_amdgcn_ballot_w64(d == 0 || s.c.w != 0.0f) == 0) return s;   // (wave-uniform)
    const float4 A = texel(d, t.y0, t.x0, ka, aa, K), Bv = texel(d, t.y0, t.x1, kb, ab, K);
    const float4 C = texel(d, t.y1, t.x0, kc, ac, K), Dv = texel(d, t.y1, t.x1, kd, ad, K);
    s.c.x = blend4(t, A.x, Bv.x, C.x, Dv.x);
    s.c.y = blend4(t, A.y, Bv.y, C.y, Dv.y);
    s.c.z = blend4(t, A.z, Bv.z, C.z, Dv.z);
    return s;
  }
};

// The segments of a pixel through LDS, combined back to front in the thread of segment 0, which hands the finished pixel to store(o0, o1, o2, od).
template <class Store>
__device__ __forceinline__ void sphere_combine(const SphereBlock &s, float o0, float o1, float o2, float od, float tr, Store store) {
  __shared__ float s_part[RENDER_SEGS][64][5];
  const int seg = s.seg;
  s_part[seg][threadIdx.x][0] = o0; s_part[seg][threadIdx.x][1] = o1; s_part[seg][threadIdx.x][2] = o2;
  s_part[seg][threadIdx.x][3] = od; s_part[seg][threadIdx.x][4] = tr;
  __syncthreads();
  if (seg != 0 || !s.valid) return;
#pragma unroll
  for (int sg = 1; sg < RENDER_SEGS; ++sg) {    // segment 0 holds the farthest layers
    const float *q = s_part[sg][threadIdx.x];
    o0 = q[0] + q[4] * o0; o1 = q[1] + q[4] * o1; o2 = q[2] + q[4] * o2;
    od = q[3] + q[4] * od;
  }
  store(o0, o1, o2, od);
}

// Many views of one stack per launch (msi_render_views_f32 / _packed: geo_render.hip; msi_render_ods_views: geo_ods.hip): render_kernel's
// per-layer arithmetic for V target cameras per sample, view_ray's cameras, from a stack in texel format FMT.  A workgroup is one (sample, view,
// target row, 64-pixel block).  Outputs rgb [B,V,h,w,3] and depth [B,V,h,w].  One body, three kernel names, the ones the profiles know them by.
// (sphere_views_body is the body for any stack type with SphereStack's first / end / layer: stack(b) makes sample b's.  K: the constants of the STACK size.)
template <int MODE, int CAMERA, class MakeStack>
__device__ __forceinline__ void sphere_views_body(MakeStack stack, const float *pose_rt, const float *tgt_pos, const float *intrinsics,
                                                  const float *eye_radius, const float *trig, int batch, int views, int nd, int out_h, int out_w,
                                                  float *out_rgb, float *out_depth, const PixConsts &K, const DepthFrac &F, int *status) {
  SphereBlock s(out_h, out_w, views, batch);
  if (s.past_end()) return;
  s.decode(views, out_w);
  const unsigned bv = s.bv;
  ViewRay r = view_ray<CAMERA>(intrinsics, eye_radius, trig, tgt_pos, bv, s.i, s.j, out_h, out_w);
  apply_pose(pose_rt + (size_t)bv * 16, r);
  const SphereQuad q = sphere_quad(r);
  const auto S = stack(s.b);
  const size_t pix = (size_t)bv * out_h * out_w + (size_t)s.i * out_w + s.j;
  float o0 = 0.f, o1 = 0.f, o2 = 0.f, od = 0.f, tr = 1.f;
  float qc_max = -1.0f;
#pragma unroll decltype(S)::UNROLL
  for (int d = S.first(s.seg); d < S.end(s.seg); ++d) {
    const auto t = S.layer(d, r, q, K, qc_max);
    qc_max = t.qc_max;
    const Composite n = over_step<MODE>(o0, o1, o2, od, tr, d, t.c, [&] { return depth_frac(F, d, nd); });
    o0 = n.o0; o1 = n.o1; o2 = n.o2; od = n.od; tr = n.tr;
  }
  if (status != nullptr) {
    if constexpr (CAMERA == CAMERA_ODS) {         // (the wave votes)
      const bool any = __builtin_amdgcn_ballot_w64(!(qc_max < 0.0f) || q.cc != q.cc) != 0;   // (wave-uniform)
      if (any && threadIdx.x == 0) atomicOr(status, MSI_RENDER_STATUS_ORIGIN_OUTSIDE);
    } else {                                      // (lane 0 speaks for the wave)
      if (threadIdx.x == 0 && (!(qc_max < 0.0f) || q.cc != q.cc)) atomicOr(status, MSI_RENDER_STATUS_ORIGIN_OUTSIDE);
    }
  }
  sphere_combine(s, o0, o1, o2, od, tr,
                 [&](float o0, float o1, float o2, float od) { store_pixel<MODE>(out_rgb, out_depth, pix, o0, o1, o2, od); });
}

template <int MODE, int CAMERA, int FMT>
__device__ __forceinline__ void render_views_body(const void *layers, const float *pose_rt, const float *tgt_pos, const float *intrinsics,
                                                  const float *eye_radius, const float *depths, const float *trig, int batch, int views,
                                                  int height, int width, int nd, int out_h, int out_w, float *out_rgb, float *out_depth,
                                                  const PixConsts &K, const DepthFrac &F, int *status) {
  sphere_views_body<MODE, CAMERA>([&](int b) { return SphereStack<FMT>(layers, depths, b, nd, height, width); }, pose_rt, tgt_pos, intrinsics,
                                  eye_radius, trig, batch, views, nd, out_h, out_w, out_rgb, out_depth, K, F, status);
}

// ---- host helpers -------------------------------------------------------------------------------------------------------------
// every family with a 1-D grid-stride kernel (prep, layers)
int grid_1d(size_t n) {
  size_t blocks = (n + 255) / 256;
  if (blocks > 256 * 16) blocks = 256 * 16;  // grid-stride the rest
  if (blocks == 0) blocks = 1;
  return (int)blocks;
}

// sweep, layers, planar: non-temporal stores (sweep_store16 and its siblings) for a destination that cannot stay in the 256-MiB Infinity Cache anyway
bool beyond_infinity_cache(size_t bytes) { return bytes > ((size_t)256 << 20); }

// layers (msi_hres_layers) and sparse (msi_hres_index_tiles, msi_hres_layers_sparse): the checks every entry point of the high-res stack makes of
// its inputs and sizes, in ONE order, and the scales of msi_resize_bilinear_f32
int hres_check(const char *who, bool inputs, int32_t batch, int32_t low_height, int32_t low_width, int32_t height, int32_t width, int32_t num_planes) {
  MSI_REQUIRE(inputs, "%s: null pointer", who);
  MSI_REQUIRE(batch >= 0 && low_height > 0 && low_width > 0 && height > 0 && width > 0 && num_planes > 0, "%s: bad dims", who);
  if (num_planes % 4 != 0)
    return msi::fail(MSI_E_UNSUPPORTED, "%s: num_planes=%d must be a multiple of 4", who, num_planes);
  MSI_REQUIRE(height <= 65535 && batch <= 65535 && (long)height * width < (1L << 24),
              "%s: problem too large (24-bit pixel offsets: H * W < 2^24, H <= 65535)", who);
  MSI_REQUIRE((long)low_height * low_width * num_planes < (1L << 31), "%s: low-res tensors too large (h * w * D < 2^31)", who);
  return MSI_OK;
}
float hres_scale(int low, int high) { return high > 1 ? (float)(low - 1) / (float)(high - 1) : 0.0f; }
// planar-hres (msi_pp_hres_layers, msi_pp_hres_layers_sparse) and sparse-hres (msi_hres_index_tiles_edge): after hres_check, what the perspective sweep
// asks of an image (msi_perspective_plane_sweep_f32: uv_grid divides by n - 1; 32-bit byte offsets into one [H,W,3] image)
int pp_hres_check(const char *who, int32_t height, int32_t width) {
  MSI_REQUIRE(height > 1 && width > 1, "%s: bad dims (a perspective sweep needs H > 1 and W > 1)", who);
  MSI_REQUIRE((long)height * width * 12 < 2147483647L, "%s: problem too large (H * W * 12 < 2^31)", who);
  return MSI_OK;
}

// render, ods, planar, cube: the grid of a many-views launch (ViewBlock), blocks_per_view x views x batch workgroups rounded up to a multiple of 8; each
// factor is < 2^31 and every product is checked before the next
int view_grid(const char *who, long blocks_per_view, int views, int batch, unsigned *grid) {
  const long lim = (1L << 31) - 8;
  long nblk = blocks_per_view;
  MSI_REQUIRE(nblk < lim, "%s: too many target pixels for one launch", who);
  nblk *= views;
  MSI_REQUIRE(nblk < lim, "%s: too many target pixels for one launch", who);
  nblk *= batch;
  MSI_REQUIRE(nblk < lim, "%s: too many target pixels for one launch", who);
  *grid = (unsigned)((nblk + 7) / 8 * 8);
  return MSI_OK;
}

// render, ods, sparse, planar, cube: the argument checks of the five *_render_views entry points, in ONE order (msi_hip.h states each entry point's
// instance of it).  The entry point fills in what it has; its own checks are the two callables, made at their place in the order, each returning
// MSI_OK or the result of msi::fail.  Returns the grid; the caller returns MSI_OK without a launch when batch == 0.
constexpr unsigned ANY_FORMAT = 1u << MSI_LAYERS_F32 | 1u << MSI_LAYERS_RGBA8 | 1u << MSI_LAYERS_RGBA16F;
struct ViewArgs {
  const char *who;                              // names the entry point in the error text
  const void *out_rgb, *out_depth;
  bool inputs;                                  // every input the entry point requires is non-NULL
  int format;
  unsigned formats;                             // bit f: format f is allowed
  const char *format_note;                      // appended to "unknown format %d"
  const int32_t *camera;                        // nullptr: an entry point without a camera code (ods, mpi)
  const void *trig, *intrinsics, *eye_radius;   // the tables of the equirect and pinhole cameras; sparse: the ODS camera's, which goes with equirect
  bool dims;                                    // batch >= 0 and every stack dimension > 0
  long texels;                                  // H * W of a layer, 0 where no 24-bit texel offset is used (cube)
  int views, batch, out_h, out_w;
  int rows;                                     // target rows per workgroup (ViewBlock<ROWS>)
};

inline int no_check() { return MSI_OK; }

template <class Unsupported, class Limits>
int check_views(const ViewArgs &a, Unsupported unsupported, Limits limits, unsigned *grid) {
  const char *who = a.who;
  MSI_REQUIRE(a.out_rgb || a.out_depth, "%s: both outputs are NULL", who);
  MSI_REQUIRE(a.inputs, "%s: null pointer", who);
  MSI_REQUIRE(a.format >= 0 && a.format < 32 && ((a.formats >> a.format) & 1u), "%s: unknown format %d%s", who, a.format, a.format_note);
  const int camera = a.camera ? *a.camera : MSI_CAMERA_EQUIRECT;
  MSI_REQUIRE(camera == MSI_CAMERA_EQUIRECT || camera == MSI_CAMERA_PINHOLE, "%s: unknown camera %d", who, camera);
  if (a.camera) {
    MSI_REQUIRE(camera != MSI_CAMERA_EQUIRECT || a.trig, "%s: null pointer (equirect camera needs trig)", who);
    MSI_REQUIRE(camera != MSI_CAMERA_PINHOLE || a.intrinsics, "%s: null pointer (pinhole camera needs intrinsics)", who);
    MSI_REQUIRE(camera == MSI_CAMERA_EQUIRECT || !a.eye_radius, "%s: eye_radius (the ODS camera) goes with MSI_CAMERA_EQUIRECT", who);
  }
  MSI_REQUIRE(a.dims, "%s: bad dims", who);
  if (const int e = unsupported()) return e;    // shapes the kernels do not support (MSI_E_UNSUPPORTED)
  MSI_REQUIRE(a.views >= 1, "%s: views must be >= 1 (got %d)", who, a.views);
  const int min_out = camera == MSI_CAMERA_PINHOLE ? 2 : 1;
  MSI_REQUIRE(a.out_h >= min_out && a.out_w >= min_out, "%s: bad output size %d x %d", who, a.out_h, a.out_w);
  MSI_REQUIRE(a.texels < (1L << 24), "%s: layers of more than 2^24 texels (24-bit texel offsets)", who);
  if (const int e = limits()) return e;         // the entry point's own addressing limits
  return view_grid(who, (long)((a.out_w + 63) / 64) * ((a.out_h + a.rows - 1) / a.rows), a.views, a.batch, grid);
}

DepthFrac depth_fractions(int num_planes) {
  DepthFrac F;
  for (int d = 0; d < DEPTH_FRAC_MAX; ++d) F.f[d] = d < num_planes ? (float)((double)d / (double)num_planes) : 0.0f;
  return F;
}

inline int render_mode(const void *out_rgb, const void *out_depth) { return (out_rgb ? RENDER_RGB : 0) | (out_depth ? RENDER_DEPTH : 0); }

// the launch tables: f is called with the run-time value as a compile-time constant, f(Const<V>{}); in f, `decltype(c)::value` is a template argument.
// (mode: rgb, depth or both; format: one of MSI_LAYERS_*, validated by the caller; camera: MSI_CAMERA_EQUIRECT or MSI_CAMERA_PINHOLE, validated)
template <int V> using Const = std::integral_constant<int, V>;
template <class F> void for_mode(int mode, F f) {
  switch (mode) {
    case RENDER_RGB: f(Const<RENDER_RGB>{}); break;
    case RENDER_DEPTH: f(Const<RENDER_DEPTH>{}); break;
    default: f(Const<RENDER_RGB | RENDER_DEPTH>{}); break;
  }
}
template <class F> void for_format(int format, F f) {
  switch (format) {
    case MSI_LAYERS_RGBA8: f(Const<MSI_LAYERS_RGBA8>{}); break;
    case MSI_LAYERS_RGBA16F: f(Const<MSI_LAYERS_RGBA16F>{}); break;
    default: f(Const<MSI_LAYERS_F32>{}); break;
  }
}
template <class F> void for_camera(int camera, F f) {
  if (camera == MSI_CAMERA_PINHOLE) f(Const<MSI_CAMERA_PINHOLE>{});
  else f(Const<MSI_CAMERA_EQUIRECT>{});
}
// the table of a viewer with view_ray's three cameras: f(M, CAM, FMT) once; ods: CAMERA_ODS, whatever the (equirect) camera code
template <class F> void for_view_kernel(int mode, int format, bool ods, int camera, F f) {
  for_mode(mode, [&](auto M) { for_format(format, [&](auto FMT) {
    if (ods) f(M, Const<CAMERA_ODS>{}, FMT);
    else for_camera(camera, [&](auto CAM) { f(M, CAM, FMT); });
  }); });
}

// layers, planar-hres, cube-sweep (msi_hres_layers, msi_pp_hres_layers, msi_cube_hres_layers): ONE store policy and ONE table of instantiations for the
// dense builders.  NT bit 0 / bit 1: non-temporal stores of the fp32 / the packed stack when that destination (texels x 16 / 8 / 4 bytes) cannot stay
// in the Infinity Cache.  launch(Const<FMT>, Const<WITH_F32>, Const<NT>) is called for exactly one of: fp32 alone NT 0, 1; packed + fp32 NT 0..3;
// packed alone NT 0, 2.  format: validated by the caller where layers_out is set.
template <class Launch>
void hres_dense_launch(int format, const void *rgba_native, const void *layers_out, size_t texels, Launch launch) {
  const int fmt = layers_out ? format : MSI_LAYERS_F32;
  const int nt = (rgba_native && beyond_infinity_cache(texels * 16) ? 1 : 0) |
                 (layers_out && beyond_infinity_cache(texels << (fmt == MSI_LAYERS_RGBA8 ? 2 : 3)) ? 2 : 0);
  for_format(fmt, [&](auto FMT) {
    if constexpr (decltype(FMT)::value == MSI_LAYERS_F32) {
      if (nt) launch(FMT, Const<1>{}, Const<1>{}); else launch(FMT, Const<1>{}, Const<0>{});
    } else if (rgba_native) {
      switch (nt) {
        case 0: launch(FMT, Const<1>{}, Const<0>{}); break;
        case 1: launch(FMT, Const<1>{}, Const<1>{}); break;
        case 2: launch(FMT, Const<1>{}, Const<2>{}); break;
        default: launch(FMT, Const<1>{}, Const<3>{}); break;
      }
    } else {
      if (nt) launch(FMT, Const<0>{}, Const<2>{}); else launch(FMT, Const<0>{}, Const<0>{});
    }
  });
}

// render (RAY_PERSPECTIVE) and planar: spherical.uv_grid (spherical.py:46-48) = tf.linspace(-1 + 1/n, 1 - 1/n, n) with its fp32 semantics; v[i] = start + step * i
struct UvGrid { float start, step; };
UvGrid uv_grid(int n) {
  const float s0 = (float)(-1.0 + 1.0 / n), s1 = (float)(1.0 - 1.0 / n);
  return UvGrid{s0, (s1 - s0) / (float)(n - 1)};
}

// sweep and planar: x / n = __umulhi(x, magic) (+ one correction in the kernel), see cnn.hip udiv_magic
unsigned udiv_magic32(int n) { return n == 1 ? 0xffffffffu : (unsigned)((1ull << 32) / (unsigned)n); }

}  // namespace
