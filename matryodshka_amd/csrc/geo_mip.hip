// Mip-mapped layer stacks (msi_hip.h has the two rules in full): msi_build_mips -- build_mips_kernel, the levels 1 .. L-1 of a [B,D,H,W,4] stack
// in any texel format, the base read once, every level written in one launch -- and msi_render_views_mip -- render_views_mip_kernel, K4 (the sphere
// render of geometry_device.h: the body of render_views_kernel, geo_render.hip, and of render_ods_views_kernel, geo_ods.hip) with a trilinear texel:
// the same pieces around another layer loop, as in geo_sparse_views.hip -- and msi_render_views_aniso -- render_views_aniso_kernel, that kernel with
// several trilinear samples along the major axis of each pixel's footprint.  Kernels first, the C ABI entry points below.
#include "geometry_device.h"

namespace {

// byte offset of level l (1 .. L-1) inside the mips buffer: the levels are consecutive, level l is [B,D,H>>l,W>>l] texels.  A kernel argument,
// indexed with the wave-uniform level: scalar loads.
struct MipOffsets { unsigned long long off[MSI_MIP_MAX_LEVELS]; };

MipOffsets mip_offsets(int batch, int nd, int height, int width, int levels, int shift) {
  MipOffsets o;
  unsigned long long at = 0;
  for (int l = 0; l < MSI_MIP_MAX_LEVELS; ++l) {
    o.off[l] = l >= 1 && l < levels ? at : 0;
    if (l >= 1 && l < levels) at += ((unsigned long long)batch * nd * (height >> l) * (width >> l)) << shift;
  }
  return o;
}

// the size rule of both entry points: 1 <= L <= MSI_MIP_MAX_LEVELS, H and W multiples of 2^(L-1), the top level at least 2 x 2
int mip_levels_check(const char *who, int height, int width, int levels) {
  MSI_REQUIRE(levels >= 1 && levels <= MSI_MIP_MAX_LEVELS, "%s: levels must be in 1..%d (got %d)", who, MSI_MIP_MAX_LEVELS, levels);
  const int t = 1 << (levels - 1);
  MSI_REQUIRE(height % t == 0 && width % t == 0, "%s: %d levels need H and W to be multiples of %d (got %d x %d)", who, levels, t, height, width);
  MSI_REQUIRE(levels == 1 || ((height >> (levels - 1)) >= 2 && (width >> (levels - 1)) >= 2), "%s: the top level of %d levels of %d x %d is below 2 x 2",
              who, levels, height, width);
  return MSI_OK;
}

// ---- msi_build_mips ---------------------------------------------------------------------------------------------------------------
// The partial sums of a coarse texel over the decoded base texels it covers: A = sum a, P_k = sum fl(a c_k), Q_k = sum c_k.  Never quantised.
constexpr int MIP_FIELDS = 7;
struct MipPart { float v[MIP_FIELDS]; };   // A, P_0..2, Q_0..2

__device__ __forceinline__ MipPart mip_part(const float4 &t) {
  return MipPart{{t.w, t.w * t.x, t.w * t.y, t.w * t.z, t.x, t.y, t.z}};
}
// (tl + tr) + (bl + br), field by field: THE order of the rule
__device__ __forceinline__ MipPart mip_sum4(const MipPart &tl, const MipPart &tr, const MipPart &bl, const MipPart &br) {
  MipPart s;
#pragma unroll
  for (int k = 0; k < MIP_FIELDS; ++k) s.v[k] = (tl.v[k] + tr.v[k]) + (bl.v[k] + br.v[k]);
  return s;
}
// the texel of a level whose texels cover n = 1 / inv_n base texels: alpha the mean; colour P / A (IEEE divide) where the layer weighs its colours
// (not layer 0) and A > 0, else the plain mean
__device__ __forceinline__ float4 mip_texel(const MipPart &p, float inv_n, bool weighted_layer) {
  const bool wgt = weighted_layer && p.v[0] > 0.0f;
  float4 t;
  t.w = p.v[0] * inv_n;
  t.x = wgt ? p.v[1] / p.v[0] : p.v[4] * inv_n;
  t.y = wgt ? p.v[2] / p.v[0] : p.v[5] * inv_n;
  t.z = wgt ? p.v[3] / p.v[0] : p.v[6] * inv_n;
  return t;
}

// two horizontally adjacent texels of a row, decoded: one 32- / 16- / 8-byte load (x0 is even and W is even: aligned)
template <int FMT> __device__ __forceinline__ void mip_load2(const void *base, size_t texel, float4 &a, float4 &b) {
  if constexpr (FMT == MSI_LAYERS_F32) {
    const float4 *p = static_cast<const float4 *>(base) + texel;
    a = p[0]; b = p[1];
  } else if constexpr (FMT == MSI_LAYERS_RGBA8) {
    const uint2 q = *reinterpret_cast<const uint2 *>(static_cast<const unsigned *>(base) + texel);
    a = rgba8_decode(q.x); b = rgba8_decode(q.y);
  } else {
    const uint4 q = *reinterpret_cast<const uint4 *>(static_cast<const u32x2_g *>(base) + texel);
    u32x2_g lo, hi;
    lo.x = q.x; lo.y = q.y; hi.x = q.z; hi.y = q.w;
    a = rgba16f_decode(lo); b = rgba16f_decode(hi);
  }
}
template <int FMT> __device__ __forceinline__ void mip_store(void *level, size_t texel, const float4 &t) {
  if constexpr (FMT == MSI_LAYERS_F32) static_cast<float4 *>(level)[texel] = t;
  else hres_store_packed<FMT, 0>(level, texel, t);
}

// One workgroup = the 32 x 32 base texels at (32 by, 32 bx) of one (sample, layer): thread (ty, tx) of 16 x 16 loads its 2 x 2 block -- a wave is four
// rows of sixteen threads, i.e. 2 x 4 runs of 32 consecutive base texels -- reduces it in registers to the level-1 partials, stores the level-1 texel
// (a row of sixteen threads stores 16 consecutive texels) and leaves the partials in LDS; level l = 2 .. L-1 is then (16 >> (l-1))^2 threads summing four
// partials of level l-1 from LDS, in the rule's order.  A tile of the rule, 2^(L-1) <= 32 square, lies inside one workgroup; H and W are multiples
// of it, so a workgroup at the right or bottom border holds whole tiles and texels past the border are never a child of a texel inside.
// level l's partials in s_part[k]: (16 >> (l-1))^2 entries from 256 + 64 + .. = (1024 - 4^(6-l)) / 3 on: 0, 256, 320, 336, 340 for l = 1 .. 5
__device__ __forceinline__ int mip_lds_at(int l) { return (1024 - (1024 >> (2 * (l - 1)))) / 3; }

template <int FMT>
__global__ void __launch_bounds__(256)
build_mips_kernel(const void *__restrict__ base, void *__restrict__ mips, MipOffsets O, int nd, int height, int width, int levels, unsigned gx,
                  unsigned gy) {
  __shared__ float s_part[MIP_FIELDS][344];
  const unsigned bx = blockIdx.x % gx, rest = blockIdx.x / gx;
  const unsigned by = rest % gy, layer = rest / gy;                  // layer = b * D + d
  const bool weighted_layer = layer % (unsigned)nd != 0;
  const int tid = threadIdx.x;
  char *out = static_cast<char *>(mips);
  {
    const int h1 = height >> 1, w1 = width >> 1;
    const int y = (int)by * 16 + (tid >> 4), x = (int)bx * 16 + (tid & 15);
    MipPart p = {};
    if (y < h1 && x < w1) {
      const size_t row = ((size_t)layer * height + 2 * y) * width + 2 * x;
      float4 tl, tr, bl, br;
      mip_load2<FMT>(base, row, tl, tr);
      mip_load2<FMT>(base, row + width, bl, br);
      p = mip_sum4(mip_part(tl), mip_part(tr), mip_part(bl), mip_part(br));
      mip_store<FMT>(out + O.off[1], ((size_t)layer * h1 + y) * w1 + x, mip_texel(p, 0.25f, weighted_layer));
    }
#pragma unroll
    for (int k = 0; k < MIP_FIELDS; ++k) s_part[k][tid] = p.v[k];
  }
  float inv_n = 0.25f;
  for (int l = 2; l < levels; ++l) {                                 // (levels is the same in every thread: the barriers are uniform)
    __syncthreads();
    inv_n *= 0.25f;
    const int n = 16 >> (l - 1);                                     // this level's side inside the workgroup; the level below has 2 n
    if (tid >= n * n) continue;
    const int ly = tid / n, lx = tid - ly * n;
    const int from = mip_lds_at(l - 1) + (2 * ly) * (2 * n) + 2 * lx;
    MipPart c[4];
#pragma unroll
    for (int k = 0; k < MIP_FIELDS; ++k) {
      c[0].v[k] = s_part[k][from]; c[1].v[k] = s_part[k][from + 1];
      c[2].v[k] = s_part[k][from + 2 * n]; c[3].v[k] = s_part[k][from + 2 * n + 1];
    }
    const MipPart p = mip_sum4(c[0], c[1], c[2], c[3]);
    const int hl = height >> l, wl = width >> l;
    const int y = (int)by * n + ly, x = (int)bx * n + lx;
    if (y < hl && x < wl) mip_store<FMT>(out + O.off[l], ((size_t)layer * hl + y) * wl + x, mip_texel(p, inv_n, weighted_layer));
#pragma unroll
    for (int k = 0; k < MIP_FIELDS; ++k) s_part[k][mip_lds_at(l) + tid] = p.v[k];
  }
}

// ---- msi_render_views_mip ------------------------------------------------------------------------------------------------------------
// render_views_body (geometry_device.h) with view_ray's three cameras and the trilinear texel of msi_hip.h.  Per pixel three rays -- its own, its
// column neighbour's and its row neighbour's, each the whole view_ray / apply_pose / sphere_quad of that pixel -- and per layer their three hits: the
// two differences give rho and lambda.  The levels a lane reads differ from lane to lane and a buffer resource is wave-uniform, so the levels go in
// a loop of wave-uniform steps: level l is fetched when some lane of the wavefront wants it (l0, or l1 with f > 0), by every lane that wants it (the
// others send an offset past the resource, which a buffer load answers with zeros without a memory access).  A wavefront that is magnified, or one
// with lod_bias <= -64 or one level, runs level 0 alone, with SphereStack::layer's coordinates, taps, blend and bits.
constexpr unsigned MIP_NO_TEXEL = 0x0fffffffu;   // a TEXEL index whose byte offset (<< 2 .. 4) is past any layer here (below 2^28 bytes: H * W < 2^24)

template <int MODE, int CAMERA, int FMT>
__global__ void __launch_bounds__(256)
render_views_mip_kernel(const void *__restrict__ layers, const void *__restrict__ mips, MipOffsets O, int levels, float lod_bias,
                        const float *__restrict__ pose_rt, const float *__restrict__ tgt_pos, const float *__restrict__ intrinsics,
                        const float *__restrict__ eye_radius, const float *__restrict__ depths, const float *__restrict__ trig, int batch, int views,
                        int height, int width, int nd, int out_h, int out_w, float *__restrict__ out_rgb, float *__restrict__ out_depth, PixConsts K,
                        DepthFrac F, int *__restrict__ status) {
  constexpr int SH = StackTexel<FMT>::shift;
  SphereBlock s(out_h, out_w, views, batch);
  if (s.past_end()) return;
  s.decode(views, out_w);
  const unsigned bv = s.bv;
  const float *P = pose_rt + (size_t)bv * 16;
  ViewRay r = view_ray<CAMERA>(intrinsics, eye_radius, trig, tgt_pos, bv, s.i, s.j, out_h, out_w);
  apply_pose(P, r);
  const SphereQuad q = sphere_quad(r);
  // the neighbours: j + 1 (i + 1) where that is inside the image, else j - 1 (i - 1); an axis of one pixel: the pixel itself, difference 0
  const bool lod_on = levels > 1 && lod_bias > -64.0f;                                  // (wave-uniform)
  const int jn = s.j + 1 < out_w ? s.j + 1 : max(s.j - 1, 0), in = s.i + 1 < out_h ? s.i + 1 : max(s.i - 1, 0);
  ViewRay rx = view_ray<CAMERA>(intrinsics, eye_radius, trig, tgt_pos, bv, s.i, jn, out_h, out_w);
  ViewRay ry = view_ray<CAMERA>(intrinsics, eye_radius, trig, tgt_pos, bv, in, s.j, out_h, out_w);
  apply_pose(P, rx);
  apply_pose(P, ry);
  const SphereQuad qx = sphere_quad(rx), qy = sphere_quad(ry);
  const float wf = (float)width, inv_wf = 1.0f / wf, top = (float)(levels - 1);
  const char *base_c = static_cast<const char *>(layers), *mips_c = static_cast<const char *>(mips);
  const size_t pix = (size_t)bv * out_h * out_w + (size_t)s.i * out_w + s.j;
  float o0 = 0.f, o1 = 0.f, o2 = 0.f, od = 0.f, tr = 1.f;
  float qc_max = -1.0f;
  const int d_lo = (s.seg * nd) / RENDER_SEGS, d_hi = ((s.seg + 1) * nd) / RENDER_SEGS;
  for (int d = d_lo; d < d_hi; ++d) {
    const float radius = depths[d];
    const SphereUv p = sphere_uv(radius, r, q, K);
    qc_max = fmaxf(qc_max, p.qc);
    float lam = 0.0f;
    if (lod_on) {
      const SphereUv px = sphere_uv(radius, rx, qx, K), py = sphere_uv(radius, ry, qy, K);
      float dux = px.u - p.u, duy = py.u - p.u;
      const float dvx = px.v - p.v, dvy = py.v - p.v;
      dux -= wf * rintf(dux * inv_wf);                                                  // u wraps: the nearer way round
      duy -= wf * rintf(duy * inv_wf);
      const float rho2 = fmaxf(dux * dux + dvx * dvx, duy * duy + dvy * dvy);
      // log2 rho = log2(rho^2) / 2; rho = 0: -inf -> 0; NaN: fmaxf returns its other operand -> 0
      lam = fminf(fmaxf(0.5f * __log2f(rho2) + lod_bias, 0.0f), top);
    }
    const float fl = floorf(lam), f = lam - fl;
    const int l0 = (int)fl, l1 = min(l0 + 1, levels - 1);
    float4 t0 = {0.f, 0.f, 0.f, 0.f}, t1 = {0.f, 0.f, 0.f, 0.f};
    for (int l = 0; l < levels; ++l) {
      const bool want = l == l0 || (l == l1 && f > 0.0f);
      if (__builtin_amdgcn_ballot_w64(want) == 0) continue;                             // (wave-uniform: no lane reads this level)
      const int wl = width >> l, hl = height >> l;
      float ul = p.u, vl = p.v;                                                         // (level 0: the hit itself, the plain render's bits)
      if (l != 0) {
        const float sc = __builtin_bit_cast(float, (127 - l) << 23);                    // 2^-l
        ul = (p.u + 0.5f) * sc - 0.5f;
        vl = (p.v + 0.5f) * sc - 0.5f;
      }
      const TapsXY tp = make_taps_xy(ul, vl, wl, hl);
      const unsigned r0 = __umul24(tp.y0, (unsigned)wl), r1 = __umul24(tp.y1, (unsigned)wl);
      const size_t hw = (size_t)hl * wl;
      const char *lv = l != 0 ? mips_c + O.off[l] : base_c;
      const __amdgpu_buffer_rsrc_t L =
          __builtin_amdgcn_make_buffer_rsrc((void *)(lv + ((((size_t)s.b * nd + d) * hw) << SH)), 0, (int)(hw << SH), 0x00020000);
      const float4 A = StackTexel<FMT>::tap(L, want ? r0 + tp.x0 : MIP_NO_TEXEL), Bv = StackTexel<FMT>::tap(L, want ? r0 + tp.x1 : MIP_NO_TEXEL);
      const float4 C = StackTexel<FMT>::tap(L, want ? r1 + tp.x0 : MIP_NO_TEXEL), Dv = StackTexel<FMT>::tap(L, want ? r1 + tp.x1 : MIP_NO_TEXEL);
      float4 c;
      c.w = blend4(tp, A.w, Bv.w, C.w, Dv.w);
      c.x = blend4(tp, A.x, Bv.x, C.x, Dv.x);
      c.y = blend4(tp, A.y, Bv.y, C.y, Dv.y);
      c.z = blend4(tp, A.z, Bv.z, C.z, Dv.z);
      if (l == l0) t0 = c;
      if (l == l1) t1 = c;
    }
    float4 c = t0;
    if (f > 0.0f) {
      c.w = t0.w + f * (t1.w - t0.w); c.x = t0.x + f * (t1.x - t0.x);
      c.y = t0.y + f * (t1.y - t0.y); c.z = t0.z + f * (t1.z - t0.z);
    }
    const Composite n = over_step<MODE>(o0, o1, o2, od, tr, d, c, [&] { return depth_frac(F, d, nd); });
    o0 = n.o0; o1 = n.o1; o2 = n.o2; od = n.od; tr = n.tr;
  }
  if (status != nullptr) {
    if constexpr (CAMERA == CAMERA_ODS) {         // (the origin is a property of the lane: every lane tests its own, the wave votes)
      const bool any = __builtin_amdgcn_ballot_w64(!(qc_max < 0.0f) || q.cc != q.cc) != 0;
      if (any && threadIdx.x == 0) atomicOr(status, MSI_RENDER_STATUS_ORIGIN_OUTSIDE);
    } else {                                      // (one lane per wave: the origin is a property of the view)
      if (threadIdx.x == 0 && (!(qc_max < 0.0f) || q.cc != q.cc)) atomicOr(status, MSI_RENDER_STATUS_ORIGIN_OUTSIDE);
    }
  }
  sphere_combine(s, o0, o1, o2, od, tr,
                 [&](float o0, float o1, float o2, float od) { store_pixel<MODE>(out_rgb, out_depth, pix, o0, o1, o2, od); });
}

// ---- msi_render_views_aniso ----------------------------------------------------------------------------------------------------------
// render_views_mip_kernel with the anisotropic texel of msi_hip.h: the same three rays and three hits per layer, but the four differences are
// read as the 2 x 2 footprint Jacobian, whose singular values give the level (from the MINOR axis, capped) and the number of trilinear samples
// along the MAJOR axis.  Per layer a lane has lambda, ratio and M; sample k = 0 is the centre, k = 2m - 1 / 2m the samples +m / -m.  The sample
// loop runs to the wavefront's largest 2 M (a ballot), and inside it the level loop of the mip kernel: a lane that does not want sample k
// (m > M) or level l sends MIP_NO_TEXEL, which makes no memory access.  A wavefront whose lanes all have M = 0 runs k = 0 alone, whose
// coordinates are the hit itself: exactly the loads of the mip kernel.  One sample body for every k (k is wave-uniform: the offset and the wrap
// of k > 0 sit behind a scalar branch), so an instantiation has the mip kernel's eight buffer loads.
template <int MODE, int CAMERA, int FMT>
__global__ void __launch_bounds__(256)
render_views_aniso_kernel(const void *__restrict__ layers, const void *__restrict__ mips, MipOffsets O, int levels, float lod_bias, float max_aniso,
                          const float *__restrict__ pose_rt, const float *__restrict__ tgt_pos, const float *__restrict__ intrinsics,
                          const float *__restrict__ eye_radius, const float *__restrict__ depths, const float *__restrict__ trig, int batch, int views,
                          int height, int width, int nd, int out_h, int out_w, float *__restrict__ out_rgb, float *__restrict__ out_depth, PixConsts K,
                          DepthFrac F, int *__restrict__ status) {
  constexpr int SH = StackTexel<FMT>::shift;
  SphereBlock s(out_h, out_w, views, batch);
  if (s.past_end()) return;
  s.decode(views, out_w);
  const unsigned bv = s.bv;
  const float *P = pose_rt + (size_t)bv * 16;
  ViewRay r = view_ray<CAMERA>(intrinsics, eye_radius, trig, tgt_pos, bv, s.i, s.j, out_h, out_w);
  apply_pose(P, r);
  const SphereQuad q = sphere_quad(r);
  const bool filter_on = lod_bias > -64.0f;                                              // (wave-uniform; one level is still filtered along the major axis)
  const float cap = fminf(max_aniso, (float)MSI_ANISO_MAX);                              // (the host checked it: the sample loop ends at k = 2 * 8 whatever arrives)
  const int jn = s.j + 1 < out_w ? s.j + 1 : max(s.j - 1, 0), in = s.i + 1 < out_h ? s.i + 1 : max(s.i - 1, 0);
  ViewRay rx = view_ray<CAMERA>(intrinsics, eye_radius, trig, tgt_pos, bv, s.i, jn, out_h, out_w);
  ViewRay ry = view_ray<CAMERA>(intrinsics, eye_radius, trig, tgt_pos, bv, in, s.j, out_h, out_w);
  apply_pose(P, rx);
  apply_pose(P, ry);
  const SphereQuad qx = sphere_quad(rx), qy = sphere_quad(ry);
  const float wf = (float)width, inv_wf = 1.0f / wf, hf = (float)height, inv_hf = 1.0f / hf, top = (float)(levels - 1);
  const char *base_c = static_cast<const char *>(layers), *mips_c = static_cast<const char *>(mips);
  const size_t pix = (size_t)bv * out_h * out_w + (size_t)s.i * out_w + s.j;
  float o0 = 0.f, o1 = 0.f, o2 = 0.f, od = 0.f, tr = 1.f;
  float qc_max = -1.0f;
  const int d_lo = (s.seg * nd) / RENDER_SEGS, d_hi = ((s.seg + 1) * nd) / RENDER_SEGS;
  for (int d = d_lo; d < d_hi; ++d) {
    const float radius = depths[d];
    const SphereUv p = sphere_uv(radius, r, q, K);
    qc_max = fmaxf(qc_max, p.qc);
    float lam = 0.0f, ratio = 1.0f, su = 0.0f, sv = 0.0f;                                // su, sv: step * major axis, base texels between samples
    if (filter_on) {
      const SphereUv px = sphere_uv(radius, rx, qx, K), py = sphere_uv(radius, ry, qy, K);
      float dux = px.u - p.u, duy = py.u - p.u;
      const float dvx = px.v - p.v, dvy = py.v - p.v;
      dux -= wf * rintf(dux * inv_wf);                                                  // u wraps: the nearer way round
      duy -= wf * rintf(duy * inv_wf);
      const float E = dux * dux + duy * duy, G = dvx * dvx + dvy * dvy, Fm = dux * dvx + duy * dvy;
      const float h = 0.5f * (E - G), R = t_sqrt(h * h + Fm * Fm);
      const float smax = t_sqrt(0.5f * (E + G) + R);
      const float smin = t_div(fabsf(dux * dvy - duy * dvx), smax);
      // smax = 0 or NaN: the comparison fails, ratio stays 1; fmaxf / fminf return their other operand for a NaN
      if (smax > 1.0f) ratio = fminf(fmaxf(t_div(smax, fmaxf(smin, 1.0f)), 1.0f), cap);
      const float step = t_div(smax, ratio);
      lam = fminf(fmaxf(__log2f(step) + lod_bias, 0.0f), top);                          // step = 0: -inf -> 0; NaN -> 0
      const float ax = h >= 0.0f ? h + R : Fm, ay = h >= 0.0f ? Fm : R - h;
      const float n2 = ax * ax + ay * ay, inv_n = __builtin_amdgcn_rsqf(n2);
      su = step * (n2 > 0.0f ? ax * inv_n : 1.0f);
      sv = step * (n2 > 0.0f ? ay * inv_n : 0.0f);
    }
    const float fl = floorf(lam), f = lam - fl;
    const int l0 = (int)fl, l1 = min(l0 + 1, levels - 1);
    const int M2 = 2 * (int)ceilf(0.5f * (ratio - 1.0f));                                // 2 M: the lane's last sample index
    const float half_r = 0.5f * ratio, inv_ratio = 1.0f / ratio;                        // (IEEE divide: 1 / 1 = 1)
    float4 acc = {0.f, 0.f, 0.f, 0.f};
    int k = 0;
    do {                                                                                // (k is wave-uniform)
      const int m = (k + 1) >> 1;
      const bool mine = k <= M2;
      float us = p.u, vs = p.v;                                                         // (k = 0: the hit itself, the mip kernel's coordinates)
      if (k != 0) {
        const float t = (k & 1) ? (float)m : -(float)m;
        us = p.u + t * su;
        vs = p.v + t * sv;
        us -= wf * floorf((us + 0.5f) * inv_wf);                                        // both axes wrap, by whole widths / heights: [-0.5, W - 0.5)
        vs -= hf * floorf((vs + 0.5f) * inv_hf);
      }
      float4 t0 = {0.f, 0.f, 0.f, 0.f}, t1 = {0.f, 0.f, 0.f, 0.f};
      for (int l = 0; l < levels; ++l) {
        const bool want = mine && (l == l0 || (l == l1 && f > 0.0f));
        if (__builtin_amdgcn_ballot_w64(want) == 0) continue;                           // (wave-uniform: no lane reads this level)
        const int wl = width >> l, hl = height >> l;
        float ul = us, vl = vs;
        if (l != 0) {
          const float sc = __builtin_bit_cast(float, (127 - l) << 23);                  // 2^-l
          ul = (us + 0.5f) * sc - 0.5f;
          vl = (vs + 0.5f) * sc - 0.5f;
        }
        const TapsXY tp = make_taps_xy(ul, vl, wl, hl);
        const unsigned r0 = __umul24(tp.y0, (unsigned)wl), r1 = __umul24(tp.y1, (unsigned)wl);
        const size_t hw = (size_t)hl * wl;
        const char *lv = l != 0 ? mips_c + O.off[l] : base_c;
        const __amdgpu_buffer_rsrc_t L =
            __builtin_amdgcn_make_buffer_rsrc((void *)(lv + ((((size_t)s.b * nd + d) * hw) << SH)), 0, (int)(hw << SH), 0x00020000);
        const float4 A = StackTexel<FMT>::tap(L, want ? r0 + tp.x0 : MIP_NO_TEXEL), Bv = StackTexel<FMT>::tap(L, want ? r0 + tp.x1 : MIP_NO_TEXEL);
        const float4 C = StackTexel<FMT>::tap(L, want ? r1 + tp.x0 : MIP_NO_TEXEL), Dv = StackTexel<FMT>::tap(L, want ? r1 + tp.x1 : MIP_NO_TEXEL);
        float4 c;
        c.w = blend4(tp, A.w, Bv.w, C.w, Dv.w);
        c.x = blend4(tp, A.x, Bv.x, C.x, Dv.x);
        c.y = blend4(tp, A.y, Bv.y, C.y, Dv.y);
        c.z = blend4(tp, A.z, Bv.z, C.z, Dv.z);
        if (l == l0) t0 = c;
        if (l == l1) t1 = c;
      }
      float4 c = t0;
      if (f > 0.0f) {
        c.w = t0.w + f * (t1.w - t0.w); c.x = t0.x + f * (t1.x - t0.x);
        c.y = t0.y + f * (t1.y - t0.y); c.z = t0.z + f * (t1.z - t0.z);
      }
      const float wm = fminf(fmaxf(half_r - ((float)m - 0.5f), 0.0f), 1.0f) * inv_ratio;   // (k = 0: 1 / ratio; ratio = 1: 1, the sample's own bits)
      if (k == 0) {
        acc.w = wm * c.w; acc.x = wm * c.x; acc.y = wm * c.y; acc.z = wm * c.z;
      } else if (mine) {
        acc.w = acc.w + wm * c.w; acc.x = acc.x + wm * c.x; acc.y = acc.y + wm * c.y; acc.z = acc.z + wm * c.z;
      }
      ++k;
    } while (__builtin_amdgcn_ballot_w64(k <= M2) != 0);
    const Composite n = over_step<MODE>(o0, o1, o2, od, tr, d, acc, [&] { return depth_frac(F, d, nd); });
    o0 = n.o0; o1 = n.o1; o2 = n.o2; od = n.od; tr = n.tr;
  }
  if (status != nullptr) {
    if constexpr (CAMERA == CAMERA_ODS) {         // (the origin is a property of the lane: every lane tests its own, the wave votes)
      const bool any = __builtin_amdgcn_ballot_w64(!(qc_max < 0.0f) || q.cc != q.cc) != 0;
      if (any && threadIdx.x == 0) atomicOr(status, MSI_RENDER_STATUS_ORIGIN_OUTSIDE);
    } else {                                      // (one lane per wave: the origin is a property of the view)
      if (threadIdx.x == 0 && (!(qc_max < 0.0f) || q.cc != q.cc)) atomicOr(status, MSI_RENDER_STATUS_ORIGIN_OUTSIDE);
    }
  }
  sphere_combine(s, o0, o1, o2, od, tr,
                 [&](float o0, float o1, float o2, float od) { store_pixel<MODE>(out_rgb, out_depth, pix, o0, o1, o2, od); });
}

}  // namespace

extern "C" {

int msi_build_mips(const void *layers, int32_t format, int32_t batch, int32_t num_planes, int32_t height, int32_t width, int32_t levels,
                   void *mips_out, msi_stream_t stream) {
  const char *who = "build_mips";
  MSI_REQUIRE(layers && (mips_out || levels == 1), "%s: null pointer", who);
  MSI_REQUIRE(format == MSI_LAYERS_F32 || format == MSI_LAYERS_RGBA8 || format == MSI_LAYERS_RGBA16F, "%s: unknown format %d", who, format);
  MSI_REQUIRE(batch >= 0 && num_planes > 0 && height > 0 && width > 0, "%s: bad dims", who);
  if (const int e = mip_levels_check(who, height, width, levels)) return e;
  if (batch == 0 || levels == 1) return MSI_OK;
  const unsigned gx = (unsigned)((width >> 1) + 15) / 16, gy = (unsigned)((height >> 1) + 15) / 16;
  const long blocks = (long)gx * gy * batch * num_planes;
  MSI_REQUIRE(blocks < (1L << 31), "%s: too many tiles for one launch", who);
  for_format(format, [&](auto FMT) {
    constexpr int fmt = decltype(FMT)::value;
    const MipOffsets O = mip_offsets(batch, num_planes, height, width, levels, StackTexel<fmt>::shift);
    hipLaunchKernelGGL((build_mips_kernel<fmt>), dim3((unsigned)blocks), dim3(256), 0, msi::as_stream(stream), layers, mips_out, O, num_planes, height,
                       width, levels, gx, gy);
  });
  return msi::check_launch(who);
}

int msi_render_views_mip(const void *layers, int32_t format, const void *mips, int32_t levels, float lod_bias, const float *tgt_pose_rt,
                         const float *tgt_pos, const float *intrinsics, const float *eye_radius, const float *depths, const float *trig,
                         int32_t batch, int32_t views, int32_t height, int32_t width, int32_t num_planes, int32_t camera, int32_t out_height,
                         int32_t out_width, float *out_rgb, float *out_depth, int32_t *status_device, msi_stream_t stream) {
  const char *who = "render_views_mip";
  const ViewArgs a = {who, out_rgb, out_depth, layers && (mips || levels == 1) && tgt_pose_rt && tgt_pos && depths, format, ANY_FORMAT, "", &camera, trig,
                      intrinsics, eye_radius, batch >= 0 && height > 0 && width > 0 && num_planes > 0, (long)height * width, views, batch, out_height,
                      out_width, 1};
  const auto mip_args = [&] {
    MSI_REQUIRE(lod_bias == lod_bias, "%s: lod_bias is NaN", who);
    return mip_levels_check(who, height, width, levels);
  };
  unsigned grid;
  if (const int e = check_views(a, mip_args, no_check, &grid)) return e;
  if (batch == 0) return MSI_OK;
  const dim3 block(64, RENDER_SEGS);
  const PixConsts K = make_consts(height, width);
  const DepthFrac F = depth_fractions(num_planes);
  hipStream_t s = msi::as_stream(stream);
  auto launch = [&](auto M, auto CAM, auto FMT) {
    constexpr int fmt = decltype(FMT)::value;
    const MipOffsets O = mip_offsets(batch, num_planes, height, width, levels, StackTexel<fmt>::shift);
    hipLaunchKernelGGL((render_views_mip_kernel<decltype(M)::value, decltype(CAM)::value, fmt>), dim3(grid), block, 0, s, layers, mips, O, levels,
                       lod_bias, tgt_pose_rt, tgt_pos, intrinsics, eye_radius, depths, trig, batch, views, height, width, num_planes, out_height, out_width,
                       out_rgb, out_depth, K, F, status_device);
  };
  for_view_kernel(render_mode(out_rgb, out_depth), format, eye_radius != nullptr, camera, launch);
  return msi::check_launch(who);
}

int msi_render_views_aniso(const void *layers, int32_t format, const void *mips, int32_t levels, float lod_bias, float max_anisotropy,
                           const float *tgt_pose_rt, const float *tgt_pos, const float *intrinsics, const float *eye_radius, const float *depths,
                           const float *trig, int32_t batch, int32_t views, int32_t height, int32_t width, int32_t num_planes, int32_t camera,
                           int32_t out_height, int32_t out_width, float *out_rgb, float *out_depth, int32_t *status_device, msi_stream_t stream) {
  const char *who = "render_views_aniso";
  const ViewArgs a = {who, out_rgb, out_depth, layers && (mips || levels == 1) && tgt_pose_rt && tgt_pos && depths, format, ANY_FORMAT, "", &camera, trig,
                      intrinsics, eye_radius, batch >= 0 && height > 0 && width > 0 && num_planes > 0, (long)height * width, views, batch, out_height,
                      out_width, 1};
  const auto mip_args = [&] {
    MSI_REQUIRE(lod_bias == lod_bias, "%s: lod_bias is NaN", who);
    MSI_REQUIRE(max_anisotropy >= 1.0f && max_anisotropy <= (float)MSI_ANISO_MAX, "%s: max_anisotropy must be in 1..%d (got %g)", who, MSI_ANISO_MAX,
                (double)max_anisotropy);                                                // (a NaN fails both comparisons)
    return mip_levels_check(who, height, width, levels);
  };
  unsigned grid;
  if (const int e = check_views(a, mip_args, no_check, &grid)) return e;
  if (batch == 0) return MSI_OK;
  const dim3 block(64, RENDER_SEGS);
  const PixConsts K = make_consts(height, width);
  const DepthFrac F = depth_fractions(num_planes);
  hipStream_t s = msi::as_stream(stream);
  auto launch = [&](auto M, auto CAM, auto FMT) {
    constexpr int fmt = decltype(FMT)::value;
    const MipOffsets O = mip_offsets(batch, num_planes, height, width, levels, StackTexel<fmt>::shift);
    hipLaunchKernelGGL((render_views_aniso_kernel<decltype(M)::value, decltype(CAM)::value, fmt>), dim3(grid), block, 0, s, layers, mips, O, levels,
                       lod_bias, max_anisotropy, tgt_pose_rt, tgt_pos, intrinsics, eye_radius, depths, trig, batch, views, height, width, num_planes,
                       out_height, out_width, out_rgb, out_depth, K, F, status_device);
  };
  for_view_kernel(render_mode(out_rgb, out_depth), format, eye_radius != nullptr, camera, launch);
  return msi::check_launch(who);
}

}  // extern "C"
