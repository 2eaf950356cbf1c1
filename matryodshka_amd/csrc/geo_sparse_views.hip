// The viewers of the sparse layer stacks (geo_sparse.h has the format): msi_render_views_sparse -- K4, the sphere render of geometry_device.h (the body
// of render_views_kernel, geo_render.hip, and of render_ods_views_kernel, geo_ods.hip), from a stack made with the wrap keep rule --, and
// msi_mpi_render_views_sparse / msi_cube_render_views_sparse, the planar and cube renders from a stack made with the edge rule.  Each is the dense
// kernel's pixel with one table lookup per tap tile in front of the gathers; kernels first, the C ABI entry points below.
#include "geometry_device.h"
#include "geo_sparse.h"
#include "geo_cube.h"

namespace {

// ---- what the three viewers share -----------------------------------------------------------------------------------------------
// The table entries of a 2 x 2 tap footprint: the pool tiles of its taps (y0,x0) (y0,x1) (y1,x0) (y1,x1) within their layer, -1 = dropped.  The
// base of each kernel's Look (as a member it changed every instruction stream: profiles/sparse_units_isa.txt).
struct TapTiles {
  int ia, ib, ic, id;
  __device__ __forceinline__ bool present() const { return (ia | ib | ic | id) >= 0; }
};

// The lookup: oa .. od are the entries' byte offsets in T, which each kernel computes for itself.  The shortcut: a wave is 64 neighbouring pixels
// of one target row, so most waves have no footprint across a tile's bottom border; when no lane has its two tap rows in different tile rows
// (two_tile_rows), the second row takes the first row's entries without a load.
__device__ __forceinline__ void tap_tiles(TapTiles &t, __amdgpu_buffer_rsrc_t T, unsigned oa, unsigned ob, unsigned oc, unsigned od, bool two_tile_rows) {
  t.ia = (int)__builtin_amdgcn_raw_buffer_load_b32(T, oa, 0, 0);
  t.ib = (int)__builtin_amdgcn_raw_buffer_load_b32(T, ob, 0, 0);
  if (__builtin_amdgcn_ballot_w64(two_tile_rows) != 0) {
    t.ic = (int)__builtin_amdgcn_raw_buffer_load_b32(T, oc, 0, 0);
    t.id = (int)__builtin_amdgcn_raw_buffer_load_b32(T, od, 0, 0);
  } else {
    t.ic = t.ia; t.id = t.ib;
  }
}

// ---- K4 from a sparse stack ---------------------------------------------------------------------------------------------------
// (The taps are make_taps_xy's, geometry_device.h: make_taps_ranged's weights and wrapped corners, kept as coordinates.)
// The sparse sibling of SphereStack: layer d of sample b is two buffer resources -- its row of the table ([H/4, W/16] int32) and its kept tiles in
// the pool (pool_rsrc, geo_sparse.h).  The per-layer step is split where the memory round trips are: lookup() is SphereStack::layer up to the taps
// (sphere_uv) plus the table loads of the tap tiles; gather() is its four taps and blends for the lanes whose tap tiles are all present.
template <int FMT> struct SparseStack {
  const char *pool;
  const int *table;
  const long long *layer_start;
  const float *depths;
  int b, nd, height, width, tx_n, table_bytes;
  __device__ __forceinline__ SparseStack(const void *pool_, const int *table_, const long long *layer_start_, const float *depths_, int b_, int nd_,
                                         int height_, int width_)
      : pool(static_cast<const char *>(pool_)), table(table_), layer_start(layer_start_), depths(depths_), b(b_), nd(nd_), height(height_),
        width(width_), tx_n(width_ / TILE_W), table_bytes((height_ / TILE_H) * (width_ / TILE_W) * 4) {}
  __device__ __forceinline__ int first(int seg) const { return (seg * nd) / RENDER_SEGS; }
  __device__ __forceinline__ int end(int seg) const { return ((seg + 1) * nd) / RENDER_SEGS; }

  struct Look : TapTiles {
    TapsXY tp;
    float qc_max;
  };
  __device__ __forceinline__ Look lookup(int d, const ViewRay &r, const SphereQuad &q, const PixConsts &K, float qc_max) const {
    Look s;
    const SphereUv p = sphere_uv(depths[d], r, q, K);
    s.qc_max = fmaxf(qc_max, p.qc);
    s.tp = make_taps_xy(p.u, p.v, width, height);
    const size_t l = (size_t)b * nd + d;
    const __amdgpu_buffer_rsrc_t T = table_rsrc(table + l * (size_t)(table_bytes >> 2), table_bytes);
    const unsigned r0 = __umul24(s.tp.y0 >> 2, (unsigned)tx_n), r1 = __umul24(s.tp.y1 >> 2, (unsigned)tx_n);
    const unsigned c0 = s.tp.x0 >> 4, c1 = s.tp.x1 >> 4;
    tap_tiles(s, T, (r0 + c0) << 2, (r0 + c1) << 2, (r1 + c0) << 2, (r1 + c1) << 2, r0 != r1);
    return s;
  }

  // (lanes with a dropped tap tile take tile 0 of the layer or, when the layer keeps none, the zeros of an empty resource; the caller discards them)
  __device__ __forceinline__ float4 gather(int d, const Look &s) const {
    const size_t l = (size_t)b * nd + d;
    const long long ls = layer_start[l];
    // pool_rsrc's resource with a 32-bit byte count: a layer keeps at most H * W < 2^24 texels (sparse_dims, check_views), below 2^27 bytes, so
    // the product cannot overflow.  Through pool_rsrc itself (64-bit, clamped) the kernels grew by 9 instructions and were 1-4 % slower on the
    // pinhole points: profiles/sparse_units_timing.txt.
    constexpr int SH = StackTexel<FMT>::shift;
    const int kept_bytes = (int)(layer_start[l + 1] - ls) * (TILE_TEXELS << SH);
    const __amdgpu_buffer_rsrc_t L = __builtin_amdgcn_make_buffer_rsrc((void *)(pool + (((size_t)ls * TILE_TEXELS) << SH)), 0, kept_bytes, 0x00020000);
    const bool ok = s.present();
    const unsigned i0 = (s.tp.y0 & 3u) << 4, i1 = (s.tp.y1 & 3u) << 4, j0 = s.tp.x0 & 15u, j1 = s.tp.x1 & 15u;
    const unsigned ta = ok ? (unsigned)s.ia << 6 : 0u, tb = ok ? (unsigned)s.ib << 6 : 0u;
    const unsigned tc = ok ? (unsigned)s.ic << 6 : 0u, td = ok ? (unsigned)s.id << 6 : 0u;
    const float4 A = StackTexel<FMT>::tap(L, ta + i0 + j0), Bv = StackTexel<FMT>::tap(L, tb + i0 + j1);
    const float4 C = StackTexel<FMT>::tap(L, tc + i1 + j0), Dv = StackTexel<FMT>::tap(L, td + i1 + j1);
    float4 c;
    c.w = blend4(s.tp, A.w, Bv.w, C.w, Dv.w);
    c.x = blend4(s.tp, A.x, Bv.x, C.x, Dv.x);
    c.y = blend4(s.tp, A.y, Bv.y, C.y, Dv.y);
    c.z = blend4(s.tp, A.z, Bv.z, C.z, Dv.z);
    return c;
  }
};

// render_views_body (geometry_device.h) with view_ray's three cameras, from a sparse stack: the same pieces around another layer loop.  The layers
// of a segment go in groups of GROUP: first the geometry and the table lookups of the whole group (the lookups are a second dependent memory round
// trip in front of every gather: issued together they overlap), then per layer the gathers and the over step -- for the lanes whose four tap tiles
// are present; when the wave has none the gathers are not issued.  A lane with a dropped tap tile leaves o, od, tr as they are: in the dense render
// its four alphas are zero, the blended alpha is zero and the step is c 0 + o 1 = o (a zero's sign may differ; colours must be finite there).
// qc_max and the status word see every layer.  A group that runs past the segment's end repeats its last layer's lookup and skips its step.
constexpr int SPARSE_GROUP = 2;

template <int MODE, int CAMERA, int FMT>
__global__ void __launch_bounds__(256)
render_views_sparse_kernel(const void *__restrict__ pool, const int *__restrict__ table, const long long *__restrict__ layer_start,
                           const float *__restrict__ pose_rt, const float *__restrict__ tgt_pos, const float *__restrict__ intrinsics,
                           const float *__restrict__ eye_radius, const float *__restrict__ depths, const float *__restrict__ trig,
                           int batch, int views, int height, int width, int nd, int out_h, int out_w, float *__restrict__ out_rgb,
                           float *__restrict__ out_depth, PixConsts K, DepthFrac F, int *__restrict__ status) {
  SphereBlock s(out_h, out_w, views, batch);
  if (s.past_end()) return;
  s.decode(views, out_w);
  const unsigned bv = s.bv;
  ViewRay r = view_ray<CAMERA>(intrinsics, eye_radius, trig, tgt_pos, bv, s.i, s.j, out_h, out_w);
  apply_pose(pose_rt + (size_t)bv * 16, r);
  const SphereQuad q = sphere_quad(r);
  const SparseStack<FMT> S(pool, table, layer_start, depths, s.b, nd, height, width);
  const size_t pix = (size_t)bv * out_h * out_w + (size_t)s.i * out_w + s.j;
  float o0 = 0.f, o1 = 0.f, o2 = 0.f, od = 0.f, tr = 1.f;
  float qc_max = -1.0f;
  const int d_end = S.end(s.seg);
  for (int d0 = S.first(s.seg); d0 < d_end; d0 += SPARSE_GROUP) {
    typename SparseStack<FMT>::Look look[SPARSE_GROUP];
#pragma unroll
    for (int g = 0; g < SPARSE_GROUP; ++g) {
      look[g] = S.lookup(min(d0 + g, d_end - 1), r, q, K, qc_max);
      qc_max = look[g].qc_max;
    }
#pragma unroll
    for (int g = 0; g < SPARSE_GROUP; ++g) {
      const int d = d0 + g;
      if (d >= d_end) break;
      const bool ok = look[g].present();
      if (__builtin_amdgcn_ballot_w64(ok) == 0) continue;     // (wave-uniform: nothing of this layer under these 64 pixels)
      const float4 c = S.gather(d, look[g]);
      const Composite n = over_step<MODE>(o0, o1, o2, od, tr, d, c, [&] { return depth_frac(F, d, nd); });
      if (ok) { o0 = n.o0; o1 = n.o1; o2 = n.o2; od = n.od; tr = n.tr; }
    }
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

// ---- the planar and cube renders from an edge-rule stack (msi_mpi_render_views_sparse, msi_cube_render_views_sparse) ----------------------------
// Both are the dense kernel's pixel (mpi_render_views_kernel, geo_planar.hip; cube_render_views_kernel, geo_cube.hip) around another layer loop.
// The layers go in groups of PLANAR_GROUP, and a group in three passes, each a run of independent memory operations:
//   look    the layer's geometry and the table entries of its tap tiles (a second dependent round trip in front of every gather);
//   fetch   the four texel loads, undecoded, for the layers on which some lane of the wavefront has every tap tile present -- a wave-uniform branch
//           around loads alone;
//   blend   decode, the dense kernel's weights and sum order, the dense kernel's over step, for the lanes that are present.
// (What hipcc makes of it -- profiles/sparse_planar_isa.txt: a layer's own loads issue together, a layer's results are waited for before the next
// layer's loads issue.  A form whose binary issues the group's loads back to back measured no faster: profiles/sparse_planar_timing.txt.)
// A lane with a tap in a dropped tile leaves its composite as it is: by the edge rule every alpha of its footprint is zero, the dense blend gives
// alpha 0 and the dense step is c 0 + o 1 = o (a zero's sign may differ; colours must be finite there).  Its loads carry an offset past the
// resource, which a buffer load answers with zeros without a memory access.
// The loop is each kernel's own text, twice: as one always-inline template over the kernel's look_up / fetch / blend it added 5-20 instructions to
// every instantiation and missed the timing margin in both kernels (cube pinhole +0.7-1.7 %) -- profiles/sparse_units_isa.txt, sparse_units_timing.txt.
constexpr int PLANAR_GROUP = 2;                  // (SPARSE_GROUP's: at 4 the cube kernels need 76-84 VGPRs, 5-6 waves per SIMD instead of 8)

template <int FMT> using RawTexel = std::conditional_t<FMT == MSI_LAYERS_RGBA8, unsigned, u32x2_g>;
template <int FMT> __device__ __forceinline__ RawTexel<FMT> raw_tap(__amdgpu_buffer_rsrc_t L, unsigned byte_offset) {
  if constexpr (FMT == MSI_LAYERS_RGBA8) return __builtin_amdgcn_raw_buffer_load_b32(L, byte_offset, 0, 0);
  else return (u32x2_g)__builtin_amdgcn_raw_buffer_load_b64(L, byte_offset, 0, 0);
}
template <int FMT> __device__ __forceinline__ float4 decode_tap(RawTexel<FMT> q) {     // StackTexel<FMT>::tap's decode
  if constexpr (FMT == MSI_LAYERS_RGBA8) return rgba8_decode(q);
  else return rgba16f_decode(q);
}
// mpi_tap's value (geo_planar.hip): the texel when ok, else the zeros of fetch_or_zero (the loaded zero word is alpha 0 and, rgba8, colour -1)
template <int FMT> __device__ __forceinline__ float4 decode_tap_or_zero(RawTexel<FMT> q, bool ok) {
  float4 t = decode_tap<FMT>(q);
  if constexpr (FMT == MSI_LAYERS_RGBA8) { t.x = ok ? t.x : 0.0f; t.y = ok ? t.y : 0.0f; t.z = ok ? t.z : 0.0f; }
  return t;
}
template <int FMT> struct RawTaps { RawTexel<FMT> a, b, c, d; };


// The two steps of mpi_render_views_kernel (geo_planar.hip) that do not depend on how the stack is stored, repeated op for op.  (As shared
// always-inline pieces they changed the dense kernel's instruction stream -- profiles/sparse_planar_isa.txt --, so the dense kernel keeps its own text.)
// mpi_homography is its prologue, mpi_render_kernel's: rot_t, divide_safe, m1, K_s @ m1, @ K_t_inv -> the nine entries of plane `depth`'s inverse
// homography.  mpi_coords is its per-layer coordinate step: the three dot products, divide_safe on ws, the two IEEE divides, the (-1, W) x (-1, H)
// test of tf.contrib.resampler, floor, and which of the 2 x 2 taps lie inside the layer.  A pixel that samples outside (or NaN) gets the coordinate
// (0, 0) with every tap masked.
constexpr int MPI_SPARSE_MAX_PLANES = 128;       // (MPI_MAX_PLANES of geo_planar.hip: the LDS table of homographies)

__device__ __forceinline__ void mpi_homography(const float *P, const float *Ks, const float *Ki, float depth, float *h) {
  float rt[3][3], t[3];
#pragma unroll
  for (int r = 0; r < 3; ++r) {
#pragma unroll
    for (int c = 0; c < 3; ++c) rt[r][c] = P[c * 4 + r];  // rot_t = transpose(pose[:3,:3])
    t[r] = P[r * 4 + 3];
  }
  const float a = -depth;
  const float nrt_t = (rt[2][0] * t[0] + rt[2][1] * t[1]) + rt[2][2] * t[2];
  float den = a - nrt_t;
  den += 1e-8f * (den == 0.0f ? 1.0f : 0.0f);  // divide_safe
  float m1[3][3];
#pragma unroll
  for (int r = 0; r < 3; ++r) {
    const float q = (rt[r][0] * t[0] + rt[r][1] * t[1]) + rt[r][2] * t[2];  // (rot_t @ t)[r]
#pragma unroll
    for (int c = 0; c < 3; ++c) m1[r][c] = rt[r][c] + (q * rt[2][c]) / den;
  }
  float m2[3][3];
#pragma unroll
  for (int r = 0; r < 3; ++r)
#pragma unroll
    for (int c = 0; c < 3; ++c)
      m2[r][c] = (Ks[r * 3 + 0] * m1[0][c] + Ks[r * 3 + 1] * m1[1][c]) + Ks[r * 3 + 2] * m1[2][c];
#pragma unroll
  for (int r = 0; r < 3; ++r)
#pragma unroll
    for (int c = 0; c < 3; ++c)
      h[r * 3 + c] = (m2[r][0] * Ki[0 * 3 + c] + m2[r][1] * Ki[1 * 3 + c]) + m2[r][2] * Ki[2 * 3 + c];
}

struct MpiCoords {
  bool inside;          // the pixel samples inside (-1, W) x (-1, H)
  int fx, fy;           // the footprint's origin: fx in [-1, W-1], fy in [-1, H-1]; its other corner is (fx + 1, fy + 1)
  float dx, dy;         // (fx + 1) - x, (fy + 1) - y
  bool x0, x1, y0, y1;  // column fx / fx + 1 and row fy / fy + 1 lie inside the layer (x0, x1: and the pixel is inside)
};

__device__ __forceinline__ MpiCoords mpi_coords(const float *h, float uu, float vv, float wf, float hf, int width, int height) {
  MpiCoords m;
  const float xs = (uu * h[0] + vv * h[1]) + 1.0f * h[2];
  const float ys = (uu * h[3] + vv * h[4]) + 1.0f * h[5];
  float ws = (uu * h[6] + vv * h[7]) + 1.0f * h[8];
  ws += 1e-8f * (ws == 0.0f ? 1.0f : 0.0f);
  const float xq = xs / ws, yq = ys / ws;
  // tf.contrib.resampler: zero outside (-1, W) x (-1, H); missing corners are 0
  m.inside = xq > -1.0f && yq > -1.0f && xq < wf && yq < hf;
  const float x = m.inside ? xq : 0.0f, y = m.inside ? yq : 0.0f;
  const float fxf = floorf(x), fyf = floorf(y);
  m.fx = (int)fxf; m.fy = (int)fyf;
  const int cx = m.fx + 1, cy = m.fy + 1;
  m.dx = (float)cx - x; m.dy = (float)cy - y;
  m.x0 = m.inside && m.fx >= 0; m.x1 = m.inside && cx < width; m.y0 = m.fy >= 0; m.y1 = cy < height;
  return m;
}

// The MPI render.  Grid, prologue and per-layer coordinates are mpi_render_views_kernel's (ViewBlock<4>, mpi_homography, mpi_coords).  The layer index
// is wave-uniform, so the layer's table row and its slice of the pool are scalar descriptors.  Only the tiles of the in-range taps are looked up: a
// masked tap (outside the image) sends NO_TEXEL, reads back index 0 and so never counts as absent; its value is the zero of mpi_tap.  A pixel that
// samples outside (-1, W) x (-1, H) is present with every tap masked: the dense kernel's c = 0 step.
template <int MODE, int FMT>
__global__ void __launch_bounds__(256)
mpi_render_views_sparse_kernel(const void *__restrict__ pool, const int *__restrict__ table, const long long *__restrict__ layer_start,
                               const float *__restrict__ tgt_pose, const float *__restrict__ intrinsics,
                               const float *__restrict__ tgt_intrinsics_inv, const float *__restrict__ depths, int batch, int views, int height,
                               int width, int nd, int out_h, int out_w, float *__restrict__ out_rgb, float *__restrict__ out_depth, DepthFrac F) {
  constexpr int SH = StackTexel<FMT>::shift;
  __shared__ float hom[MPI_SPARSE_MAX_PLANES][9];
  ViewBlock<4> k(out_h, out_w, views, batch);
  if (k.past_end()) return;                             // (grid rounded up to a multiple of 8; whole workgroups leave)
  k.decode(views);
  const unsigned bv = k.bv;
  const int i = k.i, j = k.j, b = k.b;
  const int tid = threadIdx.y * 64 + threadIdx.x;
  if (tid < nd)
    mpi_homography(tgt_pose + (size_t)bv * 16, intrinsics + (size_t)b * 9, tgt_intrinsics_inv + (size_t)bv * 9, depths[tid], hom[tid]);
  __syncthreads();
  if (j >= out_w || i >= out_h) return;
  const float uu = (float)j, vv = (float)i;  // meshgrid_abs of the OUTPUT size
  const float wf = (float)width, hf = (float)height;
  const int tx_n = width / TILE_W, table_bytes = (height / TILE_H) * tx_n * 4;
  const char *pool_c = static_cast<const char *>(pool);
  float o0 = 0.f, o1 = 0.f, o2 = 0.f, od = 0.f;

  struct Look : TapTiles {   // of (fy, fx) (fy, cx) (cy, fx) (cy, cx); 0 for a masked tap
    MpiCoords m;
  };
  const auto look_up = [&](int d) {
    Look s;
    s.m = mpi_coords(hom[d], uu, vv, wf, hf, width, height);
    const size_t l = (size_t)b * nd + d;
    const __amdgpu_buffer_rsrc_t T = table_rsrc(table + l * (size_t)(table_bytes >> 2), table_bytes);
    const int ty0 = s.m.fy >> 2, ty1 = (s.m.fy + 1) >> 2;                       // (fy = -1 -> -1: a masked row never equals the row below)
    const unsigned r0 = (unsigned)(ty0 * tx_n), r1 = (unsigned)(ty1 * tx_n);
    const unsigned c0 = (unsigned)(s.m.fx >> 4), c1 = (unsigned)((s.m.fx + 1) >> 4);
    // (a masked tap sends NO_TEXEL; where both rows are in one tile row, both are inside the image)
    tap_tiles(s, T, s.m.x0 && s.m.y0 ? (r0 + c0) << 2 : NO_TEXEL, s.m.x1 && s.m.y0 ? (r0 + c1) << 2 : NO_TEXEL,
              s.m.x0 && s.m.y1 ? (r1 + c0) << 2 : NO_TEXEL, s.m.x1 && s.m.y1 ? (r1 + c1) << 2 : NO_TEXEL, ty0 != ty1);
    return s;
  };
  const auto fetch = [&](int d, const Look &s, bool ok) {
    const size_t l = (size_t)b * nd + d;
    const long long ls = layer_start[l];
    const __amdgpu_buffer_rsrc_t L = pool_rsrc<FMT>(pool_c, ls, layer_start[l + 1] - ls);
    const unsigned i0 = ((unsigned)s.m.fy & 3u) << 4, i1 = ((unsigned)(s.m.fy + 1) & 3u) << 4;
    const unsigned j0 = (unsigned)s.m.fx & 15u, j1 = (unsigned)(s.m.fx + 1) & 15u;
    const auto at = [&](int tile, unsigned in_tile, bool tap_ok) { return ok && tap_ok ? (((unsigned)tile << 6) + in_tile) << SH : NO_TEXEL; };
    RawTaps<FMT> q;
    q.a = raw_tap<FMT>(L, at(s.ia, i0 + j0, s.m.x0 && s.m.y0));
    q.d = raw_tap<FMT>(L, at(s.id, i1 + j1, s.m.x1 && s.m.y1));
    q.c = raw_tap<FMT>(L, at(s.ic, i1 + j0, s.m.x0 && s.m.y1));
    q.b = raw_tap<FMT>(L, at(s.ib, i0 + j1, s.m.x1 && s.m.y0));
    return q;
  };
  // mpi_render_views_kernel's blend: the four weights and the sum order w00 a00 + w11 a11 + w01 a01 + w10 a10, zero for a pixel that samples outside
  const auto blend = [&](const Look &s, const RawTaps<FMT> &q) {
    const MpiCoords &m = s.m;
    const float4 a00 = decode_tap_or_zero<FMT>(q.a, m.x0 && m.y0), a11 = decode_tap_or_zero<FMT>(q.d, m.x1 && m.y1);
    const float4 a01 = decode_tap_or_zero<FMT>(q.c, m.x0 && m.y1), a10 = decode_tap_or_zero<FMT>(q.b, m.x1 && m.y0);
    const float dx = m.dx, dy = m.dy;
    const float w00 = dx * dy, w11 = (1.0f - dx) * (1.0f - dy), w01 = dx * (1.0f - dy), w10 = (1.0f - dx) * dy;
    float4 c;
    c.w = m.inside ? ((w00 * a00.w + w11 * a11.w) + w01 * a01.w) + w10 * a10.w : 0.0f;
    c.x = m.inside ? ((w00 * a00.x + w11 * a11.x) + w01 * a01.x) + w10 * a10.x : 0.0f;
    c.y = m.inside ? ((w00 * a00.y + w11 * a11.y) + w01 * a01.y) + w10 * a10.y : 0.0f;
    c.z = m.inside ? ((w00 * a00.z + w11 * a11.z) + w01 * a01.z) + w10 * a10.z : 0.0f;
    return c;
  };
  for (int d0 = 0; d0 < nd; d0 += PLANAR_GROUP) {
    Look look[PLANAR_GROUP];
    RawTaps<FMT> raw[PLANAR_GROUP];
    bool ok[PLANAR_GROUP], some[PLANAR_GROUP];
#pragma unroll
    for (int g = 0; g < PLANAR_GROUP; ++g) look[g] = look_up(min(d0 + g, nd - 1));     // (past the end: the last layer's again, its step skipped)
#pragma unroll
    for (int g = 0; g < PLANAR_GROUP; ++g) {
      ok[g] = look[g].present();
      some[g] = d0 + g < nd && __builtin_amdgcn_ballot_w64(ok[g]) != 0;                // (wave-uniform)
      raw[g] = RawTaps<FMT>{};
      if (some[g]) raw[g] = fetch(d0 + g, look[g], ok[g]);
    }
#pragma unroll
    for (int g = 0; g < PLANAR_GROUP; ++g) {
      const int d = d0 + g;
      if (!some[g]) continue;
      const float4 c = blend(look[g], raw[g]);
      const Composite n = over_step<MODE>(o0, o1, o2, od, 1.0f, d, c, [&] { return F.f[d]; });
      if (ok[g]) { o0 = n.o0; o1 = n.o1; o2 = n.o2; od = n.od; }
    }
  }
  store_pixel<MODE>(out_rgb, out_depth, ((size_t)bv * out_h + i) * out_w + j, o0, o1, o2, od);
}

// The cube render.  Ray (CAMERA_ODS included), shell hit with hi = S-1, blend and origin test are geo_cube.h's pieces, as in cube_render_views_kernel;
// the clamped tap coordinates are that kernel's.  The face differs per lane, so the table, layer_start
// and the pool get one descriptor per SAMPLE -- the six faces' table rows [6 D, S/4, S/16], their 6 D + 1 entries of layer_start, and the kept tiles
// from layer_start[6 b D] to layer_start[6 (b + 1) D] (below 2^31 bytes: the host refuses a sample whose DENSE stacks reach that) -- and the lane's
// layer f D + d goes into the per-lane offsets.  The layer's first tile, relative to the sample's (the low words' difference: it fits 32 bits), is
// loaded in the look pass next to the table entries: both depend on (f, d) alone.  Clamped taps never leave the face, so every tap is looked up; the
// two tap rows are in one tile row wherever the clamp made them coincide.
template <int MODE, int CAMERA, int FMT>
__global__ void __launch_bounds__(256)
cube_render_views_sparse_kernel(const void *__restrict__ pool, const int *__restrict__ table, const long long *__restrict__ layer_start,
                                const float *__restrict__ pose_rt, const float *__restrict__ tgt_pos, const float *__restrict__ intrinsics,
                                const float *__restrict__ stack_intrinsics, const float *__restrict__ depths, const float *__restrict__ trig,
                                int batch, int views, int face, int nd, int out_h, int out_w, float *__restrict__ out_rgb,
                                float *__restrict__ out_depth, DepthFrac F, int *__restrict__ status) {
  constexpr int SH = StackTexel<FMT>::shift;
  ViewBlock<4> k(out_h, out_w, views, batch);
  if (k.past_end()) return;                             // (grid rounded up to a multiple of 8; whole workgroups leave)
  k.decode(views);
  const unsigned bv = k.bv;
  const int i = k.i, j = k.j, b = k.b;
  if (j >= out_w || i >= out_h) return;                 // (no barrier below; lane (0, 0) of a workgroup is always inside)

  const CubeRay r = cube_ray<CAMERA>(intrinsics, trig, tgt_pos, pose_rt, bv, i, j, out_h, out_w);
  const CubeCamera cam = cube_stack_camera(stack_intrinsics, b);
  const float sm1 = (float)(face - 1);
  const unsigned tx_n = (unsigned)face / TILE_W, ty_n = (unsigned)face / TILE_H;
  const size_t layer0 = (size_t)6 * b * nd;             // the sample's first layer
  const int layers_n = 6 * nd;
  const __amdgpu_buffer_rsrc_t T = table_rsrc(table + layer0 * ty_n * tx_n, (int)(layers_n * ty_n * tx_n * 4u));
  const __amdgpu_buffer_rsrc_t LS = table_rsrc(layer_start + layer0, (layers_n + 1) * 8);
  const long long first = layer_start[layer0];
  const __amdgpu_buffer_rsrc_t L = pool_rsrc<FMT>(static_cast<const char *>(pool), first, layer_start[layer0 + layers_n] - first);
  const unsigned first_lo = (unsigned)first;
  float o0 = 0.f, o1 = 0.f, o2 = 0.f, od = 0.f;
  float hmin = __builtin_inff();

  struct Look : TapTiles {
    float dx0, dy0;
    unsigned in_a, in_b, in_c, in_d;   // the taps' offsets inside their tiles
    unsigned start;                    // the layer's first tile, relative to the sample's
  };
  const auto look_up = [&](int d) {
    Look s;
    const float h = depths[d];
    hmin = fminf(hmin, h);
    const CubeHit p = cube_hit(r, cam, h, sm1);
    const float fx0 = floorf(p.u), fy0 = floorf(p.v);
    s.dx0 = p.u - fx0; s.dy0 = p.v - fy0;
    const int x0 = (int)fx0, y0 = (int)fy0;             // in [0, S-1]
    const int x1 = min(x0 + 1, face - 1), y1 = min(y0 + 1, face - 1);
    const unsigned lr = p.f * (unsigned)nd + (unsigned)d; // the lane's layer within the sample: below 6 D
    const unsigned ty0 = (unsigned)y0 >> 2, ty1 = (unsigned)y1 >> 2;
    const unsigned r0 = (lr * ty_n + ty0) * tx_n, r1 = (lr * ty_n + ty1) * tx_n;
    const unsigned c0 = (unsigned)x0 >> 4, c1 = (unsigned)x1 >> 4;
    s.start = __builtin_amdgcn_raw_buffer_load_b32(LS, lr << 3, 0, 0) - first_lo;
    tap_tiles(s, T, (r0 + c0) << 2, (r0 + c1) << 2, (r1 + c0) << 2, (r1 + c1) << 2, ty0 != ty1);
    const unsigned i0 = ((unsigned)y0 & 3u) << 4, i1 = ((unsigned)y1 & 3u) << 4, j0 = (unsigned)x0 & 15u, j1 = (unsigned)x1 & 15u;
    s.in_a = i0 + j0; s.in_b = i0 + j1; s.in_c = i1 + j0; s.in_d = i1 + j1;
    return s;
  };
  const auto fetch = [&](const Look &s, bool ok) {
    const auto at = [&](int tile, unsigned in_tile) { return ok ? (((s.start + (unsigned)tile) << 6) + in_tile) << SH : NO_TEXEL; };
    RawTaps<FMT> q;
    q.a = raw_tap<FMT>(L, at(s.ia, s.in_a));
    q.b = raw_tap<FMT>(L, at(s.ib, s.in_b));
    q.c = raw_tap<FMT>(L, at(s.ic, s.in_c));
    q.d = raw_tap<FMT>(L, at(s.id, s.in_d));
    return q;
  };
  const auto blend = [&](const Look &s, const RawTaps<FMT> &q) {
    return cube_blend(s.dx0, s.dy0, decode_tap<FMT>(q.a), decode_tap<FMT>(q.b), decode_tap<FMT>(q.c), decode_tap<FMT>(q.d));
  };
  for (int d0 = 0; d0 < nd; d0 += PLANAR_GROUP) {
    Look look[PLANAR_GROUP];
    RawTaps<FMT> raw[PLANAR_GROUP];
    bool ok[PLANAR_GROUP], some[PLANAR_GROUP];
#pragma unroll
    for (int g = 0; g < PLANAR_GROUP; ++g) look[g] = look_up(min(d0 + g, nd - 1));     // (past the end: the last layer's again, its step skipped)
#pragma unroll
    for (int g = 0; g < PLANAR_GROUP; ++g) {
      ok[g] = look[g].present();
      some[g] = d0 + g < nd && __builtin_amdgcn_ballot_w64(ok[g]) != 0;                // (wave-uniform)
      raw[g] = RawTaps<FMT>{};
      if (some[g]) raw[g] = fetch(look[g], ok[g]);
    }
#pragma unroll
    for (int g = 0; g < PLANAR_GROUP; ++g) {
      const int d = d0 + g;
      if (!some[g]) continue;
      const float4 c = blend(look[g], raw[g]);
      const Composite n = over_step<MODE>(o0, o1, o2, od, 1.0f, d, c, [&] { return F.f[d]; });
      if (ok[g]) { o0 = n.o0; o1 = n.o1; o2 = n.o2; od = n.od; }
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

}  // namespace

extern "C" {

int msi_render_views_sparse(const void *pool, const int32_t *table, const int64_t *layer_start, int32_t format, const float *tgt_pose_rt,
                            const float *tgt_pos, const float *intrinsics, const float *eye_radius, const float *depths, const float *trig,
                            int32_t batch, int32_t views, int32_t height, int32_t width, int32_t num_planes, int32_t camera,
                            int32_t out_height, int32_t out_width, float *out_rgb, float *out_depth, int32_t *status_device,
                            msi_stream_t stream) {
  const char *who = "render_views_sparse";
  const ViewArgs a = {who, out_rgb, out_depth, pool && table && layer_start && tgt_pose_rt && tgt_pos && depths, format, SPARSE_FORMATS,
                      SPARSE_FORMATS_NOTE, &camera, trig, intrinsics, eye_radius,
                      batch >= 0 && height > 0 && width > 0 && num_planes > 0, (long)height * width, views, batch, out_height, out_width, 1};
  unsigned grid;
  if (const int e = check_views(a, [&] { return whole_tiles(who, height, width); }, no_check, &grid)) return e;
  if (batch == 0) return MSI_OK;
  const dim3 block(64, RENDER_SEGS);
  const PixConsts K = make_consts(height, width);
  const DepthFrac F = depth_fractions(num_planes);
  hipStream_t s = msi::as_stream(stream);
  auto launch = [&](auto M, auto CAM, auto FMT) {
    constexpr int fmt = decltype(FMT)::value;
    if constexpr (fmt != MSI_LAYERS_F32)
      hipLaunchKernelGGL((render_views_sparse_kernel<decltype(M)::value, decltype(CAM)::value, fmt>), dim3(grid), block, 0, s, pool, table,
                         tile_starts(layer_start), tgt_pose_rt, tgt_pos, intrinsics, eye_radius, depths, trig, batch, views, height, width, num_planes,
                         out_height, out_width, out_rgb, out_depth, K, F, status_device);
  };
  for_view_kernel(render_mode(out_rgb, out_depth), format, eye_radius != nullptr, camera, launch);
  return msi::check_launch(who);
}

int msi_mpi_render_views_sparse(const void *pool, const int32_t *table, const int64_t *layer_start, int32_t format, const float *tgt_pose,
                                const float *intrinsics, const float *tgt_intrinsics_inv, const float *depths, int32_t batch, int32_t views,
                                int32_t height, int32_t width, int32_t num_planes, int32_t out_height, int32_t out_width, float *out_rgb,
                                float *out_depth, msi_stream_t stream) {
  const char *who = "mpi_render_views_sparse";
  const ViewArgs a = {who, out_rgb, out_depth, pool && table && layer_start && tgt_pose && intrinsics && tgt_intrinsics_inv && depths, format,
                      SPARSE_FORMATS, SPARSE_FORMATS_NOTE, nullptr, nullptr, nullptr, nullptr,
                      batch >= 0 && height > 0 && width > 0 && num_planes > 0, (long)height * width, views, batch, out_height, out_width, 4};
  const auto unsupported = [&] {
    if (num_planes > MPI_SPARSE_MAX_PLANES) return msi::fail(MSI_E_UNSUPPORTED, "%s: at most %d planes", who, MPI_SPARSE_MAX_PLANES);
    return whole_tiles(who, height, width);
  };
  unsigned grid;
  if (const int e = check_views(a, unsupported, no_check, &grid)) return e;
  if (batch == 0) return MSI_OK;
  const DepthFrac F = depth_fractions(num_planes);
  hipStream_t s = msi::as_stream(stream);
  for_mode(render_mode(out_rgb, out_depth), [&](auto M) { for_format(format, [&](auto FMT) {
    constexpr int fmt = decltype(FMT)::value;
    if constexpr (fmt != MSI_LAYERS_F32)
      hipLaunchKernelGGL((mpi_render_views_sparse_kernel<decltype(M)::value, fmt>), dim3(grid), dim3(64, 4), 0, s, pool, table, tile_starts(layer_start),
                         tgt_pose, intrinsics, tgt_intrinsics_inv, depths, batch, views, height, width, num_planes, out_height, out_width, out_rgb,
                         out_depth, F);
  }); });
  return msi::check_launch(who);
}

// msi_cube_render_views_sparse and msi_cube_render_ods_views_sparse: one set of checks, one launch.  ods: no camera code, every table required,
// `camera_table` is eye_radius [B*V] (it travels in the kernel's `intrinsics` argument).
static int cube_views_sparse_launch(const char *who, bool ods, const void *pool, const int32_t *table, const int64_t *layer_start, int32_t format,
                                    const float *tgt_pose_rt, const float *tgt_pos, const float *camera_table, const float *stack_intrinsics,
                                    const float *depths, const float *trig, int32_t batch, int32_t views, int32_t face_size, int32_t num_planes,
                                    int32_t camera, int32_t out_height, int32_t out_width, float *out_rgb, float *out_depth,
                                    int32_t *status_device, msi_stream_t stream) {
  const bool inputs = pool && table && layer_start && tgt_pose_rt && tgt_pos && stack_intrinsics && depths && (!ods || (camera_table && trig));
  const ViewArgs a = {who, out_rgb, out_depth, inputs, format, SPARSE_FORMATS, SPARSE_FORMATS_NOTE, ods ? nullptr : &camera, trig, camera_table, nullptr,
                      batch >= 0 && face_size > 0 && num_planes > 0, 0, views, batch, out_height, out_width, 4};
  const auto unsupported = [&] {
    if (num_planes > DEPTH_FRAC_MAX) return msi::fail(MSI_E_UNSUPPORTED, "%s: at most %d planes", who, DEPTH_FRAC_MAX);
    if (face_size % TILE_W == 0) return (int)MSI_OK;        // (and with it S % 4 == 0)
    return msi::fail(MSI_E_UNSUPPORTED, "%s: a sparse cube needs S %% %d == 0 (got %d)", who, TILE_W, face_size);
  };
  const auto sample_bytes = [&] { return cube_sample_bytes_check(who, format, face_size, num_planes); };   // (the DENSE stacks' bound)
  unsigned grid;
  if (const int e = check_views(a, unsupported, sample_bytes, &grid)) return e;
  if (batch == 0) return MSI_OK;
  const DepthFrac F = depth_fractions(num_planes);
  hipStream_t s = msi::as_stream(stream);
  const auto launch = [&](auto M, auto CAM, auto FMT) {
    constexpr int fmt = decltype(FMT)::value;
    if constexpr (fmt != MSI_LAYERS_F32)
      hipLaunchKernelGGL((cube_render_views_sparse_kernel<decltype(M)::value, decltype(CAM)::value, fmt>), dim3(grid), dim3(64, 4), 0, s, pool, table,
                         tile_starts(layer_start), tgt_pose_rt, tgt_pos, camera_table, stack_intrinsics, depths, trig, batch, views, face_size,
                         num_planes, out_height, out_width, out_rgb, out_depth, F, status_device);
  };
  for_view_kernel(render_mode(out_rgb, out_depth), format, ods, camera, launch);
  return msi::check_launch(who);
}

int msi_cube_render_views_sparse(const void *pool, const int32_t *table, const int64_t *layer_start, int32_t format, const float *tgt_pose_rt,
                                 const float *tgt_pos, const float *tgt_intrinsics, const float *stack_intrinsics, const float *depths,
                                 const float *trig, int32_t batch, int32_t views, int32_t face_size, int32_t num_planes, int32_t camera,
                                 int32_t out_height, int32_t out_width, float *out_rgb, float *out_depth, int32_t *status_device,
                                 msi_stream_t stream) {
  return cube_views_sparse_launch("cube_render_views_sparse", false, pool, table, layer_start, format, tgt_pose_rt, tgt_pos, tgt_intrinsics,
                                  stack_intrinsics, depths, trig, batch, views, face_size, num_planes, camera, out_height, out_width, out_rgb, out_depth,
                                  status_device, stream);
}

int msi_cube_render_ods_views_sparse(const void *pool, const int32_t *table, const int64_t *layer_start, int32_t format, const float *tgt_pose_rt,
                                     const float *tgt_pos, const float *eye_radius, const float *stack_intrinsics, const float *depths,
                                     const float *trig, int32_t batch, int32_t views, int32_t face_size, int32_t num_planes,
                                     int32_t out_height, int32_t out_width, float *out_rgb, float *out_depth, int32_t *status_device,
                                     msi_stream_t stream) {
  return cube_views_sparse_launch("cube_render_ods_views_sparse", true, pool, table, layer_start, format, tgt_pose_rt, tgt_pos, eye_radius,
                                  stack_intrinsics, depths, trig, batch, views, face_size, num_planes, MSI_CAMERA_EQUIRECT, out_height, out_width,
                                  out_rgb, out_depth, status_device, stream);
}

}  // extern "C"
