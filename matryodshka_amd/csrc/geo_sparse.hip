// Sparse layer stacks (msi_sparse_index_tiles / _gather_tiles / _expand, msi_render_views_sparse): a packed [B,D,H,W] stack (rgba8 / rgba16f) that
// stores only the 4 x 16 tiles a sphere render can see, and K4 reading it directly -- the sphere render of geometry_device.h (the body of
// render_views_kernel, geo_render.hip, and of render_ods_views_kernel, geo_ods.hip) with one table lookup per tap tile in front of the gathers.
// The format and the keep rule are stated in msi_hip.h and, in numpy, in matryodshka_amd/sparse.py; kernels first, the C ABI entry points below.
#include "geometry_device.h"

namespace {

constexpr int TILE_H = 4, TILE_W = 16;             // texels; a tile row is one 64-byte (rgba8) / 128-byte (rgba16f) run
constexpr int TILE_TEXELS = TILE_H * TILE_W;

// ---- the keep rule ------------------------------------------------------------------------------------------------------------
// "alpha decodes to zero" on the raw codes: rgba8 alpha is the top byte of the texel's word; an rgba16f alpha is the top half of the texel's second
// word, and +0 / -0 both decode to zero (a NaN or a denormal does not).  nonzero-result <=> some texel is NOT empty.
template <int FMT> __device__ __forceinline__ unsigned alpha_bits16(const char *p) {   // 16 texels from a 16-byte aligned address
  const uint4 *q = reinterpret_cast<const uint4 *>(p);
  if constexpr (FMT == MSI_LAYERS_RGBA8) {
    unsigned r = 0;
#pragma unroll
    for (int k = 0; k < 4; ++k) { const uint4 v = q[k]; r |= (v.x | v.y | v.z | v.w); }
    return r & 0xff000000u;
  } else {
    unsigned r = 0;
#pragma unroll
    for (int k = 0; k < 8; ++k) { const uint4 v = q[k]; r |= (v.y | v.w); }
    return r & 0x7fff0000u;
  }
}
template <int FMT> __device__ __forceinline__ unsigned alpha_bits1(const char *p) {    // one texel
  if constexpr (FMT == MSI_LAYERS_RGBA8) return *reinterpret_cast<const unsigned *>(p) & 0xff000000u;
  else return reinterpret_cast<const unsigned *>(p)[1] & 0x7fff0000u;
}

// One thread per tile: 1 where the tile is kept -- layer 0, or a texel of the tile's 6 x 18 window (x modulo W, y modulo H) is not empty --, else 0.
// Adjacent windows overlap by their borders only, so a texel is read ~1.7 times, once from HBM.
template <int FMT>
__global__ void __launch_bounds__(256)
sparse_keep_kernel(const char *__restrict__ layers, int nd, int height, int width, size_t tiles, int *__restrict__ table) {
  constexpr int SH = StackTexel<FMT>::shift;
  const int tx_n = width / TILE_W, ty_n = height / TILE_H;
  const size_t per_layer = (size_t)tx_n * ty_n;
  for (size_t g = (size_t)blockIdx.x * blockDim.x + threadIdx.x; g < tiles; g += (size_t)gridDim.x * blockDim.x) {
    const size_t layer = g / per_layer;
    const int t = (int)(g - layer * per_layer);
    const int ty = t / tx_n, tx = t - ty * tx_n;
    unsigned any = (layer % (size_t)nd) == 0 ? 1u : 0u;
    const char *base = layers + ((layer * (size_t)height * width) << SH);
    const int x0 = tx * TILE_W;
    const int xl = x0 == 0 ? width - 1 : x0 - 1, xr = x0 + TILE_W == width ? 0 : x0 + TILE_W;
    for (int r = -1; r <= TILE_H && !any; ++r) {
      int y = ty * TILE_H + r;
      y = y < 0 ? height - 1 : (y >= height ? 0 : y);
      const char *row = base + (((size_t)y * width) << SH);
      any = alpha_bits16<FMT>(row + ((size_t)x0 << SH)) | alpha_bits1<FMT>(row + ((size_t)xl << SH)) | alpha_bits1<FMT>(row + ((size_t)xr << SH));
    }
    table[g] = any ? 1 : 0;
  }
}

// One workgroup per layer (b, d): the 0 / 1 flags of its tiles, in row-major order, become the tile's index among the kept ones or -1, and the
// layer's count.  Every thread reads and writes its own entries only, the order is the tile order: no atomic decides an index.
constexpr int SCAN_THREADS = 1024;
__global__ void __launch_bounds__(SCAN_THREADS)
sparse_scan_kernel(int *__restrict__ table, int per_layer, int *__restrict__ counts) {
  __shared__ int s_wave[SCAN_THREADS / 64];
  int *t = table + (size_t)blockIdx.x * per_layer;
  const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
  int base = 0;
  for (int c = 0; c < per_layer; c += SCAN_THREADS) {
    const int i = c + (int)threadIdx.x;
    const bool keep = i < per_layer && t[i] != 0;
    const unsigned long long m = __builtin_amdgcn_ballot_w64(keep);
    if (lane == 0) s_wave[wave] = __builtin_popcountll(m);
    __syncthreads();
    int before = 0, total = 0;
#pragma unroll
    for (int w = 0; w < SCAN_THREADS / 64; ++w) {
      const int n = s_wave[w];
      before += w < wave ? n : 0;
      total += n;
    }
    if (i < per_layer) t[i] = keep ? base + before + __builtin_popcountll(m & ((1ull << lane) - 1ull)) : -1;
    base += total;
    __syncthreads();
  }
  if (threadIdx.x == 0) counts[blockIdx.x] = base;
}

// Copies between the dense stack and the pool, one thread per 16 bytes of a tile: TO_POOL gathers the kept tiles, otherwise the dense stack is
// written whole, all-zero bytes in dropped tiles.
template <int FMT, bool TO_POOL>
__global__ void __launch_bounds__(256)
sparse_copy_kernel(char *__restrict__ dense, char *__restrict__ pool, const int *__restrict__ table, const long long *__restrict__ layer_start,
                   int height, int width, size_t tiles) {
  constexpr int SH = StackTexel<FMT>::shift;
  constexpr int ROW_PIECES = (TILE_W << SH) / 16;          // 16-byte pieces of a tile row: 4 (rgba8) / 8 (rgba16f)
  constexpr int PIECES = ROW_PIECES * TILE_H;
  const int tx_n = width / TILE_W, ty_n = height / TILE_H;
  const size_t per_layer = (size_t)tx_n * ty_n, n = tiles * PIECES;
  for (size_t e = (size_t)blockIdx.x * blockDim.x + threadIdx.x; e < n; e += (size_t)gridDim.x * blockDim.x) {
    const size_t g = e / PIECES;
    const int p = (int)(e - g * PIECES), r = p / ROW_PIECES, c = p - r * ROW_PIECES;
    const size_t layer = g / per_layer;
    const int t = (int)(g - layer * per_layer);
    const int ty = t / tx_n, tx = t - ty * tx_n;
    const int idx = table[g];
    uint4 *d = reinterpret_cast<uint4 *>(dense + (((layer * height + (size_t)(ty * TILE_H + r)) * width + (size_t)tx * TILE_W) << SH)) + c;
    uint4 *q = reinterpret_cast<uint4 *>(pool + (((size_t)layer_start[layer] + (size_t)(idx < 0 ? 0 : idx)) * TILE_TEXELS << SH)) + p;
    if (TO_POOL) {
      if (idx >= 0) *q = *d;
    } else {
      *d = idx >= 0 ? *q : make_uint4(0, 0, 0, 0);
    }
  }
}

// ---- K4 from a sparse stack ---------------------------------------------------------------------------------------------------
// make_taps_ranged (geometry_device.h) with the wrapped corner coordinates kept apart instead of folded into flat texel offsets: the same weights,
// op for op, and the same wrapped (x, y) of every corner.
struct TapsS {
  unsigned x0, x1, y0, y1;
  float wa, wb, wc, wd;
};

__device__ __forceinline__ TapsS make_taps_sparse(float x, float y, int width, int height) {
  TapsS t;
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

__device__ __forceinline__ float blend4(const TapsS &t, float a, float b, float c, float d) {
  return ((t.wa * a + t.wb * b) + t.wc * c) + t.wd * d;
}

// The sparse sibling of SphereStack: layer d of sample b is two buffer resources -- its row of the table ([H/4, W/16] int32) and its kept tiles in
// the pool (base = pool + layer_start * tile bytes, num_records = the layer's kept bytes: a texel offset idx * 64 + (y & 3) * 16 + (x & 15) stays
// below H * W < 2^24 whatever the pool's size, and an offset past the layer's tiles reads zeros instead of another layer).  The per-layer step is
// split where the memory round trips are: lookup() is SphereStack::layer up to the taps (sphere_uv) plus the table loads of the tap tiles;
// gather() is its four taps and blends for the lanes whose tap tiles are all present.
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

  struct Look {
    TapsS tp;
    int ia, ib, ic, id;   // the pool tiles of (y0,x0) (y0,x1) (y1,x0) (y1,x1), -1 = dropped
    float qc_max;
  };
  __device__ __forceinline__ Look lookup(int d, const ViewRay &r, const SphereQuad &q, const PixConsts &K, float qc_max) const {
    Look s;
    const SphereUv p = sphere_uv(depths[d], r, q, K);
    s.qc_max = fmaxf(qc_max, p.qc);
    s.tp = make_taps_sparse(p.u, p.v, width, height);
    const size_t l = (size_t)b * nd + d;
    const __amdgpu_buffer_rsrc_t T = __builtin_amdgcn_make_buffer_rsrc((void *)(table + l * (size_t)(table_bytes >> 2)), 0, table_bytes, 0x00020000);
    const unsigned r0 = __umul24(s.tp.y0 >> 2, (unsigned)tx_n), r1 = __umul24(s.tp.y1 >> 2, (unsigned)tx_n);
    const unsigned c0 = s.tp.x0 >> 4, c1 = s.tp.x1 >> 4;
    s.ia = (int)__builtin_amdgcn_raw_buffer_load_b32(T, (r0 + c0) << 2, 0, 0);
    s.ib = (int)__builtin_amdgcn_raw_buffer_load_b32(T, (r0 + c1) << 2, 0, 0);
    // the shortcut: a wave is 64 neighbouring pixels of one target row, so most waves have no footprint across a tile's bottom border
    if (__builtin_amdgcn_ballot_w64(r0 != r1) != 0) {
      s.ic = (int)__builtin_amdgcn_raw_buffer_load_b32(T, (r1 + c0) << 2, 0, 0);
      s.id = (int)__builtin_amdgcn_raw_buffer_load_b32(T, (r1 + c1) << 2, 0, 0);
    } else {
      s.ic = s.ia; s.id = s.ib;
    }
    return s;
  }
  static __device__ __forceinline__ bool present(const Look &s) { return (s.ia | s.ib | s.ic | s.id) >= 0; }

  // (lanes with a dropped tap tile take tile 0 of the layer or, when the layer keeps none, the zeros of an empty resource; the caller discards them)
  __device__ __forceinline__ float4 gather(int d, const Look &s) const {
    constexpr int SH = StackTexel<FMT>::shift;
    const size_t l = (size_t)b * nd + d;
    const long long ls = layer_start[l];
    const int kept_bytes = (int)(layer_start[l + 1] - ls) * (TILE_TEXELS << SH);
    const __amdgpu_buffer_rsrc_t L = __builtin_amdgcn_make_buffer_rsrc((void *)(pool + (((size_t)ls * TILE_TEXELS) << SH)), 0, kept_bytes, 0x00020000);
    const bool ok = present(s);
    const unsigned i0 = (s.tp.y0 & 3u) << 4, i1 = (s.tp.y1 & 3u) << 4, j0 = s.tp.x0 & 15u, j1 = s.tp.x1 & 15u;
    const unsigned ta = ok ? (unsigned)s.ia << 6 : 0u, tb = ok ? (unsigned)s.ib << 6 : 0u, tc = ok ? (unsigned)s.ic << 6 : 0u, td = ok ? (unsigned)s.id << 6 : 0u;
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
      const bool ok = SparseStack<FMT>::present(look[g]);
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

// the checks the three tile entry points share; *tiles = B * D * (H / 4) * (W / 16)
int sparse_dims(const char *who, int32_t format, int32_t batch, int32_t num_planes, int32_t height, int32_t width, size_t *tiles) {
  MSI_REQUIRE(format == MSI_LAYERS_RGBA8 || format == MSI_LAYERS_RGBA16F, "%s: unknown format %d (a sparse stack is rgba8 or rgba16f)", who, format);
  MSI_REQUIRE(batch >= 0 && height > 0 && width > 0 && num_planes > 0, "%s: bad dims", who);
  if (height % TILE_H != 0 || width % TILE_W != 0)
    return msi::fail(MSI_E_UNSUPPORTED, "%s: a sparse stack needs H %% %d == 0 and W %% %d == 0 (got %d x %d)", who, TILE_H, TILE_W, height, width);
  MSI_REQUIRE((long)height * width < (1L << 24), "%s: layers of more than 2^24 texels (24-bit texel offsets)", who);
  MSI_REQUIRE((long)batch * num_planes < (1L << 31), "%s: more than 2^31 - 1 layers", who);
  *tiles = (size_t)batch * num_planes * (size_t)(height / TILE_H) * (size_t)(width / TILE_W);
  return MSI_OK;
}

}  // namespace

extern "C" {

int msi_sparse_index_tiles(const void *layers, int32_t format, int32_t batch, int32_t num_planes, int32_t height, int32_t width,
                           int32_t *table_out, int32_t *counts_out, msi_stream_t stream) {
  MSI_REQUIRE(layers && table_out && counts_out, "sparse_index_tiles: null pointer");
  size_t tiles;
  if (const int e = sparse_dims("sparse_index_tiles", format, batch, num_planes, height, width, &tiles)) return e;
  if (batch == 0) return MSI_OK;
  hipStream_t s = msi::as_stream(stream);
  for_format(format, [&](auto FMT) {
    if constexpr (decltype(FMT)::value != MSI_LAYERS_F32)
      hipLaunchKernelGGL((sparse_keep_kernel<decltype(FMT)::value>), dim3(grid_1d(tiles)), dim3(256), 0, s, static_cast<const char *>(layers),
                         num_planes, height, width, tiles, table_out);
  });
  if (const int e = msi::check_launch("sparse_index_tiles")) return e;
  hipLaunchKernelGGL(sparse_scan_kernel, dim3((unsigned)(batch * num_planes)), dim3(SCAN_THREADS), 0, s, table_out,
                     (height / TILE_H) * (width / TILE_W), counts_out);
  return msi::check_launch("sparse_index_tiles");
}

static int sparse_copy(const char *who, bool to_pool, const void *dense, const void *pool, const int32_t *table, const int64_t *layer_start,
                       int32_t format, int32_t batch, int32_t num_planes, int32_t height, int32_t width, msi_stream_t stream) {
  MSI_REQUIRE(dense && pool && table && layer_start, "%s: null pointer", who);
  size_t tiles;
  if (const int e = sparse_dims(who, format, batch, num_planes, height, width, &tiles)) return e;
  if (batch == 0) return MSI_OK;
  hipStream_t s = msi::as_stream(stream);
  for_format(format, [&](auto FMT) {
    constexpr int fmt = decltype(FMT)::value;
    if constexpr (fmt != MSI_LAYERS_F32) {
      const size_t pieces = tiles * (size_t)(TILE_TEXELS << StackTexel<fmt>::shift) / 16;
      char *d = static_cast<char *>(const_cast<void *>(dense)), *p = static_cast<char *>(const_cast<void *>(pool));
      const long long *ls = reinterpret_cast<const long long *>(layer_start);
      if (to_pool)
        hipLaunchKernelGGL((sparse_copy_kernel<fmt, true>), dim3(grid_1d(pieces)), dim3(256), 0, s, d, p, table, ls, height, width, tiles);
      else
        hipLaunchKernelGGL((sparse_copy_kernel<fmt, false>), dim3(grid_1d(pieces)), dim3(256), 0, s, d, p, table, ls, height, width, tiles);
    }
  });
  return msi::check_launch(who);
}

int msi_sparse_gather_tiles(const void *layers, int32_t format, const int32_t *table, const int64_t *layer_start, int32_t batch,
                            int32_t num_planes, int32_t height, int32_t width, void *pool_out, msi_stream_t stream) {
  return sparse_copy("sparse_gather_tiles", true, layers, pool_out, table, layer_start, format, batch, num_planes, height, width, stream);
}

int msi_sparse_expand(const void *pool, const int32_t *table, const int64_t *layer_start, int32_t format, int32_t batch, int32_t num_planes,
                      int32_t height, int32_t width, void *layers_out, msi_stream_t stream) {
  return sparse_copy("sparse_expand", false, layers_out, pool, table, layer_start, format, batch, num_planes, height, width, stream);
}

int msi_render_views_sparse(const void *pool, const int32_t *table, const int64_t *layer_start, int32_t format, const float *tgt_pose_rt,
                            const float *tgt_pos, const float *intrinsics, const float *eye_radius, const float *depths, const float *trig,
                            int32_t batch, int32_t views, int32_t height, int32_t width, int32_t num_planes, int32_t camera,
                            int32_t out_height, int32_t out_width, float *out_rgb, float *out_depth, int32_t *status_device,
                            msi_stream_t stream) {
  const char *who = "render_views_sparse";
  const ViewArgs a = {who, out_rgb, out_depth, pool && table && layer_start && tgt_pose_rt && tgt_pos && depths, format,
                      1u << MSI_LAYERS_RGBA8 | 1u << MSI_LAYERS_RGBA16F, " (a sparse stack is rgba8 or rgba16f)", &camera, trig, intrinsics, eye_radius,
                      batch >= 0 && height > 0 && width > 0 && num_planes > 0, (long)height * width, views, batch, out_height, out_width, 1};
  unsigned grid;
  const auto tiles = [&] {
    if (height % TILE_H == 0 && width % TILE_W == 0) return (int)MSI_OK;
    return msi::fail(MSI_E_UNSUPPORTED, "%s: a sparse stack needs H %% %d == 0 and W %% %d == 0 (got %d x %d)", who, TILE_H, TILE_W, height, width);
  };
  if (const int e = check_views(a, tiles, no_check, &grid)) return e;
  if (batch == 0) return MSI_OK;
  const dim3 block(64, RENDER_SEGS);
  const PixConsts K = make_consts(height, width);
  const DepthFrac F = depth_fractions(num_planes);
  hipStream_t s = msi::as_stream(stream);
  const long long *ls = reinterpret_cast<const long long *>(layer_start);
  auto launch = [&](auto M, auto CAM, auto FMT) {
    constexpr int fmt = decltype(FMT)::value;
    if constexpr (fmt != MSI_LAYERS_F32)
      hipLaunchKernelGGL((render_views_sparse_kernel<decltype(M)::value, decltype(CAM)::value, fmt>), dim3(grid), block, 0, s, pool, table, ls,
                         tgt_pose_rt, tgt_pos, intrinsics, eye_radius, depths, trig, batch, views, height, width, num_planes, out_height,
                         out_width, out_rgb, out_depth, K, F, status_device);
  };
  for_mode(render_mode(out_rgb, out_depth), [&](auto M) { for_format(format, [&](auto FMT) {
    if (eye_radius) launch(M, Const<CAMERA_ODS>{}, FMT);
    else for_camera(camera, [&](auto CAM) { launch(M, CAM, FMT); });
  }); });
  return msi::check_launch(who);
}

}  // extern "C"
