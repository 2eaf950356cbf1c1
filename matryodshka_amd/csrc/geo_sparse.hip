// Sparse layer stacks (msi_sparse_index_tiles / _gather_tiles / _expand, msi_render_views_sparse): a packed [B,D,H,W] stack (rgba8 / rgba16f) that
// stores only the 4 x 16 tiles a sphere render can see, and K4 reading it directly -- the sphere render of geometry_device.h (the body of
// render_views_kernel, geo_render.hip, and of render_ods_views_kernel, geo_ods.hip) with one table lookup per tap tile in front of the gathers.
// Also here, because they share the tile, the scan and the argument checks: the high-res stack built sparse (msi_hres_index_tiles,
// msi_hres_layers_sparse), the keep rule from the low-res alphas and hres_layers_kernel's texel for kept tiles only; and the stacks of the surfaces
// that do not wrap (msi_sparse_index_tiles_edge, msi_mpi_render_views_sparse, msi_cube_render_views_sparse): the keep rule with its window clipped
// to the image, and the planar and cube renders reading such a stack.
// The format and the keep rule are stated in msi_hip.h and, in numpy, in matryodshka_amd/sparse.py; kernels first, the C ABI entry points below.
#include "geometry_device.h"

namespace {

constexpr int TILE_H = 4, TILE_W = 16;             // texels; a tile row is one 64-byte (rgba8) / 128-byte (rgba16f) run
constexpr int TILE_TEXELS = TILE_H * TILE_W;

// ---- the keep rule ------------------------------------------------------------------------------------------------------------
// "alpha decodes to zero" on the raw codes: rgba8 alpha is the top byte of the texel's word; an rgba16f alpha is the top half of the texel's second
// word, and +0 / -0 both decode to zero (a NaN or a denormal does not).  nonzero-result <=> some texel is NOT empty.
template <int FMT> constexpr unsigned ALPHA_MASK = FMT == MSI_LAYERS_RGBA8 ? 0xff000000u : 0x7fff0000u;   // of the texel's word that holds alpha
template <int FMT> __device__ __forceinline__ unsigned alpha_bits16(const char *p) {   // 16 texels from a 16-byte aligned address
  const uint4 *q = reinterpret_cast<const uint4 *>(p);
  if constexpr (FMT == MSI_LAYERS_RGBA8) {
    unsigned r = 0;
#pragma unroll
    for (int k = 0; k < 4; ++k) { const uint4 v = q[k]; r |= (v.x | v.y | v.z | v.w); }
    return r & ALPHA_MASK<FMT>;
  } else {
    unsigned r = 0;
#pragma unroll
    for (int k = 0; k < 8; ++k) { const uint4 v = q[k]; r |= (v.y | v.w); }
    return r & ALPHA_MASK<FMT>;
  }
}
template <int FMT> __device__ __forceinline__ unsigned alpha_bits1(const char *p) {    // one texel
  if constexpr (FMT == MSI_LAYERS_RGBA8) return *reinterpret_cast<const unsigned *>(p) & ALPHA_MASK<FMT>;
  else return reinterpret_cast<const unsigned *>(p)[1] & ALPHA_MASK<FMT>;
}
// the same bits of the code an alpha WOULD be stored as: the encoder of msi_common.h itself on a texel whose only live channel is alpha (the
// compiler drops the colours), so a NaN, a negative, a > 1, a denormal-half or a -0.0 alpha lands where the stored code puts it
template <int FMT> __device__ __forceinline__ unsigned alpha_bits_of(float alpha) {
  const float4 t = make_float4(0.0f, 0.0f, 0.0f, alpha);
  if constexpr (FMT == MSI_LAYERS_RGBA8) return rgba8_encode(t) & ALPHA_MASK<FMT>;
  else return rgba16f_encode(t).y & ALPHA_MASK<FMT>;
}

// One thread per tile: 1 where the tile is kept -- layer 0, or a texel of the tile's 6 x 18 window is not empty --, else 0.  BORDER_WRAP takes the
// window's x modulo W and y modulo H (the sphere renders wrap); BORDER_EDGE clips it to the image (the planar render zero-pads and the cube render
// clamps to the edge of the face: neither reads the opposite border).  Adjacent windows overlap by their borders only, so a texel is read ~1.7
// times, once from HBM.
constexpr int BORDER_WRAP = 0, BORDER_EDGE = 1;

template <int FMT, int BORDER>
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
    if constexpr (BORDER == BORDER_WRAP) {
      const int xl = x0 == 0 ? width - 1 : x0 - 1, xr = x0 + TILE_W == width ? 0 : x0 + TILE_W;
      for (int r = -1; r <= TILE_H && !any; ++r) {
        int y = ty * TILE_H + r;
        y = y < 0 ? height - 1 : (y >= height ? 0 : y);
        const char *row = base + (((size_t)y * width) << SH);
        any = alpha_bits16<FMT>(row + ((size_t)x0 << SH)) | alpha_bits1<FMT>(row + ((size_t)xl << SH)) | alpha_bits1<FMT>(row + ((size_t)xr << SH));
      }
    } else {
      // (a column outside the image is replaced by the tile's own first / last column, which alpha_bits16 covers already: nothing is added, no branch)
      const int xl = x0 == 0 ? x0 : x0 - 1, xr = x0 + TILE_W == width ? x0 + TILE_W - 1 : x0 + TILE_W;
      const int y_first = max(ty * TILE_H - 1, 0), y_last = min(ty * TILE_H + TILE_H, height - 1);
      for (int y = y_first; y <= y_last && !any; ++y) {
        const char *row = base + (((size_t)y * width) << SH);
        any = alpha_bits16<FMT>(row + ((size_t)x0 << SH)) | alpha_bits1<FMT>(row + ((size_t)xl << SH)) | alpha_bits1<FMT>(row + ((size_t)xr << SH));
      }
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

// ---- the high-res stack, built sparse (msi_hres_index_tiles, msi_hres_layers_sparse) ----------------------------------------------------------
// hres_layers_kernel (geo_layers.hip) stores o.w = the resized alpha: a texel's alpha -- and with it the keep rule -- is a function of the low-res
// alphas alone.  So the table comes first, from [B,h,w,D] alphas, and the texels of kept tiles go straight into the pool; the dense stack never exists.
//
// The keep pass.  One thread per tile x group of HRES_G layers (alphas are layer-fastest: hres_lerp covers the group; the groups of a tile are
// neighbouring lanes, so a wave reads whole 128-byte lines of the low-res tensor): the flags of sparse_keep_kernel for the alphas the dense kernel
// would have stored.  The decision is the walk: the tile's 6 x 18 window, each texel's alpha by the dense kernel's expression (hres_corners /
// hres_lerp, geometry_device.h) through the encoder, until every layer of the group has a texel that is not empty.  In front of it, a proof that
// spares most dropped tiles the walk: the window's texels interpolate the low-res texels of at most 3 x 3 rectangles (hres_axis is monotone; the
// wrapped row and column are rectangles of their own), a lerp2 of values in [lo, hi] lies in [lo, hi] widened by its rounding (three roundings per
// lerp, two levels: < 16 ulp of max(|lo|, |hi|); 2^-18 of it is taken), and both encoders are monotone with the empty codes an interval around
// zero -- so when the encoder calls both widened ends empty (and every value is finite), every texel of the window is empty.  A layer proven empty is not
// walked for; the walk decides the rest.  No zeroing, no atomics, no store race.  groups = B * tiles per layer * D / HRES_G.
template <int FMT> __device__ __forceinline__ bool range_is_empty(float lo, float hi) {
  const float slack = fmaxf(fabsf(lo), fabsf(hi)) * 0x1p-18f;
  return (alpha_bits_of<FMT>(lo - slack) | alpha_bits_of<FMT>(hi + slack)) == 0u;
}

// run k of the window along one axis of n texels in tiles of `tile`: 0 the tile and its neighbours inside the image, 1 the wrapped neighbour of
// the first tile, 2 that of the last; empty (last < first) where there is none
__device__ __forceinline__ void window_run(int k, int tile_index, int tile, int n, int &first, int &last) {
  const int t0 = tile_index * tile;
  if (k == 0) { first = max(t0 - 1, 0); last = min(t0 + tile, n - 1); }
  else if (k == 1) { first = n - 1; last = t0 == 0 ? n - 1 : n - 2; }
  else { first = 0; last = t0 + tile == n ? 0 : -1; }
}

template <int FMT>
__global__ void __launch_bounds__(256)
hres_keep_kernel(const float *__restrict__ alphas, int low_h, int low_w, int height, int width, int nd, float sy, float sx, size_t groups,
                 int *__restrict__ table) {
  constexpr unsigned ALL = (1u << HRES_G) - 1u;
  const int tx_n = width / TILE_W, ty_n = height / TILE_H;
  const size_t per_layer = (size_t)tx_n * ty_n, dg_n = (size_t)(nd / HRES_G);
  for (size_t g = (size_t)blockIdx.x * blockDim.x + threadIdx.x; g < groups; g += (size_t)gridDim.x * blockDim.x) {
    const size_t bt = g / dg_n;                                // sample * tiles per layer + tile
    const int d0 = (int)(g - bt * dg_n) * HRES_G;
    const size_t b = bt / per_layer;
    const int t = (int)(bt - b * per_layer);
    const int ty = t / tx_n, tx = t - ty * tx_n;
    const float *al = alphas + b * (size_t)low_h * low_w * nd + d0;
    unsigned found = d0 == 0 ? 1u : 0u;                        // bit q: layer d0 + q is kept (layer 0 always)

    float lo[HRES_G], hi[HRES_G];
    unsigned nan = 0u;
#pragma unroll
    for (int q = 0; q < HRES_G; ++q) { lo[q] = INFINITY; hi[q] = -INFINITY; }
    for (int ky = 0; ky < 3; ++ky) {
      int ya, yb;
      window_run(ky, ty, TILE_H, height, ya, yb);
      if (yb < ya) continue;
      const int ly0 = hres_axis(ya, sy, low_h).lo, ly1 = hres_axis(yb, sy, low_h).hi;
      for (int kx = 0; kx < 3; ++kx) {
        int xa, xb;
        window_run(kx, tx, TILE_W, width, xa, xb);
        if (xb < xa) continue;
        const int lx0 = hres_axis(xa, sx, low_w).lo, lx1 = hres_axis(xb, sx, low_w).hi;
        for (int ly = ly0; ly <= ly1; ++ly)
          for (int lx = lx0; lx <= lx1; ++lx) {
            const hres_vec v = *reinterpret_cast<const hres_vec *>(al + (unsigned)(ly * low_w + lx) * (unsigned)nd);
#pragma unroll
            for (int q = 0; q < HRES_G; ++q) {
              lo[q] = fminf(lo[q], v[q]); hi[q] = fmaxf(hi[q], v[q]);
              nan |= fabsf(v[q]) < INFINITY ? 0u : 1u << q;       // (a NaN or an infinity: nothing is proven, the walk decides)
            }
          }
      }
    }
    unsigned proven = 0u;                                      // bit q: every texel of the window is empty in layer d0 + q
#pragma unroll
    for (int q = 0; q < HRES_G; ++q) proven |= !((nan >> q) & 1u) && range_is_empty<FMT>(lo[q], hi[q]) ? 1u << q : 0u;

    for (int r = -1; r <= TILE_H && (found | proven) != ALL; ++r) {
      int y = ty * TILE_H + r;
      y = y < 0 ? height - 1 : (y >= height ? 0 : y);
      for (int c = -1; c <= TILE_W && (found | proven) != ALL; ++c) {
        int x = tx * TILE_W + c;
        x = x < 0 ? width - 1 : (x >= width ? 0 : x);
        const hres_vec av = hres_lerp(al, hres_corners(y, x, sy, sx, low_h, low_w, nd));
#pragma unroll
        for (int q = 0; q < HRES_G; ++q) found |= alpha_bits_of<FMT>(av[q]) ? 1u << q : 0u;
      }
    }
#pragma unroll
    for (int q = 0; q < HRES_G; ++q) table[(b * nd + (size_t)(d0 + q)) * per_layer + t] = (int)((found >> q) & 1u);
  }
}

// The texel pass: hres_layers_kernel's mapping (a lane is one pixel of a 256-column run of row blockIdx.y and walks the layers in groups of HRES_G) and
// its texel (hres_taps -> hres_fetch -> hres_blend, geometry_device.h: the steps of hres_texel), written for kept tiles only, at
// pool[(layer_start[b D + d] + index) * 64 + (i & 3) * 16 + (j & 15)]: a tile row is one 64- / 128-byte run from 16 lanes, every texel of a kept tile
// is stored, the empty ones too, and pool offsets are 64-bit.  Per layer a lane reads its tile's table entry (16 lanes share it; the tile row is the
// block's).  A lane of a dropped tile computes no sample position (when the wave has none the instructions are skipped), blends nothing and stores
// nothing; its eight loads carry an offset past the image, which a buffer load answers with zeros without a memory access -- they stay in the
// instruction stream so that the loads of layer q + 1 are in flight, unconditionally, while layer q is blended: behind a branch of their own every
// layer's gathers would wait for the layer before (the effect of MSI_HRES_GROUP, geometry_device.h).
constexpr unsigned HRES_NO_TEXEL = 0x80000000u;               // a byte offset past any image (H * W * 12 < 2^28)

template <int FMT, int NT>
__global__ void __launch_bounds__(256) __attribute__((amdgpu_waves_per_eu(MSI_HRES_WAVES, 8)))
hres_layers_sparse_kernel(const float *__restrict__ image0, const float *__restrict__ image1, const float *__restrict__ pose0,
                          const float *__restrict__ pose1, const float *__restrict__ intrinsics, const float *__restrict__ depths,
                          const float *__restrict__ trig, const float *__restrict__ blend_weights, const float *__restrict__ alphas,
                          int low_h, int low_w, int height, int width, int nd, float sy, float sx, PixConsts K,
                          const int *__restrict__ table, const long long *__restrict__ layer_start, void *__restrict__ pool) {
  // grid = (ceil(W / 256), H, B): one thread per pixel, all layers
  const int j = blockIdx.x * 256 + threadIdx.x;
  if (j >= width) return;
  const int i = blockIdx.y, b = blockIdx.z;
  const HresPixel px = hres_pixel(image0, image1, pose0, pose1, intrinsics, trig, b, i, j, height, width);
  const HresCorners k = hres_corners(i, j, sy, sx, low_h, low_w, nd);
  const size_t low_base = (size_t)b * low_h * low_w * nd;
  const float *bw = blend_weights + low_base, *al = alphas + low_base;

  const int tx_n = width / TILE_W;
  const size_t per_layer = (size_t)tx_n * (height / TILE_H);
  const size_t layer0 = (size_t)b * nd;
  const int *entry = table + layer0 * per_layer + (size_t)(i / TILE_H) * tx_n + (j / TILE_W);   // this pixel's tile in layer 0
  const unsigned in_tile = (unsigned)((i % TILE_H) * TILE_W + (j % TILE_W));
  for (int d0 = 0; d0 < nd; d0 += HRES_G) {
    int idx[HRES_G];
    int none = -1;
#pragma unroll
    for (int q = 0; q < HRES_G; ++q) { idx[q] = entry[(size_t)(d0 + q) * per_layer]; none &= idx[q]; }
    if (none < 0) continue;                                    // every tile of the group dropped (the sign bits are all set)
    const hres_vec wv = hres_lerp(bw + d0, k);
    const hres_vec av = hres_lerp(al + d0, k);
    HresTaps tp[HRES_G];
    HresRgb rgb[HRES_G];
    const auto stage = [&](int q) {
      tp[q].fg = tp[q].bg = TapsB{HRES_NO_TEXEL, HRES_NO_TEXEL, HRES_NO_TEXEL, HRES_NO_TEXEL, 0.0f, 0.0f, 0.0f, 0.0f};
      if (idx[q] >= 0) tp[q] = hres_taps(px, depths[d0 + q], K, width, height);
      rgb[q] = hres_fetch(px, tp[q]);
    };
    const auto finish = [&](int q) {
      if (idx[q] >= 0) {
        const float4 o = hres_blend(tp[q], rgb[q], wv[q], av[q]);
        const size_t tile = (size_t)layer_start[layer0 + (size_t)(d0 + q)] + (size_t)idx[q];
        hres_store_packed<FMT, NT>(pool, tile * TILE_TEXELS + in_tile, o);
      }
    };
#pragma unroll
    for (int q = 0; q < HRES_G; ++q) {
      stage(q);
      if (q > 0) finish(q - 1);
    }
    finish(HRES_G - 1);
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

// ---- the planar and cube renders from an edge-rule stack (msi_mpi_render_views_sparse, msi_cube_render_views_sparse) ----------------------------
// Both are the dense kernel's pixel (mpi_render_views_kernel, geo_planar.hip; cube_render_views_kernel, geo_cube.hip) around another layer loop.  The
// layers go in groups of PLANAR_GROUP, and a group in three passes, each a run of independent memory operations:
//   look    the layer's geometry and the table entries of its tap tiles (a second dependent round trip in front of every gather);
//   fetch   the four texel loads, undecoded, for the layers on which some lane of the wavefront has every tap tile present -- a wave-uniform branch
//           around loads alone;
//   blend   decode, the dense kernel's weights and sum order, the dense kernel's over step, for the lanes that are present.
// (What hipcc makes of it -- profiles/sparse_planar_isa.txt: a layer's own loads issue together, a layer's results are waited for before the next
// layer's loads issue.  A form whose binary issues the group's loads back to back measured no faster: profiles/sparse_planar_timing.txt.)
// A lane with a tap in a dropped tile leaves its composite as it is: by the edge rule every alpha of its footprint is zero, the dense blend gives
// alpha 0 and the dense step is c 0 + o 1 = o (a zero's sign may differ; colours must be finite there).  Its loads carry an offset past the
// resource, which a buffer load answers with zeros without a memory access.
constexpr int PLANAR_GROUP = 2;                  // (SPARSE_GROUP's: at 4 the cube kernels need 76-84 VGPRs, 5-6 waves per SIMD instead of 8)
constexpr unsigned NO_TEXEL = 0x80000000u;       // a byte offset past any resource here (each is below 2^31 bytes)

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

// A layer's table row(s) and kept tiles as buffer resources (SparseStack has the reasoning): `tiles` kept tiles from tile `first` of the pool.
template <int FMT> __device__ __forceinline__ __amdgpu_buffer_rsrc_t pool_rsrc(const char *pool, long long first, long long tiles) {
  constexpr int SH = StackTexel<FMT>::shift;
  const long long bytes = tiles * (long long)(TILE_TEXELS << SH);
  return __builtin_amdgcn_make_buffer_rsrc((void *)(pool + (((size_t)first * TILE_TEXELS) << SH)), 0, (int)(bytes < 0x7fffffffLL ? bytes : 0x7fffffffLL),
                                           0x00020000);
}

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

  struct Look {
    MpiCoords m;
    int ia, ib, ic, id;   // the pool tiles of (fy, fx) (fy, cx) (cy, fx) (cy, cx); 0 for a masked tap, -1 = dropped
  };
  const auto look_up = [&](int d) {
    Look s;
    s.m = mpi_coords(hom[d], uu, vv, wf, hf, width, height);
    const size_t l = (size_t)b * nd + d;
    const __amdgpu_buffer_rsrc_t T = __builtin_amdgcn_make_buffer_rsrc((void *)(table + l * (size_t)(table_bytes >> 2)), 0, table_bytes, 0x00020000);
    const int ty0 = s.m.fy >> 2, ty1 = (s.m.fy + 1) >> 2;                       // (fy = -1 -> -1: a masked row never equals the row below)
    const unsigned r0 = (unsigned)(ty0 * tx_n), r1 = (unsigned)(ty1 * tx_n);
    const unsigned c0 = (unsigned)(s.m.fx >> 4), c1 = (unsigned)((s.m.fx + 1) >> 4);
    s.ia = (int)__builtin_amdgcn_raw_buffer_load_b32(T, s.m.x0 && s.m.y0 ? (r0 + c0) << 2 : NO_TEXEL, 0, 0);
    s.ib = (int)__builtin_amdgcn_raw_buffer_load_b32(T, s.m.x1 && s.m.y0 ? (r0 + c1) << 2 : NO_TEXEL, 0, 0);
    // the shortcut of SparseStack::lookup: a wave is 64 neighbouring pixels of one target row
    if (__builtin_amdgcn_ballot_w64(ty0 != ty1) != 0) {
      s.ic = (int)__builtin_amdgcn_raw_buffer_load_b32(T, s.m.x0 && s.m.y1 ? (r1 + c0) << 2 : NO_TEXEL, 0, 0);
      s.id = (int)__builtin_amdgcn_raw_buffer_load_b32(T, s.m.x1 && s.m.y1 ? (r1 + c1) << 2 : NO_TEXEL, 0, 0);
    } else {                                                                       // (both rows in one tile row: both inside the image)
      s.ic = s.ia; s.id = s.ib;
    }
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
      ok[g] = (look[g].ia | look[g].ib | look[g].ic | look[g].id) >= 0;
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

// The cube render.  Rays, shell, face and clamped taps are cube_render_views_kernel's, op for op.  The face differs per lane, so the table, layer_start
// and the pool get one descriptor per SAMPLE -- the six faces' table rows [6 D, S/4, S/16], their 6 D + 1 entries of layer_start, and the kept tiles
// from layer_start[6 b D] to layer_start[6 (b + 1) D] (below 2^31 bytes: the host refuses a sample whose DENSE stacks reach that) -- and the lane's
// layer f D + d goes into the per-lane offsets.  The layer's first tile, relative to the sample's (the low words' difference: it fits 32 bits), is
// loaded in the look pass next to the table entries: both depend on (f, d) alone.  Clamped taps never leave the face, so every tap is looked up; when
// no lane of the wavefront has its two tap rows in different tile rows (always so where the clamp made them coincide) the second row shares the
// first row's lookups.
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
  const unsigned tx_n = (unsigned)face / TILE_W, ty_n = (unsigned)face / TILE_H;
  const size_t layer0 = (size_t)6 * b * nd;             // the sample's first layer
  const int layers_n = 6 * nd;
  const __amdgpu_buffer_rsrc_t T = __builtin_amdgcn_make_buffer_rsrc((void *)(table + layer0 * ty_n * tx_n), 0, (int)(layers_n * ty_n * tx_n * 4u), 0x00020000);
  const __amdgpu_buffer_rsrc_t LS = __builtin_amdgcn_make_buffer_rsrc((void *)(layer_start + layer0), 0, (layers_n + 1) * 8, 0x00020000);
  const long long first = layer_start[layer0];
  const __amdgpu_buffer_rsrc_t L = pool_rsrc<FMT>(static_cast<const char *>(pool), first, layer_start[layer0 + layers_n] - first);
  const unsigned first_lo = (unsigned)first;
  float o0 = 0.f, o1 = 0.f, o2 = 0.f, od = 0.f;
  float hmin = inf;

  struct Look {
    float dx0, dy0;
    unsigned in_a, in_b, in_c, in_d;   // the taps' offsets inside their tiles
    int ia, ib, ic, id;                // the pool tiles of (y0, x0) (y0, x1) (y1, x0) (y1, x1) within their layer, -1 = dropped
    unsigned start;                    // the layer's first tile, relative to the sample's
  };
  const auto look_up = [&](int d) {
    Look s;
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
    s.dx0 = u - fx0; s.dy0 = v - fy0;
    const int x0 = (int)fx0, y0 = (int)fy0;             // in [0, S-1]
    const int x1 = min(x0 + 1, face - 1), y1 = min(y0 + 1, face - 1);
    const unsigned lr = f * (unsigned)nd + (unsigned)d; // the lane's layer within the sample: below 6 D
    const unsigned ty0 = (unsigned)y0 >> 2, ty1 = (unsigned)y1 >> 2;
    const unsigned r0 = (lr * ty_n + ty0) * tx_n, r1 = (lr * ty_n + ty1) * tx_n;
    const unsigned c0 = (unsigned)x0 >> 4, c1 = (unsigned)x1 >> 4;
    s.start = __builtin_amdgcn_raw_buffer_load_b32(LS, lr << 3, 0, 0) - first_lo;
    s.ia = (int)__builtin_amdgcn_raw_buffer_load_b32(T, (r0 + c0) << 2, 0, 0);
    s.ib = (int)__builtin_amdgcn_raw_buffer_load_b32(T, (r0 + c1) << 2, 0, 0);
    if (__builtin_amdgcn_ballot_w64(ty0 != ty1) != 0) {
      s.ic = (int)__builtin_amdgcn_raw_buffer_load_b32(T, (r1 + c0) << 2, 0, 0);
      s.id = (int)__builtin_amdgcn_raw_buffer_load_b32(T, (r1 + c1) << 2, 0, 0);
    } else {
      s.ic = s.ia; s.id = s.ib;
    }
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
  // cube_render_views_kernel's blend: wa A + wb B + wc C + wd D
  const auto blend = [&](const Look &s, const RawTaps<FMT> &q) {
    const float4 A = decode_tap<FMT>(q.a), Bv = decode_tap<FMT>(q.b), C = decode_tap<FMT>(q.c), Dv = decode_tap<FMT>(q.d);
    const float dx0 = s.dx0, dy0 = s.dy0, dx1 = 1.0f - dx0, dy1 = 1.0f - dy0;
    const float wa = dy1 * dx1, wb = dy1 * dx0, wc = dy0 * dx1, wd = dy0 * dx0;
    float4 c;
    c.w = ((wa * A.w + wb * Bv.w) + wc * C.w) + wd * Dv.w;
    c.x = ((wa * A.x + wb * Bv.x) + wc * C.x) + wd * Dv.x;
    c.y = ((wa * A.y + wb * Bv.y) + wc * C.y) + wd * Dv.y;
    c.z = ((wa * A.z + wb * Bv.z) + wc * C.z) + wd * Dv.z;
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
      ok[g] = (look[g].ia | look[g].ib | look[g].ic | look[g].id) >= 0;
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
  // the origin is a property of the view: every lane agrees (fmaxf drops a NaN, so it is tested by itself)
  if (status != nullptr && threadIdx.x == 0 && threadIdx.y == 0) {
    const float omax = fmaxf(fmaxf(fabsf(ox), fabsf(oy)), fabsf(oz));
    if (!(omax < hmin) || ox != ox || oy != oy || oz != oz) atomicOr(status, MSI_RENDER_STATUS_ORIGIN_OUTSIDE);
  }
  store_pixel<MODE>(out_rgb, out_depth, ((size_t)bv * out_h + i) * out_w + j, o0, o1, o2, od);
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

// the second launch of both index entry points: 0 / 1 flags -> indices and counts
int scan_tiles(const char *who, int32_t *table, int32_t *counts, int32_t batch, int32_t num_planes, int32_t height, int32_t width, hipStream_t s) {
  hipLaunchKernelGGL(sparse_scan_kernel, dim3((unsigned)(batch * num_planes)), dim3(SCAN_THREADS), 0, s, table,
                     (height / TILE_H) * (width / TILE_W), counts);
  return msi::check_launch(who);
}

}  // namespace

extern "C" {

// both keep rules: the checks, the keep kernel of `border`, the scan
static int index_tiles(const char *who, int border, const void *layers, int32_t format, int32_t batch, int32_t num_planes, int32_t height, int32_t width,
                       int32_t *table_out, int32_t *counts_out, msi_stream_t stream) {
  MSI_REQUIRE(layers && table_out && counts_out, "%s: null pointer", who);
  size_t tiles;
  if (const int e = sparse_dims(who, format, batch, num_planes, height, width, &tiles)) return e;
  if (batch == 0) return MSI_OK;
  hipStream_t s = msi::as_stream(stream);
  for_format(format, [&](auto FMT) {
    constexpr int fmt = decltype(FMT)::value;
    if constexpr (fmt != MSI_LAYERS_F32) {
      const char *in = static_cast<const char *>(layers);
      if (border == BORDER_EDGE)
        hipLaunchKernelGGL((sparse_keep_kernel<fmt, BORDER_EDGE>), dim3(grid_1d(tiles)), dim3(256), 0, s, in, num_planes, height, width, tiles, table_out);
      else
        hipLaunchKernelGGL((sparse_keep_kernel<fmt, BORDER_WRAP>), dim3(grid_1d(tiles)), dim3(256), 0, s, in, num_planes, height, width, tiles, table_out);
    }
  });
  if (const int e = msi::check_launch(who)) return e;
  return scan_tiles(who, table_out, counts_out, batch, num_planes, height, width, s);
}

int msi_sparse_index_tiles(const void *layers, int32_t format, int32_t batch, int32_t num_planes, int32_t height, int32_t width,
                           int32_t *table_out, int32_t *counts_out, msi_stream_t stream) {
  return index_tiles("sparse_index_tiles", BORDER_WRAP, layers, format, batch, num_planes, height, width, table_out, counts_out, stream);
}

int msi_sparse_index_tiles_edge(const void *layers, int32_t format, int32_t batch, int32_t num_planes, int32_t height, int32_t width,
                                int32_t *table_out, int32_t *counts_out, msi_stream_t stream) {
  return index_tiles("sparse_index_tiles_edge", BORDER_EDGE, layers, format, batch, num_planes, height, width, table_out, counts_out, stream);
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

int msi_hres_index_tiles(const float *alphas, int32_t format, int32_t batch, int32_t low_height, int32_t low_width, int32_t height, int32_t width,
                         int32_t num_planes, int32_t *table_out, int32_t *counts_out, msi_stream_t stream) {
  const char *who = "hres_index_tiles";
  if (const int e = hres_check(who, alphas && table_out && counts_out, batch, low_height, low_width, height, width, num_planes)) return e;
  size_t tiles;
  if (const int e = sparse_dims(who, format, batch, num_planes, height, width, &tiles)) return e;
  if (batch == 0) return MSI_OK;
  hipStream_t s = msi::as_stream(stream);
  const size_t groups = tiles / HRES_G;
  for_format(format, [&](auto FMT) {
    if constexpr (decltype(FMT)::value != MSI_LAYERS_F32)
      hipLaunchKernelGGL((hres_keep_kernel<decltype(FMT)::value>), dim3(grid_1d(groups)), dim3(256), 0, s, alphas, low_height, low_width, height,
                         width, num_planes, hres_scale(low_height, height), hres_scale(low_width, width), groups, table_out);
  });
  if (const int e = msi::check_launch(who)) return e;
  return scan_tiles(who, table_out, counts_out, batch, num_planes, height, width, s);
}

int msi_hres_layers_sparse(const float *ref_image, const float *src_image, const float *ref_curr_pose, const float *src_curr_pose,
                           const float *intrinsics, const float *depths, const float *trig, const float *blend_weights, const float *alphas,
                           int32_t batch, int32_t low_height, int32_t low_width, int32_t height, int32_t width, int32_t num_planes,
                           const int32_t *table, const int64_t *layer_start, void *pool_out, int32_t format, msi_stream_t stream) {
  const char *who = "hres_layers_sparse";
  if (const int e = hres_check(who, ref_image && src_image && ref_curr_pose && src_curr_pose && intrinsics && depths && trig && blend_weights &&
                               alphas && table && layer_start && pool_out, batch, low_height, low_width, height, width, num_planes)) return e;
  size_t tiles;
  if (const int e = sparse_dims(who, format, batch, num_planes, height, width, &tiles)) return e;
  if (batch == 0) return MSI_OK;
  hipStream_t s = msi::as_stream(stream);
  // msi_hres_layers' store policy needs the pool's bytes, and only layer_start knows them.  A pool is never larger than the dense stack: where
  // that stays within the Infinity Cache the answer is known; otherwise layer_start's last entry comes back to the host (the caller has just
  // waited for the same number to allocate the pool: the stream is idle)
  const int shift = format == MSI_LAYERS_RGBA8 ? StackTexel<MSI_LAYERS_RGBA8>::shift : StackTexel<MSI_LAYERS_RGBA16F>::shift;
  long long kept = (long long)tiles;
  if (beyond_infinity_cache((tiles * TILE_TEXELS) << shift)) {
    hipError_t e = hipMemcpyAsync(&kept, layer_start + (size_t)batch * num_planes, sizeof kept, hipMemcpyDeviceToHost, s);
    if (e == hipSuccess) e = hipStreamSynchronize(s);
    if (e != hipSuccess) return msi::fail(MSI_E_LAUNCH, "%s: %s", who, hipGetErrorString(e));
    MSI_REQUIRE(kept >= 0 && (size_t)kept <= tiles, "%s: layer_start ends at %lld tiles of %zu", who, kept, tiles);
    if (kept == 0) return MSI_OK;
  }
  const float sy = hres_scale(low_height, height), sx = hres_scale(low_width, width);
  const PixConsts K = make_consts(height, width);
  const long long *ls = reinterpret_cast<const long long *>(layer_start);
  const dim3 grid((unsigned)((width + 255) / 256), height, batch);
  for_format(format, [&](auto FMT) {
    constexpr int fmt = decltype(FMT)::value;
    if constexpr (fmt != MSI_LAYERS_F32) {
      auto launch = [&](auto NT) {
        hipLaunchKernelGGL((hres_layers_sparse_kernel<fmt, decltype(NT)::value>), grid, dim3(256), 0, s, ref_image, src_image, ref_curr_pose,
                           src_curr_pose, intrinsics, depths, trig, blend_weights, alphas, low_height, low_width, height, width, num_planes, sy, sx,
                           K, table, ls, pool_out);
      };
      // non-temporal stores for a pool that cannot stay in the Infinity Cache (as msi_hres_layers)
      if (beyond_infinity_cache(((size_t)kept * TILE_TEXELS) << StackTexel<fmt>::shift)) launch(Const<1>{});
      else launch(Const<0>{});
    }
  });
  return msi::check_launch(who);
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

int msi_mpi_render_views_sparse(const void *pool, const int32_t *table, const int64_t *layer_start, int32_t format, const float *tgt_pose,
                                const float *intrinsics, const float *tgt_intrinsics_inv, const float *depths, int32_t batch, int32_t views,
                                int32_t height, int32_t width, int32_t num_planes, int32_t out_height, int32_t out_width, float *out_rgb,
                                float *out_depth, msi_stream_t stream) {
  const char *who = "mpi_render_views_sparse";
  const ViewArgs a = {who, out_rgb, out_depth, pool && table && layer_start && tgt_pose && intrinsics && tgt_intrinsics_inv && depths, format,
                      1u << MSI_LAYERS_RGBA8 | 1u << MSI_LAYERS_RGBA16F, " (a sparse stack is rgba8 or rgba16f)", nullptr, nullptr, nullptr, nullptr,
                      batch >= 0 && height > 0 && width > 0 && num_planes > 0, (long)height * width, views, batch, out_height, out_width, 4};
  const auto unsupported = [&] {
    if (num_planes > MPI_SPARSE_MAX_PLANES) return msi::fail(MSI_E_UNSUPPORTED, "%s: at most %d planes", who, MPI_SPARSE_MAX_PLANES);
    if (height % TILE_H == 0 && width % TILE_W == 0) return (int)MSI_OK;
    return msi::fail(MSI_E_UNSUPPORTED, "%s: a sparse stack needs H %% %d == 0 and W %% %d == 0 (got %d x %d)", who, TILE_H, TILE_W, height, width);
  };
  unsigned grid;
  if (const int e = check_views(a, unsupported, no_check, &grid)) return e;
  if (batch == 0) return MSI_OK;
  const DepthFrac F = depth_fractions(num_planes);
  hipStream_t s = msi::as_stream(stream);
  const long long *ls = reinterpret_cast<const long long *>(layer_start);
  for_mode(render_mode(out_rgb, out_depth), [&](auto M) { for_format(format, [&](auto FMT) {
    constexpr int fmt = decltype(FMT)::value;
    if constexpr (fmt != MSI_LAYERS_F32)
      hipLaunchKernelGGL((mpi_render_views_sparse_kernel<decltype(M)::value, fmt>), dim3(grid), dim3(64, 4), 0, s, pool, table, ls, tgt_pose,
                         intrinsics, tgt_intrinsics_inv, depths, batch, views, height, width, num_planes, out_height, out_width, out_rgb, out_depth, F);
  }); });
  return msi::check_launch(who);
}

int msi_cube_render_views_sparse(const void *pool, const int32_t *table, const int64_t *layer_start, int32_t format, const float *tgt_pose_rt,
                                 const float *tgt_pos, const float *tgt_intrinsics, const float *stack_intrinsics, const float *depths,
                                 const float *trig, int32_t batch, int32_t views, int32_t face_size, int32_t num_planes, int32_t camera,
                                 int32_t out_height, int32_t out_width, float *out_rgb, float *out_depth, int32_t *status_device,
                                 msi_stream_t stream) {
  const char *who = "cube_render_views_sparse";
  const ViewArgs a = {who, out_rgb, out_depth, pool && table && layer_start && tgt_pose_rt && tgt_pos && stack_intrinsics && depths, format,
                      1u << MSI_LAYERS_RGBA8 | 1u << MSI_LAYERS_RGBA16F, " (a sparse stack is rgba8 or rgba16f)", &camera, trig, tgt_intrinsics, nullptr,
                      batch >= 0 && face_size > 0 && num_planes > 0, 0, views, batch, out_height, out_width, 4};
  const auto unsupported = [&] {
    if (num_planes > DEPTH_FRAC_MAX) return msi::fail(MSI_E_UNSUPPORTED, "%s: at most %d planes", who, DEPTH_FRAC_MAX);
    if (face_size % TILE_W == 0) return (int)MSI_OK;        // (and with it S % 4 == 0)
    return msi::fail(MSI_E_UNSUPPORTED, "%s: a sparse cube needs S %% %d == 0 (got %d)", who, TILE_W, face_size);
  };
  // the per-sample descriptor of the pool: a sample's kept tiles are addressed with one 32-bit byte offset per lane; they are no more than its dense
  // stacks, which msi_cube_render_views holds to the same bound
  const auto sample_bytes = [&] {
    const int texel_bytes = format == MSI_LAYERS_RGBA16F ? 8 : 4;
    MSI_REQUIRE(face_size < (1 << 15) && (long)face_size * face_size * 6 * num_planes * texel_bytes < (1L << 31),
                "%s: a sample's six face stacks (6 x %d x %d x %d texels of %d bytes) reach 2^31 bytes (32-bit offsets)", who, num_planes,
                face_size, face_size, texel_bytes);
    return (int)MSI_OK;
  };
  unsigned grid;
  if (const int e = check_views(a, unsupported, sample_bytes, &grid)) return e;
  if (batch == 0) return MSI_OK;
  const DepthFrac F = depth_fractions(num_planes);
  hipStream_t s = msi::as_stream(stream);
  const long long *ls = reinterpret_cast<const long long *>(layer_start);
  for_mode(render_mode(out_rgb, out_depth), [&](auto M) { for_camera(camera, [&](auto CAM) { for_format(format, [&](auto FMT) {
    constexpr int fmt = decltype(FMT)::value;
    if constexpr (fmt != MSI_LAYERS_F32)
      hipLaunchKernelGGL((cube_render_views_sparse_kernel<decltype(M)::value, decltype(CAM)::value, fmt>), dim3(grid), dim3(64, 4), 0, s, pool, table,
                         ls, tgt_pose_rt, tgt_pos, tgt_intrinsics, stack_intrinsics, depths, trig, batch, views, face_size, num_planes, out_height,
                         out_width, out_rgb, out_depth, F, status_device);
  }); }); });
  return msi::check_launch(who);
}

}  // extern "C"
