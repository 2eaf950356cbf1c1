// The high-res stack, built sparse (msi_hres_index_tiles / _index_tiles_edge, msi_hres_layers_sparse): the keep rule of geo_sparse.hip from the low-res alphas, and
// hres_layers_kernel's texel (geo_layers.hip) for kept tiles only.
// hres_layers_kernel stores o.w = the resized alpha: a texel's alpha -- and with it the keep rule -- is a function of the low-res
// alphas alone.  So the table comes first, from [B,h,w,D] alphas, and the texels of kept tiles go straight into the pool; the dense stack never exists.
#include "geometry_device.h"
#include "geo_sparse.h"

namespace {

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

// BORDER (geo_sparse.h): BORDER_WRAP is the window above; BORDER_EDGE applies sparse_keep_kernel<..., BORDER_EDGE>'s rule -- the window clipped to the
// image: run 0 alone in the proof, no wrapped row or column in the walk (the stacks of the planar and cube renders, geo_planar_hres.hip).
template <int FMT, int BORDER>
__global__ void __launch_bounds__(256)
hres_keep_kernel(const float *__restrict__ alphas, int low_h, int low_w, int height, int width, int nd, float sy, float sx, size_t groups,
                 int *__restrict__ table) {
  constexpr unsigned ALL = (1u << HRES_G) - 1u;
  constexpr int RUNS = BORDER == BORDER_WRAP ? 3 : 1;         // runs of window_run per axis
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
    for (int ky = 0; ky < RUNS; ++ky) {
      int ya, yb;
      window_run(ky, ty, TILE_H, height, ya, yb);
      if (yb < ya) continue;
      const int ly0 = hres_axis(ya, sy, low_h).lo, ly1 = hres_axis(yb, sy, low_h).hi;
      for (int kx = 0; kx < RUNS; ++kx) {
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
      if constexpr (BORDER == BORDER_WRAP) y = y < 0 ? height - 1 : (y >= height ? 0 : y);
      else if (y < 0 || y >= height) continue;                 // (clipped: the row outside the image is not in the window)
      for (int c = -1; c <= TILE_W && (found | proven) != ALL; ++c) {
        int x = tx * TILE_W + c;
        if constexpr (BORDER == BORDER_WRAP) x = x < 0 ? width - 1 : (x >= width ? 0 : x);
        else if (x < 0 || x >= width) continue;
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
// its texel (OdsHres::taps -> fetch -> hres_blend, geometry_device.h: the steps of hres_texel), written for kept tiles only, at
// pool[(layer_start[b D + d] + index) * 64 + (i & 3) * 16 + (j & 15)]: a tile row is one 64- / 128-byte run from 16 lanes, every texel of a kept tile
// is stored, the empty ones too, and pool offsets are 64-bit.  Per layer a lane reads its tile's table entry (16 lanes share it; the tile row is the
// block's).  A lane of a dropped tile computes no sample position (when the wave has none the instructions are skipped), blends nothing and stores
// nothing; its eight loads carry NO_TEXEL, an offset past the image (H * W * 12 < 2^28), which a buffer load answers with zeros without a memory
// access -- they stay in the instruction stream so that the loads of layer q + 1 are in flight, unconditionally, while layer q is blended: behind a
// branch of their own every layer's gathers would wait for the layer before (the effect of MSI_HRES_GROUP, geometry_device.h).
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
  const OdsHres px = ods_hres(image0, image1, pose0, pose1, intrinsics, trig, K, b, i, j, height, width);
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
      tp[q].fg = tp[q].bg = TapsB{NO_TEXEL, NO_TEXEL, NO_TEXEL, NO_TEXEL, 0.0f, 0.0f, 0.0f, 0.0f};
      if (idx[q] >= 0) tp[q] = px.taps(depths[d0 + q]);
      rgb[q] = px.fetch(tp[q]);
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

}  // namespace

extern "C" {

// both keep rules: the checks, the keep kernel of `border`, the scan
static int hres_index_tiles(const char *who, int border, const float *alphas, int32_t format, int32_t batch, int32_t low_height, int32_t low_width,
                            int32_t height, int32_t width, int32_t num_planes, int32_t *table_out, int32_t *counts_out, msi_stream_t stream) {
  if (const int e = hres_check(who, alphas && table_out && counts_out, batch, low_height, low_width, height, width, num_planes)) return e;
  if (border == BORDER_EDGE)
    if (const int e = pp_hres_check(who, height, width)) return e;
  size_t tiles;
  if (const int e = sparse_dims(who, format, batch, num_planes, height, width, &tiles)) return e;
  if (batch == 0) return MSI_OK;
  hipStream_t s = msi::as_stream(stream);
  const size_t groups = tiles / HRES_G;
  const float sy = hres_scale(low_height, height), sx = hres_scale(low_width, width);
  for_format(format, [&](auto FMT) {
    constexpr int fmt = decltype(FMT)::value;
    if constexpr (fmt != MSI_LAYERS_F32) {
      if (border == BORDER_EDGE)
        hipLaunchKernelGGL((hres_keep_kernel<fmt, BORDER_EDGE>), dim3(grid_1d(groups)), dim3(256), 0, s, alphas, low_height, low_width, height, width,
                           num_planes, sy, sx, groups, table_out);
      else
        hipLaunchKernelGGL((hres_keep_kernel<fmt, BORDER_WRAP>), dim3(grid_1d(groups)), dim3(256), 0, s, alphas, low_height, low_width, height, width,
                           num_planes, sy, sx, groups, table_out);
    }
  });
  if (const int e = msi::check_launch(who)) return e;
  return scan_tiles(who, table_out, counts_out, batch, num_planes, height, width, s);
}

int msi_hres_index_tiles(const float *alphas, int32_t format, int32_t batch, int32_t low_height, int32_t low_width, int32_t height, int32_t width,
                         int32_t num_planes, int32_t *table_out, int32_t *counts_out, msi_stream_t stream) {
  return hres_index_tiles("hres_index_tiles", BORDER_WRAP, alphas, format, batch, low_height, low_width, height, width, num_planes, table_out, counts_out,
                          stream);
}

int msi_hres_index_tiles_edge(const float *alphas, int32_t format, int32_t batch, int32_t low_height, int32_t low_width, int32_t height, int32_t width,
                              int32_t num_planes, int32_t *table_out, int32_t *counts_out, msi_stream_t stream) {
  return hres_index_tiles("hres_index_tiles_edge", BORDER_EDGE, alphas, format, batch, low_height, low_width, height, width, num_planes, table_out,
                          counts_out, stream);
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
  const float sy = hres_scale(low_height, height), sx = hres_scale(low_width, width);
  const PixConsts K = make_consts(height, width);
  const dim3 grid((unsigned)((width + 255) / 256), height, batch);
  hipStream_t s = msi::as_stream(stream);
  return hres_sparse_launch(who, format, tiles, layer_start, (size_t)batch * num_planes, s, [&](auto FMT, auto NT) {
    hipLaunchKernelGGL((hres_layers_sparse_kernel<decltype(FMT)::value, decltype(NT)::value>), grid, dim3(256), 0, s, ref_image, src_image,
                       ref_curr_pose, src_curr_pose, intrinsics, depths, trig, blend_weights, alphas, low_height, low_width, height, width, num_planes,
                       sy, sx, K, table, tile_starts(layer_start), pool_out);
  });
}

}  // extern "C"
