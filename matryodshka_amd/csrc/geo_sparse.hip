// The format of the sparse layer stacks (msi_sparse_index_tiles / _index_tiles_edge / _gather_tiles / _expand): which 4 x 16 tiles of a packed
// [B,D,H,W] stack (rgba8 / rgba16f) a render can see -- the keep rule, for the sphere renders, which wrap, and for the surfaces that do not (the
// planar and cube renders) --, the scan that numbers the kept tiles, and the copies between the dense stack and the pool.  Its one definition of
// the scan and of the tile entry points' checks also serves the high-res builder (geo_sparse_hres.hip); the viewers are in geo_sparse_views.hip.
// The format and the keep rule are stated in msi_hip.h and, in numpy, in matryodshka_amd/sparse.py; kernels first, the C ABI entry points below.
#include "geometry_device.h"
#include "geo_sparse.h"

namespace {

// ---- the keep rule ------------------------------------------------------------------------------------------------------------
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

// One thread per tile: 1 where the tile is kept -- layer 0, or a texel of the tile's 6 x 18 window is not empty --, else 0.  BORDER_WRAP takes the
// window's x modulo W and y modulo H (the sphere renders wrap); BORDER_EDGE clips it to the image (the planar render zero-pads and the cube render
// clamps to the edge of the face: neither reads the opposite border).  Adjacent windows overlap by their borders only, so a texel is read ~1.7
// times, once from HBM.  (BORDER_WRAP / BORDER_EDGE: geo_sparse.h, with hres_keep_kernel)

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

}  // namespace

int sparse_dims(const char *who, int32_t format, int32_t batch, int32_t num_planes, int32_t height, int32_t width, size_t *tiles) {
  MSI_REQUIRE(format >= 0 && format < 32 && ((SPARSE_FORMATS >> format) & 1u), "%s: unknown format %d%s", who, format, SPARSE_FORMATS_NOTE);
  MSI_REQUIRE(batch >= 0 && height > 0 && width > 0 && num_planes > 0, "%s: bad dims", who);
  if (const int e = whole_tiles(who, height, width)) return e;
  MSI_REQUIRE((long)height * width < (1L << 24), "%s: layers of more than 2^24 texels (24-bit texel offsets)", who);
  MSI_REQUIRE((long)batch * num_planes < (1L << 31), "%s: more than 2^31 - 1 layers", who);
  *tiles = (size_t)batch * num_planes * (size_t)(height / TILE_H) * (size_t)(width / TILE_W);
  return MSI_OK;
}

int scan_tiles(const char *who, int32_t *table, int32_t *counts, int32_t batch, int32_t num_planes, int32_t height, int32_t width, hipStream_t s) {
  hipLaunchKernelGGL(sparse_scan_kernel, dim3((unsigned)(batch * num_planes)), dim3(SCAN_THREADS), 0, s, table,
                     (height / TILE_H) * (width / TILE_W), counts);
  return msi::check_launch(who);
}

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
      if (to_pool)
        hipLaunchKernelGGL((sparse_copy_kernel<fmt, true>), dim3(grid_1d(pieces)), dim3(256), 0, s, d, p, table, tile_starts(layer_start), height, width, tiles);
      else
        hipLaunchKernelGGL((sparse_copy_kernel<fmt, false>), dim3(grid_1d(pieces)), dim3(256), 0, s, d, p, table, tile_starts(layer_start), height, width, tiles);
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

}  // extern "C"
