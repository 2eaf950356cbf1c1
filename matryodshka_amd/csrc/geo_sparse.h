// Shared by the three units of the sparse layer stacks -- a packed [B,D,H,W] stack (rgba8 / rgba16f) that stores only the 4 x 16 tiles a render can
// see: a table [B,D,H/4,W/16] of indices into a pool of kept tiles, and layer_start [B D + 1], each layer's first tile:
//   geo_sparse.hip        the format: the keep rule (both borders), the scan, the copies between a dense stack and a pool
//   geo_sparse_hres.hip   the high-res stack built sparse: hres_keep_kernel (both borders), hres_layers_sparse_kernel
//   geo_sparse_views.hip  the viewers reading such a stack: render_views_sparse_kernel, mpi_render_views_sparse_kernel, cube_render_views_sparse_kernel
// and by geo_planar_hres.hip and geo_cube_sweep.hip, whose pp_ / cube_hres_layers_sparse_kernel write their high-res stacks into such a pool: the three
// sparse builders share one launcher (hres_sparse_launch), here.
// Here: ONLY what more than one of them uses.  The format and the keep rule are stated in msi_hip.h and, in numpy, in matryodshka_amd/sparse.py.
#pragma once
#include "geometry_device.h"

namespace {

constexpr int TILE_H = 4, TILE_W = 16;             // texels; a tile row is one 64-byte (rgba8) / 128-byte (rgba16f) run
constexpr int TILE_TEXELS = TILE_H * TILE_W;

// ---- the keep rule's two borders (format: sparse_keep_kernel; hres: hres_keep_kernel) ---------------------------------------------------
// BORDER_WRAP takes a tile's 6 x 18 window modulo the image (the sphere renders wrap); BORDER_EDGE clips it to the image (the planar render zero-pads
// and the cube render clamps to the edge of the face: neither reads the opposite border).
constexpr int BORDER_WRAP = 0, BORDER_EDGE = 1;

// ---- the keep rule's test (format, hres) ----------------------------------------------------------------------------------------
// "alpha decodes to zero" on the raw codes: rgba8 alpha is the top byte of the texel's word; an rgba16f alpha is the top half of the texel's second
// word, and +0 / -0 both decode to zero (a NaN or a denormal does not).  nonzero-result <=> some texel is NOT empty.
template <int FMT> constexpr unsigned ALPHA_MASK = FMT == MSI_LAYERS_RGBA8 ? 0xff000000u : 0x7fff0000u;   // of the texel's word that holds alpha
// the same bits of the code an alpha WOULD be stored as: the encoder of msi_common.h itself on a texel whose only live channel is alpha (the
// compiler drops the colours), so a NaN, a negative, a > 1, a denormal-half or a -0.0 alpha lands where the stored code puts it
template <int FMT> __device__ __forceinline__ unsigned alpha_bits_of(float alpha) {
  const float4 t = make_float4(0.0f, 0.0f, 0.0f, alpha);
  if constexpr (FMT == MSI_LAYERS_RGBA8) return rgba8_encode(t) & ALPHA_MASK<FMT>;
  else return rgba16f_encode(t).y & ALPHA_MASK<FMT>;
}

// ---- buffer resources (hres, views) -----------------------------------------------------------------------------------------------
constexpr unsigned NO_TEXEL = 0x80000000u;       // a byte offset past any image or resource here (each is below 2^31 bytes): a load of it reads zeros

// `bytes` of a table (rows of the tile table, entries of layer_start) from `first`
__device__ __forceinline__ __amdgpu_buffer_rsrc_t table_rsrc(const void *first, int bytes) {
  return __builtin_amdgcn_make_buffer_rsrc(const_cast<void *>(first), 0, bytes, 0x00020000);
}
// `tiles` kept tiles from tile `first` of the pool (a layer's: a texel offset idx * 64 + (y & 3) * 16 + (x & 15) stays below H * W < 2^24 whatever
// the pool's size, and an offset past the layer's tiles reads zeros instead of another layer)
template <int FMT> __device__ __forceinline__ __amdgpu_buffer_rsrc_t pool_rsrc(const char *pool, long long first, long long tiles) {
  constexpr int SH = StackTexel<FMT>::shift;
  const long long bytes = tiles * (long long)(TILE_TEXELS << SH);
  return __builtin_amdgcn_make_buffer_rsrc((void *)(pool + (((size_t)first * TILE_TEXELS) << SH)), 0, (int)(bytes < 0x7fffffffLL ? bytes : 0x7fffffffLL),
                                           0x00020000);
}

// ---- host helpers ---------------------------------------------------------------------------------------------------------------
constexpr unsigned SPARSE_FORMATS = 1u << MSI_LAYERS_RGBA8 | 1u << MSI_LAYERS_RGBA16F;
constexpr const char *SPARSE_FORMATS_NOTE = " (a sparse stack is rgba8 or rgba16f)";

inline int whole_tiles(const char *who, int height, int width) {
  if (height % TILE_H == 0 && width % TILE_W == 0) return MSI_OK;
  return msi::fail(MSI_E_UNSUPPORTED, "%s: a sparse stack needs H %% %d == 0 and W %% %d == 0 (got %d x %d)", who, TILE_H, TILE_W, height, width);
}

inline const long long *tile_starts(const int64_t *layer_start) { return reinterpret_cast<const long long *>(layer_start); }   // (the kernels' type)

// msi_hres_layers_sparse, msi_pp_hres_layers_sparse, msi_cube_hres_layers_sparse, after their checks (format: rgba8 or rgba16f, sparse_dims; `tiles` from
// it; layers = B * D): ONE store policy for the sparse builders.  It needs the pool's bytes, and only layer_start knows them.  A pool is never larger
// than the dense stack: where that stays within the Infinity Cache the answer is known; otherwise layer_start's last entry comes back to the host (the
// caller has just waited for the same number to allocate the pool: the stream is idle).  launch(Const<FMT>, Const<NT>), NT = non-temporal stores,
// unless nothing is kept.
template <class Launch>
int hres_sparse_launch(const char *who, int format, size_t tiles, const int64_t *layer_start, size_t layers, hipStream_t s, Launch launch) {
  const int shift = format == MSI_LAYERS_RGBA8 ? StackTexel<MSI_LAYERS_RGBA8>::shift : StackTexel<MSI_LAYERS_RGBA16F>::shift;
  long long kept = (long long)tiles;
  if (beyond_infinity_cache((tiles * TILE_TEXELS) << shift)) {
    hipError_t e = hipMemcpyAsync(&kept, layer_start + layers, sizeof kept, hipMemcpyDeviceToHost, s);
    if (e == hipSuccess) e = hipStreamSynchronize(s);
    if (e != hipSuccess) return msi::fail(MSI_E_LAUNCH, "%s: %s", who, hipGetErrorString(e));
    MSI_REQUIRE(kept >= 0 && (size_t)kept <= tiles, "%s: layer_start ends at %lld tiles of %zu", who, kept, tiles);
    if (kept == 0) return MSI_OK;
  }
  for_format(format, [&](auto FMT) {
    if constexpr (decltype(FMT)::value != MSI_LAYERS_F32) {
      if (beyond_infinity_cache(((size_t)kept * TILE_TEXELS) << StackTexel<decltype(FMT)::value>::shift)) launch(FMT, Const<1>{});
      else launch(FMT, Const<0>{});
    }
  });
  return msi::check_launch(who);
}

}  // namespace

// Defined in geo_sparse.hip.  sparse_dims: the checks every tile entry point makes; *tiles = B * D * (H / 4) * (W / 16).  scan_tiles: the second
// launch of every index entry point, 0 / 1 flags -> indices and counts.
extern int sparse_dims(const char *who, int32_t format, int32_t batch, int32_t num_planes, int32_t height, int32_t width, size_t *tiles);
extern int scan_tiles(const char *who, int32_t *table, int32_t *counts, int32_t batch, int32_t num_planes, int32_t height, int32_t width, hipStream_t s);
