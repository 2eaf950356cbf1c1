// The high-res layer stack of the PP path in ONE pass (msi_pp_hres_layers, msi_pp_hres_layers_sparse): what the planar viewer (msi_mpi_render_views)
// and the cube-map viewer (msi_cube_render_views) read, fp32 or packed, dense or sparse.  The three-launch form -- pp_sweep_kernel twice (geo_planar.hip)
// -> resize_bilinear_kernel -> assemble_kernel<0, COLOR_BLEND_PSV> (geo_layers.hip) -- writes and re-reads a [B,Hh,Wh,6D] volume and a [B,Hh,Wh,2D]
// tensor; these kernels run the same arithmetic per texel (the PP source PpHres: pp_hres, taps, fetch; then hres_corners / hres_lerp, hres_blend and
// hres_store_packed: geometry_device.h) without contraction, so every texel has the bits of the three launches.  The mapping, the store policy and the
// sparse structure are hres_layers_kernel's (geo_layers.hip: its loop, restated) and hres_layers_sparse_kernel's (geo_sparse_hres.hip: its
// loop, restated), behind the same launchers (hres_dense_launch, hres_sparse_launch); the table of a sparse PP stack comes from
// msi_hres_index_tiles_edge (geo_sparse_hres.hip).  Kernels first, their C ABI entry points below.
#include "geometry_device.h"
#include "geo_sparse.h"

// (groups of HRES_G layers at MSI_HRES_WAVES waves per SIMD, the ODS builder's: 101-105 VGPRs dense, 125 sparse, no scratch -- profiles/pp_hres_isa.txt)

namespace {

// hres_layers_kernel's mapping: grid = (ceil(W / 256), H, B), a lane is one pixel of a 256-column run of row blockIdx.y and walks the layers; S, T and the
// resize corners are per-pixel work done once, K, the poses and both M are per-sample (SGPRs), each layer's store is one contiguous run per wave.
// FMT, WITH_F32, NT: as hres_layers_kernel.  (The loop is written per kernel: as one function under the three dense builders it missed the timing
// margin, profiles/hres_bodies_isa.txt; written out, on the source type, each builder has the instructions it had before.)
template <int FMT, int WITH_F32, int NT>
__global__ void __launch_bounds__(256) __attribute__((amdgpu_waves_per_eu(MSI_HRES_WAVES, MSI_HRES_WAVES)))
pp_hres_layers_kernel(const float *__restrict__ image0, const float *__restrict__ image1, const float *__restrict__ pose0,
                      const float *__restrict__ pose1, const float *__restrict__ intrinsics, const float *__restrict__ depths,
                      const float *__restrict__ blend_weights, const float *__restrict__ alphas, int low_h, int low_w, int height, int width, int nd,
                      float sy, float sx, float s0, float sstep, float t0, float tstep, float4 *__restrict__ rgba, void *__restrict__ packed) {
  const int j = blockIdx.x * 256 + threadIdx.x;
  if (j >= width) return;
  const int i = blockIdx.y, b = blockIdx.z;
  const PpHres px = pp_hres(image0, image1, pose0, pose1, intrinsics, b, i, j, height, width, s0, sstep, t0, tstep);
  const HresCorners k = hres_corners(i, j, sy, sx, low_h, low_w, nd);
  const size_t low_base = (size_t)b * low_h * low_w * nd;          // (h * w * D < 2^31: checked on the host)
  const float *bw = blend_weights + low_base, *al = alphas + low_base;

  const size_t hw = (size_t)height * width;
  size_t texel = (size_t)b * nd * hw + (size_t)i * width + j;      // layer 0 of this pixel in the [B,D,H,W] stack
  for (int d0 = 0; d0 < nd; d0 += HRES_G) {                        // (nd % 4 == 0: checked on the host)
    const hres_vec wv = hres_lerp(bw + d0, k);
    const hres_vec av = hres_lerp(al + d0, k);
#pragma unroll
    for (int q = 0; q < HRES_G; ++q) {
      const float4 o = hres_texel(px, depths[d0 + q], wv[q], av[q]);
      if (WITH_F32) sweep_store16(reinterpret_cast<uint4 *>(rgba + texel), __builtin_bit_cast(uint4, o), NT & 1);
      if constexpr (FMT != MSI_LAYERS_F32) hres_store_packed<FMT, (NT >> 1) & 1>(packed, texel, o);
      texel += hw;
    }
  }
}

// hres_layers_sparse_kernel's structure with the PP source's steps: per layer a lane reads its tile's table entry; a lane of a dropped tile computes no
// sample position, blends nothing and stores nothing, and its eight loads carry NO_TEXEL (past the image: zeros, no memory access), so that the gathers
// of layer q + 1 are in flight, unconditionally, while layer q is blended; pool offsets are 64-bit.  (The loop is written per kernel: shared as one
// function it changes the instruction streams of all three sparse builders and missed the timing margin, profiles/hres_bodies_isa.txt.)
template <int FMT, int NT>
__global__ void __launch_bounds__(256) __attribute__((amdgpu_waves_per_eu(MSI_HRES_WAVES, 8)))
pp_hres_layers_sparse_kernel(const float *__restrict__ image0, const float *__restrict__ image1, const float *__restrict__ pose0,
                             const float *__restrict__ pose1, const float *__restrict__ intrinsics, const float *__restrict__ depths,
                             const float *__restrict__ blend_weights, const float *__restrict__ alphas, int low_h, int low_w, int height, int width,
                             int nd, float sy, float sx, float s0, float sstep, float t0, float tstep, const int *__restrict__ table,
                             const long long *__restrict__ layer_start, void *__restrict__ pool) {
  const int j = blockIdx.x * 256 + threadIdx.x;
  if (j >= width) return;
  const int i = blockIdx.y, b = blockIdx.z;
  const PpHres px = pp_hres(image0, image1, pose0, pose1, intrinsics, b, i, j, height, width, s0, sstep, t0, tstep);
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

int msi_pp_hres_layers(const float *ref_image, const float *src_image, const float *ref_curr_pose, const float *src_curr_pose,
                       const float *intrinsics, const float *depths, const float *blend_weights, const float *alphas, int32_t batch,
                       int32_t low_height, int32_t low_width, int32_t height, int32_t width, int32_t num_planes, float *rgba_native,
                       void *layers_out, int32_t format, msi_stream_t stream) {
  const char *who = "pp_hres_layers";
  MSI_REQUIRE(!layers_out || format == MSI_LAYERS_RGBA8 || format == MSI_LAYERS_RGBA16F, "%s: unknown format %d", who, format);
  MSI_REQUIRE(rgba_native || layers_out, "%s: null pointer (both outputs are NULL)", who);
  if (const int e = hres_check(who, ref_image && src_image && ref_curr_pose && src_curr_pose && intrinsics && depths && blend_weights && alphas, batch,
                               low_height, low_width, height, width, num_planes)) return e;
  if (const int e = pp_hres_check(who, height, width)) return e;
  if (batch == 0) return MSI_OK;
  const float sy = hres_scale(low_height, height), sx = hres_scale(low_width, width);
  const UvGrid gs = uv_grid(width), gt = uv_grid(height);
  const dim3 grid((unsigned)((width + 255) / 256), height, batch);
  hipStream_t s = msi::as_stream(stream);
  hres_dense_launch(format, rgba_native, layers_out, (size_t)batch * num_planes * height * width, [&](auto FMT, auto F32, auto NT) {
    hipLaunchKernelGGL((pp_hres_layers_kernel<decltype(FMT)::value, decltype(F32)::value, decltype(NT)::value>), grid, dim3(256), 0, s, ref_image,
                       src_image, ref_curr_pose, src_curr_pose, intrinsics, depths, blend_weights, alphas, low_height, low_width, height, width,
                       num_planes, sy, sx, gs.start, gs.step, gt.start, gt.step, reinterpret_cast<float4 *>(rgba_native), layers_out);
  });
  return msi::check_launch(who);
}

int msi_pp_hres_layers_sparse(const float *ref_image, const float *src_image, const float *ref_curr_pose, const float *src_curr_pose,
                              const float *intrinsics, const float *depths, const float *blend_weights, const float *alphas, int32_t batch,
                              int32_t low_height, int32_t low_width, int32_t height, int32_t width, int32_t num_planes, const int32_t *table,
                              const int64_t *layer_start, void *pool_out, int32_t format, msi_stream_t stream) {
  const char *who = "pp_hres_layers_sparse";
  if (const int e = hres_check(who, ref_image && src_image && ref_curr_pose && src_curr_pose && intrinsics && depths && blend_weights && alphas &&
                               table && layer_start && pool_out, batch, low_height, low_width, height, width, num_planes)) return e;
  if (const int e = pp_hres_check(who, height, width)) return e;
  size_t tiles;
  if (const int e = sparse_dims(who, format, batch, num_planes, height, width, &tiles)) return e;
  if (batch == 0) return MSI_OK;
  const float sy = hres_scale(low_height, height), sx = hres_scale(low_width, width);
  const UvGrid gs = uv_grid(width), gt = uv_grid(height);
  const dim3 grid((unsigned)((width + 255) / 256), height, batch);
  hipStream_t s = msi::as_stream(stream);
  return hres_sparse_launch(who, format, tiles, layer_start, (size_t)batch * num_planes, s, [&](auto FMT, auto NT) {
    hipLaunchKernelGGL((pp_hres_layers_sparse_kernel<decltype(FMT)::value, decltype(NT)::value>), grid, dim3(256), 0, s, ref_image, src_image,
                       ref_curr_pose, src_curr_pose, intrinsics, depths, blend_weights, alphas, low_height, low_width, height, width, num_planes, sy,
                       sx, gs.start, gs.step, gt.start, gt.step, table, tile_starts(layer_start), pool_out);
  });
}

}  // extern "C"
