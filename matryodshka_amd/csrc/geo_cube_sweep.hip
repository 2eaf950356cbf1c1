// The cube path's source half, sampled from the source PANORAMA (src_sampling='panorama' of MSI.infer_cube / MSI.hres_cube_layers): a plane point of a
// cube face is looked up in the panorama along its own direction (cube_pano_taps, geometry_device.h: the one definition every kernel here calls), so a
// point that projects past a face's border gets the neighbouring face's content instead of the wrap-around texels of its own face.  Each kernel is its
// face-wise twin with that one change:
//   cube_sweep_kernel               pp_sweep_kernel (geo_planar.hip): one source's 3 D channel window of the fp32 volume [6B,S,S,C]
//   cube_sweep_volume_bf16_kernel   pp_sweep_volume_bf16_kernel: the whole bf16 network input, ref half from the ref FACES exactly as there
//   cube_hres_layers_kernel         pp_hres_layers_kernel (geo_planar_hres.hip): the high-res stack in one pass, background taps from the panorama
//   cube_hres_layers_sparse_kernel  pp_hres_layers_sparse_kernel: the same into a sparse pool (table: msi_hres_index_tiles_edge -- alphas do not
//                                   depend on the sweep)
// Each sweep pair is one body (sweep_body, sweep_volume_bf16_body: geometry_device.h) run on two sources; the high-res builders run the PP builders' loops,
// restated, on the cube source.
// Entry n of the [6B,...] batch (blockIdx.z) is face n % 6 of cube n / 6.  Mappings, forms, host conditions and store policies are the twins'; the
// panorama is read through one range-checked descriptor per cube with 32-bit byte offsets (Hp * Wp * 12 < 2^31) in every form.  Kernels first, their
// C ABI entry points below.
#include "geometry_device.h"
#include "geo_sparse.h"

namespace {

// Where the cube sweeps sample their source: the panorama of cube n / 6, along the posed plane point's own direction (cube_pano_taps).  The same in
// both forms of a kernel.
struct CubePanoSource {
  static constexpr bool CAMERA = false;
  __amdgpu_buffer_rsrc_t pano;
  const float *P;                  // the source pose of face n
  int f, pano_h, pano_w;
  // (the face camera Kb is not needed: the direction is looked up along itself)
  template <int FAST> __device__ __forceinline__ void sample(const float *, const Vec3 &a, float *o) const {
    gather3(pano, cube_pano_taps(P, f, a, pano_h, pano_w), o);
  }
};
__device__ __forceinline__ CubePanoSource cube_pano_source(const float *__restrict__ panorama, const float *__restrict__ pose, int n, int pano_h, int pano_w) {
  const int sample = n / 6;
  return CubePanoSource{image_rsrc(panorama, sample, pano_h, pano_w), pose + (size_t)n * 16, n - sample * 6, pano_h, pano_w};
}

// pp_sweep_kernel with the source taken from the panorama (sweep_body, geometry_device.h): the same index math, backproject_planar and apply_pose, then
// CubePanoSource in place of M = K4 @ pose, the two divides and make_taps.  FAST: whole pixels through the wave's LDS strip, 16-byte stores (the host
// decides, as there).  grid = (ceil(S*D / 256), S, 6B).
template <int FAST>
__global__ void __launch_bounds__(256)
cube_sweep_kernel(const float *__restrict__ panorama, const float *__restrict__ pose, const float *__restrict__ intrinsics,
                  const float *__restrict__ depths, int pano_h, int pano_w, int face, int nd, float s0, float sstep, float *__restrict__ psv,
                  int channels, int coff, unsigned nd_magic, int nt) {
  sweep_body<FAST>(cube_pano_source(panorama, pose, blockIdx.z, pano_h, pano_w), intrinsics, depths, face, face, nd, s0, sstep, s0,
                   sstep, psv, channels, coff, nd_magic, nt);
}

// pp_sweep_volume_bf16_kernel with the src half from the panorama (sweep_volume_bf16_body): backproject_planar once per thread for both halves; the ref
// half (image0 = the ref faces, pose0, M = K4 @ pose0, make_taps, 12-byte buffer loads) is that kernel's, op for op, so it has its bits; the src half is
// cube_sweep_kernel's value rounded to nearest even.  FAST, NT and the store: as there.  grid = (ceil(S*D / 256), S, 6B).
template <int FAST, int NT>
__global__ void __launch_bounds__(256)
cube_sweep_volume_bf16_kernel(const float *__restrict__ image0, const float *__restrict__ panorama, const float *__restrict__ pose0,
                              const float *__restrict__ pose1, const float *__restrict__ intrinsics, const float *__restrict__ depths,
                              int pano_h, int pano_w, int face, int nd, int nd_shift, float s0, float sstep, unsigned short *__restrict__ psv) {
  sweep_volume_bf16_body<FAST, NT>(image0, pose0 + (size_t)blockIdx.z * 16, cube_pano_source(panorama, pose1, blockIdx.z, pano_h, pano_w), intrinsics, depths,
                                   face, face, nd, nd_shift, s0, sstep, s0, sstep, psv);
}

// pp_hres_layers_kernel with the cube source (CubeHres, geometry_device.h): grid = (ceil(S / 256), S, 6B), a lane is one pixel and
// walks the layers.  FMT, WITH_F32, NT: as hres_layers_kernel.
template <int FMT, int WITH_F32, int NT>
__global__ void __launch_bounds__(256) __attribute__((amdgpu_waves_per_eu(MSI_HRES_WAVES, MSI_HRES_WAVES)))
cube_hres_layers_kernel(const float *__restrict__ ref_faces, const float *__restrict__ panorama, const float *__restrict__ pose0,
                        const float *__restrict__ pose1, const float *__restrict__ intrinsics, const float *__restrict__ depths,
                        const float *__restrict__ blend_weights, const float *__restrict__ alphas, int pano_h, int pano_w, int low, int face, int nd,
                        float sc, float s0, float sstep, float4 *__restrict__ rgba, void *__restrict__ packed) {
  const int j = blockIdx.x * 256 + threadIdx.x;
  if (j >= face) return;
  const int i = blockIdx.y, b = blockIdx.z;
  const CubeHres px = cube_hres(ref_faces, panorama, pose0, pose1, intrinsics, b, i, j, face, pano_h, pano_w, s0, sstep);
  const HresCorners k = hres_corners(i, j, sc, sc, low, low, nd);
  const size_t low_base = (size_t)b * low * low * nd;          // (h * w * D < 2^31: checked on the host)
  const float *bw = blend_weights + low_base, *al = alphas + low_base;

  const size_t hw = (size_t)face * face;
  size_t texel = (size_t)b * nd * hw + (size_t)i * face + j;      // layer 0 of this pixel in the [B,D,H,W] stack
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

// pp_hres_layers_sparse_kernel with the cube source's steps: a lane of a dropped tile computes no sample position, blends nothing and stores nothing, and
// its eight loads carry NO_TEXEL (past the face AND the panorama, both below 2^31 bytes: zeros, no memory access).
template <int FMT, int NT>
__global__ void __launch_bounds__(256) __attribute__((amdgpu_waves_per_eu(MSI_HRES_WAVES, 8)))
cube_hres_layers_sparse_kernel(const float *__restrict__ ref_faces, const float *__restrict__ panorama, const float *__restrict__ pose0,
                               const float *__restrict__ pose1, const float *__restrict__ intrinsics, const float *__restrict__ depths,
                               const float *__restrict__ blend_weights, const float *__restrict__ alphas, int pano_h, int pano_w, int low, int face,
                               int nd, float sc, float s0, float sstep, const int *__restrict__ table, const long long *__restrict__ layer_start,
                               void *__restrict__ pool) {
  const int j = blockIdx.x * 256 + threadIdx.x;
  if (j >= face) return;
  const int i = blockIdx.y, b = blockIdx.z;
  const CubeHres px = cube_hres(ref_faces, panorama, pose0, pose1, intrinsics, b, i, j, face, pano_h, pano_w, s0, sstep);
  const HresCorners k = hres_corners(i, j, sc, sc, low, low, nd);
  const size_t low_base = (size_t)b * low * low * nd;
  const float *bw = blend_weights + low_base, *al = alphas + low_base;

  const int tx_n = face / TILE_W;
  const size_t per_layer = (size_t)tx_n * (face / TILE_H);
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

// what every entry point here asks of the cubes and the panorama, in ONE order, after its own null-pointer check; *faces = 6 * batch
int cube_sweep_check(const char *who, int32_t batch, int32_t pano_height, int32_t pano_width, int32_t face_size, int32_t *faces) {
  MSI_REQUIRE(batch >= 0 && face_size > 1, "%s: bad dims (batch >= 0, faces of at least 2 x 2)", who);
  MSI_REQUIRE(pano_height >= 2 && pano_width >= 2, "%s: bad dims (a panorama of at least 2 x 2, got %d x %d)", who, pano_height, pano_width);
  MSI_REQUIRE((long)pano_height * pano_width * 12 < 2147483647L, "%s: panorama too large (Hp * Wp * 12 < 2^31)", who);
  MSI_REQUIRE(6L * batch <= 65535 && face_size <= 65535, "%s: problem too large (6 * batch and face_size at most 65535)", who);
  MSI_REQUIRE((long)face_size * face_size * 12 < 2147483647L, "%s: problem too large (S * S * 12 < 2^31)", who);
  *faces = 6 * batch;
  return MSI_OK;
}

}  // namespace

extern "C" {

int msi_cube_plane_sweep_f32(const float *panorama, const float *face_pose, const float *intrinsics, const float *depths, int32_t batch,
                             int32_t pano_height, int32_t pano_width, int32_t face_size, int32_t num_depths, float *psv, int32_t psv_channels,
                             int32_t channel_offset, msi_stream_t stream) {
  const char *who = "cube_plane_sweep";
  MSI_REQUIRE(panorama && face_pose && intrinsics && depths && psv, "%s: null pointer", who);
  MSI_REQUIRE(num_depths > 0, "%s: bad dims (num_depths must be positive)", who);
  int32_t faces;
  if (const int e = cube_sweep_check(who, batch, pano_height, pano_width, face_size, &faces)) return e;
  MSI_REQUIRE(channel_offset >= 0 && (long)channel_offset + 3L * num_depths <= psv_channels, "%s: channel window outside %d channels", who, psv_channels);
  MSI_REQUIRE((long)face_size * num_depths < 2147483647L, "%s: problem too large", who);
  if (batch == 0) return MSI_OK;
  const dim3 grid((unsigned)(((long)face_size * num_depths + 255) / 256), face_size, faces);
  const UvGrid g = uv_grid(face_size);
  const unsigned magic = udiv_magic32(num_depths);
  const int nt = beyond_infinity_cache((size_t)faces * face_size * face_size * psv_channels * 4) ? 1 : 0;
  // msi_perspective_plane_sweep_f32's condition: full waves of complete pixels whose 3 D-float runs are 16-byte aligned
  const bool fast = 64 % num_depths == 0 && ((long)face_size * num_depths) % 256 == 0 && (3 * num_depths) % 4 == 0 && psv_channels % 4 == 0 &&
                    channel_offset % 4 == 0 && num_depths >= 4;
  hipStream_t s = msi::as_stream(stream);
  if (fast)
    hipLaunchKernelGGL(cube_sweep_kernel<1>, grid, dim3(256), 0, s, panorama, face_pose, intrinsics, depths, pano_height, pano_width, face_size,
                       num_depths, g.start, g.step, psv, psv_channels, channel_offset, magic, nt);
  else
    hipLaunchKernelGGL(cube_sweep_kernel<0>, grid, dim3(256), 0, s, panorama, face_pose, intrinsics, depths, pano_height, pano_width, face_size,
                       num_depths, g.start, g.step, psv, psv_channels, channel_offset, magic, nt);
  return msi::check_launch(who);
}

int msi_cube_sweep_volume_bf16(const float *ref_faces, const float *src_panorama, const float *ref_face_pose, const float *src_face_pose,
                               const float *intrinsics, const float *depths, int32_t batch, int32_t pano_height, int32_t pano_width,
                               int32_t face_size, int32_t num_depths, void *psv_bf16, msi_stream_t stream) {
  const char *who = "cube_sweep_volume_bf16";
  MSI_REQUIRE(ref_faces && src_panorama && ref_face_pose && src_face_pose && intrinsics && depths && psv_bf16, "%s: null pointer", who);
  MSI_REQUIRE(num_depths > 0, "%s: bad dims (num_depths must be positive)", who);
  int32_t faces;
  if (const int e = cube_sweep_check(who, batch, pano_height, pano_width, face_size, &faces)) return e;
  MSI_REQUIRE((long)face_size * num_depths < 2147483647L, "%s: problem too large", who);
  if (batch == 0) return MSI_OK;
  const dim3 grid((unsigned)(((long)face_size * num_depths + 255) / 256), face_size, faces);
  const UvGrid g = uv_grid(face_size);
  const int nt = beyond_infinity_cache((size_t)faces * face_size * face_size * 6 * num_depths * 2) ? 1 : 0;
  int shift = 0;
  while ((1 << shift) < num_depths) ++shift;
  // msi_perspective_sweep_volume_bf16's condition: whole waves of complete pixels (D a power of two up to 64), 16-byte-aligned volume
  const bool fast = 64 % num_depths == 0 && ((long)face_size * num_depths) % 64 == 0 && reinterpret_cast<uintptr_t>(psv_bf16) % 16 == 0;
  unsigned short *psv = static_cast<unsigned short *>(psv_bf16);
#define MSI_LAUNCH_CSV(FAST_, NT_)                                                                                                          \
  hipLaunchKernelGGL((cube_sweep_volume_bf16_kernel<FAST_, NT_>), grid, dim3(256), 0, msi::as_stream(stream), ref_faces, src_panorama,     \
                     ref_face_pose, src_face_pose, intrinsics, depths, pano_height, pano_width, face_size, num_depths, shift, g.start, g.step, psv)
  if (fast && nt)
    MSI_LAUNCH_CSV(1, 1);
  else if (fast)
    MSI_LAUNCH_CSV(1, 0);
  else
    MSI_LAUNCH_CSV(0, 0);
#undef MSI_LAUNCH_CSV
  return msi::check_launch(who);
}

int msi_cube_hres_layers(const float *ref_faces, const float *src_panorama, const float *ref_face_pose, const float *src_face_pose,
                         const float *intrinsics, const float *depths, const float *blend_weights, const float *alphas, int32_t batch,
                         int32_t pano_height, int32_t pano_width, int32_t low_size, int32_t face_size, int32_t num_planes, float *rgba_native,
                         void *layers_out, int32_t format, msi_stream_t stream) {
  const char *who = "cube_hres_layers";
  MSI_REQUIRE(!layers_out || format == MSI_LAYERS_RGBA8 || format == MSI_LAYERS_RGBA16F, "%s: unknown format %d", who, format);
  MSI_REQUIRE(rgba_native || layers_out, "%s: null pointer (both outputs are NULL)", who);
  MSI_REQUIRE(ref_faces && src_panorama && ref_face_pose && src_face_pose && intrinsics && depths && blend_weights && alphas, "%s: null pointer", who);
  int32_t faces;
  if (const int e = cube_sweep_check(who, batch, pano_height, pano_width, face_size, &faces)) return e;
  if (const int e = hres_check(who, true, faces, low_size, low_size, face_size, face_size, num_planes)) return e;
  if (batch == 0) return MSI_OK;
  const float sc = hres_scale(low_size, face_size);
  const UvGrid g = uv_grid(face_size);
  const dim3 grid((unsigned)((face_size + 255) / 256), face_size, faces);
  hipStream_t s = msi::as_stream(stream);
  hres_dense_launch(format, rgba_native, layers_out, (size_t)faces * num_planes * face_size * face_size, [&](auto FMT, auto F32, auto NT) {
    hipLaunchKernelGGL((cube_hres_layers_kernel<decltype(FMT)::value, decltype(F32)::value, decltype(NT)::value>), grid, dim3(256), 0, s, ref_faces,
                       src_panorama, ref_face_pose, src_face_pose, intrinsics, depths, blend_weights, alphas, pano_height, pano_width, low_size,
                       face_size, num_planes, sc, g.start, g.step, reinterpret_cast<float4 *>(rgba_native), layers_out);
  });
  return msi::check_launch(who);
}

int msi_cube_hres_layers_sparse(const float *ref_faces, const float *src_panorama, const float *ref_face_pose, const float *src_face_pose,
                                const float *intrinsics, const float *depths, const float *blend_weights, const float *alphas, int32_t batch,
                                int32_t pano_height, int32_t pano_width, int32_t low_size, int32_t face_size, int32_t num_planes,
                                const int32_t *table, const int64_t *layer_start, void *pool_out, int32_t format, msi_stream_t stream) {
  const char *who = "cube_hres_layers_sparse";
  MSI_REQUIRE(ref_faces && src_panorama && ref_face_pose && src_face_pose && intrinsics && depths && blend_weights && alphas && table && layer_start &&
              pool_out, "%s: null pointer", who);
  int32_t faces;
  if (const int e = cube_sweep_check(who, batch, pano_height, pano_width, face_size, &faces)) return e;
  if (const int e = hres_check(who, true, faces, low_size, low_size, face_size, face_size, num_planes)) return e;
  size_t tiles;
  if (const int e = sparse_dims(who, format, faces, num_planes, face_size, face_size, &tiles)) return e;
  if (batch == 0) return MSI_OK;
  const float sc = hres_scale(low_size, face_size);
  const UvGrid g = uv_grid(face_size);
  const dim3 grid((unsigned)((face_size + 255) / 256), face_size, faces);
  hipStream_t s = msi::as_stream(stream);
  return hres_sparse_launch(who, format, tiles, layer_start, (size_t)faces * num_planes, s, [&](auto FMT, auto NT) {
    hipLaunchKernelGGL((cube_hres_layers_sparse_kernel<decltype(FMT)::value, decltype(NT)::value>), grid, dim3(256), 0, s, ref_faces, src_panorama,
                       ref_face_pose, src_face_pose, intrinsics, depths, blend_weights, alphas, pano_height, pano_width, low_size, face_size,
                       num_planes, sc, g.start, g.step, table, tile_starts(layer_start), pool_out);
  });
}

}  // extern "C"
