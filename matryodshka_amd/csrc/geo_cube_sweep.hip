// The cube path's source half, sampled from the source PANORAMA (src_sampling='panorama' of MSI.infer_cube / MSI.hres_cube_layers): a plane point of a
// cube face is looked up in the panorama along its own direction (cube_pano_taps, geometry_device.h: the one definition every kernel here calls), so a
// point that projects past a face's border gets the neighbouring face's content instead of the wrap-around texels of its own face.  Each kernel is its
// face-wise twin with that one change:
//   cube_sweep_kernel               pp_sweep_kernel (geo_planar.hip): one source's 3 D channel window of the fp32 volume [6B,S,S,C]
//   cube_sweep_volume_bf16_kernel   pp_sweep_volume_bf16_kernel: the whole bf16 network input, ref half from the ref FACES exactly as there
//   cube_hres_layers_kernel         pp_hres_layers_kernel (geo_planar_hres.hip): the high-res stack in one pass, background taps from the panorama
//   cube_hres_layers_sparse_kernel  pp_hres_layers_sparse_kernel: the same into a sparse pool (table: msi_hres_index_tiles_edge -- alphas do not
//                                   depend on the sweep)
// Entry n of the [6B,...] batch (blockIdx.z) is face n % 6 of cube n / 6.  Mappings, forms, host conditions and store policies are the twins'; the
// panorama is read through one range-checked descriptor per cube with 32-bit byte offsets (Hp * Wp * 12 < 2^31) in every form.  Kernels first, their
// C ABI entry points below.
#include "geometry_device.h"
#include "geo_sparse.h"

namespace {

// pp_sweep_kernel with the source taken from the panorama: the same index math, backproject_planar and apply_pose, then cube_pano_taps in place of
// M = K4 @ pose, the two divides and make_taps.  FAST: whole pixels through the wave's LDS strip, 16-byte stores (the host decides, as there).
template <int FAST>
__global__ void __launch_bounds__(256)
cube_sweep_kernel(const float *__restrict__ panorama, const float *__restrict__ pose, const float *__restrict__ intrinsics,
                  const float *__restrict__ depths, int pano_h, int pano_w, int face, int nd, float s0, float sstep, float *__restrict__ psv,
                  int channels, int coff, unsigned nd_magic, int nt) {
  // grid = (ceil(S*D / 256), S, 6B): 32-bit index math only
  const int idx = blockIdx.x * 256 + threadIdx.x;
  if (!FAST && idx >= face * nd) return;
  int j, d;
  if (FAST) {
    unsigned jq = __umulhi((unsigned)idx, nd_magic);   // idx / nd by multiply-high (+ one correction)
    if ((unsigned)idx - jq * (unsigned)nd >= (unsigned)nd) ++jq;
    j = (int)jq; d = idx - j * nd;
  } else {
    j = idx / nd; d = idx - j * nd;
  }
  const int i = blockIdx.y, n = blockIdx.z;
  const int sample = n / 6, f = n - sample * 6;
  const float S = s0 + sstep * (float)j, T = s0 + sstep * (float)i;
  const float depth = depths[d];
  const float *Kb = intrinsics + (size_t)n * 9;
  const float fx = Kb[0], fy = Kb[4], cx = Kb[2], cy = Kb[5];
  // backproject_planar (spherical.py:146-148): x = depth*S*cx/fx, y = depth*T*cy/fy, z = depth*1
  const float x = ((depth * S) * cx) / fx;
  const float y = ((depth * T) * cy) / fy;
  const float z = depth * 1.0f;
  const float *P = pose + (size_t)n * 16;
  // apply_pose (projector.py:275-291)
  const float ax = ((P[0] * x + P[1] * y) + P[2] * z) + P[3] * 1.0f;
  const float ay = ((P[4] * x + P[5] * y) + P[6] * z) + P[7] * 1.0f;
  const float az = ((P[8] * x + P[9] * y) + P[10] * z) + P[11] * 1.0f;
  const TapsB t = cube_pano_taps(P, f, ax, ay, az, pano_h, pano_w);
  float o[3];
  gather3(cube_pano_rsrc(panorama, sample, pano_h, pano_w), t, o);
  if (FAST) {
    // whole-pixel runs through the wave's strip: lane = (pixel of the wave, depth); the wave's 64 / D pixels are consecutive, each owns 3 D contiguous floats at + coff
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
      const long pw0 = ((long)n * face + i) * face + (long)((blockIdx.x * 256 + wave * 64) / nd);
      uint4 *dst = reinterpret_cast<uint4 *>(psv + (size_t)(pw0 + pl) * channels + coff) + k;
      sweep_store16(dst, reinterpret_cast<const uint4 *>(w)[lane], nt);
    }
    return;
  }
  const long p = ((long)n * face + i) * face + j;
  float *dst = psv + (size_t)p * channels + coff + d * 3;
  dst[0] = o[0]; dst[1] = o[1]; dst[2] = o[2];
}

// pp_sweep_volume_bf16_kernel with the src half from the panorama: backproject_planar once per thread for both halves; the ref half (image0 = the ref
// faces, pose0, M = K4 @ pose0, make_taps, 12-byte buffer loads) is that kernel's, op for op, so it has its bits; the src half is cube_sweep_kernel's
// value rounded to nearest even.  FAST, NT and the store: as there.
template <int FAST, int NT>
__global__ void __launch_bounds__(256)
cube_sweep_volume_bf16_kernel(const float *__restrict__ image0, const float *__restrict__ panorama, const float *__restrict__ pose0,
                              const float *__restrict__ pose1, const float *__restrict__ intrinsics, const float *__restrict__ depths,
                              int pano_h, int pano_w, int face, int nd, int nd_shift, float s0, float sstep, unsigned short *__restrict__ psv) {
  // grid = (ceil(S*D / 256), S, 6B): 32-bit index math only
  const int idx = blockIdx.x * 256 + threadIdx.x;
  const int i = blockIdx.y, n = blockIdx.z;
  const int sample = n / 6, f = n - sample * 6;
  const float *Kb = intrinsics + (size_t)n * 9;
  const float fx = Kb[0], fy = Kb[4], cx = Kb[2], cy = Kb[5];
  const float T = s0 + sstep * (float)i;
  const float *P0 = pose0 + (size_t)n * 16, *P1 = pose1 + (size_t)n * 16;
  __shared__ float s_m[12];
  __shared__ float s_y[64];
  if (FAST) {
    // project_perspective's M = K4 @ pose of the ref half, and backproject_planar's y = depth*T*cy/fy per plane of this row
    const int tid = threadIdx.x;
    if (tid < 12) {
      const int r = tid >> 2, c = tid & 3;
      s_m[tid] = ((Kb[r * 3 + 0] * P0[c] + Kb[r * 3 + 1] * P0[4 + c]) + Kb[r * 3 + 2] * P0[8 + c]) + 0.0f * P0[12 + c];
    } else if (tid >= 64 && tid < 64 + nd) {
      s_y[tid - 64] = ((depths[tid - 64] * T) * cy) / fy;
    }
    __syncthreads();
    if (idx >= face * nd) return;   // (S * D) % 64 == 0: whole waves
  } else {
    if (idx >= face * nd) return;
  }
  const int j = FAST ? idx >> nd_shift : idx / nd;
  const int d = FAST ? idx & (nd - 1) : idx - j * nd;
  const float S = s0 + sstep * (float)j;
  const float depth = depths[d];
  // backproject_planar (spherical.py:146-148), shared by both halves
  const float x0 = ((depth * S) * cx) / fx;
  const float y0 = FAST ? s_y[d] : ((depth * T) * cy) / fy;
  const float z0 = depth * 1.0f;
  float out[2][3];
  {  // ref half: the ref face through its own camera (pp_sweep_volume_bf16_kernel, s = 0)
    const float x = ((P0[0] * x0 + P0[1] * y0) + P0[2] * z0) + P0[3] * 1.0f;
    const float y = ((P0[4] * x0 + P0[5] * y0) + P0[6] * z0) + P0[7] * 1.0f;
    const float z = ((P0[8] * x0 + P0[9] * y0) + P0[10] * z0) + P0[11] * 1.0f;
    float pr[3];
    if (FAST) {
#pragma unroll
      for (int r = 0; r < 3; ++r) pr[r] = ((s_m[r * 4 + 0] * x + s_m[r * 4 + 1] * y) + s_m[r * 4 + 2] * z) + s_m[r * 4 + 3] * 1.0f;
    } else {
#pragma unroll
      for (int r = 0; r < 3; ++r) {
        float m[4];
#pragma unroll
        for (int c = 0; c < 4; ++c)
          m[c] = ((Kb[r * 3 + 0] * P0[c] + Kb[r * 3 + 1] * P0[4 + c]) + Kb[r * 3 + 2] * P0[8 + c]) + 0.0f * P0[12 + c];
        pr[r] = ((m[0] * x + m[1] * y) + m[2] * z) + m[3] * 1.0f;
      }
    }
    const float u = pr[0] / pr[2], v = pr[1] / pr[2];
    const Taps t = make_taps(u, v, face, face);
    const __amdgpu_buffer_rsrc_t img = __builtin_amdgcn_make_buffer_rsrc((void *)(image0 + (size_t)n * face * face * 3), 0, face * face * 12, 0x00020000);
    const f32x3_g a = __builtin_bit_cast(f32x3_g, (u32x3_g)__builtin_amdgcn_raw_buffer_load_b96(img, (unsigned)(t.y0 * face + t.x0) * 12u, 0, 0));
    const f32x3_g bq = __builtin_bit_cast(f32x3_g, (u32x3_g)__builtin_amdgcn_raw_buffer_load_b96(img, (unsigned)(t.y0 * face + t.x1) * 12u, 0, 0));
    const f32x3_g c = __builtin_bit_cast(f32x3_g, (u32x3_g)__builtin_amdgcn_raw_buffer_load_b96(img, (unsigned)(t.y1 * face + t.x0) * 12u, 0, 0));
    const f32x3_g dq = __builtin_bit_cast(f32x3_g, (u32x3_g)__builtin_amdgcn_raw_buffer_load_b96(img, (unsigned)(t.y1 * face + t.x1) * 12u, 0, 0));
    out[0][0] = blend4(t, a.x, bq.x, c.x, dq.x);
    out[0][1] = blend4(t, a.y, bq.y, c.y, dq.y);
    out[0][2] = blend4(t, a.z, bq.z, c.z, dq.z);
  }
  {  // src half: the panorama along the plane point's own direction (cube_sweep_kernel)
    const float ax = ((P1[0] * x0 + P1[1] * y0) + P1[2] * z0) + P1[3] * 1.0f;
    const float ay = ((P1[4] * x0 + P1[5] * y0) + P1[6] * z0) + P1[7] * 1.0f;
    const float az = ((P1[8] * x0 + P1[9] * y0) + P1[10] * z0) + P1[11] * 1.0f;
    const TapsB t = cube_pano_taps(P1, f, ax, ay, az, pano_h, pano_w);
    gather3(cube_pano_rsrc(panorama, sample, pano_h, pano_w), t, out[1]);
  }
  const long p = ((long)n * face + i) * face + j;
  if (FAST) {
    // the wave's 64 / D pixels are consecutive and each owns 6 D contiguous channels: lane = pl * D + d writes its two triples into the
    // strip at pl * 6 D + {0, 3 D} + 3 d, then lanes 0..47 each pack 8 of the 384 values into one 16-byte store
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

// pp_hres_layers_kernel with the cube texel (cube_hres_pixel / cube_hres_texel, geometry_device.h): grid = (ceil(S / 256), S, 6B), a lane is one pixel and
// walks the layers.  FMT, WITH_F32, NT: as hres_layers_kernel.
template <int FMT, int WITH_F32, int NT>
__global__ void __launch_bounds__(256) __attribute__((amdgpu_waves_per_eu(MSI_HRES_WAVES, MSI_HRES_WAVES)))
cube_hres_layers_kernel(const float *__restrict__ ref_faces, const float *__restrict__ panorama, const float *__restrict__ pose0,
                        const float *__restrict__ pose1, const float *__restrict__ intrinsics, const float *__restrict__ depths,
                        const float *__restrict__ blend_weights, const float *__restrict__ alphas, int pano_h, int pano_w, int low, int face, int nd,
                        float sc, float s0, float sstep, float4 *__restrict__ rgba, void *__restrict__ packed) {
  const int j = blockIdx.x * 256 + threadIdx.x;
  if (j >= face) return;
  const int i = blockIdx.y, n = blockIdx.z;

  const CubeHresPixel px = cube_hres_pixel(ref_faces, panorama, pose0, pose1, intrinsics, n, i, j, face, face, pano_h, pano_w, s0, sstep, s0, sstep);
  const HresCorners k = hres_corners(i, j, sc, sc, low, low, nd);
  const size_t low_base = (size_t)n * low * low * nd;             // (s * s * D < 2^31: checked on the host)
  const float *bw = blend_weights + low_base, *al = alphas + low_base;

  const size_t hw = (size_t)face * face;
  size_t texel = (size_t)n * nd * hw + (size_t)i * face + j;       // layer 0 of this pixel in the [6B,D,S,S] stack
  for (int d0 = 0; d0 < nd; d0 += HRES_G) {                        // (nd % 4 == 0: checked on the host)
    const hres_vec wv = hres_lerp(bw + d0, k);
    const hres_vec av = hres_lerp(al + d0, k);
#pragma unroll
    for (int q = 0; q < HRES_G; ++q) {
      const float4 o = cube_hres_texel(px, depths[d0 + q], face, face, wv[q], av[q]);
      if (WITH_F32) sweep_store16(reinterpret_cast<uint4 *>(rgba + texel), __builtin_bit_cast(uint4, o), NT & 1);
      if constexpr (FMT != MSI_LAYERS_F32) hres_store_packed<FMT, (NT >> 1) & 1>(packed, texel, o);
      texel += hw;
    }
  }
}

// pp_hres_layers_sparse_kernel with the cube texel's steps: a lane of a dropped tile computes no sample position, blends nothing and stores nothing, and
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
  const int i = blockIdx.y, n = blockIdx.z;
  const CubeHresPixel px = cube_hres_pixel(ref_faces, panorama, pose0, pose1, intrinsics, n, i, j, face, face, pano_h, pano_w, s0, sstep, s0, sstep);
  const HresCorners k = hres_corners(i, j, sc, sc, low, low, nd);
  const size_t low_base = (size_t)n * low * low * nd;
  const float *bw = blend_weights + low_base, *al = alphas + low_base;

  const int tx_n = face / TILE_W;
  const size_t per_layer = (size_t)tx_n * (face / TILE_H);
  const size_t layer0 = (size_t)n * nd;
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
      if (idx[q] >= 0) tp[q] = cube_hres_taps(px, depths[d0 + q], face, face);
      rgb[q] = cube_hres_fetch(px, tp[q]);
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
  const int fmt = layers_out ? format : MSI_LAYERS_F32;
  // non-temporal stores for a destination that cannot stay in the Infinity Cache (as msi_hres_layers)
  const size_t texels = (size_t)faces * num_planes * face_size * face_size;
  const int nt = (rgba_native && beyond_infinity_cache(texels * 16) ? 1 : 0) |
                 (layers_out && beyond_infinity_cache(texels << (fmt == MSI_LAYERS_RGBA8 ? 2 : 3)) ? 2 : 0);
  const dim3 grid((unsigned)((face_size + 255) / 256), face_size, faces);
  hipStream_t s = msi::as_stream(stream);
  const auto launch = [&](auto FMT, auto F32, auto NT) {
    hipLaunchKernelGGL((cube_hres_layers_kernel<decltype(FMT)::value, decltype(F32)::value, decltype(NT)::value>), grid, dim3(256), 0, s, ref_faces,
                       src_panorama, ref_face_pose, src_face_pose, intrinsics, depths, blend_weights, alphas, pano_height, pano_width, low_size,
                       face_size, num_planes, sc, g.start, g.step, reinterpret_cast<float4 *>(rgba_native), layers_out);
  };
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
  hipStream_t s = msi::as_stream(stream);
  // the store policy needs the pool's bytes, and only layer_start knows them (as msi_pp_hres_layers_sparse)
  const int shift = format == MSI_LAYERS_RGBA8 ? StackTexel<MSI_LAYERS_RGBA8>::shift : StackTexel<MSI_LAYERS_RGBA16F>::shift;
  long long kept = (long long)tiles;
  if (beyond_infinity_cache((tiles * TILE_TEXELS) << shift)) {
    hipError_t e = hipMemcpyAsync(&kept, layer_start + (size_t)faces * num_planes, sizeof kept, hipMemcpyDeviceToHost, s);
    if (e == hipSuccess) e = hipStreamSynchronize(s);
    if (e != hipSuccess) return msi::fail(MSI_E_LAUNCH, "%s: %s", who, hipGetErrorString(e));
    MSI_REQUIRE(kept >= 0 && (size_t)kept <= tiles, "%s: layer_start ends at %lld tiles of %zu", who, kept, tiles);
    if (kept == 0) return MSI_OK;
  }
  const float sc = hres_scale(low_size, face_size);
  const UvGrid g = uv_grid(face_size);
  const dim3 grid((unsigned)((face_size + 255) / 256), face_size, faces);
  for_format(format, [&](auto FMT) {
    constexpr int fmt = decltype(FMT)::value;
    if constexpr (fmt != MSI_LAYERS_F32) {
      auto launch = [&](auto NT) {
        hipLaunchKernelGGL((cube_hres_layers_sparse_kernel<fmt, decltype(NT)::value>), grid, dim3(256), 0, s, ref_faces, src_panorama, ref_face_pose,
                           src_face_pose, intrinsics, depths, blend_weights, alphas, pano_height, pano_width, low_size, face_size, num_planes, sc,
                           g.start, g.step, table, tile_starts(layer_start), pool_out);
      };
      if (beyond_infinity_cache(((size_t)kept * TILE_TEXELS) << StackTexel<fmt>::shift)) launch(Const<1>{});
      else launch(Const<0>{});
    }
  });
  return msi::check_launch(who);
}

}  // extern "C"
