// The planar (PP) path of the geometry side: pp_sweep_kernel, pp_sweep_volume_bf16_kernel, mpi_render_kernel and mpi_render_views_kernel (many
// views of one MPI per launch, from an fp32 or a packed stack); kernels first, their C ABI entry points below.
#include "geometry_device.h"

namespace {

// ------------------------------------------------------------------------ PP path (config 5)
// pj.perspective_plane_sweep (projector.py:221-223) = sweep_one with spherical.uv_grid (:46-48),
// backproject_planar (:131-149), apply_pose, project_perspective (:248-266) and the SAME
// wrap-around sampler as the ODS sweep.  Faithful to the reference, the pose is applied twice:
// once by apply_pose (projector.py:155) and once inside project_perspective through
// intrinsics @ pose (spherical.py:258-259); the 3x3 intrinsics are zero-padded to 4x4
// (projector.py:145-148), so only rows 0..2 of the product are used.
// FAST (round 6): the form for full waves of complete pixels (64 % D == 0, (W * D) % 256 == 0, 16-byte-aligned runs; the host decides).  Same arithmetic, same bits;
// what changes is the plumbing the ODS sweep went through in rounds 1-2: (a) M = K4 @ pose -- 60 multiply-adds that depend on the FACE only -- is computed by twelve
// threads and broadcast through LDS instead of by every thread; (b) a corner is ONE 12-byte buffer load, not three dword loads behind 64-bit address arithmetic;
// (c) a wave's 64 / D complete pixels leave through a wave-private LDS strip as 16-byte-per-lane stores of whole 3 D-float runs instead of 3 dword stores at a
// 12-byte stride per lane; non-temporal when the volume exceeds the Infinity Cache (sweep_store16).  Measured at configs[4] (64 faces, two sweeps each): DESIGN.md section 4.
// The arithmetic is geometry_device.h's (the steps of the planar sweep, sweep_body); here is where pp_sweep_kernel samples: image b through its own camera.
struct PpSweepSource {
  const float *image, *P;          // the [B,H,W,3] batch; the pose [4,4] of sample b
  int b, height, width;
  template <int FAST> __device__ __forceinline__ void sample(const float *Kb, const Vec3 &a, float *o) const {
    if (FAST) {
      __shared__ float s_m[12];
      if (threadIdx.x < 12) s_m[threadIdx.x] = k4_pose(Kb, P, threadIdx.x >> 2, threadIdx.x & 3);
      __syncthreads();
      wrap_gather3(image_rsrc(image, b, height, width), project_rows(s_m, a), width, height, o);
      return;
    }
    const Uv p = project_k4_pose(Kb, P, a);
    const Taps t = make_taps(p.u, p.v, width, height);
    const float *img = image + (size_t)b * height * width * 3;
    const float *pa = img + ((size_t)t.y0 * width + t.x0) * 3;
    const float *pb = img + ((size_t)t.y0 * width + t.x1) * 3;
    const float *pc = img + ((size_t)t.y1 * width + t.x0) * 3;
    const float *pd = img + ((size_t)t.y1 * width + t.x1) * 3;
    o[0] = blend4(t, pa[0], pb[0], pc[0], pd[0]);
    o[1] = blend4(t, pa[1], pb[1], pc[1], pd[1]);
    o[2] = blend4(t, pa[2], pb[2], pc[2], pd[2]);
  }
};

template <int FAST>
__global__ void __launch_bounds__(256)
pp_sweep_kernel(const float *__restrict__ image, const float *__restrict__ pose,
                const float *__restrict__ intrinsics, const float *__restrict__ depths, int batch,
                int height, int width, int nd, float s0, float sstep, float t0, float tstep,
                float *__restrict__ psv, int channels, int coff, unsigned nd_magic, int nt) {
  // grid = (ceil(W*D / 256), H, B)
  const int b = blockIdx.z;
  sweep_body<FAST>(PpSweepSource{image, pose + (size_t)b * 16, b, height, width}, intrinsics, depths, height, width, nd, s0, sstep, t0, tstep, psv, channels,
                   coff, nd_magic, nt);
}

// The whole bf16 PP network input of format_network_input (msi.py:1157-1161) in one launch: ref into channels [0, 3D), src into [3D, 6D)
// of psv [B,H,W,6D].  Every value is the round-to-nearest-even of what pp_sweep_kernel computes for the same sample, bit for bit: the
// arithmetic below is pp_sweep_kernel's, op for op.  What changes is what is shared: backproject_planar's (x, y, z) depend on the face's
// intrinsics, the plane and the pixel, not on the pose, so one thread per (pixel, plane) computes them once for both sources (5 IEEE
// divides per thread instead of 10 over two launches), and y -- a function of (row, plane) -- once per block into LDS; M = K4 @ pose is
// computed once per face and source (24 threads, LDS).
// FAST (64 % D == 0, (W * D) % 64 == 0; the host decides): a wave holds 64 / D complete pixels, whose 6 D channels are one contiguous run,
// so the wave's 768 bytes leave through a wave-private fp32 strip as 48 16-byte stores of packed pairs (v_cvt_pk_bf16_f32: round to nearest
// even, what f32_to_bf16 computes for the finite values stored here); non-temporal when the volume exceeds the Infinity Cache (sweep_store16).
// Generic: one thread per (pixel, plane) stores its six values as bf16 halves.  Corners are 12-byte buffer loads with 32-bit offsets
// (H * W * 12 < 2^31, checked on the host) in both forms; make_taps' wrapped indices lie inside the image.  The kernel is VALU-bound
// (DESIGN.md section 4).  NT is a template argument, not sweep_store16's runtime flag: with the packed value computed ahead of the
// branch, hipcc merges the two stores into one plain store.
// (the src half of sweep_volume_bf16_body: a second image of the ref half's camera)
struct PpSecondImage {
  static constexpr bool CAMERA = true;
  const float *image, *P;          // the [B,H,W,3] batch; the pose of sample b
};

template <int FAST, int NT>
__global__ void __launch_bounds__(256)
pp_sweep_volume_bf16_kernel(const float *__restrict__ image0, const float *__restrict__ image1, const float *__restrict__ pose0,
                            const float *__restrict__ pose1, const float *__restrict__ intrinsics, const float *__restrict__ depths,
                            int height, int width, int nd, int nd_shift, float s0, float sstep, float t0, float tstep,
                            unsigned short *__restrict__ psv) {
  // grid = (ceil(W*D / 256), H, B)
  sweep_volume_bf16_body<FAST, NT>(image0, pose0 + (size_t)blockIdx.z * 16, PpSecondImage{image1, pose1 + (size_t)blockIdx.z * 16}, intrinsics, depths,
                                   height, width, nd, nd_shift, s0, sstep, t0, tstep, psv);
}

// MSI.mpi_render_view (msi.py:527-548): pj.projective_forward_homography (projector.py:343-373) ->
// homography.planar_transform (homography.py:120-157: inv_homography :35-58, transform_points
// :60-80, normalize_homogeneous :82-94, divide_safe :30-33) -> sampling.bilinear_wrapper =
// tf.contrib.resampler (zero padding) -> pj.over_composite, fused.  The per-(layer, sample)
// inverse homographies (a few dozen flops each) are computed once per workgroup into LDS.
constexpr int MPI_MAX_PLANES = 128;

__device__ __forceinline__ float4 fetch_or_zero(const float4 *L, int x, int y, int width, int height) {
  if (x >= 0 && y >= 0 && x < width && y < height) return L[(size_t)y * width + x];
  return make_float4(0.f, 0.f, 0.f, 0.f);
}

__global__ void __launch_bounds__(256)
mpi_render_kernel(const float4 *__restrict__ rgba, const float *__restrict__ tgt_pose,
                  const float *__restrict__ intrinsics, const float *__restrict__ intrinsics_inv,
                  const float *__restrict__ depths, int batch, int height, int width, int nd,
                  float *__restrict__ out_rgb) {
  __shared__ float hom[MPI_MAX_PLANES][9];
  const int b = blockIdx.z;
  const int tid = threadIdx.y * 64 + threadIdx.x;
  if (tid < nd) {
    const float *P = tgt_pose + (size_t)b * 16;
    const float *Ks = intrinsics + (size_t)b * 9, *Ki = intrinsics_inv + (size_t)b * 9;
    float rt[3][3], t[3];
#pragma unroll
    for (int r = 0; r < 3; ++r) {
#pragma unroll
      for (int c = 0; c < 3; ++c) rt[r][c] = P[c * 4 + r];  // rot_t = transpose(pose[:3,:3])
      t[r] = P[r * 4 + 3];
    }
    const float a = -depths[tid];
    // n_hat = [0,0,1]: n_hat @ rot_t = row 2 of rot_t
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
        hom[tid][r * 3 + c] = (m2[r][0] * Ki[0 * 3 + c] + m2[r][1] * Ki[1 * 3 + c]) + m2[r][2] * Ki[2 * 3 + c];
  }
  __syncthreads();
  const int j = blockIdx.x * 64 + threadIdx.x;
  const int i = blockIdx.y * 4 + threadIdx.y;
  if (j >= width || i >= height) return;
  const float uu = (float)j, vv = (float)i;  // meshgrid_abs (projector.py:478-499)
  const size_t hw = (size_t)height * width;
  float o0 = 0.f, o1 = 0.f, o2 = 0.f;
  for (int d = 0; d < nd; ++d) {
    const float *h = hom[d];
    const float xs = (uu * h[0] + vv * h[1]) + 1.0f * h[2];
    const float ys = (uu * h[3] + vv * h[4]) + 1.0f * h[5];
    float ws = (uu * h[6] + vv * h[7]) + 1.0f * h[8];
    ws += 1e-8f * (ws == 0.0f ? 1.0f : 0.0f);
    const float x = xs / ws, y = ys / ws;
    float4 v = make_float4(0.f, 0.f, 0.f, 0.f);
    // tf.contrib.resampler [TF-knowledge]: zero outside (-1, W) x (-1, H); missing corners are 0
    if (x > -1.0f && y > -1.0f && x < (float)width && y < (float)height) {
      const float fxf = floorf(x), fyf = floorf(y);
      const int fx = (int)fxf, fy = (int)fyf, cx = fx + 1, cy = fy + 1;
      const float dx = (float)cx - x, dy = (float)cy - y;
      const float4 *L = rgba + ((size_t)b * nd + d) * hw;
      const float4 a00 = fetch_or_zero(L, fx, fy, width, height), a11 = fetch_or_zero(L, cx, cy, width, height);
      const float4 a01 = fetch_or_zero(L, fx, cy, width, height), a10 = fetch_or_zero(L, cx, fy, width, height);
      const float w00 = dx * dy, w11 = (1.0f - dx) * (1.0f - dy), w01 = dx * (1.0f - dy), w10 = (1.0f - dx) * dy;
      v.x = ((w00 * a00.x + w11 * a11.x) + w01 * a01.x) + w10 * a10.x;
      v.y = ((w00 * a00.y + w11 * a11.y) + w01 * a01.y) + w10 * a10.y;
      v.z = ((w00 * a00.z + w11 * a11.z) + w01 * a01.z) + w10 * a10.z;
      v.w = ((w00 * a00.w + w11 * a11.w) + w01 * a01.w) + w10 * a10.w;
    }
    if (d == 0) {
      o0 = v.x; o1 = v.y; o2 = v.z;
    } else {
      const float om = 1.0f - v.w;
      o0 = v.x * v.w + o0 * om;
      o1 = v.y * v.w + o1 * om;
      o2 = v.z * v.w + o2 * om;
    }
  }
  float *o = out_rgb + ((size_t)b * hw + (size_t)i * width + j) * 3;
  o[0] = o0; o[1] = o1; o[2] = o2;
}

// The MPI render for a viewer (msi_mpi_render_views; no reference counterpart): V target cameras per stack in one launch, any output size,
// rgb and / or the one-channel depth of over_composite_depth, from an fp32, rgba8 or rgba16f stack.  mpi_render_kernel above stays as it is;
// this kernel repeats its arithmetic op for op -- the homography (rot_t, divide_safe, m1, K_s @ m1, @ K_t_inv), the three dot products,
// divide_safe on ws, the two IEEE divides, the (-1, W) x (-1, H) test, floor, the four weights, the sum order w00 a00 + w11 a11 + w01 a01 +
// w10 a10 and the strictly sequential composite in one thread -- so at the stack's own size its rgb has the bits of msi_mpi_render_f32.
// What changes is the plumbing:
//   grid    1-D, sample -> view -> 4-row group -> 64-pixel block with the XCD-aware mapping of every many-views render (ViewBlock, geometry_device.h): the views of one stack follow
//           each other through the Infinity Cache and adjacent row groups share an XCD's L2.  A workgroup is 64 x 4 pixels of one (sample,
//           view), a wave one row; its D inverse homographies (source K of sample b, pose and inverse target K of view (b, v)) are computed
//           once in the prologue into LDS.
//   taps    buffer loads through a per-layer descriptor (the layer index is wave-uniform: scalar), one 16-, 8- or 4-byte load per tap.  A
//           tap outside the layer is given an offset beyond the descriptor's range and comes back as zeros: no branch.  The mask covers
//           columns AND rows: a column outside [0, W) would alias the neighbouring row, and a row outside [0, H) would leave the range by
//           itself, but at byte offsets within 16 bytes of 2^32 -- the explicit mask keeps every offset that is sent either inside the layer
//           or at 2^31.  fp32 and rgba16f zeros decode to the (0, 0, 0, 0) of fetch_or_zero; an rgba8 zero decodes to colour -1, so its three
//           colour channels are selected to zero by the same mask.  Decoders: geometry_device.h, the rule of msi_unpack_layers.
//   pixels  that sample outside (-1, W) x (-1, H) (or NaN) run the same instructions on the coordinate (0, 0) with every tap masked, and
//           their layer value is selected to zero: no divergent branch around the loads, same bits for the pixels inside.
//   loop    unrolled by 4: the warp of a layer does not depend on the running composite, so the taps of several layers are in flight under
//           the sequential blend.
// the texel at offset `texel` of layer L when ok, else the zeros of fetch_or_zero
template <int FMT>
__device__ __forceinline__ float4 mpi_tap(__amdgpu_buffer_rsrc_t L, int texel, bool ok) {
  float4 t = StackTexel<FMT>::tap(L, ok ? (unsigned)texel : 0x80000000u >> StackTexel<FMT>::shift);
  if constexpr (FMT == MSI_LAYERS_RGBA8) {   // (code 0 is colour -1; alpha 0 and the fp32 / rgba16f zeros are 0 already)
    t.x = ok ? t.x : 0.0f; t.y = ok ? t.y : 0.0f; t.z = ok ? t.z : 0.0f;
  }
  return t;
}

template <int MODE, int FMT>
__global__ void __launch_bounds__(256)
mpi_render_views_kernel(const void *__restrict__ layers, const float *__restrict__ tgt_pose, const float *__restrict__ intrinsics,
                        const float *__restrict__ tgt_intrinsics_inv, const float *__restrict__ depths, int batch, int views,
                        int height, int width, int nd, int out_h, int out_w, float *__restrict__ out_rgb,
                        float *__restrict__ out_depth, DepthFrac F) {
  __shared__ float hom[MPI_MAX_PLANES][9];
  ViewBlock<4> k(out_h, out_w, views, batch);
  if (k.past_end()) return;                             // (grid rounded up to a multiple of 8; whole workgroups leave)
  k.decode(views);
  const unsigned bv = k.bv;
  const int i = k.i, j = k.j, b = k.b;
  const int tid = threadIdx.y * 64 + threadIdx.x;
  if (tid < nd) {   // mpi_render_kernel's prologue, op for op
    const float *P = tgt_pose + (size_t)bv * 16;
    const float *Ks = intrinsics + (size_t)b * 9, *Ki = tgt_intrinsics_inv + (size_t)bv * 9;
    float rt[3][3], t[3];
#pragma unroll
    for (int r = 0; r < 3; ++r) {
#pragma unroll
      for (int c = 0; c < 3; ++c) rt[r][c] = P[c * 4 + r];  // rot_t = transpose(pose[:3,:3])
      t[r] = P[r * 4 + 3];
    }
    const float a = -depths[tid];
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
        hom[tid][r * 3 + c] = (m2[r][0] * Ki[0 * 3 + c] + m2[r][1] * Ki[1 * 3 + c]) + m2[r][2] * Ki[2 * 3 + c];
  }
  __syncthreads();
  if (j >= out_w || i >= out_h) return;
  const float uu = (float)j, vv = (float)i;  // meshgrid_abs of the OUTPUT size
  const size_t hw = (size_t)height * width;
  const float wf = (float)width, hf = (float)height;
  float o0 = 0.f, o1 = 0.f, o2 = 0.f, od = 0.f;
#pragma unroll 4
  for (int d = 0; d < nd; ++d) {
    const float *h = hom[d];
    const float xs = (uu * h[0] + vv * h[1]) + 1.0f * h[2];
    const float ys = (uu * h[3] + vv * h[4]) + 1.0f * h[5];
    float ws = (uu * h[6] + vv * h[7]) + 1.0f * h[8];
    ws += 1e-8f * (ws == 0.0f ? 1.0f : 0.0f);
    const float xq = xs / ws, yq = ys / ws;
    // tf.contrib.resampler: zero outside (-1, W) x (-1, H); missing corners are 0
    const bool inside = xq > -1.0f && yq > -1.0f && xq < wf && yq < hf;
    const float x = inside ? xq : 0.0f, y = inside ? yq : 0.0f;
    const float fxf = floorf(x), fyf = floorf(y);
    const int fx = (int)fxf, fy = (int)fyf, cx = fx + 1, cy = fy + 1;   // fx in [-1, W-1], fy in [-1, H-1]
    const float dx = (float)cx - x, dy = (float)cy - y;
    const bool x0 = inside && fx >= 0, x1 = inside && cx < width, y0 = fy >= 0, y1 = cy < height;
    const int r0 = fy * width, r1 = r0 + width;
    const __amdgpu_buffer_rsrc_t L = StackTexel<FMT>::layer(layers, b, nd, d, hw, (int)(hw << StackTexel<FMT>::shift));   // (H * W < 2^24, checked on the host)
    const float4 a00 = mpi_tap<FMT>(L, r0 + fx, x0 && y0), a11 = mpi_tap<FMT>(L, r1 + cx, x1 && y1);
    const float4 a01 = mpi_tap<FMT>(L, r1 + fx, x0 && y1), a10 = mpi_tap<FMT>(L, r0 + cx, x1 && y0);
    const float w00 = dx * dy, w11 = (1.0f - dx) * (1.0f - dy), w01 = dx * (1.0f - dy), w10 = (1.0f - dx) * dy;
    float4 c;   // (zero for a pixel that samples outside)
    c.w = inside ? ((w00 * a00.w + w11 * a11.w) + w01 * a01.w) + w10 * a10.w : 0.0f;
    c.x = inside ? ((w00 * a00.x + w11 * a11.x) + w01 * a01.x) + w10 * a10.x : 0.0f;
    c.y = inside ? ((w00 * a00.y + w11 * a11.y) + w01 * a01.y) + w10 * a10.y : 0.0f;
    c.z = inside ? ((w00 * a00.z + w11 * a11.z) + w01 * a01.z) + w10 * a10.z : 0.0f;
    const float al = c.w;
    if (MODE & RENDER_RGB) {
      if (d == 0) {
        o0 = c.x; o1 = c.y; o2 = c.z;
      } else {
        const float om = 1.0f - al;
        o0 = c.x * al + o0 * om;
        o1 = c.y * al + o1 * om;
        o2 = c.z * al + o2 * om;
      }
    }
    if (MODE & RENDER_DEPTH) {   // over_composite_depth: 0 at layer 0, then (d / D) a + out (1 - a)
      if (d == 0) od = 0.0f;
      else od = F.f[d] * al + od * (1.0f - al);
    }
  }
  store_pixel<MODE>(out_rgb, out_depth, ((size_t)bv * out_h + i) * out_w + j, o0, o1, o2, od);
}

}  // namespace

extern "C" {

int msi_perspective_plane_sweep_f32(const float *image, const float *pose, const float *intrinsics,
                                    const float *depths, int32_t batch, int32_t height, int32_t width,
                                    int32_t num_depths, float *psv, int32_t psv_channels,
                                    int32_t channel_offset, msi_stream_t stream) {
  MSI_REQUIRE(image && pose && intrinsics && depths && psv, "perspective_plane_sweep: null pointer");
  MSI_REQUIRE(batch >= 0 && height > 1 && width > 1 && num_depths > 0, "perspective_plane_sweep: bad dims");
  MSI_REQUIRE(channel_offset >= 0 && channel_offset + 3 * num_depths <= psv_channels,
              "perspective_plane_sweep: channel window outside %d channels", psv_channels);
  if (batch == 0) return MSI_OK;
  MSI_REQUIRE((long)width * num_depths < 2147483647L && height <= 65535 && batch <= 65535,
              "perspective_plane_sweep: problem too large");
  const dim3 grid((unsigned)(((long)width * num_depths + 255) / 256), height, batch);
  const UvGrid gs = uv_grid(width), gt = uv_grid(height);
  const unsigned magic = udiv_magic32(num_depths);
  const int nt = beyond_infinity_cache((size_t)batch * height * width * psv_channels * 4) ? 1 : 0;
  // full waves of complete pixels whose 3 D-float runs are 16-byte aligned, 32-bit byte offsets into one face
  const bool fast = 64 % num_depths == 0 && ((long)width * num_depths) % 256 == 0 && (3 * num_depths) % 4 == 0 && psv_channels % 4 == 0 && channel_offset % 4 == 0 &&
                    (long)height * width * 12 < 2147483647L && num_depths >= 4;
  if (fast)
    hipLaunchKernelGGL(pp_sweep_kernel<1>, grid, dim3(256), 0, msi::as_stream(stream), image, pose,
                       intrinsics, depths, batch, height, width, num_depths, gs.start, gs.step, gt.start, gt.step,
                       psv, psv_channels, channel_offset, magic, nt);
  else
    hipLaunchKernelGGL(pp_sweep_kernel<0>, grid, dim3(256), 0, msi::as_stream(stream), image, pose,
                       intrinsics, depths, batch, height, width, num_depths, gs.start, gs.step, gt.start, gt.step,
                       psv, psv_channels, channel_offset, magic, nt);
  return msi::check_launch("perspective_plane_sweep");
}

int msi_perspective_sweep_volume_bf16(const float *ref_image, const float *src_image, const float *ref_curr_pose,
                                      const float *src_curr_pose, const float *intrinsics, const float *depths,
                                      int32_t batch, int32_t height, int32_t width, int32_t num_depths,
                                      void *psv_bf16, msi_stream_t stream) {
  MSI_REQUIRE(ref_image && src_image && ref_curr_pose && src_curr_pose && intrinsics && depths && psv_bf16,
              "perspective_sweep_volume_bf16: null pointer");
  MSI_REQUIRE(batch >= 0 && height > 1 && width > 1 && num_depths > 0, "perspective_sweep_volume_bf16: bad dims");
  if (batch == 0) return MSI_OK;
  MSI_REQUIRE((long)width * num_depths < 2147483647L && height <= 65535 && batch <= 65535 && (long)height * width * 12 < 2147483647L,
              "perspective_sweep_volume_bf16: problem too large");
  const dim3 grid((unsigned)(((long)width * num_depths + 255) / 256), height, batch);
  const UvGrid gs = uv_grid(width), gt = uv_grid(height);
  const int nt = beyond_infinity_cache((size_t)batch * height * width * 6 * num_depths * 2) ? 1 : 0;
  int shift = 0;
  while ((1 << shift) < num_depths) ++shift;
  // whole waves of complete pixels (D a power of two up to 64), 16-byte-aligned volume
  const bool fast = 64 % num_depths == 0 && ((long)width * num_depths) % 64 == 0 && reinterpret_cast<uintptr_t>(psv_bf16) % 16 == 0;
  unsigned short *psv = static_cast<unsigned short *>(psv_bf16);
#define MSI_LAUNCH_PPV(FAST_, NT_)                                                                                                        \
  hipLaunchKernelGGL((pp_sweep_volume_bf16_kernel<FAST_, NT_>), grid, dim3(256), 0, msi::as_stream(stream), ref_image, src_image,       \
                     ref_curr_pose, src_curr_pose, intrinsics, depths, height, width, num_depths, shift, gs.start, gs.step, gt.start, gt.step, psv)
  if (fast && nt)
    MSI_LAUNCH_PPV(1, 1);
  else if (fast)
    MSI_LAUNCH_PPV(1, 0);
  else
    MSI_LAUNCH_PPV(0, 0);
#undef MSI_LAUNCH_PPV
  return msi::check_launch("perspective_sweep_volume_bf16");
}

int msi_mpi_render_f32(const float *rgba_native, const float *tgt_pose, const float *intrinsics,
                       const float *intrinsics_inv, const float *depths, int32_t batch, int32_t height,
                       int32_t width, int32_t num_planes, float *out_rgb, msi_stream_t stream) {
  MSI_REQUIRE(rgba_native && tgt_pose && intrinsics && intrinsics_inv && depths && out_rgb, "mpi_render: null pointer");
  MSI_REQUIRE(batch >= 0 && height > 0 && width > 0 && num_planes > 0, "mpi_render: bad dims");
  if (num_planes > MPI_MAX_PLANES)
    return msi::fail(MSI_E_UNSUPPORTED, "mpi_render: at most %d planes", MPI_MAX_PLANES);
  if (batch == 0) return MSI_OK;
  const dim3 grid((width + 63) / 64, (height + 3) / 4, batch), block(64, 4);
  hipLaunchKernelGGL(mpi_render_kernel, grid, block, 0, msi::as_stream(stream),
                     reinterpret_cast<const float4 *>(rgba_native), tgt_pose, intrinsics, intrinsics_inv, depths, batch,
                     height, width, num_planes, out_rgb);
  return msi::check_launch("mpi_render");
}

int msi_mpi_render_views(const void *layers, int32_t format, const float *tgt_pose, const float *intrinsics,
                         const float *tgt_intrinsics_inv, const float *depths, int32_t batch, int32_t views, int32_t height,
                         int32_t width, int32_t num_planes, int32_t out_height, int32_t out_width, float *out_rgb,
                         float *out_depth, msi_stream_t stream) {
  const ViewArgs a = {"mpi_render_views", out_rgb, out_depth, layers && tgt_pose && intrinsics && tgt_intrinsics_inv && depths, format, ANY_FORMAT, "",
                      nullptr, nullptr, nullptr, nullptr, batch >= 0 && height > 0 && width > 0 && num_planes > 0, (long)height * width,
                      views, batch, out_height, out_width, 4};
  const auto planes = [&] {
    return num_planes <= MPI_MAX_PLANES ? (int)MSI_OK : msi::fail(MSI_E_UNSUPPORTED, "mpi_render_views: at most %d planes", MPI_MAX_PLANES);
  };
  unsigned grid;
  if (const int e = check_views(a, planes, no_check, &grid)) return e;
  if (batch == 0) return MSI_OK;
  const DepthFrac F = depth_fractions(num_planes);
  hipStream_t s = msi::as_stream(stream);
  for_mode(render_mode(out_rgb, out_depth), [&](auto M) { for_format(format, [&](auto FMT) {
    hipLaunchKernelGGL((mpi_render_views_kernel<decltype(M)::value, decltype(FMT)::value>), dim3(grid), dim3(64, 4), 0, s, layers, tgt_pose,
                       intrinsics, tgt_intrinsics_inv, depths, batch, views, height, width, num_planes, out_height, out_width, out_rgb, out_depth, F);
  }); });
  return msi::check_launch("mpi_render_views");
}

}  // extern "C"
