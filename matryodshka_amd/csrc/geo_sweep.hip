// K1 of the geometry side, the ODS sphere sweep: ods_sweep_kernel (gathers from memory) and ods_sweep_lds_kernel (LDS-staged source patch), then
// sweep_common and the three C ABI entry points that launch them.  ods_quad / ods_tail / make_taps_bytes / gather3 are in geometry_device.h:
// hres_layers_kernel (geo_layers.hip) runs the same functions.
#include "geometry_device.h"

// tuning macros of this unit (MSI_GEO_DEFINES="-DMSI_SWEEP_WAVES=5" ...)
#ifndef MSI_SWEEP_WAVES   // amdgpu_waves_per_eu of ods_sweep_kernel's frame-loop form (LOOP = 1)
#define MSI_SWEEP_WAVES 4
#endif
#ifndef MSI_SWEEP_PREFETCH   // 1: the next frame's patch texels are requested into registers before this frame's gathers (tuning: 0 frees six registers)
#define MSI_SWEEP_PREFETCH 1
#endif
#ifndef MSI_SWEEP_PMAX
#define MSI_SWEEP_PMAX 192
#endif
#ifndef MSI_SWEEP_LDS_WAVES   // amdgpu_waves_per_eu of ods_sweep_lds_kernel (tuning)
#define MSI_SWEEP_LDS_WAVES 6
#endif
#ifndef MSI_SWEEP_NS_DEFAULT
#define MSI_SWEEP_NS_DEFAULT 2
#endif
#ifndef MSI_SWEEP_BCHUNK
#define MSI_SWEEP_BCHUNK 16
#endif
#ifndef MSI_SWEEP_NT   // -1 never / 0 by volume size / 1 always (A/B builds)
#define MSI_SWEEP_NT 0
#endif
#ifndef MSI_SWEEP_LDS_MIN_BATCH   // smallest batch that takes ods_sweep_lds_kernel (tuning: -DMSI_SWEEP_LDS_MIN_BATCH=1 / a huge value)
#define MSI_SWEEP_LDS_MIN_BATCH 2
#endif

namespace {

// One work item = (pixel, NS consecutive depths) for up to `bchunk` frames of the batch; depth is the fastest index so a
// wavefront's 64 lanes write 64 x NS consecutive 12-byte texels of the NHWC volume.  The source images (2.4 MB) stay L2-resident.
// OutT = float, or unsigned short = bf16 bits (the bf16 network input of BASELINE configs[2]).
// NS = samples (consecutive depths of one pixel) per thread: with two, the per-pixel work (trigonometry,
// index arithmetic) is shared and hipcc pairs the independent multiplies / adds of the two samples into
// v_pk_mul_f32 / v_pk_add_f32 (IEEE, same roundings as the scalar forms).
// NSRC = 1: one source (image0, pose0, order) -> channels [coff, coff + 3D).
// NSRC = 2: the whole double volume of format_network_input (msi.py:1124-1129): source 0 with order +1 into
// channels [0, 3D), source 1 with order -1 into [3D, 6D); the quadratic is shared when the two poses are equal.
// BATCH LOOP (round 4): the sample position (u, v), its four corners and weights depend on (pixel, depth, pose, baseline)
// only -- not on the image.  The reference recomputes them per batch element (projector.py:129-170 runs per sample); on
// the test path every frame has the identity pose and the camera file's baseline (data_loader.py:146-160), so a thread
// keeps the corners of its samples in registers (TapsB: ~230 of the ~276 VALU per sample) and walks the frames
// [blockIdx.z * bchunk, + bchunk): per frame a wave-uniform comparison of the 24 pose entries + baseline with those the
// previous frame's (bit patterns; scalar loads, scalar branch) decides between "gather with the held corners" and
// "recompute" -- the same arithmetic either way, so the volume is bit-identical to the frame-at-a-time form.
// LOOP = 0: one frame per thread (grid.z = batch, nothing to reuse: the compiler interleaves the corner arithmetic with
// the gathers and needs 88 instead of 119 registers -- five waves per SIMD; 61 vs 70 us at batch 1).
template <typename OutT, int NS, int NSRC, int LOOP>
__global__ void __launch_bounds__(256) __attribute__((amdgpu_waves_per_eu(LOOP ? MSI_SWEEP_WAVES : 1, 8)))
ods_sweep_kernel(const float *__restrict__ image0, const float *__restrict__ image1, const float *__restrict__ pose0,
                 const float *__restrict__ pose1, const float *__restrict__ intrinsics, const float *__restrict__ depths,
                 const float *__restrict__ trig, int batch, int height, int width, int nd,
                 float order, OutT *__restrict__ psv, int channels, int coff, PixConsts K, unsigned ng_magic, int coalesce,
                 int bchunk) {
  // grid = (ceil(W*(D/NS) / 256), H, ceil(B / bchunk)): 32-bit index math only (64-bit div/mod are emulated in ~100
  // VALU instructions each and used to dominate this kernel)
  const int ng = nd / NS;                       // depth groups per pixel (nd % NS == 0, checked on the host)
  const int idx = blockIdx.x * 256 + threadIdx.x;
  if (idx >= width * ng) return;
  unsigned jq = __umulhi((unsigned)idx, ng_magic);   // idx / ng by multiply-high (+ one correction), see cnn.hip udiv_magic
  if ((unsigned)idx - jq * (unsigned)ng >= (unsigned)ng) ++jq;
  const int j = (int)jq, d0 = (idx - j * ng) * NS;
  const int i = blockIdx.y;
  const int b_lo = LOOP ? blockIdx.z * bchunk : blockIdx.z, b_hi = LOOP ? min(batch, b_lo + bchunk) : b_lo + 1;

  const float cs = trig[j], ss = trig[width + j];
  const float ct = trig[2 * width + i], st = trig[2 * width + height + i];
  const int img_bytes = height * width * 12;
  const float csct = cs * ct, ssct = ss * ct;
  float depth[NS];
#pragma unroll
  for (int q = 0; q < NS; ++q) depth[q] = depths[d0 + q];

  // lane -> (pixel of the wave, depth group) for the whole-pixel store path
  const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
  unsigned plq = __umulhi((unsigned)lane, ng_magic);      // lane / ng by multiply-high (+ one correction), like idx / ng above
  if ((unsigned)lane - plq * (unsigned)ng >= (unsigned)ng) ++plq;
  const int pl = (int)plq, dg = lane - pl * ng;
  constexpr int WAVE_ELEMS = 384 * NS;
  __shared__ __attribute__((aligned(16))) OutT s_out[4][WAVE_ELEMS];

  // bit k of eqmask: frame b_lo + k has bit for bit the poses and the baseline of frame b_lo + k - 1 (wave-uniform: scalar
  // loads and integer compares, all issued before the frame loop so that no frame waits on them)
  unsigned eqmask = 0;
  if (LOOP) {
    const unsigned *U0 = reinterpret_cast<const unsigned *>(pose0), *U1 = reinterpret_cast<const unsigned *>(NSRC == 2 ? pose1 : pose0);
    const unsigned *UI = reinterpret_cast<const unsigned *>(intrinsics);
    for (int b = b_lo + 1; b < b_hi; ++b) {
      bool eq = UI[(size_t)b * 9] == UI[(size_t)(b - 1) * 9];
#pragma unroll
      for (int k = 0; k < 12; ++k)
        eq = eq && (U0[(size_t)b * 16 + k] == U0[(size_t)(b - 1) * 16 + k]) && (NSRC == 1 || U1[(size_t)b * 16 + k] == U1[(size_t)(b - 1) * 16 + k]);
      eqmask |= (eq ? 1u : 0u) << (b - b_lo);
    }
    eqmask = __builtin_amdgcn_readfirstlane(eqmask);
  }
  TapsB taps[NSRC][NS];
  for (int b = b_lo; b < b_hi; ++b) {
    const float *P0 = pose0 + (size_t)b * 16;
    const float *P1 = NSRC == 2 ? pose1 + (size_t)b * 16 : P0;
    const bool reuse = (eqmask >> (b - b_lo)) & 1u;   // the corners in `taps` were computed for an identical frame
    const __amdgpu_buffer_rsrc_t img0 = __builtin_amdgcn_make_buffer_rsrc((void *)(image0 + (size_t)b * height * width * 3), 0, img_bytes, 0x00020000);
    const __amdgpu_buffer_rsrc_t img1 = NSRC == 2 ? __builtin_amdgcn_make_buffer_rsrc((void *)(image1 + (size_t)b * height * width * 3), 0, img_bytes, 0x00020000) : img0;
    float out[NSRC][NS][3];
    if (!reuse) {
      const float r = intrinsics[(size_t)b * 9];
      bool same = NSRC == 2;                      // both sources share the quadratic when their poses are equal
      if (NSRC == 2) {
#pragma unroll
        for (int k = 0; k < 12; ++k) same = same && (P0[k] == P1[k]);
      }
#pragma unroll
      for (int q = 0; q < NS; ++q) {
        float u, v;
        const OdsQuad q0 = ods_quad(P0, r, depth[q], csct, st, ssct);
        ods_tail(q0, NSRC == 2 ? 1.0f : order, K, u, v);
        taps[0][q] = make_taps_bytes(u, v, width, height);
        if (!LOOP) gather3(img0, taps[0][q], out[0][q]);      // (one frame per thread: request each sample as soon as its corners exist)
        if (NSRC == 2) {
          if (same) {
            ods_tail(q0, -1.0f, K, u, v);
          } else {
            const OdsQuad q1 = ods_quad(P1, r, depth[q], csct, st, ssct);
            ods_tail(q1, -1.0f, K, u, v);
          }
          taps[NSRC - 1][q] = make_taps_bytes(u, v, width, height);
          if (!LOOP) gather3(img1, taps[NSRC - 1][q], out[NSRC - 1][q]);
        }
      }
    }
    if (LOOP) {
#pragma unroll
      for (int q = 0; q < NS; ++q) {
        gather3(img0, taps[0][q], out[0][q]);
        if (NSRC == 2) gather3(img1, taps[NSRC - 1][q], out[NSRC - 1][q]);
      }
    }
    const long p = ((long)b * height + i) * width + j;
    if (NSRC == 2 && coalesce) {
      // Whole-pixel stores: with both sources in one thread a wavefront owns 64 / ng complete pixels = 384 NS
      // CONTIGUOUS elements of the NHWC volume.  They are exchanged through a wave-private LDS strip and leave as
      // 16-byte-per-lane stores (3 fully coalesced instructions per wave instead of 12 strided dword stores per lane,
      // which kept the store path -- not the VALU -- the limiter of this kernel).  No block barrier: LDS operations of
      // one wave are performed in order (the next frame's strip writes follow this frame's strip reads).
      OutT *w = s_out[wave];
      __builtin_amdgcn_wave_barrier();
#pragma unroll
      for (int sidx = 0; sidx < 2; ++sidx) {
        const int e0 = pl * 6 * nd + sidx * 3 * nd + dg * NS * 3;     // a lane's 3 NS values per source are contiguous
        if constexpr (sizeof(OutT) == 2 && NS % 2 == 0) {
          // bf16, two values per instruction (v_cvt_pk_bf16_f32: round to nearest even, what f32_to_bf16 computes for the
          // finite values stored here) and dword LDS stores (e0 is even): 12 integer-rounding sequences + 12 ds_write_b16 per
          // lane and frame were a third of the per-frame instruction stream once the corners are reused
          unsigned *wd = reinterpret_cast<unsigned *>(w + e0);
          const float *v = &out[sidx][0][0];
#pragma unroll
          for (int k = 0; k < 3 * NS / 2; ++k) {
            unsigned pk;
            asm("v_cvt_pk_bf16_f32 %0, %1, %2" : "=v"(pk) : "v"(v[2 * k]), "v"(v[2 * k + 1]));
            wd[k] = pk;
          }
        } else {
#pragma unroll
          for (int q = 0; q < NS; ++q)
#pragma unroll
            for (int c = 0; c < 3; ++c) store_elem(w, (size_t)(e0 + q * 3 + c), out[sidx][q][c]);
        }
      }
      __builtin_amdgcn_wave_barrier();
      const size_t first = (size_t)(p - pl) * channels;      // element offset of the wave's first pixel (lane 0's pixel)
      const uint4 *src = reinterpret_cast<const uint4 *>(w);
      uint4 *dst = reinterpret_cast<uint4 *>(psv + first);
      constexpr int NV = WAVE_ELEMS * (int)sizeof(OutT) / 16;
#pragma unroll
      for (int k = lane; k < NV; k += 64) sweep_store16(dst + k, src[k], coalesce >> 1);
      continue;
    }
#pragma unroll
    for (int sidx = 0; sidx < NSRC; ++sidx) {
      const size_t o = (size_t)p * channels + (NSRC == 2 ? sidx * 3 * nd : coff) + d0 * 3;
#pragma unroll
      for (int q = 0; q < NS; ++q) {
        store_elem(psv, o + q * 3 + 0, out[sidx][q][0]);
        store_elem(psv, o + q * 3 + 1, out[sidx][q][1]);
        store_elem(psv, o + q * 3 + 2, out[sidx][q][2]);
      }
    }
  }
}

// ---- K1 with an LDS-staged source patch (round 6) --------------------------------
// What bounds ods_sweep_kernel once the corners are reused across frames is neither bytes (1.07 x the algorithmic traffic) nor VALU but the
// SIXTEEN dependent 12-byte gathers per thread and frame through the vector L1's address path (~21 cycles per instruction and CU).  The
// footprint of those gathers is tiny: a block's 256 / ng pixels of one row sample, over all depths and both sources, a patch of a few rows
// x (pixels + 2 disparities) columns of each image.  This kernel stages that patch once per frame and block in LDS -- coalesced row segments,
// texels padded to 16 bytes -- and gathers with ds_read_b128 (two address registers per sample: the corners are base, base + 16, base + pitch,
// base + pitch + 16) instead of buffer_load_dwordx3.  The patch is found, not assumed: when a thread computes its corners it also takes the
// UNWRAPPED corner (x0, y0) relative to the block's own position (W - 1 - j0, i), wrapped into [-n/2, n/2) so that the seam is nothing special;
// a block-wide min / max gives the box, and a block whose box does not fit (polar rows, where the disparity grows like 1 / cos(lat); rows whose
// near planes are invalid and sample pixel (1, 1); rotated poses) keeps gathering from memory exactly as ods_sweep_kernel does -- a block-uniform
// choice made once per (pose, baseline), not per frame.  Same corners, same weights, same blend: the volume is bit-identical.
// Frames: patch buffers alternate (frame b in buffer b & 1), so ONE block barrier per frame orders both "patch b is visible" and "everybody is
// done with patch b - 1"; the next frame's texels are requested into registers before this frame's gathers.
// Occupancy is what this kernel is most sensitive to (r06, same-box A/Bs at configs[2] / [3], gpurun_out/r06_occ*.log, r06_w6.log): 384 texels and four waves per SIMD
// 0.98 / 5.97 ms; 256 texels -- ONE staged texel per thread and source instead of two -- 0.90 / 5.27; five waves per SIMD (91 VGPRs) 0.81 / 5.05-5.3; and, once the
// per-sample state was cut to a weight quadruple + one packed corner word (TapsC) and the depths are re-read where the corners are computed, SIX waves without a spill
// (80 VGPRs; 192 texels so that six blocks' LDS fit with fp32 strips: 24.6 KB) 0.74 / 4.85 ms.  Six waves WITH spills (56 bytes) had lost (0.93 / 6.4); 128 texels: more
// fallback blocks at configs[3] (5.2 ms).
constexpr int SW_PMAX = MSI_SWEEP_PMAX;                 // texels per source and buffer (16 B each): 2 buffers x 2 sources x 3 KB
constexpr int SW_NST = (SW_PMAX + 255) / 256;   // texels a thread stages per source

struct TapsL {
  TapsB t;
  int x0, y0;                                // unwrapped, clamped corner (make_taps_ranged's x0 / y0)
};
// What ods_sweep_lds_kernel keeps per sample across frames: the weights and ONE word for the corners.  Blocks that read their patch from LDS need no memory offsets at
// all; fallback blocks rebuild the four byte offsets from corner a's (bits 0-27: H * W * 12 < 2^28) and two flags -- x1 wrapped to column 0 (bit 30), y1 wrapped to row 0
// (bit 31) -- with three adds per frame and sample.  Twelve registers less than four offsets per sample: the kernel fits five waves per SIMD with room to spare.
struct TapsC {
  unsigned oaf;
  float wa, wb, wc, wd;
};
__device__ __forceinline__ TapsC compact_taps(const TapsB &t) {
  TapsC c;
  c.oaf = t.oa | (t.ob < t.oa ? 0x40000000u : 0u) | (t.oc < t.oa ? 0x80000000u : 0u);   // (x1 = x0 + 1 unless it wrapped to 0: then ob < oa; likewise y1)
  c.wa = t.wa; c.wb = t.wb; c.wc = t.wc; c.wd = t.wd;
  return c;
}
__device__ __forceinline__ TapsB expand_taps(const TapsC &c, int width, int height) {
  TapsB t;
  t.oa = c.oaf & 0x0fffffffu;
  const unsigned dx = (c.oaf & 0x40000000u) ? (unsigned)(-(width - 1) * 12) : 12u;
  const unsigned dy = (c.oaf & 0x80000000u) ? (unsigned)(-(height - 1) * width * 12) : (unsigned)(width * 12);
  t.ob = t.oa + dx; t.oc = t.oa + dy; t.od = t.oa + dy + dx;
  t.wa = c.wa; t.wb = c.wb; t.wc = c.wc; t.wd = c.wd;
  return t;
}
__device__ __forceinline__ float blend4(const TapsC &t, float a, float b, float c, float d) {
  return ((t.wa * a + t.wb * b) + t.wc * c) + t.wd * d;
}
__device__ __forceinline__ TapsL make_taps_lds(float u, float v, int width, int height) {
  TapsL r;
  r.t = make_taps_bytes(u, v, width, height);
  r.x0 = max(-1, min((int)floorf(u), width - 1));
  r.y0 = max(-1, min((int)floorf(v), height - 1));
  return r;
}
__device__ __forceinline__ int centred(int d, int n) {          // d in (-2n, 2n) -> the representative of d mod n in [-n/2, n/2)
  const int half = n >> 1;
  d = d < -half ? d + n : d;
  d = d >= n - half ? d - n : d;
  d = d < -half ? d + n : d;
  d = d >= n - half ? d - n : d;
  return d;
}
__device__ __forceinline__ int wave_min_i(int v) {
#pragma unroll
  for (int o = 32; o > 0; o >>= 1) v = min(v, __shfl_xor(v, o, 64));
  return v;
}
__device__ __forceinline__ int wave_max_i(int v) {
#pragma unroll
  for (int o = 32; o > 0; o >>= 1) v = max(v, __shfl_xor(v, o, 64));
  return v;
}

template <typename OutT, int NS>
__global__ void __launch_bounds__(256) __attribute__((amdgpu_waves_per_eu(MSI_SWEEP_LDS_WAVES, 8)))
ods_sweep_lds_kernel(const float *__restrict__ image0, const float *__restrict__ image1, const float *__restrict__ pose0,
                     const float *__restrict__ pose1, const float *__restrict__ intrinsics, const float *__restrict__ depths,
                     const float *__restrict__ trig, int batch, int height, int width, int nd,
                     OutT *__restrict__ psv, int channels, PixConsts K, unsigned ng_magic, int bchunk, int nt) {
  // grid as ods_sweep_kernel<OutT, NS, 2, 1> with the whole-pixel store path; the host guarantees 256 % ng == 0 and (W * ng) % 256 == 0,
  // so every block is full and owns 256 / ng complete pixels of row blockIdx.y
  const int ng = nd / NS;
  const int tid = threadIdx.x;
  const int idx = blockIdx.x * 256 + tid;
  unsigned jq = __umulhi((unsigned)idx, ng_magic);
  if ((unsigned)idx - jq * (unsigned)ng >= (unsigned)ng) ++jq;
  const int j = (int)jq, d0 = (idx - j * ng) * NS;
  const int i = blockIdx.y;
  const int b_lo = blockIdx.z * bchunk, b_hi = min(batch, b_lo + bchunk);
  unsigned j0q = __umulhi((unsigned)(blockIdx.x * 256), ng_magic);
  if ((unsigned)(blockIdx.x * 256) - j0q * (unsigned)ng >= (unsigned)ng) ++j0q;
  const int xc = width - 1 - (int)j0q;        // where the block's first pixel samples at infinite depth (identity pose): the centre the box is measured from

  const float cs = trig[j], ss = trig[width + j];
  const float ct = trig[2 * width + i], st = trig[2 * width + height + i];
  const int img_bytes = height * width * 12;
  const float csct = cs * ct, ssct = ss * ct;

  const int lane = tid & 63, wave = tid >> 6;
  unsigned plq = __umulhi((unsigned)lane, ng_magic);
  if ((unsigned)lane - plq * (unsigned)ng >= (unsigned)ng) ++plq;
  const int pl = (int)plq, dg = lane - pl * ng;
  constexpr int WAVE_ELEMS = 384 * NS;
  __shared__ __attribute__((aligned(16))) OutT s_out[4][WAVE_ELEMS];
  __shared__ __attribute__((aligned(16))) float4 s_patch[2][2][SW_PMAX];     // [buffer][source][texel]
  __shared__ int s_box[4];

  // (r06, measured and dropped: the frame-equality mask worked out by wave 0 alone and handed over through LDS -- 3 % slower; wave-PRIVATE patches without any block
  //  barrier in the frame loop -- 8 % slower at configs[2], 4 % at configs[3]: 2.3 x the staging loads, more fallback waves; gpurun_out/r06_eq.log, r06_wp.log)
  unsigned eqmask = 0;
  {
    const unsigned *U0 = reinterpret_cast<const unsigned *>(pose0), *U1 = reinterpret_cast<const unsigned *>(pose1);
    const unsigned *UI = reinterpret_cast<const unsigned *>(intrinsics);
    for (int b = b_lo + 1; b < b_hi; ++b) {
      bool eq = UI[(size_t)b * 9] == UI[(size_t)(b - 1) * 9];
#pragma unroll
      for (int k = 0; k < 12; ++k)
        eq = eq && (U0[(size_t)b * 16 + k] == U0[(size_t)(b - 1) * 16 + k]) && (U1[(size_t)b * 16 + k] == U1[(size_t)(b - 1) * 16 + k]);
      eqmask |= (eq ? 1u : 0u) << (b - b_lo);
    }
    eqmask = __builtin_amdgcn_readfirstlane(eqmask);
  }
  // (the wave's strip goes to its first pixel's row of the volume: one 64-bit product here, an add per frame)
  const size_t frame_elems = (size_t)height * width * channels;
  OutT *wdst = psv + (size_t)((((long)b_lo * height + i) * width + j) - pl) * channels;
  TapsC taps[2][NS];
  int lbase[2][NS];                            // float4 index of a sample's corner (y0, x0) in its source's patch
  unsigned goff[SW_NST];                       // byte offset in the image of the texels this thread stages (same for both sources), ~0u = none
  f32x3_g stg[2][SW_NST];
  int pitch = 0;
  bool lds_mode = false, pending = false;
  auto stage_load = [&](int b) __attribute__((always_inline)) {
    const __amdgpu_buffer_rsrc_t im0 = __builtin_amdgcn_make_buffer_rsrc((void *)(image0 + (size_t)b * height * width * 3), 0, img_bytes, 0x00020000);
    const __amdgpu_buffer_rsrc_t im1 = __builtin_amdgcn_make_buffer_rsrc((void *)(image1 + (size_t)b * height * width * 3), 0, img_bytes, 0x00020000);
#pragma unroll
    for (int k = 0; k < SW_NST; ++k) {           // (offsets beyond the descriptor -- ~0u -- return zeros: texels nobody reads)
      stg[0][k] = __builtin_bit_cast(f32x3_g, (u32x3_g)__builtin_amdgcn_raw_buffer_load_b96(im0, goff[k], 0, 0));
      stg[1][k] = __builtin_bit_cast(f32x3_g, (u32x3_g)__builtin_amdgcn_raw_buffer_load_b96(im1, goff[k], 0, 0));
    }
  };
  for (int b = b_lo; b < b_hi; ++b) {
    const float *P0 = pose0 + (size_t)b * 16;
    const float *P1 = pose1 + (size_t)b * 16;
    const bool reuse = (eqmask >> (b - b_lo)) & 1u;
    float out[2][NS][3];
    if (!reuse) {
      const float r = intrinsics[(size_t)b * 9];
      bool same = true;
#pragma unroll
      for (int k = 0; k < 12; ++k) same = same && (P0[k] == P1[k]);
      int xr[2][NS], yr[2][NS];
      float depth[NS];                          // (read where the corners are computed, not held across the frame loop)
#pragma unroll
      for (int q = 0; q < NS; ++q) depth[q] = depths[d0 + q];
      int xmin = 0x7fffffff, xmax = -0x7fffffff, ymin = 0x7fffffff, ymax = -0x7fffffff;
#pragma unroll
      for (int q = 0; q < NS; ++q) {
        float u, v;
        const OdsQuad q0 = ods_quad(P0, r, depth[q], csct, st, ssct);
        ods_tail(q0, 1.0f, K, u, v);
        TapsL t0 = make_taps_lds(u, v, width, height);
        if (same) {
          ods_tail(q0, -1.0f, K, u, v);
        } else {
          const OdsQuad q1 = ods_quad(P1, r, depth[q], csct, st, ssct);
          ods_tail(q1, -1.0f, K, u, v);
        }
        TapsL t1 = make_taps_lds(u, v, width, height);
        taps[0][q] = compact_taps(t0.t); taps[1][q] = compact_taps(t1.t);
        xr[0][q] = centred(t0.x0 - xc, width); yr[0][q] = centred(t0.y0 - i, height);
        xr[1][q] = centred(t1.x0 - xc, width); yr[1][q] = centred(t1.y0 - i, height);
#pragma unroll
        for (int s_ = 0; s_ < 2; ++s_) {
          xmin = min(xmin, xr[s_][q]); xmax = max(xmax, xr[s_][q]);
          ymin = min(ymin, yr[s_][q]); ymax = max(ymax, yr[s_][q]);
        }
      }
      // the block's box (both sources share it: the two disparities mirror each other around the same centre)
      if (tid == 0) { s_box[0] = 0x7fffffff; s_box[1] = -0x7fffffff; s_box[2] = 0x7fffffff; s_box[3] = -0x7fffffff; }
      __syncthreads();
      xmin = wave_min_i(xmin); xmax = wave_max_i(xmax); ymin = wave_min_i(ymin); ymax = wave_max_i(ymax);
      if (lane == 0) { atomicMin(&s_box[0], xmin); atomicMax(&s_box[1], xmax); atomicMin(&s_box[2], ymin); atomicMax(&s_box[3], ymax); }
      __syncthreads();
      xmin = s_box[0]; xmax = s_box[1]; ymin = s_box[2]; ymax = s_box[3];
      __syncthreads();                                              // (every wave has read the box before a later recompute -- possibly with no frame barrier in between: fallback blocks -- re-initialises it)
      const int pw = xmax - xmin + 2, ph = ymax - ymin + 2;          // (+ the x1 / y1 corners)
      pitch = ((pw + 7) & ~15) + 8;                                   // >= pw, = 8 mod 16: consecutive patch rows start half the banks apart
      lds_mode = ph * pitch <= SW_PMAX;
      pending = false;
      if (lds_mode) {
#pragma unroll
        for (int q = 0; q < NS; ++q) {
          lbase[0][q] = (yr[0][q] - ymin) * pitch + (xr[0][q] - xmin);
          lbase[1][q] = (yr[1][q] - ymin) * pitch + (xr[1][q] - xmin);
        }
        const float rp = 1.0f / (float)pitch;
#pragma unroll
        for (int k = 0; k < SW_NST; ++k) {
          const int t = tid + k * 256;
          int yy = (int)(((float)t + 0.5f) * rp);                     // t / pitch (t < 512, pitch <= 384: exact up to the correction below)
          yy += (t - yy * pitch >= pitch) ? 1 : 0;
          yy -= (t - yy * pitch < 0) ? 1 : 0;
          const int xx = t - yy * pitch;
          const int row = floor_mod(i + ymin + yy + height, height), col = floor_mod(xc + xmin + xx + width, width);
          goff[k] = (t < SW_PMAX && yy < ph && xx < pw) ? __umul24((unsigned)(row * width + col), 12u) : 0xffffffffu;
        }
      }
    }
    if (lds_mode) {
      if (!pending) stage_load(b);
      float4 *pb0 = s_patch[b & 1][0], *pb1 = s_patch[b & 1][1];
#pragma unroll
      for (int k = 0; k < SW_NST; ++k) {
        const int t = tid + k * 256;
        if (t < SW_PMAX) {
          pb0[t] = float4{stg[0][k].x, stg[0][k].y, stg[0][k].z, 0.f};
          pb1[t] = float4{stg[1][k].x, stg[1][k].y, stg[1][k].z, 0.f};
        }
      }
      __syncthreads();                                                 // patch b visible; everybody is done with patch b - 1 (its buffer is free for b + 1)
      pending = MSI_SWEEP_PREFETCH && (b + 1 < b_hi) && ((eqmask >> (b + 1 - b_lo)) & 1u);
      if (pending) stage_load(b + 1);
#pragma unroll
      for (int q = 0; q < NS; ++q)
#pragma unroll
        for (int s_ = 0; s_ < 2; ++s_) {
          const float4 *pp = (s_ ? pb1 : pb0) + lbase[s_][q];
          const float4 a = pp[0], bb = pp[1], c = pp[pitch], d = pp[pitch + 1];
          const TapsC &t = taps[s_][q];
          out[s_][q][0] = blend4(t, a.x, bb.x, c.x, d.x);
          out[s_][q][1] = blend4(t, a.y, bb.y, c.y, d.y);
          out[s_][q][2] = blend4(t, a.z, bb.z, c.z, d.z);
        }
    } else {
      const __amdgpu_buffer_rsrc_t img0 = __builtin_amdgcn_make_buffer_rsrc((void *)(image0 + (size_t)b * height * width * 3), 0, img_bytes, 0x00020000);
      const __amdgpu_buffer_rsrc_t img1 = __builtin_amdgcn_make_buffer_rsrc((void *)(image1 + (size_t)b * height * width * 3), 0, img_bytes, 0x00020000);
#pragma unroll
      for (int q = 0; q < NS; ++q) {
        gather3(img0, expand_taps(taps[0][q], width, height), out[0][q]);
        gather3(img1, expand_taps(taps[1][q], width, height), out[1][q]);
      }
    }
    // whole-pixel stores through the wave's strip: exactly ods_sweep_kernel's
    OutT *w = s_out[wave];
    __builtin_amdgcn_wave_barrier();
#pragma unroll
    for (int sidx = 0; sidx < 2; ++sidx) {
      const int e0 = pl * 6 * nd + sidx * 3 * nd + dg * NS * 3;
      if constexpr (sizeof(OutT) == 2 && NS % 2 == 0) {
        unsigned *wd = reinterpret_cast<unsigned *>(w + e0);
        const float *v = &out[sidx][0][0];
#pragma unroll
        for (int k = 0; k < 3 * NS / 2; ++k) {
          unsigned pk;
          asm("v_cvt_pk_bf16_f32 %0, %1, %2" : "=v"(pk) : "v"(v[2 * k]), "v"(v[2 * k + 1]));
          wd[k] = pk;
        }
      } else {
#pragma unroll
        for (int q = 0; q < NS; ++q)
#pragma unroll
          for (int c = 0; c < 3; ++c) store_elem(w, (size_t)(e0 + q * 3 + c), out[sidx][q][c]);
      }
    }
    __builtin_amdgcn_wave_barrier();
    const uint4 *src = reinterpret_cast<const uint4 *>(w);
    uint4 *dst = reinterpret_cast<uint4 *>(wdst);          // the wave's first pixel of frame b
    wdst += frame_elems;
    constexpr int NV = WAVE_ELEMS * (int)sizeof(OutT) / 16;
#pragma unroll
    for (int k = lane; k < NV; k += 64) sweep_store16(dst + k, src[k], nt);
  }
}

}  // namespace

extern "C" {

// (which form a shape takes, restated on the host: sweep_form in tests/sweep_cases.py -- its case table reaches every form; keep the two in step)
static int sweep_common(const float *image, const float *image1, const float *pose, const float *pose1,
                        const float *intrinsics,
                        const float *depths, const float *trig, int32_t batch,
                        int32_t height, int32_t width, int32_t num_depths, int32_t order,
                        void *psv, int psv_bf16, int32_t psv_channels, int32_t channel_offset,
                        msi_stream_t stream) {
  const bool pair = image1 != nullptr;
  MSI_REQUIRE(image && pose && intrinsics && depths && trig && psv && (!pair || pose1), "ods_sphere_sweep: null pointer");
  MSI_REQUIRE(batch >= 0 && height > 0 && width > 0 && num_depths > 0, "ods_sphere_sweep: bad dims");
  MSI_REQUIRE(order == 1 || order == -1, "ods_sphere_sweep: order must be +1 or -1");
  MSI_REQUIRE(channel_offset >= 0 && channel_offset + (pair ? 6 : 3) * num_depths <= psv_channels,
              "ods_sphere_sweep: channel window [%d,%d) outside %d channels", channel_offset,
              channel_offset + (pair ? 6 : 3) * num_depths, psv_channels);
  if (batch == 0) return MSI_OK;
  MSI_REQUIRE((long)width * num_depths < 2147483647L && height <= 65535 && batch <= 65535 && (long)height * width < (1L << 24),
              "ods_sphere_sweep: problem too large (24-bit pixel offsets: H * W < 2^24)");
  // NS depths per thread (bit-identical results for every NS; -DMSI_SWEEP_NS_DEFAULT=1/2/4 at build time)
  int ns = MSI_SWEEP_NS_DEFAULT;
  while (num_depths % ns != 0) ns >>= 1;
  // frames per thread (see the kernel's BATCH LOOP): up to MSI_SWEEP_BCHUNK consecutive frames share a thread's sample
  // corners when their poses / baselines agree; chunks keep grid.z >= 1 and every chunk but the last full
  const int bchunk = batch < MSI_SWEEP_BCHUNK ? batch : MSI_SWEEP_BCHUNK;
  const dim3 grid((unsigned)(((long)width * (num_depths / ns) + 255) / 256), height, (batch + bchunk - 1) / bchunk);
  // non-temporal whole-pixel stores when the volume cannot stay in the Infinity Cache anyway (sweep_store16)
  const int nt = MSI_SWEEP_NT < 0 ? 0 : (MSI_SWEEP_NT > 0 || beyond_infinity_cache((size_t)batch * height * width * psv_channels * (psv_bf16 ? 2 : 4))) ? 1 : 0;
#define MSI_LAUNCH_SWEEP(T, NS_, NSRC_, LOOP_)                                                                          \
  hipLaunchKernelGGL((ods_sweep_kernel<T, NS_, NSRC_, LOOP_>), grid, dim3(256), 0, msi::as_stream(stream), image, image1, \
                     pose, pose1, intrinsics, depths, trig, batch, height, width, num_depths, (float)order,      \
                     static_cast<T *>(psv), psv_channels, channel_offset, make_consts(height, width),           \
                     udiv_magic32(num_depths / NS_),                                                            \
                     (pair && 64 % (num_depths / NS_) == 0 && ((long)width * (num_depths / NS_)) % 64 == 0) ? 1 + 2 * nt : 0, bchunk)
#define MSI_LAUNCH_SWEEP_N(T, NSRC_, LOOP_)                                                              \
  { if (ns == 4) MSI_LAUNCH_SWEEP(T, 4, NSRC_, LOOP_); else if (ns == 2) MSI_LAUNCH_SWEEP(T, 2, NSRC_, LOOP_); else MSI_LAUNCH_SWEEP(T, 1, NSRC_, LOOP_); }
#define MSI_LAUNCH_SWEEP_L(T, NSRC_) { if (bchunk > 1) MSI_LAUNCH_SWEEP_N(T, NSRC_, 1) else MSI_LAUNCH_SWEEP_N(T, NSRC_, 0) }
#define MSI_LAUNCH_SWEEP_T(T) { if (pair) MSI_LAUNCH_SWEEP_L(T, 2) else MSI_LAUNCH_SWEEP_L(T, 1) }
  // the LDS-staged form (ods_sweep_lds_kernel): the double volume with whole-pixel stores, full blocks of complete pixels, NS = 2, and a batch worth a frame loop
  const int ng2 = num_depths / 2;
  if (pair && ns == 2 && batch >= MSI_SWEEP_LDS_MIN_BATCH && ng2 > 0 && 64 % ng2 == 0 && ((long)width * ng2) % 256 == 0) {
    const unsigned magic = udiv_magic32(ng2);
    if (psv_bf16)
      hipLaunchKernelGGL((ods_sweep_lds_kernel<unsigned short, 2>), grid, dim3(256), 0, msi::as_stream(stream), image, image1, pose, pose1, intrinsics, depths, trig, batch,
                         height, width, num_depths, static_cast<unsigned short *>(psv), psv_channels, make_consts(height, width), magic, bchunk, nt);
    else
      hipLaunchKernelGGL((ods_sweep_lds_kernel<float, 2>), grid, dim3(256), 0, msi::as_stream(stream), image, image1, pose, pose1, intrinsics, depths, trig, batch,
                         height, width, num_depths, static_cast<float *>(psv), psv_channels, make_consts(height, width), magic, bchunk, nt);
    return msi::check_launch("ods_sphere_sweep (lds)");
  }
  if (psv_bf16) MSI_LAUNCH_SWEEP_T(unsigned short) else MSI_LAUNCH_SWEEP_T(float)
#undef MSI_LAUNCH_SWEEP_T
#undef MSI_LAUNCH_SWEEP_L
#undef MSI_LAUNCH_SWEEP_N
#undef MSI_LAUNCH_SWEEP
  return msi::check_launch("ods_sphere_sweep");
}

int msi_ods_sphere_sweep_f32(const float *image, const float *pose, const float *intrinsics,
                             const float *depths, const float *trig, int32_t batch,
                             int32_t height, int32_t width, int32_t num_depths, int32_t order,
                             float *psv, int32_t psv_channels, int32_t channel_offset,
                             msi_stream_t stream) {
  return sweep_common(image, nullptr, pose, nullptr, intrinsics, depths, trig, batch, height, width, num_depths, order, psv, 0,
                      psv_channels, channel_offset, stream);
}

int msi_ods_sphere_sweep_bf16(const float *image, const float *pose, const float *intrinsics,
                              const float *depths, const float *trig, int32_t batch,
                              int32_t height, int32_t width, int32_t num_depths, int32_t order,
                              void *psv_bf16, int32_t psv_channels, int32_t channel_offset,
                              msi_stream_t stream) {
  return sweep_common(image, nullptr, pose, nullptr, intrinsics, depths, trig, batch, height, width, num_depths, order, psv_bf16, 1,
                      psv_channels, channel_offset, stream);
}

int msi_ods_sweep_volume(const float *ref_image, const float *src_image, const float *ref_curr_pose,
                         const float *src_curr_pose, const float *intrinsics, const float *depths, const float *trig,
                         int32_t batch, int32_t height, int32_t width, int32_t num_depths, void *psv, int32_t psv_is_bf16,
                         msi_stream_t stream) {
  MSI_REQUIRE(src_image, "ods_sweep_volume: null pointer");
  return sweep_common(ref_image, src_image, ref_curr_pose, src_curr_pose, intrinsics, depths, trig, batch, height, width,
                      num_depths, 1, psv, psv_is_bf16 != 0, 6 * num_depths, 0, stream);
}

}  // extern "C"
