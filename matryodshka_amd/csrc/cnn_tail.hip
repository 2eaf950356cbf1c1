// the fused tail (1x1 head + RGBA assembly), LayerNorm finish / apply, zero -- part of the K2 convolution path (see cnn.hip for the design notes, cnn_device.h for the shared pieces).
#include "cnn_device.h"

namespace {

// ---- fused tail: 1x1 head (+ the producer's LayerNorm) + RGBA layer assembly ------------------------------------
// color_pred (nets.py:509-515) followed by infer_msi's layer_prediction for blend_psv (msi.py:130-147) in ONE kernel:
// `pred` (52 MB at the BASELINE size) is never written to or re-read from HBM and one launch disappears.  A workgroup
// owns 32 consecutive pixels: the sweep-volume tile (32 x 6D floats, contiguous) is requested first and stays in
// flight while the 32 x C0 activations (conv8_2 raw, normalised + ReLU'd on the way like the stand-alone head does)
// and the 2D x C0 weights go to LDS and 2 D / 32 waves run the k-steps on the fp32 MFMA -- the SAME instruction
// sequence as the stand-alone head (k ascending, transposed accumulators), so the prediction is bit-identical --
// then bias + tanh + (x+1)/2 land in an LDS tile and the assembly of K3 (geo_layers.hip, same expressions, no
// contraction) writes float4 texels of the D-major stack.  HBM-bound: reads C0 + 6D floats, writes 4D per pixel.

// A workgroup owns 32 pixels x lg layers (layer group g = blockIdx.y: blend weights g lg .. + lg, the alphas behind
// them, and the foreground / background colours of those layers: two runs of 3 lg channels of the sweep volume).
// Locally everything is a D = lg problem: output column n < lg is blend weight g lg + n, column lg + n its alpha.
// D <= 32: one group (the whole row is one run).  D = 64: two groups; the 32 x C0 activations are read by both
// (8 KB of 65 KB per workgroup), each keeps the 34 KB LDS footprint = four workgroups per CU (one 64-layer workgroup
// needed 66 KB: two per CU, 1.6 TB/s).
// BF16IN (bf16 plans): the sweep volume is bf16 (widened exactly on the way into LDS) and the normalised activation is
// rounded to bf16 (round to nearest even, where ln_apply_kernel<1> rounds it) before it enters the fp32 MFMA with the
// bf16-rounded weights: the operands of the bf16 head, exact products, fp32 accumulation.
// FMT (a constant of the including kernel, see head_assemble_packed_kernel): MSI_LAYERS_F32 writes the fp32 stack p.rgba, as ever.
// MSI_LAYERS_RGBA8 / MSI_LAYERS_RGBA16F write the texel to p.layers in that format -- the encoders of msi_pack_layers on the same fp32
// o.x .. o.w, so the packed stack is bit-identical to msi_pack_layers of the fp32 one -- and the fp32 stack only when p.rgba is not
// null.  A thread stores its 4 / 8 bytes direct: the 32 pixels of a tile are one aligned 128- / 256-byte run of a layer row, a wave
// writes two such rows (its two layers) per store instruction, and no LDS is spent on a transpose (LDS is what bounds the occupancy).
// The fp32 form: what msi_net_plan_forward_rgba launches (head_assemble_kernel<0> / <1> in a kernel trace).
template <int BF16IN>
__global__ void __launch_bounds__(256) __attribute__((amdgpu_waves_per_eu(BF16IN ? 6 : 5)))
head_assemble_kernel(const HeadAsmParams p) {
  [[maybe_unused]] constexpr int FMT = MSI_LAYERS_F32;
#include "cnn_tail_head_assemble.inc"
}

// The packed forms (msi_net_plan_forward_layers with a layers_out): the same body storing rgba8 / rgba16f texels, the fp32 stack optional.
template <int BF16IN, int FMT>
__global__ void __launch_bounds__(256) __attribute__((amdgpu_waves_per_eu(BF16IN ? 6 : 5)))
head_assemble_packed_kernel(const HeadAsmParams p) {
  static_assert(FMT == MSI_LAYERS_RGBA8 || FMT == MSI_LAYERS_RGBA16F, "a packed texel format");
#include "cnn_tail_head_assemble.inc"
}

// The affine of one layer's LayerNorm, scale | shift per channel, for consumers that apply it themselves while loading
// (head_assemble_kernel): one workgroup per sample.
__global__ void __launch_bounds__(256)
ln_finish_kernel(const long long *__restrict__ sums, double inv_n, const double *__restrict__ scl, int *status,
                 const float *__restrict__ gamma, const float *__restrict__ beta, int C, float *__restrict__ aff, int raw16) {
  __shared__ double s_stat[2];
  const int b = blockIdx.x, tid = threadIdx.x;
  ln_mean_inv(sums + (size_t)b * LN_SHARDS * LN_WORDS, inv_n, scl, status, s_stat, tid);
  const double mu = s_stat[0], inv = s_stat[1];
  const double up = raw16 ? scl[2] * 16777216.0 : 1.0;   // 2^e: the consumer reads the raw output as fp16 of x * 2^-e
  for (int c = tid; c < C; c += 256) {
    const double sc = inv * (double)gamma[c];
    aff[(size_t)b * 2 * C + c] = (float)(sc * up);
    aff[(size_t)b * 2 * C + C + c] = (float)((double)beta[c] - mu * sc);
  }
}

// LayerNorm apply (+ ReLU), one launch per layer.  Every workgroup derives the affine of slim.layer_norm,
//   scale = gamma * rsqrt(var + eps), shift = beta - mean * scale,
// from the sample's 64 x 2 fixed-point sums (ln_mean_inv), keeps it in LDS, and applies
// x = max(x*scale[c] + shift[c], 0) to its grid-stride slice (nets.py:401,485 arg_scope: normalizer, then the
// default ReLU).  Workgroup 0 also publishes the affine (tests).
// BF16OUT = 1: the normalised activation is written as bf16 to `yb` (the operand buffer of the bf16 path)
// and the fp32 raw output is left alone; 0: x is normalised in place.
// tickets and LayerNorm sums of one forward start from zero
__global__ void __launch_bounds__(256) zero_kernel(float4 *__restrict__ p, size_t n16) {
  const size_t i = (size_t)blockIdx.x * 256 + threadIdx.x;
  if (i < n16) p[i] = float4{0.f, 0.f, 0.f, 0.f};
}

template <int BF16OUT>
__global__ void __launch_bounds__(256)
ln_apply_kernel(float *__restrict__ x, const long long *__restrict__ sums, double inv_n, const double *__restrict__ scl,
                int *status, const float *__restrict__ gamma, const float *__restrict__ beta, size_t per_sample, int C,
                float *__restrict__ aff, unsigned short *__restrict__ yb) {
  extern __shared__ __attribute__((aligned(16))) float s_aff[];  // scale[C] shift[C]
  __shared__ double s_stat[2];
  const int b = blockIdx.y, tid = threadIdx.x;
  ln_mean_inv(sums + (size_t)b * LN_SHARDS * LN_WORDS, inv_n, scl, (blockIdx.x == 0 ? status : nullptr), s_stat, tid);
  const double mu = s_stat[0], inv = s_stat[1];
  // BF16OUT: the raw output is fp16 of x * 2^-e (emit_tile_impl RAW16): the scale applied to it carries 2^e (exact)
  const double up = BF16OUT ? scl[2] * 16777216.0 : 1.0;
  for (int c = tid; c < C; c += 256) {
    const double sc = inv * (double)gamma[c];
    const float fs = (float)sc, ft = (float)((double)beta[c] - mu * sc);
    s_aff[c] = BF16OUT ? (float)(sc * up) : fs;
    s_aff[C + c] = ft;
    if (blockIdx.x == 0) {      // (published for the tests: the affine of the UNSCALED raw output)
      aff[(size_t)b * 2 * C + c] = fs;
      aff[(size_t)b * 2 * C + C + c] = ft;
    }
  }
  __syncthreads();

  typedef _Float16 h4_t __attribute__((ext_vector_type(4)));
  const h4_t *xh = reinterpret_cast<const h4_t *>(reinterpret_cast<const _Float16 *>(x) + (size_t)b * per_sample);
  v4f *xv = reinterpret_cast<v4f *>(x + (size_t)b * per_sample);
  auto get = [&](size_t i) __attribute__((always_inline)) -> v4f {
    if (BF16OUT == 1) { const h4_t h = xh[i]; return v4f{(float)h.x, (float)h.y, (float)h.z, (float)h.w}; }
    return xv[i];
  };
  const size_t nvec = per_sample / 4;
  const size_t stride = (size_t)gridDim.x * blockDim.x;
  auto apply = [](v4f v, const v4f s4, const v4f t4) __attribute__((always_inline)) -> v4f {
    v.x = fmaxf(v.x * s4.x + t4.x, 0.f);
    v.y = fmaxf(v.y * s4.y + t4.y, 0.f);
    v.z = fmaxf(v.z * s4.z + t4.z, 0.f);
    v.w = fmaxf(v.w * s4.w + t4.w, 0.f);
    return v;
  };
  // fp32 -> bf16, round to nearest even (finite inputs: the LayerNorm output)
  auto bf16_bits = [](float f) __attribute__((always_inline)) -> unsigned {
    const unsigned u = __builtin_bit_cast(unsigned, f);
    return (u + 0x7fffu + ((u >> 16) & 1u)) >> 16;
  };
  typedef unsigned v2u __attribute__((ext_vector_type(2)));
  v2u *yv = reinterpret_cast<v2u *>(yb + (size_t)b * per_sample);
  auto put = [&](size_t i, const v4f v) __attribute__((always_inline)) {
    if (BF16OUT == 1) yv[i] = v2u{bf16_bits(v.x) | (bf16_bits(v.y) << 16), bf16_bits(v.z) | (bf16_bits(v.w) << 16)};
    else xv[i] = v;
  };
  if ((256 * 4) % C == 0) {
    // every grid-stride step advances a thread by a multiple of C floats: its four channels are fixed
    const int c = (tid * 4) % C;
    const v4f s4 = *reinterpret_cast<const v4f *>(s_aff + c);
    const v4f t4 = *reinterpret_cast<const v4f *>(s_aff + C + c);
    for (size_t i = (size_t)blockIdx.x * blockDim.x + tid; i < nvec; i += stride) put(i, apply(get(i), s4, t4));
  } else {
    for (size_t i = (size_t)blockIdx.x * blockDim.x + tid; i < nvec; i += stride) {
      const int c = (int)((i * 4) % C);
      put(i, apply(get(i), *reinterpret_cast<const v4f *>(s_aff + c), *reinterpret_cast<const v4f *>(s_aff + C + c)));
    }
  }
}

}  // namespace

namespace msi_cnn {
int launch_zero(void *ptr, size_t n16, hipStream_t stream) {
  hipLaunchKernelGGL(zero_kernel, dim3((unsigned)((n16 + 255) / 256)), dim3(256), 0, stream, reinterpret_cast<float4 *>(ptr), n16);
  return msi::check_launch("zero");
}
int launch_ln_finish(int batch, hipStream_t stream, const long long *sums, double inv_n, const double *scl, int *status, const float *gamma, const float *beta, int C,
                     float *aff, int raw16) {
  hipLaunchKernelGGL(ln_finish_kernel, dim3(batch), dim3(256), 0, stream, sums, inv_n, scl, status, gamma, beta, C, aff, raw16);
  return msi::check_launch("ln_finish");
}
int launch_ln_apply(int bf16out, unsigned blocks, int batch, size_t lds, hipStream_t stream, float *x, const long long *sums, double inv_n, const double *scl, int *status,
                    const float *gamma, const float *beta, size_t per_sample, int C, float *aff, unsigned short *yb) {
  const dim3 grid(blocks, batch);
  if (bf16out) hipLaunchKernelGGL(ln_apply_kernel<1>, grid, dim3(256), lds, stream, x, sums, inv_n, scl, status, gamma, beta, per_sample, C, aff, yb);
  else hipLaunchKernelGGL(ln_apply_kernel<0>, grid, dim3(256), lds, stream, x, sums, inv_n, scl, status, gamma, beta, per_sample, C, aff, yb);
  return msi::check_launch("ln_apply");
}
int launch_head_assemble(int bf16in, int format, unsigned grid_x, size_t lds, hipStream_t stream, const HeadAsmParams &q) {
#define MSI_LAUNCH_HA(K) hipLaunchKernelGGL(K, dim3(grid_x), dim3(256), lds, stream, q)
  switch (format) {
    case MSI_LAYERS_F32:
      if (bf16in) MSI_LAUNCH_HA(head_assemble_kernel<1>); else MSI_LAUNCH_HA(head_assemble_kernel<0>);
      break;
    case MSI_LAYERS_RGBA8:
      if (bf16in) MSI_LAUNCH_HA((head_assemble_packed_kernel<1, MSI_LAYERS_RGBA8>)); else MSI_LAUNCH_HA((head_assemble_packed_kernel<0, MSI_LAYERS_RGBA8>));
      break;
    case MSI_LAYERS_RGBA16F:
      if (bf16in) MSI_LAUNCH_HA((head_assemble_packed_kernel<1, MSI_LAYERS_RGBA16F>)); else MSI_LAUNCH_HA((head_assemble_packed_kernel<0, MSI_LAYERS_RGBA16F>));
      break;
    default:
      return msi::fail(MSI_E_BADARG, "head_assemble: unknown format %d", format);
  }
#undef MSI_LAUNCH_HA
  return msi::check_launch("head_assemble");
}
}  // namespace msi_cnn
