// The layer stack of the geometry side: K3 RGBA assembly, the bilinear resize, the fused high-res stack (hres_layers_kernel: sweep + resize +
// assembly in one pass, through the sweep's device functions of geometry_device.h) and pack / unpack of the compact formats; kernels first,
// their C ABI entry points below.
#include "geometry_device.h"

// (the tuning macros of hres_layers_kernel, MSI_HRES_GROUP and MSI_HRES_WAVES: geometry_device.h, with the texel that geo_sparse_hres.hip shares)

namespace {

// ------------------------------------------------------------------------ K3
// A block owns TP=32 consecutive pixels.  Phase 1 streams the contiguous PSV
// (32 x 6D floats) and pred (32 x 2D floats) tiles into LDS with 16-byte loads;
// phase 2 re-reads them transposed (row stride padded to an odd dword count, so
// the 32 lanes of a half-wave hit 32 different banks) and writes float4 texels
// of the D-major stack: 512 contiguous bytes per (half-wave, layer).
constexpr int K3_TP = 32;

// PSV_BF16: the PSV is the bf16 network input (converted to fp32 on its way into LDS).
// COLOR: which_color_pred of infer_msi (msi.py:119-275):
//   0 blend_psv    pred = [w | alpha]              rgb = w fg + (1-w) bg_psv                       (msi.py:130-147)
//   1 blend_bg     pred = [w | alpha | bg(3)]      rgb = w fg + (1-w) bg      (bg: raw tanh output, msi.py:177-188)
//   2 blend_bg_psv pred = [w | alpha | bw | bg(3)] rgb = bw (w fg + (1-w) bg_psv) + (1-bw) bg      (msi.py:223-242)
//   3 alpha_only   pred = [alpha]                  rgb = fg                                        (msi.py:258-268)
// with w, alpha, bw = (x + 1) / 2.  The channel counts of 1 and 2 are odd, so those modes place pred element
// by element (the 32-pixel tile is still one contiguous, 16-byte aligned run) and write the optional
// [B,H,W,D] outputs from phase 2.
enum { COLOR_BLEND_PSV = 0, COLOR_BLEND_BG = 1, COLOR_BLEND_BG_PSV = 2, COLOR_ALPHA_ONLY = 3 };

template <int PSV_BF16, int COLOR>
__global__ void __launch_bounds__(256)
assemble_kernel(const void *__restrict__ psv_, const float *__restrict__ pred,
                float4 *__restrict__ rgba, float *__restrict__ bw_out,
                float *__restrict__ al_out, float *__restrict__ bgw_out, long npix_total, int hw, int nd, int pred_scaled) {
  extern __shared__ __attribute__((aligned(16))) float smem[];
  const int c_psv = 6 * nd;
  const int c_pred = COLOR == COLOR_BLEND_PSV ? 2 * nd : (COLOR == COLOR_BLEND_BG ? 2 * nd + 3 : (COLOR == COLOR_BLEND_BG_PSV ? 3 * nd + 3 : nd));
  const int s_psv = c_psv + 1, s_pred = c_pred | 1;  // odd row strides
  float *l_psv = smem;
  float *l_pred = smem + K3_TP * s_psv;

  const long p0 = (long)blockIdx.x * K3_TP;
  const int npx = (int)((npix_total - p0) < K3_TP ? (npix_total - p0) : K3_TP);
  const int tid = threadIdx.x;

  if (PSV_BF16) {
    const uint4 *g = reinterpret_cast<const uint4 *>(static_cast<const unsigned short *>(psv_) + p0 * c_psv);
    const int nv = npx * c_psv / 8;
    for (int v = tid; v < nv; v += 256) {
      const uint4 q = g[v];
      const int e = v * 8;
      const int row = e / c_psv, col = e - row * c_psv;  // c_psv % 8 == 0 (D % 4 == 0): no row straddle
      float *dst = l_psv + row * s_psv + col;
      const unsigned w[4] = {q.x, q.y, q.z, q.w};
#pragma unroll
      for (int k = 0; k < 4; ++k) {
        dst[2 * k] = bf16_to_f32((unsigned short)(w[k] & 0xffffu));
        dst[2 * k + 1] = bf16_to_f32((unsigned short)(w[k] >> 16));
      }
    }
  } else {
    const float4 *g = reinterpret_cast<const float4 *>(static_cast<const float *>(psv_) + p0 * c_psv);
    const int nv = npx * c_psv / 4;
    for (int v = tid; v < nv; v += 256) {
      const float4 q = g[v];
      const int e = v * 4;
      const int row = e / c_psv, col = e - row * c_psv;  // c_psv % 4 == 0: no row straddle
      float *dst = l_psv + row * s_psv + col;
      dst[0] = q.x; dst[1] = q.y; dst[2] = q.z; dst[3] = q.w;
    }
  }
  if (COLOR == COLOR_BLEND_PSV) {
    const float4 *g = reinterpret_cast<const float4 *>(pred + p0 * c_pred);
    const int nv = npx * c_pred / 4;
    for (int v = tid; v < nv; v += 256) {
      float4 q = g[v];
      if (!pred_scaled) {  // (x + 1) / 2 (msi.py:132-133); already applied on the high-res path
        q.x = (q.x + 1.0f) / 2.0f; q.y = (q.y + 1.0f) / 2.0f;
        q.z = (q.z + 1.0f) / 2.0f; q.w = (q.w + 1.0f) / 2.0f;
      }
      const int e = v * 4;
      const int row = e / c_pred, col = e - row * c_pred;
      float *dst = l_pred + row * s_pred + col;
      dst[0] = q.x; dst[1] = q.y; dst[2] = q.z; dst[3] = q.w;
      // optional extra outputs, [B,H,W,D] each (msi.py:281-287)
      if (col < nd) {
        if (bw_out) *reinterpret_cast<float4 *>(bw_out + (p0 + row) * nd + col) = q;
      } else {
        if (al_out) *reinterpret_cast<float4 *>(al_out + (p0 + row) * nd + (col - nd)) = q;
      }
    }
  } else {
    const float *g = pred + p0 * c_pred;
    const int n = npx * c_pred;
    const int nscaled = c_pred - ((COLOR == COLOR_BLEND_BG || COLOR == COLOR_BLEND_BG_PSV) ? 3 : 0);  // bg stays in [-1, 1]
    for (int e = tid; e < n; e += 256) {
      const int row = e / c_pred, col = e - row * c_pred;
      float x = g[e];
      if (col < nscaled) x = (x + 1.0f) / 2.0f;
      l_pred[row * s_pred + col] = x;
    }
  }
  __syncthreads();

  const int px = tid & (K3_TP - 1);
  if (px >= npx) return;
  const long p = p0 + px;
  const long b = p / hw;
  const long off = p - b * hw;
  const float *rp = l_psv + px * s_psv;
  const float *rq = l_pred + px * s_pred;
  for (int d = tid / K3_TP; d < nd; d += 256 / K3_TP) {
    const float *fg = rp + d * 3;
    const float *bg = rp + (nd + d) * 3;
    float4 o;
    if (COLOR == COLOR_BLEND_PSV) {
      const float w = rq[d];
      const float omw = 1.0f - w;
      o.x = w * fg[0] + omw * bg[0];
      o.y = w * fg[1] + omw * bg[1];
      o.z = w * fg[2] + omw * bg[2];
      o.w = rq[nd + d];
    } else if (COLOR == COLOR_BLEND_BG) {
      const float w = rq[d];
      const float omw = 1.0f - w;
      const float *pb = rq + 2 * nd;
      o.x = w * fg[0] + omw * pb[0];
      o.y = w * fg[1] + omw * pb[1];
      o.z = w * fg[2] + omw * pb[2];
      o.w = rq[nd + d];
      if (bw_out) bw_out[p * nd + d] = w;
      if (al_out) al_out[p * nd + d] = o.w;
    } else if (COLOR == COLOR_BLEND_BG_PSV) {
      const float w = rq[d], bw = rq[2 * nd + d];
      const float omw = 1.0f - w, ombw = 1.0f - bw;
      const float *pb = rq + 3 * nd;
      o.x = bw * (w * fg[0] + omw * bg[0]) + ombw * pb[0];
      o.y = bw * (w * fg[1] + omw * bg[1]) + ombw * pb[1];
      o.z = bw * (w * fg[2] + omw * bg[2]) + ombw * pb[2];
      o.w = rq[nd + d];
      if (bw_out) bw_out[p * nd + d] = w;
      if (al_out) al_out[p * nd + d] = o.w;
      if (bgw_out) bgw_out[p * nd + d] = bw;
    } else {
      o.x = fg[0]; o.y = fg[1]; o.z = fg[2];
      o.w = rq[d];
      if (al_out) al_out[p * nd + d] = o.w;
    }
    rgba[(b * nd + d) * hw + off] = o;
  }
}

// msi_pack_layers / msi_unpack_layers: streaming conversions of the native stack, 16-byte loads and stores on both sides.  One
// thread takes the texels of one 16-byte piece of the packed stack -- four rgba8 texels (four float4 loads, one store) or two
// rgba16f texels -- and the < 4 texels that do not fill a piece go one at a time through the first threads of the grid.
// NT = 1 (the host picks it when the destination is larger than the 256-MiB Infinity Cache): non-temporal stores, as in the sweep
// (a template argument: behind a runtime flag hipcc merges the two stores into one plain store).
// The encoders (rgba8_encode, rgba16f_encode) are in msi_common.h.
template <int FMT, int NT>
__global__ void __launch_bounds__(256)
pack_layers_kernel(const float4 *__restrict__ in, void *__restrict__ out, size_t texels) {
  constexpr int TPP = FMT == MSI_LAYERS_RGBA8 ? 4 : 2;   // texels per 16-byte piece
  const size_t pieces = texels / TPP;
  const size_t tid = (size_t)blockIdx.x * blockDim.x + threadIdx.x, stride = (size_t)gridDim.x * blockDim.x;
  for (size_t p = tid; p < pieces; p += stride) {
    float4 t[TPP];
#pragma unroll
    for (int k = 0; k < TPP; ++k) t[k] = in[p * TPP + k];
    uint4 v;
    if constexpr (FMT == MSI_LAYERS_RGBA8) {
      v.x = rgba8_encode(t[0]); v.y = rgba8_encode(t[1]); v.z = rgba8_encode(t[2]); v.w = rgba8_encode(t[3]);
    } else {
      const u32x2_g lo = rgba16f_encode(t[0]), hi = rgba16f_encode(t[1]);
      v.x = lo.x; v.y = lo.y; v.z = hi.x; v.w = hi.y;
    }
    sweep_store16(static_cast<uint4 *>(out) + p, v, NT);
  }
  const size_t tail = pieces * TPP + tid;
  if (tid < (size_t)TPP && tail < texels) {
    if (FMT == MSI_LAYERS_RGBA8) static_cast<unsigned *>(out)[tail] = rgba8_encode(in[tail]);
    else static_cast<u32x2_g *>(out)[tail] = rgba16f_encode(in[tail]);
  }
}

template <int FMT, int NT>
__global__ void __launch_bounds__(256)
unpack_layers_kernel(const void *__restrict__ in, float4 *__restrict__ out, size_t texels) {
  constexpr int TPP = FMT == MSI_LAYERS_RGBA8 ? 4 : 2;
  const size_t pieces = texels / TPP;
  const size_t tid = (size_t)blockIdx.x * blockDim.x + threadIdx.x, stride = (size_t)gridDim.x * blockDim.x;
  for (size_t p = tid; p < pieces; p += stride) {
    const uint4 v = static_cast<const uint4 *>(in)[p];
    float4 t[TPP];
    if constexpr (FMT == MSI_LAYERS_RGBA8) {
      t[0] = rgba8_decode(v.x); t[1] = rgba8_decode(v.y); t[2] = rgba8_decode(v.z); t[3] = rgba8_decode(v.w);
    } else {
      u32x2_g lo, hi;
      lo.x = v.x; lo.y = v.y; hi.x = v.z; hi.y = v.w;
      t[0] = rgba16f_decode(lo); t[1] = rgba16f_decode(hi);
    }
#pragma unroll
    for (int k = 0; k < TPP; ++k) sweep_store16(reinterpret_cast<uint4 *>(out + p * TPP + k), __builtin_bit_cast(uint4, t[k]), NT);
  }
  const size_t tail = pieces * TPP + tid;
  if (tid < (size_t)TPP && tail < texels) {
    if (FMT == MSI_LAYERS_RGBA8) out[tail] = rgba8_decode(static_cast<const unsigned *>(in)[tail]);
    else out[tail] = rgba16f_decode(static_cast<const u32x2_g *>(in)[tail]);
  }
}

// tf.image.resize(..., BILINEAR, align_corners=True): the expression is lerp2 of geometry_device.h, per component.
__global__ void resize_bilinear_kernel(const float4 *__restrict__ in, float4 *__restrict__ out, size_t n,
                                       int in_h, int in_w, int c4, int out_h, int out_w, float sy, float sx) {
  size_t idx = (size_t)blockIdx.x * blockDim.x + threadIdx.x;
  const size_t stride = (size_t)gridDim.x * blockDim.x;
  for (; idx < n; idx += stride) {
    const int c = (int)(idx % c4);
    size_t r = idx / c4;
    const int x = (int)(r % out_w);
    r /= out_w;
    const int y = (int)(r % out_h);
    const size_t b = r / out_h;
    const float fy = (float)y * sy, fx = (float)x * sx;
    const int y0 = (int)floorf(fy), x0 = (int)floorf(fx);
    const int y1 = min((int)ceilf(fy), in_h - 1), x1 = min((int)ceilf(fx), in_w - 1);
    const float yl = fy - (float)y0, xl = fx - (float)x0;
    const float4 *base = in + b * (size_t)in_h * in_w * c4;
    const float4 tl = base[((size_t)y0 * in_w + x0) * c4 + c], tr = base[((size_t)y0 * in_w + x1) * c4 + c];
    const float4 bl = base[((size_t)y1 * in_w + x0) * c4 + c], br = base[((size_t)y1 * in_w + x1) * c4 + c];
    float4 o;
    o.x = lerp2(tl.x, tr.x, bl.x, br.x, xl, yl); o.y = lerp2(tl.y, tr.y, bl.y, br.y, xl, yl);
    o.z = lerp2(tl.z, tr.z, bl.z, br.z, xl, yl); o.w = lerp2(tl.w, tr.w, bl.w, br.w, xl, yl);
    out[idx] = o;
  }
}

// ---- msi_hres_layers: the high-res layer stack of test.py:283-394 in ONE pass -----------------------------------------------
// A texel of that stack is a function of two image gathers (the ODS sweep samples of the ref / src image), eight low-res taps (the
// bilinear resize of its blend weight and alpha) and one blend; the three-launch form (ods_sweep_kernel<float, NS, 2, 0> ->
// resize_bilinear_kernel -> assemble_kernel<0, COLOR_BLEND_PSV>) writes and re-reads a [B,Hh,Wh,6D] volume and a [B,Hh,Wh,2D] tensor
// to get there.  This kernel calls the SAME device functions (ods_quad, ods_tail, make_taps_bytes, gather3 / blend4), the resize's
// expressions and the assembly's blend in the same order -- the file is compiled without contraction, so every texel has the bits of
// the three launches -- and stores it as 16 (fp32), 8 (rgba16f) or 4 (rgba8) bytes, or as fp32 and one packed format at once.
// Mapping: the output is D-major, so unlike the sweep (depth in the fastest lanes, NHWC) a lane is one PIXEL of a 256-column run of
// row blockIdx.y and walks the layers: trigonometry, the resize corners and the pose comparison are per-pixel work done once, each
// layer's store is one contiguous run per wave (64 x 16 / 8 / 4 bytes; a lane's fp32 texel is one 16-byte piece), and neighbouring
// lanes gather neighbouring texels of the images.  Weights and alphas are [B,h,w,D] (layer fastest): one float4 per corner covers
// four layers, so the eight taps of a texel cost two 16-byte loads; a row of blocks shares two low-res rows, which stay in L1 / L2.
// FMT: MSI_LAYERS_F32 (no packed output), MSI_LAYERS_RGBA8 or MSI_LAYERS_RGBA16F; WITH_F32: the fp32 stack is written (too);
// NT: bit 0 / bit 1 = non-temporal stores of the fp32 / the packed stack (the host sets a bit when that destination is larger
// than the 256-MiB Infinity Cache; a template argument, as in pack_layers_kernel).
// The texel (OdsHres, hres_texel) is in geometry_device.h: the PP and cube builders run this loop, restated, on their sources, and
// hres_layers_sparse_kernel (geo_sparse_hres.hip) writes the same texels into a pool of kept tiles.
template <int FMT, int WITH_F32, int NT>
// (waves_per_eu with the maximum at MSI_HRES_WAVES too: with the texel in shared device functions the allocator settles at 93-95 VGPRs, which
// would run five waves, and at five the launch is 5 % slower at 1280x640 -- same-process A/B in profiles/hres_sparse_isa.txt)
__global__ void __launch_bounds__(256) __attribute__((amdgpu_waves_per_eu(MSI_HRES_WAVES, MSI_HRES_WAVES)))
hres_layers_kernel(const float *__restrict__ image0, const float *__restrict__ image1, const float *__restrict__ pose0,
                   const float *__restrict__ pose1, const float *__restrict__ intrinsics, const float *__restrict__ depths,
                   const float *__restrict__ trig, const float *__restrict__ blend_weights, const float *__restrict__ alphas,
                   int low_h, int low_w, int height, int width, int nd, float sy, float sx, PixConsts K,
                   float4 *__restrict__ rgba, void *__restrict__ packed) {
  // grid = (ceil(W / 256), H, B): one thread per pixel, all layers
  const int j = blockIdx.x * 256 + threadIdx.x;
  if (j >= width) return;
  const int i = blockIdx.y, b = blockIdx.z;
  const OdsHres px = ods_hres(image0, image1, pose0, pose1, intrinsics, trig, K, b, i, j, height, width);
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

}  // namespace

extern "C" {

static int assemble_common(const void *psv, int psv_bf16, const float *pred, int color, float *rgba_native,
                           float *blend_weights, float *alphas, float *bg_blend_weights, int32_t batch, int32_t height,
                           int32_t width, int32_t num_planes, int pred_scaled, msi_stream_t stream) {
  MSI_REQUIRE(psv && pred && rgba_native, "assemble_rgba: null pointer");
  MSI_REQUIRE(batch >= 0 && height > 0 && width > 0 && num_planes > 0, "assemble_rgba: bad dims");
  MSI_REQUIRE(color >= COLOR_BLEND_PSV && color <= COLOR_ALPHA_ONLY, "assemble_rgba: which_color_pred %d", color);
  if (num_planes % 4 != 0)
    return msi::fail(MSI_E_UNSUPPORTED, "assemble_rgba: num_planes=%d must be a multiple of 4",
                     num_planes);
  const int c_pred = color == COLOR_BLEND_PSV ? 2 * num_planes : (color == COLOR_BLEND_BG ? 2 * num_planes + 3
                     : (color == COLOR_BLEND_BG_PSV ? 3 * num_planes + 3 : num_planes));
  const size_t lds = (size_t)K3_TP * ((6 * num_planes + 1) + (c_pred | 1)) * sizeof(float);
  if (lds > 160 * 1024)
    return msi::fail(MSI_E_UNSUPPORTED, "assemble_rgba: num_planes=%d needs %zu B of LDS", num_planes,
                     lds);
  const long npix = (long)batch * height * width;
  if (npix == 0) return MSI_OK;
  const long blocks = (npix + K3_TP - 1) / K3_TP;
  typedef void (*kern_t)(const void *, const float *, float4 *, float *, float *, float *, long, int, int, int);
  static const kern_t table[2][4] = {
      {assemble_kernel<0, 0>, assemble_kernel<0, 1>, assemble_kernel<0, 2>, assemble_kernel<0, 3>},
      {assemble_kernel<1, 0>, assemble_kernel<1, 1>, assemble_kernel<1, 2>, assemble_kernel<1, 3>}};
  const kern_t kern = table[psv_bf16 ? 1 : 0][color];
  if (lds > 64 * 1024) {
    hipError_t e = hipFuncSetAttribute(reinterpret_cast<const void *>(kern), hipFuncAttributeMaxDynamicSharedMemorySize, (int)lds);
    if (e != hipSuccess) return msi::fail(MSI_E_LAUNCH, "assemble_rgba: %s", hipGetErrorString(e));
  }
  hipLaunchKernelGGL(kern, dim3((unsigned)blocks), dim3(256), lds, msi::as_stream(stream), psv, pred,
                     reinterpret_cast<float4 *>(rgba_native), blend_weights, alphas, bg_blend_weights, npix,
                     height * width, num_planes, pred_scaled);
  return msi::check_launch("assemble_rgba");
}

int msi_assemble_rgba_f32(const float *psv, const float *pred, float *rgba_native,
                          float *blend_weights, float *alphas, int32_t batch, int32_t height,
                          int32_t width, int32_t num_planes, msi_stream_t stream) {
  return assemble_common(psv, 0, pred, COLOR_BLEND_PSV, rgba_native, blend_weights, alphas, nullptr, batch, height, width,
                         num_planes, 0, stream);
}

int msi_assemble_rgba_bf16psv_f32(const void *psv_bf16, const float *pred, float *rgba_native,
                                  float *blend_weights, float *alphas, int32_t batch, int32_t height,
                                  int32_t width, int32_t num_planes, msi_stream_t stream) {
  return assemble_common(psv_bf16, 1, pred, COLOR_BLEND_PSV, rgba_native, blend_weights, alphas, nullptr, batch, height,
                         width, num_planes, 0, stream);
}

int msi_assemble_rgba_color_f32(const void *psv, int32_t psv_is_bf16, const float *pred, int32_t which_color_pred,
                                float *rgba_native, float *blend_weights, float *alphas, float *bg_blend_weights,
                                int32_t batch, int32_t height, int32_t width, int32_t num_planes, msi_stream_t stream) {
  return assemble_common(psv, psv_is_bf16 != 0, pred, which_color_pred, rgba_native, blend_weights, alphas,
                         bg_blend_weights, batch, height, width, num_planes, 0, stream);
}

int msi_assemble_rgba_scaled_f32(const float *psv, const float *weights_alphas, float *rgba_native,
                                 int32_t batch, int32_t height, int32_t width, int32_t num_planes,
                                 msi_stream_t stream) {
  return assemble_common(psv, 0, weights_alphas, COLOR_BLEND_PSV, rgba_native, nullptr, nullptr, nullptr, batch, height,
                         width, num_planes, 1, stream);
}

int msi_resize_bilinear_f32(const float *in, float *out, int32_t batch, int32_t in_h, int32_t in_w,
                            int32_t channels, int32_t out_h, int32_t out_w, msi_stream_t stream) {
  MSI_REQUIRE(in && out, "resize_bilinear: null pointer");
  MSI_REQUIRE(batch >= 0 && in_h > 0 && in_w > 0 && channels > 0 && out_h > 0 && out_w > 0, "resize_bilinear: bad dims");
  if (channels % 4 != 0)
    return msi::fail(MSI_E_UNSUPPORTED, "resize_bilinear: channels=%d must be a multiple of 4", channels);
  const size_t n = (size_t)batch * out_h * out_w * (channels / 4);
  if (n == 0) return MSI_OK;
  const float sy = out_h > 1 ? (float)(in_h - 1) / (float)(out_h - 1) : 0.0f;
  const float sx = out_w > 1 ? (float)(in_w - 1) / (float)(out_w - 1) : 0.0f;
  hipLaunchKernelGGL(resize_bilinear_kernel, dim3(grid_1d(n)), dim3(256), 0, msi::as_stream(stream),
                     reinterpret_cast<const float4 *>(in), reinterpret_cast<float4 *>(out), n, in_h, in_w,
                     channels / 4, out_h, out_w, sy, sx);
  return msi::check_launch("resize_bilinear");
}

int msi_hres_layers(const float *ref_image, const float *src_image, const float *ref_curr_pose, const float *src_curr_pose,
                    const float *intrinsics, const float *depths, const float *trig, const float *blend_weights,
                    const float *alphas, int32_t batch, int32_t low_height, int32_t low_width, int32_t height, int32_t width,
                    int32_t num_planes, float *rgba_native, void *layers_out, int32_t format, msi_stream_t stream) {
  MSI_REQUIRE(!layers_out || format == MSI_LAYERS_RGBA8 || format == MSI_LAYERS_RGBA16F, "hres_layers: unknown format %d", format);
  MSI_REQUIRE(rgba_native || layers_out, "hres_layers: null pointer (both outputs are NULL)");
  if (const int e = hres_check("hres_layers", ref_image && src_image && ref_curr_pose && src_curr_pose && intrinsics && depths && trig &&
                               blend_weights && alphas, batch, low_height, low_width, height, width, num_planes)) return e;
  if (batch == 0) return MSI_OK;
  const float sy = hres_scale(low_height, height), sx = hres_scale(low_width, width);
  const PixConsts K = make_consts(height, width);
  const dim3 grid((unsigned)((width + 255) / 256), height, batch);
  hipStream_t s = msi::as_stream(stream);
  hres_dense_launch(format, rgba_native, layers_out, (size_t)batch * num_planes * height * width, [&](auto FMT, auto F32, auto NT) {
    hipLaunchKernelGGL((hres_layers_kernel<decltype(FMT)::value, decltype(F32)::value, decltype(NT)::value>), grid, dim3(256), 0, s, ref_image,
                       src_image, ref_curr_pose, src_curr_pose, intrinsics, depths, trig, blend_weights, alphas, low_height, low_width, height, width,
                       num_planes, sy, sx, K, reinterpret_cast<float4 *>(rgba_native), layers_out);
  });
  return msi::check_launch("hres_layers");
}

// grid of the pack / unpack kernels: one thread per 16-byte piece of the packed stack (grid-stride beyond 2^20 workgroups)
static unsigned pack_grid(int64_t texels, int per_piece) {
  const int64_t pieces = texels / per_piece, blocks = (pieces + 255) / 256;
  return (unsigned)(blocks < 1 ? 1 : blocks > (1 << 20) ? (1 << 20) : blocks);
}

int msi_pack_layers(const float *rgba_native, int32_t format, void *packed, int64_t texels, msi_stream_t stream) {
  MSI_REQUIRE(rgba_native && packed, "pack_layers: null pointer");
  MSI_REQUIRE(format != MSI_LAYERS_F32, "pack_layers: MSI_LAYERS_F32 is the unpacked format (nothing to pack)");
  MSI_REQUIRE(format == MSI_LAYERS_RGBA8 || format == MSI_LAYERS_RGBA16F, "pack_layers: unknown format %d", format);
  MSI_REQUIRE(texels >= 0, "pack_layers: negative texel count");
  if (texels == 0) return MSI_OK;
  const float4 *in = reinterpret_cast<const float4 *>(rgba_native);
  hipStream_t s = msi::as_stream(stream);
  const bool nt = beyond_infinity_cache((size_t)texels * (format == MSI_LAYERS_RGBA8 ? 4 : 8));
#define MSI_LAUNCH_PACK(FMT, TPP, NT) \
  hipLaunchKernelGGL((pack_layers_kernel<FMT, NT>), dim3(pack_grid(texels, TPP)), dim3(256), 0, s, in, packed, (size_t)texels)
  if (format == MSI_LAYERS_RGBA8) {
    if (nt) MSI_LAUNCH_PACK(MSI_LAYERS_RGBA8, 4, 1); else MSI_LAUNCH_PACK(MSI_LAYERS_RGBA8, 4, 0);
  } else {
    if (nt) MSI_LAUNCH_PACK(MSI_LAYERS_RGBA16F, 2, 1); else MSI_LAUNCH_PACK(MSI_LAYERS_RGBA16F, 2, 0);
  }
#undef MSI_LAUNCH_PACK
  return msi::check_launch("pack_layers");
}

int msi_unpack_layers(const void *packed, int32_t format, float *rgba_native, int64_t texels, msi_stream_t stream) {
  MSI_REQUIRE(rgba_native && packed, "unpack_layers: null pointer");
  MSI_REQUIRE(format != MSI_LAYERS_F32, "unpack_layers: MSI_LAYERS_F32 is the unpacked format (nothing to unpack)");
  MSI_REQUIRE(format == MSI_LAYERS_RGBA8 || format == MSI_LAYERS_RGBA16F, "unpack_layers: unknown format %d", format);
  MSI_REQUIRE(texels >= 0, "unpack_layers: negative texel count");
  if (texels == 0) return MSI_OK;
  float4 *out = reinterpret_cast<float4 *>(rgba_native);
  hipStream_t s = msi::as_stream(stream);
  const bool nt = beyond_infinity_cache((size_t)texels * 16);
#define MSI_LAUNCH_UNPACK(FMT, TPP, NT) \
  hipLaunchKernelGGL((unpack_layers_kernel<FMT, NT>), dim3(pack_grid(texels, TPP)), dim3(256), 0, s, packed, out, (size_t)texels)
  if (format == MSI_LAYERS_RGBA8) {
    if (nt) MSI_LAUNCH_UNPACK(MSI_LAYERS_RGBA8, 4, 1); else MSI_LAUNCH_UNPACK(MSI_LAYERS_RGBA8, 4, 0);
  } else {
    if (nt) MSI_LAUNCH_UNPACK(MSI_LAYERS_RGBA16F, 2, 1); else MSI_LAUNCH_UNPACK(MSI_LAYERS_RGBA16F, 2, 0);
  }
#undef MSI_LAUNCH_UNPACK
  return msi::check_launch("unpack_layers");
}

}  // extern "C"
