// Image scores on the device (msi_score_images; eval.py:127-174 computed tf.image.ssim / tf.image.psnr with TensorFlow ops on the GPU): per pair of
// images MSE, PSNR, mean absolute difference and SSIM with tf.image.ssim semantics, optionally with one weight per image row.  fp64 throughout:
// matryodshka_amd/evaluate.py (fp64) is the metric of record, and SSIM's variances E[x^2] - mu^2 cancel values up to 65025 against c2 = 58.5.
//
// Two launches.  score_tiles_kernel: one workgroup per (pair, tile of 16 x 32 SSIM-map positions), channel by channel: the (16+10) x (32+10) patch of
// both images is staged into LDS as transformed doubles, the vertical 11-tap pass writes the five moments (x, y, x^2, y^2, xy) of 16 x 42 positions to
// LDS, the horizontal pass runs from there in registers, and the workgroup's sums (weighted squared error, absolute error, SSIM map) are reduced in a
// fixed order -- shuffle tree inside a wave, then wave 0..3 -- into ONE record of three doubles in the workspace.  Every image pixel is counted for the
// error sums by exactly one workgroup: a tile owns the first 16 rows / 32 columns of its patch, and the last tile of each direction owns the rest of it
// (which reaches the image edge: tiles = ceil((size - 10) / tile), so the last patch ends at or behind the last pixel).  score_finalize_kernel: one
// wave per pair adds the pair's records (lane l takes records l, l + 64, ... in index order, then the same shuffle tree), divides and takes the
// logarithm.  No atomics and nothing to zero: every record of the workspace is written before it is read, a pair's numbers depend on its own records
// only, and the order of every sum is fixed by the shapes -- results are bit-reproducible and independent of what else shares the launch.
//
// Built with -ffp-contract=off: the 8-bit quantisation below restates deprocess_kernel (geo_prep.hip) op for op, and the SSIM map of two identical
// images has to come out as exactly 1 (2 mu mu + c1 over mu^2 + mu^2 + c1).  The filter taps use explicit fma.
#include "msi_common.h"

#include <cmath>
#include <limits>

namespace {

constexpr int kTaps = 11;                    // tf.image.ssim: filter_size 11, sigma 1.5
constexpr int kHalo = kTaps - 1;
constexpr int kTileH = 16, kTileW = 32;      // SSIM-map positions per workgroup
constexpr int kPatchH = kTileH + kHalo, kPatchW = kTileW + kHalo;
constexpr int kThreads = 256;
constexpr int kRecord = 3;                   // doubles per workgroup record: weighted SSE, weighted SAD, weighted sum of the SSIM map

enum StageMode { STAGE_RAW = 0, STAGE_IMAGE = 1, STAGE_DEPTH = 2, STAGE_IMAGE_Q = 3, STAGE_DEPTH_Q = 4 };

struct ScoreTaps {
  double col[kTaps];   // vertical factors (rows of the window summed), as _filter_valid of evaluate.py takes them
  double row[kTaps];   // horizontal factors
};

// The level MSI.deprocess_image / deprocess_depth_image store (deprocess_kernel, geo_prep.hip), op for op in fp32; NaN -> 0 through fmaxf.
__device__ __forceinline__ float quantize_level(float x, bool is_depth) {
#pragma clang fp contract(off)
  if (!is_depth) x = (x + 1.0f) / 2.0f;
  float y = truncf(x * 255.5f);
  y = fminf(fmaxf(y, 0.0f), 255.0f);
  return y;
}

__device__ __forceinline__ double stage_value(uint8_t v, int) { return (double)v; }

__device__ __forceinline__ double stage_value(float v, int mode) {
  switch (mode) {
    case STAGE_IMAGE: return ((double)v + 1.0) / 2.0 * 255.0;
    case STAGE_DEPTH: return (double)v * 255.0;
    case STAGE_IMAGE_Q: return (double)quantize_level(v, false);
    case STAGE_DEPTH_Q: return (double)quantize_level(v, true);
    default: return (double)v;
  }
}

// Sum over the 64 lanes in a fixed tree; the total is in lane 0.
__device__ __forceinline__ double wave_sum(double v) {
#pragma unroll
  for (int off = 32; off > 0; off >>= 1) v += __shfl_down(v, off, 64);
  return v;
}

template <typename T>
__global__ __launch_bounds__(kThreads) void score_tiles_kernel(const T *__restrict__ pred, const T *__restrict__ target, int mode, int group,
                                                               int height, int width, int channels, int tiles_x, int tiles_y,
                                                               const double *__restrict__ row_weights, int do_ssim, double c1, double c2,
                                                               ScoreTaps taps, double *__restrict__ records) {
  __shared__ double sx[kPatchH * kPatchW];
  __shared__ double sy[kPatchH * kPatchW];
  __shared__ double sv[5][kTileH * kPatchW];
  __shared__ double red[kThreads / 64][kRecord];

  const int tid = threadIdx.x;
  const unsigned tiles = (unsigned)tiles_x * (unsigned)tiles_y;
  const unsigned pair = blockIdx.x / tiles, tile = blockIdx.x % tiles;
  const int ty = (int)(tile / (unsigned)tiles_x), tx = (int)(tile % (unsigned)tiles_x);
  const int r0 = ty * kTileH, c0 = tx * kTileW;
  const bool last_y = ty == tiles_y - 1, last_x = tx == tiles_x - 1;
  const size_t image = (size_t)height * width * channels;
  const T *__restrict__ p = pred + (size_t)pair * image;
  const T *__restrict__ t = target + (size_t)(pair / (unsigned)group) * image;

  double sse = 0.0, sad = 0.0, ssum = 0.0;
  for (int ch = 0; ch < channels; ++ch) {
    if (ch) __syncthreads();                    // the previous channel's readers of sx / sy / sv are done
    for (int it = tid; it < kPatchH * kPatchW; it += kThreads) {
      const int pr = it / kPatchW, pc = it % kPatchW;
      const int gr = r0 + pr, gc = c0 + pc;
      double x = 0.0, y = 0.0;
      if (gr < height && gc < width) {
        const size_t o = ((size_t)gr * width + gc) * channels + ch;
        x = stage_value(p[o], mode);
        y = stage_value(t[o], mode);
        if ((pr < kTileH || last_y) && (pc < kTileW || last_x)) {      // this workgroup owns the pixel
          const double w = row_weights ? row_weights[gr] : 1.0;
          const double d = x - y;
          sse += w * (d * d);
          sad += w * fabs(d);
        }
      }
      sx[it] = x;
      sy[it] = y;
    }
    if (!do_ssim) continue;                     // (uniform)
    __syncthreads();
    for (int it = tid; it < kTileH * kPatchW; it += kThreads) {
      double ax = 0.0, ay = 0.0, axx = 0.0, ayy = 0.0, axy = 0.0;
#pragma unroll
      for (int i = 0; i < kTaps; ++i) {
        const double x = sx[it + i * kPatchW], y = sy[it + i * kPatchW], w = taps.col[i];
        ax = fma(w, x, ax);
        ay = fma(w, y, ay);
        axx = fma(w, x * x, axx);
        ayy = fma(w, y * y, ayy);
        axy = fma(w, x * y, axy);
      }
      sv[0][it] = ax; sv[1][it] = ay; sv[2][it] = axx; sv[3][it] = ayy; sv[4][it] = axy;
    }
    __syncthreads();
#pragma unroll
    for (int k = 0; k < kTileH * kTileW / kThreads; ++k) {
      const int r = (tid >> 5) + k * (kThreads / kTileW), c = tid & (kTileW - 1);
      const int orow = r0 + r, ocol = c0 + c;
      if (orow < height - kHalo && ocol < width - kHalo) {
        const int base = r * kPatchW + c;
        double mx = 0.0, my = 0.0, exx = 0.0, eyy = 0.0, exy = 0.0;
#pragma unroll
        for (int j = 0; j < kTaps; ++j) {
          const double w = taps.row[j];
          mx = fma(w, sv[0][base + j], mx);
          my = fma(w, sv[1][base + j], my);
          exx = fma(w, sv[2][base + j], exx);
          eyy = fma(w, sv[3][base + j], eyy);
          exy = fma(w, sv[4][base + j], exy);
        }
        // evaluate.ssim's expressions in its order (no contraction in this unit)
        const double num0 = mx * my * 2.0, den0 = mx * mx + my * my;
        const double lum = (num0 + c1) / (den0 + c1);
        const double num1 = exy * 2.0, den1 = exx + eyy;
        const double cs = (num1 - num0 + c2) / (den1 - den0 + c2);
        const double w = row_weights ? row_weights[orow + kHalo / 2] : 1.0;     // the window's centre row
        ssum += w * (lum * cs);
      }
    }
  }

  sse = wave_sum(sse);
  sad = wave_sum(sad);
  ssum = wave_sum(ssum);
  if ((tid & 63) == 0) {
    red[tid >> 6][0] = sse; red[tid >> 6][1] = sad; red[tid >> 6][2] = ssum;
  }
  __syncthreads();
  if (tid < kRecord) {
    double v = red[0][tid];
#pragma unroll
    for (int wv = 1; wv < kThreads / 64; ++wv) v += red[wv][tid];
    records[(size_t)blockIdx.x * kRecord + tid] = v;
  }
}

// One wave per pair: out[pair] = {mse, mae, ssim, psnr}, NaN where not requested.
__global__ __launch_bounds__(64) void score_finalize_kernel(const double *__restrict__ records, int tiles, int height, int width, int channels,
                                                            const double *__restrict__ row_weights, double max_val, unsigned metrics,
                                                            double *__restrict__ out) {
  const int lane = threadIdx.x;
  const double *__restrict__ rec = records + (size_t)blockIdx.x * tiles * kRecord;
  double sse = 0.0, sad = 0.0, ssum = 0.0;
  for (int i = lane; i < tiles; i += 64) {
    sse += rec[(size_t)i * kRecord + 0];
    sad += rec[(size_t)i * kRecord + 1];
    ssum += rec[(size_t)i * kRecord + 2];
  }
  sse = wave_sum(sse);
  sad = wave_sum(sad);
  ssum = wave_sum(ssum);
  double wall = (double)height, wmap = (double)(height - kHalo);
  if (row_weights) {                            // sums of the weights over the image rows / over the rows that centre a window
    double a = 0.0, b = 0.0;
    for (int r = lane; r < height; r += 64) {
      const double w = row_weights[r];
      a += w;
      if (r >= kHalo / 2 && r < height - kHalo / 2) b += w;
    }
    wall = wave_sum(a);
    wmap = wave_sum(b);
  }
  if (lane == 0) {
    const double nan = std::numeric_limits<double>::quiet_NaN();
    const double count = wall * (double)width * (double)channels;
    double mse = nan, mae = nan, ssim = nan, psnr = nan;
    if (metrics & MSI_SCORE_MSE) {
      mse = sse / count;
      psnr = mse == 0.0 ? std::numeric_limits<double>::infinity() : 20.0 * log10(max_val) - 10.0 * log10(mse);
    }
    if (metrics & MSI_SCORE_MAE) mae = sad / count;
    if (metrics & MSI_SCORE_SSIM) ssim = ssum / (wmap * (double)(width - kHalo) * (double)channels);
    double *o = out + (size_t)blockIdx.x * 4;
    o[0] = mse; o[1] = mae; o[2] = ssim; o[3] = psnr;
  }
}

// The 1-D factors of the softmax-normalised 11 x 11 Gaussian, by the construction of evaluate.py (_gauss_window, _filter_valid), in fp64.
void build_taps(ScoreTaps *taps) {
  const double sigma = 1.5;
  double g[kTaps], win[kTaps][kTaps];
  for (int i = 0; i < kTaps; ++i) {
    const double c = (double)i - (kTaps - 1) / 2.0;
    g[i] = -0.5 * c * c / (sigma * sigma);
  }
  double gmax = g[0] + g[0];
  for (int i = 0; i < kTaps; ++i)
    for (int j = 0; j < kTaps; ++j) gmax = std::fmax(gmax, g[j] + g[i]);
  double sum = 0.0;
  for (int i = 0; i < kTaps; ++i)
    for (int j = 0; j < kTaps; ++j) {
      win[i][j] = std::exp(g[j] + g[i] - gmax);
      sum += win[i][j];
    }
  for (int i = 0; i < kTaps; ++i) taps->col[i] = taps->row[i] = 0.0;
  for (int i = 0; i < kTaps; ++i)
    for (int j = 0; j < kTaps; ++j) {
      const double w = win[i][j] / sum;
      taps->col[i] += w;
      taps->row[j] += w;
    }
}

inline int tiles_along(int size, int tile) { return size > kHalo ? (size - kHalo + tile - 1) / tile : 1; }

}  // namespace

size_t msi_score_workspace_bytes(int32_t n_pairs, int32_t height, int32_t width, int32_t channels) {
  if (n_pairs < 1 || height < 1 || width < 1 || channels < 1 || channels > 4) {
    msi::fail(MSI_E_BADARG, "score_workspace_bytes: bad dims (n_pairs %d, %d x %d x %d)", (int)n_pairs, (int)height, (int)width, (int)channels);
    return 0;
  }
  return (size_t)n_pairs * (size_t)tiles_along(height, kTileH) * (size_t)tiles_along(width, kTileW) * kRecord * sizeof(double);
}

int msi_score_images(const void *pred, const void *target, int32_t dtype, int32_t transform, int32_t quantize, int32_t n_pairs, int32_t group,
                     int32_t height, int32_t width, int32_t channels, const double *row_weights, double max_val, uint32_t metrics, double *out,
                     void *workspace, size_t workspace_bytes, msi_stream_t stream) {
  MSI_REQUIRE(pred && target && out && workspace, "score_images: null pointer");
  MSI_REQUIRE(n_pairs >= 1, "score_images: n_pairs %d < 1", (int)n_pairs);
  MSI_REQUIRE(group >= 1 && n_pairs % group == 0, "score_images: group %d does not divide n_pairs %d", (int)group, (int)n_pairs);
  MSI_REQUIRE(height >= 1 && width >= 1, "score_images: bad dims %d x %d", (int)height, (int)width);
  MSI_REQUIRE(channels >= 1 && channels <= 4, "score_images: channels %d outside 1..4", (int)channels);
  MSI_REQUIRE(dtype == MSI_SCORE_F32 || dtype == MSI_SCORE_U8, "score_images: unknown dtype %d", (int)dtype);
  MSI_REQUIRE(transform == MSI_SCORE_RAW || transform == MSI_SCORE_IMAGE || transform == MSI_SCORE_DEPTH, "score_images: unknown transform %d",
              (int)transform);
  MSI_REQUIRE(quantize == 0 || quantize == 1, "score_images: quantize must be 0 or 1");
  MSI_REQUIRE(dtype != MSI_SCORE_U8 || (transform == MSI_SCORE_RAW && !quantize), "score_images: uint8 images take the RAW transform without quantize");
  MSI_REQUIRE(!(quantize && transform == MSI_SCORE_RAW), "score_images: quantize needs the IMAGE or DEPTH transform");
  MSI_REQUIRE(metrics != 0 && (metrics & ~(uint32_t)(MSI_SCORE_MSE | MSI_SCORE_MAE | MSI_SCORE_SSIM)) == 0, "score_images: empty or unknown metrics mask 0x%x",
              (unsigned)metrics);
  MSI_REQUIRE(!(metrics & MSI_SCORE_SSIM) || (height >= kTaps && width >= kTaps), "score_images: SSIM needs an image of at least %d x %d, got %d x %d",
              kTaps, kTaps, (int)height, (int)width);
  MSI_REQUIRE(max_val > 0.0, "score_images: max_val must be positive");     // (false for NaN too)
  const int tiles_y = tiles_along(height, kTileH), tiles_x = tiles_along(width, kTileW);
  const size_t tiles = (size_t)tiles_y * (size_t)tiles_x;
  if (tiles * (size_t)n_pairs > (size_t)0x7fffffff)
    return msi::fail(MSI_E_UNSUPPORTED, "score_images: %zu workgroups exceed one launch (2^31 - 1)", tiles * (size_t)n_pairs);
  const size_t need = msi_score_workspace_bytes(n_pairs, height, width, channels);
  if (workspace_bytes < need) return msi::fail(MSI_E_WORKSPACE, "score_images: workspace of %zu bytes, %zu needed", workspace_bytes, need);

  ScoreTaps taps;
  build_taps(&taps);
  const double c1 = (0.01 * max_val) * (0.01 * max_val), c2 = (0.03 * max_val) * (0.03 * max_val);
  const int mode = transform == MSI_SCORE_RAW ? STAGE_RAW
                   : transform == MSI_SCORE_IMAGE ? (quantize ? STAGE_IMAGE_Q : STAGE_IMAGE)
                                                  : (quantize ? STAGE_DEPTH_Q : STAGE_DEPTH);
  const int do_ssim = (metrics & MSI_SCORE_SSIM) ? 1 : 0;
  double *records = static_cast<double *>(workspace);
  const dim3 grid((unsigned)(tiles * (size_t)n_pairs));
  if (dtype == MSI_SCORE_U8)
    hipLaunchKernelGGL(score_tiles_kernel<uint8_t>, grid, dim3(kThreads), 0, msi::as_stream(stream), static_cast<const uint8_t *>(pred),
                       static_cast<const uint8_t *>(target), mode, (int)group, (int)height, (int)width, (int)channels, tiles_x, tiles_y, row_weights,
                       do_ssim, c1, c2, taps, records);
  else
    hipLaunchKernelGGL(score_tiles_kernel<float>, grid, dim3(kThreads), 0, msi::as_stream(stream), static_cast<const float *>(pred),
                       static_cast<const float *>(target), mode, (int)group, (int)height, (int)width, (int)channels, tiles_x, tiles_y, row_weights,
                       do_ssim, c1, c2, taps, records);
  int rc = msi::check_launch("score_tiles");
  if (rc != MSI_OK) return rc;
  hipLaunchKernelGGL(score_finalize_kernel, dim3((unsigned)n_pairs), dim3(64), 0, msi::as_stream(stream), records, (int)tiles, (int)height, (int)width,
                     (int)channels, row_weights, max_val, (unsigned)metrics, out);
  return msi::check_launch("score_finalize");
}
