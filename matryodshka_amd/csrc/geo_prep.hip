// K5 of the geometry side: pre/deprocess (single images and the pair of a frame), pose composition, and the host-built trig tables every
// other family reads.  Kernels first, their C ABI entry points below.  (What the geometry units share: geometry_device.h.)
#include "geometry_device.h"

namespace {

// ------------------------------------------------------------------------ K5
__global__ void preprocess_u8_kernel(const uint8_t *__restrict__ in, float *__restrict__ out,
                                     size_t n) {
  size_t i = (size_t)blockIdx.x * blockDim.x + threadIdx.x;
  const size_t stride = (size_t)gridDim.x * blockDim.x;
  for (; i < n; i += stride) {
    float x = (float)in[i] * (1.0f / 255.0f);
    out[i] = x * 2.0f - 1.0f;
  }
}

__global__ void preprocess_f32_kernel(const float *__restrict__ in, float *__restrict__ out,
                                      size_t n) {
  size_t i = (size_t)blockIdx.x * blockDim.x + threadIdx.x;
  const size_t stride = (size_t)gridDim.x * blockDim.x;
  for (; i < n; i += stride) out[i] = in[i] * 2.0f - 1.0f;
}

__global__ void deprocess_kernel(const float *__restrict__ in, uint8_t *__restrict__ out, size_t n,
                                 int is_depth) {
  size_t i = (size_t)blockIdx.x * blockDim.x + threadIdx.x;
  const size_t stride = (size_t)gridDim.x * blockDim.x;
  for (; i < n; i += stride) {
    float x = in[i];
    if (!is_depth) x = (x + 1.0f) / 2.0f;
    float y = truncf(x * 255.5f);
    y = fminf(fmaxf(y, 0.0f), 255.0f);
    out[i] = (uint8_t)y;
  }
}

// The two images of a frame (ref + src in, rgb + depth out) in ONE launch each: at 2.7 ms per frame every ~5 us
// launch of these 2.5 MB kernels is 0.2 % of the frame.
__global__ void preprocess_u8_pair_kernel(const uint8_t *__restrict__ in0, const uint8_t *__restrict__ in1,
                                          float *__restrict__ out0, float *__restrict__ out1, size_t n) {
  size_t i = (size_t)blockIdx.x * blockDim.x + threadIdx.x;
  const size_t stride = (size_t)gridDim.x * blockDim.x;
  for (; i < 2 * n; i += stride) {
    const bool second = i >= n;
    const size_t k = second ? i - n : i;
    const float x = (float)(second ? in1 : in0)[k] * (1.0f / 255.0f);
    (second ? out1 : out0)[k] = x * 2.0f - 1.0f;
  }
}

__global__ void deprocess_pair_kernel(const float *__restrict__ rgb, const float *__restrict__ depth,
                                      uint8_t *__restrict__ out_rgb, uint8_t *__restrict__ out_depth, size_t n) {
  size_t i = (size_t)blockIdx.x * blockDim.x + threadIdx.x;
  const size_t stride = (size_t)gridDim.x * blockDim.x;
  for (; i < 2 * n; i += stride) {
    const bool second = i >= n;
    const size_t k = second ? i - n : i;
    float x = (second ? depth : rgb)[k];
    if (!second) x = (x + 1.0f) / 2.0f;
    float y = truncf(x * 255.5f);
    y = fminf(fmaxf(y, 0.0f), 255.0f);
    (second ? out_depth : out_rgb)[k] = (uint8_t)y;
  }
}

// [B,4,4] @ [B,4,4], one thread per output element, products summed k = 0..3 (no fma: this file is
// compiled with -ffp-contract=off), like a plain fp32 matmul loop.
__global__ void __launch_bounds__(256)
compose_poses_kernel(const float *__restrict__ lhs, const float *__restrict__ rhs, float *__restrict__ out, int batch) {
  const int i = blockIdx.x * blockDim.x + threadIdx.x;
  if (i >= batch * 16) return;
  const int b = i >> 4, r = (i >> 2) & 3, c = i & 3;
  const float *A = lhs + b * 16 + r * 4, *Bm = rhs + b * 16 + c;
  float acc = A[0] * Bm[0];
  acc = acc + A[1] * Bm[4];
  acc = acc + A[2] * Bm[8];
  acc = acc + A[3] * Bm[12];
  out[i] = acc;
}

// out0 = lhs0 @ rhs, out1 = lhs1 @ rhs in one launch: the two curr_pose of format_network_input (msi.py:1124-1125)
__global__ void __launch_bounds__(256)
compose_pose_pair_kernel(const float *__restrict__ lhs0, const float *__restrict__ lhs1, const float *__restrict__ rhs,
                         float *__restrict__ out0, float *__restrict__ out1, int batch) {
  const int t = blockIdx.x * blockDim.x + threadIdx.x;
  if (t >= batch * 32) return;
  const int which = t / (batch * 16), i = t - which * batch * 16;
  const int b = i >> 4, r = (i >> 2) & 3, c = i & 3;
  const float *A = (which ? lhs1 : lhs0) + b * 16 + r * 4, *Bm = rhs + b * 16 + c;
  float acc = A[0] * Bm[0];
  acc = acc + A[1] * Bm[4];
  acc = acc + A[2] * Bm[8];
  acc = acc + A[3] * Bm[12];
  (which ? out1 : out0)[i] = acc;
}

}  // namespace

extern "C" {

size_t msi_trig_table_floats(int32_t height, int32_t width) {
  if (height <= 0 || width <= 0) return 0;
  return (size_t)2 * width + (size_t)2 * height;
}

static void linspace_f32(double start_d, double stop_d, int n, float *out) {
  // tf.linspace, TF 1.14: step = (stop - start) / (num - 1); v[i] = start + step * i (fp32)
  const float start = (float)start_d, stop = (float)stop_d;
  if (n == 1) { out[0] = start; return; }
  volatile float step = (stop - start) / (float)(n - 1);
  for (int i = 0; i < n; ++i) {
    volatile float prod = step * (float)i;  // volatile: one rounding per op on the host too
    out[i] = start + prod;
  }
}

int msi_build_trig_tables_host(int32_t height, int32_t width, float *out_host) {
  MSI_REQUIRE(height > 0 && width > 0 && out_host, "build_trig_tables: bad arguments");
  const double PI = 3.14159265358979323846;
  float *cs = out_host, *ss = out_host + width;
  float *ct = out_host + 2 * width, *st = ct + height;
  linspace_f32(-PI + PI / width, PI - PI / width, width, cs);
  linspace_f32(-PI / 2.0 + PI / (2 * height), PI / 2.0 - PI / (2 * height), height, ct);
  for (int j = 0; j < width; ++j) {
    const double a = (double)cs[j];
    ss[j] = (float)sin(a);
    cs[j] = (float)cos(a);
  }
  for (int i = 0; i < height; ++i) {
    const double a = (double)ct[i];
    st[i] = (float)sin(a);
    ct[i] = (float)cos(a);
  }
  return MSI_OK;
}

int msi_preprocess_u8_f32(const uint8_t *in, float *out, size_t n, msi_stream_t stream) {
  MSI_REQUIRE(in && out, "preprocess_u8: null pointer");
  if (n == 0) return MSI_OK;
  hipLaunchKernelGGL(preprocess_u8_kernel, dim3(grid_1d(n)), dim3(256), 0, msi::as_stream(stream),
                     in, out, n);
  return msi::check_launch("preprocess_u8");
}

int msi_preprocess_pair_u8_f32(const uint8_t *in0, const uint8_t *in1, float *out0, float *out1, size_t n,
                               msi_stream_t stream) {
  MSI_REQUIRE(in0 && in1 && out0 && out1, "preprocess_pair: null pointer");
  if (n == 0) return MSI_OK;
  hipLaunchKernelGGL(preprocess_u8_pair_kernel, dim3(grid_1d(2 * n)), dim3(256), 0, msi::as_stream(stream), in0, in1,
                     out0, out1, n);
  return msi::check_launch("preprocess_pair");
}

int msi_deprocess_pair_f32_u8(const float *rgb, const float *depth, uint8_t *out_rgb, uint8_t *out_depth, size_t n,
                              msi_stream_t stream) {
  MSI_REQUIRE(rgb && depth && out_rgb && out_depth, "deprocess_pair: null pointer");
  if (n == 0) return MSI_OK;
  hipLaunchKernelGGL(deprocess_pair_kernel, dim3(grid_1d(2 * n)), dim3(256), 0, msi::as_stream(stream), rgb, depth,
                     out_rgb, out_depth, n);
  return msi::check_launch("deprocess_pair");
}

int msi_preprocess_f32(const float *in, float *out, size_t n, msi_stream_t stream) {
  MSI_REQUIRE(in && out, "preprocess_f32: null pointer");
  if (n == 0) return MSI_OK;
  hipLaunchKernelGGL(preprocess_f32_kernel, dim3(grid_1d(n)), dim3(256), 0, msi::as_stream(stream),
                     in, out, n);
  return msi::check_launch("preprocess_f32");
}

int msi_deprocess_f32_u8(const float *in, uint8_t *out, size_t n, int32_t is_depth,
                         msi_stream_t stream) {
  MSI_REQUIRE(in && out, "deprocess: null pointer");
  if (n == 0) return MSI_OK;
  hipLaunchKernelGGL(deprocess_kernel, dim3(grid_1d(n)), dim3(256), 0, msi::as_stream(stream), in,
                     out, n, (int)is_depth);
  return msi::check_launch("deprocess");
}

int msi_compose_pose_pair_f32(const float *lhs0, const float *lhs1, const float *rhs, float *out0, float *out1,
                              int32_t batch, msi_stream_t stream) {
  MSI_REQUIRE(lhs0 && lhs1 && rhs && out0 && out1, "compose_pose_pair: null pointer");
  MSI_REQUIRE(batch >= 0, "compose_pose_pair: bad batch");
  if (batch == 0) return MSI_OK;
  hipLaunchKernelGGL(compose_pose_pair_kernel, dim3(grid_1d((size_t)batch * 32)), dim3(256), 0, msi::as_stream(stream),
                     lhs0, lhs1, rhs, out0, out1, (int)batch);
  return msi::check_launch("compose_pose_pair");
}

int msi_compose_poses_f32(const float *lhs, const float *rhs, float *out, int32_t batch,
                          msi_stream_t stream) {
  MSI_REQUIRE(lhs && rhs && out, "compose_poses: null pointer");
  MSI_REQUIRE(batch >= 0, "compose_poses: bad batch");
  if (batch == 0) return MSI_OK;
  hipLaunchKernelGGL(compose_poses_kernel, dim3(grid_1d((size_t)batch * 16)), dim3(256), 0, msi::as_stream(stream),
                     lhs, rhs, out, (int)batch);
  return msi::check_launch("compose_poses");
}

}  // extern "C"
