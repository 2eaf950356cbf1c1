// Shared host-side helpers of libmsi_hip.so (error text, launch checks).
#pragma once
#include <hip/hip_runtime.h>
#include <cstdarg>
#include <cstdio>

#include "msi_hip.h"

namespace msi {

char *error_buffer();          // thread-local, 512 bytes
int fail(int code, const char *fmt, ...);

inline hipStream_t as_stream(msi_stream_t s) { return reinterpret_cast<hipStream_t>(s); }

// Checks the launch that has just been enqueued (no synchronisation).
inline int check_launch(const char *what) {
  hipError_t e = hipGetLastError();
  if (e != hipSuccess) return fail(MSI_E_LAUNCH, "%s: %s", what, hipGetErrorString(e));
  return MSI_OK;
}

}  // namespace msi

// ---- the texel encoders of the compact layer formats (MSI_LAYERS_RGBA8 / MSI_LAYERS_RGBA16F; the rule is stated in msi_hip.h) ----
// ONE definition for every kernel that writes a packed texel: pack_layers_kernel (geo_layers.hip) and the packed forms of the fused
// tail (cnn_tail.hip).  fp32 arithmetic with one rounding per operation: the bodies switch contraction off themselves, so that a
// unit compiled without -ffp-contract=off inlines the same operations.
// NaN inputs of the rgba8 encoder (outside the contract): fmaxf returns its other operand, so a NaN channel encodes as code 0.
#if defined(__HIPCC__)
typedef _Float16 half4_g __attribute__((ext_vector_type(4)));
typedef unsigned u32x2_g __attribute__((ext_vector_type(2)));

__device__ __forceinline__ unsigned rgba8_encode(const float4 &t) {
#pragma clang fp contract(off)
  const unsigned r = (unsigned)rintf((fminf(fmaxf(t.x, -1.0f), 1.0f) + 1.0f) * 127.5f);
  const unsigned g = (unsigned)rintf((fminf(fmaxf(t.y, -1.0f), 1.0f) + 1.0f) * 127.5f);
  const unsigned b = (unsigned)rintf((fminf(fmaxf(t.z, -1.0f), 1.0f) + 1.0f) * 127.5f);
  const unsigned a = (unsigned)rintf(fminf(fmaxf(t.w, 0.0f), 1.0f) * 255.0f);
  return r | (g << 8) | (b << 16) | (a << 24);
}

__device__ __forceinline__ u32x2_g rgba16f_encode(const float4 &t) {
  half4_g h;
  h.x = (_Float16)t.x; h.y = (_Float16)t.y; h.z = (_Float16)t.z; h.w = (_Float16)t.w;
  return __builtin_bit_cast(u32x2_g, h);
}
#endif

#define MSI_REQUIRE(cond, ...)                        \
  do {                                                  \
    if (!(cond)) return msi::fail(MSI_E_BADARG, __VA_ARGS__); \
  } while (0)
