// Host-side types of the K2 convolution path, shared by its three host units: the layer table (cnn_net.hip builds it), the plan (cnn_plan.hip fills it),
// the forward loop (cnn.hip reads it).  No kernel and no launch here.
#pragma once
#include "cnn_device.h"

namespace msi_cnn {

struct Layer {
  char name[16];
  int kind;  // MODE_*
  int cin, cout, has_coord, stride, rate;
  int in_h, in_w, out_h, out_w;
  int src0, src1;  // producer layer indices (-1 = net_input; src1 = -1: none)
  int c0, c1;
  int ntaps, cpt0, cpt1, ksteps, nclass, npad;
  int wrapt;       // conv-transpose of msi_train_net: GEMM rows cover the uncropped VALID output (see tap_delta)
  int mh, mw;      // GEMM row grid per sample and class
  double ln_count; // elements per sample the LayerNorm statistics run over
  size_t param_off, param_floats;  // floats
  size_t packed_off;               // floats: weights, then gamma, beta (or bias), then the CoordNet bias table
  size_t packed_w_floats;
  size_t gamma_off, beta_off, coord_off;  // floats inside the packed blob
  size_t lnscl_off;                       // floats inside the packed blob: LN_SCL_DOUBLES doubles (8-byte aligned)
  size_t x3_off;                          // floats inside the packed blob: the 3-way bf16 split of the weights (conv_halo_x3_kernel), 0 = none
  size_t x2_off;                          // ... the 2-way fp16 split (h, m' = (w - h) 2^11: plan option F32_SPLIT_F16), 0 = none
  size_t raw_off, aff_off;                // bytes inside the workspace
  size_t act_off;                         // bf16 path: normalised bf16 activation (the next layer's operand)
  size_t sums_off;                        // LayerNorm sums [B][LN_SHARDS][LN_WORDS] int64
};

inline size_t round_up(size_t v, size_t a) { return (v + a - 1) / a * a; }

struct Net {
  std::vector<Layer> layers;
  size_t param_floats = 0, packed_floats = 0, ws_bytes = 0, partial_off = 0, partial_bytes = 0;
  size_t zero_off = 0, zero_bytes = 0;   // [tickets of the in-launch fix-up | LayerNorm sums]: one memset per forward
  size_t cnt_off = 0;   // arrival tickets: [layer][5 * num_cus] ints
  size_t err_off = 0;   // one int: the plan's status word (STATUS_* bits), behind the LayerNorm sums
  // bf16 plans: the head's weights (rounded to bf16) once more as fp32 rows, for the fused tail (head_assemble_kernel
  // runs the 1x1 head on the fp32 MFMA: exact products of bf16 values, fp32 accumulate -- the bf16 head's arithmetic)
  size_t head_f32_off = 0;
  int head_f32_ksteps = 0, head_f32_npad = 0;
};

int build_net(const msi_net_desc *d, int num_cus, Net &net);   // cnn_net.hip
int device_cu_count();   // cnn.hip: the device's CU count, DEFAULT_CUS without a device (a host program that links the planner without the forward supplies its own)

}  // namespace msi_cnn

struct msi_net_plan {
  msi_net_desc desc;
  int num_cus;
  int opt[MSI_NET_OPT_COUNT];
  Net net;
  LayerLaunch launch[MSI_NET_NUM_LAYERS];
};
