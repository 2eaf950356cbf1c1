// K2: the encoder-decoder CNN of nets.msi_coord_train_net / nets.msi_train_net
// (reference nets.py:471-515 / 387-450) as implicit-GEMM convolutions on the
// gfx950 fp32 MFMA (v_mfma_f32_32x32x2_f32: exact fp32, a k-ordered fma chain).
//
// Design rule (measured, tools/ubench/mfma_valu_overlap.hip): on gfx950 the fp32-input MFMA
// runs on the SIMD's fp32 ALUs -- MFMA and VALU work do NOT overlap, neither inside one wave
// (8 MFMA + 128 fma = 6.3 ms vs 4.4 + 2.6 alone) nor between two waves of one SIMD.  Every
// VALU instruction in the k-loop is therefore paid for in matrix throughput, so the k-loop of
// this kernel contains no VALU at all:
//   * both GEMM operands go HBM/L2 -> LDS by buffer DMA (`buffer_load_dwordx4 ... lds`):
//     no VGPR staging, no ds_write; the per-lane offsets are constant over a (tap, source)
//     segment and the channel walk is a scalar soffset;
//   * zero padding, M-tile tails and channel tails are lanes whose offset is out of range of the
//     buffer descriptor: the hardware zero-fills those LDS slots (probed: tools/ubench/dma_oob.hip);
//   * the LDS image is linear per row (128 B = 32 channels) with the 16-byte slot XOR-swizzled by
//     (row>>1)&7 -- applied to the per-lane SOURCE offset for A and baked into the packed
//     weights for B -- which makes the ds_read_b128 operand fetch bank-conflict free;
//   * the operand fetch is inline asm: eight address VGPRs, the stage offset is the ds_read
//     immediate, all eight reads of a k-step are issued before its MFMAs (counted lgkmcnt waits);
//   * a 2-stage LDS ring (32 KB => five workgroups per CU), one barrier per k-step, the next
//     k-step's DMA issued after the first MFMA quarter.
// Consequence: the producer's LayerNorm + ReLU can no longer be applied in the operand loader;
// it is applied once, in place, by ln_apply_kernel (HBM-bound, ~1 read + 1 write per activation)
// instead of 9 x Cout/BN times in VALU.
//
// One kernel template serves every layer:
//   * conv3x3 (stride 1/2, rate 1/2, SAME-zero or wrap padding), the 1x1 head,
//     and conv-transpose 4x4 s2 as four output-parity sub-convolutions of 2x2
//     taps each (a class index in the 1-D grid);
//   * GEMM view: M = pixels of one sample, N = Cout, K = taps x Cin, walked in
//     k-steps of 32 channels of one tap; two sources = skip concat by descriptor pair;
//   * CoordNet's |sin(lat)| channel (nets.py:260-265) is constant along W and independent of the image:
//     its share of the convolution is a host-built table [out row][column border class][Cout] that the
//     epilogue adds to the accumulators (no extra k-step);
//   * the accumulators are kept TRANSPOSED (weights are the MFMA's row operand): a lane owns one
//     pixel and 16 channels in four runs of four, so the epilogue stores 16-byte pieces straight
//     from registers (no LDS staging, no barrier) and takes the LayerNorm sums from the same registers;
//   * LayerNorm statistics: every wave adds its (sum x, sum x^2) -- formed about a wave-uniform pivot in fp32,
//     completed in fp64 -- to 64 sharded FIXED-POINT accumulators with integer atomics: integer addition is
//     associative, so the totals are bit-identical whatever the arrival order, and the consumer
//     (ln_apply_kernel, or the 1x1 head while loading) derives mean / variance from 64 x 4 words instead of
//     merging thousands of per-workgroup partials;
//   * bf16 operands (BF16 = 1): the same 128-byte rows hold 64 channels, v_mfma_f32_32x32x16_bf16.
//
// Tiling: 256 threads = 4 wavefronts (2x2), wave tile (BM/2)x(BN/2) of 32x32 MFMA tiles, BK=32;
// work decomposition ("tail split": the tiles of the partial last wave are cut along K inside the launch, the
// last arriving workgroup of a tile sums the partial accumulators) and the measured alternatives: DESIGN.md 4.
// The decomposition (tile_work, tile_index), the hand-off (splitk_arrive, splitk_sum), the LayerNorm affine a consumer applies while staging
// (ln_affine_read, ln_scale_shift) and the timing stamps (ConvStamps) are in cnn_device.h; a kernel that spells one of them out says why at the place.
#include "cnn_plan.h"

namespace msi_cnn {

int device_cu_count() {
  int dev = 0;
  hipDeviceProp_t prop;
  if (hipGetDevice(&dev) != hipSuccess || hipGetDeviceProperties(&prop, dev) != hipSuccess || prop.multiProcessorCount <= 0) {
    (void)hipGetLastError();   // no device (build container): sizes for the default part
    return DEFAULT_CUS;
  }
  return prop.multiProcessorCount;
}

// One layer's conv launch: the family's unit launches the instantiation Q.variant names; where the plan sums the split tiles in a launch of their own
// (plan option FIXUP_KERNEL, or more split tiles than tickets), conv_fixup_kernel follows -- for the tile and mode of the record, the conv-transpose halo
// kernels' two class slabs per K-range as grid.y.
int launch_conv(const LayerLaunch &Q, const ConvParams &p, hipStream_t stream) {
  const ConvVariant &V = Q.variant;
  int rc;
  switch (V.family) {
    case CONV_IGEMM: rc = launch_igemm(Q, p, stream); break;
    case CONV_HALO: case CONV_HALO_S2: case CONVT_HALO: rc = launch_halo_f32(Q, p, stream); break;
    case CONV_HALO_X3: case CONV_HALO8_X3: case CONV_HALO_S2_X3: case CONV_HALO8_S2_X3: case CONVT_HALO_X3: case CONVT_HALO8_X3: rc = launch_x3(Q, p, stream); break;
    case CONV_HALO_BF16: case CONV_HALO_BF16_S2: case CONVT_HALO_BF16: rc = launch_bf16_halo(Q, p, stream); break;
    default: return msi::fail(MSI_E_UNSUPPORTED, "conv: unknown kernel family %d", V.family);
  }
  if (rc || Q.nfix == 0 || p.tile_cnt != nullptr) return rc;
  const int mode = V.family == CONV_IGEMM ? V.mode : (V.is_convt() ? MODE_CONVT : MODE_CONV);
  return launch_fixup(V.bm, V.bn, mode, V.family == CONV_IGEMM && V.bf16 && mode != MODE_HEAD, Q.nfix, V.is_convt() ? 2 : 1, p, stream);
}

}  // namespace msi_cnn

#if defined(MSI_CONV_TIMING) || defined(MSI_DEBUG_STATS)
// tools/conv_timing.py: per-workgroup phase stamps of one layer's conv launch (debug builds only)
static unsigned long long *g_timing_buf = nullptr;
static int g_timing_layer = -1;
extern "C" int msi_debug_conv_occupancy(int lds_bytes) {
  return msi_cnn::debug_conv_occupancy(lds_bytes);
}
extern "C" void msi_debug_conv_timing(void *device_buffer, int layer) {
  g_timing_buf = static_cast<unsigned long long *>(device_buffer);
  g_timing_layer = layer;
}
#endif

extern "C" {

#ifdef MSI_DEBUG_SUMS   // (debug builds only: byte offset of a layer's LayerNorm sums in the workspace)
extern "C" long long msi_debug_sums_offset(const msi_net_plan *plan, int layer) { return (long long)plan->net.layers[layer].sums_off; }
extern "C" long long msi_debug_partial_offset(const msi_net_plan *plan) { return (long long)plan->net.partial_off; }
#endif
static int run_layers(const msi_net_plan *plan, const float *packed, const void *net_input, float *pred,
                      void *workspace, size_t workspace_bytes, msi_stream_t stream_, int nlayers) {
  MSI_REQUIRE(plan, "net_forward: null plan");
  const msi_net_desc *desc = &plan->desc;
  const Net &net = plan->net;
  const int bf16 = desc->dtype == MSI_DTYPE_BF16;
  MSI_REQUIRE(packed && net_input && workspace, "net_forward: null pointer");
  if (workspace_bytes < net.ws_bytes)
    return msi::fail(MSI_E_WORKSPACE, "net_forward: workspace %zu B < required %zu B", workspace_bytes,
                     net.ws_bytes);
  if (desc->batch == 0) return MSI_OK;
  hipStream_t stream = msi::as_stream(stream_);
  char *ws = static_cast<char *>(workspace);
  // tickets of the in-launch fix-ups and the LayerNorm sums start from zero
  // (a kernel of the library's own instead of hipMemsetAsync: the runtime's fill is a blit with its own barrier packets)
  {
    const size_t n16 = net.zero_bytes / 16;               // zero_off is a multiple of 256, zero_bytes of 64
    int rc0 = launch_zero(ws + net.zero_off, n16, stream);
    if (rc0) return rc0;
  }
  int *cnt = reinterpret_cast<int *>(ws + net.cnt_off);
  for (int li = 0; li < nlayers; ++li) {
    const Layer &L = net.layers[li];
    const LayerLaunch &Q = plan->launch[li];
    ConvParams p = Q.p;
    // sources: the network input, or the normalised output of the producer -- in place in its raw
    // buffer (fp32) or the bf16 copy ln_apply wrote next to it
    auto src_ptr = [&](int s) -> const char * {
      if (s < 0) return static_cast<const char *>(net_input);
      return ws + (bf16 ? net.layers[s].act_off : net.layers[s].raw_off);
    };
    p.x0 = src_ptr(L.src0);
    p.x1 = L.src1 >= 0 ? src_ptr(L.src1) : p.x0;  // unused second source: alias the first (cpt1 = 0 keeps it unselected)
    p.wpk = reinterpret_cast<const char *>(packed + L.packed_off);
    p.coord_bias = L.has_coord ? packed + L.coord_off : nullptr;
    p.bias = L.kind == MODE_HEAD ? packed + L.gamma_off : nullptr;
    if (Q.fuse_ln) {   // fp32 head: its producer's LayerNorm + ReLU is applied while loading (the producer's buffer holds the raw output)
      const Layer &S = net.layers[L.src0];
      p.ln_sums = reinterpret_cast<const long long *>(ws + S.sums_off);
      p.ln_gamma = packed + S.gamma_off;
      p.ln_beta = packed + S.beta_off;
    }
    p.y = L.kind == MODE_HEAD ? pred : reinterpret_cast<float *>(ws + L.raw_off);
    p.sums = L.kind == MODE_HEAD ? nullptr : reinterpret_cast<long long *>(ws + L.sums_off);
    auto scl_of = [&](int li2) { return reinterpret_cast<const double *>(packed + net.layers[li2].lnscl_off); };
    p.ln_scl = L.kind == MODE_HEAD ? nullptr : scl_of(li);
    p.ln_scl_src = L.src0 >= 0 ? scl_of(L.src0) : nullptr;
    p.ln_scl_src1 = L.src1 >= 0 ? scl_of(L.src1) : nullptr;
    p.status = reinterpret_cast<int *>(ws + net.err_off);
    p.partial = reinterpret_cast<float *>(ws + net.partial_off);
    p.tile_cnt = Q.inlaunch ? cnt + (size_t)li * CONV_SLOTS_PER_CU * plan->num_cus : nullptr;
#if defined(MSI_CONV_TIMING) || defined(MSI_DEBUG_STATS)
    p.dbg = (li == g_timing_layer) ? g_timing_buf : nullptr;
#endif
    // pointers of the sources whose LayerNorm the consumer applies while staging its patch, then the launch (launch_conv reads Q.variant)
    auto raw_source = [&](int s, bool second) {   // source s is read RAW: its sums / gamma / beta; bf16 plans: also repointed to the raw fp16 buffer (fp32: the raw buffer IS the source buffer)
      const Layer &S = net.layers[s];
      if (!second) {
        if (bf16) p.x0 = ws + S.raw_off;
        p.ln_sums = reinterpret_cast<const long long *>(ws + S.sums_off); p.ln_gamma = packed + S.gamma_off; p.ln_beta = packed + S.beta_off;
      } else {
        if (bf16) p.x1 = ws + S.raw_off;
        p.ln_sums1 = reinterpret_cast<const long long *>(ws + S.sums_off); p.ln_gamma1 = packed + S.gamma_off; p.ln_beta1 = packed + S.beta_off;
      }
    };
    const ConvVariant &V = Q.variant;
    if (V.is_convt()) {         // conv-transpose halo kernels: either source may be raw
      if (p.halo_apply & 1) raw_source(L.src0, false);
      if (p.halo_apply & 2) raw_source(L.src1, true);
    } else if (V.apply) {       // the patch comes from the producer's RAW output
      raw_source(L.src0, false);
    }
    if (V.six_product()) p.wpk_x3 = reinterpret_cast<const char *>(packed + (V.planes == 2 ? L.x2_off : L.x3_off));
    int rc = launch_conv(Q, p, stream);
    if (rc) return rc;
    // (bf16 fused tail: head_assemble_kernel normalises + rounds the head's source itself)
    const bool tail_src = bf16 && nlayers == MSI_NET_NUM_LAYERS - 1 && li == net.layers[MSI_NET_NUM_LAYERS - 1].src0;
    if (L.kind != MODE_HEAD && !Q.skip_apply && !tail_src) {
      const size_t per_sample = (size_t)L.out_h * L.out_w * L.cout;
      float *raw = reinterpret_cast<float *>(ws + L.raw_off), *aff = reinterpret_cast<float *>(ws + L.aff_off);
      const size_t lds = (size_t)2 * L.cout * sizeof(float);
      const long long *sums = reinterpret_cast<const long long *>(ws + L.sums_off);
      rc = launch_ln_apply(bf16, Q.ln_blocks, desc->batch, lds, stream, raw, sums, 1.0 / L.ln_count, scl_of(li), p.status, packed + L.gamma_off, packed + L.beta_off,
                           per_sample, L.cout, aff, bf16 ? reinterpret_cast<unsigned short *>(ws + L.act_off) : static_cast<unsigned short *>(nullptr));
      if (rc) return rc;
    }
  }
  return MSI_OK;
}

int32_t msi_net_plan_status(const msi_net_plan *plan, const void *workspace, msi_stream_t stream_, int32_t *status_bits) {
  MSI_REQUIRE(plan && workspace, "net_plan_status: null pointer");
  hipStream_t stream = msi::as_stream(stream_);
  int word = 0;
  hipError_t e = hipMemcpyAsync(&word, static_cast<const char *>(workspace) + plan->net.err_off, sizeof(int), hipMemcpyDeviceToHost, stream);
  if (e == hipSuccess) e = hipStreamSynchronize(stream);
  if (e != hipSuccess) return msi::fail(MSI_E_LAUNCH, "net_plan_status: %s", hipGetErrorString(e));
  if (status_bits) *status_bits = word;
  if (word == 0) return MSI_OK;
  return msi::fail(MSI_E_RANGE, "net_plan_status: 0x%x:%s%s%s", word,
                   (word & STATUS_F16_SPLIT_RANGE) ? " an operand of a layer on the fp16 split exceeded the fp16 range (|x| > 65504): set MSI_NET_OPT_F32_SPLIT_F16 = 0" : "",
                   (word & STATUS_LN_OVERFLOW) ? " a LayerNorm sum left its fixed-point window (raw convolution output far above the scale the weights predict: non-finite or mis-scaled input?)" : "",
                   (word & STATUS_LN_UNDERFLOW) ? " a LayerNorm variance is below the resolution of its fixed-point window (raw convolution output far below the scale the weights predict, or constant)" : "");
}

// LayerNorm window calibration.  The fixed-point window of a layer's sums follows an exponent the packer ESTIMATES from the weights
// (sqrt(K) rms(w) rms(input)); trained gamma / beta / weights may put a layer's real raw output 2^+-12 away from that estimate, and then every forward ends in
// MSI_E_RANGE.  This entry point MEASURES instead: layer by layer (a layer's input is only right once its producers' windows are), run layers 0 .. L, read L's sums
// and the status word, move the exponent by 12 while the sums overflow / underflow, then centre it on the measured rms (log-mid of the smallest and largest sample),
// write {S1, S2, 1 / S1, 1 / S2} into the packed blob ON THE DEVICE and run 0 .. L once more so that L's consumers see sums in the new unit.  Synchronous (it reads
// the sums back: a one-off, ~40 forwards' worth of kernels), allocates nothing, leaves the workspace as a forward of layers 0 .. 16 would.
int32_t msi_net_plan_calibrate(const msi_net_plan *plan, float *packed, const void *net_input, void *workspace, size_t workspace_bytes,
                               msi_stream_t stream_, int32_t *layers_changed) {
  MSI_REQUIRE(plan && packed && net_input && workspace, "net_plan_calibrate: null pointer");
  const Net &net = plan->net;
  const msi_net_desc *desc = &plan->desc;
  hipStream_t stream = msi::as_stream(stream_);
  if (layers_changed) *layers_changed = 0;
  if (desc->batch == 0) return MSI_OK;
  const size_t nwords = (size_t)desc->batch * LN_SHARDS * LN_WORDS;
  std::vector<long long> sums(nwords);
  char *ws = static_cast<char *>(workspace);
  // ALL OR NOTHING: the windows of every layer as they were on entry; any error return writes back those of the layers touched so far, so a frame that
  // cannot be calibrated on (constant, non-finite) leaves the packed blob exactly as it found it.
  constexpr int NL = MSI_NET_NUM_LAYERS - 1;
  double orig[NL][LN_SCL_DOUBLES];
  hipError_t he = hipSuccess;
  for (int li = 0; li < NL && he == hipSuccess; ++li)
    he = hipMemcpyAsync(orig[li], packed + net.layers[li].lnscl_off, sizeof(orig[li]), hipMemcpyDeviceToHost, stream);
  if (he == hipSuccess) he = hipStreamSynchronize(stream);
  if (he != hipSuccess) return msi::fail(MSI_E_LAUNCH, "net_plan_calibrate: %s", hipGetErrorString(he));
  int touched = 0;                         // layers 0 .. touched - 1 may hold new windows
  auto restore = [&]() {
    for (int l = 0; l < touched; ++l)
      (void)hipMemcpyAsync(packed + net.layers[l].lnscl_off, orig[l], sizeof(orig[l]), hipMemcpyHostToDevice, stream);
    (void)hipStreamSynchronize(stream);    // (orig is on this stack frame)
  };
  for (int li = 0; li < NL; ++li) {
    const Layer &L = net.layers[li];
    const double *scl = orig[li];
    int e0 = LN_S1_BITS - (int)lrint(log2(scl[0])), e = e0;
    bool settled = false;
    touched = li + 1;
    for (int it = 0; it < 24 && !settled; ++it) {
      const double ns[LN_SCL_DOUBLES] = {ldexp(1.0, LN_S1_BITS - e), ldexp(1.0, LN_S2_BITS - 2 * e), ldexp(1.0, -(LN_S1_BITS - e)), ldexp(1.0, -(LN_S2_BITS - 2 * e))};
      he = hipMemcpyAsync(packed + L.lnscl_off, ns, sizeof(ns), hipMemcpyHostToDevice, stream);
      if (he == hipSuccess) he = hipStreamSynchronize(stream);   // (ns is on this stack frame)
      if (he != hipSuccess) { restore(); return msi::fail(MSI_E_LAUNCH, "net_plan_calibrate: %s", hipGetErrorString(he)); }
      int rc = run_layers(plan, packed, net_input, nullptr, workspace, workspace_bytes, stream_, li + 1);
      if (rc) { restore(); return rc; }
      int word = 0;
      he = hipMemcpyAsync(sums.data(), ws + L.sums_off, nwords * sizeof(long long), hipMemcpyDeviceToHost, stream);
      if (he == hipSuccess) he = hipMemcpyAsync(&word, ws + net.err_off, sizeof(int), hipMemcpyDeviceToHost, stream);
      if (he == hipSuccess) he = hipStreamSynchronize(stream);
      if (he != hipSuccess) { restore(); return msi::fail(MSI_E_LAUNCH, "net_plan_calibrate: %s", hipGetErrorString(he)); }
      if (word & STATUS_LN_OVERFLOW) { e += 12; if (e > 120) break; continue; }   // a share left the window (or the data is not finite: the loop gives up at 2^120)
      // per sample: sum x^2 in units of 1 / S2; below ~1e6 sqrt(waves) units the variance is resolved to < 6 digits (ln_mean_inv's rule, restated on the host).
      // The window is centred on the samples it RESOLVES; a constant sample (a black frame in a batch) or one far below the others is left out instead of
      // dragging the window down 12 bits at a time until nothing fits -- a forward flags such a sample itself.
      double rmin = 1e300, rmax = 0.0, amin = 1e300, amax = 0.0;   // (resolved samples | every sample with a non-zero sum of squares)
      for (int b = 0; b < desc->batch; ++b) {
        double h2 = 0.0;
        for (int sh = 0; sh < LN_SHARDS; ++sh)
          h2 += (double)sums[((size_t)b * LN_SHARDS + sh) * LN_WORDS + 1];
        const bool under = h2 * h2 < LN_UNDERFLOW_UNITS_SQ * (L.ln_count / 1024.0 + 1.0);
        const double ms = h2 * ns[3] / L.ln_count;           // E[x^2]: the window has to hold the raw values themselves
        const double r = sqrt(ms > 0.0 ? ms : 0.0);
        if (r > 0.0) { amin = r < amin ? r : amin; amax = r > amax ? r : amax; }
        if (r > 0.0 && !under) { rmin = r < rmin ? r : rmin; rmax = r > rmax ? r : rmax; }
      }
      if (rmax > 0.0) {                                                              // something is resolved: centre on it (to within an octave), measure once more in the new unit
        const int ec = (int)lrint(0.5 * (log2(rmax) + log2(rmin)));
        if (ec > e + 1 || ec < e - 1) { e = ec; continue; }
        settled = true;
      } else if (amax > 0.0) {                                                       // seen but not resolved: go to where the coarse reading points, else lower
        const int ec = (int)lrint(0.5 * (log2(amax) + log2(amin)));
        if (ec > e + 1 || ec < e - 1) e = ec; else e -= 12;
        if (e < -120) break;
      } else { e -= 12; if (e < -120) break; }                                       // nothing at all in this window: look lower
    }
    if (!settled) {
      restore();
      if (layers_changed) *layers_changed = 0;
      return msi::fail(MSI_E_RANGE, "net_plan_calibrate: layer %s has no finite, non-constant raw output to centre a LayerNorm window on (non-finite input or weights, "
                       "or a constant frame?); the windows are unchanged", L.name);
    }
    if (e != e0 && layers_changed) ++*layers_changed;
  }
  return MSI_OK;
}

int msi_net_plan_forward(const msi_net_plan *plan, const float *packed, const void *net_input, float *pred,
                         void *workspace, size_t workspace_bytes, msi_stream_t stream_) {
  MSI_REQUIRE(pred, "net_forward: null pointer");
  return run_layers(plan, packed, net_input, pred, workspace, workspace_bytes, stream_, MSI_NET_NUM_LAYERS);
}

// The fused tail behind msi_net_plan_forward_rgba (format = MSI_LAYERS_F32, layers_out = null: head_assemble_kernel) and
// msi_net_plan_forward_layers (a packed layers_out: head_assemble_packed_kernel, rgba_native optional); `who` names the caller in error texts.
static int forward_fused_tail(const char *who, const msi_net_plan *plan, const float *packed, const void *net_input, float *rgba_native,
                              void *layers_out, int32_t format, float *blend_weights, float *alphas, float *pred, void *workspace,
                              size_t workspace_bytes, msi_stream_t stream_, void *event_after_convs) {
  MSI_REQUIRE(plan, "%s: null plan", who);
  const msi_net_desc *desc = &plan->desc;
  const Net &net = plan->net;
  const Layer &H = net.layers[MSI_NET_NUM_LAYERS - 1];
  const int nd = desc->num_outputs / 2;
  const int bf16 = desc->dtype == MSI_DTYPE_BF16;
  if ((!bf16 && !plan->launch[MSI_NET_NUM_LAYERS - 1].fuse_ln) || (bf16 && !plan->opt[MSI_NET_OPT_HEAD_FUSE_LN]) ||
      H.c0 > 64 || H.c0 % 4 != 0 || desc->num_outputs != 2 * nd || nd % 4 != 0 || nd > 64 || desc->in_channels != 6 * nd ||
      ((long)desc->height * desc->width) % HA_TP != 0)
    return msi::fail(MSI_E_UNSUPPORTED, "%s: fused tail needs a blend_psv network (in = 6 D, out = 2 D, "
                     "D %% 4 == 0, D <= 64, ngf <= 64, HEAD_FUSE_LN on)", who);
  MSI_REQUIRE(rgba_native || layers_out, "%s: null pointer", who);
  MSI_REQUIRE(!layers_out || (reinterpret_cast<uintptr_t>(layers_out) & 15) == 0, "%s: layers_out is not 16-byte aligned", who);
  const int ng = (nd + HA_LG - 1) / HA_LG;   // layer groups (grid.y of the fused tail): D = 64 -> 2 x 32 layers
  if (nd % ng != 0 || (nd / ng) % 4 != 0 || (ng > 1 && bf16 && (nd / ng) % 8 != 0))
    return msi::fail(MSI_E_UNSUPPORTED, "%s: D = %d does not split into layer groups of a multiple of %d", who, nd, bf16 ? 8 : 4);
  // (bf16: the head's source stays raw fp32 -- no ln_apply launch, no bf16 copy: this kernel normalises and rounds it)
  int rc = run_layers(plan, packed, net_input, nullptr, workspace, workspace_bytes, stream_, MSI_NET_NUM_LAYERS - 1);
  if (rc || desc->batch == 0) return rc;
  hipStream_t stream = msi::as_stream(stream_);
  if (event_after_convs) {
    hipError_t e = hipEventRecord(static_cast<hipEvent_t>(event_after_convs), stream);
    if (e != hipSuccess) return msi::fail(MSI_E_LAUNCH, "%s: %s", who, hipGetErrorString(e));
  }
  char *ws = static_cast<char *>(workspace);
  const Layer &S = net.layers[H.src0];
  HeadAsmParams q;
  q.x = reinterpret_cast<const float *>(ws + S.raw_off);
  q.wpk = packed + H.packed_off;   // (bf16 plans: the packed bf16 rows themselves -- the fp32-format copy at head_f32_off is unused since r04)
  q.bias = packed + H.gamma_off;
  float *aff = reinterpret_cast<float *>(ws + S.aff_off);
  rc = launch_ln_finish(desc->batch, stream, reinterpret_cast<const long long *>(ws + S.sums_off), 1.0 / S.ln_count,
                        reinterpret_cast<const double *>(packed + S.lnscl_off), reinterpret_cast<int *>(ws + net.err_off),
                        packed + S.gamma_off, packed + S.beta_off, S.cout, aff, bf16);
  if (rc) return rc;
  q.aff = aff;
  q.psv = net_input;
  q.rgba = reinterpret_cast<float4 *>(rgba_native);
  q.layers = layers_out;
  q.bw_out = blend_weights;
  q.al_out = alphas;
  q.pred_out = pred;
  q.C0 = H.c0; q.ksteps = H.ksteps; q.npad = H.npad;   // (bf16: one k-step of 64 channels)
  q.nd = nd; q.hw = desc->height * desc->width;
  q.npix_total = (long)desc->batch * q.hw;
  q.lg = nd / ng;
  q.ng = ng;
  {
    auto magic = [](unsigned d) { return d == 1 ? 0xffffffffu : (unsigned)((1ull << 32) / d); };
    const int vec = bf16 ? 8 : 4;                                  // elements per 16-byte vector of the sweep volume
    const unsigned vpp = (unsigned)((ng == 1 ? 6 * nd : 2 * 3 * q.lg) / vec);
    q.mg_vpp = magic(vpp);
    q.mg_nchunk = magic((unsigned)(q.ksteps * 8));
    q.mg_hw = magic((unsigned)q.hw);
    if (q.npix_total >= (1L << 32)) return msi::fail(MSI_E_UNSUPPORTED, "%s: more than 2^32 pixels per batch", who);
  }
  constexpr int BN = 64;
  size_t r_bytes = (size_t)q.ksteps * (HA_TP + BN) * ROW_BYTES;
  if (r_bytes < (size_t)HA_TP * (6 * q.lg + 1) * sizeof(float)) r_bytes = (size_t)HA_TP * (6 * q.lg + 1) * sizeof(float);
  if (bf16) {   // no weight tile in LDS, packed-bf16 sweep tile (see the kernel)
    r_bytes = (size_t)q.ksteps * HA_TP * ROW_BYTES;
    if (r_bytes < (size_t)HA_TP * (3 * q.lg + 1) * sizeof(unsigned)) r_bytes = (size_t)HA_TP * (3 * q.lg + 1) * sizeof(unsigned);
  }
  const size_t lds = 2 * 64 * 4 + 64 + ((r_bytes + 15) & ~(size_t)15) + (size_t)HA_TP * (2 * q.lg + 1) * sizeof(float);
  const long ntile = q.npix_total / HA_TP;
  if (((ntile + 7) / 8) * 8 * ng >= (1L << 31)) return msi::fail(MSI_E_UNSUPPORTED, "%s: too many pixel tiles for one launch", who);
  // (see the kernel: XCD x takes tiles x, x + 8, ...; the layer groups of a tile are neighbours there)
  return launch_head_assemble(bf16, layers_out ? format : MSI_LAYERS_F32, (unsigned)(((ntile + 7) / 8) * 8 * ng), lds, stream, q);
}

int msi_net_plan_forward_rgba(const msi_net_plan *plan, const float *packed, const void *net_input, float *rgba_native,
                              float *blend_weights, float *alphas, float *pred, void *workspace, size_t workspace_bytes,
                              msi_stream_t stream_, void *event_after_convs) {
  return forward_fused_tail("net_forward_rgba", plan, packed, net_input, rgba_native, nullptr, MSI_LAYERS_F32, blend_weights, alphas, pred,
                            workspace, workspace_bytes, stream_, event_after_convs);
}

int msi_net_plan_forward_layers(const msi_net_plan *plan, const float *packed, const void *net_input, float *rgba_native,
                                void *layers_out, int32_t format, float *blend_weights, float *alphas, float *pred, void *workspace,
                                size_t workspace_bytes, msi_stream_t stream_, void *event_after_convs) {
  // (the first two checks need no plan, hence no device)
  MSI_REQUIRE(!layers_out || format == MSI_LAYERS_RGBA8 || format == MSI_LAYERS_RGBA16F,
              "net_forward_layers: unknown format %d (layers_out is MSI_LAYERS_RGBA8 or MSI_LAYERS_RGBA16F)", format);
  MSI_REQUIRE(rgba_native || layers_out, "net_forward_layers: null pointer");
  return forward_fused_tail("net_forward_layers", plan, packed, net_input, rgba_native, layers_out, format, blend_weights, alphas, pred,
                            workspace, workspace_bytes, stream_, event_after_convs);
}

// ---- descriptor-level convenience (a transient plan per call; the frame loop uses a plan) -----------
size_t msi_net_workspace_bytes(const msi_net_desc *desc) {
  msi_net_plan *pl = nullptr;
  if (msi_net_plan_create(desc, &pl)) return 0;
  const size_t n = pl->net.ws_bytes;
  msi_net_plan_destroy(pl);
  return n;
}

static int forward_once(const msi_net_desc *desc, const float *packed, const void *net_input, float *pred,
                        void *workspace, size_t workspace_bytes, msi_stream_t stream) {
  msi_net_plan *pl = nullptr;
  int rc = msi_net_plan_create(desc, &pl);
  if (rc) return rc;
  rc = msi_net_plan_forward(pl, packed, net_input, pred, workspace, workspace_bytes, stream);
  msi_net_plan_destroy(pl);
  return rc;
}

int msi_net_forward_f32(const msi_net_desc *desc, const float *packed, const float *net_input,
                        float *pred, void *workspace, size_t workspace_bytes, msi_stream_t stream) {
  MSI_REQUIRE(desc && desc->dtype == MSI_DTYPE_F32, "net_forward_f32: desc->dtype must be MSI_DTYPE_F32");
  return forward_once(desc, packed, net_input, pred, workspace, workspace_bytes, stream);
}

int msi_net_forward_bf16(const msi_net_desc *desc, const float *packed, const void *net_input_bf16,
                         float *pred, void *workspace, size_t workspace_bytes, msi_stream_t stream) {
  MSI_REQUIRE(desc && desc->dtype == MSI_DTYPE_BF16, "net_forward_bf16: desc->dtype must be MSI_DTYPE_BF16");
  return forward_once(desc, packed, net_input_bf16, pred, workspace, workspace_bytes, stream);
}

}  // extern "C"
