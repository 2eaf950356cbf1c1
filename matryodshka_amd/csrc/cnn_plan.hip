// K2, host side: the plan.  plan_tiles cuts a layer into tiles and K-ranges, choose_variant picks the kernel (a ConvVariant: cnn_device.h) -- once, here --
// and plan_layers fills every layer's launch record; the forward loop (cnn.hip), the family launchers and msi_net_plan_layer_kernel only read it.
#include "cnn_plan.h"

namespace {

// Work decomposition of one layer ("tail split", see the kernel) for a BM x BN tile.
void plan_tiles(ConvParams &p, int BM, int BN, int batch, int num_cus, int tailsplit, int max_split, int *nblocks, int *nfix,
                int uniform_split = 0, int split_overhead = 0, bool split_any_tile = false) {
  const int mtot = p.Mh * p.Mw;
  p.tiles_m = (mtot + BM - 1) / BM;
  if (p.halo_tx) p.tiles_m = ((p.Mh + BM / 16 - 1) / (BM / 16)) * p.halo_tx;   // (BM / 16) x 16 spatial tiles (ragged at the right / bottom edge when Mh, Mw are no multiples)
  p.tiles_n = (p.Cout + BN - 1) / BN;
  p.ntiles = p.tiles_m * p.tiles_n * p.nclass * batch;
  // whole tiles in multiples of the CU count, the remainder cut into `split` K-ranges so that
  // (remainder x split) is again close to a multiple of the CU count
  p.n_main = p.ntiles;
  p.split0 = 1;
  p.split = 1;
  // Residency-aware form (tailsplit = 2; NOT the default -- measured slower, see below), for grids of at least one full
  // residency Q = 5 workgroups x CUs:
  // per-workgroup phase stamps (tools/conv_timing.py, r02_l) show the matrix pipes saturated while five workgroups
  // share a CU and starved when the last whole tile of a CU runs beside one short K-range -- e.g. 1 600 tiles = 6 whole
  // per CU + a quarter: the sixth tile ran with 2 waves per SIMD for a whole tile time (14 % of the launch).  So whole
  // tiles are issued in multiples of Q only, and the remaining < Q tiles are cut into K-ranges that fill one more
  // residency (1 600 -> 1 280 whole + 320 x 4 ranges; 3 200 -> 2 560 + 640 x 2): long blocks first, short ones last.
  // Measured (profiles/r02_m): conv2_1 115 -> 124 us, conv7_1 189 -> 205, conv1_1 325 -> 335: the extra K-range blocks
  // (prologue + epilogue + slab traffic each) cost more than the straggler they remove.
  const int Q = CONV_SLOTS_PER_CU * num_cus;
  if (BM * BN == 64 * 64 && tailsplit == 2 && p.ntiles >= Q && p.ntiles % Q != 0 && p.ksteps >= 2 * MAX_SPLIT) {
    const int remq = p.ntiles % Q;
    int best = 1;
    double best_cost = 1.0;   // time of the tail in tile-times: ceil(rem*s/Q)/s
    for (int sp = 2; sp <= max_split; ++sp) {
      if ((long)remq * sp > 2L * num_cus * MAX_SPLIT) break;     // slab capacity of the workspace
      const double cost = (double)((remq * sp + Q - 1) / Q) / sp;
      if (cost < best_cost - 1e-9) { best_cost = cost; best = sp; }
    }
    if (best > 1) { p.split = best; p.n_main = p.ntiles - remq; }
  }
  // Uniform split (plan option UNIFORM_SPLIT = s >= 2): layers with between one and two tiles per CU (the 40x80 ones: 400
  // tiles on 256 CUs) cut EVERY tile into s equal K-ranges instead of halves of the first group + sixths of the rest
  const bool uniform = uniform_split >= 2 && BM * BN == 64 * 64 && tailsplit && p.ntiles >= num_cus && p.ntiles < 2 * num_cus &&
                       uniform_split <= max_split && p.ksteps >= 2 * MAX_SPLIT;
  if (uniform) { p.n_main = 0; p.split0 = 1; p.split = uniform_split; }
  const int rem = p.ntiles % num_cus;
  if (!uniform && (BM * BN == 64 * 64 || split_any_tile) && p.split == 1 &&   // (the bf16 big tiles are only chosen for big grids)
      rem != 0 && p.ntiles > num_cus / 2 && p.ksteps >= 2 * MAX_SPLIT && tailsplit && !(tailsplit == 2 && p.ntiles >= Q)) {
    int best = 1;
    // time of the tail in k-steps: ceil(rem * s / CUs) rounds of K / s k-steps, each visit paying `split_overhead` k-steps of
    // prologue + epilogue (plan option SPLIT_OVERHEAD; 0 = the r01 rule, which minimises ceil(rem * s / CUs) / s alone)
    const double K = (double)p.ksteps, ovh = (double)split_overhead;
    double best_cost = K + ovh;
    for (int sp = 2; sp <= max_split; ++sp) {
      const double cost = (double)((rem * sp + num_cus - 1) / num_cus) * (K / sp + ovh);
      if (cost < best_cost - 1e-9) { best_cost = cost; best = sp; }
    }
    if (best > 1) { p.split = best; p.n_main = p.ntiles - rem; }
    // One whole tile per CU next to four short K-ranges ends with that tile running alone (one wave per
    // SIMD, nothing to hide its barriers behind): such layers (CUs <= tiles < 2 CUs: the 40x80 ones) also cut
    // the first group in two.  Measured (r01): 2.750 -> 2.72 ms per frame, flat over 2..4 x 5..8.
    if (p.n_main == num_cus && p.split > 1 && p.ksteps >= 4 * MAX_SPLIT && max_split >= 2) {
      p.split0 = 2;
      if (split_overhead == 0) p.split = p.split > 6 ? 6 : p.split;   // remainder ranges not much shorter than the halves
    }
  }
  p.nb_main = p.n_main * p.split0;
  auto magic = [](int d) { return d == 1 ? 0xffffffffu : (unsigned)((1ull << 32) / (unsigned)d); };
  p.mg_mw = magic(p.Mw); p.mg_tm = magic(p.tiles_m); p.mg_tn = magic(p.tiles_n); p.mg_nc = magic(p.nclass);
  p.mg_sp0 = magic(p.split0);
  p.mg_sp = magic(p.split);
  *nblocks = p.nb_main + (p.ntiles - p.n_main) * p.split;
  *nfix = (p.split0 > 1 ? p.n_main : 0) + (p.split > 1 ? p.ntiles - p.n_main : 0);
}

// families a choice may not take: the conv-transpose halo kernels' slab-capacity fallbacks (plan_layers) choose again without them
enum { NO_CONVT_TILE8 = 1, NO_CONVT_HALO = 2 };

// The kernel of layer `li` -- the ONE place that decides it, from the layer, the plan's options, dtype, batch and CU count -- into `v`, and what follows from the
// choice into `p` (whose padding is set): the tile enumeration's classes, halo tiles per row, row parity.  Returns the K-ranges a tile may be cut into at most.
int choose_variant(const msi_net_plan *pl, int li, int exclude, ConvVariant &v, ConvParams &p) {
  const msi_net_desc *desc = &pl->desc;
  const Layer &L = pl->net.layers[li];
  const int bf16 = desc->dtype == MSI_DTYPE_BF16;
  int max_split = MAX_SPLIT;
  memset(&v, 0, sizeof(v));
  p.nclass = L.nclass;
  p.halo_tx = 0;
  // bf16: at 4 MFMAs per k-step the 64x64 tile is bound by its LDS traffic; where the grid stays large
  // (>= 4 tiles per CU) and Cout allows, the 128x128 tile (64x64 per wave) halves that traffic per flop
  const long tiles_big = (long)((L.mh * L.mw + 127) / 128) * ((L.cout + 127) / 128) * L.nclass * desc->batch;
  const int bigmode = pl->opt[MSI_NET_OPT_BIGTILE];   // 0 = never, 1 = auto, 2 = whenever Cout allows (tests)
  v.family = CONV_IGEMM; v.bm = 64; v.bn = 64; v.mode = L.kind; v.bf16 = bf16;
  if (bf16 && L.cout % 128 == 0 && bigmode != 0 && (tiles_big >= 4L * pl->num_cus || bigmode == 2)) {
    v.bm = 128; v.bn = 128;
  } else if (bf16 && L.cout % 64 == 0 && bigmode != 0 && ((tiles_big >= 4L * pl->num_cus && L.cin <= 128) || bigmode == 2)) {
    v.bm = 128; v.bn = 64;   // Cout = 64, short K (conv8_2: 495 vs 599 us; conv1_1 / conv8_1 are faster at 64x64)
  }
  const bool tile64 = v.bm == 64 && v.bn == 64;   // (the fp32 halo-patch kernels replace the 64x64 tap kernel only)
  const bool halo_ok = !((pl->opt[MSI_NET_OPT_HALO_SKIP] >> li) & 1);
  // the six-product form (plan option F32_SPLIT3) of a halo-patch layer, its fp16 form (F32_SPLIT_F16), the 8-row tiles' bit and grid rule (X3_TILE8)
  const bool x3_on = !bf16 && L.x3_off != 0 && ((pl->opt[MSI_NET_OPT_F32_SPLIT3] >> li) & 1);
  const int planes = ((pl->opt[MSI_NET_OPT_F32_SPLIT_F16] >> li) & 1) ? 2 : 3;
  const bool tile8_bit = (pl->opt[MSI_NET_OPT_X3_TILE8] >> li) & 1, tile8_force = (pl->opt[MSI_NET_OPT_X3_TILE8] >> 30) & 1;
  // halo-patch kernel (conv_halo_kernel): stride-1 3x3 layers with one source, fp32, whole 4 x 16 tiles and 32-channel chunks
  if (halo_ok && (pl->opt[MSI_NET_OPT_HALO] & 1) && !bf16 && tile64 &&
      L.kind == MODE_CONV && L.stride == 1 && L.src1 < 0 && L.in_h % 4 == 0 && L.in_w % 16 == 0 && L.c0 % 32 == 0 &&
      (L.rate == 1 || L.rate == 2)) {
    v.family = CONV_HALO; v.rate = L.rate;
    p.halo_tx = L.in_w / 16;
    if (x3_on) {
      v.family = CONV_HALO_X3; v.planes = planes;
      // the 8 x 16-pixel tile of the six-product form (conv_halo8_x3_kernel): stride 1, rate 1, whole 8-row tiles
      // where the grid stays >= 3 tiles per CU (measured at 640 x 320, profiles/r05_tile8.txt: conv1_1 215 -> 201, conv2_1 80 -> 74, conv7_2 82 -> 75, conv8_2 87 -> 81 us;
      // the 400-tile layers conv3_x / conv6_x, cut into K-ranges either way, LOSE 12 %); bit 30 of the option forces it on every eligible layer (tests)
      if (planes == 3 && L.rate == 1 && L.in_h % 8 == 0 && tile8_bit && ((long)(L.in_h / 8) * (L.in_w / 16) * ((L.cout + 63) / 64) * desc->batch >= 3L * pl->num_cus || tile8_force)) {
        v.family = CONV_HALO8_X3; v.bm = 128; v.rate = 0;
      }
      // rate-2 layers of the split kernels on row-parity tiles (conv_halo_x3_kernel<3, ...>, halo_row): the dilation along H becomes the tile's row stride --
      // a 6 x 20-pixel patch, the two-stage weight ring, three workgroups per CU (the plain rate-2 tile: 8 x 20, three stages, two)
      if (L.rate == 2 && L.in_h % 8 == 0 && ((pl->opt[MSI_NET_OPT_X3_ROWPAR] >> li) & 1)) v.rate = 3;
    }
  }
  // stride-2 halo kernel (conv_halo_s2_kernel; HALO bit 2): the stride-2 3x3 layers, fp32, one source, whole 4 x 16 tiles of the
  // OUTPUT grid, an even input (TF SAME then pads one row / column at the far side only) or wrap_pad(1, 1) + VALID
  if (halo_ok && (pl->opt[MSI_NET_OPT_HALO] & 4) && !bf16 && tile64 &&
      L.kind == MODE_CONV && L.stride == 2 && L.rate == 1 && L.src1 < 0 && L.in_h % 2 == 0 && L.in_w % 2 == 0 &&
      L.out_h % 4 == 0 && L.out_w % 16 == 0 && L.c0 % 32 == 0 && p.pad_t == p.pad_l && (p.pad_t == 0 || p.pad_t == 1) &&
      // (measured at 640 x 320: conv1_2 / conv2_2 gain their producers' ln_apply launches, -22 / -11 us for +4 / +3 us of
      // kernel time; conv3_3, 400 tiles cut into K-ranges of two groups, loses 11 us to save 6: tap kernel)
      ((long)(L.out_h / 4) * (L.out_w / 16) * (L.cout / 64) * desc->batch >= 3L * pl->num_cus ||
       // (r04: through the six-product split the halo form wins on conv3_3's 400 tiles as well: 76 -> 5x us)
       (L.x3_off != 0 && ((pl->opt[MSI_NET_OPT_F32_SPLIT3] >> li) & 1) && !(pl->opt[MSI_NET_OPT_HALO_SKIP] >> 20 & 1)))) {
    v.family = CONV_HALO_S2;
    p.halo_tx = L.out_w / 16;
    if (x3_on) {
      v.family = CONV_HALO_S2_X3; v.planes = planes;
      // ... and the stride-2 layers of the six-product form (conv_halo8_s2_x3_kernel, r05): whole 8 x 16 tiles of the OUTPUT grid, same bit and grid rule
      if (planes == 3 && L.out_h % 8 == 0 && tile8_bit && ((long)(L.out_h / 8) * (L.out_w / 16) * ((L.cout + 63) / 64) * desc->batch >= 3L * pl->num_cus || tile8_force)) {
        v.family = CONV_HALO8_S2_X3; v.bm = 128; v.planes = 0;
      }
    }
  }
  // bf16 halo-patch kernel (conv_halo_bf16_kernel): the same layers with 64-channel chunks and whole
  // 8 x 16 pixel x 128 channel or 16 x 16 x 64 tiles
  if (halo_ok && (pl->opt[MSI_NET_OPT_HALO] & 1) && bf16 && L.kind == MODE_CONV && L.stride == 1 && L.src1 < 0 && L.in_w % 16 == 0 &&
      L.c0 % 64 == 0 && bigmode != 0) {
    if (L.cout % 128 == 0 && L.in_h % 8 == 0 && (L.rate == 1 || L.rate == 2)) { v.family = CONV_HALO_BF16; v.bm = 128; v.bn = 128; v.rate = L.rate; v.waves = pl->opt[MSI_NET_OPT_BF16_WAVES] == 8 ? 8 : 4; }
    else if (L.cout == 64 && L.in_h % 16 == 0 && L.rate == 1) { v.family = CONV_HALO_BF16; v.bm = 256; v.bn = 64; v.rate = 1; v.waves = 4; }
    if (v.family == CONV_HALO_BF16) { p.halo_tx = L.in_w / 16; max_split = 1; }
  }
  // ... and its stride-2 form (conv_halo_bf16_s2_kernel; HALO bit 2): whole 8 x 16 x 128 tiles of the OUTPUT grid, an even input
  if (halo_ok && (pl->opt[MSI_NET_OPT_HALO] & 4) && bf16 && L.kind == MODE_CONV && L.stride == 2 && L.rate == 1 &&
      L.src1 < 0 && L.in_h % 2 == 0 && L.in_w % 2 == 0 && L.out_h % 8 == 0 && L.out_w % 16 == 0 && L.c0 % 64 == 0 && L.cout % 128 == 0 &&
      p.pad_t == p.pad_l && (p.pad_t == 0 || p.pad_t == 1) && bigmode != 0) {
    v.family = CONV_HALO_BF16_S2; v.bm = 128; v.bn = 128; v.waves = 4; p.halo_tx = L.out_w / 16; max_split = 1;
  }
  // conv-transpose halo kernel (convt_halo_kernel; HALO bit 1, NOT the default -- measured slower, see the kernel): SAME conv-transposes (CoordNet), fp32, whole
  // 4 x 16 input tiles and 32-channel chunks of both sources; one workgroup per output-row parity (enumerated as two "classes")
  if (!(exclude & NO_CONVT_HALO) &&
      halo_ok && ((pl->opt[MSI_NET_OPT_HALO] & 2) || (x3_on && pl->opt[MSI_NET_OPT_HALO] != 0)) && !bf16   // (HALO = 0: no halo-patch kernel at all)
      && tile64 && L.kind == MODE_CONVT && ((!L.wrapt && L.in_h % 4 == 0 && L.in_w % 16 == 0) || (L.wrapt && x3_on)) &&
      L.c0 % 32 == 0 && L.c1 % 32 == 0) {   // (wrapt: (H + 1) x (W + 5) GEMM rows per class in ragged 4 x 16 tiles -- the split form only)
    // (r04 kept msi_train_net's VALID transposes off the fp16 form: one wave's share of the layer's sum of squares came out low in ~0.1 % of
    // back-to-back forwards.  r05 found the instruction: a compiler-made `v_pk_mul_f32 d, a, b op_sel:[0,1] op_sel_hi:[1,0]` of the generic
    // epilogue's statistics -- low lane = a.lo * b.HI -- evaluated to 0 for lanes 48-63; this file is now built with -fno-slp-vectorize, which
    // is what forms that operand routing, and matryodshka_amd/build.py refuses a library that contains it.  DESIGN.md section 4, "the wobble".)
    v.family = x3_on ? CONVT_HALO_X3 : CONVT_HALO; v.planes = x3_on ? planes : 0;
    p.nclass = 2;                                      // tiles are enumerated per (ph, tile_m, tile_n, sample): a workgroup owns pw = 0, 1
    p.halo_tx = L.wrapt ? (L.mw + 15) / 16 : L.in_w / 16;
    if (L.cpt0 + L.cpt1 < max_split) max_split = L.cpt0 + L.cpt1;
    // the 8 x 16-pixel tile of the six-product conv-transpose (convt_halo8_x3_kernel, r05): same rule as the stride-1 tile (X3_TILE8: bit li, >= 3 tiles per CU or bit 30)
    if (!(exclude & NO_CONVT_TILE8) && x3_on && planes == 3 && !L.wrapt && L.in_h % 8 == 0 && tile8_bit &&
        (2L * (L.in_h / 8) * (L.in_w / 16) * ((L.cout + 63) / 64) * desc->batch >= 3L * pl->num_cus || tile8_force)) {
      v.family = CONVT_HALO8_X3; v.bm = 128; v.planes = 0;
    }
  }
  // bf16 conv-transpose halo kernel (convt_halo_bf16_kernel): SAME conv-transposes, 64-channel chunks of both sources,
  // whole 8 x 16 x 128 or 16 x 16 x 64 tiles, one workgroup per output-row parity (enumerated as two "classes")
  if (halo_ok && (pl->opt[MSI_NET_OPT_HALO] & 1) && bf16 && L.kind == MODE_CONVT && !L.wrapt &&
      L.in_w % 16 == 0 && L.c0 % 64 == 0 && L.c1 % 64 == 0 && bigmode != 0) {
    if (L.cout % 128 == 0 && L.in_h % 8 == 0) { v.family = CONVT_HALO_BF16; v.bm = 128; v.bn = 128; }
    else if (L.cout == 64 && L.in_h % 8 == 0) { v.family = CONVT_HALO_BF16; v.bm = 128; v.bn = 64; }   // (256 x 64 with two classes spills: 128 accumulator + 80 fragment registers)
    if (v.family == CONVT_HALO_BF16) { p.halo_tx = L.in_w / 16; p.nclass = 2; max_split = 1; }
  }
  if (v.is_halo()) {
    v.mode = 0; v.bf16 = 0;                                             // (arguments of the tap kernel's template only)
    p.mg_htx = p.halo_tx == 1 ? 0xffffffffu : (unsigned)((1ull << 32) / (unsigned)p.halo_tx);   // (the tap kernel does not read it: a fallback to it leaves it as it was)
    if (!v.is_convt_f32() && L.cpt0 < max_split) max_split = L.cpt0;      // K-ranges are whole chunks (bf16: whole tiles only)
  }
  p.halo_xor = (v.is_halo() && !bf16) ? 8 : 0;
  p.row_par = (v.family == CONV_HALO_X3 && v.rate == 3) ? 1 : 0;
  return max_split;
}

int plan_layers(msi_net_plan *pl) {
  const msi_net_desc *desc = &pl->desc;
  int rc = build_net(desc, pl->num_cus, pl->net);
  if (rc) return rc;
  const Net &net = pl->net;
  const int bf16 = desc->dtype == MSI_DTYPE_BF16;
  const int head_src = net.layers[MSI_NET_NUM_LAYERS - 1].src0;
  // The head (1x1, two k-steps, HBM-bound) applies its producer's LayerNorm + ReLU itself: one HBM round trip of
  // that activation less (fp32 only; option MSI_NET_OPT_HEAD_FUSE_LN = 0 restores the separate pass)
  const bool fuse_head_ln = !bf16 && pl->opt[MSI_NET_OPT_HEAD_FUSE_LN] && net.layers[head_src].cout <= HEAD_MAX_C;
  for (int li = 0; li < MSI_NET_NUM_LAYERS; ++li) {
    const Layer &L = net.layers[li];
    LayerLaunch &Q = pl->launch[li];
    memset(&Q, 0, sizeof(Q));
    ConvParams &p = Q.p;
    ConvVariant &V = Q.variant;
    p.C0 = L.c0;
    p.C1 = L.src1 >= 0 ? L.c1 : 0;
    p.cb_stride = (int)round_up(L.cout, 4);
    p.Hin = L.in_h; p.Win = L.in_w; p.Hout = L.out_h; p.Wout = L.out_w;
    p.Cout = L.cout; p.npad = L.npad;
    p.ntaps = L.ntaps; p.cpt0 = L.cpt0; p.cpt1 = L.cpt1; p.ksteps = L.ksteps;
    p.mode = L.kind;
    p.wrap = desc->coord_net ? 0 : 1;
    p.rate = L.rate;
    p.Mh = L.mh; p.Mw = L.mw;
    p.stride = 1;
    if (L.kind == MODE_CONV) {
      p.stride = L.stride;
      if (desc->coord_net) {
        // TF SAME: total = max((out-1)*s + k_eff - in, 0), floor(total/2) before
        const int keff = 2 * L.rate + 1;
        const int th = (L.out_h - 1) * L.stride + keff - L.in_h, tw = (L.out_w - 1) * L.stride + keff - L.in_w;
        p.pad_t = (th > 0 ? th : 0) / 2;
        p.pad_l = (tw > 0 ? tw : 0) / 2;
      } else {
        p.pad_t = L.rate;  // wrap_pad(x, rate, rate) + VALID (nets.py:403-421)
        p.pad_l = L.rate;
      }
    } else if (L.kind == MODE_CONVT && L.wrapt) {
      p.pad_t = 0;   // tap v reads input row mh - v and padded column mw - v = image column mw - v - 2 (tap_delta)
      p.pad_l = 2;
    }
    if (L.kind == MODE_HEAD && fuse_head_ln) {
      Q.fuse_ln = 1;
      p.ln_inv_n = 1.0 / net.layers[L.src0].ln_count;
    }
    Q.skip_apply = fuse_head_ln && li == head_src;
    // The kernel, then its tiles.  A conv-transpose halo kernel keeps two slabs per K-range: where they do not fit the partial-accumulator workspace the layer
    // chooses again without that family -- the 8-row tile falls back to the 4-row tile, the 4-row tile to the tap kernel.
    for (int exclude = 0;;) {
      const int max_split = choose_variant(pl, li, exclude, V, p);
      const bool tap_fallback = exclude & NO_CONVT_HALO;   // (has always planned without UNIFORM_SPLIT / SPLIT_OVERHEAD)
      plan_tiles(p, V.bm, V.bn, desc->batch, pl->num_cus, pl->opt[MSI_NET_OPT_TAILSPLIT], max_split, &Q.nblocks, &Q.nfix,
                 tap_fallback ? 0 : pl->opt[MSI_NET_OPT_UNIFORM_SPLIT], tap_fallback ? 0 : pl->opt[MSI_NET_OPT_SPLIT_OVERHEAD], V.tile8());
      Q.inlaunch = !pl->opt[MSI_NET_OPT_FIXUP_KERNEL] && Q.nfix <= CONV_SLOTS_PER_CU * pl->num_cus;
      const size_t slab_bytes = (size_t)(Q.nblocks - (p.split0 == 1 ? p.nb_main : 0)) * (V.is_convt_f32() ? 2 : 1) * V.bm * V.bn * sizeof(float);
      if (slab_bytes <= net.partial_bytes) break;
      if (!V.is_convt_f32()) return msi::fail(MSI_E_WORKSPACE, "conv %s: %d partial accumulators exceed the workspace", L.name, Q.nblocks);
      exclude |= V.tile8() ? NO_CONVT_TILE8 : NO_CONVT_HALO;   // (slabs of the 8-row tile do not fit: 4-row tile; two slabs per K-range do not fit: the tap kernel)
    }
    if (L.kind != MODE_HEAD) {
      const size_t per_sample = (size_t)L.out_h * L.out_w * L.cout;
      size_t blocks = (per_sample / 4 + 255) / 256;
      if (blocks > 1024) blocks = 1024;  // grid-stride
      Q.ln_blocks = (unsigned)blocks;
    }
  }
  // A layer whose EVERY consumer can apply its LayerNorm while staging a patch is never normalised in memory: halo conv
  // layers (their one source) and conv-transpose halo layers (either source).  (Until r03 the bf16 256x64 tile and the
  // bf16 conv-transpose halo kernel read bf16 copies only: with fp32 raw outputs they had no registers for the staging;
  // the fp16 raw output is 16 bytes per 8-channel slot like the copy.)
  for (int s = 0; s < MSI_NET_NUM_LAYERS - 1; ++s) {
    int consumers = 0, capable = 0;
    for (int li = s + 1; li < MSI_NET_NUM_LAYERS; ++li) {
      const Layer &L = net.layers[li];
      if (L.src0 == s || L.src1 == s) {
        ++consumers;
        const ConvVariant &C = pl->launch[li].variant;
        // (bf16 conv-transposes: only the 128 x 64 tile has registers for the staging -- 128 x 128 with APPLY spills)
        const int stage_raw = pl->opt[MSI_NET_OPT_BF16_STAGE_RAW];   // bit 0: the 256 x 64 conv tile, bit 1: the 128 x 64 conv-transpose tile
        if (C.is_convt_f32() || (C.family == CONVT_HALO_BF16 && C.bn == 64 && (stage_raw & 2)) ||
            (C.is_halo() && !C.is_convt() && L.src0 == s && (!bf16 || (L.c0 <= 512 && (C.bm != 256 || (stage_raw & 1)))))) ++capable;
      }
    }
    if (consumers > 0 && consumers == capable) {
      pl->launch[s].skip_apply = 1;
      for (int li = s + 1; li < MSI_NET_NUM_LAYERS; ++li) {
        const Layer &L = net.layers[li];
        LayerLaunch &C = pl->launch[li];
        if (C.variant.is_convt()) {
          if (L.src0 == s) { C.p.halo_apply |= 1; C.p.ln_inv_n = 1.0 / net.layers[s].ln_count; }
          if (L.src1 == s) { C.p.halo_apply |= 2; C.p.ln_inv_n1 = 1.0 / net.layers[s].ln_count; }
          if ((L.src0 == s || L.src1 == s) && C.variant.family == CONVT_HALO_BF16) C.variant.apply = 1;
        } else if (L.src0 == s) {
          C.variant.apply = 1;   // (with these: the only write to a variant after the choice)
          C.p.ln_inv_n = 1.0 / net.layers[s].ln_count;
        }
      }
    }
  }
  return MSI_OK;
}

}  // namespace

extern "C" {

// ---- plan ---------------------------------------------------------------------------------------
int msi_net_plan_create(const msi_net_desc *desc, msi_net_plan **out) {
  MSI_REQUIRE(desc && out, "net_plan_create: null pointer");
  *out = nullptr;
  msi_net_plan *pl = new (std::nothrow) msi_net_plan();
  if (!pl) return msi::fail(MSI_E_WORKSPACE, "net_plan_create: out of host memory");
  pl->desc = *desc;
  pl->num_cus = device_cu_count();
  pl->opt[MSI_NET_OPT_FIXUP_KERNEL] = 0;
  pl->opt[MSI_NET_OPT_TAILSPLIT] = 1;   // (2, the residency-aware form, measured 6-10 % slower on every layer it changes: r02_m)
  pl->opt[MSI_NET_OPT_BIGTILE] = 1;
  pl->opt[MSI_NET_OPT_HEAD_FUSE_LN] = 1;
  pl->opt[MSI_NET_OPT_NUM_CUS] = pl->num_cus;
  pl->opt[MSI_NET_OPT_HALO] = 5;   // bits 0 and 2 (bit 1, the fp32 conv-transpose halo kernel: measured slower than the tap kernel + ln_apply, see the kernel)
  pl->opt[MSI_NET_OPT_UNIFORM_SPLIT] = 0;
  pl->opt[MSI_NET_OPT_SPLIT_OVERHEAD] = 0;
  pl->opt[MSI_NET_OPT_BF16_WAVES] = 8;
  // F32_SPLIT_F16 (the three-product fp16 form) is OPT-IN: measured against fp64 it has the error of a plain fp32 convolution at half the matrix work of the
  // six-product bf16 form (profiles/r04_split_numerics.txt) -- but its operands carry 22 significand bits, not 24, and the round-3 review ruled that a
  // two-way / three-product split must not be the arithmetic a `dtype f32` number is quoted on.  The default stays the six-product form (dropped terms < 2^-26).
  pl->opt[MSI_NET_OPT_F32_SPLIT_F16] = 0;
  pl->opt[MSI_NET_OPT_X3_TILE8] = 0x3ffff;   // (r05: every eligible layer whose grid is >= 3 tiles per CU)
  pl->opt[MSI_NET_OPT_X3_ROWPAR] = 0x3ffff;  // (r05: every rate-2 layer of the split kernels)
  pl->opt[MSI_NET_OPT_F32_SPLIT3] = 0x3ffff;   // every layer that has the kernel (r04: same error against the oracle as the native path, 1.35-1.45 x faster per layer)
  pl->opt[MSI_NET_OPT_BF16_STAGE_RAW] = 1;   // (bit 1, conv8_1 staging its raw sources: measured 50 us per 16 frames SLOWER -- ~180 VALU per chunk
                                               // against 2 048 matrix cycles of the 128 x 64 tile; bit 0, conv8_2: 130 us faster.  Three interleaved repeats)
  int rc = plan_layers(pl);
  if (rc) { delete pl; return rc; }
  *out = pl;
  return MSI_OK;
}

void msi_net_plan_destroy(msi_net_plan *plan) { delete plan; }

int msi_net_plan_set_option(msi_net_plan *plan, int32_t option, int32_t value) {
  MSI_REQUIRE(plan, "net_plan_set_option: null plan");
  MSI_REQUIRE(option >= 0 && option < MSI_NET_OPT_COUNT, "net_plan_set_option: unknown option %d", option);
  if (option == MSI_NET_OPT_F32_TILE || option == MSI_NET_OPT_F32_TILE_MASK || option == MSI_NET_OPT_APPLY_AHEAD) {   // retired keys: 0 is all they take
    if (option == MSI_NET_OPT_F32_TILE) MSI_REQUIRE(value >= 0 && value <= 2, "net_plan_set_option: f32 tile %d", value);
    if (value != 0) return msi::fail(MSI_E_UNSUPPORTED, "net_plan_set_option: option %d was an experiment (measured slower) whose code this library no longer has", option);
    return MSI_OK;
  }
  if (option == MSI_NET_OPT_NUM_CUS) {
    MSI_REQUIRE(value >= 8 && value <= 4096, "net_plan_set_option: num_cus %d out of range", value);
    plan->num_cus = value;
  }
  if (option == MSI_NET_OPT_BIGTILE) MSI_REQUIRE(value >= 0 && value <= 2, "net_plan_set_option: bigtile %d", value);
  if (option == MSI_NET_OPT_HALO) MSI_REQUIRE(value >= 0 && value <= 7, "net_plan_set_option: halo %d (bit 0 conv, bit 1 conv-transpose, bit 2 stride-2 conv)", value);
  if (option == MSI_NET_OPT_TAILSPLIT) MSI_REQUIRE(value >= 0 && value <= 2, "net_plan_set_option: tailsplit %d", value);
  if (option == MSI_NET_OPT_BF16_WAVES) MSI_REQUIRE(value == 4 || value == 8, "net_plan_set_option: bf16 waves %d (4 or 8)", value);
  const int old = plan->opt[option];
  plan->opt[option] = value;
  int rc = plan_layers(plan);
  if (rc) {   // keep the plan usable
    plan->opt[option] = old;
    if (option == MSI_NET_OPT_NUM_CUS) plan->num_cus = old;
    plan_layers(plan);
  }
  return rc;
}

size_t msi_net_plan_workspace_bytes(const msi_net_plan *plan) { return plan ? plan->net.ws_bytes : 0; }

int32_t msi_net_plan_layer_is_normalized(const msi_net_plan *plan, int32_t layer) {
  if (!plan || layer < 0 || layer >= MSI_NET_NUM_LAYERS - 1) return -1;
  return plan->launch[layer].skip_apply ? 0 : 1;
}

// The kernel instantiation launch_conv launches for `layer`: the plan's record (LayerLaunch::variant, what the launchers switch on), spelled
// as rocprofv3 prints it without the namespace -- so that a parity test can assert WHICH variants a plan at a given batch
// took (the choice depends on batch x tiles vs CUs) and a profile's kernel table can be matched against tested plans.
int32_t msi_net_plan_layer_kernel(const msi_net_plan *plan, int32_t layer, char *name, size_t name_bytes, int32_t *nblocks,
                                  int32_t *nsplit_tiles) {
  MSI_REQUIRE(plan && name && name_bytes > 0, "net_plan_layer_kernel: null pointer");
  MSI_REQUIRE(layer >= 0 && layer < MSI_NET_NUM_LAYERS, "net_plan_layer_kernel: bad layer %d", layer);
  const LayerLaunch &Q = plan->launch[layer];
  const ConvVariant &V = Q.variant;
  switch (V.family) {
    case CONV_IGEMM: snprintf(name, name_bytes, "conv_igemm_kernel<%d, %d, %d, %d>", V.bm, V.bn, V.mode, V.bf16); break;
    case CONV_HALO: snprintf(name, name_bytes, "conv_halo_kernel<%d, %d>", V.rate, V.apply); break;
    case CONV_HALO_S2: snprintf(name, name_bytes, "conv_halo_s2_kernel<%d>", V.apply); break;
    case CONVT_HALO: snprintf(name, name_bytes, "convt_halo_kernel"); break;
    case CONV_HALO_X3: snprintf(name, name_bytes, "conv_halo_x3_kernel<%d, %d, %d>", V.rate, V.apply, V.planes); break;
    case CONV_HALO8_X3: snprintf(name, name_bytes, "conv_halo8_x3_kernel<%d, %d>", V.apply, V.planes); break;
    case CONV_HALO_S2_X3: snprintf(name, name_bytes, "conv_halo_s2_x3_kernel<%d, %d>", V.apply, V.planes); break;
    case CONV_HALO8_S2_X3: snprintf(name, name_bytes, "conv_halo8_s2_x3_kernel<%d>", V.apply); break;
    case CONVT_HALO_X3: snprintf(name, name_bytes, "convt_halo_x3_kernel<%d>", V.planes); break;
    case CONVT_HALO8_X3: snprintf(name, name_bytes, "convt_halo8_x3_kernel"); break;
    case CONV_HALO_BF16: snprintf(name, name_bytes, "conv_halo_bf16_kernel<%d, %d, %d, %d, %d>", V.bm, V.bn, V.rate, V.apply, V.waves); break;
    case CONV_HALO_BF16_S2: snprintf(name, name_bytes, "conv_halo_bf16_s2_kernel<%d, %d>", V.apply, V.waves); break;
    case CONVT_HALO_BF16: snprintf(name, name_bytes, "convt_halo_bf16_kernel<%d, %d, %d>", V.bm, V.bn, V.apply); break;
    default: return msi::fail(MSI_E_UNSUPPORTED, "net_plan_layer_kernel: unknown kernel family %d", V.family);
  }
  if (nblocks) *nblocks = Q.nblocks;
  if (nsplit_tiles) *nsplit_tiles = Q.nfix;
  return MSI_OK;
}

// What the kernels of `layer` are launched with, for host-side tests of the planner: the planned ConvParams (pointers null: they are per forward; the record was
// zeroed before it was filled, padding included), then inlaunch, fuse_ln, skip_apply, ln_blocks as four int32.  *needed = that many bytes; out may be null to ask.
int32_t msi_net_plan_layer_params(const msi_net_plan *plan, int32_t layer, void *out, size_t bytes, size_t *needed) {
  MSI_REQUIRE(plan && (out || needed), "net_plan_layer_params: null pointer");
  MSI_REQUIRE(layer >= 0 && layer < MSI_NET_NUM_LAYERS, "net_plan_layer_params: bad layer %d", layer);
  const LayerLaunch &Q = plan->launch[layer];
  const int32_t tail[4] = {Q.inlaunch, Q.fuse_ln, Q.skip_apply, (int32_t)Q.ln_blocks};
  if (needed) *needed = sizeof(ConvParams) + sizeof(tail);
  if (!out) return MSI_OK;
  MSI_REQUIRE(bytes >= sizeof(ConvParams) + sizeof(tail), "net_plan_layer_params: %zu bytes, %zu needed", bytes, sizeof(ConvParams) + sizeof(tail));
  memcpy(out, &Q.p, sizeof(ConvParams));
  memcpy(static_cast<char *>(out) + sizeof(ConvParams), tail, sizeof(tail));
  return MSI_OK;
}

}  // extern "C"
