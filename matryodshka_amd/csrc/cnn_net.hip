// K2, host side: the network description (build_net: layer table, offsets into the parameter blob, the packed blob and the workspace) and the host weight
// packer.  Built with the flags of the other cnn units: the packer's fixed-point window arithmetic must contract as it always has (the packed bits depend on it).
#include "cnn_plan.h"

namespace msi_cnn {

int build_net(const msi_net_desc *d, int num_cus, Net &net) {
  if (!d) return msi::fail(MSI_E_BADARG, "net: null descriptor");
  if (d->batch < 0 || d->height <= 0 || d->width <= 0 || d->in_channels <= 0 || d->num_outputs <= 0 ||
      d->ngf <= 0)
    return msi::fail(MSI_E_BADARG, "net: bad descriptor");
  if (d->height % 8 || d->width % 8)
    return msi::fail(MSI_E_UNSUPPORTED, "net: height and width must be multiples of 8 (got %dx%d)",
                     d->height, d->width);
  if (d->in_channels % 4 || d->ngf % 4)
    return msi::fail(MSI_E_UNSUPPORTED, "net: in_channels and ngf must be multiples of 4");
  if (d->dtype != MSI_DTYPE_F32 && d->dtype != MSI_DTYPE_BF16)
    return msi::fail(MSI_E_BADARG, "net: dtype %d (MSI_DTYPE_F32 or MSI_DTYPE_BF16)", d->dtype);
  const int bf16 = d->dtype == MSI_DTYPE_BF16;
  const int esz = bf16 ? 2 : 4, bke = ROW_BYTES / esz;   // operand bytes, channels per k-step
  if (bf16 && (d->in_channels % 8 || d->ngf % 8))
    return msi::fail(MSI_E_UNSUPPORTED, "net: bf16 needs in_channels and ngf in multiples of 8 (16-byte channel chunks)");
  if ((long)(d->height + 16) * (d->width + 16) >= (1L << 24))
    return msi::fail(MSI_E_UNSUPPORTED, "net: more than 2^24 pixels per sample (24-bit pixel index in the conv kernel)");
  const int ngf = d->ngf, ex = d->coord_net ? 1 : 0;
  struct Spec { const char *name; int kind, src0, src1, cout, stride, rate; };
  const Spec specs[MSI_NET_NUM_LAYERS] = {
      {"conv1_1", MODE_CONV, -1, -1, ngf, 1, 1},      {"conv1_2", MODE_CONV, 0, -1, ngf * 2, 2, 1},
      {"conv2_1", MODE_CONV, 1, -1, ngf * 2, 1, 1},   {"conv2_2", MODE_CONV, 2, -1, ngf * 4, 2, 1},
      {"conv3_1", MODE_CONV, 3, -1, ngf * 4, 1, 1},   {"conv3_2", MODE_CONV, 4, -1, ngf * 4, 1, 1},
      {"conv3_3", MODE_CONV, 5, -1, ngf * 8, 2, 1},   {"conv4_1", MODE_CONV, 6, -1, ngf * 8, 1, 2},
      {"conv4_2", MODE_CONV, 7, -1, ngf * 8, 1, 2},   {"conv4_3", MODE_CONV, 8, -1, ngf * 8, 1, 2},
      {"conv6_1", MODE_CONVT, 9, 6, ngf * 4, 2, 1},   {"conv6_2", MODE_CONV, 10, -1, ngf * 4, 1, 1},
      {"conv6_3", MODE_CONV, 11, -1, ngf * 4, 1, 1},  {"conv7_1", MODE_CONVT, 12, 3, ngf * 2, 2, 1},
      {"conv7_2", MODE_CONV, 13, -1, ngf * 2, 1, 1},  {"conv8_1", MODE_CONVT, 14, 1, ngf, 2, 1},
      {"conv8_2", MODE_CONV, 15, -1, ngf, 1, 1},      {"color_pred", MODE_HEAD, 16, -1, d->num_outputs, 1, 1},
  };
  net.layers.resize(MSI_NET_NUM_LAYERS);
  size_t poff = 0, koff = 0, woff = 0;
  for (int i = 0; i < MSI_NET_NUM_LAYERS; ++i) {
    Layer &L = net.layers[i];
    const Spec &s = specs[i];
    memset(&L, 0, sizeof(L));
    strncpy(L.name, s.name, sizeof(L.name) - 1);
    L.kind = s.kind;
    L.src0 = s.src0;
    L.src1 = s.src1;
    L.cout = s.cout;
    L.stride = s.stride;
    L.rate = s.rate;
    const int sh = s.src0 < 0 ? d->height : net.layers[s.src0].out_h;
    const int sw = s.src0 < 0 ? d->width : net.layers[s.src0].out_w;
    L.in_h = sh;
    L.in_w = sw;
    L.c0 = s.src0 < 0 ? d->in_channels : net.layers[s.src0].cout;
    L.c1 = s.src1 < 0 ? 0 : net.layers[s.src1].cout;
    if (s.src1 >= 0 && (net.layers[s.src1].out_h != sh || net.layers[s.src1].out_w != sw))
      return msi::fail(MSI_E_BADARG, "net: skip shapes disagree at %s", s.name);
    L.cin = L.c0 + L.c1;
    L.has_coord = (s.kind == MODE_CONV) ? ex : 0;
    if (s.kind == MODE_CONV) {
      L.out_h = (sh + s.stride - 1) / s.stride;
      L.out_w = (sw + s.stride - 1) / s.stride;
      L.ntaps = 9;
      L.nclass = 1;
      L.mh = L.out_h; L.mw = L.out_w;
      L.ln_count = (double)L.out_h * L.out_w * L.cout;
    } else if (s.kind == MODE_CONVT) {
      L.out_h = sh * 2;
      L.out_w = sw * 2;
      L.ntaps = 4;
      L.nclass = 4;
      L.wrapt = d->coord_net ? 0 : 1;
      if (L.wrapt) {   // nets.py:423-435: LayerNorm over the uncropped (2H+10) x (2W+10) VALID output
        L.mh = sh + 1; L.mw = sw + 5;
        L.ln_count = (double)(2 * sh + 10) * (2 * sw + 10) * L.cout;
      } else {
        L.mh = sh; L.mw = sw;
        L.ln_count = (double)L.out_h * L.out_w * L.cout;
      }
    } else {
      L.out_h = sh;
      L.out_w = sw;
      L.ntaps = 1;
      L.nclass = 1;
      L.mh = sh; L.mw = sw;
    }
    if ((size_t)sh * sw * (size_t)(L.c0 > L.c1 ? L.c0 : L.c1) * esz >= ((size_t)1 << 31))
      return msi::fail(MSI_E_UNSUPPORTED, "net: %s input exceeds 2 GiB per sample", s.name);
    L.cpt0 = (L.c0 + bke - 1) / bke;
    L.cpt1 = (L.c1 + bke - 1) / bke;
    L.ksteps = L.ntaps * (L.cpt0 + L.cpt1);   // (the CoordNet channel is not a k-step: see the bias table below)
    L.npad = (int)round_up(L.cout, NPAD_ALIGN);
    // parameter blob (reference layout)
    const size_t wf = (s.kind == MODE_CONV)    ? (size_t)9 * (L.cin + L.has_coord) * L.cout
                      : (s.kind == MODE_CONVT) ? (size_t)16 * L.cout * L.cin
                                               : (size_t)L.cin * L.cout;
    L.param_off = poff;
    L.param_floats = wf + (s.kind == MODE_HEAD ? (size_t)L.cout : (size_t)2 * L.cout);
    poff += L.param_floats;
    // packed blob
    L.packed_off = koff;
    L.packed_w_floats = (size_t)L.nclass * L.ksteps * L.npad * (ROW_BYTES / 4);   // 128-byte rows in both types
    L.gamma_off = L.packed_off + L.packed_w_floats;
    L.beta_off = L.gamma_off + round_up(L.cout, 4);
    L.lnscl_off = L.beta_off + round_up(L.cout, 4);
    L.coord_off = L.lnscl_off + 2 * LN_SCL_DOUBLES;
    koff = L.coord_off + (L.has_coord ? (size_t)L.out_h * COORD_CLASSES * round_up(L.cout, 4) : 0);
    koff = round_up(koff, 64);
    // fp32 plans: the stride-1 one-source 3x3 layers also carry their weights as three bf16 planes (plan option F32_SPLIT3):
    // [tap][chunk of 32 channels][plane][npad rows][64 B]
    if (!bf16 && ((s.kind == MODE_CONV && s.src1 < 0 && L.c0 % 32 == 0) ||
                  (s.kind == MODE_CONVT && L.c0 % 32 == 0 && L.c1 % 32 == 0))) {
      L.x3_off = koff;
      koff = round_up(koff + (size_t)L.nclass * L.ksteps * 3 * L.npad * 16, 64);
      L.x2_off = koff;   // the same rows as two fp16 planes
      koff = round_up(koff + (size_t)L.nclass * L.ksteps * 2 * L.npad * 16, 64);
    }
    // workspace
    if (s.kind != MODE_HEAD) {
      L.raw_off = woff;
      woff += round_up((size_t)d->batch * L.out_h * L.out_w * L.cout * sizeof(float), 256);
      L.aff_off = woff;
      woff += round_up((size_t)d->batch * 2 * L.cout * sizeof(float), 256);
      if (bf16) {
        L.act_off = woff;
        woff += round_up((size_t)d->batch * L.out_h * L.out_w * L.cout * 2, 256);
      }
    } else {
      L.raw_off = (size_t)-1;
      L.aff_off = (size_t)-1;
    }
  }
  if (bf16) {
    const Layer &H = net.layers.back();
    net.head_f32_ksteps = (H.c0 + 31) / 32;
    net.head_f32_npad = (int)round_up(H.cout, 64);
    net.head_f32_off = koff;
    koff = round_up(koff + (size_t)net.head_f32_ksteps * net.head_f32_npad * (ROW_BYTES / 4), 64);
  }
  net.param_floats = poff;
  net.packed_floats = koff;
  net.partial_off = woff;
  // split tiles per launch: < num_cus remainder tiles, or < 2 num_cus when the first group is split too;
  // at most MAX_SPLIT K-ranges each, 64x64 fp32 accumulators per range
  net.partial_bytes = (size_t)2 * num_cus * MAX_SPLIT * 64 * 64 * sizeof(float);
  net.zero_off = net.partial_off + net.partial_bytes;
  net.cnt_off = net.zero_off;
  size_t zoff = net.cnt_off + round_up((size_t)MSI_NET_NUM_LAYERS * CONV_SLOTS_PER_CU * num_cus * sizeof(int), 256);
  for (int i = 0; i < MSI_NET_NUM_LAYERS; ++i) {
    net.layers[i].sums_off = zoff;
    if (net.layers[i].kind != MODE_HEAD) zoff += (size_t)d->batch * LN_SHARDS * LN_WORDS * sizeof(long long);
  }
  net.err_off = zoff;   // (the sums are 1 KB per sample and layer: 256-byte aligned)
  zoff += 64;
  net.zero_bytes = zoff - net.zero_off;
  net.ws_bytes = round_up(zoff, 256);
  return MSI_OK;
}

}  // namespace msi_cnn

extern "C" {

int msi_net_layer_info(const msi_net_desc *desc, int32_t layer, msi_layer_info *out) {
  Net net;
  int rc = build_net(desc, DEFAULT_CUS, net);
  if (rc) return rc;
  MSI_REQUIRE(out && layer >= 0 && layer < MSI_NET_NUM_LAYERS, "net_layer_info: bad layer %d", layer);
  const Layer &L = net.layers[layer];
  memset(out, 0, sizeof(*out));
  strncpy(out->name, L.name, sizeof(out->name) - 1);
  out->kind = L.kind; out->cin = L.cin; out->cout = L.cout; out->has_coord = L.has_coord;
  out->stride = L.stride; out->rate = L.rate;
  out->in_h = L.in_h; out->in_w = L.in_w; out->out_h = L.out_h; out->out_w = L.out_w;
  out->param_offset = L.param_off; out->param_floats = L.param_floats;
  out->raw_offset = (uint64_t)L.raw_off; out->affine_offset = (uint64_t)L.aff_off;
  out->ln_scale_offset = (uint64_t)L.lnscl_off;
  return MSI_OK;
}

size_t msi_net_param_floats(const msi_net_desc *desc) {
  Net net;
  return build_net(desc, DEFAULT_CUS, net) ? 0 : net.param_floats;
}

size_t msi_net_packed_floats(const msi_net_desc *desc) {
  Net net;
  return build_net(desc, DEFAULT_CUS, net) ? 0 : net.packed_floats;
}

int msi_net_pack_weights_host(const msi_net_desc *desc, const float *params, float *packed) {
  Net net;
  int rc = build_net(desc, DEFAULT_CUS, net);
  if (rc) return rc;
  MSI_REQUIRE(params && packed, "net_pack_weights: null pointer");
  memset(packed, 0, net.packed_floats * sizeof(float));
  const int bf16 = desc->dtype == MSI_DTYPE_BF16;
  const int bke = bf16 ? 64 : 32;
  // element kk of a 128-byte row: 16-byte chunk (kk * esz / 16) goes to slot chunk ^ swz
  auto put_elem = [bf16](char *row, int kk, int swz, float v) {
    if (bf16) {
      uint32_t u;
      memcpy(&u, &v, 4);
      const uint16_t h = (uint16_t)((u + 0x7fffu + ((u >> 16) & 1u)) >> 16);   // round to nearest even
      memcpy(row + (((kk >> 3) ^ swz) << 4) + (kk & 7) * 2, &h, 2);
    } else {
      memcpy(row + (((kk >> 2) ^ swz) << 4) + (kk & 3) * 4, &v, 4);
    }
  };
  for (const Layer &L : net.layers) {
    const float *w = params + L.param_off;
    float *o = packed + L.packed_off;
    const int cin_w = L.cin + L.has_coord;  // channel extent of the TF weight tensor
    const int cpt = L.cpt0 + L.cpt1;
    for (int cls = 0; cls < L.nclass; ++cls) {
      const int ph = cls >> 1, pw = cls & 1;
      for (int s = 0; s < L.ksteps; ++s) {
        // k-step order of the kernel's generator: tap-major, then source 0 chunks, then source 1 chunks
        const int tap_s = s / cpt;
        const int within = s % cpt;
        const int src = within < L.cpt0 ? 0 : 1;
        const int chunk = src ? within - L.cpt0 : within;
        const int csrc = src ? L.c1 : L.c0, cbase = src ? L.c0 : 0;
        for (int n = 0; n < L.cout; ++n) {
          char *row = reinterpret_cast<char *>(o) + (((size_t)cls * L.ksteps + s) * L.npad + n) * ROW_BYTES;
          const int swz = (n >> 1) & 7;  // LDS slot j of row n holds data chunk j ^ swz (see the kernel)
          for (int kk = 0; kk < bke; ++kk) {
            if (chunk * bke + kk >= csrc) continue;
            const int tap = tap_s, c = cbase + chunk * bke + kk;
            float v;
            if (L.kind == MODE_CONV) {            // [3,3,cin_w,cout]
              v = w[((size_t)tap * cin_w + c) * L.cout + n];
            } else if (L.kind == MODE_CONVT) {    // [4,4,cout,cin]
              const int th = tap >> 1, tw = tap & 1;
              // SAME: y[2i+k-1] += x[i] w[k] (see tap_delta); VALID over the wrap-padded input: k = parity + 2 v
              const int kh = L.wrapt ? ph + 2 * th : (ph == 0 ? 1 + 2 * th : 2 - 2 * th);
              const int kw = L.wrapt ? pw + 2 * tw : (pw == 0 ? 1 + 2 * tw : 2 - 2 * tw);
              v = w[(((size_t)kh * 4 + kw) * L.cout + n) * L.cin + c];
            } else {                              // [1,1,cin,cout]
              v = w[(size_t)c * L.cout + n];
            }
            put_elem(row, kk, swz, v);
          }
        }
      }
    }
    const size_t wf = L.param_floats - (L.kind == MODE_HEAD ? (size_t)L.cout : (size_t)2 * L.cout);
    if (L.kind != MODE_HEAD) {
      // fixed-point window of this layer's LayerNorm sums (see LN_S1_BITS): e = round(log2(expected rms of the raw output)),
      // expected rms = sqrt(K) * rms(w) * rms(input), K = products per output, rms(input) = 0.5 for the sweep volume
      // (images in [-1, 1]) and sqrt(mean(gamma^2) / 2 + mean(beta^2)) for a LayerNorm + ReLU'd producer
      double sw = 0.0;
      for (size_t i = 0; i < wf; ++i) sw += (double)w[i] * (double)w[i];
      const double rms_w = sqrt(sw / (double)(wf ? wf : 1));
      auto in_ms = [&](int src) -> double {
        if (src < 0) return 0.25;
        const Layer &S = net.layers[src];
        const float *g = params + S.param_off + (S.param_floats - 2 * (size_t)S.cout), *be = g + S.cout;
        double sg = 0.0, sb = 0.0;
        for (int c = 0; c < S.cout; ++c) { sg += (double)g[c] * g[c]; sb += (double)be[c] * be[c]; }
        return 0.5 * sg / S.cout + sb / S.cout;
      };
      double ms_in = in_ms(L.src0);
      if (L.src1 >= 0) ms_in = (ms_in * L.c0 + in_ms(L.src1) * L.c1) / (double)(L.c0 + L.c1);
      const double K = (L.kind == MODE_CONV ? 9.0 : 4.0) * (double)(L.cin + L.has_coord);
      const double est = sqrt(K * ms_in) * rms_w;
      int e = (est > 0.0 && std::isfinite(est)) ? (int)lrint(log2(est)) : 0;
      e = e < -60 ? -60 : (e > 60 ? 60 : e);
      const double scl[LN_SCL_DOUBLES] = {ldexp(1.0, LN_S1_BITS - e), ldexp(1.0, LN_S2_BITS - 2 * e),
                                          ldexp(1.0, -(LN_S1_BITS - e)), ldexp(1.0, -(LN_S2_BITS - 2 * e))};
      memcpy(packed + L.lnscl_off, scl, sizeof(scl));
    }
    if (L.x3_off) {
      // x3 block (conv_halo_x3_kernel and its stride-2 / conv-transpose forms): the k-steps of the loop above, each as three planes
      // of 64-byte rows -- [class][k-step][plane h | m | l][npad][32 bf16] -- with w = h + m + l, bf16 parts by round-to-nearest-even
      // of the successive (exact) remainders; 16-byte slot j (channels 8 j .. 8 j + 7 of the chunk) of row n is stored at slot
      // j ^ ((n >> 2) & 3) (HaloGeomX3: conflict-free fragment reads)
      auto bf16_rne = [](float v) -> uint16_t {
        uint32_t u;
        memcpy(&u, &v, 4);
        return (uint16_t)((u + 0x7fffu + ((u >> 16) & 1u)) >> 16);
      };
      auto widen = [](uint16_t h) -> float {
        const uint32_t u = (uint32_t)h << 16;
        float f;
        memcpy(&f, &u, 4);
        return f;
      };
      char *base = reinterpret_cast<char *>(packed + L.x3_off);
      for (int cls = 0; cls < L.nclass; ++cls) {
        const int ph = cls >> 1, pw = cls & 1;
        for (int s = 0; s < L.ksteps; ++s) {
          const int tap = s / cpt, within = s % cpt;
          const int src = within < L.cpt0 ? 0 : 1;
          const int chunk = src ? within - L.cpt0 : within;
          const int cbase = src ? L.c0 : 0;
          for (int n = 0; n < L.cout; ++n)
            for (int kk = 0; kk < 32; ++kk) {
              const int c = cbase + chunk * 32 + kk;
              float v;
              if (L.kind == MODE_CONV) {
                v = w[((size_t)tap * cin_w + c) * L.cout + n];
              } else {   // MODE_CONVT: SAME, or VALID over the wrap-padded input (kernel index = parity + 2 tap: see tap_delta)
                const int th = tap >> 1, tw = tap & 1;
                const int kh = L.wrapt ? ph + 2 * th : (ph == 0 ? 1 + 2 * th : 2 - 2 * th);
                const int kw = L.wrapt ? pw + 2 * tw : (pw == 0 ? 1 + 2 * tw : 2 - 2 * tw);
                v = w[(((size_t)kh * 4 + kw) * L.cout + n) * L.cin + c];
              }
              uint16_t part[3];
              part[0] = bf16_rne(v);
              const float r1 = v - widen(part[0]);
              part[1] = bf16_rne(r1);
              part[2] = bf16_rne(r1 - widen(part[1]));
              const int slot = (kk >> 3) ^ ((n >> 2) & 3);
              for (int pl = 0; pl < 3; ++pl)
                memcpy(base + ((((size_t)cls * L.ksteps + s) * 3 + pl) * L.npad + n) * 64 + slot * 16 + (kk & 7) * 2, &part[pl], 2);
              // x2 block: w = h + m' 2^-11 with fp16 parts (round to nearest even; w - h is exact, m' keeps 11 of its bits:
              // 22 significand bits in all).  |w| > 65504 packs as inf and poisons the layer (LN_OVERFLOW in the status word)
              const _Float16 hh = (_Float16)v;
              const _Float16 hm = (_Float16)((v - (float)hh) * 2048.f);
              char *base2 = reinterpret_cast<char *>(packed + L.x2_off);
              memcpy(base2 + ((((size_t)cls * L.ksteps + s) * 2 + 0) * L.npad + n) * 64 + slot * 16 + (kk & 7) * 2, &hh, 2);
              memcpy(base2 + ((((size_t)cls * L.ksteps + s) * 2 + 1) * L.npad + n) * 64 + slot * 16 + (kk & 7) * 2, &hm, 2);
            }
        }
      }
    }
    if (L.kind == MODE_HEAD) {
      memcpy(packed + L.gamma_off, w + wf, L.cout * sizeof(float));  // biases
    } else {
      memcpy(packed + L.gamma_off, w + wf, L.cout * sizeof(float));
      memcpy(packed + L.beta_off, w + wf + L.cout, L.cout * sizeof(float));
    }
    if (L.has_coord) {
      // nets.add_sph_coords (nets.py:260-265): the extra input channel abs(sin(np.linspace(-pi/2, pi/2, H)))
      // (fp64 -> fp32) is constant along W and independent of the image, so its share of the 3x3
      // convolution is tabulated here instead of being computed per frame:
      //   bias[out_row][column class][n] = sum over the taps (kh,kw) that land inside the image of
      //   coord[ih] * w[kh][kw][cin][n]     (zero padding elsewhere; column classes = the two border
      //   columns on each side | interior), accumulated in fp64, stored fp32 and added to the fp32
      //   accumulators in the conv epilogue.  In the bf16 path both factors are rounded to bf16 first
      //   (they are convolution operands there).
      const double PI = 3.14159265358979323846;
      const double start = -PI / 2.0, stop = PI / 2.0;
      const int h = L.in_h;
      const double step = h > 1 ? (stop - start) / (h - 1) : 0.0;
      auto operand = [bf16](float v) -> double {
        if (!bf16) return (double)v;
        uint32_t u;
        memcpy(&u, &v, 4);
        u = (u + 0x7fffu + ((u >> 16) & 1u)) & 0xffff0000u;
        float r;
        memcpy(&r, &u, 4);
        return (double)r;
      };
      std::vector<double> coord(h);
      for (int i = 0; i < h; ++i) {
        double a = (double)i * step + start;
        if (i == h - 1 && h > 1) a = stop;
        coord[i] = operand((float)fabs(sin(a)));
      }
      const int keff = 2 * L.rate + 1;
      const int th = (L.out_h - 1) * L.stride + keff - L.in_h, tw = (L.out_w - 1) * L.stride + keff - L.in_w;
      const int pad_t = (th > 0 ? th : 0) / 2, pad_l = (tw > 0 ? tw : 0) / 2;  // TF SAME (CoordNet only)
      const int reps[COORD_CLASSES] = {0, 1, 2, L.out_w - 2, L.out_w - 1};
      const size_t cbs = round_up(L.cout, 4);
      float *tab = packed + L.coord_off;
      for (int mh = 0; mh < L.out_h; ++mh)
        for (int cc = 0; cc < COORD_CLASSES; ++cc) {
          const int mw = reps[cc];
          if (mw < 0 || mw >= L.out_w) continue;
          for (int n = 0; n < L.cout; ++n) {
            double acc = 0.0;
            for (int tap = 0; tap < 9; ++tap) {
              const int kh = tap / 3, kw = tap % 3;
              const int ih = mh * L.stride - pad_t + kh * L.rate, iw = mw * L.stride - pad_l + kw * L.rate;
              if (ih < 0 || ih >= L.in_h || iw < 0 || iw >= L.in_w) continue;
              acc += coord[ih] * operand(w[((size_t)tap * cin_w + L.cin) * L.cout + n]);
            }
            tab[((size_t)mh * COORD_CLASSES + cc) * cbs + n] = (float)acc;
          }
        }
    }
  }
  if (bf16) {   // fp32 rows of the bf16-rounded head weights (the fp32 kernels' LDS image: 32 channels per 128-byte row)
    const Layer &H = net.layers.back();
    const float *w = params + H.param_off;
    for (int ks = 0; ks < net.head_f32_ksteps; ++ks)
      for (int n = 0; n < H.cout; ++n) {
        char *row = reinterpret_cast<char *>(packed + net.head_f32_off) + ((size_t)ks * net.head_f32_npad + n) * ROW_BYTES;
        const int swz = (n >> 1) & 7;
        for (int kk = 0; kk < 32; ++kk) {
          const int c = ks * 32 + kk;
          if (c >= H.c0) continue;
          float v = w[(size_t)c * H.cout + n];
          uint32_t u;
          memcpy(&u, &v, 4);
          u = (u + 0x7fffu + ((u >> 16) & 1u)) & 0xffff0000u;
          memcpy(row + (((kk >> 2) ^ swz) << 4) + (kk & 3) * 4, &u, 4);
        }
      }
  }
  return MSI_OK;
}

}  // extern "C"
