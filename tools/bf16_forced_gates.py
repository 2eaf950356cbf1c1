#!/usr/bin/env python3
"""CPU stand-in for a bf16 network plan, and the gates of the teacher-forced layer check measured on it (no GPU, oracle code only).

The forced check (tests/util.py: forced_layer_errors) feeds each layer of the oracle the RAW outputs another implementation stored for
that layer's sources and compares the layer's own raw output.  What a correct implementation may still differ by is modelled here:

  * K summed in pieces in another order, fp32: 64-channel chunks x kernel rows, last piece first (the oracle: one torch convolution);
  * the raw output stored as fp16, round to nearest even (the oracle's "/raw" is the fp32 accumulator);
  * LayerNorm statistics taken from the unrounded accumulators (the forced oracle takes them from the stored values, two-pass in fp64),
    as fp32 sums about a pivot over shares of 1024 values, fixed-point shares, one-pass variance (cnn_device.h's epilogue);
  * the LayerNorm affine derived with fp32 operations (the oracle: fp64, rounded once) and applied with a fused multiply-add;
  * the head: another fp32 summation order (16-channel pieces, last first).

`python tools/bf16_forced_gates.py [--out profiles/bf16_forced_gates.txt]` runs the stand-in at the shapes of tests/test_gpu_bf16_forced.py
and of the two older bf16 tests that carry the forced assertion, two seeds each, and prints the worst legitimate forced error per shape, the
gates (3 x the worst, the factor of _BF16_LAYER_GATES) and the table of single-layer faults (MUTATIONS): forced error at the faulty layer
against the gates, and whether the chained per-layer gates of tests/test_gpu_bf16.py would have passed the same fault.
tests/test_bf16_forced_cpu.py asserts that table."""
import argparse
import os
import sys

import numpy as np
import torch
import torch.nn.functional as TF

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
if ROOT not in sys.path:
    sys.path.insert(0, ROOT)
from oracle import nets as onets  # noqa: E402

F32 = np.float32
# (batch, H, W, Cin, Cout, ngf), coord_net: tests/test_gpu_bf16_forced.py, then test_gpu_decomposition.py's D and test_gpu_bf16.py's per-layer test
GATE_SHAPES = [((1, 64, 128, 64, 16, 64), True), ((1, 64, 128, 64, 16, 64), False), ((2, 32, 64, 64, 16, 32), True),
               ((2, 16, 40, 24, 8, 16), True), ((2, 16, 40, 24, 8, 16), False),
               ((2, 32, 128, 64, 16, 64), False), ((1, 64, 128, 96, 32, 32), True),
               ((1, 64, 128, 16, 8, 144), True), ((1, 32, 64, 64, 128, 32), True), ((1, 32, 64, 64, 64, 32), True),
               ((1, 32, 64, 64, 16, 32), True), ((1, 32, 64, 64, 16, 32), False)]      # (tests/test_bf16_forced_cpu.py; its batch-2 CoordNet case is above)
GATE_SEEDS = (101, 202)
MUTATION_SHAPE = (1, 32, 64, 64, 16, 32)
# name -> (fault, layer whose arithmetic is faulty, coord_net, batch, layers that miss a forced gate): each fault is confined to ONE layer and seen at that layer
# alone -- except the truncating store.  The statistics come from the accumulators, so stored values that lean towards zero no longer have the variance they are
# normalised with; the forced oracle of the CONSUMER derives the statistics from the stored values, gets another scale (by the lean: ~6e-5) and sees every
# output of the consumer off in proportion (its bias gate).  One fault, seen from both sides of the buffer.
MUTATIONS = {
    "activations truncated to bf16 while staging": ("trunc_act", "conv4_2", True, 1, ["conv4_2"]),
    "fp16 store truncates": ("trunc_store", "conv6_3", True, 1, ["conv6_3", "conv7_1"]),
    "one tap of one 64-channel chunk dropped in one tile": ("drop_tap", "conv6_3", True, 1, ["conv6_3"]),
    "left wrap column from the wrong side in one tile": ("wrap_left", "conv3_2", False, 1, ["conv3_2"]),
    "LayerNorm shift of sample 0 from sample 1's mean": ("ln_shift", "conv7_2", True, 2, ["conv7_2"]),
}
DEVICE_MARK = "==== observed on the device"
MSI_TANH_ERR = 2.0e-7       # cnn_device.h msi_tanh: absolute error against fp64 (exp2 / rcp of the hardware), which torch.tanh here does not have
TILE = (slice(None), slice(0, 128), slice(0, 8), slice(0, 16))       # one 8 x 16-pixel x 128-channel tile (NCHW)


def trunc_bf16(t):
    """fp32 -> bf16 by dropping the low 16 bits (what a staging path that forgets the rounding add does)."""
    return (t.contiguous().view(torch.int32) & -65536).view(torch.float32)


def trunc_f16(t):
    """fp32 -> fp16 toward zero -> fp32."""
    a = t.numpy()
    h = a.astype(np.float16)
    u = h.view(np.uint16)
    u[np.abs(h.astype(F32)) > np.abs(a)] -= 1        # (sign-magnitude: one step towards zero)
    return torch.from_numpy(h.astype(F32))


def _pieces(c, k):
    """(channel range, kernel row) pieces of a K = k rows x c channels reduction, in the stand-in's order: last first."""
    return [(c0, min(c0 + 64, c), ky) for c0 in range(0, c, 64) for ky in range(k)][::-1]


def _summed(fn, x, w, k, cin_axis):
    """sum over _pieces of fn(x's channels, w's channels and kernel row, kernel row), fp32, last piece first."""
    y = None
    for c0, c1, ky in _pieces(x.shape[1], k):
        part = fn(x[:, c0:c1], w.narrow(cin_axis, c0, c1 - c0)[:, :, ky:ky + 1, :], ky)
        y = part if y is None else y + part
    return y


def _wave_statistics(y):
    """Per-sample mean and 1 / sqrt(var + eps) [B,1,1,1] fp64 of the fp32 accumulators y, the way the kernels' epilogue takes them (cnn_device.h):
    d = y - pivot, sum d and sum d^2 in fp32 over shares of 1024 values, every share rounded to one fixed-point unit (2^(e - 24) resp.
    2^(2 e - 16), 2^e ~ the rms), the shares added exactly, one-pass variance in fp64."""
    b = y.shape[0]
    n = y[0].numel()
    flat = y.reshape(b, n)
    pivot = flat[:, :1]
    d = TF.pad(flat - pivot, (0, -n % 1024)).reshape(b, -1, 1024)
    e = torch.round(torch.log2(flat.double().pow(2).mean(dim=1, keepdim=True).sqrt()))
    u1, u2 = torch.exp2(e - 24), torch.exp2(2 * e - 16)
    s1 = (torch.round(d.sum(dim=2).double() / u1) * u1).sum(dim=1, keepdim=True)
    s2 = (torch.round((d * d).sum(dim=2).double() / u2) * u2).sum(dim=1, keepdim=True)
    p = pivot.double()
    mu = (n * p + s1) / n
    var = ((s2 + 2 * p * s1 + n * p * p) / n - mu * mu).clamp_min(0.0)
    return mu.view(b, 1, 1, 1), torch.rsqrt(var + onets.LN_EPS).view(b, 1, 1, 1)


def standin_forward(weights, net_input, coord_net=True, mutate=None):
    """The bf16 network as a correct device plan may compute it (module docstring).  net_input: [B,H,W,Cin] fp32, bf16-representable.
    mutate: None | (fault, layer) of MUTATIONS.  Returns (prediction [B,H,W,Cout], {layer: stored raw output [B,H,W,C] fp32}) -- for
    msi_train_net's conv-transposes the stored raw output is the [5:-5] crop, as in a plan's workspace."""
    fault, where = mutate or (None, None)
    rnd = onets.bf16_round
    x = rnd(torch.from_numpy(np.ascontiguousarray(np.transpose(net_input, (0, 3, 1, 2)))).float())
    acc, stored = {}, {}

    def finish(name, y):
        acc[name] = y                                                    # fp32 accumulators: the statistics' source
        stored[name] = trunc_f16(y) if (fault == "trunc_store" and where == name) else y.half().float()

    def activation(src, consumer, crop=0):
        """LayerNorm + ReLU + bf16 rounding of layer `src` as `consumer` stages it."""
        mean, inv = _wave_statistics(acc[src])
        g = torch.from_numpy(weights[src + "/LayerNorm/gamma"]).view(1, -1, 1, 1)
        be = torch.from_numpy(weights[src + "/LayerNorm/beta"]).view(1, -1, 1, 1)
        if fault == "ln_shift" and where == consumer:
            mean = torch.cat([mean[1:2], mean[1:]], dim=0)               # sample 0's shift from sample 1's mean
        # the affine from fp32 operations only, the mean as hi + lo floats (the staging kernels of cnn_bf16.hip; the oracle rounds fp64 values once),
        # and applied with a fused multiply-add (products of two floats are exact in fp64)
        scale = inv.float() * g
        mu_hi = mean.float()
        mu_lo = (mean - mu_hi.double()).float()
        shift = (be.double() - mu_hi.double() * scale.double()).float()
        shift = (shift.double() - mu_lo.double() * scale.double()).float()
        y = torch.relu((stored[src].double() * scale.double() + shift.double()).float())
        if crop:
            y = y[:, :, crop:-crop, crop:-crop]
        return trunc_bf16(y) if (fault == "trunc_act" and where == consumer) else rnd(y)

    def conv(name, x, stride=1, rate=1):
        w = rnd(onets._conv_w(weights[name + "/weights"]))
        x0 = x
        if coord_net:
            x = rnd(onets.add_sph_coords(x))
            pt, pb = onets._same_pad(x.shape[2], 2 * rate + 1, stride)
            pl, pr = onets._same_pad(x.shape[3], 2 * rate + 1, stride)
            x = TF.pad(x, (pl, pr, pt, pb))
        else:
            x = onets.wrap_pad(x, rate, rate)
        hout = (x.shape[2] - (2 * rate + 1)) // stride + 1

        def piece(xc, wc, ky):       # kernel row ky alone: the input rows it reads
            return TF.conv2d(xc[:, :, ky * rate:ky * rate + (hout - 1) * stride + 1], wc, stride=stride, dilation=rate)
        y = _summed(piece, x, w, 3, 1)
        if fault == "drop_tap" and where == name:                        # tap (0, 2) of channels 64 .. 127, in one tile
            wt = torch.zeros_like(w)
            wt[:, 64:128, 0, 2] = w[:, 64:128, 0, 2]
            y = y.clone()
            y[TILE] -= TF.conv2d(x, wt, stride=stride, dilation=rate)[TILE]
        if fault == "wrap_left" and where == name:                       # the left pad column read from column 0 instead of column W - 1
            xw = TF.pad(torch.cat([x0[..., :rate], x0, x0[..., :rate]], dim=-1), (0, 0, rate, rate))
            y = y.clone()
            y[TILE] = _summed(piece, xw, w, 3, 1)[TILE]
        finish(name, y)

    def convT(name, x):
        w = rnd(onets._convT_w(weights[name + "/weights"]))               # [Cin, Cout, 4, 4]
        pad = 1 if coord_net else 0
        if not coord_net:
            x = onets.wrap_pad(x, 2, 2)
        hin = x.shape[2]

        def piece(xc, wc, ky):       # kernel row ky alone lands on output rows 2 i + ky - pad: the full-height transpose of a one-row kernel, shifted
            full = TF.conv_transpose2d(xc, wc, stride=2, padding=(0, pad))                       # [.., 2 hin - 1, ..] rows 2 i
            out = torch.zeros(full.shape[0], full.shape[1], 2 * hin + 2 - 2 * pad, full.shape[3])
            lo = ky - pad
            src = full[:, :, max(0, -lo):, :]
            n = min(src.shape[2], out.shape[2] - max(0, lo))
            out[:, :, max(0, lo):max(0, lo) + n] = src[:, :, :n]
            return out
        finish(name, _summed(piece, x, w, 4, 0))

    with torch.no_grad():
        conv("conv1_1", x)
        chain = [("conv1_2", "conv1_1", 2, 1), ("conv2_1", "conv1_2", 1, 1), ("conv2_2", "conv2_1", 2, 1), ("conv3_1", "conv2_2", 1, 1),
                 ("conv3_2", "conv3_1", 1, 1), ("conv3_3", "conv3_2", 2, 1), ("conv4_1", "conv3_3", 1, 2), ("conv4_2", "conv4_1", 1, 2),
                 ("conv4_3", "conv4_2", 1, 2)]
        for name, src, stride, rate in chain:
            conv(name, activation(src, name), stride=stride, rate=rate)
        crop = 0 if coord_net else 5
        convT("conv6_1", torch.cat([activation("conv4_3", "conv6_1"), activation("conv3_3", "conv6_1")], dim=1))
        conv("conv6_2", activation("conv6_1", "conv6_2", crop))
        conv("conv6_3", activation("conv6_2", "conv6_3"))
        convT("conv7_1", torch.cat([activation("conv6_3", "conv7_1"), activation("conv2_2", "conv7_1")], dim=1))
        conv("conv7_2", activation("conv7_1", "conv7_2", crop))
        convT("conv8_1", torch.cat([activation("conv7_2", "conv8_1"), activation("conv1_2", "conv8_1")], dim=1))
        conv("conv8_2", activation("conv8_1", "conv8_2", crop))
        a = activation("conv8_2", "color_pred")
        w = rnd(onets._conv_w(weights["color_pred/weights"]))
        y = None
        for c0 in range(0, a.shape[1], 16)[::-1]:
            part = TF.conv2d(a[:, c0:c0 + 16], w[:, c0:c0 + 16])
            y = part if y is None else y + part
        pred = torch.tanh(y + torch.from_numpy(weights["color_pred/biases"]).view(1, -1, 1, 1))
    raws = {}
    for name, t in stored.items():
        if not coord_net and name in ("conv6_1", "conv7_1", "conv8_1"):
            t = t[:, :, 5:-5, 5:-5]
        raws[name] = np.ascontiguousarray(t.permute(0, 2, 3, 1).numpy())
    return np.ascontiguousarray(pred.permute(0, 2, 3, 1).numpy()), raws


def make_case(shape, coord, seed):
    b, h, w, cin, nout, ngf = shape
    weights = onets.init_weights(cin, nout, ngf=ngf, coord_net=coord, seed=seed, randomize_affine=True)
    x = onets.bf16_round(np.random.RandomState(seed + 1).uniform(-1, 1, size=(b, h, w, cin)).astype(F32))
    return weights, x


def chained_errors(weights, x, coord, raws):
    """{layer: (max, mean)} of |stand-in - FREE-RUNNING bf16 oracle| relative to the layer scale: what the older per-layer tests measure."""
    _, acts = onets.forward(weights, x, coord_net=coord, return_activations=True, bf16=True)
    out = {}
    for name, raw in raws.items():
        o = acts[name + "/raw"]
        e = np.abs(raw - o) / np.abs(o).max()
        out[name] = (float(e.max()), float(e.mean()))
    return out


def main():
    from tests.util import BF16_FORCED_GATES, forced_gates, forced_layer_errors
    from tests.test_gpu_bf16 import _BF16_LAYER_GATES
    ap = argparse.ArgumentParser(description=__doc__.split("\n")[0])
    ap.add_argument("--out", help="also write the report to this file")
    args = ap.parse_args()
    torch.manual_seed(0)
    lines = []

    def say(s=""):
        print(s)
        lines.append(s)

    say("legitimate stand-in against the forced oracle (max, mean of |stand-in - oracle| / max |oracle raw|; head absolute; bias: module docstring of tests/util.py)")
    keys = ("layer_max", "layer_mean", "layer_bias", "head_max", "head_mean")
    worst = {}
    for shape, coord in GATE_SHAPES:
        for seed in GATE_SEEDS:
            weights, x = make_case(shape, coord, seed)
            pred, raws = standin_forward(weights, x, coord)
            rep = forced_layer_errors(weights, x, coord, raws, pred)
            lm = max(rep["layers"].items(), key=lambda kv: kv[1][0])
            ln_ = max(rep["layers"].items(), key=lambda kv: kv[1][1])
            lb = max(rep["bias"].items(), key=lambda kv: abs(kv[1]))
            fm = max(chained_errors(weights, x, coord, raws).items(), key=lambda kv: kv[1][0])
            say("  %-24s %-5s seed %3d: worst max %.2e (%s)  worst mean %.2e (%s)  worst |bias| %.2e (%s)  head %.2e / %.2e   [free-running: worst max %.2e (%s)]"
                % ("x".join(map(str, shape)), "coord" if coord else "wrap", seed, lm[1][0], lm[0], ln_[1][1], ln_[0], abs(lb[1]), lb[0],
                   rep["head"][0], rep["head"][1], fm[1][0], fm[0]))
            w_ = worst.setdefault(shape[5], dict.fromkeys(keys, 0.0))
            for k, v in zip(keys, (lm[1][0], ln_[1][1], abs(lb[1]), rep["head"][0] + MSI_TANH_ERR, rep["head"][1] + MSI_TANH_ERR)):
                w_[k] = max(w_[k], v)
    say("worst legitimate value and gate (3 x) per network width ngf (head: + %.1e, the documented error of the kernels' tanh):" % MSI_TANH_ERR)
    for ngf in sorted(worst):
        say("  ngf %2d: worst " % ngf + "  ".join("%s %.2e" % (k, worst[ngf][k]) for k in keys))
        say("          gate  " + "  ".join("%s %.2e" % (k, 3 * worst[ngf][k]) for k in keys))
    say("gates in tests/util.py (ngf >= 64 takes those of 64, tests.util.forced_gates: the runs at 144 stay below every worst value of 64):")
    for ngf in sorted(BF16_FORCED_GATES):
        say("  ngf %2d: " % ngf + "  ".join("%s %.2e" % (k, BF16_FORCED_GATES[ngf][k]) for k in keys))
    say()
    say("single-layer faults at %s (forced error AT the faulty layer; 'chained' = the free-running comparison under _BF16_LAYER_GATES)" % "x".join(map(str, MUTATION_SHAPE)))
    for what, (fault, layer, coord, batch, _) in MUTATIONS.items():
        shape = (batch,) + MUTATION_SHAPE[1:]
        weights, x = make_case(shape, coord, GATE_SEEDS[0])
        pred, raws = standin_forward(weights, x, coord, mutate=(fault, layer))
        rep = forced_layer_errors(weights, x, coord, raws, pred, gates=forced_gates(shape[5]))
        ch = chained_errors(weights, x, coord, raws)
        chained_fail = [n for n, (mx, mn) in ch.items() if mx > _BF16_LAYER_GATES[n][0] or mn > _BF16_LAYER_GATES[n][1]]
        say("  %-52s %-8s forced: max %.2e mean %.2e bias %+.2e -> fails at %s | chained: max %.2e mean %.2e -> %s"
            % (what, layer, rep["layers"][layer][0], rep["layers"][layer][1], rep["bias"][layer], ",".join(rep["failed_layers"]) or "NOTHING",
               ch[layer][0], ch[layer][1], ("fails at " + ",".join(chained_fail)) if chained_fail else "PASSES"))
    if args.out:        # (what a device gave is kept below DEVICE_MARK in the same file, by hand: an observation, no input of this tool)
        kept = ""
        if os.path.exists(args.out):
            old = open(args.out).read()
            kept = old[old.index(DEVICE_MARK):] if DEVICE_MARK in old else ""
        with open(args.out, "w") as f:
            f.write("\n".join(lines) + "\n" + kept)


if __name__ == "__main__":
    main()
