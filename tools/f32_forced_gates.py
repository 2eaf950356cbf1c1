#!/usr/bin/env python3
"""Gates of the teacher-forced fp64 check of the fp32 network tier, measured on the CPU (no GPU, oracle code only), and the single-layer faults it must see.

The check (tests/util.py: forced_layer_errors_f32) recomputes every layer in fp64 from the tensors an fp32 plan stored for that layer's own sources.  What a CORRECT
kernel may differ from that by is its arithmetic: six bf16 products with fp32 accumulation ("x3"), three fp16 products ("f16"), or plain fp32 ("native"), the
LayerNorm affine of its input applied in fp32.  The stand-in for each is the oracle's own emulation, forced on the same tensors:

    forward(split3_products=True | "f16" | False, forced_raw=R)    against    forward(precision="fp64", forced_raw=R),       R = the fp32 oracle's raw outputs,

at shapes A, B, C and E of tests/test_plan_decomposition.py, each at ngf 32 and 64, GATE_SEEDS weight / input seeds each.  The gate per arithmetic and metric
(layer max, layer rms, head max, head rms) is 3 x the worst stand-in value over all layers, shapes and seeds: the stand-in sums in another order than a kernel and
applies the affine without a fused multiply-add (the factor of the bf16 tier's forced gates).  The head's gates are derived the same way, from the stand-in's tanh output alone.

Then the faults (FAULTS x FAULT_LAYERS, at MUTATION_SHAPE): the stand-in FREE-RUNNING with ONE term of ONE layer's product form wrong -- everything downstream
computed from the faulty output, as on a device -- checked by forced_layer_errors_f32 under the gates of tests/util.py and by the older free-running gates
(2e-4 of the layer scale, 6e-4 for the fp16 form, against the fp32 oracle).  Operand order in a term's name: activation part . weight part.

`python tools/f32_forced_gates.py [--out profiles/f32_forced_gates.txt] [--seeds N]`; tests/test_f32_forced_cpu.py asserts the fault table."""
import argparse
import os
import sys

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
if ROOT not in sys.path:
    sys.path.insert(0, ROOT)
from oracle import nets as onets  # noqa: E402

F32 = np.float32
# (batch, H, W, Cin, Cout, ngf), coord_net: shapes A, B, C, E of tests/test_plan_decomposition.py, at both widths
_BASE = [("A", (1, 64, 128, 96, 32), True), ("B", (1, 32, 384, 96, 32), True), ("C", (3, 64, 128, 96, 32), False), ("E", (1, 32, 128, 96, 32), False)]
GATE_SHAPES = [(n, s + (ngf,), coord) for n, s, coord in _BASE for ngf in (32, 64)]
GATE_SEEDS = (101, 202, 303, 404, 505)
ARITHMETICS = {"x3": True, "f16": "f16", "native": False}      # name -> forward's split3_products
KEYS = ("layer_max", "layer_rms", "head_max", "head_rms")
DEVICE_MARK = "==== observed on the device"

MUTATION_SHAPE = (1, 32, 64, 32, 8, 32)
MUTATION_SEED = 101
# fault -> (product form, what is wrong)
FAULTS = {
    "drop_mm": ("x3", "m.m dropped"),
    "drop_hl": ("x3", "h.l dropped (the weights' l plane unused)"),
    "drop_lh": ("x3", "l.h dropped (the patch's l plane unused)"),
    "wl_roll": ("x3", "the weights' l plane rolled by one output channel"),
    "xl_shift": ("x3", "the patch's l plane taken from the neighbouring pixel"),
    "drop_lh_krange": ("x3", "l.h dropped in one K-range (the second half of the input channels) only"),
    "drop_hm": ("f16", "h.m' dropped"),
    "drop_mh": ("f16", "m'.h dropped"),
}
# layer kind -> layer
FAULT_LAYERS = {"stride 1": "conv2_1", "stride 2": "conv2_2", "rate 2": "conv4_2", "conv-transpose": "conv7_1", "conv8_2": "conv8_2"}
CONVT = ("conv6_1", "conv7_1", "conv8_1")
OLD_GATES = {"x3": 2e-4, "f16": 6e-4}      # tests/test_gpu_decomposition.py _check_case: per layer, of the layer scale, against the free-running fp32 oracle
# a kernel name of each arithmetic, as msi_net_plan_layer_kernel spells it (tests.util.f32_arithmetic reads the arithmetic off it)
KERNEL_OF = {"x3": "conv_halo_x3_kernel<1, 0, 3>", "f16": "conv_halo_x3_kernel<1, 0, 2>", "native": "conv_igemm_kernel<64, 64, 0, 0>"}


def layer_names():
    return [t[0] for t in onets.layer_table(1, 1) if t[1] != "h"]


def kernels_of(arith):
    """18 (kernel, 0, 0) entries in plan.kernels()'s form: every layer and the head on the arithmetic `arith`."""
    return [(KERNEL_OF[arith], 0, 0)] * 18


def make_case(shape, coord, seed):
    b, h, w, cin, nout, ngf = shape
    weights = onets.init_weights(cin, nout, ngf=ngf, coord_net=coord, seed=seed, randomize_affine=True)
    x = np.random.RandomState(seed + 1).uniform(-1, 1, size=(b, h, w, cin)).astype(F32)
    return weights, x


def faulty_products(form, fault=None, layer=None):
    """forward's split3_products as a callable: the product form `form` ("x3" | "f16") on every layer, with `fault` (FAULTS) in `layer` alone."""
    def products(name, fn, x, w):
        if name != layer or fault is None:
            return (onets.conv_split_f16 if form == "f16" else onets.conv_split3)(fn, x, w)
        assert FAULTS[fault][0] == form, (fault, form)
        if form == "f16":
            xh, xm = onets.split_f16(x)
            wh, wm = onets.split_f16(w)
            mh = fn(xm, wh)
            hm = fn(xh, wm)
            if fault == "drop_mh":
                mh = torch.zeros_like(mh)
            if fault == "drop_hm":
                hm = torch.zeros_like(hm)
            return fn(xh, wh) + (mh + hm) * (1.0 / 2048.0)
        xh, xm, xl = onets.split3(x)
        wh, wm, wl = onets.split3(w)
        if fault == "wl_roll":
            wl = torch.roll(wl, 1, dims=1 if name in CONVT else 0)      # output channels: [Cout, Cin, kh, kw], conv-transposes [Cin, Cout, kh, kw]
        if fault == "xl_shift":
            xl = torch.roll(xl, 1, dims=3)
        if fault == "drop_lh_krange":
            xl = xl.clone()
            xl[:, xl.shape[1] // 2:] = 0
        mm, lh, hl = fn(xm, wm), fn(xl, wh), fn(xh, wl)
        if fault == "drop_mm":
            mm = torch.zeros_like(mm)
        if fault == "drop_lh":
            lh = torch.zeros_like(lh)
        if fault == "drop_hl":
            hl = torch.zeros_like(hl)
        return ((mm + lh) + hl) + ((fn(xm, wh) + fn(xh, wm)) + fn(xh, wh))      # (conv_split3's order)
    return products


def device_standin(weights, x, coord, form, fault=None, layer=None, normalized=()):
    """What a plan of product form `form` would leave behind, from the oracle's emulation running FREE (each layer fed its own upstream results, the faulty layer's
    included): (prediction, {layer: stored tensor} -- the activation for the layers in `normalized`, the raw output otherwise)."""
    pred, acts = onets.forward(weights, x, coord_net=coord, return_activations=True, split3_products=faulty_products(form, fault, layer))
    return pred, {n: (acts[n] if n in normalized else acts[n + "/raw"]) for n in layer_names()}


def free_running_errors(coord, stored, normalized=()):
    """{layer: max |stored - FREE-RUNNING fp32 oracle| / max |oracle|} of the mutation case: what the older per-layer tests measure."""
    ref, acts = _fp32_oracle(coord)
    out = {}
    for name, t in stored.items():
        o = acts[name] if name in normalized else acts[name + "/raw"]
        out[name] = float(np.abs(t - o).max() / np.abs(o).max())
    return out


_FP32 = {}


def _fp32_oracle(coord):
    """(prediction, activations) of the free-running fp32 oracle on mutation_case(coord): computed once per (coord, shape, seed), never written."""
    key = (coord, MUTATION_SHAPE, MUTATION_SEED)
    if key not in _FP32:
        weights, x = mutation_case(coord)
        _FP32[key] = onets.forward(weights, x, coord_net=coord, return_activations=True)
    return _FP32[key]


def standin_errors(weights, x, coord):
    """{arithmetic: ({layer: (max, rms)}, (head max, head rms))} of each arithmetic's emulation against the fp64 forward, both forced on the fp32 oracle's raw outputs."""
    from tests.util import rel_max_rms
    names = layer_names()
    _, acts = onets.forward(weights, x, coord_net=coord, return_activations=True)
    forced = {n: acts[n + "/raw"] for n in names}
    p64, a64 = onets.forward(weights, x, coord_net=coord, return_activations=True, precision="fp64", forced_raw=forced)
    out = {}
    for arith, products in ARITHMETICS.items():
        p, a = onets.forward(weights, x, coord_net=coord, return_activations=True, split3_products=products, forced_raw=forced)
        out[arith] = ({n: rel_max_rms(a[n + "/raw"], a64[n + "/raw"]) for n in names}, rel_max_rms(p, p64))
    return out


def fault_report(fault, layer, coord=True, normalized=()):
    """(forced report under the gates of tests/util.py, {layer: free-running error}, free-running error of the prediction) of the stand-in with `fault` in `layer`
    (fault None: the fault-free stand-in of `layer`, a product form's name)."""
    from tests.util import F32_FORCED_GATES, forced_layer_errors_f32
    form = FAULTS[fault][0] if fault else layer
    weights, x = mutation_case(coord)
    pred, stored = device_standin(weights, x, coord, form, fault, layer, normalized)
    rep = forced_layer_errors_f32(weights, x, coord, stored, normalized, pred, gates=F32_FORCED_GATES, kernels=kernels_of(form))
    ref, _ = _fp32_oracle(coord)
    return rep, free_running_errors(coord, stored, normalized), float(np.abs(pred - ref).max())


def chain_model(cin, cout, npix, kstep=16, nsplit=1, seed=0):
    """An EXPLANATION, never a gate: one 3 x 3 layer as a GEMM (K = 9 cin) in the six-product form, (a) as the oracle emulates it -- one fp32 GEMM per term, the terms
    added smallest first -- and (b) with all six products of a k-step added into ONE fp32 accumulator (cnn_x3.hip split_mfma<6>: the 8-row conv-transpose tile; split_mfma<3> keeps the small
    products in a second accumulator because of what this shows), k-steps of 16, a tile
    cut into `nsplit` K-ranges summed at the end): exact products, one rounding per accumulate.  Returns ((max, rms) of a, (max, rms) of b) against fp64."""
    from tests.util import rel_max_rms
    g = torch.Generator().manual_seed(seed)
    k = 9 * cin
    x = torch.relu(torch.randn(npix, k, generator=g) * 0.8 + 0.1)                                   # activations after LayerNorm + ReLU
    w = (torch.rand(k, cout, generator=g) * 2 - 1) * (6.0 / (9 * cin + 9 * cout)) ** 0.5            # Xavier
    ref = (x.double() @ w.double()).numpy()
    (xh, xm, xl), (wh, wm, wl) = onets.split3(x), onets.split3(w)
    terms = [(xm, wm), (xl, wh), (xh, wl), (xm, wh), (xh, wm), (xh, wh)]
    emu = sum((a @ b for a, b in terms[1:]), terms[0][0] @ terms[0][1])
    per = k // nsplit
    parts = []
    for s in range(nsplit):
        acc = torch.zeros(npix, cout)
        for k0 in range(s * per, (s + 1) * per, kstep):
            for a, b in terms:
                acc = (acc.double() + a[:, k0:k0 + kstep].double() @ b[k0:k0 + kstep].double()).float()
        parts.append(acc)
    return rel_max_rms(emu.numpy(), ref), rel_max_rms(sum(parts[1:], parts[0]).numpy(), ref)


_CASES = {}


def mutation_case(coord):
    key = (coord, MUTATION_SHAPE, MUTATION_SEED)
    if key not in _CASES:
        _CASES[key] = make_case(MUTATION_SHAPE, coord, MUTATION_SEED)
    return _CASES[key]


def main():
    from tests.util import F32_FORCED_GATES
    ap = argparse.ArgumentParser(description=__doc__.split("\n")[0])
    ap.add_argument("--out", help="also write the report to this file")
    ap.add_argument("--seeds", type=int, default=len(GATE_SEEDS), help="seeds per shape (default: all %d)" % len(GATE_SEEDS))
    ap.add_argument("--skip-gates", action="store_true", help="the fault table only")
    args = ap.parse_args()
    lines = []

    def say(s=""):
        print(s, flush=True)
        lines.append(s)

    names = layer_names()
    worst = {a: dict.fromkeys(KEYS, 0.0) for a in ARITHMETICS}
    if not args.skip_gates:
        say("stand-in of each arithmetic against forward(precision='fp64'), both forced on the fp32 oracle's raw outputs: worst layer max (of the fp64 tensor's max-abs), "
            "worst layer rms (of its rms), head max / rms (of the fp64 tanh output's max-abs / rms)")
        for sname, shape, coord in GATE_SHAPES:
            for seed in GATE_SEEDS[:args.seeds]:
                weights, x = make_case(shape, coord, seed)
                for arith, (layers, head) in standin_errors(weights, x, coord).items():
                    lm = max(layers.items(), key=lambda kv: kv[1][0])
                    lr = max(layers.items(), key=lambda kv: kv[1][1])
                    say("  %s %-22s %-5s seed %3d %-6s: layer max %.3e (%s)  layer rms %.3e (%s)  head %.3e / %.3e"
                        % (sname, "x".join(map(str, shape)), "coord" if coord else "wrap", seed, arith, lm[1][0], lm[0], lr[1][1], lr[0], head[0], head[1]))
                    say("      per layer max: " + " ".join("%.2e" % layers[n][0] for n in names))
                    say("      per layer rms: " + " ".join("%.2e" % layers[n][1] for n in names))
                    for k, v in zip(KEYS, (lm[1][0], lr[1][1], head[0], head[1])):
                        worst[arith][k] = max(worst[arith][k], v)
        say()
        say("worst stand-in value and gate (3 x) per arithmetic:")
        for arith in ARITHMETICS:
            say("  %-6s worst " % arith + "  ".join("%s %.3e" % (k, worst[arith][k]) for k in KEYS))
            say("         gate  " + "  ".join("%s %.2e" % (k, 3 * worst[arith][k]) for k in KEYS))
    say("gates in tests/util.py (F32_FORCED_GATES):")
    for arith in ARITHMETICS:
        say("  %-6s " % arith + "  ".join("%s %.2e" % (k, F32_FORCED_GATES[arith][k]) for k in KEYS))
    say()
    say("single-layer faults at %s, CoordNet (forced: max / rms AT the faulty layer and the layers that miss a forced gate; free-running: the fault's layer and the "
        "worst layer against the fp32 oracle under the older gate)" % "x".join(map(str, MUTATION_SHAPE)))
    smallest = {}       # (form, kind) -> [smallest max, smallest rms]
    for fault, (form, text) in FAULTS.items():
        for kind, layer in FAULT_LAYERS.items():
            rep, free, e_pred = fault_report(fault, layer)
            mx, rms = rep["layers"][layer]
            s = smallest.setdefault((form, kind), [np.inf, np.inf])
            s[0], s[1] = min(s[0], mx), min(s[1], rms)
            say("  %-14s %-8s (%-14s) forced: max %.2e rms %.2e -> fails at %-18s | free-running: %.2e there, worst %.2e, prediction %.1e -> the %.0e gate %s"
                % (fault, layer, kind, mx, rms, ",".join(rep["failed_layers"]) or "NOTHING", free[layer], max(free.values()), e_pred, OLD_GATES[form],
                   "PASSES it" if max(free.values()) < OLD_GATES[form] and e_pred <= 1e-3 else "fails"))
    say()
    say("separation: the smallest fault value per product form and layer kind over the gate (the condition: gate < half the smallest fault, on the max or else the rms metric)")
    for (form, kind), (mx, rms) in smallest.items():
        g = F32_FORCED_GATES[form]
        fm, fr = mx / max(g["layer_max"], 1e-300), rms / max(g["layer_rms"], 1e-300)
        say("  %-4s %-14s smallest fault max %.2e = %.1f x gate, rms %.2e = %.1f x gate -> %s"
            % (form, kind, mx, fm, rms, fr, "met by the max metric" + (" and the rms metric" if fr > 2 else "") if fm > 2 else ("met by the rms metric" if fr > 2 else "NOT MET")))
    say()
    say("why the split kernels keep two accumulators (an explanation, never a gate): one 3 x 3 layer as a GEMM in the six-product form, against fp64 -- the oracle's emulation "
        "(one fp32 GEMM per term) and a one-accumulator chain (all six products of every 16-wide k-step into ONE fp32 accumulator: cnn_x3.hip split_mfma<6>)")
    for cin, cout, npix, kstep, nsplit in ((128, 128, 512, 16, 1), (256, 256, 256, 16, 1), (512, 512, 128, 16, 1), (512, 512, 128, 16, 3), (512, 512, 128, 8, 1)):
        emu, chain = chain_model(cin, cout, npix, kstep, nsplit)
        say("  cin %3d cout %3d K %4d, k-step %2d, %d K-range(s): emulation max %.2e rms %.2e | one-accumulator chain max %.2e rms %.2e"
            % (cin, cout, 9 * cin, kstep, nsplit, emu[0], emu[1], chain[0], chain[1]))
    if args.out:        # (what a device gave is kept below DEVICE_MARK in the same file, by hand: an observation, no input of this tool)
        kept = ""
        if os.path.exists(args.out):
            old = open(args.out).read()
            kept = old[old.index(DEVICE_MARK):] if DEVICE_MARK in old else ""
        with open(args.out, "w") as f:
            f.write("\n".join(lines) + "\n" + kept)


if __name__ == "__main__":
    main()
