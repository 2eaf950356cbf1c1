"""Shared synthetic inputs for the parity tests: band-limited noise
ODS pairs, identity poses, baseline 0.032, target position inside the unit sphere."""
import numpy as np


from matryodshka_amd.synthetic import smooth_noise, make_inputs, random_rgba, pp_inputs  # noqa: F401,E402


# ---- include/msi_hip.h as the ABI tests read it
def header_text(comments=False):
    import os
    import re
    text = open(os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "include", "msi_hip.h")).read()
    return text if comments else re.sub(r"/\*.*?\*/", "", text, flags=re.S)


def declared(name):
    """(restype, [(ctype, parameter name)]) of function `name` as include/msi_hip.h declares it.  Scalars are the ctypes of
    matryodshka_amd/_native.py and msi_stream_t is c_void_p; a pointer is POINTER(what it points to) -- the binding's Structure
    for msi_net_desc / msi_layer_info -- and c_void_p for `void *` and the opaque msi_net_plan; a `const char *` return is
    c_char_p, a `void` return None.  A binding may spell any pointer c_void_p: untyped() of the ctype."""
    import ctypes as C
    import re
    from matryodshka_amd import _native as N
    m = re.search(r"(?:^|[;}\n])\s*((?:const\s+)?\w+[\s*]+)%s\s*\((.*?)\)\s*;" % name, header_text(), flags=re.S)
    assert m, "%s is not declared in include/msi_hip.h" % name
    scalars = {"int": C.c_int32, "int32_t": C.c_int32, "uint32_t": C.c_uint32, "int64_t": C.c_int64, "uint64_t": C.c_uint64, "uint8_t": C.c_uint8,
               "size_t": C.c_size_t, "float": C.c_float, "double": C.c_double, "char": C.c_char, "msi_stream_t": C.c_void_p,
               "msi_net_desc": N.NetDesc, "msi_layer_info": N.LayerInfo}

    def ctype(words, ret=False):
        words = [w for w in words if w != "const"]
        base, stars = words[0], words.count("*")
        assert len(words) == 1 + stars, words
        if ret and (base, stars) == ("char", 1):
            return C.c_char_p
        if base in ("void", "msi_net_plan"):            # (`void` itself: a return type only; nothing takes a msi_net_plan by value)
            assert stars or (ret and base == "void"), words
            kind, stars = (C.c_void_p if stars else None), stars - 1
        else:
            assert base in scalars, words
            kind = scalars[base]
        for _ in range(max(stars, 0)):
            kind = C.POINTER(kind)
        return kind

    params = [p.replace("*", " * ").split() for p in m.group(2).split(",")]
    params = [] if params in ([["void"]], [[]]) else params
    return ctype(m.group(1).replace("*", " * ").split(), ret=True), [(ctype(p[:-1]), p[-1]) for p in params]


def check_binding(native_lib, name, int32_and_pointers=False):
    """Asserts that _native.SIGNATURES[name] is the header's declaration of `name` -- the return type, and every parameter as its
    ctype or, a pointer, as c_void_p; with int32_and_pointers, that it returns int32 and takes nothing but int32_t and pointers
    bound as c_void_p -- and returns the declared parameter names."""
    import ctypes
    ret, params = declared(name)
    res, args = native_lib.SIGNATURES[name]
    assert res is ret, (name, res, ret)
    assert len(args) == len(params), (name, len(args), len(params))
    for k, (arg, (kind, pname)) in enumerate(zip(args, params)):
        assert arg in (kind, untyped(kind)), (name, k, pname, arg, kind)
    if int32_and_pointers:
        assert res is ctypes.c_int32 and set(args) <= {ctypes.c_void_p, ctypes.c_int32}, name
    return [pname for _, pname in params]


def untyped(kind):
    """c_void_p for a ctypes pointer type, `kind` itself otherwise: how most of _native.SIGNATURES spells a pointer."""
    import ctypes
    return ctypes.c_void_p if isinstance(kind, type) and issubclass(kind, ctypes._Pointer) else kind


# ---- stratified dense sample set of the full-size fixtures (tests/golden/make_golden.py writes the values, the -m gpu
# tests regenerate the SAME indices from (shape, extra pixels, seed): only values and the oracle-derived pixels are stored)
def stratified_rows(h):
    """Eight full rows: both polar pairs, the equator pair, and one odd / one even row in between."""
    return sorted({0, 1, h // 2 - 1, h // 2, h - 2, h - 1, (h // 3) | 1, (2 * h // 3) & ~1})


def stratified_pixels(h, w, extra=None):
    """Sorted flat pixel indices y * w + x: eight full rows (polar rows included), the columns on both sides of every
    64-pixel tile seam (x % 64 in {0, 63}), and `extra` (the pixels the oracle marks disc < 0 on the far / near plane)."""
    mask = np.zeros((h, w), dtype=bool)
    mask[stratified_rows(h), :] = True
    mask[:, 0::64] = True
    mask[:, 63::64] = True
    pix = np.flatnonzero(mask.reshape(-1))
    if extra is not None and len(extra):
        pix = np.union1d(pix, np.asarray(extra, dtype=np.int64))
    return pix.astype(np.int64)


def stratified_index(shape, extra=None, seed=0, cap=262144):
    """Flat indices into a C-ordered array of `shape` = (B, H, W, *rest): every batch element, the stratified_pixels,
    and per pixel either all `rest` elements or -- when that exceeds `cap` values in total -- k seeded random ones
    (k = cap // pixels, at least 1).  At least `cap` values whenever the tensor has that many at the pixel set."""
    b, h, w = int(shape[0]), int(shape[1]), int(shape[2])
    rest = int(np.prod(shape[3:])) if len(shape) > 3 else 1
    pix = stratified_pixels(h, w, extra)
    base = (np.arange(b, dtype=np.int64)[:, None] * (h * w) + pix[None, :]).reshape(-1) * rest     # [B * P]
    if base.size * rest <= cap:
        ch = np.arange(rest, dtype=np.int64)[None, :]
        return (base[:, None] + ch).reshape(-1)
    k = max(1, -(-cap // base.size))
    rng = np.random.RandomState(seed)
    ch = rng.randint(0, rest, size=(base.size, k)).astype(np.int64)
    return (base[:, None] + ch).reshape(-1)


def count_equal_11(psv, pre_images, d, round_fn=None):
    """[2, B, D]: texels of the sweep volume whose three channels equal the source image's (1, 1) pixel -- what a
    pixel with a negative discriminant gathers (spherical.py:226-229: u = v = 1).  round_fn: the rounding the volume
    went through (bf16 volumes)."""
    b = psv.shape[0]
    out = np.zeros((2, b, d), dtype=np.int64)
    for s in range(2):
        for k in range(b):
            ref = pre_images[s][k, 1, 1, :].astype(np.float32)
            if round_fn is not None:
                ref = np.asarray(round_fn(ref), dtype=np.float32)
            for j in range(d):
                ch = s * 3 * d + 3 * j
                out[s, k, j] = int(np.all(psv[k, :, :, ch:ch + 3].astype(np.float32) == ref[None, None, :], axis=-1).sum())
    return out


def read_raw_output(ws, packed, info, batch, dtype):
    """A layer's raw (pre-LayerNorm) convolution output [B,H,W,C] as float32 numpy from a plan's workspace (torch uint8
    tensor): fp32 plans store fp32; bf16 plans store fp16 of x * 2^-e, with 2^e = 2^24 / S1 from the layer's LayerNorm
    window in the packed blob (include/msi_hip.h: msi_layer_info.ln_scale_offset)."""
    import torch
    n = batch * info.out_h * info.out_w * info.cout
    shape = (batch, info.out_h, info.out_w, info.cout)
    if dtype == "f32":
        return ws[info.raw_offset:info.raw_offset + 4 * n].view(torch.float32).reshape(shape).cpu().numpy()
    scl = packed[info.ln_scale_offset:info.ln_scale_offset + 8].cpu().numpy().view(np.float64)
    up = np.float32(16777216.0 / scl[0])
    return ws[info.raw_offset:info.raw_offset + 2 * n].view(torch.float16).reshape(shape).float().cpu().numpy() * up


def poison_workspace(m, b, h, w, cin, nout, ngf):
    """Fill the network workspace of model `m` (matryodshka_amd.MSI, with its current net_options) for this shape with
    0xFF bytes -- NaN as fp32, fp16 and bf16 -- and return it.  Call it BEFORE the first forward of a plan.

    MSI._net allocates the workspace with torch.empty, and the caching allocator likes to hand a new plan the block a
    dropped model has just released: a same-input A/B test (tile8 vs 4-row, halo vs tap, fix-up vs in-launch) can then
    read the OTHER variant's correct raw outputs where its own variant computed no tile or lost a store.  On a poisoned
    workspace such an element stays NaN, and so does everything downstream of it.

    The whole workspace is poisoned: nothing in it is written once and kept.  Its regions are (cnn_net.hip: build_net) the
    layers' raw outputs / published affines / bf16 activation copies, the K-range slabs, and the zero region (arrival
    tickets, LayerNorm sums, status word) -- the first three are written by the forward that reads
    them, the last is cleared by every forward's first launch.  What IS written once outside the forward (packed weights,
    LayerNorm windows, msi_net_plan_calibrate's result) lives in the packed blob, which this does not touch."""
    _, _, ws = m._net(b, h, w, cin, nout, ngf)
    ws.fill_(0xFF)
    return ws


# ---- the teacher-forced layer check of the bf16 tier
# Gates of forced_layer_errors, MEASURED ON THE CPU (tools/bf16_forced_gates.py, profiles/bf16_forced_gates.txt): 3 x the worst value of a
# stand-in with exactly a correct kernel's freedoms, over the shapes of the tests that use them, two seeds each.  Never set from a device run.
# Keyed by the network width ngf: a flipped bf16 operand weighs ~ 1 / sqrt(K) of a layer's scale and K follows ngf, and the narrow shapes' small layers
# see the largest difference between statistics of stored and of unrounded values -- within one width all 17 layers share one gate, each width's gate is
# 3 x the worst of ITS runs (so none is above 3 x the worst of all runs).  layer_bias: see forced_layer_errors; head_*: absolute, and include 2e-7 for msi_tanh.
BF16_FORCED_GATES = {
    16: dict(layer_max=4.39e-3, layer_mean=3.47e-4, layer_bias=1.98e-5, head_max=1.77e-2, head_mean=2.99e-5),   # worst 1.46e-3 1.16e-4 6.59e-6 | 5.89e-3 9.97e-6
    32: dict(layer_max=2.04e-3, layer_mean=2.14e-4, layer_bias=1.20e-5, head_max=1.00e-2, head_mean=1.23e-5),   # worst 6.79e-4 7.12e-5 4.01e-6 | 3.34e-3 4.11e-6
    64: dict(layer_max=1.79e-3, layer_mean=1.31e-4, layer_bias=2.48e-6, head_max=1.19e-2, head_mean=9.32e-6),   # worst 5.96e-4 4.37e-5 8.27e-7 | 3.95e-3 3.11e-6
}


def forced_gates(ngf):
    """BF16_FORCED_GATES of a network of width ngf: a measured width, or -- ngf >= 64 -- the widest measured class (the runs at ngf = 144 stay below every
    worst value of ngf = 64: beyond it the fp16 store is what is left)."""
    return BF16_FORCED_GATES[64 if ngf >= 64 else ngf]


def forced_layer_errors(weights, x, coord, raws, pred, gates=None, kernels=None):
    """One run of the teacher-forced bf16 oracle (oracle/nets.py forward(bf16=True, forced_raw=raws)): every layer recomputed from the
    raw outputs `raws` ({layer: [B,H,W,C] fp32}: tests.util.read_raw_output of a bf16 plan, or a stand-in's) of its OWN sources, so a
    layer's error is that layer's alone -- summation order, the fp16 store, isolated operand flips -- at conv8_2 as at conv1_1.

    Returns a dict:
      "layers": {layer: (max, mean)} of |raws[layer] - forced oracle| / max |forced oracle's raw output|;
      "bias":   {layer: mean of sign(oracle) (raws[layer] - oracle) / scale}: how far the stored values lean towards zero (-) or away
                (+); round-to-nearest stores do not lean (|bias| ~ mean / sqrt(elements)), a truncating store leans by its whole mean error;
      "head":   (max, mean) of |pred - forced prediction|, absolute (tanh output in [-1, 1]);
    and, with `gates` (BF16_FORCED_GATES),
      "over":   {layer: elements above the max gate}, "first": {layer: (b, y, x, c) of the first of them};
      "failed_layers": layers (and "color_pred") that miss a gate, "failures": one line each, with the layer's kernel where
                `kernels` (plan.kernels()) is given."""
    from oracle import nets as onets
    names = [t[0] for t in onets.layer_table(1, 1) if t[1] != "h"]
    assert sorted(raws) == sorted(names), sorted(raws)
    ref, acts = onets.forward(weights, x, coord_net=coord, return_activations=True, bf16=True, forced_raw=raws)
    rep = dict(layers={}, bias={}, over={}, first={}, failed_layers=[], failures=[])
    for li, name in enumerate(names):
        o = acts[name + "/raw"]
        assert raws[name].shape == o.shape, (name, raws[name].shape, o.shape)
        scale = float(np.abs(o).max()) + 1e-30
        d = (raws[name].astype(np.float64) - o) / scale
        e = np.abs(d)
        rep["layers"][name] = (float(e.max()), float(e.mean()))
        rep["bias"][name] = float((np.sign(o) * d).mean())
        if gates is None:
            continue
        over = e > gates["layer_max"]
        rep["over"][name] = int(over.sum())
        if rep["over"][name]:
            rep["first"][name] = tuple(int(i) for i in np.argwhere(over)[0])
        if rep["over"][name] or e.mean() > gates["layer_mean"] or abs(rep["bias"][name]) > gates["layer_bias"]:
            rep["failed_layers"].append(name)
            rep["failures"].append("%s%s: max %.2e (gate %.1e; %d of %d elements over it%s), mean %.2e (gate %.1e), bias %+.2e (gate %.1e)" % (
                name, " [%s]" % kernels[li][0] if kernels else "", e.max(), gates["layer_max"], rep["over"][name], e.size,
                ", first at (b, y, x, c) = %r" % (rep["first"][name],) if rep["over"][name] else "", e.mean(), gates["layer_mean"],
                rep["bias"][name], gates["layer_bias"]))
    eh = np.abs(np.asarray(pred, dtype=np.float64) - ref)
    rep["head"] = (float(eh.max()), float(eh.mean()))
    if gates is not None and (eh.max() > gates["head_max"] or eh.mean() > gates["head_mean"]):
        over = eh > gates["head_max"]
        rep["failed_layers"].append("color_pred")
        rep["failures"].append("color_pred%s: max %.2e (gate %.1e; %d elements over it%s), mean %.2e (gate %.1e)" % (
            " [%s]" % kernels[17][0] if kernels else "", eh.max(), gates["head_max"], int(over.sum()),
            ", first at (b, y, x, c) = %r" % (tuple(int(i) for i in np.argwhere(over)[0]),) if over.any() else "", eh.mean(), gates["head_mean"]))
    return rep


# ---- the teacher-forced layer check of the fp32 tier, against an fp64 reference
# Gates of forced_layer_errors_f32 per ARITHMETIC of a layer's kernel, MEASURED ON THE CPU (tools/f32_forced_gates.py, profiles/f32_forced_gates.txt): 3 x the worst
# value, over all 17 layers, shapes A / B / C / E of tests/test_plan_decomposition.py at ngf 32 and 64 and five seeds each, of the oracle's own emulation of that
# arithmetic (forward(split3_products=True | "f16" | False, forced_raw=R)) against forward(precision="fp64", forced_raw=R).  Never set from a device run.
# layer_*: relative to the fp64 tensor's max-abs (max) and rms (rms); head_*: the same of the tanh output (the head always runs the native tap kernel: its gates are "native"'s).
F32_FORCED_GATES = {
    "x3": dict(layer_max=1.40e-6, layer_rms=5.23e-7, head_max=9.36e-7, head_rms=2.04e-7),         # worst 4.665e-7 1.743e-7 | 3.121e-7 6.797e-8
    "f16": dict(layer_max=3.12e-6, layer_rms=1.25e-6, head_max=1.98e-6, head_rms=3.63e-7),        # worst 1.039e-6 4.168e-7 | 6.600e-7 1.210e-7
    "native": dict(layer_max=3.41e-6, layer_rms=1.26e-6, head_max=1.83e-6, head_rms=3.03e-7),     # worst 1.138e-6 4.202e-7 | 6.113e-7 1.009e-7
}


def f32_arithmetic(kernel):
    """The arithmetic of an fp32 plan's kernel, read off its msi_net_plan_layer_kernel name: "x3" (six bf16 products), "f16" (three fp16 products: the split
    kernels whose last template argument, the plane count, is 2) or "native" (fp32 MFMA: conv_halo*_kernel, conv_igemm_kernel)."""
    if "_x3_kernel" not in kernel:
        return "native"
    return "f16" if "_x3_kernel<" in kernel and kernel.endswith("2>") else "x3"


def rel_max_rms(got, ref):
    """(max |got - ref| / max |ref|, rms (got - ref) / rms ref), in fp64."""
    ref = np.asarray(ref, dtype=np.float64)
    d = np.asarray(got, dtype=np.float64) - ref
    return (float(np.abs(d).max() / (np.abs(ref).max() + 1e-300)), float(np.sqrt((d * d).mean()) / (np.sqrt((ref * ref).mean()) + 1e-300)))


def forced_layer_errors_f32(weights, x, coord, stored, normalized, pred, gates=None, kernels=None):
    """One run of the teacher-forced fp64 oracle (oracle/nets.py forward(precision="fp64", forced_raw=..., forced_act=...)) on what an fp32 plan left in its
    workspace: `stored` = {layer: [B,H,W,C] fp32} for all 17 layers, `normalized` = the layers whose buffer holds the ACTIVATION (the plan applied LayerNorm + ReLU
    in place: msi_net_plan_layer_is_normalized != 0), every other buffer the raw output.  Every layer is recomputed in fp64 from the stored tensors of its OWN
    sources, so a layer's error is that layer's alone: its product form, its summation order, its operands' planes.  A normalized layer forces its consumers
    with the stored activation and is compared as an activation (the oracle's own LayerNorm + ReLU, in fp64, of its own fp64 raw output); it is never left out.

    Returns a dict:
      "layers":   {layer: (max, rms)} of stored - fp64, the max relative to the fp64 tensor's max-abs, the rms to its rms;
      "compared": {layer: "raw" | "activation"};
      "head":     (max, rms) of pred - the forced fp64 prediction, relative in the same way;
    and, with `gates` (F32_FORCED_GATES) and `kernels` (plan.kernels(): 18 entries whose first item is the kernel name; each layer is held to the gates of
    f32_arithmetic(its kernel)),
      "over":     {layer: elements above the max gate}, "first": {layer: (b, y, x, c) of the first of them};
      "failed_layers": layers (and "color_pred") that miss a gate, "failures": one line each, with the layer's kernel."""
    from oracle import nets as onets
    names = [t[0] for t in onets.layer_table(1, 1) if t[1] != "h"]
    assert sorted(stored) == sorted(names), sorted(stored)
    normalized = set(normalized)
    assert normalized <= set(names), sorted(normalized)
    assert gates is None or (kernels is not None and len(kernels) == 18), "gates are per kernel arithmetic: pass the plan's kernels"
    ref, acts = onets.forward(weights, x, coord_net=coord, return_activations=True, precision="fp64",
                              forced_raw={n: stored[n] for n in names if n not in normalized},
                              forced_act={n: stored[n] for n in names if n in normalized})
    rep = dict(layers={}, compared={}, over={}, first={}, failed_layers=[], failures=[])
    for li, name in enumerate(names):
        what = "activation" if name in normalized else "raw"
        o = acts[name] if name in normalized else acts[name + "/raw"]
        assert stored[name].shape == o.shape, (name, stored[name].shape, o.shape)
        rep["compared"][name] = what
        rep["layers"][name] = mx, rms = rel_max_rms(stored[name], o)
        if gates is None:
            continue
        g = gates[f32_arithmetic(kernels[li][0])]
        over = np.abs(stored[name].astype(np.float64) - o) > g["layer_max"] * np.abs(o).max()
        rep["over"][name] = int(over.sum())
        if rep["over"][name]:
            rep["first"][name] = tuple(int(i) for i in np.argwhere(over)[0])
        if not (mx <= g["layer_max"] and rms <= g["layer_rms"]):         # (a NaN fails)
            rep["failed_layers"].append(name)
            rep["failures"].append("%s [%s, %s, %s]: max %.2e (gate %.2e; %d of %d elements over it%s), rms %.2e (gate %.2e)" % (
                name, kernels[li][0], f32_arithmetic(kernels[li][0]), what, mx, g["layer_max"], rep["over"][name], over.size,
                ", first at (b, y, x, c) = %r" % (rep["first"][name],) if rep["over"][name] else "", rms, g["layer_rms"]))
    rep["head"] = hmx, hrms = rel_max_rms(pred, ref)
    if gates is not None:
        g = gates[f32_arithmetic(kernels[17][0])]
        if not (hmx <= g["head_max"] and hrms <= g["head_rms"]):
            rep["failed_layers"].append("color_pred")
            rep["failures"].append("color_pred [%s, %s]: max %.2e (gate %.2e), rms %.2e (gate %.2e)" % (
                kernels[17][0], f32_arithmetic(kernels[17][0]), hmx, g["head_max"], hrms, g["head_rms"]))
    return rep
