#!/usr/bin/env python
"""High-res layer stack: msi_hres_layers (one launch) against the three launches it replaces.  One process; per shape, after a
warm-up and a bit-for-bit comparison of the outputs, the forms ALTERNATE for --repeats rounds and the median is reported:
  (a)   msi_ods_sweep_volume -> msi_resize_bilinear_f32 -> msi_assemble_rgba_scaled_f32   (fp32 stack),
  (a')  the same followed by msi_pack_layers (rgba8 / rgba16f),
  (b)   msi_hres_layers writing the fp32 stack / the rgba8 stack / the rgba16f stack.
Device-event times around each form on preallocated buffers, the algorithmic bytes of each form (images and low-res tensors
read once, every intermediate written and read back, stacks written) and the share of 8 TB/s they amount to; then the peak
allocated memory of each form when it allocates its own buffers, and the end-to-end MSI.msi_render_equirect_hres time against
the same method on the three launches (the body it had before msi_hres_layers existed).
Shapes: 4096x2048x32 from 640x320 (the reference's default high-res size) and 1280x640x32 (configs[3]'s size).
Kernel times: run this under `rocprofv3 --kernel-trace --stats` in a run of its own (--repeats 1 keeps the trace short)."""
import argparse
import os
import sys

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import numpy as np
import torch

ap = argparse.ArgumentParser()
ap.add_argument("--repeats", type=int, default=9, help="alternated rounds; the median is reported")
ap.add_argument("--shapes", default="4096x2048,1280x640", help="comma-separated high-res sizes WxH")
ap.add_argument("--planes", type=int, default=32)
ap.add_argument("--out", default=None, help="also write the table to this text file")
a = ap.parse_args()

from matryodshka_amd import MSI, _native as N

HBM = 8e12
LOW_H, LOW_W = 320, 640
lines = []


def say(s=""):
    print(s, flush=True)
    lines.append(s)


def run_shape(hw, hh, d):
    m = MSI()
    dev, b = m.device, 1
    g = torch.Generator(device="cuda").manual_seed(1)
    ref = torch.rand((b, hh, hw, 3), generator=g, device=dev) * 2 - 1
    src = torch.rand((b, hh, hw, 3), generator=g, device=dev) * 2 - 1
    bw = torch.rand((b, LOW_H, LOW_W, d), generator=g, device=dev)
    al = torch.rand((b, LOW_H, LOW_W, d), generator=g, device=dev)
    low = torch.cat([bw, al], dim=-1).contiguous()
    eye = torch.eye(4, device=dev)[None].contiguous()
    intr = torch.tensor([[[0.032, 0, 0], [0, 1, 0], [0, 0, 1]]], device=dev)
    planes = m.inv_depths(1.0, 100.0, d)
    depths, trig = m._planes(planes), m._trig(hh, hw)
    stream = torch.cuda.current_stream().cuda_stream
    texels = b * d * hh * hw
    new = lambda *shape, dtype=torch.float32: torch.empty(shape, dtype=dtype, device=dev)
    code_dtype = {"rgba8": torch.uint8, "rgba16f": torch.float16}

    def old(psv, up, rgba):
        N.check(N.lib.msi_ods_sweep_volume(ref.data_ptr(), src.data_ptr(), eye.data_ptr(), eye.data_ptr(), intr.data_ptr(),
                                           depths.data_ptr(), trig.data_ptr(), b, hh, hw, d, psv.data_ptr(), 0, stream), "sweep")
        N.check(N.lib.msi_resize_bilinear_f32(low.data_ptr(), up.data_ptr(), b, LOW_H, LOW_W, 2 * d, hh, hw, stream), "resize")
        N.check(N.lib.msi_assemble_rgba_scaled_f32(psv.data_ptr(), up.data_ptr(), rgba.data_ptr(), b, hh, hw, d, stream), "assemble")

    def pack(rgba, fmt, out):
        N.check(N.lib.msi_pack_layers(rgba.data_ptr(), m.LAYER_FORMATS[fmt], out.data_ptr(), texels, stream), "pack")

    def fused(rgba, codes, fmt):
        N.check(N.lib.msi_hres_layers(ref.data_ptr(), src.data_ptr(), eye.data_ptr(), eye.data_ptr(), intr.data_ptr(), depths.data_ptr(),
                                      trig.data_ptr(), bw.data_ptr(), al.data_ptr(), b, LOW_H, LOW_W, hh, hw, d,
                                      0 if rgba is None else rgba.data_ptr(), 0 if codes is None else codes.data_ptr(),
                                      m.LAYER_FORMATS.get(fmt, 0), stream), "hres_layers")

    psv, up, rgba_a, rgba_b = new(b, hh, hw, 6 * d), new(b, hh, hw, 2 * d), new(b, d, hh, hw, 4), new(b, d, hh, hw, 4)
    pk_a = {f: new(b, d, hh, hw, 4, dtype=t) for f, t in code_dtype.items()}
    pk_b = {f: new(b, d, hh, hw, 4, dtype=t) for f, t in code_dtype.items()}
    forms = {"a": lambda: old(psv, up, rgba_a),
             "a8": lambda: (old(psv, up, rgba_a), pack(rgba_a, "rgba8", pk_a["rgba8"])),
             "a16": lambda: (old(psv, up, rgba_a), pack(rgba_a, "rgba16f", pk_a["rgba16f"])),
             "b": lambda: fused(rgba_b, None, None),
             "b8": lambda: fused(None, pk_b["rgba8"], "rgba8"),
             "b16": lambda: fused(None, pk_b["rgba16f"], "rgba16f")}
    names = {"a": "(a)  sweep + resize + assemble", "a8": "(a') ... + pack_layers rgba8", "a16": "(a') ... + pack_layers rgba16f",
             "b": "(b)  hres_layers f32", "b8": "(b)  hres_layers rgba8", "b16": "(b)  hres_layers rgba16f"}
    inputs = 2 * b * hh * hw * 12 + 2 * b * LOW_H * LOW_W * d * 4
    three = inputs + 2 * b * hh * hw * 6 * d * 4 + 2 * b * hh * hw * 2 * d * 4 + texels * 16
    nbytes = {"a": three, "a8": three + texels * 20, "a16": three + texels * 24, "b": inputs + texels * 16, "b8": inputs + texels * 4,
              "b16": inputs + texels * 8}
    t0, t1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)

    def timed(fn):
        t0.record()
        fn()
        t1.record()
        t1.synchronize()
        return t0.elapsed_time(t1) * 1e3          # us

    for fn in forms.values():                     # warm-up, then the outputs bit for bit
        timed(fn)
    torch.cuda.synchronize()
    assert torch.equal(rgba_a.view(torch.int32), rgba_b.view(torch.int32)), "the fp32 stacks differ"
    for f in code_dtype:
        assert torch.equal(pk_a[f].view(torch.uint8), pk_b[f].view(torch.uint8)), "the %s stacks differ" % f
    samples = {k: [] for k in forms}
    for _ in range(a.repeats):
        for k, fn in forms.items():
            samples[k].append(timed(fn))
    med = {k: float(np.median(v)) for k, v in samples.items()}
    say("%dx%dx%d from %dx%d, batch 1  (outputs of (b) == outputs of (a) / (a'), bit for bit: checked)" % (hw, hh, d, LOW_W, LOW_H))
    for k in forms:
        say("  %-34s %9.1f us   %8.1f MB algorithmic = %.2f of 8 TB/s   min %.1f max %.1f  [%s]" % (
            names[k], med[k], nbytes[k] / 1e6, nbytes[k] / HBM * 1e6 / med[k], min(samples[k]), max(samples[k]),
            ", ".join("%.1f" % v for v in samples[k])))
    say("  (a) / (b f32) = %.3f   (a' rgba8) / (b rgba8) = %.3f   (a' rgba16f) / (b rgba16f) = %.3f   (> 1: the fused launch is faster)"
        % (med["a"] / med["b"], med["a8"] / med["b8"], med["a16"] / med["b16"]))

    # peak allocated memory of each form when it allocates what it needs itself
    del psv, up, rgba_a, rgba_b, pk_a, pk_b, forms
    alloc = {"a": lambda: old(new(b, hh, hw, 6 * d), new(b, hh, hw, 2 * d), new(b, d, hh, hw, 4)),
             "b": lambda: fused(new(b, d, hh, hw, 4), None, None),
             "b8": lambda: fused(None, new(b, d, hh, hw, 4, dtype=torch.uint8), "rgba8"),
             "b16": lambda: fused(None, new(b, d, hh, hw, 4, dtype=torch.float16), "rgba16f")}

    def a_packed(fmt):
        r = new(b, d, hh, hw, 4)
        old(new(b, hh, hw, 6 * d), new(b, hh, hw, 2 * d), r)
        pack(r, fmt, new(b, d, hh, hw, 4, dtype=code_dtype[fmt]))
    alloc["a8"], alloc["a16"] = lambda: a_packed("rgba8"), lambda: a_packed("rgba16f")
    peaks = []
    short = {"a": "(a)", "a8": "(a' rgba8)", "a16": "(a' rgba16f)", "b": "(b f32)", "b8": "(b rgba8)", "b16": "(b rgba16f)"}
    for k in ("a", "a8", "a16", "b", "b8", "b16"):
        torch.cuda.synchronize()
        torch.cuda.empty_cache()
        torch.cuda.reset_peak_memory_stats()
        before = torch.cuda.memory_allocated()
        alloc[k]()
        torch.cuda.synchronize()
        peaks.append("%s %.2f GB" % (short[k], (torch.cuda.max_memory_allocated() - before) / 1e9))
    say("  peak allocated beyond the inputs: " + ";  ".join(peaks))

    # end to end: MSI.msi_render_equirect_hres (fused stack) against the same method on the three launches
    pos = np.array([[0.02, -0.01, 0.03]], np.float32)
    eye_np = np.eye(4, dtype=np.float32)[None]
    raw_ref, raw_src = (ref + 1) / 2, (src + 1) / 2

    def e2e_old():
        hres_ref, hres_src = m.preprocess_image(raw_ref), m.preprocess_image(raw_src)
        p = m.format_network_input(hres_ref, hres_src, eye_np, eye_np, planes, intr, dtype='f32')
        lo = torch.cat([bw, al], dim=-1).contiguous()
        u = new(b, hh, hw, 2 * d)
        N.check(N.lib.msi_resize_bilinear_f32(lo.data_ptr(), u.data_ptr(), b, LOW_H, LOW_W, 2 * d, hh, hw, stream), "resize")
        r = new(b, d, hh, hw, 4)
        N.check(N.lib.msi_assemble_rgba_scaled_f32(p.data_ptr(), u.data_ptr(), r.data_ptr(), b, hh, hw, d, stream), "assemble")
        return m.msi_render_equirect_view_and_depth(r.permute(0, 2, 3, 1, 4), eye_np, pos, planes, intr)

    def e2e_new():
        return m.msi_render_equirect_hres(bw, al, raw_ref, raw_src, eye_np, eye_np, eye_np, pos, planes, intr)

    e2e = {"three launches": e2e_old, "hres_layers": e2e_new}
    outs = {k: fn() for k, fn in e2e.items()}
    torch.cuda.synchronize()
    assert all(torch.equal(x.view(torch.int32), y.view(torch.int32)) for x, y in zip(*outs.values())), "the renders differ"
    del outs
    es = {k: [] for k in e2e}
    for _ in range(a.repeats):
        for k, fn in e2e.items():
            es[k].append(timed(fn))
    for k in e2e:
        say("  msi_render_equirect_hres, %-15s %9.1f us   min %.1f max %.1f  [%s]" % (k + ":", float(np.median(es[k])), min(es[k]), max(es[k]),
                                                                                    ", ".join("%.1f" % v for v in es[k])))
    say("  three launches / hres_layers = %.3f" % (float(np.median(es["three launches"])) / float(np.median(es["hres_layers"]))))
    say()


say("high-res layer stack, one launch against three: device-event time per form, median of %d alternated rounds" % a.repeats)
say("device: %s" % torch.cuda.get_device_name(0))
say()
for s in a.shapes.split(","):
    w_, h_ = (int(v) for v in s.split("x"))
    run_shape(w_, h_, a.planes)
    torch.cuda.empty_cache()
if a.out:
    os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
    with open(a.out, "w") as f:
        f.write("\n".join(lines) + "\n")
