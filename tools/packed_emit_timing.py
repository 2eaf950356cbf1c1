#!/usr/bin/env python
"""Fused-tail timing with a packed layer stack as the output: what does emitting rgba8 / rgba16f straight from
head_assemble_packed_kernel cost against the detour through the fp32 stack?  One process; per case, after a warm-up, three forms
ALTERNATE for --repeats rounds and the median is reported:
  (a) msi_net_plan_forward_rgba followed by msi_pack_layers   (the fp32 stack is written, read back and packed),
  (b) msi_net_plan_forward_layers writing the packed stack only,
  (c) msi_net_plan_forward_rgba alone                          (what the fp32 store costs; no packed stack exists).
Only the TAIL is timed: device events from `event_after_convs` (recorded by the forward between the last convolution and the
fused tail) to the end of the form -- the convolutions in front are the same launches in all three.
Cases: BASELINE configs[1] (fp32, 1 x 320 x 640 x 32) and configs[2] (bf16 + CoordNet, 16 x 320 x 640 x 64), both formats.
Per case: the times, (a) / (b), the algorithmic bytes of each form (activations + sweep volume read, stacks written and read
back) and the share of 8 TB/s they amount to.  Before anything is reported the bytes of (b) are asserted equal to the bytes of (a).
Kernel times: run this under `rocprofv3 --kernel-trace --stats` in a run of its own (--repeats 1 keeps the trace short)."""
import argparse
import os
import sys

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import numpy as np
import torch

ap = argparse.ArgumentParser()
ap.add_argument("--repeats", type=int, default=9, help="alternated rounds; the median is reported")
ap.add_argument("--configs", default="1,2", help="comma-separated BASELINE configs to time (1: fp32 batch 1 D 32; 2: bf16 batch 16 D 64)")
ap.add_argument("--out", default=None, help="also write the table to this text file")
a = ap.parse_args()

from matryodshka_amd import MSI, nets, _native as N
from matryodshka_amd.packed import BYTES_PER_TEXEL

HBM = 8e12
NGF = 64
CASES = {1: dict(name="configs[1] fp32 1x320x640x32", dtype="f32", b=1, h=320, w=640, d=32, coord=True),
         2: dict(name="configs[2] bf16 16x320x640x64", dtype="bf16", b=16, h=320, w=640, d=64, coord=True)}
lines = []


def say(s=""):
    print(s, flush=True)
    lines.append(s)


def run_case(c):
    b, h, w, d = c["b"], c["h"], c["w"], c["d"]
    bf16 = c["dtype"] == "bf16"
    weights = nets.init_weights(6 * d, 2 * d, NGF, c["coord"], seed=8964)
    m = MSI(weights=weights, coord_net=c["coord"], dtype=c["dtype"])
    g = torch.Generator(device="cuda").manual_seed(1)
    x = (torch.rand((b, h, w, 6 * d), generator=g, device="cuda") * 2 - 1).to(torch.bfloat16 if bf16 else torch.float32)
    desc, blob, ws = m._net(b, h, w, 6 * d, 2 * d, NGF)
    plan = m._plan(b, h, w, 6 * d, 2 * d, NGF)
    texels = b * d * h * w
    rgba = torch.empty((b, d, h, w, 4), device="cuda")
    stream = torch.cuda.current_stream().cuda_stream
    mid, end = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    mid.record(); end.record()                       # (recorded once: the handles exist)
    torch.cuda.synchronize()

    def forward_rgba():
        N.check(N.lib.msi_net_plan_forward_rgba(plan.handle, blob.data_ptr(), x.data_ptr(), rgba.data_ptr(), 0, 0, 0, ws.data_ptr(),
                                                ws.numel(), stream, mid.cuda_event), "forward_rgba")

    # bytes per pixel the tail reads: conv8_2's raw output (fp32; fp16 in a bf16 plan) + the sweep volume (fp32 / bf16)
    read_px = NGF * (2 if bf16 else 4) + 6 * d * (2 if bf16 else 4)
    npix = b * h * w
    for fmt in ("rgba8", "rgba16f"):
        tb = BYTES_PER_TEXEL[fmt]
        code = m.LAYER_FORMATS[fmt]
        pk_a = torch.empty((b, d, h, w, 4), dtype=torch.uint8 if fmt == "rgba8" else torch.float16, device="cuda")
        pk_b = torch.empty_like(pk_a)

        def form_a():
            forward_rgba()
            N.check(N.lib.msi_pack_layers(rgba.data_ptr(), code, pk_a.data_ptr(), texels, stream), "pack_layers")

        def form_b():
            N.check(N.lib.msi_net_plan_forward_layers(plan.handle, blob.data_ptr(), x.data_ptr(), 0, pk_b.data_ptr(), code, 0, 0, 0,
                                                      ws.data_ptr(), ws.numel(), stream, mid.cuda_event), "forward_layers")

        forms = {"a": form_a, "b": form_b, "c": forward_rgba}
        nbytes = {"a": npix * read_px + texels * (16 + 16 + tb), "b": npix * read_px + texels * tb, "c": npix * read_px + texels * 16}

        def timed(fn):
            fn()
            end.record()
            end.synchronize()
            return mid.elapsed_time(end) * 1e3       # us, event_after_convs -> end

        for fn in forms.values():                    # warm-up (and the check below)
            timed(fn)
        pk_a.zero_(); pk_b.zero_()
        form_a(); form_b()
        torch.cuda.synchronize()
        assert torch.equal(pk_a.view(torch.uint8), pk_b.view(torch.uint8)), "%s %s: the emitted stack differs from pack_layers" % (c["name"], fmt)
        try:
            m.network_status()
        except N.MsiError as e:                      # (reported, not fatal: the timing does not depend on it)
            say("  network_status: %s" % e)
        samples = {k: [] for k in forms}
        for _ in range(a.repeats):
            for k, fn in forms.items():
                samples[k].append(timed(fn))
        med = {k: float(np.median(v)) for k, v in samples.items()}
        say("%s  %s  (bytes of (b) == bytes of (a): checked)" % (c["name"], fmt))
        for k, what in (("a", "forward_rgba + pack_layers"), ("b", "forward_layers, packed only"), ("c", "forward_rgba alone")):
            share = nbytes[k] / HBM * 1e6 / med[k]
            say("  (%s) %-28s %9.1f us   %8.1f MB algorithmic = %.2f of 8 TB/s   min %.1f max %.1f  [%s]" % (
                k, what, med[k], nbytes[k] / 1e6, share, min(samples[k]), max(samples[k]), ", ".join("%.1f" % v for v in samples[k])))
        say("  (a) / (b) = %.3f   (c) / (b) = %.3f   (> 1: emitting the packed stack is faster)" % (med["a"] / med["b"], med["c"] / med["b"]))
        say()
    del m, x, rgba


say("fused tail with a packed stack as output: tail time from event_after_convs to the end of the form, median of %d alternated rounds" % a.repeats)
say("device: %s" % torch.cuda.get_device_name(0))
say()
for k in a.configs.split(","):
    run_case(CASES[int(k)])
    torch.cuda.empty_cache()
if a.out:
    os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
    with open(a.out, "w") as f:
        f.write("\n".join(lines) + "\n")
