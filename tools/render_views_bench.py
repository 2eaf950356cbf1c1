#!/usr/bin/env python
"""MSI.render_views timing: many views of one 640x320x32 MSI per launch.  Device events around --iters calls, one warm-up
pass, the median of --repeats repeats in which the compared forms ALTERNATE (one process).  Cases:
  (a) V = 8 equirect 640x320 views of one stack in ONE render_views call  vs  8 back-to-back msi_render_equirect_view_and_depth
      calls on the same stack (both with device-side poses: no host domain check, no sync);
  (b) V = 2 and V = 8 pinhole views at 1024x1024, fx = fy = 512 (90 degrees);
  (c) B = 4 stacks x V = 8 equirect views in one call (the grid runs sample -> view -> row);
  (d) one 2048x1024x32 stack (fp32 1.07 GB, rgba8 268 MB), V = 2 pinhole views at 1024x1024;
  (e) MSI.pack_layers / unpack_layers of one 640x320x32 stack against their byte floors (bytes read + written).
In (a)-(d) the fp32 stack and its rgba8 / rgba16f PackedLayers are alternated forms of the same call; each packed form is
reported with its ratio to fp32 from the same process (> 1: the packed form is slower).
Per case: us per call, views/s, and the byte floor -- each stack read once + the output bytes -- over 8 TB/s as a share of
the measured time (a floor, not a roofline: the render is VALU / gather-issue bound).  Kernel times: run this under
`rocprofv3 --kernel-trace --stats` in a run of its own (--repeats 1 keeps the trace short)."""
import argparse
import json
import os
import sys

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import numpy as np
import torch

ap = argparse.ArgumentParser()
ap.add_argument("--iters", type=int, default=20, help="calls per timed window")
ap.add_argument("--repeats", type=int, default=5, help="alternated repeats; the median is reported")
ap.add_argument("--out", default=None, help="write the results as JSON here")
a = ap.parse_args()

from matryodshka_amd import MSI

HBM = 8e12
H, W, D = 320, 640, 32
m = MSI()
planes = m.inv_depths(1.0, 100.0, D)
g = torch.Generator(device="cpu").manual_seed(0)


def stacks(b):
    native = torch.rand((b, D, H, W, 4), generator=g).cuda()
    return native.permute(0, 2, 3, 1, 4)             # the [B,H,W,D,4] view of the native stack (no copy on the way in)


def poses(b, v):
    rng = np.random.RandomState(b * 100 + v)
    pose = np.tile(np.eye(4, dtype=np.float32), (b, v, 1, 1))
    for i in range(b):
        for k in range(v):
            ang = rng.uniform(-np.pi, np.pi)
            c, s = np.cos(ang), np.sin(ang)
            pose[i, k, 0, 0], pose[i, k, 0, 2], pose[i, k, 2, 0], pose[i, k, 2, 2] = c, s, -s, c
            pose[i, k, :3, 3] = rng.uniform(-0.05, 0.05, 3)
    pos = rng.uniform(-0.05, 0.05, (b, v, 3)).astype(np.float32)
    return torch.from_numpy(pose).cuda(), torch.from_numpy(pos).cuda()


def timed(fn):
    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    e0.record()
    for _ in range(a.iters):
        fn()
    e1.record()
    e1.synchronize()
    return e0.elapsed_time(e1) * 1e3 / a.iters       # us per call


def measure(forms):
    """forms: name -> callable.  Warm-up, then `repeats` rounds alternating the forms; median us per call of each."""
    for fn in forms.values():
        fn()
    torch.cuda.synchronize()
    samples = {k: [] for k in forms}
    for _ in range(a.repeats):
        for k, fn in forms.items():
            samples[k].append(timed(fn))
    return {k: float(np.median(v)) for k, v in samples.items()}, samples


stack_bytes = H * W * D * 16
results = []
TEXEL_BYTES = {"f32": 16, "rgba8": 4, "rgba16f": 8}


def report(case, us, b, v, oh, ow, samples, texels=H * W * D, fmt="f32", f32_us=None):
    out_bytes = b * v * oh * ow * 16                 # rgb (12 B) + depth (4 B) per pixel
    floor_us = (b * texels * TEXEL_BYTES[fmt] + out_bytes) / HBM * 1e6
    r = dict(case=case, us_per_call=round(us, 2), views_per_s=round(b * v / us * 1e6, 1), batch=b, views=v, size=[oh, ow],
             byte_floor_us=round(floor_us, 2), byte_floor_share_of_8TBps=round(floor_us / us, 3),
             samples_us=[round(x, 2) for x in samples])
    if fmt != "f32":
        r.update(format=fmt, ratio_to_f32=round(us / f32_us, 3))
    results.append(r)
    print("%-34s %9.1f us/call  %9.0f views/s   byte floor %.1f us = %.2f of the measured time at 8 TB/s  (repeats %s)" % (
        case, us, r["views_per_s"], floor_us, floor_us / us, ", ".join("%.1f" % x for x in samples)), flush=True)
    return r


def with_packed(case, layers_f32, call, b, v, oh, ow, texels=H * W * D, extra=None):
    """`call(stack)` with the fp32 stack and its two packed forms, alternated; one report line per form."""
    stacks_ = {"f32": layers_f32, "rgba8": m.pack_layers(layers_f32, "rgba8"), "rgba16f": m.pack_layers(layers_f32, "rgba16f")}
    forms = {k: (lambda s=s: call(s)) for k, s in stacks_.items()}
    forms.update(extra or {})
    med, smp = measure(forms)
    for k in stacks_:
        name = case if k == "f32" else "%s [%s]" % (case, k)
        report(name, med[k], b, v, oh, ow, smp[k], texels, k, med["f32"])
        if k != "f32":
            print("    %s / fp32 = %.3f  (fp32 repeats %s)" % (k, med[k] / med["f32"], ", ".join("%.1f" % x for x in smp["f32"])), flush=True)
    return med, smp


# (a) one call of 8 views vs 8 single-view calls on one stack
layers = stacks(1)
pose8, pos8 = poses(1, 8)
singles = [(pose8[0, k:k + 1].contiguous(), pos8[0, k:k + 1].contiguous()) for k in range(8)]


def eight_singles():
    for p, q in singles:
        m.msi_render_equirect_view_and_depth(layers, p, q, planes, None)


med, smp = with_packed("(a) equirect V=8, one call", layers, lambda s: m.render_views(s, pose8, pos8, planes), 1, 8, H, W,
                       extra={"singles": eight_singles})
rb = report("(a) equirect 8 x single-view calls", med["singles"], 1, 8, H, W, smp["singles"])
ratio = med["singles"] / med["f32"]
print("(a) 8 single calls / one 8-view call = %.3f (> 1: the one call is faster)" % ratio, flush=True)

# (b) pinhole eyes at 1024^2, 90 degrees
K = torch.tensor([[512.0, 0, 512.0], [0, 512.0, 512.0], [0, 0, 1]]).cuda()
pose2, pos2 = poses(1, 2)
med, smp = measure({"v2": lambda: m.render_views(layers, pose2, pos2, planes, camera="pinhole", intrinsics=K, size=(1024, 1024))})
report("(b) pinhole V=2 1024x1024", med["v2"], 1, 2, 1024, 1024, smp["v2"])
with_packed("(b) pinhole V=8 1024x1024", layers,
            lambda s: m.render_views(s, pose8, pos8, planes, camera="pinhole", intrinsics=K, size=(1024, 1024)), 1, 8, 1024, 1024)

# (c) four stacks x 8 views in one call
layers4 = stacks(4)
pose48, pos48 = poses(4, 8)
with_packed("(c) equirect B=4 x V=8, one call", layers4, lambda s: m.render_views(s, pose48, pos48, planes), 4, 8, H, W)
del layers4

# (d) one high-resolution stack, two pinhole eyes
HH, WH = 1024, 2048
gd = torch.Generator(device="cuda").manual_seed(1)
layers_hi = torch.rand((1, D, HH, WH, 4), generator=gd, device="cuda").permute(0, 2, 3, 1, 4)
with_packed("(d) pinhole V=2 1024x1024 from 2048x1024x32", layers_hi,
            lambda s: m.render_views(s, pose2, pos2, planes, camera="pinhole", intrinsics=K, size=(1024, 1024)), 1, 2, 1024, 1024,
            texels=HH * WH * D)
del layers_hi

# (e) pack / unpack of one 640x320x32 stack; floor = (bytes read + bytes written) / 8 TB/s
packed_ = {f: m.pack_layers(layers, f) for f in ("rgba8", "rgba16f")}
forms = {}
for f in packed_:
    forms["pack " + f] = lambda f=f: m.pack_layers(layers, f)
    forms["unpack " + f] = lambda f=f: m.unpack_layers(packed_[f])
med, smp = measure(forms)
for k in forms:
    floor_us = H * W * D * (16 + TEXEL_BYTES[k.split()[1]]) / HBM * 1e6
    results.append(dict(case="(e) " + k, us_per_call=round(med[k], 2), byte_floor_us=round(floor_us, 2),
                        byte_floor_share_of_8TBps=round(floor_us / med[k], 3), samples_us=[round(x, 2) for x in smp[k]]))
    print("%-34s %9.1f us/call  byte floor %.1f us = %.2f of the measured time at 8 TB/s  (repeats %s)" % (
        "(e) " + k, med[k], floor_us, floor_us / med[k], ", ".join("%.1f" % x for x in smp[k])), flush=True)

m.render_status()                                    # every origin of the run was inside the innermost sphere
print(json.dumps({"render_views_bench": results, "a_ratio_singles_over_views": round(ratio, 3)}))
if a.out:
    with open(a.out, "w") as f:
        json.dump({"render_views_bench": results, "a_ratio_singles_over_views": ratio}, f, indent=1)
