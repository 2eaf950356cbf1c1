#!/usr/bin/env python
"""MSI.render_views(camera='ods') timing at the size a user runs: both eyes of one 640x320x32 MSI per launch.  Device events
around --iters calls, one warm-up pass, --repeats repeats in which the compared forms ALTERNATE (one process); per form the
median and the repeat spread (min .. max).  Forms, all on the same stack with device-side inputs (no host check, no sync):
  (a) both eyes in ONE launch (msi_render_ods_views, V = 2, rgb + depth), 640x320;
  (b) two msi_render_ods_view launches (one eye each, rgb only, mirrored: what the project could do before);
  (c) render_views(camera='equirect'), V = 2, 640x320 (the kernel (a) moves the bytes of);
  (d) (a) from the rgba8 and the rgba16f PackedLayers of the stack;
  (e) (a) at a 1280x640 output from the same 640x320 stack.
Reported: us per call of each form, (a)/(b) and (a)/(c) with the spread of the per-repeat ratios.  No speed is promised: (a)
also writes depth, which (b) cannot.  Kernel times: run this under `rocprofv3 --kernel-trace --stats` in a run of its own."""
import argparse
import json
import os
import sys

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import numpy as np
import torch

ap = argparse.ArgumentParser()
ap.add_argument("--iters", type=int, default=20, help="calls per timed window")
ap.add_argument("--repeats", type=int, default=7, help="alternated repeats; median and min .. max are reported")
ap.add_argument("--out", default=None, help="write the results as JSON here")
a = ap.parse_args()

from matryodshka_amd import MSI

H, W, D, BASELINE = 320, 640, 32, 0.032
m = MSI()
planes = m.inv_depths(1.0, 100.0, D)
g = torch.Generator(device="cpu").manual_seed(0)
layers = torch.rand((1, D, H, W, 4), generator=g).cuda().permute(0, 2, 3, 1, 4)      # the [B,H,W,D,4] view of the native stack
packed = {f: m.pack_layers(layers, f) for f in ("rgba8", "rgba16f")}

rng = np.random.RandomState(2)
ang = rng.uniform(-np.pi, np.pi)
head = np.eye(4, dtype=np.float32)
head[0, 0], head[0, 2], head[2, 0], head[2, 2] = np.cos(ang), np.sin(ang), -np.sin(ang), np.cos(ang)
head[:3, 3] = rng.uniform(-0.05, 0.05, 3)
pose2 = torch.from_numpy(np.tile(head, (1, 2, 1, 1))).cuda()                         # both eyes share the head pose
pos2 = torch.from_numpy(np.tile(rng.uniform(-0.05, 0.05, 3).astype(np.float32), (1, 2, 1))).cuda()
pose1, zero1 = pose2[:, 0].contiguous(), torch.zeros((1, 3), device="cuda")
eye = torch.tensor([[1.0, -1.0]]).cuda()
baseline = torch.tensor(BASELINE).cuda()           # (device-side like eye: a host float would be copied over on every call)
intr = torch.tensor([[[BASELINE, 0, 0], [0, 1, 0], [0, 0, 1]]]).cuda()


def ods(stack, size=None):
    return m.render_views(stack, pose2, pos2, planes, camera="ods", eye=eye, baseline=baseline, size=size)


def two_single_eyes():
    m.msi_render_ods_view(layers, 1, pose1, zero1, planes, intr)
    m.msi_render_ods_view(layers, -1, pose1, zero1, planes, intr)


forms = {"(a) ods pair, one launch": lambda: ods(layers),
         "(b) 2 x msi_render_ods_view": two_single_eyes,
         "(c) equirect V=2": lambda: m.render_views(layers, pose2, pos2, planes),
         "(d) ods pair [rgba8]": lambda: ods(packed["rgba8"]),
         "(d) ods pair [rgba16f]": lambda: ods(packed["rgba16f"]),
         "(e) ods pair -> 1280x640": lambda: ods(layers, (2 * H, 2 * W))}


def timed(fn):
    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    e0.record()
    for _ in range(a.iters):
        fn()
    e1.record()
    e1.synchronize()
    return e0.elapsed_time(e1) * 1e3 / a.iters       # us per call


for fn in forms.values():                            # warm-up: trig tables cached, kernels loaded
    fn()
torch.cuda.synchronize()
samples = {k: [] for k in forms}
for _ in range(a.repeats):
    for k, fn in forms.items():
        samples[k].append(timed(fn))
m.render_status()                                    # every origin of the run was inside the innermost sphere

results = {}
for k, v in samples.items():
    results[k] = dict(median_us=round(float(np.median(v)), 2), min_us=round(min(v), 2), max_us=round(max(v), 2),
                      samples_us=[round(x, 2) for x in v])
    print("%-30s %9.1f us/call  (repeats %.1f .. %.1f)" % (k, np.median(v), min(v), max(v)), flush=True)


def ratio(num, den):
    r = [x / y for x, y in zip(samples[num], samples[den])]      # per repeat: the two forms ran back to back
    out = dict(median=round(float(np.median(r)), 3), min=round(min(r), 3), max=round(max(r), 3))
    print("%s / %s = %.3f  (repeats %.3f .. %.3f; < 1: the first is faster)" % (num, den, out["median"], out["min"], out["max"]),
          flush=True)
    return out


A = "(a) ods pair, one launch"
summary = {"a_over_b": ratio(A, "(b) 2 x msi_render_ods_view"), "a_over_c": ratio(A, "(c) equirect V=2"),
           "rgba8_over_a": ratio("(d) ods pair [rgba8]", A), "rgba16f_over_a": ratio("(d) ods pair [rgba16f]", A),
           "hi_over_a": ratio("(e) ods pair -> 1280x640", A)}
print(json.dumps({"ods_views_bench": results, "ratios": summary}))
if a.out:
    with open(a.out, "w") as f:
        json.dump({"ods_views_bench": results, "ratios": summary, "iters": a.iters, "repeats": a.repeats}, f, indent=1)
