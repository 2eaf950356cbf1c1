#!/usr/bin/env python
"""Sparse against dense packed stacks in the view renders (MSI.render_views on a SparseLayers against the PackedLayers it was made
from: the dense kernels are the yardstick), and what MSI.sparsify_layers itself costs.  rgba8 stacks of 640x320x32 and
4096x2048x32 at synthetic occupancies (blocky masks: 64 x 64-texel blocks of layers 1.. switched on at random; layer 0 is always
kept, so the occupancy asked for is approached, and the one measured is printed), three workloads each:
  (i)   8 equirect views at the stack's size;
  (ii)  two 1024 x 1024 pinhole eyes;
  (iii) the ODS pair at the stack's size.
Before anything is timed every sparse output is compared with the dense one at the timed size (torch.equal: == per element).  Device
events around a window of calls, one warm-up pass, --repeats repeats in which dense and sparse ALTERNATE (one process); per form the
median and the repeat spread (min .. max), and sparse / dense from the per-repeat ratios (< 1: sparse is faster).  A window is at
least --iters calls and at least --window_ms long: each form's call count is set from one calibration window after the warm-up (a
window of a millisecond measures the clock ramp and the host's enqueue rate as much as the kernel) and printed.  Inputs are
device-side (no host check, no sync).  Also printed: nbytes dense against sparse.  Nothing is gated on these numbers.
Kernel times and resources: run this under `rocprofv3 --kernel-trace --stats` in a run of its own."""
import argparse
import json
import os
import sys

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import numpy as np
import torch

ap = argparse.ArgumentParser()
ap.add_argument("--iters", type=int, default=5, help="calls per timed window, at least")
ap.add_argument("--window_ms", type=float, default=50.0, help="a timed window is at least this long: calls per window = max(--iters, window_ms / one call)")
ap.add_argument("--repeats", type=int, default=5, help="alternated repeats; median and min .. max are reported")
ap.add_argument("--sizes", default="640x320,4096x2048", help="stack sizes WxH, comma-separated")
ap.add_argument("--occupancies", default="1.0,0.5,0.25,0.1")
ap.add_argument("--planes", type=int, default=32)
ap.add_argument("--out", default=None, help="write the results as JSON here")
a = ap.parse_args()

from matryodshka_amd import MSI
from matryodshka_amd.packed import PackedLayers

D, BLOCK = a.planes, 64
m = MSI()
planes = m.inv_depths(1.0, 100.0, D)
rng = np.random.RandomState(3)


def stack(h, w, occupancy, seed):
    """rgba8 codes [1,D,H,W,4] on the device: random colours, alpha in 1..255 inside the blocks that are on and 0 elsewhere."""
    g = torch.Generator(device="cuda").manual_seed(seed)
    codes = torch.randint(0, 256, (1, D, h, w, 4), generator=g, device="cuda", dtype=torch.uint8)
    p = 1.0 if occupancy >= 1.0 else max((occupancy * D - 1.0) / (D - 1.0), 0.0)     # layer 0 is kept whole
    on = torch.rand((1, D, (h + BLOCK - 1) // BLOCK, (w + BLOCK - 1) // BLOCK), generator=g, device="cuda") < p
    on = on.repeat_interleave(BLOCK, 2).repeat_interleave(BLOCK, 3)[:, :, :h, :w]
    codes[..., 3] = torch.where(on, torch.clamp(codes[..., 3], min=1), torch.zeros_like(codes[..., 3]))
    return PackedLayers(codes, "rgba8", planes)


def views(v):
    pose = np.tile(np.eye(4, dtype=np.float32), (1, v, 1, 1))
    for k in range(v):
        ang = rng.uniform(-np.pi, np.pi)
        pose[0, k, 0, 0], pose[0, k, 0, 2], pose[0, k, 2, 0], pose[0, k, 2, 2] = np.cos(ang), np.sin(ang), -np.sin(ang), np.cos(ang)
        pose[0, k, :3, 3] = rng.uniform(-0.05, 0.05, 3)
    pos = rng.uniform(-0.05, 0.05, size=(1, v, 3)).astype(np.float32)
    return torch.from_numpy(pose).cuda(), torch.from_numpy(pos).cuda()


pose8, pos8 = views(8)
pose2, pos2 = views(2)
pose2[:, 1], pos2[:, 1] = pose2[:, 0], pos2[:, 0]                   # both eyes share the head
K = torch.tensor([[512.0, 0, 512.0], [0, 512.0, 512.0], [0, 0, 1]]).cuda()
eye, baseline = torch.tensor([[1.0, -1.0]]).cuda(), torch.tensor(0.032).cuda()
WORKLOADS = {"(i) 8 equirect views": lambda s: m.render_views(s, pose8, pos8),
             "(ii) 2 pinhole 1024^2": lambda s: m.render_views(s, pose2, pos2, camera="pinhole", intrinsics=K, size=(1024, 1024)),
             "(iii) ODS pair": lambda s: m.render_views(s, pose2, pos2, camera="ods", eye=eye, baseline=baseline)}


def timed(fn, iters):
    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    e0.record()
    for _ in range(iters):
        fn()
    e1.record()
    e1.synchronize()
    return e0.elapsed_time(e1) * 1e3 / iters         # us per call


def stats(v):
    return dict(median_us=round(float(np.median(v)), 1), min_us=round(min(v), 1), max_us=round(max(v), 1))


results = []
for size in a.sizes.split(","):
    w, h = (int(x) for x in size.split("x"))
    for k, occ in enumerate(float(x) for x in a.occupancies.split(",")):
        dense = stack(h, w, occ, 10 + k)
        sparse = m.sparsify_layers(dense)
        entry = dict(size=size, planes=D, asked=occ, occupancy=round(sparse.occupancy, 4), dense_nbytes=dense.nbytes, sparse_nbytes=sparse.nbytes)
        print("%s x %d rgba8, occupancy %.3f (asked %.2f): %d bytes dense, %d sparse (x %.3f)" % (
            size, D, sparse.occupancy, occ, dense.nbytes, sparse.nbytes, sparse.nbytes / float(dense.nbytes)), flush=True)
        forms = {}
        for name, fn in WORKLOADS.items():
            for got, ref in zip(fn(sparse), fn(dense)):      # the same pixels, at the timed size, before any timing
                assert torch.equal(got, ref), (size, occ, name)
            del got, ref
            forms[name + " dense"] = lambda fn=fn: fn(dense)
            forms[name + " sparse"] = lambda fn=fn: fn(sparse)
        forms["sparsify_layers"] = lambda: m.sparsify_layers(dense)
        for fn in forms.values():                    # warm-up: trig tables cached, kernels loaded
            fn()
        torch.cuda.synchronize()
        calls = {n: max(a.iters, int(np.ceil(a.window_ms * 1e3 / timed(fn, a.iters)))) for n, fn in forms.items()}     # the calibration window
        for name in WORKLOADS:                       # dense and sparse of a workload: the same number of calls
            calls[name + " dense"] = calls[name + " sparse"] = max(calls[name + " dense"], calls[name + " sparse"])
        entry["calls_per_window"] = calls
        print("  calls per window: " + ", ".join("%s %d" % (n, calls[n + " dense"]) for n in WORKLOADS) + ", sparsify_layers %d" % calls["sparsify_layers"], flush=True)
        samples = {n: [] for n in forms}
        for _ in range(a.repeats):
            for n, fn in forms.items():
                samples[n].append(timed(fn, calls[n]))
        m.render_status()                            # every origin of the run was inside the innermost sphere
        for name in WORKLOADS:
            d, s = samples[name + " dense"], samples[name + " sparse"]
            r = [x / y for x, y in zip(s, d)]        # per repeat: the two forms ran back to back
            entry[name] = dict(dense=stats(d), sparse=stats(s),
                               sparse_over_dense=dict(median=round(float(np.median(r)), 3), min=round(min(r), 3), max=round(max(r), 3)))
            print("  %-24s dense %9.1f us (%.1f .. %.1f)   sparse %9.1f us (%.1f .. %.1f)   sparse / dense %.3f (%.3f .. %.3f)" % (
                name, np.median(d), min(d), max(d), np.median(s), min(s), max(s), np.median(r), min(r), max(r)), flush=True)
        entry["sparsify_layers"] = stats(samples["sparsify_layers"])
        print("  %-24s %9.1f us (%.1f .. %.1f), one host synchronisation included" % (
            "sparsify_layers", np.median(samples["sparsify_layers"]), min(samples["sparsify_layers"]), max(samples["sparsify_layers"])), flush=True)
        results.append(entry)
        del dense, sparse, forms
        torch.cuda.empty_cache()
print(json.dumps({"sparse_views_bench": results, "iters": a.iters, "window_ms": a.window_ms, "repeats": a.repeats}))
if a.out:
    with open(a.out, "w") as f:
        json.dump({"sparse_views_bench": results, "iters": a.iters, "window_ms": a.window_ms, "repeats": a.repeats}, f, indent=1)
