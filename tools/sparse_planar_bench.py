#!/usr/bin/env python
"""Sparse against dense packed stacks in the planar and cube view renders (MSI.cube_render_views / mpi_render_views on an edge-rule
SparseLayers against the PackedLayers it was made from: the dense rgba8 kernels are the yardstick), and what
MSI.sparsify_layers(border='edge') itself costs.  rgba8 stacks at synthetic occupancies (blocky masks, tools/sparse_views_bench.py's
generator: 64 x 64-texel blocks of layers 1.. switched on at random; layer 0 is always kept, so the occupancy asked for is
approached, and the one measured is printed):
  cube  6 x 256^2 x 32:  (i) one 640 x 320 panorama;  (ii) 8 of them;  (iii) two 1024 x 1024 pinhole eyes;
  MPI   256^2 x 32:      (iv) 8 views at the stack's size.
Before anything is timed every sparse output is compared with the dense one at the timed size (torch.equal: == per element).  Device
events around a window of calls, one warm-up pass, --repeats repeats in which dense and sparse ALTERNATE (one process); per form the
median and the repeat spread (min .. max), and sparse / dense from the per-repeat ratios (< 1: sparse is faster).  A window is at
least --iters calls and at least --window_ms long: each form's call count is set from one calibration window after the warm-up and
printed.  Inputs are device-side (no host check, no sync).  Also printed: nbytes dense against sparse.  Nothing is gated on these
numbers.  Kernel times and resources: run this under `rocprofv3 --kernel-trace --stats` in a run of its own."""
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
ap.add_argument("--face", type=int, default=256, help="cube face and MPI size S")
ap.add_argument("--occupancies", default="1.0,0.5,0.25,0.1")
ap.add_argument("--planes", type=int, default=32)
ap.add_argument("--out", default=None, help="write the results as JSON here")
a = ap.parse_args()

from matryodshka_amd import MSI
from matryodshka_amd.packed import PackedLayers

D, S, BLOCK = a.planes, a.face, 64
m = MSI()
planes = m.inv_depths(1.0, 100.0, D)
rng = np.random.RandomState(3)


def stack(n, occupancy, seed):
    """rgba8 codes [n,D,S,S,4] on the device: random colours, alpha in 1..255 inside the blocks that are on and 0 elsewhere."""
    g = torch.Generator(device="cuda").manual_seed(seed)
    codes = torch.randint(0, 256, (n, D, S, S, 4), generator=g, device="cuda", dtype=torch.uint8)
    p = 1.0 if occupancy >= 1.0 else max((occupancy * D - 1.0) / (D - 1.0), 0.0)     # layer 0 is kept whole
    on = torch.rand((n, D, (S + BLOCK - 1) // BLOCK, (S + BLOCK - 1) // BLOCK), generator=g, device="cuda") < p
    on = on.repeat_interleave(BLOCK, 2).repeat_interleave(BLOCK, 3)[:, :, :S, :S]
    codes[..., 3] = torch.where(on, torch.clamp(codes[..., 3], min=1), torch.zeros_like(codes[..., 3]))
    return PackedLayers(codes, "rgba8", planes)


def cube_views(v):
    pose = np.tile(np.eye(4, dtype=np.float32), (1, v, 1, 1))
    for k in range(v):
        ang = rng.uniform(-np.pi, np.pi)
        pose[0, k, 0, 0], pose[0, k, 0, 2], pose[0, k, 2, 0], pose[0, k, 2, 2] = np.cos(ang), np.sin(ang), -np.sin(ang), np.cos(ang)
        pose[0, k, :3, 3] = rng.uniform(-0.05, 0.05, 3)
    pos = rng.uniform(-0.05, 0.05, size=(1, v, 3)).astype(np.float32)
    return torch.from_numpy(pose).cuda(), torch.from_numpy(pos).cuda()


def mpi_views(v):
    pose = np.tile(np.eye(4, dtype=np.float32), (1, v, 1, 1))
    for k in range(v):
        ang = rng.uniform(-0.1, 0.1)
        pose[0, k, 0, 0], pose[0, k, 0, 2], pose[0, k, 2, 0], pose[0, k, 2, 2] = np.cos(ang), np.sin(ang), -np.sin(ang), np.cos(ang)
        pose[0, k, :3, 3] = rng.uniform(-0.05, 0.05, 3)
    return torch.from_numpy(pose).cuda()


pose1, pos1 = cube_views(1)
pose8, pos8 = cube_views(8)
pose2, pos2 = cube_views(2)
pose2[:, 1], pos2[:, 1] = pose2[:, 0], pos2[:, 0]                   # both eyes share the head
K_eye = torch.tensor([[512.0, 0, 512.0], [0, 512.0, 512.0], [0, 0, 1]]).cuda()
K_mpi = torch.tensor([[S / 2.0, 0, S / 2.0], [0, S / 2.0, S / 2.0], [0, 0, 1]]).cuda()
mpi_pose8 = mpi_views(8)
CUBE = {"(i) cube, 1 panorama 640x320": lambda s: m.cube_render_views(s, pose1, pos1, size=(320, 640)),
        "(ii) cube, 8 panoramas 640x320": lambda s: m.cube_render_views(s, pose8, pos8, size=(320, 640)),
        "(iii) cube, 2 pinhole 1024^2": lambda s: m.cube_render_views(s, pose2, pos2, camera="pinhole", intrinsics=K_eye, size=(1024, 1024))}
MPI = {"(iv) MPI, 8 views %dx%d" % (S, S): lambda s: m.mpi_render_views(s, mpi_pose8, intrinsics=K_mpi)}


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
for kind, n, workloads in (("cube 6x%dx%dx%d" % (S, S, D), 6, CUBE), ("MPI %dx%dx%d" % (S, S, D), 1, MPI)):
    for k, occ in enumerate(float(x) for x in a.occupancies.split(",")):
        dense = stack(n, occ, 10 + k)
        sparse = m.sparsify_layers(dense, border='edge')
        entry = dict(stack=kind, planes=D, asked=occ, occupancy=round(sparse.occupancy, 4), dense_nbytes=dense.nbytes, sparse_nbytes=sparse.nbytes)
        print("%s rgba8, occupancy %.3f (asked %.2f): %d bytes dense, %d sparse (x %.3f)" % (
            kind, sparse.occupancy, occ, dense.nbytes, sparse.nbytes, sparse.nbytes / float(dense.nbytes)), flush=True)
        forms = {}
        for name, fn in workloads.items():
            for got, ref in zip(fn(sparse), fn(dense)):      # the same pixels, at the timed size, before any timing
                assert torch.equal(got, ref), (kind, occ, name)
            del got, ref
            forms[name + " dense"] = lambda fn=fn: fn(dense)
            forms[name + " sparse"] = lambda fn=fn: fn(sparse)
        forms["sparsify_layers"] = lambda: m.sparsify_layers(dense, border='edge')
        for fn in forms.values():                    # warm-up: trig tables cached, kernels loaded
            fn()
        torch.cuda.synchronize()
        calls = {nm: max(a.iters, int(np.ceil(a.window_ms * 1e3 / timed(fn, a.iters)))) for nm, fn in forms.items()}     # the calibration window
        for name in workloads:                       # dense and sparse of a workload: the same number of calls
            calls[name + " dense"] = calls[name + " sparse"] = max(calls[name + " dense"], calls[name + " sparse"])
        entry["calls_per_window"] = calls
        print("  calls per window: " + ", ".join("%s %d" % (nm, calls[nm + " dense"]) for nm in workloads) + ", sparsify_layers %d" % calls["sparsify_layers"], flush=True)
        samples = {nm: [] for nm in forms}
        for _ in range(a.repeats):
            for nm, fn in forms.items():
                samples[nm].append(timed(fn, calls[nm]))
        m.render_status()                            # every origin of the run was inside the innermost shell
        for name in workloads:
            d, s = samples[name + " dense"], samples[name + " sparse"]
            r = [x / y for x, y in zip(s, d)]        # per repeat: the two forms ran back to back
            entry[name] = dict(dense=stats(d), sparse=stats(s),
                               sparse_over_dense=dict(median=round(float(np.median(r)), 3), min=round(min(r), 3), max=round(max(r), 3)))
            print("  %-32s dense %9.1f us (%.1f .. %.1f)   sparse %9.1f us (%.1f .. %.1f)   sparse / dense %.3f (%.3f .. %.3f)" % (
                name, np.median(d), min(d), max(d), np.median(s), min(s), max(s), np.median(r), min(r), max(r)), flush=True)
        entry["sparsify_layers"] = stats(samples["sparsify_layers"])
        print("  %-32s %9.1f us (%.1f .. %.1f), one host synchronisation included" % (
            "sparsify_layers", np.median(samples["sparsify_layers"]), min(samples["sparsify_layers"]), max(samples["sparsify_layers"])), flush=True)
        results.append(entry)
        del dense, sparse, forms
        torch.cuda.empty_cache()
print(json.dumps({"sparse_planar_bench": results, "iters": a.iters, "window_ms": a.window_ms, "repeats": a.repeats}))
if a.out:
    with open(a.out, "w") as f:
        json.dump({"sparse_planar_bench": results, "iters": a.iters, "window_ms": a.window_ms, "repeats": a.repeats}, f, indent=1)
