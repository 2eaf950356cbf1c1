#!/usr/bin/env python
"""MSI.mpi_render_views timing: many views of one 256x256x32 MPI per launch.  Device events around --iters calls, one warm-up
pass, the median of --repeats repeats in which the compared forms ALTERNATE (one process); before anything is timed the
outputs of the compared forms are checked bit for bit.  Cases:
  (a) V = 2 and V = 8 views at 256x256 of B = 1 and B = 64 stacks: ONE mpi_render_views call (rgb only, as the single-view
      render writes) vs V back-to-back mpi_render_view calls on the same stacks -- those calls run mpi_render_kernel, which
      this tool's subject does not touch: the yardstick.  Every view of the one call must equal its single-view render.
  (b) the same calls with rgb + depth from the fp32 stack and from its rgba8 / rgba16f PackedLayers, alternated; each
      packed form is reported with its ratio to fp32 from the same process (> 1: the packed form is slower) and must equal
      the render of its unpacked stack.
  (c) V = 2 and V = 8 views at 1024x1024 from one 256x256x32 stack, the three formats alternated.
All poses, cameras and planes are device tensors (no host inversion, no sync inside a timed window).  Per case: us per call,
views/s, and the byte floor -- each stack read once + the output bytes -- over 8 TB/s as a share of the measured time (a
floor, not a roofline).  Kernel times: run this under `rocprofv3 --kernel-trace --stats` in a run of its own (--repeats 1)."""
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
ap.add_argument("--big-batch", type=int, default=64, help="the larger batch of cases (a) and (b)")
ap.add_argument("--out", default=None, help="write the results as JSON here")
a = ap.parse_args()

from matryodshka_amd import MSI

HBM = 8e12
H, W, D = 256, 256, 32
TEXEL_BYTES = {"f32": 16, "rgba8": 4, "rgba16f": 8}
m = MSI()
planes = torch.tensor(m.inv_depths(1.0, 100.0, D), dtype=torch.float32).cuda()
gd = torch.Generator(device="cuda").manual_seed(0)


def camera(h, w):
    return np.array([[w / 2, 0, w / 2], [0, h / 2, h / 2], [0, 0, 1]], np.float32)


def stacks(b):
    native = torch.rand((b, D, H, W, 4), generator=gd, device="cuda")
    native[..., :3] = native[..., :3] * 2 - 1
    return native.permute(0, 2, 3, 1, 4)             # the [B,H,W,D,4] view of the native stack (no copy on the way in)


def poses(b, v):
    """Head-motion sized: a few degrees about y, a few centimetres of translation."""
    rng = np.random.RandomState(b * 100 + v)
    pose = np.tile(np.eye(4, dtype=np.float32), (b, v, 1, 1))
    for i in range(b):
        for k in range(v):
            ang = rng.uniform(-0.05, 0.05)
            c, s = np.cos(ang), np.sin(ang)
            pose[i, k, 0, 0], pose[i, k, 0, 2], pose[i, k, 2, 0], pose[i, k, 2, 2] = c, s, -s, c
            pose[i, k, :3, 3] = rng.uniform(-0.05, 0.05, 3)
    return torch.from_numpy(pose).cuda()


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


results = []


def report(case, us, b, v, oh, ow, samples, out_bytes_per_pixel, fmt="f32", f32_us=None):
    out_bytes = b * v * oh * ow * out_bytes_per_pixel
    floor_us = (b * H * W * D * TEXEL_BYTES[fmt] + out_bytes) / HBM * 1e6
    r = dict(case=case, us_per_call=round(us, 2), views_per_s=round(b * v / us * 1e6, 1), batch=b, views=v, size=[oh, ow],
             format=fmt, byte_floor_us=round(floor_us, 2), byte_floor_share_of_8TBps=round(floor_us / us, 3),
             samples_us=[round(x, 2) for x in samples])
    if f32_us is not None and fmt != "f32":
        r.update(ratio_to_f32=round(us / f32_us, 3))
    results.append(r)
    print("%-46s %9.1f us/call  %9.0f views/s   byte floor %.1f us = %.2f of the measured time at 8 TB/s  (repeats %s)" % (
        case, us, r["views_per_s"], floor_us, floor_us / us, ", ".join("%.1f" % x for x in samples)), flush=True)
    return r


def formats(case, layers, b, v, pose, k_s, k_inv, size):
    """rgb + depth from the fp32 stack and its two packed forms, alternated; each packed render == the render of its unpacked stack."""
    forms_ = {"f32": layers, "rgba8": m.pack_layers(layers, "rgba8"), "rgba16f": m.pack_layers(layers, "rgba16f")}
    call = lambda s: m.mpi_render_views(s, pose, planes, k_s, intrinsics_inv=k_inv, size=size)
    for k in ("rgba8", "rgba16f"):
        got, want = call(forms_[k]), call(m.unpack_layers(forms_[k]))
        assert torch.equal(got[0], want[0]) and torch.equal(got[1], want[1]), "%s: packed != unpacked (%s)" % (case, k)
    med, smp = measure({k: (lambda s=s: call(s)) for k, s in forms_.items()})
    for k in forms_:
        report("%s [%s]" % (case, k), med[k], b, v, size[0], size[1], smp[k], 16, k, med["f32"])
        if k != "f32":
            print("    %s / fp32 = %.3f" % (k, med[k] / med["f32"]), flush=True)


ratios = {}
for b in (1, a.big_batch):
    layers = stacks(b)
    k_s = torch.from_numpy(np.tile(camera(H, W)[None], (b, 1, 1))).cuda()
    for v in (2, 8):
        pose = poses(b, v)
        k_inv = torch.linalg.inv(k_s.cpu().double()).float().cuda()
        k_inv_v = k_inv[:, None].expand(b, v, 3, 3).contiguous()
        singles_args = [pose[:, k].contiguous() for k in range(v)]

        def one_call():
            return m.mpi_render_views(layers, pose, planes, k_s, intrinsics_inv=k_inv_v, want_depth=False)[0]

        def singles():
            return [m.mpi_render_view(layers, p, planes, k_s, k_inv) for p in singles_args]

        # bit for bit before timing
        got, want = one_call(), singles()
        for k in range(v):
            assert torch.equal(got[:, k], want[k]), "(a) B=%d V=%d: view %d differs from its single-view render" % (b, v, k)
        del got, want
        med, smp = measure({"views": one_call, "singles": singles})
        report("(a) B=%d V=%d 256x256 rgb, one call" % (b, v), med["views"], b, v, H, W, smp["views"], 12)
        report("(a) B=%d V=%d 256x256 rgb, V single-view calls" % (b, v), med["singles"], b, v, H, W, smp["singles"], 12)
        ratios["B%d_V%d" % (b, v)] = med["singles"] / med["views"]
        print("(a) B=%d V=%d: V single calls / one call = %.3f (> 1: the one call is faster)" % (b, v, ratios["B%d_V%d" % (b, v)]), flush=True)
        formats("(b) B=%d V=%d 256x256 rgb+depth" % (b, v), layers, b, v, pose, k_s, k_inv_v, (H, W))
    if b == 1:
        k_t_inv = torch.linalg.inv(torch.from_numpy(camera(1024, 1024)).double()).float().cuda()
        for v in (2, 8):
            formats("(c) B=1 V=%d 1024x1024 rgb+depth" % v, layers, 1, v, poses(1, v), k_s, k_t_inv[None, None].expand(1, v, 3, 3).contiguous(),
                    (1024, 1024))
    del layers
    torch.cuda.empty_cache()

print(json.dumps({"mpi_views_bench": results, "a_ratio_singles_over_views": {k: round(x, 3) for k, x in ratios.items()}}))
if a.out:
    with open(a.out, "w") as f:
        json.dump({"mpi_views_bench": results, "a_ratio_singles_over_views": ratios}, f, indent=1)
