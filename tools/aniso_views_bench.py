#!/usr/bin/env python
"""Anisotropic filtering of mip-mapped stacks (MSI.render_views on a MipLayers with max_anisotropy > 1: msi_render_views_aniso): what the
mode costs per view against the trilinear render (msi_render_views_mip) of the same stack in the same build.
  stack        4096x2048x32, rgba8 and fp32, all levels the sizes allow
  workloads    two 1024^2 pinhole eyes (fx = 512) at the horizon -- footprints about 1 : 1, little for the filter to do --; the same
               eyes looking straight up at the stack's pole, where a footprint is many texels long; a centred 640x320 panorama with
               the identity pose -- every footprint is a square, every ratio 1 up to the rounding of the hits, which puts most lanes
               a hair above 1 and so at M = 1: the reading is the price of the Jacobian AND of two samples of next to no weight --;
               the same panorama tilted by 90 degrees, the stack's poles on its equator
  forms        trilinear, max_anisotropy 4 and 16
Device events around a window of calls (at least --iters calls and --window_ms long, set from one calibration window after the
warm-up), --repeats repeats in which the forms ALTERNATE (one process); per form the median and the repeat spread (min .. max), per
cap the quotient of each repeat's times.  Before a case is timed, its lod_bias = -64 render at the cap 16 is compared == with the
trilinear entry point's.  Inputs are device-side (no host check, no sync inside a window).  Nothing is gated on these numbers.
  python tools/aniso_views_bench.py [--out results.json] > profiles/aniso_views_timing.txt"""
import argparse
import json
import os
import sys

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import numpy as np
import torch

ap = argparse.ArgumentParser()
ap.add_argument("--iters", type=int, default=2, help="calls per timed window, at least")
ap.add_argument("--window_ms", type=float, default=40.0, help="a timed window is at least this long")
ap.add_argument("--repeats", type=int, default=5, help="alternated repeats; median and min .. max are reported")
ap.add_argument("--size", default="4096x2048", help="stack size WxH")
ap.add_argument("--formats", default="rgba8,f32")
ap.add_argument("--planes", type=int, default=32)
ap.add_argument("--caps", default="4,16")
ap.add_argument("--out", default=None, help="write the results as JSON here")
a = ap.parse_args()

from matryodshka_amd import MSI
from matryodshka_amd.packed import PackedLayers

D = a.planes
CAPS = [float(c) for c in a.caps.split(",")]
m = MSI()
planes = m.inv_depths(1.0, 100.0, D)
dev_planes = torch.tensor(planes, dtype=torch.float32).cuda()


def stack(h, w, fmt, seed):
    """A native stack of seeded noise with blocky alphas (a third of the 16 x 16 blocks of the layers above 0 transparent), made
    in the texel format itself (tools/mip_views_bench.py's)."""
    g = torch.Generator(device="cuda").manual_seed(seed)
    on = (torch.rand((1, D, (h + 15) // 16, (w + 15) // 16, 1), generator=g, device="cuda") > 1.0 / 3).repeat_interleave(16, 2).repeat_interleave(16, 3)[:, :, :h, :w]
    on[:, 0] = True
    if fmt == "rgba8":
        data = torch.randint(0, 256, (1, D, h, w, 4), generator=g, device="cuda", dtype=torch.uint8)
        data[..., 3:] *= on
        return PackedLayers(data, fmt, planes)
    x = torch.rand((1, D, h, w, 4), generator=g, device="cuda")
    x[..., :3] = x[..., :3] * 2 - 1
    x[..., 3:] *= on
    return x.permute(0, 2, 3, 1, 4)


def rot(i, j, deg):
    """Rotation by deg in the (i, j) plane, as a pose."""
    c, s = np.cos(np.deg2rad(deg)), np.sin(np.deg2rad(deg))
    P = np.eye(4, dtype=np.float32)
    P[i, i], P[i, j], P[j, i], P[j, j] = c, -s, s, c
    return P


def device(pose, v):
    pose = np.tile(pose[None, None], (1, v, 1, 1))
    pos = np.zeros((1, v, 3), np.float32)
    if v == 2:
        pos[0, :, 0] = (-0.03, 0.03)                  # two eyes, 6 cm apart; a single panorama is centred
    return torch.from_numpy(pose).cuda(), torch.from_numpy(pos).cuda()


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


def measure(forms):
    """Warm-up, one calibration window, then --repeats alternated rounds -> {form: [us per call]} and the calls per window."""
    for fn in forms.values():
        fn()
    torch.cuda.synchronize()
    calls = {n: max(a.iters, int(np.ceil(a.window_ms * 1e3 / timed(fn, a.iters)))) for n, fn in forms.items()}
    samples = {n: [] for n in forms}
    for _ in range(a.repeats):
        for n, fn in forms.items():
            samples[n].append(timed(fn, calls[n]))
    return samples, calls


w, h = (int(x) for x in a.size.split("x"))
K = torch.tensor([[512.0, 0, 512.0], [0, 512.0, 512.0], [0, 0, 1]]).cuda()
eyes = dict(camera="pinhole", intrinsics=K, size=(1024, 1024))
pano = dict(size=(320, 640))
cases = [("pinhole V=2 1024^2, at the horizon", device(np.eye(4, dtype=np.float32), 2), eyes),
         ("pinhole V=2 1024^2, looking straight up", device(rot(0, 1, 90.0), 2), eyes),
         ("equirect V=1 640x320, identity pose (every ratio 1 up to rounding)", device(np.eye(4, dtype=np.float32), 1), pano),
         ("equirect V=1 640x320, tilted by 90 degrees", device(rot(1, 2, 90.0), 1), pano)]

results = []
for fmt in a.formats.split(","):
    mip = m.build_mips(stack(h, w, fmt, 30))
    print("views of the %s x %d %s stack, L = %d" % (a.size, D, fmt, mip.levels), flush=True)
    for name, (pose, pos), kw in cases:
        def fn(pose=pose, pos=pos, kw=kw, **more):
            return m.render_views(mip, pose, pos, dev_planes, **kw, **more)
        want, got = fn(lod_bias=-64.0), fn(lod_bias=-64.0, max_anisotropy=max(CAPS))
        assert all(bool((g == r).all()) for g, r in zip(got, want)), name      # level 0 alone from either entry point, before any timing
        del want, got
        forms = {"trilinear": fn}
        for cap in CAPS:
            forms["max_anisotropy %g" % cap] = lambda cap=cap: fn(max_anisotropy=cap)
        samples, calls = measure(forms)
        entry = dict(format=fmt, case=name, forms={n: stats(v) for n, v in samples.items()}, calls_per_window=calls, over_trilinear={})
        print("  %s" % name, flush=True)
        for n, v in samples.items():
            print("    %-20s %10.1f us (%.1f .. %.1f)   %3d calls per window" % (n, np.median(v), min(v), max(v), calls[n]), flush=True)
        for cap in CAPS:
            q = [x / y for x, y in zip(samples["max_anisotropy %g" % cap], samples["trilinear"])]
            entry["over_trilinear"]["%g" % cap] = dict(median=round(float(np.median(q)), 3), min=round(min(q), 3), max=round(max(q), 3))
            print("    max_anisotropy %g / trilinear %.3f (%.3f .. %.3f)" % (cap, np.median(q), min(q), max(q)), flush=True)
        results.append(entry)
    del mip
    torch.cuda.empty_cache()
torch.cuda.synchronize()
m.render_status()
out = {"aniso_views": results, "size": a.size, "planes": D, "iters": a.iters, "window_ms": a.window_ms, "repeats": a.repeats}
print(json.dumps(out))
if a.out:
    with open(a.out, "w") as fh:
        json.dump(out, fh, indent=1)
