#!/usr/bin/env python
"""Mip-mapped stacks (MSI.build_mips, MSI.render_views on a MipLayers: msi_build_mips, msi_render_views_mip): what the pyramid costs
to build and what the trilinear texel costs -- or saves -- per view, against the plain render of the same stack in the same build.
  build_mips   at 4096x2048x32 and 640x320x32, rgba8 and fp32, all levels the sizes allow, against its HBM bound: (base bytes +
               level bytes) / 6.29 TB/s (the measured copy rate of the device)
  views        of the 4096x2048x32 rgba8 stack (--view_format): a 640x320 equirect view, V = 1 and 8 -- minified 6.4 x: trilinear reads
               coarse levels --, two 1024^2 pinhole eyes with fx = 512 (11.4 pixels per degree at the centre against the stack's 11.4
               texels: about 1 : 1, magnified towards the edges), and views at and above the stack's own size, where trilinear can
               only cost; per case the plain render of .base, the trilinear render, and the trilinear render with lod_bias = -64 (level 0
               alone: the price of the three rays and the level loop without a second level)
Device events around a window of calls (at least --iters calls and --window_ms long, set from one calibration window after the
warm-up), --repeats repeats in which the forms ALTERNATE (one process); per form the median and the repeat spread (min .. max).
Before a case is timed, its lod_bias = -64 render is compared == with the plain render.  Inputs are device-side (no host check, no
sync inside a window).  Nothing is gated on these numbers.
  python tools/mip_views_bench.py [--out results.json] > profiles/mip_views_timing.txt"""
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
ap.add_argument("--build_sizes", default="4096x2048,640x320", help="stack sizes WxH of the build_mips points, comma-separated")
ap.add_argument("--view_size", default="4096x2048", help="stack size WxH of the view points")
ap.add_argument("--view_format", default="rgba8")
ap.add_argument("--planes", type=int, default=32)
ap.add_argument("--out", default=None, help="write the results as JSON here")
a = ap.parse_args()

from matryodshka_amd import MSI
from matryodshka_amd.packed import PackedLayers

HBM_BYTES_PER_S = 6.29e12
D = a.planes
m = MSI()
planes = m.inv_depths(1.0, 100.0, D)
dev_planes = torch.tensor(planes, dtype=torch.float32).cuda()
rng = np.random.RandomState(5)


def stack(h, w, fmt, seed):
    """A native stack of seeded noise with blocky alphas (a third of the 16 x 16 blocks of the layers above 0 transparent), made
    in the texel format itself: uint8 codes, halves, or floats."""
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
    return PackedLayers(x.half(), fmt, planes) if fmt == "rgba16f" else x.permute(0, 2, 3, 1, 4)


def views(v):
    pose = np.tile(np.eye(4, dtype=np.float32), (1, v, 1, 1))
    for k in range(v):
        ang = rng.uniform(-np.pi, np.pi)
        pose[0, k, 0, 0], pose[0, k, 0, 2], pose[0, k, 2, 0], pose[0, k, 2, 2] = np.cos(ang), np.sin(ang), -np.sin(ang), np.cos(ang)
        pose[0, k, :3, 3] = rng.uniform(-0.05, 0.05, 3)
    pos = rng.uniform(-0.05, 0.05, size=(1, v, 3)).astype(np.float32)
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


def parse(s):
    w, h = (int(x) for x in s.split("x"))
    return h, w


builds = []
for size in a.build_sizes.split(","):
    h, w = parse(size)
    forms, bounds = {}, {}
    for fmt in ("rgba8", "f32"):
        layers = stack(h, w, fmt, 20)
        mip = m.build_mips(layers)
        base_bytes = mip.data.numel() * mip.data.element_size()
        bounds[fmt] = (mip.levels, base_bytes, mip.nbytes - base_bytes, mip.nbytes / HBM_BYTES_PER_S * 1e6)
        forms[fmt] = lambda layers=layers: m.build_mips(layers)
        del mip
    samples, calls = measure(forms)
    for fmt, v in samples.items():
        levels, base_bytes, level_bytes, bound_us = bounds[fmt]
        med = float(np.median(v))
        builds.append(dict(size=size, planes=D, format=fmt, levels=levels, base_bytes=base_bytes, level_bytes=level_bytes, hbm_bound_us=round(bound_us, 1),
                           calls_per_window=calls[fmt], over_bound=round(med / bound_us, 2), **stats(v)))
        print("build_mips %s x %d %-6s L = %d: %10.1f us (%.1f .. %.1f)   %d + %d bytes, HBM bound %.1f us, x %.2f of it   %d calls per window" % (
            size, D, fmt, levels, med, min(v), max(v), base_bytes, level_bytes, bound_us, med / bound_us, calls[fmt]), flush=True)
    del forms
    torch.cuda.empty_cache()

h, w = parse(a.view_size)
mip = m.build_mips(stack(h, w, a.view_format, 30))
base = mip.base if isinstance(mip.base, PackedLayers) else mip.base.permute(0, 2, 3, 1, 4)
print("views of the %s x %d %s stack, L = %d, %d + %d bytes" % (a.view_size, D, a.view_format, mip.levels, mip.nbytes - mip.mips.numel() * mip.mips.element_size(),
                                                              mip.mips.numel() * mip.mips.element_size()), flush=True)
K = torch.tensor([[512.0, 0, 512.0], [0, 512.0, 512.0], [0, 0, 1]]).cuda()
cases = {}
for v in (1, 8):
    pose, pos = views(v)
    cases["equirect V=%d 640x320 (minified)" % v] = lambda s, pose=pose, pos=pos, **kw: m.render_views(s, pose, pos, dev_planes, size=(320, 640), **kw)
pose2, pos2 = views(2)
cases["pinhole V=2 1024^2 (fx 512: 1 : 1 at the centre)"] = lambda s, **kw: m.render_views(s, pose2, pos2, dev_planes, camera="pinhole", intrinsics=K, size=(1024, 1024), **kw)
pose1, pos1 = views(1)
cases["equirect V=1 stack size"] = lambda s, **kw: m.render_views(s, pose1, pos1, dev_planes, **kw)
K4 = torch.tensor([[2048.0, 0, 2048.0], [0, 2048.0, 2048.0], [0, 0, 1]]).cuda()
cases["pinhole V=2 4096^2 (magnified)"] = lambda s, **kw: m.render_views(s, pose2, pos2, dev_planes, camera="pinhole", intrinsics=K4, size=(4096, 4096), **kw)

results = []
for name, fn in cases.items():
    want, got = fn(base), fn(mip, lod_bias=-64.0)
    assert all(bool((g == r).all()) for g, r in zip(got, want)), name       # level 0 alone: the plain render's pixels, before any timing
    del want, got
    forms = {"plain (.base)": lambda: fn(base), "trilinear": lambda: fn(mip), "trilinear, lod_bias -64": lambda: fn(mip, lod_bias=-64.0)}
    samples, calls = measure(forms)
    ratio = [x / y for x, y in zip(samples["trilinear"], samples["plain (.base)"])]
    results.append(dict(case=name, forms={n: stats(v) for n, v in samples.items()}, calls_per_window=calls,
                        trilinear_over_plain=dict(median=round(float(np.median(ratio)), 3), min=round(min(ratio), 3), max=round(max(ratio), 3))))
    print("  %s" % name, flush=True)
    for n, v in samples.items():
        print("    %-26s %10.1f us (%.1f .. %.1f)   %3d calls per window" % (n, np.median(v), min(v), max(v), calls[n]), flush=True)
    print("    trilinear / plain %.3f (%.3f .. %.3f)" % (np.median(ratio), min(ratio), max(ratio)), flush=True)
torch.cuda.synchronize()
m.render_status()
out = {"build_mips": builds, "mip_views": results, "iters": a.iters, "window_ms": a.window_ms, "repeats": a.repeats}
print(json.dumps(out))
if a.out:
    with open(a.out, "w") as fh:
        json.dump(out, fh, indent=1)
