#!/usr/bin/env python
"""Views straight from the factors of a high-res stack (MSI.render_views on a FactoredLayers: msi_render_views_factored) against
building the stack and rendering it.  Stacks of 4096x2048x32 over a 640x320 network and of 1280x640x32 over 640x320; per size
  pinhole V = 1, 2, 8 eyes at 1024 x 1024; one equirect view at the stack's size; the ODS pair at 640 x 320
and per case five forms:
  (a)  materialize_layers(f, 'f32') + render_views      (a') render_views of that fp32 stack alone
  (b)  materialize_layers(f, 'rgba8') + render_views    (b') render_views of that packed stack alone
  (c)  render_views(f)
materialize_layers is msi_hres_layers on the stored pieces -- hres_layers without its preprocessing and pose composition, which
favours (a) and (b).  Before anything is timed (c) is compared with (a') at the timed size (== per element) and the status word is
read.  Device events around a window of calls (at least --iters calls and --window_ms long, set from one calibration window after the
warm-up), --repeats repeats in which the five forms ALTERNATE (one process); per form the median and the repeat spread (min .. max).
Per full form also torch.cuda.max_memory_allocated over one call, above what is resident before it (the factors and the views).
Inputs are device-side (no host check, no sync inside a window).
--variants name=LIB,...: other builds of the library (tools/build_variants.sh noskip::-DMSI_FACTORED_SKIP=0 for the A/B of the zero-alpha
skip, w4::-DMSI_FACTORED_WAVES=4 for an occupancy); each one's msi_render_views_factored, called directly, alternates with the installed one's on blocky
low-res alpha masks (tools/sparse_views_bench.py's, scaled to the low-res grid: 10 x 10 blocks of layers 1.. switched on at random) at
occupancy 1.0 and ~0.2, at the first size, after its pixels are compared with the installed build's.
Nothing is gated on these numbers.
  python tools/hres_factored_bench.py [--variants noskip=tools/_variants/libmsi_noskip.so] [--out results.json] > profiles/hres_factored_timing.txt"""
import argparse
import ctypes
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
ap.add_argument("--sizes", default="4096x2048,1280x640", help="stack sizes WxH, comma-separated")
ap.add_argument("--low", default="640x320", help="the network's size WxH")
ap.add_argument("--planes", type=int, default=32)
ap.add_argument("--variants", default=None, help="name=library,...: other builds of the library whose factored viewer alternates with the installed one")
ap.add_argument("--out", default=None, help="write the results as JSON here")
a = ap.parse_args()

from matryodshka_amd import MSI, _native as N
from matryodshka_amd.synthetic import make_inputs

D = a.planes
LW, LH = (int(x) for x in a.low.split("x"))
m = MSI()
planes = m.inv_depths(1.0, 100.0, D)
rng = np.random.RandomState(5)


def factors(h, w, seed, occupancy=None):
    """Seeded uniform (0,1) blend weights and alphas over make_inputs images (a 40 x 88 tile repeated to the size); occupancy: the blocky mask."""
    g = torch.Generator(device="cuda").manual_seed(seed)
    bw = torch.rand((1, LH, LW, D), generator=g, device="cuda")
    al = torch.rand((1, LH, LW, D), generator=g, device="cuda").clamp_(min=2.0 ** -20)
    if occupancy is not None:
        p = 1.0 if occupancy >= 1.0 else max((occupancy * D - 1.0) / (D - 1.0), 0.0)      # layer 0 is always seen
        on = torch.rand((1, (LH + 9) // 10, (LW + 9) // 10, D), generator=g, device="cuda") < p
        on = on.repeat_interleave(10, 1).repeat_interleave(10, 2)[:, :LH, :LW]
        on[..., 0] = True
        al = torch.where(on, al, torch.zeros_like(al))
    inp = make_inputs(seed + 1, 1, 40, 88)
    tile = lambda x: torch.from_numpy(np.ascontiguousarray(np.tile(x, (1, -(-h // 40), -(-w // 88), 1))[:, :h, :w]))
    src_pose = inp["src_pose"].copy()
    src_pose[:, :3, 3] = (0.03, 0.01, -0.02)          # the two sources do not share their quadratic
    return m.hres_factors(bw, al, tile(inp["ref_image"]), tile(inp["src_image"]), inp["ref_pose"], src_pose, planes, inp["intrinsics"])


def views(v):
    pose = np.tile(np.eye(4, dtype=np.float32), (1, v, 1, 1))
    for k in range(v):
        ang = rng.uniform(-np.pi, np.pi)
        pose[0, k, 0, 0], pose[0, k, 0, 2], pose[0, k, 2, 0], pose[0, k, 2, 2] = np.cos(ang), np.sin(ang), -np.sin(ang), np.cos(ang)
        pose[0, k, :3, 3] = rng.uniform(-0.05, 0.05, 3)
    pos = rng.uniform(-0.05, 0.05, size=(1, v, 3)).astype(np.float32)
    return torch.from_numpy(pose).cuda(), torch.from_numpy(pos).cuda()


K = torch.tensor([[512.0, 0, 512.0], [0, 512.0, 512.0], [0, 0, 1]]).cuda()
eye, baseline = torch.tensor([[1.0, -1.0]]).cuda(), torch.tensor(0.032).cuda()
dev_planes = torch.tensor(planes, dtype=torch.float32).cuda()


def workloads():
    w = {}
    for v in (1, 2, 8):
        pose, pos = views(v)
        w["pinhole V=%d 1024^2" % v] = lambda s, pose=pose, pos=pos: m.render_views(s, pose, pos, dev_planes, camera="pinhole", intrinsics=K, size=(1024, 1024))
    pose1, pos1 = views(1)
    w["equirect V=1 stack size"] = lambda s: m.render_views(s, pose1, pos1, dev_planes)
    pose2, pos2 = views(2)
    pose2[:, 1], pos2[:, 1] = pose2[:, 0], pos2[:, 0]                   # both eyes share the head
    w["ODS pair 640x320"] = lambda s: m.render_views(s, pose2, pos2, dev_planes, camera="ods", eye=eye, baseline=baseline, size=(320, 640))
    return w


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


def peak_bytes(fn):
    torch.cuda.synchronize()
    torch.cuda.empty_cache()
    torch.cuda.reset_peak_memory_stats()
    before = torch.cuda.memory_allocated()
    out = fn()
    torch.cuda.synchronize()
    peak = torch.cuda.max_memory_allocated() - before
    del out
    return int(peak)


def same(got, want):
    return all(bool((g == w).all()) for g, w in zip(got, want))


results = []
sizes = [tuple(int(x) for x in s.split("x")) for s in a.sizes.split(",")]
for w, h in sizes:
    f = factors(h, w, 20)
    f32_bytes, rgba8_bytes = h * w * D * 16, h * w * D * 4
    print("%dx%dx%d over %dx%d: factors %d bytes; the fp32 stack %d (x %.1f), rgba8 %d (x %.2f)" % (
        w, h, D, LW, LH, f.nbytes, f32_bytes, f32_bytes / f.nbytes, rgba8_bytes, rgba8_bytes / f.nbytes), flush=True)
    for name, fn in workloads().items():
        dense = m.materialize_layers(f, "f32")["rgba_layers"]
        packed = m.materialize_layers(f, "rgba8")["packed_layers"]
        assert same(fn(f), fn(dense)), (w, h, name)                      # the same pixels, at the timed size, before any timing
        torch.cuda.synchronize()
        assert m.render_status() == 0
        forms = {"(a) build f32 + render": lambda: fn(m.materialize_layers(f, "f32")["rgba_layers"]),
                 "(a') render f32": lambda: fn(dense),
                 "(b) build rgba8 + render": lambda: fn(m.materialize_layers(f, "rgba8")["packed_layers"]),
                 "(b') render rgba8": lambda: fn(packed),
                 "(c) render factors": lambda: fn(f)}
        samples, calls = measure(forms)
        del dense, packed
        peaks = {n: peak_bytes(forms[n]) for n in ("(a) build f32 + render", "(b) build rgba8 + render", "(c) render factors")}
        entry = dict(size="%dx%d" % (w, h), low="%dx%d" % (LW, LH), planes=D, case=name, factors_nbytes=f.nbytes, calls_per_window=calls,
                     forms={n: stats(v) for n, v in samples.items()}, peak_bytes_above_resident=peaks,
                     factors_over_build_f32=round(float(np.median(samples["(c) render factors"]) / np.median(samples["(a) build f32 + render"])), 3),
                     factors_over_build_rgba8=round(float(np.median(samples["(c) render factors"]) / np.median(samples["(b) build rgba8 + render"])), 3),
                     factors_over_render_f32=round(float(np.median(samples["(c) render factors"]) / np.median(samples["(a') render f32"])), 3))
        results.append(entry)
        print("  %s" % name, flush=True)
        for n, v in samples.items():
            print("    %-26s %10.1f us (%.1f .. %.1f)   %3d calls per window%s" % (
                n, np.median(v), min(v), max(v), calls[n], "   peak %d bytes" % peaks[n] if n in peaks else ""), flush=True)
        print("    (c) / (a) %.3f   (c) / (b) %.3f   (c) / (a') %.3f" % (
            entry["factors_over_build_f32"], entry["factors_over_build_rgba8"], entry["factors_over_render_f32"]), flush=True)
    del f
    torch.cuda.empty_cache()

skip = []
if a.variants:
    def entry_point(path):
        fn = ctypes.CDLL(os.path.abspath(path)).msi_render_views_factored
        fn.restype, fn.argtypes = N.SIGNATURES["msi_render_views_factored"]
        return fn

    def direct(fn, f, pose, pos, camera, size, intr=None):
        """One call of a build's msi_render_views_factored with the C argument list of include/msi_hip.h -> (rgb, depth)."""
        b, hh, hw, d = f.shape
        lh, lw = f.alphas.shape[1:3]
        v, (oh, ow) = pose.shape[1], size
        stack_trig, view_trig = m._trig(hh, hw), m._trig(oh, ow) if intr is None else None
        rgb = torch.empty((b, v, oh, ow, 3), dtype=torch.float32, device="cuda")
        dep = torch.empty((b, v, oh, ow), dtype=torch.float32, device="cuda")
        rc = fn(f.ref_image.data_ptr(), f.src_image.data_ptr(), f.ref_pose.data_ptr(), f.src_pose.data_ptr(), f.intrinsics.data_ptr(),
                dev_planes.data_ptr(), stack_trig.data_ptr(), f.blend_weights.data_ptr(), f.alphas.data_ptr(), b, lh, lw, hh, hw, d,
                pose.data_ptr(), pos.data_ptr(), None if intr is None else intr.data_ptr(), None,
                None if view_trig is None else view_trig.data_ptr(), v, camera, oh, ow, rgb.data_ptr(), dep.data_ptr(),
                m._render_status.data_ptr(), m._stream())
        assert rc == 0, N.last_error()
        return rgb, dep

    builds = {"installed": N.lib.msi_render_views_factored}
    builds.update((k, entry_point(v)) for k, v in (x.split("=") for x in a.variants.split(",")))
    w, h = sizes[0]
    pose2, pos2 = views(2)
    pose1, pos1 = views(1)
    K2 = K.expand(2, 3, 3).contiguous()
    cases = {"pinhole V=2 1024^2": lambda fn, f: direct(fn, f, pose2, pos2, N.MSI_CAMERA_PINHOLE, (1024, 1024), K2),
             "equirect V=1 stack size": lambda fn, f: direct(fn, f, pose1, pos1, N.MSI_CAMERA_EQUIRECT, (h, w))}
    for occ in (1.0, 0.2):
        f = factors(h, w, 30, occupancy=occ)
        seen = float((f.alphas != 0).float().mean())
        print("builds of the factored viewer at %dx%dx%d, blocky masks, low-res alphas != 0: %.3f (asked %.2f)" % (w, h, D, seen, occ), flush=True)
        for name, case in cases.items():
            forms = {k: (lambda fn=fn: case(fn, f)) for k, fn in builds.items()}
            want = forms["installed"]()
            for k, form in forms.items():
                assert same(form(), want), (occ, name, k)
            del want
            samples, calls = measure(forms)
            entry = dict(size="%dx%d" % (w, h), case=name, asked=occ, alphas_nonzero=round(seen, 4), builds={})
            for k, v in samples.items():
                r = [x / y for x, y in zip(v, samples["installed"])]
                entry["builds"][k] = dict(stats(v), over_installed=dict(median=round(float(np.median(r)), 3), min=round(min(r), 3), max=round(max(r), 3)))
                print("  %-26s %-10s %10.1f us (%.1f .. %.1f)   / installed %.3f (%.3f .. %.3f)" % (
                    name, k, np.median(v), min(v), max(v), np.median(r), min(r), max(r)), flush=True)
            skip.append(entry)
        del f
m.render_status()
out = {"hres_factored_bench": results, "builds_ab": skip, "iters": a.iters, "window_ms": a.window_ms, "repeats": a.repeats}
print(json.dumps(out))
if a.out:
    with open(a.out, "w") as fh:
        json.dump(out, fh, indent=1)
