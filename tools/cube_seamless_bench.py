#!/usr/bin/env python
"""MSI.cube_render_views(filtering='seamless') against filtering='clamp': what the seamless filter of the cube viewer costs.
One cube of six 256x256x32 PP face stacks (the cube camera fx = cx = 128), fp32 and its rgba8 PackedLayers.  Device events
around --iters calls, one warm-up pass, the median of --repeats windows in which the two filters ALTERNATE (one process).
Before anything is timed: the seamless packed render is checked bit for bit against the seamless render of the unpacked stack,
the share of pixels that differ from the clamp render is counted (the strip: about 2/S of the rays per shell), and the status
word is read (0: the cube camera was recognised).  Cases:
  (a) -> 640x320 equirect, V = 1        (b) -> 640x320 equirect, V = 8        (c) -> two 1024x1024 pinhole eyes (V = 2)
All poses, positions, cameras and planes are device tensors (no host check, no sync inside a timed window).
  python tools/cube_seamless_bench.py [--out results.json] > profiles/cube_seamless_timing.txt"""
import argparse
import json
import os
import sys

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import numpy as np
import torch

ap = argparse.ArgumentParser()
ap.add_argument("--iters", type=int, default=20, help="calls per timed window")
ap.add_argument("--repeats", type=int, default=7, help="alternated windows; the median is reported")
ap.add_argument("--out", default=None, help="write the results as JSON here")
a = ap.parse_args()

from matryodshka_amd import MSI, cubemap

S, D = 256, 32
m = MSI()
planes = torch.tensor(m.inv_depths(1.0, 100.0, D), dtype=torch.float32).cuda()
gd = torch.Generator(device="cuda").manual_seed(0)
native = torch.rand((6, D, S, S, 4), generator=gd, device="cuda")
native[..., :3] = native[..., :3] * 2 - 1
cube = native.permute(0, 2, 3, 1, 4)                 # the public view of the native stack (no copy on the way in)
stacks = {"f32": cube, "rgba8": m.pack_layers(cube, "rgba8")}
k_face = torch.from_numpy(cubemap.default_face_intrinsics(S)).cuda()


def views(v):
    """Head-motion sized: up to 0.3 rad about y, a few centimetres of translation and target position."""
    rng = np.random.RandomState(v)
    pose = np.tile(np.eye(4, dtype=np.float32), (1, v, 1, 1))
    for k in range(v):
        ang = rng.uniform(-0.3, 0.3)
        c, s = np.cos(ang), np.sin(ang)
        pose[0, k, 0, 0], pose[0, k, 0, 2], pose[0, k, 2, 0], pose[0, k, 2, 2] = c, s, -s, c
        pose[0, k, :3, 3] = rng.uniform(-0.05, 0.05, 3)
    pos = rng.uniform(-0.05, 0.05, (1, v, 3)).astype(np.float32)
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
    for fn in forms.values():
        fn()
    torch.cuda.synchronize()
    samples = {k: [] for k in forms}
    for _ in range(a.repeats):
        for k, fn in forms.items():
            samples[k].append(timed(fn))
    return samples


results = []


def run_case(case, v, camera, size, intrinsics):
    pose, pos = views(v)
    kw = dict(camera=camera, size=size, intrinsics=intrinsics)
    call = lambda layers, filtering: m.cube_render_views(layers, pose, pos, planes, k_face, filtering=filtering, **kw)
    got, want = call(stacks["rgba8"], "seamless"), call(m.unpack_layers(stacks["rgba8"]), "seamless")
    assert torch.equal(got[0], want[0]) and torch.equal(got[1], want[1]), "%s: packed != unpacked" % case
    clamp = call(stacks["f32"], "clamp")
    seam = call(stacks["f32"], "seamless")
    differ = float(((seam[0] != clamp[0]).any(dim=-1) | (seam[1] != clamp[1])).float().mean())
    torch.cuda.synchronize()
    assert m.render_status() == 0
    del got, want, clamp, seam
    for fmt, layers in stacks.items():
        smp = measure({"clamp": lambda: call(layers, "clamp"), "seamless": lambda: call(layers, "seamless")})
        med = {k: float(np.median(x)) for k, x in smp.items()}
        spread = {k: (max(x) - min(x)) / med[k] for k, x in smp.items()}
        r = dict(case=case, format=fmt, views=v, size=list(size), clamp_us=round(med["clamp"], 2), seamless_us=round(med["seamless"], 2),
                 ratio=round(med["seamless"] / med["clamp"], 3), pixels_differing=round(differ, 4),
                 clamp_windows_us=[round(x, 2) for x in smp["clamp"]], seamless_windows_us=[round(x, 2) for x in smp["seamless"]])
        results.append(r)
        print("%-28s %-6s clamp %9.1f us/call   seamless %9.1f us/call   x%.3f   (repeat spread clamp %.1f %%, seamless %.1f %%; %.1f %% of the "
              "pixels differ from clamp)" % (case, fmt, med["clamp"], med["seamless"], r["ratio"], 100 * spread["clamp"], 100 * spread["seamless"],
                                             100 * differ), flush=True)
        print("%-28s %-6s   windows clamp [%s]  seamless [%s]" % ("", "", ", ".join("%.1f" % x for x in smp["clamp"]),
                                                                    ", ".join("%.1f" % x for x in smp["seamless"])), flush=True)


for v in (1, 8):
    run_case("(%s) equirect 640x320 V=%d" % ("a" if v == 1 else "b", v), v, "equirect", (320, 640), None)
k_pin = torch.tensor([[512.0, 0, 512.0], [0, 512.0, 512.0], [0, 0, 1]]).cuda()
run_case("(c) pinhole 1024x1024 V=2", 2, "pinhole", (1024, 1024), k_pin)

print(json.dumps({"cube_seamless_bench": results}))
if a.out:
    with open(a.out, "w") as f:
        json.dump({"cube_seamless_bench": results}, f, indent=1)
