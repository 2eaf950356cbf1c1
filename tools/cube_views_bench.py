#!/usr/bin/env python
"""MSI.cube_render_views timing: views of one cube of six 256x256x32 PP face stacks per launch.  Device events around --iters
calls, one warm-up pass, the median of --repeats windows in which the compared forms ALTERNATE (one process); before
anything is timed each packed render is checked bit for bit against the render of its unpacked stack.  Cases:
  (a) 6x256x256x32 -> 640x320 equirect, V = 1 and V = 8, from the fp32 cube and its rgba8 / rgba16f PackedLayers.
  (b) 6x256x256x32 -> pinhole 1024x1024, V = 2, the three formats.
Yardsticks, same process, same output sizes and views, alternated with the fp32 form of each case:
  render_views of a 640x320x32 MSI (the same tap count per output pixel: 4 taps x D shells), and
  six mpi_render_views launches over the same six face stacks (what a caller without cube_render_views has to do; each
  launch renders the whole output, zero-padded outside its face's frustum).
All poses, positions, cameras and planes are device tensors (no host check, no sync inside a timed window).  Next to each
time: the algorithmic byte floor of the gather, 4 taps x D x texel bytes per output pixel, over 8 TB/s (what the taps would
cost with no reuse in any cache: a yardstick, not a roofline; the stack itself is 201 / 50 / 101 MB).
  python tools/cube_views_bench.py [--out results.json] > profiles/cube_views_timing.txt"""
import argparse
import json
import os
import sys

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import numpy as np
import torch

ap = argparse.ArgumentParser()
ap.add_argument("--iters", type=int, default=20, help="calls per timed window")
ap.add_argument("--repeats", type=int, default=5, help="alternated windows; the median is reported")
ap.add_argument("--out", default=None, help="write the results as JSON here")
a = ap.parse_args()

from matryodshka_amd import MSI, cubemap

HBM = 8e12
S, D = 256, 32
MSI_H, MSI_W = 320, 640
TEXEL_BYTES = {"f32": 16, "rgba8": 4, "rgba16f": 8}
m = MSI()
planes = torch.tensor(m.inv_depths(1.0, 100.0, D), dtype=torch.float32).cuda()
gd = torch.Generator(device="cuda").manual_seed(0)


def stack(n, h, w):
    native = torch.rand((n, D, h, w, 4), generator=gd, device="cuda")
    native[..., :3] = native[..., :3] * 2 - 1
    return native.permute(0, 2, 3, 1, 4)             # the public view of the native stack (no copy on the way in)


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
    return {k: float(np.median(v)) for k, v in samples.items()}, samples


results = []


def report(case, form, us, v, oh, ow, samples, texel_bytes, ref_us=None):
    floor_us = 4.0 * D * texel_bytes * v * oh * ow / HBM * 1e6
    r = dict(case=case, form=form, us_per_call=round(us, 2), views_per_s=round(v / us * 1e6, 1), views=v, size=[oh, ow],
             tap_byte_floor_us=round(floor_us, 2), samples_us=[round(x, 2) for x in samples])
    if ref_us is not None:
        r["ratio_to_cube_f32"] = round(us / ref_us, 3)
    results.append(r)
    print("%-34s %-28s %9.1f us/call %9.0f views/s   tap-byte floor %7.1f us%s  (windows %s)" % (
        case, form, us, r["views_per_s"], floor_us, "" if ref_us is None else "   x%.3f of cube fp32" % (us / ref_us),
        ", ".join("%.1f" % x for x in samples)), flush=True)


cube = stack(6, S, S)
msi_stack = stack(1, MSI_H, MSI_W)
k_face = torch.from_numpy(cubemap.default_face_intrinsics(S)).cuda()
packed = {"rgba8": m.pack_layers(cube, "rgba8"), "rgba16f": m.pack_layers(cube, "rgba16f")}


def run_case(case, v, camera, size, intrinsics):
    pose, pos = views(v)
    kw = dict(camera=camera, size=size, intrinsics=intrinsics)
    call = lambda layers: m.cube_render_views(layers, pose, pos, planes, k_face, **kw)
    for name, p in packed.items():
        got, want = call(p), call(m.unpack_layers(p))
        assert torch.equal(got[0], want[0]) and torch.equal(got[1], want[1]), "%s: packed != unpacked (%s)" % (case, name)
        del got, want
    # six MPI launches over the six face stacks, each at the case's output size and view count with a 90-degree pinhole camera and
    # identity poses (every sample inside its face: the full tap cost; a launch's time does not depend on which face it reads)
    eye6 = [torch.eye(4, device="cuda").expand(1, v, 4, 4).contiguous() for _ in range(6)]
    k_out = torch.tensor([[size[1] / 2, 0, size[1] / 2], [0, size[0] / 2, size[0] / 2], [0, 0, 1]], dtype=torch.float32).cuda()
    k_out_inv = torch.linalg.inv(k_out.cpu().double()).float().cuda()[None, None].expand(1, v, 3, 3).contiguous()
    faces = [cube[f:f + 1] for f in range(6)]
    forms = {
        "cube f32": lambda: call(cube),
        "cube rgba8": lambda: call(packed["rgba8"]),
        "cube rgba16f": lambda: call(packed["rgba16f"]),
        "render_views 640x320x32 MSI": lambda: m.render_views(msi_stack, pose, pos, planes, **kw),
        "6 x mpi_render_views": lambda: [m.mpi_render_views(faces[f], eye6[f], planes, k_face, intrinsics_inv=k_out_inv, size=size)
                                         for f in range(6)],
    }
    med, smp = measure(forms)
    texel = {"cube f32": 16, "cube rgba8": 4, "cube rgba16f": 8, "render_views 640x320x32 MSI": 16, "6 x mpi_render_views": 16 * 6}
    for name in forms:
        report(case, name, med[name], v, size[0], size[1], smp[name], texel[name], None if name == "cube f32" else med["cube f32"])


for v in (1, 8):
    run_case("(a) equirect 640x320 V=%d" % v, v, "equirect", (MSI_H, MSI_W), None)
k_pin = torch.tensor([[512.0, 0, 512.0], [0, 512.0, 512.0], [0, 0, 1]]).cuda()
run_case("(b) pinhole 1024x1024 V=2", 2, "pinhole", (1024, 1024), k_pin)

print(json.dumps({"cube_views_bench": results}))
if a.out:
    with open(a.out, "w") as f:
        json.dump({"cube_views_bench": results}, f, indent=1)
