#!/usr/bin/env python
"""MSI.cube_render_views(camera='ods'): what a stereo 360 frame from a cube costs.
One cube of six 256x256x32 PP face stacks (the cube camera fx = cx = 128) -> two 640x320 eye panoramas with depth, fp32 and its
rgba8 PackedLayers, filtering 'clamp' and 'seamless'.  Device events around --iters calls, one warm-up pass, the median of
--repeats windows in which the three forms ALTERNATE (one process):
  (a) one ODS pair launch (V = 2: left and right eye, baseline 0.064) with depth
  (b) the equirect V = 2 launch of the same build (the same two poses: what the per-lane origin costs)
  (c) two single-eye ODS launches (what the one launch saves)
Before anything is timed: the pair launch is checked bit for bit against the two single-eye launches, with baseline 0 against the
equirect launch, the eyes are checked to differ, and the status word is read.  All poses, positions, radii, cameras and planes are
device tensors (no host check, no sync inside a timed window).
  python tools/cube_ods_bench.py [--out results.json] > profiles/cube_ods_timing.txt"""
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

S, D, SIZE, BASELINE = 256, 32, (320, 640), 0.064
m = MSI()
planes = torch.tensor(m.inv_depths(1.0, 100.0, D), dtype=torch.float32).cuda()
gd = torch.Generator(device="cuda").manual_seed(0)
native = torch.rand((6, D, S, S, 4), generator=gd, device="cuda")
native[..., :3] = native[..., :3] * 2 - 1
cube = native.permute(0, 2, 3, 1, 4)                 # the public view of the native stack (no copy on the way in)
stacks = {"f32": cube, "rgba8": m.pack_layers(cube, "rgba8")}
k_face = torch.from_numpy(cubemap.default_face_intrinsics(S)).cuda()

# one head, turned 0.2 rad about y and a few centimetres off the centre; both eyes share it
pose1 = np.eye(4, dtype=np.float32)
c, s = np.cos(0.2), np.sin(0.2)
pose1[0, 0], pose1[0, 2], pose1[2, 0], pose1[2, 2] = c, s, -s, c
pose1[:3, 3] = (0.03, -0.02, 0.04)
pose = torch.from_numpy(np.tile(pose1, (1, 2, 1, 1))).cuda()
pos = torch.from_numpy(np.tile(np.array([0.02, 0.01, -0.03], np.float32), (1, 2, 1))).cuda()
eye = torch.tensor([[1.0, -1.0]]).cuda()
base = torch.tensor(BASELINE).cuda()


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
for fmt, layers in stacks.items():
    for filtering in ("clamp", "seamless"):
        kw = dict(planes=planes, stack_intrinsics=k_face, size=SIZE, filtering=filtering)
        pair = lambda: m.cube_render_views(layers, pose, pos, camera='ods', eye=eye, baseline=base, **kw)
        mono = lambda: m.cube_render_views(layers, pose, pos, camera='equirect', **kw)
        one = lambda v: m.cube_render_views(layers, pose[:, v:v + 1], pos[:, v:v + 1], camera='ods', eye=eye[:, v:v + 1], baseline=base, **kw)
        two = lambda: (one(0), one(1))
        got, (left, right) = pair(), two()
        assert torch.equal(got[0][:, :1], left[0]) and torch.equal(got[0][:, 1:], right[0]), "pair != two single eyes"
        assert torch.equal(got[1][:, :1], left[1]) and torch.equal(got[1][:, 1:], right[1]), "pair != two single eyes (depth)"
        zero = m.cube_render_views(layers, pose, pos, camera='ods', eye=eye, baseline=torch.tensor(0.0).cuda(), **kw)
        want = mono()
        assert torch.equal(zero[0], want[0]) and torch.equal(zero[1], want[1]), "baseline 0 != equirect"
        differ = float((got[0][:, 0] != got[0][:, 1]).any(dim=-1).float().mean())
        assert differ > 0.5, "the eyes do not differ"
        torch.cuda.synchronize()
        assert m.render_status() == 0
        del got, left, right, zero, want
        smp = measure({"pair": pair, "equirect": mono, "two": two})
        med = {k: float(np.median(x)) for k, x in smp.items()}
        spread = {k: (max(x) - min(x)) / med[k] for k, x in smp.items()}
        r = dict(format=fmt, filtering=filtering, size=list(SIZE), ods_pair_us=round(med["pair"], 2), equirect_v2_us=round(med["equirect"], 2),
                 two_single_eyes_us=round(med["two"], 2), pair_over_equirect=round(med["pair"] / med["equirect"], 3),
                 two_over_pair=round(med["two"] / med["pair"], 3), eye_pixels_differing=round(differ, 4),
                 windows_us={k: [round(x, 2) for x in v] for k, v in smp.items()})
        results.append(r)
        print("%-6s %-9s (a) ODS pair %8.1f us   (b) equirect V=2 %8.1f us   (c) two single eyes %8.1f us   a/b x%.3f   c/a x%.3f   "
              "(repeat spread a %.1f %%, b %.1f %%, c %.1f %%)" % (fmt, filtering, med["pair"], med["equirect"], med["two"], r["pair_over_equirect"],
                                                                 r["two_over_pair"], 100 * spread["pair"], 100 * spread["equirect"], 100 * spread["two"]),
              flush=True)
        for k in ("pair", "equirect", "two"):
            print("%-6s %-9s   windows %-8s [%s]" % ("", "", k, ", ".join("%.1f" % x for x in smp[k])), flush=True)

print(json.dumps({"cube_ods_bench": results}))
if a.out:
    with open(a.out, "w") as f:
        json.dump({"cube_ods_bench": results}, f, indent=1)
