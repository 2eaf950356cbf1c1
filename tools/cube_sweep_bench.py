#!/usr/bin/env python
"""Cube path, source half: sampling the source PANORAMA (src_sampling='panorama') against the face-wise path (src_sampling='face').  One process; per
shape, after a warm-up, the forms ALTERNATE for --repeats rounds and the median is reported with min / max.
  fp32 source sweep, 6 x SxS x D       (a)  msi_equirect_to_cube_f32 of the source panorama + msi_perspective_plane_sweep_f32 of its faces
                                       (a0) that sweep alone (the cut made beforehand)
                                       (b)  msi_cube_plane_sweep_f32
  bf16 network input, 6 B x SxS x D    (a)  msi_equirect_to_cube_f32 of the source panorama + msi_perspective_sweep_volume_bf16
                                       (a0) that volume alone
                                       (b)  msi_cube_sweep_volume_bf16
  (on preallocated buffers; the ref faces are cut beforehand for every form: both modes need them)
  MSI.hres_cube_layers in rgba8        'face' against 'panorama', the methods themselves (the ref cut, the preprocessing and the allocation of both
                                       modes included; 'face' also cuts the source panorama)
The panorama has the faces' angular resolution (2 S x 4 S).  The new sweep does one atan2, one asin and one sqrt per sample more than the face
sweep and saves the cut; nothing is gated on these numbers.
Kernel times and resources: run this under `rocprofv3 --kernel-trace --stats` in a run of its own (--repeats 1)."""
import argparse
import os
import sys

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import numpy as np
import torch

ap = argparse.ArgumentParser()
ap.add_argument("--repeats", type=int, default=9, help="alternated rounds; the median is reported")
ap.add_argument("--face", type=int, default=256, help="face size S of the sweeps")
ap.add_argument("--planes", type=int, default=32)
ap.add_argument("--bf16-cubes", type=int, default=11, help="cubes of the bf16 shape (11 cubes = 66 faces: the whole cubes nearest to the 64 faces of configs[4])")
ap.add_argument("--hres-faces", default="512,1024", help="comma-separated high-res face sizes of hres_cube_layers")
ap.add_argument("--out", default=None, help="also write the table to this text file")
a = ap.parse_args()

from matryodshka_amd import MSI, _native as N, cubemap

lines = []


def say(s=""):
    print(s, flush=True)
    lines.append(s)


def med(v):
    return float(np.median(v))


t0, t1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)


def timed(fn):
    t0.record()
    fn()
    t1.record()
    t1.synchronize()
    return t0.elapsed_time(t1) * 1e3          # us


def alternate(forms, names, ratios):
    for fn in forms.values():
        timed(fn)
    samples = {k: [] for k in forms}
    for _ in range(a.repeats):
        for k, fn in forms.items():
            samples[k].append(timed(fn))
    for k in forms:
        say("  %-62s %9.1f us   min %.1f max %.1f" % (names[k], med(samples[k]), min(samples[k]), max(samples[k])))
    for x, y, what in ratios:
        r = [p / q for p, q in zip(samples[x], samples[y])]
        say("  %-34s = %.3f of the medians; per round %.3f (min %.3f, max %.3f)" % (what, med(samples[x]) / med(samples[y]), med(r), min(r), max(r)))


def source_pose(dev):
    th = 0.03
    p = torch.eye(4, device=dev)
    p[0, 0] = p[2, 2] = float(np.cos(th))
    p[0, 2], p[2, 0] = float(np.sin(th)), -float(np.sin(th))
    p[0, 3] = -0.064
    return p


def run_sweeps(m, b, s, d, bf16):
    dev = m.device
    g = torch.Generator(device="cuda").manual_seed(1)
    hp, wp = 2 * s, 4 * s
    src_pano = torch.rand((b, hp, wp, 3), generator=g, device=dev) * 2 - 1
    ref_faces = torch.rand((6 * b, s, s, 3), generator=g, device=dev) * 2 - 1
    k = cubemap.default_face_intrinsics(s)
    kb = m._f32(k).reshape(1, 3, 3).expand(b, 3, 3).contiguous()
    kf = m._f32(k).reshape(1, 3, 3).expand(6 * b, 3, 3).contiguous()
    eye = torch.eye(4, device=dev)[None].expand(6 * b, 4, 4).contiguous()
    face_src = cubemap.face_poses(source_pose(dev)[None].expand(b, 4, 4)).reshape(6 * b, 4, 4).contiguous()
    depths = m._planes(m.inv_depths(1.0, 100.0, d))
    st = torch.cuda.current_stream().cuda_stream
    src_faces = torch.empty((6 * b, s, s, 3), device=dev)
    psv_a = torch.empty((6 * b, s, s, 6 * d), dtype=torch.bfloat16 if bf16 else torch.float32, device=dev)
    psv_b = torch.empty_like(psv_a)

    def cut():
        N.check(N.lib.msi_equirect_to_cube_f32(src_pano.data_ptr(), kb.data_ptr(), b, hp, wp, 3, s, src_faces.data_ptr(), st), "cut")

    if bf16:
        def face():
            N.check(N.lib.msi_perspective_sweep_volume_bf16(ref_faces.data_ptr(), src_faces.data_ptr(), eye.data_ptr(), face_src.data_ptr(), kf.data_ptr(),
                                                            depths.data_ptr(), 6 * b, s, s, d, psv_a.data_ptr(), st), "pp volume")

        def pano():
            N.check(N.lib.msi_cube_sweep_volume_bf16(ref_faces.data_ptr(), src_pano.data_ptr(), eye.data_ptr(), face_src.data_ptr(), kf.data_ptr(),
                                                     depths.data_ptr(), b, hp, wp, s, d, psv_b.data_ptr(), st), "cube volume")
        what = ("msi_perspective_sweep_volume_bf16", "msi_cube_sweep_volume_bf16")
    else:
        def face():
            N.check(N.lib.msi_perspective_plane_sweep_f32(src_faces.data_ptr(), face_src.data_ptr(), kf.data_ptr(), depths.data_ptr(), 6 * b, s, s, d,
                                                          psv_a.data_ptr(), 6 * d, 3 * d, st), "pp sweep")

        def pano():
            N.check(N.lib.msi_cube_plane_sweep_f32(src_pano.data_ptr(), face_src.data_ptr(), kf.data_ptr(), depths.data_ptr(), b, hp, wp, s, d,
                                                   psv_b.data_ptr(), 6 * d, 3 * d, st), "cube sweep")
        what = ("msi_perspective_plane_sweep_f32 (src half)", "msi_cube_plane_sweep_f32 (src half)")
    cut()
    say("%s, %d faces of %dx%dx%d, panorama %dx%d" % ("bf16 network input" if bf16 else "fp32 source sweep", 6 * b, s, s, d, hp, wp))
    alternate({"a": lambda: (cut(), face()), "a0": face, "b": pano},
              {"a": "(a)  msi_equirect_to_cube_f32 + " + what[0], "a0": "(a0) " + what[0] + " alone", "b": "(b)  " + what[1]},
              (("b", "a", "(b) / (a)"), ("b", "a0", "(b) / (a0)")))
    # where the face position is well inside the face the two forms see the same scene
    torch.cuda.synchronize()
    diff = (psv_a[:6, :, :, 3 * d:].float() - psv_b[:6, :, :, 3 * d:].float()).abs().flatten()[::7]
    say("  src halves of the first cube: median |face - panorama| %.2e, 90th percentile %.2e (white-noise panorama: they differ by the resampling of the cut, "
        "and past the borders)" % (float(diff.median()), float(diff.quantile(0.9))))
    say()


def run_hres(m, s, low, d):
    dev, b = m.device, 1
    g = torch.Generator(device="cuda").manual_seed(2)
    raw_src, raw_ref = torch.rand((b, 2 * s, 4 * s, 3), generator=g, device=dev), torch.rand((b, 2 * s, 4 * s, 3), generator=g, device=dev)
    bw, al = torch.rand((6 * b, low, low, d), generator=g, device=dev), torch.rand((6 * b, low, low, d), generator=g, device=dev)
    planes = m.inv_depths(1.0, 100.0, d)
    pose = source_pose(dev)
    form = lambda mode: (lambda: m.hres_cube_layers(bw, al, raw_src, raw_ref, pose, s, planes, layer_format='rgba8', src_sampling=mode))
    say("MSI.hres_cube_layers rgba8, 6 x %dx%dx%d from 6 x %dx%d, panoramas %dx%d" % (s, s, d, low, low, 2 * s, 4 * s))
    alternate({"a": form('face'), "b": form('panorama')},
              {"a": "(a)  src_sampling='face'", "b": "(b)  src_sampling='panorama'"}, (("b", "a", "(b) / (a)"),))
    say()


say("Cube path, source half from the panorama against the face-wise path: device-event time per form, median of %d alternated rounds" % a.repeats)
say("device: %s" % torch.cuda.get_device_name(0))
say()
model = MSI(input_type='PP')
run_sweeps(model, 1, a.face, a.planes, bf16=False)
run_sweeps(model, a.bf16_cubes, a.face, a.planes, bf16=True)
torch.cuda.empty_cache()
for s_ in a.hres_faces.split(","):
    run_hres(model, int(s_), a.face, a.planes)
    torch.cuda.empty_cache()
if a.out:
    os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
    with open(a.out, "w") as f:
        f.write("\n".join(lines) + "\n")
