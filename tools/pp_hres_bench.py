#!/usr/bin/env python
"""PP high-res layer stack: msi_pp_hres_layers (one launch) against the three launches it replaces, and the direct sparse build against
dense + sparsify_layers(border='edge').  One process; per shape, after a warm-up and a bit-for-bit comparison of the outputs, the forms
ALTERNATE for --repeats rounds and the median is reported with min / max:
  (a)   msi_perspective_plane_sweep_f32 x 2 -> msi_resize_bilinear_f32 -> msi_assemble_rgba_scaled_f32   (fp32 stack),
  (a')  the same followed by msi_pack_layers (rgba8 / rgba16f),
  (b)   msi_pp_hres_layers writing the fp32 stack / the rgba8 stack / the rgba16f stack,
on preallocated buffers, then the peak allocated memory of each form when it allocates its own buffers; then, per occupancy (blocky
alphas: 16 x 16-texel low-res blocks of layers 1.. switched on at random, the generator of tools/sparse_planar_bench.py at the
low-res size),
  (c)   MSI.mpi_hres_layers(rgba8) + MSI.sparsify_layers(border='edge')      (d)   MSI.mpi_hres_layers_sparse(rgba8)
as the methods themselves (allocation and the one host synchronisation included), with their peak allocations.
Shapes: six faces of SxS from six of 256x256, D planes.  Nothing is gated on these numbers.
Kernel times and resources: run this under `rocprofv3 --kernel-trace --stats` in a run of its own (--repeats 1)."""
import argparse
import os
import sys

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import numpy as np
import torch

ap = argparse.ArgumentParser()
ap.add_argument("--repeats", type=int, default=9, help="alternated rounds; the median is reported")
ap.add_argument("--faces", default="1024,512", help="comma-separated high-res face sizes S (six faces of S x S)")
ap.add_argument("--low", type=int, default=256, help="low-res face size")
ap.add_argument("--planes", type=int, default=32)
ap.add_argument("--occupancies", default="0.2,0.5", help="kept fractions asked of the blocky alphas")
ap.add_argument("--out", default=None, help="also write the table to this text file")
a = ap.parse_args()

from matryodshka_amd import MSI, _native as N

B = 6
lines = []


def say(s=""):
    print(s, flush=True)
    lines.append(s)


def med(v):
    return float(np.median(v))


def run_shape(s, low, d):
    m = MSI(input_type='PP')
    dev, b = m.device, B
    g = torch.Generator(device="cuda").manual_seed(1)
    raw_ref, raw_src = torch.rand((b, s, s, 3), generator=g, device=dev), torch.rand((b, s, s, 3), generator=g, device=dev)
    ref, src = raw_ref * 2 - 1, raw_src * 2 - 1
    bw = torch.rand((b, low, low, d), generator=g, device=dev)
    al = torch.rand((b, low, low, d), generator=g, device=dev)
    lowt = torch.cat([bw, al], dim=-1).contiguous()
    eye = torch.eye(4, device=dev)[None].expand(b, 4, 4).contiguous()
    th = 0.03
    src_pose = eye.clone()
    src_pose[:, 0, 0] = src_pose[:, 2, 2] = float(np.cos(th))
    src_pose[:, 0, 2], src_pose[:, 2, 0] = float(np.sin(th)), -float(np.sin(th))
    src_pose[:, 0, 3] = -0.064
    intr = torch.tensor([[s / 2, 0, s / 2], [0, s / 2, s / 2], [0, 0, 1]], device=dev)[None].expand(b, 3, 3).contiguous()
    planes = m.inv_depths(1.0, 100.0, d)
    depths = m._planes(planes)
    stream = torch.cuda.current_stream().cuda_stream
    texels = b * d * s * s
    new = lambda *shape, dtype=torch.float32: torch.empty(shape, dtype=dtype, device=dev)
    code_dtype = {"rgba8": torch.uint8, "rgba16f": torch.float16}

    def old(psv, up, rgba):
        for i, (img, pose) in enumerate(((ref, eye), (src, src_pose))):
            N.check(N.lib.msi_perspective_plane_sweep_f32(img.data_ptr(), pose.data_ptr(), intr.data_ptr(), depths.data_ptr(), b, s, s, d,
                                                          psv.data_ptr(), 6 * d, i * 3 * d, stream), "sweep")
        N.check(N.lib.msi_resize_bilinear_f32(lowt.data_ptr(), up.data_ptr(), b, low, low, 2 * d, s, s, stream), "resize")
        N.check(N.lib.msi_assemble_rgba_scaled_f32(psv.data_ptr(), up.data_ptr(), rgba.data_ptr(), b, s, s, d, stream), "assemble")

    def pack(rgba, fmt, out):
        N.check(N.lib.msi_pack_layers(rgba.data_ptr(), m.LAYER_FORMATS[fmt], out.data_ptr(), texels, stream), "pack")

    def fused(rgba, codes, fmt):
        N.check(N.lib.msi_pp_hres_layers(ref.data_ptr(), src.data_ptr(), eye.data_ptr(), src_pose.data_ptr(), intr.data_ptr(), depths.data_ptr(),
                                         bw.data_ptr(), al.data_ptr(), b, low, low, s, s, d, 0 if rgba is None else rgba.data_ptr(),
                                         0 if codes is None else codes.data_ptr(), m.LAYER_FORMATS.get(fmt, 0), stream), "pp_hres_layers")

    psv, up, rgba_a, rgba_b = new(b, s, s, 6 * d), new(b, s, s, 2 * d), new(b, d, s, s, 4), new(b, d, s, s, 4)
    pk_a = {f: new(b, d, s, s, 4, dtype=t) for f, t in code_dtype.items()}
    pk_b = {f: new(b, d, s, s, 4, dtype=t) for f, t in code_dtype.items()}
    forms = {"a": lambda: old(psv, up, rgba_a),
             "a8": lambda: (old(psv, up, rgba_a), pack(rgba_a, "rgba8", pk_a["rgba8"])),
             "a16": lambda: (old(psv, up, rgba_a), pack(rgba_a, "rgba16f", pk_a["rgba16f"])),
             "b": lambda: fused(rgba_b, None, None),
             "b8": lambda: fused(None, pk_b["rgba8"], "rgba8"),
             "b16": lambda: fused(None, pk_b["rgba16f"], "rgba16f")}
    names = {"a": "(a)  2 sweeps + resize + assemble", "a8": "(a') ... + pack_layers rgba8", "a16": "(a') ... + pack_layers rgba16f",
             "b": "(b)  pp_hres_layers f32", "b8": "(b)  pp_hres_layers rgba8", "b16": "(b)  pp_hres_layers rgba16f"}
    t0, t1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)

    def timed(fn):
        t0.record()
        fn()
        t1.record()
        t1.synchronize()
        return t0.elapsed_time(t1) * 1e3          # us

    for fn in forms.values():                     # warm-up, then the outputs bit for bit
        timed(fn)
    torch.cuda.synchronize()
    assert torch.equal(rgba_a.view(torch.int32), rgba_b.view(torch.int32)), "the fp32 stacks differ"
    for f in code_dtype:
        assert torch.equal(pk_a[f].view(torch.uint8), pk_b[f].view(torch.uint8)), "the %s stacks differ" % f
    samples = {k: [] for k in forms}
    for _ in range(a.repeats):
        for k, fn in forms.items():
            samples[k].append(timed(fn))
    say("6 x %dx%dx%d from 6 x %dx%d  (outputs of (b) == outputs of (a) / (a'), bit for bit: checked)" % (s, s, d, low, low))
    for k in forms:
        say("  %-36s %9.1f us   min %.1f max %.1f  [%s]" % (names[k], med(samples[k]), min(samples[k]), max(samples[k]),
                                                            ", ".join("%.1f" % v for v in samples[k])))
    for x, y, what in (("a", "b", "(a) / (b f32)"), ("a8", "b8", "(a' rgba8) / (b rgba8)"), ("a16", "b16", "(a' rgba16f) / (b rgba16f)")):
        r = [p / q for p, q in zip(samples[x], samples[y])]
        say("  %-28s = %.3f of the medians; per round %.3f (min %.3f, max %.3f)   (> 1: the fused launch is faster)" % (
            what, med(samples[x]) / med(samples[y]), med(r), min(r), max(r)))

    # peak allocated memory of each form when it allocates what it needs itself
    del psv, up, rgba_a, rgba_b, pk_a, pk_b, forms
    alloc = {"a": lambda: old(new(b, s, s, 6 * d), new(b, s, s, 2 * d), new(b, d, s, s, 4)),
             "b": lambda: fused(new(b, d, s, s, 4), None, None),
             "b8": lambda: fused(None, new(b, d, s, s, 4, dtype=torch.uint8), "rgba8"),
             "b16": lambda: fused(None, new(b, d, s, s, 4, dtype=torch.float16), "rgba16f")}

    def a_packed(fmt):
        r = new(b, d, s, s, 4)
        old(new(b, s, s, 6 * d), new(b, s, s, 2 * d), r)
        pack(r, fmt, new(b, d, s, s, 4, dtype=code_dtype[fmt]))
    alloc["a8"], alloc["a16"] = lambda: a_packed("rgba8"), lambda: a_packed("rgba16f")

    def peak(fn):
        torch.cuda.synchronize()
        torch.cuda.empty_cache()
        torch.cuda.reset_peak_memory_stats()
        before = torch.cuda.memory_allocated()
        fn()
        torch.cuda.synchronize()
        return (torch.cuda.max_memory_allocated() - before) / 1e9
    short = {"a": "(a)", "a8": "(a' rgba8)", "a16": "(a' rgba16f)", "b": "(b f32)", "b8": "(b rgba8)", "b16": "(b rgba16f)"}
    say("  peak allocated beyond the inputs: " + ";  ".join("%s %.2f GB" % (short[k], peak(alloc[k])) for k in ("a", "a8", "a16", "b", "b8", "b16")))

    # the sparse build: the methods themselves
    args = lambda alphas: (bw, alphas, raw_ref, raw_src, eye, src_pose, planes, intr)
    blk = 16
    for occ in (float(v) for v in a.occupancies.split(",")):
        on = torch.rand((b, -(-low // blk), -(-low // blk), d), generator=g, device=dev) < occ
        on[..., 0] = True
        mask = on.repeat_interleave(blk, 1).repeat_interleave(blk, 2)[:, :low, :low].to(torch.float32)
        alm = (0.05 + 0.9 * al) * mask
        two = lambda: m.sparsify_layers(m.mpi_hres_layers(*args(alm), ref_pose_inv=eye, layer_format='rgba8')['packed_layers'], border='edge')
        one = lambda: m.mpi_hres_layers_sparse(*args(alm), ref_pose_inv=eye, layer_format='rgba8')['sparse_layers']
        sp2, sp1 = two(), one()
        torch.cuda.synchronize()
        for name in ("table", "layer_start", "pool"):
            assert torch.equal(getattr(sp1, name), getattr(sp2, name)), "the sparse stacks differ in %s" % name
        kept, nbytes = sp1.occupancy, sp1.nbytes
        del sp1, sp2
        ts = {"c": [], "d": []}
        for _ in range(a.repeats):
            for k, fn in (("c", two), ("d", one)):
                ts[k].append(timed(fn))
        r = [p / q for p, q in zip(ts["c"], ts["d"])]
        say("  blocky alphas, asked %.2f, kept fraction %.3f (sparse stack %.1f MB; table, layer_start and pool equal: checked)" % (occ, kept, nbytes / 1e6))
        say("    (c) mpi_hres_layers rgba8 + sparsify_layers(edge) %9.1f us   min %.1f max %.1f   peak %.2f GB" % (med(ts["c"]), min(ts["c"]), max(ts["c"]), peak(two)))
        say("    (d) mpi_hres_layers_sparse rgba8                  %9.1f us   min %.1f max %.1f   peak %.2f GB" % (med(ts["d"]), min(ts["d"]), max(ts["d"]), peak(one)))
        say("    (c) / (d) = %.3f of the medians; per round %.3f (min %.3f, max %.3f)   (> 1: the direct build is faster)" % (
            med(ts["c"]) / med(ts["d"]), med(r), min(r), max(r)))
    say()


say("PP high-res layer stack, one launch against three: device-event time per form, median of %d alternated rounds" % a.repeats)
say("device: %s" % torch.cuda.get_device_name(0))
say()
for s_ in a.faces.split(","):
    run_shape(int(s_), a.low, a.planes)
    torch.cuda.empty_cache()
if a.out:
    os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
    with open(a.out, "w") as f:
        f.write("\n".join(lines) + "\n")
