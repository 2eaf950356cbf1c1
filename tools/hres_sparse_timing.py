#!/usr/bin/env python
"""Sparse high-res layer stacks: MSI.hres_layers_sparse(fmt) against the only path there was before it,
MSI.hres_layers(fmt) + MSI.sparsify_layers.  The protocol of tools/hres_layers_timing.py: one process; per size, format and mask,
after a warm-up and a bit-for-bit comparison of the results (table, layer_start, pool), the two forms ALTERNATE for --repeats
rounds and the median is reported with min / max:
  (a)  hres_layers(fmt)['packed_layers'] -> sparsify_layers            (dense stack written, read back, kept tiles copied)
  (b)  hres_layers_sparse(fmt)                                        (keep pass over the alphas, scan, texels of kept tiles)
Both end to end -- wall clock from the call to a device synchronisation behind it, the host synchronisation in the middle of
each included.  Then the device-event time of each new launch on its own, on preallocated buffers (msi_hres_index_tiles: the
keep pass and the scan; msi_hres_layers_sparse: its 8-byte read-back and the texel pass), next to the dense msi_hres_layers
launch, and the peak allocation of both forms beyond their inputs.
Sizes: 4096x2048x32 and 1280x640x32, both from 640x320.  Masks: blocks of 10 x 10 low-res texels of layers 1.. switched on at
random so that the nominal occupancy is approached (layer 0 is always kept); the occupancy measured is printed."""
import argparse
import os
import sys
import time

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import numpy as np
import torch

ap = argparse.ArgumentParser()
ap.add_argument("--repeats", type=int, default=7, help="alternated rounds; the median is reported")
ap.add_argument("--shapes", default="4096x2048,1280x640", help="comma-separated high-res sizes WxH")
ap.add_argument("--formats", default="rgba8,rgba16f")
ap.add_argument("--occupancies", default="1.0,0.64,0.36,0.14")
ap.add_argument("--planes", type=int, default=32)
ap.add_argument("--out", default=None, help="also write the table to this text file")
a = ap.parse_args()

from matryodshka_amd import MSI, _native as N
from matryodshka_amd.sparse import TILE_H, TILE_W

LOW_H, LOW_W, BLOCK = 320, 640, 10
lines = []


def say(s=""):
    print(s, flush=True)
    lines.append(s)


def alphas(occupancy, d, seed):
    rng = np.random.RandomState(seed)
    p = 1.0 if occupancy >= 1.0 else max((occupancy * d - 1.0) / (d - 1.0), 0.0)        # layer 0 is kept whole
    on = rng.uniform(size=(LOW_H // BLOCK, LOW_W // BLOCK, d)) < p
    mask = np.repeat(np.repeat(on, BLOCK, axis=0), BLOCK, axis=1).astype(np.float32)
    return ((0.05 + 0.9 * rng.uniform(size=(1, LOW_H, LOW_W, d))) * mask[None]).astype(np.float32)


def med(v):
    return float(np.median(v))


def spread(v):
    return "%9.1f us  (min %.1f max %.1f)" % (med(v), min(v), max(v))


def run(m, hw, hh, d, fmt, occ, seed, inputs):
    dev, b = m.device, 1
    raw_ref, raw_src, bw, eye, intr, planes = inputs
    al = torch.from_numpy(alphas(occ, d, seed)).to(dev)
    form_a = lambda: m.sparsify_layers(m.hres_layers(bw, al, raw_ref, raw_src, eye, eye, planes, intr, layer_format=fmt)["packed_layers"])
    form_b = lambda: m.hres_layers_sparse(bw, al, raw_ref, raw_src, eye, eye, planes, intr, layer_format=fmt)["sparse_layers"]
    forms = {"a": form_a, "b": form_b}

    def wall(fn):
        torch.cuda.synchronize()
        t = time.perf_counter()
        out = fn()
        torch.cuda.synchronize()
        return (time.perf_counter() - t) * 1e6, out

    # warm-up, then the results bit for bit
    outs = {k: wall(fn)[1] for k, fn in forms.items()}
    words = lambda t: t.contiguous().view({8: torch.int64, 4: torch.int32, 2: torch.int16, 1: torch.uint8}[t.element_size()])
    for name in ("table", "layer_start", "pool"):
        assert torch.equal(words(getattr(outs["a"], name)), words(getattr(outs["b"], name))), "%s differs" % name
    measured, nbytes = outs["b"].occupancy, outs["b"].nbytes
    sp = outs["b"]
    del outs
    samples = {k: [] for k in forms}
    for _ in range(a.repeats):
        for k, fn in forms.items():
            samples[k].append(wall(fn)[0])

    # each new launch on its own, on the buffers of the result; the dense launch next to them
    stream = torch.cuda.current_stream().cuda_stream
    f = m.LAYER_FORMATS[fmt]
    ref, src = m.preprocess_image(raw_ref), m.preprocess_image(raw_src)
    depths, trig = m._planes(planes), m._trig(hh, hw)
    eye_d = torch.eye(4, device=dev)[None].contiguous()
    table, counts = torch.empty_like(sp.table), torch.empty((b * d,), dtype=torch.int32, device=dev)
    pool = torch.empty_like(sp.pool)
    t0, t1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)

    def timed(fn):
        t0.record()
        fn()
        t1.record()
        t1.synchronize()
        return t0.elapsed_time(t1) * 1e3

    index = lambda: N.check(N.lib.msi_hres_index_tiles(al.data_ptr(), f, b, LOW_H, LOW_W, hh, hw, d, table.data_ptr(), counts.data_ptr(), stream), "index")
    texels = lambda: N.check(N.lib.msi_hres_layers_sparse(ref.data_ptr(), src.data_ptr(), eye_d.data_ptr(), eye_d.data_ptr(), intr.data_ptr(),
                                                          depths.data_ptr(), trig.data_ptr(), bw.data_ptr(), al.data_ptr(), b, LOW_H, LOW_W, hh, hw, d,
                                                          sp.table.data_ptr(), sp.layer_start.data_ptr(), pool.data_ptr(), f, stream), "texels")
    dev_t = {"index": [], "texels": []}
    for k, fn in (("index", index), ("texels", texels)):
        timed(fn)
    assert torch.equal(table, sp.table) and torch.equal(words(pool), words(sp.pool))
    for _ in range(a.repeats):
        for k, fn in (("index", index), ("texels", texels)):
            dev_t[k].append(timed(fn))
    del table, counts, pool, sp
    codes = torch.empty((b, d, hh, hw, 4), dtype=torch.uint8 if fmt == "rgba8" else torch.float16, device=dev)
    dense = lambda: N.check(N.lib.msi_hres_layers(ref.data_ptr(), src.data_ptr(), eye_d.data_ptr(), eye_d.data_ptr(), intr.data_ptr(), depths.data_ptr(),
                                                  trig.data_ptr(), bw.data_ptr(), al.data_ptr(), b, LOW_H, LOW_W, hh, hw, d, 0, codes.data_ptr(), f,
                                                  stream), "dense")
    timed(dense)
    dev_t["dense"] = [timed(dense) for _ in range(a.repeats)]
    del codes

    peaks = {}
    for k, fn in forms.items():
        torch.cuda.synchronize()
        torch.cuda.empty_cache()
        torch.cuda.reset_peak_memory_stats()
        before = torch.cuda.memory_allocated()
        out = fn()
        torch.cuda.synchronize()
        peaks[k] = (torch.cuda.max_memory_allocated() - before) / 1e6
        del out
    say("  %-7s occupancy %.3f (asked %.2f), result %.1f MB" % (fmt, measured, occ, nbytes / 1e6))
    say("    (a) hres_layers + sparsify_layers   %s   peak %8.1f MB" % (spread(samples["a"]), peaks["a"]))
    say("    (b) hres_layers_sparse             %s   peak %8.1f MB   (a) / (b) = %.3f" % (spread(samples["b"]), peaks["b"],
                                                                                          med(samples["a"]) / med(samples["b"])))
    say("    device: msi_hres_index_tiles        %s" % spread(dev_t["index"]))
    say("    device: msi_hres_layers_sparse      %s" % spread(dev_t["texels"]))
    say("    device: msi_hres_layers (dense)     %s" % spread(dev_t["dense"]))
    return med(dev_t["texels"]), (min(dev_t["texels"]), max(dev_t["texels"]))


say("sparse high-res layer stacks, direct against dense + sparsify: median of %d alternated rounds; results compared bit for bit first" % a.repeats)
say("device: %s" % torch.cuda.get_device_name(0))
say()
m = MSI()
d = a.planes
for s in a.shapes.split(","):
    hw, hh = (int(v) for v in s.split("x"))
    assert hh % TILE_H == 0 and hw % TILE_W == 0
    g = torch.Generator(device="cuda").manual_seed(1)
    inputs = (torch.rand((1, hh, hw, 3), generator=g, device=m.device), torch.rand((1, hh, hw, 3), generator=g, device=m.device),
              torch.rand((1, LOW_H, LOW_W, d), generator=g, device=m.device), np.eye(4, dtype=np.float32)[None],
              torch.tensor([[[0.032, 0, 0], [0, 1, 0], [0, 0, 1]]], device=m.device), m.inv_depths(1.0, 100.0, d))
    say("%dx%dx%d from %dx%d, batch 1" % (hw, hh, d, LOW_W, LOW_H))
    for fmt in a.formats.split(","):
        for k, occ in enumerate(float(x) for x in a.occupancies.split(",")):
            run(m, hw, hh, d, fmt, occ, 100 + k, inputs)
    say()
    del inputs
    torch.cuda.empty_cache()
if a.out:
    os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
    with open(a.out, "w") as f:
        f.write("\n".join(lines) + "\n")
