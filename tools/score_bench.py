#!/usr/bin/env python
"""MSI.score_views timing against the host path it replaces, in one process.  Cases (pairs x H x W x C):
  (a) 8 pairs at 320 x 640 x 3      (the frames of the test set)
  (b) 1 pair at 2048 x 4096 x 3     (one high-res frame)
  (c) 64 pairs at 1024 x 1024 x 3
each for {psnr only, psnr + ssim} and for fp32 renders scored at their 8-bit level (transform='image', quantize=True) and uint8 images.
Device: device events around --iters score_views calls after a warm-up call of the same shape, the median of --repeats windows
(no synchronisation inside a window; the workspace allocation of every call is inside it).
Host: what the parent commit offers for the same numbers on the same box -- deprocess_image on the device for fp32 renders, the
device -> host copy, then evaluate.psnr / evaluate.ssim per pair on min(16, pairs) host threads -- on a host clock that starts before
the copy and ends when the last pair is scored; run --host-repeats times (default once: case (b) alone takes seconds).
Before anything is timed the device numbers are checked against the host numbers (1e-9; uint8 / quantised mse exactly).
Per case: us per call, pairs/s, the byte floor (both images read once at 8 TB/s) as a share of the measured time -- a floor, not a
roofline: the kernel is fp64 VALU work -- and host time / device time.  Kernel times: run under `rocprofv3 --kernel-trace --stats`
in a run of its own (--repeats 1 --skip-host)."""
import argparse
import json
import os
import sys
import time
from concurrent.futures import ThreadPoolExecutor

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import numpy as np
import torch

ap = argparse.ArgumentParser()
ap.add_argument("--iters", type=int, default=10, help="calls per timed window")
ap.add_argument("--repeats", type=int, default=5, help="timed windows; the median is reported")
ap.add_argument("--host-repeats", type=int, default=1)
ap.add_argument("--host-threads", type=int, default=16)
ap.add_argument("--skip-host", action="store_true", help="device timings only (profiling runs)")
ap.add_argument("--cases", default="a,b,c")
ap.add_argument("--out", default=None, help="write the results as JSON here")
a = ap.parse_args()

from matryodshka_amd import MSI, evaluate as E

HBM = 8e12
CASES = {"a": (8, 320, 640, 3), "b": (1, 2048, 4096, 3), "c": (64, 1024, 1024, 3)}
m = MSI()
gd = torch.Generator(device="cuda").manual_seed(0)
results = []


def images(n, h, w, c, kind):
    """A smooth pattern + noise and a noisy copy (SSIM mid-range), as fp32 in [-1,1] or as uint8 levels."""
    yy = torch.arange(h, device="cuda", dtype=torch.float32)[:, None, None]
    xx = torch.arange(w, device="cuda", dtype=torch.float32)[None, :, None]
    base = 0.6 * torch.sin(xx / 9.0) * torch.cos(yy / 7.0)
    tgt = (base[None] + 0.2 * torch.randn((n, h, w, c), generator=gd, device="cuda")).clamp(-1, 1)
    pred = (tgt + 0.1 * torch.randn((n, h, w, c), generator=gd, device="cuda")).clamp(-1, 1)
    if kind == "u8":
        return m.deprocess_image(pred), m.deprocess_image(tgt)
    return pred, tgt


def device_window(fn):
    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    e0.record()
    for _ in range(a.iters):
        fn()
    e1.record()
    e1.synchronize()
    return e0.elapsed_time(e1) * 1e3 / a.iters       # us per call


def host_path(pred, tgt, with_ssim):
    """-> (seconds, [(mse-free) psnr, ssim or None per pair])"""
    torch.cuda.synchronize()
    t0 = time.perf_counter()
    if pred.dtype != torch.uint8:
        pred, tgt = m.deprocess_image(pred), m.deprocess_image(tgt)
    p, t = pred.cpu().numpy(), tgt.cpu().numpy()

    def one(i):
        return E.psnr(p[i], t[i], 255.0), (E.ssim(p[i], t[i], 255.0) if with_ssim else None)

    with ThreadPoolExecutor(max_workers=max(1, min(a.host_threads, 16, p.shape[0]))) as pool:
        scores = list(pool.map(one, range(p.shape[0])))
    return time.perf_counter() - t0, scores


for name in [c for c in a.cases.split(",") if c]:
    n, h, w, c = CASES[name]
    for kind in ("f32", "u8"):
        pred, tgt = images(n, h, w, c, kind)
        for metrics in (("psnr",), ("psnr", "ssim")):
            with_ssim = "ssim" in metrics
            call = lambda: m.score_views(pred, tgt, metrics=metrics, transform="image", quantize=True)
            got = {k: v.cpu().numpy() for k, v in call().items()}          # (also the warm-up of this shape)
            label = "(%s) %d x %dx%dx%d %s %s" % (name, n, h, w, c, kind, "+".join(metrics))
            host_s = None
            if not a.skip_host:
                times = []
                for _ in range(a.host_repeats):
                    s, scores = host_path(pred, tgt, with_ssim)
                    times.append(s)
                host_s = float(np.median(times))
                for i, (ps, ss) in enumerate(scores):
                    assert abs(got["psnr"][i] - ps) <= 1e-9, (label, i, got["psnr"][i], ps)
                    assert not with_ssim or abs(got["ssim"][i] - ss) <= 1e-9, (label, i, got["ssim"][i], ss)
            samples = [device_window(call) for _ in range(a.repeats)]
            us = float(np.median(samples))
            floor_us = 2.0 * n * h * w * c * pred.element_size() / HBM * 1e6
            r = dict(case=label, us_per_call=round(us, 2), pairs_per_s=round(n / us * 1e6, 1), byte_floor_us=round(floor_us, 2),
                     byte_floor_share_of_8TBps=round(floor_us / us, 4), samples_us=[round(x, 2) for x in samples])
            if host_s is not None:
                r.update(host_s=round(host_s, 4), host_over_device=round(host_s * 1e6 / us, 1))
            results.append(r)
            print("%-44s %10.1f us/call %10.0f pairs/s  byte floor %.1f us = %.3f of it%s" % (
                label, us, r["pairs_per_s"], floor_us, floor_us / us,
                "" if host_s is None else "   host path %.3f s = %.0f x" % (host_s, host_s * 1e6 / us)), flush=True)
        del pred, tgt
        torch.cuda.empty_cache()

print(json.dumps({"score_bench": results}))
if a.out:
    with open(a.out, "w") as f:
        json.dump({"score_bench": results}, f, indent=1)
