#!/usr/bin/env python
"""The scorer's kernels (matryodshka_amd/csrc/score.hip) on the CPU, against evaluate.py -- evidence that needs no GPU.
The device code of the unit (everything inside its anonymous namespace: score_tiles_kernel, score_finalize_kernel, the tap
construction) is compiled unchanged as a host program: a shim turns a workgroup into real threads with a barrier, threadIdx /
blockIdx into variables, __shared__ into static storage and __shfl_down into an exchange through memory; images sit in heap blocks
of their exact size and the workspace is filled with 0xFF bytes.  With --sanitize the program is built with
-fsanitize=address,undefined (host code, a stand-alone program): an out-of-bounds index of a kernel is a report, and any output on
stderr fails the run.  It checks what tests/test_gpu_score.py checks on the device -- tile-boundary sizes, pixel ownership, images
below the window, the five staging modes with NaN / inf, row weights, grouping, a pair alone and among others, C = 2 / 4 -- with that
file's tolerances (1e-9; exact mse / mae for 8-bit levels).  No timing: a CPU run says nothing about the GPU.
  python tools/score_emulate.py [--sanitize] [--keep DIR]"""
import argparse
import os
import struct
import subprocess
import sys
import tempfile

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
import numpy as np

from matryodshka_amd import evaluate as E, isa_lint

SHIM = r'''
#include <barrier>
#include <cmath>
#include <cstdint>
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <limits>
#include <thread>
#include <vector>
#include "msi_hip.h"
#define __global__
#define __device__
#define __forceinline__ inline
#define __shared__ static
#define __launch_bounds__(x)
#define __restrict__
struct Idx { unsigned x; };
static thread_local Idx threadIdx;
static Idx blockIdx;
static std::barrier<> *g_bar;
static double g_shfl[256];
static void __syncthreads() { g_bar->arrive_and_wait(); }
static double __shfl_down(double v, int off, int) {      // called by every thread of the workgroup at once (wave_sum)
  g_shfl[threadIdx.x] = v;
  g_bar->arrive_and_wait();
  const unsigned lane = threadIdx.x & 63;
  const double r = (lane + off < 64) ? g_shfl[threadIdx.x + off] : v;
  g_bar->arrive_and_wait();
  return r;
}
using std::fabs;
using std::fma;
'''

MAIN = r'''
template <typename F> static void run_block(unsigned bid, int nthreads, F f) {
  blockIdx.x = bid;
  std::barrier<> bar(nthreads);
  g_bar = &bar;
  std::vector<std::thread> ts;
  for (int t = 0; t < nthreads; ++t) ts.emplace_back([=] { threadIdx.x = t; f(); });
  for (auto &t : ts) t.join();
}
int main(int, char **argv) {
  FILE *f = fopen(argv[1], "rb");
  int32_t hd[9];
  if (!f || fread(hd, 4, 9, f) != 9) return 2;
  const int n = hd[0], group = hd[1], H = hd[2], W = hd[3], C = hd[4], dtype = hd[5], mode = hd[6], hasw = hd[7];
  const unsigned metrics = hd[8];
  const size_t img = (size_t)H * W * C, esz = dtype ? 1 : 4;
  char *pred = (char *)malloc(n * img * esz), *tgt = (char *)malloc((n / group) * img * esz);
  if (fread(pred, esz, n * img, f) != n * img || fread(tgt, esz, (n / group) * img, f) != (n / group) * img) return 2;
  double *wts = nullptr;
  if (hasw) { wts = (double *)malloc(H * 8); if (fread(wts, 8, H, f) != (size_t)H) return 2; }
  const int ty = tiles_along(H, kTileH), tx = tiles_along(W, kTileW);
  const size_t tiles = (size_t)ty * tx;
  if (msi_score_workspace_bytes(n, H, W, C) != n * tiles * kRecord * 8) return 3;
  double *rec = (double *)malloc(n * tiles * kRecord * 8);
  memset(rec, 0xFF, n * tiles * kRecord * 8);
  double *out = (double *)malloc(n * 4 * 8);
  ScoreTaps taps;
  build_taps(&taps);
  const double c1 = (0.01 * 255.0) * (0.01 * 255.0), c2 = (0.03 * 255.0) * (0.03 * 255.0);
  const int do_ssim = (metrics & MSI_SCORE_SSIM) ? 1 : 0;
  for (unsigned b = 0; b < n * tiles; ++b) {
    if (dtype) run_block(b, kThreads, [&] { score_tiles_kernel<uint8_t>((const uint8_t *)pred, (const uint8_t *)tgt, mode, group, H, W, C, tx, ty, wts, do_ssim, c1, c2, taps, rec); });
    else run_block(b, kThreads, [&] { score_tiles_kernel<float>((const float *)pred, (const float *)tgt, mode, group, H, W, C, tx, ty, wts, do_ssim, c1, c2, taps, rec); });
  }
  for (int p = 0; p < n; ++p) run_block(p, 64, [&] { score_finalize_kernel(rec, (int)tiles, H, W, C, wts, 255.0, metrics, out); });
  for (int i = 0; i < n * 4; ++i) printf("%a\n", out[i]);
  for (int i = 0; i < kTaps; ++i) printf("%a %a\n", taps.col[i], taps.row[i]);
  free(pred); free(tgt); free(rec); free(out); free(wts);
  return 0;
}
'''


def build(workdir, sanitize):
    src = open(os.path.join(ROOT, "matryodshka_amd", "csrc", "score.hip")).read()
    body = src[src.index("namespace {"):src.index("}  // namespace") + len("}  // namespace")]
    # the workspace query is host code outside the namespace: take it along so that the program sizes its workspace by it
    query = src[src.index("size_t msi_score_workspace_bytes"):src.index("int msi_score_images")]
    query = query.replace("msi::fail(MSI_E_BADARG,", "fprintf(stderr,")
    with open(os.path.join(workdir, "emul.cpp"), "w") as f:
        f.write(SHIM + body + "\n" + query + MAIN)
    cxx = os.environ.get("CXX") or os.path.join(os.path.dirname(isa_lint._find_objdump()), "clang++")
    cmd = [cxx, "-std=c++20", "-O1", "-g", "-ffp-contract=off", "-pthread", "-I" + os.path.join(ROOT, "include"),
           os.path.join(workdir, "emul.cpp"), "-o", os.path.join(workdir, "emul")]
    if sanitize:
        cmd.insert(1, "-fsanitize=address,undefined")
    subprocess.check_call(cmd)
    return os.path.join(workdir, "emul")


def run(exe, workdir, pred, tgt, group=1, mode=0, weights=None, metrics=7):
    """-> ([n,4] mse, mae, ssim, psnr; [11,2] the tap factors).  mode: 0 raw, 1 image, 2 depth, 3 image quantised, 4 depth quantised."""
    n, (h, w, c) = pred.shape[0], pred.shape[1:]
    case = os.path.join(workdir, "case.bin")
    with open(case, "wb") as f:
        f.write(struct.pack("9i", n, group, h, w, c, int(pred.dtype == np.uint8), mode, int(weights is not None), metrics))
        f.write(np.ascontiguousarray(pred).tobytes())
        f.write(np.ascontiguousarray(tgt).tobytes())
        if weights is not None:
            f.write(np.asarray(weights, np.float64).tobytes())
    r = subprocess.run([exe, case], stdout=subprocess.PIPE, stderr=subprocess.PIPE, universal_newlines=True)
    if r.returncode != 0 or r.stderr.strip():
        raise RuntimeError("emulation failed (rc %d):\n%s" % (r.returncode, r.stderr[-4000:]))
    lines = r.stdout.split("\n")
    out = np.array([float.fromhex(x) for x in lines[:n * 4]]).reshape(n, 4)
    taps = np.array([[float.fromhex(v) for v in l.split()] for l in lines[n * 4:n * 4 + 11]])
    return out, taps


def pattern(rng, h, w, c):
    yy, xx = np.mgrid[0:h, 0:w]
    base = 127.5 + 70.0 * np.sin(xx / 3.0 + 0.3)[:, :, None] * np.cos(yy / 4.0)[:, :, None] + np.arange(c)[None, None, :] * 9.0
    a = np.clip(base + rng.normal(0, 25.0, (h, w, c)), 0, 255).astype(np.uint8)
    return a, np.clip(a.astype(np.float64) + rng.normal(0, 25.0, (h, w, c)), 0, 255).astype(np.uint8)


def level(x, depth):
    """deprocess_kernel in numpy fp32."""
    x = x.astype(np.float32)
    if not depth:
        x = (x + np.float32(1)) / np.float32(2)
    with np.errstate(invalid="ignore"):
        y = np.trunc(x * np.float32(255.5))
        y = np.where(np.isnan(y), 0, np.clip(y, 0, 255))
    return y.astype(np.uint8)


WORST = [0.0]


def check(out, hp, ht, exact, weights=None, ssim=True, what=""):
    x, y = np.asarray(hp, np.float64), np.asarray(ht, np.float64)
    want = {"mse": float(((x - y) ** 2).mean()) if weights is None else E._weighted_mean((x - y) ** 2, weights),
            "mae": E.mae(x, y, row_weights=weights), "psnr": E.psnr(x, y, 255.0, row_weights=weights)}
    if ssim:
        want["ssim"] = E.ssim(x, y, 255.0, row_weights=weights)
    got = dict(zip(("mse", "mae", "ssim", "psnr"), out))
    for k, v in want.items():
        if k in ("mse", "mae") and exact or np.isinf(v):
            assert got[k] == v, (what, k, got[k], v)
        else:
            assert abs(got[k] - v) <= 1e-9, (what, k, got[k], v)
            WORST[0] = max(WORST[0], abs(got[k] - v))


def main():
    ap = argparse.ArgumentParser(description=__doc__, formatter_class=argparse.RawDescriptionHelpFormatter)
    ap.add_argument("--sanitize", action="store_true", help="build the host program with -fsanitize=address,undefined")
    ap.add_argument("--keep", default=None, help="build and run in this directory and keep it")
    a = ap.parse_args()
    workdir = a.keep or tempfile.mkdtemp(prefix="score_emul_")
    os.makedirs(workdir, exist_ok=True)
    exe = build(workdir, a.sanitize)
    go = lambda *args, **kw: run(exe, workdir, *args, **kw)
    rng = np.random.RandomState(5)
    out, taps = go(*[np.zeros((1, 11, 11, 1), np.uint8)] * 2)
    win = E._gauss_window()
    assert np.abs(taps[:, 0] - win.sum(axis=1)).max() <= 1e-15 and np.abs(taps[:, 1] - win.sum(axis=0)).max() <= 1e-15
    assert out[0, 0] == 0 and out[0, 1] == 0 and out[0, 2] == 1.0 and np.isinf(out[0, 3])
    for h, w in [(12, w) for w in (11, 12, 41, 42, 43, 44, 74, 75, 76)] + [(h, 23) for h in (11, 12, 26, 27, 28, 42, 43, 44)]:
        p, t = pattern(rng, h, w, 1)
        check(go(p[None], t[None])[0][0], p, t, True, what="%dx%d" % (h, w))
    for h, w in [(11, 11), (27, 43), (37, 45), (64, 80)]:
        t = rng.randint(0, 255, size=(h, w, 3)).astype(np.uint8)
        o = go(t[None] + 1, t[None])[0][0]
        assert o[0] == 1.0 and o[1] == 1.0, (h, w, o)
    for h, w in [(1, 1), (3, 10), (10, 200)]:
        p, t = pattern(rng, h, w, 3)
        check(go(p[None], t[None], metrics=3)[0][0], p, t, True, ssim=False, what="below the window")
    x = rng.uniform(-1.3, 1.3, size=(37, 45, 3)).astype(np.float32)
    y = (x + rng.normal(0, 0.05, x.shape)).astype(np.float32)
    check(go(x[None], y[None], mode=0)[0][0], x, y, False, what="raw")
    check(go(x[None], y[None], mode=1)[0][0], (x.astype(np.float64) + 1) / 2 * 255, (y.astype(np.float64) + 1) / 2 * 255, False, what="image")
    check(go(x[None], y[None], mode=2)[0][0], x.astype(np.float64) * 255, y.astype(np.float64) * 255, False, what="depth")
    x[3, 4, 1], y[20, 44, 2], x[36, 0, 0] = np.nan, np.nan, np.inf
    check(go(x[None], y[None], mode=3)[0][0], level(x, False), level(y, False), True, what="image quantised")
    check(go(x[None], y[None], mode=4)[0][0], level(x, True), level(y, True), True, what="depth quantised")
    p, t = pattern(rng, 40, 64, 3)
    for wts in (E.solid_angle_row_weights(40), rng.uniform(0.1, 3.0, 40)):
        check(go(p[None], t[None], weights=wts)[0][0], p, t, False, weights=wts, what="row weights")
    t = rng.randint(0, 256, size=(3, 24, 31, 3)).astype(np.uint8)
    p = np.clip(t[:, None].astype(int) + rng.randint(-9, 10, size=(3, 5, 24, 31, 3)), 0, 255).astype(np.uint8).reshape(15, 24, 31, 3)
    many = go(p, t, group=5)[0]
    for k in range(15):
        check(many[k], p[k], t[k // 5], True, what="group")
    for k in (0, 7, 14):
        alone = go(p[k:k + 1], t[k // 5:k // 5 + 1])[0][0]
        assert np.array_equal(alone.view(np.int64), many[k].view(np.int64)), k
    for c in (4, 2):
        p, t = pattern(rng, 13, 17, c)
        check(go(p[None], t[None])[0][0], p, t, True, what="C = %d" % c)
    o = go(p[None], t[None], metrics=2)[0][0]
    assert np.isnan(o[[0, 2, 3]]).all() and np.isfinite(o[1])
    print("score_emulate: every case agrees with evaluate.py%s; worst |kernel - host| = %.3g" % (
        " under -fsanitize=address,undefined" if a.sanitize else "", WORST[0]))


if __name__ == "__main__":
    main()
