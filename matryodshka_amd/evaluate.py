"""Quality metrics of the reference's eval.py on written result files (host numpy; no device work).

    python -m matryodshka_amd.evaluate --result_root results --model_names msi-hip --output_table eval.json

`--on_device` scores the same PNG pairs with MSI.score_views (msi_score_images: the fp64 device statement of the functions below)
instead; the table has the same keys.  Everything else here stays host numpy and is the metric of record the device scorer is
tested against.

eval.py:127-145 `evaluate_one`: per example directory, `tgt_image_*` (ground truth) against `output_tgt_*` (render):
  tf.image.ssim(pred, tgt, max_val=255) and tf.image.psnr(pred, tgt, max_val=255)
eval.py:147-174 `evaluate_consecutive_one`: mean absolute frame-to-frame difference of `output_tgt_*` / `output_depth_*`
of consecutive video frames (temporal consistency).  E-LPIPS (eval.py:138, the vendored elpips/ network + weights) is
out of scope: it is a training / evaluation network of its own, not part of the infer -> render path.

tf.image.ssim / psnr semantics restated here are [TF-knowledge] (TF 1.14 image_ops_impl.py): 11x11 Gaussian window,
sigma 1.5, normalised by softmax of -(x^2+y^2)/(2 sigma^2), VALID depth-wise filtering, k1 = 0.01, k2 = 0.03,
luminance = (2 mu_x mu_y + c1) / (mu_x^2 + mu_y^2 + c1), cs = (2 (E[xy] - mu_x mu_y) + c2) / (E[x^2 + y^2] - mu_x^2 - mu_y^2 + c2),
SSIM = mean over window positions per channel, then mean over channels; PSNR = 20 log10(max) - 10 log10(mean squared error).
"""
import argparse
import glob
import json
import os

import numpy as np


def _gauss_window(size=11, sigma=1.5):
    coords = np.arange(size, dtype=np.float64) - (size - 1) / 2.0
    g = -0.5 * coords * coords / (sigma * sigma)
    g2 = g[None, :] + g[:, None]
    e = np.exp(g2 - g2.max())
    return e / e.sum()          # softmax over the 121 taps


def _filter_valid(x, win):
    """VALID cross-correlation of [H,W,C] with the separable window (its rows and columns are proportional)."""
    k = win.shape[0]
    col = win.sum(axis=1)                       # 1-D factors of the (exactly separable) normalised Gaussian
    row = win.sum(axis=0)
    h, w, _ = x.shape
    tmp = np.zeros((h - k + 1, w, x.shape[2]))
    for i in range(k):
        tmp += col[i] * x[i:i + h - k + 1]
    out = np.zeros((h - k + 1, w - k + 1, x.shape[2]))
    for j in range(k):
        out += row[j] * tmp[:, j:j + w - k + 1]
    return out


def solid_angle_row_weights(h):
    """cos((i + 0.5 - h/2) pi / h), i = 0..h-1: the solid angle of a pixel of row i of an equirectangular image, up to a
    constant -- the weighting of WS-PSNR.  It is NOT the reference's create_spherical_weights, which is an attention term of
    its training loss and out of scope here."""
    return np.cos((np.arange(h, dtype=np.float64) + 0.5 - h / 2.0) * (np.pi / h))


def _row_weights(row_weights, h):
    w = np.asarray(row_weights, dtype=np.float64).reshape(-1)
    if w.shape[0] != h:
        raise ValueError("row_weights: %d weights for %d rows" % (w.shape[0], h))
    return w


def ssim(img1, img2, max_val=255.0, filter_size=11, filter_sigma=1.5, k1=0.01, k2=0.03, row_weights=None):
    """tf.image.ssim for one image pair [H,W,C] (eval.py:139).  row_weights [H] (default None: the plain mean): a row of the
    lum * cs map counts with the weight of its window's centre row,
    sum_i w[i+r] sum_{j,ch} map[i,j,ch] / (sum_i w[i+r] * (W - 2r) * C), r = filter_size // 2."""
    x = np.asarray(img1, dtype=np.float64)
    y = np.asarray(img2, dtype=np.float64)
    if x.shape != y.shape or x.ndim != 3:
        raise ValueError("ssim: images must be [H,W,C] and agree")
    if min(x.shape[0], x.shape[1]) < filter_size:
        raise ValueError("ssim: image smaller than the %dx%d window" % (filter_size, filter_size))
    win = _gauss_window(filter_size, filter_sigma)
    c1, c2 = (k1 * max_val) ** 2, (k2 * max_val) ** 2
    mx, my = _filter_valid(x, win), _filter_valid(y, win)
    num0, den0 = mx * my * 2.0, mx * mx + my * my
    lum = (num0 + c1) / (den0 + c1)
    num1 = _filter_valid(x * y, win) * 2.0
    den1 = _filter_valid(x * x + y * y, win)
    cs = (num1 - num0 + c2) / (den1 - den0 + c2)
    if row_weights is None:
        return float((lum * cs).mean(axis=(0, 1)).mean())
    r = filter_size // 2
    w = _row_weights(row_weights, x.shape[0])[r:x.shape[0] - r]
    m = lum * cs
    return float((w * m.sum(axis=(1, 2))).sum() / (w.sum() * m.shape[1] * m.shape[2]))


def _weighted_mean(v, row_weights):
    """sum_r w_r sum_{c,ch} v / (sum_r w_r * W * C) of v [H,W,C]."""
    w = _row_weights(row_weights, v.shape[0])
    return float((w * v.sum(axis=(1, 2))).sum() / (w.sum() * v.shape[1] * v.shape[2]))


def psnr(img1, img2, max_val=255.0, row_weights=None):
    """tf.image.psnr (eval.py:140); inf for identical images.  row_weights [H]: the squared error of row r counts with
    w_r (with solid_angle_row_weights: WS-PSNR)."""
    x = np.asarray(img1, dtype=np.float64)
    y = np.asarray(img2, dtype=np.float64)
    mse = float(((x - y) ** 2).mean()) if row_weights is None else _weighted_mean((x - y) ** 2, row_weights)
    if mse == 0.0:
        return float("inf")
    return float(20.0 * np.log10(max_val) - 10.0 * np.log10(mse))


def mae(img1, img2, row_weights=None):
    """Mean absolute difference of two images [H,W,C] in fp64 (eval.py:147-174 takes it of consecutive frames), optionally
    with one weight per row."""
    x = np.asarray(img1, dtype=np.float64)
    y = np.asarray(img2, dtype=np.float64)
    if x.shape != y.shape or x.ndim != 3:
        raise ValueError("mae: images must be [H,W,C] and agree")
    return float(np.abs(x - y).mean()) if row_weights is None else _weighted_mean(np.abs(x - y), row_weights)


def load_image(path):
    """eval.py load_image: the PNG as float values 0..255, [H,W,3]."""
    from PIL import Image
    return np.asarray(Image.open(path).convert("RGB"), dtype=np.float32)


def evaluate_one(result_root, model_name, example):
    """eval.py:127-145 without the E-LPIPS term: (ssim, psnr) of output_tgt_* against tgt_image_*."""
    d = os.path.join(result_root, model_name, example)
    tgts, preds = sorted(glob.glob(os.path.join(d, "tgt_image_*"))), sorted(glob.glob(os.path.join(d, "output_tgt_*")))
    if not tgts or not preds:
        raise FileNotFoundError("%s: needs tgt_image_* and output_tgt_* (run the harness with 'tgt_image' in --test_outputs)" % d)
    tgt, pred = load_image(tgts[0]), load_image(preds[0])
    return ssim(pred, tgt, 255.0), psnr(pred, tgt, 255.0)


def _pick(files):
    """eval.py:155-158: of two candidates prefer the one whose name contains 'blurred'."""
    files = sorted(files)
    if len(files) > 1 and "blurred" in files[1]:
        return files[1]
    return files[0]


def evaluate_consecutive_one(result_root, model_name, pair):
    """eval.py:147-174: mean |frame1 - frame2| of the rendered target and depth images of two consecutive frames."""
    d1, d2 = (os.path.join(result_root, model_name, e) for e in pair)
    t1, t2 = (load_image(_pick(glob.glob(os.path.join(d, "output_tgt_*")))) for d in (d1, d2))
    z1, z2 = (load_image(_pick(glob.glob(os.path.join(d, "output_depth_*")))) for d in (d1, d2))
    return float(np.abs(t1 - t2).mean()), float(np.abs(z1 - z2).mean())


def _example_dirs(result_root, model_name):
    root = os.path.join(result_root, model_name)
    return [e for e in os.listdir(root) if not e.endswith(".txt") and os.path.isdir(os.path.join(root, e))]


def collect_examples(result_root, model_names):
    """eval.py:62-78: the NON-video example directories present for every model (`step.txt` and every entry whose name
    contains 'video' are skipped; an example missing for some model is an error there: `assert not skipped`)."""
    counts = {}
    for m in model_names:
        for e in _example_dirs(result_root, m):
            if "video" in e:
                continue
            counts[e] = counts.get(e, 0) + 1
    skipped = sorted(k for k, v in counts.items() if v != len(model_names))
    if skipped:
        raise ValueError("examples missing for some model: %s" % ", ".join(skipped[:5]))
    return sorted(counts)


def collect_video_consecutive_examples(result_root, model_names, scene_names):
    """eval.py:102-126: per scene (an entry is a frame of scene s when its name contains 'video' and s), the frame
    directories present for every model sorted by name, as consecutive pairs WITHIN the scene: [scene][pair] -> (e0, e1)."""
    out = []
    for scene in scene_names:
        counts = {}
        for m in model_names:
            for e in _example_dirs(result_root, m):
                if "video" in e and scene in e:
                    counts[e] = counts.get(e, 0) + 1
        skipped = sorted(k for k, v in counts.items() if v != len(model_names))
        if skipped:
            raise ValueError("video frames missing for some model: %s" % ", ".join(skipped[:5]))
        frames = sorted(counts)
        out.append([(frames[j], frames[j + 1]) for j in range(len(frames) - 1)])
    return out


def _device_scores(result_root, models, examples, pairs):
    """--on_device: what evaluate_one / evaluate_consecutive_one return for every (model, example) and (model, frame pair),
    from MSI.score_views on the uint8 levels of the same PNG files; one read-back after the last launch."""
    import torch
    from . import MSI
    model = MSI()

    def up(path):
        return torch.from_numpy(load_image(path).astype(np.uint8)).to(model.device)

    def first(d, pattern, pick=lambda f: sorted(f)[0]):
        files = glob.glob(os.path.join(d, pattern))
        if not files:
            raise FileNotFoundError("%s: no %s (run the harness with 'tgt_image' in --test_outputs)" % (d, pattern))
        return up(pick(files))

    one, cons = [], []
    for e in examples:
        row = []
        for m in models:
            d = os.path.join(result_root, m, e)
            row.append(model.score_views(first(d, "output_tgt_*"), first(d, "tgt_image_*"), metrics=("ssim", "psnr")))
        one.append(row)
    for scene_pairs in pairs:
        rows = []
        for pr in scene_pairs:
            row = []
            for m in models:
                d1, d2 = (os.path.join(result_root, m, e) for e in pr)
                row.append([model.score_views(first(d1, pat, _pick), first(d2, pat, _pick), metrics=("mae",))["mae"]
                            for pat in ("output_tgt_*", "output_depth_*")])
            rows.append(row)
        cons.append(rows)
    ssim_t = [[float(s["ssim"]) for s in row] for row in one]
    psnr_t = [[float(s["psnr"]) for s in row] for row in one]
    cons_t = [[[[float(v) for v in md] for md in row] for row in rows] for rows in cons]
    return ssim_t, psnr_t, cons_t


def main(argv=None):
    ap = argparse.ArgumentParser(description=__doc__, formatter_class=argparse.RawDescriptionHelpFormatter)
    ap.add_argument("--result_root", default="results")
    ap.add_argument("--model_names", default="msi-hip", help="comma-separated experiment names under result_root")
    ap.add_argument("--output_table", default="eval.json")
    ap.add_argument("--video", action="store_true",
                    help="eval_type on_video (eval.py:185-215): frame-to-frame differences of the 'video' examples, per scene")
    ap.add_argument("--videos", default="room_0 room_2 office_0 apartment_0", help="scene names of the video examples (eval.py:43)")
    ap.add_argument("--on_device", action="store_true",
                    help="score the PNG pairs on the GPU (MSI.score_views on their uint8 levels) instead of in host numpy; same table")
    a = ap.parse_args(argv)
    models = [m for m in a.model_names.split(",") if m]
    examples = collect_examples(a.result_root, models)
    table = {"model_names": models, "examples": examples, "ssim": [], "psnr": []}
    scenes = [s for s in a.videos.split(" ") if s] if a.video else []
    pairs = collect_video_consecutive_examples(a.result_root, models, scenes) if a.video else []
    if a.on_device:
        table["ssim"], table["psnr"], device_diffs = _device_scores(a.result_root, models, examples, pairs)
    else:
        for e in examples:
            scores = [evaluate_one(a.result_root, m, e) for m in models]
            table["ssim"].append([s[0] for s in scores])
            table["psnr"].append([s[1] for s in scores])
    table["mean_ssim"] = [float(np.mean([r[i] for r in table["ssim"]])) for i in range(len(models))] if examples else []
    table["mean_psnr"] = [float(np.mean([r[i] for r in table["psnr"]])) for i in range(len(models))] if examples else []
    if a.video:
        table["video_scenes"] = scenes
        if a.on_device:
            table["consecutive"] = [[{"frames": list(pr), "diffs": device_diffs[i][j]} for j, pr in enumerate(scene_pairs)]
                                    for i, scene_pairs in enumerate(pairs)]
        else:
            table["consecutive"] = [[{"frames": list(pr), "diffs": [list(evaluate_consecutive_one(a.result_root, m, pr)) for m in models]}
                                     for pr in scene_pairs] for scene_pairs in pairs]
    with open(a.output_table, "w") as f:
        json.dump(table, f)
    print("Output written to %s" % a.output_table)
    return table


if __name__ == "__main__":
    main()
