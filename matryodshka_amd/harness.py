"""test.py-equivalent inference harness (reference test.py:87-281) on the MI355X path.

    python -m matryodshka_amd.harness --cameras_glob 'glob/test/ods/*.txt' --image_dir glob/test_640x320 \
        --weights weights.npz --output_root results --experiment_name ods-wotemp-elpips-coord

Reads the reference's camera files (one sample per line: `scene_id id_ref id_src id_tgt baseline tx
ty tz`, datasets.py:413-425), loads `<image_dir>/<scene>_pos<id>.jpeg` (datasets.py:539), area-resizes
to --height x --width (datasets.py:513-515), runs infer_msi + the equirect RGB / depth render
(test.py:137-159) and writes the reference's output files (test.py:209-281):
  <output_root>/<experiment>/<scene>_<ref><src><tgt>/{tgt_image,output_tgt,output_depth}_<dir>.png,
  src_image/ref_image, psv_plane_%.3d.png, blend_weights.npy, blend_weight_%.3d.png, alphas.npy,
  msi_alpha_%.2d.png, msi_rgb_%.2d.png, and <output_root>/<experiment>/step.txt.
Modes (test.py:76-78): `--test_type` concatenates on_video (directory names `video_[<prefix>_]<scene>_...`, :209-217),
high_res (after the low-res pass, the high-res re-render of :283-394 from the saved blend_weights.npy / alphas.npy and
`--hres_image_dir`: output_hrestgt_* / output_hresdepth_*), high_res_only (only that); `--input_type PP` takes perspective
camera lines (`scene ref src tgt input_offset tgt_offset`, datasets.py:427-437) through the plane-sweep / mpi_render_view path;
`--dtype bf16` runs either input type on the bf16 network tier.
`--msi_format rgba8|rgba16f` also keeps each sample's MSI as a compact stack: the inference launch that writes the fp32 layers
emits the packed ones as well, saved with their planes as `msi_<dir>.npz` (PackedLayers.save) -- the stored-frame feed of
MSI.render_views; in the high_res modes the high-res stack is kept the same way, as `msi_hres_<dir>.npz` (MSI.hres_layers).
`--msi_sparse` (with --msi_format, ODS inputs) saves `msi_<dir>.npz` as a SparseLayers instead (MSI.sparsify_layers of the packed stack:
only the 4 x 16 tiles a sphere render can see; SparseLayers.load reads it, MSI.render_views renders from it with the dense
render's pixels), prints each sample's occupancy and bytes and writes them to <output_root>/<experiment>/sparse.json -- how sparse
the stacks of real content are is read off here.  The high-res stack of `--test_type high_res` (`msi_hres_<dir>.npz`) is not sparsified.
`--msi_pp_sparse` (with --msi_format and --input_type PP; --height % 4 == 0, --width % 16 == 0) is its counterpart for planar stacks: `msi_<dir>.npz`
is an edge-rule SparseLayers (MSI.sparsify_layers(border='edge'): the tiles a render that never reads the opposite border can see), which
MSI.mpi_render_views renders with the dense render's pixels; occupancies and bytes go to <experiment>/pp_sparse.json, with sparse.json's keys.
`--msi_hres_sparse` (with --msi_format and a high_res mode; --hres_height % 4 == 0, --hres_width % 16 == 0) saves `msi_hres_<dir>.npz` as a
SparseLayers built directly (MSI.hres_layers_sparse: the kept tiles follow from the low-res alphas, only their texels are computed
and the dense high-res stack is never allocated) and writes each sample's occupancy and bytes to <experiment>/hres_sparse.json; the
images are the bytes of a run without the flag.
`--hres_factored` (a high_res mode; not with --msi_format / --msi_hres_sparse) builds no high-res stack: the high-res pass renders the target view
and depth straight from the stack's factors (MSI.hres_factors -> MSI.render_views) and saves them as `msi_hres_factors_<dir>.npz`
(FactoredLayers.save); the images are the bytes of a run without the flag.
`--checkpoint` reads a TF V2 checkpoint directly (tf_checkpoint.py), `--weights` an .npz of the TF variables
(see nets.variable_shapes); without either Xavier-initialised
weights are used (there is no network access for the pretrained checkpoint), step.txt then says 0.
`--score` also scores every sample that renders output_tgt against its tgt_image on the device (MSI.score_views on the 8-bit
levels the PNG files hold) and writes <output_root>/<experiment>/scores.json: example names, ssim and psnr per example, their means,
and with on_video the mean absolute difference of consecutive output_tgt / output_depth frames per scene -- the numbers of
matryodshka_amd.evaluate without reading the files back.
`--recon_score` (with --score, ODS inputs) also renders each sample's two INPUT eyes back from its MSI -- one MSI.render_ods_pair
launch at the sample's own baseline, identity pose -- writes them as recon_ref_<dir>.png / recon_src_<dir>.png (upright, unlike
the reference-compatible output_ref / output_src) and scores them against ref_image / src_image the same way: scores.json gains
recon_ref_ssim, recon_ref_psnr, recon_src_ssim, recon_src_psnr and their mean_recon_* means.
Host I/O only: all arithmetic is in libmsi_hip.so.
"""
import argparse
import glob
import json
import os

import numpy as np


def write_image(filename, image):
    """utils.write_image (utils.py:76-81): clip to [0,255], uint8, PNG."""
    from PIL import Image
    arr = np.clip(np.asarray(image), 0, 255).astype("uint8")
    if arr.ndim == 3 and arr.shape[2] == 1:
        arr = arr[:, :, 0]
    Image.fromarray(arr).save(filename)


def resize_area(img, height, width):
    """tf.image.resize_area on a float image [H,W,3]: exact box mean for integer factors (the
    Replica test set is rendered at a multiple of 640x320), PIL box filter otherwise."""
    h, w, c = img.shape
    if h == height and w == width:
        return img.astype(np.float32)
    if h % height == 0 and w % width == 0:
        fy, fx = h // height, w // width
        return img.reshape(height, fy, width, fx, c).mean(axis=(1, 3)).astype(np.float32)
    from PIL import Image
    chans = [np.asarray(Image.fromarray(img[..., k].astype(np.float32), mode="F").resize((width, height), Image.BOX))
             for k in range(c)]
    return np.stack(chans, axis=-1).astype(np.float32)


def load_image(path, height, width):
    from PIL import Image
    img = np.asarray(Image.open(path).convert("RGB"), dtype=np.float32) * np.float32(1.0 / 255.0)
    return resize_area(img, height, width)


def parse_camera_files(pattern, input_type="ODS"):
    """Yields (scene_id, (id_ref, id_src, id_tgt), camera) per non-empty line: camera = [baseline, tx, ty, tz] for ODS
    lines (datasets.py:413-425) or [input_offset, tgt_offset] for perspective ones (datasets.py:427-437)."""
    nf = 8 if input_type == "ODS" else 6
    for path in sorted(glob.glob(pattern)):
        with open(path) as f:
            for line in f.read().split("\n"):
                parts = line.split(" ")
                if len(parts) < nf:
                    continue
                yield parts[0], tuple(parts[1:4]), [float(x) for x in parts[4:nf]]


def write_layer_outputs(outs, jouts, src, ref, num_planes, test_outputs, output_dir, dirname, which_color_pred):
    """The input images and per-layer files of test.py:246-281 (shared by the ODS and PP paths)."""
    if "src_image" in test_outputs:
        write_image(os.path.join(output_dir, "src_image_%s.png" % dirname), src[0].numpy() * 255.0)
    if "ref_image" in test_outputs:
        write_image(os.path.join(output_dir, "ref_image_%s.png" % dirname), ref[0].numpy() * 255.0)
    if "psv" in test_outputs:
        psv = outs["psv"].float().cpu().numpy()       # (a bf16 volume: numpy has no bfloat16)
        for j in range(num_planes):
            write_image(os.path.join(output_dir, "psv_plane_%.3d.png" % j), (psv[0, :, :, j * 3:(j + 1) * 3] + 1.) / 2. * 255)
    if "blend" in which_color_pred and "blend_weights" in test_outputs:      # test.py:262
        bw = outs["blend_weights"].cpu().numpy()
        np.save(os.path.join(output_dir, "blend_weights.npy"), bw)
        for i in range(num_planes):
            write_image(os.path.join(output_dir, "blend_weight_%.3d.png" % i), bw[0, :, :, i] * 255.0)
    if "alphas" in test_outputs:
        np.save(os.path.join(output_dir, "alphas.npy"), outs["alphas"].cpu().numpy())
    if "rgba_layers" in test_outputs:
        rgba = outs["rgba_layers"].cpu().numpy()
        for i in range(num_planes):
            write_image(os.path.join(output_dir, "msi_alpha_%.2d.png" % i), rgba[0, :, :, i, 3] * 255.0)
            write_image(os.path.join(output_dir, "msi_rgb_%.2d.png" % i), (rgba[0, :, :, i, :3] + 1.) / 2. * 255)
        if jouts is not None:        # test.py:276-280
            jr = jouts["rgba_layers"].cpu().numpy()
            for i in range(num_planes):
                write_image(os.path.join(output_dir, "jitter_msi_alpha_%.2d.png" % i), jr[0, :, :, i, 3] * 255.0)
                write_image(os.path.join(output_dir, "jitter_msi_rgb_%.2d.png" % i), (jr[0, :, :, i, :3] + 1.) / 2. * 255)


def save_packed_msi(outs, output_dir, dirname, model=None, sparse_log=None, border='wrap'):
    """--msi_format: the sample's packed stack (with its planes) as msi_<dirname>.npz next to its other files.  sparse_log (--msi_sparse, or
    --msi_pp_sparse with border='edge'; a list, needs model): the file is the stack's SparseLayers instead, made with the keep rule `border`, and
    the sample's occupancy and bytes are appended to the list."""
    if "packed_layers" not in outs:
        return
    packed = outs["packed_layers"]
    if sparse_log is None:
        packed.save(os.path.join(output_dir, "msi_%s.npz" % dirname))
        return
    sparse = model.sparsify_layers(packed, border=border)
    sparse.save(os.path.join(output_dir, "msi_%s.npz" % dirname))
    entry = dict(name=dirname, occupancy=sparse.occupancy, nbytes=sparse.nbytes, dense_nbytes=packed.nbytes)
    sparse_log.append(entry)
    print("Sparse MSI of %s: occupancy %.4f, %d bytes (dense %s: %d bytes)" % (dirname, entry["occupancy"], entry["nbytes"], packed.format,
                                                                              entry["dense_nbytes"]))


class DeviceScores(object):
    """--score: SSIM / PSNR of each sample's output_tgt against its tgt_image, and for video runs the frame-to-frame differences
    of output_tgt / output_depth per scene, from MSI.score_views on the uint8 levels write_image stores (so they are
    evaluate.evaluate_one / evaluate_consecutive_one of the written files).  Nothing is read back before table()."""

    def __init__(self, model, keep_frames=False):
        self.model, self.keep_frames = model, keep_frames
        self.names, self.scores, self.frames = [], [], {}
        self.recon = None       # --recon_score: {"ref": [score dicts], "src": [...]}, one entry per scored sample

    def add(self, dirname, scene, tgt_image, output_tgt, output_depth=None):
        """tgt_image: the float image handed to write_image; output_tgt / output_depth: the uint8 device images written."""
        import torch
        tgt = torch.from_numpy(np.clip(np.asarray(tgt_image), 0, 255).astype("uint8")).to(self.model.device)
        self.names.append(dirname)
        self.scores.append(self.model.score_views(output_tgt, tgt, metrics=("ssim", "psnr")))
        if self.keep_frames:
            self.frames.setdefault(scene, []).append((dirname, output_tgt, output_depth))

    def add_recon(self, ref_image, src_image, recon_ref, recon_src):
        """--recon_score: the float input images handed to write_image and the uint8 device images of the two eyes rendered back."""
        import torch
        if self.recon is None:
            self.recon = {"ref": [], "src": []}
        for key, image, recon in (("ref", ref_image, recon_ref), ("src", src_image, recon_src)):
            tgt = torch.from_numpy(np.clip(np.asarray(image), 0, 255).astype("uint8")).to(self.model.device)
            self.recon[key].append(self.model.score_views(recon, tgt, metrics=("ssim", "psnr")))

    def table(self):
        import torch
        ssim, psnr = ([float(s[k]) for s in self.scores] for k in ("ssim", "psnr"))
        table = {"examples": self.names, "ssim": ssim, "psnr": psnr,
                 "mean_ssim": float(np.mean(ssim)) if ssim else None, "mean_psnr": float(np.mean(psnr)) if psnr else None}
        if self.recon is not None:
            for eye in ("ref", "src"):
                for k in ("ssim", "psnr"):
                    vals = [float(s[k]) for s in self.recon[eye]]
                    table["recon_%s_%s" % (eye, k)] = vals
                    table["mean_recon_%s_%s" % (eye, k)] = float(np.mean(vals)) if vals else None
        if self.keep_frames:
            table["consecutive"] = []
            for scene in sorted(self.frames):
                frames = sorted(self.frames[scene], key=lambda f: f[0])
                entry = {"scene": scene, "frames": [f[0] for f in frames], "output_tgt": [], "output_depth": []}
                for key, col in (("output_tgt", 1), ("output_depth", 2)):
                    if len(frames) > 1 and all(f[col] is not None for f in frames):
                        stack = torch.stack([f[col].reshape(f[col].shape[0], f[col].shape[1], -1) for f in frames])
                        entry[key] = [float(v) for v in self.model.score_consecutive(stack).cpu()]
                table["consecutive"].append(entry)
        return table


def run_sample(model, images, baseline, tgt_pos, planes, num_planes, ngf, test_outputs, output_dir, dirname,
               which_color_pred="blend_psv", jitter_pose=None, msi_format=None, scorer=None, scene=None, recon=False, sparse_log=None):
    """One iteration of the loop at test.py:199-281.  images = (ref, src, tgt) float [H,W,3] in [0,1]
    (image order ref, src, tgt: data_loader.py:134-136).  msi_format ('rgba8' | 'rgba16f'): the sample's inference also
    emits the packed stack, saved as msi_<dirname>.npz; every other output is unchanged.  recon (--recon_score; needs scorer):
    both input eyes rendered back from the MSI in one launch, written as recon_ref_* / recon_src_* and scored.  sparse_log (--msi_sparse):
    see save_packed_msi."""
    import torch
    ref, src, tgt = (torch.from_numpy(np.ascontiguousarray(x[None])) for x in images)
    eye = np.eye(4, dtype=np.float32)[None]
    intr = np.array([[[baseline, 0, 0], [0, 1, 0], [0, 0, 1]]], dtype=np.float32)       # data_loader.py:160
    pos = np.asarray(tgt_pos, dtype=np.float32)[None]
    layer_format = "f32" if msi_format is None else ("f32", msi_format)
    outs, net_input = model.infer_msi(src, ref, None, None, eye, eye, intr, which_color_pred, num_planes, planes,
                                      extra_outputs="blend_weights alphas psv", ngf=ngf, layer_format=layer_format)
    # (after EVERY forward: the status word is reset by the next one -- ADVICE r03.  A flagged forward does not stop the sample: its
    # files are written first and the error is raised at the end, so that main()'s "flag and continue" finds them on disk -- ADVICE r04)
    from ._native import MsiError
    deferred = []
    def check_status():
        try:
            model.network_status()
        except MsiError as e:
            deferred.append(e)
    check_status()
    # Calibration state is per packed blob (one per resolution / channel count: a blob for another size has its own windows) and is recorded only when
    # msi_net_plan_calibrate SUCCEEDED -- it is all-or-nothing, so a degenerate first sample (a black frame) leaves the windows as they were and the next flagged
    # sample tries again (at most three failed attempts per blob).
    nout = {"blend_psv": 2 * num_planes, "blend_bg": 2 * num_planes + 3, "blend_bg_psv": 3 * num_planes + 3, "alpha_only": num_planes}[which_color_pred]
    ckey = tuple(net_input.shape[1:]) + (nout, ngf)
    cstate = model.__dict__.setdefault("_harness_calibration", {})     # ckey -> "ok" | number of failed attempts
    if deferred and "LayerNorm" in str(deferred[0]) and cstate.get(ckey, 0) != "ok" and cstate.get(ckey, 0) < 3:
        # the windows are an estimate from the weights (msi_hip.h, msi_net_plan_calibrate): measure them on this sample and repeat the forward
        try:
            moved = model.calibrate(net_input, nout, ngf)
            cstate[ckey] = "ok"
            print("LayerNorm windows calibrated on %s: %d layers moved" % (dirname, moved))
            del deferred[:]
            outs, net_input = model.infer_msi(src, ref, None, None, eye, eye, intr, which_color_pred, num_planes, planes,
                                              extra_outputs="blend_weights alphas psv", ngf=ngf, layer_format=layer_format)
            check_status()
        except MsiError as e:
            if cstate.get(ckey, 0) != "ok":
                cstate[ckey] = cstate.get(ckey, 0) + 1
                print("LayerNorm windows NOT calibrated on %s (windows unchanged; attempt %d of 3): %s" % (dirname, cstate[ckey], e))
            deferred.append(e)
    jouts = None
    if jitter_pose is not None:      # test.py:141-147: second inference with the sweep rotated by jitter_pose^-1
        jinv = np.linalg.inv(np.asarray(jitter_pose, dtype=np.float64)).astype(np.float32)
        jouts, _ = model.infer_msi(src, ref, None, None, eye, eye, intr, which_color_pred, num_planes, planes,
                                   extra_outputs="blend_weights alphas psv", ngf=ngf, jitter_pose_inv=jinv)
        check_status()
    os.makedirs(output_dir, exist_ok=True)
    if "tgt_image" in test_outputs:
        rgb, dep = model.msi_render_equirect_view_and_depth(outs["rgba_layers"], eye, pos, planes, intr)
        write_image(os.path.join(output_dir, "tgt_image_%s.png" % dirname), tgt[0].numpy() * 255.0)
        rgb8, dep8 = model.deprocess_image(rgb)[0], model.deprocess_depth_image(dep)[0]
        write_image(os.path.join(output_dir, "output_tgt_%s.png" % dirname), rgb8.cpu().numpy())
        write_image(os.path.join(output_dir, "output_depth_%s.png" % dirname), dep8.cpu().numpy())
        if scorer is not None:
            if recon:       # (before scorer.add: a sample the domain guard refuses here adds to neither list)
                pair = model.render_ods_pair(outs["rgba_layers"], planes, intrinsics=intr)       # [1,2,H,W,3]: left = ref, right = src
                pair8 = model.deprocess_image(pair[0])
                write_image(os.path.join(output_dir, "recon_ref_%s.png" % dirname), pair8[0].cpu().numpy())
                write_image(os.path.join(output_dir, "recon_src_%s.png" % dirname), pair8[1].cpu().numpy())
                scorer.add_recon(ref[0].numpy() * 255.0, src[0].numpy() * 255.0, pair8[0], pair8[1])
            scorer.add(dirname, scene, tgt[0].numpy() * 255.0, rgb8, dep8)
        if jouts is not None:        # test.py:160-165 renders through the jitter pose; :237-240 (the reference reads a
            # 'jitter_output_depth' it never produces -- here the depth is rendered the same way)
            jrgb, jdep = model.msi_render_equirect_view_and_depth(jouts["rgba_layers"], np.asarray(jitter_pose, np.float32),
                                                                  pos, planes, intr)
            write_image(os.path.join(output_dir, "jitter_output_tgt_%s.png" % dirname),
                        model.deprocess_image(jrgb)[0].cpu().numpy())
            write_image(os.path.join(output_dir, "jitter_output_depth_%s.png" % dirname),
                        model.deprocess_depth_image(jdep)[0].cpu().numpy())
    if "src_output_image" in test_outputs:
        o = model.msi_render_ods_view(outs["rgba_layers"], -1, eye, pos, planes, intr)
        write_image(os.path.join(output_dir, "output_src_%s.png" % dirname), model.deprocess_image(o)[0].cpu().numpy())
    if "ref_output_image" in test_outputs:
        o = model.msi_render_ods_view(outs["rgba_layers"], 1, eye, pos, planes, intr)
        write_image(os.path.join(output_dir, "output_ref_%s.png" % dirname), model.deprocess_image(o)[0].cpu().numpy())
    if "psp" in test_outputs:
        for vw in range(4):
            o = model.msi_render_perspective_view(outs["rgba_layers"], eye, pos, planes, intr, viewing_window=vw)
            write_image(os.path.join(output_dir, "output_ptgt%d_%s.png" % (vw, dirname)),
                        model.deprocess_image(o)[0].cpu().numpy())
    write_layer_outputs(outs, jouts, src, ref, num_planes, test_outputs, output_dir, dirname, which_color_pred)
    save_packed_msi(outs, output_dir, dirname, model, sparse_log)
    if deferred:
        raise deferred[0]
    return outs


def sample_dirname(scene, ids, test_type="", prefix=""):
    """test.py:209-217: `[video_[<prefix>_]]<scene>_<ref><src><tgt>`."""
    if "on_video" in test_type:
        name = "video_" + ("%s_" % prefix if prefix else "") + scene
    else:
        name = scene
    return name + "_%s%s%s" % (ids[0], ids[1], ids[2])


def run_sample_pp(model, images, input_offset, tgt_offset, planes, num_planes, ngf, test_outputs, output_dir, dirname,
                  which_color_pred="blend_psv", msi_format=None, scorer=None, scene=None, sparse_log=None):
    """input_type=PP (test.py:51; data_loader.py:205-226): perspective pair, source camera shifted by -input_offset along
    x, target by -tgt_offset, intrinsics fx = cx = W/2, fy = cy = H/2; plane-sweep volume at the slerp mid-point pose
    (train.py:118-121), target view by mpi_render_view through tgt_pose @ interp_pose_inv (msi.py:644-646).  The MPI path
    has no depth render (the reference has none either).  msi_format: as in run_sample.  sparse_log (--msi_pp_sparse): the saved stack
    is an edge-rule SparseLayers, which MSI.mpi_render_views reads; see save_packed_msi."""
    import torch
    from . import poses
    ref, src, tgt = (torch.from_numpy(np.ascontiguousarray(x[None])) for x in images)
    h, w = images[0].shape[:2]
    eye = np.eye(4, dtype=np.float32)[None]
    src_pose, tgt_pose = eye.copy(), eye.copy()
    src_pose[0, 0, 3] = -input_offset
    tgt_pose[0, 0, 3] = -tgt_offset
    K = np.array([[[0.5 * w, 0, 0.5 * w], [0, 0.5 * h, 0.5 * h], [0, 0, 1]]], dtype=np.float32)
    interp_inv = np.linalg.inv(poses.interpolate_pose(eye, src_pose).astype(np.float64)).astype(np.float32)
    outs, net_input = model.infer_msi(src, ref, None, None, eye, src_pose, K, which_color_pred, num_planes, planes,
                                      extra_outputs="blend_weights alphas psv", ngf=ngf, ref_pose_inv=interp_inv,
                                      layer_format="f32" if msi_format is None else ("f32", msi_format))
    os.makedirs(output_dir, exist_ok=True)
    if "tgt_image" in test_outputs:
        rgb = model.mpi_render_view(outs["rgba_layers"], np.matmul(tgt_pose, interp_inv).astype(np.float32), planes, K)
        write_image(os.path.join(output_dir, "tgt_image_%s.png" % dirname), tgt[0].numpy() * 255.0)
        rgb8 = model.deprocess_image(rgb)[0]
        write_image(os.path.join(output_dir, "output_tgt_%s.png" % dirname), rgb8.cpu().numpy())
        if scorer is not None:
            scorer.add(dirname, scene, tgt[0].numpy() * 255.0, rgb8)
    write_layer_outputs(outs, None, src, ref, num_planes, test_outputs, output_dir, dirname, which_color_pred)
    save_packed_msi(outs, output_dir, dirname, model, sparse_log, border='edge')
    return outs


def run_hres_sample(model, hres_images, baseline, tgt_pos, planes, output_dir, dirname, msi_format=None, hres_sparse_log=None,
                    factored=False):
    """The high-res pass of test.py:283-394 for one sample: the low-res blend weights / alphas the first pass saved
    (blend_weights.npy, alphas.npy, test.py:264-271) are upsampled (align_corners), the layers re-assembled from the
    high-res sweep volume and rendered -- one fused device pass (MSI.msi_render_equirect_hres) instead of the
    reference's per-plane sess.run + numpy composite -- and written as test.py:383-394 does: (x + 1) / 2 * 255 and
    depth * 255, clipped and truncated to uint8 by write_image.  msi_format ('rgba8' | 'rgba16f'): the launch that builds the
    high-res stack (MSI.hres_layers) also emits it packed, saved with its planes as msi_hres_<dirname>.npz; the images are
    the same bytes either way.  hres_sparse_log (--msi_hres_sparse; a list, needs msi_format): msi_hres_<dirname>.npz is the
    SparseLayers of MSI.hres_layers_sparse instead -- the dense packed stack is never built --, the sample's occupancy and bytes
    are appended to the list, and the images come from the fp32 stack as in a run without any of these flags.  factored
    (--hres_factored; without msi_format): no high-res stack is built at all -- the sample's FactoredLayers (MSI.hres_factors) is
    rendered directly (MSI.render_views) and saved as msi_hres_factors_<dirname>.npz; the images are the same bytes."""
    import torch
    bw_path, al_path = os.path.join(output_dir, "blend_weights.npy"), os.path.join(output_dir, "alphas.npy")
    if not (os.path.exists(bw_path) and os.path.exists(al_path)):
        raise FileNotFoundError("%s: the high-res pass needs blend_weights.npy and alphas.npy of the low-res pass "
                                "(run without high_res_only first, with blend_weights and alphas in --test_outputs)" % output_dir)
    bw, al = np.load(bw_path), np.load(al_path)
    ref, src = (torch.from_numpy(np.ascontiguousarray(x[None])) for x in hres_images[:2])
    eye = np.eye(4, dtype=np.float32)[None]
    intr = np.array([[[baseline, 0, 0], [0, 1, 0], [0, 0, 1]]], dtype=np.float32)
    pos = np.asarray(tgt_pos, dtype=np.float32)[None]
    packed = None
    if factored:
        factors = model.hres_factors(bw, al, ref, src, eye, eye, planes, intr)
        rgb, dep = model.render_views(factors, eye, pos)                          # [1,1,Hh,Wh,3], [1,1,Hh,Wh]
        rgb, dep = rgb[:, 0], dep[:, 0, :, :, None].expand(-1, -1, -1, 3)         # (the depth image has three equal channels)
    elif hres_sparse_log is not None:
        rgb, dep = model.msi_render_equirect_hres(bw, al, ref, src, eye, eye, eye, pos, planes, intr)
        packed = model.hres_layers_sparse(bw, al, ref, src, eye, eye, planes, intr, layer_format=msi_format)["sparse_layers"]
        b, hh, hw, d = packed.shape
        entry = dict(name=dirname, occupancy=packed.occupancy, nbytes=packed.nbytes,
                     dense_nbytes=b * d * hh * hw * packed.pool.element_size() * 4)
        hres_sparse_log.append(entry)
        print("Sparse high-res MSI of %s: occupancy %.4f, %d bytes (dense %s: %d bytes, never allocated)" % (
            dirname, entry["occupancy"], entry["nbytes"], msi_format, entry["dense_nbytes"]))
    elif msi_format is None:
        rgb, dep = model.msi_render_equirect_hres(bw, al, ref, src, eye, eye, eye, pos, planes, intr)
    else:
        layers = model.hres_layers(bw, al, ref, src, eye, eye, planes, intr, layer_format=("f32", msi_format))
        rgb, dep = model.msi_render_equirect_view_and_depth(layers["rgba_layers"], eye, pos, planes, intr)
        packed = layers["packed_layers"]
    os.makedirs(output_dir, exist_ok=True)
    print("Saving high-res output to %s" % output_dir)
    write_image(os.path.join(output_dir, "output_hrestgt_%s.png" % dirname), ((rgb[0].cpu().numpy() + 1.) / 2.) * 255.)
    write_image(os.path.join(output_dir, "output_hresdepth_%s.png" % dirname), dep[0].cpu().numpy() * 255.)
    if packed is not None:
        packed.save(os.path.join(output_dir, "msi_hres_%s.npz" % dirname))
    if factored:
        factors.save(os.path.join(output_dir, "msi_hres_factors_%s.npz" % dirname))
    return rgb, dep


def write_occupancy_log(path, msi_format, samples, what):
    """The occupancy log of a sparse run (sparse.json, pp_sparse.json, hres_sparse.json: one set of keys)."""
    from .sparse import TILE_H, TILE_W
    with open(path, "w") as f:
        json.dump(dict(format=msi_format, tile=[TILE_H, TILE_W], samples=samples,
                       mean_occupancy=float(np.mean([e["occupancy"] for e in samples])) if samples else None), f)
    print("%s written to %s" % (what, path))


def main(argv=None):
    ap = argparse.ArgumentParser(description=__doc__, formatter_class=argparse.RawDescriptionHelpFormatter)
    ap.add_argument("--cameras_glob", default="glob/test/ods/*.txt")
    ap.add_argument("--image_dir", default="glob/test_640x320")
    ap.add_argument("--hres_image_dir", default="glob/test_4096x2048", help="high-resolution images of the same samples (test.py:42)")
    ap.add_argument("--output_root", default="results")
    ap.add_argument("--experiment_name", default="msi-hip")
    ap.add_argument("--weights", default="", help=".npz of TF variables (net/<layer>/weights ...)")
    ap.add_argument("--checkpoint", default="", help="TF checkpoint prefix or directory (test.py:192-202: "
                    "<checkpoint_dir>/<experiment_name>); read without TensorFlow (matryodshka_amd/tf_checkpoint.py)")
    ap.add_argument("--step", type=int, default=0, help="global step recorded in step.txt (test.py:225-229)")
    ap.add_argument("--input_type", default="ODS", choices=["ODS", "PP"],
                    help="ODS pairs (camera lines `scene ref src tgt baseline tx ty tz`) or perspective pairs (`scene ref src tgt "
                         "input_offset tgt_offset`, datasets.py:427-437) -- test.py:51")
    ap.add_argument("--dtype", default="f32", choices=["f32", "bf16"],
                    help="f32, or bf16: the bf16 network tier (bf16 sweep volume, weights and activations; fp32 geometry) for "
                         "either input type")
    ap.add_argument("--msi_format", default=None, choices=["rgba8", "rgba16f"],
                    help="also save each sample's MSI as a compact layer stack msi_<dir>.npz (PackedLayers.save, planes included), "
                         "emitted by the same launch that writes the fp32 layers (with --test_type high_res also the high-res "
                         "stack, msi_hres_<dir>.npz); default: off")
    ap.add_argument("--msi_sparse", action="store_true",
                    help="with --msi_format, ODS inputs: save msi_<dir>.npz as a SparseLayers (only the occupied 4 x 16 tiles; --height %% 4 == 0 "
                         "and --width %% 16 == 0) and write each sample's occupancy and bytes to <experiment>/sparse.json; the high-res stack of "
                         "--test_type high_res (msi_hres_<dir>.npz) is not sparsified and stays dense, and high_res_only is refused; default: off")
    ap.add_argument("--height", type=int, default=320)
    ap.add_argument("--width", type=int, default=640)
    ap.add_argument("--msi_pp_sparse", action="store_true",
                    help="with --msi_format and --input_type PP: save msi_<dir>.npz as an edge-rule SparseLayers (the occupied 4 x 16 tiles a "
                         "render that never reads the opposite border can see: MSI.mpi_render_views reads it; --height %% 4 == 0 and "
                         "--width %% 16 == 0) and write each sample's occupancy and bytes to <experiment>/pp_sparse.json; the images are the "
                         "bytes of a run without the flag; default: off")
    ap.add_argument("--msi_hres_sparse", action="store_true",
                    help="with --msi_format and a high_res --test_type: save the high-res stack msi_hres_<dir>.npz as a SparseLayers built "
                         "directly from the low-res alphas and the high-res images (MSI.hres_layers_sparse: the dense high-res stack is "
                         "never allocated; --hres_height %% 4 == 0 and --hres_width %% 16 == 0) and write each sample's occupancy and bytes to "
                         "<experiment>/hres_sparse.json; the images are the bytes of a run without the flag; default: off")
    ap.add_argument("--hres_factored", action="store_true",
                    help="with a high_res --test_type: build NO high-res stack -- render the target view and depth straight from the stack's "
                         "factors (MSI.hres_factors, MSI.render_views) and save them as msi_hres_factors_<dir>.npz (a FactoredLayers); the "
                         "images are the bytes of a run without the flag; not with --msi_format or --msi_hres_sparse, which ask for a "
                         "materialised stack; default: off")
    ap.add_argument("--hres_height", type=int, default=2048, help="loader.py:34")
    ap.add_argument("--hres_width", type=int, default=4096, help="loader.py:35")
    ap.add_argument("--num_msi_planes", type=int, default=32)
    ap.add_argument("--num_psv_planes", type=int, default=32,
                    help="test.py:60; must equal --num_msi_planes: the reference indexes the source volume with num_msi_planes "
                         "(msi.py:138), so other combinations are not defined there either")
    ap.add_argument("--min_depth", type=float, default=1.0)
    ap.add_argument("--max_depth", type=float, default=100.0)
    ap.add_argument("--ngf", type=int, default=64)
    ap.add_argument("--coord_net", action="store_true",
                    help="msi_coord_train_net (FLAGS.coord_net, test.py:52, default False = msi_train_net); the released "
                         "ODS models use it (scripts/test/ods-wotemp-elpips-coord-reg.sh).  With --checkpoint / --weights "
                         "the network is inferred from conv1_1/weights' input channels when the flag is absent")
    ap.add_argument("--which_color_pred", default="blend_psv",
                    help="blend_psv | blend_bg | blend_bg_psv | alpha_only (test.py:55-56)")
    ap.add_argument("--transform_inverse_reg", action="store_true",
                    help="also infer with a jittered sweep pose and write jitter_output_* (test.py:141-147, 160-165)")
    ap.add_argument("--rot_factor", type=float, default=1.0, help="test.py:72")
    ap.add_argument("--tr_factor", type=float, default=1.0, help="test.py:73")
    ap.add_argument("--random_seed", type=int, default=8964)
    ap.add_argument("--test_type", default="",
                    help="concatenate with _: on_video (directory names video_[<prefix>_]<scene>_..., test.py:209-217), high_res "
                         "(low-res pass, then the high-res re-render of test.py:283-394), high_res_only (only the latter)")
    ap.add_argument("--prefix", default="", help="test.py:78: prefix of on_video directory names")
    ap.add_argument("--test_outputs", default="rgba_layers_src_image_ref_image_tgt_image_blend_weights_alphas",
                    help="test.py:79-82")
    ap.add_argument("--num_runs", type=int, default=-1)
    ap.add_argument("--score", action="store_true",
                    help="score output_tgt against tgt_image on the device (MSI.score_views) and write <experiment>/scores.json: ssim and "
                         "psnr per example and their means; with on_video also the consecutive-frame differences per scene; default: off")
    ap.add_argument("--recon_score", action="store_true",
                    help="with --score, ODS inputs: render both input eyes back from each sample's MSI in one launch (MSI.render_ods_pair), "
                         "write recon_ref_<dir>.png / recon_src_<dir>.png and add their ssim / psnr against ref_image / src_image to scores.json")
    ap.add_argument("--strict", action="store_true",
                    help="abort at the first sample whose LayerNorm statistics leave the kernels' fixed-point window or whose target "
                         "position lies outside the innermost sphere (default: write UNRELIABLE.txt next to its files and go on)")
    args = ap.parse_args(argv)
    if args.recon_score and not args.score:
        ap.error("--recon_score needs --score")
    if args.recon_score and args.input_type != "ODS":
        ap.error("--recon_score renders ODS eyes: --input_type ODS only")
    if args.msi_sparse and args.msi_format is None:
        ap.error("--msi_sparse needs --msi_format")
    if args.msi_sparse and args.input_type != "ODS":
        ap.error("--msi_sparse keeps sphere stacks (the planar viewer does not read sparse stacks): --input_type ODS only")
    if args.msi_sparse and (args.height % 4 or args.width % 16):
        ap.error("--msi_sparse needs --height % 4 == 0 and --width % 16 == 0")
    if args.msi_sparse and "high_res_only" in args.test_type:
        ap.error("--msi_sparse sparsifies the low-res stacks only: --test_type high_res_only has none (the high-res stack stays dense)")
    if args.msi_pp_sparse and args.msi_format is None:
        ap.error("--msi_pp_sparse needs --msi_format")
    if args.msi_pp_sparse and args.input_type != "PP":
        ap.error("--msi_pp_sparse keeps planar stacks: it needs --input_type PP (ODS inputs: --msi_sparse)")
    if args.msi_pp_sparse and (args.height % 4 or args.width % 16):
        ap.error("--msi_pp_sparse needs --height % 4 == 0 and --width % 16 == 0")
    if args.msi_hres_sparse and args.msi_format is None:
        ap.error("--msi_hres_sparse needs --msi_format")
    if args.msi_hres_sparse and "high_res" not in args.test_type:
        ap.error("--msi_hres_sparse builds the high-res stack: it needs a high_res --test_type")
    if args.msi_hres_sparse and (args.hres_height % 4 or args.hres_width % 16):
        ap.error("--msi_hres_sparse needs --hres_height % 4 == 0 and --hres_width % 16 == 0")
    if args.hres_factored and (args.msi_format is not None or args.msi_hres_sparse):
        ap.error("--hres_factored builds no high-res stack: --msi_format and --msi_hres_sparse ask for a materialised one")
    if args.hres_factored and "high_res" not in args.test_type:
        ap.error("--hres_factored renders the high-res pass: it needs a high_res --test_type")
    if args.num_psv_planes != args.num_msi_planes:
        raise SystemExit("--num_psv_planes must equal --num_msi_planes (msi.py:138 indexes the source volume with num_msi_planes)")
    if "high_res" in args.test_type and args.input_type != "ODS":
        raise SystemExit("--test_type high_res is the ODS path (test.py:283-394)")

    from . import MSI, nets
    from ._native import MsiError
    failed = []
    d = args.num_msi_planes
    coord = args.coord_net
    nout = {"blend_psv": 2 * d, "blend_bg": 2 * d + 3, "blend_bg_psv": 3 * d + 3, "alpha_only": d}[args.which_color_pred]
    if args.checkpoint:
        from . import tf_checkpoint
        weights, args.step = tf_checkpoint.network_weights(args.checkpoint)
    elif args.weights:
        weights = dict(np.load(args.weights))
    else:
        weights = nets.init_weights(6 * d, nout, args.ngf, coord)
    # with weights the network (CoordNet or not) follows from conv1_1/weights' input channels unless the flag insists
    model = MSI(weights=weights, coord_net=True if coord else None, input_type=args.input_type, dtype=args.dtype)
    # test.py:112 evaluates tf_random_rotation INSIDE the graph: every sess.run (every sample) draws a new jitter pose;
    # here one seeded generator is advanced per sample
    jitter_rng = np.random.RandomState(args.random_seed) if args.transform_inverse_reg else None
    planes = model.inv_depths(args.min_depth, args.max_depth, d)
    exp_dir = os.path.join(args.output_root, args.experiment_name)
    os.makedirs(exp_dir, exist_ok=True)
    scorer = DeviceScores(model, keep_frames="on_video" in args.test_type) if args.score else None
    sparse_log = [] if args.msi_sparse else None
    hres_sparse_log = [] if args.msi_hres_sparse else None
    pp_sparse_log = [] if args.msi_pp_sparse else None
    samples = list(parse_camera_files(args.cameras_glob, args.input_type))
    if args.num_runs >= 0:
        samples = samples[:args.num_runs]
    n = 0
    if "high_res_only" not in args.test_type:
        for scene, ids, cam in samples:
            images = [load_image(os.path.join(args.image_dir, "%s_pos%s.jpeg" % (scene, i)), args.height, args.width)
                      for i in ids]
            dirname = sample_dirname(scene, ids, args.test_type, args.prefix)
            out_dir = os.path.join(exp_dir, dirname)
            print("Saving to %s" % out_dir)
            if n == 0:
                with open(os.path.join(exp_dir, "step.txt"), "w") as f:
                    f.write("%d" % args.step)
            try:
                if args.input_type == "PP":
                    run_sample_pp(model, images, cam[0], cam[1], planes, d, args.ngf, args.test_outputs, out_dir, dirname,
                                  which_color_pred=args.which_color_pred, msi_format=args.msi_format, scorer=scorer, scene=scene,
                                  sparse_log=pp_sparse_log)
                    model.network_status()   # raises if a LayerNorm statistic left the range the kernels resolve
                else:
                    jitter = None
                    if jitter_rng is not None:
                        from . import poses
                        jitter = poses.random_rotation(args.rot_factor, args.tr_factor, jitter_rng)
                    run_sample(model, images, cam[0], cam[1:4], planes, d, args.ngf, args.test_outputs, out_dir, dirname,
                               which_color_pred=args.which_color_pred, jitter_pose=jitter, msi_format=args.msi_format,
                               scorer=scorer, scene=scene, recon=args.recon_score, sparse_log=sparse_log)
                model.render_status()        # raises if a render's ray origin was outside the innermost sphere
            except (MsiError, ValueError) as e:
                # a sample whose statistics leave the LayerNorm window (a heuristic built from the weights) or whose target lies
                # outside the innermost sphere must not stop the remaining samples: its files are on disk but
                # flagged; --strict restores the abort
                if args.strict:
                    raise
                failed.append(dirname)
                print("WARNING: sample %s is outside the range the kernels resolve: %s" % (dirname, e))
                os.makedirs(out_dir, exist_ok=True)   # (a ValueError of the host-side domain guard can precede the first file)
                with open(os.path.join(out_dir, "UNRELIABLE.txt"), "w") as f:
                    f.write(str(e) + "\n")
            n += 1
    if "high_res" in args.test_type:
        for scene, ids, cam in samples:
            hres = [load_image(os.path.join(args.hres_image_dir, "%s_pos%s.jpeg" % (scene, i)), args.hres_height, args.hres_width)
                    for i in ids[:2]]
            dirname = sample_dirname(scene, ids, args.test_type, args.prefix)
            run_hres_sample(model, hres, cam[0], cam[1:4], planes, os.path.join(exp_dir, dirname), dirname, msi_format=args.msi_format,
                            hres_sparse_log=hres_sparse_log, factored=args.hres_factored)
            n += "high_res_only" in args.test_type
    for log, name, what in ((hres_sparse_log, "hres_sparse.json", "High-res occupancies"), (pp_sparse_log, "pp_sparse.json", "PP occupancies"),
                            (sparse_log, "sparse.json", "Occupancies")):
        if log is not None:
            write_occupancy_log(os.path.join(exp_dir, name), args.msi_format, log, what)
    if scorer is not None:
        with open(os.path.join(exp_dir, "scores.json"), "w") as f:
            json.dump(scorer.table(), f)
        print("Scores written to %s" % os.path.join(exp_dir, "scores.json"))
    print("processed %d samples%s" % (n, " (%d flagged UNRELIABLE: %s)" % (len(failed), ", ".join(failed)) if failed else ""))
    return n


if __name__ == "__main__":
    main()
