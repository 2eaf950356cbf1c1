"""--test_type high_res with --msi_format (matryodshka_amd/harness.py): the high-res pass also keeps its layer stack, packed,
as msi_hres_<dir>.npz -- written by the launch that builds the fp32 stack (MSI.hres_layers) -- and the images it writes are
the bytes of a run without --msi_format."""
import numpy as np
import pytest

pytestmark = pytest.mark.gpu


def test_harness_high_res_mode_keeps_the_packed_stack(tmp_path):
    import torch
    from matryodshka_amd import MSI, harness
    from matryodshka_amd.packed import PackedLayers
    from oracle import nets as onets
    from tests.test_gpu_harness import _write_sample_images
    h, w, hh, hw, d, ngf = 32, 64, 64, 128, 8, 16                       # the sizes of the harness' high-res test
    _write_sample_images(tmp_path / "lo", "office_0", h, w, 7)
    _write_sample_images(tmp_path / "hi", "office_0", 2 * hh, 2 * hw, 8)
    cam = tmp_path / "cams.txt"
    cam.write_text("office_0 000 001 002 0.032 0.02 -0.01 0.03\n")
    weights = onets.init_weights(6 * d, 2 * d, ngf=ngf, coord_net=True, seed=17, randomize_affine=True)
    np.savez(str(tmp_path / "w.npz"), **weights)

    def run(out, extra):
        args = ["--cameras_glob", str(cam), "--image_dir", str(tmp_path / "lo"), "--hres_image_dir", str(tmp_path / "hi"),
                "--output_root", str(tmp_path / out), "--experiment_name", "e", "--height", str(h), "--width", str(w),
                "--hres_height", str(hh), "--hres_width", str(hw), "--num_msi_planes", str(d), "--num_psv_planes", str(d),
                "--ngf", str(ngf), "--weights", str(tmp_path / "w.npz"), "--test_type", "high_res"]
        assert harness.main(args + extra) == 1
        return tmp_path / out / "e" / tag

    tag = "office_0_000001002"
    plain, packed = run("plain", []), run("packed", ["--msi_format", "rgba8"])
    assert not (plain / ("msi_hres_%s.npz" % tag)).exists()
    for name in ("output_hrestgt_%s.png" % tag, "output_hresdepth_%s.png" % tag, "output_tgt_%s.png" % tag):
        assert (packed / name).read_bytes() == (plain / name).read_bytes(), name
    assert (packed / ("msi_%s.npz" % tag)).exists()                     # (the low-res stack of the first pass, as before)
    got = PackedLayers.load(str(packed / ("msi_hres_%s.npz" % tag)))
    assert got.format == "rgba8" and got.shape == (1, hh, hw, d)
    # the same stack from hres_layers called directly on what the harness read
    m = MSI(weights=weights)
    planes = m.inv_depths(1.0, 100.0, d)
    assert got.planes == tuple(float(p) for p in planes)
    href, hsrc = (torch.from_numpy(harness.load_image(str(tmp_path / "hi" / ("office_0_pos%s.jpeg" % n)), hh, hw)[None])
                  for n in ("000", "001"))
    eye = np.eye(4, dtype=np.float32)[None]
    intr = np.array([[[0.032, 0, 0], [0, 1, 0], [0, 0, 1]]], np.float32)
    want = m.hres_layers(np.load(str(packed / "blend_weights.npy")), np.load(str(packed / "alphas.npy")), href, hsrc, eye, eye,
                         planes, intr, layer_format="rgba8")["packed_layers"]
    assert torch.equal(got.data, want.data.cpu())
    assert int(got.data.max()) > int(got.data.min())
