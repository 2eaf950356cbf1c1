"""--test_type high_res with --msi_hres_sparse (matryodshka_amd/harness.py): msi_hres_<dir>.npz is the SparseLayers that
MSI.hres_layers_sparse builds without the dense stack -- equal to SparseLayers.from_codes of the packed file a
--msi_format-only run writes --, <experiment>/hres_sparse.json has the sample's occupancy and bytes, and the images are the bytes
of a run without the flag.  The sizes of tests/test_gpu_hres_harness.py."""
import json

import numpy as np
import pytest

pytestmark = pytest.mark.gpu


def test_harness_high_res_mode_keeps_the_stack_sparse(tmp_path):
    from matryodshka_amd import harness
    from matryodshka_amd.packed import PackedLayers
    from matryodshka_amd.sparse import SparseLayers
    from oracle import nets as onets
    from tests.test_gpu_harness import _write_sample_images
    h, w, hh, hw, d, ngf = 32, 64, 64, 128, 8, 16
    _write_sample_images(tmp_path / "lo", "office_0", h, w, 7)
    _write_sample_images(tmp_path / "hi", "office_0", 2 * hh, 2 * hw, 8)
    cam = tmp_path / "cams.txt"
    cam.write_text("office_0 000 001 002 0.032 0.02 -0.01 0.03\n")
    weights = onets.init_weights(6 * d, 2 * d, ngf=ngf, coord_net=True, seed=17, randomize_affine=True)
    np.savez(str(tmp_path / "w.npz"), **weights)
    tag = "office_0_000001002"

    def run(out, extra):
        args = ["--cameras_glob", str(cam), "--image_dir", str(tmp_path / "lo"), "--hres_image_dir", str(tmp_path / "hi"),
                "--output_root", str(tmp_path / out), "--experiment_name", "e", "--height", str(h), "--width", str(w),
                "--hres_height", str(hh), "--hres_width", str(hw), "--num_msi_planes", str(d), "--num_psv_planes", str(d),
                "--ngf", str(ngf), "--weights", str(tmp_path / "w.npz"), "--test_type", "high_res"]
        assert harness.main(args + extra) == 1
        return tmp_path / out / "e" / tag

    plain, packed = run("plain", []), run("packed", ["--msi_format", "rgba16f"])
    sparse = run("sparse", ["--msi_format", "rgba16f", "--msi_hres_sparse"])
    for name in ("output_hrestgt_%s.png" % tag, "output_hresdepth_%s.png" % tag, "output_tgt_%s.png" % tag):
        assert (sparse / name).read_bytes() == (plain / name).read_bytes(), name
    assert not (plain.parent / "hres_sparse.json").exists() and not (packed.parent / "hres_sparse.json").exists()
    # the low-res stack of the first pass stays what --msi_format makes it: dense
    low = PackedLayers.load(str(sparse / ("msi_%s.npz" % tag)))
    assert np.array_equal(low.data.numpy(), PackedLayers.load(str(packed / ("msi_%s.npz" % tag))).data.numpy())
    got = SparseLayers.load(str(sparse / ("msi_hres_%s.npz" % tag)))
    dense = PackedLayers.load(str(packed / ("msi_hres_%s.npz" % tag)))
    want = SparseLayers.from_codes(dense, dense.format)
    assert got.format == want.format == "rgba16f" and got.shape == want.shape == (1, hh, hw, d) and got.planes == want.planes == dense.planes
    for name in ("table", "layer_start", "pool"):
        a, b = getattr(got, name).numpy(), getattr(want, name).numpy()
        assert a.dtype == b.dtype and a.shape == b.shape and np.array_equal(a.view(np.uint8), b.view(np.uint8)), name
    log = json.loads((sparse.parent / "hres_sparse.json").read_text())
    assert log["format"] == "rgba16f" and log["tile"] == [4, 16] and [e["name"] for e in log["samples"]] == [tag]
    entry = log["samples"][0]
    assert entry["occupancy"] == got.occupancy == log["mean_occupancy"] and 0 < entry["occupancy"] <= 1
    assert entry["nbytes"] == got.nbytes and entry["dense_nbytes"] == dense.nbytes == 8 * d * hh * hw
