"""--msi_pp_sparse (matryodshka_amd/harness.py): with --msi_format and --input_type PP the harness keeps each sample's MPI as an edge-rule
SparseLayers -- the file loads as one, MSI.mpi_render_views renders from it the pixels of the dense msi_<dir>.npz of the same run
without the flag, the run's pp_sparse.json holds the sample's occupancy and bytes, and every image is the bytes of that other run."""
import json
import os

import numpy as np
import pytest

pytestmark = pytest.mark.gpu


def test_harness_saves_an_edge_stack_that_renders_like_the_dense_one(tmp_path):
    import torch
    from PIL import Image
    from matryodshka_amd import MSI, harness
    from matryodshka_amd.packed import PackedLayers
    from matryodshka_amd.sparse import SparseLayers
    h, w, d, ngf = 16, 32, 4, 8                   # (the smallest frame of the harness tests: one tile column more than a tile, four tile rows)
    img_dir = tmp_path / "images"; img_dir.mkdir()
    rng = np.random.RandomState(0)
    for name in ("000", "001", "002"):
        arr = np.clip(rng.uniform(0, 255, size=(2 * h, 2 * w, 3)), 0, 255).astype(np.uint8)
        Image.fromarray(arr).save(str(img_dir / ("room_1_pos%s.jpeg" % name)), quality=95)
    cam = tmp_path / "cams.txt"
    cam.write_text("room_1 000 001 002 0.064 0.03\n")
    name = "room_1_000001002"
    common = ["--cameras_glob", str(cam), "--image_dir", str(img_dir), "--experiment_name", "exp", "--height", str(h), "--width", str(w),
              "--num_msi_planes", str(d), "--num_psv_planes", str(d), "--ngf", str(ngf), "--test_outputs", "tgt_image_rgba_layers",
              "--input_type", "PP", "--msi_format", "rgba8"]
    assert harness.main(common + ["--output_root", str(tmp_path / "dense")]) == 1
    assert harness.main(common + ["--output_root", str(tmp_path / "sparse"), "--msi_pp_sparse"]) == 1
    assert not (tmp_path / "dense" / "exp" / "pp_sparse.json").exists()
    log = json.loads((tmp_path / "sparse" / "exp" / "pp_sparse.json").read_text())
    assert sorted(log) == ["format", "mean_occupancy", "samples", "tile"]                       # sparse.json's keys
    assert log["format"] == "rgba8" and log["tile"] == [4, 16] and [e["name"] for e in log["samples"]] == [name]
    assert sorted(log["samples"][0]) == ["dense_nbytes", "name", "nbytes", "occupancy"]
    sp = SparseLayers.load(str(tmp_path / "sparse" / "exp" / name / ("msi_%s.npz" % name)))
    pk = PackedLayers.load(str(tmp_path / "dense" / "exp" / name / ("msi_%s.npz" % name)))
    assert sp.border == 'edge' and sp.format == "rgba8" and sp.shape == pk.shape == (1, h, w, d) and sp.planes == pk.planes and len(sp.planes) == d
    entry = log["samples"][0]
    assert entry["occupancy"] == sp.occupancy == log["mean_occupancy"] and 1.0 / d <= sp.occupancy <= 1.0
    assert entry["nbytes"] == sp.nbytes and entry["dense_nbytes"] == pk.nbytes
    m = MSI()
    assert np.array_equal(sp.expand_np(), m.densify_layers(sp).data.cpu().numpy())
    K = np.array([[0.5 * w, 0, 0.5 * w], [0, 0.5 * h, 0.5 * h], [0, 0, 1]], np.float32)
    pose = np.tile(np.eye(4, dtype=np.float32), (1, 2, 1, 1))
    pose[0, 0, 0, 3] = -0.03                      # the harness's own target offset, and a view that looks past the border
    pose[0, 1, :3, 3] = [0.3, 0.0, 0.1]
    for size in (None, (h + 3, w + 5)):
        rgb_s, dep_s = m.mpi_render_views(sp, pose, intrinsics=K, size=size)
        rgb_d, dep_d = m.mpi_render_views(pk, pose, intrinsics=K, size=size)
        assert np.array_equal(rgb_s.cpu().numpy(), rgb_d.cpu().numpy()) and np.array_equal(dep_s.cpu().numpy(), dep_d.cpu().numpy())
    with pytest.raises(TypeError):
        m.render_views(sp, pose, np.zeros((1, 2, 3), np.float32))
    # every image of the run is the bytes of the run without the flag
    images = sorted(f for f in os.listdir(str(tmp_path / "dense" / "exp" / name)) if f.endswith(".png"))
    assert len(images) > 2 and images == sorted(f for f in os.listdir(str(tmp_path / "sparse" / "exp" / name)) if f.endswith(".png"))
    for f in images:
        assert (tmp_path / "dense" / "exp" / name / f).read_bytes() == (tmp_path / "sparse" / "exp" / name / f).read_bytes(), f
    torch.cuda.synchronize()
