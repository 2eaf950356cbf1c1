"""--msi_sparse (matryodshka_amd/harness.py): with --msi_format the harness keeps each sample's MSI as a SparseLayers -- the file loads
as one, renders the pixels of the dense msi_<dir>.npz of the same run without the flag, and the run's sparse.json holds every
sample's occupancy and bytes."""
import json

import numpy as np
import pytest

pytestmark = pytest.mark.gpu


def test_harness_saves_sparse_stacks_that_render_like_the_dense_ones(tmp_path):
    import torch
    from PIL import Image
    from matryodshka_amd import MSI, harness
    from matryodshka_amd.packed import PackedLayers
    from matryodshka_amd.sparse import SparseLayers
    h, w, d, ngf = 16, 32, 4, 8
    img_dir = tmp_path / "images"; img_dir.mkdir()
    rng = np.random.RandomState(0)
    for name in ("000", "001", "002", "003"):
        arr = np.clip(rng.uniform(0, 255, size=(2 * h, 2 * w, 3)), 0, 255).astype(np.uint8)
        Image.fromarray(arr).save(str(img_dir / ("room_0_pos%s.jpeg" % name)), quality=95)
    cam = tmp_path / "cams.txt"
    cam.write_text("room_0 000 001 002 0.032 0.01 -0.02 0.03\nroom_0 001 002 003 0.032 -0.02 0.01 0.02\n")
    names = ["room_0_000001002", "room_0_001002003"]
    common = ["--cameras_glob", str(cam), "--image_dir", str(img_dir), "--experiment_name", "exp", "--height", str(h), "--width", str(w),
              "--num_msi_planes", str(d), "--num_psv_planes", str(d), "--ngf", str(ngf), "--test_outputs", "tgt_image",
              "--msi_format", "rgba8"]
    assert harness.main(common + ["--output_root", str(tmp_path / "dense")]) == 2
    assert harness.main(common + ["--output_root", str(tmp_path / "sparse"), "--msi_sparse"]) == 2
    assert not (tmp_path / "dense" / "exp" / "sparse.json").exists()
    log = json.loads((tmp_path / "sparse" / "exp" / "sparse.json").read_text())
    assert log["format"] == "rgba8" and log["tile"] == [4, 16] and [e["name"] for e in log["samples"]] == names
    m = MSI()
    pose = np.tile(np.eye(4, dtype=np.float32), (1, 2, 1, 1))
    pose[0, 1, :3, :3] = [[0, -1, 0], [1, 0, 0], [0, 0, 1]]
    pos = np.array([[[0.02, -0.01, 0.03], [-0.03, 0.02, 0.01]]], np.float32)
    for name, entry in zip(names, log["samples"]):
        sparse_path = str(tmp_path / "sparse" / "exp" / name / ("msi_%s.npz" % name))
        sp = SparseLayers.load(sparse_path)
        pk = PackedLayers.load(str(tmp_path / "dense" / "exp" / name / ("msi_%s.npz" % name)))
        assert sp.format == "rgba8" and sp.shape == pk.shape == (1, h, w, d) and sp.planes == pk.planes and len(sp.planes) == d
        assert entry["occupancy"] == sp.occupancy and 1.0 / d <= sp.occupancy <= 1.0
        assert entry["nbytes"] == sp.nbytes and entry["dense_nbytes"] == pk.nbytes
        assert np.array_equal(sp.expand_np(), m.densify_layers(sp).data.cpu().numpy())
        with pytest.raises(ValueError):                              # the dense file is not a SparseLayers file
            SparseLayers.load(str(tmp_path / "dense" / "exp" / name / ("msi_%s.npz" % name)))
        for kw in ({}, dict(camera='ods', eye=np.array([1.0, -1.0], np.float32), baseline=0.032, size=(h + 3, w + 5))):
            rgb_s, dep_s = m.render_views(sp, pose, pos, **kw)
            rgb_d, dep_d = m.render_views(pk, pose, pos, **kw)
            assert np.array_equal(rgb_s.cpu().numpy(), rgb_d.cpu().numpy()) and np.array_equal(dep_s.cpu().numpy(), dep_d.cpu().numpy())
    assert log["mean_occupancy"] == float(np.mean([e["occupancy"] for e in log["samples"]]))
    torch.cuda.synchronize()
    assert m.render_status() == 0
