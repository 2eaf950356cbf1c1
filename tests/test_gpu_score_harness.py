"""harness --score and evaluate --on_device: the scores the device computes during a run are the scores evaluate.py computes
from the PNG files the same run wrote.  The data set is the small synthetic one of the harness tests (jpeg frames at the working
size, camera lines of one scene), at their smallest size: 16 x 32, 4 planes, ngf 8 for ODS; 64 x 64, 8 planes, ngf 16 for PP.

SSIM and PSNR agree to 1e-9 (fp64 on both sides, tests/test_gpu_score.py derives the bound).  The frame differences are sums of
integers: the device value equals the fp64 mean exactly; evaluate_consecutive_one takes the mean of FLOAT32 images, so its value
is the float32 rounding of the same quotient (the sum stays below 2^24 here and is exact in float32) and is compared as that."""
import json

import numpy as np
import pytest

pytestmark = pytest.mark.gpu

TOL = 1e-9


def _write_frames(img_dir, scene, h, w, seed, count):
    from PIL import Image
    from matryodshka_amd.synthetic import smooth_noise
    img_dir.mkdir(exist_ok=True)
    rng = np.random.RandomState(seed)
    for k in range(count):
        arr = (smooth_noise(rng, 1, h, w)[0] * 255).astype(np.uint8)
        Image.fromarray(arr).save(str(img_dir / ("%s_pos%.3d.jpeg" % (scene, k))), quality=95)


def _ods_run(tmp_path, extra, name="e"):
    """Three ODS samples of one scene (frames k, k+1, k+2 of five) at 16 x 32 -> the experiment directory."""
    from matryodshka_amd import harness
    h, w, d, ngf = 16, 32, 4, 8
    _write_frames(tmp_path / "img", "room_0", h, w, 7, 5)
    cam = tmp_path / "cams.txt"
    cam.write_text("".join("room_0 %.3d %.3d %.3d 0.032 %.3f -0.02 0.03\n" % (k, k + 1, k + 2, 0.01 * (k + 1)) for k in range(3)))
    assert harness.main(["--cameras_glob", str(cam), "--image_dir", str(tmp_path / "img"), "--output_root", str(tmp_path / "o"),
                         "--experiment_name", name, "--height", str(h), "--width", str(w), "--num_msi_planes", str(d),
                         "--num_psv_planes", str(d), "--ngf", str(ngf), "--test_outputs", "tgt_image"] + extra) == 3
    return tmp_path / "o" / name


def _check_examples(root, exp, scores, names):
    from matryodshka_amd import evaluate as E
    assert scores["examples"] == names
    assert len(scores["ssim"]) == len(scores["psnr"]) == len(names)
    for k, e in enumerate(names):
        ssim, psnr = E.evaluate_one(str(root), exp, e)
        print(e, scores["ssim"][k], ssim, scores["psnr"][k], psnr)
        assert abs(scores["ssim"][k] - ssim) <= TOL and abs(scores["psnr"][k] - psnr) <= TOL, e
        assert ssim < 1.0 and np.isfinite(psnr)
    assert abs(scores["mean_ssim"] - np.mean(scores["ssim"])) <= 1e-12 and abs(scores["mean_psnr"] - np.mean(scores["psnr"])) <= 1e-12


def _check_tables(host, dev):
    assert sorted(host) == sorted(dev)
    assert host["model_names"] == dev["model_names"] and host["examples"] == dev["examples"]
    for key in ("ssim", "psnr", "mean_ssim", "mean_psnr"):
        a, b = np.asarray(host[key], np.float64), np.asarray(dev[key], np.float64)
        assert a.shape == b.shape and (a.size == 0 or np.abs(a - b).max() <= TOL), key


def test_ods_scores_equal_evaluate_on_the_written_files(tmp_path):
    from matryodshka_amd import evaluate as E
    exp = _ods_run(tmp_path, ["--score"])
    scores = json.loads((exp / "scores.json").read_text())
    names = ["room_0_%.3d%.3d%.3d" % (k, k + 1, k + 2) for k in range(3)]
    _check_examples(tmp_path / "o", "e", scores, names)
    assert "consecutive" not in scores
    # evaluate.main on the same files: host table == device table
    common = ["--result_root", str(tmp_path / "o"), "--model_names", "e"]
    host = E.main(common + ["--output_table", str(tmp_path / "host.json")])
    dev = E.main(common + ["--output_table", str(tmp_path / "dev.json"), "--on_device"])
    assert host["examples"] == names
    _check_tables(host, dev)
    _check_tables(json.loads((tmp_path / "host.json").read_text()), json.loads((tmp_path / "dev.json").read_text()))
    assert np.abs(np.asarray(host["ssim"])[:, 0] - scores["ssim"]).max() <= TOL


def test_video_run_scores_consecutive_frames(tmp_path):
    from matryodshka_amd import evaluate as E
    exp = _ods_run(tmp_path, ["--score", "--test_type", "on_video"])
    scores = json.loads((exp / "scores.json").read_text())
    names = ["video_room_0_%.3d%.3d%.3d" % (k, k + 1, k + 2) for k in range(3)]
    _check_examples(tmp_path / "o", "e", scores, names)
    assert len(scores["consecutive"]) == 1
    entry = scores["consecutive"][0]
    assert entry["scene"] == "room_0" and entry["frames"] == names
    assert len(entry["output_tgt"]) == len(entry["output_depth"]) == 2
    for k in range(2):
        pair = (names[k], names[k + 1])
        t32, z32 = E.evaluate_consecutive_one(str(tmp_path / "o"), "e", pair)
        imgs = [[E.load_image(str(exp / e / ("%s_%s.png" % (kind, e)))) for e in pair] for kind in ("output_tgt", "output_depth")]
        print(pair, entry["output_tgt"][k], t32, entry["output_depth"][k], z32)
        assert entry["output_tgt"][k] == E.mae(*imgs[0]) and entry["output_depth"][k] == E.mae(*imgs[1])
        assert np.float32(entry["output_tgt"][k]) == np.float32(t32) and np.float32(entry["output_depth"][k]) == np.float32(z32)
        assert t32 > 0
    # evaluate --video: the host table and the device table agree on the frame differences as well
    common = ["--result_root", str(tmp_path / "o"), "--model_names", "e", "--video", "--videos", "room_0 office_0"]
    host = E.main(common + ["--output_table", str(tmp_path / "host.json")])
    dev = E.main(common + ["--output_table", str(tmp_path / "dev.json"), "--on_device"])
    _check_tables(host, dev)
    assert host["video_scenes"] == dev["video_scenes"] == ["room_0", "office_0"]
    assert [len(s) for s in host["consecutive"]] == [2, 0] == [len(s) for s in dev["consecutive"]]
    for k, (a, b) in enumerate(zip(host["consecutive"][0], dev["consecutive"][0])):
        assert a["frames"] == b["frames"] == [names[k], names[k + 1]]
        assert np.shape(b["diffs"]) == (1, 2) and np.array_equal(np.float32(a["diffs"]), np.float32(b["diffs"]))
        assert b["diffs"][0] == [entry["output_tgt"][k], entry["output_depth"][k]]          # the harness scored the same levels


def test_pp_run_scores_and_no_file_without_the_flag(tmp_path):
    from matryodshka_amd import harness
    n, d, ngf = 64, 8, 16
    _write_frames(tmp_path / "img", "room_1", n, n, 9, 4)
    cam = tmp_path / "cams.txt"
    cam.write_text("room_1 000 001 002 0.064 0.03\nroom_1 001 002 003 0.064 0.02\n")
    args = ["--cameras_glob", str(cam), "--image_dir", str(tmp_path / "img"), "--output_root", str(tmp_path / "o"), "--height", str(n),
            "--width", str(n), "--num_msi_planes", str(d), "--num_psv_planes", str(d), "--ngf", str(ngf), "--coord_net", "--input_type", "PP",
            "--test_outputs", "tgt_image"]
    assert harness.main(args + ["--experiment_name", "scored", "--score"]) == 2
    scores = json.loads((tmp_path / "o" / "scored" / "scores.json").read_text())
    _check_examples(tmp_path / "o", "scored", scores, ["room_1_000001002", "room_1_001002003"])
    # without --score: no scores.json, and the images are the same bytes
    assert harness.main(args + ["--experiment_name", "plain"]) == 2
    assert not (tmp_path / "o" / "plain" / "scores.json").exists()
    for e in scores["examples"]:
        for kind in ("output_tgt", "tgt_image"):
            f = "%s_%s.png" % (kind, e)
            assert (tmp_path / "o" / "plain" / e / f).read_bytes() == (tmp_path / "o" / "scored" / e / f).read_bytes(), f
