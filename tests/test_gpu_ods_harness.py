"""harness --score --recon_score: both input eyes of every ODS sample are rendered back from its MSI (one MSI.render_ods_pair
launch), written as recon_ref_* / recon_src_* and scored on the device; the scores are the ones evaluate.py computes from the
written files against the written inputs.  Without the flag the run is today's: the same scores.json keys, no recon file.
The data set is the synthetic one of tests/test_gpu_score_harness.py, at its size (16 x 32, 4 planes, ngf 8).  SSIM and PSNR
agree to 1e-9 (fp64 on both sides, tests/test_gpu_score.py derives the bound)."""
import json

import numpy as np
import pytest

from tests.test_gpu_score_harness import _write_frames

pytestmark = pytest.mark.gpu

TOL = 1e-9
RECON_KEYS = ["recon_%s_%s" % (eye, k) for eye in ("ref", "src") for k in ("ssim", "psnr")]
TODAY = ["examples", "ssim", "psnr", "mean_ssim", "mean_psnr"]


def _args(tmp_path, name):
    h, w, d, ngf = 16, 32, 4, 8
    _write_frames(tmp_path / "img", "room_0", h, w, 7, 5)
    cam = tmp_path / "cams.txt"
    cam.write_text("".join("room_0 %.3d %.3d %.3d 0.032 %.3f -0.02 0.03\n" % (k, k + 1, k + 2, 0.01 * (k + 1)) for k in range(3)))
    return ["--cameras_glob", str(cam), "--image_dir", str(tmp_path / "img"), "--output_root", str(tmp_path / "o"),
            "--experiment_name", name, "--height", str(h), "--width", str(w), "--num_msi_planes", str(d),
            "--num_psv_planes", str(d), "--ngf", str(ngf), "--test_outputs", "tgt_image_ref_image_src_image"]


def test_recon_scores_equal_evaluate_on_the_written_files_and_nothing_changes_without_the_flag(tmp_path):
    from matryodshka_amd import evaluate as E
    from matryodshka_amd import harness
    assert harness.main(_args(tmp_path, "recon") + ["--score", "--recon_score"]) == 3
    assert harness.main(_args(tmp_path, "plain") + ["--score"]) == 3
    recon, plain = tmp_path / "o" / "recon", tmp_path / "o" / "plain"
    scores = json.loads((recon / "scores.json").read_text())
    names = ["room_0_%.3d%.3d%.3d" % (k, k + 1, k + 2) for k in range(3)]
    assert scores["examples"] == names
    assert sorted(scores) == sorted(TODAY + RECON_KEYS + ["mean_" + k for k in RECON_KEYS])
    for eye in ("ref", "src"):
        assert len(scores["recon_%s_ssim" % eye]) == len(scores["recon_%s_psnr" % eye]) == 3
        for k, e in enumerate(names):
            png = recon / e / ("recon_%s_%s.png" % (eye, e))
            assert png.exists()
            pred, tgt = E.load_image(str(png)), E.load_image(str(recon / e / ("%s_image_%s.png" % (eye, e))))
            assert pred.shape == tgt.shape == (16, 32, 3)
            ssim, psnr = E.ssim(pred, tgt, 255.0), E.psnr(pred, tgt, 255.0)
            print(e, eye, scores["recon_%s_ssim" % eye][k], ssim, scores["recon_%s_psnr" % eye][k], psnr)
            assert abs(scores["recon_%s_ssim" % eye][k] - ssim) <= TOL and abs(scores["recon_%s_psnr" % eye][k] - psnr) <= TOL
            assert np.isfinite(psnr)
        for k in ("ssim", "psnr"):
            assert abs(scores["mean_recon_%s_%s" % (eye, k)] - np.mean(scores["recon_%s_%s" % (eye, k)])) <= 1e-12
    # without the flag: exactly today's keys, the same numbers, no recon file, and every other file has the same bytes
    today = json.loads((plain / "scores.json").read_text())
    assert sorted(today) == sorted(TODAY)
    assert all(today[k] == scores[k] for k in TODAY)
    for e in names:
        assert not [f.name for f in (plain / e).iterdir() if f.name.startswith("recon_")]
        mine = sorted(f.name for f in (recon / e).iterdir() if not f.name.startswith("recon_"))
        assert mine == sorted(f.name for f in (plain / e).iterdir())
        for f in mine:
            assert (plain / e / f).read_bytes() == (recon / e / f).read_bytes(), f


def test_recon_score_alone_is_an_argparse_error(tmp_path, capsys):
    from matryodshka_amd import harness
    with pytest.raises(SystemExit) as exc:
        harness.main(_args(tmp_path, "alone") + ["--recon_score"])
    assert exc.value.code == 2
    assert "--recon_score needs --score" in capsys.readouterr().err
    assert not (tmp_path / "o" / "alone").exists()
