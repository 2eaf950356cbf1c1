"""FactoredLayers (matryodshka_amd/factored.py) without a device: the .npz round trip, the layout version, nbytes, its checks, the package
export that does not load the native library, and the harness's --hres_factored refusals and --help."""
import os
import subprocess
import sys

import numpy as np
import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def _factors(seed=3, b=2, h=4, w=6, hh=9, hw=14, d=4):
    from matryodshka_amd.factored import FactoredLayers
    rng = np.random.RandomState(seed)
    f32 = lambda *shape: rng.standard_normal(shape).astype(np.float32)
    planes = tuple(float(p) for p in 1.0 / np.linspace(0.01, 1.0, d))
    return FactoredLayers(f32(b, h, w, d), f32(b, h, w, d), f32(b, hh, hw, 3), f32(b, hh, hw, 3), f32(b, 4, 4), f32(b, 4, 4), f32(b, 3, 3), planes)


ARRAYS = ("blend_weights", "alphas", "ref_image", "src_image", "ref_pose", "src_pose", "intrinsics")


def test_shape_nbytes_and_planes():
    f = _factors()
    assert f.shape == (2, 9, 14, 4)
    assert f.nbytes == sum(getattr(f, a).numel() * 4 for a in ARRAYS) == 4 * (2 * (2 * 4 * 6 * 4) + 2 * (2 * 9 * 14 * 3) + 2 * 32 + 18)
    assert len(f.planes) == 4 and all(isinstance(p, float) for p in f.planes)
    g = f.to("cpu")
    assert g.shape == f.shape and g.planes == f.planes


def test_npz_round_trip_is_bit_exact(tmp_path):
    import torch
    f = _factors()
    f.blend_weights[0, 0, 0, 0] = -0.0                       # (bits, not values)
    f.alphas[0, 0, 0, 1] = float("nan")
    path = str(tmp_path / "f.npz")
    f.save(path)
    g = type(f).load(path)
    for a in ARRAYS:
        x, y = getattr(f, a), getattr(g, a)
        assert x.shape == y.shape and y.dtype == torch.float32 and torch.equal(x.view(torch.int32), y.view(torch.int32)), a
    assert g.planes == f.planes and g.shape == f.shape and g.nbytes == f.nbytes
    with np.load(path, allow_pickle=False) as z:
        assert int(z["factored_layout_version"]) == 1 and set(z.files) == set(ARRAYS) | {"planes", "factored_layout_version"}


def test_load_refuses_an_unknown_layout_version_and_other_files(tmp_path):
    from matryodshka_amd.factored import FactoredLayers
    f = _factors()
    path = str(tmp_path / "f.npz")
    f.save(path)
    with np.load(path) as z:
        items = {k: z[k] for k in z.files}
    items["factored_layout_version"] = np.int64(2)
    np.savez(str(tmp_path / "v2.npz"), **items)
    with pytest.raises(ValueError, match="layout version 2"):
        FactoredLayers.load(str(tmp_path / "v2.npz"))
    del items["factored_layout_version"]
    np.savez(str(tmp_path / "none.npz"), **items)
    with pytest.raises(ValueError, match="not a FactoredLayers file"):
        FactoredLayers.load(str(tmp_path / "none.npz"))
    items["factored_layout_version"] = np.int64(1)
    items["alphas"] = items["alphas"].astype(np.float16)
    np.savez(str(tmp_path / "half.npz"), **items)
    with pytest.raises(ValueError, match="alphas stored as float16"):
        FactoredLayers.load(str(tmp_path / "half.npz"))


def test_the_constructor_checks_its_pieces():
    from matryodshka_amd.factored import FactoredLayers
    f = _factors()
    a = [getattr(f, n) for n in ARRAYS]
    for k, bad, text in ((1, a[1][:, :3], "agree"), (3, a[3][:, :, :5], "agree"), (2, a[2][:1], "batch"), (4, a[4][:, :3], r"\[B,4,4\]"),
                         (6, a[6][:1], r"\[B,3,3\]"), (0, a[0].double(), "fp32")):
        args = list(a)
        args[k] = bad
        with pytest.raises(ValueError, match=text):
            FactoredLayers(*args, planes=f.planes)
    with pytest.raises(ValueError, match="planes"):
        FactoredLayers(*a, planes=f.planes[:3])


def test_the_package_exports_it_without_loading_the_library():
    code = ("import sys, matryodshka_amd; from matryodshka_amd import FactoredLayers; "
            "assert FactoredLayers.__module__ == 'matryodshka_amd.factored'; "
            "assert 'matryodshka_amd._native' not in sys.modules and 'matryodshka_amd.msi' not in sys.modules")
    assert subprocess.run([sys.executable, "-c", code], cwd=ROOT).returncode == 0


# ------------------------------------------------------------------------------------------------ the harness, without a device
def test_harness_help_names_the_flag(capsys):
    from matryodshka_amd import harness
    with pytest.raises(SystemExit) as e:
        harness.main(["--help"])
    assert e.value.code == 0
    out = " ".join(capsys.readouterr().out.split())
    assert "--hres_factored" in out and "msi_hres_factors_<dir>.npz" in out and "MSI.hres_factors" in out


@pytest.mark.parametrize("extra,text", [
    (["--hres_factored", "--test_type", "high_res", "--msi_format", "rgba8"], "materialised"),
    (["--hres_factored", "--test_type", "high_res_only", "--msi_format", "rgba16f", "--msi_hres_sparse"], "materialised"),
    (["--hres_factored"], "high_res"),
    (["--hres_factored", "--test_type", "on_video"], "high_res")])
def test_harness_refuses_hres_factored_where_it_cannot_apply(capsys, extra, text):
    """Argument errors come before the model is built: no device is needed."""
    from matryodshka_amd import harness
    with pytest.raises(SystemExit) as e:
        harness.main(["--cameras_glob", "none/*.txt"] + extra)
    assert e.value.code == 2
    err = capsys.readouterr().err
    assert "--hres_factored" in err and text in err
