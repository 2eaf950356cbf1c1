"""The three facts that fix the convention of the ODS camera of render_views (include/msi_hip.h: msi_render_ods_views), held on
the composed CPU reference itself (tests/ods_views_reference.py) -- the GPU tests then hold the kernel to that reference and to
the same facts.  No device, no native library."""
import numpy as np
import pytest

from oracle import geometry as G
from tests.ods_views_reference import oracle_ods_view, smooth_image, swept_single_layer
from tests.test_gpu_render_views import _poses, oracle_view
from tests.util import random_rgba

F = np.float32


def _planes(d):
    return [float(x) for x in 1.0 / np.linspace(1.0 / 100.0, 1.0, d)]     # (MSI.inv_depths(1, 100, d): far -> near)


@pytest.mark.parametrize("size", [None, (20, 50)])
def test_fact_1_radius_zero_is_the_equirect_camera(size):
    h, w, d = 16, 32, 3
    rgba = random_rgba(5, 1, h, w, d)[0]
    pose, pos = _poses(6, 1, 2)
    for k in range(2):
        rgb, dep = oracle_ods_view(rgba, pose[0, k], pos[0, k], 0.0, _planes(d), size)
        r_e, d_e = oracle_view(rgba, pose[0, k], pos[0, k], _planes(d), 'equirect', size or (h, w))
        assert np.array_equal(rgb, r_e) and np.array_equal(dep, d_e)
    # (and a radius changes the image: the equality above is not vacuous)
    assert not np.array_equal(oracle_ods_view(rgba, pose[0, 0], pos[0, 0], 0.2, _planes(d), size)[0], r_e)


@pytest.mark.parametrize("order", [1, -1])
def test_fact_2_column_j_is_column_w_minus_1_minus_j_of_the_reference_render(order):
    h, w, d, baseline = 32, 64, 4, 0.064
    rgba = np.stack([np.concatenate([smooth_image(h, w) * F(0.9 - 0.1 * k), np.full((h, w, 1), F(0.3 + 0.1 * k))], axis=-1)
                     for k in range(d)], axis=2)                                        # [h,w,d,4], smooth
    jitter, _ = _poses(9, 1, 1, trans=0.05)
    jitter = jitter[0, 0]
    planes = _planes(d)
    intr = np.zeros((1, 3, 3), F)
    intr[0, 0, 0] = baseline
    layers = np.transpose(rgba, (2, 0, 1, 3))[:, None]                                  # [D,1,H,W,4]
    warped = G.projective_forward_ods(layers, order, intr, jitter[None], np.asarray(planes, F)[:, None])
    ref = G.over_composite([warped[k] for k in range(d)])[0]                             # [H,W,3]
    rgb, _ = oracle_ods_view(rgba, jitter, np.zeros(3, F), order * baseline, planes)
    err = np.abs(rgb.astype(np.float64) - ref[:, ::-1])
    print("fact 2, order %+d: max |ours - flipped reference| = %.3g" % (order, err.max()))
    assert err.max() <= 1e-4
    assert np.abs(rgb.astype(np.float64) - ref).max() > 0.05                             # (unflipped it is another image)


@pytest.mark.parametrize("order", [1, -1])
def test_fact_3_upright_and_the_eye_sign_is_the_sweeps(order):
    h, w = 32, 64
    image = smooth_image(h, w)
    rgba, planes = swept_single_layer(image, order)
    eye_pose, zero = np.eye(4, dtype=F), np.zeros(3, F)
    rows = slice(4, h - 4)
    good = np.abs(oracle_ods_view(rgba, eye_pose, zero, order * 0.2, planes)[0] - image)[rows]
    bad = np.abs(oracle_ods_view(rgba, eye_pose, zero, -order * 0.2, planes)[0] - image)[rows]
    print("fact 3, order %+d: right eye mean %.4f max %.4f; wrong eye mean %.4f" % (order, good.mean(), good.max(), bad.mean()))
    assert good.mean() <= 0.01
    assert bad.mean() >= 0.1
