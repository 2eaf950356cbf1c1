"""The fp64 reference of the cube path's panorama sampling (tests/cube_sweep_reference.py) checked by itself, and the cases of the GPU tests
(tests/cube_sweep_cases.py) checked to mean something.  No GPU, no native call."""
import numpy as np
import pytest

from tests import cube_sweep_cases as cases
from tests import cube_sweep_reference as ref


def test_the_face_table_is_the_packages():
    from matryodshka_amd import cubemap
    assert np.array_equal(ref.R, cubemap.FACE_ROTATIONS)
    p = cases.source_poses()
    assert np.allclose(ref.face_poses(p), cubemap.face_poses(p.astype(np.float64)).reshape(-1, 4, 4), atol=0, rtol=0)
    # the appendix's RFACE: row f = the three axes = R_f transposed; R_f^T R_f = I
    for f in range(6):
        assert np.array_equal(ref.R[f].T @ ref.R[f], np.eye(3))


def _directions(hp, wp):
    """Cube-frame unit direction of every panorama pixel centre: lon = atan2(x, z), lat = asin(y)."""
    lon = (np.arange(wp) + 0.5) / wp * 2 * np.pi - np.pi
    lat = (np.arange(hp) + 0.5) / hp * np.pi - np.pi / 2
    lon, lat = np.meshgrid(lon, lat)
    return np.stack([np.sin(lon) * np.cos(lat), np.sin(lat), np.cos(lon) * np.cos(lat)], axis=-1)


# (a) ---------------------------------------------------------------------------------------------------------------------
def test_a_identity_pose_and_a_panorama_linear_in_the_angles_give_the_analytic_value():
    """P = I: Y = X, so face f's pixel (i, j) looks along R_f (S_j cx / fx, T_i cy / fy, 1) for every plane.  A panorama whose value is linear in
    its pixel coordinates -- i.e. in (lon, lat) -- is reproduced exactly by bilinear interpolation away from the wrap column and the clamped rows."""
    s, hp, wp = 10, 40, 80
    yy, xx = np.meshgrid(np.arange(hp, dtype=np.float64), np.arange(wp, dtype=np.float64), indexing='ij')
    pano = np.stack([0.01 * xx - 0.4, 0.02 * yy - 0.3, 0.005 * xx - 0.01 * yy], axis=-1)[None]
    k = cases.face_intrinsics(s, 6).astype(np.float64)
    k[:, 0, 0] *= 1.1                                   # (fx != cx: the divides matter)
    r = ref.cube_sweep(pano, np.tile(np.eye(4), (6, 1, 1)), k, (7.0, 2.0), s)
    g = ref.uv_grid(s)
    for f in range(6):
        q = np.stack(np.broadcast_arrays(g[None, :] * (k[f, 0, 2] / k[f, 0, 0]), g[:, None] * (k[f, 1, 2] / k[f, 1, 1]), 1.0), axis=-1)
        dcube = q @ ref.R[f].T
        lon = np.arctan2(dcube[..., 0], dcube[..., 2])
        lat = np.arcsin(dcube[..., 1] / np.linalg.norm(dcube, axis=-1))
        u, v = (lon + np.pi) / (2 * np.pi) * wp - 0.5, (lat + np.pi / 2) / np.pi * hp - 0.5
        ok = (u >= 0) & (u <= wp - 1) & (v >= 0) & (v <= hp - 1)
        assert ok.mean() > 0.8
        want = np.stack([0.01 * u - 0.4, 0.02 * v - 0.3, 0.005 * u - 0.01 * v], axis=-1)
        for d in range(2):                              # the same direction on every plane
            assert np.abs(r["value"][f, :, :, d] - want)[ok].max() < 1e-12
            assert np.abs(r["u"][f, :, :, d] - u).max() < 1e-9 and np.abs(r["v"][f, :, :, d] - v).max() < 1e-9


def test_a2_the_sampler_wraps_in_u_clamps_in_v_and_takes_nan_to_the_lower_bound():
    pano = np.arange(2 * 4 * 1, dtype=np.float64).reshape(2, 4, 1)          # rows (0 1 2 3), (4 5 6 7)
    at = lambda u, v: float(ref.bilinear_panorama(pano, np.array([u]), np.array([v]))[0, 0])
    assert at(-0.5, 0.0) == 0.5 * 3 + 0.5 * 0 and at(3.5, 0.0) == 0.5 * 3 + 0.5 * 0       # both ends meet across the seam
    assert at(-7.0, 0.0) == at(-0.5, 0.0) and at(9.0, 1.0) == 0.5 * 7 + 0.5 * 4           # clamped, then wrapped
    assert at(1.0, -3.0) == 1.0 and at(1.0, 5.0) == 5.0 and at(1.25, 0.5) == 0.5 * 1.25 + 0.5 * 5.25
    assert at(np.nan, np.nan) == at(-0.5, 0.0)


# (b) ---------------------------------------------------------------------------------------------------------------------
def test_b_past_the_border_a_sample_is_the_scene_along_its_own_direction():
    """A panorama that evaluates a smooth function g of direction, a translated (and turned) source: wherever the face position lies past the
    face's border, the sample is g(R_f Y) up to the interpolation error of the lat-long grid.  Bound: bilinear interpolation on a grid of pitch h
    is off by at most h^2 / 8 times the second derivative per axis; h = pi / 128, and along (lon, lat) the second derivatives of g below stay
    under 20 (|grad| <= 6 per component, frequencies <= 3), so 2 * (pi / 128)^2 / 8 * 20 = 3.0e-3.  Samples in the clamped polar half rows are
    left out (constant extrapolation there)."""
    hp, wp, s = 128, 256, 24
    g = lambda d: np.stack([np.sin(2.0 * d[..., 0]) * d[..., 2], np.cos(3.0 * d[..., 1]) + 0.5 * d[..., 0], d[..., 0] * d[..., 1] - d[..., 2] ** 2], axis=-1)
    pano = g(_directions(hp, wp))[None]
    src = np.eye(4)[None].copy()
    src[0, :3, :3] = cases.rotation((0.3, 1.0, -0.2), 12.0)
    src[0, :3, 3] = (0.3, 0.1, -0.2)
    fp, k, planes = ref.face_poses(src), cases.face_intrinsics(s, 6), (50.0, 4.0, 1.0)
    r = ref.cube_sweep(pano, fp, k, planes, s)
    y = ref.plane_points(fp, k, planes, s)
    dcube = np.einsum('nij,n...j->n...i', ref.R, y)
    dcube /= np.linalg.norm(dcube, axis=-1, keepdims=True)
    past = ref.outside_face(r, s) & (r["v"] >= 0) & (r["v"] <= hp - 1)
    assert past.mean() > 0.1 and all(past[f].any() for f in range(6))
    err = np.abs(r["value"] - g(dcube)).max(axis=-1)
    print("past the border: %d samples, max error %.2e" % (past.sum(), err[past].max()))
    assert err[past].max() < 3.0e-3
    # while the face-wise sweep of the cut faces is wrong there by a visible amount: the cut is made in fp64 from the same panorama
    from tests.cube_reference import equirect_to_cube
    faces = equirect_to_cube(pano, s, k[0])[0]
    old = np.abs(ref.face_sweep(faces, fp, k, planes) - g(dcube)).max(axis=-1)
    assert np.median(old[past]) > 30 * 3.0e-3


# (c) ---------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("name", sorted(cases.SHAPES))
def test_c_the_cases_reach_past_every_face_border(name):
    x, r = cases.case(name), cases.reference(name)
    out = ref.outside_face(r, x["size"])
    exc = ref.excluded(r)
    faces = np.arange(out.shape[0]) % 6
    print("%s: outside %.1f %%, pr2 <= 0: %d, excluded %.3f %%" % (name, 100 * out.mean(), int((r["pr2"] <= 0).sum()), 100 * exc.mean()))
    assert out.mean() >= 0.05
    for f in range(6):
        assert out[faces == f].any(), f
    assert exc.mean() <= 0.01
    assert np.isfinite(r["value"]).all() and np.abs(r["value"]).max() <= 1.0
    # the identity cube is there too: it reaches past the last row and column only
    assert 0 < out[:6].mean() < out[6:].mean()


def test_c_some_case_has_samples_behind_the_face_camera():
    assert any((cases.reference(name)["pr2"] <= 0).any() for name in cases.SHAPES)
