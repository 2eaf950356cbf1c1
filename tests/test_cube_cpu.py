"""CPU-only checks of the cube-map conventions: the face table and pose helpers of matryodshka_amd.cubemap, and self-checks
of the fp64 reference tests/cube_reference.py that the GPU tests of MSI.cube_render_views / MSI.equirect_to_cube compare
against (the reference calls nothing of the package; these tests are what ties the two statements of the face table)."""
import numpy as np
import pytest

from matryodshka_amd import cubemap as C
from tests import cube_reference as ref

TABLE = {  # f: (looks along, x axis, y axis, z axis) in the cube frame (x right, y down, z forward)
    0: ((0, 0, 1), (1, 0, 0), (0, 1, 0), (0, 0, 1)),
    1: ((1, 0, 0), (0, 0, -1), (0, 1, 0), (1, 0, 0)),
    2: ((0, 0, -1), (-1, 0, 0), (0, 1, 0), (0, 0, -1)),
    3: ((-1, 0, 0), (0, 0, 1), (0, 1, 0), (-1, 0, 0)),
    4: ((0, -1, 0), (1, 0, 0), (0, 0, 1), (0, -1, 0)),
    5: ((0, 1, 0), (1, 0, 0), (0, 0, -1), (0, 1, 0)),
}


def _rot(ax, ang):
    ax = np.asarray(ax, np.float64) / np.linalg.norm(ax)
    k = np.array([[0, -ax[2], ax[1]], [ax[2], 0, -ax[0]], [-ax[1], ax[0], 0]])
    return np.eye(3) + np.sin(ang) * k + (1 - np.cos(ang)) * (k @ k)


def _pose(ax, ang, t):
    p = np.eye(4)
    p[:3, :3] = _rot(ax, ang)
    p[:3, 3] = t
    return p


def _random_cube(seed, s, d):
    rng = np.random.RandomState(seed)
    x = rng.uniform(-1, 1, size=(6, s, s, d, 4))
    x[..., 3] = rng.uniform(0.05, 0.95, size=(6, s, s, d))
    return x


# ------------------------------------------------------------------------------------------------------- the face table
def test_face_rotations_are_the_table():
    r = C.FACE_ROTATIONS
    assert r.shape == (6, 3, 3)
    for f, (look, x, y, z) in TABLE.items():
        assert np.array_equal(r[f][:, 0], x) and np.array_equal(r[f][:, 1], y) and np.array_equal(r[f][:, 2], z)
        assert np.array_equal(r[f] @ [0, 0, 1], look)
        assert np.array_equal(r[f] @ r[f].T, np.eye(3))
        assert np.linalg.det(r[f]) == pytest.approx(1.0, abs=0)
    assert np.array_equal(r, ref.R)                      # the reference's own statement of the table


def test_face_poses_is_the_conjugation():
    pose = _pose((0.3, -1.0, 0.2), 0.4, (0.1, -0.2, 0.05))
    fp = C.face_poses(pose)
    assert fp.shape == (6, 4, 4)
    for f in range(6):
        ff = np.eye(4)
        ff[:3, :3] = C.FACE_ROTATIONS[f]
        assert np.allclose(fp[f], ff.T @ pose @ ff, atol=1e-15)
    assert np.array_equal(fp[0], pose)
    assert np.array_equal(C.face_poses(np.eye(4)), np.tile(np.eye(4), (6, 1, 1)))
    batch = np.stack([pose, np.eye(4)]).astype(np.float32)
    out = C.face_poses(batch)
    assert out.shape == (2, 6, 4, 4) and out.dtype == np.float32
    assert np.allclose(out[0], fp, atol=1e-6) and np.array_equal(out[1], np.tile(np.eye(4, dtype=np.float32), (6, 1, 1)))


def test_face_poses_takes_torch_tensors():
    torch = pytest.importorskip("torch")
    pose = _pose((0.3, -1.0, 0.2), 0.4, (0.1, -0.2, 0.05))
    out = C.face_poses(torch.from_numpy(pose)[None])
    assert tuple(out.shape) == (1, 6, 4, 4)
    assert np.allclose(out.numpy()[0], C.face_poses(pose), atol=1e-15)


def test_face_view_helpers():
    k = C.default_face_intrinsics(16)
    assert np.array_equal(k, np.array([[8, 0, 8], [0, 8, 8], [0, 0, 1]], np.float32))
    kv = C.face_view_intrinsics(k)
    assert np.array_equal(kv, np.array([[8, 0, 8.5], [0, 8, 8.5], [0, 0, 1]], np.float32))
    swap = np.array([[0, 0, 1], [0, 1, 0], [1, 0, 0]], np.float64)
    for f in range(6):
        p = C.face_view_pose(f)
        assert p.dtype == np.float32 and np.array_equal(p[:3, 3], [0, 0, 0])
        # the render frame's forward axis (+x) goes to the face's viewing direction, written in the render frame
        assert np.array_equal(swap @ p[:3, :3].astype(np.float64) @ [1, 0, 0], TABLE[f][0])


# -------------------------------------------------------------------------------------------- the reference, checked alone
@pytest.mark.parametrize("f", range(6))
def test_reference_centre_view_lands_on_the_face_texels(f):
    """A pinhole view from the centre with face_view_pose(f) / face_view_intrinsics(K) at S x S is the plain per-texel
    over-composite of face f, for every pixel off the cube edges (margin > 1e-9)."""
    s, d = 16, 4
    cube = _random_cube(3, s, d)
    k = C.default_face_intrinsics(s)
    out = ref.render_view(cube, [100.0, 10.0, 3.0, 1.0], k, C.face_view_pose(f), (0, 0, 0), 'pinhole', (s, s),
                          C.face_view_intrinsics(k))
    rgb, dep = ref.over_composite(cube[f])
    keep = out["margin"] > 1e-9
    assert keep.mean() > 0.85                            # (column 0 and row 0 sit on the edges of a fx = cx = S/2 face)
    assert np.abs(out["rgb"] - rgb)[keep].max() <= 1e-12
    assert np.abs(out["depth"] - dep)[keep].max() <= 1e-12


@pytest.mark.parametrize("camera", ["equirect", "pinhole"])
def test_reference_constant_opaque_shell_renders_its_constant(camera):
    s, d = 12, 3
    cube = _random_cube(4, s, d)
    colour = np.array([0.25, -0.5, 0.75])
    cube[..., 1, :3] = colour
    cube[..., 1, 3] = 1.0
    cube[..., 2, 3] = 0.0
    k = C.default_face_intrinsics(s)
    kt = np.array([[9.0, 0, 10], [0, 9.0, 8], [0, 0, 1]])
    for pose, pos in ((np.eye(4), (0, 0, 0)), (_pose((1, 2, 3), 0.7, (0.3, -0.2, 0.4)), (0.2, 0.1, -0.3))):
        out = ref.render_view(cube, [50.0, 5.0, 1.0], k, pose, pos, camera, (16, 20), kt)
        assert np.abs(out["rgb"] - colour).max() <= 1e-12
        assert np.abs(out["depth"] - 1.0 / 3.0).max() <= 1e-12


def test_reference_equirect_to_cube_of_a_constant_is_the_constant():
    img = np.full((2, 9, 14, 3), 0.375)
    out = ref.equirect_to_cube(img, 8, C.default_face_intrinsics(8))
    assert out.shape == (2, 6, 8, 8, 3)
    assert np.abs(out - 0.375).max() <= 1e-15


def test_reference_round_trip_of_a_linear_panorama_within_the_bilinear_bound():
    """Panorama f(dir) = a . dir (|a| = 1, dir the unit ray of the lat-long grid) at H x W = 16 x 32 -> equirect_to_cube
    with symmetric faces (fx = cx = (S-1)/2, S = 32: texel centres span [-1, 1] in tan space, nothing is clamped in the
    render) -> one opaque shell rendered from the centre at 16 x 32.  Both passes are bilinear interpolations of f on a
    regular grid, each within sum over the two grid axes of step^2 / 8 max|f''| (the error of linear interpolation):
      pass 1, the panorama grid: steps 2 pi / W and pi / H in longitude and latitude; dir moves on circles of radius <= 1,
              so |f''| <= |a| on both axes:                     E1 = ((2 pi / W)^2 + (pi / H)^2) / 8
      pass 2, a face grid: step 2 / (S-1) in tan space; for n = d / |d|, d = d0 + x e, the second derivative has norm
              (2 sin t cos t + sin^2 t) / |d|^2 <= 1/2 + sqrt(5)/2 < 1.62 (t the angle between d and e, |d| >= 1):
                                                                E2 = 2 * 1.62 * (2 / (S-1))^2 / 8
    Interpolation is a convex combination, so pass 2 carries pass 1's error without growing it: |out - f| <= E1 + E2 =
    9.64e-3 + 1.69e-3.  The clamp in v holds the outermost panorama row over the half row beyond its centre, a FIRST-order
    error of up to |a| pi / (2 H) on face texels within pi / (2 H) of a pole; the taps of an output pixel lie within
    2 sqrt(2) / (S-1) rad of its ray, so only output rows 0 and H-1 (|lat| = 1.47 > pi/2 - pi/(2H) - 2 sqrt(2)/(S-1) = 1.38;
    row 1 is at 1.28) can touch them and get E1 + E2 + pi / (2 H)."""
    h, w, s = 16, 32, 32
    a = np.array([0.6, -0.48, 0.64])
    assert abs(np.linalg.norm(a) - 1) < 1e-12
    lon = -np.pi + (np.arange(w) + 0.5) * (2 * np.pi / w)
    lat = -np.pi / 2 + (np.arange(h) + 0.5) * (np.pi / h)
    lon, lat = np.meshgrid(lon, lat)
    pano = (a[0] * np.cos(lon) * np.cos(lat) + a[1] * np.sin(lat) + a[2] * np.sin(lon) * np.cos(lat))[None, :, :, None]
    k = np.array([[(s - 1) / 2, 0, (s - 1) / 2], [0, (s - 1) / 2, (s - 1) / 2], [0, 0, 1]])
    faces = ref.equirect_to_cube(np.repeat(pano, 3, axis=-1), s, k)[0]                   # [6,S,S,3]
    cube = np.concatenate([faces, np.ones((6, s, s, 1))], axis=-1)[:, :, :, None, :]    # one opaque shell
    out = ref.render_view(cube, [1.0], k, np.eye(4), (0, 0, 0), 'equirect', (h, w))
    assert not out["clamped"][out["margin"] > 1e-9].any()
    err = np.abs(out["rgb"][..., 0] - pano[0, :, :, 0])
    e1 = ((2 * np.pi / w) ** 2 + (np.pi / h) ** 2) / 8
    e2 = 2 * 1.62 * (2 / (s - 1)) ** 2 / 8
    print("round trip: interior rows %.3e (bound %.3e), polar rows %.3e (bound %.3e)"
          % (err[1:-1].max(), e1 + e2, err[[0, -1]].max(), e1 + e2 + np.pi / (2 * h)))
    assert err[1:-1].max() <= e1 + e2
    assert err[[0, -1]].max() <= e1 + e2 + np.pi / (2 * h)
