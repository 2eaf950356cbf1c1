"""CPU-only checks of the ODS camera of the cube-map viewer: the facts that fix the convention, held by the fp64 reference
tests/cube_ods_reference.py (which the GPU tests of MSI.cube_render_views(camera='ods') compare against), the precondition of the
GPU cases, and the host-side guards."""
import numpy as np
import pytest

from matryodshka_amd import cubemap as C
from tests import cube_ods_cases as cases
from tests import cube_ods_reference as oref
from tests import cube_reference as ref
from tests import cube_seamless_reference as sref
from tests.test_gpu_cube_views import _k_stack, _poses

EDGE = 1e-4      # the margin and the cap of tests/test_gpu_cube_views.py
CAP = 0.01


# ------------------------------------------------------------------------------------------- 1. e = 0 is the equirect camera
@pytest.mark.parametrize("size", cases.SIZES)
def test_1_radius_zero_is_the_equirect_reference_exactly(size):
    x, k = cases.stack(), _k_stack(cases.S)
    pose, pos = _poses(3)
    for b in range(cases.B):
        for v in range(3):
            for e in (0.0, -0.0):
                got = oref.render_view(x[6 * b:6 * b + 6], cases.PLANES, k, pose[b][v], pos[b][v], e, size)
                want = ref.render_view(x[6 * b:6 * b + 6], cases.PLANES, k, pose[b][v], pos[b][v], 'equirect', size)
                assert sorted(got) == sorted(want)
                for key in want:
                    assert np.array_equal(got[key], want[key]), (b, v, key)
            got = oref.render_view(x[6 * b:6 * b + 6], cases.PLANES, k, pose[b][v], pos[b][v], 0.0, size, seamless=True)
            want = sref.render_view(x[6 * b:6 * b + 6], cases.PLANES, k, pose[b][v], pos[b][v], 'equirect', size)
            for key in want:
                assert np.array_equal(got[key], want[key]), (b, v, key)
    assert ref.target_rays.__module__ == ref.__name__        # (the wrapper put the equirect ray builder back)


# ------------------------------------------------------------------------------------------------------------ 2. tangency
@pytest.mark.parametrize("e", [0.064, -0.064, 0.5])
def test_2_every_ray_is_tangent_to_the_viewing_circle(e):
    pose, pos = _poses(3)
    pose = pose.astype(np.float64)
    for b in range(cases.B):
        for v in range(3):
            # (the shared poses are rounded to fp32, orthonormal to 1e-7 only: the rotation is put back on SO(3) in fp64, where the property holds)
            u, _, vt = np.linalg.svd(pose[b][v][:3, :3])
            pose[b][v][:3, :3] = u @ vt
            o, r, head = oref.ods_rays((7, 13), pose[b][v], pos[b][v], e)
            off = o - head
            assert np.abs(np.einsum('...k,...k->...', off, r)).max() <= 1e-12
            assert np.abs(np.linalg.norm(off, axis=-1) - abs(e)).max() <= 1e-12
            o_eq, r_eq = ref.target_rays('equirect', (7, 13), pose[b][v], pos[b][v])
            assert np.array_equal(r, r_eq) and np.abs(head - o_eq).max() == 0     # the equirect camera's directions and head position
    # the formula itself, at identity: origin (render frame) = (tgt_pos[2] + sin S e, tgt_pos[1], tgt_pos[0] - cos S e)
    tp = np.array([0.1, -0.2, 0.3])
    o, r, head = oref.ods_rays((4, 8), np.eye(4), tp, e)
    lon = -np.pi + (np.arange(8) + 0.5) * (2 * np.pi / 8)
    want = np.stack([tp[2] + np.sin(lon) * e, np.full(8, tp[1]), tp[0] - np.cos(lon) * e], axis=-1)[:, ::-1]      # -> cube frame
    assert np.abs(o - want[None]).max() <= 1e-15


# ----------------------------------------------------------------------------------------- 3. parallax vanishes with distance
def test_3_parallax_vanishes_with_distance():
    """One opaque shell cut from a smooth function of the direction, half-side h.  The seamless filter renders it (the cube cut
    with the cube camera is continuous across the edges under that filter only: under the clamp filter a ray that changes face
    between the two cameras would step by a texel's worth of content, whatever h)."""
    s, size, e = 32, (12, 24), 0.064
    x, k = sref.analytic_cube(s), _k_stack(s)
    pose, pos = _poses(3)

    def error(h, p, tp):
        worst = 0.0
        for eye in (1.0, -1.0):
            got = oref.render_view(x, [h], k, p, tp, eye * e, size, seamless=True)["rgb"]
            want = sref.render_view(x, [h], k, p, tp, 'equirect', size)["rgb"]
            worst = max(worst, np.abs(got - want).max())
        return worst
    errs = {ratio: error(ratio * e, np.eye(4), np.zeros(3)) for ratio in (10.0, 1e2, 1e3, 1e4)}
    print("ODS vs equirect render of a smooth shell at h / e = 10, 1e2, 1e3, 1e4: %s" % ", ".join("%.3e" % errs[r] for r in sorted(errs)))
    assert errs[1e4] < errs[10.0] and errs[1e4] < 1e-3
    assert errs[10.0] > 1e-3                                   # (at h / e = 10 the parallax is there to see)
    assert errs[1e4] < errs[1e3] < errs[1e2] < errs[10.0]      # it converges
    assert error(1e4 * e, pose[0][1], pos[0][1]) < 1e-3        # the same with a turned, translated head inside the far shell


# --------------------------------------------------------------------------------------------------------- 4. eye symmetry
def _mirror_symmetric_cube(s, d, seed):
    """[6,S,S,D,4] whose content is symmetric under the render frame's right axis z -> -z, i.e. the cube frame's x -> -x: with the
    cube camera texel ix of a face sits at tan = 2 ix / S - 1, which has no mirror texel, so the symmetric camera fx = cx = (S-1)/2
    is used: x -> -x maps texel ix to S-1-ix on the front, back, up and down faces and swaps the right and left faces mirrored."""
    rng = np.random.RandomState(seed)
    x = rng.uniform(-1, 1, size=(6, s, s, d, 4))
    x[..., 3] = rng.uniform(0.05, 0.95, size=x.shape[:-1])
    for f in (0, 2, 4, 5):
        x[f] = 0.5 * (x[f] + x[f][:, ::-1])
    x[3] = x[1][:, ::-1]
    return x


def test_4_the_right_eye_is_the_left_eye_mirrored_for_mirror_symmetric_content():
    s, d, size, e = 16, 3, (12, 24), 0.064
    k = np.array([[(s - 1) / 2, 0, (s - 1) / 2], [0, (s - 1) / 2, (s - 1) / 2], [0, 0, 1]])
    x = _mirror_symmetric_cube(s, d, 5)
    # the content is what it claims: the equirect render from the centre is its own mirror image
    mono = ref.render_view(x, [10.0, 3.0, 1.0], k, np.eye(4), np.zeros(3), 'equirect', size)
    assert np.abs(mono["rgb"] - mono["rgb"][:, ::-1]).max() <= 1e-12
    left = oref.render_view(x, [10.0, 3.0, 1.0], k, np.eye(4), np.zeros(3), +e, size)
    right = oref.render_view(x, [10.0, 3.0, 1.0], k, np.eye(4), np.zeros(3), -e, size)
    keep = (left["margin"] >= EDGE) & (right["margin"][:, ::-1] >= EDGE)
    assert keep.mean() >= 1 - 2 * CAP
    assert np.abs(right["rgb"][:, ::-1] - left["rgb"])[keep].max() <= 1e-12
    assert np.abs(right["depth"][:, ::-1] - left["depth"])[keep].max() <= 1e-12
    # ... and the sign matters: the left eye is not its own mirror image, so swapping the eyes would show
    assert np.abs(left["rgb"][:, ::-1] - left["rgb"])[keep].max() > 1e-3
    # the sphere camera's sign: e > 0 (left eye) looking forward (+x of the render frame, +z of the cube frame) sits on the LEFT,
    # the render frame's -z = the cube frame's -x
    o4, r4, _ = oref.ods_rays((1, 4), np.eye(4), np.zeros(3), e)        # longitudes -3pi/4, -pi/4, pi/4, 3pi/4
    fwd = 0.5 * (o4[0, 1] + o4[0, 2])                                    # between the two columns around longitude 0
    assert fwd[0] < 0 and abs(fwd[2]) < 1e-15 and (r4[0, 1] + r4[0, 2])[2] > 0


# ------------------------------------------------------------------------------------------ 5. the GPU cases' exclusion cap
@pytest.mark.parametrize("views,size,seamless", cases.CASES)
def test_5_the_gpu_cases_exclude_at_most_one_percent_of_each_view(views, size, seamless):
    c = cases.case(views, size, seamless)
    excluded = (c["margin"] < EDGE).mean(axis=(2, 3))
    print("cube ODS %s -> %s %s: excluded %s" % (views, size, c["filtering"], np.round(excluded, 4)))
    assert excluded.shape == (cases.B, len(c["eye"]))
    assert (excluded <= CAP).all(), excluded
    assert (np.abs(c["rgb"]) <= 1).all() and (c["depth"] >= 0).all() and (c["depth"] <= 1).all()
    if seamless:
        assert (c["strip"] > 0).any()                          # some pixel reaches a virtual texel
    else:
        assert c["clamped"].any()
    # the viewing circles of the case lie inside the innermost shell: the host guard accepts them
    C.check_ods_circle_inside(c["pos"], c["pose"], c["planes"], c["radius"])


# ------------------------------------------------------------------------------------------------------ 6. the host guards
def test_6_the_circle_guard_accepts_just_below_the_innermost_shell_and_raises_from_equality_on():
    planes = [50.0, 10.0, 3.0, 1.5, 1.0]
    eye4 = np.eye(4)
    for e in (0.25, -0.25):
        C.check_ods_circle_inside([[0.0, 0.0, np.nextafter(0.75, 0)]], eye4[None], planes, [e])       # 0.75 - ulp + 0.25 < 1
        for at in (0.75, 0.8, 2.0):
            with pytest.raises(ValueError):
                C.check_ods_circle_inside([[0.0, 0.0, at]], eye4[None], planes, [e])
    # max_k |o_k|, not |o|: the corner direction is inside although its norm exceeds 1
    C.check_ods_circle_inside([[0.7, 0.7, 0.7]], eye4[None], planes, [0.25])
    # the POSED head position counts (rotation and translation), per view
    pose, pos = _poses(3)
    C.check_ods_circle_inside(pos, pose, planes, np.full((2, 3), 0.064))
    moved = pose.copy()
    head = pose[1, 2, :3, :3].astype(np.float64) @ pos[1, 2][::-1].astype(np.float64) + pose[1, 2, :3, 3]
    axis = int(np.argmax(np.abs(head)))
    moved[1, 2, axis, 3] += np.sign(head[axis]) * (0.96 - abs(head[axis]))       # that view's head to 0.96 along its largest axis
    with pytest.raises(ValueError):
        C.check_ods_circle_inside(pos, moved, planes, np.full((2, 3), 0.064))
    head = moved[1, 2, :3, :3].astype(np.float64) @ pos[1, 2][::-1].astype(np.float64) + moved[1, 2, :3, 3]
    assert np.abs(head).max() < 1.0 <= np.abs(head).max() + 0.064       # the head is inside, its circle is not
    C.check_origin_inside(pos, moved, planes)                            # (the equirect guard accepts that head)
    with pytest.raises(ValueError):
        C.check_ods_circle_inside([[0.0, 0.0, 0.0]], eye4[None], planes, [np.nan])
    with pytest.raises(ValueError):
        C.check_ods_circle_inside([[0.0, np.nan, 0.0]], eye4[None], planes, [0.064])


def test_6_camera_eye_and_baseline_are_checked_before_anything_touches_a_device():
    """cubemap.check_ods_arguments is the first thing MSI.cube_render_views does."""
    assert C.check_ods_arguments('ods', 1, 0.064) is True and C.check_ods_arguments('ods', 'left', 0.0) is True
    assert C.check_ods_arguments('equirect', None, None) is False and C.check_ods_arguments('pinhole', None, None) is False
    with pytest.raises(ValueError, match="baseline"):
        C.check_ods_arguments('ods', 1, None)
    with pytest.raises(ValueError, match="eye"):
        C.check_ods_arguments('ods', None, 0.064)
    for baseline in (-0.064, [0.064, -1e-9], np.inf, np.nan):
        with pytest.raises(ValueError, match="baseline"):
            C.check_ods_arguments('ods', 1, baseline)
    for camera in ('equirect', 'pinhole'):
        with pytest.raises(ValueError, match="camera='ods'"):
            C.check_ods_arguments(camera, 1, None)
        with pytest.raises(ValueError, match="camera='ods'"):
            C.check_ods_arguments(camera, None, 0.064)
    for camera in ('fisheye', None, 2):
        with pytest.raises(ValueError, match="camera must be"):
            C.check_ods_arguments(camera, None, None)
