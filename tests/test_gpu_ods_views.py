"""MSI.render_views(camera='ods') / MSI.render_ods_pair / msi_render_ods_views: both ODS eyes of each stack in one launch, from
fp32 or packed stacks, at any output size, rgb and depth.

The kernel is held to the composed CPU reference (tests/ods_views_reference.py) and to the three facts that fix its convention
(tests/test_ods_views_cpu.py holds the reference itself to them): radius 0 is the equirect camera bit for bit, column j is column
W-1-j of msi_render_ods_view, and the image is upright with the sweep's eye sign.  Tolerances as test_gpu_render_views.py: max-abs
1e-3, and the 99.99th percentile below 1e-4 over all values of a case once it has 100 000 of them."""
import numpy as np
import pytest

from tests.ods_views_reference import oracle_ods_view, smooth_image, swept_single_layer
from tests.test_gpu_render_views import _poses
from tests.util import random_rgba

pytestmark = pytest.mark.gpu

F = np.float32
TOL = 1e-3
FORMATS = [None, 'rgba8', 'rgba16f']      # None: the fp32 stack itself


@pytest.fixture(scope="module")
def gpu():
    import torch
    assert torch.cuda.is_available(), "GPU tests need a HIP device"
    from matryodshka_amd import MSI
    return torch, MSI()


def _np(t):
    return t.detach().cpu().numpy()


def _stack(torch, m, seed, b, h, w, d, fmt=None):
    rgba = torch.from_numpy(random_rgba(seed, b, h, w, d)).cuda()
    return rgba if fmt is None else m.pack_layers(rgba, fmt)


# 1 ---------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("fmt", FORMATS)
@pytest.mark.parametrize("size", [(30, 70), (50, 100)])
def test_radius_zero_is_bit_identical_to_the_equirect_camera(gpu, fmt, size):
    torch, m = gpu
    b, v, h, w, d = 2, 3, 30, 70, 5
    layers = _stack(torch, m, 11, b, h, w, d, fmt)
    pose, pos = _poses(13, b, v)
    planes = m.inv_depths(1.0, 100.0, d)
    rgb, dep = m.render_views(layers, pose, pos, planes, camera='ods', eye=np.array([1, -1, 1], F), baseline=0.0, size=size)
    r_e, d_e = m.render_views(layers, pose, pos, planes, camera='equirect', size=size)
    assert tuple(rgb.shape) == (b, v) + size + (3,) and tuple(dep.shape) == (b, v) + size
    assert torch.equal(rgb, r_e) and torch.equal(dep, d_e)


# 2 ---------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("h,w,d,oh,ow", [(32, 64, 4, 32, 64),
                                         (32, 64, 3, 50, 100),        # D below the four layer segments
                                         (30, 70, 5, 40, 130)])      # a row = two full 64-pixel blocks and a partial one
def test_matches_the_composed_reference(gpu, h, w, d, oh, ow):
    torch, m = gpu
    b, v = 2, 4
    rgba = random_rgba(21 + d, b, h, w, d)
    pose, pos = _poses(23 + d, b, v)                      # |origin| <= 0.2 sqrt(3) = 0.35; + 0.2 < 1
    planes = m.inv_depths(1.0, 100.0, d)
    eye = np.array([[1, -1, -1, 1], [-1, 1, 1, -1]], F)
    baseline = np.array([[0.032, 0.2, 0.0, 0.2], [0.2, 0.0, 0.032, 0.032]], F)
    rgb, dep = m.render_views(torch.from_numpy(rgba).cuda(), pose, pos, planes, camera='ods', eye=eye, baseline=baseline, size=(oh, ow))
    assert tuple(rgb.shape) == (b, v, oh, ow, 3) and tuple(dep.shape) == (b, v, oh, ow)
    assert m.render_status() == 0
    rgb, dep = _np(rgb), _np(dep)
    errs = []
    for i in range(b):
        for k in range(v):
            r_o, d_o = oracle_ods_view(rgba[i], pose[i, k], pos[i, k], eye[i, k] * baseline[i, k], planes, (oh, ow))
            errs += [np.abs(rgb[i, k].astype(np.float64) - r_o).ravel(), np.abs(dep[i, k].astype(np.float64) - d_o).ravel()]
    err = np.concatenate(errs)
    print("ods views %s -> %s: max %.3g, p99.99 %.3g over %d values" % ((h, w, d), (oh, ow), err.max(), np.percentile(err, 99.99), err.size))
    assert err.max() <= TOL
    if err.size >= 100000:
        assert np.percentile(err, 99.99) < 1e-4


# 3 ---------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("order", [1, -1])
def test_is_the_mirror_of_the_reference_single_view_ods_render(gpu, order):
    torch, m = gpu
    b, h, w, d = 2, 32, 64, 6
    rgba = torch.from_numpy(random_rgba(31, b, h, w, d)).cuda()
    jitter, _ = _poses(33, b, 1, trans=0.05)
    planes = m.inv_depths(1.0, 100.0, d)
    intr = np.zeros((b, 3, 3), F)
    intr[:, 0, 0] = [0.032, 0.1]
    ref = m.msi_render_ods_view(rgba, order, jitter[:, 0], np.zeros((b, 3), F), planes, intr)          # [B,H,W,3], mirrored
    rgb, _ = m.render_views(rgba, jitter, np.zeros((b, 1, 3), F), planes, camera='ods', eye=order, intrinsics=intr)
    err = torch.abs(rgb[:, 0] - torch.flip(ref, dims=[2])).max().item()
    print("against the flipped msi_render_ods_view, order %+d: max %.3g" % (order, err))
    assert err <= TOL
    assert torch.abs(rgb[:, 0] - ref).max().item() > 0.05         # (unflipped it is another image)


# 4 ---------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("order", [1, -1])
def test_upright_and_the_eye_sign_is_the_sweeps(gpu, order):
    torch, m = gpu
    h, w = 32, 64
    image = smooth_image(h, w)
    rgba, planes = swept_single_layer(image, order)
    layers = torch.from_numpy(rgba[None]).cuda()
    pose, pos = np.eye(4, dtype=F)[None, None], np.zeros((1, 1, 3), F)
    rows = slice(4, h - 4)
    good = np.abs(_np(m.render_views(layers, pose, pos, planes, camera='ods', eye=order, baseline=0.2)[0])[0, 0] - image)[rows]
    bad = np.abs(_np(m.render_views(layers, pose, pos, planes, camera='ods', eye=-order, baseline=0.2)[0])[0, 0] - image)[rows]
    print("order %+d: right eye mean %.4f max %.4f; wrong eye mean %.4f" % (order, good.mean(), good.max(), bad.mean()))
    assert good.mean() <= 0.01
    assert bad.mean() >= 0.1


# 5 ---------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("fmt", ['rgba8', 'rgba16f'])
def test_packed_is_bit_identical_to_unpacked(gpu, fmt):
    torch, m = gpu
    b, v, h, w, d = 2, 2, 30, 70, 5
    packed = _stack(torch, m, 41, b, h, w, d, fmt)
    pose, pos = _poses(43, b, v)
    planes = m.inv_depths(1.0, 100.0, d)
    kw = dict(camera='ods', eye=[1, -1], baseline=[0.064, 0.2], size=(40, 130))
    rgb, dep = m.render_views(packed, pose, pos, planes, **kw)
    r_u, d_u = m.render_views(m.unpack_layers(packed), pose, pos, planes, **kw)
    assert torch.equal(rgb, r_u) and torch.equal(dep, d_u)
    # planes=None: the planes the PackedLayers carries
    carried = m.pack_layers(m.unpack_layers(packed), fmt, planes=planes)
    assert torch.equal(m.render_views(carried, pose, pos, **kw)[0], rgb)


# 6 ---------------------------------------------------------------------------------------------------------------------
def test_forms_and_independence(gpu):
    torch, m = gpu
    b, v, h, w, d = 2, 4, 30, 70, 5
    rgba = _stack(torch, m, 51, b, h, w, d)
    pose, pos = _poses(53, b, v)
    planes = m.inv_depths(1.0, 100.0, d)
    eye = np.array([[1, -1, 1, -1], [-1, -1, 1, 1]], F)
    baseline = np.array([[0.032, 0.032, 0.2, 0.1], [0.1, 0.2, 0.0, 0.064]], F)
    kw = dict(camera='ods', size=(36, 75))
    rgb, dep = m.render_views(rgba, pose, pos, planes, eye=eye, baseline=baseline, **kw)
    r_only, none = m.render_views(rgba, pose, pos, planes, eye=eye, baseline=baseline, want_depth=False, **kw)
    none2, d_only = m.render_views(rgba, pose, pos, planes, eye=eye, baseline=baseline, want_rgb=False, **kw)
    assert none is None and none2 is None
    assert torch.equal(r_only, rgb) and torch.equal(d_only, dep)
    for i in range(b):
        for k in range(v):          # alone
            r1, d1 = m.render_views(rgba[i:i + 1], pose[i, k][None, None], pos[i, k][None, None], planes,
                                    eye=eye[i, k], baseline=float(baseline[i, k]), **kw)
            assert torch.equal(rgb[i, k], r1[0, 0]) and torch.equal(dep[i, k], d1[0, 0]), (i, k)
    # in another position of the batch: samples swapped, views reversed
    swap = np.array([1, 0])
    r2, d2 = m.render_views(rgba[[1, 0]], pose[swap][:, ::-1].copy(), pos[swap][:, ::-1].copy(), planes,
                            eye=eye[swap][:, ::-1].copy(), baseline=baseline[swap][:, ::-1].copy(), **kw)
    assert torch.equal(torch.flip(r2, dims=[0, 1]), rgb) and torch.equal(torch.flip(d2, dims=[0, 1]), dep)


# 7 ---------------------------------------------------------------------------------------------------------------------
def test_status_host_device_partial_circle_and_nan(gpu):
    torch, m = gpu
    b, v, h, w, d = 1, 2, 16, 32, 4
    rgba = _stack(torch, m, 61, b, h, w, d)
    planes = m.inv_depths(1.0, 100.0, d)                  # innermost sphere: radius 1
    pose = np.tile(np.eye(4, dtype=F), (b, v, 1, 1))
    pos = np.zeros((b, v, 3), F)
    m.render_status()                                      # (start from a clear word)
    m.render_views(rgba, pose, pos, planes, camera='ods', eye=[1, -1], baseline=0.2)
    assert m.render_status() == 0
    # host inputs: |origin| + |e| >= 1 raises -- through tgt_pos, through the pose's translation, through the radius alone
    off = pos.copy()
    off[0, 1] = [0.0, 0.0, 0.9]
    with pytest.raises(ValueError):
        m.render_views(rgba, pose, off, planes, camera='ods', eye=[1, -1], baseline=0.2)
    moved = pose.copy()
    moved[0, 0, :3, 3] = [0.0, 0.85, 0.0]
    with pytest.raises(ValueError):
        m.render_views(rgba, moved, pos, planes, camera='ods', eye=[1, -1], baseline=0.2)
    with pytest.raises(ValueError):
        m.render_views(rgba, pose, pos, planes, camera='ods', eye=[1, -1], baseline=1.0)
    m.render_views(rgba, pose, off, planes, camera='ods', eye=[1, -1], baseline=0.05)       # 0.95 < 1: fine
    assert m.render_status() == 0
    # device inputs, head offset 0.9 and baseline 0.2: the circle spans |c| in [0.7, 1.1] -- only a part of it is outside, and
    # the column of lane 0 of the one wave of a row (S = -pi + pi/W: the origin at about (0.9 - 0, ., 0.2)) is INSIDE
    rgb, dep = m.render_views(rgba, pose, torch.from_numpy(off).cuda(), planes, camera='ods', eye=[1, -1], baseline=0.2)
    assert bool(torch.isfinite(rgb).all()) and bool(torch.isfinite(dep).all())
    with pytest.raises(ValueError):
        m.render_status()
    assert m.render_status() == 0                          # (render_status reset the word)
    m.render_views(rgba, pose, torch.from_numpy(pos).cuda(), planes, camera='ods', eye=[1, -1], baseline=0.2)
    assert m.render_status() == 0                          # the next in-domain call leaves it clear
    nan = pos.copy()
    nan[0, 0, 1] = np.nan
    m.render_views(rgba, pose, torch.from_numpy(nan).cuda(), planes, camera='ods', eye=[1, -1], baseline=0.2)
    with pytest.raises(ValueError):
        m.render_status()
    assert m.render_status() == 0


# 8 ---------------------------------------------------------------------------------------------------------------------
def test_render_ods_pair(gpu):
    torch, m = gpu
    b, h, w, d = 2, 30, 70, 5
    rgba = _stack(torch, m, 71, b, h, w, d)
    planes = m.inv_depths(1.0, 100.0, d)
    pose, pos = _poses(73, b, 1)
    intr = np.zeros((b, 3, 3), F)
    intr[:, 0, 0] = [0.032, 0.1]
    size = (20, 50)
    views, vdep = m.render_ods_pair(rgba, planes, intrinsics=intr, tgt_pose_rt=pose[:, 0], tgt_pos=pos[:, 0], size=size, want_depth=True)
    assert tuple(views.shape) == (b, 2) + size + (3,) and tuple(vdep.shape) == (b, 2) + size
    r2, d2 = m.render_views(rgba, np.repeat(pose, 2, axis=1), np.repeat(pos, 2, axis=1), planes, camera='ods', eye=[1, -1],
                            baseline=intr[:, 0, 0], size=size)
    assert torch.equal(views, r2) and torch.equal(vdep, d2)
    only = m.render_ods_pair(rgba, planes, intrinsics=intr, tgt_pose_rt=pose[:, 0], tgt_pos=pos[:, 0], size=size)
    assert torch.is_tensor(only) and torch.equal(only, views)
    tb, tbd = m.render_ods_pair(rgba, planes, intrinsics=intr, tgt_pose_rt=pose[:, 0], tgt_pos=pos[:, 0], size=size, want_depth=True,
                                layout='top_bottom')
    assert tuple(tb.shape) == (b, 2 * size[0], size[1], 3) and tuple(tbd.shape) == (b, 2 * size[0], size[1])
    assert torch.equal(tb[:, :size[0]], views[:, 0]) and torch.equal(tb[:, size[0]:], views[:, 1])       # rows [0,h): the left eye
    assert torch.equal(tbd[:, :size[0]], vdep[:, 0])
    # top_bottom is a view of the [B,2,h,w,3] tensor the launch wrote: the same storage, no copy
    assert tb._base is not None and tuple(tb._base.shape) == tuple(views.shape)
    assert tb.data_ptr() == tb._base.data_ptr() and tbd.data_ptr() == tbd._base.data_ptr()
    assert torch.equal(tb._base, views)
    # defaults: identity pose, position 0, the stack's size, a float baseline
    dflt = m.render_ods_pair(rgba, planes, baseline=0.064)
    eye4 = np.tile(np.eye(4, dtype=F), (b, 2, 1, 1))
    r3, _ = m.render_views(rgba, eye4, np.zeros((b, 2, 3), F), planes, camera='ods', eye='left', baseline=0.064)
    assert tuple(dflt.shape) == (b, 2, h, w, 3) and torch.equal(dflt[:, 0], r3[:, 0])
    with pytest.raises(ValueError):
        m.render_ods_pair(rgba, planes, baseline=0.064, layout='side_by_side')


# 9 ---------------------------------------------------------------------------------------------------------------------
def test_python_argument_errors(gpu):
    torch, m = gpu
    b, v, h, w, d = 2, 2, 16, 32, 4
    rgba = _stack(torch, m, 81, b, h, w, d)
    planes = m.inv_depths(1.0, 100.0, d)
    pose, pos = _poses(83, b, v)
    intr = np.zeros((b, 3, 3), F)
    intr[:, 0, 0] = 0.032
    ok = dict(camera='ods', eye=1, baseline=0.032)
    m.render_views(rgba, pose, pos, planes, **ok)
    m.render_views(rgba, pose, pos, planes, camera='ods', eye='right', intrinsics=intr[:1])            # [1,3,3]
    bad = [dict(camera='ods', baseline=0.032),                                   # eye missing
           dict(camera='ods', eye=2, baseline=0.032), dict(camera='ods', eye=0, baseline=0.032),
           dict(camera='ods', eye=[1, 0.5], baseline=0.032), dict(camera='ods', eye='both', baseline=0.032),
           dict(camera='ods', eye=1, baseline=-0.032), dict(camera='ods', eye=1, baseline=float('nan')),
           dict(camera='ods', eye=1, baseline=float('inf')), dict(camera='ods', eye=1, baseline=[0.1, -0.1]),
           dict(camera='ods', eye=[1, -1, 1], baseline=0.032),                   # eye [3] with V = 2
           dict(camera='ods', eye=np.ones((3, 2), F), baseline=0.032),           # eye [3,2] with B = 2
           dict(camera='ods', eye=1, baseline=[0.1, 0.1, 0.1]),                  # baseline [3] with B = 2
           dict(camera='ods', eye=1, baseline=np.full((2, 3), 0.1, F)),
           dict(camera='ods', eye=1),                                            # neither baseline nor intrinsics
           dict(camera='ods', eye=1, intrinsics=np.zeros((3, 3, 3), F)),         # intrinsics [3,3,3] with B = 2
           dict(camera='ods', eye=1, intrinsics=np.zeros((b, 4, 4), F)),
           dict(camera='equirect', eye=1), dict(camera='equirect', baseline=0.032),
           dict(camera='pinhole', eye=1, intrinsics=np.eye(3, dtype=F), size=(8, 8)),
           dict(camera='fisheye')]
    for kw in bad:
        with pytest.raises(ValueError):
            m.render_views(rgba, pose, pos, planes, **kw)
    with pytest.raises(ValueError):
        m.render_views(rgba, pose, pos, planes, want_rgb=False, want_depth=False, **ok)
    with pytest.raises(ValueError):
        m.cube_render_views(torch.zeros((6, 8, 8, 2, 4), device="cuda"), np.eye(4, dtype=F)[None, None], np.zeros((1, 1, 3), F),
                            [2.0, 1.0], camera='ods', size=(8, 16))              # the cube viewer has no ODS camera
    assert m.render_status() == 0
