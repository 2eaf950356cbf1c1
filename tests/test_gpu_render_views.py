"""MSI.render_views / msi_render_views_f32: V equirect or pinhole views of each MSI in one launch.

The CPU reference for the new cameras is composed here from the oracle's primitives (lat-long rays of any size, pinhole
rays, _transform_ray, _sphere_hit_pixels with the stack's (W, H), resample, over_composite[_depth]); the equirect camera
at the stack's own size is held bit for bit to the existing render.  Tolerances as test_gpu_geometry.py: max-abs 1e-3,
and the 99.99th percentile below 1e-4 where one flipped bilinear tap would show."""
import numpy as np
import pytest

from oracle import geometry as G
from tests.util import random_rgba

pytestmark = pytest.mark.gpu

F = np.float32
TOL = 1e-3


@pytest.fixture(scope="module")
def gpu():
    import torch
    assert torch.cuda.is_available(), "GPU tests need a HIP device"
    from matryodshka_amd import MSI
    return torch, MSI()


def _np(t):
    return t.detach().cpu().numpy()


def _rot(ax, ay, az):
    cx, sx, cy, sy, cz, sz = np.cos(ax), np.sin(ax), np.cos(ay), np.sin(ay), np.cos(az), np.sin(az)
    rx = np.array([[1, 0, 0], [0, cx, -sx], [0, sx, cx]])
    ry = np.array([[cy, 0, sy], [0, 1, 0], [-sy, 0, cy]])
    rz = np.array([[cz, -sz, 0], [sz, cz, 0], [0, 0, 1]])
    return rz @ ry @ rx


def _poses(seed, b, v, trans=0.1):
    """[B,V,4,4] rotated and translated poses and [B,V,3] target positions whose ray origins stay inside the unit sphere."""
    rng = np.random.RandomState(seed)
    pose = np.tile(np.eye(4, dtype=F), (b, v, 1, 1))
    for i in range(b):
        for k in range(v):
            pose[i, k, :3, :3] = _rot(*rng.uniform(-np.pi, np.pi, 3))
            pose[i, k, :3, 3] = rng.uniform(-trans, trans, 3)
    pos = rng.uniform(-trans, trans, size=(b, v, 3)).astype(F)
    return pose, pos


def _intrinsics(fx, fy, cx, cy):
    return np.array([[fx, 0, cx], [0, fy, cy], [0, 0, 1]], F)


def _rays(camera, oh, ow, K=None, rows=None):
    """Target rays before the pose, [len(rows), ow] each."""
    rows = np.arange(oh) if rows is None else np.asarray(rows)
    if camera == 'equirect':
        S, T = G.lat_long_grid((oh, ow))
        S, T = S[rows], T[rows]
        cosT = G.cos_f32(T)
        return G.cos_f32(S) * cosT, G.sin_f32(T), G.sin_f32(S) * cosT
    K = np.asarray(K, F)
    i = rows.astype(F)[:, None]
    j = np.arange(ow, dtype=F)[None, :]
    ry = ((i + F(0.5)) - K[1, 2]) / K[1, 1]
    rz = ((j + F(0.5)) - K[0, 2]) / K[0, 0]
    shape = (len(rows), ow)
    return np.ones(shape, F), np.broadcast_to(ry, shape).astype(F), np.broadcast_to(rz, shape).astype(F)


def oracle_view(rgba, pose, pos, planes, camera, size, K=None, rows=None):
    """One view of one stack: rgba [H,W,D,4]; pose [4,4]; pos [3] -> rgb [rows,w,3], depth [rows,w]."""
    h, w, d, _ = rgba.shape
    r = _rays(camera, size[0], size[1], K, rows)
    c = (F(pos[2]), F(pos[1]), F(pos[0]))
    r, c = G._transform_ray(r, c, pose)
    radius = np.asarray(planes, F).reshape(-1, 1, 1)
    pix = G._sphere_hit_pixels(r, c, radius, w, h)                   # [D,rows,w,2]
    layers = np.transpose(rgba, (2, 0, 1, 3))                         # [D,H,W,4]
    warped = G.resample(layers, pix)
    ws = [warped[k] for k in range(d)]
    return G.over_composite(ws), G.over_composite_depth(ws)[..., 0]


def _compare(got, ref, what):
    err = np.abs(got.astype(np.float64) - ref)
    assert err.max() <= TOL, (what, err.max())
    if err.size >= 100000:      # (on fewer values the 99.99th percentile is the maximum)
        assert np.percentile(err, 99.99) < 1e-4, (what, np.percentile(err, 99.99))


# 1 ---------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("h,w,d", [(32, 64, 4), (40, 80, 8), (30, 70, 5), (320, 640, 32)])
def test_equirect_is_bit_identical_to_the_single_view_render(gpu, h, w, d):
    torch, m = gpu
    b, v = 2, 3
    rgba = torch.from_numpy(random_rgba(31 + d, b, h, w, d)).cuda()
    pose, pos = _poses(7 + d, b, v)
    planes = m.inv_depths(1.0, 100.0, d)
    rgb, dep = m.render_views(rgba, pose, pos, planes)
    assert tuple(rgb.shape) == (b, v, h, w, 3) and tuple(dep.shape) == (b, v, h, w)
    for i in range(b):
        for k in range(v):
            r1, d1 = m.msi_render_equirect_view_and_depth(rgba[i:i + 1], pose[i, k][None], pos[i, k][None], planes, None)
            assert torch.equal(rgb[i, k], r1[0]), (i, k)
            assert torch.equal(dep[i, k], d1[0, ..., 0]), (i, k)
    # the single-output forms are the same numbers
    r_only, none = m.render_views(rgba, pose, pos, planes, want_depth=False)
    none2, d_only = m.render_views(rgba, pose, pos, planes, want_rgb=False)
    assert none is None and none2 is None
    assert torch.equal(r_only, rgb) and torch.equal(d_only, dep)


# 2 ---------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("h,w,d,oh,ow", [(32, 64, 4, 64, 128), (32, 64, 4, 50, 100), (320, 640, 32, 640, 1280)])
def test_equirect_at_other_sizes_matches_the_composed_oracle(gpu, h, w, d, oh, ow):
    torch, m = gpu
    b, v = 1, 2
    rgba = random_rgba(41, b, h, w, d)
    pose, pos = _poses(43, b, v)
    planes = m.inv_depths(1.0, 100.0, d)
    rgb, dep = m.render_views(torch.from_numpy(rgba).cuda(), pose, pos, planes, size=(oh, ow))
    assert tuple(rgb.shape) == (b, v, oh, ow, 3) and tuple(dep.shape) == (b, v, oh, ow)
    rgb, dep = _np(rgb), _np(dep)
    # (the full-size case against a stratified row set: poles, equator and rows in between -- the oracle is numpy)
    rows = np.arange(oh) if oh * ow <= 64 * 128 else np.unique(np.r_[0, 1, oh // 2 - 1, oh // 2, oh - 2, oh - 1,
                                                                     np.linspace(0, oh - 1, 24).astype(int)])
    for k in range(v):
        r_o, d_o = oracle_view(rgba[0], pose[0, k], pos[0, k], planes, 'equirect', (oh, ow), rows=rows)
        _compare(rgb[0, k][rows], r_o, ("rgb", k))
        _compare(dep[0, k][rows], d_o, ("depth", k))


# 3 ---------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("oh,ow", [(48, 64), (300, 347)])     # (the second: not a multiple of 64, 1e5 pixels a view)
def test_pinhole_matches_the_composed_oracle(gpu, oh, ow):
    torch, m = gpu
    b, v, h, w, d = 2, 3, 32, 64, 6
    rgba = random_rgba(51, b, h, w, d)
    pose, pos = _poses(53, b, v)
    planes = m.inv_depths(1.0, 100.0, d)
    # off-centre principal points, fx != fy, a different K per view
    K = np.stack([np.stack([_intrinsics(0.6 * ow * (1 + 0.3 * k), 0.45 * oh * (1 + 0.2 * i), ow * (0.5 + 0.07 * k), oh * (0.42 + 0.05 * i))
                            for k in range(v)]) for i in range(b)])
    rgb, dep = m.render_views(torch.from_numpy(rgba).cuda(), pose, pos, planes, camera='pinhole', intrinsics=K, size=(oh, ow))
    assert tuple(rgb.shape) == (b, v, oh, ow, 3) and tuple(dep.shape) == (b, v, oh, ow)
    rgb, dep = _np(rgb), _np(dep)
    for i in range(b):
        for k in range(v):
            r_o, d_o = oracle_view(rgba[i], pose[i, k], pos[i, k], planes, 'pinhole', (oh, ow), K[i, k])
            _compare(rgb[i, k], r_o, ("rgb", i, k))
            _compare(dep[i, k], d_o, ("depth", i, k))
    # one [3,3] K is shared by every view
    one = m.render_views(torch.from_numpy(rgba).cuda(), pose, pos, planes, camera='pinhole', intrinsics=K[0, 0], size=(oh, ow))[0]
    r_o, _ = oracle_view(rgba[1], pose[1, 2], pos[1, 2], planes, 'pinhole', (oh, ow), K[0, 0])
    _compare(_np(one)[1, 2], r_o, "shared K")


# 4 ---------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("vw", [0, 1, 3])
def test_pinhole_reproduces_the_reference_perspective_crop(gpu, vw):
    """K = [[w/4, 0, w/2], [0, h/2, h/2]] and pose = Ry(vw pi/2) @ M (M: x <- z, z <- -x) with the SAME tgt_pos give the
    rays of msi_render_perspective_view(viewing_window=vw) up to a positive scale."""
    torch, m = gpu
    b, h, w, d, ph, pw = 1, 32, 64, 5, 27, 48
    rgba = torch.from_numpy(random_rgba(22, b, h, w, d)).cuda()
    planes = m.inv_depths(1.0, 100.0, d)
    pos = np.array([[0.04, -0.03, 0.06]], F)
    crop = m.msi_render_perspective_view(rgba, np.eye(4, dtype=F)[None], pos, planes, None, viewing_window=vw,
                                         psp_height=ph, psp_width=pw)
    M = np.zeros((4, 4), F)
    M[0, 2], M[1, 1], M[2, 0], M[3, 3] = 1, 1, -1, 1
    pose = (m._crop_pose(vw).astype(np.float64) @ M).astype(F)
    K = _intrinsics(pw / 4.0, ph / 2.0, pw / 2.0, ph / 2.0)
    rgb, _ = m.render_views(rgba, pose[None, None], pos[None], planes, camera='pinhole', intrinsics=K, size=(ph, pw))
    assert torch.abs(rgb[0, 0] - crop[0]).max().item() <= TOL


# 5 ---------------------------------------------------------------------------------------------------------------------
def _full_stack(torch, alpha_fn):
    b, h, w, d = 1, 320, 640, 32
    col = torch.linspace(-1, 1, d).view(1, d, 1, 1, 1).expand(b, d, h, w, 3)
    return torch.cat([col, alpha_fn(b, d, h, w)], dim=-1).cuda().contiguous(), col[0, :, 0, 0, 0].tolist()


def _eight_heads(seed):
    pose, pos = _poses(seed, 1, 8, trans=0.05)
    K = _intrinsics(512.0, 512.0, 512.0, 512.0)
    return pose, pos, K


def test_pinhole_kat_constant_layers_at_1024(gpu):
    torch, m = gpu
    native, col = _full_stack(torch, lambda b, d, h, w: torch.full((b, d, h, w, 1), 0.25))
    planes = m.inv_depths(1.0, 100.0, 32)
    pose, pos, K = _eight_heads(61)
    rgb, dep = m.render_views(native.permute(0, 2, 3, 1, 4), pose, pos, planes, camera='pinhole', intrinsics=K, size=(1024, 1024))
    exp, exp_d = col[0], 0.0
    for i in range(1, 32):
        exp = col[i] * 0.25 + exp * 0.75
        exp_d = (i / 32.0) * 0.25 + exp_d * 0.75
    assert tuple(rgb.shape) == (1, 8, 1024, 1024, 3)
    assert torch.abs(rgb - exp).max().item() < 1e-5
    assert torch.abs(dep - exp_d).max().item() < 1e-5


def test_pinhole_kat_opaque_layer_at_1024(gpu):
    torch, m = gpu
    k = 13

    def alpha(b, d, h, w):
        a = torch.zeros((b, d, h, w, 1))
        a[:, k] = 1.0
        a[:, 0] = 0.37        # the farthest layer's alpha is ignored
        return a
    native, col = _full_stack(torch, alpha)
    planes = m.inv_depths(1.0, 100.0, 32)
    pose, pos, K = _eight_heads(62)
    rgb, dep = m.render_views(native.permute(0, 2, 3, 1, 4), pose, pos, planes, camera='pinhole', intrinsics=K, size=(1024, 1024))
    assert torch.abs(rgb - col[k]).max().item() < 1e-5
    assert torch.abs(dep - k / 32.0).max().item() < 1e-5


# 6 ---------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("camera", ["equirect", "pinhole"])
def test_views_and_samples_are_independent(gpu, camera):
    torch, m = gpu
    b, v, h, w, d = 2, 8, 40, 80, 8
    rgba = torch.from_numpy(random_rgba(71, b, h, w, d)).cuda()
    pose, pos = _poses(73, b, v)
    planes = m.inv_depths(1.0, 100.0, d)
    kw = dict(camera=camera, size=(36, 52))
    if camera == 'pinhole':
        kw['intrinsics'] = np.stack([np.stack([_intrinsics(30 + k, 24 + i, 25.5 - k, 17 + i) for k in range(v)]) for i in range(b)])
    rgb, dep = m.render_views(rgba, pose, pos, planes, **kw)
    for i in range(b):
        for k in range(v):
            one = dict(kw)
            if camera == 'pinhole':
                one['intrinsics'] = kw['intrinsics'][i, k]
            r1, d1 = m.render_views(rgba[i:i + 1], pose[i, k][None, None], pos[i, k][None, None], planes, **one)
            assert torch.equal(rgb[i, k], r1[0, 0]) and torch.equal(dep[i, k], d1[0, 0]), (i, k)
        alone = dict(kw)
        if camera == 'pinhole':
            alone['intrinsics'] = kw['intrinsics'][i]
        ra, da = m.render_views(rgba[i:i + 1], pose[i], pos[i], planes, **alone)      # ([V,4,4] / [V,3] for B = 1)
        assert torch.equal(rgb[i], ra[0]) and torch.equal(dep[i], da[0]), i


# 7 ---------------------------------------------------------------------------------------------------------------------
def test_one_stack_no_copies(gpu):
    torch, m = gpu
    b, v, h, w, d = 1, 16, 320, 640, 32
    native = torch.rand((b, d, h, w, 4), device="cuda")
    layers = native.permute(0, 2, 3, 1, 4)
    planes = m.inv_depths(1.0, 100.0, d)
    pose, pos = _poses(81, b, v, trans=0.05)
    m.render_views(layers, pose, pos, planes)              # warm-up: the trig table of the size is cached
    torch.cuda.synchronize()
    torch.cuda.reset_peak_memory_stats()
    base = torch.cuda.memory_allocated()
    rgb, dep = m.render_views(layers, pose, pos, planes)
    torch.cuda.synchronize()
    out_bytes = (rgb.numel() + dep.numel()) * 4
    assert torch.cuda.max_memory_allocated() - base <= out_bytes + (1 << 20)


# 8 ---------------------------------------------------------------------------------------------------------------------
def test_domain_host_device_and_clear(gpu):
    torch, m = gpu
    b, v, h, w, d = 1, 4, 16, 32, 4
    rgba = torch.from_numpy(random_rgba(91, b, h, w, d)).cuda()
    planes = m.inv_depths(1.0, 100.0, d)
    pose, pos = _poses(93, b, v, trans=0.05)
    m.render_status()                                      # (start from a clear word)
    m.render_views(rgba, pose, pos, planes)
    torch.cuda.synchronize()
    assert m.render_status() == 0                          # in-domain: the status stays clear
    bad = pose.copy()
    bad[0, 2, :3, 3] = [1.5, 0.0, 0.0]                     # one view's origin outside the innermost sphere (radius 1)
    with pytest.raises(ValueError):
        m.render_views(rgba, bad, pos, planes)
    K = _intrinsics(20.0, 20.0, 16.0, 8.0)
    with pytest.raises(ValueError):
        m.render_views(rgba, bad, pos, planes, camera='pinhole', intrinsics=K, size=(16, 32))
    # the same pose in device memory: no sync, no check at the call; the kernel flags it
    m.render_views(rgba, torch.from_numpy(bad).cuda(), pos, planes)
    with pytest.raises(ValueError):
        m.render_status()
    assert m.render_status() == 0                          # (render_status reset the word)
