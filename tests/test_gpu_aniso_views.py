"""MSI.render_views / MSI.render_ods_pair on a MipLayers with max_anisotropy > 1 (msi_render_views_aniso): the anisotropic texel for
the three cameras, the three output modes and the three texel formats.

(a) against the fp64 statement of the rule (tests/aniso_reference.py) at the project's render gate, max-abs <= 1e-3 on rgb and
    depth, no pixel excluded (the rule is continuous), on views whose footprints near the stack's poles run through every sample
    count up to the cap's;
(b) the bit-for-bit facts: max_anisotropy = 1 is today's render; a view that minifies nothing, and lod_bias = -64, have the plain
    render's bits; a packed pyramid renders == to its unpacked levels; render_ods_pair is the two single views; the status word is
    the plain render's;
(c) on the device as on the reference, a tilted view is closer to the supersampled view than the trilinear render."""
import numpy as np
import pytest

from matryodshka_amd.mips import MipLayers
from matryodshka_amd.packed import decode_np
from tests import aniso_reference as A
from tests import mip_reference as R
from tests.test_aniso_cpu import rms, tilt
from tests.test_gpu_render_views import _intrinsics, _rot
from tests.util import random_rgba

pytestmark = pytest.mark.gpu

F = np.float32
TOL = 1e-3
B, V = 2, 2
CAMERAS = ['equirect', 'pinhole', 'ods']
MODES = [(True, True), (True, False), (False, True)]
CAPS = [2.0, 8.0, 16.0]
# (height, width, layers, levels, format): D = 3 and D = 5 straddle the four layer segments
STACKS = [(16, 32, 3, 3, 'f32'), (24, 40, 5, 4, 'rgba8'), (64, 128, 4, 4, 'rgba16f'), (64, 128, 4, 4, 'f32')]
QUALITY_PLANES = [100.0, 3.0, 1.5, 1.0]


@pytest.fixture(scope="module")
def gpu():
    import torch
    assert torch.cuda.is_available(), "GPU tests need a HIP device"
    from matryodshka_amd import MSI
    return torch, MSI()


def _np(t):
    return None if t is None else t.detach().cpu().numpy()


def _status(m):
    bits = int(m._render_status.item())
    m._render_status.zero_()
    return bits


def _stack_np(h, w, d):
    """[B,H,W,D,4] fp32: smooth noise for the small stacks, near-Nyquist content (tests/mip_reference.py) at 64 x 128."""
    if (h, w) == (64, 128):
        return np.stack([R.near_nyquist_stack(3 + i, h, w, d) for i in range(B)]).transpose(0, 2, 3, 1, 4).copy()
    return random_rgba(100 + h, B, h, w, d)


def _mip(torch, m, h, w, d, levels, fmt, planes):
    rgba = torch.from_numpy(_stack_np(h, w, d)).cuda()
    return m.build_mips(rgba if fmt == 'f32' else m.pack_layers(rgba, fmt), levels, planes)


def _plain(torch, mip):
    """What render_views takes for the plain render of a MipLayers' level 0."""
    return mip.base.permute(0, 2, 3, 1, 4) if torch.is_tensor(mip.base) else mip.base


def _levels_np(mip):
    """[level 0, ..] of a MipLayers as decoded numpy arrays [B,D,h,w,4]."""
    out = []
    for l in range(mip.levels):
        lv = mip.level(l)
        out.append(lv.cpu().numpy() if mip.format == 'f32' else decode_np(lv.data.cpu().numpy(), mip.format))
    return out


def _views(camera):
    """Poses [B,V,4,4] and positions [B,V,3]: the view's poles turned away from the stack's by 90 and by 60 degrees, each centred
    and translated.  The equirect cameras roll about the forward axis (the stack's poles come to lie on the view's equator); the
    pinhole camera turns its forward axis onto the stack's pole (90 degrees) and 30 degrees short of it."""
    pose = np.tile(np.eye(4, dtype=F), (B, V, 1, 1))
    for k, deg in enumerate((90.0, 60.0)):
        rot = _rot(0.0, 0.0, np.deg2rad(deg)).astype(F) if camera == 'pinhole' else tilt(deg)[:3, :3]
        pose[:, k, :3, :3] = rot
    pos = np.zeros((B, V, 3), F)
    pos[0, 1] = pos[1, 0] = (0.3, -0.2, 0.25)          # sample 0: 90 centred, 60 translated; sample 1: 90 translated, 60 centred
    return pose, pos


def _sizes(camera):
    return [(24, 24)] if camera == 'pinhole' else [(7, 13), (16, 32), (1, 9), (9, 1)]    # none a multiple of 64: partial wavefronts


def _camera_args(camera, size):
    oh, ow = size
    if camera == 'pinhole':      # a wide field of view: tan(half angle) = 2
        return dict(camera='pinhole', size=size, intrinsics=_intrinsics(ow / 4.0, ow / 4.0, ow / 2.0, oh / 2.0))
    if camera == 'ods':          # both eyes among the views
        return dict(camera='ods', size=size, eye=np.array([1, -1], F), baseline=0.03)
    return dict(camera='equirect', size=size)


def _reference(lv, planes, camera, size, cap, pose, pos, kw, lod_bias=0.0):
    """The fp64 views [B][V] -> (rgb, depth, ratio, lambda) each."""
    out = []
    for i in range(B):
        row = []
        for k in range(V):
            e = None if camera != 'ods' else kw['eye'][k] * kw['baseline']
            K = kw.get('intrinsics') if camera == 'pinhole' else None
            row.append(A.aniso_view([x[i] for x in lv], pose[i, k], pos[i, k], planes, camera, size, K=K, e=e, lod_bias=lod_bias,
                                    max_anisotropy=cap, details=True))
        out.append(row)
    return out


# (a) ---------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("camera", CAMERAS)
@pytest.mark.parametrize("h,w,d,levels,fmt", STACKS)
def test_matches_the_fp64_reference(gpu, h, w, d, levels, fmt, camera):
    """Every stack x camera; per case the outputs 7 x 13, 16 x 32, 1 x 9 and 9 x 1 (the pinhole camera: a 24 x 24 eye), the caps 2, 8
    and 16, B = V = 2 views tilted by 90 and 60 degrees, centred and translated, and all three output modes.  On the reference:
    every (size, cap) has a (layer, pixel) with ratio > 1.5, and with the cap 16 some pixel of the case reaches M = 8, the end of the
    sample loop.  Gate: max-abs <= 1e-3 on rgb and on depth, every pixel.
    Measured on an MI355X, the maxima over all cases: rgb 9.5e-6 (pinhole, 64 x 128 fp32 and rgba16f), depth 1.5e-6 (pinhole, 24 x 40
    rgba8); per stack and camera the rgb maxima are 1.1e-6 .. 2.1e-6 at 16 x 32 and 24 x 40 and 6.2e-6 .. 9.5e-6 at 64 x 128, whose
    near-Nyquist content turns a coordinate error into the largest colour error ("Anisotropic filtering")."""
    torch, m = gpu
    planes = m.inv_depths(1.0, 100.0, d)
    mip = _mip(torch, m, h, w, d, levels, fmt, planes)
    assert mip.levels == levels and mip.format == fmt
    lv = _levels_np(mip)
    pose, pos = _views(camera)
    worst, most_m = {}, 0
    _status(m)
    for size in _sizes(camera):
        kw = _camera_args(camera, size)
        for cap in CAPS:
            ref = _reference(lv, planes, camera, size, cap, pose, pos, kw)
            top = max(float(ref[i][k][2].max()) for i in range(B) for k in range(V))
            assert top > 1.5, (size, cap, top)
            if cap == 16.0:
                most_m = max(most_m, max(int(A.sample_count(ref[i][k][2]).max()) for i in range(B) for k in range(V)))
            for want_rgb, want_depth in MODES:
                rgb, dep = m.render_views(mip, pose, pos, max_anisotropy=cap, want_rgb=want_rgb, want_depth=want_depth, **kw)
                assert _status(m) == 0
                assert (rgb is None) == (not want_rgb) and (dep is None) == (not want_depth)
                er = ed = 0.0
                if want_rgb:
                    assert tuple(rgb.shape) == (B, V) + size + (3,)
                    rgb = _np(rgb).astype(np.float64)
                    er = max(float(np.abs(rgb[i, k] - ref[i][k][0]).max()) for i in range(B) for k in range(V))
                if want_depth:
                    assert tuple(dep.shape) == (B, V) + size
                    dep = _np(dep).astype(np.float64)
                    ed = max(float(np.abs(dep[i, k] - ref[i][k][1]).max()) for i in range(B) for k in range(V))
                w0 = worst.get((size, cap), (0.0, 0.0))
                worst[(size, cap)] = (max(w0[0], er), max(w0[1], ed))
    for key in sorted(worst):
        print("aniso views %s %dx%dx%d %s -> %s cap %g: max rgb %.3g depth %.3g" % ((camera, h, w, d, fmt) + key + worst[key]))
    assert most_m == 8, most_m
    for key, (er, ed) in worst.items():
        assert er <= TOL and ed <= TOL, (key, er, ed)


# (b) ---------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("camera", CAMERAS)
def test_cap_1_is_todays_render(gpu, camera):
    torch, m = gpu
    planes = m.inv_depths(1.0, 100.0, 5)
    mip = _mip(torch, m, 24, 40, 5, 4, 'rgba8', planes)
    pose, pos = _views(camera)
    for size in _sizes(camera):
        kw = _camera_args(camera, size)
        for bias in (0.0, 0.5):
            a = m.render_views(mip, pose, pos, lod_bias=bias, **kw)
            b = m.render_views(mip, pose, pos, lod_bias=bias, max_anisotropy=1.0, **kw)
            assert torch.equal(a[0], b[0]) and torch.equal(a[1], b[1]), (size, bias)


@pytest.mark.parametrize("fmt", ['f32', 'rgba8', 'rgba16f'])
@pytest.mark.parametrize("camera", CAMERAS)
def test_nothing_minified_and_bias_minus_64_have_the_plain_renders_bits(gpu, camera, fmt):
    """A view with sigma_max <= 1 on every layer -- the identity pose at twice the stack's size, a pinhole eye with a long focal
    length -- for any cap, and any view with lod_bias = -64: every output element and the status word equal
    the plain render of .base, in all three modes."""
    torch, m = gpu
    h, w, d = 16, 32, 5
    planes = m.inv_depths(1.0, 100.0, d)
    mip = _mip(torch, m, h, w, d, 3, fmt, planes)
    ident = np.tile(np.eye(4, dtype=F), (B, V, 1, 1))
    zero = np.zeros((B, V, 3), F)
    tilted = _views(camera)
    if camera == 'pinhole':      # 70 x 70 pixels of focal length 400: 0.0025 rad per pixel against the stack's 0.196 rad per texel
        magnified = dict(camera='pinhole', size=(9, 70), intrinsics=_intrinsics(400.0, 400.0, 35.0, 4.5))
    elif camera == 'ods':
        # (a small circle: next to a pole the hits of an ODS eye twist about the axis by baseline / distance, and with it du_y grows)
        magnified = dict(camera='ods', size=(2 * h, 2 * w + 6), eye=np.array([1, -1], F), baseline=0.001)
    else:
        magnified = dict(camera='equirect', size=(2 * h, 2 * w + 6))
    for view in _reference(_levels_np(mip), planes, camera, magnified['size'], 16.0, ident, zero, magnified)[0]:     # the premise, on the reference
        assert np.all(view[2] == 1.0) and np.all(view[3] == 0.0)
    _status(m)
    for (pose, pos), kw, bias in ((((ident, zero)), magnified, 0.0), (tilted, _camera_args(camera, _sizes(camera)[0]), -64.0)):
        for want_rgb, want_depth in MODES:
            ref = m.render_views(_plain(torch, mip), pose, pos, planes, want_rgb=want_rgb, want_depth=want_depth, **kw)
            assert _status(m) == 0
            for cap in (2.0, 16.0):
                got = m.render_views(mip, pose, pos, want_rgb=want_rgb, want_depth=want_depth, lod_bias=bias, max_anisotropy=cap, **kw)
                assert _status(m) == 0
                for g, r in zip(got, ref):
                    assert (g is None) == (r is None)
                    if g is not None:
                        assert g.shape == r.shape and torch.equal(g, r), (kw['size'], want_rgb, want_depth, bias, cap)


@pytest.mark.parametrize("fmt", ['rgba8', 'rgba16f'])
@pytest.mark.parametrize("camera", CAMERAS)
def test_a_packed_pyramid_renders_as_its_unpacked_levels(gpu, camera, fmt):
    torch, m = gpu
    planes = m.inv_depths(1.0, 100.0, 5)
    mip = _mip(torch, m, 24, 40, 5, 3, fmt, planes)
    pose, pos = _views(camera)

    def native(packed):
        return m.unpack_layers(packed).permute(0, 3, 1, 2, 4).contiguous()
    unpacked = MipLayers(native(mip.base), torch.cat([native(mip.level(l)).reshape(-1) for l in (1, 2)]), 3, planes)
    assert unpacked.format == 'f32'
    for size in _sizes(camera)[:2]:
        kw = _camera_args(camera, size)
        for cap in (2.0, 16.0):
            a = m.render_views(mip, pose, pos, max_anisotropy=cap, **kw)
            b = m.render_views(unpacked, pose, pos, max_anisotropy=cap, **kw)
            assert torch.equal(a[0], b[0]) and torch.equal(a[1], b[1]), (size, cap)


@pytest.mark.parametrize("fmt", ['f32', 'rgba8', 'rgba16f'])
def test_render_ods_pair_is_the_two_single_views(gpu, fmt):
    torch, m = gpu
    planes = m.inv_depths(1.0, 100.0, 5)
    mip = _mip(torch, m, 16, 32, 5, 3, fmt, planes)
    pose, pos = _views('ods')
    size, bl = (9, 20), np.array([0.1, 0.05], F)
    rgb, dep = m.render_ods_pair(mip, baseline=bl, tgt_pose_rt=pose[:, 0], tgt_pos=pos[:, 0], size=size, layout='top_bottom', want_depth=True,
                                 max_anisotropy=8.0)
    assert tuple(rgb.shape) == (B, 18, 20, 3) and tuple(dep.shape) == (B, 18, 20)
    for k, eye in enumerate((1.0, -1.0)):
        r1, d1 = m.render_views(mip, pose[:, :1], pos[:, :1], camera='ods', eye=eye, baseline=bl, size=size, max_anisotropy=8.0)
        assert torch.equal(rgb[:, 9 * k:9 * k + 9], r1[:, 0]) and torch.equal(dep[:, 9 * k:9 * k + 9], d1[:, 0])
    views = m.render_ods_pair(mip, baseline=bl, tgt_pose_rt=pose[:, 0], tgt_pos=pos[:, 0], size=size, max_anisotropy=8.0)
    assert tuple(views.shape) == (B, 2, 9, 20, 3) and torch.equal(views.reshape(B, 18, 20, 3), rgb)
    trilinear = m.render_ods_pair(mip, baseline=bl, tgt_pose_rt=pose[:, 0], tgt_pos=pos[:, 0], size=size)
    assert float((views - trilinear).abs().max()) > 0.01         # (the keyword reaches the kernel)


@pytest.mark.parametrize("camera", CAMERAS)
def test_the_status_word_is_the_plain_renders(gpu, camera):
    """Device-side positions outside the innermost sphere (the host-side guard cannot look): both renders set the same bit -- for
    the ODS camera, whose origin is a property of the lane, too."""
    torch, m = gpu
    planes = m.inv_depths(1.0, 100.0, 5)
    mip = _mip(torch, m, 16, 32, 5, 3, 'rgba8', planes)
    pose, pos = _views(camera)
    kw = _camera_args(camera, _sizes(camera)[0])
    _status(m)
    m.render_views(mip, pose, torch.from_numpy(pos).cuda(), max_anisotropy=8.0, **kw)
    assert _status(m) == 0
    pos[1, 1] = [3.0, 0.0, 0.0]
    pos_d = torch.from_numpy(pos).cuda()
    m.render_views(mip.base, pose, pos_d, planes, **kw)
    s_ref = _status(m)
    got = m.render_views(mip, pose, pos_d, max_anisotropy=8.0, **kw)
    s_got = _status(m)
    assert s_ref == s_got == 1
    assert bool(torch.isfinite(got[0]).all()) and bool(torch.isfinite(got[1]).all())


def test_the_keyword_belongs_to_a_miplayers(gpu):
    torch, m = gpu
    rgba = torch.from_numpy(random_rgba(95, B, 16, 32, 5)).cuda()
    planes = m.inv_depths(1.0, 100.0, 5)
    pose, pos = _views('equirect')
    packed = m.pack_layers(rgba, 'rgba8', planes)
    for stack in (rgba, packed, m.sparsify_layers(packed)):
        with pytest.raises(ValueError, match="max_anisotropy belongs to a MipLayers"):
            m.render_views(stack, pose, pos, planes, max_anisotropy=2.0)
        m.render_views(stack, pose, pos, planes, max_anisotropy=1.0)
    with pytest.raises(ValueError, match="max_anisotropy belongs to a MipLayers"):
        m.render_ods_pair(packed, baseline=0.1, max_anisotropy=4.0)
    mip = m.build_mips(rgba, 3, planes)
    for bad in (float("nan"), 0.5, 16.5):
        with pytest.raises(ValueError, match="max_anisotropy must be in"):
            m.render_views(mip, pose, pos, max_anisotropy=bad)


# (c) ---------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("pos", [(0.0, 0.0, 0.0), (0.3, -0.2, 0.25)])
def test_on_the_device_too_a_tilted_view_is_closer_to_the_supersampled_view(gpu, pos):
    """tests/test_aniso_cpu.py's quality fact with the device's renders: the 16 x 32 view tilted by 90 degrees of the 64 x 128 x 4
    near-Nyquist stack, max_anisotropy = 8, against the fp64 8 x 8 supersampled view, on the reference's mask (largest ratio over
    the layers >= 2): anisotropic RMS <= 0.6 x trilinear RMS.  Measured on an MI355X: 0.0947 -> 0.0398 (x 0.420) centred, 0.0860 ->
    0.0382 (x 0.444) translated, the reference's own figures."""
    torch, m = gpu
    base = R.near_nyquist_stack(3)
    rgba = torch.from_numpy(base[None]).cuda().permute(0, 2, 3, 1, 4)
    mip = m.build_mips(rgba, 4, QUALITY_PLANES)
    size, P = (16, 32), tilt(90)
    sup, _ = R.supersampled_view(base, P, pos, QUALITY_PLANES, 'equirect', size)
    _, _, ratio, _ = A.aniso_view([x[0] for x in _levels_np(mip)], P, pos, QUALITY_PLANES, size=size, max_anisotropy=8.0, details=True)
    mask = ratio.max(axis=0) >= 2.0
    assert mask.mean() >= 0.3
    pose, p = P[None, None], np.asarray(pos, F)[None, None]
    tri, _ = m.render_views(mip, pose, p, size=size)
    an, _ = m.render_views(mip, pose, p, size=size, max_anisotropy=8.0)
    tri, an = _np(tri)[0, 0].astype(np.float64), _np(an)[0, 0].astype(np.float64)
    print("device, pos %s: masked %.3f | trilinear %.4f anisotropic %.4f quotient %.3f" % (
        pos, mask.mean(), rms(tri, sup, mask), rms(an, sup, mask), rms(an, sup, mask) / rms(tri, sup, mask)))
    assert rms(an, sup, mask) <= 0.6 * rms(tri, sup, mask)
