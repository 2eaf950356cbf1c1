"""MSI.render_views / MSI.render_ods_pair on a MipLayers (msi_render_views_mip): the trilinear texel for the three cameras, the three
output modes and the three texel formats.

(a) where the rule says level 0 alone -- lod_bias <= -64, one level -- every output element and the status word equal the plain
    render of .base;
(b) against the fp64 statement of the rule (tests/mip_reference.py) at the project's render gate, max-abs <= 1e-3 on rgb and depth,
    no pixel excluded (the rule is continuous);
(c) a packed MipLayers renders == to the MipLayers of its unpacked base and unpacked levels;
(d) render_ods_pair's top_bottom output is the two single views;
(e) the unsupported entry points and arguments raise."""
import numpy as np
import pytest

from matryodshka_amd.mips import MipLayers
from matryodshka_amd.packed import decode_np
from tests import mip_reference as R
from tests.test_gpu_render_views import _intrinsics, _poses, _rot
from tests.util import random_rgba

pytestmark = pytest.mark.gpu

F = np.float32
TOL = 1e-3
FORMATS = ['f32', 'rgba8', 'rgba16f']
CAMERAS = ['equirect', 'pinhole', 'ods']
MODES = [(True, True), (True, False), (False, True)]
B, V, D = 2, 3, 5


@pytest.fixture(scope="module")
def gpu():
    import torch
    assert torch.cuda.is_available(), "GPU tests need a HIP device"
    from matryodshka_amd import MSI
    return torch, MSI()


def _np(t):
    return None if t is None else t.detach().cpu().numpy()


def _layers(torch, m, seed, h, w, fmt):
    rgba = torch.from_numpy(random_rgba(seed, B, h, w, D)).cuda()
    return rgba if fmt == 'f32' else m.pack_layers(rgba, fmt)


def _plain(torch, mip):
    """What render_views takes for the plain render of a MipLayers' level 0."""
    return mip.base.permute(0, 2, 3, 1, 4) if torch.is_tensor(mip.base) else mip.base


def _views(seed):
    """Poses [B,V,4,4] and positions [B,V,3]: random rotations and translations (tests/test_gpu_render_views.py), with view 0 of
    sample 0 tilted by 1.4 rad about z -- its rows pass the stack's poles, where u runs fast: lambda spans every level within 64
    columns -- and view 1 turned by pi about y: a pinhole camera there looks at the stack's u seam."""
    pose, pos = _poses(seed, B, V)
    pose[0, 0, :3, :3] = _rot(0.0, 0.0, 1.4)
    pose[0, 1, :3, :3] = _rot(0.0, np.pi, 0.0)
    return pose, pos


def _camera_args(camera, size):
    oh, ow = size
    if camera == 'pinhole':      # a wide field of view: tan(half angle) = 2
        return dict(camera='pinhole', size=size, intrinsics=_intrinsics(ow / 4.0, ow / 4.0, ow / 2.0, oh / 2.0))
    if camera == 'ods':          # both eyes among the views
        return dict(camera='ods', size=size, eye=np.array([1, -1, 1], F), baseline=0.1)
    return dict(camera='equirect', size=size)


def _status(m):
    bits = int(m._render_status.item())
    m._render_status.zero_()
    return bits


# (a) ---------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("fmt", FORMATS)
@pytest.mark.parametrize("camera", CAMERAS)
def test_level_0_alone_has_the_bits_of_the_plain_render(gpu, camera, fmt):
    """lod_bias = -64 on a three-level pyramid, and a one-level MipLayers at any bias: output widths 13 (a partial block), 64 (the
    block boundary), 65 (a last block with one valid lane) and 70; D = 5 is no multiple of the four layer segments."""
    torch, m = gpu
    h, w = 16, 32
    layers = _layers(torch, m, 51, h, w, fmt)
    planes = m.inv_depths(1.0, 100.0, D)
    pose, pos = _views(53)
    mip3, mip1 = m.build_mips(layers, 3, planes), m.build_mips(layers, 1, planes)
    assert mip3.levels == 3 and mip1.levels == 1 and mip1.mips.numel() == 0
    _status(m)
    for ow in (13, 64, 65, 70):
        kw = _camera_args(camera, (7, ow))
        for want_rgb, want_depth in MODES:
            ref = m.render_views(_plain(torch, mip3), pose, pos, planes, want_rgb=want_rgb, want_depth=want_depth, **kw)
            assert _status(m) == 0
            for mip, bias in ((mip3, -64.0), (mip3, -100.0), (mip1, 0.0), (mip1, 3.0)):
                got = m.render_views(mip, pose, pos, want_rgb=want_rgb, want_depth=want_depth, lod_bias=bias, **kw)
                assert _status(m) == 0
                for g, r in zip(got, ref):
                    assert (g is None) == (r is None)
                    if g is not None:
                        assert g.shape == r.shape and torch.equal(g, r), (ow, want_rgb, want_depth, mip.levels, bias)


@pytest.mark.parametrize("camera", CAMERAS)
def test_the_status_word_is_the_plain_renders(gpu, camera):
    """Device-side positions outside the innermost sphere (the host-side guard cannot look): both renders set the same bit."""
    torch, m = gpu
    layers = _layers(torch, m, 55, 16, 32, 'rgba8')
    planes = m.inv_depths(1.0, 100.0, D)
    pose, pos = _views(57)
    pos[1, 2] = [3.0, 0.0, 0.0]
    pos_d = torch.from_numpy(pos).cuda()
    mip = m.build_mips(layers, 3, planes)
    kw = _camera_args(camera, (7, 70))
    _status(m)
    ref = m.render_views(mip.base, pose, pos_d, planes, **kw)
    s_ref = _status(m)
    got = m.render_views(mip, pose, pos_d, lod_bias=-64.0, **kw)
    s_got = _status(m)
    assert s_ref == s_got == 1
    assert torch.equal(got[0], ref[0]) and torch.equal(got[1], ref[1])
    m.render_views(mip, pose, pos_d, lod_bias=0.5, **kw)
    assert _status(m) == 1


# (b) ---------------------------------------------------------------------------------------------------------------------
def _levels_np(mip):
    """[level 0, ..] of a MipLayers as decoded numpy arrays [B,D,h,w,4]."""
    out = []
    for l in range(mip.levels):
        lv = mip.level(l)
        out.append(lv.cpu().numpy() if mip.format == 'f32' else decode_np(lv.data.cpu().numpy(), mip.format))
    return out


@pytest.mark.parametrize("camera", CAMERAS)
@pytest.mark.parametrize("h,w,fmt", [(16, 32, 'f32'), (24, 40, 'rgba8'), (24, 40, 'f32'), (16, 32, 'rgba16f')])
def test_matches_the_fp64_reference(gpu, h, w, fmt, camera):
    """Three levels; outputs 7 x 13, 16 x 70 (a full 64-pixel block and a partial one), 1 x 9 and 9 x 1 (an axis without a neighbour;
    not for the pinhole camera, whose smallest size is 2 x 2); rotated and translated poses, a view across the u seam, both ODS eyes;
    lod_bias 0, 0.5 and 64 (the top level alone).  At 16 x 70, view 0 of sample 0 has lambda from 0 to L - 1 inside one wavefront
    (asserted on the reference).  Gate: max-abs <= 1e-3 on rgb and on depth, every pixel.
    Measured on an MI355X, the maxima over all cases: rgb 3.9e-6 (pinhole, 16 x 32 fp32 -> 16 x 70), depth 6.1e-7; per stack and
    camera the rgb maxima lie between 1.4e-6 and 3.9e-6 at 16 x 70 and below 2.1e-6 at the smaller outputs (DESIGN.md section 4,
    "Mip-mapped stacks")."""
    torch, m = gpu
    levels = 3
    layers = _layers(torch, m, 61 + h, h, w, fmt)
    planes = m.inv_depths(1.0, 100.0, D)
    pose, pos = _views(63 + w)
    mip = m.build_mips(layers, levels, planes)
    lv = _levels_np(mip)
    sizes = [(7, 13), (16, 70)] + ([] if camera == 'pinhole' else [(1, 9), (9, 1)])
    worst = {}
    spans = False
    _status(m)
    for size in sizes:
        kw = _camera_args(camera, size)
        for bias in (0.0, 0.5, 64.0):
            rgb, dep = m.render_views(mip, pose, pos, lod_bias=bias, **kw)
            assert tuple(rgb.shape) == (B, V) + size + (3,) and tuple(dep.shape) == (B, V) + size
            assert _status(m) == 0
            rgb, dep = _np(rgb), _np(dep)
            for i in range(B):
                for k in range(V):
                    e = None if camera != 'ods' else kw['eye'][k] * kw['baseline']
                    K = kw.get('intrinsics') if camera == 'pinhole' else None
                    r_o, d_o, lam = R.mip_view([x[i] for x in lv], pose[i, k], pos[i, k], planes, camera, size, K=K, e=e, lod_bias=bias,
                                               return_lod=True)
                    if bias == 64.0:
                        assert np.all(lam == levels - 1)
                    if bias == 0.0 and size == (16, 70) and (i, k) == (0, 0):
                        block = lam[:, :, :64]                                   # [D, rows, the first wavefront of each row]
                        spans = spans or bool(np.any((block.min(axis=(0, 2)) == 0.0) & (block.max(axis=(0, 2)) == levels - 1.0)))
                    key = (size, bias)
                    er = float(np.abs(rgb[i, k].astype(np.float64) - r_o).max())
                    ed = float(np.abs(dep[i, k].astype(np.float64) - d_o).max())
                    w0 = worst.get(key, (0.0, 0.0))
                    worst[key] = (max(w0[0], er), max(w0[1], ed))
    for key in sorted(worst):
        print("mip views %s %dx%d %s -> %s bias %g: max rgb %.3g depth %.3g" % ((camera, h, w, fmt) + key + worst[key]))
    if camera == 'equirect' and (h, w) == (16, 32):          # (16 rows of 16: rho = 1 vertically, 32 / 70 horizontally, away from the poles)
        assert spans, "no row of view (0, 0) at 16 x 70 spans lambda 0 .. L-1 within its first 64 columns"
    for key, (er, ed) in worst.items():
        assert er <= TOL and ed <= TOL, (key, er, ed)


def test_the_trilinear_render_is_not_the_plain_render(gpu):
    """The new path does something: a 4 x minified view differs from the plain render of the base by far more than the gate."""
    torch, m = gpu
    layers = _layers(torch, m, 71, 16, 32, 'f32')
    planes = m.inv_depths(1.0, 100.0, D)
    pose, pos = _views(73)
    mip = m.build_mips(layers, 3, planes)
    tri, _ = m.render_views(mip, pose, pos, size=(4, 8))
    plain, _ = m.render_views(_plain(torch, mip), pose, pos, planes, size=(4, 8))
    assert float((tri - plain).abs().max()) > 0.02


# (c) ---------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("fmt", ['rgba8', 'rgba16f'])
@pytest.mark.parametrize("camera", CAMERAS)
def test_a_packed_pyramid_renders_as_its_unpacked_levels(gpu, camera, fmt):
    torch, m = gpu
    layers = _layers(torch, m, 81, 24, 40, fmt)
    planes = m.inv_depths(1.0, 100.0, D)
    pose, pos = _views(83)
    mip = m.build_mips(layers, 3, planes)

    def native(packed):
        return m.unpack_layers(packed).permute(0, 3, 1, 2, 4).contiguous()
    unpacked = MipLayers(native(mip.base), torch.cat([native(mip.level(l)).reshape(-1) for l in (1, 2)]), 3, planes)
    assert unpacked.format == 'f32'
    for size in ((7, 13), (16, 70)):
        kw = _camera_args(camera, size)
        for bias in (0.0, 0.5):
            a = m.render_views(mip, pose, pos, lod_bias=bias, **kw)
            b = m.render_views(unpacked, pose, pos, lod_bias=bias, **kw)
            assert torch.equal(a[0], b[0]) and torch.equal(a[1], b[1]), (size, bias)


# (d) ---------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("fmt", FORMATS)
def test_render_ods_pair_is_the_two_single_views(gpu, fmt):
    torch, m = gpu
    layers = _layers(torch, m, 91, 16, 32, fmt)
    planes = m.inv_depths(1.0, 100.0, D)
    pose, pos = _views(93)
    mip = m.build_mips(layers, 3, planes)
    size, bl = (9, 20), np.array([0.1, 0.05], F)
    rgb, dep = m.render_ods_pair(mip, baseline=bl, tgt_pose_rt=pose[:, 0], tgt_pos=pos[:, 0], size=size, layout='top_bottom', want_depth=True,
                                 lod_bias=0.25)
    assert tuple(rgb.shape) == (B, 18, 20, 3) and tuple(dep.shape) == (B, 18, 20)
    for k, eye in enumerate((1.0, -1.0)):
        r1, d1 = m.render_views(mip, pose[:, :1], pos[:, :1], camera='ods', eye=eye, baseline=bl, size=size, lod_bias=0.25)
        assert torch.equal(rgb[:, 9 * k:9 * k + 9], r1[:, 0]) and torch.equal(dep[:, 9 * k:9 * k + 9], d1[:, 0])
    views = m.render_ods_pair(mip, baseline=bl, tgt_pose_rt=pose[:, 0], tgt_pos=pos[:, 0], size=size, lod_bias=0.25)
    assert tuple(views.shape) == (B, 2, 9, 20, 3) and torch.equal(views.reshape(B, 18, 20, 3), rgb)


# (e) ---------------------------------------------------------------------------------------------------------------------
def test_unsupported_entry_points_and_arguments_raise(gpu):
    torch, m = gpu
    rgba = torch.from_numpy(random_rgba(95, B, 16, 32, D)).cuda()
    planes = m.inv_depths(1.0, 100.0, D)
    pose, pos = _views(97)
    mip = m.build_mips(rgba, 3, planes)
    packed = m.pack_layers(rgba, 'rgba8', planes)
    # lod_bias belongs to a MipLayers
    for stack in (rgba, packed, m.sparsify_layers(packed)):
        with pytest.raises(ValueError, match="lod_bias"):
            m.render_views(stack, pose, pos, planes, lod_bias=0.5)
        m.render_views(stack, pose, pos, planes, lod_bias=0.0)
    with pytest.raises(ValueError, match="lod_bias"):
        m.render_ods_pair(packed, baseline=0.1, lod_bias=-1.0)
    with pytest.raises(ValueError, match="NaN"):
        m.render_views(mip, pose, pos, lod_bias=float("nan"))
    # planes: carried, or required
    with pytest.raises(ValueError, match="planes"):
        m.render_views(m.build_mips(rgba, 3), pose, pos)
    assert m.build_mips(packed, 2).planes == tuple(planes)
    # every other entry point that takes a stack names .base
    ident = np.tile(np.eye(4, dtype=F), (B, 1, 1))
    zero = np.zeros((B, 3), F)
    calls = [lambda: m.mpi_render_views(mip, pose, planes, intrinsics=np.eye(3, dtype=F)),
             lambda: m.cube_render_views(mip, pose, pos, planes, size=(8, 16)),
             lambda: m.cube_render_ods_pair(mip, planes, baseline=0.1, size=(8, 16)),
             lambda: m.pack_layers(mip),
             lambda: m.sparsify_layers(mip),
             lambda: m.unpack_layers(mip),
             lambda: m.build_mips(mip),
             lambda: m.msi_render_equirect_view_and_depth(mip, ident, zero, planes, None),
             lambda: m.msi_render_equirect_view_single(mip, ident, zero, planes, None)]
    for call in calls:
        with pytest.raises(TypeError, match=r"\.base"):
            call()
    with pytest.raises(TypeError):
        m.build_mips(m.sparsify_layers(packed))
    with pytest.raises(ValueError):
        m.build_mips(rgba, 5)                       # 16 x 32: a 1 x 2 top level
    with pytest.raises(ValueError):
        m.build_mips(rgba, 3, planes[:-1])
