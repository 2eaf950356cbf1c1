"""Edge-rule sparse stacks on the device: MSI.sparsify_layers(border='edge') (msi_sparse_index_tiles_edge) against the numpy rule of
matryodshka_amd/sparse.py bit for bit, and MSI.mpi_render_views / cube_render_views from such a SparseLayers
(msi_mpi_render_views_sparse, msi_cube_render_views_sparse) against the dense packed render of the stack it was made from: every
output element compares == (a zero may differ in sign: a skipped step does not add c * 0), the status word too.  All checks are
exact equalities; the stacks are the smallest with more than one tile in each direction."""
import functools

import numpy as np
import pytest

from matryodshka_amd import packed as P
from matryodshka_amd import sparse as S

pytestmark = pytest.mark.gpu

F = np.float32
FORMATS = list(P.FORMATS)
BITS = {'rgba8': np.uint8, 'rgba16f': np.uint16}
B, V, D = 2, 2, 4
STACKS = [(8, 32), (12, 48)]                       # 2 x 2 and 3 x 3 tiles
MODES = [(True, True), (True, False), (False, True)]
ODD_D = 5                                          # an odd layer count: the planar render's last group of two runs past the end
CUBE_D = 3
CUBE_PLANES = [50.0, 5.0, 1.0]


@pytest.fixture(scope="module")
def gpu():
    import torch
    assert torch.cuda.is_available(), "GPU tests need a HIP device"
    from matryodshka_amd import MSI
    return torch, MSI()


def _np(t):
    return t.detach().cpu().numpy()


def _same_bits(a, b, fmt):
    return np.array_equal(np.asarray(a).view(BITS[fmt]), np.asarray(b).view(BITS[fmt]))


def _status(m):
    try:
        return m.render_status()
    except ValueError:
        return 1


def _native(x):
    return np.ascontiguousarray(np.transpose(x, (0, 3, 1, 2, 4)))


def _colours(seed, shape):
    rng = np.random.RandomState(seed)
    x = rng.uniform(-1, 1, size=shape + (4,)).astype(F)
    x[..., 3] = rng.uniform(0.05, 0.95, size=shape).astype(F)
    return x


# ------------------------------------------------------------------------------------------------ the planar stacks
@functools.lru_cache(maxsize=None)
def planar_stack(h, w, d=D):
    """fp32 [B,H,W,d,4], read-only: layer 0 all alpha 0 (its colour counts anyway), layer 1 empty (no kept tile), layer 2 a 2 x 6 block in a
    corner of the image (the top-left one in sample 0, the bottom-right one in sample 1: it touches the outer ring), layer 3 full; with
    d = ODD_D, layer 4 is layer 2's block in the opposite corner."""
    x = _colours(900 + h, (B, h, w, d))
    mask = np.zeros((B, h, w, d), F)
    mask[0, :2, :6, 2] = 1
    mask[1, h - 2:, w - 6:, 2] = 1
    mask[..., 3] = 1
    if d == ODD_D:
        mask[0, h - 2:, w - 6:, 4] = 1
        mask[1, :2, :6, 4] = 1
    x[..., 3] *= mask
    x.setflags(write=False)
    return x


def _planes(m, d):
    return [float(p) for p in m.inv_depths(1.0, 100.0, d)]


def _cam(h, w):
    return np.array([[w / 2, 0, w / 2], [0, h / 2, h / 2], [0, 0, 1]], F)


def _ry(th, t):
    p = np.eye(4, dtype=F)
    p[0, 0] = np.cos(th); p[0, 2] = np.sin(th); p[2, 0] = -np.sin(th); p[2, 2] = np.cos(th)
    p[:3, 3] = t
    return p


def planar_poses():
    """[B,V,4,4]: a near-identity view, then a translated one that looks past the layer's border."""
    s0 = [_ry(0.02, (-0.03, 0.0, 0.0)), _ry(-0.15, (0.3, 0.0, 0.1))]
    s1 = [_ry(-0.02, (0.03, 0.01, 0.0)), _ry(0.15, (-0.3, 0.0, 0.1))]
    return np.stack([np.stack(s0), np.stack(s1)]).astype(F)


def sample_coords(pose, k_s, k_t, depth, oh, ow):
    """The kernel's inverse homography (mpi_homography) in fp64: where output pixel (i, j) samples plane `depth` -> x, y [oh,ow]."""
    pose, k_s, k_t = (np.asarray(a, np.float64) for a in (pose, k_s, k_t))
    rt, t = pose[:3, :3].T, pose[:3, 3]
    m1 = rt + np.outer(rt @ t, rt[2]) / (-depth - rt[2] @ t)
    hom = k_s @ m1 @ np.linalg.inv(k_t)
    jj, ii = np.meshgrid(np.arange(ow, dtype=np.float64), np.arange(oh, dtype=np.float64))
    p = np.einsum('rc,chw->rhw', hom, np.stack([jj, ii, np.ones_like(jj)]))
    return p[0] / p[2], p[1] / p[2]


# ------------------------------------------------------------------------------------------------ the cube stacks
@functools.lru_cache(maxsize=None)
def cube_stack(s, cubes):
    """fp32 [6 cubes,S,S,D,4], read-only: layer 0 alpha 0; layer 1 occupied in its top three rows on even faces and its left five columns on odd
    faces (the outer ring); layer 2 occupied in a 3 x 3 block whose place depends on the face, and not at all on face 5."""
    n = 6 * cubes
    x = _colours(700 + s + cubes, (n, s, s, CUBE_D))
    mask = np.zeros((n, s, s, CUBE_D), F)
    mask[0::2, :3, :, 1] = 1
    mask[1::2, :, :5, 1] = 1
    for f in range(n):
        if f % 6 != 5:
            y0, x0 = (3 * f) % (s - 3), (5 * f + 7) % (s - 3)
            mask[f, y0:y0 + 3, x0:x0 + 3, 2] = 1
    x[..., 3] *= mask
    x.setflags(write=False)
    return x


def _rot(ax, ang):
    ax = np.asarray(ax, np.float64) / np.linalg.norm(ax)
    k = np.array([[0, -ax[2], ax[1]], [ax[2], 0, -ax[0]], [-ax[1], ax[0], 0]])
    return np.eye(3) + np.sin(ang) * k + (1 - np.cos(ang)) * (k @ k)


def _pose(ax, ang, t):
    p = np.eye(4)
    p[:3, :3] = _rot(ax, ang)
    p[:3, 3] = t
    return p.astype(F)


def cube_poses(cubes):
    """([cubes,2,4,4], [cubes,2,3]): the identity at the centre, and a rotated, translated origin inside the innermost shell (half-side 1)."""
    views = [(_pose((0, 1, 0), 0.0, (0, 0, 0)), (0, 0, 0)), (_pose((1, 2, 3), 0.7, (0.2, -0.15, 0.25)), (0.1, 0.2, -0.15)),
             (_pose((3, -1, 2), -1.1, (-0.25, 0.2, 0.1)), (0.15, -0.1, 0.2))]
    pose = np.stack([np.stack([views[0][0], views[1 + c % 2][0]]) for c in range(cubes)]).astype(F)
    pos = np.array([[views[0][1], views[1 + c % 2][1]] for c in range(cubes)], F)
    return pose, pos


def _k_stack(s):
    return np.array([[s / 2, 0, s / 2], [0, s / 2, s / 2], [0, 0, 1]], F)


CUBE_OUTPUTS = {"equirect": dict(camera='equirect', size=(16, 32)),
                "pinhole": dict(camera='pinhole', size=(24, 24), intrinsics=np.array([[10.8, 0, 12.5], [0, 12.0, 11.3], [0, 0, 1]], F))}


# 0 ---------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("fmt", FORMATS)
def test_0_the_masks_drop_and_keep_tiles(fmt):
    """Written against the CPU rule: tiles are dropped, tiles of layers > 0 are kept, and the edge rule differs from the wrap rule here."""
    for codes in [P.encode_np(_native(planar_stack(h, w)), fmt) for h, w in STACKS] + \
                 [P.encode_np(_native(cube_stack(s, c)), fmt) for s in (16, 32) for c in (1, 2)]:
        edge, wrap = S.keep_np(codes, fmt, 'edge'), S.keep_np(codes, fmt, 'wrap')
        assert not edge.all() and edge[:, 1:].any() and np.all(edge <= wrap) and not np.array_equal(edge, wrap)
    h, w = STACKS[0]
    per_layer = S.keep_np(P.encode_np(_native(planar_stack(h, w)), fmt), fmt, 'edge').reshape(B, D, -1).sum(-1)
    assert np.array_equal(per_layer, [[4, 0, 1, 4]] * B)               # whole, empty, one tile, full
    odd = S.keep_np(P.encode_np(_native(planar_stack(h, w, ODD_D)), fmt), fmt, 'edge')
    assert np.array_equal(odd.reshape(B, ODD_D, -1).sum(-1), [[4, 0, 1, 4, 1]] * B)      # the fifth layer: one tile kept, three dropped
    assert not np.array_equal(odd[:, 2], odd[:, 4])                                      # (in the opposite corner)


# 1 ---------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("h,w", STACKS)
@pytest.mark.parametrize("fmt", FORMATS)
def test_1_sparsify_edge_equals_sparsify_np_bit_for_bit(gpu, fmt, h, w):
    torch, m = gpu
    planes = _planes(m, D)
    pk = m.pack_layers(torch.from_numpy(planar_stack(h, w)).cuda(), fmt, planes=planes)
    codes = _np(pk.data)
    table, layer_start, pool = S.sparsify_np(codes, fmt, border='edge')
    sp = m.sparsify_layers(pk, border='edge')
    assert sp.border == 'edge' and sp.format == fmt and sp.shape == (B, h, w, D) and sp.planes == tuple(planes)
    assert np.array_equal(_np(sp.table), table) and np.array_equal(_np(sp.layer_start), layer_start)
    assert tuple(sp.pool.shape) == pool.shape and _same_bits(_np(sp.pool), pool, fmt)
    counts = np.diff(layer_start).reshape(B, D)
    tiles = (h // 4) * (w // 16)
    assert np.all(counts[:, 1] == 0) and np.all(counts[:, 3] == tiles) and np.all(counts[:, 2] == 1)   # no kept tile; a full layer; one tile
    wrap = m.sparsify_layers(pk)                                                     # the default is the sphere rule, unchanged
    assert wrap.border == 'wrap' and np.array_equal(_np(wrap.table), S.sparsify_np(codes, fmt)[0])
    assert int(wrap.layer_start[-1]) > int(sp.layer_start[-1])                       # (the corner block reaches across both borders)
    dense = m.densify_layers(sp)
    assert isinstance(dense, P.PackedLayers) and _same_bits(_np(dense.data), S.expand_np(table, layer_start, pool, fmt), fmt)
    assert _same_bits(_np(m.densify_layers(wrap).data), S.expand_np(*S.sparsify_np(codes, fmt), fmt), fmt)
    from_f32 = m.sparsify_layers(torch.from_numpy(planar_stack(h, w)).cuda(), fmt, planes=planes, border='edge')
    assert torch.equal(from_f32.table, sp.table) and _same_bits(_np(from_f32.pool), pool, fmt) and from_f32.border == 'edge'
    with pytest.raises(ValueError):
        m.sparsify_layers(pk, border='clamp')


# 2 ---------------------------------------------------------------------------------------------------------------------
def test_2_the_translated_pose_samples_outside_for_some_pixels_only():
    """From the pixel coordinates in numpy (fp64, with a margin that fp32 rounding cannot cross)."""
    from oracle.msi import MSI as OracleMSI
    for h, w in STACKS:
        for oh, ow in ((h, w), (7, 45)):
            for b in range(B):
                outside = np.zeros((oh, ow), bool)
                inside = np.zeros((oh, ow), bool)
                for depth in OracleMSI(input_type='PP').inv_depths(1.0, 100.0, D):
                    x, y = sample_coords(planar_poses()[b, 1], _cam(h, w), _cam(oh, ow), float(depth), oh, ow)
                    outside |= (x < -1.01) | (y < -1.01) | (x > w + 0.01) | (y > h + 0.01)
                    inside |= (x > -0.99) & (y > -0.99) & (x < w - 0.01) & (y < h - 0.01)
                assert outside.any() and not outside.all() and inside.any(), (h, w, oh, ow, b)


@pytest.mark.parametrize("h,w", STACKS)
@pytest.mark.parametrize("own_size", [True, False])
@pytest.mark.parametrize("fmt", FORMATS)
def test_2_planar_render_from_sparse_equals_the_dense_render(gpu, fmt, own_size, h, w):
    torch, m = gpu
    planes = _planes(m, D)
    oh, ow = (h, w) if own_size else (7, 45)            # 7 x 45: a partial last row group and a partial 64-pixel block
    pk = m.pack_layers(torch.from_numpy(planar_stack(h, w)).cuda(), fmt, planes=planes)
    sp = m.sparsify_layers(pk, border='edge')
    assert 0 < sp.occupancy < 1
    kw = dict(intrinsics=_cam(h, w), tgt_intrinsics=_cam(oh, ow), size=(oh, ow))
    pose = planar_poses()
    background = np.array(planar_stack(h, w))
    background[..., 1:, 3] = 0
    r_bg, _ = m.mpi_render_views(m.pack_layers(torch.from_numpy(background).cuda(), fmt), pose, planes, want_depth=False, **kw)
    for want_rgb, want_depth in MODES:
        rgb_s, dep_s = m.mpi_render_views(sp, pose, want_rgb=want_rgb, want_depth=want_depth, **kw)      # planes: the ones the stack carries
        rgb_d, dep_d = m.mpi_render_views(pk, pose, want_rgb=want_rgb, want_depth=want_depth, **kw)
        assert (rgb_s is None) == (not want_rgb) and (dep_s is None) == (not want_depth)
        if want_rgb:
            assert tuple(rgb_s.shape) == (B, V, oh, ow, 3)
            assert np.array_equal(_np(rgb_s), _np(rgb_d)), (want_rgb, want_depth)
            assert np.isfinite(_np(rgb_s)).all()
        if want_depth:
            assert tuple(dep_s.shape) == (B, V, oh, ow)
            assert np.array_equal(_np(dep_s), _np(dep_d)), (want_rgb, want_depth)
    assert not np.array_equal(_np(m.mpi_render_views(pk, pose, want_depth=False, **kw)[0]), _np(r_bg))   # kept layers matter
    back = m.densify_layers(sp)
    assert torch.equal(m.mpi_render_views(back, pose, **kw)[0], m.mpi_render_views(sp, pose, **kw)[0])


@pytest.mark.parametrize("want_rgb,want_depth", MODES)
@pytest.mark.parametrize("fmt", FORMATS)
def test_2_planar_render_with_an_odd_layer_count_equals_the_dense_render(gpu, fmt, want_rgb, want_depth):
    """D = 5 in groups of two layers: the last group's second lookup is past the end (the last layer's again, its step skipped)."""
    torch, m = gpu
    h, w = STACKS[0]
    pk = m.pack_layers(torch.from_numpy(planar_stack(h, w, ODD_D)).cuda(), fmt, planes=_planes(m, ODD_D))
    sp = m.sparsify_layers(pk, border='edge')
    assert sp.shape == (B, h, w, ODD_D) and np.array_equal(np.diff(_np(sp.layer_start)).reshape(B, ODD_D), [[4, 0, 1, 4, 1]] * B)
    kw = dict(intrinsics=_cam(h, w), want_rgb=want_rgb, want_depth=want_depth)
    for out_s, out_d in zip(m.mpi_render_views(sp, planar_poses(), **kw), m.mpi_render_views(pk, planar_poses(), **kw)):
        assert (out_s is None) == (out_d is None)
        if out_s is not None:
            assert tuple(out_s.shape)[:4] == (B, V, h, w) and np.array_equal(_np(out_s), _np(out_d))
    # the fifth layer is composited: without it the render differs
    if want_rgb:
        four = np.array(planar_stack(h, w, ODD_D))
        four[..., 4, 3] = 0
        r4 = m.mpi_render_views(m.pack_layers(torch.from_numpy(four).cuda(), fmt, planes=_planes(m, ODD_D)), planar_poses(), **kw)[0]
        assert not np.array_equal(_np(r4), _np(m.mpi_render_views(sp, planar_poses(), **kw)[0]))


# 3 ---------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("s,cubes", [(16, 1), (16, 2), (32, 1), (32, 2)])
@pytest.mark.parametrize("output", sorted(CUBE_OUTPUTS))
@pytest.mark.parametrize("fmt", FORMATS)
def test_3_cube_render_from_sparse_equals_the_dense_render(gpu, fmt, output, s, cubes):
    torch, m = gpu
    pk = m.pack_layers(torch.from_numpy(cube_stack(s, cubes)).cuda(), fmt, planes=CUBE_PLANES)
    sp = m.sparsify_layers(pk, border='edge')
    assert sp.shape == (6 * cubes, s, s, CUBE_D) and 0 < sp.occupancy < 1
    assert _same_bits(_np(sp.pool), S.sparsify_np(_np(pk.data), fmt, border='edge')[2], fmt)
    kw = dict(stack_intrinsics=_k_stack(s), **CUBE_OUTPUTS[output])
    oh, ow = kw['size']
    pose, pos = cube_poses(cubes)
    m.render_status()
    for want_rgb, want_depth in MODES:
        got = []
        for stack in (sp, pk):
            rgb, dep = m.cube_render_views(stack, pose, pos, want_rgb=want_rgb, want_depth=want_depth, **kw)
            torch.cuda.synchronize()
            got.append((rgb, dep, _status(m)))
        assert got[0][2] == got[1][2] == 0
        if want_rgb:
            assert tuple(got[0][0].shape) == (cubes, 2, oh, ow, 3)
            assert np.array_equal(_np(got[0][0]), _np(got[1][0])), (want_rgb, want_depth)
            assert np.isfinite(_np(got[0][0])).all()
        if want_depth:
            assert np.array_equal(_np(got[0][1]), _np(got[1][1])), (want_rgb, want_depth)
    # the moved view's rows take their texels from more than one face, and the kept layers matter
    background = np.array(cube_stack(s, cubes))
    background[..., 1:, 3] = 0
    r_bg, _ = m.cube_render_views(m.pack_layers(torch.from_numpy(background).cuda(), fmt), pose, pos, CUBE_PLANES, want_depth=False, **kw)
    assert not np.array_equal(_np(r_bg), _np(m.cube_render_views(pk, pose, pos, want_depth=False, **kw)[0]))
    # an origin outside the innermost shell (device-side pose: the kernel flags it): the same pixels and the same status word
    bad = pose.copy()
    bad[0, 1, :3, 3] = [1.5, 0.0, 0.0]
    got = []
    for stack in (sp, pk):
        rgb, dep = m.cube_render_views(stack, torch.from_numpy(bad).cuda(), pos, **kw)
        torch.cuda.synchronize()
        got.append((_np(rgb), _np(dep), _status(m)))
    assert got[0][2] == got[1][2] == 1
    assert np.array_equal(got[0][0], got[1][0]) and np.array_equal(got[0][1], got[1][1])
    assert m.render_status() == 0


def test_3_neighbouring_lanes_choose_different_faces():
    """The moved views of the cube cases look at several faces within one output row, which is one wavefront (fp64, cubemap's face rule on the rays of the equirect camera)."""
    pose, pos = cube_poses(2)
    oh, ow = CUBE_OUTPUTS["equirect"]["size"]
    for c in range(2):
        lon = (np.arange(ow) + 0.5) / ow * 2 * np.pi - np.pi
        lat = (np.arange(oh) + 0.5) / oh * np.pi - np.pi / 2
        dirs = np.stack([np.cos(lon)[None] * np.cos(lat)[:, None], np.sin(lat)[:, None] * np.ones(ow)[None], np.sin(lon)[None] * np.cos(lat)[:, None]], -1)
        dirs = dirs @ pose[c, 1, :3, :3].astype(np.float64).T
        axis = np.abs(dirs).argmax(-1) * 2 + (np.take_along_axis(dirs, np.abs(dirs).argmax(-1)[..., None], -1)[..., 0] < 0)
        assert sum(len(set(row)) > 1 for row in axis.tolist()) >= oh // 2          # (a row next to a pole may see one face only)


# 4 ---------------------------------------------------------------------------------------------------------------------
def test_4_refusals_and_the_saved_file(gpu, tmp_path):
    torch, m = gpu
    h, w = STACKS[1]
    planes = _planes(m, D)
    x = torch.from_numpy(planar_stack(h, w)).cuda()
    edge = m.sparsify_layers(x, 'rgba8', planes=planes, border='edge')
    wrap = m.sparsify_layers(x, 'rgba8', planes=planes)
    pose = planar_poses()
    pos = np.zeros((B, V, 3), F)
    kw = dict(intrinsics=_cam(h, w))
    # a stack goes to the viewers of the surface it was made for
    cube_edge = m.sparsify_layers(torch.from_numpy(cube_stack(16, 1)).cuda(), 'rgba8', planes=CUBE_PLANES, border='edge')
    cube_wrap = m.sparsify_layers(torch.from_numpy(cube_stack(16, 1)).cuda(), 'rgba8', planes=CUBE_PLANES)
    cpose, cpos = cube_poses(1)
    for call, border in ((lambda: m.render_views(edge, pose, pos), "'wrap'"),
                         (lambda: m.render_ods_pair(edge, baseline=0.03), "'wrap'"),
                         (lambda: m.mpi_render_views(wrap, pose, **kw), "'edge'"),
                         (lambda: m.cube_render_views(cube_wrap, cpose, cpos, size=(16, 32)), "'edge'")):
        with pytest.raises(TypeError) as e:
            call()
        assert "densify_layers" in str(e.value) and "border=" + border in str(e.value)
    with pytest.raises(ValueError):                                                 # S = 24: S % 16 != 0
        m.sparsify_layers(torch.from_numpy(_colours(1, (6, 24, 24, CUBE_D))).cuda(), 'rgba8', border='edge')
    with pytest.raises(ValueError):
        m.mpi_render_views(m.sparsify_layers(x, 'rgba8', border='edge'), pose, **kw)      # no planes anywhere
    with pytest.raises(ValueError):
        m.mpi_render_views(edge, pose, planes[:-1], **kw)
    # saved, loaded and rendered: the same bits
    rgb, dep = m.mpi_render_views(edge, pose, **kw)
    path = str(tmp_path / "edge.npz")
    edge.save(path)
    loaded = S.SparseLayers.load(path, device="cuda")
    assert loaded.border == 'edge' and loaded.planes == edge.planes and torch.equal(loaded.table, edge.table) and torch.equal(loaded.pool, edge.pool)
    assert torch.equal(m.mpi_render_views(loaded, pose, **kw)[0], rgb)
    assert torch.equal(m.mpi_render_views(S.SparseLayers.load(path), pose, want_rgb=False, **kw)[1], dep)   # a host-side stack is moved on the way in
    with pytest.raises(TypeError):
        m.render_views(loaded, pose, pos)
    crgb, _ = m.cube_render_views(cube_edge, cpose, cpos, size=(16, 32))
    cube_edge.save(path)
    assert torch.equal(m.cube_render_views(S.SparseLayers.load(path, device="cuda"), cpose, cpos, size=(16, 32))[0], crgb)
