"""Sparse layer stacks on the device: MSI.sparsify_layers / densify_layers (msi_sparse_index_tiles, _gather_tiles, _expand) against
the numpy rule of matryodshka_amd/sparse.py bit for bit, and MSI.render_views / render_ods_pair from a SparseLayers
(msi_render_views_sparse) against the dense packed render of the stack it was made from and of its densify_layers: every output
element compares == (a zero may differ in sign: a skipped step does not add c * 0).  All checks are exact equalities."""
import numpy as np
import pytest

from matryodshka_amd import packed as P
from matryodshka_amd import sparse as S
from tests.util import random_rgba

pytestmark = pytest.mark.gpu

F = np.float32
FORMATS = list(P.FORMATS)
BITS = {'rgba8': np.uint8, 'rgba16f': np.uint16}
SHAPES = [(12, 48, 3), (12, 48, 6), (16, 64, 9), (32, 128, 32)]       # (H, W, D); D = 3 < RENDER_SEGS: a layer segment is empty
B, V = 2, 2
MODES = [(True, False), (False, True), (True, True)]                  # (want_rgb, want_depth)


@pytest.fixture(scope="module")
def gpu():
    import torch
    assert torch.cuda.is_available(), "GPU tests need a HIP device"
    from matryodshka_amd import MSI
    return torch, MSI()


def _rot(ax, ay, az):
    cx, sx, cy, sy, cz, sz = np.cos(ax), np.sin(ax), np.cos(ay), np.sin(ay), np.cos(az), np.sin(az)
    rx = np.array([[1, 0, 0], [0, cx, -sx], [0, sx, cx]])
    ry = np.array([[cy, 0, sy], [0, 1, 0], [-sy, 0, cy]])
    rz = np.array([[cz, -sz, 0], [sz, cz, 0], [0, 0, 1]])
    return rz @ ry @ rx


def _poses(seed, b, v, trans=0.1):
    """Rotated and translated poses [B,V,4,4] and target positions [B,V,3], as tests/test_gpu_packed_layers.py."""
    rng = np.random.RandomState(seed)
    pose = np.tile(np.eye(4, dtype=F), (b, v, 1, 1))
    for i in range(b):
        for k in range(v):
            pose[i, k, :3, :3] = _rot(*rng.uniform(-np.pi, np.pi, 3))
            pose[i, k, :3, 3] = rng.uniform(-trans, trans, 3)
    pos = rng.uniform(-trans, trans, size=(b, v, 3)).astype(F)
    return pose, pos


def special_layer(d):
    """The first layer of a later segment (RENDER_SEGS = 4 segments; segment s starts at s * D // 4) that the fixed layers 0..3 leave free."""
    firsts = [s * d // 4 for s in range(1, 4)]
    return next((l for l in firsts if l >= 4), None)


def alpha_mask(h, w, d):
    """[B,H,W,D] of 0 / 1: layer 0 all zero (the background rule: its colour counts anyway), layer 1 empty, layer 2 one texel at (0, 0), layer 3
    one at (3, 15), the first layer of a later segment empty in sample 0 and full in sample 1, every other layer a rectangle of a third of the
    area -- the last one touching x = W - 1 and y = H - 1."""
    m = np.zeros((B, h, w, d), F)
    rh, rw = h // 2, 2 * w // 3
    for l in range(1, d):
        if l == 1:
            continue
        if l == 2:
            m[:, 0, 0, l] = 1
        elif l == 3:
            m[:, 3, 15, l] = 1
        elif l == special_layer(d):
            m[1, :, :, l] = 1
        else:
            y0, x0 = ((l * 3) % (h - rh + 1), (l * 7) % (w - rw + 1)) if l != d - 1 else (h - rh, w - rw)
            m[:, y0:y0 + rh, x0:x0 + rw, l] = 1
    return m


_STACKS = {}


def masked_stack(h, w, d):
    """fp32 [B,H,W,D,4], made once per shape and left unchanged: random colour everywhere, alpha in [0.05, 0.95] under the mask and 0 elsewhere."""
    if (h, w, d) not in _STACKS:
        x = random_rgba(400 + d, B, h, w, d)
        x[..., 3] = (0.05 + 0.9 * x[..., 3]) * alpha_mask(h, w, d)
        x.setflags(write=False)
        _STACKS[(h, w, d)] = x
    return _STACKS[(h, w, d)]


def _native(x):
    return np.ascontiguousarray(np.transpose(x, (0, 3, 1, 2, 4)))


def _np(t):
    return t.detach().cpu().numpy()


def _same_bits(a, b, fmt):
    return np.array_equal(np.asarray(a).view(BITS[fmt]), np.asarray(b).view(BITS[fmt]))


def _status(m):
    try:
        return m.render_status()
    except ValueError:
        return 1


def _cameras(h, w):
    """name -> render_views keywords: equirect at the stack's size and at an odd size whose width is not a multiple of 64, pinhole at that odd size,
    and both ODS eyes (V = 2: left, right) with a non-zero baseline."""
    oh, ow = h + 7, w + 37
    assert ow % 64 != 0
    K = np.array([[0.6 * ow, 0, 0.5 * ow], [0, 0.45 * oh, 0.45 * oh], [0, 0, 1]], F)
    return {"equirect": {}, "equirect_odd": dict(size=(oh, ow)), "pinhole_odd": dict(camera='pinhole', intrinsics=K, size=(oh, ow)),
            "ods": dict(camera='ods', eye=np.array([1.0, -1.0], F), baseline=0.05, size=(oh, ow))}


# the masks are written against the CPU rule: occupied enough for the kept layers to matter, empty enough for tiles to be dropped
@pytest.mark.parametrize("h,w,d", SHAPES)
@pytest.mark.parametrize("fmt", FORMATS)
def test_0_masks_are_neither_empty_nor_full(fmt, h, w, d):
    codes = P.encode_np(_native(masked_stack(h, w, d)), fmt)
    table, layer_start, pool = S.sparsify_np(codes, fmt)
    occupancy = pool.shape[0] / float(table.size)
    print("%dx%dx%d %s: occupancy %.3f" % (w, h, d, fmt, occupancy))
    assert 0.2 <= occupancy <= 0.8
    per_layer = np.diff(layer_start).reshape(B, d)
    tiles = (h // 4) * (w // 16)
    assert np.all(per_layer[:, 0] == tiles) and np.all(per_layer[:, 1] == 0)
    if d > 2:
        assert np.all(per_layer[:, 2] == 4)                    # the texel at (0, 0) reaches four tiles through both wraps
    if d > 3:
        assert np.all(per_layer[:, 3] == 4)
    if special_layer(d) is not None:
        assert per_layer[0, special_layer(d)] == 0 and per_layer[1, special_layer(d)] == tiles


# 1 ---------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("h,w,d", SHAPES)
@pytest.mark.parametrize("fmt", FORMATS)
def test_1_sparsify_equals_sparsify_np_bit_for_bit(gpu, fmt, h, w, d):
    torch, m = gpu
    planes = m.inv_depths(1.0, 100.0, d)
    pk = m.pack_layers(torch.from_numpy(masked_stack(h, w, d)).cuda(), fmt, planes=planes)
    codes = _np(pk.data)
    assert _same_bits(codes, P.encode_np(_native(masked_stack(h, w, d)), fmt), fmt)
    table, layer_start, pool = S.sparsify_np(codes, fmt)
    sp = m.sparsify_layers(pk)
    assert isinstance(sp, S.SparseLayers) and sp.format == fmt and sp.shape == (B, h, w, d) and sp.tile == (4, 16)
    assert sp.planes == tuple(planes) and sp.pool.is_cuda
    assert sp.table.dtype == torch.int32 and sp.layer_start.dtype == torch.int64
    assert np.array_equal(_np(sp.table), table)
    assert np.array_equal(_np(sp.layer_start), layer_start)
    assert tuple(sp.pool.shape) == pool.shape and _same_bits(_np(sp.pool), pool, fmt)
    assert sp.nbytes == table.nbytes + layer_start.nbytes + pool.nbytes < pk.nbytes
    assert sp.occupancy == pool.shape[0] / float(table.size)
    again = m.sparsify_layers(pk)                                                   # twice: identical bytes
    assert torch.equal(again.table, sp.table) and torch.equal(again.layer_start, sp.layer_start)
    assert _same_bits(_np(again.pool), _np(sp.pool), fmt)
    from_f32 = m.sparsify_layers(torch.from_numpy(masked_stack(h, w, d)).cuda(), fmt, planes=planes)   # an fp32 stack is packed first
    assert torch.equal(from_f32.table, sp.table) and _same_bits(_np(from_f32.pool), pool, fmt) and from_f32.planes == sp.planes


# 2 ---------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("h,w,d", SHAPES)
@pytest.mark.parametrize("fmt", FORMATS)
def test_2_densify_equals_expand_np(gpu, fmt, h, w, d):
    torch, m = gpu
    pk = m.pack_layers(torch.from_numpy(masked_stack(h, w, d)).cuda(), fmt)
    sp = m.sparsify_layers(pk)
    dense = m.densify_layers(sp)
    assert isinstance(dense, P.PackedLayers) and dense.format == fmt and dense.shape == pk.shape and dense.planes is None
    ref = S.expand_np(*S.sparsify_np(_np(pk.data), fmt), fmt)
    assert _same_bits(_np(dense.data), ref, fmt)
    assert not _same_bits(_np(dense.data), _np(pk.data), fmt)                       # (layer 0's dropped-alpha colours stay, tiles elsewhere went)
    assert _same_bits(_np(m.densify_layers(S.SparseLayers.from_codes(_np(pk.data), fmt)).data), ref, fmt)     # a host-side stack is moved on the way in


# 3 ---------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("h,w,d", SHAPES)
@pytest.mark.parametrize("camera", ["equirect", "equirect_odd", "pinhole_odd", "ods"])
@pytest.mark.parametrize("fmt", FORMATS)
def test_3_render_from_sparse_equals_the_dense_render(gpu, fmt, camera, h, w, d):
    torch, m = gpu
    planes = m.inv_depths(1.0, 100.0, d)
    pk = m.pack_layers(torch.from_numpy(masked_stack(h, w, d)).cuda(), fmt, planes=planes)
    sp = m.sparsify_layers(pk)
    back = m.densify_layers(sp)
    pose, pos = _poses(17 + d, B, V)
    kw = _cameras(h, w)[camera]
    oh, ow = kw.get('size', (h, w))
    # kept layers matter: the dense render is not the render of layer 0 alone
    background = np.array(masked_stack(h, w, d))
    background[..., 1:, 3] = 0
    r_bg, _ = m.render_views(m.pack_layers(torch.from_numpy(background).cuda(), fmt), pose, pos, planes, want_depth=False, **kw)
    m.render_status()
    for want_rgb, want_depth in MODES:
        out = []
        for stack in (sp, pk, back):
            rgb, dep = m.render_views(stack, pose, pos, want_rgb=want_rgb, want_depth=want_depth, **kw)     # planes: the ones each stack carries
            torch.cuda.synchronize()
            out.append((rgb, dep, _status(m)))
        assert (out[0][0] is None) == (not want_rgb) and (out[0][1] is None) == (not want_depth)
        for other in out[1:]:
            if want_rgb:
                assert tuple(out[0][0].shape) == (B, V, oh, ow, 3)
                assert np.array_equal(_np(out[0][0]), _np(other[0])), (want_rgb, want_depth)
            if want_depth:
                assert tuple(out[0][1].shape) == (B, V, oh, ow)
                assert np.array_equal(_np(out[0][1]), _np(other[1])), (want_rgb, want_depth)
            assert out[0][2] == other[2] == 0
        if want_rgb and not want_depth:
            assert not np.array_equal(_np(out[1][0]), _np(r_bg))
            assert np.isfinite(_np(out[0][0])).all()


@pytest.mark.parametrize("fmt", FORMATS)
def test_3b_ods_pair_from_sparse_equals_the_dense_pair(gpu, fmt):
    torch, m = gpu
    h, w, d = 16, 64, 9
    planes = m.inv_depths(1.0, 100.0, d)
    pk = m.pack_layers(torch.from_numpy(masked_stack(h, w, d)).cuda(), fmt, planes=planes)
    sp = m.sparsify_layers(pk)
    pose, pos = _poses(29, B, 1)
    kw = dict(baseline=np.array([0.032, 0.06], F), tgt_pose_rt=pose[:, 0], tgt_pos=pos[:, 0], size=(h + 7, w + 37))     # a moved head
    rgb_s, dep_s = m.render_ods_pair(sp, want_depth=True, **kw)
    rgb_d, dep_d = m.render_ods_pair(pk, want_depth=True, **kw)
    assert tuple(rgb_s.shape) == (B, 2, h + 7, w + 37, 3)
    assert np.array_equal(_np(rgb_s), _np(rgb_d)) and np.array_equal(_np(dep_s), _np(dep_d))
    assert not np.array_equal(_np(rgb_s[:, 0]), _np(rgb_s[:, 1]))                   # two eyes
    tb = m.render_ods_pair(sp, layout='top_bottom', **kw)
    assert tuple(tb.shape) == (B, 2 * (h + 7), w + 37, 3) and np.array_equal(_np(tb).reshape(_np(rgb_s).shape), _np(rgb_s))
    torch.cuda.synchronize()
    assert m.render_status() == 0


# 4 ---------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("camera", ["equirect", "pinhole_odd", "ods"])
@pytest.mark.parametrize("fmt", FORMATS)
def test_4_an_origin_outside_sets_the_dense_renders_status_bit(gpu, fmt, camera):
    torch, m = gpu
    h, w, d = 12, 48, 6
    planes = m.inv_depths(1.0, 100.0, d)
    pk = m.pack_layers(torch.from_numpy(masked_stack(h, w, d)).cuda(), fmt, planes=planes)
    sp = m.sparsify_layers(pk)
    pose, pos = _poses(41, B, V, trans=0.05)
    kw = _cameras(h, w)[camera]
    m.render_status()
    bad = pose.copy()
    bad[1, 0, :3, 3] = [1.5, 0.0, 0.0]                      # one view's origin outside the innermost sphere (radius 1)
    with pytest.raises(ValueError):
        m.render_views(sp, bad, pos, **kw)                  # host-side guard, with the planes the stack carries
    for p, flagged in ((pose, 0), (bad, 1)):
        got = []
        for stack in (sp, pk):
            rgb, dep = m.render_views(stack, torch.from_numpy(p).cuda(), pos, **kw)      # device-side pose: the kernel flags it
            torch.cuda.synchronize()
            got.append((_np(rgb), _np(dep), _status(m)))
        assert got[0][2] == got[1][2] == flagged
        assert np.array_equal(got[0][0], got[1][0]) and np.array_equal(got[0][1], got[1][1])     # (clamped: finite, and the same pixels)
    assert m.render_status() == 0


# 5 ---------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("which", ["full", "background_only"])
@pytest.mark.parametrize("fmt", FORMATS)
def test_5_fully_occupied_and_background_only_stacks_render_equal(gpu, fmt, which):
    torch, m = gpu
    h, w, d = 16, 64, 9
    planes = m.inv_depths(1.0, 100.0, d)
    x = random_rgba(77, B, h, w, d)
    if which == "full":
        x[..., 3] = 0.05 + 0.9 * x[..., 3]
    else:
        x[..., 1:, 3] = 0
    pk = m.pack_layers(torch.from_numpy(x).cuda(), fmt, planes=planes)
    sp = m.sparsify_layers(pk)
    assert sp.occupancy == (1.0 if which == "full" else 1.0 / d)
    assert int(sp.layer_start[-1]) == B * (d if which == "full" else 1) * (h // 4) * (w // 16)
    pose, pos = _poses(53, B, V)
    for name, kw in sorted(_cameras(h, w).items()):
        rgb_s, dep_s = m.render_views(sp, pose, pos, **kw)
        rgb_d, dep_d = m.render_views(pk, pose, pos, **kw)
        assert np.array_equal(_np(rgb_s), _np(rgb_d)) and np.array_equal(_np(dep_s), _np(dep_d)), name
    if which == "full":
        assert _same_bits(_np(m.densify_layers(sp).data), _np(pk.data), fmt)
    torch.cuda.synchronize()
    assert m.render_status() == 0


# 6 ---------------------------------------------------------------------------------------------------------------------
def test_6_python_refusals_and_the_saved_file(gpu, tmp_path):
    torch, m = gpu
    h, w, d = 12, 48, 6
    planes = m.inv_depths(1.0, 100.0, d)
    x = torch.from_numpy(masked_stack(h, w, d)).cuda()
    sp = m.sparsify_layers(x, 'rgba8', planes=planes)
    without = m.sparsify_layers(x, 'rgba8')
    pose, pos = _poses(61, B, V)
    rgb, dep = m.render_views(sp, pose, pos)
    with pytest.raises(ValueError):
        m.render_views(without, pose, pos)                                          # no planes anywhere
    assert torch.equal(m.render_views(without, pose, pos, planes)[0], rgb)
    with pytest.raises(ValueError):
        m.render_views(sp, pose, pos, planes[:-1])                                  # len(planes) != D
    with pytest.raises(ValueError):
        m.sparsify_layers(x, 'rgba4')
    with pytest.raises(ValueError):
        m.sparsify_layers(x, 'rgba8', planes=planes[:-1])
    for hh, ww in ((10, 48), (12, 40)):                                             # not whole tiles
        with pytest.raises(ValueError):
            m.sparsify_layers(torch.from_numpy(random_rgba(5, 1, hh, ww, 2)).cuda())
    with pytest.raises(TypeError):
        m.sparsify_layers(sp)
    with pytest.raises(TypeError):
        m.densify_layers(m.densify_layers(sp))
    # every other entry point says where a sparse stack can go
    K = np.eye(3, dtype=F)[None].repeat(B, 0)
    for call in (lambda: m.msi_render_equirect_view(sp, pose[:, 0], pos[:, 0], planes, None),
                 lambda: m.mpi_render_view(sp, pose[:, 0], planes, K),
                 lambda: m.mpi_render_views(sp, pose, planes, K),
                 lambda: m.cube_render_views(sp, pose, pos, planes),
                 lambda: m.unpack_layers(sp),
                 lambda: m.pack_layers(sp)):
        with pytest.raises(TypeError) as e:
            call()
        assert "densify_layers" in str(e.value)
    # saved, loaded and rendered: the same bits
    path = str(tmp_path / "sparse.npz")
    sp.save(path)
    loaded = S.SparseLayers.load(path, device="cuda")
    assert loaded.planes == sp.planes and torch.equal(loaded.table, sp.table) and torch.equal(loaded.pool, sp.pool)
    assert torch.equal(m.render_views(loaded, pose, pos)[0], rgb)
    assert torch.equal(m.render_views(S.SparseLayers.load(path), pose, pos, want_rgb=False)[1], dep)       # a host-side stack is moved on the way in
