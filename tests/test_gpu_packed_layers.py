"""Compact layer stacks on the device: msi_pack_layers / msi_unpack_layers against the numpy rule of
matryodshka_amd/packed.py bit for bit, and MSI.render_views from a PackedLayers (msi_render_views_packed) against
render_views on the unpacked stack, bit for bit.  Against the ORIGINAL fp32 stack the render differs by the quantisation of the
texels only; the bound of test 4 is derived there, not tuned."""
import numpy as np
import pytest

from matryodshka_amd import packed as P
from tests.util import random_rgba

pytestmark = pytest.mark.gpu

F = np.float32
FORMATS = list(P.FORMATS)
BITS = {'rgba8': np.uint8, 'rgba16f': np.uint16}
SIZES = [(32, 64, 4), (30, 70, 5), (320, 640, 32)]


@pytest.fixture(scope="module")
def gpu():
    import torch
    assert torch.cuda.is_available(), "GPU tests need a HIP device"
    from matryodshka_amd import MSI
    return torch, MSI()


def _np(t):
    return t.detach().cpu().numpy()


def _native(x):
    """[B,H,W,D,4] -> contiguous native [B,D,H,W,4] (numpy)."""
    return np.ascontiguousarray(np.transpose(x, (0, 3, 1, 2, 4)))


def _rot(ax, ay, az):
    cx, sx, cy, sy, cz, sz = np.cos(ax), np.sin(ax), np.cos(ay), np.sin(ay), np.cos(az), np.sin(az)
    rx = np.array([[1, 0, 0], [0, cx, -sx], [0, sx, cx]])
    ry = np.array([[cy, 0, sy], [0, 1, 0], [-sy, 0, cy]])
    rz = np.array([[cz, -sz, 0], [sz, cz, 0], [0, 0, 1]])
    return rz @ ry @ rx


def _poses(seed, b, v, trans=0.1):
    """Rotated and translated poses [B,V,4,4] and target positions [B,V,3], as tests/test_gpu_render_views.py."""
    rng = np.random.RandomState(seed)
    pose = np.tile(np.eye(4, dtype=F), (b, v, 1, 1))
    for i in range(b):
        for k in range(v):
            pose[i, k, :3, :3] = _rot(*rng.uniform(-np.pi, np.pi, 3))
            pose[i, k, :3, 3] = rng.uniform(-trans, trans, 3)
    pos = rng.uniform(-trans, trans, size=(b, v, 3)).astype(F)
    return pose, pos


def _camera_kw(camera, h, w):
    """Equirect at the stack's size; pinhole at another size whose width is not a multiple of 64."""
    if camera == 'equirect':
        return {}
    oh, ow = h + 7, w + 37
    assert ow % 64 != 0
    K = np.array([[0.6 * ow, 0, 0.5 * ow], [0, 0.45 * oh, 0.45 * oh], [0, 0, 1]], F)
    return dict(camera='pinhole', intrinsics=K, size=(oh, ow))


def _edge_block():
    """[1,1,n,1,4] (H = 1, W = n, D = 1; n is odd, so the converters' one-texel tail runs too): +-1, +-0, every exact half-code
    tie candidate of both rules, the neighbours of the range ends, +-1.5, huge values and denormals."""
    k = np.arange(255, dtype=np.float64)
    vals = np.concatenate([
        np.array([1, -1, 0.0, -0.0, 1.5, -1.5, 0.5, -0.5, 3e38, -3e38, 70000, -70000, 65520, 6e-8, -6e-8], F),
        ((k + 0.5) / 127.5 - 1.0).astype(F), ((k + 0.5) / 255.0).astype(F),
        np.nextafter(F(1), F(2), dtype=F)[None], np.nextafter(F(1), F(0), dtype=F)[None],
        np.nextafter(F(-1), F(-2), dtype=F)[None], np.nextafter(F(-1), F(0), dtype=F)[None],
        np.array([1e-40, -1e-40, 1.4e-45, -1.4e-45, 1.1754942e-38, -1.1754942e-38], F)])
    if vals.size % 2 == 0:
        vals = np.append(vals, F(0.25))
    x = np.empty((1, 1, vals.size, 1, 4), F)
    for c in range(4):
        x[0, 0, :, 0, c] = np.roll(vals, 3 * c)           # (every value meets every channel's rule)
    return x


# 1 ---------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("fmt", FORMATS)
@pytest.mark.parametrize("what", ["small", "full", "edges"])
def test_pack_equals_encode_np_bit_for_bit(gpu, fmt, what):
    torch, m = gpu
    x = {"small": lambda: random_rgba(11, 2, 30, 70, 5), "full": lambda: random_rgba(12, 1, 320, 640, 32), "edges": _edge_block}[what]()
    pk = m.pack_layers(torch.from_numpy(x).cuda(), fmt)
    b, h, w, d = x.shape[:4]
    assert pk.format == fmt and pk.shape == (b, h, w, d) and tuple(pk.data.shape) == (b, d, h, w, 4)
    assert pk.nbytes == b * h * w * d * P.BYTES_PER_TEXEL[fmt] and pk.planes is None
    ref = P.encode_np(_native(x), fmt)
    got = _np(pk.data)
    assert got.dtype == ref.dtype
    assert np.array_equal(got.view(BITS[fmt]), ref.view(BITS[fmt]))
    # a permuted view of a native stack goes through as it is
    view = torch.from_numpy(_native(x)).cuda().permute(0, 2, 3, 1, 4)
    assert torch.equal(m.pack_layers(view, fmt).data, pk.data)


# 2 ---------------------------------------------------------------------------------------------------------------------
def test_unpack_rgba8_equals_decode_np_for_every_code(gpu):
    torch, m = gpu
    codes = np.empty((1024 + 3, 4), np.uint8)                       # (+ 3: the one-texel tail)
    for n in range(codes.shape[0]):
        q, c = n % 256, (n // 256) % 4
        codes[n] = [(q * 7 + 13 * j + 5) % 256 for j in range(4)]
        codes[n, c] = q                                             # code q in channel c
    for c in range(4):
        assert set(codes[256 * c:256 * (c + 1), c].tolist()) == set(range(256))
    pk = P.PackedLayers(torch.from_numpy(codes.reshape(1, 1, 1, -1, 4)).cuda(), 'rgba8')
    got = _np(m.unpack_layers(pk).permute(0, 3, 1, 2, 4)).reshape(-1, 4)
    assert np.array_equal(got.view(np.uint32), P.decode_np(codes, 'rgba8').view(np.uint32))


def test_unpack_rgba16f_equals_decode_np_for_every_bit_pattern(gpu):
    torch, m = gpu
    codes = np.arange(65536, dtype=np.uint16).view(np.float16).reshape(1, 1, 128, 128, 4)
    pk = P.PackedLayers(torch.from_numpy(codes).cuda(), 'rgba16f')
    out = m.unpack_layers(pk)
    assert tuple(out.shape) == (1, 128, 128, 1, 4)
    got = _np(out.permute(0, 3, 1, 2, 4))
    ref = P.decode_np(codes, 'rgba16f')
    nan = np.isnan(ref)
    assert nan.sum() == 2 * 1023                                    # every NaN pattern of a half
    assert np.all(np.isnan(got[nan]))
    assert np.array_equal(got[~nan].view(np.uint32), ref[~nan].view(np.uint32))


@pytest.mark.parametrize("fmt", FORMATS)
def test_pack_then_unpack_is_decode_of_encode(gpu, fmt):
    torch, m = gpu
    x = random_rgba(13, 2, 30, 70, 5)
    back = m.unpack_layers(m.pack_layers(torch.from_numpy(x).cuda(), fmt))
    assert tuple(back.shape) == x.shape and back.permute(0, 3, 1, 2, 4).is_contiguous()     # a view of a native stack
    ref = np.transpose(P.decode_np(P.encode_np(_native(x), fmt), fmt), (0, 2, 3, 1, 4))
    assert np.array_equal(_np(back).view(np.uint32), ref.view(np.uint32))


# 3 ---------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("h,w,d", SIZES)
@pytest.mark.parametrize("camera", ["equirect", "pinhole"])
@pytest.mark.parametrize("fmt", FORMATS)
def test_render_from_packed_is_bit_identical_to_render_of_unpacked(gpu, fmt, camera, h, w, d):
    torch, m = gpu
    b, v = 2, 3
    rgba = torch.from_numpy(random_rgba(31 + d, b, h, w, d)).cuda()
    pose, pos = _poses(7 + d, b, v)
    planes = m.inv_depths(1.0, 100.0, d)
    kw = _camera_kw(camera, h, w)
    pk = m.pack_layers(rgba, fmt)
    expanded = m.unpack_layers(pk)
    oh, ow = kw.get('size', (h, w))
    for want_rgb, want_depth in ((True, True), (True, False), (False, True)):
        r_p, d_p = m.render_views(pk, pose, pos, planes, want_rgb=want_rgb, want_depth=want_depth, **kw)
        r_u, d_u = m.render_views(expanded, pose, pos, planes, want_rgb=want_rgb, want_depth=want_depth, **kw)
        assert (r_p is None) == (not want_rgb) and (d_p is None) == (not want_depth)
        if want_rgb:
            assert tuple(r_p.shape) == (b, v, oh, ow, 3)
            assert torch.equal(r_p, r_u), (want_rgb, want_depth)
        if want_depth:
            assert tuple(d_p.shape) == (b, v, oh, ow)
            assert torch.equal(d_p, d_u), (want_rgb, want_depth)
    torch.cuda.synchronize()
    assert m.render_status() == 0


# 4 ---------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("h,w,d", SIZES)
@pytest.mark.parametrize("camera", ["equirect", "pinhole"])
@pytest.mark.parametrize("fmt", FORMATS)
def test_render_from_packed_stays_within_the_quantisation_bound(gpu, fmt, camera, h, w, d):
    """The composite is multilinear in the texels and the bilinear taps are convex combinations: changing one alpha by e_a moves
    a colour output by at most 2 e_a (colours in [-1, 1]) and a depth output by at most e_a; changing the colours by e_c moves a
    colour output by at most e_c.  D - 1 alphas take part (the farthest layer's is ignored).
      rgba8:   e_c = 1/255, e_a = 1/510  ->  rgb 1/255 + 2 (D-1)/510 + 1e-5,  depth (D-1)/510 + 1e-5
      rgba16f: e = 2^-12 (half an ulp of a half below 1)  ->  2^-12 (1 + 2 (D-1)) + 1e-5 on both
    (1e-5: fp32 rounding of the two composites.)  Loose on purpose: the bound catches a wrong channel order or scale.
    The measured max, mean and PSNR (evaluate.psnr on the 0..255 scale) are printed; DESIGN.md section 4 K4 records them."""
    torch, m = gpu
    b, v = 2, 3
    rgba = torch.from_numpy(random_rgba(31 + d, b, h, w, d)).cuda()
    pose, pos = _poses(7 + d, b, v)
    planes = m.inv_depths(1.0, 100.0, d)
    kw = _camera_kw(camera, h, w)
    r_p, d_p = m.render_views(m.pack_layers(rgba, fmt), pose, pos, planes, **kw)
    r_f, d_f = m.render_views(rgba, pose, pos, planes, **kw)
    er, ed = torch.abs(r_p - r_f), torch.abs(d_p - d_f)
    if fmt == 'rgba8':
        bound_rgb, bound_depth = 1 / 255 + 2 * (d - 1) / 510 + 1e-5, (d - 1) / 510 + 1e-5
    else:
        bound_rgb = bound_depth = 2.0 ** -12 * (1 + 2 * (d - 1)) + 1e-5
    from matryodshka_amd import evaluate
    psnr = evaluate.psnr(_np((r_p + 1) / 2 * 255), _np((r_f + 1) / 2 * 255))
    print("%s %s %dx%dx%d: rgb max %.3e mean %.3e (bound %.3e), depth max %.3e mean %.3e (bound %.3e), PSNR %.2f dB" % (
        fmt, camera, w, h, d, er.max().item(), er.mean().item(), bound_rgb, ed.max().item(), ed.mean().item(), bound_depth, psnr))
    assert er.max().item() <= bound_rgb
    assert ed.max().item() <= bound_depth


# 5 ---------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("fmt", FORMATS)
def test_domain_host_device_and_clear_through_the_packed_path(gpu, fmt):
    torch, m = gpu
    b, v, h, w, d = 1, 4, 16, 32, 4
    planes = m.inv_depths(1.0, 100.0, d)
    pk = m.pack_layers(torch.from_numpy(random_rgba(91, b, h, w, d)).cuda(), fmt, planes=planes)
    pose, pos = _poses(93, b, v, trans=0.05)
    m.render_status()                                      # (start from a clear word)
    m.render_views(pk, pose, pos)
    torch.cuda.synchronize()
    assert m.render_status() == 0                          # in-domain: the status stays clear
    bad = pose.copy()
    bad[0, 2, :3, 3] = [1.5, 0.0, 0.0]                     # one view's origin outside the innermost sphere (radius 1)
    with pytest.raises(ValueError):
        m.render_views(pk, bad, pos)                       # host-side guard, with the planes the stack carries
    with pytest.raises(ValueError):
        m.render_views(pk, bad, pos, planes)
    m.render_views(pk, torch.from_numpy(bad).cuda(), pos)  # device-side pose: the kernel flags it
    with pytest.raises(ValueError):
        m.render_status()
    assert m.render_status() == 0                          # (render_status reset the word)


# 6 ---------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("fmt", FORMATS)
def test_planes_travel_with_the_stack(gpu, fmt, tmp_path):
    torch, m = gpu
    b, v, h, w, d = 2, 3, 30, 70, 5
    rgba = torch.from_numpy(random_rgba(61, b, h, w, d)).cuda()
    planes = m.inv_depths(1.0, 100.0, d)
    pose, pos = _poses(63, b, v)
    with_planes = m.pack_layers(rgba, fmt, planes=planes)
    without = m.pack_layers(rgba, fmt)
    assert with_planes.planes == tuple(planes) and without.planes is None
    rgb, dep = m.render_views(with_planes, pose, pos)                          # planes=None: the stored ones
    rgb2, dep2 = m.render_views(without, pose, pos, planes)
    assert torch.equal(rgb, rgb2) and torch.equal(dep, dep2)
    with pytest.raises(ValueError):
        m.render_views(without, pose, pos)                                     # no planes anywhere
    with pytest.raises(ValueError):
        m.render_views(rgba, pose, pos)                                        # an fp32 stack needs planes
    with pytest.raises(ValueError):
        m.render_views(with_planes, pose, pos, planes[:-1])                    # len(planes) != D
    with pytest.raises(ValueError):
        m.pack_layers(rgba, fmt, planes=planes[:-1])
    with pytest.raises(ValueError):
        m.pack_layers(rgba, 'rgba4')
    # the other renders say where a packed stack can go
    with pytest.raises(TypeError) as e:
        m.msi_render_equirect_view(with_planes, pose[:, 0], pos[:, 0], planes, None)
    assert "render_views" in str(e.value) and "unpack_layers" in str(e.value)
    with pytest.raises(TypeError):
        m.mpi_render_view(with_planes, pose[:, 0], planes, np.eye(3, dtype=F)[None].repeat(b, 0))
    # saved, loaded and rendered: the same bits
    path = str(tmp_path / "stack.npz")
    with_planes.save(path)
    loaded = P.PackedLayers.load(path, device="cuda")
    assert loaded.format == fmt and loaded.shape == (b, h, w, d) and loaded.planes == with_planes.planes
    assert torch.equal(loaded.data, with_planes.data)
    rgb3, dep3 = m.render_views(loaded, pose, pos)
    assert torch.equal(rgb3, rgb) and torch.equal(dep3, dep)
    on_host = P.PackedLayers.load(path)                                        # a host-side stack is moved on the way in
    rgb4, _ = m.render_views(on_host, pose, pos, want_depth=False)
    assert torch.equal(rgb4, rgb)
