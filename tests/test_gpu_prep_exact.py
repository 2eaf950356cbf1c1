"""K5 (pre/deprocess, geo_prep.hip) on the SAME floats as the oracle, equal bytes.  Every PNG the harness writes and every quantised PSNR / SSIM goes through
deprocess_kernel's expression; the other tests meet it only on rendered images whose float inputs already differ between device and oracle (+-1 level on
< 0.1 % of pixels), or against the scorer's copy of the same device expression.

Inputs, one flat fp32 tensor: all 65536 floats whose low 16 bits are zero (+-0, denormals, +-inf, NaNs); for every level boundary k = 0..256 its pre-image
(k / 255.5 for depth images, 2 k / 255.5 - 1 for images) and the four floats on either side of it -- and, for images, the four values on either side in
steps of 2^-23, the spacing of x + 1: near x = 0 the nine neighbouring floats all give one x + 1 and 29 of the boundaries would not be straddled; 2^17
seeded uniform values in [-1.25, 1.25]."""
import numpy as np
import pytest

pytestmark = pytest.mark.gpu

F = np.float32
U8_SENTINEL, F32_SENTINEL, TAIL = 0xA5, 7.0, 64


def _neighbours(x, n=4):
    out = [x]
    lo = hi = x
    for _ in range(n):
        lo, hi = np.nextafter(lo, F(-np.inf)), np.nextafter(hi, F(np.inf))
        out += [lo, hi]
    return out


def _steps(x, n=4):
    """x and n values on either side of it in steps of 2^-23 (the spacing of the floats in [1, 2): of x + 1 for x in [0, 1))."""
    return [F(x + F(j * 2.0 ** -23)) for j in range(-n, n + 1)]


def _boundaries():
    vals = []
    for k in range(257):
        for pre in (F(k / 255.5), F(2.0 * k / 255.5 - 1.0)):
            vals += _neighbours(pre)
    for k in range(257):
        vals += _steps(F(2.0 * k / 255.5 - 1.0))
    return np.array(vals, dtype=F)


def _inputs():
    every = (np.arange(65536, dtype=np.uint32) << 16).view(F)
    rng = np.random.RandomState(5)
    x = np.concatenate([every, _boundaries(), rng.uniform(-1.25, 1.25, size=1 << 17).astype(F)])
    assert np.isnan(x).sum() == 2 * 127 and np.isinf(x).sum() == 2 and x.dtype == F
    return x


@pytest.fixture(scope="module")
def gpu():
    import torch
    assert torch.cuda.is_available(), "GPU tests need a HIP device"
    from matryodshka_amd import MSI, _native as N
    from oracle.msi import MSI as OracleMSI
    x = _inputs()
    return torch, MSI(), OracleMSI(), N, x, torch.from_numpy(x).cuda()


def _oracle_levels(o, x, depth):
    """The oracle's bytes where x is a number; what the kernel defines where the oracle's cast is undefined: 0 for NaN (and -inf), 255 for +inf."""
    finite = np.where(np.isnan(x), F(0), x)
    with np.errstate(all="ignore"):
        want = (o.deprocess_depth_image if depth else o.deprocess_image)(finite)
    want = np.where(np.isnan(x), np.uint8(0), want)
    assert np.all(want[x == np.inf] == 255) and np.all(want[x == -np.inf] == 0)
    return want.astype(np.uint8)


def _assert_levels(got, want, x, what):
    bad = np.flatnonzero(got != want)
    assert bad.size == 0, (what, bad.size, [(float(x[i]), x[i:i + 1].view(np.uint32)[0], int(got[i]), int(want[i])) for i in bad[:5]])


def test_deprocess_equals_the_oracle_on_the_same_floats(gpu):
    torch, m, o, N, x, xt = gpu
    want_img, want_dep = _oracle_levels(o, x, False), _oracle_levels(o, x, True)
    assert len(set(want_img.tolist())) == 256 and len(set(want_dep.tolist())) == 256             # every level is asked for
    _assert_levels(m.deprocess_image(xt).cpu().numpy(), want_img, x, "deprocess_image")
    _assert_levels(m.deprocess_depth_image(xt).cpu().numpy(), want_dep, x, "deprocess_depth_image")
    # the pair kernel: the image half and the depth half, on the same floats and on different ones
    rev = torch.flip(xt, dims=(0,)).contiguous()
    for rgb, dep, w_rgb, w_dep in ((xt, xt, want_img, want_dep), (xt, rev, want_img, want_dep[::-1]), (rev, xt, want_img[::-1], want_dep)):
        got_rgb, got_dep = m.deprocess_image_and_depth(rgb, dep)
        _assert_levels(got_rgb.cpu().numpy(), w_rgb, rgb.cpu().numpy(), "pair, image half")
        _assert_levels(got_dep.cpu().numpy(), w_dep, dep.cpu().numpy(), "pair, depth half")


def test_level_boundaries_sit_where_the_pre_images_say(gpu):
    """The oracle itself: around each pre-image the level steps from k - 1 to k within the nine values (so the inputs do straddle every boundary)."""
    torch, m, o, N, x, xt = gpu
    for k in range(1, 256):
        for depth, around in ((True, _neighbours(F(k / 255.5))), (False, _steps(F(2.0 * k / 255.5 - 1.0)))):
            lv = _oracle_levels(o, np.array(sorted(around), dtype=F), depth)
            assert lv[0] == k - 1 and lv[-1] == k and np.all(np.diff(lv.astype(int)) >= 0), (depth, k, lv)


def test_preprocess_equals_the_oracle_on_the_same_floats_and_bytes(gpu):
    torch, m, o, N, x, xt = gpu
    got = m.preprocess_image(xt).cpu().numpy()
    with np.errstate(all="ignore"):
        want = o.preprocess_image(x)
    assert got.dtype == want.dtype == F
    nan = np.isnan(want)
    assert np.array_equal(np.isnan(got), nan) and nan.sum() == 2 * 127
    assert np.array_equal(got[~nan].view(np.uint32), want[~nan].view(np.uint32))
    a = np.arange(256, dtype=np.uint8)
    b = a[::-1].copy()
    ga = m.preprocess_image(torch.from_numpy(a)).cpu().numpy()
    assert np.array_equal(ga.view(np.uint32), o.preprocess_image(a).view(np.uint32))
    p0, p1 = m.preprocess_image_pair(torch.from_numpy(a), torch.from_numpy(b))
    assert np.array_equal(p0.cpu().numpy().view(np.uint32), ga.view(np.uint32))
    assert np.array_equal(p1.cpu().numpy().view(np.uint32), o.preprocess_image(b).view(np.uint32))


@pytest.mark.parametrize("n", [1, 255, 256, 257])
def test_sizes_through_the_c_abi_write_n_elements_and_no_more(gpu, n):
    torch, m, o, N, x, xt = gpu
    lo = 65536 + 9 * 2 * 100                                   # from the pre-images of level 100 on
    f0, f1 = xt[lo:lo + n].contiguous(), xt[lo + 300:lo + 300 + n].contiguous()
    x0, x1 = x[lo:lo + n], x[lo + 300:lo + 300 + n]
    u0 = torch.arange(n, dtype=torch.int32).to(torch.uint8).cuda()
    u1 = torch.flip(u0, dims=(0,)).contiguous()

    def u8():
        return torch.full((n + TAIL,), U8_SENTINEL, dtype=torch.uint8, device="cuda")

    def f32():
        return torch.full((n + TAIL,), F32_SENTINEL, dtype=torch.float32, device="cuda")

    outs = {}
    for depth in (0, 1):
        outs["deprocess", depth] = out = u8()
        N.check(N.lib.msi_deprocess_f32_u8(f0.data_ptr(), out.data_ptr(), n, depth, None), "msi_deprocess_f32_u8")
    outs["pair_rgb"], outs["pair_depth"] = u8(), u8()
    N.check(N.lib.msi_deprocess_pair_f32_u8(f0.data_ptr(), f1.data_ptr(), outs["pair_rgb"].data_ptr(), outs["pair_depth"].data_ptr(), n, None), "msi_deprocess_pair_f32_u8")
    outs["pre_f32"] = f32()
    N.check(N.lib.msi_preprocess_f32(f0.data_ptr(), outs["pre_f32"].data_ptr(), n, None), "msi_preprocess_f32")
    outs["pre_u8"] = f32()
    N.check(N.lib.msi_preprocess_u8_f32(u0.data_ptr(), outs["pre_u8"].data_ptr(), n, None), "msi_preprocess_u8_f32")
    outs["pre_pair0"], outs["pre_pair1"] = f32(), f32()
    N.check(N.lib.msi_preprocess_pair_u8_f32(u0.data_ptr(), u1.data_ptr(), outs["pre_pair0"].data_ptr(), outs["pre_pair1"].data_ptr(), n, None), "msi_preprocess_pair_u8_f32")
    torch.cuda.synchronize()
    want = {("deprocess", 0): _oracle_levels(o, x0, False), ("deprocess", 1): _oracle_levels(o, x0, True),
            "pair_rgb": _oracle_levels(o, x0, False), "pair_depth": _oracle_levels(o, x1, True),
            "pre_f32": o.preprocess_image(x0), "pre_u8": o.preprocess_image(u0.cpu().numpy()),
            "pre_pair0": o.preprocess_image(u0.cpu().numpy()), "pre_pair1": o.preprocess_image(u1.cpu().numpy())}
    for key, out in outs.items():
        got = out.cpu().numpy()
        assert np.array_equal(got[:n], want[key]), key
        assert np.all(got[n:] == (U8_SENTINEL if got.dtype == np.uint8 else F32_SENTINEL)), key
