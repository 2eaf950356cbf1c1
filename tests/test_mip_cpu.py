"""CPU facts of the mip-mapped stacks: the pyramid rule in numpy (matryodshka_amd/mips.py: build_mips_np), the MipLayers container,
and the reason the feature exists -- on the fp64 reference alone (tests/mip_reference.py), a minified trilinear view is several
times closer to the supersampled view than the plain bilinear one.  Nothing here loads the native library."""
import numpy as np
import pytest
import torch

from matryodshka_amd import mips as M
from matryodshka_amd.packed import PackedLayers, decode_np, encode_np
from tests import mip_reference as R

F = np.float32


# ---- build_mips_np -----------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("alpha", [0, 1, 77, 255])
def test_a_constant_rgba8_stack_gives_constant_codes_at_every_level(alpha):
    codes = np.empty((2, 3, 64, 128, 4), np.uint8)
    codes[...] = [200, 3, 128, alpha]
    levels = M.build_mips_np(codes, 'rgba8', 6)
    assert [x.shape for x in levels] == [(2, 3, 64 >> l, 128 >> l, 4) for l in range(1, 6)]
    for x in levels:
        assert x.dtype == np.uint8 and np.all(x == codes[0, 0, 0, 0])


def _one_red_among_green():
    base = np.zeros((1, 2, 2, 2, 4), F)
    base[..., :] = [-1, 1, -1, 0]                      # transparent green
    base[:, :, 1, 0, :] = [1, -1, -1, 1]               # one opaque red texel, in both layers
    return base


def test_a_transparent_texels_colour_does_not_bleed():
    """One opaque red texel among three transparent green ones: a red texel with alpha 1/4 -- not the brown of a plain mean."""
    # (a 2 x 2 level needs a 4 x 4 base: the block in the top-left corner, the rest of the base all green)
    base = np.zeros((1, 2, 4, 4, 4), F)
    base[..., :] = [-1, 1, -1, 0]
    base[:, :, :2, :2, :] = _one_red_among_green()
    (l1,) = M.build_mips_np(base, 'f32', 2)
    assert l1.shape == (1, 2, 2, 2, 4)
    assert np.array_equal(l1[0, 1, 0, 0], np.array([1, -1, -1, 0.25], F))
    # elsewhere in layer 1 nothing is visible: the plain mean, green with alpha 0
    assert np.array_equal(l1[0, 1, 1, 1], np.array([-1, 1, -1, 0], F))
    for fmt in ('rgba8', 'rgba16f'):
        (q,) = M.build_mips_np(encode_np(base, fmt), fmt, 2)
        assert np.array_equal(decode_np(q, fmt)[0, 1, 0, 0, :3], np.array([1, -1, -1], F))


def test_layer_0_takes_the_plain_mean():
    base = np.zeros((1, 2, 4, 4, 4), F)
    base[..., :] = [-1, 1, -1, 0]
    base[:, :, :2, :2, :] = _one_red_among_green()
    (l1,) = M.build_mips_np(base, 'f32', 2)
    assert np.array_equal(l1[0, 0, 0, 0], np.array([-0.5, 0.5, -1, 0.25], F))     # over-compositing ignores layer 0's alpha


def test_alpha_is_the_exact_mean():
    rng = np.random.RandomState(5)
    base = rng.uniform(-1, 1, (2, 3, 64, 64, 4)).astype(F)
    base[..., 3] = rng.randint(0, 257, (2, 3, 64, 64)) / 256.0          # dyadic: every fp32 sum below is exact
    for l, x in enumerate(M.build_mips_np(base, 'f32', 6), start=1):
        n = 1 << l
        exact = base[..., 3].astype(np.float64).reshape(2, 3, 64 // n, n, 64 // n, n).mean(axis=(3, 5))
        assert np.array_equal(x[..., 3].astype(np.float64), exact), l


def test_the_partials_are_not_quantised_between_levels():
    """Level 2 of an rgba8 stack is computed from the partial sums, not from the stored codes of level 1."""
    rng = np.random.RandomState(7)
    codes = rng.randint(0, 256, (1, 2, 8, 8, 4)).astype(np.uint8)
    l1, l2 = M.build_mips_np(codes, 'rgba8', 3)
    x = decode_np(codes, 'rgba8').astype(np.float64)
    a, c = x[..., 3:], x[..., :3]
    A = a.reshape(1, 2, 2, 4, 2, 4, 1).sum(axis=(3, 5))
    P = (a * c).reshape(1, 2, 2, 4, 2, 4, 3).sum(axis=(3, 5))
    want = np.where(A > 0, P / np.where(A > 0, A, 1), c.reshape(1, 2, 2, 4, 2, 4, 3).mean(axis=(3, 5)))
    got = decode_np(l2, 'rgba8')[0, 1, ..., :3]
    assert np.abs(got - want[0, 1]).max() <= 0.5 / 127.5 + 1e-6          # half a code step of the exact value


@pytest.mark.parametrize("shape,levels", [((16, 32), 0), ((16, 32), 7), ((16, 32), -1),         # the level count
                                          ((18, 32), 3), ((16, 30), 3), ((24, 40), 5),         # divisibility by 2^(L-1)
                                          ((16, 32), 5), ((4, 64), 3), ((32, 2), 2), ((32, 64), 6)])   # a top level below 2 x 2
def test_the_size_rule_is_enforced(shape, levels):
    base = np.zeros((1, 2) + shape + (4,), F)
    with pytest.raises(ValueError):
        M.build_mips_np(base, 'f32', levels)
    with pytest.raises(ValueError):
        M.check_levels(shape[0], shape[1], levels)


def test_max_levels():
    assert M.max_levels(16, 32) == 4 and M.max_levels(24, 40) == 4 and M.max_levels(64, 128) == 6 and M.max_levels(2048, 4096) == 6
    assert M.max_levels(30, 70) == 2 and M.max_levels(15, 32) == 1 and M.max_levels(2, 2) == 1
    assert M.build_mips_np(np.zeros((1, 1, 6, 6, 4), F), 'f32', 1) == []


def test_format_and_dtype_are_checked():
    with pytest.raises(ValueError):
        M.build_mips_np(np.zeros((1, 1, 4, 4, 4), F), 'rgba4', 2)
    with pytest.raises(ValueError):
        M.build_mips_np(np.zeros((1, 1, 4, 4, 4), F), 'rgba8', 2)
    with pytest.raises(ValueError):
        M.build_mips_np(np.zeros((1, 4, 4, 4), F), 'f32', 2)


# ---- MipLayers ---------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("fmt", M.FORMATS)
def test_miplayers_levels_shapes_and_round_trip(tmp_path, fmt):
    rng = np.random.RandomState(11)
    base = rng.uniform(-1, 1, (2, 3, 24, 40, 4)).astype(F)
    base[..., 3] = np.abs(base[..., 3])
    planes = [100.0, 3.0, 1.0]
    stored = base if fmt == 'f32' else encode_np(base, fmt)
    mip = M.MipLayers.from_numpy(stored, fmt, 3, planes)
    assert mip.levels == 3 and mip.format == fmt and mip.shape == (2, 24, 40, 3) and mip.planes == (100.0, 3.0, 1.0)
    texel = {'f32': 16, 'rgba8': 4, 'rgba16f': 8}[fmt]
    assert mip.nbytes == 2 * 3 * (24 * 40 + 12 * 20 + 6 * 10) * texel
    want = M.build_mips_np(stored, fmt, 3)
    for l in range(3):
        lv = mip.level(l)
        data = lv.data if isinstance(lv, PackedLayers) else lv
        assert isinstance(lv, PackedLayers) == (fmt != 'f32')
        assert tuple(data.shape) == (2, 3, 24 >> l, 40 >> l, 4)
        assert np.array_equal(data.numpy(), stored if l == 0 else want[l - 1])
        if fmt != 'f32':
            assert lv.format == fmt and lv.planes == mip.planes
    with pytest.raises(ValueError):
        mip.level(3)
    path = str(tmp_path / "mip.npz")
    mip.save(path)
    with np.load(path, allow_pickle=False) as z:
        assert int(z["layout_version"]) == M.LAYOUT_VERSION
    back = M.MipLayers.load(path)
    assert back.levels == 3 and back.format == fmt and back.planes == mip.planes
    assert torch.equal(back.data, mip.data) and torch.equal(back.mips, mip.mips)
    assert back.to("cpu").shape == mip.shape


def test_miplayers_refuses_a_wrong_buffer():
    base = torch.zeros((1, 2, 8, 8, 4))
    with pytest.raises(ValueError):
        M.MipLayers(base, torch.zeros(5), 2)
    with pytest.raises(ValueError):
        M.MipLayers(base, torch.zeros(2 * 16 * 4, dtype=torch.float16), 2)
    with pytest.raises(ValueError):
        M.MipLayers(base, torch.zeros(0), 4)
    assert M.MipLayers(base, torch.zeros(0), 1).nbytes == base.numel() * 4


def test_a_newer_layout_version_is_refused(tmp_path):
    mip = M.MipLayers.from_numpy(np.zeros((1, 1, 4, 4, 4), F), 'f32', 2)
    path = str(tmp_path / "mip.npz")
    mip.save(path)
    with np.load(path) as z:
        arrays = dict(z)
    arrays["layout_version"] = np.int64(M.LAYOUT_VERSION + 1)
    np.savez(path, **arrays)
    with pytest.raises(ValueError):
        M.MipLayers.load(path)


# ---- the reference: its own consistency, and the quality fact ----------------------------------------------------------------------
PLANES = [100.0, 3.0, 1.5, 1.0]
I4 = np.eye(4, dtype=F)


def _pyramid(base, levels):
    return [base] + [x[0] for x in M.build_mips_np(base[None], 'f32', levels)]


def test_one_level_and_a_large_negative_bias_are_the_plain_render():
    base = R.near_nyquist_stack(2, 16, 32, 3)
    pyr = _pyramid(base, 3)
    plain = R.mip_view([base], I4, (0.1, 0.2, -0.1), PLANES[:3], size=(7, 13))
    biased = R.mip_view(pyr, I4, (0.1, 0.2, -0.1), PLANES[:3], size=(7, 13), lod_bias=-64.0)
    assert np.array_equal(plain[0], biased[0]) and np.array_equal(plain[1], biased[1])
    top = R.mip_view(pyr, I4, (0.1, 0.2, -0.1), PLANES[:3], size=(7, 13), lod_bias=64.0, return_lod=True)
    assert np.all(top[2] == 2.0)


def test_a_single_row_or_column_has_no_neighbour_on_that_axis():
    assert list(R.neighbour(1)) == [0] and list(R.neighbour(4)) == [1, 2, 3, 2]
    base = R.near_nyquist_stack(2, 16, 32, 3)
    for size in ((1, 9), (9, 1)):
        rgb, dep, lam = R.mip_view(_pyramid(base, 3), I4, (0, 0, 0), PLANES[:3], size=size, return_lod=True)
        assert rgb.shape == size + (3,) and np.all(np.isfinite(rgb)) and np.all((lam >= 0) & (lam <= 2))


@pytest.mark.parametrize("size", [(16, 32), (20, 40)])                                    # 4 x and 3.2 x minification of 64 x 128
@pytest.mark.parametrize("pos", [(0.0, 0.0, 0.0), (0.3, -0.2, 0.25)])
def test_trilinear_is_closer_to_the_supersampled_view_than_bilinear(size, pos):
    """The quality fact, on the fp64 reference alone: against an 8 x 8 supersampled bilinear render of a 64 x 128 x 4 stack with
    near-Nyquist content, the trilinear render's RMS error is at most half the plain bilinear render's.  Measured (rgb; bilinear
    RMS, trilinear RMS, ratio):
        16 x 32  centre      0.136  0.0074  0.054        16 x 32  translated  0.191  0.0212  0.111
        20 x 40  centre      0.286  0.0323  0.113        20 x 40  translated  0.292  0.0390  0.134
    (and 24 x 40: 0.116 / 0.137).  The statement is about rgb; the depth image is printed, not gated (its layer fractions are
    not a signal that aliases the same way: at 20 x 40, centre, trilinear depth is 0.015 against 0.009)."""
    base = R.near_nyquist_stack(3)
    pyr = _pyramid(base, 4)
    sup, sup_d = R.supersampled_view(base, I4, pos, PLANES, 'equirect', size)
    bi, bi_d = R.mip_view([base], I4, pos, PLANES, size=size)
    tri, tri_d = R.mip_view(pyr, I4, pos, PLANES, size=size)

    def rms(a, b):
        return float(np.sqrt(np.mean((a - b) ** 2)))
    print("size %s pos %s: bilinear %.4f trilinear %.4f ratio %.3f | depth %.4f %.4f" % (
        size, pos, rms(bi, sup), rms(tri, sup), rms(tri, sup) / rms(bi, sup), rms(bi_d, sup_d), rms(tri_d, sup_d)))
    assert rms(bi, sup) > 0.1                                    # the defect is there
    assert rms(tri, sup) <= 0.5 * rms(bi, sup)
