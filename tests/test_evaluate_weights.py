"""CPU-only: the row-weighted forms of evaluate.ssim / psnr / mae (the host statement of what msi_score_images computes).
With the default row_weights=None every function returns the bits it returned before the keyword existed (restated below from
the unweighted definition); all-ones weights agree with it; a weight vector that selects one row gives that row's mean."""
import numpy as np
import pytest

from matryodshka_amd import evaluate as E


def _images():
    rng = np.random.RandomState(11)
    out = []
    for h, w, c in ((11, 11, 3), (23, 37, 3), (40, 64, 1)):
        yy, xx = np.mgrid[0:h, 0:w]
        base = 127.5 + 100.0 * np.sin(xx / 5.0)[:, :, None] * np.cos(yy / 7.0)[:, :, None] + rng.uniform(-20, 20, (h, w, c))
        a = np.clip(base, 0, 255).astype(np.uint8)
        b = np.clip(a.astype(np.float64) + rng.normal(0, 6, (h, w, c)), 0, 255).astype(np.uint8)
        out.append((a, b))
    return out


def _ssim_map(x, y, max_val=255.0):
    """The lum * cs map of evaluate.ssim, from its own helpers."""
    x, y = np.asarray(x, np.float64), np.asarray(y, np.float64)
    win = E._gauss_window(11, 1.5)
    c1, c2 = (0.01 * max_val) ** 2, (0.03 * max_val) ** 2
    mx, my = E._filter_valid(x, win), E._filter_valid(y, win)
    num0, den0 = mx * my * 2.0, mx * mx + my * my
    lum = (num0 + c1) / (den0 + c1)
    cs = (E._filter_valid(x * y, win) * 2.0 - num0 + c2) / (E._filter_valid(x * x + y * y, win) - den0 + c2)
    return lum * cs


def test_defaults_return_the_unweighted_bits():
    for a, b in _images():
        x, y = a.astype(np.float64), b.astype(np.float64)
        want_ssim = float(_ssim_map(a, b).mean(axis=(0, 1)).mean())
        mse = float(((x - y) ** 2).mean())
        want_psnr = float(20.0 * np.log10(255.0) - 10.0 * np.log10(mse))
        assert E.ssim(a, b, 255.0) == want_ssim == E.ssim(a, b, 255.0, row_weights=None)
        assert E.psnr(a, b, 255.0) == want_psnr == E.psnr(a, b, 255.0, row_weights=None)
        assert E.mae(a, b) == float(np.abs(x - y).mean())
        assert E.psnr(a, a) == float("inf") and E.ssim(a, a) == 1.0 and E.mae(a, a) == 0.0


def test_all_ones_weights_agree_with_unweighted():
    for a, b in _images():
        ones = np.ones(a.shape[0])
        assert abs(E.ssim(a, b, row_weights=ones) - E.ssim(a, b)) <= 1e-12
        assert abs(E.psnr(a, b, row_weights=ones) - E.psnr(a, b)) <= 1e-12
        assert abs(E.mae(a, b, row_weights=ones) - E.mae(a, b)) <= 1e-12


def test_one_hot_weights_give_that_rows_mean():
    for a, b in _images():
        x, y = a.astype(np.float64), b.astype(np.float64)
        h = a.shape[0]
        smap = _ssim_map(a, b)
        for r in sorted({0, 5, h // 2, h - 6, h - 1}):
            wts = np.zeros(h)
            wts[r] = 1.0
            row_mse = ((x[r] - y[r]) ** 2).mean()
            assert abs(E.psnr(a, b, row_weights=wts) - (20.0 * np.log10(255.0) - 10.0 * np.log10(row_mse))) <= 1e-12
            assert abs(E.mae(a, b, row_weights=wts) - np.abs(x[r] - y[r]).mean()) <= 1e-12
            if 5 <= r < h - 5:            # the map row whose window is centred on image row r
                assert abs(E.ssim(a, b, row_weights=wts) - smap[r - 5].mean()) <= 1e-12


def test_weight_vectors_of_the_wrong_length_are_refused():
    a, b = _images()[1]
    for fn in (E.ssim, E.psnr, E.mae):
        with pytest.raises(ValueError):
            fn(a, b, row_weights=np.ones(a.shape[0] + 1))


@pytest.mark.parametrize("h", [1, 2, 11, 40, 320, 2048])
def test_solid_angle_row_weights(h):
    w = E.solid_angle_row_weights(h)
    assert w.shape == (h,) and w.dtype == np.float64
    assert (w > 0).all()
    assert np.allclose(w, w[::-1], rtol=0, atol=1e-15)
    i = np.arange(h)
    assert np.array_equal(w, np.cos((i + 0.5 - h / 2.0) * (np.pi / h)))
    if h >= 11:                           # the midpoint rule of the integral of cos over [-pi/2, pi/2], times h / pi
        assert abs(w.sum() - 2.0 * h / np.pi) <= 0.01 * 2.0 * h / np.pi
