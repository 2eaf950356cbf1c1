"""The device scorer (MSI.score_views / score_consecutive -> msi_score_images) against matryodshka_amd/evaluate.py on the host,
fed the same values: uint8 arrays, MSI.deprocess_image / deprocess_depth_image output for quantised fp32 images, the fp64
transform for unquantised ones.  Every pair of every case is compared.

Tolerances (derived, not measured):
  * SSIM, and mae / mse of unquantised fp32 images: |device - host| <= 1e-9.  Both sides are fp64; the error bound of an SSIM
    map value is about 3e-12 (22 taps on values up to 65025, then a division by a denominator >= c2 = 58.5), and a tiled fp64
    restatement with another summation order differed from evaluate.ssim by at most 1.9e-14 on the CPU.
  * uint8 and quantised images: the squared and absolute errors are integers and their sums stay below 2^53, so every partial
    sum is exact in any order and mse / mae must EQUAL numpy's fp64 mean; psnr (two log10) within 1e-9 dB.
The tile of the kernel is 16 rows x 32 columns of SSIM-map positions (TH, TW below): the size sweep runs through one window
position, two, a tile boundary +- 1 and more than one tile in each direction."""
import numpy as np
import pytest

pytestmark = pytest.mark.gpu

TH, TW = 16, 32
TOL = 1e-9


@pytest.fixture(scope="module")
def model():
    from matryodshka_amd import MSI
    return MSI()


def _pattern(rng, h, w, c, noise=25.0):
    """uint8 pair: a smooth pattern + noise, and the same + small noise -- SSIM lands mid-range."""
    yy, xx = np.mgrid[0:h, 0:w]
    base = 127.5 + 70.0 * np.sin(xx / 3.0 + 0.3)[:, :, None] * np.cos(yy / 4.0)[:, :, None] + np.arange(c)[None, None, :] * 9.0
    a = np.clip(base + rng.normal(0, 25.0, (h, w, c)), 0, 255).astype(np.uint8)
    b = np.clip(a.astype(np.float64) + rng.normal(0, noise, (h, w, c)), 0, 255).astype(np.uint8)
    return a, b


def _dev(model, a):
    import torch
    return torch.from_numpy(np.ascontiguousarray(a)).to(model.device)


def _host(pred, tgt, with_ssim=True, weights=None):
    from matryodshka_amd import evaluate as E
    x, y = np.asarray(pred, np.float64), np.asarray(tgt, np.float64)
    if weights is None:
        mse, mae = float(((x - y) ** 2).mean()), float(np.abs(x - y).mean())
    else:
        mse, mae = E._weighted_mean((x - y) ** 2, weights), E.mae(x, y, row_weights=weights)
    out = {"mse": mse, "mae": mae, "psnr": E.psnr(x, y, 255.0, row_weights=weights)}
    if with_ssim:
        out["ssim"] = E.ssim(x, y, 255.0, row_weights=weights)
    return out


def _check(got, want, exact, what):
    """got: dict of python floats from the device; want: _host's dict."""
    print(what, {k: (got[k], want[k]) for k in sorted(want)})
    for k in ("mse", "mae"):
        if exact:
            assert got[k] == want[k], (what, k, got[k], want[k])
        else:
            assert abs(got[k] - want[k]) <= TOL, (what, k, got[k], want[k])
    if np.isinf(want["psnr"]):
        assert got["psnr"] == want["psnr"], what
    else:
        assert abs(got["psnr"] - want["psnr"]) <= TOL, (what, got["psnr"], want["psnr"])
    if "ssim" in want:
        assert abs(got["ssim"] - want["ssim"]) <= TOL, (what, got["ssim"], want["ssim"])


def _floats(scores, index=()):
    return {k: float(v[index]) for k, v in scores.items()}


ALL = ("psnr", "ssim", "mae")


def test_size_sweep_through_the_tiling(model):
    """C = 1, uint8: every W from 11 to 2 TW + 12 at H = 12, every H from 11 to 2 TH + 12 at W = 23."""
    rng = np.random.RandomState(5)
    shapes = [(12, w) for w in range(11, 2 * TW + 13)] + [(h, 23) for h in range(11, 2 * TH + 13)]
    assert (12, 76) in shapes and (44, 23) in shapes and len(shapes) == 100
    pairs = [_pattern(rng, h, w, 1) for h, w in shapes]
    scores = [model.score_views(_dev(model, a), _dev(model, b), metrics=ALL) for a, b in pairs]      # 100 launches, one wait
    mid = 0
    for (h, w), (a, b), s in zip(shapes, pairs, scores):
        want = _host(a, b)
        _check(_floats(s), want, True, "%dx%d" % (h, w))
        mid += 0.05 < want["ssim"] < 0.98
    assert mid >= 90           # (the pattern is meant to land SSIM mid-range, where an error would show)


@pytest.mark.parametrize("h,w", [(11, 11), (27, 43), (37, 45), (64, 80)])
def test_every_pixel_is_counted_exactly_once(model, h, w):
    """pred = target + 1 everywhere: a halo counted twice or a trailing strip left out gives another integer than 1."""
    rng = np.random.RandomState(h * 100 + w)
    t = rng.randint(0, 255, size=(h, w, 3)).astype(np.uint8)
    p = (t + 1).astype(np.uint8)
    got = _floats(model.score_views(_dev(model, p), _dev(model, t), metrics=ALL))
    assert got["mse"] == 1.0 and got["mae"] == 1.0
    assert abs(got["psnr"] - 20.0 * np.log10(255.0)) <= TOL
    _check(got, _host(p, t), True, "plus one %dx%d" % (h, w))
    # ... and with row weights the weighted means of a constant are that constant (to rounding)
    got = _floats(model.score_views(_dev(model, p), _dev(model, t), metrics=("psnr", "mae"), row_weights="solid_angle"))
    assert abs(got["mse"] - 1.0) <= 1e-12 and abs(got["mae"] - 1.0) <= 1e-12


@pytest.mark.parametrize("h,w", [(1, 1), (3, 10), (10, 200)])
def test_psnr_only_below_the_window_size(model, h, w):
    rng = np.random.RandomState(h + w)
    a, b = _pattern(rng, h, w, 3)
    s = model.score_views(_dev(model, a), _dev(model, b), metrics=("psnr", "mae"))
    assert sorted(s) == ["mae", "mse", "psnr"]
    _check(_floats(s), _host(a, b, with_ssim=False), True, "small %dx%d" % (h, w))
    with pytest.raises(ValueError, match="%d x %d" % (h, w)):
        model.score_views(_dev(model, a), _dev(model, b), metrics=("psnr", "ssim"))
    with pytest.raises(ValueError):
        model.score_views(_dev(model, a), _dev(model, b))               # the default metrics include SSIM


def test_identical_images(model):
    import torch
    rng = np.random.RandomState(2)
    for h, w, c in ((11, 11, 1), (24, 31, 3), (37, 45, 3), (48, 70, 4)):
        a, _ = _pattern(rng, h, w, c)
        f = _dev(model, rng.uniform(-1.2, 1.2, size=(h, w, c)).astype(np.float32))
        runs = [model.score_views(_dev(model, a), _dev(model, a), metrics=ALL),
                model.score_views(f, f.clone(), metrics=ALL, transform="image", quantize=True),
                model.score_views(f, f.clone(), metrics=ALL, transform="image", quantize=False),
                model.score_views(f, f.clone(), metrics=ALL, transform="raw", quantize=False),
                model.score_views(_dev(model, a), _dev(model, a), metrics=ALL, row_weights="solid_angle")]
        for s in runs:
            got = _floats(s)
            assert got["mse"] == 0.0 and got["mae"] == 0.0 and got["psnr"] == float("inf"), got
        for s in runs[:4]:
            assert float(s["ssim"]) == 1.0
        assert abs(float(runs[4]["ssim"]) - 1.0) <= 1e-12       # (a weighted sum of ones over the sum of the weights)
        assert all(v.dtype == torch.float64 and v.device == model.device and v.shape == () for s in runs for v in s.values())


@pytest.mark.parametrize("quantize", [True, False])
@pytest.mark.parametrize("transform", ["image", "depth"])
def test_fp32_paths(model, transform, quantize):
    """37 x 45 x 3, values partly outside [-1, 1] (and [0, 1]) so that the clamp matters; quantised: a NaN pixel is level 0."""
    import torch
    rng = np.random.RandomState(17)
    h, w, c = 37, 45, 3
    x = rng.uniform(-1.3, 1.3, size=(h, w, c)).astype(np.float32)
    y = (x + rng.normal(0, 0.05, size=x.shape)).astype(np.float32)
    if quantize:
        x[3, 4, 1] = np.nan
        y[20, 44, 2] = np.nan
        x[36, 0, 0] = np.inf
    xd, yd = _dev(model, x), _dev(model, y)
    got = _floats(model.score_views(xd, yd, metrics=ALL, transform=transform, quantize=quantize))
    if quantize:
        dep = model.deprocess_image if transform == "image" else model.deprocess_depth_image
        hx, hy = dep(xd).cpu().numpy(), dep(yd).cpu().numpy()
        assert hx[3, 4, 1] == 0 and hy[20, 44, 2] == 0 and hx[36, 0, 0] == 255
        assert hx.min() == 0 and hx.max() == 255                # both clamps are exercised
    else:
        hx, hy = ((v.astype(np.float64) + 1.0) / 2.0 * 255.0 if transform == "image" else v.astype(np.float64) * 255.0 for v in (x, y))
    _check(got, _host(hx, hy), quantize, "%s quantize=%s" % (transform, quantize))
    # 'raw' on the values themselves
    raw = _floats(model.score_views(_dev(model, np.nan_to_num(x, nan=0.0, posinf=1.0)), _dev(model, np.nan_to_num(y)), metrics=ALL,
                                    transform="raw", quantize=True))          # (quantize has no meaning for raw values and is dropped)
    _check(raw, _host(np.nan_to_num(x, nan=0.0, posinf=1.0), np.nan_to_num(y)), False, "raw")


def _native_score(model, pred, target, group, fill=0xFF, metrics=7):
    """msi_score_images called directly, on a workspace of `fill` bytes: [n_pairs, 4] as numpy."""
    import torch
    from matryodshka_amd import _native as N
    n = pred.shape[0]
    h, w, c = pred.shape[-3:]
    dtype = N.MSI_SCORE_U8 if pred.dtype == torch.uint8 else N.MSI_SCORE_F32
    transform, quantize = (N.MSI_SCORE_RAW, 0) if pred.dtype == torch.uint8 else (N.MSI_SCORE_IMAGE, 1)
    nbytes = N.lib.msi_score_workspace_bytes(n, h, w, c)
    ws = torch.full((nbytes,), fill, dtype=torch.uint8, device=model.device)
    out = torch.full((n, 4), -7.0, dtype=torch.float64, device=model.device)
    N.check(N.lib.msi_score_images(pred.data_ptr(), target.data_ptr(), dtype, transform, quantize, n, group, h, w, c, None, 255.0, metrics,
                                   out.data_ptr(), ws.data_ptr(), nbytes, torch.cuda.current_stream(model.device).cuda_stream), "msi_score_images")
    return out.cpu().numpy()


def _bits(a):
    return np.ascontiguousarray(a, dtype=np.float64).view(np.int64)


def test_grouping_equals_one_to_one_calls(model):
    rng = np.random.RandomState(23)
    b, v, h, w, c = 3, 5, 24, 31, 3
    tgt = rng.uniform(-1, 1, size=(b, h, w, c)).astype(np.float32)
    pred = (tgt[:, None] + rng.normal(0, 0.08, size=(b, v, h, w, c))).astype(np.float32)
    pd, td = _dev(model, pred), _dev(model, tgt)
    grouped = {k: s.cpu().numpy() for k, s in model.score_views(pd, td, metrics=ALL).items()}
    single = {k: s.cpu().numpy() for k, s in model.score_views(pd, td[1], metrics=ALL).items()}
    assert all(s.shape == (b, v) for s in grouped.values()) and all(s.shape == (b, v) for s in single.values())
    p8, t8 = model.deprocess_image(pd).cpu().numpy(), model.deprocess_image(td).cpu().numpy()
    for i in range(b):
        for j in range(v):
            one = _floats(model.score_views(pd[i, j], td[i], metrics=ALL))
            one1 = _floats(model.score_views(pd[i, j], td[1], metrics=ALL))
            for k in one:
                assert _bits(grouped[k][i, j]) == _bits(one[k]) and _bits(single[k][i, j]) == _bits(one1[k]), (i, j, k)
            _check({k: float(grouped[k][i, j]) for k in grouped}, _host(p8[i, j], t8[i]), True, "group %d %d" % (i, j))
            _check({k: float(single[k][i, j]) for k in single}, _host(p8[i, j], t8[1]), True, "single %d %d" % (i, j))
    # a target batch that is no prefix, other dtypes, another device
    import torch
    for bad_p, bad_t in ((pd, td[:2]), (pd, td[:, :, :30]), (pd, td.double()), (pd, td.cpu()), (pd, model.deprocess_image(td))):
        with pytest.raises((ValueError, TypeError)):
            model.score_views(bad_p, bad_t)
    with pytest.raises(ValueError, match=r"\(3, 5, 24, 31, 3\).*\(2, 24, 31, 3\)"):
        model.score_views(pd, td[:2])


@pytest.mark.parametrize("kind", ["u8", "f32"])
def test_a_pair_scores_the_same_bits_alone_among_65_and_twice(model, kind):
    """The workspace arrives as 0xFF bytes (NaNs): nothing may be read before it is written; no atomics, fixed orders."""
    rng = np.random.RandomState(31)
    n, h, w, c = 65, 24, 31, 3
    if kind == "u8":
        t = rng.randint(0, 256, size=(n, h, w, c)).astype(np.uint8)
        p = np.clip(t.astype(np.int64) + rng.randint(-9, 10, size=t.shape), 0, 255).astype(np.uint8)
    else:
        t = rng.uniform(-1, 1, size=(n, h, w, c)).astype(np.float32)
        p = (t + rng.normal(0, 0.03, size=t.shape)).astype(np.float32)
    pd, td = _dev(model, p), _dev(model, t)
    many = _native_score(model, pd, td, 1)
    again = _native_score(model, pd, td, 1, fill=0x00)
    assert np.isfinite(many).all() and np.array_equal(_bits(many), _bits(again))
    for k in (0, 1, 31, 63, 64):
        alone = _native_score(model, pd[k:k + 1], td[k:k + 1], 1)
        assert np.array_equal(_bits(alone[0]), _bits(many[k])), k
    against_one = _native_score(model, pd, td[7:8], n)          # group = n_pairs: everything against one image
    assert np.array_equal(_bits(against_one[7]), _bits(many[7]))
    # what is not requested is NaN, what is requested keeps its bits
    only = _native_score(model, pd, td, 1, metrics=2)
    assert np.isnan(only[:, [0, 2, 3]]).all() and np.array_equal(_bits(only[:, 1]), _bits(many[:, 1]))
    only = _native_score(model, pd, td, 1, metrics=1)
    assert np.isnan(only[:, [1, 2]]).all() and np.array_equal(_bits(only[:, [0, 3]]), _bits(many[:, [0, 3]]))
    hp, ht = (p, t) if kind == "u8" else (model.deprocess_image(pd).cpu().numpy(), model.deprocess_image(td).cpu().numpy())
    for k in range(n):
        _check(dict(zip(("mse", "mae", "ssim", "psnr"), many[k])), _host(hp[k], ht[k]), True, "pair %d" % k)


@pytest.mark.parametrize("weights", ["solid_angle", "random"])
def test_row_weights(model, weights):
    from matryodshka_amd import evaluate as E
    rng = np.random.RandomState(41)
    h, w, c = 40, 64, 3
    a, b = _pattern(rng, h, w, c)
    wts = E.solid_angle_row_weights(h) if weights == "solid_angle" else rng.uniform(0.1, 3.0, size=h)
    arg = "solid_angle" if weights == "solid_angle" else _dev(model, wts)
    got = _floats(model.score_views(_dev(model, a), _dev(model, b), metrics=ALL, row_weights=arg))
    want = _host(a, b, weights=wts)
    _check(got, want, False, "weights %s" % weights)
    plain = _host(a, b)
    assert abs(want["ssim"] - plain["ssim"]) > 1e-6 and abs(want["psnr"] - plain["psnr"]) > 1e-6      # (the weights matter here)
    if weights == "random":
        got_np = _floats(model.score_views(_dev(model, a), _dev(model, b), metrics=ALL, row_weights=wts))       # host weights are uploaded
        assert got_np == got
        with pytest.raises(ValueError):
            model.score_views(_dev(model, a), _dev(model, b), row_weights=wts[:-1])


def test_score_consecutive(model):
    from matryodshka_amd import evaluate as E
    rng = np.random.RandomState(43)
    frames = np.cumsum(rng.normal(0, 0.05, size=(6, 24, 31, 3)), axis=0).astype(np.float32)
    fd = _dev(model, frames)
    got = model.score_consecutive(fd)
    assert tuple(got.shape) == (5,)
    f8 = model.deprocess_image(fd).cpu().numpy()
    for i in range(5):
        a, b = f8[i].astype(np.float64), f8[i + 1].astype(np.float64)
        assert float(got[i]) == float(np.abs(a - b).mean()) == E.mae(f8[i], f8[i + 1]), i
    d8 = model.deprocess_depth_image(fd).cpu().numpy()
    got = model.score_consecutive(fd, transform="depth")
    assert [float(v) for v in got] == [E.mae(d8[i], d8[i + 1]) for i in range(5)]
    got = model.score_consecutive(fd, quantize=False)
    x = (frames.astype(np.float64) + 1.0) / 2.0 * 255.0
    assert max(abs(float(got[i]) - E.mae(x[i], x[i + 1])) for i in range(5)) <= TOL
    assert [float(v) for v in model.score_consecutive(_dev(model, f8))] == [E.mae(f8[i], f8[i + 1]) for i in range(5)]


@pytest.mark.parametrize("c", [4, 2])
def test_other_channel_counts(model, c):
    rng = np.random.RandomState(c)
    a, b = _pattern(rng, 13, 17, c)
    _check(_floats(model.score_views(_dev(model, a), _dev(model, b), metrics=ALL)), _host(a, b), True, "C=%d" % c)
