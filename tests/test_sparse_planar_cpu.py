"""The edge keep rule of matryodshka_amd/sparse.py (border='edge': the tile's 6 x 18 window clipped to the image, for the planar and cube
viewers, whose samplers never read the opposite border) on the CPU: border='wrap' is today's rule and file, byte for byte; the edge
file is version 2 and today's readers refuse it; edge keep is a subset of wrap keep, equal to it when the outer texel ring is
empty and different in a pinned case; and, by brute force over every footprint of both samplers, a footprint with an in-range tap
in a dropped tile has all in-range alphas zero."""
import io

import numpy as np
import pytest

from matryodshka_amd import packed as P
from matryodshka_amd import sparse as S

FORMATS = list(P.FORMATS)
DTYPE = {'rgba8': np.uint8, 'rgba16f': np.float16}


def blocky_codes(seed, b, d, h, w, fmt, ring=True, p=0.35):
    """Codes [B,D,H,W,4]: random colours everywhere; alpha non-zero inside random 3 x 5 blocks of layers 1.. and, with `ring`, in a few texels of
    the outermost ring (corners included); zero elsewhere.  rgba16f zeros alternate in sign."""
    rng = np.random.RandomState(seed)
    on = np.zeros((b, d, h, w), bool)
    for l in range(1, d):
        for _ in range(2):
            if rng.uniform() < p + 0.3:
                y, x = rng.randint(1, h - 3), rng.randint(1, w - 5)
                on[rng.randint(b), l, y:y + 3, x:x + 5] = True
    if ring:
        on[0, d - 1, 0, 0] = on[b - 1, 1, h - 1, w - 1] = on[0, 1, 0, w // 2] = on[b - 1, d - 1, h // 2, 0] = True
    else:
        on[:, :, 0, :] = on[:, :, -1, :] = on[:, :, :, 0] = on[:, :, :, -1] = False
    if fmt == 'rgba8':
        q = rng.randint(0, 256, size=(b, d, h, w, 4)).astype(np.uint8)
        q[..., 3] = np.where(on, np.maximum(q[..., 3], 1), 0)
    else:
        q = rng.uniform(-1, 1, size=(b, d, h, w, 4)).astype(np.float16)
        zero = np.where(rng.uniform(size=on.shape) < 0.5, np.float16(0.0), np.float16(-0.0))
        q[..., 3] = np.where(on, rng.uniform(0.1, 1.0, size=on.shape).astype(np.float16), zero)
    return q, on


def _bits(a):
    a = np.asarray(a)
    return a.view(np.uint16) if a.dtype == np.float16 else a


def _same(a, b):
    return all(x.dtype == y.dtype and x.shape == y.shape and np.array_equal(_bits(x), _bits(y)) for x, y in zip(a, b))


# ------------------------------------------------------------------------------------------------ 'wrap' is today's behaviour
@pytest.mark.parametrize("fmt", FORMATS)
def test_wrap_is_the_default_bit_for_bit(fmt, tmp_path):
    q, _ = blocky_codes(1, 2, 3, 12, 48, fmt)
    assert np.array_equal(S.keep_np(q, fmt), S.keep_np(q, fmt, border='wrap'))
    assert _same(S.sparsify_np(q, fmt), S.sparsify_np(q, fmt, border='wrap'))
    a, b = S.SparseLayers.from_codes(q, fmt, planes=[3.0, 2.0, 1.0]), S.SparseLayers.from_codes(q, fmt, planes=[3.0, 2.0, 1.0], border='wrap')
    assert a.border == b.border == 'wrap' and a.to("cpu").border == 'wrap'
    assert S.SparseLayers(a.table, a.layer_start, a.pool, fmt).border == 'wrap'
    files = []
    for k, s in enumerate((a, b)):
        path = str(tmp_path / ("wrap%d.npz" % k))
        s.save(path)
        files.append(open(path, "rb").read())
    assert files[0] == files[1]
    with np.load(io.BytesIO(files[0]), allow_pickle=False) as z:
        assert sorted(z.files) == sorted(["sparse_layout_version", "format", "tile_h", "tile_w", "table", "layer_start", "pool", "has_planes", "planes"])
        assert int(z["sparse_layout_version"]) == 1
    assert S.SparseLayers.load(str(tmp_path / "wrap0.npz")).border == 'wrap'
    with pytest.raises(ValueError):
        S.keep_np(q, fmt, border='clamp')
    with pytest.raises(ValueError):
        S.SparseLayers(a.table, a.layer_start, a.pool, fmt, border='zero')


# ------------------------------------------------------------------------------------------------ the edge file
@pytest.mark.parametrize("fmt", FORMATS)
def test_an_edge_stack_round_trips_and_its_file_is_refused_by_readers_of_version_1(fmt, tmp_path):
    q, _ = blocky_codes(2, 2, 3, 12, 48, fmt)
    s = S.SparseLayers.from_codes(q, fmt, planes=[3.0, 2.0, 1.0], border='edge')
    assert s.border == 'edge' and s.to("cpu").border == 'edge'
    assert _same(S.sparsify_np(q, fmt, border='edge'), (s.table.numpy(), s.layer_start.numpy(), s.pool.numpy()))
    path = str(tmp_path / "edge.npz")
    s.save(path)
    back = S.SparseLayers.load(path)
    assert back.border == 'edge' and back.format == fmt and back.planes == s.planes
    assert _same((back.table.numpy(), back.layer_start.numpy(), back.pool.numpy()), (s.table.numpy(), s.layer_start.numpy(), s.pool.numpy()))
    assert np.array_equal(_bits(back.expand_np()), _bits(S.expand_np(*S.sparsify_np(q, fmt, border='edge'), fmt)))      # expand_np knows no rule
    with np.load(path, allow_pickle=False) as z:
        entries = {k: z[k] for k in z.files}
    assert int(entries["sparse_layout_version"]) == 2 and str(entries["border"]) == 'edge'
    assert int(entries["sparse_layout_version"]) != S.LAYOUT_VERSION            # what a reader written for version 1 compares, and refuses
    for change in (lambda e: e.pop("border"), lambda e: e.update(sparse_layout_version=np.int64(3)), lambda e: e.update(border=np.array('wrap'))):
        e = dict(entries)
        change(e)
        bad = str(tmp_path / "bad.npz")
        np.savez(bad, **e)
        with pytest.raises(ValueError):
            S.SparseLayers.load(bad)


# ------------------------------------------------------------------------------------------------ edge against wrap
@pytest.mark.parametrize("fmt", FORMATS)
def test_edge_keep_is_a_subset_of_wrap_keep(fmt):
    strictly = 0
    for seed in range(8):
        q, _ = blocky_codes(10 + seed, 2, 4, 16, 64, fmt)
        edge, wrap = S.keep_np(q, fmt, 'edge'), S.keep_np(q, fmt, 'wrap')
        assert np.all(edge <= wrap) and edge[:, 0].all()
        strictly += int((edge != wrap).any())
    assert strictly > 0


@pytest.mark.parametrize("fmt", FORMATS)
def test_the_rules_agree_when_the_outer_ring_is_empty(fmt):
    for seed in range(4):
        q, on = blocky_codes(30 + seed, 2, 4, 16, 64, fmt, ring=False)
        assert on.any()
        assert np.array_equal(S.keep_np(q, fmt, 'edge'), S.keep_np(q, fmt, 'wrap'))
        assert _same(S.sparsify_np(q, fmt, 'edge'), S.sparsify_np(q, fmt, 'wrap'))


@pytest.mark.parametrize("fmt", FORMATS)
def test_the_pinned_case_one_texel_in_a_corner(fmt):
    q = np.zeros((1, 2, 8, 32, 4), DTYPE[fmt])
    q[0, 1, 0, 0, 3] = 1
    edge, wrap = S.keep_np(q, fmt, 'edge'), S.keep_np(q, fmt, 'wrap')
    assert edge[0, 0].all() and wrap[0, 0].all()
    assert np.array_equal(edge[0, 1], [[True, False], [False, False]])
    assert wrap[0, 1].all() and wrap[0, 1].size == 4
    assert np.array_equal(np.diff(S.sparsify_np(q, fmt, 'edge')[1]), [4, 1]) and np.array_equal(np.diff(S.sparsify_np(q, fmt, 'wrap')[1]), [4, 4])


# ------------------------------------------------------------------------------------------------ sufficiency, by brute force
def _decoded_alpha(q, fmt):
    return P.decode_np(q, fmt)[..., 3]


@pytest.mark.parametrize("h,w", [(8, 32), (12, 48)])
@pytest.mark.parametrize("fmt", FORMATS)
def test_a_footprint_with_a_tap_in_a_dropped_tile_has_zero_alphas(fmt, h, w):
    d = 3
    q, on = blocky_codes(50 + h, 2, d, h, w, fmt)
    keep = S.keep_np(q, fmt, 'edge')
    ring = on.copy()
    ring[:, :, 1:-1, 1:-1] = False
    assert not keep.all() and keep[:, 1:].any() and ring.any()                  # tiles dropped, tiles of layers > 0 kept, texels on the outer ring
    alpha = _decoded_alpha(q, fmt)
    assert np.array_equal(alpha != 0, on)
    kept_texel = np.repeat(np.repeat(keep, S.TILE_H, axis=2), S.TILE_W, axis=3)   # [B,D,H,W]: the texel's tile is kept
    checked = 0
    # planar: every integer footprint origin in [-1, W-1] x [-1, H-1], taps outside the image ignored
    for y0 in range(-1, h):
        for x0 in range(-1, w):
            ys = [y for y in (y0, y0 + 1) if 0 <= y < h]
            xs = [x for x in (x0, x0 + 1) if 0 <= x < w]
            dropped = ~kept_texel[:, :, ys][:, :, :, xs].all(axis=(2, 3))       # [B,D]: some in-range tap lies in a dropped tile
            zero = (alpha[:, :, ys][:, :, :, xs] == 0).all(axis=(2, 3))
            assert np.all(zero[dropped]), (y0, x0)
            checked += int(dropped.sum())
    # cube: every clamped footprint (x0, y0) .. (min(x0 + 1, W - 1), min(y0 + 1, H - 1))
    for y0 in range(h):
        for x0 in range(w):
            ys, xs = sorted({y0, min(y0 + 1, h - 1)}), sorted({x0, min(x0 + 1, w - 1)})
            dropped = ~kept_texel[:, :, ys][:, :, :, xs].all(axis=(2, 3))
            zero = (alpha[:, :, ys][:, :, :, xs] == 0).all(axis=(2, 3))
            assert np.all(zero[dropped]), (y0, x0)
            checked += int(dropped.sum())
    assert checked > 0
    # and the rule is not looser than it has to be at the border: the same check FAILS for a wrapping sampler on this mask
    wrap_violated = False
    for y0 in (-1, h - 1):
        for x0 in range(-1, w):
            ys, xs = [y0 % h, (y0 + 1) % h], [x0 % w, (x0 + 1) % w]
            dropped = ~kept_texel[:, :, ys][:, :, :, xs].all(axis=(2, 3))
            zero = (alpha[:, :, ys][:, :, :, xs] == 0).all(axis=(2, 3))
            wrap_violated |= bool(np.any(~zero[dropped]))
    assert wrap_violated
