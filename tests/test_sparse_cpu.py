"""The numpy rule of sparse layer stacks (matryodshka_amd/sparse.py), without a device: the property the sparse render rests on --
a bilinear footprint with any tap in a dropped tile has four zero alphas --, exhaustively on the torus; known answers of the keep
rule; sparsify / expand consistency; and the .npz round trip with its refusals."""
import numpy as np
import pytest

from matryodshka_amd import sparse as S
from matryodshka_amd.packed import PackedLayers

FORMATS = ['rgba8', 'rgba16f']
DTYPE = {'rgba8': np.uint8, 'rgba16f': np.float16}
BITS = {'rgba8': np.uint8, 'rgba16f': np.uint16}


def _codes(fmt, b, d, h, w, seed, texels_per_layer):
    """Random colours everywhere, alpha zero except at a few random texels per layer (some layers none; rgba16f zeros of both signs)."""
    rng = np.random.RandomState(seed)
    if fmt == 'rgba8':
        q = rng.randint(0, 256, size=(b, d, h, w, 4)).astype(np.uint8)
        q[..., 3] = 0
    else:
        q = rng.uniform(-1, 1, size=(b, d, h, w, 4)).astype(np.float16)
        q[..., 3] = np.where(rng.rand(b, d, h, w) < 0.5, np.float16(0.0), np.float16(-0.0))
    for i in range(b):
        for k in range(d):
            for _ in range(texels_per_layer[(i * d + k) % len(texels_per_layer)]):
                y, x = rng.randint(h), rng.randint(w)
                q[i, k, y, x, 3] = 200 if fmt == 'rgba8' else np.float16(0.75)
    return q


def _zeroed(q, keep):
    """q with the texels of dropped tiles set to all-zero bytes."""
    mask = np.repeat(np.repeat(keep, S.TILE_H, axis=2), S.TILE_W, axis=3)
    out = q.copy()
    out[~mask] = 0
    return out


# (a) ---------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("fmt", FORMATS)
@pytest.mark.parametrize("d,h,w", [(5, 8, 32), (6, 12, 48)])
@pytest.mark.parametrize("seed", [0, 1, 2, 3])
def test_a_footprint_with_a_dropped_tap_has_four_zero_alphas(fmt, d, h, w, seed):
    q = _codes(fmt, 2, d, h, w, seed, texels_per_layer=[1, 0, 2, 3, 1, 5])
    keep = S.keep_np(q, fmt)
    assert keep[:, 0].all()
    dropped = ~np.repeat(np.repeat(keep, S.TILE_H, axis=2), S.TILE_W, axis=3)       # per texel [B,D,H,W]
    empty = q[..., 3] == 0                                                          # (-0.0 == 0)
    taps = [(0, 0), (0, -1), (-1, 0), (-1, -1)]                                     # roll by -1: the neighbour at +1, modulo the size
    any_dropped = np.zeros_like(dropped)
    all_empty = np.ones_like(empty)
    for dy, dx in taps:                                                             # every 2 x 2 footprint of the torus, by its top-left texel
        any_dropped |= np.roll(dropped, (dy, dx), axis=(2, 3))
        all_empty &= np.roll(empty, (dy, dx), axis=(2, 3))
    any_dropped, all_empty = any_dropped[:, 1:], all_empty[:, 1:]                   # layers d >= 1
    assert any_dropped.any() and (~any_dropped).any() and (~all_empty).any()        # (not vacuous)
    assert np.all(all_empty[any_dropped])


# (b) ---------------------------------------------------------------------------------------------------------------------
def _one_texel(fmt, y, x, value=None):
    """[1,2,12,48,4]: layer 0 all-zero alpha, layer 1 one non-empty texel at (y, x) (none when y is None)."""
    q = np.zeros((1, 2, 12, 48, 4), DTYPE[fmt])
    q[..., :3] = 7
    if y is not None:
        q[0, 1, y, x, 3] = (9 if fmt == 'rgba8' else np.float16(0.5)) if value is None else value
    return q


@pytest.mark.parametrize("fmt", FORMATS)
def test_known_answers_at_3x3_tiles(fmt):
    tiles = lambda q: sorted(map(tuple, np.argwhere(S.keep_np(q, fmt)[0, 1]).tolist()))
    q = _one_texel(fmt, None, None)
    assert tiles(q) == []                                                           # an all-empty layer keeps nothing
    assert S.keep_np(q, fmt)[0, 0].sum() == 9                                       # layer 0 keeps all 9 tiles with all-zero alpha
    table, layer_start, pool = S.sparsify_np(q, fmt)
    assert layer_start.tolist() == [0, 9, 9] and pool.shape == (9, 4, 16, 4)
    assert np.array_equal(table[0, 0].reshape(-1), np.arange(9)) and np.all(table[0, 1] == -1)
    assert tiles(_one_texel(fmt, 0, 0)) == [(0, 0), (0, 2), (2, 0), (2, 2)]         # the wrap reaches both axes
    assert tiles(_one_texel(fmt, 3, 15)) == [(0, 0), (0, 1), (1, 0), (1, 1)]
    assert tiles(_one_texel(fmt, 5, 20)) == [(1, 1)]
    assert tiles(_one_texel(fmt, 11, 47)) == [(0, 0), (0, 2), (2, 0), (2, 2)]
    assert tiles(_one_texel(fmt, 4, 17)) == [(0, 1), (1, 1)] and tiles(_one_texel(fmt, 5, 16)) == [(1, 0), (1, 1)]


def test_rgba16f_minus_zero_alpha_is_empty_and_a_denormal_is_not():
    tiles = lambda q: int(S.keep_np(q, 'rgba16f')[0, 1].sum())
    assert tiles(_one_texel('rgba16f', 5, 20, np.float16(-0.0))) == 0
    assert tiles(_one_texel('rgba16f', 5, 20, np.float16(6e-8))) == 1
    assert tiles(_one_texel('rgba16f', 5, 20, np.float16(np.nan))) == 1
    assert int(S.keep_np(_one_texel('rgba8', 5, 20, 1), 'rgba8')[0, 1].sum()) == 1


# (c) ---------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("fmt", FORMATS)
def test_expand_of_sparsify_is_the_stack_with_dropped_tiles_zeroed(fmt):
    b, d, h, w = 2, 6, 12, 48
    q = _codes(fmt, b, d, h, w, 11, texels_per_layer=[1, 0, 2, 3, 1, 5])
    keep = S.keep_np(q, fmt)
    table, layer_start, pool = S.sparsify_np(q, fmt)
    assert table.dtype == np.int32 and table.shape == (b, d, 3, 3)
    assert layer_start.dtype == np.int64 and layer_start.shape == (b * d + 1,) and layer_start[0] == 0
    assert pool.dtype == DTYPE[fmt] and pool.shape == (keep.sum(), 4, 16, 4) and layer_start[-1] == keep.sum()
    assert np.array_equal(table >= 0, keep)
    assert np.array_equal(np.diff(layer_start), keep.reshape(b * d, -1).sum(axis=1))
    for l in range(b * d):                                                          # indices are row-major within each layer
        t = table.reshape(b * d, -1)[l]
        assert np.array_equal(t[t >= 0], np.arange((t >= 0).sum()))
        for k, pos in enumerate(np.flatnonzero(t >= 0)):                            # and tile k of the layer is that tile's texels
            ty, tx = divmod(int(pos), 3)
            src = q.reshape(b * d, h, w, 4)[l, ty * 4:ty * 4 + 4, tx * 16:tx * 16 + 16]
            assert np.array_equal(pool[layer_start[l] + k].view(BITS[fmt]), src.view(BITS[fmt]))
    back = S.expand_np(table, layer_start, pool, fmt)
    assert back.dtype == q.dtype and back.shape == q.shape
    assert np.array_equal(back.view(BITS[fmt]), _zeroed(q, keep).view(BITS[fmt]))
    assert not np.array_equal(back.view(BITS[fmt]), q.view(BITS[fmt]))              # (something was dropped)
    again = S.sparsify_np(back, fmt)                                                # expanding keeps the kept set
    assert all(np.array_equal(x, y) for x, y in zip(again[:2], (table, layer_start)))
    assert np.array_equal(again[2].view(BITS[fmt]), pool.view(BITS[fmt]))


def test_sizes_that_are_not_whole_tiles_are_refused():
    for h, w in ((10, 48), (12, 40)):
        with pytest.raises(ValueError):
            S.sparsify_np(np.zeros((1, 2, h, w, 4), np.uint8), 'rgba8')
    with pytest.raises(ValueError):
        S.sparsify_np(np.zeros((1, 2, 12, 48, 4), np.float16), 'rgba8')            # codes of the other format
    with pytest.raises(ValueError):
        S.sparsify_np(np.zeros((1, 2, 12, 48, 4), np.uint8), 'rgba4')


# (d) ---------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("fmt", FORMATS)
def test_object_and_save_load_round_trip(fmt, tmp_path):
    import torch
    b, d, h, w = 2, 5, 8, 32
    q = _codes(fmt, b, d, h, w, 5, texels_per_layer=[1, 0, 2])
    planes = tuple(float(p) for p in np.linspace(100.0, 1.0, d))
    sp = S.SparseLayers.from_codes(q, fmt, planes)
    table, layer_start, pool = S.sparsify_np(q, fmt)
    assert sp.format == fmt and sp.shape == (b, h, w, d) and sp.planes == planes and sp.tile == (4, 16)
    assert sp.table.dtype == torch.int32 and sp.layer_start.dtype == torch.int64
    assert sp.nbytes == table.nbytes + layer_start.nbytes + pool.nbytes
    assert sp.occupancy == pool.shape[0] / float(b * d * (h // 4) * (w // 16)) and 0 < sp.occupancy < 1
    assert np.array_equal(sp.expand_np().view(BITS[fmt]), S.expand_np(table, layer_start, pool, fmt).view(BITS[fmt]))
    same = S.SparseLayers.from_codes(PackedLayers(q, fmt, planes), None)             # a host-side PackedLayers brings format and planes
    assert same.format == fmt and same.planes == planes and torch.equal(same.pool, sp.pool)
    path = str(tmp_path / "sparse.npz")
    sp.save(path)
    back = S.SparseLayers.load(path)
    assert back.format == fmt and back.shape == sp.shape and back.planes == planes and back.tile == (4, 16)
    assert torch.equal(back.table, sp.table) and torch.equal(back.layer_start, sp.layer_start)
    assert np.array_equal(back.pool.numpy().view(BITS[fmt]), sp.pool.numpy().view(BITS[fmt]))
    assert S.SparseLayers.from_codes(q, fmt).planes is None
    S.SparseLayers.from_codes(q, fmt).save(path)
    assert S.SparseLayers.load(path).planes is None

    with np.load(path, allow_pickle=False) as z:
        fields = {k: z[k] for k in z.files}

    def refused(**change):
        f = dict(fields)
        f.update(change)
        bad = str(tmp_path / "bad.npz")
        with open(bad, "wb") as fh:
            np.savez(fh, **f)
        with pytest.raises(ValueError):
            S.SparseLayers.load(bad)
    refused(sparse_layout_version=np.int64(S.LAYOUT_VERSION + 1))                    # a wrong version
    refused(pool=fields["pool"].astype(np.float32))                                  # a wrong dtype
    refused(pool=fields["pool"].view(np.uint8 if fmt == 'rgba16f' else np.int8))     # the other format's / a signed dtype
    refused(table=fields["table"].astype(np.int64))
    refused(layer_start=fields["layer_start"].astype(np.int32))
    refused(format=np.array("rgba4"))
    refused(tile_w=np.int64(8))
    refused(pool=fields["pool"][:-1])                                                # arrays that do not belong together
    # ... also where the totals still agree: the copy kernels address pool[layer_start[l] + index] unchecked
    counts = np.diff(fields["layer_start"])
    l = 0                                                                            # (layer 0 keeps all its tiles, and others are kept too)
    bad = fields["table"].copy().reshape(b * d, -1)
    bad[l, int(np.argmax(bad[l]))] = counts[l]                                       # one past its own layer, still below T
    assert bad.max() < fields["pool"].shape[0]
    refused(table=bad.reshape(fields["table"].shape))
    bad = fields["table"].copy()
    bad[0, 1, 0, 0] = -2
    refused(table=bad)
    swapped = fields["layer_start"].copy()
    swapped[1] = swapped[-1]                                                         # 0, T, ...: decreasing after it, the ends unchanged
    assert swapped[2] < swapped[1]
    refused(layer_start=swapped)
    shifted = fields["layer_start"].copy()
    shifted[0] = 1
    refused(layer_start=shifted)
    with pytest.raises(ValueError):                                                  # the constructor refuses the same host-side arrays
        S.SparseLayers(fields["table"], swapped, fields["pool"], fmt)
    # a PackedLayers file is not a SparseLayers file, and the other way round
    PackedLayers(q, fmt).save(path)
    with pytest.raises(ValueError):
        S.SparseLayers.load(path)
    sp.save(path)
    with pytest.raises((ValueError, KeyError)):
        PackedLayers.load(path)


def test_constructor_refusals():
    q = _codes('rgba8', 1, 3, 8, 32, 9, texels_per_layer=[1])
    table, layer_start, pool = S.sparsify_np(q, 'rgba8')
    S.SparseLayers(table, layer_start, pool, 'rgba8', planes=(3.0, 2.0, 1.0))
    for args, kw in [((table, layer_start, pool, 'rgba16f'), {}), ((table.astype(np.int64), layer_start, pool, 'rgba8'), {}),
                     ((table, layer_start[:-1], pool, 'rgba8'), {}), ((table, layer_start, pool.reshape(-1, 16, 4, 4), 'rgba8'), {}),
                     ((table, layer_start, pool, 'rgba8'), dict(planes=(1.0, 2.0))), ((table, layer_start, pool, 'rgba8'), dict(tile=(8, 8)))]:
        with pytest.raises(ValueError):
            S.SparseLayers(*args, **kw)
