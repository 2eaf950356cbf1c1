"""The sparse high-res stack without a GPU: the shared test inputs (tests/hres_sparse_cases.py) give tile tables that are neither
empty nor full at every shape and format, and the keep rule restated from the low-res alphas alone -- resize, encoder, keep_np --
is the table pattern sparsify_np makes of the same codes.  What the kernels do with these inputs is in
tests/test_gpu_hres_sparse.py, against the dense path."""
import numpy as np
import pytest

from matryodshka_amd import sparse
from tests import hres_sparse_cases as cases


@pytest.mark.parametrize("fmt", cases.FORMATS)
@pytest.mark.parametrize("shape", cases.SHAPES, ids=cases.SHAPE_IDS)
def test_0_masks_are_neither_empty_nor_full(shape, fmt):
    _, al = cases.low_res(shape)
    _, _, hh, hw, d = shape
    keep = cases.restated_keep(al, hh, hw, fmt)
    assert keep.shape == (cases.B, d, hh // sparse.TILE_H, hw // sparse.TILE_W)
    occ = cases.check_masks(keep)
    print("%s %s: occupancy %.3f" % (shape, fmt, occ))
    for layer in (2, 3):                                  # one corner texel: a handful of tiles, through both wraps
        n = keep[:, layer].reshape(cases.B, -1).sum(axis=1)
        assert ((n >= 4) & (n <= 16)).all(), (layer, n)
        assert keep[:, layer, 0, 0].all() and keep[:, layer, -1, -1].all() and keep[:, layer, 0, -1].all() and keep[:, layer, -1, 0].all()
    if d > 4:
        assert not keep[0, d - 1].any() and keep[1, d - 1].all()


@pytest.mark.parametrize("fmt", cases.FORMATS)
@pytest.mark.parametrize("shape", cases.SHAPES, ids=cases.SHAPE_IDS)
def test_restated_keep_is_the_table_pattern_of_sparsify_np(shape, fmt):
    _, al = cases.low_res(shape)
    _, _, hh, hw, d = shape
    codes = cases.restated_codes(al, hh, hw, fmt)
    table, layer_start, pool = sparse.sparsify_np(codes, fmt)
    keep = sparse.keep_np(codes, fmt)
    assert np.array_equal(table >= 0, keep)
    assert int(layer_start[-1]) == int(keep.sum()) == pool.shape[0]
    assert np.array_equal(np.diff(layer_start), keep.reshape(cases.B * d, -1).sum(axis=1))
    assert np.array_equal(sparse.expand_np(table, layer_start, pool, fmt)[..., 3] != 0, (codes[..., 3] != 0) & np.repeat(
        np.repeat(keep, sparse.TILE_H, axis=2), sparse.TILE_W, axis=3))


def test_the_restated_encoders_treat_odd_alphas_as_the_formats_do():
    """-0.0, a negative, > 1, a value too small for the format and NaN: the side of the keep rule each lands on."""
    a = np.array([-0.0, -0.25, 1.5, 1e-9, np.nan, 0.5 / 255 * 0.99, 0.5 / 255 * 1.01, 6e-8, 2e-8], np.float32)
    q8, q16 = cases.alpha_codes_np(a, "rgba8"), cases.alpha_codes_np(a, "rgba16f")
    assert (q8 != 0).tolist() == [False, False, True, False, False, False, True, False, False]
    # (a half keeps a negative, a NaN and a denormal -- 6e-8 rounds to the smallest one -- and loses 1e-9 / 2e-8 to zero; -0.0 != 0 is False)
    assert (q16 != 0).tolist() == [False, True, True, False, True, True, True, True, False]


def test_resize_np_is_the_identity_at_scale_one_and_exact_at_whole_steps():
    rng = np.random.RandomState(3)
    al = rng.uniform(size=(1, 5, 7, 4)).astype(np.float32)
    assert np.array_equal(cases.resize_np(al, 5, 7), al)
    up = cases.resize_np(al, 9, 13)                       # (in - 1) / (out - 1) = 1/2 exactly: every other output is an input
    assert np.array_equal(up[:, ::2, ::2], al)
    assert np.array_equal(up[:, 1, 0], al[:, 0, 0] + (al[:, 1, 0] - al[:, 0, 0]) * np.float32(0.5))
