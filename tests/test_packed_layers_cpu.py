"""The compact layer formats in numpy (matryodshka_amd/packed.py): the rgba8 rule's exact properties, rgba16f, and the .npz
round trip of a PackedLayers.  No GPU and no native library."""
import numpy as np
import pytest

from matryodshka_amd import packed as P
from tests.util import random_rgba

F = np.float32
CODES = np.arange(256, dtype=np.uint8)


def _table():
    """decode_np of every code in every channel: [256,4]."""
    return P.decode_np(np.repeat(CODES[:, None], 4, axis=1), 'rgba8')


def test_formats_and_constants():
    assert P.FORMATS == ('rgba8', 'rgba16f')
    assert float(P.KC).hex() == '0x1.0101020000000p-7' and float(P.KA).hex() == '0x1.0101020000000p-8'
    with pytest.raises(ValueError):
        P.encode_np(np.zeros((1, 4), F), 'rgba4')
    with pytest.raises(ValueError):
        P.decode_np(np.zeros((1, 4), np.uint8), 'rgba16f')     # wrong code dtype for the format


def test_rgba8_end_codes_are_exact():
    t = _table()
    assert t.dtype == F
    assert np.all(t[0, :3] == F(-1)) and np.all(t[255, :3] == F(1))
    assert t[0, 3] == F(0) and t[255, 3] == F(1)


def test_rgba8_colour_is_antisymmetric_and_tables_increase():
    t = _table()
    for c in range(3):
        assert np.array_equal(t[::-1, c], -t[:, c])
    assert np.all(np.diff(t.astype(np.float64), axis=0) > 0)


def test_rgba8_encode_of_decode_is_the_identity():
    q = np.repeat(CODES[:, None], 4, axis=1)
    assert np.array_equal(P.encode_np(P.decode_np(q, 'rgba8'), 'rgba8'), q)


def test_rgba8_ties_round_to_even():
    """Inputs whose scaled value is exactly k + 0.5 in fp32: alpha (k + 0.5) / 255 does not hit the tie exactly in general, so
    the ties are built backwards from the scaled value and kept only where the fp32 rule reproduces it exactly."""
    k = np.arange(255, dtype=np.float64)
    col = ((k + 0.5) / 127.5 - 1.0).astype(F)                       # colour candidates
    exact_c = ((col + F(1)) * F(127.5)).astype(np.float64) == k + 0.5
    alp = ((k + 0.5) / 255.0).astype(F)
    exact_a = (alp * F(255)).astype(np.float64) == k + 0.5
    assert exact_c.sum() >= 16 and exact_a.sum() >= 16               # (enough exact half-codes of both parities)
    even = (2 * np.round((k + 0.5) / 2)).astype(np.uint8)            # the even neighbour of k + 0.5
    x = np.zeros((255, 4), F)
    x[:, 0] = x[:, 1] = x[:, 2] = col
    x[:, 3] = alp
    q = P.encode_np(x, 'rgba8')
    for c in range(3):
        assert np.array_equal(q[exact_c, c], even[exact_c])
    assert np.array_equal(q[exact_a, 3], even[exact_a])
    assert set(even[exact_c] % 2) == {0} and len(set((k[exact_c] % 2).tolist())) == 2   # ties above odd AND even codes


def test_rgba8_out_of_range_inputs_clamp():
    x = np.array([[-1.5, 1.5, -1.0000001, -0.25], [np.inf, -np.inf, 1.0000001, 1.5], [-3e38, 3e38, -1, 7]], F)
    q = P.encode_np(x, 'rgba8')
    assert q.tolist() == [[0, 255, 0, 0], [255, 0, 255, 255], [0, 255, 0, 255]]


def test_rgba8_nan_encodes_as_code_zero():
    q = P.encode_np(np.full((1, 4), np.nan, F), 'rgba8')
    assert q.tolist() == [[0, 0, 0, 0]]


@pytest.mark.parametrize("shape", [(2, 30, 70, 5), (1, 64, 128, 8)])
def test_rgba8_round_trip_error(shape):
    """<= half a step + 1e-6: 1/255 for colour, 1/510 for alpha (the 1e-6 covers the three fp32 roundings of the rule, each
    below 1.3e-7 at these magnitudes)."""
    x = random_rgba(3, *shape)
    y = P.decode_np(P.encode_np(x, 'rgba8'), 'rgba8')
    err = np.abs(y.astype(np.float64) - x.astype(np.float64))
    ec, ea = err[..., :3].max(), err[..., 3].max()
    print("rgba8 round trip: colour %.9g (1/255 = %.9g), alpha %.9g (1/510 = %.9g)" % (ec, 1 / 255, ea, 1 / 510))
    assert ec <= 1 / 255 + 1e-6
    assert ea <= 1 / 510 + 1e-6


def test_rgba16f_is_astype_float16():
    x = random_rgba(5, 1, 16, 32, 3)
    x[0, 0, 0, 0] = [70000.0, -70000.0, 1e-8, -0.0]                 # overflow to inf, underflow, signed zero: no clamp
    q = P.encode_np(x, 'rgba16f')
    assert q.dtype == np.float16
    with np.errstate(over='ignore'):
        assert np.array_equal(q.view(np.uint16), x.astype(np.float16).view(np.uint16))
    assert np.array_equal(P.decode_np(q, 'rgba16f').view(np.uint32), q.astype(F).view(np.uint32))


def _stack(format, planes):
    x = random_rgba(9, 2, 6, 10, 3)                                  # [B,H,W,D,4]
    codes = P.encode_np(np.ascontiguousarray(np.transpose(x, (0, 3, 1, 2, 4))), format)     # native [B,D,H,W,4]
    return P.PackedLayers(codes, format, planes), codes


@pytest.mark.parametrize("format", P.FORMATS)
@pytest.mark.parametrize("planes", [None, (100.0, 2.5, 1.0)])
def test_save_load_round_trip(tmp_path, format, planes):
    pk, codes = _stack(format, planes)
    assert pk.shape == (2, 6, 10, 3) and pk.format == format
    assert pk.nbytes == 2 * 3 * 6 * 10 * P.BYTES_PER_TEXEL[format] == pk.data.numel() * pk.data.element_size()
    path = str(tmp_path / "stack.npz")
    pk.save(path)
    back = P.PackedLayers.load(path)
    assert back.format == format and back.shape == pk.shape and back.planes == planes and back.nbytes == pk.nbytes
    assert back.data.dtype == pk.data.dtype
    bits = np.uint8 if format == 'rgba8' else np.uint16
    assert np.array_equal(back.data.numpy().view(bits), codes.view(bits))
    with np.load(path, allow_pickle=False) as z:                     # readable without pickle
        assert sorted(z.files) == ["codes", "format", "has_planes", "layout_version", "planes"]


def test_packed_layers_checks_its_arguments():
    pk, codes = _stack('rgba8', None)
    with pytest.raises(ValueError):
        P.PackedLayers(codes, 'rgba16f')                             # uint8 codes are not halves
    with pytest.raises(ValueError):
        P.PackedLayers(codes[0], 'rgba8')                            # not [B,D,H,W,4]
    with pytest.raises(ValueError):
        P.PackedLayers(codes, 'rgba8', planes=(1.0, 2.0))            # three layers, two planes
    with pytest.raises(ValueError):
        P.PackedLayers(codes, 'bc7')


def _rewrite(path, **changes):
    with np.load(path, allow_pickle=False) as z:
        fields = {k: z[k] for k in z.files}
    fields.update(changes)
    with open(path, "wb") as f:
        np.savez(f, **fields)


def test_load_refuses_unknown_layout_version_and_format(tmp_path):
    pk, _ = _stack('rgba8', (100.0, 2.5, 1.0))
    path = str(tmp_path / "stack.npz")
    pk.save(path)
    _rewrite(path, layout_version=np.int64(P.LAYOUT_VERSION + 1))
    with pytest.raises(ValueError, match="layout version"):
        P.PackedLayers.load(path)
    pk.save(path)
    _rewrite(path, format=np.array("rgb565"))
    with pytest.raises(ValueError, match="format"):
        P.PackedLayers.load(path)
    pk.save(path)
    assert P.PackedLayers.load(path).planes == (100.0, 2.5, 1.0)     # (control: the untouched file loads)


def test_package_exports_packed_layers():
    import matryodshka_amd
    assert matryodshka_amd.PackedLayers is P.PackedLayers
