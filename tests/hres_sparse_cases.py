"""Inputs shared by the tests of the sparse high-res stack (MSI.hres_layers_sparse, msi_hres_index_tiles, msi_hres_layers_sparse):
low-res alphas with whole layers, single texels and rectangles switched off, so that the tile table has kept and dropped tiles in
every layout a kernel can get wrong, and the keep rule restated in numpy from the low-res alphas alone -- the fp32 align-corners
resize in the kernels' operation order, the encoders of packed.py's formats, sparse.keep_np -- for the tests without a GPU."""
import numpy as np

from matryodshka_amd import sparse

FORMATS = ("rgba8", "rgba16f")
B = 2
# (low h, w -> high Hh, Wh, D): the smallest shapes that reach each path
SHAPES = [
    (16, 32, 40, 96, 8),       # non-integer scale
    (8, 16, 12, 48, 4),        # 3 x 3 tiles: every wrap neighbour is a different tile
    (4, 20, 8, 272, 4),        # a second 256-column block with 16 live columns
    (16, 32, 16, 32, 8),       # scale 1
    (8, 24, 64, 1040, 8),      # 1040 tiles per layer: more than one chunk of sparse_scan_kernel
]
SHAPE_IDS = ["x".join(str(v) for v in s) for s in SHAPES]
SEED = 1300


def masks(h, w, d, b=B):
    """mask [B,h,w,D] of the low-res alphas: layer 0 all zero (kept whatever its alpha), layer 1 empty, layers 2 and 3 one corner
    texel each (after the resize: the corner, so the kept tiles come through both wraps), the last layer (D > 4) empty in sample 0
    and full in sample 1, every other layer a rectangle that moves with the layer."""
    m = np.zeros((b, h, w, d), np.float32)
    m[:, 0, 0, 2] = 1.0
    m[:, h - 1, w - 1, 3] = 1.0
    rh, rw = h // 2, 2 * w // 3
    for l in range(4, d):
        if l == d - 1:
            m[1:, :, :, l] = 1.0
            continue
        y0, x0 = (3 * l) % (h - rh + 1), (7 * l) % (w - rw + 1)
        m[:, y0:y0 + rh, x0:x0 + rw, l] = 1.0
    return m


def low_res(shape, seed=SEED, b=B):
    """(blend weights uniform in (0,1), alphas = (0.05 + 0.9 u) * mask), both fp32 [B,h,w,D]."""
    h, w, _, _, d = shape
    rng = np.random.RandomState(seed)
    bw = rng.uniform(0.0, 1.0, size=(b, h, w, d)).astype(np.float32)
    al = ((np.float32(0.05) + np.float32(0.9) * rng.uniform(0.0, 1.0, size=(b, h, w, d)).astype(np.float32)) * masks(h, w, d, b)).astype(np.float32)
    return bw, al


def case(shape, seed=SEED, b=B, tile_from=None):
    """The arguments of MSI.hres_layers for `shape`: images from tests.util-style make_inputs at the high-res size (or a tile of
    that, repeated), identity-free random poses as make_inputs gives them."""
    from tests.test_gpu_hres_layers import _case
    h, w, hh, hw, d = shape
    x = _case(seed + 1, b, h, w, hh, hw, d, tile_from=tile_from)
    x["bw"], x["al"] = low_res(shape, seed, b)
    return x


# ---- the rule in numpy, from the low-res alphas ----------------------------------------------------------------------------------
def _axis(n_low, n_high):
    """lower / upper corner and fraction of the align-corners resize along one axis, in fp32 as the kernels compute them."""
    s = np.float32(n_low - 1) / np.float32(n_high - 1) if n_high > 1 else np.float32(0)
    f = np.arange(n_high, dtype=np.float32) * s
    lo = np.floor(f).astype(np.int64)
    hi = np.minimum(np.ceil(f).astype(np.int64), n_low - 1)
    return lo, hi, (f - lo.astype(np.float32)).astype(np.float32)


def resize_np(al, hh, hw):
    """[B,h,w,D] -> [B,Hh,Wh,D]: top = tl + (tr - tl) xl, bottom likewise, out = top + (bottom - top) yl, every op in fp32."""
    al = np.asarray(al, np.float32)
    y0, y1, yl = _axis(al.shape[1], hh)
    x0, x1, xl = _axis(al.shape[2], hw)
    xl, yl = xl[None, None, :, None], yl[None, :, None, None]
    with np.errstate(invalid="ignore"):
        tl, tr = al[:, y0][:, :, x0], al[:, y0][:, :, x1]
        bl, br = al[:, y1][:, :, x0], al[:, y1][:, :, x1]
        top = tl + (tr - tl) * xl
        bot = bl + (br - bl) * xl
        return (top + (bot - top) * yl).astype(np.float32)


def alpha_codes_np(alpha, fmt):
    """The code an alpha is stored as: rgba8 rint(min(max(a, 0), 1) * 255) with C's fmaxf / fminf (a NaN gives 0), rgba16f the
    IEEE conversion to half."""
    with np.errstate(invalid="ignore", over="ignore"):
        if fmt == "rgba8":
            return np.rint(np.fmin(np.fmax(alpha, np.float32(0)), np.float32(1)) * np.float32(255)).astype(np.uint8)
        return alpha.astype(np.float16)


def restated_codes(al, hh, hw, fmt):
    """Codes [B,D,Hh,Wh,4] with the alpha the dense stack would hold and zero colours: all the keep rule looks at."""
    a = alpha_codes_np(resize_np(al, hh, hw), fmt).transpose(0, 3, 1, 2)
    q = np.zeros(a.shape + (4,), a.dtype)
    q[..., 3] = a
    return q


def restated_keep(al, hh, hw, fmt):
    return sparse.keep_np(restated_codes(al, hh, hw, fmt), fmt)


def check_masks(keep):
    """The condition every test file asserts first: the table is neither empty nor full, layer 0 whole, layer 1 empty."""
    occ = float(keep.mean())
    assert 0.2 <= occ <= 0.8, occ
    assert keep[:, 0].all() and not keep[:, 1].any()
    return occ
