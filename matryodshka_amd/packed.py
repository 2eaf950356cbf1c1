"""Compact layer stacks: the `rgba8` and `rgba16f` texel formats of include/msi_hip.h (MSI_LAYERS_*).

A `PackedLayers` holds an MSI in the native [B,D,H,W,4] layout with 4 (`rgba8`) or 8 (`rgba16f`) instead of 16 bytes per
texel.  `MSI.pack_layers` makes one on the device, `MSI.render_views` renders from it directly (bit-identical to rendering
its `MSI.unpack_layers`), and `save` / `load` keep it in one `.npz`.  `encode_np` / `decode_np` are the format rule in numpy:
a host without a GPU reads a saved stack with them, and the GPU tests compare the kernels against them bit for bit.

This module does not load the native library.

rgba8 (bytes r, g, b, a; fp32 arithmetic, one rounding per operation; rint rounds half to even):
    encode colour  q = rint((min(max(x, -1), 1) + 1) * 127.5)      encode alpha  q = rint(min(max(x, 0), 1) * 255)
    decode colour  x = (float(q) - 127.5) * fl32(1 / 127.5)        decode alpha  x = float(q) * fl32(1 / 255)
  Codes 0 / 255 decode to exactly -1 / +1 (colour) and 0 / 1 (alpha), decode(255 - q) == -decode(q) for colour, both tables
  increase strictly and encode(decode(q)) == q.  A NaN input is outside the contract; it encodes as code 0 here and on the
  device (max / min return their other operand).
rgba16f: four IEEE halves, round-to-nearest-even of the fp32 value, no clamp; decode is exact.
"""
import numpy as np
import torch

FORMATS = ('rgba8', 'rgba16f')
LAYOUT_VERSION = 1            # of the .npz written by PackedLayers.save

_F = np.float32
KC = _F(float.fromhex('0x1.010102p-7'))     # fl32(1 / 127.5)
KA = _F(float.fromhex('0x1.010102p-8'))     # fl32(1 / 255)
_NP_DTYPE = {'rgba8': np.uint8, 'rgba16f': np.float16}
_TORCH_DTYPE = {'rgba8': torch.uint8, 'rgba16f': torch.float16}
BYTES_PER_TEXEL = {'rgba8': 4, 'rgba16f': 8}


def _check_format(format):
    if format not in FORMATS:
        raise ValueError("format must be one of %s, not %r" % (FORMATS, format))


def encode_np(rgba, format):
    """fp32 [...,4] -> codes [...,4]: uint8 (`rgba8`) or float16 (`rgba16f`)."""
    _check_format(format)
    x = np.asarray(rgba, dtype=_F)
    if x.shape[-1] != 4:
        raise ValueError("rgba must end in a dimension of 4")
    if format == 'rgba16f':
        with np.errstate(over='ignore'):          # no clamp: |x| > 65504 becomes inf, as on the device
            return x.astype(np.float16)
    q = np.empty(x.shape, dtype=_F)
    q[..., :3] = np.rint((np.fmin(np.fmax(x[..., :3], _F(-1)), _F(1)) + _F(1)) * _F(127.5))
    q[..., 3] = np.rint(np.fmin(np.fmax(x[..., 3], _F(0)), _F(1)) * _F(255))
    return q.astype(np.uint8)


def decode_np(codes, format):
    """codes [...,4] (uint8 / float16) -> fp32 [...,4]."""
    _check_format(format)
    q = np.asarray(codes)
    if q.dtype != _NP_DTYPE[format] or q.shape[-1] != 4:
        raise ValueError("%s codes must be %s [...,4]" % (format, np.dtype(_NP_DTYPE[format]).name))
    if format == 'rgba16f':
        return q.astype(_F)
    x = np.empty(q.shape, dtype=_F)
    x[..., :3] = (q[..., :3].astype(_F) - _F(127.5)) * KC
    x[..., 3] = q[..., 3].astype(_F) * KA
    return x


class PackedLayers(object):
    """An MSI layer stack in a compact texel format.

    data    torch tensor, native layout [B,D,H,W,4], uint8 (`rgba8`) or float16 (`rgba16f`), contiguous
    format  'rgba8' | 'rgba16f'
    shape   (B, H, W, D): the [B,H,W,D,4] stack it stands for
    nbytes  bytes of `data`
    planes  the sphere radii the stack was made for (tuple of floats, far -> near), or None"""

    def __init__(self, data, format, planes=None):
        _check_format(format)
        if not torch.is_tensor(data):
            data = torch.from_numpy(np.ascontiguousarray(data))
        if data.dtype != _TORCH_DTYPE[format]:
            raise ValueError("%s data must be %s, not %s" % (format, _TORCH_DTYPE[format], data.dtype))
        if data.dim() != 5 or data.shape[-1] != 4:
            raise ValueError("data must be the native layout [B,D,H,W,4]")
        self.data = data.contiguous()
        self.format = format
        b, d, h, w, _ = self.data.shape
        if planes is not None:
            if torch.is_tensor(planes):
                planes = planes.detach().cpu().reshape(-1).tolist()
            planes = tuple(float(p) for p in planes)
            if len(planes) != d:
                raise ValueError("len(planes) != number of layers")
        self.planes = planes

    @property
    def shape(self):
        b, d, h, w, _ = self.data.shape
        return (b, h, w, d)

    @property
    def nbytes(self):
        return self.data.numel() * self.data.element_size()

    def to(self, device):
        return PackedLayers(self.data.to(device), self.format, self.planes)

    def save(self, path):
        """One .npz (no pickle): codes, format, planes, layout_version."""
        planes = np.zeros(0, np.float64) if self.planes is None else np.asarray(self.planes, np.float64)
        with open(path, "wb") as f:
            np.savez(f, layout_version=np.int64(LAYOUT_VERSION), format=np.array(self.format), codes=self.data.cpu().numpy(),
                     has_planes=np.bool_(self.planes is not None), planes=planes)

    @classmethod
    def load(cls, path, device=None):
        with np.load(path, allow_pickle=False) as z:
            version = int(z["layout_version"])
            if version != LAYOUT_VERSION:
                raise ValueError("%s: layout version %d, this reader is written for %d" % (path, version, LAYOUT_VERSION))
            format = str(z["format"])
            if format not in FORMATS:
                raise ValueError("%s: unknown format %r (known: %s)" % (path, format, FORMATS))
            codes = z["codes"]
            planes = tuple(z["planes"].tolist()) if bool(z["has_planes"]) else None
        if codes.dtype != _NP_DTYPE[format]:
            raise ValueError("%s: %s codes stored as %s" % (path, format, codes.dtype))
        data = torch.from_numpy(codes)
        return cls(data if device is None else data.to(device), format, planes)
