"""Mip-mapped layer stacks: a stack plus its coarser levels, for alias-free minified views.

A `MipLayers` holds a native [B,D,H,W,4] stack (fp32, or a `PackedLayers` in `rgba8` / `rgba16f`) as level 0 and, in one buffer,
the levels 1 .. L-1 of its pyramid: level l is native [B,D,H>>l,W>>l,4] in the base's texel format, about a third of the base's
bytes in all.  `MSI.build_mips` makes one on the device (msi_build_mips: one launch, the base read once), `MSI.render_views` /
`render_ods_pair` render from it with trilinear filtering (msi_render_views_mip; the texel rule is in include/msi_hip.h), and
`save` / `load` keep it in one `.npz`.  `build_mips_np` is the pyramid rule in numpy: the GPU tests compare the kernel against it
bit for bit.

This module does not load the native library.

The rule (all fp32, one rounding per operation, no fused multiply-add), on DECODED texels (a, c_0..c_2) = (alpha, colour):
    level 1   texel (y, x) owns the base block (2y..2y+1, 2x..2x+1) = tl, tr, bl, br.  Its partial sums are
                  A = sum a,  P_k = sum fl(a * c_k),  Q_k = sum c_k,  each summed as (tl + tr) + (bl + br).
    level l   the partials of texel (y, x) are the sums of the four partials of level l-1 at (2y..2y+1, 2x..2x+1), in the same
              order.  Partials are never quantised: only the texel that is stored is.
    texel     with n = 4^l:  alpha = A * (1 / n);  colour_k = P_k / A (IEEE divide) where the layer d != 0 and A > 0,
              else colour_k = Q_k * (1 / n).  Layer 0 always takes the plain mean: the composite ignores its alpha.
    store     the texel is encoded with the format's encoder (packed.encode_np); fp32 stores it as it is.
A transparent texel's colour therefore never bleeds into a coarser level: the colour of a coarse texel is the alpha-weighted
mean of what it covers, which is what an over-composite of the averaged footprint wants.
"""
import numpy as np
import torch

from .packed import FORMATS as PACKED_FORMATS, PackedLayers, decode_np, encode_np, _NP_DTYPE

MAX_LEVELS = 6                # MSI_MIP_MAX_LEVELS of include/msi_hip.h
LAYOUT_VERSION = 1            # of the .npz written by MipLayers.save
FORMATS = ('f32',) + PACKED_FORMATS

_F = np.float32


def check_levels(height, width, levels):
    """The size rule of msi_build_mips: 1 <= L <= MAX_LEVELS, H and W multiples of 2^(L-1), the top level at least 2 x 2."""
    levels = int(levels)
    if not 1 <= levels <= MAX_LEVELS:
        raise ValueError("levels must be in 1..%d, not %d" % (MAX_LEVELS, levels))
    t = 1 << (levels - 1)
    if height % t or width % t:
        raise ValueError("%d levels need H and W to be multiples of %d, not %d x %d" % (levels, t, height, width))
    if levels > 1 and (height >> (levels - 1) < 2 or width >> (levels - 1) < 2):
        raise ValueError("the top level of %d levels of %d x %d is below 2 x 2" % (levels, height, width))
    return levels


def max_levels(height, width):
    """The largest L check_levels accepts for an H x W stack (at least 1)."""
    levels = 1
    while levels < MAX_LEVELS:
        try:
            check_levels(height, width, levels + 1)
        except ValueError:
            break
        levels += 1
    return levels


def level_shapes(shape, levels):
    """[(B, D, H>>l, W>>l, 4) for l in 1 .. L-1] of a native base of `shape` [B,D,H,W,4]."""
    b, d, h, w = (int(s) for s in shape[:4])
    return [(b, d, h >> l, w >> l, 4) for l in range(1, levels)]


def _sum4(p):
    """[..., 2y, 2x, C] -> [..., y, x, C]: (tl + tr) + (bl + br) in fp32."""
    tl, tr, bl, br = p[..., 0::2, 0::2, :], p[..., 0::2, 1::2, :], p[..., 1::2, 0::2, :], p[..., 1::2, 1::2, :]
    return ((tl + tr).astype(_F) + (bl + br).astype(_F)).astype(_F)


def build_mips_np(base, format, levels):
    """The pyramid rule above.  base: native [B,D,H,W,4], fp32 (`f32`) or codes (`rgba8`: uint8, `rgba16f`: float16) ->
    [level 1, .., level L-1], each native [B,D,H>>l,W>>l,4] in the base's dtype."""
    if format not in FORMATS:
        raise ValueError("format must be one of %s, not %r" % (FORMATS, format))
    base = np.asarray(base)
    if base.ndim != 5 or base.shape[-1] != 4:
        raise ValueError("base must be the native layout [B,D,H,W,4]")
    if base.dtype != (_F if format == 'f32' else _NP_DTYPE[format]):
        raise ValueError("%s base stored as %s" % (format, base.dtype))
    levels = check_levels(base.shape[2], base.shape[3], levels)
    x = base if format == 'f32' else decode_np(base, format)
    out = []
    with np.errstate(all='ignore'):
        a, c = x[..., 3:4], x[..., :3]
        # partials [..., 7] = A, P_0..2, Q_0..2
        part = np.concatenate([a, (a * c).astype(_F), c], axis=-1).astype(_F)
        for l in range(1, levels):
            part = _sum4(part)
            inv_n = _F(1.0 / 4 ** l)
            A, P, Q = part[..., 0:1], part[..., 1:4], part[..., 4:7]
            weighted = (A > 0) & (np.arange(part.shape[1]).reshape(1, -1, 1, 1, 1) != 0)
            colour = np.where(weighted, (P / A).astype(_F), (Q * inv_n).astype(_F))
            texel = np.concatenate([colour, (A * inv_n).astype(_F)], axis=-1).astype(_F)
            out.append(texel if format == 'f32' else encode_np(texel, format))
    return out


class MipLayers(object):
    """A layer stack with its mip pyramid.

    base    level 0: an fp32 tensor in the native layout [B,D,H,W,4], or a PackedLayers
    mips    levels 1 .. L-1, consecutive, in ONE 1-D tensor of the base's dtype (empty when L = 1)
    levels  L, 1 .. MAX_LEVELS
    format  'f32' | 'rgba8' | 'rgba16f'
    planes  the sphere radii the stack was made for (tuple of floats, far -> near), or None
    shape   (B, H, W, D): the [B,H,W,D,4] stack it stands for
    nbytes  bytes of the base and the levels"""

    def __init__(self, base, mips, levels, planes=None):
        if isinstance(base, PackedLayers):
            self.format, data = base.format, base.data
            planes = base.planes if planes is None else planes
        else:
            if not torch.is_tensor(base):
                base = torch.from_numpy(np.ascontiguousarray(base))
            if base.dtype != torch.float32:
                raise ValueError("an unpacked base is fp32, not %s" % (base.dtype,))
            if base.dim() != 5 or base.shape[-1] != 4:
                raise ValueError("base must be the native layout [B,D,H,W,4]")
            base = base.contiguous()
            self.format, data = 'f32', base
        b, d, h, w, _ = data.shape
        self.levels = check_levels(h, w, levels)
        if not torch.is_tensor(mips):
            mips = torch.from_numpy(np.ascontiguousarray(mips))
        mips = mips.contiguous().reshape(-1)
        want = sum(int(np.prod(s)) for s in level_shapes(data.shape, self.levels))
        if mips.dtype != data.dtype or mips.numel() != want:
            raise ValueError("mips must be %d elements of %s, got %d of %s" % (want, data.dtype, mips.numel(), mips.dtype))
        if mips.device != data.device:
            raise ValueError("base and mips must live on one device")
        if planes is not None:
            if torch.is_tensor(planes):
                planes = planes.detach().cpu().reshape(-1).tolist()
            planes = tuple(float(p) for p in planes)
            if len(planes) != d:
                raise ValueError("len(planes) != number of layers")
        self.base, self.mips, self.planes = base, mips, planes

    @property
    def data(self):
        """The base's native tensor [B,D,H,W,4]."""
        return self.base.data if isinstance(self.base, PackedLayers) else self.base

    @property
    def shape(self):
        b, d, h, w, _ = self.data.shape
        return (b, h, w, d)

    @property
    def nbytes(self):
        return self.data.numel() * self.data.element_size() + self.mips.numel() * self.mips.element_size()

    def to(self, device):
        return MipLayers(self.base.to(device), self.mips.to(device), self.levels, self.planes)

    def level(self, l):
        """Level l as a stack of its own: a native fp32 tensor [B,D,H>>l,W>>l,4] or a PackedLayers (a view of `mips`; level 0 is
        the base)."""
        l = int(l)
        if not 0 <= l < self.levels:
            raise ValueError("level must be in 0..%d, not %d" % (self.levels - 1, l))
        if l == 0:
            return self.base
        shapes = level_shapes(self.data.shape, self.levels)
        start = sum(int(np.prod(s)) for s in shapes[:l - 1])
        data = self.mips[start:start + int(np.prod(shapes[l - 1]))].view(shapes[l - 1])
        return data if self.format == 'f32' else PackedLayers(data, self.format, self.planes)

    @classmethod
    def from_numpy(cls, base, format, levels, planes=None, device=None):
        """build_mips_np of a native numpy base (fp32 or codes) as a MipLayers: the host-side builder."""
        lv = build_mips_np(base, format, levels)
        dtype = _F if format == 'f32' else _NP_DTYPE[format]
        mips = np.concatenate([x.reshape(-1) for x in lv]) if lv else np.zeros(0, dtype)
        bt, mt = torch.from_numpy(np.ascontiguousarray(base)), torch.from_numpy(mips)
        if device is not None:
            bt, mt = bt.to(device), mt.to(device)
        return cls(bt if format == 'f32' else PackedLayers(bt, format, planes), mt, levels, planes)

    def save(self, path):
        """One .npz (no pickle): base, mips, levels, format, planes, layout_version."""
        planes = np.zeros(0, np.float64) if self.planes is None else np.asarray(self.planes, np.float64)
        with open(path, "wb") as f:
            np.savez(f, layout_version=np.int64(LAYOUT_VERSION), format=np.array(self.format), levels=np.int64(self.levels),
                     base=self.data.cpu().numpy(), mips=self.mips.cpu().numpy(), has_planes=np.bool_(self.planes is not None),
                     planes=planes)

    @classmethod
    def load(cls, path, device=None):
        with np.load(path, allow_pickle=False) as z:
            version = int(z["layout_version"])
            if version != LAYOUT_VERSION:
                raise ValueError("%s: layout version %d, this reader is written for %d" % (path, version, LAYOUT_VERSION))
            format = str(z["format"])
            if format not in FORMATS:
                raise ValueError("%s: unknown format %r (known: %s)" % (path, format, FORMATS))
            levels = int(z["levels"])
            base, mips = z["base"], z["mips"]
            planes = tuple(z["planes"].tolist()) if bool(z["has_planes"]) else None
        want = np.dtype(_F) if format == 'f32' else np.dtype(_NP_DTYPE[format])
        if base.dtype != want or mips.dtype != want:
            raise ValueError("%s: %s texels stored as %s / %s" % (path, format, base.dtype, mips.dtype))
        bt, mt = torch.from_numpy(base), torch.from_numpy(mips)
        if device is not None:
            bt, mt = bt.to(device), mt.to(device)
        return cls(bt if format == 'f32' else PackedLayers(bt, format, planes), mt, levels, planes)
