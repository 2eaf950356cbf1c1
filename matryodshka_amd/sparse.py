"""Sparse layer stacks: a `PackedLayers` (`rgba8` / `rgba16f`, packed.py) that stores only the tiles a sphere render can see.

An MSI is not a dense object: a ray meets colour on a few of its spheres and nothing on the rest, and a texel whose alpha
decodes to zero contributes exactly nothing to the over-composite (layer 0 excepted: the composite takes its colour whatever
its alpha).  A `SparseLayers` keeps the occupied tiles of the native [B,D,H,W,4] codes in one pool and a table that says where
each tile went; `MSI.sparsify_layers` makes one on the device, `MSI.render_views` / `render_ods_pair` render from it directly
with the pixels of the dense render, `MSI.densify_layers` expands it, and `save` / `load` keep it in one `.npz`.
`sparsify_np` / `expand_np` are the rule in numpy: a host without a GPU reads a saved stack with them, and the GPU tests compare
the kernels against them bit for bit.

This module does not load the native library.

The rule (include/msi_hip.h states it for the C ABI):
  tile         TILE_H x TILE_W = 4 rows x 16 columns of texels (a tile row is one 64-byte run of rgba8, 128 bytes of rgba16f);
               H % 4 == 0 and W % 16 == 0 are required.
  empty texel  its alpha DECODES to zero: code 0 (rgba8), +0 or -0 (rgba16f).
  keep         tile (ty, tx) of layer d of sample b is kept iff d == 0 or any texel within Chebyshev distance 1 of the tile --
               its 6 x 18 window, x taken modulo W and y modulo H, as the bilinear taps of the sphere renders wrap -- is not
               empty.  Then a bilinear footprint (2 x 2 texels on the torus) with ANY tap in a dropped tile has all four alphas
               zero: one predicate per layer, "all four tap tiles present", decides whether the layer can contribute.
  table        int32 [B,D,H/4,W/16]: the tile's index among the kept tiles of its own layer (b, d), row-major, or -1.
  layer_start  int64 [B*D+1]: exclusive prefix sum of the kept tiles per layer; layer_start[-1] = T.
  pool         [T,4,16,4] codes (uint8 / float16); tile k of layer (b, d) is pool[layer_start[b*D+d] + k].
  border       which surface the stack was made for.  'wrap' is the rule above, for the sphere renders.  'edge' is for samplers that never
               read the opposite border -- the planar viewer zero-pads, the cube viewer clamps to the edge of the face --: the same rule
               with the 6 x 18 window CLIPPED to the image instead of wrapped.  An edge stack keeps a subset of the wrap stack's tiles;
               a sphere render of it would be wrong, so the viewers accept only the rule they were made for.
"""
import numpy as np
import torch

from .packed import FORMATS, PackedLayers, _NP_DTYPE, _TORCH_DTYPE, _check_format

TILE_H, TILE_W = 4, 16
LAYOUT_VERSION = 1            # of the .npz written by SparseLayers.save for a 'wrap' stack
EDGE_LAYOUT_VERSION = 2       # ... for an 'edge' stack: version 1 plus a `border` key (a reader written for 1 refuses it)
BORDERS = ('wrap', 'edge')


def _check_border(border):
    if border not in BORDERS:
        raise ValueError("border must be one of %s, not %r" % (BORDERS, border))


def _check_tiles(h, w):
    if h % TILE_H or w % TILE_W:
        raise ValueError("a sparse stack needs H %% %d == 0 and W %% %d == 0, not %d x %d" % (TILE_H, TILE_W, h, w))


def _codes(codes, format):
    _check_format(format)
    q = np.asarray(codes)
    if q.dtype != _NP_DTYPE[format] or q.ndim != 5 or q.shape[-1] != 4:
        raise ValueError("%s codes must be %s in the native layout [B,D,H,W,4]" % (format, np.dtype(_NP_DTYPE[format]).name))
    _check_tiles(q.shape[2], q.shape[3])
    return q


def _tiles(q):
    """[B,D,H,W,4] -> [B,D,H/4,W/16,4,16,4] (a view)."""
    b, d, h, w, _ = q.shape
    return q.reshape(b, d, h // TILE_H, TILE_H, w // TILE_W, TILE_W, 4).transpose(0, 1, 2, 4, 3, 5, 6)


def _shift_clipped(a, dy, dx):
    """`a` [B,D,H,W] moved by (dy, dx) along (H, W), False moved in: np.roll without the wrap."""
    out = np.zeros_like(a)
    h, w = a.shape[2], a.shape[3]
    ys, yd = (slice(0, h - dy), slice(dy, h)) if dy >= 0 else (slice(-dy, h), slice(0, h + dy))
    xs, xd = (slice(0, w - dx), slice(dx, w)) if dx >= 0 else (slice(-dx, w), slice(0, w + dx))
    out[:, :, yd, xd] = a[:, :, ys, xs]
    return out


def keep_np(codes, format, border='wrap'):
    """bool [B,D,H/4,W/16]: the keep rule."""
    _check_border(border)
    q = _codes(codes, format)
    b, d, h, w, _ = q.shape
    occupied = q[..., 3] != 0                                       # (-0.0 != 0 is False: both zeros of a half are empty)
    near = np.zeros_like(occupied)
    for dy in (-1, 0, 1):
        for dx in (-1, 0, 1):
            if border == 'wrap':
                near |= np.roll(occupied, (dy, dx), axis=(2, 3))    # the torus: both axes wrap
            else:
                near |= _shift_clipped(occupied, dy, dx)            # the window is clipped to the image
    keep = near.reshape(b, d, h // TILE_H, TILE_H, w // TILE_W, TILE_W).any(axis=(3, 5))
    keep[:, 0] = True
    return keep


def sparsify_np(codes, format, border='wrap'):
    """codes [B,D,H,W,4] (uint8 / float16) -> (table int32 [B,D,H/4,W/16], layer_start int64 [B*D+1], pool [T,4,16,4])."""
    q = _codes(codes, format)
    keep = keep_np(q, format, border)
    b, d, ty, tx = keep.shape
    flat = keep.reshape(b * d, ty * tx)
    table = np.where(flat, np.cumsum(flat, axis=1) - 1, -1).astype(np.int32).reshape(b, d, ty, tx)
    layer_start = np.zeros(b * d + 1, np.int64)
    layer_start[1:] = np.cumsum(flat.sum(axis=1, dtype=np.int64))
    pool = np.ascontiguousarray(_tiles(q)[keep])                    # (boolean indexing runs b, d, ty, tx in row-major order)
    return table, layer_start, pool.reshape(-1, TILE_H, TILE_W, 4)


def expand_np(table, layer_start, pool, format):
    """The dense codes [B,D,H,W,4] a sparse stack stands for: all-zero bytes in dropped tiles."""
    _check_format(format)
    table, layer_start, pool = np.asarray(table), np.asarray(layer_start), np.asarray(pool)
    b, d, ty, tx = table.shape
    where = table.reshape(b * d, ty * tx).astype(np.int64) + layer_start[:-1, None]
    kept = table.reshape(b * d, ty * tx) >= 0
    tiles = np.zeros((b * d, ty * tx, TILE_H, TILE_W, 4), _NP_DTYPE[format])
    tiles[kept] = pool[where[kept]]
    tiles = tiles.reshape(b, d, ty, tx, TILE_H, TILE_W, 4).transpose(0, 1, 2, 4, 3, 5, 6)      # [B,D,ty,4,tx,16,4]
    return np.ascontiguousarray(tiles).reshape(b, d, ty * TILE_H, tx * TILE_W, 4)


def consistent_np(table, layer_start, tiles):
    """True when every index of `table` stays inside its own layer's run of the pool: layer_start [B*D+1] starts at 0, never decreases and ends
    at `tiles`, and -1 <= table[b,d] < that layer's count.  The copy kernels address pool[layer_start[l] + index] as they are told
    (msi_sparse_expand has no bound of its own), so SparseLayers refuses host-side arrays that fail this -- a damaged or edited file."""
    table, layer_start = np.asarray(table), np.asarray(layer_start)
    if table.ndim != 4 or layer_start.shape != (table.shape[0] * table.shape[1] + 1,):
        return False
    counts = np.diff(layer_start)
    per_layer = table.reshape(counts.shape[0], -1)
    return bool(int(layer_start[0]) == 0 and int(layer_start[-1]) == int(tiles) and np.all(counts >= 0) and np.all(per_layer >= -1)
                and np.all(per_layer.max(axis=1, initial=-1) < counts))


class SparseLayers(object):
    """An MSI layer stack that stores only its occupied tiles.

    format       'rgba8' | 'rgba16f'
    shape        (B, H, W, D): the [B,H,W,D,4] stack it stands for
    planes       the sphere radii the stack was made for (tuple of floats, far -> near), or None
    border       'wrap' (a sphere stack: render_views, render_ods_pair) | 'edge' (a planar or cube-face stack: mpi_render_views,
                 cube_render_views)
    tile         (4, 16)
    table        torch int32 [B,D,H/4,W/16]
    layer_start  torch int64 [B*D+1]
    pool         torch [T,4,16,4], uint8 / float16
    nbytes       bytes of the three arrays
    occupancy    T / number of tiles"""

    def __init__(self, table, layer_start, pool, format, planes=None, tile=(TILE_H, TILE_W), border='wrap'):
        _check_format(format)
        _check_border(border)
        if tuple(int(t) for t in tile) != (TILE_H, TILE_W):
            raise ValueError("tile must be %r, not %r" % ((TILE_H, TILE_W), tuple(tile)))
        as_tensor = lambda x: x if torch.is_tensor(x) else torch.from_numpy(np.ascontiguousarray(x))
        table, layer_start, pool = as_tensor(table), as_tensor(layer_start), as_tensor(pool)
        if table.dtype != torch.int32 or table.dim() != 4:
            raise ValueError("table must be int32 [B,D,H/%d,W/%d]" % (TILE_H, TILE_W))
        b, d = table.shape[:2]
        if layer_start.dtype != torch.int64 or tuple(layer_start.shape) != (b * d + 1,):
            raise ValueError("layer_start must be int64 [B*D+1] = %s" % ((b * d + 1,),))
        if pool.dtype != _TORCH_DTYPE[format]:
            raise ValueError("%s pool must be %s, not %s" % (format, _TORCH_DTYPE[format], pool.dtype))
        if pool.dim() != 4 or tuple(pool.shape[1:]) != (TILE_H, TILE_W, 4):
            raise ValueError("pool must be [T,%d,%d,4]" % (TILE_H, TILE_W))
        if not (table.device == layer_start.device == pool.device):
            raise ValueError("table, layer_start and pool must live on one device")
        # (host-side arrays are checked here, at no synchronisation; device-side ones come from sparsify_layers or from .to() of a checked object)
        if not table.is_cuda and not consistent_np(table.numpy(), layer_start.numpy(), pool.shape[0]):
            raise ValueError("table, layer_start and pool do not belong together")
        self.table, self.layer_start, self.pool = table.contiguous(), layer_start.contiguous(), pool.contiguous()
        self.format = format
        self.border = border
        self.tile = (TILE_H, TILE_W)
        if planes is not None:
            if torch.is_tensor(planes):
                planes = planes.detach().cpu().reshape(-1).tolist()
            planes = tuple(float(p) for p in planes)
            if len(planes) != d:
                raise ValueError("len(planes) != number of layers")
        self.planes = planes

    @classmethod
    def from_codes(cls, codes, format, planes=None, border='wrap'):
        """The numpy rule on host-side codes [B,D,H,W,4] (or a host-side PackedLayers)."""
        if isinstance(codes, PackedLayers):
            codes, format, planes = codes.data.cpu().numpy(), codes.format, codes.planes if planes is None else planes
        table, layer_start, pool = sparsify_np(codes, format, border)
        return cls(table, layer_start, pool, format, planes, border=border)

    @property
    def shape(self):
        b, d, ty, tx = self.table.shape
        return (b, ty * TILE_H, tx * TILE_W, d)

    @property
    def nbytes(self):
        return sum(t.numel() * t.element_size() for t in (self.table, self.layer_start, self.pool))

    @property
    def occupancy(self):
        return self.pool.shape[0] / float(max(self.table.numel(), 1))

    def to(self, device):
        return SparseLayers(self.table.to(device), self.layer_start.to(device), self.pool.to(device), self.format, self.planes,
                            border=self.border)

    def expand_np(self):
        """The dense codes [B,D,H,W,4] (numpy), dropped tiles zeroed."""
        return expand_np(self.table.cpu().numpy(), self.layer_start.cpu().numpy(), self.pool.cpu().numpy(), self.format)

    def save(self, path):
        """One .npz (no pickle): table, layer_start, pool, format, tile, planes, layout_version -- version 1 for a 'wrap' stack; an 'edge'
        stack is version 2 with a `border` key, so that a reader written for version 1 refuses it instead of rendering it on a sphere."""
        planes = np.zeros(0, np.float64) if self.planes is None else np.asarray(self.planes, np.float64)
        edge = dict(border=np.array(self.border)) if self.border == 'edge' else {}
        with open(path, "wb") as f:
            np.savez(f, sparse_layout_version=np.int64(EDGE_LAYOUT_VERSION if edge else LAYOUT_VERSION), format=np.array(self.format),
                     tile_h=np.int64(TILE_H), tile_w=np.int64(TILE_W), table=self.table.cpu().numpy(),
                     layer_start=self.layer_start.cpu().numpy(), pool=self.pool.cpu().numpy(),
                     has_planes=np.bool_(self.planes is not None), planes=planes, **edge)

    @classmethod
    def load(cls, path, device=None):
        with np.load(path, allow_pickle=False) as z:
            if "sparse_layout_version" not in z.files:
                raise ValueError("%s: not a SparseLayers file (no sparse_layout_version)" % path)
            version = int(z["sparse_layout_version"])
            if version not in (LAYOUT_VERSION, EDGE_LAYOUT_VERSION):
                raise ValueError("%s: sparse layout version %d, this reader is written for %d and %d"
                                 % (path, version, LAYOUT_VERSION, EDGE_LAYOUT_VERSION))
            border = 'wrap'
            if version == EDGE_LAYOUT_VERSION:
                if "border" not in z.files or str(z["border"]) != 'edge':
                    raise ValueError("%s: a version %d file must say border = 'edge'" % (path, EDGE_LAYOUT_VERSION))
                border = 'edge'
            format = str(z["format"])
            if format not in FORMATS:
                raise ValueError("%s: unknown format %r (known: %s)" % (path, format, FORMATS))
            tile = (int(z["tile_h"]), int(z["tile_w"]))
            if tile != (TILE_H, TILE_W):
                raise ValueError("%s: tile %r, this reader is written for %r" % (path, tile, (TILE_H, TILE_W)))
            table, layer_start, pool = z["table"], z["layer_start"], z["pool"]
            planes = tuple(z["planes"].tolist()) if bool(z["has_planes"]) else None
        if pool.dtype != _NP_DTYPE[format]:
            raise ValueError("%s: %s pool stored as %s" % (path, format, pool.dtype))
        if table.dtype != np.int32 or layer_start.dtype != np.int64:
            raise ValueError("%s: table / layer_start stored as %s / %s" % (path, table.dtype, layer_start.dtype))
        if not consistent_np(table, layer_start, pool.shape[0]):
            raise ValueError("%s: table, layer_start and pool do not belong together" % path)
        out = cls(table, layer_start, pool, format, planes, border=border)
        return out if device is None else out.to(device)
