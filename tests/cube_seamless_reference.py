"""fp64 numpy reference of the seamless filter of the cube-map viewer (MSI.cube_render_views(filtering='seamless')), written
from the rule and the cube's geometry; it calls nothing of the package.  Rays, shell hit and face choice are
tests/cube_reference.py's.

The rule (cube camera fx = fy = cx = cy = S/2 only): u, v clamped to [0, S]; x0 = min(floor(u), S-1), x1 = x0 + 1, du = u - x0,
likewise y; four bilinear taps; a tap with x < S and y < S is the face's own texel; a tap with x = S or y = S is a virtual
texel at its cube point P: the other faces that contain P in ascending index, the first whose lattice coordinates of P lie in
[0, S-1]^2 supplies its texel; when none does, the mean of the clamped texels of all faces meeting at P.

The virtual-texel table is built from GEOMETRY: the cube point of every out-of-range lattice point is projected into every
other face (no closed form; tests compare the package's closed form, cubemap.virtual_texel, with this table)."""
import functools

import numpy as np

from tests import cube_reference as ref

R = ref.R


def cube_point(f, x, y, s):
    """Cube-frame point (half-side 1) of lattice point (x, y) of face f with the cube camera: R_f (2x/S - 1, 2y/S - 1, 1)."""
    return R[f] @ np.array([2.0 * x / s - 1.0, 2.0 * y / s - 1.0, 1.0])


def faces_containing(p, s):
    """[(g, x', y')] for every face g whose plane holds the cube point p, with p's lattice coordinates in g (integers)."""
    out = []
    for g in range(6):
        q = R[g].T @ p
        if q[2] == 1.0:
            xy = (q[:2] + 1.0) * s / 2.0
            ixy = np.rint(xy)
            assert np.abs(xy - ixy).max() < 1e-9, (g, xy)
            out.append((g, int(ixy[0]), int(ixy[1])))
    return out


@functools.lru_cache(maxsize=None)
def virtual_table(s):
    """{(f, x, y): [(face, x', y', weight), ...]} for every lattice point with x == S or y == S (0 <= x, y <= S) of every face."""
    table = {}
    for f in range(6):
        for y in range(s + 1):
            for x in range(s + 1):
                if x < s and y < s:
                    continue
                p = cube_point(f, x, y, s)
                others = [(g, gx, gy) for g, gx, gy in faces_containing(p, s) if g != f]       # ascending g
                assert len(others) in (1, 2), (f, x, y, others)
                stored = [(g, gx, gy) for g, gx, gy in others if 0 <= gx < s and 0 <= gy < s]
                if stored:
                    g, gx, gy = stored[0]
                    table[(f, x, y)] = [(g, gx, gy, 1.0)]
                else:
                    meet = [(f, x, y)] + others
                    w = 1.0 / len(meet)
                    table[(f, x, y)] = [(g, min(max(gx, 0), s - 1), min(max(gy, 0), s - 1), w) for g, gx, gy in meet]
    return table


def edge_classes(s):
    """The 12 cube edges by how many faces store their interior points: {frozenset({f, g}): number of storing faces}."""
    classes = {}
    for f in range(6):
        for side in range(4):               # x = 0, x = S, y = 0, y = S at an interior running coordinate
            for t in range(1, s):
                x, y = [(0, t), (s, t), (t, 0), (t, s)][side]
                here = faces_containing(cube_point(f, x, y, s), s)
                assert len(here) == 2
                key = frozenset(g for g, _, _ in here)
                n = sum(1 for _, gx, gy in here if 0 <= gx < s and 0 <= gy < s)
                assert classes.setdefault(key, n) == n
    return classes


@functools.lru_cache(maxsize=None)
def _table_arrays(s):
    """The table as arrays over (f, y, x) in [0, S]^2, own texels included: faces / xs / ys [6,S+1,S+1,3] and weights (0-padded)."""
    g = np.zeros((6, s + 1, s + 1, 3), np.int64)
    gx, gy, w = g.copy(), g.copy(), np.zeros(g.shape)
    tab = virtual_table(s)
    for f in range(6):
        for y in range(s + 1):
            for x in range(s + 1):
                ent = tab.get((f, x, y), [(f, x, y, 1.0)])
                for k, (a, b, c, d) in enumerate(ent):
                    g[f, y, x, k], gx[f, y, x, k], gy[f, y, x, k], w[f, y, x, k] = a, b, c, d
    return g, gx, gy, w


def render_view(stack, planes, k, pose, tgt_pos, camera, size, intrinsics=None, seamless=True):
    """One view of one cube.  stack [6,S,S,D,4], k = stack camera [3,3] (the rule needs fx = fy = cx = cy = S/2).
    Returns dict(rgb [h,w,3], depth [h,w], margin [h,w], strip [h,w], corner [h,w]): margin as cube_reference.render_view;
    strip = the largest of u - (S-1) and v - (S-1) over the shells (> 0: some tap of the pixel is a virtual texel); corner = some
    shell of the pixel took a three-face mean with a non-zero weight.  seamless=False switches the rule off: the clamp filter."""
    stack = np.asarray(stack)
    s, d = stack.shape[1], stack.shape[3]
    k = np.asarray(k, np.float64)
    if seamless:
        assert k[0, 0] == k[1, 1] == k[0, 2] == k[1, 2] == s / 2.0, "the seamless rule is defined for the cube camera only"
    o, r = ref.target_rays(camera, size, pose, tgt_pos, intrinsics)
    hi = s if seamless else s - 1
    tg, tx, ty, tw = _table_arrays(s)
    rgb = dep = None
    margin = np.full(r.shape[:2], np.inf)
    strip = np.full(r.shape[:2], -np.inf)
    corner = np.zeros(r.shape[:2], dtype=bool)
    for l in range(d):
        h = float(planes[l])
        p = ref._hit(o, r, h)
        margin = np.minimum(margin, 1.0 - np.sort(np.abs(p), axis=-1)[..., 1] / h)
        f, q = ref._face_of(p)
        u = k[0, 0] * q[..., 0] / h + k[0, 2]
        v = k[1, 1] * q[..., 1] / h + k[1, 2]
        strip = np.maximum(strip, np.maximum(u - (s - 1), v - (s - 1)))
        u, v = np.clip(u, 0, hi), np.clip(v, 0, hi)
        x0, y0 = np.minimum(np.floor(u), s - 1).astype(np.int64), np.minimum(np.floor(v), s - 1).astype(np.int64)
        x1, y1 = np.minimum(x0 + 1, hi), np.minimum(y0 + 1, hi)
        du, dv = (u - x0)[..., None], (v - y0)[..., None]
        tex = stack[:, :, :, l, :]

        def tap(yy, xx, weight):
            nonlocal corner
            val = tex[tg[f, yy, xx, 0], ty[f, yy, xx, 0], tx[f, yy, xx, 0]].astype(np.float64) * tw[f, yy, xx, 0][..., None]
            for e in (1, 2):                               # the means: a few pixels
                m = tw[f, yy, xx, e] > 0
                if m.any():
                    fm, ym, xm = f[m], yy[m], xx[m]
                    val[m] += tex[tg[fm, ym, xm, e], ty[fm, ym, xm, e], tx[fm, ym, xm, e]].astype(np.float64) * tw[fm, ym, xm, e][..., None]
            corner |= (tw[f, yy, xx, 2] > 0) & (weight[..., 0] > 0)
            return val * weight

        val = (tap(y0, x0, (1 - dv) * (1 - du)) + tap(y0, x1, (1 - dv) * du) + tap(y1, x0, dv * (1 - du)) + tap(y1, x1, dv * du))
        a = val[..., 3:]
        if l == 0:
            rgb, dep = val[..., :3], np.zeros(val.shape[:2])
        else:
            rgb = val[..., :3] * a + rgb * (1 - a)
            dep = (l / d) * a[..., 0] + dep * (1 - a[..., 0])
    return dict(rgb=rgb, depth=dep, margin=margin, strip=strip, corner=corner)


KEYS = ("rgb", "depth", "margin", "strip", "corner")


def render_views(stack, planes, k, pose, tgt_pos, camera, size, intrinsics=None, seamless=True):
    """stack [6B,S,S,D,4], pose [B,V,4,4], tgt_pos [B,V,3] -> dict of rgb [B,V,h,w,3], depth / margin / strip / corner [B,V,h,w]."""
    b_, v_ = np.asarray(pose).shape[:2]
    outs = [[render_view(stack[6 * b:6 * b + 6], planes, k, pose[b][v], tgt_pos[b][v], camera, size, intrinsics, seamless)
             for v in range(v_)] for b in range(b_)]
    return {key: np.stack([np.stack([o[key] for o in row]) for row in outs]) for key in KEYS}


# ---- the shared inputs of the continuity and round-trip checks
def constant_faces(s, colours):
    """[6,S,S,1,4]: face f filled with colours[f] (rgb), alpha 1."""
    x = np.ones((6, s, s, 1, 4))
    for f in range(6):
        x[f, ..., :3] = np.asarray(colours[f], np.float64)
    return x


CONSTANT_COLOURS = [(1, -1, -1), (-1, 1, -1), (0.5, 0.5, 1), (0.5, 0.5, 1), (0.5, 0.5, 1), (-1, -1, 1)]   # faces 2, 3 and 4 equal


def largest_neighbour_step(img):
    """Largest absolute difference between horizontally (wrapping) or vertically adjacent pixels, over the channels."""
    img = np.asarray(img, np.float64)
    return max(np.abs(img - np.roll(img, 1, axis=1)).max(), np.abs(img[1:] - img[:-1]).max())


def analytic_panorama(d):
    """A smooth function of the direction d [...,3] (cube frame), values in [-1,1]: [...,3]."""
    d = d / np.linalg.norm(d, axis=-1, keepdims=True)
    x, y, z = d[..., 0], d[..., 1], d[..., 2]
    return np.stack([np.sin(2.0 * x + 1.0) * np.cos(1.5 * y), np.cos(2.5 * z - 0.5) * np.sin(1.2 * x + 2.0 * y), np.sin(3.0 * y + z)], axis=-1)


def analytic_cube(s):
    """[6,S,S,1,4]: the cube cut exactly from analytic_panorama with the cube camera, one opaque layer."""
    ix, iy = np.meshgrid(np.arange(s, dtype=np.float64), np.arange(s, dtype=np.float64))
    q = np.stack([2.0 * ix / s - 1.0, 2.0 * iy / s - 1.0, np.ones_like(ix)], axis=-1)
    x = np.ones((6, s, s, 1, 4))
    for f in range(6):
        x[f, :, :, 0, :3] = analytic_panorama(q @ R[f].T)
    return x
