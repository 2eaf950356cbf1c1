"""The fp64 statement of the trilinear view rule of msi_render_views_mip (include/msi_hip.h) for its three cameras, built like
tests/ods_views_reference.py from the oracle's primitives: the lat-long axes and the correctly rounded fp32 trig tables of the
OUTPUT size (what the kernel reads), then -- in fp64 -- the pose, the ray / sphere hit, the pixel coordinates of the stack's size,
the level of detail from the two neighbour hits, two wrap-around bilinear lookups, the lerp between them and the over-composite.
With one level (or trilinear=False) it is the plain bilinear render in fp64.  Shared by the CPU facts (test_mip_cpu.py) and the
GPU tests (test_gpu_mip_views.py)."""
import numpy as np

from oracle import geometry as G

F = np.float32
D = np.float64


def view_rays(camera, oh, ow, pos, K=None, e=None):
    """Rays of one view before the pose, fp64 [oh,ow] each: direction (rx, ry, rz), origin (cx, cy, cz).  'equirect' and 'ods'
    take the fp32 trig tables of (oh, ow); 'ods' moves the origin onto the viewing circle, e = eye * baseline (signed)."""
    pos = np.asarray(pos, F).astype(D)
    shape = (oh, ow)
    if camera == 'pinhole':
        K = np.asarray(K, F).astype(D)
        i = np.arange(oh, dtype=D)[:, None]
        j = np.arange(ow, dtype=D)[None, :]
        r = (np.ones(shape, D), np.broadcast_to(((i + 0.5) - K[1, 2]) / K[1, 1], shape), np.broadcast_to(((j + 0.5) - K[0, 2]) / K[0, 0], shape))
        c = (np.full(shape, pos[2]), np.full(shape, pos[1]), np.full(shape, pos[0]))
        return r, c
    s, t = G.lat_long_axes(oh, ow)
    cs, ss = G.cos_f32(s).astype(D)[None, :], G.sin_f32(s).astype(D)[None, :]
    ct, st = G.cos_f32(t).astype(D)[:, None], G.sin_f32(t).astype(D)[:, None]
    r = (cs * ct, np.broadcast_to(st, shape), ss * ct)
    if camera == 'ods':
        e = D(F(e))
        c = (np.broadcast_to(pos[2] + ss * e, shape), np.full(shape, pos[1]), np.broadcast_to(pos[0] + (-cs) * e, shape))
    else:
        assert camera == 'equirect', camera
        c = (np.full(shape, pos[2]), np.full(shape, pos[1]), np.full(shape, pos[0]))
    return r, c


def sphere_hits(r, c, pose, planes, width, height):
    """r <- pose[:3,:3] r, c <- pose (c, 1), then where each ray meets each sphere, as pixel coordinates of a (height, width)
    layer: (u, v), fp64 [D,oh,ow] each (spherical.get_sphere_intersections + project_spherical + theta_phi_to_pixels)."""
    P = np.asarray(pose, F).astype(D)
    rx, ry, rz = (P[k, 0] * r[0] + P[k, 1] * r[1] + P[k, 2] * r[2] for k in range(3))
    cx, cy, cz = (P[k, 0] * c[0] + P[k, 1] * c[1] + P[k, 2] * c[2] + P[k, 3] for k in range(3))
    radius = np.asarray(planes, F).astype(D).reshape(-1, 1, 1)
    a = rx * rx + ry * ry + rz * rz
    b = 2.0 * (rx * cx + ry * cy + rz * cz)
    cc = (cx * cx + cy * cy + cz * cz) - radius * radius
    t = (-b + np.sqrt(np.maximum(b * b - 4.0 * a * cc, 0.0))) / (2.0 * a)
    x, y, z = cx + t * rx, cy + t * ry, cz + t * rz
    theta, phi = -np.arctan2(z, x), np.arctan2(y, np.sqrt(x * x + z * z))
    u = ((theta + np.pi) - np.pi / width) / (2 * np.pi - 2 * np.pi / width) * (width - 1)
    v = ((phi + 0.5 * np.pi) - 0.5 * np.pi / height) / (np.pi - np.pi / height) * (height - 1)
    return u, v


def bilinear(layer, u, v):
    """sampling.resample in fp64: layer [H,W,C], (u, v) [...] -> [...,C]; weights from the unwrapped corners, indices wrapped
    in both axes, summed in the order a, b, c, d."""
    h, w, _ = layer.shape
    x0, y0 = np.floor(u), np.floor(v)
    dx0, dy0 = (u - x0)[..., None], (v - y0)[..., None]
    dx1, dy1 = 1.0 - dx0, 1.0 - dy0
    xi0, yi0 = np.mod(x0.astype(np.int64), w), np.mod(y0.astype(np.int64), h)
    xi1, yi1 = np.mod(x0.astype(np.int64) + 1, w), np.mod(y0.astype(np.int64) + 1, h)
    return ((dy1 * dx1) * layer[yi0, xi0] + (dy1 * dx0) * layer[yi0, xi1]) + (dy0 * dx1) * layer[yi1, xi0] + (dy0 * dx0) * layer[yi1, xi1]


def neighbour(n):
    """Index of the neighbour along an axis of n pixels: k + 1 where that is inside, else k - 1 (n = 1: the pixel itself, whose
    difference is 0)."""
    k = np.arange(n)
    return np.where(k + 1 < n, k + 1, np.maximum(k - 1, 0))


def lod(u, v, width, levels, lod_bias):
    """lambda of every (layer, pixel): (u, v) [D,oh,ow] of the stack's own size."""
    du_x, dv_x = u[:, :, neighbour(u.shape[2])] - u, v[:, :, neighbour(u.shape[2])] - v
    du_y, dv_y = u[:, neighbour(u.shape[1]), :] - u, v[:, neighbour(u.shape[1]), :] - v
    du_x, du_y = du_x - width * np.rint(du_x / width), du_y - width * np.rint(du_y / width)
    rho = np.maximum(np.hypot(du_x, dv_x), np.hypot(du_y, dv_y))
    with np.errstate(divide='ignore'):
        lam = np.log2(rho) + lod_bias
    return np.where(rho > 0, np.minimum(np.maximum(lam, 0.0), levels - 1.0), 0.0)


def mip_view(levels, pose, pos, planes, camera='equirect', size=None, K=None, e=None, lod_bias=0.0, return_lod=False):
    """One view of one stack.  levels: [level 0, level 1, ..] as decoded arrays [D,H>>l,W>>l,4] (one entry: the plain bilinear
    render) -> rgb [oh,ow,3], depth [oh,ow] in fp64 (and lambda [D,oh,ow] with return_lod)."""
    levels = [np.asarray(x, D) for x in levels]
    nd, h, w, _ = levels[0].shape
    oh, ow = (h, w) if size is None else size
    r, c = view_rays(camera, oh, ow, pos, K, e)
    u, v = sphere_hits(r, c, pose, planes, w, h)
    L = len(levels)
    lam = lod(u, v, w, L, lod_bias)
    l0 = np.floor(lam).astype(np.int64)
    f = lam - l0
    l1 = np.minimum(l0 + 1, L - 1)
    rgb, dep = None, None
    for d in range(nd):
        at = [bilinear(levels[l][d], (u[d] + 0.5) * 0.5 ** l - 0.5, (v[d] + 0.5) * 0.5 ** l - 0.5) for l in range(L)]
        t0, t1 = np.zeros(at[0].shape, D), np.zeros(at[0].shape, D)
        for l in range(L):
            t0 = np.where((l0[d] == l)[..., None], at[l], t0)
            t1 = np.where((l1[d] == l)[..., None], at[l], t1)
        t = t0 + f[d][..., None] * (t1 - t0)
        a = t[..., 3]
        if d == 0:
            rgb, dep = t[..., :3], np.zeros(a.shape, D)
        else:
            rgb = t[..., :3] * a[..., None] + rgb * (1.0 - a[..., None])
            dep = (float(d) / nd) * a + dep * (1.0 - a)
    return (rgb, dep, lam) if return_lod else (rgb, dep)


def supersampled_view(base, pose, pos, planes, camera, size, factor=8, e=None):
    """The view at `size` as the box average of factor x factor plain bilinear samples per pixel: the lat-long grid of
    (factor * oh, factor * ow) subdivides every pixel of the (oh, ow) grid evenly.  ('equirect' and 'ods'.)"""
    oh, ow = size
    rgb, dep = mip_view([base], pose, pos, planes, camera, (factor * oh, factor * ow), e=e)
    return rgb.reshape(oh, factor, ow, factor, 3).mean(axis=(1, 3)), dep.reshape(oh, factor, ow, factor).mean(axis=(1, 3))


def near_nyquist_stack(seed, h=64, w=128, d=4):
    """A stack [D,H,W,4] (native order, fp32) with content near the Nyquist rate of its own grid: sinusoids of period ~4 texels,
    a 2-texel checker, noise, and blob-shaped alphas (layer 0 opaque) -- what a minified plain bilinear render aliases on."""
    rng = np.random.RandomState(seed)
    y, x = np.meshgrid(np.arange(h, dtype=D), np.arange(w, dtype=D), indexing='ij')
    out = np.zeros((d, h, w, 4), D)
    for k in range(d):
        ph = rng.uniform(0, 2 * np.pi, 4)
        out[k, ..., 0] = 0.8 * np.sin(2 * np.pi * x / (4.0 + 0.3 * k) + ph[0]) * np.cos(2 * np.pi * y / 4.5 + ph[1])
        out[k, ..., 1] = 0.7 * (((x // 2 + y // 2 + k) % 2) * 2 - 1)
        out[k, ..., 2] = 0.5 * np.sin(2 * np.pi * (x + y) / 3.7 + ph[2]) + 0.4 * rng.uniform(-1, 1, (h, w))
        if k == 0:
            out[k, ..., 3] = 1.0
        else:
            a = np.zeros((h, w), D)
            for _ in range(6):
                cy, cx, s = rng.uniform(0, h), rng.uniform(0, w), rng.uniform(3, 10)
                dx = np.minimum(np.abs(x - cx), w - np.abs(x - cx))
                a = np.maximum(a, np.exp(-(dx * dx + (y - cy) ** 2) / (2 * s * s)))
            out[k, ..., 3] = np.clip(1.3 * a - 0.15, 0, 1)
    return out.astype(F)
