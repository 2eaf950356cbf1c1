"""The fp64 statement of the anisotropic texel rule of msi_render_views_aniso (include/msi_hip.h), built from the pieces of
tests/mip_reference.py: its rays, sphere hits, neighbour choice and wrap-around bilinear lookup.  Per layer the four hit differences
are the 2 x 2 footprint Jacobian; its singular values give the level (from the minor axis, capped at max_anisotropy) and the number
of trilinear samples along the major axis.  Shared by the CPU facts (test_aniso_cpu.py) and the GPU tests
(test_gpu_aniso_views.py)."""
import numpy as np

from tests import mip_reference as R

D = np.float64


def footprint(u, v, width, levels, lod_bias, max_anisotropy):
    """(u, v) [D,oh,ow] of the stack's own size -> ratio, lambda, step and the unit major axis (mu_u, mu_v), [D,oh,ow] each."""
    nx, ny = R.neighbour(u.shape[2]), R.neighbour(u.shape[1])
    du_x, dv_x = u[:, :, nx] - u, v[:, :, nx] - v
    du_y, dv_y = u[:, ny, :] - u, v[:, ny, :] - v
    du_x, du_y = du_x - width * np.rint(du_x / width), du_y - width * np.rint(du_y / width)
    E, G, Fm = du_x * du_x + du_y * du_y, dv_x * dv_x + dv_y * dv_y, du_x * dv_x + du_y * dv_y
    h = 0.5 * (E - G)
    Rr = np.hypot(h, Fm)
    s_max = np.sqrt(0.5 * (E + G) + Rr)
    with np.errstate(divide='ignore', invalid='ignore'):
        s_min = np.abs(du_x * dv_y - du_y * dv_x) / s_max
        ratio = np.where(s_max > 1.0, np.minimum(np.maximum(s_max / np.maximum(s_min, 1.0), 1.0), max_anisotropy), 1.0)
        step = s_max / ratio
        lam = np.where(step > 0, np.minimum(np.maximum(np.log2(step) + lod_bias, 0.0), levels - 1.0), 0.0)
        a_u, a_v = np.where(h >= 0, h + Rr, Fm), np.where(h >= 0, Fm, Rr - h)
        n = np.hypot(a_u, a_v)
        mu_u, mu_v = np.where(n > 0, a_u / n, 1.0), np.where(n > 0, a_v / n, 0.0)
    return ratio, lam, step, mu_u, mu_v


def sample_count(ratio):
    """M of every (layer, pixel): the samples are m = -M .. M."""
    return np.ceil(0.5 * (ratio - 1.0)).astype(np.int64)


def weight(ratio, m):
    """w_m: a box of length `ratio` cut into unit cells around the samples."""
    return np.clip(0.5 * ratio - (abs(m) - 0.5), 0.0, 1.0) / ratio


def aniso_view(levels, pose, pos, planes, camera='equirect', size=None, K=None, e=None, lod_bias=0.0, max_anisotropy=8.0, details=False):
    """One view of one stack.  levels: [level 0, level 1, ..] as decoded arrays [D,H>>l,W>>l,4] -> rgb [oh,ow,3], depth [oh,ow] in
    fp64 (and ratio, lambda [D,oh,ow] with details).  lod_bias <= -64 is the plain render: the filter is skipped."""
    levels = [np.asarray(x, D) for x in levels]
    nd, h, w, _ = levels[0].shape
    oh, ow = (h, w) if size is None else size
    r, c = R.view_rays(camera, oh, ow, pos, K, e)
    u, v = R.sphere_hits(r, c, pose, planes, w, h)
    L = len(levels)
    if lod_bias <= -64.0:
        ratio, lam = np.ones(u.shape, D), np.zeros(u.shape, D)
        step = mu_u = mu_v = np.zeros(u.shape, D)
    else:
        ratio, lam, step, mu_u, mu_v = footprint(u, v, w, L, lod_bias, float(max_anisotropy))
    l0 = np.floor(lam).astype(np.int64)
    f = lam - l0
    l1 = np.minimum(l0 + 1, L - 1)
    M = sample_count(ratio)
    rgb, dep = None, None
    for d in range(nd):
        t = None
        for k in range(2 * int(M[d].max()) + 1):                 # the kernel's order: the centre, then +1, -1, +2, -2, ..
            m = (k + 1) // 2 * (1 if k % 2 else -1)
            mine = abs(m) <= M[d]
            with np.errstate(invalid='ignore'):
                uu = np.where(mine, u[d] + m * (step[d] * mu_u[d]), u[d]) if m else u[d]
                vv = np.where(mine, v[d] + m * (step[d] * mu_v[d]), v[d]) if m else v[d]
            at = [R.bilinear(levels[l][d], (uu + 0.5) * 0.5 ** l - 0.5, (vv + 0.5) * 0.5 ** l - 0.5) for l in range(L)]
            t0, t1 = np.zeros(at[0].shape, D), np.zeros(at[0].shape, D)
            for l in range(L):
                t0 = np.where((l0[d] == l)[..., None], at[l], t0)
                t1 = np.where((l1[d] == l)[..., None], at[l], t1)
            s = np.where((f[d] > 0)[..., None], t0 + f[d][..., None] * (t1 - t0), t0)
            wm = np.where(mine, weight(ratio[d], m), 0.0)[..., None]
            t = wm * s if t is None else np.where(mine[..., None], t + wm * s, t)
        a = t[..., 3]
        if d == 0:
            rgb, dep = t[..., :3], np.zeros(a.shape, D)
        else:
            rgb = t[..., :3] * a[..., None] + rgb * (1.0 - a[..., None])
            dep = (float(d) / nd) * a + dep * (1.0 - a)
    return (rgb, dep, ratio, lam) if details else (rgb, dep)
