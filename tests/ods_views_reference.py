"""The composed CPU reference of the ODS camera of MSI.render_views (msi_render_ods_views), built like oracle_view of
tests/test_gpu_render_views.py from the oracle's primitives: the lat-long rays of the OUTPUT size, the origin on the viewing
circle in fp32 and in the kernel's op order, _transform_ray, _sphere_hit_pixels with the stack's (W, H), resample and
over_composite[_depth].  Shared by the CPU facts (test_ods_views_cpu.py) and the GPU tests (test_gpu_ods_views.py)."""
import numpy as np

from oracle import geometry as G

F = np.float32


def ods_rays(oh, ow, pos, e, rows=None):
    """Rays of one ODS view before the pose: direction r = (cosS cosT, sinT, sinS cosT), the equirect camera's, and origin
    c = (pos[2] + sinS * e, pos[1], pos[0] + (-cosS) * e), each [len(rows), ow]; e = eye * baseline (signed, fp32)."""
    rows = np.arange(oh) if rows is None else np.asarray(rows)
    S, T = G.lat_long_grid((oh, ow))
    S, T = S[rows], T[rows]
    cs, ss, cosT = G.cos_f32(S), G.sin_f32(S), G.cos_f32(T)
    e = F(e)
    r = (cs * cosT, G.sin_f32(T), ss * cosT)
    c = ((F(pos[2]) + ss * e).astype(F), np.full_like(cs, F(pos[1])), (F(pos[0]) + (-cs) * e).astype(F))
    return r, c


def oracle_ods_view(rgba, pose, pos, e, planes, size=None, rows=None):
    """One ODS view of one stack: rgba [H,W,D,4]; pose [4,4]; pos [3]; e the signed radius -> rgb [rows,w,3], depth [rows,w]."""
    h, w, d, _ = rgba.shape
    oh, ow = (h, w) if size is None else size
    r, c = ods_rays(oh, ow, pos, e, rows)
    r, c = G._transform_ray(r, c, pose)
    radius = np.asarray(planes, F).reshape(-1, 1, 1)
    pix = G._sphere_hit_pixels(r, c, radius, w, h)                   # [D,rows,w,2]
    layers = np.transpose(rgba, (2, 0, 1, 3))                         # [D,H,W,4]
    warped = G.resample(layers, pix)
    ws = [warped[k] for k in range(d)]
    return G.over_composite(ws), G.over_composite_depth(ws)[..., 0]


def smooth_image(h, w):
    """A smooth, asymmetric [h,w,3] image in [-1,1]: periodic in longitude, no left-right or up-down symmetry (so a mirror, a
    flip or the other eye cannot reproduce it)."""
    S, T = G.lat_long_grid((h, w))
    S, T = S.astype(np.float64), T.astype(np.float64)
    img = np.stack([np.sin(S + 0.4) * np.cos(T), 0.7 * np.sin(2 * S - 1.1) * np.cos(T) + 0.3 * np.sin(T),
                    0.6 * np.cos(S - 2.0) + 0.4 * np.sin(T + 0.3) * np.sin(S)], axis=-1)
    return np.clip(img, -1, 1).astype(F)


def swept_single_layer(image, order, depth=1.5, baseline=0.2):
    """Fact 3's stack: `image` [h,w,3] swept with ods_sphere_sweep(order, depths=[depth], baseline) at identity pose, as ONE
    opaque layer -> (rgba [h,w,1,4], planes [depth])."""
    h, w, _ = image.shape
    intr = np.zeros((1, 3, 3), F)
    intr[0, 0, 0] = baseline
    swept = G.ods_sphere_sweep(image[None], order, [depth], np.eye(4, dtype=F)[None], intr)[0]      # [h,w,3]
    rgba = np.concatenate([swept, np.ones((h, w, 1), F)], axis=-1)[:, :, None, :]
    return np.ascontiguousarray(rgba), [depth]
