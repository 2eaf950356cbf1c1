"""fp64 numpy reference of the cube-map viewer (MSI.cube_render_views, MSI.equirect_to_cube), written from the conventions
alone; it calls nothing of the package.  The face table is restated here on purpose (tests compare it with the package's).

Cube frame = camera frame of face 0 (x right, y down, z forward).  R_f has the face camera's x, y, z axes as COLUMNS.
Texel (ix, iy) of layer d of face f is R_f planes[d] K^-1 (ix, iy, 1).  The render frame of the target cameras (forward +x,
down +y, right +z) is the cube frame with x and z swapped."""
import numpy as np

FACE_AXES = [  # (x axis, y axis, z axis) of each face camera in the cube frame
    ((1, 0, 0), (0, 1, 0), (0, 0, 1)),      # 0 front  +z
    ((0, 0, -1), (0, 1, 0), (1, 0, 0)),     # 1 right  +x
    ((-1, 0, 0), (0, 1, 0), (0, 0, -1)),    # 2 back   -z
    ((0, 0, 1), (0, 1, 0), (-1, 0, 0)),     # 3 left   -x
    ((1, 0, 0), (0, 0, 1), (0, -1, 0)),     # 4 up     -y
    ((1, 0, 0), (0, 0, -1), (0, 1, 0)),     # 5 down   +y
]
R = np.stack([np.array(a, dtype=np.float64).T for a in FACE_AXES])


def target_rays(camera, size, pose, tgt_pos, intrinsics=None):
    """(origin [3], directions [h,w,3]) in the CUBE frame for one view."""
    h, w = size
    pose = np.asarray(pose, np.float64)
    if camera == 'equirect':
        lon = -np.pi + (np.arange(w) + 0.5) * (2 * np.pi / w)
        lat = -np.pi / 2 + (np.arange(h) + 0.5) * (np.pi / h)
        lon, lat = np.meshgrid(lon, lat)
        r = np.stack([np.cos(lon) * np.cos(lat), np.sin(lat), np.sin(lon) * np.cos(lat)], axis=-1)
    else:
        k = np.asarray(intrinsics, np.float64)
        j, i = np.meshgrid(np.arange(w, dtype=np.float64), np.arange(h, dtype=np.float64))
        r = np.stack([np.ones_like(j), (i + 0.5 - k[1, 2]) / k[1, 1], (j + 0.5 - k[0, 2]) / k[0, 0]], axis=-1)
    r = r @ pose[:3, :3].T
    tp = np.asarray(tgt_pos, np.float64)
    o = pose[:3, :3] @ np.array([tp[2], tp[1], tp[0]]) + pose[:3, 3]
    return o[::-1].copy(), r[..., ::-1].copy()          # render frame -> cube frame: x <-> z


def _hit(o, r, h):
    """Point where the ray leaves the cube shell of half-side h: t = min_k (h sign(r_k) - o_k) / r_k over r_k != 0."""
    with np.errstate(divide='ignore', invalid='ignore'):
        t = np.where(r != 0, (h * np.sign(r) - o) / r, np.inf)
    return o + t.min(axis=-1, keepdims=True) * r


def _face_of(p):
    """Face index and p = R_f^T P: the axis of the largest |P_k| with its sign, ties z, x, y."""
    a = np.abs(p)
    order = np.array([2, 0, 1])                           # z, x, y
    axis = order[np.argmax(a[..., order], axis=-1)]       # argmax takes the first of equals
    val = np.take_along_axis(p, axis[..., None], axis=-1)[..., 0]
    table = {(2, False): 0, (0, False): 1, (2, True): 2, (0, True): 3, (1, True): 4, (1, False): 5}
    f = np.empty(axis.shape, dtype=np.int64)
    for (ax, neg), idx in table.items():
        f[(axis == ax) & ((val < 0) == neg)] = idx
    q = np.einsum('...ji,...j->...i', R[f], p)
    return f, q


def render_view(stack, planes, k, pose, tgt_pos, camera, size, intrinsics=None):
    """One view of one cube.  stack [6,S,S,D,4] (public layout; layer 0 farthest), k = stack camera [3,3].
    Returns dict(rgb [h,w,3], depth [h,w], margin [h,w], clamped [h,w]): margin = min over the shells of
    1 - second-largest |P_k| / h (distance from a cube edge, where the face choice is discontinuous); clamped = some shell's
    sample coordinate was outside [0, S-1] before the clamp."""
    stack = np.asarray(stack)                             # (converted to fp64 tap by tap: a full-size stack stays as it is)
    s, d = stack.shape[1], stack.shape[3]
    k = np.asarray(k, np.float64)
    o, r = target_rays(camera, size, pose, tgt_pos, intrinsics)
    rgb = dep = None
    margin = np.full(r.shape[:2], np.inf)
    clamped = np.zeros(r.shape[:2], dtype=bool)
    for l in range(d):
        h = float(planes[l])
        p = _hit(o, r, h)
        margin = np.minimum(margin, 1.0 - np.sort(np.abs(p), axis=-1)[..., 1] / h)
        f, q = _face_of(p)
        u = k[0, 0] * q[..., 0] / h + k[0, 2]
        v = k[1, 1] * q[..., 1] / h + k[1, 2]
        clamped |= (u < 0) | (u > s - 1) | (v < 0) | (v > s - 1)
        u, v = np.clip(u, 0, s - 1), np.clip(v, 0, s - 1)
        x0, y0 = np.floor(u).astype(np.int64), np.floor(v).astype(np.int64)
        x1, y1 = np.minimum(x0 + 1, s - 1), np.minimum(y0 + 1, s - 1)
        du, dv = (u - x0)[..., None], (v - y0)[..., None]
        tex = stack[:, :, :, l, :]
        tap = lambda yy, xx: tex[f, yy, xx].astype(np.float64)
        val = (tap(y0, x0) * (1 - dv) * (1 - du) + tap(y0, x1) * (1 - dv) * du +
               tap(y1, x0) * dv * (1 - du) + tap(y1, x1) * dv * du)
        a = val[..., 3:]
        if l == 0:
            rgb, dep = val[..., :3], np.zeros(val.shape[:2])
        else:
            rgb = val[..., :3] * a + rgb * (1 - a)
            dep = (l / d) * a[..., 0] + dep * (1 - a[..., 0])
    return dict(rgb=rgb, depth=dep, margin=margin, clamped=clamped)


def render_views(stack, planes, k, pose, tgt_pos, camera, size, intrinsics=None):
    """stack [6B,S,S,D,4], pose [B,V,4,4], tgt_pos [B,V,3], k [3,3], intrinsics [3,3] or None ->
    dict of rgb [B,V,h,w,3], depth / margin / clamped [B,V,h,w]."""
    b_, v_ = np.asarray(pose).shape[:2]
    outs = [[render_view(stack[6 * b:6 * b + 6], planes, k, pose[b][v], tgt_pos[b][v], camera, size, intrinsics)
             for v in range(v_)] for b in range(b_)]
    return {key: np.stack([np.stack([o[key] for o in row]) for row in outs]) for key in ("rgb", "depth", "margin", "clamped")}


def over_composite(face_stack):
    """Plain per-texel composite of one face's layers [S,S,D,4] -> (rgb [S,S,3], depth [S,S])."""
    x = np.asarray(face_stack, np.float64)
    d = x.shape[2]
    rgb, dep = x[:, :, 0, :3], np.zeros(x.shape[:2])
    for l in range(1, d):
        a = x[:, :, l, 3:]
        rgb = x[:, :, l, :3] * a + rgb * (1 - a)
        dep = (l / d) * a[..., 0] + dep * (1 - a[..., 0])
    return rgb, dep


def equirect_to_cube(image, face_size, k):
    """image [B,H,W,C] -> [B,6,S,S,C]: texel (ix, iy) of face f looks along R_f K^-1 (ix, iy, 1); x <-> z into the render
    frame; u = (atan2(z, x) + pi) / 2pi W - 0.5, v = (asin(y / |dir|) + pi/2) / pi H - 0.5; bilinear, wrapping in u and
    clamping in v.  A texel that looks straight at a pole has longitude 0."""
    image = np.asarray(image, np.float64)
    b, h, w, c = image.shape
    s = int(face_size)
    k = np.asarray(k, np.float64)
    ix, iy = np.meshgrid(np.arange(s, dtype=np.float64), np.arange(s, dtype=np.float64))
    q = np.stack([(ix - k[0, 2]) / k[0, 0], (iy - k[1, 2]) / k[1, 1], np.ones_like(ix)], axis=-1)
    out = np.empty((b, 6, s, s, c))
    for f in range(6):
        dcube = q @ R[f].T
        x, y, z = dcube[..., 2], dcube[..., 1], dcube[..., 0]       # render frame
        lon = np.arctan2(z + 0.0, x + 0.0)                             # (-0 -> +0: at a pole, atan2(+0, +0) = 0 on either face)
        lat = np.arcsin(y / np.linalg.norm(dcube, axis=-1))
        u = (lon + np.pi) / (2 * np.pi) * w - 0.5
        v = np.clip((lat + np.pi / 2) / np.pi * h - 0.5, 0, h - 1)
        x0, y0 = np.floor(u).astype(np.int64), np.floor(v).astype(np.int64)
        du, dv = (u - x0)[..., None], (v - y0)[..., None]
        x1, y1 = (x0 + 1) % w, np.minimum(y0 + 1, h - 1)
        x0 = x0 % w
        out[:, f] = (image[:, y0, x0] * (1 - dv) * (1 - du) + image[:, y0, x1] * (1 - dv) * du +
                     image[:, y1, x0] * dv * (1 - du) + image[:, y1, x1] * dv * du)
    return out
