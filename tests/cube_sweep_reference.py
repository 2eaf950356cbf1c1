"""fp64 numpy reference of the cube path's panorama sampling (msi_cube_plane_sweep_f32 and what is built on it), written from the
definition alone; it calls nothing of the package.  The face table is restated here on purpose.

For face f = n % 6 of entry n of a [6B,...] batch, pixel (i, j) and plane depth d, with P the face's source pose and K the face camera:
    X = (d S_j cx / fx, d T_i cy / fy, d)              backproject_planar on spherical.uv_grid
    Y = apply_pose(P, apply_pose(P, X))                 the pose twice, as the face sweep applies it (pr = K Y)
    dir = R_f Y                                         R_f: the face camera's axes as columns
    lon = atan2(dir_x + 0, dir_z + 0), lat = asin(dir_y / |dir|)
    u = (lon + pi) / 2pi Wp - 0.5, v = (lat + pi/2) / pi Hp - 0.5;  u clamped to [-0.5, Wp - 0.5] and wrapped, v clamped to [0, Hp - 1]
    value = bilinear(panorama[n // 6], u, v)
The face sweep this replaces samples the face's own image at (pr0 / pr2, pr1 / pr2) with a sampler that wraps in both axes."""
import numpy as np

FACE_AXES = [  # (x axis, y axis, z axis) of each face camera in the cube frame
    ((1, 0, 0), (0, 1, 0), (0, 0, 1)),      # 0 front  +z
    ((0, 0, -1), (0, 1, 0), (1, 0, 0)),     # 1 right  +x
    ((-1, 0, 0), (0, 1, 0), (0, 0, -1)),    # 2 back   -z
    ((0, 0, 1), (0, 1, 0), (-1, 0, 0)),     # 3 left   -x
    ((1, 0, 0), (0, 0, 1), (0, -1, 0)),     # 4 up     -y
    ((1, 0, 0), (0, 0, -1), (0, 1, 0)),     # 5 down   +y
]
R = np.stack([np.array(a, dtype=np.float64).T for a in FACE_AXES])      # [6,3,3], columns = axes


def face_poses(pose):
    """[B,4,4] cube-frame source poses -> [6B,4,4]: F_f^T pose F_f with F_f = diag(R_f, 1), the pose written in each face's frame."""
    pose = np.asarray(pose, np.float64).reshape(-1, 4, 4)
    f = np.tile(np.eye(4), (6, 1, 1))
    f[:, :3, :3] = R
    return (np.swapaxes(f, -1, -2)[None] @ pose[:, None] @ f[None]).reshape(-1, 4, 4)


def uv_grid(n):
    """spherical.uv_grid: linspace(-1 + 1/n, 1 - 1/n, n)."""
    s0, s1 = -1.0 + 1.0 / n, 1.0 - 1.0 / n
    return s0 + (s1 - s0) / (n - 1) * np.arange(n, dtype=np.float64)


def plane_points(face_pose, k, planes, size):
    """Y [N,S,S,D,3]: backproject_planar, then the pose twice."""
    p = np.asarray(face_pose, np.float64).reshape(-1, 4, 4)
    k = np.asarray(k, np.float64).reshape(-1, 3, 3)
    g = uv_grid(size)
    d = np.asarray(planes, np.float64)
    fx, fy, cx, cy = (k[:, a, b][:, None, None, None] for a, b in ((0, 0), (1, 1), (0, 2), (1, 2)))
    sj, ti, dd = g[None, None, :, None], g[None, :, None, None], d[None, None, None, :]
    x = np.stack(np.broadcast_arrays(dd * sj * cx / fx, dd * ti * cy / fy, dd * np.ones_like(sj * ti * cx)), axis=-1)    # [N,S,S,D,3]
    rot, t = p[:, None, None, None, :3, :3], p[:, None, None, None, :3, 3]
    a = np.einsum('...ij,...j->...i', rot, x) + t
    return np.einsum('...ij,...j->...i', rot, a) + t


def panorama_uv(y, faces_of=None):
    """Cube-frame direction, its lat-long angles and |Y| for plane points y [N,...,3] of a [6B] batch -> (lon, lat, coslat, norm)."""
    n = y.shape[0]
    f = np.arange(n) % 6 if faces_of is None else np.asarray(faces_of)
    dcube = np.einsum('nij,n...j->n...i', R[f], y)
    norm = np.linalg.norm(dcube, axis=-1)
    with np.errstate(divide='ignore', invalid='ignore'):
        lon = np.arctan2(dcube[..., 0] + 0.0, dcube[..., 2] + 0.0)
        s = np.clip(dcube[..., 1] / norm, -1.0, 1.0)
        lat = np.arcsin(s)
        coslat = np.hypot(dcube[..., 0], dcube[..., 2]) / norm
    return lon, lat, coslat, norm


def bilinear_panorama(pano, u, v):
    """pano [Hp,Wp,C], u / v of any one shape -> [..., C]: u clamped to [-0.5, Wp - 0.5] and wrapped, v clamped to [0, Hp - 1]; a NaN coordinate
    is the lower bound."""
    pano = np.asarray(pano, np.float64)
    hp, wp = pano.shape[:2]
    u = np.clip(np.where(np.isnan(u), -0.5, u), -0.5, wp - 0.5)
    v = np.clip(np.where(np.isnan(v), 0.0, v), 0.0, hp - 1.0)
    x0, y0 = np.floor(u).astype(np.int64), np.floor(v).astype(np.int64)
    du, dv = (u - x0)[..., None], (v - y0)[..., None]
    x1, y1 = (x0 + 1) % wp, np.minimum(y0 + 1, hp - 1)
    x0 = x0 % wp
    return (pano[y0, x0] * (1 - dv) * (1 - du) + pano[y0, x1] * (1 - dv) * du + pano[y1, x0] * dv * (1 - du) + pano[y1, x1] * dv * du)


def cube_sweep(panorama, face_pose, k, planes, size):
    """panorama [B,Hp,Wp,3], face_pose [6B,4,4], k [6B,3,3] -> dict:
      value   [6B,S,S,D,3]  the sweep (channel 3 d + c of the volume's window is value[..., d, c])
      u, v    [6B,S,S,D]    the panorama position before the clamps
      u_face, v_face, pr2   the face sweep's position (pr0 / pr2, pr1 / pr2) and pr2, pr = K Y
      coslat, norm          cos(lat) and |Y|: where either is tiny the longitude / the direction is ill-conditioned"""
    panorama = np.asarray(panorama, np.float64)
    b, hp, wp, _ = panorama.shape
    kk = np.asarray(k, np.float64).reshape(-1, 3, 3)
    y = plane_points(face_pose, kk, planes, size)
    assert y.shape[0] == 6 * b
    lon, lat, coslat, norm = panorama_uv(y)
    u = (lon + np.pi) / (2 * np.pi) * wp - 0.5
    v = (lat + np.pi / 2) / np.pi * hp - 0.5
    value = np.stack([bilinear_panorama(panorama[n // 6], u[n], v[n]) for n in range(6 * b)])
    pr = np.einsum('nij,n...j->n...i', kk, y)
    with np.errstate(divide='ignore', invalid='ignore'):
        uf, vf = pr[..., 0] / pr[..., 2], pr[..., 1] / pr[..., 2]
    return dict(value=value, u=u, v=v, u_face=uf, v_face=vf, pr2=pr[..., 2], coslat=coslat, norm=norm)


def face_sweep(faces, face_pose, k, planes):
    """The face-wise sweep in fp64: faces [N,S,S,3] sampled at (pr0 / pr2, pr1 / pr2) with the wrap-around sampler (weights from the unwrapped
    corners, indices modulo the face in both axes) -> [N,S,S,D,3]."""
    faces = np.asarray(faces, np.float64)
    n, s = faces.shape[:2]
    kk = np.asarray(k, np.float64).reshape(-1, 3, 3)
    y = plane_points(face_pose, kk, planes, s)
    pr = np.einsum('nij,n...j->n...i', kk, y)
    with np.errstate(divide='ignore', invalid='ignore'):
        u, v = pr[..., 0] / pr[..., 2], pr[..., 1] / pr[..., 2]
    x0, y0 = np.floor(u).astype(np.int64), np.floor(v).astype(np.int64)
    du, dv = (u - x0)[..., None], (v - y0)[..., None]
    idx = np.arange(n)[:, None, None, None]
    tap = lambda yy, xx: faces[idx, yy % s, xx % s]
    return tap(y0, x0) * (1 - dv) * (1 - du) + tap(y0, x0 + 1) * (1 - dv) * du + tap(y0 + 1, x0) * dv * (1 - du) + tap(y0 + 1, x0 + 1) * dv * du


def outside_face(ref, size):
    """Samples whose face position lies outside [0, S-1]^2 (or behind the camera / at infinity): where the face sweep wraps."""
    with np.errstate(invalid='ignore'):
        inside = (ref["u_face"] >= 0) & (ref["u_face"] <= size - 1) & (ref["v_face"] >= 0) & (ref["v_face"] <= size - 1) & (ref["pr2"] > 0)
    return ~inside


def excluded(ref, margin=1e-3):
    """The pole / centre margin: cos(lat) < margin (the longitude is ill-conditioned) or |Y| < margin (the direction is)."""
    with np.errstate(invalid='ignore'):
        return ~((ref["coslat"] >= margin) & (ref["norm"] >= margin))
