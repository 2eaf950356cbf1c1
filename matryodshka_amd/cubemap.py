"""Cube-map conventions of the PP path (MSI.equirect_to_cube, MSI.infer_cube, MSI.cube_render_views; include/msi_hip.h
states the same table for the C ABI).  Host-side helpers only: small pose and camera algebra in numpy (torch tensors are
taken and returned as torch tensors on their device).

The cube frame is the camera frame of face 0: x right, y down, z forward.  Face f has orientation R_f = FACE_ROTATIONS[f],
whose COLUMNS are the face camera's x, y and z axes written in the cube frame:

    f          looks along   x axis      y axis      z axis
    0 front    +z            (1,0,0)     (0,1,0)     (0,0,1)
    1 right    +x            (0,0,-1)    (0,1,0)     (1,0,0)
    2 back     -z            (-1,0,0)    (0,1,0)     (0,0,-1)
    3 left     -x            (0,0,1)     (0,1,0)     (-1,0,0)
    4 up       -y            (1,0,0)     (0,0,1)     (0,-1,0)
    5 down     +y            (1,0,0)     (0,0,-1)    (0,1,0)

The renders' frame (render_views, cube_render_views: forward +x, down +y, right +z) is the cube frame with x and z swapped."""
import numpy as np

_AXES = [  # (x, y, z) axes of each face camera in the cube frame
    ((1, 0, 0), (0, 1, 0), (0, 0, 1)),
    ((0, 0, -1), (0, 1, 0), (1, 0, 0)),
    ((-1, 0, 0), (0, 1, 0), (0, 0, -1)),
    ((0, 0, 1), (0, 1, 0), (-1, 0, 0)),
    ((1, 0, 0), (0, 0, 1), (0, -1, 0)),
    ((1, 0, 0), (0, 0, -1), (0, 1, 0)),
]
FACE_ROTATIONS = np.stack([np.array(a, dtype=np.float64).T for a in _AXES])   # [6,3,3], columns = axes
FACE_ROTATIONS.setflags(write=False)
FACE_NAMES = ("front", "right", "back", "left", "up", "down")
_SWAP_XZ = np.array([[0, 0, 1], [0, 1, 0], [1, 0, 0]], dtype=np.float64)


def _face_4x4():
    f = np.tile(np.eye(4), (6, 1, 1))
    f[:, :3, :3] = FACE_ROTATIONS
    return f


def face_poses(pose):
    """[...,4,4] -> [...,6,4,4]: entry f is F_f^T @ pose @ F_f with F_f = diag(R_f, 1) -- a camera pose of the cube frame
    rewritten in each face's frame, the src_pose of format_network_input for that face.  Identity maps to identities and
    entry 0 is the input."""
    f = _face_4x4()
    try:
        import torch
    except ImportError:     # pragma: no cover
        torch = None
    if torch is not None and torch.is_tensor(pose):
        ft = torch.as_tensor(f, dtype=pose.dtype, device=pose.device)
        return ft.transpose(-1, -2) @ pose[..., None, :, :] @ ft
    pose = np.asarray(pose)
    out = np.swapaxes(f, -1, -2) @ pose[..., None, :, :].astype(np.float64) @ f
    return out.astype(pose.dtype if pose.dtype.kind == "f" else np.float64)


def face_view_pose(f):
    """The tgt_pose_rt [4,4] (fp32) with which a pinhole view from the centre of the cube looks through face f with the
    face camera's orientation: R_f carried to the render frame, swap @ R_f @ swap, no translation."""
    p = np.eye(4)
    p[:3, :3] = _SWAP_XZ @ FACE_ROTATIONS[int(f)] @ _SWAP_XZ
    return p.astype(np.float32)


def face_view_intrinsics(k):
    """The pinhole intrinsics (cx + 0.5, cy + 0.5) with which that view's pixel (i, j) lands exactly on texel (j, i) of the
    face: the pinhole camera of the renders looks through pixel CENTRES, ((j + 0.5 - cx) / fx), the stack camera K uses the
    MPI path's integer-pixel convention ((j - cx) / fx).  k [...,3,3] -> same shape, fp32."""
    k = np.array(k, dtype=np.float64, copy=True)
    k[..., 0, 2] += 0.5
    k[..., 1, 2] += 0.5
    return k.astype(np.float32)


def default_face_intrinsics(face_size):
    """The harness's PP intrinsics for a square face: fx = fy = cx = cy = S / 2 (a 90-degree face; it covers [-1, 1 - 2/S]
    in tan space).  [3,3] fp32."""
    s = float(face_size)
    return np.array([[s / 2, 0, s / 2], [0, s / 2, s / 2], [0, 0, 1]], dtype=np.float32)


# ---- the seamless filter of MSI.cube_render_views(filtering='seamless') (msi_cube_render_views_seamless) --------------------
# Defined for default_face_intrinsics only.  A face then stores tan = -1 .. 1 - 2/S and nothing on its +x and +y edges; the cube
# point of lattice point (x, y), 0 <= x, y <= S, of a face is a lattice point of every other face that contains it.  The rule
# (include/msi_hip.h and csrc/geo_cube.hip state the same): u, v are clamped to [0, S]; x0 = min(floor(u), S-1), x1 = x0 + 1,
# du = u - x0, likewise y; four bilinear taps with the clamp filter's weights and sum order; a tap with x < S and y < S is the
# face's own texel; a tap with x = S or y = S is a VIRTUAL texel at its cube point P (an edge point, or a cube corner when the
# other coordinate is 0 or S): the other faces containing P (one on an edge, two at a corner) are tried in ascending face index
# and the first whose lattice coordinates of P lie in [0, S-1]^2 supplies its texel; when none stores P, the virtual texel is
# the mean of the clamped texels (coordinates clamped to [0, S-1]) of all faces meeting at P, own face first, then the others in
# ascending index -- (a + b) * 0.5f, ((a + b) + c) * (1.0f / 3.0f) -- per channel, alpha included.
# Of the 12 cube edges 8 are stored by one face (the ring front -> right -> back -> left -> front, front/up, front/down,
# up/right, down/left: continuous filter), 2 by none (right/down, back/down: the mean, continuous over two texels) and 2 by both
# (up/back, up/left: each face keeps its own texel, a step in the CONTENT of the two faces remains; not a filtering artefact).
def _side_px(f, t, s):
    """Across x = S at running coordinate t = y: (neighbour, x', y') -- the kernel's cube_side_px."""
    return ((f + 1) & 3, 0, t) if f < 4 else ((1, s - t, 0) if f == 4 else (1, t, s))


def _side_py(f, t, s):
    """Across y = S at running coordinate t = x -- cube_side_py."""
    g = 5 if f < 4 else (0 if f == 4 else 2)
    if f in (0, 4):
        return g, t, 0
    return (g, s, t) if f == 1 else ((g, 0, s - t) if f == 3 else (g, s - t, s))


def _corner_ny(f, s):
    """The third face at corner (S, 0), across y = 0 -- cube_corner_ny."""
    return (4 if f < 4 else (2 if f == 4 else 0)), (s if f in (0, 1, 5) else 0), (s if f in (0, 3, 5) else 0)


def _corner_nx(f, s):
    """The third face at corner (0, S), across x = 0 -- cube_corner_nx."""
    return ((f + 3) & 3 if f < 4 else 3), (0 if f == 5 else s), (0 if f == 4 else s)


def virtual_texel(f, x, y, face_size):
    """The texels behind lattice point (x, y), 0 <= x, y <= S, of face f under the seamless filter, in closed form as the
    kernel derives them (cube_virtual_texel, csrc/geo_cube.hip): [(face, x', y', weight), ...] with every x', y' in [0, S-1]
    and the weights summing to 1.  One entry (weight 1) for an own texel or a point another face stores; the own clamped texel
    first and then the other faces in ascending index, weights 1/2 or 1/3, where no face stores the point."""
    f, x, y, s = int(f), int(x), int(y), int(face_size)
    if not (0 <= f < 6 and 0 <= x <= s and 0 <= y <= s and s >= 1):
        raise ValueError("virtual_texel: face in [0, 5] and 0 <= x, y <= S wanted, got f = %d, (x, y) = (%d, %d), S = %d" % (f, x, y, s))
    if x < s and y < s:
        return [(f, x, y, 1.0)]
    xs, ys = x == s, y == s
    cands = [_side_px(f, y, s) if xs else _side_py(f, x, s)]
    if xs and ys:
        cands.append(_side_py(f, x, s))
    elif xs and y == 0:
        cands.append(_corner_ny(f, s))
    elif ys and x == 0:
        cands.append(_corner_nx(f, s))
    cands.sort(key=lambda c: c[0])
    for g, gx, gy in cands:
        if gx < s and gy < s:
            return [(g, gx, gy, 1.0)]
    m = s - 1
    w = 1.0 / (1 + len(cands))
    return [(f, min(x, m), min(y, m), w)] + [(g, min(gx, m), min(gy, m), w) for g, gx, gy in cands]


def is_default_face_intrinsics(k, face_size):
    """True when every camera of k ([3,3] or [B,3,3]) has fx = fy = cx = cy = S/2 exactly: the camera the seamless filter needs."""
    k = np.asarray(k, dtype=np.float64).reshape(-1, 3, 3)
    h = face_size / 2.0
    return bool(np.all(k[:, [0, 1, 0, 1], [0, 1, 2, 2]] == h))


def cube_view_shapes(stack_shape, pose_shape, pos_shape, size):
    """The shape rules of MSI.cube_render_views, checked before anything touches a device: native stack [6B,D,S,S,4],
    tgt_pose_rt [B,V,4,4], tgt_pos [B,V,3] ([V,4,4] / [V,3] when B = 1), size = (h, w) required.
    Returns (B, V, S, D, h, w); ValueError otherwise."""
    stack_shape, pose_shape, pos_shape = tuple(stack_shape), tuple(pose_shape), tuple(pos_shape)
    if len(stack_shape) != 5 or stack_shape[-1] != 4:
        raise ValueError("cube_render_views: the stack must be [6B,S,S,D,4], got native shape %s" % (stack_shape,))
    n, d, h, w, _ = stack_shape
    if n == 0 or n % 6:
        raise ValueError("cube_render_views: the leading dimension is 6 faces per sample, %d is not a multiple of 6" % n)
    if h != w:
        raise ValueError("cube_render_views: cube faces are square, got %d x %d" % (h, w))
    if size is None:
        raise ValueError("cube_render_views: size=(h, w) is required for both cameras (a cube stack has no output size of its own)")
    oh, ow = int(size[0]), int(size[1])
    b = n // 6
    if b == 1 and len(pose_shape) == 3 and len(pos_shape) == 2:
        pose_shape, pos_shape = (1,) + pose_shape, (1,) + pos_shape
    if len(pose_shape) != 4 or pose_shape[0] != b or pose_shape[2:] != (4, 4):
        raise ValueError("tgt_pose_rt must be [B,V,4,4] with B = %d (or [V,4,4] for B = 1), got %s" % (b, pose_shape))
    v = pose_shape[1]
    if pos_shape != (b, v, 3):
        raise ValueError("tgt_pos must be [B,V,3] = %s, got %s" % ((b, v, 3), pos_shape))
    return b, v, h, d, oh, ow


def check_origin_inside(tgt_pos, pose, planes):
    """Host-side domain guard of MSI.cube_render_views: every view's ray origin, pose @ (tgt_pos[2], tgt_pos[1], tgt_pos[0], 1),
    must lie strictly inside the innermost cube shell (max_k |o_k| < min planes; the x <-> z swap into the cube frame does not
    change that maximum).  ValueError otherwise (NaN included).  Host arrays only: the caller skips it for device inputs."""
    tp = np.asarray(tgt_pos, dtype=np.float64).reshape(-1, 3)
    ps = np.asarray(pose, dtype=np.float64).reshape(-1, 4, 4)
    if ps.shape[0] != tp.shape[0]:
        return      # the shape check reports it
    c = np.stack([tp[:, 2], tp[:, 1], tp[:, 0]], axis=1)
    origin = np.einsum('bij,bj->bi', ps[:, :3, :3], c) + ps[:, :3, 3]
    hmin = float(np.min(np.asarray(planes, dtype=np.float64)))
    if not np.all(np.abs(origin).max(axis=1) < hmin):
        raise ValueError("the target ray origin (pose @ tgt_pos) must lie inside the innermost cube shell (half-side %g)" % hmin)


def check_ods_circle_inside(tgt_pos, pose, planes, radius):
    """check_origin_inside for MSI.cube_render_views(camera='ods'): with o the posed head position pose @ (tgt_pos[2], tgt_pos[1],
    tgt_pos[0], 1) and e = radius [B*V] (eye * baseline, signed), max_k |o_k| + |e| < min planes must hold.  A point of the viewing
    circle is o + R (sin S, 0, -cos S) e and every component of a rotated unit vector is at most 1, so no component of the offset
    exceeds |e| under any rotation: the bound keeps the WHOLE circle strictly inside the innermost shell (sufficient, not necessary).
    ValueError otherwise (NaN included).  Host arrays only."""
    tp = np.asarray(tgt_pos, dtype=np.float64).reshape(-1, 3)
    ps = np.asarray(pose, dtype=np.float64).reshape(-1, 4, 4)
    e = np.abs(np.asarray(radius, dtype=np.float64).reshape(-1))
    if ps.shape[0] != tp.shape[0] or e.shape[0] != tp.shape[0]:
        return      # the shape checks report it
    c = np.stack([tp[:, 2], tp[:, 1], tp[:, 0]], axis=1)
    origin = np.einsum('bij,bj->bi', ps[:, :3, :3], c) + ps[:, :3, 3]
    hmin = float(np.min(np.asarray(planes, dtype=np.float64)))
    if not np.all(np.abs(origin).max(axis=1) + e < hmin):
        raise ValueError("the ODS viewing circle (max_k |(pose @ tgt_pos)_k| + |eye * baseline|) must lie inside the innermost cube "
                         "shell (half-side %g)" % hmin)


CAMERAS = ('equirect', 'pinhole', 'ods')


def check_ods_arguments(camera, eye, baseline):
    """The rules of MSI.cube_render_views' camera, eye and baseline, checked before anything touches a device: an unknown
    camera; eye or baseline with a camera other than 'ods'; 'ods' without eye, or without baseline (a cube stack carries no ODS
    intrinsics to default from); a host-side baseline that is negative or not finite.  ValueError; returns camera == 'ods'."""
    if camera not in CAMERAS:
        raise ValueError("camera must be 'equirect', 'pinhole' or 'ods', not %r" % (camera,))
    ods = camera == 'ods'
    if not ods and (eye is not None or baseline is not None):
        raise ValueError("cube_render_views: eye and baseline belong to camera='ods', not %r" % (camera,))
    if ods and eye is None:
        raise ValueError("cube_render_views: camera='ods' needs eye (+1 / 'left' or -1 / 'right', or an array [V] / [B,V])")
    if ods and baseline is None:
        raise ValueError("cube_render_views: camera='ods' needs baseline (a cube stack carries no ODS intrinsics to take it from)")
    if ods and not (hasattr(baseline, "is_cuda") and baseline.is_cuda):
        bl = np.asarray(baseline, dtype=np.float64)
        if not (np.all(np.isfinite(bl)) and np.all(bl >= 0)):
            raise ValueError("baseline must be finite and >= 0")
    return ods
