"""fp64 numpy reference of the ODS stereo camera of the cube-map viewer (MSI.cube_render_views(camera='ods')), written from the
convention; it calls nothing of the package.

The camera is the equirect camera of tests/cube_reference.py with the ray origin moved onto the viewing circle of the view.  For
pixel (i, j) of the lat-long grid of the output, before the pose (render frame: forward +x, down +y, right +z):
    direction  r = (cos S_j cos T_i, sin T_i, sin S_j cos T_i)
    origin     c = (tgt_pos[2] + sin S_j * e, tgt_pos[1], tgt_pos[0] - cos S_j * e),   e = eye * baseline (signed: e > 0 left eye)
then r <- pose[:3,:3] r, c <- pose (c, 1), then x <-> z into the cube frame.

Everything after the ray -- shell hit, face choice, taps, composite, edge margin -- is the per-shell logic of
tests/cube_reference.py (clamp) and tests/cube_seamless_reference.py (seamless), unchanged: both take their rays from
cube_reference.target_rays and broadcast the origin against the directions, so a per-pixel origin [h,w,3] goes through the same
lines as the single origin [3].  This module WRAPS them: for the duration of a call target_rays is the ODS ray builder below.
The posed origin is written as (posed head position) + pose[:3,:3] (circle offset): the same point (the pose is affine), and with
e = 0 the offset is an exact zero, so the e = 0 render IS cube_reference.render_view(camera='equirect'), element for element."""
import contextlib

import numpy as np

from tests import cube_reference as ref
from tests import cube_seamless_reference as sref


def ods_rays(size, pose, tgt_pos, e):
    """(origins [h,w,3], directions [h,w,3], head position [3]) in the CUBE frame for one view with signed eye radius e."""
    h, w = size
    pose = np.asarray(pose, np.float64)
    lon = -np.pi + (np.arange(w) + 0.5) * (2 * np.pi / w)
    lat = -np.pi / 2 + (np.arange(h) + 0.5) * (np.pi / h)
    lon, lat = np.meshgrid(lon, lat)
    r = np.stack([np.cos(lon) * np.cos(lat), np.sin(lat), np.sin(lon) * np.cos(lat)], axis=-1)
    r = r @ pose[:3, :3].T
    tp = np.asarray(tgt_pos, np.float64)
    head = pose[:3, :3] @ np.array([tp[2], tp[1], tp[0]]) + pose[:3, 3]
    e = float(e)
    off = np.stack([np.sin(lon) * e, np.zeros_like(lon), -np.cos(lon) * e], axis=-1) @ pose[:3, :3].T
    o = head + off
    return o[..., ::-1].copy(), r[..., ::-1].copy(), head[::-1].copy()       # render frame -> cube frame: x <-> z


@contextlib.contextmanager
def _ods_camera(e):
    """cube_reference.target_rays (which cube_seamless_reference calls through the module too) answers with the ODS rays."""
    saved = ref.target_rays

    def target_rays(camera, size, pose, tgt_pos, intrinsics=None):
        assert camera == 'equirect', "the ODS camera is the equirect camera with another origin"
        return ods_rays(size, pose, tgt_pos, e)[:2]
    ref.target_rays = target_rays
    try:
        yield
    finally:
        ref.target_rays = saved


def render_view(stack, planes, k, pose, tgt_pos, e, size, seamless=False):
    """One eye panorama of one cube.  stack [6,S,S,D,4], k = stack camera [3,3], e = eye * baseline.  Returns
    cube_reference.render_view's dict (rgb, depth, margin, clamped) or, seamless, cube_seamless_reference.render_view's
    (rgb, depth, margin, strip, corner)."""
    with _ods_camera(e):
        if seamless:
            return sref.render_view(stack, planes, k, pose, tgt_pos, 'equirect', size)
        return ref.render_view(stack, planes, k, pose, tgt_pos, 'equirect', size)


def render_views(stack, planes, k, pose, tgt_pos, radius, size, seamless=False):
    """stack [6B,S,S,D,4], pose [B,V,4,4], tgt_pos [B,V,3], radius [B,V] -> dict of [B,V,...] arrays."""
    b_, v_ = np.asarray(pose).shape[:2]
    outs = [[render_view(stack[6 * b:6 * b + 6], planes, k, pose[b][v], tgt_pos[b][v], radius[b][v], size, seamless)
             for v in range(v_)] for b in range(b_)]
    return {key: np.stack([np.stack([o[key] for o in row]) for row in outs]) for key in outs[0][0]}
