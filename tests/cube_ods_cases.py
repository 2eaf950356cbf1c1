"""The cases the tests of the cube viewer's ODS camera share (tests/test_cube_ods_cpu.py holds the reference to them,
tests/test_gpu_cube_ods.py the kernels): inputs and the fp64 reference's outputs, computed once and read-only.

The shapes are the smallest at which the kernels can still go wrong: S = 16 (the smallest whole-tile face of a sparse cube), D = 5
(not a multiple of the dense kernels' 4-way unroll nor of the sparse kernel's groups of two), B = 2 cubes; V = 2 with opposite
eyes of one baseline, and V = 3 with mixed eyes and per-view baselines; outputs 12 x 24 and an odd 7 x 13 (partial 64-pixel
blocks, a partial 4-row group); turned and translated heads (the general views of tests/test_gpu_cube_views.py; V = 3 adds the
identity at the centre); baseline 0.064 against planes [50, 10, 3, 1.5, 1].
The stack has empty tiles and finite colours under zero alphas, so one stack serves the dense, packed and sparse checks: layer 0
and layer 4 are full, layer 1 is empty, layer 2 is occupied in its top three rows on even faces and its left five columns on odd
faces, layer 3 in a 3 x 3 block whose place depends on the face (none on face 5)."""
import functools

import numpy as np

from tests import cube_ods_reference as oref
from tests.test_gpu_cube_views import _k_stack, _poses

F = np.float32
S, D, B = 16, 5, 2
PLANES = [50.0, 10.0, 3.0, 1.5, 1.0]
BASELINE = 0.064
SIZES = [(12, 24), (7, 13)]
# name -> eye [V] and baseline (a float, or [B,V])
VIEWS = {"pair": (np.array([1.0, -1.0], F), BASELINE),
         "mixed": (np.array([-1.0, 1.0, 1.0], F), np.array([[0.064, 0.03, 0.1], [0.0, 0.064, 0.02]], F))}
CASES = [(views, size, seamless) for views in VIEWS for size in SIZES for seamless in (False, True)]


@functools.lru_cache(maxsize=None)
def stack():
    rng = np.random.RandomState(2016)
    n = 6 * B
    x = rng.uniform(-1, 1, size=(n, S, S, D, 4)).astype(F)
    x[..., 3] = rng.uniform(0.05, 0.95, size=x.shape[:-1]).astype(F)
    mask = np.zeros((n, S, S, D), F)
    mask[..., 0] = 1
    mask[..., 4] = 1
    mask[0::2, :3, :, 2] = 1
    mask[1::2, :, :5, 2] = 1
    for f in range(n):
        if f % 6 != 5:
            y0, x0 = (3 * f) % (S - 3), (5 * f + 7) % (S - 3)
            mask[f, y0:y0 + 3, x0:x0 + 3, 3] = 1
    x[..., 3] *= mask
    x.setflags(write=False)
    return x


def radius(views):
    """The signed eye radius e = eye * baseline of every view, [B,V] fp32 -- what the kernel is handed."""
    eye, baseline = VIEWS[views]
    return np.ascontiguousarray(np.broadcast_to(eye * np.asarray(baseline, F), (B, len(eye)))).astype(F)


@functools.lru_cache(maxsize=None)
def case(views, size, seamless):
    eye, baseline = VIEWS[views]
    pose, pos = _poses(len(eye))
    e, k = radius(views), _k_stack(S)
    out = oref.render_views(stack(), PLANES, k, pose, pos, e, size, seamless)
    for a in list(out.values()) + [pose, pos, e]:
        a.setflags(write=False)
    return dict(stack=stack(), planes=PLANES, k=k, pose=pose, pos=pos, eye=eye, baseline=baseline, radius=e, size=size,
                filtering="seamless" if seamless else "clamp", **out)
