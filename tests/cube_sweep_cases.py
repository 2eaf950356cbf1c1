"""The cases of the cube panorama-sampling tests (tests/test_cube_sweep_cpu.py checks on the CPU that they mean something;
tests/test_gpu_cube_sweep.py runs them): B = 2 cubes -- one identity source pose, one rotated and translated -- at the three shapes where the
sweep kernels take different forms.  Inputs are fp32 arrays; the fp64 reference reads the same fp32 values."""
import functools

import numpy as np

from matryodshka_amd.synthetic import smooth_noise
from tests import cube_sweep_reference as ref

F = np.float32
# name -> (face size S, planes, panorama (Hp, Wp))
SHAPES = {
    "s64_d4": (64, (100.0, 10.0, 3.0, 1.0), (32, 64)),      # S * D = 256: the fp32 sweep's whole-pixel form
    "s16_d4": (16, (100.0, 10.0, 3.0, 1.0), (24, 50)),      # S * D = 64: the bf16 volume's whole-pixel form, the fp32 sweep's generic form
    "s12_d3": (12, (100.0, 3.0, 1.0), (24, 50)),            # 64 % 3 != 0: the generic form of both
}
B = 2


def rotation(axis, degrees):
    ax = np.asarray(axis, np.float64)
    ax = ax / np.linalg.norm(ax)
    a = np.deg2rad(degrees)
    k = np.array([[0, -ax[2], ax[1]], [ax[2], 0, -ax[0]], [-ax[1], ax[0], 0]])
    return np.eye(3) + np.sin(a) * k + (1 - np.cos(a)) * (k @ k)


def source_poses():
    """[B,4,4] fp32 in the cube frame: the identity, and 28 degrees about a skew axis with a translation of up to 0.3 -- applied twice by the
    sweep, that is 56 degrees and about 0.6 of the nearest plane: every face sees past all four of its borders, and corner rays of the near
    planes turn behind the face camera (pr2 <= 0)."""
    p = np.tile(np.eye(4), (B, 1, 1))
    p[1, :3, :3] = rotation((1.0, 2.0, 0.5), 28.0)
    p[1, :3, 3] = (0.3, -0.2, 0.25)
    return p.astype(F)


def face_intrinsics(size, n):
    s = float(size)
    return np.tile(np.array([[s / 2, 0, s / 2], [0, s / 2, s / 2], [0, 0, 1]], F)[None], (n, 1, 1))


@functools.lru_cache(maxsize=None)
def case(name, seed=5):
    """dict(size, planes, pano [B,Hp,Wp,3] in [-1,1], src_pose [B,4,4], face_pose [6B,4,4], k [6B,3,3]), all fp32 and read-only."""
    size, planes, (hp, wp) = SHAPES[name]
    rng = np.random.RandomState(seed + sorted(SHAPES).index(name))
    x = dict(name=name, size=size, planes=planes, d=len(planes))
    x["pano"] = (2.0 * smooth_noise(rng, B, hp, wp, factor=4) - 1.0).astype(F)      # band-limited noise, upsampled from 1/4 size
    x["ref_pano"] = (2.0 * smooth_noise(rng, B, hp, wp, factor=4) - 1.0).astype(F)
    x["src_pose"] = source_poses()
    x["face_pose"] = ref.face_poses(x["src_pose"]).astype(F)
    x["k"] = face_intrinsics(size, 6 * B)
    for v in x.values():
        if isinstance(v, np.ndarray):
            v.setflags(write=False)
    return x


@functools.lru_cache(maxsize=None)
def reference(name):
    """The fp64 reference of a case, computed once and shared."""
    x = case(name)
    r = ref.cube_sweep(x["pano"], x["face_pose"], x["k"], x["planes"], x["size"])
    for v in r.values():
        v.setflags(write=False)
    return r
