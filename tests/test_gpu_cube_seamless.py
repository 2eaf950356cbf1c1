"""GPU checks of the seamless filter of the cube-map viewer: MSI.cube_render_views(filtering='seamless')
(msi_cube_render_views_seamless; the rule: include/msi_hip.h, cubemap.virtual_texel).

The reference is tests/cube_seamless_reference.py: fp64 numpy with a virtual-texel table built from the cube's geometry, calling
nothing of the package (tests/test_cube_seamless_cpu.py checks it by itself).  Inputs, the ones of tests/test_gpu_cube_views.py
restated: cubes of uniformly random colours in [-1,1] and alphas in (0,1); S = 16, D = 4 with planes [100, 10, 3, 1] and S = 12,
D = 3 with planes [50, 5, 1]; B = 2 cubes, V = 3 views each (the identity at the centre, two general rotations with a translation
and a non-zero tgt_pos inside the innermost shell); the cube camera fx = fy = cx = cy = S/2.  Outputs: equirect 32 x 64, equirect
33 x 70, pinhole 24 x 40.  One full-size cube, S = 256, D = 32 -> 320 x 640, V = 2, runs the real grid.

Gate against the reference: max-abs <= 1e-3 on rgb and depth (the project's render gate) over the pixels whose reference edge
margin is >= 1e-4; at most 1 % of each view's pixels are excluded, and every case has pixels in the strip (strip > 0: a virtual
texel) and pixels that take the three-face corner rule."""
import functools

import numpy as np
import pytest

from tests import cube_reference as ref
from tests import cube_seamless_reference as sref

gpu_test = pytest.mark.gpu       # (test_the_cases_mean_something needs no device and runs with the CPU suite too)
TOL = 1e-3
EDGE = 1e-4
F = np.float32
B, V = 2, 3
STACKS = {(16, 4): [100.0, 10.0, 3.0, 1.0], (12, 3): [50.0, 5.0, 1.0]}
OUTPUTS = [("equirect", (32, 64)), ("equirect", (33, 70)), ("pinhole", (24, 40))]
CASES = [(s, d, cam, size) for (s, d) in STACKS for cam, size in OUTPUTS]
BIG = (256, 32, "equirect", (320, 640))


@pytest.fixture(scope="module")
def gpu():
    import torch
    assert torch.cuda.is_available(), "GPU tests need a HIP device"
    from matryodshka_amd import MSI
    return torch, MSI()


def _np(t):
    return t.detach().cpu().numpy()


def _dev(torch, x):
    return torch.from_numpy(np.ascontiguousarray(x)).cuda()


def _rot(ax, ang):
    ax = np.asarray(ax, np.float64) / np.linalg.norm(ax)
    k = np.array([[0, -ax[2], ax[1]], [ax[2], 0, -ax[0]], [-ax[1], ax[0], 0]])
    return np.eye(3) + np.sin(ang) * k + (1 - np.cos(ang)) * (k @ k)


def _pose(ax, ang, t):
    p = np.eye(4)
    p[:3, :3] = _rot(ax, ang)
    p[:3, 3] = t
    return p.astype(F)


def _poses(views=V):
    """([B,views,4,4], [B,views,3]): identity at the centre, then two general views; the last `views` of them."""
    s0 = [(_pose((0, 1, 0), 0.0, (0, 0, 0)), (0, 0, 0)),
          (_pose((1, 2, 3), 0.7, (0.2, -0.15, 0.25)), (0.1, 0.2, -0.15)),
          (_pose((-2, 1, 0.5), 2.4, (-0.3, 0.1, -0.2)), (-0.2, 0.05, 0.3))]
    s1 = [(_pose((0, 1, 0), 0.0, (0, 0, 0)), (0, 0, 0)),
          (_pose((3, -1, 2), -1.1, (-0.25, 0.2, 0.1)), (0.15, -0.1, 0.2)),
          (_pose((0.2, 1, -0.4), 3.0, (0.1, -0.3, 0.3)), (0.3, 0.2, -0.1))]
    pose = np.stack([np.stack([p for p, _ in s[-views:]]) for s in (s0, s1)]).astype(F)
    pos = np.array([[q for _, q in s[-views:]] for s in (s0, s1)], F)
    return pose, pos


def _k_stack(s):
    return np.array([[s / 2, 0, s / 2], [0, s / 2, s / 2], [0, 0, 1]], F)


def _k_target(size):
    h, w = size
    return np.array([[0.45 * w, 0, 0.52 * w], [0, 0.5 * w, 0.47 * h], [0, 0, 1]], F)      # ~96 degrees wide, off-centre


@functools.lru_cache(maxsize=None)
def _cube(s, d, cubes=B):
    rng = np.random.RandomState(100 + s + d)
    x = rng.uniform(-1, 1, size=(6 * cubes, s, s, d, 4)).astype(F)
    x[..., 3] = rng.uniform(0.02, 0.98, size=x.shape[:-1]).astype(F)
    x.setflags(write=False)
    return x


@functools.lru_cache(maxsize=None)
def _case(s, d, camera, size):
    """Everything a case shares, computed once: inputs and the seamless reference's outputs (read-only)."""
    big = s == 256
    stack = _cube(s, d, 1 if big else B)
    pose, pos = _poses(2 if big else V)
    if big:
        pose, pos = pose[:1], pos[:1]
        planes = [float(p) for p in 1.0 / np.linspace(1.0 / 100.0, 1.0, d)]
    else:
        planes = STACKS[(s, d)]
    k, kt = _k_stack(s), (_k_target(size) if camera == "pinhole" else None)
    out = sref.render_views(stack, planes, k, pose, pos, camera, size, kt)
    for a in list(out.values()) + [pose, pos]:
        a.setflags(write=False)
    return dict(stack=stack, pose=pose, pos=pos, planes=planes, k=k, kt=kt, camera=camera, size=size, **out)


def _render(torch, m, c, layers=None, filtering="seamless", **kw):
    args = dict(planes=c["planes"], stack_intrinsics=c["k"], camera=c["camera"], intrinsics=c["kt"], size=c["size"])
    args.update(kw)
    pose, pos = args.pop("pose", c["pose"]), args.pop("pos", c["pos"])
    return m.cube_render_views(_dev(torch, c["stack"]) if layers is None else layers, pose, pos, filtering=filtering, **args)


# ------------------------------------------------------------------------------------------------ preconditions (CPU side)
@pytest.mark.parametrize("s,d,camera,size", CASES)
def test_the_cases_mean_something(s, d, camera, size):
    """At most 1 % of each view's pixels lie within the edge margin (the same rays as the clamp viewer's cases); every case has
    pixels in the strip and pixels that take the three-face corner rule."""
    c = _case(s, d, camera, size)
    excluded = (c["margin"] < EDGE).mean(axis=(2, 3))
    print("cube %dx%dx%d -> %s %s: excluded %s, in the strip %.3f, three-face corner rule %d pixels"
          % (s, s, d, camera, size, np.round(excluded, 4), (c["strip"] > 0).mean(), c["corner"].sum()))
    assert (excluded <= 0.01).all(), excluded
    assert (c["strip"] > 0).any() and c["corner"].any()
    assert (np.abs(c["rgb"]) <= 1).all() and (c["depth"] >= 0).all() and (c["depth"] <= 1).all()


# ----------------------------------------------------------------------------------------- 1. against the fp64 reference
def _check_against_reference(torch, m, c, what):
    rgb, dep = _render(torch, m, c)
    b, v = c["pose"].shape[:2]
    assert tuple(rgb.shape) == (b, v) + tuple(c["size"]) + (3,) and tuple(dep.shape) == (b, v) + tuple(c["size"])
    keep = c["margin"] >= EDGE
    excluded = 1.0 - keep.mean(axis=(2, 3))
    e_rgb = np.abs(_np(rgb) - c["rgb"])[keep].max()
    e_dep = np.abs(_np(dep) - c["depth"])[keep].max()
    in_strip = keep & (c["strip"] > 0)
    print("seamless cube_render_views vs fp64 reference %s: rgb %.3e depth %.3e (in the strip: rgb %.3e; excluded %.4f, strip %.3f of the "
          "pixels, %d corner-rule pixels)" % (what, e_rgb, e_dep, np.abs(_np(rgb) - c["rgb"])[in_strip].max(), excluded.max(),
                                             (c["strip"] > 0).mean(), c["corner"].sum()))
    assert (excluded <= 0.01).all(), excluded
    assert (c["strip"] > 0).any() and c["corner"].any()
    assert e_rgb <= TOL and e_dep <= TOL, (e_rgb, e_dep)
    assert torch.isfinite(rgb).all() and torch.isfinite(dep).all()
    torch.cuda.synchronize()
    assert m.render_status() == 0


@gpu_test
@pytest.mark.parametrize("s,d,camera,size", CASES)
def test_matches_the_fp64_reference(gpu, s, d, camera, size):
    torch, m = gpu
    _check_against_reference(torch, m, _case(s, d, camera, size), "%dx%dx%d -> %s %s" % (s, s, d, camera, size))


@gpu_test
def test_matches_the_fp64_reference_full_size(gpu):
    torch, m = gpu
    _check_against_reference(torch, m, _case(*BIG), "256x256x32 -> equirect (320, 640)")


# ------------------------------------------------------------------------------------------- 2. seamless against clamp
@gpu_test
@pytest.mark.parametrize("s,d,camera,size", CASES)
def test_outside_the_strip_the_pixels_are_the_clamp_renders(gpu, s, d, camera, size):
    torch, m = gpu
    c = _case(s, d, camera, size)
    x = _dev(torch, c["stack"])
    rgb, dep = _render(torch, m, c, x)
    rgb_c, dep_c = _render(torch, m, c, x, filtering="clamp")
    default = _render(torch, m, c, x, filtering="clamp")
    plain = m.cube_render_views(x, c["pose"], c["pos"], c["planes"], c["k"], camera=c["camera"], intrinsics=c["kt"], size=c["size"])
    assert torch.equal(plain[0], default[0]) and torch.equal(plain[1], default[1])       # 'clamp' is the default
    away = torch.from_numpy(c["strip"] < -1e-3).cuda()
    inside = torch.from_numpy(c["strip"] > 0).cuda()
    assert bool(away.any()) and bool(inside.any())
    assert torch.equal(rgb[away], rgb_c[away]) and torch.equal(dep[away], dep_c[away])
    differ = (rgb != rgb_c).any(dim=-1) | (dep != dep_c)
    print("seamless vs clamp %dx%dx%d -> %s %s: %d of the %d strip pixels differ" % (s, s, d, camera, size, int((differ & inside).sum()), int(inside.sum())))
    assert bool((differ & inside).any())


# ------------------------------------------------------------------------------------------------------ 3. bit-exactness
@gpu_test
@pytest.mark.parametrize("fmt", ["rgba8", "rgba16f"])
@pytest.mark.parametrize("s,d,camera,size", [CASES[1], CASES[5]])
def test_packed_render_is_bit_identical_to_the_render_of_the_unpacked_stack(gpu, s, d, camera, size, fmt):
    torch, m = gpu
    c = _case(s, d, camera, size)
    x = _dev(torch, c["stack"])
    packed = m.pack_layers(x, fmt, c["planes"])
    unpacked = m.unpack_layers(packed)
    for want_rgb, want_depth in ((True, True), (True, False), (False, True)):
        got = _render(torch, m, c, packed, planes=None, want_rgb=want_rgb, want_depth=want_depth)
        want = _render(torch, m, c, unpacked, want_rgb=want_rgb, want_depth=want_depth)
        for g, w, on in zip(got, want, (want_rgb, want_depth)):
            assert (g is not None) == on and (w is not None) == on
            if on:
                assert torch.equal(g, w), (fmt, want_rgb, want_depth)
    assert not torch.equal(_render(torch, m, c, x)[0], _render(torch, m, c, packed)[0])      # (the quantised stack, not the original)
    assert not torch.equal(_render(torch, m, c, packed)[0], _render(torch, m, c, packed, filtering="clamp")[0])


# --------------------------------------------------------------- 4. a view from the centre through a face IS that face's composite
def _own_composite_f32(face_stack):
    """The kernel's composite of a face's own texels, op for op in fp32 (no contraction): [S,S,D,4] -> (rgb [S,S,3], depth [S,S])."""
    x = np.asarray(face_stack, F)
    d = x.shape[2]
    rgb, dep = x[:, :, 0, :3].copy(), np.zeros(x.shape[:2], F)
    for l in range(1, d):
        a = x[:, :, l, 3]
        om = F(1.0) - a
        rgb = x[:, :, l, :3] * a[..., None] + rgb * om[..., None]
        dep = F(float(l) / float(d)) * a + dep * om
    return rgb, dep


@gpu_test
@pytest.mark.parametrize("s,d", sorted(STACKS))
def test_centre_views_are_the_faces_own_composites(gpu, s, d):
    """With face_view_pose / face_view_intrinsics pixel (i, j) looks at texel (j, i) of the face, so the view is the face's own
    composite -- as far as fp32 lands the taps on the texels.  It does not land them exactly: u = fma(p_x, fx (1 / h), cx) carries
    the rounding of 1 / h (h = 100, 10, 3, 50, 5), so du is 0 or a few 1e-7 either side of a texel, and already the CLAMP viewer's
    centre views differ from the op-for-op fp32 composite in a last bit at 914 of 1728 (S = 12) and 1250 of 3072 (S = 16) pixels
    (measured on an MI355X; the seamless viewer: 849 and 1151, row 0 and column 0 -- the face-choice tie -- included in all four).
    What holds, and is asserted, off row 0 and column 0 as tests/test_gpu_cube_views.py has it:
      * the seamless view is within the render gate (1e-3) of the face's own fp32 composite, the last row and column included;
      * up to row and column S-2 (u, v <= S-2 + 1e-6: no tap at S) it is the clamp viewer's view bit for bit;
      * in the last row and column |u - (S-1)| <= 2^-18: three roundings of relative size 2^-24 (the ray's (j - cx) / fx, p_x, 1 / h) on
        |u - cx| <= 8 and the fma's own half ulp of 15.  A virtual texel then weighs at most 2^-18 per axis, so a shell's colour and
        alpha move by eps <= 2 * 2^-18 * 2 = 1.6e-5 (|virtual - own| <= 2), and the composite of D <= 4 shells by at most
        D (eps + 2 eps) = 1.9e-4: the bound asserted against the clamp view is 2e-4."""
    from matryodshka_amd import cubemap
    torch, m = gpu
    stack, planes, k = _cube(s, d), STACKS[(s, d)], _k_stack(s)
    x = _dev(torch, stack)
    pose = np.tile(np.stack([cubemap.face_view_pose(f) for f in range(6)])[None], (B, 1, 1, 1))
    kw = dict(camera="pinhole", intrinsics=cubemap.face_view_intrinsics(k), size=(s, s))
    rgb, dep = m.cube_render_views(x, pose, np.zeros((B, 6, 3), F), planes, k, filtering="seamless", **kw)
    rgb_c, dep_c = m.cube_render_views(x, pose, np.zeros((B, 6, 3), F), planes, k, **kw)
    rgb, dep, rgb_c, dep_c = _np(rgb), _np(dep), _np(rgb_c), _np(dep_c)
    bits = bits_c = 0
    worst = last = 0.0
    for b in range(B):
        for f in range(6):
            want_rgb, want_dep = _own_composite_f32(stack[6 * b + f])
            bits += int(((rgb[b, f] != want_rgb).any(axis=-1) | (dep[b, f] != want_dep))[1:, 1:].sum())
            bits_c += int(((rgb_c[b, f] != want_rgb).any(axis=-1) | (dep_c[b, f] != want_dep))[1:, 1:].sum())
            worst = max(worst, float(np.abs(rgb[b, f] - want_rgb)[1:, 1:].max()), float(np.abs(dep[b, f] - want_dep)[1:, 1:].max()))
    last = max(float(np.abs(rgb - rgb_c)[:, :, 1:, 1:].max()), float(np.abs(dep - dep_c)[:, :, 1:, 1:].max()))
    print("centre views vs the faces' own fp32 composites (S = %d, off row and column 0): seamless %d, clamp %d of %d pixels differ in a bit; "
          "seamless max %.3e; seamless vs clamp max %.3e" % (s, bits, bits_c, B * 6 * (s - 1) ** 2, worst, last))
    assert worst <= TOL
    assert np.array_equal(rgb[:, :, 1:s - 1, 1:s - 1], rgb_c[:, :, 1:s - 1, 1:s - 1]) and np.array_equal(dep[:, :, 1:s - 1, 1:s - 1], dep_c[:, :, 1:s - 1, 1:s - 1])
    assert last <= 2e-4


# ------------------------------------------------------------------------------------------------------- 5. continuity
@gpu_test
def test_constant_faces_are_continuous_across_the_edges(gpu):
    torch, m = gpu
    s, size = 8, (128, 256)
    stack = sref.constant_faces(s, sref.CONSTANT_COLOURS)
    want = sref.render_view(stack, [1.0], _k_stack(s).astype(np.float64), np.eye(4), (0, 0, 0), "equirect", size)
    step_ref = sref.largest_neighbour_step(want["rgb"])
    args = (_dev(torch, stack.astype(F)), np.eye(4, dtype=F)[None], np.zeros((1, 3), F), [1.0], _k_stack(s))
    rgb, _ = m.cube_render_views(*args, camera="equirect", size=size, filtering="seamless")
    rgb_c, _ = m.cube_render_views(*args, camera="equirect", size=size)
    step, step_c = sref.largest_neighbour_step(_np(rgb)[0, 0]), sref.largest_neighbour_step(_np(rgb_c)[0, 0])
    print("six constant faces, S = 8 -> 128 x 256: largest neighbour step GPU seamless %.4f, reference %.4f, GPU clamp %.4f" % (step, step_ref, step_c))
    assert step <= step_ref + 2e-3


# ------------------------------------------------------------------------------------------------------------ 6. domain
@gpu_test
def test_other_cameras_sparse_stacks_and_unknown_filters(gpu):
    torch, m = gpu
    c = _case(16, 4, "equirect", (32, 64))
    x = _dev(torch, c["stack"])
    m.render_status()                                     # (start from a clear word)
    _render(torch, m, c, x)
    _render(torch, m, c, x, stack_intrinsics=None)
    _render(torch, m, c, x, stack_intrinsics=_dev(torch, c["k"]))
    _render(torch, m, c, x, filtering="clamp")
    torch.cuda.synchronize()
    assert m.render_status() == 0                         # default cameras: nothing is flagged
    sym = np.array([[7.5, 0, 7.5], [0, 7.5, 7.5], [0, 0, 1]], F)
    with pytest.raises(ValueError):
        _render(torch, m, c, x, stack_intrinsics=sym)     # host-side: refused before the launch
    one_bad = np.stack([c["k"], sym])
    with pytest.raises(ValueError):
        _render(torch, m, c, x, stack_intrinsics=one_bad)
    assert m.render_status() == 0
    for ks in (sym, one_bad):                             # device-side: rendered with the clamp rule, flagged
        rgb, dep = _render(torch, m, c, x, stack_intrinsics=_dev(torch, ks))
        torch.cuda.synchronize()
        assert m.render_status() == 2
        assert m.render_status() == 0                     # (render_status reset the word)
        rgb_c, dep_c = _render(torch, m, c, x, stack_intrinsics=_dev(torch, ks), filtering="clamp")
        if ks is sym:
            assert torch.equal(rgb, rgb_c) and torch.equal(dep, dep_c)
        else:                                             # per sample: cube 0 has the cube camera, cube 1 has not
            assert torch.equal(rgb[1], rgb_c[1]) and torch.equal(dep[1], dep_c[1]) and not torch.equal(rgb[0], rgb_c[0])
            assert torch.equal(rgb[0], _render(torch, m, c, x)[0][0])
        assert m.render_status() == 0                     # the clamp filter flags no camera
    sparse = m.sparsify_layers(m.pack_layers(x, "rgba8", c["planes"]), border="edge")
    _render(torch, m, c, sparse, planes=None, filtering="clamp")
    with pytest.raises(TypeError, match="densify_layers"):
        _render(torch, m, c, sparse, planes=None)
    with pytest.raises(ValueError):
        _render(torch, m, c, x, filtering="wrap")
    with pytest.raises(ValueError):
        _render(torch, m, c, x, filtering=None)
    assert m.render_status() == 0
