"""GPU checks of the cube-map viewer: MSI.cube_render_views (msi_cube_render_views: V views of a cube of six PP face stacks per
launch, equirect and pinhole cameras, fp32 / rgba8 / rgba16f stacks), MSI.equirect_to_cube and MSI.infer_cube.

The reference is tests/cube_reference.py: fp64 numpy written from the conventions, calling nothing of the package
(tests/test_cube_cpu.py checks it by itself).  Inputs: cubes of uniformly random colours in [-1,1] and alphas in (0,1);
S = 16, D = 4 with planes [100, 10, 3, 1] and S = 12, D = 3 with planes [50, 5, 1]; B = 2 cubes, V = 3 views each: the identity
at the centre and two general rotations with a translation and a non-zero tgt_pos, all inside the unit cube (the innermost
shell); stack camera fx = cx = S/2 (the harness's PP intrinsics), so the rays between tan = 1 - 2/S and 1 clamp to the edge.
Outputs: equirect 32 x 64, equirect 33 x 70 (a partial 64-pixel block, an odd row count, a row group of one row), pinhole
24 x 40.  One full-size cube, S = 256, D = 32 -> 320 x 640, V = 2, runs the real grid and the XCD mapping.

Gate against the reference: max-abs <= 1e-3 on rgb and depth (the project's render gate against its oracle; values in [-1,1],
plane fraction in [0,1]), over the pixels whose reference edge margin is >= 1e-4 -- the face choice is discontinuous on the
cube's edges -- and the test asserts that at most 1 % of each view's pixels are excluded and that each case has clamped taps."""
import functools

import numpy as np
import pytest

from tests import cube_reference as ref

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
    """Everything a case shares, computed once: inputs and the reference's outputs (read-only)."""
    big = s == 256
    stack = _cube(s, d, 1 if big else B)
    pose, pos = _poses(2 if big else V)
    if big:
        pose, pos = pose[:1], pos[:1]
        planes = [float(p) for p in 1.0 / np.linspace(1.0 / 100.0, 1.0, d)]
    else:
        planes = STACKS[(s, d)]
    k, kt = _k_stack(s), (_k_target(size) if camera == "pinhole" else None)
    out = ref.render_views(stack, planes, k, pose, pos, camera, size, kt)
    for a in list(out.values()) + [pose, pos]:
        a.setflags(write=False)
    return dict(stack=stack, pose=pose, pos=pos, planes=planes, k=k, kt=kt, camera=camera, size=size, **out)


def _render(torch, m, c, layers=None, **kw):
    args = dict(planes=c["planes"], stack_intrinsics=c["k"], camera=c["camera"], intrinsics=c["kt"], size=c["size"])
    args.update(kw)
    pose, pos = args.pop("pose", c["pose"]), args.pop("pos", c["pos"])
    return m.cube_render_views(_dev(torch, c["stack"]) if layers is None else layers, pose, pos, **args)


# ------------------------------------------------------------------------------------------------ preconditions (CPU side)
@pytest.mark.parametrize("s,d,camera,size", CASES)
def test_the_cases_mean_something(s, d, camera, size):
    """At most 1 % of each view's pixels lie within the edge margin, and every case reaches clamped taps."""
    c = _case(s, d, camera, size)
    excluded = (c["margin"] < EDGE).mean(axis=(2, 3))
    clamped = c["clamped"].mean(axis=(2, 3))
    print("cube %dx%dx%d -> %s %s: excluded %s clamped %s" % (s, s, d, camera, size, np.round(excluded, 4), np.round(clamped, 3)))
    assert (excluded <= 0.01).all(), excluded
    assert (clamped > 0).all(), clamped
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
    print("cube_render_views vs fp64 reference %s: rgb %.3e depth %.3e (excluded %.4f, clamped %.3f of the pixels)"
          % (what, e_rgb, e_dep, excluded.max(), c["clamped"].mean()))
    assert (excluded <= 0.01).all(), excluded
    assert c["clamped"].mean() > 0
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


# --------------------------------------------------------------- 2. a view from the centre through a face IS that face's MPI
@gpu_test
@pytest.mark.parametrize("s,d", sorted(STACKS))
def test_centre_views_are_the_faces_own_mpi_renders(gpu, s, d):
    from matryodshka_amd import cubemap
    torch, m = gpu
    stack, planes, k = _cube(s, d), STACKS[(s, d)], _k_stack(s)
    x = _dev(torch, stack)
    pose = np.tile(np.stack([cubemap.face_view_pose(f) for f in range(6)])[None], (B, 1, 1, 1))
    rgb, dep = m.cube_render_views(x, pose, np.zeros((B, 6, 3), F), planes, k, camera="pinhole",
                                   intrinsics=cubemap.face_view_intrinsics(k), size=(s, s))
    eye = np.tile(np.eye(4, dtype=F), (B, 1, 1, 1))
    worst = 0.0
    for f in range(6):
        want_rgb, want_dep = m.mpi_render_views(x[f::6], eye, planes, k)          # identity pose: the face's own texels
        e = max(float((rgb[:, f, 1:, 1:] - want_rgb[:, 0, 1:, 1:]).abs().max()), float((dep[:, f, 1:, 1:] - want_dep[:, 0, 1:, 1:]).abs().max()))
        worst = max(worst, e)
        assert e <= TOL, (f, e)
    print("centre views vs mpi_render_views of the six faces (S = %d, off the edge row and column): max %.3e" % (s, worst))


# ------------------------------------------------------------------------------------------------------ 3. bit-exactness
@gpu_test
@pytest.mark.parametrize("fmt", ["rgba8", "rgba16f"])
@pytest.mark.parametrize("s,d,camera,size", [CASES[1], CASES[5], BIG])
def test_packed_render_is_bit_identical_to_the_render_of_the_unpacked_stack(gpu, s, d, camera, size, fmt):
    torch, m = gpu
    c = _case(s, d, camera, size)
    x = _dev(torch, c["stack"])
    packed = m.pack_layers(x, fmt, c["planes"])
    unpacked = m.unpack_layers(packed)
    for want_rgb, want_depth in ((True, True), (True, False), (False, True)):
        got = _render(torch, m, c, packed, planes=None, want_rgb=want_rgb, want_depth=want_depth)     # planes: the stack's own
        want = _render(torch, m, c, unpacked, want_rgb=want_rgb, want_depth=want_depth)
        for g, w, on in zip(got, want, (want_rgb, want_depth)):
            assert (g is not None) == on and (w is not None) == on
            if on:
                assert torch.equal(g, w), (fmt, want_rgb, want_depth)
    assert not torch.equal(_render(torch, m, c, x)[0], _render(torch, m, c, packed)[0])      # (the quantised stack, not the original)
    with pytest.raises(ValueError):
        _render(torch, m, c, m.pack_layers(x, fmt), planes=None)                              # a packed stack without planes


@gpu_test
@pytest.mark.parametrize("s,d,camera,size", [CASES[1], CASES[2], CASES[3]])
def test_views_samples_outputs_and_calls_are_independent(gpu, s, d, camera, size):
    torch, m = gpu
    c = _case(s, d, camera, size)
    x = _dev(torch, c["stack"])
    rgb, dep = _render(torch, m, c, x)
    again = _render(torch, m, c, x)
    assert torch.equal(again[0], rgb) and torch.equal(again[1], dep)
    for v in range(V):                                   # a view among V = the view alone
        one = _render(torch, m, c, x, pose=c["pose"][:, v:v + 1], pos=c["pos"][:, v:v + 1])
        assert torch.equal(one[0][:, 0], rgb[:, v]) and torch.equal(one[1][:, 0], dep[:, v])
    for b in range(B):                                   # a cube among B = the cube alone ([V,4,4] / [V,3] for B = 1)
        one = _render(torch, m, c, x[6 * b:6 * b + 6], pose=c["pose"][b], pos=c["pos"][b])
        assert torch.equal(one[0][0], rgb[b]) and torch.equal(one[1][0], dep[b])
    only_rgb = _render(torch, m, c, x, want_depth=False)
    only_dep = _render(torch, m, c, x, want_rgb=False)
    assert only_rgb[1] is None and torch.equal(only_rgb[0], rgb)
    assert only_dep[0] is None and torch.equal(only_dep[1], dep)
    # a permuted view of the native stack goes through as it is; a contiguous public-layout copy gives the same bits
    copy = _render(torch, m, c, x.permute(0, 3, 1, 2, 4).contiguous().permute(0, 2, 3, 1, 4))
    assert torch.equal(copy[0], rgb) and torch.equal(copy[1], dep)


# ----------------------------------------------------------------------------------------------- 4. panorama -> six faces
@gpu_test
@pytest.mark.parametrize("shape", [(2, 16, 32, 3), (1, 15, 34, 3)])
@pytest.mark.parametrize("s", [8, 12])
def test_equirect_to_cube_matches_the_fp64_reference(gpu, shape, s):
    """Poles (v clamps) and the u-wrap column included: nothing is masked."""
    from matryodshka_amd import cubemap
    torch, m = gpu
    img = np.random.RandomState(7 + s + shape[1]).uniform(-1, 1, size=shape).astype(F)
    k = cubemap.default_face_intrinsics(s)
    got = m.equirect_to_cube(_dev(torch, img), s)
    assert tuple(got.shape) == (shape[0], 6, s, s, 3)
    want = ref.equirect_to_cube(img, s, k)
    e = np.abs(_np(got) - want).max()
    print("equirect_to_cube %s -> S = %d vs fp64 reference: %.3e" % (shape, s, e))
    assert e <= TOL
    sym = np.array([[(s - 1) / 2, 0, (s - 1) / 2], [0, (s - 1) / 2, (s - 1) / 2], [0, 0, 1]], F)      # explicit, per-sample cameras
    got = m.equirect_to_cube(_dev(torch, img), s, np.tile(sym[None], (shape[0], 1, 1)))
    assert np.abs(_np(got) - ref.equirect_to_cube(img, s, sym)).max() <= TOL
    one = m.equirect_to_cube(_dev(torch, img[..., :1]), s)                                             # C = 1
    assert torch.equal(one[..., 0], m.equirect_to_cube(_dev(torch, img), s)[..., 0])


# -------------------------------------------------------------------------------------------------------------- 5. domain
@gpu_test
def test_domain_host_guard_device_flag_and_finite_pixels(gpu):
    torch, m = gpu
    c = _case(16, 4, "equirect", (32, 64))
    x = _dev(torch, c["stack"])
    m.render_status()                                     # (start from a clear word)
    rgb, dep = _render(torch, m, c, x)
    torch.cuda.synchronize()
    assert m.render_status() == 0
    bad = c["pos"].copy()
    bad[1, 1] = [0.0, 0.0, 2.5]                           # origin = pose @ (2.5, 0, 0): outside the innermost shell (half-side 1)
    origin = c["pose"][1, 1, :3, :3].astype(np.float64) @ [2.5, 0, 0] + c["pose"][1, 1, :3, 3]
    assert np.abs(origin).max() >= 1.0 and np.isfinite(origin).all()
    with pytest.raises(ValueError):
        _render(torch, m, c, x, pos=bad)                  # host-side inputs: the guard
    assert m.render_status() == 0                         # (nothing was launched)
    rgb_b, dep_b = _render(torch, m, c, x, pos=_dev(torch, bad))      # device-side: no sync, no check at the call; the kernel flags it
    with pytest.raises(ValueError):
        m.render_status()
    assert m.render_status() == 0                         # (render_status reset the word)
    assert torch.isfinite(rgb_b).all() and torch.isfinite(dep_b).all()
    keep = torch.ones((B, V), dtype=torch.bool)
    keep[1, 1] = False
    assert torch.equal(rgb_b[keep], rgb[keep]) and torch.equal(dep_b[keep], dep[keep])
    nan = c["pos"].copy()
    nan[0, 2, 1] = np.nan
    with pytest.raises(ValueError):
        _render(torch, m, c, x, pos=nan)
    _render(torch, m, c, x, pos=_dev(torch, nan))
    with pytest.raises(ValueError):
        m.render_status()


@gpu_test
def test_argument_errors(gpu):
    torch, m = gpu
    c = _case(16, 4, "pinhole", (24, 40))
    x = _dev(torch, c["stack"])
    _render(torch, m, c, x)
    with pytest.raises(ValueError):
        _render(torch, m, c, x[:10])                      # not six faces per cube
    with pytest.raises(ValueError):
        _render(torch, m, c, x[:, :, :12])                # faces are square
    with pytest.raises(ValueError):
        _render(torch, m, c, x, size=None)
    with pytest.raises(ValueError):
        _render(torch, m, c, x, camera="equirect", size=None)
    with pytest.raises(ValueError):
        _render(torch, m, c, x, pose=c["pose"][:1])
    with pytest.raises(ValueError):
        _render(torch, m, c, x, pos=c["pos"][:, :2])
    with pytest.raises(ValueError):
        _render(torch, m, c, x, planes=c["planes"][:-1])
    with pytest.raises(ValueError):
        _render(torch, m, c, x, planes=None)              # an fp32 stack carries no planes
    with pytest.raises(ValueError):
        _render(torch, m, c, x, intrinsics=None)          # the pinhole camera needs its intrinsics
    with pytest.raises(ValueError):
        _render(torch, m, c, x, camera="fisheye")
    with pytest.raises(ValueError):
        _render(torch, m, c, x, want_rgb=False, want_depth=False)
    with pytest.raises(ValueError):
        _render(torch, m, c, x, stack_intrinsics=np.tile(c["k"][None], (3, 1, 1)))
    with pytest.raises(ValueError):
        m.infer_cube(np.zeros((1, 16, 32, 3), F), np.zeros((1, 16, 32, 3), F), np.eye(4, dtype=F), 16, c["planes"])   # an ODS model


# ---------------------------------------------------------------------------------------- 6. from a panorama pair to the viewer
@gpu_test
def test_from_a_panorama_pair_to_the_viewer(gpu):
    torch, _ = gpu
    from matryodshka_amd import MSI, PackedLayers
    from matryodshka_amd.synthetic import smooth_noise
    from oracle import nets as onets
    b, s, d, ngf = 1, 16, 4, 16
    rng = np.random.RandomState(11)
    ref_pano, src_pano = smooth_noise(rng, b, 16, 32), smooth_noise(rng, b, 16, 32)
    weights = onets.init_weights(6 * d, 2 * d, ngf=ngf, coord_net=True, seed=3, randomize_affine=True)
    m = MSI(weights=weights, coord_net=True, input_type='PP')
    planes = m.inv_depths(1.0, 100.0, d)
    src_pose = np.eye(4, dtype=F)
    src_pose[0, 3] = -0.064
    pred = m.infer_cube(torch.from_numpy(src_pano), torch.from_numpy(ref_pano), src_pose, s, planes, ngf=ngf, layer_format=('f32', 'rgba8'))
    assert tuple(pred['rgba_layers'].shape) == (6 * b, s, s, d, 4)
    assert isinstance(pred['packed_layers'], PackedLayers) and tuple(pred['packed_layers'].data.shape) == (6 * b, d, s, s, 4)
    assert pred['packed_layers'].planes == tuple(float(p) for p in planes)
    assert torch.isfinite(pred['rgba_layers']).all()
    pose, pos = _poses()
    pose, pos = pose[:1], pos[:1]
    kw = dict(camera='equirect', size=(32, 64))
    rgb, dep = m.cube_render_views(pred['rgba_layers'], pose, pos, planes, **kw)
    rgb_p, dep_p = m.cube_render_views(pred['packed_layers'], pose, pos, **kw)
    rgb_u, dep_u = m.cube_render_views(m.unpack_layers(pred['packed_layers']), pose, pos, planes, **kw)
    assert tuple(rgb.shape) == (b, V, 32, 64, 3) and tuple(dep.shape) == (b, V, 32, 64)
    for t in (rgb, dep, rgb_p, dep_p):
        assert torch.isfinite(t).all()
    assert torch.equal(rgb_p, rgb_u) and torch.equal(dep_p, dep_u)
    e_rgb, e_dep = float((rgb_p - rgb).abs().max()), float((dep_p - dep).abs().max())
    print("rgba8 cube of the PP network vs its fp32 cube through cube_render_views: rgb %.3e depth %.3e" % (e_rgb, e_dep))
    assert e_rgb <= 1 / 255 + 2 * (d - 1) / 510 and e_dep <= (d - 1) / 510 + 1e-5      # (the bounds of the MPI viewer's rgba8 test)
    scores = m.score_views(rgb_p, rgb, metrics=('psnr', 'ssim', 'mae'))
    # (the bound above is 2 of 255 levels, the 8-bit rounding of both images one more: MSE <= 9, PSNR >= 38.6 dB)
    assert tuple(scores['psnr'].shape) == (b, V) and torch.isfinite(scores['ssim']).all() and float(scores['psnr'].min()) >= 38.6
    torch.cuda.synchronize()
    assert m.render_status() == 0


# ------------------------------------------------------------------------------- 7. every kernel form at the smallest shapes
# Every instantiation of the three cube viewer kernels (mode x camera x format; clamp, seamless, sparse) at the smallest shapes that take
# every branch: output 5 x 70 (two 64-pixel blocks, the second partial; a row group of four and one of one row), B = 2, V = 2, D = 3 and
# D = 6 (an odd sparse group of two; a remainder of the seamless group of four), S = 8 dense and S = 16 sparse (whole tiles).  The forms
# are held to each other with the viewer's identities, all bit for bit: a single output is that half of the double render, a packed render
# is the render of the unpacked stack, the ODS camera with baseline 0 is the equirect camera, the seamless filter with another stack camera
# is the clamp render (and says so in the status word), a sparse render == the render of the packed stack it was made from.
SMALL_PLANES = {3: [50.0, 5.0, 1.0], 6: [100.0, 30.0, 10.0, 3.0, 1.5, 1.0]}
SMALL_SIZE = (5, 70)
MODES = [(True, True), (True, False), (False, True)]


def _small_cameras(torch, m, layers, s, planes, ks=None, **kw):
    """{camera: {mode: (rgb, depth)}} of one stack for the three cameras and the three output modes, the status word checked after each."""
    pose, pos = _poses(2)
    out = {}
    for camera, extra in (("equirect", {}), ("pinhole", dict(intrinsics=_k_target(SMALL_SIZE))), ("ods", dict(eye=[1, -1], baseline=0.06)),
                          ("ods0", dict(eye=[1, -1], baseline=0.0))):
        out[camera] = {}
        for mode in MODES:
            out[camera][mode] = m.cube_render_views(layers, pose, pos, planes=planes, stack_intrinsics=_k_stack(s) if ks is None else ks,
                                                    camera=camera.rstrip("0"), size=SMALL_SIZE, want_rgb=mode[0], want_depth=mode[1],
                                                    **extra, **kw)
            torch.cuda.synchronize()
            assert m.render_status() == (0 if ks is None or kw.get("filtering", "clamp") == "clamp" else 2), (camera, mode)
    return out


def _assert_modes_and_cameras(torch, r, what):
    for camera in r:
        rgb, dep = r[camera][(True, True)]
        assert tuple(rgb.shape) == (B, 2) + SMALL_SIZE + (3,) and tuple(dep.shape) == (B, 2) + SMALL_SIZE
        assert torch.isfinite(rgb).all() and torch.isfinite(dep).all()
        only_rgb, only_dep = r[camera][(True, False)], r[camera][(False, True)]
        assert only_rgb[1] is None and torch.equal(only_rgb[0], rgb), (what, camera)
        assert only_dep[0] is None and torch.equal(only_dep[1], dep), (what, camera)
    assert all(torch.equal(a, b) for a, b in zip(r["ods0"][(True, True)], r["equirect"][(True, True)])), what
    assert not torch.equal(r["ods"][(True, True)][0], r["equirect"][(True, True)][0]), what        # (the baseline is in the pixels)
    assert not torch.equal(r["pinhole"][(True, True)][0], r["equirect"][(True, True)][0]), what


def _same_bits(torch, a, b):
    return all(torch.equal(a[c][mode][i], b[c][mode][i]) for c in a for mode in MODES for i in (0, 1) if a[c][mode][i] is not None)


@gpu_test
@pytest.mark.parametrize("d", sorted(SMALL_PLANES))
def test_every_dense_kernel_form_at_the_smallest_shapes(gpu, d):
    torch, m = gpu
    s, planes = 8, SMALL_PLANES[d]
    x = _dev(torch, _cube(s, d))
    other = _dev(torch, np.array([[3.5, 0, 3.5], [0, 3.5, 3.5], [0, 0, 1]], F))     # (S-1)/2, handed over on the device: not the cube camera
    m.render_status()
    for fmt in ("f32", "rgba8", "rgba16f"):
        layers = x if fmt == "f32" else m.pack_layers(x, fmt, planes)
        clamp = _small_cameras(torch, m, layers, s, planes)
        seamless = _small_cameras(torch, m, layers, s, planes, filtering="seamless")
        for r, what in ((clamp, (fmt, "clamp")), (seamless, (fmt, "seamless"))):
            _assert_modes_and_cameras(torch, r, what)
        assert not _same_bits(torch, clamp, seamless), fmt                             # (S = 8: a quarter of the rays are in the strip)
        assert _same_bits(torch, _small_cameras(torch, m, layers, s, planes, ks=other, filtering="seamless"),
                          _small_cameras(torch, m, layers, s, planes, ks=other)), fmt
        if fmt != "f32":
            unpacked = m.unpack_layers(layers)
            assert _same_bits(torch, clamp, _small_cameras(torch, m, unpacked, s, planes)), fmt
            assert _same_bits(torch, seamless, _small_cameras(torch, m, unpacked, s, planes, filtering="seamless")), fmt


@gpu_test
@pytest.mark.parametrize("d", sorted(SMALL_PLANES))
def test_every_sparse_kernel_form_at_the_smallest_shapes(gpu, d):
    torch, m = gpu
    s, planes = 16, SMALL_PLANES[d]
    x = np.array(_cube(s, d))
    x[:, 8:, :, 1, 3] = 0.0                                  # layer 1 is empty in the lower half of every face ...
    x[0::2, :, :, d - 1, 3] = 0.0                            # ... and the nearest layer on the even faces: tiles to drop
    x = _dev(torch, x)
    m.render_status()
    for fmt in ("rgba8", "rgba16f"):
        packed = m.pack_layers(x, fmt, planes)
        sparse = m.sparsify_layers(packed, border="edge")
        assert 0 < sparse.occupancy < 1
        from_sparse, dense = _small_cameras(torch, m, sparse, s, None), _small_cameras(torch, m, packed, s, None)
        _assert_modes_and_cameras(torch, from_sparse, (fmt, "sparse"))
        for camera in dense:
            for mode in MODES:
                for g, w in zip(from_sparse[camera][mode], dense[camera][mode]):
                    assert (g is None) == (w is None)
                    assert g is None or bool((g == w).all()), (fmt, camera, mode)          # == : a zero may differ in sign
