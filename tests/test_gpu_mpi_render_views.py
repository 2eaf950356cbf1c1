"""GPU checks of MSI.mpi_render_views (msi_mpi_render_views): V views of each MPI per launch, any output size, rgb and the
one-channel depth, from fp32, rgba8 and rgba16f stacks.

Inputs: stacks from tests.util.random_rgba; stack camera K = [[W/2,0,W/2],[0,H/2,H/2],[0,0,1]] and a target camera of the
same form for the output size; planes inv_depths(1, 100, D) ([2.0] for D = 1); three poses per stack,
  (a) t = (-0.03, 0.01, 0)      (b) Ry(0.02), t_x = -0.03      (c) Ry(-0.15), t = (0.3, 0, 0.1)
for sample 0 and their mirror images (angles and t_x negated) for sample 1.  Each shape has a width that is not a multiple
of 64, a height that is not a multiple of 4 (the workgroup's rows) in the stack or the output, and a D that is not a multiple
of the unroll (4) except (16,64,8) -> (33,65), which runs the unrolled body alone.

The CPU oracle is composed here from oracle.geometry.inv_homography, resampler_zero_pad, over_composite and
over_composite_depth (test_the_composed_oracle_is_the_oracles_mpi_render checks that at the stack's size it IS
oracle.msi.MSI.mpi_render_view, exactly).  The same pass over the oracle's sample coordinates asserts the precondition that
makes these tests mean something (test_poses_reach_every_sampler_branch): at every small shape every pose puts >= 4 % of its
samples on the border with missing corners and one pose of each stack puts >= 5 % of a layer's samples fully outside.  The
256x256x32 case runs the bit-identity tests only (its one-texel border ring is 1.6 % of a layer whatever the pose).

Gate against the oracle: max-abs <= 1e-3 (TOL of the GPU-versus-oracle tests).  The kernel repeats the oracle's operations in
its order, so the difference should be near 0; test_matches_the_composed_oracle prints it."""
import functools

import numpy as np
import pytest

from oracle import geometry as G
from tests.util import random_rgba

gpu_test = pytest.mark.gpu       # (the two precondition tests below need no device and run with the CPU suite too)
TOL = 1e-3
F = np.float32
B, V = 2, 3

SHAPES = [((18, 40, 5), (18, 40)), ((18, 40, 5), (23, 70)), ((16, 64, 8), (33, 65)), ((12, 24, 1), (12, 24)),
          ((12, 24, 3), (7, 100))]
BIG = (256, 256, 32)


@pytest.fixture(scope="module")
def gpu():
    import torch
    assert torch.cuda.is_available(), "GPU tests need a HIP device"
    from matryodshka_amd import MSI
    return torch, MSI()


def _np(t):
    return t.detach().cpu().numpy()


def _cam(h, w):
    return np.array([[w / 2, 0, w / 2], [0, h / 2, h / 2], [0, 0, 1]], F)


def _inv(k):
    return np.linalg.inv(k.astype(np.float64)).astype(F)


def _planes(d):
    from oracle.msi import MSI as OracleMSI
    return [2.0] if d == 1 else [float(p) for p in OracleMSI(input_type='PP').inv_depths(1.0, 100.0, d)]


def _ry(th, t):
    p = np.eye(4, dtype=F)
    p[0, 0] = np.cos(th); p[0, 2] = np.sin(th); p[2, 0] = -np.sin(th); p[2, 2] = np.cos(th)
    p[:3, 3] = t
    return p


def _poses(views=V):
    """[B,views,4,4]: (a), (b), (c) for sample 0, mirrored for sample 1; views = 2 keeps (b) and (c)."""
    s0 = [_ry(0.0, (-0.03, 0.01, 0.0)), _ry(0.02, (-0.03, 0.0, 0.0)), _ry(-0.15, (0.3, 0.0, 0.1))]
    s1 = [_ry(0.0, (0.03, 0.01, 0.0)), _ry(-0.02, (0.03, 0.0, 0.0)), _ry(0.15, (-0.3, 0.0, 0.1))]
    return np.stack([np.stack(s0[-views:]), np.stack(s1[-views:])]).astype(F)


@functools.lru_cache(maxsize=None)
def _stack(h, w, d):
    x = random_rgba(1000 + h + w + d, B, h, w, d)
    x.setflags(write=False)
    return x


def _oracle_render(stack, pose, planes, k_s, k_t_inv, oh, ow):
    """(rgb [B,V,oh,ow,3], depth [B,V,oh,ow], outside [B,V,D], missing [B,V]) of the composed oracle: the fraction of each
    layer's samples outside (-1, W) x (-1, H), and of all of a view's samples that are inside with a corner off the layer."""
    b_, h, w, d, _ = stack.shape
    v_ = pose.shape[1]
    xs, ys = np.meshgrid(np.arange(ow, dtype=F), np.arange(oh, dtype=F))    # meshgrid_abs of the output size
    one = F(1)
    rgb = np.empty((b_, v_, oh, ow, 3), F); dep = np.empty((b_, v_, oh, ow), F)
    outside = np.empty((b_, v_, d)); missing = np.empty((b_, v_))
    for b in range(b_):
        for v in range(v_):
            warped, miss = [], 0
            for l in range(d):
                hm = G.inv_homography(k_s, k_t_inv, pose[b, v, :3, :3], pose[b, v, :3, 3], -F(planes[l]))
                with np.errstate(all="ignore"):
                    px = (xs * hm[0, 0] + ys * hm[0, 1]) + one * hm[0, 2]
                    py = (xs * hm[1, 0] + ys * hm[1, 1]) + one * hm[1, 2]
                    pw = (xs * hm[2, 0] + ys * hm[2, 1]) + one * hm[2, 2]
                    pw = pw + F(1e-8) * (pw == 0).astype(F)
                    x, y = (px / pw).astype(F), (py / pw).astype(F)
                warped.append(G.resampler_zero_pad(stack[b:b + 1, :, :, l, :], np.stack([x, y], axis=-1)[None]))
                inside = (x > -1) & (y > -1) & (x < w) & (y < h)
                fx, fy = np.floor(x), np.floor(y)
                outside[b, v, l] = 1.0 - inside.mean()
                miss += (inside & ((fx < 0) | (fx + 1 >= w) | (fy < 0) | (fy + 1 >= h))).sum()
            missing[b, v] = miss / float(d * oh * ow)
            rgb[b, v] = G.over_composite(warped)[0]
            dep[b, v] = G.over_composite_depth(warped)[0, ..., 0]
    return rgb, dep, outside, missing


@functools.lru_cache(maxsize=None)
def _case(idx):
    """Everything a small case shares, computed once: inputs and the oracle's outputs (read-only)."""
    (h, w, d), (oh, ow) = SHAPES[idx]
    stack, pose, planes = _stack(h, w, d), _poses(), _planes(d)
    k_s, k_t = _cam(h, w), _cam(oh, ow)
    k_t_inv = _inv(k_t)
    rgb, dep, outside, missing = _oracle_render(stack, pose, planes, k_s, k_t_inv, oh, ow)
    for a in (rgb, dep, pose):
        a.setflags(write=False)
    return dict(stack=stack, pose=pose, planes=planes, k_s=k_s, k_t=k_t, k_t_inv=k_t_inv, size=(oh, ow), rgb=rgb, dep=dep,
                outside=outside, missing=missing, d=d)


def _dev(torch, x):
    return torch.from_numpy(np.ascontiguousarray(x)).cuda()


# ---------------------------------------------------------------------------------------------- preconditions (CPU side)
@pytest.mark.parametrize("idx", range(len(SHAPES)))
def test_poses_reach_every_sampler_branch(idx):
    c = _case(idx)
    assert (c["missing"] >= 0.04).all(), c["missing"]
    assert (c["outside"].max(axis=(1, 2)) >= 0.05).all(), c["outside"].max(axis=2)


@pytest.mark.parametrize("idx", [0, 3])
def test_the_composed_oracle_is_the_oracles_mpi_render(idx):
    from oracle.msi import MSI as OracleMSI
    c = _case(idx)
    (h, w, d), (oh, ow) = SHAPES[idx]
    assert (oh, ow) == (h, w)
    o = OracleMSI(input_type='PP')
    k = np.tile(c["k_s"][None], (B, 1, 1))
    for v in range(V):
        ref = o.mpi_render_view(c["stack"], c["pose"][:, v], c["planes"], k, np.tile(c["k_t_inv"][None], (B, 1, 1)))
        assert np.array_equal(ref, c["rgb"][:, v])


# ------------------------------------------------------------------------------- 1. bit-identical to the single-view render
def _check_equals_single_view(torch, m, stack, pose, planes, k_s):
    b, h, w, d, _ = stack.shape
    k_inv = _inv(k_s)
    x = _dev(torch, stack)
    rgb, dep = m.mpi_render_views(x, pose, planes, k_s, intrinsics_inv=k_inv)
    assert tuple(rgb.shape) == (b, pose.shape[1], h, w, 3) and tuple(dep.shape) == (b, pose.shape[1], h, w)
    kb = np.tile(k_s[None], (b, 1, 1)); kib = np.tile(k_inv[None], (b, 1, 1))
    for v in range(pose.shape[1]):
        one = m.mpi_render_view(x, pose[:, v], planes, kb, kib)
        assert torch.equal(rgb[:, v], one), v


@gpu_test
@pytest.mark.parametrize("idx", [0, 3])
def test_each_view_is_bit_identical_to_mpi_render_view(gpu, idx):
    torch, m = gpu
    c = _case(idx)
    _check_equals_single_view(torch, m, c["stack"], c["pose"], c["planes"], c["k_s"])


@gpu_test
@pytest.mark.parametrize("h,w,d", [(16, 64, 8), (12, 24, 3)])
def test_each_view_is_bit_identical_to_mpi_render_view_at_the_other_stacks(gpu, h, w, d):
    torch, m = gpu
    _check_equals_single_view(torch, m, _stack(h, w, d), _poses(), _planes(d), _cam(h, w))


@gpu_test
def test_each_view_is_bit_identical_to_mpi_render_view_256(gpu):
    torch, m = gpu
    h, w, d = BIG
    _check_equals_single_view(torch, m, _stack(h, w, d), _poses(2), _planes(d), _cam(h, w))


# ------------------------------------------------------------------- 2. other sizes and the depth, against the composed oracle
@gpu_test
@pytest.mark.parametrize("idx", range(len(SHAPES)))
def test_matches_the_composed_oracle(gpu, idx):
    torch, m = gpu
    c = _case(idx)
    rgb, dep = m.mpi_render_views(_dev(torch, c["stack"]), c["pose"], c["planes"], c["k_s"], tgt_intrinsics=c["k_t"], size=c["size"])
    e_rgb, e_dep = np.abs(_np(rgb) - c["rgb"]).max(), np.abs(_np(dep) - c["dep"]).max()
    print("mpi_render_views vs oracle %s -> %s: rgb %.3e depth %.3e" % (SHAPES[idx][0], SHAPES[idx][1], e_rgb, e_dep))
    assert e_rgb <= TOL and e_dep <= TOL, (e_rgb, e_dep)
    # where every layer samples outside, rgb and depth are exact zeros on both sides
    dead = (c["rgb"] == 0).all(axis=-1) & (c["dep"] == 0)
    assert not _np(rgb)[dead].any() and not _np(dep)[dead].any()


@gpu_test
def test_tgt_intrinsics_is_inverted_in_fp64_on_the_host(gpu):
    torch, m = gpu
    c = _case(1)
    x = _dev(torch, c["stack"])
    inv = torch.linalg.inv(torch.from_numpy(c["k_t"]).double()).float()
    got = m.mpi_render_views(x, c["pose"], c["planes"], c["k_s"], tgt_intrinsics=c["k_t"], size=c["size"])
    want = m.mpi_render_views(x, c["pose"], c["planes"], c["k_s"], intrinsics_inv=inv, size=c["size"])
    assert torch.equal(got[0], want[0]) and torch.equal(got[1], want[1])
    # per-view cameras [B,V,3,3] and per-sample cameras [B,3,3] are the same cameras here
    per_view = m.mpi_render_views(x, c["pose"], c["planes"], np.tile(c["k_s"][None], (B, 1, 1)),
                                  tgt_intrinsics=np.tile(c["k_t"][None, None], (B, V, 1, 1)), size=c["size"])
    per_sample = m.mpi_render_views(x, c["pose"], c["planes"], c["k_s"], intrinsics_inv=np.tile(_np(inv)[None], (B, 1, 1)), size=c["size"])
    for other in (per_view, per_sample):
        assert torch.equal(got[0], other[0]) and torch.equal(got[1], other[1])


# ------------------------------------------------------------------------------------ 3. packed = unpacked, bit for bit
def _check_packed_equals_unpacked(torch, m, stack, pose, planes, k_s, k_t, size, fmt):
    x = _dev(torch, stack)
    packed = m.pack_layers(x, fmt, planes)
    unpacked = m.unpack_layers(packed)
    kw = dict(intrinsics=k_s, tgt_intrinsics=k_t, size=size)
    for want_rgb, want_depth in ((True, True), (True, False), (False, True)):
        got = m.mpi_render_views(packed, pose, want_rgb=want_rgb, want_depth=want_depth, **kw)        # planes=None: the stack's
        ref = m.mpi_render_views(unpacked, pose, planes, want_rgb=want_rgb, want_depth=want_depth, **kw)
        for g, r, want in zip(got, ref, (want_rgb, want_depth)):
            assert (g is not None) == want and (r is not None) == want
            if want:
                assert torch.equal(g, r), (fmt, want_rgb, want_depth)
    # (a render of the quantised stack, not of the original)
    assert not torch.equal(m.mpi_render_views(x, pose, planes, **kw)[0], m.mpi_render_views(packed, pose, **kw)[0])


@gpu_test
@pytest.mark.parametrize("fmt", ["rgba8", "rgba16f"])
@pytest.mark.parametrize("idx", [1, 4])
def test_packed_render_is_bit_identical_to_the_render_of_the_unpacked_stack(gpu, idx, fmt):
    torch, m = gpu
    c = _case(idx)
    _check_packed_equals_unpacked(torch, m, c["stack"], c["pose"], c["planes"], c["k_s"], c["k_t"], c["size"], fmt)


@gpu_test
@pytest.mark.parametrize("fmt", ["rgba8", "rgba16f"])
def test_packed_render_is_bit_identical_to_the_render_of_the_unpacked_stack_256(gpu, fmt):
    torch, m = gpu
    h, w, d = BIG
    _check_packed_equals_unpacked(torch, m, _stack(h, w, d), _poses(2), _planes(d), _cam(h, w), _cam(h, w), (h, w), fmt)


@gpu_test
def test_a_packed_stack_without_planes_needs_them(gpu):
    torch, m = gpu
    c = _case(0)
    packed = m.pack_layers(_dev(torch, c["stack"]), "rgba8")
    assert packed.planes is None
    with pytest.raises(ValueError):
        m.mpi_render_views(packed, c["pose"], intrinsics=c["k_s"])
    rgb, _ = m.mpi_render_views(packed, c["pose"], c["planes"], c["k_s"])
    with_planes = m.pack_layers(_dev(torch, c["stack"]), "rgba8", c["planes"])
    assert torch.equal(rgb, m.mpi_render_views(with_planes, c["pose"], intrinsics=c["k_s"])[0])
    # the single-view method still refuses a packed stack
    with pytest.raises(TypeError):
        m.mpi_render_view(with_planes, c["pose"][:, 0], c["planes"], np.tile(c["k_s"][None], (B, 1, 1)))


# ------------------------------------------------------------------------------------------------- 4. known answers
def _composite(stack):
    d = stack.shape[3]
    rgb = stack[..., 0, :3]
    dep = np.zeros(stack.shape[:3], F)
    for i in range(1, d):
        a = stack[..., i, 3:]
        rgb = stack[..., i, :3] * a + rgb * (1 - a)
        dep = F(i / d) * a[..., 0] + dep * (1 - a[..., 0])
    return rgb, dep


@gpu_test
def test_identity_pose_reproduces_the_over_composite(gpu):
    torch, m = gpu
    c = _case(0)
    eye = np.tile(np.eye(4, dtype=F), (B, 1, 1, 1))
    rgb, dep = m.mpi_render_views(_dev(torch, c["stack"]), eye, c["planes"], c["k_s"])        # target camera: the stack's
    exp_rgb, exp_dep = _composite(c["stack"])
    assert np.abs(_np(rgb)[:, 0] - exp_rgb).max() < 1e-5
    assert np.abs(_np(dep)[:, 0] - exp_dep).max() < 1e-5


@gpu_test
@pytest.mark.parametrize("k", [0, 2, 4])
def test_an_opaque_layer_behind_transparent_ones_shows_through(gpu, k):
    torch, m = gpu
    c = _case(0)
    d = c["d"]
    stack = c["stack"].copy()
    stack[..., k, 3] = 1.0
    stack[..., k + 1:, 3] = 0.0
    eye = np.tile(np.eye(4, dtype=F), (B, 1, 1, 1))
    rgb, dep = m.mpi_render_views(_dev(torch, stack), eye, c["planes"], c["k_s"])
    assert np.abs(_np(rgb)[:, 0] - stack[..., k, :3]).max() < 1e-5
    assert np.abs(_np(dep)[:, 0] - F(k / d)).max() < 1e-5


@gpu_test
def test_an_x_shift_brings_in_zeros_not_wrapped_texels(gpu):
    """x-translation of 0.5 at depth 1 with fx = n/2 = 8 shifts by exactly 4 px: four border columns are exact zeros in rgb and
    depth, for the fp32 stack and both packed ones."""
    torch, m = gpu
    n = 16
    stack = random_rgba(8, 1, n, n, 2).copy()
    stack[..., 3] = 1.0
    shift = np.eye(4, dtype=F)[None, None].copy(); shift[0, 0, 0, 3] = 0.5
    planes, k = [1.0, 1.0], _cam(n, n)
    x = _dev(torch, stack)
    for layers in (x, m.pack_layers(x, "rgba8"), m.pack_layers(x, "rgba16f")):
        rgb, dep = (_np(t)[0, 0] for t in m.mpi_render_views(layers, shift, planes, k))
        zero_cols = [j for j in range(n) if not rgb[:, j].any()]
        assert len(zero_cols) == 4 and (zero_cols == [0, 1, 2, 3] or zero_cols == [n - 4, n - 3, n - 2, n - 1])
        assert [j for j in range(n) if not dep[:, j].any()] == zero_cols
        keep = [j for j in range(n) if j not in zero_cols]
        assert (dep[:, keep] == 0.5).all()                  # layer 1 of 2, opaque


# ------------------------------------------------------------------------------- 5. views and samples are independent
@gpu_test
def test_views_samples_and_outputs_are_independent(gpu):
    torch, m = gpu
    c = _case(2)
    kw = dict(planes=c["planes"], intrinsics=c["k_s"], tgt_intrinsics=c["k_t"], size=c["size"])
    x = _dev(torch, c["stack"])
    rgb, dep = m.mpi_render_views(x, c["pose"], **kw)
    perm = [2, 0, 1]
    rgb_p, dep_p = m.mpi_render_views(x, c["pose"][:, perm], **kw)
    assert torch.equal(rgb_p, rgb[:, perm]) and torch.equal(dep_p, dep[:, perm])
    other = c["stack"].copy()
    other[1] = random_rgba(77, 1, *c["stack"].shape[1:4])[0]
    rgb_o, dep_o = m.mpi_render_views(_dev(torch, other), c["pose"], **kw)
    assert torch.equal(rgb_o[0], rgb[0]) and torch.equal(dep_o[0], dep[0])
    assert not torch.equal(rgb_o[1], rgb[1])
    only_rgb = m.mpi_render_views(x, c["pose"], want_depth=False, **kw)
    only_dep = m.mpi_render_views(x, c["pose"], want_rgb=False, **kw)
    assert only_rgb[1] is None and torch.equal(only_rgb[0], rgb)
    assert only_dep[0] is None and torch.equal(only_dep[1], dep)
    # B = 1 takes [V,4,4]
    one = m.mpi_render_views(x[:1], c["pose"][0], **kw)
    assert torch.equal(one[0], rgb[:1]) and torch.equal(one[1], dep[:1])


# ------------------------------------------------------------------------------------- 6. from the network to the viewer
@gpu_test
def test_from_the_pp_network_to_the_viewer(gpu, tmp_path):
    torch, _ = gpu
    from matryodshka_amd import MSI, PackedLayers
    from oracle import nets as onets
    from tests.util import pp_inputs
    b, n, d, ngf = 2, 32, 8, 16
    ref, src, K, eye, src_pose, _ = pp_inputs(5, b, n)
    weights = onets.init_weights(6 * d, 2 * d, ngf=ngf, coord_net=True, seed=3, randomize_affine=True)
    m = MSI(weights=weights, coord_net=True, input_type='PP')
    planes = m.inv_depths(1.0, 100.0, d)
    pred, _ = m.infer_msi(torch.from_numpy(src), torch.from_numpy(ref), None, None, eye, src_pose, K, "blend_psv", d, planes,
                          ngf=ngf, layer_format=('f32', 'rgba8'))
    path = str(tmp_path / "msi_face.npz")
    pred['packed_layers'].save(path)
    loaded = PackedLayers.load(path)
    assert loaded.format == 'rgba8' and loaded.planes == tuple(float(p) for p in planes)
    pose = _poses()
    rgb, dep = m.mpi_render_views(loaded, pose, intrinsics=K)
    rgb_u, dep_u = m.mpi_render_views(m.unpack_layers(pred['packed_layers']), pose, planes, K)
    assert torch.equal(rgb, rgb_u) and torch.equal(dep, dep_u)
    rgb_f, dep_f = m.mpi_render_views(pred['rgba_layers'], pose, planes, K)
    e_rgb, e_dep = float((rgb - rgb_f).abs().max()), float((dep - dep_f).abs().max())
    print("rgba8 stack of the PP network vs its fp32 stack through mpi_render_views: rgb %.3e depth %.3e" % (e_rgb, e_dep))
    assert 0 < e_rgb <= 1 / 255 + 2 * (d - 1) / 510
    assert e_dep <= (d - 1) / 510 + 1e-5
    for v in range(V):     # and the fp32 render is the single-view render of the same stack (default target camera)
        assert torch.equal(rgb_f[:, v], m.mpi_render_view(pred['rgba_layers'], pose[:, v], planes, K))


# ------------------------------------------------------------------------------------------------ 7. argument errors
@gpu_test
def test_argument_errors(gpu):
    torch, m = gpu
    c = _case(0)
    x = _dev(torch, c["stack"])
    ok = dict(planes=c["planes"], intrinsics=c["k_s"])
    m.mpi_render_views(x, c["pose"], **ok)
    with pytest.raises(ValueError):
        m.mpi_render_views(x, c["pose"], tgt_intrinsics=c["k_t"], intrinsics_inv=c["k_t_inv"], **ok)
    with pytest.raises(ValueError):
        m.mpi_render_views(x, c["pose"][:1], **ok)                              # pose batch 1, stack batch 2
    with pytest.raises(ValueError):
        m.mpi_render_views(x, c["pose"][0], **ok)                               # [V,4,4] with B = 2
    with pytest.raises(ValueError):
        m.mpi_render_views(x, c["pose"], c["planes"], np.tile(c["k_s"][None], (3, 1, 1)))          # intrinsics batch 3
    with pytest.raises(ValueError):
        m.mpi_render_views(x, c["pose"], tgt_intrinsics=np.tile(c["k_t"][None], (3, 1, 1)), **ok)  # target batch 3
    with pytest.raises(ValueError):
        m.mpi_render_views(x, c["pose"], intrinsics_inv=np.tile(c["k_t_inv"][None, None], (B, 2, 1, 1)), **ok)   # 2 cameras, 3 views
    with pytest.raises(ValueError):
        m.mpi_render_views(x, c["pose"], c["planes"][:-1], c["k_s"])
    with pytest.raises(ValueError):
        m.mpi_render_views(x, c["pose"], want_rgb=False, want_depth=False, **ok)
    with pytest.raises(ValueError):
        m.mpi_render_views(x, c["pose"], intrinsics=c["k_s"])                   # an fp32 stack carries no planes
