"""MSI.render_views / render_ods_pair from a FactoredLayers (msi_render_views_factored): views of a high-res stack that is never built.
The yardstick is existing code -- render_views / render_ods_pair of materialize_layers(f)['rgba_layers'], i.e. msi_hres_layers +
msi_render_views_f32 / msi_render_ods_views -- and the comparison is elementwise ==, on rgb, depth and the status word: the factored
stack runs the builders' texel function at the four taps of the dense render in a unit compiled without contraction, so the only
licence is the sign of a zero (a layer no lane of a wavefront can see is skipped).  No tolerance appears in this file."""
import numpy as np
import pytest

from tests.util import make_inputs

pytestmark = pytest.mark.gpu

BASE = (16, 32, 40, 88, 8)           # low 16x32 -> high 40x88 (non-integer scale), D = 8


@pytest.fixture(scope="module")
def model():
    from matryodshka_amd import MSI
    return MSI()


def _case(seed, b, h, w, hh, hw, d, tile_from=None):
    """tests/test_gpu_hres_layers.py::_case: seeded uniform (0,1) blend weights / alphas, make_inputs images (or a make_inputs tile repeated
    to the sizes where band-limited noise would take the CPU seconds)."""
    rng = np.random.RandomState(seed)
    x = dict(bw=rng.uniform(0.0, 1.0, size=(b, h, w, d)).astype(np.float32),
             al=rng.uniform(0.0, 1.0, size=(b, h, w, d)).astype(np.float32), d=d)
    if tile_from is None:
        inp = make_inputs(seed + 1, b, hh, hw)
    else:
        inp = make_inputs(seed + 1, b, *tile_from)
        reps = (1, -(-hh // tile_from[0]), -(-hw // tile_from[1]), 1)
        for k in ("ref_image", "src_image"):
            inp[k] = np.ascontiguousarray(np.tile(inp[k], reps)[:, :hh, :hw])
    x.update(ref=inp["ref_image"], src=inp["src_image"], ref_pose=inp["ref_pose"], src_pose=inp["src_pose"], intr=inp["intrinsics"])
    return x


def _stacks(m, x):
    """(factors, the dense fp32 stack they stand for, planes)."""
    planes = m.inv_depths(1.0, 100.0, x["d"])
    f = m.hres_factors(x["bw"], x["al"], x["ref"], x["src"], x["ref_pose"], x["src_pose"], planes, x["intr"])
    return f, m.materialize_layers(f)["rgba_layers"], planes


def _eq(a, b):
    import torch
    return a.shape == b.shape and a.dtype == b.dtype and torch.equal(a == b, torch.ones_like(a, dtype=torch.bool))


def _both(m, call, f, dense, planes):
    """call(stack, planes) on the factors (which carry their planes) and on the dense stack -> the two results, compared with their status
    words; the model's status word is left clear."""
    out = []
    for stack, pl in ((f, None), (dense, planes)):
        m._render_status.zero_()
        res = call(stack, pl)
        out.append((res if isinstance(res, tuple) else (res,), int(m._render_status.item())))
    m._render_status.zero_()
    (got, got_status), (want, want_status) = out
    assert got_status == want_status
    assert len(got) == len(want)
    for g, w in zip(got, want):
        assert (g is None) == (w is None)
        if g is not None:
            assert _eq(g, w)
    return got, got_status


def _rot(ax, ay, t):
    cx, sx, cy, sy = np.cos(ax), np.sin(ax), np.cos(ay), np.sin(ay)
    p = np.eye(4, dtype=np.float32)
    p[:3, :3] = (np.array([[1, 0, 0], [0, cx, -sx], [0, sx, cx]]) @ np.array([[cy, 0, sy], [0, 1, 0], [-sy, 0, cy]])).astype(np.float32)
    p[:3, 3] = t
    return p


def _views(b, v):
    """[B,V,4,4] poses (view 0 the identity, the others rotated and translated) and [B,V,3] positions, all inside the innermost sphere (radius 1)."""
    pose = np.stack([np.stack([np.eye(4, dtype=np.float32) if k == 0 else _rot(0.3 * k + 0.1 * s, -0.7 * k, (0.1 * k, -0.05, 0.08 * (s + 1)))
                               for k in range(v)]) for s in range(b)])
    pos = np.stack([np.stack([np.array([0.02 * k, -0.03 * (s + 1), 0.05 * k], np.float32) for k in range(v)]) for s in range(b)])
    return pose, pos


PINHOLE_K = np.array([[30.0, 0, 21.5], [0, 28.0, 13.0], [0, 0, 1]], np.float32)       # off-centre principal point (33 x 47)


@pytest.fixture(scope="module")
def base(model):
    x = _case(700, 1, *BASE)
    return (x,) + _stacks(model, x)


def test_the_factors_are_what_hres_layers_is_built_from(model, base):
    import torch
    x, f, dense, planes = base
    assert f.shape == (1, 40, 88, 8) and f.planes == tuple(float(p) for p in planes)
    assert f.nbytes == 4 * (2 * 16 * 32 * 8 + 2 * 40 * 88 * 3 + 32 + 9)
    want = model.hres_layers(x["bw"], x["al"], x["ref"], x["src"], x["ref_pose"], x["src_pose"], planes, x["intr"], layer_format=("f32", "rgba8"))
    got = model.materialize_layers(f, ("f32", "rgba8"))
    assert torch.equal(got["rgba_layers"].contiguous().view(torch.int32), want["rgba_layers"].contiguous().view(torch.int32))
    assert torch.equal(got["packed_layers"].data, want["packed_layers"].data) and got["packed_layers"].planes == f.planes


def test_materialize_layers_reaches_the_direct_sparse_builder(model):
    import torch
    x = _case(705, 1, 16, 32, 32, 64, 8)                               # (a sparse stack needs H % 4 == 0 and W % 16 == 0)
    x["al"][:, :, 10:, 2:] = 0.0                                        # some tiles to drop
    f, dense, planes = _stacks(model, x)
    got = model.materialize_layers(f, "rgba8", sparse=True)["sparse_layers"]
    want = model.hres_layers_sparse(x["bw"], x["al"], x["ref"], x["src"], x["ref_pose"], x["src_pose"], planes, x["intr"])["sparse_layers"]
    assert got.format == want.format == "rgba8" and got.border == "wrap" and got.planes == f.planes and 0.0 < got.occupancy < 1.0
    for name in ("table", "layer_start", "pool"):
        assert torch.equal(getattr(got, name), getattr(want, name)), name
    with pytest.raises(ValueError, match="rgba8"):
        model.materialize_layers(f, "f32", sparse=True)
    with pytest.raises(ValueError, match=r"W % 16"):
        model.materialize_layers(_stacks(model, _case(706, 1, *BASE))[0], "rgba8", sparse=True)


@pytest.mark.parametrize("want_rgb,want_depth", [(True, True), (True, False), (False, True)])
def test_equirect_views_at_stack_size(model, base, want_rgb, want_depth):
    x, f, dense, planes = base
    pose, pos = _views(1, 2)
    (rgb, dep), status = _both(model, lambda s, pl: model.render_views(s, pose[0], pos[0], pl, want_rgb=want_rgb, want_depth=want_depth),
                               f, dense, planes)
    assert status == 0 and (rgb is not None) == want_rgb and (dep is not None) == want_depth
    if rgb is not None:
        assert tuple(rgb.shape) == (1, 2, 40, 88, 3) and float(rgb.max()) > float(rgb.min())
    if dep is not None:
        assert tuple(dep.shape) == (1, 2, 40, 88) and float(dep.max()) > float(dep.min())


@pytest.mark.parametrize("as_planes", ["host float64 tensor", "host float32 tensor", "strided device tensor", "list"])
def test_planes_given_as_a_tensor_that_has_to_be_moved_or_converted(model, base, as_planes):
    """Such planes become a NEW device tensor, which must live until the launch: the host-side poses allocated after it are of the
    same size class and would take its block."""
    import torch
    x, f, dense, planes = base
    pose, pos = _views(1, 2)                                            # (host-side: uploaded inside render_views)
    given = {"host float64 tensor": lambda: torch.tensor(planes, dtype=torch.float64),
             "host float32 tensor": lambda: torch.tensor(planes, dtype=torch.float32),
             "strided device tensor": lambda: torch.tensor(planes, dtype=torch.float32, device=model.device).repeat_interleave(2)[::2],
             "list": lambda: list(planes)}[as_planes]
    want = model.render_views(f, pose[0], pos[0])
    for call in (lambda pl: model.render_views(f, pose[0], pos[0], pl),
                 lambda pl: model.render_views(f, pose[0], pos[0], pl, camera='pinhole', intrinsics=PINHOLE_K, size=(33, 47)),
                 lambda pl: model.render_ods_pair(f, pl, intrinsics=x["intr"], want_depth=True)):
        got, ref = call(given()), call(None)
        assert all(_eq(g, r) for g, r in zip(got, ref))
    assert all(_eq(g, w) for g, w in zip(model.render_views(f, pose[0], pos[0], given()), want))
    torch.cuda.synchronize()
    assert model.render_status() == 0


@pytest.mark.parametrize("size", [(24, 50), (7, 130)])
def test_equirect_output_sizes(model, base, size):
    x, f, dense, planes = base
    pose, pos = _views(1, 2)
    (rgb, dep), _ = _both(model, lambda s, pl: model.render_views(s, pose[0], pos[0], pl, size=size), f, dense, planes)
    assert tuple(rgb.shape) == (1, 2) + size + (3,)


def test_pinhole_with_an_off_centre_principal_point(model, base):
    x, f, dense, planes = base
    pose, pos = _views(1, 2)
    (rgb, dep), _ = _both(model, lambda s, pl: model.render_views(s, pose[0], pos[0], pl, camera='pinhole', intrinsics=PINHOLE_K, size=(33, 47)),
                          f, dense, planes)
    assert tuple(rgb.shape) == (1, 2, 33, 47, 3) and tuple(dep.shape) == (1, 2, 33, 47)


def test_ods_pair(model, base):
    x, f, dense, planes = base
    (rgb, dep), status = _both(model, lambda s, pl: model.render_ods_pair(s, pl, intrinsics=x["intr"], want_depth=True), f, dense, planes)
    assert status == 0 and tuple(rgb.shape) == (1, 2, 40, 88, 3) and not _eq(rgb[:, 0], rgb[:, 1])
    pose, pos = _views(1, 2)
    (tb,), _ = _both(model, lambda s, pl: model.render_ods_pair(s, pl, baseline=0.05, tgt_pose_rt=pose[0, 1], tgt_pos=pos[0, 1], size=(24, 50),
                                                                 layout='top_bottom'), f, dense, planes)
    assert tuple(tb.shape) == (1, 48, 50, 3)
    # baseline 0 is the equirect camera
    zero, zdep = model.render_ods_pair(f, baseline=0.0, want_depth=True)
    eq_rgb, eq_dep = model.render_views(f, np.eye(4, dtype=np.float32)[None], np.zeros((1, 3), np.float32))
    for eye in (0, 1):
        assert _eq(zero[:, eye], eq_rgb[:, 0]) and _eq(zdep[:, eye], eq_dep[:, 0])


def test_batch_of_two_with_equal_and_unequal_source_poses(model):
    x = _case(710, 2, *BASE)
    x["src_pose"][1] = _rot(0.02, -0.03, (0.03, 0.01, -0.02))         # sample 0: both poses equal (the shared quadratic); sample 1: not
    f, dense, planes = _stacks(model, x)
    assert bool((f.ref_pose[0] == f.src_pose[0]).all()) and not bool((f.ref_pose[1] == f.src_pose[1]).all())
    pose, pos = _views(2, 3)
    _both(model, lambda s, pl: model.render_views(s, pose, pos, pl, size=(20, 70)), f, dense, planes)
    _both(model, lambda s, pl: model.render_views(s, pose, pos, pl, camera='pinhole', intrinsics=PINHOLE_K, size=(33, 47)), f, dense, planes)
    _both(model, lambda s, pl: model.render_ods_pair(s, pl, intrinsics=x["intr"], size=(12, 66)), f, dense, planes)


@pytest.mark.parametrize("d", [4, 12, 64])
def test_layer_counts(model, d):
    x = _case(720 + d, 1, 16, 32, 40, 88, d)
    f, dense, planes = _stacks(model, x)
    pose, pos = _views(1, 2)
    _both(model, lambda s, pl: model.render_views(s, pose[0], pos[0], pl, size=(10, 70)), f, dense, planes)


@pytest.mark.parametrize("low,high", [((16, 32), (16, 32)), ((16, 32), (33, 70))])
def test_resize_geometry(model, low, high):
    x = _case(730 + high[0], 1, low[0], low[1], high[0], high[1], 8)
    f, dense, planes = _stacks(model, x)
    pose, pos = _views(1, 2)
    _both(model, lambda s, pl: model.render_views(s, pose[0], pos[0], pl), f, dense, planes)
    _both(model, lambda s, pl: model.render_views(s, pose[0], pos[0], pl, camera='pinhole', intrinsics=PINHOLE_K, size=(33, 47)), f, dense, planes)


def test_alpha_blocks_of_exact_zeros_and_ones(model):
    """Low-res alpha blocks of exactly 0 and exactly 1: the zero-alpha skip is taken on some layers and wavefronts and not on others, and
    within a wavefront some lanes have a zero footprint while others do not."""
    import torch
    x = _case(740, 1, *BASE)
    al = np.zeros_like(x["al"])
    for d in range(8):
        if d % 3 != 2:                                                # (layers 2 and 5 stay empty: every wavefront skips them)
            al[:, 2 + d:10 + d, 4 + 2 * d:14 + 2 * d, d] = 1.0       # one block per layer, moving with the layer
    x["al"] = al
    f, dense, planes = _stacks(model, x)
    a = dense[0, :, :, :, 3].permute(2, 0, 1)                                       # [D,H,W]
    foot = a + a.roll(-1, 1) + a.roll(-1, 2) + a.roll((-1, -1), (1, 2))             # the 2 x 2 footprints on the torus
    assert bool((a == 1).any())
    for d in (1, 3, 4, 6, 7):
        run = foot[d, :, :64]                                                       # the first wavefront's columns of an identity view
        assert bool(((run == 0).any(dim=1) & (run != 0).any(dim=1)).any()), d     # a row with zero and non-zero footprints side by side
    assert bool((foot[2] == 0).all()) and bool((foot[5] == 0).all())
    pose, pos = _views(1, 2)
    (rgb, dep), _ = _both(model, lambda s, pl: model.render_views(s, pose[0], pos[0], pl), f, dense, planes)
    assert float(dep.max()) > 0.0
    _both(model, lambda s, pl: model.render_views(s, pose[0], pos[0], pl, camera='pinhole', intrinsics=PINHOLE_K, size=(33, 47)), f, dense, planes)
    _both(model, lambda s, pl: model.render_ods_pair(s, pl, intrinsics=x["intr"], want_depth=True), f, dense, planes)


def test_all_zero_alphas(model):
    """Nothing but layer 0 can be seen: the depth is == 0 everywhere and the colour is layer 0's."""
    import torch
    x = _case(750, 1, *BASE)
    x["al"] = np.zeros_like(x["al"])
    f, dense, planes = _stacks(model, x)
    pose, pos = _views(1, 2)
    (rgb, dep), _ = _both(model, lambda s, pl: model.render_views(s, pose[0], pos[0], pl), f, dense, planes)
    assert _eq(dep, torch.zeros_like(dep))
    only0 = dense.clone()
    only0[:, :, :, 1:] = 0.0
    want, _ = model.render_views(only0, pose[0], pos[0], planes)
    assert _eq(rgb, want)


def test_an_origin_outside_the_spheres_sets_the_same_status_word(model, base):
    """Device-side positions skip the host guard; the kernels clamp and flag.  The flag and the pixels are the dense render's."""
    import torch
    x, f, dense, planes = base
    pose, _ = _views(1, 2)
    pos = torch.tensor([[0.0, 0.0, 0.0], [0.0, 0.3, 1.5]], device=model.device)
    _, status = _both(model, lambda s, pl: model.render_views(s, pose[0], pos, pl, size=(9, 70)), f, dense, planes)
    assert status != 0


def test_every_other_entry_point_names_materialize_layers(model, base):
    x, f, dense, planes = base
    eye, pos, intr = np.eye(4, dtype=np.float32)[None], np.zeros((1, 3), np.float32), x["intr"]
    calls = [lambda: model.pack_layers(f), lambda: model.sparsify_layers(f), lambda: model.unpack_layers(f),
             lambda: model.msi_render_equirect_view(f, eye, pos, planes, intr), lambda: model.msi_render_equirect_depth(f, eye, pos, planes, intr),
             lambda: model.msi_render_equirect_view_and_depth(f, eye, pos, planes, intr),
             lambda: model.msi_render_equirect_view_single(f, eye, pos, planes, intr), lambda: model.msi_render_ods_view(f, 1, eye, pos, planes, intr),
             lambda: model.msi_render_perspective_view(f, eye, pos, planes, intr), lambda: model.mpi_render_view(f, eye, planes, PINHOLE_K[None]),
             lambda: model.mpi_render_views(f, eye, planes, intrinsics=PINHOLE_K[None]), lambda: model.cube_render_views(f, eye, pos, planes)]
    for call in calls:
        with pytest.raises(TypeError, match="materialize_layers"):
            call()
    with pytest.raises(TypeError, match="FactoredLayers"):
        model.materialize_layers(dense)


def test_hres_factors_is_for_ods_models(base):
    from matryodshka_amd import MSI
    x, f, dense, planes = base
    with pytest.raises(ValueError, match="input_type='ODS'"):
        MSI(input_type='PP').hres_factors(x["bw"], x["al"], x["ref"], x["src"], x["ref_pose"], x["src_pose"], planes, x["intr"])


def test_mid_size_two_pinhole_eyes(model):
    """Low 320 x 640 -> high 640 x 1280, D = 32 (a 419 MB fp32 stack on the dense side), two 512 x 512 eyes."""
    import torch
    x = _case(760, 1, 320, 640, 640, 1280, 32, tile_from=(40, 88))
    f, dense, planes = _stacks(model, x)
    pose, pos = _views(1, 2)
    k = np.array([[256.0, 0, 256.0], [0, 256.0, 256.0], [0, 0, 1]], np.float32)
    (rgb, dep), _ = _both(model, lambda s, pl: model.render_views(s, pose[0], pos[0], pl, camera='pinhole', intrinsics=k, size=(512, 512)),
                          f, dense, planes)
    assert tuple(rgb.shape) == (1, 2, 512, 512, 3) and float(rgb.max()) > float(rgb.min())
    del dense
    torch.cuda.empty_cache()
