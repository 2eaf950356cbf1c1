"""GPU checks of the ODS stereo camera of the cube-map viewer: MSI.cube_render_views(camera='ods') (msi_cube_render_ods_views with
the clamp and the seamless taps, msi_cube_render_ods_views_sparse) and MSI.cube_render_ods_pair.

The reference is tests/cube_ods_reference.py (fp64 numpy; tests/test_cube_ods_cpu.py holds it to the convention's facts and
asserts the exclusion cap of every case used here).  The cases are tests/cube_ods_cases.py's: S = 16, D = 5, B = 2, V = 2 with
opposite eyes and V = 3 with mixed eyes and per-view baselines, outputs 12 x 24 and 7 x 13, turned and translated heads,
baseline 0.064 against planes [50, 10, 3, 1.5, 1]; one stack with empty tiles and finite colours under zero alphas.

Gate against the reference: max-abs <= 1e-3 on rgb and depth (the project's render gate), over the pixels whose reference edge
margin is >= 1e-4, at most 1 % of each view excluded.  Measured on an MI355X, the worst of the cases: clamp rgb 8.0e-6 / depth
3.0e-6, seamless rgb 8.1e-6 / depth 2.8e-6 (at most 0.35 % of a view excluded)."""
import numpy as np
import pytest

from tests import cube_ods_cases as cases
from tests.test_gpu_cube_views import _dev, _np

pytestmark = pytest.mark.gpu
TOL = 1e-3
EDGE = 1e-4
F = np.float32
MODES = [(True, True), (True, False), (False, True)]


@pytest.fixture(scope="module")
def gpu():
    import torch
    assert torch.cuda.is_available(), "GPU tests need a HIP device"
    from matryodshka_amd import MSI
    m = MSI()
    x = _dev(torch, cases.stack())
    stacks = {"f32": x}
    for fmt in ("rgba8", "rgba16f"):
        stacks[fmt] = m.pack_layers(x, fmt, cases.PLANES)
        stacks[fmt + "_sparse"] = m.sparsify_layers(stacks[fmt], border="edge")
    return torch, m, stacks


def _status(m):
    """The raw status word since the last call, reset."""
    bits = int(m._render_status.item())
    m._render_status.zero_()
    return bits


def _render(m, c, layers, **kw):
    args = dict(planes=c["planes"], stack_intrinsics=c["k"], camera="ods", size=c["size"], filtering=c["filtering"], eye=c["eye"],
                baseline=c["baseline"])
    args.update(kw)
    pose, pos = args.pop("pose", c["pose"]), args.pop("pos", c["pos"])
    return m.cube_render_views(layers, pose, pos, **args)


def _same(torch, a, b):
    return all((x is None and y is None) or torch.equal(x, y) for x, y in zip(a, b))


# ------------------------------------------------------------------------------------- 1. e = 0 is the equirect camera
@pytest.mark.parametrize("stack", ["f32", "rgba8", "rgba16f", "rgba8_sparse", "rgba16f_sparse"])
@pytest.mark.parametrize("size", cases.SIZES)
def test_1_baseline_zero_is_the_equirect_camera_bit_for_bit(gpu, size, stack):
    torch, m, stacks = gpu
    _status(m)
    for seamless in ((False,) if stack.endswith("_sparse") else (False, True)):
        c = cases.case("mixed", size, seamless)
        for want_rgb, want_depth in MODES:
            kw = dict(want_rgb=want_rgb, want_depth=want_depth)
            got = _render(m, c, stacks[stack], baseline=0.0, **kw)
            s_got = _status(m)
            want = _render(m, c, stacks[stack], camera="equirect", eye=None, baseline=None, **kw)
            s_want = _status(m)
            assert _same(torch, got, want), (stack, seamless, want_rgb, want_depth)
            assert s_got == s_want == 0
        # ... and the status word with it: a head outside the innermost shell, handed over on the device
        bad = c["pos"].copy()
        bad[1, 1] = [0.0, 0.0, 2.5]
        got = _render(m, c, stacks[stack], pos=_dev(torch, bad), baseline=0.0)
        s_got = _status(m)
        want = _render(m, c, stacks[stack], pos=_dev(torch, bad), camera="equirect", eye=None, baseline=None)
        assert _same(torch, got, want) and s_got == _status(m) == 1


# ---------------------------------------------------------------------------------------- 2. against the fp64 reference
@pytest.mark.parametrize("views,size,seamless", cases.CASES)
def test_2_matches_the_fp64_reference(gpu, views, size, seamless):
    torch, m, stacks = gpu
    c = cases.case(views, size, seamless)
    _status(m)
    rgb, dep = _render(m, c, stacks["f32"])
    b, v = c["pose"].shape[:2]
    assert tuple(rgb.shape) == (b, v) + tuple(size) + (3,) and tuple(dep.shape) == (b, v) + tuple(size)
    keep = c["margin"] >= EDGE
    excluded = 1.0 - keep.mean(axis=(2, 3))
    e_rgb = np.abs(_np(rgb) - c["rgb"])[keep].max()
    e_dep = np.abs(_np(dep) - c["depth"])[keep].max()
    print("cube ODS vs fp64 reference %s -> %s %s: rgb %.3e depth %.3e (excluded %.4f)" % (views, size, c["filtering"], e_rgb, e_dep, excluded.max()))
    assert (excluded <= 0.01).all(), excluded
    assert e_rgb <= TOL and e_dep <= TOL, (e_rgb, e_dep)
    assert torch.isfinite(rgb).all() and torch.isfinite(dep).all()
    assert _status(m) == 0
    # the eyes differ, and differ from the mono render: the parallax is in the pixels
    mono = _render(m, c, stacks["f32"], camera="equirect", eye=None, baseline=None)[0]
    moved = c["radius"] != 0
    assert all(not torch.equal(rgb[i, j], mono[i, j]) for i, j in zip(*np.nonzero(moved)))


# ------------------------------------------------------------------------------------ 3. packed = unpacked, sparse = dense
@pytest.mark.parametrize("fmt", ["rgba8", "rgba16f"])
@pytest.mark.parametrize("views,size", [("pair", (7, 13)), ("mixed", (12, 24))])
def test_3_packed_is_unpacked_and_sparse_is_dense(gpu, views, size, fmt):
    torch, m, stacks = gpu
    packed, sparse = stacks[fmt], stacks[fmt + "_sparse"]
    assert 0 < sparse.occupancy < 1 and sparse.border == "edge"
    unpacked = m.unpack_layers(packed)
    _status(m)
    for seamless in (False, True):
        c = cases.case(views, size, seamless)
        for want_rgb, want_depth in MODES:
            kw = dict(want_rgb=want_rgb, want_depth=want_depth)
            got = _render(m, c, packed, planes=None, **kw)                    # planes: the stack's own
            assert _same(torch, got, _render(m, c, unpacked, **kw)), (fmt, seamless, want_rgb, want_depth)
            if not seamless:
                from_sparse = _render(m, c, sparse, planes=None, **kw)
                for g, w in zip(from_sparse, got):
                    assert (g is None) == (w is None)
                    assert g is None or bool((g == w).all()), (fmt, want_rgb, want_depth)          # == : a zero may differ in sign
        assert not torch.equal(_render(m, c, stacks["f32"])[0], _render(m, c, packed)[0])          # (the quantised stack, not the original)
    assert _status(m) == 0
    # the status word is the dense render's: only a part of the circle outside (test 6's inputs)
    c = cases.case(views, size, False)
    pos, radius = _partly_outside(c)
    for layers in (packed, sparse):
        rgb, dep = m.cube_render_views(layers, c["pose"], _dev(torch, pos), stack_intrinsics=c["k"], camera="ods", size=size, eye=1,
                                       baseline=_dev(torch, np.abs(radius)))
        assert _status(m) == 1 and torch.isfinite(rgb).all() and torch.isfinite(dep).all()


# --------------------------------------------------------------------------------------- 4. seamless away from the strip
@pytest.mark.parametrize("views,size", [("pair", (12, 24)), ("mixed", (7, 13))])
def test_4_seamless_away_from_the_strip_is_the_clamp_render(gpu, views, size):
    torch, m, stacks = gpu
    c = cases.case(views, size, True)
    rgb, dep = _render(m, c, stacks["f32"])
    rgb_c, dep_c = _render(m, c, stacks["f32"], filtering="clamp")
    away = torch.from_numpy(c["strip"] < -1e-3).cuda()          # every tap of the pixel has u, v <= S-1, with a margin for fp32
    inside = torch.from_numpy(c["strip"] > 0).cuda()
    assert bool(away.any()) and bool(inside.any())
    assert torch.equal(rgb[away], rgb_c[away]) and torch.equal(dep[away], dep_c[away])
    differ = (rgb != rgb_c).any(dim=-1) | (dep != dep_c)
    print("cube ODS seamless vs clamp %s -> %s: %d of the %d strip pixels differ" % (views, size, int((differ & inside).sum()), int(inside.sum())))
    assert bool((differ & inside).any())


# ------------------------------------------------------------------------------------------------------------ 5. modes
@pytest.mark.parametrize("stack", ["f32", "rgba8", "rgba16f", "rgba8_sparse", "rgba16f_sparse"])
def test_5_single_outputs_are_the_halves_of_the_double_render(gpu, stack):
    torch, m, stacks = gpu
    for seamless in ((False,) if stack.endswith("_sparse") else (False, True)):
        for views, size in (("pair", (12, 24)), ("mixed", (7, 13))):
            c = cases.case(views, size, seamless)
            rgb, dep = _render(m, c, stacks[stack])
            only_rgb = _render(m, c, stacks[stack], want_depth=False)
            only_dep = _render(m, c, stacks[stack], want_rgb=False)
            assert only_rgb[1] is None and torch.equal(only_rgb[0], rgb)
            assert only_dep[0] is None and torch.equal(only_dep[1], dep)
            # a view among V is the view alone (an eye does not depend on the other eye of the launch)
            for v in range(len(c["eye"])):
                one = _render(m, c, stacks[stack], pose=c["pose"][:, v:v + 1], pos=c["pos"][:, v:v + 1], eye=c["eye"][v:v + 1],
                              baseline=c["baseline"] if np.ndim(c["baseline"]) == 0 else c["baseline"][:, v:v + 1])
                assert torch.equal(one[0][:, 0], rgb[:, v]) and torch.equal(one[1][:, 0], dep[:, v])


# ----------------------------------------------------------------------------------------------------------- 6. status
def _partly_outside(c):
    """A head at max_k |o_k| = 0.8 (inside the innermost shell, half-side 1) with |e| = 0.35: only a part of the viewing circle is
    outside.  Returns (tgt_pos [B,V,3] with view [1, 0] moved there, radius [B,V] with that view's e = 0.35)."""
    pose = c["pose"][1, 0].astype(np.float64)
    head = np.array([0.8, 0.1, -0.2])                      # render frame, after the pose
    tp = np.linalg.solve(pose[:3, :3], head - pose[:3, 3])  # before the pose: (tgt_pos[2], tgt_pos[1], tgt_pos[0])
    pos = c["pos"].copy()
    pos[1, 0] = tp[::-1]
    radius = np.array(c["radius"])
    radius[1, 0] = 0.35
    return pos, radius


@pytest.mark.parametrize("stack", ["f32", "rgba8_sparse"])
@pytest.mark.parametrize("seamless", [False, True])
def test_6_status_word_part_of_the_circle_outside_and_nan_radius(gpu, seamless, stack):
    torch, m, stacks = gpu
    if seamless and stack.endswith("_sparse"):
        seamless = False                                    # (no seamless sparse form: the clamp form once more, from the other format)
        stack = "rgba16f_sparse"
    c = cases.case("pair", (12, 24), seamless)
    layers = stacks[stack]
    pos, radius = _partly_outside(c)
    # the fp64 origins: the head is inside, some but not all of the circle's points are outside
    from tests import cube_ods_reference as oref
    o, _, head = oref.ods_rays(c["size"], c["pose"][1, 0], pos[1, 0], 0.35)
    outside = np.abs(o).max(axis=-1) >= 1.0
    assert np.abs(head).max() < 1.0 and outside.any() and not outside.all()
    kw = dict(stack_intrinsics=c["k"], camera="ods", size=c["size"], filtering=c["filtering"], planes=c["planes"])
    with pytest.raises(ValueError):                         # host-side: the guard, before any launch
        m.cube_render_views(layers, c["pose"], pos, eye=1, baseline=np.abs(radius), **kw)
    _status(m)
    rgb, dep = m.cube_render_views(layers, c["pose"], _dev(torch, pos), eye=1, baseline=_dev(torch, np.abs(radius)), **kw)
    assert _status(m) == 1
    assert torch.isfinite(rgb).all() and torch.isfinite(dep).all()
    with pytest.raises(ValueError):                         # ... which render_status() reports
        m.cube_render_views(layers, c["pose"], _dev(torch, pos), eye=1, baseline=_dev(torch, np.abs(radius)), **kw)
        m.render_status()
    assert m.render_status() == 0
    # the same head with a small circle: nothing is flagged
    small = np.abs(radius).copy()
    small[1, 0] = 0.064
    m.cube_render_views(layers, c["pose"], pos, eye=1, baseline=small, **kw)              # (the host guard accepts it)
    ok = m.cube_render_views(layers, c["pose"], _dev(torch, pos), eye=1, baseline=_dev(torch, small), **kw)
    assert _status(m) == 0 and torch.isfinite(ok[0]).all()
    # a NaN radius on the device: flagged, finite pixels; the other views are untouched
    nan = small.copy()
    nan[0, 1] = np.nan
    rgb_n, dep_n = m.cube_render_views(layers, c["pose"], _dev(torch, pos), eye=1, baseline=_dev(torch, nan), **kw)
    assert _status(m) == 1
    assert torch.isfinite(rgb_n).all() and torch.isfinite(dep_n).all()
    keep = torch.ones((cases.B, 2), dtype=torch.bool)
    keep[0, 1] = False
    assert torch.equal(rgb_n[keep], ok[0][keep]) and torch.equal(dep_n[keep], ok[1][keep])


# ------------------------------------------------------------------------------------------------ 7. cube_render_ods_pair
@pytest.mark.parametrize("stack,filtering", [("f32", "clamp"), ("f32", "seamless"), ("rgba16f", "seamless"), ("rgba8_sparse", "clamp")])
def test_7_ods_pair_is_the_two_view_call_and_top_bottom_is_its_storage(gpu, stack, filtering):
    torch, m, stacks = gpu
    c = cases.case("pair", (7, 13), filtering == "seamless")
    layers, size = stacks[stack], c["size"]
    planes = None if stack != "f32" else c["planes"]
    pose1, pos1 = c["pose"][:, 0], c["pos"][:, 0]               # one head per cube
    pose2, pos2 = np.repeat(pose1[:, None], 2, axis=1), np.repeat(pos1[:, None], 2, axis=1)
    want = m.cube_render_views(layers, pose2, pos2, planes, camera="ods", size=size, filtering=filtering, eye=[+1, -1], baseline=cases.BASELINE)
    views, vdep = m.cube_render_ods_pair(layers, planes, cases.BASELINE, tgt_pose_rt=pose1, tgt_pos=pos1, size=size, filtering=filtering,
                                         want_depth=True)
    assert tuple(views.shape) == (cases.B, 2) + size + (3,) and tuple(vdep.shape) == (cases.B, 2) + size
    assert torch.equal(views, want[0]) and torch.equal(vdep, want[1])
    assert not torch.equal(views[:, 0], views[:, 1])
    only = m.cube_render_ods_pair(layers, planes, cases.BASELINE, tgt_pose_rt=pose1, tgt_pos=pos1, size=size, filtering=filtering)
    assert torch.is_tensor(only) and torch.equal(only, views)
    only_dep = m.cube_render_ods_pair(layers, planes, cases.BASELINE, tgt_pose_rt=pose1, tgt_pos=pos1, size=size, filtering=filtering,
                                      want_rgb=False, want_depth=True)
    assert torch.is_tensor(only_dep) and torch.equal(only_dep, vdep)
    tb, tbd = m.cube_render_ods_pair(layers, planes, cases.BASELINE, tgt_pose_rt=pose1, tgt_pos=pos1, size=size, filtering=filtering,
                                     want_depth=True, layout="top_bottom")
    assert tuple(tb.shape) == (cases.B, 2 * size[0], size[1], 3) and tuple(tbd.shape) == (cases.B, 2 * size[0], size[1])
    assert torch.equal(tb[:, :size[0]], views[:, 0]) and torch.equal(tb[:, size[0]:], views[:, 1])       # rows [0, h): the left eye
    assert torch.equal(tbd[:, :size[0]], vdep[:, 0]) and torch.equal(tbd[:, size[0]:], vdep[:, 1])
    # top_bottom is a view of the [B,2,h,w,3] tensor the launch wrote: the same storage, no copy
    assert tb.is_contiguous() and tbd.is_contiguous()
    assert tb._base is not None and tuple(tb._base.shape) == tuple(views.shape)
    assert tb.data_ptr() == tb._base.data_ptr() and tbd.data_ptr() == tbd._base.data_ptr()
    assert torch.equal(tb._base, views)
    # defaults: identity pose, head at the centre; a per-sample baseline [B]
    per = m.cube_render_ods_pair(layers, planes, np.array([cases.BASELINE, 0.0], F), size=size, filtering=filtering)
    eye4, zero = np.tile(np.eye(4, dtype=F), (cases.B, 2, 1, 1)), np.zeros((cases.B, 2, 3), F)
    ref2 = m.cube_render_views(layers, eye4, zero, planes, camera="ods", size=size, filtering=filtering, eye=[1, -1],
                               baseline=np.array([cases.BASELINE, 0.0], F), want_depth=False)[0]
    assert torch.equal(per, ref2) and torch.equal(per[1, 0], per[1, 1]) and not torch.equal(per[0, 0], per[0, 1])
    with pytest.raises(ValueError):
        m.cube_render_ods_pair(layers, planes, cases.BASELINE, size=size, layout="side_by_side")
    with pytest.raises(ValueError):
        m.cube_render_ods_pair(layers, planes, size=size)                                               # the baseline is required
    with pytest.raises(ValueError):
        m.cube_render_ods_pair(layers, planes, np.full((cases.B, 2), cases.BASELINE, F), size=size)     # a float or [B]
    with pytest.raises(ValueError):
        m.cube_render_ods_pair(layers, planes, cases.BASELINE, tgt_pos=np.zeros((3, 3), F), size=size)


# ------------------------------------------------------------------------------------------------------ 8. host errors
def test_8_host_errors(gpu):
    torch, m, stacks = gpu
    c = cases.case("pair", (12, 24), False)
    x = stacks["f32"]
    _status(m)
    with pytest.raises(TypeError, match="densify_layers"):
        _render(m, c, stacks["rgba8_sparse"], planes=None, filtering="seamless")
    wrap = m.sparsify_layers(stacks["rgba8"])                                   # border='wrap': a sphere stack
    with pytest.raises(TypeError, match="'edge'"):
        _render(m, c, wrap, planes=None)
    sym = np.array([[7.5, 0, 7.5], [0, 7.5, 7.5], [0, 0, 1]], F)
    with pytest.raises(ValueError, match="seamless"):
        _render(m, c, x, filtering="seamless", stack_intrinsics=sym)
    _render(m, c, x, stack_intrinsics=sym)                                      # (the clamp filter takes any stack camera)
    rgb, _ = _render(m, c, x, filtering="seamless", stack_intrinsics=_dev(torch, sym))         # device-side: clamp rule, flagged
    assert _status(m) == 2 and torch.equal(rgb, _render(m, c, x, stack_intrinsics=sym)[0])
    with pytest.raises(ValueError, match="baseline"):
        _render(m, c, x, baseline=None)
    with pytest.raises(ValueError, match="baseline"):
        _render(m, c, x, baseline=-0.064)
    with pytest.raises(ValueError, match="eye"):
        _render(m, c, x, eye=None)
    with pytest.raises(ValueError):
        _render(m, c, x, eye=[1, 0.5])
    with pytest.raises(ValueError):
        _render(m, c, x, eye=[1, -1, 1])                                        # [V] = [2]
    with pytest.raises(ValueError):
        _render(m, c, x, baseline=np.full((3,), 0.064, F))                      # [B] = [2]
    for camera in ("equirect", "pinhole"):
        with pytest.raises(ValueError, match="camera='ods'"):
            _render(m, c, x, camera=camera)                                     # eye and baseline belong to 'ods'
    with pytest.raises(ValueError):
        _render(m, c, x, camera="fisheye", eye=None, baseline=None)
    with pytest.raises(ValueError):
        _render(m, c, x, size=None)
    with pytest.raises(ValueError):
        _render(m, c, x, want_rgb=False, want_depth=False)
    with pytest.raises(ValueError):
        _render(m, c, x, planes=None)                                           # an fp32 stack carries no planes
    assert _status(m) == 0                                                      # (nothing of this was launched with a bad origin)
    # a string for the eye
    a = _render(m, c, x, eye=np.array([1, -1]))
    b = torch.cat([_render(m, c, x, pose=c["pose"][:, :1], pos=c["pos"][:, :1], eye="left")[0],
                   _render(m, c, x, pose=c["pose"][:, 1:], pos=c["pos"][:, 1:], eye="right")[0]], dim=1)
    assert torch.equal(a[0], b)
