"""MSI.hres_layers / msi_hres_layers: the high-res layer stack (fp32, rgba8, rgba16f, or fp32 + one packed format) in one
launch.  The yardstick is the three-launch path it replaces, called directly through the binding -- msi_ods_sweep_volume ->
msi_resize_bilinear_f32 of cat([blend_weights, alphas]) -> msi_assemble_rgba_scaled_f32, plus msi_pack_layers -- and the
comparison is on the raw bits: the kernel runs the same device functions in the same order in a unit compiled without
contraction, so there is no tolerance anywhere in this file except in the one test against the CPU oracle."""
import numpy as np
import pytest

from tests.util import make_inputs

pytestmark = pytest.mark.gpu

LOW = (16, 32)
BASE = (16, 32, 40, 88, 8)           # low 16x32 -> high 40x88 (non-integer scale), D = 8
CODE_DTYPE = {"rgba8": "uint8", "rgba16f": "float16"}


@pytest.fixture(scope="module")
def model():
    from matryodshka_amd import MSI
    return MSI()


def _case(seed, b, h, w, hh, hw, d, tile_from=None):
    """blend weights / alphas: seeded uniform (0,1) (no network needed); images: make_inputs at the high-res size, or -- for
    the sizes where band-limited noise would take the CPU seconds -- a make_inputs tile repeated to that size."""
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
    x.update(ref=inp["ref_image"], src=inp["src_image"], ref_pose=inp["ref_pose"], src_pose=inp["src_pose"],
             intr=inp["intrinsics"], ref_pose_inv=None)
    return x


def _bits(t):
    import torch
    t = t.contiguous()
    return t.view({4: torch.int32, 2: torch.int16, 1: torch.uint8}[t.element_size()])


def _same_bits(a, b):
    import torch
    return a.shape == b.shape and a.dtype == b.dtype and torch.equal(_bits(a), _bits(b))


def _old_stack(m, x):
    """The three launches -> native fp32 stack [B,D,Hh,Wh,4]."""
    import torch
    from matryodshka_amd import _native as N
    ref, src = m.preprocess_image(torch.from_numpy(x["ref"])), m.preprocess_image(torch.from_numpy(x["src"]))
    b, hh, hw, _ = ref.shape
    bw, al = m._f32(x["bw"]), m._f32(x["al"])
    _, h, w, d = bw.shape
    rpi = x["ref_pose_inv"]
    if rpi is None:
        rpi = torch.linalg.inv(torch.as_tensor(x["ref_pose"], dtype=torch.float32).double()).float()
    rp, sp, rpi = m._f32(x["ref_pose"]), m._f32(x["src_pose"]), m._f32(rpi)
    cur = torch.empty((2, b, 4, 4), dtype=torch.float32, device=m.device)
    s = m._stream()
    N.check(N.lib.msi_compose_pose_pair_f32(rp.data_ptr(), sp.data_ptr(), rpi.data_ptr(), cur[0].data_ptr(), cur[1].data_ptr(),
                                            b, s), "compose")
    planes = m.inv_depths(1.0, 100.0, d)
    depths, trig, intr = m._planes(planes), m._trig(hh, hw), m._f32(x["intr"])
    psv = torch.empty((b, hh, hw, 6 * d), dtype=torch.float32, device=m.device)
    N.check(N.lib.msi_ods_sweep_volume(ref.data_ptr(), src.data_ptr(), cur[0].data_ptr(), cur[1].data_ptr(), intr.data_ptr(),
                                       depths.data_ptr(), trig.data_ptr(), b, hh, hw, d, psv.data_ptr(), 0, s), "sweep")
    low = torch.cat([bw, al], dim=-1).contiguous()
    up = torch.empty((b, hh, hw, 2 * d), dtype=torch.float32, device=m.device)
    N.check(N.lib.msi_resize_bilinear_f32(low.data_ptr(), up.data_ptr(), b, h, w, 2 * d, hh, hw, s), "resize")
    rgba = torch.empty((b, d, hh, hw, 4), dtype=torch.float32, device=m.device)
    N.check(N.lib.msi_assemble_rgba_scaled_f32(psv.data_ptr(), up.data_ptr(), rgba.data_ptr(), b, hh, hw, d, s), "assemble")
    return rgba


def _old_packed(m, rgba, fmt):
    import torch
    from matryodshka_amd import _native as N
    codes = torch.empty(rgba.shape, dtype=getattr(torch, CODE_DTYPE[fmt]), device=m.device)
    N.check(N.lib.msi_pack_layers(rgba.data_ptr(), m.LAYER_FORMATS[fmt], codes.data_ptr(), rgba.numel() // 4, m._stream()), "pack")
    return codes


def _new(m, x, layer_format):
    planes = m.inv_depths(1.0, 100.0, x["d"])
    return m.hres_layers(x["bw"], x["al"], x["ref"], x["src"], x["ref_pose"], x["src_pose"], planes, x["intr"],
                         ref_pose_inv=x["ref_pose_inv"], layer_format=layer_format)


def _native(rgba_layers):
    return rgba_layers.permute(0, 3, 1, 2, 4)


def _check_all_formats(m, x):
    """fp32 + rgba8 in one launch, rgba16f alone: every stack against the three launches (+ msi_pack_layers)."""
    old = _old_stack(m, x)
    both = _new(m, x, ("f32", "rgba8"))
    assert sorted(both) == ["packed_layers", "rgba_layers"]
    assert _same_bits(_native(both["rgba_layers"]), old)
    assert both["packed_layers"].format == "rgba8" and _same_bits(both["packed_layers"].data, _old_packed(m, old, "rgba8"))
    half = _new(m, x, "rgba16f")
    assert sorted(half) == ["packed_layers"]
    assert _same_bits(half["packed_layers"].data, _old_packed(m, old, "rgba16f"))
    return old


@pytest.fixture(scope="module")
def base(model):
    x = _case(500, 1, *BASE)
    return x, _old_stack(model, x)


@pytest.mark.parametrize("layer_format", ["f32", "rgba8", "rgba16f", ("f32", "rgba8"), ("f32", "rgba16f")])
def test_base_case_has_the_bits_of_the_three_launches(model, base, layer_format):
    x, old = base
    got = _new(model, x, layer_format)
    req = (layer_format,) if isinstance(layer_format, str) else layer_format
    assert ("rgba_layers" in got) == ("f32" in req) and ("packed_layers" in got) == (len(req) > 1 or "f32" not in req)
    if "rgba_layers" in got:
        b, d, hh, hw, _ = old.shape
        assert tuple(got["rgba_layers"].shape) == (b, hh, hw, d, 4)
        assert _same_bits(_native(got["rgba_layers"]), old)
    if "packed_layers" in got:
        pk = got["packed_layers"]
        assert pk.planes == tuple(float(p) for p in model.inv_depths(1.0, 100.0, x["d"]))
        assert _same_bits(pk.data, _old_packed(model, old, pk.format))
        assert not bool((_bits(pk.data) == 0).all())


@pytest.mark.parametrize("shape", [
    (16, 32, 33, 70, 8),      # partial wave, odd rows, rows that are no multiple of 16 bytes in rgba8
    (16, 32, 40, 88, 4),      # the smallest layer count
    (16, 32, 40, 88, 12),     # not a power of two
    (16, 32, 40, 88, 64),
    (16, 32, 16, 32, 8),      # scale exactly 1
    (16, 32, 31, 63, 8),      # x2 - 1 outputs: (in - 1) / (out - 1) = 1/2 exactly
    (16, 32, 9, 20, 8),       # downscale
    (16, 32, 8, 64, 8),       # one full wave per row
    (16, 32, 12, 300, 8),     # more than one block per row, the last one partial
    (5, 7, 40, 88, 8),        # odd low-res sizes
    (1, 1, 6, 10, 4),         # one low-res texel: every tap is the same
], ids=lambda s: "x".join(str(v) for v in s))
def test_edge_shapes(model, shape):
    _check_all_formats(model, _case(600 + shape[2] + shape[4], 1, *shape))


def _rot(axis, angle, t):
    c, s = np.cos(angle), np.sin(angle)
    i, j = [(1, 2), (0, 2), (0, 1)][axis]
    m = np.eye(4, dtype=np.float64)
    m[i, i], m[i, j], m[j, i], m[j, j] = c, -s, s, c
    m[:3, 3] = t
    return m.astype(np.float32)


def test_poses_that_differ_per_frame_and_per_source(model):
    """B = 2, a translated and a rotated + translated source pose: the two sources do not share the quadratic."""
    x = _case(700, 2, *BASE)
    x["src_pose"] = np.stack([_rot(1, 0.0, (0.03, -0.01, 0.02)), _rot(1, 0.2, (-0.02, 0.015, 0.01))])
    _check_all_formats(model, x)


def test_identity_ref_pose_with_a_given_inverse(model):
    x = _case(701, 1, *BASE)
    x["ref_pose_inv"] = _rot(2, -0.1, (0.01, 0.02, -0.015))[None]
    _check_all_formats(model, x)


def test_equal_poses_share_the_quadratic(model):
    """ref_pose == src_pose (not the identity): both composed poses are equal, the kernel's shared-quadratic path runs."""
    x = _case(702, 2, *BASE)
    x["ref_pose"] = np.stack([_rot(0, 0.15, (0.01, 0.0, 0.02)), _rot(1, -0.3, (0.0, 0.02, 0.0))])
    x["src_pose"] = x["ref_pose"].copy()
    x["ref_pose_inv"] = np.tile(np.eye(4, dtype=np.float32)[None], (2, 1, 1))
    _check_all_formats(model, x)


def test_baseline_per_frame(model):
    x = _case(703, 2, *BASE)
    x["intr"] = x["intr"].copy()
    x["intr"][:, 0, 0] = (0.032, 0.05)
    x["src_pose"] = np.stack([_rot(1, 0.0, (0.02, 0.0, 0.0)), _rot(1, 0.0, (0.0, 0.0, 0.03))])
    _check_all_formats(model, x)


def test_non_temporal_fp32_stack(model):
    """An fp32 stack just over 256 MiB (1040 x 2048 x 8 x 16 B = 260 MiB): the non-temporal fp32 form, alone and next to an
    rgba16f stack that stays under the threshold."""
    import torch
    x = _case(800, 1, 16, 32, 1040, 2048, 8, tile_from=(65, 128))
    old = _old_stack(model, x)
    assert old.numel() * 4 > 256 << 20 > old.numel() * 2
    assert _same_bits(_native(_new(model, x, "f32")["rgba_layers"]), old)
    both = _new(model, x, ("f32", "rgba16f"))
    assert _same_bits(_native(both["rgba_layers"]), old)
    assert _same_bits(both["packed_layers"].data, _old_packed(model, old, "rgba16f"))
    del old, both
    torch.cuda.empty_cache()


def test_non_temporal_rgba8_stack(model):
    """An rgba8 stack just over 256 MiB (2080 x 4096 x 8 x 4 B = 260 MiB): the non-temporal packed form alone, and both
    non-temporal forms in one launch -- there the byte offsets of the fp32 stack pass 2^31."""
    import torch
    x = _case(801, 1, 16, 32, 2080, 4096, 8, tile_from=(65, 128))
    old = _old_stack(model, x)
    assert old.numel() > 256 << 20
    want = _old_packed(model, old, "rgba8")
    assert _same_bits(_new(model, x, "rgba8")["packed_layers"].data, want)
    both = _new(model, x, ("f32", "rgba8"))
    assert _same_bits(both["packed_layers"].data, want)
    assert _same_bits(_native(both["rgba_layers"]), old)
    del old, want, both
    torch.cuda.empty_cache()


def test_no_intermediates_are_allocated(model):
    """256 x 512 x 32: a packed-only request stays below the sweep volume ALONE (6 D Hh Wh floats), an fp32 request below
    stack + sweep volume -- neither the volume nor the upsampled tensor exists."""
    import torch
    d, hh, hw = 32, 256, 512
    x = _case(900, 1, 16, 32, hh, hw, d, tile_from=(64, 128))
    _new(model, x, "rgba8")                                   # (trig table, planes: cached by the model)
    sweep, stack = 6 * d * hh * hw * 4, 16 * d * hh * hw
    for fmt, bound in (("rgba8", sweep), ("f32", stack + sweep)):
        torch.cuda.synchronize()
        torch.cuda.empty_cache()
        torch.cuda.reset_peak_memory_stats()
        before = torch.cuda.memory_allocated()
        out = _new(model, x, fmt)
        torch.cuda.synchronize()
        rise = torch.cuda.max_memory_allocated() - before
        print("hres_layers(%s) at %dx%dx%d: peak rise %.1f MB (bound %.1f MB)" % (fmt, hw, hh, d, rise / 1e6, bound / 1e6))
        assert 0 < rise < bound, (fmt, rise, bound)
        del out


def test_packed_result_feeds_render_views(model, base):
    import torch
    x, old = base
    planes = model.inv_depths(1.0, 100.0, x["d"])
    b, d, hh, hw, _ = old.shape
    rng = np.random.RandomState(5)
    pose = np.stack([_rot(1, 0.0, (0, 0, 0)), _rot(1, 0.4, (0, 0, 0)), _rot(0, -0.3, (0, 0, 0))])
    pos = rng.uniform(-0.05, 0.05, size=(3, 3)).astype(np.float32)
    K = np.array([[32.0, 0, 32.0], [0, 32.0, 32.0], [0, 0, 1]], np.float32)
    for fmt in ("rgba8", "rgba16f"):
        got = _new(model, x, fmt)["packed_layers"]
        from matryodshka_amd.packed import PackedLayers
        want = PackedLayers(_old_packed(model, old, fmt), fmt, planes)
        for kw in (dict(camera="equirect"), dict(camera="pinhole", intrinsics=K, size=(64, 64))):
            rgb, dep = model.render_views(got, pose, pos, **kw)               # (planes: the ones the stack carries)
            rgb_w, dep_w = model.render_views(want, pose, pos, **kw)
            assert tuple(rgb.shape[2:4]) == ((hh, hw) if kw["camera"] == "equirect" else (64, 64))
            assert _same_bits(rgb, rgb_w) and _same_bits(dep, dep_w)
            assert float(rgb.abs().max()) > 0
    model.render_status()


def test_msi_render_equirect_hres_is_unchanged(model, base):
    x, old = base
    planes = model.inv_depths(1.0, 100.0, x["d"])
    inp = make_inputs(31, 1, *LOW)
    rgb, dep = model.msi_render_equirect_hres(x["bw"], x["al"], x["ref"], x["src"], x["ref_pose"], x["src_pose"],
                                              inp["tgt_pose_rt"], inp["tgt_pos"], planes, x["intr"])
    rgb_w, dep_w = model.msi_render_equirect_view_and_depth(old.permute(0, 2, 3, 1, 4), inp["tgt_pose_rt"], inp["tgt_pos"],
                                                            planes, x["intr"])
    assert _same_bits(rgb, rgb_w) and _same_bits(dep, dep_w)


def test_packed_result_round_trips_through_a_file(model, base, tmp_path):
    from matryodshka_amd.packed import PackedLayers
    x, _ = base
    for fmt in ("rgba8", "rgba16f"):
        pk = _new(model, x, fmt)["packed_layers"]
        path = str(tmp_path / ("hres_%s.npz" % fmt))
        pk.save(path)
        back = PackedLayers.load(path)
        assert back.format == fmt and back.planes == pk.planes and back.shape == pk.shape
        assert _same_bits(back.data, pk.data.cpu())


def test_fp32_stack_matches_the_cpu_oracle(model, base):
    """oracle.msi: sweep + align_corners resize + blend on the CPU; the suite's tolerance for these stages."""
    from oracle.msi import MSI as OracleMSI
    from tests.test_gpu_pipeline import TOL
    x, old = base
    d = x["d"]
    o = OracleMSI()
    planes = o.inv_depths(1.0, 100.0, d)
    b, _, hh, hw, _ = old.shape
    psv = o.format_network_input(o.preprocess_image(x["ref"]), o.preprocess_image(x["src"]), x["ref_pose"], x["src_pose"],
                                 planes, x["intr"])
    uw, ua = o.resize_bilinear_align_corners(x["bw"], hh, hw), o.resize_bilinear_align_corners(x["al"], hh, hw)
    fg = psv[..., :3 * d].reshape(b, hh, hw, d, 3)
    bg = psv[..., 3 * d:].reshape(b, hh, hw, d, 3)
    want = np.concatenate([uw[..., None] * fg + (np.float32(1) - uw[..., None]) * bg, ua[..., None]], axis=-1)
    got = _new(model, x, "f32")["rgba_layers"].cpu().numpy()
    assert got.shape == want.shape
    err = np.abs(got - want).max()
    print("hres_layers vs oracle: max abs error %.3g" % err)
    assert err <= TOL


def test_a_bf16_model_gives_the_same_bits(base, model):
    from matryodshka_amd import MSI
    x, old = base
    got = _new(MSI(dtype="bf16"), x, ("f32", "rgba8"))
    assert _same_bits(_native(got["rgba_layers"]), old)
    assert _same_bits(got["packed_layers"].data, _old_packed(model, old, "rgba8"))


def test_a_perspective_model_is_refused(base):
    from matryodshka_amd import MSI
    x, _ = base
    with pytest.raises(ValueError):
        _new(MSI(input_type="PP"), x, "f32")
