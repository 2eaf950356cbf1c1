"""The fused tail emitting a compact layer stack (msi_net_plan_forward_layers; MSI.infer_layers / infer_msi with
layer_format): the packed stack the kernel writes itself must be, BIT FOR BIT, msi_pack_layers of the fp32 stack that
msi_net_plan_forward_rgba writes for the same plan and input -- fp32 and bf16 plans, one and two layer groups, rgba8 and
rgba16f -- and the fp32 outputs of a launch that writes both must be the default call's.  Every comparison is exact.

The shapes are the fused-tail tests' smallest ones: D = 4 (a layer loop shorter than its stride of 8), D = 64 and 48 (two
layer groups), b = 3 at 16 x 24 (36 pixel tiles in a grid rounded up to 40: the early-return workgroups run)."""
import numpy as np
import pytest

from tests.util import make_inputs

pytestmark = pytest.mark.gpu

FORMATS = ("rgba8", "rgba16f")
F32_SHAPES = [(True, 1, 32, 64, 32, 64), (False, 2, 16, 40, 8, 16), (True, 1, 16, 32, 64, 16), (True, 3, 16, 24, 4, 12)]
BF16_SHAPES = [(2, 32, 64, 8, 16), (1, 32, 64, 32, 32), (1, 16, 32, 48, 16), (1, 16, 32, 64, 16)]
SHAPE_B3, SHAPE_D64 = F32_SHAPES[3], F32_SHAPES[2]


@pytest.fixture(scope="module")
def env():
    import torch
    assert torch.cuda.is_available(), "GPU tests need a HIP device"
    from matryodshka_amd import MSI, _native, packed
    from oracle import nets as onets
    return torch, MSI, _native, packed, onets


_CASES = {}


def _case(env, dtype, coord, b, h, w, d, ngf, scale=1.0):
    """(model, input, the default call's outputs incl. blend weights / alphas, its native fp32 stack as numpy) -- computed
    once per shape and shared, never modified."""
    torch, MSI, N, packed, onets = env
    key = (dtype, coord, b, h, w, d, ngf, scale)
    if key not in _CASES:
        if dtype == "f32":
            weights = onets.init_weights(6 * d, 2 * d, ngf=ngf, coord_net=coord, seed=33, randomize_affine=True)
            x = torch.from_numpy(np.random.RandomState(5).uniform(-scale, scale, size=(b, h, w, 6 * d)).astype(np.float32)).cuda()
        else:
            weights = onets.init_weights(6 * d, 2 * d, ngf=ngf, coord_net=coord, seed=77, randomize_affine=True)
            x = torch.from_numpy(onets.bf16_round(np.random.RandomState(2).uniform(-scale, scale, size=(b, h, w, 6 * d))
                                                  .astype(np.float32))).cuda().bfloat16()
        m = MSI(weights=weights, coord_net=coord, dtype=dtype)
        ref = m.infer_layers(x, d, ngf, extra_outputs="blend_weights alphas")
        native = ref["rgba_layers"].permute(0, 3, 1, 2, 4).contiguous().cpu().numpy()
        _CASES[key] = (m, x, ref, native)
    return _CASES[key]


def _bits(a):
    a = np.ascontiguousarray(a)
    return a.view(np.uint16) if a.dtype == np.float16 else a


def _check_packed(env, m, pk, ref, native, fmt):
    """pk (a PackedLayers from the fused kernel) == pack_layers of the fp32 stack == the numpy rule on it."""
    torch, MSI, N, packed, onets = env
    assert isinstance(pk, packed.PackedLayers) and pk.format == fmt
    assert tuple(pk.data.shape) == native.shape and pk.shape == tuple(ref["rgba_layers"].shape[:4])
    want = m.pack_layers(ref["rgba_layers"], fmt)
    assert pk.data.dtype == want.data.dtype
    assert torch.equal(pk.data, want.data)
    assert np.array_equal(_bits(pk.data.cpu().numpy()), _bits(packed.encode_np(native, fmt)))


@pytest.mark.parametrize("fmt", FORMATS)
@pytest.mark.parametrize("coord,b,h,w,d,ngf", F32_SHAPES)
def test_fp32_plan_emits_the_bits_of_pack_layers(env, coord, b, h, w, d, ngf, fmt):
    m, x, ref, native = _case(env, "f32", coord, b, h, w, d, ngf)
    out = m.infer_layers(x, d, ngf, layer_format=fmt)
    assert "rgba_layers" not in out                      # a packed-only request has no fp32 stack
    assert out["packed_layers"].planes is None           # infer_layers has no planes to attach
    _check_packed(env, m, out["packed_layers"], ref, native, fmt)


@pytest.mark.parametrize("fmt", FORMATS)
@pytest.mark.parametrize("coord,b,h,w,d,ngf", F32_SHAPES)
def test_one_launch_writes_both_stacks_and_the_optional_outputs(env, coord, b, h, w, d, ngf, fmt):
    torch, MSI, N, packed, onets = env
    m, x, ref, native = _case(env, "f32", coord, b, h, w, d, ngf)
    out = m.infer_layers(x, d, ngf, extra_outputs="blend_weights alphas", layer_format=("f32", fmt))
    for k in ("rgba_layers", "blend_weights", "alphas"):
        assert torch.equal(out[k], ref[k]), k
    _check_packed(env, m, out["packed_layers"], ref, native, fmt)
    # through the C ABI: the optional tanh output of the packed kernel == the stand-alone network
    desc, blob, ws = m._net(b, h, w, 6 * d, 2 * d, ngf)
    plan = m._plan(b, h, w, 6 * d, 2 * d, ngf)
    rgba = torch.empty((b, d, h, w, 4), device="cuda")
    codes = torch.empty((b, d, h, w, 4), dtype=out["packed_layers"].data.dtype, device="cuda")
    p2 = torch.empty((b, h, w, 2 * d), device="cuda")
    N.check(N.lib.msi_net_plan_forward_layers(plan.handle, blob.data_ptr(), x.data_ptr(), rgba.data_ptr(), codes.data_ptr(),
                                              m.LAYER_FORMATS[fmt], 0, 0, p2.data_ptr(), ws.data_ptr(), ws.numel(), None, None),
            "forward_layers")
    assert torch.equal(p2, m.run_net(x, 2 * d, ngf))
    assert torch.equal(codes, out["packed_layers"].data)
    assert torch.equal(rgba.permute(0, 2, 3, 1, 4), ref["rgba_layers"])


@pytest.mark.parametrize("fmt", FORMATS)
@pytest.mark.parametrize("b,h,w,d,ngf", BF16_SHAPES)
def test_bf16_plan_emits_the_bits_of_pack_layers(env, b, h, w, d, ngf, fmt):
    torch, MSI, N, packed, onets = env
    m, x, ref, native = _case(env, "bf16", True, b, h, w, d, ngf)
    _check_packed(env, m, m.infer_layers(x, d, ngf, layer_format=fmt)["packed_layers"], ref, native, fmt)
    both = m.infer_layers(x, d, ngf, extra_outputs="blend_weights alphas", layer_format=(fmt, "f32"))
    for k in ("rgba_layers", "blend_weights", "alphas"):
        assert torch.equal(both[k], ref[k]), k
    _check_packed(env, m, both["packed_layers"], ref, native, fmt)


@pytest.mark.parametrize("dtype,coord,b,h,w,d,ngf", [("f32", False, 2, 16, 40, 8, 16), ("bf16", True, 2, 32, 64, 8, 16)])
def test_clamp_and_rounding_where_colours_leave_the_unit_range(env, dtype, coord, b, h, w, d, ngf):
    """Input in [-2, 2): the blended colours leave [-1, 1].  rgba8 saturates to 0 / 255 exactly where the numpy rule does;
    rgba16f does not clamp."""
    torch, MSI, N, packed, onets = env
    m, x, ref, native = _case(env, dtype, coord, b, h, w, d, ngf, scale=2.0)
    colour = native[..., :3]
    assert (colour > 1.0).any() and (colour < -1.0).any(), (colour.min(), colour.max())     # not vacuous
    q8 = m.infer_layers(x, d, ngf, layer_format="rgba8")["packed_layers"]
    _check_packed(env, m, q8, ref, native, "rgba8")
    c8 = q8.data.cpu().numpy()[..., :3]
    assert (c8[colour >= 1.0] == 255).all() and (c8[colour <= -1.0] == 0).all()
    assert np.array_equal(c8 == 255, packed.encode_np(native, "rgba8")[..., :3] == 255)
    assert np.array_equal(c8 == 0, packed.encode_np(native, "rgba8")[..., :3] == 0)
    q16 = m.infer_layers(x, d, ngf, layer_format="rgba16f")["packed_layers"]
    _check_packed(env, m, q16, ref, native, "rgba16f")
    c16 = q16.data.cpu().numpy()[..., :3].astype(np.float32)
    assert (c16 > 1.0).any() and (c16 < -1.0).any()
    assert np.array_equal(c16 > 1.0, colour.astype(np.float16).astype(np.float32) > 1.0)


@pytest.mark.parametrize("fmt", FORMATS)
@pytest.mark.parametrize("coord,b,h,w,d,ngf", [SHAPE_B3, SHAPE_D64])
def test_no_stray_writes_around_a_packed_only_output(env, coord, b, h, w, d, ngf, fmt):
    """layers_out 256 bytes into a sentinel-filled buffer, rgba_native = NULL: the bytes in front of and behind the
    B*D*H*W texels are untouched, the texels are the packed stack."""
    torch, MSI, N, packed, onets = env
    m, x, ref, native = _case(env, "f32", coord, b, h, w, d, ngf)
    n = b * d * h * w * packed.BYTES_PER_TEXEL[fmt]
    guard = 256
    buf = torch.full((guard + n + 4096,), 0xA5, dtype=torch.uint8, device="cuda")
    assert (buf.data_ptr() + guard) % 16 == 0
    desc, blob, ws = m._net(b, h, w, 6 * d, 2 * d, ngf)
    plan = m._plan(b, h, w, 6 * d, 2 * d, ngf)
    N.check(N.lib.msi_net_plan_forward_layers(plan.handle, blob.data_ptr(), x.data_ptr(), None, buf.data_ptr() + guard,
                                              m.LAYER_FORMATS[fmt], None, None, None, ws.data_ptr(), ws.numel(), None, None),
            "forward_layers")
    torch.cuda.synchronize()
    host = buf.cpu().numpy()
    assert (host[:guard] == 0xA5).all()
    assert (host[guard + n:] == 0xA5).all()
    want = np.ascontiguousarray(packed.encode_np(native, fmt)).view(np.uint8).reshape(-1)
    assert np.array_equal(host[guard:guard + n], want)


@pytest.mark.parametrize("fmt", FORMATS)
def test_repeated_calls_give_equal_bytes(env, fmt):
    torch, MSI, N, packed, onets = env
    for dtype, shape in (("f32", SHAPE_D64), ("bf16", (True,) + BF16_SHAPES[2])):
        m, x, ref, native = _case(env, dtype, *shape)
        d, ngf = shape[4], shape[5]
        first = m.infer_layers(x, d, ngf, layer_format=fmt)["packed_layers"].data
        for _ in range(2):
            assert torch.equal(m.infer_layers(x, d, ngf, layer_format=fmt)["packed_layers"].data, first)


@pytest.mark.parametrize("scheme,fuse_ln", [("blend_bg", 1), ("blend_psv", 0)])
def test_configurations_without_the_fused_tail_pack_the_assembled_stack(env, scheme, fuse_ln):
    """Other colour schemes / HEAD_FUSE_LN = 0: layer_format works through assemble_layers + pack_layers."""
    torch, MSI, N, packed, onets = env
    b, h, w, d, ngf = 1, 16, 32, 8, 16
    nout = {"blend_psv": 2 * d, "blend_bg": 2 * d + 3}[scheme]
    weights = onets.init_weights(6 * d, nout, ngf=ngf, coord_net=True, seed=41, randomize_affine=True)
    m = MSI(weights=weights, coord_net=True)
    m.net_options[N.NET_OPT_HEAD_FUSE_LN] = fuse_ln
    x = torch.from_numpy(np.random.RandomState(6).uniform(-1, 1, size=(b, h, w, 6 * d)).astype(np.float32)).cuda()
    ref = m.infer_layers(x, d, ngf, which_color_pred=scheme)
    out = m.infer_layers(x, d, ngf, which_color_pred=scheme, layer_format="rgba8")
    assert "rgba_layers" not in out
    assert torch.equal(out["packed_layers"].data, m.pack_layers(ref["rgba_layers"], "rgba8").data)
    both = m.infer_layers(x, d, ngf, which_color_pred=scheme, layer_format=("f32", "rgba8"))
    assert torch.equal(both["rgba_layers"], ref["rgba_layers"])
    assert torch.equal(both["packed_layers"].data, out["packed_layers"].data)


def test_infer_msi_to_render_views_from_the_emitted_stack(env):
    """infer_msi(layer_format='rgba8') -> render_views with the planes the stack carries == render_views of pack_layers of
    the fp32 stack, colour and depth."""
    torch, MSI, N, packed, onets = env
    b, h, w, d, ngf = 1, 16, 32, 4, 8
    inp = make_inputs(11, b, h, w)
    weights = onets.init_weights(6 * d, 2 * d, ngf=ngf, coord_net=True, seed=12, randomize_affine=True)
    m = MSI(weights=weights, coord_net=True)
    planes = m.inv_depths(1.0, 100.0, d)
    args = (torch.from_numpy(inp["src_image"]), torch.from_numpy(inp["ref_image"]), None, None, inp["ref_pose"], inp["src_pose"],
            inp["intrinsics"], "blend_psv", d, planes)
    out, _ = m.infer_msi(*args, ngf=ngf, layer_format="rgba8")
    ref, _ = m.infer_msi(*args, ngf=ngf)
    pk = out["packed_layers"]
    assert "rgba_layers" not in out and "packed_layers" not in ref
    assert pk.planes == tuple(float(p) for p in planes)
    want = m.pack_layers(ref["rgba_layers"], "rgba8", planes)
    assert torch.equal(pk.data, want.data)
    rgb, dep = m.render_views(pk, inp["tgt_pose_rt"], inp["tgt_pos"])
    rgb_w, dep_w = m.render_views(want, inp["tgt_pose_rt"], inp["tgt_pos"])
    assert torch.equal(rgb, rgb_w) and torch.equal(dep, dep_w)


def test_harness_saves_the_packed_stack_next_to_the_reference_outputs(tmp_path, env):
    torch, MSI, N, packed, onets = env
    from PIL import Image
    from matryodshka_amd import harness
    h, w, d, ngf = 16, 32, 4, 8
    img_dir = tmp_path / "images"; img_dir.mkdir()
    rng = np.random.RandomState(0)
    for name in ("000", "001", "002"):
        arr = np.clip(rng.uniform(0, 255, size=(2 * h, 2 * w, 3)), 0, 255).astype(np.uint8)
        Image.fromarray(arr).save(str(img_dir / ("room_0_pos%s.jpeg" % name)), quality=95)
    cam = tmp_path / "cams.txt"
    cam.write_text("room_0 000 001 002 0.032 0.01 -0.02 0.03\n")
    common = ["--cameras_glob", str(cam), "--image_dir", str(img_dir), "--experiment_name", "exp", "--height", str(h),
              "--width", str(w), "--num_msi_planes", str(d), "--num_psv_planes", str(d), "--ngf", str(ngf),
              "--test_outputs", "src_image_ref_image_tgt_image_psv_rgba_layers_blend_weights_alphas"]
    assert harness.main(common + ["--output_root", str(tmp_path / "out"), "--msi_format", "rgba8"]) == 1
    sample = tmp_path / "out" / "exp" / "room_0_000001002"
    pk = packed.PackedLayers.load(str(sample / "msi_room_0_000001002.npz"))
    assert pk.format == "rgba8" and pk.shape == (1, h, w, d)
    assert pk.planes == tuple(float(p) for p in MSI.inv_depths(None, 1.0, 100.0, d))
    codes = pk.data.numpy()
    dec = packed.decode_np(codes, "rgba8")
    for i in range(d):      # the PNGs truncate (utils.write_image) where the format rounds: at most one code apart
        rgb_png = np.asarray(Image.open(str(sample / ("msi_rgb_%.2d.png" % i)))).astype(np.float64)
        al_png = np.asarray(Image.open(str(sample / ("msi_alpha_%.2d.png" % i)))).astype(np.float64)
        assert np.abs(np.rint((dec[0, i, :, :, :3].astype(np.float64) + 1.0) / 2.0 * 255.0) - rgb_png).max() <= 1
        assert np.abs(np.rint(dec[0, i, :, :, 3].astype(np.float64) * 255.0) - al_png).max() <= 1
    # without the flag: the same files, no .npz
    assert harness.main(common + ["--output_root", str(tmp_path / "plain")]) == 1
    plain = tmp_path / "plain" / "exp" / "room_0_000001002"
    assert not list(plain.glob("*.npz"))
    assert sorted(p.name for p in plain.iterdir()) == sorted(p.name for p in sample.iterdir() if p.suffix != ".npz")


@pytest.mark.parametrize("bad", ["rgba4", ("rgba8", "rgba16f")])
def test_bad_layer_formats_raise(env, bad):
    torch, MSI, N, packed, onets = env
    m, x, ref, native = _case(env, "f32", *SHAPE_B3)
    with pytest.raises(ValueError) as e:
        m.infer_layers(x, SHAPE_B3[4], SHAPE_B3[5], layer_format=bad)
    assert "rgba8" in str(e.value) and "rgba16f" in str(e.value) and "f32" in str(e.value)
