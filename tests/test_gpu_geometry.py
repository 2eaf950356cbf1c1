"""GPU parity of the geometry kernels (K1 sweep, K3 assemble, K4 render, K5
pre/deprocess) against the CPU oracle, through the C ABI (via the MSI class).

Tolerances: the sweep's branch masks are checked bit-exactly through the
invalid-pixel rule; float outputs within 1e-3 max-abs (north_star), observed
~1e-5; uint8 outputs equal up to +-1 LSB on <0.1% of pixels.
"""
import numpy as np
import pytest

from tests.util import make_inputs, random_rgba

pytestmark = pytest.mark.gpu

TOL = 1e-3


@pytest.fixture(scope="module")
def gpu():
    import torch
    assert torch.cuda.is_available(), "GPU tests need a HIP device"
    from matryodshka_amd import MSI
    from oracle.msi import MSI as OracleMSI
    return torch, MSI(), OracleMSI()


def _np(t):
    return t.detach().cpu().numpy()


@pytest.mark.parametrize("b,h,w,d", [(1, 32, 64, 4), (2, 40, 80, 8), (1, 64, 128, 32)])
def test_preprocess_and_sweep_matches_oracle(gpu, b, h, w, d):
    torch, m, o = gpu
    inp = make_inputs(1 + h, b, h, w)
    planes = m.inv_depths(1.0, 100.0, d)
    assert planes == o.inv_depths(1.0, 100.0, d)
    ref = m.preprocess_image(torch.from_numpy(inp["ref_image"]))
    src = m.preprocess_image(torch.from_numpy(inp["src_image"]))
    ref_o = o.preprocess_image(inp["ref_image"])
    src_o = o.preprocess_image(inp["src_image"])
    assert np.array_equal(_np(ref), ref_o)  # K5 is exact
    psv = m.format_network_input(ref, src, inp["ref_pose"], inp["src_pose"], planes, inp["intrinsics"])
    psv_o = o.format_network_input(ref_o, src_o, inp["ref_pose"], inp["src_pose"], planes, inp["intrinsics"])
    assert psv.shape == psv_o.shape == (b, h, w, 6 * d)
    err = np.abs(_np(psv) - psv_o)
    assert err.max() <= TOL, "max-abs %g" % err.max()
    # every branch (z_larger_x, disc>=0) agreed: a flipped branch samples pixel (1,1) or a
    # far-away texel and shows up as O(1) error, so a tight percentile bound pins it
    assert np.percentile(err, 99.99) < 1e-4


def test_sweep_float_input_and_nonidentity_pose(gpu):
    torch, m, o = gpu
    b, h, w, d = 1, 32, 64, 8
    inp = make_inputs(7, b, h, w, as_uint8=False)
    planes = m.inv_depths(1.0, 100.0, d)
    th = 0.05
    pose = np.array([[np.cos(th), 0, np.sin(th), 0.01], [0, 1, 0, -0.02], [-np.sin(th), 0, np.cos(th), 0.015],
                     [0, 0, 0, 1]], dtype=np.float32)[None]
    ref = m.preprocess_image(torch.from_numpy(inp["ref_image"]))
    src = m.preprocess_image(torch.from_numpy(inp["src_image"]))
    psv = m.format_network_input(ref, src, inp["ref_pose"], pose, planes, inp["intrinsics"])
    psv_o = o.format_network_input(o.preprocess_image(inp["ref_image"]), o.preprocess_image(inp["src_image"]),
                                   inp["ref_pose"], pose, planes, inp["intrinsics"])
    err = np.abs(_np(psv) - psv_o)
    # pose composition (k = 0..3, no fma), apply_pose and the quadratic up to the discriminant follow one op order on
    # both sides: no branch flips, so the bound is on the MAXIMUM (8a-7 was only percentile-tested)
    assert err.max() <= TOL, (err.max(), float((err > TOL).mean()))


def test_compose_poses_matches_matmul(gpu):
    """msi_compose_poses_f32 = the fp32 4x4 product of msi.py:1125, summed k = 0..3 without fma."""
    torch, m, o = gpu
    rng = np.random.RandomState(3)
    a = rng.uniform(-2, 2, (5, 4, 4)).astype(np.float32)
    bm = rng.uniform(-2, 2, (5, 4, 4)).astype(np.float32)
    got = _np(m._compose(torch.from_numpy(a), torch.from_numpy(bm)))
    want = np.zeros_like(a)
    for k in range(4):                                       # same order, plain fp32 mul + add
        want = (want + a[:, :, k:k + 1] * bm[:, k:k + 1, :]).astype(np.float32) if k else (a[:, :, :1] * bm[:, :1, :])
    assert np.array_equal(got, want)
    eye = np.eye(4, dtype=np.float32)[None]
    assert np.array_equal(_np(m._compose(torch.from_numpy(a[:1]), torch.from_numpy(eye))), a[:1])   # identity is exact


@pytest.mark.parametrize("b,h,w,d", [(1, 32, 64, 4), (2, 24, 96, 8), (1, 20, 50, 12)])
def test_assemble_matches_oracle(gpu, b, h, w, d):
    torch, m, o = gpu
    rng = np.random.RandomState(3)
    psv = rng.uniform(-1, 1, size=(b, h, w, 6 * d)).astype(np.float32)
    pred = np.tanh(rng.normal(size=(b, h, w, 2 * d))).astype(np.float32)
    out = m.assemble_layers(torch.from_numpy(psv).cuda(), torch.from_numpy(pred).cuda(), d,
                            extra_outputs="blend_weights_alphas_psv")
    ref = o.assemble(psv, pred, d, "blend_weights_alphas_psv")
    assert tuple(out["rgba_layers"].shape) == (b, h, w, d, 4)
    assert np.array_equal(_np(out["rgba_layers"]), ref["rgba_layers"])   # same op order: exact
    assert np.array_equal(_np(out["blend_weights"]), ref["blend_weights"])
    assert np.array_equal(_np(out["alphas"]), ref["alphas"])


@pytest.mark.parametrize("b,h,w,d", [(1, 32, 64, 4), (2, 40, 80, 8), (1, 30, 70, 5)])
def test_render_matches_oracle(gpu, b, h, w, d):
    torch, m, o = gpu
    rgba = random_rgba(11, b, h, w, d)
    inp = make_inputs(5, b, h, w)
    planes = m.inv_depths(1.0, 100.0, d)
    t_rgba = torch.from_numpy(rgba).cuda()
    rgb = m.msi_render_equirect_view(t_rgba, inp["tgt_pose_rt"], inp["tgt_pos"], planes, inp["intrinsics"])
    dep = m.msi_render_equirect_depth(t_rgba, inp["tgt_pose_rt"], inp["tgt_pos"], planes, inp["intrinsics"])
    lay = m.msi_render_equirect_view_single(t_rgba, inp["tgt_pose_rt"], inp["tgt_pos"], planes, inp["intrinsics"])
    rgb_o = o.msi_render_equirect_view(rgba, inp["tgt_pose_rt"], inp["tgt_pos"], planes, inp["intrinsics"])
    dep_o = o.msi_render_equirect_depth(rgba, inp["tgt_pose_rt"], inp["tgt_pos"], planes, inp["intrinsics"])
    lay_o = o.msi_render_equirect_view_single(rgba, inp["tgt_pose_rt"], inp["tgt_pos"], planes, inp["intrinsics"])
    assert np.abs(_np(rgb) - rgb_o).max() <= TOL
    assert np.abs(_np(dep) - dep_o).max() <= TOL
    assert np.abs(_np(lay) - lay_o).max() <= TOL
    both_rgb, both_dep = m.msi_render_equirect_view_and_depth(t_rgba, inp["tgt_pose_rt"], inp["tgt_pos"], planes,
                                                              inp["intrinsics"])
    assert torch.equal(both_rgb, rgb) and torch.equal(both_dep, dep)
    # uint8 outputs of test.py:149-159
    u8 = _np(m.deprocess_image(rgb)).astype(int)
    u8_o = o.deprocess_image(rgb_o).astype(int)
    diff = np.abs(u8 - u8_o)
    assert diff.max() <= 1 and (diff > 0).mean() < 1e-3
    d8 = _np(m.deprocess_depth_image(dep)).astype(int)
    d8_o = o.deprocess_depth_image(dep_o).astype(int)
    assert np.abs(d8 - d8_o).max() <= 1


def test_render_identity_is_mirrored_composite(gpu):
    """KAT 3: tgt_pos = 0, pose = I  =>  u = W-1-j, v = i, so the render is the
    over-composite of the horizontally mirrored layers (to bilinear round-off 6e-5 px)."""
    torch, m, o = gpu
    b, h, w, d = 1, 32, 64, 6
    rgba = random_rgba(2, b, h, w, d)
    planes = m.inv_depths(1.0, 100.0, d)
    zero = np.zeros((1, 3), np.float32)
    rgb = _np(m.msi_render_equirect_view(torch.from_numpy(rgba).cuda(), np.eye(4, dtype=np.float32)[None], zero,
                                         planes, None))
    mirrored = rgba[:, :, ::-1]
    out = mirrored[..., 0, :3]
    for i in range(1, d):
        a = mirrored[..., i, 3:]
        out = mirrored[..., i, :3] * a + out * (1 - a)
    assert np.abs(rgb - out).max() < 5e-4


def test_render_opaque_layer_kat(gpu):
    """KAT 7: alpha_k = 1 and alpha_{>k} = 0 => out = rgb_k (warped), depth = k/D;
    the farthest layer's alpha is ignored."""
    torch, m, o = gpu
    b, h, w, d, k = 1, 16, 32, 8, 3
    rgba = random_rgba(4, b, h, w, d)
    rgba[..., :, 3] = 0.0
    rgba[..., k, 3] = 1.0
    rgba[..., 0, 3] = 0.37  # ignored
    for i in range(d):
        rgba[..., i, :3] = (i + 1) / 10.0   # constant colour per layer: warp-invariant
    planes = m.inv_depths(1.0, 100.0, d)
    pos = np.array([[0.05, -0.02, 0.03]], np.float32)
    t = torch.from_numpy(rgba).cuda()
    rgb, dep = m.msi_render_equirect_view_and_depth(t, np.eye(4, dtype=np.float32)[None], pos, planes, None)
    assert np.abs(_np(rgb) - (k + 1) / 10.0).max() < 1e-5
    assert np.abs(_np(dep) - k / d).max() < 1e-5


def test_domain_guard(gpu):
    torch, m, o = gpu
    rgba = torch.zeros((1, 8, 16, 2, 4), device="cuda")
    with pytest.raises(ValueError):
        m.msi_render_equirect_view(rgba, np.eye(4, dtype=np.float32)[None], np.array([[1.5, 0, 0]], np.float32),
                                   [100.0, 1.0], None)


def test_full_size_render_properties(gpu):
    """BASELINE size (640x320x32): size-independent properties instead of the oracle --
    (a) constant-colour layers composite to the closed form, (b) linearity in rgb."""
    torch, m, o = gpu
    b, h, w, d = 1, 320, 640, 32
    g = torch.Generator(device="cpu").manual_seed(0)
    alpha = torch.rand((b, d, h, w, 1), generator=g)
    col = torch.linspace(-1, 1, d).view(1, d, 1, 1, 1).expand(b, d, h, w, 3)
    rgba = torch.cat([col, alpha.mul(0).add(0.25)], dim=-1).cuda().permute(0, 2, 3, 1, 4)
    planes = m.inv_depths(1.0, 100.0, d)
    pos = np.array([[0.03, 0.05, -0.08]], np.float32)
    eye = np.eye(4, dtype=np.float32)[None]
    rgb = m.msi_render_equirect_view(rgba, eye, pos, planes, None)
    exp = float(col[0, 0, 0, 0, 0])
    for i in range(1, d):
        exp = float(col[0, i, 0, 0, 0]) * 0.25 + exp * 0.75
    assert torch.abs(rgb - exp).max().item() < 1e-5
    # linearity: render(2*rgb_layers) == 2*render(rgb_layers) for the colour channels
    rnd = torch.rand((b, h, w, d, 4), generator=g).cuda()
    r1 = m.msi_render_equirect_view(rnd, eye, pos, planes, None)
    rnd2 = rnd.clone()
    rnd2[..., :3] *= 2
    r2 = m.msi_render_equirect_view(rnd2, eye, pos, planes, None)
    assert torch.allclose(r2, 2 * r1, atol=1e-5)


@pytest.mark.parametrize("order", [1, -1])
def test_render_ods_view_matches_oracle(gpu, order):
    """msi_render_ods_view (msi.py:502-525; test.py:176-188 renders both eyes)."""
    torch, m, o = gpu
    b, h, w, d = 2, 32, 64, 6
    rgba = random_rgba(21, b, h, w, d)
    inp = make_inputs(9, b, h, w)
    planes = m.inv_depths(1.0, 100.0, d)
    eye = np.eye(4, dtype=np.float32)[None]
    got = m.msi_render_ods_view(torch.from_numpy(rgba).cuda(), order, eye, inp["tgt_pos"], planes, inp["intrinsics"])
    ref = o.msi_render_ods_view(rgba, order, eye, inp["tgt_pos"], planes, inp["intrinsics"])
    assert tuple(got.shape) == ref.shape == (b, h, w, 3)
    assert np.abs(_np(got) - ref).max() <= TOL


@pytest.mark.parametrize("vw", [0, 1, 3])
def test_render_perspective_view_matches_oracle(gpu, vw):
    """msi_render_perspective_view (msi.py:475-500; test.py:160-175 renders four crops)."""
    torch, m, o = gpu
    b, h, w, d = 1, 32, 64, 5
    rgba = random_rgba(22, b, h, w, d)
    inp = make_inputs(10, b, h, w)
    planes = m.inv_depths(1.0, 100.0, d)
    got = m.msi_render_perspective_view(torch.from_numpy(rgba).cuda(), inp["tgt_pose_rt"], inp["tgt_pos"], planes,
                                        inp["intrinsics"], viewing_window=vw, psp_height=27, psp_width=48)
    ref = o.msi_render_perspective_view(rgba, inp["tgt_pose_rt"], inp["tgt_pos"], planes, inp["intrinsics"],
                                        viewing_window=vw, psp_height=27, psp_width=48)
    assert tuple(got.shape) == ref.shape == (b, 27, 48, 3)
    assert np.abs(_np(got) - ref).max() <= TOL


@pytest.mark.parametrize("scheme", ["blend_psv", "blend_bg", "blend_bg_psv", "alpha_only"])
@pytest.mark.parametrize("bf16_psv", [False, True])
def test_assemble_colour_schemes_bit_exact(gpu, scheme, bf16_psv):
    """which_color_pred (msi.py:119-275) through K3: same fp32 op order as the oracle -> bit-exact, including the odd
    channel counts of blend_bg (2D+3) and blend_bg_psv (3D+3) and the optional [B,H,W,D] outputs (msi.py:276-289)."""
    torch, m, o = gpu
    from oracle import nets as onets
    b, h, w, d = 2, 24, 40, 8
    rng = np.random.RandomState(17)
    psv = rng.uniform(-1, 1, size=(b, h, w, 6 * d)).astype(np.float32)
    if bf16_psv:
        psv = onets.bf16_round(psv)
    nout = {"blend_psv": 2 * d, "blend_bg": 2 * d + 3, "blend_bg_psv": 3 * d + 3, "alpha_only": d}[scheme]
    pred = np.tanh(rng.normal(size=(b, h, w, nout))).astype(np.float32)
    t_psv = torch.from_numpy(psv).cuda()
    out = m.assemble_layers(t_psv.bfloat16() if bf16_psv else t_psv, torch.from_numpy(pred).cuda(), d,
                            extra_outputs="blend_weights_alphas", which_color_pred=scheme)
    ref = o.assemble(psv, pred, d, "blend_weights_alphas", scheme)
    assert set(out) == set(ref), (sorted(out), sorted(ref))
    for k in ref:
        assert np.array_equal(_np(out[k]), ref[k]), k


def test_jitter_pose_enters_the_sweep(gpu):
    """FLAGS.jitter (msi.py:1118-1120): ref_pose_inv <- ref_pose_inv @ jitter_pose_inv before the sweep."""
    torch, m, o = gpu
    from matryodshka_amd import poses
    b, h, w, d = 1, 32, 64, 4
    inp = make_inputs(9, b, h, w)
    planes = m.inv_depths(1.0, 100.0, d)
    jit = poses.random_rotation(1.0, 1.0, np.random.RandomState(4))
    jinv = np.linalg.inv(jit.astype(np.float64)).astype(np.float32)
    ref = m.preprocess_image(torch.from_numpy(inp["ref_image"]))
    src = m.preprocess_image(torch.from_numpy(inp["src_image"]))
    psv = m.format_network_input(ref, src, inp["ref_pose"], inp["src_pose"], planes, inp["intrinsics"], jitter_pose_inv=jinv)
    psv0 = m.format_network_input(ref, src, inp["ref_pose"], inp["src_pose"], planes, inp["intrinsics"])
    psv_o = o.format_network_input(o.preprocess_image(inp["ref_image"]), o.preprocess_image(inp["src_image"]),
                                   inp["ref_pose"], inp["src_pose"], planes, inp["intrinsics"], jitter_pose_inv=jinv)
    assert np.abs(_np(psv) - psv_o).max() <= TOL
    assert np.abs(_np(psv) - _np(psv0)).max() > 1e-2          # the jitter really moved the samples


def test_domain_guard_uses_the_full_pose(gpu):
    """The ray origin is pose @ permuted(tgt_pos), translation included (spherical.py:286-310): a small tgt_pos with a
    large pose translation is outside the innermost sphere and must be rejected on the host; device-side inputs skip
    the guard and stay finite (clamped discriminant)."""
    torch, m, o = gpu
    b, h, w, d = 1, 16, 32, 4
    rgba = torch.from_numpy(random_rgba(1, b, h, w, d)).cuda()
    planes = m.inv_depths(1.0, 100.0, d)
    pose = np.eye(4, dtype=np.float32)[None].copy()
    pose[0, 0, 3] = 1.5
    pos = np.zeros((1, 3), np.float32)
    with pytest.raises(ValueError):
        m.msi_render_equirect_view(rgba, pose, pos, planes, None)
    with pytest.raises(ValueError):
        m.msi_render_perspective_view(rgba, pose, np.array([[0.0, 0.0, 1.2]], np.float32), planes, None, psp_height=8, psp_width=8)
    assert m.render_status() == 0                              # (nothing launched so far: the host guard raised first)
    out = m.msi_render_equirect_view(rgba, torch.from_numpy(pose).cuda(), torch.from_numpy(pos).cuda(), planes, None)
    assert bool(torch.isfinite(out).all())
    with pytest.raises(ValueError):                            # device-side inputs: the kernel clamps AND says so (status word)
        m.render_status()
    assert m.render_status() == 0                              # (the word is reset by the report)
    ok = pose.copy(); ok[0, 0, 3] = 0.5                        # inside the innermost sphere (radius 1): no bit
    m.msi_render_equirect_view(rgba, torch.from_numpy(ok).cuda(), torch.from_numpy(pos).cuda(), planes, None)
    m.msi_render_equirect_view_single(rgba, torch.from_numpy(ok).cuda(), torch.from_numpy(pos).cuda(), planes, None)
    assert m.render_status() == 0
    m.msi_render_equirect_view_single(rgba, torch.from_numpy(pose).cuda(), torch.from_numpy(pos).cuda(), planes, None)
    with pytest.raises(ValueError):
        m.render_status()
    same = m.msi_render_equirect_depth_single(rgba, np.eye(4, dtype=np.float32)[None], pos, planes, None)
    assert torch.equal(same, m.msi_render_equirect_view_single(rgba, np.eye(4, dtype=np.float32)[None], pos, planes, None))


@pytest.mark.parametrize("d", [8, 6])          # 8: whole-pixel coalesced stores; 6 (3 depth groups per pixel): strided path
@pytest.mark.parametrize("same_pose", [True, False])
@pytest.mark.parametrize("bf16", [False, True])
def test_sweep_volume_equals_two_single_source_sweeps(gpu, same_pose, bf16, d):
    """msi_ods_sweep_volume (both sources in one launch, the branch-deciding quadratic shared when the two poses are
    equal) against two msi_ods_sphere_sweep_* calls through the C ABI: bit-identical either way."""
    torch, m, o = gpu
    from matryodshka_amd import _native as N
    b, h, w = 2, 24, 48
    inp = make_inputs(23, b, h, w)
    ref = m.preprocess_image(torch.from_numpy(inp["ref_image"]))
    src = m.preprocess_image(torch.from_numpy(inp["src_image"]))
    p0 = np.tile(np.eye(4, dtype=np.float32)[None], (b, 1, 1))
    p1 = p0.copy()
    if not same_pose:
        p1[:, 0, 3] = 0.01; p1[1, 1, 3] = -0.02
    t0, t1 = torch.from_numpy(p0).cuda(), torch.from_numpy(p1).cuda()
    intr = torch.from_numpy(inp["intrinsics"]).cuda()
    depths = torch.tensor(m.inv_depths(1.0, 100.0, d), dtype=torch.float32).cuda()
    trig = m._trig(h, w)
    dt = torch.bfloat16 if bf16 else torch.float32
    both = torch.zeros((b, h, w, 6 * d), dtype=dt, device="cuda")
    two = torch.zeros_like(both)
    N.check(N.lib.msi_ods_sweep_volume(ref.data_ptr(), src.data_ptr(), t0.data_ptr(), t1.data_ptr(), intr.data_ptr(),
                                       depths.data_ptr(), trig.data_ptr(), b, h, w, d, both.data_ptr(), int(bf16), None), "volume")
    single = N.lib.msi_ods_sphere_sweep_bf16 if bf16 else N.lib.msi_ods_sphere_sweep_f32
    for i, (img, pose, order) in enumerate(((ref, t0, 1), (src, t1, -1))):
        N.check(single(img.data_ptr(), pose.data_ptr(), intr.data_ptr(), depths.data_ptr(), trig.data_ptr(), b, h, w, d,
                       order, two.data_ptr(), 6 * d, i * 3 * d, None), "single")
    torch.cuda.synchronize()
    assert torch.equal(both, two)
    if not bf16:
        want = np.concatenate([__import__("oracle.geometry", fromlist=["x"]).ods_sphere_sweep(o.preprocess_image(img), order, m.inv_depths(1.0, 100.0, d), pose, inp["intrinsics"])
                               for img, pose, order in ((inp["ref_image"], p0, 1), (inp["src_image"], p1, -1))], axis=3)
        assert np.abs(_np(both) - want).max() <= TOL


@pytest.mark.parametrize("bf16", [False, True])
@pytest.mark.parametrize("b,d", [(7, 8), (19, 8), (5, 6)])     # 19 > the 16-frame chunk of a thread; d = 6: strided store path
def test_sweep_batch_loop_reuses_corners_only_between_equal_frames(gpu, b, d, bf16):
    """Round 4: a thread keeps the sample corners of its (pixel, depths) and walks the frames of the batch, recomputing
    them only when a frame's (ref pose, src pose, baseline) differ from the frame they were computed for (wave-uniform
    compare).  One batch mixing runs of equal frames, a changed src pose, a changed ref pose, a changed baseline and a
    return to the first setting must equal -- bit for bit -- every frame swept ALONE (batch 1: nothing to reuse), and
    the oracle within 1e-3."""
    torch, m, o = gpu
    from matryodshka_amd import _native as N
    h, w = 24, 48
    inp = make_inputs(41, b, h, w)
    ref = m.preprocess_image(torch.from_numpy(inp["ref_image"]))
    src = m.preprocess_image(torch.from_numpy(inp["src_image"]))
    p0 = np.tile(np.eye(4, dtype=np.float32)[None], (b, 1, 1))
    p1 = p0.copy()
    intr = inp["intrinsics"].copy()
    p1[2, 0, 3] = 0.01                         # frame 2: src pose differs (frames 0, 1 equal; 3 returns to the first setting)
    if b > 4:
        p0[4, 1, 3] = -0.02                    # frame 4: ref pose differs
    if b > 5:
        intr[5:7, 0, 0] = 0.05                 # frames 5, 6: another baseline, equal to each other
    if b > 17:
        p1[17, 2, 3] = 0.015                   # second chunk of 16: frame 16 starts it, 17 differs, 18 equals 16
    t0, t1, ti = torch.from_numpy(p0).cuda(), torch.from_numpy(p1).cuda(), torch.from_numpy(intr).cuda()
    depths = torch.tensor(m.inv_depths(1.0, 100.0, d), dtype=torch.float32).cuda()
    trig = m._trig(h, w)
    dt = torch.bfloat16 if bf16 else torch.float32
    whole = torch.zeros((b, h, w, 6 * d), dtype=dt, device="cuda")
    alone = torch.zeros_like(whole)
    N.check(N.lib.msi_ods_sweep_volume(ref.data_ptr(), src.data_ptr(), t0.data_ptr(), t1.data_ptr(), ti.data_ptr(),
                                       depths.data_ptr(), trig.data_ptr(), b, h, w, d, whole.data_ptr(), int(bf16), None), "volume")
    for k in range(b):
        N.check(N.lib.msi_ods_sweep_volume(ref[k:k + 1].data_ptr(), src[k:k + 1].data_ptr(), t0[k:k + 1].data_ptr(), t1[k:k + 1].data_ptr(),
                                           ti[k:k + 1].data_ptr(), depths.data_ptr(), trig.data_ptr(), 1, h, w, d,
                                           alone[k:k + 1].data_ptr(), int(bf16), None), "volume of one frame")
    torch.cuda.synchronize()
    assert torch.equal(whole, alone)
    assert not torch.equal(whole[1], whole[2]) and not torch.equal(whole[0], whole[1])       # (different images / poses)
    if not bf16:
        G = __import__("oracle.geometry", fromlist=["x"])
        want = np.concatenate([G.ods_sphere_sweep(o.preprocess_image(img), order, m.inv_depths(1.0, 100.0, d), pose, intr)
                               for img, pose, order in ((inp["ref_image"], p0, 1), (inp["src_image"], p1, -1))], axis=3)
        assert np.abs(_np(whole) - want).max() <= TOL


def _rot(ax, ay, az):
    cx, sx, cy, sy, cz, sz = np.cos(ax), np.sin(ax), np.cos(ay), np.sin(ay), np.cos(az), np.sin(az)
    rx = np.array([[1, 0, 0], [0, cx, -sx], [0, sx, cx]]); ry = np.array([[cy, 0, sy], [0, 1, 0], [-sy, 0, cy]]); rz = np.array([[cz, -sz, 0], [sz, cz, 0], [0, 0, 1]])
    m = np.eye(4); m[:3, :3] = rz @ ry @ rx
    return m.astype(np.float32)


@pytest.mark.parametrize("bf16", [False, True])
@pytest.mark.parametrize("h,w,d,b", [(24, 64, 16, 5), (40, 64, 32, 3), (16, 32, 64, 2), (24, 128, 8, 19), (24, 64, 16, 19)])      # (how many blocks of each stage: tests/test_sweep_cases_cpu.py)
def test_lds_staged_sweep_is_bit_identical_to_the_gather_kernel(gpu, h, w, d, b, bf16):
    """Round 6: ods_sweep_lds_kernel stages the source patch a block's samples fall into in LDS and gathers from there; blocks whose box
    does not fit keep gathering from memory.  Taken for the double volume at batch >= 2 when blocks are full ((W * D / 2) % 256 == 0).  It must reproduce, bit for
    bit, (a) the two single-source sweeps (ods_sweep_kernel, the gather form) and (b) every frame swept alone (batch 1: gather form) -- on a batch that mixes identical
    frames (corner reuse + patch prefetch), a translated source, a ROTATED source (samples anywhere: fallback blocks), a rotated reference, a large baseline
    (wide polar boxes, invalid near planes sampling pixel (1, 1)), and, at b = 19, a second 16-frame chunk."""
    torch, m, o = gpu
    from matryodshka_amd import _native as N
    assert (w * (d // 2)) % 256 == 0 and 64 % (d // 2) == 0
    inp = make_inputs(77, b, h, w)
    ref = m.preprocess_image(torch.from_numpy(inp["ref_image"]))
    src = m.preprocess_image(torch.from_numpy(inp["src_image"]))
    p0 = np.tile(np.eye(4, dtype=np.float32)[None], (b, 1, 1))
    p1 = p0.copy()
    intr = inp["intrinsics"].copy()
    p1[1, 0, 3] = 0.01                                   # frame 1: translated source
    if b > 2:
        p1[2] = _rot(0.3, -0.5, 0.2); p1[2, :3, 3] = (0.01, -0.02, 0.005)      # frame 2: rotated source
    if b > 3:
        p0[3] = _rot(-0.1, 0.05, 0.0)                    # frame 3: rotated reference (frame 4 returns to the identity setting of frame 0)
    if b > 6:
        intr[5:7, 0, 0] = 0.4                            # frames 5, 6: a baseline 12 x the usual one, equal to each other (reuse with wide boxes)
    if b > 17:
        p1[17, 2, 3] = 0.015
    t0, t1, ti = torch.from_numpy(p0).cuda(), torch.from_numpy(p1).cuda(), torch.from_numpy(intr).cuda()
    depths = torch.tensor(m.inv_depths(1.0, 100.0, d), dtype=torch.float32).cuda()
    trig = m._trig(h, w)
    dt = torch.bfloat16 if bf16 else torch.float32
    whole = torch.full((b, h, w, 6 * d), 7.0, dtype=dt, device="cuda")
    two = torch.zeros_like(whole)
    alone = torch.zeros_like(whole)
    N.check(N.lib.msi_ods_sweep_volume(ref.data_ptr(), src.data_ptr(), t0.data_ptr(), t1.data_ptr(), ti.data_ptr(),
                                       depths.data_ptr(), trig.data_ptr(), b, h, w, d, whole.data_ptr(), int(bf16), None), "volume")
    single = N.lib.msi_ods_sphere_sweep_bf16 if bf16 else N.lib.msi_ods_sphere_sweep_f32
    for k, (img, pose, order) in enumerate(((ref, t0, 1), (src, t1, -1))):
        N.check(single(img.data_ptr(), pose.data_ptr(), ti.data_ptr(), depths.data_ptr(), trig.data_ptr(), b, h, w, d,
                       order, two.data_ptr(), 6 * d, k * 3 * d, None), "single")
    for k in range(b):
        N.check(N.lib.msi_ods_sweep_volume(ref[k:k + 1].data_ptr(), src[k:k + 1].data_ptr(), t0[k:k + 1].data_ptr(), t1[k:k + 1].data_ptr(),
                                           ti[k:k + 1].data_ptr(), depths.data_ptr(), trig.data_ptr(), 1, h, w, d,
                                           alone[k:k + 1].data_ptr(), int(bf16), None), "volume of one frame")
    torch.cuda.synchronize()
    assert torch.equal(whole, two), int((whole != two).sum())
    assert torch.equal(whole, alone)
    if not bf16:
        G = __import__("oracle.geometry", fromlist=["x"])
        want = np.concatenate([G.ods_sphere_sweep(o.preprocess_image(img), order, m.inv_depths(1.0, 100.0, d), pose, intr)
                               for img, pose, order in ((inp["ref_image"], p0, 1), (inp["src_image"], p1, -1))], axis=3)
        assert np.abs(_np(whole) - want).max() <= TOL


@pytest.mark.parametrize("h,w,d,b", [(16, 32, 32, 3), (24, 64, 16, 2), (8, 64, 4, 2), (8, 8, 64, 1)])
def test_pp_sweep_fast_form_is_bit_identical_to_the_generic_one(gpu, h, w, d, b):
    """Round 6: pp_sweep_kernel<1> (face matrix through LDS, 12-byte buffer loads, whole-pixel 16-byte stores through a wave strip) is taken when waves hold complete
    pixels and the runs are 16-byte aligned; a channel offset of 1 into a wider volume forces the generic form on the SAME problem: every value must agree bit for bit."""
    torch, m, o = gpu
    from matryodshka_amd import _native as N
    assert 64 % d == 0 and (w * d) % 256 == 0
    rng = np.random.RandomState(5 + d)
    img = torch.from_numpy(rng.uniform(-1, 1, size=(b, h, w, 3)).astype(np.float32)).cuda()
    pose = np.tile(np.eye(4, dtype=np.float32)[None], (b, 1, 1))
    pose[:, 0, 3] = -0.032
    if b > 1:
        pose[1] = _rot(0.05, -0.1, 0.02); pose[1, :3, 3] = (0.02, 0.01, -0.03)
    intr = np.tile(np.array([[w / 2.0, 0, w / 2.0], [0, h / 2.0, h / 2.0], [0, 0, 1]], dtype=np.float32)[None], (b, 1, 1))
    depths = torch.tensor(m.inv_depths(1.0, 100.0, d), dtype=torch.float32).cuda()
    tp, ti = torch.from_numpy(pose).cuda(), torch.from_numpy(intr).cuda()
    fast = torch.full((b, h, w, 6 * d), 7.0, device="cuda")
    slow = torch.full((b, h, w, 6 * d + 4), 7.0, device="cuda")
    for coff in (0, 3 * d):
        N.check(N.lib.msi_perspective_plane_sweep_f32(img.data_ptr(), tp.data_ptr(), ti.data_ptr(), depths.data_ptr(), b, h, w, d, fast.data_ptr(), 6 * d, coff, None), "pp fast")
        N.check(N.lib.msi_perspective_plane_sweep_f32(img.data_ptr(), tp.data_ptr(), ti.data_ptr(), depths.data_ptr(), b, h, w, d, slow.data_ptr(), 6 * d + 4, coff + 1, None), "pp generic")
    torch.cuda.synchronize()
    assert torch.equal(fast, slow[..., 1:6 * d + 1])
    assert bool((slow[..., 0] == 7.0).all()) and bool((slow[..., 6 * d + 1:] == 7.0).all()) and not bool((fast == 7.0).any())


def test_pair_launches_equal_single_ones(gpu):
    """preprocess / deprocess of the two images of a frame in one launch: same bits as the single-image entry points."""
    torch, m, o = gpu
    inp = make_inputs(4, 2, 16, 32)
    a, b = torch.from_numpy(inp["ref_image"]).cuda(), torch.from_numpy(inp["src_image"]).cuda()
    pa, pb = m.preprocess_image_pair(a, b)
    assert torch.equal(pa, m.preprocess_image(a)) and torch.equal(pb, m.preprocess_image(b))
    x = torch.rand((2, 16, 32, 3), device="cuda") * 2.4 - 1.2
    y = torch.rand((2, 16, 32, 3), device="cuda") * 1.2 - 0.1
    r8, d8 = m.deprocess_image_and_depth(x, y)
    assert torch.equal(r8, m.deprocess_image(x)) and torch.equal(d8, m.deprocess_depth_image(y))
