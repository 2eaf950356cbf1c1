"""GPU checks of the bf16 network tier on perspective (PP) inputs: the one-launch bf16 sweep volume
(msi_perspective_sweep_volume_bf16) is the round-to-nearest-even of the fp32 volume of two msi_perspective_plane_sweep_f32
launches, bit for bit, in both of its forms and with non-temporal stores; the pipeline (sweep -> bf16 network -> assembly ->
mpi_render_view) tracks the bf16 oracle (oracle/msi.py with dtype='bf16', input_type='PP') at the bf16 tolerances of
tests/test_gpu_bf16.py: max-abs 6e-2, mean-abs 3e-3; and the harness runs it with --dtype bf16."""
import numpy as np
import pytest

pytestmark = pytest.mark.gpu

# BASELINE configs[4] fixture (tests/golden/make_golden_pp_bf16.py)
FIXTURE = "full_config4_pp_bf16_256x256x32_b2_samples.npz"


@pytest.fixture(scope="module")
def torch():
    import torch
    assert torch.cuda.is_available(), "GPU tests need a HIP device"
    return torch


def _rot(ax, ay, az):
    cx, sx, cy, sy, cz, sz = np.cos(ax), np.sin(ax), np.cos(ay), np.sin(ay), np.cos(az), np.sin(az)
    rx = np.array([[1, 0, 0], [0, cx, -sx], [0, sx, cx]]); ry = np.array([[cy, 0, sy], [0, 1, 0], [-sy, 0, cy]]); rz = np.array([[cz, -sz, 0], [sz, cz, 0], [0, 0, 1]])
    return rz @ ry @ rx


def _case(seed, b, h, w):
    """Raw [0,1] images, PP intrinsics (fx = cx = W/2, fy = cy = H/2), identity ref poses, src poses shifted along -x and
    (on odd faces) rotated, and ref_pose_inv = the inverse of the slerp mid-point pose (train.py:118-121)."""
    from matryodshka_amd import poses
    from tests.util import smooth_noise
    if h == w:
        from tests.golden.make_golden import pp_inputs
        ref, src, K, eye, src_pose, _ = pp_inputs(seed, b, h)
    else:
        rng = np.random.RandomState(seed)
        ref, src = smooth_noise(rng, b, h, w), smooth_noise(rng, b, h, w)
        K = np.tile(np.array([[w / 2, 0, w / 2], [0, h / 2, h / 2], [0, 0, 1]], np.float32)[None], (b, 1, 1))
        eye = np.tile(np.eye(4, dtype=np.float32)[None], (b, 1, 1))
        src_pose = eye.copy()
        src_pose[:, 0, 3] = -0.064
        for k in range(1, b, 2):
            src_pose[k, :3, :3] = _rot(0.02 * k, 0.05, -0.01).astype(np.float32)
    interp_inv = np.linalg.inv(poses.interpolate_pose(eye, src_pose).astype(np.float64)).astype(np.float32)
    return ref, src, K, eye, src_pose, interp_inv


def _volumes(torch, m, case, d):
    """(bf16 volume of the new entry point, fp32 volume of the two fp32 launches) through format_network_input."""
    ref, src, K, eye, src_pose, interp_inv = case
    planes = m.inv_depths(1.0, 100.0, d)
    r, s = m.preprocess_image_pair(torch.from_numpy(ref), torch.from_numpy(src))
    v16 = m.format_network_input(r, s, eye, src_pose, planes, K, ref_pose_inv=interp_inv)
    v32 = m.format_network_input(r, s, eye, src_pose, planes, K, ref_pose_inv=interp_inv, dtype="f32")
    torch.cuda.synchronize()
    assert v16.dtype == torch.bfloat16 and v32.dtype == torch.float32
    return v16, v32


def _assert_bits_equal(torch, v16, v32):
    want = v32.to(torch.bfloat16).view(torch.int16)
    got = v16.view(torch.int16)
    assert got.shape == want.shape
    assert torch.equal(got, want), int((got != want).sum())


@pytest.mark.parametrize("b,h,w,d", [
    (4, 256, 256, 32),    # configs[4] faces, fast form; odd faces have rotated sources
    (2, 40, 50, 6),       # generic form (D does not divide 64, W * D % 64 != 0)
    (3, 33, 47, 5),       # generic form, odd sizes
    (2, 32, 64, 64),      # D = 64: one pixel per wave
    (3, 48, 96, 16),      # H != W
    (2, 16, 64, 2),       # D = 2 (inv_depths gives at least the two end planes): 32 pixels per wave
    (11, 256, 256, 32),   # 277 MB > 256 MB: the non-temporal stores
])
def test_bf16_pp_volume_is_the_rounded_fp32_volume(torch, b, h, w, d):
    from matryodshka_amd import MSI
    m = MSI(input_type="PP", dtype="bf16")
    v16, v32 = _volumes(torch, m, _case(100 + d, b, h, w), d)
    assert v16.shape == (b, h, w, 6 * d)
    _assert_bits_equal(torch, v16, v32)
    assert bool(torch.isfinite(v32).all())


def test_bf16_pp_volume_far_outside_the_face_is_the_rounded_fp32_volume(torch):
    """Source cameras turned and moved far enough that many samples land outside [-1, n] and wrap around (make_taps' generic
    floor-mod inside the fast form, mixed with in-range samples in the same waves); one camera is turned by 3 rad."""
    from matryodshka_amd import MSI
    b, n, d = 4, 64, 16
    ref, src, K, eye, src_pose, interp_inv = _case(71, b, n, n)
    for k, (ang, t) in enumerate(((0.4, 0.5), (-0.7, -1.5), (1.2, 3.0), (3.0, 0.2))):
        src_pose[k, :3, :3] = _rot(0.3 * ang, ang, -0.5 * ang).astype(np.float32)
        src_pose[k, :3, 3] = (t, -0.5 * t, 0.25 * t)
    m = MSI(input_type="PP", dtype="bf16")
    v16, v32 = _volumes(torch, m, (ref, src, K, eye, src_pose, np.tile(np.eye(4, dtype=np.float32)[None], (b, 1, 1))), d)
    _assert_bits_equal(torch, v16, v32)


@pytest.mark.parametrize("b,h,w,d", [(2, 64, 64, 32), (3, 32, 64, 8)])
def test_bf16_pp_fast_form_equals_generic_form(torch, b, h, w, d):
    """A volume pointer that is not 16-byte aligned sends the same problem to the generic form: bit for bit the same values,
    and nothing outside the volume is written."""
    from matryodshka_amd import MSI, _native as N
    m = MSI(input_type="PP", dtype="bf16")
    ref, src, K, eye, src_pose, interp_inv = _case(7 + d, b, h, w)
    r, s = m.preprocess_image_pair(torch.from_numpy(ref), torch.from_numpy(src))
    p0, p1, inv = (torch.from_numpy(np.ascontiguousarray(x)).cuda() for x in (eye, src_pose, interp_inv))
    cur = torch.empty((2, b, 4, 4), dtype=torch.float32, device="cuda")
    N.check(N.lib.msi_compose_pose_pair_f32(p0.data_ptr(), p1.data_ptr(), inv.data_ptr(), cur[0].data_ptr(), cur[1].data_ptr(), b, None), "poses")
    intr = torch.from_numpy(K).cuda()
    depths = torch.tensor(m.inv_depths(1.0, 100.0, d), dtype=torch.float32).cuda()
    n = b * h * w * 6 * d
    bufs = []
    for off in (0, 1):     # element offset 0: 16-byte aligned (fast form); 1: 2 bytes past it (generic form)
        buf = torch.full((n + 8,), 0x5a5a, dtype=torch.int16, device="cuda")
        N.check(N.lib.msi_perspective_sweep_volume_bf16(r.data_ptr(), s.data_ptr(), cur[0].data_ptr(), cur[1].data_ptr(), intr.data_ptr(),
                                                        depths.data_ptr(), b, h, w, d, buf.data_ptr() + 2 * off, None), "sweep volume")
        bufs.append(buf)
    torch.cuda.synchronize()
    fast, slow = bufs
    assert torch.equal(fast[:n], slow[1:n + 1])
    assert bool((fast[n:] == 0x5a5a).all()) and int(slow[0]) == 0x5a5a and bool((slow[n + 1:] == 0x5a5a).all())
    assert not bool((fast[:n] == 0x5a5a).all())


def test_bf16_pp_volume_matches_bf16_oracle(torch):
    from matryodshka_amd import MSI
    from oracle.msi import MSI as OracleMSI
    b, h, w, d = 2, 32, 48, 8
    ref, src, K, eye, src_pose, interp_inv = _case(21, b, h, w)
    m = MSI(input_type="PP", dtype="bf16")
    o = OracleMSI(input_type="PP", dtype="bf16")
    planes = m.inv_depths(1.0, 100.0, d)
    v16, _ = _volumes(torch, m, (ref, src, K, eye, src_pose, interp_inv), d)
    want = o.format_network_input(o.preprocess_image(ref), o.preprocess_image(src), eye, src_pose, planes, K, ref_pose_inv=interp_inv)
    err = np.abs(v16.float().cpu().numpy().astype(np.float64) - want)
    # the same bf16 rounding of fp32 values that may differ in the last bits: a rounding boundary crossed at most once per value
    assert err.max() <= 2.0 ** -7 and err.mean() <= 1e-5, (err.max(), err.mean())


@pytest.mark.parametrize("coord", [True, False])
@pytest.mark.parametrize("scheme", ["blend_psv", "alpha_only", "blend_bg"])
def test_bf16_pp_pipeline_matches_bf16_oracle(torch, coord, scheme):
    """infer_msi -> mpi_render_view on a bf16 PP model against the bf16 oracle.  blend_psv takes the fused head + assembly
    (msi_net_plan_forward_rgba, on the bf16 volume as colour source); the other schemes take run_net + assemble_layers."""
    from matryodshka_amd import MSI
    from oracle import nets as onets
    from oracle.msi import MSI as OracleMSI
    b, h, w, d, ngf = 2, 32, 48, 8, 16
    nout = {"blend_psv": 2 * d, "blend_bg": 2 * d + 3, "alpha_only": d}[scheme]
    ref, src, K, eye, src_pose, interp_inv = _case(31, b, h, w)
    tgt_pose = eye.copy()
    tgt_pose[:, 0, 3], tgt_pose[:, 1, 3] = -0.03, 0.01
    weights = onets.init_weights(6 * d, nout, ngf=ngf, coord_net=coord, seed=41, randomize_affine=True)
    m = MSI(weights=weights, coord_net=coord, input_type="PP", dtype="bf16")
    o = OracleMSI(weights=weights, coord_net=coord, input_type="PP", dtype="bf16")
    planes = m.inv_depths(1.0, 100.0, d)
    calls = []
    run_net = m.run_net
    m.run_net = lambda *a, **k: calls.append(1) or run_net(*a, **k)
    pred, net_input = m.infer_msi(torch.from_numpy(src), torch.from_numpy(ref), None, None, eye, src_pose, K, scheme, d, planes,
                                  ngf=ngf, ref_pose_inv=interp_inv)
    rel = np.matmul(tgt_pose, interp_inv).astype(np.float32)
    rgb = m.mpi_render_view(pred["rgba_layers"], rel, planes, K)
    torch.cuda.synchronize()
    assert net_input.dtype == torch.bfloat16
    assert calls == ([] if scheme == "blend_psv" else [1])          # fused path only for blend_psv
    assert m.network_status() == 0
    pred_o, _ = o.infer_msi(src, ref, None, None, eye, src_pose, K, scheme, d, planes, ngf=ngf, ref_pose_inv=interp_inv)
    rgb_o = o.mpi_render_view(pred_o["rgba_layers"], rel, planes, K)
    for name, got, want in (("rgba_layers", pred["rgba_layers"], pred_o["rgba_layers"]), ("rgb", rgb, rgb_o)):
        err = np.abs(got.cpu().numpy().astype(np.float64) - want)
        assert err.max() <= 6e-2 and err.mean() <= 3e-3, (name, err.max(), err.mean())


def test_bf16_pp_full_size_config4_matches_oracle(torch):
    """BASELINE configs[4] in bf16: two 256x256 faces (the second with a rotated source), 32 planes, ngf 64, CoordNet, against the
    bf16 oracle's dense samples (max-abs 6e-2, mean-abs 3e-3; the volume within one bf16 rounding) -- and the distance of this path
    from the FP32 oracle against the distance of the bf16 oracle from it (+10 % on the mean, +25 % on the max, as for configs[2])."""
    import os
    from matryodshka_amd import MSI, poses
    from oracle import nets as onets
    from tests.golden.make_golden import pp_inputs
    from tests.util import stratified_index
    path = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", FIXTURE)
    z = np.load(path, allow_pickle=True)
    cfg = {k: v for k, v in z["cfg"]}
    b, n, d, ngf, seed = (int(cfg[k]) for k in ("b", "n", "d", "ngf", "seed"))
    ref, src, K, eye, src_pose, tgt_pose = pp_inputs(seed, b, n)
    weights = onets.init_weights(6 * d, 2 * d, ngf=ngf, coord_net=True, seed=seed, randomize_affine=True)
    m = MSI(weights=weights, coord_net=True, input_type="PP", dtype="bf16")
    planes = m.inv_depths(1.0, 100.0, d)
    interp_inv = np.linalg.inv(poses.interpolate_pose(eye, src_pose).astype(np.float64)).astype(np.float32)
    pred, net_input = m.infer_msi(torch.from_numpy(src), torch.from_numpy(ref), None, None, eye, src_pose, K, "blend_psv", d, planes,
                                  ngf=ngf, ref_pose_inv=interp_inv)
    rgb = m.mpi_render_view(pred["rgba_layers"], np.matmul(tgt_pose, interp_inv).astype(np.float32), planes, K)
    assert m.network_status() == 0
    got = dict(psv=net_input.float().cpu().numpy(), rgba_layers=pred["rgba_layers"].cpu().numpy(), rgb=rgb.cpu().numpy())
    seed_s, cap = int(z["sample_seed"]), int(z["sample_cap"])
    psv_want = (z["bits_psv"].astype(np.uint32) << 16).view(np.float32)
    for k in ("psv", "rgba_layers", "rgb"):
        a = got[k]
        assert tuple(a.shape) == tuple(int(v) for v in z["shape_" + k]), (k, a.shape)
        idx = stratified_index(a.shape, None, seed_s, cap=cap)
        v = a.reshape(-1)[idx].astype(np.float64)
        want = psv_want if k == "psv" else z["val_" + k]
        assert idx.size == want.size
        err = np.abs(v - want)
        if k == "psv":
            assert err.max() <= 2.0 ** -7 and err.mean() <= 1e-5, (k, err.max(), err.mean())
            continue
        assert err.max() <= 6e-2 and err.mean() <= 3e-3, (k, err.max(), err.mean())
        assert abs(float(a.astype(np.float64).mean()) - float(z["mean_" + k])) < 2e-3, k
        e32 = np.abs(v - z["f32val_" + k])
        omax, omean = float(z["bf16_vs_f32_max_" + k]), float(z["bf16_vs_f32_mean_" + k])
        print("config4 bf16 %-11s |HIP - bf16 oracle| max %.3e mean %.3e   |HIP - fp32 oracle| max %.3e mean %.3e   "
              "|bf16 oracle - fp32 oracle| max %.3e mean %.3e" % (k, err.max(), err.mean(), e32.max(), e32.mean(), omax, omean))
        assert e32.mean() <= 1.10 * omean + 1e-5, (k, e32.mean(), omean)
        assert e32.max() <= 1.25 * omax + 1e-3, (k, e32.max(), omax)


def test_bf16_pp_volume_is_batch_independent(torch):
    """A 16-face batch (each face with its own pose and intrinsics) equals each face swept alone, bit for bit."""
    from matryodshka_amd import MSI
    b, n, d = 16, 64, 32
    ref, src, K, eye, src_pose, _ = _case(51, b, n, n)
    rng = np.random.RandomState(52)
    for k in range(b):
        src_pose[k, :3, :3] = _rot(*rng.uniform(-0.05, 0.05, size=3)).astype(np.float32)
        src_pose[k, :3, 3] = rng.uniform(-0.08, 0.08, size=3)
        K[k, 0, 0] *= np.float32(1.0 + 0.02 * k)
    from matryodshka_amd import poses
    interp_inv = np.linalg.inv(poses.interpolate_pose(eye, src_pose).astype(np.float64)).astype(np.float32)
    m = MSI(input_type="PP", dtype="bf16")
    planes = m.inv_depths(1.0, 100.0, d)
    r, s = m.preprocess_image_pair(torch.from_numpy(ref), torch.from_numpy(src))
    whole = m.format_network_input(r, s, eye, src_pose, planes, K, ref_pose_inv=interp_inv)
    for k in range(b):
        one = m.format_network_input(r[k:k + 1], s[k:k + 1], eye[k:k + 1], src_pose[k:k + 1], planes, K[k:k + 1],
                                     ref_pose_inv=interp_inv[k:k + 1])
        assert torch.equal(whole[k:k + 1].view(torch.int16), one.view(torch.int16)), k
    assert not torch.equal(whole[0], whole[1])


def test_harness_pp_bf16(tmp_path, torch):
    """harness --input_type PP --dtype bf16 writes the target and the per-plane psv PNGs; the target is within the bf16 bound of
    the same run with --dtype f32 (6e-2 max / 3e-3 mean in [-1, 1], i.e. 7.7 / 0.4 LSB plus the uint8 truncation)."""
    from PIL import Image
    from matryodshka_amd import harness
    from oracle import nets as onets
    from tests.util import smooth_noise
    n, d, ngf = 64, 8, 16
    img = tmp_path / "img"
    img.mkdir()
    rng = np.random.RandomState(61)
    for name in ("000", "001", "002"):
        Image.fromarray((smooth_noise(rng, 1, n, n)[0] * 255).astype(np.uint8)).save(str(img / ("room_2_pos%s.jpeg" % name)), quality=95)
    cam = tmp_path / "cams.txt"
    cam.write_text("room_2 000 001 002 0.064 0.03\n")
    weights = onets.init_weights(6 * d, 2 * d, ngf=ngf, coord_net=True, seed=62, randomize_affine=True)
    np.savez(str(tmp_path / "w.npz"), **weights)
    tag = "room_2_000001002"
    out = {}
    for dtype in ("bf16", "f32"):
        assert harness.main(["--cameras_glob", str(cam), "--image_dir", str(img), "--output_root", str(tmp_path / "o"),
                             "--experiment_name", dtype, "--height", str(n), "--width", str(n), "--num_msi_planes", str(d),
                             "--num_psv_planes", str(d), "--ngf", str(ngf), "--weights", str(tmp_path / "w.npz"), "--input_type", "PP",
                             "--dtype", dtype, "--strict", "--test_outputs", "tgt_image_rgba_layers_alphas_psv"]) == 1
        sample = tmp_path / "o" / dtype / tag
        out[dtype] = sample
        assert (sample / ("output_tgt_%s.png" % tag)).exists()
        for j in range(d):
            assert (sample / ("psv_plane_%.3d.png" % j)).exists(), j
        assert not (sample / "UNRELIABLE.txt").exists()
    png = lambda p: np.asarray(Image.open(str(p))).astype(int)
    diff = np.abs(png(out["bf16"] / ("output_tgt_%s.png" % tag)) - png(out["f32"] / ("output_tgt_%s.png" % tag)))
    assert diff.max() <= 9 and diff.mean() <= 1.0, (diff.max(), diff.mean())
    for j in (0, d - 1):
        dp = np.abs(png(out["bf16"] / ("psv_plane_%.3d.png" % j)) - png(out["f32"] / ("psv_plane_%.3d.png" % j)))
        assert dp.max() <= 1, (j, dp.max())
