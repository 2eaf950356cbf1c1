"""The cube path's source half sampled from the source panorama (msi_cube_plane_sweep_f32, msi_cube_sweep_volume_bf16; MSI.format_cube_input,
MSI.infer_cube(src_sampling='panorama')) against the fp64 reference of tests/cube_sweep_reference.py at the cases of tests/cube_sweep_cases.py
(tests/test_cube_sweep_cpu.py shows on the CPU that they reach past every face border).  The one tolerance against the reference is the
project's parity gate for sweep and render values in [-1, 1], 1e-3 max-abs; everything else is compared on raw bits."""
import numpy as np
import pytest

from tests import cube_sweep_cases as cases
from tests import cube_sweep_reference as ref

pytestmark = pytest.mark.gpu

F = np.float32
GATE = 1e-3
NAMES = sorted(cases.SHAPES)


@pytest.fixture(scope="module")
def model():
    from matryodshka_amd import MSI
    return MSI(input_type='PP')


def _bits(t):
    import torch
    t = t.contiguous()
    return t.view({4: torch.int32, 2: torch.int16}[t.element_size()])


_SWEPT = {}


def _sweep(m, name):
    """The fp32 cube sweep of a case into the src window of a poisoned [6B,S,S,6D] volume, run once and shared: (psv, poison bits)."""
    import torch
    from matryodshka_amd import _native as N
    if name not in _SWEPT:
        x = cases.case(name)
        s, d = x["size"], x["d"]
        pano, pose, k, depths = m._f32(x["pano"]), m._f32(x["face_pose"]), m._f32(x["k"]), m._planes(x["planes"])
        psv = torch.full((6 * cases.B, s, s, 6 * d), float('nan'), dtype=torch.float32, device=m.device)
        N.check(N.lib.msi_cube_plane_sweep_f32(pano.data_ptr(), pose.data_ptr(), k.data_ptr(), depths.data_ptr(), cases.B, pano.shape[1], pano.shape[2],
                                               s, d, psv.data_ptr(), 6 * d, 3 * d, m._stream()), "msi_cube_plane_sweep_f32")
        _SWEPT[name] = psv
    return _SWEPT[name]


# 1 ---------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("name", NAMES)
def test_1_fp32_sweep_against_the_fp64_reference(model, name):
    import torch
    x, r = cases.case(name), cases.reference(name)
    s, d = x["size"], x["d"]
    psv = _sweep(model, name)
    got = psv[..., 3 * d:].cpu().numpy().reshape(6 * cases.B, s, s, d, 3).astype(np.float64)
    exc = ref.excluded(r)
    err = np.abs(got - r["value"]).max(axis=-1)
    out = ref.outside_face(r, s)
    print("%s: max-abs error %.3e (past the face border %.3e, inside %.3e), excluded %.3f %%" % (
        name, err[~exc].max(), err[out & ~exc].max(), err[~out & ~exc].max(), 100 * exc.mean()))
    assert exc.mean() <= 0.01
    assert np.isfinite(got).all()
    assert err[~exc].max() <= GATE
    # nothing else of the volume is touched: the ref window still holds the poison
    poison = torch.full((1,), float('nan'), dtype=torch.float32).view(torch.int32).item()
    assert bool((_bits(psv[..., :3 * d]) == poison).all())


def test_1b_a_window_at_offset_zero_of_a_wider_volume(model):
    """The other placement: channels [0, 3D) of a volume with 3D + 4 channels (the whole-pixel form's 16-byte runs at another stride)."""
    import torch
    from matryodshka_amd import _native as N
    m, x = model, cases.case("s64_d4")
    s, d = x["size"], x["d"]
    pano, pose, k, depths = m._f32(x["pano"]), m._f32(x["face_pose"]), m._f32(x["k"]), m._planes(x["planes"])
    psv = torch.full((6 * cases.B, s, s, 3 * d + 4), float('nan'), dtype=torch.float32, device=m.device)
    N.check(N.lib.msi_cube_plane_sweep_f32(pano.data_ptr(), pose.data_ptr(), k.data_ptr(), depths.data_ptr(), cases.B, pano.shape[1], pano.shape[2], s, d,
                                           psv.data_ptr(), 3 * d + 4, 0, m._stream()), "msi_cube_plane_sweep_f32")
    assert torch.equal(_bits(psv[..., :3 * d]), _bits(_sweep(m, "s64_d4")[..., 3 * d:]))
    assert bool(torch.isnan(psv[..., 3 * d:]).all())


# 2 ---------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("name", NAMES)
def test_2_bf16_volume_is_the_rounded_sweep_and_the_face_wise_ref_half(model, name):
    import torch
    from matryodshka_amd import _native as N
    m, x = model, cases.case(name)
    s, d = x["size"], x["d"]
    ref_faces = m.equirect_to_cube(m._f32(x["ref_pano"]), s, x["k"][0]).reshape(6 * cases.B, s, s, 3)
    vol = m.format_cube_input(ref_faces, x["pano"], x["face_pose"], x["planes"], x["k"], dtype='bf16')
    assert vol.dtype == torch.bfloat16 and tuple(vol.shape) == (6 * cases.B, s, s, 6 * d)
    # src half: round to nearest even of the fp32 sweep
    assert torch.equal(_bits(vol[..., 3 * d:]), _bits(_sweep(m, name)[..., 3 * d:].to(torch.bfloat16)))
    # ref half: msi_perspective_sweep_volume_bf16's, whatever its src image is
    eye = torch.eye(4, dtype=torch.float32, device=m.device).expand(6 * cases.B, 4, 4).contiguous()
    k, depths = m._f32(x["k"]), m._planes(x["planes"])
    old = torch.empty_like(vol)
    N.check(N.lib.msi_perspective_sweep_volume_bf16(ref_faces.data_ptr(), ref_faces.data_ptr(), eye.data_ptr(), eye.data_ptr(), k.data_ptr(),
                                                    depths.data_ptr(), 6 * cases.B, s, s, d, old.data_ptr(), m._stream()), "msi_perspective_sweep_volume_bf16")
    assert torch.equal(_bits(vol[..., :3 * d]), _bits(old[..., :3 * d]))
    # and the fp32 volume of format_cube_input is the two fp32 sweeps
    vol32 = m.format_cube_input(ref_faces, x["pano"], x["face_pose"], x["planes"], x["k"], dtype='f32')
    assert torch.equal(_bits(vol32[..., 3 * d:]), _bits(_sweep(m, name)[..., 3 * d:]))
    want = m.format_network_input(ref_faces, ref_faces, eye, eye, x["planes"], k, ref_pose_inv=eye, dtype='f32')
    assert torch.equal(_bits(vol32[..., :3 * d]), _bits(want[..., :3 * d]))


# 3 ---------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("name", NAMES)
def test_3_interior_agreement_with_the_face_wise_path(model, name):
    """Where the face position lies in [1, S-2]^2 in front of the camera, the face-wise sweep (cut the source panorama into faces, sweep each) and
    the panorama sampling see the same scene; they differ by the resampling of the cut, m, which the two fp64 references measure."""
    import torch
    from tests.cube_reference import equirect_to_cube
    m, x, r = model, cases.case(name), cases.reference(name)
    s, d = x["size"], x["d"]
    src_faces = m.equirect_to_cube(m._f32(x["pano"]), s, x["k"][0]).reshape(6 * cases.B, s, s, 3)
    eye = torch.eye(4, dtype=torch.float32, device=m.device).expand(6 * cases.B, 4, 4).contiguous()
    old = m.format_network_input(src_faces, src_faces, eye, m._f32(x["face_pose"]), x["planes"], m._f32(x["k"]), ref_pose_inv=eye, dtype='f32')
    old = old[..., 3 * d:].cpu().numpy().reshape(6 * cases.B, s, s, d, 3).astype(np.float64)
    new = _sweep(m, name)[..., 3 * d:].cpu().numpy().reshape(6 * cases.B, s, s, d, 3).astype(np.float64)
    faces64 = equirect_to_cube(x["pano"], s, x["k"][0]).reshape(6 * cases.B, s, s, 3)
    mdiff = np.abs(r["value"] - ref.face_sweep(faces64, x["face_pose"], x["k"], x["planes"]))
    with np.errstate(invalid='ignore'):
        interior = (r["u_face"] >= 1) & (r["u_face"] <= s - 2) & (r["v_face"] >= 1) & (r["v_face"] <= s - 2) & (r["pr2"] > 0)
    interior &= ~ref.excluded(r)
    assert interior.mean() > 0.3
    diff = np.abs(new - old)
    print("%s: %d interior samples; m = %.3e max, %.3e mean; |new - old| = %.3e max; past the border |new - old| = %.3e max" % (
        name, interior.sum(), mdiff[interior].max(), mdiff[interior].mean(), diff[interior].max(), diff[~interior].max()))
    assert (diff[interior] <= mdiff[interior] + 2e-3).all()


# 4 ---------------------------------------------------------------------------------------------------------------------
def test_4_a_non_finite_pose_stays_inside_its_panorama(model):
    """NaN and Inf in ONE face's pose: the clamps take a NaN coordinate to the lower bound before any index is formed, so that face reads texels of its
    own panorama -- its values are finite or NaN and within the image range -- and every other face has the bits of the clean run."""
    import torch
    from matryodshka_amd import _native as N
    m, x = model, cases.case("s16_d4")
    s, d = x["size"], x["d"]
    pose = np.array(x["face_pose"])
    pose[7, 0, 3], pose[7, 1, 1], pose[7, 2, 0] = np.nan, np.inf, -np.inf
    pano, pose, k, depths = m._f32(x["pano"]), m._f32(pose), m._f32(x["k"]), m._planes(x["planes"])
    psv = torch.zeros((6 * cases.B, s, s, 6 * d), dtype=torch.float32, device=m.device)
    N.check(N.lib.msi_cube_plane_sweep_f32(pano.data_ptr(), pose.data_ptr(), k.data_ptr(), depths.data_ptr(), cases.B, pano.shape[1], pano.shape[2], s, d,
                                           psv.data_ptr(), 6 * d, 3 * d, m._stream()), "msi_cube_plane_sweep_f32")
    torch.cuda.synchronize()
    got, clean = psv[..., 3 * d:], _sweep(m, "s16_d4")[..., 3 * d:]
    others = [n for n in range(6 * cases.B) if n != 7]
    assert torch.equal(_bits(got[others]), _bits(clean[others]))
    bad = got[7]
    assert not bool(torch.isinf(bad).any())
    finite = bad[torch.isfinite(bad)]
    assert finite.numel() == 0 or float(finite.abs().max()) <= 1.0


# 5 ---------------------------------------------------------------------------------------------------------------------
def test_5_infer_cube_with_panorama_sampling():
    import torch
    from matryodshka_amd import MSI, cubemap
    from oracle import nets as onets
    x = cases.case("s16_d4")
    s, d, ngf, b = x["size"], x["d"], 16, cases.B
    weights = onets.init_weights(6 * d, 2 * d, ngf=ngf, coord_net=True, seed=3, randomize_affine=True)
    m = MSI(weights=weights, coord_net=True, input_type='PP')
    planes = list(x["planes"])
    raw_src, raw_ref = torch.from_numpy((np.array(x["pano"]) + 1) / 2), torch.from_numpy((np.array(x["ref_pano"]) + 1) / 2)     # [0, 1]
    got = m.infer_cube(raw_src, raw_ref, x["src_pose"], s, planes, ngf=ngf, extra_outputs='blend_weights alphas', src_sampling='panorama')
    # the composition written out
    src, ref_p = m.preprocess_image(raw_src), m.preprocess_image(raw_ref)
    k = cubemap.default_face_intrinsics(s)
    ref_faces = m.equirect_to_cube(ref_p, s, k).reshape(6 * b, s, s, 3)
    face_src = cubemap.face_poses(m._f32(x["src_pose"])).reshape(6 * b, 4, 4).contiguous()
    kf = m._f32(k).reshape(1, 3, 3).expand(6 * b, 3, 3).contiguous()
    net_input = m.format_cube_input(ref_faces, src, face_src, planes, kf)
    assert tuple(net_input.shape) == (6 * b, s, s, 6 * d) and net_input.dtype == torch.float32
    want = m.infer_layers(net_input, d, ngf, 'blend_weights alphas', 'blend_psv', layer_format='f32')
    assert sorted(got) == sorted(want)
    for key in want:
        assert torch.equal(_bits(got[key]), _bits(want[key])), key
    # the stack has the cube's shape and goes into the viewer
    assert tuple(got['rgba_layers'].shape) == (6 * b, s, s, d, 4)
    pose = np.tile(np.eye(4, dtype=F)[None, None], (b, 2, 1, 1))
    pos = np.zeros((b, 2, 3), F)
    pos[:, 1, 0] = 0.1
    rgb, dep = m.cube_render_views(got['rgba_layers'], pose, pos, planes, size=(16, 32))
    assert tuple(rgb.shape) == (b, 2, 16, 32, 3) and bool(torch.isfinite(rgb).all()) and float(rgb.abs().max()) > 0
    # 'face' is the default and is today's composition, bit for bit
    src_faces = m.equirect_to_cube(src, s, k).reshape(6 * b, s, s, 3)
    eye = torch.eye(4, dtype=torch.float32, device=m.device).expand(6 * b, 4, 4).contiguous()
    old_input = m.format_network_input(ref_faces, src_faces, eye, face_src, planes, kf, ref_pose_inv=eye)
    old = m.infer_layers(old_input, d, ngf, 'blend_weights alphas', 'blend_psv', layer_format='f32')
    for kw in (dict(), dict(src_sampling='face')):
        face = m.infer_cube(raw_src, raw_ref, x["src_pose"], s, planes, ngf=ngf, extra_outputs='blend_weights alphas', **kw)
        for key in old:
            assert torch.equal(_bits(face[key]), _bits(old[key])), key
    # the two modes differ (the source half does, past the borders), and nothing else is a mode
    assert not torch.equal(_bits(net_input[..., 3 * d:]), _bits(old_input[..., 3 * d:]))
    assert torch.equal(_bits(net_input[..., :3 * d]), _bits(old_input[..., :3 * d]))
    with pytest.raises(ValueError, match="src_sampling"):
        m.infer_cube(raw_src, raw_ref, x["src_pose"], s, planes, ngf=ngf, src_sampling='edge')
