"""Every kernel form sweep_common (geo_sweep.hip) can launch in the default build, run through the C ABI at shapes of a few thousand pixels: the cases of
tests/sweep_cases.py, which tests/test_sweep_cases_cpu.py shows to reach all 26 forms, to stage patches in the LDS form, to contain the seam / wrap /
invalid samples they are there for, and whose comparisons it shows to fail on the faults they are there for.

Per case: the fp32 double volume against the oracle (max-abs 1e-3, 99.99th percentile 1e-4 from 1e5 values on: _compare of tests/test_gpu_render_views.py;
the MAXIMUM -- these poses are translations, one op order up to the discriminant, no isolated branch flips); the double volume against the two single-source
entry points and against every frame swept alone, bit for bit, in fp32 and bf16; the bf16 volume against the rounded fp32 volume, bit for bit.  Every
output buffer is prefilled with a sentinel.  Then the fp32 perspective sweep against the oracle at the shapes where tests/test_gpu_pp_bf16.py uses it as
the reference of the bf16 volume.  Run with -s for the per-case record kept in profiles/sweep_forms.txt."""
import functools

import numpy as np
import pytest

from tests import sweep_cases as SC

pytestmark = pytest.mark.gpu

IDS = [c["name"] for c in SC.CASES]
SENTINEL = 7.0          # exact in bf16; no sweep value reaches it (images in [-1, 1], convex weights)


@pytest.fixture(scope="module")
def gpu():
    import torch
    assert torch.cuda.is_available(), "GPU tests need a HIP device"
    from matryodshka_amd import MSI, _native as N
    return torch, MSI(), N


def _volume(N, t, b, h, w, d, out, bf16, lo=0):
    """msi_ods_sweep_volume of frames [lo, lo + b) into out."""
    N.check(N.lib.msi_ods_sweep_volume(t["ref"][lo:].data_ptr(), t["src"][lo:].data_ptr(), t["pose0"][lo:].data_ptr(), t["pose1"][lo:].data_ptr(),
                                       t["intr"][lo:].data_ptr(), t["depths"].data_ptr(), t["trig"].data_ptr(), b, h, w, d, out.data_ptr(), int(bf16), None),
            "msi_ods_sweep_volume")


def _single(N, t, source, b, h, w, d, out, bf16, channels, coff):
    fn = N.lib.msi_ods_sphere_sweep_bf16 if bf16 else N.lib.msi_ods_sphere_sweep_f32
    img, pose, order = ((t["ref"], t["pose0"], 1), (t["src"], t["pose1"], -1))[source]
    N.check(fn(img.data_ptr(), pose.data_ptr(), t["intr"].data_ptr(), t["depths"].data_ptr(), t["trig"].data_ptr(), b, h, w, d, order,
               out.data_ptr(), channels, coff, None), "msi_ods_sphere_sweep")


@functools.lru_cache(maxsize=None)
def _run(name):
    """Every launch of a case, once: {(what, bf16): volume} for what in volume / single / alone, the device inputs, and the oracle's volume."""
    import torch
    from matryodshka_amd import MSI, _native as N
    case = SC.case_by_name(name)
    b, h, w, d = case["b"], case["h"], case["w"], case["d"]
    inp = SC.case_inputs(case)
    t = {k: torch.from_numpy(v).cuda() for k, v in inp.items()}
    t["trig"] = MSI()._trig(h, w)
    out = {}
    for bf16 in (False, True):
        dt = torch.bfloat16 if bf16 else torch.float32
        for what in ("volume", "single", "alone"):
            out[what, bf16] = torch.full((b, h, w, 6 * d), SENTINEL, dtype=dt, device="cuda")
        _volume(N, t, b, h, w, d, out["volume", bf16], bf16)
        for source in (0, 1):
            _single(N, t, source, b, h, w, d, out["single", bf16], bf16, 6 * d, source * 3 * d)
        for k in range(b):
            _volume(N, t, 1, h, w, d, out["alone", bf16][k:k + 1], bf16, lo=k)
    torch.cuda.synchronize()
    return case, inp, t, out


@functools.lru_cache(maxsize=None)
def _oracle(name):
    vol = SC.oracle_volume(SC.case_inputs(SC.case_by_name(name)))
    vol.setflags(write=False)
    return vol


def _bits(torch, x):
    return x.view(torch.int16) if x.dtype == torch.bfloat16 else x.view(torch.int32)


@pytest.mark.parametrize("name", IDS)
def test_fp32_volume_matches_the_oracle(gpu, name):
    torch, m, N = gpu
    case, inp, t, out = _run(name)
    got = out["volume", False].cpu().numpy()
    mx, pct = SC.errors_f32(got, _oracle(name))
    forms = "  ".join("%s b=%d %s: %s" % (what, nb, "bf16" if bf16 else "f32", "/".join(str(x) for x in SC.sweep_form(nb, case["h"], case["w"], case["d"], pair, bf16)[1:]))
                      for what, nb, pair, bf16 in SC.launches(case["b"], case["h"], case["w"], case["d"]) if not bf16)
    print("\n%-14s %s\n%-14s fp32 volume against the oracle: max-abs %.3e%s" % (name, forms, "", mx, "" if pct is None else "   99.99th percentile %.3e" % pct))
    assert not bool((out["volume", False] == SENTINEL).any())
    SC.compare_f32(got, _oracle(name), name)


@pytest.mark.parametrize("bf16", [False, True])
@pytest.mark.parametrize("name", IDS)
def test_volume_equals_the_single_source_sweeps_and_every_frame_alone(gpu, name, bf16):
    torch, m, N = gpu
    case, inp, t, out = _run(name)
    both, two, alone = (_bits(torch, out[what, bf16]) for what in ("volume", "single", "alone"))
    for what in ("volume", "single", "alone"):
        assert not bool((out[what, bf16] == SENTINEL).any()), what
    assert torch.equal(both, two), int((both != two).sum())
    assert torch.equal(both, alone), [k for k in range(case["b"]) if not torch.equal(both[k], alone[k])]
    if case["b"] > 1 and case["frames"][0] == case["frames"][1]:
        assert not torch.equal(both[0], both[1])                    # (equal settings, different images)


@pytest.mark.parametrize("name", IDS)
def test_bf16_volume_is_the_rounded_fp32_volume(gpu, name):
    torch, m, N = gpu
    case, inp, t, out = _run(name)
    got = out["volume", True].view(torch.int16)
    want = out["volume", False].to(torch.bfloat16).view(torch.int16)
    assert torch.equal(got, want), int((got != want).sum())
    assert SC.bf16_bits_differ(got.cpu().numpy(), out["volume", False].cpu().numpy()) == 0      # (the comparison the host test shows to see truncation)


@pytest.mark.parametrize("bf16", [False, True])
@pytest.mark.parametrize("name", SC.WINDOW_CASES)
def test_single_source_sweep_into_a_window_writes_nothing_else(gpu, name, bf16):
    """A single-source sweep into channels [2, 2 + 3D) of a volume of 3D + 5: the window is the plain sweep, bit for bit, and every other channel keeps the sentinel."""
    torch, m, N = gpu
    case, inp, t, out = _run(name)
    b, h, w, d = case["b"], case["h"], case["w"], case["d"]
    dt = torch.bfloat16 if bf16 else torch.float32
    for source in (0, 1):
        wide = torch.full((b, h, w, 3 * d + 5), SENTINEL, dtype=dt, device="cuda")
        plain = torch.full((b, h, w, 3 * d), SENTINEL, dtype=dt, device="cuda")
        _single(N, t, source, b, h, w, d, wide, bf16, 3 * d + 5, 2)
        _single(N, t, source, b, h, w, d, plain, bf16, 3 * d, 0)
        torch.cuda.synchronize()
        assert torch.equal(_bits(torch, wide[..., 2:2 + 3 * d].contiguous()), _bits(torch, plain)), source
        assert bool((wide[..., :2] == SENTINEL).all()) and bool((wide[..., 2 + 3 * d:] == SENTINEL).all()), source
        assert not bool((wide[..., 2:2 + 3 * d] == SENTINEL).any()), source
        assert torch.equal(_bits(torch, plain), _bits(torch, out["volume", bf16][..., source * 3 * d:(source + 1) * 3 * d].contiguous())), source


@pytest.mark.parametrize("bf16", [False, True])
def test_empty_batch_is_ok_and_writes_nothing(gpu, bf16):
    torch, m, N = gpu
    case, inp, t, out = _run("b1_8x32x4")
    h, w, d = case["h"], case["w"], case["d"]
    buf = torch.full((1, h, w, 6 * d), SENTINEL, dtype=torch.bfloat16 if bf16 else torch.float32, device="cuda")
    assert N.lib.msi_ods_sweep_volume(t["ref"].data_ptr(), t["src"].data_ptr(), t["pose0"].data_ptr(), t["pose1"].data_ptr(), t["intr"].data_ptr(),
                                      t["depths"].data_ptr(), t["trig"].data_ptr(), 0, h, w, d, buf.data_ptr(), int(bf16), None) == N.MSI_OK
    fn = N.lib.msi_ods_sphere_sweep_bf16 if bf16 else N.lib.msi_ods_sphere_sweep_f32
    for order, coff in ((1, 0), (-1, 3 * d)):
        assert fn(t["ref"].data_ptr(), t["pose0"].data_ptr(), t["intr"].data_ptr(), t["depths"].data_ptr(), t["trig"].data_ptr(), 0, h, w, d, order,
                  buf.data_ptr(), 6 * d, coff, None) == N.MSI_OK
    torch.cuda.synchronize()
    assert bool((buf == SENTINEL).all())


# ---- the fp32 perspective sweep: the reference of tests/test_gpu_pp_bf16.py's bf16 volume, against the oracle at that file's shapes below the full-size ones
def _pp_volumes(torch, case, d):
    from matryodshka_amd import MSI
    from oracle.msi import MSI as OracleMSI
    ref, src, K, eye, src_pose, interp_inv = case
    m, o = MSI(input_type="PP"), OracleMSI(input_type="PP")
    planes = m.inv_depths(1.0, 100.0, d)
    r, s = m.preprocess_image_pair(torch.from_numpy(ref), torch.from_numpy(src))
    got = m.format_network_input(r, s, eye, src_pose, planes, K, ref_pose_inv=interp_inv, dtype="f32")
    torch.cuda.synchronize()
    assert got.dtype == torch.float32
    want = o.format_network_input(o.preprocess_image(ref), o.preprocess_image(src), eye, src_pose, planes, K, ref_pose_inv=interp_inv)
    return got.cpu().numpy(), want


@pytest.mark.parametrize("b,h,w,d", [(2, 40, 50, 6), (3, 33, 47, 5), (2, 32, 64, 64), (3, 48, 96, 16), (2, 16, 64, 2)])
def test_fp32_pp_volume_matches_the_oracle(gpu, b, h, w, d):
    torch = gpu[0]
    from tests.test_gpu_pp_bf16 import _case
    got, want = _pp_volumes(torch, _case(100 + d, b, h, w), d)          # (the inputs of test_bf16_pp_volume_is_the_rounded_fp32_volume)
    assert got.shape == want.shape == (b, h, w, 6 * d)
    mx, pct = SC.errors_f32(got, want)
    print("\nPP (%d,%d,%d,%d) fp32 volume against the oracle: max-abs %.3e%s" % (b, h, w, d, mx, "" if pct is None else "   99.99th percentile %.3e" % pct))
    SC.compare_f32(got, want, (b, h, w, d))


def test_fp32_pp_volume_far_outside_the_face_matches_the_oracle(gpu):
    """The inputs of test_bf16_pp_volume_far_outside_the_face_is_the_rounded_fp32_volume (cameras turned by up to 3 rad and moved by up to 3 units).
    Held to the gates of every other case here, on the MAXIMUM: the pose product, apply_pose, K @ pose and the two divisions follow the oracle op for op in
    IEEE fp32, so the rotated cameras bring no flipped taps and the 99.9th-percentile gate of the posed fuzz frames is not needed (observed: 0 of 1572864
    elements differ from the oracle at all, here as at the five shapes above; profiles/sweep_forms.txt)."""
    torch = gpu[0]
    from tests.test_gpu_pp_bf16 import _case, _rot
    b, n, d = 4, 64, 16
    ref, src, K, eye, src_pose, interp_inv = _case(71, b, n, n)
    for k, (ang, t) in enumerate(((0.4, 0.5), (-0.7, -1.5), (1.2, 3.0), (3.0, 0.2))):
        src_pose[k, :3, :3] = _rot(0.3 * ang, ang, -0.5 * ang).astype(np.float32)
        src_pose[k, :3, 3] = (t, -0.5 * t, 0.25 * t)
    got, want = _pp_volumes(torch, (ref, src, K, eye, src_pose, np.tile(np.eye(4, dtype=np.float32)[None], (b, 1, 1))), d)
    err = np.abs(got.astype(np.float64) - want)
    print("\nPP far outside the face: max-abs %.3e   99.99th percentile %.3e   99.9th percentile %.3e   elements above 1e-3: %d of %d" % (
        err.max(), np.percentile(err, 99.99), np.percentile(err, 99.9), int((err > 1e-3).sum()), err.size))
    SC.compare_f32(got, want, "far outside the face")
