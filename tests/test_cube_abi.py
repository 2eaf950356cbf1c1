"""CPU-only checks of the cube-map viewer's plumbing: msi_cube_render_views and msi_equirect_to_cube_f32 are exported and bound
with the signatures the header declares (ABI still 9: new entry points change no existing signature), their argument checks
reject bad calls with the documented code before any launch, and the shape rules and the host-side domain guard of
MSI.cube_render_views (matryodshka_amd.cubemap) raise without a device.  No kernel is launched here: every native call below
fails its validation, or has an empty batch, before it could reach a device (the dummy pointers are never dereferenced)."""
import numpy as np
import pytest

from tests.util import check_binding

MSI_E_BADARG, MSI_E_UNSUPPORTED = -1, -3
F32, RGBA8, RGBA16F = 0, 1, 2
EQUIRECT, PINHOLE = 0, 1

NAMES = {
    "msi_cube_render_views": ["layers", "format", "tgt_pose_rt", "tgt_pos", "tgt_intrinsics", "stack_intrinsics", "depths", "trig",
                              "batch", "views", "face_size", "num_planes", "camera", "out_height", "out_width", "out_rgb",
                              "out_depth", "status_device", "stream"],
    "msi_equirect_to_cube_f32": ["image", "intrinsics", "batch", "height", "width", "channels", "face_size", "out", "stream"],
}


@pytest.mark.parametrize("name", sorted(NAMES))
def test_exported_and_bound(native_lib, name):
    assert name in native_lib.SIGNATURES
    assert hasattr(native_lib.lib, name)
    assert native_lib.MSI_ABI_VERSION == 9
    assert native_lib.lib.msi_abi_version() == 9


@pytest.mark.parametrize("name", sorted(NAMES))
def test_header_and_binding_agree_on_the_signature(native_lib, name):
    assert check_binding(native_lib, name, int32_and_pointers=True) == NAMES[name]


def test_the_unit_is_a_geometry_unit():
    from matryodshka_amd import build
    assert "geo_cube.hip" in build.GEO_UNITS
    flags = dict(build.SOURCES)["geo_cube.hip"]
    assert "-ffp-contract=off" in flags and "-fno-slp-vectorize" in flags


# ------------------------------------------------------------------------------------------------ msi_cube_render_views
def _ptrs():
    # layers, tgt_pose_rt, tgt_pos, tgt_intrinsics, stack_intrinsics, depths, trig, out_rgb, out_depth, status
    return [4096 * (k + 1) for k in range(10)]


def _call(lib, ptrs, fmt=F32, batch=2, views=3, face_size=16, num_planes=4, camera=EQUIRECT, out_height=16, out_width=32):
    layers, pose, pos, intr, ks, depths, trig, out_rgb, out_depth, status = ptrs
    return lib.msi_cube_render_views(layers, fmt, pose, pos, intr, ks, depths, trig, batch, views, face_size, num_planes, camera,
                                     out_height, out_width, out_rgb, out_depth, status, None)


def _rejects(native_lib, what=None, code=MSI_E_BADARG, **kw):
    ptrs = _ptrs()
    for k, v in (what or {}).items():
        ptrs[k] = v
    assert _call(native_lib.lib, ptrs, **kw) == code
    msg = native_lib.last_error()
    assert "cube_render_views" in msg
    return msg


@pytest.mark.parametrize("fmt", [F32, RGBA8, RGBA16F])
@pytest.mark.parametrize("null", [0, 1, 2, 4, 5])
def test_rejects_null_inputs(native_lib, fmt, null):
    assert "null pointer" in _rejects(native_lib, {null: None}, fmt=fmt)


def test_each_camera_needs_its_own_table(native_lib):
    assert "trig" in _rejects(native_lib, {6: None}, camera=EQUIRECT)
    assert "intrinsics" in _rejects(native_lib, {3: None}, camera=PINHOLE)
    ptrs = _ptrs(); ptrs[3] = None
    assert _call(native_lib.lib, ptrs, camera=EQUIRECT, batch=0) == 0       # (and not the other camera's)
    ptrs = _ptrs(); ptrs[6] = None
    assert _call(native_lib.lib, ptrs, camera=PINHOLE, batch=0) == 0


def test_rejects_both_outputs_null(native_lib):
    assert "both outputs are NULL" in _rejects(native_lib, {7: None, 8: None})


@pytest.mark.parametrize("views", [0, -1])
def test_rejects_views_below_one(native_lib, views):
    assert "views" in _rejects(native_lib, views=views)


@pytest.mark.parametrize("kw", [dict(out_height=0), dict(out_width=0), dict(out_height=-4), dict(camera=PINHOLE, out_height=1),
                                dict(camera=PINHOLE, out_width=1)])
def test_rejects_a_bad_output_size(native_lib, kw):
    assert "output size" in _rejects(native_lib, **kw)


@pytest.mark.parametrize("dims", [dict(face_size=0), dict(num_planes=0), dict(batch=-1), dict(face_size=-3)])
def test_rejects_bad_dims(native_lib, dims):
    assert "bad dims" in _rejects(native_lib, **dims)


@pytest.mark.parametrize("fmt", [3, -1, 16])
def test_rejects_an_unknown_format(native_lib, fmt):
    assert "unknown format" in _rejects(native_lib, fmt=fmt)


@pytest.mark.parametrize("camera", [2, -1])
def test_rejects_an_unknown_camera(native_lib, camera):
    assert "unknown camera" in _rejects(native_lib, camera=camera)


def test_rejects_129_planes_as_unsupported(native_lib):
    assert "at most 128 planes" in _rejects(native_lib, code=MSI_E_UNSUPPORTED, num_planes=129)
    assert _call(native_lib.lib, _ptrs(), batch=0, num_planes=128) == 0


@pytest.mark.parametrize("fmt,face,planes,ok", [
    (F32, 1024, 21, True), (F32, 1024, 22, False),      # 6 * 21 * 2^20 * 16 = 2016 * 2^20 < 2^31 <= 2112 * 2^20
    (RGBA16F, 1024, 42, True), (RGBA16F, 1024, 43, False),
    (RGBA8, 1024, 85, True), (RGBA8, 1024, 86, False),
    (F32, 40000, 1, False),
])
def test_refuses_a_sample_its_32_bit_offsets_cannot_cover(native_lib, fmt, face, planes, ok):
    """The per-lane byte offset spans a sample's six face stacks: 6 D S^2 texel_bytes must stay below 2^31."""
    texel = {F32: 16, RGBA16F: 8, RGBA8: 4}[fmt]
    assert (6 * planes * face * face * texel < 2 ** 31) == ok
    if ok:
        assert _call(native_lib.lib, _ptrs(), fmt=fmt, batch=0, face_size=face, num_planes=planes) == 0
    else:
        assert "2^31 bytes" in _rejects(native_lib, fmt=fmt, face_size=face, num_planes=planes)


@pytest.mark.parametrize("kw", [dict(out_height=1 << 30, out_width=1 << 14),
                                dict(views=1 << 20, out_height=1 << 12, out_width=1 << 12),
                                dict(batch=1 << 20, views=1 << 8, out_height=1 << 11, out_width=1 << 10)])
def test_rejects_grid_overflow(native_lib, kw):
    assert "too many target pixels" in _rejects(native_lib, **kw)


@pytest.mark.parametrize("fmt", [F32, RGBA8, RGBA16F])
@pytest.mark.parametrize("camera", [EQUIRECT, PINHOLE])
def test_a_valid_empty_batch_passes_validation(native_lib, fmt, camera):
    assert _call(native_lib.lib, _ptrs(), fmt=fmt, camera=camera, batch=0) == 0
    for out in (7, 8, 9):       # either output alone; no status word
        ptrs = _ptrs()
        ptrs[out] = None
        assert _call(native_lib.lib, ptrs, fmt=fmt, camera=camera, batch=0) == 0


# --------------------------------------------------------------------------------------------- msi_equirect_to_cube_f32
def _e2c(lib, image=4096, intr=8192, batch=2, height=16, width=32, channels=3, face_size=8, out=12288):
    return lib.msi_equirect_to_cube_f32(image, intr, batch, height, width, channels, face_size, out, None)


@pytest.mark.parametrize("kw,text", [(dict(image=None), "null pointer"), (dict(intr=None), "null pointer"), (dict(out=None), "null pointer"),
                                     (dict(batch=-1), "bad dims"), (dict(height=0), "bad dims"), (dict(width=0), "bad dims"),
                                     (dict(face_size=0), "bad dims"), (dict(channels=0), "channels"), (dict(channels=5), "channels"),
                                     (dict(height=4096, width=4096), "2^24"), (dict(face_size=4096), "4096")])
def test_equirect_to_cube_rejects(native_lib, kw, text):
    assert _e2c(native_lib.lib, **kw) == MSI_E_BADARG
    msg = native_lib.last_error()
    assert "equirect_to_cube" in msg and text in msg


@pytest.mark.parametrize("channels", [1, 2, 3, 4])
def test_equirect_to_cube_accepts_an_empty_batch(native_lib, channels):
    assert _e2c(native_lib.lib, batch=0, channels=channels) == 0


# ------------------------------------------------------------------- the Python layer's rules that need no device
def _shapes(stack=(12, 4, 16, 16, 4), pose=(2, 3, 4, 4), pos=(2, 3, 3), size=(8, 16)):
    from matryodshka_amd import cubemap
    return cubemap.cube_view_shapes(stack, pose, pos, size)


def test_shape_rules_accept_the_documented_shapes():
    assert _shapes() == (2, 3, 16, 4, 8, 16)
    assert _shapes(stack=(6, 4, 16, 16, 4), pose=(3, 4, 4), pos=(3, 3)) == (1, 3, 16, 4, 8, 16)     # B = 1 takes [V,4,4] / [V,3]


@pytest.mark.parametrize("kw", [dict(stack=(10, 4, 16, 16, 4)),            # not a multiple of 6
                                dict(stack=(0, 4, 16, 16, 4)),
                                dict(stack=(12, 4, 16, 18, 4)),            # faces are square
                                dict(stack=(12, 4, 16, 16)),
                                dict(size=None),                            # required for both cameras
                                dict(pose=(1, 3, 4, 4)),                    # pose batch 1, two cubes
                                dict(pose=(3, 4, 4), pos=(3, 3)),           # [V,4,4] with B = 2
                                dict(pose=(2, 3, 3, 4)),
                                dict(pos=(2, 2, 3)), dict(pos=(2, 3)), dict(pos=(6, 3))])
def test_shape_rules_raise_value_error(kw):
    with pytest.raises(ValueError):
        _shapes(**kw)


def test_the_host_side_guard_wants_the_origin_strictly_inside_the_innermost_shell():
    from matryodshka_amd import cubemap
    planes = [100.0, 10.0, 3.0, 1.0]
    eye = np.tile(np.eye(4, dtype=np.float32), (3, 1, 1))
    inside = np.array([[0, 0, 0], [0.9, -0.9, 0.9], [0.99, 0, 0]], np.float32)       # |o| = 1.56 for the second: a CUBE, not a sphere
    cubemap.check_origin_inside(inside, eye, planes)
    for bad in ([1.0, 0, 0], [0, -1.5, 0], [0, 0, np.nan]):
        pos = inside.copy()
        pos[1] = bad
        with pytest.raises(ValueError):
            cubemap.check_origin_inside(pos, eye, planes)
    shifted = eye.copy()
    shifted[2, 1, 3] = 0.5                       # the pose's translation counts: (0, 0.5 + 0.6, 0)
    with pytest.raises(ValueError):
        cubemap.check_origin_inside(np.array([[0, 0, 0], [0, 0, 0], [0, 0.6, 0]], np.float32), shifted, planes)
    cubemap.check_origin_inside(np.array([[0, 0, 0], [0, 0, 0], [0, 0.4, 0]], np.float32), shifted, planes)
