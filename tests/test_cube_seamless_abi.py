"""CPU-only checks of msi_cube_render_views_seamless' plumbing, as tests/test_cube_abi.py does them for msi_cube_render_views: the
entry point is exported and bound with the signature the header declares -- the argument list of msi_cube_render_views, ABI still
9 -- and its argument checks reject bad calls with that entry point's codes before any launch.  No kernel is launched here: every
call fails its validation, or has an empty batch (the dummy pointers are never dereferenced).  The Python layer's rules that need
no device are here too."""
import pytest

from tests.util import check_binding

MSI_E_BADARG, MSI_E_UNSUPPORTED = -1, -3
F32, RGBA8, RGBA16F = 0, 1, 2
EQUIRECT, PINHOLE = 0, 1
NAME = "msi_cube_render_views_seamless"


def test_exported_and_bound(native_lib):
    assert NAME in native_lib.SIGNATURES
    assert hasattr(native_lib.lib, NAME)
    assert native_lib.MSI_ABI_VERSION == 9 and native_lib.lib.msi_abi_version() == 9
    assert native_lib.RENDER_STATUS_NOT_CUBE_CAMERA == 2 and native_lib.RENDER_STATUS_ORIGIN_OUTSIDE == 1


def test_it_takes_the_argument_list_of_msi_cube_render_views(native_lib):
    names = check_binding(native_lib, NAME, int32_and_pointers=True)
    assert names == check_binding(native_lib, "msi_cube_render_views", int32_and_pointers=True)
    assert native_lib.SIGNATURES[NAME] == native_lib.SIGNATURES["msi_cube_render_views"]


def test_the_header_names_the_status_bit_and_the_addition():
    import os
    text = open(os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "include", "msi_hip.h")).read()
    assert "#define MSI_RENDER_STATUS_NOT_CUBE_CAMERA 2" in text
    assert text.index("additions since, no bump") < text.index(NAME) < text.index("#define MSI_ABI_VERSION 9")


def _ptrs():
    # layers, tgt_pose_rt, tgt_pos, tgt_intrinsics, stack_intrinsics, depths, trig, out_rgb, out_depth, status
    return [4096 * (k + 1) for k in range(10)]


def _call(lib, ptrs, entry=NAME, fmt=F32, batch=2, views=3, face_size=16, num_planes=4, camera=EQUIRECT, out_height=16, out_width=32):
    layers, pose, pos, intr, ks, depths, trig, out_rgb, out_depth, status = ptrs
    return getattr(lib, entry)(layers, fmt, pose, pos, intr, ks, depths, trig, batch, views, face_size, num_planes, camera,
                               out_height, out_width, out_rgb, out_depth, status, None)


def _rejects(native_lib, what=None, code=MSI_E_BADARG, **kw):
    """Both entry points refuse the call with the same code; returns the seamless one's message."""
    ptrs = _ptrs()
    for k, v in (what or {}).items():
        ptrs[k] = v
    assert _call(native_lib.lib, ptrs, entry="msi_cube_render_views", **kw) == code
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
    assert _call(native_lib.lib, ptrs, camera=EQUIRECT, batch=0) == 0
    ptrs = _ptrs(); ptrs[6] = None
    assert _call(native_lib.lib, ptrs, camera=PINHOLE, batch=0) == 0


@pytest.mark.parametrize("kw,text", [
    (dict(what={7: None, 8: None}), "both outputs are NULL"),
    (dict(views=0), "views"), (dict(views=-1), "views"),
    (dict(out_height=0), "output size"), (dict(out_width=0), "output size"), (dict(camera=PINHOLE, out_height=1), "output size"),
    (dict(face_size=0), "bad dims"), (dict(num_planes=0), "bad dims"), (dict(batch=-1), "bad dims"),
    (dict(fmt=3), "unknown format"), (dict(fmt=-1), "unknown format"),
    (dict(camera=2), "unknown camera"), (dict(camera=-1), "unknown camera"),
    (dict(fmt=F32, face_size=1024, num_planes=22), "2^31 bytes"), (dict(fmt=RGBA8, face_size=1024, num_planes=86), "2^31 bytes"),
    (dict(face_size=40000, num_planes=1), "2^31 bytes"),
    (dict(out_height=1 << 30, out_width=1 << 14), "too many target pixels"),
])
def test_rejects_bad_arguments_with_the_clamp_entry_points_codes(native_lib, kw, text):
    kw = dict(kw)
    assert text in _rejects(native_lib, kw.pop("what", None), **kw)


def test_rejects_129_planes_as_unsupported(native_lib):
    assert "at most 128 planes" in _rejects(native_lib, code=MSI_E_UNSUPPORTED, num_planes=129)
    assert _call(native_lib.lib, _ptrs(), batch=0, num_planes=128) == 0


@pytest.mark.parametrize("fmt", [F32, RGBA8, RGBA16F])
@pytest.mark.parametrize("camera", [EQUIRECT, PINHOLE])
def test_a_valid_empty_batch_passes_validation(native_lib, fmt, camera):
    assert _call(native_lib.lib, _ptrs(), fmt=fmt, camera=camera, batch=0) == 0
    for out in (7, 8, 9):       # either output alone; no status word
        ptrs = _ptrs()
        ptrs[out] = None
        assert _call(native_lib.lib, ptrs, fmt=fmt, camera=camera, batch=0) == 0
    assert _call(native_lib.lib, _ptrs(), fmt=fmt, camera=camera, batch=0, face_size=1024, num_planes=21 if fmt == F32 else 42) == 0


# ------------------------------------------------------------------- the Python layer's rules that need no device
def test_the_default_camera_is_the_only_cube_camera():
    import numpy as np
    from matryodshka_amd import cubemap
    k = cubemap.default_face_intrinsics(12)
    assert cubemap.is_default_face_intrinsics(k, 12) and cubemap.is_default_face_intrinsics(np.tile(k[None], (3, 1, 1)), 12)
    assert not cubemap.is_default_face_intrinsics(k, 16)
    for r, c in [(0, 0), (1, 1), (0, 2), (1, 2)]:
        bad = np.tile(k[None], (2, 1, 1))
        bad[1, r, c] = 5.5
        assert not cubemap.is_default_face_intrinsics(bad, 12)
    nan = k.copy()
    nan[0, 0] = np.nan
    assert not cubemap.is_default_face_intrinsics(nan, 12)
