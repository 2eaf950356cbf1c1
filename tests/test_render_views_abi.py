"""CPU-only checks of the many-views render's plumbing: msi_render_views_f32 is exported and bound (ABI still 9: a new
entry point changes no existing signature), and its argument checks reject bad calls with MSI_E_BADARG before any launch.
No kernel is launched here: every call below fails its validation before it could reach a device (the non-zero dummy
pointers are never dereferenced)."""
import pytest

MSI_E_BADARG = -1
EQUIRECT, PINHOLE = 0, 1


def test_render_views_is_exported_and_bound(native_lib):
    assert "msi_render_views_f32" in native_lib.SIGNATURES
    assert hasattr(native_lib.lib, "msi_render_views_f32")
    assert (native_lib.MSI_CAMERA_EQUIRECT, native_lib.MSI_CAMERA_PINHOLE) == (EQUIRECT, PINHOLE)
    assert native_lib.MSI_ABI_VERSION == 9
    assert native_lib.lib.msi_abi_version() == 9


def _ptrs():
    # rgba, pose, pos, intrinsics, depths, trig, out_rgb, out_depth, status
    return [4096 * (k + 1) for k in range(9)]


def _call(lib, ptrs, batch=2, views=3, height=16, width=32, num_planes=4, camera=EQUIRECT, out_height=16, out_width=32):
    rgba, pose, pos, intr, depths, trig, out_rgb, out_depth, status = ptrs
    return lib.msi_render_views_f32(rgba, pose, pos, intr, depths, trig, batch, views, height, width, num_planes, camera,
                                    out_height, out_width, out_rgb, out_depth, status, None)


def _rejects(native_lib, what=None, **kw):
    ptrs = _ptrs()
    for k, v in (what or {}).items():
        ptrs[k] = v
    assert _call(native_lib.lib, ptrs, **kw) == MSI_E_BADARG
    msg = native_lib.last_error()
    assert "render_views" in msg
    return msg


@pytest.mark.parametrize("camera", [EQUIRECT, PINHOLE])
@pytest.mark.parametrize("null", [0, 1, 2, 4])
def test_rejects_null_inputs(native_lib, camera, null):
    assert "null pointer" in _rejects(native_lib, {null: None}, camera=camera)


def test_rejects_missing_camera_tables(native_lib):
    assert "null pointer" in _rejects(native_lib, {5: None}, camera=EQUIRECT)      # equirect needs trig
    assert "null pointer" in _rejects(native_lib, {3: None}, camera=PINHOLE)       # pinhole needs intrinsics


def test_rejects_both_outputs_null(native_lib):
    assert "both outputs are NULL" in _rejects(native_lib, {6: None, 7: None})


@pytest.mark.parametrize("views", [0, -1])
def test_rejects_views_below_one(native_lib, views):
    assert "views" in _rejects(native_lib, views=views)


@pytest.mark.parametrize("camera,oh,ow", [(EQUIRECT, 0, 32), (EQUIRECT, 16, 0), (EQUIRECT, -4, 8),
                                          (PINHOLE, 1, 32), (PINHOLE, 16, 1), (PINHOLE, 0, 0)])
def test_rejects_bad_output_size(native_lib, camera, oh, ow):
    assert "output size" in _rejects(native_lib, camera=camera, out_height=oh, out_width=ow)


@pytest.mark.parametrize("camera", [2, -1, 7])
def test_rejects_unknown_camera(native_lib, camera):
    assert "camera" in _rejects(native_lib, camera=camera)


@pytest.mark.parametrize("dims", [dict(height=0), dict(width=0), dict(num_planes=0), dict(batch=-1)])
def test_rejects_bad_dims(native_lib, dims):
    assert "bad dims" in _rejects(native_lib, **dims)


def test_rejects_stacks_of_2_24_texels(native_lib):
    assert "2^24" in _rejects(native_lib, height=4096, width=4096)


@pytest.mark.parametrize("kw", [dict(out_height=1 << 30, out_width=1 << 12),                 # one view alone
                                dict(views=1 << 20, out_height=1 << 12, out_width=1 << 12),  # the views
                                dict(batch=1 << 20, views=1 << 8, out_height=1 << 10, out_width=1 << 10),
                                dict(batch=1 << 30, views=1 << 30, out_height=1 << 30, out_width=1 << 30)])
def test_rejects_grid_overflow(native_lib, kw):
    assert "too many target pixels" in _rejects(native_lib, **kw)


def test_a_valid_empty_batch_passes_validation(native_lib):
    """Control for the cases above: the same arguments with nothing wrong and B = 0 are accepted (nothing to launch)."""
    for camera in (EQUIRECT, PINHOLE):
        assert _call(native_lib.lib, _ptrs(), batch=0, camera=camera) == 0
