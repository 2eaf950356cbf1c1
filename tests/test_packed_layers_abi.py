"""CPU-only checks of the compact-stack entry points: msi_pack_layers, msi_unpack_layers and msi_render_views_packed are
exported and bound (ABI still 9: new entry points change no existing signature), and their argument checks reject bad calls
with MSI_E_BADARG and a message that names the entry point, before any launch.  No kernel is launched here: every call
below fails its validation or has nothing to do (the non-zero dummy pointers are never dereferenced)."""
import pytest

MSI_E_BADARG = -1
EQUIRECT, PINHOLE = 0, 1
F32, RGBA8, RGBA16F = 0, 1, 2


def test_symbols_are_exported_and_bound(native_lib):
    for name in ("msi_pack_layers", "msi_unpack_layers", "msi_render_views_packed"):
        assert name in native_lib.SIGNATURES
        assert hasattr(native_lib.lib, name)
    assert (native_lib.MSI_LAYERS_F32, native_lib.MSI_LAYERS_RGBA8, native_lib.MSI_LAYERS_RGBA16F) == (F32, RGBA8, RGBA16F)
    assert native_lib.MSI_ABI_VERSION == 9
    assert native_lib.lib.msi_abi_version() == 9


def test_header_defines_the_format_constants():
    import re
    from tests.util import header_text
    header = header_text()
    for name, value in (("MSI_LAYERS_F32", 0), ("MSI_LAYERS_RGBA8", 1), ("MSI_LAYERS_RGBA16F", 2), ("MSI_ABI_VERSION", 9)):
        assert re.search(r"#define\s+%s\s+%d\b" % (name, value), header), name


# ---- pack / unpack -----------------------------------------------------------------------------------------------------
def _pack(lib, src=4096, fmt=RGBA8, dst=8192, texels=64):
    return lib.msi_pack_layers(src, fmt, dst, texels, None)


def _unpack(lib, src=4096, fmt=RGBA8, dst=8192, texels=64):
    return lib.msi_unpack_layers(src, fmt, dst, texels, None)


CONVERTERS = [("pack_layers", _pack), ("unpack_layers", _unpack)]


def _bad(native_lib, name, fn, **kw):
    assert fn(native_lib.lib, **kw) == MSI_E_BADARG
    msg = native_lib.last_error()
    assert name in msg, msg
    return msg


@pytest.mark.parametrize("name,fn", CONVERTERS)
@pytest.mark.parametrize("null", ["src", "dst"])
@pytest.mark.parametrize("fmt", [RGBA8, RGBA16F])
def test_converters_reject_null_pointers(native_lib, name, fn, null, fmt):
    assert "null pointer" in _bad(native_lib, name, fn, fmt=fmt, **{null: None})


@pytest.mark.parametrize("name,fn", CONVERTERS)
@pytest.mark.parametrize("fmt", [3, -1, 255])
def test_converters_reject_unknown_formats(native_lib, name, fn, fmt):
    assert "unknown format" in _bad(native_lib, name, fn, fmt=fmt)


@pytest.mark.parametrize("name,fn", CONVERTERS)
def test_converters_reject_f32(native_lib, name, fn):
    assert "MSI_LAYERS_F32" in _bad(native_lib, name, fn, fmt=F32)


@pytest.mark.parametrize("name,fn", CONVERTERS)
@pytest.mark.parametrize("texels", [-1, -(1 << 40)])
def test_converters_reject_negative_texels(native_lib, name, fn, texels):
    assert "negative" in _bad(native_lib, name, fn, texels=texels)


@pytest.mark.parametrize("name,fn", CONVERTERS)
@pytest.mark.parametrize("fmt", [RGBA8, RGBA16F])
def test_zero_texels_pass_validation(native_lib, name, fn, fmt):
    """Control: the same arguments with nothing wrong and no texels are accepted (nothing to launch)."""
    assert fn(native_lib.lib, fmt=fmt, texels=0) == 0


# ---- msi_render_views_packed: every rejection of msi_render_views_f32 (tests/test_render_views_abi.py), per format --------
def _ptrs():
    # layers, pose, pos, intrinsics, depths, trig, out_rgb, out_depth, status
    return [4096 * (k + 1) for k in range(9)]


def _call(lib, ptrs, fmt=RGBA8, batch=2, views=3, height=16, width=32, num_planes=4, camera=EQUIRECT, out_height=16, out_width=32):
    layers, pose, pos, intr, depths, trig, out_rgb, out_depth, status = ptrs
    return lib.msi_render_views_packed(layers, fmt, pose, pos, intr, depths, trig, batch, views, height, width, num_planes, camera,
                                       out_height, out_width, out_rgb, out_depth, status, None)


def _rejects(native_lib, what=None, **kw):
    ptrs = _ptrs()
    for k, v in (what or {}).items():
        ptrs[k] = v
    assert _call(native_lib.lib, ptrs, **kw) == MSI_E_BADARG
    msg = native_lib.last_error()
    assert "render_views_packed" in msg, msg
    return msg


FORMATS = [F32, RGBA8, RGBA16F]


@pytest.mark.parametrize("fmt", [3, -1, 100])
def test_views_reject_unknown_format(native_lib, fmt):
    assert "unknown format" in _rejects(native_lib, fmt=fmt)


@pytest.mark.parametrize("fmt", FORMATS)
@pytest.mark.parametrize("camera", [EQUIRECT, PINHOLE])
@pytest.mark.parametrize("null", [0, 1, 2, 4])
def test_views_reject_null_inputs(native_lib, fmt, camera, null):
    assert "null pointer" in _rejects(native_lib, {null: None}, fmt=fmt, camera=camera)


@pytest.mark.parametrize("fmt", FORMATS)
def test_views_reject_missing_camera_tables(native_lib, fmt):
    assert "null pointer" in _rejects(native_lib, {5: None}, fmt=fmt, camera=EQUIRECT)      # equirect needs trig
    assert "null pointer" in _rejects(native_lib, {3: None}, fmt=fmt, camera=PINHOLE)       # pinhole needs intrinsics


@pytest.mark.parametrize("fmt", FORMATS)
def test_views_reject_both_outputs_null(native_lib, fmt):
    assert "both outputs are NULL" in _rejects(native_lib, {6: None, 7: None}, fmt=fmt)


@pytest.mark.parametrize("fmt", FORMATS)
@pytest.mark.parametrize("views", [0, -1])
def test_views_reject_views_below_one(native_lib, fmt, views):
    assert "views" in _rejects(native_lib, fmt=fmt, views=views)


@pytest.mark.parametrize("fmt", FORMATS)
@pytest.mark.parametrize("camera,oh,ow", [(EQUIRECT, 0, 32), (EQUIRECT, 16, 0), (EQUIRECT, -4, 8),
                                          (PINHOLE, 1, 32), (PINHOLE, 16, 1), (PINHOLE, 0, 0)])
def test_views_reject_bad_output_size(native_lib, fmt, camera, oh, ow):
    assert "output size" in _rejects(native_lib, fmt=fmt, camera=camera, out_height=oh, out_width=ow)


@pytest.mark.parametrize("fmt", FORMATS)
@pytest.mark.parametrize("camera", [2, -1, 7])
def test_views_reject_unknown_camera(native_lib, fmt, camera):
    assert "camera" in _rejects(native_lib, fmt=fmt, camera=camera)


@pytest.mark.parametrize("fmt", FORMATS)
@pytest.mark.parametrize("dims", [dict(height=0), dict(width=0), dict(num_planes=0), dict(batch=-1)])
def test_views_reject_bad_dims(native_lib, fmt, dims):
    assert "bad dims" in _rejects(native_lib, fmt=fmt, **dims)


@pytest.mark.parametrize("fmt", FORMATS)
def test_views_reject_stacks_of_2_24_texels(native_lib, fmt):
    assert "2^24" in _rejects(native_lib, fmt=fmt, height=4096, width=4096)


@pytest.mark.parametrize("fmt", FORMATS)
@pytest.mark.parametrize("kw", [dict(out_height=1 << 30, out_width=1 << 12),                 # one view alone
                                dict(views=1 << 20, out_height=1 << 12, out_width=1 << 12),  # the views
                                dict(batch=1 << 20, views=1 << 8, out_height=1 << 10, out_width=1 << 10),
                                dict(batch=1 << 30, views=1 << 30, out_height=1 << 30, out_width=1 << 30)])
def test_views_reject_grid_overflow(native_lib, fmt, kw):
    assert "too many target pixels" in _rejects(native_lib, fmt=fmt, **kw)


@pytest.mark.parametrize("fmt", FORMATS)
def test_a_valid_empty_batch_passes_validation(native_lib, fmt):
    """Control for the cases above: the same arguments with nothing wrong and B = 0 are accepted (nothing to launch)."""
    for camera in (EQUIRECT, PINHOLE):
        assert _call(native_lib.lib, _ptrs(), fmt=fmt, batch=0, camera=camera) == 0


def test_the_f32_entry_point_still_names_itself(native_lib):
    """msi_render_views_f32 shares the checks: its messages keep naming render_views, not the packed entry point."""
    p = _ptrs()
    assert native_lib.lib.msi_render_views_f32(p[0], p[1], p[2], p[3], p[4], p[5], 2, 0, 16, 32, 4, EQUIRECT, 16, 32, p[6], p[7],
                                               p[8], None) == MSI_E_BADARG
    msg = native_lib.last_error()
    assert msg.startswith("render_views:") or "render_views:" in msg
    assert "render_views_packed" not in msg
