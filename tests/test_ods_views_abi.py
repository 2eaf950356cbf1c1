"""CPU-only checks of the ODS camera's plumbing: msi_render_ods_views is exported, bound and declared with one signature (ABI
still 9: a new entry point changes no existing signature), defined in exactly one unit -- a geometry unit --, and its argument
checks reject bad calls with the documented text before any launch.  The ODS camera is an entry point of its own: camera code 2
is still unknown to the three *_render_views functions.  No kernel is launched here: every native call below fails its
validation, or has an empty batch, before it could reach a device (the dummy pointers are never dereferenced)."""
import os
import re

import pytest

from tests.util import check_binding, header_text

MSI_E_BADARG = -1
F32, RGBA8, RGBA16F = 0, 1, 2
NAME = "msi_render_ods_views"
PARAMS = ["layers", "format", "tgt_pose_rt", "tgt_pos", "eye_radius", "depths", "trig", "batch", "views", "height", "width",
          "num_planes", "out_height", "out_width", "out_rgb", "out_depth", "status_device", "stream"]


def test_exported_and_bound(native_lib):
    assert NAME in native_lib.SIGNATURES
    assert hasattr(native_lib.lib, NAME)
    assert native_lib.MSI_ABI_VERSION == 9
    assert native_lib.lib.msi_abi_version() == 9


def test_header_and_binding_agree_on_the_signature(native_lib):
    assert "#define MSI_ABI_VERSION 9" in header_text()
    assert check_binding(native_lib, NAME, int32_and_pointers=True) == PARAMS


def test_defined_once_in_a_geometry_unit():
    from matryodshka_amd import build
    assert "geo_ods.hip" in build.GEO_UNITS
    flags = dict(build.SOURCES)["geo_ods.hip"]
    assert "-ffp-contract=off" in flags and "-fno-slp-vectorize" in flags
    pattern = re.compile(r"^int\s+%s\(" % NAME, re.M)
    hits = {}
    for unit in sorted(os.listdir(build.CSRC)):
        if unit.endswith((".hip", ".cpp")):
            with open(os.path.join(build.CSRC, unit)) as f:
                n = len(pattern.findall(f.read()))
            if n:
                hits[unit] = n
    assert hits == {"geo_ods.hip": 1}


# ------------------------------------------------------------------------------------------------ argument checks
def _ptrs():
    # layers, tgt_pose_rt, tgt_pos, eye_radius, depths, trig, out_rgb, out_depth, status
    return [4096 * (k + 1) for k in range(9)]


def _call(lib, ptrs, fmt=F32, batch=2, views=2, height=16, width=32, num_planes=4, out_height=16, out_width=32):
    layers, pose, pos, radius, depths, trig, out_rgb, out_depth, status = ptrs
    return lib.msi_render_ods_views(layers, fmt, pose, pos, radius, depths, trig, batch, views, height, width, num_planes,
                                    out_height, out_width, out_rgb, out_depth, status, None)


def _rejects(native_lib, what=None, **kw):
    ptrs = _ptrs()
    for k, v in (what or {}).items():
        ptrs[k] = v
    assert _call(native_lib.lib, ptrs, **kw) == MSI_E_BADARG
    msg = native_lib.last_error()
    assert "render_ods_views" in msg
    return msg


@pytest.mark.parametrize("fmt", [F32, RGBA8, RGBA16F])
@pytest.mark.parametrize("null", [0, 1, 2, 3, 4, 5])          # (eye_radius = 3 and trig = 5 included)
def test_rejects_null_inputs(native_lib, fmt, null):
    assert "null pointer" in _rejects(native_lib, {null: None}, fmt=fmt)


def test_rejects_both_outputs_null(native_lib):
    assert "both outputs are NULL" in _rejects(native_lib, {6: None, 7: None})


@pytest.mark.parametrize("fmt", [3, -1, 16])
def test_rejects_an_unknown_format(native_lib, fmt):
    assert "unknown format" in _rejects(native_lib, fmt=fmt)


@pytest.mark.parametrize("views", [0, -1])
def test_rejects_views_below_one(native_lib, views):
    assert "views must be >= 1" in _rejects(native_lib, views=views)


@pytest.mark.parametrize("dims", [dict(height=0), dict(width=0), dict(num_planes=0), dict(batch=-1), dict(height=-3)])
def test_rejects_bad_dims(native_lib, dims):
    assert "bad dims" in _rejects(native_lib, **dims)


@pytest.mark.parametrize("kw", [dict(out_height=0), dict(out_width=0), dict(out_height=-4)])
def test_rejects_a_bad_output_size(native_lib, kw):
    assert "bad output size" in _rejects(native_lib, **kw)
    assert _call(native_lib.lib, _ptrs(), batch=0, out_height=1, out_width=1) == 0          # (1 x 1 is a size)


def test_rejects_layers_beyond_24_bit_texel_offsets(native_lib):
    assert "2^24" in _rejects(native_lib, height=4096, width=4096)
    assert _call(native_lib.lib, _ptrs(), batch=0, height=4096, width=4095) == 0


@pytest.mark.parametrize("kw", [dict(out_height=1 << 30, out_width=1 << 14),                               # rows x blocks
                                dict(views=1 << 20, out_height=1 << 12, out_width=1 << 12),               # ... x views
                                dict(batch=1 << 20, views=1 << 8, out_height=1 << 11, out_width=1 << 10)])  # ... x batch
def test_rejects_grid_overflow(native_lib, kw):
    assert "too many target pixels" in _rejects(native_lib, **kw)


@pytest.mark.parametrize("fmt", [F32, RGBA8, RGBA16F])
def test_a_valid_empty_batch_passes_validation(native_lib, fmt):
    assert _call(native_lib.lib, _ptrs(), fmt=fmt, batch=0) == 0
    for out in (6, 7, 8):       # either output alone; no status word
        ptrs = _ptrs()
        ptrs[out] = None
        assert _call(native_lib.lib, ptrs, fmt=fmt, batch=0) == 0


# ----------------------------------------------------------------- the ODS camera is not a camera code of the other viewers
def test_camera_code_2_is_still_unknown_to_the_existing_entry_points(native_lib):
    lib = native_lib.lib
    p = [4096 * (k + 1) for k in range(10)]
    assert lib.msi_render_views_f32(p[0], p[1], p[2], p[3], p[4], p[5], 0, 2, 16, 32, 4, 2, 16, 32, p[6], p[7], p[8], None) == MSI_E_BADARG
    assert "unknown camera" in native_lib.last_error()
    assert lib.msi_render_views_packed(p[0], RGBA8, p[1], p[2], p[3], p[4], p[5], 0, 2, 16, 32, 4, 2, 16, 32, p[6], p[7], p[8],
                                       None) == MSI_E_BADARG
    assert "unknown camera" in native_lib.last_error()
    assert lib.msi_cube_render_views(p[0], F32, p[1], p[2], p[3], p[4], p[5], p[6], 0, 2, 16, 4, 2, 16, 32, p[7], p[8], p[9],
                                     None) == MSI_E_BADARG
    assert "unknown camera" in native_lib.last_error()
