"""CPU-only checks of the mip-mapped stacks' plumbing: msi_build_mips and msi_render_views_mip are exported, bound and declared
with one signature (ABI still 9: new entry points change no existing signature), defined in exactly one unit -- geo_mip.hip, a
geometry unit --, and their argument checks reject bad calls with the documented text before any launch.  No kernel is launched
here: every native call below fails its validation, or has an empty batch, before it could reach a device (the dummy pointers
are never dereferenced)."""
import ctypes
import os
import re

import pytest

from tests.util import check_binding, header_text

MSI_E_BADARG = -1
F32, RGBA8, RGBA16F = 0, 1, 2
EQUIRECT, PINHOLE = 0, 1
BUILD, VIEWS = "msi_build_mips", "msi_render_views_mip"
BUILD_PARAMS = ["layers", "format", "batch", "num_planes", "height", "width", "levels", "mips_out", "stream"]
VIEWS_PARAMS = ["layers", "format", "mips", "levels", "lod_bias", "tgt_pose_rt", "tgt_pos", "intrinsics", "eye_radius", "depths", "trig",
                "batch", "views", "height", "width", "num_planes", "camera", "out_height", "out_width", "out_rgb", "out_depth",
                "status_device", "stream"]


def test_exported_and_bound(native_lib):
    for name in (BUILD, VIEWS):
        assert name in native_lib.SIGNATURES and hasattr(native_lib.lib, name)
    assert native_lib.MSI_ABI_VERSION == 9 and native_lib.lib.msi_abi_version() == 9


def test_header_and_binding_agree_on_the_signatures(native_lib):
    assert "#define MSI_ABI_VERSION 9" in header_text()
    assert check_binding(native_lib, BUILD, int32_and_pointers=True) == BUILD_PARAMS
    assert check_binding(native_lib, VIEWS) == VIEWS_PARAMS
    assert native_lib.SIGNATURES[VIEWS][1][4] is ctypes.c_float                     # lod_bias, the one scalar that is not an int32
    # msi_render_views_packed's list, plus mips / levels / lod_bias behind the format and eye_radius behind intrinsics
    packed = check_binding(native_lib, "msi_render_views_packed")
    assert [p for p in VIEWS_PARAMS if p not in ("mips", "levels", "lod_bias", "eye_radius")] == packed


def test_the_level_limit_is_the_headers():
    from matryodshka_amd import mips
    assert "#define MSI_MIP_MAX_LEVELS %d" % mips.MAX_LEVELS in header_text() and mips.MAX_LEVELS == 6


def test_defined_once_in_a_geometry_unit():
    from matryodshka_amd import build
    assert "geo_mip.hip" in build.GEO_UNITS
    flags = dict(build.SOURCES)["geo_mip.hip"]
    assert "-ffp-contract=off" in flags and "-fno-slp-vectorize" in flags
    for name in (BUILD, VIEWS):
        pattern = re.compile(r"^int\s+%s\(" % name, re.M)
        hits = {}
        for unit in sorted(os.listdir(build.CSRC)):
            if unit.endswith((".hip", ".cpp")):
                with open(os.path.join(build.CSRC, unit)) as f:
                    n = len(pattern.findall(f.read()))
                if n:
                    hits[unit] = n
        assert hits == {"geo_mip.hip": 1}, name


def test_mips_py_does_not_load_the_native_library():
    import subprocess
    import sys
    code = "import sys; from matryodshka_amd import mips, MipLayers; assert 'matryodshka_amd._native' not in sys.modules"
    root = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    assert subprocess.run([sys.executable, "-c", code], cwd=root).returncode == 0


# ------------------------------------------------------------------------------------------------ msi_build_mips
def _build(lib, layers=4096, fmt=RGBA8, batch=2, num_planes=4, height=16, width=32, levels=3, mips=8192):
    return lib.msi_build_mips(layers, fmt, batch, num_planes, height, width, levels, mips, None)


def _build_rejects(native_lib, **kw):
    assert _build(native_lib.lib, **kw) == MSI_E_BADARG
    msg = native_lib.last_error()
    assert msg.startswith("build_mips:")
    return msg


def test_build_rejects_null_pointers(native_lib):
    assert "null pointer" in _build_rejects(native_lib, layers=None)
    assert "null pointer" in _build_rejects(native_lib, mips=None)
    assert _build(native_lib.lib, mips=None, levels=1, batch=0) == 0              # (one level: nothing to write)


@pytest.mark.parametrize("fmt", [3, -1, 16])
def test_build_rejects_an_unknown_format(native_lib, fmt):
    assert "unknown format" in _build_rejects(native_lib, fmt=fmt)


@pytest.mark.parametrize("dims", [dict(height=0), dict(width=-2), dict(num_planes=0), dict(batch=-1)])
def test_build_rejects_bad_dims(native_lib, dims):
    assert "bad dims" in _build_rejects(native_lib, **dims)


@pytest.mark.parametrize("levels", [0, -1, 7, 100])
def test_build_rejects_levels_outside_1_to_6(native_lib, levels):
    assert "levels must be in 1..6" in _build_rejects(native_lib, levels=levels)


@pytest.mark.parametrize("kw", [dict(height=18, levels=3), dict(width=30, levels=3), dict(height=24, width=40, levels=5)])
def test_build_rejects_sizes_not_divisible_by_the_tile(native_lib, kw):
    assert "multiples of" in _build_rejects(native_lib, **kw)


@pytest.mark.parametrize("kw", [dict(levels=5), dict(height=4, width=64, levels=3), dict(height=32, width=2, levels=2),
                                dict(height=32, width=64, levels=6)])
def test_build_rejects_a_top_level_below_2_x_2(native_lib, kw):
    assert "below 2 x 2" in _build_rejects(native_lib, **kw)


@pytest.mark.parametrize("fmt", [F32, RGBA8, RGBA16F])
def test_build_accepts_a_valid_empty_batch(native_lib, fmt):
    assert _build(native_lib.lib, fmt=fmt, batch=0) == 0
    assert _build(native_lib.lib, fmt=fmt, batch=0, height=64, width=128, levels=6) == 0
    assert _build(native_lib.lib, fmt=fmt, batch=0, levels=4) == 0                # 16 x 32: a 2 x 4 top level


# ------------------------------------------------------------------------------------------------ msi_render_views_mip
def _ptrs():
    # layers, mips, tgt_pose_rt, tgt_pos, intrinsics, eye_radius, depths, trig, out_rgb, out_depth, status
    return [4096 * (k + 1) for k in range(11)]


def _views(lib, ptrs, fmt=RGBA8, levels=3, lod_bias=0.0, batch=2, views=2, height=16, width=32, num_planes=4, camera=EQUIRECT,
           out_height=7, out_width=13):
    layers, mips, pose, pos, intr, radius, depths, trig, out_rgb, out_depth, status = ptrs
    return lib.msi_render_views_mip(layers, fmt, mips, levels, lod_bias, pose, pos, intr, radius, depths, trig, batch, views, height, width,
                                    num_planes, camera, out_height, out_width, out_rgb, out_depth, status, None)


def _views_rejects(native_lib, what=None, **kw):
    ptrs = _ptrs()
    for k, v in (what or {}).items():
        ptrs[k] = v
    assert _views(native_lib.lib, ptrs, **kw) == MSI_E_BADARG
    msg = native_lib.last_error()
    assert msg.startswith("render_views_mip:")
    return msg


@pytest.mark.parametrize("fmt", [F32, RGBA8, RGBA16F])
@pytest.mark.parametrize("null", [0, 1, 2, 3, 6])                  # layers, mips, pose, position, depths
def test_views_rejects_null_inputs(native_lib, fmt, null):
    assert "null pointer" in _views_rejects(native_lib, {null: None}, fmt=fmt)


def test_views_camera_tables(native_lib):
    assert "equirect camera needs trig" in _views_rejects(native_lib, {7: None})
    assert "pinhole camera needs intrinsics" in _views_rejects(native_lib, {4: None, 5: None}, camera=PINHOLE)
    assert "eye_radius" in _views_rejects(native_lib, camera=PINHOLE)              # (the ODS camera goes with the equirect code)
    assert "unknown camera" in _views_rejects(native_lib, camera=2)
    ptrs = _ptrs()
    ptrs[4] = ptrs[5] = None                                                        # equirect: neither intrinsics nor eye_radius
    assert _views(native_lib.lib, ptrs, batch=0) == 0
    ptrs = _ptrs()
    ptrs[1] = None                                                                  # one level: no mips buffer
    assert _views(native_lib.lib, ptrs, batch=0, levels=1) == 0


def test_views_rejects_both_outputs_null(native_lib):
    assert "both outputs are NULL" in _views_rejects(native_lib, {8: None, 9: None})


@pytest.mark.parametrize("fmt", [3, -1, 16])
def test_views_rejects_an_unknown_format(native_lib, fmt):
    assert "unknown format" in _views_rejects(native_lib, fmt=fmt)


@pytest.mark.parametrize("levels", [0, -1, 7])
def test_views_rejects_levels_outside_1_to_6(native_lib, levels):
    assert "levels must be in 1..6" in _views_rejects(native_lib, levels=levels)


@pytest.mark.parametrize("kw", [dict(height=18, levels=3), dict(width=30, levels=3), dict(height=24, width=40, levels=5)])
def test_views_rejects_sizes_not_divisible_by_the_tile(native_lib, kw):
    assert "multiples of" in _views_rejects(native_lib, **kw)


@pytest.mark.parametrize("kw", [dict(levels=5), dict(height=4, width=64, levels=3), dict(height=32, width=64, levels=6)])
def test_views_rejects_a_top_level_below_2_x_2(native_lib, kw):
    assert "below 2 x 2" in _views_rejects(native_lib, **kw)


def test_views_rejects_a_nan_bias_and_the_common_view_checks(native_lib):
    assert "lod_bias is NaN" in _views_rejects(native_lib, lod_bias=float("nan"))
    assert "bad dims" in _views_rejects(native_lib, num_planes=0)
    assert "views must be >= 1" in _views_rejects(native_lib, views=0)
    assert "bad output size" in _views_rejects(native_lib, out_width=0)
    assert "bad output size" in _views_rejects(native_lib, {5: None}, camera=PINHOLE, out_height=1)
    assert "2^24" in _views_rejects(native_lib, height=4096, width=4096)
    assert "too many target pixels" in _views_rejects(native_lib, out_height=1 << 30, out_width=1 << 14)


@pytest.mark.parametrize("fmt", [F32, RGBA8, RGBA16F])
def test_views_accepts_a_valid_empty_batch(native_lib, fmt):
    for bias in (0.0, -64.0, 64.0, float("inf")):
        assert _views(native_lib.lib, _ptrs(), fmt=fmt, batch=0, lod_bias=bias) == 0
    for out in (8, 9, 10):       # either output alone; no status word
        ptrs = _ptrs()
        ptrs[out] = None
        assert _views(native_lib.lib, ptrs, fmt=fmt, batch=0) == 0
