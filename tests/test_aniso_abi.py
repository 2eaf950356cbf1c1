"""CPU-only checks of the anisotropic viewer's plumbing: msi_render_views_aniso is exported, bound and declared with one signature
-- msi_render_views_mip's with max_anisotropy behind lod_bias; ABI still 9 --, defined once, in geo_mip.hip, and its argument
checks reject bad calls with the documented text before any launch; MSI.render_views refuses a bad max_anisotropy before it
touches a device.  No kernel is launched here: every native call below fails its validation, or has an empty batch (the dummy
pointers are never dereferenced)."""
import ctypes
import os
import re

import numpy as np
import pytest

from tests.util import check_binding, header_text

MSI_E_BADARG = -1
F32, RGBA8, RGBA16F = 0, 1, 2
EQUIRECT, PINHOLE = 0, 1
ANISO, MIP = "msi_render_views_aniso", "msi_render_views_mip"


def test_exported_bound_and_listed_without_a_bump(native_lib):
    assert ANISO in native_lib.SIGNATURES and hasattr(native_lib.lib, ANISO)
    assert native_lib.MSI_ABI_VERSION == 9 and native_lib.lib.msi_abi_version() == 9
    text = header_text(comments=True)
    at = text.index("#define MSI_ABI_VERSION 9")
    assert ANISO in text[text.index("additions since, no bump"):at]
    assert "#define MSI_ANISO_MAX %d" % native_lib.MSI_ANISO_MAX in header_text() and native_lib.MSI_ANISO_MAX == 16


def test_the_signature_is_the_mip_viewers_plus_max_anisotropy(native_lib):
    params, mip = check_binding(native_lib, ANISO), check_binding(native_lib, MIP)
    at = mip.index("lod_bias") + 1
    assert params == mip[:at] + ["max_anisotropy"] + mip[at:]
    args, mip_args = native_lib.SIGNATURES[ANISO][1], native_lib.SIGNATURES[MIP][1]
    assert args[at] is ctypes.c_float and args[at - 1] is ctypes.c_float
    assert args[:at] + args[at + 1:] == mip_args


def test_defined_once_in_the_mip_unit():
    from matryodshka_amd import build
    assert "geo_mip.hip" in build.GEO_UNITS
    pattern = re.compile(r"^int\s+%s\(" % ANISO, re.M)
    hits = {}
    for unit in sorted(os.listdir(build.CSRC)):
        if unit.endswith((".hip", ".cpp")):
            with open(os.path.join(build.CSRC, unit)) as f:
                n = len(pattern.findall(f.read()))
            if n:
                hits[unit] = n
    assert hits == {"geo_mip.hip": 1}


# ------------------------------------------------------------------------------------------------ msi_render_views_aniso
def _ptrs():
    # layers, mips, tgt_pose_rt, tgt_pos, intrinsics, eye_radius, depths, trig, out_rgb, out_depth, status
    return [4096 * (k + 1) for k in range(11)]


def _views(lib, ptrs, fmt=RGBA8, levels=3, lod_bias=0.0, max_anisotropy=8.0, batch=2, views=2, height=16, width=32, num_planes=4,
           camera=EQUIRECT, out_height=7, out_width=13):
    layers, mips, pose, pos, intr, radius, depths, trig, out_rgb, out_depth, status = ptrs
    return lib.msi_render_views_aniso(layers, fmt, mips, levels, lod_bias, max_anisotropy, pose, pos, intr, radius, depths, trig, batch, views,
                                      height, width, num_planes, camera, out_height, out_width, out_rgb, out_depth, status, None)


def _rejects(native_lib, what=None, **kw):
    ptrs = _ptrs()
    for k, v in (what or {}).items():
        ptrs[k] = v
    assert _views(native_lib.lib, ptrs, **kw) == MSI_E_BADARG
    msg = native_lib.last_error()
    assert msg.startswith("render_views_aniso:")
    return msg


@pytest.mark.parametrize("fmt", [F32, RGBA8, RGBA16F])
@pytest.mark.parametrize("null", [0, 1, 2, 3, 6])                  # layers, mips, pose, position, depths
def test_rejects_null_inputs(native_lib, fmt, null):
    assert "null pointer" in _rejects(native_lib, {null: None}, fmt=fmt)


def test_rejects_both_outputs_null(native_lib):
    assert "both outputs are NULL" in _rejects(native_lib, {8: None, 9: None})


@pytest.mark.parametrize("fmt", [3, -1, 16])
def test_rejects_an_unknown_format(native_lib, fmt):
    assert "unknown format" in _rejects(native_lib, fmt=fmt)


def test_camera_tables(native_lib):
    assert "equirect camera needs trig" in _rejects(native_lib, {7: None})
    assert "pinhole camera needs intrinsics" in _rejects(native_lib, {4: None, 5: None}, camera=PINHOLE)
    assert "eye_radius" in _rejects(native_lib, camera=PINHOLE)                    # (the ODS camera goes with the equirect code)
    assert "unknown camera" in _rejects(native_lib, camera=2)
    ptrs = _ptrs()
    ptrs[4] = ptrs[5] = None                                                        # equirect: neither intrinsics nor eye_radius
    assert _views(native_lib.lib, ptrs, batch=0) == 0
    ptrs = _ptrs()
    ptrs[1] = None                                                                  # one level: no mips buffer, still a valid call
    assert _views(native_lib.lib, ptrs, batch=0, levels=1) == 0


@pytest.mark.parametrize("levels", [0, -1, 7])
def test_rejects_levels_outside_1_to_6(native_lib, levels):
    assert "levels must be in 1..6" in _rejects(native_lib, levels=levels)


@pytest.mark.parametrize("kw", [dict(height=18, levels=3), dict(width=30, levels=3), dict(height=24, width=40, levels=5)])
def test_rejects_sizes_not_divisible_by_the_tile(native_lib, kw):
    assert "multiples of" in _rejects(native_lib, **kw)


@pytest.mark.parametrize("kw", [dict(levels=5), dict(height=4, width=64, levels=3), dict(height=32, width=64, levels=6)])
def test_rejects_a_top_level_below_2_x_2(native_lib, kw):
    assert "below 2 x 2" in _rejects(native_lib, **kw)


@pytest.mark.parametrize("value", [float("nan"), 0.5, 16.5, 0.0, -2.0, float("inf")])
def test_rejects_a_max_anisotropy_outside_1_to_16(native_lib, value):
    assert "max_anisotropy must be in 1..16" in _rejects(native_lib, max_anisotropy=value)


def test_the_checks_keep_the_mip_viewers_order(native_lib):
    assert "lod_bias is NaN" in _rejects(native_lib, lod_bias=float("nan"), max_anisotropy=0.5)        # the bias first
    assert "max_anisotropy" in _rejects(native_lib, max_anisotropy=0.5, levels=7)                      # then the cap, then the levels
    assert "bad dims" in _rejects(native_lib, num_planes=0, max_anisotropy=0.5)                        # the dims before all three
    assert "views must be >= 1" in _rejects(native_lib, views=0)
    assert "bad output size" in _rejects(native_lib, out_width=0)
    assert "bad output size" in _rejects(native_lib, {5: None}, camera=PINHOLE, out_height=1)
    assert "2^24" in _rejects(native_lib, height=4096, width=4096)
    assert "too many target pixels" in _rejects(native_lib, out_height=1 << 30, out_width=1 << 14)


@pytest.mark.parametrize("fmt", [F32, RGBA8, RGBA16F])
def test_accepts_a_valid_empty_batch(native_lib, fmt):
    for cap in (1.0, 1.5, 16.0):
        for bias in (0.0, -64.0, float("inf")):
            assert _views(native_lib.lib, _ptrs(), fmt=fmt, batch=0, lod_bias=bias, max_anisotropy=cap) == 0
    for out in (8, 9, 10):       # either output alone; no status word
        ptrs = _ptrs()
        ptrs[out] = None
        assert _views(native_lib.lib, ptrs, fmt=fmt, batch=0) == 0


# ------------------------------------------------------------------------------------------------ MSI.render_views
def test_render_views_refuses_a_bad_max_anisotropy_before_any_device_work(native_lib):
    """The keyword's checks come before the stack, the poses and the outputs are looked at: the method itself (under the wrapper
    that makes the model's device current) on an MSI that was never initialised and a host-side stack are enough."""
    import inspect
    import torch
    from matryodshka_amd import MSI
    m, render_views = object.__new__(MSI), MSI.render_views.__wrapped__
    for fn in (MSI.render_views, MSI.render_ods_pair):
        assert inspect.signature(fn).parameters["max_anisotropy"].default == 1.0
    stack = torch.zeros((1, 16, 32, 2, 4))
    pose, pos, planes = np.eye(4, dtype=np.float32)[None, None], np.zeros((1, 1, 3), np.float32), [10.0, 1.0]
    for bad in (float("nan"), 0.5, 0.0, 16.5, float("inf")):
        with pytest.raises(ValueError, match="max_anisotropy must be in"):
            render_views(m, stack, pose, pos, planes, max_anisotropy=bad)
    for cap in (1.5, 2.0, 16.0):
        with pytest.raises(ValueError, match="max_anisotropy belongs to a MipLayers"):
            render_views(m, stack, pose, pos, planes, max_anisotropy=cap)
