"""CPU-only checks of the sparse stacks' plumbing: the four entry points are exported, bound and declared with one signature (ABI
still 9: new entry points change no existing signature), defined in exactly one unit -- a geometry unit --, and their argument
checks reject bad calls with the documented code and text before any HIP call.  No kernel is launched here: every native call
below fails its validation, or has an empty batch, before it could reach a device (the dummy pointers are never dereferenced).
Python level: an MSI object cannot be constructed without a device (MSI.__init__ raises RuntimeError when none is available, and
every method runs under the model's device), so the TypeError / ValueError paths of MSI.sparsify_layers, densify_layers and
render_views on a SparseLayers are in tests/test_gpu_sparse_layers.py (test_6); what needs no device is here: the package export,
the harness's --msi_sparse argument refusals and its --help, and (tests/test_sparse_cpu.py) SparseLayers' own refusals."""
import os
import re

import pytest

from tests.util import check_binding, header_text

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
MSI_E_BADARG, MSI_E_UNSUPPORTED = -1, -3
F32, RGBA8, RGBA16F = 0, 1, 2
EQUIRECT, PINHOLE = 0, 1
PARAMS = {
    "msi_sparse_index_tiles": ["layers", "format", "batch", "num_planes", "height", "width", "table_out", "counts_out", "stream"],
    "msi_sparse_gather_tiles": ["layers", "format", "table", "layer_start", "batch", "num_planes", "height", "width", "pool_out", "stream"],
    "msi_sparse_expand": ["pool", "table", "layer_start", "format", "batch", "num_planes", "height", "width", "layers_out", "stream"],
    "msi_render_views_sparse": ["pool", "table", "layer_start", "format", "tgt_pose_rt", "tgt_pos", "intrinsics", "eye_radius", "depths",
                                "trig", "batch", "views", "height", "width", "num_planes", "camera", "out_height", "out_width", "out_rgb",
                                "out_depth", "status_device", "stream"],
}


def test_exported_and_bound(native_lib):
    for name in PARAMS:
        assert name in native_lib.SIGNATURES
        assert hasattr(native_lib.lib, name)
    assert native_lib.MSI_ABI_VERSION == 9
    assert native_lib.lib.msi_abi_version() == 9


@pytest.mark.parametrize("name", sorted(PARAMS))
def test_header_and_binding_agree_on_the_signature(native_lib, name):
    assert "#define MSI_ABI_VERSION 9" in header_text()
    assert check_binding(native_lib, name, int32_and_pointers=True) == PARAMS[name]


def test_defined_once_in_a_geometry_unit():
    from matryodshka_amd import build
    for name in PARAMS:
        where = "geo_sparse_views.hip" if name == "msi_render_views_sparse" else "geo_sparse.hip"
        assert where in build.GEO_UNITS
        flags = dict(build.SOURCES)[where]
        assert "-ffp-contract=off" in flags and "-fno-slp-vectorize" in flags
        pattern = re.compile(r"^int\s+%s\(" % name, re.M)
        hits = {}
        for unit in sorted(os.listdir(build.CSRC)):
            if unit.endswith((".hip", ".cpp")):
                with open(os.path.join(build.CSRC, unit)) as f:
                    n = len(pattern.findall(f.read()))
                if n:
                    hits[unit] = n
        assert hits == {where: 1}, name


def test_the_python_rule_and_the_kernels_agree_on_the_tile():
    from matryodshka_amd import build, sparse
    text = open(os.path.join(build.CSRC, "geo_sparse.h")).read()
    m = re.search(r"constexpr int TILE_H = (\d+), TILE_W = (\d+);", text)
    assert m and (int(m.group(1)), int(m.group(2))) == (sparse.TILE_H, sparse.TILE_W) == (4, 16)


# ------------------------------------------------------------------------------------------------ the tile entry points
def _p(k):
    return 4096 * (k + 1)


def _tile_call(lib, name, ptrs, fmt=RGBA8, batch=2, num_planes=4, height=16, width=32):
    a, b, c, d = ptrs
    if name == "msi_sparse_index_tiles":      # layers, table_out, counts_out
        return lib.msi_sparse_index_tiles(a, fmt, batch, num_planes, height, width, b, c, None)
    if name == "msi_sparse_gather_tiles":     # layers, table, layer_start, pool_out
        return lib.msi_sparse_gather_tiles(a, fmt, b, c, batch, num_planes, height, width, d, None)
    return lib.msi_sparse_expand(a, b, c, fmt, batch, num_planes, height, width, d, None)   # pool, table, layer_start, layers_out


TILE_ENTRIES = [("msi_sparse_index_tiles", 3), ("msi_sparse_gather_tiles", 4), ("msi_sparse_expand", 4)]


def _tile_rejects(native_lib, name, code=MSI_E_BADARG, null=None, **kw):
    ptrs = [_p(k) for k in range(4)]
    if null is not None:
        ptrs[null] = None
    assert _tile_call(native_lib.lib, name, ptrs, **kw) == code
    msg = native_lib.last_error()
    assert name[len("msi_"):] in msg
    return msg


@pytest.mark.parametrize("name,n_ptrs", TILE_ENTRIES)
def test_tile_entry_points_reject_bad_calls(native_lib, name, n_ptrs):
    for null in range(n_ptrs):
        assert "null pointer" in _tile_rejects(native_lib, name, null=null)
    for fmt in (F32, 3, -1):                                                  # (fp32 pools are not built)
        assert "unknown format" in _tile_rejects(native_lib, name, fmt=fmt)
    for dims in (dict(height=0), dict(width=0), dict(num_planes=0), dict(batch=-1), dict(width=-16)):
        assert "bad dims" in _tile_rejects(native_lib, name, **dims)
    assert "H % 4" in _tile_rejects(native_lib, name, code=MSI_E_UNSUPPORTED, height=18)
    assert "W % 16" in _tile_rejects(native_lib, name, code=MSI_E_UNSUPPORTED, width=40)
    assert "2^24" in _tile_rejects(native_lib, name, height=4096, width=4096)
    for fmt in (RGBA8, RGBA16F):                                              # a valid empty batch passes, without a launch
        assert _tile_call(native_lib.lib, name, [_p(k) for k in range(4)], fmt=fmt, batch=0) == 0
        assert _tile_call(native_lib.lib, name, [_p(k) for k in range(4)], fmt=fmt, batch=0, height=4096, width=4080) == 0


# ------------------------------------------------------------------------------------------------ msi_render_views_sparse
def _ptrs():
    # pool, table, layer_start, tgt_pose_rt, tgt_pos, intrinsics, eye_radius, depths, trig, out_rgb, out_depth, status
    p = [_p(k) for k in range(12)]
    p[6] = None                 # (no eye_radius: the cameras of render_views)
    return p


def _call(lib, ptrs, fmt=RGBA8, batch=2, views=2, height=16, width=32, num_planes=4, camera=EQUIRECT, out_height=16, out_width=32):
    pool, table, ls, pose, pos, intr, radius, depths, trig, out_rgb, out_depth, status = ptrs
    return lib.msi_render_views_sparse(pool, table, ls, fmt, pose, pos, intr, radius, depths, trig, batch, views, height, width, num_planes,
                                       camera, out_height, out_width, out_rgb, out_depth, status, None)


def _rejects(native_lib, what=None, code=MSI_E_BADARG, **kw):
    ptrs = _ptrs()
    for k, v in (what or {}).items():
        ptrs[k] = v
    assert _call(native_lib.lib, ptrs, **kw) == code
    msg = native_lib.last_error()
    assert "render_views_sparse" in msg
    return msg


@pytest.mark.parametrize("fmt", [RGBA8, RGBA16F])
@pytest.mark.parametrize("camera", [EQUIRECT, PINHOLE])
@pytest.mark.parametrize("null", [0, 1, 2, 3, 4, 7])          # pool, table, layer_start, pose, position, depths
def test_rejects_null_inputs(native_lib, fmt, camera, null):
    assert "null pointer" in _rejects(native_lib, {null: None}, fmt=fmt, camera=camera)


def test_rejects_the_null_input_of_a_camera(native_lib):
    assert "equirect camera needs trig" in _rejects(native_lib, {8: None}, camera=EQUIRECT)
    assert "pinhole camera needs intrinsics" in _rejects(native_lib, {5: None}, camera=PINHOLE)
    assert "equirect camera needs trig" in _rejects(native_lib, {8: None, 6: _p(20)}, camera=EQUIRECT)     # the ODS camera
    for unused, camera in ((5, EQUIRECT), (8, PINHOLE)):                     # the other camera's input may be NULL
        ptrs = _ptrs()
        ptrs[unused] = None
        assert _call(native_lib.lib, ptrs, batch=0, camera=camera) == 0


def test_rejects_both_outputs_null(native_lib):
    assert "both outputs are NULL" in _rejects(native_lib, {9: None, 10: None})
    assert "both outputs are NULL" in _rejects(native_lib, {9: None, 10: None, 0: None})      # (checked first)


@pytest.mark.parametrize("fmt", [F32, 3, -1, 16])
def test_rejects_an_unknown_format(native_lib, fmt):
    assert "unknown format" in _rejects(native_lib, fmt=fmt)


@pytest.mark.parametrize("camera", [2, -1, 7])
def test_rejects_a_bad_camera(native_lib, camera):
    assert "unknown camera" in _rejects(native_lib, camera=camera)
    assert "unknown camera" in _rejects(native_lib, {6: _p(20)}, camera=camera)


def test_the_ods_camera_is_eye_radius_with_the_equirect_code(native_lib):
    assert "eye_radius" in _rejects(native_lib, {6: _p(20)}, camera=PINHOLE)
    ptrs = _ptrs()
    ptrs[6] = _p(20)
    assert _call(native_lib.lib, ptrs, batch=0, camera=EQUIRECT) == 0


@pytest.mark.parametrize("views", [0, -1])
def test_rejects_views_below_one(native_lib, views):
    assert "views must be >= 1" in _rejects(native_lib, views=views)


@pytest.mark.parametrize("dims", [dict(height=0), dict(width=0), dict(num_planes=0), dict(batch=-1), dict(height=-4)])
def test_rejects_bad_dims(native_lib, dims):
    assert "bad dims" in _rejects(native_lib, **dims)


@pytest.mark.parametrize("kw,text", [(dict(height=18), "H % 4"), (dict(height=2), "H % 4"), (dict(width=40), "W % 16"), (dict(width=8), "W % 16")])
def test_sizes_that_are_not_whole_tiles_are_unsupported(native_lib, kw, text):
    assert text in _rejects(native_lib, code=MSI_E_UNSUPPORTED, **kw)
    assert text in _rejects(native_lib, code=MSI_E_UNSUPPORTED, batch=0, **kw)


@pytest.mark.parametrize("kw", [dict(out_height=0), dict(out_width=0), dict(out_height=-4), dict(camera=PINHOLE, out_height=1)])
def test_rejects_a_bad_output_size(native_lib, kw):
    assert "bad output size" in _rejects(native_lib, **kw)
    assert _call(native_lib.lib, _ptrs(), batch=0, out_height=1, out_width=1) == 0          # (1 x 1 is a size of the equirect camera)


def test_rejects_layers_beyond_24_bit_texel_offsets(native_lib):
    assert "2^24" in _rejects(native_lib, height=4096, width=4096)
    assert _call(native_lib.lib, _ptrs(), batch=0, height=4096, width=4080) == 0


@pytest.mark.parametrize("kw", [dict(out_height=1 << 30, out_width=1 << 14),
                                dict(views=1 << 20, out_height=1 << 12, out_width=1 << 12),
                                dict(batch=1 << 20, views=1 << 8, out_height=1 << 11, out_width=1 << 10)])
def test_rejects_grid_overflow(native_lib, kw):
    assert "too many target pixels" in _rejects(native_lib, **kw)


@pytest.mark.parametrize("fmt", [RGBA8, RGBA16F])
@pytest.mark.parametrize("camera", [EQUIRECT, PINHOLE])
def test_a_valid_empty_batch_passes_validation(native_lib, fmt, camera):
    assert _call(native_lib.lib, _ptrs(), fmt=fmt, camera=camera, batch=0) == 0
    for out in (9, 10, 11):       # either output alone; no status word
        ptrs = _ptrs()
        ptrs[out] = None
        assert _call(native_lib.lib, ptrs, fmt=fmt, camera=camera, batch=0) == 0


# ------------------------------------------------------------------------------------------------ Python, without a device
def test_the_package_exports_sparse_layers_without_loading_the_library():
    import subprocess
    import sys
    code = ("import sys, matryodshka_amd as m; from matryodshka_amd.sparse import SparseLayers; assert m.SparseLayers is SparseLayers; "
            "assert 'matryodshka_amd._native' not in sys.modules")
    assert subprocess.run([sys.executable, "-c", code], cwd=ROOT).returncode == 0


def test_harness_help_prints_and_exits_cleanly(capsys):
    from matryodshka_amd import harness
    with pytest.raises(SystemExit) as e:
        harness.main(["--help"])                  # (argparse %-expands every help string)
    assert e.value.code == 0
    out = " ".join(capsys.readouterr().out.split())
    assert "--msi_sparse" in out and "--height % 4 == 0" in out and "high_res_only is refused" in out


@pytest.mark.parametrize("extra,text", [
    (["--msi_sparse"], "needs --msi_format"),
    (["--msi_sparse", "--msi_format", "rgba8", "--width", "40"], "--width % 16 == 0"),
    (["--msi_sparse", "--msi_format", "rgba8", "--height", "18"], "--height % 4 == 0"),
    (["--msi_sparse", "--msi_format", "rgba8", "--input_type", "PP"], "ODS only"),
    (["--msi_sparse", "--msi_format", "rgba8", "--test_type", "on_video_high_res_only"], "high_res_only")])
def test_harness_refuses_msi_sparse_where_it_cannot_apply(capsys, extra, text):
    """Argument errors come before the model is built: no device is needed."""
    from matryodshka_amd import harness
    with pytest.raises(SystemExit) as e:
        harness.main(["--cameras_glob", "none/*.txt"] + extra)
    assert e.value.code == 2
    assert text in capsys.readouterr().err
