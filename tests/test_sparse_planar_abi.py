"""CPU-only checks of the plumbing of the edge-rule sparse stacks: msi_sparse_index_tiles_edge, msi_mpi_render_views_sparse and
msi_cube_render_views_sparse are exported, bound and declared with one signature (ABI still 9), defined once, in geo_sparse.hip / geo_sparse_views.hip, and
their argument checks reject bad calls with the documented code and text before any HIP call.  No kernel is launched here: every
native call below fails its validation, or has an empty batch, before it could reach a device (the dummy pointers are never
dereferenced).  The harness's --msi_pp_sparse refusals and its --help need no device either; the TypeError / ValueError paths of the
MSI methods need an MSI object and are in tests/test_gpu_sparse_planar.py."""
import os
import re

import pytest

from tests.util import check_binding, header_text

MSI_E_BADARG, MSI_E_UNSUPPORTED = -1, -3
F32, RGBA8, RGBA16F = 0, 1, 2
EQUIRECT, PINHOLE = 0, 1
PARAMS = {
    "msi_sparse_index_tiles_edge": ["layers", "format", "batch", "num_planes", "height", "width", "table_out", "counts_out", "stream"],
    "msi_mpi_render_views_sparse": ["pool", "table", "layer_start", "format", "tgt_pose", "intrinsics", "tgt_intrinsics_inv", "depths", "batch",
                                    "views", "height", "width", "num_planes", "out_height", "out_width", "out_rgb", "out_depth", "stream"],
    "msi_cube_render_views_sparse": ["pool", "table", "layer_start", "format", "tgt_pose_rt", "tgt_pos", "tgt_intrinsics", "stack_intrinsics",
                                     "depths", "trig", "batch", "views", "face_size", "num_planes", "camera", "out_height", "out_width", "out_rgb",
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


def test_the_sparse_forms_take_the_dense_entry_points_arguments(native_lib):
    """(pool, table, layer_start, format) in place of (layers, format); the edge index takes msi_sparse_index_tiles' list."""
    for dense in ("msi_mpi_render_views", "msi_cube_render_views"):
        assert check_binding(native_lib, dense)[:2] == ["layers", "format"]
        assert PARAMS[dense + "_sparse"][4:] == check_binding(native_lib, dense)[2:]
    assert PARAMS["msi_sparse_index_tiles_edge"] == check_binding(native_lib, "msi_sparse_index_tiles")
    assert native_lib.SIGNATURES["msi_sparse_index_tiles_edge"] == native_lib.SIGNATURES["msi_sparse_index_tiles"]


def test_defined_once_in_geo_sparse():
    from matryodshka_amd import build
    for name in PARAMS:
        where = "geo_sparse.hip" if name == "msi_sparse_index_tiles_edge" else "geo_sparse_views.hip"
        pattern = re.compile(r"^int\s+%s\(" % name, re.M)
        hits = {}
        for unit in sorted(os.listdir(build.CSRC)):
            if unit.endswith((".hip", ".cpp", ".h", ".inc")):
                with open(os.path.join(build.CSRC, unit)) as f:
                    n = len(pattern.findall(f.read()))
                if n:
                    hits[unit] = n
        assert hits == {where: 1}, name


# ------------------------------------------------------------------------------------------------ msi_sparse_index_tiles_edge
def _p(k):
    return 4096 * (k + 1)


def _index(lib, ptrs, fmt=RGBA8, batch=2, num_planes=4, height=16, width=32):
    a, b, c = ptrs
    return lib.msi_sparse_index_tiles_edge(a, fmt, batch, num_planes, height, width, b, c, None)


def _index_rejects(native_lib, code=MSI_E_BADARG, null=None, **kw):
    ptrs = [_p(k) for k in range(3)]
    if null is not None:
        ptrs[null] = None
    assert _index(native_lib.lib, ptrs, **kw) == code
    msg = native_lib.last_error()
    assert "sparse_index_tiles_edge" in msg
    return msg


def test_the_edge_index_makes_the_tile_entry_points_checks(native_lib):
    for null in range(3):
        assert "null pointer" in _index_rejects(native_lib, null=null)
    for fmt in (F32, 3, -1):
        assert "unknown format" in _index_rejects(native_lib, fmt=fmt)
    for dims in (dict(height=0), dict(width=0), dict(num_planes=0), dict(batch=-1)):
        assert "bad dims" in _index_rejects(native_lib, **dims)
    assert "H % 4" in _index_rejects(native_lib, code=MSI_E_UNSUPPORTED, height=18)
    assert "W % 16" in _index_rejects(native_lib, code=MSI_E_UNSUPPORTED, width=40)
    assert "2^24" in _index_rejects(native_lib, height=4096, width=4096)
    for fmt in (RGBA8, RGBA16F):
        assert _index(native_lib.lib, [_p(k) for k in range(3)], fmt=fmt, batch=0) == 0


# ------------------------------------------------------------------------------------------------ msi_mpi_render_views_sparse
MPI_INPUTS = 7      # pool, table, layer_start, tgt_pose, intrinsics, tgt_intrinsics_inv, depths; then out_rgb, out_depth


def _mpi(lib, ptrs, fmt=RGBA8, batch=2, views=2, height=16, width=32, num_planes=4, out_height=16, out_width=32):
    pool, table, ls, pose, k, k_inv, depths, out_rgb, out_depth = ptrs
    return lib.msi_mpi_render_views_sparse(pool, table, ls, fmt, pose, k, k_inv, depths, batch, views, height, width, num_planes, out_height,
                                           out_width, out_rgb, out_depth, None)


def _mpi_rejects(native_lib, what=None, code=MSI_E_BADARG, **kw):
    ptrs = [_p(k) for k in range(MPI_INPUTS + 2)]
    for k, v in (what or {}).items():
        ptrs[k] = v
    assert _mpi(native_lib.lib, ptrs, **kw) == code
    msg = native_lib.last_error()
    assert "mpi_render_views_sparse" in msg
    return msg


def test_mpi_render_views_sparse_rejects_bad_calls(native_lib):
    for null in range(MPI_INPUTS):
        assert "null pointer" in _mpi_rejects(native_lib, {null: None})
    assert "both outputs are NULL" in _mpi_rejects(native_lib, {7: None, 8: None})
    assert "both outputs are NULL" in _mpi_rejects(native_lib, {7: None, 8: None, 0: None})       # (checked first)
    for fmt in (F32, 3, -1, 16):                                                                  # (fp32 pools are not built)
        assert "unknown format" in _mpi_rejects(native_lib, fmt=fmt)
    for dims in (dict(height=0), dict(width=0), dict(num_planes=0), dict(batch=-1)):
        assert "bad dims" in _mpi_rejects(native_lib, **dims)
    assert "at most 128 planes" in _mpi_rejects(native_lib, code=MSI_E_UNSUPPORTED, num_planes=129)
    for kw, text in ((dict(height=18), "H % 4"), (dict(height=2), "H % 4"), (dict(width=40), "W % 16"), (dict(width=8), "W % 16")):
        assert text in _mpi_rejects(native_lib, code=MSI_E_UNSUPPORTED, **kw)
        assert text in _mpi_rejects(native_lib, code=MSI_E_UNSUPPORTED, batch=0, **kw)             # (an empty batch is still validated)
    for views in (0, -1):
        assert "views must be >= 1" in _mpi_rejects(native_lib, views=views)
    for kw in (dict(out_height=0), dict(out_width=-3)):
        assert "bad output size" in _mpi_rejects(native_lib, **kw)
    assert "2^24" in _mpi_rejects(native_lib, height=4096, width=4096)
    assert "too many target pixels" in _mpi_rejects(native_lib, out_height=1 << 30, out_width=1 << 14)


@pytest.mark.parametrize("fmt", [RGBA8, RGBA16F])
def test_mpi_render_views_sparse_passes_a_valid_empty_batch(native_lib, fmt):
    ptrs = [_p(k) for k in range(MPI_INPUTS + 2)]
    assert _mpi(native_lib.lib, ptrs, fmt=fmt, batch=0) == 0
    assert _mpi(native_lib.lib, ptrs, fmt=fmt, batch=0, out_height=7, out_width=45, num_planes=128) == 0
    for out in (7, 8):                                    # either output alone
        one = list(ptrs)
        one[out] = None
        assert _mpi(native_lib.lib, one, fmt=fmt, batch=0) == 0


# ------------------------------------------------------------------------------------------------ msi_cube_render_views_sparse
def _cube_ptrs():
    # pool, table, layer_start, tgt_pose_rt, tgt_pos, tgt_intrinsics, stack_intrinsics, depths, trig, out_rgb, out_depth, status
    return [_p(k) for k in range(12)]


def _cube(lib, ptrs, fmt=RGBA8, batch=2, views=2, face_size=16, num_planes=3, camera=EQUIRECT, out_height=16, out_width=32):
    pool, table, ls, pose, pos, kt, ks, depths, trig, out_rgb, out_depth, status = ptrs
    return lib.msi_cube_render_views_sparse(pool, table, ls, fmt, pose, pos, kt, ks, depths, trig, batch, views, face_size, num_planes, camera,
                                            out_height, out_width, out_rgb, out_depth, status, None)


def _cube_rejects(native_lib, what=None, code=MSI_E_BADARG, **kw):
    ptrs = _cube_ptrs()
    for k, v in (what or {}).items():
        ptrs[k] = v
    assert _cube(native_lib.lib, ptrs, **kw) == code
    msg = native_lib.last_error()
    assert "cube_render_views_sparse" in msg
    return msg


def test_cube_render_views_sparse_rejects_bad_calls(native_lib):
    for camera in (EQUIRECT, PINHOLE):
        for null in (0, 1, 2, 3, 4, 6, 7):                # pool, table, layer_start, pose, position, stack_intrinsics, depths
            assert "null pointer" in _cube_rejects(native_lib, {null: None}, camera=camera)
    assert "equirect camera needs trig" in _cube_rejects(native_lib, {8: None}, camera=EQUIRECT)
    assert "pinhole camera needs intrinsics" in _cube_rejects(native_lib, {5: None}, camera=PINHOLE)
    assert "both outputs are NULL" in _cube_rejects(native_lib, {9: None, 10: None})
    assert "both outputs are NULL" in _cube_rejects(native_lib, {9: None, 10: None, 1: None})     # (checked first)
    for fmt in (F32, 3, -1, 16):
        assert "unknown format" in _cube_rejects(native_lib, fmt=fmt)
    for camera in (2, -1):
        assert "unknown camera" in _cube_rejects(native_lib, camera=camera)
    for dims in (dict(face_size=0), dict(num_planes=0), dict(batch=-1)):
        assert "bad dims" in _cube_rejects(native_lib, **dims)
    assert "at most 128 planes" in _cube_rejects(native_lib, code=MSI_E_UNSUPPORTED, num_planes=129)
    for s in (24, 12, 8, 20):
        assert "S % 16" in _cube_rejects(native_lib, code=MSI_E_UNSUPPORTED, face_size=s)
        assert "S % 16" in _cube_rejects(native_lib, code=MSI_E_UNSUPPORTED, face_size=s, batch=0)
    for views in (0, -1):
        assert "views must be >= 1" in _cube_rejects(native_lib, views=views)
    assert "bad output size" in _cube_rejects(native_lib, out_height=0)
    assert "bad output size" in _cube_rejects(native_lib, camera=PINHOLE, out_height=1)
    assert "2^31 bytes" in _cube_rejects(native_lib, face_size=4096, num_planes=32, fmt=RGBA8)    # 6 x 32 x 4096^2 x 4 = 12 GiB of dense faces
    assert "2^31 bytes" in _cube_rejects(native_lib, face_size=2048, num_planes=16, fmt=RGBA16F)  # 3 GiB
    assert "too many target pixels" in _cube_rejects(native_lib, out_height=1 << 30, out_width=1 << 14)


@pytest.mark.parametrize("fmt", [RGBA8, RGBA16F])
@pytest.mark.parametrize("camera", [EQUIRECT, PINHOLE])
def test_cube_render_views_sparse_passes_a_valid_empty_batch(native_lib, fmt, camera):
    assert _cube(native_lib.lib, _cube_ptrs(), fmt=fmt, camera=camera, batch=0) == 0
    for unused in ((5,) if camera == EQUIRECT else (8,)) + (9, 10, 11):       # the other camera's table, either output, the status word
        ptrs = _cube_ptrs()
        ptrs[unused] = None
        assert _cube(native_lib.lib, ptrs, fmt=fmt, camera=camera, batch=0) == 0
    assert _cube(native_lib.lib, _cube_ptrs(), fmt=fmt, camera=camera, batch=0, face_size=1024, num_planes=32) == 0     # 768 MiB / 1.5 GiB of dense faces


# ------------------------------------------------------------------------------------------------ the harness, without a device
def test_harness_help_names_the_flag(capsys):
    from matryodshka_amd import harness
    with pytest.raises(SystemExit) as e:
        harness.main(["--help"])                  # (argparse %-expands every help string)
    assert e.value.code == 0
    out = " ".join(capsys.readouterr().out.split())
    assert "--msi_pp_sparse" in out and "pp_sparse.json" in out and "--input_type PP" in out
    assert "--msi_sparse" in out and "high_res_only is refused" in out        # (--msi_sparse keeps its text)


@pytest.mark.parametrize("extra,text", [
    (["--msi_pp_sparse", "--input_type", "PP"], "needs --msi_format"),
    (["--msi_pp_sparse", "--msi_format", "rgba8"], "--input_type PP"),
    (["--msi_pp_sparse", "--msi_format", "rgba8", "--input_type", "ODS"], "--input_type PP"),
    (["--msi_pp_sparse", "--msi_format", "rgba8", "--input_type", "PP", "--height", "18"], "--height % 4 == 0"),
    (["--msi_pp_sparse", "--msi_format", "rgba16f", "--input_type", "PP", "--width", "40"], "--width % 16 == 0")])
def test_harness_refuses_msi_pp_sparse_where_it_cannot_apply(capsys, extra, text):
    """Argument errors come before the model is built: no device is needed."""
    from matryodshka_amd import harness
    with pytest.raises(SystemExit) as e:
        harness.main(["--cameras_glob", "none/*.txt"] + extra)
    assert e.value.code == 2
    err = capsys.readouterr().err
    assert "--msi_pp_sparse" in err and text in err


def test_msi_sparse_keeps_refusing_pp_inputs_with_its_text(capsys):
    from matryodshka_amd import harness
    with pytest.raises(SystemExit) as e:
        harness.main(["--cameras_glob", "none/*.txt", "--msi_sparse", "--msi_format", "rgba8", "--input_type", "PP"])
    assert e.value.code == 2
    assert "ODS only" in capsys.readouterr().err
