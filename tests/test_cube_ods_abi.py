"""CPU-only checks of the plumbing of the cube viewer's ODS camera: msi_cube_render_ods_views and msi_cube_render_ods_views_sparse are
exported, bound and declared with one signature (ABI still 9), and their argument checks reject bad calls with the documented code
and text, in the documented order, before any HIP call.  No kernel is launched here: every native call below fails its validation,
or has an empty batch, before it could reach a device (the dummy pointers are never dereferenced).  The camera codes of the three
existing cube entry points stay 0 and 1 (tests/test_sparse_planar_abi.py and tests/test_native_abi.py pin camera = 2 as unknown)."""
import pytest

from tests.util import check_binding

MSI_E_BADARG, MSI_E_UNSUPPORTED = -1, -3
F32, RGBA8, RGBA16F = 0, 1, 2
CLAMP, SEAMLESS = 0, 1
TAIL = ["tgt_pose_rt", "tgt_pos", "eye_radius", "stack_intrinsics", "depths", "trig", "batch", "views", "face_size", "num_planes"]
OUT = ["out_height", "out_width", "out_rgb", "out_depth", "status_device", "stream"]
PARAMS = {
    "msi_cube_render_ods_views": ["layers", "format"] + TAIL + ["filtering"] + OUT,
    "msi_cube_render_ods_views_sparse": ["pool", "table", "layer_start", "format"] + TAIL + OUT,
}


def test_exported_and_bound(native_lib):
    for name in PARAMS:
        assert name in native_lib.SIGNATURES
        assert hasattr(native_lib.lib, name)
    assert native_lib.MSI_ABI_VERSION == 9
    assert native_lib.lib.msi_abi_version() == 9


@pytest.mark.parametrize("name", sorted(PARAMS))
def test_header_and_binding_agree_on_the_signature(native_lib, name):
    assert check_binding(native_lib, name, int32_and_pointers=True) == PARAMS[name]


def test_the_argument_lists_mirror_the_camera_code_entry_points(native_lib):
    """eye_radius where tgt_intrinsics goes; no camera code; the dense form has a filtering code in its place."""
    dense = check_binding(native_lib, "msi_cube_render_views")
    assert [("eye_radius" if a == "tgt_intrinsics" else "filtering" if a == "camera" else a) for a in dense] == PARAMS["msi_cube_render_ods_views"]
    sparse = check_binding(native_lib, "msi_cube_render_views_sparse")
    assert [("eye_radius" if a == "tgt_intrinsics" else a) for a in sparse if a != "camera"] == PARAMS["msi_cube_render_ods_views_sparse"]


def _p(k):
    return 4096 * (k + 1)


# ------------------------------------------------------------------------------------------------ msi_cube_render_ods_views
DENSE_INPUTS = 7     # layers, tgt_pose_rt, tgt_pos, eye_radius, stack_intrinsics, depths, trig; then out_rgb, out_depth, status


def _dense(lib, ptrs, fmt=F32, batch=2, views=2, face_size=16, num_planes=5, filtering=CLAMP, out_height=12, out_width=24):
    layers, pose, pos, radius, ks, depths, trig, out_rgb, out_depth, status = ptrs
    return lib.msi_cube_render_ods_views(layers, fmt, pose, pos, radius, ks, depths, trig, batch, views, face_size, num_planes, filtering,
                                         out_height, out_width, out_rgb, out_depth, status, None)


def _dense_rejects(native_lib, what=None, code=MSI_E_BADARG, **kw):
    ptrs = [_p(k) for k in range(DENSE_INPUTS + 3)]
    for k, v in (what or {}).items():
        ptrs[k] = v
    assert _dense(native_lib.lib, ptrs, **kw) == code
    msg = native_lib.last_error()
    assert "cube_render_ods_views:" in msg
    return msg


def test_dense_rejects_bad_calls_in_the_documented_order(native_lib):
    for filtering in (CLAMP, SEAMLESS):
        for null in range(DENSE_INPUTS):                  # every input is required: eye_radius (3) and trig (6) included
            assert "null pointer" in _dense_rejects(native_lib, {null: None}, filtering=filtering)
    both = {DENSE_INPUTS: None, DENSE_INPUTS + 1: None}
    assert "both outputs are NULL" in _dense_rejects(native_lib, both)
    assert "both outputs are NULL" in _dense_rejects(native_lib, {0: None, **both})             # (checked first)
    assert "null pointer" in _dense_rejects(native_lib, {3: None}, fmt=7)                             # a NULL input before the format
    for fmt in (3, -1, 16):
        assert "unknown format" in _dense_rejects(native_lib, fmt=fmt)
    assert "unknown format" in _dense_rejects(native_lib, fmt=3, face_size=0)                         # the format before the dims
    for dims in (dict(face_size=0), dict(num_planes=0), dict(batch=-1)):
        assert "bad dims" in _dense_rejects(native_lib, **dims)
    assert "bad dims" in _dense_rejects(native_lib, face_size=0, filtering=2)                         # the dims before the filtering
    for filtering in (2, -1):
        assert "unknown filtering" in _dense_rejects(native_lib, filtering=filtering)
        assert "unknown filtering" in _dense_rejects(native_lib, filtering=filtering, batch=0)
    assert "unknown filtering" in _dense_rejects(native_lib, filtering=2, num_planes=129)             # the filtering before the plane count
    assert "at most 128 planes" in _dense_rejects(native_lib, code=MSI_E_UNSUPPORTED, num_planes=129)
    assert "at most 128 planes" in _dense_rejects(native_lib, code=MSI_E_UNSUPPORTED, num_planes=129, views=0)
    for views in (0, -1):
        assert "views must be >= 1" in _dense_rejects(native_lib, views=views)
    assert "bad output size" in _dense_rejects(native_lib, out_height=0)
    assert "bad output size" in _dense_rejects(native_lib, out_width=0)
    assert "2^31 bytes" in _dense_rejects(native_lib, face_size=1024, num_planes=32, fmt=F32)         # 6 x 32 x 1024^2 x 16 = 3 GiB
    assert "2^31 bytes" in _dense_rejects(native_lib, face_size=2048, num_planes=16, fmt=RGBA16F)     # 3 GiB
    assert "2^31 bytes" in _dense_rejects(native_lib, face_size=4096, num_planes=32, fmt=RGBA8, filtering=SEAMLESS)
    assert "too many target pixels" in _dense_rejects(native_lib, out_height=1 << 30, out_width=1 << 14)


@pytest.mark.parametrize("fmt", [F32, RGBA8, RGBA16F])
@pytest.mark.parametrize("filtering", [CLAMP, SEAMLESS])
def test_dense_passes_a_valid_empty_batch(native_lib, fmt, filtering):
    ptrs = [_p(k) for k in range(DENSE_INPUTS + 3)]
    assert _dense(native_lib.lib, ptrs, fmt=fmt, filtering=filtering, batch=0) == 0
    assert _dense(native_lib.lib, ptrs, fmt=fmt, filtering=filtering, batch=0, out_height=1, out_width=1) == 0     # 1 x 1: no pinhole minimum
    for unused in (DENSE_INPUTS, DENSE_INPUTS + 1, DENSE_INPUTS + 2):          # either output, the status word
        one = list(ptrs)
        one[unused] = None
        assert _dense(native_lib.lib, one, fmt=fmt, filtering=filtering, batch=0) == 0


# ------------------------------------------------------------------------------------------------ msi_cube_render_ods_views_sparse
SPARSE_INPUTS = 9    # pool, table, layer_start, tgt_pose_rt, tgt_pos, eye_radius, stack_intrinsics, depths, trig


def _sparse(lib, ptrs, fmt=RGBA8, batch=2, views=2, face_size=16, num_planes=5, out_height=12, out_width=24):
    pool, table, ls, pose, pos, radius, ks, depths, trig, out_rgb, out_depth, status = ptrs
    return lib.msi_cube_render_ods_views_sparse(pool, table, ls, fmt, pose, pos, radius, ks, depths, trig, batch, views, face_size, num_planes,
                                                out_height, out_width, out_rgb, out_depth, status, None)


def _sparse_rejects(native_lib, what=None, code=MSI_E_BADARG, **kw):
    ptrs = [_p(k) for k in range(SPARSE_INPUTS + 3)]
    for k, v in (what or {}).items():
        ptrs[k] = v
    assert _sparse(native_lib.lib, ptrs, **kw) == code
    msg = native_lib.last_error()
    assert "cube_render_ods_views_sparse:" in msg
    return msg


def test_sparse_rejects_bad_calls_in_the_documented_order(native_lib):
    for null in range(SPARSE_INPUTS):
        assert "null pointer" in _sparse_rejects(native_lib, {null: None})
    both = {SPARSE_INPUTS: None, SPARSE_INPUTS + 1: None}
    assert "both outputs are NULL" in _sparse_rejects(native_lib, both)
    assert "both outputs are NULL" in _sparse_rejects(native_lib, {1: None, **both})            # (checked first)
    for fmt in (F32, 3, -1, 16):                           # no fp32 pools
        assert "unknown format" in _sparse_rejects(native_lib, fmt=fmt)
    for dims in (dict(face_size=0), dict(num_planes=0), dict(batch=-1)):
        assert "bad dims" in _sparse_rejects(native_lib, **dims)
    assert "at most 128 planes" in _sparse_rejects(native_lib, code=MSI_E_UNSUPPORTED, num_planes=129)
    assert "at most 128 planes" in _sparse_rejects(native_lib, code=MSI_E_UNSUPPORTED, num_planes=129, face_size=24)     # the planes before S % 16
    for s in (24, 12, 8, 20):
        assert "S % 16" in _sparse_rejects(native_lib, code=MSI_E_UNSUPPORTED, face_size=s)
        assert "S % 16" in _sparse_rejects(native_lib, code=MSI_E_UNSUPPORTED, face_size=s, batch=0)
        assert "S % 16" in _sparse_rejects(native_lib, code=MSI_E_UNSUPPORTED, face_size=s, views=0)                     # S % 16 before the views
    for views in (0, -1):
        assert "views must be >= 1" in _sparse_rejects(native_lib, views=views)
    assert "bad output size" in _sparse_rejects(native_lib, out_height=0)
    assert "2^31 bytes" in _sparse_rejects(native_lib, face_size=4096, num_planes=32, fmt=RGBA8)      # 12 GiB of dense faces
    assert "2^31 bytes" in _sparse_rejects(native_lib, face_size=2048, num_planes=16, fmt=RGBA16F)    # 3 GiB
    assert "too many target pixels" in _sparse_rejects(native_lib, out_height=1 << 30, out_width=1 << 14)


@pytest.mark.parametrize("fmt", [RGBA8, RGBA16F])
def test_sparse_passes_a_valid_empty_batch(native_lib, fmt):
    ptrs = [_p(k) for k in range(SPARSE_INPUTS + 3)]
    assert _sparse(native_lib.lib, ptrs, fmt=fmt, batch=0) == 0
    for unused in (SPARSE_INPUTS, SPARSE_INPUTS + 1, SPARSE_INPUTS + 2):
        one = list(ptrs)
        one[unused] = None
        assert _sparse(native_lib.lib, one, fmt=fmt, batch=0) == 0
    assert _sparse(native_lib.lib, ptrs, fmt=fmt, batch=0, face_size=1024, num_planes=32) == 0        # 768 MiB / 1.5 GiB of dense faces
