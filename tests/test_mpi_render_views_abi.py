"""CPU-only checks of the many-views MPI render's plumbing: msi_mpi_render_views is exported and bound with the signature
the header declares (ABI still 9: a new entry point changes no existing signature), and its argument checks reject bad calls
with the documented code before any launch.  No kernel is launched here: every call below fails its validation, or has an
empty batch, before it could reach a device (the non-zero dummy pointers are never dereferenced)."""
import pytest

from tests.util import check_binding

MSI_E_BADARG, MSI_E_UNSUPPORTED = -1, -3
F32, RGBA8, RGBA16F = 0, 1, 2


def test_mpi_render_views_is_exported_and_bound(native_lib):
    assert "msi_mpi_render_views" in native_lib.SIGNATURES
    assert hasattr(native_lib.lib, "msi_mpi_render_views")
    assert native_lib.MSI_ABI_VERSION == 9
    assert native_lib.lib.msi_abi_version() == 9


def test_header_and_binding_agree_on_the_signature(native_lib):
    names = check_binding(native_lib, "msi_mpi_render_views", int32_and_pointers=True)
    assert names == ["layers", "format", "tgt_pose", "intrinsics", "tgt_intrinsics_inv", "depths", "batch", "views", "height",
                     "width", "num_planes", "out_height", "out_width", "out_rgb", "out_depth", "stream"]


def _ptrs():
    # layers, tgt_pose, intrinsics, tgt_intrinsics_inv, depths, out_rgb, out_depth
    return [4096 * (k + 1) for k in range(7)]


def _call(lib, ptrs, fmt=F32, batch=2, views=3, height=16, width=32, num_planes=4, out_height=16, out_width=32):
    layers, pose, intr, intr_inv, depths, out_rgb, out_depth = ptrs
    return lib.msi_mpi_render_views(layers, fmt, pose, intr, intr_inv, depths, batch, views, height, width, num_planes,
                                    out_height, out_width, out_rgb, out_depth, None)


def _rejects(native_lib, what=None, code=MSI_E_BADARG, **kw):
    ptrs = _ptrs()
    for k, v in (what or {}).items():
        ptrs[k] = v
    assert _call(native_lib.lib, ptrs, **kw) == code
    msg = native_lib.last_error()
    assert "mpi_render_views" in msg
    return msg


@pytest.mark.parametrize("fmt", [F32, RGBA8, RGBA16F])
@pytest.mark.parametrize("null", [0, 1, 2, 3, 4])
def test_rejects_null_inputs(native_lib, fmt, null):
    assert "null pointer" in _rejects(native_lib, {null: None}, fmt=fmt)


def test_rejects_both_outputs_null(native_lib):
    assert "both outputs are NULL" in _rejects(native_lib, {5: None, 6: None})


@pytest.mark.parametrize("views", [0, -1])
def test_rejects_views_below_one(native_lib, views):
    assert "views" in _rejects(native_lib, views=views)


@pytest.mark.parametrize("oh,ow", [(0, 32), (16, 0), (-4, 8), (0, 0)])
def test_rejects_an_output_size_below_one(native_lib, oh, ow):
    assert "output size" in _rejects(native_lib, out_height=oh, out_width=ow)


@pytest.mark.parametrize("dims", [dict(height=0), dict(width=0), dict(num_planes=0), dict(batch=-1), dict(height=-3)])
def test_rejects_bad_dims(native_lib, dims):
    assert "bad dims" in _rejects(native_lib, **dims)


@pytest.mark.parametrize("fmt", [3, -1, 16])
def test_rejects_an_unknown_format(native_lib, fmt):
    assert "unknown format" in _rejects(native_lib, fmt=fmt)


def test_rejects_129_planes_as_unsupported(native_lib):
    assert "at most 128 planes" in _rejects(native_lib, code=MSI_E_UNSUPPORTED, num_planes=129)
    assert _call(native_lib.lib, _ptrs(), batch=0, num_planes=128) == 0      # (128 is the limit, not beyond it)


def test_rejects_stacks_of_2_24_texels(native_lib):
    assert "2^24" in _rejects(native_lib, height=4096, width=4096)


@pytest.mark.parametrize("kw", [dict(out_height=1 << 30, out_width=1 << 14),                 # one view alone
                                dict(views=1 << 20, out_height=1 << 12, out_width=1 << 12),  # the views
                                dict(batch=1 << 20, views=1 << 8, out_height=1 << 11, out_width=1 << 10),
                                dict(batch=1 << 30, views=1 << 30, out_height=1 << 30, out_width=1 << 30)])
def test_rejects_grid_overflow(native_lib, kw):
    assert "too many target pixels" in _rejects(native_lib, **kw)


@pytest.mark.parametrize("fmt", [F32, RGBA8, RGBA16F])
def test_a_valid_empty_batch_passes_validation(native_lib, fmt):
    """Control for the cases above: the same arguments with nothing wrong and B = 0 are accepted (nothing to launch), with
    both outputs or either one."""
    assert _call(native_lib.lib, _ptrs(), fmt=fmt, batch=0) == 0
    for out in (5, 6):
        ptrs = _ptrs()
        ptrs[out] = None
        assert _call(native_lib.lib, ptrs, fmt=fmt, batch=0) == 0
