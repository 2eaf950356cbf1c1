"""CPU-only checks of msi_hres_layers (the high-res layer stack in one launch, fp32 and / or packed): the symbol is exported
and bound (19 arguments, ABI still 9: a new entry point changes no existing signature), the header states its bit-identity
contract, and its argument checks reject bad calls in the documented order -- unknown format with a layers_out, both outputs
NULL, other NULL pointers, bad dims, num_planes % 4 (MSI_E_UNSUPPORTED), the size limits -- with a message that names
hres_layers.  No kernel is launched here: every call fails its validation or has an empty batch (the non-zero dummy pointers
are never dereferenced)."""
import pytest

MSI_OK, MSI_E_BADARG, MSI_E_UNSUPPORTED = 0, -1, -3
F32, RGBA8, RGBA16F = 0, 1, 2
NAME = "msi_hres_layers"
POINTERS = ("ref", "src", "pose0", "pose1", "intr", "depths", "trig", "bw", "al")


def _call(lib, rgba=4096, layers=8192, fmt=RGBA8, batch=1, h=16, w=32, hh=40, hw=88, d=8, **ptr):
    p = [ptr.get(k, 256 * (n + 1)) for n, k in enumerate(POINTERS)]
    # (ref_image, src_image, ref_curr_pose, src_curr_pose, intrinsics, depths, trig, blend_weights, alphas,
    #  batch, low_height, low_width, height, width, num_planes, rgba_native, layers_out, format, stream)
    return lib.msi_hres_layers(*p, batch, h, w, hh, hw, d, rgba, layers, fmt, None)


def _fails(native_lib, code=MSI_E_BADARG, **kw):
    assert _call(native_lib.lib, **kw) == code
    msg = native_lib.last_error()
    assert "hres_layers" in msg, msg
    return msg


def test_symbol_is_exported_and_bound(native_lib):
    assert NAME in native_lib.SIGNATURES
    assert hasattr(native_lib.lib, NAME)
    res, args = native_lib.SIGNATURES[NAME]
    assert len(args) == 19
    assert native_lib.MSI_ABI_VERSION == 9
    assert native_lib.lib.msi_abi_version() == 9


def test_header_declares_the_entry_point_and_its_contract(native_lib):
    import re
    from tests.util import check_binding, header_text
    header = header_text(comments=True)
    m = re.search(r"/\*((?:(?!\*/).)*)\*/\s*int\s+msi_hres_layers\s*\(", header, re.S)
    assert m, "msi_hres_layers is not declared behind its comment"
    assert len(check_binding(native_lib, NAME, int32_and_pointers=True)) == 19
    assert "bit-identical" in m.group(1)
    for word in ("msi_ods_sweep_volume", "msi_resize_bilinear_f32", "msi_assemble_rgba_scaled_f32", "msi_pack_layers"):
        assert word in m.group(1), word
    assert re.search(r"#define\s+MSI_ABI_VERSION\s+9\b", header)


@pytest.mark.parametrize("fmt", [3, -1, 255, F32])
@pytest.mark.parametrize("rgba", [4096, None])
def test_unknown_format_with_a_layers_out_comes_first(native_lib, fmt, rgba):
    """(before every other check: the other arguments are bad as well)"""
    assert "unknown format" in _fails(native_lib, fmt=fmt, rgba=rgba, ref=None, h=0, d=3)


@pytest.mark.parametrize("fmt", [RGBA8, RGBA16F, F32, 3, -1])
def test_both_outputs_null_comes_second(native_lib, fmt):
    """(the format is ignored when layers_out is NULL: an unknown one is not what is reported)"""
    assert "null pointer" in _fails(native_lib, rgba=None, layers=None, fmt=fmt, h=0, d=3)


@pytest.mark.parametrize("which", POINTERS)
def test_other_null_pointers_come_before_the_dims(native_lib, which):
    assert "null pointer" in _fails(native_lib, h=0, d=3, **{which: None})


@pytest.mark.parametrize("dims", [dict(batch=-1), dict(h=0), dict(w=0), dict(hh=0), dict(hw=-4), dict(d=0)])
def test_bad_dims_come_before_the_layer_count(native_lib, dims):
    kw = dict(d=3)
    kw.update(dims)
    assert "bad dims" in _fails(native_lib, **kw)


@pytest.mark.parametrize("d", [1, 3, 6, 30])
def test_layer_counts_that_are_no_multiple_of_four_are_unsupported(native_lib, d):
    """(before the size limits: the shape is too large as well)"""
    assert "multiple of 4" in _fails(native_lib, code=MSI_E_UNSUPPORTED, d=d, hh=4096, hw=4096)


@pytest.mark.parametrize("dims", [dict(hh=4096, hw=4096),            # Hh * Wh = 2^24
                                  dict(hh=65536, hw=8),              # Hh > 65535
                                  dict(batch=65536),
                                  dict(h=4096, w=4096, d=128)])      # h * w * D = 2^31
def test_size_limits(native_lib, dims):
    assert "too large" in _fails(native_lib, **dims)


@pytest.mark.parametrize("rgba,layers,fmt", [(4096, None, 77), (None, 8192, RGBA8), (4096, 8192, RGBA16F)])
def test_an_empty_batch_is_ok_without_a_launch(native_lib, rgba, layers, fmt):
    assert _call(native_lib.lib, batch=0, rgba=rgba, layers=layers, fmt=fmt) == MSI_OK


def test_the_three_launch_entry_points_are_still_there(native_lib):
    for name in ("msi_ods_sweep_volume", "msi_resize_bilinear_f32", "msi_assemble_rgba_scaled_f32", "msi_pack_layers"):
        assert name in native_lib.SIGNATURES and hasattr(native_lib.lib, name)


def test_layer_format_requests_are_validated_before_any_device_work(native_lib):
    """MSI.hres_layers hands layer_format to MSI._layer_formats first -- a static method: no device needed."""
    import inspect
    from matryodshka_amd.msi import MSI
    sig = inspect.signature(MSI.hres_layers)
    assert list(sig.parameters) == ["self", "blend_weights", "alphas", "raw_hres_ref_image", "raw_hres_src_image", "ref_pose",
                                    "src_pose", "planes", "intrinsics", "ref_pose_inv", "layer_format"]
    assert sig.parameters["layer_format"].default == 'f32' and sig.parameters["ref_pose_inv"].default is None
    assert MSI._layer_formats('f32') == (True, None)
    assert MSI._layer_formats(('f32', 'rgba8')) == (True, 'rgba8')

    class NoDevice(object):            # stands in for a model: anything beyond the format check would touch these
        _layer_formats = staticmethod(MSI._layer_formats)

        def __getattr__(self, name):
            raise AssertionError("hres_layers touched %s before validating layer_format" % name)

    fn = inspect.unwrap(MSI.hres_layers)
    for bad in ('rgba4', ('rgba8', 'rgba16f'), ('f32', 'rgba8', 'rgba16f'), (), None, 1, ('f32', 7)):
        with pytest.raises(ValueError) as e:
            fn(NoDevice(), None, None, None, None, None, None, None, None, layer_format=bad)
        assert "f32" in str(e.value) and "rgba8" in str(e.value) and "rgba16f" in str(e.value)
