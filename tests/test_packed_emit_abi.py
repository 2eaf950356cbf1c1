"""CPU-only checks of msi_net_plan_forward_layers (the fused tail emitting an rgba8 / rgba16f stack): the symbol is exported
and bound (ABI still 9: a new entry point changes no existing signature), and its argument checks reject bad calls with
MSI_E_BADARG in the documented order -- unknown format, both outputs NULL, then the checks of msi_net_plan_forward_rgba (NULL
plan first) -- with a message that names net_forward_layers.  No kernel is launched here: every call fails its validation
before a plan is touched (the non-zero dummy pointers are never dereferenced)."""
import pytest

MSI_E_BADARG = -1
F32, RGBA8, RGBA16F = 0, 1, 2
NAME = "msi_net_plan_forward_layers"


def _call(lib, plan=None, rgba=4096, layers=8192, fmt=RGBA8):
    # (plan, packed, net_input, rgba_native, layers_out, format, blend_weights, alphas, pred, workspace, workspace_bytes, stream, event)
    return lib.msi_net_plan_forward_layers(plan, 256, 512, rgba, layers, fmt, None, None, None, 1024, 1 << 20, None, None)


def _bad(native_lib, **kw):
    assert _call(native_lib.lib, **kw) == MSI_E_BADARG
    msg = native_lib.last_error()
    assert "net_forward_layers" in msg, msg
    return msg


def test_symbol_is_exported_and_bound(native_lib):
    assert NAME in native_lib.SIGNATURES
    assert hasattr(native_lib.lib, NAME)
    res, args = native_lib.SIGNATURES[NAME]
    assert len(args) == 13
    assert native_lib.MSI_ABI_VERSION == 9
    assert native_lib.lib.msi_abi_version() == 9


def test_header_declares_the_entry_point_and_its_contract():
    import re
    from tests.util import declared, header_text
    header = header_text(comments=True)
    assert len(declared(NAME)[1]) == 13
    assert re.search(r"#define\s+MSI_ABI_VERSION\s+9\b", header)
    assert "bit-identical to msi_pack_layers" in header


@pytest.mark.parametrize("fmt", [3, -1, 255])
@pytest.mark.parametrize("rgba", [4096, None])
def test_rejects_unknown_formats(native_lib, fmt, rgba):
    assert "unknown format" in _bad(native_lib, fmt=fmt, rgba=rgba)


def test_f32_is_not_a_format_of_layers_out(native_lib):
    assert "unknown format" in _bad(native_lib, fmt=F32)


@pytest.mark.parametrize("fmt", [RGBA8, RGBA16F, F32, 3, -1])
def test_rejects_both_outputs_null(native_lib, fmt):
    """(the format is ignored when layers_out is NULL: an unknown one is not what is reported)"""
    assert "null pointer" in _bad(native_lib, rgba=None, layers=None, fmt=fmt)


@pytest.mark.parametrize("fmt", [RGBA8, RGBA16F])
@pytest.mark.parametrize("rgba,layers", [(4096, 8192), (None, 8192), (4096, None)])
def test_rejects_a_null_plan(native_lib, fmt, rgba, layers):
    assert "null plan" in _bad(native_lib, fmt=fmt, rgba=rgba, layers=layers)


def test_the_fp32_entry_point_still_names_itself(native_lib):
    """msi_net_plan_forward_rgba runs the same checks behind the new entry point: its error texts keep their name."""
    assert native_lib.lib.msi_net_plan_forward_rgba(None, 256, 512, 4096, None, None, None, 1024, 1 << 20, None, None) == MSI_E_BADARG
    msg = native_lib.last_error()
    assert "net_forward_rgba" in msg and "null plan" in msg, msg


def test_layer_format_requests_are_validated_before_any_device_work(native_lib):
    """MSI._layer_formats (what infer_layers / infer_msi do with layer_format) -- a static method: no device needed."""
    from matryodshka_amd.msi import MSI
    assert MSI._layer_formats('f32') == (True, None)
    assert MSI._layer_formats('rgba8') == (False, 'rgba8')
    assert MSI._layer_formats(('f32', 'rgba16f')) == (True, 'rgba16f')
    assert MSI._layer_formats(('rgba16f', 'f32')) == (True, 'rgba16f')
    for bad in ('rgba4', ('rgba8', 'rgba16f'), ('f32', 'rgba8', 'rgba16f'), (), None, 1, ('f32', 7)):
        with pytest.raises(ValueError) as e:
            MSI._layer_formats(bad)
        assert "f32" in str(e.value) and "rgba8" in str(e.value) and "rgba16f" in str(e.value)
