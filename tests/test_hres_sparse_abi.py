"""CPU-only checks of the sparse high-res stack's plumbing: msi_hres_index_tiles and msi_hres_layers_sparse are exported, bound and
declared with one signature (ABI still 9), defined in exactly one unit -- a geometry unit, the one that holds the tile constants
and the scan they share with msi_sparse_index_tiles --, and their argument checks reject bad calls with the documented code and
text before any HIP call.  No kernel is launched here: every native call below fails its validation, or has an empty batch, before
it could reach a device (the dummy pointers are never dereferenced).  The harness's --msi_hres_sparse refusals and its --help need
no device either; MSI.hres_layers_sparse's own refusals need an MSI object and are in tests/test_gpu_hres_sparse.py."""
import os
import re

import pytest

from tests.util import check_binding, header_text

MSI_E_BADARG, MSI_E_UNSUPPORTED = -1, -3
F32, RGBA8, RGBA16F = 0, 1, 2
HRES_INPUTS = ["ref_image", "src_image", "ref_curr_pose", "src_curr_pose", "intrinsics", "depths", "trig", "blend_weights", "alphas",
               "batch", "low_height", "low_width", "height", "width", "num_planes"]
PARAMS = {
    "msi_hres_index_tiles": ["alphas", "format", "batch", "low_height", "low_width", "height", "width", "num_planes", "table_out",
                             "counts_out", "stream"],
    "msi_hres_layers_sparse": HRES_INPUTS + ["table", "layer_start", "pool_out", "format", "stream"],
}
N_PTRS = {"msi_hres_index_tiles": 3, "msi_hres_layers_sparse": 12}


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


def test_the_sparse_form_takes_the_inputs_of_msi_hres_layers_in_its_order(native_lib):
    assert check_binding(native_lib, "msi_hres_layers")[:len(HRES_INPUTS)] == HRES_INPUTS


def test_defined_once_in_a_geometry_unit():
    from matryodshka_amd import build
    for name in PARAMS:
        pattern = re.compile(r"^int\s+%s\(" % name, re.M)
        hits = {}
        for unit in sorted(os.listdir(build.CSRC)):
            if unit.endswith((".hip", ".cpp")):
                with open(os.path.join(build.CSRC, unit)) as f:
                    n = len(pattern.findall(f.read()))
                if n:
                    hits[unit] = n
        assert len(hits) == 1 and list(hits.values()) == [1], (name, hits)
        unit = list(hits)[0]
        assert unit in build.GEO_UNITS
        flags = dict(build.SOURCES)[unit]
        assert "-ffp-contract=off" in flags and "-fno-slp-vectorize" in flags


def test_the_texel_and_the_tile_are_each_defined_once():
    """One definition of the high-res texel, of the ODS source and of the two launchers, in the headers the kernels' units include, and one of the
    tile and of the scan.  (The builders' group loops are written per kernel: as shared bodies they missed the timing margin,
    profiles/hres_bodies_isa.txt.)"""
    from matryodshka_amd import build
    texts = {u: open(os.path.join(build.CSRC, u)).read() for u in os.listdir(build.CSRC) if u.endswith((".hip", ".h", ".cpp", ".inc"))}
    for pattern, where in ((r"float4 hres_texel\(", "geometry_device.h"), (r"struct OdsHres \{", "geometry_device.h"),
                           (r"void hres_dense_launch\(", "geometry_device.h"), (r"int hres_sparse_launch\(", "geo_sparse.h"),
                           (r"constexpr int TILE_H = ", "geo_sparse.h"), (r"\nsparse_scan_kernel\(", "geo_sparse.hip"),
                           (r"\nint sparse_dims\(", "geo_sparse.hip")):
        assert {u: len(re.findall(pattern, t)) for u, t in texts.items() if re.search(pattern, t)} == {where: 1}, pattern
    # the dense kernel calls the one texel, the sparse kernel the texel's steps, both on the ODS source; the source's taps is where the sweep's
    # functions are called
    for unit, kernel, body_name in (("geo_layers.hip", "hres_layers_kernel", "hres_texel(px, "),
                                    ("geo_sparse_hres.hip", "hres_layers_sparse_kernel", "px.taps(")):
        body = texts[unit][texts[unit].index("\n%s(" % kernel):]
        body = body[:body.index("\n}\n")]
        assert body_name in body and "OdsHres" in body and "ods_quad" not in body and "gather3(" not in body, unit
    header = texts["geometry_device.h"]
    source = header[header.index("struct OdsHres {"):]
    source = source[:source.index("\n};\n")]
    assert "HresTaps taps(" in source and "ods_quad(" in source and "HresRgb fetch(" in source
    texel = header[header.index("float4 hres_texel("):]
    texel = texel[:texel.index("\n}\n")]
    assert "src.taps(" in texel and "src.fetch(" in texel and "hres_blend(" in texel
    sparse = texts["geo_sparse_hres.hip"][texts["geo_sparse_hres.hip"].index("\nhres_layers_sparse_kernel("):]
    sparse = sparse[:sparse.index("\n}\n")]
    assert "px.taps(" in sparse and "px.fetch(" in sparse and "hres_blend(" in sparse


# ------------------------------------------------------------------------------------------------ the argument checks
def _p(k):
    return 4096 * (k + 1)


def _call(lib, name, ptrs, fmt=RGBA8, batch=2, low_height=8, low_width=16, height=16, width=32, num_planes=4):
    if name == "msi_hres_index_tiles":        # alphas, table_out, counts_out
        a, t, c = ptrs
        return lib.msi_hres_index_tiles(a, fmt, batch, low_height, low_width, height, width, num_planes, t, c, None)
    return lib.msi_hres_layers_sparse(*(list(ptrs[:9]) + [batch, low_height, low_width, height, width, num_planes] + list(ptrs[9:]) + [fmt, None]))


def _rejects(native_lib, name, code=MSI_E_BADARG, null=None, **kw):
    ptrs = [_p(k) for k in range(N_PTRS[name])]
    if null is not None:
        ptrs[null] = None
    assert _call(native_lib.lib, name, ptrs, **kw) == code
    msg = native_lib.last_error()
    assert name[len("msi_"):] in msg
    return msg


@pytest.mark.parametrize("name", sorted(PARAMS))
def test_entry_points_reject_bad_calls(native_lib, name):
    for null in range(N_PTRS[name]):
        assert "null pointer" in _rejects(native_lib, name, null=null)
    for fmt in (F32, 3, -1):                                                  # (fp32 pools are not built)
        assert "unknown format" in _rejects(native_lib, name, fmt=fmt)
    for dims in (dict(height=0), dict(width=0), dict(num_planes=0), dict(batch=-1), dict(low_height=0), dict(low_width=-1)):
        assert "bad dims" in _rejects(native_lib, name, **dims)
    assert "H % 4" in _rejects(native_lib, name, code=MSI_E_UNSUPPORTED, height=18)
    assert "W % 16" in _rejects(native_lib, name, code=MSI_E_UNSUPPORTED, width=40)
    for d in (2, 6):
        assert "multiple of 4" in _rejects(native_lib, name, code=MSI_E_UNSUPPORTED, num_planes=d)
    assert "2^24" in _rejects(native_lib, name, height=4096, width=4096)
    assert "2^31" in _rejects(native_lib, name, low_height=1 << 14, low_width=1 << 14, num_planes=8)


@pytest.mark.parametrize("name", sorted(PARAMS))
def test_the_checks_come_in_the_documented_order(native_lib, name):
    """msi_hres_layers' checks, then the tile entry points': a call that is wrong in several ways reports the first."""
    assert "null pointer" in _rejects(native_lib, name, null=0, fmt=F32, height=18, num_planes=6)
    assert "bad dims" in _rejects(native_lib, name, fmt=F32, height=0, num_planes=6)
    assert "multiple of 4" in _rejects(native_lib, name, code=MSI_E_UNSUPPORTED, fmt=F32, height=18, num_planes=6)
    assert "2^24" in _rejects(native_lib, name, fmt=F32, height=4098, width=4096)
    assert "unknown format" in _rejects(native_lib, name, fmt=F32, height=18)
    assert "H % 4" in _rejects(native_lib, name, code=MSI_E_UNSUPPORTED, height=18, width=40)
    assert "H % 4" in _rejects(native_lib, name, code=MSI_E_UNSUPPORTED, height=18, batch=0)      # (an empty batch is still validated)


@pytest.mark.parametrize("name", sorted(PARAMS))
@pytest.mark.parametrize("fmt", [RGBA8, RGBA16F])
def test_a_valid_empty_batch_passes_validation(native_lib, name, fmt):
    ptrs = [_p(k) for k in range(N_PTRS[name])]
    assert _call(native_lib.lib, name, ptrs, fmt=fmt, batch=0) == 0
    assert _call(native_lib.lib, name, ptrs, fmt=fmt, batch=0, height=4096, width=4080) == 0


# ------------------------------------------------------------------------------------------------ the harness, without a device
def test_harness_help_names_the_flag(capsys):
    from matryodshka_amd import harness
    with pytest.raises(SystemExit) as e:
        harness.main(["--help"])                  # (argparse %-expands every help string)
    assert e.value.code == 0
    out = " ".join(capsys.readouterr().out.split())
    assert "--msi_hres_sparse" in out and "--hres_height % 4 == 0" in out and "--hres_width % 16 == 0" in out and "hres_sparse.json" in out
    assert "--msi_sparse" in out and "high_res_only is refused" in out        # (--msi_sparse keeps its text)


@pytest.mark.parametrize("extra,text", [
    (["--msi_hres_sparse", "--test_type", "high_res"], "needs --msi_format"),
    (["--msi_hres_sparse", "--msi_format", "rgba8"], "high_res"),
    (["--msi_hres_sparse", "--msi_format", "rgba8", "--test_type", "on_video"], "high_res"),
    (["--msi_hres_sparse", "--msi_format", "rgba8", "--test_type", "high_res", "--hres_height", "18"], "--hres_height % 4 == 0"),
    (["--msi_hres_sparse", "--msi_format", "rgba16f", "--test_type", "high_res_only", "--hres_width", "40"], "--hres_width % 16 == 0")])
def test_harness_refuses_msi_hres_sparse_where_it_cannot_apply(capsys, extra, text):
    """Argument errors come before the model is built: no device is needed."""
    from matryodshka_amd import harness
    with pytest.raises(SystemExit) as e:
        harness.main(["--cameras_glob", "none/*.txt"] + extra)
    assert e.value.code == 2
    err = capsys.readouterr().err
    assert "--msi_hres_sparse" in err and text in err
