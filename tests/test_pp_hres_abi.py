"""CPU-only checks of the PP high-res builder's plumbing: msi_pp_hres_layers, msi_hres_index_tiles_edge and msi_pp_hres_layers_sparse
are exported, bound and declared with one signature (ABI still 9) -- their siblings' parameters, without `trig` --, each is defined in
exactly one geometry unit, and their argument checks reject bad calls before any HIP call.  No kernel is launched here: every native
call below fails its validation, or has an empty batch, before it could reach a device (the dummy pointers are never dereferenced).
MSI.mpi_hres_layers' own refusals need an MSI object and are in tests/test_gpu_pp_hres.py."""
import os
import re

import pytest

from tests.util import check_binding, header_text

MSI_E_BADARG, MSI_E_UNSUPPORTED = -1, -3
F32, RGBA8, RGBA16F = 0, 1, 2
SIBLING = {"msi_pp_hres_layers": "msi_hres_layers", "msi_hres_index_tiles_edge": "msi_hres_index_tiles",
           "msi_pp_hres_layers_sparse": "msi_hres_layers_sparse"}
N_PTRS = {"msi_pp_hres_layers": 10, "msi_hres_index_tiles_edge": 3, "msi_pp_hres_layers_sparse": 11}
SPARSE = ("msi_hres_index_tiles_edge", "msi_pp_hres_layers_sparse")
UNIT = {"msi_pp_hres_layers": "geo_planar_hres.hip", "msi_hres_index_tiles_edge": "geo_sparse_hres.hip",
        "msi_pp_hres_layers_sparse": "geo_planar_hres.hip"}


def test_exported_and_bound(native_lib):
    for name in SIBLING:
        assert name in native_lib.SIGNATURES
        assert hasattr(native_lib.lib, name)
    assert native_lib.MSI_ABI_VERSION == 9
    assert native_lib.lib.msi_abi_version() == 9
    assert "#define MSI_ABI_VERSION 9" in header_text()


@pytest.mark.parametrize("name", sorted(SIBLING))
def test_the_parameters_are_the_siblings_without_trig(native_lib, name):
    want = [p for p in check_binding(native_lib, SIBLING[name], int32_and_pointers=True) if p != "trig"]
    assert check_binding(native_lib, name, int32_and_pointers=True) == want


def test_each_is_defined_once_in_its_geometry_unit():
    from matryodshka_amd import build
    assert "geo_planar_hres.hip" in build.GEO_UNITS
    for name in SIBLING:
        pattern = re.compile(r"^int\s+%s\(" % name, re.M)
        hits = {}
        for unit in sorted(os.listdir(build.CSRC)):
            if unit.endswith((".hip", ".cpp")):
                with open(os.path.join(build.CSRC, unit)) as f:
                    n = len(pattern.findall(f.read()))
                if n:
                    hits[unit] = n
        assert hits == {UNIT[name]: 1}, (name, hits)
        flags = dict(build.SOURCES)[UNIT[name]]
        assert "-ffp-contract=off" in flags and "-fno-slp-vectorize" in flags


def test_the_pp_texel_is_defined_once_and_both_kernels_call_it():
    from matryodshka_amd import build
    texts = {u: open(os.path.join(build.CSRC, u)).read() for u in os.listdir(build.CSRC) if u.endswith((".hip", ".h", ".cpp", ".inc"))}
    # the PP source, its pixel state, and where a plane point lands in one source image: one definition each
    for pattern in (r"struct PpHres : ", r"PpHres pp_hres\(", r"TapsB pp_hres_source_taps\("):
        assert {u: len(re.findall(pattern, t)) for u, t in texts.items() if re.search(pattern, t)} == {"geometry_device.h": 1}, pattern
    # the dense kernel calls the one texel, the sparse kernel the texel's steps, both on the PP source; the source's taps calls the one definition
    # (the group loops are written in these kernels: as the shared bodies they missed the timing margin, profiles/hres_bodies_isa.txt)
    unit = texts["geo_planar_hres.hip"]
    for kernel, body_name in (("pp_hres_layers_kernel", "hres_texel(px, "), ("pp_hres_layers_sparse_kernel", "px.taps(")):
        body = unit[unit.index("\n%s(" % kernel):]
        body = body[:body.index("\n}\n")]
        assert body_name in body and "PpHres" in body and "pp_hres(" in body and "make_taps" not in body, kernel
    header = texts["geometry_device.h"]
    source = header[header.index("struct PpHres : "):]
    source = source[:source.index("\n};\n")]
    assert "HresTaps taps(" in source and "pp_hres_source_taps(" in source and "HresRgb fetch(" in source


# ------------------------------------------------------------------------------------------------ the argument checks
def _p(k):
    return 4096 * (k + 1)


def _call(lib, name, ptrs, fmt=RGBA8, batch=2, low_height=8, low_width=16, height=16, width=32, num_planes=4):
    dims = [batch, low_height, low_width, height, width, num_planes]
    if name == "msi_hres_index_tiles_edge":      # alphas, table_out, counts_out
        a, t, c = ptrs
        return lib.msi_hres_index_tiles_edge(a, fmt, *(dims + [t, c, None]))
    return getattr(lib, name)(*(list(ptrs[:8]) + dims + list(ptrs[8:]) + [fmt, None]))


def _rejects(native_lib, name, code=MSI_E_BADARG, null=None, **kw):
    ptrs = [_p(k) for k in range(N_PTRS[name])]
    if null is not None:
        ptrs[null] = None
    assert _call(native_lib.lib, name, ptrs, **kw) == code
    msg = native_lib.last_error()
    assert name[len("msi_"):] in msg
    return msg


@pytest.mark.parametrize("name", sorted(SIBLING))
def test_null_inputs_and_unknown_formats_are_refused(native_lib, name):
    inputs = N_PTRS[name] if name in SPARSE else 8              # (msi_pp_hres_layers: either output may be NULL, not both)
    for null in range(inputs):
        assert "null pointer" in _rejects(native_lib, name, null=null)
    for fmt in (3, -1) + ((F32,) if name in SPARSE else ()):
        assert "unknown format" in _rejects(native_lib, name, fmt=fmt)
    if name == "msi_pp_hres_layers":
        ptrs = [_p(k) for k in range(8)] + [None, None]
        assert _call(native_lib.lib, name, ptrs) == MSI_E_BADARG and "both outputs are NULL" in native_lib.last_error()
        assert _call(native_lib.lib, name, [_p(k) for k in range(9)] + [None], fmt=77, batch=0) == 0    # (no packed output: the format is not read)


@pytest.mark.parametrize("name", sorted(SIBLING))
def test_bad_sizes_are_refused(native_lib, name):
    for dims in (dict(height=0), dict(width=0), dict(num_planes=0), dict(batch=-1), dict(low_height=0), dict(low_width=-1)):
        assert "bad dims" in _rejects(native_lib, name, **dims)
    for d in (2, 6, 9):
        assert "multiple of 4" in _rejects(native_lib, name, code=MSI_E_UNSUPPORTED, num_planes=d)
    # the perspective sweep's own: H or W equal to 1 (uv_grid divides by n - 1)
    assert "H > 1 and W > 1" in _rejects(native_lib, name, height=1)
    assert "H > 1 and W > 1" in _rejects(native_lib, name, width=1)
    assert "H > 1 and W > 1" in _rejects(native_lib, name, height=1, batch=0)                          # (an empty batch is still validated)
    assert "2^24" in _rejects(native_lib, name, height=4096, width=4096)
    assert "2^31" in _rejects(native_lib, name, low_height=1 << 14, low_width=1 << 14, num_planes=8)


@pytest.mark.parametrize("name", SPARSE)
def test_the_sparse_entry_points_want_whole_tiles(native_lib, name):
    assert "H % 4" in _rejects(native_lib, name, code=MSI_E_UNSUPPORTED, height=18)
    assert "W % 16" in _rejects(native_lib, name, code=MSI_E_UNSUPPORTED, width=40)
    assert "multiple of 4" in _rejects(native_lib, name, code=MSI_E_UNSUPPORTED, fmt=F32, height=18, num_planes=6)   # (the siblings' order)
    assert "unknown format" in _rejects(native_lib, name, fmt=F32, height=18)


@pytest.mark.parametrize("name", sorted(SIBLING))
@pytest.mark.parametrize("fmt", [RGBA8, RGBA16F])
def test_a_valid_empty_batch_returns_ok(native_lib, name, fmt):
    ptrs = [_p(k) for k in range(N_PTRS[name])]
    assert _call(native_lib.lib, name, ptrs, fmt=fmt, batch=0) == 0
    assert _call(native_lib.lib, name, ptrs, fmt=fmt, batch=0, height=4096, width=4080) == 0
