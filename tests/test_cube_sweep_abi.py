"""CPU-only checks of the cube panorama-sampling entry points' plumbing: msi_cube_plane_sweep_f32, msi_cube_sweep_volume_bf16,
msi_cube_hres_layers and msi_cube_hres_layers_sparse are exported, bound and declared with one signature (ABI still 9), defined once in
geo_cube_sweep.hip, all sample through one device function, and their argument checks reject bad calls before any HIP call.  No kernel
is launched here: every native call below fails its validation, or has an empty batch, before it could reach a device (the dummy
pointers are never dereferenced)."""
import os
import re

import pytest

from tests.util import check_binding, header_text

MSI_E_BADARG, MSI_E_UNSUPPORTED = -1, -3
F32, RGBA8, RGBA16F = 0, 1, 2
# name -> number of pointer arguments (without the stream)
N_PTRS = {"msi_cube_plane_sweep_f32": 5, "msi_cube_sweep_volume_bf16": 7, "msi_cube_hres_layers": 10, "msi_cube_hres_layers_sparse": 11}
SWEEPS = ("msi_cube_plane_sweep_f32", "msi_cube_sweep_volume_bf16")
HRES = ("msi_cube_hres_layers", "msi_cube_hres_layers_sparse")


def test_exported_bound_and_declared(native_lib):
    for name in N_PTRS:
        assert name in native_lib.SIGNATURES and hasattr(native_lib.lib, name)
        params = check_binding(native_lib, name, int32_and_pointers=True)
        assert [p for p in ("batch", "pano_height", "pano_width", "face_size") if p in params] == ["batch", "pano_height", "pano_width", "face_size"]
    assert native_lib.MSI_ABI_VERSION == 9 and native_lib.lib.msi_abi_version() == 9
    assert "#define MSI_ABI_VERSION 9" in header_text()
    # the sweep's arguments as the header states them
    assert check_binding(native_lib, "msi_cube_plane_sweep_f32") == ["panorama", "face_pose", "intrinsics", "depths", "batch", "pano_height", "pano_width",
                                                                     "face_size", "num_depths", "psv", "psv_channels", "channel_offset", "stream"]


def test_defined_once_in_the_new_unit_and_one_sample_position():
    from matryodshka_amd import build
    assert "geo_cube_sweep.hip" in build.GEO_UNITS
    flags = dict(build.SOURCES)["geo_cube_sweep.hip"]
    assert "-ffp-contract=off" in flags and "-fno-slp-vectorize" in flags
    texts = {u: open(os.path.join(build.CSRC, u)).read() for u in os.listdir(build.CSRC) if u.endswith((".hip", ".h", ".cpp", ".inc"))}
    for name in N_PTRS:
        hits = {u: len(re.findall(r"^int\s+%s\(" % name, t, re.M)) for u, t in texts.items()}
        assert {u: n for u, n in hits.items() if n} == {"geo_cube_sweep.hip": 1}, (name, hits)
    assert {u: len(re.findall(r"TapsB cube_pano_taps\(", t)) for u, t in texts.items() if "TapsB cube_pano_taps(" in t} == {"geometry_device.h": 1}
    unit = texts["geo_cube_sweep.hip"]
    # each sweep kernel names the one body of its kind, each builder the texel or its steps, and all the source type that samples the panorama
    for kernel, body_name, source in (("cube_sweep_kernel", "sweep_body<", "cube_pano_source("),
                                      ("cube_sweep_volume_bf16_kernel", "sweep_volume_bf16_body<", "cube_pano_source("),
                                      ("cube_hres_layers_kernel", "hres_texel(px, ", "cube_hres("),
                                      ("cube_hres_layers_sparse_kernel", "px.taps(", "cube_hres(")):
        body = unit[unit.index("\n%s(" % kernel):]
        body = body[:body.index("\n}\n")]
        assert body_name in body and source in body and "atan2f" not in body and "asinf" not in body, kernel
    # both source types go through the one function, and nothing else in the library computes the position
    header = texts["geometry_device.h"]
    for text, struct, member in ((unit, "struct CubePanoSource {", "void sample("), (header, "struct CubeHres : ", "HresTaps taps(")):
        assert text.count(struct) == 1
        source = text[text.index(struct):]
        source = source[:source.index("\n};\n")]
        assert member in source and "cube_pano_taps(" in source and "atan2f" not in source and "asinf" not in source, struct
    for pattern in (r"CubeHres cube_hres\(", r"void sweep_body\(", r"void sweep_volume_bf16_body\("):
        assert {u: len(re.findall(pattern, t)) for u, t in texts.items() if re.search(pattern, t)} == {"geometry_device.h": 1}, pattern
    # the definition and two callers: CubePanoSource::sample (both sweep kernels) and CubeHres::taps (both high-res builders)
    assert sum(t.count("cube_pano_taps(") for t in texts.values()) == 3


# ------------------------------------------------------------------------------------------------ the argument checks
def _p(k):
    return 4096 * (k + 1)


def _call(lib, name, ptrs, batch=2, pano_height=16, pano_width=32, face_size=16, num=4, low_size=8, fmt=RGBA8, psv_channels=24, channel_offset=12):
    if name == "msi_cube_plane_sweep_f32":
        return lib.msi_cube_plane_sweep_f32(*(list(ptrs[:4]) + [batch, pano_height, pano_width, face_size, num, ptrs[4], psv_channels, channel_offset, None]))
    if name == "msi_cube_sweep_volume_bf16":
        return lib.msi_cube_sweep_volume_bf16(*(list(ptrs[:6]) + [batch, pano_height, pano_width, face_size, num, ptrs[6], None]))
    return getattr(lib, name)(*(list(ptrs[:8]) + [batch, pano_height, pano_width, low_size, face_size, num] + list(ptrs[8:]) + [fmt, None]))


def _rejects(native_lib, name, code=MSI_E_BADARG, null=None, **kw):
    ptrs = [_p(k) for k in range(N_PTRS[name])]
    if null is not None:
        ptrs[null] = None
    assert _call(native_lib.lib, name, ptrs, **kw) == code
    msg = native_lib.last_error()
    assert name[len("msi_"):].replace("_f32", "") in msg
    return msg


@pytest.mark.parametrize("name", sorted(N_PTRS))
def test_null_pointers_are_refused(native_lib, name):
    inputs = 8 if name == "msi_cube_hres_layers" else N_PTRS[name]       # (msi_cube_hres_layers: either output may be NULL, not both)
    for null in range(inputs):
        assert "null pointer" in _rejects(native_lib, name, null=null)
        assert "null pointer" in _rejects(native_lib, name, null=null, batch=0)
    if name == "msi_cube_hres_layers":
        ptrs = [_p(k) for k in range(8)] + [None, None]
        assert _call(native_lib.lib, name, ptrs) == MSI_E_BADARG and "both outputs are NULL" in native_lib.last_error()
        assert _call(native_lib.lib, name, [_p(k) for k in range(9)] + [None], fmt=77, batch=0) == 0       # (no packed output: the format is not read)


@pytest.mark.parametrize("name", sorted(N_PTRS))
def test_the_panorama_and_the_cubes_are_checked(native_lib, name):
    for dims in (dict(pano_height=1), dict(pano_width=1), dict(pano_height=0), dict(pano_width=-3), dict(batch=-1), dict(face_size=1), dict(face_size=0),
                 dict(num=0)):
        assert "bad dims" in _rejects(native_lib, name, **dims)
    assert "bad dims" in _rejects(native_lib, name, pano_height=1, batch=0)                                # (an empty batch is still validated)
    assert "Hp * Wp * 12 < 2^31" in _rejects(native_lib, name, pano_height=1 << 14, pano_width=1 << 14)
    assert "Hp * Wp * 12 < 2^31" in _rejects(native_lib, name, pano_height=13378, pano_width=13378)      # 13378^2 * 12 = 2^31 + 0.2 %
    # the leading dimension is 6 * batch: the grid's z takes 65535 faces
    assert "6 * batch" in _rejects(native_lib, name, batch=10923)
    assert "6 * batch" in _rejects(native_lib, name, batch=1 << 30)


@pytest.mark.parametrize("name", SWEEPS)
def test_the_sweeps_own_limits(native_lib, name):
    assert "65535" in _rejects(native_lib, name, face_size=65536)
    assert "S * S * 12 < 2^31" in _rejects(native_lib, name, face_size=13378)
    if name == "msi_cube_plane_sweep_f32":
        for window in (dict(channel_offset=-1), dict(channel_offset=13), dict(psv_channels=11, channel_offset=0), dict(channel_offset=2147483647)):
            assert "channel window" in _rejects(native_lib, name, **window)


@pytest.mark.parametrize("name", HRES)
def test_the_hres_builders_own_limits(native_lib, name):
    for fmt in (3, -1) + ((F32,) if name.endswith("_sparse") else ()):
        assert "unknown format" in _rejects(native_lib, name, fmt=fmt)
    assert "bad dims" in _rejects(native_lib, name, low_size=0)
    for d in (2, 6, 9):
        assert "multiple of 4" in _rejects(native_lib, name, code=MSI_E_UNSUPPORTED, num=d)
    assert "2^24" in _rejects(native_lib, name, face_size=4096)
    assert "2^31" in _rejects(native_lib, name, low_size=1 << 14, num=8)
    if name.endswith("_sparse"):
        assert "H % 4" in _rejects(native_lib, name, code=MSI_E_UNSUPPORTED, face_size=18)
        assert "W % 16" in _rejects(native_lib, name, code=MSI_E_UNSUPPORTED, face_size=40)


@pytest.mark.parametrize("name", sorted(N_PTRS))
def test_a_valid_empty_batch_returns_ok(native_lib, name):
    ptrs = [_p(k) for k in range(N_PTRS[name])]
    for fmt in (RGBA8, RGBA16F):
        assert _call(native_lib.lib, name, ptrs, fmt=fmt, batch=0) == 0
        assert _call(native_lib.lib, name, ptrs, fmt=fmt, batch=0, pano_height=2, pano_width=2, face_size=4080) == 0
