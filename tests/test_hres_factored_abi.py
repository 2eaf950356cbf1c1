"""CPU-only checks of the factored viewer's plumbing: msi_render_views_factored is exported, bound and declared with one signature (ABI
still 9), defined in exactly one unit -- a geometry unit, built without contraction --, takes msi_hres_layers' inputs in its order, and its
argument checks reject bad calls with the documented code and text before any HIP call.  No kernel is launched here: every native call
below fails its validation, or has an empty batch, before it could reach a device (the dummy pointers are never dereferenced)."""
import os
import re

import pytest

from tests.util import check_binding, header_text

MSI_E_BADARG, MSI_E_UNSUPPORTED = -1, -3
EQUIRECT, PINHOLE = 0, 1
NAME = "msi_render_views_factored"
HRES_INPUTS = ["ref_image", "src_image", "ref_curr_pose", "src_curr_pose", "intrinsics", "depths", "trig", "blend_weights", "alphas",
               "batch", "low_height", "low_width", "height", "width", "num_planes"]
VIEW_ARGS = ["tgt_pose_rt", "tgt_pos", "view_intrinsics", "eye_radius", "view_trig", "views", "camera", "out_height", "out_width",
             "out_rgb", "out_depth", "status_device", "stream"]


def test_exported_and_bound(native_lib):
    assert NAME in native_lib.SIGNATURES
    assert hasattr(native_lib.lib, NAME)
    assert native_lib.MSI_ABI_VERSION == 9
    assert native_lib.lib.msi_abi_version() == 9


def test_header_and_binding_agree_on_the_signature(native_lib):
    assert "#define MSI_ABI_VERSION 9" in header_text()
    assert check_binding(native_lib, NAME, int32_and_pointers=True) == HRES_INPUTS + VIEW_ARGS
    assert NAME in header_text(comments=True).split("#define MSI_ABI_VERSION 9")[0].split("additions since, no bump")[1]


def test_it_takes_the_inputs_of_msi_hres_layers_in_its_order(native_lib):
    n = len(HRES_INPUTS)
    assert check_binding(native_lib, NAME)[:n] == check_binding(native_lib, "msi_hres_layers")[:n] == HRES_INPUTS
    assert native_lib.SIGNATURES[NAME][1][:n] == native_lib.SIGNATURES["msi_hres_layers"][1][:n]


def _texts():
    from matryodshka_amd import build
    return {u: open(os.path.join(build.CSRC, u)).read() for u in os.listdir(build.CSRC) if u.endswith((".hip", ".h", ".cpp", ".inc"))}


def test_defined_once_in_a_geometry_unit():
    from matryodshka_amd import build
    pattern = re.compile(r"^int\s+%s\(" % NAME, re.M)
    hits = {u: len(pattern.findall(t)) for u, t in _texts().items() if pattern.search(t)}
    assert hits == {"geo_factored.hip": 1}
    assert "geo_factored.hip" in build.GEO_UNITS
    flags = dict(build.SOURCES)["geo_factored.hip"]
    assert "-ffp-contract=off" in flags and "-fno-slp-vectorize" in flags
    assert '#include "geometry_device.h"' in _texts()["geo_factored.hip"]


def test_the_texel_the_source_and_the_tap_coordinates_are_each_defined_once():
    """The factored stack calls the builders' texel and the renders' tap arithmetic; it restates neither."""
    texts = _texts()
    for pattern in (r"float4 hres_texel\(", r"struct OdsHres \{", r"TapsXY make_taps_xy\(", r"struct FactoredSphereStack \{",
                    r"HresCorners hres_corners\(", r"\bT lerp2\("):
        assert {u: len(re.findall(pattern, t)) for u, t in texts.items() if re.search(pattern, t)} == {"geometry_device.h": 1}, pattern
    # the clamp / wrap arithmetic (x0 + width, y0 + height as unsigned) is written in make_taps_xy alone
    assert sum(len(re.findall(r"\(unsigned\)\(x0 \+ width\)", t)) for t in texts.values()) == 1
    header = texts["geometry_device.h"]
    stack = header[header.index("struct FactoredSphereStack {"):]
    stack = stack[:stack.index("\n};\n")]
    for call in ("sphere_uv(", "make_taps_xy(", "hres_corners(", "lerp2(", "ods_hres(", "hres_texel(", "blend4(", "ballot_w64("):
        assert call in stack, call
    for restated in ("ods_quad(", "gather3", "floorf(", "make_taps_ranged("):
        assert restated not in stack, restated
    ranged = header[header.index("TapsR make_taps_ranged("):]
    assert "make_taps_xy(" in ranged[:ranged.index("\n}\n")]
    kernel = texts["geo_factored.hip"]
    assert "sphere_views_body<MODE, CAMERA>(" in kernel and "FactoredSphereStack{" in kernel


# ------------------------------------------------------------------------------------------------ the argument checks
def _p(k):
    return 4096 * (k + 1)


N_STACK_PTRS, N_PTRS = 9, 17       # then: pose, pos, view_intrinsics, eye_radius, view_trig, out_rgb, out_depth, status


def _call(lib, ptrs, batch=2, low_height=8, low_width=16, height=16, width=32, num_planes=4, views=2, camera=EQUIRECT, out_height=8,
          out_width=70):
    return lib.msi_render_views_factored(*(list(ptrs[:9]) + [batch, low_height, low_width, height, width, num_planes] + list(ptrs[9:14]) +
                                           [views, camera, out_height, out_width] + list(ptrs[14:17]) + [None]))


def _ptrs(camera=EQUIRECT, null=()):
    ptrs = [_p(k) for k in range(N_PTRS)]
    ptrs[12] = None                                   # eye_radius: the ODS camera, off
    if camera == PINHOLE:
        ptrs[13] = None
    else:
        ptrs[11] = None
    for k in null:
        ptrs[k] = None
    return ptrs


def _rejects(native_lib, code=MSI_E_BADARG, null=(), ptrs=None, **kw):
    ptrs = _ptrs(kw.get("camera", EQUIRECT), null) if ptrs is None else ptrs
    assert _call(native_lib.lib, ptrs, **kw) == code
    msg = native_lib.last_error()
    assert "render_views_factored" in msg
    return msg


def test_it_rejects_bad_calls(native_lib):
    for null in list(range(N_STACK_PTRS)) + [9, 10]:
        assert "null pointer" in _rejects(native_lib, null=(null,))
    assert "equirect camera needs trig" in _rejects(native_lib, null=(13,))
    assert "pinhole camera needs intrinsics" in _rejects(native_lib, camera=PINHOLE, null=(11,))
    ods_pinhole = _ptrs(PINHOLE)
    ods_pinhole[12] = _p(12)
    assert "eye_radius" in _rejects(native_lib, ptrs=ods_pinhole, camera=PINHOLE)
    for dims in (dict(height=0), dict(width=0), dict(num_planes=0), dict(batch=-1), dict(low_height=0), dict(low_width=-1)):
        assert "bad dims" in _rejects(native_lib, **dims)
    for d in (2, 6):
        assert "multiple of 4" in _rejects(native_lib, code=MSI_E_UNSUPPORTED, num_planes=d)
    assert "2^24" in _rejects(native_lib, height=4096, width=4096)
    assert "2^31" in _rejects(native_lib, low_height=1 << 14, low_width=1 << 14, num_planes=8)
    for camera in (2, -1):
        assert "unknown camera" in _rejects(native_lib, ptrs=_ptrs(), camera=camera)
    assert "both outputs are NULL" in _rejects(native_lib, null=(14, 15))
    assert "views must be >= 1" in _rejects(native_lib, views=0)
    assert "bad output size" in _rejects(native_lib, out_height=0)
    assert "bad output size" in _rejects(native_lib, camera=PINHOLE, out_width=1)


def test_the_checks_come_in_the_documented_order(native_lib):
    """msi_hres_layers' checks, then the views': a call that is wrong in several ways reports the first."""
    assert "null pointer" in _rejects(native_lib, null=(0, 14, 15), height=0, num_planes=6, camera=7)
    assert "bad dims" in _rejects(native_lib, null=(14, 15), height=0, num_planes=6, camera=7)
    assert "multiple of 4" in _rejects(native_lib, code=MSI_E_UNSUPPORTED, null=(14, 15), num_planes=6, ptrs=None, views=0)
    assert "2^24" in _rejects(native_lib, null=(14, 15), height=4096, width=4096, views=0)
    assert "both outputs are NULL" in _rejects(native_lib, null=(9, 14, 15), views=0)
    assert "null pointer" in _rejects(native_lib, null=(9,), views=0)
    assert "unknown camera" in _rejects(native_lib, ptrs=_ptrs(), camera=5, views=0)
    assert "views must be >= 1" in _rejects(native_lib, views=0, out_height=0)
    assert "views must be >= 1" in _rejects(native_lib, views=0, batch=0)              # (an empty batch is still validated)


@pytest.mark.parametrize("camera", [EQUIRECT, PINHOLE])
def test_a_valid_empty_batch_passes_validation(native_lib, camera):
    assert _call(native_lib.lib, _ptrs(camera), batch=0, camera=camera) == 0
    assert _call(native_lib.lib, _ptrs(camera, null=(14,)), batch=0, camera=camera, height=4096, width=4095) == 0
    ods = _ptrs(EQUIRECT)
    ods[12] = _p(12)
    assert _call(native_lib.lib, ods, batch=0) == 0


# ------------------------------------------------------------------------------------------------ what the compiler made of the layer step
def test_the_four_taps_share_their_row_and_column_work_in_the_built_kernels(native_lib):
    """The four taps of a layer step call ods_hres and hres_corners four times; that their rows and columns share the trig lookups is left to
    the compiler's common-subexpression elimination (profiles/hres_factored_isa.txt has the counts).  Held here on the library as built: per
    kernel (one layer step, not unrolled) the colour forms have the 32 image-texel loads, at most 42 other vector loads (16 alpha + 16
    blend-weight + 8 trig + the view's own) and no scratch; the depth-only forms load no image texel at all."""
    import subprocess
    import tempfile
    from matryodshka_amd import isa_lint
    objdump = isa_lint.OBJDUMP or isa_lint._find_objdump()
    kernels = {}
    for _, blob in isa_lint.code_objects(native_lib.LIB_PATH):
        with tempfile.NamedTemporaryFile(suffix=".hsaco") as f:
            f.write(blob)
            f.flush()
            txt = subprocess.run([objdump, "-d", "--no-show-raw-insn", f.name], check=True, stdout=subprocess.PIPE).stdout.decode()
        cur = None
        for line in txt.splitlines():
            m = re.match(r"^[0-9a-f]+ <(.+)>:", line)
            if m:
                cur = m.group(1) if "render_views_factored_kernel" in m.group(1) else None
                continue
            if cur:
                kernels.setdefault(cur, []).append(line.split("//")[0].strip())
    assert len(kernels) == 9
    for name, ins in kernels.items():
        mode = int(re.search(r"render_views_factored_kernelILi(\d)E", name).group(1))
        count = lambda prefix: sum(1 for i in ins if i.startswith(prefix))
        assert count("scratch_") == 0, name
        if mode == 2:                                  # RENDER_DEPTH alone
            assert count("buffer_load") == 0 and count("global_load") <= 18, (name, count("global_load"))
        else:
            assert count("buffer_load") == 32 and count("global_load") <= 42, (name, count("buffer_load"), count("global_load"))
