"""CPU-only checks of the device scorer's plumbing: msi_score_workspace_bytes and msi_score_images are exported and bound with the
signatures the header declares (ABI still 9), every argument error comes back as its documented code with an error text, and the
workspace query is non-zero and monotone.  No kernel is launched: every msi_score_images call below fails its validation, which
is decided before any HIP call (the non-zero dummy pointers are never dereferenced)."""
import ctypes
import re

import pytest

from tests.util import check_binding, declared, header_text, untyped

MSI_E_BADARG, MSI_E_WORKSPACE = -1, -4
F32, U8 = 0, 1
RAW, IMAGE, DEPTH = 0, 1, 2
MSE, MAE, SSIM = 1, 2, 4


def test_both_symbols_are_exported_and_bound_with_the_declared_signature(native_lib):
    assert native_lib.MSI_ABI_VERSION == 9 and native_lib.lib.msi_abi_version() == 9
    for name, restype in (("msi_score_workspace_bytes", ctypes.c_size_t), ("msi_score_images", ctypes.c_int32)):
        assert name in native_lib.SIGNATURES and hasattr(native_lib.lib, name)
        names = check_binding(native_lib, name)
        res, args = native_lib.SIGNATURES[name]
        assert res is restype
        assert args == [untyped(kind) for kind, _ in declared(name)[1]], name
    assert names == ["pred", "target", "dtype", "transform", "quantize", "n_pairs", "group", "height", "width", "channels", "row_weights",
                     "max_val", "metrics", "out", "workspace", "workspace_bytes", "stream"]
    header = header_text()
    for macro, value in (("MSI_SCORE_F32", "0"), ("MSI_SCORE_U8", "1"), ("MSI_SCORE_RAW", "0"), ("MSI_SCORE_IMAGE", "1"), ("MSI_SCORE_DEPTH", "2"),
                         ("MSI_SCORE_MSE", "1u"), ("MSI_SCORE_MAE", "2u"), ("MSI_SCORE_SSIM", "4u")):
        assert re.search(r"#define\s+%s\s+%s\b" % (macro, value), header), macro
    assert (native_lib.MSI_SCORE_F32, native_lib.MSI_SCORE_U8) == (F32, U8)
    assert (native_lib.MSI_SCORE_RAW, native_lib.MSI_SCORE_IMAGE, native_lib.MSI_SCORE_DEPTH) == (RAW, IMAGE, DEPTH)
    assert (native_lib.MSI_SCORE_MSE, native_lib.MSI_SCORE_MAE, native_lib.MSI_SCORE_SSIM) == (MSE, MAE, SSIM)


GOOD = dict(pred=4096, target=8192, dtype=F32, transform=IMAGE, quantize=1, n_pairs=6, group=3, height=16, width=32, channels=3, row_weights=0,
            max_val=255.0, metrics=MSE | MAE | SSIM, out=12288, workspace=16384, workspace_bytes=None)


def _call(lib, **change):
    a = dict(GOOD, **change)
    if a["workspace_bytes"] is None:
        a["workspace_bytes"] = 1 << 30
    return lib.msi_score_images(a["pred"], a["target"], a["dtype"], a["transform"], a["quantize"], a["n_pairs"], a["group"], a["height"],
                                a["width"], a["channels"], a["row_weights"], a["max_val"], a["metrics"], a["out"], a["workspace"],
                                a["workspace_bytes"], None)


BAD = {
    "null pred": dict(pred=0),
    "null target": dict(target=0),
    "null out": dict(out=0),
    "null workspace": dict(workspace=0),
    "n_pairs 0": dict(n_pairs=0, group=1),
    "n_pairs negative": dict(n_pairs=-3, group=1),
    "group 0": dict(group=0),
    "group negative": dict(group=-2),
    "group does not divide n_pairs": dict(group=4),
    "channels 0": dict(channels=0),
    "channels 5": dict(channels=5),
    "quantize with uint8": dict(dtype=U8, transform=RAW, quantize=1),
    "image transform with uint8": dict(dtype=U8, transform=IMAGE, quantize=0),
    "depth transform with uint8": dict(dtype=U8, transform=DEPTH, quantize=0),
    "quantize with raw": dict(transform=RAW, quantize=1),
    "ssim with height 10": dict(height=10),
    "ssim with width 10": dict(width=10),
    "max_val 0": dict(max_val=0.0),
    "max_val negative": dict(max_val=-255.0),
    "empty metrics": dict(metrics=0),
}


@pytest.mark.parametrize("case", sorted(BAD))
def test_bad_arguments_come_back_as_badarg_with_a_text(native_lib, case):
    lib = native_lib.lib
    assert _call(lib, **BAD[case]) == MSI_E_BADARG, case
    assert native_lib.last_error().strip(), case


def test_a_small_workspace_comes_back_as_workspace_error(native_lib):
    lib = native_lib.lib
    need = lib.msi_score_workspace_bytes(GOOD["n_pairs"], GOOD["height"], GOOD["width"], GOOD["channels"])
    assert need > 0
    for size in (0, need - 1):
        assert _call(lib, workspace_bytes=size) == MSI_E_WORKSPACE
        assert native_lib.last_error().strip()
    # an argument error wins over the workspace error (both are decided before any HIP call)
    assert _call(lib, workspace_bytes=0, metrics=0) == MSI_E_BADARG
    # SSIM not requested: images below the window are fine as far as the argument checks go (the too-small workspace stops the call)
    assert _call(lib, height=3, width=10, metrics=MSE, workspace_bytes=0) == MSI_E_WORKSPACE


def test_workspace_bytes_is_nonzero_and_non_decreasing_in_each_argument(native_lib):
    ws = native_lib.lib.msi_score_workspace_bytes
    sizes = [1, 2, 3, 10, 11, 12, 16, 26, 27, 32, 42, 43, 64, 75, 76, 77, 320, 640, 2048, 4096]
    for n in (1, 2, 7, 64):
        for c in (1, 2, 3, 4):
            for h in sizes:
                prev = 0
                for w in sizes:
                    b = ws(n, h, w, c)
                    assert b > 0 and b >= prev, (n, h, w, c)
                    prev = b
    for h in sizes:
        for w in sizes:
            assert all(ws(n + 1, h, w, 3) >= ws(n, h, w, 3) > 0 for n in (1, 2, 7, 64))
            assert all(ws(3, h, w, c + 1) >= ws(3, h, w, c) > 0 for c in (1, 2, 3))
    for w in sizes:
        col = [ws(2, h, w, 3) for h in sizes]
        assert col == sorted(col)
    assert ws(0, 16, 16, 3) == 0 and native_lib.last_error().strip()
    assert ws(1, 16, 16, 5) == 0 and ws(1, 0, 16, 3) == 0
