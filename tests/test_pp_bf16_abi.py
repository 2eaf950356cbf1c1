"""CPU-only checks of the bf16 PP tier's plumbing: the one-launch bf16 perspective sweep volume is exported and bound
(ABI 9), its argument checks reject bad calls before any launch, and the harness takes --dtype.  No kernel is launched
here: every call below fails its validation (or is argparse's) before it could reach a device."""
import pytest

MSI_E_BADARG = -1


def test_sweep_volume_bf16_is_exported_and_bound(native_lib):
    assert "msi_perspective_sweep_volume_bf16" in native_lib.SIGNATURES
    assert hasattr(native_lib.lib, "msi_perspective_sweep_volume_bf16")
    assert native_lib.MSI_ABI_VERSION == 9
    assert native_lib.lib.msi_abi_version() == 9


def _call(lib, ptrs, batch=2, height=16, width=16, num_depths=8):
    ref, src, p0, p1, intr, depths, psv = ptrs
    return lib.msi_perspective_sweep_volume_bf16(ref, src, p0, p1, intr, depths, batch, height, width, num_depths, psv, None)


@pytest.mark.parametrize("null", range(7))
def test_sweep_volume_bf16_rejects_null_pointers(native_lib, null):
    # (non-zero dummies are never dereferenced: validation fails first)
    ptrs = [4096 * (k + 1) for k in range(7)]
    ptrs[null] = None
    assert _call(native_lib.lib, ptrs) == MSI_E_BADARG
    assert "null pointer" in native_lib.last_error()


@pytest.mark.parametrize("dims", [dict(height=1), dict(height=0), dict(num_depths=0), dict(num_depths=-3), dict(width=1),
                                  dict(batch=-1)])
def test_sweep_volume_bf16_rejects_bad_dims(native_lib, dims):
    ptrs = [4096 * (k + 1) for k in range(7)]
    assert _call(native_lib.lib, ptrs, **dims) == MSI_E_BADARG
    msg = native_lib.last_error()
    assert msg and "perspective_sweep_volume_bf16" in msg


def test_sweep_volume_bf16_rejects_32bit_overflow(native_lib):
    ptrs = [4096 * (k + 1) for k in range(7)]
    assert _call(native_lib.lib, ptrs, height=16, width=1 << 26, num_depths=64) == MSI_E_BADARG
    assert "too large" in native_lib.last_error()


def test_harness_dtype_flag(native_lib, capsys):
    from matryodshka_amd import harness
    with pytest.raises(SystemExit) as e:
        harness.main(["--dtype", "fp16"])
    assert e.value.code == 2
    assert "--dtype" in capsys.readouterr().err
    # bf16 parses: the next check of main() (before any model exists) is what stops this call
    with pytest.raises(SystemExit) as e:
        harness.main(["--dtype", "bf16", "--input_type", "PP", "--num_msi_planes", "4", "--num_psv_planes", "8"])
    assert "--num_psv_planes must equal --num_msi_planes" in str(e.value.code)
