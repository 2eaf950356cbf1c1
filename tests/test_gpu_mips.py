"""msi_build_mips (MSI.build_mips) against the rule in numpy (matryodshka_amd/mips.py: build_mips_np), bit for bit, in all three
texel formats: shapes with one and with several workgroups per layer, a border workgroup that holds whole tiles only (24 x 40),
every level count's reduction depth up to the 32 x 32 tile of L = 6, L = 1 (nothing written), random stacks and stacks with
zero-alpha regions (where a texel takes the plain mean of its colours).

32 x 64 with L = 6 would have a 1 x 2 top level, which the size rule (a top level of at least 2 x 2) refuses, so the 32 x 32 tile is
reached at 64 x 128, the smallest size the rule admits for L = 6, and 32 x 64 runs at L = 5, the most it admits (the refusal itself is
held in tests/test_mip_abi.py and tests/test_mip_cpu.py)."""
import numpy as np
import pytest

from matryodshka_amd.mips import build_mips_np
from tests.util import random_rgba

pytestmark = pytest.mark.gpu

F = np.float32
FORMATS = ['f32', 'rgba8', 'rgba16f']
B, D = 2, 5


@pytest.fixture(scope="module")
def gpu():
    import torch
    assert torch.cuda.is_available(), "GPU tests need a HIP device"
    from matryodshka_amd import MSI
    return torch, MSI()


def _stack(seed, h, w, holes):
    """[B,H,W,D,4] fp32; with `holes`, zero-alpha regions of several sizes and alignments: whole 2 x 2 blocks, whole tiles, a
    region that cuts through blocks, one layer all transparent -- and layer 0 transparent in places too (it never weighs)."""
    rgba = random_rgba(seed, B, h, w, D)
    if holes:
        rgba[:, 0:2, 0:2, :, 3] = 0
        rgba[:, h // 2:, : w // 4, 1:3, 3] = 0
        rgba[:, 3:h - 3, 5:w - 7, 3, 3] = 0
        rgba[0, :, :, 4, 3] = 0
        rgba[1, 1::2, :, 0, 3] = 0
    return rgba


def _bits(a):
    return a.view({2: np.uint16, 4: np.uint32, 1: np.uint8}[a.dtype.itemsize])


@pytest.mark.parametrize("holes", [False, True])
@pytest.mark.parametrize("fmt", FORMATS)
@pytest.mark.parametrize("h,w,levels", [(16, 32, 3), (24, 40, 3), (32, 64, 5), (64, 128, 6), (16, 32, 1), (16, 32, 2), (16, 32, 4)])
def test_build_mips_is_the_numpy_rule_bit_for_bit(gpu, h, w, levels, fmt, holes):
    torch, m = gpu
    rgba = torch.from_numpy(_stack(41 + h + levels, h, w, holes)).cuda()
    planes = m.inv_depths(1.0, 100.0, D)
    layers = rgba if fmt == 'f32' else m.pack_layers(rgba, fmt)
    mip = m.build_mips(layers, levels, planes)
    assert mip.levels == levels and mip.format == fmt and mip.shape == (B, h, w, D) and mip.planes == tuple(planes)
    base = mip.data.cpu().numpy()
    assert base.shape == (B, D, h, w, 4)
    want = build_mips_np(base, fmt, levels)
    got = mip.mips.cpu().numpy()
    if levels == 1:
        assert got.size == 0 and want == []
        return
    flat = np.concatenate([x.reshape(-1) for x in want])
    assert got.dtype == flat.dtype and got.shape == flat.shape
    assert np.array_equal(_bits(got), _bits(flat)), "first difference at element %d" % int(np.flatnonzero(_bits(got) != _bits(flat))[0])
    for l in range(1, levels):
        lv = mip.level(l)
        data = (lv if fmt == 'f32' else lv.data).cpu().numpy()
        assert np.array_equal(_bits(data), _bits(want[l - 1]))
    # the base is untouched
    ref = rgba.permute(0, 3, 1, 2, 4).contiguous() if fmt == 'f32' else layers.data
    assert torch.equal(mip.data, ref)


def test_levels_none_takes_the_most_the_sizes_allow(gpu):
    torch, m = gpu
    for (h, w), want in (((16, 32), 4), ((24, 40), 4), ((64, 128), 6), ((30, 70), 2), ((15, 33), 1)):
        rgba = torch.from_numpy(random_rgba(3, 1, h, w, 2)).cuda()
        assert m.build_mips(rgba).levels == want
    with pytest.raises(ValueError):
        m.build_mips(torch.from_numpy(random_rgba(3, 1, 32, 64, 2)).cuda(), levels=6)
    with pytest.raises(ValueError):
        m.build_mips(torch.from_numpy(random_rgba(3, 1, 30, 64, 2)).cuda(), levels=3)
