"""conv1_1 of the fp32 tier on operands whose convolution is EXACT in fp32: the device's raw output must equal the fp64 convolution bit for bit.

tests/test_x3_exact_cpu.py holds the construction (values +-(a + b 2^-9 + c 2^-18) whose bf16 parts are exactly h, m, l; three families whose dropped terms vanish; two
for the fp16 three-product form), asserts on the CPU that every case used here meets the exactness condition (max sum |x| |w| <= 2^6) and that the oracle's emulations
reproduce fp64 bit for bit, and shows that any lost term changes thousands of outputs.  Every product and every partial sum being an fp32 number in any order, the result
does not depend on the tile shape, the K-range hand-off, the fix-up launch or the MFMA's summation order: np.array_equal, no tolerance.

Plans (EXACT_PLANS there; the CPU half pins conv1_1's kernel, whether its tiles are cut, and that its buffer stays raw): conv_halo_x3_kernel<1, 0, 3> in whole tiles,
cut into K-ranges at NUM_CUS 9 and 13 with the in-launch hand-off and with FIXUP_KERNEL = 1, conv_halo8_x3_kernel<0, 3> whole and cut, the fp16 form <1, 0, 2> whole and
cut, wrap padding whole and cut, batch 2 with another sparsity pattern per sample.  CoordNet plans get zero coordinate-channel weights in conv1_1 (the tabulated bias is
exactly 0); the other layers keep init_weights' values and see odd statistics, so only conv1_1 is looked at and the status word is not asserted."""
import numpy as np
import pytest

from tests.test_x3_exact_cpu import EXACT_IDS, EXERCISED, PLAN_BY_ID, conv11, exact_case, form_of, terms
from tests.util import poison_workspace, read_raw_output

pytestmark = pytest.mark.gpu
_BASE = {}      # (shape, coord) -> init_weights: made once, never written


def _weights(case, w11):
    from oracle import nets as onets
    b, h, w, cin, nout, ngf = case["shape"]
    key = (case["shape"], case["coord"])
    if key not in _BASE:
        _BASE[key] = onets.init_weights(cin, nout, ngf=ngf, coord_net=case["coord"], seed=7)
    weights = dict(_BASE[key])
    full = np.zeros_like(weights["conv1_1/weights"])        # [3, 3, Cin (+ 1: the coordinate channel, LAST -- add_sph_coords -- and zero here), Cout]
    full[:, :, :cin, :] = w11
    weights["conv1_1/weights"] = full
    return weights


@pytest.mark.parametrize("pid,family", EXACT_IDS, ids=["%s-%s" % t for t in EXACT_IDS])
def test_conv1_1_equals_the_fp64_convolution_bit_for_bit(pid, family):
    import torch
    from matryodshka_amd import MSI, _native as N, nets
    case, extra, kernel, split, _ = PLAN_BY_ID[pid]
    b, h, w, cin, nout, ngf = case["shape"]
    x, w11, ref = exact_case(family, case["shape"], case["coord"])          # (asserts the exactness condition and fp32 representability)
    m = MSI(weights=_weights(case, w11), coord_net=case["coord"], dtype="f32")
    for k, v in [("NUM_CUS", case["num_cus"])] + list(case["options"].items()) + list((extra or {}).items()):
        m.net_options[getattr(N, "NET_OPT_" + k)] = v
    poison_workspace(m, b, h, w, cin, nout, ngf)
    m.run_net(torch.from_numpy(x).cuda(), nout, ngf)
    torch.cuda.synchronize()
    desc, packed, ws = m._net(b, h, w, cin, nout, ngf)
    plan = m._plan(b, h, w, cin, nout, ngf)
    name, _, nsplit = plan.layer_kernel(0)
    assert name == kernel and (nsplit > 0) == split, (pid, name, nsplit)
    assert N.lib.msi_net_plan_layer_is_normalized(plan.handle, 0) == 0, pid
    info = nets.layer_infos(desc)[0]
    assert info.name.decode() == "conv1_1"
    raw = read_raw_output(ws, packed, info, b, "f32")
    assert raw.shape == ref.shape and np.isfinite(raw).all(), (pid, family, int((~np.isfinite(raw)).sum()))
    bad = raw != ref
    if bad.any():       # which term's loss would explain it: mismatches left against the emulation without that term
        left = {d: int((conv11(x, w11, case["coord"], terms(form_of(family), d)) != raw).sum()) for d in EXERCISED[family]}
        first = tuple(int(i) for i in np.argwhere(bad)[0])
        raise AssertionError("%s %s [%s]: %d of %d outputs differ from the fp64 convolution, first at (b, y, x, c) = %r: %r against %r (largest difference %.3g); "
                             "mismatches left against the emulation without a term: %r"
                             % (pid, family, name, int(bad.sum()), bad.size, first, float(raw[first]), float(ref[first]), float(np.abs(raw - ref).max()), left))
