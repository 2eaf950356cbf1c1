"""Every layer of the fp32 network tier against an fp64 reference fed THE DEVICE'S OWN tensors (teacher forcing), plan by plan.

An fp32 plan leaves every layer's output in its workspace -- raw, or LayerNorm + ReLU applied in place (msi_net_plan_layer_is_normalized) -- so an fp64 forward can
recompute layer L from what the device itself produced for L's sources (oracle/nets.py forward(precision="fp64", forced_raw=..., forced_act=...);
tests.util.forced_layer_errors_f32).  What then separates the two is the layer's own arithmetic, and each layer and the head is held to the gates of the arithmetic
its kernel runs (read off the kernel's name): six bf16 products, three fp16 products, or native fp32.  A kernel that lost one of the three small products, or reads an
l plane from the wrong row, slot or stage, is 1.5e-6 .. 5e-6 of the layer's rms off: above these gates, far below every free-running gate of the suite (2e-4, 6e-4,
1e-5), as tests/test_f32_forced_cpu.py shows on the CPU.

Cases: tests/test_f32_forced_cpu.py FORCED_CASES (cases of tests/test_plan_decomposition.py and plans that reach the remaining instantiations) -- between them every
fp32 conv instantiation a plan can take.  Each case: seeded weights with a random affine, uniform input, a workspace poisoned with NaN bytes before the first forward,
network_status() == 0, every stored tensor finite, the kernels the host-side plan promises.

The gates (tests.util.F32_FORCED_GATES) are 3 x the worst value of the oracle's own emulation of each arithmetic on the CPU (tools/f32_forced_gates.py,
profiles/f32_forced_gates.txt), measured before any device run and never moved by one; relative to the fp64 tensor's max-abs (max) and rms (rms):

  arithmetic   layer max   layer rms   head max   head rms
  x3           1.40e-6     5.23e-7     9.36e-7    2.04e-7
  f16          3.12e-6     1.25e-6     1.98e-6    3.63e-7
  native       3.41e-6     1.26e-6     1.83e-6    3.03e-7

What the device gave is recorded next to these in the profile, as an observation.

On an MI355X (profiles/f32_forced_gates.txt): worst six-product layer 1.03e-6 max, 4.49e-7 rms (conv8_1 on the 8-row conv-transpose tile, the one split kernel that
adds all six products into a single accumulator: cnn_x3.hip split_mfma<6>; with the small products in a second accumulator, split_mfma<3>, layers of K = 1152 .. 4608
measure 2.1e-7 .. 3.3e-7); fp16 form 9.0e-7 / 3.9e-7; native 2.48e-6 / 7.6e-7; the head <= 6.3e-7 max, 9.7e-8 rms."""
import numpy as np
import pytest

from tests.test_f32_forced_cpu import FORCED_BY_ID, FORCED_CASES
from tests.test_gpu_decomposition import _forward
from tests.test_plan_decomposition import plan_for
from tests.util import F32_FORCED_GATES, f32_arithmetic, forced_layer_errors_f32

pytestmark = pytest.mark.gpu


@pytest.mark.parametrize("cid", [c["id"] for c in FORCED_CASES])
def test_every_layer_matches_the_fp64_reference_fed_the_devices_own_tensors(cid):
    from matryodshka_amd import _native as N
    from tests.test_gpu_decomposition import _model, _oracle
    case = FORCED_BY_ID[cid]
    pred, stored, _, plan = _forward(case)                   # (poisoned workspace; asserts network_status() == 0)
    kernels = plan.kernels()
    assert kernels == plan_for(case).kernels(), cid
    for name, t in stored.items():
        assert np.isfinite(t).all(), "%s %s: %d non-finite stored values" % (cid, name, int((~np.isfinite(t)).sum()))
    assert len(stored) == 17 and np.isfinite(pred).all(), cid
    normalized = [name for li, name in enumerate(stored) if N.lib.msi_net_plan_layer_is_normalized(plan.handle, li) != 0]
    weights, x, _, _ = _oracle(case)
    rep = forced_layer_errors_f32(weights, x, case["coord"], stored, normalized, pred, gates=F32_FORCED_GATES, kernels=kernels)
    _model(case)._ws_cache.clear()
    wmax = max(rep["layers"].items(), key=lambda kv: kv[1][0])
    wrms = max(rep["layers"].items(), key=lambda kv: kv[1][1])
    names = list(stored)
    print("f32 forced %s: worst layer max %.2e (%s, %s), rms %.2e (%s, %s); head max %.2e, rms %.2e; %d layers normalized in place; arithmetics %s"
          % (cid, wmax[1][0], wmax[0], f32_arithmetic(kernels[names.index(wmax[0])][0]), wrms[1][1], wrms[0], f32_arithmetic(kernels[names.index(wrms[0])][0]),
             rep["head"][0], rep["head"][1], len(normalized), "/".join(sorted({f32_arithmetic(k[0]) for k in kernels[:17]}))))
    assert not rep["failures"], "%s:\n%s" % (cid, "\n".join(rep["failures"]))
