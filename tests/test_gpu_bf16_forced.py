"""Every layer of the bf16 network tier against the oracle ON THE DEVICE'S OWN INPUTS (teacher forcing), plan by plan.

A bf16 plan keeps every layer's raw output in its workspace (fp16 of x 2^-e; tests.util.read_raw_output), so the oracle can recompute layer L from what the
device itself produced for L's sources (oracle/nets.py forward(forced_raw=...); tests.util.forced_layer_errors).  What then separates the two is the layer's own
freedom -- fp32 summation order, the fp16 store, isolated operand flips from the last bits of the LayerNorm affine -- which does not grow with depth, where the
free-running comparisons of tests/test_gpu_bf16.py need gates of up to 1.7e-2 of the layer scale (max) and 2e-3 (mean) at the deep layers and let a rounding bug
confined to one of them pass (tests/test_bf16_forced_cpu.py shows both).

Cases: tests/test_bf16_forced_cpu.py FORCED_CASES -- between them every bf16 kernel instantiation the launchers have; each asserts the kernels its plan took.
Each case: seeded weights with a random affine, bf16-rounded uniform input, a workspace poisoned with NaN bytes before the first forward,
network_status() == 0, every raw tensor finite, then on all 17 layers and the head the gates of tests.util.BF16_FORCED_GATES for the case's width.

The gates are 3 x the worst value of a CPU stand-in that has exactly a correct kernel's freedoms (tools/bf16_forced_gates.py; the run is
profiles/bf16_forced_gates.txt), measured before any device run and never moved by one.  Worst legitimate value -> gate, relative to the layer scale (head: absolute):

  ngf   layer max            layer mean           layer |bias|         head max             head mean
  16    1.46e-3 -> 4.39e-3   1.16e-4 -> 3.47e-4   6.59e-6 -> 1.98e-5   5.89e-3 -> 1.77e-2   9.97e-6 -> 2.99e-5
  32    6.79e-4 -> 2.04e-3   7.12e-5 -> 2.14e-4   4.01e-6 -> 1.20e-5   3.34e-3 -> 1.00e-2   4.11e-6 -> 1.23e-5
  >=64  5.96e-4 -> 1.79e-3   4.37e-5 -> 1.31e-4   8.27e-7 -> 2.48e-6   3.95e-3 -> 1.19e-2   3.11e-6 -> 9.32e-6

(max: the fp16 store's 2^-11 plus a flipped bf16 operand or two, which weigh ~ 1 / sqrt(K) -- hence by width; mean: the fp16 store; bias: how far the stored
values lean towards zero, which a round-to-nearest store does not and a truncating one does by its whole mean error -- the one fault the other two gates miss.)
What the device gave is recorded next to these in the profile, as an observation."""
import numpy as np
import pytest

from tests.test_bf16_forced_cpu import FORCED_BY_ID, FORCED_CASES, kernels_of
from tests.util import forced_gates, forced_layer_errors, poison_workspace, read_raw_output

pytestmark = pytest.mark.gpu
SEED = 23
_INPUTS = {}     # (shape, coord) -> (weights, x): made once, never written


def _inputs(case):
    from oracle import nets as onets
    key = (case["shape"], case["coord"])
    if key not in _INPUTS:
        b, h, w, cin, nout, ngf = case["shape"]
        weights = onets.init_weights(cin, nout, ngf=ngf, coord_net=case["coord"], seed=SEED, randomize_affine=True)
        x = onets.bf16_round(np.random.RandomState(SEED + 1).uniform(-1, 1, size=(b, h, w, cin)).astype(np.float32))
        x.setflags(write=False)
        _INPUTS[key] = (weights, x)
    return _INPUTS[key]


def _forward(case, extra=None):
    """One forward of `case` (+ `extra` options) on a poisoned workspace: (prediction, {layer: raw output}, the plan's kernels)."""
    import torch
    from matryodshka_amd import MSI, _native as N, nets
    weights, x = _inputs(case)
    b, h, w, cin, nout, ngf = case["shape"]
    m = MSI(weights=weights, coord_net=case["coord"], dtype="bf16")
    for k, v in [("NUM_CUS", case["num_cus"])] + list(case["options"].items()) + list((extra or {}).items()):
        m.net_options[getattr(N, "NET_OPT_" + k)] = v
    poison_workspace(m, b, h, w, cin, nout, ngf)
    pred = m.run_net(torch.from_numpy(x.copy()).cuda().bfloat16(), nout, ngf)
    torch.cuda.synchronize()
    assert m.network_status() == 0, case["id"]
    desc, packed, ws = m._net(b, h, w, cin, nout, ngf)
    kernels = m._plan(b, h, w, cin, nout, ngf).kernels()
    raws = {}
    for info in nets.layer_infos(desc):
        if info.kind != nets.KIND_HEAD:
            raws[info.name.decode()] = read_raw_output(ws, packed, info, b, "bf16")
    pred = pred.cpu().numpy()
    for name, raw in raws.items():
        assert np.isfinite(raw).all(), "%s %s: %d non-finite raw outputs" % (case["id"], name, int((~np.isfinite(raw)).sum()))
    assert len(raws) == 17 and np.isfinite(pred).all(), case["id"]
    return pred, raws, kernels


@pytest.mark.parametrize("cid", [c["id"] for c in FORCED_CASES])
def test_every_layer_matches_the_oracle_fed_the_devices_own_raw_outputs(cid):
    case = FORCED_BY_ID[cid]
    weights, x = _inputs(case)
    pred, raws, kernels = _forward(case)
    assert [k[0] for k in kernels] == kernels_of(cid), cid
    rep = forced_layer_errors(weights, x, case["coord"], raws, pred, gates=forced_gates(case["shape"][5]), kernels=kernels)
    wmax = max(rep["layers"].items(), key=lambda kv: kv[1][0])
    wmean = max(rep["layers"].items(), key=lambda kv: kv[1][1])
    wbias = max(rep["bias"].items(), key=lambda kv: abs(kv[1]))
    print("forced %s: worst layer max %.2e (%s), mean %.2e (%s), |bias| %.2e (%s); head max %.2e, mean %.2e"
          % (cid, wmax[1][0], wmax[0], wmean[1][1], wmean[0], abs(wbias[1]), wbias[0], rep["head"][0], rep["head"][1]))
    assert not rep["failures"], "%s:\n%s" % (cid, "\n".join(rep["failures"]))
    if cid == "A-tap-cus24":        # the separate fix-up launch sums the same K-ranges in the same order: bit for bit, layers and prediction
        pred_f, raws_f, kernels_f = _forward(case, {"FIXUP_KERNEL": 1})
        assert [k[1:] for k in kernels_f] == [k[1:] for k in kernels]
        assert np.array_equal(pred_f, pred)
        for name, raw in raws.items():
            assert np.array_equal(raws_f[name], raw), name
