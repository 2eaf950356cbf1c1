"""The conv kernels' K-range splits EXECUTED at small shapes across CU counts (plan option NUM_CUS): the cases of
tests/test_plan_decomposition.py (which holds, host-side, the table of kernel families x decomposition classes they reach),
each on a workspace poisoned with NaN bytes (tests.util.poison_workspace):

  1. every layer's full raw tensor is finite and within the existing gate of its arithmetic against the CPU oracle, relative
     to the layer's scale -- 2e-4 for fp32 and the six-product form, 6e-4 for the fp16 three-product form, the per-layer gates
     of test_gpu_bf16.py for bf16 -- the prediction within 1e-3 (bf16: 6e-2), and network_status() == 0; a bf16 plan's layers are ALSO held, all 17 and
     the head, to the gates of the teacher-forced oracle (tests.util.forced_layer_errors: each layer recomputed from this run's own raw outputs of its
     sources; <= 1.8e-3 of the scale and 1.3e-4 in the mean at this width, the same at conv8_2 as at conv1_1);
  2. against the same plan with TAILSPLIT = 0 at the same NUM_CUS (whole tiles only): another summation order only, layers
     within 2e-5 of their scale and the prediction within 2e-5 (fp32).  Between two FREE-RUNNING bf16 plans that bound cannot
     be met (against the forced oracle of check 1 a tight bound is met: there each layer starts from the same inputs on both
     sides): raw outputs are stored as fp16 (one flipped rounding = up to 2^-10 of the value, 5e-4 .. 1e-3 of the
     scale) and activations are rounded to bf16, and a flipped activation (2^-8 of an operand) moves every output that reads
     it, which flips further roundings in the next layer: the difference grows with depth the way the error against the
     oracle does, which is why the bf16 oracle gates grow from 5e-4 to 1.7e-2.  So for bf16: conv1_1 (identical operands: the
     summation order plus isolated fp16 flips, whose mean is the summation-order difference itself) within 5e-4 everywhere
     and 2e-5 in the mean; every other layer within BOTH bf16 oracle gates of test_gpu_bf16.py, the largest and the mean
     difference (two runs of the same kernels and the same LayerNorm arithmetic must be at least as close to each other as
     either is to the CPU emulation; the mean gate is 5 - 10 times tighter than the max gate and sees a wrong tile, whose
     4096 elements are 3 % of the smallest layer here); the prediction within 4e-2 and 3e-3 in the mean;
  3. FIXUP_KERNEL = 1 (separate fix-up launch) reproduces the in-launch hand-off bit for bit, layers and prediction;
  4. three repeats are bit-identical;
  5. the plan that ran has the kernels and classes the host-side table promises.

NUM_CUS only steers the host-side decomposition (how many workgroups, which tiles are cut, how large the slab and ticket
regions are); no kernel assumes that its workgroups are co-resident.  The split-K hand-off never waits: a workgroup stores
its slab, takes a ticket with one atomic add and returns unless it is the last arriver, which sums the slabs (cnn_x3.hip /
cnn_halo.hip / cnn_igemm.hip: `if (*s_old != nsp - 1) return;`).  No kernel of the library has a spin loop.  So CU counts below and above the device's
(up to 320 here; a 304-CU part's decomposition is one of the cases) cannot hang, and slabs / tickets are sized from the
same NUM_CUS the decomposition uses.

The CPU oracle runs once per (dtype, shape, seed) and is shared, read-only, by every CU count and option of that shape."""
import numpy as np
import pytest

from tests.test_gpu_bf16 import _BF16_LAYER_GATES
from tests.util import forced_gates, forced_layer_errors, poison_workspace, read_raw_output
from tests.test_plan_decomposition import (BACK_TO_BACK_CASES, CASE_BY_ID, COVERAGE, DECOMP_CASES, OPTION_CASES, changed_layers,
                                           pairs_of, plan_for)

pytestmark = pytest.mark.gpu
SEED = 11
_ORACLE = {}     # (dtype, shape, coord) -> (weights, x, ref, acts): computed once, never written
_MODELS = {}     # (dtype, shape, coord) -> MSI


def _oracle(case):
    from oracle import nets as onets
    key = (case["dtype"], case["shape"], case["coord"])
    if key not in _ORACLE:
        b, h, w, cin, nout, ngf = case["shape"]
        bf16 = case["dtype"] == "bf16"
        weights = onets.init_weights(cin, nout, ngf=ngf, coord_net=case["coord"], seed=SEED, randomize_affine=True)
        x = np.random.RandomState(SEED + 1).uniform(-1, 1, size=(b, h, w, cin)).astype(np.float32)
        if bf16:
            x = onets.bf16_round(x)
        ref, acts = onets.forward(weights, x, coord_net=case["coord"], return_activations=True, bf16=bf16)
        for a in [x, ref] + list(acts.values()):
            a.setflags(write=False)
        _ORACLE[key] = (weights, x, ref, acts)
    return _ORACLE[key]


def _model(case):
    from matryodshka_amd import MSI
    key = (case["dtype"], case["shape"], case["coord"])
    if key not in _MODELS:
        _MODELS[key] = MSI(weights=_oracle(case)[0], coord_net=case["coord"], dtype=case["dtype"])
    return _MODELS[key]


def _set_options(m, case, extra=None):
    from matryodshka_amd import _native as N
    named = [("NUM_CUS", case["num_cus"])] + list(case["options"].items()) + list((extra or {}).items())
    m.net_options = {}
    for k, v in named:                           # (a later entry replaces an earlier one: TAILSPLIT = 0 of check 2)
        m.net_options[getattr(N, "NET_OPT_" + k)] = v


def _forward(case, extra=None, x=None, repeats=0):
    """One forward of `case` (+ `extra` options) on a poisoned workspace: (prediction, {layer: raw fp32 tensor}, expected
    {layer: oracle tensor for what the plan leaves in that buffer}, plan)."""
    import torch
    from matryodshka_amd import _native as N, nets
    weights, x0, ref, acts = _oracle(case)
    b, h, w, cin, nout, ngf = case["shape"]
    m = _model(case)
    _set_options(m, case, extra)
    ws = poison_workspace(m, b, h, w, cin, nout, ngf)
    xt = torch.from_numpy(x0 if x is None else x).cuda()
    if case["dtype"] == "bf16":
        xt = xt.bfloat16()
    pred = m.run_net(xt, nout, ngf)
    torch.cuda.synchronize()
    assert m.network_status() == 0
    for _ in range(repeats):
        assert torch.equal(m.run_net(xt, nout, ngf), pred), (case["id"], extra, "not deterministic")
    desc, packed, ws = m._net(b, h, w, cin, nout, ngf)
    plan = m._plan(b, h, w, cin, nout, ngf)
    raws, want = {}, {}
    for li, info in enumerate(nets.layer_infos(desc)):
        if info.kind == nets.KIND_HEAD:
            continue
        name = info.name.decode()
        raws[name] = read_raw_output(ws, packed, info, b, case["dtype"])
        # fp32 plans normalise a layer in place unless every consumer applies its LayerNorm while loading; bf16 plans keep the raw buffer
        raw_kept = case["dtype"] == "bf16" or N.lib.msi_net_plan_layer_is_normalized(plan.handle, li) == 0
        want[name] = acts[name + "/raw"] if raw_kept else acts[name]
    return pred.cpu().numpy(), raws, want, plan


def _check_case(case, extra=None):
    _, _, ref, _ = _oracle(case)
    bf16 = case["dtype"] == "bf16"
    pred, raws, want, plan = _forward(case, extra, repeats=3)                            # 4. determinism
    # 5. the kernels that ran
    host = plan_for(case, extra)
    assert plan.kernels() == host.kernels(), case["id"]
    if extra is None:
        assert pairs_of(case, plan) == sorted(p for p, ids in COVERAGE.items() if case["id"] in ids), case["id"]
    # 1. against the oracle
    kernels = plan.kernels()
    worst = ("", 0.0)
    assert len(raws) == 17
    for li, (name, raw) in enumerate(raws.items()):
        # the gate of the layer's own arithmetic: the two-plane fp16 form (last template argument 2) 6e-4, everything else fp32 2e-4
        gate = 6e-4 if "_x3_kernel<" in kernels[li][0] and kernels[li][0].endswith("2>") else 2e-4
        o = want[name]
        assert raw.shape == o.shape, name
        assert np.isfinite(raw).all(), "%s %s: %d non-finite raw outputs" % (case["id"], name, int((~np.isfinite(raw)).sum()))
        err = np.abs(raw - o) / (np.abs(o).max() + 1e-12)
        worst = max(worst, (name, float(err.max())), key=lambda t: t[1])
        if bf16:
            gmx, gmn = _BF16_LAYER_GATES[name]
            assert err.max() <= gmx and err.mean() <= gmn, (case["id"], name, float(err.max()), float(err.mean()), gmx, gmn)
        else:
            assert err.max() < gate, "%s %s: relative max err %g" % (case["id"], name, err.max())
    e_pred = float(np.abs(pred - ref).max())
    assert np.isfinite(pred).all() and e_pred <= (6e-2 if bf16 else 1e-3), (case["id"], e_pred)
    if bf16:        # ... and, bf16, each layer against the oracle fed this run's own raw outputs: one tight gate for all 17 layers
        weights, x0, _, _ = _oracle(case)
        rep = forced_layer_errors(weights, x0, case["coord"], raws, pred, gates=forced_gates(case["shape"][5]), kernels=kernels)
        print("decomposition %s %s: forced, worst layer max %.2e mean %.2e, head max %.2e mean %.2e" % (
            case["id"], extra or "", max(v[0] for v in rep["layers"].values()), max(v[1] for v in rep["layers"].values()), rep["head"][0], rep["head"][1]))
        assert not rep["failures"], "%s:\n%s" % (case["id"], "\n".join(rep["failures"]))
    # 2. against whole tiles only
    pred_u, raws_u, _, plan_u = _forward(case, dict(extra or {}, TAILSPLIT=0))
    assert all(k[2] == 0 for k in plan_u.kernels()[:17]), plan_u.kernels()
    worst_u, worst_bf16 = ("", 0.0), ("", 0.0)
    for name, raw in raws.items():
        assert np.isfinite(raws_u[name]).all(), (case["id"], name)
        d = float(np.abs(raw - raws_u[name]).max() / (np.abs(want[name]).max() + 1e-12))
        worst_u = max(worst_u, (name, d), key=lambda t: t[1])
        tol = 2e-5 if not bf16 else (5e-4 if name == "conv1_1" else _BF16_LAYER_GATES[name][0])
        assert d <= tol, "%s %s: split vs whole tiles %g" % (case["id"], name, d)
        if bf16:        # the mean as well (see the module docstring)
            mean = float((np.abs(raw - raws_u[name]) / (np.abs(want[name]).max() + 1e-12)).mean())
            worst_bf16 = max(worst_bf16, (name, mean), key=lambda t: t[1])
            assert mean <= (2e-5 if name == "conv1_1" else _BF16_LAYER_GATES[name][1]), (case["id"], name, mean)
    d_pred = float(np.abs(pred - pred_u).max())
    assert d_pred <= (4e-2 if bf16 else 2e-5), (case["id"], d_pred)
    if bf16:
        m_pred = float(np.abs(pred - pred_u).mean())
        assert m_pred <= 3e-3, (case["id"], m_pred)
        print("decomposition %s %s: bf16 split vs whole tiles, worst layer mean %.2e (%s), prediction mean %.2e"
              % (case["id"], extra or "", worst_bf16[1], worst_bf16[0], m_pred))
    # 3. the separate fix-up launch
    pred_f, raws_f, _, plan_f = _forward(case, dict(extra or {}, FIXUP_KERNEL=1))
    assert [k[1:] for k in plan_f.kernels()] == [k[1:] for k in plan.kernels()]
    assert np.array_equal(pred_f, pred), (case["id"], float(np.abs(pred_f - pred).max()))
    for name, raw in raws.items():
        assert np.array_equal(raws_f[name], raw), (case["id"], name)
    _model(case)._ws_cache.clear()       # (plans and workspaces of this case: up to 3 x 80 MB of slabs at 304 CUs)
    print("decomposition %s %s: worst layer vs oracle %.2e (%s), prediction vs oracle %.2e | worst layer vs whole tiles %.2e (%s), prediction %.2e"
          % (case["id"], extra or "", worst[1], worst[0], e_pred, worst_u[1], worst_u[0], d_pred))


@pytest.mark.parametrize("cid", [c["id"] for c in DECOMP_CASES])
def test_split_plans_match_the_oracle_the_whole_tile_plan_and_the_fixup_launch(cid):
    _check_case(CASE_BY_ID[cid])


@pytest.mark.parametrize("case,extra", OPTION_CASES, ids=[c["id"] + "-" + "-".join("%s%d" % kv for kv in e.items()) for c, e in OPTION_CASES])
def test_other_split_options(case, extra):
    """TAILSPLIT = 2 (residency-aware: the tiles beyond a multiple of 5 NUM_CUS), UNIFORM_SPLIT (every tile of a layer with
    NUM_CUS <= tiles < 2 NUM_CUS in s K-ranges), SPLIT_OVERHEAD (another cost rule for the remainder's split): live options of
    the default library that no default plan takes.  Checks 1 - 4, and the option really changed a layer's workgroups."""
    assert changed_layers(case, extra), (case["id"], extra)
    _check_case(case, extra)


@pytest.mark.parametrize("cid", BACK_TO_BACK_CASES)
def test_different_inputs_back_to_back_equal_their_solo_runs(cid):
    """Repeating one input cannot show a stale slab, ticket or LayerNorm shard (it holds the values the next forward writes):
    four DIFFERENT inputs queued without a host sync in between must each equal, bit for bit, their run on an idle device."""
    import torch
    case = CASE_BY_ID[cid]
    b, h, w, cin, nout, ngf = case["shape"]
    m = _model(case)
    _set_options(m, case)
    poison_workspace(m, b, h, w, cin, nout, ngf)
    g = torch.Generator(device="cuda").manual_seed(7)
    xs = [torch.rand((b, h, w, cin), device="cuda", generator=g) * (0.5 + 0.25 * i) - 0.3 * i for i in range(4)]
    solo = []
    for x in xs:
        torch.cuda.synchronize()
        solo.append(m.run_net(x, nout, ngf).clone())
        torch.cuda.synchronize()
        assert bool(torch.isfinite(solo[-1]).all())
    assert m.network_status() == 0
    assert not torch.equal(solo[0], solo[1])
    for rep in range(3):
        queued = [m.run_net(x, nout, ngf) for x in xs]
        torch.cuda.synchronize()
        for i, (q, s) in enumerate(zip(queued, solo)):
            assert torch.equal(q, s), (cid, rep, i, float((q - s).abs().max()))
