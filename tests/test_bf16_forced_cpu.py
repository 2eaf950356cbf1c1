"""The teacher-forced check of the bf16 network tier, WITHOUT a GPU: its cases and the kernels their plans take, and proof that the checker has teeth.

Every older bf16 layer test compares the device with the oracle's FREE-RUNNING bf16 forward: both sides round activations to bf16, one flipped rounding
moves everything downstream, and the gates have to follow that drift (_BF16_LAYER_GATES grows from 5e-4 of the layer scale at conv1_1 to 1.7e-2 at conv6_3).
tests.util.forced_layer_errors feeds every layer of the oracle the raw outputs the implementation under test stored for that layer's own sources
(oracle/nets.py forward(forced_raw=...)), so what is left is the layer's own freedom -- the same at conv8_2 as at conv1_1 -- and one gate per network width
(tests.util.BF16_FORCED_GATES, measured on the CPU by tools/bf16_forced_gates.py; profiles/bf16_forced_gates.txt) holds for all 17 layers.

Here:
  * FORCED_CASES, the plans tests/test_gpu_bf16_forced.py executes, with the kernel of every layer pinned (KERNELS) and the table of which case reaches which
    bf16 instantiation (COVERAGE): every instantiation the launchers' switches of cnn_bf16.hip and cnn_igemm.hip have is reached by a case;
  * the stand-in of tools/bf16_forced_gates.py in the device's place: it passes every gate as it is, and with ONE layer made subtly wrong (MUTATIONS) it fails
    the forced gates at that layer and at no other (one fault: and at its consumer) -- while the chained gates pass three of the five faults (printed; the table is kept in the profile);
  * forward(forced_raw=None) is the forward it was, and forcing a layer to its own output changes nothing, bit for bit."""
import os
import re
import sys

import numpy as np
import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "tools"))
import bf16_forced_gates as standin   # noqa: E402  (tools/bf16_forced_gates.py: the CPU stand-in and the list of faults)
from tests.test_plan_decomposition import _case, plan_for   # noqa: E402
from tests.util import BF16_FORCED_GATES, forced_gates, forced_layer_errors   # noqa: E402

A = (1, 64, 128, 64, 16, 64)      # the smallest shape at which every level tiles into the bf16 halo kernels (conv4_x: 8 x 16)
# NUM_CUS is set in every case (256: an MI355X), so the plans -- conv8_1 of A-wrap cut into K-ranges, the tap layers of W144 -- are the same on any part
FORCED_CASES = [
    _case("A", "bf16", A, True, 256),
    _case("A-waves4", "bf16", A, True, 256, {"BF16_WAVES": 4}),                  # the four <128, 128, ., ., 4> forms
    _case("A-stage0", "bf16", A, True, 256, {"BF16_STAGE_RAW": 0}),              # conv8_2 on <256, 64, 1, 0, 4>, fed from the bf16 copy
    _case("A-stage3", "bf16", A, True, 256, {"BF16_STAGE_RAW": 3}),              # convt_halo_bf16_kernel<128, 64, 1>; conv2_1 becomes <128, 128, 1, 1, 8>
    _case("A-wrap", "bf16", A, False, 256),                                      # wrap padding through the halo kernels, the VALID conv-transposes on the tap kernel
    _case("A-tap-bigtile", "bf16", A, True, 256, {"HALO": 0, "BIGTILE": 2}),     # the 128 x 128 and 128 x 64 tap tiles
    _case("A-tap-cus24", "bf16", A, True, 24, {"BIGTILE": 0}),                   # 64 x 64 tap tiles, 14 of 17 layers cut into K-ranges, in-launch hand-off (and FIXUP_KERNEL = 1)
    _case("B2-mixed", "bf16", (2, 32, 64, 64, 16, 32), True, 256),               # batch 2, halo and tap layers in one plan
    _case("R-coord", "bf16", (2, 16, 40, 24, 8, 16), True, 256),                 # ragged tiles, channel counts that are no multiple of 64
    _case("R-wrap", "bf16", (2, 16, 40, 24, 8, 16), False, 256),
    # conv_halo_bf16_s2_kernel<0, 4>: a stride-2 layer's one source has no other consumer, so the plan always lets it stage the raw output (APPLY = 1) -- unless its
    # input has more than the 512 channels the staging table holds (plan_layers: `L.c0 <= 512`), which is conv3_3 (4 ngf channels) from ngf = 144 on
    _case("W144-s2raw", "bf16", (1, 64, 128, 16, 8, 144), True, 256),
    _case("B1-head128", "bf16", (1, 32, 64, 64, 128, 32), True, 256, {"BIGTILE": 2}),   # the head on the 128 x 128 tile (what configs[2] takes), ...
    _case("B1-head64", "bf16", (1, 32, 64, 64, 64, 32), True, 256, {"BIGTILE": 2}),     # ... and on 128 x 64
]
FORCED_BY_ID = {c["id"]: c for c in FORCED_CASES}
SPLIT_LAYERS = {"A-wrap": 1, "A-tap-cus24": 14, "W144-s2raw": 6}     # layers with tiles cut into K-ranges (every other case: none)

# every layer's kernel, graph order (17 conv layers, then the head); H / S / T / G = conv_halo_bf16 / conv_halo_bf16_s2 / convt_halo_bf16 / conv_igemm _kernel
_ALIAS = {"H": "conv_halo_bf16_kernel", "S": "conv_halo_bf16_s2_kernel", "T": "convt_halo_bf16_kernel", "G": "conv_igemm_kernel"}
KERNELS = {
    "A": "H<256, 64, 1, 0, 4> | S<1, 4> | H<128, 128, 1, 0, 8> | S<1, 4> | H<128, 128, 1, 0, 8> | H<128, 128, 1, 1, 8> | S<1, 4> | H<128, 128, 2, 0, 8> | 2 x H<128, 128, 2, 1, 8> | T<128, 128, 0> | 2 x H<128, 128, 1, 1, 8> | T<128, 128, 0> | H<128, 128, 1, 1, 8> | T<128, 64, 0> | H<256, 64, 1, 1, 4> | G<64, 64, 2, 1>",
    "A-waves4": "H<256, 64, 1, 0, 4> | S<1, 4> | H<128, 128, 1, 0, 4> | S<1, 4> | H<128, 128, 1, 0, 4> | H<128, 128, 1, 1, 4> | S<1, 4> | H<128, 128, 2, 0, 4> | 2 x H<128, 128, 2, 1, 4> | T<128, 128, 0> | 2 x H<128, 128, 1, 1, 4> | T<128, 128, 0> | H<128, 128, 1, 1, 4> | T<128, 64, 0> | H<256, 64, 1, 1, 4> | G<64, 64, 2, 1>",
    "A-stage0": "H<256, 64, 1, 0, 4> | S<1, 4> | H<128, 128, 1, 0, 8> | S<1, 4> | H<128, 128, 1, 0, 8> | H<128, 128, 1, 1, 8> | S<1, 4> | H<128, 128, 2, 0, 8> | 2 x H<128, 128, 2, 1, 8> | T<128, 128, 0> | 2 x H<128, 128, 1, 1, 8> | T<128, 128, 0> | H<128, 128, 1, 1, 8> | T<128, 64, 0> | H<256, 64, 1, 0, 4> | G<64, 64, 2, 1>",
    "A-stage3": "H<256, 64, 1, 0, 4> | S<1, 4> | H<128, 128, 1, 1, 8> | S<1, 4> | H<128, 128, 1, 0, 8> | H<128, 128, 1, 1, 8> | S<1, 4> | H<128, 128, 2, 0, 8> | 2 x H<128, 128, 2, 1, 8> | T<128, 128, 0> | 2 x H<128, 128, 1, 1, 8> | T<128, 128, 0> | H<128, 128, 1, 1, 8> | T<128, 64, 1> | H<256, 64, 1, 1, 4> | G<64, 64, 2, 1>",
    "A-wrap": "H<256, 64, 1, 0, 4> | S<1, 4> | H<128, 128, 1, 0, 8> | S<1, 4> | H<128, 128, 1, 0, 8> | H<128, 128, 1, 1, 8> | S<1, 4> | H<128, 128, 2, 0, 8> | 2 x H<128, 128, 2, 1, 8> | G<64, 64, 1, 1> | 2 x H<128, 128, 1, 1, 8> | G<64, 64, 1, 1> | H<128, 128, 1, 1, 8> | G<64, 64, 1, 1> | H<256, 64, 1, 1, 4> | G<64, 64, 2, 1>",
    "A-tap-bigtile": "G<128, 64, 0, 1> | 9 x G<128, 128, 0, 1> | G<128, 128, 1, 1> | 2 x G<128, 128, 0, 1> | G<128, 128, 1, 1> | G<128, 128, 0, 1> | G<128, 64, 1, 1> | G<128, 64, 0, 1> | G<64, 64, 2, 1>",
    "A-tap-cus24": "10 x G<64, 64, 0, 1> | G<64, 64, 1, 1> | 2 x G<64, 64, 0, 1> | G<64, 64, 1, 1> | G<64, 64, 0, 1> | G<64, 64, 1, 1> | G<64, 64, 0, 1> | G<64, 64, 2, 1>",
    "B2-mixed": "2 x G<64, 64, 0, 1> | H<256, 64, 1, 0, 4> | S<1, 4> | H<128, 128, 1, 0, 8> | H<128, 128, 1, 1, 8> | 4 x G<64, 64, 0, 1> | G<64, 64, 1, 1> | 2 x H<128, 128, 1, 1, 8> | T<128, 64, 0> | H<256, 64, 1, 1, 4> | G<64, 64, 1, 1> | G<64, 64, 0, 1> | G<64, 64, 2, 1>",
    "R-coord": "10 x G<64, 64, 0, 1> | G<64, 64, 1, 1> | 2 x G<64, 64, 0, 1> | G<64, 64, 1, 1> | G<64, 64, 0, 1> | G<64, 64, 1, 1> | G<64, 64, 0, 1> | G<64, 64, 2, 1>",
    "R-wrap": "10 x G<64, 64, 0, 1> | G<64, 64, 1, 1> | 2 x G<64, 64, 0, 1> | G<64, 64, 1, 1> | G<64, 64, 0, 1> | G<64, 64, 1, 1> | G<64, 64, 0, 1> | G<64, 64, 2, 1>",
    "W144-s2raw": "6 x G<64, 64, 0, 1> | S<0, 4> | 3 x H<128, 128, 2, 0, 8> | G<64, 64, 1, 1> | 2 x G<64, 64, 0, 1> | G<64, 64, 1, 1> | G<64, 64, 0, 1> | G<64, 64, 1, 1> | G<64, 64, 0, 1> | G<64, 64, 2, 1>",
    "B1-head128": "G<64, 64, 0, 1> | G<128, 64, 0, 1> | H<256, 64, 1, 0, 4> | S<1, 4> | H<128, 128, 1, 0, 8> | H<128, 128, 1, 1, 8> | 4 x G<128, 128, 0, 1> | G<128, 128, 1, 1> | 2 x H<128, 128, 1, 1, 8> | T<128, 64, 0> | H<256, 64, 1, 1, 4> | G<64, 64, 1, 1> | G<64, 64, 0, 1> | G<128, 128, 2, 1>",
    "B1-head64": "G<64, 64, 0, 1> | G<128, 64, 0, 1> | H<256, 64, 1, 0, 4> | S<1, 4> | H<128, 128, 1, 0, 8> | H<128, 128, 1, 1, 8> | 4 x G<128, 128, 0, 1> | G<128, 128, 1, 1> | 2 x H<128, 128, 1, 1, 8> | T<128, 64, 0> | H<256, 64, 1, 1, 4> | G<64, 64, 1, 1> | G<64, 64, 0, 1> | G<128, 64, 2, 1>",
}

def kernels_of(cid):
    """The 18 kernel names pinned for case `cid`."""
    out = []
    for item in KERNELS[cid].split(" | "):
        n, k = item.split(" x ") if " x " in item else (1, item)
        out += [_ALIAS[k[0]] + k[1:]] * int(n)
    assert len(out) == 18, (cid, len(out))
    return out


# instantiation -> the cases whose plan takes it (test_coverage_table_is_what_the_plans_give recomputes this)
COVERAGE = {
    "conv_halo_bf16_kernel<128, 128, 1, 0, 4>": ["A-waves4"],
    "conv_halo_bf16_kernel<128, 128, 1, 0, 8>": ["A", "A-stage0", "A-stage3", "A-wrap", "B2-mixed", "B1-head128", "B1-head64"],
    "conv_halo_bf16_kernel<128, 128, 1, 1, 4>": ["A-waves4"],
    "conv_halo_bf16_kernel<128, 128, 1, 1, 8>": ["A", "A-stage0", "A-stage3", "A-wrap", "B2-mixed", "B1-head128", "B1-head64"],
    "conv_halo_bf16_kernel<128, 128, 2, 0, 4>": ["A-waves4"],
    "conv_halo_bf16_kernel<128, 128, 2, 0, 8>": ["A", "A-stage0", "A-stage3", "A-wrap", "W144-s2raw"],
    "conv_halo_bf16_kernel<128, 128, 2, 1, 4>": ["A-waves4"],
    "conv_halo_bf16_kernel<128, 128, 2, 1, 8>": ["A", "A-stage0", "A-stage3", "A-wrap"],
    "conv_halo_bf16_kernel<256, 64, 1, 0, 4>": ["A", "A-waves4", "A-stage0", "A-stage3", "A-wrap", "B2-mixed", "B1-head128", "B1-head64"],
    "conv_halo_bf16_kernel<256, 64, 1, 1, 4>": ["A", "A-waves4", "A-stage3", "A-wrap", "B2-mixed", "B1-head128", "B1-head64"],
    "conv_halo_bf16_s2_kernel<0, 4>": ["W144-s2raw"],
    "conv_halo_bf16_s2_kernel<1, 4>": ["A", "A-waves4", "A-stage0", "A-stage3", "A-wrap", "B2-mixed", "B1-head128", "B1-head64"],
    "conv_igemm_kernel<128, 128, 0, 1>": ["A-tap-bigtile", "B1-head128", "B1-head64"],
    "conv_igemm_kernel<128, 128, 1, 1>": ["A-tap-bigtile", "B1-head128", "B1-head64"],
    "conv_igemm_kernel<128, 128, 2, 1>": ["B1-head128"],
    "conv_igemm_kernel<128, 64, 0, 1>": ["A-tap-bigtile", "B1-head128", "B1-head64"],
    "conv_igemm_kernel<128, 64, 1, 1>": ["A-tap-bigtile"],
    "conv_igemm_kernel<128, 64, 2, 1>": ["B1-head64"],
    "conv_igemm_kernel<64, 64, 0, 1>": ["A-tap-cus24", "B2-mixed", "R-coord", "R-wrap", "W144-s2raw", "B1-head128", "B1-head64"],
    "conv_igemm_kernel<64, 64, 1, 1>": ["A-wrap", "A-tap-cus24", "B2-mixed", "R-coord", "R-wrap", "W144-s2raw", "B1-head128", "B1-head64"],
    "conv_igemm_kernel<64, 64, 2, 1>": ["A", "A-waves4", "A-stage0", "A-stage3", "A-wrap", "A-tap-bigtile", "A-tap-cus24", "B2-mixed", "R-coord", "R-wrap", "W144-s2raw"],
    "convt_halo_bf16_kernel<128, 128, 0>": ["A", "A-waves4", "A-stage0", "A-stage3"],
    "convt_halo_bf16_kernel<128, 64, 0>": ["A", "A-waves4", "A-stage0", "B2-mixed", "B1-head128", "B1-head64"],
    "convt_halo_bf16_kernel<128, 64, 1>": ["A-stage3"],
}

UNREACHED = {}       # instantiation -> why no case takes it: none


def test_forced_case_plans_take_the_pinned_kernels():
    for case in FORCED_CASES:
        ks = plan_for(case).kernels()
        assert [k[0] for k in ks] == kernels_of(case["id"]), case["id"]
        assert sum(1 for k in ks if k[2]) == SPLIT_LAYERS.get(case["id"], 0), (case["id"], [k[2] for k in ks])


def test_coverage_table_is_what_the_plans_give():
    got = {}
    for case in FORCED_CASES:
        for k in sorted(set(kernels_of(case["id"]))):
            got.setdefault(k, []).append(case["id"])
    assert got == COVERAGE, "\n".join("    %r: %r," % kv for kv in sorted(got.items()))


def built_bf16_instantiations():
    """What the launchers can launch for a bf16 plan: the cases of launch_bf16_halo's switch (cnn_bf16.hip) and the BF16 = 1 cases of the tap kernel's
    (cnn_igemm.hip), spelled as msi_net_plan_layer_kernel spells them."""
    src = os.path.join(ROOT, "matryodshka_amd", "csrc")
    out = set()
    text = open(os.path.join(src, "cnn_bf16.hip")).read()
    for fn, args in re.findall(r"return (launch_halo_bf16|launch_halo_bf16_s2|launch_convt_halo_bf16)<([0-9, ]+)>\(Q, p, stream\)", text):
        out.add({"launch_halo_bf16": "conv_halo_bf16_kernel", "launch_halo_bf16_s2": "conv_halo_bf16_s2_kernel", "launch_convt_halo_bf16": "convt_halo_bf16_kernel"}[fn]
                + "<" + args + ">")
    mode = {"MODE_CONV": 0, "MODE_CONVT": 1, "MODE_HEAD": 2}
    for bm, bn, m, bf in re.findall(r"return launch_conv_mode<(\d+), (\d+), (MODE_\w+), (\d)>\(Q, p, stream\)", open(os.path.join(src, "cnn_igemm.hip")).read()):
        if bf == "1":
            out.add("conv_igemm_kernel<%s, %s, %d, 1>" % (bm, bn, mode[m]))
    return out


def test_every_bf16_instantiation_is_reached_or_named():
    built = built_bf16_instantiations()
    assert len(built) == 24, sorted(built)          # 10 + 2 + 3 halo forms, 9 tap forms: the regular expressions above still read the switches
    assert not set(COVERAGE) & set(UNREACHED)
    assert set(COVERAGE) | set(UNREACHED) == built, (sorted(built - set(COVERAGE) - set(UNREACHED)), sorted((set(COVERAGE) | set(UNREACHED)) - built))
    assert all(UNREACHED.values())


# ---- the checker's teeth
_RUNS = {}      # (coord, batch, fault) -> (weights, x, raws, pred, report): computed once, never written


def _run(coord, batch, mutate=None):
    key = (coord, batch, mutate)
    if key not in _RUNS:
        shape = (batch,) + standin.MUTATION_SHAPE[1:]
        weights, x = standin.make_case(shape, coord, standin.GATE_SEEDS[0])
        pred, raws = standin.standin_forward(weights, x, coord, mutate=mutate)
        _RUNS[key] = (weights, x, raws, pred, forced_layer_errors(weights, x, coord, raws, pred, gates=forced_gates(shape[5])))
    return _RUNS[key]


@pytest.mark.parametrize("coord,batch", [(True, 1), (False, 1), (True, 2)])
def test_the_legitimate_stand_in_passes_every_forced_gate(coord, batch):
    rep = _run(coord, batch)[4]
    assert len(rep["layers"]) == 17 and not rep["failures"], "\n".join(rep["failures"])
    # ... with the room the gates were given: 3 x the worst legitimate run
    g = BF16_FORCED_GATES[standin.MUTATION_SHAPE[5]]
    assert max(v[0] for v in rep["layers"].values()) <= g["layer_max"] / 2 and max(v[1] for v in rep["layers"].values()) <= g["layer_mean"] / 2


@pytest.mark.parametrize("what", list(standin.MUTATIONS))
def test_a_fault_in_one_layer_fails_the_forced_gates_there_and_nowhere_else(what):
    from tests.test_gpu_bf16 import _BF16_LAYER_GATES
    fault, layer, coord, batch, seen_at = standin.MUTATIONS[what]
    weights, x, raws, pred, rep = _run(coord, batch, (fault, layer))
    chained = standin.chained_errors(weights, x, coord, raws)
    chained_fail = [n for n, (mx, mn) in chained.items() if mx > _BF16_LAYER_GATES[n][0] or mn > _BF16_LAYER_GATES[n][1]]
    print("%s at %s: forced max %.2e mean %.2e bias %+.2e; chained max %.2e mean %.2e -> the chained gates %s"
          % (what, layer, rep["layers"][layer][0], rep["layers"][layer][1], rep["bias"][layer], chained[layer][0], chained[layer][1],
             ("fail at " + ", ".join(chained_fail)) if chained_fail else "PASS it"))
    # at the faulty layer and at no other (the truncating store: and at its consumer, whose statistics it falsifies -- see MUTATIONS)
    assert seen_at[0] == layer and rep["failed_layers"] == seen_at, (what, rep["failed_layers"], rep["failures"])
    assert rep["failures"][0].startswith(layer)
    # the same network without the fault is the run of the test above: it is the fault that fails
    assert not _run(coord, batch)[4]["failures"]


def test_a_failure_names_the_elements_and_the_kernel():
    fault, layer, coord, batch, _ = standin.MUTATIONS["one tap of one 64-channel chunk dropped in one tile"]
    weights, x, raws, pred, _ = _run(coord, batch, (fault, layer))
    kernels = [(k, 0, 0) for k in kernels_of("B2-mixed")]
    rep = forced_layer_errors(weights, x, coord, raws, pred, gates=BF16_FORCED_GATES[32], kernels=kernels)
    assert rep["failed_layers"] == [layer] and "[conv_halo_bf16_kernel<128, 128, 1, 1, 8>]" in rep["failures"][0]
    b, y, xx, c = rep["first"][layer]
    assert b == 0 and y < 8 and xx < 16 and c < 128                      # inside the faulty tile
    assert 0 < rep["over"][layer] <= 8 * 16 * 128 and all(n == 0 for k, n in rep["over"].items() if k != layer)


# ---- forced_raw leaves the unforced forward alone
@pytest.mark.parametrize("bf16,coord", [(False, False), (True, True)])
def test_forced_raw_none_is_the_forward_it_was_and_own_outputs_force_nothing(bf16, coord):
    from oracle import nets as onets
    b, h, w, cin, nout, ngf = 2, 16, 32, 16, 8, 16
    weights = onets.init_weights(cin, nout, ngf=ngf, coord_net=coord, seed=5, randomize_affine=True)
    x = np.random.RandomState(6).uniform(-1, 1, size=(b, h, w, cin)).astype(np.float32)
    ref, acts = onets.forward(weights, x, coord_net=coord, return_activations=True, bf16=bf16)
    names = [t[0] for t in onets.layer_table(cin, nout, ngf, coord) if t[1] != "h"]
    own = {n: acts[n + "/raw"] for n in names}
    for forced in (None, {}, own, {"conv6_1": own["conv6_1"]}):
        p, a = onets.forward(weights, x, coord_net=coord, return_activations=True, bf16=bf16, forced_raw=forced)
        assert np.array_equal(p, ref)
        assert sorted(a) == sorted(acts) and all(np.array_equal(a[k], acts[k]) for k in acts)
    # a forced layer still records its OWN raw output, and everything downstream follows the forced one
    bumped = dict(own, conv3_2=own["conv3_2"] * np.float32(1.5) + np.float32(0.25))
    p, a = onets.forward(weights, x, coord_net=coord, return_activations=True, bf16=bf16, forced_raw=bumped)
    assert np.array_equal(a["conv3_2/raw"], acts["conv3_2/raw"]) and not np.array_equal(a["conv3_2"], acts["conv3_2"])
    assert not np.array_equal(a["conv3_3/raw"], acts["conv3_3/raw"])
    assert np.array_equal(a["conv3_1"], acts["conv3_1"])
    # (forcing conv3_3 .. conv8_2 to their own outputs again cuts the change off: the prediction is the unforced one)
    assert np.array_equal(p, ref)
