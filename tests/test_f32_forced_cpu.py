"""The teacher-forced fp64 check of the fp32 network tier, WITHOUT a GPU: the oracle's fp64 mode, the cases of the GPU file and the kernel instantiations they reach,
and proof that the checker sees what the older gates do not.

Every older fp32 layer test compares a free-running device plan with the free-running fp32 oracle under 2e-4 of the layer scale (6e-4 for the fp16 three-product
form; 1e-5 in tests/test_gpu_layer_probe.py, two shapes).  A kernel that lost ONE of the three small products of the six-product form, or reads the l plane of its
weights or its patch from the wrong place, is off by 2e-6 .. 5e-6 and passes all of them -- with 16-bit operands.  tests.util.forced_layer_errors_f32 recomputes every
layer in fp64 from the tensors the implementation under test stored for that layer's own sources (oracle/nets.py forward(precision="fp64", forced_raw=...,
forced_act=...)) and holds it to the gates of its kernel's arithmetic (tests.util.F32_FORCED_GATES: 3 x the worst value of the oracle's own emulation of that
arithmetic, tools/f32_forced_gates.py, profiles/f32_forced_gates.txt -- 1.4e-6 max and 5.2e-7 rms for the six-product form).

Here:
  * the fp64 mode and the second forcing entry point (activations) leave the fp32 forward alone and agree with it;
  * FORCED_CASES, the plans tests/test_gpu_f32_forced.py executes, and COVERAGE: every fp32 conv instantiation the launchers of cnn_x3.hip, cnn_halo.hip and
    cnn_igemm.hip have, spelled as cnn_plan.hip's msi_net_plan_layer_kernel spells it, is reached by a case or named in UNREACHABLE with the planner line that says why;
  * the stand-in in the device's place passes every gate as it is, with raw and with in-place normalized layers; with ONE fault in ONE layer (tools/f32_forced_gates.py
    FAULTS x FAULT_LAYERS) it fails at exactly that layer -- and the older gates let every one of them through (printed; the table is kept in the profile).
The rms metric is the one that separates: the smallest fault (l.h lost in one of two K-ranges) is 2.9 x the rms gate and 1.2 x the max gate."""
import os
import re
import sys

import numpy as np
import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "tools"))
import f32_forced_gates as standin   # noqa: E402  (tools/f32_forced_gates.py: the stand-in and the list of faults)
from tests.test_plan_decomposition import A, ALL, CASE_BY_ID, E, _case, plan_for   # noqa: E402
from tests.util import F32_FORCED_GATES, f32_arithmetic, forced_layer_errors_f32, rel_max_rms   # noqa: E402

SKIP6 = 1 << 10      # HALO_SKIP bit of conv6_1: the tap kernel there, so conv3_3 is normalized in place and conv4_1 loads an activation (APPLY = 0)
# NUM_CUS is set in every case, so the plans -- and COVERAGE below -- are the same on any part; A-cus256 / E-cus256 pin the CU count an MI355X reports (and a plan
# takes where there is no device): the plan that part takes by default, by value and not by leaving the option alone
FORCED_CASES = [CASE_BY_ID[i] for i in ("A-cus13", "B-cus9", "A-tile8-cus13", "E-tile8-cus11", "C-cus304", "E-f16-cus9", "A-native-cus9", "E-native-cus19")] + [
    _case("A-cus256", "f32", A, True, 256),
    _case("E-cus256", "f32", E, False, 256),
    _case("A-skip6-cus13", "f32", A, True, 13, {"HALO_SKIP": SKIP6}),                               # conv_halo_x3_kernel<3, 0, 3>
    _case("E-skip6-cus9", "f32", E, False, 9, {"HALO_SKIP": SKIP6}),                                # conv_halo_x3_kernel<2, 0, 3>
    _case("A-f16-skip6-cus13", "f32", A, True, 13, {"F32_SPLIT_F16": ALL, "HALO_SKIP": SKIP6}),     # conv_halo_x3_kernel<3, 0, 2> and <3, 1, 2>
    _case("E-f16-skip6-cus9", "f32", E, False, 9, {"F32_SPLIT_F16": ALL, "HALO_SKIP": SKIP6}),      # conv_halo_x3_kernel<2, 0, 2>
]
FORCED_BY_ID = {c["id"]: c for c in FORCED_CASES}

# instantiation -> the cases whose plan takes it (test_coverage_table_is_what_the_plans_give recomputes this)
COVERAGE = {
    "conv_halo8_s2_x3_kernel<1>": ["A-tile8-cus13", "E-tile8-cus11"],
    "conv_halo8_x3_kernel<0, 3>": ["A-cus13", "B-cus9", "A-tile8-cus13", "E-tile8-cus11", "A-skip6-cus13", "E-skip6-cus9"],
    "conv_halo8_x3_kernel<1, 3>": ["A-cus13", "B-cus9", "A-tile8-cus13", "E-tile8-cus11", "A-skip6-cus13", "E-skip6-cus9"],
    "conv_halo_kernel<1, 0>": ["A-native-cus9", "E-native-cus19"],
    "conv_halo_kernel<1, 1>": ["A-native-cus9", "E-native-cus19"],
    "conv_halo_kernel<2, 0>": ["E-native-cus19"],
    "conv_halo_kernel<2, 1>": ["A-native-cus9", "E-native-cus19"],
    "conv_halo_s2_kernel<1>": ["A-native-cus9"],
    "conv_halo_s2_x3_kernel<1, 2>": ["E-f16-cus9", "A-f16-skip6-cus13", "E-f16-skip6-cus9"],
    "conv_halo_s2_x3_kernel<1, 3>": ["A-cus13", "B-cus9", "E-tile8-cus11", "C-cus304", "A-cus256", "E-cus256", "A-skip6-cus13", "E-skip6-cus9"],
    "conv_halo_x3_kernel<1, 0, 2>": ["E-f16-cus9", "A-f16-skip6-cus13", "E-f16-skip6-cus9"],
    "conv_halo_x3_kernel<1, 0, 3>": ["C-cus304", "A-cus256", "E-cus256"],
    "conv_halo_x3_kernel<1, 1, 2>": ["E-f16-cus9", "A-f16-skip6-cus13", "E-f16-skip6-cus9"],
    "conv_halo_x3_kernel<1, 1, 3>": ["A-cus13", "B-cus9", "C-cus304", "A-cus256", "E-cus256", "A-skip6-cus13", "E-skip6-cus9"],
    "conv_halo_x3_kernel<2, 0, 2>": ["E-f16-skip6-cus9"],
    "conv_halo_x3_kernel<2, 0, 3>": ["E-skip6-cus9"],
    "conv_halo_x3_kernel<2, 1, 2>": ["E-f16-cus9", "E-f16-skip6-cus9"],
    "conv_halo_x3_kernel<2, 1, 3>": ["B-cus9", "E-tile8-cus11", "E-cus256", "E-skip6-cus9"],
    "conv_halo_x3_kernel<3, 0, 2>": ["A-f16-skip6-cus13"],
    "conv_halo_x3_kernel<3, 0, 3>": ["A-skip6-cus13"],
    "conv_halo_x3_kernel<3, 1, 2>": ["A-f16-skip6-cus13"],
    "conv_halo_x3_kernel<3, 1, 3>": ["A-cus13", "A-tile8-cus13", "C-cus304", "A-cus256", "A-skip6-cus13"],
    "conv_igemm_kernel<64, 64, 0, 0>": ["A-native-cus9", "E-native-cus19"],
    "conv_igemm_kernel<64, 64, 1, 0>": ["E-native-cus19", "A-skip6-cus13", "E-skip6-cus9", "A-f16-skip6-cus13", "E-f16-skip6-cus9"],
    "conv_igemm_kernel<64, 64, 2, 0>": ["A-cus13", "B-cus9", "A-tile8-cus13", "E-tile8-cus11", "C-cus304", "E-f16-cus9", "A-native-cus9", "E-native-cus19", "A-cus256", "E-cus256", "A-skip6-cus13", "E-skip6-cus9", "A-f16-skip6-cus13", "E-f16-skip6-cus9"],
    "convt_halo8_x3_kernel": ["B-cus9", "A-tile8-cus13"],
    "convt_halo_kernel": ["A-native-cus9"],
    "convt_halo_x3_kernel<2>": ["E-f16-cus9", "A-f16-skip6-cus13", "E-f16-skip6-cus9"],
    "convt_halo_x3_kernel<3>": ["A-cus13", "B-cus9", "A-tile8-cus13", "E-tile8-cus11", "C-cus304", "A-cus256", "E-cus256", "A-skip6-cus13", "E-skip6-cus9"],
}

# instantiation -> (line of matryodshka_amd/csrc/cnn_plan.hip, text on that line, why no plan of ANY shape takes it)
_S2_WHY = ("a stride-2 layer's source (conv1_1, conv2_1, conv3_2) has no other consumer, and in an fp32 plan a halo kernel can always apply its source's LayerNorm "
           "while staging: the source is never normalized in memory, so the stride-2 halo kernels only run with APPLY = 1")
UNREACHABLE = {
    "conv_halo_s2_x3_kernel<0, 2>": (278, "C.is_halo() && !C.is_convt() && L.src0 == s && (!bf16 ||", _S2_WHY),
    "conv_halo_s2_x3_kernel<0, 3>": (278, "C.is_halo() && !C.is_convt() && L.src0 == s && (!bf16 ||", _S2_WHY),
    "conv_halo8_s2_x3_kernel<0>": (278, "C.is_halo() && !C.is_convt() && L.src0 == s && (!bf16 ||", _S2_WHY),
    "conv_halo_s2_kernel<0>": (278, "C.is_halo() && !C.is_convt() && L.src0 == s && (!bf16 ||", _S2_WHY),
}


def built_f32_instantiations():
    """What the launchers can launch for an fp32 plan: the cases of launch_x3's switch (cnn_x3.hip), of launch_halo_f32's (cnn_halo.hip) and the BF16 = 0 cases of the
    tap kernel's (cnn_igemm.hip), spelled by the formats of msi_net_plan_layer_kernel (cnn_plan.hip)."""
    src = os.path.join(ROOT, "matryodshka_amd", "csrc")
    names = {fam: (fmt, re.findall(r"V\.(\w+)", fields)) for fam, fmt, fields in
             re.findall(r'case (\w+): snprintf\(name, name_bytes, "([^"]+)"((?:, V\.\w+)*)\);', open(os.path.join(src, "cnn_plan.hip")).read())}
    out = set()
    for fname, order in (("cnn_x3.hip", ("rate", "apply", "planes")), ("cnn_halo.hip", ("rate", "apply"))):      # (the launchers' vkey(family, ...) argument order)
        for fam, args in re.findall(r"case vkey\((\w+)((?:, \d+)*)\): return launch_", open(os.path.join(src, fname)).read()):
            v = dict.fromkeys(order, 0)
            v.update(zip(order, (int(a) for a in args.split(", ")[1:])))
            fmt, fields = names[fam]
            out.add(fmt % tuple(v[f] for f in fields))
    mode = {"MODE_CONV": 0, "MODE_CONVT": 1, "MODE_HEAD": 2}
    for bm, bn, m, bf in re.findall(r"case vkey\(CONV_IGEMM, (\d), (\d), (MODE_\w+), (\d)\): return launch_conv_mode", open(os.path.join(src, "cnn_igemm.hip")).read()):
        if bf == "0":
            out.add(names["CONV_IGEMM"][0] % (64 * int(bm), 64 * int(bn), mode[m], 0))
    return out


def test_coverage_table_is_what_the_plans_give():
    got = {}
    for case in FORCED_CASES:
        for k in sorted({k[0] for k in plan_for(case).kernels()}):
            got.setdefault(k, []).append(case["id"])
    assert got == COVERAGE, "\n".join("    %r: %r," % kv for kv in sorted(got.items()))


def test_every_fp32_instantiation_is_reached_or_named():
    built = built_f32_instantiations()
    assert len(built) == 33, sorted(built)          # 23 split forms, 7 fp32 halo forms, 3 tap forms: the regular expressions above still read the switches
    assert not set(COVERAGE) & set(UNREACHABLE)
    assert set(COVERAGE) | set(UNREACHABLE) == built, (sorted(built - set(COVERAGE) - set(UNREACHABLE)), sorted((set(COVERAGE) | set(UNREACHABLE)) - built))
    lines = open(os.path.join(ROOT, "matryodshka_amd", "csrc", "cnn_plan.hip")).read().split("\n")
    for inst, (line, text, why) in UNREACHABLE.items():      # (within a few lines: an edit above them must not fail this)
        assert why and any(text in ln for ln in lines[max(0, line - 13):line + 12]), (inst, line, lines[line - 1])
    # every arithmetic has its gates, and a case whose every layer runs it
    assert {f32_arithmetic(k) for k in built} == set(F32_FORCED_GATES) == {"x3", "f16", "native"}


def test_no_plan_of_the_decomposition_sweep_shapes_takes_an_unreachable_instantiation():
    from tests.test_plan_decomposition import CONFIG_DESCS, SWEEP_OPTIONS, _native, _options
    N, nets = _native()
    for what, dtype, shape, coord in CONFIG_DESCS:
        if dtype != "f32":
            continue
        b, h, w, cin, nout, ngf = shape
        for named in list(SWEEP_OPTIONS) + [{"HALO_SKIP": SKIP6}, {"F32_SPLIT_F16": ALL}, {"HALO_SKIP": 0x3ffff & ~0x4a}]:     # (the last: every layer but the stride-2 ones on the tap kernel)
            ks = {k[0] for k in N.NetPlan(nets.make_desc(b, h, w, cin, nout, ngf, coord, dtype), _options(N, named)).kernels()}
            assert not ks & set(UNREACHABLE), (what, named, sorted(ks & set(UNREACHABLE)))


def test_the_arithmetic_is_read_off_the_kernel_name():
    for k in built_f32_instantiations():
        planes2 = "_x3_kernel<" in k and k.endswith("2>")
        assert f32_arithmetic(k) == ("native" if "_x3_" not in k else ("f16" if planes2 else "x3")), k
    assert f32_arithmetic("conv_halo8_s2_x3_kernel<1>") == "x3" and f32_arithmetic("convt_halo8_x3_kernel") == "x3"
    assert f32_arithmetic("convt_halo_x3_kernel<2>") == "f16" and f32_arithmetic("conv_halo_s2_x3_kernel<1, 2>") == "f16"
    assert f32_arithmetic("conv_igemm_kernel<64, 64, 2, 0>") == "native" and f32_arithmetic("convt_halo_kernel") == "native"


# ---- the oracle's fp64 mode and the forcing of activations
@pytest.mark.parametrize("coord", [True, False], ids=["coord", "wrap"])
def test_fp64_mode_agrees_with_the_fp32_forward_and_forcing_own_tensors_changes_nothing(coord):
    from oracle import nets as onets
    b, h, w, cin, nout, ngf = 2, 16, 32, 16, 8, 16
    weights = onets.init_weights(cin, nout, ngf=ngf, coord_net=coord, seed=5, randomize_affine=True)
    x = np.random.RandomState(6).uniform(-1, 1, size=(b, h, w, cin)).astype(np.float32)
    ref, acts = onets.forward(weights, x, coord_net=coord, return_activations=True)
    names = standin.layer_names()
    # the default is the fp32 forward it was; the new arguments at their defaults change nothing
    p, a = onets.forward(weights, x, coord_net=coord, return_activations=True, precision="fp32", forced_act=None)
    assert p.dtype == np.float32 and np.array_equal(p, ref) and all(np.array_equal(a[k], acts[k]) for k in acts)
    # fp64, free-running: float64 tensors, close to the fp32 forward (whose error grows with depth: 1e-5 is far above it, far below a wrong graph)
    p64, a64 = onets.forward(weights, x, coord_net=coord, return_activations=True, precision="fp64")
    assert p64.dtype == np.float64 and sorted(a64) == sorted(acts) and all(a64[n + "/raw"].dtype == np.float64 for n in names)
    assert max(rel_max_rms(acts[n + "/raw"], a64[n + "/raw"])[0] for n in names) < 1e-5 and np.abs(p64 - ref).max() < 1e-5
    # fp64, forced by its own (float32-rounded) tensors: each layer within one fp32 rounding of its inputs' effect
    own_raw = {n: a64[n + "/raw"].astype(np.float32) for n in names}
    pf, af = onets.forward(weights, x, coord_net=coord, return_activations=True, precision="fp64", forced_raw=own_raw)
    assert max(rel_max_rms(af[n + "/raw"], a64[n + "/raw"])[0] for n in names) < 2e-7
    # activations force like raw outputs: the fp32 forward forced by its OWN activations (some layers) and raw outputs (the rest) is itself, bit for bit
    some = set(names[::3]) | {"conv6_1", "conv8_2"}
    p2, a2 = onets.forward(weights, x, coord_net=coord, return_activations=True, forced_raw={n: acts[n + "/raw"] for n in names if n not in some},
                           forced_act={n: acts[n] for n in some})
    assert np.array_equal(p2, ref) and all(np.array_equal(a2[k], acts[k]) for k in acts)
    # a forced activation is what the consumers read; the layer still records its own
    bumped = acts["conv3_2"] * np.float32(1.5)
    p3, a3 = onets.forward(weights, x, coord_net=coord, return_activations=True, forced_act={"conv3_2": bumped})
    assert np.array_equal(a3["conv3_2"], acts["conv3_2"]) and np.array_equal(a3["conv3_1/raw"], acts["conv3_1/raw"])
    assert not np.array_equal(a3["conv3_3/raw"], acts["conv3_3/raw"])
    with pytest.raises(AssertionError):
        onets.forward(weights, x, coord_net=coord, forced_raw={"conv3_2": acts["conv3_2/raw"]}, forced_act={"conv3_2": bumped})
    with pytest.raises(AssertionError):
        onets.forward(weights, x, coord_net=coord, precision="fp64", split3_products=True)


# ---- the checker's teeth
# the layers an fp32 plan typically normalizes in place (the conv-transposes' outputs and a source of two consumers), for the runs that exercise that path
NORMALIZED = ("conv1_2", "conv3_3", "conv6_1", "conv7_1", "conv8_1")


@pytest.mark.parametrize("normalized", [(), NORMALIZED], ids=["raw", "normalized"])
@pytest.mark.parametrize("coord", [True, False], ids=["coord", "wrap"])
@pytest.mark.parametrize("form", ["x3", "f16"])
def test_the_fault_free_stand_in_passes_every_gate(form, coord, normalized):
    rep, free, e_pred = standin.fault_report(None, form, coord, normalized)
    assert len(rep["layers"]) == 17 and not rep["failures"], "\n".join(rep["failures"])
    assert sorted(n for n, w in rep["compared"].items() if w == "activation") == sorted(normalized)
    g = F32_FORCED_GATES[form]
    print("%s %s %s: worst layer max %.2e (gate %.2e), rms %.2e (gate %.2e); head %.2e / %.2e" % (
        form, "coord" if coord else "wrap", "normalized" if normalized else "raw", max(v[0] for v in rep["layers"].values()), g["layer_max"],
        max(v[1] for v in rep["layers"].values()), g["layer_rms"], rep["head"][0], rep["head"][1]))


@pytest.mark.parametrize("kind", list(standin.FAULT_LAYERS))
@pytest.mark.parametrize("fault", list(standin.FAULTS))
def test_one_fault_in_one_layer_fails_there_and_nowhere_else_and_passes_the_older_gates(fault, kind):
    layer = standin.FAULT_LAYERS[kind]
    form = standin.FAULTS[fault][0]
    rep, free, e_pred = standin.fault_report(fault, layer)
    mx, rms = rep["layers"][layer]
    g = F32_FORCED_GATES[form]
    print("%s at %s (%s): forced max %.2e = %.1f x gate, rms %.2e = %.1f x gate; free-running worst layer %.2e, prediction %.1e (gates %.0e, 1e-3)"
          % (fault, layer, kind, mx, mx / g["layer_max"], rms, rms / g["layer_rms"], max(free.values()), e_pred, standin.OLD_GATES[form]))
    assert rep["failed_layers"] == [layer], (fault, layer, rep["failed_layers"], rep["failures"])
    assert rep["failures"][0].startswith(layer + " [" + standin.KERNEL_OF[form])
    assert rms > 2 * g["layer_rms"]                                     # the separation the gates were required to have: at least 2 x, on the rms metric
    # the older gates -- every layer against the free-running fp32 oracle, and the prediction -- let it through
    assert max(free.values()) < standin.OLD_GATES[form] and e_pred <= 1e-3, (fault, layer, max(free.values()), e_pred)


@pytest.mark.parametrize("fault,layer,coord", [("drop_mm", "conv7_1", True), ("wl_roll", "conv3_3", True), ("drop_lh", "conv8_1", False), ("xl_shift", "conv6_1", False)])
def test_a_fault_in_a_layer_normalized_in_place_is_seen_in_its_activation(fault, layer, coord):
    """The buffer of such a layer holds LayerNorm + ReLU of the faulty raw output: the layer is compared as an activation, never left out (msi_train_net's
    conv-transposes: the stored [5:-5] crop, pasted into the oracle's own border)."""
    rep, free, e_pred = standin.fault_report(fault, layer, coord, NORMALIZED)
    assert rep["compared"][layer] == "activation" and rep["failed_layers"] == [layer], (rep["failed_layers"], rep["failures"])
    assert "activation" in rep["failures"][0]
    assert max(free.values()) < 2e-4 and e_pred <= 1e-3


def test_a_failure_names_the_elements_and_the_kernel_and_nan_fails():
    weights, x = standin.mutation_case(True)
    pred, stored = standin.device_standin(weights, x, True, "x3", "drop_hl", "conv4_2")
    kernels = [("conv_halo_x3_kernel<3, 1, 3>", 0, 0)] * 17 + [("conv_igemm_kernel<64, 64, 2, 0>", 0, 0)]
    rep = forced_layer_errors_f32(weights, x, True, stored, (), pred, gates=F32_FORCED_GATES, kernels=kernels)
    assert rep["failed_layers"] == ["conv4_2"] and "[conv_halo_x3_kernel<3, 1, 3>, x3, raw]" in rep["failures"][0]
    assert rep["over"]["conv4_2"] > 0 and len(rep["first"]["conv4_2"]) == 4 and all(n == 0 for k, n in rep["over"].items() if k != "conv4_2")
    # a non-finite stored value fails its layer
    stored = dict(stored, conv2_1=stored["conv2_1"].copy())
    stored["conv2_1"][0, 3, 5, 7] = np.nan
    rep = forced_layer_errors_f32(weights, x, True, stored, (), pred, gates=F32_FORCED_GATES, kernels=kernels)
    assert "conv2_1" in rep["failed_layers"]
