"""Work decomposition of the conv kernels as a function of tiles against the CU count (plan_tiles / choose_variant / plan_layers in
matryodshka_amd/csrc/cnn_plan.hip), on the HOST: no GPU is needed to create a plan, set options and ask which kernel a layer takes.

Plan option NUM_CUS (8 .. 4096) makes small grids reach what only the 160 x 320 and 320 x 640 shapes reach on a 256-CU
device: tiles cut into K-ranges, the first tile group cut as well (split0 = 2), the in-launch hand-off and the fix-up
launch, both branches of the XCD interleave of whole tiles (n_main a multiple of 8 or not: odd CU counts), the slab-capacity
fallbacks.  DECOMP_CASES is the list of (dtype, shape, options, NUM_CUS) that tests/test_gpu_decomposition.py EXECUTES;
this module holds, without a GPU,

  * COVERAGE: which (kernel family, decomposition class) pairs each case reaches -- recomputed from the plans and compared,
    so that a planner change which turns a GPU case into a run of whole tiles fails here, before any GPU time;
  * UNREACHABLE: the pairs the planner can never produce, each with the line of cnn_plan.hip that says so (the text is looked
    for around that line, and the robustness sweep asserts that no plan produces the pair);
  * the robustness sweep: every CU count 8 .. 320, 512 and 4096 under the options that move the decomposition;
  * the plan digests: one SHA-256 per (description, option set) over that sweep and one per DECOMP_CASES / OPTION_CASES plan, of every
    layer's kernel name, workgroups, tiles cut and the bytes of msi_net_plan_layer_params (the planned kernel argument, inlaunch, fuse_ln,
    skip_apply, ln_blocks), against tests/golden/plan_digests.json (tools/plan_golden.py computes and records them): a change of the
    planner's code that is meant to change no plan changes none of them.

Classes of a layer (msi_net_plan_layer_kernel's nsplit_tiles): "whole" = no tile is cut; "rem" = 0 < nsplit_tiles < NUM_CUS,
the remainder group is cut; "both" = nsplit_tiles >= NUM_CUS, the first group is cut in two as well (NUM_CUS <= tiles < 2 NUM_CUS).
"""
import os
import sys

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "tools"))
import plan_golden   # noqa: E402  (tools/plan_golden.py: the digest functions the recorder uses)
ALL = 0x3ffff
FORCE8 = ALL | (1 << 30)          # X3_TILE8: the 8-row tiles on every eligible layer, whatever its grid
CLASSES = ("whole", "rem", "both")

# shapes (batch, H, W, Cin, Cout, ngf): 64 x 128 at most with ngf 64, 32 x 384 with ngf 32 -- what the CPU oracle does in < 1 s
A = (1, 64, 128, 96, 32, 64)      # CoordNet
B = (1, 32, 384, 96, 32, 32)      # CoordNet; 1/8 resolution: 4 x 48 (no row-parity tiles: plain rate-2 tiles)
C = (3, 64, 128, 96, 32, 64)      # batch 3, wrap padding (msi_train_net)
D = (2, 32, 128, 64, 16, 64)      # bf16, wrap padding: every conv-transpose and the 1/8-resolution layers on conv_igemm_kernel
E = (1, 32, 128, 96, 32, 64)      # wrap padding; 1/8 resolution: 4 x 16
NATIVE = {"F32_SPLIT3": 0, "HALO": 7}      # the fp32-MFMA halo kernels (conv-transposes included: HALO bit 1)


def _case(cid, dtype, shape, coord, num_cus, options=None):
    return dict(id=cid, dtype=dtype, shape=shape, coord=coord, num_cus=num_cus, options=dict(options or {}))


# option names are _native's NET_OPT_* without the prefix (resolved in plan_for: importing the binding needs the built library)
DECOMP_CASES = [
    _case("A-cus12", "f32", A, True, 12),
    _case("A-cus13", "f32", A, True, 13),
    _case("A-cus20", "f32", A, True, 20),
    _case("A-cus24", "f32", A, True, 24),
    _case("B-cus9", "f32", B, True, 9),
    _case("A-tile8-cus13", "f32", A, True, 13, {"X3_TILE8": FORCE8}),
    _case("A-tile8-cus39", "f32", A, True, 39, {"X3_TILE8": FORCE8}),
    _case("B-tile8-cus13", "f32", B, True, 13, {"X3_TILE8": FORCE8}),
    _case("E-tile8-cus11", "f32", E, False, 11, {"X3_TILE8": FORCE8}),
    _case("E-f16-cus9", "f32", E, False, 9, {"F32_SPLIT_F16": ALL}),
    _case("E-f16-cus19", "f32", E, False, 19, {"F32_SPLIT_F16": ALL}),
    _case("A-native-cus9", "f32", A, True, 9, NATIVE),
    _case("A-native-cus11", "f32", A, True, 11, NATIVE),
    _case("E-native-cus19", "f32", E, False, 19, NATIVE),
    _case("C-native-cus37", "f32", C, False, 37, NATIVE),
    _case("C-cus304", "f32", C, False, 304),          # a 304-CU part: more CUs than the device the suite runs on
    _case("D-bf16-cus9", "bf16", D, False, 9),
    _case("D-bf16-cus12", "bf16", D, False, 12),
    _case("D-bf16-cus19", "bf16", D, False, 19),
    _case("D-bf16-cus35", "bf16", D, False, 35),
]
CASE_BY_ID = {c["id"]: c for c in DECOMP_CASES}
# the two cases with the most split x3 families (one at an odd CU count): four different inputs queued back to back
BACK_TO_BACK_CASES = ("A-cus20", "A-tile8-cus13")

# the split options no default plan uses: (case, the option under test); each must change the workgroup count of a layer
OPTION_CASES = [
    (_case("C-native-cus9", "f32", C, False, 9, NATIVE), {"TAILSPLIT": 2}),       # 64 x 64 tiles, >= 5 NUM_CUS of them
    (_case("E-native-cus9", "f32", E, False, 9, NATIVE), {"UNIFORM_SPLIT": 2}),   # NUM_CUS <= tiles < 2 NUM_CUS at 1/4 resolution
    (_case("E-cus9", "f32", E, False, 9), {"UNIFORM_SPLIT": 3}),
    (_case("D-bf16-cus9", "bf16", D, False, 9), {"UNIFORM_SPLIT": 4}),
    (_case("E-cus14", "f32", E, False, 14), {"SPLIT_OVERHEAD": 4}),
    (_case("A-native-cus14", "f32", A, True, 14, NATIVE), {"SPLIT_OVERHEAD": 4}),
]


def family(kernel, coord):
    """The kernel family of a msi_net_plan_layer_kernel name (the issue's list; `coord` tells the SAME conv-transpose
    from msi_train_net's wrap-padded one, whose (H + 1) x (W + 5) rows per class are tiled raggedly)."""
    base = kernel.split("<")[0]
    args = kernel[kernel.index("<") + 1:-1].split(", ") if "<" in kernel else []
    if base == "conv_halo_x3_kernel":
        if args[2] == "2":
            return "conv_halo_x3_kernel<fp16>"
        return {"1": "conv_halo_x3_kernel<rate 1>", "2": "conv_halo_x3_kernel<rate 2>", "3": "conv_halo_x3_kernel<row-parity>"}[args[0]]
    if base == "convt_halo_x3_kernel":
        return base if coord else "convt_halo_x3_kernel(wrap, ragged)"
    if base == "conv_igemm_kernel":
        return "conv_igemm_kernel<bf16>" if args[3] == "1" else "conv_igemm_kernel<f32, mode %s>" % args[2]
    return base


def klass(nsplit, num_cus):
    return "whole" if nsplit == 0 else ("rem" if nsplit < num_cus else "both")


SPLIT_FAMILIES = (
    "conv_halo_x3_kernel<rate 1>", "conv_halo_x3_kernel<rate 2>", "conv_halo_x3_kernel<row-parity>", "conv_halo_x3_kernel<fp16>",
    "conv_halo8_x3_kernel", "conv_halo_s2_x3_kernel", "conv_halo8_s2_x3_kernel", "convt_halo_x3_kernel",
    "convt_halo_x3_kernel(wrap, ragged)", "convt_halo8_x3_kernel", "conv_halo_kernel", "conv_halo_s2_kernel", "convt_halo_kernel",
    "conv_igemm_kernel<f32, mode 0>", "conv_igemm_kernel<f32, mode 1>", "conv_igemm_kernel<bf16>",
)
BF16_HALO_FAMILIES = ("conv_halo_bf16_kernel", "conv_halo_bf16_s2_kernel", "convt_halo_bf16_kernel")

# (family, class) the planner can never produce: (line of matryodshka_amd/csrc/cnn_plan.hip, text on that line, why)
UNREACHABLE = {
    ("conv_halo_s2_kernel", "both"): (137, ">= 3L * pl->num_cus", "without the six-product form the stride-2 halo kernel is only chosen for "
                                      "grids of at least 3 tiles per CU; split0 = 2 needs fewer than 2"),
    ("conv_halo_bf16_kernel", "rem"): (156, "max_split = 1", "bf16 halo tiles are never cut into K-ranges"),
    ("conv_halo_bf16_kernel", "both"): (156, "max_split = 1", "bf16 halo tiles are never cut into K-ranges"),
    ("conv_halo_bf16_s2_kernel", "rem"): (162, "max_split = 1", "bf16 halo tiles are never cut into K-ranges"),
    ("conv_halo_bf16_s2_kernel", "both"): (162, "max_split = 1", "bf16 halo tiles are never cut into K-ranges"),
    ("convt_halo_bf16_kernel", "rem"): (191, "max_split = 1", "bf16 halo tiles are never cut into K-ranges"),
    ("convt_halo_bf16_kernel", "both"): (191, "max_split = 1", "bf16 halo tiles are never cut into K-ranges"),
}

# (family, class) -> the DECOMP_CASES that reach it (test_coverage_table_is_what_the_plans_give recomputes this)
COVERAGE = {
    ("conv_halo_x3_kernel<rate 1>", "whole"): ["A-cus13", "C-cus304"],
    ("conv_halo_x3_kernel<rate 1>", "rem"): ["A-cus12", "A-cus13", "A-cus20", "A-cus24", "B-cus9", "C-cus304"],
    ("conv_halo_x3_kernel<rate 1>", "both"): ["A-cus20", "A-cus24"],
    ("conv_halo_x3_kernel<rate 2>", "whole"): ["B-tile8-cus13"],
    ("conv_halo_x3_kernel<rate 2>", "rem"): ["E-tile8-cus11"],
    ("conv_halo_x3_kernel<rate 2>", "both"): ["B-cus9"],
    ("conv_halo_x3_kernel<row-parity>", "whole"): ["A-tile8-cus39", "C-cus304"],
    ("conv_halo_x3_kernel<row-parity>", "rem"): ["A-cus20", "A-cus24"],
    ("conv_halo_x3_kernel<row-parity>", "both"): ["A-cus12", "A-cus13", "A-tile8-cus13"],
    ("conv_halo_x3_kernel<fp16>", "whole"): ["E-f16-cus9", "E-f16-cus19"],
    ("conv_halo_x3_kernel<fp16>", "rem"): ["E-f16-cus9", "E-f16-cus19"],
    ("conv_halo_x3_kernel<fp16>", "both"): ["E-f16-cus9", "E-f16-cus19"],
    ("conv_halo8_x3_kernel", "whole"): ["A-cus13", "B-cus9", "A-tile8-cus13", "A-tile8-cus39", "B-tile8-cus13", "E-tile8-cus11"],
    ("conv_halo8_x3_kernel", "rem"): ["A-cus12", "A-cus20", "B-cus9", "A-tile8-cus13", "A-tile8-cus39", "B-tile8-cus13", "E-tile8-cus11"],
    ("conv_halo8_x3_kernel", "both"): ["A-tile8-cus13", "E-tile8-cus11"],
    ("conv_halo_s2_x3_kernel", "whole"): ["A-cus13", "A-cus24", "B-cus9", "B-tile8-cus13", "E-f16-cus9", "E-f16-cus19", "C-cus304"],
    ("conv_halo_s2_x3_kernel", "rem"): ["A-cus12", "A-cus13", "A-cus20", "A-cus24", "E-tile8-cus11"],
    ("conv_halo_s2_x3_kernel", "both"): ["A-cus12", "A-cus13", "A-cus20", "A-cus24", "B-cus9"],
    ("conv_halo8_s2_x3_kernel", "whole"): ["A-tile8-cus39", "B-tile8-cus13"],
    ("conv_halo8_s2_x3_kernel", "rem"): ["A-tile8-cus13", "E-tile8-cus11"],
    ("conv_halo8_s2_x3_kernel", "both"): ["A-tile8-cus13"],
    ("convt_halo_x3_kernel", "whole"): ["A-cus13", "B-tile8-cus13"],
    ("convt_halo_x3_kernel", "rem"): ["A-cus12", "A-cus13", "A-cus20", "A-cus24", "B-cus9"],
    ("convt_halo_x3_kernel", "both"): ["A-cus12", "A-cus13", "A-cus20", "A-cus24", "B-cus9", "A-tile8-cus13", "A-tile8-cus39"],
    ("convt_halo_x3_kernel(wrap, ragged)", "whole"): ["E-tile8-cus11", "E-f16-cus9", "E-f16-cus19", "C-cus304"],
    ("convt_halo_x3_kernel(wrap, ragged)", "rem"): ["E-tile8-cus11", "E-f16-cus9", "E-f16-cus19", "C-cus304"],
    ("convt_halo_x3_kernel(wrap, ragged)", "both"): ["E-f16-cus19"],
    ("convt_halo8_x3_kernel", "whole"): ["A-tile8-cus39", "B-tile8-cus13"],
    ("convt_halo8_x3_kernel", "rem"): ["B-cus9", "A-tile8-cus13", "B-tile8-cus13"],
    ("convt_halo8_x3_kernel", "both"): ["A-tile8-cus13"],
    ("conv_halo_kernel", "whole"): ["A-native-cus11", "E-native-cus19"],
    ("conv_halo_kernel", "rem"): ["A-native-cus9", "A-native-cus11", "E-native-cus19", "C-native-cus37"],
    ("conv_halo_kernel", "both"): ["A-native-cus9", "A-native-cus11", "E-native-cus19", "C-native-cus37"],
    ("conv_halo_s2_kernel", "whole"): ["A-native-cus11"],
    ("conv_halo_s2_kernel", "rem"): ["A-native-cus9", "C-native-cus37"],
    ("convt_halo_kernel", "whole"): ["A-native-cus11"],
    ("convt_halo_kernel", "rem"): ["A-native-cus9", "A-native-cus11"],
    ("convt_halo_kernel", "both"): ["A-native-cus9", "A-native-cus11"],
    ("conv_igemm_kernel<f32, mode 0>", "whole"): ["A-native-cus11", "E-native-cus19"],
    ("conv_igemm_kernel<f32, mode 0>", "rem"): ["E-native-cus19", "C-native-cus37"],
    ("conv_igemm_kernel<f32, mode 0>", "both"): ["A-native-cus9", "A-native-cus11", "C-native-cus37"],
    ("conv_igemm_kernel<f32, mode 1>", "whole"): ["E-native-cus19", "C-native-cus37"],
    ("conv_igemm_kernel<f32, mode 1>", "rem"): ["E-native-cus19", "C-native-cus37"],
    ("conv_igemm_kernel<f32, mode 1>", "both"): ["E-native-cus19"],
    ("conv_igemm_kernel<bf16>", "whole"): ["D-bf16-cus9", "D-bf16-cus12", "D-bf16-cus19", "D-bf16-cus35"],
    ("conv_igemm_kernel<bf16>", "rem"): ["D-bf16-cus9", "D-bf16-cus12", "D-bf16-cus19", "D-bf16-cus35"],
    ("conv_igemm_kernel<bf16>", "both"): ["D-bf16-cus9", "D-bf16-cus12", "D-bf16-cus35"],
}


def _native():
    from matryodshka_amd import build
    build.build(verbose=False)
    from matryodshka_amd import _native as N, nets
    return N, nets


def _options(N, named):
    return {getattr(N, "NET_OPT_" + k): v for k, v in named.items()}


def plan_for(case, extra=None):
    """A host-side plan of `case` (NUM_CUS first, then its options, then `extra`: {name: value})."""
    N, nets = _native()
    b, h, w, cin, nout, ngf = case["shape"]
    plan = N.NetPlan(nets.make_desc(b, h, w, cin, nout, ngf, case["coord"], case["dtype"]))
    plan.set_option(N.NET_OPT_NUM_CUS, case["num_cus"])
    for k, v in list(case["options"].items()) + list((extra or {}).items()):
        plan.set_option(getattr(N, "NET_OPT_" + k), v)
    return plan


def decomposition(plan, coord, num_cus):
    """[(family, class, kernel, workgroups, tiles cut)] of the 17 conv layers of `plan`."""
    out = []
    for li in range(17):
        kernel, nblocks, nsplit = plan.layer_kernel(li)
        out.append((family(kernel, coord), klass(nsplit, num_cus), kernel, nblocks, nsplit))
    return out


def pairs_of(case, plan=None):
    """The (family, class) pairs of the families under test that `case` reaches."""
    plan = plan or plan_for(case)
    return sorted({(f, c) for f, c, _, _, _ in decomposition(plan, case["coord"], case["num_cus"]) if f in SPLIT_FAMILIES})


def test_coverage_table_is_what_the_plans_give():
    got = {}
    for case in DECOMP_CASES:
        for pair in pairs_of(case):
            got.setdefault(pair, []).append(case["id"])
    assert got == COVERAGE, "\n".join("    %r: %r," % kv for kv in sorted(got.items()))


def test_every_family_is_covered_in_every_reachable_class():
    missing = [(f, c) for f in SPLIT_FAMILIES for c in CLASSES if (f, c) not in COVERAGE and (f, c) not in UNREACHABLE]
    assert not missing, missing
    assert not set(COVERAGE) & set(UNREACHABLE)
    for f in BF16_HALO_FAMILIES:
        assert (f, "rem") in UNREACHABLE and (f, "both") in UNREACHABLE
    # at least two cases per family run its split forms at an odd CU count (n_main % 8 != 0 in the XCD interleave)
    for f in SPLIT_FAMILIES:
        odd = {cid for c in ("rem", "both") for cid in COVERAGE.get((f, c), []) if CASE_BY_ID[cid]["num_cus"] % 2}
        assert len(odd) >= 2, (f, sorted(odd))


def changed_layers(case, extra):
    """[(layer, workgroups by default, workgroups with `extra`, tiles cut by default, tiles cut with `extra`)] where they differ."""
    d0 = decomposition(plan_for(case), case["coord"], case["num_cus"])
    d1 = decomposition(plan_for(case, extra), case["coord"], case["num_cus"])
    return [(li, d0[li][3], d1[li][3], d0[li][4], d1[li][4]) for li in range(17) if d0[li][3] != d1[li][3]]


@pytest.mark.parametrize("case,extra", OPTION_CASES, ids=[c["id"] + "-" + "-".join("%s%d" % kv for kv in e.items()) for c, e in OPTION_CASES])
def test_split_options_change_the_decomposition(case, extra):
    changed = changed_layers(case, extra)
    assert changed, (case["id"], extra)
    cus = case["num_cus"]
    if extra.get("TAILSPLIT") == 2:        # the residency-aware form: more tiles cut than one CU group holds, on some layer
        assert any(n1 > n0 and n1 >= cus for _, _, _, n0, n1 in changed), changed
    if "UNIFORM_SPLIT" in extra:           # every tile of a layer with NUM_CUS <= tiles < 2 NUM_CUS in s K-ranges
        s_ = extra["UNIFORM_SPLIT"]
        assert any(cus <= n1 < 2 * cus and b1 == s_ * n1 for _, _, b1, _, n1 in changed), changed


def test_back_to_back_cases_split_every_x3_family_they_run():
    for cid in BACK_TO_BACK_CASES:
        case = CASE_BY_ID[cid]
        fams = {f for f, c in pairs_of(case) if "x3" in f}
        split = {f for f, c in pairs_of(case) if "x3" in f and c != "whole"}
        assert fams == split and len(split) >= 5, (cid, sorted(fams - split))
    assert any(CASE_BY_ID[cid]["num_cus"] % 2 for cid in BACK_TO_BACK_CASES)


def test_unreachable_pairs_cite_the_line_that_says_so():
    lines = open(os.path.join(ROOT, "matryodshka_amd", "csrc", "cnn_plan.hip")).read().split("\n")
    for pair, (line, text, _) in UNREACHABLE.items():      # (within a few lines: an edit above them must not fail this)
        assert any(text in ln for ln in lines[max(0, line - 13):line + 12]), (pair, line, lines[line - 1])


# ---- robustness: every CU count under the options that move the decomposition
CONFIG_DESCS = [
    ("configs[1]", "f32", (1, 320, 640, 192, 64, 64), True),
    ("configs[1] wrap", "f32", (1, 320, 640, 192, 64, 64), False),
    ("configs[2]", "bf16", (16, 320, 640, 384, 128, 64), True),
    ("configs[3]", "f32", (32, 640, 1280, 192, 64, 64), True),
    ("configs[4]", "f32", (64, 256, 256, 192, 64, 64), True),
]
SWEEP_DESCS = CONFIG_DESCS + sorted({("case shape", c["dtype"], c["shape"], c["coord"]) for c in DECOMP_CASES})
SWEEP_OPTIONS = [{}, {"X3_TILE8": FORCE8}, {"TAILSPLIT": 0}, {"TAILSPLIT": 2}, {"UNIFORM_SPLIT": 2}, {"UNIFORM_SPLIT": 3},
                 {"UNIFORM_SPLIT": 4}, {"SPLIT_OVERHEAD": 4}, {"HALO": 0}, {"HALO": 7}, NATIVE]
MAX_SPLIT = 8                      # cnn_device.h: K-ranges per tile at most; the slab region holds 2 NUM_CUS MAX_SPLIT slabs of 64 x 64 floats
SWEEP_CUS = list(range(8, 321)) + [512, 4096]


def _tile_of(kernel):
    """What decides a layer's tile count: the kernel family (conv_igemm_kernel: its BM, BN template arguments too)."""
    return kernel if kernel.startswith("conv_igemm_kernel") else kernel.split("<")[0]


def _device_default_cus():
    import torch
    if torch.cuda.is_available():
        return torch.cuda.get_device_properties(torch.cuda.current_device()).multi_processor_count
    return 256                     # cnn_device.h: DEFAULT_CUS, what a plan takes where there is no device


@pytest.mark.parametrize("what,dtype,shape,coord", SWEEP_DESCS,
                         ids=["%s-%s-%s-%s" % (d[0].replace(" ", "_"), d[1], "x".join(map(str, d[2])), "coord" if d[3] else "wrap") for d in SWEEP_DESCS])
def test_no_cu_count_breaks_a_plan(what, dtype, shape, coord):
    N, nets = _native()
    b, h, w, cin, nout, ngf = shape
    default_cus = _device_default_cus()
    seen = set()
    for named in SWEEP_OPTIONS:
        plan = N.NetPlan(nets.make_desc(b, h, w, cin, nout, ngf, coord, dtype), _options(N, named))
        original = plan.kernels()
        whole = N.NetPlan(nets.make_desc(b, h, w, cin, nout, ngf, coord, dtype), _options(N, dict(named, TAILSPLIT=0)))   # the same plan in whole tiles
        for cus in SWEEP_CUS:
            rc = N.lib.msi_net_plan_set_option(plan.handle, N.NET_OPT_NUM_CUS, cus)
            assert rc == 0, (what, named, cus, N.last_error())
            whole.set_option(N.NET_OPT_NUM_CUS, cus)
            for li in range(17):
                kernel, nblocks, nsplit = plan.layer_kernel(li)
                # what the slab region is really sized for, under every option: the K-range workgroups of a launch (all workgroups
                # but the whole tiles; the tile count is the whole-tile plan's workgroup count where it takes the same tile),
                # one slab each -- two for the conv-transpose halo kernels -- of the kernel's tile, in 2 NUM_CUS MAX_SPLIT slabs of 64 x 64
                kernel_w, ntiles, nsplit_w = whole.layer_kernel(li)
                assert nsplit_w == 0
                if _tile_of(kernel_w) == _tile_of(kernel):
                    kranges = nblocks - (ntiles - nsplit)
                    assert (kranges == 0) == (nsplit == 0) and 2 * nsplit <= kranges <= MAX_SPLIT * nsplit, (what, named, cus, li, kernel)
                    slabs = kranges * (2 if kernel.startswith("convt_halo") else 1) * (2 if "halo8" in kernel else 1)
                    assert slabs <= 2 * cus * MAX_SPLIT, (what, named, cus, li, kernel, nblocks, nsplit, ntiles)
                else:               # (a conv-transpose halo tile whose two slabs per K-range did not fit fell back: 4-row tile, or the tap kernel)
                    assert kernel_w.startswith("convt_halo"), (what, named, cus, li, kernel, kernel_w)
                # the slab workspace is sized for the K-ranges of fewer than 2 NUM_CUS tiles (cnn_net.hip: net.partial_bytes).
                # TAILSPLIT = 2 (the residency-aware form, not the default) cuts the tiles beyond a multiple of Q = 5 NUM_CUS
                # instead: up to Q - 1 of them, in as many K-ranges as the same slabs hold (plan_tiles: `remq * sp > 2L *
                # num_cus * MAX_SPLIT`; its own example is 3 200 tiles on 256 CUs = 2 560 whole + 640 x 2) -- there the
                # bounds are Q, which is also what the arrival tickets are sized for, and the planner's slab check, whose
                # failure would be the MSI_E_WORKSPACE refused above
                bound = 5 * cus if named.get("TAILSPLIT") == 2 else 2 * cus
                assert 0 <= nsplit < bound and nblocks >= 1, (what, named, cus, li, kernel, nblocks, nsplit)
                seen.add((family(kernel, coord), klass(nsplit, cus)))
            assert plan.workspace_bytes() > 0
        plan.set_option(N.NET_OPT_NUM_CUS, default_cus)
        assert plan.kernels() == original, (what, named)
    assert not seen & set(UNREACHABLE), sorted(seen & set(UNREACHABLE))


# ---- the plans themselves: digests recorded from the planner as it was before choose_variant (tools/plan_golden.py --record on that commit)
@pytest.mark.parametrize("what,dtype,shape,coord", SWEEP_DESCS,
                         ids=["%s-%s-%s-%s" % (d[0].replace(" ", "_"), d[1], "x".join(map(str, d[2])), "coord" if d[3] else "wrap") for d in SWEEP_DESCS])
def test_sweep_plans_are_the_recorded_ones(what, dtype, shape, coord):
    golden = plan_golden.golden()
    for named in SWEEP_OPTIONS:
        assert plan_golden.sweep_digest(dtype, shape, coord, named, SWEEP_CUS) == golden[plan_golden.sweep_key(dtype, shape, coord, named)], (what, named)


def test_case_plans_are_the_recorded_ones():
    golden = plan_golden.golden()
    for case, extra in [(c, None) for c in DECOMP_CASES] + list(OPTION_CASES) + [(c, None) for c, _ in OPTION_CASES]:
        assert plan_golden.plan_digest(plan_for(case, extra)) == golden[plan_golden.case_key(case, extra)], (case["id"], extra)
    # nothing recorded that no test recomputes (the weight digests: tests/test_native_abi.py)
    keys = {plan_golden.sweep_key(d[1], d[2], d[3], named) for d in SWEEP_DESCS for named in SWEEP_OPTIONS}
    keys |= {plan_golden.case_key(c, e) for c, e in [(c, None) for c in DECOMP_CASES] + list(OPTION_CASES) + [(c, None) for c, _ in OPTION_CASES]}
    assert set(golden) == keys | {"weights|" + w for w in plan_golden.WEIGHT_DESCS}
