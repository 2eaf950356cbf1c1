"""Exact operand families for conv1_1 of the fp32 tier, WITHOUT a GPU: the construction, its proof obligations, and that it has teeth.

conv1_1 reads the network input, so both of its operands can be chosen.  They are chosen so that every product and every partial sum, in ANY order, is exactly
representable in fp32: the raw output of conv1_1 must then equal the fp64 convolution bit for bit -- whatever the tile shape, the K-range hand-off, the fix-up launch
or the MFMA summation order (tests/test_gpu_x3_exact.py runs that on the device).  One lost term, tap or chunk is a mismatch there, not a 2e-6 blur.

Construction.  A value is 0 or +-(a + b 2^-9 + c 2^-18), a in {1, 2}, b, c in {0, 1}, c <= b: its bf16 parts (oracle/nets.py split3) are exactly h = +-a, m = +-b 2^-9,
l = +-c 2^-18 (with b = 0 a lone 2^-18 would be the m part: hence c <= b).  Three families whose DROPPED terms (m.l, l.m, l.l) vanish identically:
    "hm_hm":  activations h+m   x weights h+m      exercises m.m, h.m, m.h
    "hml_h":  activations h+m+l x weights h        exercises l.h (and m.h)
    "h_hml":  activations h     x weights h+m+l    exercises h.l (and h.m)
and for the fp16 three-product form a + b 2^-12 (fp16 parts h = +-a, m' = +-b / 2): "f16_hm_h" (exercises m'.h) and "f16_h_hm" (h.m').
Every product is a multiple of 2^-18 (2^-12), so is every partial sum, and with  max over outputs of sum |x| |w| <= 2^6  each needs at most 24 bits: exact.
Non-zeros (about 8 % of both operands) are also put, on purpose, in the two border columns on each side, the first and last row, and the first and last channel of
every 32-channel chunk.  The coordinate-channel weights of conv1_1 are zero (CoordNet), so the kernels' tabulated coordinate bias is exactly 0."""
import numpy as np
import pytest
import torch
import torch.nn.functional as TF

from tests.test_plan_decomposition import ALL, FORCE8, _case, plan_for

SHAPE = (1, 32, 64, 96, 8, 32)        # conv1_1: 96 -> 32 channels at 32 x 64 (4-row tiles: 8 x 4, three 32-channel chunks x 9 taps)
SHAPE_B2 = (2,) + SHAPE[1:]
BOUND = 64.0                          # 2^6: with a granularity of 2^-18, 24 bits
X3_FAMILIES = ("hm_hm", "hml_h", "h_hml")
F16_FAMILIES = ("f16_hm_h", "f16_h_hm")
# terms a family exercises beyond h.h (activation part . weight part), as the keys of terms()
EXERCISED = {"hm_hm": ("mm", "hm", "mh"), "hml_h": ("lh", "mh"), "h_hml": ("hl", "hm"), "f16_hm_h": ("mh",), "f16_h_hm": ("hm",)}
DENSITY = 0.08

# the plans tests/test_gpu_x3_exact.py runs: (case, extra options, conv1_1's kernel, conv1_1 cut into K-ranges?, families)
W3, T8, F16K = "conv_halo_x3_kernel<1, 0, 3>", "conv_halo8_x3_kernel<0, 3>", "conv_halo_x3_kernel<1, 0, 2>"
EXACT_PLANS = [
    (_case("whole", "f32", SHAPE, True, 256), None, W3, False, X3_FAMILIES),
    (_case("cus9", "f32", SHAPE, True, 9), None, W3, True, X3_FAMILIES),
    (_case("cus13", "f32", SHAPE, True, 13), None, W3, True, X3_FAMILIES),
    (_case("cus13-fixup", "f32", SHAPE, True, 13), {"FIXUP_KERNEL": 1}, W3, True, X3_FAMILIES),
    (_case("tile8", "f32", SHAPE, True, 256, {"X3_TILE8": FORCE8}), None, T8, False, X3_FAMILIES),
    (_case("tile8-cus13", "f32", SHAPE, True, 13, {"X3_TILE8": FORCE8}), None, T8, True, X3_FAMILIES),
    (_case("f16", "f32", SHAPE, True, 256, {"F32_SPLIT_F16": ALL}), None, F16K, False, F16_FAMILIES),
    (_case("f16-cus9", "f32", SHAPE, True, 9, {"F32_SPLIT_F16": ALL}), None, F16K, True, F16_FAMILIES),
    (_case("wrap", "f32", SHAPE, False, 256), None, W3, False, X3_FAMILIES),
    (_case("wrap-cus13", "f32", SHAPE, False, 13), None, W3, True, X3_FAMILIES),
    (_case("batch2-cus9", "f32", SHAPE_B2, True, 9, {"X3_TILE8": 0}), None, W3, True, X3_FAMILIES),
]
EXACT_IDS = [(p[0]["id"], fam) for p in EXACT_PLANS for fam in p[4]]
PLAN_BY_ID = {p[0]["id"]: p for p in EXACT_PLANS}


def _values(rng, mask, parts):
    """+-(a + b g1 + c g2) on `mask`, 0 elsewhere; parts: "h" | "hm" | "hml" | "f16_h" | "f16_hm"."""
    a = rng.randint(1, 3, size=mask.shape).astype(np.float64)
    b = rng.randint(0, 2, size=mask.shape).astype(np.float64)
    c = rng.randint(0, 2, size=mask.shape).astype(np.float64) * b          # c <= b
    sign = rng.randint(0, 2, size=mask.shape) * 2.0 - 1.0
    v = {"h": a, "hm": a + b * 2.0 ** -9, "hml": a + b * 2.0 ** -9 + c * 2.0 ** -18, "f16_h": a, "f16_hm": a + b * 2.0 ** -12}[parts]
    out = (sign * v * mask).astype(np.float32)
    assert np.array_equal(out.astype(np.float64), sign * v * mask)          # (every value is an fp32 number)
    return out


def make_operands(family, shape=SHAPE, seed=0):
    """(x [B,H,W,Cin], w [3,3,Cin,Cout]) fp32 of `family`: ~8 % non-zeros each, plus the deliberate ones at the patch's and the chunks' edges."""
    b, h, w, cin, _, ngf = shape
    rng = np.random.RandomState(1000 + seed)
    xp, wp = {"hm_hm": ("hm", "hm"), "hml_h": ("hml", "h"), "h_hml": ("h", "hml"), "f16_hm_h": ("f16_hm", "f16_h"), "f16_h_hm": ("f16_h", "f16_hm")}[family]
    edge_ch = sorted({c for c0 in range(0, cin, 32) for c in (c0, min(c0 + 31, cin - 1))})
    mx = rng.uniform(size=(b, h, w, cin)) < DENSITY                          # (another pattern per sample)
    for i, ch in enumerate(edge_ch):                                         # border columns: every other row; first / last row: every third column
        mx[:, (i % 2)::2, [0, 1, w - 2, w - 1], ch] = True
        mx[:, [0, h - 1], (i % 3)::3, ch] = True
    mw = rng.uniform(size=(3, 3, cin, ngf)) < DENSITY
    for i, ch in enumerate(edge_ch):                                         # every tap of a chunk's first / last channel, for a sixth of the output channels
        mw[:, :, ch, i::len(edge_ch)] = True
    return _values(rng, mx, xp), _values(rng, mw, wp)


def conv11(x, w, coord, products=None):
    """conv1_1's raw output [B,H,W,Cout] of x [B,H,W,Cin], w [3,3,Cin,Cout] (the coordinate channel's weights being zero): products None = the fp64 convolution
    (float64 array), else products(fn, x, w) with fn an fp32 convolution (oracle/nets.py conv_split3 / conv_split_f16 or a variant of them)."""
    from oracle import nets as onets
    dt = torch.float64 if products is None else torch.float32
    xt = torch.from_numpy(np.ascontiguousarray(np.transpose(x, (0, 3, 1, 2)))).to(dt)
    wt = onets._conv_w(w).to(dt)
    xt = TF.pad(xt, (1, 1, 1, 1)) if coord else onets.wrap_pad(xt, 1, 1)
    y = TF.conv2d(xt, wt) if products is None else products(lambda a, b_: TF.conv2d(a, b_), xt, wt)
    return np.ascontiguousarray(y.permute(0, 2, 3, 1).numpy())


def abs_bound(x, w, coord):
    """max over outputs of sum |x| |w|."""
    return float(conv11(np.abs(x), np.abs(w), coord).max())


def terms(form, drop=None):
    """The product form `form` ("x3" | "f16") with term `drop` (activation part . weight part: "mm", "hm", "mh", "hl", "lh") left out."""
    from oracle import nets as onets

    def products(fn, x, w):
        if form == "f16":
            (xh, xm), (wh, wm) = onets.split_f16(x), onets.split_f16(w)
            t = {"mh": fn(xm, wh), "hm": fn(xh, wm)}
            t = {k: (torch.zeros_like(v) if k == drop else v) for k, v in t.items()}
            return fn(xh, wh) + (t["mh"] + t["hm"]) * (1.0 / 2048.0)
        (xh, xm, xl), (wh, wm, wl) = onets.split3(x), onets.split3(w)
        t = {"mm": fn(xm, wm), "lh": fn(xl, wh), "hl": fn(xh, wl), "mh": fn(xm, wh), "hm": fn(xh, wm)}
        t = {k: (torch.zeros_like(v) if k == drop else v) for k, v in t.items()}
        return ((t["mm"] + t["lh"]) + t["hl"]) + ((t["mh"] + t["hm"]) + fn(xh, wh))
    return products


def form_of(family):
    return "f16" if family.startswith("f16") else "x3"


def exact_case(family, shape, coord, seed=0):
    """(x, w, the fp64 convolution as fp32) of a case the GPU half may use: the exactness condition and fp32 representability are ASSERTED here."""
    x, w = make_operands(family, shape, seed)
    bound = abs_bound(x, w, coord)
    assert bound <= BOUND, (family, shape, coord, bound)
    ref = conv11(x, w, coord)
    assert np.array_equal(ref.astype(np.float32).astype(np.float64), ref), family
    return x, w, ref.astype(np.float32)


@pytest.mark.parametrize("family", X3_FAMILIES + F16_FAMILIES)
def test_the_parts_are_the_intended_ones_and_the_dropped_terms_vanish(family):
    from oracle import nets as onets
    x, w = make_operands(family)
    xt, wt = torch.from_numpy(x), torch.from_numpy(w)
    if form_of(family) == "f16":
        for t, has_m in ((xt, family == "f16_hm_h"), (wt, family == "f16_h_hm")):
            h, m = onets.split_f16(t)
            assert set(np.unique(np.abs(h.numpy()))) == {0.0, 1.0, 2.0}
            assert set(np.unique(np.abs(m.numpy()))) == ({0.0, 0.5} if has_m else {0.0})
            assert torch.equal(h + m / 2048.0, t)
        return
    parts = {"hm_hm": ("hm", "hm"), "hml_h": ("hml", "h"), "h_hml": ("h", "hml")}[family]
    for t, p in zip((xt, wt), parts):
        h, m, l_ = onets.split3(t)
        assert set(np.unique(np.abs(h.numpy()))) == {0.0, 1.0, 2.0}
        assert set(np.unique(np.abs(m.numpy()))) == ({0.0, 2.0 ** -9} if "m" in p else {0.0})
        assert set(np.unique(np.abs(l_.numpy()))) == ({0.0, 2.0 ** -18} if "l" in p else {0.0})
        assert torch.equal((h + m) + l_, t)
    # m.l, l.m, l.l: one operand of each is identically zero
    (_, xm, xl), (_, wm, wl) = onets.split3(xt), onets.split3(wt)
    for a, b_ in ((xm, wl), (xl, wm), (xl, wl)):
        assert not a.any() or not b_.any()


@pytest.mark.parametrize("coord", [True, False], ids=["coord", "wrap"])
@pytest.mark.parametrize("family", X3_FAMILIES + F16_FAMILIES)
def test_exactness_bound_fp32_representability_and_the_emulations_reproduce_fp64_bit_for_bit(family, coord):
    x, w, ref = exact_case(family, SHAPE_B2, coord)
    bound = abs_bound(x, w, coord)
    gran = 2.0 ** -12 if form_of(family) == "f16" else 2.0 ** -18
    low = float((np.abs(ref.astype(np.float64)) / gran % 2 == 1).mean())
    print("%s %s: max sum |x| |w| = %.1f (bound %g), %.0f %% of the outputs carry the 2^%d bit, %.1f %% / %.1f %% non-zeros"
          % (family, "coord" if coord else "wrap", bound, BOUND, 100 * low, int(np.log2(gran)), 100 * (x != 0).mean(), 100 * (w != 0).mean()))
    assert low > 0.25                                          # the lowest bit is really in use
    assert np.array_equal(conv11(x, w, coord, terms(form_of(family))), ref)
    # ... by the oracle's own functions too
    from oracle import nets as onets
    assert np.array_equal(conv11(x, w, coord, onets.conv_split_f16 if form_of(family) == "f16" else onets.conv_split3), ref)
    # the two samples have different patterns
    assert not np.array_equal(x[0] != 0, x[1] != 0)
    # the deliberate non-zeros: border columns, first / last row, first / last channel of every chunk (activations), every tap of those channels (weights)
    for ch in (0, 31, 32, 63, 64, 95):
        assert all((x[:, :, col, ch] != 0).any() for col in (0, 1, x.shape[2] - 2, x.shape[2] - 1)) and all((x[:, row, :, ch] != 0).any() for row in (0, x.shape[1] - 1))
        assert (w[:, :, ch, :] != 0).any(axis=-1).all()


@pytest.mark.parametrize("family", X3_FAMILIES + F16_FAMILIES)
def test_dropping_any_exercised_term_changes_thousands_of_outputs(family):
    x, w, ref = exact_case(family, SHAPE, True)
    for drop in EXERCISED[family]:
        got = conv11(x, w, True, terms(form_of(family), drop))
        changed = int((got != ref).sum())
        print("%s without %s: %d of %d outputs change" % (family, drop, changed, ref.size))
        assert changed >= 4000, (family, drop, changed)
    # one tap of one chunk lost, one 4 x 16 tile only: a mismatch as well
    wt = w.copy()
    wt[0, 2, 32:64, :] = 0
    lost = conv11(x, wt, True, terms(form_of(family)))[:, :4, :16] != ref[:, :4, :16]
    assert lost.sum() >= 100, (family, int(lost.sum()))


def test_the_plans_take_the_kernels_under_test_and_keep_conv1_1_raw():
    from matryodshka_amd import _native as N
    for case, extra, kernel, split, _ in EXACT_PLANS:
        plan = plan_for(case, extra)
        name, nblocks, nsplit = plan.layer_kernel(0)
        assert name == kernel, (case["id"], name)
        assert (nsplit > 0) == split, (case["id"], nblocks, nsplit)
        assert N.lib.msi_net_plan_layer_is_normalized(plan.handle, 0) == 0, case["id"]       # the buffer holds conv1_1's raw output
