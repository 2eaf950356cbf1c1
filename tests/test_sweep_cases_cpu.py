"""The case table of tests/sweep_cases.py means what it claims (no device): its launches reach every form sweep_common can take, its LDS cases stage patches
(and so do the older LDS tests' parametrizations), the samples a case is there for exist in the oracle's positions, the device test's own comparisons fail on
stand-ins with the faults they are there for, and a correct kernel's freedom (the documented 2.6e-7 rad of t_angles) stays within a third of every gate.
Run with -s for the figures recorded in profiles/sweep_forms.txt."""
import numpy as np
import pytest

from oracle import geometry as G
from tests import sweep_cases as SC

F = np.float32
IDS = [c["name"] for c in SC.CASES]
_volumes = {}


def _inputs_and_volume(case):
    """(case_inputs, the oracle's double volume), computed once per case and never changed."""
    if case["name"] not in _volumes:
        inp = SC.case_inputs(case)
        vol = SC.oracle_volume(inp)
        vol.setflags(write=False)
        _volumes[case["name"]] = (inp, vol)
    return _volumes[case["name"]]


# 1 ---------------------------------------------------------------------------------------------------------------------
def test_the_table_reaches_every_form():
    reached = set()
    for case in SC.CASES:
        forms = SC.case_forms(case)
        print("%-14s %s" % (case["name"], "  ".join(_fmt(f) for f in sorted(forms, key=str))))
        reached |= forms
    for name in SC.WINDOW_CASES:
        c = SC.case_by_name(name)
        reached |= {SC.sweep_form(c["b"], c["h"], c["w"], c["d"], False, bf16) for bf16 in (False, True)}
    print("%d of %d forms" % (len(reached & SC.ALL_FORMS), len(SC.ALL_FORMS)))
    assert reached == SC.ALL_FORMS, (sorted(SC.ALL_FORMS - reached, key=str), sorted(reached - SC.ALL_FORMS, key=str))
    ns_of = {SC.sweep_form(SC.case_by_name(n)["b"], SC.case_by_name(n)["h"], SC.case_by_name(n)["w"], SC.case_by_name(n)["d"], False, False)[2] for n in SC.WINDOW_CASES}
    assert ns_of == {1, 2}


def _fmt(form):
    return "%s/lds" % form[0] if form[1] == "lds" else "%s/NS%d/NSRC%d/LOOP%d/co%d" % (form[0], form[2], form[3], form[4], form[5])


def test_sweep_form_follows_the_dispatch_at_its_thresholds():
    f = SC.sweep_form
    assert f(2, 16, 64, 16, True, False) == ("f32", "lds") and f(1, 16, 64, 16, True, False) == ("f32", "gather", 2, 2, 0, 1)      # LDS needs a batch
    assert f(2, 16, 64, 16, False, True) == ("bf16", "gather", 2, 1, 1, 0)                                                           # ... and both sources
    assert f(2, 8, 32, 4, True, False) == ("f32", "gather", 2, 2, 1, 1) and f(2, 8, 64, 4, True, False) == ("f32", "gather", 2, 2, 1, 1)   # W * ng = 64, 128: no full blocks
    assert f(2, 8, 128, 4, True, False) == ("f32", "lds")
    assert f(2, 12, 40, 6, True, False)[5] == 0 and f(2, 16, 64, 1, True, True) == ("bf16", "gather", 1, 2, 1, 1) and f(2, 16, 32, 1, True, True)[5] == 0
    assert f(2, 20, 70, 5, True, False) == ("f32", "gather", 1, 2, 1, 0)


# 2 ---------------------------------------------------------------------------------------------------------------------
def _staging_sets():
    """(label, batch, (stages, seam, wrap) [b, h, blocks], equal-to-predecessor [b]) of every LDS case of the table and of the older tests' parametrizations.
    The fuzz slice is one test with one fixed seed: its ten draws are one set."""
    out = []
    for case in SC.CASES:
        if "lds" not in case["claims"]:
            continue
        inp = SC.case_inputs(case)
        out.append(("table %s" % case["name"], "table", SC.staging(case["h"], case["w"], case["d"], inp["pose0"], inp["pose1"], inp["intr"][:, 0, 0], inp["depths"]),
                    [k > 0 and case["frames"][k] == case["frames"][k - 1] for k in range(case["b"])]))
    for h, w, d, b in SC.LDS_GEOMETRY_PARAMS:
        p0, p1, bl, dep = SC.lds_geometry_frames(h, w, d, b)
        out.append(("test_gpu_geometry (%d,%d,%d,%d)" % (h, w, d, b), "geometry", SC.staging(h, w, d, p0, p1, bl, dep), None))
    return out


def test_lds_cases_stage_patches_fall_back_and_cross_the_seam():
    sets = _staging_sets()
    for label, _, (st, seam, wrap), _ in sets:
        share = float(st.mean())
        print("%-36s share of blocks that stage %.3f   fall back %d   staging across the column seam %d   across the row wrap %d   per frame %s" % (
            label, share, int((~st).sum()), int((st & seam).sum()), int((st & wrap).sum()), " ".join("%.2f" % x for x in st.mean(axis=(1, 2)))))
        assert share >= 0.10, (label, share)
        assert (~st).any(), (label, "no block falls back")
        assert (st & seam).any(), (label, "no staging block crosses the column seam")
    # the fuzz slice (one test, one seed): the same three conditions over its ten draws
    n = staged = fallback = seamed = 0
    for h, w, d, b, p0, p1, bl, dep in SC.lds_fuzz_frames():
        assert SC.sweep_form(b, h, w, d, True, False) == ("f32", "lds")
        st, seam, _ = SC.staging(h, w, d, p0, p1, bl, dep)
        print("test_gpu_fuzz (%d,%d,%d,%d) baseline %.3f   share %.3f   fall back %d   staging across the column seam %d" % (
            h, w, d, b, bl[0], st.mean(), int((~st).sum()), int((st & seam).sum())))
        n += st.size; staged += int(st.sum()); fallback += int((~st).sum()); seamed += int((st & seam).sum())
    print("test_gpu_fuzz, the slice: share %.3f   fall back %d   staging across the column seam %d" % (staged / n, fallback, seamed))
    assert staged / n >= 0.10 and fallback >= 1 and seamed >= 1


def test_every_lds_parametrization_takes_the_lds_form():
    for h, w, d, b in SC.LDS_GEOMETRY_PARAMS:
        assert SC.sweep_form(b, h, w, d, True, False) == ("f32", "lds") and SC.sweep_form(b, h, w, d, True, True) == ("bf16", "lds")
    import inspect
    from tests import test_gpu_geometry as T
    mark = [m for m in T.test_lds_staged_sweep_is_bit_identical_to_the_gather_kernel.pytestmark if m.name == "parametrize" and m.args[0] == "h,w,d,b"][0]
    assert list(mark.args[1]) == SC.LDS_GEOMETRY_PARAMS                    # the model restates the test's table: they change together
    src = inspect.getsource(__import__("tests.test_gpu_fuzz", fromlist=["x"]).test_random_sweep_shapes_on_the_lds_staged_kernel_match_oracle_and_the_gather_kernel)
    assert "RandomState(606)" in src and "range(10)" in src


def test_the_table_stages_across_the_row_wrap_after_equal_frames_and_in_second_chunks():
    row_wrap = prefetch = False
    for label, kind, (st, seam, wrap), equal in _staging_sets():
        if kind != "table":
            continue
        row_wrap |= bool((st & wrap).any())
        b = st.shape[0]
        # the next frame's patch is prefetched where it has, bit for bit, its predecessor's setting and sits in the same 16-frame chunk
        prefetch |= any(equal[k] and k % SC.BCHUNK != 0 and st[k].any() for k in range(b))
        if b > SC.BCHUNK:
            best = max(float(st[k].mean()) for k in range(SC.BCHUNK, min(b, 2 * SC.BCHUNK)))
            print("%s: best share of a frame of the second chunk %.2f" % (label, best))
            assert best >= 0.50, (label, best)
    assert row_wrap and prefetch
    # (24,128,8,19) cannot meet the second-chunk condition (0.17 at best); the (24,64,16,19) parametrization next to it does
    h, w, d, b = SC.LDS_GEOMETRY_PARAMS[-1]
    st = SC.staging(h, w, d, *SC.lds_geometry_frames(h, w, d, b))[0]
    assert b > SC.BCHUNK and max(float(st[k].mean()) for k in range(SC.BCHUNK, b)) >= 0.50


def test_chunked_cases_change_and_repeat_at_a_chunk_start():
    chunked = [c for c in SC.CASES if c["b"] > SC.BCHUNK]
    changes = [c["frames"][16] != c["frames"][15] for c in chunked]
    assert any(changes) and not all(changes)
    for lds in (False, True):
        sub = [c for c in chunked if ("lds" in c["claims"]) == lds]
        assert any(c["frames"][16] != c["frames"][15] for c in sub) and any(c["frames"][16] == c["frames"][15] for c in sub), lds
    for c in SC.CASES:
        if c["b"] >= 16:
            kinds = set(c["frames"])
            assert {SC.S0, SC.S1, SC.S2, SC.S3} <= kinds and c["frames"][0] == SC.S0 and SC.S0 in c["frames"][5:], c["name"]       # every change and a return
            assert any(c["frames"][k] == c["frames"][k - 1] for k in range(1, c["b"])), c["name"]


# 3 ---------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("name", IDS)
def test_claimed_samples_exist(name):
    case = SC.case_by_name(name)
    inp = SC.case_inputs(case)
    h, w, d = case["h"], case["w"], case["d"]
    count = dict(seam_x1=0, seam_x0=0, row_m1=0, row_h1=0, invalid=0)
    for k in range(case["b"]):
        for pose, order in ((inp["pose0"][k], 1), (inp["pose1"][k], -1)):
            uv, valid = SC.oracle_uv(h, w, inp["depths"], pose, inp["intr"][k, 0, 0], order)
            x0, y0 = np.floor(uv[..., 0]), np.floor(uv[..., 1])
            count["seam_x1"] += int((x0 == w - 1).sum()); count["seam_x0"] += int((x0 == -1).sum())
            count["row_m1"] += int((y0 == -1).sum()); count["row_h1"] += int((y0 == h - 1).sum()); count["invalid"] += int((~valid).sum())
    print(name, count)
    for claim in count:
        if claim in case["claims"]:
            assert count[claim] > 0, (name, claim, count)
    assert ("odd_d" in case["claims"]) == (d % 2 == 1 and d > 1)
    assert ("baseline" in case["claims"]) == (len({f[2] for f in case["frames"]}) > 1)
    assert ("chunk2" in case["claims"]) == (case["b"] > SC.BCHUNK)
    assert ("lds" in case["claims"]) == (SC.sweep_form(case["b"], h, w, d, True, False)[1] == "lds")


# 4 ---------------------------------------------------------------------------------------------------------------------
def _faulty_resample(fault):
    """oracle.geometry.resample with one fault in its corner indices."""
    def resample(image, pixels):
        image, pixels = np.asarray(image, dtype=F), np.asarray(pixels, dtype=F)
        n, ht, wt, _ = pixels.shape
        _, height, width, ch = image.shape
        x, y = pixels[..., 0].reshape(n, -1), pixels[..., 1].reshape(n, -1)
        x0 = np.floor(x).astype(np.int32); x1 = x0 + 1
        y0 = np.floor(y).astype(np.int32); y1 = y0 + 1
        dx0, dy0, dx1, dy1 = x - x0.astype(F), y - y0.astype(F), x1.astype(F) - x, y1.astype(F) - y
        wx0, wy0, wx1, wy1 = np.mod(x0 + width, width), np.mod(y0 + height, height), np.mod(x1 + width, width), np.mod(y1 + height, height)
        if fault == "x1_clamped":
            wx1 = np.where(x1 == width, width - 1, wx1)
        elif fault == "row_m1_clamped":
            wy0 = np.where(y0 == -1, 0, wy0)
        else:
            raise ValueError(fault)
        b = np.arange(n)[:, None]
        res = (((dy1 * dx1)[..., None] * image[b, wy0, wx0] + (dy1 * dx0)[..., None] * image[b, wy0, wx1]) + (dy0 * dx1)[..., None] * image[b, wy1, wx0]) \
            + (dy0 * dx0)[..., None] * image[b, wy1, wx1]
        return res.reshape(n, ht, wt, ch).astype(F)
    return resample


def _stand_in(fault, case, inp, monkeypatch):
    if fault in ("x1_clamped", "row_m1_clamped"):
        with monkeypatch.context() as mp:
            mp.setattr(G, "resample", _faulty_resample(fault))
            return SC.oracle_volume(inp)
    if fault == "stale_baseline":           # frame k + 1 swept with frame k's baseline: corners kept across a baseline change
        intr = inp["intr"].copy()
        intr[1:, 0, 0] = inp["intr"][:-1, 0, 0]
        return SC.oracle_volume(inp, intr=intr)
    if fault == "source1_order":
        return SC.oracle_volume(inp, order1=1)
    if fault == "last_depth":               # the last sphere of an odd stack taken from its neighbour (a pair kernel on an odd count)
        depths = inp["depths"].copy()
        depths[-1] = depths[-2]
        return SC.oracle_volume(inp, depths=depths)
    raise ValueError(fault)


FAULT_CLAIM = dict(x1_clamped="seam_x1", row_m1_clamped="row_m1", stale_baseline="baseline", source1_order=None, last_depth="odd_d")


@pytest.mark.parametrize("fault", sorted(FAULT_CLAIM))
def test_the_fp32_comparison_sees_the_fault(fault, monkeypatch):
    claim = FAULT_CLAIM[fault]
    cases = [c for c in SC.CASES if claim is None or claim in c["claims"]]
    assert len(cases) >= (2 if claim else len(SC.CASES))
    for case in cases:
        inp, want = _inputs_and_volume(case)
        bad = _stand_in(fault, case, inp, monkeypatch)
        mx, pct = SC.errors_f32(bad, want)
        print("%-16s %-14s max-abs %.3g (gate %.0e)" % (fault, case["name"], mx, SC.TOL))
        with pytest.raises(AssertionError):
            SC.compare_f32(bad, want, case["name"])
    # the patched oracle is the oracle again
    inp, want = _inputs_and_volume(SC.CASES[0])
    assert np.array_equal(SC.oracle_volume(inp), want)


def test_the_fp32_comparison_passes_the_oracle_itself():
    for case in SC.CASES:
        inp, want = _inputs_and_volume(case)
        assert SC.compare_f32(want.copy(), want, case["name"])[0] == 0.0


@pytest.mark.parametrize("name", IDS)
def test_the_bf16_comparison_sees_truncation(name):
    _, want = _inputs_and_volume(SC.case_by_name(name))
    truncated = (np.ascontiguousarray(want).view(np.uint32) >> 16).astype(np.uint16).view(np.int16)
    differ = SC.bf16_bits_differ(truncated, want)
    print(name, "truncated elements that differ from round-to-nearest-even: %d of %d" % (differ, want.size))
    assert differ >= 1
    assert SC.bf16_bits_differ(SC.bf16_bits(want), want) == 0


# 5 ---------------------------------------------------------------------------------------------------------------------
ANGLE_ERROR = 2.6e-7        # rad: the documented error of t_angles (geometry_device.h), the only freedom ods_tail takes from the oracle's op order


class _MovedAngles:
    """numpy for oracle.geometry with arctan2 moved by +-ANGLE_ERROR: project_ods calls it for theta, then for phi, once per frame and source."""

    def __init__(self, sign):
        self._moved_by, self._calls = sign, 0

    def __getattr__(self, name):
        return getattr(np, name)

    def arctan2(self, a, b):
        which = self._calls % 2
        self._calls += 1
        with np.errstate(all="ignore"):
            r = np.arctan2(a, b)
        return (r + (self._moved_by(which, r.shape) * F(ANGLE_ERROR)).astype(F)).astype(F)


def _moved_volume(inp, sign, monkeypatch):
    with monkeypatch.context() as mp:
        mp.setattr(G, "np", _MovedAngles(sign))
        return SC.oracle_volume(inp)


@pytest.mark.parametrize("name", IDS)
def test_a_correct_kernels_freedom_is_a_third_of_each_gate(name, monkeypatch):
    case = SC.case_by_name(name)
    inp, want = _inputs_and_volume(case)
    worst = np.zeros(want.shape, dtype=np.float64)
    for st in (1, -1):                       # the worst of the four uniform sign patterns, per sample
        for sp in (1, -1):
            vol = _moved_volume(inp, lambda which, shape, st=st, sp=sp: F(sp if which else st) * np.ones(shape, dtype=F), monkeypatch)
            worst = np.maximum(worst, np.abs(vol.astype(np.float64) - want))
    for seed in (1, 2):                      # and two random sign fields
        rng = np.random.RandomState(1000 * seed + case["seed"])
        vol = _moved_volume(inp, lambda which, shape: rng.choice(np.array([-1, 1], dtype=F), size=shape), monkeypatch)
        worst = np.maximum(worst, np.abs(vol.astype(np.float64) - want))
    mx = float(worst.max())
    pct = float(np.percentile(worst, 99.99)) if worst.size >= 100000 else None
    print("%-14s freedom of a correct kernel: max-abs %.3e (a third of the gate: %.2e)%s" % (
        name, mx, SC.TOL / 3, "" if pct is None else "   99.99th percentile %.3e (%.2e)" % (pct, SC.TOL_PCT / 3)))
    assert mx > 0.0                          # (the angles did move)
    assert mx <= SC.TOL / 3, (name, mx)
    if pct is not None:
        assert pct < SC.TOL_PCT / 3, (name, pct)
    assert G.np is np
