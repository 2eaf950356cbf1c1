"""The case table of the sweep-form tests (tests/test_gpu_sweep_forms.py on the device, tests/test_sweep_cases_cpu.py on the host) and a host-side
model of what sweep_common (matryodshka_amd/csrc/geo_sweep.hip) launches for a shape and of what ods_sweep_lds_kernel's blocks decide on the device.

sweep_form:  the kernel form of a launch, condition by condition from sweep_common in the default build.
lds_blocks:  per block of ods_sweep_lds_kernel, whether its source patch fits in LDS (it stages) or not (it gathers from memory like ods_sweep_kernel),
             from the oracle's sample positions: the device decides this per block and nothing it writes tells which way it went.
CASES:       shapes of a few thousand pixels that between them reach every form, with per-frame poses and baselines.
compare_f32 / bf16_bits_differ: the two comparisons of the device test; the host test shows that they see the faults they are there for.
"""
import numpy as np

from oracle import geometry as G

F = np.float32

# ---- sweep_common, default build (the macros of geo_sweep.hip)
SW_PMAX = 192            # MSI_SWEEP_PMAX: texels of a staged patch per source
BCHUNK = 16              # MSI_SWEEP_BCHUNK: frames a thread walks
NS_DEFAULT = 2           # MSI_SWEEP_NS_DEFAULT
LDS_MIN_BATCH = 2        # MSI_SWEEP_LDS_MIN_BATCH


def sweep_form(b, h, w, d, pair, bf16):
    """What sweep_common launches for batch b > 0, an [h, w] image and d spheres: ("f32" | "bf16", "lds") or (dtype, "gather", NS, NSRC, LOOP, coalesce).
    pair: msi_ods_sweep_volume (both sources); otherwise one of the single-source entry points.  coalesce is MSI_LAUNCH_SWEEP's expression without the
    non-temporal bit (volumes beyond 256 MiB)."""
    assert b > 0 and h > 0 and w > 0 and d > 0
    dtype = "bf16" if bf16 else "f32"
    ns = NS_DEFAULT
    while d % ns != 0:
        ns >>= 1
    bchunk = b if b < BCHUNK else BCHUNK
    ng2 = d // 2
    if pair and ns == 2 and b >= LDS_MIN_BATCH and ng2 > 0 and 64 % ng2 == 0 and (w * ng2) % 256 == 0:
        return (dtype, "lds")
    ng = d // ns
    coalesce = 1 if (pair and 64 % ng == 0 and (w * ng) % 64 == 0) else 0
    return (dtype, "gather", ns, 2 if pair else 1, 1 if bchunk > 1 else 0, coalesce)


def _all_forms():
    forms = []
    for dtype in ("f32", "bf16"):
        forms.append((dtype, "lds"))
        forms += [(dtype, "gather", ns, 2, loop, co) for ns in (1, 2) for loop in (0, 1) for co in (0, 1)]
        forms += [(dtype, "gather", ns, 1, loop, 0) for ns in (1, 2) for loop in (0, 1)]
    return frozenset(forms)


ALL_FORMS = _all_forms()          # the 26 forms the default build can launch
assert len(ALL_FORMS) == 26


def launches(b, h, w, d):
    """(what, b, pair, bf16) of every sweep launch the device test makes for a case: the double volume of the whole batch, the two single-source sweeps
    of the whole batch and the double volume of every frame alone, each in fp32 and bf16."""
    out = []
    for bf16 in (False, True):
        out += [("volume", b, True, bf16), ("single", b, False, bf16), ("alone", 1, True, bf16)]
    return out


def case_forms(case):
    return {sweep_form(nb, case["h"], case["w"], case["d"], pair, bf16) for _, nb, pair, bf16 in launches(case["b"], case["h"], case["w"], case["d"])}


# ---- the per-block model of ods_sweep_lds_kernel
def centred(d, n):
    """geo_sweep.hip centred(): d in (-2n, 2n) -> the representative of d mod n in [-n/2, n/2)."""
    d = np.asarray(d, dtype=np.int64).copy()
    half = n >> 1
    for _ in range(2):
        d = np.where(d < -half, d + n, d)
        d = np.where(d >= n - half, d - n, d)
    return d


def oracle_uv(h, w, depths, pose, baseline, order):
    """The oracle's sample positions [D, h, w, 2] (x, y) of one frame and one source."""
    intr = np.zeros((1, 3, 3), dtype=F)
    intr[0, 0, 0] = baseline
    _, masks = G.ods_sphere_sweep(np.zeros((1, h, w, 3), dtype=F), order, depths, np.asarray(pose, dtype=F)[None], intr, return_masks=True)
    return masks[0][2], masks[0][1]


def corners(uv, h, w):
    """make_taps_lds' clamped, unwrapped corner (x0, y0) of every sample."""
    with np.errstate(invalid="ignore"):
        x0 = np.clip(np.floor(uv[..., 0]), -1, w - 1).astype(np.int64)
        y0 = np.clip(np.floor(uv[..., 1]), -1, h - 1).astype(np.int64)
    return x0, y0


def lds_blocks(h, w, d, pose0, pose1, baseline, depths):
    """One frame of ods_sweep_lds_kernel<*, 2>: per block (row i, block bx of 256 / (d / 2) pixels) three [h, blocks per row] bool arrays:
    stages (its box fits: ph * pitch <= SW_PMAX), seam (the patch spans the column seam W-1 | 0) and wrap (it spans the row wrap H-1 | 0).
    Both sources' sample positions come from the oracle (pose0 with order +1, pose1 with order -1); the box is measured, as on the device, from
    (W - 1 - j0, i) with centred()."""
    ng = d // 2
    assert d % 2 == 0 and 64 % ng == 0 and (w * ng) % 256 == 0
    ppb = 256 // ng                                      # pixels per block
    nbx = w // ppb
    xs, ys = [], []
    for pose, order in ((pose0, 1), (pose1, -1)):
        uv, _ = oracle_uv(h, w, depths, pose, baseline, order)
        x0, y0 = corners(uv, h, w)
        xs.append(x0); ys.append(y0)
    x0 = np.stack(xs)                                    # [2, D, h, w]
    y0 = np.stack(ys)
    stages = np.zeros((h, nbx), dtype=bool)
    seam = np.zeros((h, nbx), dtype=bool)
    wrap = np.zeros((h, nbx), dtype=bool)
    rows = np.arange(h).reshape(1, 1, h, 1)
    for bx in range(nbx):
        j0 = bx * ppb
        xc = w - 1 - j0
        xr = centred(x0[:, :, :, j0:j0 + ppb] - xc, w)
        yr = centred(y0[:, :, :, j0:j0 + ppb] - rows, h)
        xmin, xmax = xr.min(axis=(0, 1, 3)), xr.max(axis=(0, 1, 3))      # [h]
        ymin, ymax = yr.min(axis=(0, 1, 3)), yr.max(axis=(0, 1, 3))
        pw, ph = xmax - xmin + 2, ymax - ymin + 2
        pitch = ((pw + 7) & ~15) + 8
        stages[:, bx] = ph * pitch <= SW_PMAX
        lo, hi = xc + xmin, xc + xmin + pw - 1                             # unwrapped first and last patch column
        seam[:, bx] = (lo // w) != (hi // w)
        lo, hi = np.arange(h) + ymin, np.arange(h) + ymin + ph - 1
        wrap[:, bx] = (lo // h) != (hi // h)
    return stages, seam, wrap


# ---- the cases
IDENT = (0.0, 0.0, 0.0)
SHIFT = (0.01, -0.02, 0.015)
BASELINE = 0.032
# per-frame settings: (translation of the reference pose, translation of the source pose, baseline)
S0 = (IDENT, IDENT, BASELINE)            # the test path: identity poses, the camera file's baseline (both sources share the quadratic)
S1 = (IDENT, SHIFT, BASELINE)            # a changed source pose
S2 = (SHIFT, IDENT, BASELINE)            # a changed reference pose
S3 = (IDENT, IDENT, 0.05)                # a changed baseline


def _runs(*runs):
    out = []
    for setting, n in runs:
        out += [setting] * n
    return out


_CHUNK16 = _runs((S0, 4), (S1, 3), (S2, 2), (S3, 3), (S0, 4))      # runs of equal frames, every change, a return to the first setting


def _case(b, h, w, d, frames, claims, seed):
    assert len(frames) == b
    return dict(name="b%d_%dx%dx%d" % (b, h, w, d), b=b, h=h, w=w, d=d, frames=frames, claims=frozenset(claims), seed=seed)


# claims: what an entry is there for, each shown by tests/test_sweep_cases_cpu.py --
#   seam_x1 / seam_x0: samples with x0 = W-1 (x1 wraps to column 0) / x0 = -1 (wraps to W-1); row_m1 / row_h1: y0 = -1 / y0 = H-1; invalid: disc < 0 samples;
#   odd_d: D is odd and > 1; baseline: the baseline changes between frames; lds: the double volume takes ods_sweep_lds_kernel; chunk2: more than 16 frames.
CASES = [
    _case(1, 20, 70, 5, [S1], ("seam_x1", "seam_x0", "row_m1", "row_h1", "invalid", "odd_d"), 11),
    _case(3, 20, 70, 5, [S0, S0, S1], ("seam_x1", "seam_x0", "row_m1", "row_h1", "invalid", "odd_d"), 12),
    _case(1, 16, 64, 1, [S1], ("seam_x1", "seam_x0", "row_m1", "row_h1"), 13),
    _case(3, 16, 64, 1, [S1, S3, S3], ("seam_x1", "seam_x0", "row_m1", "row_h1", "baseline"), 14),
    _case(1, 12, 40, 6, [S1], ("seam_x1", "seam_x0", "row_m1", "row_h1", "invalid"), 15),
    _case(2, 12, 40, 6, [S2, S1], ("seam_x1", "seam_x0", "row_m1", "row_h1", "invalid"), 16),
    _case(1, 8, 32, 4, [S1], ("seam_x0", "row_m1", "row_h1"), 17),
    _case(2, 8, 32, 4, [S0, S3], ("baseline",), 18),
    _case(16, 8, 32, 4, _CHUNK16, ("baseline",), 19),
    _case(17, 8, 32, 4, _CHUNK16 + [S1], ("baseline", "chunk2"), 20),                                              # frame 16 differs from frame 15
    _case(33, 8, 32, 4, _CHUNK16 + _runs((S0, 2), (S3, 5), (S1, 4), (S2, 5)) + [S1], ("baseline", "chunk2"), 21),  # frame 16 equals frame 15; frame 32 changes
    _case(2, 16, 64, 16, [S0, S0], ("lds",), 22),
    _case(17, 16, 64, 16, _CHUNK16 + [S3], ("lds", "baseline", "chunk2"), 23),                                     # the baseline changes AT the chunk start
    _case(33, 8, 64, 16, _CHUNK16 + _runs((S0, 3), (S3, 5), (S1, 4), (S2, 4)) + [S3], ("lds", "baseline", "chunk2"), 24),
]

WINDOW_CASES = ("b3_20x70x5", "b2_12x40x6")      # the window test: one NS = 1 and one NS = 2 case, single source


def case_by_name(name):
    return next(c for c in CASES if c["name"] == name)


def depths_of(d):
    """The d sphere radii of a case: MSI.inv_depths(1, 100, d); a single sphere sits at 0.5 (inv_depths needs both ends)."""
    if d == 1:
        return [0.5]
    from oracle.msi import MSI as OracleMSI
    return OracleMSI().inv_depths(1.0, 100.0, d)


def case_inputs(case):
    """Images (per-texel uniform noise in [-1, 1]: every wrong texel shows), poses, intrinsics and depths of a case, as fp32 numpy arrays."""
    b, h, w = case["b"], case["h"], case["w"]
    rng = np.random.RandomState(case["seed"])
    ref = rng.uniform(-1.0, 1.0, size=(b, h, w, 3)).astype(F)
    src = rng.uniform(-1.0, 1.0, size=(b, h, w, 3)).astype(F)
    pose0 = np.tile(np.eye(4, dtype=F)[None], (b, 1, 1))
    pose1 = pose0.copy()
    intr = np.tile(np.eye(3, dtype=F)[None], (b, 1, 1))
    for k, (t0, t1, bl) in enumerate(case["frames"]):
        pose0[k, :3, 3] = t0
        pose1[k, :3, 3] = t1
        intr[k, 0, 0] = bl
    return dict(ref=ref, src=src, pose0=pose0, pose1=pose1, intr=intr, depths=np.asarray(depths_of(case["d"]), dtype=F))


def oracle_volume(inp, depths=None, intr=None, order1=-1):
    """The oracle's double volume of case_inputs: ods_sphere_sweep per source, concatenated.  depths / intr / order1: the perturbed calls of the fault tests."""
    depths = inp["depths"] if depths is None else depths
    intr = inp["intr"] if intr is None else intr
    return np.concatenate([G.ods_sphere_sweep(inp["ref"], 1, depths, inp["pose0"], intr),
                           G.ods_sphere_sweep(inp["src"], order1, depths, inp["pose1"], intr)], axis=3)


# ---- the comparisons of the device test
TOL = 1e-3                 # max-abs gate of the project (tests/test_gpu_render_views.py _compare)
TOL_PCT = 1e-4             # 99.99th percentile, where there are at least 1e5 values


def errors_f32(got, want):
    """(max-abs, 99.99th percentile or None below 1e5 values) of an fp32 volume against the oracle's."""
    err = np.abs(np.asarray(got).astype(np.float64) - want)
    return float(err.max()), (float(np.percentile(err, 99.99)) if err.size >= 100000 else None)


def compare_f32(got, want, what="", scale=1.0):
    """The gates of _compare in tests/test_gpu_render_views.py; scale < 1 tightens both (the host test holds a correct kernel's freedom to a third)."""
    mx, pct = errors_f32(got, want)
    assert np.isfinite(mx) and mx <= TOL * scale, (what, "max-abs", mx)
    if pct is not None:
        assert pct < TOL_PCT * scale, (what, "99.99th percentile", pct)
    return mx, pct


def bf16_bits(x):
    """int16 bit patterns of the round-to-nearest-even bf16 of an fp32 array (torch's conversion, on the host)."""
    import torch
    return torch.from_numpy(np.array(x, dtype=F)).to(torch.bfloat16).view(torch.int16).numpy()


def bf16_bits_differ(got_bits, volume_f32):
    """Number of elements whose bf16 bit pattern is not the rounded fp32 volume's."""
    return int((np.asarray(got_bits) != bf16_bits(volume_f32)).sum())


# ---- the parametrizations of the two older tests of the LDS-staged sweep, restated for the staging model
def _rot(ax, ay, az):
    cx, sx, cy, sy, cz, sz = np.cos(ax), np.sin(ax), np.cos(ay), np.sin(ay), np.cos(az), np.sin(az)
    rx = np.array([[1, 0, 0], [0, cx, -sx], [0, sx, cx]]); ry = np.array([[cy, 0, sy], [0, 1, 0], [-sy, 0, cy]]); rz = np.array([[cz, -sz, 0], [sz, cz, 0], [0, 0, 1]])
    m = np.eye(4); m[:3, :3] = rz @ ry @ rx
    return m.astype(F)


LDS_GEOMETRY_PARAMS = [(24, 64, 16, 5), (40, 64, 32, 3), (16, 32, 64, 2), (24, 128, 8, 19), (24, 64, 16, 19)]     # (h, w, d, b) of test_lds_staged_sweep_is_bit_identical_to_the_gather_kernel


def lds_geometry_frames(h, w, d, b):
    """(pose0, pose1, baselines, depths) of tests/test_gpu_geometry.py test_lds_staged_sweep_is_bit_identical_to_the_gather_kernel."""
    p0 = np.tile(np.eye(4, dtype=F)[None], (b, 1, 1))
    p1 = p0.copy()
    bl = np.full(b, 0.032, dtype=F)
    p1[1, 0, 3] = 0.01
    if b > 2:
        p1[2] = _rot(0.3, -0.5, 0.2); p1[2, :3, 3] = (0.01, -0.02, 0.005)
    if b > 3:
        p0[3] = _rot(-0.1, 0.05, 0.0)
    if b > 6:
        bl[5:7] = 0.4
    if b > 17:
        p1[17, 2, 3] = 0.015
    return p0, p1, bl, np.asarray(depths_of(d), dtype=F)


def lds_fuzz_frames():
    """[(h, w, d, b, pose0, pose1, baselines, depths)] of the ten draws of tests/test_gpu_fuzz.py
    test_random_sweep_shapes_on_the_lds_staged_kernel_match_oracle_and_the_gather_kernel (seed 606, the same draws in the same order)."""
    from oracle.msi import MSI as OracleMSI
    rng = np.random.RandomState(606)
    out = []
    for _ in range(10):
        b = int(rng.choice([2, 3, 5]))
        d = int(rng.choice([16, 32, 64]))
        h, w = 2 * int(rng.randint(4, 24)), 32 * int(rng.randint(1, 5))
        rng.randint(1 << 30)                              # the seed of the images
        bl = np.full(b, rng.uniform(0.01, 0.3), dtype=F)
        p0 = np.tile(np.eye(4, dtype=F)[None], (b, 1, 1))
        p1 = p0.copy()
        if rng.rand() < 0.5:
            th = rng.uniform(-0.05, 0.05)
            p = np.eye(4, dtype=F)
            p[0, 0], p[0, 2], p[2, 0], p[2, 2] = np.cos(th), np.sin(th), -np.sin(th), np.cos(th)
            p[:3, 3] = rng.uniform(-0.02, 0.02, 3)
            p1 = np.tile(p[None], (b, 1, 1))
        depths = np.asarray(OracleMSI().inv_depths(1.0, float(rng.uniform(20, 100)), d), dtype=F)
        out.append((h, w, d, b, p0, p1, bl, depths))
    return out


def staging(h, w, d, pose0, pose1, baselines, depths):
    """lds_blocks of every frame of a batch: three [b, h, blocks per row] bool arrays.  Equal consecutive settings are modelled once."""
    memo, frames = {}, []
    for k in range(len(baselines)):
        key = (pose0[k].tobytes(), pose1[k].tobytes(), F(baselines[k]).tobytes())
        if key not in memo:
            memo[key] = lds_blocks(h, w, d, pose0[k], pose1[k], baselines[k], depths)
        frames.append(memo[key])
    return tuple(np.stack([f[i] for f in frames]) for i in range(3))
