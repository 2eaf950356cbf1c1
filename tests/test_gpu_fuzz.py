"""Randomised GPU parity of the network against the oracle (a fixed-seed slice of tools/fuzz_parity.py):
random batch / image size / channel counts / CoordNet / dtype within the supported set -- M-tile tails,
channel tails (Cin, ngf not multiples of 32), N tails, widths at which the column border classes overlap."""
import numpy as np
import pytest

from tests.util import poison_workspace
pytestmark = pytest.mark.gpu


def test_random_network_shapes_match_oracle():
    import torch
    from matryodshka_amd import MSI
    from oracle import nets as onets
    rng = np.random.RandomState(2024)
    for it in range(14):
        dtype = "bf16" if it % 4 == 3 else "f32"
        q = 8 if dtype == "bf16" else 4
        b = int(rng.choice([1, 2, 3]))
        h, w = 8 * int(rng.randint(1, 7)), 8 * int(rng.randint(1, 10))
        cin, nout, ngf = q * int(rng.randint(1, 11)), 4 * int(rng.randint(1, 9)), q * int(rng.randint(1, 5))
        coord = bool(rng.rand() < 0.6)
        if not coord:            # wrap_pad(x, 2, 2) at 1/8 resolution needs two columns / rows
            h, w = max(h, 16), max(w, 16)
        weights = onets.init_weights(cin, nout, ngf=ngf, coord_net=coord, seed=int(rng.randint(1 << 30)), randomize_affine=True)
        x = rng.uniform(-1, 1, size=(b, h, w, cin)).astype(np.float32)
        if dtype == "bf16":
            x = onets.bf16_round(x)
        m = MSI(weights=weights, coord_net=coord, dtype=dtype)
        xt = torch.from_numpy(x).cuda()
        pred = m.run_net(xt.bfloat16() if dtype == "bf16" else xt, nout, ngf).cpu().numpy()
        ref = onets.forward(weights, x, coord_net=coord, bf16=dtype == "bf16")
        err = np.abs(pred - ref).max()
        assert np.isfinite(pred).all() and err <= (6e-2 if dtype == "bf16" else 1e-3), (it, dtype, b, h, w, cin, nout, ngf, coord, err)


FUZZ_NUM_CUS = (8, 9, 12, 20, 24, 56, 104, 256)     # tools/fuzz_parity.py --halo draws from the same set


def test_random_halo_shapes_options_and_cu_counts_match_oracle():
    """A fixed-seed slice of tools/fuzz_parity.py --halo: ngf 32 / 64 and maps that tile into 4 x 16 / 8 x 16 / 16 x 16 patches, so
    that the halo-patch kernels run, with a random HALO in {0, 1, 3, 5, 7}, FIXUP_KERNEL, BIGTILE in {1, 2} and NUM_CUS (small
    counts: the K-range splits, odd counts, the stride-2 halo kernels on small grids), each on a workspace poisoned with NaN
    bytes.  Sizes are capped at 64 x 128 pixels per batch so that the CPU oracle stays a fraction of a second per case."""
    import torch
    from matryodshka_amd import MSI, _native as N
    from oracle import nets as onets
    rng = np.random.RandomState(777)
    split_cases = 0
    for it in range(12):
        dtype = "bf16" if it % 3 == 2 else "f32"
        q = 8 if dtype == "bf16" else 4
        b = int(rng.choice([1, 1, 2, 3]))
        h, w = 16 * int(rng.randint(1, 5)), 16 * int(rng.randint(1, 9))
        if rng.rand() < 0.5:
            h, w = 32 * int(rng.randint(1, 3)), 128          # every level tiles into patches
        while b * h * w > 64 * 128:
            b -= 1
        ngf = int(rng.choice([32, 64]))
        cq = 64 if dtype == "bf16" else 32
        cin = cq * int(rng.randint(1, 4)) if rng.rand() < 0.7 else q * int(rng.randint(1, 13))
        nout = 4 * int(rng.randint(1, 9))
        coord = bool(rng.rand() < 0.6)
        opts = {N.NET_OPT_HALO: int(rng.choice([0, 1, 3, 5, 5, 7])), N.NET_OPT_FIXUP_KERNEL: int(rng.rand() < 0.3),
                N.NET_OPT_BIGTILE: int(rng.choice([1, 1, 2])), N.NET_OPT_NUM_CUS: int(rng.choice(FUZZ_NUM_CUS))}
        weights = onets.init_weights(cin, nout, ngf=ngf, coord_net=coord, seed=int(rng.randint(1 << 30)), randomize_affine=True)
        x = rng.uniform(-1, 1, size=(b, h, w, cin)).astype(np.float32)
        if dtype == "bf16":
            x = onets.bf16_round(x)
        m = MSI(weights=weights, coord_net=coord, dtype=dtype)
        m.net_options.update(opts)
        poison_workspace(m, b, h, w, cin, nout, ngf)
        split_cases += any(k[2] > 0 for k in m._plan(b, h, w, cin, nout, ngf).kernels()[:17])
        xt = torch.from_numpy(x).cuda()
        pred = m.run_net(xt.bfloat16() if dtype == "bf16" else xt, nout, ngf).cpu().numpy()
        ref = onets.forward(weights, x, coord_net=coord, bf16=dtype == "bf16")
        err = np.abs(pred - ref).max()
        assert np.isfinite(pred).all() and err <= (6e-2 if dtype == "bf16" else 1e-3), \
            (it, dtype, b, h, w, cin, nout, ngf, coord, "HALO %d FIXUP_KERNEL %d BIGTILE %d NUM_CUS %d" % tuple(
                opts[k] for k in (N.NET_OPT_HALO, N.NET_OPT_FIXUP_KERNEL, N.NET_OPT_BIGTILE, N.NET_OPT_NUM_CUS)), err)
    assert split_cases >= 6, split_cases      # (the slice is about K-range splits: most of its plans must cut tiles -- 10 of 12 when it was written)


def test_random_sweep_shapes_on_the_lds_staged_kernel_match_oracle_and_the_gather_kernel():
    """Round 6: a fixed-seed slice over shapes that take ods_sweep_lds_kernel (batch >= 2, (W * D / 2) % 256 == 0): random sizes, sphere counts, baselines (up to 10 x the
    usual one: wide polar boxes, fallback blocks), far planes, identity and small rigid source poses -- the volume against the oracle (identity poses: max; posed: 99.9th
    percentile, isolated branch flips allowed as in tests/test_gpu_geometry.py) and, bit for bit, against each frame swept alone (batch 1: the gather kernel)."""
    import torch
    from matryodshka_amd import MSI
    from oracle.msi import MSI as OracleMSI
    from matryodshka_amd.synthetic import make_inputs
    rng = np.random.RandomState(606)
    m, o = MSI(), OracleMSI()
    for it in range(10):
        b = int(rng.choice([2, 3, 5]))
        d = int(rng.choice([16, 32, 64]))
        h, w = 2 * int(rng.randint(4, 24)), 32 * int(rng.randint(1, 5))
        assert (w * (d // 2)) % 256 == 0
        inp = make_inputs(int(rng.randint(1 << 30)), b, h, w)
        inp["intrinsics"][:, 0, 0] = rng.uniform(0.01, 0.3)
        posed = rng.rand() < 0.5
        if posed:
            th = rng.uniform(-0.05, 0.05)
            p = np.eye(4, dtype=np.float32)
            p[0, 0], p[0, 2], p[2, 0], p[2, 2] = np.cos(th), np.sin(th), -np.sin(th), np.cos(th)
            p[:3, 3] = rng.uniform(-0.02, 0.02, 3)
            inp["src_pose"] = np.tile(p[None], (b, 1, 1))
        planes = m.inv_depths(1.0, float(rng.uniform(20, 100)), d)
        ref, src = m.preprocess_image(torch.from_numpy(inp["ref_image"])), m.preprocess_image(torch.from_numpy(inp["src_image"]))
        psv_t = m.format_network_input(ref, src, inp["ref_pose"], inp["src_pose"], planes, inp["intrinsics"])
        for k in range(b):
            one = m.format_network_input(ref[k:k + 1], src[k:k + 1], inp["ref_pose"][k:k + 1], inp["src_pose"][k:k + 1], planes, inp["intrinsics"][k:k + 1])
            assert torch.equal(one[0], psv_t[k]), (it, k, b, h, w, d)
        psv_o = o.format_network_input(o.preprocess_image(inp["ref_image"]), o.preprocess_image(inp["src_image"]),
                                       inp["ref_pose"], inp["src_pose"], planes, inp["intrinsics"])
        e = np.abs(psv_t.cpu().numpy() - psv_o)
        g = float(np.percentile(e, 99.9)) if posed else float(e.max())
        assert g <= 1e-3, (it, b, h, w, d, posed, g)
