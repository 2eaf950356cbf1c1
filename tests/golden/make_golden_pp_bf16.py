#!/usr/bin/env python
"""Generates tests/golden/full_config4_pp_bf16_256x256x32_b2_samples.npz from the CPU oracle: BASELINE configs[4]
(input_type=PP, two 256x256 cube faces, the second with a rotated source camera, 32 planes, ngf 64, CoordNet) with the
bf16 network as the build defines it (oracle/nets.py forward(bf16=True), the volume rounded to bf16), plus the distance
of that definition from the fp32 oracle on the same inputs -- what full_config2() of make_golden.py stores for the ODS
bf16 tier.

    python tests/golden/make_golden_pp_bf16.py      # a few minutes of CPU

The inputs are make_golden.pp_inputs / full_config4's.  The samples are the stratified set of tests.util.stratified_index
with a smaller per-stage cap (CAP) than the other full-size fixtures, so that the file stays under the repository's
1 MiB limit; the sweep volume's samples are stored as bf16 bits (exact).  tests/test_gpu_pp_bf16.py rebuilds the index
from (shape, seed, CAP)."""
import os
import sys

import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, os.path.dirname(os.path.dirname(HERE)))

from oracle import nets as onets  # noqa: E402
from oracle import poses as oposes  # noqa: E402
from oracle.msi import MSI as OracleMSI  # noqa: E402
from tests.golden.make_golden import pp_inputs  # noqa: E402

NAME = "full_config4_pp_bf16_256x256x32_b2_samples.npz"
CAP = 65536
SEED = 6
CFG = dict(seed=8968, b=2, n=256, d=32, ngf=64, coord=True)


def sample_index(shape):
    from tests.util import stratified_index
    return stratified_index(shape, None, SEED, cap=CAP)


def run(dtype):
    ref, src, K, eye, src_pose, tgt_pose = pp_inputs(CFG["seed"], CFG["b"], CFG["n"])
    d, ngf = CFG["d"], CFG["ngf"]
    weights = onets.init_weights(6 * d, 2 * d, ngf=ngf, coord_net=True, seed=CFG["seed"], randomize_affine=True)
    o = OracleMSI(weights=weights, coord_net=True, input_type="PP", dtype=dtype)
    planes = o.inv_depths(1.0, 100.0, d)
    interp = oposes.interpolate_pose(eye, src_pose)
    interp_inv = np.linalg.inv(interp.astype(np.float64)).astype(np.float32)
    pred, net_input = o.infer_msi(src, ref, None, None, eye, src_pose, K, "blend_psv", d, planes, ngf=ngf, ref_pose_inv=interp_inv)
    rgb = o.mpi_render_view(pred["rgba_layers"], np.matmul(tgt_pose, interp_inv).astype(np.float32), planes, K)
    return dict(psv=net_input, rgba_layers=pred["rgba_layers"], rgb=rgb)


def main():
    outs = {dtype: run(dtype) for dtype in ("bf16", "f32")}
    s = {"sample_seed": np.int64(SEED), "sample_cap": np.int64(CAP)}
    for k in ("psv", "rgba_layers", "rgb"):
        a = np.asarray(outs["bf16"][k], dtype=np.float32)
        idx = sample_index(a.shape)
        v = a.reshape(-1)[idx]
        s["shape_" + k] = np.array(a.shape, dtype=np.int64)
        s["mean_" + k] = np.float64(a.astype(np.float64).mean())
        if k == "psv":
            assert np.array_equal(onets.bf16_round(v), v)
            s["bits_psv"] = (v.view(np.uint32) >> 16).astype(np.uint16)
            continue
        s["val_" + k] = v
        f = np.asarray(outs["f32"][k], dtype=np.float32)
        s["f32val_" + k] = f.reshape(-1)[idx]
        diff = np.abs(a.astype(np.float64) - f.astype(np.float64))
        s["bf16_vs_f32_max_" + k] = np.float64(diff.max())
        s["bf16_vs_f32_mean_" + k] = np.float64(diff.mean())
    path = os.path.join(HERE, NAME)
    np.savez_compressed(path, cfg=np.array(sorted(CFG.items()), dtype=object), **s)
    print("wrote", NAME, os.path.getsize(path), "bytes", {k: float(s[k]) for k in s if k.startswith("bf16_vs_f32")})


if __name__ == "__main__":
    main()
