#!/usr/bin/env python
"""SHA-256 digests of everything the conv planner decides and of the host weight packer's output, against tests/golden/plan_digests.json:
a refactor of csrc/cnn_plan.hip or csrc/cnn_net.hip must leave every one of them as it was.  No GPU is needed.

A plan digest covers, for every CU count given and each of the 18 layers: msi_net_plan_layer_kernel's name, workgroups and tiles cut, and
the bytes of msi_net_plan_layer_params (the planned kernel argument, then inlaunch, fuse_ln, skip_apply, ln_blocks).  There is one per
(SWEEP_DESCS entry, SWEEP_OPTIONS entry) over SWEEP_CUS and one per DECOMP_CASES / OPTION_CASES plan at its own CU count (the lists of
tests/test_plan_decomposition.py, which imports the digest functions below); the weight digests are those of tests/test_native_abi.py.

  python tools/plan_golden.py            recompute everything and compare with the file (exit 1 on a difference)
  python tools/plan_golden.py --record   write the file -- from the commit BEFORE a planner change, never from the changed planner
A change of the argument record's SIZE (members added to or removed from ConvParams) moves every plan digest: it is re-recorded from the changed tree only
after a byte-for-byte comparison of every layer record of every plan above against the parent's -- names, workgroups, tiles cut, the common part of the bytes."""
import hashlib
import json
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
if ROOT not in sys.path:
    sys.path.insert(0, ROOT)
GOLDEN = os.path.join(ROOT, "tests", "golden", "plan_digests.json")
WEIGHT_DESCS = {"A": ("f32", (1, 64, 128, 96, 32, 64), True), "D": ("bf16", (2, 32, 128, 64, 16, 64), False)}   # test_plan_decomposition's A and D


def _native():
    from matryodshka_amd import build
    build.build(verbose=False)
    from matryodshka_amd import _native as N, nets
    return N, nets


def _add_layers(h, plan):
    for li in range(18):
        kernel, nblocks, nsplit = plan.layer_kernel(li)
        h.update(("%d|%s|%d|%d|" % (li, kernel, nblocks, nsplit)).encode())
        h.update(plan.layer_params(li))


def sweep_digest(dtype, shape, coord, named, cus_list):
    """One description under the options `named` ({name without NET_OPT_: value}), NUM_CUS walked over `cus_list`."""
    N, nets = _native()
    b, hh, w, cin, nout, ngf = shape
    plan = N.NetPlan(nets.make_desc(b, hh, w, cin, nout, ngf, coord, dtype), {getattr(N, "NET_OPT_" + k): v for k, v in named.items()})
    h = hashlib.sha256()
    for cus in cus_list:
        plan.set_option(N.NET_OPT_NUM_CUS, cus)
        h.update(("cus %d|" % cus).encode())
        _add_layers(h, plan)
    return h.hexdigest()


def plan_digest(plan):
    """A plan as it stands (test_plan_decomposition.plan_for's)."""
    h = hashlib.sha256()
    _add_layers(h, plan)
    return h.hexdigest()


def weights_digest(which):
    """msi_net_pack_weights_host's output for WEIGHT_DESCS[which] on numpy.random.default_rng(0) parameters."""
    import numpy as np
    N, nets = _native()
    dtype, (b, hh, w, cin, nout, ngf), coord = WEIGHT_DESCS[which]
    desc = nets.make_desc(b, hh, w, cin, nout, ngf, coord, dtype)
    params = np.random.default_rng(0).standard_normal(N.lib.msi_net_param_floats(desc), dtype=np.float32)
    return hashlib.sha256(nets.pack_params(desc, params).tobytes()).hexdigest()


def sweep_key(dtype, shape, coord, named):
    return "sweep|%s|%s|%s|%s" % (dtype, "x".join(map(str, shape)), "coord" if coord else "wrap", json.dumps(named, sort_keys=True))


def case_key(case, extra=None):
    return "case|%s|%s" % (case["id"], json.dumps(extra or {}, sort_keys=True))


def all_digests():
    from tests import test_plan_decomposition as T
    out = {}
    for _, dtype, shape, coord in T.SWEEP_DESCS:
        for named in T.SWEEP_OPTIONS:
            out[sweep_key(dtype, shape, coord, named)] = sweep_digest(dtype, shape, coord, named, T.SWEEP_CUS)
    for case, extra in [(c, None) for c in T.DECOMP_CASES] + list(T.OPTION_CASES) + [(c, None) for c, _ in T.OPTION_CASES]:
        out[case_key(case, extra)] = plan_digest(T.plan_for(case, extra))
    for which in sorted(WEIGHT_DESCS):
        out["weights|" + which] = weights_digest(which)
    return out


def golden():
    with open(GOLDEN) as f:
        return json.load(f)


if __name__ == "__main__":
    got = all_digests()
    if "--record" in sys.argv:
        with open(GOLDEN, "w") as f:
            json.dump(got, f, indent=0, sort_keys=True)
            f.write("\n")
        print("wrote %d digests to %s" % (len(got), GOLDEN))
    else:
        want = golden()
        bad = sorted(k for k in set(got) | set(want) if got.get(k) != want.get(k))
        print("%d digests, %d differ%s" % (len(got), len(bad), "".join("\n  " + k for k in bad)))
        sys.exit(1 if bad else 0)
