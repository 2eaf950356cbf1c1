"""MSI.hres_cube_layers(src_sampling='panorama') (msi_cube_hres_layers, msi_cube_hres_layers_sparse): the high-res cube stack in one pass with its
background sampled from the source panorama.  The yardstick is the three launches it replaces, called through the binding --
MSI.format_cube_input at the high size (fp32) -> msi_resize_bilinear_f32 of cat([blend_weights, alphas]) -> msi_assemble_rgba_scaled_f32, plus
msi_pack_layers -- and sparsify_layers(..., border='edge') of the dense packed stack for the sparse build.  Every comparison is on raw bits."""
import functools

import numpy as np
import pytest

from matryodshka_amd.synthetic import smooth_noise
from tests import cube_sweep_cases as cases

pytestmark = pytest.mark.gpu

F = np.float32
LOW, D = 8, 4
PLANES = (100.0, 10.0, 3.0, 1.0)
# D = 4 is ONE layer group of the builders (HRES_G = 4): their group loop runs once.  This case has two, with alpha blocks sparse enough that whole groups drop.
SEED_TWO_GROUPS = 3       # (by the keep rule restated in numpy: 5 of the 24 tiles drop all of layers 4..7, 17 keep some of them, 2 keep all four)
TWO_GROUPS = dict(s=16, b=1, d=8, planes=(100.0, 30.0, 10.0, 5.0, 3.0, 2.0, 1.5, 1.0), on=0.06, seed=SEED_TWO_GROUPS)
FORMATS = ["f32", "rgba8", "rgba16f", ("f32", "rgba8")]
CODE_DTYPE = {"rgba8": "uint8", "rgba16f": "float16"}
SHAPES = [(16, 1), (16, 2), (32, 1), (32, 2)]          # (face size, cubes)


@pytest.fixture(scope="module")
def model():
    from matryodshka_amd import MSI
    return MSI()                       # (any model: the stack is built from its arguments)


@functools.lru_cache(maxsize=None)
def _case(s, b, d=D, planes=PLANES, on=0.25, seed=None):
    """Low-res blend weights and alphas [6B,8,8,D] (alphas zero outside random 2 x 3-texel blocks, each on with probability `on`, so that the sparse
    build drops tiles), a pair of raw panoramas in [0, 1], and the source poses: the rotated and translated one, after the identity when B = 2."""
    rng = np.random.RandomState(100 * s + b if seed is None else seed)
    x = dict(s=s, b=b, d=d, planes=planes)
    x["bw"] = rng.uniform(0.0, 1.0, size=(6 * b, LOW, LOW, d)).astype(F)
    on = rng.uniform(size=(6 * b, LOW // 2, -(-LOW // 3), d)) < on
    x["al"] = (rng.uniform(0.05, 0.95, size=(6 * b, LOW, LOW, d)) * np.repeat(np.repeat(on, 2, axis=1), 3, axis=2)[:, :LOW, :LOW]).astype(F)
    x["raw_src"], x["raw_ref"] = smooth_noise(rng, b, 24, 50, factor=4), smooth_noise(rng, b, 24, 50, factor=4)
    x["src_pose"] = cases.source_poses()[2 - b:]
    for v in x.values():
        if isinstance(v, np.ndarray):
            v.setflags(write=False)
    return x


def _bits(t):
    import torch
    t = t.contiguous()
    return t.view({4: torch.int32, 2: torch.int16, 1: torch.uint8}[t.element_size()])


def _same_bits(a, b):
    import torch
    return a.shape == b.shape and a.dtype == b.dtype and torch.equal(_bits(a), _bits(b))


_YARDSTICK = {}


def _three_launches(m, s, b, **case):
    """The native fp32 stack [6B,D,S,S,4] of the three launches, on the inputs hres_cube_layers prepares; run once per case and shared."""
    import torch
    from matryodshka_amd import _native as N, cubemap
    key = (s, b) + tuple(sorted(case.items()))
    if key not in _YARDSTICK:
        x = _case(s, b, **case)
        D, PLANES = x["d"], x["planes"]
        k = cubemap.default_face_intrinsics(s)
        ref_faces = m.preprocess_image(m.equirect_to_cube(m._f32(x["raw_ref"]), s, k).reshape(6 * b, s, s, 3))
        pano = m.preprocess_image(m._f32(x["raw_src"]))
        face_src = cubemap.face_poses(m._f32(x["src_pose"])).reshape(6 * b, 4, 4).contiguous()
        kf = m._f32(k).reshape(1, 3, 3).expand(6 * b, 3, 3).contiguous()
        psv = m.format_cube_input(ref_faces, pano, face_src, PLANES, kf, dtype='f32')
        st = m._stream()
        low = torch.cat([m._f32(x["bw"]), m._f32(x["al"])], dim=-1).contiguous()
        up = torch.empty((6 * b, s, s, 2 * D), dtype=torch.float32, device=m.device)
        N.check(N.lib.msi_resize_bilinear_f32(low.data_ptr(), up.data_ptr(), 6 * b, LOW, LOW, 2 * D, s, s, st), "resize")
        rgba = torch.empty((6 * b, D, s, s, 4), dtype=torch.float32, device=m.device)
        N.check(N.lib.msi_assemble_rgba_scaled_f32(psv.data_ptr(), up.data_ptr(), rgba.data_ptr(), 6 * b, s, s, D, st), "assemble")
        _YARDSTICK[key] = rgba
    return _YARDSTICK[key]


def _pack(m, rgba, fmt):
    import torch
    from matryodshka_amd import _native as N
    codes = torch.empty(rgba.shape, dtype=getattr(torch, CODE_DTYPE[fmt]), device=m.device)
    N.check(N.lib.msi_pack_layers(rgba.data_ptr(), m.LAYER_FORMATS[fmt], codes.data_ptr(), rgba.numel() // 4, m._stream()), "pack")
    return codes


def _new(m, s, b, case=None, **kw):
    x = _case(s, b, **(case or {}))
    return m.hres_cube_layers(x["bw"], x["al"], x["raw_src"], x["raw_ref"], x["src_pose"], s, x["planes"], src_sampling='panorama', **kw)


@pytest.mark.parametrize("layer_format", FORMATS, ids=lambda f: f if isinstance(f, str) else "+".join(f))
@pytest.mark.parametrize("s,b", SHAPES)
def test_1_every_request_has_the_bits_of_the_three_launches(model, s, b, layer_format):
    import torch
    m = model
    want = _three_launches(m, s, b)
    got = _new(m, s, b, layer_format=layer_format)
    req = (layer_format,) if isinstance(layer_format, str) else layer_format
    assert sorted(got) == sorted({"f32": "rgba_layers"}.get(f, "packed_layers") for f in req)
    assert bool(torch.isfinite(want).all()) and float(want[..., :3].abs().max()) > 0.1
    if "f32" in req:
        assert _same_bits(got["rgba_layers"], want.permute(0, 2, 3, 1, 4))
    for f in req:
        if f != "f32":
            pk = got["packed_layers"]
            assert pk.format == f and pk.planes == tuple(float(p) for p in PLANES)
            assert _same_bits(pk.data, _pack(m, want, f))


def test_1b_the_background_is_the_panoramas_not_the_cut_faces(model):
    """The two modes build different stacks (the background differs past the face borders) with equal alphas; 'face' stays the default."""
    m, (s, b) = model, (16, 2)
    x = _case(s, b)
    args = (x["bw"], x["al"], x["raw_src"], x["raw_ref"], x["src_pose"], s, PLANES)
    new = _new(m, s, b, layer_format='f32')["rgba_layers"]
    old = m.hres_cube_layers(*args, layer_format='f32')["rgba_layers"]
    assert _same_bits(old, m.hres_cube_layers(*args, layer_format='f32', src_sampling='face')["rgba_layers"])
    assert _same_bits(new[..., 3], old[..., 3]) and not _same_bits(new[..., :3], old[..., :3])
    with pytest.raises(ValueError, match="src_sampling"):
        m.hres_cube_layers(*args, src_sampling='seamless')


@pytest.mark.parametrize("fmt", ["rgba8", "rgba16f"])
@pytest.mark.parametrize("s,b", SHAPES)
def test_2_sparse_request_has_the_bits_of_sparsify_edge_of_the_dense_request(model, s, b, fmt):
    import torch
    m = model
    dense = _new(m, s, b, layer_format=fmt)["packed_layers"]
    want = m.sparsify_layers(dense, border='edge')
    got = _new(m, s, b, layer_format=fmt, sparse=True)
    assert sorted(got) == ["sparse_layers"]
    got = got["sparse_layers"]
    assert got.border == 'edge' and got.format == fmt and got.planes == tuple(float(p) for p in PLANES)
    assert 0.0 < got.occupancy < 1.0                                           # (tiles are dropped and tiles are kept)
    for name in ("table", "layer_start", "pool"):
        assert torch.equal(getattr(got, name), getattr(want, name)) and getattr(got, name).dtype == getattr(want, name).dtype, name
    with pytest.raises(ValueError):
        _new(m, s, b, layer_format='f32', sparse=True)


def test_3_the_result_goes_into_the_cube_viewer(model):
    import torch
    m, (s, b) = model, (32, 2)
    dense = _new(m, s, b)                                                    # (packed is the default)
    assert sorted(dense) == ["packed_layers"] and dense["packed_layers"].format == "rgba8"
    sparse = _new(m, s, b, sparse=True)["sparse_layers"]
    pose = np.tile(np.eye(4, dtype=F)[None, None], (b, 2, 1, 1))
    pos = np.zeros((b, 2, 3), F)
    pos[:, 1, 2] = 0.2
    rgb_d, dep_d = m.cube_render_views(dense["packed_layers"], pose, pos, size=(24, 48))
    rgb_s, dep_s = m.cube_render_views(sparse, pose, pos, size=(24, 48))
    assert bool((rgb_s == rgb_d).all()) and bool((dep_s == dep_d).all())
    assert bool(torch.isfinite(rgb_d).all()) and float(rgb_d.abs().max()) > 0


def test_4_two_layer_groups_with_a_whole_group_dropped(model):
    """Face 16, one cube, D = 8: the dense builder steps from one group's texels to the next, and the sparse builder meets a tile whose whole second
    group is dropped (it skips the group) next to tiles where that group is partly kept.  Same yardsticks as tests 1 and 2."""
    import torch
    m = model
    case = dict(TWO_GROUPS)
    s, b = case.pop("s"), case.pop("b")
    want = _three_launches(m, s, b, **case)
    assert bool(torch.isfinite(want).all()) and float(want[..., :3].abs().max()) > 0.1
    got = _new(m, s, b, case, layer_format=("f32", "rgba8"))
    assert _same_bits(got["rgba_layers"], want.permute(0, 2, 3, 1, 4))
    assert _same_bits(got["packed_layers"].data, _pack(m, want, "rgba8"))
    sparse = _new(m, s, b, case, layer_format="rgba8", sparse=True)["sparse_layers"]
    ref = m.sparsify_layers(got["packed_layers"], border='edge')
    for name in ("table", "layer_start", "pool"):
        assert torch.equal(getattr(sparse, name), getattr(ref, name)) and getattr(sparse, name).dtype == getattr(ref, name).dtype, name
    kept = (sparse.table >= 0).cpu().numpy()                 # [6, 8, S / 4, S / 16]
    assert kept.shape == (6, 8, s // 4, s // 16) and kept[:, 0].all()
    group1 = kept[:, 4:8].sum(axis=1)                          # kept layers of the second group, per tile
    assert (group1 == 0).any(), "no tile has its whole second group dropped"
    assert ((group1 > 0) & (group1 < 4)).any(), "no tile has its second group partly kept"
