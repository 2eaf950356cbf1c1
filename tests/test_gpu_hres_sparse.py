"""MSI.hres_layers_sparse / msi_hres_index_tiles / msi_hres_layers_sparse: the high-res stack built sparse, without the dense
stack.  The yardstick is the path that existed before: sparsify_layers(hres_layers(layer_format=fmt)['packed_layers']) on the
device and sparse.sparsify_np of the dense codes on the host -- never the new code -- and every comparison is on raw bits: there is
no tolerance anywhere in this file.  Inputs: tests/hres_sparse_cases.py."""
import numpy as np
import pytest

from matryodshka_amd import sparse as S
from tests import hres_sparse_cases as cases
from tests.test_gpu_hres_layers import _rot

pytestmark = pytest.mark.gpu

BASE = cases.SHAPES[0]                     # low 16x32 -> high 40x96 (non-integer scale), D = 8


@pytest.fixture(scope="module")
def model():
    from matryodshka_amd import MSI
    return MSI()


def _with_poses(x, poses):
    b = x["bw"].shape[0]
    x = dict(x)
    if poses == "equal":                   # ref_pose == src_pose (not the identity): the shared-quadratic path
        x["ref_pose"] = np.stack([_rot(0, 0.15, (0.01, 0.0, 0.02)), _rot(1, -0.3, (0.0, 0.02, 0.0))])[:b]
        x["src_pose"] = x["ref_pose"].copy()
        x["ref_pose_inv"] = np.tile(np.eye(4, dtype=np.float32)[None], (b, 1, 1))
    else:                                  # a translated and a rotated + translated source pose: two quadratics
        x["src_pose"] = np.stack([_rot(1, 0.0, (0.03, -0.01, 0.02)), _rot(1, 0.2, (-0.02, 0.015, 0.01))])[:b]
    return x


def _call(m, x, fmt, sparse=False):
    """MSI.hres_layers, or MSI.hres_layers_sparse on the same arguments."""
    planes = m.inv_depths(1.0, 100.0, x["d"])
    fn = m.hres_layers_sparse if sparse else m.hres_layers
    return fn(x["bw"], x["al"], x["ref"], x["src"], x["ref_pose"], x["src_pose"], planes, x["intr"],
              ref_pose_inv=x["ref_pose_inv"], layer_format=fmt)


def _dense(m, x, fmt):
    return _call(m, x, fmt)["packed_layers"]


def _sparse(m, x, fmt):
    out = _call(m, x, fmt, sparse=True)
    assert sorted(out) == ["sparse_layers"] and isinstance(out["sparse_layers"], S.SparseLayers)
    return out["sparse_layers"]


def _words(t):
    import torch
    t = t.contiguous()
    return t.view({8: torch.int64, 4: torch.int32, 2: torch.int16, 1: torch.uint8}[t.element_size()])


def _assert_same_stack(got, want):
    """table, layer_start and pool on raw words; format, shape and planes."""
    import torch
    assert got.format == want.format and got.shape == want.shape and got.planes == want.planes
    for name in ("table", "layer_start", "pool"):
        a, b = getattr(got, name), getattr(want, name)
        assert a.dtype == b.dtype and a.shape == b.shape, name
        assert torch.equal(_words(a), _words(b.to(a.device))), name


def _check(m, x, fmt, masks=True):
    """hres_layers_sparse against sparsify_layers of the dense request and sparsify_np of its codes; returns (sparse, dense)."""
    pk = _dense(m, x, fmt)
    want = m.sparsify_layers(pk)
    table, layer_start, pool = S.sparsify_np(pk.data.cpu().numpy(), fmt)
    occ = float((table >= 0).mean())
    print("%s %s: occupancy %.3f, %d tiles" % (tuple(pk.data.shape), fmt, occ, pool.shape[0]))
    if masks:
        assert cases.check_masks(table >= 0) == occ
    else:
        assert 0.2 <= occ <= 0.8, occ
    got = _sparse(m, x, fmt)
    assert got.planes == tuple(float(p) for p in m.inv_depths(1.0, 100.0, x["d"]))
    _assert_same_stack(got, want)
    _assert_same_stack(got, S.SparseLayers(table, layer_start, pool, fmt, got.planes))
    return got, pk


# 1 ---------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("poses", ["equal", "different"])
@pytest.mark.parametrize("fmt", cases.FORMATS)
@pytest.mark.parametrize("shape", cases.SHAPES, ids=cases.SHAPE_IDS)
def test_1_sparse_request_has_the_bits_of_sparsify_of_the_dense_request(model, shape, fmt, poses):
    _check(model, _with_poses(cases.case(shape), poses), fmt)


# 2 ---------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("fmt", cases.FORMATS)
@pytest.mark.parametrize("shape", [cases.SHAPES[0], cases.SHAPES[4]], ids=[cases.SHAPE_IDS[0], cases.SHAPE_IDS[4]])
def test_2_index_tiles_from_alphas_equals_index_tiles_of_the_dense_codes(model, shape, fmt):
    import torch
    from matryodshka_amd import _native as N
    m = model
    x = cases.case(shape)
    h, w, hh, hw, d = shape
    b = cases.B
    codes = _dense(m, x, fmt).data
    f = m.LAYER_FORMATS[fmt]

    def tables():
        return (torch.full((b, d, hh // 4, hw // 16), -7, dtype=torch.int32, device=m.device),
                torch.full((b * d,), -7, dtype=torch.int32, device=m.device))
    t_want, c_want = tables()
    N.check(N.lib.msi_sparse_index_tiles(codes.data_ptr(), f, b, d, hh, hw, t_want.data_ptr(), c_want.data_ptr(), m._stream()), "sparse_index_tiles")
    t_got, c_got = tables()
    al = m._f32(x["al"])
    N.check(N.lib.msi_hres_index_tiles(al.data_ptr(), f, b, h, w, hh, hw, d, t_got.data_ptr(), c_got.data_ptr(), m._stream()), "hres_index_tiles")
    torch.cuda.synchronize()
    cases.check_masks((t_want >= 0).cpu().numpy())
    assert torch.equal(t_got, t_want) and torch.equal(c_got, c_want)
    assert int(c_got.min()) == 0 and int(c_got.max()) == (hh // 4) * (hw // 16)


# 3 ---------------------------------------------------------------------------------------------------------------------
def _odd_alphas(x):
    """Low-res values the encoders treat differently, in blocks of layer 1 (empty in the plain case) and one NaN in a rectangle layer:
    -0.0 and 1e-9 (zero in both formats: 1e-9 underflows in fp16 and rounds to code 0), a negative (code 0 in rgba8, a negative
    half in rgba16f), 1.5 (clamped to 255 / stored as 1.5), NaN (code 0 in rgba8: fmaxf drops it; a NaN half in rgba16f)."""
    x = dict(x)
    al = x["al"].copy()
    al[:, 0:3, 0:6, 1] = -0.0
    al[:, 0:3, 8:14, 1] = 1e-9
    al[:, 6:9, 0:6, 1] = -0.25
    al[:, 6:9, 16:22, 1] = 1.5
    al[0, 12, 12, 1] = np.nan
    al[1, 5, 20, 5] = np.nan
    x["al"] = al
    return x


def test_3_odd_alphas_land_where_the_stored_codes_put_them(model):
    import torch
    x = _odd_alphas(_with_poses(cases.case(BASE), "different"))
    tables = {}
    for fmt in cases.FORMATS:
        got, _ = _check(model, x, fmt, masks=False)
        tables[fmt] = got.table[:, 1] >= 0
    # the inputs bite: layer 1 keeps tiles, and the negative and the NaN block keep tiles in rgba16f only
    assert bool(tables["rgba8"].any()) and not bool(tables["rgba8"].all())
    assert bool((tables["rgba16f"] & ~tables["rgba8"]).any()) and not bool((tables["rgba8"] & ~tables["rgba16f"]).any())
    assert not torch.equal(tables["rgba16f"][0], tables["rgba16f"][1])           # (sample 0 alone has the NaN in layer 1)


@pytest.mark.parametrize("fmt", cases.FORMATS)
def test_3b_alphas_around_the_smallest_stored_value(model, fmt):
    """Layer 1 ramps across the format's threshold between "stored as zero" and "stored as the smallest code" (rgba8: 0.5 / 255;
    rgba16f: 2^-25), left to right: dropped tiles on the left, kept ones on the right, and in between the tiles whose fate only
    the texels themselves decide.  Layer 5 holds the same ramp with the sign flipped: empty in rgba8, mirrored in rgba16f."""
    x = _with_poses(cases.case(BASE), "different")
    h, w = BASE[:2]
    t = {"rgba8": 0.5 / 255, "rgba16f": 2.0 ** -25}[fmt]
    ramp = (t * (0.9 + 0.2 * np.arange(w, dtype=np.float64) / (w - 1))).astype(np.float32)
    al = x["al"].copy()
    al[:, :, :, 1] = ramp[None, None, :]
    al[:, :, :, 5] = -ramp[None, None, :]
    x["al"] = al
    got, _ = _check(model, x, fmt, masks=False)
    kept = (got.table[:, 1] >= 0).cpu().numpy()
    # (tile column 0 is kept through the wrap: its window holds x = Wh - 1, the top of the ramp; column 1 sees <= 0.97 of the threshold)
    assert kept[:, :, 0].all() and not kept[:, :, 1].any() and kept[:, :, -2].all() and kept[:, :, -1].all()
    kept5 = (got.table[:, 5] >= 0).cpu().numpy()
    assert (not kept5.any()) if fmt == "rgba8" else np.array_equal(kept5, kept)


# 4 ---------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("fmt", cases.FORMATS)
def test_4_renders_from_the_result_are_the_renders_of_the_dense_stack(model, fmt):
    import torch
    from tests.test_gpu_sparse_layers import _cameras, _poses
    m = model
    x = _with_poses(cases.case(BASE), "different")
    sp, pk = _sparse(m, x, fmt), _dense(m, x, fmt)
    _, _, hh, hw, _ = BASE
    pose, pos = _poses(71, cases.B, 2)
    m.render_status()
    cams = _cameras(hh, hw)
    for name in ("equirect", "pinhole_odd"):
        rgb_s, dep_s = m.render_views(sp, pose, pos, **cams[name])               # (planes: the ones each stack carries)
        rgb_d, dep_d = m.render_views(pk, pose, pos, **cams[name])
        assert tuple(rgb_s.shape[2:4]) == ((hh, hw) if name == "equirect" else (hh + 7, hw + 37))
        assert bool((rgb_s == rgb_d).all()) and bool((dep_s == dep_d).all()), name
        assert float(rgb_s.abs().max()) > 0
    kw = dict(baseline=np.array([0.032, 0.06], np.float32), tgt_pose_rt=pose[:, 0], tgt_pos=pos[:, 0], size=(hh + 7, hw + 37))
    rgb_s, dep_s = m.render_ods_pair(sp, want_depth=True, **kw)
    rgb_d, dep_d = m.render_ods_pair(pk, want_depth=True, **kw)
    assert bool((rgb_s == rgb_d).all()) and bool((dep_s == dep_d).all())
    assert not torch.equal(rgb_s[:, 0], rgb_s[:, 1])                             # two eyes
    torch.cuda.synchronize()
    assert m.render_status() == 0
    # ... and densify_layers expands it to what the sparsified dense stack expands to
    assert torch.equal(_words(m.densify_layers(sp).data), _words(m.densify_layers(m.sparsify_layers(pk)).data))


def test_4b_result_round_trips_through_a_file(model, tmp_path):
    import torch
    x = cases.case(BASE)
    sp = _sparse(model, x, "rgba16f")
    path = str(tmp_path / "hres_sparse.npz")
    sp.save(path)
    back = S.SparseLayers.load(path)
    _assert_same_stack(back, sp.to("cpu"))
    assert torch.equal(_words(model.densify_layers(back).data), _words(model.densify_layers(sp).data))


# 5 ---------------------------------------------------------------------------------------------------------------------
def test_5_no_dense_stack_is_allocated(model):
    """256 x 512 x 32 from 16 x 32: the peak rise of the sparse request against that of the dense rgba8 request in the same
    process.  rise_sparse <= rise_dense - dense_bytes + result.nbytes + 1 MiB: the MiB covers the counts, the prefix sum and
    allocator rounding; everything else (images, poses, low-res tensors on the device) cancels."""
    import torch
    m = model
    shape = (16, 32, 256, 512, 32)
    x = cases.case(shape, b=1, tile_from=(64, 128))
    _, _, hh, hw, d = shape
    warm = _sparse(m, x, "rgba8")                             # (trig table, planes: cached by the model)
    assert 0.2 <= warm.occupancy <= 0.6, warm.occupancy
    nbytes = warm.nbytes
    del warm
    rise = {}
    for which in ("dense", "sparse"):
        torch.cuda.synchronize()
        torch.cuda.empty_cache()
        torch.cuda.reset_peak_memory_stats()
        before = torch.cuda.memory_allocated()
        out = _dense(m, x, "rgba8") if which == "dense" else _sparse(m, x, "rgba8")
        torch.cuda.synchronize()
        rise[which] = torch.cuda.max_memory_allocated() - before
        assert out.nbytes == (4 * d * hh * hw if which == "dense" else nbytes)
        del out
    dense_bytes = 4 * d * hh * hw
    print("hres_layers rgba8 at %dx%dx%d: peak rise dense %.2f MB, sparse %.2f MB (dense stack %.2f MB, sparse result %.2f MB)" % (
        hw, hh, d, rise["dense"] / 1e6, rise["sparse"] / 1e6, dense_bytes / 1e6, nbytes / 1e6))
    assert 0 < rise["sparse"] <= rise["dense"] - dense_bytes + nbytes + (1 << 20), rise


# 6 ---------------------------------------------------------------------------------------------------------------------
def test_6_non_temporal_pool(model):
    """An rgba8 pool just over 256 MiB (2080 x 4096 x 8 x 4 B = 260 MiB at occupancy 1: alphas >= 0.05 everywhere): the
    non-temporal form of the texel pass.  The pool is the dense codes regrouped into tiles."""
    import torch
    shape = (16, 32, 2080, 4096, 8)
    h, w, hh, hw, d = shape
    x = cases.case(shape, b=1, tile_from=(65, 128))
    rng = np.random.RandomState(77)
    x["al"] = (0.05 + 0.9 * rng.uniform(size=(1, h, w, d))).astype(np.float32)
    sp = _sparse(model, x, "rgba8")
    assert sp.occupancy == 1.0 and sp.pool.numel() > 256 << 20
    per_layer = (hh // 4) * (hw // 16)
    assert torch.equal(sp.layer_start.cpu(), torch.arange(d + 1, dtype=torch.int64) * per_layer)
    assert torch.equal(sp.table.reshape(d, per_layer).cpu(), torch.arange(per_layer, dtype=torch.int32)[None].expand(d, per_layer))
    codes = _dense(model, x, "rgba8").data                                       # [1,D,Hh,Wh,4]
    tiles = codes.view(1, d, hh // 4, 4, hw // 16, 16, 4).permute(0, 1, 2, 4, 3, 5, 6).reshape(-1, 4, 16, 4)
    assert torch.equal(sp.pool, tiles)
    del sp, codes, tiles
    torch.cuda.empty_cache()


# 7 ---------------------------------------------------------------------------------------------------------------------
def test_7_refusals_and_the_default(model):
    """hres_layers_sparse refuses what it cannot build; hres_layers itself is what it was (its parameter list is pinned in
    tests/test_hres_layers_abi.py) and returns exactly its keys."""
    x = cases.case(BASE)
    for fmt in ("f32", ("f32", "rgba8")):
        with pytest.raises(ValueError):
            _call(model, x, fmt, sparse=True)
    for shape in ((16, 32, 10, 96, 8), (16, 32, 40, 40, 8)):                     # Hh = 10, Wh = 40
        with pytest.raises(ValueError):
            _call(model, cases.case(shape), "rgba8", sparse=True)
    from matryodshka_amd import MSI
    with pytest.raises(ValueError):
        _call(MSI(input_type="PP"), x, "rgba8", sparse=True)
    assert sorted(_call(model, x, "rgba8", sparse=False)) == ["packed_layers"]
    assert sorted(_call(model, x, ("f32", "rgba16f"), sparse=False)) == ["packed_layers", "rgba_layers"]
    assert sorted(_call(model, x, "f32")) == ["rgba_layers"]
