"""CPU checks of the seamless cube filter: the fp64 reference (tests/cube_seamless_reference.py) by itself, its geometry-built
virtual-texel table against the package's closed form (cubemap.virtual_texel, the twin of the kernel's selects), and what the
rule buys: continuity across cube edges and a smaller error of a panorama round trip.  No device."""
import functools

import numpy as np
import pytest

from tests import cube_reference as ref
from tests import cube_seamless_reference as sref

FRONT, RIGHT, BACK, LEFT, UP, DOWN = range(6)
ONE = {frozenset(e) for e in [(FRONT, RIGHT), (RIGHT, BACK), (BACK, LEFT), (LEFT, FRONT), (FRONT, UP), (FRONT, DOWN), (UP, RIGHT), (DOWN, LEFT)]}
NONE = {frozenset(e) for e in [(RIGHT, DOWN), (BACK, DOWN)]}
TWICE = {frozenset(e) for e in [(UP, BACK), (UP, LEFT)]}
EYE = np.eye(4)


def _k(s):
    return np.array([[s / 2, 0, s / 2], [0, s / 2, s / 2], [0, 0, 1]], np.float64)


def _rot(ax, ang):
    ax = np.asarray(ax, np.float64) / np.linalg.norm(ax)
    k = np.array([[0, -ax[2], ax[1]], [ax[2], 0, -ax[0]], [-ax[1], ax[0], 0]])
    p = np.eye(4)
    p[:3, :3] = np.eye(3) + np.sin(ang) * k + (1 - np.cos(ang)) * (k @ k)
    return p


@pytest.mark.parametrize("camera,size", [("equirect", (17, 40)), ("pinhole", (12, 20))])
def test_with_the_rule_off_the_reference_is_the_clamp_reference(camera, size):
    rng = np.random.RandomState(3)
    s, d = 8, 3
    stack = rng.uniform(-1, 1, size=(6, s, s, d, 4))
    stack[..., 3] = rng.uniform(0.05, 0.95, size=stack.shape[:-1])
    pose = _rot((1, 2, 3), 0.7)
    pose[:3, 3] = (0.2, -0.15, 0.25)
    kt = np.array([[9.0, 0, 10.4], [0, 10.0, 5.6], [0, 0, 1]]) if camera == "pinhole" else None
    args = (stack, [50.0, 5.0, 1.0], _k(s), pose, (0.1, 0.2, -0.15), camera, size, kt)
    want = ref.render_view(*args)
    got = sref.render_view(*args, seamless=False)
    assert np.abs(got["rgb"] - want["rgb"]).max() <= 1e-12 and np.abs(got["depth"] - want["depth"]).max() <= 1e-12
    assert np.array_equal(got["margin"], want["margin"])
    assert np.array_equal(got["strip"] > 0, want["clamped"] & (got["strip"] > 0)) and not got["corner"].any()
    on = sref.render_view(*args)
    assert np.abs(on["rgb"] - want["rgb"]).max() > 1e-3          # (the rule does something)
    inside = on["strip"] <= 0
    assert inside.any() and np.abs(on["rgb"] - want["rgb"])[inside].max() <= 1e-12


@pytest.mark.parametrize("s", [8, 12])
def test_the_twelve_edges_fall_into_the_three_classes(s):
    classes = sref.edge_classes(s)
    assert len(classes) == 12
    assert {e for e, n in classes.items() if n == 1} == ONE
    assert {e for e, n in classes.items() if n == 0} == NONE
    assert {e for e, n in classes.items() if n == 2} == TWICE
    # the virtual texels of the table say the same: one fetch across a once-stored edge, a two-face mean across an unstored one, and
    # no face ever asks across a twice-stored edge (neither of its faces has it on an open side)
    asked = {}
    for (f, x, y), ent in sref.virtual_table(s).items():
        if 0 < x < s or 0 < y < s:                         # an edge point, not a corner
            if len(ent) == 1:
                asked.setdefault(frozenset((f, ent[0][0])), set()).add(1)
            else:
                assert len(ent) == 2 and ent[0][0] == f and ent[0][3] == ent[1][3] == 0.5
                asked.setdefault(frozenset((f, ent[1][0])), set()).add(2)
    assert {e for e, n in asked.items() if n == {1}} == ONE and {e for e, n in asked.items() if n == {2}} == NONE
    assert set(asked) == ONE | NONE


@pytest.mark.parametrize("s", [4, 8, 12])
def test_the_closed_form_is_the_geometry_built_table(s):
    from matryodshka_amd import cubemap
    table = sref.virtual_table(s)
    assert len(table) == 6 * (2 * s + 1)
    threes = 0
    for (f, x, y), want in table.items():
        got = cubemap.virtual_texel(f, x, y, s)
        assert [e[:3] for e in got] == [e[:3] for e in want], (f, x, y, got, want)
        assert np.allclose([e[3] for e in got], [e[3] for e in want], rtol=0, atol=1e-15)
        assert all(0 <= g < 6 and 0 <= gx < s and 0 <= gy < s for g, gx, gy, _ in got)
        threes += len(got) == 3
    assert threes == 9                                      # the three cube corners no face stores, seen from three faces each
    for f in range(6):
        for y in range(s):
            for x in range(s):
                assert cubemap.virtual_texel(f, x, y, s) == [(f, x, y, 1.0)]
    for bad in [(6, 0, 0), (-1, 0, 0), (0, s + 1, 0), (0, 0, -1)]:
        with pytest.raises(ValueError):
            cubemap.virtual_texel(*bad, s)


def test_every_face_that_sees_a_corner_agrees_on_its_value():
    """The three-face rule: at a cube corner no face stores, every face whose virtual texel it is averages the same three texels."""
    s = 8
    by_point = {}
    for (f, x, y), ent in sref.virtual_table(s).items():
        if len(ent) == 3:
            p = tuple(np.rint(sref.cube_point(f, x, y, s)).astype(int))
            by_point.setdefault(p, []).append(sorted(e[:3] for e in ent))
    assert sorted(by_point) == [(-1, 1, -1), (1, 1, -1), (1, 1, 1)]
    for p, sets in by_point.items():
        assert len(sets) == 3 and all(t == sets[0] for t in sets), (p, sets)


def test_a_cube_of_six_equal_faces_renders_as_clamp():
    rng = np.random.RandomState(5)
    s, d = 8, 2
    face = rng.uniform(-1, 1, size=(d, 4))
    face[:, 3] = (0.7, 0.4)
    stack = np.tile(face[None, None, None], (6, s, s, 1, 1))        # every texel of layer l is face[l]: six equal faces per layer
    pose = _rot((3, -1, 2), -1.1)
    pose[:3, 3] = (-0.25, 0.2, 0.1)
    args = (stack, [5.0, 1.0], _k(s), pose, (0.15, -0.1, 0.2), "equirect", (24, 48))
    on, off = sref.render_view(*args), sref.render_view(*args, seamless=False)
    assert (on["strip"] > 0).any() and on["corner"].any()
    assert np.abs(on["rgb"] - off["rgb"]).max() <= 1e-12 and np.abs(on["depth"] - off["depth"]).max() <= 1e-12


@functools.lru_cache(maxsize=None)
def constant_faces_steps(size):
    """(largest neighbour step of the seamless render, of the clamp render) of the six constant faces from the centre.
    S = 8: the seamless ramp between two faces is one texel wide, and a texel at a face's edge (tan = 1) subtends (2/S) / 2 rad
    = 10.2 pixels of a 512-wide panorama, so the step between neighbouring pixels is at most 2 sqrt(2) / 10.2 = 0.28 of a colour
    difference of 2 (sqrt(2): a pixel step that crosses the ramp diagonally near a corner); clamp steps by the full 2."""
    s = 8
    stack = sref.constant_faces(s, sref.CONSTANT_COLOURS)
    args = (stack, [1.0], _k(s), EYE, (0, 0, 0), "equirect", size)
    on, off = sref.render_view(*args), sref.render_view(*args, seamless=False)
    return sref.largest_neighbour_step(on["rgb"]), sref.largest_neighbour_step(off["rgb"])


def test_constant_faces_are_continuous_across_the_edges():
    on, off = constant_faces_steps((256, 512))
    print("six constant faces (2, 3, 4 equal), 256 x 512: largest neighbour step seamless %.4f, clamp %.4f" % (on, off))
    assert on < 0.25 * off


@pytest.mark.parametrize("s", [16, 32])
def test_panorama_round_trip(s):
    stack = sref.analytic_cube(s)
    size = (64, 128)
    args = (stack, [1.0], _k(s), EYE, (0, 0, 0), "equirect", size)
    _, rays = ref.target_rays("equirect", size, EYE, (0, 0, 0))
    truth = sref.analytic_panorama(rays)
    err = {name: np.abs(sref.render_view(*args, seamless=flag)["rgb"] - truth) for name, flag in (("seamless", True), ("clamp", False))}
    mx = {n: e.max() for n, e in err.items()}
    p99 = {n: np.percentile(e, 99) for n, e in err.items()}
    print("panorama round trip S = %d: max abs error seamless %.4f clamp %.4f; 99th percentile seamless %.4f clamp %.4f (x%.2f)"
          % (s, mx["seamless"], mx["clamp"], p99["seamless"], p99["clamp"], p99["seamless"] / p99["clamp"]))
    assert mx["seamless"] < mx["clamp"]
    assert p99["seamless"] <= 0.5 * p99["clamp"]
