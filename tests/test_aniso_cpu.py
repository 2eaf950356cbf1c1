"""CPU facts of the anisotropic texel rule (include/msi_hip.h, msi_render_views_aniso) on its fp64 statement alone
(tests/aniso_reference.py): its limits -- the trilinear render away from the poles, the plain render's bits where nothing is
minified --, its weights and sample counts, its continuity, and the reason the feature exists: near the stack's poles a tilted view
is about twice as close to the supersampled view as the trilinear one.  Nothing here loads the native library."""
import numpy as np
import pytest

from matryodshka_amd import mips as M
from tests import aniso_reference as A
from tests import mip_reference as R

F = np.float32
PLANES = [100.0, 3.0, 1.5, 1.0]
I4 = np.eye(4, dtype=F)


def tilt(deg):
    """Rotation by `deg` in the (1, 2) plane: the view's poles leave the stack's."""
    a = np.deg2rad(deg)
    c, s = np.cos(a), np.sin(a)
    P = np.eye(4)
    P[1, 1], P[1, 2], P[2, 1], P[2, 2] = c, -s, s, c
    return P.astype(F)


def _pyramid(base, levels):
    return [base] + [x[0] for x in M.build_mips_np(base[None], 'f32', levels)]


@pytest.fixture(scope="module")
def stack():
    base = R.near_nyquist_stack(3)
    return base, _pyramid(base, 4)


def rms(a, b, mask=None):
    d = (a - b) ** 2
    return float(np.sqrt(np.mean(d[mask] if mask is not None else d)))


def test_away_from_the_poles_it_is_the_trilinear_render(stack):
    """Identity pose, equirect camera, 16 x 32 of the 64 x 128 x 4 stack: the footprint's axes are the image axes and sigma_max is
    the trilinear rule's rho.  With one sample (max_anisotropy = 1) the two renders agree to 1e-7 (measured 3.5e-9: what is left is
    lambda from sigma_max against lambda from the longer column).  With max_anisotropy = 8 the footprint is a 4 x 4 square up to
    the rounding of the fp32 trig tables behind the hits -- 6e-8 of a coordinate of up to 128 texels, i.e. up to 1e-5 texels in a
    difference -- so ratio - 1, the weights of the samples +-1 and lambda move by that order, each times a texel difference of order
    1: bound 1e-5, measured 2.6e-7."""
    base, pyr = stack
    tri, tri_d = R.mip_view(pyr, I4, (0, 0, 0), PLANES, size=(16, 32))
    for cap, bound in ((1.0, 1e-7), (8.0, 1e-5)):
        an, an_d, ratio, lam = A.aniso_view(pyr, I4, (0, 0, 0), PLANES, size=(16, 32), max_anisotropy=cap, details=True)
        print("aniso (cap %g) vs trilinear, identity pose: rgb %.3g depth %.3g, largest ratio - 1 %.3g" % (
            cap, np.abs(an - tri).max(), np.abs(an_d - tri_d).max(), ratio.max() - 1.0))
        assert np.abs(an - tri).max() <= bound and np.abs(an_d - tri_d).max() <= bound


@pytest.mark.parametrize("cap", [1.0, 2.0, 16.0])
def test_nothing_minified_has_the_plain_renders_bits(stack, cap):
    """sigma_max <= 1 on every layer (identity pose, an output twice the stack's size): one sample of weight 1 at level 0."""
    base, pyr = stack
    an, an_d, ratio, lam = A.aniso_view(pyr, I4, (0, 0, 0), PLANES, size=(128, 256), max_anisotropy=cap, details=True)
    plain, plain_d = R.mip_view([base], I4, (0, 0, 0), PLANES, size=(128, 256))
    assert np.all(ratio == 1.0) and np.all(lam == 0.0)
    assert np.array_equal(an, plain) and np.array_equal(an_d, plain_d)
    # and so has any view with lod_bias <= -64, and the cap 1 at a bias that keeps lambda at 0
    an, an_d = A.aniso_view(pyr, tilt(90), (0.3, -0.2, 0.25), PLANES, size=(7, 13), max_anisotropy=cap, lod_bias=-64.0)
    plain, plain_d = R.mip_view([base], tilt(90), (0.3, -0.2, 0.25), PLANES, size=(7, 13))
    assert np.array_equal(an, plain) and np.array_equal(an_d, plain_d)


@pytest.mark.parametrize("cap", [1.0, 1.5, 2.0, 3.0, 4.0, 7.0, 8.0, 16.0])
def test_weights_sum_to_one_and_the_sample_count_is_bounded(cap):
    ratio = np.concatenate([np.linspace(1.0, cap, 1001), np.minimum(np.arange(1.0, 17.0), cap)])
    Mx = A.sample_count(ratio)
    most = 2 * int(np.ceil((cap - 1) / 2)) + 1
    assert np.all(2 * Mx + 1 <= most) and most <= 17
    total = sum(np.where(abs(m) <= Mx, A.weight(ratio, m), 0.0) for m in range(-8, 9))
    assert np.abs(total - 1.0).max() <= 1e-12
    # the outermost weight vanishes exactly where M changes (ratio = 2 M + 1), and no sample beyond M has any weight
    for m in range(1, 9):
        assert A.weight(np.array([2.0 * m - 1.0]), m)[0] == 0.0
        assert np.all(A.weight(ratio, m)[Mx < m] == 0.0)


def test_the_sign_of_the_axis_does_not_matter_and_the_axis_only_where_ratio_exceeds_1(stack, monkeypatch):
    """The samples are symmetric about the hit: with the axis negated the view is the same up to the order of the sum; with the
    axis turned by 90 degrees only pixels with ratio > 1 on some layer change."""
    base, pyr = stack
    args = (pyr, tilt(60), (0.3, -0.2, 0.25), PLANES)
    want, _, ratio, _ = A.aniso_view(*args, size=(12, 24), details=True)
    footprint = A.footprint

    def negated(*a):
        ratio, lam, step, mu_u, mu_v = footprint(*a)
        return ratio, lam, step, -mu_u, -mu_v

    def turned(*a):
        ratio, lam, step, mu_u, mu_v = footprint(*a)
        return ratio, lam, step, -mu_v, mu_u
    monkeypatch.setattr(A, "footprint", negated)
    assert np.abs(A.aniso_view(*args, size=(12, 24))[0] - want).max() <= 1e-14
    monkeypatch.setattr(A, "footprint", turned)
    changed = np.abs(A.aniso_view(*args, size=(12, 24))[0] - want).max(axis=-1) > 0
    assert changed.any() and not np.any(changed & (ratio.max(axis=0) == 1.0))


def test_one_level_is_still_filtered_along_the_major_axis(stack):
    """mips = NULL: lambda is 0 everywhere, and a tilted view still takes its samples along the major axis at level 0."""
    base, pyr = stack
    an, _, ratio, lam = A.aniso_view([base], tilt(90), (0, 0, 0), PLANES, size=(16, 32), details=True)
    plain, _ = R.mip_view([base], tilt(90), (0, 0, 0), PLANES, size=(16, 32))
    assert np.all(lam == 0.0) and ratio.max() == 8.0 and np.abs(an - plain).max() > 0.05


@pytest.mark.parametrize("size", [(16, 32), (32, 64)])
@pytest.mark.parametrize("pos", [(0.0, 0.0, 0.0), (0.3, -0.2, 0.25)])
def test_anisotropic_is_closer_to_the_supersampled_view_than_trilinear(stack, size, pos):
    """The quality fact, on the fp64 reference alone: a view tilted by 90 degrees of the 64 x 128 x 4 near-Nyquist stack, against
    its 8 x 8 supersampled render, max_anisotropy = 8.  On the pixels whose ratio reaches 2 on some layer the anisotropic RMS error
    is at most 0.6 of the trilinear one; on the whole image it is no larger.  Measured (share of masked pixels; masked trilinear
    RMS, anisotropic RMS, their quotient; whole-image trilinear, anisotropic):
        16 x 32  centre      0.434   0.0947  0.0398  0.420   0.0684  0.0469        16 x 32  translated  0.512   0.0860  0.0382  0.444   0.0674  0.0477
        32 x 64  centre      0.404   0.1030  0.0465  0.452   0.0887  0.0514        32 x 64  translated  0.407   0.0927  0.0430  0.463   0.0805  0.0469
    (max_anisotropy = 2 at 16 x 32, centre: 0.83 -- the bound of 0.6 bites; 4 and 16 give what 8 gives on this content.)"""
    base, pyr = stack
    P = tilt(90)
    sup, _ = R.supersampled_view(base, P, pos, PLANES, 'equirect', size)
    tri, _ = R.mip_view(pyr, P, pos, PLANES, size=size)
    an, _, ratio, lam = A.aniso_view(pyr, P, pos, PLANES, size=size, max_anisotropy=8.0, details=True)
    mask = ratio.max(axis=0) >= 2.0
    print("size %s pos %s: masked %.3f | masked trilinear %.4f anisotropic %.4f quotient %.3f | whole %.4f %.4f" % (
        size, pos, mask.mean(), rms(tri, sup, mask), rms(an, sup, mask), rms(an, sup, mask) / rms(tri, sup, mask), rms(tri, sup), rms(an, sup)))
    assert mask.mean() >= 0.3                                     # the test is not vacuous
    assert rms(an, sup, mask) <= 0.6 * rms(tri, sup, mask)
    assert rms(an, sup) <= rms(tri, sup)


def test_the_rule_is_continuous_in_the_ray(stack):
    """200 steps of 0.01 degrees from a tilt of 60 degrees, 12 x 24 outputs: the largest change of any pixel in one step is at most
    twice the median over the steps (measured 1.2: no step stands out, so M, the level and the axis change without a jump)."""
    base, pyr = stack
    prev, jumps = None, []
    for k in range(201):
        an, _ = A.aniso_view(pyr, tilt(60 + 0.01 * k), (0.1, 0.0, 0.1), PLANES, size=(12, 24))
        if prev is not None:
            jumps.append(float(np.abs(an - prev).max()))
        prev = an
    print("per-step change over %d steps: max %.4g median %.4g quotient %.2f" % (len(jumps), max(jumps), np.median(jumps), max(jumps) / np.median(jumps)))
    assert max(jumps) <= 2.0 * np.median(jumps)
