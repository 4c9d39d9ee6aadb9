"""transmission_loss without a GPU: the ray-tube definition itself (its NumPy restatement in tests/tl_reference.py) against
the isovelocity image-source sum and against the closed form of a linear sound-speed gradient (a CPU-oracle fan), and the
argument errors refused before anything reaches the device."""
import math

import numpy as np
import pytest

import pygenray_amd as pr
from pygenray_amd.host_physics import bilinear_interp

import tl_reference as tlr

C0, H, ZS = 1500.0, 5000.0, 1000.0


def folded_fan(n_rays=20001, max_angle=80.0, ranges=np.linspace(0.0, 20e3, 201)):
    """Straight rays from (0, ZS) folded at the surface and the bottom: stored-convention (M, S) zs / ps."""
    th = np.linspace(-max_angle, max_angle, n_rays)
    u = ZS + ranges[None, :] * np.tan(np.radians(th))[:, None]          # unfolded depth
    w = np.mod(u, 2 * H)
    depth = np.where(w <= H, w, 2 * H - w)
    s = np.sin(np.radians(th))[:, None] / C0
    sign = np.where(np.mod(np.floor(u / H), 2) == 0, 1.0, -1.0)         # p flips at every reflection
    return th, -depth, -(s * sign), ranges


def test_restatement_matches_the_image_sum_in_an_isovelocity_waveguide():
    th, zs, ps, x = folded_fan()
    cin = np.full((2, 3), C0)
    rin, zin = np.array([-1.0, 30e3]), np.array([0.0, 3000.0, 6000.0])
    p0 = np.sin(np.radians(th)) / C0
    depths = np.arange(tlr.MARGIN, H - tlr.MARGIN + 1, 50.0)
    I = tlr.tube_intensity(zs, ps, x, p0, depths, cin, rin, zin)
    assert np.isnan(I[:, 0]).all()
    keep = (x >= 1e3) & (x <= 20e3)
    ref = tlr.image_intensity(x[keep], depths, ZS, H, 80.0)
    err = np.abs(tlr.to_db(I[:, keep]) - tlr.to_db(ref))
    assert err.max() < tlr.TOL_DB, err.max()
    # outside the water column no tube reaches: +inf
    out = tlr.tube_intensity(zs, ps, x, p0, np.array([-10.0, H + 10.0]), cin, rin, zin)
    assert (out[:, 1:] == 0).all()


def test_vectorised_bilinear_is_host_bilinear_interp_bit_for_bit():
    rng = np.random.default_rng(3)
    z = pr.eflat(np.arange(0, 5600, 2.0), 35.0)[0]
    r = np.linspace(0, 200e3, 33)
    cin = 1500 + rng.standard_normal((len(r), len(z)))
    x = np.concatenate([rng.uniform(-1e3, 201e3, 300), r[:5], [r[-1]]])
    y = np.concatenate([rng.uniform(-50, 5700, 300), z[:5], [z[-1]]])
    v = tlr.bilinear(x, y, r, z, cin)
    w = np.array([bilinear_interp(a, b, r, z, cin) for a, b in zip(x, y)])
    assert np.array_equal(v, w)


def _host_fan(n=4, S=5, source_depths=None, rs=None):
    th = np.linspace(-5, 5, n)
    r = np.linspace(0, 10e3, S)
    zs = -(1000.0 + np.outer(np.tan(np.radians(th)), r))
    ps = np.tile(np.sin(np.radians(th))[:, None] / 1500.0, (1, S))
    return pr.RayFan.from_arrays(th, np.tile(r, (n, 1)) if rs is None else rs, np.zeros((n, S)), zs, ps,
                                 np.zeros(n, np.int64), np.zeros(n, np.int64),
                                 np.full(n, 1000.0) if source_depths is None else source_depths)


@pytest.mark.parametrize("depths, msg", [([10.0, 5.0], "ascending"), ([10.0, 10.0], "ascending"), ([1.0, np.nan], "finite"),
                                         ([np.inf], "finite"), ([], "non-empty")])
def test_receiver_depths_are_checked(depths, msg):
    env = pr.OceanEnvironment2D(flat_earth_transform=False)
    with pytest.raises(ValueError, match=msg):
        pr.transmission_loss(_host_fan(), depths, env, flatearth=False)


def test_fans_that_cannot_form_tubes_are_refused():
    env = pr.OceanEnvironment2D(flat_earth_transform=False)
    with pytest.raises(ValueError, match="source depths"):
        pr.transmission_loss(_host_fan(source_depths=np.array([1000.0, 1000.0, 900.0, 1000.0])), [100.0], env, flatearth=False)
    rs = np.tile(np.linspace(0, 10e3, 5), (4, 1))
    rs[2, 3] += 1.0
    with pytest.raises(ValueError, match="rows of rays.rs differ"):
        pr.transmission_loss(_host_fan(rs=rs), [100.0], env, flatearth=False)
    with pytest.raises(ValueError, match="at least 2 rays"):
        pr.transmission_loss(_host_fan(n=1), [100.0], env, flatearth=False)


def test_flatearth_without_the_transform_is_refused_with_the_reference_message():
    env = pr.OceanEnvironment2D(flat_earth_transform=False)
    with pytest.raises(ValueError, match="Flat earth transformation has not been applied"):
        pr.transmission_loss(_host_fan(), [100.0], env)


def test_transmission_loss_is_exported():
    assert "transmission_loss" in pr.__all__ and callable(pr.transmission_loss)


# ---- a refracting medium: c = 1520 - 0.02 z, rays are circular arcs (tl_reference.linear_gradient_intensity) ------------

CA, GAMMA, ZS_G, AP = tlr.GRADIENT_CA, tlr.GRADIENT_GAMMA, tlr.GRADIENT_ZS, tlr.GRADIENT_APERTURE


def _oracle_gradient_fan():
    import oracle
    from helpers import y0_for
    env = tlr.gradient_env()
    arrs = pr._unpack_envi(env, flatearth=False)
    theta = np.linspace(-AP, AP, 2001)                                # depth-down (ODE convention)
    y0 = y0_for(oracle, arrs, ZS_G, 0.0, theta)
    o = oracle.shoot_fan(*arrs, y0, 0.0, tlr.GRADIENT_X1, tlr.GRADIENT_S)
    assert (o["status"] == 0).all()
    cin, _, rin, zin = arrs[:4]
    I = tlr.tube_intensity(-o["z"], -o["p"], o["r"], y0[:, 2], tlr.GRADIENT_DEPTHS, cin, rin, zin)
    return o, np.radians(theta), I


def test_closed_form_derivative_matches_mpmath():
    import mpmath
    mpmath.mp.dps = 40
    for r in (1e3, 7.5e3, 15e3):
        for t in np.radians([-8.0, -3.3, 0.0, 2.1, 8.0]):
            _, _, dz = tlr.linear_gradient_ray(r, float(t), ZS_G, CA, GAMMA, m=math)
            num = mpmath.diff(lambda u: tlr.linear_gradient_ray(r, u, ZS_G, CA, GAMMA, m=mpmath)[0], mpmath.mpf(float(t)))
            assert abs(dz - float(num)) <= 1e-9 * abs(float(num)), (r, t, dz, num)
    # and the isovelocity limit: I -> 1 / R^2
    I = tlr.linear_gradient_intensity([5e3], [1500.0], ZS_G, 1500.0, 1e-9, -8.0, 8.0)
    assert abs(I[0, 0] * (5e3 ** 2 + 500.0 ** 2) - 1) < 1e-6


def test_restatement_matches_the_linear_gradient_closed_form():
    o, theta0, I = _oracle_gradient_fan()
    worst, ref, inside = tlr.check_gradient_fan(o["r"], -o["z"], I, theta0, o["n_bott"], o["n_surf"])
    # measured: 1.49e-4 dB worst (median 1.8e-5) over 12 817 receivers inside the wedge
    assert worst < 2e-4
    # the test's power: the definition with c_s for c(d), or with cos(theta0) for cos(theta(r)), misses the bound >= 10x
    x = o["r"][o["r"] >= 1e3]
    c_s = CA + GAMMA * ZS_G
    _, th = tlr.linear_gradient_intensity(x, tlr.GRADIENT_DEPTHS, ZS_G, CA, GAMMA, -AP, AP, _solve=True)
    th = np.where(inside, th, 0.0)
    k_r = tlr.linear_gradient_ray(x[None, :], th, ZS_G, CA, GAMMA)[1]
    Ik = I[:, o["r"] >= 1e3][inside]
    for wrong in (ref * c_s / (CA + GAMMA * tlr.GRADIENT_DEPTHS[:, None]), ref * k_r / np.cos(th)):
        miss = np.abs(tlr.to_db(Ik) - tlr.to_db(wrong[inside])).max()
        assert miss > 10 * tlr.TOL_DB_GRADIENT, miss
