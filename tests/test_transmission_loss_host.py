"""transmission_loss without a GPU: the ray-tube definition itself (its NumPy restatement in tests/tl_reference.py) against
the isovelocity image-source sum, and the argument errors refused before anything reaches the device."""
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
