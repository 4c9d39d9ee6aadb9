"""transmission_loss on the GPU (csrc/pgr_tl.h): the isovelocity image sum end to end, bit parity with the NumPy
restatement of tests/tl_reference.py on both trajectory layouts, one answer whatever the path, and the edges."""
import numpy as np
import pytest

import tl_reference as tlr

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module")
def pr():
    from pygenray_amd import _lib
    if _lib.ARITH != "reference":
        pytest.skip("bit parity is claimed for the reference arithmetic only (PGR_ARITH=contracted: tests/test_contracted_arith.py)")
    _lib.load()
    assert _lib.device_count() >= 1
    import pygenray_amd
    return pygenray_amd


def _env(pr, z, r, cin, br, bd):
    ssp = pr.DataArray(cin, dims=["range", "depth"], coords={"range": r, "depth": z})
    bathy = pr.DataArray(bd, dims=["range"], coords={"range": br})
    return pr.OceanEnvironment2D(ssp, bathy, flat_earth_transform=False)


def munk_env(pr, ztop=6000.0):
    """range-independent Munk, 5000 m flat bottom: LDS tables, rows layout"""
    z = np.arange(0, ztop, 1.0)
    r = np.linspace(0, 200e3, 100)
    return _env(pr, z, r, np.tile(pr.munk_ssp(z), (100, 1)), r, np.full(100, 5000.0))


def sloping_env(pr):
    """range-dependent Munk over a sloping bottom: tables in HBM, sample-blocked layout"""
    z = np.linspace(0, 5500, 1377)
    r = np.linspace(0, 200e3, 33)
    br = np.linspace(0, 200e3, 9)
    return _env(pr, z, r, np.array([pr.munk_ssp(z, 1300 + 5e-4 * ri) for ri in r]), br, 4800 + 300 * np.sin(br / 40e3))


DEPTHS = np.linspace(-150.0, 5850.0, 1000)          # some above the surface and below the bottom


def _same(a, b):
    return np.array_equal(a, b, equal_nan=True)


def test_isovelocity_fan_end_to_end_matches_the_image_sum(pr):
    z = np.arange(0, 6000, 10.0)
    r = np.linspace(0, 25e3, 6)
    env = _env(pr, z, r, np.full((len(r), len(z)), 1500.0), r, np.full(len(r), 5000.0))
    # 10 m between save ranges: a sample next to a reflection may come from the reflected segment's dense output evaluated
    # up to half a sample spacing before the reflection (the reference's nearest-index re-sampling), i.e. up to
    # 5 m x tan(80 deg) = 28 m outside the water column -- inside the receivers' margin
    fan = pr.shoot_rays(1000.0, 0.0, np.linspace(-80, 80, 20001), 20e3, 2001, env, flatearth=False, debug=False)
    assert len(fan) == 20001 and fan.device_resident
    depths = np.arange(tlr.MARGIN, 5000 - tlr.MARGIN + 1, 50.0)
    tl = pr.transmission_loss(fan, depths, env, flatearth=False)
    x = np.asarray(fan.rs[0])
    assert np.isnan(tl[:, 0]).all()
    keep = (x >= 1e3) & (x <= 20e3)
    err = np.abs(tl[:, keep] - tlr.to_db(tlr.image_intensity(x[keep], depths, 1000.0, 5000.0, 80.0)))
    j, k = np.unravel_index(np.argmax(err), err.shape)
    assert err.max() < tlr.TOL_DB, (err.max(), depths[j], x[keep][k])


@pytest.mark.parametrize("case", ["munk", "sloping", "flatearth"])
def test_bit_identical_to_the_restatement(pr, case):
    if case == "munk":
        env, fe, blocked = munk_env(pr), False, False
    elif case == "sloping":
        env, fe, blocked = sloping_env(pr), False, True
    else:
        env, fe, blocked = pr.OceanEnvironment2D(), True, False
    fan = pr.shoot_rays(1000.0, 0.0, np.linspace(-20, 20, 3000), 100e3, 201, env, flatearth=fe, debug=False,
                        device_resident=True)
    assert fan.device_resident and fan._dev._env.blocked_layout == blocked
    I = pr.transmission_loss(fan, DEPTHS, env, flatearth=fe, intensity=True)
    assert fan.device_resident and "_zs" not in fan.__dict__        # processed in place, nothing fetched
    assert I.shape == (len(DEPTHS), 201)
    ref = tlr.fan_intensity(fan, DEPTHS, env, flatearth=fe)
    assert _same(I, ref)
    assert (I[:, 1:] > 0).mean() > 0.3 and (I[0, 1:] == 0).all()   # covered, and a shadow above the surface


def test_one_answer_whatever_the_path(pr):
    env = sloping_env(pr)
    ang = np.linspace(-20, 20, 3000)
    dev = pr.shoot_rays(1000.0, 0.0, ang, 100e3, 201, env, flatearth=False, debug=False, device_resident=True)
    host = pr.shoot_rays(1000.0, 0.0, ang, 100e3, 201, env, flatearth=False, debug=False, device_resident=False)
    assert dev._dev._env.blocked_layout
    a = pr.transmission_loss(dev, DEPTHS, env, flatearth=False)
    assert dev.device_resident
    b = pr.transmission_loss(host, DEPTHS, env, flatearth=False)
    assert _same(a, b)
    # the same fan: sample-blocked in HBM, then fetched and uploaded again as rows
    dev.to_host()
    assert not dev.device_resident
    assert _same(a, pr.transmission_loss(dev, DEPTHS, env, flatearth=False))


def test_headline_fan_twice_bit_equal(pr):
    env = pr.OceanEnvironment2D()
    fan = pr.shoot_rays(1000.0, 0.0, np.linspace(-20, 20, 100_000), 100e3, 1001, env, debug=False)
    assert fan.device_resident
    a = pr.transmission_loss(fan, DEPTHS, env, intensity=True)
    b = pr.transmission_loss(fan, DEPTHS, env, intensity=True)
    assert fan.device_resident and a.shape == (1000, 1001)
    assert _same(a, b) and (a[:, 1:] > 0).mean() > 0.3


def test_dropped_rays_are_skipped_and_their_neighbours_joined(pr):
    env = munk_env(pr, ztop=4200.0)                     # table shallower than the sea floor: deep rays leave it, dropped
    ang = np.linspace(-20, 20, 800)
    dev = pr.shoot_rays(1000.0, 0.0, ang, 100e3, 101, env, flatearth=False, debug=False, device_resident=True)
    host = pr.shoot_rays(1000.0, 0.0, ang, 100e3, 101, env, flatearth=False, debug=False, device_resident=False)
    assert 20 < len(ang) - len(dev) < 700 and len(dev) == len(host)
    a = pr.transmission_loss(dev, DEPTHS, env, flatearth=False, intensity=True)
    assert dev.device_resident
    b = pr.transmission_loss(host, DEPTHS, env, flatearth=False, intensity=True)
    assert _same(a, b) and _same(a, tlr.fan_intensity(host, DEPTHS, env, flatearth=False))


def test_backwards_fan(pr):
    env = sloping_env(pr)
    fan = pr.shoot_rays(900.0, 150e3, np.linspace(-15, 15, 500), 40e3, 111, env, flatearth=False, debug=False,
                        device_resident=True)
    assert fan.rs[0, 0] == 150e3 and fan.rs[0, -1] == 40e3
    I = pr.transmission_loss(fan, DEPTHS, env, flatearth=False, intensity=True)
    assert np.isnan(I[:, 0]).all() and (I[:, 1:] > 0).mean() > 0.3
    assert _same(I, tlr.fan_intensity(fan, DEPTHS, env, flatearth=False))


def test_two_rays_one_receiver_and_receivers_on_sample_depths(pr):
    env = munk_env(pr)
    fan = pr.shoot_rays(1000.0, 0.0, [-5.0, 5.0], 50e3, 51, env, flatearth=False, debug=False)
    tl = pr.transmission_loss(fan, [1000.0], env, flatearth=False)
    assert tl.shape == (1, 51) and np.isnan(tl[0, 0])
    assert _same(tl, tlr.to_db(tlr.fan_intensity(fan, [1000.0], env, flatearth=False)))
    # receivers exactly on sample depths: [lo, hi) counts a receiver on a shared ray once
    fan = pr.shoot_rays(1000.0, 0.0, np.linspace(-10, 10, 200), 50e3, 51, env, flatearth=False, debug=False)
    d = np.unique(-fan.zs[::7, 10:40:3].ravel())
    I = pr.transmission_loss(fan, d, env, flatearth=False, intensity=True)
    assert _same(I, tlr.fan_intensity(fan, d, env, flatearth=False))


def test_source_column_is_nan_and_shadows_are_inf(pr):
    env = munk_env(pr)
    fan = pr.shoot_rays(1000.0, 0.0, np.linspace(-10, 10, 300), 50e3, 51, env, flatearth=False, debug=False)
    tl = pr.transmission_loss(fan, [-50.0, 1000.0, 5100.0], env, flatearth=False)
    assert np.isnan(tl[:, 0]).all()
    assert np.isposinf(tl[[0, 2], 1:]).all()
    assert np.isfinite(tl[1, 1:]).any()


def test_value_errors(pr):
    env = pr.OceanEnvironment2D()
    fan = pr.shoot_rays(1000.0, 0.0, np.linspace(-10, 10, 100), 20e3, 21, env, debug=False, device_resident=True)
    with pytest.raises(ValueError, match="another environment"):
        pr.transmission_loss(fan, [100.0], env, flatearth=False)
    with pytest.raises(ValueError, match="ascending"):
        pr.transmission_loss(fan, [100.0, 50.0], env)
    with pytest.raises(ValueError, match="finite"):
        pr.transmission_loss(fan, [np.nan], env)
    one = pr.shoot_rays(1000.0, 0.0, [3.0], 20e3, 21, env, debug=False)
    with pytest.raises(ValueError, match="at least 2 rays"):
        pr.transmission_loss(one, [100.0], env)
    with pytest.raises(ValueError, match="Flat earth transformation has not been applied"):
        pr.transmission_loss(fan, [100.0], munk_env(pr))
    assert fan.device_resident
