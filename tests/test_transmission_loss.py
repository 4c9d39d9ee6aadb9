"""transmission_loss on the GPU (csrc/pgr_tl.h): the isovelocity image sum and the linear-gradient closed form end to end,
bit parity with the NumPy restatement of tests/tl_reference.py on both trajectory layouts and on synthetic inputs aimed at
the kernel's chunk, band and adds-nothing edges, one answer whatever the path."""
import numpy as np
import pytest

import tl_reference as tlr
from tube_gpu import (DEPTHS, SYN_R, SYN_Z, _device_intensity, _env, _same, munk_env, pr, pr_any, sloping_env,  # noqa: F401
                      sloping_env_shallow_table, syn_env, synthetic_fan)  # (pr, pr_any, syn_env: fixtures)

pytestmark = pytest.mark.gpu


def test_isovelocity_fan_end_to_end_matches_the_image_sum(pr_any):
    z = np.arange(0, 6000, 10.0)
    r = np.linspace(0, 25e3, 6)
    env = _env(pr_any, z, r, np.full((len(r), len(z)), 1500.0), r, np.full(len(r), 5000.0))
    # 10 m between save ranges: a sample next to a reflection may come from the reflected segment's dense output evaluated
    # up to half a sample spacing before the reflection (the reference's nearest-index re-sampling), i.e. up to
    # 5 m x tan(80 deg) = 28 m outside the water column -- inside the receivers' margin
    fan = pr_any.shoot_rays(1000.0, 0.0, np.linspace(-80, 80, 20001), 20e3, 2001, env, flatearth=False, debug=False)
    assert len(fan) == 20001 and fan.device_resident
    depths = np.arange(tlr.MARGIN, 5000 - tlr.MARGIN + 1, 50.0)
    tl = pr_any.transmission_loss(fan, depths, env, flatearth=False)
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


def test_headline_fan_twice_bit_equal(pr_any):
    env = pr_any.OceanEnvironment2D()
    fan = pr_any.shoot_rays(1000.0, 0.0, np.linspace(-20, 20, 100_000), 100e3, 1001, env, debug=False)
    assert fan.device_resident
    a = pr_any.transmission_loss(fan, DEPTHS, env, intensity=True)
    b = pr_any.transmission_loss(fan, DEPTHS, env, intensity=True)
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


# ---- the kernel on synthetic inputs: pgr_intensity_device against tube_intensity, bit for bit -------------------------
#
# pgr_tl_sum walks the chunks of 63 tubes (64 rays) 64 at a time, a wave per band of 64 receivers.  The ray counts make the
# last chunk full or hold one tube, and give 64 / 65 chunks (M = 4033 / 4034: one / two ballot rounds); 8300 rays take
# three rounds.  The receiver counts make the last band hold 1 / 63 / 64 receivers, and 4200 take more than 64 bands.

SYN_CASES = ([(M, 5, 129, False) for M in (2, 3, 63, 64, 65, 126, 127, 128, 4033, 4034, 4035, 8300)]
             + [(500, 5, R, False) for R in (1, 63, 64, 65, 128, 129, 4200)]
             + [(300, S, 100, False) for S in (1, 2, 5, 100)]
             + [(4100, 6, 300, True)])


@pytest.mark.parametrize("M, S, R, shuffle", SYN_CASES, ids=[f"M{M}-S{S}-R{R}{'-shuffled' if sh else ''}"
                                                              for M, S, R, sh in SYN_CASES])
def test_kernel_bit_identical_on_synthetic_inputs(pr, syn_env, M, S, R, shuffle):
    env, cin = syn_env
    z, p, x, p0, depths = synthetic_fan(M, S, R, seed=M * 1009 + S * 31 + R, cin=cin, shuffle=shuffle)
    I = _device_intensity(env, z, p, x, p0, depths)
    ref = tlr.tube_intensity(z.T, p.T, x, p0, depths, cin, SYN_R, SYN_Z)
    assert I.shape == (R, S)
    bad = ~((I == ref) | (np.isnan(I) & np.isnan(ref)))
    assert not bad.any(), (np.argwhere(bad)[:5], I[bad][:5], ref[bad][:5])
    src = x == x[0]
    assert np.isnan(I[:, src]).all() and not np.isnan(I[:, ~src]).any()
    if M >= 8 and S >= 3:
        assert (I[:, ~src] > 0).any()                               # (not vacuous: tubes reached receivers)


# ---- fan-level parity on the paths the tests above do not take ---------------------------------------------------------

@pytest.mark.parametrize("case", ["munk", "sloping"])
def test_several_ballot_rounds_bit_identical_to_the_restatement(pr, case):
    # >= 8200 surviving rays: > 128 chunks, three rounds of the 64-chunk ballot in pgr_tl_sum, on both layouts
    env, blocked = (munk_env(pr), False) if case == "munk" else (sloping_env(pr), True)
    fan = pr.shoot_rays(1000.0, 0.0, np.linspace(-20, 20, 8400), 100e3, 101, env, flatearth=False, debug=False,
                        device_resident=True)
    assert fan.device_resident and fan._dev._env.blocked_layout == blocked and len(fan) >= 8200
    depths = np.linspace(-50.0, 5050.0, 300)
    I = pr.transmission_loss(fan, depths, env, flatearth=False, intensity=True)
    assert _same(I, tlr.fan_intensity(fan, depths, env, flatearth=False))
    assert (I[:, 1:] > 0).mean() > 0.3


def test_dropped_rays_on_the_sample_blocked_layout(pr):
    env = sloping_env_shallow_table(pr)
    ang = np.linspace(-20, 20, 800)
    dev = pr.shoot_rays(1000.0, 0.0, ang, 100e3, 101, env, flatearth=False, debug=False, device_resident=True)
    host = pr.shoot_rays(1000.0, 0.0, ang, 100e3, 101, env, flatearth=False, debug=False, device_resident=False)
    assert dev._dev._env.blocked_layout                        # keep[m] through the blocked tl_index
    assert 20 < len(ang) - len(dev) < 700 and len(dev) == len(host)
    a = pr.transmission_loss(dev, DEPTHS, env, flatearth=False, intensity=True)
    assert dev.device_resident
    b = pr.transmission_loss(host, DEPTHS, env, flatearth=False, intensity=True)
    assert _same(a, b) and _same(a, tlr.fan_intensity(host, DEPTHS, env, flatearth=False))
    assert (a[:, 1:] > 0).mean() > 0.3


def test_backwards_host_fan(pr):
    env = sloping_env(pr)                                      # range dependent: c is looked up in the mirrored frame
    args = (900.0, 150e3, np.linspace(-15, 15, 500), 40e3, 111, env)
    dev = pr.shoot_rays(*args, flatearth=False, debug=False, device_resident=True)
    host = pr.shoot_rays(*args, flatearth=False, debug=False, device_resident=False)
    assert not host.device_resident and host.rs[0, 0] == 150e3
    a = pr.transmission_loss(dev, DEPTHS, env, flatearth=False, intensity=True)
    b = pr.transmission_loss(host, DEPTHS, env, flatearth=False, intensity=True)
    assert _same(a, b) and _same(b, tlr.fan_intensity(host, DEPTHS, env, flatearth=False))
    assert (b[:, 1:] > 0).mean() > 0.3


def test_flatearth_host_fan(pr):
    env = pr.OceanEnvironment2D()
    args = (1000.0, 0.0, np.linspace(-20, 20, 3000), 100e3, 201, env)
    dev = pr.shoot_rays(*args, debug=False, device_resident=True)
    host = pr.shoot_rays(*args, debug=False, device_resident=False)
    assert not host.device_resident
    a = pr.transmission_loss(dev, DEPTHS, env, intensity=True)
    b = pr.transmission_loss(host, DEPTHS, env, intensity=True)
    assert _same(a, b) and _same(b, tlr.fan_intensity(host, DEPTHS, env))
    assert (b[:, 1:] > 0).mean() > 0.3


# ---- a refracting medium: the HIP fan and TL against the linear-gradient closed form ------------------------------------

@pytest.mark.parametrize("device_resident", [True, False])
def test_linear_gradient_fan_matches_the_closed_form(pr_any, device_resident):
    env = tlr.gradient_env()
    fan = pr_any.shoot_rays(tlr.GRADIENT_ZS, 0.0, np.linspace(-tlr.GRADIENT_APERTURE, tlr.GRADIENT_APERTURE, 2001),
                        tlr.GRADIENT_X1, tlr.GRADIENT_S, env, flatearth=False, debug=False, device_resident=device_resident)
    assert len(fan) == 2001 and fan.device_resident == device_resident
    I = pr_any.transmission_loss(fan, tlr.GRADIENT_DEPTHS, env, flatearth=False, intensity=True)
    # the depth-down launch angle from the fan itself (stored p = -sin(theta0) / c_s), not from the user angles (Q1)
    c_s = tlr.GRADIENT_CA + tlr.GRADIENT_GAMMA * tlr.GRADIENT_ZS
    theta0 = np.arcsin(-np.asarray(fan.ps)[:, 0] * c_s)
    tlr.check_gradient_fan(np.asarray(fan.rs[0]), fan.zs, I, theta0, fan.n_botts, fan.n_surfs)
