"""beam_transmission_loss on the GPU (csrc/pgr_beams.h): bit parity with the NumPy restatement of tests/beam_reference.py on
synthetic inputs aimed at the kernel's chunk, halo, band and 4-sigma edges and on fans of both trajectory layouts, one
answer whatever the path, and the isovelocity image sum and the energy identity end to end."""
import math

import numpy as np
import pytest

import beam_reference as bref
import tl_reference as tlr
from pygenray_amd.host_physics import bilinear_interp
from pygenray_amd.launch_rays import _initial_slowness
from tube_gpu import (SYN_R, SYN_Z, _device_beams, _env, _same, munk_env, pr, pr_any, sloping_env,  # noqa: F401
                      sloping_env_shallow_table, syn_env, synthetic_fan)  # (pr, pr_any, syn_env: fixtures)

pytestmark = pytest.mark.gpu

DEPTHS = np.linspace(-150.0, 5850.0, 600)           # some above the surface and below the bottom


def _check_synthetic(env, cin, z, p, x, p0, bottom, depths, w_min):
    I = _device_beams(env, z, p, x, p0, bottom, depths, w_min)
    ref = bref.beam_intensity(z.T, p.T, x, p0, depths, cin, SYN_R, SYN_Z, bottom, w_min)
    assert I.shape == (len(depths), len(x))
    bad = ~((I == ref) | (np.isnan(I) & np.isnan(ref)))
    assert not bad.any(), (np.argwhere(bad)[:5], I[bad][:5], ref[bad][:5])
    src = x == x[0]
    assert np.isnan(I[:, src]).all() and not np.isnan(I[:, ~src]).any()
    return I


# ---- the kernel on synthetic inputs: pgr_beam_intensity_device against beam_intensity, bit for bit ---------------------
#
# A chunk is 61 tubes (lane t loads ray 61 c - 1 + t: the chunk's 62 rays and one neighbour either side).  The ray counts
# make the last chunk full or hold one / two tubes, give 64 and 65 chunks (M = 3905 / 3906: one / two ballot rounds), and
# 8300 rays take three rounds.  The receiver counts make the last band hold 1 / 63 / 64 receivers; 4200 take 66 bands.
# The widths: the monotone and cubic columns' tubes are a few metres wide (w_min = 40 dominates), the scrambled ones
# thousands (it does not); w_min = 0.5 leaves every sigma to the tubes.

SYN_CASES = ([(M, 5, 129, 40.0) for M in (2, 3, 60, 61, 62, 63, 64, 122, 123, 124, 3905, 3906, 8300)]
             + [(500, 5, R, 0.5) for R in (1, 63, 64, 65, 129, 4200)]
             + [(300, S, 100, 40.0) for S in (1, 2, 5, 100)])


@pytest.mark.parametrize("M, S, R, w_min", SYN_CASES, ids=[f"M{M}-S{S}-R{R}-w{w}" for M, S, R, w in SYN_CASES])
def test_kernel_bit_identical_on_synthetic_inputs(pr, syn_env, M, S, R, w_min):
    env, cin = syn_env
    z, p, x, p0, depths = synthetic_fan(M, S, R, seed=M * 1013 + S * 37 + R, cin=cin)
    bottom = np.linspace(4700.0, 5150.0, S)                  # a sloping bottom, crossed by the fan's samples
    I = _check_synthetic(env, cin, z, p, x, p0, bottom, depths, w_min)
    if M >= 8 and S >= 3:
        assert (I[:, x != x[0]] > 0).any()                   # (not vacuous: beams reached receivers)


def test_receivers_on_the_four_sigma_edges(pr, syn_env):
    # receivers at centre -+ 4 sigma and one ulp either side, for the beam and both its images: each term the
    # definition keeps must be kept and each it drops dropped, whatever the chunk test decided
    env, cin = syn_env
    M, S = 400, 4
    z, p, x, p0, depths = synthetic_fan(M, S, 64, seed=11, cin=cin)
    bottom = np.array([4900.0, 4950.0, 5000.0, 5050.0])
    w_min = 25.0
    valid, m, sigma, _, _, r = bref._tubes(z.T, p.T, x, p0, cin, SYN_R, SYN_Z, w_min)
    edge = []
    assert x[2] == x[0]                                               # (column 2 is the source's: NaN)
    for s in (1, 3):
        k = np.flatnonzero(valid[:, s])
        near_top = k[np.argsort(np.abs(m[k, s]))[:6]]                  # beams that reach the surface
        near_bot = k[np.argsort(np.abs(m[k, s] - bottom[s]))[:6]]      # ... and the bottom
        for kk in np.concatenate([k[::37], near_top, near_bot]):
            for ctr in (m[kk, s], -m[kk, s], 2.0 * bottom[s] - m[kk, s]):
                for e in (ctr - 4 * sigma[kk, s], ctr + 4 * sigma[kk, s]):
                    edge += [np.nextafter(e, -np.inf), e, np.nextafter(e, np.inf)]
    depths = np.unique(np.concatenate([depths, edge]))
    assert len(depths) > 500
    I = _check_synthetic(env, cin, z, p, x, p0, bottom, depths, w_min)
    assert (I[:, [1, 3]] > 0).mean() > 0.3


def test_all_sigmas_from_the_tubes_and_receivers_outside_the_column(pr, syn_env):
    env, cin = syn_env
    z, p, x, p0, _ = synthetic_fan(700, 6, 8, seed=5, cin=cin)
    depths = np.concatenate([np.linspace(-400.0, -1.0, 40), np.linspace(0.0, 5000.0, 90), np.linspace(5001.0, 5600.0, 40)])
    _check_synthetic(env, cin, z, p, x, p0, np.full(6, 5000.0), depths, 1e-3)


# ---- fans, bit for bit against the restatement on the fetched fan ---------------------------------------------------------

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
    I = pr.beam_transmission_loss(fan, DEPTHS, env, flatearth=fe, intensity=True)
    assert fan.device_resident and "_zs" not in fan.__dict__        # processed in place, nothing fetched
    assert I.shape == (len(DEPTHS), 201)
    assert _same(I, bref.fan_beam_intensity(fan, DEPTHS, env, 10.0, flatearth=fe))
    assert (I[:, 1:] > 0).mean() > 0.3


@pytest.mark.parametrize("case", ["munk", "sloping"])
def test_dropped_rays_are_skipped(pr, case):
    env = munk_env(pr, ztop=4200.0) if case == "munk" else sloping_env_shallow_table(pr)
    ang = np.linspace(-20, 20, 800)
    dev = pr.shoot_rays(1000.0, 0.0, ang, 100e3, 101, env, flatearth=False, debug=False, device_resident=True)
    host = pr.shoot_rays(1000.0, 0.0, ang, 100e3, 101, env, flatearth=False, debug=False, device_resident=False)
    assert dev._dev._env.blocked_layout == (case == "sloping")
    assert 20 < len(ang) - len(dev) < 700 and len(dev) == len(host)
    a = pr.beam_transmission_loss(dev, DEPTHS, env, flatearth=False, intensity=True, min_width=5.0)
    assert dev.device_resident
    b = pr.beam_transmission_loss(host, DEPTHS, env, flatearth=False, intensity=True, min_width=5.0)
    assert _same(a, b) and _same(a, bref.fan_beam_intensity(host, DEPTHS, env, 5.0, flatearth=False))
    assert (a[:, 1:] > 0).mean() > 0.3


@pytest.mark.parametrize("case", ["backwards", "flatearth"])
def test_one_answer_from_the_device_and_host_paths(pr, case):
    if case == "backwards":
        env, fe = sloping_env(pr), False                   # range dependent: c and b in the mirrored frame
        args = (900.0, 150e3, np.linspace(-15, 15, 500), 40e3, 111, env)
    else:
        env, fe = pr.OceanEnvironment2D(), True
        args = (1000.0, 0.0, np.linspace(-20, 20, 3000), 100e3, 201, env)
    dev = pr.shoot_rays(*args, flatearth=fe, debug=False, device_resident=True)
    host = pr.shoot_rays(*args, flatearth=fe, debug=False, device_resident=False)
    assert not host.device_resident
    a = pr.beam_transmission_loss(dev, DEPTHS, env, flatearth=fe, intensity=True)
    assert dev.device_resident
    b = pr.beam_transmission_loss(host, DEPTHS, env, flatearth=fe, intensity=True)
    assert _same(a, b) and _same(b, bref.fan_beam_intensity(host, DEPTHS, env, 10.0, flatearth=fe))
    assert np.isnan(a[:, 0]).all() and (a[:, 1:] > 0).mean() > 0.3


def test_headline_fan_twice_bit_equal(pr_any):
    env = pr_any.OceanEnvironment2D()
    fan = pr_any.shoot_rays(1000.0, 0.0, np.linspace(-20, 20, 100_000), 100e3, 1001, env, debug=False)
    assert fan.device_resident
    depths = np.linspace(0.0, 5000.0, 1000)
    a = pr_any.beam_transmission_loss(fan, depths, env, intensity=True)
    b = pr_any.beam_transmission_loss(fan, depths, env, intensity=True)
    assert fan.device_resident and a.shape == (1000, 1001)
    assert _same(a, b) and (a[:, 1:] > 0).mean() > 0.3


def test_value_errors(pr):
    env = pr.OceanEnvironment2D()
    fan = pr.shoot_rays(1000.0, 0.0, np.linspace(-10, 10, 100), 20e3, 21, env, debug=False, device_resident=True)
    with pytest.raises(ValueError, match="another environment"):
        pr.beam_transmission_loss(fan, [100.0], env, flatearth=False)
    with pytest.raises(ValueError, match="min_width"):
        pr.beam_transmission_loss(fan, [100.0], env, min_width=0.0)
    assert fan.device_resident


@pytest.mark.parametrize("w", [0.0, -1.0, np.nan, np.inf])
def test_the_c_entries_refuse_a_bad_min_width_and_write_nothing(pr, syn_env, w):
    import torch
    from pygenray_amd import _lib
    env = pr.OceanEnvironment2D()
    fan = pr.shoot_rays(1000.0, 0.0, np.linspace(-10, 10, 100), 20e3, 21, env, debug=False, device_resident=True)
    M, S = len(fan), 21
    dev = torch.device("cuda", 0)
    stream = torch.cuda.current_stream(dev).cuda_stream
    p0 = torch.zeros(M, dtype=torch.float64, device=dev)
    bottom = torch.full((S,), 5000.0, dtype=torch.float64, device=dev)
    depths = torch.full((1,), 1000.0, dtype=torch.float64, device=dev)
    out = torch.full((1, S), -1.0, dtype=torch.float64, device=dev)
    with pytest.raises(_lib.PgrError, match="min_width"):
        fan._dev.beam_intensity(p0.data_ptr(), bottom.data_ptr(), depths.data_ptr(), 1, w, out.data_ptr(), stream)
    assert fan.device_resident
    senv, cin = syn_env
    z = torch.full((S, M), -1000.0, dtype=torch.float64, device=dev)
    x = torch.linspace(0.0, 20e3, S, dtype=torch.float64, device=dev)
    with pytest.raises(_lib.PgrError, match="min_width"):
        _lib.beam_intensity_device(senv, z.data_ptr(), z.data_ptr(), M, S, x.data_ptr(), p0.data_ptr(), bottom.data_ptr(),
                                   depths.data_ptr(), 1, w, out.data_ptr(), stream)
    assert (out.cpu().numpy() == -1.0).all()


# ---- physics on HIP fans ------------------------------------------------------------------------------------------------

def test_isovelocity_fan_end_to_end_matches_the_image_sum(pr_any):
    z = np.arange(0, 6000, 10.0)
    r = np.linspace(0, 25e3, 6)
    env = _env(pr_any, z, r, np.full((len(r), len(z)), 1500.0), r, np.full(len(r), 5000.0))
    fan = pr_any.shoot_rays(1000.0, 0.0, np.linspace(-80, 80, 20001), 20e3, 2001, env, flatearth=False, debug=False)
    assert len(fan) == 20001 and fan.device_resident
    depths = np.arange(tlr.MARGIN, 5000 - tlr.MARGIN + 1, 50.0)
    tl = pr_any.beam_transmission_loss(fan, depths, env, flatearth=False)
    x = np.asarray(fan.rs[0])
    assert np.isnan(tl[:, 0]).all()
    keep = (x >= 1e3) & (x <= 20e3)
    err = np.abs(tl[:, keep] - tlr.to_db(tlr.image_intensity(x[keep], depths, 1000.0, 5000.0, 80.0)))
    use = bref.clear_of_the_aperture_edge(depths, x[keep], 20001, 80.0, 1000.0, 5000.0, 10.0)
    assert use.mean() > 0.75
    err = np.where(use, err, 0.0)
    j, k = np.unravel_index(np.argmax(err), err.shape)
    assert err.max() < tlr.TOL_DB, (err.max(), depths[j], x[keep][k])


def test_energy_identity_on_a_munk_fan(pr_any):
    # at a few columns, the trapezoid integral of the kernel's intensity over [0, b] on a grid of w_min / 8 is the sum of
    # the beams' energies times their masses inside the column (tests/test_beam_tl_host.py derives the bound)
    env = munk_env(pr_any)
    w_min = 10.0
    fan = pr_any.shoot_rays(1000.0, 0.0, np.linspace(-20, 20, 2000), 60e3, 61, env, flatearth=False, debug=False)
    H = 5000.0
    depths = np.linspace(0.0, H, int(math.ceil(H / (w_min / 8))) + 1)
    h = depths[1] - depths[0]
    I = pr_any.beam_transmission_loss(fan, depths, env, flatearth=False, intensity=True, min_width=w_min)
    cols = np.array([0, 7, 30, 60])
    xf, cin, rin, zin, bd, br = bref.frame_tables(np.asarray(fan.rs[0]), env, flatearth=False)
    p0 = _initial_slowness(fan.thetas, bilinear_interp(xf[0], 1000.0, rin, zin, cin))
    E, mass, sigma, A = bref.beam_masses(fan.zs[:, cols], fan.ps[:, cols], xf[cols], p0, cin, rin, zin,
                                         np.full(len(cols), H), w_min)
    for i, s in enumerate(cols[1:], start=1):
        total = np.sum(E[:, i] * mass[:, i])
        trap = h * (I[:, s].sum() - 0.5 * (I[0, s] + I[-1, s]))
        a = A[:, i][E[:, i] > 0]
        bound = 3 * np.sum(2 * h * a * math.exp(-8.0)) + 1e-12 * total
        assert abs(trap - total) <= bound, (s, trap, total, bound)
        assert np.abs(mass[E[:, i] > 0, i] - bref.TRUNCATED_MASS).max() < 1e-12
