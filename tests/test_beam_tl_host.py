"""beam_transmission_loss without a GPU: the kernel's exp against mpmath, the Gaussian-beam definition itself (its NumPy
restatement in tests/beam_reference.py) against the isovelocity image-source sum, the energy each beam puts into the water
column and the closed form of a linear sound-speed gradient (a CPU-oracle fan), and the argument errors refused before
anything reaches the device."""
import math

import numpy as np
import pytest

import pygenray_amd as pr

import beam_reference as bref
import tl_reference as tlr

C0, H, ZS, AP = 1500.0, 5000.0, 1000.0, 80.0
W_MIN = 10.0
ISO_CIN = np.full((2, 3), C0)
ISO_RIN, ISO_ZIN = np.array([-1.0, 30e3]), np.array([0.0, 3000.0, 6000.0])


def _gexp_samples():
    y = np.concatenate([np.linspace(-8.0, 0.0, 20001), -np.random.default_rng(5).uniform(0.0, 8.0, 2000),
                        [np.nextafter(-8.0, 0.0), -0.0, -1e-300, -np.log(2) / 2, np.log(2) / 2 - 1.0]])
    assert y.min() == -8.0 and y.max() == 0.0
    return y


def test_gexp_is_within_one_and_a_half_ulp_of_exp():
    import mpmath
    mpmath.mp.dps = 40
    y = _gexp_samples()
    g = bref.gexp(y)
    worst = 0.0
    for a, b in zip(y, g):
        e = mpmath.exp(mpmath.mpf(float(a)))
        worst = max(worst, abs(float((mpmath.mpf(float(b)) - e) / np.spacing(float(e)))))
    assert worst <= bref.GEXP_ULPS, worst
    assert bref.gexp(0.0) == 1.0


def test_contracted_gexp_error_is_the_one_the_contracted_beam_bound_uses():
    # gexp with every a * b + c fused (the contracted library) on the same samples: the measured worst error is
    # bref.GEXP_CONTRACTED_ULPS, which tests/test_contracted_arith.py puts into its bound on the beams' values
    import mpmath
    mpmath.mp.dps = 40
    worst = 0.0
    for a in _gexp_samples():
        e = mpmath.exp(mpmath.mpf(float(a)))
        worst = max(worst, abs(float((mpmath.mpf(bref.gexp_contracted(a)) - e) / np.spacing(float(e)))))
    assert 0.5 < worst <= bref.GEXP_CONTRACTED_ULPS, worst
    assert bref.gexp_contracted(0.0) == 1.0


def test_restatement_matches_the_image_sum_in_an_isovelocity_waveguide():
    x = np.array([0.0, 1e3, 2e3, 5e3, 10e3, 15e3, 20e3])
    th, zs, ps = bref.folded_fan(max_angle=AP, ranges=x)
    p0 = np.sin(np.radians(th)) / C0
    depths = np.arange(0.0, H + 1, 10.0)
    I = bref.beam_intensity(zs, ps, x, p0, depths, ISO_CIN, ISO_RIN, ISO_ZIN, np.full(len(x), H), W_MIN)
    assert np.isnan(I[:, 0]).all() and np.isfinite(I[:, 1:]).all()
    ref = tlr.image_intensity(x[1:], depths, ZS, H, AP)
    err = np.abs(tlr.to_db(I[:, 1:]) - tlr.to_db(ref))
    use = bref.clear_of_the_aperture_edge(depths, x[1:], len(th), AP, ZS, H, W_MIN)
    assert use.mean() > 0.75
    inner = ((depths >= 2 * W_MIN) & (depths <= H - 2 * W_MIN))[:, None] & use
    assert err[use].max() < 0.1, err[use].max()                  # measured 0.061 dB, next to the boundaries at 20 km
    assert err[inner].max() < 0.02, err[inner].max()             # measured 0.0049 dB
    # what the beams fix: the top hat, on the same receivers, is off by more than 0.5 dB (1.5 dB measured)
    It = tlr.tube_intensity(zs, ps, x, p0, depths, ISO_CIN, ISO_RIN, ISO_ZIN)
    with np.errstate(invalid="ignore"):
        tube_err = np.abs(tlr.to_db(It[:, 1:]) - tlr.to_db(ref))
    assert np.nanmax(np.where(use, tube_err, np.nan)) > 0.5


def test_energy_in_the_water_column_is_the_sum_of_the_beams_masses():
    x = np.array([0.0, 2e3, 7e3, 20e3])
    th, zs, ps = bref.folded_fan(n_rays=4001, max_angle=AP, ranges=x)
    p0 = np.sin(np.radians(th)) / C0
    bottom = np.full(len(x), H)
    n = int(math.ceil(H / (W_MIN / 8)))
    depths = np.linspace(0.0, H, n + 1)
    h = depths[1] - depths[0]
    I = bref.beam_intensity(zs, ps, x, p0, depths, ISO_CIN, ISO_RIN, ISO_ZIN, bottom, W_MIN)
    E, mass, sigma, A = bref.beam_masses(zs, ps, x, p0, ISO_CIN, ISO_RIN, ISO_ZIN, bottom, W_MIN)
    for s in range(1, len(x)):
        total = np.sum(E[:, s] * mass[:, s])
        trap = h * (I[:, s].sum() - 0.5 * (I[0, s] + I[-1, s]))
        # the quadrature error.  Uncut, a beam plus its images is even about 0 and about b, so the trapezoid rule on a grid
        # ending on both is the rule on a period of a smooth periodic function: exact up to exp(-2 pi^2 sigma^2 / h^2)
        # (Poisson summation; h <= sigma / 8 makes that e^-1263).  Each cut at 4 sigma removes a tail that falls
        # monotonically from A e^-8 and is integrated with an error of at most h A e^-8: two cuts for each of three centres.
        # (9e-5 of the total here; measured 1e-7.  A missing image would lose about 1 %.)
        a, sg = A[:, s][E[:, s] > 0], sigma[:, s][E[:, s] > 0]
        bound = 3 * np.sum(2 * h * a * math.exp(-8.0)) + 1e-12 * total
        assert abs(trap - total) <= bound, (x[s], trap, total, bound)
        # a beam 4 sigma clear of both boundaries keeps erf(2 sqrt 2) of its energy, wherever it is
        m = 0.5 * (-zs[:-1, s] - zs[1:, s])
        clear = (E[:, s] > 0) & (m - 4 * sigma[:, s] > 0) & (m + 4 * sigma[:, s] < H)
        assert clear.sum() > 1000 and np.allclose(mass[clear, s], bref.TRUNCATED_MASS, rtol=0, atol=1e-15)
        # and so does one that crosses a boundary: its image puts back what leaves the column
        assert (clear < (E[:, s] > 0)).sum() > 50
        assert np.abs(mass[E[:, s] > 0, s] - bref.TRUNCATED_MASS).max() < 1e-12


# ---- a refracting medium: c = 1520 - 0.02 z, rays are circular arcs (tl_reference.linear_gradient_intensity) ------------

def test_restatement_matches_the_linear_gradient_closed_form():
    import oracle
    from helpers import y0_for
    env = tlr.gradient_env()
    arrs = pr._unpack_envi(env, flatearth=False)
    theta = np.linspace(-tlr.GRADIENT_APERTURE, tlr.GRADIENT_APERTURE, 2001)
    y0 = y0_for(oracle, arrs, tlr.GRADIENT_ZS, 0.0, theta)
    o = oracle.shoot_fan(*arrs, y0, 0.0, tlr.GRADIENT_X1, tlr.GRADIENT_S)
    assert (o["status"] == 0).all() and (o["n_bott"] == 0).all() and (o["n_surf"] == 0).all()
    cin, _, rin, zin, bd, br = arrs[:6]
    x = o["r"]
    bottom = bref.bottom_depths(x, bd, br)
    assert (bottom == 5000.0).all()
    depths = tlr.GRADIENT_DEPTHS
    I = bref.beam_intensity(-o["z"], -o["p"], x, y0[:, 2], depths, cin, rin, zin, bottom, W_MIN)
    keep = x >= 1e3
    zs_, ca, gamma = tlr.GRADIENT_ZS, tlr.GRADIENT_CA, tlr.GRADIENT_GAMMA
    ref = tlr.linear_gradient_intensity(x[keep], depths, zs_, ca, gamma, -tlr.GRADIENT_APERTURE, tlr.GRADIENT_APERTURE)
    # the smoothing: a Gaussian of width sigma turns I into I + sigma^2 I'' / 2 + O(sigma^4); I'' from the closed form
    # itself (central differences over 2 sigma), sigma the widest beam at the column, and only receivers whose every beam
    # stays inside the wedge (4 sigma from its edges, where the closed form has a step)
    _, _, sigma, _, _, _ = bref._tubes(-o["z"], -o["p"], x, y0[:, 2], cin, rin, zin, W_MIN)
    sig = np.nanmax(sigma[:, keep], axis=0)
    dz = 2 * sig
    lo_edge = np.min(o["z"][:, keep], axis=0)                        # the wedge's upper edge (the oracle's z: depth) ...
    hi_edge = np.max(o["z"][:, keep], axis=0)                        # ... and its lower edge
    inside = (depths[:, None] >= lo_edge + 4 * sig + 2 * dz) & (depths[:, None] <= hi_edge - 4 * sig - 2 * dz)
    assert inside.mean() > 0.3
    xs = x[keep]
    Ip, Im = np.zeros_like(ref), np.zeros_like(ref)
    for k in range(len(xs)):
        Ip[:, k] = tlr.linear_gradient_intensity([xs[k]], depths + dz[k], zs_, ca, gamma, -tlr.GRADIENT_APERTURE,
                                                 tlr.GRADIENT_APERTURE)[:, 0]
        Im[:, k] = tlr.linear_gradient_intensity([xs[k]], depths - dz[k], zs_, ca, gamma, -tlr.GRADIENT_APERTURE,
                                                 tlr.GRADIENT_APERTURE)[:, 0]
    d2 = (Ip - 2 * ref + Im) / dz[None, :] ** 2
    with np.errstate(invalid="ignore", divide="ignore"):                 # (ref = 0 outside the wedge)
        smooth_db = 10 / math.log(10) * sig[None, :] ** 2 * np.abs(d2) / (2 * ref)
    # the sum over discrete tubes: Gaussians closer than sigma sum to the convolution within 2 exp(-2 pi^2) except at
    # the cuts, where a tube's term drops from A e^-8 to 0; the tubes switched on or off there cover at most one tube
    # width Dmax at each of the two cuts, a share of at most 2 (Dmax / sigma) e^-8 / sqrt(2 pi) of the beam's weight
    widths = np.abs(np.diff(o["z"][:, keep], axis=0))
    dmax = widths.max(axis=0)
    assert (dmax < sig).all()
    cut_db = 10 / math.log(10) * 2 * (dmax / sig) * math.exp(-8.0) / math.sqrt(2 * math.pi)
    # and the traced fan's own error, against the exact rays of the closed form: a beam sum is a mean over its tubes, so
    # a relative error e in the tubes' spacing (the ray density) reaches it at most as e
    c_s = ca + gamma * zs_
    z_exact = tlr.linear_gradient_ray(x[keep][None, :], np.arcsin(y0[:, 2] * c_s)[:, None], zs_, ca, gamma)[0]
    dens = np.abs(np.diff(o["z"][:, keep], axis=0) / np.diff(z_exact, axis=0) - 1)
    fan_db = 10 / math.log(10) * dens.max(axis=0)
    bound = 2.8e-4 + smooth_db + cut_db[None, :] + fan_db[None, :]
    with np.errstate(invalid="ignore"):                                 # (outside the wedge: inf - inf, not used)
        err = np.abs(tlr.to_db(I[:, keep]) - tlr.to_db(ref))
        excess = np.where(inside, err - bound, -np.inf)
    j, k = np.unravel_index(np.argmax(excess), excess.shape)
    assert excess.max() <= 0, (err[j, k], bound[j, k], depths[j], xs[k])


# ---- argument errors, refused before any device work --------------------------------------------------------------------

def _host_fan(n=4, S=5):
    th = np.linspace(-5, 5, n)
    r = np.linspace(0, 10e3, S)
    zs = -(1000.0 + np.outer(np.tan(np.radians(th)), r))
    ps = np.tile(np.sin(np.radians(th))[:, None] / 1500.0, (1, S))
    return pr.RayFan.from_arrays(th, np.tile(r, (n, 1)), np.zeros((n, S)), zs, ps, np.zeros(n, np.int64),
                                 np.zeros(n, np.int64), np.full(n, 1000.0))


@pytest.mark.parametrize("w", [0.0, -1.0, np.nan, np.inf])
def test_min_width_is_checked(w):
    env = pr.OceanEnvironment2D(flat_earth_transform=False)
    with pytest.raises(ValueError, match="min_width"):
        pr.beam_transmission_loss(_host_fan(), [100.0], env, flatearth=False, min_width=w)


@pytest.mark.parametrize("depths, msg", [([10.0, 5.0], "ascending"), ([1.0, np.nan], "finite"), ([], "non-empty")])
def test_receiver_depths_are_checked(depths, msg):
    env = pr.OceanEnvironment2D(flat_earth_transform=False)
    with pytest.raises(ValueError, match=msg):
        pr.beam_transmission_loss(_host_fan(), depths, env, flatearth=False)


def test_fans_that_cannot_form_tubes_and_flatearth_without_the_transform_are_refused():
    env = pr.OceanEnvironment2D(flat_earth_transform=False)
    with pytest.raises(ValueError, match="beam_transmission_loss needs a fan of at least 2 rays"):
        pr.beam_transmission_loss(_host_fan(n=1), [100.0], env, flatearth=False)
    with pytest.raises(ValueError, match="Flat earth transformation has not been applied"):
        pr.beam_transmission_loss(_host_fan(), [100.0], env)


def test_beam_transmission_loss_is_exported():
    assert "beam_transmission_loss" in pr.__all__ and callable(pr.beam_transmission_loss)
