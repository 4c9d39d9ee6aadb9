"""Path integrals and volume absorption without a GPU: Thorp's formula, the library's exp on the weights' range, the NumPy
restatement of the running path integral (tests/path_reference.py) against two closed forms, and the argument errors
refused before anything reaches the device."""
import math

import numpy as np
import pytest

import pygenray_amd as pr

import beam_reference as bref
import path_reference as pref
import tl_reference as tlr

EPS = np.finfo(float).eps


# ---- Thorp ---------------------------------------------------------------------------------------------------------------

def test_thorp_values_are_the_formula_evaluated_by_hand():
    # f = 1 kHz: f^2 = 1:  0.11 / 2 + 44 / 4101 + 2.75e-4 + 0.003
    assert pr.thorp_absorption(1000.0) == pytest.approx(0.055 + 44.0 / 4101.0 + 0.000275 + 0.003, rel=1e-14)
    assert pr.thorp_absorption(1000.0) == pytest.approx(0.0690040909, abs=1e-9)
    # f = 250 Hz: f^2 = 1 / 16:  0.11 / 17 + 44 / 65601 + 2.75e-4 / 16 + 0.003
    assert pr.thorp_absorption(250.0) == pytest.approx(0.11 / 17.0 + 44.0 / 65601.0 + 2.75e-4 / 16.0 + 0.003, rel=1e-14)
    assert pr.thorp_absorption(250.0) == pytest.approx(0.0101585, abs=1e-6)
    # the issue's orders of magnitude over 1000 km: about 10 dB at 250 Hz, about 70 dB at 1 kHz
    assert 9.0 < 1000 * pr.thorp_absorption(250.0) < 11.0 and 65.0 < 1000 * pr.thorp_absorption(1000.0) < 75.0
    # vectorised, shape kept; a scalar gives a float
    f = np.array([[50.0, 250.0], [1000.0, 10e3]])
    a = pr.thorp_absorption(f)
    assert a.shape == (2, 2) and a[0, 1] == pr.thorp_absorption(250.0) and isinstance(pr.thorp_absorption(250), float)
    assert np.all(np.diff(a.ravel()) > 0)


@pytest.mark.parametrize("f", [0.0, -1.0, [100.0, 0.0], np.nan, np.inf])
def test_thorp_refuses_frequencies_that_are_not_positive(f):
    with pytest.raises(ValueError, match="> 0"):
        pr.thorp_absorption(f)


# ---- the weights' exp ----------------------------------------------------------------------------------------------------

def _gexp_samples():
    rng = np.random.default_rng(11)
    k = np.arange(-1009, 1) * math.log(2)                # arguments at and next to the reduction's breakpoints (k +- 1/2) ln 2
    edges = np.concatenate([k + 0.5 * math.log(2), np.nextafter(k + 0.5 * math.log(2), -np.inf), k])
    y = np.concatenate([rng.uniform(-700.0, 0.0, 20000), -np.logspace(-300, 2.845, 2000), edges, [-700.0, 0.0, -0.0]])
    return y[(y >= -700.0) & (y <= 0.0)]


def test_gexp_is_within_one_and_a_half_ulp_of_exp_down_to_minus_700():
    import mpmath
    mpmath.mp.dps = 40
    y = _gexp_samples()
    g = pref.gexp(y)
    assert np.array_equal(g[y >= -8.0], bref.gexp(y[y >= -8.0]))     # the beams' exp, the same bits
    worst = 0.0
    for a, b in zip(y, g):
        e = mpmath.exp(mpmath.mpf(float(a)))
        worst = max(worst, abs(float((mpmath.mpf(float(b)) - e) / np.spacing(float(e)))))
    print(f"gexp on [-700, 0]: worst error {worst:.3f} ulp over {len(y)} arguments")
    assert worst <= 1.5, worst                            # tests/test_beam_tl_host.py's bound (beam_reference.GEXP_ULPS)
    assert pref.gexp(0.0) == 1.0 and pref.gexp(-0.0) == 1.0


def test_weights_are_cut_at_minus_700_and_keep_nan():
    K = pref.LN10_10
    assert K == float.fromhex("0x1.d791c5f888822p-3") and abs(K - math.log(10) / 10) <= np.spacing(K)
    A_cut = 700.0 / K
    A = np.array([0.0, -0.0, 10.0, 3040.0, np.nextafter(A_cut, 0.0), A_cut * (1 + 4 * EPS), 1e6, np.inf, np.nan])
    W = pref.weights(A)
    assert W[0] == 1.0 and W[1] == 1.0
    assert W[2] == pytest.approx(0.1, rel=4 * EPS) and W[3] == pytest.approx(1e-304, rel=1e-12)
    assert -(A[4] * K) >= -700.0 and W[4] > 0 and W[4] == pytest.approx(math.exp(-700.0), rel=1e-12)
    assert -(A[5] * K) < -700.0 and W[5] == 0.0 and W[6] == 0.0 and W[7] == 0.0 and np.isnan(W[8])


# ---- the restatement against closed forms --------------------------------------------------------------------------------

def test_profile_is_linear_inside_the_nodes_and_held_outside():
    nodes, al = np.array([100.0, 200.0, 1000.0]), np.array([1.0, 3.0, 2.0])
    d = np.array([-50.0, 100.0, 150.0, 200.0, np.nextafter(200.0, 0), 600.0, 1000.0, 5000.0, np.nan])
    v = pref.alpha_at(d, nodes, al)
    assert np.array_equal(v[:4], [1.0, 1.0, 2.0, 3.0]) and v[4] == pytest.approx(3.0, rel=4 * EPS)
    assert np.array_equal(v[5:8], [2.5, 2.0, 2.0]) and np.isnan(v[8])
    assert np.array_equal(pref.alpha_at(d, None, np.array([0.25])), np.full(len(d), 0.25))


def test_isovelocity_path_length_is_c0_times_travel_time():
    c0, S = 1500.0, 1001
    th = np.radians(np.linspace(-60.0, 60.0, 41))
    x = np.linspace(0.0, 1000e3, S)
    zs = -(1000.0 + np.outer(np.tan(th), x))                      # straight rays (no boundaries: depths leave the table)
    ts = np.outer(1.0 / (c0 * np.cos(th)), x)
    cin = np.full((2, 3), c0)
    rin, zin = np.array([-1.0, 2000e3]), np.array([-4e6, 0.0, 4e6])
    L = pref.path_integral(ts, zs, x, None, np.ones(1), cin, rin, zin)
    assert (L[:, 0] == 0).all() and (np.diff(L, axis=1) > 0).all()
    # Real arithmetic: the increments c0 (T_s+1 - T_s) telescope to c0 (T_s - T_0).  Rounding: per step the difference, the
    # product and the running add, 3 roundings of relative size u = EPS / 2 on numbers <= L: 1.5 EPS L per step, S steps;
    # the bilinear look-up of a constant table (3 products and 3 adds of weights, and their formation) is off by a few EPS
    # relative, which the sum inherits once, as is c0 * T itself: 8 EPS L covers both
    bound = (1.5 * np.arange(S)[None, :] + 8.0) * EPS * (c0 * ts)
    err = np.abs(L - c0 * ts)
    assert (err <= bound).all(), (err / np.maximum(bound, 1e-300)).max()
    # and the geometry: L = x / cos(theta)
    assert np.allclose(L[:, -1], x[-1] / np.cos(th), rtol=1e-12)
    # a constant alpha scales it: 0.07 dB/km over 1000 km at 0 degrees is 70 dB
    A = pref.path_integral(ts, zs, x, None, np.array([0.07e-3]), cin, rin, zin)
    assert A[20, -1] == pytest.approx(70.0, rel=1e-12)


def test_linear_gradient_path_length_is_the_circular_arc():
    import oracle
    from helpers import y0_for
    ca, gamma, z_s = tlr.GRADIENT_CA, tlr.GRADIENT_GAMMA, tlr.GRADIENT_ZS
    arrs = pr._unpack_envi(tlr.gradient_env(), flatearth=False)
    theta = np.linspace(-tlr.GRADIENT_APERTURE, tlr.GRADIENT_APERTURE, 201)          # depth-down (ODE convention)
    o = oracle.shoot_fan(*arrs, y0_for(oracle, arrs, z_s, 0.0, theta), 0.0, tlr.GRADIENT_X1, tlr.GRADIENT_S)
    assert (o["status"] == 0).all() and (o["n_bott"] == 0).all() and (o["n_surf"] == 0).all()
    cin, _, rin, zin = arrs[:4]
    L = pref.path_integral(o["T"], -o["z"], o["r"], None, np.ones(1), cin, rin, zin)
    ref = pref.arc_length(o["r"][None, :], np.radians(theta)[:, None])
    # The tolerance, from the trapezoid rule's error term: over steps of h in T the rule is off by at most
    # (T_end - T_0) h^2 / 12 max|c''(T)|.  Along a ray dc/dT = gamma c sin(theta) and d(theta)/dT = -a c with a = gamma
    # cos(theta0) / c_s, so c'' = gamma^2 c sin^2(theta) - gamma a c^2 cos(theta), |c''| <= gamma^2 c_max (1 + c_max / c_s).
    # The samples themselves are the tracer's: 1e-8 relative (the accuracy the fan is held to) on top.
    c_max, c_s = float(cin.max()), ca + gamma * z_s
    h = np.diff(o["T"], axis=1).max()
    tol = o["T"].max() * h * h / 12.0 * gamma * gamma * c_max * (1.0 + c_max / c_s) + 1e-8 * ref.max()
    err = np.abs(L - ref).max()
    print(f"linear gradient: path length off by {err:.3e} m at most, tolerance {tol:.3e} m, paths to {ref.max():.0f} m")
    assert tol < 0.01 and err < tol, (err, tol)
    # the test's power: an integral with c at the source instead of c(d) misses the arc a hundred tolerances over
    wrong = c_s * (o["T"] - o["T"][:, :1])
    assert np.abs(wrong - ref).max() > 100 * tol


# ---- argument and keyword errors, no GPU ---------------------------------------------------------------------------------

def _host_fan(n=4, S=5):
    th = np.linspace(-5, 5, n)
    r = np.linspace(0, 10e3, S)
    zs = -(1000.0 + np.outer(np.tan(np.radians(th)), r))
    ps = np.tile(np.sin(np.radians(th))[:, None] / 1500.0, (1, S))
    ts = np.outer(1.0 / (1500.0 * np.cos(np.radians(th))), r)
    return pr.RayFan.from_arrays(th, np.tile(r, (n, 1)), ts, zs, ps, np.zeros(n, np.int64), np.zeros(n, np.int64),
                                 np.full(n, 1000.0))


BAD_ABSORPTION = [(-0.1, ">= 0"), (np.nan, "finite"), (np.inf, "finite"), (([0.0, 100.0], [0.1, -0.1]), ">= 0"),
                  (([0.0, 100.0], [0.1, np.nan]), "finite"), (([100.0, 100.0], [0.1, 0.1]), "ascending"),
                  (([100.0, 50.0], [0.1, 0.1]), "ascending"), (([0.0, np.nan], [0.1, 0.1]), "ascending"),
                  (([0.0, 100.0], [0.1]), "equal"), (([], []), "equal"), ([0.1, 0.2, 0.3], "scalar"), ("thorp", None)]


@pytest.mark.parametrize("absorption, msg", BAD_ABSORPTION)
def test_bad_absorption_is_refused_before_the_device_by_every_function_that_takes_it(absorption, msg):
    env = pr.OceanEnvironment2D(flat_earth_transform=False)
    fan = _host_fan()
    calls = [lambda: pr.path_loss(fan, env, absorption, flatearth=False),
             lambda: pr.transmission_loss(fan, [100.0], env, flatearth=False, absorption=absorption),
             lambda: pr.beam_transmission_loss(fan, [100.0], env, flatearth=False, absorption=absorption),
             lambda: pr.arrivals(fan, [100.0], env, flatearth=False, absorption=absorption)]
    for call in calls:
        with pytest.raises(ValueError, match=msg):
            call()


def test_path_functions_check_their_other_arguments_before_the_device():
    env = pr.OceanEnvironment2D(flat_earth_transform=False)
    fan = _host_fan()
    for call in (lambda **k: pr.path_length(fan, env, **k), lambda **k: pr.path_loss(fan, env, 0.07, **k)):
        with pytest.raises(ValueError, match="Flat earth transformation has not been applied"):
            call()
        for bad, msg in (([5], "range_indices must lie"), ([-6], "range_indices must lie"), ([0.5], "integers"), ([], "non-empty")):
            with pytest.raises(ValueError, match=msg):
                call(flatearth=False, range_indices=bad)
    with pytest.raises(ValueError, match="no rays"):
        pr.path_length(fan[np.zeros(4, bool)], env, flatearth=False)
    rs = np.tile(np.linspace(0, 10e3, 5), (4, 1))
    rs[2, 3] += 1.0
    fan.rs = rs
    with pytest.raises(ValueError, match="rows of rays.rs differ"):
        pr.path_length(fan, env, flatearth=False)


def test_the_new_functions_are_exported():
    for name in ("thorp_absorption", "path_length", "path_loss"):
        assert name in pr.__all__ and callable(getattr(pr, name))
    import inspect
    for f in (pr.transmission_loss, pr.beam_transmission_loss, pr.arrivals):
        assert inspect.signature(f).parameters["absorption"].default is None


def test_weighted_restatements_without_weights_are_the_unweighted_ones():
    # path_reference's tube products with W = None against tl_reference / beam_reference / arrivals_reference themselves
    import arrivals_reference as aref
    from tube_gpu import SYN_R, SYN_Z, syn_cin, synthetic_fan
    cin = syn_cin()
    z, p, x, p0, depths = synthetic_fan(200, 6, 70, seed=3, cin=cin)
    t = np.cumsum(np.random.default_rng(1).uniform(0.2, 1.5, z.shape), axis=0)
    bottom = np.linspace(4700.0, 5150.0, 6)
    same = lambda a, b: np.array_equal(a, b, equal_nan=True)   # noqa: E731
    assert same(pref.tube_intensity(z.T, p.T, x, p0, depths, cin, SYN_R, SYN_Z, None),
                tlr.tube_intensity(z.T, p.T, x, p0, depths, cin, SYN_R, SYN_Z))
    B = pref.beam_intensity(z.T, p.T, x, p0, depths, cin, SYN_R, SYN_Z, bottom, 25.0, None)
    assert same(B, bref.beam_intensity(z.T, p.T, x, p0, depths, cin, SYN_R, SYN_Z, bottom, 25.0)) and (np.nan_to_num(B) > 0).any()
    cols = [1, 5, 2]
    a = pref.tube_arrivals(z.T, p.T, t.T, x, p0, depths, cols, cin, SYN_R, SYN_Z, None)
    b = aref.tube_arrivals(z.T, p.T, t.T, x, p0, depths, cols, cin, SYN_R, SYN_Z)
    assert len(b["tube"]) > 50 and all(same(a[k], b[k]) for k in b)
    # and weights of exactly 1.0 change nothing, while others do
    one = np.ones(z.T.shape)
    assert same(pref.beam_intensity(z.T, p.T, x, p0, depths, cin, SYN_R, SYN_Z, bottom, 25.0, one), B)
    assert not same(pref.beam_intensity(z.T, p.T, x, p0, depths, cin, SYN_R, SYN_Z, bottom, 25.0, 0.5 * one), B)
