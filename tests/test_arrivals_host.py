"""arrivals without a GPU: the definition itself (its NumPy restatement in tests/arrivals_reference.py) against the
isovelocity image sources and the linear-gradient travel time (a CPU-oracle fan), the sum identity with the TL restatement,
and the argument errors refused before anything reaches the device."""

import numpy as np
import pytest

import pygenray_amd as pr

import arrivals_reference as ar
import tl_reference as tlr
from test_transmission_loss_host import C0, H, ZS, _host_fan, _oracle_gradient_fan, folded_fan


def _folded_arrivals(cols, depths):
    th, zs, ps, x = folded_fan()
    ts = x[None, :] / (C0 * np.cos(np.radians(th)))[:, None]            # straight rays: path length / c0
    cin = np.full((2, 3), C0)
    rin, zin = np.array([-1.0, 30e3]), np.array([0.0, 3000.0, 6000.0])
    p0 = np.sin(np.radians(th)) / C0
    a = ar.tube_arrivals(zs, ps, ts, x, p0, depths, cols, cin, rin, zin)
    return th, zs, ps, x, p0, a, (cin, rin, zin)


def test_restatement_sums_to_the_tl_restatement_bit_for_bit():
    depths = np.arange(tlr.MARGIN, H - tlr.MARGIN + 1, 250.0)
    cols = [200, 0, 37, 200, 5]                                          # repeated, shuffled, with the source column
    th, zs, ps, x, p0, a, (cin, rin, zin) = _folded_arrivals(cols, depths)
    I = tlr.tube_intensity(zs, ps, x, p0, depths, cin, rin, zin)
    sums = ar.sequential_sums(a["offsets"], a["I"]).reshape(len(depths), len(cols))
    ref = I[:, cols]
    assert ar.same(sums[:, [0, 2, 3, 4]], ref[:, [0, 2, 3, 4]])
    assert (np.diff(a["offsets"]).reshape(len(depths), len(cols))[:, 1] == 0).all()   # r = 0: no arrivals
    assert ar.same(sums[:, 0], sums[:, 3])


def test_restatement_finds_every_image_source_and_nothing_else():
    depths = np.arange(tlr.MARGIN, H - tlr.MARGIN + 1, 250.0)
    cols = list(range(10, 201, 10))                                      # 1 .. 20 km
    th, zs, ps, x, p0, a, _ = _folded_arrivals(cols, depths)
    n = len(cols)
    worst = 0.0
    for j, D in enumerate(depths):
        for c, s in enumerate(cols):
            sl = slice(a["offsets"][j * n + c], a["offsets"][j * n + c + 1])
            R_img, ang = ar.isovelocity_images(x[s], D, ZS, H, 80.0)
            assert sl.stop - sl.start == len(R_img), (D, x[s])
            o = np.argsort(a["T"][sl])
            T, tube = a["T"][sl][o], a["tube"][sl][o]
            ref = np.sort(R_img) / C0
            bound = ar.tube_time_bound(ps, zs, tube, s)
            assert (np.abs(T - ref) <= bound + 4e-16 * ref).all(), (D, x[s], np.abs(T - ref).max(), bound.max())
            worst = max(worst, (np.abs(T - ref) / bound).max())
    assert worst < 1.0


def test_gradient_travel_time_matches_mpmath_quadrature():
    for r in (1e3, 7.5e3, 15e3):
        for t in np.radians([-8.0, -3.3, 0.0, 2.1, 8.0]):
            T = ar.gradient_travel_time(r, float(t))
            q = ar.gradient_travel_time_quad(r, float(t))
            assert abs(T - q) <= 1e-12 * q, (r, t, T, q)


def test_restatement_on_the_oracle_gradient_fan_matches_the_closed_form():
    import oracle
    from helpers import y0_for
    o, theta0, I = _oracle_gradient_fan()
    x = o["r"]
    cols = np.nonzero(x >= 1e3)[0]
    arrs = pr._unpack_envi(tlr.gradient_env(), flatearth=False)
    y0 = y0_for(oracle, arrs, tlr.GRADIENT_ZS, 0.0, np.linspace(-tlr.GRADIENT_APERTURE, tlr.GRADIENT_APERTURE, 2001))  # (as _oracle_gradient_fan)
    cin, _, rin, zin = arrs[:4]
    a = ar.tube_arrivals(-o["z"], -o["p"], o["T"], x, y0[:, 2], tlr.GRADIENT_DEPTHS, cols, cin, rin, zin)
    worst = check_gradient_arrivals(a, x, cols, -o["z"], -o["p"], o["T"], I, theta_deg=-np.degrees(theta0))
    # measured: the fan's own T misses the closed form by up to 1.0e-7 s (7e-8 relative, the integrator's tolerance), the
    # interpolation adds at most 0.5 of its tube bound
    assert worst < 0.6, worst


def check_gradient_arrivals(a, x, cols, zs, ps, ts, I, theta_deg, launch_angle=None):
    """One arrival per receiver inside the wedge and none outside, T within the tube bound of the closed form -- beyond the
    error the fan's own T carries at the tube's two rays (the integrator's, measured against the closed form per ray) --
    the launch angle within one fan spacing of theta0, and I equal to TL's value.  theta_deg: the fan's launch angles in
    RayFan.thetas' convention (positive up); launch_angle: the arrivals' own (None: interpolated here) -> the worst
    interpolation error as a fraction of its tube bound."""
    n = len(cols)
    _, th = tlr.linear_gradient_intensity(x[cols], tlr.GRADIENT_DEPTHS, tlr.GRADIENT_ZS, tlr.GRADIENT_CA,
                                          tlr.GRADIENT_GAMMA, -tlr.GRADIENT_APERTURE, tlr.GRADIENT_APERTURE, _solve=True)
    inside = np.isfinite(th)
    counts = np.diff(a["offsets"]).reshape(len(tlr.GRADIENT_DEPTHS), n)
    assert (counts[inside] == 1).all() and (counts[~inside] == 0).all()
    j, c = np.nonzero(inside)                                # (row-major: the arrivals' own order)
    s = np.asarray(cols)[c]
    T_ref = ar.gradient_travel_time(x[s], th[j, c])
    bound = ar.tube_time_bound(ps, zs, a["tube"], s)
    k = a["tube"]
    ray_err = [np.abs(np.asarray(ts)[kk, s] - ar.gradient_travel_time(x[s], np.radians(-theta_deg[kk]))) for kk in (k, k + 1)]
    excess = np.abs(a["T"] - T_ref) - np.fmax(*ray_err) - 1e-12 * T_ref
    assert (excess <= bound).all(), (excess.max(), bound.max())
    if launch_angle is None:
        t0, t1 = theta_deg[a["tube"]], theta_deg[a["tube"] + 1]
        launch_angle = t0 + a["w"] * (t1 - t0)
    spacing = np.abs(np.diff(theta_deg)).max()
    assert (np.abs(launch_angle + np.degrees(th[j, c])) <= spacing).all()     # depth-down theta0 = -thetas
    assert ar.same(a["I"], I[j, s])
    return (excess / bound).max()


# ---- argument errors (no device reached) -------------------------------------------------------------------------------

@pytest.mark.parametrize("ri, msg", [([], "non-empty"), ([5], "lie in"), ([-6], "lie in"), ([1.0], "integers"),
                                     ([True], "integers"), (["1"], "integers"), ([[1, 2]], "1-D")])
def test_range_indices_are_checked(ri, msg):
    env = pr.OceanEnvironment2D(flat_earth_transform=False)
    with pytest.raises(ValueError, match=msg):
        pr.arrivals(_host_fan(), [100.0], env, flatearth=False, range_indices=ri)


@pytest.mark.parametrize("depths, msg", [([10.0, 5.0], "ascending"), ([1.0, np.nan], "finite"), ([], "non-empty")])
def test_receiver_depths_are_checked(depths, msg):
    env = pr.OceanEnvironment2D(flat_earth_transform=False)
    with pytest.raises(ValueError, match=msg):
        pr.arrivals(_host_fan(), depths, env, flatearth=False)


def test_fans_that_cannot_form_tubes_are_refused():
    env = pr.OceanEnvironment2D(flat_earth_transform=False)
    with pytest.raises(ValueError, match="arrivals needs a fan of at least 2 rays"):
        pr.arrivals(_host_fan(n=1), [100.0], env, flatearth=False)
    with pytest.raises(ValueError, match="source depths"):
        pr.arrivals(_host_fan(source_depths=np.array([1000.0, 1000.0, 900.0, 1000.0])), [100.0], env, flatearth=False)
    with pytest.raises(ValueError, match="Flat earth transformation has not been applied"):
        pr.arrivals(_host_fan(), [100.0], env)


def test_arrivals_are_exported():
    assert {"arrivals", "Arrivals"} <= set(pr.__all__) and callable(pr.arrivals)
