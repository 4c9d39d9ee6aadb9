"""Test helpers for transmission_loss (not a product path): the tolerances, a plain NumPy restatement of the ray-tube sum of
DESIGN.md ("Transmission loss"), and the two closed forms it must reproduce: the isovelocity image-source sum and the
refracted field of a linear sound-speed profile."""
import math

import numpy as np

from pygenray_amd.environment import _mirror_envi_arrays, _unpack_envi
from pygenray_amd.host_physics import bilinear_interp
from pygenray_amd.launch_rays import _initial_slowness

# analytic checks.  Bit parity with tube_intensity is the kernel's contract; these bound the DEFINITION's error.
# Isovelocity image sum: receivers >= MARGIN m from either boundary, ranges 1-20 km, a 20 001-ray +-80 deg fan folded at both
# boundaries -- the top hat and the boundary strip dominate, so the bound is loose.
TOL_DB = 0.1
MARGIN = 100.0
# Linear gradient (no boundary touched, no caustic): 2001 rays over +-8 deg, ranges 1-15 km, every receiver inside the wedge.
# The top hat's error is first order in the tube's width there; the CPU oracle's fan measured 1.49e-4 dB worst
# (tests/test_transmission_loss_host.py).  A definition that took c at the source instead of c(d), or cos(theta0) instead
# of the local cos(theta), misses this bound by 0.22 dB, 400 times over.
TOL_DB_GRADIENT = 5e-4


def bilinear(x, y, x_grid, y_grid, values):
    """host_physics.bilinear_interp element-wise over arrays: the same cell rule (searchsorted side='left' - 1, clamped) and
    the same operations in the same order, so the same bits (tests/test_transmission_loss_host.py checks that)."""
    x = np.asarray(x, dtype=float)
    y = np.asarray(y, dtype=float)
    i = np.clip(np.searchsorted(x_grid, x) - 1, 0, len(x_grid) - 2)
    j = np.clip(np.searchsorted(y_grid, y) - 1, 0, len(y_grid) - 2)
    wx = (x - x_grid[i]) / (x_grid[i + 1] - x_grid[i])
    wy = (y - y_grid[j]) / (y_grid[j + 1] - y_grid[j])
    return ((1 - wx) * (1 - wy) * values[i, j] + wx * (1 - wy) * values[i + 1, j]
            + (1 - wx) * wy * values[i, j + 1] + wx * wy * values[i + 1, j + 1])


def tube_intensity(zs, ps, x, p0, depths, cin, rin, zin):
    """The definition, restated: zs / ps (M, S) stored convention (depth = -z), x (S,) save ranges in the frame of the tables,
    p0 (M,) launch slowness -> I (len(depths), S).  A loop over tubes in increasing k, vectorised over receivers."""
    zs = np.asarray(zs, dtype=float)
    ps = np.asarray(ps, dtype=float)
    depths = np.asarray(depths, dtype=float)
    M, S = zs.shape
    d = -zs
    c = bilinear(np.broadcast_to(x, (M, S)), d, rin, zin, cin)
    pc = ps * c
    ok = np.abs(pc) < 1                                  # (False for NaN)
    g = np.full((M, S), np.nan)
    with np.errstate(invalid="ignore"):
        g[ok] = c[ok] / np.sqrt(1 - pc[ok] * pc[ok])
    r = np.abs(np.asarray(x, dtype=float) - x[0])
    out = np.zeros((len(depths), S))
    with np.errstate(invalid="ignore", divide="ignore", over="ignore"):
        for k in range(M - 1):
            d0, d1 = d[k], d[k + 1]
            valid = ~np.isnan(g[k]) & ~np.isnan(g[k + 1]) & (d0 != d1)
            lo, hi = np.fmin(d0, d1), np.fmax(d0, d1)
            Ik = 0.5 * (g[k] + g[k + 1]) * np.abs(p0[k + 1] - p0[k]) / (r * np.abs(d1 - d0))
            hit = valid[None, :] & (lo[None, :] <= depths[:, None]) & (depths[:, None] < hi[None, :])
            out = np.where(hit, out + Ik[None, :], out)
    out[:, r == 0] = np.nan
    return out


def fan_intensity(rays, depths, environment, flatearth=True):
    """tube_intensity of a host fan from shoot_rays, prepared the way the definition says: the tables of the environment the
    fan was traced in (mirrored for a backwards fan) and p0 = sin(radians(theta)) / c_source."""
    x = np.asarray(rays.rs, dtype=float)[0]
    cin, cpin, rin, zin, bd, br, ba = _unpack_envi(environment, flatearth=flatearth)
    if len(x) > 1 and x[-1] < x[0]:
        cin, cpin, rin, bd, br, ba = _mirror_envi_arrays(cin, cpin, rin, bd, br, ba)
        x = -x
    c_source = bilinear_interp(x[0], float(rays.source_depths[0]), rin, zin, cin)
    p0 = _initial_slowness(rays.thetas, c_source)
    return tube_intensity(rays.zs, rays.ps, x, p0, depths, cin, rin, zin)


def image_intensity(ranges, depths, source_depth, water_depth, max_angle_deg):
    """Isovelocity waveguide with perfectly reflecting surface and bottom: sum over image sources of 1 / R^2, keeping the
    images whose launch angle |atan(dz / r)| lies inside the fan's aperture -> (len(depths), len(ranges))."""
    r = np.asarray(ranges, dtype=float)[None, :, None]
    d = np.asarray(depths, dtype=float)[:, None, None]
    tmax = np.tan(np.radians(max_angle_deg))
    nmax = int(np.ceil(tmax * np.max(ranges) / (2 * water_depth))) + 2
    n = np.arange(-nmax, nmax + 1)
    zi = np.concatenate([2 * n * water_depth + source_depth, 2 * n * water_depth - source_depth])[None, None, :]
    dz = np.abs(zi - d)
    inside = dz <= tmax * r
    return np.where(inside, 1.0 / (r * r + dz * dz), 0.0).sum(axis=2)


def linear_gradient_ray(r, theta0, z_s, c_a, gamma, m=np):
    """The ray launched at depth-down angle theta0 (radians) from depth z_s in c(z) = c_a + gamma z, at range r >= 0 ->
    (z, cos theta, dz / dtheta0).  Snell (cos theta / c = xi = cos theta0 / c_s) makes the ray a circular arc:
        sin theta(r) = sin theta0 - xi gamma r,   z = z_s + (cos theta - cos theta0) / (xi gamma)
    valid while |sin theta| < 1 (no vertical tangent).  dz / dtheta0 at fixed r in closed form.  ``m``: the maths module
    (NumPy for arrays, ``mpmath`` for the cross-check of the derivative)."""
    c_s = c_a + gamma * z_s
    s0, k0 = m.sin(theta0), m.cos(theta0)
    a = gamma * k0 / c_s                                 # xi gamma
    da = -gamma * s0 / c_s                               # d(xi gamma) / dtheta0
    s = s0 - a * r
    k = m.sqrt(1 - s * s)
    z = z_s + (k - k0) / a
    ds = k0 - r * da
    dk = -s / k * ds
    dz = ((dk + s0) * a - (k - k0) * da) / (a * a)
    return z, k, dz


def linear_gradient_intensity(ranges, depths, z_s, c_a, gamma, theta_min, theta_max, _solve=False):
    """Ray-tube intensity of a point source at depth z_s in an UNBOUNDED c(z) = c_a + gamma z (gamma != 0), fan of depth-down
    launch angles [theta_min, theta_max] (degrees) -> (len(depths), len(ranges)):

        I(r, d) = (c(d) / c_s) cos theta0 / (r cos theta(r) |dz/dtheta0|_r),   z(r; theta0) = d

    -- the continuum limit of the tube sum (p0 = sin theta0 / c_s, g = c / cos theta), 1 / R^2 as gamma -> 0.  theta0 by
    brentq on the aperture; 0 where d lies outside the wedge [z(r; theta_min), z(r; theta_max)] (the caller asserts that
    z is increasing in theta0 over the aperture: no caustic).  ``_solve=True`` also returns theta0 (NaN outside)."""
    from scipy.optimize import brentq
    r = np.asarray(ranges, dtype=float)
    d = np.asarray(depths, dtype=float)
    t_lo, t_hi = math.radians(theta_min), math.radians(theta_max)
    c_s = c_a + gamma * z_s
    I = np.zeros((len(d), len(r)))
    th = np.full((len(d), len(r)), np.nan)
    for k, rk in enumerate(r):
        z_lo = linear_gradient_ray(rk, t_lo, z_s, c_a, gamma, m=math)[0]
        z_hi = linear_gradient_ray(rk, t_hi, z_s, c_a, gamma, m=math)[0]
        for j, dj in enumerate(d):
            if not (z_lo <= dj <= z_hi):
                continue
            t0 = brentq(lambda t: linear_gradient_ray(rk, t, z_s, c_a, gamma, m=math)[0] - dj, t_lo, t_hi,
                        xtol=1e-15, rtol=4 * np.finfo(float).eps, maxiter=200)
            _, k_r, dz = linear_gradient_ray(rk, t0, z_s, c_a, gamma, m=math)
            I[j, k] = ((c_a + gamma * dj) / c_s) * math.cos(t0) / (rk * k_r * abs(dz))
            th[j, k] = t0
    return (I, th) if _solve else I


# The refracting case shared by the CPU and GPU tests.  Source at 1000 m in c = 1520 - 0.02 z, fan +-8 deg, ranges 1-15 km:
# the +8 deg ray reaches ~4700 m and the -8 deg ray turns at ~260 m, so no ray touches the surface or the 5000 m bottom,
# and the rays of an unbounded linear gradient (coaxal circles) have no caustic.  check_gradient_fan asserts both premises.
GRADIENT_CA, GRADIENT_GAMMA, GRADIENT_ZS, GRADIENT_X1, GRADIENT_S, GRADIENT_APERTURE = 1520.0, -0.02, 1000.0, 15e3, 151, 8.0
GRADIENT_DEPTHS = np.arange(25.0, 5000.0, 25.0)


def gradient_env():
    from pygenray_amd import DataArray, OceanEnvironment2D
    z = np.arange(0.0, 6001.0, 10.0)
    r = np.linspace(0.0, 20e3, 5)
    c = GRADIENT_CA + GRADIENT_GAMMA * z
    ssp = DataArray(np.tile(c, (len(r), 1)), dims=["range", "depth"], coords={"range": r, "depth": z})
    bathy = DataArray(np.full(len(r), 5000.0), dims=["range"], coords={"range": r})
    return OceanEnvironment2D(ssp, bathy, flat_earth_transform=False)


def check_gradient_fan(x, zs, I, theta0, n_botts, n_surfs):
    """A fan traced in gradient_env (save ranges x, stored-convention zs (M, S), depth-down launch angles theta0 in radians)
    and its intensity I at GRADIENT_DEPTHS: the premises, then I against linear_gradient_intensity within TOL_DB_GRADIENT
    at every receiver inside the wedge (ranges >= 1 km), and exactly 0 outside -> (worst error in dB, reference, inside)."""
    assert (np.asarray(n_botts) == 0).all() and (np.asarray(n_surfs) == 0).all()
    d = -np.asarray(zs)
    assert np.isfinite(d).all() and d.min() > 200.0 and d.max() < 4800.0
    keep = x >= 1e3
    zs_, ca, gamma = GRADIENT_ZS, GRADIENT_CA, GRADIENT_GAMMA
    th = np.linspace(theta0.min(), theta0.max(), 4001)
    assert (linear_gradient_ray(x[keep][None, :], th[:, None], zs_, ca, gamma)[2] > 0).all()   # no caustic
    ref = linear_gradient_intensity(x[keep], GRADIENT_DEPTHS, zs_, ca, gamma, np.degrees(theta0.min()),
                                    np.degrees(theta0.max()))
    inside = ref > 0
    assert 0.3 < inside.mean() < 0.9
    Ik = I[:, keep]
    assert (Ik[~inside] == 0).all()
    with np.errstate(invalid="ignore"):
        err = np.where(inside, np.abs(to_db(Ik) - to_db(ref)), 0.0)
    j, k = np.unravel_index(np.argmax(err), err.shape)
    assert err.max() < TOL_DB_GRADIENT, (err.max(), GRADIENT_DEPTHS[j], x[keep][k])
    return err.max(), ref, inside


def to_db(I):
    with np.errstate(divide="ignore"):
        return -10.0 * np.log10(I)
