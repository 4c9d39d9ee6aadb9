"""Test helpers for caustic_index / pressure_field (not a product path): a plain NumPy restatement of DESIGN.md section 16,
written from the definition -- the caustic index of every tube, the library's cos(2 pi t) / sin(2 pi t) operation for
operation, the coherent tube sum -- and the set-ups shared by the CPU and GPU tests (the focusing medium, Lloyd's mirror)."""
import numpy as np

import bounce_reference as bref
import path_reference as pref

# ---- cos(2 pi t), sin(2 pi t) on [-0.5, 0.5] ------------------------------------------------------------------------------

TWO_PI_HI = float.fromhex("0x1.921fb54442d18p+2")       # the double nearest 2 pi
TWO_PI_LO = float.fromhex("0x1.1a62633145c07p-52")      # the double nearest 2 pi - TWO_PI_HI
# Taylor coefficients of sin(2 pi b) / b - 2 pi and of cos(2 pi b) - 1 in z = b^2, from z^1 up: (-1)^n (2 pi)^(2n+1) / (2n+1)!
# and (-1)^n (2 pi)^(2n) / (2n)!, n = 1 ... 8, each the nearest double
SIN_C = [float.fromhex(h) for h in (
    "-0x1.4abbce625be53p+5", "0x1.466bc6775aae2p+6", "-0x1.32d2cce62bd86p+6", "0x1.50783487ee782p+5",
    "-0x1.e3074fde8871fp+3", "0x1.e8f434d018d63p+1", "-0x1.6fadb9f155744p-1", "0x1.aaec32af93359p-4")]
COS_C = [float.fromhex(h) for h in (
    "-0x1.3bd3cc9be45dep+4", "0x1.03c1f081b5ac4p+6", "-0x1.55d3c7e3cbffap+6", "0x1.e1f506891babbp+5",
    "-0x1.a6d1f2a204a8cp+4", "0x1.f9d38a3763cc3p+2", "-0x1.b6e24f44b128fp+0", "0x1.20c62c2f2d7f5p-2")]

# the bound of the issue on the absolute error of both functions (two ulp of 1.0), and the worst value measured against
# mpmath on test_coherent_host.py's points (24 000 random, every fold seam and its neighbours, +-0.5, 0)
TRIG_BOUND = 2.0 ** -51
TRIG_MEASURED = 1.36e-16


def _octant(t):
    """t in [-0.5, 0.5] -> (S, C, swap, flip): sin and cos of 2 pi b at the octant's b in [0, 0.125], and how they map back"""
    t = np.asarray(t, dtype=float)
    a = np.where(t < 0.0, -t, t)
    flip = a > 0.25
    a = np.where(flip, 0.5 - a, a)
    swap = a > 0.125
    b = np.where(swap, 0.25 - a, a)
    z = b * b
    ps = np.full_like(z, SIN_C[-1])
    for c in SIN_C[-2::-1]:
        ps = ps * z + c
    pc = np.full_like(z, COS_C[-1])
    for c in COS_C[-2::-1]:
        pc = pc * z + c
    S = b * TWO_PI_HI + b * (TWO_PI_LO + z * ps)
    C = 1.0 + z * pc
    return S, C, swap, flip


def gcos2pi(t):
    """cos(2 pi t), the kernel's operations in the kernel's order (csrc/pgr_trig.h), for t in [-0.5, 0.5]; NaN for a NaN"""
    S, C, swap, flip = _octant(t)
    v = np.where(swap, S, C)
    return np.where(flip, -v, v)


def gsin2pi(t):
    """sin(2 pi t) likewise"""
    S, C, swap, _ = _octant(t)
    v = np.where(swap, C, S)
    return np.where(np.asarray(t, dtype=float) < 0.0, -v, v)


# ---- the caustic index ------------------------------------------------------------------------------------------------------

def caustic_index(d, nb=None, ns=None):
    """The definition: depths d (M, S) of the surviving rays in launch order, per-sample bounce counts nb / ns (M, S) or None
    (all zero) -> kappa (M - 1, S) int32, one row per tube.  A loop over the columns in order, vectorised over tubes."""
    d = np.asarray(d, dtype=float)
    M, S = d.shape
    nb = np.zeros((M, S), np.int64) if nb is None else np.asarray(nb).astype(np.int64)
    ns = np.zeros((M, S), np.int64) if ns is None else np.asarray(ns).astype(np.int64)
    kappa = np.zeros((M - 1, S), np.int32)
    sig = np.zeros(M - 1, np.int64)
    n = np.zeros(M - 1, np.int32)
    for s in range(S):
        d0, d1 = d[:-1, s], d[1:, s]
        valid = ~np.isnan(d0) & ~np.isnan(d1) & (d1 != d0) & (nb[:-1, s] == nb[1:, s]) & (ns[:-1, s] == ns[1:, s])
        u = np.where(d1 > d0, 1, -1) * np.where((nb[:-1, s] + ns[:-1, s]) & 1, -1, 1)
        n = n + (valid & (sig != 0) & (u != sig))
        sig = np.where(valid, u, sig)
        kappa[:, s] = n
    return kappa


def tube_phase(kappa, nb, ns):
    """q (M, S) int32 of pressure_field: kappa + 2 ns of the tube's first ray, -1 where the two rays' counts differ; the
    last row (no tube) 0.  nb / ns None: kappa itself."""
    M1, S = kappa.shape
    q = np.zeros((M1 + 1, S), np.int32)
    q[:-1] = kappa
    if nb is not None:
        nb, ns = np.asarray(nb).astype(np.int64), np.asarray(ns).astype(np.int64)
        q[:-1] = np.where((nb[:-1] == nb[1:]) & (ns[:-1] == ns[1:]), kappa + 2 * ns[:-1], -1)
    return q


# ---- the coherent tube sum --------------------------------------------------------------------------------------------------

def as_complex(re, im):
    """re + i im with each part's own bits: `re + 1j * im` multiplies im by (0 + 1j), and 0 * inf puts a NaN into the real part
    of a sum that is infinite in the imaginary one only"""
    out = np.empty(np.shape(re), dtype=np.complex128)
    out.real, out.imag = re, im
    return out


def phase_cycles(T, q, f):
    """t of the definition: f T - q / 4 brought to [-0.5, 0.5] cycles in the kernel's steps"""
    y = f * T
    y = y - np.rint(y)
    t = y - 0.25 * (q & 3)
    return t - np.rint(t)


def tube_pressure(zs, ps, ts, x, p0, depths, cin, rin, zin, W, q, f):
    """The definition, restated: zs / ps / ts (M, S) stored convention (depth = -z), x (S,) save ranges in the frame of the
    tables, p0 (M,), weights W (M, S) or None, phase index q (M, S) integers or None, frequency f -> (re, im), each
    (len(depths), S).  path_reference.tube_intensity's loop over the tubes in increasing k, with the arrival's T."""
    depths = np.asarray(depths, dtype=float)
    ts = np.asarray(ts, dtype=float)
    d = -np.asarray(zs, dtype=float)
    M, S = d.shape
    g = pref.weighted_g(zs, ps, x, cin, rin, zin, W)
    r = np.abs(np.asarray(x, dtype=float) - x[0])
    re, im = np.zeros((len(depths), S)), np.zeros((len(depths), S))
    D = depths[:, None]
    with np.errstate(invalid="ignore", divide="ignore", over="ignore"):
        for k in range(M - 1):
            d0, d1 = d[k], d[k + 1]
            valid = ~np.isnan(g[k]) & ~np.isnan(g[k + 1]) & (d0 != d1)
            qk = np.zeros(S, np.int64) if q is None else np.asarray(q[k]).astype(np.int64)
            lo, hi = np.fmin(d0, d1), np.fmax(d0, d1)
            Ik = 0.5 * (g[k] + g[k + 1]) * np.abs(p0[k + 1] - p0[k]) / (r * np.abs(d1 - d0))
            hit = (valid & (qk >= 0))[None, :] & (lo[None, :] <= D) & (D < hi[None, :])
            if not hit.any():
                continue
            w = (D - d0[None, :]) / (d1 - d0)[None, :]
            T = ts[k][None, :] + w * (ts[k + 1] - ts[k])[None, :]
            a = np.sqrt(Ik)[None, :]
            t = phase_cycles(T, qk[None, :], f)
            re = np.where(hit, re + a * gcos2pi(t), re)
            im = np.where(hit, im + a * gsin2pi(t), im)
    re[:, r == 0] = np.nan
    im[:, r == 0] = np.nan
    return re, im


# ---- the focusing medium: c(z) = C0 cosh((z - Z0) / L) -------------------------------------------------------------------------
# Snell and the cosh profile make every ray z = Z0 + L asinh(tan(theta0) sin(x / L)): all rays of a source at Z0 meet again at
# x = n pi L, and between two foci adjacent rays keep their order, so tube k has passed floor(x / (pi L)) caustics at x.

FOCUS_C0, FOCUS_Z0, FOCUS_L, FOCUS_X1, FOCUS_S, FOCUS_N, FOCUS_APERTURE = 1480.0, 2500.0, 4000.0, 60e3, 601, 401, 10.0


def focus_env(pr):
    z = np.arange(0.0, 5001.0, 5.0)
    r = np.linspace(0.0, 80e3, 5)
    c = FOCUS_C0 * np.cosh((z - FOCUS_Z0) / FOCUS_L)
    ssp = pr.DataArray(np.tile(c, (len(r), 1)), dims=["range", "depth"], coords={"range": r, "depth": z})
    bathy = pr.DataArray(np.full(len(r), 5000.0), dims=["range"], coords={"range": r})
    return pr.OceanEnvironment2D(ssp, bathy, flat_earth_transform=False)


def focus_angles():
    return np.linspace(-FOCUS_APERTURE, FOCUS_APERTURE, FOCUS_N)


def check_focus_fan(x, zs, kappa, status, n_botts, n_surfs):
    """a fan traced in focus_env (stored-convention zs (M, S)) and its caustic index (M - 1, S): the premises, then the closed
    form at every tube and column"""
    assert (np.asarray(status) == 0).all() and (np.asarray(n_botts) == 0).all() and (np.asarray(n_surfs) == 0).all()
    d = -np.asarray(zs)
    assert d.shape == (FOCUS_N, FOCUS_S) and np.isfinite(d).all() and d.min() > 1700.0 and d.max() < 3300.0
    ref = np.floor(np.asarray(x) / (np.pi * FOCUS_L)).astype(np.int64)
    assert ref[-1] == 4 and kappa.shape == (FOCUS_N - 1, FOCUS_S)
    bad = np.argwhere(kappa != ref[None, :])
    assert len(bad) == 0, (len(bad), bad[:5])


# ---- Lloyd's mirror ---------------------------------------------------------------------------------------------------------
# Isovelocity, pressure-release surface: p = exp(i k R1) / R1 - exp(i k R2) / R2, R1 / R2 the distances from the source and
# from its image in the surface.

LLOYD_C, LLOYD_ZS, LLOYD_X1, LLOYD_S, LLOYD_N, LLOYD_APERTURE, LLOYD_F = 1500.0, 100.0, 5e3, 51, 6001, 30.0, 50.0
LLOYD_DEPTHS = np.arange(20.0, 401.0, 20.0)
LLOYD_COLS = np.array([10, 20, 30, 40, 50])            # the save columns at 1, 2, 3, 4, 5 km
# the worst e = |p - p_ref| / sqrt(1 / R1^2 + 1 / R2^2) of the restatement on the CPU oracle's fan
# (tests/test_coherent_host.py prints it), and the bound of the issue: twice that, in any case below 0.05
LLOYD_MEASURED = 3.0265691817525873e-05
LLOYD_BOUND = 2.0 * LLOYD_MEASURED


def lloyd_env(pr):
    z = np.arange(0.0, 6001.0, 10.0)
    r = np.linspace(0.0, 10e3, 5)
    ssp = pr.DataArray(np.full((len(r), len(z)), LLOYD_C), dims=["range", "depth"], coords={"range": r, "depth": z})
    bathy = pr.DataArray(np.full(len(r), 5000.0), dims=["range"], coords={"range": r})
    return pr.OceanEnvironment2D(ssp, bathy, flat_earth_transform=False)


def lloyd_angles():
    return np.linspace(-LLOYD_APERTURE, LLOYD_APERTURE, LLOYD_N)


def lloyd_error(p, x):
    """p (len(LLOYD_DEPTHS), len(LLOYD_COLS)) complex at the ranges x -> e, the error against the two-path closed form in units
    of the incoherent amplitude; the premise that every receiver lies inside the aperture of both paths is asserted"""
    D, X = LLOYD_DEPTHS[:, None], np.asarray(x, dtype=float)[None, :]
    R1, R2 = np.hypot(X, D - LLOYD_ZS), np.hypot(X, D + LLOYD_ZS)
    assert (np.degrees(np.arctan2(D + LLOYD_ZS, X)) < LLOYD_APERTURE - 1.0).all()
    k = 2.0 * np.pi * LLOYD_F / LLOYD_C
    ref = np.exp(1j * k * R1) / R1 - np.exp(1j * k * R2) / R2
    return np.abs(p - ref) / np.sqrt(1.0 / R1 ** 2 + 1.0 / R2 ** 2)


def log_counts(bx, bk, xf):
    """nb, ns (M, S): section 14's rule on a log bx / bk (M, K) -- event e counts at column s when j_e <= s, every logged event
    at the last column (bounce_reference.sample_index: np.argmin itself)"""
    bk = np.asarray(bk)
    S = len(xf)
    j = bref.sample_index(np.asarray(xf, dtype=float), bx)
    hit = (j[:, :, None] <= np.arange(S)[None, None, :]) | (np.arange(S)[None, None, :] == S - 1)
    nb = (hit & (bk == 1)[:, :, None]).sum(axis=1)
    ns = (hit & (bk == 0)[:, :, None]).sum(axis=1)
    return nb, ns


def fan_pressure(rays, depths, environment, f, flatearth=True, W=None, nb=None, ns=None, q=None):
    """pressure_field's definition on a host fan: the frame and p0 as tl_reference.fan_intensity prepares them, q from the
    restated caustic index and the per-sample counts nb / ns (M, S) (None: a fan without bounces) -> complex (R, S).  A q
    (M, S) given is used in place of the definition's (the tests' power checks: a deliberately wrong convention)."""
    from pygenray_amd.environment import _mirror_envi_arrays, _unpack_envi
    from pygenray_amd.host_physics import bilinear_interp
    from pygenray_amd.launch_rays import _initial_slowness
    x = np.asarray(rays.rs, dtype=float)[0]
    cin, cpin, rin, zin, bd, br, ba = _unpack_envi(environment, flatearth=flatearth)
    if len(x) > 1 and x[-1] < x[0]:
        cin, cpin, rin, bd, br, ba = _mirror_envi_arrays(cin, cpin, rin, bd, br, ba)
        x = -x
    c_source = bilinear_interp(x[0], float(rays.source_depths[0]), rin, zin, cin)
    p0 = _initial_slowness(rays.thetas, c_source)
    if q is None:
        q = tube_phase(caustic_index(-np.asarray(rays.zs), nb, ns), nb, ns)
    re, im = tube_pressure(rays.zs, rays.ps, rays.ts, x, p0, depths, cin, rin, zin, W, q, f)
    return as_complex(re, im)
