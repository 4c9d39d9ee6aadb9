"""Test helpers (not a product path): two wave-theory truths for the coherent products that share nothing with the ray code --
the normal modes of coherent_reference's focusing medium (the caustic phase), and the image sum of an isovelocity waveguide with
a pressure-release surface and a rigid bottom (the bounce counts, the flips, the boundary phases) as a CW field, a transfer
function with a reduction time and a Gaussian pulse -- with the set-ups shared by the CPU and GPU tests and the errors measured
on the CPU oracle's fans (tests/test_coherent_wave_host.py prints them)."""
import numpy as np

import coherent_reference as cref
import signal_reference as sref

# ---- normal modes of the focusing medium --------------------------------------------------------------------------------------
# psi'' + (w^2 / c(z)^2 - k^2) psi = 0 between Dirichlet walls at 500 m and 4500 m by second-order finite differences on the
# piecewise-linear profile of focus_env's 5 m table; the modes that matter (launch angles within +-10 degrees) turn within
# +-1500 m of the axis, so the walls are not involved.  Far field of a point source of unit strength re 1 m:
#     p(r, z) = e^{i pi / 4} sum_m w_m psi_m(z_s) psi_m(z) e^{i k_m r} sqrt(2 pi / (k_m r)),   sum psi^2 dz = 1
# with a cos^2 taper w_m in the mode angle acos(k_m C0 / w) from 1 at 14 degrees to 0 at 21 degrees: a sharp cut radiates from
# its edge (e = 0.14 then).

MODE_WALLS = (500.0, 4500.0)
MODE_DZ = 1.0                                 # 3999 unknowns, 56 modes at 50 Hz; at half of it the worst e at 50 Hz is 0.0162, not 0.0180
MODE_TAPER = (14.0, 21.0)
MODE_F = (40.0, 50.0, 60.0)
MODE_DEPTHS = np.arange(1800.0, 3201.0, 50.0)
MODE_X_MIN, MODE_FOCUS_CLEAR, MODE_FAN_ANGLE = 3e3, 2e3, 8.0
# the worst e = |p - p_modes| / |p_modes| over mode_cells() of the restatement cref.fan_pressure on the CPU oracle's fan at
# 40 / 50 / 60 Hz, and the one bound: twice the worst of the three, in any case below 0.1
MODE_MEASURED = {40.0: 0.024703018038808405, 50.0: 0.018028396675759707, 60.0: 0.014461548829689964}
MODE_BOUND = 2.0 * max(MODE_MEASURED.values())


def focus_profile(z):
    """c at the depths z: np.interp of focus_env's 5 m nodes, the piecewise-linear profile the fan is traced in"""
    zn = np.arange(0.0, 5001.0, 5.0)
    return np.interp(z, zn, cref.FOCUS_C0 * np.cosh((zn - cref.FOCUS_Z0) / cref.FOCUS_L))


def modes(f, dz=MODE_DZ):
    """(k (m,), psi (m, n), z (n,), w (m,)): the modes with k > (w / C0) cos 21 degrees on the interior grid z, normalised to
    sum psi^2 dz = 1, and their taper weights"""
    from scipy.linalg import eigh_tridiagonal
    n = int(round((MODE_WALLS[1] - MODE_WALLS[0]) / dz)) - 1
    z = MODE_WALLS[0] + dz * np.arange(1, n + 1)
    om = 2.0 * np.pi * f
    diag = (om / focus_profile(z)) ** 2 - 2.0 / dz ** 2
    k0 = om / cref.FOCUS_C0
    lo = (k0 * np.cos(np.radians(MODE_TAPER[1]))) ** 2
    k2, vec = eigh_tridiagonal(diag, np.full(n - 1, 1.0 / dz ** 2), select="v", select_range=(lo, 1.01 * k0 ** 2))
    k = np.sqrt(k2)
    psi = vec.T / np.sqrt((vec.T ** 2).sum(axis=1, keepdims=True) * dz)
    angle = np.degrees(np.arccos(np.minimum(k / k0, 1.0)))
    u = np.clip((angle - MODE_TAPER[0]) / (MODE_TAPER[1] - MODE_TAPER[0]), 0.0, 1.0)
    return k, psi, z, np.cos(0.5 * np.pi * u) ** 2


def modal_field(f, depths, ranges, dz=MODE_DZ, source_depth=cref.FOCUS_Z0):
    """p (len(depths), len(ranges)) complex of the far-field mode sum at the frequency f; NaN at r = 0"""
    k, psi, z, w = modes(f, dz)
    at = lambda d: np.array([np.interp(d, z, row) for row in psi])          # noqa: E731  (m, len(d))
    a = w * at(np.array([source_depth]))[:, 0]
    r = np.asarray(ranges, dtype=float)
    with np.errstate(divide="ignore", invalid="ignore"):
        spread = np.exp(1j * k[:, None] * r[None, :]) * np.sqrt(2.0 * np.pi / (k[:, None] * r[None, :]))
        p = np.exp(0.25j * np.pi) * ((a[:, None] * at(np.asarray(depths, dtype=float))).T @ spread)
    p[:, r == 0] = np.nan
    return p


def mode_cells(x):
    """(cells (len(MODE_DEPTHS), len(x)) bool, kappa (len(x),)): the comparison points -- columns beyond 3 km and more than 2 km
    from every focus n pi L, depths inside the fan with a 2 degree margin -- and the foci floor(x / pi L) the one ray there has
    passed"""
    x = np.asarray(x, dtype=float)
    focus = np.pi * cref.FOCUS_L
    kappa = np.floor(x / focus).astype(np.int64)
    col = (x > MODE_X_MIN) & (np.abs(x - focus * np.rint(x / focus)) > MODE_FOCUS_CLEAR)
    reach = cref.FOCUS_L * np.arcsinh(np.tan(np.radians(MODE_FAN_ANGLE)) * np.abs(np.sin(x / cref.FOCUS_L)))
    return col[None, :] & (np.abs(MODE_DEPTHS[:, None] - cref.FOCUS_Z0) < reach[None, :]), kappa


def check_mode_cells(cells, kappa):
    """the premises of the comparison: every kappa from 0 to 4 keeps at least 1000 cells"""
    per = [int(cells[:, kappa == n].sum()) for n in range(5)]
    assert kappa.max() == 4 and min(per) >= 1000, per
    return per


def mode_error(p, ref, cells):
    """e = |p - p_modes| / |p_modes| on the comparison cells, 0 elsewhere"""
    with np.errstate(invalid="ignore", divide="ignore"):
        return np.where(cells, np.abs(p - ref) / np.abs(ref), 0.0)


# ---- the isovelocity waveguide: Lloyd's mirror with a bottom ----------------------------------------------------------------
# c = 1500 m/s between a pressure-release surface and a rigid flat bottom at H = 1000 m, source at 300 m.  The images sit at
# 2 n H +- z_s; the straight line from an image to the receiver is the unfolded path, and it crosses the surface once for every
# level 2 m H between their depths (as test_bounce_log.py's image sum counts the bottom's levels (2 m + 1) H): the image adds
# (-1)^(n_s) e^{i k R} / R, the bottom +1.  Only the images inside the fan's +-40 degrees count.

GUIDE_C, GUIDE_H, GUIDE_ZTOP, GUIDE_ZS, GUIDE_X1, GUIDE_S, GUIDE_N, GUIDE_APERTURE = 1500.0, 1000.0, 1200.0, 300.0, 5e3, 51, 4001, 40.0
GUIDE_F, GUIDE_K = 50.0, 8                                   # Hz; the bounce log's slots
GUIDE_DEPTHS = np.arange(75.0, 926.0, 50.0)
GUIDE_COLS = np.array([10, 20, 30, 40, 50])                   # the save columns at 1, 2, 3, 4, 5 km
GUIDE_EDGE = 0.5                                             # degrees: a cell with an image this close to the aperture's edge is left out
GUIDE_BAND = np.linspace(40.0, 60.0, 5)
GUIDE_B, GUIDE_DT, GUIDE_NT, GUIDE_LEAD = 20.0, 4e-3, 352, 0.15
# the worst e = |p - p_ref| / sqrt(sum 1 / R^2) of the restatements on the CPU oracle's fan: cref.fan_pressure at 50 Hz,
# spectrum_reference.spectrum_sum over GUIDE_BAND with t_reduce = x / c, signal_reference.signal_sum over every sample
GUIDE_MEASURED = 0.00012985387768344752
GUIDE_BAND_MEASURED = 0.0001298538776663307
GUIDE_PULSE_MEASURED = 8.676346210685428e-05
GUIDE_BOUND, GUIDE_BAND_BOUND, GUIDE_PULSE_BOUND = 2.0 * GUIDE_MEASURED, 2.0 * GUIDE_BAND_MEASURED, 2.0 * GUIDE_PULSE_MEASURED


def guide_env(pr):
    z = np.arange(0.0, GUIDE_ZTOP + 1.0, 10.0)
    r = np.linspace(0.0, 10e3, 5)
    ssp = pr.DataArray(np.full((len(r), len(z)), GUIDE_C), dims=["range", "depth"], coords={"range": r, "depth": z})
    bathy = pr.DataArray(np.full(len(r), GUIDE_H), dims=["range"], coords={"range": r})
    return pr.OceanEnvironment2D(ssp, bathy, flat_earth_transform=False)


def guide_angles(n=GUIDE_N):
    return np.linspace(-GUIDE_APERTURE, GUIDE_APERTURE, n)


def guide_strip(x):
    """the width of the strip along either boundary in which arrivals are missing: a bounce counts from the nearest save column,
    and before its bounce the sample there is the reflected segment continued backwards, up to tan(theta_max) dx / 2 beyond the
    boundary (DESIGN.md sections 14 and 16)"""
    return np.tan(np.radians(GUIDE_APERTURE)) * 0.5 * np.diff(np.asarray(x, dtype=float)).max()


def guide_images(x, depths=GUIDE_DEPTHS):
    """the images seen from the receivers `depths` at the ranges x -> (R, sign, inside, keep): distances and (-1)^(n_s), each
    (len(depths), len(x), images), whether the image lies inside the aperture, and keep (len(depths), len(x)): no image within
    GUIDE_EDGE degrees of the aperture's edge"""
    X = np.asarray(x, dtype=float)[None, :, None]
    D = np.asarray(depths, dtype=float)[:, None, None]
    H = GUIDE_H
    nmax = int(np.ceil(np.tan(np.radians(GUIDE_APERTURE)) * X.max() / (2 * H))) + 2
    n = np.arange(-nmax, nmax + 1)
    zi = np.concatenate([2 * n * H + GUIDE_ZS, 2 * n * H - GUIDE_ZS])[None, None, :]
    lo, hi = np.minimum(zi, D), np.maximum(zi, D)
    n_s = np.maximum(np.floor(hi / (2 * H)) - np.ceil(lo / (2 * H)) + 1, 0)          # the levels 2 m H in [lo, hi]
    angle = np.degrees(np.arctan2(np.abs(zi - D), X))
    R = np.hypot(X, zi - D)
    return R, 1.0 - 2.0 * (n_s % 2), angle <= GUIDE_APERTURE, (np.abs(angle - GUIDE_APERTURE) >= GUIDE_EDGE).all(axis=2)


def check_guide_cells(x):
    """the premises: at most a fifth of the cells is left out, the others see up to 9 images, and every receiver stays outside
    the strip along the boundaries -> keep"""
    R, sign, inside, keep = guide_images(x)
    assert 1.0 - keep.mean() <= 0.2, keep.sum()
    seen = inside.sum(axis=2)[keep]
    assert seen.max() == 9 and seen.min() >= 1 and (seen >= 5).mean() > 0.5
    full = np.linspace(0.0, GUIDE_X1, GUIDE_S)
    assert GUIDE_DEPTHS.min() > guide_strip(full) and GUIDE_DEPTHS.max() < GUIDE_H - guide_strip(full)
    return keep


def _norm(R, inside):
    return np.sqrt(np.where(inside, 1.0 / R ** 2, 0.0).sum(axis=2))


def waveguide_field(f, depths, x):
    """the CW image sum at the frequency f -> complex (len(depths), len(x))"""
    R, sign, inside, _ = guide_images(x, depths)
    k = 2.0 * np.pi * f / GUIDE_C
    return np.where(inside, sign * np.exp(1j * k * R) / R, 0.0).sum(axis=2)


def guide_error(p, x, f=GUIDE_F):
    """p (len(GUIDE_DEPTHS), len(x)) complex -> e, the error against the image sum in units of the incoherent amplitude, on the
    cells kept (0 elsewhere)"""
    R, sign, inside, keep = guide_images(x)
    return np.where(keep, np.abs(p - waveguide_field(f, GUIDE_DEPTHS, x)) / _norm(R, inside), 0.0)


def guide_band_error(Hf, x, freq=GUIDE_BAND):
    """Hf (len(GUIDE_DEPTHS), len(x), len(freq)), the transfer function with t_reduce = x / c per column -> e (same shape)
    against sum +- e^{i 2 pi f (R / c - x / c)} / R"""
    R, sign, inside, keep = guide_images(x)
    tau = (R - np.asarray(x, dtype=float)[None, :, None]) / GUIDE_C
    ref = np.stack([np.where(inside, sign * np.exp(2j * np.pi * f * tau) / R, 0.0).sum(axis=2) for f in freq], axis=2)
    return np.where(keep[:, :, None], np.abs(Hf - ref) / _norm(R, inside)[:, :, None], 0.0)


def guide_t0(x):
    """the start time per column: GUIDE_LEAD before x / c"""
    return np.asarray(x, dtype=float) / GUIDE_C - GUIDE_LEAD


def guide_pulse_error(u, x):
    """u (len(GUIDE_DEPTHS), len(x), GUIDE_NT) complex on the time axes guide_t0(x) + n GUIDE_DT -> e (same shape) against
    sum +- (1 / R) exp(-(t - R / c)^2 / (2 sigma^2)) e^{i 2 pi f R / c}, the envelope cut at 8 sigma as received_signal cuts it"""
    R, sign, inside, keep = guide_images(x)
    sigma = sref.pulse_sigma(GUIDE_B)
    k = 2.0 * np.pi * GUIDE_F / GUIDE_C
    amp = np.where(inside, sign * np.exp(1j * k * R) / R, 0.0)
    t = guide_t0(x)[None, :, None] + (np.arange(GUIDE_NT) * GUIDE_DT)[None, None, :]
    ref = np.zeros((len(GUIDE_DEPTHS), len(x), GUIDE_NT), complex)
    for i in np.flatnonzero(inside.any(axis=(0, 1))):
        tau = t - (R[:, :, i] / GUIDE_C)[:, :, None]
        ref = ref + amp[:, :, i, None] * np.where(np.abs(tau) <= 8.0 * sigma, np.exp(-tau ** 2 / (2.0 * sigma ** 2)), 0.0)
    return np.where(keep[:, :, None], np.abs(u - ref) / _norm(R, inside)[:, :, None], 0.0)


def check_guide_pulse(x):
    """the premises of the pulse test: every image's pulse lies on the time axis with its 8 sigma, somewhere two images overlap
    (less than one sigma apart) and somewhere neighbours in time are resolved (more than 16 sigma apart: their cut envelopes do
    not touch)"""
    R, sign, inside, keep = guide_images(x)
    sigma = sref.pulse_sigma(GUIDE_B)
    T = np.where(inside & keep[:, :, None], R / GUIDE_C, np.nan)
    rel = T - guide_t0(x)[None, :, None]
    assert np.nanmin(rel) > 8.0 * sigma and np.nanmax(rel) < (GUIDE_NT - 1) * GUIDE_DT - 8.0 * sigma, (np.nanmin(rel), np.nanmax(rel))
    gaps = np.diff(np.sort(T, axis=2), axis=2)
    assert np.nanmin(gaps) < sigma and np.nanmax(gaps) > 16.0 * sigma, (np.nanmin(gaps), np.nanmax(gaps), sigma)
