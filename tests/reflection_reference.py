"""Test helpers for the complex bottom reflection (not a product path): DESIGN.md section 19 restated in plain NumPy, written from
the definition and independently of pygenray_amd/reflection.py -- the Rayleigh coefficient of a fluid half-space, the lag every ray
has collected at its bottom bounces (bounce_reference's accumulation with the lag table in the bottom's slot), the three coherent
sums with a lag per arrival on coherent_reference / signal_reference / spectrum_reference, and the image sum of wave_reference's
waveguide with R(theta)^(n_b) per image -- with the set-ups shared by the CPU and GPU tests and the errors measured on the CPU
oracle's fan (tests/test_reflection_host.py prints them).

The image sum is the RAY-THEORETIC one with the plane-wave coefficient: every image carries R at its own grazing angle once per
bottom level it crosses.  It is not the exact Pekeris solution -- beam displacement and the lateral wave are in neither side."""
import numpy as np

import arrivals_reference as aref
import bounce_reference as bref
import coherent_reference as cref
import path_reference as pref
import signal_reference as sref
import spectrum_reference as spref
import wave_reference as wref
from beam_reference import gexp

# ---- the Rayleigh coefficient -------------------------------------------------------------------------------------------------

NEPER_PER_DB_WAVELENGTH = 1.0 / (40.0 * np.pi * np.log10(np.e))


def rayleigh(grazing_deg, c_b, rho_b, att=0.0, c_w=1500.0, rho_w=1000.0):
    """R of a fluid half-space at the grazing angles given, from the vertical wavenumbers (in units of w / c_w): kw = sin(theta)
    in the water, kb = sqrt(n^2 - cos^2(theta)) in the bottom with Im kb >= 0 (the wave decays downwards), n = c_w / c_b with the
    attenuation in dB per wavelength as the index's imaginary part; R = (rho_b kw - rho_w kb) / (rho_b kw + rho_w kb), time
    dependence e^{-i w t}"""
    th = np.radians(np.asarray(grazing_deg, dtype=float))
    n = (c_w / c_b) * (1.0 + 1j * att * NEPER_PER_DB_WAVELENGTH)
    kw = np.sin(th).astype(complex)
    kb = np.sqrt(n * n - np.cos(th) ** 2 + 0j)
    kb = np.where(kb.imag < 0.0, -kb, kb)
    return (rho_b * kw - rho_w * kb) / (rho_b * kw + rho_w * kb)


def critical_angle(c_b, c_w=1500.0):
    return np.degrees(np.arccos(c_w / c_b))


# ---- the accumulated lag ------------------------------------------------------------------------------------------------------

def ray_lags(bx, bp, bk, x, cin, rin, zin, br, bd, lag_table, beta, psign=-1.0):
    """Phi (M, S): the lag in cycles every ray has collected at the bottom bounces that precede each save column -- section 14's
    accumulation with the lag table in the bottom's slot and 0.0 for the surface: bounce_reference's per-event value (the same
    event angle and table rule) and sample assignment, the running sum from 0.0 in bounce order (np.cumsum adds one event at a
    time, in order).  bounce_reference.boundary_loss is this with Python loops; test_reflection_host.py compares the two."""
    bk = np.asarray(bk)
    M, K = bk.shape
    S = len(x)
    lag = bref.event_loss(bx, bp, bk, cin, rin, zin, br, bd, lag_table, (None, np.zeros(1)), beta, psign)
    j = bref.sample_index(np.asarray(x, dtype=float), bx)
    E = np.where((bk >= 0).all(axis=1), K, np.argmax(bk < 0, axis=1))                    # the leading slots with an event
    live = np.arange(K)[None, :] < E[:, None]
    run = np.concatenate([np.zeros((M, 1)), np.cumsum(np.where(live, lag, 0.0), axis=1)], axis=1)
    seg = (live[:, :, None] & (j[:, :, None] <= np.arange(S)[None, None, :])).sum(axis=1)
    seg[:, S - 1] = E
    return np.take_along_axis(run, seg, axis=1)


def arrival_lag(P0, P1, w):
    """phi_a from the edge rays' lags and the arrival's w: subtract, multiply, add"""
    d = P1 - P0
    d = w * d
    return P0 + d


def turn_back(t, phi):
    """the two operations the sums add behind their own t = t - rint(t): r = phi - rint(phi); t = t - r; t = t - rint(t)"""
    r = phi - np.rint(phi)
    t = t - r
    return t - np.rint(t)


# ---- the three sums -----------------------------------------------------------------------------------------------------------

def tube_pressure(zs, ps, ts, x, p0, depths, cin, rin, zin, W, q, f, Phi):
    """coherent_reference.tube_pressure with Phi (M, S), the rays' lag in cycles: the arrival of tube k takes
    arrival_lag(Phi_k, Phi_k+1, w) and its phase is turned back by it -> (re, im), each (len(depths), S)"""
    depths = np.asarray(depths, dtype=float)
    ts, Phi = np.asarray(ts, dtype=float), np.asarray(Phi, dtype=float)
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
            t = turn_back(cref.phase_cycles(T, qk[None, :], f), arrival_lag(Phi[k][None, :], Phi[k + 1][None, :], w))
            re = np.where(hit, re + a * cref.gcos2pi(t), re)
            im = np.where(hit, im + a * cref.gsin2pi(t), im)
    re[:, r == 0] = np.nan
    im[:, r == 0] = np.nan
    return re, im


def arrival_terms(T, I, q, f, phi):
    """signal_reference.arrival_terms with a lag per arrival: (amp * cv, amp * sv, adds)"""
    T, I = np.asarray(T, dtype=float), np.asarray(I, dtype=float)
    q = np.zeros(len(T), np.int64) if q is None else np.asarray(q).astype(np.int64)
    with np.errstate(invalid="ignore"):
        amp = np.sqrt(I)
        ph = turn_back(cref.phase_cycles(T, q, f), np.asarray(phi, dtype=float))
        return amp * cref.gcos2pi(ph), amp * cref.gsin2pi(ph), q >= 0


def signal_sum(off, T, I, q, phi, tstart, f, rs, dt, n_times):
    """signal_reference.signal_sum with a lag per arrival -> u (G, n_times) complex"""
    off = np.asarray(off, dtype=np.int64)
    T = np.asarray(T, dtype=float)
    G = len(off) - 1
    C, Sn, adds = arrival_terms(T, I, q, f, phi)
    t = sref.sample_times(tstart, dt, n_times)
    re, im = np.zeros((G, n_times)), np.zeros((G, n_times))
    cnt = np.diff(off)
    with np.errstate(invalid="ignore", over="ignore"):
        for rank in range(int(cnt.max()) if G else 0):
            g = np.flatnonzero(cnt > rank)
            a = off[g] + rank
            x = (t[g] - T[a][:, None]) * rs
            v = x * x
            keep = adds[a][:, None] & (v <= sref.CUT)
            E = gexp(-0.5 * np.where(keep, v, 0.0))
            re[g] = np.where(keep, re[g] + C[a][:, None] * E, re[g])
            im[g] = np.where(keep, im[g] + Sn[a][:, None] * E, im[g])
    return cref.as_complex(re, im)


def cw_sum(off, T, I, q, phi, f):
    """signal_reference.cw_sum with a lag per arrival -> (G,) complex"""
    C, Sn, adds = arrival_terms(T, I, q, f, phi)
    off = np.asarray(off, dtype=np.int64)
    out = np.zeros(len(off) - 1, complex)
    for g in range(len(off) - 1):
        re = im = 0.0
        for a in range(off[g], off[g + 1]):
            if adds[a]:
                re, im = re + C[a], im + Sn[a]
        out[g] = complex(re, im)
    return out


def spectrum_sum(off, T, I, q, phi, L, tred, freq, alpha):
    """spectrum_reference.spectrum_sum with a lag per arrival -> H (G, F) complex"""
    off = np.asarray(off, dtype=np.int64)
    T, I, phi = np.asarray(T, dtype=float), np.asarray(I, dtype=float), np.asarray(phi, dtype=float)
    freq, tred = np.asarray(freq, dtype=float), np.asarray(tred, dtype=float)
    assert (L is None) == (alpha is None)
    G, F = len(off) - 1, len(freq)
    qq = np.zeros(len(T), np.int64) if q is None else np.asarray(q).astype(np.int64)
    re, im = np.zeros((G, F)), np.zeros((G, F))
    cnt = np.diff(off)
    with np.errstate(invalid="ignore", over="ignore"):
        amp = np.sqrt(I)
        for rank in range(int(cnt.max()) if G else 0):
            g = np.flatnonzero(cnt > rank)
            a = off[g] + rank
            g, a = g[qq[a] >= 0], a[qq[a] >= 0]
            tau = T[a] - tred[g]
            ph = turn_back(cref.phase_cycles(tau[:, None], qq[a][:, None], freq[None, :]), phi[a][:, None])
            cv, sv = cref.gcos2pi(ph), cref.gsin2pi(ph)
            if alpha is None:
                re[g] = re[g] + amp[a][:, None] * cv
                im[g] = im[g] + amp[a][:, None] * sv
            else:
                W = spref.amplitude_weight(np.asarray(alpha, dtype=float)[None, :], np.asarray(L, dtype=float)[a][:, None])
                re[g] = re[g] + (amp[a][:, None] * cv) * W
                im[g] = im[g] + (amp[a][:, None] * sv) * W
    return cref.as_complex(re, im)


# ---- synthetic inputs of the GPU tests ----------------------------------------------------------------------------------------

def synthetic_lags(shape, seed):
    """lags in cycles: most within +-3, exact zeros, whole cycles, values beyond +-1e3, and (sizes allowing) one NaN"""
    rng = np.random.default_rng(seed)
    phi = rng.uniform(-3.0, 3.0, shape)
    pick = rng.random(shape)
    phi[pick < 0.10] = 0.0
    phi[(pick >= 0.10) & (pick < 0.15)] = 2.0
    phi[(pick >= 0.15) & (pick < 0.20)] = 1e3 * (1.0 + rng.random(int(((pick >= 0.15) & (pick < 0.20)).sum())))
    phi[(pick >= 0.20) & (pick < 0.25)] = -4e3 * (1.0 + rng.random(int(((pick >= 0.20) & (pick < 0.25)).sum())))
    flat = phi.reshape(-1)
    if flat.size:
        flat[0] = -1234.625
    if flat.size >= 3:
        flat[1], flat[2] = 0.0, 5678.3
    if flat.size >= 16:
        flat[flat.size // 2 + 1] = np.nan
    return phi


# ---- fans ---------------------------------------------------------------------------------------------------------------------

def fan_frame(rays, environment, flatearth=True):
    """(x in the traced frame, cin, rin, zin, bottom ranges, bottom depths, bottom angles, p0) of a host fan, as
    coherent_reference.fan_pressure prepares them"""
    from pygenray_amd.environment import _mirror_envi_arrays, _unpack_envi
    from pygenray_amd.host_physics import bilinear_interp
    from pygenray_amd.launch_rays import _initial_slowness
    x = np.asarray(rays.rs, dtype=float)[0]
    cin, cpin, rin, zin, bd, br, ba = _unpack_envi(environment, flatearth=flatearth)
    if len(x) > 1 and x[-1] < x[0]:
        cin, cpin, rin, bd, br, ba = _mirror_envi_arrays(cin, cpin, rin, bd, br, ba)
        x = -x
    c_source = bilinear_interp(x[0], float(rays.source_depths[0]), rin, zin, cin)
    return x, cin, rin, zin, br, bd, ba, _initial_slowness(rays.thetas, c_source)


def fan_pressure(rays, depths, environment, f, Phi, flatearth=True, W=None, nb=None, ns=None):
    """pressure_field's definition with a complex bottom on a host fan: coherent_reference.fan_pressure with the rays' lags
    Phi (M, S) -> complex (R, S)"""
    x, cin, rin, zin, _, _, _, p0 = fan_frame(rays, environment, flatearth)
    q = cref.tube_phase(cref.caustic_index(-np.asarray(rays.zs), nb, ns), nb, ns)
    re, im = tube_pressure(rays.zs, rays.ps, rays.ts, x, p0, depths, cin, rin, zin, W, q, f, Phi)
    return cref.as_complex(re, im)


def fan_arrivals(rays, depths, environment, cols, Phi, flatearth=True, nb=None, ns=None):
    """signal_reference.fan_arrivals and every arrival's lag from the rays' lags Phi (M, S) -> (off, T, I, q, phi)"""
    a = aref.fan_arrivals(rays, depths, environment, cols, flatearth)
    qfull = cref.tube_phase(cref.caustic_index(-np.asarray(rays.zs), nb, ns), nb, ns)
    slot = np.repeat(np.arange(len(a["offsets"]) - 1), np.diff(a["offsets"])) % len(cols)
    col = np.asarray(cols)[slot]
    k = a["tube"].astype(np.int64)
    return a["offsets"], a["T"], a["I"], qfull[k, col], arrival_lag(Phi[k, col], Phi[k + 1, col], a["w"])


# ---- the isovelocity waveguide over a fluid half-space --------------------------------------------------------------------------
# wave_reference's guide unchanged (c = 1500 m/s, H = 1000 m, source at 300 m, 4001 rays +-40 degrees, 51 save ranges to 5 km, a
# log of 8 slots, 50 Hz, receivers 75 ... 925 m at 1 ... 5 km) over a sand-like bottom: 1700 m/s, 1800 kg/m^3, 0.5 dB per
# wavelength.  The unfolded path of an image crosses the bottom once for every level (2 m + 1) H between the image's depth and
# the receiver's, each time at the image's own grazing angle: the image adds (-1)^(n_s) R(theta)^(n_b) e^{i k R} / R.

GUIDE_BOTTOM = (1700.0, 1800.0, 0.5)             # sound speed m/s, density kg/m^3, attenuation dB per wavelength
GUIDE_CRITICAL = 28.07                           # degrees: acos(1500 / 1700)
GUIDE_KEPT, GUIDE_SUBCRITICAL = 74, 44           # cells the edge rule keeps; those of them with a bottom image 1 degree below critical
# the worst e = |p - p_ref| / sqrt(sum 1 / R^2) over the kept cells of the restatements on the CPU oracle's fan: the tube sum at
# 50 Hz, the band sum over wave_reference.GUIDE_BAND with t_reduce = x / c, the pulse sum with the guide's pulse
# (tests/test_reflection_host.py prints them); the bounds are twice them (DESIGN.md section 16's rule)
GUIDE_MEASURED = 0.00033131177037807057
GUIDE_BAND_MEASURED = 0.0003928383547143986
GUIDE_PULSE_MEASURED = 0.0003231643976981109

# what the bottom could wrongly have been taken for: name -> the coefficient in R's place
WRONG_BOTTOMS = {"rigid": lambda R: np.ones_like(R), "magnitude without the phase": lambda R: np.abs(R) + 0j,
                 "conjugate phase": np.conj, "pressure release": lambda R: -np.ones_like(R)}
# the least e of each on the subcritical cells, from the closed forms alone (the right image sum against the wrong one)
WRONG_AT_LEAST = {"rigid": 0.084, "magnitude without the phase": 0.127, "conjugate phase": 0.278, "pressure release": 0.094}


def guide_bounds():
    return 2.0 * GUIDE_MEASURED, 2.0 * GUIDE_BAND_MEASURED, 2.0 * GUIDE_PULSE_MEASURED


def guide_bottom_images(x, depths=wref.GUIDE_DEPTHS, coefficient=None):
    """wave_reference.guide_images with the bottom's factor: (R, amp, inside, keep, n_b, angle) -- amp (len(depths), len(x),
    images) complex = (-1)^(n_s) C^(n_b), C = coefficient(rayleigh at the image's grazing angle) (None: R itself), n_b the levels
    (2 m + 1) H in [lo, hi] of the image's and the receiver's depths"""
    R, sign, inside, keep = wref.guide_images(x, depths)
    X = np.asarray(x, dtype=float)[None, :, None]
    D = np.asarray(depths, dtype=float)[:, None, None]
    H = wref.GUIDE_H
    nmax = int(np.ceil(np.tan(np.radians(wref.GUIDE_APERTURE)) * X.max() / (2 * H))) + 2
    n = np.arange(-nmax, nmax + 1)
    zi = np.concatenate([2 * n * H + wref.GUIDE_ZS, 2 * n * H - wref.GUIDE_ZS])[None, None, :]
    assert np.array_equal(np.hypot(X, zi - D), R)                       # (the same images in the same order)
    lo, hi = np.minimum(zi, D), np.maximum(zi, D)
    n_b = np.maximum(np.floor((hi - H) / (2 * H)) - np.ceil((lo - H) / (2 * H)) + 1, 0).astype(np.int64)
    n_b = np.broadcast_to(n_b, R.shape)
    angle = np.degrees(np.arctan2(np.abs(zi - D), X))
    C = rayleigh(angle, *GUIDE_BOTTOM, c_w=wref.GUIDE_C)
    if coefficient is not None:
        C = coefficient(C)
    return R, sign * C ** n_b, inside, keep, n_b, angle


def check_guide_bottom_cells(x):
    """the premises: the edge rule (geometry only) keeps 74 of the 90 cells, its cap of one fifth left out holds, and 44 of the
    74 see an image that has bounced off the bottom at least 1 degree below the critical angle -> (keep, subcritical)"""
    R, amp, inside, keep, n_b, angle = guide_bottom_images(x)
    assert abs(critical_angle(GUIDE_BOTTOM[0], wref.GUIDE_C) - GUIDE_CRITICAL) < 0.005
    assert keep.size == 90 and int(keep.sum()) == GUIDE_KEPT and 1.0 - keep.mean() <= 0.2
    sub = keep & (inside & (n_b >= 1) & (angle <= GUIDE_CRITICAL - 1.0)).any(axis=2)
    assert int(sub.sum()) == GUIDE_SUBCRITICAL, int(sub.sum())
    return keep, sub


def _norm(R, inside):
    return np.sqrt(np.where(inside, 1.0 / R ** 2, 0.0).sum(axis=2))


def guide_field(x, f=wref.GUIDE_F, coefficient=None):
    """the CW image sum over the fluid bottom -> complex (len(GUIDE_DEPTHS), len(x))"""
    R, amp, inside, _, _, _ = guide_bottom_images(x, coefficient=coefficient)
    k = 2.0 * np.pi * f / wref.GUIDE_C
    return np.where(inside, amp * np.exp(1j * k * R) / R, 0.0).sum(axis=2)


def guide_error(p, x, coefficient=None):
    """p (len(GUIDE_DEPTHS), len(x)) complex at 50 Hz -> e against the image sum, in units of the incoherent amplitude of the
    rigid guide's images (geometry only), on the cells kept (0 elsewhere)"""
    R, amp, inside, keep, _, _ = guide_bottom_images(x)
    return np.where(keep, np.abs(p - guide_field(x, coefficient=coefficient)) / _norm(R, inside), 0.0)


def guide_band_error(Hf, x, freq=wref.GUIDE_BAND):
    """Hf (len(GUIDE_DEPTHS), len(x), len(freq)), the transfer function with t_reduce = x / c per column -> e (same shape)"""
    R, amp, inside, keep, _, _ = guide_bottom_images(x)
    tau = (R - np.asarray(x, dtype=float)[None, :, None]) / wref.GUIDE_C
    ref = np.stack([np.where(inside, amp * np.exp(2j * np.pi * f * tau) / R, 0.0).sum(axis=2) for f in freq], axis=2)
    return np.where(keep[:, :, None], np.abs(Hf - ref) / _norm(R, inside)[:, :, None], 0.0)


def guide_pulse_error(u, x):
    """u (len(GUIDE_DEPTHS), len(x), GUIDE_NT) complex on the time axes guide_t0(x) + n GUIDE_DT -> e (same shape), the envelope
    cut at 8 sigma as received_signal cuts it"""
    R, amp, inside, keep, _, _ = guide_bottom_images(x)
    sigma = sref.pulse_sigma(wref.GUIDE_B)
    k = 2.0 * np.pi * wref.GUIDE_F / wref.GUIDE_C
    a = np.where(inside, amp * np.exp(1j * k * R) / R, 0.0)
    t = wref.guide_t0(x)[None, :, None] + (np.arange(wref.GUIDE_NT) * wref.GUIDE_DT)[None, None, :]
    ref = np.zeros((len(wref.GUIDE_DEPTHS), len(x), wref.GUIDE_NT), complex)
    for i in np.flatnonzero(inside.any(axis=(0, 1))):
        tau = t - (R[:, :, i] / wref.GUIDE_C)[:, :, None]
        ref = ref + a[:, :, i, None] * np.where(np.abs(tau) <= 8.0 * sigma, np.exp(-tau ** 2 / (2.0 * sigma ** 2)), 0.0)
    return np.where(keep[:, :, None], np.abs(u - ref) / _norm(R, inside)[:, :, None], 0.0)
