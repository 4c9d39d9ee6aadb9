"""Test helpers for band_intensity / band_transmission_loss (not a product path): DESIGN.md section 23 restated in plain NumPy in
its operation order -- spectrum_reference.spectrum_sum's (re, im) per frequency (with a lag reflection_reference's twin),
P = re re + im im, the 64 lane partials in increasing k and the xor tree -- and the set-up shared by the CPU and GPU tests:
Lloyd's mirror over a band on section 20's exact straight rays, with the errors measured on the CPU
(tests/test_band_host.py prints them)."""
import numpy as np

import arrivals_reference as aref
import beam_arrivals_reference as baref
import beam_pressure_reference as bp
import reflection_reference as rref
import spectrum_reference as spref

LANES = 64


def band_terms(off, T, I, q, phi, L, freq, alpha):
    """(re, im), each (G, F): the sums of pgr_spectrum_device with tred = 0.0, with phi those of pgr_spectrum_device_phi"""
    zero = np.zeros(len(off) - 1)
    if phi is None:
        H = spref.spectrum_sum(off, T, I, q, L, zero, freq, alpha)
    else:
        H = rref.spectrum_sum(off, T, I, q, phi, L, zero, freq, alpha)
    return H.real, H.imag


def reduce_band(re, im, wf):
    """re, im (G, F) and the weights wf (F,) -> out (G,): P_k, the lane partials s_l over k = l, l + 64, ... in increasing k, the
    six exchanges of the xor tree on all 64 lanes at once, lane 0"""
    re, im, wf = np.asarray(re, dtype=float), np.asarray(im, dtype=float), np.asarray(wf, dtype=float)
    G, F = re.shape
    with np.errstate(invalid="ignore", over="ignore"):
        rr, ii = re * re, im * im
        P = rr + ii
        s = np.zeros((G, LANES))
        for k in range(F):
            s[:, k % LANES] = s[:, k % LANES] + wf[k] * P[:, k]
        lane = np.arange(LANES)
        for d in (32, 16, 8, 4, 2, 1):
            s = s + s[:, lane ^ d]
    return s[:, 0].copy()


def band_power(off, T, I, q, phi, L, freq, alpha, wf):
    """The definition, restated -> out (G,) float64"""
    re, im = band_terms(off, T, I, q, phi, L, freq, alpha)
    return reduce_band(re, im, wf)


# ---- Lloyd's mirror over a band, on section 20's exact straight rays ------------------------------------------------------------
# beam_pressure_reference's set-up: isovelocity 1500 m/s under a pressure-release surface, source at 200 m, receivers 75 ... 925 m
# every 50 m at 2, 3, 4, 5 km, 4001 straight rays over +-40 degrees, folded tubes left out (q = -1).  The band: 64 frequencies
# over 60 ... 90 Hz, uniform weights.  The yardstick is formed per frequency from the geometry alone.

BAND_FREQ = np.linspace(60.0, 90.0, 64)
BAND_UNIFORM = np.full(64, 1.0 / 64)
BAND_COLS = [1, 2, 3, 4]
# the worst e = |P - P_closed| / (1 / R1^2 + 1 / R2^2) over all 18 x 4 cells of the restatement, on the tube list and on the beam
# list at min_width 10 m with curvature (tests/test_band_host.py prints them); the bounds are twice them (DESIGN.md section 19's
# rule: the margin covers the GPU's table look-up)
BAND_LLOYD_MEASURED = 7.752283883245613e-05
BAND_LLOYD_BEAM_MEASURED = 0.00026605304657624024


def spectrum_shaped_weights():
    """a non-uniform source spectrum over BAND_FREQ, summing to 1: a ramp that weighs 90 Hz nine times 60 Hz"""
    w = np.linspace(1.0, 9.0, len(BAND_FREQ))
    return w / w.sum()


def lloyd_paths(source_depth=bp.LLOYD_ZS, depths=bp.LLOYD_DEPTHS, ranges=bp.EXACT_RANGES):
    D, X = np.asarray(depths, dtype=float)[:, None], np.asarray(ranges, dtype=float)[None, :]
    return np.hypot(X, D - source_depth), np.hypot(X, D + source_depth)


def lloyd_band_closed(wf, freq=BAND_FREQ, surface=-1.0):
    """sum_k w_k |e^{2 pi i f_k R1 / c} / R1 + surface e^{2 pi i f_k R2 / c} / R2|^2 per cell (len(depths), len(ranges)), formed
    frequency by frequency; `surface` -1: the pressure-release surface's half cycle"""
    R1, R2 = lloyd_paths()
    P = np.zeros(R1.shape)
    for w, f in zip(wf, freq):
        H = np.exp(2j * np.pi * f * R1 / bp.EXACT_C) / R1 + surface * np.exp(2j * np.pi * f * R2 / bp.EXACT_C) / R2
        P = P + w * np.abs(H) ** 2
    return P


def lloyd_band_error(P, wf, freq=BAND_FREQ):
    """e (len(depths), len(ranges)) of a band power P against the closed form, in units of the incoherent power"""
    R1, R2 = lloyd_paths()
    return np.abs(P - lloyd_band_closed(wf, freq)) / (1.0 / R1 ** 2 + 1.0 / R2 ** 2)


def exact_tube_lists():
    """the ray-tube arrivals of beam_pressure_reference.exact_fan at the Lloyd receivers and the four ranges ->
    (offsets, T, I, q per arrival)"""
    zs, ps, ts, x, p0, q = bp.exact_fan(bp.LLOYD_ZS)
    a = aref.tube_arrivals(zs, ps, ts, x, p0, bp.LLOYD_DEPTHS, BAND_COLS, bp.EXACT_CIN, bp.EXACT_RIN, bp.EXACT_ZIN)
    slot = np.repeat(np.arange(len(a["offsets"]) - 1), np.diff(a["offsets"])) % len(BAND_COLS)
    return a["offsets"], a["T"], a["I"], q[a["tube"], np.asarray(BAND_COLS)[slot]]


def exact_beam_lists(w_min=10.0, curvature=True):
    """the beam arrivals of the same fan -> (offsets, T, I = amplitude * amplitude, q)"""
    b = baref.exact_lloyd_arrivals(w_min, curvature)
    return b["offsets"], b["time"], b["amplitude"] * b["amplitude"], b["q"]


def as_cells(out):
    return np.asarray(out).reshape(len(bp.LLOYD_DEPTHS), len(BAND_COLS))
