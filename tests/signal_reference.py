"""Test helpers for received_signal (not a product path): a plain NumPy restatement of DESIGN.md section 17, written from the
definition -- the sum over each group's arrivals at every time sample, in the kernel's operation order and without
contraction -- on coherent_reference's phase_cycles / gcos2pi / gsin2pi and beam_reference's gexp, and the set-ups shared by
the CPU and GPU tests (the Fourier identity, Lloyd's mirror with a pulse)."""
import math

import numpy as np

import coherent_reference as cref
from beam_reference import gexp

CUT = 64.0                                   # v = ((t - T) / sigma)^2 <= 64: the envelope is cut at 8 sigma


def pulse_sigma(B):
    """sigma of the Gaussian envelope whose spectrum has the half-power full bandwidth B"""
    return math.sqrt(math.log(2.0)) / (math.pi * B)


def inv_sigma(B):
    """rs = 1 / sigma as received_signal forms it: pi B / sqrt(ln 2), 0.0 for B = 0"""
    return math.pi * B / math.sqrt(math.log(2.0))


def sample_times(tstart, dt, n_times):
    """t_n = tstart[g] + (double)n * dt -> (G, n_times)"""
    return np.asarray(tstart, dtype=float)[:, None] + (np.arange(n_times).astype(float) * dt)[None, :]


def arrival_terms(T, I, q, f):
    """per arrival: (amp * cv, amp * sv, adds) -- the constants of the definition and whether q lets the arrival add"""
    T, I = np.asarray(T, dtype=float), np.asarray(I, dtype=float)
    q = np.zeros(len(T), np.int64) if q is None else np.asarray(q).astype(np.int64)
    with np.errstate(invalid="ignore"):
        amp = np.sqrt(I)
        ph = cref.phase_cycles(T, q, f)
        return amp * cref.gcos2pi(ph), amp * cref.gsin2pi(ph), q >= 0


def signal_sum(off, T, I, q, tstart, f, rs, dt, n_times):
    """The definition, restated: groups [off[g], off[g + 1]) of arrivals T / I / q (q None: all zero), start times tstart (G,)
    -> u (G, n_times) complex.  A loop over the rank of an arrival within its group, vectorised over groups and samples: each
    sample's sums are formed from 0.0 one arrival at a time, in order."""
    off = np.asarray(off, dtype=np.int64)
    T = np.asarray(T, dtype=float)
    G = len(off) - 1
    C, Sn, adds = arrival_terms(T, I, q, f)
    t = sample_times(tstart, dt, n_times)
    re, im = np.zeros((G, n_times)), np.zeros((G, n_times))
    cnt = np.diff(off)
    with np.errstate(invalid="ignore", over="ignore"):
        for rank in range(int(cnt.max()) if G else 0):
            g = np.flatnonzero(cnt > rank)
            a = off[g] + rank
            x = (t[g] - T[a][:, None]) * rs
            v = x * x
            keep = adds[a][:, None] & (v <= CUT)                       # (False for a NaN v)
            E = gexp(-0.5 * np.where(keep, v, 0.0))
            re[g] = np.where(keep, re[g] + C[a][:, None] * E, re[g])
            im[g] = np.where(keep, im[g] + Sn[a][:, None] * E, im[g])
    return cref.as_complex(re, im)


def cw_sum(off, T, I, q, f):
    """P(f) of each group: the coherent sum of the same arrivals at one frequency, pressure_field's sum -> (G,) complex"""
    C, Sn, adds = arrival_terms(T, I, q, f)
    off = np.asarray(off, dtype=np.int64)
    out = np.zeros(len(off) - 1, complex)
    for g in range(len(off) - 1):
        re = im = 0.0
        for a in range(off[g], off[g + 1]):
            if adds[a]:
                re, im = re + C[a], im + Sn[a]
        out[g] = complex(re, im)
    return out


# ---- the Fourier identity -------------------------------------------------------------------------------------------------
# U(nu) = dt sum_n u(t_n) exp(i 2 pi nu t_n) = Ehat(nu) P(f + nu),  Ehat(nu) = sigma sqrt(2 pi) exp(-2 pi^2 sigma^2 nu^2):
# the spectrum of the baseband signal is the CW sum at f + nu under the pulse's own spectrum.  The bound on the difference,
# FOURIER_REL * sigma sqrt(2 pi) * sum_a amp_a, is derived: the cut at 8 sigma leaves 1.3e-14 per term, the aliasing of the
# Riemann sum is e^-79 at dt = sigma / 2, and the phase rounding of f T and nu t at these magnitudes is about 6e-12 rad.

FOURIER_F, FOURIER_B = 75.0, 20.0
FOURIER_NU = (-15.0, -3.3, 0.0, 4.7, 15.0)
FOURIER_REL = 1e-10


def pulse_spectrum(sigma, nu):
    return sigma * math.sqrt(2.0 * math.pi) * math.exp(-2.0 * math.pi ** 2 * sigma ** 2 * nu ** 2)


def spectrum(u, t, dt, nu):
    """U(nu) of sampled signals u (..., n_times) at the times t (..., n_times)"""
    return dt * np.sum(u * np.exp(2j * np.pi * nu * t), axis=-1)


def covering_axis(t_first, t_last, sigma, margin=9.0):
    """(t0, dt, n_times) of a time axis with dt = sigma / 2 that covers [t_first, t_last] by `margin` sigma on either side"""
    dt = 0.5 * sigma
    t0 = t_first - margin * sigma
    return t0, dt, int(math.ceil((t_last + margin * sigma - t0) / dt)) + 1


# ---- Lloyd's mirror with a pulse ------------------------------------------------------------------------------------------------
# coherent_reference's set-up (isovelocity, source at 100 m, 50 Hz, receivers 20 ... 400 m at 1 ... 5 km) with B = 20 Hz:
# u(t) = E(t - R1 / c) e^{i k R1} / R1 - E(t - R2 / c) e^{i k R2} / R2.

LLOYD_B, LLOYD_DT, LLOYD_NT, LLOYD_LEAD = 20.0, 4e-3, 128, 0.15
# the worst e = |u - u_ref| / sqrt(1 / R1^2 + 1 / R2^2) over every receiver, range and sample of the restatement on the CPU
# oracle's fan (tests/test_signal_host.py prints it), and the bound: twice that (DESIGN.md section 16's rule)
LLOYD_PULSE_MEASURED = 2.363809404840052e-05
LLOYD_PULSE_BOUND = 2.0 * LLOYD_PULSE_MEASURED


def lloyd_t0(x):
    """the start time per column: LLOYD_LEAD before x / c"""
    return np.asarray(x, dtype=float) / cref.LLOYD_C - LLOYD_LEAD


def lloyd_pulse_error(u, x):
    """u (len(LLOYD_DEPTHS), len(x), LLOYD_NT) complex on the time axes lloyd_t0(x) + n LLOYD_DT -> e (same shape), the error
    against the two-path closed form in units of the incoherent amplitude"""
    D, X = cref.LLOYD_DEPTHS[:, None, None], np.asarray(x, dtype=float)[None, :, None]
    t = lloyd_t0(x)[None, :, None] + (np.arange(LLOYD_NT) * LLOYD_DT)[None, None, :]
    R1, R2 = np.hypot(X, D - cref.LLOYD_ZS), np.hypot(X, D + cref.LLOYD_ZS)
    sigma = pulse_sigma(LLOYD_B)
    k = 2.0 * np.pi * cref.LLOYD_F / cref.LLOYD_C

    def E(tau):
        return np.where(np.abs(tau) <= 8.0 * sigma, np.exp(-tau ** 2 / (2.0 * sigma ** 2)), 0.0)
    ref = E(t - R1 / cref.LLOYD_C) * np.exp(1j * k * R1) / R1 - E(t - R2 / cref.LLOYD_C) * np.exp(1j * k * R2) / R2
    return np.abs(u - ref) / np.sqrt(1.0 / R1 ** 2 + 1.0 / R2 ** 2)


def fan_arrivals(rays, depths, environment, cols, flatearth=True, nb=None, ns=None):
    """The arrivals of a host fan and their phase index from the restatements: arrivals_reference's walk and coherent_reference's
    caustic index with the per-sample counts nb / ns (M, S) (None: a fan without bounces) -> (off, T, I, q)"""
    import arrivals_reference as aref
    a = aref.fan_arrivals(rays, depths, environment, cols, flatearth)
    qfull = cref.tube_phase(cref.caustic_index(-np.asarray(rays.zs), nb, ns), nb, ns)
    slot = np.repeat(np.arange(len(a["offsets"]) - 1), np.diff(a["offsets"])) % len(cols)
    return a["offsets"], a["T"], a["I"], qfull[a["tube"], np.asarray(cols)[slot]]
