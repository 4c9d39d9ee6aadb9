"""Test helpers for array_response (not a product path): a plain NumPy restatement of DESIGN.md section 22, written from the
definition -- the sum over the elements and over each element's arrivals at every look and time sample, in the kernel's
operation order and without contraction -- on signal_reference's sample times, coherent_reference's cos / sin, beam_reference's
gexp and reflection_reference's turn_back; and the set-up shared by the CPU and GPU tests: Lloyd's mirror seen by a vertical
array, against a closed form built from passband delay-and-sum."""
import numpy as np

import arrivals_reference as aref
import beam_pressure_reference as bp
import coherent_reference as cref
import reflection_reference as rref
import signal_reference as sref
from beam_reference import gexp


def array_sum(off, T, I, q, phi, delay, weight, tstart, R, n_cols, f, rs, dt, n_times):
    """The definition, restated: groups g = j n_cols + c of arrivals T / I / q (q None: all zero) / phi (None: no lag), delay
    (R n_cols, B) seconds, weight (R n_cols,), start times tstart (n_cols,) -> y (n_cols, B, n_times) complex.  Per column slot
    a loop over the elements and over each element's arrivals in order, vectorised over looks and samples: each sample's sums
    are formed from 0.0 one arrival at a time."""
    off = np.asarray(off, dtype=np.int64)
    T, I = np.asarray(T, dtype=float), np.asarray(I, dtype=float)
    delay, weight = np.asarray(delay, dtype=float), np.asarray(weight, dtype=float)
    B = delay.shape[1]
    assert len(off) == R * n_cols + 1 and delay.shape == (R * n_cols, B) and weight.shape == (R * n_cols,)
    qq = np.zeros(len(T), np.int64) if q is None else np.asarray(q).astype(np.int64)
    t = sref.sample_times(tstart, dt, n_times)                               # (n_cols, n_times)
    re, im = np.zeros((n_cols, B, n_times)), np.zeros((n_cols, B, n_times))
    with np.errstate(invalid="ignore", over="ignore"):
        for c in range(n_cols):
            for j in range(R):
                g = j * n_cols + c
                sl = slice(off[g], off[g + 1])
                # the constants of the group's arrivals at every look: (count, B)
                Ts = T[sl][:, None] - delay[g][None, :]
                amp = np.sqrt(I[sl])
                amp = amp * weight[g]
                ph = cref.phase_cycles(Ts, qq[sl][:, None], f)
                if phi is not None:
                    ph = rref.turn_back(ph, np.asarray(phi, dtype=float)[sl][:, None])
                C, Sn = amp[:, None] * cref.gcos2pi(ph), amp[:, None] * cref.gsin2pi(ph)
                for k in np.flatnonzero(qq[sl] >= 0):
                    x = (t[c][None, :] - Ts[k][:, None]) * rs
                    v = x * x
                    keep = v <= sref.CUT                                     # (False for a NaN v)
                    if not keep.any():                                       # (nothing to add anywhere: the sums stay)
                        continue
                    E = gexp(-0.5 * np.where(keep, v, 0.0))
                    re[c] = np.where(keep, re[c] + C[k][:, None] * E, re[c])
                    im[c] = np.where(keep, im[c] + Sn[k][:, None] * E, im[c])
    return cref.as_complex(re, im)


def steering(depths, angles, c, d_ref=None):
    """delta (R, B) = -sin(radians(theta_b)) / c (d_j - d_ref), from the formula (d_ref None: the mean depth)"""
    d = np.asarray(depths, dtype=float)
    d_ref = d.mean() if d_ref is None else d_ref
    return np.array([[-np.sin(np.radians(a)) / c * (dj - d_ref) for a in np.asarray(angles, dtype=float)] for dj in d])


def group_layout(per_element, n_cols):
    """per-element values (R, ...) -> per-group values (R n_cols, ...), g = j n_cols + c"""
    return np.repeat(np.asarray(per_element), n_cols, axis=0)


# ---- Lloyd's mirror seen by a vertical array ---------------------------------------------------------------------------------------
# Isovelocity 1500 m/s under a pressure-release surface, source at 200 m, 75 Hz with a 20 Hz pulse, range 5 km; 41 elements at
# 10 m spacing centred at 500 m; looks -15 ... 15 degrees in steps of 0.5.  At the centre element the direct path arrives 3.4
# degrees and the surface path 8.0 degrees downwards (received_angle: -3.4, -8.0), 26 ms apart: against sigma = 13 ms and a
# beamwidth lambda / L = 2.9 degrees they are separable both ways.

ARRAY_C, ARRAY_ZS, ARRAY_X, ARRAY_F, ARRAY_B = bp.EXACT_C, 200.0, 5e3, 75.0, 20.0
ARRAY_DEPTHS = 500.0 + 10.0 * np.arange(-20, 21)
ARRAY_LOOKS = np.arange(-15.0, 15.25, 0.5)
ARRAY_LEAD, ARRAY_DT, ARRAY_NT = 0.1, 2e-3, 128
ARRAY_BEAMWIDTH = np.degrees((ARRAY_C / ARRAY_F) / (ARRAY_DEPTHS[-1] - ARRAY_DEPTHS[0]))          # lambda / L, 2.9 degrees
# the worst e = |y - y_closed| / sum_j |w_j| sqrt(1 / R1^2 + 1 / R2^2) over every look and sample of the restatement on the
# exact straight rays (tests/test_array_response_host.py prints it), and the bound: twice that (DESIGN.md section 19's rule;
# the margin covers the GPU's table look-up)
ARRAY_MEASURED = 1.137067899184816e-05
ARRAY_BOUND = 2.0 * ARRAY_MEASURED


def array_t0(x=ARRAY_X):
    return x / ARRAY_C - ARRAY_LEAD


def array_paths(depths=ARRAY_DEPTHS, x=ARRAY_X):
    """R1, R2 (R,): the lengths of the direct path and of the path over the surface to every element"""
    d = np.asarray(depths, dtype=float)
    return np.hypot(x, d - ARRAY_ZS), np.hypot(x, d + ARRAY_ZS)


def array_geometry(depth=500.0, x=ARRAY_X):
    """(received angles in degrees, travel times) of the direct and the surface path at `depth`: both travel downwards there,
    which received_angle counts negative"""
    R1, R2 = np.hypot(x, depth - ARRAY_ZS), np.hypot(x, depth + ARRAY_ZS)
    return (-np.degrees(np.arctan2(depth - ARRAY_ZS, x)), -np.degrees(np.arctan2(depth + ARRAY_ZS, x))), (R1 / ARRAY_C, R2 / ARRAY_C)


def array_closed_form(weights, delta, depths=ARRAY_DEPTHS, x=ARRAY_X):
    """Passband delay-and-sum of the two spherical paths, brought to baseband: element j records the analytic signal
    s_j(t) = sum_p (+-1 / R_pj) E(t - R_pj / c) exp(-2 pi i f (t - R_pj / c)), the beamformer adds w_j s_j(t + delta_jb), and
    y = exp(2 pi i f t) times that -> (B, ARRAY_NT) complex; the surface path carries the half cycle as its sign"""
    R1, R2 = array_paths(depths, x)
    sigma = sref.pulse_sigma(ARRAY_B)
    t = array_t0(x) + np.arange(ARRAY_NT) * ARRAY_DT
    z = np.zeros((delta.shape[1], ARRAY_NT), complex)                     # the passband sum
    for j in range(len(R1)):
        tj = t[None, :] + delta[j][:, None]                               # the element's own time, per look
        for sign, Rp in ((1.0, R1[j]), (-1.0, R2[j])):
            tau = tj - Rp / ARRAY_C
            E = np.where(np.abs(tau) <= 8.0 * sigma, np.exp(-tau ** 2 / (2.0 * sigma ** 2)), 0.0)
            z += weights[j] * (sign / Rp) * E * np.exp(-2j * np.pi * ARRAY_F * tau)
    return z * np.exp(2j * np.pi * ARRAY_F * t)[None, :]


def array_error(y, weights, delta, depths=ARRAY_DEPTHS, x=ARRAY_X):
    """e (B, ARRAY_NT) of a response y against the closed form, in units of the weighted incoherent amplitude"""
    R1, R2 = array_paths(depths, x)
    return np.abs(y - array_closed_form(weights, delta, depths, x)) / np.sum(np.abs(weights) * np.sqrt(1.0 / R1 ** 2 + 1.0 / R2 ** 2))


def two_largest_maxima(m):
    """the (look, sample) grid points of the two largest local maxima of the map m (B, n_times) >= 0, largest first: a grid
    point above its (up to) eight neighbours"""
    B, N = m.shape
    pad = np.full((B + 2, N + 2), -np.inf)
    pad[1:-1, 1:-1] = m
    peak = np.ones((B, N), bool)
    for db in (-1, 0, 1):
        for dn in (-1, 0, 1):
            if db or dn:
                peak &= m > pad[1 + db:B + 1 + db, 1 + dn:N + 1 + dn]
    idx = np.argwhere(peak)
    order = np.argsort(-m[peak])
    return [tuple(int(v) for v in idx[i]) for i in order[:2]]


def exact_array_arrivals(depths=ARRAY_DEPTHS, x=ARRAY_X):
    """the ray-tube arrivals of beam_pressure_reference.exact_fan (straight rays, folded at the surface) at the elements ->
    (arrivals_reference's dict, q per arrival)"""
    zs, ps, ts, xs, p0, q = bp.exact_fan(ARRAY_ZS, ranges=np.array([x]))
    a = aref.tube_arrivals(zs, ps, ts, xs, p0, depths, [1], bp.EXACT_CIN, bp.EXACT_RIN, bp.EXACT_ZIN)
    return a, q[a["tube"], 1]
