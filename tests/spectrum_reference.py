"""Test helpers for transfer_function / received_waveform (not a product path): a plain NumPy restatement of DESIGN.md section
18, written from the definition -- the sum over each group's arrivals at every frequency, in the kernel's operation order and
without contraction -- on coherent_reference's phase_cycles / gcos2pi / gsin2pi and beam_reference's gexp, the three lines of
received_waveform's synthesis, and the set-ups shared by the CPU and GPU tests (the synthesis identity with a Gaussian source)."""
import math

import numpy as np

import coherent_reference as cref
import signal_reference as sref
from beam_reference import gexp

PATH_LN10_10 = float.fromhex("0x1.d791c5f888822p-3")     # the double nearest ln(10) / 10 (csrc/pgr_path.h)
K20 = 0.5 * PATH_LN10_10                                 # exact: the double nearest ln(10) / 20
SYNTH_REL = sref.FOURIER_REL                             # the synthesis identity's bound, in units of sum_a amp_a


def amplitude_weight(alpha, L):
    """W of the definition for alpha (dB/m) and L (m), broadcast: gexp(-((alpha L) K20)), 0.0 below -700, NaN for a NaN"""
    with np.errstate(invalid="ignore", over="ignore"):
        yw = -((np.asarray(alpha, dtype=float) * np.asarray(L, dtype=float)) * K20)
        W = gexp(np.where((yw >= -700.0), yw, 0.0))
    return np.where(yw != yw, np.nan, np.where(yw < -700.0, 0.0, W))


def arrival_lengths(L0, L1, w):
    """L_a from the edge rays' path lengths and the arrival's w: subtract, multiply, add"""
    d = L1 - L0
    d = w * d
    return L0 + d


def spectrum_sum(off, T, I, q, L, tred, freq, alpha):
    """The definition, restated: groups [off[g], off[g + 1]) of arrivals T / I / q (q None: all zero) / L (None: none),
    reduction times tred (G,), frequencies freq (F,), alpha (F,) in dB/m or None -> H (G, F) complex.  A loop over the rank
    of an arrival within its group, vectorised over groups and frequencies: each entry's sums are formed from 0.0 one arrival
    at a time, in order."""
    off = np.asarray(off, dtype=np.int64)
    T, I = np.asarray(T, dtype=float), np.asarray(I, dtype=float)
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
            ph = cref.phase_cycles(tau[:, None], qq[a][:, None], freq[None, :])
            cv, sv = cref.gcos2pi(ph), cref.gsin2pi(ph)
            if alpha is None:
                re[g] = re[g] + amp[a][:, None] * cv
                im[g] = im[g] + amp[a][:, None] * sv
            else:
                W = amplitude_weight(np.asarray(alpha, dtype=float)[None, :], np.asarray(L, dtype=float)[a][:, None])
                re[g] = re[g] + (amp[a][:, None] * cv) * W
                im[g] = im[g] + (amp[a][:, None] * sv) * W
    return cref.as_complex(re, im)


def waveform(H_of, source, dt, carrier, t0, n_fft, n_times=None):
    """received_waveform's three lines: H_of(frequencies, t_reduce) -> H (..., n_fft), t0 a scalar -> u (..., n_times)"""
    nu = np.fft.fftfreq(n_fft, dt)
    Shat = n_fft * np.fft.ifft(np.asarray(source, dtype=complex), n_fft)
    H = H_of(carrier + nu, t0)
    u = np.fft.fft(Shat * H, axis=-1) / n_fft * np.exp(2j * np.pi * (carrier * t0 - np.rint(carrier * t0)))
    return u[..., :n_fft if n_times is None else n_times]


# ---- the synthesis identity ------------------------------------------------------------------------------------------------
# A Gaussian source exp(-(i dt - tc)^2 / (2 sigma^2)) centred at the emission time tc = 9 sigma, on dt = sigma / 4: the
# synthesised u(t) is received_signal's value at t - tc, i.e. signal_sum with every T moved by tc, times e^{-2 pi i f tc} (the
# carrier phase the later arrival collects).  The bound SYNTH_REL * sum_a amp_a is section 17's FOURIER_REL rule: the
# source's cut at 9 sigma leaves e^-40.5 = 2.6e-18, signal_sum's at 8 sigma 1.3e-14 per term, the source's spectrum aliases
# at exp(-2 pi^2 sigma^2 / (2 dt)^2) = e^-79 at dt = sigma / 4 (e^-19.7 = 2.7e-9 at sigma / 2: too coarse), and the phase
# rounding of f T at T = 60 s is about 6e-12 rad.

SYNTH_F, SYNTH_B = sref.FOURIER_F, sref.FOURIER_B
SYNTH_MARGIN = 9.0                                        # the source's centre and the lead before the first arrival, in sigma


def gaussian_source(sigma, dt):
    """(source, tc): the Gaussian envelope of width sigma centred at tc = 9 sigma, sampled at i dt over [0, 18 sigma]"""
    tc = SYNTH_MARGIN * sigma
    t = np.arange(int(round(2 * SYNTH_MARGIN * sigma / dt)) + 1) * dt
    return np.exp(-(t - tc) ** 2 / (2.0 * sigma ** 2)).astype(complex), tc


def covering_fft(t_first, t_last, sigma, dt, n_source):
    """(t0, n_fft): t0 = t_first - 9 sigma and the next power of two of samples that holds every arrival up to t_last, 9 sigma
    behind it and the source record"""
    t0 = t_first - SYNTH_MARGIN * sigma
    need = int(math.ceil((t_last + SYNTH_MARGIN * sigma - t0) / dt)) + 1 + n_source
    return t0, 1 << (need - 1).bit_length()


def group_amplitudes(off, I, q):
    """sum_a amp_a over the arrivals that add (q >= 0), per group"""
    amp = np.where(np.asarray(q) >= 0, np.sqrt(np.asarray(I, dtype=float)), 0.0)
    return np.array([amp[off[g]:off[g + 1]].sum() for g in range(len(off) - 1)])
