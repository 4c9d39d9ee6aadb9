"""``transfer_function``: the channel's transfer function H(f) over a band of frequencies, summed over the fan's ray-tube
arrivals, and ``received_waveform``: the received waveform of any source signal, synthesised from it ("Transfer
function over a frequency band").

No reference counterpart: pygenray gives back rays, not amplitudes.  The arrivals (csrc/pgr_arrivals.h), their phase index
(csrc/pgr_phase.h), their path length (csrc/pgr_path.h) and the sum over them at every frequency (csrc/pgr_spectrum.h) run in
HIP and stay on the device from the fan to H -- in HBM for a device-resident fan, uploaded through torch for a host fan.
There is no CPU path.  The FFTs of ``received_waveform`` are NumPy's, on the host.
"""
import numpy as np

from . import _lib
from .coherent import _needs_counts
from .ray_objects import _columns
from .signal import _arrival_terms, _check_fits, _per_column, _to_host
from .transmission import _FanFrame, _absorption_profile, _boundary_spec, _lag_spec


def _band_absorption(absorption, freq):
    """``absorption(freq)``, a callable's dB/km at every frequency, checked -> alpha in dB per METRE (F,); the callable's own
    errors propagate"""
    a = np.asarray(absorption(freq.copy()), dtype=float)
    if a.shape != freq.shape:
        raise ValueError(f"absorption(frequencies) must give one value in dB/km per frequency: shape {freq.shape}, not "
                         f"{a.shape}")
    if not np.all(np.isfinite(a)) or np.any(a < 0):
        raise ValueError("absorption(frequencies) must be finite and >= 0 dB/km")
    return np.ascontiguousarray(a / 1000.0)


def _arrival_lengths(f, col, tube, w):
    """L_a of every arrival, on the device: the path length of the tube's two edge rays at the arrival's column, interpolated
    by the arrival's w in three separate operations, L_k + w (L_k+1 - L_k)"""
    L = f.path_integral(None, np.ones(1))                             # (S, M): the path length, alpha = 1
    k = tube.long()
    L0, L1 = L[col, k], L[col, k + 1]
    d = L1 - L0
    d = w * d
    return L0 + d


def transfer_function(rays, receiver_depths, env, frequencies, range_indices=None, absorption=None, bottom_loss=None,
                      surface_loss=None, t_reduce=None, flatearth=True, device=0):
    """The transfer function of the channel from the source of ``rays`` (a ``RayFan`` from ``shoot_rays``) to
    ``receiver_depths`` (metres, positive down, strictly ascending) at the save columns ``range_indices`` (default
    ``[S - 1]``, as in ``arrivals``), at the ``frequencies`` (Hz; a non-empty 1-D sequence, finite, >= 0, in any order) ->
    complex128 ndarray ``(R, n, F)``, re 1 m.  Every arrival of ``arrivals`` -- every tube ``pressure_field`` adds --
    contributes

        H(f) += sqrt(I) W(f) exp(i (2 pi f (T - t_reduce) - (pi / 2) q)),   q = kappa + 2 n_surf

    summed arrival by arrival in tube order, in ``pressure_field``'s sign convention: with ``t_reduce=None`` and without a
    callable ``absorption`` (W = 1), ``H[j, c, k]`` is ``pressure_field(..., frequencies[k])[j, column]`` bit for bit.
    ``t_reduce`` (seconds; None: 0.0, a scalar, or one value per requested column, e.g. the reduced time x / c_red) takes the
    common delay out of H, which makes it smooth enough in f to sample.  A requested column with r = 0 is NaN.

    ``absorption``: None; a scalar in dB/km or a pair ``(depths_m, dB_per_km)`` -- the frequency-blind weights of
    ``transmission_loss``, exactly; or a callable ``f_hz_array -> dB/km array`` such as ``thorp_absorption``: sea-water
    absorption that follows the frequency.  The tube weights then carry no volume absorption and every arrival is weighted by
    W(f) = 10^(-alpha(f) L / 20), alpha = ``absorption(frequencies) / 1000`` dB/m (its result must have the frequencies' shape
    and be finite and >= 0; its own errors propagate: ``thorp_absorption`` refuses f = 0) and L the arrival's path length,
    ``path_length`` interpolated across the tube as the travel time is.  ``bottom_loss``, ``surface_loss``: the weights of
    ``transmission_loss``, with any ``absorption``; a ``BottomReflection`` as ``bottom_loss`` also turns every arrival by its
    bottom bounces' phase, as in ``pressure_field`` -- one table across the band: the plane-wave coefficient of
    ``fluid_halfspace`` does not depend on frequency.  The frame, the sound speed and the errors are ``pressure_field``'s (a fan
    with bounces needs its bounce log, ``shoot_rays(..., max_bounces=K)``).  ``ValueError`` when ``R * n * F`` complex entries
    do not fit in the free device memory, before any kernel runs.  A device-resident fan is processed where it is and stays
    device resident."""
    freq = np.asarray(frequencies, dtype=float)
    if freq.ndim != 1 or len(freq) == 0:
        raise ValueError("frequencies must be a non-empty 1-D sequence")
    freq = np.ascontiguousarray(freq)
    if not np.all(np.isfinite(freq)) or np.any(freq < 0):
        raise ValueError("frequencies must be finite and >= 0 Hz")
    F = len(freq)
    if F > 65535 * 256:
        raise ValueError(f"at most {65535 * 256} frequencies per call")
    alpha = profile = None
    if callable(absorption):
        alpha = _band_absorption(absorption, freq)
    elif absorption is not None:
        profile = _absorption_profile(absorption)
    boundary = _boundary_spec(rays, bottom_loss, surface_loss)
    f = _FanFrame(rays, receiver_depths, env, flatearth, "transfer_function")
    counts = _needs_counts(rays)
    cols = _columns(range_indices, len(f.x))
    R, n = len(f.depths), len(cols)
    reduce = _per_column(0.0 if t_reduce is None else t_reduce, n, "t_reduce", "reduction time")
    f.to_device(device)
    import torch
    _check_fits(f, R, n, F, "transfer function", "entries")
    lag = _lag_spec(bottom_loss)
    offsets, tube, w, T, I, qa, col, *phi = _arrival_terms(f, cols, profile, boundary, counts, lag)
    La = None
    if alpha is not None:
        La = _arrival_lengths(f, col, tube, w) if len(tube) else torch.zeros(1, dtype=torch.float64, device=f.dev)
    tred = f.upload(np.tile(reduce, R))
    re, im = (torch.empty((R, n, F), dtype=torch.float64, device=f.dev) for _ in range(2))
    if lag is None:
        _lib.spectrum_device(f.env.device, offsets.data_ptr(), R * n, T.data_ptr(), I.data_ptr(), qa.data_ptr(),
                             0 if La is None else La.data_ptr(), tred.data_ptr(), freq, alpha, re.data_ptr(), im.data_ptr(),
                             f.stream)
    else:
        _lib.spectrum_phi_device(f.env.device, offsets.data_ptr(), R * n, T.data_ptr(), I.data_ptr(), qa.data_ptr(),
                                 phi[0].data_ptr(), 0 if La is None else La.data_ptr(), tred.data_ptr(), freq, alpha,
                                 re.data_ptr(), im.data_ptr(), f.stream)
    return _to_host(f, cols, re, im)


def _fft_sizes(n_source, n_times, n_fft):
    """(n_times, n_fft) of ``received_waveform`` from what was given, checked"""
    def whole(v, name):
        if isinstance(v, (bool, float)) or int(v) != v or int(v) < 1:
            raise ValueError(f"{name} must be an integer >= 1")
        return int(v)
    if n_times is None and n_fft is None:
        raise ValueError("give n_times, n_fft or both")
    nt = None if n_times is None else whole(n_times, "n_times")
    if n_fft is None:
        nf = 1 << (nt + n_source - 1).bit_length()
    else:
        nf = whole(n_fft, "n_fft")
    nt = nf if nt is None else nt
    if nf < n_source:
        raise ValueError(f"n_fft ({nf}) must be at least the length of source ({n_source})")
    if nt > nf:
        raise ValueError(f"n_times ({nt}) must be <= n_fft ({nf})")
    return nt, nf


def _synthesise(H_of, source, dt, carrier, t0, n_times, n_fft):
    """``received_waveform``'s checks and its FFT synthesis around a transfer function: ``H_of(frequencies, t_reduce)`` -> H
    (R, n, n_fft), as ``transfer_function`` gives it -> u (R, n, n_times).  Shared with ``beam_received_waveform``."""
    s = np.asarray(source)
    if s.ndim != 1 or len(s) == 0:
        raise ValueError("source must be a non-empty 1-D sequence of complex baseband samples")
    s = s.astype(np.complex128)
    if not np.all(np.isfinite(s)):
        raise ValueError("source must be finite")
    step, fc = float(dt), float(carrier)
    if not (np.isfinite(step) and step > 0):
        raise ValueError("dt must be finite and > 0 seconds")
    if not (np.isfinite(fc) and fc >= 1.0 / (2.0 * step)):
        raise ValueError("carrier must be finite and at least 1 / (2 dt) Hz: the band carrier +- 1 / (2 dt) must not reach "
                         "negative frequencies")
    nt, nf = _fft_sizes(len(s), n_times, n_fft)
    start = np.asarray(t0, dtype=float)
    if not np.all(np.isfinite(start)):
        raise ValueError("t0 must be finite")
    nu = np.fft.fftfreq(nf, step)
    Shat = nf * np.fft.ifft(s, nf)
    H = H_of(fc + nu, start)
    cyc = fc * np.broadcast_to(start, (H.shape[1],))
    turn = np.exp(2j * np.pi * (cyc - np.rint(cyc)))
    u = np.fft.fft(Shat * H, axis=-1) / nf * turn[None, :, None]
    return np.ascontiguousarray(u[:, :, :nt])


def received_waveform(rays, receiver_depths, env, source, dt, carrier, t0, n_times=None, n_fft=None, range_indices=None,
                      absorption=None, bottom_loss=None, surface_loss=None, flatearth=True, device=0):
    """The signal a receiver records when the source sends ANY waveform: the complex baseband envelope ``source[i]`` (a
    non-empty 1-D complex sequence) at the emission times ``i * dt`` (``dt`` > 0 seconds) on the carrier ``carrier`` (Hz) --
    the analytic passband signal s(t) exp(-2j pi carrier t), in ``pressure_field``'s sign convention -> complex128 ndarray
    ``(R, n, n_times)``: the complex baseband signal at the times ``t0 + arange(n_times) * dt`` (``t0`` a scalar or one
    value per requested column), in ``received_signal``'s convention.  Synthesised from ``transfer_function``:

        nu = fftfreq(n_fft, dt);   Shat = n_fft * ifft(source padded to n_fft)             # sum_i s_i exp(+2j pi nu i dt)
        H  = transfer_function(..., frequencies=carrier + nu, t_reduce=t0)
        u  = fft(Shat * H) / n_fft * exp(2j pi (carrier t0 - rint(carrier t0)))            # the first n_times kept

    with NumPy's FFT on the host.  ``n_fft`` defaults to the next power of two >= ``n_times + len(source)``, ``n_times`` to
    ``n_fft``.  The result is CIRCULAR with the period ``n_fft * dt``: an arrival later than
    ``t0 + (n_fft - len(source)) * dt`` or earlier than ``t0`` wraps around, so choose ``t0`` and ``n_fft`` to hold every
    arrival and the source record behind it.  ``dt`` must sample the envelope finely enough for its spectrum to have died out
    at +-1 / (2 dt).  For a Gaussian ``source`` centred at the emission time tc, u(t) is ``received_signal``'s value at
    t - tc.

    ``absorption`` as in ``transfer_function``: a callable such as ``thorp_absorption`` makes the absorption follow the
    frequency across the band.  ``ValueError`` for a ``carrier`` below 1 / (2 dt) (the band would reach negative
    frequencies), ``n_fft < len(source)`` and ``n_times > n_fft``; every other argument, error and the device residency are
    ``transfer_function``'s."""
    return _synthesise(lambda freq, start: transfer_function(rays, receiver_depths, env, freq, range_indices=range_indices,
                                                             absorption=absorption, bottom_loss=bottom_loss,
                                                             surface_loss=surface_loss, t_reduce=start, flatearth=flatearth,
                                                             device=device),
                       source, dt, carrier, t0, n_times, n_fft)


__all__ = ["transfer_function", "received_waveform"]
