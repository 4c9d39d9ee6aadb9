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
from ._fan_frame import (_arrival_lengths, _arrival_terms, _band, _band_absorption, _check_fits, _coherent_frame, _lag_spec,
                         _one_zero, _per_column, _synthesise, _to_host, _fft_sizes)   # noqa: F401  (_fft_sizes lived here)
from .ray_objects import _columns


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
    freq = _band(frequencies)
    F = len(freq)
    alpha = _band_absorption(absorption, freq) if callable(absorption) else None
    f, profile, boundary, counts = _coherent_frame(rays, receiver_depths, env, None if callable(absorption) else absorption,
                                                   bottom_loss, surface_loss, flatearth, "transfer_function")
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
        La = _arrival_lengths(f, col, tube, w) if len(tube) else _one_zero(f.dev)
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
