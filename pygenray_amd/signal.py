"""``received_signal``: the time series a receiver records when the source sends a Gaussian pulse, summed over the fan's
ray-tube arrivals ("Received signal of a Gaussian pulse").

No reference counterpart: pygenray gives back rays, not amplitudes.  The arrivals (csrc/pgr_arrivals.h), their phase index
(csrc/pgr_phase.h) and the sum over them at every time sample (csrc/pgr_signal.h) run in HIP and stay on the device from the
fan to the signal -- in HBM for a device-resident fan, uploaded through torch for a host fan.  There is no CPU path.
"""
import math

import numpy as np

from . import _lib
from ._fan_frame import _arrival_terms, _check_fits, _coherent_frame, _lag_spec, _per_column, _pulse, _to_host
from ._fan_frame import _inv_sigma   # noqa: F401  (lived here: still importable from here)
from .ray_objects import _columns


def pulse_sigma(bandwidth):
    """The width sigma (seconds) of the Gaussian envelope exp(-t^2 / (2 sigma^2)) whose spectrum has the half-power full
    bandwidth ``bandwidth`` (Hz, finite, >= 0): sigma = sqrt(ln 2) / (pi B); ``inf`` for 0, a continuous wave."""
    B = float(bandwidth)
    if not (math.isfinite(B) and B >= 0):
        raise ValueError("bandwidth must be finite and >= 0 Hz")
    return math.inf if B == 0 else math.sqrt(math.log(2.0)) / (math.pi * B)


def received_signal(rays, receiver_depths, env, frequency, bandwidth, t0, dt, n_times, range_indices=None, absorption=None,
                    bottom_loss=None, surface_loss=None, flatearth=True, device=0):
    """The complex-demodulated signal of ``rays`` (a ``RayFan`` from ``shoot_rays``) at ``receiver_depths`` (metres, positive
    down, strictly ascending) and the save columns ``range_indices`` (default ``[S - 1]``, as in ``arrivals``) when the source
    sends a Gaussian pulse of centre ``frequency`` (Hz, finite, >= 0) and half-power full bandwidth ``bandwidth`` (Hz,
    finite, >= 0) -> complex128 ndarray ``(R, n, n_times)``, re 1 m, at the times ``t0 + arange(n_times) * dt`` (``dt`` > 0
    seconds; ``t0`` a scalar or one value per requested column, e.g. the reduced time x / c_red).  Every arrival of
    ``arrivals`` -- every tube ``pressure_field`` adds -- contributes

        u(t) += sqrt(I) exp(i (2 pi f T - (pi / 2) q)) E(t - T),   E(tau) = exp(-tau^2 / (2 sigma^2)),  q = kappa + 2 n_surf

    with sigma = ``pulse_sigma(bandwidth)``, the envelope cut at 8 sigma (E = 1.3e-14), summed arrival by arrival in tube
    order.  u is the baseband signal; the analytic passband signal is ``u(t) exp(-2j pi f t)``, in ``pressure_field``'s sign
    convention.  ``bandwidth=0`` is the CW limit: every sample equals ``pressure_field(...)[j, column]``.  A requested column
    with r = 0 is NaN, as in ``pressure_field``; where no arrival is within 8 sigma the signal is 0.

    ``absorption``, ``bottom_loss``, ``surface_loss``: the weights of ``transmission_loss``, exactly; a ``BottomReflection``
    as ``bottom_loss`` also turns every arrival by its bottom bounces' phase, as in ``pressure_field``.  The absorption
    weights are those of the one profile given, i.e. of the centre frequency: they are not varied across the band
    (``received_waveform`` with a callable ``absorption`` varies them).  The
    frame, the sound speed and the errors are ``pressure_field``'s (a fan with bounces needs its bounce log,
    ``shoot_rays(..., max_bounces=K)``).  ``ValueError`` when ``R * n * n_times`` complex samples do not fit in the free
    device memory, before any kernel runs.  A device-resident fan is processed where it is and stays device resident."""
    f0, rs, step, nt = _pulse(frequency, bandwidth, dt, n_times)
    f, profile, boundary, counts = _coherent_frame(rays, receiver_depths, env, absorption, bottom_loss, surface_loss, flatearth,
                                                   "received_signal")
    cols = _columns(range_indices, len(f.x))
    R, n = len(f.depths), len(cols)
    start = _per_column(t0, n, "t0", "start time")
    f.to_device(device)
    import torch
    _check_fits(f, R, n, nt, "signal", "samples")
    lag = _lag_spec(bottom_loss)
    offsets, _, _, T, I, qa, _, *phi = _arrival_terms(f, cols, profile, boundary, counts, lag)
    tstart = f.upload(np.tile(start, R))
    re, im = (torch.empty((R, n, nt), dtype=torch.float64, device=f.dev) for _ in range(2))
    if lag is None:
        _lib.signal_device(f.env.device, offsets.data_ptr(), R * n, T.data_ptr(), I.data_ptr(), qa.data_ptr(), tstart.data_ptr(),
                           f0, rs, step, nt, re.data_ptr(), im.data_ptr(), f.stream)
    else:
        _lib.signal_phi_device(f.env.device, offsets.data_ptr(), R * n, T.data_ptr(), I.data_ptr(), qa.data_ptr(),
                               phi[0].data_ptr(), tstart.data_ptr(), f0, rs, step, nt, re.data_ptr(), im.data_ptr(), f.stream)
    return _to_host(f, cols, re, im)


__all__ = ["received_signal", "pulse_sigma"]
