"""``array_response``: the time-angle response of a vertical line array, delay-and-sum beamforming over the elements' arrivals
("Vertical-array beamforming").

A delayed element signal is the element's own arrival list with every travel time shifted by the steering delay, so the
beamformer is ``received_signal``'s sum under one more loop (csrc/pgr_array.h): the fan, the arrivals of every element and the
sum over elements, looks and samples stay on the device -- in HBM for a device-resident fan, uploaded through torch for a host
fan.  There is no CPU path; ``steering_delays`` alone is host arithmetic.
"""
import numpy as np

from . import _lib
from ._fan_frame import _arrival_terms, _check_fits, _coherent_frame, _lag_spec, _per_column, _pulse, _to_host
from .arrivals import _bilinear
from .beam_arrivals import _beam_frame, _device_beam_arrivals, _sum_terms
from .ray_objects import _columns


def _looks(angles):
    """``angles``, the look angles in degrees, checked -> contiguous float64 (B,)"""
    a = np.asarray(angles, dtype=float)
    if a.ndim != 1 or len(a) == 0:
        raise ValueError("angles must be a non-empty 1-D sequence of look angles in degrees")
    if not np.all(np.isfinite(a)) or np.any(np.abs(a) > 90.0):
        raise ValueError("angles must be finite and lie in [-90, 90] degrees")
    return np.ascontiguousarray(a)


def _elements(receiver_depths):
    d = np.asarray(receiver_depths, dtype=float)
    if d.ndim != 1 or len(d) == 0:
        raise ValueError("receiver_depths must be a non-empty 1-D sequence: an array has at least 1 element")
    if not np.all(np.isfinite(d)):
        raise ValueError("receiver_depths must be finite")
    return d


def _reference_depth(reference_depth, depths):
    if reference_depth is None:
        return float(np.mean(depths))
    d = float(reference_depth)
    if not np.isfinite(d):
        raise ValueError("reference_depth must be finite")
    return d


def _sound_speed(sound_speed, n=None):
    """a scalar, or one value per column when `n` says how many -> float array, finite and > 0"""
    c = np.asarray(sound_speed, dtype=float) if n is None else _per_column(sound_speed, n, "sound_speed", "sound speed")
    if c.ndim > 1:
        raise ValueError("sound_speed must be a scalar or a 1-D sequence, one sound speed per column")
    if not np.all(np.isfinite(c)) or np.any(c <= 0):
        raise ValueError("sound_speed must be finite and > 0 m/s")
    return c


def _shading(shading, R):
    if shading is None:
        return np.full(R, 1.0 / R)
    w = np.asarray(shading, dtype=float)
    if w.shape != (R,):
        raise ValueError(f"shading must hold one weight per element ({R})")
    if not np.all(np.isfinite(w)):
        raise ValueError("shading must be finite")
    return np.ascontiguousarray(w)


def steering_delays(receiver_depths, angles, sound_speed, reference_depth=None):
    """The plane-wave steering delays of a vertical line array -> float64 ``(R, B)`` seconds: for the element at depth d_j
    (``receiver_depths``, metres, positive down) and the look angle theta_b (``angles``, degrees in [-90, 90])

        delta[j, b] = -sin(radians(theta_b)) / c * (d_j - d_ref)

    with ``sound_speed`` c (m/s, > 0) and ``reference_depth`` d_ref (default: the mean of the depths).  The angles are in
    ``Arrivals.received_angle``'s convention: a plane wave whose ``received_angle`` is theta reaches element j the time
    delta[j] after it reaches d_ref, so a look at theta -- every element's signal advanced by its delta -- aligns it.
    ``sound_speed`` may hold one value per save column (1-D, n of them): the result is then ``(n, R, B)``.  Host arithmetic
    only."""
    d = _elements(receiver_depths)
    a = _looks(angles)
    c = _sound_speed(sound_speed)
    s = -np.sin(np.radians(a))
    lever = d - _reference_depth(reference_depth, d)
    if c.ndim == 0:
        return (s / float(c))[None, :] * lever[:, None]
    return (s[None, :] / c[:, None])[:, None, :] * lever[None, :, None]


def _array_arguments(angles, frequency, bandwidth, dt, n_times, shading, receiver_depths, reference_depth):
    """an array product's own arguments, checked in this order before the fan's -> (f0, 1 / sigma, dt, n_times, looks, weights,
    d_ref)"""
    f0, rs, step, nt = _pulse(frequency, bandwidth, dt, n_times)
    looks = _looks(angles)
    d = _elements(receiver_depths)
    return f0, rs, step, nt, looks, _shading(shading, len(d)), _reference_depth(reference_depth, d)


def _delay_and_sum(f, cols, offsets, T, I, qa, phi, looks, sound_speed, dref, w, start, f0, rs, step, nt):
    """pgr_array_response_device over the arrival lists of the frame `f` (on the device, R * n groups) -> complex128
    (n, B, n_times) on the host, the source's own columns NaN"""
    import torch
    R, n, B = len(f.depths), len(cols), len(looks)
    if sound_speed is None:                                          # received_angle's look-up, at the reference depth
        cin, rin, zin = f.tables
        sound_speed = _bilinear(f.xf[cols], np.full(n, dref), rin, zin, cin)
    delay = steering_delays(f.depths, looks, sound_speed, dref)       # (n, R, B)
    d_delay = f.upload(delay.transpose(1, 0, 2))                      # [g = j * n + c][b]
    d_w = f.upload(np.repeat(w, n))
    tstart = f.upload(start)
    re, im = (torch.empty((n, B, nt), dtype=torch.float64, device=f.dev) for _ in range(2))
    _lib.array_response_sum(f.env.device, offsets.data_ptr(), R, n, T.data_ptr(), I.data_ptr(), qa.data_ptr(),
                            0 if phi is None else phi.data_ptr(), d_delay.data_ptr(), d_w.data_ptr(), tstart.data_ptr(), f0, rs,
                            step, nt, B, re.data_ptr(), im.data_ptr(), f.stream)
    return _to_host(f, cols, re, im, axis=0)


def array_response(rays, receiver_depths, env, angles, frequency, bandwidth, t0, dt, n_times, range_indices=None,
                   sound_speed=None, reference_depth=None, shading=None, absorption=None, bottom_loss=None, surface_loss=None,
                   flatearth=True, device=0):
    """The time-angle response of a vertical line array with elements at ``receiver_depths`` (metres, positive down, strictly
    ascending; R of them) to the Gaussian pulse of ``received_signal``: the delay-and-sum beamformer output at the look angles
    ``angles`` (degrees in [-90, 90], ``Arrivals.received_angle``'s convention; B of them) -> complex128 ndarray
    ``(n, B, n_times)``, re 1 m, at the save columns ``range_indices`` and the times ``t0 + arange(n_times) * dt``:

        y(t) = sum_j w_j exp(-2 pi i f delta_j) u_j(t + delta_j),   delta = steering_delays(...)

    with u_j ``received_signal``'s baseband signal at element j -- formed exactly, not interpolated: every arrival of element j
    enters with its travel time shifted by delta_j, which turns its phase and delays its envelope at once.  A look at theta
    aligns an arrival whose ``received_angle`` is theta.  ``bandwidth=0`` is the CW conventional beamformer.

    ``sound_speed`` (m/s; a scalar or one value per requested column) is the c of the steering delays; None takes, per
    column, the value of the frame's sound-speed table at the column's range and ``reference_depth``, the look-up
    ``received_angle`` uses.  ``reference_depth`` defaults to the mean element depth.  ``shading`` holds one weight per
    element (finite; None: 1 / R each).  The pulse arguments, ``t0``, the weights ``absorption``, ``bottom_loss``,
    ``surface_loss`` (a ``BottomReflection`` also turns every arrival by its bottom bounces' phase), the frame and the errors
    are ``received_signal``'s.  With one element, ``angles=[0]`` and ``shading=[1]`` the result is ``received_signal``'s bit
    for bit.  A requested column with r = 0 is NaN.  ``ValueError`` when ``n * B * n_times`` complex samples do not fit in
    the free device memory, before any kernel runs.  A device-resident fan is processed where it is and stays device
    resident."""
    f0, rs, step, nt, looks, w, dref = _array_arguments(angles, frequency, bandwidth, dt, n_times, shading, receiver_depths,
                                                        reference_depth)
    f, profile, boundary, counts = _coherent_frame(rays, receiver_depths, env, absorption, bottom_loss, surface_loss, flatearth,
                                                   "array_response")
    cols = _columns(range_indices, len(f.x))
    n = len(cols)
    start = _per_column(t0, n, "t0", "start time")
    c = None if sound_speed is None else _sound_speed(sound_speed, n)
    f.to_device(device)
    _check_fits(f, n, len(looks), nt, "array response", "samples")
    lag = _lag_spec(bottom_loss)
    offsets, _, _, T, I, qa, _, *phi = _arrival_terms(f, cols, profile, boundary, counts, lag)
    return _delay_and_sum(f, cols, offsets, T, I, qa, phi[0] if phi else None, looks, c, dref, w, start, f0, rs, step, nt)


def beam_array_response(rays, receiver_depths, env, angles, frequency, bandwidth, t0, dt, n_times, min_width=10.0,
                        curvature=True, range_indices=None, sound_speed=None, reference_depth=None, shading=None,
                        absorption=None, bottom_loss=None, surface_loss=None, flatearth=True, device=0):
    """``array_response`` summed over the beam arrivals of ``beam_arrivals`` instead of the tube arrivals, as
    ``beam_received_signal`` is to ``received_signal`` -> complex128 ndarray ``(n, B, n_times)``.  The array's arguments and
    their errors are ``array_response``'s; ``min_width``, ``curvature``, the weights and every other error are
    ``beam_arrivals``' (a ``BottomReflection`` as ``bottom_loss`` is refused).  A device-resident fan is processed where it
    is and stays device resident."""
    f0, rs, step, nt, looks, w, dref = _array_arguments(angles, frequency, bandwidth, dt, n_times, shading, receiver_depths,
                                                        reference_depth)
    f, cols, width, profile, boundary, counts = _beam_frame(rays, receiver_depths, env, min_width, range_indices, absorption,
                                                            bottom_loss, surface_loss, flatearth, "beam_array_response")
    n = len(cols)
    start = _per_column(t0, n, "t0", "start time")
    c = None if sound_speed is None else _sound_speed(sound_speed, n)
    f.to_device(device)
    _check_fits(f, n, len(looks), nt, "array response", "samples")
    offsets, _, _, T, amp, qa = _device_beam_arrivals(f, cols, width, curvature, profile, boundary, counts, extra_bytes=8)
    T, I, qa = _sum_terms(T, amp, qa)
    return _delay_and_sum(f, cols, offsets, T, I, qa, None, looks, c, dref, w, start, f0, rs, step, nt)


__all__ = ["steering_delays", "array_response", "beam_array_response"]
