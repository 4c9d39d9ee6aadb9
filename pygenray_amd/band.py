"""``band_intensity`` and ``band_transmission_loss``: the power a receiver takes from a band of frequencies, sum_k w_k |H(f_k)|^2,
and its level in dB -- the band-averaged transmission loss of a third-octave band or a source spectrum -- with their Gaussian-beam
twins ``beam_band_intensity`` and ``beam_band_transmission_loss`` ("Band-averaged transmission loss").

No reference counterpart: pygenray gives back rays, not amplitudes.  H is ``transfer_function``'s, term for term, and is never
stored: the kernel that forms it at every frequency reduces it over the band where it stands (csrc/pgr_band.h), so a range-depth
map costs its own (R, n) values of memory, not (R, n, F).  The fan, the arrivals and the sum stay on the device -- in HBM for a
device-resident fan, uploaded through torch for a host fan.  There is no CPU path.
"""
import math

import numpy as np

from . import _lib
from ._fan_frame import (_arrival_columns, _arrival_lengths, _arrival_terms, _band, _band_absorption, _check_fits,
                         _coherent_frame, _lag_spec, _one_zero, _ptr)
from .beam_arrivals import _beam_frame, _device_beam_arrivals, _sum_terms
from .ray_objects import _columns


def _band_weights(weights, F):
    """``weights`` of the band products, checked -> contiguous float64 (F,): None is 1 / F each"""
    if weights is None:
        return np.full(F, 1.0 / F)
    w = np.asarray(weights, dtype=float)
    if w.shape != (F,):
        raise ValueError(f"weights must hold one weight per frequency ({F})")
    if not np.all(np.isfinite(w)) or np.any(w < 0):
        raise ValueError("weights must be finite and >= 0")
    if not np.any(w > 0):
        raise ValueError("weights must not all be zero")
    return np.ascontiguousarray(w)


def _level_db(P):
    """a band intensity -> -10 log10 P dB (+inf where it is 0)"""
    with np.errstate(divide="ignore"):
        return -10.0 * np.log10(P)


def _band_power(f, cols, offsets, T, I, qa, phi, La, freq, alpha, wf):
    """pgr_band_power_device over the arrival lists of the frame `f` (on the device, R * n groups) -> float64 (R, n) on the host,
    the source's own columns NaN"""
    import torch
    R, n = len(f.depths), len(cols)
    out = torch.empty((R, n), dtype=torch.float64, device=f.dev)
    _lib.band_power_sum(f.env.device, offsets.data_ptr(), R * n, T.data_ptr(), I.data_ptr(), qa.data_ptr(), _ptr(phi), _ptr(La),
                        freq, alpha, wf, out.data_ptr(), f.stream)
    at_source = np.flatnonzero(np.abs(np.asarray(f.x)[cols] - f.x[0]) == 0)
    if len(at_source):                                                # the source's own column, as pressure_field has it
        out.index_fill_(1, torch.from_numpy(at_source).to(f.dev), math.nan)
    return out.cpu().numpy()


def band_intensity(rays, receiver_depths, env, frequencies, weights=None, range_indices=None, absorption=None, bottom_loss=None,
                   surface_loss=None, flatearth=True, device=0):
    """The power the channel passes from the source of ``rays`` (a ``RayFan`` from ``shoot_rays``) to ``receiver_depths``
    (metres, positive down, strictly ascending) at the save columns ``range_indices`` (default ``[S - 1]``), summed over the
    band ``frequencies`` (Hz; a non-empty 1-D sequence, finite, >= 0) -> float64 ndarray ``(R, n)``, re 1 m:

        P = sum_k w_k |H(f_k)|^2,   H = transfer_function(..., frequencies)   (``t_reduce`` does not enter |H|)

    ``weights``: None, 1 / F each (the band average); else F finite values >= 0, not all zero, used as given -- a source
    spectrum.  Every H(f_k) is ``transfer_function``'s, term for term and in its order, and P is summed in a fixed order
    (DESIGN.md section 23): with one frequency and ``weights=[1.0]`` it is re^2 + im^2 of ``pressure_field`` bit for bit.  H
    is not stored: the map needs ``(R, n)`` values of device memory whatever F.  A requested column with r = 0 is NaN.

    ``absorption`` (a callable such as ``thorp_absorption`` makes it follow the frequency), ``bottom_loss`` (a
    ``BottomReflection`` also turns every arrival by its bottom bounces' phase), ``surface_loss``, the frame and every error
    are ``transfer_function``'s.  ``ValueError`` when the output does not fit in the free device memory, before any kernel
    runs.  A device-resident fan is processed where it is and stays device resident."""
    freq = _band(frequencies)
    wf = _band_weights(weights, len(freq))
    alpha = _band_absorption(absorption, freq) if callable(absorption) else None
    f, profile, boundary, counts = _coherent_frame(rays, receiver_depths, env, None if callable(absorption) else absorption,
                                                   bottom_loss, surface_loss, flatearth, "band_intensity")
    cols = _columns(range_indices, len(f.x))
    f.to_device(device)
    _check_fits(f, len(f.depths), len(cols), 1, "band intensity", "values", kind="real")
    lag = _lag_spec(bottom_loss)
    offsets, tube, w, T, I, qa, col, *phi = _arrival_terms(f, cols, profile, boundary, counts, lag)
    La = None
    if alpha is not None:
        La = _arrival_lengths(f, col, tube, w) if len(tube) else _one_zero(f.dev)
    return _band_power(f, cols, offsets, T, I, qa, phi[0] if phi else None, La, freq, alpha, wf)


def band_transmission_loss(rays, receiver_depths, env, frequencies, weights=None, range_indices=None, absorption=None,
                           bottom_loss=None, surface_loss=None, flatearth=True, device=0):
    """Band-averaged transmission loss: ``-10 log10 P`` dB re 1 m of ``band_intensity``, whose arguments it takes (``+inf``
    where no ray tube reaches, NaN in the source's own column)."""
    return _level_db(band_intensity(rays, receiver_depths, env, frequencies, weights=weights, range_indices=range_indices,
                                    absorption=absorption, bottom_loss=bottom_loss, surface_loss=surface_loss,
                                    flatearth=flatearth, device=device))


def beam_band_intensity(rays, receiver_depths, env, frequencies, weights=None, min_width=10.0, curvature=True,
                        range_indices=None, absorption=None, bottom_loss=None, surface_loss=None, flatearth=True, device=0):
    """``band_intensity`` summed over the beam arrivals of ``beam_arrivals`` instead of the tube arrivals -> float64 ndarray
    ``(R, n)``: P = sum_k w_k |H(f_k)|^2 with H ``beam_transfer_function``'s, term for term.  ``frequencies``, ``weights``
    and their errors are ``band_intensity``'s; ``min_width``, ``curvature``, ``absorption`` (with a callable the arrival's
    path length is the mean of its tube's two rays), the boundary weights, the memory check by the arrivals' count and every
    other error are ``beam_transfer_function``'s (a ``BottomReflection`` as ``bottom_loss`` is refused).  A device-resident
    fan is processed where it is and stays device resident."""
    freq = _band(frequencies)
    wf = _band_weights(weights, len(freq))
    alpha = _band_absorption(absorption, freq) if callable(absorption) else None
    f, cols, width, profile, boundary, counts = _beam_frame(rays, receiver_depths, env, min_width, range_indices,
                                                            None if callable(absorption) else absorption, bottom_loss,
                                                            surface_loss, flatearth, "beam_band_intensity")
    f.to_device(device)
    _check_fits(f, len(f.depths), len(cols), 1, "band intensity", "values", kind="real")
    # (what beam_transfer_function forms of the arrivals behind the emit pass)
    offsets, tube, _, T, amp, qa = _device_beam_arrivals(f, cols, width, curvature, profile, boundary, counts,
                                                         extra_bytes=8 if alpha is None else 8 + 3 * 8 + 4 * 8,
                                                         fixed_bytes=0 if alpha is None else 8 * len(f.x) * len(f.rays))
    La = None
    if alpha is not None:
        La = _one_zero(f.dev)
        if len(tube):
            La = _arrival_lengths(f, _arrival_columns(f, offsets, cols), tube, 0.5).contiguous()
    T, I, qa = _sum_terms(T, amp, qa)
    return _band_power(f, cols, offsets, T, I, qa, None, La, freq, alpha, wf)


def beam_band_transmission_loss(rays, receiver_depths, env, frequencies, weights=None, min_width=10.0, curvature=True,
                                range_indices=None, absorption=None, bottom_loss=None, surface_loss=None, flatearth=True,
                                device=0):
    """Band-averaged Gaussian-beam transmission loss: ``-10 log10 P`` dB re 1 m of ``beam_band_intensity``, whose arguments it
    takes."""
    return _level_db(beam_band_intensity(rays, receiver_depths, env, frequencies, weights=weights, min_width=min_width,
                                         curvature=curvature, range_indices=range_indices, absorption=absorption,
                                         bottom_loss=bottom_loss, surface_loss=surface_loss, flatearth=flatearth, device=device))


__all__ = ["band_intensity", "band_transmission_loss", "beam_band_intensity", "beam_band_transmission_loss"]
