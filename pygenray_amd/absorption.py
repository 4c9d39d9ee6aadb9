"""Volume absorption and path length along the rays of a fan: ``thorp_absorption``, ``path_length``, ``path_loss``
("Path integrals and volume absorption").

No reference counterpart: pygenray gives back rays, not amplitudes.  The running integral of alpha ds along every ray,
ds = c dT, runs in HIP (csrc/pgr_path.h) on the fan's trajectories where they already are -- in HBM for a device-resident
fan, uploaded through torch for a host fan.  There is no CPU path.  ``transmission_loss``, ``beam_transmission_loss`` and
``arrivals`` take the same integral as their ``absorption`` keyword.
"""
import numpy as np

from .ray_objects import _columns
from ._fan_frame import _TracedFan, _absorption_profile, _check_flatearth, _save_grid


def thorp_absorption(frequency_hz):
    """Thorp's sea-water absorption at ``frequency_hz`` (Hz, > 0; scalar or array) -> dB/km:
    ``0.11 f^2 / (1 + f^2) + 44 f^2 / (4100 + f^2) + 2.75e-4 f^2 + 0.003`` with f in kHz.  About 0.01 dB/km at 250 Hz and
    0.07 dB/km at 1 kHz: 10 and 70 dB over 1000 km."""
    f = np.asarray(frequency_hz, dtype=float)
    if not np.all(np.isfinite(f)) or not np.all(f > 0):
        raise ValueError("frequency_hz must be finite and > 0")
    f2 = (f / 1000.0) ** 2
    a = 0.11 * f2 / (1.0 + f2) + 44.0 * f2 / (4100.0 + f2) + 2.75e-4 * f2 + 0.003
    return float(a) if a.ndim == 0 else a


def _path_integral(rays, environment, profile, flatearth, range_indices, device):
    """(M, n) host array: the running path integral of ``rays`` at the save columns asked for (selected on the device)"""
    _check_flatearth(environment, flatearth)
    M = len(rays)
    if M == 0:
        raise ValueError("the fan has no rays")
    f = _TracedFan(rays, _save_grid(rays), environment, flatearth)
    S = len(f.x)
    cols = np.arange(S, dtype=np.int32) if range_indices is None else _columns(range_indices, S)
    f.to_device(device)
    import torch
    A = f.path_integral(*profile)
    if range_indices is not None:
        A = A[torch.from_numpy(cols.astype(np.int64)).to(f.dev)]
    return A.cpu().numpy().T


def path_length(rays, environment, flatearth=True, range_indices=None, device=0):
    """The path length of every ray of ``rays`` (a ``RayFan`` from ``shoot_rays``) from the source to the save columns
    ``range_indices`` (default: all S; any integers in -S .. S - 1) -> ndarray ``(M, n)``, metres: the trapezoid sum of
    ds = c dT over the ray's samples, added in order from 0.0 (0 in column 0, NaN from a NaN sample on), c the
    bilinear look-up in the environment the fan was traced in (``environment`` with ``flatearth``; the mirrored frame of a
    backwards fan).

    Depths and sound speed are those of the traced frame: with ``flatearth=True`` this is the FLAT-EARTH length, longer
    than the true one by a factor of at most exp(z / R_earth), about 1 + 8e-4 at 5 km depth.  A device-resident fan is
    processed where it is and stays device resident; the integral takes one trajectory array of device memory (0.8 GB for
    1e5 rays x 1001 samples, 8 GB at 1e6 rays) and only the columns asked for are copied to the host."""
    return _path_integral(rays, environment, (None, np.ones(1)), flatearth, range_indices, device)


def path_loss(rays, environment, absorption, flatearth=True, range_indices=None, device=0):
    """The volume-absorption loss of every ray of ``rays`` from the source to the save columns ``range_indices`` (default:
    all S) -> ndarray ``(M, n)``, dB: the integral of alpha ds along the ray, ds = c dT, by the trapezoid rule over the
    ray's samples, added in order from 0.0.  ``absorption``: a scalar in dB/km (``thorp_absorption(f)``), or a pair
    ``(depths_m, dB_per_km)`` -- depths positive down, strictly ascending, in the frame's depths as ``receiver_depths``
    are; linear between the nodes, held at the end values outside them.  Frame, flat-earth caveat (the lengths are the
    traced frame's, at most 8e-4 long at 5 km), device residency and memory as ``path_length``, which is this with 1 dB/m.
    ``transmission_loss(..., absorption=...)`` weights every ray's g by 10^(-path_loss / 10)."""
    return _path_integral(rays, environment, _absorption_profile(absorption), flatearth, range_indices, device)


__all__ = ["thorp_absorption", "path_length", "path_loss"]
