"""Boundary reflection loss along the rays of a fan: ``boundary_loss`` ("Bounce log and boundary loss").

No reference counterpart: pygenray gives back rays, not amplitudes.  The loss every ray collects at its surface and bottom
bounces is formed in HIP (csrc/pgr_bounce.h) from the bounce log a fan keeps when it is traced with
``shoot_rays(..., max_bounces=K)`` -- in HBM for a device-resident fan, uploaded through torch for a host fan.  There is no
CPU path.  ``transmission_loss``, ``beam_transmission_loss`` and ``arrivals`` take the same loss as their ``bottom_loss`` /
``surface_loss`` keywords.
"""
import numpy as np

from .ray_objects import _columns
from ._fan_frame import _TracedFan, _check_flatearth, _loss_table, _save_grid


def boundary_loss(rays, environment, bottom_loss=None, surface_loss=None, range_indices=None, flatearth=True, device=0):
    """The reflection loss every ray of ``rays`` (a ``RayFan`` from ``shoot_rays(..., max_bounces=K)``) has collected at its
    bounces on the way to the save columns ``range_indices`` (default: all S; any integers in -S .. S - 1) -> ndarray
    ``(M, n)``, dB.  ``bottom_loss`` / ``surface_loss``: None (no loss at that boundary), a scalar in dB per bounce, or a
    pair ``(grazing_deg, dB)`` -- grazing angles in degrees, strictly ascending; linear between the nodes, held at the end
    values outside them.  The grazing angle of a bounce is that of the reflected ray, degrees(asin(p c)) with the sound
    speed at the boundary, against the horizontal at the surface and against the bottom's own slope at the bottom.  A
    bounce precedes the samples the reference's re-sampling gives the segment that starts at it
    (``RayFan.bounce_counts``); the losses are added in the order the bounces happened, from 0.0.  Frame: the environment
    the fan was traced in (``environment`` with ``flatearth``; the mirrored frame of a backwards fan).  A device-resident
    fan is processed where it is and stays device resident; only the columns asked for are copied to the host."""
    _check_flatearth(environment, flatearth)
    if len(rays) == 0:
        raise ValueError("the fan has no rays")
    spec = (_loss_table(bottom_loss, "bottom_loss"), _loss_table(surface_loss, "surface_loss"))
    if not rays._has_bounce_log():
        raise ValueError("boundary loss needs a fan traced with a bounce log: shoot_rays(..., max_bounces=K)")
    f = _TracedFan(rays, _save_grid(rays), environment, flatearth)
    S = len(f.x)
    cols = np.arange(S, dtype=np.int32) if range_indices is None else _columns(range_indices, S)
    f.to_device(device)
    import torch
    B = f.boundary_loss(spec)
    if range_indices is not None:
        B = B[torch.from_numpy(cols.astype(np.int64)).to(f.dev)]
    return B.cpu().numpy().T


__all__ = ["boundary_loss"]
