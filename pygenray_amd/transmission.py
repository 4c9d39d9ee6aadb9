"""Incoherent transmission loss of a fan on a range-depth grid: ``transmission_loss``, the ray-tube (top hat) sum (DESIGN.md,
"Transmission loss"), and ``beam_transmission_loss``, the same tubes spread as geometric Gaussian beams (DESIGN.md,
"Gaussian beams").

No reference counterpart: pygenray gives back rays, not amplitudes.  Both sums run in HIP (csrc/pgr_tl.h, csrc/pgr_beams.h)
on the fan's trajectories where they already are -- in HBM for a device-resident fan, uploaded through torch for a host
fan.  There is no CPU path.
"""
import numpy as np

from ._fan_frame import _FanFrame, _absorption_profile, _boundary_spec, _min_width
from ._fan_frame import _TracedFan, _lag_spec, _loss_table, _save_grid   # noqa: F401  (lived here: still importable from here)


def _db(out, intensity):
    """an intensity image on the device -> the host array: I itself, or -10 log10(I) dB"""
    I = out.cpu().numpy()
    if intensity:
        return I
    with np.errstate(divide="ignore"):
        return -10.0 * np.log10(I)


def transmission_loss(rays, receiver_depths, environment, flatearth=True, device=0, intensity=False, absorption=None,
                      bottom_loss=None, surface_loss=None):
    """Incoherent ray-tube transmission loss of ``rays`` (a ``RayFan`` from ``shoot_rays``) at ``receiver_depths`` (metres,
    positive down, strictly ascending) on the fan's save ranges -> ndarray ``(len(receiver_depths), S)``:
    ``-10 log10(I)`` dB re 1 m (``+inf`` where no ray tube reaches, NaN in the source's own column), or ``I`` itself with
    ``intensity=True``.  Adjacent rays bound a tube; energy conservation over the tube with cylindrical spreading gives

        I = 0.5 (g_k + g_k+1) |p0_k+1 - p0_k| / (r |z_k+1 - z_k|),   g = c / sqrt(1 - (p c)^2)

    summed, tube by tube in launch order, over the tubes whose depth interval [lo, hi) holds the receiver.  Top hat,
    incoherent, perfect boundary reflection; the sound speed is the bilinear look-up in the environment the fan was traced
    in (``environment`` with ``flatearth`` -- flat-earth depths, as the fan's ``zs`` -- and the mirrored frame of a
    backwards fan).  Known artefacts of the method: spikes at caustics and a strip about one tube wide along the surface
    and the bottom.  A device-resident fan is processed where it is and stays device resident.

    ``absorption`` (default None: none, exactly the call without it): volume absorption along the ray paths, a scalar in
    dB/km (``thorp_absorption(f)``) or a pair ``(depths_m, dB_per_km)`` (depths positive down, strictly ascending, in the
    frame's depths as ``receiver_depths``; linear between the nodes, held outside them).  Every ray's g is then weighted by
    10^(-A / 10), A the ray's running loss in dB (``path_loss``), so a tube carries the mean of its two rays' weighted g.
    The weights are one trajectory array on the device for the duration of the call: 0.8 GB for 1e5 rays x 1001 samples,
    8 GB at 1e6 rays.

    ``bottom_loss`` / ``surface_loss`` (default None and None: perfect reflection, exactly the call without them): the loss
    at every bounce off that boundary, a scalar in dB per bounce or a pair ``(grazing_deg, dB)`` (linear between the
    nodes, held outside them; the grazing angle is taken against the sloping bottom).  Every ray's g is weighted by
    10^(-B / 10), B the loss of the bounces that precede the sample (``boundary_loss``); with ``absorption`` the weight is
    10^(-(A + B) / 10).  Needs a fan traced with a bounce log, ``shoot_rays(..., max_bounces=K)``: ``ValueError`` otherwise."""
    profile = None if absorption is None else _absorption_profile(absorption)
    boundary = _boundary_spec(rays, bottom_loss, surface_loss)
    f = _FanFrame(rays, receiver_depths, environment, flatearth, "transmission_loss").to_device(device).absorb(profile, boundary)
    out = f.image()
    f.run("intensity", f.d_depths.data_ptr(), len(f.depths), out.data_ptr())
    return _db(out, intensity)


def beam_transmission_loss(rays, receiver_depths, environment, flatearth=True, device=0, intensity=False, min_width=10.0,
                           absorption=None, bottom_loss=None, surface_loss=None):
    """Incoherent Gaussian-beam transmission loss of ``rays`` (a ``RayFan`` from ``shoot_rays``) at ``receiver_depths``
    (metres, positive down, strictly ascending) on the fan's save ranges -> ndarray ``(len(receiver_depths), S)``:
    ``-10 log10(I)`` dB re 1 m (``+inf`` where no beam reaches, NaN in the source's own column), or ``I`` itself with
    ``intensity=True``.  The ray tubes of ``transmission_loss``, each spread over depth as a geometric Gaussian beam instead
    of a top hat (as in Bellhop): tube k (rays k, k + 1) carries

        E_k = 0.5 (g_k + g_k+1) |p0_k+1 - p0_k| / r,   g = c / sqrt(1 - (p c)^2)

    (transmission_loss's I times the tube's depth extent) in a Gaussian of centre m_k = (d_k + d_k+1) / 2 and width
    sigma_k = max(|Δd_k-1|, |Δd_k|, |Δd_k+1|, min_width) -- the widest of the tube and its two neighbours, so that a tube
    folded at a reflection spreads a full tube's energy over a full tube's width -- and

        I(d) = sum_k  A_k [G(d - m_k) + G(d + m_k) + G(d - 2 b + m_k)],   A_k = E_k / (sigma_k sqrt(2 pi)),
        G(e) = exp(-e^2 / (2 sigma_k^2)) for |e| <= 4 sigma_k, else 0,

    summed tube by tube in launch order: the beam and its images in the surface and in the bottom b (the bathymetry at each
    save range), which fold the energy that would leave the water column back into it.  Beams are cut at 4 sigma (the mass
    lost, 1 - erf(2 sqrt 2) = 6.3e-5, is 2.8e-4 dB).  ``min_width`` (metres, > 0) is a floor on the beam width: about a
    wavelength c / f.  Incoherent, perfect boundary reflection; the sound speed and bathymetry are those of the environment
    the fan was traced in (``environment`` with ``flatearth``; the mirrored frame of a backwards fan).  Unlike the top hat,
    no spikes at caustics and no strip along the boundaries; receivers outside [0, b] get what the formula gives.  A
    device-resident fan is processed where it is and stays device resident.

    ``absorption``: volume absorption as in ``transmission_loss`` (E_k takes the weighted g; None, the default, runs
    exactly the call without it; one trajectory array of device memory for the duration of the call).
    ``bottom_loss`` / ``surface_loss``: boundary reflection loss as in ``transmission_loss`` (None and None: exactly the
    call without them; a fan with a bounce log otherwise)."""
    w = _min_width(min_width)
    profile = None if absorption is None else _absorption_profile(absorption)
    boundary = _boundary_spec(rays, bottom_loss, surface_loss)
    f = _FanFrame(rays, receiver_depths, environment, flatearth, "beam_transmission_loss").to_device(device).absorb(profile, boundary)
    out, d_b = f.image(), f.upload(f.bottom())
    f.run("beam_intensity", d_b.data_ptr(), f.d_depths.data_ptr(), len(f.depths), w, out.data_ptr())
    return _db(out, intensity)


__all__ = ["transmission_loss", "beam_transmission_loss"]
