"""Coherent field of a fan: ``caustic_index``, ``pressure_field``, ``coherent_transmission_loss`` ("Coherent
ray-tube pressure") and ``beam_pressure_field``, ``coherent_beam_transmission_loss``, the same tubes spread as geometric
Gaussian beams with the wavefront curvature in their phase ("Coherent Gaussian-beam pressure").

No reference counterpart: pygenray gives back rays, not amplitudes.  The caustic index of every tube and the coherent sums
run in HIP (csrc/pgr_phase.h, csrc/pgr_beam_phase.h) on the fan's trajectories where they already are -- in HBM for a device-resident
fan, uploaded through torch for a host fan.  There is no CPU path.
"""
import numpy as np

from ._fan_frame import (_TracedFan, _check_flatearth, _coherent_frame, _frequency, _kappa, _lag_spec, _loss_table, _min_width,
                         _phase_index, _needs_counts, _save_grid)


def _loss_db(p):
    """a complex pressure -> -20 log10 |p| dB (+inf where it is 0)"""
    with np.errstate(divide="ignore"):
        return -20.0 * np.log10(np.abs(p))


def caustic_index(rays, env=None, flatearth=True, device=0):
    """The number of caustics every ray tube of ``rays`` (a ``RayFan`` from ``shoot_rays``) has passed on its way to every
    save range -> int64 ndarray ``(M - 1, S)``; tube k is rays k and k + 1.  A tube passes a caustic where its signed width
    d_k+1 - d_k changes sign between two save ranges -- with the mirror flips of reflections undone: the width is taken
    times (-1)^(bounces), and a sample at which the two rays have bounced a different number of times (the tube is folded
    over the boundary), or at which either ray has no sample, is passed over.  Column 0 (every ray at the source) never
    counts.  The save grid must resolve the caustics: two between consecutive save ranges cancel.

    A fan none of whose rays bounced (``n_botts`` and ``n_surfs`` all zero) needs nothing else; a fan with bounces needs
    its bounce log (``shoot_rays(..., max_bounces=K)``) and ``env`` (with ``flatearth``), the environment it was traced in
    -- ``ValueError`` naming ``max_bounces`` without a log or with one that overflowed.  A device-resident fan is processed
    where it is and stays device resident."""
    if len(rays) < 2:
        raise ValueError("caustic_index needs a fan of at least 2 rays (one ray tube)")
    counts = _needs_counts(rays)
    if env is not None:
        _check_flatearth(env, flatearth)
        f = _TracedFan(rays, _save_grid(rays), env, flatearth).to_device(device)
        nb = ns = None
        if counts:
            zero = (_loss_table(None, "bottom_loss"), _loss_table(None, "surface_loss"))
            _, nb, ns = f.boundary_loss(zero, counts=True)
        kappa = _kappa(f, nb, ns)
    elif counts:
        raise ValueError("caustic_index of a fan with bounces needs `env`, the environment the fan was traced in")
    else:
        handle = rays.__dict__.get("_dev")
        S = handle.S if handle is not None else np.shape(rays.zs)[1]        # (no frame: of the save ranges only their number)
        f = _TracedFan(rays, np.empty(S), None, flatearth).on_device(handle._env.device if handle is not None else int(device))
        kappa = _kappa(f, None, None)
    return kappa[:, :-1].cpu().numpy().T.astype(np.int64)


def pressure_field(rays, receiver_depths, env, frequency, absorption=None, bottom_loss=None, surface_loss=None, flatearth=True,
                   device=0):
    """Coherent ray-tube pressure of ``rays`` (a ``RayFan`` from ``shoot_rays``) at ``receiver_depths`` (metres, positive
    down, strictly ascending) on the fan's save ranges, at ``frequency`` (Hz, finite, >= 0) -> complex128 ndarray
    ``(len(receiver_depths), S)``, re 1 m: 0 where no ray tube reaches, NaN in the source's own column.  Every tube that
    ``transmission_loss`` counts at a receiver -- each arrival of ``arrivals`` -- adds

        sqrt(I) exp(i (2 pi f T - (pi / 2) q)),   q = kappa + 2 n_surf

    with the arrival's own intensity I and travel time T (interpolated across the tube), kappa the tube's
    ``caustic_index`` (-pi/2 per caustic) and n_surf its surface bounces so far (pi each: a pressure-release surface); the
    bottom is rigid, phase 0, unless ``bottom_loss`` is a ``BottomReflection`` (``fluid_halfspace(...)``, or a table from
    elsewhere): every bottom bounce then also turns the phase by arg R at its grazing angle -- the term gains
    exp(-2 pi i phi), phi the lag in cycles the tube's two rays have collected at their bottom bounces so far (the bounce
    post-pass run once more on the table's lag), interpolated across the tube as T is.  Summed tube by tube in launch order, so ``abs(p) ** 2`` is ``transmission_loss``'s
    intensity wherever one tube arrives.  A tube whose two rays have bounced a different number of times (folded over a
    boundary) is left out, and a bounce counts from the save range nearest to it, where the ray's sample before the bounce
    is the reflected segment continued backwards, beyond the boundary: arrivals are missing in a strip up to
    tan(theta_max) dx / 2 wide along both boundaries (dx the save step, theta_max the steepest ray's angle there), not
    just one tube's width.  The tube spike at a caustic remains.  ``absorption``, ``bottom_loss``, ``surface_loss``: the weights of ``transmission_loss``, exactly (amplitudes
    take their square root through I).  The frame and the sound speed are ``transmission_loss``'s.  A fan with bounces
    needs its bounce log (``shoot_rays(..., max_bounces=K)``): ``ValueError`` otherwise.  A device-resident fan is
    processed where it is and stays device resident."""
    f0 = _frequency(frequency)
    f, profile, boundary, counts = _coherent_frame(rays, receiver_depths, env, absorption, bottom_loss, surface_loss, flatearth,
                                                   "pressure_field")
    f.to_device(device).absorb(profile, boundary, counts=counts)      # (one run of the boundary loss: weights and counts)
    import torch
    q = _phase_index(f, counts)
    lag = _lag_spec(bottom_loss)
    re, im = f.image(), f.image()
    if lag is None:
        f.run("pressure", q.data_ptr(), f0, f.d_depths.data_ptr(), len(f.depths), re.data_ptr(), im.data_ptr())
    else:
        phi = f.boundary_loss(lag)                                        # (S, M): the post-pass once more, lags for dB
        f.run("pressure_phi", q.data_ptr(), phi.data_ptr(), f0, f.d_depths.data_ptr(), len(f.depths), re.data_ptr(),
              im.data_ptr())
    return torch.complex(re, im).cpu().numpy()


def coherent_transmission_loss(rays, receiver_depths, env, frequency, absorption=None, bottom_loss=None, surface_loss=None,
                               flatearth=True, device=0):
    """Coherent ray-tube transmission loss: ``-20 log10 |p|`` dB re 1 m of ``pressure_field``, whose arguments it takes
    (``+inf`` where no ray tube reaches or the paths cancel, NaN in the source's own column)."""
    return _loss_db(pressure_field(rays, receiver_depths, env, frequency, absorption=absorption, bottom_loss=bottom_loss,
                                   surface_loss=surface_loss, flatearth=flatearth, device=device))


def beam_pressure_field(rays, receiver_depths, env, frequency, min_width=10.0, curvature=True, absorption=None,
                        bottom_loss=None, surface_loss=None, flatearth=True, device=0):
    """Coherent Gaussian-beam pressure of ``rays`` (a ``RayFan`` from ``shoot_rays``) at ``receiver_depths`` (metres, positive
    down, strictly ascending) on the fan's save ranges, at ``frequency`` (Hz, finite, >= 0) -> complex128 ndarray
    ``(len(receiver_depths), S)``, re 1 m: 0 where no beam reaches, NaN in the source's own column.  The ray tubes of
    ``pressure_field``, each spread over depth as the geometric Gaussian beam of ``beam_transmission_loss`` -- the same centre
    m_k, width sigma_k = max(the tube's and its neighbours' widths, ``min_width``), energy E_k and cut at 4 sigma_k -- and
    carrying the tube's phase: the beam, its image in the pressure-release surface (a half cycle) and its image in the rigid
    bottom each add

        A'_k exp(-e^2 / (2 sigma_k^2)) exp(i (2 pi f (T_m + p_m e + kappa_k e^2 / 2) - (pi / 2) q)),
        A'_k = sqrt(E_k D_k) / (sigma_k sqrt(2 pi)),   kappa_k = (p_k+1 - p_k) / (d_k+1 - d_k)

    with e the receiver's offset from the beam's centre (mirrored with the image), T_m and p_m the means of the two rays'
    travel time and vertical slowness dT/dz, D_k the tube's width and q = kappa + 2 n_surf ``pressure_field``'s phase index.
    Beams D apart and sigma wide, in phase, sum to sqrt(E / D), the tube's amplitude, so away from caustics and boundaries
    the field is ``pressure_field``'s; at a caustic, where D -> 0, A' -> 0 and the field stays bounded by the sum of the
    beams' amplitudes, the receivers along both boundaries are reached by the images, and shadow edges are sigma wide.
    ``curvature`` (default True): kappa_k, the wavefront's curvature across the tube, which keeps a beam much wider than its
    tube (sigma_k = ``min_width``, about a wavelength) accurate; False gives the plain geometric beam, linear phase only.
    kappa_k grows without bound at a caustic while A' -> 0 there.  A tube whose two rays have bounced a different number of
    times adds nothing, as in ``pressure_field``.

    ``absorption``, ``bottom_loss``, ``surface_loss``: the weights of ``transmission_loss``, exactly.  A ``BottomReflection``
    as ``bottom_loss`` is refused with a ``ValueError``: the beam product does not yet apply a complex bottom phase, and its
    magnitude alone would be wrong physics; pass its ``.loss`` pair for the loss without the phase.  The frame, the sound
    speed and the bathymetry are ``beam_transmission_loss``'s.  A fan with bounces needs its bounce log
    (``shoot_rays(..., max_bounces=K)``): ``ValueError`` otherwise.  A device-resident fan is processed where it is and stays
    device resident."""
    f0, w = float(frequency), float(min_width)          # (both converted before either is refused)
    f0, w = _frequency(f0), _min_width(w)
    f, profile, boundary, counts = _coherent_frame(rays, receiver_depths, env, absorption, bottom_loss, surface_loss, flatearth,
                                                   "beam_pressure_field", beams=True)
    f.to_device(device).absorb(profile, boundary, counts=counts)      # (one run of the boundary loss: weights and counts)
    import torch
    q = _phase_index(f, counts)
    re, im, d_b = f.image(), f.image(), f.upload(f.bottom())
    f.run("beam_pressure", q.data_ptr(), f0, d_b.data_ptr(), f.d_depths.data_ptr(), len(f.depths), w, bool(curvature),
          re.data_ptr(), im.data_ptr())
    return torch.complex(re, im).cpu().numpy()


def coherent_beam_transmission_loss(rays, receiver_depths, env, frequency, min_width=10.0, curvature=True, absorption=None,
                                    bottom_loss=None, surface_loss=None, flatearth=True, device=0):
    """Coherent Gaussian-beam transmission loss: ``-20 log10 |p|`` dB re 1 m of ``beam_pressure_field``, whose arguments it
    takes (``+inf`` where no beam reaches or the paths cancel, NaN in the source's own column)."""
    return _loss_db(beam_pressure_field(rays, receiver_depths, env, frequency, min_width=min_width, curvature=curvature,
                                        absorption=absorption, bottom_loss=bottom_loss, surface_loss=surface_loss,
                                        flatearth=flatearth, device=device))


__all__ = ["caustic_index", "pressure_field", "coherent_transmission_loss", "beam_pressure_field",
           "coherent_beam_transmission_loss"]
