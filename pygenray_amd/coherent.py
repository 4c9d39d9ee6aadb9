"""Coherent field of a fan: ``caustic_index``, ``pressure_field``, ``coherent_transmission_loss`` ("Coherent
ray-tube pressure") and ``beam_pressure_field``, ``coherent_beam_transmission_loss``, the same tubes spread as geometric
Gaussian beams with the wavefront curvature in their phase ("Coherent Gaussian-beam pressure").

No reference counterpart: pygenray gives back rays, not amplitudes.  The caustic index of every tube and the coherent sums
run in HIP (csrc/pgr_phase.h, csrc/pgr_beam_phase.h) on the fan's trajectories where they already are -- in HBM for a device-resident
fan, uploaded through torch for a host fan.  There is no CPU path.
"""
import numpy as np

from . import _lib
from .reflection import BottomReflection
from .transmission import (_FanFrame, _TracedFan, _absorption_profile, _boundary_spec, _check_flatearth, _lag_spec,
                           _loss_table, _ptr, _save_grid)


def _needs_counts(rays):
    """False for a fan none of whose rays bounced; True for a bounced fan whose bounce log holds every bounce; a bounced fan
    without such a log is refused.  Nothing is fetched or launched."""
    total = np.asarray(rays.n_botts, dtype=np.int64) + np.asarray(rays.n_surfs, dtype=np.int64)
    if len(total) == 0 or not total.any():
        return False
    if not rays._has_bounce_log():
        raise ValueError("the fan's rays bounce and it has no bounce log: the caustic index needs the bounces at every save "
                         "range, trace the fan with shoot_rays(..., max_bounces=K)")
    log = rays.__dict__.get("_bounces")
    K = log.capacity if log is not None else rays.__dict__["_dev"].K
    if int(total.max()) > K:
        raise ValueError(f"the fan's bounce log overflowed: a ray bounces {int(total.max())} times and the log holds {K} "
                         f"(max_bounces={int(total.max())} holds every bounce)")
    return True


def _kappa(f, nb, ns):
    """kappa [S][M] int32 on the device of the traced fan `f` (a _TracedFan after to_device) from the per-sample bounce counts
    nb, ns [S][M] int32 on that device (None, None: a fan without bounces)"""
    import torch
    S, M = len(f.x), len(f.rays)
    kappa = torch.empty((S, M), dtype=torch.int32, device=f.dev)
    if f.handle is not None:
        f.handle.caustic_index(_ptr(nb), _ptr(ns), kappa.data_ptr(), f.stream)
    else:
        _lib.caustic_index_device(f.env.device, f._host_fan("zs"), M, S, _ptr(nb), _ptr(ns), kappa.data_ptr(), f.stream)
    return kappa


def _phase_index(f, counts):
    """q [S][M] int32 on the device of the frame `f` (a _FanFrame after to_device and absorb(..., counts=counts)): the tubes'
    phase index in quarter cycles, kappa + 2 n_surf where the tube's two rays have bounced alike and -1 (the tube adds
    nothing) elsewhere; kappa itself for a fan without bounces (`counts` False)."""
    import torch
    nb, ns = f.d_counts if counts else (None, None)
    q = _kappa(f, nb, ns)
    if counts:
        # on the device: kappa + 2 n_surf where the tube's two rays have bounced alike, -1 (the tube adds nothing) elsewhere
        same = (nb[:, :-1] == nb[:, 1:]) & (ns[:, :-1] == ns[:, 1:])
        q[:, :-1] = torch.where(same, q[:, :-1] + 2 * ns[:, :-1], torch.full_like(q[:, :-1], -1))
    return q


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
    import torch
    handle = rays.__dict__.get("_dev")
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
        M = len(rays)
        dev = torch.device("cuda", handle._env.device if handle is not None else int(device))
        stream = torch.cuda.current_stream(dev).cuda_stream
        if handle is not None:
            kappa = torch.empty((handle.S, M), dtype=torch.int32, device=dev)
            handle.caustic_index(0, 0, kappa.data_ptr(), stream)
        else:
            z = torch.from_numpy(np.ascontiguousarray(np.asarray(rays.zs, dtype=float).T)).to(dev)
            kappa = torch.empty(tuple(z.shape), dtype=torch.int32, device=dev)
            _lib.caustic_index_device(dev.index, z.data_ptr(), M, z.shape[0], 0, 0, kappa.data_ptr(), stream)
            torch.cuda.current_stream(dev).synchronize()               # (the upload is freed when this returns)
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
    f0 = float(frequency)
    if not (np.isfinite(f0) and f0 >= 0):
        raise ValueError("frequency must be finite and >= 0 Hz")
    profile = None if absorption is None else _absorption_profile(absorption)
    boundary = _boundary_spec(rays, bottom_loss, surface_loss)
    f = _FanFrame(rays, receiver_depths, env, flatearth, "pressure_field")
    counts = _needs_counts(rays)
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
    p = pressure_field(rays, receiver_depths, env, frequency, absorption=absorption, bottom_loss=bottom_loss,
                       surface_loss=surface_loss, flatearth=flatearth, device=device)
    with np.errstate(divide="ignore"):
        return -20.0 * np.log10(np.abs(p))


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
    f0, w = float(frequency), float(min_width)
    if not (np.isfinite(f0) and f0 >= 0):
        raise ValueError("frequency must be finite and >= 0 Hz")
    if not (np.isfinite(w) and w > 0):
        raise ValueError("min_width must be finite and > 0")
    if isinstance(bottom_loss, BottomReflection):
        raise ValueError("beam_pressure_field does not yet apply a complex bottom phase: a BottomReflection as bottom_loss is "
                         "refused (its magnitude alone would be wrong physics); pass bottom_loss=reflection.loss for the "
                         "loss without the phase")
    profile = None if absorption is None else _absorption_profile(absorption)
    boundary = _boundary_spec(rays, bottom_loss, surface_loss)
    f = _FanFrame(rays, receiver_depths, env, flatearth, "beam_pressure_field")
    counts = _needs_counts(rays)
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
    p = beam_pressure_field(rays, receiver_depths, env, frequency, min_width=min_width, curvature=curvature,
                            absorption=absorption, bottom_loss=bottom_loss, surface_loss=surface_loss, flatearth=flatearth,
                            device=device)
    with np.errstate(divide="ignore"):
        return -20.0 * np.log10(np.abs(p))


__all__ = ["caustic_index", "pressure_field", "coherent_transmission_loss", "beam_pressure_field",
           "coherent_beam_transmission_loss"]
