"""Incoherent transmission loss of a fan on a range-depth grid: ``transmission_loss``, the ray-tube (top hat) sum (DESIGN.md,
"Transmission loss"), and ``beam_transmission_loss``, the same tubes spread as geometric Gaussian beams (DESIGN.md,
"Gaussian beams").

No reference counterpart: pygenray gives back rays, not amplitudes.  Both sums run in HIP (csrc/pgr_tl.h, csrc/pgr_beams.h)
on the fan's trajectories where they already are -- in HBM for a device-resident fan, uploaded through torch for a host
fan.  There is no CPU path.
"""
import numpy as np

from . import _lib
from .environment import _mirror_envi_arrays, _unpack_envi
from .host_physics import bilinear_interp, linear_interp
from .launch_rays import _device_env, _initial_slowness

_NO_FE_MSG = ("Flat earth transformation has not been applied. Set `flat_earth_transform=True` "
              "when creating the OceanEnvironment2D object.")


def _check_arguments(rays, receiver_depths, environment, flatearth, who="transmission_loss"):
    """Everything that can be refused without a GPU; -> (depths, save ranges x, source depth)."""
    d = np.asarray(receiver_depths, dtype=float)
    if d.ndim != 1 or len(d) == 0:
        raise ValueError("receiver_depths must be a non-empty 1-D sequence")
    if not np.all(np.isfinite(d)):
        raise ValueError("receiver_depths must be finite")
    if not np.all(np.diff(d) > 0):
        raise ValueError("receiver_depths must be strictly ascending")
    if flatearth and not hasattr(environment, "sound_speed_fe"):
        raise ValueError(_NO_FE_MSG)
    if len(rays) < 2:
        raise ValueError(f"{who} needs a fan of at least 2 rays (one ray tube)")
    sd = np.asarray(rays.source_depths, dtype=float)
    if not np.all(sd == sd[0]):
        raise ValueError("the fan mixes source depths: ray tubes need one source")
    r = rays.__dict__.get("_r")
    if r is not None and rays.__dict__.get("_rs") is None:
        x = np.asarray(r, dtype=float)          # (a device fan: one save grid by construction)
    else:
        rs = np.asarray(rays.rs, dtype=float)
        x = rs[0]
        if not np.array_equal(rs, np.broadcast_to(x, rs.shape)):
            raise ValueError("the rows of rays.rs differ: the fan must share one save grid")
    return np.ascontiguousarray(d), x, float(sd[0])


class _FanFrame:
    """A fan checked for the tube kernels (`who` names the caller in errors): the receiver depths and the save ranges x.
    ``to_device`` then sets up the frame the fan was traced in -- xf (mirrored for a backwards fan), the EnvHandle and its
    tables (cin, rin, zin), the launch slowness p0, the device copies of p0 and the depths, the torch stream and the fan's
    device handle (None for a host fan)."""

    def __init__(self, rays, receiver_depths, environment, flatearth, who):
        self.depths, self.x, self.source_depth = _check_arguments(rays, receiver_depths, environment, flatearth, who)
        self.rays, self.environment, self.flatearth = rays, environment, flatearth

    def to_device(self, device):
        import torch

        x = self.x
        self.backwards = len(x) > 1 and x[-1] < x[0]
        self.xf = -x if self.backwards else x            # the frame the fan was traced in
        self.env, self.tables = _device_env(self.environment, self.flatearth, self.backwards, device)
        cin, rin, zin = self.tables
        c_source = bilinear_interp(self.xf[0], self.source_depth, rin, zin, cin)
        self.p0 = _initial_slowness(self.rays.thetas, c_source)
        self.dev = torch.device("cuda", self.env.device)
        self.d_p0 = torch.from_numpy(np.ascontiguousarray(self.p0)).to(self.dev)
        self.d_depths = torch.from_numpy(self.depths).to(self.dev)
        self.stream = torch.cuda.current_stream(self.dev).cuda_stream
        self.handle = self.rays.__dict__.get("_dev")
        if self.handle is not None and self.handle._env is not self.env:
            raise ValueError("the fan was traced in another environment (or flatearth setting) than the one given")
        return self

    def upload_rows(self, a):
        """A host fan's (M, S) array as the (S, M) device rows the kernels read (the transposed view shoot_rays hands out is
        that layout already)."""
        import torch
        return torch.from_numpy(np.ascontiguousarray(np.asarray(a, dtype=float).T)).to(self.dev)

    def upload_x(self):
        import torch
        return torch.from_numpy(np.ascontiguousarray(self.xf)).to(self.dev)

    def bottom(self):
        """The bottom depth at each save range in the frame the fan was traced in (flat-earth, mirrored for a backwards fan):
        host_physics.linear_interp of the bathymetry at xf."""
        cin, cpin, rin, _, depths, depth_ranges, angles = _unpack_envi(self.environment, flatearth=self.flatearth)
        if self.backwards:
            depths, depth_ranges = _mirror_envi_arrays(cin, cpin, rin, depths, depth_ranges, angles)[3:5]
        return np.array([linear_interp(float(v), depth_ranges, depths) for v in self.xf])


def transmission_loss(rays, receiver_depths, environment, flatearth=True, device=0, intensity=False):
    """Incoherent ray-tube transmission loss of ``rays`` (a ``RayFan`` from ``shoot_rays``) at ``receiver_depths`` (metres,
    positive down, strictly ascending) on the fan's save ranges -> ndarray ``(len(receiver_depths), S)``:
    ``-10 log10(I)`` dB re 1 m (``+inf`` where no ray tube reaches, NaN in the source's own column), or ``I`` itself with
    ``intensity=True``.  Adjacent rays bound a tube; energy conservation over the tube with cylindrical spreading gives

        I = 0.5 (g_k + g_k+1) |p0_k+1 - p0_k| / (r |z_k+1 - z_k|),   g = c / sqrt(1 - (p c)^2)

    summed, tube by tube in launch order, over the tubes whose depth interval [lo, hi) holds the receiver.  Top hat,
    incoherent, perfect boundary reflection; the sound speed is the bilinear look-up in the environment the fan was traced
    in (``environment`` with ``flatearth`` -- flat-earth depths, as the fan's ``zs`` -- and the mirrored frame of a
    backwards fan).  Known artefacts of the method: spikes at caustics and a strip about one tube wide along the surface
    and the bottom.  A device-resident fan is processed where it is and stays device resident."""
    f = _FanFrame(rays, receiver_depths, environment, flatearth, "transmission_loss").to_device(device)
    import torch

    R, S = len(f.depths), len(f.x)
    out = torch.empty((R, S), dtype=torch.float64, device=f.dev)
    if f.handle is not None:
        f.handle.intensity(f.d_p0.data_ptr(), f.d_depths.data_ptr(), R, out.data_ptr(), f.stream)
    else:
        z, p, d_x = f.upload_rows(rays.zs), f.upload_rows(rays.ps), f.upload_x()
        _lib.intensity_device(f.env, z.data_ptr(), p.data_ptr(), len(rays), S, d_x.data_ptr(), f.d_p0.data_ptr(),
                              f.d_depths.data_ptr(), R, out.data_ptr(), f.stream)
    I = out.cpu().numpy()
    if intensity:
        return I
    with np.errstate(divide="ignore"):
        return -10.0 * np.log10(I)


def beam_transmission_loss(rays, receiver_depths, environment, flatearth=True, device=0, intensity=False, min_width=10.0):
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
    device-resident fan is processed where it is and stays device resident."""
    w = float(min_width)
    if not (np.isfinite(w) and w > 0):
        raise ValueError("min_width must be finite and > 0")
    f = _FanFrame(rays, receiver_depths, environment, flatearth, "beam_transmission_loss").to_device(device)
    import torch

    R, S = len(f.depths), len(f.x)
    out = torch.empty((R, S), dtype=torch.float64, device=f.dev)
    d_b = torch.from_numpy(f.bottom()).to(f.dev)
    if f.handle is not None:
        f.handle.beam_intensity(f.d_p0.data_ptr(), d_b.data_ptr(), f.d_depths.data_ptr(), R, w, out.data_ptr(), f.stream)
    else:
        z, p, d_x = f.upload_rows(rays.zs), f.upload_rows(rays.ps), f.upload_x()
        _lib.beam_intensity_device(f.env, z.data_ptr(), p.data_ptr(), len(rays), S, d_x.data_ptr(), f.d_p0.data_ptr(),
                                   d_b.data_ptr(), f.d_depths.data_ptr(), R, w, out.data_ptr(), f.stream)
    I = out.cpu().numpy()
    if intensity:
        return I
    with np.errstate(divide="ignore"):
        return -10.0 * np.log10(I)


__all__ = ["transmission_loss", "beam_transmission_loss"]
