"""``transmission_loss``: incoherent ray-tube transmission loss of a fan on a range-depth grid ("Transmission loss").

No reference counterpart: pygenray gives back rays, not amplitudes.  The tube sum runs in HIP (csrc/pgr_tl.h) on the fan's
trajectories where they already are -- in HBM for a device-resident fan, uploaded through torch for a host fan.  There is
no CPU path.
"""
import numpy as np

from . import _lib
from .host_physics import bilinear_interp
from .launch_rays import _device_env, _initial_slowness

_NO_FE_MSG = ("Flat earth transformation has not been applied. Set `flat_earth_transform=True` "
              "when creating the OceanEnvironment2D object.")


def _check_arguments(rays, receiver_depths, environment, flatearth):
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
        raise ValueError("transmission_loss needs a fan of at least 2 rays (one ray tube)")
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
    depths, x, source_depth = _check_arguments(rays, receiver_depths, environment, flatearth)
    import torch

    backwards = len(x) > 1 and x[-1] < x[0]
    xf = -x if backwards else x                  # the frame the fan was traced in
    env, (cin, rin, zin) = _device_env(environment, flatearth, backwards, device)
    c_source = bilinear_interp(xf[0], source_depth, rin, zin, cin)
    p0 = _initial_slowness(rays.thetas, c_source)
    dev = torch.device("cuda", env.device)
    f64 = dict(dtype=torch.float64, device=dev)
    R, S = len(depths), len(x)
    d_p0 = torch.from_numpy(np.ascontiguousarray(p0)).to(dev)
    d_depths = torch.from_numpy(depths).to(dev)
    out = torch.empty((R, S), **f64)
    stream = torch.cuda.current_stream(dev).cuda_stream
    handle = rays.__dict__.get("_dev")
    if handle is not None:
        if handle._env is not env:
            raise ValueError("the fan was traced in another environment (or flatearth setting) than the one given")
        handle.intensity(d_p0.data_ptr(), d_depths.data_ptr(), R, out.data_ptr(), stream)
    else:
        # (S, M) rows, stored sign convention: the transposed view shoot_rays hands out is that layout already
        z = torch.from_numpy(np.ascontiguousarray(np.asarray(rays.zs, dtype=float).T)).to(dev)
        p = torch.from_numpy(np.ascontiguousarray(np.asarray(rays.ps, dtype=float).T)).to(dev)
        d_x = torch.from_numpy(np.ascontiguousarray(xf)).to(dev)
        _lib.intensity_device(env, z.data_ptr(), p.data_ptr(), len(rays), S, d_x.data_ptr(), d_p0.data_ptr(),
                              d_depths.data_ptr(), R, out.data_ptr(), stream)
    I = out.cpu().numpy()
    if intensity:
        return I
    with np.errstate(divide="ignore"):
        return -10.0 * np.log10(I)


__all__ = ["transmission_loss"]
