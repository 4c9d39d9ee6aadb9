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


__all__ = ["transmission_loss"]
