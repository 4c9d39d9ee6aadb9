"""Travel-time sensitivity kernels of a fan on a range-depth grid: ``travel_time_kernel``, the linear map dT = K . dc from a
sound-speed perturbation on the grid to the rays' travel times ("Travel-time sensitivity kernels").

No reference counterpart: pygenray gives back rays and travel times, and the only other way to K is one re-shot fan per
model node.  The kernel runs in HIP (csrc/pgr_sens.h) on the fan's trajectories where they already are -- in HBM for a
device-resident fan, uploaded through torch for a host fan.  There is no CPU path.
"""
import numbers

import numpy as np

from . import _lib
from .environment import _unpack_envi
from .ray_objects import EigenRays, RayFan
from ._fan_frame import _TracedFan, _check_flatearth, _save_grid


def _grid(v, name, most):
    """a kernel grid axis checked; ``most`` the entry's limit (include/pgr.h), checked before the values are read"""
    if hasattr(v, "__len__") and len(v) > most:
        raise ValueError(f"{name} has {len(v)} values, more than the {most} supported")
    g = np.asarray(v, dtype=float)
    if g.ndim != 1 or len(g) < 2:
        raise ValueError(f"{name} must be a 1-D sequence of at least 2 values")
    if not np.all(np.isfinite(g)):
        raise ValueError(f"{name} must be finite")
    if not np.all(np.diff(g) > 0):
        raise ValueError(f"{name} must be strictly ascending")
    return np.ascontiguousarray(g)


class _KernelJob(_TracedFan):
    """One fan checked for the kernel: its save grid and the column its paths end at (everything that can be refused
    without a GPU); ``run`` computes K on the device."""

    def __init__(self, rays, environment, flatearth, range_index):
        super().__init__(rays, _save_grid(rays) if len(rays) else np.zeros(0), environment, flatearth)
        S = len(self.x)
        if len(rays) and not -S <= range_index < S:
            raise ValueError(f"range_index {range_index} is out of range for a fan of {S} save ranges")
        self.col = range_index % S if len(rays) else 0

    def run(self, ranges, depths, device):
        """K (M, A, B) as a device tensor, the range axis in the user's order"""
        import torch

        M, A, B = len(self.rays), len(ranges), len(depths)
        if M == 0:
            return torch.zeros((0, A, B), dtype=torch.float64, device=torch.device("cuda", device))
        self.to_device(device)
        g = -ranges[::-1] if self.backwards else ranges          # the traced frame's grid, ascending
        d_g, d_h = self.upload(g), self.upload(depths)
        out = torch.empty((M, A, B), dtype=torch.float64, device=self.dev)
        args = (d_g.data_ptr(), A, d_h.data_ptr(), B, self.col, out.data_ptr(), self.stream)
        if self.handle is not None:
            self.handle.travel_time_kernel(*args)
        else:
            _lib.travel_time_kernel_device(self.env, self._host_fan("ts"), self._host_fan("zs"), M, len(self.x),
                                           self._host_fan("xf"), *args)
        return torch.flip(out, [1]) if self.backwards else out


def travel_time_kernel(rays, environment, ranges=None, depths=None, flatearth=True, range_index=-1, device=0,
                       as_tensor=False, max_bytes=4 << 30):
    """The travel-time sensitivity kernel of ``rays`` on a range-depth grid -> K, shape ``(M, len(ranges), len(depths))`` in
    s / (m/s): ``δT_m = Σ_ab K[m, a, b] δc_ab`` to first order (Fermat, δT = -∫ δc / c² ds along ray m), for the travel time
    at save column ``range_index`` and a perturbation ``δc(x, d) = Σ_ab δc_ab φ_ab(x, d)``, φ_ab the bilinear weight of
    node (a, b) that ``host_physics.bilinear_interp`` gives (clamped cell, unclamped weights: outside the grid it
    extrapolates as the fan's look-up does).

    ``rays``: a ``RayFan`` (host or device resident; a device fan is processed where it is and stays resident), or an
    ``EigenRays``, which gives a dict keyed by receiver-depth index of ``(M_j, A, B)`` kernels.  One ray is enough, and
    source depths may differ.  ``ranges`` / ``depths`` (metres, strictly ascending, at least 2 each): the grid in the
    user's coordinates (a backwards fan's is mirrored internally; the result's axes are always in the order given);
    default the table of the environment the fan was traced in (``environment`` with ``flatearth``), on which
    ``K · cin = -(T(range_index) - T(0))`` to rounding.  Each ray's path is the polyline through its samples, each chord cut
    at the grid lines and integrated by Simpson's rule in the chord's own travel time.  A ray with a NaN sample
    up to ``range_index`` gives a NaN row; ``range_index`` 0 gives zeros.

    With ``flatearth=True`` K is the derivative with respect to the flat-earth table ``sound_speed_fe``, whose node (a, b)
    is node (a, b) of ``sound_speed`` times ``F_b = 1 + E_b (1 + E_b)``, ``E_b = z_b / R_e(lat)`` (``environment.eflat``):
    on the default grid the derivative with respect to the true sound speed is ``K * F`` (F broadcast over depth).

    A float64 NumPy array, or with ``as_tensor=True`` the ``torch`` tensor on ``device``.  A ``ValueError`` before any GPU
    work for a result larger than ``max_bytes``, or for more than 65535 ranges or 2^30 depths."""
    _check_flatearth(environment, flatearth)
    if isinstance(range_index, (bool, np.bool_)) or not isinstance(range_index, numbers.Integral):
        raise ValueError(f"range_index must be an integer, not {range_index!r}")
    range_index = int(range_index)
    if isinstance(rays, EigenRays):
        keys = list(rays.ts.keys())
        fans = {}
        for k in keys:
            n = len(rays.launch_angles[k])
            a = [np.asarray(getattr(rays, name)[k], dtype=float).reshape(n, -1) if n else np.zeros((0, 0))
                 for name in ("rs", "ts", "zs", "ps")]
            fans[k] = RayFan.from_arrays(np.asarray(rays.launch_angles[k]), *a, rays.n_botts[k], rays.n_surfs[k],
                                         -a[2][:, 0] if n else np.zeros(0))
    elif isinstance(rays, RayFan):
        keys, fans = None, {None: rays}
    else:
        raise ValueError(f"rays must be a RayFan or EigenRays, not {type(rays).__name__}")
    jobs = {k: _KernelJob(f, environment, flatearth, range_index) for k, f in fans.items()}
    if ranges is None or depths is None:
        _, _, rin, zin = _unpack_envi(environment, flatearth=flatearth)[:4]
    g = _grid(rin if ranges is None else ranges, "ranges", 65535)     # (a range node is a launch's gridDim.y)
    h = _grid(zin if depths is None else depths, "depths", 1 << 30)
    M = sum(len(f) for f in fans.values())
    size = M * len(g) * len(h) * 8
    if size > max_bytes:
        raise ValueError(f"the kernel of {M} rays on a {len(g)} x {len(h)} grid needs {size} bytes, more than max_bytes = "
                         f"{max_bytes}")
    out = {}
    for k, job in jobs.items():
        K = job.run(g, h, device)
        out[k] = K if as_tensor else K.cpu().numpy()
    return out if keys is not None else out[None]


__all__ = ["travel_time_kernel"]
