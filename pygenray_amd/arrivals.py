"""``arrivals``: the ray-tube arrivals of a fan at receiver depths ("Arrivals").

Every ray tube that ``transmission_loss`` counts at a receiver and save range is one arrival, with its travel time and
slowness interpolated across the tube.  The walk runs in HIP (csrc/pgr_arrivals.h) on the fan's trajectories where they
already are -- in HBM for a device-resident fan, uploaded through torch for a host fan.  There is no CPU path.
"""
import numpy as np

from .ray_objects import _columns
from ._fan_frame import (_FanFrame, _absorption_profile, _arrival_columns, _arrival_lags, _boundary_spec, _device_arrivals,
                         _lag_spec)


def _bilinear(x, y, x_grid, y_grid, values):
    """host_physics.bilinear_interp element-wise over arrays: the same cell rule and operations in the same order."""
    i = np.clip(np.searchsorted(x_grid, x) - 1, 0, len(x_grid) - 2)
    j = np.clip(np.searchsorted(y_grid, y) - 1, 0, len(y_grid) - 2)
    wx = (x - x_grid[i]) / (x_grid[i + 1] - x_grid[i])
    wy = (y - y_grid[j]) / (y_grid[j + 1] - y_grid[j])
    return ((1 - wx) * (1 - wy) * values[i, j] + wx * (1 - wy) * values[i + 1, j]
            + (1 - wx) * wy * values[i, j + 1] + wx * wy * values[i + 1, j + 1])


class Arrivals:
    """The arrivals of a fan at ``receiver_depths`` (R) and the requested save columns ``range_indices`` (n), host arrays.

    Arrivals are grouped by receiver j, then by requested column c (the caller's order), then by increasing tube;
    those of (j, c) are ``[offsets[j * n + c], offsets[j * n + c + 1])`` (``at(j, c)`` slices them).  Per arrival:

    - ``tube``: index k into the fan's (surviving) rays; the tube is rays k and k + 1
    - ``w``: (D_j - d_k) / (d_k+1 - d_k), where the receiver lies across the tube (0 <= w <= 1)
    - ``time``: T_k + w (T_k+1 - T_k), seconds
    - ``p``: p_k + w (p_k+1 - p_k), the slowness in ``RayFan.ps``'s sign convention
    - ``intensity``: the tube's term of ``transmission_loss(..., intensity=True)``; summed in order from 0.0 it gives that
      value at (j, c) bit for bit -- in either arithmetic, against that library's own TL (``PGR_ARITH=contracted``: the
      counts, order and this sum are exact; the values are within a derived bound of the reference build's)
    - lazily: ``launch_angle`` (degrees, ``rays.thetas``' convention, interpolated by w), ``amplitude`` = sqrt(intensity),
      ``received_angle`` = degrees(arcsin(p c(x, D_j))) with c from the tables of the frame the fan was traced in
      (``host_physics.ray_angle``'s definition; ``EigenRays.received_angles`` uses the non-flat-earth table instead).

    - ``turning_points`` (n_arrivals, 2) int64: the turning points of rays ``tube`` and ``tube + 1`` on their way to the
      arrival's column (``RayFan.turning_points``); ``ray_number`` (float): the count the two share times the sign of
      ``launch_angle`` -- the reference's numeric ray id, what tomography matches arrivals to predictions by -- and NaN
      where the two edge rays differ: a tube straddling a turning point has no one identifier.  Both are ``None`` for an
      ``Arrivals`` built without the counts.
    - lazily: ``caustics`` (int64): the caustics the arrival's tube has passed on its way to the arrival's column,
      ``caustic_index(rays, environment)[tube, column]`` -- computed on first access from the fan the arrivals were made from,
      which the ``Arrivals`` of ``arrivals()`` therefore keeps alive (a device-resident fan stays so); ``ValueError`` as
      ``caustic_index`` raises it (a fan with bounces and no bounce log), and for an ``Arrivals`` built without its fan.

    - ``bottom_phase``: the lag in cycles the arrival has collected at its bottom bounces, -arg R / 2 pi summed over them (the
      arrival adds exp(-2 pi i bottom_phase) in ``pressure_field``'s convention), when ``arrivals(..., bottom_loss=<a
      BottomReflection>)`` made the object: the edge rays' lags interpolated by ``w``, Phi_k + w (Phi_k+1 - Phi_k).  ``None``
      otherwise.

    Bounce counts are known only at a ray's end: at the fan's last column, ``rays.n_surfs[tube]`` and
    ``rays.n_botts[tube]`` apply.  The source's own column (r = 0) has no arrivals."""

    def __init__(self, offsets, receiver_depths, ranges, range_indices, tube, w, time, p, intensity, thetas, c_rx,
                 turning_points=None, *, bottom_phase=None):
        self.turning_points = turning_points
        self.bottom_phase = bottom_phase
        self.offsets = offsets
        self.receiver_depths = receiver_depths
        self.ranges = ranges
        self.range_indices = range_indices
        self.tube = tube
        self.w = w
        self.time = time
        self.p = p
        self.intensity = intensity
        self._thetas = thetas
        self._c_rx = c_rx                      # (R, n) sound speed at the receivers, in the traced frame
        self._lazy = {}
        self._source = None                    # (rays, environment, flatearth, device) of arrivals(): what `caustics` needs

    def __len__(self):
        return len(self.tube)

    def _pairs(self):
        """(receiver, column slot) of every arrival"""
        if "pairs" not in self._lazy:
            n = len(self.range_indices)
            idx = np.repeat(np.arange(len(self.offsets) - 1), np.diff(self.offsets))
            self._lazy["pairs"] = (idx // n, idx % n)
        return self._lazy["pairs"]

    @property
    def launch_angle(self):
        if "launch_angle" not in self._lazy:
            t0, t1 = self._thetas[self.tube], self._thetas[self.tube + 1]
            self._lazy["launch_angle"] = t0 + self.w * (t1 - t0)
        return self._lazy["launch_angle"]

    @property
    def amplitude(self):
        if "amplitude" not in self._lazy:
            self._lazy["amplitude"] = np.sqrt(self.intensity)
        return self._lazy["amplitude"]

    @property
    def received_angle(self):
        if "received_angle" not in self._lazy:
            j, c = self._pairs()
            with np.errstate(invalid="ignore"):
                self._lazy["received_angle"] = np.degrees(np.arcsin(self.p * self._c_rx[j, c]))
        return self._lazy["received_angle"]

    @property
    def caustics(self):
        if "caustics" not in self._lazy:
            if self._source is None:
                raise ValueError("these Arrivals were built without their fan: caustics needs arrivals(rays, ...)'s own result")
            from .coherent import caustic_index
            rays, environment, flatearth, device = self._source
            if "_dev" in rays.__dict__ and rays.__dict__["_dev"] is None and "_zs" not in rays.__dict__:
                raise ValueError("the fan of these Arrivals was released before its depths were read: caustics cannot be computed")
            kappa = caustic_index(rays, environment, flatearth=flatearth, device=device)
            self._lazy["caustics"] = kappa[self.tube, self.range_indices[self._pairs()[1]]]
        return self._lazy["caustics"]

    @property
    def ray_number(self):
        if self.turning_points is None:
            return None
        if "ray_number" not in self._lazy:
            a, b = self.turning_points[:, 0], self.turning_points[:, 1]
            self._lazy["ray_number"] = np.where(a == b, a * np.sign(self.launch_angle), np.nan)
        return self._lazy["ray_number"]

    def at(self, j, c):
        """The arrivals at receiver j and requested column slot c -> dict of arrays (views)."""
        n = len(self.range_indices)
        if not (0 <= j < len(self.receiver_depths) and 0 <= c < n):
            raise IndexError(f"(j, c) = ({j}, {c}) outside ({len(self.receiver_depths)}, {n})")
        sl = slice(int(self.offsets[j * n + c]), int(self.offsets[j * n + c + 1]))
        return dict(tube=self.tube[sl], w=self.w[sl], time=self.time[sl], p=self.p[sl], intensity=self.intensity[sl],
                    launch_angle=self.launch_angle[sl], amplitude=self.amplitude[sl],
                    received_angle=self.received_angle[sl])

    def __repr__(self):
        return (f"Arrivals({len(self)} arrivals at {len(self.receiver_depths)} receiver depths x "
                f"{len(self.range_indices)} ranges)")


def arrivals(rays, receiver_depths, environment, flatearth=True, range_indices=None, device=0, absorption=None,
             bottom_loss=None, surface_loss=None):
    """Ray-tube arrivals of ``rays`` (a ``RayFan`` from ``shoot_rays``) at ``receiver_depths`` (metres, positive down,
    strictly ascending) and the save columns ``range_indices`` (default ``[S - 1]``, the receiver range; any integers in
    -S .. S - 1) -> ``Arrivals``.

    Every tube that ``transmission_loss`` counts at a receiver is one arrival: travel time and slowness interpolated
    linearly in depth across the tube, the tube's intensity, its index into the fan.  The arguments, the frame (flat-earth,
    mirrored for a backwards fan) and the sound speed are ``transmission_loss``'s.  A device-resident fan is processed
    where it is and stays device resident.

    ``absorption``: volume absorption as in ``transmission_loss`` -- ``intensity`` (and ``amplitude``, its square root) is
    the weighted tube's term, which still adds up to the weighted ``transmission_loss`` bit for bit; the arrivals found,
    their order, times and slownesses do not change.  None (default) runs exactly the call without it; the weights take
    one trajectory array of device memory for the duration of the call.

    ``bottom_loss`` / ``surface_loss``: boundary reflection loss as in ``transmission_loss``, one more factor of the same
    weights (None and None, the default: exactly the call without them; a fan with a bounce log otherwise).  A
    ``BottomReflection`` as ``bottom_loss`` weights by its magnitude and also fills ``Arrivals.bottom_phase``.

    The ``Arrivals`` returned keeps a reference to ``rays`` and ``environment`` for its lazily computed ``caustics``: a
    device-resident fan's HBM stays allocated while the ``Arrivals`` lives, unless the fan is fetched (``to_host()``) or
    ``release()``d -- after a release without its depths read, ``caustics`` raises ``ValueError``."""
    profile = None if absorption is None else _absorption_profile(absorption)
    boundary = _boundary_spec(rays, bottom_loss, surface_loss)
    f = _FanFrame(rays, receiver_depths, environment, flatearth, "arrivals")
    S = len(f.x)
    cols = _columns(range_indices, S)
    f.to_device(device).absorb(profile, boundary)
    R, n = len(f.depths), len(cols)
    offsets, tube, w, T, P, I = _device_arrivals(f, cols)
    phase = None
    lag = _lag_spec(bottom_loss)
    if lag is not None:
        col = _arrival_columns(f, offsets, cols)
        phase = _arrival_lags(f, lag, col, tube, w).cpu().numpy() if len(tube) else np.zeros(0)
    cin, rin, zin = f.tables
    xs = f.xf[cols]
    c_rx = _bilinear(np.broadcast_to(xs[None, :], (R, n)), np.broadcast_to(f.depths[:, None], (R, n)), rin, zin, cin)
    offsets, tube = offsets.cpu().numpy(), tube.cpu().numpy()
    # the edge rays' turning points at each arrival's column: one more call on the fan where it is (NumPy on a host fan)
    turns = rays.turning_points(cols)
    slot = np.repeat(np.arange(R * n), np.diff(offsets)) % n
    turns = np.stack([turns[tube, slot], turns[tube + 1, slot]], axis=1)
    out = Arrivals(offsets, f.depths, np.asarray(f.x)[cols], cols.astype(np.int64), tube,
                   w.cpu().numpy(), T.cpu().numpy(), P.cpu().numpy(), I.cpu().numpy(), np.asarray(rays.thetas, dtype=float),
                   c_rx, turns, bottom_phase=phase)
    out._source = (rays, environment, flatearth, device)
    return out


__all__ = ["arrivals", "Arrivals"]
