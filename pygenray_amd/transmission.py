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
from .reflection import BottomReflection

_NO_FE_MSG = ("Flat earth transformation has not been applied. Set `flat_earth_transform=True` "
              "when creating the OceanEnvironment2D object.")


def _check_flatearth(environment, flatearth):
    if flatearth and not hasattr(environment, "sound_speed_fe"):
        raise ValueError(_NO_FE_MSG)


def _save_grid(rays):
    """the fan's one save grid x (S,), refused when the rows of rays.rs differ"""
    r = rays.__dict__.get("_r")
    if r is not None and rays.__dict__.get("_rs") is None:
        return np.asarray(r, dtype=float)          # (a device fan: one save grid by construction)
    rs = np.asarray(rays.rs, dtype=float)
    x = rs[0]
    if not np.array_equal(rs, np.broadcast_to(x, rs.shape)):
        raise ValueError("the rows of rays.rs differ: the fan must share one save grid")
    return x


def _absorption_profile(absorption):
    """``absorption`` -> (depth nodes or None, alpha in dB per METRE), as the path kernels take them: a scalar in dB/km (a
    constant profile), or a pair ``(depths_m, dB_per_km)`` of equal-length 1-D sequences, the depths strictly ascending.
    dB/km -> dB/m is ``value / 1000.0``.  Everything that can be refused without a GPU is refused here."""
    if isinstance(absorption, (tuple, list)) and len(absorption) == 2 and np.ndim(absorption[0]) == 1:
        d, a = (np.asarray(v, dtype=float) for v in absorption)
        if a.ndim != 1 or len(a) != len(d) or len(d) == 0:
            raise ValueError("absorption = (depths_m, dB_per_km) needs two 1-D sequences of equal, non-zero length")
        if not np.all(np.isfinite(d)) or not np.all(np.diff(d) > 0):
            raise ValueError("absorption depths must be finite and strictly ascending")
    else:
        d, a = None, np.asarray(absorption, dtype=float)
        if a.ndim != 0:
            raise ValueError("absorption must be a scalar in dB/km or a pair (depths_m, dB_per_km)")
        a = a.reshape(1)
    if not np.all(np.isfinite(a)) or np.any(a < 0):
        raise ValueError("absorption must be finite and >= 0 dB/km")
    return (None if d is None else np.ascontiguousarray(d)), np.ascontiguousarray(a / 1000.0)


def _loss_table(loss, name):
    """A boundary loss as the public functions take it -> (grazing-angle nodes in degrees or None, dB per bounce): None (no
    loss: 0.0 dB), a scalar in dB per bounce, or a pair ``(grazing_deg, dB)`` of equal-length 1-D sequences, the angles
    strictly ascending (linear between the nodes, held at the end values outside them).  Everything that can be refused
    without a GPU is refused here.  A ``BottomReflection`` (the bottom only) stands for its ``.loss`` pair."""
    if isinstance(loss, BottomReflection):
        if name != "bottom_loss":
            raise ValueError(f"{name}: a BottomReflection describes the bottom; pass it as bottom_loss")
        loss = loss.loss
    if loss is None:
        return None, np.zeros(1)
    if isinstance(loss, (tuple, list)) and len(loss) == 2 and np.ndim(loss[0]) == 1:
        g, v = (np.asarray(a, dtype=float) for a in loss)
        if v.ndim != 1 or len(v) != len(g) or len(g) == 0:
            raise ValueError(f"{name} = (grazing_deg, dB) needs two 1-D sequences of equal, non-zero length")
        if not np.all(np.isfinite(g)) or not np.all(np.diff(g) > 0):
            raise ValueError(f"{name}: the grazing angles must be finite and strictly ascending")
    else:
        g, v = None, np.asarray(loss, dtype=float)
        if v.ndim != 0:
            raise ValueError(f"{name} must be a scalar in dB per bounce or a pair (grazing_deg, dB)")
        v = v.reshape(1)
    if not np.all(np.isfinite(v)) or np.any(v < 0):
        raise ValueError(f"{name} must be finite and >= 0 dB")
    if g is not None and len(g) == 1:
        g = None
    return (None if g is None else np.ascontiguousarray(g)), np.ascontiguousarray(v)


def _boundary_spec(rays, bottom_loss, surface_loss):
    """None when neither loss is given (the calls without them), else the two tables; a fan without a bounce log is refused"""
    if bottom_loss is None and surface_loss is None:
        return None
    spec = (_loss_table(bottom_loss, "bottom_loss"), _loss_table(surface_loss, "surface_loss"))
    if not rays._has_bounce_log():
        raise ValueError("boundary loss needs a fan traced with a bounce log: shoot_rays(..., max_bounces=K)")
    return spec


def _lag_spec(bottom_loss):
    """None for every ``bottom_loss`` but a ``BottomReflection``; for one, the tables the boundary post-pass accumulates the
    bottom's lag in cycles from: its ``.lag`` pair in the bottom's slot (one node: a constant) and 0.0 for the surface"""
    if not isinstance(bottom_loss, BottomReflection):
        return None
    g, v = bottom_loss.lag
    return ((None if len(g) == 1 else np.ascontiguousarray(g)), np.ascontiguousarray(v)), (None, np.zeros(1))


def _ptr(t):
    """a device tensor's address, 0 for None"""
    return 0 if t is None else t.data_ptr()


class _TracedFan:
    """A fan (host or device resident) on its save ranges x, and -- after ``to_device`` -- the frame it was traced in: xf
    (mirrored for a backwards fan), the EnvHandle and its tables (cin, rin, zin), the torch stream and the fan's device
    handle (None for a host fan).  ``_host_fan`` uploads a host fan's arrays once.  Shared by the products that read a
    fan's trajectories: the tube products (_FanFrame) and the travel-time kernel (sensitivity.py)."""

    def __init__(self, rays, x, environment, flatearth):
        self.rays, self.x, self.environment, self.flatearth = rays, x, environment, flatearth

    def to_device(self, device):
        import torch

        x = self.x
        self.backwards = len(x) > 1 and x[-1] < x[0]
        self.xf = -x if self.backwards else x            # the frame the fan was traced in
        self.env, self.tables = _device_env(self.environment, self.flatearth, self.backwards, device)
        self.dev = torch.device("cuda", self.env.device)
        self.stream = torch.cuda.current_stream(self.dev).cuda_stream
        self.handle = self.rays.__dict__.get("_dev")
        if self.handle is not None and self.handle._env is not self.env:
            raise ValueError("the fan was traced in another environment (or flatearth setting) than the one given")
        self._host = {}
        return self

    def upload(self, a):
        import torch
        return torch.from_numpy(np.ascontiguousarray(a, dtype=float)).to(self.dev)

    def _host_fan(self, name):
        """A host fan's array `name` on the device, uploaded once per frame: the (M, S) arrays as the (S, M) rows the kernels
        read (the transposed view shoot_rays hands out is that layout already), xf as it is."""
        if name not in self._host:
            a = self.xf if name == "xf" else np.asarray(getattr(self.rays, name), dtype=float).T
            self._host[name] = self.upload(a)
        return self._host[name].data_ptr()

    def path_integral(self, a_depths, alpha):
        """The running path integral A (S, M) of the fan's rays, a float64 device tensor (csrc/pgr_path.h): alpha in dB/m on
        the depth nodes a_depths (None with one alpha).  A device-resident fan is read where it is; a host fan's ts and zs
        are uploaded (once per frame)."""
        import torch
        S, M = len(self.x), len(self.rays)
        out = torch.empty((S, M), dtype=torch.float64, device=self.dev)
        if self.handle is not None:
            self.handle.path_integral(a_depths, alpha, out.data_ptr(), self.stream)
        else:
            _lib.path_integral_device(self.env, self._host_fan("ts"), self._host_fan("zs"), M, S, self._host_fan("xf"),
                                      a_depths, alpha, out.data_ptr(), self.stream)
        return out

    def bottom_slope(self):
        """(depth_ranges, bottom_angles in degrees) of the frame the fan was traced in (mirrored for a backwards fan)"""
        cin, cpin, rin, _, depths, depth_ranges, angles = _unpack_envi(self.environment, flatearth=self.flatearth)
        if self.backwards:
            depths, depth_ranges, angles = _mirror_envi_arrays(cin, cpin, rin, depths, depth_ranges, angles)[3:6]
        return np.ascontiguousarray(depth_ranges, dtype=float), np.ascontiguousarray(angles, dtype=float)

    def boundary_loss(self, spec, counts=False):
        """The boundary loss B (S, M) in dB every ray has collected up to every save range, a float64 device tensor
        (csrc/pgr_bounce.h), from the fan's bounce log and the tables `spec` of _boundary_spec; with `counts` also the
        bottom and surface bounce counts (S, M) int32.  A device-resident fan's log is read where it is; a host fan's is
        uploaded."""
        import torch
        S, M = len(self.x), len(self.rays)
        out = torch.empty((S, M), dtype=torch.float64, device=self.dev)
        nb, ns = ((torch.empty((S, M), dtype=torch.int32, device=self.dev) for _ in range(2)) if counts else (None, None))
        tables = _lib.boundary_tables(spec[0], spec[1], self.bottom_slope())
        ptr = _ptr
        if self.handle is not None:
            self.handle.boundary_loss(tables, out.data_ptr(), ptr(nb), ptr(ns), self.stream)
        else:
            log = self.rays.bounces
            bx, bp = self.upload(log.x.T), self.upload(log.p.T)
            bk = torch.from_numpy(np.ascontiguousarray(log.kind.T)).to(self.dev)
            _lib.boundary_loss_device(self.env, bx.data_ptr(), bp.data_ptr(), bk.data_ptr(), M, log.capacity,
                                      float(self.xf[0]), float(self.xf[-1]), S, tables, out.data_ptr(), ptr(nb), ptr(ns),
                                      self.stream)
            torch.cuda.current_stream(self.dev).synchronize()      # (the uploads are freed when this returns)
        return (out, nb, ns) if counts else out


class _FanFrame(_TracedFan):
    """A fan checked for the tube kernels (`who` names the caller in errors): the receiver depths, the save ranges x and the
    source depth -- everything that can be refused without a GPU.  ``to_device`` then sets up _TracedFan's frame, the launch
    slowness p0 and the device copies of p0 and the depths, and ``run`` calls a tube entry there."""

    def __init__(self, rays, receiver_depths, environment, flatearth, who):
        d = np.asarray(receiver_depths, dtype=float)
        if d.ndim != 1 or len(d) == 0:
            raise ValueError("receiver_depths must be a non-empty 1-D sequence")
        if not np.all(np.isfinite(d)):
            raise ValueError("receiver_depths must be finite")
        if not np.all(np.diff(d) > 0):
            raise ValueError("receiver_depths must be strictly ascending")
        _check_flatearth(environment, flatearth)
        if len(rays) < 2:
            raise ValueError(f"{who} needs a fan of at least 2 rays (one ray tube)")
        sd = np.asarray(rays.source_depths, dtype=float)
        if not np.all(sd == sd[0]):
            raise ValueError("the fan mixes source depths: ray tubes need one source")
        super().__init__(rays, _save_grid(rays), environment, flatearth)
        self.depths, self.source_depth = np.ascontiguousarray(d), float(sd[0])

    def to_device(self, device):
        super().to_device(device)
        cin, rin, zin = self.tables
        c_source = bilinear_interp(self.xf[0], self.source_depth, rin, zin, cin)
        self.p0 = _initial_slowness(self.rays.thetas, c_source)
        self.d_p0 = self.upload(self.p0)
        self.d_depths = self.upload(self.depths)
        self.d_W = None
        return self

    def absorb(self, profile, boundary=None, counts=False):
        """Volume absorption and boundary loss for the entries ``run`` calls from here on: the path integral A of the
        profile (from _absorption_profile) and the boundary loss B of the tables (from _boundary_spec) run once each and
        their sum A + B (either alone when the other is None) becomes, in place, the weights W = 10^(-(A + B) / 10) of g, one
        trajectory array in size, freed with this frame.  Both None: no weights, the unweighted entries.  `counts`: the same
        run of the boundary loss (with zero-loss tables when `boundary` is None, its B then unused) also leaves the
        per-sample bounce counts nb, ns (S, M) int32 in ``self.d_counts``."""
        A = None if profile is None else self.path_integral(*profile)
        self.d_counts = None
        if boundary is not None or counts:
            spec = boundary if boundary is not None else (_loss_table(None, "bottom_loss"), _loss_table(None, "surface_loss"))
            B = self.boundary_loss(spec, counts=counts)
            if counts:
                B, *self.d_counts = B
            if boundary is not None:
                A = B if A is None else A.add_(B)
        if A is not None:
            _lib.absorption_weights_device(self.env.device, A.data_ptr(), A.numel(), A.data_ptr(), self.stream)
            self.d_W = A
        return self

    def run(self, entry, *args):
        """Tube entry `entry` on the fan, with p0, the arguments after it and the stream: ``FanHandle.<entry>`` on a
        device-resident fan, else ``_lib.<entry>_device`` on the host fan's trajectories (ts only for ``arrivals`` and
        ``pressure`` / ``pressure_phi`` / ``beam_pressure`` / ``beam_arrival_counts`` / ``beam_arrivals``)."""
        args = (self.d_p0.data_ptr(),) + args + (self.stream,)
        # (the arrival counts have no weighted twin: finite weights leave the tubes counted as they are)
        kw = {"weights": self.d_W.data_ptr()} if self.d_W is not None and entry != "arrival_counts" else {}
        if self.handle is not None:
            return getattr(self.handle, entry)(*args, **kw)
        fan = [self._host_fan(k) for k in (("ts", "zs", "ps") if entry in ("arrivals", "pressure", "pressure_phi", "beam_pressure", "beam_arrival_counts", "beam_arrivals") else ("zs", "ps"))]
        getattr(_lib, entry + "_device")(self.env, *fan, len(self.rays), len(self.x), self._host_fan("xf"), *args, **kw)

    def image(self):
        """an empty (R, S) float64 device array: an intensity image's output"""
        import torch
        return torch.empty((len(self.depths), len(self.x)), dtype=torch.float64, device=self.dev)

    def bottom(self):
        """The bottom depth at each save range in the frame the fan was traced in (flat-earth, mirrored for a backwards fan):
        host_physics.linear_interp of the bathymetry at xf."""
        cin, cpin, rin, _, depths, depth_ranges, angles = _unpack_envi(self.environment, flatearth=self.flatearth)
        if self.backwards:
            depths, depth_ranges = _mirror_envi_arrays(cin, cpin, rin, depths, depth_ranges, angles)[3:5]
        return np.array([linear_interp(float(v), depth_ranges, depths) for v in self.xf])


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
    w = float(min_width)
    if not (np.isfinite(w) and w > 0):
        raise ValueError("min_width must be finite and > 0")
    profile = None if absorption is None else _absorption_profile(absorption)
    boundary = _boundary_spec(rays, bottom_loss, surface_loss)
    f = _FanFrame(rays, receiver_depths, environment, flatearth, "beam_transmission_loss").to_device(device).absorb(profile, boundary)
    out, d_b = f.image(), f.upload(f.bottom())
    f.run("beam_intensity", d_b.data_ptr(), f.d_depths.data_ptr(), len(f.depths), w, out.data_ptr())
    return _db(out, intensity)


__all__ = ["transmission_loss", "beam_transmission_loss"]
