"""The layer the fan products share: the traced fan and the frame of the tube kernels (``_TracedFan``, ``_FanFrame``), the
argument checks and prologues of the public product functions, and what the sums over a fan's arrivals take, left on the
device.  A product module states its product; what two of them need is here, not in either."""
import inspect
import math

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


def _entry_takes(entry):
    """What the buffer entry ``_lib.<entry>_device`` takes of a host fan, read off its own parameters -> (the rows among
    "ts", "zs", "ps" it reads, whether it takes weights).  No GPU, no library."""
    params = inspect.signature(getattr(_lib, entry + "_device")).parameters
    return tuple(k for k, p in (("ts", "t_ptr"), ("zs", "z_ptr"), ("ps", "p_ptr")) if p in params), "weights" in params


class _TracedFan:
    """A fan (host or device resident) on its save ranges x, and -- after ``to_device`` -- the frame it was traced in: xf
    (mirrored for a backwards fan), the EnvHandle and its tables (cin, rin, zin), the torch stream and the fan's device
    handle (None for a host fan).  ``_host_fan`` uploads a host fan's arrays once.  Shared by the products that read a
    fan's trajectories: the tube products (_FanFrame) and the travel-time kernel (sensitivity.py)."""

    def __init__(self, rays, x, environment, flatearth):
        self.rays, self.x, self.environment, self.flatearth = rays, x, environment, flatearth

    def to_device(self, device):
        x = self.x
        self.backwards = len(x) > 1 and x[-1] < x[0]
        self.xf = -x if self.backwards else x            # the frame the fan was traced in
        self.env, self.tables = _device_env(self.environment, self.flatearth, self.backwards, device)
        self.on_device(self.env.device)
        if self.handle is not None and self.handle._env is not self.env:
            raise ValueError("the fan was traced in another environment (or flatearth setting) than the one given")
        return self

    def on_device(self, index):
        """The part of ``to_device`` that needs no environment: the torch device `index` and its current stream, the fan's
        device handle and the uploads of a host fan (what ``_kappa`` reads)."""
        import torch
        self.dev = torch.device("cuda", index)
        self.stream = torch.cuda.current_stream(self.dev).cuda_stream
        self.handle = self.rays.__dict__.get("_dev")
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

    def bathymetry(self):
        """(depths, depth_ranges, bottom_angles in degrees) of the frame the fan was traced in (flat-earth, mirrored for a
        backwards fan)"""
        cin, cpin, rin, _, depths, depth_ranges, angles = _unpack_envi(self.environment, flatearth=self.flatearth)
        if self.backwards:
            depths, depth_ranges, angles = _mirror_envi_arrays(cin, cpin, rin, depths, depth_ranges, angles)[3:6]
        return depths, depth_ranges, angles

    def bottom_slope(self):
        """(depth_ranges, bottom_angles in degrees) of ``bathymetry``"""
        _, depth_ranges, angles = self.bathymetry()
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
        device-resident fan, else ``_lib.<entry>_device`` on the rows of the host fan's trajectories that entry reads; the
        weights of ``absorb`` go to the entries that take any (``_entry_takes``)."""
        args = (self.d_p0.data_ptr(),) + args + (self.stream,)
        rows, weighted = _entry_takes(entry)
        # (the arrival counts have no weighted twin: finite weights leave the tubes counted as they are)
        kw = {"weights": self.d_W.data_ptr()} if self.d_W is not None and weighted else {}
        if self.handle is not None:
            return getattr(self.handle, entry)(*args, **kw)
        getattr(_lib, entry + "_device")(self.env, *(self._host_fan(k) for k in rows), len(self.rays), len(self.x),
                                         self._host_fan("xf"), *args, **kw)

    def image(self):
        """an empty (R, S) float64 device array: an intensity image's output"""
        import torch
        return torch.empty((len(self.depths), len(self.x)), dtype=torch.float64, device=self.dev)

    def bottom(self):
        """The bottom depth at each save range in the frame the fan was traced in (flat-earth, mirrored for a backwards fan):
        host_physics.linear_interp of the bathymetry at xf."""
        depths, depth_ranges, _ = self.bathymetry()
        return np.array([linear_interp(float(v), depth_ranges, depths) for v in self.xf])


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
    """kappa [S][M] int32 on the device of the traced fan `f` (a _TracedFan after to_device or on_device) from the per-sample
    bounce counts nb, ns [S][M] int32 on that device (None, None: a fan without bounces)"""
    import torch
    S, M = len(f.x), len(f.rays)
    kappa = torch.empty((S, M), dtype=torch.int32, device=f.dev)
    if f.handle is not None:
        f.handle.caustic_index(_ptr(nb), _ptr(ns), kappa.data_ptr(), f.stream)
    else:
        _lib.caustic_index_device(f.dev.index, f._host_fan("zs"), M, S, _ptr(nb), _ptr(ns), kappa.data_ptr(), f.stream)
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


def _device_arrivals(f, cols):
    """The arrivals of the frame `f` (a _FanFrame after to_device and absorb) at its receiver depths and the save columns
    `cols`, left on the device -> (offsets int64 [R * n + 1], tube int32, w, T, p, I float64 [n_arrivals]): the count, the scan
    and the emit entries, in ``Arrivals``' order."""
    import torch
    R, n = len(f.depths), len(cols)
    counts = torch.empty(R * n, dtype=torch.int64, device=f.dev)
    f.run("arrival_counts", f.d_depths.data_ptr(), R, cols, counts.data_ptr())
    offsets = torch.zeros(R * n + 1, dtype=torch.int64, device=f.dev)
    torch.cumsum(counts, 0, out=offsets[1:])
    total = int(offsets[-1].item())
    tube = torch.empty(total, dtype=torch.int32, device=f.dev)
    w, T, P, I = (torch.empty(total, dtype=torch.float64, device=f.dev) for _ in range(4))
    if total:
        f.run("arrivals", f.d_depths.data_ptr(), R, cols, offsets.data_ptr(), total, tube.data_ptr(), w.data_ptr(),
              T.data_ptr(), P.data_ptr(), I.data_ptr())
    return offsets, tube, w, T, P, I


def _inv_sigma(bandwidth):
    """1 / sigma of ``pulse_sigma``, formed without the detour over inf: pi B / sqrt(ln 2), 0.0 for B = 0"""
    B = float(bandwidth)
    if not (math.isfinite(B) and B >= 0):
        raise ValueError("bandwidth must be finite and >= 0 Hz")
    return math.pi * B / math.sqrt(math.log(2.0))


def _frequency(frequency):
    f0 = float(frequency)
    if not (np.isfinite(f0) and f0 >= 0):
        raise ValueError("frequency must be finite and >= 0 Hz")
    return f0


def _min_width(min_width):
    w = float(min_width)
    if not (np.isfinite(w) and w > 0):
        raise ValueError("min_width must be finite and > 0")
    return w


def _pulse(frequency, bandwidth, dt, n_times):
    """The pulse arguments of the received signals, checked in this order -> (f0, 1 / sigma, dt, n_times)"""
    f0 = _frequency(frequency)
    rs = _inv_sigma(bandwidth)
    step = float(dt)
    if not (np.isfinite(step) and step > 0):
        raise ValueError("dt must be finite and > 0 seconds")
    if isinstance(n_times, (bool, float)) or int(n_times) != n_times or int(n_times) < 1:
        raise ValueError("n_times must be an integer >= 1")
    nt = int(n_times)
    if nt > 65535 * 256:
        raise ValueError(f"n_times must be <= {65535 * 256}")
    return f0, rs, step, nt


def _band(frequencies):
    """The ``frequencies`` of the transfer functions, checked -> contiguous float64 (F,)"""
    freq = np.asarray(frequencies, dtype=float)
    if freq.ndim != 1 or len(freq) == 0:
        raise ValueError("frequencies must be a non-empty 1-D sequence")
    freq = np.ascontiguousarray(freq)
    if not np.all(np.isfinite(freq)) or np.any(freq < 0):
        raise ValueError("frequencies must be finite and >= 0 Hz")
    if len(freq) > 65535 * 256:
        raise ValueError(f"at most {65535 * 256} frequencies per call")
    return freq


def _coherent_frame(rays, receiver_depths, env, absorption, bottom_loss, surface_loss, flatearth, who, beams=False):
    """What a coherent product refuses without a GPU after its own arguments, in this order -> (frame, profile, boundary,
    counts): the weights' tables (``absorption`` None, a scalar or a pair: a callable is the caller's), the _FanFrame named
    `who`, whether the phase index needs the bounce counts.  `beams`: the beam products refuse a ``BottomReflection`` first."""
    if beams and isinstance(bottom_loss, BottomReflection):
        raise ValueError("beam_pressure_field does not yet apply a complex bottom phase: a BottomReflection as bottom_loss is "
                         "refused (its magnitude alone would be wrong physics); pass bottom_loss=reflection.loss for the "
                         "loss without the phase")
    profile = None if absorption is None else _absorption_profile(absorption)
    boundary = _boundary_spec(rays, bottom_loss, surface_loss)
    f = _FanFrame(rays, receiver_depths, env, flatearth, who)
    return f, profile, boundary, _needs_counts(rays)


def _per_column(value, n, name, what):
    """``value``, a scalar or one value per requested column -> float array (n,), finite (``name`` and ``what`` word the
    errors)"""
    v = np.asarray(value, dtype=float)
    if v.ndim == 0:
        v = np.full(n, float(v))
    if v.shape != (n,):
        raise ValueError(f"{name} must be a scalar or one {what} per requested column ({n})")
    if not np.all(np.isfinite(v)):
        raise ValueError(f"{name} must be finite")
    return v


def _check_fits(f, R, n, m, product, entries, kind="complex"):
    """``ValueError`` when re and im, (R, n, m) float64 each -- with `kind` "real" one such array -- do not fit in the free
    memory of the frame's device"""
    import torch
    # re and im on the device; the host copy is made of them one after the other
    need = (16 if kind == "complex" else 8) * R * n * m
    free = torch.cuda.mem_get_info(f.dev)[0]
    if need > free:
        raise ValueError(f"the {product} needs {need} bytes of device memory ({R} x {n} x {m} {kind} {entries}) and {free} "
                         f"are free: ask for fewer depths, columns or {entries} per call")


def _one_zero(dev, dtype=None):
    """One zero (float64, or `dtype`) on `dev`: what stands for an array of the arrivals when there are none -- the entries
    that sum over arrivals refuse null pointers."""
    import torch
    return torch.zeros(1, dtype=dtype or torch.float64, device=dev)


def _arrival_columns(f, offsets, cols):
    """The save column of every arrival, int64 on the device of the frame `f`: arrivals come in groups (receiver j, slot c of
    `cols`) of the sizes `offsets` [R * n + 1] bounds, and a group's column is cols[c]."""
    import torch
    G, n = len(f.depths) * len(cols), len(cols)
    group = torch.repeat_interleave(torch.arange(G, device=f.dev), offsets[1:] - offsets[:-1])
    return torch.from_numpy(cols.astype(np.int64)).to(f.dev)[group % n]


def _arrival_lengths(f, col, tube, w):
    """L_a of every arrival, on the device: the path length of the tube's two edge rays at the arrival's column, interpolated
    by the arrival's w in three separate operations, L_k + w (L_k+1 - L_k)"""
    L = f.path_integral(None, np.ones(1))                             # (S, M): the path length, alpha = 1
    k = tube.long()
    L0, L1 = L[col, k], L[col, k + 1]
    d = L1 - L0
    d = w * d
    return L0 + d


def _arrival_lags(f, lag, col, tube, w):
    """phi_a of every arrival, on the device: the lag in cycles of the tube's two edge rays at the arrival's column -- the
    boundary post-pass on the tables `lag` of _lag_spec -- interpolated by the arrival's w in three separate operations,
    Phi_k + w (Phi_k+1 - Phi_k), as pgr_coh_sum_phi forms it"""
    Phi = f.boundary_loss(lag)                                        # (S, M)
    k = tube.long()
    P0, P1 = Phi[col, k], Phi[col, k + 1]
    d = P1 - P0
    d = w * d
    return P0 + d


def _arrival_terms(f, cols, profile, boundary, counts, lag=None):
    """What the sums over a fan's arrivals take, left on the device of the frame `f` (a _FanFrame after to_device): the
    weights of `profile` / `boundary`, the tubes' phase index and the arrivals at the save columns `cols` -> (offsets int64
    [R * n + 1], tube int32, w, T, I float64, q int32, column int64), per arrival from `tube` on: q and column are the phase
    index and the save column of the arrival's tube and group.  Without arrivals T, I and q hold one zero each (the entries
    refuse null pointers).  With `lag` (the tables of _lag_spec) one more element follows: phi float64, every arrival's
    bottom lag in cycles (one zero without arrivals)."""
    import torch
    f.absorb(profile, boundary, counts=counts)                        # (one run of the boundary loss: weights and counts)
    q = _phase_index(f, counts)
    offsets, tube, w, T, _, I = _device_arrivals(f, cols)
    # every arrival's phase index: q[column, tube], the column of its group's slot
    col = _arrival_columns(f, offsets, cols)
    qa = q[col, tube.long()].contiguous()
    if len(T) == 0:
        T, I, qa = _one_zero(f.dev), _one_zero(f.dev), _one_zero(f.dev, torch.int32)
    if lag is not None:
        phi = _arrival_lags(f, lag, col, tube, w) if len(tube) else _one_zero(f.dev)
        return offsets, tube, w, T, I, qa, col, phi.contiguous()
    return offsets, tube, w, T, I, qa, col


def _to_host(f, cols, re, im, axis=1):
    """re / im (R, n, m) on the device -> complex128 (R, n, m) on the host, re then im, the source's own columns NaN (`axis`:
    the axis of the n columns when it is not 1)"""
    import torch
    at_source = np.flatnonzero(np.abs(np.asarray(f.x)[cols] - f.x[0]) == 0)
    if len(at_source):                                                # the source's own column, as pressure_field has it
        idx = torch.from_numpy(at_source).to(f.dev)
        re.index_fill_(axis, idx, math.nan)
        im.index_fill_(axis, idx, math.nan)
    out = np.empty(tuple(re.shape), dtype=np.complex128)
    out.real = re.cpu().numpy()
    out.imag = im.cpu().numpy()
    return out


def _band_absorption(absorption, freq):
    """``absorption(freq)``, a callable's dB/km at every frequency, checked -> alpha in dB per METRE (F,); the callable's own
    errors propagate"""
    a = np.asarray(absorption(freq.copy()), dtype=float)
    if a.shape != freq.shape:
        raise ValueError(f"absorption(frequencies) must give one value in dB/km per frequency: shape {freq.shape}, not "
                         f"{a.shape}")
    if not np.all(np.isfinite(a)) or np.any(a < 0):
        raise ValueError("absorption(frequencies) must be finite and >= 0 dB/km")
    return np.ascontiguousarray(a / 1000.0)


def _fft_sizes(n_source, n_times, n_fft):
    """(n_times, n_fft) of ``received_waveform`` from what was given, checked"""
    def whole(v, name):
        if isinstance(v, (bool, float)) or int(v) != v or int(v) < 1:
            raise ValueError(f"{name} must be an integer >= 1")
        return int(v)
    if n_times is None and n_fft is None:
        raise ValueError("give n_times, n_fft or both")
    nt = None if n_times is None else whole(n_times, "n_times")
    if n_fft is None:
        nf = 1 << (nt + n_source - 1).bit_length()
    else:
        nf = whole(n_fft, "n_fft")
    nt = nf if nt is None else nt
    if nf < n_source:
        raise ValueError(f"n_fft ({nf}) must be at least the length of source ({n_source})")
    if nt > nf:
        raise ValueError(f"n_times ({nt}) must be <= n_fft ({nf})")
    return nt, nf


def _synthesise(H_of, source, dt, carrier, t0, n_times, n_fft):
    """``received_waveform``'s checks and its FFT synthesis around a transfer function: ``H_of(frequencies, t_reduce)`` -> H
    (R, n, n_fft), as ``transfer_function`` gives it -> u (R, n, n_times).  Shared with ``beam_received_waveform``."""
    s = np.asarray(source)
    if s.ndim != 1 or len(s) == 0:
        raise ValueError("source must be a non-empty 1-D sequence of complex baseband samples")
    s = s.astype(np.complex128)
    if not np.all(np.isfinite(s)):
        raise ValueError("source must be finite")
    step, fc = float(dt), float(carrier)
    if not (np.isfinite(step) and step > 0):
        raise ValueError("dt must be finite and > 0 seconds")
    if not (np.isfinite(fc) and fc >= 1.0 / (2.0 * step)):
        raise ValueError("carrier must be finite and at least 1 / (2 dt) Hz: the band carrier +- 1 / (2 dt) must not reach "
                         "negative frequencies")
    nt, nf = _fft_sizes(len(s), n_times, n_fft)
    start = np.asarray(t0, dtype=float)
    if not np.all(np.isfinite(start)):
        raise ValueError("t0 must be finite")
    nu = np.fft.fftfreq(nf, step)
    Shat = nf * np.fft.ifft(s, nf)
    H = H_of(fc + nu, start)
    cyc = fc * np.broadcast_to(start, (H.shape[1],))
    turn = np.exp(2j * np.pi * (cyc - np.rint(cyc)))
    u = np.fft.fft(Shat * H, axis=-1) / nf * turn[None, :, None]
    return np.ascontiguousarray(u[:, :, :nt])
