"""Result containers with pygenray's layout and sign convention.

Mirrors ``pygenray.ray_objects`` (REF = /root/reference/src/pygenray): ``Ray``
(REF/ray_objects.py:7-59), ``RayFan`` (REF/ray_objects.py:75-155, 262-430) and ``EigenRays``
(REF/ray_objects.py:433-548).  Stored convention: ``z = -z_ode``, ``p = -p_ode`` (Q3).
``RayFan.from_arrays`` builds a fan straight from the SoA buffers the HIP path returns,
without materialising per-ray Python objects.
"""
import numpy as np


def _columns(range_indices, S):
    """range_indices -> int32 column indices in 0 .. S - 1 (negative ones counted from the end)."""
    if range_indices is None:
        return np.array([S - 1], dtype=np.int32)
    ri = np.atleast_1d(np.asarray(range_indices))
    if ri.ndim != 1 or len(ri) == 0:
        raise ValueError("range_indices must be a non-empty 1-D sequence of column indices")
    if ri.dtype.kind not in "iu":
        raise ValueError("range_indices must be integers")
    if not np.all((ri >= -S) & (ri < S)):
        raise ValueError(f"range_indices must lie in -{S} .. {S - 1} (the fan has {S} save ranges)")
    if len(ri) > 65535:
        raise ValueError("at most 65535 range_indices")
    return np.ascontiguousarray(np.where(ri < 0, ri + S, ri), dtype=np.int32)


def _id_strings(numbers, n_botts, n_surfs):
    """the reference's ray-id strings (REF/ray_objects.py:143-155): the numeric id as text, 'b' when the ray touched a
    boundary"""
    txt = numbers.astype(str)  # same text as str(np.float64): '-3.0', '0.0', ...
    return np.where((n_botts == 0) & (n_surfs == 0), txt, np.char.add(txt, "b"))


class BounceLog:
    """The bounce log of a fan (``shoot_rays(..., max_bounces=K)``), host arrays over the fan's M rays:

    - ``x`` (M, K): the range of each bounce in the frame the fan was traced in (a backwards fan is traced mirrored: minus
      the user's range), in the order the bounces happened
    - ``p`` (M, K): the slowness the ray leaves the bounce with, the stored sign convention of ``RayFan.ps``
    - ``kind`` (M, K) int8: 0 surface, 1 bottom; -1 in the slots a ray did not use (``x`` and ``p`` are NaN there)
    - ``count`` (M,) int64: the bounces logged per ray, ``n_botts + n_surfs`` of a fan ``shoot_rays`` returns"""

    def __init__(self, x, p, kind):
        self.x, self.p, self.kind = np.asarray(x, dtype=float), np.asarray(p, dtype=float), np.asarray(kind, dtype=np.int8)

    @property
    def count(self):
        return np.sum(self.kind >= 0, axis=1).astype(np.int64)

    @property
    def capacity(self):
        return self.kind.shape[1]

    def __len__(self):
        return self.kind.shape[0]

    def take(self, idx):
        return BounceLog(self.x[idx], self.p[idx], self.kind[idx])

    @staticmethod
    def concatenate(a, b):
        """two fans' logs, the narrower one padded with empty slots"""
        K = max(a.capacity, b.capacity)

        def pad(v, fill):
            out = np.full((v.shape[0], K), fill, dtype=v.dtype)
            out[:, :v.shape[1]] = v
            return out
        return BounceLog(*(np.concatenate([pad(u, f), pad(v, f)]) for u, v, f in
                           ((a.x, b.x, np.nan), (a.p, b.p, np.nan), (a.kind, b.kind, -1))))

    def sample_index(self, xf):
        """j_e = argmin_s |xf_s - x_e| (first minimum), the sample from which the reference's _interpolate_ray gives a
        segment that starts at x_e its samples (REF/launch_rays.py:745-784) -> (M, K) int64; xf: the save ranges in the
        traced frame.  Slots without an event get len(xf) (beyond every column)."""
        xf = np.asarray(xf, dtype=float)
        j = np.zeros(self.x.shape, np.int64)
        step = max(1, 4_000_000 // max(1, self.x.shape[1] * len(xf)))       # (np.argmin itself, a few million distances at a time)
        with np.errstate(invalid="ignore"):
            for m in range(0, self.x.shape[0], step):
                j[m:m + step] = np.argmin(np.abs(xf[None, None, :] - self.x[m:m + step, :, None]), axis=2)
        j = np.where(np.isfinite(self.x), j, 0)
        return np.where(self.kind >= 0, j, len(xf)).astype(np.int64)

    def counts(self, xf, cols):
        """(n_bott, n_surf), each (M, len(cols)) int64: the logged bounces of each kind that precede the samples at the
        columns `cols` of the save ranges xf -- the rule of DESIGN.md section 14: an event counts at column s when
        j_e <= s, and every logged event counts at the last column."""
        S, cols = len(xf), np.asarray(cols)
        M, K = self.kind.shape
        j = self.sample_index(xf)
        nb, ns = np.zeros((M, len(cols)), np.int64), np.zeros((M, len(cols)), np.int64)
        step = max(1, 4_000_000 // max(1, K * len(cols)))           # (a few million comparisons at a time, as sample_index)
        for m in range(0, M, step):
            hit = (j[m:m + step, :, None] <= cols[None, None, :]) | (cols[None, None, :] == S - 1)
            for out, kind in ((nb, 1), (ns, 0)):
                out[m:m + step] = (hit & (self.kind[m:m + step] == kind)[:, :, None]).sum(axis=1)
        return nb, ns


class Ray:
    """Single ray (REF/ray_objects.py:7-59).  ``y`` is ODE-convention [T; z; p] of shape (3, S)."""

    def __init__(self, r, y, n_bottom, n_surface, launch_angle=None, source_depth=None):
        self.r = r
        self.t = y[0, :]
        self.z = -y[1, :]  # negative-z storage convention
        self.p = -y[2, :]
        self.n_bottom = n_bottom
        self.n_surface = n_surface
        if launch_angle is not None:
            self.launch_angle = launch_angle
        if source_depth is not None:
            self.source_depth = source_depth

    def plot(self, **kwargs):
        from matplotlib import pyplot as plt
        plt.plot(self.r, self.z, **kwargs)
        plt.xlabel("time [s]")
        plt.ylabel("depth [m]")
        plt.ylim([self.z.min(), self.z.max()])


class RayFan:
    """Ray fan (REF/ray_objects.py:75-136): ``thetas (M,)``, ``rs/ts/zs/ps (M, S)``,
    ``n_botts/n_surfs/source_depths (M,)``, ``ray_ids (M,)``."""

    def __init__(self, Rays):
        self.thetas = np.array([r.launch_angle for r in Rays])
        self.rs = np.array([r.r for r in Rays])
        self.ts = np.array([r.t for r in Rays])
        self.zs = np.array([r.z for r in Rays])
        self.ps = np.array([r.p for r in Rays])
        self.n_botts = np.array([r.n_bottom for r in Rays])
        self.n_surfs = np.array([r.n_surface for r in Rays])
        self.source_depths = np.array([r.source_depth for r in Rays])
        self.compute_rayids()

    @classmethod
    def from_arrays(cls, thetas, rs, ts, zs, ps, n_botts, n_surfs, source_depths):
        """Stored-convention arrays in, no copies of the (M, S) blocks."""
        self = cls.__new__(cls)
        self.thetas = np.asarray(thetas)
        self.rs, self.ts, self.zs, self.ps = rs, ts, zs, ps
        self.n_botts = np.asarray(n_botts)
        self.n_surfs = np.asarray(n_surfs)
        self.source_depths = np.asarray(source_depths)
        self._ray_ids = None  # built on first access (a million-ray fan pays 0.2 s for the strings)
        self._bounces = None
        return self

    @classmethod
    def from_device(cls, handle, thetas, r, end, n_botts, n_surfs, source_depths):
        """A fan whose trajectories are still in HBM (``_lib.FanHandle``, launched with the stored sign convention):
        ``ts`` / ``zs`` / ``ps`` cross PCIe when they are first read -- each on its own, dropped rays already squeezed
        out on the device -- and are ordinary (M, S) arrays from then on; ``rs`` is a broadcast view of the save grid.
        The per-ray arrays and the end states (``ts_end``, ``zs_end``, ``ps_end``: the last column, what
        ``find_eigenrays`` brackets on, REF/eigenrays.py:65-79) are on the host from the start.  `end` is the
        ODE-convention end state of the surviving rays."""
        self = cls.__new__(cls)
        self.thetas = np.asarray(thetas)
        self._dev = handle
        self._r = np.asarray(r)
        self._end = np.asarray(end)
        self.n_botts = np.asarray(n_botts)
        self.n_surfs = np.asarray(n_surfs)
        self.source_depths = np.asarray(source_depths)
        self._ray_ids = None
        self._bounces = None     # (a fan launched with a log: fetched from the handle on first access)
        return self

    # ts / zs / ps / rs: plain attributes for a host fan, fetched from the device on first access for a device fan
    def _lazy(name, key):   # noqa: N805  (a property factory, not a method)
        def get(self):
            d = self.__dict__
            if name not in d:
                dev = d.get("_dev")
                if dev is None:
                    raise AttributeError(name[1:])
                d[name] = dev.fetch_samples((key,), compact=True)[key].T     # (M, S) view of the [S][M] block
                if all(k in d for k in ("_ts", "_zs", "_ps")):
                    self.bounces            # noqa: B018  (the log, if the fan has one, comes over before the handle goes)
                    dev.close()             # everything is on the host: give the HBM back
                    d["_dev"] = None
            return d[name]

        def set_(self, value):
            self.__dict__[name] = value
        return property(get, set_)

    ts = _lazy("_ts", "T")
    zs = _lazy("_zs", "z")
    ps = _lazy("_ps", "p")
    del _lazy

    @property
    def rs(self):
        d = self.__dict__
        if "_rs" not in d:
            if d.get("_r") is None:
                raise AttributeError("rs")
            d["_rs"] = np.broadcast_to(d["_r"], (len(self.thetas), len(d["_r"])))
        return d["_rs"]

    @rs.setter
    def rs(self, value):
        self.__dict__["_rs"] = value

    @property
    def device_resident(self):
        """True while some trajectory array has not been fetched from the GPU yet."""
        return self.__dict__.get("_dev") is not None

    # A device-resident fan pins 3 * N * S * 8 B of HBM (2.4 GB for 1e5 rays x 1001 samples) until ts, zs AND ps have been
    # read, or to_host() / release() is called, or the fan is garbage collected; `rs` of such a fan is a read-only broadcast
    # view of the save grid (np.array(fan.rs) for a private copy).
    def to_host(self):
        """Fetch whatever is still on the GPU and give the HBM back; the fan is a plain host object afterwards."""
        if self.device_resident:
            self.ts, self.zs, self.ps       # noqa: B018  (the third read closes the handle)
        return self

    def release(self):
        """Give the HBM back WITHOUT fetching: trajectory arrays not read so far are gone (reading them raises
        AttributeError); end states, bounce counts and launch angles stay."""
        dev = self.__dict__.get("_dev")
        if dev is not None:
            self.bounces                    # noqa: B018  (per-ray data, 17 bytes per slot: it stays, like the bounce counts)
            dev.close()
            self.__dict__["_dev"] = None

    # ---- the bounce log ----
    @property
    def bounces(self):
        """The fan's ``BounceLog`` (``shoot_rays(..., max_bounces=K)``), or None for a fan traced without one.  Fetched from
        the device on first access (K * M * 17 bytes); a device-resident fan stays device resident."""
        d = self.__dict__
        if d.get("_bounces") is None:
            dev = d.get("_dev")
            if dev is not None and getattr(dev, "K", 0):
                x, p, k = dev.fetch_bounces()
                d["_bounces"] = BounceLog(x.T, p.T, k.T)
        return d.get("_bounces")

    def _has_bounce_log(self):
        """a log on the host or on the fan's device handle (asking fetches nothing)"""
        d = self.__dict__
        return d.get("_bounces") is not None or bool(getattr(d.get("_dev"), "K", 0))

    def _traced_ranges(self):
        """the save ranges in the frame the fan was traced in (mirrored for a backwards fan)"""
        r = self.__dict__.get("_r")
        x = np.asarray(r if r is not None else np.asarray(self.rs)[0], dtype=float)
        return -x if (len(x) > 1 and x[-1] < x[0]) else x

    def bounce_counts(self, range_indices=None):
        """The bottom and surface bounces every ray has made on its way to the save columns ``range_indices`` (default
        ``[S - 1]``; any integers in -S .. S - 1) -> ``(n_bott, n_surf)``, each ``(M, n)`` int64.  A bounce precedes the
        samples the reference's re-sampling gives the segment that starts at it: column s counts the bounces whose nearest
        save range (``np.argmin``'s first minimum) is at or before s, and the last column counts them all, so that it
        equals ``n_botts`` / ``n_surfs``.  Needs a fan traced with a bounce log (``max_bounces=``)."""
        log = self.bounces
        if log is None:
            raise ValueError("the fan has no bounce log: trace it with shoot_rays(..., max_bounces=K)")
        xf = self._traced_ranges()
        cols = _columns(range_indices, len(xf))
        return log.counts(xf, cols)

    def __getstate__(self):
        """pickle / copy.deepcopy / multiprocessing: the state of a plain host fan (the reference's RayFan is a plain
        object).  A device-resident fan is fetched first -- its handle wraps a device pointer that means nothing in
        another process."""
        self.to_host()
        d = dict(self.__dict__)
        d.pop("_dev", None)
        if d.get("_r") is not None:
            d.pop("_rs", None)              # the broadcast view is rebuilt from the save grid on first access
        return d

    def __setstate__(self, state):
        self.__dict__.update(state)
        self.__dict__.setdefault("_ray_ids", None)
        self.__dict__.setdefault("_bounces", None)

    # the state at receiver_range, stored convention, without touching the trajectories
    @property
    def ts_end(self):
        e = self.__dict__.get("_end")
        return e[:, 0] if e is not None else self.ts[:, -1]

    @property
    def zs_end(self):
        e = self.__dict__.get("_end")
        if e is None:
            return self.zs[:, -1]
        if self.__dict__.get("_zs_end") is None:      # (what find_eigenrays brackets on, once per receiver depth)
            self.__dict__["_zs_end"] = -e[:, 1]
        return self.__dict__["_zs_end"]

    @property
    def ps_end(self):
        e = self.__dict__.get("_end")
        return -e[:, 2] if e is not None else self.ps[:, -1]

    @property
    def ray_ids(self):
        if getattr(self, "_ray_ids", None) is None:
            self.compute_rayids()
        return self._ray_ids

    @ray_ids.setter
    def ray_ids(self, value):
        self._ray_ids = value

    def compute_rayids(self):
        """Ray IDs: number of sign changes of p times sign(theta), 'b' suffix when the ray
        touched a boundary (REF/ray_objects.py:138-155)."""
        if len(self.thetas) == 0:
            self.ray_ids = np.array([], dtype=str)
            return
        if self._ps_in_hbm():      # the count from the kernel, where the fan is: no (M, S) block crosses PCIe for M integers
            turns = self.turning_points()[:, 0]
        else:
            turns = np.sum(np.diff(np.sign(self.ps)) != 0, axis=1)
        self.ray_ids = _id_strings(turns * np.sign(self.thetas), self.n_botts, self.n_surfs)

    # ---- turning points and time fronts at any save column ----
    def _ps_in_hbm(self):
        """a device-resident fan whose ps has not been fetched"""
        return self.__dict__.get("_dev") is not None and "_ps" not in self.__dict__

    def _n_save(self):
        dev = self.__dict__.get("_dev")
        return dev.S if dev is not None else np.shape(self.ps)[1]

    def _front_device(self, cols, samples):
        """pgr_fan_time_front on the fan in HBM -> turns (M, n) int64 and, with `samples`, t, z, p (M, n); nothing else is
        fetched and the fan stays device resident"""
        import torch
        h = self._dev
        dev = torch.device("cuda", h._env.device)
        n, M = len(cols), len(self.thetas)
        turns = torch.empty((n, M), dtype=torch.int32, device=dev)
        tzp = [torch.empty((n, M), dtype=torch.float64, device=dev) for _ in range(3 if samples else 0)]
        h.time_front(cols, *([a.data_ptr() for a in tzp] or [0, 0, 0]), turns.data_ptr(),
                     torch.cuda.current_stream(dev).cuda_stream)
        return (turns.cpu().numpy().T.astype(np.int64),) + tuple(a.cpu().numpy().T for a in tzp)

    def turning_points(self, range_indices=None):
        """The number of turning points of every ray on its way to the save columns ``range_indices`` (default ``[S - 1]``,
        the receiver range; any integers in -S .. S - 1) -> ``(M, n)`` int64: the sign changes of p up to each column,
        ``np.sum(np.diff(np.sign(ps[:, :col + 1]), axis=1) != 0, axis=1)`` -- the reference's ray-id count
        (REF/ray_objects.py:142) applied to the path so far.  A device-resident fan whose ``ps`` has not been read is
        counted where it is (csrc/pgr_front.h) and stays device resident; the values are the same either way."""
        cols = _columns(range_indices, self._n_save())
        if len(self.thetas) == 0:
            return np.zeros((0, len(cols)), dtype=np.int64)
        if self._ps_in_hbm():
            return self._front_device(cols, False)[0]
        ps = np.asarray(self.ps)
        if len(cols) == 1:
            return np.sum(np.diff(np.sign(ps[:, :cols[0] + 1]), axis=1) != 0, axis=1).astype(np.int64)[:, None]
        last = int(cols.max())
        run = np.zeros((ps.shape[0], last + 1), dtype=np.int64)         # run[:, c]: the changes in front of column c
        np.cumsum(np.diff(np.sign(ps[:, :last + 1]), axis=1) != 0, axis=1, out=run[:, 1:])
        return run[:, cols]

    def time_front(self, range_idx=-1):
        """The time front at save column ``range_idx`` (an integer in -S .. S - 1) -> ``TimeFront``: travel time, depth,
        slowness and turning-point count of every ray there.  A device-resident fan hands over that one column of each
        array (csrc/pgr_front.h) and stays device resident; ``ts[:, k]``, ``zs[:, k]``, ``ps[:, k]`` bit for bit."""
        if np.ndim(range_idx) != 0:
            raise ValueError("range_idx must be one column index")
        S = self._n_save()
        k = int(_columns(range_idx, S)[0])
        M = len(self.thetas)
        if self.device_resident and M:
            turns, t, z, p = (a[:, 0] for a in self._front_device([k], True))
        else:
            turns = self.turning_points([k])[:, 0]
            t, z, p = (np.asarray(a)[:, k] for a in (self.ts, self.zs, self.ps))
        rng = np.asarray(self.rs)[:, k] if M else np.zeros(0)
        if k == S - 1:
            ids = self.ray_ids
        elif M and self.bounces is not None:       # a logged fan knows its bounces at every column
            nb, ns = self.bounce_counts([k])
            ids = _id_strings(turns * np.sign(self.thetas), nb[:, 0], ns[:, 0])
        else:
            ids = None
        return TimeFront(rng, k, self.thetas, t, z, p, turns, ids)

    def __len__(self):
        return len(self.thetas)

    def _ray(self, i):
        # REF/ray_objects.py:385-393: re-negate so Ray() flips back to the stored convention
        return Ray(r=self.rs[i], y=np.array([self.ts[i], -self.zs[i], -self.ps[i]]),
                   n_bottom=self.n_botts[i], n_surface=self.n_surfs[i],
                   launch_angle=self.thetas[i], source_depth=self.source_depths[i])

    def __getitem__(self, key):
        """int -> Ray; slice / index array / boolean mask -> RayFan (REF/ray_objects.py:358-430)."""
        if isinstance(key, (int, np.integer)):
            key = int(key)
            if key < 0:
                key = len(self.thetas) + key
            if key < 0 or key >= len(self.thetas):
                raise IndexError(
                    f"Index {key} is out of bounds for RayFan with {len(self.thetas)} rays")
            return self._ray(key)
        if isinstance(key, slice):
            idx = np.arange(len(self.thetas))[key]
        else:
            idx = np.asarray(key)
            if idx.dtype == bool:
                idx = np.where(idx)[0]
        if idx.ndim == 0:
            idx = idx.reshape(1)
        elif idx.ndim != 1:
            raise ValueError("Invalid indexing array shape")
        out = RayFan.from_arrays(self.thetas[idx], self.rs[idx], self.ts[idx], self.zs[idx],
                                 self.ps[idx], self.n_botts[idx], self.n_surfs[idx],
                                 self.source_depths[idx])
        if self.bounces is not None:
            out._bounces = self.bounces.take(idx)
        return out

    def __add__(self, other):
        """Concatenate along the launch-angle dimension (REF/ray_objects.py:290-345).  Unlike
        the reference (whose ``__add__`` rebuilds Rays without re-negating and so flips the
        sign of zs/ps, Q3), the stored convention is preserved."""
        if not isinstance(other, RayFan):
            raise TypeError("Can only add RayFan objects together")
        if not np.array_equal(self.rs[0], other.rs[0]):
            raise ValueError("Range arrays (rs) must be equivalent for concatenation")
        cat = np.concatenate
        out = RayFan.from_arrays(cat([self.thetas, other.thetas]), cat([self.rs, other.rs]),
                                 cat([self.ts, other.ts]), cat([self.zs, other.zs]),
                                 cat([self.ps, other.ps]), cat([self.n_botts, other.n_botts]),
                                 cat([self.n_surfs, other.n_surfs]),
                                 cat([self.source_depths, other.source_depths]))
        if self.bounces is not None and other.bounces is not None:     # (a sum with an unlogged fan has no log)
            out._bounces = BounceLog.concatenate(self.bounces, other.bounces)
        return out

    def save_mat(self, filename):
        """.mat export with the reference's schema (REF/ray_objects.py:262-288)."""
        from scipy import io
        io.savemat(filename, {"rayfan": {
            "thetas": self.thetas, "xs": self.rs, "ts": self.ts, "zs": self.zs, "ps": self.ps,
            "n_botts": self.n_botts, "n_surfs": self.n_surfs, "source_depths": self.source_depths}})

    # ---- plots (REF/ray_objects.py:157-260) ----
    def plot_time_front(self, include_lines=False, range_idx=-1, add_colorbar=True, ray_id=False,
                        **kwargs):
        self.time_front(range_idx).plot(include_lines=include_lines, add_colorbar=add_colorbar,
                                        ray_id=self.ray_ids if ray_id else False, **kwargs)

    def plot_ray_fan(self, **kwargs):
        from matplotlib import pyplot as plt
        a = 10 * 1 / max(len(self.thetas), 1)
        kw = {"c": "k", "lw": 1, "alpha": 1 if (a > 1 or a < 0) else a}
        kw.update(kwargs)
        plt.plot(self.rs.T, self.zs.T, **kw)

    def plot_depth_v_angle(self, include_line=False, **kwargs):
        from matplotlib import pyplot as plt
        kw = {"c": self.thetas, "cmap": "viridis", "s": 2, "lw": 0, "zorder": 6}
        kw.update(kwargs)
        if include_line:
            plt.plot(self.thetas, self.zs[:, -1], c="#aaaaaa", lw=0.5)
        plt.scatter(self.thetas, self.zs[:, -1], **kw)
        plt.xlabel("launch angle [°]")
        plt.ylabel("depth [m]")


class TimeFront:
    """The time front of a fan at one save column (``RayFan.time_front``; what the reference's ``plot_time_front(range_idx=k)``
    scatters, REF/ray_objects.py:157-222), host arrays over the fan's M rays:

    - ``range`` (M,): the column's range; ``range_index``: the column k (0 .. S - 1)
    - ``thetas``: launch angles, degrees, ``RayFan.thetas``
    - ``t``, ``z``, ``p``: ``ts[:, k]``, ``zs[:, k]``, ``ps[:, k]``, the stored sign convention, bit for bit
    - ``turning_points`` (int64): the sign changes of p on the way to column k (``RayFan.turning_points``)
    - ``ray_numbers``: ``turning_points * np.sign(thetas)``, the reference's numeric ray id (REF/ray_objects.py:142)
    - ``ray_ids``: the reference's strings, the number with a ``b`` suffix for a ray that touched a boundary.  Without a
      bounce log the counts ``n_botts`` / ``n_surfs`` are known only at a ray's end, so the strings exist at the fan's last
      column (where they equal ``RayFan.ray_ids``) and are ``None`` at every other column; a fan traced with a bounce log
      (``shoot_rays(..., max_bounces=K)``) has them at every column, from ``RayFan.bounce_counts``."""

    def __init__(self, range, range_index, thetas, t, z, p, turning_points, ray_ids=None):   # noqa: A002
        self.range = range
        self.range_index = range_index
        self.thetas = thetas
        self.t, self.z, self.p = t, z, p
        self.turning_points = turning_points
        self.ray_ids = ray_ids

    def __len__(self):
        return len(self.thetas)

    @property
    def ray_numbers(self):
        return self.turning_points * np.sign(self.thetas)

    def plot(self, include_lines=False, add_colorbar=True, ray_id=False, **kwargs):
        """The scatter of ``RayFan.plot_time_front``: depth against travel time, coloured by launch angle, or with
        ``ray_id`` by ray id: True for this front's own (``ray_ids``, else ``ray_numbers``), or one label per ray."""
        from matplotlib import pyplot as plt
        if include_lines:
            plt.plot(self.t, self.z, c="#aaaaaa", lw=0.5, zorder=5)
        kw = {"c": self.thetas, "cmap": "viridis", "s": 2, "lw": 0, "zorder": 6}
        kw.update(kwargs)
        if ray_id is not False and ray_id is not None:
            ids = ray_id if not isinstance(ray_id, (bool, np.bool_)) else (
                self.ray_ids if self.ray_ids is not None else self.ray_numbers.astype(str))
            cats = np.unique(ids)
            colors = plt.cm.tab20(np.linspace(0, 1, len(cats)))
            lut = dict(zip(cats, colors))
            kw.update({"c": [lut[c] for c in ids]})
            kw.pop("cmap", None)
            add_colorbar = False
        plt.scatter(self.t, self.z, **kw)
        if add_colorbar:
            plt.colorbar(label="launch angle [°]")
        plt.xlabel("time [s]")
        plt.ylabel("depth [m]")

    def __repr__(self):
        return f"TimeFront({len(self)} rays at column {self.range_index})"


class EigenRays:
    """Eigenrays per receiver depth (REF/ray_objects.py:433-548)."""

    def __init__(self, receiver_depths, eigenray_dict, environment, num_eigenrays,
                 num_eigenrays_found, failed_eray_theta_brackets):
        from .host_physics import ray_angle
        from .environment import OceanEnvironment2D
        self.receiver_depths = receiver_depths
        self.rs, self.ts, self.zs, self.ps = {}, {}, {}, {}
        self.received_angles, self.launch_angles = {}, {}
        self.n_botts, self.n_surfs = {}, {}
        self.ray_id, self.ray_id_int = {}, {}
        self.num_eigenrays = num_eigenrays
        self.num_eigenrays_found = num_eigenrays_found
        self.failed_eray_theta_brackets = failed_eray_theta_brackets
        cin, rin, zin = OceanEnvironment2D._range_depth(environment.sound_speed)
        for ridx in range(len(receiver_depths)):
            fan = eigenray_dict[ridx]
            if not isinstance(fan, RayFan):
                fan = RayFan(fan)
            self.rs[ridx], self.ts[ridx], self.zs[ridx], self.ps[ridx] = fan.rs, fan.ts, fan.zs, fan.ps
            self.n_botts[ridx], self.n_surfs[ridx] = fan.n_botts, fan.n_surfs
            ang, ids, ids_int = [], [], []
            for k in range(len(fan)):
                # REF/ray_objects.py:521-534: received angle from the stored (negative-z)
                # state and the non-flat-earth table, exactly as the reference does (Q13)
                y_last = np.array([fan.ts[k, -1], fan.zs[k, -1], fan.ps[k, -1]])
                with np.errstate(invalid="ignore"):
                    theta, _ = ray_angle(fan.rs[k, -1], y_last, cin, rin, zin)
                ang.append(theta)
                rid = np.sum(np.diff(np.sign(fan.ps[k, :])) != 0) * np.sign(fan.thetas[k])
                flag = "" if (fan.n_botts[k] == 0 and fan.n_surfs[k] == 0) else "b"
                ids.append(f"{rid}{flag}")
                ids_int.append(int(rid))
            self.received_angles[ridx] = np.array(ang)
            self.launch_angles[ridx] = fan.thetas
            self.ray_id[ridx] = np.array(ids)
            self.ray_id_int[ridx] = np.array(ids_int)

    def plot_angle_time(self, ridxs=None, **kwargs):
        """Received angle against arrival time (REF/ray_objects.py:550-561)."""
        from matplotlib import pyplot as plt
        for ridx in (ridxs if ridxs is not None else list(self.received_angles.keys())):
            plt.scatter(self.ts[ridx][:, -1], self.received_angles[ridx], **kwargs)
        plt.xlabel("time [s]")
        plt.ylabel("received angle [deg]")
        plt.title("Received Angle vs Time")

    def plot(self, ridxs=[0], **kwargs):
        """All eigenrays of the given receiver-depth indices (REF/ray_objects.py:563-585)."""
        from matplotlib import pyplot as plt
        if isinstance(ridxs, (int, np.integer)):
            ridxs = [ridxs]
        kw = {"c": "k"}
        kw.update(kwargs)
        for ridx in ridxs:
            plt.plot(self.rs[ridx].T, self.zs[ridx].T, **kw)
        plt.xlabel("range [m]")
        plt.ylabel("depth [m]")
        plt.title("Eigen Rays")
        if len(ridxs) and self.zs[ridxs[-1]].size:
            plt.ylim([self.zs[ridxs[-1]].min(), self.zs[ridxs[-1]].max()])

    def plot_ducted(self, **kwargs):
        """The eigenrays that never touch a boundary, all receiver depths (REF/ray_objects.py:587-602; the
        reference plots -z here, depth positive down)."""
        from matplotlib import pyplot as plt
        kw = {"c": "k"}
        kw.update(kwargs)
        for ridx in self.ray_id.keys():
            mask = (self.n_botts[ridx] == 0) & (self.n_surfs[ridx] == 0)
            plt.plot(self.rs[ridx][mask].T, -self.zs[ridx][mask].T, **kw)
        plt.xlabel("range [m]")
        plt.ylabel("depth [m]")
        plt.title("Ducted Eigen Rays")

    def save_mat(self, filename):
        """.mat export with the reference's schema (REF/ray_objects.py:604-636): one struct per receiver depth,
        ``eigenrays.receiver_depth_<k>.{receiver_depth, xs, ts, zs, ps, received_angles, launch_angles, ray_id,
        ray_id_int, n_bottom, n_surface, source_depth, num_eigenrays, num_eigenrays_found}``.  (The per-depth counts
        are dictionaries in memory; MATLAB field names must be strings, so their keys are written as text.)"""
        from scipy import io

        def _fields(d):
            return {("k_" + str(k).replace(".", "p").replace("-", "m")): v for k, v in dict(d).items()}
        data = {}
        for ridx, rdepth in enumerate(self.receiver_depths):
            data[f"receiver_depth_{ridx}"] = {
                "receiver_depth": rdepth, "xs": self.rs[ridx], "ts": self.ts[ridx], "zs": self.zs[ridx], "ps": self.ps[ridx],
                "received_angles": self.received_angles[ridx], "launch_angles": self.launch_angles[ridx],
                "ray_id": self.ray_id[ridx], "ray_id_int": self.ray_id_int[ridx],
                "n_bottom": self.n_botts[ridx] if hasattr(self, "n_botts") else np.nan,
                "n_surface": self.n_surfs[ridx] if hasattr(self, "n_surfs") else np.nan,
                "source_depth": self.source_depths[ridx] if hasattr(self, "source_depths") else np.nan,
                "num_eigenrays": _fields(self.num_eigenrays), "num_eigenrays_found": _fields(self.num_eigenrays_found)}
        io.savemat(filename, {"eigenrays": data})


__all__ = ["Ray", "RayFan", "BounceLog", "TimeFront", "EigenRays"]
