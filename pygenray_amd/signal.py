"""``received_signal``: the time series a receiver records when the source sends a Gaussian pulse, summed over the fan's
ray-tube arrivals ("Received signal of a Gaussian pulse").

No reference counterpart: pygenray gives back rays, not amplitudes.  The arrivals (csrc/pgr_arrivals.h), their phase index
(csrc/pgr_phase.h) and the sum over them at every time sample (csrc/pgr_signal.h) run in HIP and stay on the device from the
fan to the signal -- in HBM for a device-resident fan, uploaded through torch for a host fan.  There is no CPU path.
"""
import math

import numpy as np

from . import _lib
from .arrivals import _device_arrivals
from .coherent import _needs_counts, _phase_index
from .ray_objects import _columns
from .transmission import _FanFrame, _absorption_profile, _boundary_spec, _lag_spec


def pulse_sigma(bandwidth):
    """The width sigma (seconds) of the Gaussian envelope exp(-t^2 / (2 sigma^2)) whose spectrum has the half-power full
    bandwidth ``bandwidth`` (Hz, finite, >= 0): sigma = sqrt(ln 2) / (pi B); ``inf`` for 0, a continuous wave."""
    B = float(bandwidth)
    if not (math.isfinite(B) and B >= 0):
        raise ValueError("bandwidth must be finite and >= 0 Hz")
    return math.inf if B == 0 else math.sqrt(math.log(2.0)) / (math.pi * B)


def _inv_sigma(bandwidth):
    """1 / sigma of ``pulse_sigma``, formed without the detour over inf: pi B / sqrt(ln 2), 0.0 for B = 0"""
    B = float(bandwidth)
    if not (math.isfinite(B) and B >= 0):
        raise ValueError("bandwidth must be finite and >= 0 Hz")
    return math.pi * B / math.sqrt(math.log(2.0))


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


def _check_fits(f, R, n, m, product, entries):
    """``ValueError`` when re and im, (R, n, m) float64 each, do not fit in the free memory of the frame's device"""
    import torch
    # re and im on the device; the host copy is made of them one after the other
    need = 16 * R * n * m
    free = torch.cuda.mem_get_info(f.dev)[0]
    if need > free:
        raise ValueError(f"the {product} needs {need} bytes of device memory ({R} x {n} x {m} complex {entries}) and {free} "
                         f"are free: ask for fewer depths, columns or {entries} per call")


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
    G, n = len(f.depths) * len(cols), len(cols)
    # every arrival's phase index: q[column, tube], the column of its group's slot
    group = torch.repeat_interleave(torch.arange(G, device=f.dev), offsets[1:] - offsets[:-1])
    col = torch.from_numpy(cols.astype(np.int64)).to(f.dev)[group % n]
    qa = q[col, tube.long()].contiguous()
    if len(T) == 0:                                                   # (no arrivals at all: the entry refuses null pointers)
        T, I = (torch.zeros(1, dtype=torch.float64, device=f.dev) for _ in range(2))
        qa = torch.zeros(1, dtype=torch.int32, device=f.dev)
    if lag is not None:
        phi = _arrival_lags(f, lag, col, tube, w) if len(tube) else torch.zeros(1, dtype=torch.float64, device=f.dev)
        return offsets, tube, w, T, I, qa, col, phi.contiguous()
    return offsets, tube, w, T, I, qa, col


def _to_host(f, cols, re, im):
    """re / im (R, n, m) on the device -> complex128 (R, n, m) on the host, re then im, the source's own columns NaN"""
    import torch
    at_source = np.flatnonzero(np.abs(np.asarray(f.x)[cols] - f.x[0]) == 0)
    if len(at_source):                                                # the source's own column, as pressure_field has it
        idx = torch.from_numpy(at_source).to(f.dev)
        re[:, idx, :] = math.nan
        im[:, idx, :] = math.nan
    out = np.empty(tuple(re.shape), dtype=np.complex128)
    out.real = re.cpu().numpy()
    out.imag = im.cpu().numpy()
    return out


def received_signal(rays, receiver_depths, env, frequency, bandwidth, t0, dt, n_times, range_indices=None, absorption=None,
                    bottom_loss=None, surface_loss=None, flatearth=True, device=0):
    """The complex-demodulated signal of ``rays`` (a ``RayFan`` from ``shoot_rays``) at ``receiver_depths`` (metres, positive
    down, strictly ascending) and the save columns ``range_indices`` (default ``[S - 1]``, as in ``arrivals``) when the source
    sends a Gaussian pulse of centre ``frequency`` (Hz, finite, >= 0) and half-power full bandwidth ``bandwidth`` (Hz,
    finite, >= 0) -> complex128 ndarray ``(R, n, n_times)``, re 1 m, at the times ``t0 + arange(n_times) * dt`` (``dt`` > 0
    seconds; ``t0`` a scalar or one value per requested column, e.g. the reduced time x / c_red).  Every arrival of
    ``arrivals`` -- every tube ``pressure_field`` adds -- contributes

        u(t) += sqrt(I) exp(i (2 pi f T - (pi / 2) q)) E(t - T),   E(tau) = exp(-tau^2 / (2 sigma^2)),  q = kappa + 2 n_surf

    with sigma = ``pulse_sigma(bandwidth)``, the envelope cut at 8 sigma (E = 1.3e-14), summed arrival by arrival in tube
    order.  u is the baseband signal; the analytic passband signal is ``u(t) exp(-2j pi f t)``, in ``pressure_field``'s sign
    convention.  ``bandwidth=0`` is the CW limit: every sample equals ``pressure_field(...)[j, column]``.  A requested column
    with r = 0 is NaN, as in ``pressure_field``; where no arrival is within 8 sigma the signal is 0.

    ``absorption``, ``bottom_loss``, ``surface_loss``: the weights of ``transmission_loss``, exactly; a ``BottomReflection``
    as ``bottom_loss`` also turns every arrival by its bottom bounces' phase, as in ``pressure_field``.  The absorption
    weights are those of the one profile given, i.e. of the centre frequency: they are not varied across the band
    (``received_waveform`` with a callable ``absorption`` varies them).  The
    frame, the sound speed and the errors are ``pressure_field``'s (a fan with bounces needs its bounce log,
    ``shoot_rays(..., max_bounces=K)``).  ``ValueError`` when ``R * n * n_times`` complex samples do not fit in the free
    device memory, before any kernel runs.  A device-resident fan is processed where it is and stays device resident."""
    f0 = float(frequency)
    if not (np.isfinite(f0) and f0 >= 0):
        raise ValueError("frequency must be finite and >= 0 Hz")
    rs = _inv_sigma(bandwidth)
    step = float(dt)
    if not (np.isfinite(step) and step > 0):
        raise ValueError("dt must be finite and > 0 seconds")
    if isinstance(n_times, (bool, float)) or int(n_times) != n_times or int(n_times) < 1:
        raise ValueError("n_times must be an integer >= 1")
    nt = int(n_times)
    if nt > 65535 * 256:
        raise ValueError(f"n_times must be <= {65535 * 256}")
    profile = None if absorption is None else _absorption_profile(absorption)
    boundary = _boundary_spec(rays, bottom_loss, surface_loss)
    f = _FanFrame(rays, receiver_depths, env, flatearth, "received_signal")
    counts = _needs_counts(rays)
    cols = _columns(range_indices, len(f.x))
    R, n = len(f.depths), len(cols)
    start = _per_column(t0, n, "t0", "start time")
    f.to_device(device)
    import torch
    _check_fits(f, R, n, nt, "signal", "samples")
    lag = _lag_spec(bottom_loss)
    offsets, _, _, T, I, qa, _, *phi = _arrival_terms(f, cols, profile, boundary, counts, lag)
    tstart = f.upload(np.tile(start, R))
    re, im = (torch.empty((R, n, nt), dtype=torch.float64, device=f.dev) for _ in range(2))
    if lag is None:
        _lib.signal_device(f.env.device, offsets.data_ptr(), R * n, T.data_ptr(), I.data_ptr(), qa.data_ptr(), tstart.data_ptr(),
                           f0, rs, step, nt, re.data_ptr(), im.data_ptr(), f.stream)
    else:
        _lib.signal_phi_device(f.env.device, offsets.data_ptr(), R * n, T.data_ptr(), I.data_ptr(), qa.data_ptr(),
                               phi[0].data_ptr(), tstart.data_ptr(), f0, rs, step, nt, re.data_ptr(), im.data_ptr(), f.stream)
    return _to_host(f, cols, re, im)


__all__ = ["received_signal", "pulse_sigma"]
