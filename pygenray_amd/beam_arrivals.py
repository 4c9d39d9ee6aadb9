"""``beam_arrivals``: the terms of the coherent Gaussian-beam sum of a fan listed as arrivals, and the products summed over
them -- ``beam_received_signal``, ``beam_transfer_function``, ``beam_received_waveform``: the pulses and bands of ``signal`` and
``spectrum`` from beams instead of ray tubes ("Gaussian-beam arrivals").

A beam's term at a receiver does not depend on the frequency apart from exp(2 pi i f tau): its amplitude, its delay and its
phase index make it an arrival, and the sums of csrc/pgr_signal.h and csrc/pgr_spectrum.h take the list as they take the
tubes'.  The walk that lists the terms runs in HIP (csrc/pgr_beam_arrivals.h) on the fan's trajectories where they already
are -- in HBM for a device-resident fan, uploaded through torch for a host fan -- and the list stays on the device up to the
sum.  There is no CPU path.
"""
import numpy as np

from . import _lib
from ._fan_frame import (_arrival_columns, _arrival_lengths, _band, _band_absorption, _check_fits, _coherent_frame, _min_width,
                         _one_zero, _per_column, _phase_index, _pulse, _synthesise, _to_host)
from .ray_objects import _columns

_ARRIVAL_BYTES = 28          # tube, image, phase_index int32 and time, amplitude float64


class BeamArrivals:
    """The beam arrivals of a fan at ``receiver_depths`` (R) and the requested save columns ``range_indices`` (n), host arrays.

    Arrivals are grouped by receiver j, then by requested column c (the caller's order), then by increasing tube and, per
    tube, by image; those of (j, c) are ``[offsets[j * n + c], offsets[j * n + c + 1])`` (``at(j, c)`` slices them).  Per
    arrival:

    - ``tube``: index k into the fan's (surviving) rays; the beam is that of rays k and k + 1
    - ``image``: 0 the beam itself, 1 its image in the surface, 2 its image in the bottom
    - ``time``: T_m + p_m e + kappa e^2 / 2, seconds: the beam's travel time carried to the receiver, e the receiver's offset
      from the beam's centre (mirrored with the image)
    - ``amplitude``: A'_k exp(-e^2 / (2 sigma_k^2)), re 1 m; lazily ``intensity`` = ``amplitude ** 2``
    - ``phase_index``: quarter cycles, 0 ... 3: the tube's kappa + 2 n_surf, plus 2 for the surface image

    The arrival adds ``amplitude * exp(i (2 pi f time - (pi / 2) phase_index))`` to ``beam_pressure_field`` at every
    frequency f: summed in order from 0.0 they give that field at (j, column) bit for bit.  The source's own column (r = 0)
    has no arrivals."""

    def __init__(self, offsets, receiver_depths, ranges, range_indices, tube, image, time, amplitude, phase_index):
        self.offsets = offsets
        self.receiver_depths = receiver_depths
        self.ranges = ranges
        self.range_indices = range_indices
        self.tube = tube
        self.image = image
        self.time = time
        self.amplitude = amplitude
        self.phase_index = phase_index
        self._lazy = {}

    def __len__(self):
        return len(self.tube)

    @property
    def intensity(self):
        if "intensity" not in self._lazy:
            self._lazy["intensity"] = self.amplitude ** 2
        return self._lazy["intensity"]

    def at(self, j, c):
        """The arrivals at receiver j and requested column slot c -> dict of arrays (views)."""
        n = len(self.range_indices)
        if not (0 <= j < len(self.receiver_depths) and 0 <= c < n):
            raise IndexError(f"(j, c) = ({j}, {c}) outside ({len(self.receiver_depths)}, {n})")
        sl = slice(int(self.offsets[j * n + c]), int(self.offsets[j * n + c + 1]))
        return dict(tube=self.tube[sl], image=self.image[sl], time=self.time[sl], amplitude=self.amplitude[sl],
                    phase_index=self.phase_index[sl], intensity=self.intensity[sl])

    def __repr__(self):
        return (f"BeamArrivals({len(self)} arrivals at {len(self.receiver_depths)} receiver depths x "
                f"{len(self.range_indices)} ranges)")


def _beam_frame(rays, receiver_depths, env, min_width, range_indices, absorption, bottom_loss, surface_loss, flatearth, who):
    """Everything ``beam_pressure_field`` and ``arrivals`` refuse without a GPU -> (frame, cols, min_width, profile, boundary,
    counts); ``absorption`` None, a scalar or a pair (a callable is the caller's)."""
    w = _min_width(min_width)
    f, profile, boundary, counts = _coherent_frame(rays, receiver_depths, env, absorption, bottom_loss, surface_loss, flatearth,
                                                   who, beams=True)
    return f, _columns(range_indices, len(f.x)), w, profile, boundary, counts


def _device_beam_arrivals(f, cols, min_width, curvature, profile, boundary, counts, extra_bytes=0, fixed_bytes=0):
    """The beam arrivals of the frame `f` (a _FanFrame after to_device) at its receiver depths and the save columns `cols`,
    left on the device -> (offsets int64 [R * n + 1], tube, image int32, time, amplitude float64, q int32 [n_arrivals]): the
    weights and the phase index as ``beam_pressure_field`` forms them, then the count, the scan and the emit entries.
    ``ValueError`` before the emit pass when the arrays, with what the caller forms from them afterwards (`extra_bytes` more
    per arrival and `fixed_bytes` whatever their number), do not fit in free memory."""
    import torch
    f.absorb(profile, boundary, counts=counts)                        # (one run of the boundary loss: weights and counts)
    q = _phase_index(f, counts)
    d_b = f.upload(f.bottom())
    R, n = len(f.depths), len(cols)
    cnt = torch.empty(R * n, dtype=torch.int64, device=f.dev)
    f.run("beam_arrival_counts", q.data_ptr(), d_b.data_ptr(), f.d_depths.data_ptr(), R, min_width, cols, cnt.data_ptr())
    offsets = torch.zeros(R * n + 1, dtype=torch.int64, device=f.dev)
    torch.cumsum(cnt, 0, out=offsets[1:])
    total = int(offsets[-1].item())
    need, free = (_ARRIVAL_BYTES + extra_bytes) * total + fixed_bytes, torch.cuda.mem_get_info(f.dev)[0]
    if need > free:
        raise ValueError(f"the {total} beam arrivals need {need} bytes of device memory and {free} are free: ask for fewer "
                         "depths or columns per call")
    tube, image, qa = (torch.empty(total, dtype=torch.int32, device=f.dev) for _ in range(3))
    T, amp = (torch.empty(total, dtype=torch.float64, device=f.dev) for _ in range(2))
    if total:
        f.run("beam_arrivals", q.data_ptr(), d_b.data_ptr(), f.d_depths.data_ptr(), R, min_width, cols, bool(curvature),
              offsets.data_ptr(), total, tube.data_ptr(), image.data_ptr(), T.data_ptr(), amp.data_ptr(), qa.data_ptr())
    return offsets, tube, image, T, amp, qa


def _sum_terms(T, amp, qa):
    """(T, I, q) as pgr_signal_device / pgr_spectrum_device take them: I = amplitude * amplitude formed on the device; without
    arrivals one zero each (the entries refuse null pointers)"""
    import torch
    if len(T) == 0:
        return _one_zero(T.device), _one_zero(T.device), _one_zero(T.device, torch.int32)
    return T, amp * amp, qa


def beam_arrivals(rays, receiver_depths, env, min_width=10.0, curvature=True, range_indices=None, absorption=None,
                  bottom_loss=None, surface_loss=None, flatearth=True, device=0):
    """The Gaussian-beam arrivals of ``rays`` (a ``RayFan`` from ``shoot_rays``) at ``receiver_depths`` (metres, positive down,
    strictly ascending) and the save columns ``range_indices`` (default ``[S - 1]``, the receiver range; any integers in
    -S .. S - 1, as in ``arrivals``) -> ``BeamArrivals``.

    Every term ``beam_pressure_field`` adds at a receiver -- a tube's beam, its image in the surface or its image in the bottom,
    within 4 sigma of the receiver -- is one arrival: its delay, its amplitude and its phase index, none of which depends on the
    frequency.  ``min_width``, ``curvature``, ``absorption``, ``bottom_loss``, ``surface_loss``, the frame, the bathymetry
    and the errors are ``beam_pressure_field``'s (a ``BottomReflection`` as ``bottom_loss`` is refused; a fan with bounces
    needs its bounce log).  Unlike the tube arrivals of ``arrivals`` these have no spike at a caustic, reach the receivers
    along both boundaries and fade over sigma at a shadow edge.  ``ValueError`` naming their count when the arrivals do not
    fit in the free device memory.  A device-resident fan is processed where it is and stays device resident."""
    f, cols, w, profile, boundary, counts = _beam_frame(rays, receiver_depths, env, min_width, range_indices, absorption,
                                                        bottom_loss, surface_loss, flatearth, "beam_arrivals")
    f.to_device(device)
    offsets, tube, image, T, amp, qa = _device_beam_arrivals(f, cols, w, curvature, profile, boundary, counts)
    return BeamArrivals(offsets.cpu().numpy(), f.depths, np.asarray(f.x)[cols], cols.astype(np.int64), tube.cpu().numpy(),
                        image.cpu().numpy(), T.cpu().numpy(), amp.cpu().numpy(), qa.cpu().numpy())


def beam_received_signal(rays, receiver_depths, env, frequency, bandwidth, t0, dt, n_times, min_width=10.0, curvature=True,
                         range_indices=None, absorption=None, bottom_loss=None, surface_loss=None, flatearth=True, device=0):
    """``received_signal`` summed over the beam arrivals of ``beam_arrivals`` instead of the tube arrivals: the
    complex-demodulated signal of a Gaussian pulse of centre ``frequency`` and half-power full bandwidth ``bandwidth`` ->
    complex128 ndarray ``(R, n, n_times)`` at the times ``t0 + arange(n_times) * dt``; every arrival contributes

        u(t) += amplitude exp(i (2 pi f time - (pi / 2) phase_index)) E(t - time),   E(tau) = exp(-tau^2 / (2 sigma^2))

    as there.  ``bandwidth=0`` is the CW limit: every sample equals ``beam_pressure_field(...)[j, column]`` bit for bit.  The
    pulse arguments, their errors and the memory check are ``received_signal``'s; ``min_width``, ``curvature``, the weights
    and every other error are ``beam_arrivals``'.  A device-resident fan is processed where it is and stays device resident."""
    f0, rs, step, nt = _pulse(frequency, bandwidth, dt, n_times)
    f, cols, w, profile, boundary, counts = _beam_frame(rays, receiver_depths, env, min_width, range_indices, absorption,
                                                        bottom_loss, surface_loss, flatearth, "beam_received_signal")
    R, n = len(f.depths), len(cols)
    start = _per_column(t0, n, "t0", "start time")
    f.to_device(device)
    import torch
    _check_fits(f, R, n, nt, "signal", "samples")
    offsets, _, _, T, amp, qa = _device_beam_arrivals(f, cols, w, curvature, profile, boundary, counts, extra_bytes=8)
    T, I, qa = _sum_terms(T, amp, qa)
    tstart = f.upload(np.tile(start, R))
    re, im = (torch.empty((R, n, nt), dtype=torch.float64, device=f.dev) for _ in range(2))
    _lib.signal_device(f.env.device, offsets.data_ptr(), R * n, T.data_ptr(), I.data_ptr(), qa.data_ptr(), tstart.data_ptr(),
                       f0, rs, step, nt, re.data_ptr(), im.data_ptr(), f.stream)
    return _to_host(f, cols, re, im)


def beam_transfer_function(rays, receiver_depths, env, frequencies, min_width=10.0, curvature=True, range_indices=None,
                           absorption=None, bottom_loss=None, surface_loss=None, t_reduce=None, flatearth=True, device=0):
    """``transfer_function`` summed over the beam arrivals of ``beam_arrivals`` instead of the tube arrivals -> complex128
    ndarray ``(R, n, F)``, re 1 m; every arrival contributes

        H(f) += amplitude W(f) exp(i (2 pi f (time - t_reduce) - (pi / 2) phase_index))

    as there: with ``t_reduce=None`` and without a callable ``absorption`` (W = 1), ``H[j, c, k]`` is
    ``beam_pressure_field(..., frequencies[k])[j, column]`` bit for bit.  ``frequencies``, ``t_reduce``, ``absorption`` (a
    callable such as ``thorp_absorption`` makes the absorption follow the frequency), their errors and the memory check are
    ``transfer_function``'s; with a callable the arrival's path length L is the mean of its tube's two rays at the arrival's
    column.  ``min_width``, ``curvature``, the boundary weights and every other error are ``beam_arrivals``'.  A
    device-resident fan is processed where it is and stays device resident."""
    freq = _band(frequencies)
    F = len(freq)
    alpha = _band_absorption(absorption, freq) if callable(absorption) else None
    f, cols, w, profile, boundary, counts = _beam_frame(rays, receiver_depths, env, min_width, range_indices,
                                                        None if callable(absorption) else absorption, bottom_loss,
                                                        surface_loss, flatearth, "beam_transfer_function")
    R, n = len(f.depths), len(cols)
    reduce = _per_column(0.0 if t_reduce is None else t_reduce, n, "t_reduce", "reduction time")
    f.to_device(device)
    import torch
    _check_fits(f, R, n, F, "transfer function", "entries")
    # (I; with a callable also every arrival's group, column and tube as int64, the two edge lengths, their difference and
    # L_a, and the fan's (S, M) path lengths)
    offsets, tube, _, T, amp, qa = _device_beam_arrivals(f, cols, w, curvature, profile, boundary, counts,
                                                         extra_bytes=8 if alpha is None else 8 + 3 * 8 + 4 * 8,
                                                         fixed_bytes=0 if alpha is None else 8 * len(f.x) * len(f.rays))
    La = None
    if alpha is not None:
        La = _one_zero(f.dev)
        if len(tube):
            # the mean of the tube's two rays at the arrival's column: L_k + 0.5 (L_k+1 - L_k)
            La = _arrival_lengths(f, _arrival_columns(f, offsets, cols), tube, 0.5).contiguous()
    T, I, qa = _sum_terms(T, amp, qa)
    tred = f.upload(np.tile(reduce, R))
    re, im = (torch.empty((R, n, F), dtype=torch.float64, device=f.dev) for _ in range(2))
    _lib.spectrum_device(f.env.device, offsets.data_ptr(), R * n, T.data_ptr(), I.data_ptr(), qa.data_ptr(),
                         0 if La is None else La.data_ptr(), tred.data_ptr(), freq, alpha, re.data_ptr(), im.data_ptr(), f.stream)
    return _to_host(f, cols, re, im)


def beam_received_waveform(rays, receiver_depths, env, source, dt, carrier, t0, n_times=None, n_fft=None, min_width=10.0,
                           curvature=True, range_indices=None, absorption=None, bottom_loss=None, surface_loss=None,
                           flatearth=True, device=0):
    """``received_waveform`` synthesised from ``beam_transfer_function`` instead of ``transfer_function``: the signal a
    receiver records when the source sends the complex baseband envelope ``source`` on the carrier ``carrier`` -> complex128
    ndarray ``(R, n, n_times)``.  The same three lines of synthesis, circular with the period ``n_fft * dt``; for a Gaussian
    ``source`` centred at the emission time tc, u(t) is ``beam_received_signal``'s value at t - tc.  ``source``, ``dt``,
    ``carrier``, ``t0``, ``n_times``, ``n_fft`` and their errors are ``received_waveform``'s, every other argument and error
    ``beam_transfer_function``'s."""
    return _synthesise(lambda freq, start: beam_transfer_function(rays, receiver_depths, env, freq, min_width=min_width,
                                                                  curvature=curvature, range_indices=range_indices,
                                                                  absorption=absorption, bottom_loss=bottom_loss,
                                                                  surface_loss=surface_loss, t_reduce=start,
                                                                  flatearth=flatearth, device=device),
                       source, dt, carrier, t0, n_times, n_fft)


__all__ = ["beam_arrivals", "BeamArrivals", "beam_received_signal", "beam_transfer_function", "beam_received_waveform"]
