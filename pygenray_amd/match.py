"""``matched_field``: matched-field processing on a vertical array -- the Bartlett ambiguity surface of the array's measured
snapshot over a range-depth grid of candidate source positions -- and its Gaussian-beam twin ``beam_matched_field`` (DESIGN.md,
"Matched-field processing").

No reference counterpart: pygenray gives back rays, not amplitudes.  The replica of element j for a candidate cell is
``transfer_function``'s H of the fan shot FROM the element, read at the cell (reciprocity; see ``matched_field``), term for term.
No replica is stored: the kernel that forms H_j at every frequency folds it with the data over the elements and reduces it over
the band where it stands (csrc/pgr_match.h), so a map costs its own (R, n) values of memory, not N (R, n, F).  The fans, their
arrivals and the sum stay on the device -- in HBM for device-resident fans, uploaded through torch for host fans.  There is no
CPU path.
"""
import math

import numpy as np

from . import _lib
from ._fan_frame import (_arrival_columns, _arrival_lengths, _arrival_terms, _band, _band_absorption, _check_fits,
                         _coherent_frame, _lag_spec, _one_zero, _ptr)
from .band import _band_weights
from .beam_arrivals import _beam_frame, _device_beam_arrivals, _sum_terms
from .ray_objects import RayFan, _columns


def _snapshot(fans, data, frequencies, weights, normalize):
    """What both products refuse of the array's side without a GPU -> (fans as a list, freq, the kernel's weights wf, data
    complex128 (N, F)): with `normalize` wf[k] = w_k / sum_j |d_jk|^2"""
    freq = _band(frequencies)
    w = _band_weights(weights, len(freq))
    fans = list(fans) if isinstance(fans, (list, tuple)) else None
    if not fans or not all(isinstance(f, RayFan) for f in fans):
        raise ValueError("fans must be a non-empty sequence of RayFans, one shot from each array element")
    d = np.asarray(data)
    if d.shape != (len(fans), len(freq)) or d.dtype.kind not in "fciu":
        raise ValueError(f"data must be complex of the shape (elements, frequencies) = ({len(fans)}, {len(freq)})")
    d = np.ascontiguousarray(d, dtype=np.complex128)
    if not np.all(np.isfinite(d.real)) or not np.all(np.isfinite(d.imag)):
        raise ValueError("data must be finite")
    if normalize:
        e = (d.real * d.real + d.imag * d.imag).sum(axis=0)
        if np.any((w > 0) & (e == 0)):
            raise ValueError("data vanishes at a frequency with a positive weight: the normalised processor divides by "
                             "sum_j |d_jk|^2 there (give that frequency the weight 0, or normalize=False)")
        with np.errstate(over="ignore"):
            w = np.where(w > 0, w / np.where(e > 0, e, 1.0), 0.0)
        if not np.all(np.isfinite(w)):
            raise ValueError("weights / sum_j |d_jk|^2 overflows: scale the data")
    return fans, freq, np.ascontiguousarray(w), d


def _same_grid(frames):
    x = frames[0].x
    for f in frames[1:]:
        if not np.array_equal(np.asarray(f.x), np.asarray(x)):
            raise ValueError("the fans must share one save grid: the x of every fan must equal that of the first")


def _joined(lists, dev, n_groups):
    """The element fans' arrival lists [(offsets, T, I, q, phi or None, L or None), ...] (each on the device, a fan without
    arrivals holding one zero per array) concatenated element-major -> the same six, the offsets of fan j shifted by the
    arrivals before it.  ``ValueError`` naming the arrivals' count when the copy does not fit in free memory."""
    import torch
    counts = [int(o[-1].item()) for o, *_ in lists]
    total = sum(counts)
    has_phi, has_L = lists[0][4] is not None, lists[0][5] is not None
    need = (8 + 8 + 4 + 8 * has_phi + 8 * has_L) * total + 8 * (len(lists) * n_groups + 1)
    free = torch.cuda.mem_get_info(dev)[0]
    if need > free:
        raise ValueError(f"the {total} arrivals of the {len(lists)} fans need {need} bytes of device memory and {free} are free: "
                         "ask for fewer depths or columns per call")
    shift = np.concatenate([[0], np.cumsum(counts)])
    offsets = torch.cat([lists[0][0]] + [o[1:] + int(s) for (o, *_), s in zip(lists[1:], shift[1:])])

    def cat(i, dtype=None):
        if lists[0][i] is None:
            return None
        return torch.cat([l[i][:c] for l, c in zip(lists, counts)]) if total else _one_zero(dev, dtype)
    return offsets, cat(1), cat(2), cat(3, torch.int32), cat(4), cat(5)


def _bartlett(f, cols, lists, freq, alpha, wf, data, normalize):
    """pgr_matched_field_device over the element fans' lists on the grid of the frame `f` -> float64 (R, n) on the host, the
    source's own columns NaN"""
    import torch
    R, n = len(f.depths), len(cols)
    offsets, T, I, qa, phi, La = _joined(lists, f.dev, R * n)
    out = torch.empty((R, n), dtype=torch.float64, device=f.dev)
    _lib.matched_field_sum(f.env.device, offsets.data_ptr(), len(lists), R * n, T.data_ptr(), I.data_ptr(), qa.data_ptr(),
                           _ptr(phi), _ptr(La), freq, alpha, wf, data, normalize, out.data_ptr(), f.stream)
    at_source = np.flatnonzero(np.abs(np.asarray(f.x)[cols] - f.x[0]) == 0)
    if len(at_source):                                                # the elements' own column, as pressure_field has it
        out.index_fill_(1, torch.from_numpy(at_source).to(f.dev), math.nan)
    return out.cpu().numpy()


def matched_field(fans, data, candidate_depths, env, frequencies, weights=None, range_indices=None, normalize=True,
                  absorption=None, bottom_loss=None, surface_loss=None, flatearth=True, device=0):
    """Where is the source?  The Bartlett ambiguity surface of the snapshot ``data`` of an N-element vertical array over the
    candidate source positions ``candidate_depths`` (metres, positive down, strictly ascending) x the save columns
    ``range_indices`` (default ``[S - 1]``) -> float64 ndarray ``(R, n)``; the source is read off its peak.

    ``fans``: a non-empty sequence of N ``RayFan``s from ``shoot_rays``, fan j shot FROM the depth of array element j, all on
    one save grid x (``ValueError`` otherwise); ``data``: complex ``(N, F)``, finite, d[j, k] the element's measured pressure
    at ``frequencies[k]`` (Hz; a non-empty 1-D sequence, finite, >= 0) in ``pressure_field``'s sign convention.  The replica
    of element j for a source in cell (depth, column) is H_j = ``transfer_function(fans[j], candidate_depths, ...)`` at that
    cell -- the modelling premise is reciprocity: the field at the element of a source at the cell is taken to be the field at
    the cell of a source at the element.  That is exact in an isovelocity medium.  In a range-independent stratified one the
    continuous ray-tube intensity is still symmetric -- the factor c(receiver) cos(theta_source) / (c(source)
    cos(theta_receiver)) it carries is 1 by Snell's law and the two spreading terms are equal -- so what
    differs between the two directions is the discretisation into tubes (which tubes fold, the top hat, a caustic's
    neighbourhood) and anything range-dependent; a factor per cell and frequency common to all elements drops out of the
    normalised processor.  With ``weights`` w (None: 1 / F each; else ``band_intensity``'s rules)

        normalize=True:   sum_k w_k |sum_j conj(H_jk) d_jk|^2 / (sum_j |H_jk|^2  sum_j |d_jk|^2)
        normalize=False:  sum_k w_k |sum_j conj(H_jk) d_jk|^2

    The first is the broadband Bartlett power, the mean over the band of |w^H d|^2 / (|w|^2 |d|^2): with sum w = 1 it lies in
    [0, 1] and is 1 where the replicas are the data up to a factor per frequency; a frequency with positive weight whose data
    vanish is refused there.  A cell no fan reaches is 0.  Every H_jk is ``transfer_function``'s, term for term and in its
    order, and the sums over j and k run in a fixed order (section 24).  No replica is stored: the map needs ``(R, n)`` values
    of device memory whatever N and F, beside the arrival lists.  A requested column with r = 0 is NaN.

    ``absorption`` (a callable such as ``thorp_absorption`` makes it follow the frequency), ``bottom_loss`` (a
    ``BottomReflection`` also turns every arrival by its bottom bounces' phase), ``surface_loss``, the frame and every other
    error are ``transfer_function``'s, fan by fan.  ``ValueError`` when the output, or the fans' arrival lists joined into one,
    do not fit in the free device memory, before the processor's kernel runs.  Device-resident fans are processed where they
    are and stay device resident."""
    fans, freq, wf, d = _snapshot(fans, data, frequencies, weights, normalize)
    alpha = _band_absorption(absorption, freq) if callable(absorption) else None
    frames = [_coherent_frame(fan, candidate_depths, env, None if callable(absorption) else absorption, bottom_loss,
                              surface_loss, flatearth, "matched_field") for fan in fans]
    _same_grid([fr[0] for fr in frames])
    cols = _columns(range_indices, len(frames[0][0].x))
    lag = _lag_spec(bottom_loss)
    lists = []
    for f, profile, boundary, counts in frames:
        f.to_device(device)
        if not lists:
            _check_fits(f, len(f.depths), len(cols), 1, "ambiguity surface", "values", kind="real")
        offsets, tube, w, T, I, qa, col, *phi = _arrival_terms(f, cols, profile, boundary, counts, lag)
        La = None
        if alpha is not None:
            La = _arrival_lengths(f, col, tube, w) if len(tube) else _one_zero(f.dev)
        lists.append((offsets, T, I, qa, phi[0] if phi else None, La))
    return _bartlett(frames[0][0], cols, lists, freq, alpha, wf, d, bool(normalize))


def beam_matched_field(fans, data, candidate_depths, env, frequencies, weights=None, min_width=10.0, curvature=True,
                       range_indices=None, normalize=True, absorption=None, bottom_loss=None, surface_loss=None, flatearth=True,
                       device=0):
    """``matched_field`` with the replicas summed over the beam arrivals of ``beam_arrivals`` instead of the tube arrivals ->
    float64 ndarray ``(R, n)``: H_j = ``beam_transfer_function(fans[j], candidate_depths, ...)``, term for term, under the
    same reciprocity premise.  ``fans``, ``data``, ``frequencies``, ``weights``, ``normalize`` and their errors are
    ``matched_field``'s; ``min_width``, ``curvature``, ``absorption`` (with a callable the arrival's path length is the mean of
    its tube's two rays), the boundary weights, the memory check by the arrivals' count and every other error are
    ``beam_transfer_function``'s (a ``BottomReflection`` as ``bottom_loss`` is refused).  Device-resident fans are processed
    where they are and stay device resident."""
    fans, freq, wf, d = _snapshot(fans, data, frequencies, weights, normalize)
    alpha = _band_absorption(absorption, freq) if callable(absorption) else None
    frames = [_beam_frame(fan, candidate_depths, env, min_width, range_indices, None if callable(absorption) else absorption,
                          bottom_loss, surface_loss, flatearth, "beam_matched_field") for fan in fans]
    _same_grid([fr[0] for fr in frames])
    lists = []
    for f, cols, width, profile, boundary, counts in frames:
        f.to_device(device)
        if not lists:
            _check_fits(f, len(f.depths), len(cols), 1, "ambiguity surface", "values", kind="real")
        # (what beam_band_intensity forms of the arrivals behind the emit pass, and their copy into the joined lists)
        offsets, tube, _, T, amp, qa = _device_beam_arrivals(
            f, cols, width, curvature, profile, boundary, counts,
            extra_bytes=8 + 20 if alpha is None else 8 + 28 + 3 * 8 + 4 * 8,
            fixed_bytes=0 if alpha is None else 8 * len(f.x) * len(f.rays))
        La = None
        if alpha is not None:
            La = _one_zero(f.dev)
            if len(tube):
                La = _arrival_lengths(f, _arrival_columns(f, offsets, cols), tube, 0.5).contiguous()
        T, I, qa = _sum_terms(T, amp, qa)
        lists.append((offsets, T, I, qa, None, La))
    f, cols = frames[0][0], frames[0][1]
    return _bartlett(f, cols, lists, freq, alpha, wf, d, bool(normalize))


__all__ = ["matched_field", "beam_matched_field"]
