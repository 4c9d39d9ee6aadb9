"""Arrival-time histogram cases shared by the reference-mode and contracted-mode GPU tests (not a test module itself).

np.histogram places a value by its uniform-bin estimate, then corrects it against the np.linspace edges
RN(RN(j * step) + first).  A kernel that rounds an edge differently -- one fused multiply-add, RN(first + j * step) --
puts the values on that edge, or one ulp below it, one bin away.  So every case holds values on every edge and one ulp
either side, the range ends and their outer neighbours, NaN, and dropped rays on some edge values; and every range whose
step is inexact counts, in exact rationals, the edges where the two roundings differ, so that the case cannot pass
vacuously."""
from fractions import Fraction

import numpy as np

# (name, t_min, t_max, bins, at least this many edges where a fused edge differs from np.linspace's)
RANGES = [
    ("configs4", 1000e3 / 1560, 1000e3 / 1400, 4096, 50),     # BASELINE configs[4]'s window
    ("wide-max-bins", -3.7, 1e4 / 3, 16384, 50),               # a negative start, the most bins the kernel takes
    ("one-bin", 1000e3 / 1560, 1000e3 / 1400, 1, 0),           # (edges are the range ends: nothing to round)
    ("seven-bins", 0.1, 0.8, 7, 1),
    ("near-degenerate", 666.0, 666.0 + 96 * 2.0 ** -43, 64, 0),  # edges 1.5 ulp apart; j * step is exact here
]

DEGENERATE = (666.0, 666.0 + 1e-12, 4096)   # np.linspace's edges are not strictly increasing: np.histogram refuses it


def fused_edge_mismatches(t_min, t_max, bins):
    """How many interior edges j * step + first round differently when the product is not rounded first."""
    first, last = float(t_min), float(t_max)
    step = (last - first) / bins                                  # np.linspace: delta / div
    n = 0
    for j in range(1, bins):
        plain = (j * step) + first                                 # two roundings (Python floats do not contract)
        fused = float(Fraction(first) + j * Fraction(step))       # one rounding: Fraction -> float is correctly rounded
        n += plain != fused
    return n


def case_values(t_min, t_max, bins, seed=0):
    """(t, status): float64 times and int32 statuses for one range"""
    rng = np.random.default_rng(seed + bins)
    edges = np.linspace(t_min, t_max, bins + 1)
    parts = [edges, np.nextafter(edges, np.inf), np.nextafter(edges, -np.inf),
             np.nextafter(np.array([t_min]), -np.inf), np.nextafter(np.array([t_max]), np.inf),   # just outside
             np.array([t_min, t_max, np.nan, np.nan, np.inf, -np.inf]),
             rng.uniform(t_min, t_max, 4 * bins + 64)]
    t = np.concatenate(parts)
    st = np.zeros(len(t), np.int32)
    st[: 3 * (bins + 1)][::5] = rng.integers(1, 9, len(st[: 3 * (bins + 1)][::5]))   # dropped rays on edge values
    perm = rng.permutation(len(t))
    return t[perm], st[perm]


def numpy_counts(t, st, t_min, t_max, bins):
    keep = (st == 0) & ~np.isnan(t)
    return np.histogram(t[keep], bins=bins, range=(t_min, t_max))[0]


def check_device_histogram(t_min, t_max, bins, min_mismatches):
    """The device histogram of one range against np.histogram, count for count, read through a strided end[:, 0] view
    and through the packed 40-byte end records; says how many counts moved when they differ."""
    import torch
    from pygenray_amd.distributed import arrival_time_histogram
    assert fused_edge_mismatches(t_min, t_max, bins) >= min_mismatches
    t, st = case_values(t_min, t_max, bins)
    want = numpy_counts(t, st, t_min, t_max, bins)
    assert want.sum() > 3 * bins                                  # (the edge values were counted, not dropped)
    n = len(t)
    end = torch.zeros(n, 3, dtype=torch.float64, device="cuda")
    end[:, 0] = torch.from_numpy(t).cuda()
    std = torch.from_numpy(st).cuda()
    rec = torch.zeros(n, 5, dtype=torch.float64, device="cuda")
    rec[:, 0] = end[:, 0]
    rec.view(torch.int32).view(n, 10)[:, 8] = std
    for label, h in (("end[:, 0]", arrival_time_histogram(end[:, 0], std, bins, t_min, t_max)),
                     ("packed records", arrival_time_histogram(rec[:, 0], rec.view(torch.int32).view(n, 10)[:, 8], bins,
                                                               t_min, t_max))):
        got = h.cpu().numpy()
        moved = int(np.abs(got - want).sum()) // 2
        assert h.dtype == torch.int64 and np.array_equal(got, want), \
            f"{label}: {moved} counts moved, first bins {np.nonzero(got != want)[0][:8]}"
