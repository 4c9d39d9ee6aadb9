"""Matched-field processing on section 23's Munk set-up: one fan of 1e5 launch angles to 1000 km, S = 1001,
device resident with a bounce log of 64 slots, from each of 8 array elements (900 ... 1250 m every 50 m); 500 candidate depths over
0 ... 5000 m, 8 save columns, 64 frequencies over 60 ... 90 Hz, uniform weights.  After a warm-up round, 2 REPS rounds of
matched_field (pgr_mfp_sum behind the arrival kernels) and, in the same process and on the same arrival lists, of what it
replaces: transfer_function per element (N launches of pgr_spec_sum), the copies to the host and the Bartlett reduction in
NumPy; the two take turns at going first in a round.  Meant to run under
`rocprofv3 --kernel-trace --stats -- python scripts/match_bench.py`, in a run of its own without counters, so that the kernels of
the calls land in the stats files; without the profiler it prints the wall clock of each call.  It also records, with no
assertion, the size of the reciprocity premise in this refracting medium: the Bartlett power at the true cell when the data come
from a forward fan shot at the source and the replicas from the element fans."""
import argparse
import json
import os
import sys
import time

ap = argparse.ArgumentParser()
ap.add_argument("--rays", type=int, default=100_000)
ap.add_argument("--reps", type=int, default=3)
ap.add_argument("--elements", type=int, default=8)
ap.add_argument("--depths", type=int, default=500)
ap.add_argument("--columns", type=int, default=8)
ap.add_argument("--frequencies", type=int, default=64)
args = ap.parse_args()
sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import numpy as np  # noqa: E402
import torch  # noqa: E402
import pygenray_amd as pr  # noqa: E402
from pygenray_amd import _lib  # noqa: E402

S = 1001
z = np.arange(0, 6000, 1.0)
r = np.linspace(0, 1000e3, 100)
env = pr.OceanEnvironment2D(pr.DataArray(np.tile(pr.munk_ssp(z), (100, 1)), dims=["range", "depth"],
                                         coords={"range": r, "depth": z}),
                            pr.DataArray(np.full(100, 5000.0), dims=["range"], coords={"range": r}), flat_earth_transform=False)
angles = np.linspace(-20, 20, args.rays)


def shoot(depth):
    return pr.shoot_rays(depth, 0.0, angles, 1000e3, S, env, flatearth=False, debug=False, device_resident=True, max_bounces=64)


element_depths = 900.0 + 50.0 * np.arange(args.elements)
fans = [shoot(zj) for zj in element_depths]
depths = np.linspace(0.0, 5000.0, args.depths)
cols = np.linspace(S // args.columns, S - 1, args.columns).astype(int)
freq = np.linspace(60.0, 90.0, args.frequencies)
w = np.full(len(freq), 1.0 / len(freq))
rng = np.random.default_rng(0)
data = rng.normal(size=(args.elements, len(freq))) + 1j * rng.normal(size=(args.elements, len(freq)))


def bartlett(Hs, d):
    """the normalised processor in NumPy's own order on stored replicas Hs (N, R, n, F)"""
    num = np.abs((np.conj(Hs) * d[:, None, None, :]).sum(axis=0)) ** 2
    nn = (Hs.real * Hs.real + Hs.imag * Hs.imag).sum(axis=0)
    e = (np.abs(d) ** 2).sum(axis=0)
    with np.errstate(invalid="ignore", divide="ignore"):
        return (np.where(nn > 0, num / nn, 0.0) * (w / e)).sum(axis=-1)


walls = {"matched_field": [], "transfer_functions_and_numpy": []}
by_place = {(name, place): [] for name in walls for place in ("first", "second")}
worst = 0.0
for rep in range(2 * args.reps + 1):
    out = {}
    # (the two take turns at going first: the first call of a round follows the host's work on the round before)
    for place, name in zip(("first", "second"), list(walls)[::-1 if rep % 2 else 1]):
        torch.cuda.synchronize()
        t = time.perf_counter()
        if name == "matched_field":
            out[name] = pr.matched_field(fans, data, depths, env, freq, range_indices=cols, flatearth=False)
        else:
            Hs = np.stack([pr.transfer_function(fan, depths, env, freq, range_indices=cols, flatearth=False) for fan in fans])
            out[name] = bartlett(Hs, data)
            del Hs
        torch.cuda.synchronize()
        if rep:
            walls[name].append(1e3 * (time.perf_counter() - t))
            by_place[name, place].append(walls[name][-1])
    P, Q = out["matched_field"], out["transfer_functions_and_numpy"]
    lit = Q > 0
    worst = max(worst, float(np.abs(P - Q)[lit].max()))                 # (the two sum in different orders: roundings only)

# the reciprocity premise: a source in a cell seen by the array through a FORWARD fan, matched against the element fans' replicas
true = (args.depths // 5, args.columns // 2)
forward = shoot(float(depths[true[0]]))
seen = pr.transfer_function(forward, element_depths, env, freq, range_indices=[cols[true[1]]], flatearth=False)[:, 0, :]
heard = np.abs(seen).sum(axis=0) > 0
B = pr.matched_field(fans, seen[:, heard], depths, env, freq[heard], range_indices=cols, flatearth=False)
peak = np.unravel_index(np.nanargmax(B), B.shape)
n_arrivals = [len(pr.arrivals(fan, depths, env, flatearth=False, range_indices=cols)) for fan in fans]
assert all(fan.device_resident for fan in fans)
print(json.dumps({"rays": len(fans[0]), "elements": args.elements, "depths": args.depths, "columns": args.columns,
                  "frequencies": args.frequencies, "reps": args.reps, "arrivals": n_arrivals,
                  "cells": args.depths * args.columns, "bytes_surface": 8 * args.depths * args.columns,
                  "bytes_replicas": 16 * args.elements * args.depths * args.columns * args.frequencies,
                  "fraction_lit": float(lit.mean()), "worst_difference": worst,
                  "reciprocity": {"true_depth_m": float(depths[true[0]]), "true_range_m": float(fans[0].rs[0][cols[true[1]]]),
                                  "frequencies_heard": int(heard.sum()), "bartlett_at_true_cell": float(B[true]),
                                  "peak_depth_m": float(depths[peak[0]]), "peak_column": int(peak[1]),
                                  "bartlett_at_peak": float(B[peak])},
                  "build": _lib.build_info(), "device_code_sha256": _lib.device_code_sha256(),
                  **{k + "_wall_ms": v for k, v in walls.items()},
                  **{k + "_wall_ms_median": float(np.median(v)) for k, v in walls.items()},
                  **{f"{k}_wall_ms_when_{place}": v for (k, place), v in by_place.items()}}))
