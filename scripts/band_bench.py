"""Band-averaged intensity on the headline fan: Munk, 1e5 launch angles, 1000 km, S = 1001, device
resident with a bounce log of 64 slots; 500 depths over 0 ... 5000 m, 8 save columns, 256 frequencies over 60 ... 90 Hz, uniform
weights.  After a warm-up round, 2 REPS rounds of band_intensity (pgr_band_sum behind the arrival kernels) and, in the same
process and on the same arrival lists, of what it replaces: transfer_function (pgr_spec_sum), its copy to the host and the
reduction over frequency in NumPy; the two take turns at going first in a round.  Meant to run under
`rocprofv3 --kernel-trace --stats -- python scripts/band_bench.py`, in a run of its own without counters, so that the kernels of
the calls land in the stats files; without the profiler it prints the wall clock of each call."""
import argparse
import json
import os
import sys
import time

ap = argparse.ArgumentParser()
ap.add_argument("--rays", type=int, default=100_000)
ap.add_argument("--reps", type=int, default=3)
ap.add_argument("--depths", type=int, default=500)
ap.add_argument("--columns", type=int, default=8)
ap.add_argument("--frequencies", type=int, default=256)
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
fan = pr.shoot_rays(1000.0, 0.0, np.linspace(-20, 20, args.rays), 1000e3, S, env, flatearth=False, debug=False,
                    device_resident=True, max_bounces=64)
depths = np.linspace(0.0, 5000.0, args.depths)
cols = np.linspace(S // args.columns, S - 1, args.columns).astype(int)
freq = np.linspace(60.0, 90.0, args.frequencies)
w = np.full(len(freq), 1.0 / len(freq))
walls = {"band_intensity": [], "transfer_function_and_numpy": []}
by_place = {(name, place): [] for name in walls for place in ("first", "second")}
worst = 0.0
for rep in range(2 * args.reps + 1):
    out = {}
    # (the two take turns at going first: the first call of a round follows the host's work on the round before)
    for place, name in zip(("first", "second"), list(walls)[::-1 if rep % 2 else 1]):
        torch.cuda.synchronize()
        t = time.perf_counter()
        if name == "band_intensity":
            out[name] = pr.band_intensity(fan, depths, env, freq, range_indices=cols, flatearth=False)
        else:
            H = pr.transfer_function(fan, depths, env, freq, range_indices=cols, flatearth=False)
            out[name] = ((H.real * H.real + H.imag * H.imag) * w).sum(axis=2)
            del H
        torch.cuda.synchronize()
        if rep:
            walls[name].append(1e3 * (time.perf_counter() - t))
            by_place[name, place].append(walls[name][-1])
    P, Q = out["band_intensity"], out["transfer_function_and_numpy"]
    lit = Q > 0
    worst = max(worst, float((np.abs(P - Q)[lit] / Q[lit]).max()))      # (the two sum in different orders: roundings only)
n_arrivals = len(pr.arrivals(fan, depths, env, flatearth=False, range_indices=cols))
assert fan.device_resident
print(json.dumps({"rays": len(fan), "depths": args.depths, "columns": args.columns, "frequencies": args.frequencies,
                  "reps": args.reps, "arrivals": n_arrivals, "groups": args.depths * args.columns,
                  "bytes_band_output": 8 * args.depths * args.columns,
                  "bytes_transfer_function": 16 * args.depths * args.columns * args.frequencies,
                  "fraction_lit": float(lit.mean()), "worst_relative_difference": worst,
                  "build": _lib.build_info(), "device_code_sha256": _lib.device_code_sha256(),
                  **{k + "_wall_ms": v for k, v in walls.items()},
                  **{k + "_wall_ms_median": float(np.median(v)) for k, v in walls.items()},
                  **{f"{k}_wall_ms_when_{place}": v for (k, place), v in by_place.items()}}))
