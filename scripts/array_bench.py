"""The time-angle response of a vertical array on the headline fan: Munk, 1e5 launch angles, 1000 km,
S = 1001, device resident with a bounce log of 64 slots; 40 elements 10 m apart centred at 1000 m, 121 looks over +-15
degrees, the last save column, 2048 samples of 2 ms from 4 s before x / 1500 m/s, f = 75 Hz, B = 20 Hz.  After a warm-up round,
REPS rounds of array_response (pgr_bf_sum behind the arrival kernels) and, in the same process, of received_signal at the same
40 depths (pgr_sig_sum on the same 40 groups): B times the latter is what the beamformer is compared against.
Meant to run under `rocprofv3 --kernel-trace --stats -- python scripts/array_bench.py`, in a run of its own without counters, so
that the kernels of the calls land in the stats files; without the profiler it prints the wall clock of each call."""
import argparse
import json
import os
import sys
import time

ap = argparse.ArgumentParser()
ap.add_argument("--rays", type=int, default=100_000)
ap.add_argument("--reps", type=int, default=3)
ap.add_argument("--elements", type=int, default=40)
ap.add_argument("--looks", type=int, default=121)
ap.add_argument("--samples", type=int, default=2048)
ap.add_argument("--dt", type=float, default=2e-3)
ap.add_argument("--frequency", type=float, default=75.0)
ap.add_argument("--bandwidth", type=float, default=20.0)
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
depths = 1000.0 + 10.0 * (np.arange(args.elements) - 0.5 * (args.elements - 1))
looks = np.linspace(-15.0, 15.0, args.looks)
t0 = float(np.asarray(fan.rs[0])[-1]) / 1500.0 - 4.0
pulse = (args.frequency, args.bandwidth, t0, args.dt, args.samples)
walls, lit, n_arrivals = {"array_response": [], "received_signal": []}, None, None
for rep in range(args.reps + 1):
    for name in walls:
        torch.cuda.synchronize()
        t = time.perf_counter()
        if name == "array_response":
            y = pr.array_response(fan, depths, env, looks, *pulse, flatearth=False)
        else:
            y = pr.received_signal(fan, depths, env, *pulse, flatearth=False)
        torch.cuda.synchronize()
        if rep:
            walls[name].append(1e3 * (time.perf_counter() - t))
        if name == "array_response":
            lit = float((np.abs(y) > 0).mean())
        del y
n_arrivals = len(pr.arrivals(fan, depths, env, flatearth=False))
assert fan.device_resident
print(json.dumps({"rays": len(fan), "elements": args.elements, "looks": args.looks, "samples": args.samples, "dt": args.dt,
                  "reps": args.reps, "arrivals": n_arrivals, "bytes_written": args.looks * args.samples * 16,
                  "fraction_of_samples_lit": lit, "build": _lib.build_info(), "device_code_sha256": _lib.device_code_sha256(),
                  **{k + "_wall_ms": v for k, v in walls.items()},
                  **{k + "_wall_ms_median": float(np.median(v)) for k, v in walls.items()}}))
