"""The received signal of a Gaussian pulse on the headline fan: Munk, 1e5 launch angles, 1000 km,
S = 1001, device resident with a bounce log of 64 slots, 1000 receiver depths, 8 save columns, 4096 samples of 2 ms from 4 s
before x / 1500 m/s at each column, f = 75 Hz, B = 20 Hz.  After a warm-up call, REPS calls of received_signal (its bounce
counts, caustic scan, arrival count / scan / emit and the sum itself).
Meant to run under `rocprofv3 --kernel-trace --stats -- python scripts/signal_bench.py`, in a run of its own without counters,
so that the kernels of the calls land in the stats files; without the profiler it prints the wall clock of each call.
--halfspace: every round also calls received_signal with bottom_loss=fluid_halfspace(1700, 1800, 0.5)
(pgr_sig_sum_phi), in the same process as the rigid call (pgr_sig_sum)."""
import argparse
import json
import os
import sys
import time

ap = argparse.ArgumentParser()
ap.add_argument("--rays", type=int, default=100_000)
ap.add_argument("--reps", type=int, default=3)
ap.add_argument("--depths", type=int, default=1000)
ap.add_argument("--columns", type=int, default=8)
ap.add_argument("--samples", type=int, default=4096)
ap.add_argument("--dt", type=float, default=2e-3)
ap.add_argument("--frequency", type=float, default=75.0)
ap.add_argument("--bandwidth", type=float, default=20.0)
ap.add_argument("--halfspace", action="store_true")
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
fan = pr.shoot_rays(1000.0, 0.0, angles, 1000e3, S, env, flatearth=False, debug=False, device_resident=True, max_bounces=64)
depths = np.linspace(0.0, 5000.0, args.depths)
cols = np.linspace(S // args.columns, S - 1, args.columns).astype(int)
t0 = np.asarray(fan.rs[0])[cols] / 1500.0 - 4.0
variants = {"rigid": {}}
if args.halfspace:
    variants["halfspace"] = dict(bottom_loss=pr.fluid_halfspace(1700.0, 1800.0, 0.5))
walls, lit = {k: [] for k in variants}, None
for rep in range(args.reps + 1):
    for name, kw in variants.items():
        torch.cuda.synchronize()
        t = time.perf_counter()
        u = pr.received_signal(fan, depths, env, args.frequency, args.bandwidth, t0, args.dt, args.samples, range_indices=cols,
                               flatearth=False, **kw)
        torch.cuda.synchronize()
        if rep:
            walls[name].append(1e3 * (time.perf_counter() - t))
        if name == "rigid":
            lit = float((np.abs(u) > 0).mean())
        del u
wall = walls["rigid"]
assert fan.device_resident
print(json.dumps({"rays": len(fan), "depths": args.depths, "columns": [int(c) for c in cols], "samples": args.samples,
                  "dt": args.dt, "reps": args.reps, "bytes_written": args.depths * args.columns * args.samples * 16,
                  "fraction_of_samples_lit": lit, "build": _lib.build_info(), "device_code_sha256": _lib.device_code_sha256(),
                  "wall_ms": wall, "wall_ms_median": float(np.median(wall)),
                  **({"halfspace_wall_ms": walls["halfspace"], "halfspace_wall_ms_median": float(np.median(walls["halfspace"]))}
                     if args.halfspace else {})}))
