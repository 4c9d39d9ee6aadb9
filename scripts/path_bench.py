"""The tube products and the path integral on the headline fan: Munk, 1e5 launch angles, 1000 km,
S = 1001, device resident, 1000 receiver depths.  After a warm-up round, REPS rounds of transmission_loss,
beam_transmission_loss and arrivals (last column) -- with --absorption DB_PER_KM the weighted calls and path_loss as well.
Meant to run under `rocprofv3 --kernel-trace --stats -- python scripts/path_bench.py ...`, one process per variant, so that
the weighted and the unweighted launches of a kernel land in separate stats files; prints the wall clock of each call.
--root <checkout>: measure that checkout's package (the parent commit's, without --absorption) with the same script."""
import argparse
import json
import os
import sys
import time

ap = argparse.ArgumentParser()
ap.add_argument("--root", default=os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
ap.add_argument("--absorption", type=float, default=None, help="dB/km; default: the unweighted calls")
ap.add_argument("--rays", type=int, default=100_000)
ap.add_argument("--reps", type=int, default=5)
args = ap.parse_args()
sys.path.insert(0, os.path.abspath(args.root))
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
                    device_resident=True)
depths = np.linspace(0.0, 5000.0, 1000)
kw = {} if args.absorption is None else {"absorption": args.absorption}
calls = {"transmission_loss": lambda: pr.transmission_loss(fan, depths, env, flatearth=False, intensity=True, **kw),
         "beam_transmission_loss": lambda: pr.beam_transmission_loss(fan, depths, env, flatearth=False, intensity=True, **kw),
         "arrivals": lambda: pr.arrivals(fan, depths, env, flatearth=False, **kw)}
if args.absorption is not None:
    calls["path_loss_last_column"] = lambda: pr.path_loss(fan, env, args.absorption, flatearth=False, range_indices=[-1])
wall = {k: [] for k in calls}
for rep in range(args.reps + 1):
    for k, f in calls.items():
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        f()
        torch.cuda.synchronize()
        if rep:
            wall[k].append(1e3 * (time.perf_counter() - t0))
assert fan.device_resident
print(json.dumps({"rays": len(fan), "absorption_db_per_km": args.absorption, "reps": args.reps, "build": _lib.build_info(),
                  "device_code_sha256": _lib.device_code_sha256(),
                  "wall_ms_median": {k: float(np.median(v)) for k, v in wall.items()}}))
