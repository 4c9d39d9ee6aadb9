"""Beam arrivals on the headline fan: the Munk fan of signal_bench.py and spectrum_bench.py -- 1e5 launch
angles, 1000 km, S = 1001, device resident with a bounce log of 64 slots, 1000 receiver depths, 8 save columns -- at min_width
15 m.  After a warm-up round, REPS rounds of beam_arrivals (pgr_gba_bounds, pgr_gba_count, pgr_gba_emit and the copy of the
list to the host) and of beam_pressure_field (pgr_gbc_sum over all S columns, for the count + emit time beside the sum's on the
same fan and receivers: divide its time by S / columns).  --products: every round also calls beam_received_signal (--samples of
2 ms from 4 s before x / 1500 m/s, 75 Hz, B = 20 Hz) and beam_transfer_function (--frequencies of 75 Hz +- 20 Hz, reduced by
x / 1500 m/s), whose sums are pgr_sig_sum and pgr_spec_sum over the beam list.
Meant to run under `rocprofv3 --kernel-trace --stats -- python scripts/beam_arrivals_bench.py`, in a run of its own without
counters, so that the kernels of the calls land in the stats files; prints the wall clock of each call and the arrivals per
receiver and column."""
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
ap.add_argument("--min-width", type=float, default=15.0)
ap.add_argument("--products", action="store_true", help="also beam_received_signal and beam_transfer_function")
ap.add_argument("--samples", type=int, default=4096)
ap.add_argument("--frequencies", type=int, default=4096)
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
x = np.asarray(fan.rs[0])[cols]
kw = dict(min_width=args.min_width, flatearth=False)
calls = {"beam_arrivals": lambda: pr.beam_arrivals(fan, depths, env, range_indices=cols, **kw),
         "beam_pressure_field": lambda: pr.beam_pressure_field(fan, depths, env, 75.0, **kw)}
if args.products:
    calls["beam_received_signal"] = lambda: pr.beam_received_signal(fan, depths, env, 75.0, 20.0, x / 1500.0 - 4.0, 2e-3,
                                                                    args.samples, range_indices=cols, **kw)
    calls["beam_transfer_function"] = lambda: pr.beam_transfer_function(fan, depths, env, np.linspace(55.0, 95.0, args.frequencies),
                                                                        range_indices=cols, t_reduce=x / 1500.0, **kw)
walls, per = {k: [] for k in calls}, None
for rep in range(args.reps + 1):
    for name, call in calls.items():
        torch.cuda.synchronize()
        t = time.perf_counter()
        out = call()
        torch.cuda.synchronize()
        if rep:
            walls[name].append(1e3 * (time.perf_counter() - t))
        if name == "beam_arrivals":
            per = np.diff(out.offsets)
        del out
assert fan.device_resident
print(json.dumps({"rays": len(fan), "depths": args.depths, "columns": [int(c) for c in cols], "min_width": args.min_width,
                  "reps": args.reps, "arrivals": int(per.sum()),
                  "arrivals_per_receiver_and_column": {"mean": float(per.mean()), "min": int(per.min()), "max": int(per.max())},
                  "samples": args.samples if args.products else None, "frequencies": args.frequencies if args.products else None,
                  "build": _lib.build_info(), "device_code_sha256": _lib.device_code_sha256(),
                  "wall_ms": walls, "wall_ms_median": {k: float(np.median(v)) for k, v in walls.items()}}))
