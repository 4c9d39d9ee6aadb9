"""The coherent tube sum beside the incoherent one on the headline fan: Munk, 1e5 launch angles,
1000 km, S = 1001, device resident with a bounce log, 1000 receiver depths.  After a warm-up round, REPS rounds of
transmission_loss and -- unless --tl-only -- pressure_field (its caustic scan and bounce counts included).
Meant to run under `rocprofv3 --kernel-trace --stats -- python scripts/coherent_bench.py ...`, one process per tree, so that
each tree's kernels land in their own stats files; prints the wall clock of each call.
--root <checkout> --tl-only: measure that checkout's package (the parent commit's) with the same script.
--halfspace: also pressure_field over a sand-like fluid half-space, once with its magnitude alone
(bottom_loss=<its .loss pair>: pgr_coh_sum with weights, one boundary post-pass) and once complex (bottom_loss=<the
BottomReflection>: pgr_coh_sum_phi, the post-pass run once more for the lags), in the same process as the rigid call.
--beams: also beam_transmission_loss (pgr_gb_sum) and beam_pressure_field (pgr_gbc_sum) at --min-width,
in the same process, so that the three sums' kernels come from one run; a checkout without beam_pressure_field (--root <the
parent's>) runs the other two."""
import argparse
import json
import os
import sys
import time

ap = argparse.ArgumentParser()
ap.add_argument("--root", default=os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
ap.add_argument("--tl-only", action="store_true", help="transmission_loss alone (a tree without pressure_field)")
ap.add_argument("--halfspace", action="store_true", help="also pressure_field with bottom_loss=fluid_halfspace(1700, 1800, 0.5)")
ap.add_argument("--beams", action="store_true", help="also beam_transmission_loss and (where the tree has it) beam_pressure_field")
ap.add_argument("--min-width", type=float, default=10.0)
ap.add_argument("--rays", type=int, default=100_000)
ap.add_argument("--reps", type=int, default=3)
ap.add_argument("--frequency", type=float, default=75.0)
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
angles = np.linspace(-20, 20, args.rays)
shoot = lambda **kw: pr.shoot_rays(1000.0, 0.0, angles, 1000e3, S, env, flatearth=False, debug=False,  # noqa: E731
                                   device_resident=True, **kw)
fan = shoot()
need = int((fan.n_botts + fan.n_surfs).max())          # the log's size: the most bounces of any ray
fan.release()
fan = shoot(max_bounces=max(need, 1))
depths = np.linspace(0.0, 5000.0, 1000)
calls = {"transmission_loss": lambda: pr.transmission_loss(fan, depths, env, flatearth=False, intensity=True)}
if not args.tl_only:
    calls["pressure_field"] = lambda: pr.pressure_field(fan, depths, env, args.frequency, flatearth=False)
if args.halfspace:
    sand = pr.fluid_halfspace(1700.0, 1800.0, 0.5)
    calls["pressure_field_bottom_loss"] = lambda: pr.pressure_field(fan, depths, env, args.frequency, flatearth=False,
                                                                    bottom_loss=sand.loss)
    calls["pressure_field_halfspace"] = lambda: pr.pressure_field(fan, depths, env, args.frequency, flatearth=False,
                                                                  bottom_loss=sand)
if args.beams:
    calls["beam_transmission_loss"] = lambda: pr.beam_transmission_loss(fan, depths, env, flatearth=False, intensity=True,
                                                                        min_width=args.min_width)
    if hasattr(pr, "beam_pressure_field"):
        calls["beam_pressure_field"] = lambda: pr.beam_pressure_field(fan, depths, env, args.frequency, flatearth=False,
                                                                      min_width=args.min_width)
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
print(json.dumps({"rays": len(fan), "max_bounces": need, "reps": args.reps, "build": _lib.build_info(),
                  "device_code_sha256": _lib.device_code_sha256(),
                  "wall_ms_median": {k: float(np.median(v)) for k, v in wall.items()}}))
