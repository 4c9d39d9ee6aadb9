"""Time-front timings on the headline fan: Munk, 1e5 launch angles, 1000 km, S = 1001, device
resident.  Median of REPS timed repeats after a warm-up call:

  (a) turning_points() at the last column          (b) time_front(500)
  (c) turning_points(range(0, 1001, 10))           (d) compute_rayids(), wall clock, ps not yet fetched

(a) - (c): HIP events around the library call (pgr_fan_time_front, outputs allocated beforehand), and beside them the wall
clock of the Python call that ends with the result on the host.  (d) is the one figure a checkout without the feature has
too -- there it fetches the (M, S) block of ps: run this script with --root <that checkout> --out <file> and hand the file
to the run on this checkout as --parent <file>; both land in one JSON with their ratio."""
import argparse
import json
import os
import sys
import time

ap = argparse.ArgumentParser()
ap.add_argument("--root", default=os.path.dirname(os.path.dirname(os.path.abspath(__file__))),
                help="the checkout whose package is measured (default: this one)")
ap.add_argument("--out", default=None, help="JSON file to write (default: profiles/front_bench.json of this checkout)")
ap.add_argument("--parent", default=None, help="the JSON a run on the parent checkout wrote: its (d) is folded in")
ap.add_argument("--rays", type=int, default=100_000)
ap.add_argument("--reps", type=int, default=7)
args = ap.parse_args()
HERE = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.abspath(args.root))
import numpy as np  # noqa: E402
import torch  # noqa: E402
import pygenray_amd as pr  # noqa: E402
from pygenray_amd import _lib  # noqa: E402

REPS = max(5, args.reps)
S = 1001
z = np.arange(0, 6000, 1.0)
r = np.linspace(0, 1000e3, 100)
env = pr.OceanEnvironment2D(pr.DataArray(np.tile(pr.munk_ssp(z), (100, 1)), dims=["range", "depth"],
                                         coords={"range": r, "depth": z}),
                            pr.DataArray(np.full(100, 5000.0), dims=["range"], coords={"range": r}), flat_earth_transform=False)
fan = pr.shoot_rays(1000.0, 0.0, np.linspace(-20, 20, args.rays), 1000e3, S, env, flatearth=False, debug=False,
                    device_resident=True)
M = len(fan)
have = hasattr(fan, "turning_points")
res = {"workload": f"pr.shoot_rays(1000 m, 0, linspace(-20, 20, {args.rays}), 1000 km, {S}, Munk, flatearth=False, "
                   f"device_resident=True): {M} surviving rays", "reps": REPS, "feature": have,
       "package": "this checkout" if os.path.abspath(args.root) == HERE else "another checkout",
       "build": _lib.build_info(), "device_code_sha256": _lib.device_code_sha256()}


def median_ms(f):
    f()
    torch.cuda.synchronize()
    ts = []
    for _ in range(REPS):
        ts.append(f())
    return {"median_ms": float(np.median(ts)), "min_ms": float(np.min(ts)), "max_ms": float(np.max(ts))}


def wall(f):
    def run():
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        f()
        torch.cuda.synchronize()
        return 1e3 * (time.perf_counter() - t0)
    return run


def events(cols, samples):
    """HIP events around pgr_fan_time_front for `cols`, turns and (with `samples`) T, z, p asked for"""
    h = fan._dev
    dev = torch.device("cuda", h._env.device)
    n = len(cols)
    turns = torch.empty((n, M), dtype=torch.int32, device=dev)
    tzp = [torch.empty((n, M), dtype=torch.float64, device=dev) for _ in range(3 if samples else 0)]
    ptrs = [a.data_ptr() for a in tzp] or [0, 0, 0]
    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)

    def run():
        st = torch.cuda.current_stream(dev)
        e0.record(st)
        h.time_front(cols, *ptrs, turns.data_ptr(), st.cuda_stream)
        e1.record(st)
        e1.synchronize()
        return e0.elapsed_time(e1)
    return run


def rayids():
    fan.__dict__.pop("_ps", None)          # (a checkout without the feature fetched it: every repeat pays the same)
    fan._ray_ids = None
    fan.compute_rayids()


if have:
    every10 = list(range(0, S, 10))
    p_bytes = 8.0 * M
    for key, cols, samples, call in (
            ("a_turning_points_last", [S - 1], False, lambda: fan.turning_points()),
            ("b_time_front_500", [500], True, lambda: fan.time_front(500)),
            ("c_turning_points_every_10th", every10, False, lambda: fan.turning_points(every10))):
        res[key] = {"library_call_hip_events": median_ms(events(cols, samples)), "python_call_wall": median_ms(wall(call)),
                    "p_bytes_read_floor": p_bytes * (max(cols) + 1)}
        ev = res[key]["library_call_hip_events"]["median_ms"]
        res[key]["p_bytes_over_event_time_GBps"] = res[key]["p_bytes_read_floor"] / (ev * 1e-3) / 1e9
        print(f"{key}: library call {ev:.3f} ms (HIP events), Python call "
              f"{res[key]['python_call_wall']['median_ms']:.3f} ms wall, p read at "
              f"{res[key]['p_bytes_over_event_time_GBps']:.0f} GB/s", flush=True)
res["d_compute_rayids_wall"] = median_ms(wall(rayids))
print(f"d_compute_rayids_wall: {res['d_compute_rayids_wall']['median_ms']:.3f} ms "
      f"({'kernel count' if have else 'ps fetched over PCIe'})", flush=True)
if have:
    assert fan.device_resident and "_ps" not in fan.__dict__
if args.parent:
    with open(args.parent) as f:
        par = json.load(f)
    res["d_compute_rayids_wall_parent"] = par["d_compute_rayids_wall"]
    res["parent_device_code_sha256"] = par.get("device_code_sha256")
    res["d_ratio_parent_over_this"] = par["d_compute_rayids_wall"]["median_ms"] / res["d_compute_rayids_wall"]["median_ms"]
    print(f"d: parent {par['d_compute_rayids_wall']['median_ms']:.3f} ms / this "
          f"{res['d_compute_rayids_wall']['median_ms']:.3f} ms = {res['d_ratio_parent_over_this']:.2f}", flush=True)
out = args.out or os.path.join(HERE, "profiles", "front_bench.json")
os.makedirs(os.path.dirname(os.path.abspath(out)), exist_ok=True)
with open(out, "w") as f:
    json.dump(res, f, indent=1)
    f.write("\n")
print("wrote", out)
