"""Travel-time sensitivity kernel timings: an eigenray set and a 1e4-ray fan (Munk, 100 km, 1001
samples), each on the table's own grid (100 x 6000) and on a coarse 50 x 200 grid.  Wall time per call after a warm-up
call, the result left on the device (as_tensor=True) and the device synchronised behind every call."""
import os
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
import numpy as np  # noqa: E402
import torch  # noqa: E402
import pygenray_amd as pr  # noqa: E402

REPS = 3
z = np.arange(0, 6000, 1.0)
r = np.linspace(0, 200e3, 100)
env = pr.OceanEnvironment2D(pr.DataArray(np.tile(pr.munk_ssp(z), (100, 1)), dims=["range", "depth"],
                                         coords={"range": r, "depth": z}),
                            pr.DataArray(np.full(100, 5000.0), dims=["range"], coords={"range": r}), flat_earth_transform=False)
kw = dict(flatearth=False, debug=False)
fan = pr.shoot_rays(1000.0, 0.0, np.linspace(-14, 14, 10_000), 100e3, 1001, env, device_resident=True, **kw)
seed = pr.shoot_rays(1000.0, 0.0, np.linspace(-14, 14, 2000), 100e3, 1001, env, **kw)
eig = pr.find_eigenrays(seed, [800.0, 1500.0, 3000.0], 1000.0, 0.0, 100e3, 1001, env, ztol=1e-3, **kw)
n_eig = sum(len(v) for v in eig.launch_angles.values())
grids = {"default 100 x 6000": {}, "coarse 50 x 200": dict(ranges=np.linspace(0, 100e3, 50), depths=np.linspace(0, 5000, 200))}


def timed(label, f):
    f()
    torch.cuda.synchronize()
    ts = []
    for _ in range(REPS):
        t0 = time.perf_counter()
        out = f()
        torch.cuda.synchronize()
        ts.append(time.perf_counter() - t0)
        del out
    print(f"{label}: {1e3 * min(ts):.2f} ms min, {1e3 * np.median(ts):.2f} ms median of {REPS}", flush=True)


for name, g in grids.items():
    timed(f"eigenrays ({n_eig} rays), {name}", lambda: pr.travel_time_kernel(eig, env, flatearth=False, as_tensor=True, **g))
    timed(f"fan ({len(fan)} rays, device resident), {name}",
          lambda: pr.travel_time_kernel(fan, env, flatearth=False, as_tensor=True, max_bytes=64 << 30, **g))
