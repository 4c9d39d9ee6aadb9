"""Test helpers for arrivals (not a product path): a plain NumPy restatement of the ray-tube arrivals of DESIGN.md
("Arrivals") on top of tl_reference's tube definition, the sequential per-(receiver, column) sum that must give the TL
intensity, and the closed-form travel time of a linear sound-speed gradient."""
import math

import numpy as np

import tl_reference as tlr
from pygenray_amd.environment import _mirror_envi_arrays, _unpack_envi
from pygenray_amd.host_physics import bilinear_interp
from pygenray_amd.launch_rays import _initial_slowness


def tube_arrivals(zs, ps, ts, x, p0, depths, cols, cin, rin, zin):
    """The definition, restated: zs / ps / ts (M, S) stored convention (depth = -z), x (S,) save ranges in the frame of the
    tables, p0 (M,), receiver depths (R,), columns cols (n,) -> dict(offsets, tube, w, T, p, I), grouped by receiver, then
    by requested column (in the order given), then by increasing tube.  The tubes, their validity, [lo, hi) and I are
    tl_reference.tube_intensity's, operation for operation."""
    zs, ps, ts = (np.asarray(a, dtype=float) for a in (zs, ps, ts))
    depths = np.asarray(depths, dtype=float)
    cols = np.asarray(cols, dtype=np.int64)
    M, S = zs.shape
    R, n = len(depths), len(cols)
    d = -zs
    c = tlr.bilinear(np.broadcast_to(x, (M, S)), d, rin, zin, cin)
    pc = ps * c
    ok = np.abs(pc) < 1
    g = np.full((M, S), np.nan)
    with np.errstate(invalid="ignore"):
        g[ok] = c[ok] / np.sqrt(1 - pc[ok] * pc[ok])
    r = np.abs(np.asarray(x, dtype=float) - x[0])
    keys, fields = [], []
    with np.errstate(invalid="ignore", divide="ignore", over="ignore"):
        for slot, s in enumerate(cols):
            if r[s] == 0:
                continue
            d0, d1 = d[:-1, s], d[1:, s]
            valid = ~np.isnan(g[:-1, s]) & ~np.isnan(g[1:, s]) & (d0 != d1)
            lo, hi = np.fmin(d0, d1), np.fmax(d0, d1)
            Ik = 0.5 * (g[:-1, s] + g[1:, s]) * np.abs(p0[1:] - p0[:-1]) / (r[s] * np.abs(d1 - d0))
            hit = valid[None, :] & (lo[None, :] <= depths[:, None]) & (depths[:, None] < hi[None, :])
            j, k = np.nonzero(hit)
            w = (depths[j] - d0[k]) / (d1[k] - d0[k])
            T = ts[k, s] + w * (ts[k + 1, s] - ts[k, s])
            p = ps[k, s] + w * (ps[k + 1, s] - ps[k, s])
            keys.append((j, np.full(len(j), slot), k))
            fields.append((k, w, T, p, Ik[k]))
    if keys:
        j, sl, k = (np.concatenate([kk[i] for kk in keys]) for i in range(3))
        f = [np.concatenate([ff[i] for ff in fields]) for i in range(5)]
        order = np.lexsort((k, sl, j))
        tube, w, T, p, I = (a[order] for a in f)
        counts = np.bincount(j * n + sl, minlength=R * n)
    else:
        tube, w, T, p, I = np.zeros(0, np.int64), *(np.zeros(0) for _ in range(4))
        counts = np.zeros(R * n, np.int64)
    offsets = np.concatenate([[0], np.cumsum(counts)])
    return dict(offsets=offsets, tube=tube.astype(np.int32), w=w, T=T, p=p, I=I)


def fan_arrivals(rays, depths, environment, cols, flatearth=True):
    """tube_arrivals of a host fan, prepared as tl_reference.fan_intensity prepares tube_intensity."""
    x = np.asarray(rays.rs, dtype=float)[0]
    cin, cpin, rin, zin, bd, br, ba = _unpack_envi(environment, flatearth=flatearth)
    if len(x) > 1 and x[-1] < x[0]:
        cin, cpin, rin, bd, br, ba = _mirror_envi_arrays(cin, cpin, rin, bd, br, ba)
        x = -x
    c_source = bilinear_interp(x[0], float(rays.source_depths[0]), rin, zin, cin)
    p0 = _initial_slowness(rays.thetas, c_source)
    return tube_arrivals(rays.zs, rays.ps, rays.ts, x, p0, depths, cols, cin, rin, zin)


def sequential_sums(offsets, I):
    """For every (receiver, column) group, the sum of its intensities in arrival order starting from 0.0 -- one add at a
    time, as np.add.accumulate would (not np.sum's pairwise order) -> (len(offsets) - 1,)"""
    offsets = np.asarray(offsets)
    counts = np.diff(offsets)
    acc = np.zeros(len(counts))
    for m in range(int(counts.max()) if len(counts) else 0):
        g = np.nonzero(counts > m)[0]
        acc[g] = acc[g] + I[offsets[g] + m]
    return acc


def gradient_travel_time(r, theta0, z_s=tlr.GRADIENT_ZS, c_a=tlr.GRADIENT_CA, gamma=tlr.GRADIENT_GAMMA):
    """Travel time to range r of the ray launched at depth-down angle theta0 (radians) in c(z) = c_a + gamma z:
    dT = dr / (c cos theta) with sin theta(r) = sin theta0 - xi gamma r gives T = (atanh(sin theta0) - atanh(sin theta)) / gamma."""
    c_s = c_a + gamma * z_s
    s0 = np.sin(theta0)
    s = s0 - np.cos(theta0) / c_s * gamma * r
    return (np.arctanh(s0) - np.arctanh(s)) / gamma


def gradient_travel_time_quad(r, theta0, z_s=tlr.GRADIENT_ZS, c_a=tlr.GRADIENT_CA, gamma=tlr.GRADIENT_GAMMA):
    """The same by mpmath quadrature of dr / (c(z(r)) cos theta(r)) along the circular arc (tl_reference.linear_gradient_ray)."""
    import mpmath

    def f(q):
        z, k, _ = tlr.linear_gradient_ray(q, theta0, z_s, c_a, gamma, m=mpmath)
        return 1 / ((c_a + gamma * z) * k)
    return float(mpmath.quad(f, [0, r]))


def same(a, b):
    return np.array_equal(a, b, equal_nan=True)


def tube_time_bound(ps, zs, tube, s):
    """The a-posteriori bound |p_k+1 - p_k| |d_k+1 - d_k| / 2 on the linear interpolation of T across tube k at column s
    (dT/dd along the wavefront is the vertical slowness p, which varies monotonically by at most |dp| across the tube)."""
    ps, zs = np.asarray(ps), np.asarray(zs)
    return 0.5 * np.abs(ps[tube + 1, s] - ps[tube, s]) * np.abs(zs[tube + 1, s] - zs[tube, s])


def isovelocity_images(r, depth, source_depth, water_depth, max_angle_deg):
    """The paths of an isovelocity waveguide with perfectly reflecting boundaries from (0, source_depth) to (r, depth)
    whose launch angle lies inside +-max_angle_deg -> (path lengths, depth-down launch angles in degrees), by unfolding:
    the receiver's images lie at unfolded depths 2 m H +- depth."""
    tmax = math.tan(math.radians(max_angle_deg))
    nmax = int(math.ceil(tmax * r / (2 * water_depth))) + 2
    m = np.arange(-nmax, nmax + 1)
    u = np.concatenate([2 * m * water_depth + depth, 2 * m * water_depth - depth]) - source_depth
    u = u[np.abs(u) <= tmax * r]
    return np.sqrt(r * r + u * u), np.degrees(np.arctan2(u, r))
