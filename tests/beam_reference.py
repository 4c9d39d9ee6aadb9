"""Test helpers for beam_transmission_loss (not a product path): a plain NumPy restatement of the Gaussian-beam sum of
DESIGN.md ("Gaussian beams") -- its exp, the bottom depths, the sum itself -- and each beam's truncated, folded mass inside
the water column, for the energy identity."""
import math

import numpy as np

import tl_reference as tlr
from pygenray_amd.environment import _mirror_envi_arrays, _unpack_envi
from pygenray_amd.host_physics import bilinear_interp, linear_interp
from pygenray_amd.launch_rays import _initial_slowness

SQRT_2PI = float.fromhex("0x1.40d931ff62706p+1")        # the double nearest sqrt(2 pi)
TRUNCATED_MASS = math.erf(2 * math.sqrt(2))              # a beam's mass inside 4 sigma
TRUNCATION_DB = -10 * math.log10(TRUNCATED_MASS)         # 2.75e-4 dB

_LOG2E = float.fromhex("0x1.71547652b82fep+0")
_LN2_HI = 6.93147180369123816490e-01                     # fdlibm's split of ln 2
_LN2_LO = 1.90821492927058770002e-10
_TAYLOR = [1.0 / math.factorial(n) for n in range(13, -1, -1)]


def gexp(y):
    """exp(y) for y in [-8, 0], the kernel's operations in the kernel's order (csrc/pgr_beams.h)."""
    y = np.asarray(y, dtype=float)
    k = np.rint(y * _LOG2E)
    r = (y - k * _LN2_HI) - k * _LN2_LO
    p = np.full_like(r, _TAYLOR[0])
    for c in _TAYLOR[1:]:
        p = p * r + c
    return np.ldexp(p, k.astype(np.int64))


def _fma(a, b, c):
    """a * b + c rounded once (Fraction -> float is correctly rounded)"""
    from fractions import Fraction
    return float(Fraction(a) * Fraction(b) + Fraction(c))


def gexp_contracted(y):
    """gexp of one y as the contracted library computes it: every a * b + c of gexp fused (-ffp-contract=fast-honor-pragmas)."""
    y = float(y)
    k = float(np.rint(y * _LOG2E))
    r = _fma(-k, _LN2_LO, _fma(-k, _LN2_HI, y))
    p = _TAYLOR[0]
    for c in _TAYLOR[1:]:
        p = _fma(p, r, c)
    return math.ldexp(p, int(k))


# the worst errors of gexp and gexp_contracted against exp on test_beam_tl_host.py's [-8, 0] sample set, in ulps of exp, as
# measured there (0.84 for the contracted one): tests/test_contracted_arith.py bounds the beams' values with them
GEXP_ULPS = 1.5
GEXP_CONTRACTED_ULPS = 0.84


def frame_tables(x, environment, flatearth=True):
    """The tables of the frame a fan with save ranges x was traced in -> (x in that frame, cin, rin, zin, depths,
    depth_ranges): mirrored, x -> -x, for a backwards fan."""
    x = np.asarray(x, dtype=float)
    cin, cpin, rin, zin, bd, br, ba = _unpack_envi(environment, flatearth=flatearth)
    if len(x) > 1 and x[-1] < x[0]:
        cin, cpin, rin, bd, br, ba = _mirror_envi_arrays(cin, cpin, rin, bd, br, ba)
        x = -x
    return x, cin, rin, zin, bd, br


def bottom_depths(xf, depths, depth_ranges):
    """The bottom depth at each save range xf (in the traced frame): host_physics.linear_interp of the bathymetry."""
    return np.array([linear_interp(float(v), depth_ranges, depths) for v in xf])


def _tubes(zs, ps, x, p0, cin, rin, zin, w_min):
    """Per tube (M-1, S): valid, m, sigma, E, A -- the kernel's operations in its order."""
    zs = np.asarray(zs, dtype=float)
    ps = np.asarray(ps, dtype=float)
    x = np.asarray(x, dtype=float)
    M, S = zs.shape
    d = -zs
    c = tlr.bilinear(np.broadcast_to(x, (M, S)), d, rin, zin, cin)
    pc = ps * c
    ok = np.abs(pc) < 1                                  # (False for NaN)
    g = np.full((M, S), np.nan)
    with np.errstate(invalid="ignore", divide="ignore", over="ignore"):
        g[ok] = c[ok] / np.sqrt(1 - pc[ok] * pc[ok])
        r = np.abs(x - x[0])
        valid = ~np.isnan(g[:-1]) & ~np.isnan(g[1:])
        E = 0.5 * (g[:-1] + g[1:]) * np.abs(p0[1:] - p0[:-1])[:, None] / r[None, :]
        D = np.full((M + 1, S), np.nan)
        D[1:-1] = np.abs(d[1:] - d[:-1])                 # D[i + 1] = |d_i+1 - d_i|; none beyond the fan's ends
        sigma = np.fmax(np.fmax(np.fmax(D[:-2], D[1:-1]), D[2:]), w_min)
        m = 0.5 * (d[:-1] + d[1:])
        A = E / (sigma * SQRT_2PI)
    return valid, m, sigma, E, A, r


def beam_intensity(zs, ps, x, p0, depths, cin, rin, zin, bottom, w_min, a_scale=None):
    """The definition, restated: zs / ps (M, S) stored convention (depth = -z), x (S,) save ranges in the frame of the tables,
    p0 (M,) launch slowness, bottom (S,) bottom depths in that frame -> I (len(depths), S).

    Per column, every (receiver, tube, centre) term the definition keeps is formed with the kernel's operations, then the
    terms of each receiver are added from 0.0 one at a time in (tube, centre) order."""
    depths = np.asarray(depths, dtype=float)
    bottom = np.asarray(bottom, dtype=float)
    valid, m, sigma, E, A, r = _tubes(zs, ps, x, p0, cin, rin, zin, w_min)
    if a_scale is not None:                              # (M-1, S): every term of tube k scaled (error bounds)
        A = A * a_scale
    R, S = len(depths), len(r)
    order = np.argsort(depths, kind="stable")
    ds = depths[order]
    out = np.zeros((R, S))
    with np.errstate(invalid="ignore", over="ignore"):
        for s in range(S):
            if r[s] == 0:
                out[:, s] = np.nan
                continue
            k = np.flatnonzero(valid[:, s])
            ms, sg, As = m[k, s], sigma[k, s], A[k, s]
            parts = []
            for which, ctr in enumerate((ms, -ms, 2.0 * bottom[s] - ms)):
                reach = sg * 4.001                       # candidates: a superset of the receivers within 4 sigma
                j0 = np.searchsorted(ds, ctr - reach, side="left")
                j1 = np.searchsorted(ds, ctr + reach, side="right")
                n = np.where(np.isnan(ctr), 0, j1 - j0)
                t = np.repeat(np.arange(len(k)), n)
                jj = np.repeat(j0, n) + (np.arange(n.sum()) - np.repeat(np.cumsum(n) - n, n))
                u = (ds[jj] - ctr[t]) / sg[t]
                v = u * u
                keep = v <= 16
                t, jj, v = t[keep], jj[keep], v[keep]
                parts.append((order[jj], k[t], np.full(len(t), which), As[t] * gexp(-0.5 * v)))
            j, kk, w, term = (np.concatenate(p) for p in zip(*parts))
            srt = np.lexsort((w, kk, j))                 # by receiver, then tube, then centre
            j, term = j[srt], term[srt]
            cnt = np.bincount(j, minlength=R)
            rank = np.arange(len(j)) - np.repeat(np.cumsum(cnt) - cnt, cnt)
            T = np.zeros((R, int(cnt.max()) if len(j) else 0))
            T[j, rank] = term
            acc = np.zeros(R)
            for q in range(T.shape[1]):
                acc = acc + T[:, q]                      # adding a 0.0 where a receiver has no more terms is exact
            out[:, s] = acc
    return out


def beam_masses(zs, ps, x, p0, cin, rin, zin, bottom, w_min):
    """Per tube (M-1, S): (E, mass) -- E the tube's depth-integrated intensity (0 where the tube adds nothing) and mass its
    beam's share inside [0, bottom], from math.erf: the beam and its two images, each cut at 4 sigma.  Integrated over the
    water column the beam intensity is sum_k E_k mass_k; mass = erf(2 sqrt 2) for a beam 4 sigma clear of both boundaries."""
    valid, m, sigma, E, A, r = _tubes(zs, ps, x, p0, cin, rin, zin, w_min)
    mass = np.zeros(m.shape)
    for k, s in zip(*np.nonzero(valid)):
        b, sg = float(bottom[s]), float(sigma[k, s])
        for ctr in (m[k, s], -m[k, s], 2 * b - m[k, s]):
            lo, hi = max(0.0, ctr - 4 * sg), min(b, ctr + 4 * sg)
            if hi > lo:
                mass[k, s] += 0.5 * (math.erf((hi - ctr) / (sg * math.sqrt(2))) - math.erf((lo - ctr) / (sg * math.sqrt(2))))
    return np.where(valid, E, 0.0), mass, sigma, A


def fan_beam_intensity(rays, depths, environment, w_min, flatearth=True):
    """beam_intensity of a host fan from shoot_rays, prepared the way the definition says: the tables and bathymetry of the
    frame the fan was traced in and p0 = sin(radians(theta)) / c_source."""
    xf, cin, rin, zin, bd, br = frame_tables(np.asarray(rays.rs, dtype=float)[0], environment, flatearth)
    c_source = bilinear_interp(xf[0], float(rays.source_depths[0]), rin, zin, cin)
    p0 = _initial_slowness(rays.thetas, c_source)
    return beam_intensity(rays.zs, rays.ps, xf, p0, depths, cin, rin, zin, bottom_depths(xf, bd, br), w_min)


def folded_fan(n_rays=20001, max_angle=80.0, ranges=np.linspace(0.0, 20e3, 201), zs=1000.0, H=5000.0, c0=1500.0):
    """Straight rays from (0, zs) folded at the surface and the bottom of an isovelocity waveguide: launch angles (deg) and
    stored-convention (M, S) zs / ps."""
    th = np.linspace(-max_angle, max_angle, n_rays)
    u = zs + ranges[None, :] * np.tan(np.radians(th))[:, None]          # unfolded depth
    w = np.mod(u, 2 * H)
    depth = np.where(w <= H, w, 2 * H - w)
    s = np.sin(np.radians(th))[:, None] / c0
    sign = np.where(np.mod(np.floor(u / H), 2) == 0, 1.0, -1.0)         # p flips at every reflection
    return th, -depth, -(s * sign)


def clear_of_the_aperture_edge(depths, ranges, n_rays, max_angle, source_depth, H, w_min):
    """(len(depths), len(ranges)) bool: the receivers of an isovelocity waveguide more than 4 beam widths from the fan's
    +-max_angle edge rays, folded into [0, H].  The image sum keeps an image or drops it there; the beams smooth that step
    over their width, so the image sum is no reference next to it.  The edge tube's width, r dtheta / cos^2(max_angle),
    counts half as much again for sigma's neighbouring tubes."""
    depths = np.asarray(depths, dtype=float)
    ranges = np.asarray(ranges, dtype=float)
    t = math.radians(max_angle)
    edge_width = ranges * math.radians(2 * max_angle / (n_rays - 1)) / math.cos(t) ** 2
    reach = 4 * np.maximum(w_min, 1.5 * edge_width)
    use = np.ones((len(depths), len(ranges)), bool)
    for sign in (1.0, -1.0):
        u = np.mod(source_depth + sign * ranges * math.tan(t), 2 * H)
        edge = np.where(u <= H, u, 2 * H - u)
        use &= np.abs(depths[:, None] - edge[None, :]) > reach[None, :]
    return use

