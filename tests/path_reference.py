"""Test helpers for path_length / path_loss and the absorption-weighted tube products (not a product path): a plain NumPy
restatement of the running path integral of DESIGN.md ("Path integrals and volume absorption"), written from the definition;
its exp and the weights 10^(-A / 10); and the restatements of the tube products (tl_reference, beam_reference,
arrivals_reference) fed the weighted g."""
import math

import numpy as np

import beam_reference as bref
import frame_independent as fi
import tl_reference as tlr

LN10_10 = float.fromhex("0x1.d791c5f888822p-3")         # the double nearest ln(10) / 10
W_CUT = -700.0                                           # below this argument the weight is 0

_LOG2E = float.fromhex("0x1.71547652b82fep+0")
_LN2_HI = 6.93147180369123816490e-01                     # fdlibm's split of ln 2
_LN2_LO = 1.90821492927058770002e-10
_TAYLOR = [1.0 / math.factorial(n) for n in range(13, -1, -1)]


def gexp(y):
    """exp(y), the kernel's operations in the kernel's order (csrc/pgr_beams.h), for finite y in [-700, 0] and a little
    beyond: y = k ln2 + r, the degree-13 Taylor polynomial of exp(r) in Horner form, scaled by 2^k."""
    y = np.asarray(y, dtype=float)
    k = np.rint(y * _LOG2E)
    r = (y - k * _LN2_HI) - k * _LN2_LO
    p = np.full_like(r, _TAYLOR[0])
    for c in _TAYLOR[1:]:
        p = p * r + c
    return np.ldexp(p, k.astype(np.int64))


def weights(A):
    """W = 10^(-A / 10) as the library defines it: gexp(-(A K)), 0.0 for an argument below -700, NaN for a NaN."""
    A = np.asarray(A, dtype=float)
    y = -(A * LN10_10)
    plain = ~np.isnan(y) & (y >= W_CUT)
    W = np.where(np.isnan(y), np.nan, 0.0)
    W[plain] = gexp(y[plain])
    return W


def alpha_at(d, a_depths, alpha):
    """The absorption profile at depths d: the constant for one node; else alpha[0] at and above the first node, alpha[-1] at
    and below the last, and alpha_j + w (alpha_j+1 - alpha_j) in cell j = searchsorted(side="right") - 1, clamped; NaN for
    a NaN depth."""
    d = np.asarray(d, dtype=float)
    alpha = np.asarray(alpha, dtype=float)
    if len(alpha) == 1:
        return np.full(d.shape, alpha[0])
    a_depths = np.asarray(a_depths, dtype=float)
    j = np.clip(np.searchsorted(a_depths, d, side="right") - 1, 0, len(a_depths) - 2)
    with np.errstate(invalid="ignore"):
        w = (d - a_depths[j]) / (a_depths[j + 1] - a_depths[j])
        v = alpha[j] + w * (alpha[j + 1] - alpha[j])
        v = np.where(d <= a_depths[0], alpha[0], v)
        v = np.where(d >= a_depths[-1], alpha[-1], v)
    return v


def path_integral(ts, zs, x, a_depths, alpha, cin, rin, zin):
    """The definition, restated: ts / zs (M, S) stored convention (depth = -z), x (S,) save ranges in the frame of the
    tables, alpha in dB/m on a_depths -> A (M, S): A[:, 0] = 0.0, A[:, s + 1] = A[:, s] + inc_s, one add at a time."""
    ts, zs = np.asarray(ts, dtype=float), np.asarray(zs, dtype=float)
    M, S = zs.shape
    d = -zs
    with np.errstate(invalid="ignore"):
        c = tlr.bilinear(np.broadcast_to(x, (M, S)), d, rin, zin, cin)
        q = alpha_at(d, a_depths, alpha) * c
        A = np.zeros((M, S))
        for s in range(S - 1):
            inc = (0.5 * (q[:, s] + q[:, s + 1])) * (ts[:, s + 1] - ts[:, s])
            A[:, s + 1] = A[:, s] + inc
    return A


def profile_db_per_m(absorption):
    """``absorption`` as the public functions take it (dB/km: a scalar or (depths_m, dB_per_km)) -> (a_depths, alpha dB/m)"""
    if isinstance(absorption, (tuple, list)):
        return np.asarray(absorption[0], dtype=float), np.asarray(absorption[1], dtype=float) / 1000.0
    return None, np.array([float(absorption)]) / 1000.0


def fan_path_integral(rays, environment, absorption, flatearth=True):
    """path_integral of a host fan in the frame it was traced in, the frame derived by frame_independent; ``absorption`` in
    dB/km as the public functions take it, or None for alpha = 1 (the path length)."""
    xf, cin, rin, zin, _, _ = fi.traced_frame(environment, np.asarray(rays.rs, dtype=float)[0], flatearth)
    a_depths, alpha = (None, np.ones(1)) if absorption is None else profile_db_per_m(absorption)
    return path_integral(rays.ts, rays.zs, xf, a_depths, alpha, cin, rin, zin)


def weighted_g(zs, ps, x, cin, rin, zin, W):
    """g = c / sqrt(1 - (p c)^2) (NaN for a NaN sample or |p c| >= 1) times the weights W (M, S); None: g itself"""
    zs, ps = np.asarray(zs, dtype=float), np.asarray(ps, dtype=float)
    M, S = zs.shape
    c = tlr.bilinear(np.broadcast_to(x, (M, S)), -zs, rin, zin, cin)
    pc = ps * c
    ok = np.abs(pc) < 1
    g = np.full((M, S), np.nan)
    with np.errstate(invalid="ignore"):
        g[ok] = c[ok] / np.sqrt(1 - pc[ok] * pc[ok])
        return g if W is None else g * W


def tube_intensity(zs, ps, x, p0, depths, cin, rin, zin, W):
    """tl_reference.tube_intensity, operation for operation, with the weighted g"""
    depths = np.asarray(depths, dtype=float)
    d = -np.asarray(zs, dtype=float)
    M, S = d.shape
    g = weighted_g(zs, ps, x, cin, rin, zin, W)
    r = np.abs(np.asarray(x, dtype=float) - x[0])
    out = np.zeros((len(depths), S))
    with np.errstate(invalid="ignore", divide="ignore", over="ignore"):
        for k in range(M - 1):
            d0, d1 = d[k], d[k + 1]
            valid = ~np.isnan(g[k]) & ~np.isnan(g[k + 1]) & (d0 != d1)
            lo, hi = np.fmin(d0, d1), np.fmax(d0, d1)
            Ik = 0.5 * (g[k] + g[k + 1]) * np.abs(p0[k + 1] - p0[k]) / (r * np.abs(d1 - d0))
            hit = valid[None, :] & (lo[None, :] <= depths[:, None]) & (depths[:, None] < hi[None, :])
            out = np.where(hit, out + Ik[None, :], out)
    out[:, r == 0] = np.nan
    return out


def tube_arrivals(zs, ps, ts, x, p0, depths, cols, cin, rin, zin, W):
    """arrivals_reference.tube_arrivals, operation for operation, with the weighted g"""
    zs, ps, ts = (np.asarray(a, dtype=float) for a in (zs, ps, ts))
    depths = np.asarray(depths, dtype=float)
    cols = np.asarray(cols, dtype=np.int64)
    R, n = len(depths), len(cols)
    d = -zs
    g = weighted_g(zs, ps, x, cin, rin, zin, W)
    r = np.abs(np.asarray(x, dtype=float) - x[0])
    rows = []
    with np.errstate(invalid="ignore", divide="ignore", over="ignore"):
        for slot, s in enumerate(cols):
            if r[s] == 0:
                continue
            d0, d1 = d[:-1, s], d[1:, s]
            valid = ~np.isnan(g[:-1, s]) & ~np.isnan(g[1:, s]) & (d0 != d1)
            lo, hi = np.fmin(d0, d1), np.fmax(d0, d1)
            Ik = 0.5 * (g[:-1, s] + g[1:, s]) * np.abs(p0[1:] - p0[:-1]) / (r[s] * np.abs(d1 - d0))
            j, k = np.nonzero(valid[None, :] & (lo[None, :] <= depths[:, None]) & (depths[:, None] < hi[None, :]))
            w = (depths[j] - d0[k]) / (d1[k] - d0[k])
            rows.append((j, np.full(len(j), slot), k, w, ts[k, s] + w * (ts[k + 1, s] - ts[k, s]),
                         ps[k, s] + w * (ps[k + 1, s] - ps[k, s]), Ik[k]))
    if rows:
        j, sl, k, w, T, p, I = (np.concatenate([row[i] for row in rows]) for i in range(7))
    else:
        j, sl, k = (np.zeros(0, np.int64) for _ in range(3))
        w, T, p, I = (np.zeros(0) for _ in range(4))
    order = np.lexsort((k, sl, j))
    offsets = np.concatenate([[0], np.cumsum(np.bincount(j * n + sl, minlength=R * n))])
    return dict(offsets=offsets, tube=k[order].astype(np.int32), w=w[order], T=T[order], p=p[order], I=I[order])


def beam_intensity(zs, ps, x, p0, depths, cin, rin, zin, bottom, w_min, W):
    """The Gaussian-beam sum of DESIGN.md ("Gaussian beams") restated with the weighted g, operation for operation as
    beam_reference.beam_intensity does it without: E_k = 0.5 (g_k W_k + g_k+1 W_k+1) |dp0| / r, then validity, widths,
    centres, the 4 sigma cut and each receiver's terms added from 0.0 one at a time in (tube, centre) order."""
    depths, bottom, x = (np.asarray(a, dtype=float) for a in (depths, bottom, x))
    d = -np.asarray(zs, dtype=float)
    M, S = d.shape
    g = weighted_g(zs, ps, x, cin, rin, zin, W)
    with np.errstate(invalid="ignore", divide="ignore", over="ignore"):
        r = np.abs(x - x[0])
        valid = ~np.isnan(g[:-1]) & ~np.isnan(g[1:])
        E = 0.5 * (g[:-1] + g[1:]) * np.abs(p0[1:] - p0[:-1])[:, None] / r[None, :]
        D = np.full((M + 1, S), np.nan)
        D[1:-1] = np.abs(d[1:] - d[:-1])                 # D[i + 1] = |d_i+1 - d_i|; none beyond the fan's ends
        sigma = np.fmax(np.fmax(np.fmax(D[:-2], D[1:-1]), D[2:]), w_min)
        mid = 0.5 * (d[:-1] + d[1:])
        amp = E / (sigma * bref.SQRT_2PI)
    R = len(depths)
    out = np.zeros((R, S))
    with np.errstate(invalid="ignore", over="ignore"):
        for s in range(S):
            if r[s] == 0:
                out[:, s] = np.nan
                continue
            acc = np.zeros(R)
            for k in np.flatnonzero(valid[:, s]):        # tubes in order; per tube the beam, its surface and bottom images
                m, sg, a = mid[k, s], sigma[k, s], amp[k, s]
                for ctr in (m, -m, 2.0 * bottom[s] - m):
                    u = (depths - ctr) / sg
                    v = u * u
                    near = v <= 16
                    acc[near] = acc[near] + a * gexp(-0.5 * v[near])
            out[:, s] = acc
    return out


def arc_length(r, theta0, z_s=tlr.GRADIENT_ZS, c_a=tlr.GRADIENT_CA, gamma=tlr.GRADIENT_GAMMA):
    """The length, to range r, of the circular-arc ray launched at depth-down angle theta0 (radians) in c = c_a + gamma z
    (tl_reference.linear_gradient_ray): radius 1 / |xi gamma| times the angle turned, theta0 - theta(r)."""
    a = gamma * np.cos(theta0) / (c_a + gamma * z_s)
    return (theta0 - np.arcsin(np.sin(theta0) - a * r)) / a
