"""Test helpers for beam_arrivals and the sums over them (not a product path): a plain NumPy restatement of DESIGN.md section
21, written from the definition -- per save column every tube's two tests against every receiver at once, then the kept terms
of each (receiver, slot) read off in tube and image order -- independently of beam_pressure_reference.beam_pressure (which
walks tube by tube and adds), on beam_reference's centres and widths, path_reference's weighted g and the library's exp; and
the set-up shared by the CPU and GPU tests: Lloyd's mirror with a pulse on section 20's exact straight rays."""
import numpy as np

import beam_pressure_reference as bp
import beam_reference as bref
import path_reference as pref
import signal_reference as sref

GB_REACH = float.fromhex("0x1.00001p+2")                 # 4 (1 + 2^-20): the cheap test of csrc/pgr_beams.h


def beam_arrivals(zs, ps, ts, x, p0, depths, cin, rin, zin, bottom, w_min, W, q, cols, curvature=True):
    """The definition, restated: zs / ps / ts (M, S) stored convention (depth d = -z, slowness along increasing depth -p), x (S,)
    save ranges in the frame of the tables, p0 (M,), bottom (S,), weights W (M, S) or None, phase index q (M, S) integers or
    None, cols the requested columns -> dict(offsets int64 (R n + 1,), tube, image, q int32, time, amplitude float64), grouped
    by g = j n + c; and `cap`, the A'_k of each arrival's tube, which its amplitude cannot exceed."""
    zs, ps, ts, x, depths, bottom = (np.asarray(a, dtype=float) for a in (zs, ps, ts, x, depths, bottom))
    d, pd = -zs, -ps
    M, S = d.shape
    R, n = len(depths), len(cols)
    g = pref.weighted_g(zs, ps, x, cin, rin, zin, W)
    _, mid, sigma, _, _, r = bref._tubes(zs, ps, x, p0, cin, rin, zin, w_min)      # centres and widths: section 10's
    per_group = [[None] * n for _ in range(R)]
    dj = depths[:, None]
    with np.errstate(invalid="ignore", divide="ignore", over="ignore"):
        for c, s in enumerate(int(v) for v in cols):
            if r[s] == 0:                                                           # the source's own column
                for j in range(R):
                    per_group[j][c] = tuple(np.zeros(0, t) for t in (np.int32, np.int32, float, float, np.int32, float))
                continue
            live = ~np.isnan(g[:-1, s]) & ~np.isnan(g[1:, s])
            qk = np.zeros(M - 1, np.int64) if q is None else np.asarray(q)[:-1, s].astype(np.int64)
            live &= qk >= 0
            E = 0.5 * (g[:-1, s] + g[1:, s]) * np.abs(p0[1:] - p0[:-1]) / r[s]
            dd = d[1:, s] - d[:-1, s]
            D = np.abs(dd)
            sg, m = sigma[:, s], mid[:, s]
            A = np.sqrt(E * D) / (sg * bref.SQRT_2PI)
            Tm = 0.5 * (ts[:-1, s] + ts[1:, s])
            pm = 0.5 * (pd[:-1, s] + pd[1:, s])
            hk = np.where(D > 0, 0.5 * ((pd[1:, s] - pd[:-1, s]) / dd), 0.0) if curvature else np.zeros(M - 1)
            b2 = 2.0 * bottom[s]
            kept, tau, amp = (np.zeros((R, M - 1, 3), t) for t in (bool, float, float))
            for ci, (ctr, e) in enumerate(((m, dj - m), (-m, (-dj) - m), (b2 - m, (b2 - dj) - m))):
                e0 = dj - ctr
                u = e0 / sg
                v = u * u
                kept[:, :, ci] = live & (np.abs(e0) <= sg * GB_REACH) & (v <= 16.0)
                amp[:, :, ci] = A * bref.gexp(-0.5 * np.where(kept[:, :, ci], v, 0.0))
                tau[:, :, ci] = Tm + (pm * e + hk * (e * e))
            for j in range(R):
                k, ci = np.nonzero(kept[j])                                         # row-major: tube order, then image order
                per_group[j][c] = (k.astype(np.int32), ci.astype(np.int32), tau[j, k, ci], amp[j, k, ci],
                                   ((qk[k] + np.array([0, 2, 0])[ci]) & 3).astype(np.int32), A[k])
    flat = [per_group[j][c] for j in range(R) for c in range(n)]
    offsets = np.concatenate([[0], np.cumsum([len(f[0]) for f in flat])]).astype(np.int64)
    tube, image, time, amplitude, qa, cap = (np.concatenate([f[i] for f in flat]) for i in range(6))
    return dict(offsets=offsets, tube=tube, image=image, time=time, amplitude=amplitude, q=qa, cap=cap)


def no_subnormal_squares(amplitude):
    """the precondition of sqrt(fl(a a)) == a: no amplitude in (0, 2^-511)"""
    a = np.asarray(amplitude, dtype=float)
    return not ((a > 0) & (a < 2.0 ** -511)).any()


def fan_beam_arrivals(rays, depths, environment, cols, w_min=10.0, curvature=True, flatearth=True, W=None, nb=None, ns=None):
    """beam_arrivals' definition on a host fan: the frame, the bathymetry and p0 as beam_reference.fan_beam_intensity prepares
    them, q from the restated caustic index and the per-sample counts nb / ns (M, S) (None: a fan without bounces)"""
    import coherent_reference as cref
    from pygenray_amd.host_physics import bilinear_interp
    from pygenray_amd.launch_rays import _initial_slowness
    xf, cin, rin, zin, bd, br = bref.frame_tables(np.asarray(rays.rs, dtype=float)[0], environment, flatearth)
    c_source = bilinear_interp(xf[0], float(rays.source_depths[0]), rin, zin, cin)
    p0 = _initial_slowness(rays.thetas, c_source)
    zs, ps, ts = (np.asarray(a, dtype=float) for a in (rays.zs, rays.ps, rays.ts))
    q = cref.tube_phase(cref.caustic_index(-zs, nb, ns), nb, ns)
    sel = np.concatenate([[0], np.asarray(cols, dtype=np.int64)])                   # (the source's column is kept for r)
    Wc = None if W is None else np.asarray(W)[:, sel]
    return beam_arrivals(zs[:, sel], ps[:, sel], ts[:, sel], xf[sel], p0, depths, cin, rin, zin,
                         bref.bottom_depths(xf, bd, br)[sel], w_min, Wc, np.asarray(q)[:, sel], 1 + np.arange(len(cols)),
                         curvature)


# ---- Lloyd's mirror with a pulse, on section 20's exact straight rays --------------------------------------------------------
# beam_pressure_reference's set-up (isovelocity, source at 200 m, receivers 75 ... 925 m at 2 ... 5 km, min_width 10 m) with
# signal_reference's pulse: 75 Hz centre, 20 Hz bandwidth, on signal_reference's time axes (LLOYD_LEAD before x / c, LLOYD_DT,
# LLOYD_NT).  The yardstick is the two-path closed form of signal_reference.lloyd_pulse_error, which is written for
# coherent_reference's source depth, receivers and frequency: lloyd_pulse_error below is the same expression with those three
# as arguments, and tests/test_beam_arrivals_host.py asserts that it gives signal_reference's values when given them.

PULSE_F, PULSE_B = sref.FOURIER_F, sref.FOURIER_B
# the worst e = |u - u_ref| / sqrt(1 / R1^2 + 1 / R2^2) over every receiver, the four ranges and every sample of the restatement
# (tests/test_beam_arrivals_host.py prints it), and the bound: twice that (DESIGN.md section 19's rule)
LLOYD_PULSE_MEASURED = 9.575190772066419e-05
LLOYD_PULSE_BOUND = 2.0 * LLOYD_PULSE_MEASURED


def lloyd_pulse_error(u, x, source_depth=bp.LLOYD_ZS, depths=bp.LLOYD_DEPTHS, f=PULSE_F, c=bp.EXACT_C, B=PULSE_B):
    """u (len(depths), len(x), LLOYD_NT) complex on the time axes x / c - LLOYD_LEAD + n LLOYD_DT -> e (same shape), the error
    against E(t - R1 / c) e^{i k R1} / R1 - E(t - R2 / c) e^{i k R2} / R2 in units of the incoherent amplitude"""
    D, X = np.asarray(depths, dtype=float)[:, None, None], np.asarray(x, dtype=float)[None, :, None]
    t = (np.asarray(x, dtype=float) / c - sref.LLOYD_LEAD)[None, :, None] + (np.arange(sref.LLOYD_NT) * sref.LLOYD_DT)[None, None, :]
    R1, R2 = np.hypot(X, D - source_depth), np.hypot(X, D + source_depth)
    sigma = sref.pulse_sigma(B)
    k = 2.0 * np.pi * f / c

    def E(tau):
        return np.where(np.abs(tau) <= 8.0 * sigma, np.exp(-tau ** 2 / (2.0 * sigma ** 2)), 0.0)
    ref = E(t - R1 / c) * np.exp(1j * k * R1) / R1 - E(t - R2 / c) * np.exp(1j * k * R2) / R2
    return np.abs(u - ref) / np.sqrt(1.0 / R1 ** 2 + 1.0 / R2 ** 2)


def exact_lloyd_arrivals(w_min=10.0, curvature=True):
    """the restatement on beam_pressure_reference.exact_fan at the four ranges -> its dict"""
    zs, ps, ts, x, p0, q = bp.exact_fan(bp.LLOYD_ZS)
    return beam_arrivals(zs, ps, ts, x, p0, bp.LLOYD_DEPTHS, bp.EXACT_CIN, bp.EXACT_RIN, bp.EXACT_ZIN,
                         np.full(len(x), bp.EXACT_BOTTOM), w_min, None, q, [1, 2, 3, 4], curvature)


def pulse_of(a, x, f=PULSE_F, B=PULSE_B, c=bp.EXACT_C):
    """signal_reference.signal_sum of an arrival dict `a` at the ranges x (one per slot) on the Lloyd time axes ->
    (R, len(x), LLOYD_NT) complex"""
    n = len(x)
    R = (len(a["offsets"]) - 1) // n
    tstart = np.tile(np.asarray(x, dtype=float) / c - sref.LLOYD_LEAD, R)
    u = sref.signal_sum(a["offsets"], a["time"], a["amplitude"] * a["amplitude"], a["q"], tstart, f, sref.inv_sigma(B),
                        sref.LLOYD_DT, sref.LLOYD_NT)
    return u.reshape(R, n, sref.LLOYD_NT)
