"""Test helpers for the bounce log and boundary loss (not a product path): a plain NumPy restatement of DESIGN.md section 14,
written from the definition -- the per-event loss, the samples an event counts for (np.argmin itself), the running sum --
and the literal slice assignment of the reference's _interpolate_ray that the argmin rule stands for."""
import numpy as np

import oracle
import path_reference as pref
import tl_reference as tlr

DEG = 180.0 / np.pi


def table_at(q, nodes, values):
    """a loss / slope table at q: section 13's rule (path_reference.alpha_at); NaN for a NaN q, a constant table included"""
    q = np.asarray(q, dtype=float)
    v = pref.alpha_at(q, nodes, values)
    return np.where(np.isnan(q), np.nan, v)


def bottom_at(x, br, bd):
    """the frame's bottom depth at x as the fan kernel evaluates it: (1 - w) d_i + w d_i+1 in the cell that holds x"""
    x, br, bd = (np.asarray(a, dtype=float) for a in (x, br, bd))
    i = np.clip(np.searchsorted(br, x, side="right") - 1, 0, len(br) - 2)
    w = (x - br[i]) / (br[i + 1] - br[i])
    return (1 - w) * bd[i] + w * bd[i + 1]


def grazing(x, p, kind, cin, rin, zin, br, bd, beta):
    """one event at range x with the ODE-sign slowness p on the boundary `kind` -> (phi, p c_e): the grazing angle in degrees
    (NaN where x or p is NaN or |p c_e| > 1) and the sine it is the arcsine of"""
    if not (x == x and p == p):
        return np.nan, np.nan
    d = float(bottom_at(x, br, bd)) if kind else 0.0
    pc = p * float(tlr.bilinear(np.array([x]), np.array([d]), rin, zin, cin)[0])
    if not abs(pc) <= 1.0:
        return np.nan, pc
    theta = float(oracle.math_fn("asin", np.array([pc]))[0]) * DEG
    return (abs(theta - float(table_at(x, *beta))) if kind else abs(theta)), pc


def event_loss_one_by_one(bx, bp, bk, cin, rin, zin, br, bd, bottom, surface, beta, psign=-1.0):
    """loss_e of every slot of a log (any shape): NaN where bx or bp is NaN or |p c| > 1; 0.0 in the slots without an event.
    bottom / surface / beta: (nodes or None, values) tables.  The definition, one event at a time through grazing()."""
    bx, bp, bk = np.asarray(bx, dtype=float), np.asarray(bp, dtype=float), np.asarray(bk)
    out = np.zeros(bx.shape)
    for idx in np.ndindex(bx.shape):
        kind = int(bk[idx])
        if kind < 0:
            continue
        phi = grazing(bx[idx], psign * bp[idx], kind, cin, rin, zin, br, bd, beta)[0]
        out[idx] = float(table_at(phi, *(bottom if kind else surface))) if phi == phi else np.nan
    return out


def event_loss(bx, bp, bk, cin, rin, zin, br, bd, bottom, surface, beta, psign=-1.0):
    """event_loss_one_by_one over all events at once: the same operations on every event, in the same order, so the same
    bits (tests/test_bounce_log_host.py compares the two); one call of the oracle's asin for the whole log."""
    bx, bp, bk = np.asarray(bx, dtype=float), np.asarray(bp, dtype=float), np.asarray(bk)
    out = np.zeros(bx.shape)
    live = bk >= 0
    if not live.any():
        return out
    x, p, kind = bx[live], psign * bp[live], bk[live] > 0
    with np.errstate(invalid="ignore"):
        d = np.where(kind, bottom_at(x, br, bd), 0.0)
        pc = p * tlr.bilinear(x, d, rin, zin, cin)
        ok = (x == x) & (p == p) & (np.abs(pc) <= 1.0)
        theta = np.full(x.shape, np.nan)
        theta[ok] = oracle.math_fn("asin", pc[ok]) * DEG
        phi = np.where(kind, np.abs(theta - table_at(x, *beta)), np.abs(theta))
        out[live] = np.where(kind, table_at(phi, *bottom), table_at(phi, *surface))
    return out


def sample_index(x, bx):
    """j_e = np.argmin(|x - bx_e|) (first minimum); 0 for a bx that is not finite"""
    bx = np.asarray(bx, dtype=float)
    j = np.zeros(bx.shape, np.int64)
    with np.errstate(invalid="ignore"):
        for idx in np.ndindex(bx.shape):
            j[idx] = int(np.argmin(np.abs(x - bx[idx]))) if np.isfinite(bx[idx]) else 0
    return j


def boundary_loss(bx, bp, bk, x, cin, rin, zin, br, bd, bottom, surface, beta, psign=-1.0):
    """The definition: bx, bp, bk (M, K) -> B (M, S) float64, nb, ns (M, S) int64.  E = the leading slots with bk >= 0;
    seg(s) = #{e < E: j_e <= s} for s < S - 1, seg(S - 1) = E; B = sum of the first seg(s) losses from 0.0, one add at a time."""
    bk = np.asarray(bk)
    M, K = bk.shape
    S = len(x)
    loss = event_loss(bx, bp, bk, cin, rin, zin, br, bd, bottom, surface, beta, psign)
    j = sample_index(np.asarray(x, dtype=float), bx)
    B, nb, ns = np.zeros((M, S)), np.zeros((M, S), np.int64), np.zeros((M, S), np.int64)
    for m in range(M):
        E = K if (bk[m] >= 0).all() else int(np.argmax(bk[m] < 0))
        for s in range(S):
            seg = E if s == S - 1 else int(np.sum(j[m, :E] <= s))
            run = 0.0
            for e in range(seg):
                run = run + loss[m, e]
            B[m, s] = run
            nb[m, s] = int(np.sum(bk[m, :seg] == 1))
            ns[m, s] = int(np.sum(bk[m, :seg] == 0))
    return B, nb, ns


def segments_by_slice_assignment(x, starts, x_end):
    """The reference's _interpolate_ray, literally (REF/launch_rays.py:745-784): segment k runs from starts[k] to starts[k + 1]
    (the last one to x_end) and is given the samples [idx(start), idx(end)), idx = np.argmin(|x - .|); segments with equal
    ends are skipped; the last sample is the end state, of the last segment.  -> the segment index of every sample."""
    x = np.asarray(x, dtype=float)
    ends = list(starts[1:]) + [x_end]
    owner = np.full(len(x), -1, np.int64)
    for k, (a, b) in enumerate(zip(starts, ends)):
        if a == b:
            continue
        i1, i2 = int(np.argmin(np.abs(x - a))), int(np.argmin(np.abs(x - b)))
        owner[i1:i2] = k
    owner[-1] = len(starts) - 1
    return owner


def trace_bounces(arrs, y0, x0, x1, max_rows=60000, rtol=1e-9, terminate_backwards=True):
    """the bounces of one ray from the oracle's step trace (correctly rounded libm): the first row of every segment k >= 1
    holds the bounce's range and the reflected state -> (bx, bp ODE sign, bk) arrays; bk from the boundary the depth sits on.
    rtol / terminate_backwards: the shot's own, handed to oracle.trace_ray; max_rows: the step attempts the trace may hold
    (asserted not to be reached)"""
    rows = oracle.trace_ray(*arrs, y0, x0, x1, rtol=rtol, terminate_backwards=terminate_backwards, math=oracle.MATH_CR,
                            max_rows=max_rows)
    assert 0 < len(rows) < max_rows
    first = np.flatnonzero(np.diff(rows[:, 11]) > 0) + 1
    bx, bz, bp = rows[first, 0], rows[first, 3], rows[first, 4]
    return bx, bp, (np.abs(bz) > 100.0).astype(np.int8)
