"""Test helper for travel_time_kernel (not a product path): a plain Python/NumPy restatement of the travel-time sensitivity
kernel of DESIGN.md ("Travel-time sensitivity kernels"), operation for operation as csrc/pgr_sens.h forms it, so the GPU
must match it bit for bit; and the frame and finite-difference helpers the tests share."""
import numpy as np

from pygenray_amd.environment import _mirror_envi_arrays, _unpack_envi

import tl_reference as tlr


def _count(G, q, le):
    """#(G <= q) (le) or #(G < q): np.searchsorted side 'right' / 'left'"""
    return int(np.searchsorted(G, q, side="right" if le else "left"))


class Axis:
    """One axis of a chord q0 -> q1 on the grid G: direction, start cell, and the nc cuts in chord order (cut r is line
    first + dir * r at parameter cut(r)); cell(r) is the cell after r cuts."""

    def __init__(self, G, q0, q1):
        n = len(G)
        self.G, self.q0, self.dq = G, q0, q1 - q0
        self.dir = 1 if q1 > q0 else (-1 if q1 < q0 else 0)
        lo, hi = 1, 0
        if self.dir > 0:
            c = _count(G, q0, True)
            cell0 = c - 1
            lo, hi = max(c, 1), min(_count(G, q1, False) - 1, n - 2)
            self.first = lo
        else:
            c = _count(G, q0, False)
            cell0 = c - 1
            if self.dir < 0:
                lo, hi = max(_count(G, q1, True), 1), min(c - 1, n - 2)
            self.first = hi
        self.cell0 = min(max(cell0, 0), n - 2)
        self.nc = max(hi - lo + 1, 0)
        # the cut parameters, in chord order (non-decreasing: a division by a constant is monotone)
        self.v = [float((G[self.first + self.dir * r] - q0) / self.dq) for r in range(self.nc)]

    def cell(self, r):
        return self.cell0 + self.dir * r

    def visit(self, i):
        r = (i - self.cell0) * (self.dir if self.dir else 1)
        return r if 0 <= r <= self.nc else -1

    def count(self, p, le):
        return int(np.searchsorted(self.v, p, side="right" if le else "left"))


def reaches(X, a):
    """does a chord with range axis X reach a cell of range node a (a - 1 or a)?"""
    c1 = X.cell(X.nc)
    return min(X.cell0, c1) <= a and max(X.cell0, c1) >= a - 1


class Chord:
    def __init__(self, x0, x1, d0, d1, T0, T1, g, h):
        self.x0, self.d0 = x0, d0
        self.dx, self.dd = x1 - x0, d1 - d0
        self.L = float(np.sqrt(self.dx * self.dx + self.dd * self.dd))
        self.dT = T1 - T0
        self.X, self.D = Axis(g, x0, x1), Axis(h, d0, d1)

    def point(self, u):
        return self.x0 + u * self.dx, self.d0 + u * self.dd

    def sub(self, r):
        """range sub-chord r: (pa, pb, r0, nin), or None (not visited or zero length)"""
        if r < 0:
            return None
        pa = 0.0 if r == 0 else self.X.v[r - 1]
        pb = 1.0 if r == self.X.nc else self.X.v[r]
        if not pa < pb:
            return None
        r0 = self.D.count(pa, True)
        return pa, pb, r0, self.D.count(pb, False) - r0

    def piece(self, sub, k):
        pa, pb, r0, nin = sub
        return (pa if k == 0 else self.D.v[r0 + k - 1]), (pb if k == nin else self.D.v[r0 + k])


def kernel(T, Z, x, g, h, cin, rin, zin, col):
    """The definition, restated: T / Z (S, M) rows, stored convention (depth = -Z), x (S,) save ranges and g (A,), h (B,)
    the grid, both in the frame of the tables (cin, rin, zin), col the end column -> K (M, A, B).  Loops over rays and
    chords in Python floats; the look-ups through tl_reference.bilinear (host_physics.bilinear_interp's bits)."""
    T = np.asarray(T, dtype=float)
    Z = np.asarray(Z, dtype=float)
    x = np.asarray(x, dtype=float)
    g = np.asarray(g, dtype=float)
    h = np.asarray(h, dtype=float)
    S, M = T.shape
    A, B = len(g), len(h)
    K = np.zeros((M, A, B))

    def ic(ch, u):
        px, pd = ch.point(u)
        return 1.0 / float(tlr.bilinear(px, pd, rin, zin, cin))

    for m in range(M):
        Tm, dm = T[: col + 1, m], -Z[: col + 1, m]
        if not (np.isfinite(Tm).all() and np.isfinite(dm).all()):
            K[m] = np.nan
            continue
        chords, beta = [], []
        for s in range(col):
            ch = Chord(float(x[s]), float(x[s + 1]), float(dm[s]), float(dm[s + 1]), float(Tm[s]), float(Tm[s + 1]), g, h)
            Q1, ic0 = 0.0, ic(ch, 0.0)
            for r in range(ch.X.nc + 1):
                sub = ch.sub(r)
                if sub is None:
                    continue
                for k in range(sub[3] + 1):
                    p, q = ch.piece(sub, k)
                    w6 = (q - p) * ch.L / 6.0
                    icm, ic1 = ic(ch, 0.5 * (p + q)), ic(ch, q)
                    Q1 = Q1 + w6 * ((ic0 + 4.0 * icm) + ic1)
                    ic0 = ic1
            chords.append(ch)
            beta.append(ch.dT / Q1 if Q1 != 0.0 else 0.0)
        for a in range(A):
            acc = np.zeros(B)
            for s, ch in enumerate(chords):
                if not reaches(ch.X, a):
                    continue
                q = np.zeros(B)
                cells = (a - 1, a) if ch.X.dir >= 0 else (a, a - 1)
                for i in cells:
                    if i < 0 or i > A - 2:
                        continue
                    sub = ch.sub(ch.X.visit(i))
                    if sub is None:
                        continue
                    lo = np.zeros(B)      # lo[j]: the term of the piece in depth cell j at node j; hi[j]: at node j + 1
                    hi = np.zeros(B)
                    for k in range(sub[3] + 1):
                        j = ch.D.cell(sub[2] + k)
                        p, pq = ch.piece(sub, k)
                        w6 = (pq - p) * ch.L / 6.0
                        flo, fhi = [], []
                        for u in (p, 0.5 * (p + pq), pq):
                            c = ic(ch, u)
                            sq = c * c
                            px, pd = ch.point(u)
                            wx = (px - g[i]) / (g[i + 1] - g[i])
                            wy = (pd - h[j]) / (h[j + 1] - h[j])
                            rf = (1 - wx) if i == a else wx
                            flo.append((rf * (1 - wy)) * sq)
                            fhi.append((rf * wy) * sq)
                        lo[j] = w6 * ((flo[0] + 4.0 * flo[1]) + flo[2])
                        hi[j] = w6 * ((fhi[0] + 4.0 * fhi[1]) + fhi[2])
                    # node b: cell b - 1's upper term and cell b's lower term, in chord order
                    up = np.concatenate([[0.0], hi[:-1]])
                    q = (q + up) + lo if ch.D.dir >= 0 else (q + lo) + up
                acc = acc - beta[s] * q
            K[m, a] = acc
    return K


def traced_tables(environment, flatearth, backwards):
    """(cin, rin, zin) of the frame a fan was traced in (mirrored for a backwards fan)"""
    cin, cpin, rin, zin, bd, br, ba = _unpack_envi(environment, flatearth=flatearth)
    if backwards:
        cin, cpin, rin, bd, br, ba = _mirror_envi_arrays(cin, cpin, rin, bd, br, ba)
    return cin, rin, zin


def fan_kernel(rays, environment, ranges, depths, flatearth=True, range_index=-1):
    """kernel() of a host fan, prepared as travel_time_kernel does: the traced frame, the grid mirrored for a backwards fan
    and the range axis put back in the user's order."""
    x = np.asarray(rays.rs, dtype=float)[0]
    back = len(x) > 1 and x[-1] < x[0]
    cin, rin, zin = traced_tables(environment, flatearth, back)
    g = np.asarray(ranges, dtype=float)
    K = kernel(np.asarray(rays.ts).T, np.asarray(rays.zs).T, -x if back else x, -g[::-1] if back else g,
               np.asarray(depths, dtype=float), cin, rin, zin, range_index % len(x))
    return K[:, ::-1] if back else K
