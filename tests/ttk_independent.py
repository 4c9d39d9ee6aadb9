"""Test helper for travel_time_kernel (not a product path): an independent, high-precision evaluation of the travel-time
sensitivity kernel of DESIGN.md ("Travel-time sensitivity kernels"), written from the definition and sharing no code with
tests/ttk_reference.py, tests/tl_reference.py or the package's arithmetic (only the traced tables are taken as inputs).

How it differs from the restatement:
* Geometry is exact (``fractions.Fraction`` of the input doubles): every parameter in (0, 1) where a chord meets an
  interior kernel-grid line, on either axis, is collected, sorted and deduplicated; a piece's cell is the cell of its
  exact midpoint (``bisect_left`` - 1, clamped).  No cut is counted.  A chord lying on a line (a standing axis) takes the
  cell on the low side of it, the definition's rule for such a chord.
* Values are ``mpmath`` numbers at 200 bits (60 digits): c is the bilinear blend of the table at the point, 1/c, the basis
  weights phi_ab (the kernel cell, unclamped weights) and every sum.  Nothing is rounded to float64 before the end.
  K = -sum_s dT_s Q_ab(s) / Q_1(s): the chord length L cancels between beta_s = dT_s / Q_1 and Q_ab, so only the rounding
  bound needs it.
* ``rule="simpson"``: the kernel's definition (Simpson at 0, 1/2, 1 of each piece).  ``rule="exact"``: each piece cut
  again at the table's own lines (inside such a sub-piece c, phi and so f = phi / c^2 are smooth) and integrated by
  24-point Gauss-Legendre; for the rational f of a sub-piece that is exact far below float64 resolution.

``kernel`` also returns, for ``rule="simpson"``, per entry the magnitude ``mag`` = sum_s |beta_s| sum_pieces l/6 (|f0| +
4 |fm| + |f1|) and ``bound``: how far a float64 evaluation of the definition in the operation order of DESIGN section 11
(correctly rounded operations, nothing contracted) can be from the exact value.  Its derivation, first order in
eps = 2^-53 (the neglected terms are smaller by a factor n eps, n < 1e6, so below 1e-10 of the bound):

1. Parameters.  A cut u = (G - q0) / (q1 - q0) rounds three times: |du| <= 3 eps u <= 3 eps.  A midpoint
   0.5 (p + q) adds one rounding: |du| <= 4 eps.  So every evaluation parameter is within 4 eps of the exact one.
2. Points.  x = x0 + u dx with dx = x1 - x0 rounded and two more roundings:
   |dP_x| <= 4 eps |dx| + eps |dx| + eps |u dx| + eps |x| <= eps (6 |dx| + |x|), and the same for the depth.  This is the
   position term: at |x| = 60 km in a 100 m cell a weight loses 1e-13 absolute, far more than a relative eps.
3. Kernel-grid weights.  w = (x - g0) / (g1 - g0): |dw| <= dP_x / (g1 - g0) + 3 eps |w|; a factor 1 - w one eps of itself
   more: |d rf| <= dP_x / (g1 - g0) + 3 eps |wx| + eps |rf|, and likewise |d wyf| for the depth factor.
4. The look-up of c.  The table weights lose 3 eps relative, a factor 1 - w one eps, the two products and three sums of
   the blend 5 eps: |dc| <= 13 eps Cabs + |dc/dx| dP_x + |dc/dd| dP_d, Cabs = (|tx| + |1 - tx|)(|ty| + |1 - ty|) max|cin|
   of the cell (tx, ty its table weights), |dc/dx| <= (|ty| + |1 - ty|) Lx and |dc/dd| <= (|tx| + |1 - tx|) Ld with Lx, Ld
   the table's largest range and depth slopes.  1 / c and its square add 3 eps:  c^-2 is off by theta = 2 |dc| / c + 3 eps
   relative, 1 / c by |dc| / c + eps.
5. f = (rf wyf) c^-2 (two products): |df| <= (|d rf| |wyf| + |rf| |d wyf|) c^-2 + |rf wyf| c^-2 theta + 2 eps |f|.
6. A piece.  w6 = (q - p) L / 6 with L = sqrt(dx^2 + dd^2) 3 eps off: 6 eps relative, and its ends move by |dp|, |dq|
   (3 eps at a cut, 0 at 0 and 1).  Simpson's sum (f0 + 4 fm) + f1 2 eps, its product with w6 one:
   |dv| <= 2 L (|dp| + |dq|) max|f_k| + l/6 sum_k w_k |df_k| + 9 eps l/6 sum_k w_k |f_k|  (w = 1, 4, 1).
   The first term (twice what moving the ends costs) also covers a piece the float cuts put in the wrong order.
7. Pieces that exist in one evaluation only.  Where two cuts (a range and a depth line, or a grid corner) are within
   6 eps of each other, the float order may differ from the exact one, giving a piece of parameter length <= 6 eps in a
   cell the exact path does not enter.  Every node of every cell the chord touches within 8 eps of an exact cut gets
   |beta| 16 eps L c^-2 (|wx| + |1 - wx|)(|wy| + |1 - wy|).
8. Q_1 is the sequential sum of its pieces (positive terms): E_1 = sum_pieces (item 6 with g = 1 / c) + n_pieces eps Q_1;
   beta = dT / Q_1 with dT and the division rounded: rho = E_1 / Q_1 + 2 eps relative.
9. An entry.  Per chord q = up to four piece terms (3 eps of their magnitudes), times beta (eps), then the ordered sum over
   the n chords that reach it (n eps of the sum of magnitudes), and the final rounding of the exact value (eps):
   bound = sum_s |beta_s| [(rho_s + 4 eps) (Q_s + E_s) + E_s] + (n + 1) eps sum_s |beta_s| (Q_s + E_s),
   Q_s the piece magnitudes and E_s the items 6 and 7 of chord s at that node.
A NaN row is NaN with bound 0; an entry no piece touches is exactly 0 with bound 0.
"""
import bisect
from fractions import Fraction

import mpmath
import numpy as np
from mpmath.calculus.quadrature import GaussLegendre

EPS = 2.0 ** -53
MP = mpmath.MPContext()
MP.prec = 200
_GL = GaussLegendre(MP).calc_nodes(4, MP.prec)        # 24 (node, weight) pairs on [-1, 1]
_HALF = Fraction(1, 2)


def _mp(v):
    """an exact rational as an mpf (one rounding, at 200 bits)"""
    return MP.mpf(v.numerator) / v.denominator if isinstance(v, Fraction) else MP.mpf(v)


def _cell(GF, q):
    """the cell of q on the grid GF (Fractions): bisect_left - 1, clamped to the grid's cells"""
    return min(max(bisect.bisect_left(GF, q) - 1, 0), len(GF) - 2)


def _cuts(G, q0, q1):
    """the exact parameters in (0, 1) where q0 -> q1 meets the interior lines of the float grid G"""
    if q0 == q1:
        return []
    lo, hi = (q0, q1) if q0 < q1 else (q1, q0)
    a = max(bisect.bisect_right(G, float(lo)), 1)
    b = min(bisect.bisect_left(G, float(hi)), len(G) - 1)
    return [(Fraction(G[l]) - q0) / (q1 - q0) for l in range(a, b)]


class _Axis:
    def __init__(self, G):
        self.G = [float(v) for v in G]
        self.F = [Fraction(v) for v in self.G]
        self.M = [MP.mpf(v) for v in self.G]


class Table:
    """the traced table (cin, rin, zin): c as the exact bilinear blend, and the constants the rounding bound uses"""

    def __init__(self, cin, rin, zin):
        cin = np.asarray(cin, dtype=float)
        self.r, self.z = _Axis(rin), _Axis(zin)
        self.cf = cin
        self.Lx = float(np.max(np.abs(np.diff(cin, axis=0)) / np.diff(np.asarray(rin, float))[:, None]))
        self.Ld = float(np.max(np.abs(np.diff(cin, axis=1)) / np.diff(np.asarray(zin, float))[None, :]))

    def cells(self, X, D):
        return _cell(self.r.F, X), _cell(self.z.F, D)

    def c_at(self, i, j, X, D):
        """c at the mpf point (X, D) by the blend of table cell (i, j), and its table weights"""
        tx = (X - self.r.M[i]) / (self.r.M[i + 1] - self.r.M[i])
        ty = (D - self.z.M[j]) / (self.z.M[j + 1] - self.z.M[j])
        c00, c10, c01, c11 = (MP.mpf(float(v)) for v in self.cf[i: i + 2, j: j + 2].T.ravel())
        v = ((1 - tx) * (1 - ty) * c00 + tx * (1 - ty) * c10 + (1 - tx) * ty * c01 + tx * ty * c11)
        return v, tx, ty


def _weights(gx, gd, i, j, X, D):
    """phi of the four nodes of kernel cell (i, j) at the mpf point (X, D): [((a, b), phi)], and (wx, wy)"""
    wx = (X - gx.M[i]) / (gx.M[i + 1] - gx.M[i])
    wy = (D - gd.M[j]) / (gd.M[j + 1] - gd.M[j])
    return [((i, j), (1 - wx) * (1 - wy)), ((i + 1, j), wx * (1 - wy)), ((i, j + 1), (1 - wx) * wy),
            ((i + 1, j + 1), wx * wy)], wx, wy


def _w_derivs(D1, D2, cmin):
    """sup-norm bounds of the 2nd to 4th derivatives of w = c^-2 and the 4th of 1 / c, for c quadratic (c''' = 0) with
    |c'| <= D1, |c''| <= D2, c >= cmin > 0: w'' = 6 c^-4 c'^2 - 2 c^-3 c'', w''' = -24 c^-5 c'^3 + 18 c^-4 c' c'',
    w'''' = 120 c^-6 c'^4 - 144 c^-5 c'^2 c'' + 18 c^-4 c''^2, (1/c)'''' = 24 c^-5 c'^4 - 36 c^-4 c'^2 c'' + 6 c^-3 c''^2"""
    w2 = 6 * D1 ** 2 / cmin ** 4 + 2 * D2 / cmin ** 3
    w3 = 24 * D1 ** 3 / cmin ** 5 + 18 * D1 * D2 / cmin ** 4
    w4 = 120 * D1 ** 4 / cmin ** 6 + 144 * D1 ** 2 * D2 / cmin ** 5 + 18 * D2 ** 2 / cmin ** 4
    g4 = 24 * D1 ** 4 / cmin ** 5 + 36 * D1 ** 2 * D2 / cmin ** 4 + 6 * D2 ** 2 / cmin ** 3
    return w2, w3, w4, g4


def _quad(v0, vm, v1):
    """the quadratic through (0, v0), (1/2, vm), (1, v1) on t in [0, 1] -> (sup|v|, sup|v'|, |v''|, min v)"""
    b1, b2 = -3 * v0 + 4 * vm - v1, 2 * v0 - 4 * vm + 2 * v1
    vals = [v0, v1]
    if b2 != 0 and 0 < -b1 / (2 * b2) < 1:
        t = -b1 / (2 * b2)
        vals.append(v0 + b1 * t + b2 * t * t)
    return max(abs(v) for v in vals), max(abs(b1), abs(b1 + 2 * b2)), abs(2 * b2), min(vals)


def _remainder(cs, phis, ell):
    """Simpson's remainder on a piece inside one table cell, in the piece's own parameter t (u = p + t ell): c and phi are
    quadratic in t there (bilinear along a line), so |integral - Simpson| <= ell / 2880 sup|F''''(t)| for F = phi c^-2
    (Leibniz: phi w'''' + 4 phi' w''' + 6 phi'' w'') and for F = 1 / c -> (R_1, {node: R_ab}), in the units of the sums
    (parameter length: the factor L cancels in K)"""
    _, D1, D2, cmin = _quad(*cs)
    w2, w3, w4, g4 = _w_derivs(D1, D2, cmin)
    out = {}
    for node, (p0, pm, p1) in phis.items():
        P0, P1, P2, _ = _quad(p0, pm, p1)
        out[node] = ell / 2880 * (P0 * w4 + 4 * P1 * w3 + 6 * P2 * w2)
    return ell / 2880 * g4, out


class _Ray:
    """sparse per-entry sums of one ray"""

    def __init__(self):
        self.K, self.mag, self.err, self.n, self.rem = {}, {}, {}, {}, {}

    def add(self, node, v, mag, err):
        self.K[node] = self.K.get(node, 0) + v
        self.mag[node] = self.mag.get(node, 0.0) + mag
        self.err[node] = self.err.get(node, 0.0) + err
        self.n[node] = self.n.get(node, 0) + 1


def _chord(tab, gx, gd, x0, x1, d0, d1, T0, T1, rule, ray):
    X0, X1, D0, D1 = Fraction(x0), Fraction(x1), Fraction(d0), Fraction(d1)
    dX, dD = X1 - X0, D1 - D0
    if dX == 0 and dD == 0:
        return                                            # Q_1 = 0: beta = 0, the chord adds nothing
    us = sorted(set([Fraction(0), Fraction(1)] + _cuts(gx.G, X0, X1) + _cuts(gd.G, D0, D1)))
    dT = _mp(Fraction(T1) - Fraction(T0))
    L = MP.sqrt(_mp(dX * dX + dD * dD))
    Lf, dxf, ddf = float(L), abs(float(dX)), abs(float(dD))
    bound = rule == "simpson"

    def point(u):
        return X0 + u * dX, D0 + u * dD

    Q1, E1, Q1mag, R1, rem = MP.mpf(0), 0.0, 0.0, 0.0, {}
    terms = {}                                            # node -> [Q_ab, magnitude, E]
    for p, q in zip(us[:-1], us[1:]):
        i, j = _cell(gx.F, X0 + (p + q) * _HALF * dX), _cell(gd.F, D0 + (p + q) * _HALF * dD)
        if rule == "simpson":
            evals = [(p, Fraction(1, 6)), ((p + q) * _HALF, Fraction(4, 6)), (q, Fraction(1, 6))]
            subs = [(p, q, evals)]
        else:                                             # cut again at the table's lines: smooth sub-pieces
            su = sorted(set([p, q] + [u for u in _cuts(tab.r.G, X0, X1) + _cuts(tab.z.G, D0, D1) if p < u < q]))
            subs = [(a, b, None) for a, b in zip(su[:-1], su[1:])]
        pq_terms, g_sum, fmax, gmax, e_node, m_node, e1_piece, m1_piece = {}, MP.mpf(0), {}, 0.0, {}, {}, 0.0, 0.0
        cs, phis = [], {}                                 # c and phi at the Simpson points, for the remainder
        for a, b, evals in subs:
            ti, tj = tab.cells(*point((a + b) * _HALF))          # a sub-piece lies in one table cell
            if evals is None:
                h = _mp(b - a) / 2
                m = _mp((a + b) * _HALF)
                pts = [(m + h * t, w / 2) for t, w in _GL]
            else:
                pts = [(u, w) for u, w in evals]
            ell = _mp(b - a)
            for u, w in pts:
                if isinstance(u, Fraction):                # (c is continuous: any cell holding the point will do)
                    Xf, Df = point(u)
                    ti, tj = tab.cells(Xf, Df)
                    X, D = _mp(Xf), _mp(Df)
                else:
                    X, D = _mp(X0) + u * _mp(dX), _mp(D0) + u * _mp(dD)
                c, tx, ty = tab.c_at(ti, tj, X, D)
                ic = 1 / c
                wts, wx, wy = _weights(gx, gd, i, j, X, D)
                wm = _mp(w) * ell
                g_sum += wm * ic
                for node, phi in wts:
                    pq_terms[node] = pq_terms.get(node, 0) + wm * phi * ic * ic
                    phis.setdefault(node, []).append(float(phi))
                cs.append(float(c))
                if not bound:
                    continue
                # rounding bound, items 2 to 5 (floats: magnitudes only)
                px, pd, cf, wxf, wyf = float(X), float(D), float(c), float(wx), float(wy)
                txf, tyf = float(tx), float(ty)
                dPx, dPd = EPS * (6 * dxf + abs(px)), EPS * (6 * ddf + abs(pd))
                xe, de = abs(tyf) + abs(1 - tyf), abs(txf) + abs(1 - txf)
                cmax = float(np.max(np.abs(tab.cf[ti: ti + 2, tj: tj + 2])))
                dc = 13 * EPS * xe * de * cmax + tab.Lx * xe * dPx + tab.Ld * de * dPd
                theta = 2 * dc / cf + 3 * EPS
                sq = 1.0 / (cf * cf)
                gw, hw = gx.G[i + 1] - gx.G[i], gd.G[j + 1] - gd.G[j]
                wf, lw = float(w), float(b - a) * Lf
                for (node, _), rf, yf in zip(wts, (1 - wxf, wxf, 1 - wxf, wxf), (1 - wyf, 1 - wyf, wyf, wyf)):
                    drf = dPx / gw + 3 * EPS * abs(wxf) + EPS * abs(rf)
                    dyf = dPd / hw + 3 * EPS * abs(wyf) + EPS * abs(yf)
                    f = abs(rf * yf) * sq
                    df = (drf * abs(yf) + abs(rf) * dyf) * sq + f * theta + 2 * EPS * f
                    fmax[node] = max(fmax.get(node, 0.0), f)
                    e_node[node] = e_node.get(node, 0.0) + lw * wf * (df + 9 * EPS * f)
                    m_node[node] = m_node.get(node, 0.0) + lw * wf * f
                gmax = max(gmax, 1.0 / cf)
                e1_piece += lw * wf * (1.0 / cf * (dc / cf + EPS) + 9 * EPS / cf)
                m1_piece += lw * wf / cf
        Q1 += g_sum
        if bound:
            r1, rn = _remainder(cs, phis, float(q - p))
            R1 += r1
            for node, v in rn.items():
                rem[node] = rem.get(node, 0.0) + v
        if bound:
            dpq = (3 * EPS if 0 < p < 1 else 0.0) + (3 * EPS if 0 < q < 1 else 0.0)
            E1 += e1_piece + 2 * Lf * dpq * gmax
            Q1mag += m1_piece
        for node, v in pq_terms.items():
            t = terms.setdefault(node, [0, 0.0, 0.0])
            t[0] += v
            if bound:
                t[1] += m_node[node]
                t[2] += e_node[node] + 2 * Lf * dpq * fmax[node]
    if bound:
        # item 7: the cells within 8 eps of an exact cut
        for u in us[1:-1]:
            lo, hi = point(u - Fraction(1, 2 ** 50)), point(u + Fraction(1, 2 ** 50))
            ia, ib = sorted((_cell(gx.F, lo[0]), _cell(gx.F, hi[0])))
            ja, jb = sorted((_cell(gd.F, lo[1]), _cell(gd.F, hi[1])))
            Xc, Dc = point(u)
            ti, tj = tab.cells(Xc, Dc)
            cf = float(tab.c_at(ti, tj, _mp(Xc), _mp(Dc))[0])
            for i in range(ia, ib + 1):
                for j in range(ja, jb + 1):
                    _, wx, wy = _weights(gx, gd, i, j, _mp(Xc), _mp(Dc))
                    wxf, wyf = float(wx), float(wy)
                    phi = (abs(wxf) + abs(1 - wxf)) * (abs(wyf) + abs(1 - wyf))
                    for node in ((i, j), (i + 1, j), (i, j + 1), (i + 1, j + 1)):
                        t = terms.setdefault(node, [0, 0.0, 0.0])
                        t[2] += 16 * EPS * Lf * phi / (cf * cf)
        E1 += (len(us) - 1) * EPS * Q1mag
    Q1f = float(Q1) * Lf
    beta = abs(float(dT)) / Q1f
    rho = E1 / Q1f + 2 * EPS if bound else 0.0
    for node, (v, mag, e) in terms.items():
        ray.add(node, -dT * v / Q1, beta * (mag + e), beta * ((rho + 4 * EPS) * (mag + e) + e))
        if bound:
            q1, rab = float(Q1), rem.get(node, 0.0)
            ray.rem[node] = ray.rem.get(node, 0.0) + abs(float(dT)) * (rab + (abs(float(v)) + rab) * R1 / (q1 - R1)) / q1


def kernel(T, Z, x, g, h, cin, rin, zin, col, rule="simpson", remainder=False):
    """T / Z (S, M) rows, stored convention (depth = -Z), x (S,) save ranges and g (A,), h (B,) the kernel grid, all in the
    frame of the tables (cin, rin, zin); col the end column -> (K, mag, bound), each (M, A, B) float64: K the exact value
    rounded once, mag and bound as the module docstring defines them (zeros for rule="exact").  With ``remainder`` (rule
    "simpson", on the table's own grid) a fourth array: the bound on |K - K_exact| that ``_remainder`` derives, summed as
    |dT| (R_ab + |Q_ab| R_1 / (Q_1 - R_1)) / Q_1 per chord (the quotient Q_ab / Q_1 with both sums off by their R)."""
    if remainder:
        assert rule == "simpson" and np.array_equal(g, rin) and np.array_equal(h, zin), "the table's own grid only"
    T = np.asarray(T, dtype=float)
    Z = np.asarray(Z, dtype=float)
    x = np.asarray(x, dtype=float)
    S, M = T.shape
    A, B = len(g), len(h)
    tab, gx, gd = Table(cin, rin, zin), _Axis(g), _Axis(h)
    K, mag, bound, rem = (np.zeros((M, A, B)) for _ in range(4))
    for m in range(M):
        Tm, dm = T[: col + 1, m], -Z[: col + 1, m]
        if not (np.isfinite(Tm).all() and np.isfinite(dm).all()):
            K[m] = np.nan
            continue
        ray = _Ray()
        for s in range(col):
            _chord(tab, gx, gd, float(x[s]), float(x[s + 1]), float(dm[s]), float(dm[s + 1]), float(Tm[s]),
                   float(Tm[s + 1]), rule, ray)
        for (a, b), v in ray.K.items():
            if 0 <= a < A and 0 <= b < B:
                K[m, a, b] = float(v)
                mag[m, a, b] = ray.mag[(a, b)]
                bound[m, a, b] = ray.err[(a, b)] + (ray.n[(a, b)] + 1) * EPS * ray.mag[(a, b)]
                rem[m, a, b] = ray.rem.get((a, b), 0.0)
    return (K, mag, bound, rem) if remainder else (K, mag, bound)
