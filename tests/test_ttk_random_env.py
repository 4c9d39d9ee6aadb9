"""The travel-time sensitivity kernel (csrc/pgr_sens.h: pgr_ttk_seg, pgr_ttk_span, pgr_ttk_sum) and the time fronts
(csrc/pgr_front.h) on the random environments of helpers.random_case: the cases, API seeds, columns and receivers are
test_products_random_env.py's own objects.  Until this module the kernel had met one table on one look-up path (syn_env, ranges
-2 ... 62 km) and, through fans, frames the package derived itself; on the random environments nothing held
FanHandle.travel_time_kernel or FanHandle.time_front to a reference.  In the reference arithmetic only.

Every input is a fixed function of the seed, chosen on the CPU from the ORACLE's fan (oracle.MATH_CR) before any device run:
* kernel ranges g: A cycles through 2, 5, 9, 14 with the case's position; the first node 1 ... 5 % of the fan's span before the
  first save range and the last as far beyond the last one (those cells extrapolate); where A > 2 one node is the save range
  x[S // 2] itself, one a table range line inside the fan, the others drawn uniformly: a non-uniform grid;
* kernel depths h: B cycles through 62, 63, 64, 127 (the 63-node tile, either side of it, two tiles and a node), from 120 m
  above the surface to 150 m below the deepest floor; six nodes are depths of the fan's own samples -- three of those
  receivers() picks, three of the end column, which the device reproduces bit for bit -- so samples sit on depth lines;
* columns(S): the last, one inside, the source's own;
* the rays restated in Python (ray_subset): the first and the last surviving ray, the two with the most bounces, the one with
  the most samples outside the table's depths, then rays evenly spaced over the fan: 8 at the most, 2 of them (most samples
  outside the table, most bounces, among the rays whose look-ups extrapolate the table by at most AMP_MOST edge cells: beyond
  that ttk_independent's bound is vacuous) also given to the mpmath reference, up to 3 to the default-grid identity.  Where
  the references' estimated cost exceeds about 8 s the subset is halved (4 restated, 1 independent: ray_subset has the rule).

Level 1 (one test per case of CASES): the fan shot through the host-pointer entry (sample-major, stored sign), its status the
oracle's; travel_time_kernel_device on all surviving rays at each column: every row finite, zero at column 0, the restated rows
bit for bit against ttk_reference.kernel on the same raw arrays, the independent rows within ttk_independent's derived bound at
the last column (an entry with bound 0 exactly 0), the bound itself below 1e-9 max|K|.
Level 2 (the same test): the fan as a FanHandle: its samples the host-pointer shot's, travel_time_kernel of all M rows at each
column against the buffer entry, time_front at the columns and a repeated and an out-of-order one against
front_reference.gather / turning_points of fetch_samples(), and time_front_device on those arrays.
Level 3 (API_CASES x forwards / backwards x flatearth off / on): pr.travel_time_kernel at range_index -1 and S // 2 on the
device-resident fan (left in place) == on the host fan == ttk_reference.kernel fed by frame_independent.traced_frame; g is in
the user's coordinates, and the mirroring of a backwards fan (grid -g[::-1], result [:, ::-1]) is restated here.
ttk_reference.traced_tables and fan_kernel, which take the frame from the package, are not used.  Then turning_points,
time_front(k) and ray_ids of both fans against front_reference.
The default-grid identity, per raw case and per frame, on the identity rays: K on the traced table's own grid, bit for bit
against the restatement, and sum K cin = -(T_col - T_0) with cin from frame_independent; with flatearth=True also
sum (K F) cin_true, F = 1 + E (1 + E), the documented relation to the untransformed table.  rtol 1e-12 where the
restatement's own residual for that ray is <= 2.5e-13 (a factor 4 under), ray by ray; a ray above it is left out, and only in
the cases IDENTITY_LEFT_OUT names, with the reason.
The eigenrays of EIGEN_SEEDS, forwards: the dict's keys, shapes (M_j, A, B) and every row against the restatement.

cpu_check() re-runs everything that needs no device with the oracle's fan in the device's place (from the repository root:
PYTHONPATH=. python tests/test_ttk_random_env.py) and prints error / bound, bound / max|K| and the identity residual per case;
DESIGN.md section 4 records its output and the tallies of the MI355X run.  A seed on which the device disagrees is a finding
and stays in the list."""
import functools
import time

import numpy as np
import pytest

import frame_independent as fi
import front_reference as fr
import oracle
import ttk_independent as tti
import ttk_reference as ttr
from helpers import y0_for
from test_coherent_random_env import _Tables, api_case
from test_products_random_env import API_CASES, CASES, N_GRID, case_inputs, columns, receivers
from tube_gpu import _same, _upload, pr  # noqa: F401  (pr: fixture)

pytestmark = pytest.mark.gpu

A_CYCLE, B_CYCLE = (2, 5, 9, 14), (62, 63, 64, 127)
MOST_RESTATED, MOST_INDEPENDENT, MOST_IDENTITY = 8, 2, 3
IDENTITY_RTOL, RESIDUAL_CAP = 1e-12, 2.5e-13            # the assertion, and the restatement's own residual a factor 4 under it
VACUITY_CAP = 1e-9                                      # bound.max() < VACUITY_CAP * max|Ki| (test_travel_time_kernel.py's)
# An ESTIMATE of the references' cost, not a measurement: fixed rates in seconds per piece (pieces(): the grid lines a ray
# crosses) -- ttk_reference.kernel at three columns and ttk_independent.kernel per piece of the kernel grid, ttk_reference.kernel
# on the table's own grid per piece of that grid -- fitted once to timings of seeds 205, 215 and 409.  They keep the subset a
# fixed function of the seed; the estimate is rough (a case estimated under BUDGET_S has taken 11 s), and it stands in for
# "halve where the references need more than about 8 s".
SECONDS_PER_PIECE = dict(restated=4.5e-4, independent=1.3e-3, own=2.9e-4)
BUDGET_S, IDENTITY_S = 8.0, 3.0
AMP_MOST = 1e4                                          # 13 eps * 2 * AMP_MOST = 3e-11 of c: a tenth of the cap's room
# the cases in which a ray's restated default-grid residual exceeds RESIDUAL_CAP: that ray is left out of the identity (not of
# the bit comparison); the other identity rays of the case are asserted.  The figures are the restatement's own residuals on
# the oracle's fan, per identity ray, from cpu_check()
_WHY_202 = ("S = 3 and 40 % of the samples outside the table's depths: c is extrapolated there and weights of either sign cancel "
            "in K . cin; ")
IDENTITY_LEFT_OUT = {(202, False): _WHY_202 + "one ray of three at 8.1e-13"}
IDENTITY_LEFT_OUT_API = {(202, False, False): _WHY_202 + "7.3e-10 at the worst", (202, False, True): _WHY_202 + "2.3e-09",
                         (202, True, False): _WHY_202 + "2.6e-10", (202, True, True): _WHY_202 + "7.9e-13"}
assert len(IDENTITY_LEFT_OUT) <= 4 and len(IDENTITY_LEFT_OUT_API) <= 8
# the three API seeds whose forwards search finds the fewest eigenrays on the oracle's fan (eigen_reference's loop: 8, 15 and 10;
# the others 18 ... 137), because every row is restated in Python
EIGEN_SEEDS = (204, 209, 213)
QUANTILES = (0.2, 0.5, 0.8)


# ---- the inputs, from the oracle's fan alone ----------------------------------------------------------------------------------

def kernel_grid(idx, seed, x, rin, zs, deepest_floor):
    """-> (g (A,), h (B,)) of case number idx: x the save ranges (either direction) and rin the table's range lines, both in
    the coordinates g is wanted in; zs (M, S) the oracle fan's stored depths"""
    rng = np.random.default_rng(7000 + seed)
    A, B = A_CYCLE[idx % 4], B_CYCLE[(idx + idx // 4) % 4]
    x = np.asarray(x, dtype=float)
    lo, hi = float(min(x[0], x[-1])), float(max(x[0], x[-1]))
    nodes = [lo - rng.uniform(0.01, 0.05) * (hi - lo), hi + rng.uniform(0.01, 0.05) * (hi - lo)]
    if A > 2:
        on_save = float(x[len(x) // 2])
        lines = rin[(rin > lo) & (rin < hi) & (rin != on_save)]
        assert len(lines), "no table range line inside the fan"
        nodes += [on_save, float(lines[len(lines) // 2])]
    while len(set(nodes)) < A:
        nodes.append(float(rng.uniform(lo, hi)))
    g = np.array(sorted(set(nodes)))
    top, below = -120.0, deepest_floor + 150.0
    picks = receivers(zs, deepest_floor, seed)
    picks = picks[~np.isin(picks, np.linspace(top, below, N_GRID))]            # the depths receivers() took from the samples
    picks = picks[(picks > top) & (picks < below)]
    end = -np.asarray(zs)[:, -1]
    own = np.concatenate([picks[[len(picks) // 6, len(picks) // 2, (5 * len(picks)) // 6]],
                          rng.choice(end[(end > top) & (end < below)], 3, replace=False)])
    h = np.unique(np.concatenate([np.linspace(top, below, B - 6), own]))
    while len(h) < B:
        h = np.unique(np.append(h, rng.uniform(top, below)))
    assert len(g) == A and len(h) == B and h[0] == top and h[-1] == below
    return g, h


def pieces(zs, x, gr, gd):
    """the lines of the grid gr x gd every ray of zs (M, S) crosses from sample to sample, plus its chords: what a Python
    reference that walks the ray on that grid costs"""
    across = np.abs(np.diff(np.searchsorted(gd, -np.asarray(zs)), axis=1)).sum(axis=1)
    return across + int(np.abs(np.diff(np.searchsorted(gr, np.asarray(x)))).sum()) + len(x)


def amplification(zs, zin):
    """per ray of zs (M, S): how far its look-ups extrapolate the table in depth, in widths of the table's edge cell -- the
    |ty| of ttk_independent's item 4, whose bound on c grows by 13 eps |ty| c: beyond AMP_MOST the derived bound says little"""
    d = -np.asarray(zs)
    above, below = (zin[0] - d) / (zin[1] - zin[0]), (d - zin[-1]) / (zin[-1] - zin[-2])
    return np.maximum(np.maximum(above, below), 0.0).max(axis=1)


def ray_subset(zs, bounces, x, g, h, rin, zin, n_cols, independent=True):
    """-> (restated rays, independent rays, identity rays): rows of the surviving fan zs (M, S); x, g and rin in one frame.
    The references' seconds are estimated from pieces() at the rates SECONDS_PER_PIECE; over BUDGET_S the restated and the
    independent rays are halved (once: 4 and 1 are the least).  The identity rays are those of (most bounces, most samples
    outside the table, then the subset from its end) that fit IDENTITY_S together; where none does, the cheapest ray of the
    whole fan takes the subset's last place and is the identity ray."""
    M = len(zs)
    d = -np.asarray(zs)
    outside = ((d < zin[0]) | (d > zin[-1])).sum(axis=1)
    most_out = int(np.argmax(outside))
    bouncing = [int(v) for v in np.argsort(-np.asarray(bounces), kind="stable")[:2]]
    spaced = [int(v) for v in np.round(np.linspace(0, M - 1, MOST_RESTATED + 2))[1:-1]]
    sub = list(dict.fromkeys([0, M - 1] + bouncing + [most_out] + spaced))[:MOST_RESTATED]
    ind = []
    if independent:
        tame = amplification(zs, zin) <= AMP_MOST
        assert tame.any()
        out_tame = int(np.argmax(np.where(tame, outside, -1)))
        bounce_tame = int(np.argsort(-np.where(tame, np.asarray(bounces), -1), kind="stable")[0])
        ind = list(dict.fromkeys([out_tame, bounce_tame]))[:MOST_INDEPENDENT]
        sub = list(dict.fromkeys(ind + sub))[:MOST_RESTATED]
    small, own = pieces(zs, x, g, h), pieces(zs, x, rin, zin) * SECONDS_PER_PIECE["own"]
    seconds = small[sub].sum() * SECONDS_PER_PIECE["restated"] * n_cols / 3 + small[ind].sum() * SECONDS_PER_PIECE["independent"]
    if seconds > BUDGET_S:
        sub, ind = list(dict.fromkeys(ind[:1] + sub))[:MOST_RESTATED // 2], ind[:1]
    ident, spent = [], 0.0
    for m in dict.fromkeys([bouncing[0], most_out] + sub[::-1]):
        if m in sub and len(ident) < MOST_IDENTITY and spent + own[m] <= IDENTITY_S:
            ident.append(m)
            spent += own[m]
    if not ident:
        ident = [int(np.argmin(own))]
        sub = sub[:-1] + ident
    assert set(ind) <= set(sub) and set(ident) <= set(sub) and 4 <= len(sub) <= MOST_RESTATED
    return sub, ind, ident


def _oracle_fan(arrs, y0, x0, x1, S, shot):
    o = oracle.shoot_fan(*arrs, y0, x0, x1, S, math=oracle.MATH_CR, **shot)
    keep = o["status"] == 0
    return dict(status=o["status"], keep=keep, T=np.ascontiguousarray(o["T"][keep].T), Z=np.ascontiguousarray(-o["z"][keep].T),
                x=o["r"], bounces=(o["n_bott"] + o["n_surf"])[keep])


def _outside(Z, zin):
    d = -np.asarray(Z)
    return float(((d < zin[0]) | (d > zin[-1])).mean())


@functools.lru_cache(maxsize=None)
def raw_plan(seed, flat):
    """everything of a level-1 case that is chosen before the device runs"""
    idx = CASES.index((seed, flat))
    arrs, y0, kw, desc, mirrored = case_inputs(seed, flat)
    cin, cpin, rin, zin, bdep, brng, bang = arrs
    shot = dict(rtol=kw["rtol"], terminate_backwards=kw["terminate_backwards"])
    fan = _oracle_fan(arrs, y0, kw["x0"], kw["x1"], kw["S"], shot)
    g, h = kernel_grid(idx, seed, fan["x"], rin, fan["Z"].T, float(bdep.max()))
    sub, ind, ident = ray_subset(fan["Z"].T, fan["bounces"], fan["x"], g, h, rin, zin, len(columns(kw["S"])))
    return dict(arrs=arrs, y0=y0, kw=kw, shot=shot, desc=desc, mirrored=mirrored, fan=fan, g=g, h=h, sub=sub, ind=ind,
                ident=ident, cols=columns(kw["S"]), label=f"seed {seed}{' (flat earth)' if flat else ''}: {desc}")


@functools.lru_cache(maxsize=None)
def frame_plan(seed, lat, backwards, fe):
    """everything of a level-3 frame that is chosen before the device runs: the frame by frame_independent alone, the
    oracle's fan in it, g in the USER's coordinates"""
    idx = 4 * [s for s, _ in API_CASES].index(seed) + 2 * backwards + fe
    arrs, src, th, kw, desc = api_case(seed)
    S = kw["S"]
    xs, xr = (kw["x1"], kw["x0"]) if backwards else (kw["x0"], kw["x1"])
    x = -np.linspace(-xs, -xr, S) if backwards else np.linspace(xs, xr, S)          # (as shoot_rays saves)
    tables = _Tables(arrs, lat)
    xf, cin, rin, zin, bd, br = fi.traced_frame(tables, x, fe)
    frame_arrs = [cin, np.gradient(cin, zin, axis=1, edge_order=1), rin, zin, bd, br, fi.bottom_slope(tables, x)[1]]
    shot = dict(rtol=kw["rtol"], terminate_backwards=kw["terminate_backwards"])
    fan = _oracle_fan(frame_arrs, y0_for(oracle, frame_arrs, src, xf[0], -th), xf[0], xf[-1], S, shot)   # ODE angle: -theta
    g, h = kernel_grid(idx, seed, x, arrs[2], fan["Z"].T, float(bd.max()))
    sub, ind, ident = ray_subset(fan["Z"].T, fan["bounces"], xf, -g[::-1] if backwards else g, h, rin, zin, 2, independent=False)
    return dict(arrs=arrs, src=src, th=th, kw=kw, shot=shot, S=S, xs=xs, xr=xr, x=x, xf=xf, frame=(cin, rin, zin), fan=fan, g=g,
                h=h, sub=sub, ident=ident, tables=tables, backwards=backwards,
                label=f"seed {seed} {'backwards' if backwards else 'forwards'} flatearth={fe}: {desc}")


# ---- the references -------------------------------------------------------------------------------------------------------------

def restated(T, Z, x, g, h, frame, cols, rays):
    """ttk_reference.kernel of the rows `rays` of T / Z (S, M) at every column of cols -> {col: (len(rays), A, B)}"""
    cin, rin, zin = frame
    Tr, Zr = np.ascontiguousarray(T[:, rays]), np.ascontiguousarray(Z[:, rays])
    return {c: ttr.kernel(Tr, Zr, x, g, h, cin, rin, zin, c) for c in cols}


def independent(T, Z, x, g, h, frame, rays):
    """ttk_independent.kernel of the rows `rays` at the last column -> (Ki, bound)"""
    cin, rin, zin = frame
    Ki, _, bound = tti.kernel(np.ascontiguousarray(T[:, rays]), np.ascontiguousarray(Z[:, rays]), x, g, h, cin, rin, zin,
                              len(x) - 1)
    return Ki, bound


def within_bound(K, Ki, bound, label, check=True):
    """K against the independent reference -> (worst error / bound, bound / max|Ki|); the vacuity cap is a condition"""
    err = np.abs(K - Ki)
    cap = float(bound.max() / np.abs(Ki).max())
    if check:
        assert np.isfinite(K).all() and (err <= bound).all(), (label, "beyond the derived bound by", float(np.max(err - bound)))
        assert (K[bound == 0] == 0).all() and (K != 0).any(), (label, "an entry no piece touches is not 0, or K is 0 throughout")
        assert cap < VACUITY_CAP, (label, "the bound is vacuous", cap)
    lit = bound > 0
    return float(np.max(err[lit] / bound[lit])), cap


def residual(K, cin, T, col):
    """the default-grid identity's relative residual per ray: |sum K cin + (T_col - T_0)| / |T_col - T_0|; T (S, rays)"""
    lhs = (K * cin[None]).sum(axis=(1, 2))
    rhs = -(T[col] - T[0])
    return np.abs(lhs - rhs) / np.abs(rhs)


def flat_factor(zin_true, lat):
    """F_b = 1 + E_b (1 + E_b), E_b = z_b / R_e(lat): the flat-earth table's node (a, b) is the true one's times F_b"""
    e = np.asarray(zin_true, dtype=float) / fi.earth_radius(lat)
    return 1.0 + e * (1.0 + e)


def raw_references(plan, T, Z):
    """every expectation of a level-1 case on the fan rows T / Z (S, M): the oracle's in cpu_check, the device's in the test"""
    cin, cpin, rin, zin = plan["arrs"][:4]
    frame, x, g, h = (cin, rin, zin), plan["fan"]["x"], plan["g"], plan["h"]
    S = len(x)
    ref = restated(T, Z, x, g, h, frame, plan["cols"], plan["sub"])
    Ki, bound = independent(T, Z, x, g, h, frame, plan["ind"])
    own = restated(T, Z, x, rin, zin, frame, [S - 1], plan["ident"])[S - 1]
    return dict(ref=ref, Ki=Ki, bound=bound, own=own, residual=residual(own, cin, T[:, plan["ident"]], S - 1))


def figures(plan, r):
    """the restatement alone against the independent reference, and the fill of K -> dict"""
    S = len(plan["fan"]["x"])
    rows = [plan["sub"].index(m) for m in plan["ind"]]
    ratio, cap = within_bound(r["ref"][S - 1][rows], r["Ki"], r["bound"], plan["label"], check=False)
    zero_ok = bool((r["ref"][S - 1][rows][r["bound"] == 0] == 0).all())
    return dict(err_over_bound=ratio, bound_over_K=cap, zero_ok=zero_ok, residual=float(r["residual"].max()),
                residuals=[float(v) for v in r["residual"]],
                fill=float((r["ref"][S - 1] != 0).mean()))


def cpu_check(level1=True, level3=True):
    """The restatement-alone pre-check, no device: per case error / bound, the vacuity cap and the identity residual on the
    oracle's fan, the seconds the references take, and the conditions the tallies assert."""
    out = []
    if level1:
        n_out = 0
        for seed, flat in CASES:
            t = time.time()
            plan = raw_plan(seed, flat)
            fan = plan["fan"]
            fig = figures(plan, raw_references(plan, fan["T"], fan["Z"]))
            share = _outside(fan["Z"], plan["arrs"][3])
            n_out += share > 0.01
            left = (seed, flat) in IDENTITY_LEFT_OUT
            if not left and fig["residual"] > RESIDUAL_CAP:
                out.append(((seed, flat), f"residual {fig['residual']:.2e} > {RESIDUAL_CAP} and not in IDENTITY_LEFT_OUT"))
            if not fig["fill"] > 0:
                out.append(((seed, flat), "K is 0 throughout"))
            if not (fig["err_over_bound"] <= 1 and fig["bound_over_K"] < VACUITY_CAP and fig["zero_ok"]):
                out.append(((seed, flat), f"the restatement against the independent reference: {fig}"))
            print(f"seed {seed} flat {flat!s:5s} {time.time() - t:5.1f} s  A {len(plan['g']):2d} B {len(plan['h']):3d} rays "
                  f"{len(plan['sub'])}/{len(plan['ind'])}/{len(plan['ident'])} error/bound {fig['err_over_bound']:.3f} "
                  f"bound/max|K| {fig['bound_over_K']:.2e} residual {' '.join(f'{v:.2e}' for v in fig['residuals'])}"
                  f"{' (those above the cap left out)' if left else ''} "
                  f"fill {fig['fill']:.3f} outside the table {share:.3f}", flush=True)
        print(f"level 1: {n_out} cases with more than 1 % of their samples outside the table's depths")
        if n_out < 10:
            out.append(("level 1", f"{n_out} < 10 cases with samples outside the table"))
    if level3:
        for seed, lat in API_CASES:
            for backwards in (False, True):
                for fe in (False, True):
                    t = time.time()
                    plan = frame_plan(seed, lat, backwards, fe)
                    fan, S, key = plan["fan"], plan["S"], (seed, backwards, fe)
                    r = frame_references(plan, fan["T"], fan["Z"], lat, fe)
                    left = key in IDENTITY_LEFT_OUT_API
                    worst = np.maximum(r["residual"], r["residual_F"]) if fe else r["residual"]
                    if not left and float(worst.max()) > RESIDUAL_CAP:
                        out.append((key, f"residual {worst.max():.2e} > {RESIDUAL_CAP} and not in IDENTITY_LEFT_OUT_API"))
                    print(f"API seed {seed} backwards {backwards!s:5s} flatearth {fe!s:5s} {time.time() - t:5.1f} s  A "
                          f"{len(plan['g']):2d} B {len(plan['h']):3d} rays {len(plan['sub'])}/{len(plan['ident'])} residual "
                          f"{' '.join(f'{v:.2e}' for v in worst)}{' (those above the cap left out)' if left else ''} fill {(r['ref'][S - 1] != 0).mean():.3f}",
                          flush=True)
    print("missed:", out)
    return out


def frame_references(plan, T, Z, lat, fe):
    """every expectation of a level-3 frame on the fan rows T / Z (S, M), in the USER's axis order"""
    cin, rin, zin = plan["frame"]
    xf, S, back = plan["xf"], plan["S"], plan["backwards"]
    gf = -plan["g"][::-1] if back else plan["g"]                                  # the mirroring, restated
    ref = restated(T, Z, xf, gf, plan["h"], plan["frame"], [S - 1, S // 2], plan["sub"])
    own = restated(T, Z, xf, rin, zin, plan["frame"], [S - 1], plan["ident"])[S - 1]
    if back:
        ref, own = {c: K[:, ::-1] for c, K in ref.items()}, own[:, ::-1]
    user_cin = fi.tables(plan["tables"], fe)[0]                                   # the un-mirrored table: the user's order
    res = residual(own, user_cin, T[:, plan["ident"]], S - 1)
    res_F = None
    if fe:
        F = flat_factor(plan["arrs"][3], lat)
        res_F = residual(own * F[None, None, :], fi.tables(plan["tables"], False)[0], T[:, plan["ident"]], S - 1)
    return dict(ref=ref, own=own, residual=res, residual_F=res_F, user_cin=user_cin)


# ---- levels 1 and 2: the kernel on raw tables and the fan entries ---------------------------------------------------------------

def _device_kernel(env, T, Z, x, g, h, col):
    import torch
    from pygenray_amd import _lib
    t, stream = _upload(env, T, Z, x, g, h)
    S, M = T.shape
    out = torch.full((M, len(g), len(h)), -1.0, dtype=torch.float64, device=t[0].device)
    _lib.travel_time_kernel_device(env, t[0].data_ptr(), t[1].data_ptr(), M, S, t[2].data_ptr(), t[3].data_ptr(), len(g),
                                   t[4].data_ptr(), len(h), col, out.data_ptr(), stream)
    return out.cpu().numpy()


def _fan_kernel(h, env, g, d, col):
    import torch
    (d_g, d_h), stream = _upload(env, g, d)
    out = torch.full((h.M, len(g), len(d)), -1.0, dtype=torch.float64, device=d_g.device)
    h.travel_time_kernel(d_g.data_ptr(), len(g), d_h.data_ptr(), len(d), col, out.data_ptr(), stream)
    return out.cpu().numpy()


def _fronts(env, M, cols, call):
    """the four outputs [len(cols)][M] of a time-front entry `call(cols, t, z, p, turns pointers, stream)` -> host arrays"""
    import torch
    dev = torch.device("cuda", env.device)
    outs = [torch.full((len(cols), M), -7.25, dtype=torch.float64, device=dev) for _ in range(3)]
    outs.append(torch.full((len(cols), M), -77, dtype=torch.int32, device=dev))
    call(cols, *(o.data_ptr() for o in outs), torch.cuda.current_stream(dev).cuda_stream)
    return [o.cpu().numpy() for o in outs]


def _identity(K, cin, T, col, restated, allowed, label):
    """sum K cin = -(T_col - T_0) at IDENTITY_RTOL for every ray (rows of K, columns of T) whose restated residual is within
    RESIDUAL_CAP; a ray above it is left out, which only a case named in IDENTITY_LEFT_OUT(_API) (`allowed`) may have
    -> (rays asserted, rays left out, the largest restated residual among the asserted)"""
    keep = np.asarray(restated) <= RESIDUAL_CAP
    assert allowed or keep.all(), (label, "the restatement's own residual", restated)
    if keep.any():
        lhs = (K[keep] * cin[None]).sum(axis=(1, 2))
        np.testing.assert_allclose(lhs, -(T[col, keep] - T[0, keep]), rtol=IDENTITY_RTOL, atol=0, err_msg=str(label))
    return int(keep.sum()), int((~keep).sum()), float(np.max(np.asarray(restated)[keep], initial=0.0))


_RECORDS = {}


def _level1(pr, seed, flat):  # noqa: F811
    if (seed, flat) in _RECORDS:
        return _RECORDS[(seed, flat)]
    from pygenray_amd import _lib
    plan = raw_plan(seed, flat)
    arrs, y0, kw, shot, label = plan["arrs"], plan["y0"], plan["kw"], plan["shot"], plan["label"]
    cin, cpin, rin, zin, bdep, brng, bang = arrs
    g, h, cols, sub, S = plan["g"], plan["h"], plan["cols"], plan["sub"], kw["S"]
    env = _lib.EnvHandle(*arrs)
    shot_fan = env.shoot_fan(y0, kw["x0"], kw["x1"], S, sample_major=True, stored_sign=True, **shot)
    assert np.array_equal(shot_fan["status"], plan["fan"]["status"]), (label, "the fan's status is not the oracle's")
    keep = shot_fan["status"] == 0
    M = int(keep.sum())
    assert M >= 64, label
    T, Z, P = (np.ascontiguousarray(shot_fan[k][:, keep]) for k in "Tzp")          # (S, M)
    x = shot_fan["r"]
    assert np.isfinite(T).all() and np.isfinite(Z).all() and _same(x, plan["fan"]["x"]), label
    assert _same(Z[-1], plan["fan"]["Z"][-1]), (label, "the end depths are not the oracle's")
    on_lines = int(np.isin(-Z, h).sum())
    assert on_lines >= 3, (label, "samples on depth lines", on_lines)
    # level 1: the buffer entry against the restatement and the independent reference
    r = raw_references(plan, T, Z)
    K = {c: _device_kernel(env, T, Z, x, g, h, c) for c in cols}
    for c in cols:
        assert K[c].shape == (M, len(g), len(h)) and np.isfinite(K[c]).all(), (label, "column", c)
        bad = ~((K[c][sub] == r["ref"][c]) | (np.isnan(K[c][sub]) & np.isnan(r["ref"][c])))
        assert not bad.any(), (label, "column", c, int(bad.sum()), np.argwhere(bad)[:5].tolist(), K[c][sub][bad][:5],
                               r["ref"][c][bad][:5])
    assert (K[0] == 0).all(), (label, "column 0")
    ratio, cap = within_bound(K[S - 1][plan["ind"]], r["Ki"], r["bound"], label)
    fill = float((K[S - 1] != 0).mean())
    assert fill > 0, (label, "K is 0 throughout")
    # the default-grid identity on the identity rays
    Ti, Zi = np.ascontiguousarray(T[:, plan["ident"]]), np.ascontiguousarray(Z[:, plan["ident"]])
    own = _device_kernel(env, Ti, Zi, x, rin, zin, S - 1)
    assert _same(own, r["own"]), (label, "the default grid")
    asserted, left_out, res = _identity(own, cin, Ti, S - 1, r["residual"], (seed, flat) in IDENTITY_LEFT_OUT, label)
    # level 2: the fan entries
    fan = _lib.FanHandle(env, kw["x0"], kw["x1"], S, y0=y0, stored_sign=True, **shot)
    assert fan.wait() == (len(y0), M), label
    samples = fan.fetch_samples()
    for k, a in (("T", T), ("z", Z), ("p", P)):
        assert _same(samples[k], a), (label, "fetch_samples", k)
    for c in cols:
        assert _same(_fan_kernel(fan, env, g, h, c), K[c]), (label, "FanHandle.travel_time_kernel, column", c)
    tf_cols = cols + [cols[0], min(1, S - 1)]                                   # a repeated and an out-of-order column
    want = [fr.gather(samples[k].T, tf_cols).T for k in "Tzp"] + [fr.turning_points(samples["p"].T, tf_cols).T]
    got = _fronts(env, M, tf_cols, fan.time_front)
    d_rows, _ = _upload(env, samples["T"], samples["z"], samples["p"])
    buf = _fronts(env, M, tf_cols, lambda cs, *a: _lib.time_front_device(env.device, *(t.data_ptr() for t in d_rows), M, S, cs, *a))
    for name, w, a, b in zip(("T", "z", "p", "turns"), want, got, buf):
        assert a.shape == w.shape and _same(a, w), (label, "FanHandle.time_front", name)
        assert b.shape == w.shape and _same(b, w), (label, "time_front_device", name)
    fan.close()
    nonuniform = float(np.ptp(np.diff(rin))) > 1e-6 * float(np.mean(np.diff(rin)))
    offset = abs(rin[-1] if plan["mirrored"] else rin[0])
    rec = dict(hbm=not env.lds_path, lds=env.lds_path, blocked=env.blocked_layout, mirrored=plan["mirrored"], offset=offset > 100e3,
               nonuniform=nonuniform, flat=flat, dropped=M < len(y0), outside=_outside(Z, zin) > 0.01, rays=M, on_lines=on_lines,
               turns=int(want[3].max()), fill=fill, err_over_bound=ratio, bound_over_K=cap, residual=res, asserted=asserted, left_out=left_out,
               residual_left_out=[float(v) for v in r["residual"] if v > RESIDUAL_CAP])
    env.close()
    print(f"\n{label}: A {len(g)} B {len(h)} {rec}")
    _RECORDS[(seed, flat)] = rec
    return rec


@pytest.mark.parametrize("seed, flat", CASES, ids=[f"seed{s}{'-flat' if fl else ''}" for s, fl in CASES])
def test_kernel_and_fan_entries_on_random_raw_tables(pr, seed, flat):  # noqa: F811
    _level1(pr, seed, flat)


def test_the_sweep_holds_what_it_is_meant_to(pr):  # noqa: F811
    """the tallies over the level-1 cases (each case's record is kept by its own test; a case not run yet is run here)"""
    recs = [_level1(pr, seed, flat) for seed, flat in CASES]
    keys = ("hbm", "lds", "blocked", "mirrored", "offset", "nonuniform", "flat", "dropped", "outside", "rays", "asserted")
    tally = {k: int(sum(rec[k] for rec in recs)) for k in keys}
    tally["left_out"] = sum(rec["left_out"] > 0 for rec in recs)                 # cases with an identity ray left out
    print(f"\n{len(recs)} random environments: {tally}; fill of K {min(r['fill'] for r in recs):.4f} ... "
          f"{max(r['fill'] for r in recs):.4f}; worst error / bound {max(r['err_over_bound'] for r in recs):.3f}; worst bound / "
          f"max|K| {max(r['bound_over_K'] for r in recs):.2e}; the restatement's identity residual "
          f"{max(r['residual'] for r in recs):.2e} at the most on the {tally['asserted']} rays asserted, "
          f"{[f'{v:.2e}' for r in recs for v in r['residual_left_out']]} on the rays left out; most turning points "
          f"{min(r['turns'] for r in recs)} ... {max(r['turns'] for r in recs)}")
    for k, least in (("hbm", 6), ("lds", 6), ("blocked", 6), ("mirrored", 6), ("offset", 6), ("nonuniform", 6), ("flat", 6),
                     ("dropped", 4), ("outside", 10)):
        assert tally[k] >= least, (k, tally)
    assert all(r["fill"] > 0 for r in recs) and tally["left_out"] <= 4, tally


# ---- level 3: the API in four frames ----------------------------------------------------------------------------------------------

def _in_place(fan):
    assert fan.device_resident and not any(k in fan.__dict__ for k in ("_ts", "_zs", "_ps"))


def _environment(pr, arrs, lat):  # noqa: F811
    cin, cpin, rin, zin, bdep, brng, bang = arrs
    return pr.OceanEnvironment2D(pr.DataArray(cin, dims=["range", "depth"], coords={"range": rin, "depth": zin}),
                                 pr.DataArray(bdep, dims=["range"], coords={"range": brng}), lat=lat)


def _check_fronts(dev, host, label):
    """the checks of test_time_front._check_device_fan on a fan of any S: turning_points, time_front(k) and ray_ids of the
    device-resident fan against front_reference on the host fan's arrays; the device fan stays where it is"""
    M, S = np.shape(host.ps)
    assert len(dev) == M and _same(dev.thetas, host.thetas), label
    cols = [0, min(1, S - 1), S // 2, S - 1, S // 2, min(3, S - 1)]
    want = fr.turning_points(host.ps, cols)
    got = dev.turning_points([0, min(1, S - 1), S // 2, -1, S // 2, min(3, S - 1)])
    assert got.dtype == np.int64 and np.array_equal(got, want), (label, "turning_points")
    assert np.array_equal(dev.turning_points(), want[:, 3:4]) and np.array_equal(host.turning_points(cols), want), label
    for k in (S // 3, 0, -1):
        tf, kk = dev.time_front(k), k % S
        assert tf.range_index == kk and _same(tf.range, host.time_front(k).range) and np.all(tf.range == np.asarray(host.rs)[0][kk]), (label, k)
        for name, a in (("t", host.ts), ("z", host.zs), ("p", host.ps)):
            assert _same(getattr(tf, name), fr.gather(a, [kk])[:, 0]), (label, "time_front", k, name)
        assert tf.turning_points.dtype == np.int64 and np.array_equal(tf.turning_points, want[:, 3] if kk == S - 1 else
                                                                      fr.turning_points(host.ps, [kk])[:, 0]), (label, k)
        assert _same(tf.thetas, host.thetas) and _same(tf.ray_numbers, host.time_front(k).ray_numbers), (label, k)
        assert (tf.ray_ids is None) if kk != S - 1 else np.array_equal(tf.ray_ids, host.ray_ids), (label, k)
    ids = fr.ray_id_strings(host.ps, host.thetas, host.n_botts, host.n_surfs)
    assert dev.ray_ids.dtype.kind == "U" and np.array_equal(dev.ray_ids, ids) and np.array_equal(host.ray_ids, ids), label
    dev.compute_rayids()
    assert np.array_equal(dev.ray_ids, ids), (label, "compute_rayids")
    assert np.array_equal(dev.turning_points(cols), want), (label, "turning_points, a second time")
    _in_place(dev)
    return int(want[:, 3].max())


_API_RECORDS = {}


def _level3(pr, seed, lat, backwards, fe):  # noqa: F811
    key = (seed, backwards, fe)
    if key in _API_RECORDS:
        return _API_RECORDS[key]
    plan = frame_plan(seed, lat, backwards, fe)
    label, S, g, h, sub, ident = plan["label"], plan["S"], plan["g"], plan["h"], plan["sub"], plan["ident"]
    env = _environment(pr, plan["arrs"], lat)
    host, dev = (pr.shoot_rays(plan["src"], plan["xs"], plan["th"], plan["xr"], S, env, debug=False, flatearth=fe,
                               device_resident=dr, **plan["shot"]) for dr in (False, True))
    assert not host.device_resident and dev.device_resident and len(host) == len(dev) >= 64, label
    assert _same(host.thetas, plan["th"][plan["fan"]["keep"]]), (label, "the surviving rays are not the oracle's")
    x = np.asarray(host.rs, dtype=float)[0]
    assert _same(x, plan["x"]) and x[0] == plan["xs"] and x[-1] == plan["xr"] and np.all(np.diff(g) > 0), label
    assert len(g) == 2 or (x[S // 2] in g and np.isin(plan["arrs"][2], g).any()), (label, "the nodes on a save range and a line")
    T, Z = np.ascontiguousarray(np.asarray(host.ts).T), np.ascontiguousarray(np.asarray(host.zs).T)
    r = frame_references(plan, T, Z, lat, fe)
    for c in (-1, S // 2):
        Kd = pr.travel_time_kernel(dev, env, g, h, flatearth=fe, range_index=c)
        _in_place(dev)                                                             # processed where it is, nothing fetched
        Kh = pr.travel_time_kernel(host, env, g, h, flatearth=fe, range_index=c)
        assert Kd.shape == (len(host), len(g), len(h)) and _same(Kd, Kh), (label, "device fan against host fan, range_index", c)
        want = r["ref"][c % S]
        bad = ~((Kh[sub] == want) | (np.isnan(Kh[sub]) & np.isnan(want)))
        assert not bad.any(), (label, "range_index", c, int(bad.sum()), np.argwhere(bad)[:5].tolist(), Kh[sub][bad][:5], want[bad][:5])
        assert (Kh != 0).any(), (label, "K is 0 throughout")
    # the default grid: the identity rays as a host fan of their own (the whole fan's K on the table would be ~1 GB)
    few = pr.RayFan.from_arrays(*(np.asarray(getattr(host, n))[ident] for n in ("thetas", "rs", "ts", "zs", "ps", "n_botts",
                                                                              "n_surfs", "source_depths")))
    own = pr.travel_time_kernel(few, env, flatearth=fe)
    assert own.shape == (len(ident),) + r["user_cin"].shape and _same(own, r["own"]), (label, "the default grid")
    Ti, named = T[:, ident], key in IDENTITY_LEFT_OUT_API
    asserted, left_out, res = _identity(own, r["user_cin"], Ti, S - 1, r["residual"], named, label)
    if fe:
        F = flat_factor(plan["arrs"][3], lat)
        a_F, l_F, res_F = _identity(own * F[None, None, :], fi.tables(plan["tables"], False)[0], Ti, S - 1, r["residual_F"], named,
                                    (label, "K F on the true table"))
        asserted, left_out, res = asserted + a_F, left_out + l_F, max(res, res_F)
    turns = _check_fronts(dev, host, label)
    rec = dict(residual=res, asserted=asserted, left_out=left_out, turns=turns, rays=len(host))
    print(f"\n{label}: A {len(g)} B {len(h)} {rec}")
    _API_RECORDS[key] = rec
    return rec


@pytest.mark.parametrize("fe", [False, True], ids=["flatearth-off", "flatearth-on"])
@pytest.mark.parametrize("backwards", [False, True], ids=["forwards", "backwards"])
@pytest.mark.parametrize("seed, lat", API_CASES, ids=[f"seed{s}" for s, _ in API_CASES])
def test_api_kernel_against_frames_derived_by_hand(pr, seed, lat, backwards, fe):  # noqa: F811
    _level3(pr, seed, lat, backwards, fe)


@pytest.mark.parametrize("seed", EIGEN_SEEDS, ids=[f"seed{s}" for s in EIGEN_SEEDS])
def test_eigenrays_kernel_against_the_restatement(pr, seed):  # noqa: F811
    """pr.find_eigenrays at the depth quantiles QUANTILES of the ORACLE fan's end depths, forwards, flatearth on for every
    second seed; then travel_time_kernel of the EigenRays: one (M_j, A, B) block per receiver depth, every row the
    restatement of the eigenray's own ts / zs in the frame frame_independent derives"""
    lat = dict(API_CASES)[seed]
    fe = bool(EIGEN_SEEDS.index(seed) % 2)
    plan = frame_plan(seed, lat, False, fe)
    label, S, g, h = plan["label"] + " (eigenrays)", plan["S"], plan["g"], plan["h"]
    rds = [float(q) for q in np.quantile(-plan["fan"]["Z"][-1], QUANTILES)]
    env = _environment(pr, plan["arrs"], lat)
    fan = pr.shoot_rays(plan["src"], plan["xs"], plan["th"], plan["xr"], S, env, debug=False, flatearth=fe, device_resident=False,
                        **plan["shot"])
    er = pr.find_eigenrays(fan, rds, plan["src"], plan["xs"], plan["xr"], S, env, ztol=1, max_iter=20, quiet=True, flatearth=fe,
                           **plan["shot"])
    K = pr.travel_time_kernel(er, env, g, h, flatearth=fe)
    assert sorted(K) == list(range(len(rds))), label
    total = 0
    for j in range(len(rds)):
        n = len(er.launch_angles[j])
        assert K[j].shape == (n, len(g), len(h)), (label, j)
        if not n:
            continue
        ts, zs = np.asarray(er.ts[j], dtype=float).reshape(n, S), np.asarray(er.zs[j], dtype=float).reshape(n, S)
        want = restated(np.ascontiguousarray(ts.T), np.ascontiguousarray(zs.T), plan["xf"], g, h, plan["frame"], [S - 1],
                        list(range(n)))[S - 1]
        assert _same(K[j], want) and (K[j] != 0).any(), (label, "receiver depth", j)
        total += n
    print(f"\n{label}: {total} eigenrays")
    assert total >= 4, (label, total)


def test_the_api_sweep_holds_what_it_is_meant_to(pr):  # noqa: F811
    """the tallies over the 48 frames (each frame's record is kept by its own test; a frame not run yet is run here)"""
    recs = [_level3(pr, seed, lat, backwards, fe) for seed, lat in API_CASES for backwards in (False, True) for fe in (False, True)]
    left = sum(r["left_out"] > 0 for r in recs)
    print(f"\n{len(recs)} frames: {sum(r['rays'] for r in recs)} rays; the restatement's identity residual "
          f"{max(r['residual'] for r in recs):.2e} at the most on the {sum(r['asserted'] for r in recs)} identities asserted, "
          f"{sum(r['left_out'] for r in recs)} left out in {left} frames; most turning "
          f"points {min(r['turns'] for r in recs)} ... {max(r['turns'] for r in recs)}")
    assert 6 * left <= len(recs), left


if __name__ == "__main__":
    cpu_check()
