"""The bounce log of the fan kernel and the boundary loss formed from it, on the GPU: the log against the
oracle's step trace bit for bit, a logged fan against the unlogged one, the log's capacity, the post-pass kernels against the
NumPy restatement (tests/bounce_reference.py) on synthetic logs, the sample assignment against the oracle's segments, and the
amplitude products with boundary loss against their restatements fed the weights."""
import numpy as np
import pytest

import bounce_reference as bref
import frame_independent as fi
import oracle
import path_reference as pref
import tl_reference as tlr
from helpers import y0_for
from tube_gpu import DEPTHS, SYN_R, SYN_Z, _env, _p_with_pc, _same, munk_env, pr, pr_any, sloping_env, syn_cin  # noqa: F401

pytestmark = pytest.mark.gpu

X_SMALL, S_SMALL, N_SMALL = 30e3, 13, 200
X_BIG, S_BIG, N_BIG, EVERY = 6e3, 5, 8 * 256 * 64 + 65, 300


def munk(z, axis):
    eta = 2.0 * (z - axis) / 1300.0
    return 1500.0 * (1.0 + 0.00737 * (eta - 1.0 + np.exp(-eta)))


def small_arrays(which):
    """the environments of the small fan: `lds` (one profile: LDS table), `hbm` (range dependent: tables in HBM, sample
    blocked), `slope` (LDS table over a sloping bottom) -- 4800 m deep, as the instance walk of test_hip_parity.py"""
    z = np.arange(0, 6000, 1.0)
    r = np.linspace(0.0, 40e3, 7)
    cin = np.array([munk(z, 1300.0 + (4e-3 * ri if which == "hbm" else 0.0)) for ri in r])
    cpin = np.gradient(cin, z, axis=1, edge_order=1)
    if which == "slope":
        depths = 4800.0 - 0.02 * r
        angles = np.degrees(np.arctan(np.gradient(depths, r)))
    else:
        depths, angles = np.full(7, 4800.0), np.zeros(7)
    return [cin, cpin, r, z, depths, r.copy(), angles]


def handle_outputs(h, save=True):
    out = h.fetch_rays()
    if save:
        out.update(h.fetch_samples(compact=False))
    return out


def oracle_log(arrs, y0, x1, K):
    """(bx, bp, bk) [len(y0)][K] and counts from the oracle's trace, filled like the kernel's log"""
    n = len(y0)
    bx, bp, bk = np.full((n, K), np.nan), np.full((n, K), np.nan), np.full((n, K), -1, np.int8)
    cnt = np.zeros(n, np.int64)
    for i in range(n):
        x, p, k = bref.trace_bounces(arrs, y0[i], 0.0, x1)
        cnt[i] = len(x)
        m = min(len(x), K)
        bx[i, :m], bp[i, :m], bk[i, :m] = x[:m], p[:m], k[:m]
    return bx, bp, bk, cnt


@pytest.fixture(scope="module")
def lib(pr):  # noqa: F811
    from pygenray_amd import _lib
    return _lib


@pytest.fixture(scope="module")
def small_cases(lib):
    """per environment: arrays, y0, the unlogged and the logged (K = 24) fan's outputs, the fetched log, the oracle's log"""
    cases = {}
    for which in ("lds", "hbm", "slope"):
        arrs = small_arrays(which)
        env = lib.EnvHandle(*arrs)
        y0 = y0_for(oracle, arrs, 900.0, 0.0, np.linspace(-19.5, 19.5, N_SMALL))
        plain = lib.FanHandle(env, 0.0, X_SMALL, S_SMALL, y0=y0)
        ref = handle_outputs(plain)
        assert env.last_instance_log() == 0
        plain.close()
        logged = lib.FanHandle(env, 0.0, X_SMALL, S_SMALL, y0=y0, max_bounces=24)
        got = handle_outputs(logged)
        li = env.last_instance()
        assert env.last_instance_log() == 1 and (li["lds_tab"], li["save"], li["persist"]) == ((1, 1, 0) if which != "hbm" else (0, 3, 0))
        log = logged.fetch_bounces()
        logged.close()
        cases[which] = dict(arrs=arrs, env=env, y0=y0, ref=ref, got=got, log=log, oracle=oracle_log(arrs, y0, X_SMALL, 24))
    yield cases
    for c in cases.values():
        c["env"].close()


@pytest.mark.parametrize("which", ["lds", "hbm", "slope"])
def test_log_is_the_oracle_trace_bit_for_bit_and_the_logged_fan_is_the_unlogged_fan(small_cases, which):
    c = small_cases[which]
    for k in c["ref"]:
        assert _same(c["ref"][k], c["got"][k]), k                 # status, counts, n_steps, n_rej, end states, samples
    ok = c["ref"]["status"] == 0
    assert ok.sum() > 150
    bx, bp, bk = (a.T for a in c["log"])                           # (M, K) over the surviving rays
    ox, op, ok_, cnt = (a[ok] for a in c["oracle"])
    total = (c["ref"]["n_bott"] + c["ref"]["n_surf"])[ok]
    assert (total > 0).sum() > 20 and ((c["ref"]["n_bott"][ok] > 0) & (c["ref"]["n_surf"][ok] > 0)).any() and total.max() <= 24
    assert np.array_equal(cnt, total) and np.array_equal((bk >= 0).sum(axis=1), total)
    assert _same(bx, ox) and _same(bp, op) and np.array_equal(bk, ok_)        # (no PGR_STORED_SIGN here: the ODE sign)
    assert np.array_equal((bk == 1).sum(axis=1), c["ref"]["n_bott"][ok]) and np.array_equal((bk == 0).sum(axis=1), c["ref"]["n_surf"][ok])


@pytest.mark.parametrize("which", ["lds", "hbm"])
def test_persistent_logged_instances(lib, which):
    arrs = small_arrays(which)
    env = lib.EnvHandle(*arrs)
    y0 = y0_for(oracle, arrs, 900.0, 0.0, np.linspace(-19.5, 19.5, N_BIG))
    plain = lib.FanHandle(env, 0.0, X_BIG, S_BIG, y0=y0)
    ref = handle_outputs(plain)
    plain.close()
    logged = lib.FanHandle(env, 0.0, X_BIG, S_BIG, y0=y0, max_bounces=6)
    got = handle_outputs(logged)
    li = env.last_instance()
    assert env.last_instance_log() == 1 and (li["lds_tab"], li["save"], li["persist"]) == ((1, 1, 1) if which == "lds" else (0, 3, 1))
    for k in ref:
        assert _same(ref[k], got[k]), k
    bx, bp, bk = (a.T for a in logged.fetch_bounces())
    logged.close()
    ok = ref["status"] == 0
    sub = np.arange(0, N_BIG, EVERY)
    sub = sub[ok[sub]]
    row = (np.cumsum(ok) - 1)[sub]                                 # where the surviving ray sits in the fetched log
    assert len(sub) > 400 and len(bk) == ok.sum()
    ox, op, ok_, cnt = oracle_log(arrs, y0[sub], X_BIG, 6)
    assert (cnt > 0).sum() > 20 and cnt.max() <= 6 and np.array_equal(cnt, (ref["n_bott"] + ref["n_surf"])[sub])
    assert _same(bx[row], ox) and _same(bp[row], op) and np.array_equal(bk[row], ok_)
    env.close()


def test_every_log_instance_is_launched_and_equals_the_unlogged_fan(lib, pr):  # noqa: F811
    """The 24 LOG instances of pgr_fan_kernel (csrc/pgr_launch.h, fan_instance_exists): <LDS table, SAVE 1> and <HBM tables,
    SAVE 3> for the six depth look-ups and both PERSIST values.  The environments are those of the instance walk of
    test_hip_parity.py (its `grids`: depth grid and PGR_OPT_DEPTH_SEARCH per ZM, range-independent / range-dependent
    tables), the fans its small and its persistent one.  Each launch is confirmed to be the instance it was meant to be, the
    logged fan is the unlogged fan of the same launch bit for bit, and the log holds n_bott + n_surf slots per ray."""
    z1 = np.arange(0, 6000, 1.0)
    depf = pr.eflat(z1, 35.0, pr.munk_ssp(z1))[0]               # the flat-earth image of a uniform grid: smooth, non-uniform
    grids = {4: (z1, 0), 1: (np.arange(0, 6000, 2.0), 0), 5: (depf, 0), 3: (depf, 3), 2: (depf, 2), 0: (depf, 1)}   # zm -> (zin, PGR_OPT_DEPTH_SEARCH)
    seen = set()
    for lds in (1, 0):
        for zm, (zin, search) in grids.items():
            r = np.linspace(0.0, 40e3, 7)
            cin = np.array([munk(zin, 1300.0 + (0.0 if lds else 4e-3 * ri)) for ri in r])
            arrs = [cin, np.gradient(cin, zin, axis=1, edge_order=1), r, zin, np.full(7, 4800.0), r.copy(), np.zeros(7)]
            env = lib.EnvHandle(*arrs)
            env.set_option("depth_search", search)
            for persist, (n, x1, S, K) in enumerate(((N_SMALL, X_SMALL, S_SMALL, 24), (N_BIG, X_BIG, S_BIG, 6))):
                want = (lds, zm, 1 if lds else 3, persist)
                y0 = y0_for(oracle, arrs, 900.0, 0.0, np.linspace(-19.5, 19.5, n))
                plain = lib.FanHandle(env, 0.0, x1, S, y0=y0)
                ref = handle_outputs(plain)
                li = env.last_instance()
                assert (li["lds_tab"], li["zm"], li["save"], li["persist"], env.last_instance_log()) == want + (0,), (want, li)
                plain.close()
                logged = lib.FanHandle(env, 0.0, x1, S, y0=y0, max_bounces=K)
                got = handle_outputs(logged)
                li = env.last_instance()
                assert (li["lds_tab"], li["zm"], li["save"], li["persist"], env.last_instance_log()) == want + (1,), (want, li)
                seen.add(want + (1,))
                bk = logged.fetch_bounces()[2]                     # (K, M) over the surviving rays
                logged.close()
                total = ref["n_bott"] + ref["n_surf"]
                assert (total > 0).sum() > 20, want                # (so that nothing below holds vacuously)
                for k in ref:
                    assert _same(ref[k], got[k]), (want, k)        # status, counts, n_steps, n_rej, end states, samples
                ok = ref["status"] == 0
                assert total[ok].max() <= K and np.array_equal((bk >= 0).sum(axis=0), total[ok]), want
            env.close()
    assert len(seen) == 24 and seen == {(lds, zm, 1 if lds else 3, pv, 1) for lds in (1, 0) for zm in range(6) for pv in (0, 1)}


def test_capacity_and_refusals(lib, small_cases, pr):  # noqa: F811
    c = small_cases["lds"]
    env, y0 = c["env"], c["y0"]
    h = lib.FanHandle(env, 0.0, X_SMALL, S_SMALL, y0=y0, max_bounces=1)
    out = h.fetch_rays()
    x1, p1, k1 = h.fetch_bounces()
    h.close()
    assert _same(out["n_bott"], c["ref"]["n_bott"]) and _same(out["n_surf"], c["ref"]["n_surf"])      # the counts run on
    assert x1.shape == (1, int((out["status"] == 0).sum()))
    assert _same(x1[0], c["log"][0][0]) and _same(p1[0], c["log"][1][0]) and np.array_equal(k1[0], c["log"][2][0])
    never = c["log"][2][0] < 0
    assert never.any() and np.isnan(x1[0][never]).all() and np.isnan(p1[0][never]).all() and (k1[0][never] == -1).all()
    # refused, nothing launched: the instance record is the last launch's
    before = (env.last_instance(), env.last_instance_log())
    with pytest.raises(lib.PgrError, match="PGR_EXACT_SAMPLES"):
        lib.FanHandle(env, 0.0, X_SMALL, S_SMALL, y0=y0, max_bounces=4, exact_samples=True)
    with pytest.raises(lib.PgrError, match="trajectories"):
        lib.FanHandle(env, 0.0, X_SMALL, 0, y0=y0, max_bounces=4)
    with pytest.raises(lib.PgrError, match="max_bounces"):
        lib.FanHandle(env, 0.0, X_SMALL, S_SMALL, y0=y0, max_bounces=0)
    hbm = small_cases["hbm"]["env"]
    hbm.set_option("api_blocked", 0)
    with pytest.raises(lib.PgrError, match="PGR_OPT_API_BLOCKED"):
        lib.FanHandle(hbm, 0.0, X_SMALL, S_SMALL, y0=y0, max_bounces=4)
    hbm.set_option("api_blocked", 1)
    assert (env.last_instance(), env.last_instance_log()) == before
    plain = lib.FanHandle(env, 0.0, X_SMALL, S_SMALL, y0=y0)
    with pytest.raises(lib.PgrError, match="without a bounce log"):
        plain.fetch_bounces()
    plain.close()
    # shoot_rays names the K the fan needs
    e = munk_env(pr)
    with pytest.raises(ValueError) as err:
        pr.shoot_rays(1000.0, 0.0, np.linspace(-20, 20, 96), 100e3, 51, e, flatearth=False, debug=False, max_bounces=1)
    need = int(str(err.value).split("max_bounces=")[-1].split(" ")[0])
    fan = pr.shoot_rays(1000.0, 0.0, np.linspace(-20, 20, 96), 100e3, 51, e, flatearth=False, debug=False, max_bounces=need)
    assert need > 1 and fan.bounces.count.max() == need and np.array_equal(fan.bounces.count, fan.n_botts + fan.n_surfs)
    # a fan of no rays asked for with a log has an empty log, not none
    none = pr.shoot_rays(1000.0, 0.0, np.array([]), 100e3, 51, e, flatearth=False, debug=False, max_bounces=3)
    assert len(none) == 0 and none.bounces.x.shape == none.bounces.kind.shape == (0, 3) and none.bounces.count.shape == (0,)


# ---- the post-pass alone, on synthetic logs ---------------------------------------------------------------------------------

SYN_BD = 4200.0 + 300.0 * np.sin(SYN_R / 9e3)
SYN_X0, SYN_X1 = 2e3, 55e3
BETA = (SYN_R.copy(), 3.0 * np.cos(SYN_R / 7e3))
# the 7-node tables: the bottom's nodes lie strictly inside (0, 90), so that a grazing angle can fall off either end of both
BOTTOM7 = (np.array([2.0, 5.0, 10.0, 20.0, 40.0, 60.0, 80.0]), np.array([0.25, 0.5, 1.0, 3.0, 6.0, 9.0, 12.5]))
SURFACE7 = (np.array([1.0, 2.0, 4.0, 8.0, 16.0, 32.0, 64.0]), np.array([0.25, 0.0, 0.5, 1.0, 0.75, 2.0, 3.0]))
ON_NODE = (0, 3, 6)              # the nodes an event is put on exactly: both ends (the clamps' equality) and one inside


@pytest.fixture(scope="module")
def syn_slope_env(lib):
    cin = syn_cin()
    cpin = np.gradient(cin, SYN_Z, axis=1, edge_order=1)
    env = lib.EnvHandle(cin, cpin, SYN_R, SYN_Z, SYN_BD, SYN_R.copy(), np.zeros(len(SYN_R)))
    yield env, cin
    env.close()


def _phi(cin, x, p_ode, kind):
    return bref.grazing(x, p_ode, kind, cin, SYN_R, SYN_Z, SYN_R, SYN_BD, BETA)


@pytest.fixture(scope="module")
def syn_tables(syn_slope_env):
    """The 7-node tables and the events planted on purpose, all at bx = SYN_X0 (the first save range: no event lies before
    it), as (kind, stored bp, what).  On a node: the event comes first -- p = sin(radians(node [+ beta])) / c_e -- and the
    node is then SET to the grazing angle that event has in the definition's arithmetic (a few ulps from the round figure),
    so that phi == node holds exactly.  Off the ends: phi below the first and above the last node of each table.
    |p c| = 1: fl(p c_e) == 1.0 exactly, both signs, on each boundary."""
    cin = syn_slope_env[1]
    tables, plants = [], []
    for kind, (nodes, values) in ((1, BOTTOM7), (0, SURFACE7)):
        nodes = nodes.copy()
        d = float(bref.bottom_at(SYN_X0, SYN_R, SYN_BD)) if kind else 0.0
        c = float(tlr.bilinear(np.array([SYN_X0]), np.array([d]), SYN_R, SYN_Z, cin)[0])
        beta = float(bref.table_at(SYN_X0, *BETA)) if kind else 0.0
        for j in ON_NODE:
            p = np.sin(np.radians(nodes[j] + beta)) / c
            nodes[j] = _phi(cin, SYN_X0, p, kind)[0]
            plants.append((kind, -p, f"on node {j}"))
        assert np.all(np.diff(nodes) > 0) and np.abs(nodes - (BOTTOM7, SURFACE7)[1 - kind][0]).max() < 1e-12
        for target, what in ((0.5 * nodes[0], "below"), (0.5 * (nodes[-1] + 90.0), "above")):
            plants.append((kind, -np.sin(np.radians(target + beta)) / c, what))
        for sign in (1.0, -1.0):
            plants.append((kind, -sign * _p_with_pc(c, False), "|p c| = 1"))
        tables.append((nodes, values))
    return tables[0], tables[1], plants


PLANT_FROM = 20                  # the planted events sit in slot 0 of the rays PLANT_FROM, PLANT_FROM + 1, ...


def synthetic_log(M, S, K, seed, cin, x, plants=()):
    """(bx, bp, bk) (M, K) stored sign: sorted events per ray at x_0, on save ranges, on interval midpoints (the argmin tie) and
    one ulp either side, several in one interval, at and past the last range; E = 0 and E = K rays; NaN bp; and, from 63 rays
    on, the events of syn_tables: phi on the nodes, off both ends of both tables, |bp c| = 1."""
    rng = np.random.default_rng(seed)
    bx, bp, bk = np.full((M, K), np.nan), np.full((M, K), np.nan), np.full((M, K), -1, np.int8)
    mid = 0.5 * (x[:-1] + x[1:]) if S > 1 else np.array([x[0]])
    special = np.concatenate([[x[0], x[-1], min(x[-1] + 500.0, SYN_R[-1])], x, mid, np.nextafter(mid, np.inf), np.nextafter(mid, -np.inf)])
    for m in range(M):
        E = (0, K)[m % 2] if m < 4 else int(rng.integers(0, K + 1))
        ev = np.where(rng.random(E) < 0.5, rng.choice(special, E), rng.uniform(x[0], x[0] + 1.02 * (x[-1] - x[0] + 1.0), E))
        if E > 2 and m % 3 == 0:
            ev[1:3] = ev[0] + np.array([1.0, 2.0])                  # several in one save interval
        bx[m, :E] = np.sort(np.clip(ev, x[0], SYN_R[-1]))
        bk[m, :E] = rng.integers(0, 2, E)
        bp[m, :E] = -np.sin(np.radians(rng.uniform(-50.0, 50.0, E))) / 1500.0
    if M > 5:
        for m in range(4, M, 7):
            if bk[m, 0] < 0:
                bx[m, 0], bk[m, 0] = x[0], 1
            bp[m, 0] = np.nan
    if M >= PLANT_FROM + len(plants):
        for m, (kind, p, _) in enumerate(plants, PLANT_FROM):       # the ray's first event (its others lie at or after x_0)
            bx[m, 0], bp[m, 0], bk[m, 0] = x[0], p, kind
    return bx, bp, bk


def check_planted(bx, bp, bk, cin, bottom, surface):
    """every case the planted events stand for occurs in the log, by the definition's own arithmetic"""
    ev = [(_phi(cin, bx[i], -bp[i], int(bk[i])), int(bk[i])) for i in zip(*np.nonzero(bk >= 0))]
    assert any(phi != phi and pc != pc for (phi, pc), _ in ev)                                         # NaN bp
    for kind, (nodes, _) in ((1, bottom), (0, surface)):
        phis = np.array([phi for (phi, _), k in ev if k == kind])
        pcs = np.array([pc for (_, pc), k in ev if k == kind])
        for j in ON_NODE:
            assert (phis == nodes[j]).any(), (kind, j)                                                 # on a node, the ends included
        assert (phis < nodes[0]).any() and (phis > nodes[-1]).any(), kind                              # outside, both sides
        assert ((phis > nodes[0]) & (phis < nodes[-1]) & ~np.isin(phis, nodes)).any(), kind            # between
        assert (pcs == 1.0).any() and (pcs == -1.0).any(), kind                                        # |p c| = 1, both signs


def _device_boundary(lib, env, bx, bp, bk, x0, x1, S, tables, want=(True, True)):
    import torch
    dev = torch.device("cuda", env.device)
    M, K = bk.shape
    up = lambda a, dt: torch.from_numpy(np.ascontiguousarray(a.T)).to(dt).to(dev)  # noqa: E731
    dx, dp, dk = up(bx, torch.float64), up(bp, torch.float64), up(bk, torch.int8)
    pad = 64
    out = torch.full((S * M + pad,), -7.0, dtype=torch.float64, device=dev)
    cnt = [torch.full((S * M + pad,), -7, dtype=torch.int32, device=dev) for _ in range(2)]
    lib.boundary_loss_device(env, dx.data_ptr(), dp.data_ptr(), dk.data_ptr(), M, K, x0, x1, S, lib.boundary_tables(*tables),
                             out.data_ptr(), cnt[0].data_ptr() if want[0] else 0, cnt[1].data_ptr() if want[1] else 0,
                             torch.cuda.current_stream(dev).cuda_stream)
    torch.cuda.synchronize()
    out, nb, ns = out.cpu().numpy(), cnt[0].cpu().numpy(), cnt[1].cpu().numpy()
    assert (out[S * M:] == -7.0).all() and (nb[S * M:] == -7).all() and (ns[S * M:] == -7).all()       # the padding is intact
    for a, w in ((nb, want[0]), (ns, want[1])):
        assert w or (a == -7).all()                                                                    # NULL: not written
    return out[:S * M].reshape(S, M).T, nb[:S * M].reshape(S, M).T, ns[:S * M].reshape(S, M).T


@pytest.mark.parametrize("K", [1, 3, 40])
@pytest.mark.parametrize("S", [1, 2, 5, 200])
@pytest.mark.parametrize("M", [1, 63, 64, 65, 4035])
def test_post_pass_bit_identical_to_the_restatement_on_synthetic_logs(lib, syn_slope_env, syn_tables, M, S, K):
    env, cin = syn_slope_env
    bottom7, surface7, plants = syn_tables
    x0, x1 = SYN_X0, SYN_X1
    x = np.linspace(x0, x1, S)
    bx, bp, bk = synthetic_log(M, S, K, 1000 * M + 10 * S + K, cin, x, plants)
    planted = np.arange(PLANT_FROM, PLANT_FROM + len(plants)) if M >= 63 else np.arange(0)
    if M >= 63:
        check_planted(bx[:PLANT_FROM + len(plants)], bp[:PLANT_FROM + len(plants)], bk[:PLANT_FROM + len(plants)], cin, bottom7, surface7)
    tables = (bottom7, surface7, BETA) if (M + S + K) % 2 else ((None, [2.5]), (None, [0.75]), (None, [0.0]))
    want = [(True, True), (False, True), (True, False)][(M + K) % 3]
    B, nb, ns = _device_boundary(lib, env, bx, bp, bk, x0, x1, S, tables, want)
    if M > 300:                      # (the restatement is a Python loop per event: a stride of the big fan, its last wave, the planted)
        sub = np.unique(np.concatenate([np.arange(0, M, 17), np.arange(M - 70, M), planted]))
    else:
        sub = np.arange(M)
    rB, rnb, rns = bref.boundary_loss(bx[sub], bp[sub], bk[sub], x, cin, SYN_R, SYN_Z, SYN_R, SYN_BD, *tables)
    assert _same(B[sub], rB), (M, S, K)
    assert (not want[0] or np.array_equal(nb[sub], rnb)) and (not want[1] or np.array_equal(ns[sub], rns))
    if M == 65 and K == 3:
        assert np.isnan(rB).any() and (rB[~np.isnan(rB)] > 0).any()
        again = _device_boundary(lib, env, bx, bp, bk, x0, x1, S, tables, want)[0]
        assert _same(B, again)


def test_c_entry_refuses_bad_tables_before_writing(lib, syn_slope_env):
    import torch
    env, cin = syn_slope_env
    x = np.linspace(2e3, 55e3, 5)
    bx, bp, bk = synthetic_log(8, 5, 3, 1, cin, x)
    good = ((None, [1.0]), (None, [1.0]), (None, [0.0]))
    bad = [(([0.0, 0.0], [1.0, 1.0]), good[1], good[2]), ((None, [-1.0]), good[1], good[2]), (good[0], (None, [np.nan]), good[2]),
           (good[0], good[1], ([0.0, 1.0], [0.0, np.inf])), (good[0], ([3.0, 2.0], [0.0, 1.0]), good[2])]
    for tables in bad:
        with pytest.raises(lib.PgrError):
            _device_boundary(lib, env, bx, bp, bk, 2e3, 55e3, 5, tables)
    dev = torch.device("cuda", env.device)
    t = torch.zeros(64, dtype=torch.float64, device=dev)
    with pytest.raises(lib.PgrError, match="out_db"):
        lib.boundary_loss_device(env, t.data_ptr(), t.data_ptr(), t.data_ptr(), 8, 3, 2e3, 55e3, 5, lib.boundary_tables(*good), 0)


# ---- fans ---------------------------------------------------------------------------------------------------------------------

def test_sample_assignment_is_the_oracle_segments(lib, small_cases, pr):  # noqa: F811
    """RayFan.bounce_counts at every column of every surviving ray of the three small fans = the oracle trace's segments whose
    start argmin-index is <= s, independently of the restatement; at the last column n_bott / n_surf"""
    x = np.linspace(0.0, X_SMALL, S_SMALL)
    for which in ("lds", "hbm", "slope"):
        c = small_cases[which]
        ok = c["ref"]["status"] == 0
        M = int(ok.sum())
        z = np.zeros((M, S_SMALL))
        fan = pr.RayFan.from_arrays(np.zeros(M), np.tile(x, (M, 1)), z, z, z, c["ref"]["n_bott"][ok], c["ref"]["n_surf"][ok], np.full(M, 900.0))
        fan._bounces = pr.BounceLog(*(a.T for a in c["log"]))
        nb, ns = fan.bounce_counts(np.arange(S_SMALL))
        assert nb.shape == ns.shape == (M, S_SMALL) and nb.dtype == ns.dtype == np.int64
        tx, _, tk, cnt = (a[ok] for a in c["oracle"])              # the oracle's own trace of every ray (K = 24 holds them all)
        for m in range(M):
            j = np.array([int(np.argmin(np.abs(x - v))) for v in tx[m, :cnt[m]]], dtype=np.int64)
            for s in range(S_SMALL - 1):
                assert nb[m, s] == np.sum((j <= s) & (tk[m, :cnt[m]] == 1)) and ns[m, s] == np.sum((j <= s) & (tk[m, :cnt[m]] == 0))
        assert np.array_equal(nb[:, -1], c["ref"]["n_bott"][ok]) and np.array_equal(ns[:, -1], c["ref"]["n_surf"][ok])
        assert (nb[:, :-1] < nb[:, -1:]).any() and (nb[:, 1:] > nb[:, :1]).any()       # the counts do change along the columns


def _traced_beta(env, xf, flatearth, backwards):
    """the bottom slope of the traced frame from frame_independent.py, which shares no code with the package -- and, asserted
    here, the very arrays the package's own frame helper hands the post-pass"""
    from pygenray_amd.environment import _unpack_envi
    br, ang = fi.bottom_slope(env, -xf if backwards else xf)
    arrs = _unpack_envi(env, flatearth=flatearth)
    own_br, own_ang = np.asarray(arrs[5], dtype=float), np.asarray(arrs[6], dtype=float)
    if backwards:
        own_br, own_ang = -own_br[::-1], -own_ang[::-1]
    assert _same(br, own_br) and _same(ang, own_ang)
    return br, ang


def wall_env(pr):  # noqa: F811
    """sloping_env's range-dependent Munk (tables in HBM) over a sea floor that steps up 1000 m in 1 km at 39 km: the rays
    that meet the 45 degree wall bounce backwards and are dropped, the others bounce off the flat parts and survive"""
    z = np.linspace(0, 5500, 1377)
    r = np.linspace(0, 200e3, 33)
    br = np.array([0.0, 20e3, 39e3, 40e3, 60e3, 100e3, 200e3])
    bd = np.array([4800.0, 4800.0, 4800.0, 3800.0, 3800.0, 3800.0, 3800.0])
    return _env(pr, z, r, np.array([pr.munk_ssp(z, 1300 + 5e-4 * ri) for ri in r]), br, bd)


FAN_BOTTOM = ([0.0, 10.0, 30.0, 90.0], [0.5, 1.0, 4.0, 9.0])
FAN_SURFACE = 0.25
ARR = (("tube", "tube"), ("w", "w"), ("T", "time"), ("p", "p"), ("I", "intensity"))


@pytest.mark.parametrize("which, resident, flatearth, backwards",
                         [("munk", True, False, False), ("sloping", True, False, False), ("sloping", False, False, True),
                          ("wall", True, False, False), ("default", True, True, False)])
def test_products_with_boundary_loss_bit_identical_to_the_restatements(pr, which, resident, flatearth, backwards):  # noqa: F811
    """rows (munk) and sample-blocked (sloping) fans, dropped rays (a wall on the sea floor), backwards, flat-earth: boundary_loss,
    bounce_counts, TL, beams and arrivals against the restatements fed g W, W from B and from A + B"""
    env = {"munk": munk_env, "sloping": sloping_env, "wall": wall_env, "default": lambda p: p.OceanEnvironment2D()}[which](pr)
    src, x1 = ((900.0, 150e3), 60e3) if backwards else ((1000.0, 0.0), 80e3)
    kw = dict(flatearth=flatearth, debug=False, max_bounces=40)
    ang = np.linspace(-20, 20, 300)
    fan = pr.shoot_rays(src[0], src[1], ang, x1, 81, env, device_resident=resident, **kw)
    eager = pr.shoot_rays(src[0], src[1], ang, x1, 81, env, device_resident=False, **kw)
    plain = pr.shoot_rays(src[0], src[1], ang, x1, 81, env, device_resident=False, flatearth=flatearth, debug=False)
    assert _same(plain.zs, eager.zs) and _same(plain.ts, eager.ts) and _same(plain.ps, eager.ps) and len(eager) > 50
    assert (which != "wall") or len(eager) < 300
    log = eager.bounces
    assert (log.count > 0).sum() > 20 and np.array_equal(log.count, eager.n_botts + eager.n_surfs)
    xf, cin, rin, zin, bd, br = fi.traced_frame(env, np.asarray(eager.rs[0], dtype=float), flatearth)
    beta = _traced_beta(env, xf, flatearth, backwards)
    bottom, surface = (np.array(FAN_BOTTOM[0]), np.array(FAN_BOTTOM[1])), (None, np.array([FAN_SURFACE]))
    B_ref, nb_ref, ns_ref = bref.boundary_loss(log.x, log.p, log.kind, xf, cin, rin, zin, br, bd, bottom, surface, beta)
    assert (B_ref[:, -1] > 0).sum() > 20 and not np.isnan(B_ref).any()
    for f in (fan, eager):
        assert _same(pr.boundary_loss(f, env, FAN_BOTTOM, FAN_SURFACE, flatearth=flatearth), B_ref)
        nb, ns = f.bounce_counts(np.arange(81))
        assert np.array_equal(nb, nb_ref) and np.array_equal(ns, ns_ref)
    assert _same(pr.boundary_loss(fan, env, FAN_BOTTOM, FAN_SURFACE, range_indices=[-1, 3], flatearth=flatearth), B_ref[:, [80, 3]])
    # the counts the post-pass forms on the device, through the keep list of the fan handle (rays were dropped) and from
    # the uploaded log of the host fan: RayFan.bounce_counts, which NumPy forms from the fetched log
    from pygenray_amd._fan_frame import _TracedFan, _boundary_spec, _save_grid
    for f in (fan, eager):
        dB, dnb, dns = _TracedFan(f, _save_grid(f), env, flatearth).to_device(0).boundary_loss(
            _boundary_spec(f, FAN_BOTTOM, FAN_SURFACE), counts=True)
        assert _same(dB.cpu().numpy().T, B_ref) and np.array_equal(dnb.cpu().numpy().T, nb_ref) and np.array_equal(dns.cpu().numpy().T, ns_ref)
    front = fan.time_front(40)
    assert np.array_equal(np.char.endswith(front.ray_ids, "b"), (nb_ref[:, 40] + ns_ref[:, 40]) > 0)
    d, cols = DEPTHS[::20], [40, 80, 1]
    p0 = fi.launch_slowness(eager.thetas, eager.source_depths[0], xf, cin, rin, zin)
    A_ref = pref.fan_path_integral(eager, env, 0.07, flatearth)
    loss = dict(bottom_loss=FAN_BOTTOM, surface_loss=FAN_SURFACE)
    for W, extra in ((pref.weights(B_ref), {}), (pref.weights(A_ref + B_ref), dict(absorption=0.07))):
        I = pr.transmission_loss(fan, d, env, flatearth=flatearth, intensity=True, **loss, **extra)
        assert _same(I, pref.tube_intensity(eager.zs, eager.ps, xf, p0, d, cin, rin, zin, W)) and (I[:, 1:] > 0).mean() > 0.2
        Bm = pr.beam_transmission_loss(fan, d, env, flatearth=flatearth, intensity=True, min_width=20.0, **loss, **extra)
        assert _same(Bm, pref.beam_intensity(eager.zs, eager.ps, xf, p0, d, cin, rin, zin, fi.bottom_at(xf, bd, br), 20.0, W))
        a = pr.arrivals(fan, d, env, flatearth=flatearth, range_indices=cols, **loss, **extra)
        ref = pref.tube_arrivals(eager.zs, eager.ps, eager.ts, xf, p0, d, cols, cin, rin, zin, W)
        assert len(a) > 20 and np.array_equal(a.offsets, ref["offsets"])
        for k, name in ARR:
            assert _same(ref[k], getattr(a, name)), k
    # both losses at 0.0 dB: the unweighted calls, bit for bit
    zero = dict(bottom_loss=0.0, surface_loss=([0.0, 90.0], [0.0, 0.0]))
    assert _same(pr.transmission_loss(fan, d, env, flatearth=flatearth), pr.transmission_loss(fan, d, env, flatearth=flatearth, **zero))
    assert _same(pr.beam_transmission_loss(fan, d, env, flatearth=flatearth), pr.beam_transmission_loss(fan, d, env, flatearth=flatearth, **zero))
    a, b = pr.arrivals(fan, d, env, flatearth=flatearth, range_indices=cols), pr.arrivals(fan, d, env, flatearth=flatearth, range_indices=cols, **zero)
    for k in ("offsets", "tube", "w", "time", "p", "intensity", "amplitude", "received_angle", "turning_points"):
        assert _same(np.asarray(getattr(a, k)), np.asarray(getattr(b, k))), k
    if resident:
        assert fan.device_resident and not any(k in fan.__dict__ for k in ("_ts", "_zs", "_ps"))


def image_intensity_bottom_loss(ranges, depths, source_depth, water_depth, max_angle_deg, b_db):
    """tl_reference.image_intensity with b dB per bottom bounce: sum over the images of 10^(-b n_b / 10) / R^2, n_b counted on
    the unfolded path: the straight line from an image to the receiver crosses the bottom once for every odd multiple of
    the water depth H between their depths."""
    r = np.asarray(ranges, dtype=float)[None, :, None]
    d = np.asarray(depths, dtype=float)[:, None, None]
    H = water_depth
    tmax = np.tan(np.radians(max_angle_deg))
    nmax = int(np.ceil(tmax * np.max(ranges) / (2 * H))) + 2
    n = np.arange(-nmax, nmax + 1)
    zi = np.concatenate([2 * n * H + source_depth, 2 * n * H - source_depth])[None, None, :]
    # unfold: a straight path from the image at zi to the receiver at d (0 < d < H) crosses the levels (2 k + 1) H (bottom)
    lo, hi = np.minimum(zi, d), np.maximum(zi, d)
    n_b = np.floor((hi - H) / (2 * H)) - np.ceil((lo - H) / (2 * H)) + 1
    n_b = np.where(hi > lo, np.maximum(n_b, 0), 0)
    dz = np.abs(zi - d)
    R2 = r * r + dz * dz
    return np.where(dz <= tmax * r, 10.0 ** (-b_db * n_b / 10.0) / R2, 0.0).sum(axis=2)


def test_isovelocity_fan_with_constant_bottom_loss_matches_the_image_sum(pr_any):  # noqa: F811
    """the fan, receivers, ranges and 0.1 dB of the isovelocity test of test_transmission_loss.py, with 3 dB per bottom bounce"""
    z = np.arange(0, 6000, 10.0)
    r = np.linspace(0, 25e3, 6)
    env = _env(pr_any, z, r, np.full((len(r), len(z)), 1500.0), r, np.full(len(r), 5000.0))
    fan = pr_any.shoot_rays(1000.0, 0.0, np.linspace(-80, 80, 20001), 20e3, 2001, env, flatearth=False, debug=False, max_bounces=32)
    assert len(fan) == 20001 and fan.device_resident
    depths = np.arange(tlr.MARGIN, 5000 - tlr.MARGIN + 1, 50.0)
    tl = pr_any.transmission_loss(fan, depths, env, flatearth=False, bottom_loss=3.0)
    x = np.asarray(fan.rs[0])
    keep = (x >= 1e3) & (x <= 20e3)
    assert _same(tlr.image_intensity(x[keep], depths, 1000.0, 5000.0, 80.0),
                 image_intensity_bottom_loss(x[keep], depths, 1000.0, 5000.0, 80.0, 0.0))
    ref = tlr.to_db(image_intensity_bottom_loss(x[keep], depths, 1000.0, 5000.0, 80.0, 3.0))
    err = np.abs(tl[:, keep] - ref)
    j, k = np.unravel_index(np.argmax(err), err.shape)
    print(f"bottom-loss image sum: worst {err.max():.4f} dB at depth {depths[j]} m, range {x[keep][k]} m")
    assert err.max() < tlr.TOL_DB, (err.max(), depths[j], x[keep][k])
    plain = tlr.to_db(tlr.image_intensity(x[keep], depths, 1000.0, 5000.0, 80.0))
    assert np.abs(ref - plain).max() > 1.0 and fan.device_resident
