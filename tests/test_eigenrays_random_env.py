"""The eigenray search -- the device loop of csrc/pgr_eigen_hist.h (pgr_eigen_step, pgr_eigen_set_p0, the spread trial fan with
PGR_SKIP_NAN_Y0, the slowness callback) and the re-shoot with trajectories of eigenrays._regula_falsi_batch -- on the random
environments of helpers.random_case: the cases, API seeds and latitudes are test_products_random_env.py's own objects.  Until
this module the search had met one family of inputs, a range-independent Munk profile over a flat floor searched forwards with
flatearth=False, terminate_backwards=True and rtol 1e-9.  In the reference arithmetic only; every expectation is the loop of
tests/eigen_reference.py (REF/eigenrays.py:65-79, :118-120, :206-268 in plain NumPy) around the CPU oracle
(oracle.shoot_fan, oracle.MATH_CR) with the initial state [0, source_depth, np.sin(np.radians(-theta)) / c_source],
c_source = oracle.bilinear(...): no expected value comes from the GPU.

Level 1 (one test per case of CASES, 12 of the 40 flat-earth mapped): the fan of case_inputs shot end-state only through
EnvHandle.shoot_fan, its status, bounce counts and end states equal to the oracle's fan; the surviving rays in launch order
(user angle = minus the ODE angle, stored depth = minus the end z), receiver depths np.quantile(-z_end, [0.2, 0.5, 0.8]) of
the ORACLE's fan, the brackets of the three depths concatenated into one EnvHandle.eigen_refine (ztol 1, max_iter 20, the
case's rtol and terminate_backwards).  With the NumPy-sine callback (what find_eigenrays passes): state, n_trial, launches,
theta in all three states, z_end and t_end bit for bit (NaN for a dropped trial ray) against the oracle loop.  With
slowness=None (pgr_eigen_refine_depths): the same, bit for bit, against the same loop fed the correctly rounded sine of
(-theta) * (pi / 180) from the host build of csrc/pgr_crmath.h (tests/crmath_host.c, the fixture of tests/test_crmath.py).
No bracket has z1 == z2 (asserted: it would be a NaN trial angle).  On three cases the brackets are tiled past the sharing
thresholds of the trial fan -- an LDS-table and an HBM-table case to more than 1024 brackets, a mirrored case to more than
32768, where per_wave = 64 and spread = 1 -- and every copy equals the oracle loop's result, with the same launches.

Level 2 (API_CASES x forwards / backwards x flatearth off / on): an OceanEnvironment2D from the raw tables, pr.shoot_rays
device resident and not, pr.find_eigenrays on both fans.  The expectation is the oracle on the frame tests/frame_independent.py
derives (traced_frame, bottom_slope, np.gradient for cpin), receiver depths chosen as at level 1 from the oracle's fan: per
depth the counts and the failed brackets, launch angles, end depths and times, bounce counts of the found brackets bit for bit;
rs == np.linspace(xs, xr, S); the trajectories against the oracle's of the found angles by the rule helpers.assert_bit_parity
applies to the default sample form (bit-equal outside a step, 1e-12 x scale inside; the filler n_steps is the oracle's own);
pr.shoot_ray of three found angles bit-equal to the eigenray returned; LAST_SEARCH_STATS["reshot_differs"] == 0 and launches
= the loop's + 1; the device fan's result equal to the host fan's, array for array.

The re-shoot with spread = 1 (eigenrays.py: more than 1024 eigenrays, or found * 64 * S * 24 > 256 MiB), on the sloping,
range-dependent seed SPREAD_SEED: N_DEPTHS receiver depths at quantiles 0.05 ... 0.95 (more than 1024 found, asserted from the
oracle loop), and the three depths at an S computed from the found count (the inequality asserted).  Each equals the oracle
loop's angles and end states, and depth by depth the same search made one depth at a time at S = 2.

The seed rule (conditions, asserted, so that the sweep cannot go vacuous; cpu_check() re-runs it with the oracle alone, from
the repository root: PYTHONPATH=. python tests/test_eigenrays_random_env.py): every case or frame has >= 5 brackets and >= 5
found; per level >= 20 brackets end dropped (state 2) and >= 100 at the iteration limit (state 3); at level 1 >= 24 cases reach
22 trial rays, >= 6 cases each are mirrored, HBM-table, flat-earth mapped and terminate_backwards=False, and the two sines
give >= 5 brackets different angles (so that the second comparison is not the first run twice).  Passed over:
none at either level.  A case on which the device disagrees is a finding and stays in the list.  DESIGN.md section 4 has the
composition and the tallies of the MI355X run."""
import functools

import numpy as np
import pytest

import eigen_reference as eref
import frame_independent as fi
import oracle
from helpers import assert_bit_parity, random_case, y0_for
from test_coherent_random_env import _Tables, api_case
from test_crmath import crh  # noqa: F401  (fixture: the host build of csrc/pgr_crmath.h)
from test_products_random_env import API_CASES, CASES, case_inputs, n_rays_of
from tube_gpu import pr  # noqa: F401  (fixture)

pytestmark = pytest.mark.gpu

PASSED_OVER, PASSED_OVER_API = (), ()                     # (seed, flat) of CASES / seeds of API_CASES the rule drops
LEVEL1 = [c for c in CASES if c not in PASSED_OVER]
LEVEL2 = [c for c in API_CASES if c[0] not in PASSED_OVER_API]
assert len(PASSED_OVER) <= 2 and len(PASSED_OVER_API) == 0
QUANTILES = (0.2, 0.5, 0.8)
ZTOL, MAX_ITER = 1.0, 20
MOST_TRIALS = MAX_ITER + 2                                # trial rays of a bracket that ends at the iteration limit
CR_SINE = 3                                               # crh_eval's function number of the sine (tests/crmath_host.c)
# (seed, flat, what the case must be, brackets to tile past): chosen from the case descriptions for few brackets on a short
# range that still end in more than one state (219: 17 found, 1 dropped, 1 at the limit; 408, flat-earth mapped: 13 found, 2
# at the limit; 212: 33 found, 2 at the limit); per_wave of the trial fan doubles while ceil(nbk / per_wave) > 1024
# (csrc/pgr_eigen_hist.h)
TILED = ((219, False, "lds", 1024), (408, True, "hbm", 1024), (212, False, "mirrored", 32768))
# the re-shoot with spread = 1: a range-dependent API seed over a sloping floor (66 km, 1104 of 1272 brackets found at 56 depths)
SPREAD_SEED, N_DEPTHS = 214, 56
MIB256 = 256 * 1024 * 1024


def numpy_slowness(c0):
    """REF/launch_rays.py:284-285 of ODE angles in degrees, NumPy's own sine: what find_eigenrays hands the device loop"""
    return lambda ang: np.sin(np.radians(ang)) / c0


def oracle_shoot(arrs, src, x0, x1, c0, shot, sine=None):
    """eigen_reference's `shoot` on the CPU oracle: shoot_ray(theta) has ODE angle -theta (REF/launch_rays.py:251).  `sine`:
    the sine of (-theta) * (pi / 180) in the initial slowness instead of np.sin(np.radians(-theta))."""
    def shoot(theta_user):
        ang = -np.asarray(theta_user, dtype=float)
        p0 = (np.sin(np.radians(ang)) if sine is None else sine(ang * (np.pi / 180.0))) / c0
        y0 = np.stack([np.zeros_like(p0), np.full_like(p0, src), p0], 1)
        o = oracle.shoot_fan(*arrs, y0, x0, x1, 2, math=oracle.MATH_CR, **shot)
        return o["status"], -o["z"][:, -1], o["T"][:, -1]
    return shoot


def oracle_search(arrs, src, x0, x1, S, theta_user, shot, quantiles=QUANTILES):
    """The oracle's fan of user angles theta_user from (x0, src) on the tables arrs, the receiver depths at `quantiles` of its
    end depths, the brackets of every depth concatenated and the oracle loop on them -> dict.  `per_depth`: a slice of the
    brackets per receiver depth."""
    theta_user = np.asarray(theta_user, dtype=float)
    c0 = oracle.bilinear(x0, src, arrs[2], arrs[3], arrs[0])
    y0 = y0_for(oracle, arrs, src, x0, -theta_user)
    fan = oracle.shoot_fan(*arrs, y0, x0, x1, S, math=oracle.MATH_CR, **shot)
    kept = np.flatnonzero(fan["status"] == 0)
    theta, z_end = theta_user[kept], -fan["z"][kept, -1]
    rds = [float(q) for q in np.quantile(-z_end, quantiles)]
    br = [eref.brackets(theta, z_end, rd) for rd in rds]
    th1, th2, z1, z2 = (np.concatenate([b[k] for b in br]) for k in range(4))
    rd_k = np.concatenate([np.full(len(b[0]), rd) for b, rd in zip(br, rds)])
    edges = np.concatenate([[0], np.cumsum([len(b[0]) for b in br])])
    assert np.all(z1 != z2), "a bracket with z1 == z2: its trial angle would be a NaN"
    ref = eref.refine(oracle_shoot(arrs, src, x0, x1, c0, shot), th1, th2, z1, z2, rd_k, ztol=ZTOL, max_iter=MAX_ITER)
    return dict(c0=c0, y0=y0, fan=fan, kept=kept, theta=theta, z_end=z_end, rds=rds, th1=th1, th2=th2, z1=z1, z2=z2, rd_k=rd_k,
                per_depth=[slice(a, b) for a, b in zip(edges[:-1], edges[1:])], ref=ref)


def figures(ref):
    st = ref["state"]
    return dict(brackets=len(st), found=int((st == 1).sum()), dropped=int((st == 2).sum()), limit=int((st == 3).sum()),
                all_trials=bool(len(st) and ref["n_trial"].max() == MOST_TRIALS), launches=ref["launches"])


def misses(fig):
    """the conditions of the seed rule that one case or frame must meet"""
    return [f"{k} {fig[k]} < 5" for k in ("brackets", "found") if fig[k] < 5]


def level_misses(figs, level1):
    out = [f"{k} {sum(f[k] for f in figs)} < {least}" for k, least in (("dropped", 20), ("limit", 100))
           if sum(f[k] for f in figs) < least]
    if level1:
        out += [f"{k} {sum(f[k] for f in figs)} < {least}" for k, least in (("all_trials", 24), ("mirrored", 6), ("hbm", 6),
                                                                            ("flat", 6), ("tb_false", 6))
                if sum(f[k] for f in figs) < least]
    return out


@functools.lru_cache(maxsize=None)
def level1_expectation(seed, flat):
    """everything of a level-1 case that needs no GPU"""
    arrs, y0, kw, desc, mirrored = case_inputs(seed, flat)
    _, (src, x0, th), _, _ = random_case(seed, n_rays=n_rays_of(seed))
    assert x0 == kw["x0"]
    shot = dict(rtol=kw["rtol"], terminate_backwards=kw["terminate_backwards"])
    e = oracle_search(arrs, src, x0, kw["x1"], kw["S"], -th, shot)
    assert np.array_equal(e["y0"], y0)                     # (the ODE angle is th itself: the fan IS case_inputs')
    e.update(arrs=arrs, src=src, kw=kw, shot=shot, desc=desc, mirrored=mirrored)
    return e


def frame_tables(arrs, lat, xs, xr, S, fe):
    """the raw tables of the frame a fan from xs to xr is traced in, by frame_independent alone -> (arrs of the frame, x0, x1)"""
    tables = _Tables(arrs, lat)
    x = np.linspace(xs, xr, S)
    xf, cin, rin, zin, bd, br = fi.traced_frame(tables, x, fe)
    beta = fi.bottom_slope(tables, x)
    return [cin, np.gradient(cin, zin, axis=1, edge_order=1), rin, zin, bd, br, beta[1]], xf[0], xf[-1]


def found_trajectories(frame_arrs, src, x0, x1, S, c0, theta, shot):
    """the oracle's rays of user angles theta with S samples, as shoot_ray(theta) starts them"""
    p0 = np.sin(np.radians(-np.asarray(theta, dtype=float))) / c0
    y0 = np.stack([np.zeros_like(p0), np.full_like(p0, src), p0], 1)
    return oracle.shoot_fan(*frame_arrs, y0, x0, x1, S, math=oracle.MATH_CR, **shot)


@functools.lru_cache(maxsize=None)
def level2_expectation(seed, lat, backwards, fe, quantiles=QUANTILES, S=None):
    arrs, src, th, kw, desc = api_case(seed)
    S = kw["S"] if S is None else S
    xs, xr = (kw["x1"], kw["x0"]) if backwards else (kw["x0"], kw["x1"])
    shot = dict(rtol=kw["rtol"], terminate_backwards=kw["terminate_backwards"])
    frame_arrs, x0, x1 = frame_tables(arrs, lat, xs, xr, S, fe)
    e = oracle_search(frame_arrs, src, x0, x1, S, th, shot, quantiles)          # (128 angles and more: the ODE angle is -theta)
    e.update(arrs=arrs, frame_arrs=frame_arrs, x0=x0, x1=x1, xs=xs, xr=xr, S=S, src=src, th=th, kw=kw, shot=shot, desc=desc)
    return e


def cpu_check(level1=True, level2=True):
    """The seed rule on every case of both levels, the oracle alone: prints each case's tallies and the missed conditions."""
    import time
    out = []
    if level1:
        figs = []
        for seed, flat in CASES:
            t = time.time()
            e = level1_expectation(seed, flat)
            fig = dict(figures(e["ref"]), mirrored=e["mirrored"], hbm="range-dep True" in e["desc"], flat=flat,
                       tb_false=not e["kw"]["terminate_backwards"])
            figs.append(fig)
            out.append(((seed, flat), misses(fig)))
            print(f"seed {seed} flat {flat!s:5s} {time.time() - t:5.1f} s  misses {out[-1][1]}  {fig}  {e['desc']} "
                  f"tb {e['kw']['terminate_backwards']}", flush=True)
        print("level 1:", {k: sum(f[k] for f in figs) for k in figs[0]}, "brackets per case",
              min(f["brackets"] for f in figs), "...", max(f["brackets"] for f in figs))
        out.append(("level 1", level_misses(figs, True)))
    if level2:
        figs = []
        for seed, lat in API_CASES:
            for backwards in (False, True):
                for fe in (False, True):
                    t = time.time()
                    e = level2_expectation(seed, lat, backwards, fe)
                    figs.append(figures(e["ref"]))
                    out.append(((seed, backwards, fe), misses(figs[-1])))
                    print(f"API seed {seed} backwards {backwards!s:5s} flatearth {fe!s:5s} {time.time() - t:5.1f} s  "
                          f"misses {out[-1][1]}  {figs[-1]}  {e['desc']}", flush=True)
        print("level 2:", {k: sum(f[k] for f in figs) for k in figs[0]}, "brackets per frame",
              min(f["brackets"] for f in figs), "...", max(f["brackets"] for f in figs))
        out.append(("level 2", level_misses(figs, False)))
    print("missed:", [(c, m) for c, m in out if m])
    return out


# ---- level 1: the device loop on raw tables -----------------------------------------------------------------------------------

def _bits(a, b):
    """bit for bit, NaN patterns included"""
    a, b = np.asarray(a), np.asarray(b)
    return a.shape == b.shape and bool(np.all((a == b) | ((a != a) & (b != b))))


def same_search(got, ref, label, reps=1):
    """a result of EnvHandle.eigen_refine against the oracle loop's (tiled `reps` times), bit for bit"""
    assert got["launches"] == ref["launches"], (label, "launches", got["launches"], ref["launches"])
    for k in ("state", "n_trial"):
        assert np.array_equal(got[k], np.tile(ref[k], reps)), (label, k, np.flatnonzero(got[k] != np.tile(ref[k], reps))[:8])
    for k in ("theta", "z_end", "t_end"):
        want = np.tile(ref[k], reps)
        bad = ~((got[k] == want) | ((got[k] != got[k]) & (want != want)))
        assert not bad.any(), (label, k, int(bad.sum()), np.flatnonzero(bad)[:5], got[k][bad][:5], want[bad][:5],
                               np.tile(ref["state"], reps)[bad][:5])


def per_wave_of(nbk):
    """the sharing rule of the trial fan (csrc/pgr_eigen_hist.h)"""
    per_wave = 1
    while per_wave < 64 and (nbk + per_wave - 1) // per_wave > 1024:
        per_wave *= 2
    return per_wave


_RECORDS, _API_RECORDS = {}, {}


def _level1(pr, crh, seed, flat):  # noqa: F811
    if (seed, flat) in _RECORDS:
        return _RECORDS[(seed, flat)]
    from pygenray_amd import _lib
    e = level1_expectation(seed, flat)
    arrs, kw, shot, src, c0, ref = e["arrs"], e["kw"], e["shot"], e["src"], e["c0"], e["ref"]
    label = f"seed {seed}{' (flat earth)' if flat else ''}: {e['desc']}"
    fig = figures(ref)
    assert not misses(fig), (label, misses(fig))
    env = _lib.EnvHandle(*arrs)
    # the fan itself, end state only, against the oracle's
    g = env.shoot_fan(e["y0"], kw["x0"], kw["x1"], kw["S"], save=False, **shot)
    o = e["fan"]
    assert np.array_equal(g["status"], o["status"]), (label, "the fan's status")
    ok = o["status"] == 0
    assert np.array_equal(g["n_bott"][ok], o["n_bott"][ok]) and np.array_equal(g["n_surf"][ok], o["n_surf"][ok]), label
    end = np.stack([o["T"][:, -1], o["z"][:, -1], o["p"][:, -1]], 1)
    assert _bits(g["end"][ok], end[ok]) and np.isnan(g["end"][~ok]).all(), (label, "the fan's end states")
    # the loop, with the callback find_eigenrays passes ...
    search = (e["th1"], e["th2"], e["z1"], e["z2"], e["rd_k"], src, kw["x0"], kw["x1"], c0)
    how = dict(ztol=ZTOL, max_iter=MAX_ITER, **shot)
    got = env.eigen_refine(*search, slowness=numpy_slowness(c0), **how)
    instance = env.last_instance()
    same_search(got, ref, label + " (NumPy's sine through the callback)")
    # ... and with the device's own correctly rounded sine
    sine = lambda x: crh(CR_SINE, x)  # noqa: E731
    ref_cr = eref.refine(oracle_shoot(arrs, src, kw["x0"], kw["x1"], c0, shot, sine=sine), *search[:5], ztol=ZTOL,
                         max_iter=MAX_ITER)
    same_search(env.eigen_refine(*search, slowness=None, **how), ref_cr, label + " (the device's sine)")
    rec = dict(fig, mirrored=e["mirrored"], hbm=not env.lds_path, flat=flat, tb_false=not kw["terminate_backwards"],
               instance=tuple(instance[k] for k in ("lds_tab", "zm", "save", "persist")),
               differ_by_sine=int((ref_cr["theta"] != ref["theta"]).sum()))
    env.close()
    _RECORDS[(seed, flat)] = rec
    return rec


@pytest.mark.parametrize("seed, flat", LEVEL1, ids=[f"seed{s}{'-flat' if fl else ''}" for s, fl in LEVEL1])
def test_device_loop_on_random_raw_tables(pr, crh, seed, flat):  # noqa: F811
    _level1(pr, crh, seed, flat)


def _instances(recs):
    out = {}
    for r in recs:
        out[r["instance"]] = out.get(r["instance"], 0) + 1
    return dict(sorted(out.items()))


def test_the_level1_sweep_holds_what_it_is_meant_to(pr, crh):  # noqa: F811
    """the tallies over the level-1 cases (each case's record is kept by its own test; a case not run yet is run here)"""
    recs = [_level1(pr, crh, seed, flat) for seed, flat in LEVEL1]
    tally = {k: int(sum(r[k] for r in recs)) for k in ("brackets", "found", "dropped", "limit", "all_trials", "mirrored", "hbm",
                                                       "flat", "tb_false", "differ_by_sine")}
    print(f"\n{len(recs)} random environments: {tally}; brackets per case {min(r['brackets'] for r in recs)} ... "
          f"{max(r['brackets'] for r in recs)}; trial fans' instances (lds_tab, zm, save, persist): {_instances(recs)}")
    assert not level_misses(recs, True), (level_misses(recs, True), tally)
    # the two sines are not one test run twice: NumPy's sine differs from the correctly rounded one about once in a thousand
    # calls (tests/test_crmath.py), the sweep shoots some 15 000 trial rays, and a trial ray one ulp off moves its bracket's
    # next angle (17 brackets on the oracle)
    assert tally["differ_by_sine"] >= 5, tally


@pytest.mark.parametrize("seed, flat, kind, past", TILED, ids=[f"seed{s}-{k}-{p}" for s, _, k, p in TILED])
def test_tiled_brackets_past_the_sharing_thresholds(pr, seed, flat, kind, past):  # noqa: F811
    """Up to 1024 brackets get a wave each of the trial fan (spread 64); more share waves, 2, 4 ... 64 to a wave: the same
    brackets many times over give the oracle loop's result in every copy, with the same launches."""
    from pygenray_amd import _lib
    e = level1_expectation(seed, flat)
    arrs, kw, shot, ref = e["arrs"], e["kw"], e["shot"], e["ref"]
    n = len(e["th1"])
    reps = past // n + 1
    assert n * reps > past and per_wave_of(n) == 1
    assert per_wave_of(n * reps) == {1024: 2, 32768: 64}[past]        # (spread = 64 / per_wave: 1 past 32768 brackets)
    env = _lib.EnvHandle(*arrs)
    assert {"lds": env.lds_path, "hbm": not env.lds_path, "mirrored": e["mirrored"]}[kind], e["desc"]
    got = env.eigen_refine(*(np.tile(e[k], reps) for k in ("th1", "th2", "z1", "z2", "rd_k")), e["src"], kw["x0"], kw["x1"],
                           e["c0"], slowness=numpy_slowness(e["c0"]), ztol=ZTOL, max_iter=MAX_ITER, **shot)
    env.close()
    same_search(got, ref, f"seed {seed} tiled {reps} times: {e['desc']}", reps=reps)
    assert len(set(ref["state"])) >= 2                                # (more than one outcome among the brackets)


# ---- level 2: pr.find_eigenrays in frames derived by hand ---------------------------------------------------------------------

def _environment(pr, arrs, lat):  # noqa: F811
    cin, cpin, rin, zin, bdep, brng, bang = arrs
    return pr.OceanEnvironment2D(pr.DataArray(cin, dims=["range", "depth"], coords={"range": rin, "depth": zin}),
                                 pr.DataArray(bdep, dims=["range"], coords={"range": brng}), lat=lat)


def _search(pr, fan, e, env, fe, S=None, rds=None):  # noqa: F811
    """pr.find_eigenrays as the issue calls it -> (EigenRays, LAST_SEARCH_STATS of the call)"""
    from pygenray_amd import eigenrays
    eigenrays.LAST_SEARCH_STATS.clear()
    er = pr.find_eigenrays(fan, e["rds"] if rds is None else rds, e["src"], e["xs"], e["xr"], e["S"] if S is None else S, env,
                           ztol=1, max_iter=20, quiet=True, flatearth=fe, **e["shot"])
    return er, dict(eigenrays.LAST_SEARCH_STATS)


def same_eigenrays(er, stats, e, label, S=None, traj=None):
    """an EigenRays against the oracle loop of e, depth by depth; traj: the oracle's rays of the found angles (S samples)"""
    ref, S = e["ref"], e["S"] if S is None else S
    found = ref["state"] == 1
    assert stats["reshot_differs"] == 0, (label, stats)
    assert stats["launches"] == ref["launches"] + bool(found.any()), (label, stats, ref["launches"])
    assert stats["trial_rays"] == int(ref["n_trial"].sum()), (label, stats)
    nth = np.cumsum(found) - 1                                      # row of a found bracket in traj
    for i, (rd, sl) in enumerate(zip(e["rds"], e["per_depth"])):
        lab = (label, f"receiver depth {i}")
        f = found[sl]
        assert er.num_eigenrays[rd] == sl.stop - sl.start and er.num_eigenrays_found[i] == int(f.sum()), lab
        failed = np.array(er.failed_eray_theta_brackets[i], dtype=float).reshape(-1, 2)
        assert np.array_equal(failed, np.stack([e["th1"][sl][~f], e["th2"][sl][~f]], 1)), (lab, "failed brackets")
        assert _bits(er.launch_angles[i], ref["theta"][sl][f]), (lab, "launch angles")
        zs, ts, ps, rs = (np.asarray(a[i]) for a in (er.zs, er.ts, er.ps, er.rs))
        assert zs.shape == ts.shape == ps.shape == rs.shape == (int(f.sum()), S), lab
        assert _bits(zs[:, -1], ref["z_end"][sl][f]) and _bits(ts[:, -1], ref["t_end"][sl][f]), (lab, "end states")
        assert np.all(rs == np.linspace(e["xs"], e["xr"], S)), (lab, "rs")
        if traj is not None:
            rows = nth[sl][f]
            assert np.all(traj["status"][rows] == 0), lab
            assert np.array_equal(er.n_botts[i], traj["n_bott"][rows]) and np.array_equal(er.n_surfs[i], traj["n_surf"][rows]), lab
            want = {k: traj[k][rows] for k in ("status", "n_bott", "n_surf", "T", "z", "p", "xi", "n_steps")}
            test = dict(status=np.zeros(len(rows), np.int32), n_bott=np.asarray(er.n_botts[i]), n_surf=np.asarray(er.n_surfs[i]),
                        T=ts, z=-zs, p=-ps, end=np.stack([ts[:, -1], -zs[:, -1], -ps[:, -1]], 1), n_steps=want["n_steps"])
            assert_bit_parity(test, want, label=f"{label}, receiver depth {i}", samples=False)


def same_results(a, b, n_depths, label):
    """two EigenRays equal, array for array"""
    assert a.num_eigenrays == b.num_eigenrays and a.num_eigenrays_found == b.num_eigenrays_found, label
    assert a.failed_eray_theta_brackets == b.failed_eray_theta_brackets, label
    for name in ("rs", "ts", "zs", "ps", "launch_angles", "received_angles", "n_botts", "n_surfs", "ray_id", "ray_id_int"):
        for i in range(n_depths):
            x, y = np.asarray(getattr(a, name)[i]), np.asarray(getattr(b, name)[i])
            assert x.shape == y.shape and (np.array_equal(x, y) if x.dtype.kind in "US" else _bits(x, y)), (label, name, i)


def _level2(pr, seed, lat, backwards, fe):  # noqa: F811
    key = (seed, backwards, fe)
    if key in _API_RECORDS:
        return _API_RECORDS[key]
    from pygenray_amd.launch_rays import _device_env
    e = level2_expectation(seed, lat, backwards, fe)
    ref, S, src, xs, xr, shot = e["ref"], e["S"], e["src"], e["xs"], e["xr"], e["shot"]
    label = f"seed {seed} {'backwards' if backwards else 'forwards'} flatearth={fe}: {e['desc']}"
    fig = figures(ref)
    assert not misses(fig), (label, misses(fig))
    env = _environment(pr, e["arrs"], lat)
    host, dev = (pr.shoot_rays(src, xs, e["th"], xr, S, env, debug=False, flatearth=fe, device_resident=dr, **shot)
                 for dr in (False, True))
    assert not host.device_resident and dev.device_resident, label
    assert _bits(host.thetas, e["theta"]) and _bits(dev.thetas, e["theta"]), (label, "the fan's surviving angles")
    assert _bits(np.asarray(host.zs)[:, -1], e["z_end"]) and _bits(dev.zs_end, e["z_end"]), (label, "the fan's end depths")
    found = ref["state"] == 1
    traj = found_trajectories(e["frame_arrs"], src, e["x0"], e["x1"], S, e["c0"], ref["theta"][found], shot)
    results = []
    for fan, where in ((dev, "device fan"), (host, "host fan")):
        er, stats = _search(pr, fan, e, env, fe)
        instance = _device_env(env, fe, backwards)[0].last_instance()
        same_eigenrays(er, stats, e, f"{label} ({where})", traj=traj)
        assert fan.device_resident == (fan is dev), label
        results.append(er)
    same_results(results[0], results[1], len(e["rds"]), label)
    # pr.shoot_ray of three found angles: the eigenray returned, bit for bit
    er = results[1]
    where = [(i, k) for i in range(len(e["rds"])) for k in range(er.num_eigenrays_found[i])]
    for i, k in [where[0], where[len(where) // 2], where[-1]]:
        ray = pr.shoot_ray(src, xs, er.launch_angles[i][k], xr, S, env, debug=False, flatearth=fe, **shot)
        assert ray is not None and ray.launch_angle == -er.launch_angles[i][k], (label, i, k)
        assert _bits(ray.t, er.ts[i][k]) and _bits(ray.z, er.zs[i][k]) and _bits(ray.p, er.ps[i][k]), (label, "shoot_ray", i, k)
        assert _bits(ray.r, er.rs[i][k]) and ray.n_bottom == er.n_botts[i][k] and ray.n_surface == er.n_surfs[i][k], (label, i, k)
    rec = dict(fig, instance=tuple(instance[k] for k in ("lds_tab", "zm", "save", "persist")))
    _API_RECORDS[key] = rec
    return rec


@pytest.mark.parametrize("fe", [False, True], ids=["flatearth-off", "flatearth-on"])
@pytest.mark.parametrize("backwards", [False, True], ids=["forwards", "backwards"])
@pytest.mark.parametrize("seed, lat", LEVEL2, ids=[f"seed{s}" for s, _ in LEVEL2])
def test_find_eigenrays_in_frames_derived_by_hand(pr, seed, lat, backwards, fe):  # noqa: F811
    _level2(pr, seed, lat, backwards, fe)


def test_the_level2_sweep_holds_what_it_is_meant_to(pr):  # noqa: F811
    """the tallies over the 48 frames (each frame's record is kept by its own test; a frame not run yet is run here)"""
    recs = [_level2(pr, seed, lat, backwards, fe) for seed, lat in LEVEL2 for backwards in (False, True) for fe in (False, True)]
    tally = {k: int(sum(r[k] for r in recs)) for k in ("brackets", "found", "dropped", "limit", "all_trials")}
    print(f"\n{len(recs)} frames: {tally}; brackets per frame {min(r['brackets'] for r in recs)} ... "
          f"{max(r['brackets'] for r in recs)}; re-shoots' instances (lds_tab, zm, save, persist): {_instances(recs)}")
    assert not level_misses(recs, False), (level_misses(recs, False), tally)


# ---- the re-shoot with spread = 1, both triggers ------------------------------------------------------------------------------

def _one_depth_at_a_time(pr, host, e, env, fe, label):  # noqa: F811
    """the search of every receiver depth of e on its own at S = 2 -> [EigenRays]; held to the oracle loop here"""
    out = []
    for i, (rd, sl) in enumerate(zip(e["rds"], e["per_depth"])):
        er, _ = _search(pr, host, e, env, fe, S=2, rds=[rd])
        f = e["ref"]["state"][sl] == 1
        assert er.num_eigenrays[rd] == sl.stop - sl.start and er.num_eigenrays_found[0] == int(f.sum()), (label, i)
        assert _bits(er.launch_angles[0], e["ref"]["theta"][sl][f]), (label, i)
        out.append(er)
    return out


def _equal_depth_by_depth(er, singles, e, label):
    for i, (rd, one) in enumerate(zip(e["rds"], singles)):
        lab = (label, f"receiver depth {i}")
        assert er.num_eigenrays[rd] == one.num_eigenrays[rd] and er.num_eigenrays_found[i] == one.num_eigenrays_found[0], lab
        assert er.failed_eray_theta_brackets[i] == one.failed_eray_theta_brackets[0], lab
        assert _bits(er.launch_angles[i], one.launch_angles[0]), lab
        for name in ("ts", "zs", "ps"):
            assert _bits(np.asarray(getattr(er, name)[i])[:, -1], np.asarray(getattr(one, name)[0])[:, -1]), (lab, name)
        assert np.array_equal(er.n_botts[i], one.n_botts[0]) and np.array_equal(er.n_surfs[i], one.n_surfs[0]), lab


def _spread_case(pr, quantiles):  # noqa: F811
    lat = dict(API_CASES)[SPREAD_SEED]
    e = level2_expectation(SPREAD_SEED, lat, False, False, quantiles)
    assert "range-dep True" in e["desc"] and np.ptp(e["arrs"][4]) > 0, e["desc"]     # range dependent, over a sloping floor
    env = _environment(pr, e["arrs"], lat)
    host = pr.shoot_rays(e["src"], e["xs"], e["th"], e["xr"], e["S"], env, debug=False, flatearth=False, device_resident=False,
                         **e["shot"])
    assert _bits(host.thetas, e["theta"]) and _bits(np.asarray(host.zs)[:, -1], e["z_end"])
    return e, env, host


def test_reshoot_of_more_than_1024_eigenrays(pr):  # noqa: F811
    """spread = 1 by its first trigger: N_DEPTHS receiver depths searched together find more than 1024 eigenrays"""
    e, env, host = _spread_case(pr, tuple(np.linspace(0.05, 0.95, N_DEPTHS)))
    n_found = int((e["ref"]["state"] == 1).sum())
    label = f"seed {SPREAD_SEED}, {N_DEPTHS} receiver depths, {n_found} found"
    assert n_found > 1024, label
    er, stats = _search(pr, host, e, env, False)
    same_eigenrays(er, stats, e, label)
    _equal_depth_by_depth(er, _one_depth_at_a_time(pr, host, e, env, False, label), e, label)


def test_reshoot_of_trajectories_too_long_to_pad(pr):  # noqa: F811
    """spread = 1 by its second trigger: fewer than 1024 eigenrays whose padded launch would own more than 256 MiB a buffer"""
    e, env, host = _spread_case(pr, QUANTILES)
    n_found = int((e["ref"]["state"] == 1).sum())
    S = MIB256 // (n_found * 64 * 24) + 1
    label = f"seed {SPREAD_SEED}, {n_found} found, S {S}"
    assert 0 < n_found <= 1024 and n_found * 64 * S * 24 > MIB256 >= n_found * 64 * (S - 1) * 24, label
    er, stats = _search(pr, host, e, env, False, S=S)
    found = e["ref"]["state"] == 1
    traj = found_trajectories(e["frame_arrs"], e["src"], e["x0"], e["x1"], S, e["c0"], e["ref"]["theta"][found], e["shot"])
    same_eigenrays(er, stats, e, label, S=S, traj=traj)
    _equal_depth_by_depth(er, _one_depth_at_a_time(pr, host, e, env, False, label), e, label)


if __name__ == "__main__":
    cpu_check()
