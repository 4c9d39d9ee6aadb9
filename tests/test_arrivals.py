"""arrivals on the GPU (csrc/pgr_arrivals.h): bit parity with the NumPy restatement of tests/arrivals_reference.py on the
kernel's chunk, band and adds-nothing edges, the sum identity with transmission_loss on every fan path, the isovelocity
image sources and the linear-gradient closed form end to end, the eigenray search's brackets, and the headline fan."""
import numpy as np
import pytest

import arrivals_reference as ar
import tl_reference as tlr
from test_arrivals_host import check_gradient_arrivals
from tube_gpu import (DEPTHS, SYN_R, SYN_Z, _device_arrivals, _env, munk_env, pr, pr_any, sloping_env,  # noqa: F401
                      sloping_env_shallow_table, syn_env, synthetic_fan)  # (pr, pr_any, syn_env: fixtures)

pytestmark = pytest.mark.gpu


def _same_arrivals(a, b):
    """two Arrivals (or an Arrivals and a restatement dict) hold the same arrivals, bit for bit"""
    get = (lambda o, k: o[k]) if isinstance(b, dict) else (lambda o, k: getattr(o, k))
    names = [("offsets", "offsets"), ("tube", "tube"), ("w", "w"), ("time", "T"), ("p", "p"), ("intensity", "I")]
    for mine, theirs in names:
        x, y = getattr(a, mine), get(b, theirs if isinstance(b, dict) else mine)
        assert len(x) == len(y) and ar.same(x, y), mine
    return True


def _check_sum_identity(a, I_tl):
    """the arrivals of every (receiver, requested column), added in order from 0.0, give TL's intensity bit for bit"""
    R, n = len(a.receiver_depths), len(a.range_indices)
    sums = ar.sequential_sums(a.offsets, a.intensity).reshape(R, n)
    ref = I_tl[:, a.range_indices]
    src = np.isnan(ref).all(axis=0)                          # the source's own column: NaN in TL, no arrivals
    assert (np.diff(a.offsets).reshape(R, n)[:, src] == 0).all()
    assert ar.same(sums[:, ~src], ref[:, ~src])
    assert len(a) > 0


# ---- the kernel on synthetic inputs: pgr_arrival*_device against tube_arrivals, bit for bit ----------------------------

def _synthetic_t(M, S, seed):
    """a travel time per (sample, ray): a monotone random walk in s, a few NaNs"""
    rng = np.random.default_rng(seed + 7)
    T = np.cumsum(rng.uniform(0.5, 2.0, (S, M)), axis=0)
    if M >= 8:
        T[S - 1, M // 2] = np.nan
        T[0, 1] = np.nan
    return T


SYN_CASES = ([(M, 5, 129, False) for M in (2, 3, 63, 64, 65, 127, 128, 4033, 4034, 8300)]
             + [(500, 5, R, False) for R in (1, 63, 64, 65, 4200)]
             + [(300, S, 100, False) for S in (1, 2)]
             + [(4100, 6, 300, True)])


def _column_lists(S, seed):
    rng = np.random.default_rng(seed)
    lists = [[S - 1], list(range(S)), list(rng.permutation(S)), [S - 1, 0, S - 1, S // 2, S // 2]]
    return [np.asarray(c, dtype=np.int32) for c in lists]


@pytest.mark.parametrize("M, S, R, shuffle", SYN_CASES, ids=[f"M{M}-S{S}-R{R}{'-shuffled' if sh else ''}"
                                                              for M, S, R, sh in SYN_CASES])
def test_kernel_bit_identical_on_synthetic_inputs(pr, syn_env, M, S, R, shuffle):
    env, cin = syn_env
    seed = M * 1009 + S * 31 + R
    z, p, x, p0, depths = synthetic_fan(M, S, R, seed=seed, cin=cin, shuffle=shuffle)
    t = _synthetic_t(M, S, seed)
    I_tl = tlr.tube_intensity(z.T, p.T, x, p0, depths, cin, SYN_R, SYN_Z)
    hits = 0
    for cols in _column_lists(S, seed):
        got = _device_arrivals(env, t, z, p, x, p0, depths, cols)
        ref = ar.tube_arrivals(z.T, p.T, t.T, x, p0, depths, cols, cin, SYN_R, SYN_Z)
        for k in ("offsets", "tube", "w", "T", "p", "I"):
            assert len(got[k]) == len(ref[k]) and ar.same(got[k], ref[k]), (k, cols)
        sums = ar.sequential_sums(got["offsets"], got["I"]).reshape(R, len(cols))
        live = x[cols] != x[0]
        assert ar.same(sums[:, live], I_tl[:, cols][:, live])
        hits += len(got["tube"])
    if M >= 8 and S >= 3:
        assert hits > 0                                        # (not vacuous: tubes reached receivers)


# ---- fans: the restatement, TL's sum, one answer whatever the path ------------------------------------------------------

@pytest.mark.parametrize("case", ["munk", "sloping", "flatearth"])
def test_fan_arrivals_bit_identical_and_sum_to_tl(pr, case):
    if case == "munk":
        env, fe, blocked = munk_env(pr), False, False
    elif case == "sloping":
        env, fe, blocked = sloping_env(pr), False, True
    else:
        env, fe, blocked = pr.OceanEnvironment2D(), True, False
    fan = pr.shoot_rays(1000.0, 0.0, np.linspace(-20, 20, 3000), 100e3, 201, env, flatearth=fe, debug=False,
                        device_resident=True)
    assert fan.device_resident and fan._dev._env.blocked_layout == blocked
    I_tl = pr.transmission_loss(fan, DEPTHS, env, flatearth=fe, intensity=True)
    a = pr.arrivals(fan, DEPTHS, env, flatearth=fe, range_indices=np.arange(201))
    assert fan.device_resident and "_zs" not in fan.__dict__ and "_ts" not in fan.__dict__   # nothing fetched
    _check_sum_identity(a, I_tl)
    cols = [200, 0, 17, -1, 123, 64, 65]
    b = pr.arrivals(fan, DEPTHS, env, flatearth=fe, range_indices=cols)
    assert list(b.range_indices) == [200, 0, 17, 200, 123, 64, 65] and ar.same(b.ranges, np.asarray(fan.rs[0])[b.range_indices])
    assert _same_arrivals(b, ar.fan_arrivals(fan, DEPTHS, env, b.range_indices, flatearth=fe))
    # the derived fields
    t0, t1 = fan.thetas[b.tube], fan.thetas[b.tube + 1]
    assert ar.same(b.launch_angle, t0 + b.w * (t1 - t0)) and ar.same(b.amplitude, np.sqrt(b.intensity))
    assert np.nanmax(np.abs(b.received_angle)) < 90 and np.isfinite(b.received_angle).mean() > 0.99
    j, c = 500, 4
    rec = b.at(j, c)
    sl = slice(b.offsets[j * 7 + c], b.offsets[j * 7 + c + 1])
    assert ar.same(rec["time"], b.time[sl]) and len(rec["tube"]) == sl.stop - sl.start
    assert (np.diff(rec["tube"]) > 0).all()


def test_default_column_is_the_receiver_range(pr):
    env = munk_env(pr)
    fan = pr.shoot_rays(1000.0, 0.0, np.linspace(-10, 10, 300), 50e3, 51, env, flatearth=False, debug=False)
    a = pr.arrivals(fan, [1000.0, 2000.0], env, flatearth=False)
    assert list(a.range_indices) == [50] and a.ranges[0] == 50e3 and len(a.offsets) == 3
    assert _same_arrivals(a, ar.fan_arrivals(fan, [1000.0, 2000.0], env, [50], flatearth=False))
    src = pr.arrivals(fan, [1000.0, 2000.0], env, flatearth=False, range_indices=[0])
    assert len(src) == 0 and (src.offsets == 0).all()


@pytest.mark.parametrize("envf", [sloping_env, munk_env], ids=["sloping", "munk"])
def test_one_answer_whatever_the_path(pr, envf):
    env = envf(pr)
    ang = np.linspace(-20, 20, 3000)
    dev = pr.shoot_rays(1000.0, 0.0, ang, 100e3, 201, env, flatearth=False, debug=False, device_resident=True)
    host = pr.shoot_rays(1000.0, 0.0, ang, 100e3, 201, env, flatearth=False, debug=False, device_resident=False)
    cols = np.arange(0, 201, 5)
    a = pr.arrivals(dev, DEPTHS, env, flatearth=False, range_indices=cols)
    assert dev.device_resident
    b = pr.arrivals(host, DEPTHS, env, flatearth=False, range_indices=cols)
    assert _same_arrivals(a, b)
    _check_sum_identity(b, pr.transmission_loss(host, DEPTHS, env, flatearth=False, intensity=True))
    dev.to_host()
    assert _same_arrivals(a, pr.arrivals(dev, DEPTHS, env, flatearth=False, range_indices=cols))


@pytest.mark.parametrize("envf", [munk_env, sloping_env_shallow_table], ids=["rows", "sample-blocked"])
def test_dropped_rays_are_skipped_and_their_neighbours_joined(pr, envf):
    env = envf(pr, ztop=4200.0) if envf is munk_env else envf(pr)
    ang = np.linspace(-20, 20, 800)
    dev = pr.shoot_rays(1000.0, 0.0, ang, 100e3, 101, env, flatearth=False, debug=False, device_resident=True)
    host = pr.shoot_rays(1000.0, 0.0, ang, 100e3, 101, env, flatearth=False, debug=False, device_resident=False)
    assert 20 < len(ang) - len(dev) < 700 and len(dev) == len(host)
    assert dev._dev._env.blocked_layout == (envf is not munk_env)
    cols = np.arange(101)
    a = pr.arrivals(dev, DEPTHS, env, flatearth=False, range_indices=cols)
    assert dev.device_resident
    b = pr.arrivals(host, DEPTHS, env, flatearth=False, range_indices=cols)
    assert _same_arrivals(a, b) and _same_arrivals(b, ar.fan_arrivals(host, DEPTHS, env, cols, flatearth=False))
    _check_sum_identity(a, pr.transmission_loss(dev, DEPTHS, env, flatearth=False, intensity=True))


def test_backwards_fans(pr):
    env = sloping_env(pr)
    args = (900.0, 150e3, np.linspace(-15, 15, 500), 40e3, 111, env)
    dev = pr.shoot_rays(*args, flatearth=False, debug=False, device_resident=True)
    host = pr.shoot_rays(*args, flatearth=False, debug=False, device_resident=False)
    cols = np.arange(111)
    a = pr.arrivals(dev, DEPTHS, env, flatearth=False, range_indices=cols)
    b = pr.arrivals(host, DEPTHS, env, flatearth=False, range_indices=cols)
    assert _same_arrivals(a, b) and _same_arrivals(b, ar.fan_arrivals(host, DEPTHS, env, cols, flatearth=False))
    _check_sum_identity(a, pr.transmission_loss(dev, DEPTHS, env, flatearth=False, intensity=True))
    assert a.ranges[0] == 150e3 and a.ranges[-1] == 40e3


def test_flatearth_host_fan(pr):
    env = pr.OceanEnvironment2D()
    args = (1000.0, 0.0, np.linspace(-20, 20, 3000), 100e3, 201, env)
    dev = pr.shoot_rays(*args, debug=False, device_resident=True)
    host = pr.shoot_rays(*args, debug=False, device_resident=False)
    cols = np.arange(0, 201, 4)
    a = pr.arrivals(dev, DEPTHS, env, range_indices=cols)
    b = pr.arrivals(host, DEPTHS, env, range_indices=cols)
    assert _same_arrivals(a, b) and _same_arrivals(b, ar.fan_arrivals(host, DEPTHS, env, cols))
    _check_sum_identity(b, pr.transmission_loss(host, DEPTHS, env, intensity=True))


# ---- closed forms end to end -------------------------------------------------------------------------------------------

def test_isovelocity_fan_gives_one_arrival_per_image_source(pr_any):
    z = np.arange(0, 6000, 10.0)
    r = np.linspace(0, 25e3, 6)
    env = _env(pr_any, z, r, np.full((len(r), len(z)), 1500.0), r, np.full(len(r), 5000.0))
    fan = pr_any.shoot_rays(1000.0, 0.0, np.linspace(-80, 80, 20001), 20e3, 2001, env, flatearth=False, debug=False)
    assert len(fan) == 20001 and fan.device_resident
    depths = np.arange(tlr.MARGIN, 5000 - tlr.MARGIN + 1, 50.0)
    x = np.asarray(fan.rs[0])
    cols = np.nonzero((x >= 1e3) & (x <= 20e3))[0][::10]
    a = pr_any.arrivals(fan, depths, env, flatearth=False, range_indices=cols)
    assert fan.device_resident
    zs, ps = np.asarray(fan.zs), np.asarray(fan.ps)
    n, spacing = len(cols), 160.0 / 20000
    worst_t, dbs = 0.0, []
    for j, D in enumerate(depths):
        for c, s in enumerate(cols):
            rec = a.at(j, c)
            R_img, ang = ar.isovelocity_images(x[s], D, 1000.0, 5000.0, 80.0)
            assert len(rec["time"]) == len(R_img), (D, x[s])
            # matched by launch angle (thetas: positive up), one image per arrival and one arrival per image
            match = np.abs(rec["launch_angle"][:, None] + ang[None, :]) <= spacing
            assert (match.sum(axis=1) == 1).all() and (match.sum(axis=0) == 1).all(), (D, x[s])
            q = np.argmax(match, axis=1)
            ref = R_img[q] / 1500.0
            bound = ar.tube_time_bound(ps, zs, rec["tube"], s)
            excess = np.abs(rec["time"] - ref) - 4e-16 * ref
            assert (excess <= bound).all(), (D, x[s], excess.max(), bound.max())
            worst_t = max(worst_t, (excess / bound).max())
            dbs.append(np.abs(tlr.to_db(rec["intensity"]) - tlr.to_db(1.0 / R_img[q] ** 2)))
    db = np.concatenate(dbs)
    q50, q99, q999 = np.quantile(db, [0.5, 0.99, 0.999])
    print(f"isovelocity: {len(db)} arrivals, worst |T - R/c0| {worst_t:.3f} of the tube bound; |dI| median {q50:.2e}, "
          f"99 % {q99:.2e}, 99.9 % {q999:.2e}, worst {db.max():.3f} dB ({(db > tlr.TOL_DB).sum()} above {tlr.TOL_DB} dB)")
    # a single tube's I carries the fan's sampling next to reflections undiluted by its neighbours: the
    # bound holds for all but a few tubes
    assert q99 < tlr.TOL_DB and (db > tlr.TOL_DB).mean() < 1e-3


@pytest.mark.parametrize("device_resident", [True, False])
def test_linear_gradient_fan_matches_the_closed_form(pr_any, device_resident):
    env = tlr.gradient_env()
    fan = pr_any.shoot_rays(tlr.GRADIENT_ZS, 0.0, np.linspace(-tlr.GRADIENT_APERTURE, tlr.GRADIENT_APERTURE, 2001),
                        tlr.GRADIENT_X1, tlr.GRADIENT_S, env, flatearth=False, debug=False, device_resident=device_resident)
    x = np.asarray(fan.rs[0])
    cols = np.nonzero(x >= 1e3)[0]
    a = pr_any.arrivals(fan, tlr.GRADIENT_DEPTHS, env, flatearth=False, range_indices=cols)
    I = pr_any.transmission_loss(fan, tlr.GRADIENT_DEPTHS, env, flatearth=False, intensity=True)
    assert fan.device_resident == device_resident
    c_s = tlr.GRADIENT_CA + tlr.GRADIENT_GAMMA * tlr.GRADIENT_ZS
    theta0 = np.arcsin(-np.asarray(fan.ps)[:, 0] * c_s)       # depth-down, from the fan itself (as the TL test)
    worst = check_gradient_arrivals(dict(offsets=a.offsets, tube=a.tube, w=a.w, T=a.time, I=a.intensity), x, cols,
                                    fan.zs, fan.ps, fan.ts, I, theta_deg=-np.degrees(theta0), launch_angle=a.launch_angle)
    print(f"linear gradient: worst interpolation error {worst:.3f} of the tube bound")


# ---- against the eigenray search ---------------------------------------------------------------------------------------

def test_last_column_tubes_are_the_eigenray_brackets(pr):
    from pygenray_amd.eigenrays import _bracket
    env = pr.OceanEnvironment2D()
    fan = pr.shoot_rays(1000.0, 0.0, np.linspace(-20, 20, 2001), 100e3, 101, env, debug=False, device_resident=True)
    depths = np.array([523.7, 1234.5, 2750.3, 3801.1])
    a = pr.arrivals(fan, depths, env)
    assert fan.device_resident
    ztol = 1e-3
    er = pr.find_eigenrays(fan, depths, 1000.0, 0.0, 100e3, 11, env, ztol=ztol, max_iter=80)
    z_end = np.asarray(fan.zs_end)
    dd = np.diff(-z_end)
    worst, folds, missed, compared = 0.0, 0, 0, 0
    for j, D in enumerate(depths):
        rec = a.at(j, 0)
        starts = _bracket(fan, D)[0]
        assert np.array_equal(rec["tube"], starts) and len(starts) == er.num_eigenrays[D]
        # the eigenrays found, matched to their brackets by launch angle
        th_e, T_e = er.launch_angles[j], er.ts[j][:, -1]
        lo = np.minimum(fan.thetas[starts], fan.thetas[starts + 1])
        hi = np.maximum(fan.thetas[starts], fan.thetas[starts + 1])
        for k, tube in enumerate(starts):
            if not (0 < tube < len(dd) - 1 and np.sign(dd[tube - 1]) == np.sign(dd[tube]) == np.sign(dd[tube + 1])):
                folds += 1
                continue
            m = np.nonzero((th_e >= lo[k]) & (th_e <= hi[k]))[0]
            assert len(m) <= 1, (D, tube)
            if len(m) == 0:
                missed += 1                                    # the search did not converge in this bracket
                continue
            bound = 0.5 * abs(fan.ps_end[tube + 1] - fan.ps_end[tube]) * abs(dd[tube])
            tol = bound + abs(rec["p"][k]) * ztol + 1e-9 * T_e[m[0]]
            assert abs(rec["time"][k] - T_e[m[0]]) <= tol, (D, tube, rec["time"][k] - T_e[m[0]], bound)
            worst = max(worst, abs(rec["time"][k] - T_e[m[0]]) / tol)
            compared += 1
    assert compared > 10 * missed
    print(f"eigenrays: {compared} brackets compared, worst |T - T_eigenray| {worst:.3f} of the tolerance; {folds} fold "
          f"brackets left out, {missed} not found by the search")


# ---- headline scale ----------------------------------------------------------------------------------------------------

def test_headline_fan_twice_bit_equal(pr_any):
    env = pr_any.OceanEnvironment2D()
    fan = pr_any.shoot_rays(1000.0, 0.0, np.linspace(-20, 20, 100_000), 100e3, 1001, env, debug=False)
    assert fan.device_resident and len(fan) > 90_000
    I_tl = pr_any.transmission_loss(fan, DEPTHS, env, intensity=True)
    for cols in (None, np.arange(0, 1001, 50)):
        a = pr_any.arrivals(fan, DEPTHS, env, range_indices=cols)
        b = pr_any.arrivals(fan, DEPTHS, env, range_indices=cols)
        assert fan.device_resident and "_zs" not in fan.__dict__
        assert _same_arrivals(a, b)
        _check_sum_identity(a, I_tl)


# ---- errors ------------------------------------------------------------------------------------------------------------

def test_value_errors(pr):
    env = pr.OceanEnvironment2D()
    fan = pr.shoot_rays(1000.0, 0.0, np.linspace(-10, 10, 100), 20e3, 21, env, debug=False, device_resident=True)
    with pytest.raises(ValueError, match="another environment"):
        pr.arrivals(fan, [100.0], env, flatearth=False)
    with pytest.raises(ValueError, match="ascending"):
        pr.arrivals(fan, [100.0, 50.0], env)
    for ri, msg in (([], "non-empty"), ([21], "lie in"), ([-22], "lie in"), ([2.0], "integers")):
        with pytest.raises(ValueError, match=msg):
            pr.arrivals(fan, [100.0], env, range_indices=ri)
    with pytest.raises(ValueError, match="Flat earth transformation has not been applied"):
        pr.arrivals(fan, [100.0], munk_env(pr))
    assert fan.device_resident
    a = pr.arrivals(fan, [100.0, 2000.0], env, range_indices=[-1, -21, 20])
    assert list(a.range_indices) == [20, 0, 20]


def test_the_c_entries_refuse_bad_columns(pr, syn_env):
    import torch
    from pygenray_amd import _lib
    env, cin = syn_env
    z, p, x, p0, depths = synthetic_fan(10, 5, 3, seed=1, cin=cin)
    dev = torch.device("cuda", env.device)
    d = [torch.from_numpy(np.ascontiguousarray(a)).to(dev) for a in (z, p, x, p0, depths)]
    counts = torch.zeros(3 * 2, dtype=torch.int64, device=dev)
    for cols, msg in (([0, 5], "not a column"), ([-1, 0], "not a column")):
        with pytest.raises(RuntimeError, match=msg):
            _lib.arrival_counts_device(env, d[0].data_ptr(), d[1].data_ptr(), 10, 5, d[2].data_ptr(), d[3].data_ptr(),
                                       d[4].data_ptr(), 3, cols, counts.data_ptr())
    with pytest.raises(RuntimeError, match="n_cols"):
        _lib.arrival_counts_device(env, d[0].data_ptr(), d[1].data_ptr(), 10, 5, d[2].data_ptr(), d[3].data_ptr(),
                                   d[4].data_ptr(), 3, np.zeros(0, np.int32), counts.data_ptr())
