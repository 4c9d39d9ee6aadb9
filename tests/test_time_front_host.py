"""RayFan.turning_points / RayFan.time_front / TimeFront on host fans, against the restatement (tests/front_reference.py):
synthetic slowness blocks with zeros of both signs and NaNs, one- and two-sample fans, trajectories the reference itself
produced, the column validation, and Arrivals built without the counts.  No GPU."""
import os

import numpy as np
import pytest

import front_reference as fr

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def _same(a, b):
    return np.array_equal(a, b, equal_nan=True)


def _host_fan(T, z, p, seed=0):
    from pygenray_amd import RayFan
    M, S = p.shape
    rng = np.random.default_rng(seed)
    thetas = np.linspace(-15.0, 15.0, M) if M > 1 else np.array([3.0])
    if M > 5:
        thetas[M // 2] = 0.0
    rs = np.broadcast_to(np.linspace(0.0, 50e3, S), (M, S))
    return RayFan.from_arrays(thetas, rs, T, z, p, rng.integers(0, 3, M), rng.integers(0, 2, M), np.full(M, 1000.0))


def _check_fan(fan, p, cols_list):
    M, S = p.shape
    for cols in cols_list:
        got = fan.turning_points(cols)
        assert got.dtype == np.int64 and got.shape == (M, len(cols))
        assert np.array_equal(got, fr.turning_points(p, cols))
    assert np.array_equal(fan.turning_points(), fr.turning_points(p, [S - 1]))
    assert np.array_equal(fan.turning_points([-1, -S]), fr.turning_points(p, [S - 1, 0]))
    for k in sorted({0, min(1, S - 1), S // 2, S - 1}):
        tf = fan.time_front(k)
        assert tf.range_index == k and len(tf) == M
        assert _same(tf.t, fan.ts[:, k]) and _same(tf.z, fan.zs[:, k]) and _same(tf.p, fan.ps[:, k])
        assert _same(tf.range, fan.rs[:, k]) and _same(tf.thetas, fan.thetas)
        assert tf.turning_points.dtype == np.int64
        assert np.array_equal(tf.turning_points, fr.turning_points(p, [k])[:, 0])
        assert _same(tf.ray_numbers, fr.turning_points(p, [k])[:, 0] * np.sign(fan.thetas))
        if k != S - 1:
            assert tf.ray_ids is None
    last = fan.time_front(-1)
    assert last.range_index == S - 1
    assert np.array_equal(last.ray_ids, fan.ray_ids)
    assert np.array_equal(fan.ray_ids, fr.ray_id_strings(p, fan.thetas, fan.n_botts, fan.n_surfs))


@pytest.mark.parametrize("M, S", [(1, 1), (1, 2), (7, 1), (7, 2), (5, 5), (64, 200), (33, 1001)])
def test_host_fans_equal_the_restatement(M, S):
    T, z, p = fr.synthetic(M, S, 100 * M + S)
    assert np.isnan(p[0, 0]) and np.isnan(p[-1, -1])
    if M >= 4:
        assert not p[2].any() and not p[3].any() and np.signbit(p[3]).all()      # rays of +0.0 and of -0.0
    fan = _host_fan(T, z, p)
    _check_fan(fan, p, fr.column_cases(S, S))


def test_signed_zeros_and_nans_follow_numpy():
    """the corner cases by hand: -0.0 and +0.0 are one class, a zero between two signs is two changes, a NaN changes on
    both sides and against another NaN"""
    nan = np.nan
    p = np.array([[1.0, 2.0, -1.0, -2.0, 3.0],            # 0 0 1 1 2
                  [0.0, -0.0, 0.0, -0.0, 0.0],            # all one class
                  [1.0, 0.0, -1.0, -0.0, -1.0],           # 0 1 2 3 4
                  [1.0, nan, nan, 1.0, 1.0],              # 0 1 2 3 3
                  [nan, 1.0, 1.0, 1.0, nan],              # 0 1 1 1 2
                  [-1.0, -np.inf, np.inf, 1e-320, -1e-320]])     # 0 0 1 1 2
    want = np.array([[0, 0, 1, 1, 2], [0, 0, 0, 0, 0], [0, 1, 2, 3, 4], [0, 1, 2, 3, 3], [0, 1, 1, 1, 2], [0, 0, 1, 1, 2]])
    assert np.array_equal(fr.turning_points(p, range(5)), want)
    fan = _host_fan(np.zeros_like(p), np.zeros_like(p), p)
    assert np.array_equal(fan.turning_points(range(5)), want)
    assert np.array_equal(fan.turning_points([4, 0, 4, 2]), want[:, [4, 0, 4, 2]])


def test_reference_trajectories(golden_dir):
    """288 Munk rays to 1000 km the reference integrated (refracted and bouncing).  The vectors carry no ray id of the
    reference's own: this checks the host path on realistic input, not the definition."""
    g = np.load(os.path.join(golden_dir, "g11_munk_1000km_288.npz"))
    ok = g["ok"] == 1
    p, T, z = g["p"][ok], g["T"][ok], g["z"][ok]
    M, S = p.shape
    assert M > 200 and S == 101 and np.isfinite(p).all()
    from pygenray_amd import RayFan
    fan = RayFan.from_arrays(-g["theta_ode"][ok], np.broadcast_to(g["r"], (M, S)), T, -z, -p, g["n_bott"][ok], g["n_surf"][ok],
                             np.full(M, float(g["source_depth"])))
    cols = [0, 1, 50, S - 1]
    want = fr.turning_points(p, cols)                    # (the count does not depend on the sign convention of p)
    assert np.array_equal(want, fr.turning_points(-p, cols))
    assert want[:, -1].max() >= 10 and (want[:, 0] == 0).all()
    assert np.array_equal(fan.turning_points(cols), want)
    for i, k in enumerate(cols):
        tf = fan.time_front(k)
        assert np.array_equal(tf.turning_points, want[:, i])
        assert _same(tf.t, T[:, k]) and _same(tf.z, -z[:, k]) and _same(tf.p, -p[:, k])
    assert np.array_equal(fan.time_front(-1).ray_ids, fan.ray_ids)
    assert np.array_equal(fan.ray_ids, fr.ray_id_strings(p, fan.thetas, fan.n_botts, fan.n_surfs))
    assert any(s.endswith("b") for s in fan.ray_ids) and any(not s.endswith("b") for s in fan.ray_ids)


def test_column_validation():
    T, z, p = fr.synthetic(6, 9, 1)
    fan = _host_fan(T, z, p)
    for bad in ([9], [-10], [0, 9], [], [[0, 1]], [1.0], [True]):
        with pytest.raises(ValueError):
            fan.turning_points(bad)
    with pytest.raises(ValueError):
        fan.turning_points(np.zeros(65536, dtype=int))
    for bad in (9, -10, 1.5, [0, 1], [0]):
        with pytest.raises(ValueError):
            fan.time_front(bad)
    assert fan.time_front(-9).range_index == 0 and fan.time_front(np.int64(8)).range_index == 8


def test_plot_time_front_draws_the_time_front():
    plt = pytest.importorskip("matplotlib.pyplot")
    import matplotlib
    matplotlib.use("Agg", force=True)
    T, z, p = fr.synthetic(12, 9, 3)
    T, z = np.nan_to_num(T), np.nan_to_num(z)
    fan = _host_fan(T, z, p)
    for kw in (dict(range_idx=4), dict(range_idx=-1, ray_id=True), dict(range_idx=2, ray_id=True, include_lines=True)):
        plt.figure()
        fan.plot_time_front(**kw)
        k = kw["range_idx"] % 9
        xy = plt.gca().collections[0].get_offsets()
        assert _same(np.asarray(xy[:, 0]), T[:, k]) and _same(np.asarray(xy[:, 1]), z[:, k])
        plt.close("all")
    plt.figure()
    fan.time_front(3).plot(ray_id=True, add_colorbar=False)
    assert len(plt.gca().collections) == 1
    plt.close("all")


def test_arrivals_built_without_the_counts_still_work():
    from pygenray_amd import Arrivals
    off = np.array([0, 2, 3])
    a = Arrivals(off, np.array([100.0]), np.array([1e3, 2e3]), np.array([3, 7]), np.array([0, 1, 1], dtype=np.int32),
                 np.array([0.5, 0.25, 1.0]), np.array([1.0, 2.0, 3.0]), np.array([1e-4, -1e-4, 2e-4]),
                 np.array([1e-9, 4e-9, 9e-9]), np.array([-2.0, 2.0, 6.0]), np.full((1, 2), 1500.0))
    assert len(a) == 3 and a.turning_points is None and a.ray_number is None
    assert np.array_equal(a.launch_angle, [0.0, 3.0, 6.0]) and np.array_equal(a.at(0, 1)["tube"], [1])
    tp = np.array([[2, 2], [3, 4], [5, 5]])
    b = Arrivals(off, a.receiver_depths, a.ranges, a.range_indices, a.tube, a.w, a.time, a.p, a.intensity,
                 np.array([-2.0, -1.0, 6.0]), np.full((1, 2), 1500.0), tp)
    assert np.array_equal(b.turning_points, tp)
    assert _same(b.ray_number, [-2.0, np.nan, 5.0])
