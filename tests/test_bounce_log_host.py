"""The host side of the bounce log and boundary loss, without a GPU: the argmin rule of the
restatement against the reference's literal slice assignment, BounceLog / RayFan.bounce_counts on host fans, and every
argument the Python layer refuses before it touches a device."""
import pickle

import numpy as np
import pytest

import bounce_reference as bref
import pygenray_amd as pr
from pygenray_amd.ray_objects import BounceLog, RayFan
from pygenray_amd._fan_frame import _loss_table


def _random_events(rng, x, n):
    """n event ranges inside [x_0, x_end): some on save ranges, on midpoints, an ulp either side, several per interval"""
    picks = [rng.uniform(x[0], x[-1], n), x[rng.integers(0, len(x) - 1, n)], 0.5 * (x[:-1] + x[1:])[rng.integers(0, len(x) - 1, n)]]
    mid = 0.5 * (x[:-1] + x[1:])[rng.integers(0, len(x) - 1, n)]
    picks += [np.nextafter(mid, np.inf), np.nextafter(mid, -np.inf)]
    ev = rng.choice(np.concatenate(picks), n, replace=False)
    ev = np.sort(ev[(ev >= x[0]) & (ev < x[-1])])
    return ev[np.concatenate([[True], np.diff(ev) > 0])] if len(ev) else ev


@pytest.mark.parametrize("S", [2, 5, 13, 200])
def test_argmin_rule_is_the_reference_slice_assignment(S):
    """seg(s) = #{e: j_e <= s} (s < S - 1), seg(S - 1) = E names the segment that owns sample s in _interpolate_ray's
    slice assignment, for random event sets with ties, skipped segments and events on save ranges."""
    rng = np.random.default_rng(S)
    x = np.linspace(0.0, 30e3, S)
    for trial in range(40):
        ev = _random_events(rng, x, int(rng.integers(0, 12)))
        owner = bref.segments_by_slice_assignment(x, [x[0]] + list(ev), x[-1])
        j = bref.sample_index(x, ev)
        seg = np.array([np.sum(j <= s) for s in range(S)])
        seg[-1] = len(ev)
        # a sample no segment was given keeps the value an earlier, longer slice wrote: none here, every sample is owned
        assert (owner >= 0).all() and np.array_equal(owner, seg), (trial, ev)
        log = BounceLog(ev[None, :], np.zeros((1, len(ev))), np.ones((1, len(ev)), np.int8))
        nb, ns = log.counts(x, np.arange(S))
        assert np.array_equal(nb[0], seg) and not ns.any()


def test_event_loss_over_all_events_at_once_is_the_loss_one_event_at_a_time():
    """bounce_reference.event_loss (one call of the oracle's asin for the whole log) against the per-event form it restates,
    bit for bit: a range-dependent table over a sloping floor, both signs of p, both boundaries, tables with nodes inside
    (0, 90) and constants, empty slots, NaN bx / bp, |p c| = 1 and > 1, events outside the tables' ranges"""
    rng = np.random.default_rng(14)
    rin, zin = np.sort(rng.uniform(-40e3, 90e3, 9)), np.linspace(0.0, 5000.0, 41) ** 1.1
    cin = 1480.0 + 0.016 * zin[None, :] + 6.0 * np.sin(rin / 2e4)[:, None]
    br = np.sort(rng.uniform(-40e3, 90e3, 7))
    bd = 3000.0 + 400.0 * np.sin(br / 3e4)
    beta = (br, np.degrees(np.arctan(np.gradient(bd, br))))
    M, K = 37, 6
    bx = rng.uniform(-45e3, 95e3, (M, K))
    bp = np.sin(np.radians(rng.uniform(-89.0, 89.0, (M, K)))) / 1500.0
    bk = rng.integers(-1, 2, (M, K)).astype(np.int8)
    bp[3, 1], bx[5, 2], bp[7, 0], bp[8, 0] = np.nan, np.nan, 1.0 / 1400.0, -1.0 / 1400.0
    bk[[3, 5, 7, 8], [1, 2, 0, 0]] = [1, 0, 1, 0]
    c = bref.tlr.bilinear(bx[9, 0], 0.0, rin, zin, cin)
    bp[9, 0], bk[9, 0] = 1.0 / c, 0
    tables = [((np.array([2.0, 11.0, 35.0, 80.0]), np.array([0.5, 3.0, 1.0, 9.0])), (None, np.array([0.25])), beta),
              ((None, np.array([1.5])), (np.array([1.0, 30.0]), np.array([0.0, 2.0])), (None, np.zeros(1)))]
    for bottom, surface, slope in tables:
        for psign in (-1.0, 1.0):
            a = bref.event_loss(bx, bp, bk, cin, rin, zin, br, bd, bottom, surface, slope, psign)
            b = bref.event_loss_one_by_one(bx, bp, bk, cin, rin, zin, br, bd, bottom, surface, slope, psign)
            assert np.array_equal(a, b, equal_nan=True)
            assert np.isnan(a).sum() >= 3 and (a[bk < 0] == 0).all() and (a[~np.isnan(a)] > 0).sum() > 50


def _host_fan(M=5, S=9, K=4, backwards=False):
    x = np.linspace(40e3, 0.0, S) if backwards else np.linspace(0.0, 40e3, S)
    z = np.zeros((M, S))
    fan = RayFan.from_arrays(np.linspace(-5, 5, M), np.tile(x, (M, 1)), z + 1.0, z - 100.0, z, np.full(M, 2), np.full(M, 1),
                             np.full(M, 100.0))
    bx = np.full((M, K), np.nan); bp = np.full((M, K), np.nan); bk = np.full((M, K), -1, np.int8)
    xf = -x if backwards else x
    bx[:, 0], bx[:, 1], bx[:, 2] = xf[0] + 2e3, xf[0] + 17.5e3, xf[0] + 39e3
    bp[:, :3] = 1e-4
    bk[:, 0], bk[:, 1], bk[:, 2] = 1, 0, 1
    fan._bounces = BounceLog(bx, bp, bk)
    return fan


@pytest.mark.parametrize("backwards", [False, True])
def test_bounce_counts_of_a_host_fan(backwards):
    fan = _host_fan(backwards=backwards)
    assert np.array_equal(fan.bounces.count, np.full(5, 3)) and fan.bounces.capacity == 4
    nb, ns = fan.bounce_counts(np.arange(9))
    # save ranges every 5 km: 2 km is nearest to column 0, 17.5 km ties between 3 and 4 (the first: 3), 39 km belongs to the last
    assert np.array_equal(nb[0], [1, 1, 1, 1, 1, 1, 1, 1, 2]) and np.array_equal(ns[0], [0, 0, 0, 1, 1, 1, 1, 1, 1])
    nb, ns = fan.bounce_counts()
    assert nb.shape == (5, 1) and np.array_equal(nb[:, 0], fan.n_botts) and np.array_equal(ns[:, 0], fan.n_surfs)
    assert np.array_equal(fan.bounce_counts([-1, 0])[0], [[2, 1]] * 5)
    front = fan.time_front(3)
    assert front.ray_ids is not None and all(s.endswith("b") for s in front.ray_ids)
    assert np.array_equal(fan.time_front(-1).ray_ids, fan.ray_ids)


def test_the_log_survives_indexing_addition_and_pickling():
    fan = _host_fan()
    sub = fan[1:4]
    assert len(sub.bounces) == 3 and np.array_equal(sub.bounces.kind, fan.bounces.kind[1:4])
    assert np.array_equal(fan[np.array([True, False, True, False, False])].bounces.x, fan.bounces.x[[0, 2]], equal_nan=True)
    wide = _host_fan(K=6)
    both = fan + wide
    assert both.bounces.capacity == 6 and len(both.bounces) == 10 and np.array_equal(both.bounces.count, np.full(10, 3))
    assert (both.bounces.kind[:5, 4:] == -1).all() and np.isnan(both.bounces.x[:5, 4:]).all()
    back = pickle.loads(pickle.dumps(fan))
    assert np.array_equal(back.bounces.x, fan.bounces.x, equal_nan=True) and np.array_equal(back.bounces.kind, fan.bounces.kind)
    plain = RayFan.from_arrays(*(getattr(fan, k) for k in ("thetas", "rs", "ts", "zs", "ps", "n_botts", "n_surfs", "source_depths")))
    assert plain.bounces is None and (fan + plain).bounces is None and plain.time_front(3).ray_ids is None
    with pytest.raises(ValueError, match="max_bounces"):
        plain.bounce_counts()


def test_every_argument_error_of_the_python_layer():
    env = pr.OceanEnvironment2D()
    for bad in (0, -3, 2.5, True, "4"):
        with pytest.raises(ValueError, match="max_bounces"):
            pr.shoot_rays(1000.0, 0.0, np.linspace(-5, 5, 4), 10e3, 11, env, debug=False, max_bounces=bad)
    for bad in (-1.0, np.nan, np.inf, [1.0, 2.0], ([0.0, 10.0], [1.0]), ([10.0, 0.0], [1.0, 2.0]), ([0.0, 0.0], [1.0, 2.0]),
                ([0.0, np.nan], [1.0, 2.0]), ([0.0, 10.0], [1.0, -2.0]), ([], [])):
        with pytest.raises(ValueError):
            _loss_table(bad, "bottom_loss")
    assert _loss_table(None, "x")[0] is None and _loss_table(None, "x")[1][0] == 0.0
    g, v = _loss_table(([0.0, 45.0, 90.0], [0.0, 3.0, 10.0]), "x")
    assert list(g) == [0.0, 45.0, 90.0] and list(v) == [0.0, 3.0, 10.0]
    # a fan without a log is refused before any device work (no GPU here: anything else would fail differently)
    plain = _host_fan()
    plain._bounces = None
    d = np.array([100.0, 200.0])
    for call in (lambda: pr.boundary_loss(plain, env, bottom_loss=1.0, flatearth=True),
                 lambda: pr.transmission_loss(plain, d, env, bottom_loss=1.0),
                 lambda: pr.beam_transmission_loss(plain, d, env, surface_loss=([0.0, 90.0], [0.0, 1.0])),
                 lambda: pr.arrivals(plain, d, env, bottom_loss=0.0)):
        with pytest.raises(ValueError, match="bounce log"):
            call()
    with pytest.raises(ValueError):
        pr.transmission_loss(_host_fan(), d, env, bottom_loss=-1.0)
