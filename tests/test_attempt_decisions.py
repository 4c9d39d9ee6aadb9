"""The decisions of a step attempt's tail (csrc/pgr_fan_kernel.h: accept / reject and the step factor, the counters, the status at
t_bound, the events' wave-uniform test, the sample passes, the gate), which travel as masks in vector registers: small fans
against the C oracle in its correctly rounded mode BIT FOR BIT -- T, z, p rows, end state, n_steps, n_rej, n_bott, n_surf,
status -- on the LDS-table ZM = 4 instance and on an HBM-table instance, each with trajectories (SciPy's sample order, the
default stage-major form) and without.  The rays are chosen so that one wave holds both sides of every decision; each case first
checks, with the oracle alone, that every class it names occurred."""
import numpy as np
import pytest

import oracle
from helpers import munk, y0_for, assert_bit_parity

pytestmark = pytest.mark.gpu

X1 = 100e3
S = 65
RTOLS = (1e-3, 1e-9, 1e-12)


@pytest.fixture(scope="module")
def lib():
    from pygenray_amd import _lib
    if _lib.ARITH != "reference":
        pytest.skip("bit parity is claimed for the reference arithmetic only (PGR_ARITH=contracted: tests/test_contracted_arith.py)")
    _lib.load()
    assert _lib.device_count() >= 1
    return _lib


def mixed_env(range_dependent):
    """Munk profile on zin = j * 1 m (ZM = 4), range-independent (96 KB: the LDS-table instance) or with a sloping axis (tables in
    HBM).  The floor is at 3500 m out to 60 km and then falls through the bottom of the table (rays that follow it leave the
    bounding box); between 18 and 24 km the bottom ANGLE is 60 degrees (rays that bounce there turn backwards)."""
    z = np.arange(0, 6000, 1.0)
    r = np.linspace(0.0, X1, 101)
    cin = np.array([munk(z, 1300 + (2e-3 * ri if range_dependent else 0.0)) for ri in r])
    br = r.copy()
    depths = np.where(br <= 60e3, 3500.0, np.minimum(3500.0 + (br - 60e3) * 0.5, 7000.0))
    ba = np.zeros_like(br)
    ba[(br >= 18e3) & (br <= 24e3)] = 60.0
    return [cin, np.gradient(cin, z, axis=1, edge_order=1), r, z, depths, br, ba]


def mixed_rays(arrs):
    """128 rays, two waves.  Wave 0: quiet rays and rays that hit the surface and the bottom, shuffled.  Wave 1: sources at
    z = 0 and on the sea floor, launches within 1e-3 degrees of the vertical (dropped at once), steep launches that bounce
    hundreds of times, and four rays near the axis."""
    w0 = np.concatenate([np.linspace(-8, 8, 24), np.linspace(-20, -13, 20), np.linspace(13, 20, 20)])
    np.random.default_rng(3).shuffle(w0)
    th1 = np.linspace(-18, 18, 24)
    th_v = np.array([89.9995, -89.9995, 89.9999, -89.9999, 85.0, -85.0, 60.0, -60.0, 75.0, -75.0, 80.0, -80.0])
    return np.concatenate([y0_for(oracle, arrs, 1000.0, 0.0, w0), y0_for(oracle, arrs, 0.0, 0.0, th1),
                           y0_for(oracle, arrs, 3500.0, 0.0, th1), y0_for(oracle, arrs, 1000.0, 0.0, th_v),
                           y0_for(oracle, arrs, 1300.0, 0.0, np.array([0.0, 1.0, -1.0, 5.0]))])


_CASES = {}


def case(range_dependent, rtol):
    """inputs and the oracle's fan, computed once per (environment, rtol) and shared by the tests below"""
    key = (range_dependent, rtol)
    if key not in _CASES:
        arrs = mixed_env(range_dependent)
        y0 = mixed_rays(arrs)
        assert len(y0) == 128
        o = oracle.shoot_fan(*arrs, y0, 0.0, X1, S, rtol=rtol, math=oracle.MATH_CR)
        # every class on both sides, in ONE wave where the decision is per wave: the oracle's own counters say so
        st = o["status"]
        assert (o["n_rej"] > 0).any() and (o["n_steps"] > 0).all()
        for w in (slice(0, 64), slice(64, 128)):
            bounces = (o["n_bott"] + o["n_surf"])[w]
            assert (bounces == 0).sum() >= 4 and (o["n_bott"][w] > 0).sum() >= 8 and (o["n_surf"][w] > 0).sum() >= 8, key
            assert (st[w] == 0).sum() >= 16 and (st[w] != 0).sum() >= 8, key
        assert (st == 1).sum() >= 4 and (st == 2).sum() >= 8 and (st == 3).sum() >= 4, np.bincount(st, minlength=4)   # vertical, bbox, backward
        assert (st[64:88] == 0).any() and (st[88:112] == 0).any()        # sources at z = 0 and on the sea floor that arrive
        _CASES[key] = (arrs, y0, o)
    return _CASES[key]


def end_state_parity(g, o, label):
    assert np.array_equal(g["status"], o["status"]), label
    ok = o["status"] == 0
    for k in ("n_bott", "n_surf", "n_steps", "n_rej"):
        assert np.array_equal(g[k][ok].astype(np.int64), o[k][ok].astype(np.int64)), (label, k)
    end = np.stack([o["T"][:, -1], o["z"][:, -1], o["p"][:, -1]], 1)
    assert np.array_equal(g["end"][ok], end[ok]), label
    assert np.all(np.isnan(g["end"][~ok]))


@pytest.mark.parametrize("rtol", RTOLS)
@pytest.mark.parametrize("range_dependent", (False, True), ids=("lds_table", "hbm_table"))
def test_mixed_waves_bit_for_bit(lib, range_dependent, rtol):
    arrs, y0, o = case(range_dependent, rtol)
    env = lib.EnvHandle(*arrs)
    assert bool(env.lds_path) == (not range_dependent) and env.query(1) == 1 and env.query(5) == 0

    def ran(save):   # the instance the LAST launch selected: LDS or HBM table, ZM = 4 (dz = 1), the SAVE meant
        li = env.last_instance()
        assert (li["lds_tab"], li["zm"]) == (0 if range_dependent else 1, 4) and li["save"] in save and li["persist"] == 0, li
    label = f"{'HBM' if range_dependent else 'LDS'} table, rtol {rtol:g}"
    a = env.shoot_fan(y0, 0.0, X1, S, rtol=rtol, exact_samples=True)              # every sample in SciPy's order: all bits
    ran((2,))
    assert_bit_parity(a, o, label=label + ", SciPy-order samples")
    d = env.shoot_fan(y0, 0.0, X1, S, rtol=rtol)                                  # the stage-major sample pass
    ran((1,))
    assert_bit_parity(d, o, label=label + ", default samples", samples=False)
    m = env.shoot_fan(y0, 0.0, X1, S, rtol=rtol, sample_major=True)               # ... as the benchmark stores them
    ran((1, 3))                                                                   # (3: sample-blocked, HBM tables)
    for k in "Tzp":
        assert np.array_equal(m[k].T, d[k], equal_nan=True), (label, k)
    e = env.shoot_fan(y0, 0.0, X1, 2, rtol=rtol, save=False)                      # no trajectories: another instance
    ran((0,))
    end_state_parity(e, o, label + ", end state only")
    for k in ("n_steps", "n_rej", "n_bott", "n_surf", "status"):
        assert np.array_equal(a[k], e[k]) and np.array_equal(d[k], e[k]), (label, k)
    env.close()


def test_factor_limits_are_reached_on_both_sides():
    """The inputs reach both limits of the step factor and the limit 1 behind a rejection -- from the oracle's traces (rows: t, h,
    y, f, error_norm, accepted, h_abs after the attempt).  rtol = 1e-3: attempts accepted with 0.9 err^-0.2 above MAX_FACTOR
    (h grows by exactly 10) and rejected below MIN_FACTOR (h shrinks by exactly 0.2); rtol = 1e-12: every ray is rejected at
    least once, and a step accepted behind a rejection never grows."""
    arrs, y0, o = case(False, 1e-3)
    grown = shrunk = 0
    for k in range(32):
        rows = oracle.trace_ray(*arrs, y0[k], 0.0, X1, rtol=1e-3, math=oracle.MATH_CR)
        acc = rows[:, 9] == 1
        grown += int(np.sum(acc & (rows[:, 8] < 0.09 ** 5) & (rows[:, 10] == 10 * np.abs(rows[:, 1]))))
        shrunk += int(np.sum(~acc & (rows[:, 10] == 0.2 * np.abs(rows[:, 1]))))
    assert grown >= 32 and shrunk >= 8, (grown, shrunk)
    arrs, y0, o = case(False, 1e-12)
    assert o["n_rej"].min() >= 1 and o["n_rej"].sum() >= 2000
    behind = 0
    for k in range(0, 128, 8):
        rows = oracle.trace_ray(*arrs, y0[k], 0.0, X1, rtol=1e-12, math=oracle.MATH_CR)
        acc = rows[:, 9] == 1
        after_rej = np.flatnonzero(~acc[:-1] & acc[1:]) + 1                                          # accepted behind a rejection
        assert np.all(rows[after_rej, 10] <= np.abs(rows[after_rej, 1]))                             # ... never grows
        behind += len(after_rej)
    assert behind >= 100, behind


@pytest.mark.parametrize("range_dependent", (False, True), ids=("lds_table", "hbm_table"))
def test_last_step_lands_exactly_on_the_receiver_range(lib, range_dependent):
    """The receiver range is t + h of one of a quiet ray's own steps: its last step is NOT clamped and t_new - t_bound is +0
    (every other ray's last step is clamped onto it)."""
    arrs, y0, _ = case(range_dependent, 1e-9)
    k = int(np.argmin(np.abs(y0[:64, 2])))                                      # the flattest ray of wave 0
    rows = oracle.trace_ray(*arrs, y0[k], 0.0, X1, math=oracle.MATH_CR)
    acc = np.flatnonzero(rows[:, 9] == 1)
    j = acc[np.searchsorted(rows[acc, 0], 70e3)]
    x1 = float(rows[j, 0] + rows[j, 1])
    rows1 = oracle.trace_ray(*arrs, y0[k], 0.0, x1, math=oracle.MATH_CR)
    last = rows1[np.flatnonzero(rows1[:, 9] == 1)[-1]]
    assert last[0] + last[1] == x1 and last[1] == rows[j, 1] and last[0] == rows[j, 0]               # the same, unclamped step
    o = oracle.shoot_fan(*arrs, y0, 0.0, x1, 33, math=oracle.MATH_CR)
    assert o["status"][k] == 0
    env = lib.EnvHandle(*arrs)
    a = env.shoot_fan(y0, 0.0, x1, 33, exact_samples=True)
    assert_bit_parity(a, o, label="exact landing")
    end_state_parity(env.shoot_fan(y0, 0.0, x1, 2, save=False), o, "exact landing, end state only")
    env.close()


@pytest.mark.parametrize("range_dependent", (False, True), ids=("lds_table", "hbm_table"))
def test_nan_initial_slowness_is_skipped_and_its_wave_unchanged(lib, range_dependent):
    """PGR_SKIP_NAN_Y0: one ray of each wave has a NaN slowness -- status PGR_RAY_SKIPPED, no attempt made, and every other ray
    of its wave as in the fan without it; with trajectories and as an end-state-only fan."""
    arrs, y0, o = case(range_dependent, 1e-9)
    y = y0.copy()
    nan_rays = [5, 64 + 17]
    y[nan_rays, 2] = np.nan
    keep = np.ones(len(y), bool)
    keep[nan_rays] = False
    ok = keep & (o["status"] == 0)
    env = lib.EnvHandle(*arrs)
    for samples in (S, 0):
        fan = lib.FanHandle(env, 0.0, X1, samples, y0=y, skip_nan=True, exact_samples=True)
        g = fan.fetch_rays()
        smp = fan.fetch_samples(compact=False) if samples else None
        fan.close()
        li = env.last_instance()
        assert (li["lds_tab"], li["zm"]) == (0 if range_dependent else 1, 4) and (li["save"] != 0) == (samples != 0), li
        assert np.all(g["status"][nan_rays] == 8) and np.all(g["n_steps"][nan_rays] == 0) and np.all(g["n_rej"][nan_rays] == 0)
        assert np.array_equal(g["status"][keep], o["status"][keep])
        for k in ("n_steps", "n_rej", "n_bott", "n_surf"):
            assert np.array_equal(g[k][ok].astype(np.int64), o[k][ok].astype(np.int64)), (samples, k)
        assert np.array_equal(g["end"][ok], np.stack([o["T"][ok, -1], o["z"][ok, -1], o["p"][ok, -1]], 1)), samples
        if samples:
            for k in "Tzp":
                assert np.array_equal(smp[k].T[ok], o[k][ok]), k
                assert np.all(np.isnan(smp[k].T[~ok]))
    env.close()
