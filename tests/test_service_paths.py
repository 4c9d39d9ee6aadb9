"""The paths through the fan kernel's bounce SERVICE phase (csrc/pgr_fan_kernel.h), one small fan each: the library against the
C oracle in its correctly rounded mode BIT FOR BIT, and against the same launch under PGR_EXACT_BISECTION (the true event at
every iterate of brentq instead of the replay).  Every case first checks, with the oracle alone, that its inputs produce the
events it names."""
import numpy as np
import pytest

import bounce_reference as bref
import oracle
from helpers import munk, munk_arrays, y0_for, assert_bit_parity

pytestmark = pytest.mark.gpu

KEYS_RAY = ("status", "n_steps", "n_rej", "n_bott", "n_surf")


@pytest.fixture(scope="module")
def lib():
    from pygenray_amd import _lib
    if _lib.ARITH != "reference":
        pytest.skip("bit parity is claimed for the reference arithmetic only (PGR_ARITH=contracted: tests/test_contracted_arith.py)")
    _lib.load()
    assert _lib.device_count() >= 1
    return _lib


def same_launch(a, b, label):
    for k in ("T", "z", "p", "end"):
        assert np.array_equal(a[k], b[k], equal_nan=True), (label, k)
    for k in KEYS_RAY:
        assert np.array_equal(a[k], b[k]), (label, k)


def end_state_parity(g, o, label):
    """an end-state-only launch (no trajectories) against the oracle: status, counts, steps and the final state"""
    assert np.array_equal(g["status"], o["status"]), label
    ok = o["status"] == 0
    for k in ("n_bott", "n_surf", "n_steps", "n_rej"):
        assert np.array_equal(g[k][ok].astype(np.int64), o[k][ok].astype(np.int64)), (label, k)
    end = np.stack([o["T"][:, -1], o["z"][:, -1], o["p"][:, -1]], 1)
    assert np.array_equal(g["end"][ok], end[ok]), label
    assert np.all(np.isnan(g["end"][~ok]))


def service_case(lib, arrs, y0, x0, x1, S, label, end_state_too=False, **kw):
    """default locator == exact bisection == oracle, with trajectories (S samples, SciPy's sample order) and, where asked,
    as an end-state-only launch (S = 0: another kernel instance, the same service)"""
    env = lib.EnvHandle(*arrs)
    o = oracle.shoot_fan(*arrs, y0, x0, x1, S, math=oracle.MATH_CR, **kw)
    a = env.shoot_fan(y0, x0, x1, S, exact_samples=True, **kw)
    b = env.shoot_fan(y0, x0, x1, S, exact_samples=True, exact_bisection=True, **kw)
    same_launch(a, b, label + ": default locator vs exact bisection")
    assert_bit_parity(a, o, label=label)
    if end_state_too:
        for exact in (False, True):
            e = env.shoot_fan(y0, x0, x1, 2, save=False, exact_bisection=exact, **kw)
            end_state_parity(e, o, label + f": end state only, exact bisection {exact}")
    return env, a, o


def bounced_steps(arrs, y0, x0, x1, **kw):
    """from the oracle's step trace of one ray: (t, h, y[3], f[3]) of every accepted attempt that a bounce truncated, and the
    number of accepted attempts of every segment"""
    rows = oracle.trace_ray(*arrs, y0, x0, x1, math=oracle.MATH_CR, max_rows=400000, **kw)
    seg = rows[:, 11].astype(int)
    last = np.flatnonzero(np.diff(seg) > 0)
    per_segment = np.bincount(seg[rows[:, 9] == 1], minlength=seg.max() + 1)
    return rows[last], per_segment


STEEP = np.concatenate([np.linspace(-20.0, -14.0, 64), np.linspace(14.0, 20.0, 64)])


def test_steep_rays_on_the_munk_profile_with_and_without_trajectories(lib):
    """+-14 ... +-20 degrees over 100 km: several surface and bottom bounces per ray; S = 33 and S = 0.  A surface bounce's
    step ends above zin[0] - 1e-6 as well (the bounding box is active with the surface: active == 9): seen in the oracle's
    trace -- the truncated attempt, continued to its end, lies metres above the surface.  A 1-ray wave gives the bits the
    same ray has in the 64-ray wave."""
    arrs = munk_arrays(100e3, bathy=3500.0)
    y0 = y0_for(oracle, arrs, 300.0, 0.0, STEEP)
    env, a, o = service_case(lib, arrs, y0, 0.0, 100e3, 33, "steep Munk rays", end_state_too=True)
    assert o["n_bott"].min() >= 2 and o["n_surf"].min() >= 2 and np.all(o["status"] == 0)
    both = 0
    for k in (0, 63, 64, 127):
        st, _ = bounced_steps(arrs, y0[k], 0.0, 100e3)
        surf = st[st[:, 3] < 100.0]
        # (a step of h <= 200 m bends by less than 0.3 m: its end is the straight continuation to within that)
        short = surf[surf[:, 1] <= 200.0]
        both += int(np.sum(short[:, 3] + short[:, 1] * short[:, 6] < -1.0))
    assert both >= 4
    for k in (0, 17, 63):
        one = env.shoot_fan(y0[k:k + 1], 0.0, 100e3, 33, exact_samples=True)
        for key in ("T", "z", "p", "end") + KEYS_RAY:
            assert np.array_equal(one[key][0], a[key][k], equal_nan=True), (k, key)
    env.close()


def test_sloping_non_uniform_bathymetry(lib):
    """the bottom event goes through bathy(x) on an irregular range grid, the reflection through the bottom angle's cubic;
    range-dependent sound speed (tables in HBM)"""
    rng = np.random.default_rng(11)
    z = np.arange(0, 5500, 2.0)
    r = np.linspace(0, 150e3, 61)
    cin = np.array([munk(z, 1300 + 2e-3 * ri) for ri in r])
    br = np.sort(np.concatenate([[0.0, 150e3], rng.uniform(0, 150e3, 38)]))
    depths = 4800 + 300 * np.sin(br / 20e3)
    arrs = [cin, np.gradient(cin, z, axis=1, edge_order=1), r, z, depths, br, np.degrees(np.arctan(np.gradient(depths, br)))]
    assert np.ptp(np.diff(br)) > 1e3
    y0 = y0_for(oracle, arrs, 700.0, 0.0, np.linspace(-18, 18, 130))
    env, a, o = service_case(lib, arrs, y0, 0.0, 140e3, 31, "sloping non-uniform bathymetry", end_state_too=True)
    assert o["n_bott"].max() >= 3 and (o["n_bott"] > 0).sum() > 40
    env.close()


def test_second_bounce_inside_the_first_step_after_a_restart(lib):
    """a 5 mm layer: the restarted integrator's first step (3.5 cm) already reaches the other boundary -- segments of ONE
    accepted step in the oracle's trace"""
    z = np.arange(0, 64, 0.25)
    r = np.linspace(0, 30e3, 16)
    cin = np.tile(1500 + 0.05 * z, (16, 1))
    arrs = [cin, np.gradient(cin, z, axis=1, edge_order=1), r, z, np.full(16, 0.005), r.copy(), np.zeros(16)]
    th = np.concatenate([np.linspace(8.0, 19.0, 32), -np.linspace(8.0, 19.0, 32)])
    y0 = y0_for(oracle, arrs, 0.0025, 0.0, th)
    singles = 0
    for k in (0, 31, 32, 63):
        _, per_segment = bounced_steps(arrs, y0[k], 0.0, 3.0)
        singles += int(np.sum(per_segment[1:-1] == 1))
    assert singles >= 50
    env, a, o = service_case(lib, arrs, y0, 0.0, 3.0, 7, "second bounce in the first step", end_state_too=True)
    assert np.all(o["status"] == 0) and (o["n_bott"] + o["n_surf"]).min() >= 20
    env.close()


def test_a_ray_dropped_as_vertical(lib):
    """launched within 1e-3 degrees of the vertical the `vertical` event is set at the start and clears as the ray refracts:
    located by the exact bisection (not a surface or bottom event), the ray is dropped -- beside steep rays that go on"""
    arrs = munk_arrays(30e3, nr=12)
    th = np.concatenate([[89.9995, -89.9995, 89.999, -89.999, 89.9999, -89.9999], np.linspace(-20, 20, 58)])
    y0 = y0_for(oracle, arrs, 3000.0, 0.0, th)
    env, a, o = service_case(lib, arrs, y0, 0.0, 100.0, 5, "vertical rays", end_state_too=True)
    assert np.all(o["status"][:6] == 1) and np.all(o["status"][6:] == 0)
    assert np.all(np.isnan(a["z"][:6])) and np.all(a["status"][:6] == 1)
    env.close()


def test_lanes_of_one_packet_with_very_different_halving_counts(lib):
    """a source half a metre under the surface, +-20 degrees, 150 km: the upward rays' first bounce comes in the launch's
    third step, 0.4 -> 3.9 m (t_new > 2 t: no halving can be taken by position), the later ones at steps of 40 m ... 2.4 km
    tens of km out (37 ... 47 halvings) -- lanes of one 64-ray packet"""
    arrs = munk_arrays(150e3, nr=31)
    th = np.linspace(-20, 20, 64)
    y0 = y0_for(oracle, arrs, 0.5, 0.0, th)
    counts = []
    for k in (0, 5, 20, 58, 63):
        st, _ = bounced_steps(arrs, y0[k], 0.0, 150e3)
        t, h = st[:, 0], st[:, 1]
        dmax = (4 * 2.220446049250313e-16 + 4 * 2.220446049250313e-16 * np.maximum(np.abs(t), np.abs(t + h))) / 2
        n1 = np.floor(np.log2(h)) - np.floor(np.log2(dmax)) - 3
        counts.append(np.where((t > 0) & (t + h <= 2 * t), np.clip(n1, 0, 90), 0))
    counts = np.concatenate(counts)
    assert counts.min() == 0 and counts.max() >= 40 and len(np.unique(counts)) >= 6
    env, a, o = service_case(lib, arrs, y0, 0.0, 150e3, 33, "mixed halving counts", end_state_too=True)
    assert (o["n_bott"] + o["n_surf"] > 0).sum() >= 30
    # the same rays in packets of other shapes: one wave of 64, and 16 + 48
    for sl in (slice(0, 16), slice(16, 64)):
        part = env.shoot_fan(y0[sl], 0.0, 150e3, 33, exact_samples=True)
        for key in ("T", "z", "p", "end") + KEYS_RAY:
            assert np.array_equal(part[key], a[key][sl], equal_nan=True), key
    env.close()


def test_flat_earth_table_with_trajectories_replays_the_stages(lib):
    """the reference's default environment after the flat-earth transform (cubic depth index, ZM = 5): with trajectories its
    service replays the parked attempt's stages instead of keeping them"""
    import pygenray_amd as pr
    arrs = pr._unpack_envi(pr.OceanEnvironment2D(), flatearth=True)
    y0 = y0_for(oracle, arrs, 1000.0, 0.0, STEEP)
    env, a, o = service_case(lib, arrs, y0, 0.0, 100e3, 33, "flat-earth table", end_state_too=True)
    env.shoot_fan(y0, 0.0, 100e3, 33, exact_samples=True)
    li = env.last_instance()
    assert (li["lds_tab"], li["zm"]) == (1, 5) and li["save"] != 0
    assert (o["n_bott"] > 0).sum() > 100 and (o["n_surf"] > 0).sum() > 100
    env.close()


def _range_dependent_arrays():
    z = np.arange(0, 6000, 1.0)
    r = np.linspace(0.0, 60e3, 9)
    cin = np.array([munk(z, 1300.0 + 4e-3 * ri) for ri in r])
    return [cin, np.gradient(cin, z, axis=1, edge_order=1), r, z, np.full(9, 4800.0), r.copy(), np.zeros(9)]


def test_range_dependent_table_in_the_blocked_layout(lib):
    """tables in HBM, samples staged per lane and written [S/4][N][4] (what the sample-major API gets): the re-sample after a
    bounce goes through the service"""
    arrs = _range_dependent_arrays()
    y0 = y0_for(oracle, arrs, 900.0, 0.0, STEEP)
    env = lib.EnvHandle(*arrs)
    o = oracle.shoot_fan(*arrs, y0, 0.0, 50e3, 34, math=oracle.MATH_CR)
    assert (o["n_bott"] + o["n_surf"]).min() >= 1 and (o["n_bott"] + o["n_surf"]).max() >= 3
    a = env.shoot_fan(y0, 0.0, 50e3, 34, sample_major=True)
    li = env.last_instance()
    assert (li["lds_tab"], li["save"]) == (0, 3)
    b = env.shoot_fan(y0, 0.0, 50e3, 34, sample_major=True, exact_bisection=True)
    same_launch(a, b, "blocked layout: default locator vs exact bisection")
    g = dict(a, T=a["T"].T, z=a["z"].T, p=a["p"].T)
    assert_bit_parity(g, o, label="blocked layout", samples=False)
    env.close()


def test_bounce_log_of_a_logged_launch_equals_the_oracle_trace(lib):
    """max_bounces: the LOG instances run the same service and write each bounce's range, reflected slowness and kind"""
    arrs = _range_dependent_arrays()
    arrs[0] = np.tile(arrs[0][:1], (9, 1)); arrs[1] = np.tile(arrs[1][:1], (9, 1))     # one profile: the LDS table
    th = STEEP[::2]
    y0 = y0_for(oracle, arrs, 900.0, 0.0, th)
    K = 16
    env = lib.EnvHandle(*arrs)
    plain = lib.FanHandle(env, 0.0, 60e3, 13, y0=y0)
    ref = plain.fetch_rays(); ref.update(plain.fetch_samples(compact=False)); plain.close()
    for exact in (False, True):
        logged = lib.FanHandle(env, 0.0, 60e3, 13, y0=y0, max_bounces=K, exact_bisection=exact)
        got = logged.fetch_rays(); got.update(logged.fetch_samples(compact=False))
        assert env.last_instance_log() == 1
        bx, bp, bk = (v.T for v in logged.fetch_bounces())
        logged.close()
        for k in ref:
            assert np.array_equal(ref[k], got[k], equal_nan=True), k
        assert np.all(ref["status"] == 0)
        total = ref["n_bott"] + ref["n_surf"]
        assert (total >= 2).sum() > 40 and total.max() <= K
        for i in range(len(th)):
            x, p, kind = bref.trace_bounces(arrs, y0[i], 0.0, 60e3)
            m = len(x)
            assert m == total[i]
            assert np.array_equal(bx[i, :m], x) and np.array_equal(bp[i, :m], p) and np.array_equal(bk[i, :m], kind)
            assert np.all(bk[i, m:] == -1)
    env.close()
