"""Caustic index and coherent ray-tube pressure without a GPU: the NumPy restatement (tests/coherent_reference.py) against
closed forms on the CPU oracle's fans -- the focusing medium, folds at a boundary, Lloyd's mirror -- the library's
cos(2 pi t) / sin(2 pi t) against mpmath, and the argument errors refused before anything reaches the device."""
import inspect

import numpy as np
import pytest

import pygenray_amd as pr

import bounce_reference as bref
import coherent_reference as cref
from helpers import y0_for


# ---- the caustic index ------------------------------------------------------------------------------------------------------

def test_focusing_medium_every_tube_counts_the_foci_it_has_passed():
    import oracle
    arrs = pr._unpack_envi(cref.focus_env(pr), flatearth=False)
    y0 = y0_for(oracle, arrs, cref.FOCUS_Z0, 0.0, -cref.focus_angles())
    o = oracle.shoot_fan(*arrs, y0, 0.0, cref.FOCUS_X1, cref.FOCUS_S, math=oracle.MATH_CR)
    kappa = cref.caustic_index(o["z"])
    cref.check_focus_fan(o["r"], -o["z"], kappa, o["status"], o["n_bott"], o["n_surf"])
    # the depths' sign does not matter (every width changes sign), nor do counts that are the same for every ray
    assert np.array_equal(cref.caustic_index(-o["z"]), kappa)
    ones = np.ones(o["z"].shape, np.int32)
    assert np.array_equal(cref.caustic_index(o["z"], ones, 2 * ones), kappa)


def folded_fan(M=40, S=61):
    """straight rays of an isovelocity source at 100 m, launched upwards at 2.5 ... 12 degrees and folded at the surface:
    depths d (M, S), surface counts ns (M, S), x (S,)"""
    x = np.linspace(0.0, 3e3, S)
    rise = np.outer(np.tan(np.radians(np.linspace(2.5, 12.0, M))), x)
    return np.abs(100.0 - rise), (rise > 100.0).astype(np.int32), x


def test_a_reflection_is_not_a_caustic_and_a_straddling_tube_carries_its_sign():
    d, ns, x = folded_fan()
    nb = np.zeros_like(ns)
    straddle = ns[:-1] != ns[1:]
    assert straddle.any(axis=1).sum() > 10 and (ns[:, -1] == 1).all() and (ns[:, 0] == 0).all()   # every tube folds, then unfolds
    assert (cref.caustic_index(d, nb, ns) == 0).all()
    # the test's power: without the counts every tube's width changes sign at the fold ...
    plain = cref.caustic_index(d)
    assert (plain[:, -1] == 1).all() and (plain[:, 0] == 0).all()
    # ... and with a straddling sample counted instead of skipped the fold would count (the raw width there has either sign)
    raw = np.sign(d[1:] - d[:-1])
    assert (raw[straddle] > 0).any() and (raw[straddle] < 0).any()
    # bottom bounces flip alike, and both kinds together flip twice
    assert (cref.caustic_index(d, ns, nb) == 0).all()
    assert (cref.caustic_index(d, ns, ns)[:, -1] == 1).all()


def test_hand_made_tubes():
    nan = np.nan
    # widths + + - -: one caustic between columns 2 and 3; column 0 (equal depths) never counts
    d = np.array([[5.0, 1.0, 2.0, 3.0, 4.0],
                  [5.0, 2.0, 2.5, 2.9, 3.5]])
    assert cref.caustic_index(d).tolist() == [[0, 0, 0, 1, 1]]
    # the sign is carried across NaN samples and equal depths: + nan = - : counted once, where the width is next known
    d = np.array([[5.0, 1.0, nan, 3.0, 3.0, 4.0],
                  [5.0, 2.0, 2.5, nan, 3.0, 3.5]])
    assert cref.caustic_index(d).tolist() == [[0, 0, 0, 0, 0, 1]]
    # a fold with the straddling column skipped: raw widths + - - with counts 0|0, 0|1, 1|1 -> u = + (skipped) + : no caustic;
    # then a real one after the bounce: raw + with counts 1|1 -> u = -
    d = np.array([[5.0, 1.0, 0.5, 2.0, 3.0],
                  [5.0, 2.0, 0.2, 1.0, 3.5]])
    ns = np.array([[0, 0, 0, 1, 1],
                   [0, 0, 1, 1, 1]])
    assert cref.caustic_index(d, np.zeros_like(ns), ns).tolist() == [[0, 0, 0, 0, 1]]
    # three rays: the tubes are independent
    d = np.array([[0.0, 1.0, 3.0], [0.0, 2.0, 2.0], [0.0, 3.0, 1.0]])
    assert cref.caustic_index(d).tolist() == [[0, 0, 1], [0, 0, 1]]
    # q of pressure_field: kappa + 2 ns of the tube's first ray, -1 where the counts differ, 0 in the last row
    kappa = cref.caustic_index(np.array([[5.0, 1.0, 0.5, 2.0, 3.0], [5.0, 2.0, 0.2, 1.0, 3.5]]), np.zeros_like(ns), ns)
    assert cref.tube_phase(kappa, np.zeros_like(ns), ns).tolist() == [[0, 0, -1, 2, 3], [0, 0, 0, 0, 0]]
    assert cref.tube_phase(kappa, None, None).tolist() == [[0, 0, 0, 0, 1], [0, 0, 0, 0, 0]]


# ---- cos(2 pi t), sin(2 pi t) -----------------------------------------------------------------------------------------------

def trig_points():
    rng = np.random.default_rng(7)
    seams = np.array([0.0, 0.125, 0.25, 0.375, 0.5])
    near = np.concatenate([seams, np.nextafter(seams, 1.0), np.nextafter(seams, -1.0)])
    t = np.concatenate([rng.uniform(-0.5, 0.5, 24000), near, -near, 10.0 ** -rng.uniform(0.0, 300.0, 500)])
    return t[(t >= -0.5) & (t <= 0.5)]


def test_gcos2pi_and_gsin2pi_are_within_two_ulp_of_one_of_the_functions():
    import mpmath
    mpmath.mp.dps = 40
    t = trig_points()
    assert len(t) >= 20000 and {-0.5, 0.5, 0.125, -0.125, 0.25, -0.25, 0.375, -0.375, 0.0} <= set(t.tolist())
    c, s = cref.gcos2pi(t), cref.gsin2pi(t)
    worst_c = worst_s = 0.0
    for a, cv, sv in zip(t, c, s):
        x = 2 * mpmath.pi * mpmath.mpf(float(a))
        worst_c = max(worst_c, abs(float(mpmath.mpf(float(cv)) - mpmath.cos(x))))
        worst_s = max(worst_s, abs(float(mpmath.mpf(float(sv)) - mpmath.sin(x))))
    print(f"gcos2pi / gsin2pi on [-0.5, 0.5]: worst absolute error {worst_c:.3e} / {worst_s:.3e} over {len(t)} points "
          f"(bound {cref.TRIG_BOUND:.3e})")
    assert max(worst_c, worst_s) <= cref.TRIG_BOUND
    assert max(worst_c, worst_s) <= cref.TRIG_MEASURED <= cref.TRIG_BOUND          # the value DESIGN.md records
    # exact values at the seams, and NaN for a NaN
    assert cref.gcos2pi(np.array([0.0, 0.25, -0.25, 0.5, -0.5])).tolist() == [1.0, 0.0, 0.0, -1.0, -1.0]
    assert cref.gsin2pi(np.array([0.0, 0.25, -0.25, 0.5, -0.5])).tolist() == [0.0, 1.0, -1.0, 0.0, 0.0]
    assert np.isnan(cref.gcos2pi(np.nan)) and np.isnan(cref.gsin2pi(np.nan))
    # the phase reduction lands in [-0.5, 0.5] for every q, also for times that make f T large
    T = np.random.default_rng(1).uniform(0.0, 700.0, 4000)
    for q in (0, 1, 2, 3, 5, 1 << 20):
        ph = cref.phase_cycles(T, np.full(len(T), q), 4321.0)
        assert (np.abs(ph) <= 0.5).all()
    assert cref.phase_cycles(np.array([0.25]), np.array([5]), 1.0)[0] == 0.0       # q = 5 is q = 1: a quarter cycle


HOST_MAIN = """
#include <cstdio>
#define __device__
#define __forceinline__ inline
#include "pgr_trig.h"
int main() { double t; while (std::scanf("%la", &t) == 1) std::printf("%a %a\\n", gcos2pi(t), gsin2pi(t)); return 0; }
"""


def test_the_library_s_own_c_source_of_both_functions_equals_the_restatement_bit_for_bit(tmp_path):
    """csrc/pgr_trig.h, the source the kernels are built from, compiled for the host without contraction"""
    import os
    import shutil
    import subprocess
    from pygenray_amd import _lib
    cxx = shutil.which("g++") or shutil.which("c++") or shutil.which("clang++")
    assert cxx, "no host C++ compiler"
    (tmp_path / "main.cpp").write_text(HOST_MAIN)
    exe = str(tmp_path / "trig_host")
    subprocess.run([cxx, "-O2", "-ffp-contract=off", "-I", _lib.CSRC, "-o", exe, str(tmp_path / "main.cpp")], check=True)
    t = np.concatenate([trig_points(), [np.nan]])
    out = subprocess.run([exe], input="\n".join(float(v).hex() for v in t), capture_output=True, text=True, check=True).stdout
    val = lambda w: np.nan if "nan" in w else float.fromhex(w)   # noqa: E731
    got = np.array([[val(w) for w in line.split()] for line in out.splitlines()])
    assert got.shape == (len(t), 2) and os.path.exists(os.path.join(_lib.CSRC, "pgr_trig.h"))
    assert np.array_equal(got[:, 0], cref.gcos2pi(t), equal_nan=True) and np.array_equal(got[:, 1], cref.gsin2pi(t), equal_nan=True)


# ---- Lloyd's mirror ---------------------------------------------------------------------------------------------------------

@pytest.fixture(scope="module")
def lloyd():
    """the CPU oracle's fan of coherent_reference's Lloyd set-up as a host RayFan, its environment and the per-sample counts
    from the oracle's own bounces"""
    import oracle
    env = cref.lloyd_env(pr)
    arrs = pr._unpack_envi(env, flatearth=False)
    th = cref.lloyd_angles()
    y0 = y0_for(oracle, arrs, cref.LLOYD_ZS, 0.0, -th)
    o = oracle.shoot_fan(*arrs, y0, 0.0, cref.LLOYD_X1, cref.LLOYD_S, math=oracle.MATH_CR)
    assert (o["status"] == 0).all() and (o["n_bott"] == 0).all() and o["n_surf"].max() == 1      # no ray reaches the bottom
    M, K = len(th), 4
    bx, bk = np.full((M, K), np.nan), np.full((M, K), -1, np.int8)
    for i in np.flatnonzero(o["n_surf"] > 0):
        x, _, kind = bref.trace_bounces(arrs, y0[i], 0.0, cref.LLOYD_X1)
        assert len(x) == 1 and kind[0] == 0
        bx[i, 0], bk[i, 0] = x[0], 0
    nb, ns = cref.log_counts(bx, bk, o["r"])
    assert np.array_equal(ns[:, -1], o["n_surf"]) and not nb.any()
    fan = pr.RayFan.from_arrays(th, np.tile(o["r"], (M, 1)), o["T"], -o["z"], -o["p"], o["n_bott"], o["n_surf"],
                                np.full(M, cref.LLOYD_ZS))
    return fan, env, nb, ns


def test_lloyds_mirror_from_the_restatement(lloyd):
    fan, env, nb, ns = lloyd
    x = np.asarray(fan.rs[0])[cref.LLOYD_COLS]
    assert np.array_equal(x, [1e3, 2e3, 3e3, 4e3, 5e3])
    p = cref.fan_pressure(fan, cref.LLOYD_DEPTHS, env, cref.LLOYD_F, flatearth=False, nb=nb, ns=ns)
    e = cref.lloyd_error(p[:, cref.LLOYD_COLS], x)
    j, k = np.unravel_index(np.argmax(e), e.shape)
    print(f"Lloyd's mirror, restatement on the oracle's fan: worst e {e.max():.4e} at depth {cref.LLOYD_DEPTHS[j]} m, "
          f"range {x[k]} m; bound {cref.LLOYD_BOUND:.4e}")
    assert cref.LLOYD_BOUND == 2.0 * cref.LLOYD_MEASURED < 0.05
    assert e.max() <= cref.LLOYD_BOUND
    assert e.max() == pytest.approx(cref.LLOYD_MEASURED, rel=1e-3)                 # the constant is this fan's value
    # the test's power: without the surface phase e is of order 1
    q0 = cref.fan_pressure(fan, cref.LLOYD_DEPTHS, env, cref.LLOYD_F, flatearth=False)
    assert cref.lloyd_error(q0[:, cref.LLOYD_COLS], x).max() > 0.5
    # |p|^2 is the incoherent intensity where one tube arrives; here two do, and the field shows the interference fringes
    tl = -20 * np.log10(np.abs(p[:, cref.LLOYD_COLS]))
    assert tl.max() - tl.min() > 10.0


# ---- argument errors, no GPU -------------------------------------------------------------------------------------------------

def _host_fan(n=4, S=5, n_surfs=None, log=None):
    th = np.linspace(-5, 5, n)
    r = np.linspace(0, 10e3, S)
    zs = -(1000.0 + np.outer(np.tan(np.radians(th)), r))
    ps = np.tile(np.sin(np.radians(th))[:, None] / 1500.0, (1, S))
    ts = np.outer(1.0 / (1500.0 * np.cos(np.radians(th))), r)
    fan = pr.RayFan.from_arrays(th, np.tile(r, (n, 1)), ts, zs, ps, np.zeros(n, np.int64),
                                np.zeros(n, np.int64) if n_surfs is None else np.asarray(n_surfs), np.full(n, 1000.0))
    fan._bounces = log
    return fan


def _all_three(fan, env, **kw):
    return [lambda: pr.pressure_field(fan, [100.0], env, 50.0, flatearth=False, **kw),
            lambda: pr.coherent_transmission_loss(fan, [100.0], env, 50.0, flatearth=False, **kw),
            lambda: pr.caustic_index(fan, env, flatearth=False)]


@pytest.mark.parametrize("f", [-1.0, np.nan, np.inf, -np.inf])
def test_bad_frequency_is_refused_before_the_device(f):
    env = pr.OceanEnvironment2D(flat_earth_transform=False)
    for call in (pr.pressure_field, pr.coherent_transmission_loss):
        with pytest.raises(ValueError, match="frequency must be finite and >= 0"):
            call(_host_fan(), [100.0], env, f, flatearth=False)


def test_a_bounced_fan_needs_a_log_that_holds_every_bounce():
    env = pr.OceanEnvironment2D(flat_earth_transform=False)
    for call in _all_three(_host_fan(n_surfs=[0, 1, 0, 0]), env):
        with pytest.raises(ValueError, match="no bounce log.*max_bounces"):
            call()
    K1 = pr.BounceLog(np.full((4, 1), np.nan), np.full((4, 1), np.nan), np.full((4, 1), -1, np.int8))
    for call in _all_three(_host_fan(n_surfs=[0, 2, 0, 0], log=K1), env):
        with pytest.raises(ValueError, match="overflowed.*max_bounces=2"):
            call()
    # arrivals' lazy field raises the same error
    a = pr.Arrivals(np.zeros(2, np.int64), np.array([100.0]), np.array([10e3]), np.array([4]), np.zeros(0, np.int32),
                    *(np.zeros(0) for _ in range(4)), np.zeros(4), np.zeros((1, 1)))
    with pytest.raises(ValueError, match="built without their fan"):
        a.caustics
    a._source = (_host_fan(n_surfs=[0, 1, 0, 0]), env, False, 0)
    with pytest.raises(ValueError, match="no bounce log.*max_bounces"):
        a.caustics


def test_fewer_than_two_rays_and_the_tube_products_checks_are_refused_before_the_device():
    env = pr.OceanEnvironment2D(flat_earth_transform=False)
    for call in _all_three(_host_fan()[:1], env):
        with pytest.raises(ValueError, match="at least 2 rays"):
            call()
    with pytest.raises(ValueError, match="at least 2 rays"):
        pr.caustic_index(_host_fan()[:1])
    fan = _host_fan()
    with pytest.raises(ValueError, match="Flat earth transformation has not been applied"):
        pr.pressure_field(fan, [100.0], env, 50.0)
    with pytest.raises(ValueError, match="strictly ascending"):
        pr.pressure_field(fan, [200.0, 100.0], env, 50.0, flatearth=False)
    with pytest.raises(ValueError, match="absorption must be finite and >= 0"):
        pr.pressure_field(fan, [100.0], env, 50.0, flatearth=False, absorption=-1.0)
    with pytest.raises(ValueError, match="bounce log"):
        pr.pressure_field(fan, [100.0], env, 50.0, flatearth=False, surface_loss=1.0)
    with pytest.raises(ValueError, match="needs `env`"):
        pr.caustic_index(_host_fan(n_surfs=[0, 1, 0, 0], log=pr.BounceLog(np.full((4, 1), np.nan), np.full((4, 1), np.nan),
                                                                          np.full((4, 1), -1, np.int8))))


def test_the_new_functions_are_exported():
    for name in ("caustic_index", "pressure_field", "coherent_transmission_loss"):
        assert name in pr.__all__ and callable(getattr(pr, name))
    sig = inspect.signature(pr.pressure_field).parameters
    assert list(sig)[:8] == ["rays", "receiver_depths", "env", "frequency", "absorption", "bottom_loss", "surface_loss", "flatearth"]
    assert all(sig[k].default is None for k in ("absorption", "bottom_loss", "surface_loss")) and sig["flatearth"].default is True
    assert list(inspect.signature(pr.coherent_transmission_loss).parameters) == list(sig)
    assert list(inspect.signature(pr.caustic_index).parameters)[:2] == ["rays", "env"]
    assert inspect.signature(pr.caustic_index).parameters["env"].default is None
    assert isinstance(inspect.getattr_static(pr.Arrivals, "caustics"), property)
    from pygenray_amd import _lib
    own = _lib.HEADER_PROTOTYPES["pgr_coherent.h"]
    for name in ("pgr_fan_caustic_index", "pgr_caustic_index_device", "pgr_fan_pressure_w", "pgr_pressure_device_w"):
        assert name in own and all(name not in protos for h, protos in _lib.HEADER_PROTOTYPES.items() if h != "pgr_coherent.h")
    assert len(own) == 4
    assert len(own["pgr_pressure_device_w"][1]) == 16 and len(own["pgr_fan_pressure_w"][1]) == 10
