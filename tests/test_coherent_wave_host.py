"""The coherent convention against wave theory, without a GPU: the NumPy restatements (tests/coherent_reference.py,
signal_reference.py, spectrum_reference.py) on the CPU oracle's fans against the two truths of tests/wave_reference.py, which
share nothing with the ray code -- the normal modes of the focusing medium (the caustic phase, kappa from 0 to 4) and the image
sum of an isovelocity waveguide (bottom and surface bounces up to two each, tubes that have bounced on both).  The values
measured here are the ones wave_reference.py records; the GPU tests (tests/test_coherent_wave.py) use twice them as bounds."""
import numpy as np
import pytest

import pygenray_amd as pr

import bounce_reference as bref
import coherent_reference as cref
import signal_reference as sref
import spectrum_reference as spref
import wave_reference as wref
from helpers import y0_for


def _oracle_fan(env, source_depth, angles, x1, S):
    """the CPU oracle's fan (correctly rounded libm) as a host RayFan, with the oracle's own output and the unpacked tables"""
    import oracle
    arrs = pr._unpack_envi(env, flatearth=False)
    y0 = y0_for(oracle, arrs, source_depth, 0.0, -angles)
    o = oracle.shoot_fan(*arrs, y0, 0.0, x1, S, math=oracle.MATH_CR)
    assert (o["status"] == 0).all()
    M = len(angles)
    fan = pr.RayFan.from_arrays(angles, np.tile(o["r"], (M, 1)), o["T"], -o["z"], -o["p"], o["n_bott"], o["n_surf"],
                                np.full(M, source_depth))
    return fan, o, arrs, y0


# ---- normal modes of the focusing medium --------------------------------------------------------------------------------------

@pytest.fixture(scope="module")
def focus():
    env = cref.focus_env(pr)
    fan, o, _, _ = _oracle_fan(env, cref.FOCUS_Z0, cref.focus_angles(), cref.FOCUS_X1, cref.FOCUS_S)
    cref.check_focus_fan(o["r"], -o["z"], cref.caustic_index(o["z"]), o["status"], o["n_bott"], o["n_surf"])
    return fan, env, o["r"]


def test_the_comparison_cells_hold_every_caustic_count(focus):
    fan, _, x = focus
    cells, kappa = wref.mode_cells(x)
    per = wref.check_mode_cells(cells, kappa)
    print(f"focusing medium: {int(cells.sum())} of {cells.size} cells compared; per kappa 0 ... 4: {per}")
    assert cells.shape == (29, 601) and cells.size == 17429 and not cells[:, x <= wref.MODE_X_MIN].any()
    # inside the fan proper: every compared cell lies between the outermost rays' depths at its column
    d = -np.asarray(fan.zs)
    D = np.broadcast_to(wref.MODE_DEPTHS[:, None], cells.shape)
    assert (D[cells] > np.broadcast_to(d.min(axis=0), cells.shape)[cells]).all()
    assert (D[cells] < np.broadcast_to(d.max(axis=0), cells.shape)[cells]).all()


@pytest.mark.parametrize("f", wref.MODE_F)
def test_caustic_phase_against_the_normal_modes(focus, f):
    fan, env, x = focus
    cells, kappa = wref.mode_cells(x)
    ref = wref.modal_field(f, wref.MODE_DEPTHS, x)
    p = cref.fan_pressure(fan, wref.MODE_DEPTHS, env, f, flatearth=False)
    e = wref.mode_error(p, ref, cells)
    j, k = np.unravel_index(np.argmax(e), e.shape)
    phase = np.abs(np.angle(p[cells] / ref[cells])).max()
    print(f"normal modes at {f} Hz (dz {wref.MODE_DZ} m, {len(wref.modes(f)[0])} modes), restatement on the oracle's fan: worst e "
          f"{e.max():.4e} at depth {wref.MODE_DEPTHS[j]} m, range {x[k]} m; median {np.median(e[cells]):.2e}; worst phase "
          f"difference {phase:.4f} rad; bound {wref.MODE_BOUND:.4e}")
    assert wref.MODE_BOUND == 2.0 * max(wref.MODE_MEASURED.values()) < 0.1
    assert e.max() <= wref.MODE_BOUND
    assert e.max() == pytest.approx(wref.MODE_MEASURED[f], rel=1e-3)               # the constant is this fan's value
    # the test's power: with the caustic phase taken out, no cell behind an odd number of foci comes near
    p0 = cref.fan_pressure(fan, wref.MODE_DEPTHS, env, f, flatearth=False, q=np.zeros(np.asarray(fan.zs).shape, np.int32))
    e0 = wref.mode_error(p0, ref, cells)
    odd = cells & (kappa % 2 == 1)[None, :]
    print(f"  without the caustic phase: min e {e0[odd].min():.3f} on the {int(odd.sum())} cells with odd kappa, "
          f"{e0[cells & (kappa == 2)[None, :]].min():.3f} at kappa = 2")
    assert e0[odd].min() > 1.0
    assert e0[cells & (kappa == 0)[None, :]].max() <= wref.MODE_BOUND             # (kappa = 0 has no caustic phase to lose)


def test_the_mode_solve_is_not_what_limits_the_comparison(focus):
    """the same check at half the depth step: the worst error moves by far less than the bound's margin"""
    fan, env, x = focus
    cells, _ = wref.mode_cells(x)
    p = cref.fan_pressure(fan, wref.MODE_DEPTHS, env, 50.0, flatearth=False)
    e1 = wref.mode_error(p, wref.modal_field(50.0, wref.MODE_DEPTHS, x), cells).max()
    e2 = wref.mode_error(p, wref.modal_field(50.0, wref.MODE_DEPTHS, x, dz=0.5 * wref.MODE_DZ), cells).max()
    print(f"normal modes at 50 Hz: worst e {e1:.4e} at dz {wref.MODE_DZ} m, {e2:.4e} at dz {0.5 * wref.MODE_DZ} m")
    assert e2 <= wref.MODE_BOUND and abs(e2 - e1) < 0.25 * wref.MODE_MEASURED[50.0]


# ---- the isovelocity waveguide ------------------------------------------------------------------------------------------------

def _guide_fan(n):
    """the oracle's fan of n rays in the waveguide and the per-sample counts from the oracle's own bounces"""
    env = wref.guide_env(pr)
    th = wref.guide_angles(n)
    fan, o, arrs, y0 = _oracle_fan(env, wref.GUIDE_ZS, th, wref.GUIDE_X1, wref.GUIDE_S)
    assert o["n_bott"].max() == 2 and o["n_surf"].max() == 2
    bx, bk = np.full((n, wref.GUIDE_K), np.nan), np.full((n, wref.GUIDE_K), -1, np.int8)
    for i in np.flatnonzero(o["n_surf"] + o["n_bott"] > 0):
        xb, _, kind = bref.trace_bounces(arrs, y0[i], 0.0, wref.GUIDE_X1)
        assert len(xb) == o["n_surf"][i] + o["n_bott"][i] <= wref.GUIDE_K
        bx[i, :len(xb)], bk[i, :len(xb)] = xb, kind
    nb, ns = cref.log_counts(bx, bk, o["r"])
    assert np.array_equal(ns[:, -1], o["n_surf"]) and np.array_equal(nb[:, -1], o["n_bott"])
    assert ((nb > 0) & (ns > 0)).any()                                   # tubes that have bounced on both boundaries
    return fan, env, nb, ns, o


@pytest.fixture(scope="module")
def guide():
    return _guide_fan(wref.GUIDE_N)


def _wrong_conventions(d, nb, ns):
    """three q (M, S) the definition could have been: the bottom taken as pressure release, the mirror flips not undone (kappa
    without the counts), the surface phase dropped"""
    alike = (nb[:-1] == nb[1:]) & (ns[:-1] == ns[1:])
    kappa = cref.caustic_index(d, nb, ns)

    def q(k, extra):
        out = np.zeros(d.shape, np.int32)
        out[:-1] = np.where(alike, k + extra[:-1], -1)
        return out
    return {"bottom taken as pressure release": q(kappa, 2 * (ns + nb)), "flips not undone": q(cref.caustic_index(d), 2 * ns),
            "surface phase dropped": q(kappa, 0 * ns)}


def test_the_fan_overshoots_a_boundary_by_at_most_half_a_save_step_of_its_steepest_ray(guide):
    """a bounce counts from the nearest save column, and before its bounce the sample there is the reflected segment continued
    backwards: arrivals are missing in a strip up to tan(theta_max) dx / 2 wide, not 'about one tube' (3 m here)"""
    fan, _, _, _, o = guide
    d = o["z"]
    strip = wref.guide_strip(o["r"])
    print(f"waveguide: the oracle fan's depths span {d.min():.1f} ... {d.max():.1f} m; the strip is {strip:.1f} m wide, the tubes "
          f"{np.median(np.abs(np.diff(d[:, -1]))):.1f} m")
    assert strip == pytest.approx(41.95, abs=0.01)
    assert -strip <= d.min() < -0.9 * strip and wref.GUIDE_H + 0.9 * strip < d.max() <= wref.GUIDE_H + strip
    assert wref.GUIDE_DEPTHS.min() > strip and wref.GUIDE_DEPTHS.max() < wref.GUIDE_H - strip
    assert np.median(np.abs(np.diff(d[:, -1]))) < 0.1 * strip


def test_waveguide_image_sum_from_the_restatement(guide):
    fan, env, nb, ns, o = guide
    x = o["r"][wref.GUIDE_COLS]
    assert np.array_equal(x, [1e3, 2e3, 3e3, 4e3, 5e3])
    keep = wref.check_guide_cells(x)
    assert (cref.caustic_index(o["z"], nb, ns) == 0).all()               # straight rays: no caustic, whatever they bounce on
    p = cref.fan_pressure(fan, wref.GUIDE_DEPTHS, env, wref.GUIDE_F, flatearth=False, nb=nb, ns=ns)[:, wref.GUIDE_COLS]
    e = wref.guide_error(p, x)
    j, k = np.unravel_index(np.argmax(e), e.shape)
    print(f"waveguide, restatement on the oracle's fan: {int(keep.sum())} of {keep.size} cells; worst e {e.max():.4e} at depth "
          f"{wref.GUIDE_DEPTHS[j]} m, range {x[k]} m; median {np.median(e[keep]):.2e}; bound {wref.GUIDE_BOUND:.4e}")
    assert wref.GUIDE_BOUND == 2.0 * wref.GUIDE_MEASURED < 0.01
    assert e.max() <= wref.GUIDE_BOUND
    assert e.max() == pytest.approx(wref.GUIDE_MEASURED, rel=1e-3)                  # the constant is this fan's value
    # the test's power: each of three wrong conventions misses by order 1 on most cells
    for name, q in _wrong_conventions(o["z"], nb, ns).items():
        pw = cref.fan_pressure(fan, wref.GUIDE_DEPTHS, env, wref.GUIDE_F, flatearth=False, nb=nb, ns=ns, q=q)
        ew = wref.guide_error(pw[:, wref.GUIDE_COLS], x)[keep]
        print(f"  {name}: median e {np.median(ew):.2f}, {100 * (ew > 0.1).mean():.0f} % of the cells above 0.1")
        assert np.median(ew) > 0.5 and (ew > 0.1).mean() > 0.75, name


def test_waveguide_image_sum_with_half_the_rays():
    """the error is the fan's density, not a constant offset: 2001 rays stay within the same cap"""
    fan, env, nb, ns, o = _guide_fan(2001)
    x = o["r"][wref.GUIDE_COLS]
    p = cref.fan_pressure(fan, wref.GUIDE_DEPTHS, env, wref.GUIDE_F, flatearth=False, nb=nb, ns=ns)[:, wref.GUIDE_COLS]
    e = wref.guide_error(p, x)
    print(f"waveguide, 2001 rays: worst e {e.max():.4e}")
    assert wref.GUIDE_MEASURED < e.max() < 0.01


@pytest.fixture(scope="module")
def guide_arrivals(guide):
    fan, env, nb, ns, o = guide
    off, T, I, q = sref.fan_arrivals(fan, wref.GUIDE_DEPTHS, env, wref.GUIDE_COLS, flatearth=False, nb=nb, ns=ns)
    assert np.diff(off).max() >= 9 and {0, 2, 4} <= set(q.tolist()) <= {-1, 0, 2, 4}
    return off, T, I, q, o["r"][wref.GUIDE_COLS]


def test_waveguide_transfer_function_with_a_reduction_time_from_the_restatement(guide_arrivals):
    off, T, I, q, x = guide_arrivals
    R, n = len(wref.GUIDE_DEPTHS), len(x)
    Hf = spref.spectrum_sum(off, T, I, q, None, np.tile(x / wref.GUIDE_C, R), wref.GUIDE_BAND, None).reshape(R, n, -1)
    e = wref.guide_band_error(Hf, x)
    print(f"waveguide transfer function at {wref.GUIDE_BAND.tolist()} Hz, t_reduce = x / c, restatement on the oracle's fan: worst e "
          f"per frequency {[f'{v:.4e}' for v in e.max(axis=(0, 1))]}; bound {wref.GUIDE_BAND_BOUND:.4e}")
    assert wref.GUIDE_BAND_BOUND == 2.0 * wref.GUIDE_BAND_MEASURED < 0.01
    assert e.max() <= wref.GUIDE_BAND_BOUND
    assert e.max() == pytest.approx(wref.GUIDE_BAND_MEASURED, rel=1e-3)
    # the test's power: with the surface phase dropped e is of order 1; so it is without the reduction time wherever f x / c is
    # no whole number of cycles (it is one at 3 km for every frequency and at 45 and 60 Hz for every range: 13 entries of 25)
    keep = wref.guide_images(x)[3]
    H1 = spref.spectrum_sum(off, T, I, np.where(q >= 0, 0, q), None, np.tile(x / wref.GUIDE_C, R), wref.GUIDE_BAND, None)
    assert np.median(wref.guide_band_error(H1.reshape(R, n, -1), x)[keep]) > 0.5
    H0 = spref.spectrum_sum(off, T, I, q, None, np.zeros(R * n), wref.GUIDE_BAND, None).reshape(R, n, -1)
    cycles = np.outer(x / wref.GUIDE_C, wref.GUIDE_BAND)
    turned = np.abs(cycles - np.rint(cycles)) > 0.1
    assert turned.sum() == 12
    assert np.median(wref.guide_band_error(H0, x)[keep[:, :, None] & turned[None, :, :]]) > 0.5


def test_waveguide_pulse_from_the_restatement(guide_arrivals):
    off, T, I, q, x = guide_arrivals
    R, n = len(wref.GUIDE_DEPTHS), len(x)
    wref.check_guide_pulse(x)
    tstart = np.tile(wref.guide_t0(x), R)
    rs = sref.inv_sigma(wref.GUIDE_B)
    u = sref.signal_sum(off, T, I, q, tstart, wref.GUIDE_F, rs, wref.GUIDE_DT, wref.GUIDE_NT).reshape(R, n, wref.GUIDE_NT)
    e = wref.guide_pulse_error(u, x)
    j, k, m = np.unravel_index(np.argmax(e), e.shape)
    print(f"waveguide with a pulse, restatement on the oracle's fan: worst e {e.max():.4e} at depth {wref.GUIDE_DEPTHS[j]} m, "
          f"range {x[k]} m, sample {m}; bound {wref.GUIDE_PULSE_BOUND:.4e}")
    assert wref.GUIDE_PULSE_BOUND == 2.0 * wref.GUIDE_PULSE_MEASURED < 0.01
    assert e.max() <= wref.GUIDE_PULSE_BOUND
    assert e.max() == pytest.approx(wref.GUIDE_PULSE_MEASURED, rel=1e-3)
    keep = wref.guide_images(x)[3]
    assert (np.abs(u).max(axis=2) > 0).all() and (np.abs(u[:, :, 0]) == 0).all() and (np.abs(u[:, :, -1])[keep] == 0).all()
    # the test's power: without the surface phase e is of order 1
    u0 = sref.signal_sum(off, T, I, np.where(q >= 0, 0, q), tstart, wref.GUIDE_F, rs, wref.GUIDE_DT, wref.GUIDE_NT)
    assert wref.guide_pulse_error(u0.reshape(R, n, wref.GUIDE_NT), x).max() > 0.5
