"""Received signal of a Gaussian pulse without a GPU: the NumPy restatement (tests/signal_reference.py) against the Fourier
identity that ties it to the CW sum, against Lloyd's mirror with a pulse on the CPU oracle's fan, on hand cases at the cut and
at NaN inputs, and the argument errors refused before anything reaches the device."""
import inspect
import math

import numpy as np
import pytest

import pygenray_amd as pr

import coherent_reference as cref
import signal_reference as sref
from test_coherent_host import _host_fan, lloyd  # noqa: F401  (the oracle's Lloyd fan and the hand-made host fan)


# ---- the Fourier identity ---------------------------------------------------------------------------------------------------

def synthetic_arrivals(seed=11, G=6):
    """seeded groups of 0 ... 40 arrivals with T in [60, 62] s, intensities over six decades, q in -1 ... 9"""
    rng = np.random.default_rng(seed)
    cnt = rng.integers(1, 41, G)
    cnt[1] = 0
    off = np.concatenate([[0], np.cumsum(cnt)])
    n = int(off[-1])
    T = np.sort(rng.uniform(60.0, 62.0, n))
    I = 10.0 ** rng.uniform(-12.0, -6.0, n)
    q = rng.integers(-1, 10, n).astype(np.int32)
    return off, T, I, q


def fourier_check(off, T, I, q, u, t, dt, sigma, f=sref.FOURIER_F, say=None):
    """|U(nu) - Ehat(nu) P(f + nu)| <= FOURIER_REL sigma sqrt(2 pi) sum_a amp_a at every nu of the issue, for every group; u, t
    (G, n_times) -> the worst ratio to the bound"""
    amp = np.where(np.asarray(q) >= 0, np.sqrt(I), 0.0)
    A = np.array([amp[off[g]:off[g + 1]].sum() for g in range(len(off) - 1)])
    bound = sref.FOURIER_REL * sigma * math.sqrt(2 * math.pi) * A
    worst = 0.0
    for nu in sref.FOURIER_NU:
        U = sref.spectrum(u, t, dt, nu)
        ref = sref.pulse_spectrum(sigma, nu) * sref.cw_sum(off, T, I, q, f + nu)
        err = np.abs(U - ref)
        lit = A > 0
        worst = max(worst, float((err[lit] / bound[lit]).max())) if lit.any() else worst
        assert (err <= bound).all(), (nu, err, bound)
        assert (np.abs(ref[lit]) > 100 * bound[lit]).any()              # the identity is about something
    if say:
        print(f"{say}: worst |U - Ehat P| is {worst:.3e} of the bound")
    return worst


def test_fourier_identity_on_the_restatement(monkeypatch):
    off, T, I, q = synthetic_arrivals()
    sigma = sref.pulse_sigma(sref.FOURIER_B)
    t0, dt, nt = sref.covering_axis(T.min(), T.max(), sigma)
    assert dt == sigma / 2 and t0 <= T.min() - 9 * sigma and t0 + (nt - 1) * dt >= T.max() + 9 * sigma
    G = len(off) - 1
    tstart = np.full(G, t0)
    rs = sref.inv_sigma(sref.FOURIER_B)
    t = sref.sample_times(tstart, dt, nt)
    u = sref.signal_sum(off, T, I, q, tstart, sref.FOURIER_F, rs, dt, nt)
    assert (u[1] == 0).all() and (np.abs(u[0]) > 0).any()
    fourier_check(off, T, I, q, u, t, dt, sigma, say="Fourier identity, restatement")
    # the test's power: a 6-sigma cut, a missing q and a flipped sign of the phase all miss the bound
    monkeypatch.setattr(sref, "CUT", 36.0)
    cut6 = sref.signal_sum(off, T, I, q, tstart, sref.FOURIER_F, rs, dt, nt)
    monkeypatch.undo()
    for wrong in (cut6, sref.signal_sum(off, T, I, np.where(q >= 0, 0, q), tstart, sref.FOURIER_F, rs, dt, nt), np.conj(u)):
        with pytest.raises(AssertionError):
            fourier_check(off, T, I, q, wrong, t, dt, sigma)


# ---- Lloyd's mirror with a pulse ------------------------------------------------------------------------------------------------

def test_lloyds_mirror_with_a_pulse_from_the_restatement(lloyd):  # noqa: F811
    fan, env, nb, ns = lloyd
    x = np.asarray(fan.rs[0])[cref.LLOYD_COLS]
    off, T, I, q = sref.fan_arrivals(fan, cref.LLOYD_DEPTHS, env, cref.LLOYD_COLS, flatearth=False, nb=nb, ns=ns)
    R, n = len(cref.LLOYD_DEPTHS), len(x)
    assert (np.diff(off) >= 2).all() and {0, 2} <= set(q.tolist()) <= {-1, 0, 2}                  # the direct and the surface path
    tstart = np.tile(sref.lloyd_t0(x), R)
    rs = sref.inv_sigma(sref.LLOYD_B)
    u = sref.signal_sum(off, T, I, q, tstart, cref.LLOYD_F, rs, sref.LLOYD_DT, sref.LLOYD_NT).reshape(R, n, sref.LLOYD_NT)
    e = sref.lloyd_pulse_error(u, x)
    j, k, m = np.unravel_index(np.argmax(e), e.shape)
    print(f"Lloyd's mirror with a pulse, restatement on the oracle's fan: worst e {e.max():.4e} at depth "
          f"{cref.LLOYD_DEPTHS[j]} m, range {x[k]} m, sample {m}; bound {sref.LLOYD_PULSE_BOUND:.4e}")
    assert sref.LLOYD_PULSE_BOUND == 2.0 * sref.LLOYD_PULSE_MEASURED < 0.05
    assert e.max() <= sref.LLOYD_PULSE_BOUND
    assert e.max() == pytest.approx(sref.LLOYD_PULSE_MEASURED, rel=1e-3)            # the constant is this fan's value
    # both pulses lie on the time axis, and they overlap: the signal's peak is neither path's own amplitude
    assert (np.abs(u).max(axis=2) > 0).all() and (np.abs(u[:, :, 0]) == 0).all() and (np.abs(u[:, :, -1]) == 0).all()
    # the test's power: without the surface phase e is of order 1
    u0 = sref.signal_sum(off, T, I, np.zeros_like(q), tstart, cref.LLOYD_F, rs, sref.LLOYD_DT, sref.LLOYD_NT)
    assert sref.lloyd_pulse_error(u0.reshape(R, n, sref.LLOYD_NT), x).max() > 0.5
    # B = 0: every sample is the CW field of test_coherent_host.py, bit for bit
    cw = sref.signal_sum(off, T, I, q, tstart, cref.LLOYD_F, 0.0, sref.LLOYD_DT, 3).reshape(R, n, 3)
    p = cref.fan_pressure(fan, cref.LLOYD_DEPTHS, env, cref.LLOYD_F, flatearth=False, nb=nb, ns=ns)[:, cref.LLOYD_COLS]
    assert all(np.array_equal(cw[:, :, m], p) for m in range(3))


# ---- small hand cases -------------------------------------------------------------------------------------------------------

def test_rs_zero_reproduces_the_cw_sum_bit_for_bit():
    off, T, I, q = synthetic_arrivals(seed=3)
    G = len(off) - 1
    u = sref.signal_sum(off, T, I, q, np.linspace(-5.0, 70.0, G), 75.0, 0.0, 0.37, 5)
    p = sref.cw_sum(off, T, I, q, 75.0)
    assert all(np.array_equal(u[:, m], p) for m in range(5)) and (np.abs(p) > 0).sum() == G - 1
    from beam_reference import gexp
    assert gexp(np.array([-0.0]))[0] == 1.0 and gexp(np.array([-32.0]))[0] == pytest.approx(math.exp(-32.0), rel=1e-15)


def test_pulse_sigma():
    assert pr.pulse_sigma(0) == math.inf and pr.pulse_sigma(0.0) == math.inf
    for B in (0.5, 20.0, 1e3):
        s = pr.pulse_sigma(B)
        assert s == pytest.approx(math.sqrt(math.log(2)) / (math.pi * B), rel=1e-15) and s == sref.pulse_sigma(B)
        # the half-power points of the spectrum exp(-2 pi^2 sigma^2 nu^2) of the envelope lie B apart: |Ehat(B/2)|^2 = 1/2
        assert math.exp(-2 * math.pi ** 2 * s ** 2 * (B / 2) ** 2) ** 2 == pytest.approx(0.5, rel=1e-14)
        from pygenray_amd._fan_frame import _inv_sigma
        assert _inv_sigma(B) == sref.inv_sigma(B) == pytest.approx(1.0 / s, rel=1e-15)
    from pygenray_amd._fan_frame import _inv_sigma
    assert _inv_sigma(0) == 0.0
    for bad in (-1.0, math.nan, math.inf):
        with pytest.raises(ValueError, match="bandwidth must be finite and >= 0"):
            pr.pulse_sigma(bad)


def test_the_cut_lies_at_eight_sigma_exactly():
    # rs = 1, the sample at t = 0: an arrival at T = 8 has v = 64 and is kept; one ulp further it is not
    off = np.array([0, 1])
    one = np.ones(1)
    for T, kept in ((8.0, True), (np.nextafter(8.0, 9.0), False), (-8.0, True), (np.nextafter(-8.0, -9.0), False)):
        u = sref.signal_sum(off, np.array([T]), one, None, np.zeros(1), 0.0, 1.0, 1.0, 1)
        assert (u[0, 0] != 0) == kept, T
        if kept:
            assert u[0, 0].real == pytest.approx(math.exp(-32.0), rel=1e-14) and u[0, 0].imag == 0.0


def test_negative_q_and_nan_inputs():
    off = np.array([0, 4])
    T = np.array([1.0, 1.2, np.nan, 1.1])
    I = np.array([4.0, 9.0, 1.0, 16.0])
    tstart, rs, dt, nt = np.array([0.0]), 10.0, 0.05, 60
    base = sref.signal_sum(np.array([0, 1]), T[:1], I[:1], None, tstart, 0.0, rs, dt, nt)
    # q < 0 and a NaN T add nothing
    u = sref.signal_sum(off, T, I, np.array([0, -1, 0, -5]), tstart, 0.0, rs, dt, nt)
    assert np.array_equal(u, base) and (u.real.max() == 2.0) and not np.isnan(u.view(float)).any()
    # ... also at rs = 0, where every finite arrival is in every sample
    u0 = sref.signal_sum(off, T, I, None, tstart, 0.0, 0.0, dt, 3)
    assert (u0 == 2.0 + 3.0 + 4.0).all()
    # a NaN I makes exactly its window NaN
    In = I.copy()
    In[1] = np.nan
    un = sref.signal_sum(off, T, In, None, tstart, 0.0, rs, dt, nt)
    t = sref.sample_times(tstart, dt, nt)[0]
    x = (t - 1.2) * rs
    window = x * x <= 64.0
    assert 0 < window.sum() < nt and np.array_equal(np.isnan(un[0].real), window) and np.array_equal(np.isnan(un[0].imag), window)


# ---- argument errors and the API, no GPU ---------------------------------------------------------------------------------------

def _call(fan=None, depths=(100.0,), f=50.0, B=20.0, t0=0.0, dt=1e-3, nt=16, **kw):
    env = pr.OceanEnvironment2D(flat_earth_transform=False)
    return pr.received_signal(_host_fan() if fan is None else fan, list(depths), env, f, B, t0, dt, nt,
                              **dict(dict(flatearth=False), **kw))


def test_bad_arguments_are_refused_before_the_device():
    for f in (-1.0, np.nan, np.inf):
        with pytest.raises(ValueError, match="frequency must be finite and >= 0"):
            _call(f=f)
    for B in (-1.0, np.nan, np.inf):
        with pytest.raises(ValueError, match="bandwidth must be finite and >= 0"):
            _call(B=B)
    for dt in (0.0, -1e-3, np.nan, np.inf):
        with pytest.raises(ValueError, match="dt must be finite and > 0"):
            _call(dt=dt)
    for nt in (0, -3, 2.5, 65535 * 256 + 1):
        with pytest.raises(ValueError, match="n_times must be"):
            _call(nt=nt)
    with pytest.raises(ValueError, match="t0 must be a scalar or one start time per requested column"):
        _call(t0=[0.0, 1.0])
    with pytest.raises(ValueError, match="t0 must be a scalar or one start time per requested column"):
        _call(t0=[0.0, 1.0, 2.0], range_indices=[1, 2])
    with pytest.raises(ValueError, match="t0 must be finite"):
        _call(t0=np.nan)
    with pytest.raises(ValueError, match="range_indices must lie"):
        _call(range_indices=[5])
    # pressure_field's own errors
    with pytest.raises(ValueError, match="strictly ascending"):
        _call(depths=(200.0, 100.0))
    with pytest.raises(ValueError, match="at least 2 rays"):
        _call(fan=_host_fan()[:1])
    with pytest.raises(ValueError, match="Flat earth transformation has not been applied"):
        _call(flatearth=True)
    with pytest.raises(ValueError, match="absorption must be finite and >= 0"):
        _call(absorption=-1.0)
    with pytest.raises(ValueError, match="bounce log"):
        _call(surface_loss=1.0)
    with pytest.raises(ValueError, match="no bounce log.*max_bounces"):
        _call(fan=_host_fan(n_surfs=[0, 1, 0, 0]))


def test_the_new_names_are_exported_and_the_entry_is_bound_from_its_own_header():
    for name in ("received_signal", "pulse_sigma"):
        assert name in pr.__all__ and callable(getattr(pr, name))
    sig = inspect.signature(pr.received_signal).parameters
    assert list(sig) == ["rays", "receiver_depths", "env", "frequency", "bandwidth", "t0", "dt", "n_times", "range_indices",
                         "absorption", "bottom_loss", "surface_loss", "flatearth", "device"]
    assert all(sig[k].default is None for k in ("range_indices", "absorption", "bottom_loss", "surface_loss"))
    assert sig["flatearth"].default is True and sig["device"].default == 0
    assert "centre frequency" in pr.received_signal.__doc__ and "not varied across the band" in pr.received_signal.__doc__
    from pygenray_amd import _lib
    own = _lib.HEADER_PROTOTYPES["pgr_signal.h"]
    assert len(own) == 1 and len(own["pgr_signal_device"][1]) == 14
    assert all("pgr_signal_device" not in protos for h, protos in _lib.HEADER_PROTOTYPES.items() if h != "pgr_signal.h")
    assert callable(_lib.signal_device)
    # pgr.h hands the entry to a C caller through the header of its own
    text = open(_lib.HEADER).read()
    assert '#include "pgr_signal.h"' in text and text.index('#include "pgr_signal.h"') < text.rindex("#ifdef __cplusplus")
