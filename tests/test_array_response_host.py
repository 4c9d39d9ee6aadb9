"""Vertical-array beamforming without a GPU: ``steering_delays`` by hand, the NumPy restatement (tests/array_reference.py)
against ``signal_reference.signal_sum`` at one element, against the CW conventional beamformer at rs = 0 and against Lloyd's
mirror seen by a 41-element array on exact straight rays, and the API: the exports, the one prototype in a header of its own
and every argument refused before anything reaches the device."""
import ctypes
import inspect
import math
import os

import numpy as np
import pytest

import pygenray_amd as pr

import array_reference as xref
import beam_pressure_reference as bp
import reflection_reference as rref
import signal_reference as sref
from test_coherent_host import _host_fan
from test_signal_host import synthetic_arrivals


# ---- steering_delays ------------------------------------------------------------------------------------------------------------

def test_steering_delays_by_hand():
    d = pr.steering_delays([100.0, 200.0, 400.0], [-90.0, 0.0, 30.0], 1500.0, reference_depth=200.0)
    assert d.shape == (3, 3) and d.dtype == np.float64
    # a look at +30 degrees (an arrival travelling upwards, received_angle's sign): the element 200 m below the reference hears
    # it 200 sin(30 deg) / 1500 s EARLIER, the one 100 m above it later
    assert d[2, 2] == pytest.approx(-200.0 * 0.5 / 1500.0, rel=1e-15) and d[0, 2] == pytest.approx(100.0 * 0.5 / 1500.0, rel=1e-15)
    assert d[2, 0] == pytest.approx(200.0 / 1500.0, rel=1e-15) and (d[1] == 0).all() and (d[:, 1] == 0).all()
    assert np.array_equal(d, xref.steering([100.0, 200.0, 400.0], [-90.0, 0.0, 30.0], 1500.0, 200.0))
    # the default reference is the mean depth
    m = pr.steering_delays([100.0, 200.0, 400.0], [30.0], 1500.0)
    assert np.array_equal(m, pr.steering_delays([100.0, 200.0, 400.0], [30.0], 1500.0, reference_depth=700.0 / 3.0))
    assert abs(m.sum()) < 1e-17 and np.array_equal(m, xref.steering([100.0, 200.0, 400.0], [30.0], 1500.0))
    # one sound speed per column: one (R, B) table per column, each the scalar call's
    per = pr.steering_delays([100.0, 400.0], [-10.0, 20.0], [1480.0, 1500.0, 1520.0])
    assert per.shape == (3, 2, 2)
    for k, c in enumerate((1480.0, 1500.0, 1520.0)):
        assert np.array_equal(per[k], pr.steering_delays([100.0, 400.0], [-10.0, 20.0], c))
    for bad in ([], [[1.0]], [np.nan], [91.0], [-90.5], [np.inf]):
        with pytest.raises(ValueError, match="angles must be"):
            pr.steering_delays([100.0], bad, 1500.0)
    for bad in (0.0, -1.0, np.nan, np.inf, [[1500.0]]):
        with pytest.raises(ValueError, match="sound_speed must be"):
            pr.steering_delays([100.0], [0.0], bad)
    with pytest.raises(ValueError, match="at least 1 element"):
        pr.steering_delays([], [0.0], 1500.0)
    with pytest.raises(ValueError, match="reference_depth must be finite"):
        pr.steering_delays([100.0], [0.0], 1500.0, reference_depth=np.nan)


# ---- the restatement against the single-receiver sums -------------------------------------------------------------------------------

def _same(a, b):
    return np.array_equal(a, b, equal_nan=True)


def test_one_element_without_delay_or_weight_is_the_signal_sum_bit_for_bit():
    off, T, I, q = synthetic_arrivals(seed=21, G=3)                          # three column slots of one element
    G = len(off) - 1
    tstart = np.array([59.9, 60.3, 60.1])
    f, rs, dt, nt = 75.0, sref.inv_sigma(20.0), 2e-3, 300
    zero, one = np.zeros((G, 1)), np.ones(G)
    for qq in (q, None):
        u = sref.signal_sum(off, T, I, qq, tstart, f, rs, dt, nt)
        y = xref.array_sum(off, T, I, qq, None, zero, one, tstart, 1, G, f, rs, dt, nt)
        assert y.shape == (G, 1, nt) and _same(y[:, 0].real, u.real) and _same(y[:, 0].imag, u.imag)
        assert (np.abs(u) > 0).any() and (u[1] == 0).all()
    u = sref.signal_sum(off, T, I, q, tstart, f, rs, dt, nt)
    # phi: zero lag and whole cycles leave every bit alone ...
    rng = np.random.default_rng(4)
    for phi in (np.zeros(len(T)), rng.integers(-1000, 1001, len(T)).astype(float)):
        y = xref.array_sum(off, T, I, q, phi, zero, one, tstart, 1, G, f, rs, dt, nt)
        assert _same(y[:, 0].real, u.real) and _same(y[:, 0].imag, u.imag)
        up = rref.signal_sum(off, T, I, q, phi, tstart, f, rs, dt, nt)
        assert _same(up.real, u.real) and _same(up.imag, u.imag)
    # ... a general lag gives reflection_reference's sum, bit for bit ...
    phi = rng.uniform(-3.0, 3.0, len(T))
    y = xref.array_sum(off, T, I, q, phi, zero, one, tstart, 1, G, f, rs, dt, nt)
    up = rref.signal_sum(off, T, I, q, phi, tstart, f, rs, dt, nt)
    assert _same(y[:, 0].real, up.real) and _same(y[:, 0].imag, up.imag) and not _same(up.real, u.real)
    # ... and a quarter cycle is one more step of q: within the rounding of the phase, 1e-15 of the amplitudes that add
    y = xref.array_sum(off, T, I, q, np.full(len(T), 0.25), zero, one, tstart, 1, G, f, rs, dt, nt)
    u1 = sref.signal_sum(off, T, I, np.where(q >= 0, q + 1, q), tstart, f, rs, dt, nt)
    amp = np.where(q >= 0, np.sqrt(I), 0.0)
    A = np.array([amp[off[g]:off[g + 1]].sum() for g in range(G)])
    assert (np.abs(y[:, 0] - u1) <= 1e-15 * A[:, None]).all() and (np.abs(u1 - u) > 1e-9 * A[:, None]).any()


def _array_case(seed=31, R=4, n=2, B=5):
    """seeded arrival lists of R elements x n column slots, delays of both signs, weights with a zero and a negative one"""
    off, T, I, q = synthetic_arrivals(seed=seed, G=R * n)
    rng = np.random.default_rng(seed)
    delay = rng.uniform(-0.05, 0.05, (R * n, B))
    delay[0] = 0.0
    weight = rng.uniform(0.2, 1.0, R * n)
    weight[2], weight[3] = 0.0, -0.7
    phi = rng.uniform(-2.0, 2.0, len(T))
    return off, T, I, q, phi, delay, weight


def test_cw_limit_is_the_conventional_beamformer():
    R, n, B, f = 4, 2, 5, 75.0
    off, T, I, q, phi, delay, weight = _array_case(R=R, n=n, B=B)
    # travel times of 3 ... 5 s, a 5 km range's: f T < 512 cycles, so the roundings of f Ts and f T are at most 2.9e-14 cycles
    # each and that of Ts 1.7e-14 -- 4.6e-13 rad together, inside the bound; at 60 s the roundings of f T alone are 2.9e-12 rad
    T = T - 57.0
    assert 3.0 <= T.min() and T.max() <= 5.0 and np.abs(delay).max() <= 0.05
    amp = np.where(q >= 0, np.sqrt(I), 0.0)
    A = np.array([amp[off[g]:off[g + 1]].sum() for g in range(R * n)])
    for lag in (None, phi):
        y = xref.array_sum(off, T, I, q, lag, delay, weight, np.array([3.0, -8.0]), R, n, f, 0.0, 0.37, 3)
        p = sref.cw_sum(off, T, I, q, f) if lag is None else rref.cw_sum(off, T, I, q, lag, f)
        ref = (weight[:, None] * np.exp(-2j * np.pi * f * delay) * p[:, None]).reshape(R, n, B).sum(axis=0)     # (n, B)
        bound = 1e-12 * (np.abs(weight) * A).reshape(R, n).sum(axis=0)
        assert all((np.abs(y[:, :, m] - ref) <= bound[:, None]).all() for m in range(3))
        assert (np.abs(ref) > 1e6 * bound[:, None]).any() and _same(y[:, :, 0], y[:, :, 2])


# ---- Lloyd's mirror seen by a vertical array ---------------------------------------------------------------------------------------

@pytest.fixture(scope="module")
def lloyd_array():
    """the restatement on the exact straight rays: the response, the closed form's ingredients and the arrivals"""
    a, q = xref.exact_array_arrivals()
    R, B = len(xref.ARRAY_DEPTHS), len(xref.ARRAY_LOOKS)
    assert (np.diff(a["offsets"]) == 2).all() and set(q.tolist()) == {0, 2}          # the direct and the surface path
    delta = pr.steering_delays(xref.ARRAY_DEPTHS, xref.ARRAY_LOOKS, xref.ARRAY_C)
    w = np.full(R, 1.0 / R)
    y = xref.array_sum(a["offsets"], a["T"], a["I"], q, None, delta, w, np.array([xref.array_t0()]), R, 1, xref.ARRAY_F,
                       sref.inv_sigma(xref.ARRAY_B), xref.ARRAY_DT, xref.ARRAY_NT)[0]
    assert y.shape == (B, xref.ARRAY_NT)
    return y, a, q, delta, w


def check_lloyd_peaks(y, w, delta, received_angle):
    """the two largest local maxima of |y| fall on the closed form's grid points, those lie within half a beamwidth and sigma of
    the geometry at the centre element, and their look angles are `received_angle` (direct, surface) to one look step"""
    closed = xref.array_closed_form(w, delta)
    peaks, want = xref.two_largest_maxima(np.abs(y)), xref.two_largest_maxima(np.abs(closed))
    assert peaks == want, (peaks, want)
    angles, times = xref.array_geometry()
    sigma = sref.pulse_sigma(xref.ARRAY_B)
    step = xref.ARRAY_LOOKS[1] - xref.ARRAY_LOOKS[0]
    assert angles[0] == pytest.approx(-3.43, abs=0.01) and angles[1] == pytest.approx(-7.97, abs=0.01)
    assert times[1] - times[0] == pytest.approx(0.0265, abs=1e-4)
    for (b, m), ang, tim, ra in zip(sorted(peaks, key=lambda bm: bm[1]), angles, times, received_angle):
        look, t = xref.ARRAY_LOOKS[b], xref.array_t0() + m * xref.ARRAY_DT
        assert abs(look - ang) <= 0.5 * xref.ARRAY_BEAMWIDTH and abs(t - tim) <= sigma, (look, ang, t, tim)
        assert abs(look - ra) <= step, (look, ra)
    return peaks


def test_lloyds_mirror_on_the_array_from_the_restatement(lloyd_array):
    y, a, q, delta, w = lloyd_array
    e = xref.array_error(y, w, delta)
    b, m = np.unravel_index(np.argmax(e), e.shape)
    print(f"Lloyd's mirror on the array, restatement on exact straight rays: worst e {e.max():.6e} at look "
          f"{xref.ARRAY_LOOKS[b]} degrees, sample {m}; bound {xref.ARRAY_BOUND:.6e}")
    assert xref.ARRAY_BOUND == 2.0 * xref.ARRAY_MEASURED < 0.01
    assert e.max() <= xref.ARRAY_BOUND                                          # every look and sample: none left out
    assert e.max() == pytest.approx(xref.ARRAY_MEASURED, rel=1e-3)              # the constant is this set-up's value
    assert xref.ARRAY_BEAMWIDTH == pytest.approx(2.86, abs=0.01)
    # the look angles against the product's own received_angle at the centre element: an Arrivals of these arrivals
    R = len(xref.ARRAY_DEPTHS)
    arr = pr.Arrivals(a["offsets"], xref.ARRAY_DEPTHS, np.array([xref.ARRAY_X]), np.array([1]), a["tube"], a["w"], a["T"], a["p"],
                      a["I"], np.linspace(-bp.EXACT_APERTURE, bp.EXACT_APERTURE, bp.EXACT_N), np.full((R, 1), xref.ARRAY_C))
    centre = arr.at(R // 2, 0)
    assert xref.ARRAY_DEPTHS[R // 2] == 500.0 and len(centre["time"]) == 2
    order = np.argsort(centre["time"])                                           # the direct path first
    peaks = check_lloyd_peaks(y, w, delta, centre["received_angle"][order])
    assert np.abs(y[peaks[0]]) > 0.5 / 5009.0                                   # a main lobe holds most of 1 / R1
    # the test's power: the conjugate steering (the other sign convention) puts the peaks at the mirrored looks, a missing
    # surface phase and a missing envelope delay miss the bound
    wrong = xref.array_sum(a["offsets"], a["T"], a["I"], q, None, -delta, w, np.array([xref.array_t0()]), R, 1, xref.ARRAY_F,
                           sref.inv_sigma(xref.ARRAY_B), xref.ARRAY_DT, xref.ARRAY_NT)[0]
    assert sorted(xref.ARRAY_LOOKS[b] for b, _ in xref.two_largest_maxima(np.abs(wrong))) == \
        sorted(-xref.ARRAY_LOOKS[b] for b, _ in peaks)
    assert xref.array_error(wrong, w, delta).max() > 100 * xref.ARRAY_BOUND
    no_phase = xref.array_sum(a["offsets"], a["T"], a["I"], np.zeros_like(q), None, delta, w, np.array([xref.array_t0()]), R, 1,
                              xref.ARRAY_F, sref.inv_sigma(xref.ARRAY_B), xref.ARRAY_DT, xref.ARRAY_NT)[0]
    assert xref.array_error(no_phase, w, delta).max() > 100 * xref.ARRAY_BOUND
    # phase steering alone (every element's own signal turned by exp(-2 pi i f delta), its envelope not delayed)
    u = sref.signal_sum(a["offsets"], a["T"], a["I"], q, np.full(R, xref.array_t0()), xref.ARRAY_F, sref.inv_sigma(xref.ARRAY_B),
                        xref.ARRAY_DT, xref.ARRAY_NT)
    phase_only = np.einsum("j,jb,jn->bn", w, np.exp(-2j * np.pi * xref.ARRAY_F * delta), u)
    assert xref.array_error(phase_only, w, delta).max() > 100 * xref.ARRAY_BOUND


# ---- the API, no GPU ---------------------------------------------------------------------------------------------------------

def test_the_new_names_are_exported_and_the_entry_is_bound_from_its_own_header():
    from pygenray_amd import _lib
    for name in ("steering_delays", "array_response", "beam_array_response"):
        assert name in pr.__all__ and callable(getattr(pr, name))
    assert list(inspect.signature(pr.steering_delays).parameters) == ["receiver_depths", "angles", "sound_speed", "reference_depth"]
    sig = inspect.signature(pr.array_response).parameters
    assert list(sig) == ["rays", "receiver_depths", "env", "angles", "frequency", "bandwidth", "t0", "dt", "n_times", "range_indices",
                         "sound_speed", "reference_depth", "shading", "absorption", "bottom_loss", "surface_loss", "flatearth",
                         "device"]
    beam = inspect.signature(pr.beam_array_response).parameters
    assert list(beam) == list(sig)[:9] + ["min_width", "curvature"] + list(sig)[9:]
    assert beam["min_width"].default == 10.0 and beam["curvature"].default is True
    for s in (sig, beam):
        assert all(s[k].default is None for k in ("range_indices", "sound_speed", "reference_depth", "shading", "absorption",
                                                  "bottom_loss", "surface_loss"))
        assert s["flatearth"].default is True and s["device"].default == 0
    own = _lib.HEADER_PROTOTYPES["pgr_array.h"]
    V, D, I32, I64 = ctypes.c_void_p, ctypes.c_double, ctypes.c_int32, ctypes.c_int64
    assert own == {"pgr_array_response_device": (ctypes.c_int, [ctypes.c_int, V, I64, I64, V, V, V, V, V, V, V, D, D, D, I32, I64,
                                                                V, V, V])}
    assert all("pgr_array_response_device" not in protos for h, protos in _lib.HEADER_PROTOTYPES.items() if h != "pgr_array.h")
    assert _lib.PROTOTYPES["pgr_array_response_device"] == own["pgr_array_response_device"]
    # the wrapper: its name does not end in _device (the table of tests/test_binding_signatures_host.py is about those)
    assert callable(_lib.array_response_sum) and not hasattr(_lib, "array_response_device")
    assert str(inspect.signature(_lib.array_response_sum)) == (
        "(device, offsets_ptr, n_elements, n_cols, t_ptr, i_ptr, q_ptr, phi_ptr, delay_ptr, weight_ptr, tstart_ptr, frequency, "
        "inv_sigma, dt, n_times, n_looks, re_ptr, im_ptr, stream=0)")
    # pgr.h hands the entry to a C caller through the header of its own, behind pgr_beam_arrivals.h
    text = open(_lib.HEADER).read()
    inc = '#include "pgr_array.h"'
    assert text.count(inc) == 1 and text.index('#include "pgr_beam_arrivals.h"') < text.index(inc) < text.rindex("#ifdef __cplusplus")
    header = [h for h in _lib.HEADERS if os.path.basename(h) == "pgr_array.h"]
    assert len(header) == 1 and header[0] in _lib.build_dependencies()
    hip = open(_lib.CSRC + "/pgr_hip.hip").read()
    # (behind pgr_signal.h, whose helpers the kernel uses; pgr_spectrum.h stays the last of the translation unit)
    assert hip.index('#include "pgr_beam_arrivals.h"') < hip.index('#include "pgr_signal.h"') < hip.index('#include "pgr_array.h"')
    assert hip.index('#include "pgr_array.h"') < hip.index('#include "pgr_spectrum.h"')
    assert os.path.join(_lib.CSRC, "pgr_array.h") in _lib.build_dependencies()


def _both(fan=None, depths=(100.0, 200.0), angles=(-5.0, 0.0, 5.0), f=50.0, B=20.0, t0=0.0, dt=1e-3, nt=16, **kw):
    env = pr.OceanEnvironment2D(flat_earth_transform=False)
    fan = _host_fan() if fan is None else fan
    kw = dict(dict(flatearth=False), **kw)
    return [lambda: pr.array_response(fan, list(depths), env, angles, f, B, t0, dt, nt, **kw),
            lambda: pr.beam_array_response(fan, list(depths), env, angles, f, B, t0, dt, nt, **kw)]


def _refused(match, exc=ValueError, **kw):
    for call in _both(**kw):
        with pytest.raises(exc, match=match):
            call()


def test_bad_arguments_are_refused_before_the_device():
    for a in ([], [[0.0]], [np.nan], [np.inf], [90.5], [-91.0]):
        _refused("angles must be", angles=a)
    for s in ([1.0], [1.0, np.nan], [1.0, np.inf], [[0.5, 0.5]]):
        _refused("shading must", shading=s)
    _refused("at least 1 element|non-empty", depths=())
    for c in (0.0, -1500.0, np.nan, [1500.0, 1500.0]):
        _refused("sound_speed must", sound_speed=c)
    _refused("reference_depth must be finite", reference_depth=np.inf)
    # received_signal's own
    for f in (-1.0, np.nan, np.inf):
        _refused("frequency must be finite and >= 0", f=f)
    for B in (-1.0, np.nan, np.inf):
        _refused("bandwidth must be finite and >= 0", B=B)
    for dt in (0.0, -1e-3, np.nan, np.inf):
        _refused("dt must be finite and > 0", dt=dt)
    for nt in (0, -3, 2.5, 65535 * 256 + 1):
        _refused("n_times must be", nt=nt)
    _refused("t0 must be a scalar or one start time per requested column", t0=[0.0, 1.0])
    _refused("t0 must be finite", t0=np.nan)
    _refused("range_indices must lie", range_indices=[5])
    _refused("strictly ascending", depths=(200.0, 100.0))
    _refused("at least 2 rays", fan=_host_fan()[:1])
    _refused("Flat earth transformation has not been applied", flatearth=True)
    _refused("absorption must be finite and >= 0", absorption=-1.0)
    _refused("bounce log", surface_loss=1.0)
    _refused("no bounce log.*max_bounces", fan=_host_fan(n_surfs=[0, 1, 0, 0]))
    for w in (0.0, -1.0, np.nan):
        with pytest.raises(ValueError, match="min_width must be finite and > 0"):
            _both(min_width=w)[1]()
    # a BottomReflection: the tube response takes it (and goes on to miss the bounce log), the beam response refuses it
    b = pr.fluid_halfspace(1700.0, 1800.0, 0.5)
    tube, beam = _both(bottom_loss=b)
    with pytest.raises(ValueError, match="bounce log"):
        tube()
    with pytest.raises(ValueError, match="does not yet apply a complex bottom phase"):
        beam()
    assert math.isfinite(pr.steering_delays([100.0, 200.0], [5.0], 1500.0).sum())
