"""Transfer function over a frequency band and received waveforms without a GPU: the NumPy restatement
(tests/spectrum_reference.py) against the CW sum of tests/signal_reference.py, with a reduction time, in the synthesis identity
that ties received_waveform's three lines to the time-domain sum of a Gaussian pulse, its absorption weight against
10^(-alpha L / 20), and the interface and the argument errors refused before anything reaches the device."""
import inspect
import math
import os
from decimal import Decimal, getcontext

import numpy as np
import pytest

import pygenray_amd as pr

import signal_reference as sref
import spectrum_reference as spref
from test_coherent_host import _host_fan  # noqa: F401  (the hand-made host fan)

SEVEN = (0.0, 50.0, 75.0, 75.37, 95.0, 250.0, 1000.0)


def synthetic_arrivals(seed=18, counts=(0, 17, 200)):
    """seeded groups of 0, 17 and 200 arrivals with T in [60, 62] s, intensities over six decades, q in -1 ... 6"""
    rng = np.random.default_rng(seed)
    off = np.concatenate([[0], np.cumsum(counts)])
    n = int(off[-1])
    T = np.sort(rng.uniform(60.0, 62.0, n))
    I = 10.0 ** rng.uniform(-12.0, -6.0, n)
    q = rng.integers(-1, 7, n).astype(np.int32)
    assert n < 100 or ((q < 0).any() and (q > 3).any())
    return off, T, I, q


def _bits(a, b):
    return np.array_equal(a.real, b.real) and np.array_equal(a.imag, b.imag)


# ---- the restatement against the CW sum -------------------------------------------------------------------------------------

def test_restatement_without_reduction_is_the_cw_sum_bit_for_bit():
    off, T, I, q = synthetic_arrivals()
    G = len(off) - 1
    for qq in (q, None):
        H = spref.spectrum_sum(off, T, I, qq, None, np.zeros(G), SEVEN, None)
        assert H.shape == (G, 7) and (H[0] == 0).all()
        for k, f in enumerate(SEVEN):
            assert _bits(H[:, k], sref.cw_sum(off, T, I, qq, f)), f
    # the order of the frequencies and repeated ones do not matter to an entry
    Hq = spref.spectrum_sum(off, T, I, q, None, np.zeros(G), SEVEN, None)
    H2 = spref.spectrum_sum(off, T, I, q, None, np.zeros(G), SEVEN[::-1] + (75.0,), None)
    assert _bits(H2[:, :7], Hq[:, ::-1]) and _bits(H2[:, 7], H2[:, 4]) and not _bits(Hq, H)


def test_reduction_time_turns_the_cw_sum_by_its_phase():
    off, T, I, q = synthetic_arrivals()
    G = len(off) - 1
    A = spref.group_amplitudes(off, I, q)
    tred = np.array([59.7, 60.0 - 0.119, 58.123456])
    H = spref.spectrum_sum(off, T, I, q, None, tred, SEVEN, None)
    worst = 0.0
    for k, f in enumerate(SEVEN):
        ref = sref.cw_sum(off, T, I, q, f) * np.exp(-2j * np.pi * f * tred)
        err = np.abs(H[:, k] - ref)
        assert (err <= sref.FOURIER_REL * A).all(), (f, err, A)
        worst = max(worst, float((err[A > 0] / (sref.FOURIER_REL * A[A > 0])).max()))
        assert (np.abs(ref[A > 0]) > 100 * sref.FOURIER_REL * A[A > 0]).all()
    print(f"reduction time: worst |H - P e^(-2 pi i f t)| is {worst:.3e} of the bound")
    # ... and a reduction time that is not taken out misses it
    H0 = spref.spectrum_sum(off, T, I, q, None, np.zeros(G), SEVEN, None)
    assert (np.abs(H0[1:, 2] - H[1:, 2]) > 1e4 * sref.FOURIER_REL * A[1:]).all()


# ---- the synthesis identity ---------------------------------------------------------------------------------------------------

def synthesis_case(dt_per_sigma=0.25):
    off, T, I, q = synthetic_arrivals()
    sigma = sref.pulse_sigma(spref.SYNTH_B)
    dt = sigma * dt_per_sigma
    source, tc = spref.gaussian_source(sigma, dt)
    t0, n_fft = spref.covering_fft(60.0, 62.0, sigma, dt, len(source))
    assert t0 == 60.0 - 9.0 * sigma and tc == 9.0 * sigma
    # every arrival, 9 sigma behind it and the source record lie inside the window
    assert t0 + (n_fft - len(source)) * dt >= T.max() + 9.0 * sigma and t0 <= T.min() - 9.0 * sigma
    return off, T, I, q, sigma, dt, source, tc, t0, n_fft


def synthesis_reference(off, T, I, q, sigma, dt, tc, t0, n_fft, f=spref.SYNTH_F):
    G = len(off) - 1
    u = sref.signal_sum(off, T + tc, I, q, np.full(G, t0), f, 1.0 / sigma, dt, n_fft)
    return u * np.exp(-2j * np.pi * f * tc)


def synthesis_ratio(u, ref, off, I, q):
    """the worst |u - ref| over a group's samples in units of the bound SYNTH_REL sum_a amp_a, per group with arrivals"""
    A = spref.group_amplitudes(off, I, q)
    err = np.abs(u - ref).max(axis=-1)
    assert (err[A == 0] == 0).all()
    return err[A > 0] / (spref.SYNTH_REL * A[A > 0])


def test_synthesis_of_a_gaussian_source_is_the_time_domain_sum():
    off, T, I, q, sigma, dt, source, tc, t0, n_fft = synthesis_case()
    G, f = len(off) - 1, spref.SYNTH_F
    assert dt == sigma / 4 and n_fft == 1024 and abs(f * t0 - round(f * t0)) > 0.01

    def H_of(qq):
        return lambda fr, t: spref.spectrum_sum(off, T, I, qq, None, np.full(G, t), fr, None)
    u = spref.waveform(H_of(q), source, dt, f, t0, n_fft)
    ref = synthesis_reference(off, T, I, q, sigma, dt, tc, t0, n_fft)
    ratio = synthesis_ratio(u, ref, off, I, q)
    print(f"synthesis identity, restatement, dt = sigma / 4: worst |u - ref| is {ratio.max():.3e} of the bound "
          f"({n_fft} samples, {len(source)} source samples)")
    assert (ratio <= 1.0).all() and u.shape == (G, n_fft)
    assert (np.abs(ref).max(axis=1)[1:] > 1e6 * spref.SYNTH_REL * spref.group_amplitudes(off, I, q)[1:]).all()
    assert (u[0] == 0).all()
    # n_times keeps the first samples
    assert np.array_equal(spref.waveform(H_of(q), source, dt, f, t0, n_fft, 100), u[:, :100])
    # the test's power: a flipped sign of nu, a missing e^{2 pi i carrier t0} and a missing q all miss the bound
    turn = np.exp(2j * np.pi * (f * t0 - np.rint(f * t0)))
    flipped = spref.waveform(lambda fr, t: H_of(q)(2.0 * f - fr, t), source, dt, f, t0, n_fft)
    no_q = spref.waveform(H_of(np.where(q >= 0, 0, q)), source, dt, f, t0, n_fft)
    for name, wrong in (("nu", flipped), ("turn", u / turn), ("q", no_q)):
        assert (synthesis_ratio(wrong, ref, off, I, q) > 1e3).all(), name


def test_synthesis_at_half_sigma_sampling_is_limited_by_the_sources_aliasing():
    """dt = sigma / 2: the source's own spectrum is e^{-2 pi^2 sigma^2 nu^2} = e^-19.7 at nu = 1 / (2 dt) -- the identity still
    holds within the bound, but not by orders of magnitude (which is why the tests sample at sigma / 4)"""
    off, T, I, q, sigma, dt, source, tc, t0, n_fft = synthesis_case(0.5)
    G = len(off) - 1
    u = spref.waveform(lambda fr, t: spref.spectrum_sum(off, T, I, q, None, np.full(G, t), fr, None), source, dt,
                       spref.SYNTH_F, t0, n_fft)
    ratio = synthesis_ratio(u, synthesis_reference(off, T, I, q, sigma, dt, tc, t0, n_fft), off, I, q)
    print(f"synthesis identity, restatement, dt = sigma / 2: worst |u - ref| is {ratio.max():.3e} of the bound")
    assert 0.02 < ratio.max() <= 1.0


# ---- the absorption weight ----------------------------------------------------------------------------------------------------

def _ulps(got, ref):
    return abs(got - ref) / math.ulp(ref)


def test_absorption_weight_against_ten_to_the_minus_alpha_l_over_twenty():
    """W = gexp(-((alpha L) K20)) against 10^(-alpha L / 20) in 60-digit decimal arithmetic on 1000 seeded arguments, within 2
    ulp.  The argument's two roundings and K20's own (half an ulp of ln 10 / 20) put up to 1.5 |yw| ulp into W and gexp adds
    1.5 ulp of its own (beam_reference.GEXP_ULPS), so 2 ulp is owed for |yw| <= 1/3, alpha L <= 2.9 dB: the arguments are drawn
    from alpha L in [0, 2.5] dB.  Beyond, over the whole range down to the cut, gexp is held within 2 ulp of exp of the
    argument the definition forms."""
    getcontext().prec = 60
    rng = np.random.default_rng(1820)
    L = rng.uniform(1e3, 1.2e6, 1000)
    alpha = rng.uniform(0.0, 2.5, 1000) / L
    W = spref.amplitude_weight(alpha, L)
    ln10 = Decimal(10).ln()
    worst = 0.0
    for a, l, w in zip(alpha, L, W):
        ref = float((-(Decimal(float(a)) * Decimal(float(l))) / 20 * ln10).exp())
        worst = max(worst, _ulps(float(w), ref))
    print(f"W against 10^(-alpha L / 20), alpha L in [0, 2.5] dB: worst {worst:.2f} ulp")
    assert worst <= 2.0 and (W <= 1.0).all() and W.min() < 0.76
    # the whole range of the argument: alpha L up to 6080 dB, yw down to -700
    L2 = rng.uniform(1e3, 1.2e6, 1000)
    a2 = 10.0 ** rng.uniform(-3.0, math.log10(6080.0), 1000) / L2
    yw = -((a2 * L2) * spref.K20)
    assert yw.min() < -600.0 and (yw >= -700.0).all()
    W2 = spref.amplitude_weight(a2, L2)
    worst2 = max(_ulps(float(w), float(Decimal(float(y)).exp())) for y, w in zip(yw, W2))
    print(f"gexp against exp on [-700, 0]: worst {worst2:.2f} ulp")
    assert worst2 <= 2.0 and (W2 > 0).all()
    assert spref.K20 == 0.5 * spref.PATH_LN10_10 and spref.K20 == float(ln10 / 20)


def test_absorption_weight_at_the_cut_at_zero_and_at_nan():
    # yw = -(x * K20) for alpha L = x dB: the cut lies at yw < -700 exactly
    x = 700.0 / spref.K20
    xs = np.array([x * (1 - 1e-15), x * (1 + 1e-15), 1e5, np.inf])
    yw = -(xs * spref.K20)
    assert yw[0] >= -700.0 > yw[1]
    W = spref.amplitude_weight(xs, np.ones(4))
    assert W[0] == pytest.approx(math.exp(-700.0), rel=1e-12) and W[0] > 0 and (W[1:] == 0.0).all()
    assert spref.amplitude_weight(0.0, 5e5) == 1.0 and spref.amplitude_weight(1e-5, 0.0) == 1.0
    assert np.isnan(spref.amplitude_weight(np.nan, 1.0)) and np.isnan(spref.amplitude_weight(1e-5, np.nan))
    # in the sum: a weight of 0 removes the arrival, a NaN L makes the group's entries NaN, alpha = 0 is the sum without
    off, T, I, q = synthetic_arrivals(counts=(3, 2, 1))
    q[:] = [0, 1, 2, 3, 5, 1]
    L = np.array([1e5, 2e5, 1e9, 1e5, np.nan, 5e7])
    freq, alpha = np.array([75.0, 80.0]), np.array([1e-5, 7e-4])
    z = np.zeros(3)
    H = spref.spectrum_sum(off, T, I, q, L, z, freq, alpha)
    two = spref.spectrum_sum(np.array([0, 2]), T[:2], I[:2], q[:2], L[:2], np.zeros(1), freq, alpha)
    assert _bits(H[0], two[0]) and np.isnan(H[1].real).all() and np.isnan(H[1].imag).all()
    assert abs(H[2, 0]) > 0 and H[2, 1] == 0                           # 500 dB: 1e-25 of the amplitude; 35 000 dB: beyond the cut
    H0 = spref.spectrum_sum(off, T, I, q, np.nan_to_num(L), z, freq, np.zeros(2))
    assert _bits(H0, spref.spectrum_sum(off, T, I, q, None, z, freq, None))
    # a NaN T or I does the same, with or without alpha; q < 0 keeps it out
    Tn = T.copy()
    Tn[3] = np.nan
    Hn = spref.spectrum_sum(off, Tn, I, q, None, z, freq, None)
    assert np.isnan(Hn[1].real).all() and not np.isnan(Hn[0].real).any()
    q[3] = -1
    assert not np.isnan(spref.spectrum_sum(off, Tn, I, q, None, z, freq, None).real).any()


def test_arrival_lengths_are_three_separate_operations():
    L0, L1, w = np.array([100000.3, 5.0]), np.array([100007.9, 5.0]), np.array([1.0 / 3.0, 0.7])
    got = spref.arrival_lengths(L0, L1, w)
    assert got[0] == L0[0] + w[0] * (L1[0] - L0[0]) and got[1] == 5.0 and L0[0] < got[0] < L1[0]


# ---- the interface ----------------------------------------------------------------------------------------------------------------

def test_the_new_names_are_exported_and_the_entry_is_bound_from_its_own_header():
    for name in ("transfer_function", "received_waveform"):
        assert name in pr.__all__ and callable(getattr(pr, name))
    sig = inspect.signature(pr.transfer_function).parameters
    assert list(sig) == ["rays", "receiver_depths", "env", "frequencies", "range_indices", "absorption", "bottom_loss",
                         "surface_loss", "t_reduce", "flatearth", "device"]
    assert all(sig[k].default is None for k in ("range_indices", "absorption", "bottom_loss", "surface_loss", "t_reduce"))
    assert sig["flatearth"].default is True and sig["device"].default == 0
    sig = inspect.signature(pr.received_waveform).parameters
    assert list(sig) == ["rays", "receiver_depths", "env", "source", "dt", "carrier", "t0", "n_times", "n_fft", "range_indices",
                         "absorption", "bottom_loss", "surface_loss", "flatearth", "device"]
    assert all(sig[k].default is None for k in ("n_times", "n_fft", "range_indices", "absorption", "bottom_loss", "surface_loss"))
    doc = " ".join(pr.received_waveform.__doc__.split())
    assert "CIRCULAR with the period ``n_fft * dt``" in doc and "wraps around" in doc
    from pygenray_amd import _lib
    own = _lib.HEADER_PROTOTYPES["pgr_spectrum.h"]
    assert len(own) == 1 and len(own["pgr_spectrum_device"][1]) == 14
    for other in [protos for h, protos in _lib.HEADER_PROTOTYPES.items() if h != "pgr_spectrum.h"]:
        assert "pgr_spectrum_device" not in other
    assert callable(_lib.spectrum_device)
    # pgr.h hands the entry to a C caller through the header of its own
    text = open(_lib.HEADER).read()
    assert '#include "pgr_spectrum.h"' in text and text.index('#include "pgr_spectrum.h"') < text.rindex("#ifdef __cplusplus")
    assert text.index('#include "pgr_signal.h"') < text.index('#include "pgr_spectrum.h"')
    # the kernel's header is the last of the translation unit, and the build depends on the ABI header
    hip = open(_lib.CSRC + "/pgr_hip.hip").read()
    assert hip.rstrip().splitlines()[-1].startswith('#include "pgr_spectrum.h"')
    # the header is one of those the binding reads and the build depends on, and load() binds every name of it
    header = [h for h in _lib.HEADERS if os.path.basename(h) == "pgr_spectrum.h"]
    assert len(header) == 1 and os.path.samefile(os.path.dirname(header[0]), os.path.dirname(_lib.HEADER))
    assert header[0] in _lib.build_dependencies()
    assert all(_lib.PROTOTYPES[name] == proto for name, proto in own.items())


# ---- argument errors, no GPU --------------------------------------------------------------------------------------------------

def _tf(fan=None, depths=(100.0,), freq=(50.0, 60.0), **kw):
    env = pr.OceanEnvironment2D(flat_earth_transform=False)
    return pr.transfer_function(_host_fan() if fan is None else fan, list(depths), env, freq,
                                **dict(dict(flatearth=False), **kw))


def _wf(fan=None, depths=(100.0,), source=(1.0, 1.0j, 0.5), dt=1e-3, carrier=600.0, t0=0.0, **kw):
    env = pr.OceanEnvironment2D(flat_earth_transform=False)
    return pr.received_waveform(_host_fan() if fan is None else fan, list(depths), env, source, dt, carrier, t0,
                                **dict(dict(flatearth=False, n_times=8), **kw))


def _pressure_fields_own_errors(call):
    with pytest.raises(ValueError, match="range_indices must lie"):
        call(range_indices=[5])
    with pytest.raises(ValueError, match="strictly ascending"):
        call(depths=(200.0, 100.0))
    with pytest.raises(ValueError, match="at least 2 rays"):
        call(fan=_host_fan()[:1])
    with pytest.raises(ValueError, match="Flat earth transformation has not been applied"):
        call(flatearth=True)
    with pytest.raises(ValueError, match="absorption must be finite and >= 0"):
        call(absorption=-1.0)
    with pytest.raises(ValueError, match="bounce log"):
        call(surface_loss=1.0)
    with pytest.raises(ValueError, match="no bounce log.*max_bounces"):
        call(fan=_host_fan(n_surfs=[0, 1, 0, 0]))


def _callables_errors(call, n):
    """a callable absorption's result is checked: one finite value >= 0 per frequency; its own errors propagate"""
    for bad in (lambda f: 0.01, lambda f: np.zeros(len(f) + 1), lambda f: np.zeros((len(f), 1)), lambda f: np.zeros(0)):
        with pytest.raises(ValueError, match=r"one value in dB/km per frequency"):
            call(absorption=bad)
    for v in (np.nan, np.inf, -0.01):
        with pytest.raises(ValueError, match=r"absorption\(frequencies\) must be finite and >= 0"):
            call(absorption=lambda f: np.full(len(f), v))
    seen = []

    def broken(f):
        seen.append(np.array(f))
        raise KeyError("the caller's own")
    with pytest.raises(KeyError, match="the caller's own"):
        call(absorption=broken)
    assert len(seen) == 1 and seen[0].shape == (n,)


def test_transfer_function_refuses_bad_arguments_before_the_device():
    for freq in (75.0, [[50.0, 60.0]], np.zeros((2, 2))):
        with pytest.raises(ValueError, match="frequencies must be a non-empty 1-D sequence"):
            _tf(freq=freq)
    with pytest.raises(ValueError, match="frequencies must be a non-empty 1-D sequence"):
        _tf(freq=[])
    for bad in (np.nan, np.inf, -np.inf, -1.0):
        with pytest.raises(ValueError, match="frequencies must be finite and >= 0"):
            _tf(freq=[50.0, bad])
    with pytest.raises(ValueError, match="t_reduce must be a scalar or one reduction time per requested column"):
        _tf(t_reduce=[0.0, 1.0])
    with pytest.raises(ValueError, match="t_reduce must be a scalar or one reduction time per requested column"):
        _tf(t_reduce=[0.0, 1.0, 2.0], range_indices=[1, 2])
    for bad in (np.nan, np.inf):
        with pytest.raises(ValueError, match="t_reduce must be finite"):
            _tf(t_reduce=bad)
    _pressure_fields_own_errors(_tf)
    _callables_errors(_tf, 2)
    # thorp_absorption refuses f = 0: its own error
    with pytest.raises(ValueError, match="frequency_hz must be finite and > 0"):
        _tf(freq=[0.0, 50.0], absorption=pr.thorp_absorption)


def test_received_waveform_refuses_bad_arguments_before_the_device():
    for source in (1.0, [], [[1.0, 2.0]]):
        with pytest.raises(ValueError, match="source must be a non-empty 1-D sequence"):
            _wf(source=source)
    for bad in (np.nan, np.inf, complex(0.0, np.nan)):
        with pytest.raises(ValueError, match="source must be finite"):
            _wf(source=[1.0, bad])
    for dt in (0.0, -1e-3, np.nan, np.inf):
        with pytest.raises(ValueError, match="dt must be finite and > 0"):
            _wf(dt=dt)
    # carrier < 1 / (2 dt) would give a negative frequency
    for carrier in (499.0, 0.0, -600.0, np.nan, np.inf):
        with pytest.raises(ValueError, match=r"carrier must be finite and at least 1 / \(2 dt\)"):
            _wf(carrier=carrier)
    with pytest.raises(ValueError, match="n_fft .2. must be at least the length of source .3."):
        _wf(n_fft=2, n_times=1)
    with pytest.raises(ValueError, match="n_times .9. must be <= n_fft .8."):
        _wf(n_fft=8, n_times=9)
    with pytest.raises(ValueError, match="give n_times, n_fft or both"):
        _wf(n_times=None)
    for bad in (0, -4, 2.5, True):
        with pytest.raises(ValueError, match="n_times must be an integer >= 1"):
            _wf(n_times=bad)
        with pytest.raises(ValueError, match="n_fft must be an integer >= 1"):
            _wf(n_fft=bad)
    for bad in (np.nan, np.inf):
        with pytest.raises(ValueError, match="t0 must be finite"):
            _wf(t0=bad)
    with pytest.raises(ValueError, match="must be a scalar or one reduction time per requested column"):
        _wf(t0=[0.0, 1.0])
    _pressure_fields_own_errors(_wf)
    _callables_errors(_wf, 16)                       # n_fft defaults to the next power of two >= n_times + len(source) = 11
    with pytest.raises(ValueError, match="frequency_hz must be finite and > 0"):
        _wf(carrier=500.0, absorption=pr.thorp_absorption)          # the band's lowest frequency is 0


def test_fft_sizes_default_as_documented():
    from pygenray_amd._fan_frame import _fft_sizes
    assert _fft_sizes(73, 751, None) == (751, 1024) and _fft_sizes(24, 1000, None) == (1000, 1024)
    assert _fft_sizes(25, 1000, None) == (1000, 2048) and _fft_sizes(3, None, 64) == (64, 64) and _fft_sizes(3, 5, 7) == (5, 7)
