"""Band-averaged transmission loss without a GPU: the NumPy restatement (tests/band_reference.py) against a reduction of
``spectrum_reference.spectrum_sum`` written apart from it, its identities, Lloyd's mirror over a band on exact straight rays against
the closed form -- on the tube list and on the beam list, with the test's power asserted -- and the API: the exports, the one
prototype in a header of its own and every argument refused before anything reaches the device."""
import ctypes
import inspect
import os

import numpy as np
import pytest

import pygenray_amd as pr

import band_reference as bref
import beam_pressure_reference as bp
import coherent_reference as cref
import reflection_reference as rref
import spectrum_reference as spref
from test_coherent_host import _host_fan
from test_spectrum_host import synthetic_arrivals

NAMES = ("band_intensity", "band_transmission_loss", "beam_band_intensity", "beam_band_transmission_loss")


# ---- the restatement against an independent reduction -------------------------------------------------------------------------

def _independent(H, wf):
    """sum_k wf[k] |H[g, k]|^2 in the defined order, written apart from band_reference: Python floats, the partials of the 64
    residues of k, then a halving tree -- what lane 0 of the xor tree holds, the add being commutative"""
    out = []
    for row in np.asarray(H):
        part = [0.0] * 64
        for k, h in enumerate(row):
            re, im = float(h.real), float(h.imag)
            part[k % 64] = part[k % 64] + float(wf[k]) * (re * re + im * im)
        n = 64
        while n > 1:
            n //= 2
            part = [part[i] + part[i + n] for i in range(n)]
        out.append(part[0])
    return np.array(out)


def _weights(F, seed):
    """unequal weights with an exact 0.0 (F > 1)"""
    w = np.random.default_rng(seed).uniform(0.1, 2.0, F)
    if F > 1:
        w[F // 3] = 0.0
    return w


@pytest.mark.parametrize("F", [1, 63, 64, 65, 130, 257])
def test_restatement_is_the_defined_reduction_of_the_spectrum_sum_bit_for_bit(F):
    off, T, I, q = synthetic_arrivals(seed=23 + F)
    G = len(off) - 1
    rng = np.random.default_rng(F)
    assert (q < 0).any() and (q > 3).any()
    freq = np.linspace(60.0, 90.0, F) if F > 1 else np.array([75.0])
    wf = _weights(F, F)
    assert F == 1 or ((wf == 0).sum() == 1 and len(set(wf.tolist())) == F)
    L = rng.uniform(1e4, 1.2e6, len(T))
    alpha = rng.uniform(1e-6, 1e-5, F)
    lags = {"none": None, "zero": np.zeros(len(T)), "whole": rng.integers(-1000, 1001, len(T)).astype(float),
            "general": rng.uniform(-3.0, 3.0, len(T))}
    zero = np.zeros(G)
    seen = {}
    for qname, qq in (("q", q), ("null", None)):
        for lname, phi in lags.items():
            for LL, aa in ((None, None), (L, alpha)):
                out = bref.band_power(off, T, I, qq, phi, LL, freq, aa, wf)
                H = (spref.spectrum_sum(off, T, I, qq, LL, zero, freq, aa) if phi is None else
                     rref.spectrum_sum(off, T, I, qq, phi, LL, zero, freq, aa))
                assert out.shape == (G,) and out.dtype == np.float64
                assert np.array_equal(out, _independent(H, wf)), (qname, lname, aa is not None)
                assert out[0] == 0.0 and not np.signbit(out[0]) and (out[1:] > 0).all()      # the empty group: +0.0
                seen[qname, lname, aa is not None] = out
    # a zero lag and whole cycles leave every bit alone; a general lag, q and the absorption matter
    for key in (("q", False), ("q", True), ("null", False)):
        none = seen[key[0], "none", key[1]]
        assert np.array_equal(seen[key[0], "zero", key[1]], none) and np.array_equal(seen[key[0], "whole", key[1]], none)
        assert not np.array_equal(seen[key[0], "general", key[1]], none)
    assert not np.array_equal(seen["q", "none", False], seen["null", "none", False])
    assert not np.array_equal(seen["q", "none", True][1:], seen["q", "none", False][1:])
    # the weights enter linearly and the zero weight drops its frequency
    if F > 1:
        k = F // 3
        H = spref.spectrum_sum(off, T, I, q, None, zero, freq, None)
        other = H.copy()
        other[:, k] = 1e3
        assert np.array_equal(bref.reduce_band(other.real, other.imag, wf), seen["q", "none", False])


def test_one_frequency_with_weight_one_is_the_squared_field_and_an_empty_group_is_plus_zero():
    zs, ps, ts, x, p0, q = bp.exact_fan(bp.LLOYD_ZS)
    off, T, I, qa = bref.exact_tube_lists()
    assert (np.diff(off) == 2).all() and set(qa.tolist()) == {0, 2}
    for f in (50.0, 75.37):
        re, im = cref.tube_pressure(zs, ps, ts, x, p0, bp.LLOYD_DEPTHS, bp.EXACT_CIN, bp.EXACT_RIN, bp.EXACT_ZIN, None, q, f)
        re, im = re[:, 1:], im[:, 1:]
        out = bref.as_cells(bref.band_power(off, T, I, qa, None, None, [f], None, [1.0]))
        assert np.array_equal(out, re * re + im * im) and (out > 0).all()
    # groups without arrivals, and arrivals that add nothing
    out = bref.band_power([0, 0, 2, 2], T[:2], I[:2], None, None, None, bref.BAND_FREQ, None, bref.BAND_UNIFORM)
    assert out[0] == 0.0 and out[2] == 0.0 and not np.signbit(out[[0, 2]]).any() and out[1] > 0
    out = bref.band_power([0, 2], T[:2], I[:2], [-1, -1], None, None, bref.BAND_FREQ, None, bref.BAND_UNIFORM)
    assert out[0] == 0.0 and not np.signbit(out[0])
    # a NaN T, I or lag makes the group NaN
    for nanT, nanI, nanphi in ((np.nan, 1e-8, 0.0), (60.0, np.nan, 0.0), (60.0, 1e-8, np.nan)):
        out = bref.band_power([0, 1, 2], [nanT, 60.5], [nanI, 1e-8], None, [nanphi, 0.0], None, bref.BAND_FREQ, None,
                              bref.BAND_UNIFORM)
        assert np.isnan(out[0]) and out[1] > 0


# ---- Lloyd's mirror over a band -----------------------------------------------------------------------------------------------

def check_lloyd_band(P, measured, what):
    """every cell of a band power P (len(LLOYD_DEPTHS), 4) under uniform weights within twice the measured constant of the
    closed form -> the worst e"""
    e = bref.lloyd_band_error(P, bref.BAND_UNIFORM)
    j, c = np.unravel_index(np.argmax(e), e.shape)
    print(f"Lloyd's mirror over 60 ... 90 Hz, {what}: worst e {e.max():.16e} at {bp.LLOYD_DEPTHS[j]} m, {bp.EXACT_RANGES[c]} m; "
          f"bound {2.0 * measured:.6e}")
    assert e.shape == (18, 4) and e.max() <= 2.0 * measured                       # every cell: none left out
    return float(e.max())


def test_the_lloyd_receivers_lie_inside_the_aperture_of_both_paths():
    """section 20's premise: the direct path covers depths up to z_s + r tan 40, the reflected one up to r tan 40 - z_s, and the
    receivers lie four sigma of the widest beam inside the narrower of the two at every range"""
    edge = np.tan(np.radians(bp.EXACT_APERTURE)) * bp.EXACT_RANGES
    reach = 4.0 * bp.widest_beam(bp.LLOYD_ZS, 10.0)
    assert (bp.LLOYD_DEPTHS.max() + reach <= edge - bp.LLOYD_ZS).all() and (edge > bp.LLOYD_ZS).all()
    assert len(bref.BAND_FREQ) == 64 and bref.BAND_FREQ[0] == 60.0 and bref.BAND_FREQ[-1] == 90.0
    assert (bref.BAND_UNIFORM == 1.0 / 64).all()


@pytest.mark.parametrize("which", ["tubes", "beams"])
def test_lloyds_mirror_over_a_band_from_the_restatement(which):
    off, T, I, q = bref.exact_tube_lists() if which == "tubes" else bref.exact_beam_lists(10.0, True)
    measured = bref.BAND_LLOYD_MEASURED if which == "tubes" else bref.BAND_LLOYD_BEAM_MEASURED
    assert set(q.tolist()) == {0, 2}                                               # folded tubes are left out
    P = bref.as_cells(bref.band_power(off, T, I, q, None, None, bref.BAND_FREQ, None, bref.BAND_UNIFORM))
    worst = check_lloyd_band(P, measured, f"restatement on the exact straight rays' {which}")
    assert worst == pytest.approx(measured, rel=1e-6) and 2.0 * measured < 1e-3    # the constant is this set-up's value
    bound = 2.0 * measured
    # the test's power: each of these misses the bound by more than 100 x
    R1, R2 = bref.lloyd_paths()
    incoherent = 1.0 / R1 ** 2 + 1.0 / R2 ** 2
    assert bref.lloyd_band_error(incoherent, bref.BAND_UNIFORM).max() > 100 * bound
    shaped = bref.spectrum_shaped_weights()
    Pw = bref.as_cells(bref.band_power(off, T, I, q, None, None, bref.BAND_FREQ, None, shaped))
    e_shaped = bref.lloyd_band_error(Pw, shaped).max()
    print(f"  with the source spectrum's weights: worst e {e_shaped:.6e}")
    assert e_shaped <= bound                                                       # the weights used as given ...
    assert bref.lloyd_band_error(P, shaped).max() > 100 * bound                    # ... and ignored
    no_phase = bref.as_cells(bref.band_power(off, T, I, np.where(q == 2, 0, q), None, None, bref.BAND_FREQ, None,
                                             bref.BAND_UNIFORM))
    assert bref.lloyd_band_error(no_phase, bref.BAND_UNIFORM).max() > 100 * bound


# ---- the API, no GPU ----------------------------------------------------------------------------------------------------------

def test_the_new_names_are_exported_and_the_entry_is_bound_from_its_own_header():
    from pygenray_amd import _lib
    for name in NAMES:
        assert name in pr.__all__ and callable(getattr(pr, name))
    sig = inspect.signature(pr.band_intensity).parameters
    assert list(sig) == ["rays", "receiver_depths", "env", "frequencies", "weights", "range_indices", "absorption", "bottom_loss",
                         "surface_loss", "flatearth", "device"]
    assert list(inspect.signature(pr.band_transmission_loss).parameters) == list(sig)
    beam = inspect.signature(pr.beam_band_intensity).parameters
    assert list(beam) == list(sig)[:5] + ["min_width", "curvature"] + list(sig)[5:]
    assert list(inspect.signature(pr.beam_band_transmission_loss).parameters) == list(beam)
    assert beam["min_width"].default == 10.0 and beam["curvature"].default is True
    for s in (sig, beam):
        assert all(s[k].default is None for k in ("weights", "range_indices", "absorption", "bottom_loss", "surface_loss"))
        assert s["flatearth"].default is True and s["device"].default == 0
    own = _lib.HEADER_PROTOTYPES["pgr_band.h"]
    V, I32, I64 = ctypes.c_void_p, ctypes.c_int32, ctypes.c_int64
    assert own == {"pgr_band_power_device": (ctypes.c_int, [ctypes.c_int, V, I64, V, V, V, V, V, V, V, V, I32, V, V])}
    assert all("pgr_band_power_device" not in protos for h, protos in _lib.HEADER_PROTOTYPES.items() if h != "pgr_band.h")
    assert _lib.PROTOTYPES["pgr_band_power_device"] == own["pgr_band_power_device"]
    # the wrapper: its name does not end in _device (the table of tests/test_binding_signatures_host.py is about those)
    assert callable(_lib.band_power_sum) and not hasattr(_lib, "band_power_device")
    assert str(inspect.signature(_lib.band_power_sum)) == (
        "(device, offsets_ptr, n_groups, t_ptr, i_ptr, q_ptr, phi_ptr, l_ptr, freq, alpha, weights, out_ptr, stream=0)")
    # pgr.h hands the entry to a C caller through the header of its own, behind pgr_array.h
    text = open(_lib.HEADER).read()
    inc = '#include "pgr_band.h"'
    assert text.count(inc) == 1 and text.index('#include "pgr_array.h"') < text.index(inc) < text.rindex("#ifdef __cplusplus")
    header = [h for h in _lib.HEADERS if os.path.basename(h) == "pgr_band.h"]
    assert len(header) == 1 and header[0] in _lib.build_dependencies() and _lib.HEADERS[-1] == header[0]
    # the kernel's header stands before pgr_spectrum.h, which it includes itself, and behind the helpers both use
    hip = open(_lib.CSRC + "/pgr_hip.hip").read()
    assert hip.count(inc) == 1
    assert hip.index('#include "pgr_reflect.h"') < hip.index('#include "pgr_array.h"') < hip.index(inc) < \
        hip.index('#include "pgr_spectrum.h"')
    kernel = open(os.path.join(_lib.CSRC, "pgr_band.h")).read()
    assert kernel.index('#include "pgr_spectrum.h"') < kernel.index("struct BandArgs")
    assert os.path.join(_lib.CSRC, "pgr_band.h") in _lib.build_dependencies()


def _all_four(fan=None, depths=(100.0, 200.0), freq=(50.0, 60.0, 70.0), **kw):
    env = pr.OceanEnvironment2D(flat_earth_transform=False)
    fan = _host_fan() if fan is None else fan
    kw = dict(dict(flatearth=False), **kw)
    beam_kw = {k: kw.pop(k) for k in ("min_width", "curvature") if k in kw}
    return ([lambda n=n: getattr(pr, n)(fan, list(depths), env, freq, **kw) for n in NAMES[:2]] +
            [lambda n=n: getattr(pr, n)(fan, list(depths), env, freq, **kw, **beam_kw) for n in NAMES[2:]])


def _refused(match, exc=ValueError, **kw):
    for call in _all_four(**kw):
        with pytest.raises(exc, match=match):
            call()


def test_bad_arguments_are_refused_before_the_device():
    for freq in (75.0, [[50.0, 60.0]], np.zeros((2, 2)), []):
        _refused("frequencies must be a non-empty 1-D sequence", freq=freq)
    for bad in (np.nan, np.inf, -np.inf, -1.0):
        _refused("frequencies must be finite and >= 0", freq=[50.0, bad, 70.0])
    for w in (1.0, [1.0], [1.0, 1.0], [[1.0, 1.0, 1.0]], np.ones(4)):
        _refused(r"weights must hold one weight per frequency \(3\)", weights=w)
    for bad in (np.nan, np.inf, -np.inf, -1e-300):
        _refused("weights must be finite and >= 0", weights=[1.0, bad, 1.0])
    _refused("weights must not all be zero", weights=[0.0, 0.0, 0.0])
    # a callable absorption's result is checked; its own errors propagate
    for bad in (lambda f: 0.01, lambda f: np.zeros(len(f) + 1), lambda f: np.zeros((len(f), 1))):
        _refused("one value in dB/km per frequency", absorption=bad)
    for v in (np.nan, np.inf, -0.01):
        _refused(r"absorption\(frequencies\) must be finite and >= 0", absorption=lambda f, v=v: np.full(len(f), v))

    def broken(f):
        raise KeyError("the caller's own")
    _refused("the caller's own", exc=KeyError, absorption=broken)
    _refused("frequency_hz must be finite and > 0", freq=[0.0, 50.0, 60.0], absorption=pr.thorp_absorption)
    # transfer_function's own
    _refused("range_indices must lie", range_indices=[5])
    _refused("strictly ascending", depths=(200.0, 100.0))
    _refused("non-empty", depths=())
    _refused("at least 2 rays", fan=_host_fan()[:1])
    _refused("Flat earth transformation has not been applied", flatearth=True)
    _refused("absorption must be finite and >= 0", absorption=-1.0)
    _refused("bounce log", surface_loss=1.0)
    _refused("no bounce log.*max_bounces", fan=_host_fan(n_surfs=[0, 1, 0, 0]))
    for w in (0.0, -1.0, np.nan):
        for call in _all_four(min_width=w)[2:]:
            with pytest.raises(ValueError, match="min_width must be finite and > 0"):
                call()
    # a BottomReflection: the tube products take it (and go on to miss the bounce log), the beam products refuse it
    calls = _all_four(bottom_loss=pr.fluid_halfspace(1700.0, 1800.0, 0.5))
    for call in calls[:2]:
        with pytest.raises(ValueError, match="bounce log"):
            call()
    for call in calls[2:]:
        with pytest.raises(ValueError, match="does not yet apply a complex bottom phase"):
            call()


def test_the_wrapper_refuses_sequences_of_unequal_length_before_the_library():
    from pygenray_amd import _lib
    with pytest.raises(ValueError, match="equal length"):
        _lib.band_power_sum(0, 0, 1, 0, 0, 0, 0, 0, [50.0, 60.0], None, [1.0], 0)
    with pytest.raises(ValueError, match="equal length"):
        _lib.band_power_sum(0, 0, 1, 0, 0, 0, 0, 0, [50.0, 60.0], [1e-6], [1.0, 1.0], 0)
