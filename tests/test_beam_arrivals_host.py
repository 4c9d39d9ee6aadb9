"""beam_arrivals and the sums over them without a GPU: the NumPy restatement of
tests/beam_arrivals_reference.py tied bit for bit to beam_pressure_reference.beam_pressure through the restated sums of
sections 17 and 18, Lloyd's mirror with a pulse against the two-path closed form, the caustic bound for a pulse, the boundary
strip the tubes leave empty, and the exports, signatures, prototypes and refusals of the new functions.  The value measured
here is the one beam_arrivals_reference.py and DESIGN.md record; its bound is twice it."""
import ctypes
import inspect
import os

import numpy as np
import pytest

import pygenray_amd as pr

import beam_arrivals_reference as ba
import beam_pressure_reference as bp
import coherent_reference as cref
import signal_reference as sref
import spectrum_reference as spref
import wave_reference as wref
from test_beam_pressure import synthetic_phase
from test_beam_pressure_host import _caustic_rows
from test_coherent_host import _host_fan
from test_coherent_wave_host import _guide_fan
from tube_gpu import SYN_R, SYN_Z, syn_cin, synthetic_fan

TIE_F = (0.0, 50.0, 1e4)


def _same(a, b):
    return np.array_equal(a, b, equal_nan=True)


# ---- the tie to the restatement of section 20, bit for bit -----------------------------------------------------------------------

def _tie(zs, ps, ts, x, p0, depths, tab, bottom, w_min, W, q, cols, curvature):
    """every identity of the tie on one input -> the arrival dict"""
    a = ba.beam_arrivals(zs, ps, ts, x, p0, depths, *tab, bottom, w_min, W, q, cols, curvature)
    off, n, R = a["offsets"], len(cols), len(depths)
    # the preconditions of sqrt(fl(a a)) == a and of a term that the sums and the field treat alike
    assert ba.no_subnormal_squares(a["amplitude"]) and not np.isnan(a["time"]).any()
    I = a["amplitude"] * a["amplitude"]
    assert _same(np.sqrt(I), a["amplitude"])
    lit = (x != x[0])[np.asarray(cols)]
    H = spref.spectrum_sum(off, a["time"], I, a["q"], None, np.zeros(R * n), np.array(TIE_F), None).reshape(R, n, len(TIE_F))
    for i, f in enumerate(TIE_F):
        re, im, _, _, detail = bp.beam_pressure(zs, ps, ts, x, p0, depths, *tab, bottom, w_min, W, q, f, curvature, detail=True)
        ref = cref.as_complex(re, im)[:, cols]
        assert np.isnan(ref[:, ~lit]).all() and not np.isnan(ref[:, lit]).any()
        assert _same(H[:, lit, i].real, ref[:, lit].real) and _same(H[:, lit, i].imag, ref[:, lit].imag), f
        u = sref.signal_sum(off, a["time"], I, a["q"], np.zeros(R * n), f, 0.0, 1.0, 2).reshape(R, n, 2)
        for k in range(2):
            assert _same(u[:, lit, k].real, ref[:, lit].real) and _same(u[:, lit, k].imag, ref[:, lit].imag), f
    counts = np.diff(off).reshape(R, n)
    assert np.array_equal(counts.sum(axis=0), detail["kept"].sum(axis=(0, 1))[cols])
    assert (counts[:, ~lit] == 0).all() and counts[:, lit].sum() > 0
    return a


@pytest.mark.parametrize("curvature", [True, False])
@pytest.mark.parametrize("weighted", [True, False])
def test_the_list_summed_is_the_field_on_the_synthetic_fan(curvature, weighted):
    M, S, R = 200, 5, 70
    cin = syn_cin()
    z, p, x, p0, depths = synthetic_fan(M, S, R, seed=77, cin=cin)
    t, W, q = synthetic_phase(M, S, 78)
    bottom = np.linspace(4700.0, 5150.0, S)
    cols = [4, 1, 0, 3, 2, 2]
    tab = (cin, SYN_R, SYN_Z)
    a = ba.beam_arrivals(z.T, p.T, t.T, x, p0, depths, *tab, bottom, 25.0, W.T if weighted else None, q.T, cols, curvature)
    if np.isnan(a["time"]).any():
        # the synthetic fan's one NaN travel time lands in a kept term: taken out of the INPUT (the sums skip a NaN delay, the
        # field adds it); no output is filtered and no case is left out
        assert np.isnan(t).sum() == 1
        t = np.where(np.isnan(t), 1.0, t)
    a = _tie(z.T, p.T, t.T, x, p0, depths, tab, bottom, 25.0, W.T if weighted else None, q.T, cols, curvature)
    assert set(np.unique(a["image"])) == {0, 1, 2} and set(np.unique(a["q"])) == {0, 1, 2, 3}
    assert (a["amplitude"] >= 0).all() and (a["amplitude"] <= a["cap"]).all()


def test_the_list_summed_is_the_field_on_the_exact_lloyd_fan():
    zs, ps, ts, x, p0, q = bp.exact_fan(bp.LLOYD_ZS)
    tab = (bp.EXACT_CIN, bp.EXACT_RIN, bp.EXACT_ZIN)
    a = _tie(zs, ps, ts, x, p0, bp.LLOYD_DEPTHS, tab, np.full(len(x), bp.EXACT_BOTTOM), 10.0, None, q, [1, 2, 3, 4, 0], True)
    per = np.diff(a["offsets"]).reshape(len(bp.LLOYD_DEPTHS), 5)[:, :4]
    print(f"exact Lloyd fan, min_width 10 m: {per.min()} ... {per.max()} beam arrivals per receiver and range (mean {per.mean():.1f})")
    # (the receivers lie 4 sigma clear of the surface and the bottom is out of reach: the reflected path arrives as folded rays)
    assert set(np.unique(a["image"])) == {0} and set(np.unique(a["q"])) == {0, 2}


# ---- Lloyd's mirror with a pulse ----------------------------------------------------------------------------------------------

def test_the_closed_form_is_signal_references():
    """lloyd_pulse_error with coherent_reference's source, receivers and frequency is signal_reference's, value for value"""
    rng = np.random.default_rng(3)
    x = np.array([1e3, 3e3, 5e3])
    u = (rng.normal(size=(len(cref.LLOYD_DEPTHS), 3, sref.LLOYD_NT)) + 1j * rng.normal(size=(len(cref.LLOYD_DEPTHS), 3, sref.LLOYD_NT))) * 1e-4
    mine = ba.lloyd_pulse_error(u, x, source_depth=cref.LLOYD_ZS, depths=cref.LLOYD_DEPTHS, f=cref.LLOYD_F, c=cref.LLOYD_C,
                                B=sref.LLOYD_B)
    assert np.array_equal(mine, sref.lloyd_pulse_error(u, x))
    assert (ba.PULSE_F, ba.PULSE_B) == (75.0, 20.0) and bp.EXACT_C == cref.LLOYD_C


def test_lloyds_mirror_with_a_pulse_on_exact_rays():
    a = ba.exact_lloyd_arrivals(10.0, True)
    u = ba.pulse_of(a, bp.EXACT_RANGES)
    e = ba.lloyd_pulse_error(u, bp.EXACT_RANGES)
    # both pulses lie inside every time axis: the reflected path's delay and 8 sigma behind it
    R2 = np.hypot(bp.EXACT_RANGES[None, :], bp.LLOYD_DEPTHS[:, None] + bp.LLOYD_ZS)
    late = (R2 - bp.EXACT_RANGES[None, :]) / bp.EXACT_C + sref.LLOYD_LEAD + 8.0 * sref.pulse_sigma(ba.PULSE_B)
    assert late.max() < (sref.LLOYD_NT - 1) * sref.LLOYD_DT and sref.LLOYD_LEAD > 8.0 * sref.pulse_sigma(ba.PULSE_B)
    assert np.abs(u).max() > 1e-4
    print(f"Lloyd's mirror with a {ba.PULSE_F} Hz / {ba.PULSE_B} Hz pulse on exact rays, min_width 10 m: worst e per range "
          f"{[f'{v:.4e}' for v in e.max(axis=(0, 2))]} (worst {e.max()!r}); bound {ba.LLOYD_PULSE_BOUND:.4e}")
    assert e.max() <= ba.LLOYD_PULSE_BOUND
    assert e.max() == pytest.approx(ba.LLOYD_PULSE_MEASURED, rel=1e-3)             # the constant is this fan's value
    assert ba.LLOYD_PULSE_BOUND == 2.0 * ba.LLOYD_PULSE_MEASURED


# ---- a caustic stays bounded for a pulse ----------------------------------------------------------------------------------------

@pytest.mark.parametrize("curvature", [True, False])
def test_a_caustic_stays_bounded_for_a_pulse(curvature):
    zs, ps, ts, x, p0, depths = _caustic_rows(1e-6)
    tab = (bp.EXACT_CIN, bp.EXACT_RIN, bp.EXACT_ZIN)
    a = ba.beam_arrivals(zs, ps, ts, x, p0, depths, *tab, np.full(2, bp.EXACT_BOTTOM), 10.0, None, None, [1], curvature)
    assert len(a["tube"]) > 3 and 10 in a["tube"]
    u = ba.pulse_of(a, x[1:])[0, 0]
    bound = a["amplitude"].sum() * (1.0 + 1e-12)
    assert (np.abs(u) <= bound).all() and np.abs(u).max() > 0.1 * bound           # the triangle inequality, and nearly reached
    # the tube restatement on the same rows: its peak is the spike
    th = np.degrees(np.arcsin(p0 * 1500.0))
    fan = pr.RayFan.from_arrays(th, np.tile(x, (len(th), 1)), ts, zs, ps, np.zeros(len(th), np.int64), np.zeros(len(th), np.int64),
                                np.full(len(th), 1000.0))
    off, T, I, q = sref.fan_arrivals(fan, depths, cref.lloyd_env(pr), [1], flatearth=False)
    assert off[-1] == 1 and (q == 0).all()
    tube = sref.signal_sum(off, T, I, q, x[1:] / 1500.0 - sref.LLOYD_LEAD, ba.PULSE_F, sref.inv_sigma(ba.PULSE_B), sref.LLOYD_DT,
                           sref.LLOYD_NT)
    print(f"a tube 1e-6 m wide at the receiver, curvature {curvature}: pulse peak {np.abs(tube).max():.4e} from the tube, "
          f"{np.abs(u).max():.4e} from the beams, sum of amplitudes {a['amplitude'].sum():.4e}")
    assert np.abs(tube).max() > 100.0 * np.abs(u).max()


# ---- beams reach where tubes do not -------------------------------------------------------------------------------------------

def test_beams_reach_the_boundary_strip_the_tubes_leave_empty():
    fan, env, nb, ns, o = _guide_fan(wref.GUIDE_N)
    cols = wref.GUIDE_COLS
    strip = wref.guide_strip(o["r"])
    near = np.array([0.1, 0.25, 0.5, 1.0, 2.0, 4.0])
    depths = np.concatenate([near, wref.GUIDE_H - near[::-1]])
    assert (np.minimum(depths, wref.GUIDE_H - depths) < strip).all()
    off, T, I, q = sref.fan_arrivals(fan, depths, env, cols, flatearth=False, nb=nb, ns=ns)
    adds = np.concatenate([[0], np.cumsum(q >= 0)])
    tubes = (adds[off[1:]] - adds[off[:-1]]).reshape(len(depths), len(cols))       # the tube arrivals that add, per group
    a = ba.fan_beam_arrivals(fan, depths, env, cols, w_min=10.0, flatearth=False, nb=nb, ns=ns)
    beams = np.diff(a["offsets"]).reshape(len(depths), len(cols))
    # The tube arrival count is 0 in the plain sense -- no tube holds the receiver at all -- and, no weaker here, in the sense
    # of the sums: no tube that adds (a tube folded over the boundary is listed with q < 0 and adds nothing).  The strip's other
    # receivers are reached by some tubes and miss others; the groups below are the ones the tubes leave quite empty, all at
    # the fan's last column, where no reflected segment continued backwards fills the strip.
    listed = np.diff(off).reshape(len(depths), len(cols))
    none, empty = listed == 0, tubes == 0
    print(f"waveguide, {len(depths)} receivers within {strip:.1f} m of a boundary x {len(cols)} ranges: {int(none.sum())} groups "
          f"without any tube arrival, {int(empty.sum())} without one that adds; beam arrivals there {beams[empty].min()} ... "
          f"{beams[empty].max()}")
    assert none.sum() >= 1 and (beams[none] > 0).all() and not (none & ~empty).any()
    assert np.array_equal(none, empty) and (beams[empty] > 0).all()
    assert set(np.unique(a["image"])) <= {0, 1, 2} and {1, 2} <= set(np.unique(a["image"]))
    assert (a["amplitude"] >= 0).all() and (a["amplitude"] <= a["cap"]).all()


# ---- exports, signatures, prototypes, refusals -----------------------------------------------------------------------------------

NEW = ("beam_arrivals", "BeamArrivals", "beam_received_signal", "beam_transfer_function", "beam_received_waveform")


def _with_beam_arguments(sibling, after):
    names = list(inspect.signature(sibling).parameters)
    i = names.index(after) + 1
    return names[:i] + ["min_width", "curvature"] + names[i:]


def test_the_new_functions_are_exported_with_their_siblings_arguments():
    for name in NEW:
        assert name in pr.__all__ and callable(getattr(pr, name))
    sig = inspect.signature(pr.beam_arrivals).parameters
    assert list(sig) == ["rays", "receiver_depths", "env", "min_width", "curvature", "range_indices", "absorption", "bottom_loss",
                         "surface_loss", "flatearth", "device"]
    assert [sig[k].default for k in list(sig)[3:]] == [10.0, True, None, None, None, None, True, 0]
    for beam, sibling, after in ((pr.beam_received_signal, pr.received_signal, "n_times"),
                                 (pr.beam_transfer_function, pr.transfer_function, "frequencies"),
                                 (pr.beam_received_waveform, pr.received_waveform, "n_fft")):
        got = inspect.signature(beam).parameters
        assert list(got) == _with_beam_arguments(sibling, after)
        assert got["min_width"].default == 10.0 and got["curvature"].default is True
        for k, v in inspect.signature(sibling).parameters.items():
            assert got[k].default == v.default or (got[k].default is v.default)
    b = pr.BeamArrivals(np.array([0, 2, 3]), np.array([5.0]), np.array([1e3, 2e3]), np.array([1, 2]), np.array([4, 4, 7], np.int32),
                        np.array([0, 1, 0], np.int32), np.array([1.0, 1.1, 2.0]), np.array([0.5, 0.25, 2.0]),
                        np.array([0, 2, 1], np.int32))
    assert len(b) == 3 and "3 arrivals at 1 receiver depths x 2 ranges" in repr(b)
    assert np.array_equal(b.intensity, [0.25, 0.0625, 4.0]) and b.intensity is b.intensity
    assert np.array_equal(b.at(0, 1)["tube"], [7]) and np.array_equal(b.at(0, 0)["image"], [0, 1])
    assert set(b.at(0, 0)) == {"tube", "image", "time", "amplitude", "phase_index", "intensity"}
    with pytest.raises(IndexError):
        b.at(1, 0)


def test_the_four_entries_are_bound_from_a_header_of_their_own():
    from pygenray_amd import _lib
    own = _lib.HEADER_PROTOTYPES["pgr_beam_arrivals.h"]
    assert len(own) == 4
    V, D, I32, I64 = ctypes.c_void_p, ctypes.c_double, ctypes.c_int32, ctypes.c_int64
    fan_head, buf_head = [V, V, V, V], [V, V, V, V, I64, I32, V, V, V, V]
    counts, emit = [V, V, I64, D, V, I32, V, V], [V, V, I64, D, V, I32, I32, V, I64, V, V, V, V, V, V]
    assert own == {
        "pgr_fan_beam_arrival_counts_w": (ctypes.c_int, fan_head + counts),
        "pgr_fan_beam_arrivals_w": (ctypes.c_int, fan_head + emit),
        "pgr_beam_arrival_counts_device_w": (ctypes.c_int, buf_head + counts),
        "pgr_beam_arrivals_device_w": (ctypes.c_int, buf_head + emit)}
    for name in own:
        for other in [protos for h, protos in _lib.HEADER_PROTOTYPES.items() if h != "pgr_beam_arrivals.h"]:
            assert name not in other
    for name in ("beam_arrival_counts", "beam_arrivals"):
        assert callable(getattr(_lib, name + "_device")) and callable(getattr(_lib.FanHandle, name))
    text = open(_lib.HEADER).read()
    inc = '#include "pgr_beam_arrivals.h"'
    assert text.count(inc) == 1 and text.index('#include "pgr_beam_coherent.h"') < text.index(inc) < text.rindex("#ifdef __cplusplus")
    hip = open(_lib.CSRC + "/pgr_hip.hip").read()
    assert hip.index('#include "pgr_beam_phase.h"') < hip.index('#include "pgr_beam_arrivals.h"')
    # the header is one of those the binding reads and the build depends on, and load() binds every name of it
    header = [h for h in _lib.HEADERS if os.path.basename(h) == "pgr_beam_arrivals.h"]
    assert len(header) == 1 and os.path.samefile(os.path.dirname(header[0]), os.path.dirname(_lib.HEADER))
    assert header[0] in _lib.build_dependencies()
    assert all(_lib.PROTOTYPES[name] == proto for name, proto in own.items())
    # a host fan's ts go to both entries, with its zs and ps
    from pygenray_amd._fan_frame import _entry_takes
    for name in ("beam_arrival_counts", "beam_arrivals"):
        assert _entry_takes(name) == (("ts", "zs", "ps"), True)


def _all_four(fan, env, depths=(100.0,), **kw):
    src = np.ones(4, complex)
    return [lambda: pr.beam_arrivals(fan, depths, env, flatearth=False, **kw),
            lambda: pr.beam_received_signal(fan, depths, env, 75.0, 20.0, 0.0, 1e-3, 8, flatearth=False, **kw),
            lambda: pr.beam_transfer_function(fan, depths, env, [50.0, 60.0], flatearth=False, **kw),
            lambda: pr.beam_received_waveform(fan, depths, env, src, 1e-3, 600.0, 0.0, n_fft=8, flatearth=False, **kw)]


def test_refusals_before_the_device():
    env = pr.OceanEnvironment2D(flat_earth_transform=False)
    fan = _host_fan()
    b = pr.fluid_halfspace(1700.0, 1800.0, 0.5)
    for call in _all_four(fan, env, bottom_loss=b):
        with pytest.raises(ValueError, match="does not yet apply a complex bottom phase"):
            call()
    for call in _all_four(fan, env, bottom_loss=b.loss):                            # the loss pair passes that check
        with pytest.raises(ValueError, match="bounce log"):
            call()
    for w in (0.0, -1.0, np.nan, np.inf):
        for call in _all_four(fan, env, min_width=w):
            with pytest.raises(ValueError, match="min_width must be finite and > 0"):
                call()
    for call in _all_four(fan[:1], env):
        with pytest.raises(ValueError, match="at least 2 rays"):
            call()
    for call in _all_four(_host_fan(n_surfs=[0, 1, 0, 0]), env):
        with pytest.raises(ValueError, match="no bounce log.*max_bounces"):
            call()
    for call in _all_four(fan, env, depths=(200.0, 100.0)):
        with pytest.raises(ValueError, match="strictly ascending"):
            call()
    for call in _all_four(fan, env, range_indices=[5]):
        with pytest.raises((ValueError, IndexError)):
            call()
    for call in _all_four(fan, env, absorption=-0.1):
        with pytest.raises(ValueError, match=">= 0"):
            call()
    with pytest.raises(ValueError, match="Flat earth transformation has not been applied"):
        pr.beam_arrivals(fan, [100.0], env)
    # the pulse's and the band's own arguments: the tube siblings' errors
    for f in (-1.0, np.nan, np.inf):
        with pytest.raises(ValueError, match="frequency must be finite and >= 0"):
            pr.beam_received_signal(fan, [100.0], env, f, 20.0, 0.0, 1e-3, 8, flatearth=False)
        with pytest.raises(ValueError, match="frequencies must be finite and >= 0"):
            pr.beam_transfer_function(fan, [100.0], env, [50.0, f], flatearth=False)
    with pytest.raises(ValueError, match="bandwidth must be finite and >= 0"):
        pr.beam_received_signal(fan, [100.0], env, 75.0, -1.0, 0.0, 1e-3, 8, flatearth=False)
    with pytest.raises(ValueError, match="dt must be finite and > 0"):
        pr.beam_received_signal(fan, [100.0], env, 75.0, 20.0, 0.0, 0.0, 8, flatearth=False)
    for nt in (0, 2.5, True):
        with pytest.raises(ValueError, match="n_times must be an integer >= 1"):
            pr.beam_received_signal(fan, [100.0], env, 75.0, 20.0, 0.0, 1e-3, nt, flatearth=False)
    with pytest.raises(ValueError, match="t0 must be a scalar or one start time per requested column"):
        pr.beam_received_signal(fan, [100.0], env, 75.0, 20.0, [0.0, 1.0], 1e-3, 8, flatearth=False)
    with pytest.raises(ValueError, match="non-empty 1-D"):
        pr.beam_transfer_function(fan, [100.0], env, [], flatearth=False)
    with pytest.raises(ValueError, match="t_reduce must be a scalar or one reduction time"):
        pr.beam_transfer_function(fan, [100.0], env, [50.0], t_reduce=[0.0, 1.0], flatearth=False)
    with pytest.raises(ValueError, match="one value in dB/km per frequency"):
        pr.beam_transfer_function(fan, [100.0], env, [50.0, 60.0], absorption=lambda f: np.ones(3), flatearth=False)
    with pytest.raises(ValueError, match="carrier must be finite and at least"):
        pr.beam_received_waveform(fan, [100.0], env, np.ones(4, complex), 1e-3, 100.0, 0.0, n_fft=8, flatearth=False)
    with pytest.raises(ValueError, match="n_fft .* must be at least the length of source"):
        pr.beam_received_waveform(fan, [100.0], env, np.ones(9, complex), 1e-3, 600.0, 0.0, n_fft=8, flatearth=False)
