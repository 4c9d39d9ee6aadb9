"""Complex bottom reflection without a GPU: ``fluid_halfspace`` against the independent closed form of
tests/reflection_reference.py, every refusal of ``BottomReflection`` / ``fluid_halfspace``, how the table enters through
``bottom_loss=``, the ABI header of the four new entries, the restated sums with a lag per arrival against the restatements
without one, and the waveguide over a fluid half-space on the CPU oracle's fan against the ray-theoretic image sum.  The values
measured here are the ones reflection_reference.py records; the GPU test (tests/test_reflection.py) uses twice them as bounds."""
import inspect
import os

import numpy as np
import pytest

import pygenray_amd as pr
from pygenray_amd._fan_frame import _boundary_spec, _lag_spec, _loss_table

import bounce_reference as bref
import coherent_reference as cref
import reflection_reference as rref
import signal_reference as sref
import spectrum_reference as spref
import wave_reference as wref
from test_coherent_host import _host_fan
from test_coherent_wave_host import _oracle_fan
from test_signal_host import synthetic_arrivals as signal_arrivals
from test_spectrum_host import synthetic_arrivals as spectrum_arrivals
from tube_gpu import SYN_R, SYN_Z, syn_cin, synthetic_fan

BOTTOMS = [(1700.0, 1800.0, 0.5), (1700.0, 1800.0, 0.0), (1600.0, 1500.0, 0.2), (1800.0, 2000.0, 1.0)]


def _bits(a, b):
    return np.array_equal(a.real, b.real, equal_nan=True) and np.array_equal(a.imag, b.imag, equal_nan=True)


# ---- the coefficient ----------------------------------------------------------------------------------------------------------

@pytest.mark.parametrize("cb, rho, att", BOTTOMS)
def test_fluid_halfspace_is_the_closed_form_at_its_nodes(cb, rho, att):
    b = pr.fluid_halfspace(cb, rho, att)
    g = b.grazing_deg
    assert len(b) == 1801 and g[0] == 0.0 and g[-1] == 90.0 and np.allclose(np.diff(g), 0.05, rtol=0, atol=1e-12)
    R = rref.rayleigh(g, cb, rho, att)
    (gl, db), (gg, lag) = b.loss, b.lag
    assert np.array_equal(gl, g) and np.array_equal(gg, g)
    got = 10.0 ** (-db / 20.0) * np.exp(-2j * np.pi * lag)
    print(f"fluid_halfspace({cb}, {rho}, {att}): worst |table - R| at the nodes {np.abs(got - R).max():.2e}; lag "
          f"{lag.min():.4f} ... {lag.max():.4f}")
    assert np.abs(got - R).max() <= 1e-12
    assert np.abs(b.magnitude * np.exp(1j * np.radians(b.phase_deg)) - R).max() <= 1e-12
    assert (lag >= 0.0).all() and lag.max() <= 0.5 + 1e-15 and (db >= 0.0).all() and not np.signbit(db).any()
    # continuous: no step between neighbouring nodes beyond what the closed form itself makes there
    closed = np.unwrap(-np.angle(R)) / (2.0 * np.pi)
    assert (np.abs(np.diff(lag)) <= np.abs(np.diff(closed)) + 1e-12).all() and np.abs(np.diff(lag)).max() < 0.1


def test_lossless_bottom_normal_incidence_and_total_reflection():
    cb, rho = 1700.0, 1800.0
    b = pr.fluid_halfspace(cb, rho)
    g = b.grazing_deg
    normal = (rho * cb - 1000.0 * 1500.0) / (rho * cb + 1000.0 * 1500.0)
    assert b.magnitude[-1] == pytest.approx(normal, rel=1e-14) and b.lag[1][-1] == 0.0 and b.phase_deg[-1] == 0.0
    crit = rref.critical_angle(cb)
    below = g < crit - 1e-9
    assert 28.0 < crit < 28.1 and below.sum() == 562
    db, lag = b.loss[1], b.lag[1]
    assert (db[below] == 0.0).all() and (b.magnitude[below] == 1.0).all() and (db[~below] > 0.0).all()
    # |R| = 1 there: R = (a - i gamma) / (a + i gamma), a = m sin(theta), gamma = sqrt(cos^2 - n^2): lag = atan(gamma / a) / pi
    th = np.radians(g[below])
    a, gamma = (rho / 1000.0) * np.sin(th), np.sqrt(np.cos(th) ** 2 - (1500.0 / cb) ** 2)
    with np.errstate(divide="ignore"):
        ref = np.arctan(gamma / a) / np.pi
    assert np.abs(lag[below] - ref).max() <= 1e-14 and lag[0] == 0.5 and (np.diff(lag[below]) < 0).all()
    assert (b.phase_deg[below] < 0).all()                                # total reflection from a fast bottom: a negative phase
    assert (lag[~below] == 0.0).all()                                    # above critical a lossless R is real and positive here
    # the water's own values enter: a bottom like the water reflects nothing, and is refused for it
    with pytest.raises(ValueError, match="intromission.*0 degrees"):
        pr.fluid_halfspace(1500.0, 1000.0)
    c = pr.fluid_halfspace(1700.0, 1800.0, water_sound_speed=1480.0, water_density=1025.0)
    assert np.abs(c.magnitude * np.exp(1j * np.radians(c.phase_deg)) - rref.rayleigh(g, 1700.0, 1800.0, 0.0, 1480.0, 1025.0)).max() <= 1e-12


def test_the_table_between_its_nodes():
    """the documented limits of the linear table: measured against the closed form half way between the nodes"""
    for att, near, far in ((0.0, 0.03, 6e-5), (0.5, 1.9e-5, 1.9e-5)):
        b = pr.fluid_halfspace(1700.0, 1800.0, att)
        mid = 0.5 * (b.grazing_deg[1:] + b.grazing_deg[:-1])
        miss = np.abs(b(mid) - rref.rayleigh(mid, 1700.0, 1800.0, att))
        kink = np.abs(mid - rref.critical_angle(1700.0)) < 0.5
        print(f"attenuation {att}: the table misses R between its nodes by {miss[kink].max():.2e} within 0.5 degrees of the critical "
              f"angle, {miss[~kink].max():.2e} elsewhere")
        assert miss[kink].max() <= near * 1.05 and miss[~kink].max() <= far * 1.05
    assert miss.max() > 1e-6                                             # (a measurement, not an identity)


def test_a_slow_bottom_has_an_angle_of_intromission_and_is_refused_by_name():
    # c_b < c_w and rho_b > rho_w: R passes through zero at sin^2 = (m^2 - n^2) / (m^2 - 1)... in grazing terms below
    m, n = 1.5, 1500.0 / 1450.0
    angle = np.degrees(np.arcsin(np.sqrt((n * n - 1.0) / (m * m - 1.0))))
    step = angle / 40.0                                                  # a node exactly on it
    with pytest.raises(ValueError, match="angle of intromission") as err:
        pr.fluid_halfspace(1450.0, 1500.0, step_deg=step)
    assert f"{40 * step:g} degrees" in str(err.value)
    b = pr.fluid_halfspace(1450.0, 1500.0, 0.1)                          # with attenuation |R| stays above the floor
    R = rref.rayleigh(b.grazing_deg, 1450.0, 1500.0, 0.1)
    assert b.magnitude.min() > 1e-6 and (b.lag[1] >= 0).all()
    assert np.abs(b.magnitude * np.exp(-2j * np.pi * b.lag[1]) - R).max() <= 1e-12


def test_bottom_reflection_views():
    b = pr.BottomReflection([5.0, 10.0, 40.0], [1.0, 0.5, 0.1], [-170.0, -20.0, 30.0])
    g, db = b.loss
    assert np.array_equal(g, [5.0, 10.0, 40.0]) and db[0] == 0.0 and db[2] == pytest.approx(20.0) and db[1] == -20.0 * np.log10(0.5)
    g, lag = b.lag
    assert np.array_equal(lag, 1 - np.array([-170.0, -20.0, 30.0]) / 360.0) and lag.min() >= 0     # n = 1: 30 degrees alone is negative
    assert np.array_equal(pr.BottomReflection([1.0], [1.0], [-90.0]).lag[1], [0.25])               # n = 0
    assert np.array_equal(pr.BottomReflection([1.0, 2.0], [1.0, 1.0], [0.0, 725.0]).lag[1], [3.0, 3.0 - 725.0 / 360.0])
    assert np.array_equal(pr.BottomReflection([1.0], [0.5], [0.0]).lag[1], [0.0])
    for view in (b.loss, b.lag):                                         # copies: the object itself cannot be changed through them
        view[0][0] = 99.0
    assert b.loss[0][0] == 5.0 and not b.magnitude.flags.writeable and len(b) == 3
    R = b([5.0, 7.5, 60.0])
    assert R[0] == pytest.approx(np.exp(-1j * np.radians(170.0))) and abs(R[2]) == pytest.approx(0.1)
    assert np.angle(R[1], deg=True) == pytest.approx(-95.0) and abs(R[1]) == pytest.approx(0.5 ** 0.5)


@pytest.mark.parametrize("args, msg", [
    (([1.0, 2.0], [1.0], [0.0, 0.0]), "equal, non-zero length"), (([], [], []), "equal, non-zero length"),
    (([[1.0]], [[1.0]], [[0.0]]), "1-D"), ((1.0, 1.0, 0.0), "1-D"),
    (([1.0, 1.0], [1.0, 1.0], [0.0, 0.0]), "strictly ascending"), (([2.0, 1.0], [1.0, 1.0], [0.0, 0.0]), "strictly ascending"),
    (([1.0, np.nan], [1.0, 1.0], [0.0, 0.0]), "strictly ascending"), (([1.0, np.inf], [1.0, 1.0], [0.0, 0.0]), "finite"),
    (([1.0], [0.0], [0.0]), r"\(0, 1\]"), (([1.0], [-0.5], [0.0]), r"\(0, 1\]"), (([1.0], [1.0 + 1e-15], [0.0]), r"\(0, 1\]"),
    (([1.0], [np.nan], [0.0]), r"\(0, 1\]"), (([1.0], [1.0], [np.nan]), "phase_deg must be finite"),
    (([1.0], [1.0], [np.inf]), "phase_deg must be finite")])
def test_bottom_reflection_refuses(args, msg):
    with pytest.raises(ValueError, match=msg):
        pr.BottomReflection(*args)


@pytest.mark.parametrize("kw, msg", [
    (dict(sound_speed=0.0), "sound_speed"), (dict(sound_speed=-1700.0), "sound_speed"), (dict(sound_speed=np.nan), "sound_speed"),
    (dict(sound_speed=np.inf), "sound_speed"), (dict(density=0.0), "density"), (dict(density=np.nan), "density"),
    (dict(attenuation=-0.1), "attenuation"), (dict(attenuation=np.nan), "attenuation"), (dict(attenuation=np.inf), "attenuation"),
    (dict(water_sound_speed=0.0), "water_sound_speed"), (dict(water_density=-1.0), "water_density"),
    (dict(step_deg=0.0), "step_deg"), (dict(step_deg=-1.0), "step_deg"), (dict(step_deg=91.0), "step_deg"),
    (dict(step_deg=np.nan), "step_deg")])
def test_fluid_halfspace_refuses(kw, msg):
    with pytest.raises(ValueError, match=msg):
        pr.fluid_halfspace(**dict(dict(sound_speed=1700.0, density=1800.0), **kw))


def test_a_step_that_does_not_divide_ninety_still_ends_at_ninety():
    b = pr.fluid_halfspace(1700.0, 1800.0, 0.5, step_deg=7.0)
    assert b.grazing_deg[-1] == 90.0 and b.grazing_deg[-2] == 84.0 and len(b) == 14
    assert len(pr.fluid_halfspace(1700.0, 1800.0, 0.5, step_deg=90.0)) == 2


# ---- how it enters ------------------------------------------------------------------------------------------------------------

def test_bottom_loss_takes_the_table_and_surface_loss_refuses_it():
    b = pr.fluid_halfspace(1700.0, 1800.0, 0.5)
    g, db = _loss_table(b, "bottom_loss")
    assert np.array_equal(g, b.loss[0]) and np.array_equal(db, b.loss[1])
    plain = _loss_table(b.loss, "bottom_loss")
    assert np.array_equal(plain[0], g) and np.array_equal(plain[1], db)
    with pytest.raises(ValueError, match="surface_loss.*BottomReflection"):
        _loss_table(b, "surface_loss")
    one = pr.BottomReflection([10.0], [0.5], [-90.0])
    assert _loss_table(one, "bottom_loss")[0] is None and _lag_spec(one)[0][0] is None and _lag_spec(one)[0][1][0] == 0.25
    # the lag tables: the bottom's slot holds the lag, the surface's 0.0; every other form of bottom_loss has none
    (lg, lv), (sg, sv) = _lag_spec(b)
    assert np.array_equal(lg, b.lag[0]) and np.array_equal(lv, b.lag[1]) and sg is None and np.array_equal(sv, [0.0])
    for other in (None, 3.0, ([1.0, 2.0], [0.5, 0.7]), b.loss):
        assert _lag_spec(other) is None
    # the public functions: surface_loss refuses it; a fan without a bounce log is refused as ever
    env = pr.OceanEnvironment2D(flat_earth_transform=False)
    fan = _host_fan()
    calls = [lambda **kw: pr.pressure_field(fan, [100.0], env, 50.0, flatearth=False, **kw),
             lambda **kw: pr.coherent_transmission_loss(fan, [100.0], env, 50.0, flatearth=False, **kw),
             lambda **kw: pr.received_signal(fan, [100.0], env, 50.0, 20.0, 0.0, 1e-3, 8, flatearth=False, **kw),
             lambda **kw: pr.transfer_function(fan, [100.0], env, [50.0], flatearth=False, **kw),
             lambda **kw: pr.received_waveform(fan, [100.0], env, [1.0, 0.5], 1e-3, 600.0, 0.0, n_times=8, flatearth=False, **kw),
             lambda **kw: pr.transmission_loss(fan, [100.0], env, flatearth=False, **kw),
             lambda **kw: pr.beam_transmission_loss(fan, [100.0], env, flatearth=False, **kw),
             lambda **kw: pr.arrivals(fan, [100.0], env, flatearth=False, **kw),
             lambda **kw: pr.boundary_loss(fan, env, flatearth=False, **kw)]
    for call in calls:
        with pytest.raises(ValueError, match="surface_loss.*BottomReflection"):
            call(surface_loss=b)
        with pytest.raises(ValueError, match="max_bounces"):
            call(bottom_loss=b)
    with pytest.raises(ValueError, match="max_bounces"):
        _boundary_spec(fan, b, None)


def test_the_names_are_exported_and_no_public_signature_changed():
    for name in ("BottomReflection", "fluid_halfspace"):
        assert name in pr.__all__ and callable(getattr(pr, name))
    sig = inspect.signature(pr.fluid_halfspace).parameters
    assert list(sig) == ["sound_speed", "density", "attenuation", "water_sound_speed", "water_density", "step_deg"]
    assert [sig[k].default for k in list(sig)[2:]] == [0.0, 1500.0, 1000.0, 0.05]
    assert list(inspect.signature(pr.BottomReflection).parameters) == ["grazing_deg", "magnitude", "phase_deg"]
    assert list(inspect.signature(pr.pressure_field).parameters) == list(inspect.signature(pr.coherent_transmission_loss).parameters)
    arr = inspect.signature(pr.Arrivals).parameters
    assert list(arr)[-1] == "bottom_phase" and arr["bottom_phase"].kind is inspect.Parameter.KEYWORD_ONLY
    assert arr["bottom_phase"].default is None
    a = pr.Arrivals(np.zeros(1, np.int64), np.zeros(0), np.zeros(0), np.zeros(0, np.int64), np.zeros(0, np.int32), np.zeros(0),
                    np.zeros(0), np.zeros(0), np.zeros(0), np.zeros(2), np.zeros((0, 0)))
    assert a.bottom_phase is None


def test_the_four_entries_are_bound_from_a_header_of_their_own():
    from pygenray_amd import _lib
    names = {"pgr_fan_pressure_phi": 11, "pgr_pressure_device_phi": 17, "pgr_signal_device_phi": 15, "pgr_spectrum_device_phi": 15}
    own = _lib.HEADER_PROTOTYPES["pgr_reflection.h"]
    assert set(own) == set(names)
    for name, arity in names.items():
        assert len(own[name][1]) == arity, name
        for other in [protos for h, protos in _lib.HEADER_PROTOTYPES.items() if h != "pgr_reflection.h"]:
            assert name not in other
    # each is its sibling's prototype with one more pointer directly after q
    import ctypes
    for new, (old, table, at) in {"pgr_fan_pressure_phi": ("pgr_fan_pressure_w", _lib.HEADER_PROTOTYPES["pgr_coherent.h"], 4),
                                  "pgr_pressure_device_phi": ("pgr_pressure_device_w", _lib.HEADER_PROTOTYPES["pgr_coherent.h"], 10),
                                  "pgr_signal_device_phi": ("pgr_signal_device", _lib.HEADER_PROTOTYPES["pgr_signal.h"], 6),
                                  "pgr_spectrum_device_phi": ("pgr_spectrum_device", _lib.HEADER_PROTOTYPES["pgr_spectrum.h"], 6)}.items():
        ret, args = own[new]
        oret, oargs = table[old]
        assert ret is oret and args[:at] == oargs[:at] and args[at] is ctypes.c_void_p and args[at + 1:] == oargs[at:], new
        assert oargs[at - 1] is ctypes.c_void_p                          # (q)
    for fn in ("pressure_phi_device", "signal_phi_device", "spectrum_phi_device"):
        assert callable(getattr(_lib, fn))
    assert callable(_lib.FanHandle.pressure_phi)
    text = open(_lib.HEADER).read()
    inc = '#include "pgr_reflection.h"'
    assert text.count(inc) == 1 and text.index('#include "pgr_spectrum.h"') < text.index(inc) < text.rindex("#ifdef __cplusplus")
    hip = open(_lib.CSRC + "/pgr_hip.hip").read()
    assert hip.index('#include "pgr_signal.h"') < hip.index('#include "pgr_reflect.h"') < hip.index('#include "pgr_spectrum.h"')
    # the header is one of those the binding reads and the build depends on, and load() binds every name of it
    header = [h for h in _lib.HEADERS if os.path.basename(h) == "pgr_reflection.h"]
    assert len(header) == 1 and os.path.samefile(os.path.dirname(header[0]), os.path.dirname(_lib.HEADER))
    assert header[0] in _lib.build_dependencies()
    assert all(_lib.PROTOTYPES[name] == proto for name, proto in own.items())


# ---- the restated sums --------------------------------------------------------------------------------------------------------

def _amps(off, I, q):
    return spref.group_amplitudes(off, I, np.zeros(len(I), np.int64) if q is None else q)


def test_the_two_added_operations_leave_the_phase_alone_at_whole_cycles():
    t = np.concatenate([np.random.default_rng(3).uniform(-0.5, 0.5, 4000), [-0.5, 0.5, 0.0, -0.0, 0.25, np.nextafter(0.5, 0)]])
    for phi in (0.0, 3.0, -2.0, 1e6):
        assert np.array_equal(rref.turn_back(t, np.full(len(t), phi)), t)
    assert np.array_equal(rref.turn_back(np.array([0.1, -0.4]), np.array([0.25, 0.25])), [0.1 - 0.25, (-0.4 - 0.25) + 1.0])
    assert np.isnan(rref.turn_back(np.array([0.1]), np.array([np.nan]))).all()
    P0, P1, w = np.array([0.3, 5.0]), np.array([0.7000000001, 5.0]), np.array([1.0 / 3.0, 0.7])
    got = rref.arrival_lag(P0, P1, w)
    assert got[0] == P0[0] + w[0] * (P1[0] - P0[0]) and got[1] == 5.0


def test_signal_and_spectrum_sums_with_whole_cycles_are_the_sums_without():
    off, T, I, q = signal_arrivals()
    G, n = len(off) - 1, len(T)
    tstart = np.full(G, 59.9)
    for qq in (q, None):
        for rs in (0.0, sref.inv_sigma(20.0)):
            ref = sref.signal_sum(off, T, I, qq, tstart, 75.0, rs, 8e-3, 300)
            for phi in (0.0, 3.0, -2.0):
                assert _bits(rref.signal_sum(off, T, I, qq, np.full(n, phi), tstart, 75.0, rs, 8e-3, 300), ref), (rs, phi)
            # a quarter cycle of lag is one more quarter cycle of q
            q1 = (np.zeros(n, np.int32) if qq is None else np.where(qq >= 0, qq + 1, qq))
            lagged = rref.signal_sum(off, T, I, qq, np.full(n, 0.25), tstart, 75.0, rs, 8e-3, 300)
            shifted = sref.signal_sum(off, T, I, q1 if qq is not None else np.ones(n, np.int32), tstart, 75.0, rs, 8e-3, 300)
            A = _amps(off, I, qq)
            assert (np.abs(lagged - shifted).max(axis=1) <= 1e-15 * A).all() and not _bits(lagged, ref)
        for phi in (0.0, 3.0, -2.0):
            assert _bits(rref.cw_sum(off, T, I, qq, np.full(n, phi), 75.0), sref.cw_sum(off, T, I, qq, 75.0))
    off, T, I, q = spectrum_arrivals()
    G, n = len(off) - 1, len(T)
    freq = np.array([0.0, 50.0, 75.0, 75.37, 95.0, 250.0, 1000.0])
    L, alpha = np.linspace(9e4, 9.3e4, n), np.linspace(1e-6, 1e-5, len(freq))
    tred = np.array([59.7, 60.0 - 0.119, 58.123456])
    for qq in (q, None):
        for LL, aa in ((None, None), (L, alpha)):
            ref = spref.spectrum_sum(off, T, I, qq, LL, tred, freq, aa)
            for phi in (0.0, 3.0, -2.0):
                assert _bits(rref.spectrum_sum(off, T, I, qq, np.full(n, phi), LL, tred, freq, aa), ref), phi
            lagged = rref.spectrum_sum(off, T, I, qq, np.full(n, 0.25), LL, tred, freq, aa)
            q1 = np.ones(n, np.int32) if qq is None else np.where(qq >= 0, qq + 1, qq)
            shifted = spref.spectrum_sum(off, T, I, q1, LL, tred, freq, aa)
            A = _amps(off, I, qq)
            assert (np.abs(lagged - shifted).max(axis=1) <= 1e-15 * A).all() and not _bits(lagged, ref)
    # without a reduction time the band sum with lags is the CW sum with lags at every frequency, bit for bit
    phi = rref.synthetic_lags(n, 5)
    phi[np.isnan(phi)] = 0.125
    H = rref.spectrum_sum(off, T, I, q, phi, None, np.zeros(G), freq, None)
    u = rref.signal_sum(off, T, I, q, phi, np.zeros(G), 75.0, 0.0, 1e-3, 3)
    for k, f in enumerate(freq):
        assert _bits(H[:, k], rref.cw_sum(off, T, I, q, phi, f)), f
    assert all(_bits(u[:, m], rref.cw_sum(off, T, I, q, phi, 75.0)) for m in range(3))
    # a NaN lag makes its group NaN (the band sum) / the samples its arrival reaches NaN (the pulse sum); q < 0 keeps it out
    phi[20] = np.nan
    Hn = rref.spectrum_sum(off, T, I, q, phi, None, np.zeros(G), freq, None)
    g = int(np.searchsorted(off, 20, side="right") - 1)
    if q[20] >= 0:
        assert np.isnan(Hn[g].real).all() and not np.isnan(np.delete(Hn, g, axis=0).real).any()
    qn = q.copy()
    qn[20] = -1
    assert not np.isnan(rref.spectrum_sum(off, T, I, qn, phi, None, np.zeros(G), freq, None).real).any()


def _tube_case(M=130, S=5, R=40, seed=19):
    cin = syn_cin()
    z, p, x, p0, depths = synthetic_fan(M, S, R, seed=seed, cin=cin)
    rng = np.random.default_rng(seed + 1)
    t = np.cumsum(rng.uniform(0.2, 1.5, (S, M)), axis=0)
    W = 10.0 ** rng.uniform(-3.0, 0.0, (S, M))
    q = rng.integers(-1, 10, (S, M)).astype(np.int32)
    return cin, z, p, t, x, p0, depths, W, q


def test_tube_sum_with_whole_cycles_is_the_tube_sum_without():
    cin, z, p, t, x, p0, depths, W, q = _tube_case()
    S, M = z.shape
    f = 37.5
    for w, qq in ((W, q), (None, None)):
        args = (z.T, p.T, t.T, x, p0, depths, cin, SYN_R, SYN_Z, None if w is None else w.T, None if qq is None else qq.T, f)
        re, im = cref.tube_pressure(*args)
        assert (np.nan_to_num(re) != 0).sum() > 50
        for phi in (0.0, 3.0, -2.0):
            got = rref.tube_pressure(*args, np.full((M, S), phi))
            assert np.array_equal(got[0], re, equal_nan=True) and np.array_equal(got[1], im, equal_nan=True), phi
        # a quarter cycle on every ray is a quarter cycle on every arrival: q + 1 (0.25 + w * 0.0 exactly)
        lag = rref.tube_pressure(*args, np.full((M, S), 0.25))
        q1 = np.ones((M, S), np.int32) if qq is None else np.where(qq.T >= 0, qq.T + 1, qq.T)
        sh = cref.tube_pressure(*args[:10], q1, f)
        amp = cref.tube_pressure(*args[:10], None if qq is None else np.where(qq.T >= 0, 0, -1), 0.0)[0]     # sum of the amplitudes
        lit = ~np.isnan(re)
        assert (np.abs(lag[0] - sh[0])[lit] <= 1e-15 * amp[lit]).all() and (np.abs(lag[1] - sh[1])[lit] <= 1e-15 * amp[lit]).all()
        assert not np.array_equal(lag[0], re, equal_nan=True)
    # a NaN lag on one ray makes NaN exactly the receivers its two tubes reach in that column
    Phi = np.zeros((M, S))
    Phi[60, 2] = np.nan
    got = rref.tube_pressure(z.T, p.T, t.T, x, p0, depths, cin, SYN_R, SYN_Z, None, None, f, Phi)[0]
    ref = cref.tube_pressure(z.T, p.T, t.T, x, p0, depths, cin, SYN_R, SYN_Z, None, None, f)[0]
    new_nan = np.isnan(got) & ~np.isnan(ref)
    assert new_nan.any() and not new_nan[:, [0, 1, 3, 4]].any()
    assert np.array_equal(got[~new_nan], ref[~new_nan], equal_nan=True)


# ---- the waveguide over a fluid half-space ------------------------------------------------------------------------------------

def _guide():
    """the CPU oracle's fan in wave_reference's guide, its per-sample counts and the lag Phi (M, S) every ray has collected, from
    the oracle's own bounces (range and reflected slowness) and fluid_halfspace's table at the default step"""
    import oracle
    n = wref.GUIDE_N
    env = wref.guide_env(pr)
    fan, o, arrs, y0 = _oracle_fan(env, wref.GUIDE_ZS, wref.guide_angles(n), wref.GUIDE_X1, wref.GUIDE_S)
    assert o["n_bott"].max() == 2 and o["n_surf"].max() == 2
    K = wref.GUIDE_K
    bx, bp, bk = np.full((n, K), np.nan), np.full((n, K), np.nan), np.full((n, K), -1, np.int8)
    for i in np.flatnonzero(o["n_surf"] + o["n_bott"] > 0):
        xb, pb, kind = bref.trace_bounces(arrs, y0[i], 0.0, wref.GUIDE_X1)
        assert len(xb) == o["n_surf"][i] + o["n_bott"][i] <= K
        bx[i, :len(xb)], bp[i, :len(xb)], bk[i, :len(xb)] = xb, pb, kind
    nb, ns = cref.log_counts(bx, bk, o["r"])
    assert np.array_equal(ns[:, -1], o["n_surf"]) and np.array_equal(nb[:, -1], o["n_bott"])
    bottom = pr.fluid_halfspace(*rref.GUIDE_BOTTOM)
    cin, cpin, rin, zin, bd, br, ba = arrs
    lag = _lag_spec(bottom)[0]
    Phi = rref.ray_lags(bx, bp, bk, o["r"], cin, rin, zin, br, bd, lag, (br, ba), psign=1.0)
    some = np.flatnonzero(o["n_bott"] > 0)[::60]                         # bounce_reference's own loops on a sample of the rays
    assert len(some) > 20 and np.array_equal(Phi[some], bref.boundary_loss(bx[some], bp[some], bk[some], o["r"], cin, rin, zin, br, bd, lag,
                                                                         (None, np.zeros(1)), (br, ba), psign=1.0)[0])
    assert Phi.shape == (n, wref.GUIDE_S) and (Phi >= 0).all() and (Phi[nb == 0] == 0).all() and (Phi[nb > 0] > 0).all()
    # straight rays over a flat bottom: every bottom bounce of a ray has its launch angle's lag
    th = np.abs(wref.guide_angles(n))
    one = np.interp(th, *lag)
    assert np.abs(Phi[:, -1] - o["n_bott"] * one).max() < 1e-9
    B = rref.ray_lags(bx, bp, bk, o["r"], cin, rin, zin, br, bd, _loss_table(bottom, "bottom_loss"), (br, ba), psign=1.0)
    W = 10.0 ** (-B / 10.0)
    return fan, env, nb, ns, Phi, W, o["r"]


@pytest.fixture(scope="module")
def guide():
    return _guide()


def test_the_comparison_cells(guide):
    x = guide[-1][wref.GUIDE_COLS]
    assert np.array_equal(x, [1e3, 2e3, 3e3, 4e3, 5e3])
    keep, sub = rref.check_guide_bottom_cells(x)
    assert np.array_equal(keep, wref.check_guide_cells(x))               # the rigid guide's edge rule, unchanged
    R, amp, inside, _, n_b, angle = rref.guide_bottom_images(x)
    assert n_b[inside].max() == 2 and (n_b[inside] == 0).any()
    # the closed forms alone: how far each wrong bottom's image sum lies from the right one on the subcritical cells
    right = rref.guide_field(x)
    norm = rref._norm(R, inside)
    for name, wrong in rref.WRONG_BOTTOMS.items():
        e = (np.abs(rref.guide_field(x, coefficient=wrong) - right) / norm)[sub]
        print(f"waveguide over the half-space, image sums: a bottom taken as '{name}' is off by at least {e.min():.3f} "
              f"(median {np.median(e):.3f}) on the {int(sub.sum())} subcritical cells")
        assert e.min() >= rref.WRONG_AT_LEAST[name]
    e = (np.abs(rref.guide_field(x, coefficient=rref.WRONG_BOTTOMS["rigid"]) - right) / norm)[keep]
    print(f"  rigid against the half-space on all {int(keep.sum())} cells: median {np.median(e):.3f}")
    assert np.array_equal(rref.guide_field(x, coefficient=rref.WRONG_BOTTOMS["rigid"]), wref.waveguide_field(wref.GUIDE_F, wref.GUIDE_DEPTHS, x))


def _report(name, e, measured, x):
    idx = np.unravel_index(np.argmax(e), e.shape)
    print(f"waveguide over the half-space, {name}, restatement on the oracle's fan: worst e {e.max():.4e} at depth "
          f"{wref.GUIDE_DEPTHS[idx[0]]} m, range {x[idx[1]]} m; recorded {measured}")


def _wide_margins(error_of, bound, sub):
    """each wrong bottom's reference misses the sum by more than 100 x the bound on every subcritical cell"""
    for name, wrong in rref.WRONG_BOTTOMS.items():
        e = error_of(wrong)
        e = e.reshape(e.shape[0], e.shape[1], -1).max(axis=2)[sub]
        print(f"  against a bottom taken as '{name}': e at least {e.min():.3f}")
        assert e.min() > 100.0 * bound, name


def test_waveguide_tube_sum_over_the_half_space(guide):
    fan, env, nb, ns, Phi, W, r = guide
    x = r[wref.GUIDE_COLS]
    keep, sub = rref.check_guide_bottom_cells(x)
    p = rref.fan_pressure(fan, wref.GUIDE_DEPTHS, env, wref.GUIDE_F, Phi, flatearth=False, W=W, nb=nb, ns=ns)[:, wref.GUIDE_COLS]
    e = rref.guide_error(p, x)
    _report("tube sum at 50 Hz", e, rref.GUIDE_MEASURED, x)
    bound = rref.guide_bounds()[0]
    assert bound == 2.0 * rref.GUIDE_MEASURED < 0.01
    assert e.max() <= bound
    assert e.max() == pytest.approx(rref.GUIDE_MEASURED, rel=1e-3)                  # the constant is this fan's value
    _wide_margins(lambda wrong: rref.guide_error(p, x, coefficient=wrong), bound, sub)


@pytest.fixture(scope="module")
def guide_arrivals(guide):
    fan, env, nb, ns, Phi, W, r = guide
    import arrivals_reference as aref
    off, T, I, q, phi = rref.fan_arrivals(fan, wref.GUIDE_DEPTHS, env, wref.GUIDE_COLS, Phi, flatearth=False, nb=nb, ns=ns)
    a = aref.fan_arrivals(fan, wref.GUIDE_DEPTHS, env, wref.GUIDE_COLS, False)
    return off, T, I, q, phi, a, None, r[wref.GUIDE_COLS]


def _weighted_intensities(guide, a):
    """I_a of every arrival with the bottom's magnitude: the TL term of the arrival's tube and column from the weighted g"""
    import path_reference as pref
    fan, env, nb, ns, Phi, W, r = guide
    x, cin, rin, zin, _, _, _, p0 = rref.fan_frame(fan, env, False)
    g = pref.weighted_g(fan.zs, fan.ps, x, cin, rin, zin, W)
    d = -np.asarray(fan.zs, dtype=float)
    slot = np.repeat(np.arange(len(a["offsets"]) - 1), np.diff(a["offsets"])) % len(wref.GUIDE_COLS)
    s = wref.GUIDE_COLS[slot]
    k = a["tube"].astype(np.int64)
    rr = np.abs(x - x[0])
    return 0.5 * (g[k, s] + g[k + 1, s]) * np.abs(p0[k + 1] - p0[k]) / (rr[s] * np.abs(d[k + 1, s] - d[k, s]))


def test_waveguide_band_and_pulse_sums_over_the_half_space(guide, guide_arrivals):
    off, T, I0, q, phi, a, _, x = guide_arrivals
    I = _weighted_intensities(guide, a)
    assert (I <= I0).all() and (I < I0).any() and np.array_equal(I[phi == 0], I0[phi == 0])
    R, n = len(wref.GUIDE_DEPTHS), len(x)
    keep, sub = rref.check_guide_bottom_cells(x)
    # with t_reduce = 0 the band sum at 50 Hz is the tube sum, bit for bit: the same operations in the same order
    fan, env, nb, ns, Phi, W, r = guide
    p = rref.fan_pressure(fan, wref.GUIDE_DEPTHS, env, wref.GUIDE_F, Phi, flatearth=False, W=W, nb=nb, ns=ns)[:, wref.GUIDE_COLS]
    assert _bits(rref.cw_sum(off, T, I, q, phi, wref.GUIDE_F).reshape(R, n), p)
    tred = np.tile(x / wref.GUIDE_C, R)
    Hf = rref.spectrum_sum(off, T, I, q, phi, None, tred, wref.GUIDE_BAND, None).reshape(R, n, -1)
    e = rref.guide_band_error(Hf, x)
    _report(f"band sum at {wref.GUIDE_BAND.tolist()} Hz with t_reduce = x / c", e, rref.GUIDE_BAND_MEASURED, x)
    bound = rref.guide_bounds()[1]
    assert bound == 2.0 * rref.GUIDE_BAND_MEASURED < 0.01
    assert e.max() <= bound
    assert e.max() == pytest.approx(rref.GUIDE_BAND_MEASURED, rel=1e-3)
    mid = len(wref.GUIDE_BAND) // 2
    assert wref.GUIDE_BAND[mid] == wref.GUIDE_F
    tau = 2j * np.pi * wref.GUIDE_F * (x / wref.GUIDE_C)

    def band_error_of(wrong):
        return np.abs(Hf[:, :, mid] * np.exp(tau)[None, :] - rref.guide_field(x, coefficient=wrong)) / \
            rref._norm(*rref.guide_bottom_images(x)[0:3:2])
    _wide_margins(band_error_of, bound, sub)
    # the pulse
    wref.check_guide_pulse(x)
    tstart = np.tile(wref.guide_t0(x), R)
    rs = sref.inv_sigma(wref.GUIDE_B)
    u = rref.signal_sum(off, T, I, q, phi, tstart, wref.GUIDE_F, rs, wref.GUIDE_DT, wref.GUIDE_NT).reshape(R, n, wref.GUIDE_NT)
    e = rref.guide_pulse_error(u, x)
    _report("pulse sum", e, rref.GUIDE_PULSE_MEASURED, x)
    bound = rref.guide_bounds()[2]
    assert bound == 2.0 * rref.GUIDE_PULSE_MEASURED < 0.01
    assert e.max() <= bound
    assert e.max() == pytest.approx(rref.GUIDE_PULSE_MEASURED, rel=1e-3)
    # the pulse with a rigid bottom's sum is far off: the phase shapes the arrival
    u0 = sref.signal_sum(off, T, I0, q, tstart, wref.GUIDE_F, rs, wref.GUIDE_DT, wref.GUIDE_NT).reshape(R, n, wref.GUIDE_NT)
    assert rref.guide_pulse_error(u0, x).max(axis=2)[sub].min() > 100.0 * bound
