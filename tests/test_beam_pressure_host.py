"""beam_pressure_field without a GPU: the NumPy restatement of tests/beam_pressure_reference.py against
closed forms -- Lloyd's mirror and the free field on exact straight rays, the image sum of wave_reference's waveguide on the CPU
oracle's fan -- the caustic bound, the definition's identities, and the exports, prototypes and refusals of the new entries.
The values measured here are the ones beam_pressure_reference.py and DESIGN.md record; every bound is twice its value."""
import ctypes
import inspect
import os

import numpy as np
import pytest

import pygenray_amd as pr

import beam_pressure_reference as bp
import beam_reference as bref
import coherent_reference as cref
import wave_reference as wref
from test_coherent_host import _host_fan
from test_coherent_wave_host import _guide_fan


# ---- Lloyd's mirror on exact rays ---------------------------------------------------------------------------------------------

@pytest.fixture(scope="module")
def lloyd():
    """e (len(LLOYD_DEPTHS), 4) per (min_width, curvature)"""
    return {(w, curv): bp.lloyd_error(bp.exact_pressure(bp.LLOYD_ZS, bp.LLOYD_DEPTHS, w, curv))
            for w in bp.WIDTHS for curv in (True, False)}


def test_lloyd_receivers_lie_four_sigma_inside_the_aperture_of_both_paths():
    edge = np.tan(np.radians(bp.EXACT_APERTURE)) * bp.EXACT_RANGES
    for w in bp.WIDTHS:
        reach = 4.0 * bp.widest_beam(bp.LLOYD_ZS, w)
        # the direct path covers depths up to z_s + r tan 40, the reflected one up to r tan 40 - z_s; both reach the surface
        assert (bp.LLOYD_DEPTHS.max() + reach <= edge - bp.LLOYD_ZS).all(), w
        assert (edge > bp.LLOYD_ZS).all()
    zs, ps, ts, x, p0, q = bp.exact_fan(bp.LLOYD_ZS)
    assert (q[:, 1:] == -1).sum(axis=0).tolist() == [1, 1, 1, 1] and (q[:, 1:] == 2).any() and (q[:, 1:] == 0).any()


@pytest.mark.parametrize("w", bp.WIDTHS)
def test_lloyds_mirror_on_exact_rays(lloyd, w):
    e, e0 = lloyd[(w, True)], lloyd[(w, False)]
    print(f"Lloyd's mirror on exact rays, min_width {w} m: worst e per range with the curvature term "
          f"{[f'{v:.4e}' for v in e.max(axis=0)]} (worst {e.max():.6e}), linear phase only {[f'{v:.4e}' for v in e0.max(axis=0)]} "
          f"(worst {e0.max():.6e}); bounds {2.0 * bp.LLOYD_MEASURED[w]:.4e}, {2.0 * bp.LLOYD_MEASURED_LINEAR[w]:.4e}")
    assert e.max() <= 2.0 * bp.LLOYD_MEASURED[w]
    assert e0.max() <= 2.0 * bp.LLOYD_MEASURED_LINEAR[w]
    assert e.max() == pytest.approx(bp.LLOYD_MEASURED[w], rel=1e-3)                 # the constants are this fan's values
    assert e0.max() == pytest.approx(bp.LLOYD_MEASURED_LINEAR[w], rel=1e-3)


def test_the_curvature_term_buys_a_factor_of_ten_at_a_wavelength_scale_width(lloyd):
    e, e0 = lloyd[(10.0, True)].max(axis=0), lloyd[(10.0, False)].max(axis=0)
    print(f"min_width 10 m: the curvature term improves the worst e per range by {[f'{v:.1f}' for v in e0 / e]}")
    assert (e0 / e >= 10.0).all()
    assert lloyd[(10.0, False)].max() >= 10.0 * lloyd[(10.0, True)].max()


# ---- the free field -----------------------------------------------------------------------------------------------------------

def test_free_field_amplitude_and_phase():
    zs, ps, ts, x, p0, q = bp.exact_fan(bp.FREE_ZS)
    d = -zs[:, 1:]
    assert d.min() > 0 and (q == 0).all()                                          # no ray reaches the surface
    reach = 4.0 * bp.widest_beam(bp.FREE_ZS, 10.0)
    assert (bp.FREE_DEPTHS.min() - reach > 0).all()                                # clear of the surface: no image arrives
    assert (bp.FREE_DEPTHS.min() - reach >= d.min(axis=0)).all() and (bp.FREE_DEPTHS.max() + reach <= d.max(axis=0)).all()
    p = bp.exact_pressure(bp.FREE_ZS, bp.FREE_DEPTHS, 10.0, True)
    R = np.hypot(bp.EXACT_RANGES[None, :], bp.FREE_DEPTHS[:, None] - bp.FREE_ZS)
    amp = np.abs(np.abs(p) * R - 1.0).max()
    phase = np.abs(np.angle(p * np.exp(-2j * np.pi * bp.EXACT_F * R / bp.EXACT_C))).max()
    print(f"free field, min_width 10 m: worst | |p| R - 1 | {amp:.6e}, worst phase difference {phase:.6e} rad")
    assert amp <= 2.0 * bp.FREE_MEASURED_AMPLITUDE and phase <= 2.0 * bp.FREE_MEASURED_PHASE
    assert amp == pytest.approx(bp.FREE_MEASURED_AMPLITUDE, rel=1e-3) and phase == pytest.approx(bp.FREE_MEASURED_PHASE, rel=1e-3)


# ---- the rigid waveguide of wave_reference ------------------------------------------------------------------------------------

GUIDE_BEAM_MEASURED, GUIDE_BEAM_DROPPED_MEASURED = bp.GUIDE_BEAM_MEASURED, bp.GUIDE_BEAM_DROPPED_MEASURED


def test_waveguide_image_sum_from_the_restatement():
    fan, env, nb, ns, o = _guide_fan(wref.GUIDE_N)
    x = o["r"][wref.GUIDE_COLS]
    keep = wref.check_guide_cells(x)
    assert int(keep.sum()) == 74 and int((~keep).sum()) == 16
    p = bp.fan_beam_pressure(fan, wref.GUIDE_DEPTHS, env, wref.GUIDE_F, w_min=10.0, flatearth=False, nb=nb, ns=ns,
                             cols=wref.GUIDE_COLS)
    R, sign, inside, _ = wref.guide_images(x)
    e = np.abs(p - wref.waveguide_field(wref.GUIDE_F, wref.GUIDE_DEPTHS, x)) / wref._norm(R, inside)
    mid = keep & ((wref.GUIDE_DEPTHS >= 375.0) & (wref.GUIDE_DEPTHS <= 625.0))[:, None]
    print(f"waveguide, beam restatement on the oracle's fan: worst e {e[keep].max():.6e} on the 74 cells kept (median "
          f"{np.median(e[keep]):.2e}; the tube sum's worst is {wref.GUIDE_MEASURED:.2e}), {e[~keep].max():.6e} on the 16 cells "
          f"dropped; worst {e[mid].max():.2e} on the {int(mid.sum())} kept cells between 375 and 625 m")
    assert e[keep].max() <= 2.0 * GUIDE_BEAM_MEASURED
    assert e[keep].max() == pytest.approx(GUIDE_BEAM_MEASURED, rel=1e-3)
    # the dropped cells: measured and recorded; not below ten times the kept cells' value, so no bound is made there
    assert np.isfinite(e[~keep]).all()
    assert e[~keep].max() == pytest.approx(GUIDE_BEAM_DROPPED_MEASURED, rel=1e-3)
    assert GUIDE_BEAM_DROPPED_MEASURED >= 10.0 * GUIDE_BEAM_MEASURED


# ---- a caustic stays bounded --------------------------------------------------------------------------------------------------

def _caustic_rows(gap):
    """21 rays at 1 km, 5 m apart, rays 10 and 11 `gap` apart around the receiver at 1000 m: (zs, ps, ts, x, p0, depths)"""
    M = 21
    d = 950.0 + 5.0 * np.arange(M)
    d[11] = 1000.0 + 0.5 * gap
    d[10] = 1000.0 - 0.5 * gap
    th = np.radians(np.linspace(-2.0, 2.0, M))
    x = np.array([0.0, 1e3])
    zs = -np.stack([np.full(M, 1000.0), d], axis=1)
    ps = -np.tile((np.sin(th) / 1500.0)[:, None], (1, 2))
    ts = np.stack([np.zeros(M), 1e3 / (1500.0 * np.cos(th))], axis=1)
    return zs, ps, ts, x, np.sin(th) / 1500.0, np.array([1000.0])


@pytest.mark.parametrize("curvature", [True, False])
def test_a_caustic_stays_bounded(curvature):
    zs, ps, ts, x, p0, depths = _caustic_rows(1e-6)
    d = -zs[:, 1]
    assert d[10] < depths[0] < d[11] and max(depths[0] - d[10], d[11] - depths[0]) <= 1e-6 and (np.diff(d) > 0).all()
    tab = (bp.EXACT_CIN, bp.EXACT_RIN, bp.EXACT_ZIN)
    tre, tim = cref.tube_pressure(zs, ps, ts, x, p0, depths, *tab, None, None, 50.0)
    re, im, asum, Asum, _ = bp.beam_pressure(zs, ps, ts, x, p0, depths, *tab, np.full(2, bp.EXACT_BOTTOM), 10.0, None, None, 50.0,
                                             curvature, detail=True)
    tube, beam = np.hypot(tre[0, 1], tim[0, 1]), np.hypot(re[0, 1], im[0, 1])
    print(f"a tube 1e-6 m wide at the receiver, curvature {curvature}: tube sum |p| {tube:.4e}, beam sum |p| {beam:.4e}, "
          f"sum of A' {Asum[0, 1]:.4e}")
    assert beam > 0 and tube >= 100.0 * beam
    assert beam <= Asum[0, 1] and asum[0, 1] <= Asum[0, 1]
    # ... and the crossing itself (D = 0) adds +0: the sums are those without that tube
    zs0 = zs.copy()
    zs0[10, 1] = zs0[11, 1]
    q = np.zeros((21, 2), np.int32)
    a = bp.beam_pressure(zs0, ps, ts, x, p0, depths, *tab, np.full(2, bp.EXACT_BOTTOM), 10.0, None, q, 50.0, curvature)
    q[10] = -1
    b = bp.beam_pressure(zs0, ps, ts, x, p0, depths, *tab, np.full(2, bp.EXACT_BOTTOM), 10.0, None, q, 50.0, curvature)
    assert np.array_equal(a[0], b[0], equal_nan=True) and np.array_equal(a[1], b[1], equal_nan=True)


# ---- identities of the definition ---------------------------------------------------------------------------------------------

@pytest.fixture(scope="module")
def folded():
    """a small folded fan in an isovelocity waveguide (surface, bottom at 1000 m), with q from 0 to 5 and some -1"""
    th, zs, ps = bref.folded_fan(n_rays=301, max_angle=40.0, ranges=np.array([0.0, 1500.0, 3000.0]), zs=300.0, H=1000.0)
    ts = np.array([0.0, 1500.0, 3000.0])[None, :] / (1500.0 * np.cos(np.radians(th)))[:, None]
    rng = np.random.default_rng(7)
    q = rng.integers(0, 6, zs.shape).astype(np.int32)
    q[rng.random(zs.shape) < 0.1] = -1
    args = dict(zs=zs, ps=ps, ts=ts, x=np.array([0.0, 1500.0, 3000.0]), p0=np.sin(np.radians(th)) / 1500.0,
                depths=np.linspace(-20.0, 1020.0, 53), cin=bp.EXACT_CIN, rin=bp.EXACT_RIN, zin=bp.EXACT_ZIN,
                bottom=np.full(3, 1000.0), w_min=10.0, W=None)
    return args, q


def _same(a, b):
    return np.array_equal(a, b, equal_nan=True)


def test_identities(folded):
    args, q = folded
    re, im = bp.beam_pressure(**args, q=q, f=50.0)
    assert np.isnan(re[:, 0]).all() and np.isfinite(re[:, 1:]).all() and (np.hypot(re, im)[:, 1:] > 0).mean() > 0.9
    # f = 0 and q = 0: im = +0.0 and re the sum of a in order -- where no surface image arrives (its half cycle makes its
    # term -a): the free field's fan
    zs, ps, ts, x, p0, qf = bp.exact_fan(bp.FREE_ZS)
    free = dict(zs=zs, ps=ps, ts=ts, x=x, p0=p0, depths=bp.FREE_DEPTHS, cin=bp.EXACT_CIN, rin=bp.EXACT_RIN, zin=bp.EXACT_ZIN,
                bottom=np.full(len(x), bp.EXACT_BOTTOM), w_min=10.0, W=None)
    r0, i0, asum, _, _ = bp.beam_pressure(**free, q=qf, f=0.0, detail=True)
    assert (qf == 0).all() and _same(r0, asum) and (asum[:, 1:] > 0).all()
    assert (i0[:, 1:] == 0).all() and not np.signbit(i0[:, 1:]).any()
    rn, in_ = bp.beam_pressure(**free, q=None, f=0.0)
    assert _same(rn, r0) and _same(in_, i0)                                          # (q None: all zero)
    # ... and with the images, im is still +0.0
    i0 = bp.beam_pressure(**args, q=np.zeros_like(q), f=0.0)[1]
    assert (i0[:, 1:] == 0).all() and not np.signbit(i0[:, 1:]).any()
    # curvature False is hk = 0: it changes the field, and not where every hk is 0 anyway (one slowness: Delta p = 0)
    rl, il = bp.beam_pressure(**args, q=q, f=50.0, curvature=False)
    assert not _same(rl, re)
    flat = dict(args, ps=np.full_like(args["ps"], args["ps"][150, 1]))
    on, off = bp.beam_pressure(**flat, q=q, f=50.0), bp.beam_pressure(**flat, q=q, f=50.0, curvature=False)
    assert _same(on[0], off[0]) and _same(on[1], off[1])
    # q = -1 everywhere: 0.0
    rz, iz = bp.beam_pressure(**args, q=np.full_like(q, -1), f=50.0)
    assert (rz[:, 1:] == 0).all() and (iz[:, 1:] == 0).all() and np.isnan(rz[:, 0]).all()
    # q + 4: the same bits
    r4, i4 = bp.beam_pressure(**args, q=np.where(q >= 0, q + 4, q), f=50.0)
    assert _same(r4, re) and _same(i4, im)
    # q + 2: the field negated, re and im, bit for bit (every f tau here is beyond one cycle, so the half cycle is exact; a
    # sum to which nothing was added stays +0.0)
    r2, i2 = bp.beam_pressure(**args, q=np.where(q >= 0, q + 2, q), f=50.0)
    assert _same(r2, -re) and _same(i2, -im) and (re[:, 1:] != 0).mean() > 0.9


# ---- the helpers of the random-environment sweep can fail ---------------------------------------------------------------------

@pytest.mark.parametrize("source_depth", [bp.FREE_ZS, bp.LLOYD_ZS])
def test_the_eikonal_share_tells_the_sign_of_p(source_depth):
    """straight rays with the exact p = dT/dd: every eligible tube agrees, and not one with p in the other sign"""
    zs, ps, ts, x, p0, q = bp.exact_fan(source_depth)
    th = np.radians(np.linspace(-bp.EXACT_APERTURE, bp.EXACT_APERTURE, bp.EXACT_N))
    ns = (source_depth + x[None, :] * np.tan(th)[:, None] < 0).astype(np.int64)        # exact_fan's own fold
    assert ns.any() == (source_depth == bp.LLOYD_ZS) and np.array_equal(q[:-1] == -1, ns[:-1] != ns[1:])
    nb = np.zeros_like(ns)
    share, tubes = bp.eikonal_share(zs, ps, ts, nb, ns, x, detail=True)
    assert share == 1.0 and tubes >= 0.99 * (bp.EXACT_N - 1) * len(bp.EXACT_RANGES)
    assert bp.eikonal_share(zs, -ps, ts, nb, ns, x, detail=True) == (0.0, tubes)
    assert bp.eikonal_share(zs, ps, ts, None, None, x) == (1.0 if not ns.any() else pytest.approx(1.0, abs=1e-3))
    # a tube across a fold is not eligible, nor is the source's column, nor a tube with a NaN
    assert bp.eikonal_share(zs, ps, ts, nb, ns + 2 * np.arange(len(ns))[:, None], x, detail=True)[1] == 0
    assert np.isnan(bp.eikonal_share(zs[:, :1], ps[:, :1], ts[:, :1], None, None, x[:1]))
    holed = ts.copy()
    holed[7, 2] = np.nan
    assert bp.eikonal_share(zs, ps, holed, nb, ns, x, detail=True) == (1.0, tubes - 2)


def test_the_sign_bit_comparison_can_fail():
    from helpers import sign_flipped
    a = np.array([1.5, -2.0, 0.0, -0.0, np.nan, -np.nan, np.inf, 5e-324])
    assert sign_flipped(-a, a) and sign_flipped(a, -a) and not sign_flipped(a, a)
    for i in range(len(a)):
        b = -a
        b[i] = a[i]                                                                 # one entry's sign left as it was
        assert not sign_flipped(b, a), i
    assert not sign_flipped(-a[:-1], a) and not sign_flipped(np.abs(a), a)


# ---- exports, prototypes, refusals --------------------------------------------------------------------------------------------

def test_the_new_functions_are_exported():
    for name in ("beam_pressure_field", "coherent_beam_transmission_loss"):
        assert name in pr.__all__ and callable(getattr(pr, name))
    sig = inspect.signature(pr.beam_pressure_field).parameters
    assert list(sig) == ["rays", "receiver_depths", "env", "frequency", "min_width", "curvature", "absorption", "bottom_loss",
                         "surface_loss", "flatearth", "device"]
    assert [sig[k].default for k in list(sig)[4:]] == [10.0, True, None, None, None, True, 0]
    assert list(inspect.signature(pr.coherent_beam_transmission_loss).parameters) == list(sig)


def test_the_two_entries_are_bound_from_a_header_of_their_own():
    from pygenray_amd import _lib
    names = {"pgr_fan_beam_pressure_w": 13, "pgr_beam_pressure_device_w": 19}
    own = _lib.HEADER_PROTOTYPES["pgr_beam_coherent.h"]
    assert set(own) == set(names)
    V, D, I32, I64 = ctypes.c_void_p, ctypes.c_double, ctypes.c_int32, ctypes.c_int64
    assert own["pgr_fan_beam_pressure_w"] == (ctypes.c_int, [V, V, V, V, D, V, V, I64, D, I32, V, V, V])
    assert own["pgr_beam_pressure_device_w"] == (
        ctypes.c_int, [V, V, V, V, I64, I32, V, V, V, V, D, V, V, I64, D, I32, V, V, V])
    for name in names:
        for other in [protos for h, protos in _lib.HEADER_PROTOTYPES.items() if h != "pgr_beam_coherent.h"]:
            assert name not in other
    assert callable(_lib.beam_pressure_device) and callable(_lib.FanHandle.beam_pressure)
    text = open(_lib.HEADER).read()
    inc = '#include "pgr_beam_coherent.h"'
    assert text.count(inc) == 1 and text.index('#include "pgr_reflection.h"') < text.index(inc) < text.rindex("#ifdef __cplusplus")
    hip = open(_lib.CSRC + "/pgr_hip.hip").read()
    assert hip.index('#include "pgr_phase.h"') < hip.index('#include "pgr_beam_phase.h"')
    # the header is one of those the binding reads and the build depends on, and load() binds every name of it
    header = [h for h in _lib.HEADERS if os.path.basename(h) == "pgr_beam_coherent.h"]
    assert len(header) == 1 and os.path.samefile(os.path.dirname(header[0]), os.path.dirname(_lib.HEADER))
    assert header[0] in _lib.build_dependencies()
    assert all(_lib.PROTOTYPES[name] == proto for name, proto in own.items())


def _both(fan, env, *a, **kw):
    return [lambda: pr.beam_pressure_field(fan, [100.0], env, *a, flatearth=False, **kw),
            lambda: pr.coherent_beam_transmission_loss(fan, [100.0], env, *a, flatearth=False, **kw)]


def test_refusals_before_the_device():
    env = pr.OceanEnvironment2D(flat_earth_transform=False)
    fan = _host_fan()
    b = pr.fluid_halfspace(1700.0, 1800.0, 0.5)
    for call in _both(fan, env, 50.0, bottom_loss=b):
        with pytest.raises(ValueError, match="does not yet apply a complex bottom phase"):
            call()
    for call in _both(fan, env, 50.0, bottom_loss=b.loss):                          # the loss pair passes that check
        with pytest.raises(ValueError, match="bounce log"):
            call()
    for w in (0.0, -1.0, np.nan, np.inf):
        for call in _both(fan, env, 50.0, min_width=w):
            with pytest.raises(ValueError, match="min_width must be finite and > 0"):
                call()
    for f in (-1.0, np.nan, np.inf, -np.inf):
        for call in _both(fan, env, f):
            with pytest.raises(ValueError, match="frequency must be finite and >= 0"):
                call()
    for call in _both(fan[:1], env, 50.0):
        with pytest.raises(ValueError, match="at least 2 rays"):
            call()
    for call in _both(_host_fan(n_surfs=[0, 1, 0, 0]), env, 50.0):
        with pytest.raises(ValueError, match="no bounce log.*max_bounces"):
            call()
    with pytest.raises(ValueError, match="strictly ascending"):
        pr.beam_pressure_field(fan, [200.0, 100.0], env, 50.0, flatearth=False)
    with pytest.raises(ValueError, match="Flat earth transformation has not been applied"):
        pr.beam_pressure_field(fan, [100.0], env, 50.0)
