"""The coherent products on the GPU against wave theory (tests/wave_reference.py): fans from ``shoot_rays`` through the bounce
post-pass's counts, the caustic scan, the phase index and the sums of ``pressure_field``, ``transfer_function`` and
``received_signal`` -- against the normal modes of the focusing medium (the caustic phase) and the image sum of an isovelocity
waveguide (both boundaries, up to two bounces on each).  Every bound is twice the error of the NumPy restatements on the CPU
oracle's fan (tests/test_coherent_wave_host.py measures and pins them), so these run in the reference arithmetic (`pr`)."""
import numpy as np
import pytest

import coherent_reference as cref
import wave_reference as wref
from tube_gpu import _same, pr  # noqa: F401

pytestmark = pytest.mark.gpu


def _in_place(fan):
    assert fan.device_resident and not any(k in fan.__dict__ for k in ("_ts", "_zs", "_ps"))


# ---- normal modes of the focusing medium --------------------------------------------------------------------------------------

@pytest.fixture(scope="module")
def focus(pr):  # noqa: F811
    env = cref.focus_env(pr)
    fan = pr.shoot_rays(cref.FOCUS_Z0, 0.0, cref.focus_angles(), cref.FOCUS_X1, cref.FOCUS_S, env, flatearth=False, debug=False,
                        device_resident=True)
    assert len(fan) == cref.FOCUS_N and (fan.n_botts == 0).all() and (fan.n_surfs == 0).all()
    x = np.asarray(fan.rs[0])
    assert x.shape == (cref.FOCUS_S,) and x[0] == 0.0 and x[-1] == cref.FOCUS_X1
    cells, kappa = wref.mode_cells(x)
    wref.check_mode_cells(cells, kappa)
    return fan, env, x, cells, {f: wref.modal_field(f, wref.MODE_DEPTHS, x) for f in wref.MODE_F}


def test_pressure_field_has_the_caustic_phase_of_the_normal_modes(pr, focus):  # noqa: F811
    fan, env, x, cells, ref = focus
    p = pr.pressure_field(fan, wref.MODE_DEPTHS, env, 50.0, flatearth=False)
    _in_place(fan)
    e = wref.mode_error(p, ref[50.0], cells)
    j, k = np.unravel_index(np.argmax(e), e.shape)
    print(f"normal modes at 50 Hz from shoot_rays: worst e {e.max():.4e} at depth {wref.MODE_DEPTHS[j]} m, range {x[k]} m; "
          f"bound {wref.MODE_BOUND:.4e}")
    assert e.max() <= wref.MODE_BOUND < 0.1


def test_transfer_function_has_the_caustic_phase_of_the_normal_modes_across_the_band(pr, focus):  # noqa: F811
    fan, env, x, cells, ref = focus
    cols = np.flatnonzero(cells.any(axis=0))
    assert 250 < len(cols) < cref.FOCUS_S
    Hf = pr.transfer_function(fan, wref.MODE_DEPTHS, env, list(wref.MODE_F), range_indices=cols, flatearth=False)
    _in_place(fan)
    assert Hf.shape == (len(wref.MODE_DEPTHS), len(cols), 3)
    for i, f in enumerate(wref.MODE_F):
        e = wref.mode_error(Hf[:, :, i], ref[f][:, cols], cells[:, cols])
        j, k = np.unravel_index(np.argmax(e), e.shape)
        print(f"normal modes at {f} Hz from transfer_function: worst e {e.max():.4e} at depth {wref.MODE_DEPTHS[j]} m, range "
              f"{x[cols[k]]} m; bound {wref.MODE_BOUND:.4e}")
        assert e.max() <= wref.MODE_BOUND < 0.1, f


# ---- the isovelocity waveguide ------------------------------------------------------------------------------------------------

@pytest.fixture(scope="module")
def guide(pr):  # noqa: F811
    env = wref.guide_env(pr)
    fan = pr.shoot_rays(wref.GUIDE_ZS, 0.0, wref.guide_angles(), wref.GUIDE_X1, wref.GUIDE_S, env, flatearth=False, debug=False,
                        device_resident=True, max_bounces=wref.GUIDE_K)
    assert len(fan) == wref.GUIDE_N and fan.n_botts.max() == 2 and fan.n_surfs.max() == 2
    x = np.asarray(fan.rs[0])[wref.GUIDE_COLS]
    assert np.array_equal(x, [1e3, 2e3, 3e3, 4e3, 5e3])
    wref.check_guide_cells(x)
    return fan, env, x


def test_waveguide_pressure_field_is_the_image_sum(pr, guide):  # noqa: F811
    fan, env, x = guide
    assert (pr.caustic_index(fan, env, flatearth=False) == 0).all()
    p = pr.pressure_field(fan, wref.GUIDE_DEPTHS, env, wref.GUIDE_F, flatearth=False)
    _in_place(fan)
    e = wref.guide_error(p[:, wref.GUIDE_COLS], x)
    j, k = np.unravel_index(np.argmax(e), e.shape)
    print(f"waveguide from shoot_rays: worst e {e.max():.4e} at depth {wref.GUIDE_DEPTHS[j]} m, range {x[k]} m; "
          f"bound {wref.GUIDE_BOUND:.4e}")
    assert e.max() <= wref.GUIDE_BOUND < 0.01
    nb, ns = fan.bounce_counts(wref.GUIDE_COLS)
    assert ((nb > 0) & (ns > 0)).any() and nb.max() == 2 and ns.max() == 2
    # the same fan traced to the host (the shared one stays where it is): the same bits
    eager = pr.shoot_rays(wref.GUIDE_ZS, 0.0, wref.guide_angles(), wref.GUIDE_X1, wref.GUIDE_S, env, flatearth=False, debug=False,
                          device_resident=False, max_bounces=wref.GUIDE_K)
    assert not eager.device_resident
    host = pr.pressure_field(eager, wref.GUIDE_DEPTHS, env, wref.GUIDE_F, flatearth=False)
    assert _same(host.real, p.real) and _same(host.imag, p.imag)
    _in_place(fan)


def test_waveguide_transfer_function_with_a_reduction_time_is_the_image_sum(pr, guide):  # noqa: F811
    fan, env, x = guide
    Hf = pr.transfer_function(fan, wref.GUIDE_DEPTHS, env, wref.GUIDE_BAND, range_indices=wref.GUIDE_COLS,
                              t_reduce=x / wref.GUIDE_C, flatearth=False)
    _in_place(fan)
    e = wref.guide_band_error(Hf, x)
    print(f"waveguide transfer function from shoot_rays: worst e per frequency {[f'{v:.4e}' for v in e.max(axis=(0, 1))]}; "
          f"bound {wref.GUIDE_BAND_BOUND:.4e}")
    assert e.max() <= wref.GUIDE_BAND_BOUND < 0.01


def test_waveguide_received_signal_is_the_image_sum_of_pulses(pr, guide):  # noqa: F811
    fan, env, x = guide
    wref.check_guide_pulse(x)
    u = pr.received_signal(fan, wref.GUIDE_DEPTHS, env, wref.GUIDE_F, wref.GUIDE_B, wref.guide_t0(x), wref.GUIDE_DT,
                           wref.GUIDE_NT, range_indices=wref.GUIDE_COLS, flatearth=False)
    _in_place(fan)
    e = wref.guide_pulse_error(u, x)
    j, k, m = np.unravel_index(np.argmax(e), e.shape)
    print(f"waveguide with a pulse from shoot_rays: worst e {e.max():.4e} at depth {wref.GUIDE_DEPTHS[j]} m, range {x[k]} m, "
          f"sample {m}; bound {wref.GUIDE_PULSE_BOUND:.4e}")
    assert e.max() <= wref.GUIDE_PULSE_BOUND < 0.01
