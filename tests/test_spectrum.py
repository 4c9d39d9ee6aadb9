"""Transfer function over a frequency band on the GPU (csrc/pgr_spectrum.h): the kernel alone through ``_lib.spectrum_device``
against the restatement of tests/spectrum_reference.py on synthetic arrivals aimed at its staging and tile seams, the error paths
of the C entry, ``transfer_function`` against ``pressure_field`` frequency by frequency on a Munk fan, fans in both trajectory
layouts (dropped rays, host fans), absorption that follows the frequency against a derived bound, and ``received_waveform``
of a Gaussian source against ``received_signal``."""
import ctypes
import os
import re
import subprocess
import sys

import numpy as np
import pytest

import signal_reference as sref
import spectrum_reference as spref
from tube_gpu import (DEPTHS, _same, munk_env, pr, pr_any, sloping_env, sloping_env_shallow_table)  # noqa: F401

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
PAD = 130                    # entries behind an output that must stay as they were
MARK = -7.25


def _tile():
    """the frequencies one wave of pgr_spec_sum handles: 64 lanes times SPEC_ROWS per lane, from the kernel's own source"""
    from pygenray_amd import _lib
    text = open(os.path.join(_lib.CSRC, "pgr_spectrum.h")).read()
    return 64 * int(re.search(r"^#define SPEC_ROWS (\d+)", text, re.M).group(1))


TILE = _tile()


def _bits(a, b):
    return _same(a.real, b.real) and _same(a.imag, b.imag)


# ---- the kernel alone ---------------------------------------------------------------------------------------------------------

def _device_spectrum(off, T, I, q, L, tred, freq, alpha):
    """_lib.spectrum_device on host arrays -> H (G, F) complex; both outputs pre-filled with a sentinel, PAD entries behind
    them checked untouched and every entry before them checked written"""
    import torch
    from pygenray_amd import _lib
    dev = torch.device("cuda", 0)
    G, F = len(off) - 1, len(freq)
    up = lambda a, dt_: torch.from_numpy(np.ascontiguousarray(a, dtype=dt_)).to(dev)   # noqa: E731
    d_off, d_T, d_I, d_tr = up(off, np.int64), up(np.append(T, 0.0), float), up(np.append(I, 0.0), float), up(tred, float)
    d_q = None if q is None else up(np.append(q, 0), np.int32)
    d_L = None if L is None else up(np.append(L, 0.0), float)
    out = [torch.full((G * F + PAD,), MARK, dtype=torch.float64, device=dev) for _ in range(2)]
    _lib.spectrum_device(0, d_off.data_ptr(), G, d_T.data_ptr(), d_I.data_ptr(), 0 if d_q is None else d_q.data_ptr(),
                         0 if d_L is None else d_L.data_ptr(), d_tr.data_ptr(), freq, alpha, out[0].data_ptr(),
                         out[1].data_ptr(), torch.cuda.current_stream(dev).cuda_stream)
    h = [a.cpu().numpy() for a in out]
    assert all((a[G * F:] == MARK).all() for a in h) and not any((a[:G * F] == MARK).any() for a in h)
    return (h[0][:G * F] + 1j * h[1][:G * F]).reshape(G, F)


COUNTS = [200, 0, 65, 1, 63, 64]             # the staging seams: groups of every one of these in one call (G = 130)


def synthetic_groups(G, F, seed):
    """groups with COUNTS arrivals (then random counts up to 130); T in [60, 62] s, I over six decades with exact
    zeros, with G > 1 one NaN T and one NaN I in the last arrivals, q in -1 ... 9, L up to 1200 km and one of 1e10 m (alpha L
    beyond the cut); a reduction time per group; frequencies descending over 95 ... 55 Hz with a repeated value and 0.0; alpha up to 1e-5 dB/m with an exact 0"""
    rng = np.random.default_rng(seed)
    cnt = np.array([COUNTS[g] if g < len(COUNTS) else int(rng.integers(0, 131)) for g in range(G)])
    off = np.concatenate([[0], np.cumsum(cnt)]).astype(np.int64)
    n = int(off[-1])
    grp = np.repeat(np.arange(G), cnt)
    T = rng.uniform(60.0, 62.0, n)
    T = T[np.lexsort((T, grp))]
    I = 10.0 ** rng.uniform(-12.0, -6.0, n)
    I[rng.random(n) < 0.05] = 0.0
    q = rng.integers(-1, 10, n).astype(np.int32)
    q[[5, 6]] = [-1, 7]
    if G > 1:                                                           # (one group alone would be NaN throughout)
        I[n - 2], T[n - 1] = np.nan, np.nan
        q[[n - 2, n - 1]] = [0, 1]
    L = rng.uniform(1e4, 1.2e6, n)
    L[7] = 1e10
    tred = 59.0 + rng.uniform(0.0, 1.0, G)
    freq = np.linspace(95.0, 55.0, F) if F > 1 else np.array([0.0 if G == 1 else 75.0])
    if F > 2:
        freq[1], freq[-1] = freq[0], 0.0
    alpha = rng.uniform(1e-6, 1e-5, F)
    if F > 1:
        alpha[F // 2] = 0.0
    return off, T, I, q, L, tred, freq, alpha


F_CASES = [1, 63, 64, 65, TILE - 1, TILE, TILE + 1]


@pytest.mark.parametrize("F", F_CASES)
@pytest.mark.parametrize("G", [1, 3, 130])
def test_kernel_bit_identical_to_the_restatement_on_synthetic_groups(pr, G, F):
    off, T, I, q, L, tred, freq, alpha = synthetic_groups(G, F, seed=1000 * G + F)
    assert TILE == 256 and (G < 130 or set(COUNTS) <= set(np.diff(off).tolist()))
    assert (q < 0).any() and (q > 3).any() and (I == 0).any() and np.isnan(I).sum() == np.isnan(T).sum() == (G > 1)
    yw = -((alpha[None, :] * L[:, None]) * spref.K20)
    assert (yw < -700.0).any() and (yw > -3.0).any() and len(set(tred.tolist())) == G
    assert F < 3 or (freq[0] == freq[1] and freq[-1] == 0.0 and (np.diff(freq) <= 0).all())
    zero = np.zeros(G)
    got = {}
    for name, qq, LL, tt, aa in (("plain", q, None, zero, None), ("absorbed", q, L, zero, alpha), ("null", None, None, zero, None),
                                 ("reduced", q, None, tred, None),
                                 ("reduced absorbed", q, L, tred, alpha)):
        H = got[name] = _device_spectrum(off, T, I, qq, LL, tt, freq, aa)
        ref = spref.spectrum_sum(off, T, I, qq, LL, tt, freq, aa)
        bad = np.argwhere(~((H.real == ref.real) | (np.isnan(H.real) & np.isnan(ref.real))))
        assert _bits(H, ref), (name, bad[:5])
    again = _device_spectrum(off, T, I, q, L, tred, freq, alpha)          # repeated calls are bit-equal
    assert _bits(again, got["reduced absorbed"])
    empty = np.flatnonzero(np.diff(off) == 0)
    assert all((got[name][empty] == 0).all() for name in got)           # empty groups are written: zeros
    assert not _bits(got["plain"], got["null"]) and not _bits(got["plain"], got["absorbed"])
    assert (freq == 0).all() or not _bits(got["plain"], got["reduced"])
    # tred = 0, no alpha: every column is the group's CW sum at that frequency, pressure_field's sum
    for k in sorted({0, F // 2, F - 1}):
        assert _bits(got["plain"][:, k], sref.cw_sum(off, T, I, q, freq[k])), k
    # the NaN T and the NaN I make exactly their groups NaN
    nan_groups = np.unique(np.repeat(np.arange(G), np.diff(off))[np.isnan(T) | np.isnan(I)])
    assert np.array_equal(np.flatnonzero(np.isnan(got["plain"].real).any(axis=1)), nan_groups)
    assert np.isnan(got["plain"].real[nan_groups]).all()


# ---- the error paths of the C entry ------------------------------------------------------------------------------------------

def test_c_entry_refuses_bad_arguments_before_writing_anything(pr_any):
    import torch
    from pygenray_amd import _lib
    Lb = _lib.load()
    dev = torch.device("cuda", 0)
    G, F = 3, 70
    off, T, I, q, L, tred, freq, alpha = synthetic_groups(G, F, seed=2)
    up = lambda a, dt_: torch.from_numpy(np.ascontiguousarray(a, dtype=dt_)).to(dev)   # noqa: E731
    d = dict(off=up(off, np.int64), T=up(T, float), I=up(I, float), L=up(L, float), tr=up(tred, float))
    re_, im_ = (torch.full((G * F,), MARK, dtype=torch.float64, device=dev) for _ in range(2))
    stream = torch.cuda.current_stream(dev).cuda_stream
    good = dict(off=d["off"].data_ptr(), G=G, T=d["T"].data_ptr(), I=d["I"].data_ptr(), L=d["L"].data_ptr(), tr=d["tr"].data_ptr(),
                freq=freq, alpha=alpha, nf=F, re=re_.data_ptr(), im=im_.data_ptr())

    def call(**kw):
        a = dict(good, **kw)
        host = lambda v: None if v is None else v.ctypes.data   # noqa: E731
        return Lb.pgr_spectrum_device(0, a["off"], a["G"], a["T"], a["I"], None, a["L"], a["tr"], host(a["freq"]),
                                      host(a["alpha"]), a["nf"], a["re"], a["im"], ctypes.c_void_p(stream))

    def with_value(v, k=F // 2):
        a = freq.copy()
        a[k] = v
        return a
    cases = [(dict(off=None), "null"), (dict(T=None), "null"), (dict(I=None), "null"), (dict(tr=None), "null"),
             (dict(freq=None), "null"), (dict(re=None), "null"), (dict(im=None), "null"),
             (dict(alpha=None), "go together"), (dict(L=None), "go together"),
             (dict(G=0), "n_groups"), (dict(G=-1), "n_groups"), (dict(G=2 ** 31), "too many groups"),
             (dict(nf=0), "n_freq"), (dict(nf=-5), "n_freq"), (dict(nf=65535 * TILE + 1), "n_freq"),
             (dict(freq=with_value(-1.0)), "freq must be"), (dict(freq=with_value(np.nan)), "freq must be"),
             (dict(freq=with_value(np.inf, F - 1)), "freq must be"), (dict(freq=with_value(-np.inf, 0)), "freq must be"),
             (dict(alpha=with_value(-1e-6) * 1e-7), "alpha must be"), (dict(alpha=with_value(np.nan) * 1e-7), "alpha must be"),
             (dict(alpha=with_value(np.inf, F - 1) * 1e-7), "alpha must be")]
    for kw, msg in cases:
        rc = call(**kw)
        err = Lb.pgr_last_error().decode()
        assert rc < 0 and "pgr_spectrum_device" in err and msg in err, (kw, rc, err)
    torch.cuda.synchronize(dev)
    assert (re_.cpu().numpy() == MARK).all() and (im_.cpu().numpy() == MARK).all()
    assert call() == 0 and call(L=None, alpha=None) == 0                 # and the same buffers with good arguments: written
    assert not (re_.cpu().numpy() == MARK).any() and not (im_.cpu().numpy() == MARK).any()
    with pytest.raises(_lib.PgrError, match="pgr_spectrum_device.*freq must be"):
        _lib.spectrum_device(0, good["off"], G, good["T"], good["I"], 0, 0, good["tr"], with_value(-1.0), None, good["re"],
                             good["im"], stream)
    with pytest.raises(ValueError, match="equal length"):
        _lib.spectrum_device(0, good["off"], G, good["T"], good["I"], 0, good["L"], good["tr"], freq, alpha[:-1], good["re"],
                             good["im"], stream)


# ---- fans -----------------------------------------------------------------------------------------------------------------

def _shoot(pr, env, resident, n=300, S=81, x1=80e3, K=40):
    return pr.shoot_rays(1000.0, 0.0, np.linspace(-20.0, 20.0, n), x1, S, env, flatearth=False, debug=False,
                         device_resident=resident, max_bounces=K)


def _in_place(fan):
    assert fan.device_resident and not any(k in fan.__dict__ for k in ("_ts", "_zs", "_ps"))


@pytest.fixture(scope="module")
def munk_fan(pr_any):
    """a 2001-ray Munk fan to 100 km, device resident, with a bounce log of 64 slots; four receivers; the last column and a
    middle one"""
    env = munk_env(pr_any)
    fan = _shoot(pr_any, env, True, n=2001, S=101, x1=100e3, K=64)
    return fan, env, DEPTHS[[100, 300, 500, 700]], [100, 37]


def test_transfer_function_is_pressure_field_at_every_frequency_bit_for_bit(pr, munk_fan):
    fan, env, d, cols = munk_fan
    freq = [50.0, 75.0, 75.37, 250.0]
    for kw in ({}, dict(absorption=0.05, surface_loss=0.5)):
        H = pr.transfer_function(fan, d, env, freq, range_indices=cols, flatearth=False, **kw)
        assert H.shape == (len(d), len(cols), 4) and H.dtype == np.complex128
        for k, f in enumerate(freq):
            p = pr.pressure_field(fan, d, env, f, flatearth=False, **kw)[:, cols]
            assert (np.abs(p) > 0).sum() >= 6 and _bits(H[:, :, k], p), (kw, f)
    _in_place(fan)
    # the source's own column is NaN, as in pressure_field; a default range_indices is the last column
    H0 = pr.transfer_function(fan, d, env, freq, range_indices=[0, -1], flatearth=False)
    default = pr.transfer_function(fan, d, env, freq, flatearth=False)
    assert np.isnan(H0[:, 0]).all() and default.shape == (len(d), 1, 4) and _bits(H0[:, 1], default[:, 0])
    # a reduction time per column turns every entry by its phase: within section 17's bound of the turned field
    tr = np.array([66.0, 24.0])
    Hr = pr.transfer_function(fan, d, env, freq, range_indices=cols, t_reduce=tr, flatearth=False)
    Hp = pr.transfer_function(fan, d, env, freq, range_indices=cols, flatearth=False)
    A = _group_amplitudes(pr, fan, d, env, cols)
    turned = Hp * np.exp(-2j * np.pi * np.asarray(freq)[None, None, :] * tr[None, :, None])
    assert (np.abs(Hr - turned) <= sref.FOURIER_REL * A[:, :, None]).all() and not _bits(Hr, Hp)
    # a transfer function that does not fit in the device's memory is refused before any kernel runs
    with pytest.raises(ValueError, match="bytes of device memory"):
        pr.transfer_function(fan, np.linspace(10.0, 4000.0, 20000), env, np.linspace(55.0, 95.0, 65535 * 256), range_indices=cols,
                             flatearth=False)
    _in_place(fan)


def _group_amplitudes(pr, fan, d, env, cols, **kw):
    """sum_a amp_a per (receiver, column) over the arrivals that add: those whose tube is not folded over a boundary"""
    a = pr.arrivals(fan, d, env, flatearth=False, range_indices=cols, **kw)
    n = len(cols)
    slot = np.repeat(np.arange(len(a.offsets) - 1), np.diff(a.offsets)) % n
    nb, ns = fan.bounce_counts(cols)
    alike = (nb[a.tube, slot] == nb[a.tube + 1, slot]) & (ns[a.tube, slot] == ns[a.tube + 1, slot])
    amp = np.where(alike, np.sqrt(a.intensity), 0.0)
    return np.array([amp[a.offsets[g]:a.offsets[g + 1]].sum() for g in range(len(a.offsets) - 1)]).reshape(len(d), n)


@pytest.mark.parametrize("which", ["munk", "sloping", "munk-dropped", "sloping-dropped"])
def test_fans_in_both_layouts_resident_and_host_give_one_answer(pr, which):
    """rows (munk) and sample-blocked (sloping) fans, with dropped rays skipped through the keep list: transfer_function of the
    device-resident fan and of the same fan on the host, bit for bit, with every kind of absorption"""
    env = {"munk": munk_env, "sloping": sloping_env, "munk-dropped": lambda p: munk_env(p, ztop=4200.0),
           "sloping-dropped": sloping_env_shallow_table}[which](pr)
    fan, eager = _shoot(pr, env, True), _shoot(pr, env, False)
    assert fan._dev._env.blocked_layout == which.startswith("sloping")
    assert (len(eager) < 300) == which.endswith("dropped") and len(eager) > 50 and fan._dev.N == 300
    d, cols = DEPTHS[::100], [80, 33, 0]
    freq = np.linspace(20.0, 30.0, 70)
    x = np.asarray(eager.rs[0])[cols]
    for kw in ({}, dict(absorption=([0.0, 300.0, 1200.0, 4000.0], [0.9, 0.5, 0.08, 0.2])), dict(absorption=pr.thorp_absorption)):
        H = pr.transfer_function(fan, d, env, freq, range_indices=cols, t_reduce=x / 1500.0, flatearth=False, **kw)
        host = pr.transfer_function(eager, d, env, freq, range_indices=cols, t_reduce=x / 1500.0, flatearth=False, **kw)
        assert H.shape == (len(d), 3, 70) and _bits(H, host)
        assert np.isnan(H[:, 2]).all() and not np.isnan(H[:, :2]).any() and (np.abs(H[:, :2]).max(axis=2) > 0).mean() > 0.2
    _in_place(fan)


# ---- absorption that follows the frequency ------------------------------------------------------------------------------------

def test_band_absorption_against_pressure_field_at_each_frequency_within_the_edge_weights(pr, munk_fan):
    """transfer_function(absorption=thorp_absorption) against pressure_field(absorption=thorp_absorption(f_k)) per frequency.
    The bound is derived: pressure_field's arrival carries amp0 sqrt(0.5 (g_k W_k + g_k+1 W_k+1) / (0.5 (g_k + g_k+1))), a mean
    of the two edge rays' weights with g >= 0, and transfer_function's carries amp0 sqrt(W(L_a)) with L_a between the edge
    lengths: both amplitudes lie between amp0 sqrt(Wmin) and amp0 sqrt(Wmax), W = 10^(-alpha_k L / 10) at the longer and the
    shorter edge ray, and the phases are identical.  So per group |dH| <= sum_a amp0_a (sqrt(Wmax_a) - sqrt(Wmin_a)) + 1e-12
    sum_a amp0_a (rounding).  Measured on the MI355X: the worst ratio to the bound is in DESIGN.md section 18."""
    fan, env, d, cols = munk_fan
    freq = np.array([1000.0, 1700.0, 3000.0])
    H = pr.transfer_function(fan, d, env, freq, range_indices=cols, absorption=pr.thorp_absorption, flatearth=False)
    H0 = pr.transfer_function(fan, d, env, freq, range_indices=cols, flatearth=False)
    a = pr.arrivals(fan, d, env, flatearth=False, range_indices=cols)
    n, G = len(cols), len(d) * len(cols)
    slot = np.repeat(np.arange(G), np.diff(a.offsets)) % n
    nb, ns = fan.bounce_counts(cols)
    alike = (nb[a.tube, slot] == nb[a.tube + 1, slot]) & (ns[a.tube, slot] == ns[a.tube + 1, slot])
    amp0 = np.where(alike, np.sqrt(a.intensity), 0.0)
    PL = pr.path_length(fan, env, flatearth=False, range_indices=cols)                  # (M, n)
    L0, L1 = PL[a.tube, slot], PL[a.tube + 1, slot]
    per_group = lambda v: np.array([v[a.offsets[g]:a.offsets[g + 1]].sum() for g in range(G)]).reshape(len(d), n)   # noqa: E731
    worst = 0.0
    for k, f in enumerate(freq):
        alpha = pr.thorp_absorption(f) / 1000.0
        Wmax, Wmin = 10.0 ** (-alpha * np.minimum(L0, L1) / 10.0), 10.0 ** (-alpha * np.maximum(L0, L1) / 10.0)
        bound = per_group(amp0 * (np.sqrt(Wmax) - np.sqrt(Wmin))) + 1e-12 * per_group(amp0)
        p = pr.pressure_field(fan, d, env, f, absorption=float(pr.thorp_absorption(f)), flatearth=False)[:, cols]
        err = np.abs(H[:, :, k] - p)
        lit = per_group(amp0) > 0
        print(f"band absorption at {f} Hz: worst |H - p| / bound {(err[lit] / bound[lit]).max():.3e}, bound / (sum amp0 sqrt Wmin) "
              f"{(bound[lit] / per_group(amp0 * np.sqrt(Wmin))[lit]).max():.3e}, |H - H0| / bound "
              f"{(np.abs(H[:, :, k] - H0[:, :, k])[lit] / bound[lit]).min():.3e}")
        worst = max(worst, float((err[lit] / bound[lit]).max()))
        assert (err <= bound).all(), (f, err, bound)
        # not vacuous: absorption changes H by far more than the bound, and the bound is small against the field's scale
        assert lit.sum() >= 6 and (np.abs(H[:, :, k] - H0[:, :, k])[lit] > 10 * bound[lit]).all()
        assert (bound[lit] < 0.01 * per_group(amp0 * np.sqrt(Wmin))[lit]).all()
    print(f"band absorption: worst ratio to the bound {worst:.3e}")
    # L_a itself: the restatement's three operations on path_length and Arrivals.w, bit for bit
    from pygenray_amd._fan_frame import _arrival_terms
    from pygenray_amd._fan_frame import _arrival_lengths
    from pygenray_amd._fan_frame import _FanFrame
    from pygenray_amd._fan_frame import _needs_counts
    from pygenray_amd.ray_objects import _columns
    fr = _FanFrame(fan, d, env, False, "test").to_device(0)
    _, tube, w, _, _, _, col = _arrival_terms(fr, _columns(cols, len(fr.x)), None, None, _needs_counts(fan))
    La = _arrival_lengths(fr, col, tube, w).cpu().numpy()
    assert np.array_equal(tube.cpu().numpy(), a.tube) and np.array_equal(w.cpu().numpy(), a.w)
    assert np.array_equal(La, spref.arrival_lengths(L0, L1, a.w)) and len(La) > 20
    assert (La >= np.minimum(L0, L1)).all() and (La <= np.maximum(L0, L1)).all() and (L0 != L1).any()
    _in_place(fan)


# ---- received_waveform ----------------------------------------------------------------------------------------------------

def test_waveform_of_a_gaussian_source_is_received_signal(pr_any, munk_fan):
    """tests/test_spectrum_host.py's synthesis identity end to end, with its bound: received_waveform of the Gaussian source
    centred at tc is received_signal at t - tc.  In either arithmetic.  The source is the CPU test's (B = 20 Hz, tc = 9 sigma,
    dt = sigma / 4, so 1 / (2 dt) = 151 Hz); the carrier is 250 Hz, not the CPU test's 75 Hz, which received_waveform refuses
    at this dt: the band 75 Hz +- 151 Hz would reach negative frequencies (the restatement takes them, the product does not).
    The bound's terms hold at 250 Hz: the phase rounding of f T at T = 67 s is 1.1e-11 rad."""
    fan, env, d, cols = munk_fan
    f, B = 250.0, spref.SYNTH_B
    assert spref.SYNTH_F < 1.0 / (2.0 * sref.pulse_sigma(B) / 4) <= f
    sigma = sref.pulse_sigma(B)
    dt = sigma / 4
    source, tc = spref.gaussian_source(sigma, dt)
    a = pr_any.arrivals(fan, d, env, flatearth=False, range_indices=cols)
    n = len(cols)
    slot = np.repeat(np.arange(len(a.offsets) - 1), np.diff(a.offsets)) % n
    assert all((slot == c).sum() >= 4 for c in range(n)) and len(a) > 20
    windows = [spref.covering_fft(a.time[slot == c].min(), a.time[slot == c].max(), sigma, dt, len(source)) for c in range(n)]
    t0, n_fft = np.array([w[0] for w in windows]), max(w[1] for w in windows)
    assert n_fft <= 8192
    kw = dict(range_indices=cols, flatearth=False, surface_loss=0.5)
    u = pr_any.received_waveform(fan, d, env, source, dt, f, t0, n_fft=n_fft, **kw)
    ref = pr_any.received_signal(fan, d, env, f, B, t0 - tc, dt, n_fft, **kw)
    assert u.shape == ref.shape == (len(d), n, n_fft) and u.dtype == np.complex128
    A = _group_amplitudes(pr_any, fan, d, env, cols, surface_loss=0.5)
    err = np.abs(u - ref).max(axis=2)
    lit = A > 0
    print(f"received_waveform against received_signal: worst |u - ref| is {(err[lit] / (spref.SYNTH_REL * A[lit])).max():.3e} of "
          f"the bound; n_fft {n_fft}, {len(a)} arrivals")
    assert (err <= spref.SYNTH_REL * A).all(), (err, A)
    assert lit.sum() >= 6 and (np.abs(ref).max(axis=2)[lit] > 1e6 * spref.SYNTH_REL * A[lit]).all()
    # n_times keeps the first samples; the default n_fft is the next power of two >= n_times + len(source)
    first = pr_any.received_waveform(fan, d, env, source, dt, f, t0, n_times=n_fft - len(source), **kw)
    assert first.shape[2] == n_fft - len(source) and _bits(first, u[:, :, :n_fft - len(source)])
    _in_place(fan)


def test_waveform_identity_holds_in_contracted_arithmetic():
    from pygenray_amd import _lib
    if _lib.ARITH != "reference":
        pytest.skip("this IS the contracted process")
    if not os.path.exists(_lib.CONTRACTED_LIB):
        pytest.fail("libpgr_hip_fma.so is not built (__graft_entry__.build() builds it beside the product)")
    out = subprocess.run([sys.executable, "-m", "pytest", "-q", "-m", "gpu", "-x", "-p", "no:cacheprovider", "-k", "waveform_of_a_gaussian",
                          os.path.join(ROOT, "tests", "test_spectrum.py")],
                         cwd=ROOT, env=dict(os.environ, PGR_ARITH="contracted"), capture_output=True, text=True, timeout=600)
    tail = out.stdout[-3000:] + out.stderr[-1500:]
    assert out.returncode == 0 and " passed" in out.stdout and "failed" not in out.stdout, tail
