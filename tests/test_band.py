"""Band-averaged transmission loss on the GPU (csrc/pgr_band.h): the kernel alone through ``_lib.band_power_sum`` against the
restatement of tests/band_reference.py on synthetic arrivals aimed at its staging, tile and lane seams, and against the spectrum
entries' own output reduced on the host; the error paths of the C entry; ``band_intensity`` against the defined reduction of
``transfer_function`` on a Munk fan, resident and host, with a complex bottom and with absorption that follows the frequency; the
beam twins against ``beam_transfer_function``; and Lloyd's mirror over a band from ``shoot_rays`` against the closed form."""
import ctypes

import numpy as np
import pytest

import band_reference as bref
import beam_pressure_reference as bp
import coherent_reference as cref
import reflection_reference as rref
from test_band_host import check_lloyd_band
from test_spectrum import COUNTS, synthetic_groups
from tube_gpu import DEPTHS, _same, munk_env, pr, pr_any  # noqa: F401

pytestmark = pytest.mark.gpu

PAD = 130                    # entries before and behind the output that must stay as they were
MARK = -7.25


class _Lists:
    """arrival lists and a band on the device, and pgr_band_power_device on them"""

    def __init__(self, off, T, I, q, phi, L):
        import torch
        self.dev = torch.device("cuda", 0)
        self.stream = torch.cuda.current_stream(self.dev).cuda_stream
        up = lambda a, dt_: torch.from_numpy(np.ascontiguousarray(a, dtype=dt_)).to(self.dev)   # noqa: E731
        self.G = len(off) - 1
        # (one entry more than the lists hold, so that an empty list is no null pointer)
        self.keep = dict(off=up(off, np.int64), T=up(np.append(T, 0.0), float), I=up(np.append(I, 0.0), float),
                         q=up(np.append(q, 0), np.int32), phi=up(np.append(phi, 0.0), float), L=up(np.append(L, 0.0), float))
        self.ptr = {k: v.data_ptr() for k, v in self.keep.items()}

    def power(self, freq, alpha, wf, q=True, phi=False):
        """-> out (G,), the sentinels before and behind it checked untouched and every entry checked written"""
        import torch
        from pygenray_amd import _lib
        p, G = self.ptr, self.G
        buf = torch.full((PAD + G + PAD,), MARK, dtype=torch.float64, device=self.dev)
        _lib.band_power_sum(0, p["off"], G, p["T"], p["I"], p["q"] if q else 0, p["phi"] if phi else 0,
                            0 if alpha is None else p["L"], freq, alpha, wf, buf.data_ptr() + 8 * PAD, self.stream)
        h = buf.cpu().numpy()
        assert (h[:PAD] == MARK).all() and (h[PAD + G:] == MARK).all() and not (h[PAD:PAD + G] == MARK).any()
        return h[PAD:PAD + G].copy()

    def spectrum(self, freq, alpha, q=True, phi=False):
        """the same lists through pgr_spectrum_device / pgr_spectrum_device_phi with zero tred -> (re, im), each (G, F)"""
        import torch
        from pygenray_amd import _lib
        p, G, F = self.ptr, self.G, len(freq)
        tred = torch.zeros(G, dtype=torch.float64, device=self.dev)
        re, im = (torch.full((G, F), MARK, dtype=torch.float64, device=self.dev) for _ in range(2))
        head = (0, p["off"], G, p["T"], p["I"], p["q"] if q else 0)
        tail = (0 if alpha is None else p["L"], tred.data_ptr(), freq, alpha, re.data_ptr(), im.data_ptr(), self.stream)
        if phi:
            _lib.spectrum_phi_device(*head, p["phi"], *tail)
        else:
            _lib.spectrum_device(*head, *tail)
        return re.cpu().numpy(), im.cpu().numpy()


def band_weights(F, seed):
    """unequal weights over four decades with an exact 0.0 (F > 1)"""
    w = 10.0 ** np.random.default_rng(seed).uniform(-3.0, 1.0, F)
    if F > 1:
        w[F // 3] = 0.0
    return w


F_CASES = [1, 63, 64, 65, 255, 256, 257, 513]
VARIANTS = (("plain", True, False, False), ("null q", False, False, False), ("lagged", True, True, False),
            ("absorbed", True, False, True), ("lagged absorbed", True, True, True))


@pytest.mark.parametrize("F", F_CASES)
@pytest.mark.parametrize("G", [1, 3, 130])
def test_kernel_bit_identical_to_the_restatement_on_synthetic_groups(pr, G, F):
    off, T, I, q, L, _, freq, alpha = synthetic_groups(G, F, seed=2000 * G + F)
    phi = rref.synthetic_lags((len(T),), seed=G + F)
    wf = band_weights(F, G * F)
    assert G < 130 or set(COUNTS) <= set(np.diff(off).tolist())
    assert (q < 0).any() and (q > 3).any() and np.isnan(I).sum() == np.isnan(T).sum() == (G > 1)
    assert (np.abs(phi[np.isfinite(phi)]) > 1e3).any() and np.isnan(phi).sum() == 1
    assert F == 1 or ((wf == 0).sum() == 1 and len(set(wf.tolist())) == F)
    lists = _Lists(off, T, I, q, phi, L)
    got = {}
    for name, use_q, use_phi, absorb in VARIANTS:
        aa = alpha if absorb else None
        out = got[name] = lists.power(freq, aa, wf, q=use_q, phi=use_phi)
        re, im = bref.band_terms(off, T, I, q if use_q else None, phi if use_phi else None, L if absorb else None, freq, aa)
        ref = bref.reduce_band(re, im, wf)
        bad = np.flatnonzero(~((out == ref) | (np.isnan(out) & np.isnan(ref))))
        assert out.shape == (G,) and _same(out, ref), (name, bad[:5], out[bad[:5]], ref[bad[:5]])
        assert _same(lists.power(freq, aa, wf, q=use_q, phi=use_phi), out)      # repeated calls are bit-equal
        if name in ("plain", "lagged absorbed"):
            # the same lists through the spectrum entries, reduced on the host in the defined order
            dre, dim = lists.spectrum(freq, aa, q=use_q, phi=use_phi)
            assert _same(dre, re) and _same(dim, im) and _same(bref.reduce_band(dre, dim, wf), out), name
    empty = np.flatnonzero(np.diff(off) == 0)
    assert all((got[name][empty] == 0).all() and not np.signbit(got[name][empty]).any() for name in got)   # +0.0, written
    # the NaN T and the NaN I make exactly their groups NaN; the NaN lag its group too
    grp = np.repeat(np.arange(G), np.diff(off))
    nan_groups = np.unique(grp[np.isnan(T) | np.isnan(I)])
    assert np.array_equal(np.flatnonzero(np.isnan(got["plain"])), nan_groups)
    lag_groups = np.unique(grp[(np.isnan(T) | np.isnan(I) | np.isnan(phi)) & (q >= 0)])
    assert np.array_equal(np.flatnonzero(np.isnan(got["lagged"])), lag_groups)
    assert (np.nan_to_num(got["plain"]) > 0).any() and not _same(got["plain"], got["absorbed"])
    if (freq > 0).any():
        assert not _same(got["plain"], got["null q"]) and not _same(got["plain"], got["lagged"])


def test_one_frequency_with_weight_one_is_the_squared_spectrum_entry(pr):
    off, T, I, q, L, _, _, _ = synthetic_groups(130, 1, seed=5)
    lists = _Lists(off, T, I, q, np.zeros(len(T)), L)
    for f in (75.0, 0.0):
        re, im = lists.spectrum([f], None)
        out = lists.power([f], None, [1.0])
        assert _same(out, (re * re + im * im)[:, 0]) and (np.nan_to_num(out) > 0).any()


# ---- the error paths of the C entry --------------------------------------------------------------------------------------------

def test_c_entry_refuses_bad_arguments_before_writing_anything(pr_any):
    import torch
    from pygenray_amd import _lib
    Lb = _lib.load()
    G, F = 3, 70
    off, T, I, q, L, _, freq, alpha = synthetic_groups(G, F, seed=2)
    lists = _Lists(off, T, I, q, np.zeros(len(T)), L)
    wf = band_weights(F, 1)
    out = torch.full((G,), MARK, dtype=torch.float64, device=lists.dev)
    p = lists.ptr
    good = dict(off=p["off"], G=G, T=p["T"], I=p["I"], L=p["L"], freq=freq, alpha=alpha, wf=wf, nf=F, out=out.data_ptr())

    def call(**kw):
        a = dict(good, **kw)
        host = lambda v: None if v is None else v.ctypes.data   # noqa: E731
        return Lb.pgr_band_power_device(0, a["off"], a["G"], a["T"], a["I"], None, None, a["L"], host(a["freq"]), host(a["alpha"]),
                                        host(a["wf"]), a["nf"], a["out"], ctypes.c_void_p(lists.stream))

    def with_value(a, v, k=F // 2):
        a = a.copy()
        a[k] = v
        return a
    cases = [(dict(off=None), "null"), (dict(T=None), "null"), (dict(I=None), "null"), (dict(freq=None), "null"),
             (dict(wf=None), "null"), (dict(out=None), "null"),
             (dict(alpha=None), "go together"), (dict(L=None), "go together"),
             (dict(G=0), "n_groups"), (dict(G=-1), "n_groups"), (dict(G=2 ** 31), "too many groups"),
             (dict(nf=0), "n_freq"), (dict(nf=-5), "n_freq"), (dict(nf=65535 * 256 + 1), "n_freq"),
             (dict(freq=with_value(freq, -1.0)), "freq must be"), (dict(freq=with_value(freq, np.nan)), "freq must be"),
             (dict(freq=with_value(freq, np.inf, F - 1)), "freq must be"),
             (dict(alpha=with_value(alpha, -1e-13)), "alpha must be"), (dict(alpha=with_value(alpha, np.nan)), "alpha must be"),
             (dict(alpha=with_value(alpha, np.inf, F - 1)), "alpha must be"),
             (dict(wf=with_value(wf, -1e-300)), "wf must be"), (dict(wf=with_value(wf, np.nan, 0)), "wf must be"),
             (dict(wf=with_value(wf, np.inf, F - 1)), "wf must be"), (dict(wf=with_value(wf, -np.inf)), "wf must be")]
    for kw, msg in cases:
        rc = call(**kw)
        err = Lb.pgr_last_error().decode()
        assert rc < 0 and "pgr_band_power_device" in err and msg in err, (kw, rc, err)
    torch.cuda.synchronize(lists.dev)
    assert (out.cpu().numpy() == MARK).all()
    assert call() == 0 and call(L=None, alpha=None) == 0                 # and the same buffer with good arguments: written
    assert not (out.cpu().numpy() == MARK).any()
    with pytest.raises(_lib.PgrError, match="pgr_band_power_device.*wf must be"):
        _lib.band_power_sum(0, p["off"], G, p["T"], p["I"], 0, 0, 0, freq, None, with_value(wf, -1.0), good["out"], lists.stream)


# ---- fans -----------------------------------------------------------------------------------------------------------------

SAND = (1700.0, 1800.0, 0.5)
FAN_DEPTHS = DEPTHS[40:990:19]                       # 50 depths, 90 m ... 5.7 km
COLS = [100, 37, 0]
FREQ = np.linspace(60.0, 90.0, 65)


def _shoot(pr, env, resident):
    return pr.shoot_rays(1000.0, 0.0, np.linspace(-20.0, 20.0, 2001), 100e3, 101, env, flatearth=False, debug=False,
                         device_resident=resident, max_bounces=64)


def _in_place(fan):
    assert fan.device_resident and not any(k in fan.__dict__ for k in ("_ts", "_zs", "_ps"))


@pytest.fixture(scope="module")
def munk_fan(pr):
    """a 2001-ray Munk fan to 100 km with a bounce log of 64 slots, device resident and the same fan on the host"""
    env = munk_env(pr)
    return _shoot(pr, env, True), _shoot(pr, env, False), env


def _reduced(H, wf):
    """the defined reduction of a transfer function H (R, n, F) -> (R, n)"""
    R, n, F = H.shape
    return bref.reduce_band(H.real.reshape(R * n, F), H.imag.reshape(R * n, F), wf).reshape(R, n)


def test_band_intensity_is_the_defined_reduction_of_transfer_function(pr, munk_fan):
    fan, eager, env = munk_fan
    assert len(FAN_DEPTHS) == 50
    shaped = np.linspace(1.0, 9.0, len(FREQ)) / 5.0
    for kw, weights in ((dict(), None), (dict(bottom_loss=pr.fluid_halfspace(*SAND)), shaped),
                        (dict(absorption=pr.thorp_absorption, surface_loss=0.5), shaped)):
        opt = dict(range_indices=COLS, flatearth=False, **kw)
        P = pr.band_intensity(fan, FAN_DEPTHS, env, FREQ, weights=weights, **opt)
        _in_place(fan)
        assert P.shape == (50, 3) and P.dtype == np.float64
        assert _same(pr.band_intensity(eager, FAN_DEPTHS, env, FREQ, weights=weights, **opt), P)     # resident and host
        H = pr.transfer_function(fan, FAN_DEPTHS, env, FREQ, **opt)
        wf = np.full(len(FREQ), 1.0 / len(FREQ)) if weights is None else shaped
        assert _same(P, _reduced(H, wf))
        # the source's own column is NaN; elsewhere most receivers are lit
        assert np.isnan(P[:, 2]).all() and not np.isnan(P[:, :2]).any() and (P[:, :2] > 0).mean() > 0.5
        tl = pr.band_transmission_loss(fan, FAN_DEPTHS, env, FREQ, weights=weights, **opt)
        with np.errstate(divide="ignore"):
            assert _same(tl, -10.0 * np.log10(P)) and (tl[:, :2][P[:, :2] > 0] > 40.0).all()
    _in_place(fan)
    # the weights, the complex bottom's phase and the absorption matter
    opt = dict(range_indices=COLS, flatearth=False)
    plain = pr.band_intensity(fan, FAN_DEPTHS, env, FREQ, **opt)
    assert not _same(plain, pr.band_intensity(fan, FAN_DEPTHS, env, FREQ, weights=shaped, **opt))
    sand = pr.fluid_halfspace(*SAND)
    assert not _same(pr.band_intensity(fan, FAN_DEPTHS, env, FREQ, bottom_loss=sand, **opt),
                     pr.band_intensity(fan, FAN_DEPTHS, env, FREQ, bottom_loss=sand.loss, **opt))
    # a default range_indices is the last column
    one = pr.band_intensity(fan, FAN_DEPTHS, env, FREQ, flatearth=False)
    assert one.shape == (50, 1) and _same(one[:, 0], plain[:, 0])
    _in_place(fan)


def test_one_frequency_is_the_squared_magnitude_of_pressure_field(pr, munk_fan):
    fan, eager, env = munk_fan
    for kw in (dict(), dict(bottom_loss=pr.fluid_halfspace(*SAND), surface_loss=0.5)):
        for f in (75.0, 250.0):
            p = pr.pressure_field(fan, FAN_DEPTHS, env, f, flatearth=False, **kw)[:, COLS]
            P = pr.band_intensity(fan, FAN_DEPTHS, env, [f], weights=[1.0], range_indices=COLS, flatearth=False, **kw)
            assert _same(P, p.real * p.real + p.imag * p.imag) and (P[:, :2] > 0).sum() >= 20 and np.isnan(P[:, 2]).all()
    _in_place(fan)


def test_an_output_that_does_not_fit_is_refused_before_any_kernel(pr, munk_fan, monkeypatch):
    import torch
    fan, eager, env = munk_fan
    need = 8 * len(FAN_DEPTHS) * len(COLS)
    monkeypatch.setattr(torch.cuda, "mem_get_info", lambda *a: (need - 1, 10 ** 12))
    for name in ("band_intensity", "band_transmission_loss", "beam_band_intensity", "beam_band_transmission_loss"):
        with pytest.raises(ValueError, match=f"the band intensity needs {need} bytes of device memory.*{need - 1} are free"):
            getattr(pr, name)(fan, FAN_DEPTHS, env, FREQ, range_indices=COLS, flatearth=False)
    monkeypatch.undo()
    _in_place(fan)


def test_beam_band_intensity_is_the_defined_reduction_of_beam_transfer_function(pr, munk_fan):
    fan, eager, env = munk_fan
    d = FAN_DEPTHS[::5]
    shaped = np.linspace(1.0, 9.0, len(FREQ)) / 5.0
    for kw in (dict(), dict(min_width=25.0, curvature=False, surface_loss=0.5, absorption=pr.thorp_absorption)):
        opt = dict(range_indices=COLS, flatearth=False, **kw)
        P = pr.beam_band_intensity(fan, d, env, FREQ, weights=shaped, **opt)
        _in_place(fan)
        assert _same(pr.beam_band_intensity(eager, d, env, FREQ, weights=shaped, **opt), P)
        H = pr.beam_transfer_function(fan, d, env, FREQ, **opt)
        assert P.shape == (len(d), 3) and _same(P, _reduced(H, shaped))
        assert np.isnan(P[:, 2]).all() and not np.isnan(P[:, :2]).any() and (P[:, :2] > 0).mean() > 0.5
        tl = pr.beam_band_transmission_loss(fan, d, env, FREQ, weights=shaped, **opt)
        with np.errstate(divide="ignore"):
            assert _same(tl, -10.0 * np.log10(P))
    for name in ("beam_band_intensity", "beam_band_transmission_loss"):
        with pytest.raises(ValueError, match="does not yet apply a complex bottom phase"):
            getattr(pr, name)(fan, d, env, FREQ, bottom_loss=pr.fluid_halfspace(*SAND), range_indices=COLS, flatearth=False)
    _in_place(fan)


# ---- physics on a HIP fan -------------------------------------------------------------------------------------------------------

def test_lloyds_mirror_over_a_band_from_shoot_rays(pr):
    env = cref.lloyd_env(pr)
    fan = pr.shoot_rays(bp.LLOYD_ZS, 0.0, np.linspace(-bp.EXACT_APERTURE, bp.EXACT_APERTURE, bp.EXACT_N), 5e3, 51, env,
                        flatearth=False, debug=False, device_resident=True, max_bounces=4)
    assert len(fan) == bp.EXACT_N == 4001 and (fan.n_botts == 0).all() and fan.n_surfs.max() == 1
    cols = np.array([20, 30, 40, 50])
    assert np.array_equal(np.asarray(fan.rs[0])[cols], bp.EXACT_RANGES)
    P = pr.band_intensity(fan, bp.LLOYD_DEPTHS, env, bref.BAND_FREQ, range_indices=cols, flatearth=False)
    worst = check_lloyd_band(P, bref.BAND_LLOYD_MEASURED, "band_intensity from shoot_rays")
    Pb = pr.beam_band_intensity(fan, bp.LLOYD_DEPTHS, env, bref.BAND_FREQ, min_width=10.0, range_indices=cols, flatearth=False)
    worst_beam = check_lloyd_band(Pb, bref.BAND_LLOYD_BEAM_MEASURED, "beam_band_intensity from shoot_rays, min_width 10 m")
    _in_place(fan)
    tl = pr.band_transmission_loss(fan, bp.LLOYD_DEPTHS, env, bref.BAND_FREQ, range_indices=cols, flatearth=False)
    print(f"  worst e: tubes {worst:.6e}, beams {worst_beam:.6e}; band TL {tl.min():.2f} ... {tl.max():.2f} dB")
    assert _same(tl, -10.0 * np.log10(P)) and 55.0 < tl.min() and tl.max() < 100.0
