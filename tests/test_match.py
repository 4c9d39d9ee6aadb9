"""Matched-field processing on the GPU (csrc/pgr_match.h): the kernel alone through ``_lib.matched_field_sum`` against the
restatement of tests/match_reference.py on synthetic arrivals aimed at its staging, tile and lane seams, and against the spectrum
entries' own output per element reduced on the host; the error paths of the C entry; ``matched_field`` against the defined
reduction of the elements' ``transfer_function`` on three Munk fans, resident and host, with a complex bottom and with absorption
that follows the frequency; the beam twin against ``beam_transfer_function``; and localisation on Lloyd's mirror from eight
``shoot_rays`` fans against the processor on closed-form replicas."""
import ctypes

import numpy as np
import pytest

import band_reference as bref
import beam_pressure_reference as bp
import coherent_reference as cref
import match_reference as mref
import reflection_reference as rref
from test_band import COLS, FAN_DEPTHS, FREQ, SAND, _in_place, band_weights
from test_match_host import check_lloyd_match
from test_spectrum import COUNTS, synthetic_groups
from tube_gpu import _same, munk_env, pr, pr_any  # noqa: F401

pytestmark = pytest.mark.gpu

PAD = 130                    # entries before and behind the output that must stay as they were
MARK = -7.25


class _Lists:
    """the arrival lists of N elements x G cells on the device, and pgr_matched_field_device on them"""

    def __init__(self, N, off, T, I, q, phi, L):
        import torch
        self.dev = torch.device("cuda", 0)
        self.stream = torch.cuda.current_stream(self.dev).cuda_stream
        up = lambda a, dt_: torch.from_numpy(np.ascontiguousarray(a, dtype=dt_)).to(self.dev)   # noqa: E731
        self.N, self.G = N, (len(off) - 1) // N
        assert self.N * self.G == len(off) - 1
        # (one entry more than the lists hold, so that an empty list is no null pointer)
        self.keep = dict(off=up(off, np.int64), T=up(np.append(T, 0.0), float), I=up(np.append(I, 0.0), float),
                         q=up(np.append(q, 0), np.int32), phi=up(np.append(phi, 0.0), float), L=up(np.append(L, 0.0), float))
        self.ptr = {k: v.data_ptr() for k, v in self.keep.items()}

    def power(self, freq, alpha, wf, data, normalize, q=True, phi=False):
        """-> out (G,), the sentinels before and behind it checked untouched and every entry checked written"""
        import torch
        from pygenray_amd import _lib
        p, G = self.ptr, self.G
        buf = torch.full((PAD + G + PAD,), MARK, dtype=torch.float64, device=self.dev)
        _lib.matched_field_sum(0, p["off"], self.N, G, p["T"], p["I"], p["q"] if q else 0, p["phi"] if phi else 0,
                               0 if alpha is None else p["L"], freq, alpha, wf, data, normalize, buf.data_ptr() + 8 * PAD,
                               self.stream)
        h = buf.cpu().numpy()
        assert (h[:PAD] == MARK).all() and (h[PAD + G:] == MARK).all() and not (h[PAD:PAD + G] == MARK).any()
        return h[PAD:PAD + G].copy()

    def spectrum(self, freq, alpha, q=True, phi=False):
        """the same lists through pgr_spectrum_device / pgr_spectrum_device_phi with zero tred, one call per element ->
        (re, im), each (N, G, F)"""
        import torch
        from pygenray_amd import _lib
        p, N, G, F = self.ptr, self.N, self.G, len(freq)
        tred = torch.zeros(G, dtype=torch.float64, device=self.dev)
        re, im = (torch.full((N, G, F), MARK, dtype=torch.float64, device=self.dev) for _ in range(2))
        for j in range(N):
            head = (0, p["off"] + 8 * j * G, G, p["T"], p["I"], p["q"] if q else 0)
            tail = (0 if alpha is None else p["L"], tred.data_ptr(), freq, alpha, re[j].data_ptr(), im[j].data_ptr(), self.stream)
            if phi:
                _lib.spectrum_phi_device(*head, p["phi"], *tail)
            else:
                _lib.spectrum_device(*head, *tail)
        return re.cpu().numpy(), im.cpu().numpy()


def snapshot(N, F, seed):
    """a complex snapshot (N, F) with moduli over two decades"""
    rng = np.random.default_rng(seed)
    return (10.0 ** rng.uniform(-1.0, 1.0, (N, F))) * np.exp(2j * np.pi * rng.random((N, F)))


# (elements, cells, frequencies): every N, G and F of the issue, the staging seams of COUNTS wherever N * G >= 6
SHAPES = [(1, 1, 1), (2, 1, 63), (1, 3, 64), (5, 3, 65), (2, 3, 257), (1, 130, 63), (2, 130, 65), (5, 130, 1), (5, 1, 513),
          (2, 130, 257)]
VARIANTS = (("plain", True, False, False), ("null q", False, False, False), ("lagged", True, True, False),
            ("absorbed", True, False, True), ("lagged absorbed", True, True, True))


@pytest.mark.parametrize("N,G,F", SHAPES)
def test_kernel_bit_identical_to_the_restatement_on_synthetic_groups(pr, N, G, F):
    E = N * G
    off, T, I, q, L, _, freq, alpha = synthetic_groups(E, F, seed=3000 * E + F)
    phi = rref.synthetic_lags((len(T),), seed=E + F)
    if G == 1 and E > 1:                                               # (one cell alone would be NaN throughout)
        T[np.isnan(T)], I[np.isnan(I)], phi[np.isnan(phi)] = 61.0, 1e-9, 0.5
    wf = band_weights(F, E * F)
    data = snapshot(N, F, E + 7 * F)
    assert E < 6 or set(COUNTS) <= set(np.diff(off).tolist())
    assert (q < 0).any() and (q > 3).any() and np.isnan(I).sum() == np.isnan(T).sum() == (G > 1)
    assert (np.abs(phi[np.isfinite(phi)]) > 1e3).any() and np.isnan(phi).sum() == (G > 1 or E == 1)
    lists = _Lists(N, off, T, I, q, phi, L)
    got = {}
    for name, use_q, use_phi, absorb in VARIANTS:
        aa = alpha if absorb else None
        re, im = mref.match_terms(off, N, T, I, q if use_q else None, phi if use_phi else None, L if absorb else None, freq, aa)
        for normalize in (False, True):
            out = got[name, normalize] = lists.power(freq, aa, wf, data, normalize, q=use_q, phi=use_phi)
            ref = mref.reduce_match(re, im, data, wf, normalize)
            bad = np.flatnonzero(~((out == ref) | (np.isnan(out) & np.isnan(ref))))
            assert out.shape == (G,) and _same(out, ref), (name, normalize, bad[:5], out[bad[:5]], ref[bad[:5]])
            assert _same(lists.power(freq, aa, wf, data, normalize, q=use_q, phi=use_phi), out)    # repeated calls are bit-equal
            if name in ("plain", "lagged absorbed"):
                # the same lists through the spectrum entries per element, reduced on the host in the defined order
                dre, dim = lists.spectrum(freq, aa, q=use_q, phi=use_phi)
                assert _same(dre, re) and _same(dim, im) and _same(mref.reduce_match(dre, dim, data, wf, normalize), out), name
    cell = np.repeat(np.arange(E), np.diff(off)) % G
    reached = np.isin(np.arange(G), cell)
    for key, out in got.items():
        assert (out[~reached] == 0).all() and not np.signbit(out[~reached]).any()                   # +0.0, written
    # the NaN T and the NaN I make exactly their cells NaN; the NaN lag its cell too
    nan_cells = np.unique(cell[np.isnan(T) | np.isnan(I)])
    lag_cells = np.unique(cell[(np.isnan(T) | np.isnan(I) | np.isnan(phi)) & (q >= 0)])
    for normalize in (False, True):
        assert np.array_equal(np.flatnonzero(np.isnan(got["plain", normalize])), nan_cells)
        assert np.array_equal(np.flatnonzero(np.isnan(got["lagged", normalize])), lag_cells)
        assert (np.nan_to_num(got["plain", normalize]) > 0).any()
    assert not _same(got["plain", False], got["absorbed", False]) and not _same(got["plain", False], got["plain", True])
    if (freq > 0).any():
        assert not _same(got["plain", False], got["null q", False]) and not _same(got["plain", False], got["lagged", False])


def test_one_element_with_unit_data_is_the_band_power_entry(pr):
    from pygenray_amd import _lib
    import torch
    off, T, I, q, L, _, freq, alpha = synthetic_groups(130, 65, seed=5)
    lists = _Lists(1, off, T, I, q, np.zeros(len(T)), L)
    wf = band_weights(65, 3)
    out = lists.power(freq, alpha, wf, np.ones((1, 65), dtype=complex), False)
    band = torch.empty(130, dtype=torch.float64, device=lists.dev)
    p = lists.ptr
    _lib.band_power_sum(0, p["off"], 130, p["T"], p["I"], p["q"], 0, p["L"], freq, alpha, wf, band.data_ptr(), lists.stream)
    assert _same(out, band.cpu().numpy()) and (np.nan_to_num(out) > 0).any()


# ---- the error paths of the C entry --------------------------------------------------------------------------------------------

def test_c_entry_refuses_bad_arguments_before_writing_anything(pr_any):
    import torch
    from pygenray_amd import _lib
    Lb = _lib.load()
    N, G, F = 2, 3, 70
    off, T, I, q, L, _, freq, alpha = synthetic_groups(N * G, F, seed=2)
    lists = _Lists(N, off, T, I, q, np.zeros(len(T)), L)
    wf = band_weights(F, 1)
    data = snapshot(N, F, 4)
    dr, di = np.ascontiguousarray(data.real), np.ascontiguousarray(data.imag)
    out = torch.full((G,), MARK, dtype=torch.float64, device=lists.dev)
    p = lists.ptr
    good = dict(off=p["off"], N=N, G=G, T=p["T"], I=p["I"], L=p["L"], freq=freq, alpha=alpha, wf=wf, dr=dr, di=di, nf=F, norm=1,
                out=out.data_ptr())

    def call(**kw):
        a = dict(good, **kw)
        host = lambda v: None if v is None else v.ctypes.data   # noqa: E731
        return Lb.pgr_matched_field_device(0, a["off"], a["N"], a["G"], a["T"], a["I"], None, None, a["L"], host(a["freq"]),
                                           host(a["alpha"]), host(a["wf"]), host(a["dr"]), host(a["di"]), a["nf"], a["norm"],
                                           a["out"], ctypes.c_void_p(lists.stream))

    def with_value(a, v, k=F // 2):
        a = a.copy()
        a.reshape(-1)[k] = v
        return a
    cases = [(dict(off=None), "null"), (dict(T=None), "null"), (dict(I=None), "null"), (dict(freq=None), "null"),
             (dict(wf=None), "null"), (dict(dr=None), "null"), (dict(di=None), "null"), (dict(out=None), "null"),
             (dict(alpha=None), "go together"), (dict(L=None), "go together"),
             (dict(N=0), "n_elements"), (dict(N=-1), "n_elements"), (dict(G=0), "n_cells"), (dict(G=-1), "n_cells"),
             (dict(G=2 ** 30), "too many groups"), (dict(N=2 ** 16, G=2 ** 15), "too many groups"),
             (dict(N=1, G=2 ** 31), "too many groups"),
             (dict(nf=0), "n_freq"), (dict(nf=-5), "n_freq"), (dict(nf=65535 * 256 + 1), "n_freq"),
             (dict(freq=with_value(freq, -1.0)), "freq must be"), (dict(freq=with_value(freq, np.nan)), "freq must be"),
             (dict(freq=with_value(freq, np.inf, F - 1)), "freq must be"),
             (dict(alpha=with_value(alpha, -1e-13)), "alpha must be"), (dict(alpha=with_value(alpha, np.nan)), "alpha must be"),
             (dict(wf=with_value(wf, -1e-300)), "wf must be"), (dict(wf=with_value(wf, np.nan, 0)), "wf must be"),
             (dict(wf=with_value(wf, np.inf, F - 1)), "wf must be"), (dict(wf=with_value(wf, -np.inf)), "wf must be"),
             (dict(dr=with_value(dr, np.nan)), "data"), (dict(dr=with_value(dr, np.inf, 0)), "data"),
             (dict(di=with_value(di, -np.inf, N * F - 1)), "data"), (dict(di=with_value(di, np.nan, F)), "data"),
             (dict(norm=2), "normalize"), (dict(norm=-1), "normalize")]
    for kw, msg in cases:
        rc = call(**kw)
        err = Lb.pgr_last_error().decode()
        assert rc < 0 and "pgr_matched_field_device" in err and msg in err, (kw, rc, err)
    torch.cuda.synchronize(lists.dev)
    assert (out.cpu().numpy() == MARK).all()
    assert call() == 0 and call(L=None, alpha=None, norm=0) == 0         # and the same buffer with good arguments: written
    assert not (out.cpu().numpy() == MARK).any()
    with pytest.raises(_lib.PgrError, match="pgr_matched_field_device.*wf must be"):
        _lib.matched_field_sum(0, p["off"], N, G, p["T"], p["I"], 0, 0, 0, freq, None, with_value(wf, -1.0), data, True,
                               good["out"], lists.stream)


# ---- fans -----------------------------------------------------------------------------------------------------------------

ELEMENTS = (900.0, 1000.0, 1150.0)


def _shoot(pr, env, depth, resident):
    return pr.shoot_rays(depth, 0.0, np.linspace(-20.0, 20.0, 2001), 100e3, 101, env, flatearth=False, debug=False,
                         device_resident=resident, max_bounces=64)


@pytest.fixture(scope="module")
def munk_fans(pr):
    """three 2001-ray Munk fans to 100 km from three element depths with a bounce log of 64 slots, device resident and the
    same fans on the host"""
    env = munk_env(pr)
    return [_shoot(pr, env, z, True) for z in ELEMENTS], [_shoot(pr, env, z, False) for z in ELEMENTS], env


def _reduced(Hs, data, wf, normalize):
    """the defined reduction of the elements' transfer functions Hs [N] of (R, n, F) -> (R, n)"""
    H = np.stack(Hs)
    N, R, n, F = H.shape
    return mref.reduce_match(H.real.reshape(N, R * n, F), H.imag.reshape(N, R * n, F), data, wf, normalize).reshape(R, n)


def test_matched_field_is_the_defined_reduction_of_the_elements_transfer_functions(pr, munk_fans):
    fans, eager, env = munk_fans
    assert len(FAN_DEPTHS) == 50 and len(FREQ) == 65
    shaped = np.linspace(1.0, 9.0, len(FREQ)) / 5.0
    data = snapshot(3, len(FREQ), 11)
    for kw, weights in ((dict(), None), (dict(bottom_loss=pr.fluid_halfspace(*SAND)), shaped),
                        (dict(absorption=pr.thorp_absorption, surface_loss=0.5), shaped)):
        opt = dict(range_indices=COLS, flatearth=False, **kw)
        Hs = [pr.transfer_function(fan, FAN_DEPTHS, env, FREQ, **opt) for fan in fans]
        w = np.full(len(FREQ), 1.0 / len(FREQ)) if weights is None else shaped
        for normalize in (True, False):
            B = pr.matched_field(fans, data, FAN_DEPTHS, env, FREQ, weights=weights, normalize=normalize, **opt)
            for fan in fans:
                _in_place(fan)
            assert B.shape == (50, 3) and B.dtype == np.float64
            assert _same(pr.matched_field(eager, data, FAN_DEPTHS, env, FREQ, weights=weights, normalize=normalize, **opt), B)
            assert _same(B, _reduced(Hs, data, mref.normalised_weights(w, data) if normalize else w, normalize))
            # the elements' own column is NaN; elsewhere most cells are lit
            assert np.isnan(B[:, 2]).all() and not np.isnan(B[:, :2]).any() and (B[:, :2] > 0).mean() > 0.5
    # the self-match: the replicas of one cell as data give 1 there, and no more anywhere
    opt = dict(range_indices=COLS, flatearth=False)
    Hs = [pr.transfer_function(fan, FAN_DEPTHS, env, FREQ, **opt) for fan in fans]
    for cell in ((20, 0), (33, 1)):
        own = np.stack([H[cell] for H in Hs])
        assert (np.abs(own) > 0).all()
        B = pr.matched_field(fans, own, FAN_DEPTHS, env, FREQ, weights=shaped / shaped.sum(), **opt)
        print(f"  self-match at {FAN_DEPTHS[cell[0]]:.0f} m, column {COLS[cell[1]]}: B - 1 = {B[cell] - 1.0:.3e}; runner-up "
              f"{np.sort(B[:, :2].ravel())[-2]:.4f}")
        assert abs(B[cell] - 1.0) <= 1e-12 and (B[:, :2] <= 1.0 + 1e-12).all()
        assert np.unravel_index(np.nanargmax(B), B.shape) == cell
    # the weights, the normalisation and the order of the elements matter; a default range_indices is the last column
    plain = pr.matched_field(fans, data, FAN_DEPTHS, env, FREQ, **opt)
    assert not _same(plain, pr.matched_field(fans, data, FAN_DEPTHS, env, FREQ, weights=shaped, **opt))
    assert not _same(plain, pr.matched_field(fans[::-1], data, FAN_DEPTHS, env, FREQ, **opt))
    one = pr.matched_field(fans, data, FAN_DEPTHS, env, FREQ, flatearth=False)
    assert one.shape == (50, 1) and _same(one[:, 0], plain[:, 0])
    for fan in fans:
        _in_place(fan)


def test_an_output_that_does_not_fit_is_refused_before_any_kernel(pr, munk_fans, monkeypatch):
    import torch
    fans, eager, env = munk_fans
    data = snapshot(3, len(FREQ), 1)
    need = 8 * len(FAN_DEPTHS) * len(COLS)
    monkeypatch.setattr(torch.cuda, "mem_get_info", lambda *a: (need - 1, 10 ** 12))
    for name in ("matched_field", "beam_matched_field"):
        with pytest.raises(ValueError, match=f"the ambiguity surface needs {need} bytes of device memory.*{need - 1} are free"):
            getattr(pr, name)(fans, data, FAN_DEPTHS, env, FREQ, range_indices=COLS, flatearth=False)
    # the joined lists, by the arrivals' count
    monkeypatch.setattr(torch.cuda, "mem_get_info", lambda *a: (need + 8 * 451, 10 ** 12))
    with pytest.raises(ValueError, match=r"the \d+ arrivals of the 3 fans need \d+ bytes of device memory"):
        pr.matched_field(fans, data, FAN_DEPTHS, env, FREQ, range_indices=COLS, flatearth=False)
    monkeypatch.undo()
    for fan in fans:
        _in_place(fan)


def test_beam_matched_field_is_the_defined_reduction_of_beam_transfer_function(pr, munk_fans):
    fans, eager, env = munk_fans
    d = FAN_DEPTHS[::5]
    shaped = np.linspace(1.0, 9.0, len(FREQ)) / 5.0
    data = snapshot(3, len(FREQ), 13)
    for kw in (dict(), dict(min_width=25.0, curvature=False, surface_loss=0.5, absorption=pr.thorp_absorption)):
        opt = dict(range_indices=COLS, flatearth=False, **kw)
        Hs = [pr.beam_transfer_function(fan, d, env, FREQ, **opt) for fan in fans]
        for normalize in (True, False):
            B = pr.beam_matched_field(fans, data, d, env, FREQ, weights=shaped, normalize=normalize, **opt)
            for fan in fans:
                _in_place(fan)
            assert _same(pr.beam_matched_field(eager, data, d, env, FREQ, weights=shaped, normalize=normalize, **opt), B)
            wf = mref.normalised_weights(shaped, data) if normalize else shaped
            assert B.shape == (len(d), 3) and _same(B, _reduced(Hs, data, wf, normalize))
            assert np.isnan(B[:, 2]).all() and not np.isnan(B[:, :2]).any() and (B[:, :2] > 0).mean() > 0.5
    with pytest.raises(ValueError, match="does not yet apply a complex bottom phase"):
        pr.beam_matched_field(fans, data, d, env, FREQ, bottom_loss=pr.fluid_halfspace(*SAND), range_indices=COLS, flatearth=False)
    for fan in fans:
        _in_place(fan)


# ---- physics on HIP fans -------------------------------------------------------------------------------------------------------

@pytest.fixture(scope="module")
def lloyd_fans(pr):
    """eight 4001-ray fans over +-40 degrees in the isovelocity half space, one from each element, device resident, saved every
    match_reference.LLOYD_SAVE_SPACING = 20 m: a traced fan's samples next to a surface reflection lie up to half a save spacing
    x tan(theta) above the surface, and the save grid must keep the beams beside that fold above the shallowest cell for the
    fans to be the exact fans the bounds were recorded on (match_reference.fold_reach; tests/test_match_host.py shows what a
    100 m grid does)"""
    env = cref.lloyd_env(pr)
    angles = np.linspace(-bp.EXACT_APERTURE, bp.EXACT_APERTURE, bp.EXACT_N)
    S = int(round(5e3 / mref.LLOYD_SAVE_SPACING)) + 1
    assert S == 251 and mref.fold_reach(mref.LLOYD_SAVE_SPACING) < bp.LLOYD_DEPTHS.min()
    fans = [pr.shoot_rays(z, 0.0, angles, 5e3, S, env, flatearth=False, debug=False, device_resident=True, max_bounces=4)
            for z in mref.ELEMENT_DEPTHS]
    assert len(fans) == 8 and all(len(f) == 4001 and (f.n_botts == 0).all() and f.n_surfs.max() == 1 for f in fans)
    cols = np.array([100, 150, 200, 250])
    assert np.array_equal(np.asarray(fans[0].rs[0])[cols], bp.EXACT_RANGES)
    return fans, env, cols


def test_lloyd_localisation_from_shoot_rays(pr, lloyd_fans):
    fans, env, cols = lloyd_fans
    B = pr.matched_field(fans, mref.lloyd_data(), bp.LLOYD_DEPTHS, env, bref.BAND_FREQ, range_indices=cols, flatearth=False)
    check_lloyd_match(B, mref.MATCH_LLOYD_MEASURED, "matched_field from shoot_rays")
    for fan in fans:
        _in_place(fan)


def test_lloyd_localisation_from_shoot_rays_with_beams(pr, lloyd_fans):
    fans, env, cols = lloyd_fans
    Bb = pr.beam_matched_field(fans, mref.lloyd_data(), bp.LLOYD_DEPTHS, env, bref.BAND_FREQ, min_width=10.0, range_indices=cols,
                               flatearth=False)
    check_lloyd_match(Bb, mref.MATCH_LLOYD_BEAM_MEASURED, "beam_matched_field from shoot_rays, min_width 10 m")
    for fan in fans:
        _in_place(fan)
