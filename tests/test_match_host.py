"""Matched-field processing without a GPU: the NumPy restatement (tests/match_reference.py) against a reduction written apart
from it, its identities (the band power of one element, the self-match), its edge cases, localisation on Lloyd's mirror with exact
straight rays from eight elements against the same processor on closed-form replicas -- on the tube lists and on the beam lists,
with the test's power asserted -- and the API: the exports, the one prototype in a header of its own and every argument refused
before anything reaches the device."""
import ctypes
import inspect
import os

import numpy as np
import pytest

import pygenray_amd as pr

import band_reference as bref
import beam_pressure_reference as bp
import match_reference as mref
import reflection_reference as rref
import spectrum_reference as spref
from test_coherent_host import _host_fan
from test_spectrum_host import synthetic_arrivals

NAMES = ("matched_field", "beam_matched_field")


# ---- the restatement against an independent reduction -------------------------------------------------------------------------

def _independent(H, data, wf, normalize):
    """the definition on transfer functions H (N, G, F), written apart from match_reference: Python floats, the fold over the
    elements per (cell, frequency), the partials of the 64 residues of k, then a halving tree -- what lane 0 of the xor tree
    holds, the add being commutative"""
    H, data = np.asarray(H), np.asarray(data)
    N, G, F = H.shape
    out = []
    for g in range(G):
        part = [0.0] * 64
        for k in range(F):
            cr = ci = nn = 0.0
            for j in range(N):
                re, im = float(H[j, g, k].real), float(H[j, g, k].imag)
                dr, di = float(data[j, k].real), float(data[j, k].imag)
                cr = cr + (re * dr + im * di)
                ci = ci + (re * di - im * dr)
                nn = nn + (re * re + im * im)
            A = cr * cr + ci * ci
            B = A if not normalize else (0.0 if nn == 0.0 else A / nn)
            part[k % 64] = part[k % 64] + float(wf[k]) * B
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


def _data(N, F, seed):
    rng = np.random.default_rng(seed)
    return rng.normal(size=(N, F)) + 1j * rng.normal(size=(N, F))


def _element_lists(N, seed):
    """N elements x 3 cells of 0, 17 and 200 arrivals, element-major"""
    return synthetic_arrivals(seed=seed, counts=(0, 17, 200) * N)


@pytest.mark.parametrize("F", [1, 63, 64, 65, 130, 257])
def test_restatement_is_the_defined_reduction_of_the_spectrum_sums_bit_for_bit(F):
    freq = np.linspace(60.0, 90.0, F) if F > 1 else np.array([75.0])
    wf = _weights(F, F)
    assert F == 1 or ((wf == 0).sum() == 1 and len(set(wf.tolist())) == F)
    for N in (1, 2, 5):
        off, T, I, q = _element_lists(N, seed=29 + F + N)
        E = len(off) - 1
        assert E == 3 * N and (q < 0).any() and (q > 3).any()
        rng = np.random.default_rng(F + N)
        L = rng.uniform(1e4, 1.2e6, len(T))
        alpha = rng.uniform(1e-6, 1e-5, F)
        data = _data(N, F, F * N)
        lags = {"none": None, "zero": np.zeros(len(T)), "general": rng.uniform(-3.0, 3.0, len(T))}
        zero = np.zeros(E)
        seen = {}
        for qname, qq in (("q", q), ("null", None)):
            for lname, phi in lags.items():
                for LL, aa in ((None, None), (L, alpha)):
                    H = (spref.spectrum_sum(off, T, I, qq, LL, zero, freq, aa) if phi is None else
                         rref.spectrum_sum(off, T, I, qq, phi, LL, zero, freq, aa)).reshape(N, 3, F)
                    for normalize in (False, True):
                        out = mref.match_power(off, N, T, I, qq, phi, LL, freq, aa, wf, data, normalize)
                        assert out.shape == (3,) and out.dtype == np.float64
                        assert np.array_equal(out, _independent(H, data, wf, normalize)), (N, qname, lname, aa is not None)
                        assert out[0] == 0.0 and not np.signbit(out[0]) and (out[1:] > 0).all()   # the empty cell: +0.0
                        seen[qname, lname, aa is not None, normalize] = out
        # a zero lag leaves every bit alone; a general lag, q, the absorption and the normalisation matter (one element's
        # normalised power is sum_k wf_k |d_k|^2 whatever its replica: there they cannot)
        for key in (("q", False), ("q", True), ("null", False)):
            for normalize in (False, True):
                none = seen[key[0], "none", key[1], normalize]
                assert np.array_equal(seen[key[0], "zero", key[1], normalize], none)
                assert (N == 1 and normalize) or not np.array_equal(seen[key[0], "general", key[1], normalize], none)
        assert not np.array_equal(seen["q", "none", False, N > 1], seen["null", "none", False, N > 1])
        assert not np.array_equal(seen["q", "none", True, False][1:], seen["q", "none", False, False][1:])
        assert not np.array_equal(seen["q", "none", False, True][1:], seen["q", "none", False, False][1:])
        # the fold without normalisation through band_reference's own tree: cr, ci stand where re, im stand there
        re, im = mref.match_terms(off, N, T, I, q, None, None, freq, None)
        A = mref.fold_elements(re, im, data, False)
        assert np.array_equal(mref.reduce_lanes(A, wf), seen["q", "none", False, False])
        assert np.array_equal(mref.reduce_lanes(re[0] * re[0] + im[0] * im[0], wf), bref.reduce_band(re[0], im[0], wf))


@pytest.mark.parametrize("F", [1, 65, 257])
def test_one_element_with_unit_data_is_the_band_power_bit_for_bit(F):
    off, T, I, q = synthetic_arrivals(seed=3 + F)
    rng = np.random.default_rng(F)
    freq = np.linspace(60.0, 90.0, F) if F > 1 else np.array([75.0])
    wf = _weights(F, 7 * F)
    L, alpha, phi = rng.uniform(1e4, 1.2e6, len(T)), rng.uniform(1e-6, 1e-5, F), rng.uniform(-3.0, 3.0, len(T))
    ones = np.ones((1, F), dtype=complex)
    for qq, pp, LL, aa in ((q, None, None, None), (None, None, None, None), (q, phi, None, None), (q, phi, L, alpha)):
        out = mref.match_power(off, 1, T, I, qq, pp, LL, freq, aa, wf, ones, False)
        assert np.array_equal(out, bref.band_power(off, T, I, qq, pp, LL, freq, aa, wf)) and (out[1:] > 0).all()


def test_the_replicas_of_one_cell_as_data_match_that_cell_fully():
    N, F = 5, 65
    off, T, I, q = _element_lists(N, seed=41)
    freq = np.linspace(60.0, 90.0, F)
    w = _weights(F, 3)
    w = w / w.sum()
    for g0 in (1, 2):
        re, im = mref.match_terms(off, N, T, I, q, None, None, freq, None)
        data = re[:, g0, :] + 1j * im[:, g0, :]
        out = mref.reduce_match(re, im, data, mref.normalised_weights(w, data), True)
        print(f"self-match at cell {g0}: B - 1 = {out[g0] - 1.0:.3e}; the other cells {np.delete(out, g0)}")
        assert abs(out[g0] - 1.0) <= 1e-12 and (out <= 1.0 + 1e-12).all() and out[0] == 0.0
        assert (np.delete(out, g0) < 0.9).all()
        # without the normalisation the matched cell holds sum_k w_k (sum_j |H_jk|^2)^2
        raw = mref.reduce_match(re, im, data, w, False)
        assert raw[g0] == pytest.approx(float((w * ((re[:, g0] ** 2 + im[:, g0] ** 2).sum(axis=0)) ** 2).sum()), rel=1e-12)


def test_empty_cells_are_plus_zero_and_a_nan_stays_in_its_cell():
    F = bref.BAND_FREQ
    w = bref.BAND_UNIFORM
    # 2 elements x 3 cells: cell 0 empty at both, cell 1 lit at both, cell 2 lit at element 0 alone
    off = np.array([0, 0, 2, 3, 3, 5, 5])
    T = np.array([60.0, 60.5, 61.0, 60.2, 60.7])
    I = np.full(5, 1e-8)
    data = _data(2, len(F), 5)
    for normalize in (False, True):
        out = mref.match_power(off, 2, T, I, None, None, None, F, None, w, data, normalize)
        assert out[0] == 0.0 and not np.signbit(out[0]) and (out[1:] > 0).all()
        # arrivals that add nothing: cell 1 of q < 0 alone at both elements
        q = np.array([-1, -1, 0, -1, -1], np.int32)
        out = mref.match_power(off, 2, T, I, q, None, None, F, None, w, data, normalize)
        assert out[1] == 0.0 and not np.signbit(out[1]) and out[0] == 0.0 and out[2] > 0
        # a NaN T, I or lag makes exactly its cell NaN, whichever element's list holds it
        for a in (0, 2, 3):
            cell = {0: 1, 2: 2, 3: 1}[a]
            for name in ("T", "I", "phi"):
                TT, II, pp = T.copy(), I.copy(), np.zeros(5)
                {"T": TT, "I": II, "phi": pp}[name][a] = np.nan
                out = mref.match_power(off, 2, TT, II, None, pp, None, F, None, w, data, normalize)
                assert np.array_equal(np.flatnonzero(np.isnan(out)), [cell]), (a, name, out)
        # a NaN datum reaches every cell, 0.0 * NaN being NaN -- but for the cells no element reaches under the normalisation,
        # whose nn == 0.0 the definition asks first
        bad = data.copy()
        bad[1, 9] = np.nan
        out = mref.match_power(off, 2, T, I, None, None, None, F, None, w, bad, normalize)
        assert np.isnan(out[1:]).all() and (out[0] == 0.0 if normalize else np.isnan(out[0]))


# ---- localisation on Lloyd's mirror -------------------------------------------------------------------------------------------

def check_lloyd_match(B, measured, what, cell=mref.TRUE_CELL, w=bref.BAND_UNIFORM):
    """the peak of an ambiguity surface B (18, 4) in the true cell and every cell within twice the measured constant of the
    Bartlett processor on closed-form replicas -> the worst |B - B_closed|"""
    Bc = mref.bartlett_closed(mref.lloyd_data(cell), w)
    e = np.abs(B - Bc)
    j, c = np.unravel_index(np.argmax(e), e.shape)
    peak = np.unravel_index(np.argmax(B), B.shape)
    runner = np.sort(B.ravel())[-2]
    print(f"Lloyd localisation, {what}: peak at {bp.LLOYD_DEPTHS[peak[0]]} m, {bp.EXACT_RANGES[peak[1]]} m; 1 - B(true) "
          f"{1.0 - B[cell]:.3e}; runner-up {runner:.4f}; worst |B - B_closed| {e.max():.16e} at {bp.LLOYD_DEPTHS[j]} m, "
          f"{bp.EXACT_RANGES[c]} m; bound {2.0 * measured:.6e}")
    assert B.shape == (18, 4) and tuple(int(v) for v in peak) == tuple(cell)
    assert e.max() <= 2.0 * measured                                              # every cell: none left out
    return float(e.max())


def _restated(lists, data, w, **kw):
    off, T, I, q = lists
    q = kw.get("q", q)
    return mref.as_cells(mref.match_power(off, len(mref.ELEMENT_DEPTHS), T, I, q, None, None, bref.BAND_FREQ, None,
                                          mref.normalised_weights(w, data), data, True))


def test_the_cells_lie_inside_the_aperture_of_every_elements_fan():
    """section 20's premise for every element: the direct path covers depths up to z_j + r tan 40, the reflected one up to
    r tan 40 - z_j, and the cells lie four sigma of the widest beam inside the narrower of the two at every range"""
    edge = np.tan(np.radians(bp.EXACT_APERTURE)) * bp.EXACT_RANGES
    for zj in mref.ELEMENT_DEPTHS[[0, -1]]:
        reach = 4.0 * bp.widest_beam(zj, 10.0)
        assert (bp.LLOYD_DEPTHS.max() + reach <= edge - zj).all()
    assert len(mref.ELEMENT_DEPTHS) == 8 and mref.ELEMENT_DEPTHS[0] == 300.0 and mref.ELEMENT_DEPTHS[-1] == 650.0
    assert bp.LLOYD_DEPTHS[mref.TRUE_CELL[0]] == 425.0 and bp.EXACT_RANGES[mref.TRUE_CELL[1]] == 3e3


@pytest.mark.parametrize("which", ["tubes", "beams"])
def test_lloyd_localisation_from_the_restatement(which):
    lists = mref.element_tube_lists() if which == "tubes" else mref.element_beam_lists(10.0, True)
    measured = mref.MATCH_LLOYD_MEASURED if which == "tubes" else mref.MATCH_LLOYD_BEAM_MEASURED
    assert set(lists[3].tolist()) == {0, 2} and len(lists[0]) == 8 * 72 + 1
    uniform = bref.BAND_UNIFORM
    data = mref.lloyd_data()
    assert data.shape == (8, 64)
    B = _restated(lists, data, uniform)
    worst = check_lloyd_match(B, measured, f"restatement on the exact straight rays' {which}")
    assert worst == pytest.approx(measured, rel=1e-6) and 2.0 * measured < 1e-4     # the constant is this set-up's value
    assert 1.0 - B[mref.TRUE_CELL] < 1e-8 and np.sort(B.ravel())[-2] < 0.5
    bound = 2.0 * measured
    closed = mref.bartlett_closed(data, uniform)
    # the other two true cells tried peak where they should
    for cell in mref.OTHER_TRUE_CELLS:
        Bo = _restated(lists, mref.lloyd_data(cell), uniform)
        assert np.unravel_index(np.argmax(Bo), Bo.shape) == cell and 1.0 - Bo[cell] < 1e-8
    # the test's power: each of these misses the bound by more than 100 x
    flipped = _restated(lists, np.conj(data), uniform)          # |sum_j H d|: H d instead of conj(H) d
    print(f"  H d instead of conj(H) d: B(true) {flipped[mref.TRUE_CELL]:.3f}")
    assert np.abs(flipped - closed).max() > 100 * bound and flipped[mref.TRUE_CELL] < 0.5
    no_phase = _restated(lists, data, uniform, q=np.where(lists[3] == 2, 0, lists[3]))
    assert np.abs(no_phase - closed).max() > 100 * bound
    shaped = bref.spectrum_shaped_weights()
    Bw = _restated(lists, data, shaped)
    e_shaped = np.abs(Bw - mref.bartlett_closed(data, shaped)).max()
    print(f"  with the source spectrum's weights: worst |B - B_closed| {e_shaped:.6e}")
    assert e_shaped <= bound                                                      # the weights used as given ...
    assert np.abs(B - mref.bartlett_closed(data, shaped)).max() > 100 * bound     # ... and ignored


def test_a_traced_fans_save_grid_must_keep_the_surface_fold_above_the_cells():
    """a traced fan's samples next to a surface reflection (match_reference.resampled_fan) widen the beams beside the fold: at
    the 20 m save spacing of the GPU test's fans they end above the shallowest cell and the surface is the exact fan's bit for
    bit; at 100 m they reach the cells at 75 m and 125 m, and the beam surface misses its bound at 75 m / 2 km -- by the
    figure eight shoot_rays fans with 51 save ranges gave on the GPU, 8.118e-05"""
    shallowest = bp.LLOYD_DEPTHS.min()
    assert mref.LLOYD_SAVE_SPACING == 20.0 and mref.fold_reach(20.0) == 43.25 and mref.fold_reach(100.0) == 146.25
    assert mref.fold_reach(mref.LLOYD_SAVE_SPACING) < shallowest < bp.LLOYD_DEPTHS[1] < mref.fold_reach(100.0)
    assert all(np.array_equal(a, b) for a, b in zip(mref.resampled_fan(650.0, 0.0), bp.exact_fan(650.0)))
    data, w = mref.lloyd_data(), bref.BAND_UNIFORM
    exact = _restated(mref.element_beam_lists(10.0, True), data, w)
    fine = mref.element_beam_lists(10.0, True, save_spacing=mref.LLOYD_SAVE_SPACING)
    assert np.array_equal(_restated(fine, data, w), exact)
    coarse = _restated(mref.element_beam_lists(10.0, True, save_spacing=100.0), data, w)
    e = np.abs(coarse - mref.bartlett_closed(data, w))
    bound = 2.0 * mref.MATCH_LLOYD_BEAM_MEASURED
    print(f"beam lists of fans re-sampled at 100 m: |B - B_closed| {e[0, 0]:.6e} at 75 m / 2 km, {np.delete(e.ravel(), 0).max():.6e} "
          f"elsewhere; bound {bound:.6e}")
    assert e[0, 0] == pytest.approx(8.118e-05, rel=1e-3) and e[0, 0] > 20 * bound and np.delete(e.ravel(), 0).max() <= bound
    assert np.unravel_index(np.argmax(coarse), coarse.shape) == mref.TRUE_CELL


# ---- the API, no GPU ----------------------------------------------------------------------------------------------------------

def test_the_new_names_are_exported_and_the_entry_is_bound_from_its_own_header():
    from pygenray_amd import _lib
    for name in NAMES:
        assert name in pr.__all__ and callable(getattr(pr, name))
    sig = inspect.signature(pr.matched_field).parameters
    assert list(sig) == ["fans", "data", "candidate_depths", "env", "frequencies", "weights", "range_indices", "normalize",
                         "absorption", "bottom_loss", "surface_loss", "flatearth", "device"]
    beam = inspect.signature(pr.beam_matched_field).parameters
    assert list(beam) == list(sig)[:6] + ["min_width", "curvature"] + list(sig)[6:]
    assert beam["min_width"].default == 10.0 and beam["curvature"].default is True
    for s in (sig, beam):
        assert all(s[k].default is None for k in ("weights", "range_indices", "absorption", "bottom_loss", "surface_loss"))
        assert s["normalize"].default is True and s["flatearth"].default is True and s["device"].default == 0
    own = _lib.HEADER_PROTOTYPES["pgr_match.h"]
    V, I32, I64, I = ctypes.c_void_p, ctypes.c_int32, ctypes.c_int64, ctypes.c_int
    assert own == {"pgr_matched_field_device": (I, [I, V, I32, I64, V, V, V, V, V, V, V, V, V, V, I32, I, V, V])}
    assert all("pgr_matched_field_device" not in protos for h, protos in _lib.HEADER_PROTOTYPES.items() if h != "pgr_match.h")
    assert _lib.PROTOTYPES["pgr_matched_field_device"] == own["pgr_matched_field_device"]
    # the wrapper: its name does not end in _device (the table of tests/test_binding_signatures_host.py is about those)
    assert callable(_lib.matched_field_sum) and not hasattr(_lib, "matched_field_device")
    assert str(inspect.signature(_lib.matched_field_sum)) == (
        "(device, offsets_ptr, n_elements, n_cells, t_ptr, i_ptr, q_ptr, phi_ptr, l_ptr, freq, alpha, weights, data, normalize, "
        "out_ptr, stream=0)")
    # pgr.h hands the entry to a C caller through the header of its own, between pgr_array.h and pgr_band.h
    text = open(_lib.HEADER).read()
    inc = '#include "pgr_match.h"'
    assert text.count(inc) == 1 and text.index('#include "pgr_array.h"') < text.index(inc) < text.index('#include "pgr_band.h"')
    names = [os.path.basename(h) for h in _lib.HEADERS]
    assert names.count("pgr_match.h") == 1 and names[-3:] == ["pgr_array.h", "pgr_match.h", "pgr_band.h"]
    assert _lib.HEADERS[names.index("pgr_match.h")] in _lib.build_dependencies()
    # the kernel's header stands behind pgr_band.h and before the final pgr_spectrum.h, which it includes itself
    hip = open(_lib.CSRC + "/pgr_hip.hip").read()
    assert hip.count(inc) == 1
    assert hip.index('#include "pgr_band.h"') < hip.index(inc) < hip.index('#include "pgr_spectrum.h"')
    assert hip.rstrip().splitlines()[-1].startswith('#include "pgr_spectrum.h"')
    kernel = open(os.path.join(_lib.CSRC, "pgr_match.h")).read()
    assert kernel.index('#include "pgr_spectrum.h"') < kernel.index("struct MatchArgs") < kernel.index("pgr_mfp_sum(MatchArgs")
    assert "__shared__" not in kernel and "atomic" not in kernel.split("#ifndef")[1] and "__syncthreads" not in kernel
    assert os.path.join(_lib.CSRC, "pgr_match.h") in _lib.build_dependencies()


def _both(fans=None, data=None, depths=(100.0, 200.0), freq=(50.0, 60.0, 70.0), **kw):
    env = pr.OceanEnvironment2D(flat_earth_transform=False)
    fans = [_host_fan(), _host_fan()] if fans is None else fans
    if data is None:
        try:
            data = np.ones((len(fans), len(freq)), dtype=complex)
        except TypeError:
            data = np.ones((2, 3), dtype=complex)
    kw = dict(dict(flatearth=False), **kw)
    beam_kw = {k: kw.pop(k) for k in ("min_width", "curvature") if k in kw}
    return [lambda: pr.matched_field(fans, data, list(depths), env, freq, **kw),
            lambda: pr.beam_matched_field(fans, data, list(depths), env, freq, **kw, **beam_kw)]


def _refused(match, exc=ValueError, **kw):
    for call in _both(**kw):
        with pytest.raises(exc, match=match):
            call()


def test_bad_arguments_are_refused_before_the_device():
    # the array's side
    for fans in ([], (), _host_fan(), [_host_fan(), "fan"], "fans", 3):
        _refused("fans must be a non-empty sequence of RayFans", fans=fans, data=np.ones((2, 3), dtype=complex))
    _refused("the fans must share one save grid", fans=[_host_fan(), _host_fan(S=6)])
    _refused("the fans must share one save grid", fans=[_host_fan(), _host_fan(), _host_fan(S=4)])
    for shape in ((3,), (3, 2), (1, 3), (2, 4), (2, 3, 1)):
        _refused(r"data must be complex of the shape \(elements, frequencies\) = \(2, 3\)", data=np.ones(shape, dtype=complex))
    _refused("data must be complex of the shape", data=np.full((2, 3), "a"))
    for bad in (np.nan, np.inf, -np.inf, 1j * np.nan, -1j * np.inf):
        d = np.ones((2, 3), dtype=complex)
        d[1, 2] = bad
        _refused("data must be finite", data=d)
    d = np.ones((2, 3), dtype=complex)
    d[:, 1] = 0.0
    _refused("data vanishes at a frequency with a positive weight", data=d)
    _refused("data vanishes at a frequency with a positive weight", data=d, weights=[0.0, 1.0, 0.0])
    _refused("weights / sum_j .* overflows", data=np.full((2, 3), 1e-160 + 0j))
    # ... which the unnormalised processor and a zero weight take (and go on to the fan's own refusal)
    _refused("at least 2 rays", data=d, normalize=False, fans=[_host_fan()[:1]] * 2)
    _refused("at least 2 rays", data=d, weights=[1.0, 0.0, 1.0], fans=[_host_fan()[:1]] * 2)
    # band_intensity's frequencies and weights
    for freq in (75.0, [[50.0, 60.0]], np.zeros((2, 2)), []):
        _refused("frequencies must be a non-empty 1-D sequence", freq=freq)
    for bad in (np.nan, np.inf, -np.inf, -1.0):
        _refused("frequencies must be finite and >= 0", freq=[50.0, bad, 70.0])
    for w in (1.0, [1.0], [1.0, 1.0], [[1.0, 1.0, 1.0]], np.ones(4)):
        _refused(r"weights must hold one weight per frequency \(3\)", weights=w)
    for bad in (np.nan, np.inf, -np.inf, -1e-300):
        _refused("weights must be finite and >= 0", weights=[1.0, bad, 1.0])
    _refused("weights must not all be zero", weights=[0.0, 0.0, 0.0])
    for bad in (lambda f: 0.01, lambda f: np.zeros(len(f) + 1)):
        _refused("one value in dB/km per frequency", absorption=bad)
    _refused("frequency_hz must be finite and > 0", freq=[0.0, 50.0, 60.0], absorption=pr.thorp_absorption)
    # transfer_function's own, fan by fan
    _refused("range_indices must lie", range_indices=[5])
    _refused("strictly ascending", depths=(200.0, 100.0))
    _refused("non-empty", depths=())
    _refused("at least 2 rays", fans=[_host_fan(), _host_fan()[:1]])
    _refused("Flat earth transformation has not been applied", flatearth=True)
    _refused("absorption must be finite and >= 0", absorption=-1.0)
    _refused("bounce log", surface_loss=1.0)
    _refused("no bounce log.*max_bounces", fans=[_host_fan(), _host_fan(n_surfs=[0, 1, 0, 0])])
    for w in (0.0, -1.0, np.nan):
        with pytest.raises(ValueError, match="min_width must be finite and > 0"):
            _both(min_width=w)[1]()
    # a BottomReflection: the tube product takes it (and goes on to miss the bounce log), the beam product refuses it
    calls = _both(bottom_loss=pr.fluid_halfspace(1700.0, 1800.0, 0.5))
    with pytest.raises(ValueError, match="bounce log"):
        calls[0]()
    with pytest.raises(ValueError, match="does not yet apply a complex bottom phase"):
        calls[1]()


def test_the_wrapper_refuses_sequences_of_unequal_shape_before_the_library():
    from pygenray_amd import _lib
    ones = np.ones((2, 2), dtype=complex)
    with pytest.raises(ValueError, match="equal length"):
        _lib.matched_field_sum(0, 0, 2, 1, 0, 0, 0, 0, 0, [50.0, 60.0], None, [1.0], ones, True, 0)
    with pytest.raises(ValueError, match="equal length"):
        _lib.matched_field_sum(0, 0, 2, 1, 0, 0, 0, 0, 0, [50.0, 60.0], [1e-6], [1.0, 1.0], ones, True, 0)
    for data in (ones[:1], ones[:, :1], np.ones(2, dtype=complex)):
        with pytest.raises(ValueError, match="one complex value per element and frequency"):
            _lib.matched_field_sum(0, 0, 2, 1, 0, 0, 0, 0, 0, [50.0, 60.0], None, [1.0, 1.0], data, True, 0)
