"""PGR_ARITH=contracted -- the supported opt-in arithmetic (pygenray_amd/_lib.py): libpgr_hip_fma.so, the same sources
with FMA contraction allowed.  One library per process, chosen at import, so this module has two halves:

* ``test_contracted_mode_in_its_own_process`` (runs in the DEFAULT mode): starts a child interpreter with
  PGR_ARITH=contracted that runs the second half of this module, the drop-in API tests (tests/test_dropin_api.py) and the
  tolerance tests of the three ray-tube modules there.
* the ``contracted_*`` tests (run only in a PGR_ARITH=contracted process): the loaded library is the contracted one, and
  its fans meet rule (B) of tests/helpers.py -- within 1e-8 x scale or 10 x the self-noise of the REFERENCE's own vectors,
  class medians within 1e-8 -- on g2 ... g13; the arrival-time histogram equals np.histogram on every edge
  (tests/hist_cases.py); the ray-tube products are exact within the library (arrival slots, order, sum to TL) and within a
  derived bound of the NumPy restatements.  NO bit-parity claim is made or tested for this mode: the reference
  arithmetic (the default) is the only one the parity statements of DESIGN.md are about.

Why the mode exists: pygenray jits its physics with ``fastmath=True`` (REF/integration_processes.py:26,101,177) and SciPy's
stage sums run through BLAS dot products, so FMA contraction is inside the envelope of the reference's own arithmetic.
"""
import os
import subprocess
import sys

import numpy as np
import pytest

import hist_cases
from helpers import load, env_from, tiled_env, munk_arrays
from tube_gpu import pr_any, syn_env  # noqa: F401  (fixtures)

pytestmark = pytest.mark.gpu
# rule (B)'s self-noise for this mode: the oracle under +-1, 2, 3-ulp perturbations of p0 (+ rtol +-1 ulp) -- the sampling the
# reference's own self-noise was recorded with in the golden vectors (seven end states per ray).  Contracted arithmetic is one
# more draw from that noise: against a spread estimated from +-1 ulp alone (four runs) 2 of g11's 288 rays exceeded 10 x.
NOISE_ULPS = (1, 2, 3)
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def _arith():
    from pygenray_amd import _lib
    return _lib.ARITH


def test_contracted_mode_in_its_own_process():
    from pygenray_amd import _lib
    if _lib.ARITH != "reference":
        pytest.skip("this IS the contracted process")
    if not os.path.exists(_lib.CONTRACTED_LIB):
        pytest.fail("libpgr_hip_fma.so is not built (__graft_entry__.build() builds it beside the product)")
    env = dict(os.environ, PGR_ARITH="contracted", PGR_EIGEN_STRICT="0")
    out = subprocess.run([sys.executable, "-m", "pytest", "-q", "-m", "gpu", "-x", "-p", "no:cacheprovider",
                          os.path.join(ROOT, "tests", "test_contracted_arith.py"), os.path.join(ROOT, "tests", "test_dropin_api.py"),
                          *(os.path.join(ROOT, "tests", f) for f in ("test_transmission_loss.py", "test_arrivals.py",
                                                                    "test_beam_tl.py"))],
                         cwd=ROOT, env=env, capture_output=True, text=True, timeout=1500)
    tail = out.stdout[-3000:] + out.stderr[-1500:]
    assert out.returncode == 0, tail
    assert " passed" in out.stdout and "CONTRACTED_LIBRARY_LOADED" in out.stdout, tail
    print(out.stdout[-600:])


@pytest.fixture(scope="module")
def clib():
    from pygenray_amd import _lib
    if _lib.ARITH != "contracted":
        pytest.skip("needs PGR_ARITH=contracted at import (test_contracted_mode_in_its_own_process starts that process)")
    _lib.load()
    return _lib


def test_contracted_library_is_the_one_loaded(clib, capsys):
    import pygenray_amd as pr
    assert pr.ARITHMETIC == "contracted" and clib.LIB_PATH == clib.CONTRACTED_LIB
    info = clib.build_info()
    assert "contract" in info.lower() or "fma" in info.lower(), info
    # the product library stays untouched beside it, and the two hold different device code
    assert clib.device_code_sha256(clib.CONTRACTED_LIB) != clib.device_code_sha256(clib.REFERENCE_LIB)
    with capsys.disabled():
        print("\nCONTRACTED_LIBRARY_LOADED:", info)


def test_contracted_meets_rule_b_on_the_reference_vectors(clib):
    """Rule (B) only (bit_parity=False, noise_ulps=NOISE_ULPS): the contracted fan against the vectors the reference itself produced."""
    from test_hip_parity import golden_check
    g = load("g2_munk_100km.npz")
    golden_check(clib, g, tiled_env(g), 0.0, 100e3, 101, label="g2 [contracted]", bit_parity=False, noise_ulps=NOISE_ULPS)
    g = load("g3_munk_1000km.npz")
    golden_check(clib, g, tiled_env(g), 0.0, 1000e3, 101, label="g3 [contracted]", bit_parity=False, noise_ulps=NOISE_ULPS)
    g = load("g9_irregular_grids.npz")
    golden_check(clib, g, env_from(g), 1e3, 69e3, 61, prefix="t9_", rtol=1e-9, label="g9 [contracted]", strict_bouncing=False,
                 bit_parity=False, noise_ulps=NOISE_ULPS)
    g = load("g4_range_dependent.npz")
    floor = dict(T=1e-6, z=1e-2, p=1e-7)
    golden_check(clib, g, env_from(g), 10e3, 90e3, 81, prefix="fwd_", label="g4 fwd [contracted]", abs_floor=floor,
                 strict_bouncing=False, bit_parity=False, noise_ulps=NOISE_ULPS)
    g = load("g5_const_c.npz")
    golden_check(clib, g, env_from(g), 0.0, 30e3, 60, label="const c [contracted]", bit_parity=False, noise_ulps=NOISE_ULPS)
    g = load("g5_flatearth.npz")
    golden_check(clib, g, env_from(g), 0.0, 100e3, 101, label="flat earth [contracted]", strict_bouncing=False, bit_parity=False, noise_ulps=NOISE_ULPS)


def test_contracted_meets_rule_b_at_the_headline_range(clib):
    from test_hip_parity import golden_check
    from test_oracle_golden import end_state_check
    g = load("g11_munk_1000km_288.npz")
    out = golden_check(clib, g, tiled_env(g), 0.0, 1000e3, 101, label="g11 [contracted]", bit_parity=False, noise_ulps=NOISE_ULPS)
    print("g11 end states [contracted]:", end_state_check(g, out, "g11"))
    g = load("g12_config2_128.npz")
    arrs = munk_arrays(float(g["r_max"]), nr=int(g["nr"]), sofar_slope=float(g["sofar_slope"]))
    out = golden_check(clib, g, arrs, 0.0, 1000e3, 101, label="g12 [contracted]", bit_parity=False, noise_ulps=NOISE_ULPS)
    print("g12 end states [contracted]:", end_state_check(g, out, "g12"))
    for tag, x1 in (("100km", 100e3), ("1000km", 1000e3)):
        g = load(f"g13_default_env_{tag}.npz")
        out = golden_check(clib, g, tiled_env(g), 0.0, x1, 101, label="g13 " + tag + " [contracted]", bit_parity=False, noise_ulps=NOISE_ULPS)
        print(f"g13 {tag} end states [contracted]:", end_state_check(g, out, "g13 " + tag))


def test_contracted_reference_fixture_through_dropin_api(clib):
    """The reference's committed regression fixture (its own tolerances) through the drop-in API in contracted mode."""
    import pygenray_amd as pr
    z = np.linspace(0.0, 6000.0, 400)
    r = np.linspace(0.0, 50e3, 30)
    ssp = pr.DataArray(np.outer(np.ones(30), pr.munk_ssp(z)), dims=["range", "depth"], coords={"range": r, "depth": z})
    bathy = pr.DataArray(np.full(30, 5000.0), dims=["range"], coords={"range": r})
    env = pr.OceanEnvironment2D(sound_speed=ssp, bathymetry=bathy, flat_earth_transform=False)
    rf = pr.shoot_rays(1300.0, 0.0, [-8.0, -4.0, 0.0, 4.0, 8.0], 50e3, 50, env, n_processes=1, debug=False, flatearth=False)
    ref = load("ref_munk_regression.npz")
    np.testing.assert_allclose(rf.ts, ref["ts"], atol=5e-6)
    np.testing.assert_allclose(rf.zs, ref["zs"], atol=0.1)
    np.testing.assert_allclose(rf.ps, ref["ps"], atol=0.1)
    np.testing.assert_array_equal(rf.n_botts, ref["n_botts"])
    np.testing.assert_array_equal(rf.n_surfs, ref["n_surfs"])


# ---- the arrival-time histogram: np.histogram's edges, count for count ---------------------------------------------------

@pytest.mark.parametrize("name, t_min, t_max, bins, min_mismatches", hist_cases.RANGES, ids=[r[0] for r in hist_cases.RANGES])
def test_contracted_histogram_on_every_edge(clib, name, t_min, t_max, bins, min_mismatches):
    """The edges must be np.linspace's, RN(RN(j * step) + first), in this library too: grid_at keeps its multiply and add
    apart (`#pragma clang fp contract(off)`, honoured by -ffp-contract=fast-honor-pragmas)."""
    hist_cases.check_device_histogram(t_min, t_max, bins, min_mismatches)


# ---- the ray-tube products on the synthetic inputs of tests/tube_gpu.py --------------------------------------------------
#
# Exact within this library: every arrival slot written, tubes in increasing order holding their receiver, the arrivals
# summing to this library's TL bit for bit, repeated calls bit-equal.  Bounded against the NumPy restatements, which are
# the reference library's bits.  With u = 2^-53, per ray: the look-up c = sum of four products t_i is within 4 u sum |t_i|
# of the same exact combination of the (identical) weights in either build, so the two differ relatively by
# dc <= 8 u kappa_c, kappa_c = sum |t_i| / c.  Through pc = RN(p c), 1 - pc^2 (fused or not), sqrt and the divide,
# g = c / sqrt(1 - (p c)^2) then differs relatively by at most (dc + 5 u) (2 + pc^2 / (1 - pc^2)) <= (dc + 5 u) kappa_g,
# kappa_g = 1 + 1 / (1 - (p c)^2); we take b_g = (8 kappa_c + 8) u kappa_g.  A tube's I = 0.5 (g_k + g_k+1) |dq0| / (r |dd|)
# adds one rounding per operation in each build: b_I = max(b_g) + 8 u.  w = (D - d_k) / (d_k+1 - d_k) is the same bits;
# T = T_k + w (T_k+1 - T_k) (and p) may be fused: |dT| <= 4 u (|T| + |w dT_k|).  A cell's sum of n terms, added in the same
# order: |dS| <= sum I_k b_I,k + 2 (n - 1) u sum I_k.  Rays with |1 - |p c|| <= 8 eps may change validity under contraction:
# the tubes touching them ("flipped") may differ in structure, and the receivers they cover are left out of the value check.

U = 2.0 ** -53
EPS = 2.0 ** -52

TUBE_CASES = ([(M, 5, 129, False) for M in (63, 64, 65, 4033, 4034, 8300)]
              + [(500, 5, R, False) for R in (1, 64, 65, 4200)]
              + [(4100, 6, 300, True)])
BEAM_CASES = ([(M, 5, 129, 40.0) for M in (61, 62, 63, 3905, 3906, 8300)]
              + [(500, 5, R, 0.5) for R in (1, 64, 65, 4200)])


def _bilinear_abs(x, y, xg, yg, v):
    """sum |t_i| of tl_reference.bilinear's four products"""
    i = np.clip(np.searchsorted(xg, x) - 1, 0, len(xg) - 2)
    j = np.clip(np.searchsorted(yg, y) - 1, 0, len(yg) - 2)
    wx = (x - xg[i]) / (xg[i + 1] - xg[i])
    wy = (y - yg[j]) / (yg[j + 1] - yg[j])
    a = np.abs
    return (a(1 - wx) * a(1 - wy) * a(v[i, j]) + a(wx) * a(1 - wy) * a(v[i + 1, j])
            + a(1 - wx) * a(wy) * a(v[i, j + 1]) + a(wx) * a(wy) * a(v[i + 1, j + 1]))


def _ray_bounds(z, p, x, cin):
    """per ray (M, S): b_g (inf where the ray is invalid) and `near`, the rays whose validity may flip"""
    import tl_reference as tlr
    from tube_gpu import SYN_R, SYN_Z
    d, ps = -z.T, p.T
    X = np.broadcast_to(x, d.shape)
    with np.errstate(invalid="ignore", divide="ignore"):
        c = tlr.bilinear(X, d, SYN_R, SYN_Z, cin)
        kc = _bilinear_abs(X, d, SYN_R, SYN_Z, cin) / np.abs(c)
        pc = ps * c
        kg = np.where(np.abs(pc) < 1, 1 + 1 / (1 - pc * pc), np.inf)
        near = np.abs(1 - np.abs(pc)) <= 8 * EPS
    return (8 * kc + 8) * U * kg, near


def _flipped_cells(z, x, flip, depths, zone):
    """(R, S) cells within reach of a flipped tube: zone(d0, d1, s) -> list of (centre, half-width)"""
    d = -z.T
    out = np.zeros((len(depths), len(x)), bool)
    for k, s in zip(*np.nonzero(flip)):
        for ctr, h in zone(d[k, s], d[k + 1, s], s):
            if np.isfinite(ctr) and np.isfinite(h):
                out[:, s] |= np.abs(depths - ctr) <= h
    return out


@pytest.mark.parametrize("M, S, R, shuffle", TUBE_CASES, ids=[f"M{M}-S{S}-R{R}{'-shuffled' if sh else ''}"
                                                               for M, S, R, sh in TUBE_CASES])
def test_contracted_tl_and_arrivals_on_synthetic_inputs(clib, syn_env, M, S, R, shuffle):
    import arrivals_reference as ar
    import tl_reference as tlr
    from test_arrivals import _synthetic_t
    from tube_gpu import SYN_R, SYN_Z, _device_arrivals, _device_intensity, synthetic_fan
    env, cin = syn_env
    seed = M * 1009 + S * 31 + R
    z, p, x, p0, depths = synthetic_fan(M, S, R, seed=seed, cin=cin, shuffle=shuffle)
    t = _synthetic_t(M, S, seed)
    cols = np.arange(S, dtype=np.int32)
    I = _device_intensity(env, z, p, x, p0, depths)
    a = _device_arrivals(env, t, z, p, x, p0, depths, cols)
    # -- exact, within this library
    assert ar.same(I, _device_intensity(env, z, p, x, p0, depths))
    again = _device_arrivals(env, t, z, p, x, p0, depths, cols)
    assert all(ar.same(a[k], again[k]) for k in a)
    for sub in ([S - 1, 0, S - 1, S // 2],):                       # a column list with repeats, out of order
        b = _device_arrivals(env, t, z, p, x, p0, depths, np.asarray(sub, np.int32))
        nb = np.diff(b["offsets"]).reshape(R, len(sub))
        na = np.diff(a["offsets"]).reshape(R, S)
        assert np.array_equal(nb, na[:, sub])
    n = len(a["tube"])
    assert (a["tube"] != -1).all() and all((a[k] != -1.0).all() for k in ("w", "T", "p", "I")), "arrival slots left unwritten"
    grp = np.repeat(np.arange(R * S), np.diff(a["offsets"]))
    assert len(grp) == n
    same_grp = grp[1:] == grp[:-1]
    assert (np.diff(a["tube"].astype(np.int64))[same_grp] > 0).all()
    j, s, k = grp // S, cols[grp % S], a["tube"].astype(np.int64)
    d = -z
    lo, hi = np.fmin(d[s, k], d[s, k + 1]), np.fmax(d[s, k], d[s, k + 1])
    assert ((lo <= depths[j]) & (depths[j] < hi)).all()
    sums = ar.sequential_sums(a["offsets"], a["I"]).reshape(R, S)
    live = x != x[0]
    assert ar.same(sums[:, live], I[:, live]) and np.isnan(I[:, ~live]).all()
    assert (np.diff(a["offsets"]).reshape(R, S)[:, ~live] == 0).all()
    if M >= 8:
        assert n > 0
    # -- bounded, against the restatement
    ref = ar.tube_arrivals(z.T, p.T, t.T, x, p0, depths, cols, cin, SYN_R, SYN_Z)
    I_ref = tlr.tube_intensity(z.T, p.T, x, p0, depths, cin, SYN_R, SYN_Z)
    b_g, near = _ray_bounds(z, p, x, cin)
    flip = near[:-1] | near[1:]
    assert flip.sum() <= 16, flip.sum()                            # a few: the rays the synthetic fan puts at |p c| = 1
    b_I = np.fmax(b_g[:-1], b_g[1:]) + 8 * U                       # (M - 1, S)
    bad = _flipped_cells(z, x, flip, depths, lambda d0, d1, s: [(0.5 * (d0 + d1), 0.5 * abs(d1 - d0))])
    assert ar.same(np.isnan(I), np.isnan(I_ref))
    ok = ~bad & live[None, :]
    assert np.array_equal(I[ok] == 0, I_ref[ok] == 0)
    # the same (receiver, column, tube) keys, but for flipped tubes
    key = lambda g, kk: g * M + kk
    grp_ref = np.repeat(np.arange(R * S), np.diff(ref["offsets"]))
    kd, kr = key(grp, k), key(grp_ref, ref["tube"].astype(np.int64))
    only = np.setxor1d(kd, kr)
    assert flip[only % M, cols[(only // M) % S]].all(), "arrivals differ beyond the flipped tubes"
    mine, theirs = np.isin(kd, kr), np.isin(kr, kd)
    assert np.array_equal(kd[mine], kr[theirs])
    kk, ss = k[mine], s[mine]
    assert ar.same(a["w"][mine], ref["w"][theirs])                 # w: the same operations, none fusable
    tk, dt = t.T[kk, ss], t.T[kk + 1, ss] - t.T[kk, ss]
    pk, dp = p.T[kk, ss], p.T[kk + 1, ss] - p.T[kk, ss]
    w = ref["w"][theirs]
    for name, v0, dv in (("T", tk, dt), ("p", pk, dp)):
        got, want = a[name][mine], ref[name][theirs]
        assert ar.same(np.isnan(got), np.isnan(want)), name          # (the synthetic fan has NaN travel times)
        f = ~np.isnan(want)
        assert (np.abs(got - want)[f] <= 4 * U * (np.abs(v0) + np.abs(w * dv) + np.abs(want))[f]).all(), name
    dI = np.abs(a["I"][mine] - ref["I"][theirs])
    assert (dI <= ref["I"][theirs] * b_I[kk, ss]).all(), (dI / ref["I"][theirs] / b_I[kk, ss]).max()
    # the cells: sum I_k b_I,k + 2 (n - 1) u sum I_k over the restatement's arrivals of each cell
    kr_k, kr_s = ref["tube"].astype(np.int64), cols[grp_ref % S]
    e1 = np.bincount(grp_ref, ref["I"] * b_I[kr_k, kr_s], minlength=R * S).reshape(R, S)
    cnt = np.diff(ref["offsets"]).reshape(R, S)
    bound = e1 + 2 * np.maximum(cnt - 1, 0) * U * np.where(np.isnan(I_ref), 0, I_ref)
    err = np.abs(I - I_ref)
    assert (err[ok] <= bound[ok]).all(), (err[ok] / np.where(bound[ok] > 0, bound[ok], 1)).max()
    print(f"M{M} S{S} R{R}: {n} arrivals, {int(flip.sum())} flipped tubes, {int(bad.sum())} cells left out; worst TL "
          f"error {np.max(err[ok] / np.where(bound[ok] > 0, bound[ok], 1), initial=0.0):.3g} of the bound")


@pytest.mark.parametrize("M, S, R, w_min", BEAM_CASES, ids=[f"M{M}-S{S}-R{R}-w{w}" for M, S, R, w in BEAM_CASES])
def test_contracted_beams_on_synthetic_inputs(clib, syn_env, M, S, R, w_min):
    """The 4-sigma term set (fmax / fabs of differences and a correctly rounded divide: no fusable operation) is the
    restatement's outside the flipped tubes' reach; the values within sum_t term_t (b_A,t + 2 GEXP_CONTRACTED_ULPS eps
    + 2 u) + 2 (n - 1) u I, b_A = max(b_g) + 10 u (E and A: two more operations than TL's I), n <= 3 x the column's
    valid tubes (three centres each)."""
    import beam_reference as bref
    from tube_gpu import SYN_R, SYN_Z, _device_beams, synthetic_fan
    env, cin = syn_env
    z, p, x, p0, depths = synthetic_fan(M, S, R, seed=M * 1013 + S * 37 + R, cin=cin)
    bottom = np.linspace(4700.0, 5150.0, S)
    I = _device_beams(env, z, p, x, p0, bottom, depths, w_min)
    assert np.array_equal(I, _device_beams(env, z, p, x, p0, bottom, depths, w_min), equal_nan=True)
    ref = bref.beam_intensity(z.T, p.T, x, p0, depths, cin, SYN_R, SYN_Z, bottom, w_min)
    b_g, near = _ray_bounds(z, p, x, cin)
    flip = near[:-1] | near[1:]
    assert flip.sum() <= 16, flip.sum()
    valid, m, sigma, E, A, r = bref._tubes(z.T, p.T, x, p0, cin, SYN_R, SYN_Z, w_min)

    def reach(d0, d1, s):
        k = np.nonzero((-z.T[:-1, s] == d0) & (-z.T[1:, s] == d1))[0][0]
        ctr, h = m[k, s], 4.001 * sigma[k, s]
        return [(ctr, h), (-ctr, h), (2.0 * bottom[s] - ctr, h)]
    bad = _flipped_cells(z, x, flip, depths, reach)
    live = x != x[0]
    assert np.array_equal(np.isnan(I), np.isnan(ref)) and np.isnan(I[:, ~live]).all()
    ok = ~bad & live[None, :]
    assert np.array_equal(I[ok] == 0, ref[ok] == 0)
    b_A = np.fmax(b_g[:-1], b_g[1:]) + 10 * U
    e1 = bref.beam_intensity(z.T, p.T, x, p0, depths, cin, SYN_R, SYN_Z, bottom, w_min, a_scale=b_A)
    n_terms = 3 * valid.sum(axis=0)[None, :]
    bound = e1 + ref * (2 * bref.GEXP_CONTRACTED_ULPS * EPS + 2 * U + 2 * np.maximum(n_terms - 1, 0) * U)
    err = np.abs(I - ref)
    assert (err[ok] <= bound[ok]).all(), (err[ok] / np.where(bound[ok] > 0, bound[ok], 1)).max()
    if M >= 8:
        assert (I[ok] > 0).any()
