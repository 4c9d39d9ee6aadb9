"""Path integrals and volume absorption on the GPU (csrc/pgr_path.h and the weights of csrc/pgr_tl.h): the kernel alone
through the _device entries against the restatement of tests/path_reference.py, fans in both trajectory layouts (dropped rays,
backwards, flat earth; the frame from tests/frame_independent.py), and the weighted tube products: the identities that hold
in either arithmetic (`pr_any`; test_identities_hold_in_contracted_arithmetic runs them in a PGR_ARITH=contracted child) and
bit parity with the restatements fed the weighted g (`pr`: the reference arithmetic only)."""
import ctypes
import os
import subprocess
import sys

import numpy as np
import pytest

import arrivals_reference as aref
import frame_independent as fi
import path_reference as pref
import tl_reference as tlr
from tube_gpu import (DEPTHS, SYN_R, SYN_Z, _device_arrivals, _device_beams, _device_intensity, _env, _same, _upload,  # noqa: F401
                      munk_env, pr, pr_any, sloping_env, sloping_env_shallow_table, syn_env, synthetic_fan)

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
PAD = 130                    # entries behind an output that must stay as they were
MARK = -7.25

PROFILES = {1: (None, np.array([3.5e-4])),
            2: (np.array([500.0, 3000.0]), np.array([1e-4, 6e-4])),
            7: (np.array([0.0, 40.0, 41.0, 900.0, 2500.0, 2500.5, 5000.0]), np.array([5e-4, 4e-4, 0.0, 2e-4, 2e-4, 9e-4, 1e-4]))}
FAN_PROFILE = ([0.0, 300.0, 1200.0, 4000.0], [0.9, 0.5, 0.08, 0.2])          # dB/km, as the public functions take it


# ---- the kernel alone ----------------------------------------------------------------------------------------------------

def synthetic_paths(M, S, seed):
    """T, z (S, M) stored convention and x (S,) for pgr_path_integral_device: depths in and outside the table and the
    profiles' nodes, some exactly on nodes; NaN runs: a NaN first sample (ray 0), a NaN last sample (ray M - 1), a NaN depth
    and a NaN time mid-ray"""
    rng = np.random.default_rng(seed)
    x = np.linspace(0.0, 55e3, S)
    d = rng.uniform(-200.0, 5200.0, (S, M))
    nodes = np.concatenate([a for a, _ in PROFILES.values() if a is not None] + [SYN_Z[::9]])
    on = rng.random((S, M)) < 0.15
    d[on] = rng.choice(nodes, int(on.sum()))
    T = np.cumsum(rng.uniform(0.2, 1.5, (S, M)), axis=0)
    if M >= 2:
        d[0, 0] = T[0, 0] = np.nan
    d[S - 1, M - 1] = T[S - 1, M - 1] = np.nan
    if M >= 8 and S >= 5:
        d[S // 2, M // 2] = np.nan
        T[S // 3, M // 3] = np.nan
    return T, -d, x


def _device_path(env, T, z, x, a_depths, alpha):
    """_lib.path_integral_device on [S][M] rows -> A (M, S); the output pre-filled with a sentinel, PAD entries behind it
    checked untouched"""
    import torch
    from pygenray_amd import _lib
    (dT, dz, dx), stream = _upload(env, T, z, x)
    S, M = z.shape
    out = torch.full((S * M + PAD,), MARK, dtype=torch.float64, device=dT.device)
    _lib.path_integral_device(env, dT.data_ptr(), dz.data_ptr(), M, S, dx.data_ptr(), a_depths, alpha, out.data_ptr(), stream)
    h = out.cpu().numpy()
    assert (h[S * M:] == MARK).all()
    return h[:S * M].reshape(S, M).T


@pytest.mark.parametrize("S", [1, 2, 5, 200, 1001])
@pytest.mark.parametrize("M", [1, 63, 64, 65, 4035])
def test_kernel_bit_identical_to_the_restatement_on_synthetic_buffers(pr, syn_env, M, S):
    env, cin = syn_env
    T, z, x = synthetic_paths(M, S, 1000 * M + S)
    for n_a, (a_depths, alpha) in PROFILES.items():
        A = _device_path(env, T, z, x, a_depths, alpha)
        ref = pref.path_integral(T.T, z.T, x, a_depths, alpha, cin, SYN_R, SYN_Z)
        assert A.shape == (M, S)
        bad = ~((A == ref) | (np.isnan(A) & np.isnan(ref)))
        assert not bad.any(), (n_a, np.argwhere(bad)[:5], A[bad][:5], ref[bad][:5])
        assert (A[:, 0] == 0).all()                                     # every entry written, column 0 with 0.0
        if S >= 2:
            assert np.isnan(A[M - 1, S - 1]) and (M < 2 or np.isnan(A[0, 1:]).all())
        if M >= 8 and S >= 5:
            assert np.isnan(A[M // 2, S // 2:]).all() and not np.isnan(A[M // 2, :S // 2]).any()
            assert np.isnan(A[M // 3, S // 3:]).all() and (np.diff(A[1]) >= 0).all() and A[1, -1] > 0


def test_a_second_call_gives_the_same_array_and_alpha_one_is_the_path_length(pr_any, syn_env):
    env, cin = syn_env
    T, z, x = synthetic_paths(700, 333, 5)
    a, b = (_device_path(env, T, z, x, *PROFILES[7]) for _ in range(2))
    assert _same(a, b)
    L = _device_path(env, T, z, x, None, np.ones(1))
    ref = pref.path_integral(T.T, z.T, x, None, np.ones(1), cin, SYN_R, SYN_Z)
    ok = ~np.isnan(ref)
    assert np.array_equal(np.isnan(L), ~ok) and np.allclose(L[ok], ref[ok], rtol=1e-12, atol=0)


def test_weights_kernel_bit_identical_to_the_restatement(pr):
    import torch
    from pygenray_amd import _lib
    rng = np.random.default_rng(2)
    cut = 700.0 / pref.LN10_10
    A = np.concatenate([[0.0, -0.0, np.nan, np.inf, 1e6, np.nextafter(cut, 0), cut, np.nextafter(cut, np.inf), 3040.0, 10.0],
                        rng.uniform(0.0, 3100.0, 5000), rng.uniform(0.0, 30.0, 5000), 10.0 ** rng.uniform(-300, 1, 1000)])
    dev = torch.device("cuda", 0)
    dA = torch.from_numpy(A).to(dev)
    dW = torch.full((len(A) + PAD,), MARK, dtype=torch.float64, device=dev)
    _lib.absorption_weights_device(0, dA.data_ptr(), len(A), dW.data_ptr(), torch.cuda.current_stream(dev).cuda_stream)
    W = dW.cpu().numpy()
    assert (W[len(A):] == MARK).all()
    ref = pref.weights(A)
    assert _same(W[:len(A)], ref) and W[0] == 1.0 and W[1] == 1.0 and np.isnan(W[2]) and W[3] == 0 and W[7] == 0 and W[5] > 0
    _lib.absorption_weights_device(0, dA.data_ptr(), len(A), dA.data_ptr(), torch.cuda.current_stream(dev).cuda_stream)
    assert _same(dA.cpu().numpy(), ref)                                 # in place


# ---- fans ----------------------------------------------------------------------------------------------------------------

def _shoot(pr, env, resident, src=(1000.0, 0.0), x1=100e3, S=201, n=300, flatearth=False, amax=20.0):
    return pr.shoot_rays(src[0], src[1], np.linspace(-amax, amax, n), x1, S, env, flatearth=flatearth, debug=False,
                         device_resident=resident)


def _in_place(fan):
    assert fan.device_resident
    assert not any(k in fan.__dict__ for k in ("_ts", "_zs", "_ps"))


def _check_fan(pr, dev, eager, env, flatearth=False):
    """path_length and path_loss of the device-resident fan `dev` and of the same fan shot eagerly, bit for bit against
    the restatement on the eager fan in the frame frame_independent derives"""
    M, S = np.shape(eager.zs)
    assert len(dev) == M and M > 0
    L_ref = pref.fan_path_integral(eager, env, None, flatearth)
    A_ref = pref.fan_path_integral(eager, env, FAN_PROFILE, flatearth)
    assert not np.isnan(L_ref).any() and (L_ref[:, 0] == 0).all() and (np.diff(L_ref, axis=1) > 0).all()
    x = np.asarray(eager.rs[0], dtype=float)
    assert (L_ref[:, -1] >= (1 - 1e-6) * abs(x[-1] - x[0])).all() and (L_ref[:, -1] < 1.2 * abs(x[-1] - x[0])).all()
    L = pr.path_length(dev, env, flatearth=flatearth)
    _in_place(dev)
    assert L.shape == (M, S) and L.dtype == np.float64 and _same(L, L_ref)
    cols = [0, 1, S // 2, -1, S // 2, 3]
    A = pr.path_loss(dev, env, FAN_PROFILE, flatearth=flatearth, range_indices=cols)
    _in_place(dev)
    assert A.shape == (M, len(cols)) and _same(A, A_ref[:, cols])
    assert _same(pr.path_loss(dev, env, 0.07, flatearth=flatearth, range_indices=[-1]),
                 pref.fan_path_integral(eager, env, 0.07, flatearth)[:, -1:])
    # the host path: one answer
    assert _same(pr.path_length(eager, env, flatearth=flatearth), L_ref)
    assert _same(pr.path_loss(eager, env, FAN_PROFILE, flatearth=flatearth), A_ref)
    assert _same(pr.path_length(dev, env, flatearth=flatearth, range_indices=[S - 1]), L_ref[:, -1:])      # and again
    _in_place(dev)


@pytest.mark.parametrize("which", ["munk", "sloping"])
def test_fans_in_place_in_both_layouts(pr, which):
    """rows on the LDS-table Munk environment, sample-blocked on the HBM-table sloping one"""
    env = munk_env(pr) if which == "munk" else sloping_env(pr)
    dev, eager = _shoot(pr, env, True), _shoot(pr, env, False)
    assert dev._dev._env.blocked_layout == (which == "sloping")
    _check_fan(pr, dev, eager, env)


@pytest.mark.parametrize("which", ["munk", "sloping"])
def test_dropped_rays_are_skipped_through_the_keep_list(pr, which):
    env = munk_env(pr, ztop=4200.0) if which == "munk" else sloping_env_shallow_table(pr)
    dev, eager = _shoot(pr, env, True), _shoot(pr, env, False)
    assert 0 < len(eager) < 300 and dev._dev.N == 300 and dev._dev.M == len(eager)
    assert dev._dev._env.blocked_layout == (which == "sloping")
    _check_fan(pr, dev, eager, env)


def test_backwards_fan(pr):
    env = sloping_env(pr)
    kw = dict(src=(900.0, 150e3), x1=40e3, S=111, n=90, amax=12.0)
    dev, eager = _shoot(pr, env, True, **kw), _shoot(pr, env, False, **kw)
    assert eager.rs[0, 0] == 150e3 and eager.rs[0, -1] == 40e3
    _check_fan(pr, dev, eager, env)


def test_default_flat_earth_environment(pr):
    env = pr.OceanEnvironment2D()
    kw = dict(x1=90e3, S=181, n=200, flatearth=True, amax=12.0)
    dev, eager = _shoot(pr, env, True, **kw), _shoot(pr, env, False, **kw)
    _check_fan(pr, dev, eager, env, flatearth=True)


# ---- weighted products: the identities (either arithmetic) -----------------------------------------------------------------

ARR_FIELDS = ("offsets", "tube", "w", "time", "p", "intensity", "launch_angle", "amplitude", "received_angle",
              "turning_points", "ray_number", "ranges", "range_indices", "receiver_depths")


@pytest.mark.parametrize("which, resident", [("munk", True), ("sloping", True), ("sloping", False)])
def test_identity_zero_absorption_leaves_every_product_bit_equal(pr_any, which, resident):
    env = munk_env(pr_any) if which == "munk" else sloping_env(pr_any)
    fan = _shoot(pr_any, env, resident, n=700, S=101)
    d = DEPTHS[::10]
    for zero in (0.0, ([0.0, 1000.0], [0.0, 0.0])):
        a = pr_any.transmission_loss(fan, d, env, flatearth=False, intensity=True)
        b = pr_any.transmission_loss(fan, d, env, flatearth=False, intensity=True, absorption=zero)
        assert _same(a, b) and (a[:, 1:] > 0).mean() > 0.3
        a = pr_any.beam_transmission_loss(fan, d, env, flatearth=False, min_width=15.0)
        b = pr_any.beam_transmission_loss(fan, d, env, flatearth=False, min_width=15.0, absorption=zero)
        assert _same(a, b) and np.isfinite(a[:, 1:]).mean() > 0.3
        a = pr_any.arrivals(fan, d, env, flatearth=False, range_indices=[50, -1, 3])
        b = pr_any.arrivals(fan, d, env, flatearth=False, range_indices=[50, -1, 3], absorption=zero)
        assert len(a) > 100
        for k in ARR_FIELDS:
            assert _same(np.asarray(getattr(a, k)), np.asarray(getattr(b, k))), k
    if resident:
        _in_place(fan)


@pytest.mark.parametrize("which, resident", [("munk", True), ("sloping", False)])
def test_identity_weighted_arrivals_add_up_to_the_weighted_tl_and_are_the_unweighted_ones_otherwise(pr_any, which, resident):
    env = munk_env(pr_any) if which == "munk" else sloping_env(pr_any)
    fan = _shoot(pr_any, env, resident, n=700, S=101)
    d = DEPTHS[::10]
    cols = [50, 100, 3]
    heavy = ([0.0, 300.0, 1200.0, 4000.0], [0.9, 0.5, 0.3, 0.4])             # dB/km: 30 to 90 dB over 100 km
    a = pr_any.arrivals(fan, d, env, flatearth=False, range_indices=cols)
    b = pr_any.arrivals(fan, d, env, flatearth=False, range_indices=cols, absorption=heavy)
    assert len(a) > 100
    for k in ARR_FIELDS:
        if k not in ("intensity", "amplitude"):                               # counts, offsets, order, T, p: unchanged
            assert _same(np.asarray(getattr(a, k)), np.asarray(getattr(b, k))), k
    assert (b.intensity < a.intensity).all() and (b.intensity > 0).all()
    assert _same(b.amplitude, np.sqrt(b.intensity))
    I = pr_any.transmission_loss(fan, d, env, flatearth=False, intensity=True, absorption=heavy)
    assert _same(aref.sequential_sums(b.offsets, b.intensity).reshape(len(d), len(cols)), I[:, cols])
    I0 = pr_any.transmission_loss(fan, d, env, flatearth=False, intensity=True)
    lit = I0[:, 1:] > 0
    assert np.array_equal(I[:, 1:] > 0, lit) and (I[:, 1:][lit] < I0[:, 1:][lit]).all()
    # ... and each arrival lost what its two edge rays lost: between the smaller and the larger of their path losses
    A = pr_any.path_loss(fan, env, heavy, flatearth=False, range_indices=cols)
    slot = np.repeat(np.arange(len(a.offsets) - 1), np.diff(a.offsets)) % len(cols)
    loss = 10 * np.log10(a.intensity / b.intensity)
    lo, hi = np.minimum(A[a.tube, slot], A[a.tube + 1, slot]), np.maximum(A[a.tube, slot], A[a.tube + 1, slot])
    assert (loss >= lo - 1e-9).all() and (loss <= hi + 1e-9).all() and loss.max() > 10.0
    if resident:
        _in_place(fan)


def image_intensity_absorbed(ranges, depths, source_depth, water_depth, max_angle_deg, alpha_db_per_m):
    """tl_reference.image_intensity with volume absorption: sum over the images of 10^(-alpha R / 10) / R^2"""
    r = np.asarray(ranges, dtype=float)[None, :, None]
    d = np.asarray(depths, dtype=float)[:, None, None]
    tmax = np.tan(np.radians(max_angle_deg))
    nmax = int(np.ceil(tmax * np.max(ranges) / (2 * water_depth))) + 2
    n = np.arange(-nmax, nmax + 1)
    zi = np.concatenate([2 * n * water_depth + source_depth, 2 * n * water_depth - source_depth])[None, None, :]
    dz = np.abs(zi - d)
    R2 = r * r + dz * dz
    return np.where(dz <= tmax * r, 10.0 ** (-alpha_db_per_m * np.sqrt(R2) / 10.0) / R2, 0.0).sum(axis=2)


def test_identity_isovelocity_fan_with_constant_absorption_matches_the_absorbed_image_sum(pr_any):
    # the fan, receivers, ranges and tolerance of test_transmission_loss.py's isovelocity test; 1 dB/km: 20 dB at 20 km on
    # the direct path and 115 dB on the steepest one, so a weight taken at the wrong path length misses by far more than 0.1 dB
    z = np.arange(0, 6000, 10.0)
    r = np.linspace(0, 25e3, 6)
    env = _env(pr_any, z, r, np.full((len(r), len(z)), 1500.0), r, np.full(len(r), 5000.0))
    fan = pr_any.shoot_rays(1000.0, 0.0, np.linspace(-80, 80, 20001), 20e3, 2001, env, flatearth=False, debug=False)
    assert len(fan) == 20001 and fan.device_resident
    depths = np.arange(tlr.MARGIN, 5000 - tlr.MARGIN + 1, 50.0)
    tl = pr_any.transmission_loss(fan, depths, env, flatearth=False, absorption=1.0)
    x = np.asarray(fan.rs[0])
    keep = (x >= 1e3) & (x <= 20e3)
    ref = tlr.to_db(image_intensity_absorbed(x[keep], depths, 1000.0, 5000.0, 80.0, 1e-3))
    err = np.abs(tl[:, keep] - ref)
    j, k = np.unravel_index(np.argmax(err), err.shape)
    print(f"absorbed image sum: worst {err.max():.4f} dB at depth {depths[j]} m, range {x[keep][k]} m")
    assert err.max() < tlr.TOL_DB, (err.max(), depths[j], x[keep][k])
    plain = tlr.to_db(tlr.image_intensity(x[keep], depths, 1000.0, 5000.0, 80.0))
    assert np.abs(ref - plain).max() > 20.0 and fan.device_resident
    L = pr_any.path_length(fan, env, flatearth=False, range_indices=[-1])[:, 0]       # straight rays: L = r / cos(theta)
    # (the tracer's travel times are held to 1e-8 relative; a hundred times that)
    assert np.allclose(L, 20e3 / np.cos(np.radians(fan.thetas)), rtol=1e-6)


def test_identities_hold_in_contracted_arithmetic():
    from pygenray_amd import _lib
    if _lib.ARITH != "reference":
        pytest.skip("this IS the contracted process")
    if not os.path.exists(_lib.CONTRACTED_LIB):
        pytest.fail("libpgr_hip_fma.so is not built (__graft_entry__.build() builds it beside the product)")
    out = subprocess.run([sys.executable, "-m", "pytest", "-q", "-m", "gpu", "-x", "-p", "no:cacheprovider", "-k", "identity",
                          os.path.join(ROOT, "tests", "test_path_loss.py")],
                         cwd=ROOT, env=dict(os.environ, PGR_ARITH="contracted"), capture_output=True, text=True, timeout=900)
    tail = out.stdout[-3000:] + out.stderr[-1500:]
    assert out.returncode == 0 and " passed" in out.stdout and "failed" not in out.stdout, tail


# ---- weighted products: bit parity with the restatements fed the weighted g -------------------------------------------------

def synthetic_weights(M, S, seed, with_nan=False):
    """(S, M) weights for synthetic_fan's samples: in (0, 1], with exact ones and zeros, and (with_nan) two NaNs"""
    rng = np.random.default_rng(seed)
    W = 10.0 ** rng.uniform(-6.0, 0.0, (S, M))
    W[rng.random((S, M)) < 0.05] = 1.0
    W[rng.random((S, M)) < 0.02] = 0.0
    if with_nan and M >= 8:
        W[S - 1, M // 6] = W[0, M - 2] = np.nan
    return W


def _weighted(env, arrays, call):
    """upload `arrays`, call(pointers..., stream)"""
    t, stream = _upload(env, *arrays)
    return call(*(a.data_ptr() for a in t), stream)


def _device_intensity_w(env, z, p, x, p0, depths, W, beams=None):
    import torch
    from pygenray_amd import _lib
    S, M = z.shape
    out = torch.full((len(depths) * S + PAD,), MARK, dtype=torch.float64, device=torch.device("cuda", env.device))
    if beams is None:
        _weighted(env, (z, p, x, p0, depths, W), lambda dz, dp, dx, d0, dd, dw, st: _lib.intensity_device(
            env, dz, dp, M, S, dx, d0, dd, len(depths), out.data_ptr(), st, weights=dw))
    else:
        bottom, w_min = beams
        _weighted(env, (z, p, x, p0, bottom, depths, W), lambda dz, dp, dx, d0, db, dd, dw, st: _lib.beam_intensity_device(
            env, dz, dp, M, S, dx, d0, db, dd, len(depths), w_min, out.data_ptr(), st, weights=dw))
    h = out.cpu().numpy()
    assert (h[len(depths) * S:] == MARK).all()
    return h[:len(depths) * S].reshape(len(depths), S)


def _device_arrivals_w(env, t, z, p, x, p0, depths, cols, W):
    """tube_gpu._device_arrivals with the emit pass weighted (the counts have no weighted twin)"""
    import torch
    from pygenray_amd import _lib
    plain = _device_arrivals(env, t, z, p, x, p0, depths, cols)
    total = int(plain["offsets"][-1])
    if total == 0:
        return plain, plain
    d, stream = _upload(env, t, z, p, x, p0, depths, W)
    dev = d[0].device
    S, M = z.shape
    offsets = torch.from_numpy(plain["offsets"]).to(dev)
    tube = torch.full((total + PAD,), -1, dtype=torch.int32, device=dev)
    f = [torch.full((total + PAD,), MARK, dtype=torch.float64, device=dev) for _ in range(4)]
    _lib.arrivals_device(env, d[0].data_ptr(), d[1].data_ptr(), d[2].data_ptr(), M, S, d[3].data_ptr(), d[4].data_ptr(),
                         d[5].data_ptr(), len(depths), cols, offsets.data_ptr(), total, tube.data_ptr(),
                         *(a.data_ptr() for a in f), stream, weights=d[6].data_ptr())
    got = dict(offsets=plain["offsets"], tube=tube.cpu().numpy(), **{k: a.cpu().numpy() for k, a in zip(("w", "T", "p", "I"), f)})
    for k in ("tube", "w", "T", "p", "I"):
        assert (got[k][total:] == (-1 if k == "tube" else MARK)).all()
        got[k] = got[k][:total]
    return got, plain


SEAM_CASES = [(M, 5, 129, False) for M in (2, 63, 64, 65, 127, 4034)] + [(500, 5, R, False) for R in (1, 64, 65)] + \
    [(300, 2, 100, False), (4100, 6, 300, True)]


@pytest.mark.parametrize("M, S, R, shuffle", SEAM_CASES, ids=[f"M{M}-S{S}-R{R}{'-shuffled' if sh else ''}"
                                                               for M, S, R, sh in SEAM_CASES])
def test_weighted_kernels_bit_identical_on_the_synthetic_seam_cases(pr, syn_env, M, S, R, shuffle):
    env, cin = syn_env
    z, p, x, p0, depths = synthetic_fan(M, S, R, seed=M * 1009 + S * 31 + R, cin=cin, shuffle=shuffle)
    rng = np.random.default_rng(M + S + R)
    t = np.cumsum(rng.uniform(0.2, 1.5, (S, M)), axis=0)
    for with_nan in (False, True):
        W = synthetic_weights(M, S, M + 7 * S + R, with_nan)
        I = _device_intensity_w(env, z, p, x, p0, depths, W)
        ref = pref.tube_intensity(z.T, p.T, x, p0, depths, cin, SYN_R, SYN_Z, W.T)
        assert _same(I, ref), np.argwhere(~((I == ref) | (np.isnan(I) & np.isnan(ref))))[:5]
        if M >= 8 and S >= 3:
            assert (I[:, x != x[0]] > 0).any() and not _same(I, _device_intensity(env, z, p, x, p0, depths))
        bottom = np.linspace(4700.0, 5150.0, S)
        B = _device_intensity_w(env, z, p, x, p0, depths, W, beams=(bottom, 25.0))
        assert _same(B, pref.beam_intensity(z.T, p.T, x, p0, depths, cin, SYN_R, SYN_Z, bottom, 25.0, W.T))
    # the arrivals (finite weights: the tubes counted are the unweighted call's)
    W = synthetic_weights(M, S, M + 7 * S + R)
    cols = list(range(S)) + [0]
    got, plain = _device_arrivals_w(env, t, z, p, x, p0, depths, cols, W)
    ref = pref.tube_arrivals(z.T, p.T, t.T, x, p0, depths, cols, cin, SYN_R, SYN_Z, W.T)
    assert np.array_equal(got["offsets"], ref["offsets"])
    for k in ("tube", "w", "T", "p", "I"):
        assert _same(got[k], ref[k]), k
        if k != "I":
            assert _same(got[k], plain[k]), k
    Iw = _device_intensity_w(env, z, p, x, p0, depths, W)
    assert _same(aref.sequential_sums(got["offsets"], got["I"]).reshape(R, len(cols)), np.nan_to_num(Iw[:, cols], nan=0.0))
    # no weights: the restatements of tl_reference / arrivals_reference themselves (W = None is their g)
    assert _same(pref.tube_intensity(z.T, p.T, x, p0, depths, cin, SYN_R, SYN_Z, None),
                 tlr.tube_intensity(z.T, p.T, x, p0, depths, cin, SYN_R, SYN_Z))
    none = pref.tube_arrivals(z.T, p.T, t.T, x, p0, depths, cols, cin, SYN_R, SYN_Z, None)
    same = aref.tube_arrivals(z.T, p.T, t.T, x, p0, depths, cols, cin, SYN_R, SYN_Z)
    assert all(_same(none[k], same[k]) for k in same)


def test_weights_that_overflowed_give_the_ieee_quotient(pr, syn_env):
    """A path integral that comes out hugely negative (a sample extrapolated far out of the sound-speed table, where the
    bilinear c is negative) makes W = 10^(-A / 10) infinite: the tube's term is then inf / finite = inf, not the NaN the
    refined-reciprocal division forms by itself -- in TL, the arrivals and the beams, next to a neighbour of weight 0"""
    env, cin = syn_env
    M, S, R = 130, 4, 40
    z, p, x, p0, depths = synthetic_fan(M, S, R, seed=77, cin=cin)
    rng = np.random.default_rng(5)
    t = np.cumsum(rng.uniform(0.2, 1.5, (S, M)), axis=0)
    W = synthetic_weights(M, S, 9)
    W[:, 10:M:23] = np.inf
    W[:, 11:M:23] = 0.0
    W[1, 64] = W[1, 65] = np.inf
    ref = pref.tube_intensity(z.T, p.T, x, p0, depths, cin, SYN_R, SYN_Z, W.T)
    assert np.isinf(ref).any()
    I = _device_intensity_w(env, z, p, x, p0, depths, W)
    assert _same(I, ref), np.argwhere(~((I == ref) | (np.isnan(I) & np.isnan(ref))))[:5]
    bottom = np.linspace(4700.0, 5150.0, S)
    ref = pref.beam_intensity(z.T, p.T, x, p0, depths, cin, SYN_R, SYN_Z, bottom, 25.0, W.T)
    assert np.isinf(ref).any()
    assert _same(_device_intensity_w(env, z, p, x, p0, depths, W, beams=(bottom, 25.0)), ref)
    cols = list(range(S))
    got, _ = _device_arrivals_w(env, t, z, p, x, p0, depths, cols, W)
    ref = pref.tube_arrivals(z.T, p.T, t.T, x, p0, depths, cols, cin, SYN_R, SYN_Z, W.T)
    assert np.array_equal(got["offsets"], ref["offsets"]) and np.isinf(ref["I"]).any()
    for k in ("tube", "w", "T", "p", "I"):
        assert _same(got[k], ref[k]), k


@pytest.mark.parametrize("which, resident, flatearth", [("munk", True, False), ("sloping", True, False), ("sloping", False, False),
                                                        ("default", True, True)])
def test_weighted_fan_products_bit_identical_to_the_restatements(pr, which, resident, flatearth):
    env = {"munk": munk_env, "sloping": sloping_env, "default": lambda p: p.OceanEnvironment2D()}[which](pr)
    kw = dict(n=500, S=81, x1=80e3, flatearth=flatearth)
    fan, eager = _shoot(pr, env, resident, **kw), _shoot(pr, env, False, **kw)
    d = DEPTHS[::20]
    cols = [40, 80, 1]
    xf, cin, rin, zin, bd, br = fi.traced_frame(env, np.asarray(eager.rs[0], dtype=float), flatearth)
    p0 = fi.launch_slowness(eager.thetas, eager.source_depths[0], xf, cin, rin, zin)
    W = pref.weights(pref.fan_path_integral(eager, env, FAN_PROFILE, flatearth))
    assert W.shape == eager.zs.shape and (W[:, 0] == 1).all() and (W[:, -1] < 0.999).all() and (W > 0).all()
    I = pr.transmission_loss(fan, d, env, flatearth=flatearth, intensity=True, absorption=FAN_PROFILE)
    assert _same(I, pref.tube_intensity(eager.zs, eager.ps, xf, p0, d, cin, rin, zin, W)) and (I[:, 1:] > 0).mean() > 0.3
    B = pr.beam_transmission_loss(fan, d, env, flatearth=flatearth, intensity=True, min_width=20.0, absorption=FAN_PROFILE)
    assert _same(B, pref.beam_intensity(eager.zs, eager.ps, xf, p0, d, cin, rin, zin, fi.bottom_at(xf, bd, br), 20.0, W))
    a = pr.arrivals(fan, d, env, flatearth=flatearth, range_indices=cols, absorption=FAN_PROFILE)
    ref = pref.tube_arrivals(eager.zs, eager.ps, eager.ts, xf, p0, d, cols, cin, rin, zin, W)
    assert len(a) > 50 and np.array_equal(a.offsets, ref["offsets"])
    for k, name in (("tube", "tube"), ("w", "w"), ("T", "time"), ("p", "p"), ("I", "intensity")):
        assert _same(ref[k], getattr(a, name)), k
    if resident:
        _in_place(fan)


# ---- the error paths of the C entries ----------------------------------------------------------------------------------------

def test_c_entries_refuse_bad_arguments_before_writing_anything(pr_any, syn_env):
    import torch
    from pygenray_amd import _lib
    env, cin = syn_env
    L = _lib.load()
    M, S = 70, 6
    T, z, x = synthetic_paths(M, S, 1)
    (dT, dz, dx), stream = _upload(env, T, z, x)
    out = torch.full((S * M,), MARK, dtype=torch.float64, device=dT.device)
    vp = ctypes.c_void_p

    def arr(v):
        a = np.ascontiguousarray(v, dtype=np.float64)
        return a, vp(a.ctypes.data)

    def call(a_depths, alpha, n_a, o=out, Tp=dT, env_h=env._h):
        keep = [arr(a_depths) if a_depths is not None else (None, None), arr(alpha) if alpha is not None else (None, None)]
        rc = L.pgr_path_integral_device(env_h, vp(Tp.data_ptr()) if Tp is not None else None, vp(dz.data_ptr()), M, S,
                                        vp(dx.data_ptr()), keep[0][1], keep[1][1], n_a,
                                        vp(o.data_ptr()) if o is not None else None, vp(stream))
        return rc, L.pgr_last_error().decode()

    bad = [(([0.0, 1.0], [1e-4, 1e-4], 0), "n_a"), (([0.0, 1.0], [1e-4, 1e-4], -3), "n_a"),
           (([0.0, 0.0], [1e-4, 1e-4], 2), "ascending"), (([5.0, 1.0], [1e-4, 1e-4], 2), "ascending"),
           (([0.0, np.nan], [1e-4, 1e-4], 2), "ascending"), (([0.0, 1.0], [1e-4, -1e-4], 2), "alpha"),
           (([0.0, 1.0], [np.nan, 1e-4], 2), "alpha"), (([0.0, 1.0], [np.inf, 1e-4], 2), "alpha"),
           ((None, [1e-4, 1e-4], 2), "a_depths"), (([0.0, 1.0], None, 2), "null")]
    for args, msg in bad:
        rc, err = call(*args)
        assert rc < 0 and "pgr_path_integral_device" in err and msg in err, (args, rc, err)
    for kw in (dict(o=None), dict(Tp=None), dict(env_h=None)):
        rc, err = call([0.0, 1.0], [1e-4, 1e-4], 2, **kw)
        assert rc < 0 and "pgr_path_integral_device" in err and "null" in err
    assert (out.cpu().numpy() == MARK).all()                            # nothing was written
    rc, err = call(None, [1e-4], 1)                                      # and the same buffers with a good profile: written
    assert rc == 0 and not (out.cpu().numpy() == MARK).any()
    # the fan entry: the same checks, by name
    fan = _shoot(pr_any, munk_env(pr_any), True, n=70, S=6, x1=20e3)
    out.fill_(MARK)
    for a_depths, alpha, msg in (([1.0, 0.5], [1e-4, 1e-4], "ascending"), ([0.0, 1.0], [-1.0, 0.0], "alpha")):
        with pytest.raises(_lib.PgrError, match="pgr_fan_path_integral.*" + msg):
            fan._dev.path_integral(a_depths, alpha, out.data_ptr(), stream)
    rc = L.pgr_absorption_weights_device(0, None, 5, vp(out.data_ptr()), vp(stream))
    assert rc < 0 and "pgr_absorption_weights_device" in L.pgr_last_error().decode()
    rc = L.pgr_absorption_weights_device(0, vp(out.data_ptr()), 0, vp(out.data_ptr()), vp(stream))
    assert rc < 0
    # a weighted twin names itself and refuses what its unweighted entry refuses
    zf, p, xx, p0, depths = synthetic_fan(M, S, 9, seed=4, cin=cin)
    t, stream = _upload(env, zf, p, xx, p0, depths, np.ones((S, M)), np.full(S, 5000.0))
    with pytest.raises(_lib.PgrError, match="pgr_beam_intensity_device_w: min_width"):
        _lib.beam_intensity_device(env, t[0].data_ptr(), t[1].data_ptr(), M, S, t[2].data_ptr(), t[3].data_ptr(),
                                   t[6].data_ptr(), t[4].data_ptr(), 9, -1.0, out.data_ptr(), stream, weights=t[5].data_ptr())
    with pytest.raises(_lib.PgrError, match="pgr_intensity_device_w: need at least two rays"):
        _lib.intensity_device(env, t[0].data_ptr(), t[1].data_ptr(), 1, S, t[2].data_ptr(), t[3].data_ptr(), t[4].data_ptr(), 9,
                              out.data_ptr(), stream, weights=t[5].data_ptr())
    assert (out.cpu().numpy() == MARK).all()
