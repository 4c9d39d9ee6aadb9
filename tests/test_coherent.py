"""Caustic index and coherent ray-tube pressure on the GPU (csrc/pgr_phase.h): the kernels alone through the _device entries
against the restatement of tests/coherent_reference.py on synthetic buffers aimed at their seams, fans in both trajectory
layouts (dropped rays, host fans), an independent path (the sum formed in NumPy from ``arrivals``' own fields), the focusing
medium and Lloyd's mirror end to end, and the identities that hold in either arithmetic (`pr_any`;
test_identities_hold_in_contracted_arithmetic runs them in a PGR_ARITH=contracted child)."""
import ctypes
import os
import subprocess
import sys

import numpy as np
import pytest

import arrivals_reference as aref
import coherent_reference as cref
import path_reference as pref
from tube_gpu import (DEPTHS, SYN_R, SYN_Z, _same, _upload, munk_env, pr, pr_any, sloping_env,  # noqa: F401
                      sloping_env_shallow_table, syn_env, synthetic_fan)

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
PAD = 130                    # entries behind an output that must stay as they were
MARK = -7.25
EPS = np.finfo(float).eps
FAN_PROFILE = ([0.0, 300.0, 1200.0, 4000.0], [0.9, 0.5, 0.08, 0.2])          # dB/km, as the public functions take it


# ---- the caustic scan alone ---------------------------------------------------------------------------------------------------

def synthetic_tubes(M, S, seed):
    """z (S, M) stored convention and counts nb, ns (S, M) int32 for pgr_caustic_index_device: widths that change sign often,
    NaN samples (single and in runs, so that a sign is carried across a gap), equal depths of neighbours, counts that step
    up along s and differ between neighbours here and there"""
    rng = np.random.default_rng(seed)
    d = 2500.0 + np.cumsum(rng.normal(0.0, 30.0, (S, M)), axis=0) + 40.0 * np.arange(M)[None, :]
    d[rng.random((S, M)) < 0.08] = np.nan
    if S >= 5 and M >= 3:
        d[1:3, M // 2] = np.nan                                      # a gap of two samples in one ray
    eq = (rng.random((S, M)) < 0.05) & (np.arange(M)[None, :] > 0)
    d[eq] = np.roll(d, 1, axis=1)[eq]                                # equal depths of neighbours
    nb = (np.cumsum(rng.random(S) < 0.2)[:, None] + np.cumsum(rng.random((S, M)) < 0.03, axis=0)).astype(np.int32)
    ns = (np.cumsum(rng.random(S) < 0.2)[:, None] + np.cumsum(rng.random((S, M)) < 0.03, axis=0)).astype(np.int32)
    return -d, nb, ns


def _device_kappa(z, nb, ns):
    """_lib.caustic_index_device on [S][M] rows -> kappa (S, M); the output pre-filled with a sentinel, PAD entries behind it
    checked untouched"""
    import torch
    from pygenray_amd import _lib
    dev = torch.device("cuda", 0)
    S, M = z.shape
    dz = torch.from_numpy(np.ascontiguousarray(z)).to(dev)
    dn = [None if a is None else torch.from_numpy(np.ascontiguousarray(a, dtype=np.int32)).to(dev) for a in (nb, ns)]
    out = torch.full((S * M + PAD,), -7, dtype=torch.int32, device=dev)
    _lib.caustic_index_device(0, dz.data_ptr(), M, S, *(0 if a is None else a.data_ptr() for a in dn), out.data_ptr(),
                              torch.cuda.current_stream(dev).cuda_stream)
    h = out.cpu().numpy()
    assert (h[S * M:] == -7).all()
    return h[:S * M].reshape(S, M)


@pytest.mark.parametrize("S", [1, 2, 5, 100])
@pytest.mark.parametrize("M", [2, 63, 64, 65, 129])
def test_caustic_scan_equals_the_restatement_on_synthetic_rows(pr_any, M, S):
    z, nb, ns = synthetic_tubes(M, S, 100 * M + S)
    for cnt in ((nb, ns), (None, None), (nb, None)):
        k = _device_kappa(z, *cnt)
        ref = cref.caustic_index(-z.T, *(None if a is None else a.T for a in cnt))
        assert np.array_equal(k[:, :-1].T, ref), np.argwhere(k[:, :-1].T != ref)[:5]
        assert (k[:, -1] == 0).all() and (k[0] == 0).all()
    if S == 100:
        assert ref.max() >= 1 and (M < 63 or ref.max() > 3) and (np.diff(ref, axis=1) >= 0).all()
        assert not np.array_equal(cref.caustic_index(-z.T), cref.caustic_index(-z.T, nb.T, ns.T))     # the counts matter


# ---- the coherent sum alone ---------------------------------------------------------------------------------------------------

def _device_pressure(env, t, z, p, x, p0, depths, W, q, f):
    """_lib.pressure_device on [S][M] rows -> re, im (R, S); sentinels behind both outputs checked untouched"""
    import torch
    from pygenray_amd import _lib
    d, stream = _upload(env, t, z, p, x, p0, depths, *(() if W is None else (W,)))
    dev = d[0].device
    S, M = z.shape
    R = len(depths)
    dq = None if q is None else torch.from_numpy(np.ascontiguousarray(q, dtype=np.int32)).to(dev)
    out = [torch.full((R * S + PAD,), MARK, dtype=torch.float64, device=dev) for _ in range(2)]
    _lib.pressure_device(env, d[0].data_ptr(), d[1].data_ptr(), d[2].data_ptr(), M, S, d[3].data_ptr(), d[4].data_ptr(),
                         0 if dq is None else dq.data_ptr(), f, d[5].data_ptr(), R, out[0].data_ptr(), out[1].data_ptr(),
                         stream, weights=0 if W is None else d[6].data_ptr())
    h = [a.cpu().numpy() for a in out]
    assert all((a[R * S:] == MARK).all() for a in h)
    return tuple(a[:R * S].reshape(R, S) for a in h)


def synthetic_phase(M, S, seed):
    """travel times t (S, M), weights W (S, M) in (0, 1] with exact ones, zeros and two NaNs, and q (S, M) int32 in -1 ... 9"""
    rng = np.random.default_rng(seed)
    t = np.cumsum(rng.uniform(0.2, 1.5, (S, M)), axis=0)
    W = 10.0 ** rng.uniform(-6.0, 0.0, (S, M))
    W[rng.random((S, M)) < 0.05] = 1.0
    W[rng.random((S, M)) < 0.02] = 0.0
    if M >= 8:
        W[S - 1, M // 6] = W[0, M - 2] = np.nan
    q = rng.integers(-1, 10, (S, M)).astype(np.int32)
    return t, W, q


SEAM_CASES = [(M, 5, 129) for M in (2, 3, 63, 64, 65, 127, 128, 4035)] + [(500, 5, R) for R in (1, 63, 64, 65)] + \
    [(300, 1, 100), (300, 2, 100)]


@pytest.mark.parametrize("M, S, R", SEAM_CASES, ids=[f"M{M}-S{S}-R{R}" for M, S, R in SEAM_CASES])
def test_coherent_sum_bit_identical_to_the_restatement_on_the_synthetic_seam_cases(pr, syn_env, M, S, R):
    env, cin = syn_env
    z, p, x, p0, depths = synthetic_fan(M, S, R, seed=M * 1009 + S * 31 + R, cin=cin)
    t, W, q = synthetic_phase(M, S, M + 7 * S + R)
    f = 37.5
    assert S < 4 or (x[S - 2] == x[0])                                  # a column s > 0 with x_s == x_0: NaN
    got = {}
    variants = dict(both=(W, q), q=(None, q), w=(W, None), none=(None, None))
    if M > 1000:                                                        # (the restatement takes 2 s per call there)
        variants = dict(both=(W, q), q=(None, q), none=(None, None))
    for name, (w, qq) in variants.items():
        re, im = got[name] = _device_pressure(env, t, z, p, x, p0, depths, w, qq, f)
        ref = cref.tube_pressure(z.T, p.T, t.T, x, p0, depths, cin, SYN_R, SYN_Z, None if w is None else w.T,
                                 None if qq is None else qq.T, f)
        assert _same(re, ref[0]) and _same(im, ref[1]), (name, np.argwhere(~((re == ref[0]) | (np.isnan(re) & np.isnan(ref[0]))))[:5])
        assert np.array_equal(np.isnan(re), np.broadcast_to(x == x[0], re.shape)) and np.array_equal(np.isnan(re), np.isnan(im))
    if M >= 63 and S >= 2:
        assert (np.nan_to_num(got["none"][0]) != 0).any() and not _same(got["none"][0], got["q"][0])
        assert not _same(got["both"][0], got["q"][0])
    # f = 0: every term is its amplitude -- re is the sum of sqrt(I) over the tubes TL adds, im is 0
    re, im = _device_pressure(env, t, z, p, x, p0, depths, None, None, 0.0)
    ref = cref.tube_pressure(z.T, p.T, t.T, x, p0, depths, cin, SYN_R, SYN_Z, None, None, 0.0)
    lit = x != x[0]
    assert _same(re, ref[0]) and (im[:, lit] == 0).all() and (re[:, lit] >= 0).all()
    I = pref.tube_intensity(z.T, p.T, x, p0, depths, cin, SYN_R, SYN_Z, None)
    assert np.array_equal(re[:, lit] > 0, I[:, lit] > 0)
    if M > 1000:
        return
    # q = 4 is q = 0, and q = -1 everywhere leaves nothing
    four = _device_pressure(env, t, z, p, x, p0, depths, None, np.full((S, M), 4, np.int32), f)
    assert _same(four[0], got["none"][0]) and _same(four[1], got["none"][1])
    gone = _device_pressure(env, t, z, p, x, p0, depths, None, np.full((S, M), -1, np.int32), f)
    assert (gone[0][:, lit] == 0).all() and (gone[1][:, lit] == 0).all()


# ---- fans -----------------------------------------------------------------------------------------------------------------

def _shoot(pr, env, resident, log=True, n=300, S=81, x1=80e3):
    return pr.shoot_rays(1000.0, 0.0, np.linspace(-20.0, 20.0, n), x1, S, env, flatearth=False, debug=False,
                         device_resident=resident, **(dict(max_bounces=40) if log else {}))


def _in_place(fan):
    assert fan.device_resident and not any(k in fan.__dict__ for k in ("_ts", "_zs", "_ps"))


@pytest.mark.parametrize("which", ["munk", "sloping", "munk-dropped", "sloping-dropped"])
def test_fans_in_both_layouts_against_the_restatement(pr, which):
    """rows (munk) and sample-blocked (sloping) fans, with dropped rays skipped through the keep list: caustic_index and
    pressure_field of the device-resident fan and of the same fan on the host, against the restatement on the fetched fan"""
    env = {"munk": munk_env, "sloping": sloping_env, "munk-dropped": lambda p: munk_env(p, ztop=4200.0),
           "sloping-dropped": sloping_env_shallow_table}[which](pr)
    fan, eager = _shoot(pr, env, True), _shoot(pr, env, False)
    assert fan._dev._env.blocked_layout == which.startswith("sloping")
    assert (len(eager) < 300) == which.endswith("dropped") and len(eager) > 50 and fan._dev.N == 300
    S = 81
    nb, ns = eager.bounce_counts(np.arange(S))
    assert which.endswith("dropped") or (ns[:, -1] > 0).sum() > 10
    kref = cref.caustic_index(-np.asarray(eager.zs), nb, ns)
    assert kref.max() >= 1
    for f in (fan, eager):
        k = pr.caustic_index(f, env, flatearth=False)
        assert k.shape == (len(eager) - 1, S) and k.dtype == np.int64 and np.array_equal(k, kref)
    _in_place(fan)
    d = DEPTHS[::20]
    W = pref.weights(pref.fan_path_integral(eager, env, FAN_PROFILE, False))
    for w, kw in ((None, {}), (W, dict(absorption=FAN_PROFILE))):
        ref = cref.fan_pressure(eager, d, env, 25.0, flatearth=False, W=w, nb=nb, ns=ns)
        p = pr.pressure_field(fan, d, env, 25.0, flatearth=False, **kw)
        assert p.shape == (len(d), S) and p.dtype == np.complex128
        assert _same(p.real, ref.real) and _same(p.imag, ref.imag)
        assert np.isnan(p[:, 0]).all() and (np.abs(p[:, 1:]) > 0).mean() > 0.2
        host = pr.pressure_field(eager, d, env, 25.0, flatearth=False, **kw)                 # device and host paths: one answer
        assert _same(host.real, p.real) and _same(host.imag, p.imag)
    _in_place(fan)


def _numpy_sum_from_arrivals(pr_any, fan, env, d, cols, f, **kw):
    """pressure_field's sum formed in NumPy from arrivals()' own T, I and tube with caustic_index's kappa and the fan's bounce
    counts -> (complex (R, n), the arrivals, sum of the amplitudes (R, n))"""
    a = pr_any.arrivals(fan, d, env, flatearth=False, range_indices=cols, **kw)
    kappa = pr_any.caustic_index(fan, env, flatearth=False)
    nb, ns = fan.bounce_counts(cols)
    slot = np.repeat(np.arange(len(a.offsets) - 1), np.diff(a.offsets)) % len(cols)
    col = np.asarray(cols)[slot]
    assert np.array_equal(a.caustics, kappa[a.tube, col]) and a.caustics.dtype == np.int64
    alike = (nb[a.tube, slot] == nb[a.tube + 1, slot]) & (ns[a.tube, slot] == ns[a.tube + 1, slot])
    q = kappa[a.tube, col] + 2 * ns[a.tube, slot]
    t = cref.phase_cycles(a.time, q, f)
    amp = np.where(alike, np.sqrt(a.intensity), 0.0)
    shape = (len(d), len(cols))
    re = aref.sequential_sums(a.offsets, amp * cref.gcos2pi(t)).reshape(shape)
    im = aref.sequential_sums(a.offsets, amp * cref.gsin2pi(t)).reshape(shape)
    return re + 1j * im, a, aref.sequential_sums(a.offsets, amp).reshape(shape)


def test_identity_pressure_field_is_the_sum_over_the_arrivals(pr_any):
    """an independent path: a Munk fan of 2001 rays to 100 km; the same tubes in the same order in either arithmetic, the same
    bits in the reference arithmetic and a derived bound in the contracted one"""
    from pygenray_amd import _lib
    env = munk_env(pr_any)
    fan = _shoot(pr_any, env, True, n=2001, S=101, x1=100e3)
    d, cols, f = DEPTHS[::25], [100, 37, 1], 75.0
    for kw in ({}, dict(absorption=FAN_PROFILE, surface_loss=0.5)):
        ref, a, amps = _numpy_sum_from_arrivals(pr_any, fan, env, d, cols, f, **kw)
        assert len(a) > 200 and a.caustics.max() >= 1
        p = pr_any.pressure_field(fan, d, env, f, flatearth=False, **kw)[:, cols]
        again = pr_any.pressure_field(fan, d, env, f, flatearth=False, **kw)[:, cols]
        assert _same(p.real, again.real) and _same(p.imag, again.imag)                          # two calls are bit-equal
        assert np.array_equal(p != 0, amps > 0)                                                 # the same tubes
        if _lib.ARITH == "reference":
            assert _same(p.real, ref.real) and _same(p.imag, ref.imag)
        else:
            # contracted: per term the phase f T - rint(f T) may be formed by one fused operation instead of two (it differs by
            # at most eps / 2 of f T, in cycles: times 2 pi in the term), the amplitude's square root is within 2 ulp, the two
            # polynomials and the product differ by a few eps of 1, and each of the n adds rounds once: with A the sum of the
            # amplitudes, |dp| <= A (2 pi eps f T_max + (n + 16) eps) for both parts
            n = np.diff(a.offsets).max()
            bound = amps * (2 * np.pi * EPS * f * a.time.max() + (n + 16) * EPS)
            assert (np.abs(p.real - ref.real) <= bound).all() and (np.abs(p.imag - ref.imag) <= bound).all()
        # f = 0: what is left is the tubes' own phase, a i^(-q): the same sum with every time's phase gone
        ref0 = _numpy_sum_from_arrivals(pr_any, fan, env, d, cols, 0.0, **kw)[0]
        p0 = pr_any.pressure_field(fan, d, env, 0.0, flatearth=False, **kw)[:, cols]
        tol = (np.diff(a.offsets).max() + 16) * EPS * amps if _lib.ARITH != "reference" else 0.0
        assert (np.abs(p0.real - ref0.real) <= tol).all() and (np.abs(p0.imag - ref0.imag) <= tol).all()
        assert (np.abs(p0) <= amps * (1 + 1e-12)).all() and (np.abs(p0) > 0).sum() > 50
        tl = pr_any.coherent_transmission_loss(fan, d, env, f, flatearth=False, **kw)[:, cols]
        with np.errstate(divide="ignore"):
            assert _same(tl, -20.0 * np.log10(np.abs(p)))
    _in_place(fan)


def test_focusing_medium_from_a_hip_fan(pr):
    pr_any = pr      # (the closed form holds on the oracle's bits: the reference arithmetic)
    env = cref.focus_env(pr_any)
    fan = pr_any.shoot_rays(cref.FOCUS_Z0, 0.0, cref.focus_angles(), cref.FOCUS_X1, cref.FOCUS_S, env, flatearth=False,
                            debug=False, device_resident=True)
    assert len(fan) == cref.FOCUS_N
    kappa = pr_any.caustic_index(fan)                                   # no bounces: neither a log nor the environment
    _in_place(fan)
    assert np.array_equal(kappa, pr_any.caustic_index(fan, env, flatearth=False))
    cref.check_focus_fan(np.asarray(fan.rs[0]), fan.zs, kappa, np.zeros(len(fan)), fan.n_botts, fan.n_surfs)
    host = fan.to_host()
    assert not host.device_resident and np.array_equal(pr_any.caustic_index(host), kappa)


def test_lloyds_mirror_end_to_end(pr):
    pr_any = pr      # (the bound is the oracle fan's: the reference arithmetic)
    env = cref.lloyd_env(pr_any)
    fan = pr_any.shoot_rays(cref.LLOYD_ZS, 0.0, cref.lloyd_angles(), cref.LLOYD_X1, cref.LLOYD_S, env, flatearth=False,
                            debug=False, device_resident=True, max_bounces=4)
    assert len(fan) == cref.LLOYD_N and (fan.n_botts == 0).all() and fan.n_surfs.max() == 1
    x = np.asarray(fan.rs[0])[cref.LLOYD_COLS]
    p = pr_any.pressure_field(fan, cref.LLOYD_DEPTHS, env, cref.LLOYD_F, flatearth=False)
    _in_place(fan)
    e = cref.lloyd_error(p[:, cref.LLOYD_COLS], x)
    j, k = np.unravel_index(np.argmax(e), e.shape)
    print(f"Lloyd's mirror from shoot_rays: worst e {e.max():.4e} at depth {cref.LLOYD_DEPTHS[j]} m, range {x[k]} m; "
          f"bound {cref.LLOYD_BOUND:.4e}")
    assert e.max() <= cref.LLOYD_BOUND < 0.05
    host = pr_any.pressure_field(fan.to_host(), cref.LLOYD_DEPTHS, env, cref.LLOYD_F, flatearth=False)
    assert _same(host.real, p.real) and _same(host.imag, p.imag)


def test_identities_hold_in_contracted_arithmetic():
    from pygenray_amd import _lib
    if _lib.ARITH != "reference":
        pytest.skip("this IS the contracted process")
    if not os.path.exists(_lib.CONTRACTED_LIB):
        pytest.fail("libpgr_hip_fma.so is not built (__graft_entry__.build() builds it beside the product)")
    out = subprocess.run([sys.executable, "-m", "pytest", "-q", "-m", "gpu", "-x", "-p", "no:cacheprovider", "-k", "identity",
                          os.path.join(ROOT, "tests", "test_coherent.py")],
                         cwd=ROOT, env=dict(os.environ, PGR_ARITH="contracted"), capture_output=True, text=True, timeout=600)
    tail = out.stdout[-3000:] + out.stderr[-1500:]
    assert out.returncode == 0 and " passed" in out.stdout and "failed" not in out.stdout, tail


# ---- the error paths of the C entries ----------------------------------------------------------------------------------------

def test_c_entries_refuse_bad_arguments_before_writing_anything(pr_any, syn_env):
    import torch
    from pygenray_amd import _lib
    env, cin = syn_env
    L = _lib.load()
    M, S, R = 70, 6, 9
    z, p, x, p0, depths = synthetic_fan(M, S, R, seed=4, cin=cin)
    t, W, q = synthetic_phase(M, S, 1)
    d, stream = _upload(env, t, z, p, x, p0, depths)
    dev = d[0].device
    vp = ctypes.c_void_p
    kappa = torch.full((S * M,), -7, dtype=torch.int32, device=dev)
    for args, msg in (((None, M, S, kappa.data_ptr()), "null"), ((d[1].data_ptr(), M, S, None), "null"),
                      ((d[1].data_ptr(), 1, S, kappa.data_ptr()), "at least two rays"),
                      ((d[1].data_ptr(), M, 0, kappa.data_ptr()), "n_samples")):
        rc = L.pgr_caustic_index_device(0, args[0], args[1], args[2], None, None, args[3], vp(stream))
        err = L.pgr_last_error().decode()
        assert rc < 0 and "pgr_caustic_index_device" in err and msg in err, (args, rc, err)
    assert (kappa.cpu().numpy() == -7).all()
    re, im = (torch.full((R * S,), MARK, dtype=torch.float64, device=dev) for _ in range(2))

    def call(f=50.0, n_rays=M, re_=re, im_=im):
        _lib.pressure_device(env, d[0].data_ptr(), d[1].data_ptr(), d[2].data_ptr(), n_rays, S, d[3].data_ptr(),
                             d[4].data_ptr(), 0, f, d[5].data_ptr(), R, 0 if re_ is None else re_.data_ptr(),
                             0 if im_ is None else im_.data_ptr(), stream)
    for kw, msg in ((dict(f=-1.0), "frequency"), (dict(f=np.nan), "frequency"), (dict(f=np.inf), "frequency"),
                    (dict(n_rays=1), "at least two rays"), (dict(re_=None), "null"), (dict(im_=None), "null")):
        with pytest.raises(_lib.PgrError, match="pgr_pressure_device_w.*" + msg):
            call(**kw)
    assert (re.cpu().numpy() == MARK).all() and (im.cpu().numpy() == MARK).all()
    call()                                                               # and the same buffers with good arguments: written
    assert not (re.cpu().numpy() == MARK).any() and not (im.cpu().numpy() == MARK).any()
    # the fan entries: the same checks, by name; a fan without trajectories is refused
    fan = _shoot(pr_any, munk_env(pr_any), True, log=False, n=70, S=6, x1=20e3)
    with pytest.raises(_lib.PgrError, match="pgr_fan_caustic_index.*null"):
        fan._dev.caustic_index(0, 0, 0, stream)
    with pytest.raises(_lib.PgrError, match="pgr_fan_pressure_w.*frequency"):
        fan._dev.pressure(d[4].data_ptr(), 0, -2.0, d[5].data_ptr(), R, re.data_ptr(), im.data_ptr(), stream)
