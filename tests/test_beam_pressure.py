"""beam_pressure_field on the GPU (csrc/pgr_beam_phase.h): pgr_beam_pressure_device_w bit for bit against the restatement of
tests/beam_pressure_reference.py on synthetic buffers aimed at the kernel's chunk, halo, band and 4-sigma seams, the refusals
of both C entries, Munk fans in every layout and on either side of the bus, absorption and boundary loss, and Lloyd's mirror
and the waveguide from ``shoot_rays`` within the bounds tests/test_beam_pressure_host.py measured."""
import numpy as np
import pytest

import beam_pressure_reference as bp
import beam_reference as bref
import coherent_reference as cref
import path_reference as pref
import wave_reference as wref
from tube_gpu import (DEPTHS, SYN_R, SYN_Z, _same, _upload, munk_env, pr, pr_any, sloping_env,  # noqa: F401
                      sloping_env_shallow_table, syn_env, synthetic_fan)

pytestmark = pytest.mark.gpu

PAD = 130                    # entries either side of an output that must stay as they were
MARK = -7.25
FAN_PROFILE = ([0.0, 300.0, 1200.0, 4000.0], [0.9, 0.5, 0.08, 0.2])          # dB/km, as the public functions take it


def _device_beam_pressure(env, t, z, p, x, p0, bottom, depths, w_min, W, q, f, curvature):
    """_lib.beam_pressure_device on [S][M] rows -> re, im (R, S); sentinels before and behind both outputs checked untouched"""
    import torch
    from pygenray_amd import _lib
    d, stream = _upload(env, t, z, p, x, p0, bottom, depths, *(() if W is None else (W,)))
    dev = d[0].device
    S, M = z.shape
    R = len(depths)
    dq = None if q is None else torch.from_numpy(np.ascontiguousarray(q, dtype=np.int32)).to(dev)
    out = [torch.full((PAD + R * S + PAD,), MARK, dtype=torch.float64, device=dev) for _ in range(2)]
    _lib.beam_pressure_device(env, d[0].data_ptr(), d[1].data_ptr(), d[2].data_ptr(), M, S, d[3].data_ptr(), d[4].data_ptr(),
                              0 if dq is None else dq.data_ptr(), f, d[5].data_ptr(), d[6].data_ptr(), R, w_min, curvature,
                              out[0][PAD:].data_ptr(), out[1][PAD:].data_ptr(), stream,
                              weights=0 if W is None else d[7].data_ptr())
    h = [a.cpu().numpy() for a in out]
    assert all((a[:PAD] == MARK).all() and (a[PAD + R * S:] == MARK).all() for a in h)
    return tuple(a[PAD:PAD + R * S].reshape(R, S) for a in h)


def synthetic_phase(M, S, seed):
    """travel times t (S, M) with one NaN, weights W (S, M) in (0, 1] with exact ones, zeros and two NaNs, and q (S, M) int32
    in -1 ... 9"""
    rng = np.random.default_rng(seed)
    t = np.cumsum(rng.uniform(0.2, 1.5, (S, M)), axis=0)
    W = 10.0 ** rng.uniform(-6.0, 0.0, (S, M))
    W[rng.random((S, M)) < 0.05] = 1.0
    W[rng.random((S, M)) < 0.02] = 0.0
    if M >= 8:
        W[S - 1, M // 6] = W[0, M - 2] = np.nan
        t[S - 1, M // 7] = np.nan                                         # NaN in T alone
    q = rng.integers(-1, 10, (S, M)).astype(np.int32)
    return t, W, q


def _check(env, cin, t, z, p, x, p0, bottom, depths, w_min, W, q, f, curvature):
    re, im = _device_beam_pressure(env, t, z, p, x, p0, bottom, depths, w_min, W, q, f, curvature)
    ref = bp.beam_pressure(z.T, p.T, t.T, x, p0, depths, cin, SYN_R, SYN_Z, bottom, w_min, None if W is None else W.T,
                           None if q is None else q.T, f, curvature)
    bad = ~((re == ref[0]) | (np.isnan(re) & np.isnan(ref[0]))) | ~((im == ref[1]) | (np.isnan(im) & np.isnan(ref[1])))
    assert not bad.any(), (np.argwhere(bad)[:5], re[bad][:5], ref[0][bad][:5], im[bad][:5], ref[1][bad][:5])
    assert np.isnan(re[:, x == x[0]]).all() and np.isnan(im[:, x == x[0]]).all()
    return re, im


# ---- the kernel on synthetic inputs: pgr_beam_pressure_device_w against the restatement, bit for bit ---------------------------
#
# A chunk is 61 tubes (lane t loads ray 61 c - 1 + t): the ray counts make the last chunk full or hold one / two tubes and give
# 65 chunks (M = 3906: two ballot rounds); the receiver counts make the last band hold 1 / 63 / 64 receivers.  Every case runs
# one combination of (weights, q, curvature, f) picked from its index, so that each value of each meets every M, R and S.

SEAM_M = (2, 3, 60, 61, 62, 63, 64, 122, 123, 124, 3906)
SEAM_R = (1, 63, 64, 65, 129)
SEAM_S = (1, 2, 5)
SEAM_CASES = [(M, R, S) for M in SEAM_M for R in SEAM_R for S in SEAM_S]


@pytest.mark.parametrize("M, R, S", SEAM_CASES, ids=[f"M{M}-R{R}-S{S}" for M, R, S in SEAM_CASES])
def test_kernel_bit_identical_on_the_seam_shapes(pr, syn_env, M, R, S):
    env, cin = syn_env
    i = SEAM_CASES.index((M, R, S))
    z, p, x, p0, depths = synthetic_fan(M, S, R, seed=M * 1013 + S * 37 + R, cin=cin)
    t, W, q = synthetic_phase(M, S, M + 7 * S + R)
    bottom = np.linspace(4700.0, 5150.0, S)                  # a sloping bottom, crossed by the fan's samples
    f = (0.0, 50.0, 1e4)[i % 3]
    curvature = (i // 3) % 2
    w = W if (i // 6 + i) % 2 else None
    qq = (None, q, np.where(q > 3, -1, q), q + 4 * (q >= 0))[(i // 2 + i // 15) % 4]     # NULL, with -1 and above 3, ...
    w_min = (40.0, 0.5)[(i // 5) % 2]
    re, im = _check(env, cin, t, z, p, x, p0, bottom, depths, w_min, w, qq, f, curvature)
    again = _device_beam_pressure(env, t, z, p, x, p0, bottom, depths, w_min, w, qq, f, curvature)
    assert _same(again[0], re) and _same(again[1], im)                              # two calls are bit-equal
    if f == 0.0 and qq is None and M < 8:                                           # (no NaN T: every term's phase is its q's)
        assert (np.nan_to_num(im) == 0).all()


def test_every_variant_on_one_shape(pr, syn_env):
    """weights x q x curvature x f on one fan with every adds-nothing branch (NaN z, p, T alone, |p c| = 1, D = 0)"""
    env, cin = syn_env
    M, S, R = 200, 5, 70
    z, p, x, p0, depths = synthetic_fan(M, S, R, seed=77, cin=cin)
    t, W, q = synthetic_phase(M, S, 78)
    bottom = np.linspace(4700.0, 5150.0, S)
    got = {}
    for wname, w in (("w", W), ("-", None)):
        for qname, qq in (("null", None), ("q", q), ("q+4", np.where(q >= 0, q + 4, q))):
            for curvature in (0, 1):
                for f in (0.0, 50.0, 1e4):
                    got[(wname, qname, curvature, f)] = _check(env, cin, t, z, p, x, p0, bottom, depths, 25.0, w, qq, f, curvature)
    lit = x != x[0]
    assert (np.nan_to_num(got[("-", "null", 1, 50.0)][0][:, lit]) != 0).mean() > 0.5
    for key, val in got.items():
        if key[1] == "q+4":                                                         # whole cycles change nothing
            assert _same(val[0], got[(key[0], "q", key[2], key[3])][0]) and _same(val[1], got[(key[0], "q", key[2], key[3])][1])
    assert not _same(got[("-", "q", 1, 50.0)][0], got[("-", "q", 0, 50.0)][0])      # the curvature term is there
    assert not _same(got[("w", "q", 1, 50.0)][0], got[("-", "q", 1, 50.0)][0])
    gone = _device_beam_pressure(env, t, z, p, x, p0, bottom, depths, 25.0, None, np.full((S, M), -1, np.int32), 50.0, 1)
    assert (gone[0][:, lit] == 0).all() and (gone[1][:, lit] == 0).all()


def test_receivers_on_the_four_sigma_edges(pr, syn_env):
    # receivers at centre -+ 4 sigma and one ulp either side, for the beam and both its images: each term the definition keeps
    # must be kept and each it drops dropped, whatever the chunk test decided
    env, cin = syn_env
    M, S = 400, 4
    z, p, x, p0, depths = synthetic_fan(M, S, 64, seed=11, cin=cin)
    t, W, q = synthetic_phase(M, S, 12)
    bottom = np.array([4900.0, 4950.0, 5000.0, 5050.0])
    w_min = 25.0
    valid, m, sigma, _, _, r = bref._tubes(z.T, p.T, x, p0, cin, SYN_R, SYN_Z, w_min)
    edge = []
    assert x[2] == x[0]                                               # (column 2 is the source's: NaN)
    for s in (1, 3):
        k = np.flatnonzero(valid[:, s])
        near_top = k[np.argsort(np.abs(m[k, s]))[:6]]                  # beams that reach the surface
        near_bot = k[np.argsort(np.abs(m[k, s] - bottom[s]))[:6]]      # ... and the bottom
        for kk in np.concatenate([k[::37], near_top, near_bot]):
            for ctr in (m[kk, s], -m[kk, s], 2.0 * bottom[s] - m[kk, s]):
                for e in (ctr - 4 * sigma[kk, s], ctr + 4 * sigma[kk, s]):
                    edge += [np.nextafter(e, -np.inf), e, np.nextafter(e, np.inf)]
    depths = np.unique(np.concatenate([depths, edge]))
    assert len(depths) > 500 and depths.min() < 0 and depths.max() > bottom.max()
    for curvature in (0, 1):
        re, im = _check(env, cin, t, z, p, x, p0, bottom, depths, w_min, None, np.where(q > 5, -1, q), 50.0, curvature)
    assert (np.hypot(re, im)[:, [1, 3]] > 0).mean() > 0.3


# ---- refusals, with nothing written -------------------------------------------------------------------------------------------

def test_c_entries_refuse_bad_arguments_before_writing_anything(pr_any, syn_env):
    import torch
    from pygenray_amd import _lib
    env, cin = syn_env
    M, S, R = 70, 6, 9
    z, p, x, p0, depths = synthetic_fan(M, S, R, seed=4, cin=cin)
    t, W, q = synthetic_phase(M, S, 1)
    d, stream = _upload(env, t, z, p, x, p0, np.full(S, 5000.0), depths)
    dev = d[0].device
    re, im = (torch.full((R * S,), MARK, dtype=torch.float64, device=dev) for _ in range(2))

    def call(f=50.0, w=10.0, n_rays=M, re_=re, im_=im, bottom=d[5]):
        _lib.beam_pressure_device(env, d[0].data_ptr(), d[1].data_ptr(), d[2].data_ptr(), n_rays, S, d[3].data_ptr(),
                                  d[4].data_ptr(), 0, f, 0 if bottom is None else bottom.data_ptr(), d[6].data_ptr(), R, w, 1,
                                  0 if re_ is None else re_.data_ptr(), 0 if im_ is None else im_.data_ptr(), stream)
    for kw, msg in ((dict(f=-1.0), "frequency"), (dict(f=np.nan), "frequency"), (dict(f=np.inf), "frequency"),
                    (dict(w=0.0), "min_width"), (dict(w=-1.0), "min_width"), (dict(w=np.nan), "min_width"),
                    (dict(w=np.inf), "min_width"), (dict(n_rays=1), "at least two rays"), (dict(re_=None), "null"),
                    (dict(im_=None), "null"), (dict(bottom=None), "null")):
        with pytest.raises(_lib.PgrError, match="pgr_beam_pressure_device_w.*" + msg):
            call(**kw)
    assert (re.cpu().numpy() == MARK).all() and (im.cpu().numpy() == MARK).all()
    call()                                                               # and the same buffers with good arguments: written
    assert not (re.cpu().numpy() == MARK).any() and not (im.cpu().numpy() == MARK).any()
    # the fan entry: the same checks, by name
    fan = pr_any.shoot_rays(1000.0, 0.0, np.linspace(-20.0, 20.0, M), 20e3, S, munk_env(pr_any), flatearth=False, debug=False,
                            device_resident=True)
    re.fill_(MARK)
    im.fill_(MARK)
    for f, w, msg in ((-2.0, 10.0, "frequency"), (np.nan, 10.0, "frequency"), (50.0, 0.0, "min_width"), (50.0, np.inf, "min_width")):
        with pytest.raises(_lib.PgrError, match="pgr_fan_beam_pressure_w.*" + msg):
            fan._dev.beam_pressure(d[4].data_ptr(), 0, f, d[5].data_ptr(), d[6].data_ptr(), R, w, 1, re.data_ptr(), im.data_ptr(),
                                   stream)
    one = pr_any.shoot_rays(1000.0, 0.0, np.array([1.0]), 20e3, S, munk_env(pr_any), flatearth=False, debug=False,
                            device_resident=True)
    with pytest.raises(_lib.PgrError, match="pgr_fan_beam_pressure_w.*at least two rays"):
        one._dev.beam_pressure(d[4].data_ptr(), 0, 50.0, d[5].data_ptr(), d[6].data_ptr(), R, 10.0, 1, re.data_ptr(),
                               im.data_ptr(), stream)
    assert (re.cpu().numpy() == MARK).all() and (im.cpu().numpy() == MARK).all() and fan.device_resident


# ---- fans ---------------------------------------------------------------------------------------------------------------------

FAN_N, FAN_S, FAN_COLS = 2001, 41, [40, 17, 1]


def _shoot(pr, env, resident, n=FAN_N, S=FAN_S, x1=80e3):
    return pr.shoot_rays(1000.0, 0.0, np.linspace(-20.0, 20.0, n), x1, S, env, flatearth=False, debug=False,
                         device_resident=resident, max_bounces=64)


def _in_place(fan):
    assert fan.device_resident and not any(k in fan.__dict__ for k in ("_ts", "_zs", "_ps"))


@pytest.mark.parametrize("which", ["munk", "sloping", "munk-dropped", "sloping-dropped"])
def test_munk_fans_in_every_layout_give_one_answer(pr, which):
    """rows (munk) and sample-blocked (sloping) fans of 2001 rays, with dropped rays skipped through the keep list: the
    device-resident fan and the same fan on the host against the restatement on the fetched fan, with and without the
    curvature term, with absorption and a loss pair"""
    env = {"munk": munk_env, "sloping": sloping_env, "munk-dropped": lambda p: munk_env(p, ztop=4200.0),
           "sloping-dropped": sloping_env_shallow_table}[which](pr)
    fan, eager = _shoot(pr, env, True), _shoot(pr, env, False)
    assert fan._dev._env.blocked_layout == which.startswith("sloping")
    # (the Munk fan loses one ray of its 2001 as it is; the shallow tables lose the deep ones)
    assert (FAN_N - len(eager) > 20) == which.endswith("dropped") and len(eager) > 300 and fan._dev.N == FAN_N
    assert len(fan) == len(eager)
    nb, ns = eager.bounce_counts(np.arange(FAN_S))
    d = DEPTHS[::20]
    loss = ([5.0, 30.0, 60.0], [0.5, 2.0, 6.0])
    # the weights of absorption and a loss pair: 10^(-(A + B) / 10), A restated, B the bounce post-pass's own (test_bounce_log.py)
    B = pr.boundary_loss(eager, env, bottom_loss=loss, surface_loss=0.5, flatearth=False)
    W = pref.weights(pref.fan_path_integral(eager, env, FAN_PROFILE, False) + B)
    for w, curvature, kw in ((None, True, {}), (None, False, {}),
                             (W, True, dict(absorption=FAN_PROFILE, bottom_loss=loss, surface_loss=0.5))):
        ref = bp.fan_beam_pressure(eager, d, env, 25.0, w_min=15.0, curvature=curvature, flatearth=False, W=w, nb=nb, ns=ns,
                                   cols=FAN_COLS)
        p = pr.beam_pressure_field(fan, d, env, 25.0, min_width=15.0, curvature=curvature, flatearth=False, **kw)
        assert p.shape == (len(d), FAN_S) and p.dtype == np.complex128
        assert _same(p.real[:, FAN_COLS], ref.real) and _same(p.imag[:, FAN_COLS], ref.imag)
        assert np.isnan(p[:, 0]).all() and np.isfinite(p[:, 1:]).all() and (np.abs(p[:, 1:]) > 0).mean() > 0.2
        host = pr.beam_pressure_field(eager, d, env, 25.0, min_width=15.0, curvature=curvature, flatearth=False, **kw)
        assert _same(host.real, p.real) and _same(host.imag, p.imag)                 # device and host paths: one answer
    tl = pr.coherent_beam_transmission_loss(fan, d, env, 25.0, min_width=15.0, flatearth=False)
    with np.errstate(divide="ignore"):
        assert _same(tl, -20.0 * np.log10(np.abs(pr.beam_pressure_field(fan, d, env, 25.0, min_width=15.0, flatearth=False))))
    _in_place(fan)
    if which == "munk":
        # informative: the largest |p| of the tube sum and of the beam sum over the same grid
        tube = pr.pressure_field(fan, d, env, 25.0, flatearth=False)
        print(f"Munk fan, {len(d)} x {FAN_S - 1} cells at 25 Hz: max |p| {np.abs(tube[:, 1:]).max():.4e} from pressure_field, "
              f"{np.abs(p[:, 1:]).max():.4e} from beam_pressure_field (min_width 15 m)")
        assert np.isfinite(tube[:, 1:]).all()


def test_a_bottom_reflection_is_refused_and_its_loss_pair_is_taken(pr):
    env = munk_env(pr)
    fan = _shoot(pr, env, True, n=301, S=21, x1=40e3)
    b = pr.fluid_halfspace(1700.0, 1800.0, 0.5)
    with pytest.raises(ValueError, match="does not yet apply a complex bottom phase"):
        pr.beam_pressure_field(fan, [100.0, 2000.0], env, 25.0, flatearth=False, bottom_loss=b)
    a = pr.beam_pressure_field(fan, [100.0, 2000.0], env, 25.0, flatearth=False, bottom_loss=b.loss)
    assert np.isfinite(a[:, 1:]).all() and (np.abs(a[:, 1:]) > 0).any()
    _in_place(fan)


# ---- physics on HIP fans ------------------------------------------------------------------------------------------------------

def test_lloyds_mirror_from_shoot_rays(pr):
    env = cref.lloyd_env(pr)
    fan = pr.shoot_rays(bp.LLOYD_ZS, 0.0, np.linspace(-bp.EXACT_APERTURE, bp.EXACT_APERTURE, bp.EXACT_N), 5e3, 51, env,
                        flatearth=False, debug=False, device_resident=True, max_bounces=4)
    assert len(fan) == bp.EXACT_N and (fan.n_botts == 0).all() and fan.n_surfs.max() == 1
    cols = np.array([20, 30, 40, 50])
    x = np.asarray(fan.rs[0])[cols]
    assert np.array_equal(x, bp.EXACT_RANGES)
    worst = {}
    for curvature in (True, False):
        p = pr.beam_pressure_field(fan, bp.LLOYD_DEPTHS, env, bp.EXACT_F, min_width=10.0, curvature=curvature, flatearth=False)
        worst[curvature] = bp.lloyd_error(p[:, cols]).max(axis=0)
    _in_place(fan)
    print(f"Lloyd's mirror from shoot_rays, min_width 10 m: worst e per range {[f'{v:.4e}' for v in worst[True]]} with the "
          f"curvature term, {[f'{v:.4e}' for v in worst[False]]} without; bounds {2.0 * bp.LLOYD_MEASURED[10.0]:.4e}, "
          f"{2.0 * bp.LLOYD_MEASURED_LINEAR[10.0]:.4e}")
    assert worst[True].max() <= 2.0 * bp.LLOYD_MEASURED[10.0]
    assert worst[False].max() <= 2.0 * bp.LLOYD_MEASURED_LINEAR[10.0]
    assert (worst[False] >= 10.0 * worst[True]).all()


def test_waveguide_from_shoot_rays(pr):
    env = wref.guide_env(pr)
    fan = pr.shoot_rays(wref.GUIDE_ZS, 0.0, wref.guide_angles(), wref.GUIDE_X1, wref.GUIDE_S, env, flatearth=False, debug=False,
                        device_resident=True, max_bounces=wref.GUIDE_K)
    assert len(fan) == wref.GUIDE_N and fan.n_botts.max() == 2 and fan.n_surfs.max() == 2
    x = np.asarray(fan.rs[0])[wref.GUIDE_COLS]
    keep = wref.check_guide_cells(x)
    p = pr.beam_pressure_field(fan, wref.GUIDE_DEPTHS, env, wref.GUIDE_F, min_width=10.0, flatearth=False)[:, wref.GUIDE_COLS]
    _in_place(fan)
    R, sign, inside, _ = wref.guide_images(x)
    e = np.abs(p - wref.waveguide_field(wref.GUIDE_F, wref.GUIDE_DEPTHS, x)) / wref._norm(R, inside)
    print(f"waveguide from shoot_rays, beams: worst e {e[keep].max():.4e} on the cells kept (bound {2.0 * bp.GUIDE_BEAM_MEASURED:.4e}), "
          f"{e[~keep].max():.4e} on the cells dropped")
    assert e[keep].max() <= 2.0 * bp.GUIDE_BEAM_MEASURED
    assert np.isfinite(e).all()
