"""Complex bottom reflection on the GPU (csrc/pgr_reflect.h, csrc/pgr_spectrum.h): the three sums with a lag per arrival alone
through ``_lib.pressure_phi_device`` / ``signal_phi_device`` / ``spectrum_phi_device`` against the restatement of
tests/reflection_reference.py at their siblings' seam shapes, against the siblings themselves with a lag of zero, the error paths
of the C entries, a ``BottomReflection`` through every coherent product of a Munk fan, fans in both trajectory layouts (dropped
rays, host fans), and the waveguide over a fluid half-space from ``shoot_rays`` against the ray-theoretic image sum."""
import ctypes

import numpy as np
import pytest

import reflection_reference as rref
import signal_reference as sref
import spectrum_reference as spref
import wave_reference as wref
from tube_gpu import (DEPTHS, SYN_R, SYN_Z, _same, _upload, munk_env, pr, pr_any, sloping_env,  # noqa: F401
                      sloping_env_shallow_table, syn_env, synthetic_fan)

pytestmark = pytest.mark.gpu

PAD = 130                    # entries behind an output that must stay as they were
MARK = -7.25


def _bits(a, b):
    return _same(a.real, b.real) and _same(a.imag, b.imag)


# ---- the tube sum alone -------------------------------------------------------------------------------------------------------

def _device_pressure(env, t, z, p, x, p0, depths, W, q, phi, f):
    """_lib.pressure_phi_device (phi None: its sibling _lib.pressure_device) on [S][M] rows -> re + i im (R, S); sentinels behind
    both outputs checked untouched"""
    import torch
    from pygenray_amd import _lib
    d, stream = _upload(env, t, z, p, x, p0, depths, *(() if W is None else (W,)))
    dev = d[0].device
    S, M = z.shape
    R = len(depths)
    dq = None if q is None else torch.from_numpy(np.ascontiguousarray(q, dtype=np.int32)).to(dev)
    out = [torch.full((R * S + PAD,), MARK, dtype=torch.float64, device=dev) for _ in range(2)]
    head = (env, d[0].data_ptr(), d[1].data_ptr(), d[2].data_ptr(), M, S, d[3].data_ptr(), d[4].data_ptr(),
            0 if dq is None else dq.data_ptr())
    tail = (f, d[5].data_ptr(), R, out[0].data_ptr(), out[1].data_ptr(), stream)
    kw = dict(weights=0 if W is None else d[6].data_ptr())
    if phi is None:
        _lib.pressure_device(*head, *tail, **kw)
    else:
        dphi = torch.from_numpy(np.ascontiguousarray(phi, dtype=np.float64)).to(dev)
        _lib.pressure_phi_device(*head, dphi.data_ptr(), *tail, **kw)
    h = [a.cpu().numpy() for a in out]
    assert all((a[R * S:] == MARK).all() for a in h) and not any((a[:R * S] == MARK).any() for a in h)
    return (h[0][:R * S] + 1j * h[1][:R * S]).reshape(R, S)


def synthetic_phase(M, S, seed):
    """travel times t (S, M), weights W (S, M) in (0, 1] with exact ones and zeros, q (S, M) int32 in -1 ... 9 and the rays'
    lags phi (S, M): reflection_reference.synthetic_lags (0.0, negative values, values beyond +-1e3 cycles, one NaN)"""
    rng = np.random.default_rng(seed)
    t = np.cumsum(rng.uniform(0.2, 1.5, (S, M)), axis=0)
    W = 10.0 ** rng.uniform(-6.0, 0.0, (S, M))
    W[rng.random((S, M)) < 0.05] = 1.0
    W[rng.random((S, M)) < 0.02] = 0.0
    q = rng.integers(-1, 10, (S, M)).astype(np.int32)
    return t, W, q, rref.synthetic_lags((S, M), seed + 1)


TUBE_CASES = [(M, S, R) for M in (2, 3, 63, 64, 65, 127, 128, 4035) for R in (1, 63, 64, 65, 129) for S in (1, 2, 5)]


@pytest.mark.parametrize("M, S, R", TUBE_CASES, ids=[f"M{M}-S{S}-R{R}" for M, S, R in TUBE_CASES])
def test_tube_sum_bit_identical_to_the_restatement_and_to_its_sibling_at_zero_lag(pr, syn_env, M, S, R):
    env, cin = syn_env
    z, p, x, p0, depths = synthetic_fan(M, S, R, seed=M * 1009 + S * 31 + R, cin=cin)
    t, W, q, phi = synthetic_phase(M, S, M + 7 * S + R)
    f = 37.5
    assert (phi < 0).any() and np.abs(phi[np.isfinite(phi)]).max() > 1e3 and (phi.size < 3 or (phi == 0).any())
    assert np.isnan(phi).sum() == (phi.size >= 16)
    variants = dict(both=(W, q), none=(None, None))
    if M > 1000:                                                        # (the restatement takes 2 s per call there)
        variants = dict(both=(W, q))
    got = {}
    for name, (w, qq) in variants.items():
        u = got[name] = _device_pressure(env, t, z, p, x, p0, depths, w, qq, phi, f)
        ref = rref.tube_pressure(z.T, p.T, t.T, x, p0, depths, cin, SYN_R, SYN_Z, None if w is None else w.T,
                                 None if qq is None else qq.T, f, phi.T)
        bad = np.argwhere(~((u.real == ref[0]) | (np.isnan(u.real) & np.isnan(ref[0]))))
        assert _same(u.real, ref[0]) and _same(u.imag, ref[1]), (name, bad[:5])
        assert np.isnan(u.real[:, x == x[0]]).all() and _same(np.isnan(u.real), np.isnan(u.imag))
        # a lag of zero, and of whole cycles: the sibling's bits
        sibling = _device_pressure(env, t, z, p, x, p0, depths, w, qq, None, f)
        assert _bits(_device_pressure(env, t, z, p, x, p0, depths, w, qq, np.zeros((S, M)), f), sibling), name
        for whole in (3.0, -2.0):                                       # (the same on every ray: an arrival's lag is interpolated)
            assert _bits(_device_pressure(env, t, z, p, x, p0, depths, w, qq, np.full((S, M), whole), f), sibling), (name, whole)
        if M >= 63 and S >= 2 and R >= 63:
            assert not _bits(u, sibling)                                # the lag matters
    again = _device_pressure(env, t, z, p, x, p0, depths, W, q, phi, f)   # repeated calls are bit-equal
    assert _bits(again, got["both"])


# ---- the arrival sums alone ---------------------------------------------------------------------------------------------------

COUNTS = [200, 0, 65, 1, 63, 64]             # the staging seams: groups of every one of these in one call (G = 130)
N_CASES = [1, 63, 64, 65, 255, 256, 257]     # samples / frequencies: the lanes' and the tile's seams (4 rows of 64)


def synthetic_groups(G, n_axis, dt, seed):
    """groups with COUNTS arrivals (then random counts up to 130): T around each group's time axis tstart + [0, (n_axis - 1) dt]
    (before, on both ends, inside, behind), I over six decades with exact zeros and one NaN, q in -1 ... 9, the arrivals' lags
    (reflection_reference.synthetic_lags), path lengths L, a reduction time per group"""
    rng = np.random.default_rng(seed)
    cnt = np.array([COUNTS[g] if g < len(COUNTS) else int(rng.integers(0, 131)) for g in range(G)])
    off = np.concatenate([[0], np.cumsum(cnt)]).astype(np.int64)
    n = int(off[-1])
    tstart = 60.0 + rng.uniform(-3.0, 3.0, G)
    span = (n_axis - 1) * dt
    grp = np.repeat(np.arange(G), cnt)
    T = tstart[grp] + rng.uniform(-0.06, span + 0.06, n)
    edge = rng.random(n)
    T = np.where(edge < 0.08, tstart[grp] + rng.uniform(-0.004, 0.004, n), T)
    T = np.where(edge > 0.92, tstart[grp] + span + rng.uniform(-0.004, 0.004, n), T)
    T = T[np.lexsort((T, grp))]
    I = 10.0 ** rng.uniform(-12.0, -6.0, n)
    I[rng.random(n) < 0.05] = 0.0
    if n > 20:
        I[n // 3] = np.nan
    q = rng.integers(-1, 10, n).astype(np.int32)
    q[[5, 6]] = [-1, 7]
    phi = rref.synthetic_lags(n, seed + 1)
    L = rng.uniform(1e4, 1.2e6, n)
    L[7] = 1e10
    return off, T, I, q, phi, L, tstart


def _device_arrival_sum(which, off, T, I, q, phi, n_out, call):
    """one of the two arrival sums on host arrays -> (G, n_out) complex: `call(lib_function, head, phi_pointer_or_None, tail)`
    builds the entry's own middle arguments; sentinels behind both outputs checked untouched, every entry before them written"""
    import torch
    from pygenray_amd import _lib
    dev = torch.device("cuda", 0)
    G = len(off) - 1
    up = lambda a, dt_: torch.from_numpy(np.ascontiguousarray(a, dtype=dt_)).to(dev)   # noqa: E731
    d_off, d_T, d_I = up(off, np.int64), up(np.append(T, 0.0), float), up(np.append(I, 0.0), float)
    d_q = None if q is None else up(np.append(q, 0), np.int32)
    d_phi = None if phi is None else up(np.append(phi, 0.0), float)
    out = [torch.full((G * n_out + PAD,), MARK, dtype=torch.float64, device=dev) for _ in range(2)]
    head = (0, d_off.data_ptr(), G, d_T.data_ptr(), d_I.data_ptr(), 0 if d_q is None else d_q.data_ptr())
    tail = (out[0].data_ptr(), out[1].data_ptr(), torch.cuda.current_stream(dev).cuda_stream)
    fn = getattr(_lib, which + ("_device" if phi is None else "_phi_device"))
    keep = call(fn, head + (() if phi is None else (d_phi.data_ptr(),)), tail, up)
    h = [a.cpu().numpy() for a in out]
    del keep
    assert all((a[G * n_out:] == MARK).all() for a in h) and not any((a[:G * n_out] == MARK).any() for a in h)
    return (h[0][:G * n_out] + 1j * h[1][:G * n_out]).reshape(G, n_out)


def _device_signal(off, T, I, q, phi, tstart, f, rs, dt, nt):
    def call(fn, head, tail, up):
        d_ts = up(tstart, float)
        fn(*head, d_ts.data_ptr(), f, rs, dt, nt, *tail)
        return d_ts
    return _device_arrival_sum("signal", off, T, I, q, phi, nt, call)


def _device_spectrum(off, T, I, q, phi, L, tred, freq, alpha):
    def call(fn, head, tail, up):
        d_tr = up(tred, float)
        d_L = None if L is None else up(np.append(L, 0.0), float)
        fn(*head, 0 if d_L is None else d_L.data_ptr(), d_tr.data_ptr(), freq, alpha, *tail)
        return d_tr, d_L
    return _device_arrival_sum("spectrum", off, T, I, q, phi, len(freq), call)


@pytest.mark.parametrize("nt", N_CASES)
@pytest.mark.parametrize("G", [1, 3, 130])
def test_signal_sum_bit_identical_to_the_restatement_and_to_its_sibling_at_zero_lag(pr, G, nt):
    dt, f = 1e-3, 75.0
    off, T, I, q, phi, _, tstart = synthetic_groups(G, nt, dt, seed=1000 * G + nt)
    n = len(T)
    assert G < 130 or set(COUNTS) <= set(np.diff(off).tolist())
    assert (q < 0).any() and (q > 3).any() and (phi == 0).any() and (phi < 0).any() and np.nanmax(np.abs(phi)) > 1e3
    assert np.isnan(phi).sum() == 1 and (I == 0).any()
    for rs in (0.0, 200.0):                                            # CW, and sigma = 5 ms: windows of 80 samples
        got = {}
        for name, qq in (("q", q), ("null", None)):
            u = got[name] = _device_signal(off, T, I, qq, phi, tstart, f, rs, dt, nt)
            ref = rref.signal_sum(off, T, I, qq, phi, tstart, f, rs, dt, nt)
            bad = np.argwhere(~((u.real == ref.real) | (np.isnan(u.real) & np.isnan(ref.real))))
            assert _bits(u, ref), (rs, name, bad[:5])
            sibling = _device_signal(off, T, I, qq, None, tstart, f, rs, dt, nt)
            assert _bits(_device_signal(off, T, I, qq, np.zeros(n), tstart, f, rs, dt, nt), sibling), (rs, name)
            assert _bits(_device_signal(off, T, I, qq, np.where(np.arange(n) % 2, 3.0, -2.0), tstart, f, rs, dt, nt), sibling)
            assert G < 130 or not _bits(u, sibling)
        assert _bits(_device_signal(off, T, I, q, phi, tstart, f, rs, dt, nt), got["q"])     # repeated calls are bit-equal
        empty = np.flatnonzero(np.diff(off) == 0)
        assert all((got[name][empty] == 0).all() for name in got)      # empty groups are written: zeros
    # rs = 0: every sample of a group is the group's CW sum with the lags
    cw = _device_signal(off, T, I, q, phi, tstart, f, 0.0, dt, nt)
    ref = rref.cw_sum(off, T, I, q, phi, f)
    assert all(_bits(cw[:, m], ref) for m in range(nt))


@pytest.mark.parametrize("F", N_CASES)
@pytest.mark.parametrize("G", [1, 3, 130])
def test_spectrum_sum_bit_identical_to_the_restatement_and_to_its_sibling_at_zero_lag(pr, G, F):
    off, T, I, q, phi, L, tred = synthetic_groups(G, 64, 1e-3, seed=77 * G + F)
    n = len(T)
    rng = np.random.default_rng(F)
    freq = np.linspace(95.0, 55.0, F) if F > 1 else np.array([75.0])
    if F > 2:
        freq[1], freq[-1] = freq[0], 0.0
    alpha = rng.uniform(1e-6, 1e-5, F)
    if F > 1:
        alpha[F // 2] = 0.0
    assert (q < 0).any() and (q > 3).any() and np.isnan(phi).sum() == 1 and (phi == 0).any() and (phi < 0).any()
    zero = np.zeros(G)
    got = {}
    for name, qq, LL, tt, aa in (("plain", q, None, zero, None), ("null", None, None, zero, None),
                                 ("reduced absorbed", q, L, tred, alpha)):
        H = got[name] = _device_spectrum(off, T, I, qq, phi, LL, tt, freq, aa)
        ref = rref.spectrum_sum(off, T, I, qq, phi, LL, tt, freq, aa)
        bad = np.argwhere(~((H.real == ref.real) | (np.isnan(H.real) & np.isnan(ref.real))))
        assert _bits(H, ref), (name, bad[:5])
        sibling = _device_spectrum(off, T, I, qq, None, LL, tt, freq, aa)
        assert _bits(_device_spectrum(off, T, I, qq, np.zeros(n), LL, tt, freq, aa), sibling), name
        assert _bits(_device_spectrum(off, T, I, qq, np.where(np.arange(n) % 2, 3.0, -2.0), LL, tt, freq, aa), sibling), name
        assert G < 130 or not _bits(H, sibling)
    assert _bits(_device_spectrum(off, T, I, q, phi, L, tred, freq, alpha), got["reduced absorbed"])   # repeated calls
    empty = np.flatnonzero(np.diff(off) == 0)
    assert all((got[name][empty] == 0).all() for name in got)
    # tred = 0, no alpha: every column is the group's CW sum with the lags at that frequency
    for k in sorted({0, F // 2, F - 1}):
        assert _bits(got["plain"][:, k], rref.cw_sum(off, T, I, q, phi, freq[k])), k
    # the NaN lag and the NaN I make exactly their groups NaN (where q lets them add)
    grp = np.repeat(np.arange(G), np.diff(off))
    nan_groups = np.unique(grp[(np.isnan(phi) | np.isnan(I)) & (q >= 0)])
    assert np.array_equal(np.flatnonzero(np.isnan(got["plain"].real).any(axis=1)), nan_groups)


# ---- the error paths of the C entries ----------------------------------------------------------------------------------------

def test_c_entries_refuse_bad_arguments_before_writing_anything(pr_any, syn_env):
    import torch
    from pygenray_amd import _lib
    env, cin = syn_env
    Lb = _lib.load()
    vp = ctypes.c_void_p
    # the tube sum
    M, S, R = 70, 6, 9
    z, p, x, p0, depths = synthetic_fan(M, S, R, seed=4, cin=cin)
    t, W, q, phi = synthetic_phase(M, S, 1)
    d, stream = _upload(env, t, z, p, x, p0, depths, np.nan_to_num(phi))
    dev = d[0].device
    re, im = (torch.full((R * S,), MARK, dtype=torch.float64, device=dev) for _ in range(2))

    def tube(f=50.0, n_rays=M, re_=re, im_=im, phi_=d[6]):
        _lib.pressure_phi_device(env, d[0].data_ptr(), d[1].data_ptr(), d[2].data_ptr(), n_rays, S, d[3].data_ptr(),
                                 d[4].data_ptr(), 0, 0 if phi_ is None else phi_.data_ptr(), f, d[5].data_ptr(), R,
                                 0 if re_ is None else re_.data_ptr(), 0 if im_ is None else im_.data_ptr(), stream)
    for kw, msg in ((dict(phi_=None), "null phi"), (dict(f=-1.0), "frequency"), (dict(f=np.nan), "frequency"),
                    (dict(f=np.inf), "frequency"), (dict(n_rays=1), "at least two rays"), (dict(re_=None), "null"),
                    (dict(im_=None), "null")):
        with pytest.raises(_lib.PgrError, match="pgr_pressure_device_phi.*" + msg):
            tube(**kw)
    torch.cuda.synchronize(dev)
    assert (re.cpu().numpy() == MARK).all() and (im.cpu().numpy() == MARK).all()
    tube()                                                               # and the same buffers with good arguments: written
    assert not (re.cpu().numpy() == MARK).any() and not (im.cpu().numpy() == MARK).any()
    fan = pr_any.shoot_rays(1000.0, 0.0, np.linspace(-20.0, 20.0, 70), 20e3, 6, munk_env(pr_any), flatearth=False, debug=False,
                            device_resident=True)
    args = (d[4].data_ptr(), 0)
    with pytest.raises(_lib.PgrError, match="pgr_fan_pressure_phi.*null phi"):
        fan._dev.pressure_phi(*args, 0, 50.0, d[5].data_ptr(), R, re.data_ptr(), im.data_ptr(), stream)
    with pytest.raises(_lib.PgrError, match="pgr_fan_pressure_phi.*frequency"):
        fan._dev.pressure_phi(*args, d[6].data_ptr(), -2.0, d[5].data_ptr(), R, re.data_ptr(), im.data_ptr(), stream)
    # the arrival sums
    G, F = 3, 70
    off, T, I, q, phi, L, ts = synthetic_groups(G, F, 1e-3, seed=2)
    up = lambda a, dt_: torch.from_numpy(np.ascontiguousarray(a, dtype=dt_)).to(dev)   # noqa: E731
    a = dict(off=up(off, np.int64), T=up(T, float), I=up(I, float), phi=up(np.nan_to_num(phi), float), L=up(L, float),
             ts=up(ts, float))
    re, im = (torch.full((G * F,), MARK, dtype=torch.float64, device=dev) for _ in range(2))
    ptr = {k: v.data_ptr() for k, v in a.items()}
    freq, alpha = np.linspace(55.0, 95.0, F), np.full(F, 1e-6)
    good = dict(ptr, G=G, n=F, re=re.data_ptr(), im=im.data_ptr(), f=75.0, rs=200.0, dt=1e-3, freq=freq, alpha=alpha)
    host = lambda v: None if v is None else v.ctypes.data   # noqa: E731

    def signal(**kw):
        g = dict(good, **kw)
        return Lb.pgr_signal_device_phi(0, g["off"], g["G"], g["T"], g["I"], None, g["phi"], g["ts"], g["f"], g["rs"], g["dt"],
                                        g["n"], g["re"], g["im"], vp(stream))

    def spectrum(**kw):
        g = dict(good, **kw)
        return Lb.pgr_spectrum_device_phi(0, g["off"], g["G"], g["T"], g["I"], None, g["phi"], g["L"], g["ts"], host(g["freq"]),
                                          host(g["alpha"]), g["n"], g["re"], g["im"], vp(stream))
    common = [(dict(phi=None), "null phi"), (dict(off=None), "null"), (dict(T=None), "null"), (dict(I=None), "null"),
              (dict(ts=None), "null"), (dict(re=None), "null"), (dict(im=None), "null"), (dict(G=0), "n_groups"),
              (dict(G=2 ** 31), "too many groups")]
    bad = freq.copy()
    bad[3] = -1.0
    for entry, name, cases in ((signal, "pgr_signal_device_phi", common + [
            (dict(n=0), "n_times"), (dict(n=65535 * 256 + 1), "n_times"), (dict(f=-1.0), "frequency"), (dict(f=np.nan), "frequency"),
            (dict(rs=-1.0), "inv_sigma"), (dict(rs=np.inf), "inv_sigma"), (dict(dt=0.0), "dt must be"), (dict(dt=np.nan), "dt must be")]),
                               (spectrum, "pgr_spectrum_device_phi", common + [
            (dict(n=0), "n_freq"), (dict(n=65535 * 256 + 1), "n_freq"), (dict(freq=None), "null"), (dict(alpha=None), "go together"),
            (dict(L=None), "go together"), (dict(freq=bad), "freq must be"), (dict(alpha=bad * 1e-7), "alpha must be")])):
        for kw, msg in cases:
            rc = entry(**kw)
            err = Lb.pgr_last_error().decode()
            assert rc < 0 and name in err and msg in err, (name, kw, rc, err)
    torch.cuda.synchronize(dev)
    assert (re.cpu().numpy() == MARK).all() and (im.cpu().numpy() == MARK).all()
    assert signal() == 0
    assert not (re.cpu().numpy() == MARK).any()
    re.fill_(MARK)
    assert spectrum() == 0 and spectrum(L=None, alpha=None) == 0
    assert not (re.cpu().numpy() == MARK).any() and not (im.cpu().numpy() == MARK).any()
    with pytest.raises(ValueError, match="equal length"):
        _lib.spectrum_phi_device(0, ptr["off"], G, ptr["T"], ptr["I"], 0, ptr["phi"], ptr["L"], ptr["ts"], freq, alpha[:-1],
                                 good["re"], good["im"], stream)
    with pytest.raises(_lib.PgrError, match="pgr_signal_device_phi.*null phi"):
        _lib.signal_phi_device(0, ptr["off"], G, ptr["T"], ptr["I"], 0, 0, ptr["ts"], 75.0, 0.0, 1e-3, F, good["re"], good["im"],
                               stream)


# ---- fans -----------------------------------------------------------------------------------------------------------------

def _shoot(pr, env, resident, n=300, S=81, x1=80e3, K=40):
    return pr.shoot_rays(1000.0, 0.0, np.linspace(-20.0, 20.0, n), x1, S, env, flatearth=False, debug=False,
                         device_resident=resident, max_bounces=K)


def _in_place(fan):
    assert fan.device_resident and not any(k in fan.__dict__ for k in ("_ts", "_zs", "_ps"))


@pytest.fixture(scope="module")
def munk_fan(pr_any):
    """test_spectrum.py's fan: 2001 rays in Munk to 100 km, device resident, with a bounce log of 64 slots; four receivers; the
    last column and a middle one"""
    env = munk_env(pr_any)
    fan = _shoot(pr_any, env, True, n=2001, S=101, x1=100e3, K=64)
    assert fan.n_botts.max() >= 2
    return fan, env, DEPTHS[[100, 300, 500, 700]], [100, 37]


SAND = (1700.0, 1800.0, 0.5)


def test_a_table_without_phase_is_its_loss_pair_bit_for_bit(pr, munk_fan):
    fan, env, d, cols = munk_fan
    g, mag = [0.0, 10.0, 30.0, 90.0], [1.0, 0.8, 0.4, 0.3]
    table = pr.BottomReflection(g, mag, np.zeros(4))
    pair = table.loss
    assert pair[1][0] == 0.0 and pair[1][3] == pytest.approx(-20.0 * np.log10(0.3))
    kw = dict(flatearth=False, surface_loss=0.5)
    p = pr.pressure_field(fan, d, env, 75.0, bottom_loss=table, **kw)
    p0 = pr.pressure_field(fan, d, env, 75.0, bottom_loss=pair, **kw)
    rigid = pr.pressure_field(fan, d, env, 75.0, **kw)
    assert _bits(p, p0) and not _bits(p, rigid) and (np.abs(p[:, cols]) > 0).sum() >= 6
    u = pr.received_signal(fan, d, env, 75.0, 20.0, [66.0, 24.0], 0.01, 40, range_indices=cols, bottom_loss=table, **kw)
    u0 = pr.received_signal(fan, d, env, 75.0, 20.0, [66.0, 24.0], 0.01, 40, range_indices=cols, bottom_loss=pair, **kw)
    assert _bits(u, u0) and (np.abs(u) > 0).any()
    for absorption in (None, pr.thorp_absorption):
        H = pr.transfer_function(fan, d, env, [50.0, 75.0], range_indices=cols, bottom_loss=table, absorption=absorption, **kw)
        H0 = pr.transfer_function(fan, d, env, [50.0, 75.0], range_indices=cols, bottom_loss=pair, absorption=absorption, **kw)
        assert _bits(H, H0)
    # every incoherent product takes the magnitude alone: the call with the .loss pair, bit for bit
    sand = pr.fluid_halfspace(*SAND)
    for product in (pr.transmission_loss, pr.beam_transmission_loss):
        a, b = (product(fan, d, env, flatearth=False, bottom_loss=bl) for bl in (sand, sand.loss))
        assert _same(a, b) and not _same(a, product(fan, d, env, flatearth=False))
    assert _same(pr.boundary_loss(fan, env, bottom_loss=sand, flatearth=False), pr.boundary_loss(fan, env, bottom_loss=sand.loss, flatearth=False))
    _in_place(fan)


def test_every_coherent_product_carries_the_same_phase(pr, munk_fan):
    fan, env, d, cols = munk_fan
    sand = pr.fluid_halfspace(*SAND)
    freq = [50.0, 75.0, 75.37, 250.0]
    for kw in (dict(bottom_loss=sand), dict(bottom_loss=sand, absorption=0.05, surface_loss=0.5)):
        H = pr.transfer_function(fan, d, env, freq, range_indices=cols, flatearth=False, **kw)
        for k, f in enumerate(freq):
            p = pr.pressure_field(fan, d, env, f, flatearth=False, **kw)[:, cols]
            assert (np.abs(p) > 0).sum() >= 6 and _bits(H[:, :, k], p), (kw, f)
            magnitude_only = pr.pressure_field(fan, d, env, f, flatearth=False, **dict(kw, bottom_loss=sand.loss))[:, cols]
            assert not _bits(p, magnitude_only)                         # the phase matters
        p = pr.pressure_field(fan, d, env, 75.0, flatearth=False, **kw)[:, cols]
        u = pr.received_signal(fan, d, env, 75.0, 0.0, [66.0, 24.0], 0.01, 5, range_indices=cols, flatearth=False, **kw)
        assert all(_bits(u[:, :, m], p) for m in range(5))
        tl = pr.coherent_transmission_loss(fan, d, env, 75.0, flatearth=False, **kw)[:, cols]
        with np.errstate(divide="ignore"):
            assert _same(tl, -20.0 * np.log10(np.abs(p)))
    again = pr.pressure_field(fan, d, env, 75.0, flatearth=False, **kw)[:, cols]
    assert _bits(again, p)                                              # two calls are bit-equal
    _in_place(fan)


def test_arrivals_carry_the_lag_the_sums_use(pr, munk_fan):
    fan, env, d, cols = munk_fan
    sand = pr.fluid_halfspace(*SAND)
    a = pr.arrivals(fan, d, env, flatearth=False, range_indices=cols, bottom_loss=sand)
    plain = pr.arrivals(fan, d, env, flatearth=False, range_indices=cols, bottom_loss=sand.loss)
    assert plain.bottom_phase is None and pr.arrivals(fan, d, env, flatearth=False, range_indices=cols).bottom_phase is None
    assert np.array_equal(a.tube, plain.tube) and np.array_equal(a.w, plain.w) and np.array_equal(a.intensity, plain.intensity)
    # the lag array: the boundary post-pass with the lag table in the bottom's slot, as the public boundary_loss runs it
    Phi = pr.boundary_loss(fan, env, bottom_loss=sand.lag, range_indices=cols, flatearth=False)           # (M, n)
    slot = np.repeat(np.arange(len(a.offsets) - 1), np.diff(a.offsets)) % len(cols)
    ref = rref.arrival_lag(Phi[a.tube, slot], Phi[a.tube + 1, slot], a.w)
    assert a.bottom_phase.shape == a.w.shape and np.array_equal(a.bottom_phase, ref) and len(ref) > 20
    nb, _ = fan.bounce_counts(cols)
    bounced = nb[a.tube, slot] > 0
    assert bounced.sum() > 5 and (a.bottom_phase[bounced & (nb[a.tube + 1, slot] > 0)] > 0).all()
    assert (a.bottom_phase[(nb[a.tube, slot] == 0) & (nb[a.tube + 1, slot] == 0)] == 0).all()
    # ... and pressure_field is the sum over these arrivals with that lag
    kappa = pr.caustic_index(fan, env, flatearth=False)
    nb, ns = fan.bounce_counts(cols)
    alike = (nb[a.tube, slot] == nb[a.tube + 1, slot]) & (ns[a.tube, slot] == ns[a.tube + 1, slot])
    q = np.where(alike, kappa[a.tube, np.asarray(cols)[slot]] + 2 * ns[a.tube, slot], -1)
    p = pr.pressure_field(fan, d, env, 75.0, flatearth=False, bottom_loss=sand)[:, cols]
    assert _bits(rref.cw_sum(a.offsets, a.time, a.intensity, q, a.bottom_phase, 75.0).reshape(len(d), len(cols)), p)
    _in_place(fan)


def _group_amplitudes(pr, fan, d, env, cols, **kw):
    a = pr.arrivals(fan, d, env, flatearth=False, range_indices=cols, **kw)
    n = len(cols)
    slot = np.repeat(np.arange(len(a.offsets) - 1), np.diff(a.offsets)) % n
    nb, ns = fan.bounce_counts(cols)
    alike = (nb[a.tube, slot] == nb[a.tube + 1, slot]) & (ns[a.tube, slot] == ns[a.tube + 1, slot])
    amp = np.where(alike, np.sqrt(a.intensity), 0.0)
    return a, np.array([amp[a.offsets[g]:a.offsets[g + 1]].sum() for g in range(len(a.offsets) - 1)]).reshape(len(d), n)


def test_waveform_of_a_gaussian_source_is_received_signal_over_the_half_space(pr_any, munk_fan):
    """tests/test_spectrum.py's synthesis identity with a complex bottom, within its bound (the terms of the bound do not involve
    the arrivals' constant phases): received_waveform inherits the lag from transfer_function"""
    fan, env, d, cols = munk_fan
    f, B = 250.0, spref.SYNTH_B
    sigma = sref.pulse_sigma(B)
    dt = sigma / 4
    source, tc = spref.gaussian_source(sigma, dt)
    kw = dict(range_indices=cols, flatearth=False, surface_loss=0.5, bottom_loss=pr_any.fluid_halfspace(*SAND))
    a, A = _group_amplitudes(pr_any, fan, d, env, cols, surface_loss=0.5, bottom_loss=kw["bottom_loss"])
    n = len(cols)
    slot = np.repeat(np.arange(len(a.offsets) - 1), np.diff(a.offsets)) % n
    windows = [spref.covering_fft(a.time[slot == c].min(), a.time[slot == c].max(), sigma, dt, len(source)) for c in range(n)]
    t0, n_fft = np.array([w[0] for w in windows]), max(w[1] for w in windows)
    assert n_fft <= 8192
    u = pr_any.received_waveform(fan, d, env, source, dt, f, t0, n_fft=n_fft, **kw)
    ref = pr_any.received_signal(fan, d, env, f, B, t0 - tc, dt, n_fft, **kw)
    err = np.abs(u - ref).max(axis=2)
    lit = A > 0
    print(f"received_waveform against received_signal over the half-space: worst |u - ref| is "
          f"{(err[lit] / (spref.SYNTH_REL * A[lit])).max():.3e} of the bound; n_fft {n_fft}, {len(a)} arrivals")
    assert (err <= spref.SYNTH_REL * A).all(), (err, A)
    assert lit.sum() >= 6 and (np.abs(ref).max(axis=2)[lit] > 1e6 * spref.SYNTH_REL * A[lit]).all()
    rigid = pr_any.received_signal(fan, d, env, f, B, t0 - tc, dt, n_fft, **dict(kw, bottom_loss=kw["bottom_loss"].loss))
    assert (np.abs(rigid - ref).max(axis=2) > 1e4 * spref.SYNTH_REL * A).any()
    _in_place(fan)


@pytest.mark.parametrize("which", ["munk", "sloping", "munk-dropped", "sloping-dropped"])
def test_fans_in_both_layouts_resident_and_host_give_one_answer(pr, which):
    """rows (munk) and sample-blocked (sloping) fans, with dropped rays skipped through the keep list: the coherent products of
    the device-resident fan and of the same fan on the host, bit for bit, and against the restatement on the fetched fan"""
    env = {"munk": munk_env, "sloping": sloping_env, "munk-dropped": lambda p: munk_env(p, ztop=4200.0),
           "sloping-dropped": sloping_env_shallow_table}[which](pr)
    fan, eager = _shoot(pr, env, True), _shoot(pr, env, False)
    assert fan._dev._env.blocked_layout == which.startswith("sloping")
    assert (len(eager) < 300) == which.endswith("dropped") and len(eager) > 50 and fan._dev.N == 300
    sand = pr.fluid_halfspace(*SAND)
    d, cols = DEPTHS[::100], [80, 33, 0]
    x = np.asarray(eager.rs[0])[cols]
    kw = dict(flatearth=False, bottom_loss=sand, surface_loss=0.5)
    p, host = (pr.pressure_field(f, d, env, 25.0, **kw) for f in (fan, eager))
    assert _bits(p, host) and np.isnan(p[:, 0]).all() and (np.abs(p[:, 1:]) > 0).mean() > 0.2
    freq = np.linspace(20.0, 30.0, 70)
    H, Hh = (pr.transfer_function(f, d, env, freq, range_indices=cols, t_reduce=x / 1500.0, absorption=pr.thorp_absorption, **kw)
             for f in (fan, eager))
    assert _bits(H, Hh) and np.isnan(H[:, 2]).all() and not np.isnan(H[:, :2]).any()
    u, uh = (pr.received_signal(f, d, env, 25.0, 10.0, x / 1500.0 - 0.5, 0.02, 150, range_indices=cols, **kw) for f in (fan, eager))
    assert _bits(u, uh) and (np.abs(u[:, :2]) > 0).any()
    a, ah = (pr.arrivals(f, d, env, flatearth=False, range_indices=cols, bottom_loss=sand) for f in (fan, eager))
    assert np.array_equal(a.bottom_phase, ah.bottom_phase)
    _in_place(fan)
    # against the restatement on the fetched fan: the lags from the public boundary_loss, the weights from its dB
    nb, ns = eager.bounce_counts(np.arange(81))
    if which.endswith("dropped") or nb.max() == 0:
        return
    Phi = pr.boundary_loss(eager, env, bottom_loss=sand.lag, flatearth=False)
    B = pr.boundary_loss(eager, env, bottom_loss=sand, surface_loss=0.5, flatearth=False)
    import path_reference as pref
    ref = rref.fan_pressure(eager, d, env, 25.0, Phi, flatearth=False, W=pref.weights(B), nb=nb, ns=ns)
    assert _bits(p, ref) and (Phi > 0).any()


# ---- the waveguide over a fluid half-space ------------------------------------------------------------------------------------

def test_waveguide_over_the_half_space_from_shoot_rays(pr):
    env = wref.guide_env(pr)
    fan = pr.shoot_rays(wref.GUIDE_ZS, 0.0, wref.guide_angles(), wref.GUIDE_X1, wref.GUIDE_S, env, flatearth=False, debug=False,
                        device_resident=True, max_bounces=wref.GUIDE_K)
    assert len(fan) == wref.GUIDE_N and fan.n_botts.max() == 2 and fan.n_surfs.max() == 2
    x = np.asarray(fan.rs[0])[wref.GUIDE_COLS]
    keep, sub = rref.check_guide_bottom_cells(x)
    bottom = pr.fluid_halfspace(*rref.GUIDE_BOTTOM)
    bounds = rref.guide_bounds()
    kw = dict(flatearth=False, bottom_loss=bottom)
    p = pr.pressure_field(fan, wref.GUIDE_DEPTHS, env, wref.GUIDE_F, **kw)[:, wref.GUIDE_COLS]
    e = rref.guide_error(p, x)
    print(f"waveguide over the half-space from shoot_rays: tube sum worst e {e.max():.4e}, bound {bounds[0]:.4e}")
    assert e.max() <= bounds[0]
    Hf = pr.transfer_function(fan, wref.GUIDE_DEPTHS, env, wref.GUIDE_BAND, range_indices=wref.GUIDE_COLS,
                              t_reduce=x / wref.GUIDE_C, **kw)
    e = rref.guide_band_error(Hf, x)
    print(f"  band sum worst e per frequency {[f'{v:.4e}' for v in e.max(axis=(0, 1))]}, bound {bounds[1]:.4e}")
    assert e.max() <= bounds[1]
    u = pr.received_signal(fan, wref.GUIDE_DEPTHS, env, wref.GUIDE_F, wref.GUIDE_B, wref.guide_t0(x), wref.GUIDE_DT, wref.GUIDE_NT,
                           range_indices=wref.GUIDE_COLS, **kw)
    e = rref.guide_pulse_error(u, x)
    print(f"  pulse sum worst e {e.max():.4e}, bound {bounds[2]:.4e}")
    assert e.max() <= bounds[2]
    _in_place(fan)
