"""Received signal of a Gaussian pulse on the GPU (csrc/pgr_signal.h): the kernel alone through ``_lib.signal_device`` against
the restatement of tests/signal_reference.py on synthetic arrivals aimed at its staging and tile seams, the CW identity with
``pressure_field`` and the Fourier identity end to end on a Munk fan, fans in both trajectory layouts (dropped rays, host
fans), Lloyd's mirror with a pulse from ``shoot_rays``, and the error paths of the C entry."""
import ctypes
import math
import os
import re
import subprocess
import sys

import numpy as np
import pytest

import coherent_reference as cref
import signal_reference as sref
from tube_gpu import (DEPTHS, _same, munk_env, pr, pr_any, sloping_env, sloping_env_shallow_table)  # noqa: F401

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
PAD = 130                    # entries behind an output that must stay as they were
MARK = -7.25
FAN_PROFILE = ([0.0, 300.0, 1200.0, 4000.0], [0.9, 0.5, 0.08, 0.2])          # dB/km, as the public functions take it


def _tile():
    """the samples one wave of pgr_sig_sum handles: 64 lanes times SIG_ROWS samples per lane, from the kernel's own source"""
    from pygenray_amd import _lib
    text = open(os.path.join(_lib.CSRC, "pgr_signal.h")).read()
    return 64 * int(re.search(r"^#define SIG_ROWS (\d+)", text, re.M).group(1))


TILE = _tile()


# ---- the kernel alone ---------------------------------------------------------------------------------------------------------

def _device_signal(off, T, I, q, tstart, f, rs, dt, nt):
    """_lib.signal_device on host arrays -> u (G, nt) complex; both outputs pre-filled with a sentinel, PAD entries behind
    them checked untouched and every entry before them checked written"""
    import torch
    from pygenray_amd import _lib
    dev = torch.device("cuda", 0)
    G = len(off) - 1
    up = lambda a, dt_: torch.from_numpy(np.ascontiguousarray(a, dtype=dt_)).to(dev)   # noqa: E731
    d_off, d_T, d_I, d_ts = up(off, np.int64), up(np.append(T, 0.0), float), up(np.append(I, 0.0), float), up(tstart, float)
    d_q = None if q is None else up(np.append(q, 0), np.int32)
    out = [torch.full((G * nt + PAD,), MARK, dtype=torch.float64, device=dev) for _ in range(2)]
    _lib.signal_device(0, d_off.data_ptr(), G, d_T.data_ptr(), d_I.data_ptr(), 0 if d_q is None else d_q.data_ptr(),
                       d_ts.data_ptr(), f, rs, dt, nt, out[0].data_ptr(), out[1].data_ptr(),
                       torch.cuda.current_stream(dev).cuda_stream)
    h = [a.cpu().numpy() for a in out]
    assert all((a[G * nt:] == MARK).all() for a in h) and not any((a[:G * nt] == MARK).any() for a in h)
    return (h[0][:G * nt] + 1j * h[1][:G * nt]).reshape(G, nt)


COUNTS = [200, 0, 65, 1, 63, 64]             # the staging seams: groups of every one of these in one call (G = 130)


def synthetic_groups(G, nt, dt, seed):
    """groups with COUNTS arrivals (then random counts up to 130), a start time per group, arrivals before, after, on both
    ends of and inside each group's time axis, I over six decades with exact zeros and a NaN, q in -1 ... 9"""
    rng = np.random.default_rng(seed)
    cnt = np.array([COUNTS[g] if g < len(COUNTS) else int(rng.integers(0, 131)) for g in range(G)])
    off = np.concatenate([[0], np.cumsum(cnt)]).astype(np.int64)
    n = int(off[-1])
    tstart = 60.0 + rng.uniform(-3.0, 3.0, G)
    span = (nt - 1) * dt
    grp = np.repeat(np.arange(G), cnt)
    T = tstart[grp] + rng.uniform(-0.06, span + 0.06, n)
    edge = rng.random(n)
    T = np.where(edge < 0.08, tstart[grp] + rng.uniform(-0.004, 0.004, n), T)                 # straddling the first sample
    T = np.where(edge > 0.92, tstart[grp] + span + rng.uniform(-0.004, 0.004, n), T)          # ... and the last
    order = np.lexsort((T, grp))                                        # (any order within a group would do: this one is tidy)
    T = T[order]
    I = 10.0 ** rng.uniform(-12.0, -6.0, n)
    I[rng.random(n) < 0.05] = 0.0
    if n > 20:
        I[n // 3] = np.nan
    q = rng.integers(-1, 10, n).astype(np.int32)
    return off, T, I, q, tstart


NT_CASES = [1, 63, 64, 65, TILE - 1, TILE, TILE + 1]


@pytest.mark.parametrize("nt", NT_CASES)
@pytest.mark.parametrize("G", [1, 3, 130])
def test_kernel_bit_identical_to_the_restatement_on_synthetic_groups(pr, G, nt):
    dt, f = 1e-3, 75.0
    off, T, I, q, tstart = synthetic_groups(G, nt, dt, seed=1000 * G + nt)
    assert G < 130 or set(COUNTS) <= set(np.diff(off).tolist())
    assert len(set(tstart.tolist())) == G and (q < 0).any() and (q > 3).any() and (I == 0).any() and np.isnan(I).any()
    got = {}
    for rs in (0.0, 200.0):                                            # CW, and sigma = 5 ms: windows of 80 samples
        for name, qq in (("q", q), ("null", None)):
            u = got[rs, name] = _device_signal(off, T, I, qq, tstart, f, rs, dt, nt)
            ref = sref.signal_sum(off, T, I, qq, tstart, f, rs, dt, nt)
            bad = np.argwhere(~((u.real == ref.real) | (np.isnan(u.real) & np.isnan(ref.real))))
            assert _same(u.real, ref.real) and _same(u.imag, ref.imag), (rs, name, bad[:5])
        again = _device_signal(off, T, I, q, tstart, f, rs, dt, nt)      # repeated calls are bit-equal
        assert _same(again.real, got[rs, "q"].real) and _same(again.imag, got[rs, "q"].imag)
        assert G < 130 or not _same(got[rs, "q"].real, got[rs, "null"].real)        # q matters
    empty = np.flatnonzero(np.diff(off) == 0)
    assert all((got[rs, name][empty] == 0).all() for rs, name in got)   # empty groups are written: zeros
    # rs = 0: every sample of a group is the group's CW sum
    p = sref.cw_sum(off, T, I, q, f)
    assert all(_same(got[0.0, "q"][:, m].real, p.real) and _same(got[0.0, "q"][:, m].imag, p.imag) for m in range(nt))
    if nt >= 63 and G == 130:
        # the finite pulse: arrivals off the axis' ends by more than 8 sigma add nothing, and the signal varies along the axis
        u = got[200.0, "q"]
        assert (np.nan_to_num(np.abs(u)) > 0).any() and not _same(u[:, 0].real, u[:, -1].real)


def test_kernel_with_a_sigma_so_short_that_windows_hold_no_sample(pr):
    dt, f, nt = 1e-3, 75.0, TILE + 1
    off, T, I, q, tstart = synthetic_groups(3, nt, dt, seed=5)
    rs = 1.0 / (dt / 20.0)                                              # 8 sigma = 0.4 dt: most arrivals fall between samples
    ref = sref.signal_sum(off, T, I, q, tstart, f, rs, dt, nt)
    u = _device_signal(off, T, I, q, tstart, f, rs, dt, nt)
    assert _same(u.real, ref.real) and _same(u.imag, ref.imag)
    t = sref.sample_times(tstart, dt, nt)
    grp = np.repeat(np.arange(3), np.diff(off))
    x = (t[grp] - T[:, None]) * rs
    seen = ((x * x <= 64.0) & (q >= 0)[:, None]).any(axis=1)
    inside = (T > tstart[grp]) & (T < tstart[grp] + (nt - 1) * dt) & (q >= 0)
    assert (inside & ~seen).sum() > 20 and (inside & seen).sum() > 20
    assert 0 < (np.nan_to_num(np.abs(u)) > 0).sum() < u.size // 2


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


def test_bandwidth_zero_is_pressure_field_bit_for_bit(pr, munk_fan):
    fan, env, d, cols = munk_fan
    for kw in ({}, dict(absorption=FAN_PROFILE, surface_loss=0.5)):
        p = pr.pressure_field(fan, d, env, 75.0, flatearth=False, **kw)[:, cols]
        u = pr.received_signal(fan, d, env, 75.0, 0.0, [66.0, 24.0], 0.01, 5, range_indices=cols, flatearth=False, **kw)
        assert u.shape == (len(d), len(cols), 5) and u.dtype == np.complex128 and (np.abs(p) > 0).sum() >= 6
        for m in range(5):
            assert _same(u[:, :, m].real, p.real) and _same(u[:, :, m].imag, p.imag), m
    _in_place(fan)
    # the source's own column is NaN, as in pressure_field; a default range_indices is the last column
    u = pr.received_signal(fan, d, env, 75.0, 20.0, 0.0, 0.01, 3, range_indices=[0, -1], flatearth=False)
    assert np.isnan(u[:, 0]).all() and not np.isnan(u[:, 1]).any()
    one = pr.received_signal(fan, d, env, 75.0, 0.0, 0.0, 0.01, 2, flatearth=False)
    assert one.shape == (len(d), 1, 2) and _same(one[:, 0, 0].real, pr.pressure_field(fan, d, env, 75.0, flatearth=False)[:, -1].real)
    # a signal that does not fit in the device's memory is refused before any kernel runs
    with pytest.raises(ValueError, match="bytes of device memory"):
        pr.received_signal(fan, np.linspace(10.0, 4000.0, 20000), env, 75.0, 20.0, 0.0, 0.01, 65535 * 256, range_indices=cols,
                           flatearth=False)
    _in_place(fan)


def test_identity_spectrum_of_the_signal_is_the_cw_field_under_the_pulse_spectrum(pr_any, munk_fan):
    """the Fourier identity of tests/test_signal_host.py end to end, with its bound: in either arithmetic"""
    fan, env, d, cols = munk_fan
    f, B = sref.FOURIER_F, sref.FOURIER_B
    sigma = sref.pulse_sigma(B)
    a = pr_any.arrivals(fan, d, env, flatearth=False, range_indices=cols)
    n = len(cols)
    slot = np.repeat(np.arange(len(a.offsets) - 1), np.diff(a.offsets)) % n
    assert all((slot == c).sum() >= 4 for c in range(n)) and len(a) > 20
    axes = [sref.covering_axis(a.time[slot == c].min(), a.time[slot == c].max(), sigma) for c in range(n)]
    t0, dt, nt = np.array([ax[0] for ax in axes]), axes[0][1], max(ax[2] for ax in axes)
    assert dt == sigma / 2 and nt < 2000
    u = pr_any.received_signal(fan, d, env, f, B, t0, dt, nt, range_indices=cols, flatearth=False)
    again = pr_any.received_signal(fan, d, env, f, B, t0, dt, nt, range_indices=cols, flatearth=False)
    assert _same(u.real, again.real) and _same(u.imag, again.imag)
    t = t0[None, :, None] + (np.arange(nt) * dt)[None, None, :]
    # the amplitudes that add: the arrivals whose tube is not folded over a boundary (q >= 0)
    nb, ns = fan.bounce_counts(cols)
    alike = (nb[a.tube, slot] == nb[a.tube + 1, slot]) & (ns[a.tube, slot] == ns[a.tube + 1, slot])
    amp = np.where(alike, np.sqrt(a.intensity), 0.0)
    A = np.array([amp[a.offsets[g]:a.offsets[g + 1]].sum() for g in range(len(a.offsets) - 1)]).reshape(len(d), n)
    bound = sref.FOURIER_REL * sigma * math.sqrt(2 * math.pi) * A
    worst = 0.0
    for nu in sref.FOURIER_NU:
        U = sref.spectrum(u, t, dt, nu)
        ref = sref.pulse_spectrum(sigma, nu) * pr_any.pressure_field(fan, d, env, f + nu, flatearth=False)[:, cols]
        err = np.abs(U - ref)
        worst = max(worst, float((err[A > 0] / bound[A > 0]).max()))
        assert (err <= bound).all(), (nu, err, bound)
        assert (np.abs(ref) > 100 * bound).sum() >= 4
    print(f"Fourier identity end to end: worst |U - Ehat P| is {worst:.3e} of the bound; {nt} samples, {len(a)} arrivals")
    _in_place(fan)


def test_identities_hold_in_contracted_arithmetic():
    from pygenray_amd import _lib
    if _lib.ARITH != "reference":
        pytest.skip("this IS the contracted process")
    if not os.path.exists(_lib.CONTRACTED_LIB):
        pytest.fail("libpgr_hip_fma.so is not built (__graft_entry__.build() builds it beside the product)")
    out = subprocess.run([sys.executable, "-m", "pytest", "-q", "-m", "gpu", "-x", "-p", "no:cacheprovider", "-k", "identity_spectrum",
                          os.path.join(ROOT, "tests", "test_signal.py")],
                         cwd=ROOT, env=dict(os.environ, PGR_ARITH="contracted"), capture_output=True, text=True, timeout=600)
    tail = out.stdout[-3000:] + out.stderr[-1500:]
    assert out.returncode == 0 and " passed" in out.stdout and "failed" not in out.stdout, tail


@pytest.mark.parametrize("which", ["munk", "sloping", "munk-dropped", "sloping-dropped"])
def test_fans_in_both_layouts_resident_and_host_give_one_answer(pr, which):
    """rows (munk) and sample-blocked (sloping) fans, with dropped rays skipped through the keep list: received_signal of the
    device-resident fan and of the same fan on the host, bit for bit, and at B = 0 pressure_field's value"""
    env = {"munk": munk_env, "sloping": sloping_env, "munk-dropped": lambda p: munk_env(p, ztop=4200.0),
           "sloping-dropped": sloping_env_shallow_table}[which](pr)
    fan, eager = _shoot(pr, env, True), _shoot(pr, env, False)
    assert fan._dev._env.blocked_layout == which.startswith("sloping")
    assert (len(eager) < 300) == which.endswith("dropped") and len(eager) > 50 and fan._dev.N == 300
    d, cols = DEPTHS[::100], [80, 33]
    x = np.asarray(eager.rs[0])[cols]
    t0 = x / 1500.0 - 0.5
    for kw in ({}, dict(absorption=FAN_PROFILE)):
        u = pr.received_signal(fan, d, env, 25.0, 10.0, t0, 0.01, 300, range_indices=cols, flatearth=False, **kw)
        host = pr.received_signal(eager, d, env, 25.0, 10.0, t0, 0.01, 300, range_indices=cols, flatearth=False, **kw)
        assert u.shape == (len(d), 2, 300) and _same(u.real, host.real) and _same(u.imag, host.imag)
        assert (np.abs(u).max(axis=2) > 0).mean() > 0.2 and (np.abs(u) == 0).any()
        cw = pr.received_signal(eager, d, env, 25.0, 0.0, t0, 0.01, 2, range_indices=cols, flatearth=False, **kw)
        p = pr.pressure_field(fan, d, env, 25.0, flatearth=False, **kw)[:, cols]
        assert _same(cw[:, :, 1].real, p.real) and _same(cw[:, :, 1].imag, p.imag)
    _in_place(fan)


def test_lloyds_mirror_with_a_pulse_end_to_end(pr):
    env = cref.lloyd_env(pr)
    fan = pr.shoot_rays(cref.LLOYD_ZS, 0.0, cref.lloyd_angles(), cref.LLOYD_X1, cref.LLOYD_S, env, flatearth=False,
                        debug=False, device_resident=True, max_bounces=4)
    assert len(fan) == cref.LLOYD_N and (fan.n_botts == 0).all() and fan.n_surfs.max() == 1
    x = np.asarray(fan.rs[0])[cref.LLOYD_COLS]
    u = pr.received_signal(fan, cref.LLOYD_DEPTHS, env, cref.LLOYD_F, sref.LLOYD_B, sref.lloyd_t0(x), sref.LLOYD_DT,
                           sref.LLOYD_NT, range_indices=cref.LLOYD_COLS, flatearth=False)
    _in_place(fan)
    e = sref.lloyd_pulse_error(u, x)
    j, k, m = np.unravel_index(np.argmax(e), e.shape)
    print(f"Lloyd's mirror with a pulse from shoot_rays: worst e {e.max():.4e} at depth {cref.LLOYD_DEPTHS[j]} m, range "
          f"{x[k]} m, sample {m}; bound {sref.LLOYD_PULSE_BOUND:.4e}")
    assert e.max() <= sref.LLOYD_PULSE_BOUND < 0.05


# ---- the error paths of the C entry ------------------------------------------------------------------------------------------

def test_c_entry_refuses_bad_arguments_before_writing_anything(pr_any):
    import torch
    from pygenray_amd import _lib
    L = _lib.load()
    dev = torch.device("cuda", 0)
    G, nt = 3, 70
    off, T, I, q, tstart = synthetic_groups(G, nt, 1e-3, seed=2)
    up = lambda a, dt_: torch.from_numpy(np.ascontiguousarray(a, dtype=dt_)).to(dev)   # noqa: E731
    d = dict(off=up(off, np.int64), T=up(T, float), I=up(I, float), ts=up(tstart, float))
    re, im = (torch.full((G * nt,), MARK, dtype=torch.float64, device=dev) for _ in range(2))
    stream = torch.cuda.current_stream(dev).cuda_stream
    good = dict(off=d["off"].data_ptr(), G=G, T=d["T"].data_ptr(), I=d["I"].data_ptr(), ts=d["ts"].data_ptr(), f=75.0, rs=200.0,
                dt=1e-3, nt=nt, re=re.data_ptr(), im=im.data_ptr())

    def call(**kw):
        a = dict(good, **kw)
        return L.pgr_signal_device(0, a["off"], a["G"], a["T"], a["I"], None, a["ts"], a["f"], a["rs"], a["dt"], a["nt"],
                                   a["re"], a["im"], ctypes.c_void_p(stream))
    cases = [(dict(off=None), "null"), (dict(T=None), "null"), (dict(I=None), "null"), (dict(ts=None), "null"),
             (dict(re=None), "null"), (dict(im=None), "null"), (dict(G=0), "n_groups"), (dict(G=-1), "n_groups"),
             (dict(nt=0), "n_times"), (dict(nt=-5), "n_times"), (dict(nt=65535 * TILE + 1), "n_times"),
             (dict(f=-1.0), "frequency"), (dict(f=np.nan), "frequency"), (dict(f=np.inf), "frequency"),
             (dict(rs=-1.0), "inv_sigma"), (dict(rs=np.nan), "inv_sigma"), (dict(rs=np.inf), "inv_sigma"),
             (dict(dt=0.0), "dt"), (dict(dt=-1e-3), "dt"), (dict(dt=np.nan), "dt"), (dict(dt=np.inf), "dt")]
    for kw, msg in cases:
        rc = call(**kw)
        err = L.pgr_last_error().decode()
        assert rc < 0 and "pgr_signal_device" in err and msg in err, (kw, rc, err)
    torch.cuda.synchronize(dev)
    assert (re.cpu().numpy() == MARK).all() and (im.cpu().numpy() == MARK).all()
    assert call() == 0                                                   # and the same buffers with good arguments: written
    assert not (re.cpu().numpy() == MARK).any() and not (im.cpu().numpy() == MARK).any()
    with pytest.raises(_lib.PgrError, match="pgr_signal_device.*dt"):
        _lib.signal_device(0, good["off"], G, good["T"], good["I"], 0, good["ts"], 75.0, 200.0, 0.0, nt, good["re"], good["im"], stream)
