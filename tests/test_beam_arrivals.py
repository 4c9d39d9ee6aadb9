"""beam_arrivals and the sums over them on the GPU (csrc/pgr_beam_arrivals.h): pgr_beam_arrival_counts_device_w and
pgr_beam_arrivals_device_w bit for bit against the restatement of tests/beam_arrivals_reference.py on synthetic buffers aimed at
the kernels' chunk, halo, band, column-list and 4-sigma seams, the refusals of the four C entries, Munk fans in every layout and
on either side of the bus -- the list itself, and summed by the transfer function and the pulse it is beam_pressure_field bit for
bit -- the synthesis identity of beam_received_waveform, and Lloyd's mirror with a pulse from ``shoot_rays`` within the bound
tests/test_beam_arrivals_host.py measured."""
import numpy as np
import pytest

import beam_arrivals_reference as ba
import beam_pressure_reference as bp
import beam_reference as bref
import coherent_reference as cref
import path_reference as pref
import signal_reference as sref
import spectrum_reference as spref
from test_beam_pressure import FAN_COLS, FAN_N, FAN_PROFILE, FAN_S, _in_place, _shoot, synthetic_phase
from tube_gpu import (DEPTHS, SYN_R, SYN_Z, _same, _upload, munk_env, pr, pr_any, sloping_env,  # noqa: F401
                      sloping_env_shallow_table, syn_env, synthetic_fan)

pytestmark = pytest.mark.gpu

PAD = 130                    # entries either side of an output that must stay as they were
MARK, IMARK = -7.25, -7
KEYS = ("tube", "image", "time", "amplitude", "q")


def _padded(n, dtype, dev):
    import torch
    return torch.full((PAD + n + PAD,), IMARK if dtype != torch.float64 else MARK, dtype=dtype, device=dev)


def _inner(t, n):
    """a padded output on the host: its n entries, the sentinels either side checked untouched"""
    h = t.cpu().numpy()
    mark = MARK if h.dtype == np.float64 else IMARK
    assert (h[:PAD] == mark).all() and (h[PAD + n:] == mark).all()
    return h[PAD:PAD + n]


def _device_beam_arrivals(env, t, z, p, x, p0, bottom, depths, w_min, W, q, cols, curvature, drop=0):
    """_lib.beam_arrival_counts_device and _lib.beam_arrivals_device on [S][M] rows -> the restatement's dict; sentinels before
    and behind every output checked untouched.  `drop`: the emit pass is told the outputs hold that many arrivals fewer."""
    import torch
    from pygenray_amd import _lib
    d, stream = _upload(env, t, z, p, x, p0, bottom, depths, *(() if W is None else (W,)))
    dev = d[0].device
    S, M = z.shape
    R, n = len(depths), len(cols)
    dq = None if q is None else torch.from_numpy(np.ascontiguousarray(q, dtype=np.int32)).to(dev)
    head = (env, d[0].data_ptr(), d[1].data_ptr(), d[2].data_ptr(), M, S, d[3].data_ptr(), d[4].data_ptr(),
            0 if dq is None else dq.data_ptr(), d[5].data_ptr(), d[6].data_ptr(), R, w_min, cols)
    kw = dict(weights=0 if W is None else d[7].data_ptr())
    counts = _padded(R * n, torch.int64, dev)
    _lib.beam_arrival_counts_device(*head, counts[PAD:].data_ptr(), stream, **kw)
    cnt = _inner(counts, R * n)
    assert (cnt >= 0).all()
    offsets = np.concatenate([[0], np.cumsum(cnt)]).astype(np.int64)
    total = int(offsets[-1])
    out = dict(offsets=offsets, tube=np.zeros(0, np.int32), image=np.zeros(0, np.int32), time=np.zeros(0), amplitude=np.zeros(0),
               q=np.zeros(0, np.int32))
    if total - drop >= 1:
        d_off = torch.from_numpy(offsets).to(dev)
        bufs = {k: _padded(total, torch.float64 if k in ("time", "amplitude") else torch.int32, dev) for k in KEYS}
        _lib.beam_arrivals_device(*head, curvature, d_off.data_ptr(), total - drop, bufs["tube"][PAD:].data_ptr(),
                                  bufs["image"][PAD:].data_ptr(), bufs["time"][PAD:].data_ptr(),
                                  bufs["amplitude"][PAD:].data_ptr(), bufs["q"][PAD:].data_ptr(), stream, **kw)
        out.update({k: _inner(v, total) for k, v in bufs.items()})
    return out


def _equal(got, ref, upto=None):
    """every array of two arrival dicts, bit for bit (the first `upto` arrivals)"""
    assert np.array_equal(got["offsets"], ref["offsets"]), (got["offsets"][-1], ref["offsets"][-1])
    for k in KEYS:
        a, b = got[k][:upto], ref[k][:upto]
        assert a.dtype == b.dtype and _same(a, b), (k, np.flatnonzero(~((a == b) | ((a != a) & (b != b))))[:5])


def _check(env, cin, t, z, p, x, p0, bottom, depths, w_min, W, q, cols, curvature):
    got = _device_beam_arrivals(env, t, z, p, x, p0, bottom, depths, w_min, W, q, cols, curvature)
    ref = ba.beam_arrivals(z.T, p.T, t.T, x, p0, depths, cin, SYN_R, SYN_Z, bottom, w_min, None if W is None else W.T,
                           None if q is None else q.T, cols, curvature)
    _equal(got, ref)
    return got


# ---- the kernels on synthetic inputs: counts and every emitted array against the restatement, bit for bit ------------------------
#
# A chunk is 61 tubes (lane t loads ray 61 c - 1 + t): the ray counts make the last chunk full or hold one / two tubes; the
# receiver counts make the last band hold 1 / 63 / 64 receivers.  S = 5: column 0 is the source's and column 3 has r = 0 too.
# The column lists: one column; the source's column, the second r = 0 column, a duplicate and an unsorted order; all five.
# Every case runs one combination of (weights, q, curvature, min_width) picked from its index.

SEAM_M = (2, 3, 61, 62, 63, 122, 123, 124)
SEAM_R = (1, 63, 64, 65, 129)
SEAM_COLS = ([4], [3, 0, 2, 2, 4], [0, 1, 2, 3, 4])
SEAM_CASES = [(M, R, c) for M in SEAM_M for R in SEAM_R for c in range(len(SEAM_COLS))] + [(3906, 65, 3)]


def _seam_case(syn_env, M, R, c):
    env, cin = syn_env
    S = 5
    i = SEAM_CASES.index((M, R, c))
    cols = [4, 1] if c == 3 else SEAM_COLS[c]              # (M = 3906: 65 chunks, two ballot rounds)
    z, p, x, p0, depths = synthetic_fan(M, S, R, seed=M * 1013 + S * 37 + R, cin=cin)
    t, W, q = synthetic_phase(M, S, M + 7 * S + R)
    bottom = np.linspace(4700.0, 5150.0, S)                  # a sloping bottom, crossed by the fan's samples
    curvature = (i // 3) % 2
    w = W if (i // 6 + i) % 2 else None
    qq = (None, q, np.where(q > 3, -1, q), q + 4 * (q >= 0))[(i // 2 + i // 15) % 4]     # NULL, with -1 and above 3, ...
    w_min = (40.0, 0.5)[(i // 5) % 2]
    return env, cin, (t, z, p, x, p0, bottom, depths, w_min, w, qq, cols, curvature)


@pytest.mark.parametrize("M, R, c", SEAM_CASES, ids=[f"M{M}-R{R}-cols{c}" for M, R, c in SEAM_CASES])
def test_kernels_bit_identical_on_the_seam_shapes(pr, syn_env, M, R, c):
    env, cin, args = _seam_case(syn_env, M, R, c)
    x, cols = args[3], args[10]
    got = _check(env, cin, *args)
    again = _device_beam_arrivals(env, *args)
    _equal(again, got)                                                              # two calls are bit-equal
    total = int(got["offsets"][-1])
    per = np.diff(got["offsets"]).reshape(R, len(cols))
    assert (per[:, x[cols] == x[0]] == 0).all()                                     # the r = 0 columns have no arrivals
    if M >= 61:
        assert total > 0
    if total >= 4:
        # the outputs hold three arrivals fewer: exactly the last three are dropped, nothing else is written
        short = _device_beam_arrivals(env, *args, drop=3)
        _equal(short, got, upto=total - 3)
        assert all((short[k][total - 3:] == (MARK if short[k].dtype == np.float64 else IMARK)).all() for k in KEYS)


def test_receivers_on_the_four_sigma_edges(pr, syn_env):
    # receivers at centre -+ 4 sigma and one ulp either side, for the beam and both its images (the construction of
    # test_beam_pressure.py): the kept set is the definition's, whatever the chunk test decided
    env, cin = syn_env
    M, S = 400, 4
    z, p, x, p0, depths = synthetic_fan(M, S, 64, seed=11, cin=cin)
    t, W, q = synthetic_phase(M, S, 12)
    bottom = np.array([4900.0, 4950.0, 5000.0, 5050.0])
    w_min = 25.0
    valid, m, sigma, _, _, r = bref._tubes(z.T, p.T, x, p0, cin, SYN_R, SYN_Z, w_min)
    edge = []
    assert x[2] == x[0]                                               # (column 2 is the source's: no arrivals)
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
        got = _check(env, cin, t, z, p, x, p0, bottom, depths, w_min, None, np.where(q > 5, -1, q), [3, 1, 2], curvature)
    assert set(np.unique(got["image"])) == {0, 1, 2} and len(got["tube"]) > 1000


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
    n = 2
    counts = torch.full((R * n,), IMARK, dtype=torch.int64, device=dev)
    N = 4096
    ints = [torch.full((N,), IMARK, dtype=torch.int32, device=dev) for _ in range(3)]
    dbls = [torch.full((N,), MARK, dtype=torch.float64, device=dev) for _ in range(2)]
    offsets = torch.zeros(R * n, dtype=torch.int64, device=dev)
    ptr = lambda a: 0 if a is None else a.data_ptr()   # noqa: E731

    def count(w=10.0, n_rays=M, cols=(5, 1), bottom=d[5], out=counts):
        _lib.beam_arrival_counts_device(env, d[0].data_ptr(), d[1].data_ptr(), d[2].data_ptr(), n_rays, S, d[3].data_ptr(),
                                        d[4].data_ptr(), 0, ptr(bottom), d[6].data_ptr(), R, w, list(cols), ptr(out), stream)

    def emit(w=10.0, n_rays=M, cols=(5, 1), bottom=d[5], off=offsets, n_arr=N, tube=ints[0], image=ints[1], time=dbls[0],
             amp=dbls[1], qa=ints[2]):
        _lib.beam_arrivals_device(env, d[0].data_ptr(), d[1].data_ptr(), d[2].data_ptr(), n_rays, S, d[3].data_ptr(),
                                  d[4].data_ptr(), 0, ptr(bottom), d[6].data_ptr(), R, w, list(cols), 1, ptr(off), n_arr,
                                  ptr(tube), ptr(image), ptr(time), ptr(amp), ptr(qa), stream)
    shared = [(dict(w=0.0), "min_width"), (dict(w=-1.0), "min_width"), (dict(w=np.nan), "min_width"), (dict(w=np.inf), "min_width"),
              (dict(n_rays=1), "at least two rays"), (dict(bottom=None), "null"), (dict(cols=(1, S)), r"cols\[1\] = 6"),
              (dict(cols=(-1,)), r"cols\[0\] = -1"), (dict(cols=()), "n_cols must be|null")]
    for kw, msg in shared + [(dict(out=None), "null")]:
        with pytest.raises(_lib.PgrError, match="pgr_beam_arrival_counts_device_w.*" + msg):
            count(**kw)
    for kw, msg in shared + [(dict(off=None), "null"), (dict(tube=None), "null"), (dict(image=None), "null"),
                             (dict(time=None), "null"), (dict(amp=None), "null"), (dict(qa=None), "null"),
                             (dict(n_arr=0), "n_arrivals must be at least 1")]:
        with pytest.raises(_lib.PgrError, match="pgr_beam_arrivals_device_w.*" + msg):
            emit(**kw)
    untouched = lambda: ((counts.cpu().numpy() == IMARK).all() and all((a.cpu().numpy() == IMARK).all() for a in ints)   # noqa: E731
                         and all((a.cpu().numpy() == MARK).all() for a in dbls))
    assert untouched()
    # the fan entries: the same checks, by name
    fan = pr_any.shoot_rays(1000.0, 0.0, np.linspace(-20.0, 20.0, M), 20e3, S, munk_env(pr_any), flatearth=False, debug=False,
                            device_resident=True)
    for w, cols, msg in ((0.0, [1], "min_width"), (np.inf, [1], "min_width"), (10.0, [S], "is not a column"), (10.0, [], "n_cols must be|null")):
        with pytest.raises(_lib.PgrError, match="pgr_fan_beam_arrival_counts_w.*" + msg):
            fan._dev.beam_arrival_counts(d[4].data_ptr(), 0, d[5].data_ptr(), d[6].data_ptr(), R, w, cols, counts.data_ptr(), stream)
        with pytest.raises(_lib.PgrError, match="pgr_fan_beam_arrivals_w.*" + msg):
            fan._dev.beam_arrivals(d[4].data_ptr(), 0, d[5].data_ptr(), d[6].data_ptr(), R, w, cols, 1, offsets.data_ptr(), N,
                                   ints[0].data_ptr(), ints[1].data_ptr(), dbls[0].data_ptr(), dbls[1].data_ptr(),
                                   ints[2].data_ptr(), stream)
    with pytest.raises(_lib.PgrError, match="pgr_fan_beam_arrivals_w.*n_arrivals must be at least 1"):
        fan._dev.beam_arrivals(d[4].data_ptr(), 0, d[5].data_ptr(), d[6].data_ptr(), R, 10.0, [1], 1, offsets.data_ptr(), 0,
                               ints[0].data_ptr(), ints[1].data_ptr(), dbls[0].data_ptr(), dbls[1].data_ptr(), ints[2].data_ptr(),
                               stream)
    one = pr_any.shoot_rays(1000.0, 0.0, np.array([1.0]), 20e3, S, munk_env(pr_any), flatearth=False, debug=False,
                            device_resident=True)
    with pytest.raises(_lib.PgrError, match="pgr_fan_beam_arrival_counts_w.*at least two rays"):
        one._dev.beam_arrival_counts(d[4].data_ptr(), 0, d[5].data_ptr(), d[6].data_ptr(), R, 10.0, [1], counts.data_ptr(), stream)
    assert untouched() and fan.device_resident
    count()                                                              # and the same buffer with good arguments: written
    assert (counts.cpu().numpy() >= 0).all() and int(counts.sum().item()) > 0


# ---- fans ---------------------------------------------------------------------------------------------------------------------

def _bits(a, b):
    return _same(a.real, b.real) and _same(a.imag, b.imag)


@pytest.mark.parametrize("which", ["munk", "sloping", "munk-dropped", "sloping-dropped"])
def test_munk_fans_in_every_layout_give_one_answer(pr, which):
    """rows (munk) and sample-blocked (sloping) fans of 2001 rays, with dropped rays skipped through the keep list, resident and
    on the host: beam_arrivals is the restatement on the fetched fan, and the list summed -- by the transfer function at one
    frequency, by the pulse with bandwidth 0 at every sample -- is beam_pressure_field, all bit for bit, without weights and
    with absorption and a loss pair"""
    env = {"munk": munk_env, "sloping": sloping_env, "munk-dropped": lambda p: munk_env(p, ztop=4200.0),
           "sloping-dropped": sloping_env_shallow_table}[which](pr)
    fan, eager = _shoot(pr, env, True), _shoot(pr, env, False)
    assert fan._dev._env.blocked_layout == which.startswith("sloping")
    assert (FAN_N - len(eager) > 20) == which.endswith("dropped") and len(eager) > 300 and len(fan) == len(eager)
    nb, ns = eager.bounce_counts(np.arange(FAN_S))
    d = DEPTHS[::20]
    loss = ([5.0, 30.0, 60.0], [0.5, 2.0, 6.0])
    B = pr.boundary_loss(eager, env, bottom_loss=loss, surface_loss=0.5, flatearth=False)
    W = pref.weights(pref.fan_path_integral(eager, env, FAN_PROFILE, False) + B)
    f = 25.0
    for w, curvature, kw in ((None, False, {}), (W, True, dict(absorption=FAN_PROFILE, bottom_loss=loss, surface_loss=0.5))):
        ref = ba.fan_beam_arrivals(eager, d, env, FAN_COLS, w_min=15.0, curvature=curvature, flatearth=False, W=w, nb=nb, ns=ns)
        # the preconditions of the identities below, from the restatement
        assert ba.no_subnormal_squares(ref["amplitude"]) and not np.isnan(ref["time"]).any() and len(ref["tube"]) > 1000
        args = dict(min_width=15.0, curvature=curvature, flatearth=False, **kw)
        field = pr.beam_pressure_field(fan, d, env, f, **args)[:, FAN_COLS]
        for rays in (fan, eager):
            a = pr.beam_arrivals(rays, d, env, range_indices=FAN_COLS, **args)
            got = dict(offsets=a.offsets, tube=a.tube, image=a.image, time=a.time, amplitude=a.amplitude, q=a.phase_index)
            _equal(got, ref)
            assert np.array_equal(a.range_indices, FAN_COLS) and _same(a.intensity, a.amplitude ** 2) and len(a) == len(ref["tube"])
            H = pr.beam_transfer_function(rays, d, env, [f], range_indices=FAN_COLS, **args)
            assert H.shape == (len(d), len(FAN_COLS), 1) and H.dtype == np.complex128 and _bits(H[:, :, 0], field)
            u = pr.beam_received_signal(rays, d, env, f, 0.0, 0.0, 0.5, 3, range_indices=FAN_COLS, **args)
            assert u.shape == (len(d), len(FAN_COLS), 3) and all(_bits(u[:, :, k], field) for k in range(3))
        assert np.isfinite(field).all() and (np.abs(field) > 0).mean() > 0.2
    _in_place(fan)
    if which == "munk":
        per = np.diff(ref["offsets"])
        print(f"Munk fan, {len(d)} receivers x {len(FAN_COLS)} ranges, min_width 15 m: {len(ref['tube'])} beam arrivals, "
              f"{per.min()} ... {per.max()} per receiver and range (mean {per.mean():.1f})")
        # the source's own column is NaN, as in beam_pressure_field, and has no arrivals
        H0 = pr.beam_transfer_function(fan, d, env, [f], range_indices=[0, -1], min_width=15.0, flatearth=False)
        a0 = pr.beam_arrivals(fan, d, env, range_indices=[0, -1], min_width=15.0, flatearth=False)
        assert np.isnan(H0[:, 0]).all() and not np.isnan(H0[:, 1]).any()
        assert (np.diff(a0.offsets).reshape(len(d), 2)[:, 0] == 0).all() and len(a0) > 0
        _in_place(fan)


@pytest.mark.parametrize("which", ["munk", "sloping-dropped"])
def test_absorption_that_follows_the_frequency_is_the_restated_sum_bit_for_bit(pr, which):
    """beam_transfer_function(absorption=thorp_absorption, t_reduce=x / 1500) of a resident and a host fan against
    spectrum_reference.spectrum_sum over the restated beam list with alpha and L_a: the path length of path_reference at
    (cols[c], tube) and (cols[c], tube + 1), formed as L_k + 0.5 (L_k+1 - L_k) in three operations.  The column list is unsorted
    and n = 3, so a slot-to-column map by // for %, a wrong weight or tube + 1 for tube would show.  With a surface loss, which
    stays in the tube weights while the volume absorption leaves them."""
    env = {"munk": munk_env, "sloping-dropped": sloping_env_shallow_table}[which](pr)
    fan, eager = _shoot(pr, env, True), _shoot(pr, env, False)
    nb, ns = eager.bounce_counts(np.arange(FAN_S))
    d, cols = DEPTHS[::50], np.asarray(FAN_COLS)
    R, n = len(d), len(cols)
    freq = np.array([1000.0, 20.0, 3000.0, 25.5])
    tred = np.asarray(eager.rs[0])[cols] / 1500.0
    B = pr.boundary_loss(eager, env, surface_loss=0.5, flatearth=False)
    a = ba.fan_beam_arrivals(eager, d, env, FAN_COLS, w_min=15.0, flatearth=False, W=pref.weights(B), nb=nb, ns=ns)
    assert ba.no_subnormal_squares(a["amplitude"]) and not np.isnan(a["time"]).any() and len(a["tube"]) > 300
    L = pref.fan_path_integral(eager, env, None, False)                             # (M, S): the path length
    col = cols[np.repeat(np.arange(R * n), np.diff(a["offsets"])) % n]
    L0, L1 = L[a["tube"], col], L[a["tube"] + 1, col]
    La = spref.arrival_lengths(L0, L1, 0.5)
    assert (L0 != L1).mean() > 0.9 and len(set(col)) == 3
    alpha = pr.thorp_absorption(freq) / 1000.0
    ref = spref.spectrum_sum(a["offsets"], a["time"], a["amplitude"] * a["amplitude"], a["q"], La, np.tile(tred, R), freq,
                             alpha).reshape(R, n, len(freq))
    kw = dict(range_indices=FAN_COLS, t_reduce=tred, min_width=15.0, flatearth=False, surface_loss=0.5)
    for rays in (fan, eager):
        H = pr.beam_transfer_function(rays, d, env, freq, absorption=pr.thorp_absorption, **kw)
        assert H.shape == ref.shape and _bits(H, ref)
    plain = pr.beam_transfer_function(fan, d, env, freq, **kw)
    # not vacuous: the absorption is there, and takes amplitude away
    assert not _bits(H, plain) and (np.abs(plain) > 0).mean() > 0.2 and np.abs(H[:, :, 2]).sum() < 0.9 * np.abs(plain[:, :, 2]).sum()
    _in_place(fan)


def test_arrivals_that_do_not_fit_are_refused_by_their_count(pr_any, monkeypatch):
    import torch
    env = munk_env(pr_any)
    fan = _shoot(pr_any, env, True, n=301, S=21, x1=40e3)
    d = DEPTHS[::100]
    total = len(pr_any.beam_arrivals(fan, d, env, min_width=15.0, flatearth=False))
    assert total > 10
    # 28 bytes per arrival; with a callable absorption 36 + 56 more and the fan's (S, M) path lengths
    for call, need in ((lambda: pr_any.beam_arrivals(fan, d, env, min_width=15.0, flatearth=False), 28 * total),
                       (lambda: pr_any.beam_transfer_function(fan, d, env, [50.0], min_width=15.0, flatearth=False,
                                                              absorption=pr_any.thorp_absorption),
                        92 * total + 8 * 21 * len(fan))):
        free = need - 1
        monkeypatch.setattr(torch.cuda, "mem_get_info", lambda *a, free=free: (free, 10 ** 12))
        with pytest.raises(ValueError, match=f"the {total} beam arrivals need {need} bytes of device memory and {free} are free"):
            call()
        monkeypatch.undo()
        call()                                                                      # ... and with the memory there is, it runs
    _in_place(fan)


def test_waveform_of_a_gaussian_source_is_beam_received_signal(pr_any):
    """tests/test_spectrum.py's synthesis identity for the beam pair, with that file's bound: SYNTH_REL times the sum of the
    group's amplitudes.  The source, the carrier and the windows are that test's."""
    env = munk_env(pr_any)
    fan = _shoot(pr_any, env, True)
    d, cols = DEPTHS[[100, 300, 500, 700]], [40, 17]
    f, B = 250.0, spref.SYNTH_B
    sigma = sref.pulse_sigma(B)
    dt = sigma / 4
    source, tc = spref.gaussian_source(sigma, dt)
    kw = dict(range_indices=cols, flatearth=False, surface_loss=0.5, min_width=15.0)
    a = pr_any.beam_arrivals(fan, d, env, **kw)
    n = len(cols)
    slot = np.repeat(np.arange(len(a.offsets) - 1), np.diff(a.offsets)) % n
    assert all((slot == c).sum() >= 4 for c in range(n)) and not np.isnan(a.time).any()
    windows = [spref.covering_fft(a.time[slot == c].min(), a.time[slot == c].max(), sigma, dt, len(source)) for c in range(n)]
    t0, n_fft = np.array([w[0] for w in windows]), max(w[1] for w in windows)
    assert n_fft <= 16384
    u = pr_any.beam_received_waveform(fan, d, env, source, dt, f, t0, n_fft=n_fft, **kw)
    ref = pr_any.beam_received_signal(fan, d, env, f, B, t0 - tc, dt, n_fft, **kw)
    assert u.shape == ref.shape == (len(d), n, n_fft) and u.dtype == np.complex128
    A = np.array([a.amplitude[a.offsets[g]:a.offsets[g + 1]].sum() for g in range(len(a.offsets) - 1)]).reshape(len(d), n)
    err = np.abs(u - ref).max(axis=2)
    lit = A > 0
    print(f"beam_received_waveform against beam_received_signal: worst |u - ref| is "
          f"{(err[lit] / (spref.SYNTH_REL * A[lit])).max():.3e} of the bound; n_fft {n_fft}, {len(a)} arrivals")
    assert (err <= spref.SYNTH_REL * A).all(), (err, A)
    assert lit.sum() >= 6 and (np.abs(ref).max(axis=2)[lit] > 1e6 * spref.SYNTH_REL * A[lit]).all()
    _in_place(fan)


# ---- physics on a HIP fan -------------------------------------------------------------------------------------------------------

def test_lloyds_mirror_with_a_pulse_from_shoot_rays(pr):
    env = cref.lloyd_env(pr)
    fan = pr.shoot_rays(bp.LLOYD_ZS, 0.0, np.linspace(-bp.EXACT_APERTURE, bp.EXACT_APERTURE, bp.EXACT_N), 5e3, 51, env,
                        flatearth=False, debug=False, device_resident=True, max_bounces=4)
    assert len(fan) == bp.EXACT_N and (fan.n_botts == 0).all() and fan.n_surfs.max() == 1
    cols = np.array([20, 30, 40, 50])
    x = np.asarray(fan.rs[0])[cols]
    assert np.array_equal(x, bp.EXACT_RANGES)
    u = pr.beam_received_signal(fan, bp.LLOYD_DEPTHS, env, ba.PULSE_F, ba.PULSE_B, x / bp.EXACT_C - sref.LLOYD_LEAD, sref.LLOYD_DT,
                                sref.LLOYD_NT, min_width=10.0, range_indices=cols, flatearth=False)
    _in_place(fan)
    e = ba.lloyd_pulse_error(u, x)
    print(f"Lloyd's mirror with a pulse from shoot_rays, min_width 10 m: worst e per range {[f'{v:.4e}' for v in e.max(axis=(0, 2))]}; "
          f"bound {ba.LLOYD_PULSE_BOUND:.4e}")
    assert np.abs(u).max() > 1e-4 and e.max() <= ba.LLOYD_PULSE_BOUND
