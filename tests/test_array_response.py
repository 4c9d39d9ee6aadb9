"""Vertical-array beamforming on the GPU (csrc/pgr_array.h): the kernel alone through ``_lib.array_response_sum`` against the
restatement of tests/array_reference.py on synthetic arrival lists aimed at its staging and tile seams, its identity with
``_lib.signal_device`` / ``signal_phi_device`` at one element, ``array_response`` and ``beam_array_response`` end to end on a
Munk fan (resident and host, with a complex bottom, against the restatement fed with the product's own arrival lists),
Lloyd's mirror seen by the array from ``shoot_rays``, and the error paths of the C entry."""
import ctypes

import numpy as np
import pytest

import array_reference as xref
import coherent_reference as cref
import signal_reference as sref
from test_array_response_host import check_lloyd_peaks
from tube_gpu import DEPTHS, _same, munk_env, pr, pr_any  # noqa: F401

pytestmark = pytest.mark.gpu

PAD = 130                    # entries before and behind an output that must stay as they were
MARK = -7.25
TILE = 256                   # SIG_TILE: the samples one wave handles
COUNTS = [200, 0, 65, 1, 63, 64]             # the staging seams


def _bits(a, b):
    return _same(a.real, b.real) and _same(a.imag, b.imag)


# ---- the kernel alone ---------------------------------------------------------------------------------------------------------

def synthetic_lists(R, n_cols, B, nt, dt, seed):
    """arrival lists of R x n_cols groups with counts from COUNTS (rotated by the seed: six groups hold all of them), a start
    time per column slot, arrivals before, after, on both ends of and inside each time axis, I over six decades with exact zeros
    and a NaN, q in -1 ... 9, lags of a few cycles, beyond +-1e3 cycles and one NaN, one NaN T; delays of 0, both signs and one
    that puts every arrival of its group far off the axis; weights with 0.0 and negative values"""
    rng = np.random.default_rng(seed)
    G = R * n_cols
    cnt = np.array([COUNTS[(g + seed) % len(COUNTS)] for g in range(G)])
    off = np.concatenate([[0], np.cumsum(cnt)]).astype(np.int64)
    n = int(off[-1])
    tstart = 60.0 + rng.uniform(-3.0, 3.0, n_cols)
    span = (nt - 1) * dt
    grp = np.repeat(np.arange(G), cnt)
    base = tstart[grp % n_cols]
    T = base + rng.uniform(-0.06, span + 0.06, n)
    edge = rng.random(n)
    T = np.where(edge < 0.08, base + rng.uniform(-0.004, 0.004, n), T)                        # straddling the first sample
    T = np.where(edge > 0.92, base + span + rng.uniform(-0.004, 0.004, n), T)                 # ... and the last
    T = T[np.lexsort((T, grp))]
    I = 10.0 ** rng.uniform(-12.0, -6.0, n)
    I[rng.random(n) < 0.05] = 0.0
    q = rng.integers(-1, 10, n).astype(np.int32)
    phi = rng.uniform(-2.0, 2.0, n)
    far = rng.random(n) < 0.1
    phi[far] = rng.choice([-1.0, 1.0], far.sum()) * rng.uniform(1e3, 1e6, far.sum())
    if n > 20:
        I[n // 3], phi[n // 2], T[(2 * n) // 3] = np.nan, np.nan, np.nan
        q[n // 2], q[(2 * n) // 3], q[n // 3] = 1, 0, 6                       # (so that the NaNs are not hidden behind q < 0)
    delay = rng.uniform(0.001, 0.03, (G, B))
    delay.reshape(-1)[1::2] *= -1.0                                           # both signs, whatever the seed
    delay[0, 0] = 0.0
    if G * B > 2:
        delay[-1, -1] = 7.0                                                   # every arrival of that group 7 s off the axis
    weight = np.array([0.8, 0.0, -0.6, 1.0, 0.3, -1.7])[(np.arange(G) + seed) % 6]
    return off, T, I, q, phi, delay, weight, tstart


def _upload(dev, a, dtype):
    import torch
    return torch.from_numpy(np.ascontiguousarray(a, dtype=dtype)).to(dev)


class _Call:
    """the device copies of one case's inputs and the C entry on them, with outputs guarded by PAD sentinels on both sides"""

    def __init__(self, off, T, I, q, phi, delay, weight, tstart, R, n_cols, f, rs, dt, nt):
        import torch
        from pygenray_amd import _lib
        self.torch, self.lib = torch, _lib
        self.dev = torch.device("cuda", 0)
        self.stream = torch.cuda.current_stream(self.dev).cuda_stream
        self.R, self.n_cols, self.B, self.nt = R, n_cols, delay.shape[1], nt
        self.size = n_cols * self.B * nt
        self.keep = [_upload(self.dev, off, np.int64), _upload(self.dev, np.append(T, 0.0), float),
                     _upload(self.dev, np.append(I, 0.0), float), None if q is None else _upload(self.dev, np.append(q, 0), np.int32),
                     None if phi is None else _upload(self.dev, np.append(phi, 0.0), float), _upload(self.dev, delay, float),
                     _upload(self.dev, weight, float), _upload(self.dev, tstart, float)]
        p = [0 if t is None else t.data_ptr() for t in self.keep]
        self.good = dict(off=p[0], R=R, n=n_cols, T=p[1], I=p[2], q=p[3], phi=p[4], delay=p[5], weight=p[6], ts=p[7], f=f, rs=rs,
                         dt=dt, nt=nt, B=self.B)

    def outputs(self):
        return [self.torch.full((self.size + 2 * PAD,), MARK, dtype=self.torch.float64, device=self.dev) for _ in range(2)]

    def raw(self, out, **kw):
        """the C entry itself -> its return code; `kw` replaces arguments (None: a null pointer)"""
        a = dict(self.good, re=out[0].data_ptr() + 8 * PAD, im=out[1].data_ptr() + 8 * PAD)
        a.update(kw)
        ptr = lambda v: None if not v else v   # noqa: E731
        return self.lib.load().pgr_array_response_device(
            0, ptr(a["off"]), a["R"], a["n"], ptr(a["T"]), ptr(a["I"]), ptr(a["q"]), ptr(a["phi"]), ptr(a["delay"]),
            ptr(a["weight"]), ptr(a["ts"]), a["f"], a["rs"], a["dt"], a["nt"], a["B"], ptr(a["re"]), ptr(a["im"]),
            ctypes.c_void_p(self.stream))

    def refusals(self, out):
        """every bad argument is refused, naming the entry and the argument, and `out` stays as it was"""
        L = self.lib.load()
        cases = [(dict(off=None), "null"), (dict(T=None), "null"), (dict(I=None), "null"), (dict(ts=None), "null"),
                 (dict(re=None), "null"), (dict(im=None), "null"), (dict(delay=None), "null"), (dict(weight=None), "null"),
                 (dict(R=0), "n_elements"), (dict(R=-2), "n_elements"), (dict(n=0), "n_cols"), (dict(n=-1), "n_cols"),
                 (dict(B=0), "n_looks"), (dict(B=-3), "n_looks"), (dict(n=2 ** 16, B=2 ** 15), "n_cols \\* n_looks"),
                 (dict(n=2 ** 31), "n_cols \\* n_looks"), (dict(B=2 ** 40), "n_cols \\* n_looks"), (dict(R=2 ** 31), "too many groups"),
                 (dict(R=2 ** 62), "too many groups"), (dict(nt=0), "n_times"), (dict(nt=-5), "n_times"),
                 (dict(nt=65535 * TILE + 1), "n_times"), (dict(f=-1.0), "frequency"), (dict(f=np.nan), "frequency"),
                 (dict(f=np.inf), "frequency"), (dict(rs=-1.0), "inv_sigma"), (dict(rs=np.nan), "inv_sigma"),
                 (dict(rs=np.inf), "inv_sigma"), (dict(dt=0.0), "dt"), (dict(dt=-1e-3), "dt"), (dict(dt=np.nan), "dt"),
                 (dict(dt=np.inf), "dt")]
        import re as regex
        for kw, msg in cases:
            rc = self.raw(out, **kw)
            err = L.pgr_last_error().decode()
            assert rc < 0 and "pgr_array_response_device" in err and regex.search(msg, err), (kw, rc, err)
        self.torch.cuda.synchronize(self.dev)
        assert all((a.cpu().numpy() == MARK).all() for a in out)

    def run(self, refusals=False):
        """-> y (n_cols, B, nt) complex through _lib.array_response_sum; the sentinels before and behind both outputs checked
        untouched and every entry between them checked written"""
        out = self.outputs()
        if refusals:
            self.refusals(out)
        g = self.good
        self.lib.array_response_sum(0, g["off"], g["R"], g["n"], g["T"], g["I"], g["q"], g["phi"], g["delay"], g["weight"], g["ts"],
                                    g["f"], g["rs"], g["dt"], g["nt"], g["B"], out[0].data_ptr() + 8 * PAD,
                                    out[1].data_ptr() + 8 * PAD, self.stream)
        h = [a.cpu().numpy() for a in out]
        for a in h:
            assert (a[:PAD] == MARK).all() and (a[PAD + self.size:] == MARK).all() and not (a[PAD:PAD + self.size] == MARK).any()
        return cref.as_complex(h[0][PAD:PAD + self.size], h[1][PAD:PAD + self.size]).reshape(self.n_cols, self.B, self.nt)


NT_CASES = [1, TILE - 1, TILE, TILE + 1]


@pytest.mark.parametrize("nt", NT_CASES)
@pytest.mark.parametrize("n_cols", [1, 2])
@pytest.mark.parametrize("B", [1, 3])
@pytest.mark.parametrize("R", [1, 2, 3])
def test_kernel_bit_identical_to_the_restatement_on_synthetic_lists(pr, R, B, n_cols, nt):
    dt, f = 1e-3, 75.0
    seed = 1000 * R + 100 * B + 10 * n_cols + NT_CASES.index(nt)
    off, T, I, q, phi, delay, weight, tstart = synthetic_lists(R, n_cols, B, nt, dt, seed)
    G = R * n_cols
    assert G < 6 or set(np.diff(off).tolist()) == set(COUNTS)
    assert delay[0, 0] == 0.0 and (delay < 0).any() == (G * B > 1) and (G * B <= 2 or delay[-1, -1] == 7.0)
    if off[-1] > 20:
        assert (q < 0).any() and (q > 3).any() and (I == 0).any() and np.isnan(I).any() and np.isnan(phi).any() and np.isnan(T).any()
        assert (np.abs(phi[np.isfinite(phi)]) > 1e3).any()
    got = {}
    for rs in (200.0, 0.0):                                            # sigma = 5 ms: windows of 80 samples; and CW
        # (at rs = 0 every arrival reaches every sample: the NaN intensity and the NaN lag would leave nothing else to compare)
        Iv, phiv = (I, phi) if rs else (np.nan_to_num(I, nan=1e-9), np.nan_to_num(phi, nan=0.3))
        for name, qq, lag in (("all", q, phiv), ("q", q, None), ("null", None, None)):
            call = _Call(off, T, Iv, qq, lag, delay, weight, tstart, R, n_cols, f, rs, dt, nt)
            y = got[rs, name] = call.run(refusals=(name == "all"))
            ref = xref.array_sum(off, T, Iv, qq, lag, delay, weight, tstart, R, n_cols, f, rs, dt, nt)
            assert rs or not np.isnan(ref.real).any()
            bad = np.argwhere(~((y.real == ref.real) | (np.isnan(y.real) & np.isnan(ref.real))))
            assert y.shape == (n_cols, B, nt) and _bits(y, ref), (rs, name, bad[:5])
            assert _bits(call.run(), y)                                  # repeated calls are bit-equal
    if G * B > 2 and off[-2] < off[-1]:
        # the look 7 s away holds nothing of its (last) element at a finite pulse: for one element it is all zero
        last = got[200.0, "null"][n_cols - 1, B - 1]
        assert R > 1 or (last == 0).all()
    if off[-1] > 100 and nt >= TILE - 1:
        u = got[200.0, "q"]
        assert (np.nan_to_num(np.abs(u)) > 0).any() and not _bits(got[200.0, "q"], got[200.0, "null"])      # q matters
        assert not _bits(got[200.0, "q"], got[200.0, "all"])                                             # ... and phi


def test_one_element_without_delay_or_weight_is_the_signal_kernel_bit_for_bit(pr):
    import torch
    from pygenray_amd import _lib
    dt, f, nt, G, B = 1e-3, 75.0, TILE + 1, 6, 2
    off, T, I, q, phi, _, _, tstart = synthetic_lists(1, G, B, nt, dt, seed=7)
    phi = np.nan_to_num(phi)
    assert set(np.diff(off).tolist()) == set(COUNTS)
    for rs in (200.0, 0.0):
        for qq, lag in ((q, None), (None, None), (q, phi)):
            c = _Call(off, T, I, qq, lag, np.zeros((G, B)), np.ones(G), tstart, 1, G, f, rs, dt, nt)
            y = c.run()
            re, im = (torch.full((G * nt,), MARK, dtype=torch.float64, device=c.dev) for _ in range(2))
            g = c.good
            if lag is None:
                _lib.signal_device(0, g["off"], G, g["T"], g["I"], g["q"], g["ts"], f, rs, dt, nt, re.data_ptr(), im.data_ptr(),
                                   c.stream)
            else:
                _lib.signal_phi_device(0, g["off"], G, g["T"], g["I"], g["q"], g["phi"], g["ts"], f, rs, dt, nt, re.data_ptr(),
                                       im.data_ptr(), c.stream)
            u = cref.as_complex(re.cpu().numpy(), im.cpu().numpy()).reshape(G, nt)
            assert all(_bits(y[:, b], u) for b in range(B)) and (np.nan_to_num(np.abs(u)) > 0).any()


# ---- fans -----------------------------------------------------------------------------------------------------------------

SAND = (1700.0, 1800.0, 0.5)
ELEMENTS = DEPTHS[[300, 305, 310, 315, 320]]                      # five elements 30 m apart around 1.67 km
LOOKS = np.array([-12.0, -8.0, -3.0, 0.0, 2.5, 9.0, 14.0])
COLS = [100, 37]
SPEEDS = [1500.0, 1492.0]
F, BW, DT, NT = 75.0, 20.0, 2e-3, 512


def _shoot(pr, env, resident):
    return pr.shoot_rays(1000.0, 0.0, np.linspace(-20.0, 20.0, 2001), 100e3, 101, env, flatearth=False, debug=False,
                         device_resident=resident, max_bounces=64)


def _in_place(fan):
    assert fan.device_resident and not any(k in fan.__dict__ for k in ("_ts", "_zs", "_ps"))


@pytest.fixture(scope="module")
def munk_fan(pr):
    """a 2001-ray Munk fan to 100 km with a bounce log of 64 slots, device resident and the same fan on the host; the tube
    arrivals at the five elements and two columns, and a start time per column in the thick of them"""
    env = munk_env(pr)
    fan, eager = _shoot(pr, env, True), _shoot(pr, env, False)
    a = pr.arrivals(fan, ELEMENTS, env, flatearth=False, range_indices=COLS)
    slot = np.repeat(np.arange(len(a.offsets) - 1), np.diff(a.offsets)) % len(COLS)
    t0 = np.array([np.median(a.time[slot == c]) - 0.5 * NT * DT for c in range(len(COLS))])
    return fan, eager, env, t0


def _tube_lists(pr, fan, env, **kw):
    """(offsets, T, I, q, phi or None) of the tube arrivals at the elements, from the product's own arrivals, caustic index and
    bounce counts (tests/test_reflection.py's recipe)"""
    a = pr.arrivals(fan, ELEMENTS, env, flatearth=False, range_indices=COLS, **kw)
    slot = np.repeat(np.arange(len(a.offsets) - 1), np.diff(a.offsets)) % len(COLS)
    kappa = pr.caustic_index(fan, env, flatearth=False)
    nb, ns = fan.bounce_counts(COLS)
    alike = (nb[a.tube, slot] == nb[a.tube + 1, slot]) & (ns[a.tube, slot] == ns[a.tube + 1, slot])
    q = np.where(alike, kappa[a.tube, np.asarray(COLS)[slot]] + 2 * ns[a.tube, slot], -1)
    return a.offsets, a.time, a.intensity, q, a.bottom_phase


def _restated(lists, t0, shading=None):
    off, T, I, q, phi = lists
    R, n = len(ELEMENTS), len(COLS)
    delay = np.stack([xref.group_layout(pr_steer(c), 1) for c in SPEEDS], axis=1).reshape(R * n, len(LOOKS))
    w = np.full(R, 1.0 / R) if shading is None else np.asarray(shading, dtype=float)
    return xref.array_sum(off, T, I, q, phi, delay, xref.group_layout(w, n), t0, R, n, F, sref.inv_sigma(BW), DT, NT)


def pr_steer(c):
    import pygenray_amd
    return pygenray_amd.steering_delays(ELEMENTS, LOOKS, c)


def test_array_response_on_a_munk_fan_resident_and_host_against_the_restatement(pr, munk_fan):
    fan, eager, env, t0 = munk_fan
    shade = [0.1, 0.25, 0.3, 0.25, 0.1]
    for kw, shading in ((dict(), None), (dict(bottom_loss=pr.fluid_halfspace(*SAND)), shade),
                        (dict(absorption=0.05, surface_loss=0.5), shade)):
        args = (ELEMENTS, env, LOOKS, F, BW, t0, DT, NT)
        opt = dict(range_indices=COLS, sound_speed=SPEEDS, shading=shading, flatearth=False, **kw)
        y = pr.array_response(fan, *args, **opt)
        assert y.shape == (len(COLS), len(LOOKS), NT) and y.dtype == np.complex128
        _in_place(fan)
        assert _bits(pr.array_response(eager, *args, **opt), y) and _bits(pr.array_response(fan, *args, **opt), y)
        lists = _tube_lists(pr, fan, env, **kw)
        assert (lists[4] is not None) == ("bottom_loss" in kw) and len(lists[1]) >= 50
        assert _bits(y, _restated(lists, t0, shading))
        assert (np.abs(y).max(axis=2) > 0).all() and not _bits(y[:, 0], y[:, 3])
    _in_place(fan)
    # the complex bottom's phase matters
    rigid = pr.array_response(fan, *args, **dict(opt, bottom_loss=pr.fluid_halfspace(*SAND).loss, absorption=None, surface_loss=None))
    sand = pr.array_response(fan, *args, **dict(opt, bottom_loss=pr.fluid_halfspace(*SAND), absorption=None, surface_loss=None))
    assert not _bits(rigid, sand)


def test_one_element_looking_broadside_is_received_signal_bit_for_bit(pr, munk_fan):
    fan, eager, env, t0 = munk_fan
    for kw in (dict(), dict(bottom_loss=pr.fluid_halfspace(*SAND), surface_loss=0.5)):
        for d in ELEMENTS[[0, 3]]:
            u = pr.received_signal(fan, [d], env, F, BW, t0, DT, NT, range_indices=COLS, flatearth=False, **kw)
            y = pr.array_response(fan, [d], env, [0.0], F, BW, t0, DT, NT, range_indices=COLS, shading=[1.0], flatearth=False, **kw)
            assert y.shape == (len(COLS), 1, NT) and _bits(y[:, 0], u[0]) and (np.abs(u) > 0).any()
    _in_place(fan)


def test_default_sound_speed_is_the_table_at_the_reference_depth_and_the_source_column_is_nan(pr, munk_fan):
    fan, eager, env, t0 = munk_fan
    from pygenray_amd.environment import _unpack_envi
    cin, _, rin, zin = _unpack_envi(env, flatearth=False)[:4]
    x = np.asarray(eager.rs[0])[COLS]
    for dref in (None, 1500.0):
        at = float(np.mean(ELEMENTS)) if dref is None else dref
        c = [pr.bilinear_interp(float(xc), at, rin, zin, cin) for xc in x]
        assert 1480.0 < min(c) and max(c) < 1560.0
        args = (ELEMENTS, env, LOOKS, F, BW, t0, DT, 64)
        y = pr.array_response(fan, *args, range_indices=COLS, reference_depth=dref, flatearth=False)
        assert _bits(y, pr.array_response(fan, *args, range_indices=COLS, reference_depth=dref, sound_speed=c, flatearth=False))
    y = pr.array_response(fan, ELEMENTS, env, LOOKS, F, BW, 0.0, DT, 3, range_indices=[0, -1], flatearth=False)
    assert np.isnan(y[0]).all() and not np.isnan(y[1]).any()
    one = pr.array_response(fan, ELEMENTS, env, LOOKS, F, BW, t0[0], DT, 3, flatearth=False)          # the last column by default
    assert one.shape == (1, len(LOOKS), 3)
    with pytest.raises(ValueError, match="bytes of device memory"):
        pr.array_response(fan, ELEMENTS, env, np.linspace(-90.0, 90.0, 20000), F, BW, 0.0, DT, 65535 * 256, range_indices=COLS,
                          flatearth=False)
    _in_place(fan)


def test_beam_array_response_against_the_restatement_fed_with_beam_arrivals(pr, munk_fan):
    fan, eager, env, t0 = munk_fan
    for kw in (dict(), dict(min_width=25.0, curvature=False, surface_loss=0.5)):
        args = (ELEMENTS, env, LOOKS, F, BW, t0, DT, NT)
        y = pr.beam_array_response(fan, *args, range_indices=COLS, sound_speed=SPEEDS, flatearth=False, **kw)
        assert _bits(pr.beam_array_response(eager, *args, range_indices=COLS, sound_speed=SPEEDS, flatearth=False, **kw), y)
        b = pr.beam_arrivals(fan, ELEMENTS, env, range_indices=COLS, flatearth=False, **kw)
        assert len(b) > 100
        ref = _restated((b.offsets, b.time, b.amplitude * b.amplitude, b.phase_index, None), t0)
        assert y.shape == ref.shape and _bits(y, ref) and (np.abs(y).max(axis=2) > 0).all()
    _in_place(fan)
    with pytest.raises(ValueError, match="does not yet apply a complex bottom phase"):
        pr.beam_array_response(fan, *args, bottom_loss=pr.fluid_halfspace(*SAND), flatearth=False)


# ---- Lloyd's mirror seen by the array -----------------------------------------------------------------------------------------

def test_lloyds_mirror_on_the_array_end_to_end(pr):
    import beam_pressure_reference as bp
    env = cref.lloyd_env(pr)
    fan = pr.shoot_rays(xref.ARRAY_ZS, 0.0, np.linspace(-bp.EXACT_APERTURE, bp.EXACT_APERTURE, bp.EXACT_N), xref.ARRAY_X, 11, env,
                        flatearth=False, debug=False, device_resident=True, max_bounces=4)
    assert len(fan) == bp.EXACT_N and (fan.n_botts == 0).all() and fan.n_surfs.max() == 1
    R = len(xref.ARRAY_DEPTHS)
    y = pr.array_response(fan, xref.ARRAY_DEPTHS, env, xref.ARRAY_LOOKS, xref.ARRAY_F, xref.ARRAY_B, xref.array_t0(), xref.ARRAY_DT,
                          xref.ARRAY_NT, sound_speed=xref.ARRAY_C, flatearth=False)[0]
    _in_place(fan)
    delta, w = pr.steering_delays(xref.ARRAY_DEPTHS, xref.ARRAY_LOOKS, xref.ARRAY_C), np.full(R, 1.0 / R)
    e = xref.array_error(y, w, delta)
    b, m = np.unravel_index(np.argmax(e), e.shape)
    print(f"Lloyd's mirror on the array from shoot_rays: worst e {e.max():.6e} at look {xref.ARRAY_LOOKS[b]} degrees, sample {m}; "
          f"bound {xref.ARRAY_BOUND:.6e}")
    assert e.max() <= xref.ARRAY_BOUND < 0.01
    centre = pr.arrivals(fan, xref.ARRAY_DEPTHS, env, flatearth=False).at(R // 2, 0)
    assert len(centre["time"]) == 2
    check_lloyd_peaks(y, w, delta, centre["received_angle"][np.argsort(centre["time"])])
    # the table's own sound speed is the same 1500 m/s: the default gives the same response
    assert _bits(y, pr.array_response(fan, xref.ARRAY_DEPTHS, env, xref.ARRAY_LOOKS, xref.ARRAY_F, xref.ARRAY_B, xref.array_t0(),
                                      xref.ARRAY_DT, xref.ARRAY_NT, flatearth=False)[0])
