"""What arrives in the caller's NumPy arrays: the last stretch between a trajectory in HBM and the host, at size.

csrc/pgr_transfer.h (d2h_pipelined, squeeze_rows, pgr_gather_cols, pgr_unblock_cols) serves both host entries,
pgr_shoot_fan (EnvHandle.shoot_fan, eager pr.shoot_rays) and pgr_fan_fetch_samples (FanHandle.fetch_samples, RayFan.zs /
to_host() of a device-resident fan).  From 32 MB in all on, every array is cut into sub-jobs of 128 MiB, helper threads fault
the caller's pages in 16 MiB pieces and page-lock each sub-job, and after the kernel the sub-jobs are re-sourced and
shortened (compaction shrinks [S][N] to [S][M], un-blocking replaces the source by a scratch buffer).  This file looks at
arrays of three sub-jobs, at shortened and emptied sub-jobs, at both squeeze kernels on both paths, at both entries, at
the threshold, and at the piecewise copies a failed page-lock falls back to (PGR_OPT_D2H_REGISTER 0).

The reference never passes through pgr_transfer.h: the same fan run as a DeviceFan in plain [S][N] rows (the row kernel,
whatever the environment) and read with torch; `ref[:, keep]` in NumPy for compacted cases, `-z`, `-p` for the stored
sign (negation is exact).  One large case ties that reference to the CPU oracle, every sample of every ray.  Every
comparison is np.array_equal(..., equal_nan=True) over whole arrays: bit equality, no tolerance in this file.
"""
import ctypes
import os
import re

import numpy as np
import pytest

import oracle
from helpers import munk_arrays, y0_for

pytestmark = pytest.mark.gpu

# pygenray_amd/csrc/pgr_transfer.h: d2h_pipelined's kSub, OrderedPrefault::kPiece, and the total below which the copy is a
# plain hipMemcpyAsync per array (test_constants_mirror_the_source keeps the three in step with the source)
SUB_JOB = 128 << 20
PIECE = 16 << 20
PIPELINED_FROM = 32 << 20

SENTINEL = float.fromhex("0x1.d23456789abcdp+2")   # (7.28...: no byte of it is zero or repeated, so a stray byte written into it shows)
X1 = 100e3
N_BIG, S_BIG = 70_000, 601             # 336.56 MB per array: 134.2 + 134.2 + 68.1 MB
VERTICAL = 89.9999                     # launch angle of a placed drop (status 1, PGR_RAY_VERTICAL)
# The kept rays' launch angles: three bands in which neither environment drops a ray -- +-13 degrees (refracted, no boundary
# touched) and 15.2 .. 16 degrees either way (bouncing off surface and bottom); the angles between graze a boundary
# (surface 14.2 .. 14.4, bottom 14.7 degrees) and some of those rays leave the table.
BANDS = ((-13.0, 13.0), (15.2, 16.0), (-16.0, -15.2))


@pytest.fixture(scope="module")
def lib():
    from pygenray_amd import _lib
    if _lib.ARITH != "reference":
        pytest.skip("the row reference and the oracle anchor are bit comparisons of the reference arithmetic")
    _lib.load()
    assert _lib.device_count() >= 1
    return _lib


# ------------------------------------------------------------------ the situation a case means to be in, from the constants
def sub_jobs(nbytes):
    """Sizes of the sub-jobs d2h_pipelined cuts an array of `nbytes` into."""
    return [min(SUB_JOB, nbytes - o) for o in range(0, nbytes, SUB_JOB)]


def live_sub_jobs(nbytes, written):
    """... and what is left of each when only the first `written` bytes of the array are copied (the `live` loop)."""
    out, o = [], 0
    for b in sub_jobs(nbytes):
        out.append(0 if o >= written else min(b, written - o))
        o += b
    return out


def pipelined(n_arrays, N, S):
    return n_arrays * N * S * 8 >= PIPELINED_FROM


def same(a, b):
    return a.shape == b.shape and a.dtype == b.dtype and np.array_equal(a, b, equal_nan=True)


# ------------------------------------------------------------------ environments, drop patterns, the row reference
def lds_arrays():
    return munk_arrays(X1)                                      # range independent, full-depth table: LDS-table row kernel


def hbm_arrays():
    return munk_arrays(X1, nr=21, sofar_slope=5e-4)             # range dependent: table in HBM / L2, sample-blocked API kernel


ENVS = {"lds": lds_arrays, "hbm": hbm_arrays}


def make_env(lib, kind):
    arrs = ENVS[kind]()
    env = lib.EnvHandle(*arrs)
    assert env.lds_path == (kind == "lds") and env.blocked_layout == (kind == "hbm"), kind
    return env, arrs


def placed_drops(N, count, seed=20240):
    """Indices of `count` rays to drop, placed where a squeeze goes wrong first: ray 0 and ray N - 1, both sides of multiples
    of 64 (a wave) and 256 (a workgroup of the squeeze kernels), one long run, and a scattered random set making up the count."""
    if count == 0:
        return np.zeros(0, np.int64)
    if count == 1:
        return np.array([0], np.int64)
    assert N >= 20_000 and 40 <= count < N
    edge = [0, N - 1]
    for m in (64, 256, 64 * (N // 150), 256 * (N // 700), 64 * (N // 64), 256 * (N // 256)):
        edge += [m - 1, m, m + 1] if m + 1 < N else [m - 1]
    start = 3 * N // 7
    run = list(range(start, start + min(5000, count // 4)))
    chosen = np.unique(np.array(edge + run, np.int64))
    assert len(chosen) <= count
    rest = np.setdiff1d(np.arange(N), chosen)
    extra = np.random.default_rng(seed).choice(rest, size=count - len(chosen), replace=False)
    drops = np.unique(np.concatenate([chosen, extra]))
    assert len(drops) == count
    return drops


def fan_angles(N, drops):
    if N == 1:
        th = np.array([3.0])
    else:
        n_b = N // 5
        th = np.concatenate([np.linspace(*BANDS[0], N - 2 * n_b), np.linspace(*BANDS[1], n_b), np.linspace(*BANDS[2], n_b)])
    th[np.asarray(drops, np.int64)] = VERTICAL
    return th


def row_reference(lib, env, y0, S, exact_samples=False, x1=X1):
    """The fan as a DeviceFan in plain [S][N] rows, read with torch: T, z, p (S, N) and the per-ray arrays."""
    import torch
    from pygenray_amd.device_fan import DeviceFan
    fan = DeviceFan(env, y0, 0.0, x1, S, save=True, sample_major=True, sample_blocked=False, exact_samples=exact_samples)
    assert not fan.sample_blocked and tuple(fan.T.shape) == (S, len(y0))
    fan.run()
    torch.cuda.synchronize()
    out = {k: t.cpu().numpy() for k, t in (("T", fan.T), ("z", fan.Z), ("p", fan.P), ("end", fan.end), ("n_bott", fan.n_bott),
                                           ("n_surf", fan.n_surf), ("status", fan.status), ("n_steps", fan.n_steps),
                                           ("n_rej", fan.n_rej))}
    del fan
    torch.cuda.empty_cache()
    return out


def expect_keep(ref, N, drops):
    """keep = status == 0 is exactly the complement of the placed rays, and they are dropped as vertical."""
    keep = ref["status"] == 0
    want = np.ones(N, bool)
    want[np.asarray(drops, np.int64)] = False
    assert np.array_equal(keep, want), f"{int((keep != want).sum())} rays dropped or kept against the plan"
    assert np.all(ref["status"][~want] == 1)
    return keep


def expected_samples(ref, keep, compact, stored_sign):
    """name -> the (S, M) array the caller must get."""
    out = {}
    for k in "Tzp":
        a = ref[k][:, keep] if compact and not keep.all() else ref[k]
        out[k] = -a if (stored_sign and k != "T") else a
    return out


def check_shoot_fan(env, y0, S, ref, keep, compact, stored_sign, label):
    """EnvHandle.shoot_fan(sample_major=True) into sentinel-filled caller buffers: T, z, p and the per-ray arrays against the
    row reference, and everything beyond S * M doubles still the sentinel in all three buffers."""
    N = len(y0)
    M = int(keep.sum()) if compact else N
    bufs = [np.full((S, N), SENTINEL) for _ in range(3)]
    out = env.shoot_fan(y0, 0.0, X1, S, sample_major=True, compact=compact, stored_sign=stored_sign, buffers=bufs)
    for k in ("end", "n_bott", "n_surf", "status", "n_steps", "n_rej"):
        assert same(out[k], ref[k]), (label, k)
    want = expected_samples(ref, keep, compact, stored_sign)
    for k in "Tzp":
        assert out[k].shape == (S, M), (label, k, out[k].shape)
        assert same(out[k], want[k]), (label, k)
    for name, b in zip("Tzp", bufs):
        flat = b.reshape(-1)
        if M > 0:
            assert np.shares_memory(out[name], b) and out[name].ctypes.data == b.ctypes.data, (label, name)
        assert np.all(flat[S * M:] == SENTINEL), (label, name, "the tail of the caller's buffer was written")


def check_fan_handle(lib, env, y0, S, ref, keep, label, rounds=True):
    """FanHandle (stored sign, as RayFan launches it): all three arrays, then z alone, then all three again (the scratch is
    grow-only and sized by the arrays of the call: one, then three), compact and not; the same fetch twice gives the same
    bits; one call through pgr_fan_fetch_samples itself with sentinel-filled buffers for the untouched tail."""
    N = len(y0)
    M = int(keep.sum())
    h = lib.FanHandle(env, 0.0, X1, S, y0=y0, stored_sign=True)
    assert h.wait() == (N, M)
    rays = h.fetch_rays()
    for k in ("end", "n_bott", "n_surf", "status", "n_steps", "n_rej"):
        assert same(rays[k], ref[k]), (label, k)
    for compact in (True, False):
        want = expected_samples(ref, keep, compact, True)
        cols = M if compact else N
        first = h.fetch_samples(compact=compact)
        for k in "Tzp":
            assert first[k].shape == (S, cols) and same(first[k], want[k]), (label, compact, k)
        only_z = h.fetch_samples(("z",), compact=compact)
        assert list(only_z) == ["z"] and same(only_z["z"], want["z"]), (label, compact, "z alone")
        if rounds:
            again = h.fetch_samples(compact=compact)
            for k in "Tzp":
                assert same(again[k], first[k]) and same(again[k], want[k]), (label, compact, k, "second fetch")
            del again
        del first, only_z
    # the C entry itself, caller-owned buffers
    want = expected_samples(ref, keep, True, True)
    bufs = [np.full((S, N), SENTINEL) for _ in range(3)]
    vp = lambda a: ctypes.c_void_p(a.ctypes.data)   # noqa: E731
    lib.check(lib.load().pgr_fan_fetch_samples(h._h, vp(bufs[0]), vp(bufs[1]), vp(bufs[2]), lib.PGR_COMPACT))
    for name, b in zip("Tzp", bufs):
        flat = b.reshape(-1)
        assert same(flat[:S * M].reshape(S, M), want[name]), (label, name, "pgr_fan_fetch_samples")
        assert np.all(flat[S * M:] == SENTINEL), (label, name, "the tail of the caller's buffer was written")
    h.close()


# ------------------------------------------------------------------ the constants
def test_constants_mirror_the_source(lib):
    """SUB_JOB, PIECE and PIPELINED_FROM above are pgr_transfer.h's: a change there fails here instead of turning the large
    cases into small-path tests silently."""
    with open(os.path.join(lib.CSRC, "pgr_transfer.h")) as f:
        src = f.read()
    shift = lambda pat: [int(a) << int(b) for a, b in re.findall(pat, src)]   # noqa: E731
    assert shift(r"kSub = \(size_t\)(\d+) << (\d+);") == [SUB_JOB]
    assert shift(r"kPiece = \(size_t\)(\d+) << (\d+);") == [PIECE]
    assert shift(r"if \(total < \(\(size_t\)(\d+) << (\d+)\)\)") == [PIPELINED_FROM]
    # the big shape: three sub-jobs per array, the last one partial and not a whole number of pieces
    per_array = N_BIG * S_BIG * 8
    assert [b for b in sub_jobs(per_array)] == [SUB_JOB, SUB_JOB, per_array - 2 * SUB_JOB]
    assert 0 < per_array - 2 * SUB_JOB < SUB_JOB and per_array % PIECE != 0 and pipelined(1, N_BIG, S_BIG)


# ------------------------------------------------------------------ the large cases
# name -> number of placed drops.  M = N - drops.
BIG_PATTERNS = {
    "nothing dropped": 0,                     # 3 full sub-jobs per array, 9 in all; compact requested: nothing to squeeze
    "ends in the second sub-job": 28_001,     # M = 41 999: third sub-job emptied, second shortened
    "less than one sub-job": 49_999,          # M = 20 001: second and third emptied
    "one ray dropped": 1,                     # M = N - 1
}


def big_situation(name):
    drops = placed_drops(N_BIG, BIG_PATTERNS[name])
    M = N_BIG - len(drops)
    per_array, rows = N_BIG * S_BIG * 8, M * S_BIG * 8
    live = live_sub_jobs(per_array, rows)
    assert len(sub_jobs(per_array)) == 3 and pipelined(3, N_BIG, S_BIG)
    if name == "nothing dropped":
        assert M == N_BIG and live == sub_jobs(per_array) and 3 * len(live) == 9
    elif name == "ends in the second sub-job":
        assert live[0] == SUB_JOB and 0 < live[1] < SUB_JOB and live[2] == 0
    elif name == "less than one sub-job":
        assert 0 < live[0] < SUB_JOB and live[1] == 0 and live[2] == 0
    else:
        assert M == N_BIG - 1 and live[0] == live[1] == SUB_JOB and 0 < live[2] < sub_jobs(per_array)[2]
    if 0 < M < N_BIG:
        # the squeezed rows of one array are not a multiple of squeeze_rows' 256-byte pieces: the second and third array
        # sit at a * piece, not a * rows, in the scratch; and not a whole number of 16 MiB prefault pieces
        assert rows % 256 != 0 and rows % PIECE != 0
    return drops, M


@pytest.mark.parametrize("pattern", list(BIG_PATTERNS))
@pytest.mark.parametrize("kind", ["lds", "hbm"])
def test_large_fans_through_the_host_pointer_entry(lib, kind, pattern):
    """pgr_shoot_fan at three sub-jobs per array: no compaction, compaction that shortens / empties later sub-jobs, one ray
    or none to squeeze; stored sign on and off; the HBM-table environment through the sample-blocked kernel + un-blocking
    (PGR_OPT_API_BLOCKED 1, the default) and through plain rows (0).  Caller buffers keep the sentinel beyond S * M."""
    drops, M = big_situation(pattern)
    env, arrs = make_env(lib, kind)
    y0 = y0_for(oracle, arrs, 1000.0, 0.0, fan_angles(N_BIG, drops))
    ref = row_reference(lib, env, y0, S_BIG)
    keep = expect_keep(ref, N_BIG, drops)
    assert int(keep.sum()) == M and (0 < M < N_BIG or len(drops) == 0)
    assert (ref["n_bott"][keep] > 0).any() and (ref["n_surf"][keep] > 0).any()
    for api_blocked in ((1, 0) if kind == "hbm" else (1,)):
        env.set_option("api_blocked", api_blocked)
        assert env.blocked_layout == (kind == "hbm" and api_blocked == 1)
        label = f"{kind}, {pattern}, api_blocked {api_blocked}"
        check_shoot_fan(env, y0, S_BIG, ref, keep, compact=True, stored_sign=bool(api_blocked), label=label + ", compact")
        if len(drops) <= 1:
            # (not compacted: dropped rays stay as NaN columns; the full three sub-jobs of every array)
            check_shoot_fan(env, y0, S_BIG, ref, keep, compact=False, stored_sign=not api_blocked, label=label + ", full")
    env.close()


def test_large_fan_ray_major_output(lib):
    """Ray-major output (N, S) at the same size: the straight copy through the pipelined path."""
    drops, _ = big_situation("one ray dropped")
    env, arrs = make_env(lib, "lds")
    y0 = y0_for(oracle, arrs, 1000.0, 0.0, fan_angles(N_BIG, drops))
    ref = row_reference(lib, env, y0, S_BIG)
    expect_keep(ref, N_BIG, drops)
    bufs = [np.full((N_BIG, S_BIG), SENTINEL) for _ in range(3)]
    out = env.shoot_fan(y0, 0.0, X1, S_BIG, sample_major=False, buffers=bufs)
    for k in "Tzp":
        assert out[k] is bufs["Tzp".index(k)] and same(out[k], np.ascontiguousarray(ref[k].T)), k
    for k in ("end", "n_bott", "n_surf", "status", "n_steps", "n_rej"):
        assert same(out[k], ref[k]), k
    env.close()


def test_large_fan_every_sample_against_the_oracle(lib):
    """The anchor outside the library: an LDS-table environment, PGR_EXACT_SAMPLES, three sub-jobs per array -- every sample
    of every ray that pgr_shoot_fan delivers equals the CPU oracle's (correctly rounded libm), and so does the torch-read row
    reference the other cases compare with."""
    drops = placed_drops(N_BIG, 40)
    env, arrs = make_env(lib, "lds")
    y0 = y0_for(oracle, arrs, 1000.0, 0.0, fan_angles(N_BIG, drops))
    assert len(sub_jobs(N_BIG * S_BIG * 8)) == 3
    got = env.shoot_fan(y0, 0.0, X1, S_BIG, sample_major=True, exact_samples=True)
    ref = row_reference(lib, env, y0, S_BIG, exact_samples=True)
    o = oracle.shoot_fan(*arrs, y0, 0.0, X1, S_BIG, math=oracle.MATH_CR)
    keep = expect_keep(ref, N_BIG, drops)
    assert same(got["status"], o["status"].astype(np.int32)) and same(ref["status"], got["status"])
    assert (o["n_bott"][keep] > 0).sum() > 1000 and (o["n_surf"][keep] > 0).sum() > 1000
    for k in "Tzp":
        want = np.ascontiguousarray(o[k].T)
        assert same(got[k], want), (k, "pgr_shoot_fan against the oracle")
        assert same(ref[k], want), (k, "torch-read row reference against the oracle")
    for k in ("n_bott", "n_surf", "n_steps", "n_rej"):
        assert np.array_equal(got[k][keep], o[k][keep]) and same(got[k], ref[k]), k
    end = np.stack([o["T"][:, -1], o["z"][:, -1], o["p"][:, -1]], 1)
    assert same(got["end"][keep], end[keep]) and same(got["end"], ref["end"])
    env.close()


@pytest.mark.parametrize("kind", ["lds", "hbm"])
def test_large_fan_handles_fetch_what_the_row_reference_holds(lib, kind):
    """pgr_fan_fetch_samples above 32 MB: three arrays (nine sub-jobs, the later ones shortened and emptied by the
    compaction), one array, three again; compact and full; blocked and row layout."""
    drops, M = big_situation("ends in the second sub-job")
    env, arrs = make_env(lib, kind)
    y0 = y0_for(oracle, arrs, 1000.0, 0.0, fan_angles(N_BIG, drops))
    ref = row_reference(lib, env, y0, S_BIG)
    keep = expect_keep(ref, N_BIG, drops)
    assert pipelined(1, N_BIG, S_BIG)             # (a fetch of one array is on the pipelined path too)
    for api_blocked in ((1, 0) if kind == "hbm" else (1,)):
        env.set_option("api_blocked", api_blocked)
        assert env.blocked_layout == (kind == "hbm" and api_blocked == 1)
        check_fan_handle(lib, env, y0, S_BIG, ref, keep, f"{kind}, api_blocked {api_blocked}", rounds=bool(api_blocked))
    env.close()


@pytest.mark.parametrize("kind", ["lds", "hbm"])
def test_large_fans_without_page_locking(lib, kind):
    """PGR_OPT_D2H_REGISTER 0: no sub-job is page-locked, each goes out piece by piece as after a failed hipHostRegister
    (what a process under a locked-memory limit gets) -- the same arrays through both entries, the same untouched tails."""
    drops, M = big_situation("ends in the second sub-job")
    env, arrs = make_env(lib, kind)
    y0 = y0_for(oracle, arrs, 1000.0, 0.0, fan_angles(N_BIG, drops))
    ref = row_reference(lib, env, y0, S_BIG)
    keep = expect_keep(ref, N_BIG, drops)
    with pytest.raises(lib.PgrError):
        env.set_option("d2h_register", 2)
    env.set_option("d2h_register", 0)
    # a sub-job of 128 MiB takes several pieces, and the pieces straddle the arrays (a piece is not a divisor of an array)
    assert SUB_JOB // PIECE > 1 and (N_BIG * S_BIG * 8) % PIECE != 0
    check_shoot_fan(env, y0, S_BIG, ref, keep, compact=True, stored_sign=True, label=f"{kind}, no page-locking, compact")
    check_shoot_fan(env, y0, S_BIG, ref, keep, compact=False, stored_sign=False, label=f"{kind}, no page-locking, full")
    check_fan_handle(lib, env, y0, S_BIG, ref, keep, f"{kind}, no page-locking", rounds=False)
    env.set_option("d2h_register", 1)
    check_shoot_fan(env, y0, S_BIG, ref, keep, compact=True, stored_sign=False, label=f"{kind}, page-locking back on")
    env.close()


def test_large_device_resident_fan_equals_the_eager_fan(lib):
    """pr.shoot_rays(device_resident=True).to_host() against device_resident=False at three sub-jobs per array on the
    HBM-table environment, attribute by attribute -- and both against the row reference."""
    import pygenray_amd as pr
    drops, M = big_situation("ends in the second sub-job")
    z = np.arange(0, 6000, 1.0)
    r = np.linspace(0, X1, 21)
    c2 = np.array([pr.munk_ssp(z, 1300.0 + 5e-4 * ri) for ri in r])
    eo = pr.OceanEnvironment2D(pr.DataArray(c2, dims=["range", "depth"], coords={"range": r, "depth": z}),
                               pr.DataArray(np.full(21, 5000.0), dims=["range"], coords={"range": r}), flat_earth_transform=False)
    user = -fan_angles(N_BIG, drops)               # (a fan of 70 angles or more is integrated with ODE angle = -user angle)
    a = pr.shoot_rays(1000.0, 0.0, user, X1, S_BIG, eo, debug=False, flatearth=False, device_resident=False)
    b = pr.shoot_rays(1000.0, 0.0, user, X1, S_BIG, eo, debug=False, flatearth=False, device_resident=True)
    assert not a.device_resident and b.device_resident and len(a) == len(b) == M
    b.to_host()
    assert not b.device_resident
    for k in ("thetas", "n_botts", "n_surfs", "source_depths", "rs", "zs", "ts", "ps"):
        assert same(np.asarray(getattr(a, k)), np.asarray(getattr(b, k))), k
    assert np.array_equal(a.ray_ids, b.ray_ids)
    # the environment the API built, run as a DeviceFan in rows
    from pygenray_amd.launch_rays import _device_env, _initial_slowness
    from pygenray_amd.host_physics import bilinear_interp
    env, (cin, rin, zin) = _device_env(eo, False, False, 0)
    assert env.blocked_layout
    c0 = bilinear_interp(0.0, 1000.0, rin, zin, cin)
    y0 = np.stack([np.zeros(N_BIG), np.full(N_BIG, 1000.0), _initial_slowness(-user, c0)], 1)
    ref = row_reference(lib, env, y0, S_BIG)
    keep = expect_keep(ref, N_BIG, drops)
    want = expected_samples(ref, keep, True, True)
    for k, name in (("T", "ts"), ("z", "zs"), ("p", "ps")):
        assert same(np.ascontiguousarray(getattr(a, name).T), want[k]), name
    assert same(a.n_botts, ref["n_bott"][keep].astype(np.int64)) and same(a.thetas, user[keep])


# ------------------------------------------------------------------ the threshold
@pytest.mark.parametrize("kind", ["lds", "hbm"])
def test_both_sides_of_the_32_MB_threshold(lib, kind):
    """Two fans whose three arrays total just under and just over 32 MB: plain copies on one side, threads, sub-jobs and
    page-locking on the other; the same content rule on both."""
    S = 63
    n_over = -(-PIPELINED_FROM // (3 * S * 8))
    n_under = n_over - 1
    assert not pipelined(3, n_under, S) and pipelined(3, n_over, S) and n_over - n_under == 1
    env, arrs = make_env(lib, kind)
    for N in (n_under, n_over):
        drops = placed_drops(N, 1001)
        assert (N - len(drops)) * S * 8 % 256 != 0
        y0 = y0_for(oracle, arrs, 1000.0, 0.0, fan_angles(N, drops))
        ref = row_reference(lib, env, y0, S)
        keep = expect_keep(ref, N, drops)
        check_shoot_fan(env, y0, S, ref, keep, compact=True, stored_sign=True, label=f"{kind}, {N} rays, compact")
        check_shoot_fan(env, y0, S, ref, keep, compact=False, stored_sign=False, label=f"{kind}, {N} rays, full")
        check_fan_handle(lib, env, y0, S, ref, keep, f"{kind}, {N} rays", rounds=False)
    env.close()


# ------------------------------------------------------------------ the squeeze kernels, shape by shape (small path)
SWEEP_N = (1, 63, 64, 65, 255, 256, 257, 513)


def sweep_drops(N, pattern):
    k = np.arange(N)
    return {"none": k[:0], "all": k, "all but ray 0": k[1:], "all but the last ray": k[:-1], "every second ray": k[1::2]}[pattern]


@pytest.mark.parametrize("kind", ["lds", "hbm"])
def test_squeeze_kernels_shape_sweep(lib, kind):
    """pgr_gather_cols (row source + index list) and pgr_unblock_cols (blocked source, with and without index list) on the
    small path: S in 1 .. 9 (every S mod 4, a lone block, a partial last block), N around the wave and workgroup sizes of
    the squeeze kernels, nothing / everything / all but one end / every second ray dropped.  M = 0: the call succeeds,
    shapes (S, 0), the caller's buffers untouched."""
    env, arrs = make_env(lib, kind)
    x1 = 20e3
    n_cases = 0
    for N in SWEEP_N:
        for pattern in ("none", "all", "all but ray 0", "all but the last ray", "every second ray"):
            drops = sweep_drops(N, pattern)
            y0 = y0_for(oracle, arrs, 1000.0, 0.0, fan_angles(N, drops))
            for S in range(1, 10):
                assert not pipelined(3, N, S)
                ref = row_reference(lib, env, y0, S, x1=x1)
                keep = expect_keep(ref, N, drops)
                M = int(keep.sum())
                assert M == N - len(drops)
                label = f"{kind}, N {N}, S {S}, {pattern}"
                want = expected_samples(ref, keep, True, bool(S & 1))
                bufs = [np.full((S, N), SENTINEL) for _ in range(3)]
                out = env.shoot_fan(y0, 0.0, x1, S, sample_major=True, compact=True, stored_sign=bool(S & 1), buffers=bufs)
                assert same(out["status"], ref["status"]) and same(out["end"], ref["end"]), label
                for name, b in zip("Tzp", bufs):
                    assert out[name].shape == (S, M) and same(out[name], want[name]), (label, name)
                    assert same(b.reshape(-1)[:S * M].reshape(S, M), want[name]), (label, name)
                    assert np.all(b.reshape(-1)[S * M:] == SENTINEL), (label, name, "tail")
                h = lib.FanHandle(env, 0.0, x1, S, y0=y0, stored_sign=True)
                assert h.wait() == (N, M)
                for compact in (True, False):
                    wanted = expected_samples(ref, keep, compact, True)
                    got = h.fetch_samples(compact=compact)
                    for name in "Tzp":
                        assert got[name].shape == (S, M if compact else N) and same(got[name], wanted[name]), (label, compact, name)
                h.close()
                n_cases += 1
    assert n_cases == len(SWEEP_N) * 5 * 9
    env.close()

