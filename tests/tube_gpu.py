"""Shared scaffolding of the ray-tube GPU tests (test_transmission_loss.py, test_arrivals.py, test_beam_tl.py): the `pr`
and `pr_any` fixtures, the environments, the synthetic fans aimed at the kernels' chunk, band and adds-nothing edges, and the helpers
that upload caller buffers and call the `_device` entries.  Not a test module itself."""
import numpy as np
import pytest

import tl_reference as tlr


@pytest.fixture(scope="module")
def pr():
    """the package, for the bit-parity tests: reference arithmetic only"""
    from pygenray_amd import _lib
    if _lib.ARITH != "reference":
        pytest.skip("bit parity is claimed for the reference arithmetic only (PGR_ARITH=contracted: tests/test_contracted_arith.py)")
    _lib.load()
    assert _lib.device_count() >= 1
    import pygenray_amd
    return pygenray_amd


@pytest.fixture(scope="module")
def pr_any():
    """the package in whichever arithmetic this process loaded, for the tolerance tests (closed forms, repeatability): they
    also run in the PGR_ARITH=contracted child of tests/test_contracted_arith.py"""
    from pygenray_amd import _lib
    _lib.load()
    assert _lib.device_count() >= 1
    import pygenray_amd
    return pygenray_amd


def _env(pr, z, r, cin, br, bd):
    ssp = pr.DataArray(cin, dims=["range", "depth"], coords={"range": r, "depth": z})
    bathy = pr.DataArray(bd, dims=["range"], coords={"range": br})
    return pr.OceanEnvironment2D(ssp, bathy, flat_earth_transform=False)


def munk_env(pr, ztop=6000.0):
    """range-independent Munk, 5000 m flat bottom: LDS tables, rows layout"""
    z = np.arange(0, ztop, 1.0)
    r = np.linspace(0, 200e3, 100)
    return _env(pr, z, r, np.tile(pr.munk_ssp(z), (100, 1)), r, np.full(100, 5000.0))


def sloping_env(pr):
    """range-dependent Munk over a sloping bottom: tables in HBM, sample-blocked layout"""
    z = np.linspace(0, 5500, 1377)
    r = np.linspace(0, 200e3, 33)
    br = np.linspace(0, 200e3, 9)
    return _env(pr, z, r, np.array([pr.munk_ssp(z, 1300 + 5e-4 * ri) for ri in r]), br, 4800 + 300 * np.sin(br / 40e3))


DEPTHS = np.linspace(-150.0, 5850.0, 1000)          # some above the surface and below the bottom


def sloping_env_shallow_table(pr):
    """sloping_env with its depth table cut at 4200 m, above the sea floor: the deep rays leave it and are dropped"""
    z = np.linspace(0, 4200, 1051)
    r = np.linspace(0, 200e3, 33)
    br = np.linspace(0, 200e3, 9)
    return _env(pr, z, r, np.array([pr.munk_ssp(z, 1300 + 5e-4 * ri) for ri in r]), br, 4800 + 300 * np.sin(br / 40e3))


# ---- synthetic inputs for the kernels -----------------------------------------------------------------------------------

SYN_R = np.linspace(0.0, 60e3, 13)                           # uniform range grid
SYN_Z = np.concatenate([np.arange(0.0, 1000.0, 20.0), np.arange(1000.0, 5001.0, 50.0)])    # non-uniform depth grid


def syn_cin():
    """the sound speed of syn_env's table: smooth, positive and range dependent, so that the bilinear look-up of c matters"""
    rr, zz = np.meshgrid(SYN_R, SYN_Z, indexing="ij")
    return 1490.0 + 0.017 * zz + 8.0 * np.sin(2 * np.pi * rr / 40e3) + 6.0 * np.exp(-((zz - 1200.0) / 500.0) ** 2)


@pytest.fixture(scope="module")
def syn_env(pr_any):
    """a small range-dependent table (tables in HBM): syn_cin() on SYN_R x SYN_Z"""
    from pygenray_amd import _lib
    cin = syn_cin()
    cpin = np.gradient(cin, SYN_Z, axis=1, edge_order=1)
    nr = len(SYN_R)
    return _lib.EnvHandle(cin, cpin, SYN_R, SYN_Z, np.full(nr, 5000.0), SYN_R.copy(), np.zeros(nr)), cin


def _p_with_pc(c, target_above):
    """a slowness p > 0 with fl(p c) == 1.0 exactly (target_above False) or fl(p c) just above 1 (True)"""
    p = 1.0 / c
    for _ in range(8):
        pc = p * c
        if (pc > 1.0) if target_above else (pc == 1.0):
            return p
        p = np.nextafter(p, np.inf if pc <= 1.0 else -np.inf)
    raise AssertionError(f"no p with p c {'>' if target_above else '=='} 1 for c = {c!r}")


def synthetic_fan(M, S, R, seed, cin, shuffle=False):
    """(z, p) [S][M] stored convention, x [S], p0 [M], receiver depths [R] exercising the kernel's edges.  Column s follows
    one of four patterns: a monotone fan (chunks mostly miss a band), a fold (ray order reverses between neighbours),
    a scramble (tubes of every chunk overlap, every receiver sums across all chunks and rounds) and a fan clustered near
    the surface.  All finite depths lie in [-200, 5200] m, the ranges in the table's span."""
    rng = np.random.default_rng(seed)
    u = np.linspace(0.0, 1.0, M)
    x = np.linspace(0.0, 55e3, S)
    if S >= 4:
        x[S - 2] = x[0]                                       # a column s > 0 with r_s == 0: NaN
    d = np.empty((S, M))
    for s in range(S):
        kind = s % 4
        if kind == 0:
            d[s] = 2500.0 + 2400.0 * (2 * u - 1) + rng.uniform(-0.1, 0.1, M)
        elif kind == 1:
            d[s] = 2500.0 + 2000.0 * np.sin(3 * np.pi * u + s)
        elif kind == 2:
            d[s] = rng.uniform(-200.0, 5200.0, M)
        else:
            d[s] = 100.0 + 4000.0 * u ** 3
    p = np.sin(np.radians(rng.uniform(-30.0, 30.0, (S, M)))) / 1500.0
    p0 = np.sin(np.radians(np.linspace(-25.0, 25.0, M) + rng.uniform(-1e-3, 1e-3, M))) / 1500.0
    # the branches where a tube adds nothing, mid-ray and on the seam of chunks 0 / 1 where the fan is long enough
    cols = [s for s in range(S) if x[s] != x[0]]
    if M >= 8 and cols:
        d[cols[0], M // 2] = np.nan                                  # NaN depth, finite p
        p[cols[1 % len(cols)], M // 3] = np.nan                      # NaN p, finite depth
        s = cols[2 % len(cols)]
        d[s, M // 4 + 1] = d[s, M // 4]                              # equal depths of neighbours
        for j, (k, above) in enumerate([(M // 5, False), (M - 3, True), (min(62, M - 1), False), (min(63, M - 1), True)]):
            s = cols[j % len(cols)]
            if np.isfinite(d[s, k]) and np.isfinite(p[s, k]):
                c = tlr.bilinear(x[s], d[s, k], SYN_R, SYN_Z, cin)
                p[s, k] = (1 - 2 * (j & 1)) * _p_with_pc(c, above)  # |p c| == 1 and just above 1, both signs
    if M >= 4 * 63 + 1:
        d[S - 1, 2 * 63: 3 * 63 + 1] = np.nan                       # chunk 2 all NaN in the last column: bounds [+inf, -inf]
    depths = np.linspace(-300.0, 5300.0, R) if R > 1 else np.array([2500.0])   # the first / last above / below every sample
    if R >= 8:
        s = cols[0] if cols else 0
        fin = d[s][np.isfinite(d[s])]
        on = rng.choice(fin, R // 4, replace=len(fin) < R // 4)
        depths[1: 1 + len(on)] = on                                 # receivers on sample depths: one tube's lo, another's hi
    depths = rng.permutation(depths) if shuffle else np.sort(depths)
    assert len(depths) == R and np.isfinite(depths).all()
    return -d, p, x, p0, depths


def _same(a, b):
    return np.array_equal(a, b, equal_nan=True)


def _upload(env, *arrays):
    """the float64 host arrays on env's device, and its current stream"""
    import torch
    dev = torch.device("cuda", env.device)
    return [torch.from_numpy(np.ascontiguousarray(a, dtype=np.float64)).to(dev) for a in arrays], \
        torch.cuda.current_stream(dev).cuda_stream


def _image(env, z, depths):
    """an (R, S) float64 output on env's device, filled with -1"""
    import torch
    return torch.full((len(depths), z.shape[0]), -1.0, dtype=torch.float64, device=torch.device("cuda", env.device))


def _device_intensity(env, z, p, x, p0, depths):
    from pygenray_amd import _lib
    t, stream = _upload(env, z, p, x, p0, depths)
    S, M = z.shape
    out = _image(env, z, depths)
    _lib.intensity_device(env, t[0].data_ptr(), t[1].data_ptr(), M, S, t[2].data_ptr(), t[3].data_ptr(), t[4].data_ptr(),
                          len(depths), out.data_ptr(), stream)
    return out.cpu().numpy()


def _device_beams(env, z, p, x, p0, bottom, depths, w_min):
    from pygenray_amd import _lib
    t, stream = _upload(env, z, p, x, p0, bottom, depths)
    S, M = z.shape
    out = _image(env, z, depths)
    _lib.beam_intensity_device(env, t[0].data_ptr(), t[1].data_ptr(), M, S, t[2].data_ptr(), t[3].data_ptr(),
                               t[4].data_ptr(), t[5].data_ptr(), len(depths), w_min, out.data_ptr(), stream)
    return out.cpu().numpy()


def _device_arrivals(env, t, z, p, x, p0, depths, cols):
    import torch
    from pygenray_amd import _lib
    d, stream = _upload(env, t, z, p, x, p0, depths)
    dev = d[0].device
    S, M = z.shape
    R, n = len(depths), len(cols)
    counts = torch.full((R * n,), -1, dtype=torch.int64, device=dev)
    _lib.arrival_counts_device(env, d[1].data_ptr(), d[2].data_ptr(), M, S, d[3].data_ptr(), d[4].data_ptr(),
                               d[5].data_ptr(), R, cols, counts.data_ptr(), stream)
    offsets = torch.zeros(R * n + 1, dtype=torch.int64, device=dev)
    torch.cumsum(counts, 0, out=offsets[1:])
    total = int(offsets[-1].item())
    out = dict(offsets=offsets.cpu().numpy(), tube=np.zeros(0, np.int32), w=np.zeros(0), T=np.zeros(0), p=np.zeros(0),
               I=np.zeros(0))
    if total:
        tube = torch.full((total,), -1, dtype=torch.int32, device=dev)
        f = [torch.full((total,), -1.0, dtype=torch.float64, device=dev) for _ in range(4)]
        _lib.arrivals_device(env, d[0].data_ptr(), d[1].data_ptr(), d[2].data_ptr(), M, S, d[3].data_ptr(),
                             d[4].data_ptr(), d[5].data_ptr(), R, cols, offsets.data_ptr(), total, tube.data_ptr(),
                             *(a.data_ptr() for a in f), stream)
        out.update(tube=tube.cpu().numpy(), **{k: a.cpu().numpy() for k, a in zip(("w", "T", "p", "I"), f)})
    return out
