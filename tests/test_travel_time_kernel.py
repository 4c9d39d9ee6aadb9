"""travel_time_kernel on the GPU: the kernel alone bit for bit against the restatement (tests/ttk_reference.py) on synthetic
fans and against the independent reference (tests/ttk_independent.py) within its derived rounding bound on grids of many
tiles, the grid-size limit, the default-grid identity K . cin = -(T_c - T_0), dropped rays and the flat-earth frame, the
linearisation against finite differences of re-shot fans, the eigenrays, one answer from every path to the same fan, and
the contracted build."""
import os
import subprocess
import sys

import numpy as np
import pytest

import ttk_reference as ttr
from tube_gpu import (SYN_R, SYN_Z, _same, _upload, munk_env, pr, pr_any, sloping_env,  # noqa: F401
                      sloping_env_shallow_table, syn_env)

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


# ---- the kernel alone ---------------------------------------------------------------------------------------------------

def synthetic(M, S, seed, g, h):
    """T, Z (S, M) rows (stored convention), x (S,) in the frame of syn_env's table: depths wandering over and past the
    grid (above the surface, below the last node), samples on grid lines, a vertical chord, rays along a depth and along a
    depth line, NaN samples."""
    rng = np.random.default_rng(seed)
    x = np.linspace(-2e3, 62e3, S)
    if S >= 5:
        x[2] = g[1]                                          # a sample on a range line
        x[3] = x[2]                                          # and a vertical chord on it
    d = np.empty((S, M))
    d[0] = rng.uniform(-100.0, 5100.0, M)
    for s in range(1, S):
        d[s] = d[s - 1] + rng.normal(0.0, 300.0 if s % 3 else 30.0, M)
    d = np.clip(d, -300.0, 5400.0)
    on = rng.random((S, M)) < 0.1
    d[on] = rng.choice(h, on.sum())                          # samples on depth lines
    if S >= 3 and M >= 3:
        d[1:, 1] = d[0, 1]                                   # a ray along one depth
        d[:, 2] = h[len(h) // 2]                             # a ray along a depth line
    T = np.concatenate([np.zeros((1, M)), np.cumsum(np.hypot(np.diff(x)[:, None], np.diff(d, axis=0)), axis=0)]) / 1500.0
    T += rng.uniform(0.0, 1e-3, T.shape)
    if M >= 8 and S >= 3:
        T[S - 1, M // 2] = np.nan                            # NaN at the last column: the row is NaN there only
        d[1, M // 3] = np.nan                                # NaN at column 1
    return T, -d, x


def _device_kernel(env, T, Z, x, g, h, col):
    import torch
    from pygenray_amd import _lib
    t, stream = _upload(env, T, Z, x, g, h)
    S, M = T.shape
    out = torch.full((M, len(g), len(h)), -1.0, dtype=torch.float64, device=t[0].device)
    _lib.travel_time_kernel_device(env, t[0].data_ptr(), t[1].data_ptr(), M, S, t[2].data_ptr(), t[3].data_ptr(), len(g),
                                   t[4].data_ptr(), len(h), col, out.data_ptr(), stream)
    return out.cpu().numpy()


def _depth_grid(B):
    return np.concatenate([[0.0], np.sort(np.random.default_rng(B).uniform(1.0, 4999.0, B - 2)), [5000.0]])


# M: one ray, a wave's worth and either side, several; S: one chord, two, many; B at the depth tile (63) and +-1, and
# several tiles; A = 2; columns 0, 1, the last and a middle one
@pytest.mark.parametrize("M, S, A, B, col", [
    (1, 2, 13, 63, 1), (1, 3, 2, 64, -1), (63, 3, 13, 62, 0), (64, 200, 13, 63, -1), (65, 200, 2, 64, 100),
    (65, 200, 13, 64, 1), (300, 200, 7, 63, 137), (300, 3, 13, 130, 2)])
def test_kernel_bit_identical_on_synthetic_inputs(pr, syn_env, M, S, A, B, col):
    env, cin = syn_env
    g = np.linspace(0.0, 60e3, A) if A > 2 else np.array([5e3, 50e3])
    h = _depth_grid(B)
    T, Z, x = synthetic(M, S, 7 * M + S, g, h)
    c = col % S
    K = _device_kernel(env, T, Z, x, g, h, c)
    ref = ttr.kernel(T, Z, x, g, h, cin, SYN_R, SYN_Z, c)
    assert _same(K, ref)
    if c == 0:
        assert (K == 0).all()
    else:
        assert (K[np.isfinite(K)] != 0).any()


# ---- fans -------------------------------------------------------------------------------------------------------------

def _identity(K, cin, fan, col=-1, rtol=1e-12):
    Tc = np.asarray(fan.ts)
    lhs = (K * cin[None]).sum(axis=(1, 2))
    rhs = -(Tc[:, col] - Tc[:, 0])
    np.testing.assert_allclose(lhs, rhs, rtol=rtol, atol=0)


@pytest.mark.parametrize("which", ["munk", "sloping"])
def test_default_grid_identity(pr_any, which):
    env = munk_env(pr_any) if which == "munk" else sloping_env(pr_any)
    fan = pr_any.shoot_rays(1000.0, 0.0, np.linspace(-25, 25, 40), 100e3, 501, env, flatearth=False, debug=False)
    assert ((fan.n_botts + fan.n_surfs) > 0).sum() > 5
    K = pr_any.travel_time_kernel(fan, env, flatearth=False)
    cin, rin, zin = ttr.traced_tables(env, False, False)
    assert K.shape == (40, len(rin), len(zin)) and np.isfinite(K).all()
    _identity(K, cin, fan)
    _identity(pr_any.travel_time_kernel(fan, env, flatearth=False, range_index=250), cin, fan, 250)


@pytest.mark.parametrize("blocked", [False, True])
def test_one_answer_whatever_the_path(pr, blocked):
    """a device-resident fan (rows layout on the LDS-table Munk environment, sample-blocked on the HBM-table sloping one),
    twice, then its to_host() copy, then the restatement of that copy"""
    env = sloping_env(pr) if blocked else munk_env(pr)
    g, h = np.linspace(0.0, 100e3, 23), np.linspace(0.0, 5200.0, 130)
    dev = pr.shoot_rays(1000.0, 0.0, np.linspace(-12, 12, 150), 100e3, 201, env, flatearth=False, debug=False,
                        device_resident=True)
    assert dev.device_resident and dev._dev._env.blocked_layout == blocked
    a = pr.travel_time_kernel(dev, env, g, h, flatearth=False)
    b = pr.travel_time_kernel(dev, env, g, h, flatearth=False, range_index=-1)
    assert dev.device_resident and "_zs" not in dev.__dict__       # processed in place, nothing fetched
    dev.to_host()
    c = pr.travel_time_kernel(dev, env, g, h, flatearth=False)
    assert _same(a, b) and _same(a, c)
    assert _same(c, ttr.fan_kernel(dev, env, g, h, flatearth=False))


def _mirrored_env(pr, env):
    """the environment seen from the other side: x -> -x"""
    c, b = env.sound_speed, env.bathymetry
    r, z = np.asarray(c.coords["range"], float), np.asarray(c.coords["depth"], float)
    br = np.asarray(b.coords["range"], float)
    ssp = pr.DataArray(np.asarray(c.values)[::-1].copy(), dims=["range", "depth"], coords={"range": -r[::-1], "depth": z})
    bathy = pr.DataArray(np.asarray(b.values)[::-1].copy(), dims=["range"], coords={"range": -br[::-1]})
    return pr.OceanEnvironment2D(ssp, bathy, flat_earth_transform=False)


def test_backwards_fan_is_the_mirrored_forward_fan(pr):
    """range-dependent Munk over a flat bottom (a sloping one would differ in the bits of its mirrored bottom angles)"""
    from tube_gpu import _env
    z, r = np.linspace(0, 5500, 1377), np.linspace(0, 200e3, 33)
    env = _env(pr, z, r, np.array([pr.munk_ssp(z, 1300 + 5e-4 * ri) for ri in r]), r, np.full(33, 5000.0))
    ang = np.linspace(-12, 12, 90)
    back = pr.shoot_rays(900.0, 150e3, ang, 40e3, 111, env, flatearth=False, debug=False, device_resident=True)
    menv = _mirrored_env(pr, env)
    fwd = pr.shoot_rays(900.0, -150e3, ang, -40e3, 111, menv, flatearth=False, debug=False, device_resident=True)
    g, h = np.linspace(30e3, 160e3, 14), np.linspace(0.0, 5000.0, 64)
    Kb = pr.travel_time_kernel(back, env, g, h, flatearth=False)
    Kf = pr.travel_time_kernel(fwd, menv, -g[::-1], h, flatearth=False)
    back.to_host()
    fwd.to_host()
    assert _same(Kb, ttr.fan_kernel(back, env, g, h, flatearth=False))
    assert _same(back.ts, fwd.ts) and _same(back.zs, fwd.zs)
    assert _same(Kb, Kf[:, ::-1])


# ---- linearisation: finite differences of re-shot fans ----------------------------------------------------------------

EPS_DC = 0.01         # the largest |δc| of the ± perturbations, m/s (small: see _bound, the path-shift term)
RTOL = 1e-10          # the integrator's rtol in these runs


def blob(r, z, xc):
    """the δc shape: a Gaussian blob of 200 m by 10 km (standard deviations) at 1000 m depth and range xc, peak 1"""
    return np.exp(-0.5 * ((z[None, :] - 1000.0) / 200.0) ** 2 - 0.5 * ((r[:, None] - xc) / 10e3) ** 2)


def _perturbed(pr, env, dc):
    """a fresh environment (_unpack_envi caches by id()) with env's TRUE sound speed + dc, on the same grids"""
    c, b = env.sound_speed, env.bathymetry
    ssp = pr.DataArray(np.asarray(c.values, float) + dc, dims=["range", "depth"],
                       coords={"range": np.asarray(c.coords["range"], float), "depth": np.asarray(c.coords["depth"], float)})
    bathy = pr.DataArray(np.asarray(b.values, float), dims=["range"], coords={"range": np.asarray(b.coords["range"], float)})
    return pr.OceanEnvironment2D(ssp, bathy, lat=env.latitude, flat_earth_transform=hasattr(env, "sound_speed_fe"))


def fixed_endpoint_dT(fp, fm, col=-1):
    """½[T(+) - T(-)] at a fixed end point.  The ± rays leave at the same angle and end at depths d± = -zs± at the same
    range.  Moving an end point by δd along the end column changes T by p_d δd, p_d = dT/dd the vertical slowness; in the
    stored convention (zs = -d, ps = -p_d) p_d δd = ps · δzs.  So T(±) at the unperturbed end point is
    T± - ps · (zs± - zs), and the symmetric difference is ½(T+ - T-) - ps · ½(zs+ - zs-), with ps the mean of the ±
    runs' (their difference is first order, its product with ½(zs+ - zs-) second order and even: it cancels)."""
    ps = 0.5 * (np.asarray(fp.ps)[:, col] + np.asarray(fm.ps)[:, col])
    return 0.5 * (np.asarray(fp.ts)[:, col] - np.asarray(fm.ts)[:, col]) \
        - ps * 0.5 * (np.asarray(fp.zs)[:, col] - np.asarray(fm.zs)[:, col])


def _fd_case(pr, env, src, ang, x1, S, flatearth):
    r = np.asarray(env.sound_speed.coords["range"], float)
    z = np.asarray(env.sound_speed.coords["depth"], float)
    dc = EPS_DC * blob(r, z, 0.5 * x1)
    e_p, e_m = _perturbed(pr, env, dc), _perturbed(pr, env, -dc)
    shoot = dict(flatearth=flatearth, debug=False, rtol=RTOL)
    f0 = pr.shoot_rays(src, 0.0, ang, x1, S, env, **shoot)
    fp = pr.shoot_rays(src, 0.0, ang, x1, S, e_p, **shoot)
    fm = pr.shoot_rays(src, 0.0, ang, x1, S, e_m, **shoot)
    K = pr.travel_time_kernel(f0, env, flatearth=flatearth)
    if flatearth:                       # K is with respect to the flat-earth table: its node (a, b) moves by F_b δc_true
        F = pr.eflat(z, env.latitude, np.ones_like(z))[1]
        pred = (K * (dc * F[None, :])[None]).sum(axis=(1, 2))
    else:
        pred = (K * dc[None]).sum(axis=(1, 2))
    same = (f0.n_botts == fp.n_botts) & (f0.n_botts == fm.n_botts) & (f0.n_surfs == fp.n_surfs) & (f0.n_surfs == fm.n_surfs)
    return f0, fixed_endpoint_dT(fp, fm), pred, same


def _bound(fan, pred, dz, cmin, kappa, c2, c3):
    """The tolerance of |FD - K·δc| per ray.  ε δc peaks at EPS_DC, the blob's depth scale 200 m gives |∂δc/∂z| <= EPS_DC /
    200 m and |∂²δc/∂z²| <= EPS_DC / (200 m)², its range scale 10 km; L = T · 1600 m/s bounds the path length; the table:
    depth step dz, |∂c/∂z| / c <= kappa (the ray curvature bound), |∂²c/∂z²| <= c2, |∂³c/∂z³| <= c3.
    * the remainder of the symmetric difference: its even terms cancel, the third-order one is set by how far the
      perturbation bends the path across the blob: by up to η · 200 m, η = |∂²δc/∂z²| / cmin · L² / 8, which changes δT
      by a relative η²: η² |K·δc|;
    * the integrator's noise: each of the ± fans has its own step sequence, |err T| <= RTOL · T, and the end-depth
      correction carries the depth error RTOL · 6000 m times |ps|: 2 RTOL (T + |ps| 6000) for the difference of two runs;
    * the chord sagitta: K integrates along the chords between save samples, not the arcs; a path up to kappa Δx² / 8
      off (Δx the save spacing) sees δc / c² change by up to |∂δc/∂z| / cmin² per metre: |∂δc/∂z| / cmin² · kappa Δx² / 8 · L;
    * the cpin path inconsistency: the fan is traced with ∂c/∂z from np.gradient(cin), not the derivative of the bilinear
      c, so Fermat's first-order cancellation leaves that residual, / cmin², acting on the perturbation's path shift
      `shift` <= (|∂δc/∂z| / cmin) · sqrt(2 pi) 10 km · L (the blob's deflection times the lever arm).  Over each depth cell
      the residual has the mean dz² |∂³c/∂z³| / 4 (central differences interpolated linearly, against the cell's secant),
      acting all along the path: dz² c3 / 4 / cmin² · shift · L; its zero-mean part, up to dz / 2 · c2, averages out over
      the cells a ray crosses except where it runs level, at a turning point, over 2 sqrt(2 dz / kappa) of range, at most
      L / 20 km of them: dz / 2 · c2 / cmin² · shift · 2 sqrt(2 dz / kappa) · L / 20 km.
    The residual between two save samples with a reflection in between is left out: the blob is 5 scales from
    both boundaries, where δc < 4e-6 EPS_DC."""
    T = np.asarray(fan.ts)[:, -1]
    L = T * 1600.0
    dx = np.max(np.diff(np.asarray(fan.rs)[0]))
    grad, curv = EPS_DC / 200.0, EPS_DC / 200.0 ** 2
    eta = curv / cmin * L ** 2 / 8
    nonlin = eta ** 2 * np.abs(pred)
    noise = 2 * RTOL * (T + np.abs(np.asarray(fan.ps)[:, -1]) * 6000.0)
    sag = grad / cmin ** 2 * kappa * dx ** 2 / 8 * L
    shift = grad / cmin * np.sqrt(2 * np.pi) * 10e3 * L
    cpin = dz ** 2 * c3 / 4 / cmin ** 2 * shift * L + dz / 2 * c2 / cmin ** 2 * shift * 2 * np.sqrt(2 * dz / kappa) * L / 20e3
    return nonlin + noise + sag + cpin


def test_linearisation_refracting_fan_without_boundaries(pr_any):
    """(a) c = 1520 - 0.02 z (tl_reference.gradient_env): no boundary contact and no caustic at the end column, asserted
    as tl_reference.check_gradient_fan asserts them.  c is linear in z, so np.gradient is exact and the cpin term is 0."""
    import tl_reference as tlr
    env = tlr.gradient_env()
    ang = np.linspace(-8.0, 8.0, 41)
    f0, fd, pred, same = _fd_case(pr_any, env, tlr.GRADIENT_ZS, ang, tlr.GRADIENT_X1, tlr.GRADIENT_S, False)
    d = -np.asarray(f0.zs)
    assert (f0.n_botts == 0).all() and (f0.n_surfs == 0).all() and d.min() > 200.0 and d.max() < 4800.0
    th = np.radians(ang)
    assert (tlr.linear_gradient_ray(tlr.GRADIENT_X1, np.linspace(th.min(), th.max(), 401), tlr.GRADIENT_ZS,
                                    tlr.GRADIENT_CA, tlr.GRADIENT_GAMMA)[2] > 0).all()      # no caustic
    assert same.all()
    tol = _bound(f0, pred, 10.0, 1420.0, 0.02 / 1420.0, 0.0, 0.0)
    assert np.abs(fd).max() > 1e-3 * EPS_DC                 # the blob is seen
    assert (np.abs(fd - pred) <= tol).all(), np.max(np.abs(fd - pred) / tol)


@pytest.mark.parametrize("flatearth", [False, True])
def test_linearisation_munk_fan_with_bounces(pr_any, flatearth):
    """(b) Munk to 100 km with surface and bottom bounces, the rays whose bounce counts differ between the ± runs left
    out; (c) the same with flatearth=True, the TRUE sound speed perturbed and K · (F δc) predicting.  Munk on the 1 m grid:
    |∂c/∂z| / c <= 0.11 / 1500 m^-1, |∂²c/∂z²| <= 2e-4 (m s)^-1 and |∂³c/∂z³| <= 3e-7 (m² s)^-1 (all at the surface)."""
    z = np.arange(0, 6000, 1.0)
    r = np.linspace(0, 200e3, 100)
    ssp = pr_any.DataArray(np.tile(pr_any.munk_ssp(z), (100, 1)), dims=["range", "depth"], coords={"range": r, "depth": z})
    bathy = pr_any.DataArray(np.full(100, 5000.0), dims=["range"], coords={"range": r})
    env = pr_any.OceanEnvironment2D(ssp, bathy, flat_earth_transform=flatearth)
    ang = np.linspace(-20.0, 20.0, 81)
    f0, fd, pred, same = _fd_case(pr_any, env, 1000.0, ang, 100e3, 1001, flatearth)
    assert ((f0.n_botts + f0.n_surfs)[same] > 0).sum() > 10 and same.sum() > 50
    tol = _bound(f0, pred, 1.0, 1500.0, 0.11 / 1500.0, 2e-4, 3e-7)[same]
    err = np.abs(fd - pred)[same]
    assert np.abs(fd[same]).max() > 1e-3 * EPS_DC
    assert (err <= tol).all(), np.max(err / tol)


def test_eigenray_travel_times(pr_any):
    """travel_time_kernel(find_eigenrays(...)) predicts the change of the eigenray travel times between the ±ε
    environments: an eigenray ends at its receiver, so no end-point correction, but the search leaves the end depth up to
    ztol off: |ps| ztol (|ps| <= 7e-4 s/m) per run.  The other terms are _bound's (60 km, Δx = 100 m)."""
    env = munk_env(pr_any)
    z = np.asarray(env.sound_speed.coords["depth"], float)
    r = np.asarray(env.sound_speed.coords["range"], float)
    dc = EPS_DC * blob(r, z, 30e3)
    rx, ztol = [500.0, 800.0, 1200.0, 2000.0, 3000.0], 1e-6
    kw = dict(flatearth=False, rtol=RTOL)

    def eig(e):
        fan = pr_any.shoot_rays(1000.0, 0.0, np.linspace(-14, 14, 400), 60e3, 601, e, debug=False, **kw)
        return pr_any.find_eigenrays(fan, rx, 1000.0, 0.0, 60e3, 601, e, ztol=ztol, max_iter=60, **kw)
    e0, ep, em = eig(env), eig(_perturbed(pr_any, env, dc)), eig(_perturbed(pr_any, env, -dc))
    K = pr_any.travel_time_kernel(e0, env, flatearth=False)
    assert sorted(K) == list(range(len(rx)))
    n = 0
    for j in range(len(rx)):
        assert K[j].shape[0] == len(e0.launch_angles[j])
        if not len(e0.launch_angles[j]):
            continue
        pred = (K[j] * dc[None]).sum(axis=(1, 2))
        f0 = pr_any.RayFan.from_arrays(e0.launch_angles[j], e0.rs[j], e0.ts[j], e0.zs[j], e0.ps[j], e0.n_botts[j],
                                       e0.n_surfs[j], np.full(len(e0.ts[j]), 1000.0))
        tol = _bound(f0, pred, 1.0, 1500.0, 0.11 / 1500.0, 2e-4, 3e-7) + 2 * 7e-4 * ztol
        for m in range(len(e0.launch_angles[j])):
            key = (e0.n_botts[j][m], e0.n_surfs[j][m])

            def match(e):
                c = [k for k in range(len(e.launch_angles[j])) if (e.n_botts[j][k], e.n_surfs[j][k]) == key]
                k = min(c, key=lambda k: abs(e.launch_angles[j][k] - e0.launch_angles[j][m])) if c else None
                return k if k is not None and abs(e.launch_angles[j][k] - e0.launch_angles[j][m]) < 0.05 else None
            kp, km = match(ep), match(em)
            if kp is None or km is None:
                continue
            fd = 0.5 * (ep.ts[j][kp, -1] - em.ts[j][km, -1])
            assert abs(fd - pred[m]) <= tol[m], (j, m, fd, pred[m], tol[m])
            n += 1
    assert n >= 6


# ---- the contracted build ---------------------------------------------------------------------------------------------

def test_contracted_build_identity_in_its_own_process():
    from pygenray_amd import _lib
    if _lib.ARITH != "reference":
        pytest.skip("this IS the contracted process")
    if not os.path.exists(_lib.CONTRACTED_LIB):
        pytest.fail("libpgr_hip_fma.so is not built (__graft_entry__.build() builds it beside the product)")
    env = dict(os.environ, PGR_ARITH="contracted")
    out = subprocess.run([sys.executable, "-m", "pytest", "-q", "-m", "gpu", "-x", "-p", "no:cacheprovider",
                          os.path.join(ROOT, "tests", "test_travel_time_kernel.py"), "-k", "contracted_identity"],
                         cwd=ROOT, env=env, capture_output=True, text=True, timeout=900)
    tail = out.stdout[-3000:] + out.stderr[-1500:]
    assert out.returncode == 0 and " passed" in out.stdout, tail


def test_contracted_identity(pr_any):
    """In the contracted build every a * b + c may be fused: each fused operation rounds once instead of twice, so each
    K term moves by a few ulp (relative 2^-50) against the reference build, and the kernel stays exact for the contracted
    look-up's own c.  The look-up itself (c, fused) then differs from cin's bilinear blend by ~2^-52 relative, which enters
    K · cin once.  Every term of K · cin has one sign (no cancellation), so the relative error of the identity is the
    reference build's summation error plus ~4 · 2^-52: within the same 1e-12."""
    from pygenray_amd import _lib
    if _lib.ARITH != "contracted":
        pytest.skip("runs in the PGR_ARITH=contracted child of test_contracted_build_identity_in_its_own_process")
    env = munk_env(pr_any)
    fan = pr_any.shoot_rays(1000.0, 0.0, np.linspace(-14, 14, 20), 100e3, 501, env, flatearth=False, debug=False)
    K = pr_any.travel_time_kernel(fan, env, flatearth=False)
    cin, _, _ = ttr.traced_tables(env, False, False)
    _identity(K, cin, fan)
    assert _same(K, pr_any.travel_time_kernel(fan, env, flatearth=False))


# ---- the kernel against the independent reference (tests/ttk_independent.py) --------------------------------------------

def banded(B, h, S, seed):
    """T, Z (S, M), x (S,) on the depth grid h of B nodes (tiles of 63 nodes): rays held in narrow depth bands (most tiles
    skipped), level rays on nodes 62, 63, 125 and 126 (the tile seams), a ray weaving across the seam between cells 61
    and 64, and rays wholly above and wholly below the grid"""
    rng = np.random.default_rng(seed)
    x = np.linspace(-1e3, 61e3, S)
    rows = []
    for b in (62, 63, 125, 126):
        if b < B:
            rows.append(np.full(S, h[b]))
    if B > 65:
        lo, hi = h[61], h[65]
        rows.append(np.where(np.arange(S) % 2, hi, lo) + rng.uniform(-0.3, 0.3, S) * (hi - lo))   # weaving the seam
    for c in (0.2, 0.55, 0.9):                                         # narrow bands
        k = int(c * (B - 1))
        rows.append(h[k] + rng.uniform(0.0, 3.0, S) * (h[min(k + 1, B - 1)] - h[k]))
    rows.append(np.linspace(-150.0, -40.0, S))                          # above the grid
    rows.append(np.linspace(h[-1] + 10.0, h[-1] + 300.0, S))            # below it
    d = np.array(rows).T
    T = np.concatenate([np.zeros((1, d.shape[1])), np.cumsum(np.hypot(np.diff(x)[:, None], np.diff(d, axis=0)), axis=0)])
    return T / 1500.0 + rng.uniform(0.0, 1e-4, d.shape), -d, x


@pytest.mark.parametrize("B", [126, 127, 6000])
def test_kernel_within_the_derived_bound_of_the_independent_reference(pr, syn_env, B):
    """B = 126 is exactly two tiles of 63 nodes, 127 two and one node, 6000 95 tiles and a partial one of 15 nodes.  The
    tolerance is ttk_independent's bound (its docstring derives it); the restatement gives the same bits as the kernel."""
    import ttk_independent as tti
    env, cin = syn_env
    g = np.array([-500.0, 7e3, 19e3, 20e3, 33e3, 47.5e3, 60e3])
    h = np.linspace(0.0, 5000.0, B)
    T, Z, x = banded(B, h, 24, B)
    col = len(x) - 1
    K = _device_kernel(env, T, Z, x, g, h, col)
    Ki, mag, bound = tti.kernel(T, Z, x, g, h, cin, SYN_R, SYN_Z, col)
    assert np.isfinite(K).all()
    assert (np.abs(K - Ki) <= bound).all(), np.max(np.abs(K - Ki) - bound)
    assert (K[bound == 0] == 0).all() and (K != 0).any()
    assert bound.max() < 1e-9 * np.abs(Ki).max()                  # the bound is not vacuous
    assert _same(K, ttr.kernel(T, Z, x, g, h, cin, SYN_R, SYN_Z, col))


@pytest.mark.parametrize("S", [257, 513, 1001])
def test_kernel_bit_identical_with_more_chords_than_lanes(pr, syn_env, S):
    """more than 256 chords: pgr_ttk_seg and pgr_ttk_span stride a lane over several; the columns either side of 256 and 512"""
    env, cin = syn_env
    g = np.linspace(0.0, 60e3, 9)
    h = _depth_grid(70)
    T, Z, x = synthetic(9, S, S, g, h)
    for col in sorted({c for c in (255, 256, 257, 511, 512, S - 1) if c < S}):
        K = _device_kernel(env, T, Z, x, g, h, col)
        assert _same(K, ttr.kernel(T, Z, x, g, h, cin, SYN_R, SYN_Z, col)), col


def test_range_count_at_its_limits(pr, syn_env):
    """A = 65535 (the most a launch's gridDim.y takes) for one two-sample ray: the restatement's bits.  A = 65536 through
    the C entry: refused before any launch, the output left as it was."""
    import torch
    from pygenray_amd import _lib
    env, cin = syn_env
    x = np.array([1e3, 59e3])
    T, Z = np.array([[0.0], [39.0]]), np.array([[-900.0], [-1400.0]])
    h = np.array([0.0, 1000.0, 2000.0])
    g = np.linspace(0.0, 60e3, 65535)
    K = _device_kernel(env, T, Z, x, g, h, 1)
    assert _same(K, ttr.kernel(T, Z, x, g, h, cin, SYN_R, SYN_Z, 1)) and (K != 0).sum() > 1000
    g = np.linspace(0.0, 60e3, 65536)
    t, stream = _upload(env, T, Z, x, g, h)
    out = torch.full((1, len(g), len(h)), -1.0, dtype=torch.float64, device=t[0].device)
    with pytest.raises(_lib.PgrError, match="n_ranges must be 2 .. 65535"):
        _lib.travel_time_kernel_device(env, t[0].data_ptr(), t[1].data_ptr(), 1, 2, t[2].data_ptr(), t[3].data_ptr(),
                                       len(g), t[4].data_ptr(), len(h), 1, out.data_ptr(), stream)
    assert (out == -1.0).all()


@pytest.mark.parametrize("blocked", [False, True], ids=["rows", "sample-blocked"])
def test_dropped_rays(pr, blocked):
    """a device fan whose keep list is not the identity (tables shallower than the sea floor: the deep rays leave them and
    are dropped): one row per surviving ray, in order, the same bits as its host twin and the restatement, and the
    default-grid identity for every row, at the last and a middle column"""
    env = sloping_env_shallow_table(pr) if blocked else munk_env(pr, ztop=4200.0)
    ang = np.linspace(-20, 20, 60)
    kw = dict(flatearth=False, debug=False)
    dev = pr.shoot_rays(1000.0, 0.0, ang, 100e3, 101, env, device_resident=True, **kw)
    host = pr.shoot_rays(1000.0, 0.0, ang, 100e3, 101, env, device_resident=False, **kw)
    assert 5 < len(ang) - len(dev) < 55 and len(dev) == len(host)
    assert dev._dev._env.blocked_layout == blocked
    g, h = np.linspace(0.0, 100e3, 17), np.linspace(0.0, 4200.0, 70)
    cin = ttr.traced_tables(env, False, False)[0]
    for col in (-1, 50):
        a = pr.travel_time_kernel(dev, env, g, h, flatearth=False, range_index=col)
        b = pr.travel_time_kernel(host, env, g, h, flatearth=False, range_index=col)
        assert a.shape[0] == len(dev) and _same(a, b)
        assert _same(b, ttr.fan_kernel(host, env, g, h, flatearth=False, range_index=col))
        K = pr.travel_time_kernel(dev, env, flatearth=False, range_index=col)
        _identity(K, cin, host, col)
    assert dev.device_resident


def test_flat_earth_default_environment(pr):
    """the default environment in its flat-earth frame (non-uniform zin: the look-up's longer search): the default-grid
    identity for every ray; device fan == host fan == restatement on a few rays of a user grid"""
    env = pr.OceanEnvironment2D()
    ang = np.linspace(-15, 15, 24)
    dev = pr.shoot_rays(1000.0, 0.0, ang, 100e3, 501, env, debug=False, device_resident=True)
    host = pr.shoot_rays(1000.0, 0.0, ang, 100e3, 501, env, debug=False, device_resident=False)
    cin, rin, zin = ttr.traced_tables(env, True, False)
    assert np.ptp(np.diff(zin)) > 0
    K = pr.travel_time_kernel(dev, env)
    assert K.shape == (len(host), len(rin), len(zin)) and np.isfinite(K).all()
    _identity(K, cin, host)
    assert _same(K, pr.travel_time_kernel(host, env))
    few = pr.RayFan.from_arrays(*(np.asarray(getattr(host, n))[::8] for n in ("thetas", "rs", "ts", "zs", "ps", "n_botts",
                                                                             "n_surfs", "source_depths")))
    g, h = np.linspace(0.0, 100e3, 11), np.linspace(0.0, 5000.0, 40)
    assert _same(pr.travel_time_kernel(dev, env, g, h)[::8], ttr.fan_kernel(few, env, g, h))
