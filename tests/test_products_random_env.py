"""The ray-tube products -- transmission_loss, beam_transmission_loss, arrivals (csrc/pgr_tl.h, pgr_beams.h, pgr_arrivals.h) --
on the random environments of helpers.random_case: tables starting at -400 km, mirrored (negative, reversed) ranges, random
non-uniform range grids, stretched and power-of-two depth grids, the bathymetry on a range grid of its own.  Bit for bit,
NaN patterns and integer counts included, in the reference arithmetic only.

Three levels.  The kernels on raw tables: the buffer entries on a fan shot through the host-pointer entry against the NumPy
restatements given the same raw tables -- no frame helper on either side.  The fan entries (results in HBM, rows or
sample-blocked, dropped rays through the keep list) against the buffer entries.  The API: pr.shoot_rays forwards and
backwards, flatearth on and off, device resident or not, then the three products against the same restatements fed by
tests/frame_independent.py -- a derivation of the traced frame that shares no code with pygenray_amd/transmission.py.

The seeds were chosen with the CPU oracle and the restatements alone (DESIGN.md section 4 lists them and what they hold);
the conditions that keep the sweep from being vacuous are asserted here.  A seed on which the device disagrees is a finding
and stays in the list."""
import numpy as np
import pytest

import arrivals_reference as aref
import beam_reference as bref
import frame_independent as fi
import oracle
import tl_reference as tlr
from helpers import random_case, y0_for
from tube_gpu import _device_arrivals, _device_beams, _device_intensity, _same, _upload, pr  # noqa: F401  (pr: fixture)

pytestmark = pytest.mark.gpu

# (seed of helpers.random_case, passed through the flat-earth map first).  Chosen on the CPU, before any device run, by a
# rule the device has no say in: the first 28 seeds from 200 on as they are and the first 12 from 400 on flat-earth mapped
# whose ORACLE fan (oracle.MATH_CR) keeps >= 64 rays and, through the restatements, fills >= 12 % of the TL entries, emits
# >= 3 arrivals and has >= 6 bouncing rays.  Passed over: 200, 201, 207, 222 and (flat) 404 -- no ray bounces; 238 -- its
# sound-speed axis drifts out of the table and no ray survives.  DESIGN.md section 4 has the composition.
CASES = [(s, False) for s in (202, 203, 204, 205, 206, 208, 209, 210, 211, 212, 213, 214, 215, 216, 217, 218, 219, 220, 221,
                              223, 224, 225, 226, 227, 228, 229, 230, 231)] + \
        [(s, True) for s in (400, 401, 402, 403, 405, 406, 407, 408, 409, 410, 411, 412)]
# the API level: the first 12 un-mirrored seeds of CASES whose four frames (forwards / backwards x flatearth off / on) each
# meet the same conditions on the oracle's fan, with the latitude of the environment's flat-earth map
LATITUDES = (35.0, -52.5, 0.0, 71.0)
API_CASES = [(s, LATITUDES[s % 4]) for s in (202, 203, 204, 205, 208, 209, 210, 211, 213, 214, 215, 216)]
LAT = 35.0
N_GRID, N_ON_SAMPLES = 160, 48          # receivers per case: a grid, and depths taken from the fan's own samples
MIN_WIDTHS = (10.0, 4.0, 25.0)


def n_rays_of(seed):
    return 128 + (seed * 53) % 273       # 128 ... 400


def case_inputs(seed, flat):
    """-> (arrs, y0, shot kwargs, description, mirrored): random_case(seed) with n_rays_of(seed) rays, its tables passed
    through the flat-earth map (frame_independent's, LAT) when `flat`"""
    arrs, (src, x0, th), kw, desc = random_case(seed, n_rays=n_rays_of(seed))
    if flat:
        cin, cpin, rin, zin, depths, dr, ba = arrs
        zf = fi.flat_depth(zin, LAT)
        cf = np.stack([fi.flat_speed(row, zin, LAT) for row in cin])
        arrs = [cf, np.gradient(cf, zf, axis=1, edge_order=1), rin, zf, fi.flat_depth(depths, LAT), dr, ba]
    return arrs, y0_for(oracle, arrs, src, x0, th), kw, desc, "mirrored True" in desc


def receivers(zs, deepest_floor, seed):
    """Receiver depths of a fan with stored depths zs (M, S): a grid from above the surface to below the deepest floor
    and, as tube_gpu.synthetic_fan does, depths taken from the fan's own samples (one tube's lo, another's hi) -> strictly
    ascending."""
    rng = np.random.default_rng(seed)
    grid = np.linspace(-120.0, deepest_floor + 150.0, N_GRID)
    d = -np.asarray(zs)[:, 1:]
    fin = d[np.isfinite(d)]
    on = rng.choice(fin, N_ON_SAMPLES, replace=len(fin) < N_ON_SAMPLES) if len(fin) else np.zeros(0)
    return np.unique(np.concatenate([grid, on]))


def columns(S):
    """the requested save columns: the last, one inside, the source's own (no arrivals there)"""
    return list(dict.fromkeys([S - 1, S // 2, 0]))


def restatements(ts, zs, ps, xf, p0, depths, cols, cin, rin, zin, bottom, w_min):
    """the three NumPy restatements on a fan (M, S) in the stored convention and the tables of its frame"""
    return (tlr.tube_intensity(zs, ps, xf, p0, depths, cin, rin, zin),
            bref.beam_intensity(zs, ps, xf, p0, depths, cin, rin, zin, bottom, w_min),
            aref.tube_arrivals(zs, ps, ts, xf, p0, depths, cols, cin, rin, zin))


def not_vacuous(I, arr, n_bounce, xf, label):
    """the conditions every case meets -> (TL fill fraction outside the source column, arrivals emitted)"""
    fill = float((I[:, np.asarray(xf) != xf[0]] > 0).mean())
    n_arr = int(arr["offsets"][-1])
    assert fill >= 0.10, f"{label}: only {fill:.3f} of the TL entries outside the source column are > 0"
    assert n_arr >= 1, f"{label}: no arrival"
    assert int((np.asarray(n_bounce) > 0).sum()) >= 5, f"{label}: fewer than 5 rays bounce"
    return fill, n_arr


def same_arrivals(a, b, label):
    assert np.array_equal(a["offsets"], b["offsets"]), f"{label}: arrival counts"
    for k in ("tube", "w", "T", "p", "I"):
        assert a[k].shape == b[k].shape and _same(a[k], b[k]), f"{label}: arrivals' {k}"


def _fan_products(h, env, p0, bottom, depths, cols, w_min):
    """the four fan entries of a FanHandle -> (I, B, arrivals dict), as tube_gpu's helpers return the buffer entries'"""
    import torch
    (d_p0, d_b, d_d), stream = _upload(env, p0, bottom, depths)
    dev = d_p0.device
    R, n, S = len(depths), len(cols), h.S
    I = torch.full((R, S), -1.0, dtype=torch.float64, device=dev)
    B = torch.full((R, S), -1.0, dtype=torch.float64, device=dev)
    h.intensity(d_p0.data_ptr(), d_d.data_ptr(), R, I.data_ptr(), stream)
    h.beam_intensity(d_p0.data_ptr(), d_b.data_ptr(), d_d.data_ptr(), R, w_min, B.data_ptr(), stream)
    counts = torch.full((R * n,), -1, dtype=torch.int64, device=dev)
    h.arrival_counts(d_p0.data_ptr(), d_d.data_ptr(), R, cols, counts.data_ptr(), stream)
    offsets = torch.zeros(R * n + 1, dtype=torch.int64, device=dev)
    torch.cumsum(counts, 0, out=offsets[1:])
    total = int(offsets[-1].item())
    out = dict(offsets=offsets.cpu().numpy(), tube=np.zeros(0, np.int32), w=np.zeros(0), T=np.zeros(0), p=np.zeros(0),
               I=np.zeros(0))
    if total:
        tube = torch.full((total,), -1, dtype=torch.int32, device=dev)
        f = [torch.full((total,), -1.0, dtype=torch.float64, device=dev) for _ in range(4)]
        h.arrivals(d_p0.data_ptr(), d_d.data_ptr(), R, cols, offsets.data_ptr(), total, tube.data_ptr(),
                   *(a.data_ptr() for a in f), stream)
        out.update(tube=tube.cpu().numpy(), **{k: a.cpu().numpy() for k, a in zip(("w", "T", "p", "I"), f)})
    return I.cpu().numpy(), B.cpu().numpy(), out


def test_kernels_and_fan_entries_on_random_raw_tables(pr):
    """Per case: the fan of random_case shot on the raw tables (host-pointer entry, sample-major, stored sign), its surviving
    rays fed to intensity_device, beam_intensity_device, arrival_counts_device and arrivals_device against the restatements
    on the same raw arrays; then the same fan as a FanHandle and its four entries against the buffer entries."""
    from pygenray_amd import _lib
    tally = dict(hbm=0, lds=0, blocked=0, mirrored=0, offset=0, nonuniform=0, flat=0, dropped=0, rays=0, arrivals=0)
    fills = []
    for seed, flat in CASES:
        arrs, y0, kw, desc, mirrored = case_inputs(seed, flat)
        cin, cpin, rin, zin, bdep, brng, bang = arrs
        label = f"seed {seed}{' (flat earth)' if flat else ''}: {desc}"
        env = _lib.EnvHandle(*arrs)
        shot = dict(rtol=kw["rtol"], terminate_backwards=kw["terminate_backwards"])
        g = env.shoot_fan(y0, kw["x0"], kw["x1"], kw["S"], sample_major=True, stored_sign=True, **shot)
        keep = g["status"] == 0
        M, S = int(keep.sum()), kw["S"]
        assert M >= 64, label
        T, z, p = (np.ascontiguousarray(g[k][:, keep]) for k in "Tzp")       # (S, M)
        assert np.isfinite(z).all() and np.isfinite(T).all(), label
        x, p0 = g["r"], y0[keep, 2]
        depths = receivers(z.T, float(bdep.max()), seed)
        cols, w_min = columns(S), MIN_WIDTHS[seed % 3]
        bottom = fi.bottom_at(x, bdep, brng)
        # the buffer entries against the restatements on the raw tables
        I = _device_intensity(env, z, p, x, p0, depths)
        B = _device_beams(env, z, p, x, p0, bottom, depths, w_min)
        A = _device_arrivals(env, T, z, p, x, p0, depths, cols)
        rI, rB, rA = restatements(T.T, z.T, p.T, x, p0, depths, cols, cin, rin, zin, bottom, w_min)
        bad = ~((I == rI) | (np.isnan(I) & np.isnan(rI)))
        assert not bad.any(), (label, "intensity", np.argwhere(bad)[:5], I[bad][:5], rI[bad][:5])
        bad = ~((B == rB) | (np.isnan(B) & np.isnan(rB)))
        assert not bad.any(), (label, "beams", np.argwhere(bad)[:5], B[bad][:5], rB[bad][:5])
        same_arrivals(A, rA, label)
        fill, n_arr = not_vacuous(rI, rA, (g["n_bott"] + g["n_surf"])[keep], x, label)
        # the fan entries against the buffer entries
        h = _lib.FanHandle(env, kw["x0"], kw["x1"], S, y0=y0, stored_sign=True, **shot)
        assert h.wait() == (len(y0), M), label
        hI, hB, hA = _fan_products(h, env, p0, bottom, depths, cols, w_min)
        assert _same(hI, I) and _same(hB, B), label
        same_arrivals(hA, A, label + " (fan entries)")
        h.close()
        nonuniform = float(np.ptp(np.diff(rin))) > 1e-6 * float(np.mean(np.diff(rin)))
        offset = abs(rin[-1] if mirrored else rin[0])
        for k, hit in (("hbm", not env.lds_path), ("lds", env.lds_path), ("blocked", env.blocked_layout), ("mirrored", mirrored),
                       ("offset", offset > 100e3), ("nonuniform", nonuniform), ("flat", flat), ("dropped", M < len(y0))):
            tally[k] += bool(hit)
        tally["rays"] += M
        tally["arrivals"] += n_arr
        fills.append(fill)
        env.close()
    print(f"\n{len(CASES)} random environments: {tally}; TL fill fraction {min(fills):.3f} ... {max(fills):.3f} "
          f"(mean {np.mean(fills):.3f})")
    for k, least in (("hbm", 6), ("lds", 6), ("blocked", 6), ("mirrored", 6), ("offset", 6), ("nonuniform", 6), ("flat", 6),
                     ("dropped", 4)):
        assert tally[k] >= least, (k, tally)


@pytest.mark.parametrize("seed, lat", API_CASES, ids=[f"seed{s}" for s, _ in API_CASES])
def test_api_products_against_frames_derived_by_hand(pr, seed, lat):
    """The un-mirrored seeds as an OceanEnvironment2D (bathymetry on its own range grid): pr.shoot_rays forwards (the case's
    source range to its receiver range) and backwards (from the receiver range back), flatearth on and off, device resident
    and not, the source depth, tolerance, save grid and launch angles where the case puts them; then transmission_loss,
    beam_transmission_loss and arrivals against the restatements on the frame frame_independent.py derives."""
    arrs, (src, x0, th), kw, desc = random_case(seed, n_rays=n_rays_of(seed))
    assert "mirrored False" in desc
    cin, cpin, rin, zin, bdep, brng, bang = arrs
    env = pr.OceanEnvironment2D(pr.DataArray(cin, dims=["range", "depth"], coords={"range": rin, "depth": zin}),
                                pr.DataArray(bdep, dims=["range"], coords={"range": brng}), lat=lat)
    S, w_min = kw["S"], MIN_WIDTHS[seed % 3]
    cols = columns(S)
    for backwards in (False, True):
        xs, xr = (kw["x1"], kw["x0"]) if backwards else (kw["x0"], kw["x1"])
        for fe in (False, True):
            label = f"seed {seed} {'backwards' if backwards else 'forwards'} flatearth={fe}: {desc}"
            fans = [pr.shoot_rays(src, xs, th, xr, S, env, rtol=kw["rtol"], terminate_backwards=kw["terminate_backwards"],
                                  debug=False, flatearth=fe, device_resident=dr) for dr in (False, True)]
            host, dev = fans
            assert not host.device_resident and dev.device_resident and len(host) == len(dev) >= 64, label
            x = np.asarray(host.rs, dtype=float)[0]
            assert x[0] == xs and x[-1] == xr
            xf, fcin, frin, fzin, fbd, fbr = fi.traced_frame(env, x, fe)
            p0 = fi.launch_slowness(host.thetas, host.source_depths[0], xf, fcin, frin, fzin)
            depths = receivers(host.zs, float(fbd.max()), seed)
            rI, rB, rA = restatements(host.ts, host.zs, host.ps, xf, p0, depths, cols, fcin, frin, fzin,
                                      fi.bottom_at(xf, fbd, fbr), w_min)
            not_vacuous(rI, rA, np.asarray(host.n_botts) + np.asarray(host.n_surfs), xf, label)
            for fan, where in ((dev, "device fan"), (host, "host fan")):
                I = pr.transmission_loss(fan, depths, env, flatearth=fe, intensity=True)
                B = pr.beam_transmission_loss(fan, depths, env, flatearth=fe, intensity=True, min_width=w_min)
                a = pr.arrivals(fan, depths, env, flatearth=fe, range_indices=cols)
                assert fan.device_resident == (fan is dev), label           # processed where it is
                assert _same(I, rI), (label, where, "transmission_loss")
                assert _same(B, rB), (label, where, "beam_transmission_loss")
                same_arrivals(dict(offsets=a.offsets, tube=a.tube, w=a.w, T=a.time, p=a.p, I=a.intensity), rA,
                              f"{label} ({where})")
