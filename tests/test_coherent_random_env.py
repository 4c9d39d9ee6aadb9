"""The products added since the random-environment sweep of test_products_random_env.py -- the path integral (csrc/pgr_path.h),
the bounce post-pass with its per-sample counts (pgr_bounce.h), the caustic scan and the coherent tube sum (pgr_phase.h), the
pulse and band sums (pgr_signal.h, pgr_spectrum.h), the three sums with a bottom lag (pgr_reflect.h) and the coherent beam sum
with and without its curvature term (pgr_beam_phase.h: beam_pressure_device, FanHandle.beam_pressure, beam_pressure_field,
coherent_beam_transmission_loss; min_width MIN_WIDTHS[seed % 3]) and the terms of that sum listed as arrivals, with the pulse
and band sums over the list (pgr_beam_arrivals.h: beam_arrival_counts_device, beam_arrivals_device, the two FanHandle entries,
beam_arrivals, beam_received_signal, beam_transfer_function) -- on that sweep's
environments: tables starting at -400 km, mirrored (negative, reversed) frames, non-uniform range grids, stretched and
power-of-two depth grids, the bathymetry on a grid of its own, flat-earth mapped tables.  Bit for bit, NaN patterns and integers
included, in the reference arithmetic only.  The cases, receivers and columns are test_products_random_env.py's own objects.

Every weight at once.  Per case, each a fixed function of the seed: the bottom is fluid_halfspace(1700, 1800, 0.5) on even seeds
and a hand-made BottomReflection on odd ones (nodes 2 ... 80 degrees, inside (0, 90), and a lag that is not monotone); 0.25 dB per
surface bounce; a three-node absorption profile at 0.1 / 0.5 / 0.9 of the frame's deepest floor; 25, 75 or 237.5 Hz; a pulse of
10 or 40 Hz on 65 samples dt = sigma / 2 apart that start 32 dt before the median restated arrival time of each column (the
range over 1500 m/s where a column has none); 65 frequencies descending from 1.2 f to 0.8 f with t_reduce = that start and
Thorp's absorption; at most 64 receivers, the depths taken from the fan's own samples (exactly on tube edges) all kept.

Level 1 (one test per case): random_case's fan shot as a FanHandle with a bounce log -- its samples against the un-logged
host-pointer shot, every 8th bouncing ray's log against the oracle's step trace -- then the buffer entries on the surviving
rays' rows and the fetched log against the NumPy restatements on the same raw tables, the _phi entries at a lag of zero against
their siblings, and the handle's own entries (rows or sample-blocked, dropped rays through the keep list) against the buffer
entries.  The beam sums are written between sentinels, and once with neither weights nor q.  The beam arrivals: four lists by
count, exclusive scan and emit (BEAM_LISTS: W and q with and without the curvature term, neither weights nor q, Wb and q), the
counts and the five arrays between sentinels, against beam_arrivals_reference.beam_arrivals, which is written from the
definition with every tube at once; the weighted lists summed by spectrum_device at the one frequency f, I = amp * amp formed
with torch, against beam_pressure_device's own field and the tube-by-tube restatement's on the requested columns (two
independent references and two kernels tied together); signal_device over the curvature-1 list against signal_sum over the
restated list; spectrum_device over the Wb list with Thorp's alpha and L0 + 0.5 (L1 - L0) of the device's path lengths
against spectrum_sum over the restated list with the restated mean lengths; then all of it through the handle, equal.
Level 2 (API_CASES x forwards / backwards x flatearth off / on): pr.shoot_rays with a log, device resident and not,
against the un-logged fan, then every public product on both fans against the restatements fed by tests/frame_independent.py
alone: frame, launch slowness and bottom slope there share no code with the package.  The beams take the loss pair of the
bottom (a BottomReflection is refused, once per frame).  beam_arrivals with and without the curvature term (every array, the
echoed range_indices, ranges, intensity = amplitude ** 2, nothing in the source's column; the host fan is asked for the last
column as -1), beam_transfer_function at [f] equal to the beam field on the requested columns, beam_received_signal and
beam_transfer_function with t_reduce and Thorp's absorption against the restated sums over the restated lists.
beam_arrivals_reference.fan_beam_arrivals, which takes its frame from the package, is not used here.

The sign of p.  The restatements read p by the convention the kernels were written under, so a shared sign error would pass
every comparison above.  beam_pressure_reference.eikonal_share holds it by the eikonal equation alone: at a fixed range
T_k+1 - T_k and p_m (d_k+1 - d_k) have one sign on at least EIKONAL_SHARE of the eligible tubes of every fan (measured: 0.80
at the least; the other convention gives one minus the share).  test_fan_entries_agree_in_either_sign then launches every
level-1 fan a second time WITHOUT PGR_STORED_SIGN and holds every pgr_fan_* entry to the stored-sign handle, bit for bit.

The seed rule.  A case stays when its ORACLE fan (oracle.MATH_CR; its log from bounce_reference.trace_bounces with the case's
own rtol and terminate_backwards) meets, through the restatements alone, the conditions not_vacuous() asserts: at the last
column >= 20 bounced tubes with q >= 0, a tube with q = -1 and a caustic index >= 1; a non-zero field on at least half of the
cells outside the source column with a non-zero TL intensity; a requested column whose pulse window holds an arrival that adds.
cpu_check() re-runs that rule without a GPU (from the repository root: PYTHONPATH=. python tests/test_coherent_random_env.py).
For the beam sum the rule adds, over the columns other than the source's: at least half of the cells finite, at least half of
those non-zero, an otherwise valid tube with q < 0, and the curvature term changing at least half of the non-zero cells; over
the sweep, 30 of the 40 cases each with a kept surface image, a kept bottom image, and tubes both at the floor min_width and
above it (39 each on the oracle's fans).
For the beam arrivals the rule adds (ARRIVAL_RULES, from the restated lists alone; no case is exempt, an infinite amplitude is
an arrival like any other): at least 1000 arrivals, none at the source's column, at least half of the (receiver, column) groups
away from the source lit, no amplitude whose square is subnormal and no NaN time, the curvature term changing at least half of
the times, a requested column whose pulse window (+- 8 sigma) holds a beam arrival and a pulse sum that is not zero everywhere,
and the restated weighted lists summed at f equal to the tube-by-tube restatement's BP / BP_linear bit for bit (which a wrong
sign of p_m in a copy of the list's restatement breaks on every case tried: every time changes and nothing else); over the
sweep, 30 of the 40 cases each with a surface-image and a bottom-image arrival, and every emitted q 0 ... 3 seen.  On the
oracle's fans: 1122 (seed 228) ... 43 879 (seed 226) arrivals at level 1, lit groups 0.78 (seed 213) ... 1, 39 cases each with
a surface image (not 228) and a bottom image (not 204), 1934 and 1668 infinite amplitudes on seeds 202 and 225; the 48 frames
1402 ... 35 113 arrivals, lit groups 0.625 (seed 213 backwards) ... 1, both columns away from the source with a pulse in every
frame, 1529 ... 2432 infinite amplitudes in seed 202's four frames.
Passed over: none -- not one of the 40 cases or of the 12 API seeds (all four frames of each) missed a condition of the first
paragraph or of the beam arrivals'.  Exempt from the beam conditions alone, and still compared bit for bit: seed 225 at level 1 -- it saves two columns
and its path integral is -9.9e6 dB on 39 rays of the lit one, so their weights 10^(-(A + B) / 10) overflow; 56 live tubes hold
such a ray, three of them 2.0 - 2.9 km wide and within 4 sigma of all 64 receivers, and inf - inf makes every cell NaN (the
tube sum, a top hat, stays finite at 5 receivers) -- and seed 202 at level 2, whose weights overflow in the same way: 6 - 12 %
of its cells are finite in the four frames (54 % at level 1, where it meets the rule).  A seed on
which the device disagrees is a finding and stays in the list: seed 202, whose weights overflow, found a division that made
inf / finite a NaN (which also has the composition and the tallies of the MI355X run)."""
import numpy as np
import pytest

import beam_arrivals_reference as ba
import beam_pressure_reference as bpr
import bounce_reference as bref
import coherent_reference as cref
import frame_independent as fi
import oracle
import path_reference as pref
import reflection_reference as rref
import signal_reference as sref
import spectrum_reference as spref
from helpers import random_case, sign_flipped, y0_for
from test_products_random_env import (API_CASES, CASES, MIN_WIDTHS, N_GRID, case_inputs, columns, n_rays_of, receivers,
                                      same_arrivals)
from tube_gpu import _same, _upload, pr  # noqa: F401  (pr: fixture)

pytestmark = pytest.mark.gpu

PASSED_OVER, PASSED_OVER_API = (), ()                     # (seed, flat) of CASES / seeds of API_CASES the rule above drops
LEVEL1 = [c for c in CASES if c not in PASSED_OVER]
LEVEL2 = [c for c in API_CASES if c[0] not in PASSED_OVER_API]
assert len(PASSED_OVER) <= 8 and len(PASSED_OVER_API) <= 3
# (seed, flat) of LEVEL1 / seeds of LEVEL2 that stay in every comparison and are exempt from the beam conditions of the rule
BEAM_EXEMPT, BEAM_EXEMPT_API = ((225, False),), (202,)
assert len(BEAM_EXEMPT) <= 2 and len(BEAM_EXEMPT_API) <= 1
EIKONAL_SHARE = 0.70                                      # the least share of tubes on which dT and p_m dd agree in sign

FREQUENCIES, BANDWIDTHS = (25.0, 75.0, 237.5), (10.0, 40.0)
SURFACE_DB = 0.25
ABS_AT, ABS_DB_PER_KM = np.array([0.1, 0.5, 0.9]), np.array([0.02, 0.07, 0.04])
N_TIMES = N_FREQ = 65
LEAD = 32                                                 # samples of the time axis before the median arrival
# the odd seeds' bottom: grazing nodes that end at neither 0 nor 90, |R|, arg R in degrees -- the lag -arg R / 360 is
# 0.417, 0.056, 0.208, 0.014 cycles: not monotone
HAND_MADE = ([2.0, 11.0, 35.0, 80.0], [0.9, 0.55, 0.35, 0.5], [-150.0, -20.0, -75.0, -5.0])
MAX_ROWS = 400000                                         # step attempts of the oracle's trace of the longest rays
MARK = -7.25
PAD = 130                                                 # entries either side of a beam output that must stay as they were
BEAM_KEYS = ("tube", "image", "time", "amplitude", "q")   # a beam-arrival list's arrays, in the order the emit entries take them


def bottom_of(pr, seed):  # noqa: F811
    return pr.fluid_halfspace(1700.0, 1800.0, 0.5) if seed % 2 == 0 else pr.BottomReflection(*HAND_MADE)


def absorption_of(deepest_floor):
    """the absorption profile as the public functions take it: (depths in metres, dB/km)"""
    return ABS_AT * deepest_floor, ABS_DB_PER_KM.copy()


def band_of(f):
    return np.linspace(1.2 * f, 0.8 * f, N_FREQ)


def thinned_receivers(zs, deepest_floor, seed):
    """receivers() thinned to at most 64 depths: every depth taken from the fan's own samples and every 10th of the grid"""
    d = receivers(zs, deepest_floor, seed)
    grid = np.linspace(-120.0, deepest_floor + 150.0, N_GRID)
    out = d[~np.isin(d, grid) | np.isin(d, grid[::10])]
    assert len(out) <= 64 and np.all(np.diff(out) > 0)
    return out


_complex = cref.as_complex          # re + i im with each part's own bits


def restate(fan, frame, beta, bottom, seed, depths, cols, w_min=None):
    """Every product from the NumPy restatements alone.  fan: dict(ts, zs, ps (M, S) stored convention, x (S,) the traced
    frame's save ranges, p0 (M,), log = (bx, bp, bk) (M, K) stored sign); frame: (cin, rin, zin, bottom depths, their ranges);
    beta: (ranges, degrees); bottom: a BottomReflection, read for its two tables only.  w_min: also the Gaussian beams."""
    with np.errstate(invalid="ignore", over="ignore"):          # (NaN columns at the source, weights that underflow)
        return _restate(fan, frame, beta, bottom, seed, depths, cols, w_min)


def _restate(fan, frame, beta, bottom, seed, depths, cols, w_min):
    ts, zs, ps, xf, p0 = fan["ts"], fan["zs"], fan["ps"], np.asarray(fan["x"], dtype=float), fan["p0"]
    bx, bp, bk = fan["log"]
    cin, rin, zin, bd, br = frame
    f, band = FREQUENCIES[seed % 3], BANDWIDTHS[seed % 2]
    r = dict(f=f, absorption=absorption_of(float(np.max(bd))))
    a_depths, alpha = pref.profile_db_per_m(r["absorption"])
    r["A"] = pref.path_integral(ts, zs, xf, a_depths, alpha, cin, rin, zin)
    r["L"] = pref.path_integral(ts, zs, xf, None, np.ones(1), cin, rin, zin)
    r["tables_db"] = (tuple(bottom.loss), (None, np.array([SURFACE_DB])), beta)
    r["tables_lag"] = (tuple(bottom.lag), (None, np.zeros(1)), beta)
    r["B"], r["nb"], r["ns"] = bref.boundary_loss(bx, bp, bk, xf, cin, rin, zin, br, bd, *r["tables_db"])
    r["Phi"] = rref.ray_lags(bx, bp, bk, xf, cin, rin, zin, br, bd, r["tables_lag"][0], beta)
    nb, ns = r["nb"], r["ns"]
    W, Wb = r["W"], r["Wb"] = pref.weights(r["A"] + r["B"]), pref.weights(r["B"])
    r["kappa"] = cref.caustic_index(-zs, nb, ns)
    q = r["q"] = cref.tube_phase(r["kappa"], nb, ns)
    r["P"] = _complex(*rref.tube_pressure(zs, ps, ts, xf, p0, depths, cin, rin, zin, W, q, f, r["Phi"]))
    r["P_plain"] = _complex(*cref.tube_pressure(zs, ps, ts, xf, p0, depths, cin, rin, zin, None, q, f))
    r["I"] = pref.tube_intensity(zs, ps, xf, p0, depths, cin, rin, zin, W)
    r["eikonal"] = bpr.eikonal_share(zs, ps, ts, nb, ns, xf, detail=True)
    if w_min is not None:
        floor = fi.bottom_at(xf, bd, br)
        r["beams"] = pref.beam_intensity(zs, ps, xf, p0, depths, cin, rin, zin, floor, w_min, W)
        # the coherent beams: with the curvature term (and the counters of its kept terms) and without it, on every column;
        # and with neither weights nor q on the requested columns behind the source's own
        tab = (p0, depths, cin, rin, zin)
        *field, _, _, r["beam_detail"] = bpr.beam_pressure(zs, ps, ts, xf, *tab, floor, w_min, W, q, f, True, detail=True)
        r["BP"], r["w_min"] = _complex(*field), w_min
        r["BP_linear"] = _complex(*bpr.beam_pressure(zs, ps, ts, xf, *tab, floor, w_min, W, q, f, False))
        sel = [0] + [c for c in cols if c != 0]
        bare = _complex(*bpr.beam_pressure(zs[:, sel], ps[:, sel], ts[:, sel], xf[sel], *tab, floor[sel], w_min, None, None, f))
        r["BP_bare"] = bare[:, [sel.index(c) for c in cols]]
        # the beam arrivals from the definition, every tube at once: with and without the curvature term, with neither weights
        # nor q, and without volume absorption in the weights
        for name, w_, q_, curvature in BEAM_LISTS:
            r[name] = ba.beam_arrivals(zs, ps, ts, xf, p0, depths, cin, rin, zin, floor, w_min,
                                       {"W": W, "Wb": Wb, None: None}[w_], None if q_ is None else q, cols, curvature)
    arr = r["arr"] = pref.tube_arrivals(zs, ps, ts, xf, p0, depths, cols, cin, rin, zin, W)
    r["arr_b"] = pref.tube_arrivals(zs, ps, ts, xf, p0, depths, cols, cin, rin, zin, Wb)       # (no volume absorption)
    # per arrival: the phase index, the lag and the path length of its tube at its column
    R, n = len(depths), len(cols)
    off, k, w = arr["offsets"], arr["tube"].astype(np.int64), arr["w"]
    slot = np.repeat(np.arange(R * n), np.diff(off)) % n
    col = np.asarray(cols, dtype=np.int64)[slot]
    r["slot"], r["col"] = slot, col
    r["qa"] = q[k, col]
    r["phi"] = rref.arrival_lag(r["Phi"][k, col], r["Phi"][k + 1, col], w)
    r["La"] = spref.arrival_lengths(r["L"][k, col], r["L"][k + 1, col], w)
    # the pulse and the band
    sigma = sref.pulse_sigma(band)
    dt = r["dt"] = 0.5 * sigma
    r["band"], r["rs"], r["sigma"] = band, sref.inv_sigma(band), sigma
    r["t0"] = np.array([(np.median(arr["T"][slot == c]) if (slot == c).any() else abs(xf[cols[c]] - xf[0]) / 1500.0)
                        - LEAD * dt for c in range(n)])
    r["freq"] = band_of(f)
    r["u_raw"] = rref.signal_sum(off, arr["T"], arr["I"], r["qa"], r["phi"], np.tile(r["t0"], R), f, r["rs"], dt,
                                 N_TIMES).reshape(R, n, N_TIMES)
    if w_min is not None:
        # the beam list summed: at the one frequency f without a reduction (the field itself), by the pulse, and -- the list
        # without volume absorption, with the mean path length of each arrival's tube -- by the band (beam_band_sum)
        a, a_b = r["ba"], r["ba_b"]
        r["ba_field"] = spref.spectrum_sum(a["offsets"], a["time"], a["amplitude"] * a["amplitude"], a["q"], None,
                                           np.zeros(R * n), [f], None).reshape(R, n)
        lin = r["ba_linear"]
        r["ba_field_linear"] = spref.spectrum_sum(lin["offsets"], lin["time"], lin["amplitude"] * lin["amplitude"], lin["q"], None,
                                                  np.zeros(R * n), [f], None).reshape(R, n)
        r["bu_raw"] = sref.signal_sum(a["offsets"], a["time"], a["amplitude"] * a["amplitude"], a["q"], np.tile(r["t0"], R), f,
                                      r["rs"], dt, N_TIMES).reshape(R, n, N_TIMES)
        kb = a_b["tube"].astype(np.int64)
        colb = np.asarray(cols, dtype=np.int64)[np.repeat(np.arange(R * n), np.diff(a_b["offsets"])) % n]
        r["bLa"] = spref.arrival_lengths(r["L"][kb, colb], r["L"][kb + 1, colb], 0.5)
    return r


def band_sum(r, alpha, R, n):
    """the band sum of restate()'s arrivals without volume absorption in the tube weights, alpha (F,) dB/m per frequency"""
    a = r["arr_b"]
    return rref.spectrum_sum(a["offsets"], a["T"], a["I"], r["qa"], r["phi"], r["La"], np.tile(r["t0"], R), r["freq"],
                             alpha).reshape(R, n, N_FREQ)


def beam_band_sum(r, alpha, R, n):
    """the band sum of restate()'s beam arrivals without volume absorption in the weights, alpha (F,) dB/m per frequency"""
    a = r["ba_b"]
    return spref.spectrum_sum(a["offsets"], a["time"], a["amplitude"] * a["amplitude"], a["q"], r["bLa"], np.tile(r["t0"], R),
                              r["freq"], alpha).reshape(R, n, N_FREQ)


def at_source_nan(v, xf, cols):
    """(R, n, m) raw sums -> what the public functions return: NaN in the source's own columns"""
    v = v.copy()
    v[:, np.abs(np.asarray(xf)[np.asarray(cols)] - xf[0]) == 0, :] = complex(np.nan, np.nan)
    return v


def figures(r, xf, cols):
    """the quantities of the seed rule, from restate()'s results alone"""
    nb, ns, q = r["nb"], r["ns"], r["q"]
    bounced = (nb[:-1, -1] + ns[:-1, -1]) > 0
    lit = r["I"][:, np.asarray(xf) != xf[0]] > 0
    field = np.abs(r["P"][:, np.asarray(xf) != xf[0]]) > 0
    a = r["arr"]
    t_end = r["t0"] + (N_TIMES - 1) * r["dt"]
    inside = (r["qa"] >= 0) & (a["T"] >= r["t0"][r["slot"]] - 8.0 * r["sigma"]) & (a["T"] <= t_end[r["slot"]] + 8.0 * r["sigma"])
    fig = dict(bounced_tubes=int((bounced & (q[:-1, -1] >= 0)).sum()), left_out=int((q[:-1, -1] == -1).sum()),
                kappa_max=int(r["kappa"][:, -1].max()), kappa_max_anywhere=int(r["kappa"].max()),
                field_fill=float(field[lit].mean()) if lit.any() else 0.0, lit=int(lit.sum()),
                columns_with_a_pulse=int(len(np.unique(r["slot"][inside]))), pulse_lit=bool((np.abs(r["u_raw"]) > 0).any()),
                arrivals=int(a["offsets"][-1]), lag=bool((r["phi"] > 0).any()), surface=bool((ns[:, -1] > 0).any()),
                bottom=bool((nb[:, -1] > 0).any()), most_bounces=int((nb[:, -1] + ns[:, -1]).max()),
                eikonal_share=r["eikonal"][0], eikonal_tubes=r["eikonal"][1])
    if "BP" in r:
        fig.update(beam_figures(r, xf))
        fig.update(beam_arrival_figures(r, xf, cols))
    return fig


def beam_figures(r, xf):
    """the beam sum's quantities of the seed rule, over the columns other than the source's"""
    away = np.asarray(xf) != xf[0]
    P, Pl, dt = r["BP"][:, away], r["BP_linear"][:, away], r["beam_detail"]
    finite = np.isfinite(P.real) & np.isfinite(P.imag)
    nonzero = finite & ((P.real != 0) | (P.imag != 0))
    curved = (P.real != Pl.real) | (P.imag != Pl.imag)
    live, sigma = dt["live"], dt["sigma"]                      # (tubes of the source's column are not live)
    return dict(beam_finite=float(finite.mean()), beam_nonzero=float(nonzero.sum() / max(1, finite.sum())),
                beam_left_out=int((dt["valid"] & ~live).sum()),
                beam_curved=float(curved[nonzero].mean()) if nonzero.any() else 0.0,
                surface_image=bool((dt["kept"][1][live] > 0).any()), bottom_image=bool((dt["kept"][2][live] > 0).any()),
                sigma_both=bool((sigma[live] == r["w_min"]).any() and (sigma[live] > r["w_min"]).any()))


def beam_arrival_figures(r, xf, cols):
    """the beam arrivals' quantities of the seed rule, from the restated lists alone"""
    a, lin, a_b = r["ba"], r["ba_linear"], r["ba_b"]
    n = len(cols)
    per = np.diff(a["offsets"]).reshape(-1, n)
    at_source = np.asarray(xf)[np.asarray(cols)] == xf[0]
    slot = np.repeat(np.arange(per.size), per.ravel()) % n
    t_end = r["t0"] + (N_TIMES - 1) * r["dt"]
    inside = (a["time"] >= r["t0"][slot] - 8.0 * r["sigma"]) & (a["time"] <= t_end[slot] + 8.0 * r["sigma"])
    same_set = np.array_equal(a["offsets"], lin["offsets"]) and np.array_equal(a["tube"], lin["tube"])
    with np.errstate(invalid="ignore"):
        curved = float((a["time"] != lin["time"]).mean()) if same_set and len(a["time"]) else 0.0
    away = ~at_source
    # (the sums are 0.0 in the source's own column, which holds no arrivals; the field is NaN there)
    field = all(_bits_equal(at_source_nan(r[k][:, :, None], xf, cols)[:, :, 0], r[ref][:, cols]) and (r[k][:, at_source] == 0).all()
                for k, ref in (("ba_field", "BP"), ("ba_field_linear", "BP_linear")))
    return dict(ba_arrivals=int(a["offsets"][-1]), ba_source_dark=bool((per[:, at_source] == 0).all()),
                ba_lit_groups=float((per[:, away] > 0).mean()) if away.any() else 0.0,
                ba_squares=bool(ba.no_subnormal_squares(a["amplitude"]) and ba.no_subnormal_squares(a_b["amplitude"])),
                ba_times=bool(not np.isnan(a["time"]).any() and not np.isnan(a_b["time"]).any()), ba_curved=curved,
                ba_columns_with_a_pulse=int(len(np.unique(slot[inside]))), ba_pulse_lit=bool((np.abs(r["bu_raw"]) > 0).any()),
                ba_sums_to_field=bool(field), ba_infinite=int(np.isinf(a["amplitude"]).sum()),
                ba_surface_image=bool((a["image"] == 1).any()), ba_bottom_image=bool((a["image"] == 2).any()),
                ba_q=tuple(int(v) for v in np.unique(a["q"])))


def _bits_equal(a, b):
    return all((((x == y) | ((x != x) & (y != y))).all()) for x, y in ((a.real, b.real), (a.imag, b.imag)))


BEAM_RULES = (("beam_finite", 0.5), ("beam_nonzero", 0.5), ("beam_left_out", 1), ("beam_curved", 0.5))
BEAM_TALLIES = ("surface_image", "bottom_image", "sigma_both", "ba_surface_image", "ba_bottom_image")
# the beam arrivals' conditions, which every case meets (none is exempt: an infinite amplitude is an arrival like any other)
ARRIVAL_RULES = (("ba_arrivals", 1000), ("ba_source_dark", True), ("ba_lit_groups", 0.5), ("ba_squares", True), ("ba_times", True),
                 ("ba_curved", 0.5), ("ba_columns_with_a_pulse", 1), ("ba_pulse_lit", True), ("ba_sums_to_field", True))
# the lists of restate() and of level 1: (name, weights, q, curvature)
BEAM_LISTS = (("ba", "W", "q", True), ("ba_linear", "W", "q", False), ("ba_bare", None, None, True), ("ba_b", "Wb", "q", True))
BEAM_FLOOR = 30                                           # of the 40 level-1 cases, for each of BEAM_TALLIES


def misses(fig, beams=True):
    """the conditions of the seed rule a case misses (empty: it stays); beams False: a case of BEAM_EXEMPT"""
    rules = (("bounced_tubes", 20), ("left_out", 1), ("kappa_max", 1), ("field_fill", 0.5), ("columns_with_a_pulse", 1),
             ("pulse_lit", True), ("eikonal_share", EIKONAL_SHARE))
    if beams and "beam_finite" in fig:
        rules += BEAM_RULES
    if "ba_arrivals" in fig:
        rules += ARRIVAL_RULES
    return [f"{k} {fig[k]} < {least}" for k, least in rules if not fig[k] >= least]


def not_vacuous(r, xf, cols, label, beams=True):
    fig = figures(r, xf, cols)
    assert not misses(fig, beams), (label, misses(fig, beams), fig)
    return fig


# ---- the oracle's fan: the seed rule without a GPU ----------------------------------------------------------------------------

def oracle_fan(arrs, y0, kw):
    """the fan restate() takes, from the CPU oracle: the surviving rays of oracle.shoot_fan in the stored convention and the
    log of every bouncing ray from the oracle's step trace"""
    shot = dict(rtol=kw["rtol"], terminate_backwards=kw["terminate_backwards"])
    g = oracle.shoot_fan(*arrs, y0, kw["x0"], kw["x1"], kw["S"], math=oracle.MATH_CR, **shot)
    keep = np.flatnonzero(g["status"] == 0)
    total = (g["n_bott"] + g["n_surf"])[keep]
    K = max(1, int(total.max())) if len(keep) else 1
    bx, bp, bk = np.full((len(keep), K), np.nan), np.full((len(keep), K), np.nan), np.full((len(keep), K), -1, np.int8)
    for m in np.flatnonzero(total > 0):
        ox, op, ok = bref.trace_bounces(arrs, y0[keep[m]], kw["x0"], kw["x1"], max_rows=MAX_ROWS, **shot)
        assert len(ox) == total[m], (m, len(ox), total[m])
        bx[m, :len(ox)], bp[m, :len(ox)], bk[m, :len(ox)] = ox, -op, ok
    return dict(ts=g["T"][keep], zs=-g["z"][keep], ps=-g["p"][keep], x=g["r"], p0=y0[keep, 2], log=(bx, bp, bk), kept=keep)


def api_case(seed):
    """an un-mirrored case as the API takes it -> (raw tables, source depth, launch angles, shot kwargs, description)"""
    arrs, (src, x0, th), kw, desc = random_case(seed, n_rays=n_rays_of(seed))
    assert "mirrored False" in desc
    return arrs, src, th, kw, desc


class _Tables:
    """what frame_independent reads of an OceanEnvironment2D, without the package: the user's tables and the latitude"""

    class _DA:
        def __init__(self, values, dims, coords):
            self.values, self.dims, self.coords = values, dims, coords

    def __init__(self, arrs, lat):
        cin, _, rin, zin, bdep, brng, _ = arrs
        self.sound_speed = self._DA(cin, ("range", "depth"), {"range": rin, "depth": zin})
        self.bathymetry = self._DA(bdep, ("range",), {"range": brng})
        self.latitude = lat


def cpu_check(level1=True, level2=True):
    """The seed rule on every case of both levels with the oracle's fan in the device's place: prints each case's figures and
    the cases that miss a condition; needs no GPU."""
    import time

    import pygenray_amd as package
    out = []
    if level1:
        tally = dict(lag=0, surface=0, bottom=0, **{k: 0 for k in BEAM_TALLIES})
        q_seen = set()
        for seed, flat in CASES:
            t = time.time()
            arrs, y0, kw, desc, mirrored = case_inputs(seed, flat)
            cin, cpin, rin, zin, bdep, brng, bang = arrs
            fan = oracle_fan(arrs, y0, kw)
            depths = thinned_receivers(fan["zs"], float(bdep.max()), seed)
            cols = columns(kw["S"])
            r = restate(fan, (cin, rin, zin, bdep, brng), (brng, bang), bottom_of(package, seed), seed, depths, cols,
                        w_min=MIN_WIDTHS[seed % 3])
            fig = figures(r, fan["x"], cols)
            for k in tally:
                tally[k] += fig[k]
            q_seen |= set(fig["ba_q"])
            missed = misses(fig, (seed, flat) not in BEAM_EXEMPT)
            out.append(((seed, flat), missed))
            print(f"seed {seed} flat {flat!s:5s} {time.time() - t:5.1f} s  misses {missed}  {fig}", flush=True)
        print("level 1:", tally, "emitted q", sorted(q_seen))
        out.append(("level 1", [f"{k} {tally[k]} < {BEAM_FLOOR}" for k in BEAM_TALLIES if tally[k] < BEAM_FLOOR]
                    + [f"emitted q {sorted(q_seen)}"] * (q_seen != {0, 1, 2, 3})))
    if level2:
        for seed, lat in API_CASES:
            arrs, src, th, kw, desc = api_case(seed)
            tables = _Tables(arrs, lat)
            for backwards in (False, True):
                xs, xr = (kw["x1"], kw["x0"]) if backwards else (kw["x0"], kw["x1"])
                x = -np.linspace(-xs, -xr, kw["S"]) if backwards else np.linspace(xs, xr, kw["S"])   # (as shoot_rays saves)
                for fe in (False, True):
                    t = time.time()
                    xf, cin, rin, zin, bd, br = fi.traced_frame(tables, x, fe)
                    beta = fi.bottom_slope(tables, x)
                    frame_arrs = [cin, np.gradient(cin, zin, axis=1, edge_order=1), rin, zin, bd, br, beta[1]]
                    y0 = y0_for(oracle, frame_arrs, src, xf[0], -th)              # (128 angles and more: the ODE angle is -theta)
                    fan = oracle_fan(frame_arrs, y0, dict(kw, x0=xf[0], x1=xf[-1]))
                    fan["p0"] = fi.launch_slowness(th[fan["kept"]], src, xf, cin, rin, zin)
                    depths = thinned_receivers(fan["zs"], float(bd.max()), seed)
                    cols = columns(kw["S"])
                    r = restate(fan, (cin, rin, zin, bd, br), beta, bottom_of(package, seed), seed, depths, cols,
                                w_min=MIN_WIDTHS[seed % 3])
                    fig = figures(r, xf, cols)
                    missed = misses(fig, seed not in BEAM_EXEMPT_API)
                    out.append(((seed, backwards, fe), missed))
                    print(f"API seed {seed} backwards {backwards!s:5s} flatearth {fe!s:5s} {time.time() - t:5.1f} s  "
                          f"misses {missed}  {fig}", flush=True)
    print("missed:", [(c, m) for c, m in out if m])
    return out


# ---- level 1: kernels and fan entries on raw tables ---------------------------------------------------------------------------

def _close(a, b, what, label):
    """bit for bit, NaN patterns included"""
    a, b = np.asarray(a), np.asarray(b)
    assert a.shape == b.shape, (label, what, a.shape, b.shape)
    for x, y in ((a.real, b.real), (a.imag, b.imag)) if np.iscomplexobj(a) or np.iscomplexobj(b) else ((a, b),):
        bad = ~((x == y) | ((x != x) & (y != y)))
        assert not bad.any(), (label, what, int(bad.sum()), np.argwhere(bad)[:5].tolist(), x[bad][:5], y[bad][:5])


def same_beam_arrivals(a, b, what, label):
    """two beam-arrival lists (host dicts): the offsets and the integers equal and of one type, time and amplitude bit for bit"""
    assert a["offsets"].dtype == b["offsets"].dtype and np.array_equal(a["offsets"], b["offsets"]), (label, what, "arrival counts")
    for k in BEAM_KEYS:
        assert a[k].dtype == b[k].dtype, (label, what, k, a[k].dtype, b[k].dtype)
        _close(a[k], b[k], f"{what}: arrivals' {k}", label)


class _Device:
    """the tensors and calls shared by the buffer entries and the handle's own entries of one case"""

    def __init__(self, env, depths, p0, f):
        import torch
        self.torch, self.env, self.f = torch, env, f
        self.dev = torch.device("cuda", env.device)
        (self.depths, self.p0), self.stream = _upload(env, depths, p0)
        self.R = len(depths)

    def f64(self, *shape):
        return self.torch.full(shape, MARK, dtype=self.torch.float64, device=self.dev)

    def i32(self, *shape):
        return self.torch.full(shape, -7, dtype=self.torch.int32, device=self.dev)

    def up(self, a, dtype=np.float64):
        return self.torch.from_numpy(np.ascontiguousarray(a, dtype=dtype)).to(self.dev)

    def arrivals(self, cols, count, emit):
        """the count, the scan and the emit of one arrivals walk -> device tensors (offsets, tube, w, T, p, I)"""
        torch = self.torch
        n = len(cols)
        counts = torch.full((self.R * n,), -1, dtype=torch.int64, device=self.dev)
        count(counts.data_ptr())
        offsets = torch.zeros(self.R * n + 1, dtype=torch.int64, device=self.dev)
        torch.cumsum(counts, 0, out=offsets[1:])
        total = int(offsets[-1].item())
        assert total > 0
        tube = torch.full((total,), -1, dtype=torch.int32, device=self.dev)
        w, T, p, I = (self.f64(total) for _ in range(4))
        emit(offsets.data_ptr(), total, tube.data_ptr(), w.data_ptr(), T.data_ptr(), p.data_ptr(), I.data_ptr())
        return dict(offsets=offsets, tube=tube, w=w, T=T, p=p, I=I)

    def beam_pressure(self, call, q, W, bottom, w_min, curvature, S):
        """one beam sum through `call` (a buffer or a fan entry from p0 on) into outputs with sentinels before and behind
        -> complex (R, S)"""
        n = self.R * S
        out = [self.f64(PAD + n + PAD) for _ in range(2)]
        call(self.p0.data_ptr(), 0 if q is None else q.data_ptr(), self.f, bottom.data_ptr(), self.depths.data_ptr(), self.R,
             w_min, curvature, out[0][PAD:].data_ptr(), out[1][PAD:].data_ptr(), self.stream,
             weights=0 if W is None else W.data_ptr())
        host = [a.cpu().numpy() for a in out]
        assert all((a[:PAD] == MARK).all() and (a[PAD + n:] == MARK).all() for a in host), "written outside the output"
        return _complex(*(a[PAD:PAD + n].reshape(self.R, S) for a in host))

    def beam_list(self, cols, count, emit):
        """the count, the scan and the emit of one beam-arrival walk, the counts and the five arrays written between sentinels
        that are checked untouched before and behind -> device tensors (offsets, tube, image, time, amplitude, q)"""
        torch = self.torch
        G = self.R * len(cols)
        counts = torch.full((PAD + G + PAD,), -7, dtype=torch.int64, device=self.dev)
        count(counts[PAD:].data_ptr())
        host = counts.cpu().numpy()
        assert (host[:PAD] == -7).all() and (host[PAD + G:] == -7).all(), "written outside the counts"
        assert (host[PAD:PAD + G] >= 0).all()
        offsets = torch.zeros(G + 1, dtype=torch.int64, device=self.dev)
        torch.cumsum(counts[PAD:PAD + G], 0, out=offsets[1:])
        total = int(offsets[-1].item())
        assert total > 0
        out = {k: (self.f64 if k in ("time", "amplitude") else self.i32)(PAD + total + PAD) for k in BEAM_KEYS}
        emit(offsets.data_ptr(), total, *(out[k][PAD:].data_ptr() for k in BEAM_KEYS))
        for k, v in out.items():
            host, mark = v.cpu().numpy(), MARK if k in ("time", "amplitude") else -7
            assert (host[:PAD] == mark).all() and (host[PAD + total:] == mark).all(), f"written outside the arrivals' {k}"
        return dict(offsets=offsets, **{k: v[PAD:PAD + total] for k, v in out.items()})

    def beam_sums(self, lists, cols, L, t0, rs, dt, freq, alpha):
        """the sums of pgr_spectrum.h and pgr_signal.h over the beam lists of one side, I = amp * amp formed as beam_arrivals.py
        forms it: the weighted lists at the one frequency f without a reduction time or path lengths, the pulse of the
        curvature-1 list, and the band of the list without volume absorption with the mean path length of each arrival's tube,
        L [S][M] at (column, tube) and (column, tube + 1) as L0 + 0.5 (L1 - L0) in three operations -> complex host arrays"""
        from pygenray_amd import _lib
        torch = self.torch
        n = len(cols)
        G = self.R * n
        zero, tstart = self.up(np.zeros(G)), self.up(np.tile(t0, self.R))
        o = {}
        for name, key in (("ba_field", "ba"), ("ba_field_linear", "ba_linear")):
            a = lists[key]
            I = a["amplitude"] * a["amplitude"]
            re, im = self.f64(G, 1), self.f64(G, 1)
            _lib.spectrum_device(self.env.device, a["offsets"].data_ptr(), G, a["time"].data_ptr(), I.data_ptr(), a["q"].data_ptr(),
                                 0, zero.data_ptr(), [self.f], None, re.data_ptr(), im.data_ptr(), self.stream)
            o[name] = _complex(re.cpu().numpy(), im.cpu().numpy()).reshape(self.R, n)
        a = lists["ba"]
        I = a["amplitude"] * a["amplitude"]
        re, im = self.f64(G, N_TIMES), self.f64(G, N_TIMES)
        _lib.signal_device(self.env.device, a["offsets"].data_ptr(), G, a["time"].data_ptr(), I.data_ptr(), a["q"].data_ptr(),
                           tstart.data_ptr(), self.f, rs, dt, N_TIMES, re.data_ptr(), im.data_ptr(), self.stream)
        o["bu_raw"] = _complex(re.cpu().numpy(), im.cpu().numpy()).reshape(self.R, n, N_TIMES)
        a = lists["ba_b"]
        I = a["amplitude"] * a["amplitude"]
        group = torch.repeat_interleave(torch.arange(G, device=self.dev), a["offsets"][1:] - a["offsets"][:-1])
        col = torch.from_numpy(np.asarray(cols, dtype=np.int64)).to(self.dev)[group % n]
        k = a["tube"].long()
        L0, L1 = L[col, k], L[col, k + 1]
        step = L1 - L0
        step = 0.5 * step
        La = (L0 + step).contiguous()
        o["bLa"] = La.cpu().numpy()
        re, im = self.f64(G, N_FREQ), self.f64(G, N_FREQ)
        _lib.spectrum_device(self.env.device, a["offsets"].data_ptr(), G, a["time"].data_ptr(), I.data_ptr(), a["q"].data_ptr(),
                             La.data_ptr(), tstart.data_ptr(), freq, alpha, re.data_ptr(), im.data_ptr(), self.stream)
        o["bH"] = _complex(re.cpu().numpy(), im.cpu().numpy()).reshape(self.R, n, N_FREQ)
        return o

    def phase_index(self, kappa, nb, ns):
        """q [S][M] as coherent.py forms it on the device"""
        torch = self.torch
        q = kappa.clone()
        same = (nb[:, :-1] == nb[:, 1:]) & (ns[:, :-1] == ns[:, 1:])
        q[:, :-1] = torch.where(same, q[:, :-1] + 2 * ns[:, :-1], torch.full_like(q[:, :-1], -1))
        return q

    def per_arrival(self, a, cols, q, Phi, L):
        """every arrival's q, lag and path length as signal.py and spectrum.py form them on the device"""
        torch = self.torch
        n = len(cols)
        group = torch.repeat_interleave(torch.arange(self.R * n, device=self.dev), a["offsets"][1:] - a["offsets"][:-1])
        col = torch.from_numpy(np.asarray(cols, dtype=np.int64)).to(self.dev)[group % n]
        k = a["tube"].long()
        out = [q[col, k].contiguous()]
        for V in (Phi, L):
            V0, V1 = V[col, k], V[col, k + 1]
            d = V1 - V0
            d = a["w"] * d
            out.append((V0 + d).contiguous())
        return out

    def sums(self, a, a_b, qa, phi, La, t0, rs, dt, freq, alpha):
        """the pulse sum of the arrivals `a` and the band sum of `a_b` (phi None: the siblings without a lag)"""
        from pygenray_amd import _lib
        G = len(a["offsets"]) - 1
        n = len(t0)
        tstart = self.up(np.tile(t0, G // n))
        u = [self.f64(G, N_TIMES) for _ in range(2)]
        H = [self.f64(G, N_FREQ) for _ in range(2)]
        head = (self.env.device, a["offsets"].data_ptr(), G)
        lag = () if phi is None else (phi.data_ptr(),)
        sig, spec = (_lib.signal_device, _lib.spectrum_device) if phi is None else (_lib.signal_phi_device, _lib.spectrum_phi_device)
        sig(*head, a["T"].data_ptr(), a["I"].data_ptr(), qa.data_ptr(), *lag, tstart.data_ptr(), self.f, rs, dt, N_TIMES,
            u[0].data_ptr(), u[1].data_ptr(), self.stream)
        spec(self.env.device, a_b["offsets"].data_ptr(), G, a_b["T"].data_ptr(), a_b["I"].data_ptr(), qa.data_ptr(), *lag,
             La.data_ptr(), tstart.data_ptr(), freq, alpha, H[0].data_ptr(), H[1].data_ptr(), self.stream)
        return _complex(u[0].cpu().numpy(), u[1].cpu().numpy()), _complex(H[0].cpu().numpy(), H[1].cpu().numpy())


def _host(a):
    return {k: v.cpu().numpy() for k, v in a.items()}


_RECORDS = {}


def _level1(pr, seed, flat):  # noqa: F811
    """one case of level 1 -> its record for the sweep's tallies (cached: the tally test asks again)"""
    if (seed, flat) in _RECORDS:
        return _RECORDS[(seed, flat)]
    import torch
    from pygenray_amd import _lib
    arrs, y0, kw, desc, mirrored = case_inputs(seed, flat)
    cin, cpin, rin, zin, bdep, brng, bang = arrs
    label = f"seed {seed}{' (flat earth)' if flat else ''}: {desc}"
    env = _lib.EnvHandle(*arrs)
    shot = dict(rtol=kw["rtol"], terminate_backwards=kw["terminate_backwards"])
    x0, x1, S = kw["x0"], kw["x1"], kw["S"]
    # 1. the logged handle against the un-logged host-pointer shot
    g = env.shoot_fan(y0, x0, x1, S, sample_major=True, stored_sign=True, **shot)
    keep = g["status"] == 0
    M = int(keep.sum())
    assert M >= 64, label
    total = (g["n_bott"] + g["n_surf"])[keep].astype(np.int64)
    K = max(1, int(total.max()))
    T, z, p = (np.ascontiguousarray(g[k][:, keep]) for k in "Tzp")       # (S, M)
    h = _lib.FanHandle(env, x0, x1, S, y0=y0, stored_sign=True, max_bounces=K, **shot)
    assert h.wait() == (len(y0), M), label
    rays = h.fetch_rays()
    assert np.array_equal(rays["status"], g["status"]), label
    for k in ("n_bott", "n_surf", "n_steps", "n_rej", "end"):
        assert _same(rays[k][keep], g[k][keep]), (label, k)
    smp = h.fetch_samples()
    for k in "Tzp":
        _close(smp[k], g[k][:, keep], f"logged fan's {k}", label)
    # 2. the log against the oracle's step trace, on every 8th surviving bouncing ray
    bx, bp, bk = h.fetch_bounces()                                       # (K, M), stored sign
    assert bk.shape == (K, M) and np.array_equal((bk >= 0).sum(axis=0), total), label
    idx = np.flatnonzero(keep)
    traced = np.flatnonzero(total > 0)[::8]
    assert len(traced) >= 3, label
    for m in traced:
        ox, op, ok = bref.trace_bounces(arrs, y0[idx[m]], x0, x1, max_rows=MAX_ROWS, **shot)
        E = int(total[m])
        assert len(ox) == E, (label, m, len(ox), E)
        assert _same(bx[:E, m], ox) and _same(-bp[:E, m], op) and np.array_equal(bk[:E, m], ok), (label, "log of ray", m)
        assert np.isnan(bx[E:, m]).all() and np.isnan(bp[E:, m]).all() and (bk[E:, m] == -1).all(), (label, m)
    # the restatements on the same raw tables
    xs, p0 = g["r"], y0[keep, 2]
    depths = thinned_receivers(z.T, float(bdep.max()), seed)
    cols = columns(S)
    R, n = len(depths), len(cols)
    bottom = bottom_of(pr, seed)
    fan = dict(ts=T.T, zs=z.T, ps=p.T, x=xs, p0=p0, log=(bx.T, bp.T, bk.T))
    w_min = MIN_WIDTHS[seed % 3]
    r = restate(fan, (cin, rin, zin, bdep, brng), (brng, bang), bottom, seed, depths, cols, w_min=w_min)
    fig = not_vacuous(r, xs, cols, label, beams=(seed, flat) not in BEAM_EXEMPT)      # (the eikonal share: the device's own fan)
    f = r["f"]
    alpha_f = pr.thorp_absorption(r["freq"]) / 1000.0
    H_ref = band_sum(r, alpha_f, R, n)
    a_depths, alpha = pref.profile_db_per_m(r["absorption"])
    t_db, t_lag = _lib.boundary_tables(*r["tables_db"]), _lib.boundary_tables(*r["tables_lag"])
    # 3. the buffer entries
    d = _Device(env, depths, p0, f)
    dT, dz, dp, dx = _upload(env, T, z, p, xs)[0]
    dbx, dbp, dbk = d.up(bx), d.up(bp), d.up(bk, np.int8)
    floor = d.up(fi.bottom_at(xs, bdep, brng))
    fanp = (dT.data_ptr(), dz.data_ptr(), dp.data_ptr())
    dims = (M, S, dx.data_ptr())

    def buffers():
        o = {}
        for name, (ad, al) in (("A", (a_depths, alpha)), ("L", (None, np.ones(1)))):
            o[name] = d.f64(S, M)
            _lib.path_integral_device(env, fanp[0], fanp[1], *dims, ad, al, o[name].data_ptr(), d.stream)
        for name, tables in (("B", t_db), ("Phi", t_lag)):
            o[name], o[name + "_nb"], o[name + "_ns"] = d.f64(S, M), d.i32(S, M), d.i32(S, M)
            _lib.boundary_loss_device(env, dbx.data_ptr(), dbp.data_ptr(), dbk.data_ptr(), M, K, x0, x1, S, tables,
                                      o[name].data_ptr(), o[name + "_nb"].data_ptr(), o[name + "_ns"].data_ptr(), d.stream)
        o["kappa"] = d.i32(S, M)
        _lib.caustic_index_device(env.device, fanp[1], M, S, o["B_nb"].data_ptr(), o["B_ns"].data_ptr(), o["kappa"].data_ptr(),
                                  d.stream)
        return o

    def handle():
        o = {}
        for name, (ad, al) in (("A", (a_depths, alpha)), ("L", (None, np.ones(1)))):
            o[name] = d.f64(S, M)
            h.path_integral(ad, al, o[name].data_ptr(), d.stream)
        for name, tables in (("B", t_db), ("Phi", t_lag)):
            o[name], o[name + "_nb"], o[name + "_ns"] = d.f64(S, M), d.i32(S, M), d.i32(S, M)
            h.boundary_loss(tables, o[name].data_ptr(), o[name + "_nb"].data_ptr(), o[name + "_ns"].data_ptr(), d.stream)
        o["kappa"] = d.i32(S, M)
        h.caustic_index(o["B_nb"].data_ptr(), o["B_ns"].data_ptr(), o["kappa"].data_ptr(), d.stream)
        return o

    def weights_and_sums(o, pressure, pressure_phi, counts, emit, beam, beam_counts, beam_emit):
        """what follows the per-ray arrays, through the tube entries given"""
        for name, src in (("W", o["A"] + o["B"]), ("Wb", o["B"])):
            o[name] = d.f64(S, M)
            _lib.absorption_weights_device(env.device, src.data_ptr(), src.numel(), o[name].data_ptr(), d.stream)
        o["q"] = d.phase_index(o["kappa"], o["B_nb"], o["B_ns"])
        tail = (f, d.depths.data_ptr(), R)
        no_lag = torch.zeros_like(o["Phi"])
        for name, call, lag in (("P", pressure_phi, (o["Phi"].data_ptr(),)), ("P_sibling", pressure, ()),
                                ("P_zero_lag", pressure_phi, (no_lag.data_ptr(),))):
            re, im = d.f64(R, S), d.f64(R, S)
            call(d.p0.data_ptr(), o["q"].data_ptr(), *lag, *tail, re.data_ptr(), im.data_ptr(), d.stream, weights=o["W"].data_ptr())
            o[name] = _complex(re.cpu().numpy(), im.cpu().numpy())
        for name, q, W, curvature in (("BP", o["q"], o["W"], 1), ("BP_linear", o["q"], o["W"], 0), ("BP_bare", None, None, 1)):
            o[name] = d.beam_pressure(beam, q, W, floor, w_min, curvature, S)
        for name, W in (("arr", o["W"]), ("arr_b", o["Wb"])):
            o[name] = d.arrivals(cols, lambda c: counts(d.p0.data_ptr(), d.depths.data_ptr(), R, cols, c, d.stream),
                                 lambda *a: emit(d.p0.data_ptr(), d.depths.data_ptr(), R, cols, *a, d.stream, weights=W.data_ptr()))
        # the beam arrivals: the four lists, then the sums over them
        for name, w_, q_, curvature in BEAM_LISTS:
            W_, q_ = 0 if w_ is None else o[w_].data_ptr(), 0 if q_ is None else o["q"].data_ptr()
            head = (d.p0.data_ptr(), q_, floor.data_ptr(), d.depths.data_ptr(), R, w_min, cols)
            o[name] = d.beam_list(cols, lambda c: beam_counts(*head, c, d.stream, weights=W_),
                                  lambda *a: beam_emit(*head, int(curvature), *a, d.stream, weights=W_))
        o.update(d.beam_sums(o, cols, o["L"], r["t0"], r["rs"], r["dt"], r["freq"], alpha_f))
        return o

    b = weights_and_sums(
        buffers(),
        lambda *a, **k: _lib.pressure_device(env, *fanp, *dims, *a, **k),
        lambda *a, **k: _lib.pressure_phi_device(env, *fanp, *dims, *a, **k),
        lambda *a: _lib.arrival_counts_device(env, fanp[1], fanp[2], *dims, *a),
        lambda *a, **k: _lib.arrivals_device(env, *fanp, *dims, *a, **k),
        lambda *a, **k: _lib.beam_pressure_device(env, *fanp, *dims, *a, **k),
        lambda *a, **k: _lib.beam_arrival_counts_device(env, *fanp, *dims, *a, **k),
        lambda *a, **k: _lib.beam_arrivals_device(env, *fanp, *dims, *a, **k))
    for name in ("A", "L", "B", "Phi", "W", "Wb"):
        _close(b[name].cpu().numpy().T, r[name], name, label)
    for name in ("B", "Phi"):                                            # (the counts do not depend on the tables)
        assert np.array_equal(b[name + "_nb"].cpu().numpy().T, r["nb"]) and np.array_equal(b[name + "_ns"].cpu().numpy().T, r["ns"]), \
            (label, "bounce counts per sample", name)
    assert np.array_equal(b["kappa"].cpu().numpy().T[:-1], r["kappa"]), (label, "caustic index")
    assert np.array_equal(b["q"].cpu().numpy().T[:-1], r["q"][:-1]), (label, "phase index")
    _close(b["P"], r["P"], "pressure_phi_device", label)
    ref = cref.tube_pressure(z.T, p.T, T.T, xs, p0, depths, cin, rin, zin, r["W"], r["q"], f)
    _close(b["P_sibling"], _complex(*ref), "pressure_device", label)
    _close(b["P_zero_lag"], b["P_sibling"], "pressure_phi_device at a lag of zero", label)          # 4.
    _close(b["BP"], r["BP"], "beam_pressure_device", label)
    _close(b["BP_linear"], r["BP_linear"], "beam_pressure_device without the curvature term", label)
    _close(b["BP_bare"][:, cols], r["BP_bare"], "beam_pressure_device without weights and with q NULL", label)
    same_arrivals(_host(b["arr"]), r["arr"], label + " (weighted arrivals)")
    same_arrivals(_host(b["arr_b"]), r["arr_b"], label + " (arrivals without volume absorption)")
    qa, phi, La = d.per_arrival(b["arr"], cols, b["q"], b["Phi"], b["L"])
    assert np.array_equal(qa.cpu().numpy(), r["qa"]), (label, "arrivals' q")
    _close(phi.cpu().numpy(), r["phi"], "arrivals' lag", label)
    _close(La.cpu().numpy(), r["La"], "arrivals' path length", label)
    u, H = d.sums(b["arr"], b["arr_b"], qa, phi, La, r["t0"], r["rs"], r["dt"], r["freq"], alpha_f)
    _close(u.reshape(R, n, N_TIMES), r["u_raw"], "signal_phi_device", label)
    _close(H.reshape(R, n, N_FREQ), H_ref, "spectrum_phi_device", label)
    u0, H0 = d.sums(b["arr"], b["arr_b"], qa, torch.zeros_like(phi), La, r["t0"], r["rs"], r["dt"], r["freq"], alpha_f)    # 4.
    us, Hs = d.sums(b["arr"], b["arr_b"], qa, None, La, r["t0"], r["rs"], r["dt"], r["freq"], alpha_f)
    _close(u0, us, "signal_phi_device at a lag of zero", label)
    _close(H0, Hs, "spectrum_phi_device at a lag of zero", label)
    # the beam arrivals: every list against the restatement from the definition; the weighted lists summed at f are the beam
    # kernel's own field and the tube-by-tube restatement's on the requested columns (NaN in the source's own, where the list
    # holds nothing and its sum is 0.0); the pulse and the band against the restated sums over the restated lists
    for name, *_ in BEAM_LISTS:
        same_beam_arrivals(_host(b[name]), r[name], f"beam_arrivals_device ({name})", label)
    for name, of in (("ba_field", "BP"), ("ba_field_linear", "BP_linear")):
        assert (b[name][:, xs[cols] == xs[0]] == 0).all(), (label, name, "at the source's column")
        summed = at_source_nan(b[name][:, :, None], xs, cols)[:, :, 0]
        _close(summed, b[of][:, cols], f"the beam list summed at f against beam_pressure_device's {of}", label)
        _close(summed, r[of][:, cols], f"the beam list summed at f against the restated {of}", label)
    _close(b["bu_raw"], r["bu_raw"], "signal_device over the beam list", label)
    _close(b["bLa"], r["bLa"], "beam arrivals' mean path length", label)
    _close(b["bH"], beam_band_sum(r, alpha_f, R, n), "spectrum_device over the beam list without volume absorption", label)
    # 5. the handle's own entries against the buffer entries
    e = weights_and_sums(handle(), h.pressure, h.pressure_phi, h.arrival_counts, h.arrivals, h.beam_pressure,
                         h.beam_arrival_counts, h.beam_arrivals)
    for name in ("A", "L", "B", "Phi", "B_nb", "B_ns", "Phi_nb", "Phi_ns", "W", "Wb"):
        _close(e[name].cpu().numpy(), b[name].cpu().numpy(), f"the handle's {name}", label)
    assert np.array_equal(e["kappa"].cpu().numpy()[:, :-1], b["kappa"].cpu().numpy()[:, :-1]), (label, "the handle's caustic index")
    for name in ("P", "P_sibling", "P_zero_lag", "BP", "BP_linear", "BP_bare"):
        _close(e[name], b[name], f"the handle's {name}", label)
    for name in ("arr", "arr_b"):
        same_arrivals(_host(e[name]), _host(b[name]), f"{label} (the handle's {name})")
    for name, *_ in BEAM_LISTS:
        same_beam_arrivals(_host(e[name]), _host(b[name]), f"the handle's beam arrivals ({name})", label)
    for name in ("ba_field", "ba_field_linear", "bu_raw", "bLa", "bH"):
        _close(e[name], b[name], f"the handle's {name}", label)
    h.close()
    nonuniform = float(np.ptp(np.diff(rin))) > 1e-6 * float(np.mean(np.diff(rin)))
    offset = abs(rin[-1] if mirrored else rin[0])
    rec = dict(hbm=not env.lds_path, lds=env.lds_path, blocked=env.blocked_layout, mirrored=mirrored, offset=offset > 100e3,
               nonuniform=nonuniform, flat=flat, dropped=M < len(y0), lag=fig["lag"], surface=fig["surface"],
               bottom=fig["bottom"], rays=M, traced=len(traced), arrivals=fig["arrivals"], K=K, kappa=fig["kappa_max_anywhere"],
               bounced_tubes=fig["bounced_tubes"], field_fill=fig["field_fill"], eikonal=fig["eikonal_share"],
               beam_nonzero=fig["beam_nonzero"], beam_finite=fig["beam_finite"], beam_left_out=fig["beam_left_out"],
               ba_arrivals=fig["ba_arrivals"], ba_lit_groups=fig["ba_lit_groups"], ba_infinite=fig["ba_infinite"], ba_q=fig["ba_q"],
               **{k: fig[k] for k in BEAM_TALLIES})
    env.close()
    _RECORDS[(seed, flat)] = rec
    return rec


@pytest.mark.parametrize("seed, flat", LEVEL1, ids=[f"seed{s}{'-flat' if fl else ''}" for s, fl in LEVEL1])
def test_kernels_and_fan_entries_on_random_raw_tables(pr, seed, flat):  # noqa: F811
    _level1(pr, seed, flat)


def test_the_sweep_holds_what_it_is_meant_to(pr):  # noqa: F811
    """the tallies over the level-1 cases (each case's record is kept by its own test; a case not run yet is run here)"""
    recs = [_level1(pr, seed, flat) for seed, flat in LEVEL1]
    tally = {k: int(sum(rec[k] for rec in recs)) for k in ("hbm", "lds", "blocked", "mirrored", "offset", "nonuniform", "flat",
                                                           "dropped", "lag", "surface", "bottom", "rays", "traced", "arrivals")
             + BEAM_TALLIES}
    held = [rec for rec, case in zip(recs, LEVEL1) if case not in BEAM_EXEMPT]
    print(f"\n{len(recs)} random environments: {tally}; log capacity {min(r['K'] for r in recs)} ... {max(r['K'] for r in recs)}; "
          f"largest caustic index {min(r['kappa'] for r in recs)} ... {max(r['kappa'] for r in recs)}; bounced tubes with q >= 0 "
          f"at the last column {min(r['bounced_tubes'] for r in recs)} ... {max(r['bounced_tubes'] for r in recs)}; field fill "
          f"{min(r['field_fill'] for r in recs):.3f} ... {max(r['field_fill'] for r in recs):.3f}; eikonal share "
          f"{min(r['eikonal'] for r in recs):.3f} ... {max(r['eikonal'] for r in recs):.3f}; beam fields' non-zero share "
          f"{min(r['beam_nonzero'] for r in held):.3f} ... {max(r['beam_nonzero'] for r in held):.3f} and finite share "
          f"{min(r['beam_finite'] for r in held):.3f} ... {max(r['beam_finite'] for r in held):.3f} outside BEAM_EXEMPT; valid tubes "
          f"with q < 0 "
          f"{min(r['beam_left_out'] for r in recs)} ... {max(r['beam_left_out'] for r in recs)}")
    q_seen = sorted(set().union(*(rec["ba_q"] for rec in recs)))
    print(f"beam arrivals {min(r['ba_arrivals'] for r in recs)} ... {max(r['ba_arrivals'] for r in recs)} per case, "
          f"{sum(r['ba_arrivals'] for r in recs)} in all, {sum(r['ba_infinite'] for r in recs)} of infinite amplitude in "
          f"{sum(r['ba_infinite'] > 0 for r in recs)} cases; lit groups away from the source "
          f"{min(r['ba_lit_groups'] for r in recs):.3f} ... {max(r['ba_lit_groups'] for r in recs):.3f}; emitted q {q_seen}")
    assert q_seen == [0, 1, 2, 3], q_seen
    for k, least in (("hbm", 6), ("lds", 6), ("blocked", 6), ("mirrored", 6), ("offset", 6), ("nonuniform", 6), ("flat", 6),
                     ("dropped", 4), ("lag", 30), ("surface", 30)) + tuple((k, BEAM_FLOOR) for k in BEAM_TALLIES):
        assert tally[k] >= least, (k, tally)


# ---- every fan entry on a fan in the ODE sign ---------------------------------------------------------------------------------
# include/pgr.h: every pgr_fan_* product entry reads the fan "as launched".  A fan launched without PGR_STORED_SIGN holds z and p
# with the other sign bit; every product of it must be the stored-sign fan's, bit for bit, given the same device arguments.

_SIGN_RECORDS = {}
TTK_GRID = (5, 6)                                         # ranges x depths of the travel-time kernel's own grid


def _either_sign(pr, seed, flat):  # noqa: F811
    if (seed, flat) in _SIGN_RECORDS:
        return _SIGN_RECORDS[(seed, flat)]
    import torch
    from pygenray_amd import _lib
    arrs, y0, kw, desc, mirrored = case_inputs(seed, flat)
    cin, cpin, rin, zin, bdep, brng, bang = arrs
    label = f"seed {seed}{' (flat earth)' if flat else ''}: {desc}"
    env = _lib.EnvHandle(*arrs)
    shot = dict(rtol=kw["rtol"], terminate_backwards=kw["terminate_backwards"])
    x0, x1, S = kw["x0"], kw["x1"], kw["S"]
    scout = _lib.FanHandle(env, x0, x1, S, y0=y0, stored_sign=True, **shot)          # (un-logged: for the log's capacity)
    found = scout.fetch_rays()
    scout.close()
    keep = found["status"] == 0
    M = int(keep.sum())
    K = max(1, int((found["n_bott"] + found["n_surf"])[keep].max()))
    hs = _lib.FanHandle(env, x0, x1, S, y0=y0, stored_sign=True, max_bounces=K, **shot)
    ho = _lib.FanHandle(env, x0, x1, S, y0=y0, stored_sign=False, max_bounces=K, **shot)
    assert hs.wait() == ho.wait() == (len(y0), M) and M >= 64, label
    # the fetches
    rs, ro = hs.fetch_rays(), ho.fetch_rays()
    for k in rs:
        _close(ro[k], rs[k], f"fetch_rays {k}", label)
    ss, so = hs.fetch_samples(), ho.fetch_samples()
    _close(so["T"], ss["T"], "fetch_samples T", label)
    for k in "zp":
        assert sign_flipped(so[k], ss[k]), (label, "fetch_samples", k)
    (bxs, bps, bks), (bxo, bpo, bko) = hs.fetch_bounces(), ho.fetch_bounces()
    _close(bxo, bxs, "fetch_bounces x", label)
    assert np.array_equal(bko, bks) and (bks >= 0).any(), (label, "fetch_bounces kind")
    written = bks >= 0                               # (a slot never written holds the same NaN in either sign)
    assert sign_flipped(bpo[written], bps[written]) and np.isnan(bpo[~written]).all() and np.isnan(bps[~written]).all(), \
        (label, "fetch_bounces p")
    # the device arguments both handles are given
    xs = np.linspace(x0, x1, S)
    z = ss["z"]
    depths = thinned_receivers(z.T, float(bdep.max()), seed)
    cols, w_min, f = columns(S), MIN_WIDTHS[seed % 3], FREQUENCIES[seed % 3]
    R, n = len(depths), len(cols)
    bottom = bottom_of(pr, seed)
    a_depths, alpha = pref.profile_db_per_m(absorption_of(float(bdep.max())))
    beta = (brng, bang)
    t_db = _lib.boundary_tables(tuple(bottom.loss), (None, np.array([SURFACE_DB])), beta)
    t_lag = _lib.boundary_tables(tuple(bottom.lag), (None, np.zeros(1)), beta)
    d = _Device(env, depths, y0[keep, 2], f)
    floor = d.up(fi.bottom_at(xs, bdep, brng))
    assert x1 > x0
    grid_r, grid_d = d.up(np.linspace(x0, x1, TTK_GRID[0])), d.up(np.linspace(0.0, float(bdep.max()), TTK_GRID[1]))

    def per_ray(h, counts=None):
        """the per-ray arrays [S][M]; the caustic index from `counts` (nb, ns) when given, else from the handle's own"""
        o = {}
        for name, (ad, al) in (("A", (a_depths, alpha)), ("L", (None, np.ones(1)))):
            o[name] = d.f64(S, M)
            h.path_integral(ad, al, o[name].data_ptr(), d.stream)
        for name, tables in (("B", t_db), ("Phi", t_lag)):
            o[name], o[name + "_nb"], o[name + "_ns"] = d.f64(S, M), d.i32(S, M), d.i32(S, M)
            h.boundary_loss(tables, o[name].data_ptr(), o[name + "_nb"].data_ptr(), o[name + "_ns"].data_ptr(), d.stream)
        nb, ns = counts or (o["B_nb"], o["B_ns"])
        o["kappa"] = d.i32(S, M)
        h.caustic_index(nb.data_ptr(), ns.data_ptr(), o["kappa"].data_ptr(), d.stream)
        return o

    def products(h, W, q, Phi):
        """every tube product of the handle with the weights, the phase index and the lag given"""
        o, tail = {}, (d.depths.data_ptr(), R)
        o["I"], o["beams"] = d.f64(R, S), d.f64(R, S)
        h.intensity(d.p0.data_ptr(), *tail, o["I"].data_ptr(), d.stream, weights=W.data_ptr())
        h.beam_intensity(d.p0.data_ptr(), floor.data_ptr(), *tail, w_min, o["beams"].data_ptr(), d.stream, weights=W.data_ptr())
        o["arr"] = d.arrivals(cols, lambda c: h.arrival_counts(d.p0.data_ptr(), *tail, cols, c, d.stream),
                              lambda *a: h.arrivals(d.p0.data_ptr(), *tail, cols, *a, d.stream, weights=W.data_ptr()))
        for name, call, lag in (("P", h.pressure, ()), ("P_phi", h.pressure_phi, (Phi.data_ptr(),))):
            re, im = d.f64(R, S), d.f64(R, S)
            call(d.p0.data_ptr(), q.data_ptr(), *lag, f, *tail, re.data_ptr(), im.data_ptr(), d.stream, weights=W.data_ptr())
            o[name] = _complex(re.cpu().numpy(), im.cpu().numpy())
        for name, curvature in (("BP", 1), ("BP_linear", 0)):
            o[name] = d.beam_pressure(h.beam_pressure, q, W, floor, w_min, curvature, S)
        head = (d.p0.data_ptr(), q.data_ptr(), floor.data_ptr(), *tail, w_min, cols)
        o["ba"] = d.beam_list(cols, lambda c: h.beam_arrival_counts(*head, c, d.stream, weights=W.data_ptr()),
                              lambda *a: h.beam_arrivals(*head, 1, *a, d.stream, weights=W.data_ptr()))
        o["ttk"] = d.f64(M, *TTK_GRID)
        h.travel_time_kernel(grid_r.data_ptr(), TTK_GRID[0], grid_d.data_ptr(), TTK_GRID[1], S - 1, o["ttk"].data_ptr(), d.stream)
        o["front"] = dict(T=d.f64(n, M), z=d.f64(n, M), p=d.f64(n, M), turns=d.i32(n, M))
        h.time_front(cols, *(o["front"][k].data_ptr() for k in ("T", "z", "p", "turns")), d.stream)
        return o

    es = per_ray(hs)
    eo = per_ray(ho, (es["B_nb"], es["B_ns"]))
    for name in es:
        _close(eo[name].cpu().numpy(), es[name].cpu().numpy(), f"{name} of the fan in the ODE sign", label)
    W = d.f64(S, M)
    total = es["A"] + es["B"]
    _lib.absorption_weights_device(env.device, total.data_ptr(), total.numel(), W.data_ptr(), d.stream)
    q = d.phase_index(es["kappa"], es["B_nb"], es["B_ns"])
    ps, po = products(hs, W, q, es["Phi"]), products(ho, W, q, es["Phi"])
    for name in ("I", "beams", "P", "P_phi", "BP", "BP_linear", "ttk"):
        a, b = (v[name] if isinstance(v[name], np.ndarray) else v[name].cpu().numpy() for v in (po, ps))
        _close(a, b, f"{name} of the fan in the ODE sign", label)
    same_arrivals(_host(po["arr"]), _host(ps["arr"]), label + " (arrivals of the fan in the ODE sign)")
    same_beam_arrivals(_host(po["ba"]), _host(ps["ba"]), "beam arrivals of the fan in the ODE sign", label)
    fs, fo = _host(ps["front"]), _host(po["front"])
    _close(fo["T"], fs["T"], "time_front T", label)
    assert np.array_equal(fo["turns"], fs["turns"]), (label, "time_front turns")
    for k in "zp":
        assert sign_flipped(fo[k], fs[k]), (label, "time_front", k)
    # none of it is vacuous: the products are lit, the stored-sign arrivals' p is the fan's own sign
    away = xs != xs[0]
    # (seed 225's beam field is NaN throughout, see the module's docstring: a cell other than 0.0 is a cell terms were added to)
    assert (ps["I"].cpu().numpy()[:, away] > 0).any() and (ps["BP"][:, away] != 0).any(), label
    assert np.isfinite(ps["ttk"].cpu().numpy()).any() and (ps["ttk"].cpu().numpy() != 0).any(), label
    assert _same(fs["z"], z[cols]) and int(ps["arr"]["offsets"][-1].item()) > 0, label
    hs.close()
    ho.close()
    rec = dict(rows=not env.blocked_layout, blocked=env.blocked_layout, dropped=M < len(y0), flat=flat, mirrored=mirrored)
    env.close()
    _SIGN_RECORDS[(seed, flat)] = rec
    return rec


@pytest.mark.parametrize("seed, flat", LEVEL1, ids=[f"seed{s}{'-flat' if fl else ''}" for s, fl in LEVEL1])
def test_fan_entries_agree_in_either_sign(pr, seed, flat):  # noqa: F811
    """A logged FanHandle in the stored sign and one in the ODE sign (stored_sign=False), otherwise launched alike: the fetches
    equal (z, p and the log's p with the sign bit flipped), and every product entry bit-equal given the same device arguments
    -- path_integral, boundary_loss (dB and lag tables, with nb / ns), caustic_index, intensity, beam_intensity,
    arrival_counts, arrivals (p in the stored sign from both), pressure, pressure_phi, beam_pressure with and without the
    curvature term, beam_arrival_counts and beam_arrivals (pgr_fan_beam_arrival_counts_w, pgr_fan_beam_arrivals_w: the list with
    the curvature term, whose times read p for p_m and the curvature), travel_time_kernel on a grid of its own -- and
    time_front with z and p as the fan holds them.  The
    stored-sign side is held to the restatements by test_kernels_and_fan_entries_on_random_raw_tables; its travel_time_kernel
    and time_front, which that test does not call, by tests/test_ttk_random_env.py (the kernel against ttk_reference and
    ttk_independent on a grid of that module's, both fan entries against the buffer entries and front_reference)."""
    _either_sign(pr, seed, flat)


def test_both_layouts_and_the_keep_list_are_met_in_the_ode_sign(pr):  # noqa: F811
    recs = [_either_sign(pr, seed, flat) for seed, flat in LEVEL1]
    tally = {k: int(sum(rec[k] for rec in recs)) for k in ("rows", "blocked", "dropped", "flat", "mirrored")}
    print(f"\n{len(recs)} fans in either sign: {tally}")
    # (rows: the LDS-table environments, of which the level-1 tally asserts 6)
    for k, least in (("rows", 6), ("blocked", 6), ("dropped", 4), ("flat", 6), ("mirrored", 6)):
        assert tally[k] >= least, (k, tally)


# ---- level 2: the API in four frames ------------------------------------------------------------------------------------------

def _in_place(fan):
    assert fan.device_resident and not any(k in fan.__dict__ for k in ("_ts", "_zs", "_ps"))


@pytest.mark.parametrize("fe", [False, True], ids=["flatearth-off", "flatearth-on"])
@pytest.mark.parametrize("backwards", [False, True], ids=["forwards", "backwards"])
@pytest.mark.parametrize("seed, lat", LEVEL2, ids=[f"seed{s}" for s, _ in LEVEL2])
def test_api_products_against_frames_derived_by_hand(pr, seed, lat, backwards, fe):  # noqa: F811
    arrs, src, th, kw, desc = api_case(seed)
    cin, cpin, rin, zin, bdep, brng, bang = arrs
    env = pr.OceanEnvironment2D(pr.DataArray(cin, dims=["range", "depth"], coords={"range": rin, "depth": zin}),
                                pr.DataArray(bdep, dims=["range"], coords={"range": brng}), lat=lat)
    S, w_min = kw["S"], MIN_WIDTHS[seed % 3]
    cols = columns(S)
    xs, xr = (kw["x1"], kw["x0"]) if backwards else (kw["x0"], kw["x1"])
    label = f"seed {seed} {'backwards' if backwards else 'forwards'} flatearth={fe}: {desc}"
    shot = dict(rtol=kw["rtol"], terminate_backwards=kw["terminate_backwards"], debug=False, flatearth=fe)
    plain = pr.shoot_rays(src, xs, th, xr, S, env, device_resident=False, **shot)
    K = max(1, int((np.asarray(plain.n_botts) + np.asarray(plain.n_surfs)).max()))
    host, dev = (pr.shoot_rays(src, xs, th, xr, S, env, device_resident=dr, max_bounces=K, **shot) for dr in (False, True))
    assert not host.device_resident and dev.device_resident and len(plain) == len(host) == len(dev) >= 64, label
    for k in ("ts", "zs", "ps", "n_botts", "n_surfs", "thetas"):
        assert _same(getattr(host, k), getattr(plain, k)), (label, k)
    log = host.bounces
    assert log.capacity == K and np.array_equal(log.count, np.asarray(host.n_botts) + np.asarray(host.n_surfs)), label
    for k in ("x", "p", "kind"):
        assert _same(getattr(dev.bounces, k), getattr(log, k)), (label, "the device fan's log", k)
    resident = dev._dev.fetch_samples()                                  # (S, M) copies: the fan itself stays where it is
    for k, name in (("T", "ts"), ("z", "zs"), ("p", "ps")):
        assert _same(resident[k].T, getattr(plain, name)), (label, "the device fan's", name)
    for k in ("n_botts", "n_surfs", "thetas"):
        assert _same(getattr(dev, k), getattr(plain, k)), (label, "the device fan's", k)
    # the frame, the launch slowness and the bottom slope from frame_independent alone
    x = np.asarray(host.rs, dtype=float)[0]
    assert x[0] == xs and x[-1] == xr
    xf, fcin, frin, fzin, fbd, fbr = fi.traced_frame(env, x, fe)
    beta = fi.bottom_slope(env, x)
    p0 = fi.launch_slowness(host.thetas, host.source_depths[0], xf, fcin, frin, fzin)
    depths = thinned_receivers(host.zs, float(fbd.max()), seed)
    R, n = len(depths), len(cols)
    bottom = bottom_of(pr, seed)
    fan = dict(ts=np.asarray(host.ts), zs=np.asarray(host.zs), ps=np.asarray(host.ps), x=xf, p0=p0, log=(log.x, log.p, log.kind))
    r = restate(fan, (fcin, frin, fzin, fbd, fbr), beta, bottom, seed, depths, cols, w_min=w_min)
    not_vacuous(r, xf, cols, label, beams=seed not in BEAM_EXEMPT_API)   # (the eikonal share: host.ts / zs / ps)
    f, absorption = r["f"], r["absorption"]
    u_ref = at_source_nan(r["u_raw"], xf, cols)
    H_ref = at_source_nan(band_sum(r, pr.thorp_absorption(r["freq"]) / 1000.0, R, n), xf, cols)
    bH_ref = at_source_nan(beam_band_sum(r, pr.thorp_absorption(r["freq"]) / 1000.0, R, n), xf, cols)
    weights = dict(absorption=absorption, bottom_loss=bottom, surface_loss=SURFACE_DB)
    loss = dict(bottom_loss=bottom, surface_loss=SURFACE_DB)
    every = np.arange(S)
    for fan_, where in ((dev, "device fan"), (host, "host fan")):
        lab = f"{label} ({where})"
        _close(pr.path_loss(fan_, env, absorption, flatearth=fe), r["A"], "path_loss", lab)
        _close(pr.path_length(fan_, env, flatearth=fe), r["L"], "path_length", lab)
        _close(pr.boundary_loss(fan_, env, flatearth=fe, **loss), r["B"], "boundary_loss", lab)
        _close(pr.boundary_loss(fan_, env, bottom_loss=bottom.lag, flatearth=fe), r["Phi"], "boundary_loss of the lag table", lab)
        nb, ns = fan_.bounce_counts(every)
        assert np.array_equal(nb, r["nb"]) and np.array_equal(ns, r["ns"]), (lab, "bounce_counts")
        assert np.array_equal(pr.caustic_index(fan_, env, flatearth=fe), r["kappa"]), (lab, "caustic_index")
        _close(pr.pressure_field(fan_, depths, env, f, flatearth=fe, **weights), r["P"], "pressure_field", lab)
        _close(pr.pressure_field(fan_, depths, env, f, flatearth=fe), r["P_plain"], "pressure_field without weights", lab)
        u = pr.received_signal(fan_, depths, env, f, r["band"], r["t0"], r["dt"], N_TIMES, range_indices=cols, flatearth=fe, **weights)
        _close(u, u_ref, "received_signal", lab)
        H = pr.transfer_function(fan_, depths, env, r["freq"], range_indices=cols, t_reduce=r["t0"], flatearth=fe,
                                 absorption=pr.thorp_absorption, **loss)
        _close(H, H_ref, "transfer_function", lab)
        a = pr.arrivals(fan_, depths, env, flatearth=fe, range_indices=cols, **weights)
        same_arrivals(dict(offsets=a.offsets, tube=a.tube, w=a.w, T=a.time, p=a.p, I=a.intensity), r["arr"], lab)
        _close(a.bottom_phase, r["phi"], "arrivals' bottom_phase", lab)
        assert np.array_equal(a.caustics, r["kappa"][a.tube, r["col"]]), (lab, "arrivals' caustics")
        _close(pr.transmission_loss(fan_, depths, env, flatearth=fe, intensity=True, **weights), r["I"], "transmission_loss", lab)
        _close(pr.beam_transmission_loss(fan_, depths, env, flatearth=fe, intensity=True, min_width=w_min, **weights), r["beams"],
               "beam_transmission_loss", lab)
        # the coherent beams: r["W"] holds the loss pair of `bottom`, which is what the beams take
        beam = dict(min_width=w_min, flatearth=fe, absorption=absorption, bottom_loss=bottom.loss, surface_loss=SURFACE_DB)
        field = pr.beam_pressure_field(fan_, depths, env, f, **beam)
        _close(field, r["BP"], "beam_pressure_field", lab)
        _close(pr.beam_pressure_field(fan_, depths, env, f, curvature=False, **beam), r["BP_linear"],
               "beam_pressure_field without the curvature term", lab)
        with np.errstate(divide="ignore", invalid="ignore"):
            tl = -20.0 * np.log10(np.abs(field))
        _close(pr.coherent_beam_transmission_loss(fan_, depths, env, f, **beam), tl, "coherent_beam_transmission_loss", lab)
        # the beam arrivals, with and without the curvature term, against the restatement from the definition; the host fan is
        # asked for the last column as -1
        asked = cols if fan_ is dev else [-1 if c == S - 1 else c for c in cols]
        at_source = x[cols] == x[0]
        for name, kw in (("ba", beam), ("ba_linear", dict(beam, curvature=False))):
            a = pr.beam_arrivals(fan_, depths, env, range_indices=asked, **kw)
            same_beam_arrivals(dict(offsets=a.offsets, tube=a.tube, image=a.image, time=a.time, amplitude=a.amplitude,
                                    q=a.phase_index), r[name], f"beam_arrivals ({name})", lab)
            assert np.array_equal(a.range_indices, cols) and _same(a.ranges, x[cols]) and _same(a.receiver_depths, depths), lab
            assert _same(a.intensity, a.amplitude ** 2) and len(a) == len(r[name]["tube"]) > 0, lab
            assert at_source.sum() == 1 and (np.diff(a.offsets).reshape(R, n)[:, at_source] == 0).all(), (lab, "the source's column")
        # the list summed by the public sums: at f it is the field, in the pulse and the band the restated sums
        H1 = pr.beam_transfer_function(fan_, depths, env, [f], range_indices=cols, **beam)
        assert H1.shape == (R, n, 1) and np.isnan(H1[:, at_source].real).all() and np.isnan(H1[:, at_source].imag).all(), lab
        _close(H1[:, :, 0], field[:, cols], "beam_transfer_function at f against beam_pressure_field", lab)
        ub = pr.beam_received_signal(fan_, depths, env, f, r["band"], r["t0"], r["dt"], N_TIMES, range_indices=cols, **beam)
        _close(ub, at_source_nan(r["bu_raw"], xf, cols), "beam_received_signal", lab)
        Hb = pr.beam_transfer_function(fan_, depths, env, r["freq"], range_indices=cols, t_reduce=r["t0"], min_width=w_min,
                                       flatearth=fe, absorption=pr.thorp_absorption, bottom_loss=bottom.loss, surface_loss=SURFACE_DB)
        _close(Hb, bH_ref, "beam_transfer_function with Thorp's absorption", lab)
        if fan_ is dev:
            with pytest.raises(ValueError, match="does not yet apply a complex bottom phase"):
                pr.beam_pressure_field(fan_, depths, env, f, **dict(beam, bottom_loss=bottom))
            with pytest.raises(ValueError, match="does not yet apply a complex bottom phase"):
                pr.beam_arrivals(fan_, depths, env, range_indices=cols, **dict(beam, bottom_loss=bottom))
            _in_place(dev)
        assert fan_.device_resident == (fan_ is dev), lab               # processed where it is
    _in_place(dev)


if __name__ == "__main__":
    cpu_check()
