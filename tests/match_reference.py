"""Test helpers for matched_field / beam_matched_field (not a product path): DESIGN.md section 24 restated in plain NumPy in its
operation order -- band_reference.band_terms' (re, im) per group and frequency, the fold over the elements in increasing j,
A = cr cr + ci ci, the division by nn, then the 64 lane partials in increasing k and the xor tree -- and the set-up shared by the
CPU and GPU tests: localisation on Lloyd's mirror with section 20's exact straight rays shot from eight array elements, with
the errors measured on the CPU (tests/test_match_host.py prints them)."""
import numpy as np

import arrivals_reference as aref
import band_reference as bref
import beam_arrivals_reference as baref
import beam_pressure_reference as bp

LANES = bref.LANES


def match_terms(off, n_elements, T, I, q, phi, L, freq, alpha):
    """(re, im), each (N, G, F): band_reference.band_terms over the N * G groups, element-major"""
    re, im = bref.band_terms(off, T, I, q, phi, L, freq, alpha)
    G = (len(off) - 1) // n_elements
    assert n_elements * G == len(off) - 1
    return re.reshape(n_elements, G, -1), im.reshape(n_elements, G, -1)


def fold_elements(re, im, data, normalize):
    """re, im (N, G, F) and the data (N, F) complex -> B (G, F): cr, ci and nn folded over j = 0 ... N - 1 in increasing j,
    A = cr cr + ci ci, with `normalize` 0.0 where nn == 0.0 and A / nn elsewhere"""
    re, im = np.asarray(re, dtype=float), np.asarray(im, dtype=float)
    d = np.asarray(data, dtype=np.complex128)
    N, G, F = re.shape
    assert d.shape == (N, F)
    cr, ci, nn = np.zeros((G, F)), np.zeros((G, F)), np.zeros((G, F))
    with np.errstate(invalid="ignore", over="ignore", divide="ignore"):
        for j in range(N):
            dr, di = d[j].real[None, :], d[j].imag[None, :]
            rr, ii = re[j] * dr, im[j] * di
            cr = cr + (rr + ii)
            ri, ir = re[j] * di, im[j] * dr
            ci = ci + (ri - ir)
            r2, i2 = re[j] * re[j], im[j] * im[j]
            nn = nn + (r2 + i2)
        c2, s2 = cr * cr, ci * ci
        A = c2 + s2
        if not normalize:
            return A
        return np.where(nn == 0.0, 0.0, A / np.where(nn == 0.0, 1.0, nn))


def reduce_lanes(B, wf):
    """band_reference.reduce_band's sibling for a B_k already formed: B (G, F) and the weights wf (F,) -> out (G,), the lane
    partials s_l over k = l, l + 64, ... in increasing k, the six exchanges of the xor tree on all 64 lanes at once, lane 0"""
    B, wf = np.asarray(B, dtype=float), np.asarray(wf, dtype=float)
    G, F = B.shape
    with np.errstate(invalid="ignore", over="ignore"):
        s = np.zeros((G, LANES))
        for k in range(F):
            s[:, k % LANES] = s[:, k % LANES] + wf[k] * B[:, k]
        lane = np.arange(LANES)
        for d in (32, 16, 8, 4, 2, 1):
            s = s + s[:, lane ^ d]
    return s[:, 0].copy()


def reduce_match(re, im, data, wf, normalize):
    """the defined reduction of the elements' transfer functions re, im (N, G, F) -> out (G,)"""
    return reduce_lanes(fold_elements(re, im, data, normalize), wf)


def match_power(off, n_elements, T, I, q, phi, L, freq, alpha, wf, data, normalize):
    """The definition, restated -> out (G,) float64"""
    re, im = match_terms(off, n_elements, T, I, q, phi, L, freq, alpha)
    return reduce_match(re, im, data, wf, normalize)


def normalised_weights(w, data):
    """the kernel's weights of the normalised processor: w_k / sum_j |d_jk|^2"""
    d = np.asarray(data, dtype=np.complex128)
    return np.asarray(w, dtype=float) / (d.real * d.real + d.imag * d.imag).sum(axis=0)


# ---- localisation on Lloyd's mirror, on section 20's exact straight rays --------------------------------------------------------
# beam_pressure_reference's medium: isovelocity 1500 m/s under a pressure-release surface.  The array: 8 elements at 300 ... 650 m
# every 50 m at range 0, a fan of 4001 straight rays over +-40 degrees shot from each.  The candidate cells: LLOYD_DEPTHS (75 ...
# 925 m every 50 m) x 2, 3, 4, 5 km, 72 in all.  The band: band_reference.BAND_FREQ, 64 frequencies over 60 ... 90 Hz.  The data
# are the closed form of a true source at 425 m / 3 km seen by each element, and the yardstick is the same Bartlett processor
# run on closed-form replicas: geometry alone.

ELEMENT_DEPTHS = np.arange(300.0, 651.0, 50.0)
TRUE_CELL = (7, 1)                                        # LLOYD_DEPTHS[7] = 425 m, EXACT_RANGES[1] = 3 km
OTHER_TRUE_CELLS = ((3, 2), (14, 0))                      # 225 m / 4 km and 775 m / 2 km
# the worst |B - B_closed| over all 72 cells of the restatement under uniform weights with the true source in TRUE_CELL, on the
# tube lists and on the beam lists at min_width 10 m with curvature (tests/test_match_host.py prints them); the bounds are twice
# them (DESIGN.md section 19's rule: the margin covers the GPU's table look-up)
MATCH_LLOYD_MEASURED = 2.932073267014612e-06
MATCH_LLOYD_BEAM_MEASURED = 1.8149009716472708e-06


def lloyd_field(src_depth, src_range, rcv_depth, rcv_range, freq=bref.BAND_FREQ, surface=-1.0):
    """e^{2 pi i f R1 / c} / R1 + surface e^{2 pi i f R2 / c} / R2 between two points; the leading axes broadcast, the last
    axis is the frequency"""
    dx = np.asarray(rcv_range, dtype=float) - np.asarray(src_range, dtype=float)
    R1 = np.hypot(dx, np.asarray(rcv_depth, dtype=float) - src_depth)[..., None]
    R2 = np.hypot(dx, np.asarray(rcv_depth, dtype=float) + src_depth)[..., None]
    f = np.asarray(freq, dtype=float)
    return np.exp(2j * np.pi * f * R1 / bp.EXACT_C) / R1 + surface * np.exp(2j * np.pi * f * R2 / bp.EXACT_C) / R2


def lloyd_data(cell=TRUE_CELL, freq=bref.BAND_FREQ):
    """the snapshot (8, F) of a true source in `cell` = (depth index, range index) at the elements"""
    return lloyd_field(bp.LLOYD_DEPTHS[cell[0]], bp.EXACT_RANGES[cell[1]], ELEMENT_DEPTHS, 0.0, freq)


def lloyd_closed_replicas(freq=bref.BAND_FREQ, surface=-1.0):
    """the closed-form replicas (8, 18, 4, F): the field at element j of a source in every cell"""
    D, X = bp.LLOYD_DEPTHS[None, :, None], bp.EXACT_RANGES[None, None, :]
    return lloyd_field(D, X, ELEMENT_DEPTHS[:, None, None], 0.0, freq, surface)


def bartlett_closed(data, w, replicas=None):
    """sum_k w_k |sum_j conj(H_jk) d_jk|^2 / (sum_j |H_jk|^2 sum_j |d_jk|^2) on closed-form replicas, in NumPy's own order ->
    (18, 4)"""
    H = lloyd_closed_replicas() if replicas is None else replicas
    d = np.asarray(data)[:, None, None, :]
    num = np.abs((np.conj(H) * d).sum(axis=0)) ** 2
    den = (np.abs(H) ** 2).sum(axis=0) * (np.abs(d) ** 2).sum(axis=0)
    return (np.asarray(w) * num / den).sum(axis=-1)


_LISTS = {}


def element_tube_lists():
    """the ray-tube arrivals of beam_pressure_reference.exact_fan(z_j) for the 8 elements at the 72 cells, joined element-major
    -> (offsets [8 * 72 + 1], T, I, q per arrival); computed once"""
    if "tubes" not in _LISTS:
        parts = []
        for zj in ELEMENT_DEPTHS:
            zs, ps, ts, x, p0, q = bp.exact_fan(zj)
            a = aref.tube_arrivals(zs, ps, ts, x, p0, bp.LLOYD_DEPTHS, bref.BAND_COLS, bp.EXACT_CIN, bp.EXACT_RIN, bp.EXACT_ZIN)
            slot = np.repeat(np.arange(len(a["offsets"]) - 1), np.diff(a["offsets"])) % len(bref.BAND_COLS)
            parts.append((a["offsets"], a["T"], a["I"], q[a["tube"], np.asarray(bref.BAND_COLS)[slot]]))
        _LISTS["tubes"] = join_lists(parts)
    return _LISTS["tubes"]


def element_beam_lists(w_min=10.0, curvature=True, save_spacing=0.0):
    """the beam arrivals of the same 8 fans -> (offsets, T, I = amplitude * amplitude, q); computed once per setting.
    `save_spacing` > 0: of `resampled_fan` instead of the exact fan"""
    key = ("beams", w_min, curvature, save_spacing)
    if key not in _LISTS:
        parts = []
        for zj in ELEMENT_DEPTHS:
            zs, ps, ts, x, p0, q = resampled_fan(zj, save_spacing)
            b = baref.beam_arrivals(zs, ps, ts, x, p0, bp.LLOYD_DEPTHS, bp.EXACT_CIN, bp.EXACT_RIN, bp.EXACT_ZIN,
                                    np.full(len(x), bp.EXACT_BOTTOM), w_min, None, q, [1, 2, 3, 4], curvature)
            parts.append((b["offsets"], b["time"], b["amplitude"] * b["amplitude"], b["q"]))
        _LISTS[key] = join_lists(parts)
    return _LISTS[key]


# ---- what a traced fan's samples next to a surface reflection are, and what that asks of its save grid -----------------------------
# shoot_rays keeps the reference's re-sampling (RayFan.bounce_counts): a bounce belongs to its NEAREST save
# range, so a ray that meets the surface up to half a save spacing BEHIND a save range already has, at that range, the sample of
# its reflected segment carried backwards -- above the surface by up to h = (spacing / 2) tan(theta), with its slowness turned and
# its bounce counted.  The tube folded over the surface then joins a ray h above the surface to one h below it: it is up to 2 h wide,
# and section 10 makes the beams beside a folded tube as wide as that tube.  Those beams reach 4 sigma: a receiver deeper than
# h + 4 max(min_width, 2 h) sees none of this, and there a traced fan and the exact fan give one list of beam arrivals.

def fold_reach(save_spacing, w_min=10.0):
    """the depth down to which the beams beside the fold at the surface reach, for the steepest ray that meets the surface at the
    nearest of the ranges from the deepest element: h + 4 max(w_min, 2 h), h = (save_spacing / 2) z_max / r_min"""
    h = 0.5 * save_spacing * ELEMENT_DEPTHS.max() / bp.EXACT_RANGES.min()
    return h + 4.0 * max(w_min, 2.0 * h)


def resampled_fan(source_depth, save_spacing, ranges=bp.EXACT_RANGES):
    """beam_pressure_reference.exact_fan with the samples next to a surface reflection as a traced fan on a save grid of
    `save_spacing` metres has them (0.0: exact_fan itself): a ray that meets the surface at x_b <= x + save_spacing / 2 counts
    as reflected at the range x, and where x < x_b its sample there is the reflected segment's carried backwards, above the surface"""
    th = np.radians(np.linspace(-bp.EXACT_APERTURE, bp.EXACT_APERTURE, bp.EXACT_N))
    p0 = np.sin(th) / bp.EXACT_C
    x = np.concatenate([[0.0], np.asarray(ranges, dtype=float)])
    t = np.tan(th)[:, None]
    zu = source_depth + x[None, :] * t                              # + down, unfolded
    with np.errstate(divide="ignore", invalid="ignore"):
        xb = np.where(t < 0, -source_depth / t, np.inf)             # where the ray meets the surface
    refl = (xb <= x[None, :] + 0.5 * save_spacing) & (x[None, :] > 0)
    depth = np.where(refl, -zu, zu)
    p = np.where(refl, -p0[:, None], p0[:, None])
    T = x[None, :] / (bp.EXACT_C * np.cos(th))[:, None]
    ns = refl.astype(np.int64)
    q = np.zeros(zu.shape, np.int32)
    q[:-1] = np.where(ns[:-1] == ns[1:], 2 * ns[:-1], -1)
    return -depth, -p, T, x, p0, q


# the save grid of the GPU test's fans: 20 m (S = 251 over 5 km), for which fold_reach is 43.25 m, above the shallowest cell at 75 m;
# at 100 m (S = 51) it is 146.25 m and the cells at 75 m and 125 m see the fold (tests/test_match_host.py)
LLOYD_SAVE_SPACING = 20.0


def join_lists(parts):
    """[(offsets, a, b, ...), ...] per element -> (offsets, a, b, ...) element-major, the offsets of element j shifted by the
    arrivals before it"""
    shift = np.concatenate([[0], np.cumsum([int(p[0][-1]) for p in parts])])
    off = np.concatenate([np.asarray(parts[0][0], dtype=np.int64)] +
                         [np.asarray(p[0], dtype=np.int64)[1:] + s for p, s in zip(parts[1:], shift[1:])])
    return (off,) + tuple(np.concatenate([np.asarray(p[i]) for p in parts]) for i in range(1, len(parts[0])))


def as_cells(out):
    return np.asarray(out).reshape(len(bp.LLOYD_DEPTHS), len(bref.BAND_COLS))
