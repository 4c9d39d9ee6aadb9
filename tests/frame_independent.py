"""Test helper (not a test module, not a product path): the tables of the frame a fan was traced in, derived from an
``OceanEnvironment2D`` and the fan's save ranges in plain NumPy, WITHOUT the package's own frame helpers
(``_unpack_envi``, ``_mirror_envi_arrays``, ``bilinear_interp`` / ``linear_interp``, ``_initial_slowness``): nothing is
imported from ``pygenray_amd``; the environment object handed in is only read (``sound_speed``, ``bathymetry``,
``latitude``: the user's own tables, not the ``*_fe`` ones the package derived from them).

What the definition of the tube products says (DESIGN.md sections 8-10), restated:

- the sound speed is a (range, depth) table on the environment's range and depth coordinates; the bathymetry has a range
  grid of its own;
- ``flatearth=True``: depths (the table's depth grid and the bathymetry) and sound speeds go through the flat-earth map
  (SURVEY.md a18): ``depf = dep (1 + E (1/2 + E / 3))``, ``csf = cs (1 + E (1 + E))``, ``E = dep / re(lat)``, ``re`` the
  WGS-84 radius at the environment's latitude;
- a backwards fan (save ranges decreasing) was traced in the mirrored frame x' = -x: ranges negated and reversed, table
  rows reversed, the bathymetry likewise; its save ranges are -x;
- the bottom slope at a bounce comes from the bathymetry as the user gave it, flat-earth mapped or not:
  ``degrees(arctan(np.gradient(bathymetry, its ranges)))`` on the bathymetry's ranges; negated and reversed in the mirrored
  frame;
- the bottom at a save range is the linear interpolation of the bathymetry (cell = searchsorted - 1, clamped; weights not
  clamped);
- ``p0 = sin(radians(theta)) / c_source``, ``c_source`` the bilinear look-up at (the traced frame's first save range, the
  source depth).
"""
import numpy as np

import tl_reference as tlr

WGS84_A = 6378137.0
WGS84_B = 6356752.314


def earth_radius(lat_deg):
    """WGS-84 radius at a latitude: a^2 / sqrt(a^2 cos^2 + b^2 sin^2) * sqrt(cos^2 + (b / a)^4 sin^2)"""
    a2, b2 = WGS84_A * WGS84_A, WGS84_B * WGS84_B
    ratio4 = (WGS84_B / WGS84_A) ** 4
    phi = np.pi * lat_deg / 180.0
    co, si = np.cos(phi), np.sin(phi)
    return a2 / np.sqrt(a2 * co * co + b2 * si * si) * np.sqrt(co * co + ratio4 * si * si)


def flat_depth(dep, lat_deg):
    e = dep / earth_radius(lat_deg)
    return dep * (1.0 + e * (0.50 + e / 3.0))


def flat_speed(c, dep, lat_deg):
    e = dep / earth_radius(lat_deg)
    return c * (1.0 + e * (1.0 + e))


def _coord(da, name):
    c = da.coords[name]
    return np.array(getattr(c, "values", c), dtype=float)


def tables(environment, flatearth):
    """-> (cin (nr, nz), rin, zin, bottom depths, their ranges) of the un-mirrored frame, read from the environment's own
    ``sound_speed`` / ``bathymetry`` and flat-earth mapped here when ``flatearth``."""
    ss, ba = environment.sound_speed, environment.bathymetry
    cin = np.array(ss.values, dtype=float)
    if tuple(ss.dims) == ("depth", "range"):
        cin = cin.T.copy()
    assert tuple(ss.dims) in (("range", "depth"), ("depth", "range")) and tuple(ba.dims) == ("range",)
    rin, zin = _coord(ss, "range"), _coord(ss, "depth")
    bd, br = np.array(ba.values, dtype=float), _coord(ba, "range")
    if flatearth:
        lat = environment.latitude
        cin = np.stack([flat_speed(row, zin, lat) for row in cin])
        zin = flat_depth(zin, lat)
        bd = flat_depth(bd, lat)
    return cin, rin, zin, bd, br


def traced_frame(environment, x, flatearth):
    """The frame a fan with save ranges x (S,) was traced in -> (xf, cin, rin, zin, bottom depths, their ranges)."""
    x = np.array(x, dtype=float)
    cin, rin, zin, bd, br = tables(environment, flatearth)
    if len(x) > 1 and x[-1] < x[0]:                      # backwards: x' = -x
        n, nb = len(rin), len(br)
        flip, flip_b = np.arange(n - 1, -1, -1), np.arange(nb - 1, -1, -1)
        cin, rin, bd, br = cin[flip], -rin[flip], bd[flip_b], -br[flip_b]
        x = -x
    return x, np.ascontiguousarray(cin), rin, zin, bd, br


def bottom_slope(environment, x):
    """The bottom slope of the frame a fan with save ranges x (S,) was traced in -> (its ranges, degrees): the slope of the
    UNTRANSFORMED bathymetry, degrees(arctan(d depth / d range)) by np.gradient on the bathymetry's own range grid, whatever
    ``flatearth`` is (the reference's quirk Q10); negated and reversed, with the ranges, for a backwards fan."""
    x = np.array(x, dtype=float)
    ba = environment.bathymetry
    br = _coord(ba, "range")
    beta = np.degrees(np.arctan(np.gradient(np.array(ba.values, dtype=float), br)))
    if len(x) > 1 and x[-1] < x[0]:
        flip = np.arange(len(br) - 1, -1, -1)
        br, beta = -br[flip], -beta[flip]
    return br, beta


def bottom_at(xf, bd, br):
    """the bathymetry (bd on br) interpolated linearly at xf"""
    xf = np.asarray(xf, dtype=float)
    i = np.clip(np.searchsorted(br, xf) - 1, 0, len(br) - 2)
    w = (xf - br[i]) / (br[i + 1] - br[i])
    return (1 - w) * bd[i] + w * bd[i + 1]


def launch_slowness(thetas, source_depth, xf, cin, rin, zin):
    """p0 (M,) = sin(radians(theta)) / c_source, the source at the traced frame's first save range"""
    c_source = float(tlr.bilinear(xf[0], float(source_depth), rin, zin, cin))
    return np.sin(np.radians(np.asarray(thetas, dtype=float))) / c_source
