"""travel_time_kernel without a GPU: the definition itself (its restatement in tests/ttk_reference.py) against closed forms
in an isovelocity medium and, entry by entry, against the independent reference (tests/ttk_independent.py); Simpson's rule
against the exact integral on the table's own grid; and the argument errors refused before anything reaches the device."""
import numpy as np
import pytest

import pygenray_amd as pr

import ttk_independent as tti
import ttk_reference as ttr

C0 = 1500.0
G = np.array([0.0, 2e3, 3e3, 5e3, 8e3, 9e3, 12e3])          # non-uniform kernel ranges
H = np.array([0.0, 100.0, 250.0, 300.0, 500.0, 800.0])      # non-uniform kernel depths
RIN, ZIN = np.array([-1e3, 20e3]), np.array([0.0, 3000.0, 6000.0])
CIN = np.full((2, 3), C0)


def _iso(x, d):
    """a ray through the samples (x, d) of an isovelocity medium: T is the polyline's length / C0.  (S, 1) rows."""
    T = np.concatenate([[0.0], np.cumsum(np.hypot(np.diff(x), np.diff(d)))]) / C0
    return T[:, None], -np.asarray(d, dtype=float)[:, None], np.asarray(x, dtype=float)


def _K(x, d, col=None, g=G, h=H):
    T, Z, x = _iso(x, d)
    return ttr.kernel(T, Z, x, g, h, CIN, RIN, ZIN, len(x) - 1 if col is None else col)[0], T[:, 0]


@pytest.mark.parametrize("b", [0, 1, 3, 5])
def test_a_horizontal_chord_along_a_depth_row_integrates_the_hat_functions(b):
    x = np.linspace(G[0], G[-1], 37)                          # save ranges off the grid lines: chords cross them
    K, _ = _K(x, np.full(len(x), H[b]))
    half = np.empty(len(G))
    half[1:-1] = (G[2:] - G[:-2]) / 2
    half[0], half[-1] = (G[1] - G[0]) / 2, (G[-1] - G[-2]) / 2
    np.testing.assert_allclose(K[:, b], -half / C0 ** 2, rtol=1e-12, atol=0)
    assert (np.delete(K, b, axis=1) == 0).all()


@pytest.mark.parametrize("case", ["sloping", "corner", "on_a_range_line", "on_a_depth_line", "outside", "col_middle"])
def test_the_kernel_sums_to_the_travel_time_over_c(case):
    col = None
    if case == "sloping":          # zig-zag, crossing many lines both ways
        x = np.linspace(-500.0, 12.5e3, 41)
        d = 400.0 + 380.0 * np.sin(x / 1.3e3)
    elif case == "corner":         # through the corner (2e3, 100) at parameter 0.5 of both cuts, then corner to corner
        x, d = np.array([1e3, 3e3, 5e3, 9e3, 11e3]), np.array([-50.0, 250.0, 500.0, 800.0, 900.0])
    elif case == "on_a_range_line":   # a vertical chord on x = G[3], then along it
        x = np.array([1e3, 5e3, 5e3, 7e3, 9e3])
        d = np.array([120.0, 260.0, 700.0, 710.0, 290.0])
    elif case == "on_a_depth_line":
        x = np.array([500.0, 2.5e3, 6e3, 9e3, 11e3])
        d = np.array([300.0, 300.0, 300.0, 500.0, 500.0])
    elif case == "outside":        # above the surface, below the last depth and past both range ends
        x = np.linspace(-3e3, 15e3, 23)
        d = np.linspace(-200.0, 1100.0, 23)
    else:
        x = np.linspace(0.0, 12e3, 25)
        d = 300.0 + 250.0 * np.cos(x / 2e3)
        col = 11
    K, T = _K(x, d, col)
    c = len(x) - 1 if col is None else col
    np.testing.assert_allclose(K.sum(), -(T[c] - T[0]) / C0, rtol=1e-12, atol=0)
    # on the table's own grid the same identity is K . cin = -(T_c - T_0)
    Kt, _ = _K(x, d, col, g=RIN, h=ZIN)
    np.testing.assert_allclose((Kt * CIN).sum(), -(T[c] - T[0]), rtol=1e-12, atol=0)


def test_rows_with_nan_and_column_zero():
    x = np.linspace(0.0, 12e3, 9)
    T, Z, _ = _iso(x, np.full(9, 200.0))
    T = np.concatenate([T, T, T], axis=1)
    Z = np.concatenate([Z, Z, Z], axis=1)
    T[6, 1] = np.nan                    # past column 5: kept
    Z[3, 2] = np.nan                    # at column 3: the row is NaN
    K = ttr.kernel(T, Z, x, G, H, CIN, RIN, ZIN, 5)
    assert np.isfinite(K[:2]).all() and np.isnan(K[2]).all()
    assert np.array_equal(K[0], K[1])
    assert (ttr.kernel(T, Z, x, G, H, CIN, RIN, ZIN, 0)[:2] == 0).all()


# ---- arguments refused before anything reaches the device ---------------------------------------------------------------

def _host_fan(n=3, S=5, rs=None):
    th = np.linspace(-5, 5, n)
    r = np.linspace(0, 10e3, S)
    zs = -(1000.0 + np.outer(np.tan(np.radians(th)), r))
    ps = np.tile(np.sin(np.radians(th))[:, None] / 1500.0, (1, S))
    ts = np.tile(r, (n, 1)) / 1500.0
    return pr.RayFan.from_arrays(th, np.tile(r, (n, 1)) if rs is None else rs, ts, zs, ps, np.zeros(n, np.int64),
                                 np.zeros(n, np.int64), np.linspace(900.0, 1100.0, n))


ENV = pr.OceanEnvironment2D(flat_earth_transform=False)


@pytest.mark.parametrize("kw, msg", [
    (dict(ranges=[0.0, 10.0, 5.0]), "ranges must be strictly ascending"),
    (dict(ranges=[0.0, 0.0, 5.0]), "ranges must be strictly ascending"),
    (dict(ranges=[0.0]), "ranges must be a 1-D sequence of at least 2"),
    (dict(ranges=[[0.0, 1.0]]), "ranges must be a 1-D sequence"),
    (dict(ranges=[0.0, np.inf]), "ranges must be finite"),
    (dict(depths=[1.0, np.nan]), "depths must be finite"),
    (dict(depths=[5.0, 1.0]), "depths must be strictly ascending"),
    (dict(depths=[]), "depths must be a 1-D sequence of at least 2"),
    (dict(range_index=5), "out of range"),
    (dict(range_index=-6), "out of range"),
    (dict(range_index=2.0), "must be an integer"),
    (dict(range_index=True), "must be an integer"),
    (dict(max_bytes=3 * 100 * 6000 * 8 - 1), f"needs {3 * 100 * 6000 * 8} bytes"),
    (dict(ranges=np.arange(65536.0), depths=[0.0, 1.0]), "ranges has 65536 values, more than the 65535 supported"),
    (dict(depths=range((1 << 30) + 1)), "depths has 1073741825 values, more than the 1073741824 supported"),
])
def test_arguments_are_checked(kw, msg):
    with pytest.raises(ValueError, match=msg):
        pr.travel_time_kernel(_host_fan(), ENV, flatearth=False, **kw)


def test_fans_that_cannot_give_a_kernel_are_refused():
    rs = np.tile(np.linspace(0, 10e3, 5), (3, 1))
    rs[1, 2] += 1.0
    with pytest.raises(ValueError, match="rows of rays.rs differ"):
        pr.travel_time_kernel(_host_fan(rs=rs), ENV, flatearth=False)
    with pytest.raises(ValueError, match="Flat earth transformation has not been applied"):
        pr.travel_time_kernel(_host_fan(), ENV)
    with pytest.raises(ValueError, match="RayFan or EigenRays"):
        pr.travel_time_kernel(np.zeros((3, 5)), ENV, flatearth=False)


def test_travel_time_kernel_is_exported():
    assert "travel_time_kernel" in pr.__all__ and callable(pr.travel_time_kernel)


# ---- the restatement entry by entry against the independent reference (tests/ttk_independent.py) ----------------------

def _against_independent(T, Z, x, g, h, cin, rin, zin, col):
    """ttk_reference.kernel (float64, the kernel's operations) against ttk_independent.kernel (exact geometry, 60 digits):
    NaN rows alike, and every entry within the rounding bound that ttk_independent's docstring derives from the operation
    order (no fitted constant).  The bound must also be small against the entries, or it would prove nothing."""
    K = ttr.kernel(T, Z, x, g, h, cin, rin, zin, col)
    Ki, mag, bound = tti.kernel(T, Z, x, g, h, cin, rin, zin, col)
    assert np.array_equal(np.isnan(K), np.isnan(Ki))
    f = np.isfinite(Ki)
    err = np.abs(K - Ki)[f]
    assert (err <= bound[f]).all(), np.max(err - bound[f])
    assert (K[f][bound[f] == 0] == 0).all()
    if f.any() and col > 0:
        assert bound[f].max() < 1e-9 * np.abs(Ki[f]).max()
    return K, Ki


def _table():
    """syn_env's range-dependent table (tests/tube_gpu.py)"""
    from tube_gpu import SYN_R, SYN_Z, syn_cin
    return syn_cin(), SYN_R, SYN_Z


GU = np.array([-400.0, 3.3e3, 7e3, 17.5e3, 18e3, 31e3, 44.4e3, 59e3])     # user grids off the table's lines
HU = np.array([0.0, 35.0, 240.0, 610.0, 1215.0, 1300.0, 2900.0, 4870.0])


def _rays(x, d):
    """T (with a non-isovelocity, per-chord spread), Z rows of the depth paths d (S, M) at ranges x"""
    d = np.asarray(d, dtype=float)
    T = np.concatenate([np.zeros((1, d.shape[1])), np.cumsum(np.hypot(np.diff(x)[:, None], np.diff(d, axis=0)), axis=0)])
    T = T / 1500.0 + 1e-4 * np.arange(len(x))[:, None] ** 0.5
    return T, -d


@pytest.mark.parametrize("grid", ["table", "user"])
def test_restatement_against_the_independent_reference(grid):
    """the range-dependent table, on its own grid and on a non-uniform user grid whose lines are not the table's: rays
    wandering over the whole grid, up and down, past every edge"""
    cin, rin, zin = _table()
    g, h = (rin, zin) if grid == "table" else (GU, HU)
    rng = np.random.default_rng(3)
    x = np.linspace(-2.5e3, 62e3, 31)
    d = np.cumsum(rng.normal(0.0, 400.0, (31, 5)), axis=0) + rng.uniform(-200.0, 5200.0, 5)
    T, Z = _rays(x, d)
    for col in (30, 17):
        _against_independent(T, Z, x, g, h, cin, rin, zin, col)


def test_lines_corners_and_degenerate_chords():
    """samples on range and depth lines and on grid corners, chords through corners, vertical and level chords (on and off a
    line), chords leaving a depth line upward and downward, and a zero-length chord"""
    cin, rin, zin = _table()
    g, h = GU, HU
    x = np.array([g[1], g[2], g[2], g[3], g[4], g[4], g[5], g[6]])
    d = np.array([
        [h[1], h[2], h[4], h[3], 5.0, h[3], h[2], h[1]],               # corner to corner, vertical on a corner, a
                                                                       # steep climb from a corner, level on a line
        [h[3], h[2] + 50.0, h[2] + 50.0, h[5], h[2], h[2] - 90.0, h[6], h[6]],   # leaves a depth line upward
        [h[2], h[3], 700.0, h[2], h[2] - 10.0, h[2] - 10.0, h[1], h[1]],   # upward from a line mid-chord, downward
        [h[4], h[4], h[4], h[4], h[4], h[4], h[4], h[4]],              # level on a depth line throughout
        [600.0, 600.0, 900.0, 4000.0, 50.0, 50.0, 3000.0, 2950.0],     # a zero-length chord (samples 4 -> 5)
        [h[2], 10.0, h[5], 2000.0, 2100.0, h[5], h[4], h[2]],           # upward out of a corner
    ]).T
    T, Z = _rays(x, d)
    _against_independent(T, Z, x, g, h, cin, rin, zin, len(x) - 1)


def test_outside_the_grid_zero_chords_and_nan_rows():
    """rays wholly above, below, left and right of the grid, a ray of zero-length chords, NaN samples (one at the end
    column: the row is NaN; one past it: kept) and column 0"""
    cin, rin, zin = _table()
    g, h = GU[1:-1], HU[1:-1]
    x = np.linspace(-6e3, 66e3, 13)
    d = np.stack([np.linspace(-300.0, -5.0, 13), np.linspace(h[-1] + 10.0, 5400.0, 13),
                  np.linspace(100.0, 4000.0, 13), np.full(13, 1000.0), np.linspace(4000.0, 20.0, 13)], axis=1)
    T, Z = _rays(x, d)
    T[:, 3] = 7.0                                      # dT = 0 on every chord
    T[9, 4] = np.nan
    Z[11, 2] = np.nan
    for col in (12, 10, 0):
        K, _ = _against_independent(T, Z, x, g, h, cin, rin, zin, col)
        assert np.isnan(K[4]).all() == (col >= 9) and np.isnan(K[2]).all() == (col >= 11)
    x2 = np.array([-5e3, -1e3, 2e3, 30e3, 61e3, 70e3])         # left of the grid, through it, right of it
    T, Z = _rays(x2, np.tile(np.array([[900.0], [1000.0], [1000.0], [1500.0], [2000.0], [2100.0]]), (1, 2)))
    Z[:, 1] = -np.array([900.0, 900.0, 900.0, 900.0, 900.0, 900.0])
    _against_independent(T, Z, x2, g, h, cin, rin, zin, 5)


def test_simpson_rule_against_the_exact_integral_on_the_tables_own_grid():
    """On the table's own grid every piece lies in one table cell, where c and phi are quadratic along the chord: the
    definition (Simpson) differs from the exact integral of its own look-up by at most Simpson's remainder ell / 2880
    sup|F''''| per piece (ttk_independent._remainder bounds F'''' from the piece's c and phi), carried through the chord's
    quotient Q_ab / Q_1; both exact values are then rounded once (eps |K| each).  K is the derivative of the fan's own
    model entry by entry.  (a) A Munk path at the 100 km / 1001-sample spacing on the 1 m table: the remainder is far
    below rounding there.  (b) Steep long chords on a coarse, strongly varying table: the remainder is large, and the
    actual difference reaches a good fraction of it, so the bound is not vacuous."""
    import pygenray_amd as pr
    z, r = np.arange(0.0, 6000.0, 1.0), np.linspace(0.0, 200e3, 100)
    munk = (np.tile(pr.munk_ssp(z), (100, 1)), r, z)
    x = np.linspace(0.0, 100e3, 1001)[:241]
    rc, zc = np.array([0.0, 10e3, 25e3, 40e3]), np.array([0.0, 400.0, 1500.0, 3000.0, 5000.0])
    rr, zz = np.meshgrid(rc, zc, indexing="ij")
    coarse = (1500.0 + 60.0 * np.cos(zz / 700.0) + 20.0 * np.sin(rr / 9e3), rc, zc)
    x2 = np.array([0.0, 3e3, 9e3, 16e3, 24e3, 33e3, 40e3])
    cases = [(munk, x, 1000.0 + 700.0 * np.sin(2 * np.pi * x / 47e3), False),
             (coarse, x2, np.array([10.0, 4900.0, 200.0, 4500.0, 100.0, 4000.0, 50.0]), True)]
    for (cin, rin, zin), xs, d, steep in cases:
        T, Z = _rays(xs, d[:, None])
        col = len(xs) - 1
        K, _, _, rem = tti.kernel(T, Z, xs, rin, zin, cin, rin, zin, col, remainder=True)
        Ke = tti.kernel(T, Z, xs, rin, zin, cin, rin, zin, col, rule="exact")[0]
        diff = np.abs(K - Ke)
        assert (diff <= rem + tti.EPS * (np.abs(K) + np.abs(Ke))).all()
        if steep:
            assert diff.max() > 0.1 * rem.max() and rem.max() > 1e-6 * np.abs(K).max()
