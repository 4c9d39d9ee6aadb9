"""travel_time_kernel without a GPU: the definition itself (its restatement in tests/ttk_reference.py) against closed forms
in an isovelocity medium, and the argument errors refused before anything reaches the device."""
import numpy as np
import pytest

import pygenray_amd as pr

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
