"""Time fronts and turning-point counts on the GPU: the kernel alone through _lib.time_front_device against the restatement
(tests/front_reference.py) on synthetic buffers, then device-resident fans in both trajectory layouts, with dropped rays,
backwards and in the flat-earth frame, against the same fan shot eagerly; the ray ids, the arrivals' counts, repeatability
and the error paths of both C entries.  Every comparison is exact: integer counts and copied samples, the same in the
reference and the contracted build."""
import numpy as np
import pytest

import front_reference as fr
from tube_gpu import DEPTHS, _same, munk_env, pr_any, sloping_env, sloping_env_shallow_table  # noqa: F401

pytestmark = pytest.mark.gpu

PAD = 130                    # entries behind every output that must stay as they were
MARK_F, MARK_I = -7.25, -77


# ---- the kernel alone ---------------------------------------------------------------------------------------------------

def _device_front(T, z, p, cols, want=(True, True, True, True), device=0):
    """_lib.time_front_device on the (M, S) host blocks, uploaded as [S][M] rows -> [T, z, p, turns] (M, n) each (None
    where not asked for); outputs pre-filled with a sentinel, PAD entries behind each checked untouched"""
    import torch
    from pygenray_amd import _lib
    dev = torch.device("cuda", device)
    M, S = p.shape
    n = len(cols)
    rows = [torch.from_numpy(np.ascontiguousarray(a.T)).to(dev) for a in (T, z, p)]
    outs = [torch.full((n * M + PAD,), MARK_F, dtype=torch.float64, device=dev) if w else None for w in want[:3]]
    outs.append(torch.full((n * M + PAD,), MARK_I, dtype=torch.int32, device=dev) if want[3] else None)
    ins = [r.data_ptr() if (w or (k == 2 and want[3])) else 0 for k, (r, w) in enumerate(zip(rows, want[:3]))]
    _lib.time_front_device(device, *ins, M, S, cols, *(o.data_ptr() if o is not None else 0 for o in outs),
                           torch.cuda.current_stream(dev).cuda_stream)
    res = []
    for o, mark in zip(outs, (MARK_F, MARK_F, MARK_F, MARK_I)):
        if o is None:
            res.append(None)
            continue
        h = o.cpu().numpy()
        assert (h[n * M:] == mark).all()                       # nothing beyond n_cols x M is written
        res.append(h[:n * M].reshape(n, M).T)
    return res


def _check(T, z, p, cols, want=(True, True, True, True)):
    got = _device_front(T, z, p, cols, want)
    ref = [fr.gather(T, cols), fr.gather(z, cols), fr.gather(p, cols), fr.turning_points(p, cols)]
    for g, r, w in zip(got, ref, want):
        assert (g is not None) == w
        if w:
            assert g.shape == r.shape and _same(g, r)           # every slot (a skipped one would hold the sentinel)
    if want[3]:
        assert got[3].dtype == np.int32


@pytest.mark.parametrize("S", [1, 2, 5, 200, 1001])
@pytest.mark.parametrize("M", [1, 63, 64, 65, 4035])
def test_kernel_equals_the_restatement_on_synthetic_buffers(pr_any, M, S):
    T, z, p = fr.synthetic(M, S, 1000 * M + S)
    assert np.isnan(p[0, 0]) and np.isnan(p[-1, -1])
    if M * S >= 300:
        assert (p == 0).any() and np.signbit(p[p == 0]).any() and not np.signbit(p[p == 0]).all()
    for cols in fr.column_cases(S, M + S):
        _check(T, z, p, cols)


@pytest.mark.parametrize("M, S", [(65, 5), (300, 200), (4035, 1001)])
def test_each_output_may_be_left_out(pr_any, M, S):
    T, z, p = fr.synthetic(M, S, 5 * M + S)
    cols = fr.column_cases(S, 3)[3]
    for k in range(4):
        _check(T, z, p, cols, tuple(j != k for j in range(4)))
    _check(T, z, p, cols, (False, False, False, True))          # the count alone: T and z are not passed at all
    _check(T, z, p, cols, (True, False, False, False))          # one gather alone: p is not passed at all


def test_a_second_call_gives_the_same_arrays(pr_any):
    T, z, p = fr.synthetic(1000, 333, 9)
    cols = fr.column_cases(333, 1)[3]
    a, b = _device_front(T, z, p, cols), _device_front(T, z, p, cols)
    assert all(_same(x, y) for x, y in zip(a, b))


# ---- fans ---------------------------------------------------------------------------------------------------------------

def _shoot(pr, env, resident, src=(1000.0, 0.0), x1=100e3, S=201, n=300, flatearth=False, amax=20.0):
    return pr.shoot_rays(src[0], src[1], np.linspace(-amax, amax, n), x1, S, env, flatearth=flatearth, debug=False,
                         device_resident=resident)


def _in_place(fan):
    assert fan.device_resident
    assert not any(k in fan.__dict__ for k in ("_ts", "_zs", "_ps"))


def _check_device_fan(pr, dev, eager, env, flatearth=False):
    """everything the feature offers on the device-resident fan `dev`, against the restatement of the eager fan"""
    M, S = np.shape(eager.ps)
    assert len(dev) == M and M > 0 and _same(dev.thetas, eager.thetas)
    cols = [0, 1, S // 2, S - 1, S // 2, 3]
    want = fr.turning_points(eager.ps, cols)
    got = dev.turning_points([0, 1, S // 2, -1, S // 2, 3])
    assert got.dtype == np.int64 and np.array_equal(got, want)
    assert np.array_equal(dev.turning_points(), want[:, 3:4])
    assert np.array_equal(eager.turning_points(cols), want)             # the eager (NumPy) path
    assert want[:, 3].max() >= 2
    for k in (S // 3, 0, -1):
        tf, ref = dev.time_front(k), eager.time_front(k)
        kk = k % S
        assert tf.range_index == kk
        assert _same(tf.t, eager.ts[:, kk]) and _same(tf.z, eager.zs[:, kk]) and _same(tf.p, eager.ps[:, kk])
        assert _same(tf.range, ref.range) and _same(tf.thetas, eager.thetas)
        assert tf.turning_points.dtype == np.int64
        assert np.array_equal(tf.turning_points, fr.turning_points(eager.ps, [kk])[:, 0])
        assert _same(tf.ray_numbers, ref.ray_numbers)
        if kk != S - 1:
            assert tf.ray_ids is None
        else:
            assert np.array_equal(tf.ray_ids, eager.ray_ids)
    ids = dev.ray_ids
    assert ids.dtype.kind == "U" and np.array_equal(ids, eager.ray_ids)            # string for string
    assert np.array_equal(ids, fr.ray_id_strings(eager.ps, eager.thetas, eager.n_botts, eager.n_surfs))
    dev.compute_rayids()
    assert np.array_equal(dev.ray_ids, eager.ray_ids)
    _in_place(dev)
    if M >= 2:                                                                     # the tube products still run in place
        tl = pr.transmission_loss(dev, DEPTHS[::20], env, flatearth=flatearth, intensity=True)
        _in_place(dev)
        assert _same(tl, pr.transmission_loss(eager, DEPTHS[::20], env, flatearth=flatearth, intensity=True))
    assert np.array_equal(dev.turning_points(cols), want)                          # and again: the same arrays
    _in_place(dev)


@pytest.mark.parametrize("which", ["munk", "sloping"])
def test_device_resident_fans_in_place_in_both_layouts(pr_any, which):
    """rows on the LDS-table Munk environment, sample-blocked on the HBM-table sloping one"""
    env = munk_env(pr_any) if which == "munk" else sloping_env(pr_any)
    dev, eager = _shoot(pr_any, env, True), _shoot(pr_any, env, False)
    assert dev._dev._env.blocked_layout == (which == "sloping")
    assert ((eager.n_botts + eager.n_surfs) > 0).sum() > 5 and ((eager.n_botts + eager.n_surfs) == 0).sum() > 5
    _check_device_fan(pr_any, dev, eager, env)


def test_dropped_rays_are_skipped_through_the_keep_list(pr_any):
    env = sloping_env_shallow_table(pr_any)
    dev, eager = _shoot(pr_any, env, True), _shoot(pr_any, env, False)
    assert 0 < len(eager) < 300 and dev._dev.N == 300 and dev._dev.M == len(eager)
    _check_device_fan(pr_any, dev, eager, env)


def test_backwards_fan(pr_any):
    env = munk_env(pr_any)
    kw = dict(src=(900.0, 150e3), x1=40e3, S=111, n=90, amax=12.0)
    dev, eager = _shoot(pr_any, env, True, **kw), _shoot(pr_any, env, False, **kw)
    _check_device_fan(pr_any, dev, eager, env)


def test_default_flat_earth_environment(pr_any):
    env = pr_any.OceanEnvironment2D()
    kw = dict(x1=90e3, S=181, n=200, flatearth=True, amax=12.0)
    dev, eager = _shoot(pr_any, env, True, **kw), _shoot(pr_any, env, False, **kw)
    _check_device_fan(pr_any, dev, eager, env, flatearth=True)


def test_plot_time_front_of_a_device_fan_fetches_nothing(pr_any):
    plt = pytest.importorskip("matplotlib.pyplot")
    import matplotlib
    matplotlib.use("Agg", force=True)
    env = munk_env(pr_any)
    dev, eager = _shoot(pr_any, env, True, n=100), _shoot(pr_any, env, False, n=100)
    assert len(dev.time_front(77)) == len(eager)
    for kw in (dict(range_idx=77), dict(range_idx=-1, ray_id=True)):
        plt.figure()
        dev.plot_time_front(**kw)
        xy = plt.gca().collections[0].get_offsets()
        k = kw["range_idx"]
        assert _same(np.asarray(xy[:, 0]), eager.ts[:, k]) and _same(np.asarray(xy[:, 1]), eager.zs[:, k])
        plt.close("all")
    _in_place(dev)


@pytest.mark.parametrize("resident", [True, False])
def test_arrivals_carry_the_edge_rays_counts(pr_any, resident):
    env = munk_env(pr_any)
    fan, eager = _shoot(pr_any, env, resident), _shoot(pr_any, env, False)
    cols = [120, 200]
    arr = pr_any.arrivals(fan, DEPTHS[::10], env, flatearth=False, range_indices=cols)
    if resident:
        _in_place(fan)
    assert len(arr) > 100
    want = fr.turning_points(eager.ps, cols)
    n = len(cols)
    slot = np.repeat(np.arange(len(arr.offsets) - 1), np.diff(arr.offsets)) % n
    tp = np.stack([want[arr.tube, slot], want[arr.tube + 1, slot]], axis=1)
    assert arr.turning_points.dtype == np.int64 and np.array_equal(arr.turning_points, tp)
    differ = tp[:, 0] != tp[:, 1]
    assert differ.any() and (~differ).any()
    assert np.array_equal(np.isnan(arr.ray_number), differ)
    assert np.array_equal(arr.ray_number[~differ], (tp[:, 0] * np.sign(arr.launch_angle))[~differ])
    for j, c in ((3, 0), (30, 1)):
        sl = slice(int(arr.offsets[j * n + c]), int(arr.offsets[j * n + c + 1]))
        assert np.array_equal(arr.turning_points[sl, 0], want[arr.at(j, c)["tube"], c])


# ---- the error paths: < 0, a message, nothing launched ------------------------------------------------------------------

def _refused(call, text):
    from pygenray_amd import _lib
    with pytest.raises(_lib.PgrError) as e:
        call()
    assert text in str(e.value), str(e.value)


def test_the_buffer_entry_refuses_bad_arguments(pr_any):
    import torch
    from pygenray_amd import _lib
    dev = torch.device("cuda", 0)
    M, S = 10, 6
    rows = torch.zeros((S, M), dtype=torch.float64, device=dev)
    out = torch.full((3 * M,), MARK_F, dtype=torch.float64, device=dev)
    turns = torch.full((3 * M,), MARK_I, dtype=torch.int32, device=dev)
    r, o, t = rows.data_ptr(), out.data_ptr(), turns.data_ptr()
    f = lambda *a: (lambda: _lib.time_front_device(0, *a))      # noqa: E731
    _refused(f(r, r, r, M, S, None, o, o, o, t), "null cols")
    _refused(f(r, r, r, M, S, [0, 6, 1], o, o, o, t), "column")
    _refused(f(r, r, r, M, S, [0, -1, 1], o, o, o, t), "column")
    _refused(f(r, r, r, M, S, [], o, o, o, t), "n_cols")
    _refused(f(r, r, r, M, S, [0] * 65536, o, o, o, t), "n_cols")
    _refused(f(r, r, r, M, S, [0, 1, 2], 0, 0, 0, 0), "every output is NULL")
    _refused(f(r, r, r, 0, S, [0, 1, 2], o, o, o, t), "at least one ray")
    _refused(f(r, r, r, M, 0, [0], o, o, o, t), "n_samples")
    _refused(f(0, r, r, M, S, [0, 1, 2], o, 0, 0, 0), "input is NULL")
    _refused(f(r, 0, r, M, S, [0, 1, 2], 0, o, 0, 0), "input is NULL")
    _refused(f(r, r, 0, M, S, [0, 1, 2], 0, 0, o, 0), "input is NULL")
    _refused(f(r, r, 0, M, S, [0, 1, 2], 0, 0, 0, t), "input is NULL")
    torch.cuda.synchronize()
    assert (out == MARK_F).all() and (turns == MARK_I).all()     # nothing was launched


def test_the_fan_entry_refuses_bad_arguments(pr_any):
    import torch
    from pygenray_amd import _lib
    env = munk_env(pr_any)
    fan = _shoot(pr_any, env, True, n=80, S=50)
    h, M = fan._dev, len(fan)
    dev = torch.device("cuda", h._env.device)
    out = torch.full((3 * M,), MARK_F, dtype=torch.float64, device=dev)
    turns = torch.full((3 * M,), MARK_I, dtype=torch.int32, device=dev)
    o, t = out.data_ptr(), turns.data_ptr()
    _refused(lambda: h.time_front(None, o, o, o, t), "null cols")
    _refused(lambda: h.time_front([0, 50], o, o, o, t), "column")
    _refused(lambda: h.time_front([-1], o, o, o, t), "column")
    _refused(lambda: h.time_front([], o, o, o, t), "n_cols")
    _refused(lambda: h.time_front([0, 1, 2], 0, 0, 0, 0), "every output is NULL")
    # a fan launched without trajectories
    e = h._env
    bare = _lib.FanHandle(e, 0.0, 100e3, 0, ode_angles_deg=np.linspace(-5, 5, 70), source_depth=1000.0, c_source=1500.0)
    bare.wait()
    _refused(lambda: bare.time_front([0], o, o, o, t), "without trajectories")
    bare.close()
    # a fan none of whose rays survive: M == 0
    none = _lib.FanHandle(e, 0.0, 100e3, 11, y0=np.full((70, 3), np.nan), skip_nan=True)
    assert none.wait() == (70, 0)
    _refused(lambda: none.time_front([0], o, o, o, t), "at least one ray")
    none.close()
    torch.cuda.synchronize()
    assert (out == MARK_F).all() and (turns == MARK_I).all()     # nothing was launched
    assert np.array_equal(fan.turning_points([0])[:, 0], np.zeros(M, dtype=np.int64))     # the handle still works
