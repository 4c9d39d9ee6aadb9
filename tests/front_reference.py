"""NumPy restatement of the time-front quantities, independent of the package: the reference's own
one-line ray-identifier count (REF/ray_objects.py:142) applied to the path up to each requested column, and the column
gather.  Also the synthetic slowness blocks both test files feed it.  Not a test module itself."""
import numpy as np


def turning_points(ps, cols):
    """ps (M, S), cols a sequence of column indices 0 .. S - 1 -> (M, len(cols)) int64"""
    ps = np.asarray(ps)
    return np.stack([np.sum(np.diff(np.sign(ps[:, :int(c) + 1]), axis=1) != 0, axis=1) for c in cols], axis=1).astype(np.int64)


def gather(a, cols):
    """a (M, S) -> (M, len(cols)): the columns as they are"""
    return np.asarray(a)[:, np.asarray(cols, dtype=np.int64)]


def ray_id_strings(ps, thetas, n_botts, n_surfs):
    """the reference's ray ids (REF/ray_objects.py:138-155) of whole rays"""
    num = turning_points(ps, [np.shape(ps)[1] - 1])[:, 0] * np.sign(thetas)
    return np.array([f"{v}" + ("" if (b == 0 and s == 0) else "b") for v, b, s in zip(num, n_botts, n_surfs)], dtype=str)


def synthetic(M, S, seed):
    """T, z, p (M, S): p with sign flips at a rate drawn per ray (none ... every other sample), exact zeros of both signs,
    NaN runs, a NaN in the first and in the last sample, a ray of all zeros and one of all -0.0; T and z random with a few
    NaNs of their own."""
    rng = np.random.default_rng(seed)
    rate = rng.uniform(0.0, 0.5, M) * (rng.random(M) < 0.8)
    flips = rng.random((M, S)) < rate[:, None]
    p = np.where(np.cumsum(flips, axis=1) % 2 == 0, 1.0, -1.0) * rng.uniform(1e-7, 6.6e-4, (M, S))
    zero = rng.random((M, S)) < 0.06
    p[zero] = np.where(rng.random(int(zero.sum())) < 0.5, 0.0, -0.0)
    for m in rng.choice(M, max(1, M // 6), replace=False):
        a = int(rng.integers(0, S))
        p[m, a:a + int(rng.integers(1, 7))] = np.nan
    p[0, 0] = np.nan
    p[M - 1, S - 1] = np.nan
    if M >= 4:
        p[2, :] = 0.0
        p[3, :] = -0.0
    T = rng.uniform(0.0, 700.0, (M, S))
    z = -rng.uniform(0.0, 5000.0, (M, S))
    T[rng.random((M, S)) < 0.01] = np.nan
    z[rng.random((M, S)) < 0.01] = np.nan
    return T, z, p


def column_cases(S, seed):
    """the column lists of the kernel tests: the first, the last, all, a shuffled list with repeats, and one that makes
    segments of length 1 and of several hundred (where S allows)"""
    rng = np.random.default_rng(seed)
    far = sorted({min(v, S - 1) for v in (1, 2, 3, 4, 350, 351, 352, 990, S - 1)})
    return [[0], [S - 1], list(range(S)), [int(v) for v in rng.integers(0, S, 2 * min(S, 40) + 3)], far]
