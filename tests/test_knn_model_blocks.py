"""tests/knn_model.py against itself, no GPU: the array form of the correctly rounded fma is the scalar one element by element,
and a leave-one-out search or plan taken in row blocks (`rows=`) is the one taken at once."""
import numpy as np
import pytest

from tests import knn_model as km


def test_fma_array_is_the_scalar_fma():
    rng = np.random.default_rng(3)
    n = 20000
    t = rng.standard_normal(n) ** 2 * 10.0 ** rng.integers(-8, 8, size=n)
    acc = rng.standard_normal(n) ** 2 * 10.0 ** rng.integers(-8, 8, size=n)
    t[:50], acc[50:100] = 0.0, 0.0
    t[100:110], acc[100:110] = 1.0 + 2.0 ** -52, 2.0 ** -53  # the exact sums end in ties and near ties
    for s in (0.3, 1.0, 2.9999999999999996, float(rng.uniform(0.3, 3.0))):
        want = km._fma(t, s, acc).astype(np.float64)
        assert np.array_equal(km.fma_array(t, s, acc), want)
    assert km.fma_array(np.array([1.0 + 2.0 ** -52]), 1.0 + 2.0 ** -52, np.array([2.0 ** -105]))[0] == \
        km.fma_fraction(1.0 + 2.0 ** -52, 1.0 + 2.0 ** -52, 2.0 ** -105)


@pytest.mark.parametrize("scale,circ", [(None, ()), ((0.7, 2.3), ()), (None, (1,))])
def test_row_blocks_give_the_whole_search(scale, circ):
    rng = np.random.default_rng(11)
    N, k = 641, 5  # (N - 1) % 128 == 0: the last leaf is alone in its chunk
    pts = rng.standard_normal((N, 2))
    pts[N // 2:] += 3.0
    orig = rng.permutation(N) + 1
    whole_d2, whole_idx = km.knn(pts, orig, pts, k, loo=True, scale=scale, circ=circ)
    whole = km.plan(pts, orig, pts, k, loo=True, scale=scale, circ=circ)
    d2s, idxs, cstar, visited, total = [], [], [], 0, 0
    for r in range(0, N, 256):
        rows = slice(r, min(N, r + 256))
        d2, idx = km.knn(pts, orig, pts[rows], k, loo=True, scale=scale, circ=circ, rows=rows)
        pl = km.plan(pts, orig, pts[rows], k, loo=True, scale=scale, circ=circ, rows=rows)
        d2s.append(d2)
        idxs.append(idx)
        cstar.append(pl["cstar"])
        visited, total = visited + pl["stats"][0], total + pl["stats"][1]
    assert np.array_equal(np.concatenate(d2s), whole_d2) and np.array_equal(np.concatenate(idxs), whole_idx)
    assert np.array_equal(np.concatenate(cstar), whole["cstar"]) and (visited, total) == whole["stats"]
    assert whole["cstar"][N - 1] != N // 128  # the lone leaf's own chunk does not count for it
