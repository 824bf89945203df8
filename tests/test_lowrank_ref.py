"""CPU: the checker of the direct block-kernel tests (tests/lowrank_ref.py) checks itself -- a plain fp64 evaluation of the same operations (numpy: BLAS order, fused
or not) lies within the bound, and a reference that is wrong in one place only (one row of L dropped, the chunks of a block vector shifted by one) does not."""
import numpy as np
import pytest

from tests import lowrank_ref as lr

SHAPES = [(1, 1, 1, 4), (65, 17, 5, 4), (1000, 50, 17, 4), (257, 300, 4, 1)]


def _fp64(op, d, mode=0):
    L, W, M, X, x2 = d["L"], d["W"], d["M"], d["X"], d["x2"]
    n, k = L.shape
    ncol, _, nc = X.shape
    cols = lambda B: np.transpose(B, (1, 0, 2)).reshape(B.shape[1], -1)
    blk = lambda A: np.transpose(A.reshape(A.shape[0], ncol, nc), (1, 0, 2))
    if op == "gram":
        return ((L * W[:, None]).T @ L)[np.tril_indices(k)]
    if op == "ltwx":
        return blk(M @ (L.T @ (W[:, None] * cols(X))))
    a, x, w = L @ cols(x2), cols(X), W[:, None]
    return blk([w * x - w * a, x - a, a + np.sqrt(1.0 / w) * x, -w * a, x + w * a][mode])


def test_long_double_is_wider_than_double():
    assert lr.long_double_is_wider()


@pytest.mark.parametrize("n,k,ncol,nc", SHAPES)
def test_plain_fp64_evaluation_is_within_the_bound(n, k, ncol, nc):
    d = lr.make_inputs(n, k, ncol, nc, seed=n + k)
    lr.check(_fp64("gram", d), *lr.ref_gram(d["L"], d["W"]), what="gram")
    lr.check(_fp64("ltwx", d), *lr.ref_ltwx(d["L"], d["W"], d["M"], d["X"]), what="ltwx")
    for mode in range(5):
        lr.check(_fp64("combine", d, mode), *lr.ref_combine(d["L"], d["W"], d["X"], d["x2"], mode), what="combine %d" % mode)


@pytest.mark.parametrize("n,k,ncol,nc", SHAPES[1:])
def test_a_reference_with_one_row_of_L_dropped_is_beyond_the_bound(n, k, ncol, nc):
    d = lr.make_inputs(n, k, ncol, nc, seed=n + k)
    Lw = d["L"].copy(); Lw[n // 2] = 0.0
    with pytest.raises(AssertionError, match="the bound"):
        lr.check(_fp64("gram", d), *lr.ref_gram(Lw, d["W"]), what="gram")
    with pytest.raises(AssertionError, match="the bound"):
        lr.check(_fp64("ltwx", d), *lr.ref_ltwx(Lw, d["W"], d["M"], d["X"]), what="ltwx")
    for mode in range(5):
        with pytest.raises(AssertionError, match="the bound"):
            lr.check(_fp64("combine", d, mode), *lr.ref_combine(Lw, d["W"], d["X"], d["x2"], mode), what="combine %d" % mode)


@pytest.mark.parametrize("n,k,ncol,nc", [(65, 17, 5, 4), (1000, 50, 17, 4), (257, 300, 4, 1)])
def test_a_reference_with_the_chunks_shifted_by_one_is_beyond_the_bound(n, k, ncol, nc):
    d = lr.make_inputs(n, k, ncol, nc, seed=n + k)
    d["X"][np.isnan(d["X"])] = 1.0          # (the NaN column would move with its chunk and fail the NaN test first)
    Xs = np.roll(d["X"], 1, axis=0); x2s = np.roll(d["x2"], 1, axis=0)
    with pytest.raises(AssertionError, match="the bound"):
        lr.check(_fp64("ltwx", d), *lr.ref_ltwx(d["L"], d["W"], d["M"], Xs), what="ltwx")
    for mode in range(5):
        with pytest.raises(AssertionError, match="the bound"):
            lr.check(_fp64("combine", d, mode), *lr.ref_combine(d["L"], d["W"], d["X"], x2s, mode), what="combine %d" % mode)


def test_a_nan_in_another_place_than_the_reference_has_it_fails():
    d = lr.make_inputs(65, 17, 5, 4, seed=1)
    ref, bound = lr.ref_ltwx(d["L"], d["W"], d["M"], d["X"])
    dev = _fp64("ltwx", d)
    dev[0, 0, 0] = np.nan
    with pytest.raises(AssertionError, match="NaN"):
        lr.check(dev, ref, bound)
