"""CPU: the model of the sparse Vecchia-Laplace kernels (tests/laplace_sparse_ref.py) checked on its own -- the long-double operations against exact rationals, the
recipes against the schedule branches they are meant to reach, the fp64 restatement of the kernels' operation order against every bound (its largest ratio per class is
the non-vacuity figure the device is compared with, docs/HISTORY.md), and five mutants of the restatement, each of which has to leave a bound."""
from fractions import Fraction

import numpy as np
import pytest

from tests import laplace_sparse_ref as R

LD = R.LD
_REL = {"==": lambda a, b: a == b, ">": lambda a, b: a > b, ">=": lambda a, b: a >= b}
WORST = {}


def _note(cls, q, where):
    q = float(np.max(q))
    if q >= WORST.get(cls, (-1.0, ""))[0]:
        WORST[cls] = (q, where)


def _fr(a):
    return [[Fraction(float(v)) for v in row] for row in np.atleast_2d(a)]


def test_long_double_operations_against_exact_rationals():
    g = R.graph("tiny")
    assert g.n == 40
    x = g.operand(1)[:, 0]
    A, nn, n = g.A, g.nn, g.n
    Af, xf, Df, Wf = _fr(A), [Fraction(float(v)) for v in x], [Fraction(float(v)) for v in g.D], [Fraction(float(v)) for v in g.W]
    Bx = [xf[i] - sum(Af[i][j] * xf[nn[i, j]] for j in range(g.m) if nn[i, j] >= 0) for i in range(n)]
    Btx = list(xf)
    for i in range(n):
        for j in range(g.m):
            if nn[i, j] >= 0:
                Btx[nn[i, j]] -= Af[i][j] * xf[i]
    th = [Bx[i] / Df[i] for i in range(n)]
    sf = [Fraction(float(v)) for v in g.scale]
    z = [None] * n
    for i in range(n):
        z[i] = sf[i] * xf[i] + sum(Af[i][j] * z[nn[i, j]] for j in range(g.m) if nn[i, j] >= 0)
    t = list(xf)
    for i in range(n - 1, -1, -1):       # B' t = x: row i is final once every later row has been spread
        for j in range(g.m):
            if nn[i, j] >= 0:
                t[nn[i, j]] += Af[i][j] * t[i]
    fw, bw = g.sched(False), g.sched(True)
    X = x[:, None]

    def close(res, exact, solve=False):
        ex = np.array([LD(e.numerator) / LD(e.denominator) for e in exact])
        got, sc = (res, 100 * (1 + np.max(np.abs(ex)))) if solve else (res[0], res[1][:, 0] / R.U)      # products: relative to the sum of the terms' magnitudes
        assert np.all(np.abs(got[:, 0] - ex) <= LD(2) ** -58 * sc), float(np.max(np.abs(got[:, 0] - ex) / sc))

    close(R.product_ref(fw, A, X, 0), Bx)
    close(R.product_ref(bw, A, X, 2), Btx)
    v1 = R.product_ref(fw, A, X, 1, D=g.D)
    close(v1, th)
    th64 = v1[0].astype(np.float64)          # the second half works on the first half's fp64 result
    ap = [Fraction(float(v)) for v in th64[:, 0]]
    for i in range(n):
        for j in range(g.m):
            if nn[i, j] >= 0:
                ap[nn[i, j]] -= Af[i][j] * Fraction(float(th64[i, 0]))
    ap = [ap[i] + Wf[i] * xf[i] for i in range(n)]
    close(R.product_ref(bw, A, th64, 2, W=g.W, H=X), ap)
    close(R.solve_exact(fw, A, X, g.scale), z, solve=True)
    close(R.solve_exact(bw, A, X, None), t, solve=True)
    close(R.product_ref(fw, g.A2, X, 3), [sum(Fraction(float(g.A2[i, j])) * xf[nn[i, j]] for j in range(g.m) if nn[i, j] >= 0) for i in range(n)])
    # the exact solutions have residual 0 and pass their own check
    q, _ = R.solve_check(fw, A, X, g.scale, R.solve_exact(fw, A, X, g.scale).astype(np.float64), 1)
    assert np.all(q <= 1.0)


def test_exact_fma():
    rng = np.random.default_rng(3)
    for _ in range(2000):
        a, b, c = (float(v) for v in rng.standard_normal(3) * 10.0 ** rng.integers(-8, 8, size=3))
        assert R.fma(a, b, c) == float(Fraction(a) * Fraction(b) + Fraction(c))
    assert R.fma(0.0, 5.0, 1.5) == 1.5 and R.fma(2.0, 3.0, 0.0) == 6.0 and R.fma(1.0 + 2.0 ** -52, 1.0 - 2.0 ** -52, -1.0) == -2.0 ** -104


@pytest.mark.parametrize("name", R.GRAPHS)
def test_recipe_reaches_its_branches(name):
    g = R.graph(name)
    for solve, field, rel, want in R.REACHES[name]:
        s = g.sched(solve == "bwd")
        got = dict(s.info, **s.extra)[field]
        assert _REL[rel](got, want), (name, solve, field, rel, want, got)
    # every row sums to at most 0.9 in absolute value: ||B^-1||_inf <= 10
    assert np.all(np.abs(g.A.astype(LD)).sum(axis=1) <= LD("0.9"))
    assert np.all(g.A[g.nn < 0] == 0) and np.all(g.D > 0) and np.all(g.W > 0)


def test_morton_rank_of_the_handles_coordinates_is_sigma():
    """morton_order (gpb_laplace.inc) in one dimension: key = floor((x - min) (2^21 - 1) / (max - min)), ties by index: strictly increasing in x for distinct integers below 2^21"""
    g = R.graph("hub-m4")
    x = g.coords[:, 0]
    key = ((x - x.min()) * (float((1 << 21) - 1) / (x.max() - x.min()))).astype(np.uint64)
    assert np.array_equal(np.argsort(np.argsort(key, kind="stable"), kind="stable"), g.sigma) and np.unique(key).size == g.n


def _solve_classes(g, backward, cols, tag):
    s = g.sched(backward)
    if s.K > 64:
        return None
    num = g.operand(cols, seed=3 if backward else 4)
    den = None if backward else g.scale
    x = R.solve_fp64(s, g.A, num, den)
    q, dense = R.solve_check(s, g.A, num, den, x, 1)
    if np.any(~dense):
        _note("solve sparse rows", q[~dense], "%s %s" % (g.name, tag))
    if np.any(dense):
        _note("solve dense rows", q[dense], "%s %s" % (g.name, tag))
    return q


@pytest.mark.parametrize("name", R.GRAPHS)
def test_fp64_restatement_lies_inside_every_bound(name):
    g = R.graph(name)
    fw, bw = g.sched(False), g.sched(True)
    for backward in (False, True):
        q = _solve_classes(g, backward, 1, "bwd" if backward else "fwd")
        assert q is None or np.all(q <= 1.0), (name, backward, float(q.max()))
    X = g.operand(1, seed=5)
    for cls, s, A, mode, kw in (("B", fw, g.A, 0, {}), ("Bt", bw, g.A, 2, {}), ("apply first half", fw, g.A, 1, {"D": g.D}), ("mul_fwd", fw, g.A2, 3, {}),
                                ("mul_bwd", bw, g.A2, 3, {})):
        got = R.product_fp64(s, A, X, mode, **kw)
        val, bound = R.product_ref(s, A, X, mode, **kw)
        q = R.ratio_of(got - val, bound)
        _note(cls, q, name)
        assert np.all(q <= 1.0), (name, cls, float(q.max()))
    th = R.product_fp64(fw, g.A, X, 1, D=g.D)
    got = R.product_fp64(bw, g.A, th, 2, W=g.W, H=X)
    val, bound = R.product_ref(bw, g.A, th, 2, W=g.W, H=X)
    q = R.ratio_of(got - val, bound)
    _note("apply second half", q, name)
    assert np.all(q <= 1.0), (name, float(q.max()))


MUTANT_CASES = {"drop_last_overflow": [("layers-m70", False)], "skip_continuation_slots": [("layers-m70", False)],
                "scale_at_vecchia_index": [("layers-m12", False)], "neighbour_chunk_column": [("layers-m12", False)],
                "same_level_read_early": [("layers-m12", False)]}


@pytest.mark.parametrize("mutant", R.MUTANTS)
def test_mutant_leaves_a_bound(mutant):
    worst = 0.0
    for name, backward in MUTANT_CASES[mutant]:
        g = R.graph(name)
        s = g.sched(backward)
        num = g.operand(2, seed=4)
        den = None if backward else g.scale
        x = R.solve_fp64(s, g.A, num, den, sigma=g.sigma, mutant=mutant)
        q, _ = R.solve_check(s, g.A, num, den, x, 1)
        worst = max(worst, float(q.max()))
    print("mutant %s: largest residual / bound %.3g" % (mutant, worst))
    assert worst > 1.0


def test_zz_report_cpu_ratios():
    """Not a check: the largest ratio of the fp64 restatement to each bound, per class (docs/HISTORY.md)."""
    for k, v in sorted(WORST.items()):
        print("fp64 restatement, %-20s largest error / bound %.4f  (%s)" % (k, v[0], v[1]))
