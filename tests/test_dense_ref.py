"""CPU: tests/dense_ref.py itself.  fp64 LAPACK and a numpy restatement of the blocked right-looking algorithm stay inside every a-priori bound on every generator at
every shape the GPU test (tests/test_zz_dense_kernels_gpu.py) uses; five mutants of the restatement are reported at the sampled rows by at least 1e3 times the bound;
the long-double exact-GP reference agrees with the oracle and none of its sums cancels by more than a factor 100, so that a relative tolerance on them means something.
Each test prints the largest ratio to its bound (pytest -s); docs/HISTORY.md records them."""
import numpy as np
import pytest

from tests import dense_ref as dr

FACTOR_SHAPES = sorted(set((ld, nc) for ld, nc, _ in dr.FACTOR_CASES))


def test_long_double_is_the_80_bit_type():
    assert dr.long_double_is_wider()
    assert dr.C_PIVOT == 11 and dr.C2_INVERSE >= 4.0 * (64 + dr.C_PIVOT) / 64


@pytest.mark.parametrize("ld,ncols", FACTOR_SHAPES)
def test_lapack_factor_is_inside_the_bound(ld, ncols):
    for kind in dr.factor_kinds(ld, ncols):
        M = dr.factor_input(kind, ld, ncols)
        out = dr.lapack_partial(M, ncols)
        viol, worst = dr.factor_violations(M, out, ncols, rows=dr.sample_rows(ld, ncols), want_worst=True)
        print("LAPACK factor ld=%d ncols=%d %s: largest r / bound = %.4f" % (ld, ncols, kind, worst))
        assert viol == [], viol[:5]
        assert np.array_equal(np.triu(out, 1), np.triu(M, 1))


@pytest.mark.parametrize("ld,ncols", [(128, 64), (576, 576), (1088, 1088), (1344, 704)])
def test_blocked_restatement_is_inside_the_bound(ld, ncols):
    for kind in dr.factor_kinds(ld, ncols):
        M = dr.factor_input(kind, ld, ncols)
        out = dr.blocked_cholesky(M, ncols)
        viol, worst = dr.factor_violations(M, out, ncols, rows=dr.sample_rows(ld, ncols), want_worst=True)
        print("blocked restatement ld=%d ncols=%d %s: largest r / bound = %.4f" % (ld, ncols, kind, worst))
        assert viol == [], viol[:5]
        ref = dr.lapack_partial(M, ncols)
        scale = np.abs(ref).max()
        assert np.allclose(out, ref, rtol=0, atol=(1e-4 if kind == "ill" else 1e-10) * scale)


@pytest.mark.parametrize("mutant", dr.MUTANTS)
@pytest.mark.parametrize("ld,ncols", [(1088, 1088), (1344, 704)])
def test_mutants_are_reported_at_the_sampled_rows(ld, ncols, mutant):
    rows = dr.sample_rows(ld, ncols)
    assert rows.size <= 56 and rows.size < ld
    for kind in ("well", "ill"):
        M = dr.factor_input(kind, ld, ncols)
        out = dr.blocked_cholesky(M, ncols, mutant=mutant)
        assert not np.array_equal(out, dr.blocked_cholesky(M, ncols))
        viol, worst = dr.factor_violations(M, out, ncols, rows=rows, want_worst=True)
        print("mutant %s ld=%d ncols=%d %s: %d entries, largest r / bound = %.3g" % (mutant, ld, ncols, kind, len(viol), worst))
        assert viol and worst >= 1e3, (mutant, kind, worst)


def test_sample_rows_cover_the_block_edges():
    rows = set(dr.sample_rows(3200, 576, lookahead=True).tolist())
    for r in (0, 63, 448, 511, 512, 575, 576, 639, 1024, 1087, 1088, 1151, 3136, 3199):     # 512 edge, ncols = Jend = 576, Send = 1024 and 1088, the last block
        assert r in rows, r
    assert len(rows) <= 56
    assert dr.sample_rows(640, 640).size == 640


@pytest.mark.parametrize("n", dr.SOLVE_SIZES)
def test_lapack_solve_and_inverse_are_inside_the_bounds(n):
    for kind in dr.solve_kinds(n):
        M, b, v, cols = dr.solve_inputs(kind, n)
        np_ = dr.pad64(n)
        x = np.linalg.solve(M, b)
        be = dr.solve_backward_error(M, x, b)
        X = np.linalg.inv(M)
        res, kap = dr.inverse_residual(M, X, cols), dr.kappa_inf(M)
        print("LAPACK n=%d %s: solve backward error / bound = %.4f, inverse residual / bound = %.4f (kappa_inf = %.3g)" %
              (n, kind, be / dr.solve_bound(np_), res / dr.inverse_bound(np_, kap), kap))
        assert be <= dr.solve_bound(np_)
        assert res <= dr.inverse_bound(np_, kap)
        if kind == "ill" and n >= 65:
            assert kap > 1e6, "the ill-conditioned generator is not ill-conditioned"


def test_break_pivot_puts_the_first_bad_pivot_where_asked():
    A = dr.spd_matrix("well", 130, seed=3)
    for p in (5, 70, 129):
        M = dr.break_pivot(A, p)
        np.linalg.cholesky(M[:p, :p])
        with pytest.raises(np.linalg.LinAlgError):
            np.linalg.cholesky(M[:p + 1, :p + 1])


@pytest.mark.parametrize("n,d,ct", dr.EXACT_CASES)
def test_exact_reference_does_not_cancel_and_agrees_with_fp64(n, d, ct, orc):
    coords, y, pred, ref = dr.exact_case(n, d, ct)
    worst = max(ref["cancellation"].values())
    print("exact n=%d d=%d cov=%d: sum|terms| / |sum| = %s" % (n, d, ct, {k: round(v, 2) for k, v in ref["cancellation"].items()}))
    assert worst <= 100, ref["cancellation"]
    a = dr.exact_range_par(ct, d, n)
    o, yo = orc.exact_nll(coords, ct, np.array([0.1, dr.EXACT_VAR, a]), y, want_yaux=True)      # the oracle's parametrisation
    assert abs(o[0] - float(ref["nll2"][0])) <= 1e-9 * abs(o[0]) and abs(o[1] - float(ref["nll2"][1])) <= 1e-9 * max(1.0, abs(o[1]))
    assert np.allclose(yo, ref["y_aux"].astype(np.float64), rtol=0, atol=1e-9 * np.abs(yo).max())
    # gradient sums against central differences of the long-double value in log(var) and log(a): d/dlog(theta) of 1/2 (y' Psi^-1 y + log|Psi|) = g1 + g2
    if n in (64, 65):
        h = 1e-5
        for name, idx in (("var", 3), ("range", 5)):
            def val(f):
                r = dr.exact_reference(coords, y, ct, dr.EXACT_VAR * (f if name == "var" else 1.0), a * (f if name == "range" else 1.0))
                return 0.5 * (r["nll2"][0] + r["nll2"][1])
            fd = float((val(np.exp(h)) - val(np.exp(-h))) / (2 * h))
            g = float(ref["grad7"][idx] + ref["grad7"][idx + 1])
            assert abs(fd - g) <= 1e-7 * max(1.0, abs(g)), (name, fd, g)
    q = ref["pred_q"].astype(np.float64)
    assert np.allclose(q, q.T, rtol=0, atol=1e-15 * np.abs(q).max()) and np.all(np.diag(q) <= dr.EXACT_VAR * (1 + 1e-12))
