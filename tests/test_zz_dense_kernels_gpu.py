"""GPU (MI355X): the dense path of gpboost_amd/csrc/dense_kernels.hip pinned element by element against the a-priori bounds of tests/dense_ref.py (derived there; fp64
LAPACK is held to the same bounds in tests/test_dense_ref.py).

Factor and Schur complement through gpb_hip_dense_cholesky_check, cases (ld, ncols, lookahead) of dense_ref.FACTOR_CASES: every update form of launch_dense_cholesky
(64 x 64 tiles, syrk_mfma_db_kernel<16> with K = 512 and K = 64, from 128- and 64-aligned origins, with and without the second stream).  Look-ahead on / off pairs:
  (1088, 1088): every update takes syrk_mfma_small_kernel either way (25 tiles without look-ahead; strip 5 x 4 and rest 1 x 1 with it) -> bit-identical, asserted
  (3200, 576):  without look-ahead both wide updates take syrk_mfma_db_kernel<16> (441 tiles); with it the first strip (21 x 4 = 84 tiles) takes
                syrk_mfma_small_kernel -> different kernels, each result is held to the bound on its own
gpb_hip_dense_spd_solve (solve, inverse, both), the failure path (info, "not positive definite", and that the next call is clean), and the exact-GP entries
(nll_terms, grad_terms, psi_inv_diag, predict) against the long-double reference at the project's 1e-8 contract."""
import functools

import numpy as np
import pytest

from tests import dense_ref as dr

pytestmark = pytest.mark.gpu

RTOL = 1e-8          # BASELINE.json north_star / RTOL of tests/test_vecchia_gpu.py


@pytest.fixture(scope="module")
def shim(lib_built):
    import gpboost_amd
    assert gpboost_amd.device_count() > 0, "no GPU visible: the -m gpu tests must run on the MI355X box"
    from gpboost_amd import shim
    return shim


@functools.lru_cache(maxsize=2)
def _factor_input(kind, ld, ncols):
    M = dr.factor_input(kind, ld, ncols)
    M.setflags(write=False)
    return M


_RESULTS = {}        # (kind, ld, ncols, lookahead) -> lower triangle of the device result, for the look-ahead pairs


def _factor_params():
    return [pytest.param(ld, nc, la, kind, id="ld%d_nc%d_la%d_%s" % (ld, nc, la, kind)) for ld, nc, la in dr.FACTOR_CASES for kind in dr.factor_kinds(ld, nc)]


@pytest.mark.parametrize("ld,ncols,lookahead,kind", _factor_params())
def test_factor_and_schur_complement(shim, ld, ncols, lookahead, kind):
    assert dr.long_double_is_wider()
    M = _factor_input(kind, ld, ncols)
    out, info = shim.dense_cholesky_check(M, ncols, lookahead)
    assert info == 0
    iu = np.triu_indices(ld, 1)
    assert np.array_equal(out[iu].view(np.uint64), M[iu].view(np.uint64)), "the strict upper triangle was written"
    low = np.tril(out)
    viol, worst = dr.factor_violations(M, out, ncols, rows=dr.sample_rows(ld, ncols, bool(lookahead)), want_worst=True)
    print("factor ld=%d ncols=%d lookahead=%d %s: largest r / bound = %.4f" % (ld, ncols, lookahead, kind, worst))
    assert viol == [], (len(viol), viol[:8])
    # the lower triangle alone is significant: NaN above the diagonal changes nothing
    Mn = M.copy(); Mn[iu] = np.nan
    out_n, info_n = shim.dense_cholesky_check(Mn, ncols, lookahead)
    assert info_n == 0 and np.array_equal(np.tril(out_n).view(np.uint64), low.view(np.uint64)), "the result depends on the strict upper triangle"
    del Mn, out_n
    # run to run
    out_2, info_2 = shim.dense_cholesky_check(M, ncols, lookahead)
    assert info_2 == 0 and np.array_equal(out_2.view(np.uint64), out.view(np.uint64)), "two runs differ"
    if (ld, ncols) == (1088, 1088):       # the pair whose updates take the same kernel with and without look-ahead (module docstring)
        other = _RESULTS.get((kind, ld, ncols, 1 - lookahead))
        if other is None:
            _RESULTS[(kind, ld, ncols, lookahead)] = low
        else:
            assert np.array_equal(other.view(np.uint64), low.view(np.uint64)), "look-ahead on / off differ although every update takes the same kernel"


def _solve_params():
    return [pytest.param(n, kind, id="n%d_%s" % (n, kind)) for n in dr.SOLVE_SIZES for kind in dr.solve_kinds(n)]


@pytest.mark.parametrize("n,kind", _solve_params())
def test_dense_spd_solve(shim, n, kind):
    M, b, v, cols = dr.solve_inputs(kind, n)
    np_ = dr.pad64(n)
    kap = dr.kappa_inf(M)
    x, none = shim.dense_spd_solve(M, rhs=b)
    assert none is None
    be = dr.solve_backward_error(M, x, b)
    none, X = shim.dense_spd_solve(M, sub0=0)
    assert none is None and X.shape == (n, n)
    res = dr.inverse_residual(M, X, cols)
    print("spd_solve n=%d %s: backward error / bound = %.4f, inverse residual / bound = %.4f (kappa_inf = %.3g)" %
          (n, kind, be / dr.solve_bound(np_), res / dr.inverse_bound(np_, kap), kap))
    assert be <= dr.solve_bound(np_)
    assert res <= dr.inverse_bound(np_, kap)
    assert np.array_equal(X, X.T), "the returned inverse is not symmetric"
    sub0 = max(0, n - 37)
    x2, Xs = shim.dense_spd_solve(M, rhs=b, sub0=sub0)
    assert dr.solve_backward_error(M, x2, b) <= dr.solve_bound(np_)
    assert Xs.shape == (n - sub0, n - sub0) and np.array_equal(Xs.view(np.uint64), np.ascontiguousarray(X[sub0:, sub0:]).view(np.uint64)), "the sub-block differs from the full inverse"


def _good_factor_within_bound(shim, ld):
    M = _factor_input("well", ld, ld)
    out, info = shim.dense_cholesky_check(M, ld, 0)
    assert info == 0 and dr.factor_violations(M, out, ld, rows=dr.sample_rows(ld, ld)) == []


@pytest.mark.parametrize("p", [5, 600, 703, "nan"])
def test_failure_path_of_the_factorisation(shim, p):
    ld = 704
    A = dr.spd_matrix("well", ld, seed=21)
    M = dr.break_pivot(A, 5, np.nan) if p == "nan" else dr.break_pivot(A, p)
    out, info = shim.dense_cholesky_check(M, ld, 0)
    assert info != 0
    first = 5 if p == "nan" else p
    if first >= 64:            # the block columns before the bad pivot's 64-block are untouched by it
        blk = first // 64 * 64
        assert dr.factor_violations(A, out, ld, rows=np.arange(blk)) == []
    _good_factor_within_bound(shim, 128)       # the next call in the same process starts from a cleared info word


@pytest.mark.parametrize("p", [5, 600, 649, "nan"])
def test_failure_path_of_dense_spd_solve(shim, p):
    import gpboost_amd
    n = 650                    # np = 704: the identity padding comes after the bad pivot and must not hide it
    A = dr.spd_matrix("well", n, seed=22)
    M = dr.break_pivot(A, 5, np.nan) if p == "nan" else dr.break_pivot(A, p)
    b = A @ np.ones(n)
    with pytest.raises(gpboost_amd.GPBoostError, match="not positive definite"):
        shim.dense_spd_solve(M, rhs=b)
    with pytest.raises(gpboost_amd.GPBoostError, match="not positive definite"):
        shim.dense_spd_solve(M, sub0=n - 3)
    x, _ = shim.dense_spd_solve(A, rhs=b)
    assert dr.solve_backward_error(A, x, b) <= dr.solve_bound(dr.pad64(n))


def _close(dev, ref, what):
    """|dev - ref| <= RTOL max(|ref|, max|ref|) per entry; -> the largest |dev - ref| / |ref| met, for the record."""
    ref = np.atleast_1d(np.asarray(ref)); dev = np.atleast_1d(np.asarray(dev, dtype=np.float64)).astype(dr.LD)
    assert dev.shape == ref.shape, what
    err = np.abs(dev - ref)
    tol = RTOL * np.maximum(np.abs(ref), np.max(np.abs(ref)))
    scale = np.maximum(np.abs(ref), np.max(np.abs(ref)))
    worst = float(np.max(err / np.where(scale > 0, scale, 1)))
    print("%s: largest |device - reference| / max(|reference|, max|reference|) = %.3g" % (what, worst))
    assert np.all(err <= tol), (what, worst)
    return worst


@pytest.mark.parametrize("n,d,ct", dr.EXACT_CASES)
def test_exact_gp_entries_against_long_double(shim, n, d, ct):
    coords, y, pred, ref = dr.exact_case(n, d, ct)
    var, a = dr.EXACT_VAR, dr.exact_range_par(ct, d, n)
    tag = "exact n=%d d=%d cov=%d " % (n, d, ct)
    st = shim.ExactState(coords)
    try:
        st.set_y(y)
        out, ya, _ = st.nll_terms(ct, var, a, want_yaux=True)
        for k, name in enumerate(("y'Psi^-1 y", "log|Psi|")):
            _close(out[k], ref["nll2"][k], tag + "nll_terms " + name)
        _close(ya, ref["y_aux"], tag + "y_aux")
        g = st.grad_terms(ct, var, a)
        assert g[2] == 0.0
        for k in (0, 1, 3, 4, 5, 6):
            _close(g[k], ref["grad7"][k], tag + "grad_terms[%d]" % k)
        _close(st.psi_inv_diag(ct, var, a), ref["psi_inv_diag"], tag + "psi_inv_diag")
        mean, q = st.predict(pred, True, ct, var, a)
        _close(mean, ref["pred_mean"], tag + "predict mean")
        _close(q, ref["pred_q"], tag + "predict q")
        mean_only, none = st.predict(pred, False, ct, var, a)
        assert none is None and np.array_equal(mean_only, mean)
    finally:
        st.close()
