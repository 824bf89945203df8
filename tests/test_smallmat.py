"""CPU: gpboost_amd/csrc/gpb_smallmat.h against tests/smallmat_ref.py, bit for bit.  The header is compiled through tests/smallmat/smallmat_export.cpp with the
host flags of tests/mock_shim/Makefile (g++ -O2 -std=c++17 -ffp-contract=off) and loaded with ctypes.

Sizes k = 1, 2, 3, 7, 12; symmetric positive definite matrices with a condition number of about 1e6 (rounding shows in the first digits of the last place), one
indefinite matrix and one with a +inf diagonal (both must fail, at the reference's index), a leading dimension larger than k whose padding must stay untouched."""
import ctypes as C
import os
import subprocess

import numpy as np
import pytest

from tests import smallmat_ref as R

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
SIZES = [1, 2, 3, 7, 12]
PAD = -7.25e300


@pytest.fixture(scope="module")
def lib(tmp_path_factory):
    out = str(tmp_path_factory.mktemp("smallmat") / "libsmallmat_export_TEST_ONLY.so")
    subprocess.check_call(["g++", "-O2", "-std=c++17", "-ffp-contract=off", "-fPIC", "-shared", "-pthread", "-I" + os.path.join(ROOT, "gpboost_amd", "csrc"),
                           "-o", out, os.path.join(ROOT, "tests", "smallmat", "smallmat_export.cpp")])
    lib = C.CDLL(out)
    lib.sm_matern.restype = C.c_double
    lib.sm_matern.argtypes = [C.c_int, C.c_int, C.c_double, C.c_double]
    lib.sm_jitter_mult.restype = C.c_double
    return lib


def _p(a):
    return a.ctypes.data_as(C.POINTER(C.c_double))


def spd(k, seed=0):
    """symmetric positive definite, eigenvalues 1 .. 1e-6"""
    rng = np.random.default_rng(100 * k + seed)
    q, _ = np.linalg.qr(rng.standard_normal((k, k)))
    a = (q * np.logspace(0, -6 if k > 1 else 0, k)) @ q.T
    return (a + a.T) / 2 * 2.5


def padded(a, ld):
    out = np.full((a.shape[0], ld), PAD)
    out[:, :a.shape[1]] = a
    return out


def factor(lib, a, ld):
    """-> (ok, bad, sum_log, the matrix after the call) from the header"""
    k = a.shape[0]
    m = padded(a, ld)
    sl, bad = C.c_double(-1.0), C.c_int(-1)
    ok = lib.sm_cholesky_lower(_p(m), k, ld, C.byref(sl), C.byref(bad))
    return bool(ok), bad.value, sl.value, m


@pytest.fixture(scope="module", params=SIZES)
def case(request, lib):
    """k, the matrix, its factor by the reference (lists) and by the header (array, ld = k + 3)"""
    k = request.param
    a = spd(k)
    ok, _, Lr, slr = R.cholesky_lower(a.tolist(), k)
    okh, _, slh, m = factor(lib, a, k + 3)
    assert ok and okh
    return dict(k=k, ld=k + 3, a=a, Lr=Lr, slr=slr, Lh=m, slh=slh)


def lower(L, k):
    return np.tril(np.asarray(L, dtype=np.float64)[:k, :k])


def test_cholesky(lib, case):
    k, ld, a, m = case["k"], case["ld"], case["a"], case["Lh"]
    assert np.array_equal(lower(m, k), lower(case["Lr"], k))
    assert case["slh"] == case["slr"]                                          # sum of log L_jj in j order
    assert np.array_equal(np.triu(m[:, :k], 1), np.triu(a, 1))                 # the upper triangle is left alone ...
    assert np.all(m[:, k:] == PAD)                                             # ... and so is the padding
    for ld2 in (k, k + 1):                                                     # the result does not depend on the leading dimension
        assert np.array_equal(lower(factor(lib, a, ld2)[3], k), lower(m, k))
    assert lib.sm_cholesky_lower(_p(padded(a, ld)), k, ld, None, None) == 1    # both outputs are optional
    lib.sm_zero_upper(_p(m2 := m.copy()), k, ld)
    assert np.array_equal(m2[:, :k], lower(m, k)) and np.all(m2[:, k:] == PAD)
    assert np.abs(lower(m, k) @ lower(m, k).T - a).max() <= 1e-14 * np.abs(a).max()      # (and it is a Cholesky factor)


@pytest.mark.parametrize("k", SIZES)
@pytest.mark.parametrize("kind", ["indefinite", "inf_diagonal", "nan_diagonal"])
def test_cholesky_reports_failure(lib, k, kind):
    a = spd(k)
    at = k // 2
    a[at, at] = {"indefinite": -1.0, "inf_diagonal": np.inf, "nan_diagonal": np.nan}[kind]
    ok, bad, _, _ = R.cholesky_lower(a.tolist(), k)
    okh, badh, _, m = factor(lib, a, k + 2)
    assert not ok and not okh and badh == bad == at
    assert np.all(m[:, k:] == PAD)


def test_solves(lib, case):
    k, ld, Lh, Lr = case["k"], case["ld"], case["Lh"], case["Lr"]
    rng = np.random.default_rng(k)
    b = rng.standard_normal(k)
    for name, ref in (("sm_solve_lower", R.solve_lower), ("sm_solve_lower_transposed", R.solve_lower_transposed), ("sm_cholesky_solve", R.cholesky_solve)):
        x = b.copy()
        getattr(lib, name)(_p(Lh), k, ld, _p(x))
        assert np.array_equal(x, np.array(ref(Lr, k, b.tolist()))), name
    e = np.zeros(k); e[k - 1] = 1.0                                            # a unit vector: the leading zeros of the full solve change nothing
    x = e.copy(); lib.sm_solve_lower(_p(Lh), k, ld, _p(x))
    assert np.array_equal(x[:k - 1], np.zeros(k - 1)) and x[k - 1] == 1.0 / Lr[k - 1][k - 1]
    rows = rng.standard_normal((5, k))
    got = rows.copy()
    lib.sm_solve_lower_rows(_p(Lh), k, ld, 5, _p(got))
    assert np.array_equal(got, np.array(R.solve_lower_rows(Lr, k, rows.tolist())))


def test_inverses(lib, case):
    k, ld, Lh, Lr, a = case["k"], case["ld"], case["Lh"], case["Lr"], case["a"]
    X = np.full((k, k), PAD)
    lib.sm_tri_inverse_lower(_p(Lh), k, ld, _p(X))
    Xr = R.tri_inverse_lower(Lr, k)
    assert np.array_equal(X, np.array(Xr))                                     # the upper triangle comes back zero
    tri = np.full((k, k), PAD); sol = np.full((k, k), PAD); dg = np.full(k, PAD)
    lib.sm_spd_inverse_from_tri(_p(X), k, _p(tri))
    lib.sm_spd_inverse_by_solves(_p(Lh), k, ld, _p(sol))
    lib.sm_inverse_diagonal(_p(Lh), k, ld, _p(dg))
    assert np.array_equal(tri, np.array(R.spd_inverse_from_tri(Xr, k)))
    assert np.array_equal(sol, np.array(R.spd_inverse_by_solves(Lr, k)))
    assert np.array_equal(dg, np.array(R.inverse_diagonal(Lr, k)))
    assert np.array_equal(tri, tri.T)
    inv = np.linalg.inv(a)
    for got in (tri, sol):                                                     # (both are the inverse, to the conditioning)
        assert np.abs(got - inv).max() <= 1e-9 * np.abs(inv).max()
    if k >= 7:      # the two inverses round differently: neither may stand in for the other
        assert not np.array_equal(tri, sol)


def test_matrix_helpers(lib, case):
    k = case["k"]
    rng = np.random.default_rng(50 + k)
    A, B = rng.standard_normal((k, k)), rng.standard_normal((k, k))
    A[rng.uniform(size=(k, k)) < 0.3] = 0.0                                    # zeros are skipped: 0 * inf never appears
    B[0, 0] = np.inf if A[0, 0] == 0.0 and k > 1 else B[0, 0]
    Cm = np.full((k, k), PAD)
    lib.sm_matmul(_p(A), _p(B), k, _p(Cm))
    assert np.array_equal(Cm, np.array(R.matmul(A.tolist(), B.tolist(), k)), equal_nan=True)
    G = rng.standard_normal(k * (k + 1) // 2)
    out = np.full((k, k), PAD)
    lib.sm_sym_from_packed(_p(G), k, _p(out))
    assert np.array_equal(out, np.array(R.sym_from_packed(G.tolist(), k)))


R_GRID = np.concatenate([[0.0], np.linspace(0.0, 40.0, 321)[1:], np.random.default_rng(8).uniform(0.0, 40.0, size=60)])


@pytest.mark.parametrize("cov_type", [0, 1, 2])
def test_matern_forms(lib, cov_type):
    refs = (R.matern_gaussian_paths, R.matern_gaussian_paths_dloga, R.matern_laplace_paths, R.matern_laplace_paths_dloga)
    vals = np.empty((4, 2, R_GRID.size))
    for which, ref in enumerate(refs):
        for si, scale in enumerate((1.0, 0.73)):
            got = np.array([lib.sm_matern(which, cov_type, scale, float(r)) for r in R_GRID])
            assert np.array_equal(got, np.array([ref(cov_type, scale, float(r)) for r in R_GRID])), (which, scale)
            vals[which, si] = got
    assert np.all(vals[[0, 2], :, 0] == [[1.0, 0.73]] * 2) and np.all(vals[[1, 3], :, 0] == 0.0)      # r = 0: the scale, no slope
    np.testing.assert_allclose(vals[0], vals[2], rtol=1e-15, atol=0)                                     # the same function ...
    np.testing.assert_allclose(vals[1], vals[3], rtol=2e-15, atol=0)
    if cov_type > 0:                                                                                     # ... in two roundings (shape 0.5 has one product: no choice)
        assert not np.array_equal(vals[0], vals[2]) and not np.array_equal(vals[1], vals[3])


@pytest.mark.parametrize("k", SIZES)
@pytest.mark.parametrize("d", [1, 2, 3])
def test_inducing_point_covariance(lib, k, d):
    assert lib.sm_jitter_mult() == 1.0 + 1e-6
    pts = np.random.default_rng(10 * k + d).uniform(size=(k, d))
    colmajor = np.asfortranarray(pts).ravel(order="F").copy()
    rowmajor3 = np.zeros((k, 3)); rowmajor3[:, :d] = pts
    var, a = 0.8, 7.5
    for cov_type in (0, 1, 2):
        for lap in (0, 1):
            Sr, dSr = R.ip_cov(pts.tolist(), not lap, cov_type, var, a)
            for ip, rm in ((colmajor, 0), (rowmajor3, 1)):
                Sm, dSm, S2 = np.full((k, k), PAD), np.full((k, k), PAD), np.full((k, k), PAD)
                lib.sm_ip_cov(_p(ip), k, d, rm, lap, cov_type, C.c_double(var), C.c_double(a), _p(Sm), _p(dSm))
                lib.sm_ip_cov(_p(ip), k, d, rm, lap, cov_type, C.c_double(var), C.c_double(a), _p(S2), None)      # the derivative is optional
                assert np.array_equal(Sm, np.array(Sr)) and np.array_equal(dSm, np.array(dSr)) and np.array_equal(S2, Sm), (cov_type, lap, rm)
                assert np.all(np.diag(Sm) == var)                                                                # no jitter: the caller's


def _optimal_c(lib, z1, zP, centre=None):
    out = np.full(3, PAD)
    z1, zP = np.ascontiguousarray(z1, dtype=np.float64), np.ascontiguousarray(zP, dtype=np.float64)
    lib.sm_optimal_c(_p(z1), _p(zP), len(z1), 0 if centre is None else 1, C.c_double(0.0 if centre is None else centre), _p(out))
    return out


@pytest.mark.parametrize("t", [1, 2, 10, 50])
@pytest.mark.parametrize("centred", ["mean", "value"])
def test_optimal_c(lib, t, centred):
    """Samples of scale 1 around a mean of scale 1, so that centring loses nothing the bound does not cover.  A running sum of t terms divided by t is off by at most
    t eps max|term|; c = cov / var inherits (d cov + |c| d var) / var, and `few` = 4 covers the roundings of the centred terms themselves."""
    rng = np.random.default_rng(7 * t + (centred == "value"))
    zP = 0.5 + rng.standard_normal(t)
    z1 = 0.8 * zP + 0.3 * rng.standard_normal(t) - 0.2
    centre = None if centred == "mean" else 0.5
    c, m1, mP = _optimal_c(lib, z1, zP, centre)
    cr, m1r, mPr, ab, bb = R.optimal_c(z1, zP, centre)
    eps, few = np.finfo(np.float64).eps, 4
    assert abs(m1 - m1r) <= t * eps * np.abs(z1).max() and abs(mP - mPr) <= t * eps * np.abs(zP).max()
    if bb.mean() == 0:      # t = 1 centred with the mean
        assert t == 1 and centre is None and c == 1.0
    else:
        tol = few * t * eps * (np.abs(ab).max() + abs(cr) * bb.max()) / bb.mean()
        print("t = %d, %s: c = %.17g, off by %.3e, bound %.3e" % (t, centred, c, abs(c - cr), tol))
        assert abs(c - cr) <= tol


@pytest.mark.parametrize("centre", [None, 0.75])
def test_optimal_c_is_one_without_variance(lib, centre):
    """all control variates equal (0.75 t and its tenth are exact in float64): var == 0 -> c = 1, whatever the samples"""
    z1 = np.random.default_rng(3).standard_normal(10)
    c, m1, mP = _optimal_c(lib, z1, np.full(10, 0.75), centre)
    assert c == 1.0 and mP == 0.75 and abs(m1 - z1.mean()) <= 10 * np.finfo(np.float64).eps * np.abs(z1).max()
