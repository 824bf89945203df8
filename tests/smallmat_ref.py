"""Pure-Python restatement of gpboost_amd/csrc/gpb_smallmat.h: float64 scalars (Python floats), one operation per step in the order the routine documents,
math.exp / math.sqrt / math.log (the same libm as the library's).  Written from the call sites the header replaced, not from the header: the Cholesky here runs
column by column as the Laplace sites did (the header runs row by row as the C API did), the triangular inverse is the C API's form.  Matrices are lists of rows.
tests/test_smallmat.py asks the header for the same bits.

optimal_c is the exception: a numpy restatement in extended precision, held to a rounding bound and not to bits (its four former copies are gone with the change
that added it; tests/test_zz_laplace_grad_sites_gpu.py holds the sites to the bits they gave)."""
import math

import numpy as np


def cholesky_lower(A, k):
    """-> (ok, bad, L, sum_log): column j -- the pivot, then the rows below it; the sums over p ascending"""
    L = [row[:] for row in A]
    sum_log = 0.0
    for j in range(k):
        sd = L[j][j]
        for p in range(j):
            sd -= L[j][p] * L[j][p]
        if not (sd > 0.0) or not math.isfinite(sd):
            return False, j, L, sum_log
        l = math.sqrt(sd)
        L[j][j] = l
        sum_log += math.log(l)
        for i in range(j + 1, k):
            tv = L[i][j]
            for p in range(j):
                tv -= L[i][p] * L[j][p]
            L[i][j] = tv / l
    return True, -1, L, sum_log


def solve_lower(L, k, b):
    x = list(b)
    for i in range(k):
        v = x[i]
        for p in range(i):
            v -= L[i][p] * x[p]
        x[i] = v / L[i][i]
    return x


def solve_lower_transposed(L, k, b):
    x = list(b)
    for i in range(k - 1, -1, -1):
        v = x[i]
        for p in range(i + 1, k):
            v -= L[p][i] * x[p]
        x[i] = v / L[i][i]
    return x


def cholesky_solve(L, k, b):
    return solve_lower_transposed(L, k, solve_lower(L, k, b))


def solve_lower_rows(L, k, rows):
    return [solve_lower(L, k, r) for r in rows]


def tri_inverse_lower(L, k):
    X = [[0.0] * k for _ in range(k)]
    for c in range(k):
        X[c][c] = 1.0 / L[c][c]
        for i in range(c + 1, k):
            s = 0.0
            for q in range(c, i):
                s -= L[i][q] * X[q][c]
            X[i][c] = s / L[i][i]
    return X


def spd_inverse_from_tri(X, k):
    inv = [[0.0] * k for _ in range(k)]
    for i in range(k):
        for j in range(i + 1):
            s = 0.0
            for q in range(i, k):
                s += X[q][i] * X[q][j]
            inv[i][j] = inv[j][i] = s
    return inv


def spd_inverse_by_solves(L, k):
    inv = [[0.0] * k for _ in range(k)]
    for c in range(k):
        x = cholesky_solve(L, k, [1.0 if i == c else 0.0 for i in range(k)])
        for i in range(k):
            inv[i][c] = x[i]
    return inv


def inverse_diagonal(L, k):
    out = []
    for c in range(k):
        col, ss = [0.0] * k, 0.0
        for i in range(c, k):
            v = 1.0 if i == c else 0.0
            for p in range(c, i):
                v -= L[i][p] * col[p]
            col[i] = v / L[i][i]
            ss += col[i] * col[i]
        out.append(ss)
    return out


def matmul(A, B, k):
    C = [[0.0] * k for _ in range(k)]
    for i in range(k):
        for q in range(k):
            a = A[i][q]
            if a == 0.0:
                continue
            for j in range(k):
                C[i][j] += a * B[q][j]
    return C


def sym_from_packed(G, k):
    out = [[0.0] * k for _ in range(k)]
    for p in range(k):
        for q in range(p + 1):
            out[p][q] = out[q][p] = G[p * (p + 1) // 2 + q]
    return out


# the two Matern forms (cov_type 0 / 1 / 2 = shape 0.5 / 1.5 / 2.5), value and d / d log a at the scaled distance r
def matern_gaussian_paths(cov_type, scale, r):
    e = scale * math.exp(-r)
    return e if cov_type == 0 else (e * (1.0 + r) if cov_type == 1 else e * (1.0 + r + r * r / 3.0))


def matern_gaussian_paths_dloga(cov_type, scale, r):
    e = scale * math.exp(-r)
    return -r * e if cov_type == 0 else (-r * r * e if cov_type == 1 else -r * r * (1.0 + r) * e / 3.0)


def matern_laplace_paths(cov_type, scale, r):
    if cov_type == 0:
        return scale * math.exp(-r)
    if cov_type == 1:
        return scale * (1.0 + r) * math.exp(-r)
    return scale * (1.0 + r + r * r / 3.0) * math.exp(-r)


def matern_laplace_paths_dloga(cov_type, scale, r):
    if cov_type == 0:
        return -scale * r * math.exp(-r)
    if cov_type == 1:
        return -scale * r * r * math.exp(-r)
    return -scale * r * r * (1.0 + r) / 3.0 * math.exp(-r)


def ip_cov(points, gaussian_form, cov_type, var, a):
    """points: k rows of d coordinates -> (Sm, dSm); the squared differences are added in coordinate order (zero padding adds exact zeros)"""
    k = len(points)
    f, g = (matern_gaussian_paths, matern_gaussian_paths_dloga) if gaussian_form else (matern_laplace_paths, matern_laplace_paths_dloga)
    Sm = [[0.0] * k for _ in range(k)]
    dSm = [[0.0] * k for _ in range(k)]
    for i in range(k):
        for j in range(i + 1):
            s2 = 0.0
            for c in range(len(points[i])):
                t = points[i][c] - points[j][c]
                s2 += t * t
            r = a * math.sqrt(s2)
            Sm[i][j] = Sm[j][i] = f(cov_type, var, r)
            dSm[i][j] = dSm[j][i] = g(cov_type, var, r)
    return Sm, dSm


def optimal_c(z1, zP, centre=None):
    """CalcOptimalC: c = cov(z1, zP) / var(zP) over the t samples, 1 where the variance is 0; zP centred with `centre` or, None, with its sample mean.
    -> (c, mean1, meanP, the centred products a1 b1, the squares b1^2) in long double"""
    z1, zP = np.asarray(z1, dtype=np.longdouble), np.asarray(zP, dtype=np.longdouble)
    m1, mP = z1.mean(), zP.mean()
    a1, b1 = z1 - m1, zP - (mP if centre is None else np.longdouble(centre))
    cov, var = (a1 * b1).mean(), (b1 * b1).mean()
    return (np.longdouble(1.0) if var == 0 else cov / var), m1, mP, a1 * b1, b1 * b1
