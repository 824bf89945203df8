"""Plain numpy / np.longdouble reference for the dense (exact-GP) path of gpboost_amd/csrc/dense_kernels.hip: a-priori bounds on what the blocked Cholesky, its
Schur complement, the triangular solves and the inverse leave behind, seeded matrix generators, a numpy restatement of the blocked algorithm with mutants, and the
exact-GP quantities (Matern 0.5 / 1.5 / 2.5) in long double.  CPU only; tests/test_dense_ref.py checks this file, tests/test_zz_dense_kernels_gpu.py uses it.

The bounds (u = 2^-53, gamma(t) = t u / (1 - t u); Higham, Accuracy and Stability of Numerical Algorithms, 2nd ed., chapter 10)
--------------------------------------------------------------------------------------------------------------------------------
Factor / Schur complement, entry (i, j), j <= i, k = min(j + 1, ncols) terms of the sum:
    | M_ij - sum_{p < k} out_ip out_jp - [j >= ncols] out_ij |  <=  gamma(k + C_PIVOT) ( sum_{p < k} |out_ip| |out_jp| + [j >= ncols] |out_ij| )
Every computed entry is s = M_ij - sum of (k - 1 or k) products, evaluated in SOME order (MFMA chunks, wide / narrow / strip / rest splits, four running sums in
the panel solve), followed by a final operation.  Whatever the order, a term passes through at most k roundings on its way into s (at most k - 1 additions in a
sum of k terms, one more if the product is rounded on its own; fused multiply-adds only lower that), Higham (10.4)/(10.5) and Lemma 8.4.  The final operation adds
f roundings:
    Schur complement (j >= ncols)           f = 1   (the last subtraction, counted for the stored value)
    LAPACK-style  l_ij = s / l_jj           f = 1;   l_jj = sqrt(s): l_jj^2 = s (1 + d)^2, f = 2
    panel solve of the device               x = s * fl(1 / l_jj): f = 2 (the reciprocal and the product where the theorem has one division)
    diagonal block of the device            inv = rsqrt(piv) by the hardware estimate y0 = piv^-1/2 (1 + d0) and Newton steps
                                            y1 = y0 + y0 (1/2 - (1/2 piv y0) y0):  exactly piv^-1/2 (1 - 3/2 d0^2 - ...); the product 1/2 piv y0 is rounded (that
                                            rounding enters y1 halved), the fma forming the small bracket adds nothing of first order, the last fma rounds once:
                                            inv = piv^-1/2 (1 + e), |e| <= 3/2 u + 3/2 d0^2.  The column is l_jj = fl(piv inv), l_ij = fl(s inv), hence
                                            l_ij l_jj = s (1 + e)^2 (1 + d1)(1 + d2) and l_jj^2 = piv (1 + e)^2 (1 + d1)^2:  f = 2 + 2 |e| / u.
                                            With ONE step and the accuracy the kernel first stated for the estimate, |d0| <= 2^-26 (d0^2 = 2 u): |e| <= 4.5 u, f = 11.
C_PIVOT = 11 is the largest f; it does not depend on the matrix, its size or its condition number.  The constant was set from that statement before any device
run; the first run exceeded it (20 u in column 3 of a 64 x 64 block: the estimate is coarser than stated, d0 about 2^-25.4), and the kernel -- not the constant --
was changed: inv_sqrt_newton takes a second step, after which |e| <= 3/2 u + O(d0^4), f = 5.  The bound stays at 11.

Solve:  (M + dM) x = b with |dM| <= gamma(3 np + 1 + C_PIVOT) |L| |L'| (Thm 10.4 with the factor above), checked normwise:
    || b - M x ||_inf / ( ||M||_inf ||x||_inf + ||b||_inf )  <=  gamma(3 np + 1 + C_PIVOT)

Inverse as the device forms it: the partial factorisation of [[M, .], [I, 0]] leaves Y = I L^-T (panel solves, row i: y_i (L + dL_i)' = e_i', |dL_i| <=
gamma(np + 2) |L|) and X = fl(Y Y') (|X - Y Y'| <= gamma(np) |Y| |Y'|) with L L' = M + dM, |dM| <= gamma(np + C_PIVOT) |L| |L'|.  To first order, with F = I - Y L',
    M X - I  =  -F'  -  M F X  -  dM X  +  M (X - Y Y')
and in the max-entry norm, using Cauchy-Schwarz on the rows of L and of Y (|L| |L'| <= max diag(M) <= ||M||_inf, |Y| |Y'| <= max diag(M^-1) <= ||M^-1||_inf):
    |F|_ij <= gamma sqrt(X_ii M_jj) <= gamma kappa^(1/2),   |dM X| <= gamma ||M||_inf ||X||_1 = gamma kappa,   |M (X - Y Y')| <= gamma ||M||_inf ||M^-1||_inf = gamma kappa,
    |M F X| <= gamma kappa when the row perturbations dL_i are taken as one dL (M F X = L dL' X); row-dependent ones do not reach their worst case kappa^(3/2)
    together -- fp64 LAPACK, which inverts by the same two steps, is checked against the same bound in tests/test_dense_ref.py.
Four terms of at most gamma(np + C_PIVOT) kappa_inf(M) each:  max |M X - I| <= 4 (np + C_PIVOT) u kappa_inf / (1 - ...) <= C2_INVERSE np u kappa_inf(M) with
C2_INVERSE = 5 for every np >= 64 (4 (64 + 11) / 64 = 4.69).
"""
import functools

import numpy as np
from scipy.linalg import solve_triangular

LD = np.longdouble
U = 2.0 ** -53
C_PIVOT = 11
C2_INVERSE = 5.0
TB, OB = 64, 512          # panel width and block-column width of launch_dense_cholesky
ALL_ROWS_UP_TO = 640


def long_double_is_wider():
    return np.finfo(LD).eps < 2e-19


def gamma(t):
    return t * U / (1.0 - t * U)


# ---- componentwise backward error of a full or partial factorisation ---------------------------------------------------------------------------------
def factor_residuals(M, out, ncols, rows=None):
    """-> (rows, r, b): for every row i of `rows` (default: all) the residuals r[i][j] and the sums b[i][j], j <= i, in long double (0 for j > i)."""
    ld = M.shape[0]
    rows = np.arange(ld) if rows is None else np.asarray(sorted(set(int(r) for r in rows)))
    Lq = np.tril(out[:, :ncols]).astype(LD)           # k < min(j + 1, ncols) for j <= i: the lower trapezoid of the first ncols columns
    La = np.abs(Lq)
    r = np.zeros((rows.size, ld), dtype=LD); b = np.zeros((rows.size, ld), dtype=LD)
    for t, i in enumerate(rows):
        kk = min(i + 1, ncols)
        s = Lq[:i + 1, :kk] @ Lq[i, :kk]
        sa = La[:i + 1, :kk] @ La[i, :kk]
        res = M[i, :i + 1].astype(LD) - s
        if i >= ncols:                                 # columns ncols .. i of this row hold the Schur complement
            o = out[i, ncols:i + 1].astype(LD)
            res[ncols:] -= o
            sa[ncols:] += np.abs(o)
        r[t, :i + 1] = np.abs(res); b[t, :i + 1] = sa
    return rows, r, b


def factor_violations(M, out, ncols, rows=None, c=C_PIVOT, want_worst=False):
    """Entries (i, j, r_ij, bound_ij) of the lower triangle, i in `rows`, where r_ij > gamma(min(j + 1, ncols) + c) b_ij; a non-finite entry of `out` in a checked
    row is a violation too.  want_worst: -> (violations, largest r_ij / bound_ij)."""
    ld = M.shape[0]
    rows, r, b = factor_residuals(M, out, ncols, rows)
    k = np.minimum(np.arange(ld) + 1, ncols).astype(np.float64)
    bound = (gamma(k + c)).astype(LD)[None, :] * b
    lower = np.arange(ld)[None, :] <= rows[:, None]
    bad = lower & ~(r <= bound)                        # NaN compares false: reported
    viol = [(int(rows[t]), int(j), float(r[t, j]), float(bound[t, j])) for t, j in zip(*np.nonzero(bad))]
    if not want_worst:
        return viol
    pos = bound > 0
    ratio = np.where(lower & pos, r / np.where(pos, bound, 1), np.where(lower & ~(r <= 0), np.inf, 0))
    worst = float(np.max(ratio))
    return viol, worst if worst == worst else float("inf")


def sample_rows(ld, ncols, lookahead=False, total=48, seed=0):
    """All rows up to ld = 640.  Above: the first and the last row of every 64-block that touches a 512 block column edge, ncols, a Jend or a Send of
    launch_dense_cholesky (and of the first and last block), filled up to `total` rows with a seeded sample."""
    if ld <= ALL_ROWS_UP_TO:
        return np.arange(ld)
    edges = {0, ld, ncols}
    for J0 in range(0, ncols, OB):
        Jend = min(J0 + OB, ncols)
        edges.update((J0, Jend, min(Jend + OB, ld)))
    rows = set()
    for e in edges:
        for blk in (e // TB - 1, e // TB):
            if 0 <= blk < ld // TB:
                rows.update((blk * TB, blk * TB + TB - 1))
    rng = np.random.default_rng(seed + 7919 * ld + ncols)
    rest = [int(v) for v in rng.permutation(ld) if int(v) not in rows]
    rows.update(rest[:max(0, total - len(rows))])
    return np.asarray(sorted(rows))


# ---- solve and inverse --------------------------------------------------------------------------------------------------------------------------------
def solve_backward_error(M, x, b):
    Mq, xq, bq = M.astype(LD), np.asarray(x).astype(LD), np.asarray(b).astype(LD)
    res = np.max(np.abs(bq - Mq @ xq))
    return float(res / (np.max(np.sum(np.abs(Mq), axis=1)) * np.max(np.abs(xq)) + np.max(np.abs(bq))))


def solve_bound(np_):
    return gamma(3 * np_ + 1 + C_PIVOT)


def inverse_residual(M, X, cols):
    """max |M X[:, cols] - I[:, cols]| in long double."""
    cols = np.asarray(cols)
    R = M.astype(LD) @ np.asarray(X)[:, cols].astype(LD)
    R[cols, np.arange(cols.size)] -= 1
    return float(np.max(np.abs(R)))


def kappa_inf(M):
    return float(np.max(np.sum(np.abs(M), axis=1)) * np.max(np.sum(np.abs(np.linalg.inv(M)), axis=1)))


def inverse_bound(np_, kappa):
    return C2_INVERSE * np_ * U * kappa


def pad64(n):
    return (n + TB - 1) // TB * TB


# ---- generators (all seeded) ---------------------------------------------------------------------------------------------------------------------------
GENERATORS = ("well", "ill", "graded", "scaled_up", "scaled_down")


def matern25_1d(n, rng, rho=0.25, nugget=1e-6):
    x = np.sort(rng.uniform(size=n))
    r = np.sqrt(5.0) * np.abs(x[:, None] - x[None, :]) / rho
    return (1.0 + r + r * r / 3.0) * np.exp(-r) + nugget * np.eye(n)


def spd_matrix(kind, n, seed):
    """n x n symmetric positive definite.  well: G G' / n + I;  ill: Matern-2.5 on sorted 1-D points + 1e-6 I;  graded: D (well) D, D = 2^k, k uniform in -20 .. 20;
    scaled_up / scaled_down: well for even seeds, ill for odd ones, times 2^200 / 2^-200."""
    rng = np.random.default_rng([seed, n, GENERATORS.index(kind)])
    if kind in ("scaled_up", "scaled_down"):
        base = spd_matrix("well" if seed % 2 == 0 else "ill", n, seed + 2)
        return base * (2.0 ** 200 if kind == "scaled_up" else 2.0 ** -200)
    if kind == "ill":
        return matern25_1d(n, rng)
    G = rng.standard_normal((n, n))
    A = G @ G.T / n + np.eye(n)
    A = (A + A.T) / 2
    if kind == "graded":
        D = 2.0 ** rng.integers(-20, 21, size=n)
        A = D[:, None] * A * D[None, :]
    return A


def factor_input(kind, ld, ncols, seed=0):
    """The ld x ld symmetric input of a (partial) factorisation: the generator's matrix in the first ncols rows / columns; for ncols < ld a random C21 and a
    random symmetric C22 that is NOT definite (the Schur complement need not be)."""
    A = spd_matrix(kind, ncols, seed)
    if ncols == ld:
        return A
    rng = np.random.default_rng([seed, ld, ncols, 99])
    scale = np.sqrt(np.abs(np.diag(A)).mean())
    M = np.empty((ld, ld))
    M[:ncols, :ncols] = A
    C21 = rng.standard_normal((ld - ncols, ncols)) * scale
    C22 = rng.standard_normal((ld - ncols, ld - ncols)) * scale * scale
    M[ncols:, :ncols] = C21; M[:ncols, ncols:] = C21.T
    M[ncols:, ncols:] = (C22 + C22.T) / 2
    return M


def break_pivot(A, p, value=-1.0):
    """A copy of the positive definite A whose pivot p becomes `value` (<= 0, or NaN) while the pivots before it stay as they are."""
    L = np.linalg.cholesky(A[:p + 1, :p + 1])
    M = A.copy()
    M[p, p] = A[p, p] - L[p, p] ** 2 + value
    return M


# ---- fp64 restatements -----------------------------------------------------------------------------------------------------------------------------------
def lapack_partial(M, ncols):
    """What the factorisation leaves, by fp64 LAPACK: L (lower trapezoid of the first ncols columns), the Schur complement below / right of it (lower triangle),
    the strict upper triangle of M."""
    ld = M.shape[0]
    out = M.copy()
    L11 = np.linalg.cholesky(M[:ncols, :ncols])
    out[:ncols, :ncols] = L11
    if ncols < ld:
        L21 = solve_triangular(L11, M[ncols:, :ncols].T, lower=True).T
        out[ncols:, :ncols] = L21
        out[ncols:, ncols:] = M[ncols:, ncols:] - L21 @ L21.T
    return np.tril(out) + np.triu(M, 1)


def _potrf_block(D):
    """Unblocked Cholesky of the lower triangle of one diagonal block; a pivot that is not positive gives NaN and the sweep goes on, as on the device."""
    L = np.tril(D).copy()
    with np.errstate(invalid="ignore", divide="ignore"):
        for k in range(L.shape[0]):
            L[k, k] = np.sqrt(L[k, k])
            L[k + 1:, k] /= L[k, k]
            L[k + 1:, k + 1:] -= np.tril(np.outer(L[k + 1:, k], L[k + 1:, k]))
    return L


MUTANTS = ("skip_tile", "skip_k_chunk", "strip_twice", "panel_tail_unsolved", "beyond_c_lim")


def blocked_cholesky(M, ncols=None, mutant=None):
    """numpy fp64 restatement of launch_dense_cholesky: 64-wide panels (diagonal block, panel solve, narrow update inside the 512-wide block column), one wide
    update of the trailing matrix per block column, the Schur complement left in place.  mutant: one deliberate defect, applied once, in the first block column's
    updates of the 64-block of rows that starts at its end (tiles a bordering row sample sees):
      skip_tile            one 64 x 64 tile of the wide update is not updated
      skip_k_chunk         one 16-column chunk of K is left out of one tile of the wide update
      strip_twice          the wide update is applied twice on the columns of the next block column (the look-ahead's strip)
      panel_tail_unsolved  the last 64 rows of one panel solve keep their input
      beyond_c_lim         one narrow update also updates the 64 columns after its limit"""
    assert mutant is None or mutant in MUTANTS
    ld = M.shape[0]
    ncols = ld if ncols is None else ncols
    P = M.copy()
    done = False
    for J0 in range(0, ncols, OB):
        Jend = min(J0 + OB, ncols)
        for k0 in range(J0, Jend, TB):
            k1 = k0 + TB
            L11 = _potrf_block(P[k0:k1, k0:k1])
            P[k0:k1, k0:k1] = L11
            if k1 >= ld:
                break
            A21 = P[k1:, k0:k1].copy()
            P[k1:, k0:k1] = solve_triangular(L11, A21.T, lower=True, check_finite=False).T
            if mutant == "panel_tail_unsolved" and not done and k0 == J0:
                P[ld - TB:, k0:k1] = A21[-TB:]; done = True
            c_lim = Jend
            if mutant == "beyond_c_lim" and not done and Jend < ld and k1 < Jend:
                c_lim = Jend + TB; done = True
            if k1 < c_lim:
                P[k1:, k1:c_lim] -= P[k1:, k0:k1] @ P[k1:c_lim, k0:k1].T
        if Jend >= ld:
            break
        Lp = P[Jend:, J0:Jend]
        upd = Lp @ Lp.T
        if not done and mutant in ("skip_tile", "skip_k_chunk", "strip_twice"):
            done = True
            if mutant == "skip_tile":
                upd[:TB, :TB] = 0.0
            elif mutant == "skip_k_chunk":
                upd[:TB, :TB] -= Lp[:TB, 32:48] @ Lp[:TB, 32:48].T
            else:
                w = min(OB, ld - Jend)
                upd[:, :w] *= 2.0
        P[Jend:, Jend:] -= upd
    return np.tril(P) + np.triu(M, 1)


# ---- the exact-GP quantities in long double (n <= 600) ----------------------------------------------------------------------------------------------------
def chol_ld(A):
    A = A.astype(LD)
    n = A.shape[0]
    L = np.zeros((n, n), dtype=LD)
    for j in range(n):
        v = A[j:, j] - L[j:, :j] @ L[j, :j]
        L[j, j] = np.sqrt(v[0])
        L[j + 1:, j] = v[1:] / L[j, j]
    return L


def tri_inv_ld(L):
    n = L.shape[0]
    Y = np.zeros((n, n), dtype=LD)
    for i in range(n):
        row = -(L[i, :i] @ Y[:i, :])
        row[i] += 1
        Y[i, :] = row / L[i, i]
    return Y


def matern_ld(ct, var, a, X1, X2, want_dlog=False):
    """var k(a |x1 - x2|) in long double and, optionally, its derivative with respect to log(a): the parametrisation of oracle/orc.py: exact_nll (pars_trans =
    {., var, a}) and of gpb_hip_exact_grad_terms: k = e^-r, (1 + r) e^-r, (1 + r + r^2 / 3) e^-r with r = a d; d/dlog a = -r e^-r, -r^2 e^-r, -r^2 (1 + r) e^-r / 3."""
    X1 = np.asarray(X1).astype(LD); X2 = np.asarray(X2).astype(LD)
    d2 = np.zeros((X1.shape[0], X2.shape[0]), dtype=LD)
    for q in range(X1.shape[1]):
        df = X1[:, q][:, None] - X2[:, q][None, :]
        d2 += df * df
    r = LD(a) * np.sqrt(d2)
    e = np.exp(-r) * LD(var)
    if ct == 0:
        k, dk = e, -r * e
    elif ct == 1:
        k, dk = (1 + r) * e, -(r * r) * e
    else:
        k, dk = (1 + r + r * r / 3) * e, -(r * r) * (1 + r) * e / 3
    return (k, dk) if want_dlog else k


def exact_reference(coords, y, ct, var, a, coords_pred=None):
    """Long-double exact GP with Psi = Sigma(var, a) + I.  -> dict: nll2 {y' Psi^-1 y, log|Psi|}, y_aux, grad7 (the layout of gpb_hip_exact_grad_terms), psi_inv_diag,
    pred_mean = C Psi^-1 y and pred_q = C Psi^-1 C', and `cancellation`: sum|terms| / |sum| of every scalar output."""
    coords = np.asarray(coords, dtype=np.float64).reshape(len(y), -1)
    n = coords.shape[0]
    S, dS = matern_ld(ct, var, a, coords, coords, want_dlog=True)
    S[np.arange(n), np.arange(n)] = LD(var); dS[np.arange(n), np.arange(n)] = 0
    Psi = S + np.eye(n, dtype=LD)
    L = chol_ld(Psi)
    Li = tri_inv_ld(L)
    Pinv = Li.T @ Li
    yq = np.asarray(y).astype(LD)
    z = Li @ yq
    ya = Li.T @ z
    logs = 2 * np.log(np.diag(L))
    yy = ya[:, None] * ya[None, :]
    terms = {"ypy": z * z, "logdet": logs, "g1_var": -0.5 * S * yy, "g2_var": 0.5 * S * Pinv, "g1_range": -0.5 * dS * yy, "g2_range": 0.5 * dS * Pinv}
    sums = {k: np.sum(v) for k, v in terms.items()}
    canc = {k: float(np.sum(np.abs(v)) / abs(sums[k])) if sums[k] != 0 else (1.0 if not np.any(v) else float("inf")) for k, v in terms.items()}
    res = {"nll2": np.array([sums["ypy"], sums["logdet"]]), "y_aux": ya, "psi_inv_diag": np.diag(Pinv).copy(),
           "grad7": np.array([sums["ypy"], sums["logdet"], LD(0), sums["g1_var"], sums["g2_var"], sums["g1_range"], sums["g2_range"]]), "cancellation": canc}
    if coords_pred is not None:
        C = matern_ld(ct, var, a, np.asarray(coords_pred, dtype=np.float64).reshape(-1, coords.shape[1]), coords)
        Z = Li @ C.T
        res["pred_mean"] = Z.T @ z
        res["pred_q"] = Z.T @ Z
    return res


# the exact-GP cases of the GPU test: (n, d, covariance type); d spread over the sizes, every type at every size
EXACT_CASES = [(n, (i + ct) % 3 + 1, ct) for i, n in enumerate((1, 64, 65, 130, 513, 577)) for ct in (0, 1, 2)]
EXACT_VAR = 2.0
EXACT_NPRED = 70


def exact_range_par(ct, d, n):
    """a = c / rho with the range rho = n^(-1/d), the mean spacing of n points in the unit cube: with longer ranges (or a noisier response) the gradient sums
    y_aux' Sigma y_aux cancel by more than a factor 100 (rho twice as long: 1800) and a relative tolerance on them would say little."""
    return [1.0, 3.0 ** 0.5, 5.0 ** 0.5][ct] / float(n) ** (-1.0 / d)


def exact_inputs(n, d, ct):
    rng = np.random.default_rng([n, d, ct, 4242])
    coords = rng.uniform(size=(n, d))
    y = 1.5 + np.sin(3.0 * coords.sum(axis=1)) + 0.3 * rng.standard_normal(n)
    pred = rng.uniform(size=(EXACT_NPRED, d))
    on = min(3, n)
    pred[:on] = coords[rng.choice(n, size=on, replace=False)]      # prediction points on training points
    return coords, y, pred


@functools.lru_cache(maxsize=None)
def exact_case(n, d, ct):
    coords, y, pred = exact_inputs(n, d, ct)
    return coords, y, pred, exact_reference(coords, y, ct, EXACT_VAR, exact_range_par(ct, d, n), pred)


# ---- the cases of the GPU test (tests/test_zz_dense_kernels_gpu.py), checked against fp64 LAPACK in tests/test_dense_ref.py ----------------------------------
# (ld, ncols, lookahead) and the path of launch_dense_cholesky each one reaches
FACTOR_CASES = [
    (64, 64, 0),        # potrf only
    (128, 128, 0),      # one panel solve, one narrow update
    (128, 64, 0),       # smallest Schur complement
    (576, 576, 0),      # one wide K = 512 update onto a 64-wide remainder
    (1024, 1024, 1),    # look-ahead requested but off (np > 1024 is false)
    (1088, 1088, 0), (1088, 1088, 1),   # strip plus a 64-wide rest on the second stream
    (1344, 704, 1),     # Jend not at a 512 edge, strip ends at np
    (2688, 2688, 0),    # 289 tiles: syrk_mfma_db_kernel<16>, K = 512, without look-ahead
    (2688, 1344, 0),    # gpb_hip_dense_spd_solve with an inverse at n = 1300: narrow update with K = 320
    (3200, 576, 0),     # db kernel with K = 64 from the 64-aligned origin 576
    (3200, 576, 1),     # the same in the rest update on the second stream, origin 1088
    (3200, 3200, 1),    # rest update of 289 tiles under look-ahead
]
SMALLEST_THREE = {(64, 64), (128, 128), (128, 64)}


def factor_kinds(ld, ncols):
    return GENERATORS if (ld, ncols) in SMALLEST_THREE else ("well", "ill")


SOLVE_SIZES = (1, 63, 64, 65, 513, 1300)


def solve_kinds(n):
    return ("well", "ill") if n in (65, 513) else ("well",)


def solve_inputs(kind, n):
    """M, the right-hand side M v for a vector v of small integers, v, and 16 sampled columns (all of them for n <= 16)."""
    M = spd_matrix(kind, n, seed=11)
    rng = np.random.default_rng([n, 5])
    v = rng.integers(-4, 5, size=n).astype(np.float64)
    if not np.any(v):
        v[0] = 1.0
    cols = np.sort(rng.choice(n, size=min(16, n), replace=False))
    return M, M @ v, v, cols
