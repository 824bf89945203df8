"""Long-double restatement of the block operations of the low-rank preconditioners (gpboost_amd/csrc/pivchol_kernels.h: pc_gram, pc_ltwx, pc_combine) with a
componentwise error bound for an fp64 implementation -- the checker of tests/test_zz_lowrank_kernels_gpu.py (its own check: tests/test_lowrank_ref.py, CPU).

Layouts: L (n, k) row-major; W (n,); block vectors X / out (ncol, n, nc): [chunk][row][nc]; small operands x2 (ncol, k, nc): [chunk][k][nc]; M (k, k) row-major;
G: the lower triangle of L' diag(W) L packed by rows, e = p (p + 1) / 2 + q.

The bound.  Every output element is a sum of N products evaluated in fp64 with fused multiply-adds in SOME order (matrix instructions, partial sums per row slice,
quarters of slices): whatever the order, |computed - exact| <= gamma_N * sum |terms|, gamma_N = N u / (1 - N u), u = 2^-53 (Higham, Accuracy and Stability of Numerical
Algorithms, section 3.1), plus one rounding per product that is formed before it enters the fma (W_i X_ic, L_ip W_i, W_i acc, X / sqrt(W)).  bound = N u sum |terms|
computed here in long double; the tests assert |device - reference| <= 4 * bound: the factor covers those few extra roundings per term (at most 3: 1 / W, sqrt, product)
and the final addition -- (N + 4) u sum|terms| <= 4 N u sum|terms| for every N >= 2, and for N = 1 the count is at most 4 roundings.
  pc_gram     G_pq = sum_i L_ip W_i L_iq                          N = n
  pc_ltwx     x2_qc = sum_p M_qp sum_i L_ip W_i X_ic              N = n + k  (n for the inner sums, k more for the product with M)
  pc_combine  a_ic = sum_q L_iq x2_qc (k terms) and the epilogue's own term in X:  N = k + 1
              mode 0: W X - W a,  1: X - a,  2: a + X / sqrt(W),  3: -W a,  4: X + W a
The long-double reference itself is exact to N 2^-64 sum |terms|: 2^-11 of the bound."""
import numpy as np

LD = np.longdouble
U = LD(2.0) ** -53
FACTOR = 4


def long_double_is_wider():
    """x87 extended precision (64-bit significand): the reference is worth its name only then."""
    return np.finfo(LD).eps <= 2.0 ** -63


def make_inputs(n, k, ncol, nc, seed):
    """Mixed signs; W spans 1e-6 .. 1e2 (a Hessian diagonal); with nc = 4 the last column of the last chunk of X is NaN (the padding of a probe block whose probe count
    is no multiple of 4 is the caller's: nothing of it may reach another column)."""
    rng = np.random.default_rng(seed)
    L = rng.standard_normal((n, k)) * np.exp(rng.uniform(-2.0, 2.0, size=(1, k)))
    W = 10.0 ** rng.uniform(-6.0, 2.0, size=n)
    M = rng.standard_normal((k, k)) / np.sqrt(k)
    X = rng.standard_normal((ncol, n, nc)) * np.exp(rng.uniform(-3.0, 3.0, size=(ncol, 1, nc)))
    x2 = rng.standard_normal((ncol, k, nc))
    if nc == 4:
        X[-1, :, -1] = np.nan
    return dict(L=L, W=W, M=M, X=X, x2=x2)


def _cols(B):
    """(ncol, rows, nc) -> (rows, ncol * nc) long double"""
    return np.ascontiguousarray(np.transpose(B, (1, 0, 2)).reshape(B.shape[1], -1)).astype(LD)


def _block(A, ncol, nc):
    """(rows, ncol * nc) -> (ncol, rows, nc)"""
    return np.transpose(A.reshape(A.shape[0], ncol, nc), (1, 0, 2))


def ref_gram(L, W):
    n, k = L.shape
    Ll = L.astype(LD); LW = Ll * W.astype(LD)[:, None]
    G = LW.T @ Ll
    S = np.abs(LW).T @ np.abs(Ll)
    tri = np.tril_indices(k)
    return G[tri], (LD(n) * U * S)[tri]


def ref_ltwx(L, W, M, X):
    n, k = L.shape
    ncol, _, nc = X.shape
    LW = L.astype(LD) * W.astype(LD)[:, None]
    Xm = _cols(X)
    Ml = M.astype(LD)
    y = LW.T @ Xm
    S = np.abs(LW).T @ np.abs(Xm)
    return _block(Ml @ y, ncol, nc), _block(LD(n + k) * U * (np.abs(Ml) @ S), ncol, nc)


def combine_parts(L, x2):
    """a = L x2 and sum |L| |x2| as (n, ncol * nc) long double: shared by the five modes."""
    Ll = L.astype(LD); xm = _cols(x2)
    return Ll @ xm, np.abs(Ll) @ np.abs(xm)


def ref_combine(L, W, X, x2, mode, parts=None):
    n, k = L.shape
    ncol, _, nc = X.shape
    a, T = combine_parts(L, x2) if parts is None else parts
    w = W.astype(LD)[:, None]
    x = _cols(X)
    if mode == 0:
        r, S = w * x - w * a, np.abs(w * x) + w * T
    elif mode == 1:
        r, S = x - a, np.abs(x) + T
    elif mode == 2:
        xs = x / np.sqrt(w)
        r, S = a + xs, T + np.abs(xs)
    elif mode == 3:
        r, S = -w * a, w * T                    # (X does not enter: a NaN there reaches nothing)
    else:
        r, S = x + w * a, np.abs(x) + w * T
    return _block(r, ncol, nc), _block(LD(k + 1) * U * S, ncol, nc)


def check(dev, ref, bound, what=""):
    """|dev - ref| <= FACTOR * bound componentwise; NaN exactly where the reference has NaN.  -> the largest ratio |dev - ref| / bound (0 where both vanish)."""
    dev = np.asarray(dev); ref = np.asarray(ref); bound = np.asarray(bound)
    assert dev.shape == ref.shape == bound.shape, (what, dev.shape, ref.shape, bound.shape)
    nan = np.isnan(ref)
    assert np.array_equal(np.isnan(dev), nan), "%s: NaN at %d places, the reference has %d" % (what, int(np.isnan(dev).sum()), int(nan.sum()))
    ok = ~nan
    err = np.abs(dev[ok].astype(LD) - ref[ok])
    b = bound[ok]
    assert np.all(np.isfinite(b)) and np.all(b >= 0)
    ratio = np.where(b > 0, err / np.where(b > 0, b, 1), np.where(err > 0, np.inf, 0.0))
    worst = float(ratio.max()) if ratio.size else 0.0
    assert worst <= FACTOR, "%s: |device - reference| = %.3g x the bound N u sum|terms| at its worst element (%d of %d beyond %d x)" % (
        what, worst, int((ratio > FACTOR).sum()), ratio.size, FACTOR)
    return worst
