"""Plain numpy / np.longdouble model of ONE point of the Vecchia factor as gpboost_amd/csrc/vecchia_kernels.hip (m <= 62, d <= 3) and
vecchia_big_kernels.hip (62 < m <= 126 or d > 3) compute it, with an a-priori bound next to every value, the case tables of
tests/test_zz_vecchia_point_instances_gpu.py and mutants of the model.  CPU only, imports nothing from oracle/; tests/test_vecchia_point_ref.py checks this file.

The values (all in long double; N = the point's neighbour list without its trailing -1, k = |N| <= m)
-----------------------------------------------------------------------------------------------------
    r_rc = a dist(N_r, N_c), r_r = a dist(i, N_r)                         scaled distances
    K(r)  = var e^-r | var (1 + r) e^-r | var (1 + r + r^2 / 3) e^-r      Matern 0.5 | 1.5 | 2.5 on the transformed scale
    dK(r) = -r var e^-r | -r^2 var e^-r | -(1/3) r^2 (1 + r) var e^-r     d K / d log a
    C = K(r_rc) off the diagonal, C_rr = var + 1 | var + nug_{N_r} | fl(var (1 + 1e-10))    Gaussian | sample weights | latent (gauss = False)
    c = K(r_r),  c0 = var + 1 | var + nug_i | var
    A = C^-1 c,  D = c0 - A.c,  b = C^-1 y_N,  u = y_i - A.y_N
The seven caller-facing terms of the point, restated from orc_vecchia_nll_grad (oracle/gpb_oracle.c) and shim.grad_from_terms, gradient = g1 / sigma2 + g2:
    quad = u^2 / D,  logdet = log D,  bad = [D <= 0]
    variance: dD = D - nug_i - sum_r n_r A_r^2,  uk = -sum_r n_r b_r A_r         (n_r = the nugget of row r: 1, or nug_{N_r}; from dA = C^-1 (c - (C - diag n) A))
    range:    dD = A' dC A - 2 A.dc,             uk = b' dC A - b.dc             (dC, dc = dK of the entries of C, c; zero diagonal; from dA = C^-1 (dc - dC A))
    g1 = uk u' - u'^2 dD / 2,  g2 = dD / (2 D),  u' = u / D                      -> {quad, logdet, bad, g1v, g2v, g1r, g2r}

The bounds (u = 2^-53, gamma(t) = t u / (1 - t u); first order in ONE perturbation model)
--------------------------------------------------------------------------------------
The device factorises C + dC and solves with c + dc, c0 + dc0:
    |dC_rc| <= eK_rc + gamma(g) sqrt(C_rr C_cc),   |dc_r| <= eK_r + gamma(g) sqrt(C_rr c0),   |dc0| <= gamma(g) c0,   diagonal: gamma(g) C_rr only
eK is the error of one covariance evaluation (below); the gamma(g) part is the backward error of elimination and substitution (Higham, Accuracy and Stability of
Numerical Algorithms, 2nd ed.: Thm 10.3 |dA| <= gamma(n + 1) |R'| |R| for the factor, Thm 10.4 gamma(3 n + 1) with both substitutions, and (10.7)
(|R'| |R|)_rc <= sqrt(a_rr a_cc)).  The count g, for the augmented system of MT + 2 rows (neighbours, the point, the responses) the point kernel eliminates:
    right-looking LDL' (MT <= 30, and MT > 46 in the solving modes): entry (r, c) receives at most MT fused updates M -= L_ck (L_rk * inv_k): MT roundings, one for the
        product with inv_k, and inv_k = fast_rcp(pivot) = rcp estimate (1 + d0) and one Newton step = (1 - d0^2)(1 + u): 2^-50 + u = 9 u       -> MT + 10
    left-looking Cholesky (MT > 30 in nll mode, 30 < MT <= 46 in the solving modes): MT fused updates, then the column is scaled by rs = rsq estimate and one Newton
        step = piv^-1/2 (1 + e), |e| <= 3/2 u + 3/2 d0^2 = 13.5 u; l_rc l_cc = s (1 + e)^2 (1 + d1)(1 + d2): 2 + 2 * 13.5 = 29 (the count of tests/dense_ref.py) -> MT + 29
    back-substitution for A and b (both forms): at most MT further terms per entry, a 16-lane tree (4) and the product with 1 / S_kk where there is one  -> MT + 5
    D and u are entries of the Schur complement: no further operation.
    G_POINT(MT) = 2 (MT + 2) + 30 covers the larger (left-looking) form with its back-substitution; nll mode needs no back-substitution and is held to the same g.
    generality kernel: Cholesky with sqrt and division (k + 1), two forward (k) and two backward (k) substitutions, 128-lane tree sums (7): G_BIG(m) = 3 m + 12.
d0 is the relative error of v_rsq_f64 / v_rcp_f64: D0 = 2^-25.  tests/dense_ref.py records 2^-25.4 as observed for v_rsq_f64 on this part; that is the only source in the
project -- an observation, not a specification.
The response row is not part of the SPD system; its backward error is |dy_c| <= gamma(g) sqrt(y_N' C^-1 y_N) sqrt(C_cc) (Cauchy-Schwarz on the row L_y = S^-1 y_N of the
factor, as (10.7)), and gamma(g) (sqrt(y_N' C^-1 y_N) sqrt(c0) + |u|) on the entry that becomes u.

One covariance evaluation, derived from the operation sequence of exp_of_scaled / matern_cov_s / matern_cov_dlog_s / matern_dlog_range_s (dev_common.h), sq_dist_s and
the record gather (vecchia_kernels.hip), before any device run.  Each line: roundings of at most u relative each.
  the scaled distance rp ~ r 256 / ln2:
    sc = fl(a * kCoordScale), kCoordScale a rounded constant                                             2
    p_t = fl(fl(q_t - ctr_t) * sc): the records are CENTRED on the point, each coordinate 2 roundings relative to ITSELF, so the difference of two
          neighbours' records carries 2 u (|p_t| + |q_t|), not 2 u |p_t - q_t|: on r_rc that is 2 u (r_r + r_c) = 2 u r_rc + 2 u (r_r + r_c - r_rc);
          the second part (>= 0 by the triangle inequality, 0 for the entries of c, where the point's own record is exactly 0) is kept as its own term, C_C = 2   2
    dx = fl(p_t - q_t)                                                                                   1
    d fused adds into d2 (d <= 3: at most 3; d > 3 in the generality kernel: 10), halved by the square root   1.5 (5)
    h = rsq(d2) (1 + d0); g = fl(d2 h) enters rp halved; e = fma(-h, g, 3); rp = fl(g e)                 2.5
    Newton remainder 3/2 d0^2 = 3/2 2^-50                                                                12
    sum 21 -> C_R = 22 (26 for d > 3);  |delta r_rc| <= u (C_R r_rc + C_C (r_r + r_c - r_rc)).   The +1e-300 under the root moves r by at most 2 sqrt(1e-300) ln2 / 256 = 5.41521e-153 absolutely (R_FLOOR = 5.416e-153; a duplicate's distance, so the guard's value itself is pinned to 3e-4).
  the value, Matern 0.5:  table entry exp2(j / 256) of the host's libm (< 1 ulp = 2 u), times var (1), Horner polynomial (last fma 1, remainder 4e-17 = 0.4,
    earlier roundings and the rounded coefficients scaled by |rr| ln2 / 256 <= 1.4e-3), the product (1); v_ldexp_f64 exact above the flush             C_A = 6
  Matern 1.5:  (1 + r) with r = fl(rp * fl(ln2 / 256)) (2, weighted r / (1 + r) <= 1), its sum (1), the product (1)                                       C_A = 10
  Matern 2.5:  r (2) enters 1 + r + r^2 / 3 with weight (r + 2 r^2 / 3) / (1 + r + r^2 / 3) <= 2 (4), the rounded 1 / 3 (1), two fma (2), the product (1)  C_A = 14
  |dK|: Matern 0.5 -r ev: r (2), product (1) -> C_A(0.5) + 3 = 9;  1.5: -(r r) ev: 2 * 2 + 1 + 1 -> 12;  2.5: -(1/3)(r r)(1 + r) ev: 1 + (4 + 1) + 1 + (1 + 2) + 1 + 1 -> 18
  The error of r enters through the exact derivative:   eK = C_A u |K| + |K'(r)| |delta r| + 1e-300 var,   e_dK = C_dK u |dK| + |dK'(r)| |delta r| + 1e-300 var
  (for Matern 0.5, |K'| = K: eK = (C_A + C_R r) u K, the form eps_K(rho) = (C_A + C_R rho) u; |K'| <= K for the other two, so eps_K bounds them as well).  The last term:
  v_ldexp_f64 flushes results below the normal range, entries whose exact value is below 1e-300 var are compared absolutely.

What follows from the model (E, e_c, e0 the bounds above, |.| entrywise, Ci = |C^-1|):
    |dA| <= Ci (e_c + E |A|)                  |dD| <= e0 + 2 |A|' e_c + |A|' E |A|             |db| <= Ci (E |b| + e_y)
    |du| <= |dA|' |y_N| + gamma(k + 1) (|y_i| + |A|' |y_N|) + |A|' e_y + gamma(g) (sqrt(y_N' C^-1 y_N) sqrt(c0) + |u|)
    log D: |dD| / D;   u^2 / D: 2 |u| |du| / D + u^2 |dD| / D^2 + 3 u u^2 / D
    gradient terms: first order in dA, db, d(dC), d(dc), plus gamma(number of summands + 4) x the sum of the absolute summands; the weighted variance terms take the
    nugget as fl(var + nug) - var on the device: u (var + nug_r) absolutely.
Sums over a range of points: the sum of the per-point bounds + gamma(npoints + 16) x the sum of the absolute per-point values (fixed-order compensated reduction).
logdet needs one more term.  The point kernel keeps, per worker and per column q of 16 (the q-th point of every group), the running product of the D_i as (mantissa, exponent): one
multiply per point, rounded once, the rescaling exact -- npoints u in all on the sum of logs.  At the end every (worker, column) takes ONE logarithm, t = log(mant) + e ln2 with
mant in [1/2, 1): the device's log to 2 ulp = 4 u |log mant| <= 4 u 0.70, the product with the rounded ln2 2 u |e| ln2, the sum 1 u |t|; since e ln2 = t - log(mant),
|e| ln2 <= |t| + 0.70 and |t| <= the sum of |log D_i| over that column's points: at most u (3 |t| + 6 * 0.70) <= 8 u (sum |log D_i| + 0.70) per (worker, column).  Summed over the
16 columns of a worker and over the workers: 8 u (sum over all points |log D_i| + 16 * 0.70 workers); 16 * 0.70 = 11.2 is doubled to 23 for the workers' inactive rows and
second-order terms.  LOGDET_SUM = npoints u + 8 u (sum |log D_i| + 23 workers).  (The generality kernel takes log D_i per point: 4 u |log D_i|, inside the same expression.)

Observed error / bound
----------------------
fp64 oracle (oracle/gpb_oracle.c: LAPACK-style Cholesky on the host, libm exp), largest ratio over the checked points of the GPU case lists per class (A, D, u and the
per-point terms together; the oracle has no modes and one elimination form): ORACLE_WORST below, recorded by tests/test_vecchia_point_ref.py::test_oracle_is_inside_the_bounds.
The device's figures per (MT, mode, left- or right-looking, weights) and for the generality kernel are in DESIGN.md section 3.
Resolution: the bounds on A, D, u aggregate k^2 entry errors, so ONE entry off by 2e-13 relative is caught where the result is most sensitive to it (the point's covariance
with its nearest neighbour: 2.5 - 13 x the bound) and not reliably in a generic off-diagonal entry (C[1][0]: 0.7 - 2.1 x).
"""
import collections
import functools
import math

import numpy as np

LD = np.longdouble
U = 2.0 ** -53
D0 = 2.0 ** -25
C_R, C_R_ND, C_C = 22.0, 26.0, 2.0
C_A = {0: 6.0, 1: 10.0, 2: 14.0}
C_DK = {0: 9.0, 1: 12.0, 2: 18.0}
FLUSH = 1e-300
R_FLOOR = 5.416e-153      # the +1e-300 under the square root: 2 sqrt(1e-300) ln2 / 256 = 5.41521e-153 on r (what a duplicate's distance becomes), rounded up in the fourth digit
MT_LIST = (10, 20, 30, 40, 50, 62)
TERMS = ("quad", "logdet", "bad", "g1v", "g2v", "g1r", "g2r")

# largest error / bound of the fp64 oracle per class over the checked points of the GPU case lists (filled from test_oracle_is_inside_the_bounds)
ORACLE_WORST = {"MT=10 latent": 0.013, "MT=10 uniform": 0.041, "MT=10 weighted": 0.063, "MT=20 latent": 0.007, "MT=20 uniform": 0.031, "MT=20 weighted": 0.025, "MT=30 latent": 0.012, "MT=30 uniform": 0.015, "MT=30 weighted": 0.023,
                "MT=40 latent": 0.008, "MT=40 uniform": 0.019, "MT=40 weighted": 0.014, "MT=50 latent": 0.006, "MT=50 uniform": 0.014, "MT=50 weighted": 0.016, "MT=62 latent": 0.005, "MT=62 uniform": 0.017, "MT=62 weighted": 0.010,
                "big m=63 uniform": 0.012, "big m=63 weighted": 0.012, "big m=126 uniform": 0.008, "big m=126 weighted": 0.007}


def long_double_is_wider():
    return np.finfo(LD).eps < 2e-19


def gamma(t):
    return t * U / (1.0 - t * U)


def padded_mt(m):
    for s in MT_LIST:
        if m <= s:
            return s
    return None


def g_point(mt):
    return 2 * (mt + 2) + 30


def g_big(m):
    return 3 * m + 12


# ---- the covariance function ----------------------------------------------------------------------------------------------------------------------------
def kern(cov, r, var, third=LD(1) / 3):
    """-> (K, |K'(r)|, dK / dlog a, bound on |d(dK)/dr|) for scaled distances r (long double arrays)."""
    r = np.asarray(r, dtype=LD)
    e = LD(var) * np.exp(-r)
    if cov == 0:
        return e, e, -r * e, (1 + r) * e
    if cov == 1:
        return (1 + r) * e, r * e, -(r * r) * e, (2 * r + r * r) * e
    return (1 + r + r * r / 3) * e, (r * (1 + r) / 3) * e, -third * (r * r) * (1 + r) * e, third * (2 * r + 2 * r * r + r ** 3) * e


def eps_K(cov, rho):
    """relative error bound (C_A + C_R rho) u of one kernel value at scaled distance rho = a dist (entries of c: no centring excess)"""
    return (C_A[cov] + C_R * rho) * U


def _dist(X, Y):
    return np.sqrt(np.sum((X[:, None, :] - Y[None, :, :]) ** 2, axis=2))


# ---- long double linear algebra (numpy's linalg has none) --------------------------------------------------------------------------------------------------
def chol_ld(C):
    k = C.shape[0]
    L = np.zeros((k, k), dtype=LD)
    for j in range(k):
        s = C[j:, j] - L[j:, :j] @ L[j, :j]
        L[j:, j] = s / np.sqrt(s[0])
    return L


def lower_inverse_ld(L):
    """L^-1, all right-hand sides at once"""
    k = L.shape[0]
    X = np.zeros((k, k), dtype=LD)
    for j in range(k):
        rhs = -(L[j, :j] @ X[:j, :])
        rhs[j] += 1
        X[j, :] = rhs / L[j, j]
    return X


# ---- cases -------------------------------------------------------------------------------------------------------------------------------------------------
# kind: "inst" (b, c), "latent", "big" (d), "cov" (a)
Case = collections.namedtuple("Case", "id kind m mt cov d wt gauss var a n seed dup")
PARAMS = ((3.0, 9.0), (7.5, 11.0))
# latent (gauss = False) parameters: (0.7, 4) as the existing tests use, unless the bounds are vacuous there (conditioning of C with the 1e-10 jitter alone): the
# conditions max bound(A) <= 1e-8 and bound(D) <= 1e-8 var (asserted in tests/test_vecchia_point_ref.py) fail only for the MT = 30 case of the list below (Matern 2.5,
# d = 2: bound(A) 1.4e-7 at a = 4, 1.8e-8 at a = 6, 4.4e-9 at a = 8), which gets the shorter correlation range a = 8.  The MT >= 40 cases of this list (Matern 0.5 / d = 3,
# Matern 1.5 / d = 2, Matern 2.5 / d = 3) hold them at a = 4 (at most 2.6e-9).
LATENT_PARAMS = {10: (0.7, 4.0), 20: (0.7, 4.0), 30: (0.7, 8.0), 40: (0.7, 4.0), 50: (0.7, 4.0), 62: (0.7, 4.0)}
SMALLEST_M = {10: 1, 20: 11, 30: 21, 40: 31, 50: 41, 62: 51}


def _n_of(mt):
    return 16 * ((mt + 40 + 15) // 16) + 5


def instance_cases():
    """The 72 cases MT x COV x D3 x WT of (b) and (c).  m = MT or the smallest m that pads to MT, alternating with cov + d3 + wt, so that every (MT, m) pair meets every
    COV and both D3; D3 = False runs with d = 2, every third case with d = 1; the parameters alternate between (3, 9) and (7.5, 11)."""
    out = []
    for q, mt in enumerate(MT_LIST):
        for cov in range(3):
            for d3 in (0, 1):
                for wt in (0, 1):
                    idx = len(out)
                    m = mt if (cov + d3 + wt) % 2 == 0 else SMALLEST_M[mt]
                    d = 3 if d3 else (1 if idx % 3 == 2 else 2)
                    var, a = PARAMS[(q + cov + wt) % 2]
                    n = _n_of(mt)
                    out.append(Case("mt%d-cov%d-d%d-%s-m%d" % (mt, cov, d, "w" if wt else "u", m), "inst", m, mt, cov, d, bool(wt), True, var, a, n, 1000 + idx, True))
    return out


def latent_cases():
    """gauss = False, unweighted, one per MT (nll and factor modes: the gradient entry point is Gaussian only); no duplicated pair -- with the 1e-10 jitter alone a
    duplicate makes C singular to working precision and every bound vacuous."""
    out = []
    for q, mt in enumerate(MT_LIST):
        var, a = LATENT_PARAMS[mt]
        out.append(Case("latent-mt%d-cov%d-d%d" % (mt, q % 3, 2 + q % 2), "latent", mt, mt, q % 3, 2 + q % 2, False, False, var, a, _n_of(mt), 2000 + q, False))
    return out


def big_cases():
    """The generality kernel: m in {63, 126} x d in {2, 3, 5} x the three shapes x weights (gpb_hip.cpp admits every combination for d = 5)."""
    out = []
    for m in (63, 126):
        for d in (2, 3, 5):
            for cov in range(3):
                for wt in (0, 1):
                    idx = len(out)
                    var, a = PARAMS[(cov + wt + d) % 2]
                    out.append(Case("big-m%d-cov%d-d%d-%s" % (m, cov, d, "w" if wt else "u"), "big", m, None, cov, d, bool(wt), True, var, a, m + 37, 3000 + idx, True))
    return out


def sweep_cases():
    """(a): the covariance function alone, m = 1 (MT = 10), the three shapes, d = 1, 2, 3, both gauss settings; a = 8 (a power of two: rho = a dist is exact in d = 1)"""
    n = covariance_sweep(1)[0].shape[0]
    return [Case("sweep-cov%d-d%d-%s" % (cov, d, "gauss" if gauss else "latent"), "cov", 1, 10, cov, d, False, gauss, 3.0, 8.0, n, 4000 + 10 * cov + d, False)
            for cov in range(3) for d in (1, 2, 3) for gauss in (True, False)]


def all_cases():
    return instance_cases() + latent_cases() + big_cases()


CaseData = collections.namedtuple("CaseData", "coords nn y nug dup")


@functools.lru_cache(maxsize=None)
def case_data(case):
    """Seeded inputs of a case: coordinates uniform in the unit cube with one exactly duplicated pair, the m nearest predecessors by brute force (rows i < m are
    short), a seeded response, weights uniform in [0.3, 3] (nug = 1 / w)."""
    rng = np.random.default_rng(case.seed)
    n, m, d = case.n, case.m, case.d
    if case.kind == "cov":
        coords, nn = covariance_sweep(d, case.a)
        y = rng.standard_normal(n)
        for arr in (coords, nn, y):
            arr.setflags(write=False)
        return CaseData(coords, nn, y, None, None)
    coords = rng.uniform(size=(n, d))
    dup = None
    if case.dup:
        dup = (min(m + 3, n - 6), min(m + 9, n - 5))
        coords[dup[1]] = coords[dup[0]]
    y = rng.standard_normal(n)
    nug = 1.0 / rng.uniform(0.3, 3.0, size=n) if case.wt else None
    nn = np.full((n, m), -1, dtype=np.int32)
    for i in range(1, n):
        dist = np.sqrt(np.sum((coords[:i] - coords[i]) ** 2, axis=1))
        order = np.argsort(dist, kind="stable")[:m]
        nn[i, :order.size] = order
    for arr in (coords, nn, y) + ((nug,) if nug is not None else ()):
        arr.setflags(write=False)
    return CaseData(coords, nn, y, nug, dup)


def checked_points(case, total=24):
    """Rows 0, 1, 2, m - 1, m, m + 1, 15, 16, 17, the duplicated pair, the last three rows, filled up to `total` with a seeded sample."""
    n, m = case.n, case.m
    pts = {0, 1, 2, m - 1, m, m + 1, 15, 16, 17, n - 3, n - 2, n - 1}
    dup = case_data(case).dup
    if dup:
        pts.update(dup)
    pts = {p for p in pts if 0 <= p < n}
    rng = np.random.default_rng(case.seed + 77)
    rest = [int(v) for v in rng.permutation(n) if int(v) not in pts]
    pts.update(rest[:max(0, total - len(pts))])
    return tuple(sorted(pts))


def covariance_sweep(d, a=8.0):
    """(a): points whose scaled distance rho = a dist to point 0 sweeps 0, 1e-12 .. 1e-3, 200 values across [0.01, 50], j ln2 / 256 and (j + 1/2) ln2 / 256 (+- 1 ulp)
    for j around 255 .. 257 and 511 .. 513 (the rint half-way points and the k & 255, k >> 8 boundaries), and 700, 745, 800 (underflow).  m = 1: every row i >= 1 has
    the single neighbour 0.  d = 1: the values are exact (a is a power of two); d = 2, 3: along a fixed oblique direction, to rounding.  -> (coords, nn)"""
    rho = [0.0] + list(np.logspace(-12, -3, 19)) + list(np.linspace(0.01, 50.0, 200))
    for j in (254, 255, 256, 257, 258, 510, 511, 512, 513, 514):
        for h in (0.0, 0.5):
            v = (j + h) * math.log(2.0) / 256.0
            rho += [np.nextafter(v, 0.0), v, np.nextafter(v, np.inf)]
    rho += [700.0, 745.0, 800.0]
    rho = np.asarray(rho)
    direction = {1: np.array([1.0]), 2: np.array([0.6, 0.8]), 3: np.array([2.0, 3.0, 6.0]) / 7.0}[d]
    coords = np.zeros((rho.size + 1, d))
    coords[1:] = (rho / a)[:, None] * direction[None, :]
    nn = np.zeros((rho.size + 1, 1), dtype=np.int32)
    nn[0, 0] = -1
    return coords, nn


# ---- one point ---------------------------------------------------------------------------------------------------------------------------------------------
def point_system(coords, nn_row, i, cov, var, a, gauss, nug, mutant=None):
    """The point's system in long double: dict with N, C, c, c0, dC, dc, nv (the rows' nuggets), nug_i and the scaled distances R (k x k), r (k)."""
    N = np.asarray([int(v) for v in nn_row if v >= 0], dtype=np.int64)
    if mutant == "last_dummy" and N.size >= 1:
        N = N[:-1]
    k = N.size
    Ncoord = N.copy()
    if mutant == "mirror" and k >= 32:
        Ncoord[16], Ncoord[31] = N[31], N[16]                  # rows 16 + j and 31 - j of slot 1 exchanged (j = 0): the mirrored-lane rule ignored
    coords = np.asarray(coords, dtype=np.float64).reshape(len(coords), -1)
    X = coords[Ncoord].astype(LD).reshape(k, coords.shape[1])
    xi = coords[i].astype(LD).reshape(1, coords.shape[1])
    R = LD(a) * _dist(X, X)
    r = LD(a) * _dist(X, xi)[:, 0]
    if mutant == "newton_missing":
        R = R * (1 + LD(D0)); r = r * (1 + LD(D0))
    third = LD(1) if mutant == "m25_third" else LD(1) / 3
    C, _, dC, _ = kern(cov, R, var, third)
    c, _, dc, _ = kern(cov, r, var, third)
    if k >= 1 and mutant == "entry_rel":
        c[0] *= 1 + LD(2e-13)            # one covariance entry: the point with its nearest neighbour (module docstring: resolution)
    if k >= 2 and mutant == "table_index":
        C[1, 0] *= LD(2) ** (LD(1) / 256); C[0, 1] = C[1, 0]
    if k == 1 and mutant == "table_index":
        c[0] *= LD(2) ** (LD(1) / 256)
    if nug is not None:
        src = N + 1 if mutant == "nugget_shift" else N          # (the nugget of row r taken from the record after it)
        nv = np.asarray(nug, dtype=np.float64)[np.minimum(src, len(nug) - 1)].astype(LD)
        nug_i = LD(nug[i])
        diag = LD(var) + nv
        c0 = LD(var) + nug_i
    elif gauss:
        nv = np.ones(k, dtype=LD); nug_i = LD(1)
        diag = np.full(k, LD(var) + 1); c0 = LD(var) + 1
    else:
        nv = np.zeros(k, dtype=LD); nug_i = LD(0)
        diag = np.full(k, LD(float(var)) if mutant == "no_jitter" else LD(float(var) * (1.0 + 1e-10)))    # the host's fp64 product
        c0 = LD(var)
    idx = np.arange(k)
    C[idx, idx] = diag
    dC[idx, idx] = 0
    return dict(N=N, k=k, C=C, c=c, c0=c0, dC=dC, dc=dc, nv=nv, nug_i=nug_i, R=R, r=r, weighted=nug is not None)


def point_values(S, yN, yi):
    """A, D, b, u and the seven terms of one point from its system, long double."""
    k = S["k"]
    yN = np.asarray(yN, dtype=np.float64).astype(LD); yi = LD(yi)
    if k:
        L = chol_ld(S["C"])
        Li = lower_inverse_ld(L)
        Cinv = Li.T @ Li
        A = Cinv @ S["c"]; b = Cinv @ yN
    else:
        Cinv = np.zeros((0, 0), dtype=LD); A = np.zeros(0, dtype=LD); b = np.zeros(0, dtype=LD)
    D = S["c0"] - A @ S["c"]
    u = yi - A @ yN
    nv = S["nv"]
    dDv = D - S["nug_i"] - np.sum(nv * A * A)
    ukv = -np.sum(nv * b * A)
    dCA = S["dC"] @ A
    dDr = A @ dCA - 2 * (A @ S["dc"])
    ukr = b @ dCA - b @ S["dc"]
    up = u / D
    terms = np.array([u * u / D, np.log(D) if D > 0 else LD("nan"), 0 if D > 0 else 1,
                      ukv * up - up * up * dDv / 2, dDv / (2 * D), ukr * up - up * up * dDr / 2, dDr / (2 * D)], dtype=LD)
    return dict(A=A, D=D, b=b, u=u, terms=terms, Cinv=Cinv, dDv=dDv, ukv=ukv, dDr=dDr, ukr=ukr, up=up, yN=yN, yi=yi)


def point_bounds(S, V, cov, var, g, c_r=C_R):
    """Bounds on A (k), D, u and the seven terms of one point: see the module docstring."""
    k = S["k"]
    gm = LD(gamma(g))
    A, b, D, u, yN, yi = np.abs(V["A"]), np.abs(V["b"]), V["D"], V["u"], np.abs(V["yN"]), abs(V["yi"])
    c0 = S["c0"]
    floor = LD(FLUSH) * LD(var)
    if k:
        Ci = np.abs(V["Cinv"])
        dg = np.sqrt(np.diag(S["C"]))
        excess = np.maximum(S["r"][:, None] + S["r"][None, :] - S["R"], 0)
        dR = LD(U) * (c_r * S["R"] + C_C * excess) + LD(R_FLOOR)
        dr = LD(U) * c_r * S["r"] + LD(R_FLOOR)
        third = LD(1) / 3
        K, K1, dK, dK1 = kern(cov, S["R"], var, third)
        kc, kc1, dkc, dkc1 = kern(cov, S["r"], var, third)
        E = C_A[cov] * U * K + K1 * dR + floor
        EdC = C_DK[cov] * U * np.abs(dK) + dK1 * dR + floor
        idx = np.arange(k)
        E[idx, idx] = 0; EdC[idx, idx] = 0
        E = E + gm * np.outer(dg, dg)
        e_c = C_A[cov] * U * kc + kc1 * dr + floor + gm * dg * np.sqrt(c0)
        e_dc = C_DK[cov] * U * np.abs(dkc) + dkc1 * dr + floor
        ynorm = np.sqrt(max(V["yN"] @ V["b"], LD(0)))
        e_y = gm * ynorm * dg
        bA = Ci @ (e_c + E @ A)
        bb = Ci @ (E @ b + e_y)
    else:
        E = EdC = np.zeros((0, 0), dtype=LD); e_c = e_dc = e_y = bA = bb = dg = np.zeros(0, dtype=LD); ynorm = LD(0)
    e0 = gm * c0
    bD = e0 + 2 * (A @ e_c) + A @ (E @ A)
    bu = bA @ yN + gamma(k + 1) * (yi + A @ yN) + A @ e_y + gm * (ynorm * np.sqrt(c0) + abs(u))
    aD = abs(D)
    quad = u * u / aD
    b_quad = 2 * abs(u) * bu / aD + u * u * bD / (D * D) + 3 * U * quad
    b_logdet = bD / aD
    # gradient terms
    nv = S["nv"]
    e_nv = LD(U) * (LD(var) + nv) if S["weighted"] else np.zeros(k, dtype=LD)
    adC, adc = np.abs(S["dC"]), np.abs(S["dc"])
    ns = k * (k + 1) // 2 + k + 4
    b_dDv = bD + 2 * np.sum(nv * A * bA) + np.sum(e_nv * A * A) + gamma(k + 4) * (aD + S["nug_i"] + np.sum(nv * A * A))
    b_ukv = np.sum(nv * (bb * A + b * bA)) + np.sum(e_nv * b * A) + gamma(k + 4) * np.sum(nv * b * A)
    adCA = adC @ A
    b_dDr = 2 * (bA @ adCA) + A @ (EdC @ A) + 2 * (bA @ adc) + 2 * (A @ e_dc) + gamma(ns) * (A @ adCA + 2 * (A @ adc))
    b_ukr = bb @ adCA + (b @ adC) @ bA + b @ (EdC @ A) + bb @ adc + b @ e_dc + gamma(ns) * (b @ adCA + b @ adc)
    up = abs(V["up"])
    b_up = bu / aD + abs(u) * bD / (D * D) + 2 * U * up

    def g1(uk, b_uk, dD, b_dD):
        return b_uk * up + abs(uk) * b_up + up * b_up * abs(dD) + up * up * b_dD / 2 + 4 * U * (abs(uk) * up + up * up * abs(dD) / 2)

    def g2(dD, b_dD):
        return (b_dD / aD + abs(dD) * bD / (D * D)) / 2 + 3 * U * abs(dD) / (2 * aD)
    terms = np.array([b_quad, b_logdet, 0, g1(V["ukv"], b_ukv, V["dDv"], b_dDv), g2(V["dDv"], b_dDv),
                      g1(V["ukr"], b_ukr, V["dDr"], b_dDr), g2(V["dDr"], b_dDr)], dtype=LD)
    return dict(A=bA, D=bD, u=bu, terms=terms)


Point = collections.namedtuple("Point", "i k A D u terms bA bD bu bterms")


@functools.lru_cache(maxsize=None)
def eval_point(case, i, mutant=None):
    """Values and bounds of point i of a case (cached: the three modes and the capped run of one case share one evaluation).  A mutant changes the values only;
    the bounds always belong to the unmutated model."""
    cd = case_data(case)
    S = point_system(cd.coords, cd.nn[i], i, case.cov, case.var, case.a, case.gauss, cd.nug, mutant)
    V = point_values(S, cd.y[S["N"]], cd.y[i])
    if mutant is None:
        g = g_big(case.m) if case.kind == "big" else g_point(case.mt)
        B = point_bounds(S, V, case.cov, case.var, g, C_R_ND if case.d > 3 else C_R)
        bA, bD, bu, bt = B["A"], B["D"], B["u"], B["terms"]
    else:
        bA = bD = bu = bt = None
    Afull = np.zeros(case.m, dtype=LD)
    Afull[:S["k"]] = V["A"]
    if bA is not None:
        bfull = np.zeros(case.m, dtype=LD); bfull[:S["k"]] = bA
        bA = bfull
    return Point(i, S["k"], Afull, V["D"], V["u"], V["terms"], bA, bD, bu, bt)


def sum_bounds(case, i0, i1, nworkers=None, nterms=7):
    """Sums of the seven terms over the points [i0, i1) and their bounds (module docstring: sums over a range of points)."""
    pts = [eval_point(case, i) for i in range(i0, i1)]
    vals = np.array([p.terms for p in pts], dtype=LD)
    bnds = np.array([p.bterms for p in pts], dtype=LD)
    npts = i1 - i0
    ngroups = (npts + 15) // 16
    nworkers = ngroups if nworkers is None else nworkers
    s = vals.sum(axis=0)
    bound = bnds.sum(axis=0) + gamma(npts + 16) * np.abs(vals).sum(axis=0)
    bound[1] += npts * U + 8 * U * (np.abs(vals[:, 1]).sum() + 23 * nworkers)
    return s[:nterms], bound[:nterms], np.abs(vals).sum(axis=0)[:nterms]


def ratio(err, bound):
    """largest |err| / bound (inf where the bound is 0 and the error is not)"""
    err = np.abs(np.atleast_1d(np.asarray(err, dtype=LD))); bound = np.atleast_1d(np.asarray(bound, dtype=LD))
    with np.errstate(divide="ignore", invalid="ignore"):
        q = np.where(bound > 0, err / np.where(bound > 0, bound, 1), np.where(err > 0, np.inf, 0.0))
    q = np.where(np.isnan(err), np.inf, q)
    return float(np.max(q)) if q.size else 0.0


# ---- which kernel instance a case launches (gpb_hip.cpp vecchia_launch, vecchia_kernels.hip launch_cov) -------------------------------------------------------
def instance_of(case, mode):
    """(MT, COV, D3, MODE, WT) of vecchia_point_kernel, or ("big", dk, COV, MODE, weights) of vecchia_point_big_kernel.  WT: args.nug != nullptr, or the run-time
    weighted gradient instance of 30 < MT <= 40 that serves both."""
    if case.m > 62 or case.d > 3:
        return ("big", 0 if case.d > 3 else (3 if case.d == 3 else 2), case.cov, mode, case.wt)
    mt = padded_mt(case.m)
    wt = case.wt or (mode == 2 and 30 < mt <= 40)
    return (mt, case.cov, case.d == 3, mode, wt)
