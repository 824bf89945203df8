"""Plain numpy / np.longdouble model of every kernel of the full-scale Vecchia ("VIF") family, gpboost_amd/csrc/vif_kernels.hip, with an a-priori bound next to every
value, the case tables of tests/test_zz_vif_kernels_gpu.py and mutants of the model.  CPU only, imports nothing from oracle/; tests/test_vif_kernel_ref.py checks this file.

The checks are LAYERED: every kernel is compared with a long-double evaluation of that kernel's operation on the inputs the device itself had (read back through
gpb_hip_vecchia_vif_get_matrix / _get_point_terms), so a bound belongs to one kernel and a failure names it.  u = 2^-53, gamma(t) = t u / (1 - t u).  Every bound below
was derived from the operation sequence of the kernel before any device run.

crosscov (vif_crosscov_kernel): C_ij = var k(a |x_i - ip_j|), dC_ij = d/d log a, column k = y (exact), columns beyond k and dC from k on exactly 0
    dist3: dx = fl(p - q) (1 u on dx, 2 u on dx^2), the product (1), at most two additions of positive terms (2): 5 u on d2, halved by the square root (2.5) and its own
    rounding (1): 3.5 u; r = fl(a dist) (1): 4.5 -> C_R = 5, |delta r| <= gamma(C_R) r, entering through the exact derivative |K'(r)|.
    e = fl(var exp(-r)): the device exp and one product.  The installed ROCm ships no text that states an ulp bound for the fp64 exp of its device library, so this is
    an ASSUMPTION, named here: at most 2 ulp = 4 u (EXP_U).  e: 5 u.
    Matern 0.5: e -> C_A = 5;  1.5: e (1 + r): the sum (1), the product (1) -> 7;  2.5: fma(r, fma(r, 1/3, 1), 1) e: the rounded 1/3 (weight <= 1: 1), two fma (2), the product (1) -> 9.
    dK: 0.5 -r e: 5 + 1 -> 6;  1.5 -(r r) e: 5 + 2 -> 7;  2.5 -r r (1 + r) e (1/3): 5 + four products + the sum + the rounded 1/3 -> 11.
    bound(C) = gamma(C_A) |K| + |K'(r)| gamma(C_R) r,  bound(dC) = gamma(C_DK) |dK| + |dK'(r)| gamma(C_R) r.   (r <= a sqrt(3) < 20: no underflow.)
product (vif_gemm_kernel): Out = In M, one fma chain of kq terms per entry (ascending over the 16-wide K steps): gamma(kq + 1) sum_l |In_il| |M_lj|; the accumulate form
    adds one rounding of the sum: + u (|Out_old| + sum |In| |M|).  M is zero outside its k x k block: columns >= k of every product are exactly 0.
spmm (vif_spmm_kernel): Q_ic = X_ic - sum_j A_ij X_nn(ij),c, one fma chain of k_i terms: gamma(k_i + 1) (|X_ic| + sum_j |A_ij| |X_nn(ij),c|).  The two-matrix form runs the
    same chain per matrix: bit for bit what the single-matrix form gives.
gram (vif_gram_kernel + vif_gram_sum_kernel): G_ab = sum_i Q_ia Q_ib / D_i.  Per row: 1 / D_i (1), its product with Q_ia (1), then one fma chain over the rows of a chunk,
    rows_per_chunk = ceil(ceil(n / nchunks) / 16) 16 with nchunks = vif_gram_chunks(n, kq) (restated: gram_chunks), then the chunks added in ascending order (nchunks):
    gamma(rows_per_chunk + 2 + nchunks) sum_i |Q_ia| |Q_ib| / |D_i|.  G is symmetric exactly (the transposed tile and, in a diagonal tile, the transposed entry are copies).
vec (vif_vec_kernel): v_i = (Q_ik - Q_i . w) / D_i, z_i = C_ik - C_i . w: 16 strided fma chains of ceil(k / 16) terms, a 4-step shuffle tree, one subtraction, one division:
    gamma(ceil(k / 16) + 6) (|Q_ik| + sum |Q_ic w_c|) / |D_i|   and   gamma(ceil(k / 16) + 5) (|C_ik| + sum |C_ic w_c|).
point_factor (vif_resid_factor_kernel, from the device's own V): S = rows (N, i) of V, G_S = S S', C_nn = K - G_S + I, c = K - G_S[., i], A = C_nn^-1 c,
    D = var + 1 - G_ii - A . c, u = y_i - A . y_N.  The perturbation model of tests/vecchia_point_ref.py (Higham, Accuracy and Stability of Numerical Algorithms, 2nd ed.,
    Thm 10.3 / 10.4 and (10.7)): the device factorises C_nn + dC and solves with c + dc,
        |dC_rc| <= eK_rc + eG_rc + u (|K_rc| + |G_rc|) + gamma(g) sqrt(C_rr C_cc)   (diagonal: no eK; var + 1 is exact for the parameters of the cases),
        |dc_r| likewise with sqrt(C_rr c0), |dc0| <= eG_ii + gamma(g) (var + 1 + G_ii),   c0 = var + 1 - G_ii,
    eK the bound of one covariance value (crosscov above; dist4 always adds three squares), eG_ab = gamma(kip + 4) |V_a| . |V_b|: the scalar path (NT = 0) is one fma chain of
    kip terms; v_mfma_f64_16x16x4_f64 adds four products to the accumulator per step in an order the ISA does not state: at most 4 roundings per step of 4 columns, the last
    step padded with zero columns -> kip + 3 roundings at most.  The count g:
        register form (NT > 0): right-looking Cholesky, entry (r, c) takes at most m fused updates, sqrt, the reciprocal 1 / sd and the product with it: m + 3; forward
        substitution: at most m fused terms, the reciprocal's product: m + 1; backward the same: m + 1; D and u: the products z z, the 6-step butterfly over the wavefront,
        two subtractions: 9.   G_REG(m) = 3 m + 14.
        LDS form (NT = 0): sqrt and a division per column: m + 2; forward m + 2 (reciprocal and product), backward m + 1 (division); the 128-slot tree (7 steps), the
        products, two subtractions: 10.   G_LDS(m) = 3 m + 15.
    |dA| <= Ci (e_c + E |A|), |dD| <= e0 + 2 |A|' e_c + |A|' E |A|, |du| as in vecchia_point_ref.py with the response row's backward error gamma(g) sqrt(y_N' C^-1 y_N) sqrt(C_cc).
    The three per-point partials of factor mode: log D, u^2 / D, [D <= 0] of the device's own D and u to 3 roundings (the device log: 1 ulp assumed = 2 u, within the 3).
point_grad (vif_resid_grad_kernel, from the device's own A, D, V, C, dC, Q, QdC, X1, V1, X2r, Hm, w, v, z): Atilde = (A_i, -1) over (N, i),
        h^0_a = sum_b K_ab Atilde_b + C_a . V1_i,   h^1_a = sum_b dK_ab Atilde_b + dC_a . X1_i + C_a . X2r_i,   g_a = C_a . Hm_i  (K without nugget),
        x^p = C_nn^-1 h^p[N],  dA^p = -x^p,  dD^p = A . h^p[N] - h^p_i,  kappa = Q_i . Hm_i,  and the twelve terms as tests/vif_harness.py NumpyDevice.grad_sums has them.
    Perturbations of h: the covariance part is lpr strided fma chains over k + 1 columns and their sum: eK_ab |Atilde_b| summed + gamma(k + 7) sum |K_ab| |Atilde_b|; the
    low-rank parts are 16 strided chains of ceil(kip / 16) columns with up to two fma per column, a 4-step tree and the final sum: gamma(2 ceil(kip / 16) + 6) x the sum of
    the absolute products.  x: |dx| <= Ci (e_h + E |x|) with E of point_factor (the same set-up code runs again).  Dot products over the neighbours go through a 7-step tree:
    gamma(9) x the absolute products; dD adds |A| . e_h + e_h_i; the terms are first order in these, each with gamma(count of its own operations) of its value.
Sums: out3 and sums12 against the long-double sum of the device's per-point terms.  reduce_partials_kernel (vecchia_aux_kernels.hip) gives each of 1024 threads a
    compensated chain over ceil(n / 1024) values (one value for n <= 1024: no rounding) and adds the threads in a 10-step tree: gamma(10) sum |term| for the sizes here;
    the check uses the looser gamma(n + 16) sum |term|.

Observed error / bound per class: DESIGN.md section 4.12 (printed by tests/test_zz_vif_kernels_gpu.py::test_zz_report_worst_ratios).
"""
import collections
import functools

import numpy as np

from tests.vecchia_point_ref import LD, U, chol_ld, gamma, kern, long_double_is_wider, lower_inverse_ld, ratio  # noqa: F401

F64 = np.float64
KC = 64                      # kVifKC: columns of V per staged chunk
EXP_U = 4.0                  # the device exp: 2 ulp assumed (module docstring)
C_R = 5.0
C_A = {0: EXP_U + 1, 1: EXP_U + 3, 2: EXP_U + 5}
C_DK = {0: EXP_U + 2, 1: EXP_U + 3, 2: EXP_U + 7}
PARAMS = ((3.0, 9.0), (7.5, 11.0))
MATRICES = ("C", "dC", "V", "Q", "QdC", "Hm", "X1", "V1", "X2r", "v", "z", "G")
TERM_NAMES = tuple("S%d%s" % (s + 1, "vr"[p]) for s in range(6) for p in range(2))


def g_reg(m):
    return 3 * m + 14


def g_lds(m):
    return 3 * m + 15


# ---- the launch logic of vif_kernels.hip / gpb_hip.cpp, restated -------------------------------------------------------------------------------------------------
def vif_kq(k):
    return (k + 1 + 7) // 8 * 8


def vif_tiles(m):
    return (m + 1 + 15) // 16 if m <= 62 else 0


def threads_of(m):
    return 64 if m <= 62 else 128


def staged_rows(m):
    nt = vif_tiles(m)
    return 16 * nt if nt > 0 else m + 1


def resid_lds_bytes(m, kq_grad):
    chunk, vecs = staged_rows(m) * (KC + 1), 5 * kq_grad
    return 8 * ((m + 1) * ((m + 1) | 1) + max(chunk, vecs))


def resid_lds_max():
    """vif_resid_lds_max: the 160 KiB of a workgroup minus the static arrays of the derivative kernel at T = 128"""
    return 160 * 1024 - (8 * (6 * 128 + 2 * 4 * 128 + 4) + 4 * 128 + 32)


def largest_admitted_m(k):
    """the largest m gpb_hip_vecchia_vif_set_inducing_points admits with k inducing points (m <= 126)"""
    return max(m for m in range(1, 127) if resid_lds_bytes(m, vif_kq(k)) <= resid_lds_max())


def vectors_exceed_chunk(m, k):
    return 5 * vif_kq(k) > staged_rows(m) * (KC + 1)


def gram_chunks(n, kq):
    nt = (kq + 63) // 64
    pairs = nt * (nt + 1) // 2
    return max(1, min((1024 + pairs - 1) // pairs, (n + 255) // 256))


def gram_rows_per_chunk(n, kq):
    c = gram_chunks(n, kq)
    return ((n + c - 1) // c + 15) // 16 * 16


def lpr_of(rows, T):
    return 4 if rows <= T // 4 else (2 if rows <= T // 2 else 1)


def lpr_edge_rows(m):
    """rows i < m whose k + 1 = i + 1 sits on either side of a change of lanes-per-row of the derivative kernel"""
    T = threads_of(m)
    return sorted(i for e in (T // 4, T // 2) for i in (e - 1, e) if i <= m)


# ---- cases -------------------------------------------------------------------------------------------------------------------------------------------------------
Case = collections.namedtuple("Case", "id kind n m k d cov var a seed")
NT_M = {1: (10, 10, 15), 2: (20, 31, 20), 3: (40, 47, 40), 4: (55, 62, 55), 0: (70, 63, 70)}      # m per covariance: the usual one, the tile edge, the usual one


def instance_cases():
    """One case per (COV, NT): 15 instances of vif_resid_factor_kernel<COV, T, NT> and of vif_resid_grad_kernel<COV, T, NT>; n = 331, k = 37, d in {1, 2, 3}."""
    out = []
    for nt in (1, 2, 3, 4, 0):
        for cov in range(3):
            idx = len(out)
            m = NT_M[nt][cov]
            var, a = PARAMS[(idx + cov) % 2]
            out.append(Case("cov%d-nt%d-m%d-d%d" % (cov, nt, m, 1 + idx % 3), "inst", 331, m, 37, 1 + idx % 3, cov, var, a, 7000 + idx))
    return out


# (m, k, n, cov, d): m = None: the largest admitted m
_EDGES = ((1, 1, 211, 0, 1), (15, 3, 211, 1, 2), (15, 7, 211, 2, 3), (16, 63, 211, 0, 2), (16, 64, 401, 1, 3), (16, 65, 211, 2, 2), (31, 130, 211, 0, 2), (32, 130, 211, 1, 3),
          (47, 63, 211, 2, 2), (48, 63, 211, 0, 3), (62, 65, 211, 1, 2), (63, 65, 211, 2, 3), (64, 65, 211, 0, 2), (None, 7, 211, 1, 2), (5, 256, 300, 0, 2),
          (30, 255, 600, 1, 3), (30, 256, 257, 2, 2), (30, 254, 255, 0, 3))


def edge_cases():
    """The tile, lane, chunk and kq edges (module docstring of tests/test_zz_vif_kernels_gpu.py).  The last case: one Gram chunk (n = 255 < 256) wants k < n, so k = 254."""
    out = []
    for idx, (m, k, n, cov, d) in enumerate(_EDGES):
        m = largest_admitted_m(k) if m is None else m
        var, a = PARAMS[idx % 2]
        out.append(Case("edge-m%d-k%d-n%d-cov%d-nt%d-d%d" % (m, k, n, cov, vif_tiles(m), d), "edge", n, m, k, d, cov, var, a, 7100 + idx))
    return out


def all_cases():
    return instance_cases() + edge_cases()


def case_by_id(prefix):
    hits = [c for c in all_cases() if c.id.startswith(prefix)]
    assert len(hits) == 1, (prefix, hits)
    return hits[0]


def inducing_lattice(k, d, rng):
    """k points on a jittered lattice in the unit cube: distinct cells, each point within the middle half of its cell"""
    g = 1
    while g ** d < k:
        g += 1
    cells = rng.permutation(g ** d)[:k]
    idx = np.stack(np.unravel_index(cells, (g,) * d), axis=1)
    return (idx + 0.5 + rng.uniform(-0.25, 0.25, size=(k, d))) / g


CaseData = collections.namedtuple("CaseData", "coords y ip nn")


def brute_force_neighbors(coords, m):
    n = coords.shape[0]
    nn = np.full((n, m), -1, dtype=np.int32)
    for i in range(1, n):
        dist = np.sqrt(np.sum((coords[:i] - coords[i]) ** 2, axis=1))
        order = np.argsort(dist, kind="stable")[:m]
        nn[i, :order.size] = order
    return nn


@functools.lru_cache(maxsize=None)
def case_data(case):
    """uniform coordinates, standard normal response, inducing points on a jittered lattice; nn: the m nearest predecessors by brute force (the GPU test replaces it by
    the device's own table)"""
    rng = np.random.default_rng(case.seed)
    coords = rng.uniform(size=(case.n, case.d))
    y = rng.standard_normal(case.n)
    ip = inducing_lattice(case.k, case.d, rng)
    nn = brute_force_neighbors(coords, case.m)
    for arr in (coords, y, ip, nn):
        arr.setflags(write=False)
    return CaseData(coords, y, ip, nn)


def checked_points(case, total=20):
    """rows 0, 1, m - 1, m, m + 1, the last row, the rows on either side of an lpr edge, filled up to `total` (<= 24) with a seeded sample"""
    n, m = case.n, case.m
    pts = {0, 1, m - 1, m, m + 1, n - 1} | set(lpr_edge_rows(m))
    pts = {p for p in pts if 0 <= p < n}
    rng = np.random.default_rng(case.seed + 77)
    rest = [int(v) for v in rng.permutation(n) if int(v) not in pts]
    pts.update(rest[:max(0, total - len(pts))])
    assert len(pts) <= 24
    return tuple(sorted(pts))


# ---- the host half (long double, rounded to double: what the test hands to the device) ---------------------------------------------------------------------------
def _dist(X, Y):
    return np.sqrt(np.sum((X[:, None, :] - Y[None, :, :]) ** 2, axis=2))


def _sym(M):
    return np.ascontiguousarray(np.tril(M) + np.tril(M, -1).T)


def sigma_m(ip, cov, var, a):
    """(Sigma_m, d Sigma_m / d log a) of the inducing points, un-jittered, long double"""
    P = np.asarray(ip, dtype=F64).astype(LD)
    K, _, dK, _ = kern(cov, LD(a) * _dist(P, P), var)
    return K, dK


def spd_inverse_ld(S):
    Li = lower_inverse_ld(chol_ld(S))
    return Li.T @ Li


def whitening(case, ip):
    """Linv = chol(Sigma_m with its diagonal x (1 + 1e-6))^-1, rounded to double"""
    Sm, _ = sigma_m(ip, case.cov, case.var, case.a)
    Sm = Sm.copy()
    idx = np.arange(case.k)
    Sm[idx, idx] *= LD(1) + LD(1e-6)
    return np.tril(lower_inverse_ld(chol_ld(Sm))).astype(F64)


def grad_inputs(case, ip, G):
    """Winv, Si, N0, negMp1 (k x k, symmetric) and w of gpb_hip_vecchia_vif_grad_sums from the device's own Gram matrix G (at least (k + 1) x (k + 1)), rounded to double"""
    k = case.k
    Sm0, dSm1 = sigma_m(ip, case.cov, case.var, case.a)
    Sm = Sm0.copy()
    idx = np.arange(k)
    Sm[idx, idx] *= LD(1) + LD(1e-6)
    Gl = np.asarray(G, dtype=F64).astype(LD)
    Winv = spd_inverse_ld(Sm + Gl[:k, :k])
    Si = spd_inverse_ld(Sm)
    N0 = 2 * Si - Si @ Sm0 @ Si
    negMp1 = -(Si @ dSm1 @ Si)
    w = Winv @ Gl[:k, k]
    return tuple(_sym(M.astype(F64)) for M in (Winv, Si, N0, negMp1)) + (w.astype(F64),)


def pad_kq(M, k, kq, transpose=False):
    out = np.zeros((kq, kq))
    out[:k, :k] = np.asarray(M).T if transpose else np.asarray(M)
    return out


# ---- the kernels: value (in dtype dt) and bound ------------------------------------------------------------------------------------------------------------------
def _kern_dt(cov, r, var, dt):
    """(K, dK) in dt; long double: kern(); plain double: the device's own operation sequence"""
    if dt is LD:
        K, _, dK, _ = kern(cov, r, var)
        return K, dK
    e = var * np.exp(-r)
    if cov == 0:
        return e, -r * e
    if cov == 1:
        return e * (1.0 + r), -r * r * e
    return e * (r * (r * (1.0 / 3.0) + 1.0) + 1.0), -r * r * (1.0 + r) * e * (1.0 / 3.0)


def kern_bounds(cov, r, var):
    """bounds of one covariance value and of its derivative wrt log a at the scaled distances r (long double)"""
    K, K1, dK, dK1 = kern(cov, r, var)
    dr = gamma(C_R) * np.asarray(r, dtype=LD)
    return gamma(C_A[cov]) * np.abs(K) + K1 * dr, gamma(C_DK[cov]) * np.abs(dK) + dK1 * dr


def crosscov(coords, y, ip, cov, var, a, dt=LD):
    """-> C, dC (n x kq) in dt"""
    n = coords.shape[0]
    k = ip.shape[0]
    kq = vif_kq(k)
    r = dt(a) * _dist(np.asarray(coords, dtype=F64).astype(dt), np.asarray(ip, dtype=F64).astype(dt))
    K, dK = _kern_dt(cov, r, var, dt)
    C = np.zeros((n, kq), dtype=dt)
    dC = np.zeros((n, kq), dtype=dt)
    C[:, :k] = K
    C[:, k] = np.asarray(y, dtype=F64).astype(dt)
    dC[:, :k] = dK
    return C, dC


def crosscov_bounds(coords, ip, cov, var, a):
    n, k = coords.shape[0], ip.shape[0]
    r = LD(a) * _dist(np.asarray(coords, dtype=F64).astype(LD), np.asarray(ip, dtype=F64).astype(LD))
    bK, bdK = kern_bounds(cov, r, var)
    bC = np.zeros((n, vif_kq(k)), dtype=LD)
    bdC = np.zeros_like(bC)
    bC[:, :k] = bK
    bdC[:, :k] = bdK
    return bC, bdC


def product(In, M, dt=LD, mutant=None, k=None):
    M = np.asarray(M, dtype=F64)
    if mutant == "response_leak":                      # row k of M (what the response column multiplies) not zero
        M = M.copy()
        M[k, :k] = M[0, :k]
    return np.asarray(In, dtype=F64).astype(dt) @ M.astype(dt)


def product_bound(In, M):
    return gamma(In.shape[1] + 1) * (np.abs(In) @ np.abs(M))


def product_acc(Old, In, M, dt=LD, mutant=None):
    P = product(In, M, dt)
    return P if mutant == "gemm_acc_overwrites" else np.asarray(Old, dtype=F64).astype(dt) + P


def product_acc_bound(Old, In, M):
    s = np.abs(In) @ np.abs(M)
    return gamma(In.shape[1] + 1) * s + U * (np.abs(Old) + s)


def spmm(A, nn, X, dt=LD, mutant=None):
    X = np.asarray(X, dtype=F64).astype(dt)
    out = X.copy()
    for i in range(nn.shape[0]):
        idx = nn[i][nn[i] >= 0]
        if mutant == "spmm_stop_early":
            idx = idx[:-1]
        if idx.size:
            out[i] -= np.asarray(A[i, :idx.size], dtype=F64).astype(dt) @ X[idx]
    return out


def spmm_bound(A, nn, X):
    X = np.abs(np.asarray(X, dtype=F64))
    out = np.empty_like(X)
    for i in range(nn.shape[0]):
        idx = nn[i][nn[i] >= 0]
        out[i] = gamma(idx.size + 1) * (X[i] + (np.abs(A[i, :idx.size]) @ X[idx] if idx.size else 0.0))
    return out


def gram(Q, D, dt=LD, mutant=None):
    Q = np.asarray(Q, dtype=F64).astype(dt)
    G = Q.T @ (Q / np.asarray(D, dtype=F64).astype(dt)[:, None])
    if mutant == "gram_transpose_missing":             # the tile above the diagonal of tiles not written
        t = np.arange(G.shape[0]) // 64
        G = np.where(t[:, None] < t[None, :], 0, G)
    return G


def gram_bound(Q, D):
    n, kq = Q.shape
    Qa = np.abs(np.asarray(Q, dtype=F64))
    return gamma(gram_rows_per_chunk(n, kq) + 2 + gram_chunks(n, kq)) * (Qa.T @ (Qa / np.abs(D)[:, None]))


def vec(Q, C, D, w, k, dt=LD):
    Q, C, D, w = (np.asarray(x, dtype=F64).astype(dt) for x in (Q, C, D, w))
    return (Q[:, k] - Q[:, :k] @ w[:k]) / D, C[:, k] - C[:, :k] @ w[:k]


def vec_bounds(Q, C, D, w, k):
    t = (k + 15) // 16
    Q, C, w = np.abs(Q), np.abs(C), np.abs(w)
    return gamma(t + 6) * (Q[:, k] + Q[:, :k] @ w[:k]) / np.abs(D), gamma(t + 5) * (C[:, k] + C[:, :k] @ w[:k])


# ---- one point ---------------------------------------------------------------------------------------------------------------------------------------------------
def _gram_columns(kip, mutant):
    """the columns of V that enter G_S"""
    c0 = (kip - 1) // KC * KC                      # first column of the last chunk
    if mutant == "gram_last_col":
        return kip - 1
    if mutant == "gram_k4_tail":
        return c0 + 4 * ((kip - c0) // 4)
    return kip


def _solve(Cm, B, dt):
    """C^-1 B (B: k x q) and |C^-1|"""
    if dt is LD:
        Ci = spd_inverse_ld(Cm)
        return Ci @ B, np.abs(Ci)
    return np.linalg.solve(Cm, B), None


def point_system(case, data, i, V, dt=LD, mutant=None):
    """The point's system from the staged rows of the device's own V -> dict(N, k, K (k + 1 square, no nugget), dK, Cnn, c, c0, G, R (scaled distances))"""
    N = np.asarray([int(v) for v in data.nn[i] if v >= 0], dtype=np.int64)
    k = N.size
    al = np.concatenate([N, [i]])
    X = np.zeros((k + 1, 3), dtype=dt)
    X[:, :case.d] = np.asarray(data.coords, dtype=F64)[al].astype(dt)
    R = dt(case.a) * _dist(X, X)
    K, dK = _kern_dt(case.cov, R, case.var, dt)
    K = np.array(K, dtype=dt)
    dK = np.array(dK, dtype=dt)
    idx = np.arange(k + 1)
    K[idx, idx] = dt(case.var)
    dK[idx, idx] = 0
    S = np.asarray(V, dtype=F64)[al][:, :_gram_columns(case.k, mutant)].astype(dt)
    if mutant == "point_row_zero":
        S[k] = 0
    G = S @ S.T
    Cnn = K[:k, :k] - G[:k, :k]
    if mutant == "diag_no_G":
        Cnn[idx[:k], idx[:k]] = dt(case.var)
    Cnn[idx[:k], idx[:k]] += 1
    c = K[:k, k] - G[:k, k]
    c0 = dt(case.var) + 1 - G[k, k]
    return dict(N=N, al=al, k=k, K=K, dK=dK, Cnn=Cnn, c=c, c0=c0, G=G, R=R, S=S)


def point_factor(case, data, i, V, dt=LD, mutant=None):
    """A (m), D, u of point i in dt"""
    P = point_system(case, data, i, V, dt, mutant)
    k = P["k"]
    yN = np.asarray(data.y, dtype=F64)[P["N"]].astype(dt)
    yi = dt(data.y[i])
    A = np.zeros(case.m, dtype=dt)
    if k:
        sol, Ci = _solve(P["Cnn"], np.stack([P["c"], yN], axis=1), dt)
        A[:k] = sol[:, 0]
        P["b"], P["Ci"] = sol[:, 1], Ci
    D = P["c0"] - A[:k] @ P["c"]
    u = yi - A[:k] @ yN
    P.update(A=A, D=D, u=u, yN=yN, yi=yi)
    return P


def point_perturbation(case, P):
    """E (k x k), e_c (k), e0 of the module docstring for a point_system evaluated in long double"""
    k, m = P["k"], case.m
    gm = LD(gamma(g_reg(m) if vif_tiles(m) > 0 else g_lds(m)))
    Sa = np.abs(P["S"])
    eG = gamma(case.k + 4) * (Sa @ Sa.T)
    bK, bdK = kern_bounds(case.cov, P["R"], case.var)
    idx = np.arange(k + 1)
    Ka, Ga = np.abs(P["K"]), np.abs(P["G"])
    full = bK + eG + U * (Ka + Ga)
    full[idx, idx] -= bK[idx, idx]                     # the diagonal of C_nn is the constant var + 1, not a covariance evaluation (the derivative kernel does evaluate it)
    dg = np.sqrt(np.diag(P["Cnn"])) if k else np.zeros(0, dtype=LD)
    c0 = P["c0"]
    E = full[:k, :k] + gm * np.outer(dg, dg)
    e_c = full[:k, k] + gm * dg * np.sqrt(c0)
    e0 = eG[k, k] + gm * (LD(case.var) + 1 + Ga[k, k])
    return dict(E=E, e_c=e_c, e0=e0, gm=gm, dg=dg, bK=bK, bdK=bdK)


def point_factor_bounds(case, P):
    """bounds on A (m), D, u of a long-double point_factor"""
    k = P["k"]
    pert = point_perturbation(case, P)
    gm, dg, c0 = pert["gm"], pert["dg"], P["c0"]
    A, yN, yi, u = np.abs(P["A"][:k]), np.abs(P["yN"]), abs(P["yi"]), P["u"]
    bA = np.zeros(case.m, dtype=LD)
    if k:
        ynorm = np.sqrt(max(P["yN"] @ P["b"], LD(0)))
        e_y = gm * ynorm * dg
        bA[:k] = P["Ci"] @ (pert["e_c"] + pert["E"] @ A)
    else:
        ynorm, e_y = LD(0), np.zeros(0, dtype=LD)
    bD = pert["e0"] + 2 * (A @ pert["e_c"]) + A @ (pert["E"] @ A)
    bu = bA[:k] @ yN + gamma(k + 1) * (yi + A @ yN) + A @ e_y + gm * (ynorm * np.sqrt(c0) + abs(u))
    return dict(A=bA, D=bD, u=bu, pert=pert)


def point_grad(case, data, i, dev, dt=LD, mutant=None, bounds=True):
    """dA (2 x m), dD (2), the twelve terms of point i in dt from the device's own arrays (dev: dict by name; A, D, V and the matrices of MATRICES, w);
    dt = long double: also the bounds (bdA, bdD, bterms)"""
    P = point_system(case, data, i, dev["V"], dt)
    k, m, kip = P["k"], case.m, case.k
    N, al = P["N"], P["al"]
    f = lambda name, rows: np.asarray(dev[name], dtype=F64)[rows].astype(dt)
    A = f("A", i)[:k]
    At = np.concatenate([A, [dt(-1)]])
    Cal, dCal = f("C", al)[:, :kip], f("dC", al)[:, :kip]
    X1, V1, X2r, Hm, Qi, QdCi = (f(name, i)[:kip] for name in ("X1", "V1", "X2r", "Hm", "Q", "QdC"))
    w = np.asarray(dev["w"], dtype=F64).astype(dt)[:kip]
    Di, vi = dt(dev["D"][i]), dt(dev["v"][i])
    zN = f("z", N)
    K0 = P["dK"] if mutant == "dK_for_K" else P["K"]
    At_k = At
    if mutant == "lpr_last_sub":                       # the partial sum of the last of the lpr lanes of a row not added
        lpr = lpr_of(k + 1, threads_of(m))
        At_k = np.where(np.arange(k + 1) % lpr == lpr - 1, 0, At) if lpr > 1 else At
    h = [K0 @ At_k + Cal @ V1, P["dK"] @ At_k + dCal @ X1 + Cal @ X2r]
    g = Cal[:k] @ Hm
    if k:
        sol, Ci = _solve(P["Cnn"], np.stack([h[0][:k], h[1][:k]], axis=1), dt)
    else:
        sol, Ci = np.zeros((0, 2), dtype=dt), np.zeros((0, 0), dtype=dt)
    kappa, d_hm, q_w, d_w = Qi @ Hm, QdCi @ Hm, Qi @ w, QdCi @ w
    dA = np.zeros((2, m), dtype=dt)
    dD = np.zeros(2, dtype=dt)
    T = np.zeros(12, dtype=dt)
    tot_z, tot_g = np.zeros(2, dtype=dt), np.zeros(2, dtype=dt)
    for p in range(2):
        x = sol[:, p]
        dA[p, :k] = -x
        dD[p] = A @ h[p][:k] - h[p][k]
        tot_z[p], tot_g[p] = x @ zN, x @ g
        T[0 + p] = dD[p] / Di
        T[2 + p] = 2 * tot_z[p] * vi - vi * vi * dD[p]
        T[4 + p] = tot_g[p] / Di
        T[6 + p] = dD[p] * kappa / (Di * Di)
    T[8], T[9] = kappa / Di, d_hm / Di
    T[10], T[11] = vi * q_w, vi * d_w
    out = dict(k=k, dA=dA, dD=dD, terms=T)
    if dt is not LD or mutant is not None or not bounds:
        return out
    # ---- bounds ----
    pert = point_perturbation(case, P)
    gk, gh, g9 = gamma(k + 7), gamma(2 * ((kip + 15) // 16) + 6), gamma(9)
    aAt, aC, adC = np.abs(At), np.abs(Cal), np.abs(dCal)
    e_h = [pert["bK"] @ aAt + gk * (np.abs(P["K"]) @ aAt) + gh * (aC @ np.abs(V1)),
           pert["bdK"] @ aAt + gk * (np.abs(P["dK"]) @ aAt) + gh * (adC @ np.abs(X1) + aC @ np.abs(X2r))]
    e_g = gh * (aC[:k] @ np.abs(Hm))
    b_kappa, b_dhm = gh * (np.abs(Qi) @ np.abs(Hm)), gh * (np.abs(QdCi) @ np.abs(Hm))
    b_qw, b_dw = gh * (np.abs(Qi) @ np.abs(w)), gh * (np.abs(QdCi) @ np.abs(w))
    aA, aD, av = np.abs(A), abs(Di), abs(vi)
    bdA = np.zeros((2, m), dtype=LD)
    bdD = np.zeros(2, dtype=LD)
    bT = np.zeros(12, dtype=LD)
    for p in range(2):
        x = np.abs(sol[:, p])
        bx = Ci @ (e_h[p][:k] + pert["E"] @ x) if k else np.zeros(0, dtype=LD)
        bdA[p, :k] = bx
        bdD[p] = aA @ e_h[p][:k] + e_h[p][k] + gamma(k + 9) * (aA @ np.abs(h[p][:k]) + abs(h[p][k]))
        b_tz = bx @ np.abs(zN) + g9 * (x @ np.abs(zN))
        b_tg = bx @ np.abs(g) + x @ e_g + g9 * (x @ np.abs(g))
        bT[0 + p] = bdD[p] / aD + gamma(2) * abs(T[0 + p])
        bT[2 + p] = 2 * av * b_tz + av * av * bdD[p] + gamma(4) * (2 * abs(tot_z[p]) * av + av * av * abs(dD[p]))
        bT[4 + p] = b_tg / aD + gamma(2) * abs(T[4 + p])
        bT[6 + p] = (bdD[p] * abs(kappa) + abs(dD[p]) * b_kappa) / (aD * aD) + gamma(5) * abs(T[6 + p])      # 1 / D enters twice (2), three products
    bT[8], bT[9] = b_kappa / aD + gamma(2) * abs(T[8]), b_dhm / aD + gamma(2) * abs(T[9])
    bT[10], bT[11] = av * b_qw + gamma(1) * abs(T[10]), av * b_dw + gamma(1) * abs(T[11])
    out.update(bdA=bdA, bdD=bdD, bterms=bT)
    return out


# ---- the whole family in plain double: what a correct device would hand back, one rounding model apart ------------------------------------------------------------
def double_device(case, data):
    """Every buffer of the two device passes, each kernel evaluated in plain double on the outputs of the one before -> dict by the names the GPU test reads back"""
    n, m, k = case.n, case.m, case.k
    kq = vif_kq(k)
    dev = dict(Linv=whitening(case, data.ip))
    dev["C"], dev["dC"] = crosscov(data.coords, data.y, data.ip, case.cov, case.var, case.a, F64)
    dev["M_Linv"] = pad_kq(dev["Linv"], k, kq, transpose=True)
    dev["V"] = product(dev["C"], dev["M_Linv"], F64)
    A, D, u = np.zeros((n, m)), np.empty(n), np.empty(n)
    for i in range(n):
        P = point_factor(case, data, i, dev["V"], F64)
        A[i], D[i], u[i] = P["A"], P["D"], P["u"]
    dev.update(A=A, D=D, u=u, part3=np.stack([np.log(D), u * u / D, (D <= 0).astype(F64)]))
    dev["Q"], dev["QdC"] = spmm(A, data.nn, dev["C"], F64), spmm(A, data.nn, dev["dC"], F64)
    dev["G"] = _sym(gram(dev["Q"], D, F64))
    dev["out3"] = np.array([dev["part3"][1].sum(), dev["part3"][0].sum(), dev["part3"][2].sum()])
    add_grad_pass(case, data, dev, lambda d: _double_grad_pass(case, data, d))
    return dev


def add_grad_pass(case, data, dev, run):
    """the host's k x k inputs of the gradient pass from dev's own G, then run(dev) fills the buffers of that pass"""
    k, kq = case.k, vif_kq(case.k)
    Winv, Si, N0, negMp1, w = grad_inputs(case, data.ip, dev["G"])
    wq = np.zeros(kq)
    wq[:k] = w
    dev.update(Winv=Winv, Si=Si, N0=N0, negMp1=negMp1, w=wq, M_Winv=pad_kq(Winv, k, kq), M_Si=pad_kq(Si, k, kq), M_N0=pad_kq(N0, k, kq), M_negMp1=pad_kq(negMp1, k, kq))
    run(dev)


def _double_grad_pass(case, data, dev):
    n, m, k = case.n, case.m, case.k
    dev["Hm"], dev["X1"], dev["V1"] = (product(dev["Q"], dev[M], F64) for M in ("M_Winv", "M_Si", "M_N0"))
    dev["X2r_first"] = product(dev["QdC"], dev["M_Si"], F64)
    dev["X2r"] = product_acc(dev["X2r_first"], dev["Q"], dev["M_negMp1"], F64)
    dev["v"], dev["z"] = vec(dev["Q"], dev["C"], dev["D"], dev["w"], k, F64)
    dA, dD, T = np.zeros((2, n, m)), np.zeros((2, n)), np.zeros((12, n))
    for i in range(n):
        g = point_grad(case, data, i, dev, F64)
        dA[:, i], dD[:, i], T[:, i] = g["dA"], g["dD"], g["terms"]
    dev.update(dA=dA, dD=dD, part12=T, sums12=T.sum(axis=1))


# ---- the checks: a device's buffers against the long-double model of each kernel on that device's own inputs ----------------------------------------------------
class Findings(object):
    """largest error / bound per (kernel, quantity) and the exact conditions that failed"""

    def __init__(self):
        self.worst, self.failed, self.bad_bounds, self.largest_bound = {}, [], [], {}

    def note(self, kernel, what, err, bound, where=None):
        b = np.atleast_1d(np.asarray(bound, dtype=LD))
        if not (np.all(np.isfinite(b)) and np.all(b >= 0)):
            self.bad_bounds.append((kernel, what, where))
        self.largest_bound[(kernel, what)] = max(self.largest_bound.get((kernel, what), 0.0), float(np.max(b)) if b.size else 0.0)
        q = ratio(err, bound)
        if q >= self.worst.get((kernel, what), (-1.0, None))[0]:
            self.worst[(kernel, what)] = (q, where)
        return q

    def exact(self, ok, message):
        if not ok:
            self.failed.append(message)

    def largest(self):
        return max([v[0] for v in self.worst.values()] or [0.0])

    def ok(self):
        return not self.failed and self.largest() <= 1.0

    def report(self):
        return {"%s %s" % kw: v for kw, v in self.worst.items() if v[0] > 1.0}, self.failed


def _ld(x):
    return np.asarray(x, dtype=F64).astype(LD)


def check_crosscov(case, data, dev, F=None):
    F = F or Findings()
    k = case.k
    C, dC = crosscov(data.coords, data.y, data.ip, case.cov, case.var, case.a)
    bC, bdC = crosscov_bounds(data.coords, data.ip, case.cov, case.var, case.a)
    F.note("crosscov", "C", _ld(dev["C"])[:, :k] - C[:, :k], bC[:, :k])
    F.note("crosscov", "dC", _ld(dev["dC"])[:, :k] - dC[:, :k], bdC[:, :k])
    F.exact(np.array_equal(dev["C"][:, k], data.y), "crosscov: column k of C is not the response")
    F.exact(not np.any(dev["C"][:, k + 1:]) and not np.any(dev["dC"][:, k:]), "crosscov: columns beyond k are not zero")
    if "C_plain" in dev:
        F.exact(np.array_equal(dev["C_plain"], dev["C"]), "crosscov: C differs between the forms with and without dC")
    return F


def _check_product(F, case, dev, out, In, M, old=None):
    k = case.k
    if old is None:
        val, bnd = product(dev[In], dev[M]), product_bound(dev[In], dev[M])
    else:
        val, bnd = product_acc(dev[old], dev[In], dev[M]), product_acc_bound(dev[old], dev[In], dev[M])
    F.note("gemm", out, _ld(dev[out]) - val, bnd)
    F.exact(not np.any(dev[out][:, k:]), "gemm: columns >= k of %s are not zero" % out)


def check_gemm_factor(case, data, dev, F=None):
    F = F or Findings()
    _check_product(F, case, dev, "V", "C", "M_Linv")
    return F


def check_gemm_grad(case, data, dev, F=None):
    F = F or Findings()
    for out, M in (("Hm", "M_Winv"), ("X1", "M_Si"), ("V1", "M_N0")):
        _check_product(F, case, dev, out, "Q", M)
    # the device overwrites X2r in place: its first form is the product (B dC) Si, known to within its own bound; the accumulate form is checked on the model's value of it
    first = product(dev["QdC"], dev["M_Si"])
    b_first = product_bound(dev["QdC"], dev["M_Si"])
    s = np.abs(dev["Q"]) @ np.abs(dev["M_negMp1"])
    val = first + product(dev["Q"], dev["M_negMp1"])
    bnd = b_first + gamma(vif_kq(case.k) + 1) * s + U * (np.abs(first.astype(F64)) + b_first.astype(F64) + s)
    F.note("gemm", "X2r", _ld(dev["X2r"]) - val, bnd)
    F.exact(not np.any(dev["X2r"][:, case.k:]), "gemm: columns >= k of X2r are not zero")
    return F


def check_factor(case, data, dev, F=None):
    F = F or Findings()
    for i in checked_points(case):
        P = point_factor(case, data, i, dev["V"])
        B = point_factor_bounds(case, P)
        F.note("resid_factor", "A", _ld(dev["A"][i]) - P["A"], B["A"], i)
        F.note("resid_factor", "D", LD(dev["D"][i]) - P["D"], B["D"], i)
        F.note("resid_factor", "u", LD(dev["u"][i]) - P["u"], B["u"], i)
    F.exact(not np.any(dev["A"][data.nn < 0]), "resid_factor: A is not zero at the -1 positions")
    D, u = _ld(dev["D"]), _ld(dev["u"])
    F.note("resid_factor", "log D", _ld(dev["part3"][0]) - np.log(D), gamma(3) * np.abs(np.log(D)))
    F.note("resid_factor", "u^2 / D", _ld(dev["part3"][1]) - u * u / D, gamma(3) * np.abs(u * u / D))
    F.exact(np.array_equal(dev["part3"][2], (dev["D"] <= 0).astype(F64)), "resid_factor: the [D <= 0] partial")
    for j, q in enumerate((1, 0, 2)):                   # out3 = {quad, logdet, bad}
        t = _ld(dev["part3"][q])
        F.note("reduce", "out3", LD(dev["out3"][j]) - t.sum(), gamma(case.n + 16) * np.abs(t).sum())
    return F


def check_spmm(case, data, dev, F=None):
    F = F or Findings()
    for out, X in (("Q", "C"), ("QdC", "dC")):
        F.note("spmm", out, _ld(dev[out]) - spmm(dev["A"], data.nn, dev[X]), spmm_bound(dev["A"], data.nn, dev[X]))
    F.exact(not np.any(dev["Q"][:, case.k + 1:]) and not np.any(dev["QdC"][:, case.k:]), "spmm: the zero columns are not zero")
    if "Q_plain" in dev:
        F.exact(np.array_equal(dev["Q_plain"], dev["Q"]), "spmm: Q of the two-matrix form differs from the single-matrix form")
    return F


def check_gram(case, data, dev, F=None):
    F = F or Findings()
    kq = vif_kq(case.k)
    G = dev["G"]
    F.note("gram", "G", _ld(G) - gram(dev["Q"], dev["D"])[:G.shape[0], :G.shape[1]], gram_bound(dev["Q"], dev["D"])[:G.shape[0], :G.shape[1]])
    F.exact(np.array_equal(G, G.T), "gram: G is not symmetric")
    if G.shape[0] == kq:
        F.exact(not np.any(G[case.k + 1:]) and not np.any(G[:, case.k + 1:]), "gram: rows / columns beyond k are not zero")
    return F


def check_vec(case, data, dev, F=None):
    F = F or Findings()
    v, z = vec(dev["Q"], dev["C"], dev["D"], dev["w"], case.k)
    bv, bz = vec_bounds(dev["Q"], dev["C"], dev["D"], dev["w"], case.k)
    F.note("vec", "v", _ld(dev["v"]) - v, bv)
    F.note("vec", "z", _ld(dev["z"]) - z, bz)
    return F


def check_grad(case, data, dev, F=None):
    F = F or Findings()
    for i in checked_points(case):
        g = point_grad(case, data, i, dev)
        F.note("resid_grad", "dA", _ld(dev["dA"][:, i]) - g["dA"], g["bdA"], i)
        F.note("resid_grad", "dD", _ld(dev["dD"][:, i]) - g["dD"], g["bdD"], i)
        for q in range(12):
            F.note("resid_grad", TERM_NAMES[q], LD(dev["part12"][q, i]) - g["terms"][q], g["bterms"][q], i)
    F.exact(not np.any(dev["dA"][:, data.nn < 0]), "resid_grad: dA is not zero at the -1 positions")
    for q in range(12):
        t = _ld(dev["part12"][q])
        F.note("reduce", "sums12", LD(dev["sums12"][q]) - t.sum(), gamma(case.n + 16) * np.abs(t).sum())
    return F


CHECKS = (check_crosscov, check_gemm_factor, check_factor, check_spmm, check_gram, check_gemm_grad, check_vec, check_grad)


# ---- mutants: one-line wrong variants a subtly wrong kernel would compute; each with the case designed for it ---------------------------------------------------
MUTANTS = {"gram_last_col": "edge-m16-k65-", "gram_k4_tail": "edge-m47-k63-", "point_row_zero": "edge-m31-k130-", "diag_no_G": "cov1-nt2-", "response_leak": "edge-m15-k7-",
           "spmm_stop_early": "edge-m16-k64-", "dK_for_K": "cov2-nt3-", "lpr_last_sub": "edge-m62-k65-", "gram_transpose_missing": "edge-m16-k64-",
           "gemm_acc_overwrites": "cov0-nt1-"}


def mutant_excess(mutant, dev=None):
    """largest |mutated model - model| / bound over the checked entries of the mutant's case (dev: a double_device of that case)"""
    case = case_by_id(MUTANTS[mutant])
    data = case_data(case)
    dev = dev or double_device(case, data)
    if mutant in ("gram_last_col", "gram_k4_tail", "point_row_zero", "diag_no_G"):
        worst = 0.0
        for i in checked_points(case):
            P, Pm = point_factor(case, data, i, dev["V"]), point_factor(case, data, i, dev["V"], mutant=mutant)
            B = point_factor_bounds(case, P)
            worst = max(worst, ratio(Pm["A"] - P["A"], B["A"]), ratio(Pm["D"] - P["D"], B["D"]), ratio(Pm["u"] - P["u"], B["u"]))
        return worst
    if mutant in ("dK_for_K", "lpr_last_sub"):
        worst = 0.0
        for i in checked_points(case):
            g, gm = point_grad(case, data, i, dev), point_grad(case, data, i, dev, mutant=mutant)
            worst = max(worst, ratio(gm["dA"] - g["dA"], g["bdA"]), ratio(gm["dD"] - g["dD"], g["bdD"]), ratio(gm["terms"] - g["terms"], g["bterms"]))
        return worst
    if mutant == "response_leak":
        return ratio(product(dev["C"], dev["M_Linv"], mutant=mutant, k=case.k) - product(dev["C"], dev["M_Linv"]), product_bound(dev["C"], dev["M_Linv"]))
    if mutant == "spmm_stop_early":
        return ratio(spmm(dev["A"], data.nn, dev["C"], mutant=mutant) - spmm(dev["A"], data.nn, dev["C"]), spmm_bound(dev["A"], data.nn, dev["C"]))
    if mutant == "gram_transpose_missing":
        return ratio(gram(dev["Q"], dev["D"], mutant=mutant) - gram(dev["Q"], dev["D"]), gram_bound(dev["Q"], dev["D"]))
    if mutant == "gemm_acc_overwrites":
        args = (dev["X2r_first"], dev["Q"], dev["M_negMp1"])
        return ratio(product_acc(*args, mutant=mutant) - product_acc(*args), product_acc_bound(*args))
    raise KeyError(mutant)


# ---- the Lloyd iterations of gpb_hip_kmeans_lloyd (kmeans_assign_kernel of nn_kernels.hip + the host's ordered mean update), restated ----------------------------
def kmeans_lloyd_ref(x, means, max_it):
    """-> (means, iterations).  Assignment: the first mean at the smallest distance sqrt(sum of squares, coordinates ascending), strict <; update: per mean the sum of
    its rows in ascending order, one division; a mean without rows keeps its value; until the means repeat (the previous or the one before) or max_it."""
    x = np.asarray(x, dtype=F64)
    means = np.array(means, dtype=F64)
    n, d = x.shape
    k = means.shape[0]
    old, count = np.zeros_like(means), 0
    while True:
        oldold, old = old, means.copy()
        s2 = np.zeros((n, k))
        for c in range(d):
            t = x[:, c:c + 1] - means[None, :, c]
            s2 = s2 + t * t
        cl = np.argmin(np.sqrt(s2), axis=1)            # argmin: the first of equal minima
        for j in range(k):
            rows = np.nonzero(cl == j)[0]
            if rows.size:
                means[j] = np.cumsum(x[rows], axis=0)[-1] / rows.size      # cumsum: strictly in order
        count += 1
        if np.array_equal(means, old) or np.array_equal(means, oldold) or count == max_it:
            return means, count
