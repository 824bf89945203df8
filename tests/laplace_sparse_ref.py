"""The sparse machinery of the Vecchia-Laplace path (gpboost_amd/csrc/laplace_kernels.hip: the triangular solves of P^-1 = B^-1 (D^-1 + W)^-1 B^-T and the products with
B, B', Sigma^-1 + W) restated on the CPU: crafted neighbour graphs, the host schedule of upload_tri (gpb_laplace.inc), the operations in long double, a-priori bounds per
element, and an fp64 restatement of the kernels' operation order with five mutants.  numpy only; nothing here touches the device.

Everything below was derived from the kernels' code before any device run.  u = 2^-53, gamma(t) = t u / (1 - t u); "rounding" = one fp64 operation (an fma is ONE).
A sum  s = sum_e a_e x_e  formed by ANY tree of fma / add operations in which no term passes through more than k roundings satisfies
    |fl(s) - s| <= gamma(k) sum_e |a_e| |x_e|                                   (Higham, Accuracy and Stability of Numerical Algorithms, Lemma 3.1 + section 4.2)
with s the exact sum of the SAME operands.  All bounds are of this form, evaluated in long double with the operands the device itself used.

(S) Rows of a solve outside the dense block -- lap_sptrsv_kernel (body1 / body2), lap_sptrsv_sf_kernel, lap_sptrsv_sfw_kernel; the three promise the same bits.
    Row i of B z = scale .* t (forward; sources = its neighbours) or of B' t = r (backward; sources = the rows that have i as a neighbour, scale = 1):
        x_i = num_i den_i + sum_j A_ij x_j .
    Held to the componentwise RESIDUAL with the device's own solution xh, so no condition number enters:
        |num_i den_i + sum_j A_ij xh_j - xh_i| <= gamma(k_i) (|num_i den_i| + sum_j |A_ij| |xh_j|),
    k_i counted from the kernel for the slot layout of the row (a row of len entries takes ns = min(64, ceil(len / 64)) slots of per = ceil(len / ns) entries):
      * a lane's fma chain over its entries of one slot: 2 (head entries lane, lane + 16: `sum = fma(ha[k], g[k], sum)`, k = 0, 1);
        + 2 when the solve has overflow entries (template OVF: `fma(oa[k], g[2 + k], sum)` -- the masked ones multiply coefficient 0, which adds no error but is counted);
        + 4 per further 64 entries of the slot (the `e0` loop: four fma per trip) -- only a row of more than 4096 entries has such slots;
      * the four additions of row16_sum (the 16-lane butterfly);
      * one addition per further slot of the row (`v += s_part[..]` / `v[c] += row16_sum(..)`: the first slot's 0 + sum is exact);
      * the final add (`num + v`) or fma (`fma(num, den, v)`), which also is the single rounding of the term num_i den_i.
      k_i = chain + 4 + (ns - 1) + 1.
(D) Rows inside a dense block (LapDense: lap_dense_inv_kernel, lap_dense_rhs_kernel, lap_dense_matvec_kernel / lap_dense_gemm4_kernel + _sum_kernel).  Block-local
    N = A_blk (strictly lower triangular), M = (I - |N|)^-1 >= |(I - N)^-1| entrywise (comparison matrix; path sums).  The device forms
      inv^ : row k = e_k + sum_e A_e row_j(inv^), one fma chain of <= dmax = max in-block entries of a row per element, level by level (depth L = block levels).
             An element of (I - N)^-1 is a sum over paths of products of entries; each path of <= L edges passes <= L dmax roundings:  |inv^ - inv| <= gamma(L dmax) (M - I).
      t^   : rhs_k [* den_k] + sum over the row's entries with a source outside the block, 64 lanes: chain ceil(nout_k / 64), 6 additions of wave_sum, the final add / fma:
             c_t = ceil(max nout / 64) + 7.
      x^   : inv^ t^.  nc = 1: 4 accumulators, one fma each per 256 columns, then up to 3 more fma into a0 (the tail loop `for (; j <= k; j += 64)`), 2 additions,
             6 of wave_sum: c_mv = ceil(K / 256) + 11.
             nc = 4: per column split a chain over <= 64 ceil(ceil(K / 64) / 8) columns, 7 additions over the 8 splits: c_mv = 64 ceil(ceil(K / 64) / 8) + 7.
    Every elementary term (path product x term of the right-hand side) is perturbed by at most (1 + theta) with |theta| <= gamma(L dmax + c_t + c_mv), hence
        |xh_blk - (I - N)^-1 t| <= gamma(L dmax + c_t + c_mv) M T,     T_k = |num_k den_k| + sum_(j outside) |A_kj| |xh_j|
    and the residual of a block row, rho = t + N xh - xh = (I - N) ((I - N)^-1 t - xh), obeys   |rho| <= gamma(L dmax + c_t + c_mv) (I + |N|) M T.
(P) Products -- lap_tri_spmv_kernel: ONE chain per lane over all slots of the row: per slot 2 head fma + ceil(max(0, len_q - 32) / 16) overflow fma; then row16_sum (4).
      MODE 3 (lap_mul):  out = tot                                   k = chain + 4
      MODE 0 (lap_B), MODE 2 without W (lap_Bt):  out = x_i - tot    k = chain + 5
      MODE 1 (first half of lap_apply): (x_i - tot) * (1 / D_i): the reciprocal and the multiplication add 2:   |err| <= gamma(chain + 7) (|x_i| + sum |A||x|) / D_i
      MODE 2 with W (second half of lap_apply, on the device's own first half th): fma(W_i, h_i, th_i - tot):     |err| <= gamma(chain + 6) (|th_i| + sum |A||th| + |W_i h_i|)
    lap_vadu is (S)/(D) twice: B' t = r, then B z = rdw .* t on the device's own t.
The assertion is at the bound itself, no safety factor."""
import math

import numpy as np

LD = np.longdouble
U = LD(2) ** -53
RR, KWIDE, KDENSE_MAX, KDENSE_MINLEV = 64, 256, 8192, 16      # kTriRowsPerRound; upload_tri: kWide, kDenseMax, kDenseMinLevels


def gamma(t):
    t = np.asarray(t, dtype=LD)
    return t * U / (1 - t * U)


# ---- graphs --------------------------------------------------------------------------------------------------------------------------------------------------------
class Graph(object):
    """nn (n, m) int32: neighbours < row, -1 padded, no repeats; sigma: storage slot of Vecchia position i.  The handle gets the 1-d coordinates sigma[i] (distinct
    integers: their Morton rank is sigma itself, whatever the rounding of the scaling in morton_order)."""

    def __init__(self, name, nn, seed):
        self.name, self.nn = name, np.ascontiguousarray(nn, dtype=np.int32)
        self.n, self.m = self.nn.shape
        rng = np.random.default_rng(seed + 1000)
        self.sigma = rng.permutation(self.n).astype(np.int64)
        self.coords = self.sigma.astype(np.float64).reshape(-1, 1)
        rows = np.arange(self.n)[:, None]
        assert np.all(self.nn < rows) and np.all(self.nn >= -1)
        for i in range(self.n):
            r = self.nn[i][self.nn[i] >= 0]
            assert len(set(r.tolist())) == r.size
        # coefficients: random sign, sum_j |A_ij| <= 0.9 (so ||B^-1||_inf <= 10); D, W > 0 over six decades
        mask = self.nn >= 0
        mag = rng.uniform(0.05, 1.0, size=self.nn.shape) * mask
        tot = np.maximum(mag.sum(axis=1, keepdims=True), 1e-300)
        self.A = np.where(mask, rng.choice([-1.0, 1.0], size=self.nn.shape) * mag / tot * rng.uniform(0.3, 0.89, size=(self.n, 1)), 0.0)
        self.A2 = np.where(mask, rng.standard_normal(self.nn.shape), 0.0)
        self.D = 10.0 ** rng.uniform(-3, 3, size=self.n)
        self.W = 10.0 ** rng.uniform(-3, 3, size=self.n)
        self.scale = 1.0 / (1.0 / self.D + self.W)
        self._sched = {}

    def operand(self, ncols, seed=0):
        return np.random.default_rng(7919 * seed + self.n).standard_normal((self.n, ncols))

    def sched(self, backward):
        if backward not in self._sched:
            self._sched[backward] = schedule(self.nn, self.sigma, backward)
        return self._sched[backward]


def layers_graph(name, widths, m, kmin, kmax, reach, seed, hub=False):
    """Rows in layers (forward level = layer): a row takes k in [kmin, kmax] neighbours from the earlier layers, at least one from the layer before it; reach "prev": the
    nearest earlier layers first; "any": uniformly from all earlier rows.  hub: row 0 is a neighbour of every later row."""
    rng = np.random.default_rng(seed)
    start = np.concatenate([[0], np.cumsum(widths)])
    n = int(start[-1])
    nn = -np.ones((n, m), dtype=np.int32)
    for l in range(1, len(widths)):
        for i in range(start[l], start[l + 1]):
            k = min(int(rng.integers(kmin, kmax + 1)), int(start[l]))
            picked = [0] if hub else []
            if reach == "prev":
                ll = l - 1
                while len(picked) < k and ll >= 0:
                    pool = np.setdiff1d(np.arange(start[ll], start[ll + 1]), picked)
                    take = min(k - len(picked), pool.size)
                    picked += rng.choice(pool, size=take, replace=False).tolist()
                    ll -= 1
            else:
                first = int(rng.integers(start[l - 1], start[l]))
                if first not in picked:
                    picked.append(first)
                pool = np.setdiff1d(np.arange(0, start[l]), picked)
                picked += rng.choice(pool, size=min(k - len(picked), pool.size), replace=False).tolist()
            picked = picked[:k]
            nn[i, :len(picked)] = rng.permutation(picked)
    return Graph(name, nn, seed)


def uniform_graph(name, n, m, seed):
    """true nearest neighbours among the earlier points of n uniform points in the unit square, natural order"""
    rng = np.random.default_rng(seed)
    xy = rng.uniform(size=(n, 2))
    nn = -np.ones((n, m), dtype=np.int32)
    for i in range(1, n):
        d2 = np.sum((xy[:i] - xy[i]) ** 2, axis=1)
        k = min(m, i)
        nn[i, :k] = np.argsort(d2, kind="stable")[:k]
    return Graph(name, nn, seed)


_GRAPHS = {}


def graph(name):
    if name not in _GRAPHS:
        if name == "layers-m12":
            g = layers_graph(name, [1] * 8 + [300] + [40] * 3 + [300] + [5] * 20, 12, 12, 12, "any", 1)
        elif name == "layers-m70":
            g = layers_graph(name, [1] * 20 + [300, 30, 30, 300] + [3] * 18, 70, 30, 70, "prev", 2)
        elif name == "layers-m126":
            g = layers_graph(name, [1] * 4 + [130, 130, 300], 126, 60, 126, "prev", 3)
        elif name == "hub-m4":
            g = layers_graph(name, [1] + [5] * 8 + [4259], 4, 4, 4, "prev", 4, hub=True)
        elif name == "uniform-m20":
            g = uniform_graph(name, 1200, 20, 5)
        elif name == "tiny":
            g = layers_graph(name, [1, 2, 5, 9, 3, 12, 8], 6, 2, 6, "any", 6)
        else:
            raise KeyError(name)
        _GRAPHS[name] = g
    return _GRAPHS[name]


GRAPHS = ("layers-m12", "layers-m70", "layers-m126", "hub-m4", "uniform-m20")
# what each recipe has to reach, by the restated schedule: (solve, field, relation, value); fields as in shim.VecchiaState._LAP_INFO plus "has_ovf"
REACHES = {
    "layers-m12": [("fwd", "dense_K", "==", 0), ("fwd", "wide_segments", "==", 2), ("fwd", "run_segments", "==", 3), ("fwd", "novf", "==", 0),
                   ("bwd", "dense_K", "==", 828), ("bwd", "split_rows", ">", 0)],
    "layers-m70": [("fwd", "dense_K", "==", 20), ("bwd", "dense_K", "==", 20), ("fwd", "split_rows", ">", 0), ("fwd", "novf", ">", 0), ("bwd", "padding_slots", ">", 0),
                   ("fwd", "wide_segments", ">", 0), ("bwd", "wide_segments", ">", 0), ("bwd", "run_segments", ">", 0)],
    "layers-m126": [("fwd", "split_rows", ">", 0), ("bwd", "wide_segments", "==", 3), ("fwd", "padding_slots", ">", 0), ("fwd", "dense_K", "==", 0), ("bwd", "dense_K", "==", 0)],
    "hub-m4": [("bwd", "long_slots", ">=", 63), ("bwd", "dense_K", "==", 0), ("fwd", "dense_K", "==", 0), ("fwd", "widest_level_slots", "==", 4259),
               ("bwd", "widest_level_slots", "==", 4259), ("bwd", "max_row_entries", "==", 4299)],
    "uniform-m20": [("fwd", "dense_K", "==", 1200), ("bwd", "dense_K", "==", 1200)],
}
# (nc, ncol): single vectors; the probe block: 13 chunks = the 50-probe block, 17 crosses the 16-chunk dense pass and leaves a partial last unit of four chunks
SHAPES = [(1, 1), (1, 3), (1, 70), (4, 1), (4, 2), (4, 13), (4, 17)]
OPS = ("B", "Bt", "apply", "vadu", "fwd_solve", "mul_fwd", "mul_bwd")
SOLVE_OPS = ("vadu", "fwd_solve")


# ---- the schedule of upload_tri, restated ---------------------------------------------------------------------------------------------------------------------------
class Sched(object):
    pass


def schedule(nn, sigma, backward):
    """build_levels + upload_tri for one solve.  Entries of row i in the order the host lists them: forward the neighbours in table order, backward the rows that have i
    as a neighbour in ascending order; position = index into A.  Rows of a level in ascending storage slot."""
    n, m = nn.shape
    ent = [[] for _ in range(n)]
    lev = np.zeros(n, dtype=np.int64)
    if not backward:
        for i in range(n):
            l = 0
            for j in range(m):
                c = int(nn[i, j])
                if c >= 0:
                    ent[i].append((c, i * m + j))
                    l = max(l, lev[c] + 1)
            lev[i] = l
    else:
        for i in range(n):
            for j in range(m):
                c = int(nn[i, j])
                if c >= 0:
                    ent[c].append((i, i * m + j))
        for i in range(n - 1, -1, -1):
            for j in range(m):
                c = int(nn[i, j])
                if c >= 0:
                    lev[c] = max(lev[c], lev[i] + 1)
    nlev = int(lev.max()) + 1
    order = np.lexsort((sigma, lev))
    lptr = np.concatenate([[0], np.cumsum(np.bincount(lev, minlength=nlev))])
    s = Sched()
    s.n, s.m, s.backward, s.lev, s.nlev, s.ent, s.order, s.lptr = n, m, backward, lev, nlev, ent, order, lptr
    s.slot_row, s.slot_ns, s.slot_ent, s.ptr = [], [], [], [0] * (nlev + 1)
    s.row_slot = np.zeros(n, dtype=np.int64)
    npad = nmulti = nlong = novf = 0
    for l in range(nlev):
        s.ptr[l] = len(s.slot_row)
        for i in order[lptr[l]:lptr[l + 1]]:
            ln = len(ent[i])
            ns = min(RR, max(1, (ln + 63) // 64))
            per = (ln + ns - 1) // ns
            in_round = (len(s.slot_row) - s.ptr[l]) % RR
            if in_round + ns > RR:
                for _ in range(RR - in_round):
                    s.slot_row.append(-1); s.slot_ns.append(0); s.slot_ent.append([]); npad += 1
            nmulti += ns > 1
            s.row_slot[i] = len(s.slot_row)
            for g in range(ns):
                lo = min(ln, g * per); hi = min(ln, lo + per)
                s.slot_row.append(int(i) if g == 0 else -1); s.slot_ns.append(ns if g == 0 else 0); s.slot_ent.append(ent[i][lo:hi])
                nlong += hi - lo > 64
                novf += max(0, hi - lo - 32)
    s.ptr[nlev] = len(s.slot_row)
    cnt = np.diff(s.ptr)
    La = Lb = nlev if backward else 0
    K = 0
    if not backward:
        while Lb < nlev and cnt[Lb] < KWIDE and K + (lptr[Lb + 1] - lptr[Lb]) <= KDENSE_MAX:
            K += lptr[Lb + 1] - lptr[Lb]; Lb += 1
    else:
        while La > 0 and cnt[La - 1] < KWIDE and K + (lptr[La] - lptr[La - 1]) <= KDENSE_MAX:
            K += lptr[La] - lptr[La - 1]; La -= 1
    if Lb - La < KDENSE_MINLEV:
        La = Lb = nlev if backward else 0
        K = 0
    s.La, s.Lb, s.K = La, Lb, int(K)
    s.block_rows = order[lptr[La]:lptr[La] + K] if K else np.zeros(0, dtype=np.int64)
    s.in_block = np.zeros(n, dtype=bool)
    s.in_block[s.block_rows] = True
    s.segs = []
    l = 0
    while l < nlev:
        if La <= l < Lb:
            l = Lb
            continue
        lend = La if l < La else nlev
        if cnt[l] >= KWIDE:
            s.segs.append((l, l + 1, (cnt[l] + RR - 1) // RR)); l += 1
            continue
        e = l
        while e < lend and cnt[e] < KWIDE:
            e += 1
        s.segs.append((l, e, 1)); l = e
    s.has_ovf = novf > 0
    s.info = {"nlev": nlev, "nslots": len(s.slot_row), "novf": int(novf), "dense_K": int(K), "wide_segments": sum(1 for g in s.segs if g[2] > 1),
              "run_segments": sum(1 for g in s.segs if g[2] == 1), "padding_slots": int(npad), "split_rows": int(nmulti), "long_slots": int(nlong)}
    s.extra = {"widest_level_slots": int(cnt.max()), "max_row_entries": max(len(e) for e in ent), "has_ovf": int(s.has_ovf)}
    # CSR of the entries by row (Vecchia indices) for the long-double sums
    s.eptr = np.concatenate([[0], np.cumsum([len(e) for e in ent])]).astype(np.int64)
    flat = [x for e in ent for x in e]
    s.esrc = np.array([x[0] for x in flat], dtype=np.int64)
    s.epos = np.array([x[1] for x in flat], dtype=np.int64)
    s.erow = np.repeat(np.arange(n), np.diff(s.eptr))
    return s


def solve_roundings(s):
    """k_i of (S) for every row (the rows of the dense block get theirs from dense_constants)"""
    ln = np.diff(s.eptr)
    ns = np.minimum(RR, np.maximum(1, (ln + 63) // 64))
    per = (ln + ns - 1) // ns
    chain = 2 + (2 if s.has_ovf else 0) + 4 * ((np.maximum(per - 64, 0) + 63) // 64)
    return chain + 4 + (ns - 1) + 1


def product_chain(s):
    """fma chain of a lane of lap_tri_spmv_kernel over all slots of the row"""
    ln = np.diff(s.eptr)
    ns = np.minimum(RR, np.maximum(1, (ln + 63) // 64))
    per = (ln + ns - 1) // ns
    last = ln - (ns - 1) * per
    f = lambda q: 2 + (np.maximum(q - 32, 0) + 15) // 16
    return (ns - 1) * f(per) + f(last)


def dense_constants(s, nc):
    """L dmax + c_t + c_mv of (D)"""
    K = s.K
    loc = s.in_block
    inblk = np.array([sum(1 for c, _ in s.ent[i] if loc[c]) for i in s.block_rows])
    nout = np.array([sum(1 for c, _ in s.ent[i] if not loc[c]) for i in s.block_rows])
    L = s.Lb - s.La
    c_t = int(math.ceil(max(1, nout.max()) / 64)) + 7
    nt = (K + 63) // 64
    c_mv = (K + 255) // 256 + 11 if nc == 1 else 64 * ((nt + 7) // 8) + 7
    return L * int(max(1, inblk.max())) + c_t + c_mv


# ---- the operations in long double ------------------------------------------------------------------------------------------------------------------------------
def _row_sums(s, coef, X, absolute=False, block=64):
    """sum_e coef_e X[src_e] per row (long double; |.| of both factors with absolute), X (n, cols)"""
    n, cols = X.shape
    out = np.zeros((n, cols), dtype=LD)
    if s.esrc.size == 0:
        return out
    nonempty = np.nonzero(np.diff(s.eptr) > 0)[0]
    c = coef.astype(LD)
    for c0 in range(0, cols, block):
        Xb = X[:, c0:c0 + block].astype(LD)
        t = c[:, None] * Xb[s.esrc]
        if absolute:
            t = np.abs(t)
        out[nonempty, c0:c0 + block] = np.add.reduceat(t, s.eptr[:-1][nonempty], axis=0)
    return out


def coef_of(s, A):
    return np.asarray(A).reshape(-1)[s.epos]


def product_ref(s, A, X, mode, D=None, W=None, H=None):
    """-> (value, bound) of lap_tri_spmv_kernel<mode> on the layout s, long double (P)"""
    c = coef_of(s, A)
    Xl = X.astype(LD)
    tot, atot = _row_sums(s, c, X), _row_sums(s, c, X, absolute=True)
    chain = product_chain(s)[:, None]
    if mode == 3:
        return tot, gamma(chain + 4) * atot
    val, mag = Xl - tot, np.abs(Xl) + atot
    if mode == 0 or (mode == 2 and W is None):
        return val, gamma(chain + 5) * mag
    if mode == 1:
        Dl = D.astype(LD)[:, None]
        return val / Dl, gamma(chain + 7) * mag / Dl
    wh = W.astype(LD)[:, None] * H.astype(LD)
    return val + wh, gamma(chain + 6) * (mag + np.abs(wh))


def solve_exact(s, A, num, den):
    """the solution of x_i = num_i den_i + sum_j A_ij x_j in long double, by substitution in level order"""
    c = coef_of(s, A).astype(LD)
    x = np.zeros(num.shape, dtype=LD)
    nd = num.astype(LD) * (den.astype(LD)[:, None] if den is not None else 1)
    for i in s.order:
        e0, e1 = s.eptr[i], s.eptr[i + 1]
        x[i] = nd[i] + (c[e0:e1, None] * x[s.esrc[e0:e1]]).sum(axis=0) if e1 > e0 else nd[i]
    return x


def solve_check(s, A, num, den, xh, nc):
    """Residual of the device's solution xh against (S) / (D): -> (ratio (n, cols) = |residual| / bound, dense mask (n))."""
    c = coef_of(s, A)
    nd = num.astype(LD) * (den.astype(LD)[:, None] if den is not None else 1)
    res = np.abs(nd + _row_sums(s, c, xh) - xh.astype(LD))
    T = np.abs(nd) + _row_sums(s, c, xh, absolute=True)
    bound = gamma(solve_roundings(s))[:, None] * T
    if s.K:
        blk = s.block_rows
        loc = -np.ones(s.n, dtype=np.int64)
        loc[blk] = np.arange(s.K)
        cl = np.abs(c.astype(LD))
        # T of the block rows: only the sources outside the block; M T by substitution with |N|; then (I + |N|) M T
        out_mask = ~s.in_block[s.esrc]
        so = Sched(); so.eptr = np.concatenate([[0], np.cumsum(np.bincount(s.erow[out_mask], minlength=s.n))]); so.esrc = s.esrc[out_mask]
        Tb = (np.abs(nd) + _row_sums(so, c[out_mask], xh, absolute=True))[blk]
        y = np.zeros_like(Tb)
        for k, i in enumerate(blk):
            e = np.arange(s.eptr[i], s.eptr[i + 1])
            e = e[s.in_block[s.esrc[e]]]
            y[k] = Tb[k] + (cl[e, None] * y[loc[s.esrc[e]]]).sum(axis=0) if e.size else Tb[k]
        z = np.zeros_like(Tb)
        for k, i in enumerate(blk):
            e = np.arange(s.eptr[i], s.eptr[i + 1])
            e = e[s.in_block[s.esrc[e]]]
            z[k] = y[k] + (cl[e, None] * y[loc[s.esrc[e]]]).sum(axis=0) if e.size else y[k]
        bound[blk] = gamma(dense_constants(s, nc)) * z
    with np.errstate(divide="ignore", invalid="ignore"):
        ratio = np.where(res == 0, 0, res / bound)
    ratio = np.where(np.isfinite(ratio), ratio, np.inf)
    return ratio.astype(np.float64), s.in_block.copy()


def ratio_of(err, bound):
    with np.errstate(divide="ignore", invalid="ignore"):
        q = np.where(err == 0, 0, np.abs(err) / bound)
    return np.where(np.isfinite(q), q, np.inf).astype(np.float64)


# ---- the kernels' operation order in fp64 ----------------------------------------------------------------------------------------------------------------------
def _split(x):
    mnt, e = math.frexp(x)
    return int(mnt * 9007199254740992.0), e - 53


def fma(a, b, c):
    """correctly rounded a * b + c (integer arithmetic; no subnormal results at the magnitudes used here)"""
    if a == 0.0 or b == 0.0:
        return c + 0.0
    ia, ea = _split(a); ib, eb = _split(b)
    p, ep = ia * ib, ea + eb
    if c == 0.0:
        return math.ldexp(float(p), ep)
    ic, ec = _split(c)
    if ep >= ec:
        return math.ldexp(float((p << (ep - ec)) + ic), ec)
    return math.ldexp(float(p + (ic << (ec - ep))), ep)


def _butterfly16(v):
    """row16_sum: quad_perm [1,0,3,2], [2,3,0,1], row_half_mirror, row_mirror; every lane ends with the same bits -- lane 0's are returned"""
    v = list(v)
    for perm in ([1, 0, 3, 2, 5, 4, 7, 6, 9, 8, 11, 10, 13, 12, 15, 14], [2, 3, 0, 1, 6, 7, 4, 5, 10, 11, 8, 9, 14, 15, 12, 13],
                 [7, 6, 5, 4, 3, 2, 1, 0, 15, 14, 13, 12, 11, 10, 9, 8], [15, 14, 13, 12, 11, 10, 9, 8, 7, 6, 5, 4, 3, 2, 1, 0]):
        v = [v[l] + v[perm[l]] for l in range(16)]
    return v[0]


def _slot_sum(entries, coef, x, ovf, drop_last_ovf=False):
    """one slot, one column: lanes 0..15, chain head[lane], ovf[lane], head[lane + 16], ovf[lane + 16], then the rest of the overflow 64 at a time"""
    head, over = entries[:32], entries[32:]
    if drop_last_ovf and over:
        over = over[:-1]
    lanes = []
    for lane in range(16):
        sm = 0.0
        for k in range(2):
            if lane + 16 * k < len(head):
                e = head[lane + 16 * k]
                sm = fma(coef[e[1]], x[e[0]], sm)
            if ovf and lane + 16 * k < len(over):
                e = over[lane + 16 * k]
                sm = fma(coef[e[1]], x[e[0]], sm)
        for e0 in range(32 + lane, len(over), 64):
            for k in range(4):
                if e0 + 16 * k < len(over):
                    e = over[e0 + 16 * k]
                    sm = fma(coef[e[1]], x[e[0]], sm)
        lanes.append(sm)
    return _butterfly16(lanes)


MUTANTS = ("drop_last_overflow", "skip_continuation_slots", "scale_at_vecchia_index", "neighbour_chunk_column", "same_level_read_early")


def solve_fp64(s, A, num, den, sigma=None, mutant=None):
    """The solve in the kernels' order, all columns of num (n, cols) -> x (n, cols) fp64.  Rows of the dense block (only blocks of K <= 64 are restated: the inverse costs
    K^2 dmax / 2 scalar fma here): lap_dense_inv_kernel, lap_dense_rhs_kernel and lap_dense_matvec_kernel (nc = 1).  Mutants: MUTANTS."""
    coef = np.asarray(A, dtype=np.float64).reshape(-1).tolist()
    n, cols = num.shape
    x = [[0.0] * n for _ in range(cols)]
    if den is None:
        dn = [1.0] * n
    elif mutant == "scale_at_vecchia_index":      # the scale lives in storage order: entry sigma^-1 ... read at the wrong index
        inv = np.argsort(sigma)
        dn = [float(den[inv[i]]) for i in range(n)]
    else:
        dn = [float(v) for v in den]
    scale = den is not None

    def sparse_level(l, src):
        for q in range(s.ptr[l], s.ptr[l + 1]):
            i, ns = s.slot_row[q], s.slot_ns[q]
            if ns <= 0:
                continue
            for c in range(cols):
                xs = src[c ^ 1] if (mutant == "neighbour_chunk_column" and c == 1 and cols > 1) else src[c]
                v = 0.0
                for g in range(1 if mutant == "skip_continuation_slots" else ns):
                    v = v + _slot_sum(s.slot_ent[q + g], coef, xs, s.has_ovf, mutant == "drop_last_overflow")
                x[c][i] = fma(float(num[i, c]), dn[i], v) if scale else float(num[i, c]) + v

    def dense_block():
        K, blk = s.K, [int(i) for i in s.block_rows]
        assert K <= 64, "only small dense blocks are restated in fp64"
        loc = {i: k for k, i in enumerate(blk)}
        inv = [[0.0] * K for _ in range(K)]
        for k, i in enumerate(blk):
            for c in range(k + 1):
                acc = 1.0 if c == k else 0.0
                for (j, pos) in s.ent[i]:
                    if j in loc and c <= loc[j]:
                        acc = fma(coef[pos], inv[loc[j]][c], acc)
                inv[k][c] = acc
        for c in range(cols):
            t = []
            for k, i in enumerate(blk):
                outside = [(j, pos) for (j, pos) in s.ent[i] if j not in loc]
                lanes = [0.0] * 64
                for idx, (j, pos) in enumerate(outside):
                    lanes[idx % 64] = fma(coef[pos], x[c][j], lanes[idx % 64])
                o = 32
                while o:
                    lanes = [lanes[l] + lanes[l ^ o] for l in range(64)]
                    o >>= 1
                t.append(fma(float(num[i, c]), dn[i], lanes[0]) if scale else float(num[i, c]) + lanes[0])
            for k, i in enumerate(blk):
                lanes = [fma(inv[k][l], t[l], 0.0) if l <= k else 0.0 for l in range(64)]      # K <= 64: one fma in accumulator a0 of every lane; (a0 + a1) + (a2 + a3) exact
                o = 32
                while o:
                    lanes = [lanes[l] + lanes[l ^ o] for l in range(64)]
                    o >>= 1
                x[c][i] = lanes[0]

    widest = int(np.argmax(np.diff(s.ptr)[:-1])) if s.nlev > 1 else 0
    if s.K and not s.backward:
        dense_block()
    for l in range(s.nlev):
        if s.La <= l < s.Lb:
            continue
        if mutant == "same_level_read_early" and l == widest + 1 and not (s.La <= widest < s.Lb):
            continue          # (done with the level before it, below)
        if mutant == "same_level_read_early" and l == widest and l + 1 < s.nlev and not (s.La <= l + 1 < s.Lb):
            snap = [list(col) for col in x]
            sparse_level(l, snap); sparse_level(l + 1, snap)
        else:
            sparse_level(l, x)
    if s.K and s.backward:
        dense_block()
    return np.array(x, dtype=np.float64).T


def product_fp64(s, A, X, mode, D=None, W=None, H=None):
    """lap_tri_spmv_kernel<mode> in its order: one chain per lane over all slots of the row"""
    coef = np.asarray(A, dtype=np.float64).reshape(-1).tolist()
    n, cols = X.shape
    out = np.zeros((n, cols))
    for c in range(cols):
        xc = X[:, c].tolist()
        for q in range(len(s.slot_row)):
            i, ns = s.slot_row[q], s.slot_ns[q]
            if ns <= 0:
                continue
            lanes = [0.0] * 16
            for g in range(ns):
                en = s.slot_ent[q + g]
                head, over = en[:32], en[32:]
                for lane in range(16):
                    sm = lanes[lane]
                    for k in range(2):
                        if lane + 16 * k < len(head):
                            e = head[lane + 16 * k]
                            sm = fma(coef[e[1]], xc[e[0]], sm)
                    for j in range(lane, len(over), 16):
                        e = over[j]
                        sm = fma(coef[e[1]], xc[e[0]], sm)
                    lanes[lane] = sm
            tot = _butterfly16(lanes)
            v = tot if mode == 3 else xc[i] - tot
            if mode == 1:
                v = v * (1.0 / float(D[i]))
            if mode == 2 and W is not None:
                v = fma(float(W[i]), float(H[i, c]), v)
            out[i, c] = v
    return out
