"""GPU (MI355X): the fixed-point histogram sums (gpboost_amd/csrc/hist_kernels.hip, "fixed-point accumulation") against the exact integer model of the documented
scheme (tests/hist_fixed_point_ref.py, pinned on the CPU by tests/test_hist_fixed_point_ref.py), through shim.HistBuilder and the C ABI only.

Every build is checked three ways:
  (a) counts == the model's counts;
  (b) hist[:, 0] and hist[:, 1] BIT-equal to the model's entries fl(sum k) * q -- the scheme is deterministic integer arithmetic, so the tolerance is zero by derivation;
  (c) |hist - exact real sum| <= count * q / 2 + ulp(entry) per bin: the contract's own bound, evaluated in rationals.
The cases sit on the budgets of the integer stages: the per-chunk hessian partial (2^51 per row: one 64-bit word wraps from 4096 rows of one bin in a chunk on -- the
defect this file was written for: with it, every wrapped partial takes 2^64 q = 16384 off a bin's hessian sum), the packed gradient word between two flushes
(1792 * 2^41 < 2^52, 11-bit count), the rounding trick at |x| -> 2^51 and on ties, and the scale at max = 0, subnormal, huge and non-finite."""
import math
from fractions import Fraction

import numpy as np
import pytest

from tests import hist_fixed_point_ref as ref

pytestmark = pytest.mark.gpu


def _check(hb, bins, bo, rows, g, h, label, const_hess=1.0, model=None, exact_h=None):
    """one build against the model: (a), (b), (c).  g / h: ref.Channel (h None: constant hessian); model: a Result computed before (same row SET);
    exact_h: the exact hessian sums where the test knows them in closed form (constant per-row hessians: count * h)."""
    hist, cnt = hb.build(None if rows is None else np.ascontiguousarray(rows, dtype=np.int32), const_hess=const_hess)
    m = model if model is not None else ref.histogram(bins, bo, rows, g, h, const_hess=const_hess)
    nbad_c = int((cnt != m.counts).sum())
    bad_g = np.flatnonzero(~((hist[:, 0] == m.hist[:, 0]) | (np.isnan(hist[:, 0]) & np.isnan(m.hist[:, 0]))))
    bad_h = np.flatnonzero(~((hist[:, 1] == m.hist[:, 1]) | (np.isnan(hist[:, 1]) & np.isnan(m.hist[:, 1]))))
    worst = lambda c, bad: float(np.abs(hist[bad, c] - m.hist[bad, c]).max()) if bad.size else 0.0
    print("%s: bins differing from the model: counts %d, grad %d (max |diff| %.6g), hess %d (max |diff| %.6g)" %
          (label, nbad_c, bad_g.size, worst(0, bad_g), bad_h.size, worst(1, bad_h)))
    assert nbad_c == 0, "%s: (a) counts" % label
    assert bad_g.size == 0, "%s: (b) gradient sums differ from fl(sum k) q in %d bins, first %d: %r against %r" % (label, bad_g.size, bad_g[0], hist[bad_g[0], 0], m.hist[bad_g[0], 0])
    assert bad_h.size == 0, "%s: (b) hessian sums differ from fl(sum k) q in %d bins, first %d: %r against %r" % (label, bad_h.size, bad_h[0], hist[bad_h[0], 1], m.hist[bad_h[0], 1])
    if g.finite:
        assert ref.bound_violations(hist[:, 0], m.exact_g, cnt, g.q) == [], "%s: (c) gradient bound" % label
    if h is not None and h.finite:
        assert ref.bound_violations(hist[:, 1], exact_h if exact_h is not None else m.exact_h, cnt, h.q) == [], "%s: (c) hessian bound" % label
    elif h is None:
        assert np.array_equal(hist[:, 1], cnt.astype(np.float64) * const_hess)
    return hist, cnt, m


# ---- the per-chunk hessian partial ---------------------------------------------------------------------------------------------------------------------
def _budget_bins(n, F, seed):
    """column 0: two bins; column 1: 99 % of the rows in its most frequent bin (bin 0); column 2: 256 bins, uniform; the rest random bin counts"""
    rng = np.random.default_rng(seed)
    nb = rng.integers(2, 257, size=F); nb[0] = 2; nb[1] = 64; nb[2] = 256
    bins = np.empty((F, n), dtype=np.uint8)
    for f in range(F):
        bins[f] = rng.integers(0, nb[f], size=n)
    bins[1] = np.where(rng.uniform(size=n) < 0.99, 0, rng.integers(1, 64, size=n))
    bo = np.concatenate([[0], np.cumsum(nb)]).astype(np.int32)
    return rng, bins, bo


_HESSIANS = {"all_1.9": lambda rng, n: np.full(n, 1.9), "all_0.25": lambda rng, n: np.full(n, 0.25), "all_1.0": lambda rng, n: np.full(n, 1.0),
             "uniform_1.99_2": lambda rng, n: rng.uniform(1.99, 2.0, size=n)}


def _hessian_budget_case(lib_built, n, F, seed):
    from gpboost_amd import shim
    rng, bins, bo = _budget_bins(n, F, seed)
    grad = rng.standard_normal(n)
    g = ref.Channel(grad, False)
    leaf = np.sort(rng.choice(n, size=n // 3, replace=False))
    rowsets = [("all rows", None, None), ("sorted leaf", leaf, leaf), ("shuffled leaf", rng.permutation(leaf), leaf),        # (the model of a row SET: order-free)
               ("dominant bin's rows", np.flatnonzero(bins[1] == 0), np.flatnonzero(bins[1] == 0))]
    gm = {}          # the gradient side of the model is the same for every hessian array: once per row set
    hb = shim.HistBuilder(bins, bo)
    failures = []
    for hname, make in _HESSIANS.items():
        hess = make(rng, n)
        h = ref.Channel(hess, True)
        const = hname.startswith("all_")
        hb.set_gradients(grad, hess)
        hm = {}
        for rname, rows, mrows in rowsets:
            key = "all" if mrows is None else rname.replace("shuffled", "sorted")
            if key not in gm:
                gm[key] = ref.histogram(bins, bo, mrows, g, None)
            if key not in hm:
                hm[key] = ref.histogram(bins, bo, mrows, None, h, want_exact=not const)
            m = ref.Result()
            m.counts = gm[key].counts; m.exact_g = gm[key].exact_g; m.exact_h = hm[key].exact_h
            m.hist = np.stack([gm[key].hist[:, 0], hm[key].hist[:, 1]], axis=1)
            exact_h = [int(c) * Fraction(float(hess[0])) for c in m.counts] if const else None       # constant per-row hessians: the exact sum is count * h
            try:
                _check(hb, bins, bo, rows, g, h, "n=%d F=%d hess %s, %s" % (n, F, hname, rname), model=m, exact_h=exact_h)
            except AssertionError as e:
                failures.append(str(e).splitlines()[0])
    hb.close()
    assert not failures, "%d of %d builds:\n" % (len(failures), len(_HESSIANS) * len(rowsets)) + "\n".join(failures)


@pytest.mark.parametrize("n", [1200000, 3000000])
def test_hessian_chunk_partials_hold_2_pow_51_per_row(lib_built, n):
    """F = 50 (four feature groups): with per-row hessians at most 2 * 256 / 4 = 128 chunks, i.e. 9375 / 23438 rows per chunk; the two-bin column, the dominant bin and
    near-constant hessians put more than 4096 rows of one bin into a chunk at ~2^51 each."""
    _hessian_budget_case(lib_built, n, 50, seed=n % 1000 + 50)


def test_hessian_chunk_partials_one_feature_group(lib_built):
    """F = 16: ONE feature group, so min(ceil(n / 1024), 2 * num_cu / 1) chunks -- 512 on 256 CUs (fewer on a smaller part: more rows per chunk): n = 512 * 8192 + 50000
    leaves more than 8192 rows per chunk."""
    _hessian_budget_case(lib_built, 512 * 8192 + 50000, 16, seed=16)


# ---- the packed gradient word between two flushes ---------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("n,F", [(1000000, 64), (1000000, 50), (100000, 3)])     # whole-row kernel with a full quad / with a partial last group; hist_build_kernel with nf < 16
@pytest.mark.parametrize("pattern", ["same_sign", "alternating", "sign_per_1792_block"])
def test_gradient_word_at_its_flush_budget(lib_built, n, F, pattern):
    """Every row in ONE bin of one feature with g = +-max: |k| = 2^40 .. 2^41 per row, 1792 rows between two flushes of the packed word (sum field 53 bits, count field 11)."""
    from gpboost_amd import shim
    rng = np.random.default_rng(n + F)
    nb = np.full(F, 255); nb[0] = 3
    bins = rng.integers(0, 255, size=(F, n), dtype=np.uint8)
    bins[0] = 2                                                          # feature 0: all rows in its last bin
    if F > 1:
        bins[F - 1] = 0                                                  # ... and the last feature (the partial group's last column) in bin 0
    bo = np.concatenate([[0], np.cumsum(nb)]).astype(np.int32)
    mx = math.nextafter(2.0, 0.0)                                        # k = 2^41 exactly: the top of the budget
    i = np.arange(n)
    sign = {"same_sign": np.ones(n), "alternating": 1.0 - 2.0 * (i & 1), "sign_per_1792_block": 1.0 - 2.0 * ((i // 1792) & 1)}[pattern]
    grad = mx * sign
    if pattern == "same_sign":
        grad = -grad                                                     # all negative: every word borrows from its count field
    # per-row hessians far below their scale but for one row (k_h ~ 2^44): this test is about the gradient word, the hessian partial's own budget has its tests above
    hess = rng.uniform(0.005, 0.02, size=n); hess[1] = 1.5
    g = ref.Channel(grad, False)
    hb = shim.HistBuilder(bins, bo)
    gm = ref.histogram(bins, bo, None, g, None)
    if pattern == "same_sign":
        assert gm.tot_g[2] == -(n << 41)
    hb.set_gradients(grad, None)
    _check(hb, bins, bo, None, g, None, "%s n=%d F=%d constant hessian" % (pattern, n, F), const_hess=0.7, model=ref.histogram(bins, bo, None, g, None, const_hess=0.7))
    leaf = rng.permutation(n)[: n // 2]
    _check(hb, bins, bo, leaf, g, None, "%s n=%d F=%d constant hessian, shuffled leaf" % (pattern, n, F))
    hb.set_gradients(grad, hess)
    h = ref.Channel(hess, True)
    hm = ref.histogram(bins, bo, None, None, h)
    m = ref.Result(); m.counts = gm.counts; m.exact_g = gm.exact_g; m.exact_h = hm.exact_h; m.hist = np.stack([gm.hist[:, 0], hm.hist[:, 1]], axis=1)
    _check(hb, bins, bo, None, g, h, "%s n=%d F=%d per-row hessians" % (pattern, n, F), model=m)
    hb.close()


# ---- rounding and scale edges --------------------------------------------------------------------------------------------------------------------------------
def _edge_bins(n, F, seed):
    rng = np.random.default_rng(seed)
    nb = rng.integers(2, 257, size=F); nb[0] = 2
    bins = np.stack([rng.integers(0, nb[f], size=n) for f in range(F)]).astype(np.uint8)
    return rng, bins, np.concatenate([[0], np.cumsum(nb)]).astype(np.int32)


def _edge_arrays(rng, n, hess):
    """name -> values (gradients; hess: the same edges for non-negative hessians)"""
    bits = 51 if hess else 41
    out = {}
    for ex in (1, -7):
        q = math.ldexp(1.0, ex - bits)
        top = math.nextafter(math.ldexp(1.0, ex), 0.0)
        ties = (rng.integers(0, 1 << 20, size=n) + 0.5) * q               # exact .5 multiples of q: ties to even
        ties[0] = top                                                     # (fixes the scale)
        edge = np.full(n, top)                                            # x + kMagic -> 2^53 for hessians, k = +-2^41 for gradients
        if not hess:
            ties *= 1.0 - 2.0 * (rng.integers(0, 2, size=n)); ties[0] = top
            edge *= 1.0 - 2.0 * (rng.integers(0, 2, size=n))
        out["ties ex=%d" % ex] = ties
        out["nextafter(2^%d, 0)" % ex] = edge
    out["all zero"] = np.zeros(n)
    sub = rng.integers(1, 1 << 40, size=n) * 5e-324
    out["subnormal only"] = sub if hess else sub * (1.0 - 2.0 * rng.integers(0, 2, size=n))
    big = np.full(n, 1e-3); big[n // 2] = 1e12
    out["one 1e12 among 1e-3"] = big
    bad = rng.uniform(0.5, 2.0, size=n); bad[5] = np.inf; bad[n - 7] = np.nan
    out["one inf and one nan"] = bad
    return out


@pytest.mark.parametrize("n,F", [(60000, 20), (540000, 64)])              # hist_build_kernel; the whole-row kernel (constant hessian, >= 2048 rows per CU)
def test_rounding_and_scale_edges(lib_built, n, F):
    from gpboost_amd import shim
    rng, bins, bo = _edge_bins(n, F, seed=n + F)
    hb = shim.HistBuilder(bins, bo)
    leaf = rng.permutation(n)[: n // 3]
    plain_g = rng.standard_normal(n); plain_h = rng.uniform(0.5, 2.0, size=n)
    gp, hp = ref.Channel(plain_g, False), ref.Channel(plain_h, True)
    # the ordinary side of every pair (edge gradients + ordinary hessians, ordinary gradients + edge hessians) is modelled once
    hp_all = ref.histogram(bins, bo, None, None, hp)
    gp_all, gp_leaf = ref.histogram(bins, bo, None, gp, None), ref.histogram(bins, bo, leaf, gp, None)

    def both(mg, mh):
        m = ref.Result()
        m.counts = mg.counts; m.exact_g = mg.exact_g; m.exact_h = mh.exact_h; m.hist = np.stack([mg.hist[:, 0], mh.hist[:, 1]], axis=1)
        return m

    for name, v in _edge_arrays(rng, n, False).items():
        g = ref.Channel(v, False)
        hb.set_gradients(v, None)
        hist, cnt, m = _check(hb, bins, bo, None, g, None, "gradients %s, n=%d F=%d" % (name, n, F))
        _check(hb, bins, bo, leaf, g, None, "gradients %s, n=%d F=%d, leaf" % (name, n, F))
        if name == "all zero":
            assert not hist[:, 0].any() and int(cnt[bo[0]:bo[1]].sum()) == n
        if name == "subnormal only":
            assert np.isfinite(hist).all()
        if name == "one inf and one nan":
            assert np.isnan(hist[:, 0]).all() and np.array_equal(cnt, m.counts)
        if name == "one 1e12 among 1e-3":
            assert g.q == 0.5 and np.count_nonzero(hist[:, 0]) == F          # the documented loss, made visible: only the bins of the 1e12 row are non-zero
        hb.set_gradients(v, plain_h)                                         # the same gradients through hist_build_kernel's two-word form
        _check(hb, bins, bo, None, g, hp, "gradients %s with per-row hessians, n=%d F=%d" % (name, n, F), model=both(m, hp_all))
    for name, v in _edge_arrays(rng, n, True).items():
        h = ref.Channel(v, True)
        hb.set_gradients(plain_g, v)
        hist, cnt, m = _check(hb, bins, bo, None, gp, h, "hessians %s, n=%d F=%d" % (name, n, F), model=both(gp_all, ref.histogram(bins, bo, None, None, h)))
        _check(hb, bins, bo, leaf, gp, h, "hessians %s, n=%d F=%d, leaf" % (name, n, F), model=both(gp_leaf, ref.histogram(bins, bo, leaf, None, h)))
        if name == "all zero":
            assert not hist[:, 1].any()
        if name == "one inf and one nan":
            assert np.isnan(hist[:, 1]).all() and np.isfinite(hist[:, 0]).all() and np.array_equal(cnt, m.counts)
    hb.close()


# ---- independence of order and of the split into leaves: against the model ----------------------------------------------------------------------------------------
@pytest.mark.parametrize("n,F", [(200000, 50), (600000, 64)])           # hist_build_kernel; the whole-row kernel for the lists of all rows
def test_order_and_leaf_independence_against_the_model(lib_built, n, F):
    from gpboost_amd import shim
    rng, bins, bo = _edge_bins(n, F, seed=n)
    grad = rng.standard_normal(n); hess = rng.uniform(0.5, 2.0, size=n)
    g, h = ref.Channel(grad, False), ref.Channel(hess, True)
    mask = rng.uniform(size=n) < 0.37
    left, right = np.flatnonzero(mask), np.flatnonzero(~mask)
    forms = [("identity list", np.arange(n)), ("permuted list", rng.permutation(n)), ("left", left), ("right", right)]
    hb = shim.HistBuilder(bins, bo)
    for hs, hc in ((None, None), (hess, h)):
        hb.set_gradients(grad, hs)
        ms = {}
        for name, rows in forms:
            mrows = None if name.endswith("list") else rows
            key = "all" if mrows is None else name
            if key not in ms:
                ms[key] = ref.histogram(bins, bo, mrows, g, hc)
            _check(hb, bins, bo, rows, g, hc, "%s, n=%d F=%d, %s hessian" % (name, n, F, "constant" if hs is None else "per-row"), model=ms[key])
        _check(hb, bins, bo, None, g, hc, "no list, n=%d F=%d" % (n, F), model=ms["all"])
        assert [x + y for x, y in zip(ms["left"].tot_g, ms["right"].tot_g)] == ms["all"].tot_g
        assert hc is None or [x + y for x, y in zip(ms["left"].tot_h, ms["right"].tot_h)] == ms["all"].tot_h
        assert np.array_equal(ms["left"].counts + ms["right"].counts, ms["all"].counts)
    hb.close()


# ---- the tree grower's launch site ---------------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("n,F,chunks", [(3000000, 50, 128), (120000, 1024, 8)])
def test_tree_grower_child_histograms_at_the_hessian_budget(lib_built, n, F, chunks):
    """hist_build_planned (the smaller child's build inside gpb_hip_hist_grow_tree): n = 3e6, hessians all 1.9, F = 50.  Column 0 carries the planted splits (mean gradient
    -1 / +0.2 / +1.5 on its bins 1..114 / 115..184 / 185..254 against noise of 0.5: hundreds of standard errors); column 1 holds 99 % of the rows in its most frequent bin 0,
    column 2 has two bins: the smaller child (45 % of the rows, 128 chunks: ~10500 rows per chunk) puts more than 4096 rows of one bin into a chunk at 1.9 * 2^50 each.
    F = 1024 (64 feature groups): at most 2 * 256 / 64 = 8 chunks, so NO reduce launch -- the children's search sums the chunk partials itself
    (ChildrenSearchArgs::part_hess / part_hess_hi) -- with ~6700 rows per chunk.
    The C ABI reports counts and leaf outputs of a tree, and the leaves' histograms through get_slot: those are compared."""
    from gpboost_amd import shim
    NB, L = 255, 3
    rng = np.random.default_rng(33)
    bins = rng.integers(1, NB, size=(F, n), dtype=np.uint8)
    bins[1] = np.where(rng.uniform(size=n) < 0.99, 0, rng.integers(1, NB, size=n))
    bins[2] = rng.integers(0, 2, size=n)
    b0 = bins[0].astype(np.int64)
    grad = np.where(b0 < 115, -1.0, np.where(b0 < 185, 0.2, 1.5)) + 0.5 * rng.standard_normal(n)
    hess = np.full(n, 1.9)
    gnb = np.full(F, NB, dtype=np.int32)
    bo = np.concatenate([[0], np.cumsum(gnb)]).astype(np.int32)
    meta3 = np.tile(np.array([1, 0, 0], dtype=np.int32), (F, 1))             # offset 1 (most_freq_bin 0), default bin 0, no missing type
    lambda_l2 = 0.5
    hb = shim.HistBuilder(bins, bo)
    hb.pool_resize(L + 1)
    hb.set_fix_info((bo[:-1] + 1).astype(np.int32), gnb, np.zeros(F, dtype=np.int32))
    hb.set_split_info(meta3[:, 0], meta3[:, 1], meta3[:, 2])
    hb.set_gradients(grad, hess)
    t = hb.grow_tree(L, float(np.cumsum(grad)[-1]), float(np.cumsum(hess)[-1]), lambda_l2, 20, 1e-3, 0.0)
    assert t["num_leaves"] == 3 and list(t["split_feature_inner"]) == [0, 0]
    thr = [int(x) for x in t["threshold_in_bin"]]
    assert thr[0] in (114, 184) and thr[1] in (114, 184) and thr[0] != thr[1], thr
    # rows of the root's children and of the three leaves, replayed on the bins (numerical split without missing values: bin <= threshold goes left)
    root_left = np.flatnonzero(b0 <= thr[0]); root_right = np.flatnonzero(b0 > thr[0])
    assert t["internal_count"][0] == n
    dli = t["data_leaf_index"]
    g, h = ref.Channel(grad, False), ref.Channel(hess, True)
    k_h = int(ref.quantise(np.array([1.9]), h.inv_q)[0])
    # the first split sends bin <= thr[0] to leaf 0 and the rest to leaf 1; the second one cuts the leaf that holds thr[1] and names its right part leaf 2
    want_leaf = np.where(b0 <= thr[0], 0, 1)
    if thr[1] < thr[0]:
        want_leaf[(b0 > thr[1]) & (b0 <= thr[0])] = 2
    else:
        want_leaf[b0 > thr[1]] = 2
    assert np.array_equal(dli, want_leaf)
    leaves = [np.flatnonzero(dli == i) for i in range(3)]
    for i, rows in enumerate(leaves):
        assert t["leaf_count"][i] == rows.size
        # leaf output = -sum_g / (sum_h + lambda_l2) from sums of histogram entries: against the model's exact integer totals over the leaf's rows, at the tolerance the
        # suite uses for leaf values against the reference (1e-9); one wrapped hessian partial moves sum_h by 16384 in ~5e6
        sum_g = float(Fraction(int(ref.quantise(grad[rows], g.inv_q).astype(object).sum())) * Fraction(g.q))
        sum_h = float(Fraction(k_h * rows.size) * Fraction(h.q))
        want = -sum_g / (sum_h + lambda_l2)
        print("leaf %d: %d rows, output %.17g, from the model's totals %.17g" % (i, rows.size, t["leaf_value"][i], want))
        assert abs(t["leaf_value"][i] - want) <= 1e-9 * abs(want), (i, t["leaf_value"][i], want)
    # the histograms left in the pool: slot 1 = the root's SMALLER child, built by hist_build_planned; slot 0 = root - smaller (one fp64 subtraction per entry)
    smaller = root_left if root_left.size < root_right.size else root_right
    ms = ref.histogram(bins, bo, smaller, g, h, want_exact=False)
    mr = ref.histogram(bins, bo, None, g, h, want_exact=False)
    s1, s0 = hb.get_slot(1), hb.get_slot(0)
    for name, got, want in (("smaller child", s1, ms.hist), ("larger child = root - smaller", s0, mr.hist - ms.hist)):
        bad = np.flatnonzero(got != want)
        print("%s: entries differing from the model: %d of %d (max |diff| %.6g)" % (name, bad.size, want.size, float(np.abs(got - want).max())))
        assert bad.size == 0, (name, bad[:5], got.ravel()[bad[:5]], want.ravel()[bad[:5]])
    assert smaller.size // chunks > 4096 * 1.4, "the case must sit above the 64-bit budget of a chunk (4096 rows at 2^51, 4311 at 1.9 * 2^50)"
    hb.close()
