"""GPU: per-feature contributions (TreeSHAP) of stored trees on the device -- shim.HistBuilder.set_leaf_counts / tree_expected_value / add_contrib /
add_contrib_dev / pred_contrib (gpb_hip_hist_add_contrib*, tree_shap_kernels.hip) against the Shapley definition in exact rational arithmetic, the path
algorithm in long double (tests/tree_shap_ref.py), the reference's own pred_contrib (tests/golden/tree_shap_ref.npz), and bit by bit against itself.

Tolerances.  Against the definition and the long-double path algorithm: 1e-13 * sum |stored leaf value| per tree, summed over the trees of a call -- the
float64 path algorithm is within 3.6e-16 of that scale of its long-double run on paths of up to 16 distinct columns, and the forests here are asserted to
stay at or below 16, so the bound has a margin of about 250.  Deep paths (24 and 32 distinct columns): the algorithm's own rounding error grows about 100x
per 8 further columns, so the bound there is the float64 helper's largest deviation from the long-double helper on the same inputs, as measured by the test,
times 16 (room for a different but algebraically equal order of operations), floored at 1e-13 * sum |v|."""
import numpy as np
import pytest

from fractions import Fraction

pytestmark = pytest.mark.gpu

_CACHE = {}


def _builder(shim, col, bins):
    hb = shim.HistBuilder(bins, col["bo"])
    hb.set_fix_info(col["bo"][:-1], col["num_bin"], col["mfb"])
    hb.set_split_info(col["offset"], col["db"], col["mt"])
    return hb


def _longdouble_forest(R, shim, col, trees, shr, bins):
    """Long-double path algorithm over the Python restatement of the path tables (exact zero fractions rounded once to long double) -> (m, F + 1) long
    double, the scale sum over trees of sum |stored v|, the largest number of elements on a path."""
    F = bins.shape[0]
    out = np.zeros((bins.shape[1], F + 1), dtype=np.longdouble)
    scale, emax = 0.0, 0
    for t in trees:
        vals = t["leaf_value"] * shr                             # rounded once, as the stored tree's
        if t["num_leaves"] > 1:
            paths = R.python_paths(t, R.unpack(R.node_sets(shim, col, t)))
            emax = max(emax, max(len(p) for p in paths))
            table = R.table_from_python(paths, np.longdouble)
        else:
            table = [((), (), ())]
        R.path_contrib(table, vals, bins, F, R.expected_value(t, vals, np.longdouble), np.longdouble, out=out)
        scale += float(np.abs(vals).sum())
    return out, scale, emax


@pytest.mark.parametrize("F", [1, 2, 3, 6])
def test_definition(lib_built, F):
    """The CPU test's small trees of this F, all stored on one HistBuilder with n = 130 rows (neither a multiple of 64 nor a single wave): pred_contrib of every
    tree == the exact Shapley values at 40 rows to 1e-13 * sum |v|; all trees in one call == their exact sum."""
    from gpboost_amd import shim
    from tests import tree_shap_ref as R
    from tests.test_tree_shap_ref import small_trees
    cases = [c for c in small_trees() if c[0] == F]
    assert len(cases) == 10
    col = cases[0][1]
    rng = np.random.default_rng(130 + F)
    n = 130
    bins = np.stack([rng.integers(0, col["gnb"][f], size=n) for f in range(F)]).astype(np.uint8)
    hb = _builder(shim, col, bins)
    for i, (_, _, t, _) in enumerate(cases):
        assert hb.add_tree(t) == i
    rows = np.sort(rng.choice(n, size=40, replace=False)).astype(np.int32)
    total = [[Fraction(0)] * (F + 1) for _ in rows]
    worst = 0.0
    for i, (_, _, t, _) in enumerate(cases):
        got = hb.pred_contrib(trees=i)
        assert got.shape == (n, F + 1) and got.dtype == np.float64
        left = R.unpack(R.node_sets(shim, col, t)) if t["num_leaves"] > 1 else None
        scale = float(np.abs(t["leaf_value"]).sum())
        for j, r in enumerate(rows):
            want = R.exact_contrib(t, left, bins[:, r], F)
            total[j] = [a + b for a, b in zip(total[j], want)]
            err = max(abs(Fraction(float(g)) - w) for g, w in zip(got[r], want))
            worst = max(worst, float(err) / scale)
            assert err <= Fraction(1e-13) * Fraction(scale), (i, t["num_leaves"], int(r), float(err), scale)
    allt = hb.pred_contrib(rows=rows)
    assert allt.shape == (40, F + 1)
    scale = sum(float(np.abs(c[2]["leaf_value"]).sum()) for c in cases)
    for j in range(40):
        assert max(abs(Fraction(float(g)) - w) for g, w in zip(allt[j], total[j])) <= Fraction(1e-13) * Fraction(scale)
    print("F = %d: largest deviation from the definition %.3g of sum |v|" % (F, worst))
    hb.close()


LEAVES = (255, 255, 31, 1, 100, 255, 2)


def _forest(F, n):
    """The forest of the scoring tests' shapes -- leaves (255, 255, 31, 1, 100, 255, 2), shrinkage 0.1 -- with leaf counts, stored on a HistBuilder; the
    long-double reference on all rows (n = 5000: on 200 sampled rows).  Built once per (F, n)."""
    if (F, n) not in _CACHE:
        from gpboost_amd import shim
        from tests import tree_shap_ref as R
        rng = np.random.default_rng(7001 * F + n)                # (seeds at which the longest path has at most 16 distinct columns: 16, 14, 16, 15)
        col = R.random_columns(rng, F)
        bins = np.stack([rng.integers(0, col["gnb"][f], size=n) for f in range(F)]).astype(np.uint8)
        hb = _builder(shim, col, bins)
        trees = [R.random_tree(rng, col, L) for L in LEAVES]
        shr = 0.1
        for i, t in enumerate(trees):
            assert hb.add_tree(t, shrinkage=shr) == i
        rows = np.arange(n, dtype=np.int32) if n <= 257 else np.sort(rng.choice(n, size=200, replace=False)).astype(np.int32)
        ref, scale, emax = _longdouble_forest(R, shim, col, trees, shr, bins[:, rows])
        _CACHE[(F, n)] = dict(hb=hb, col=col, bins=bins, trees=trees, shr=shr, rows=rows, ref=ref, scale=scale, emax=emax, rng=rng)
    return _CACHE[(F, n)]


@pytest.mark.parametrize("F,n", [(50, 257), (70, 257), (200, 257), (50, 5000)])
def test_forest_shapes(lib_built, F, n):
    """Padded rows of 64, 80 and 208 bytes; trees of 1, 2 and 255 leaves with numerical and categorical nodes over all three missing types: pred_contrib ==
    the long-double path algorithm to 1e-13 * sum |v| per tree, summed; paths hold at most 16 distinct columns; at n = 5000 (20 workgroups of 256 rows) the
    row sums over all rows == add_score on zeros (local accuracy) to the same tolerance."""
    fo = _forest(F, n)
    hb = fo["hb"]
    assert fo["emax"] <= 16, fo["emax"]
    got = hb.pred_contrib()
    assert got.shape == (n, F + 1)
    err = float(np.abs(got[fo["rows"]].astype(np.longdouble) - fo["ref"]).max())
    print("(F, n) = (%d, %d): largest deviation from the long-double path algorithm %.3g = %.3g of the scale; longest path %d columns"
          % (F, n, err, err / fo["scale"], fo["emax"]))
    assert err <= 1e-13 * fo["scale"]
    if n == 5000:
        s = np.zeros(n)
        hb.add_score(s)
        dev = float(np.abs(got.sum(axis=1) - s).max())
        print("local accuracy: largest |row sum - score| %.3g" % dev)
        assert dev <= 1e-13 * fo["scale"]
    if (F, n) != (50, 257):                                      # (50, 257) is shared with test_bits
        hb.close(); del _CACHE[(F, n)]


def _followable_chain(R, shim, rng, col, columns):
    """A chain tree whose every node has stored bins on both sides (thresholds redrawn until it has): a row can follow the chain to its end."""
    t = R.chain_tree(rng, col, columns)
    for k, f in enumerate(columns):
        for _ in range(200):
            left = R.unpack(R.node_sets(shim, col, t)[k])[:col["gnb"][f]]
            if left.any() and not left.all():
                break
            t["threshold_in_bin"][k] = rng.integers(0, col["num_bin"][f]); t["default_left"][k] = rng.integers(0, 2)
        else:
            raise AssertionError("column %d cannot be split both ways" % f)
    return t


@pytest.mark.parametrize("nu", [24, 32])
def test_deep_paths(lib_built, nu):
    """Chain trees over 24 and 32 distinct columns (F = 40, n = 257; a quarter of the rows are steered right along the chain, every other one of them to its
    end).  Tolerance: 16 x the float64 helper's measured deviation from the long-double helper, floored at 1e-13 * sum |v| (module docstring).
    Measured on the MI355X (of sum |v|): 24 columns: helper 1.0e-14, device 8.3e-15; 32 columns: helper 6.4e-13, device 7.2e-13."""
    from gpboost_amd import shim
    from tests import tree_shap_ref as R
    rng = np.random.default_rng(2400 + nu)
    F, n = 40, 257
    col = R.random_columns(rng, F)
    col["is_cat"][:] = 0
    bins = np.stack([rng.integers(0, col["gnb"][f], size=n) for f in range(F)]).astype(np.uint8)
    columns = [int(c) for c in rng.permutation(F)[:nu]]
    t = _followable_chain(R, shim, rng, col, columns)
    sets = R.node_sets(shim, col, t)
    left = R.unpack(sets)
    for r in range(0, n, 4):
        depth = nu if r % 8 == 0 else int(rng.integers(1, nu + 1))
        for k in range(depth):
            f = columns[k]
            bins[f, r] = np.flatnonzero(~left[k][:col["gnb"][f]])[0]
    from tests import test_zz_tree_predict_gpu as TP
    lab = TP._numpy_leaves(shim, col, t, bins)
    assert (lab >= nu - 1).sum() >= 30                           # rows at the last node's two leaves: all nu columns decided their way
    paths = R.python_paths(t, left)
    assert max(len(p) for p in paths) == nu
    vals = t["leaf_value"]
    scale = float(np.abs(vals).sum())
    ld = R.path_contrib(R.table_from_python(paths, np.longdouble), vals, bins, F, R.expected_value(t, vals, np.longdouble), np.longdouble)
    f64 = R.path_contrib(R.table_from_library(*shim.HistBuilder.tree_shap_paths(t, sets)), vals, bins, F, R.expected_value(t, vals, np.float64))
    helper = float(np.abs(f64.astype(np.longdouble) - ld).max())
    tol = max(16.0 * helper, 1e-13 * scale)
    hb = _builder(shim, col, bins)
    assert hb.add_tree(t) == 0
    got = hb.pred_contrib()
    err = float(np.abs(got.astype(np.longdouble) - ld).max())
    print("%d distinct columns: float64 helper %.3g, device %.3g of sum |v| (tolerance %.3g)" % (nu, helper / scale, err / scale, tol / scale))
    assert err <= tol
    hb.close()


def test_bits(lib_built):
    """On the (50, 257) forest: one call == the ranges (0,2), (2,3), (3,6), (6,7) in turn; a row's result is the same in a call over all rows, over a shuffled
    third of them and through set_pred_bins of a permuted copy; add_contrib_dev on a DeviceBuffer == add_contrib; rows not listed keep their bits; column F
    == the sequential sum of tree_expected_value."""
    from gpboost_amd import shim
    fo = _forest(50, 257)
    hb, n, F, rng = fo["hb"], 257, 50, np.random.default_rng(99)
    base = rng.standard_normal((n, F + 1))
    one = base.copy()
    assert hb.add_contrib(one) is one
    assert np.mean(one != base) > 0.9                            # (the inputs: 7 random trees use nearly every one of the 50 columns)
    parts = base.copy()
    for r in ((0, 2), (2, 3), (3, 6), (6, 7)):
        hb.add_contrib(parts, trees=r)
    assert np.array_equal(parts, one)
    single = base.copy()
    for t in range(7):
        hb.add_contrib(single, trees=t)
    assert np.array_equal(single, one)
    rows = rng.permutation(n)[:n // 3].astype(np.int32)
    assert np.any(np.diff(rows) < 0)
    third = base.copy()
    hb.add_contrib(third, rows=rows)
    rest = np.setdiff1d(np.arange(n), rows)
    assert np.array_equal(third[rows], one[rows]) and np.array_equal(third[rest], base[rest])
    assert np.array_equal(hb.pred_contrib(rows=rows), hb.pred_contrib()[rows])
    perm = rng.permutation(n)
    hb.set_pred_bins(fo["bins"][:, perm])
    second = base[perm].copy()
    hb.add_contrib(second, pred=True)
    assert np.array_equal(second, one[perm])
    sub = rng.permutation(n)[:100].astype(np.int32)
    second = base[perm].copy()
    hb.add_contrib(second, rows=sub, pred=True)
    assert np.array_equal(second[sub], one[perm][sub])
    hb.set_pred_bins(None)
    dev = shim.DeviceBuffer(n * (F + 1)).from_host(base.ravel())
    hb.add_contrib_dev(dev.ptr, trees=(0, 4))
    hb.add_contrib_dev(dev.ptr, trees=(4, 7), rows=rows)         # two calls in a row, the second with a row list
    hb.add_contrib_dev(dev.ptr, trees=(4, 7), rows=rest.astype(np.int32))
    hb.sync()
    assert np.array_equal(dev.to_host().reshape(n, F + 1), one)
    s = base[:, F].copy()
    for t in range(7):
        s = s + hb.tree_expected_value(t)
    assert np.array_equal(s, one[:, F])
    assert hb.tree_expected_value(3) == fo["trees"][3]["leaf_value"][0] * fo["shr"]      # a tree of one leaf: its stored value
    hb.close(); del _CACHE[(50, 257)]


@pytest.mark.parametrize("name,bag", [("plain_l31", False), ("cat_l15", False), ("plain_l31", True)])
def test_grown_trees(lib_built, name, bag):
    """A tree grown on the device (all rows / a 70 % bag): keep_last_tree records its counts itself and gives the bits of add_tree of the dict grow_tree
    returned; the expected value == sum count / total * (value * shrinkage) in leaf order to 1e-15, relative; the contributions of every row -- out-of-bag
    rows included -- sum to its add_score value."""
    from tests.test_zz_tree_predict_gpu import _Case
    c = _Case(name, 0)
    n, F = c.n, c.bins.shape[0]
    shr = 0.1
    rows = None
    if bag:
        rows = np.sort(np.random.default_rng(77).choice(n, size=int(0.7 * n), replace=False)).astype(np.int32)
        c.hb.set_root_rows(rows)
    t = c.grow(rows=rows)
    assert t["num_leaves"] > 8 and t["leaf_count"].sum() == (n if rows is None else rows.size)
    kept = c.hb.keep_last_tree(shr)
    added = c.hb.add_tree(t, shrinkage=shr)
    assert (kept, added) == (0, 1)
    a = c.hb.pred_contrib(trees=kept)
    assert np.array_equal(a, c.hb.pred_contrib(trees=added))
    total = float(t["leaf_count"].sum())
    ev = 0.0
    for cnt, v in zip(t["leaf_count"], t["leaf_value"]):
        ev += (float(cnt) / total) * (v * shr)
    got_ev = c.hb.tree_expected_value(kept)
    assert abs(got_ev - ev) <= 1e-15 * abs(ev) and c.hb.tree_expected_value(added) == got_ev
    assert np.array_equal(a[:, F], np.full(n, got_ev))
    s = np.zeros(n)
    c.hb.add_score(s, trees=kept)
    scale = float(np.abs(t["leaf_value"] * shr).sum())
    dev = np.abs(a.sum(axis=1) - s)
    oob = np.arange(n) if rows is None else np.setdiff1d(np.arange(n), rows)
    print("%s bag=%s: largest |row sum - score| %.3g of sum |v| (out-of-bag rows: %.3g)" % (name, bag, dev.max() / scale, dev[oob].max() / scale))
    assert dev.max() <= 1e-13 * scale
    if bag:
        assert oob.size > 1000 and np.all(t["data_leaf_index"][oob] == -1)
        assert np.array_equal(c.hb.pred_contrib(trees=kept, rows=oob.astype(np.int32)), a[oob])
    c.hb.close()


def test_reference(lib_built):
    """The reference's four trees (tests/golden/tree_shap_ref.npz) through the device == its predict(X, pred_contrib=True) to 1e-13 * sum over trees sum |v|."""
    from gpboost_amd import shim
    from tests.test_tree_shap_ref import fixture_forest
    col, bins, trees, want = fixture_forest()
    hb = _builder(shim, col, bins)
    for i, t in enumerate(trees):
        assert hb.add_tree(t) == i
    got = hb.pred_contrib()
    scale = sum(float(np.abs(t["leaf_value"]).sum()) for t in trees)
    err = float(np.abs(got - want).max())
    print("largest deviation from the reference's pred_contrib %.3g = %.3g of the scale" % (err, err / scale))
    assert err <= 1e-13 * scale
    hb.close()


def test_refusals(lib_built):
    """Every refusal is a GPBoostError with its message, raised before anything is launched: the forest and later calls are untouched."""
    import gpboost_amd
    from gpboost_amd import shim
    from tests import tree_shap_ref as R
    E = gpboost_amd.GPBoostError
    rng = np.random.default_rng(12)
    F, n = 40, 300
    col = R.random_columns(rng, F)
    col["is_cat"][:] = 0
    bins = np.stack([rng.integers(0, col["gnb"][f], size=n) for f in range(F)]).astype(np.uint8)
    hb = _builder(shim, col, bins)
    good = R.random_tree(rng, col, 9)
    assert hb.add_tree(good) == 0
    want = hb.pred_contrib()
    bare = {k: v for k, v in R.random_tree(rng, col, 5).items() if k != "leaf_count"}
    assert hb.add_tree(bare) == 1
    with pytest.raises(E, match="tree 1 has no leaf counts"):
        hb.pred_contrib()
    with pytest.raises(E, match="has no leaf counts"):
        hb.tree_expected_value(1)
    with pytest.raises(E, match="leaf 2 has the count 0"):
        hb.set_leaf_counts(1, [5, 3, 0, 2, 9])
    with pytest.raises(E, match="leaf 0 has the count -4"):
        hb.set_leaf_counts(1, [-4, 3, 1, 2, 9])
    with pytest.raises(E, match="has no leaf counts"):              # the refused counts left nothing behind
        hb.pred_contrib(trees=1)
    for tid in (2, -1):
        with pytest.raises(E, match="unknown tree id"):
            hb.set_leaf_counts(tid, [1, 2, 3])
    with pytest.raises(E, match="unknown tree id"):
        hb.tree_expected_value(2)
    t33 = R.chain_tree(rng, col, list(range(33)))
    with pytest.raises(E, match="leaf 32 has 33 distinct columns"):
        hb.add_tree(t33)                                           # (the tree itself is stored, as tree 2: scoring needs no table)
    assert hb.forest_size() == 3
    with pytest.raises(E, match="tree 2 has no leaf counts"):
        hb.pred_contrib(trees=2)
    with pytest.raises(E, match="row 7 is listed twice"):
        hb.pred_contrib(trees=0, rows=np.array([3, 7, 11, 7], dtype=np.int32))
    for rows in ([n], [-1], [0, 5, n + 7]):
        with pytest.raises(E, match="outside the matrix"):
            hb.pred_contrib(trees=0, rows=np.array(rows, dtype=np.int32))
    with pytest.raises(E, match="no second matrix is attached"):
        hb.pred_contrib(trees=0, pred=True)
    with pytest.raises(E, match="no second matrix is attached"):
        hb.add_contrib_dev(shim.DeviceBuffer(8).ptr, trees=0, pred=True)
    for tr in ((0, 0), (1, 0), (0, 4), 3, -1):
        with pytest.raises(E, match="unknown tree id or empty range"):
            hb.pred_contrib(trees=tr)
    for out in (np.zeros((n, F)), np.zeros((n + 1, F + 1)), np.zeros(n * (F + 1)), np.zeros((n, F + 1), dtype=np.float32), np.zeros((F + 1, n)).T):
        with pytest.raises(E, match="out must"):
            hb.add_contrib(out, trees=0)
    # later calls: the counts arrive, the forest answers as before
    hb.set_leaf_counts(1, [5, 3, 1, 2, 9])
    assert np.array_equal(hb.pred_contrib(trees=0), want)
    both = hb.pred_contrib(trees=(0, 2))
    assert np.array_equal(both[:, F], (np.zeros(n) + hb.tree_expected_value(0)) + hb.tree_expected_value(1))
    assert hb.pred_contrib(trees=0, rows=np.zeros(0, dtype=np.int32)).shape == (0, F + 1)
    s = np.zeros(n)
    hb.add_score(s, trees=(0, 3))                                  # scoring is unaffected by a tree without a table
    assert np.all(s != 0)
    hb.close()
