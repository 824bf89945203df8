"""CPU: the path table of the per-feature contributions (gpb_hip_tree_shap_paths, host only -- the function the device path is built with) against the
Shapley definition in exact rational arithmetic, against a Python restatement of the table, and, run through the float64 path algorithm of
tests/tree_shap_ref.py, against the reference's own predict(..., pred_contrib=True) (tests/golden/tree_shap_ref.npz, scripts/make_tree_shap_golden.py)."""
import os
from fractions import Fraction

import numpy as np
import pytest

GOLDEN = os.path.join(os.path.dirname(__file__), "golden")

_SMALL = {}


def small_trees():
    """40 random trees, 10 per F in (1, 2, 3, 6), 1 to 13 leaves (a one-leaf tree and a 13-leaf tree per F; with F = 1 and 2 every tree of three leaves or more
    reuses a column on a path), 3 rows each.  -> list of (F, columns, tree, bins (F, 3)).  Built once per session, shared with the GPU tests."""
    if not _SMALL:
        from tests import tree_shap_ref as R
        rng = np.random.default_rng(4711)
        cases = []
        for F in (1, 2, 3, 6):
            col = R.random_columns(rng, F)
            for L in [1, 13] + [int(x) for x in rng.integers(2, 13, size=8)]:
                t = R.random_tree(rng, col, L)
                bins = np.stack([rng.integers(0, col["gnb"][f], size=3) for f in range(F)]).astype(np.uint8)
                cases.append((F, col, t, bins))
        _SMALL["cases"] = cases
    return _SMALL["cases"]


def test_small_trees_cover_the_cases():
    cases = small_trees()
    assert len(cases) == 40 and sorted({c[0] for c in cases}) == [1, 2, 3, 6]
    assert sum(c[2]["num_leaves"] == 1 for c in cases) == 4 and max(c[2]["num_leaves"] for c in cases) == 13
    assert all(1 <= c[2]["leaf_count"].min() and c[2]["leaf_count"].max() <= 999 for c in cases)


def test_path_table_reproduces_the_exact_definition(lib_built):
    """The library's table, run through the float64 path algorithm == the definition in Fractions, to 1e-13 * sum |v| per tree."""
    from gpboost_amd import shim
    from tests import tree_shap_ref as R
    reused = 0
    worst = 0.0
    for F, col, t, bins in small_trees():
        sets = R.node_sets(shim, col, t)
        left = R.unpack(sets) if t["num_leaves"] > 1 else np.zeros((0, 256), dtype=bool)
        first, column, s8, zero = shim.HistBuilder.tree_shap_paths(t, sets)
        assert first[0] == 0 and first.size == t["num_leaves"] + 1 and np.all(np.diff(first) >= 0) and first[-1] == column.size
        table = R.table_from_library(first, column, s8, zero)
        got = R.path_contrib(table, t["leaf_value"], bins, F, R.expected_value(t, t["leaf_value"], np.float64))
        scale = float(np.abs(t["leaf_value"]).sum())
        depth = max(R._depths(t)) if t["num_leaves"] > 1 else 0
        reused += any(len(cols) < d for (cols, _, _), d in zip(table, R._depths(t))) if t["num_leaves"] > 1 else 0
        for r in range(bins.shape[1]):
            want = R.exact_contrib(t, left, bins[:, r], F)
            err = max(abs(Fraction(float(g)) - w) for g, w in zip(got[r], want))
            worst = max(worst, float(err) / scale)
            assert err <= Fraction(1e-13) * Fraction(scale), (F, t["num_leaves"], r, float(err), scale, depth)
    print("largest deviation from the definition: %.3g of sum |v|; trees that reuse a column on a path: %d" % (worst, reused))
    assert reused >= 10


def test_zero_fractions_and_sets_are_the_restated_ones(lib_built):
    """Per leaf: the same columns in the same order as the Python restatement, sets == the AND of the node sets along the path (complemented for right turns),
    zero fractions == the exact ratios to 1e-15 * (number of factors), relative."""
    from gpboost_amd import shim
    from tests import tree_shap_ref as R
    checked = 0
    for F, col, t, bins in small_trees():
        sets = R.node_sets(shim, col, t)
        first, column, s8, zero = shim.HistBuilder.tree_shap_paths(t, sets)
        if t["num_leaves"] == 1:
            assert np.array_equal(first, [0, 0]) and column.size == 0
            continue
        table = R.table_from_library(first, column, s8, zero)
        for leaf, (p, (cols, masks, z)) in enumerate(zip(R.python_paths(t, R.unpack(sets)), table)):
            assert [e[0] for e in p] == [int(c) for c in cols], leaf
            for e, mask, zz in zip(p, masks, z):
                assert np.array_equal(e[1], mask), leaf
                assert abs(Fraction(float(zz)) - e[2]) <= Fraction(1e-15) * e[3] * e[2], (leaf, e[0], float(zz), float(e[2]), e[3])
                checked += 1
    assert checked > 300


def test_32_distinct_columns_are_accepted_and_33_refused(lib_built):
    import gpboost_amd
    from gpboost_amd import shim
    from tests import tree_shap_ref as R
    rng = np.random.default_rng(5)
    col = R.random_columns(rng, 40)
    col["is_cat"][:] = 0
    t32 = R.chain_tree(rng, col, list(range(32)))
    first, column, s8, zero = shim.HistBuilder.tree_shap_paths(t32, R.node_sets(shim, col, t32))
    assert np.array_equal(np.diff(first), list(range(1, 33)) + [32]) and np.array_equal(column[first[-2]:], np.arange(32))
    t33 = R.chain_tree(rng, col, list(range(33)))
    with pytest.raises(gpboost_amd.GPBoostError, match="leaf 32 has 33 distinct columns"):
        shim.HistBuilder.tree_shap_paths(t33, R.node_sets(shim, col, t33))
    # 33 nodes over 32 distinct columns (one repeated) are fine: elements are distinct columns, not nodes
    t33r = R.chain_tree(rng, col, list(range(32)) + [7])
    first, column, s8, zero = shim.HistBuilder.tree_shap_paths(t33r, R.node_sets(shim, col, t33r))
    assert first[-1] - first[-2] == 32
    bad = dict(t32); bad["leaf_count"] = t32["leaf_count"].copy(); bad["leaf_count"][5] = 0
    with pytest.raises(gpboost_amd.GPBoostError, match="leaf 5 has the count 0"):
        shim.HistBuilder.tree_shap_paths(bad, R.node_sets(shim, col, bad))


def fixture_forest():
    """tests/golden/tree_shap_ref.npz -> (columns, bins (F, n), trees in the numbering of the stored form, the reference's pred_contrib).  X is binned by each
    feature's sorted distinct thresholds, bin = number of thresholds < x, so that x <= threshold[k] is bin <= k: with most-frequent bin 0 and no missing
    type that is what node_go_left_mask produces for threshold_in_bin = k."""
    if "fixture" not in _SMALL:
        g = np.load(os.path.join(GOLDEN, "tree_shap_ref.npz"))
        X = g["X"]
        n, F = X.shape
        nt = int(g["num_trees"])
        thr = [np.unique(np.concatenate([g["tree%d_threshold" % i][g["tree%d_split_feature" % i] == f] for i in range(nt)])) for f in range(F)]
        bins = np.stack([np.searchsorted(thr[f], X[:, f], side="left") for f in range(F)]).astype(np.uint8)      # thresholds < x
        gnb = np.array([max(len(thr[f]) + 1, 2) for f in range(F)], dtype=np.int32)
        z = np.zeros(F, dtype=np.int32)
        col = dict(gnb=gnb, num_bin=gnb.copy(), mfb=z, is_cat=z, mt=z, db=z, bo=np.concatenate([[0], np.cumsum(gnb)]).astype(np.int32), offset=np.ones(F, dtype=np.int32))
        trees = []
        for i in range(nt):
            sf = g["tree%d_split_feature" % i]
            nn = sf.size
            t = dict(num_leaves=int(g["tree%d_num_leaves" % i]), split_feature_inner=sf.astype(np.int32), default_left=np.zeros(nn, dtype=np.int32),
                     threshold_in_bin=np.array([np.searchsorted(thr[f], v) for f, v in zip(sf, g["tree%d_threshold" % i])], dtype=np.int64),
                     left_child=g["tree%d_left_child" % i], right_child=g["tree%d_right_child" % i], leaf_value=g["tree%d_leaf_value" % i],
                     leaf_count=g["tree%d_leaf_count" % i], node_is_cat=np.zeros(nn, dtype=np.int32), node_cat_bits=np.zeros((nn, 8), dtype=np.uint32))
            assert all(thr[f][k] == v for f, k, v in zip(sf, t["threshold_in_bin"], g["tree%d_threshold" % i]))
            trees.append(t)
        _SMALL["fixture"] = (col, bins, trees, g["pred_contrib"])
    return _SMALL["fixture"]


def test_reference_pred_contrib_on_the_fixture(lib_built):
    """The library's tables of the reference's four trees, through the float64 path algorithm == the reference's predict(X, pred_contrib=True) to
    1e-13 * sum over trees of sum |v|; the binning rule is confirmed on the way (every row reaches the leaf the thresholds send it to)."""
    from gpboost_amd import shim
    from tests import tree_shap_ref as R
    from tests import test_zz_tree_predict_gpu as TP
    col, bins, trees, want = fixture_forest()
    F, n = bins.shape
    assert want.shape == (n, F + 1) and len(trees) == 4 and all(t["num_leaves"] == 15 for t in trees)
    g = np.load(os.path.join(GOLDEN, "tree_shap_ref.npz"))
    got = np.zeros((n, F + 1))
    scale = 0.0
    for i, t in enumerate(trees):
        lab = TP._numpy_leaves(shim, col, t, bins)
        node = np.zeros(n, dtype=np.int64)                       # the reference's own rule on the raw values: x <= threshold goes left
        for _ in range(t["num_leaves"] - 1):
            act = np.flatnonzero(node >= 0)
            k = node[act]
            node[act] = np.where(g["X"][act, t["split_feature_inner"][k]] <= g["tree%d_threshold" % i][k], t["left_child"][k], t["right_child"][k])
        assert np.array_equal(lab, ~node) and np.array_equal(np.bincount(lab, minlength=15), t["leaf_count"])
        table = R.table_from_library(*shim.HistBuilder.tree_shap_paths(t, R.node_sets(shim, col, t)))
        R.path_contrib(table, t["leaf_value"], bins, F, R.expected_value(t, t["leaf_value"], np.float64), out=got)
        scale += float(np.abs(t["leaf_value"]).sum())
    err = float(np.abs(got - want).max())
    print("largest deviation from the reference's pred_contrib: %.3g = %.3g of the scale %.3g" % (err, err / scale, scale))
    assert err <= 1e-13 * scale
