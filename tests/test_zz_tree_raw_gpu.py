"""GPU: stored trees scored on RAW feature rows (float64 / float32, no binning; pred="raw" -> which = 2, tree_raw_kernels.hip) against a plain numpy restatement of
Tree::Decision (include/LightGBM/tree.h:329-401).  Leaves are integers and scores are compared bit for bit with  for t: s[rows] += value_t[leaf_t[rows]]."""
import numpy as np
import pytest

from tests import test_zz_tree_predict_gpu as TP

pytestmark = pytest.mark.gpu
LEAVES = (255, 255, 31, 1, 100, 255, 2)       # raw forms of 10168 bytes + bitsets, ...: every 255-leaf tree is a 12288-byte chunk of its own, {31, 1, 100} share one
TYPES = [np.float64, np.float32]


def _goes_left(x, thr, dt, cb, ct):      # Tree::Decision of one node on float64 values; dt: bit 0 categorical, bit 1 default-left, bits 2-3 missing None / Zero / NaN
    mt, nan = (dt >> 2) & 3, np.isnan(x)
    if dt & 1:
        lo, hi = int(cb[int(thr)]), int(cb[int(thr) + 1])
        c = np.where(~nan & (x >= -2.0 ** 31) & (x < 2.0 ** 31), x, -1.0).astype(np.int64)       # (int)x truncates; outside the int range: right
        if mt != 2:
            c[nan] = 0                                                                        # NaN: right under missing type NaN, else category 0
        ok = (c >= 0) & (c < 32 * (hi - lo))
        cc = np.where(ok, c, 0)
        return ok & (((ct[lo + (cc >> 5)] >> (cc & 31).astype(np.uint32)) & 1) == 1)
    if mt != 2:
        x = np.where(nan, 0.0, x)
    kz = np.float64(np.float32(1e-35))                                                        # kZeroThreshold = 1e-35f
    default = ((mt == 1) & (x >= -kz) & (x <= kz)) | ((mt == 2) & nan)
    return np.where(default, bool(dt & 2), x <= thr)


def _leaves(t, X):
    X = X.astype(np.float64)                                                                  # exact for float32
    node = np.zeros(X.shape[0], dtype=np.int64) if t["num_leaves"] > 1 else np.full(X.shape[0], -1)
    while (node >= 0).any():
        for k in np.unique(node[node >= 0]):
            act = np.flatnonzero(node == k)
            left = _goes_left(X[act, t["split_feature_inner"][k]], t["threshold"][k], int(t["decision_type"][k]), t["cat_boundaries"], t["cat_threshold"])
            node[act] = np.where(left, t["left_child"][k], t["right_child"][k])
    return (~node).astype(np.int32)


def _handle(F):                     # F two-bin columns: the bin forms of the trees below are valid and never used
    from gpboost_amd import shim
    two, z = np.full(F, 2, dtype=np.int32), np.zeros(F, dtype=np.int32)
    hb = shim.HistBuilder(np.zeros((F, 4), dtype=np.uint8), np.arange(0, 2 * F + 1, 2, dtype=np.int32))
    hb.set_fix_info(2 * np.arange(F, dtype=np.int32), two, z)
    hb.set_split_info(z + 1, z, z)
    return dict(gnb=two, num_bin=two, is_cat=z), hb


def _raw_tree(rng, col, L):      # a random valid tree + raw rule: a third of the nodes categorical (bitsets of 1 to 3 words), random thresholds, missing types, directions
    t = TP._random_tree(rng, col, L)
    cat = rng.uniform(size=L - 1) < 1 / 3
    t["threshold"] = np.where(cat, np.cumsum(cat) - 1, rng.standard_normal(L - 1))
    t["decision_type"] = (cat | (rng.integers(0, 2, size=L - 1) << 1) | (rng.integers(0, 3, size=L - 1) << 2)).astype(np.int8)
    t["cat_boundaries"] = np.concatenate([[0], np.cumsum(rng.integers(1, 4, size=int(cat.sum())))]).astype(np.int32)
    t["cat_threshold"] = rng.integers(0, 2 ** 32, size=int(t["cat_boundaries"][-1]), dtype=np.uint64).astype(np.uint32)
    return t


def _stump(thr, dt, cb=None, ct=None):
    one = np.zeros(1, dtype=np.int32)
    return dict(num_leaves=2, split_feature_inner=one, threshold_in_bin=one, default_left=one, left_child=one - 1, right_child=one - 2, leaf_value=np.array([1.0, 2.0]),
                threshold=np.array([float(thr)]), decision_type=np.array([dt], dtype=np.int8), cat_boundaries=cb, cat_threshold=ct)


@pytest.mark.parametrize("default_left", [0, 1])
@pytest.mark.parametrize("mt", [0, 1, 2])
@pytest.mark.parametrize("T", TYPES)
def test_decision_table(lib_built, T, mt, default_left):
    """Two numerical stumps (thresholds 0.5 and 0.0) on the values at which the rule can go wrong, each in the row's own type."""
    col, hb = _handle(1)
    z, inf = T(np.float32(1e-35)), T(np.inf)
    vals = [T(np.nan), T(0.0), T(-0.0), z, -z, np.nextafter(z, inf), np.nextafter(-z, -inf), T(1e-36), np.nextafter(T(0), inf), inf, -inf,
            T(3e38 if T is np.float32 else 1e300), T(-3e38 if T is np.float32 else -1e300)]
    for thr in (T(0.5), T(0.0)):
        vals += [thr, np.nextafter(thr, inf), np.nextafter(thr, -inf)]
    X = np.array(vals, dtype=T).reshape(-1, 1)
    hb.set_pred_raw(X)
    for tid, thr in enumerate((0.5, 0.0)):
        t = _stump(thr, (default_left << 1) | (mt << 2))
        assert hb.add_tree(t) == tid
        got, want = hb.predict_leaf(tid, pred="raw"), _leaves(t, X)
        assert np.array_equal(got, want), (thr, X[got != want].ravel())


@pytest.mark.parametrize("mt", [0, 2])
@pytest.mark.parametrize("T", TYPES)
def test_categorical_table(lib_built, T, mt):
    """A categorical stump whose 3-word bitset holds {0, 3, 31, 32, 95}; values outside the int range go right."""
    col, hb = _handle(1)
    t = _stump(0, 1 | (mt << 2), np.array([0, 3], dtype=np.int32), np.array([1 | 8 | 1 << 31, 1, 1 << 31], dtype=np.uint32))
    X = np.array([-1, -0.5, 0, 3, 3.7, 31, 32, 95, 96, 1000, np.nan, 3e9, -3e9, np.inf], dtype=T).reshape(-1, 1)
    hb.set_pred_raw(X)
    got = hb.predict_leaf(hb.add_tree(t), pred="raw")
    assert np.array_equal(got, _leaves(t, X)) and np.all(got[-3:] == 1)
    assert np.array_equal(got[:10], [1, 0, 0, 0, 0, 0, 0, 0, 1, 1]) and got[10] == (1 if mt == 2 else 0)


@pytest.mark.parametrize("T", TYPES)
@pytest.mark.parametrize("F,n", [(1, 130), (7, 257), (50, 257), (50, 5000)])
def test_forest_shapes(lib_built, F, n, T):
    """Seven trees across chunk boundaries, a tenth NaN, a tenth exact zeros: leaves, one call, split ranges, a shuffled list with repeats, a borrowed device matrix."""
    from gpboost_amd import shim
    rng = np.random.default_rng(100 * F + n)
    col, hb = _handle(F)
    trees = [_raw_tree(rng, col, L) for L in LEAVES]
    assert [hb.add_tree(t, shrinkage=0.1) for t in trees] == list(range(len(trees)))
    hb.set_raw_rule(2, *[trees[2][k] for k in ("threshold", "decision_type", "cat_boundaries", "cat_threshold")])      # again: its raw form now lies behind tree 6's
    X = np.where(rng.uniform(size=(n, F)) < 0.5, rng.standard_normal((n, F)), rng.uniform(-2, 100, size=(n, F)))
    u = rng.uniform(size=(n, F))
    X[u < 0.1] = np.nan; X[u > 0.9] = 0.0
    X = np.ascontiguousarray(X, dtype=T)
    hb.set_pred_raw(X)
    labs = [_leaves(t, X) for t in trees]
    assert all(np.array_equal(hb.predict_leaf(i, pred="raw"), labs[i]) for i in range(len(trees)))
    assert len(np.unique(labs[0])) >= (4 if F == 1 else 8)         # (the inputs: the rows do spread over the leaves; one column reaches few)
    vals = [t["leaf_value"] * 0.1 for t in trees]
    base = rng.standard_normal(n)
    host = base.copy()
    for v, lab in zip(vals, labs):
        host += v[lab]
    assert np.array_equal(hb.add_score(base.copy(), pred="raw"), host)
    s = base.copy()
    for r in ((0, 2), (2, 3), (3, 7)):
        hb.add_score(s, trees=r, pred="raw")
    assert np.array_equal(s, host)
    rows = rng.permutation(n)[:n // 3]; rows = rng.permutation(np.concatenate([rows, rows[:2]])).astype(np.int32)
    exp = base.copy()
    for v, lab in zip(vals, labs):
        np.add.at(exp, rows, v[lab[rows]])                     # one addition per occurrence; rows not listed keep their bits
    assert np.array_equal(hb.add_score(base.copy(), rows=rows, pred="raw"), exp)
    raw = np.concatenate([X, np.full((n, 3), np.nan, dtype=T)], axis=1).tobytes()
    buf = shim.DeviceBuffer((len(raw) + 7) // 8).from_host(np.frombuffer(raw.ljust((len(raw) + 7) // 8 * 8, b"\0"), dtype=np.float64))
    hb.set_pred_raw_dev(buf.ptr, n, T, row_stride=F + 3)
    sc = shim.DeviceBuffer(n).from_host(base)
    hb.add_score_dev(sc.ptr, pred="raw")
    hb.sync()
    assert np.array_equal(sc.to_host(), host)


@pytest.mark.parametrize("name", ["plain_l31", "cat_l15"])
def test_raw_and_binned_paths_agree(lib_built, name):
    """A grown tree, its rule made by raw_rule_from_bins from mappers chosen here (numerical bin b = (b, b + 1], categorical bin b = a random category); X lies in its bins."""
    from gpboost_amd import shim
    c = TP._Case(name, 0)
    t = c.grow()
    tid = c.hb.keep_last_tree(0.1)
    F, n = c.bins.shape
    rng = np.random.default_rng(5)
    fb = np.where(c.bins == 0, c.mfb[:, None], c.bins.astype(np.int64) - 1 + (c.mfb[:, None] == 0))       # stored bin -> the mapper's bin (the most frequent one is stored as 0)
    ub = [np.arange(256) + 1.0 for f in range(F)]
    b2c = [rng.permutation(300)[:256] for f in range(F)]
    X = np.stack([b2c[f][fb[f]] if c.is_cat[f] else fb[f] + rng.uniform(0.1, 0.9, size=n) for f in range(F)], axis=1).astype(np.float64)
    c.hb.set_raw_rule(tid, **shim.HistBuilder.raw_rule_from_bins(t, ub, c.meta3[:, 2], b2c))
    c.hb.set_pred_raw(np.ascontiguousarray(X))
    assert t["num_leaves"] > 8 and (name != "cat_l15" or t["node_is_cat"].any())
    assert np.array_equal(c.hb.predict_leaf(tid, pred="raw"), c.hb.predict_leaf(tid))
    base = rng.standard_normal(n)
    assert np.array_equal(c.hb.add_score(base.copy(), pred="raw"), c.hb.add_score(base.copy()))


def test_reference_fixture(lib_built):
    """The reference's four trees (tests/golden/tree_shap_ref.npz: trained with use_missing=false on data without NaN, every dump_model node "<=" with missing type
    None, so decision_type = default-left | None = 2) with their real thresholds: raw scores == binned scores bit for bit == the sum of the contributions."""
    from tests.test_tree_shap_ref import fixture_forest, small_trees
    from tests.test_zz_tree_shap_gpu import _builder
    from gpboost_amd import shim
    small_trees()                    # that module's session cache is filled in this order by its own tests; it only builds the small trees while it is empty
    col, bins, trees, want = fixture_forest()
    g = np.load(TP.GOLDEN + "/tree_shap_ref.npz")
    hb = _builder(shim, col, bins)
    for i, t in enumerate(trees):
        assert hb.add_tree(dict(t, threshold=g["tree%d_threshold" % i], decision_type=np.full(t["num_leaves"] - 1, 2, dtype=np.int8))) == i
    hb.set_pred_raw(np.ascontiguousarray(g["X"], dtype=np.float64))
    n = bins.shape[1]; raw = hb.add_score(np.zeros(n), pred="raw")
    assert np.array_equal(raw, hb.add_score(np.zeros(n)))
    err = float(np.abs(raw - hb.pred_contrib().sum(axis=1)).max())
    assert err <= 1e-13 * sum(float(np.abs(t["leaf_value"]).sum()) for t in trees), err


def test_refusals(lib_built):
    """Every refusal is raised before any launch; afterwards the forest answers as before."""
    from gpboost_amd import GPBoostError as E
    rng = np.random.default_rng(8)
    col, hb = _handle(3)
    assert hb.add_tree(_raw_tree(rng, col, 9)) == 0 and hb.add_tree(TP._random_tree(rng, col, 5)) == 1
    X = rng.standard_normal((20, 3))
    for call in (lambda: hb.predict_leaf(0, pred="raw"), lambda: hb.add_score(np.zeros(0), pred="raw")):
        with pytest.raises(E, match="no raw matrix is attached"):
            call()
    hb.set_pred_raw(X)
    lab = hb.predict_leaf(0, pred="raw")
    base = dict(threshold=np.zeros(4), decision_type=np.zeros(4, dtype=np.int8))
    big = hb.add_tree(TP._random_tree(rng, col, 320))
    bad = [("unknown tree id", 7, base), ("missing type 3", 1, dict(base, decision_type=[12, 0, 0, 0])), ("non-finite threshold", 1, dict(base, threshold=[0, np.inf, 0, 0])),
           ("outside num_cat", 1, dict(threshold=[1, 0, 0, 0], decision_type=[1, 0, 0, 0], cat_boundaries=[0, 1], cat_threshold=[5])),
           ("not ascending", 1, dict(base, cat_boundaries=[0, 2, 2], cat_threshold=[1, 1])),
           ("does not fit", big, dict(threshold=np.zeros(319), decision_type=np.zeros(319, dtype=np.int8)))]
    for msg, tid, kw in bad:
        with pytest.raises(E, match=msg):
            hb.set_raw_rule(tid, **kw)
        with pytest.raises(E, match="tree 1 has no raw rule"):
            hb.add_score(np.zeros(20), pred="raw")
    for M in (X[:, :2].copy(), np.zeros((5, 4)), X.astype(np.int64), np.asfortranarray(X)):
        with pytest.raises(ValueError):
            hb.set_pred_raw(M)
    with pytest.raises(E, match="outside the matrix"):
        hb.predict_leaf(0, rows=np.array([20], dtype=np.int32), pred="raw")
    with pytest.raises(E, match="contributions need binned rows"):
        hb.pred_contrib(trees=0, pred="raw")
    col2, hb2 = _handle(104)
    with pytest.raises(E, match="GPB_TR_MAX_COLS_F64 = 103"):
        hb2.set_pred_raw(np.zeros((4, 104)))
    hb2.set_pred_raw(np.zeros((4, 104), dtype=np.float32))            # 104 float32 columns are within GPB_TR_MAX_COLS_F32 = 207
    assert np.array_equal(hb.predict_leaf(0, pred="raw"), lab) and hb.forest_size() == 3
