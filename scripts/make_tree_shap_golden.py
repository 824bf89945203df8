"""Development machine only: writes tests/golden/tree_shap_ref.npz, the reference's own per-feature contributions of a small Booster.

The reference's unmodified Python package (the scratch copy under oracle/_ref/refpkg) on the reference library that build() puts in oracle/_ref trains a
plain regression Booster without a GP model -- n = 300, X uniform on (0, 1)^6 (no NaN, no zeros), use_missing=false, num_leaves=15, min_data_in_leaf=5,
4 rounds, one thread -- and the fixture keeps X, from dump_model() per tree the split feature, threshold, children, leaf values and leaf counts, and
predict(X, pred_contrib=True).  Data only.

    python scripts/make_tree_shap_golden.py
"""
import os
import sys
import types

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
REF_LIB = os.path.join(ROOT, "oracle", "_ref", "lib_gpboost_ref.so")
sys.modules.setdefault("optuna", types.ModuleType("optuna"))
fake = types.ModuleType("gpboost.libpath")
fake.find_lib_path = lambda: [REF_LIB]
sys.modules["gpboost.libpath"] = fake
sys.path.insert(0, os.path.join(ROOT, "oracle", "_ref", "refpkg"))
import gpboost as gpb         # noqa: E402   (the reference's package)


def flatten(tree_structure):
    """dump_model()'s nested tree -> arrays in the reference's numbering (split_index / leaf_index; children ~leaf for leaves)."""
    nl = 1 if "leaf_index" not in tree_structure and "split_index" not in tree_structure else None
    nodes, leaves = {}, {}

    def walk(nd):
        if "split_index" in nd:
            assert nd["decision_type"] == "<=", nd["decision_type"]
            kids = [walk(nd["left_child"]), walk(nd["right_child"])]
            nodes[nd["split_index"]] = (nd["split_feature"], nd["threshold"], kids[0], kids[1])
            return nd["split_index"]
        k = nd.get("leaf_index", 0)
        leaves[k] = (nd["leaf_value"], nd.get("leaf_count", 0))
        return ~k
    walk(tree_structure)
    nl = len(leaves)
    nn = nl - 1
    assert sorted(nodes) == list(range(nn)) and sorted(leaves) == list(range(nl))
    return dict(num_leaves=nl,
                split_feature=np.array([nodes[i][0] for i in range(nn)], dtype=np.int32),
                threshold=np.array([nodes[i][1] for i in range(nn)], dtype=np.float64),
                left_child=np.array([nodes[i][2] for i in range(nn)], dtype=np.int32),
                right_child=np.array([nodes[i][3] for i in range(nn)], dtype=np.int32),
                leaf_value=np.array([leaves[k][0] for k in range(nl)], dtype=np.float64),
                leaf_count=np.array([leaves[k][1] for k in range(nl)], dtype=np.int32))


def main():
    rng = np.random.default_rng(20240607)
    n, F = 300, 6
    X = rng.uniform(size=(n, F))
    X[X == 0.0] = 0.5
    y = np.sin(6 * X[:, 0]) + X[:, 1] * X[:, 2] + 0.5 * (X[:, 3] > 0.4) + 0.2 * rng.standard_normal(n)
    params = dict(objective="regression", num_leaves=15, min_data_in_leaf=5, use_missing=False, num_threads=1, verbose=-1, learning_rate=0.3,
                  deterministic=True, seed=1)
    bst = gpb.train(params=params, train_set=gpb.Dataset(X, y), num_boost_round=4)
    contrib = np.asarray(bst.predict(X, pred_contrib=True), dtype=np.float64)
    raw = np.asarray(bst.predict(X), dtype=np.float64)
    assert contrib.shape == (n, F + 1) and np.allclose(contrib.sum(axis=1), raw, rtol=0, atol=1e-10)
    model = bst.dump_model()
    out = dict(X=X, pred_contrib=contrib, num_trees=np.int32(len(model["tree_info"])))
    for i, ti in enumerate(model["tree_info"]):
        for k, v in flatten(ti["tree_structure"]).items():
            out["tree%d_%s" % (i, k)] = np.asarray(v)
        print("tree %d: %d leaves" % (i, out["tree%d_num_leaves" % i]))
    path = os.path.join(ROOT, "tests", "golden", "tree_shap_ref.npz")
    np.savez_compressed(path, **out)
    print("wrote", path, os.path.getsize(path), "bytes")


if __name__ == "__main__":
    main()
