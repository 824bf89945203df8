"""GPU: tree scoring on the device (gpb_hip_hist_predict_leaf / _add_score / _add_score_dev over stored trees) -- the leaf of rows OUTSIDE a tree's own
root (out-of-bag rows, a second matrix) and the score update of GBDT::UpdateScore.  Everything is compared bit by bit: labels against the grower's own
data_leaf_index, the reference's leaf_count (tests/golden/tree_ref*.npz) and the oracle's replay of the splits (DataPartition::Split); scores against the host
loop  for t: score[rows] += value_t[leaf_t[rows]]."""
import os

import numpy as np
import pytest

pytestmark = pytest.mark.gpu

GOLDEN = os.path.join(os.path.dirname(__file__), "golden")


class _Case(object):
    """One fixture tree case: the reference's Dataset columns and its tree, a HistBuilder set up as the grower needs it."""

    def __init__(self, name, hi):
        from gpboost_amd import shim
        from tests import cases
        self.name, self.hi = name, hi
        r5 = name in cases.TREE_CASES_R5
        g = np.load(os.path.join(GOLDEN, "tree_ref_r5.npz" if r5 else "tree_ref.npz"))
        data, params, self.L, self.cfg = cases.tree_params(name)
        X, self.grad, hess, leaf = cases.make_split_data(data)
        self.n = X.shape[0]
        k = "%s_hess%d_" % (name, hi)
        self.hess = hess if hi else None
        self.bins, self.gnb, self.mfb, self.meta3 = g[k + "bins"], g[k + "group_num_bin"], g[k + "most_freq_bin"], g[k + "meta3"]
        self.is_cat = g[k + "layout"][:, 3] if r5 else np.zeros(self.bins.shape[0], dtype=np.int32)
        self.ref = dict(num_leaves=int(g[k + "num_leaves"]))
        for key in ("split_feature_inner", "threshold_in_bin", "default_left", "left_child", "right_child", "leaf_value", "leaf_count"):
            self.ref[key] = g[k + key]
        if r5:
            self.ref["node_is_cat"] = g[k + "node_is_cat"]; self.ref["node_cat_bits"] = g[k + "node_cat_bits"]
        bo = np.concatenate([[0], np.cumsum(self.gnb)]).astype(np.int32)
        hb = shim.HistBuilder(self.bins, bo)
        hb.pool_resize(self.L + 1)
        hb.set_fix_info(g[k + "view_offset"], g[k + "num_bin"], self.mfb)
        hb.set_split_info(self.meta3[:, 0], self.meta3[:, 1], self.meta3[:, 2])
        if self.is_cat.any():
            hb.set_categorical(self.is_cat, *cases.tree_cat_cfg(name))
        if len(self.cfg) > 4:
            hb.set_regularisation(self.cfg[4], self.cfg[5], self.cfg[6])
        hb.set_max_depth(cases.tree_max_depth(name))
        self.hb = hb

    def grow(self, grad=None, rows=None):
        grad = self.grad if grad is None else grad
        hs = self.hess
        self.hb.set_gradients(grad, hs)
        sel = slice(None) if rows is None else rows
        sg = float(np.cumsum(grad[sel])[-1]); sh = float(np.cumsum((np.ones(self.n) if hs is None else hs)[sel])[-1])
        return self.hb.grow_tree(self.L, sg, sh, *self.cfg[:4])

    def replay(self, orc, t, bins):
        """Leaf of every column of `bins` (F, m): the tree's splits replayed with the oracle's DataPartition::Split (the loop of the grower's own test)."""
        m = bins.shape[1]
        lab = np.zeros(m, dtype=np.int32)
        leaf_of_node = {0: 0}
        nleaves = 1
        for nd in range(t["num_leaves"] - 1):
            lf = leaf_of_node[nd]
            rows = np.flatnonzero(lab == lf).astype(np.int32)
            f = int(t["split_feature_inner"][nd])
            if self.is_cat[f]:
                lte, gt = orc.split_leaf_layout(bins[f], 1, self.gnb[f] - 1, False, self.meta3[f, 1], self.mfb[f], self.meta3[f, 2], 0, 0, True, t["node_cat_bits"][nd], rows)
            else:
                lte, gt = orc.split_leaf(bins[f], self.gnb[f] - 1, self.meta3[f, 1], self.mfb[f], self.meta3[f, 2], int(t["default_left"][nd]),
                                         int(t["threshold_in_bin"][nd]), rows)
            lab[gt] = nleaves
            if t["left_child"][nd] >= 0:
                leaf_of_node[int(t["left_child"][nd])] = lf
            if t["right_child"][nd] >= 0:
                leaf_of_node[int(t["right_child"][nd])] = nleaves
            nleaves += 1
        return lab


@pytest.mark.parametrize("name,hi", [("plain_l31", 0), ("plain_l31", 1), ("nan_l20", 0), ("nan_l20", 1), ("zero_missing_l12", 0), ("plain_depth4", 0), ("cat_l15", 0),
                                     ("cat_onehot_l1", 0), ("efb_l15", 0)])
def test_stored_tree_labels_every_row_like_the_grower_and_the_reference(lib_built, name, hi):
    """grow -> keep_last_tree -> predict_leaf over all rows == the grower's data_leaf_index, leaf sizes == the REFERENCE's leaf_count; the reference's own
    arrays stored with add_tree (nothing grown) give the same labels."""
    c = _Case(name, hi)
    t = c.grow()
    tid = c.hb.keep_last_tree()
    assert tid == 0 and c.hb.forest_size() == 1
    lab = c.hb.predict_leaf(tid)
    assert lab.dtype == np.int32 and np.array_equal(lab, t["data_leaf_index"])
    assert np.array_equal(np.bincount(lab, minlength=c.ref["num_leaves"]), c.ref["leaf_count"])
    c.hb.close()
    c2 = _Case(name, hi)
    tid2 = c2.hb.add_tree(c.ref)
    assert np.array_equal(c2.hb.predict_leaf(tid2), lab)
    c2.hb.close()


def test_out_of_bag_rows(lib_built, orc):
    """A tree grown on a sorted bag of 70 % of the rows: in-bag labels are the grower's, out-of-bag labels the oracle's replay of the splits; add_score with the
    out-of-bag list changes exactly those entries; a list that is unsorted and has repeats adds once per occurrence (Tree::AddPredictionToScore's loop)."""
    c = _Case("plain_l31", 0)
    n = c.n
    rng = np.random.default_rng(77)
    bag = np.sort(rng.choice(n, size=int(0.7 * n), replace=False)).astype(np.int32)
    oob = np.setdiff1d(np.arange(n, dtype=np.int32), bag).astype(np.int32)
    c.hb.set_root_rows(bag)
    t = c.grow(rows=bag)
    assert t["num_leaves"] > 8 and np.all(t["data_leaf_index"][oob] == -1)
    tid = c.hb.keep_last_tree(0.1)
    lab = c.hb.predict_leaf(tid)
    assert np.array_equal(lab[bag], t["data_leaf_index"][bag])
    want = c.replay(orc, t, c.bins)
    assert np.array_equal(lab, want)
    assert np.array_equal(c.hb.predict_leaf(tid, rows=oob), want[oob])
    val = t["leaf_value"] * 0.1
    s0 = rng.standard_normal(n)
    s = s0.copy()
    c.hb.add_score(s, trees=tid, rows=oob)
    exp = s0.copy(); exp[oob] += val[want[oob]]
    assert np.array_equal(s, exp) and np.array_equal(s[bag], s0[bag]) and np.all(s[oob] != s0[oob])
    rep = rng.choice(n, size=3000, replace=True).astype(np.int32)
    assert np.unique(rep).size < rep.size and np.any(np.diff(rep) < 0)
    s = s0.copy()
    c.hb.add_score(s, trees=tid, rows=rep)
    exp = s0.copy()
    np.add.at(exp, rep, val[want[rep]])                      # unbuffered: one addition per occurrence, in list order
    assert np.array_equal(s, exp)
    assert np.array_equal(c.hb.predict_leaf(tid, rows=rep), want[rep])
    c.hb.close()


def _boost(n_trees=6, lr=0.1):
    c = _Case("plain_l31", 0)
    rng = np.random.default_rng(3)
    target = np.sin(np.arange(c.n) * 0.01) + 0.3 * rng.standard_normal(c.n)
    score = np.zeros(c.n)
    vals, labs = [], []
    for it in range(n_trees):
        t = c.grow(grad=score - target)
        tid = c.hb.keep_last_tree(lr)
        assert tid == it
        lab = c.hb.predict_leaf(tid)
        assert np.array_equal(lab, t["data_leaf_index"])
        vals.append(t["leaf_value"] * lr); labs.append(lab)
        score = score + vals[-1][lab]
    return c, score, vals, labs


def test_scores_of_a_boosting_loop_are_bit_identical_however_they_are_added(lib_built):
    """Six trees at learning rate 0.1 (gradients = score - target, constant hessian): one add_score over all trees == six single-tree calls == the numpy loop over
    value_t[leaf_t], bit for bit; add_score_dev on a device buffer gives the same bits (on a torch tensor: the test below); a second run of the whole loop too."""
    from gpboost_amd import shim
    c, score, vals, labs = _boost()
    n = c.n
    assert c.hb.forest_size() == 6
    base = np.random.default_rng(9).standard_normal(n)
    host = base.copy()
    for v, lab in zip(vals, labs):
        host[np.arange(n)] += v[lab]
    one = base.copy()
    c.hb.add_score(one)
    assert np.array_equal(one, host)
    six = base.copy()
    for tid in range(6):
        c.hb.add_score(six, trees=tid)
    assert np.array_equal(six, host)
    two = base.copy()
    c.hb.add_score(two, trees=(0, 4)); c.hb.add_score(two, trees=(4, 6))
    assert np.array_equal(two, host)
    dev = shim.DeviceBuffer(n).from_host(base)
    c.hb.add_score_dev(dev.ptr)
    c.hb.sync()
    assert np.array_equal(dev.to_host(), host)
    oob = np.flatnonzero(np.random.default_rng(1).uniform(size=n) < 0.3).astype(np.int32)
    dev2 = shim.DeviceBuffer(n).from_host(base)
    c.hb.add_score_dev(dev2.ptr, rows=oob)
    c.hb.add_score_dev(dev.ptr, trees=(0, 3), rows=oob)             # two calls in a row: the second one's row list waits for the first one's copy
    c.hb.sync()
    part = base.copy(); part[oob] = host[oob]
    assert np.array_equal(dev2.to_host(), part)
    # the booster's own score (built from single-tree updates on zeros) and a second run of everything
    z = np.zeros(n)
    c.hb.add_score(z)
    assert np.array_equal(z, score)
    c.hb.close()
    c2, score2, vals2, labs2 = _boost()
    z2 = np.zeros(n)
    c2.hb.add_score(z2)
    c2.hb.close()
    assert np.array_equal(z2, z) and all(np.array_equal(a, b) for a, b in zip(vals, vals2)) and all(np.array_equal(a, b) for a, b in zip(labs, labs2))


@pytest.mark.parametrize("name", ["plain_l31", "nan_l20", "zero_missing_l12", "cat_l15"])
def test_second_matrix(lib_built, orc, name):
    """set_pred_bins: row-permuted subsets of the training bins (1, 63, 64, 257 and all 6000 rows) get the training labels under the permutation; a matrix holding
    EVERY stored bin of every column (the NaN bin of a nan column, bins no training row of a leaf has) gets the oracle's replay; detached, pred=True is refused."""
    import gpboost_amd
    c = _Case(name, 0)
    t = c.grow()
    tid = c.hb.keep_last_tree()
    lab = c.hb.predict_leaf(tid)
    rng = np.random.default_rng(11)
    for m in (1, 63, 64, 257, c.n):
        perm = rng.permutation(c.n)[:m]
        c.hb.set_pred_bins(c.bins[:, perm])
        assert np.array_equal(c.hb.predict_leaf(tid, pred=True), lab[perm]), m
        sub = rng.permutation(m)[:max(1, m // 2)].astype(np.int32)
        assert np.array_equal(c.hb.predict_leaf(tid, rows=sub, pred=True), lab[perm][sub]), m
    F = c.bins.shape[0]
    m = 4 * int(c.gnb.max())
    P = np.stack([rng.integers(0, c.gnb[f], size=m) for f in range(F)]).astype(np.uint8)
    for f in range(F):
        P[f, :c.gnb[f]] = np.arange(c.gnb[f])
        P[f, m - c.gnb[f]:] = np.arange(c.gnb[f])[::-1]
    c.hb.set_pred_bins(P)
    want = c.replay(orc, t, P)
    assert np.array_equal(c.hb.predict_leaf(tid, pred=True), want)
    s = np.zeros(m)
    c.hb.add_score(s, pred=True)
    assert np.array_equal(s, t["leaf_value"][want])
    assert np.array_equal(c.hb.predict_leaf(tid), lab)                  # the training matrix is still there
    c.hb.set_pred_bins(None)
    with pytest.raises(gpboost_amd.GPBoostError, match="no second matrix is attached"):
        c.hb.predict_leaf(tid, pred=True)
    with pytest.raises(gpboost_amd.GPBoostError, match="no second matrix is attached"):
        c.hb.add_score(np.zeros(m), pred=True)
    c.hb.close()


# ---- synthetic columns and random valid trees: widths beyond one 64-byte sector, forests beyond one chunk of LDS ----
CHUNK_BYTES = 24576


def _tree_bytes(L):
    return (48 * (L - 1) + 8 * L + 15) // 16 * 16


def _random_columns(rng, F):
    """Per column: stored bins, most_freq_bin (0 or not), missing type, default_bin, categorical flag -- and what set_fix_info / set_split_info take."""
    gnb = rng.integers(2, 257, size=F).astype(np.int32)
    gnb[:3] = (256, 2, 3)
    mfb0 = rng.uniform(size=F) < 0.5
    num_bin = np.where(mfb0, gnb, gnb - 1).astype(np.int32)
    mfb0 |= num_bin < 2
    num_bin = np.where(mfb0, gnb, gnb - 1).astype(np.int32)
    mfb = np.array([0 if z else rng.integers(1, nb) for z, nb in zip(mfb0, num_bin)], dtype=np.int32)
    is_cat = (rng.uniform(size=F) < 0.3).astype(np.int32)
    mt = np.where(is_cat == 1, rng.choice([0, 2], size=F), rng.integers(0, 3, size=F)).astype(np.int32)
    db = np.array([rng.integers(0, nb) for nb in num_bin], dtype=np.int32)
    same = rng.uniform(size=F) < 0.3
    db[same] = mfb[same]
    bo = np.concatenate([[0], np.cumsum(gnb)]).astype(np.int32)
    return dict(gnb=gnb, num_bin=num_bin, mfb=mfb, is_cat=is_cat, mt=mt, db=db, bo=bo, offset=(mfb == 0).astype(np.int32))


def _random_tree(rng, col, L):
    """A valid tree in the reference's numbering: node k is the k-th split, the left child keeps the split leaf's id, the right child is the new leaf."""
    F = col["gnb"].size
    t = dict(num_leaves=L, leaf_value=rng.standard_normal(L))
    nn = L - 1
    sf = rng.integers(0, F, size=nn).astype(np.int32)
    t["split_feature_inner"] = sf
    t["default_left"] = rng.integers(0, 2, size=nn).astype(np.int32)
    t["node_is_cat"] = col["is_cat"][sf].astype(np.int32)
    t["node_cat_bits"] = rng.integers(0, 2 ** 32, size=(nn, 8), dtype=np.uint64).astype(np.uint32)
    t["node_cat_bits"][t["node_is_cat"] == 0] = 0
    thr = np.array([rng.integers(0, col["num_bin"][f]) for f in sf], dtype=np.int64) if nn else np.zeros(0, dtype=np.int64)
    cat_nodes = np.flatnonzero(t["node_is_cat"])
    thr[cat_nodes] = np.arange(cat_nodes.size)                 # a categorical node's threshold_in_bin is its running index
    t["threshold_in_bin"] = thr
    lc = np.zeros(nn, dtype=np.int32); rc = np.zeros(nn, dtype=np.int32)
    slot = {0: None}                                           # leaf -> (node, side) that points to it
    for k in range(nn):
        leaf = int(rng.choice(sorted(slot)))
        if slot[leaf] is not None:
            nd, side = slot[leaf]
            (lc if side == 0 else rc)[nd] = k
        lc[k] = ~leaf; rc[k] = ~(k + 1)
        slot[leaf] = (k, 0); slot[k + 1] = (k, 1)
    t["left_child"], t["right_child"] = lc, rc
    return t


def _numpy_leaves(shim, col, t, bins):
    """Plain traversal with the go-left sets of node_go_left_mask (pinned to the partition rule and to Tree::DecisionInner by tests/test_tree_predict_ref.py)."""
    m = bins.shape[1]
    nn = t["num_leaves"] - 1
    if nn == 0:
        return np.zeros(m, dtype=np.int32)
    left = np.zeros((nn, 256), dtype=bool)
    b = np.arange(256)
    for k in range(nn):
        f = int(t["split_feature_inner"][k])
        w = shim.HistBuilder.node_go_left_mask(col["gnb"][f] - 1, col["db"][f], col["mfb"][f], col["mt"][f], t["default_left"][k], t["threshold_in_bin"][k],
                                               cat_bits=t["node_cat_bits"][k] if t["node_is_cat"][k] else None)
        left[k] = ((w[b >> 5] >> (b & 31).astype(np.uint32)) & 1).astype(bool)
    node = np.zeros(m, dtype=np.int64)
    for _ in range(nn):
        act = np.flatnonzero(node >= 0)
        if act.size == 0:
            break
        k = node[act]
        goes = left[k, bins[t["split_feature_inner"][k], act]]
        node[act] = np.where(goes, t["left_child"][k], t["right_child"][k])
    assert np.all(node < 0)
    return (~node).astype(np.int32)


@pytest.mark.parametrize("F,n", [(50, 257), (50, 5000), (70, 257), (70, 5000), (200, 257)])
def test_wide_rows_and_forests_beyond_one_chunk(lib_built, F, n):
    """Random bins (F = 50: padded rows of 64 bytes, a compact copy exists; F = 70: 80 bytes; F = 200: 208 bytes, the 64-rows-per-workgroup form) and random valid
    trees of up to 255 leaves with numerical and categorical nodes over all three missing types, against a plain numpy traversal.
    Chunk rule (tree_predict_kernels.h): the trees of a call are taken in order and packed greedily into chunks of at most 24576 bytes of LDS, a tree of L leaves
    taking 48 (L - 1) + 8 L bytes rounded up to 16; the first tree that would overflow a chunk opens the next.  The forest here is 255, 255, 31, 1, 100, 255, 2
    leaves: a 255-leaf tree takes 14240 bytes, more than half a chunk, so the chunks are {0}, {1, 2, 3, 4}, {5, 6} and a call over all trees crosses two chunk
    boundaries; ranges inside and across chunks must give the same bits."""
    from gpboost_amd import shim
    rng = np.random.default_rng(1000 * F + n)
    col = _random_columns(rng, F)
    bins = np.stack([rng.integers(0, col["gnb"][f], size=n) for f in range(F)]).astype(np.uint8)
    hb = shim.HistBuilder(bins, col["bo"])
    hb.set_fix_info(col["bo"][:-1], col["num_bin"], col["mfb"])
    hb.set_split_info(col["offset"], col["db"], col["mt"])
    leaves = (255, 255, 31, 1, 100, 255, 2)
    sizes = [_tree_bytes(L) for L in leaves]
    assert sizes[0] == 14240 and 2 * sizes[0] > CHUNK_BYTES and sizes[1] + sizes[2] + sizes[3] + sizes[4] <= CHUNK_BYTES < sum(sizes[1:6])
    trees = [_random_tree(rng, col, L) for L in leaves]
    shr = 0.1
    for i, t in enumerate(trees):
        assert hb.add_tree(t, shrinkage=shr) == i
    labs = [_numpy_leaves(shim, col, t, bins) for t in trees]
    for i, t in enumerate(trees):
        assert np.array_equal(hb.predict_leaf(i), labs[i]), i
    assert len(np.unique(labs[0])) >= 8                      # (the inputs: the rows do spread over the leaves of a random tree)
    base = rng.standard_normal(n)
    host = base.copy()
    for t, lab in zip(trees, labs):
        host += (t["leaf_value"] * shr)[lab]
    s = base.copy()
    hb.add_score(s)
    assert np.array_equal(s, host)
    s = base.copy()
    for r in ((0, 2), (2, 3), (3, 6), (6, 7)):
        hb.add_score(s, trees=r)
    assert np.array_equal(s, host)
    rows = np.sort(rng.choice(n, size=n // 3, replace=False)).astype(np.int32)
    s = base.copy()
    hb.add_score(s, rows=rows)
    exp = base.copy(); exp[rows] = host[rows]
    assert np.array_equal(s, exp)
    # a tree of one leaf adds its value to every listed row
    s = base.copy()
    hb.add_score(s, trees=3, rows=rows)
    exp = base.copy(); exp[rows] += trees[3]["leaf_value"][0] * shr
    assert np.array_equal(s, exp) and np.all(hb.predict_leaf(3) == 0)
    # the attached matrix goes through the same kernel
    perm = rng.permutation(n)[:min(n, 300)]
    hb.set_pred_bins(bins[:, perm])
    assert np.array_equal(hb.predict_leaf(5, pred=True), labs[5][perm])
    hb.forest_clear()
    assert hb.forest_size() == 0 and hb.add_tree(trees[2]) == 0
    assert np.array_equal(hb.predict_leaf(0), labs[2])
    hb.close()


_TORCH_CHILD = r"""
import sys
import numpy as np
import torch
torch.cuda.init()                                   # torch opens the device first, the library joins it
sys.path.insert(0, sys.argv[1])
from gpboost_amd import shim
from tests import test_zz_tree_predict_gpu as T
rng = np.random.default_rng(21)
F, n, shr = 50, 5000, 0.1
col = T._random_columns(rng, F)
bins = np.stack([rng.integers(0, col["gnb"][f], size=n) for f in range(F)]).astype(np.uint8)
hb = shim.HistBuilder(bins, col["bo"])
hb.set_fix_info(col["bo"][:-1], col["num_bin"], col["mfb"])
hb.set_split_info(col["offset"], col["db"], col["mt"])
trees = [T._random_tree(rng, col, L) for L in (31, 63, 1, 255, 255)]
for t in trees:
    hb.add_tree(t, shrinkage=shr)
base = rng.standard_normal(n)
loop = base.copy()
for i, t in enumerate(trees):
    loop += (t["leaf_value"] * shr)[hb.predict_leaf(i)]
host = base.copy()
hb.add_score(host)
dev = torch.from_numpy(base.copy()).to("cuda")
torch.cuda.synchronize()
hb.add_score_dev(dev.data_ptr())
hb.sync()
got = dev.cpu().numpy()
assert np.array_equal(got, host) and np.array_equal(got, loop)
rows = np.flatnonzero(rng.uniform(size=n) < 0.3).astype(np.int32)
dev = torch.from_numpy(base.copy()).to("cuda")
torch.cuda.synchronize()
hb.add_score_dev(dev.data_ptr(), rows=rows)
hb.sync()
part = base.copy(); part[rows] = loop[rows]
assert np.array_equal(dev.cpu().numpy(), part)
hb.close()
print("TORCH_OK")
"""


def test_add_score_dev_on_a_torch_tensor(lib_built):
    """add_score_dev on a float64 torch tensor's data_ptr() gives the bits of add_score and of the host loop.  In a process of its own: torch has to open the
    device before the library does, and in this session the library already has."""
    import subprocess
    import sys
    root = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    r = subprocess.run([sys.executable, "-c", _TORCH_CHILD, root], capture_output=True, text=True, timeout=600)
    assert r.returncode == 0 and "TORCH_OK" in r.stdout, r.stdout[-2000:] + r.stderr[-4000:]


def test_refusals(lib_built):
    """Every refusal is a GPBoostError with its message, raised before anything is launched: the forest and later calls are untouched."""
    import gpboost_amd
    from gpboost_amd import shim
    E = gpboost_amd.GPBoostError
    rng = np.random.default_rng(2)
    F, n = 6, 300
    col = _random_columns(rng, F)
    col["is_cat"][:] = 0; col["is_cat"][4] = 1
    bins = np.stack([rng.integers(0, col["gnb"][f], size=n) for f in range(F)]).astype(np.uint8)
    hb = shim.HistBuilder(bins, col["bo"])
    good = _random_tree(rng, col, 9)
    with pytest.raises(E, match="feature metas have not been set"):
        hb.add_tree(good)
    with pytest.raises(E, match="no tree has been grown"):
        hb.keep_last_tree()
    hb.set_fix_info(col["bo"][:-1], col["num_bin"], col["mfb"])
    hb.set_split_info(col["offset"], col["db"], col["mt"])
    assert hb.add_tree(good) == 0
    lab = hb.predict_leaf(0)

    def broken(**kw):
        t = {k: np.array(v, copy=True) if isinstance(v, np.ndarray) else v for k, v in good.items()}
        for k, (i, v) in kw.items():
            t[k][i] = v
        return t
    bad = [("splits column", broken(split_feature_inner=(0, F))),
           ("children are later nodes", broken(left_child=(2, 2))),                    # a node that is its own child: a cycle
           ("children are later nodes", broken(right_child=(3, 1))),                   # a child that points backwards
           ("children are later nodes", broken(left_child=(0, 8))),                    # a node index past the last node
           ("points to leaf", broken(right_child=(0, ~9))),
           ("is referenced", broken(right_child=(7, ~0)))]                              # a leaf twice, another never
    for msg, t in bad:
        with pytest.raises(E, match=msg):
            hb.add_tree(t)
    cat_node = broken(split_feature_inner=(0, 4))
    cat_node["node_is_cat"][0] = 1
    no_set = dict(cat_node); no_set["node_cat_bits"] = None
    with pytest.raises(E, match="categorical node without a set"):
        hb.add_tree(no_set)
    hb.set_categorical(col["is_cat"])
    no_flags = dict(cat_node); no_flags["node_is_cat"] = None; no_flags["node_cat_bits"] = None
    with pytest.raises(E, match="categorical node without a set"):
        hb.add_tree(no_flags)
    with pytest.raises(E, match="num_leaves = 0"):
        hb.add_tree(dict(good, num_leaves=0))
    big = _random_tree(rng, col, 440)
    with pytest.raises(E, match="does not fit"):
        hb.add_tree(big)
    assert hb.forest_size() == 1
    for call in (lambda: hb.predict_leaf(1), lambda: hb.predict_leaf(-1), lambda: hb.add_score(np.zeros(n), trees=(1, 1)), lambda: hb.add_score(np.zeros(n), trees=(0, 2))):
        with pytest.raises(E, match="unknown tree id or empty range"):
            call()
    for rows in ([n], [-1], [0, 5, n + 7]):
        with pytest.raises(E, match="outside the matrix"):
            hb.predict_leaf(0, rows=np.array(rows, dtype=np.int32))
        with pytest.raises(E, match="outside the matrix"):
            hb.add_score(np.zeros(n), rows=np.array(rows, dtype=np.int32))
    with pytest.raises(E, match="no second matrix is attached"):
        hb.predict_leaf(0, pred=True)
    hb.set_pred_bins(bins[:, :10])
    with pytest.raises(E, match="outside the matrix"):
        hb.predict_leaf(0, rows=np.array([10], dtype=np.int32), pred=True)
    assert np.array_equal(hb.predict_leaf(0), lab) and np.array_equal(hb.predict_leaf(0, pred=True), lab[:10])
    assert hb.predict_leaf(0, rows=np.zeros(0, dtype=np.int32)).size == 0
    hb.close()
