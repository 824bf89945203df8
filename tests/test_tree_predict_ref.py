"""CPU: the per-node go-left sets of tree scoring (gpb_hip_hist_node_go_left_mask, host only) against the two rules they must agree with:
the partition rule the tree grower splits rows with (the oracle's DenseBin::SplitInner / SplitCategoricalInner, already pinned to the
reference's DataPartition::Split), and the reference's PREDICTION rule, Tree::DecisionInner on the feature's bin, restated here.  Everything is
compared bit by bit."""
import os

import numpy as np
import pytest

GOLDEN = os.path.join(os.path.dirname(__file__), "golden")


def _bits(mask8, nbits):
    m = np.asarray(mask8, dtype=np.uint32)
    b = np.arange(nbits)
    return ((m[b >> 5] >> (b & 31).astype(np.uint32)) & 1).astype(bool)


def _columns():
    """(num_bin, most_freq_bin, max_bin) of single-feature columns: stored bin 0 = the most frequent bin, the other bins follow from 1 on, so a column
    has num_bin stored bins when most_freq_bin == 0 and num_bin + 1 otherwise (uint8 storage: at most 256)."""
    out = []
    for num_bin in (1, 2, 3, 5, 64, 256):
        for mfb in sorted({0, num_bin // 2, num_bin - 2, num_bin - 1}):      # 0, interior, the last two bins (max_bin == most_freq_bin + 1: the NaN column whose
            if mfb < 0 or mfb >= num_bin:                                  # most frequent bin is the NaN bin)
                continue
            stored = num_bin if mfb == 0 else num_bin + 1
            if stored <= 256:
                out.append((num_bin, mfb, stored - 1))
    return out


def test_numerical_masks_are_the_partition_rule(lib_built, orc):
    """Bit b of the mask == does a row whose stored bin is b land in lte of orc.split_leaf -- for every stored bin of the column, every threshold, the
    three missing types, default_bin equal and unequal to most_freq_bin, both default directions, one-bin columns (max_bin <= 1) included.  The partition
    decides row by row, so all stored bins are asked in one column; the small columns are asked one one-row column per bin as well."""
    from gpboost_amd import shim
    cols = _columns()
    assert any(mb <= 1 for _, _, mb in cols) and any(mb == 255 for _, _, mb in cols)
    checked = 0
    for num_bin, mfb, max_bin in cols:
        allbins = np.arange(max_bin + 1, dtype=np.uint8)
        rows = np.arange(max_bin + 1, dtype=np.int32)
        for mt in (0, 1, 2):
            for default_bin in sorted({mfb, (mfb + 1) % num_bin}):
                for dl in (0, 1):
                    for thr in range(num_bin):
                        mask = shim.HistBuilder.node_go_left_mask(max_bin, default_bin, mfb, mt, dl, thr)
                        got = _bits(mask, max_bin + 1)
                        lte, gt = orc.split_leaf(allbins, max_bin, default_bin, mfb, mt, dl, thr, rows)
                        want = np.zeros(max_bin + 1, dtype=bool); want[lte] = True
                        assert np.array_equal(got, want), (num_bin, mfb, mt, default_bin, dl, thr, np.flatnonzero(got != want))
                        checked += 1
                        if num_bin <= 5:
                            for b in range(max_bin + 1):
                                lte1, _ = orc.split_leaf(np.array([b], dtype=np.uint8), max_bin, default_bin, mfb, mt, dl, thr, np.zeros(1, dtype=np.int32))
                                assert bool(lte1.size) == bool(got[b]), (num_bin, mfb, mt, default_bin, dl, thr, b)
    assert checked > 5000


def test_categorical_masks_are_the_partition_rule(lib_built, orc):
    """The same for sets of bins (random 256-bit sets, empty and full) against orc.split_leaf_layout's DenseBin::SplitCategoricalInner, most_freq_bin 0 and > 0."""
    from gpboost_amd import shim
    rng = np.random.default_rng(5)
    checked = 0
    for num_bin, mfb, max_bin in _columns():
        allbins = np.arange(max_bin + 1, dtype=np.uint8)
        rows = np.arange(max_bin + 1, dtype=np.int32)
        sets = [np.zeros(8, dtype=np.uint32), np.full(8, 0xffffffff, dtype=np.uint32)] + [rng.integers(0, 2 ** 32, size=8, dtype=np.uint64).astype(np.uint32) for _ in range(12)]
        for bits in sets:
            for mt in (0, 2):
                mask = shim.HistBuilder.node_go_left_mask(max_bin, 0, mfb, mt, 0, 0, cat_bits=bits)
                got = _bits(mask, max_bin + 1)
                lte, gt = orc.split_leaf_layout(allbins, 1, max_bin, False, 0, mfb, mt, 0, 0, True, bits, rows)
                want = np.zeros(max_bin + 1, dtype=bool); want[lte] = True
                assert np.array_equal(got, want), (num_bin, mfb, mt, bits, np.flatnonzero(got != want))
                checked += 1
    assert checked > 300


def _decision_inner_goes_left(fbin, thr, default_left, missing_type, default_bin, max_bin_feature, cat_bits):
    """Tree::DecisionInner (include/LightGBM/tree.h:349-409) on the FEATURE's bin: NumericalDecisionInner / CategoricalDecisionInner (FindInBitset)."""
    if cat_bits is not None:
        w = fbin >> 5
        return w < 8 and bool((int(cat_bits[w]) >> (fbin & 31)) & 1)
    if (missing_type == 1 and fbin == default_bin) or (missing_type == 2 and fbin == max_bin_feature):
        return bool(default_left)
    return fbin <= thr


def _feature_bin(stored, max_stored, mfb):
    """DenseBinIterator::Get (src/LightGBM/io/dense_bin.hpp:483-490) of a single-feature group: min_bin = 1, max_bin = stored bins - 1, offset = (mfb == 0)."""
    if 1 <= stored <= max_stored:
        return stored - 1 + (1 if mfb == 0 else 0)
    return mfb


_DISAGREE = {}


def _mask_vs_decision_inner(fixture):
    """-> (nodes, (node, stored bin) pairs compared, the pairs where the mask bit differs from Tree::DecisionInner as (case, node, column, stored bin, most_freq_bin,
    is the stored bin one that occurs in the fixture's column)) over every node of every reference tree of the fixture and every stored bin of the node's column."""
    if fixture in _DISAGREE:
        return _DISAGREE[fixture]
    from gpboost_amd import shim
    g = np.load(os.path.join(GOLDEN, fixture))
    cases = sorted(k[:-len("num_leaves")] for k in g.files if k.endswith("_num_leaves"))
    assert len(cases) >= 12
    nodes = pairs = 0
    bad = []
    for k in cases:
        gnb, num_bin, mfb, meta3, bins = g[k + "group_num_bin"], g[k + "num_bin"], g[k + "most_freq_bin"], g[k + "meta3"], g[k + "bins"]
        is_cat = g[k + "node_is_cat"] if k + "node_is_cat" in g.files else None
        for nd in range(int(g[k + "num_leaves"]) - 1):
            f = int(g[k + "split_feature_inner"][nd])
            thr, dl = int(g[k + "threshold_in_bin"][nd]), int(g[k + "default_left"][nd])
            bits = g[k + "node_cat_bits"][nd] if (is_cat is not None and is_cat[nd]) else None
            max_stored = int(gnb[f]) - 1
            mask = shim.HistBuilder.node_go_left_mask(max_stored, meta3[f, 1], mfb[f], meta3[f, 2], dl, thr, cat_bits=bits)
            got = _bits(mask, max_stored + 1)
            want = np.array([_decision_inner_goes_left(_feature_bin(s, max_stored, int(mfb[f])), thr, dl, int(meta3[f, 2]), int(meta3[f, 1]), int(num_bin[f]) - 1, bits)
                             for s in range(max_stored + 1)])
            nodes += 1; pairs += max_stored + 1
            for s in np.flatnonzero(got != want):
                bad.append((k, nd, f, int(s), int(mfb[f]), bool(np.any(bins[f] == s))))
    _DISAGREE[fixture] = (nodes, pairs, bad)
    return _DISAGREE[fixture]


@pytest.mark.parametrize("fixture", ["tree_ref.npz", "tree_ref_r5.npz"])
def test_masks_are_the_reference_prediction_rule_on_the_fixture_trees(lib_built, fixture):
    """The partition rule and the reference's prediction rule are the same function of the stored bin: for every node of every reference tree in the fixture and
    every stored bin of the node's column, the mask bit equals Tree::DecisionInner on the bin the dense bin iterator gives for that stored bin.

    The stored bins of a column are the codes its encoding assigns (FeatureGroup::PushData, include/LightGBM/feature_group.h:199-214): 0 for the most frequent bin
    and, for every other bin, bin + 1 when most_freq_bin > 0 (bin itself when it is 0).  With most_freq_bin > 0 that leaves ONE code of the uint8 range
    0 .. num_bin unassigned, most_freq_bin + 1: no row can hold it, and none of the fixture does (checked).  It is compared all the same, and there -- and only there --
    the reference's two rules are NOT the same function.  FINDING, pinned below: node 1 of zero_missing_l12 (hess0 and hess1), column 1, missing type Zero,
    most_freq_bin = default_bin = 31, threshold 37, default_left 0, code 32: DenseBinIterator::Get would map it to the feature's bin 31 = default_bin, which
    NumericalDecisionInner sends by default_left (right); DenseBin::SplitInner compares a stored bin other than 0 with the threshold (32 <= 38: left), because it
    expects the rows of the most frequent bin at stored bin 0.  The masks follow the partition rule at that code (the tests above pin them to it for every value
    0 .. max_bin), so a row is always scored the way it was split.  2 of the 34374 + 6885 compared (node, code) pairs."""
    nodes, pairs, bad = _mask_vs_decision_inner(fixture)
    assert nodes > 100 and pairs > 5000
    for k, nd, f, s, mfb, occurs in bad:                      # every stored bin agrees; a difference can only sit on the unassigned code, which no row holds
        assert mfb > 0 and s == mfb + 1 and not occurs, (k, nd, f, s, mfb, occurs)
    want = [("zero_missing_l12_hess0_", 1, 1, 32, 31, False), ("zero_missing_l12_hess1_", 1, 1, 32, 31, False)] if fixture == "tree_ref.npz" else []
    assert bad == want, bad


def test_mask_arguments_are_checked(lib_built):
    import gpboost_amd
    from gpboost_amd import shim
    with pytest.raises(gpboost_amd.GPBoostError):
        shim.HistBuilder.node_go_left_mask(256, 0, 0, 0, 0, 3)
    with pytest.raises(gpboost_amd.GPBoostError):
        shim.HistBuilder.node_go_left_mask(10, 0, 0, 3, 0, 3)
