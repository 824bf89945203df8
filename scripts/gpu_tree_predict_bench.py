"""MI355X: time of one tree-scoring launch (gpb_hip_hist_add_score_dev's kernel; HIP events on the handle's stream, one warm-up launch, mean of REPS) at
n = 1e6 rows, F = 50 columns of 256 bins, random valid trees of 31 leaves: 1 tree and 100 trees, all rows and a 30 % out-of-bag row list.  Each time is set
against its traffic floor: (rows * fpad bytes of bins + 16 bytes of score per row) / the 6.29 TB/s measured copy rate.

    python scripts/gpu_tree_predict_bench.py [out.json]
"""
import json
import os
import sys

import numpy as np

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))

COPY_RATE = 6.29e12
REPS = 20


def random_tree(rng, F, L):
    nn = L - 1
    t = dict(num_leaves=L, leaf_value=rng.standard_normal(L), split_feature_inner=rng.integers(0, F, size=nn).astype(np.int32),
             default_left=np.zeros(nn, dtype=np.int32), threshold_in_bin=rng.integers(16, 240, size=nn).astype(np.int64))
    lc = np.zeros(nn, dtype=np.int32); rc = np.zeros(nn, dtype=np.int32)
    slot = {0: None}
    for k in range(nn):
        leaf = int(rng.choice(sorted(slot)))
        if slot[leaf] is not None:
            nd, side = slot[leaf]
            (lc if side == 0 else rc)[nd] = k
        lc[k] = ~leaf; rc[k] = ~(k + 1)
        slot[leaf] = (k, 0); slot[k + 1] = (k, 1)
    t["left_child"], t["right_child"] = lc, rc
    return t


def main():
    import gpboost_amd
    from gpboost_amd import shim
    assert gpboost_amd.device_count() > 0, "needs the MI355X"
    n, F, L, ntrees = 1000000, 50, 31, 100
    rng = np.random.default_rng(0)
    bins = rng.integers(0, 256, size=(F, n), dtype=np.uint8)
    bo = (256 * np.arange(F + 1)).astype(np.int32)
    hb = shim.HistBuilder(bins, bo)
    z = np.zeros(F, dtype=np.int32)
    hb.set_fix_info(bo[:-1], np.full(F, 256, dtype=np.int32), z)
    hb.set_split_info(np.ones(F, dtype=np.int32), z, z)
    trees = [random_tree(rng, F, L) for _ in range(ntrees)]
    for t in trees:
        hb.add_tree(t, shrinkage=0.1)
    oob = np.flatnonzero(rng.uniform(size=n) < 0.3).astype(np.int32)
    score = shim.DeviceBuffer(n).from_host(np.zeros(n))
    fpad = (F + 15) // 16 * 16
    out = dict(n=n, F=F, fpad=fpad, leaves=L, reps=REPS, copy_rate_TBps=COPY_RATE / 1e12, runs=[])
    for rep in range(3):                      # the whole set three times: the spread
        for nt in (1, ntrees):
            for name, rows in (("all_rows", None), ("oob_30pct", oob)):
                cnt = n if rows is None else rows.size
                ms = hb.add_score_bench(score.ptr, trees=(0, nt), rows=rows, reps=REPS)
                floor_ms = 1e3 * (cnt * fpad + 16.0 * cnt) / COPY_RATE
                out["runs"].append(dict(rep=rep, trees=nt, rows=name, cnt=int(cnt), ms=ms, floor_ms=floor_ms, ratio=ms / floor_ms))
                print("rep %d  %3d trees  %-9s  %8d rows  %8.4f ms   floor %7.4f ms   x %.2f" % (rep, nt, name, cnt, ms, floor_ms, ms / floor_ms), flush=True)
    # the labels of one tree against a host walk of the same tables (a check that what was timed computes the right thing)
    lab = hb.predict_leaf(0, rows=oob[:4096])
    t = trees[0]
    node = np.zeros(4096, dtype=np.int64)
    for _ in range(L - 1):
        act = np.flatnonzero(node >= 0)
        k = node[act]
        goes = bins[t["split_feature_inner"][k], oob[:4096][act]] <= t["threshold_in_bin"][k]
        node[act] = np.where(goes, t["left_child"][k], t["right_child"][k])
    assert np.array_equal(lab, (~node).astype(np.int32))
    out["labels_checked"] = 4096
    hb.close()
    line = json.dumps(out)
    print(line)
    if len(sys.argv) > 1:
        open(sys.argv[1], "w").write(line + "\n")


if __name__ == "__main__":
    main()
