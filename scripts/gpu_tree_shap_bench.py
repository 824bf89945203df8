"""MI355X: time of one contribution launch (gpb_hip_hist_add_contrib_dev's kernel; HIP events on the handle's stream, one warm-up launch, mean of REPS) at
n = 1e5 and 1e6 rows, F = 50 columns of 256 bins, random valid trees of 31 leaves with leaf counts uniform in 1 .. 999: 1, 10 and 100 trees, all rows.
Each time is set against the kernel's own fp64 work: per row and leaf of E path elements 9 E^2 + 9 E plain multiplications and
additions (extend 2 E^2 + 4 E, unwind 7 E^2 + 5 E), plus one addition per tree -- at 39.3 T plain fp64 operations per second (the 78.6 TFLOP/s vector peak
counts a fused multiply-add as two; the kernel is compiled without contraction).

    python scripts/gpu_tree_shap_bench.py [out.json]
"""
import json
import os
import sys

import numpy as np

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
from scripts.gpu_tree_predict_bench import random_tree      # noqa: E402

PLAIN_FP64_RATE = 39.3e12
REPS = 5


def main():
    import gpboost_amd
    from gpboost_amd import shim
    assert gpboost_amd.device_count() > 0, "needs the MI355X"
    F, L, ntrees = 50, 31, 100
    rng = np.random.default_rng(0)
    bo = (256 * np.arange(F + 1)).astype(np.int32)
    z = np.zeros(F, dtype=np.int32)
    trees = [random_tree(rng, F, L) for _ in range(ntrees)]
    for t in trees:
        t["leaf_count"] = rng.integers(1, 1000, size=L).astype(np.int32)
    out = dict(F=F, leaves=L, reps=REPS, plain_fp64_rate_Tops=PLAIN_FP64_RATE / 1e12, runs=[])
    for n in (100000, 1000000):
        bins = rng.integers(0, 256, size=(F, n), dtype=np.uint8)
        hb = shim.HistBuilder(bins, bo)
        hb.set_fix_info(bo[:-1], np.full(F, 256, dtype=np.int32), z)
        hb.set_split_info(np.ones(F, dtype=np.int32), z, z)
        ops_tree, elems = [], []
        for t in trees:
            hb.add_tree(t, shrinkage=0.1)
            sets = np.stack([shim.HistBuilder.node_go_left_mask(255, 0, 0, 0, 0, thr) for thr in t["threshold_in_bin"]])
            E = np.diff(shim.HistBuilder.tree_shap_paths(t, sets)[0]).astype(np.float64)
            ops_tree.append(float((9 * E * E + 9 * E).sum()) + 1.0)
            elems.append(float(E.mean()))
        if n == 100000:
            out["ops_per_row_and_tree_mean"] = float(np.mean(ops_tree))
            out["elements_per_leaf_mean"] = float(np.mean(elems))
        dev = shim.DeviceBuffer(n * (F + 1)).from_host(np.zeros(n * (F + 1)))
        for rep in range(3):                      # the whole set three times: the spread
            for nt in (1, 10, ntrees):
                ms = hb.add_contrib_bench(dev.ptr, trees=(0, nt), reps=REPS)
                ops = n * float(np.sum(ops_tree[:nt]))
                frac = ops / (ms * 1e-3) / PLAIN_FP64_RATE
                out["runs"].append(dict(n=n, rep=rep, trees=nt, ms=ms, ops=ops, fraction_of_plain_fp64=frac, ns_per_row_and_tree=1e6 * ms / (n * nt)))
                print("n %7d  rep %d  %3d trees  %9.4f ms   %.3e fp64 ops   %.3f of the plain-fp64 rate   %.2f ns per row and tree"
                      % (n, rep, nt, ms, ops, frac, 1e6 * ms / (n * nt)), flush=True)
        if n == 100000:      # what was timed computes the right thing: local accuracy of one tree on 4096 rows
            rows = np.arange(4096, dtype=np.int32)
            c = hb.pred_contrib(trees=0, rows=rows)
            s = np.zeros(n)
            hb.add_score(s, trees=0, rows=rows)
            dev_sum = float(np.abs(c.sum(axis=1) - s[rows]).max())
            assert dev_sum <= 1e-13 * float(np.abs(trees[0]["leaf_value"] * 0.1).sum()), dev_sum
            out["local_accuracy_checked_rows"] = 4096
        hb.close()
        del dev
    line = json.dumps(out)
    print(line)
    if len(sys.argv) > 1:
        open(sys.argv[1], "w").write(line + "\n")


if __name__ == "__main__":
    main()
