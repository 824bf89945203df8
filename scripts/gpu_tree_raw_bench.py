"""MI355X: time of one raw-row scoring launch (gpb_hip_hist_add_score_dev with which = 2: tree_raw_kernels.hip; HIP events on the handle's stream, one warm-up
launch, mean of REPS) at n = 1e6 rows of F = 50 feature values, float64 and float32, random valid 31-leaf trees with numerical nodes of all three missing types
and a third categorical nodes: 1 tree and 100 trees, all rows and a 30 % row list.  Each time is set against its traffic floor: rows * (F * sizeof(T) + 16 bytes
of score [+ 4 of index]) / the 6.29 TB/s measured copy rate.  The REPS launches re-read the same matrix (400 / 200 MB): the float32 one
fits the 256 MB Infinity Cache.  The binned path on the same trees' bin forms is timed next to it (scripts/gpu_tree_predict_bench.py's figure).

    python scripts/gpu_tree_raw_bench.py [out.json]
"""
import json
import os
import sys

import numpy as np

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
from scripts.gpu_tree_predict_bench import COPY_RATE, REPS, random_tree      # noqa: E402


def raw_rule(rng, nn):
    """Thresholds in the rows' range, a third of the nodes categorical with 4-word bitsets, random missing types and default directions."""
    cat = rng.uniform(size=nn) < 1 / 3
    dt = (cat | (rng.integers(0, 2, size=nn) << 1) | (rng.integers(0, 3, size=nn) << 2)).astype(np.int8)
    ncat = int(cat.sum())
    return dict(threshold=np.where(cat, np.cumsum(cat) - 1, rng.uniform(0, 100, size=nn)), decision_type=dt,
                cat_boundaries=(4 * np.arange(ncat + 1)).astype(np.int32), cat_threshold=rng.integers(0, 2 ** 32, size=4 * ncat, dtype=np.uint64).astype(np.uint32))


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
    for _ in range(ntrees):
        t = random_tree(rng, F, L)
        hb.add_tree(dict(t, **raw_rule(rng, L - 1)), shrinkage=0.1)
    X = rng.uniform(0, 100, size=(n, F))
    u = rng.uniform(size=(n, F))
    X[u < 0.05] = np.nan; X[u > 0.95] = 0.0
    rows30 = np.flatnonzero(rng.uniform(size=n) < 0.3).astype(np.int32)
    score = shim.DeviceBuffer(n).from_host(np.zeros(n))
    out = dict(n=n, F=F, leaves=L, reps=REPS, copy_rate_TBps=COPY_RATE / 1e12, runs=[])
    for dtype, pred in ((np.float64, "raw"), (np.float32, "raw"), (np.uint8, False)):
        eb = np.dtype(dtype).itemsize if pred else 64.0 / F          # the binned path reads fpad = 64 bytes per row
        if pred:
            hb.set_pred_raw(np.ascontiguousarray(X, dtype=dtype))
        for rep in range(3):                  # the whole set three times: the spread
            for nt in (1, ntrees):
                for name, rows in (("all_rows", None), ("list_30pct", rows30)):
                    cnt = n if rows is None else rows.size
                    ms = hb.add_score_bench(score.ptr, trees=(0, nt), rows=rows, pred=pred, reps=REPS)
                    floor_ms = 1e3 * cnt * (F * eb + 16.0 + (0 if rows is None else 4)) / COPY_RATE
                    out["runs"].append(dict(dtype=np.dtype(dtype).name, rep=rep, trees=nt, rows=name, cnt=int(cnt), ms=ms, floor_ms=floor_ms, ratio=ms / floor_ms))
                    print("%-7s rep %d  %3d trees  %-10s  %8d rows  %8.4f ms   floor %7.4f ms   x %.2f" % (np.dtype(dtype).name, rep, nt, name, cnt, ms, floor_ms, ms / floor_ms),
                          flush=True)
    hb.close()
    line = json.dumps(out)
    print(line)
    if len(sys.argv) > 1:
        open(sys.argv[1], "w").write(line + "\n")


if __name__ == "__main__":
    main()
