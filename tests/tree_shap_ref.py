"""Helpers of the TreeSHAP tests (tests/test_tree_shap_ref.py on the CPU, tests/test_zz_tree_shap_gpu.py on the device): what per-feature contributions
must equal, stated three ways.

  exact_contrib   the Shapley DEFINITION in exact rational arithmetic: phi_f = sum over S subset of N \\ {f} of |S|! (M - |S| - 1)! / M! (v(S + f) - v(S)),
                  where v(S) follows the row at a node whose column is in S and is the count-weighted mean of both children where it is not; column F is
                  v(empty set) = Tree::ExpectedValue.  No path, no weights: exponential in the columns a tree uses, for small trees only.
  python_paths    per leaf the distinct columns of its path, the AND of the go-left sets and the zero fraction as an exact Fraction (with its number of
                  factors) -- a restatement the library's table (gpb_hip_tree_shap_paths) is compared with.
  path_contrib    the path algorithm (the reference's ExtendPath / UnwoundPathSum recurrences, src/LightGBM/io/tree.cpp:827-884, in their order of operations)
                  over a path table, vectorised over rows, in float64 or numpy.longdouble.

Random columns and trees come from tests/test_zz_tree_predict_gpu.py (_random_columns, _random_tree, _numpy_leaves); leaf counts are uniform in 1 .. 999."""
from fractions import Fraction
from itertools import combinations
from math import factorial

import numpy as np

from tests import test_zz_tree_predict_gpu as TP


def random_columns(rng, F):
    """TP._random_columns needs three columns; narrower matrices keep the first F of them."""
    col = TP._random_columns(rng, max(F, 3))
    if F < 3:
        col = {k: v[:F] for k, v in col.items() if k != "bo"}
        col["bo"] = np.concatenate([[0], np.cumsum(col["gnb"])]).astype(np.int32)
    return col


def random_tree(rng, col, L):
    t = TP._random_tree(rng, col, L)
    t["leaf_count"] = rng.integers(1, 1000, size=L).astype(np.int32)
    return t


def chain_tree(rng, col, columns):
    """A chain: node k splits columns[k], its left child is leaf k, its right child the next node (the last node's: the last leaf).  The path to the last
    two leaves holds every column of the list."""
    nn = len(columns)
    L = nn + 1
    sf = np.asarray(columns, dtype=np.int32)
    t = dict(num_leaves=L, leaf_value=rng.standard_normal(L), split_feature_inner=sf, default_left=rng.integers(0, 2, size=nn).astype(np.int32),
             node_is_cat=np.zeros(nn, dtype=np.int32), node_cat_bits=np.zeros((nn, 8), dtype=np.uint32),
             threshold_in_bin=np.array([rng.integers(0, col["num_bin"][f]) for f in sf], dtype=np.int64),
             left_child=~np.arange(nn, dtype=np.int32), right_child=np.arange(1, nn + 1, dtype=np.int32),
             leaf_count=rng.integers(1, 1000, size=L).astype(np.int32))
    t["right_child"][nn - 1] = ~nn
    return t


def node_sets(shim, col, t):
    """(nodes, 8) uint32: the go-left set of every node (node_go_left_mask: what a stored tree holds)."""
    nn = t["num_leaves"] - 1
    out = np.zeros((nn, 8), dtype=np.uint32)
    for k in range(nn):
        f = int(t["split_feature_inner"][k])
        out[k] = shim.HistBuilder.node_go_left_mask(col["gnb"][f] - 1, col["db"][f], col["mfb"][f], col["mt"][f], t["default_left"][k], t["threshold_in_bin"][k],
                                                    cat_bits=t["node_cat_bits"][k] if t["node_is_cat"][k] else None)
    return out


def unpack(sets8):
    """(..., 8) uint32 -> (..., 256) bool"""
    s = np.asarray(sets8, dtype=np.uint32)
    b = np.arange(256)
    return ((s[..., b >> 5] >> (b & 31).astype(np.uint32)) & 1).astype(bool)


def node_counts(t):
    nn = t["num_leaves"] - 1
    cnt = [0] * nn
    for i in range(nn - 1, -1, -1):
        for c in (int(t["left_child"][i]), int(t["right_child"][i])):
            cnt[i] += int(t["leaf_count"][~c]) if c < 0 else cnt[c]
    return cnt


def _depths(t):
    """Nodes on the path to every leaf (a path with fewer elements than nodes reuses a column)."""
    L = t["num_leaves"]
    out = [0] * L
    if L == 1:
        return out
    dn = {0: 1}
    for i in range(L - 1):                                     # children are later nodes
        for c in (int(t["left_child"][i]), int(t["right_child"][i])):
            if c < 0:
                out[~c] = dn[i]
            else:
                dn[c] = dn[i] + 1
    return out


def exact_contrib(t, left, bins_row, F, values=None):
    """The definition, in Fractions.  left: (nodes, 256) bool; bins_row: the row's stored bin per column; values: the stored leaf values (default: the
    tree's).  -> F + 1 Fractions."""
    vals = [Fraction(float(v)) for v in (t["leaf_value"] if values is None else values)]
    out = [Fraction(0)] * (F + 1)
    if t["num_leaves"] == 1:
        out[F] = vals[0]
        return out
    cnt = node_counts(t)
    sf, lc, rc = t["split_feature_inner"], t["left_child"], t["right_child"]

    def count(c):
        return int(t["leaf_count"][~c]) if c < 0 else cnt[c]

    def v(node, S):
        if node < 0:
            return vals[~node]
        f = int(sf[node])
        l, r = int(lc[node]), int(rc[node])
        if f in S:
            return v(l if left[node, bins_row[f]] else r, S)
        return (count(l) * v(l, S) + count(r) * v(r, S)) / cnt[node]
    used = sorted(set(int(f) for f in sf))
    M = len(used)
    val = {}
    for k in range(M + 1):
        for S in combinations(used, k):
            val[frozenset(S)] = v(0, frozenset(S))
    for f in used:
        rest = [g for g in used if g != f]
        phi = Fraction(0)
        for k in range(M):
            w = Fraction(factorial(k) * factorial(M - k - 1), factorial(M))
            for S in combinations(rest, k):
                S = frozenset(S)
                phi += w * (val[S | {f}] - val[S])
        out[f] = phi
    out[F] = val[frozenset()]
    return out


def python_paths(t, left):
    """-> per leaf a list of [column, (256,) bool set, Fraction zero fraction, number of factors], in order of first appearance."""
    L = t["num_leaves"]
    paths = [None] * L
    if L == 1:
        return [[]]
    cnt = node_counts(t)

    def walk(node, path):
        f = int(t["split_feature_inner"][node])
        for side, c in ((0, int(t["left_child"][node])), (1, int(t["right_child"][node]))):
            q = Fraction(int(t["leaf_count"][~c]) if c < 0 else cnt[c], cnt[node])
            s = left[node] if side == 0 else ~left[node]
            p = [list(e) for e in path]
            for e in p:
                if e[0] == f:
                    e[1] = e[1] & s; e[2] = e[2] * q; e[3] += 1
                    break
            else:
                p.append([f, s.copy(), q, 1])
            if c < 0:
                paths[~c] = p
            else:
                walk(c, p)
    walk(0, [])
    return paths


def table_from_library(first, column, sets8, zero):
    """The arrays of shim.HistBuilder.tree_shap_paths -> per leaf (columns, (E, 256) bool, zero fractions as float64)"""
    m = unpack(sets8) if len(column) else np.zeros((0, 256), dtype=bool)
    return [(column[a:b], m[a:b], np.asarray(zero[a:b], dtype=np.float64)) for a, b in zip(first[:-1], first[1:])]


def table_from_python(paths, dtype):
    """python_paths -> the same form with the zero fractions rounded once to dtype (numerator / denominator in that type)"""
    out = []
    for p in paths:
        z = np.array([dtype(e[2].numerator) / dtype(e[2].denominator) for e in p], dtype=dtype)
        out.append((np.array([e[0] for e in p], dtype=np.int64), np.array([e[1] for e in p], dtype=bool).reshape(len(p), 256), z))
    return out


def expected_value(t, values, dtype):
    """Tree::ExpectedValue (tree.cpp:990-998): sum in leaf order of (count / total) * value"""
    if t["num_leaves"] == 1:
        return dtype(values[0])
    total = dtype(int(np.sum(t["leaf_count"].astype(np.int64))))
    ev = dtype(0)
    for c, v in zip(t["leaf_count"], values):
        ev = ev + (dtype(int(c)) / total) * dtype(v)
    return ev


def path_contrib(table, values, bins, F, ev, dtype=np.float64, out=None):
    """The path algorithm over all rows: bins (F, m) stored bins -> out (m, F + 1) in dtype, added onto `out` in (leaf, element) order.  ExtendPath and
    UnwoundPathSum with element 0 the root placeholder (zero = one = 1); the loop over a path's positions is an array axis, the arithmetic per entry is the
    reference's."""
    m = bins.shape[1]
    res = np.zeros((m, F + 1), dtype=dtype) if out is None else out
    one_ = dtype(1)
    for leaf, (cols, masks, zero) in enumerate(table):
        E = len(cols)
        if E == 0:
            continue
        v = dtype(values[leaf])
        z = np.asarray(zero, dtype=dtype)
        o = np.stack([masks[e][bins[int(cols[e])]] for e in range(E)], axis=1).astype(dtype)          # (m, E) one fractions
        pw = np.zeros((m, E + 1), dtype=dtype)
        pw[:, 0] = one_
        for d in range(1, E + 1):                                                                       # ExtendPath at unique_depth = d
            k = np.arange(d + 1).astype(dtype)
            new = np.zeros_like(pw)
            new[:, :d + 1] = z[d - 1] * pw[:, :d + 1] * (dtype(d) - k) / dtype(d + 1)
            new[:, 1:d + 1] += o[:, d - 1:d] * pw[:, :d] * k[1:] / dtype(d + 1)
            pw = new
        D = E
        nop = np.repeat(pw[:, D:D + 1], E, axis=1)                                                       # (m, E): every element's own unwinding
        tot1 = np.zeros((m, E), dtype=dtype); tot0 = np.zeros((m, E), dtype=dtype)
        for i in range(D - 1, -1, -1):
            tmp = nop * dtype(D + 1) / dtype(i + 1)                                                      # (one fraction 1: the divisor (i + 1) * one)
            tot1 = tot1 + tmp
            nop = pw[:, i:i + 1] - tmp * z[None, :] * (dtype(D - i) / dtype(D + 1))
            tot0 = tot0 + (pw[:, i:i + 1] / z[None, :]) / (dtype(D - i) / dtype(D + 1))
        w = np.where(o != 0, tot1, tot0)
        add = w * (o - z[None, :]) * v
        for e in range(E):
            res[:, int(cols[e])] += add[:, e]
    res[:, F] += dtype(ev)
    return res


def forest_contrib(tables, values, counts_trees, bins, F, dtype):
    """Sum over trees, in tree order: tables / values / trees per tree -> (m, F + 1) in dtype"""
    out = np.zeros((bins.shape[1], F + 1), dtype=dtype)
    for tab, vals, t in zip(tables, values, counts_trees):
        path_contrib(tab, vals, bins, F, expected_value(t, vals, dtype), dtype, out=out)
    return out
