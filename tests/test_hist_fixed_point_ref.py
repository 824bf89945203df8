"""CPU: the exact integer model of the fixed-point histogram sums (tests/hist_fixed_point_ref.py) against brute-force rational arithmetic -- the model is the
checker of tests/test_zz_hist_fixed_point_gpu.py, so it is pinned here first."""
import math
from fractions import Fraction

import numpy as np

from tests import hist_fixed_point_ref as ref


def _brute(bins, bo, rows, v, inv_q):
    """per flat bin: (sum of rint(v inv_q) as Fractions rounded half to even, exact sum of v, count) by one Fraction addition per (row, feature)"""
    F, n = bins.shape
    rows = np.arange(n) if rows is None else rows
    tot = [0] * int(bo[-1]); ex = [Fraction(0)] * int(bo[-1]); cnt = [0] * int(bo[-1])
    for r in rows:
        x = Fraction(float(v[r])) * Fraction(inv_q)
        k = round(x)                      # Python rounds a Fraction half to even
        for f in range(F):
            o = int(bo[f]) + int(bins[f, r])
            tot[o] += k; ex[o] += Fraction(float(v[r])); cnt[o] += 1
    return tot, ex, cnt


def _small_case(seed, n=700, F=5):
    rng = np.random.default_rng(seed)
    nb = np.array([2, 7, 256, 3, 31][:F])
    bo = np.concatenate([[0], np.cumsum(nb)]).astype(np.int32)
    bins = np.stack([rng.integers(0, nb[f], size=n) for f in range(F)]).astype(np.uint8)
    return rng, bins, bo


def test_scale_restates_the_kernel_rule():
    assert ref.scale(0.0, False) == 1.0 and ref.scale(float("nan"), True) == 1.0 and ref.scale(-1.0, False) == 1.0
    assert ref.scale(1.0, False) == 2.0 ** 40 and ref.scale(1.0, True) == 2.0 ** 50          # 1 = 0.5 * 2^1: frexp's f = 0.5 edge
    assert ref.scale(math.nextafter(1.0, 0.0), False) == 2.0 ** 41
    assert ref.scale(1.9, True) == 2.0 ** 50 and ref.scale(0.25, True) == 2.0 ** 52
    assert ref.scale(5e-324, False) == 2.0 ** 941 and ref.scale(1e-300, True) == 2.0 ** 951  # ex clamped at -900
    assert ref.scale(1e12, False) == 2.0 ** (41 - 40)


def test_ties_round_to_even_and_the_extremes_stay_inside_the_budget():
    inv_q = ref.scale(1.0, False)
    q = 1.0 / inv_q
    assert list(ref.quantise(np.array([0.5, 1.5, 2.5, -0.5, -1.5, -2.5, 3.5]) * q, inv_q)) == [0, 2, 2, 0, -2, -2, 4]
    for ex in (-30, 0, 1, 40):
        top = math.nextafter(math.ldexp(1.0, ex), 0.0)                   # 2^ex - ulp: the largest value of that scale
        for hess, bits in ((False, 41), (True, 51)):
            s = ref.scale(top, hess)
            assert s == math.ldexp(1.0, bits - ex)
            k = ref.quantise(np.array([top, -top]), s)
            assert k[0] == 2 ** bits and k[1] == -2 ** bits              # rounds up to the budget itself, never past it
            assert abs(int(ref.quantise(np.array([math.ldexp(1.0, ex)]), ref.scale(math.ldexp(1.0, ex), hess))[0])) == 2 ** (bits - 1)


def test_model_equals_brute_force_fractions():
    rng, bins, bo = _small_case(1)
    n = bins.shape[1]
    grad = rng.standard_normal(n) * np.exp(rng.uniform(-20, 3, size=n))
    grad[::7] = np.round(grad[::7] * 2.0 ** 20) / 2.0 ** 20
    hess = rng.uniform(1e-6, 2.0, size=n)
    leaf = rng.permutation(n)[: n // 2]
    for rows in (None, leaf):
        m = ref.histogram(bins, bo, rows, grad, hess)
        for col, v, hs in ((0, grad, False), (1, hess, True)):
            inv_q = ref.scale(np.abs(v).max(), hs)
            tot, ex, cnt = _brute(bins, bo, rows, v, inv_q)
            assert (m.tot_h if hs else m.tot_g) == tot
            assert (m.exact_h if hs else m.exact_g) == ex
            assert list(m.counts) == cnt
            want = np.array([float(Fraction(t) / Fraction(inv_q)) for t in tot])        # Fraction -> float is correctly rounded
            assert np.array_equal(m.hist[:, col], want)
            assert ref.bound_violations(m.hist[:, col], ex, m.counts, 1.0 / inv_q) == []
    mc = ref.histogram(bins, bo, leaf, grad, None, const_hess=0.7)
    assert np.array_equal(mc.hist[:, 1], mc.counts.astype(np.float64) * 0.7) and mc.tot_g == ref.histogram(bins, bo, leaf, grad, hess).tot_g


def test_scale_edges_zero_subnormal_huge_nonfinite():
    rng, bins, bo = _small_case(2, n=300)
    n = bins.shape[1]
    z = ref.histogram(bins, bo, None, np.zeros(n), np.zeros(n))
    assert not z.hist.any() and z.q_g == 1.0 and int(z.counts[:2].sum()) == n
    sub = rng.integers(-1000, 1000, size=n) * 5e-324
    s = ref.histogram(bins, bo, None, sub, None)
    assert np.isfinite(s.hist).all() and not any(s.tot_g)               # 2^-1074 * 2^941 rounds to 0: the documented loss
    g = np.full(n, 1e-3); g[17] = 1e12
    m = ref.histogram(bins, bo, None, g, None)
    tot, ex, cnt = _brute(bins, bo, None, g, ref.scale(1e12, False))
    assert m.tot_g == tot and ref.bound_violations(m.hist[:, 0], ex, m.counts, m.q_g) == []
    assert m.q_g == 0.5 and max(abs(float(m.hist[b, 0]) - float(ex[b])) for b in range(len(ex))) > 1e-4       # q = 0.5: the small values are gone, within the bound
    bad = rng.standard_normal(n); bad[3] = np.inf; bad[200] = np.nan
    b = ref.histogram(bins, bo, None, bad, np.ones(n))
    assert np.isnan(b.hist[:, 0]).all() and np.isfinite(b.hist[:, 1]).all() and list(b.counts) == _brute(bins, bo, None, np.ones(n), 1.0)[2]


def test_totals_do_not_depend_on_order_or_on_the_split_into_leaves():
    rng, bins, bo = _small_case(3, n=5000)
    n = bins.shape[1]
    grad = rng.standard_normal(n); hess = rng.uniform(0.5, 2.0, size=n)
    g, h = ref.Channel(grad, False), ref.Channel(hess, True)
    a = ref.histogram(bins, bo, None, g, h, want_exact=False)
    p = ref.histogram(bins, bo, rng.permutation(n), g, h, want_exact=False)
    assert a.tot_g == p.tot_g and a.tot_h == p.tot_h and np.array_equal(a.hist, p.hist) and np.array_equal(a.counts, p.counts)
    mask = rng.uniform(size=n) < 0.37
    le = ref.histogram(bins, bo, np.flatnonzero(mask), g, h, want_exact=False)
    ri = ref.histogram(bins, bo, np.flatnonzero(~mask), g, h, want_exact=False)
    assert [x + y for x, y in zip(le.tot_g, ri.tot_g)] == a.tot_g and [x + y for x, y in zip(le.tot_h, ri.tot_h)] == a.tot_h
    assert np.array_equal(le.counts + ri.counts, a.counts)


def test_a_wrapping_64_bit_chunk_partial_is_told_apart_on_the_adversarial_case():
    """Hessians all 1.9 (k = 1.9 * 2^50), a two-bin feature, 9375 rows per chunk (n = 1.2e6 rows in 128 chunks): half a chunk's rows in one bin sum to 2^63.1.  The
    variant of the model that keeps every (chunk, bin) sum in a signed 64-bit word loses 2^64 q = 16384 per wrapped partial; the exact model does not."""
    rng = np.random.default_rng(4)
    n, rpc = 4 * 9375, 9375
    bins = np.stack([rng.integers(0, 2, size=n), np.zeros(n, dtype=np.int64)]).astype(np.uint8)
    bo = np.array([0, 2, 3], dtype=np.int32)
    grad = rng.standard_normal(n); hess = np.full(n, 1.9)
    good = ref.histogram(bins, bo, None, grad, hess)
    wrapped = ref.histogram(bins, bo, None, grad, hess, want_exact=False, wrap_partials=rpc)
    k = int(ref.quantise(np.array([1.9]), ref.scale(1.9, True))[0])
    assert good.tot_h == [int(c) * k for c in good.counts]
    assert ref.bound_violations(good.hist[:, 1], good.exact_h, good.counts, good.q_h) == []
    assert wrapped.tot_g == good.tot_g and np.array_equal(wrapped.counts, good.counts)
    for b in range(3):
        lost = good.tot_h[b] - wrapped.tot_h[b]
        assert lost > 0 and lost % (1 << 64) == 0, b
        assert abs(good.hist[b, 1] - wrapped.hist[b, 1] - (lost >> 64) * 16384.0) < 1e-6        # 2^64 q = 16384 per wrapped partial
    assert ref.bound_violations(wrapped.hist[:, 1], good.exact_h, good.counts, good.q_h) == [0, 1, 2]
    # below the budget (uniform(0.5, 2) hessians at the same chunking stay under 2^63): both variants agree
    h2 = rng.uniform(0.5, 2.0, size=n)
    assert ref.histogram(bins[:1], bo[:2], None, grad, h2, want_exact=False, wrap_partials=rpc).tot_h == ref.histogram(bins[:1], bo[:2], None, grad, h2, want_exact=False).tot_h
