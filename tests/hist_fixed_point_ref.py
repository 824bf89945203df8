"""Exact integer model of the fixed-point histogram sums (gpboost_amd/csrc/hist_kernels.hip, "fixed-point accumulation") -- the checker of
tests/test_zz_hist_fixed_point_gpu.py (its own check: tests/test_hist_fixed_point_ref.py, CPU).  Plain numpy and Python integers; nothing of the product is imported.

The documented scheme: every gradient is rounded ONCE to a multiple of q = 2^(ex - 41), every hessian to a multiple of 2^(ex - 51), 2^ex >= max |value| over ALL rows
handed to set_gradients (frexp; ex clamped at -900; q = 1 when the maximum is not greater than 0); k = rint(v / q) with ties to even; the k of a bin are summed as
integers WITHOUT any wrap -- whatever the chunking, the order and the rank layout are -- and the total is converted once: entry = fl(total) * q.  With a constant
hessian the second column is count * const_hess.  A non-finite value anywhere makes every sum of that array NaN; the counts stay exact.

Contract: |entry - exact real sum of the bin| <= count * q / 2 + one rounding (ulp(entry)).

Exactness here: integers up to 2^51 are split into 21-bit limbs whose per-bin sums (np.bincount with weights, fp64) stay below 2^21 * 2^31 rows < 2^53; the limbs are
recombined as Python ints.  The exact REAL sums go the same way on the unrounded values: a double is mant * 2^e with a 53-bit integer mant (frexp), rows are grouped by e."""
import math
from fractions import Fraction

import numpy as np

GRAD_BITS, HESS_BITS, MIN_EX = 41, 51, -900
_LIMB = 21


def scale(max_abs, hess):
    """inv_q = 2^((51 if hess else 41) - ex) for max_abs = f * 2^ex, f in [0.5, 1); 1 if not max_abs > 0 (restates fixed_point_inv_q)."""
    max_abs = float(max_abs)
    if not (max_abs > 0.0):
        return 1.0
    _, ex = math.frexp(max_abs)
    ex = max(ex, MIN_EX)
    return math.ldexp(1.0, (HESS_BITS if hess else GRAD_BITS) - ex)


def quantise(v, inv_q):
    """int64 rint(v * inv_q), ties to even (v * inv_q is exact: inv_q is a power of two; it can only round where the product is subnormal, i.e. |k| << 1)."""
    return np.rint(np.asarray(v, dtype=np.float64) * inv_q).astype(np.int64)


def _limbs(k, nlimbs=3):
    """the int64 k (|k| < 2^(21 nlimbs)) as signed 21-bit limbs in fp64: k = sum_l limb_l 2^(21 l)"""
    sign = np.sign(k).astype(np.float64)
    a = np.abs(k)
    return [((a >> (_LIMB * l)) & ((1 << _LIMB) - 1)).astype(np.float64) * sign for l in range(nlimbs)]


def _int_bin_sums(idx, limbs, nbins):
    """exact per-bin sums (Python ints) over the bin indices idx of the integers given by their limbs: every limb sum stays below 2^53 in fp64"""
    tot = [0] * nbins
    for l, limb in enumerate(limbs):
        s = np.bincount(idx, weights=limb, minlength=nbins).astype(np.int64).tolist()
        tot = [t + (x << (_LIMB * l)) for t, x in zip(tot, s)]
    return tot


class _Exact(object):
    """finite doubles as mant * 2^(e) with integer mant, grouped by exponent: per-row pieces prepared once, summed per feature"""

    def __init__(self, v):
        m, e = np.frexp(np.asarray(v, dtype=np.float64))
        self.mant = np.ldexp(m, 53).astype(np.int64)                # |mant| < 2^53, exact
        self.exps, self.grp = np.unique(e.astype(np.int64) - 53, return_inverse=True)


def ulp(x):
    x = abs(float(x))
    return math.ulp(x) if math.isfinite(x) else float("nan")


class Channel(object):
    """one array (gradients or hessians) of a handle: its scale from ALL its values, its integers, its exact pieces"""

    def __init__(self, v, hess):
        v = np.asarray(v, dtype=np.float64)
        self.finite = bool(np.isfinite(v).all())
        self.max_abs = float(np.abs(v).max()) if (v.size and self.finite) else float("nan")
        self.inv_q = scale(self.max_abs, hess) if self.finite else 1.0
        self.q = 1.0 / self.inv_q
        self.v = v
        self.k = quantise(v, self.inv_q) if self.finite else None
        self._exact = None

    def exact(self):
        if self._exact is None:
            self._exact = _Exact(self.v)
        return self._exact


class Result(object):
    """per flat bin: counts (uint64), tot_g / tot_h (Python ints, units of q), hist (total_bins, 2) expected entries, exact_g / exact_h (Fractions), q_g / q_h"""
    pass


def histogram(bins, bin_offsets, rows, grad, hess, const_hess=1.0, want_exact=True, wrap_partials=None, features=None):
    """bins (F, n) uint8; rows: index array or None (all rows); grad / hess: arrays over ALL n rows (they fix the scale) or Channel objects; hess None: constant
    hessian.  wrap_partials = rows_per_chunk: the DEFECTIVE variant -- the rows are cut into chunks of that many rows in list order and every (chunk, bin) integer sum
    is wrapped to int64 before the chunks are added (what a 64-bit per-chunk partial does).  features: only these are filled (the others stay zero)."""
    bins = np.asarray(bins)
    F, n = bins.shape
    bo = np.asarray(bin_offsets, dtype=np.int64)
    total_bins = int(bo[-1])
    g = None if grad is None else (grad if isinstance(grad, Channel) else Channel(grad, False))      # None: hessian column only (the gradient column stays zero)
    h = None if hess is None else (hess if isinstance(hess, Channel) else Channel(hess, True))
    rows_a = None if rows is None else np.asarray(rows, dtype=np.int64)
    sel = (lambda a: a) if rows_a is None else (lambda a: a[rows_a])
    chans = [c for c in (g, h) if c is not None]
    ks = [_limbs(sel(c.k), 2 if c is g else 3) if c.finite else None for c in chans]          # |k| <= 2^41 / 2^51
    ex = []
    for c in chans:
        if want_exact and c.finite:
            e = c.exact()
            ex.append((e, sel(e.grp), _limbs(sel(e.mant))))
        else:
            ex.append(None)
    r = Result()
    r.counts = np.zeros(total_bins, dtype=np.uint64)
    r.tot = [[0] * total_bins for _ in chans]
    r.exact = [[Fraction(0)] * total_bins if ex[i] is not None else None for i in range(len(chans))]
    r.hist = np.zeros((total_bins, 2))
    r.q_g = None if g is None else g.q
    r.q_h = None if h is None else h.q
    m = n if rows_a is None else rows_a.size
    chunk_of = None
    if wrap_partials:
        chunk_of = np.arange(m, dtype=np.int64) // int(wrap_partials)
        nch = int(chunk_of[-1]) + 1 if m else 1
    for f in (range(F) if features is None else features):
        nb = int(bo[f + 1] - bo[f])
        idx = sel(bins[f]).astype(np.int64)
        o = int(bo[f])
        r.counts[o:o + nb] = np.bincount(idx, minlength=nb)[:nb].astype(np.uint64)
        for ci, c in enumerate(chans):
            if not c.finite:
                continue
            if chunk_of is None:
                r.tot[ci][o:o + nb] = _int_bin_sums(idx, ks[ci], nb)
            else:
                part = _int_bin_sums(idx + nb * chunk_of, ks[ci], nb * nch)
                for b in range(nb):
                    s = 0
                    for ch in range(nch):
                        p = part[ch * nb + b]
                        s += ((p + (1 << 63)) % (1 << 64)) - (1 << 63)          # a signed 64-bit word
                    r.tot[ci][o + b] = s
            if ex[ci] is not None:
                e, grp, mant = ex[ci]
                ng = e.exps.size
                tot = _int_bin_sums(idx + nb * grp, mant, nb * ng)
                emin = int(e.exps[0])                                            # np.unique sorts: the smallest exponent is the common unit
                acc = [0] * nb
                for j in np.flatnonzero(np.array([t != 0 for t in tot])):
                    acc[j % nb] += tot[j] << (int(e.exps[j // nb]) - emin)
                unit = Fraction(2) ** emin
                acc = [t * unit for t in acc]
                r.exact[ci][o:o + nb] = acc
    col = {id(g): 0, id(h): 1}
    for ci, c in enumerate(chans):
        if c.finite:
            r.hist[:, col[id(c)]] = np.array([float(t) for t in r.tot[ci]]) * c.q       # int -> float is correctly rounded; q is a power of two
        else:
            r.hist[:, col[id(c)]] = np.nan
    if h is None and g is not None:
        r.hist[:, 1] = r.counts.astype(np.float64) * const_hess
    by = {id(c): ci for ci, c in enumerate(chans)}
    r.tot_g = None if g is None else r.tot[by[id(g)]]
    r.tot_h = None if h is None else r.tot[by[id(h)]]
    r.exact_g = None if g is None else r.exact[by[id(g)]]
    r.exact_h = None if h is None else r.exact[by[id(h)]]
    return r


def bound_violations(entries, exact, counts, q):
    """bins where |entry - exact| > count * q / 2 + ulp(entry) (the contract), evaluated in rationals"""
    bad = []
    for b in range(len(exact)):
        e = float(entries[b])
        lim = Fraction(int(counts[b])) * Fraction(q) / 2 + Fraction(ulp(e))
        if abs(Fraction(e) - exact[b]) > lim:
            bad.append(b)
    return bad
