"""CPU: the per-datum restatement of the likelihood kernels (tests/lik_terms_ref.py) -- the committed grid is finite and decides every branch as 60 digits would,
the fp64 restatement (host libm) stays within the a-priori bound at eps_f = 1 for every likelihood, output and grid point, and every mutant breaks the bound at
eps_f = 16 somewhere on the grid.  No device."""
import math

import numpy as np
import pytest

from tests import lik_terms_ref as R

LIKS = list(range(9))


@pytest.mark.parametrize("lik", LIKS, ids=R.LIK_NAMES)
def test_grid_is_finite_and_decides_as_60_digits_would(lik):
    for ci, c in enumerate(R.cases(lik)):
        ref = R.reference(lik, ci)
        assert ref.finite, "%s case %s: an fp64 intermediate of the restatement is not finite; allowed() must leave the point out" % (R.LIK_NAMES[lik], c)
        assert not ref.defects, "%s case %s: 60 digits decide a branch differently: %s" % (R.LIK_NAMES[lik], c, ref.defects[:5])


def test_grid_holds_its_locations_shapes_and_configurations_and_keeps_off_the_thresholds():
    assert set(abs(x) for x in R.LOCATIONS) == {0.0, 0.4, 3.0, 8.2, 8.4, 12.0, 20.0, 27.0, 28.0, 37.4, 40.0, 60.0, 300.0}
    assert R.SHAPES == (1, 63, 257, 1500) and R.N_EACH_MAX <= 400
    for lik in LIKS:
        cs = R.cases(lik)
        for n in R.SHAPES:
            mine = [c for c in cs if c[0] == n]
            for flag in (1, 2, 3):       # re_ptr, weights, fixed effects: each shape with and without
                assert {c[flag] for c in mine} == {True, False}, (lik, n, flag)
            if R.INT_RESP[lik] and R.REAL_RESP[lik]:
                assert {c[4] for c in mine} == {True, False}, (lik, n)
        assert {c[5] for c in cs} == {0, 1, 2, 3}
        built = [R.Case(lik, *c) for c in cs]
        assert any(np.any(c.weights == 0.0) for c in built if c.has_w), "some weights are exactly 0"
        assert any(np.any(np.diff(c.re_ptr) == 0) for c in built if c.has_ptr) and max(int(np.diff(c.re_ptr).max()) for c in built if c.has_ptr) == 5, "0 to 5 data per row"
    # at least 1e-6 (relative) away from every threshold: the locations from the clamp of sigmoid_clamped (sigmoid(x) = 1e-12 at |x| = log(1e12 - 1)), from the
    # underflow of erfc (|z| about 38.5; the fixed exclusion [37.5, 38.6]) and from 0 unless it is 0; the arguments of the gamma family from its five thresholds
    for x in R.LOCATIONS:
        for thr in (math.log(1e12 - 1.0), 37.5, 38.6):
            assert abs(abs(x) - thr) > 1e-6 * thr
        assert x == 0.0 or abs(x) > 1e-6
    for lik in (R.BETA, R.NEGBIN):
        for ci in range(len(R.cases(lik))):
            R.reference(lik, ci)
    for thr, dist in R.THRESHOLD_DIST.items():
        assert 1e-6 <= dist < math.inf, "an argument of digamma / trigamma / tetragamma comes within %.3g (relative) of the threshold %r" % (dist, thr)


@pytest.mark.parametrize("lik", LIKS, ids=R.LIK_NAMES)
def test_fp64_restatement_is_within_the_bound_at_eps_1(lik):
    worst = {}
    for ci, c in enumerate(R.cases(lik)):
        ref = R.reference(lik, ci)
        for name, got in ref.f64_outputs().items():
            r = ref.ratio(name, got, 1.0)
            if r.size:
                worst[name] = max(worst.get(name, 0.0), float(r.max()))
                assert r.max() <= 1.0, "%s case %s output %s: worst ratio %.3g at element %d" % (R.LIK_NAMES[lik], c, name, r.max(), int(r.argmax()))
    print("CPU ratios %-18s %s" % (R.LIK_NAMES[lik], "  ".join("%s %.2f" % kv for kv in sorted(worst.items()))))
    assert worst and max(worst.values()) > 0.05, "a bound nothing comes near checks nothing"


def test_every_branch_of_the_device_functions_is_on_the_grid():
    for lik in LIKS:
        for ci in range(len(R.cases(lik))):
            R.reference(lik, ci)
    a = R.LIB_ARGS
    s = 0.70710678118654752440
    assert any(x > 38.7 * s for x in a["erfc"]), "series branch of normal_log_cdf (erfc underflows) and the Q == 0 branch"
    assert any(26.0 < x < 37.5 * s for x in a["erfc"]), "the last arguments before erfc underflows"
    assert min(a["lgamma"]) < 1e-14 and max(a["lgamma"]) > 9e3, "beta: tiny and huge arguments of lgamma"
    assert min(a["exp"]) <= -300.0 and max(a["exp"]) >= 300.0


@pytest.mark.parametrize("mut,lik", R.MUTANTS, ids=[m for m, _ in R.MUTANTS])
def test_mutant_breaks_the_bound_at_eps_16(mut, lik):
    ratio, where = R.mutant_worst(mut, lik, eps=16.0)
    assert ratio > 1.0, "mutant %s stays within the bound (worst ratio %.3g): the bound would not notice it" % (mut, ratio)
    assert where is not None and (math.isinf(ratio) or ratio > 1.0)


def test_there_are_at_least_ten_mutants_and_the_table_is_filled_in():
    assert len(R.MUTANTS) >= 10 and len({m for m, _ in R.MUTANTS}) == len(R.MUTANTS)
    table = R.__doc__.split("RATIO_TABLE_BEGIN")[1].split("RATIO_TABLE_END")[0]
    for name in R.LIK_NAMES:
        assert name in table, "the docstring table of tests/lik_terms_ref.py lacks " + name
    for f in R.LIB:
        assert "eps_" + f in table
