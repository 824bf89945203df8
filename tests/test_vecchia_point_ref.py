"""CPU: tests/vecchia_point_ref.py itself -- the long-double model of one Vecchia point against mpmath at 50 digits and against the fp64 oracle, the oracle inside
the a-priori bounds at every checked point of every case of the GPU lists, the bounds not vacuous, and the bounds' teeth (mutants of the model leave them)."""
import numpy as np
import pytest

from tests import vecchia_point_ref as R

LD = R.LD
pytestmark = pytest.mark.skipif(not R.long_double_is_wider(), reason="np.longdouble is not wider than float64 on this platform")

ALL = R.all_cases()
BY_ID = {c.id: c for c in ALL}


def _class_of(case):
    if case.kind == "big":
        return "big m=%d %s" % (case.m, "weighted" if case.wt else "uniform")
    return "MT=%d %s" % (case.mt, "latent" if case.kind == "latent" else ("weighted" if case.wt else "uniform"))


# ---- the case tables ---------------------------------------------------------------------------------------------------------------------------------------
def test_case_tables_reach_every_instance():
    inst = R.instance_cases()
    assert len(inst) == 72 and len({c.id for c in ALL}) == len(ALL)
    reached = {R.instance_of(c, mode) for c in inst for mode in (0, 1, 2)}
    want = {(mt, cov, d3, mode, wt) for mt in R.MT_LIST for cov in range(3) for d3 in (False, True) for mode in (0, 1, 2) for wt in (False, True)}
    # the dispatcher never launches the unweighted gradient instance of 30 < MT <= 40: the weighted one serves both (kRuntimeWeightedInstance)
    unreachable = {(40, cov, d3, 2, False) for cov in range(3) for d3 in (False, True)}
    assert reached == want - unreachable
    # every (MT, m) pair meets every COV and both D3
    for mt in R.MT_LIST:
        for m in (mt, R.SMALLEST_M[mt]):
            mine = [c for c in inst if c.mt == mt and c.m == m]
            assert {c.cov for c in mine} == {0, 1, 2} and {c.d == 3 for c in mine} == {False, True}, (mt, m)
            assert R.padded_mt(m) == mt
    assert {c.d for c in inst} == {1, 2, 3}
    for c in inst:
        assert c.n == 16 * -(-(c.mt + 40) // 16) + 5 and c.n % 16 == 5 and c.n // 16 >= 4
    big = {R.instance_of(c, mode) for c in R.big_cases() for mode in (0, 1, 2)}
    assert big == {("big", dk, cov, mode, wt) for dk in (0, 2, 3) for cov in range(3) for mode in (0, 1, 2) for wt in (False, True)}
    assert {c.mt for c in R.latent_cases()} == set(R.MT_LIST)


def test_neighbour_tables_and_checked_points():
    for c in (BY_ID["mt10-cov0-d2-u-m10"], BY_ID["mt62-cov2-d3-w-m62"], R.big_cases()[0]):
        cd = R.case_data(c)
        assert np.all(cd.nn < np.arange(c.n)[:, None])
        for i in (0, 1, c.m - 1, c.m, c.n - 1):
            row = cd.nn[i]
            k = min(i, c.m)
            assert np.all(row[:k] >= 0) and np.all(row[k:] == -1)
            if k:
                dist = np.sqrt(np.sum((cd.coords[:i] - cd.coords[i]) ** 2, axis=1))
                assert np.allclose(np.sort(dist)[:k], dist[row[:k]])
        a, b = cd.dup
        assert np.array_equal(cd.coords[a], cd.coords[b]) and cd.nn[b, 0] == a
        pts = R.checked_points(c)
        assert len(pts) == 24 and {0, 1, 2, c.m, 15, 16, 17, a, b, c.n - 1} <= set(pts)


# ---- the model against mpmath --------------------------------------------------------------------------------------------------------------------------------
def _mp_point(case, i):
    import mpmath as mp
    mp.mp.dps = 50
    cd = R.case_data(case)
    N = [int(v) for v in cd.nn[i] if v >= 0]
    k = len(N)
    X = [[mp.mpf(float(v)) for v in cd.coords[j]] for j in N]
    xi = [mp.mpf(float(v)) for v in cd.coords[i]]
    var, a = mp.mpf(case.var), mp.mpf(case.a)

    def dist(p, q):
        return mp.sqrt(sum((s - t) ** 2 for s, t in zip(p, q)))

    def K(r):
        return var * mp.exp(-r) * (1 if case.cov == 0 else (1 + r if case.cov == 1 else 1 + r + r * r / 3))

    def dK(r):
        return -var * mp.exp(-r) * (r if case.cov == 0 else (r * r if case.cov == 1 else r * r * (1 + r) / 3))
    if cd.nug is not None:
        nv = [mp.mpf(float(cd.nug[j])) for j in N]; ni = mp.mpf(float(cd.nug[i])); diag = [var + v for v in nv]; c0 = var + ni
    elif case.gauss:
        nv = [mp.mpf(1)] * k; ni = mp.mpf(1); diag = [var + 1] * k; c0 = var + 1
    else:
        nv = [mp.mpf(0)] * k; ni = mp.mpf(0); diag = [mp.mpf(float(case.var) * (1.0 + 1e-10))] * k; c0 = var
    C = mp.matrix(k, k); dC = mp.matrix(k, k); c = mp.matrix(k, 1); dc = mp.matrix(k, 1); y = mp.matrix(k, 1)
    for r in range(k):
        c[r] = K(a * dist(X[r], xi)); dc[r] = dK(a * dist(X[r], xi)); y[r] = mp.mpf(float(cd.y[N[r]]))
        for s in range(k):
            C[r, s] = diag[r] if r == s else K(a * dist(X[r], X[s]))
            dC[r, s] = 0 if r == s else dK(a * dist(X[r], X[s]))
    A, b = (mp.lu_solve(C, c), mp.lu_solve(C, y)) if k else (c, y)
    dot = lambda p, q: sum(p[t] * q[t] for t in range(k))
    D = c0 - dot(A, c); u = mp.mpf(float(cd.y[i])) - dot(A, y)
    dDv = D - ni - sum(nv[t] * A[t] ** 2 for t in range(k)); ukv = -sum(nv[t] * b[t] * A[t] for t in range(k))
    dCA = dC * A if k else A
    dDr = dot(A, dCA) - 2 * dot(A, dc); ukr = dot(b, dCA) - dot(b, dc)
    up = u / D
    terms = [u * u / D, mp.log(D), 0, ukv * up - up * up * dDv / 2, dDv / (2 * D), ukr * up - up * up * dDr / 2, dDr / (2 * D)]
    return [A[t] for t in range(k)], D, u, terms


def _ld(x):
    import mpmath as mp
    hi = float(x)
    return LD(hi) + LD(float(x - mp.mpf(hi)))


MP_POINTS = [("mt10-cov0-d2-u-m10", "dup"), ("mt10-cov0-d2-u-m10", 0), ("mt10-cov0-d2-u-m10", 7), ("mt10-cov1-d1-w-m10", "dup"), ("mt10-cov1-d1-w-m10", 30),
             ("mt10-cov2-d3-w-m10", 41), ("mt10-cov2-d1-u-m10", "dup"), ("mt20-cov1-d3-u-m20", 50), ("latent-mt10-cov0-d2", 33), ("latent-mt20-cov1-d3", 44),
             ("latent-mt30-cov2-d2", 60), ("mt30-cov2-d3-w-m30", 70)]


@pytest.mark.parametrize("cid,i", MP_POINTS)
def test_model_against_mpmath(cid, i):
    """The long-double values agree with 50-digit arithmetic to a thousandth of their own bounds: the reference's error does not count."""
    case = BY_ID[cid]
    if i == "dup":
        i = R.case_data(case).dup[1]
    P = R.eval_point(case, i)
    A, D, u, terms = _mp_point(case, i)
    assert len(A) == P.k
    for t in range(P.k):
        assert abs(P.A[t] - _ld(A[t])) <= 1e-3 * P.bA[t], (t, P.A[t], A[t])
    assert abs(P.D - _ld(D)) <= 1e-3 * P.bD and abs(P.u - _ld(u)) <= 1e-3 * P.bu
    for t in range(7):
        if t == 2 or (t >= 3 and not case.gauss):
            continue
        assert abs(P.terms[t] - _ld(terms[t])) <= 1e-3 * P.bterms[t], (R.TERMS[t], P.terms[t], terms[t], P.bterms[t])


# ---- the fp64 oracle inside the bounds -------------------------------------------------------------------------------------------------------------------------
def _oracle_point_ratios(orc, case):
    """largest |oracle - model| / bound over the checked points: (A, D, u, per-point terms)"""
    cd = R.case_data(case)
    ysafe = np.where(cd.nn >= 0, cd.y[np.maximum(cd.nn, 0)], 0.0)
    terms_o = None
    if case.wt:
        _, _, _, Ao, Do = orc.vecchia_nll_weighted(cd.coords, cd.nn, case.cov, (1.0, case.var, case.a), cd.y, cd.nug)
    elif case.gauss:
        Ao, Do, Ag, Dg, bad = orc.vecchia_factor(cd.coords, cd.nn, case.cov, case.var, case.a, gauss=True, grad=True)
        assert bad == 0
    else:
        Ao, Do, bad = orc.vecchia_factor(cd.coords, cd.nn, case.cov, case.var, case.a, gauss=False)
        assert bad == 0
    uo = cd.y - np.einsum("ij,ij->i", Ao, ysafe)
    if case.gauss and not case.wt:
        up = uo / Do
        terms_o = np.zeros((case.n, 7))
        terms_o[:, 0] = uo * uo / Do; terms_o[:, 1] = np.log(Do)
        for p in range(2):
            uk = -np.einsum("ij,ij->i", Ag[p], ysafe)
            terms_o[:, 3 + 2 * p] = uk * up - 0.5 * up * up * Dg[p]
            terms_o[:, 4 + 2 * p] = 0.5 * Dg[p] / Do
    worst = 0.0
    for i in R.checked_points(case):
        P = R.eval_point(case, i)
        assert np.all(Ao[i, P.k:] == 0)
        q = [R.ratio(Ao[i].astype(LD) - P.A, P.bA), R.ratio(LD(Do[i]) - P.D, P.bD), R.ratio(LD(uo[i]) - P.u, P.bu)]
        if terms_o is not None:
            q.append(R.ratio(terms_o[i].astype(LD) - P.terms, P.bterms))
        else:
            q.append(R.ratio(np.array([uo[i] ** 2 / Do[i], np.log(Do[i])], dtype=LD) - P.terms[:2], P.bterms[:2]))
        worst = max(worst, max(q))
    return worst


def test_oracle_is_inside_the_bounds(orc):
    """The fp64 oracle (host Cholesky, libm exp) at every checked point of every case of the GPU lists: inside the bounds, and by the margin recorded in
    vecchia_point_ref.ORACLE_WORST -- a plain fp64 evaluation uses a few per cent of a bound that has room for the device's faster arithmetic."""
    worst = {}
    for case in ALL:
        w = _oracle_point_ratios(orc, case)
        assert w <= 1.0, (case.id, w)
        worst[_class_of(case)] = max(worst.get(_class_of(case), 0.0), w)
    print("fp64 oracle, largest error / bound per class:", {k: "%.4f" % v for k, v in sorted(worst.items())})
    for k, v in worst.items():
        assert v <= 2 * R.ORACLE_WORST[k], (k, v)          # (the record; another libm moves it a little)


@pytest.mark.parametrize("cid", ["mt30-cov0-d2-u-m30", "mt62-cov2-d3-u-m51", "big-m126-cov1-d5-u"])
def test_sums_against_oracle(orc, cid):
    """orc_vecchia_nll_grad's sums (sigma2 = 1: gradient = g1 + g2) inside the summed bounds"""
    case = BY_ID[cid]
    cd = R.case_data(case)
    out, grad = orc.vecchia_nll_grad(cd.coords, cd.nn, case.cov, (1.0, case.var, case.a), cd.y)
    s, b, _ = R.sum_bounds(case, 0, case.n)
    assert abs(out[0] - s[0]) <= b[0] and abs(out[1] - s[1]) <= b[1]
    assert abs(grad[1] - (s[3] + s[4])) <= b[3] + b[4] and abs(grad[2] - (s[5] + s[6])) <= b[5] + b[6]
    g = np.asarray([s[3] + s[4], s[5] + s[6]], dtype=np.float64)
    assert np.allclose(grad[1:], g, rtol=1e-9)


# ---- the bounds are not vacuous --------------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("case", ALL, ids=[c.id for c in ALL])
def test_bounds_are_not_vacuous(case):
    for i in R.checked_points(case):
        P = R.eval_point(case, i)
        assert P.D > 0 and np.all(np.isfinite(P.bA.astype(np.float64))) and np.isfinite(float(P.bu))
        if case.gauss:
            assert P.bD / P.D <= 1e-11 and (P.k == 0 or P.bA.max() <= 1e-11), (i, float(P.bD / P.D), float(P.bA.max()))
        else:
            assert P.bD <= 1e-8 * case.var and (P.k == 0 or P.bA.max() <= 1e-8), (i, float(P.bD), float(P.bA.max()))


def test_eps_K_is_the_entry_bound_of_the_sweep():
    """(a): for the entries of c the bound of the model is eps_K(rho) K (+ the flush floor), for every shape"""
    for cov in range(3):
        rho = np.array([0.0, 1e-9, 0.3, 5.0, 40.0], dtype=LD)
        K, K1, _, _ = R.kern(cov, rho, 3.0)
        e = R.C_A[cov] * R.U * K + K1 * (R.U * R.C_R * rho)
        assert np.all(e <= R.eps_K(cov, rho) * K * (1 + 1e-15))
    coords, nn = R.covariance_sweep(1)
    rho = 8.0 * coords[1:, 0]
    assert rho[0] == 0 and rho.size > 280 and np.all(nn[1:, 0] == 0) and {700.0, 745.0, 800.0} <= set(rho)


# ---- the bounds have teeth -------------------------------------------------------------------------------------------------------------------------------------
def _leaves_bounds(case, mutant, terms=(0, 1, 3, 4, 5, 6)):
    for i in R.checked_points(case):
        P = R.eval_point(case, i); Q = R.eval_point(case, i, mutant)
        if P.k < 2:
            continue
        q = max(R.ratio(Q.A - P.A, P.bA), R.ratio(Q.D - P.D, P.bD), R.ratio(Q.u - P.u, P.bu), R.ratio((Q.terms - P.terms)[list(terms)], P.bterms[list(terms)]))
        if q > 1.0:
            return True
    return False


MUTANTS = [("entry_rel", "mt62-cov2-d3-w-m62", "mt10-cov2-d3-w-m10"), ("table_index", "mt62-cov2-d3-w-m62", "mt10-cov2-d3-w-m10"),
           ("newton_missing", "mt62-cov2-d3-w-m62", "mt10-cov2-d3-w-m10"), ("mirror", "mt62-cov2-d3-w-m62", None),
           ("nugget_shift", "mt62-cov2-d3-w-m62", "mt10-cov2-d3-w-m10"), ("last_dummy", "mt62-cov2-d3-w-m62", "mt10-cov2-d3-w-m10"),
           ("no_jitter", "latent-mt62-cov2-d3", "latent-mt10-cov0-d2"), ("m25_third", "mt62-cov2-d3-w-m62", "mt10-cov2-d3-w-m10")]


@pytest.mark.parametrize("mutant,big,small", MUTANTS, ids=[m[0] for m in MUTANTS])
def test_mutants_leave_the_bounds(mutant, big, small):
    """one covariance entry off by 2e-13 relative; the exp table index off by one in one entry; the Newton step of the square root missing; rows 16 and 31 of slot 1
    exchanged (no row 31 in a 10-neighbour case); the nugget of row r taken from row r + 1; the last real neighbour treated as a dummy; the 1e-10 jitter missing in a
    latent case; dK of Matern 2.5 without its 1/3 -- each leaves the bounds at some checked point of a 62-neighbour and of a 10-neighbour case"""
    for cid in (big, small):
        if cid is not None:
            assert _leaves_bounds(BY_ID[cid], mutant), (mutant, cid)


def test_mutants_do_change_only_what_they_name():
    case = BY_ID["mt62-cov2-d3-w-m62"]
    i = case.n - 1
    P = R.eval_point(case, i); Q = R.eval_point(case, i, "m25_third")
    assert np.array_equal(P.A, Q.A) and P.D == Q.D and not np.array_equal(P.terms[5:], Q.terms[5:]) and np.array_equal(P.terms[:5], Q.terms[:5])


@pytest.mark.parametrize("cid", ["mt62-cov2-d3-w-m62", "mt10-cov2-d3-w-m10"])
def test_a_point_missing_from_the_second_trip_leaves_the_logdet_bound(cid):
    """log D summed with one point of the second trip missing (two workers: worker 0's second trip is group 2, points 32 ..)"""
    case = BY_ID[cid]
    s, b, _ = R.sum_bounds(case, 0, case.n, nworkers=2)
    missing = [abs(R.eval_point(case, i).terms[1]) for i in range(32, 48)]
    assert min(missing) > b[1], (float(min(missing)), float(b[1]))


# ---- the sweep's bound against a CPU emulation of the device's covariance arithmetic ---------------------------------------------------------------------------
def _fma(a, b, c):
    return np.float64(LD(a) * LD(b) + LD(c))        # (64-bit mantissa: the product of two doubles is rounded once more than a true fma -- an emulation, not a model)


def _emulated_K(cov, var, a, x, delta0):
    """exp_of_scaled / matern_cov_s (dev_common.h) and A = K fast_rcp(var + 1) of the m = 1 factor in fp64, d = 1, neighbour at 0 and the point at x, with the hardware
    estimates of v_rsq_f64 and v_rcp_f64 replaced by the exact value times (1 + delta0); -> A (var + 1) in long double"""
    import math
    ln2_over_t, coord_scale = 0.0027076061740622863, 184.6649652337873
    sc = np.float64(a * coord_scale)
    dx = np.float64(np.float64(0.0 - x) * sc)
    d2 = _fma(dx, dx, 1e-300)
    h = np.float64(np.float64(1 / np.sqrt(LD(d2))) * (1 + delta0))
    g = np.float64(d2 * h); e = _fma(-h, g, 3.0); rp = np.float64(g * e)
    kf = np.rint(-rp); rr = -rp - kf
    k = int(kf) if abs(kf) < 2 ** 31 else -2 ** 31
    p = _fma(rr, 2.239395190875157e-12, 3.3083026805413713e-09); p = _fma(p, rr, 3.6655655969101062e-06); p = _fma(p, rr, ln2_over_t); p = _fma(p, rr, 1.0)
    tv = np.float64(2.0 ** ((k & 255) / 256) * var)
    try:
        ev = math.ldexp(float(np.float64(tv * p)), k >> 8)
    except OverflowError:
        ev = 0.0
    if ev < 2.2250738585072014e-308:
        ev = 0.0
    if cov == 0:
        K = ev
    elif cov == 1:
        K = np.float64(ev * _fma(rp, ln2_over_t, 1.0))
    else:
        r = np.float64(rp * ln2_over_t); K = np.float64(ev * _fma(r, _fma(r, 1.0 / 3.0, 1.0), 1.0))
    piv = np.float64(var + 1.0)
    y0 = np.float64(np.float64(1 / LD(piv)) * (1 + delta0))
    inv = _fma(y0, _fma(-piv, y0, 1.0), y0)
    return LD(np.float64(K * inv)) * (LD(var) + 1)


@pytest.mark.parametrize("delta0,limit", [(0.0, 0.2), (2.0 ** -25.4, 0.75), (-2.0 ** -25.4, 0.75), (2.0 ** -25, 1.0)])
def test_emulated_covariance_arithmetic_is_inside_the_sweep_bound(delta0, limit):
    """The device's operation sequence for one covariance value, restated in fp64 on the d = 1 sweep: inside eps_K(rho) K + 3 u K for an estimate error up to the
    assumed 2^-25 (measured here: 0.13 with exact estimates, 0.67 at the observed 2^-25.4, 0.97 at 2^-25 -- the Newton remainders dominate)."""
    for cov in range(3):
        case = [c for c in R.sweep_cases() if c.cov == cov and c.d == 1 and c.gauss][0]
        cd = R.case_data(case)
        worst = 0.0
        for i in range(1, case.n):
            x = cd.coords[i, 0]
            rho = LD(case.a) * LD(x)
            K = R.kern(cov, rho, case.var)[0]
            bound = (R.eps_K(cov, rho) + 3 * R.U) * K + LD(R.FLUSH) * case.var
            worst = max(worst, float(abs(_emulated_K(cov, case.var, case.a, x, delta0) - K) / bound))
        assert worst <= limit, (cov, delta0, worst)
