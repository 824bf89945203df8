"""GPU (MI355X): every instance of vecchia_point_kernel<MT, COV, D3, MODE, WT> (gpboost_amd/csrc/vecchia_kernels.hip) and every (dk, cov, mode, weights) combination of
the generality kernel (vecchia_big_kernels.hip), per point, against the long-double model and the a-priori bounds of tests/vecchia_point_ref.py (derived there before
any device run; tests/test_vecchia_point_ref.py checks the model on the CPU).

Which instance a case launches is vecchia_point_ref.instance_of(case, mode); the case id names it: mt<MT>-cov<COV>-d<d>-<u|w>-m<m> launches <MT, COV, d == 3, mode, WT>
in the three modes (WT = weights, or the run-time weighted gradient instance of MT = 40 that serves both), latent-mt<MT>-... the unweighted instance with
gauss = False (nll and factor), big-m<m>-cov<COV>-d<d>-<u|w> vecchia_point_big_kernel<COV, dk = 2 | 3 | 0 (d = 5), mode>.  Every point-kernel case runs twice: with the
default grid (one trip per worker at these sizes) and with gpb_hip_vecchia_set_worker_cap(2), where each of the two workers makes at least two trips, unevenly -- the
prefetch of the next trip's indices, the running sums and the running product behind log|Psi| only run from the second trip on."""
import json
import os

import numpy as np
import pytest

from tests import vecchia_point_ref as R

pytestmark = pytest.mark.gpu
LD = R.LD
MODE_NAMES = ("nll", "factor", "grad")
INST, LATENT, BIG, SWEEP = R.instance_cases(), R.latent_cases(), R.big_cases(), R.sweep_cases()
WORST = {}        # class -> (largest error / bound seen in this run, where: case, point or shard, term) (printed by the last test: the table of DESIGN.md section 3)


@pytest.fixture(scope="module")
def gpb(lib_built):
    import gpboost_amd
    assert gpboost_amd.device_count() > 0, "no GPU visible: the -m gpu tests must run on the MI355X box"
    return gpboost_amd


def _left_looking(mt, mode):
    ns = (mt + 2 + 15) // 16
    return mt > 30 and (mode == 0 or ns == 3)


def _class(case, mode):
    if case.kind == "big":
        return "big m=%d/%s/%s" % (case.m, MODE_NAMES[mode], "weighted" if case.wt else "uniform")
    return "MT=%d/%s/%s/%s" % (case.mt, MODE_NAMES[mode], "left" if _left_looking(case.mt, mode) else "right",
                               "latent" if not case.gauss else ("weighted" if case.wt else "uniform"))


def _note(case, mode, q, where=""):
    key = _class(case, mode)
    if float(q) >= WORST.get(key, (-1.0, ""))[0]:
        WORST[key] = (float(q), "%s %s" % (case.id, where))


def _worst_term(err, bound, names):
    """(largest |err| / bound, the name of the entry that attains it)"""
    qs = [R.ratio(e, b) for e, b in zip(np.atleast_1d(err), np.atleast_1d(bound))]
    j = int(np.argmax(qs))
    return qs[j], names[j]


def _state(case):
    from gpboost_amd import shim
    cd = R.case_data(case)
    st = shim.VecchiaState(cd.coords, case.m)
    assert st.m == case.m
    st.set_neighbors(cd.nn)
    st.set_y(cd.y)
    if case.wt:
        st.set_nugget_diag(cd.nug)
    return st, cd


def _caps(case):
    return (0,) if case.kind == "big" else (0, 2)


# ---- (a) the covariance function alone ------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("case", SWEEP, ids=[c.id for c in SWEEP])
def test_covariance_function_alone(gpb, case):
    """m = 1: A_i diag = K(dist_i0) to three roundings (the product with the pivot's reciprocal); K_dev within eps_K(rho) K + 3 u K of the long-double value (entries below
    1e-300 var absolutely: v_ldexp_f64 flushes them).  In grad mode a single-point shard at EVERY point of the sweep pins dK through the per-point terms (Gaussian cases)."""
    st, cd = _state(case)
    st.factor(case.cov, case.var, case.a, gauss=case.gauss)
    A, D, u = st.get_factor()
    diag = LD(case.var) + 1 if case.gauss else LD(float(case.var) * (1.0 + 1e-10))
    rho = LD(case.a) * np.sqrt(np.sum((cd.coords[1:].astype(LD) - cd.coords[0].astype(LD)) ** 2, axis=1))
    K = R.kern(case.cov, rho, case.var)[0]
    Kdev = A[1:, 0].astype(LD) * diag
    bound = (R.eps_K(case.cov, rho) + 3 * R.U) * K + LD(R.FLUSH) * LD(case.var)
    err = np.abs(Kdev - K)
    worst = int(np.argmax(err / bound))
    print("%s: largest error / bound %.3f at rho = %.17g" % (case.id, float(err[worst] / bound[worst]), float(rho[worst])))
    bad = np.nonzero(~(err <= bound))[0]
    assert bad.size == 0, [(float(rho[j]), float(Kdev[j]), float(K[j]), float(err[j] / bound[j])) for j in bad[:5]]
    WORST["sweep cov=%d" % case.cov] = max(WORST.get("sweep cov=%d" % case.cov, (0.0, "")), (float(err[worst] / bound[worst]), "%s rho=%.6g" % (case.id, float(rho[worst]))))
    assert np.all(Kdev[rho > 760] == 0) and A[0, 0] == 0
    if not case.gauss:          # (the gradient entry point is Gaussian only)
        st.close()
        return
    for i in range(1, case.n):      # every point of the sweep
        P = R.eval_point(case, i)
        assert abs(LD(D[i]) - P.D) <= P.bD and abs(LD(u[i]) - P.u) <= P.bu, i
        st.set_shard(i, i + 1)
        t = st.grad_terms(case.cov, case.var, case.a)
        q = R.ratio(t.astype(LD) - P.terms, P.bterms)
        assert q <= 1.0 and t[2] == 0, (i, float(rho[i - 1]), t, P.terms, P.bterms)
        WORST["sweep dK cov=%d" % case.cov] = max(WORST.get("sweep dK cov=%d" % case.cov, (0.0, "")), (q, "%s rho=%.6g" % (case.id, float(rho[i - 1]))))
    st.close()


# ---- (b), (d) factor mode ------------------------------------------------------------------------------------------------------------------------------------------
FACTOR_CASES = INST + LATENT + BIG


@pytest.mark.parametrize("case", FACTOR_CASES, ids=[c.id for c in FACTOR_CASES])
def test_factor_per_point(gpb, case):
    """A, D, u within their bounds at every checked point, A exactly 0 at the -1 positions of every row, and bit-identical with the default grid and with two workers."""
    st, cd = _state(case)
    runs = []
    for cap in _caps(case):
        st.set_worker_cap(cap)
        st.factor(case.cov, case.var, case.a, gauss=case.gauss)
        runs.append(st.get_factor())
    st.close()
    A, D, u = runs[0]
    assert np.all(A[cd.nn < 0] == 0)
    for i in R.checked_points(case):
        P = R.eval_point(case, i)
        qa, qd, qu = R.ratio(A[i].astype(LD) - P.A, P.bA), R.ratio(LD(D[i]) - P.D, P.bD), R.ratio(LD(u[i]) - P.u, P.bu)
        _note(case, 1, max(qa, qd, qu), "point %d %s" % (i, "ADu"[int(np.argmax([qa, qd, qu]))]))
        assert max(qa, qd, qu) <= 1.0, (i, qa, qd, qu)
    for other in runs[1:]:
        for x, z in zip(runs[0], other):
            assert np.array_equal(x.view(np.uint64), z.view(np.uint64)), "the values of a point depend on the trip that computed it"


# ---- (c), (d) nll and grad modes -------------------------------------------------------------------------------------------------------------------------------------
TERM_CASES = [(c, mode) for c in INST + BIG for mode in (0, 2)] + [(c, 0) for c in LATENT]


def _terms(st, case, mode):
    if mode == 0:
        return st.nll_terms(case.cov, case.var, case.a, gauss=case.gauss)
    return st.grad_terms(case.cov, case.var, case.a)


@pytest.mark.parametrize("case,mode", TERM_CASES, ids=["%s-%s" % (c.id, MODE_NAMES[mode]) for c, mode in TERM_CASES])
def test_terms_per_point_and_sums(gpb, case, mode):
    """Single-point shards (one active row of 16) at 12 of the checked points: every term within its bound, bad == 0.  The whole range and the unaligned shard
    [7, n - 9): the sums within the summed bounds, with the default grid and with two workers, the two within gamma(ngroups + 16) x the sum of the absolute per-point
    values of each other.  Grad mode's first three terms agree with nll mode's within twice the bound."""
    nt = 3 if mode == 0 else 7
    st, cd = _state(case)
    n = case.n
    for i in R.checked_points(case)[::2]:
        P = R.eval_point(case, i)
        st.set_shard(i, i + 1)
        t = _terms(st, case, mode)
        q, name = _worst_term(t.astype(LD) - P.terms[:nt], P.bterms[:nt], R.TERMS)
        _note(case, mode, q, "point %d %s" % (i, name))
        assert q <= 1.0 and t[2] == 0, (i, t, P.terms[:nt], P.bterms[:nt])
    for i0, i1 in ((0, n), (7, n - 9)):
        st.set_shard(i0, i1)
        ngroups = (i1 - i0 + 15) // 16
        got = []
        for cap in _caps(case):
            st.set_worker_cap(cap)
            t = _terms(st, case, mode)
            s, b, sabs = R.sum_bounds(case, i0, i1, nworkers=min(ngroups, cap) if cap else ngroups, nterms=nt)
            q, name = _worst_term(t.astype(LD) - s, b, R.TERMS)
            _note(case, mode, q, "sum [%d, %d) cap %d %s" % (i0, i1, cap, name))
            assert q <= 1.0 and t[2] == 0, (i0, i1, cap, t, s, b)
            got.append(t)
        st.set_worker_cap(0)
        if len(got) == 2:
            assert np.all(np.abs(got[0].astype(LD) - got[1].astype(LD)) <= R.gamma(ngroups + 16) * sabs), (got, sabs)
        if mode == 2:
            t0 = st.nll_terms(case.cov, case.var, case.a)
            s, b, _ = R.sum_bounds(case, i0, i1, nterms=3)
            assert np.all(np.abs(got[0][:3].astype(LD) - t0.astype(LD)) <= 2 * b), (got[0][:3], t0, b)
    st.close()


def test_zz_report_worst_ratios(gpb):
    """Not a check: prints the largest error / bound per class seen by the tests above (the table of DESIGN.md section 3), and writes it to the file named by
    GPB_POINT_RATIOS_OUT if that is set."""
    txt = json.dumps({k: [round(v[0], 4), v[1]] for k, v in sorted(WORST.items())}, indent=1)
    print("vecchia point kernels, largest error / bound per class:\n" + txt)
    out = os.environ.get("GPB_POINT_RATIOS_OUT")
    if out:
        with open(out, "w") as f:
            f.write(txt + "\n")
