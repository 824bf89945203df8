"""CPU: the long-double model of the full-scale Vecchia kernels (tests/vif_kernel_ref.py) -- that it is the operation the project means (against
tests/vif_harness.py NumpyDevice and oracle/orc.py vif_grad_terms), that its bounds are usable (positive, finite, and wide enough for the plain double evaluation of the
same operations), that each mutant of the model leaves them by a factor of 8 at least, and that the case tables cover what tests/test_zz_vif_kernels_gpu.py claims."""
import functools

import numpy as np
import pytest

from tests import cases
from tests import vif_kernel_ref as R

LD = R.LD
ALL = R.all_cases()

pytestmark = pytest.mark.skipif(not R.long_double_is_wider(), reason="np.longdouble is not wider than double on this machine")


@functools.lru_cache(maxsize=None)
def _double_device(case):
    return R.double_device(case, R.case_data(case))


def _rel(a, b):
    a, b = np.asarray(a, dtype=LD), np.asarray(b, dtype=LD)
    return float(np.max(np.abs(a - b)) / max(float(np.max(np.abs(b))), 1e-300))


@pytest.mark.parametrize("name", ["vif_u2d_n1500_exp_m15_k40_none", "vif_u3d_n2000_mat25_m20_k64_random"])
def test_model_reproduces_the_numpy_device_and_the_oracle(orc, name):
    """A, D, u, dA, dD per point and the summed twelve terms of the long-double model to 1e-10 relative: against NumpyDevice (double) fed with the same k x k inputs, and
    A, D, dA, dD against orc.vif_grad_terms (the restatement of the reference's own derivative branches)."""
    from tests import vif_harness as vh
    n, d, cf, sh, m, k, ordering, seed, cps = cases.VIF_CASES[name]
    coords, y = cases.vif_data(name)
    ct = orc.cov_type_id(cf, sh)
    perm, co, nn, ip = orc.vif_setup(coords, m, k, ordering, seed)
    pt = orc.transform_cov_pars(ct, np.asarray(cps[0]))
    case = R.Case(name, "vif", n, m, k, d, ct, float(pt[1]), float(pt[2]), 0)
    data = R.CaseData(co, y[perm], ip, nn)
    kq = R.vif_kq(k)
    nd = vh.NumpyDevice(co, nn, ip, ct, case.var, case.a, data.y)
    Linv = R.whitening(case, ip)
    o3, G = nd.factor(Linv, True)
    Winv, Si, N0, negMp1, w = R.grad_inputs(case, ip, G)
    S = nd.grad_sums(Winv, Si, N0, negMp1, w)
    quad, logdet, gg, odA, odD, oA, oD = orc.vif_grad_terms(co, nn, ip, ct, case.var, case.a, data.y)

    def pad(X, last=None):
        out = np.zeros((n, kq))
        out[:, :k] = X
        if last is not None:
            out[:, k] = last
        return out
    dev = dict(C=pad(nd.C, data.y), dC=pad(nd.dC), A=nd.A, D=nd.D, Q=pad(nd.Q, nd.u), QdC=pad(nd.QdC))
    dev["V"] = R.product(dev["C"], R.pad_kq(Linv, k, kq, transpose=True)).astype(np.float64)
    wq = np.zeros(kq)
    wq[:k] = w
    dev["w"] = wq
    for out, In, M in (("Hm", "Q", Winv), ("X1", "Q", Si), ("V1", "Q", N0)):
        dev[out] = R.product(dev[In], R.pad_kq(M, k, kq)).astype(np.float64)
    dev["X2r"] = R.product_acc(R.product(dev["QdC"], R.pad_kq(Si, k, kq)).astype(np.float64), dev["Q"], R.pad_kq(negMp1, k, kq)).astype(np.float64)
    v, z = R.vec(dev["Q"], dev["C"], dev["D"], wq, k)
    dev["v"], dev["z"] = v.astype(np.float64), z.astype(np.float64)
    A, D, u = np.zeros((n, m), dtype=LD), np.zeros(n, dtype=LD), np.zeros(n, dtype=LD)
    dA, dD, T = np.zeros((2, n, m), dtype=LD), np.zeros((2, n), dtype=LD), np.zeros((12, n), dtype=LD)
    for i in range(n):
        P = R.point_factor(case, data, i, dev["V"])
        A[i], D[i], u[i] = P["A"], P["D"], P["u"]
        g = R.point_grad(case, data, i, dev, bounds=False)
        dA[:, i], dD[:, i], T[:, i] = g["dA"], g["dD"], g["terms"]
    assert _rel(A, nd.A) <= 1e-10 and _rel(D, nd.D) <= 1e-10 and _rel(u, nd.u) <= 1e-10
    assert _rel(A, oA) <= 1e-10 and _rel(D, oD) <= 1e-10
    for p in range(2):
        assert _rel(dA[p], odA[p]) <= 1e-10 and _rel(dD[p], odD[p]) <= 1e-10, p
    Ts = T.sum(axis=1)
    assert np.all(np.abs(Ts - S) <= 1e-10 * np.abs(S)), (Ts, S)


@pytest.mark.parametrize("case", ALL, ids=[c.id for c in ALL])
def test_plain_double_stays_inside_every_bound(case):
    """Every kernel evaluated in plain double on the outputs of the one before: within every bound (a bound the obvious double evaluation breaks is wrong), every exact
    condition holds, every bound is finite and positive somewhere."""
    data = R.case_data(case)
    dev = _double_device(case)
    F = R.Findings()
    for chk in R.CHECKS:
        chk(case, data, dev, F)
    assert F.ok(), F.report()
    assert not F.bad_bounds, F.bad_bounds            # finite and not negative everywhere, zero only where the value is identically zero (a row without neighbours) ...
    assert all(b > 0 for b in F.largest_bound.values()), F.largest_bound      # ... and positive somewhere for every quantity
    kernels = {kw[0] for kw in F.worst}
    assert kernels == {"crosscov", "gemm", "resid_factor", "reduce", "spmm", "gram", "vec", "resid_grad"}
    print("%s: largest error / bound of the double evaluation %.3g" % (case.id, F.largest()))


@pytest.mark.parametrize("mutant", sorted(R.MUTANTS))
def test_every_mutant_leaves_its_bound(mutant):
    """at least one checked entry of the case designed for the mutant exceeds its bound by a factor of 8 or more"""
    case = R.case_by_id(R.MUTANTS[mutant])
    q = R.mutant_excess(mutant, _double_device(case))
    print("%s on %s: %.3g x the bound" % (mutant, case.id, q))
    assert q >= 8.0, (mutant, case.id, q)


def test_case_tables_cover_what_they_claim():
    inst, edge = R.instance_cases(), R.edge_cases()
    assert sorted((c.cov, R.vif_tiles(c.m)) for c in inst) == sorted((cov, nt) for cov in range(3) for nt in range(5))
    assert all(("cov%d-nt%d-" % (c.cov, R.vif_tiles(c.m))) in c.id for c in inst) and len({c.id for c in ALL}) == len(ALL)
    assert all(c.n == 331 and c.k == 37 for c in inst) and {c.d for c in inst} == {1, 2, 3}
    ms, ks = {c.m for c in ALL}, {c.k for c in edge}
    assert {1, 15, 16, 31, 32, 47, 48, 62, 63, 64} <= ms
    # the largest admitted m and the first refused one, from the restated formula of vif_resid_lds_bytes
    top = R.largest_admitted_m(7)
    assert top in {c.m for c in edge if c.k == 7} and R.resid_lds_bytes(top, 8) <= R.resid_lds_max() < R.resid_lds_bytes(top + 1, 8) and top + 1 <= 126
    # chunk, K-step and kq edges of the inducing-point count
    assert {1, 3, 7, 63, 64, 65, 130, 255, 256} <= ks
    assert any(c.k % 64 % 4 != 0 and c.k % 64 < 8 for c in edge) and any(R.vif_kq(c.k) == c.k + 1 for c in edge)
    assert any(R.vectors_exceed_chunk(c.m, c.k) for c in edge) and not any(R.vectors_exceed_chunk(c.m, c.k) for c in inst)
    assert any((R.vif_kq(c.k) + 63) // 64 == 5 for c in edge)
    assert any(R.gram_chunks(c.n, R.vif_kq(c.k)) == 2 for c in edge) and any(c.n < 256 for c in edge) and any(c.n % 16 for c in ALL) and all(c.n <= 600 for c in ALL)
    # the lanes-per-row edges of the derivative kernel: both sides of both edges for one and for two wavefronts, each row among the checked points
    for T, rows in ((64, (16, 17, 32, 33)), (128, (32, 33, 64, 65))):
        seen = set()
        for c in ALL:
            if R.threads_of(c.m) == T:
                pts = R.checked_points(c)
                assert len(pts) <= 24 and {0, 1, c.m - 1, c.m, c.m + 1, c.n - 1} & set(range(c.n)) <= set(pts)
                seen |= {min(i, c.m) + 1 for i in pts}
        assert set(rows) <= seen, (T, seen)
        assert [R.lpr_of(r, T) for r in rows] == [4, 2, 2, 1]
    assert all(c.k < c.n for c in ALL)
    for mutant, prefix in R.MUTANTS.items():
        R.case_by_id(prefix)


def test_kmeans_restatement_against_the_oracle(orc):
    """kmeans_lloyd_ref continues the oracle's kmeans++ run (orc.vif_setup: the reference's generator and start) from its first iterate to the same inducing points"""
    name = "vif_u2d_n1500_exp_m15_k40_random"
    n, d, cf, sh, m, k, ordering, seed, cps = cases.VIF_CASES[name]
    coords, _ = cases.vif_data(name)
    first = orc.vif_setup(coords, m, k, ordering, seed, max_it=1)
    third = orc.vif_setup(coords, m, k, ordering, seed, max_it=3)
    last = orc.vif_setup(coords, m, k, ordering, seed)
    assert not np.array_equal(first[3], third[3])
    means, count = R.kmeans_lloyd_ref(first[1], first[3], 2)
    assert count == 2 and np.array_equal(means, third[3])
    means, count = R.kmeans_lloyd_ref(first[1], first[3], 1000)
    assert 2 < count < 1000 and np.array_equal(means, last[3])
