"""GPU (MI355X): every kernel of the full-scale Vecchia family (gpboost_amd/csrc/vif_kernels.hip), element by element, against the long-double model and the a-priori
bounds of tests/vif_kernel_ref.py (derived there before any device run; tests/test_vif_kernel_ref.py checks the model on the CPU).  The checks are layered: each kernel
against the long-double evaluation of ITS operation on the inputs the device had, read back through gpb_hip_vecchia_vif_get_matrix / _get_point_terms.

Instance cases cov<COV>-nt<NT>-m<m>-d<d> launch vif_resid_factor_kernel<COV, T, NT> and vif_resid_grad_kernel<COV, T, NT> (T = 64 for NT = 1..4, 128 for NT = 0): all 15.
Edge cases edge-m<m>-k<k>-n<n>-...: m + 1 on a tile edge (15, 31, 47), 63 and 64 rows on 64 lanes (m = 62, 63), the lanes-per-row switch of the derivative kernel
(m = 64 and the short rows of every case), m = 1, the largest m the LDS admits; k with a short last chunk that is no multiple of the MFMA K step (1, 3, 65, 130), 63,
255 / 256, k + 1 a multiple of 8 (7, 63, 255: no zero column after the response), the five k-vectors larger than the chunk buffer (m = 5, k = 256), five tile rows of the
Gram kernel (k = 256) over two chunks of rows (n = 257) and over one (n = 255, which wants k < n: k = 254), n below 256 and no multiple of 16.
One device run per case (two passes, each twice: bit-identical) is shared by the test functions, one per kernel."""
import functools
import json
import os

import numpy as np
import pytest

from tests import vif_kernel_ref as R

pytestmark = pytest.mark.gpu
LD = R.LD
ALL = R.all_cases()
IDS = [c.id for c in ALL]
WORST = {}        # "kernel quantity / NT / COV" -> (largest error / bound seen in this run, case, point): the table of DESIGN.md section 4.12
FACTOR_BUFFERS = ("C", "dC", "V", "Q", "QdC", "G")
GRAD_BUFFERS = ("Hm", "X1", "V1", "X2r", "v", "z")


@pytest.fixture(scope="module")
def gpb(lib_built):
    import gpboost_amd
    assert gpboost_amd.device_count() > 0, "no GPU visible: the -m gpu tests must run on the MI355X box"
    return gpboost_amd


def _two_passes(st, case, data, Linv, inputs):
    """vif_factor without and with the derivative inputs, vif_grad_sums; every buffer read back -> dict"""
    d = {}
    d["out3_plain"], d["G_plain"] = st.vif_factor(case.cov, case.var, case.a, Linv, with_grad=False)
    d["C_plain"], d["Q_plain"] = st.vif_get_matrix("C"), st.vif_get_matrix("Q")
    d["out3"], d["G_host"] = st.vif_factor(case.cov, case.var, case.a, Linv, with_grad=True)
    for name in FACTOR_BUFFERS:
        d[name] = st.vif_get_matrix(name)
    d["A"], d["D"], d["u"] = st.get_factor()
    d["part3"] = st.vif_get_point_terms(3)
    if inputs is None:
        R.add_grad_pass(case, data, d, lambda dev: None)
    else:
        d.update(inputs)
    d["sums12"] = st.vif_grad_sums(case.cov, case.var, case.a, d["Winv"], d["Si"], d["N0"], d["negMp1"], d["w"][:case.k], keep_factor=True)
    for name in GRAD_BUFFERS:
        d[name] = st.vif_get_matrix(name)
    d["part12"] = st.vif_get_point_terms(12)
    both = [st.vif_get_grad_factor(p) for p in range(2)]
    d["dA"], d["dD"] = np.stack([b[0] for b in both]), np.stack([b[1] for b in both])
    return d


@functools.lru_cache(maxsize=None)
def _device(case):
    """-> (data with the device's own neighbour table, the device's buffers).  Winv, Si, N0, negMp1, w: the true ones, in long double from the device's G, rounded."""
    from gpboost_amd import shim
    base = R.case_data(case)
    st = shim.VecchiaState(base.coords, case.m)
    assert st.m == case.m
    st.find_neighbors()
    data = base._replace(nn=st.get_neighbors())
    assert np.all((data.nn >= 0).sum(axis=1) == np.minimum(np.arange(case.n), case.m))
    st.set_y(base.y)
    st.vif_set_inducing_points(base.ip)
    Linv = R.whitening(case, base.ip)
    kq = R.vif_kq(case.k)
    try:
        dev = _two_passes(st, case, data, Linv, None)
        inputs = {key: dev[key] for key in ("Winv", "Si", "N0", "negMp1", "w", "M_Winv", "M_Si", "M_N0", "M_negMp1")}
        again = _two_passes(st, case, data, Linv, inputs)
    except Exception as e:      # a fault of the device ends the session: nothing more is started on it
        if any(word in str(e) for word in ("illegal memory access", "launch failure", "hardware exception", "device lost")):
            pytest.exit("%s: the device faulted: %s" % (case.id, e), returncode=3)
        raise
    st.close()
    dev["not_reproduced"] = [key for key in again if isinstance(again[key], np.ndarray) and key not in inputs
                             and not np.array_equal(again[key].view(np.uint64), dev[key].view(np.uint64))]
    dev["Linv"], dev["M_Linv"] = Linv, R.pad_kq(Linv, case.k, kq, transpose=True)
    return data, dev


def _finish(case, F):
    for (kernel, what), (q, where) in F.worst.items():
        key = "%s %s / NT=%d / COV=%d" % (kernel, what, R.vif_tiles(case.m), case.cov)
        if q >= WORST.get(key, (-1.0, "", None))[0]:
            WORST[key] = (q, case.id, where)
    print("%s: %s" % (case.id, {"%s %s" % kw: round(v[0], 4) for kw, v in F.worst.items()}))
    assert F.ok(), F.report()


@pytest.mark.parametrize("case", ALL, ids=IDS)
def test_crosscov(gpb, case):
    """C and dC within their bounds everywhere; column k is the response, the columns beyond exactly 0; C of the form without dC bit for bit that of the form with it"""
    data, dev = _device(case)
    _finish(case, R.check_crosscov(case, data, dev))


@pytest.mark.parametrize("case", ALL, ids=IDS)
def test_gemm(gpb, case):
    """V = C Linv' and the four products of the gradient pass (Hm, X1, V1, and X2r with its accumulated second product), every entry; columns >= k exactly 0"""
    data, dev = _device(case)
    F = R.check_gemm_factor(case, data, dev)
    _finish(case, R.check_gemm_grad(case, data, dev, F))


@pytest.mark.parametrize("case", ALL, ids=IDS)
def test_resid_factor(gpb, case):
    """A, D, u at the checked points from the device's own V; A exactly 0 at the -1 positions; the three per-point partials from the device's own D and u to 3 roundings;
    out3 against the long-double sum of the per-point partials"""
    data, dev = _device(case)
    _finish(case, R.check_factor(case, data, dev))
    assert np.array_equal(dev["out3"], dev["out3_plain"])


@pytest.mark.parametrize("case", ALL, ids=IDS)
def test_spmm(gpb, case):
    """Q = B C and QdC = B dC, every entry; the two-matrix form's Q bit for bit the single-matrix form's"""
    data, dev = _device(case)
    _finish(case, R.check_spmm(case, data, dev))


@pytest.mark.parametrize("case", ALL, ids=IDS)
def test_gram(gpb, case):
    """every entry of G (kq x kq) from the device's own Q and D; exactly symmetric; the (k + 1) x (k + 1) block handed to the host is that of the device buffer"""
    data, dev = _device(case)
    _finish(case, R.check_gram(case, data, dev))
    k = case.k
    assert np.array_equal(dev["G_host"], dev["G"][:k + 1, :k + 1]) and np.array_equal(dev["G_plain"], dev["G_host"])


@pytest.mark.parametrize("case", ALL, ids=IDS)
def test_vec(gpb, case):
    data, dev = _device(case)
    _finish(case, R.check_vec(case, data, dev))


@pytest.mark.parametrize("case", ALL, ids=IDS)
def test_resid_grad(gpb, case):
    """dA, dD and the twelve per-point terms at the checked points from the device's own buffers; sums12 against the long-double sum of the per-point terms"""
    data, dev = _device(case)
    _finish(case, R.check_grad(case, data, dev))


@pytest.mark.parametrize("case", ALL, ids=IDS)
def test_second_call_is_bit_identical(gpb, case):
    data, dev = _device(case)
    assert not dev["not_reproduced"], dev["not_reproduced"]


def test_one_neighbour_too_many_is_refused_by_name(gpb):
    """m above the largest admitted one: gpb_hip_vecchia_vif_set_inducing_points refuses with its message, and nothing can be launched on the handle afterwards"""
    from gpboost_amd import shim
    case = R.case_by_id("edge-m%d-k7-" % R.largest_admitted_m(7))
    data = R.case_data(case)
    st = shim.VecchiaState(data.coords, case.m + 1)
    assert st.m == case.m + 1
    st.find_neighbors()
    st.set_y(data.y)
    with pytest.raises(gpb.GPBoostError, match="full-scale Vecchia: %d neighbours x 7 inducing points exceed the LDS of a CU" % (case.m + 1)):
        st.vif_set_inducing_points(data.ip)
    with pytest.raises(gpb.GPBoostError, match="no inducing points have been set"):
        st.vif_factor(case.cov, case.var, case.a, R.whitening(case, data.ip))
    st.close()


def test_seam_names_the_missing_call(gpb):
    """the read-only seam copies only what the last call produced"""
    from gpboost_amd import shim
    case = ALL[0]
    data = R.case_data(case)
    st = shim.VecchiaState(data.coords, case.m)
    st.find_neighbors()
    st.set_y(data.y)
    st.vif_set_inducing_points(data.ip)
    with pytest.raises(gpb.GPBoostError, match="needs gpb_hip_vecchia_vif_factor first"):
        st.vif_get_matrix("C")
    Linv = R.whitening(case, data.ip)
    st.vif_factor(case.cov, case.var, case.a, Linv, with_grad=False)
    with pytest.raises(gpb.GPBoostError, match=r"needs gpb_hip_vecchia_vif_factor\(with_grad = 1\) first"):
        st.vif_get_matrix("dC")
    with pytest.raises(gpb.GPBoostError, match="needs gpb_hip_vecchia_vif_grad_sums first"):
        st.vif_get_matrix("Hm")
    with pytest.raises(gpb.GPBoostError, match="needs gpb_hip_vecchia_vif_grad_sums as the last"):
        st.vif_get_point_terms(12)
    assert st.vif_get_point_terms(3).shape == (3, case.n)
    st.set_y(data.y)              # a new response: Q, G, v, z of the old one are gone
    with pytest.raises(gpb.GPBoostError, match="needs gpb_hip_vecchia_vif_factor first"):
        st.vif_get_matrix("Q")
    st.close()


# ---- the k-means assignment kernel (kmeans_assign_kernel of nn_kernels.hip, through gpb_hip_kmeans_lloyd) --------------------------------------------------------
def _kmeans_device(x, means, max_it):
    import ctypes as C
    from gpboost_amd.basic import _lib, _shim_call
    xf = np.asfortranarray(x, dtype=np.float64)
    out = np.array(means, dtype=np.float64, order="C")
    it = C.c_int32(0)
    p = lambda a: a.ctypes.data_as(C.POINTER(C.c_double))
    _shim_call(_lib().gpb_hip_kmeans_lloyd(C.c_int32(x.shape[0]), C.c_int32(x.shape[1]), p(xf), C.c_int32(out.shape[0]), p(out), C.c_int32(int(max_it)), C.byref(it)))
    return out, it.value


@pytest.mark.parametrize("n", [257, 1000])
@pytest.mark.parametrize("k", [1, 2, 256])
@pytest.mark.parametrize("d", [1, 2, 3])
def test_kmeans_lloyd_on_a_lattice(gpb, d, k, n):
    """Points and start means on an integer lattice: every difference, square and sum of the first assignment is exact and ties are true ties (the first mean wins).
    Means and iteration count after max_it = 1, 2, 1000 bit for bit those of the numpy restatement (checked on the CPU against the oracle's kmeans++).  Start means 0 and 1
    are identical: in the first iteration the first takes all their rows, the second attracts none and keeps its value, as does at every iteration a mean placed
    far from every point."""
    rng = np.random.default_rng(100 * d + k + n)
    x = rng.integers(0, 16, size=(n, d)).astype(np.float64)
    start = rng.integers(0, 16, size=(k, d)).astype(np.float64)
    if k >= 2:
        start[1] = start[0]
    if k >= 3:
        start[2] = 1000.0
    for max_it in (1, 2, 1000):
        want, want_it = R.kmeans_lloyd_ref(x, start, max_it)
        got, got_it = _kmeans_device(x, start, max_it)
        assert got_it == want_it and np.array_equal(got.view(np.uint64), want.view(np.uint64)), (max_it, got_it, want_it)
        assert max_it != 1000 or got_it < 1000
        if k >= 2 and max_it == 1:      # (from the second iteration on the first mean has moved and the second attracts rows)
            assert np.array_equal(got[1], start[1])
        if k >= 3:
            assert np.array_equal(got[2], start[2])
    if k == 1:
        assert np.array_equal(got[0], np.cumsum(x, axis=0)[-1] / n)


def test_zz_report_worst_ratios(gpb):
    """Not a check: prints the largest error / bound per class (kernel and quantity x NT x COV) seen by the tests above (the table of DESIGN.md section 4.12), and writes
    it to the file named by GPB_VIF_RATIOS_OUT if that is set."""
    txt = json.dumps({key: [round(v[0], 4), v[1], v[2]] for key, v in sorted(WORST.items())}, indent=1)
    print("full-scale Vecchia kernels, largest error / bound per class:\n" + txt)
    out = os.environ.get("GPB_VIF_RATIOS_OUT")
    if out:
        with open(out, "w") as f:
            f.write(txt + "\n")
