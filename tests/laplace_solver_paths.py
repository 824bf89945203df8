"""Case table of tests/test_zz_laplace_solver_paths_gpu.py: small Vecchia-Laplace runs through the C ABI that take every exit of the host's conjugate-gradient loops
(converged, iteration cap, warm start) and every partial block of the block solves, and the recording step that wrote tests/golden/laplace_solver_paths_mi355x.npz.

Every case is a function (shim) -> {field: number or array}.  All of them share n = 192 points in the unit square, m = 10 neighbours, Matern-1.5 at fixed
(var, a), and num_rand_vec = 6: two chunks of four probe columns, the last chunk with two padding columns.  CAP (3 CG iterations per solve, 4 Lanczos steps) ends
every loop at its cap; the defaults end them at their tolerance.

The recording is NOT a test: `python -m tests.laplace_solver_paths record OUT.npz` runs the table once on the GPU and writes the fields; `merge` puts several such files
(separate processes) together: a field they all agree on bit for bit is stored once and compared exactly, any other gets the first run's value and "<key>@spread", the
largest absolute difference between two runs."""
import ctypes as C
import sys

import numpy as np

N, M, T = 192, 10, 6
COV, VAR, A = 1, 1.0, np.sqrt(3.0) / 0.2          # Matern-1.5, sigma1^2 = 1, range 0.2
CAP = dict(cg_max_num_it=3, cg_max_num_it_tridiag=4)
N_PRED, N_SMALL, K_VIF, K_PC = 11, 40, 10, 8
PRED_TOL = 1e-10


def data(n=N, seed=11):
    rng = np.random.default_rng(seed)
    co = rng.uniform(size=(n, 2))
    f = 2.0 * np.sin(5.0 * co[:, 0]) * np.cos(3.0 * co[:, 1])
    d = dict(coords=co, y01=(rng.uniform(size=n) < 1.0 / (1.0 + np.exp(-f))).astype(np.int32), yreal=f + 0.5 * rng.standard_normal(n),
             ypos=np.exp(0.5 * f) * rng.gamma(2.0, 0.5, size=n), ip_pc=rng.uniform(size=(K_PC, 2)), ip_vif=rng.uniform(size=(K_VIF, 2)),
             coords_pred=rng.uniform(size=(N_PRED, 2)))
    # sparse rows of the quadratic forms: three distinct columns per row, one row padded with -1
    d["qf_cols"] = np.stack([rng.permutation(n)[:3] for _ in range(N_PRED)]).astype(np.int32)
    d["qf_vals"] = rng.standard_normal((N_PRED, 3))
    d["qf_cols"][4, 2] = -1
    return d


def _state(shim, d, pc="vadu", lik="bernoulli_logit", vif=False):
    st = shim.VecchiaState(d["coords"], M)
    st.find_neighbors()
    if vif:
        st.vif_set_inducing_points(d["ip_vif"])
    st.laplace_set_likelihood(lik)
    if lik == "bernoulli_logit":
        st.laplace_set_labels(d["y01"])
    else:
        st.laplace_set_response_real(d["ypos"] if lik == "gamma" else d["yreal"])
        st.laplace_set_aux({"gamma": 2.0, "gaussian_latent": 0.25}[lik])
    st.laplace_set_preconditioner(pc, K_PC if pc in ("pivoted_cholesky", "fitc") else -999)
    if pc == "fitc":
        st.laplace_set_inducing_points(d["ip_pc"])
    return st


def _eval(st, tag, **kw):
    nll, info = st.laplace_logit(COV, VAR, A, num_rand_vec=T, want_mode=True, **kw)
    return {tag + "negll": nll, tag + "newton_it": info["newton_it"], tag + "cg_it": info["cg_it"], tag + "log_det": info["log_det"],
            tag + "lanczos_it": info["lanczos_it"], tag + "mll_no_det": info["mll_no_det"], tag + "mode": info["mode"]}


def _grad(st, tag, **kw):
    nll, g, parts = st.laplace_eval_grad(COV, VAR, A, num_rand_vec=T, want_parts=True, **kw)
    return {tag + "negll": nll, tag + "grad": g, tag + "per_par": parts["per_par"], tag + "dlogdet_dmode": parts["dlogdet_dmode"],
            tag + "implicit_solve": parts["implicit_solve"], tag + "grad_F": st.laplace_grad_F()}


def case_conv(shim, pc, vif=False, lik="bernoulli_logit"):
    """default caps: every loop ends at its tolerance"""
    st = _state(shim, data(), pc, lik, vif)
    out = _eval(st, "")
    st.close()
    return out


def case_cap(shim, pc, vif=False):
    """every loop ends at its cap, from a zero mode and from the mode the capped run left behind"""
    st = _state(shim, data(), pc, vif=vif)
    out = _eval(st, "cold_", **CAP)
    out.update(_eval(st, "warm_", reset_mode=False, **CAP))
    st.close()
    return out


def case_grad(shim, pc, vif=False, lik="bernoulli_logit", **kw):
    st = _state(shim, data(), pc, lik, vif)
    out = _grad(st, "", **kw)
    if lik == "gamma":
        out["grad_aux"] = st.laplace_grad_aux()
    st.close()
    return out


def case_quad_forms(shim):
    """11 sparse rows at tc = 8: two blocks of right-hand sides, the second with three columns"""
    from gpboost_amd.basic import _lib, _shim_call
    d = data()
    st = _state(shim, d)
    _eval(st, "")
    out = {}
    for want_cov in (0, 1):
        q = np.empty(N_PRED * N_PRED if want_cov else N_PRED)
        it = C.c_int(-1)
        _shim_call(_lib().gpb_hip_vecchia_laplace_quad_forms(st.h, C.c_int(N_PRED), C.c_int(3), d["qf_cols"].ctypes.data_as(C.POINTER(C.c_int)),
                                                             d["qf_vals"].ctypes.data_as(C.POINTER(C.c_double)), C.c_int(1000), C.c_double(PRED_TOL), C.c_int(want_cov),
                                                             q.ctypes.data_as(C.POINTER(C.c_double)), C.byref(it)))
        out["cov" if want_cov else "var"] = q
        out["cov_it" if want_cov else "var_it"] = it.value
    st.close()
    return out


def quad_forms_refusal(shim):
    """-> the message of quad_forms with one iteration and a tolerance it cannot meet"""
    from gpboost_amd.basic import _lib
    d = data()
    st = _state(shim, d)
    _eval(st, "")
    q = np.empty(N_PRED)
    it = C.c_int(-1)
    rc = _lib().gpb_hip_vecchia_laplace_quad_forms(st.h, C.c_int(N_PRED), C.c_int(3), d["qf_cols"].ctypes.data_as(C.POINTER(C.c_int)),
                                                   d["qf_vals"].ctypes.data_as(C.POINTER(C.c_double)), C.c_int(1), C.c_double(1e-12), C.c_int(0),
                                                   q.ctypes.data_as(C.POINTER(C.c_double)), C.byref(it))
    msg = _lib().gpb_hip_get_last_error().decode("utf-8")
    st.close()
    return rc, msg


def case_mode_var(shim):
    """n = 40 at tc = 8: five full blocks of unit vectors"""
    from gpboost_amd.basic import _lib, _shim_call
    st = _state(shim, data(N_SMALL, seed=12))
    out = _eval(st, "")
    v = np.empty(N_SMALL)
    it = C.c_int(-1)
    _shim_call(_lib().gpb_hip_vecchia_laplace_mode_var(st.h, C.c_int(1000), C.c_double(PRED_TOL), v.ctypes.data_as(C.POINTER(C.c_double)), C.byref(it)))
    out["var"] = v
    out["var_it"] = it.value
    st.close()
    return out


def case_vif_predict(shim):
    """full-scale Vecchia, k = 10 > tc = 8: two column blocks of K^-1 W C (the second with two columns), 11 prediction points (two blocks, the second with three)"""
    from gpboost_amd.basic import _lib, _shim_call
    d = data()
    st = _state(shim, d, "fitc", vif=True)
    cp = np.asfortranarray(d["coords_pred"])
    out = {}
    for want_cov in (0, 1):
        _eval(st, "")                     # (a prediction hands the handle a new "response": the next one needs the factor again)
        mu = np.empty(N_PRED); var = np.empty(N_PRED); cov = np.empty((N_PRED, N_PRED))
        it = C.c_int(-1); dup = C.c_int(0)
        P = C.POINTER(C.c_double)
        _shim_call(_lib().gpb_hip_vecchia_vif_laplace_predict(st.h, C.c_int(N_PRED), cp.ctypes.data_as(P), C.c_int(M), C.c_int(COV), C.c_double(VAR), C.c_double(A), C.c_int(1000),
                                                              C.c_double(PRED_TOL), mu.ctypes.data_as(P), var.ctypes.data_as(P), cov.ctypes.data_as(P) if want_cov else None,
                                                              C.byref(dup), C.byref(it)))
        tag = "cov_" if want_cov else "var_"
        out[tag + "mean"] = mu
        out[tag + "var"] = var
        out[tag + "it"] = it.value
        if want_cov:
            out["cov"] = cov
    st.close()
    return out


CASES = {}
for _pc in ("vadu", "pivoted_cholesky", "fitc", "vecchia_response"):
    CASES["conv-" + _pc] = (case_conv, dict(pc=_pc))
    CASES["cap-" + _pc] = (case_cap, dict(pc=_pc))
for _pc in ("fitc", "vifdu", "none"):
    CASES["vif-conv-" + _pc] = (case_conv, dict(pc=_pc, vif=True))
for _pc in ("fitc", "vifdu"):                     # ("none" at 3 CG iterations per solve: the Newton iteration runs into its own cap of 1000 steps)
    CASES["vif-cap-" + _pc] = (case_cap, dict(pc=_pc, vif=True))
CASES["conv-gaussian_latent-vadu"] = (case_conv, dict(pc="vadu", lik="gaussian_latent"))      # one Newton step, one trial point
for _pc in ("vadu", "pivoted_cholesky", "fitc"):
    CASES["grad-" + _pc] = (case_grad, dict(pc=_pc))
for _pc in ("vadu", "pivoted_cholesky"):
    CASES["grad-cap-" + _pc] = (case_grad, dict(pc=_pc, **CAP))                                # the implicit solve ends at its cap
CASES["grad-gamma-vadu"] = (case_grad, dict(pc="vadu", lik="gamma"))                           # + the auxiliary parameter's gradient
CASES["vif-grad-fitc"] = (case_grad, dict(pc="fitc", vif=True))
CASES["quad-forms"] = (case_quad_forms, {})
CASES["mode-var-n40"] = (case_mode_var, {})
CASES["vif-predict"] = (case_vif_predict, {})


def run(name):
    from gpboost_amd import shim
    fn, kw = CASES[name]
    return {name + "/" + k: np.asarray(v) for k, v in fn(shim, **kw).items()}


def record(path):
    import time
    out = {}
    for name in CASES:
        t0 = time.perf_counter()
        out.update(run(name))
        print("%-28s %.2f s" % (name, time.perf_counter() - t0))
    np.savez(path, **out)
    print("recorded %d fields of %d cases -> %s" % (len(out), len(CASES), path))


def merge(paths, dst):
    runs = [dict(np.load(p)) for p in paths]
    out = {}
    for key, first in runs[0].items():
        out[key] = first
        if not all(np.array_equal(first, r[key]) for r in runs[1:]):
            assert not key.endswith("_it"), "iteration count %s differs between runs" % key
            stack = np.stack([r[key] for r in runs])
            out[key + "@spread"] = np.max(stack.max(axis=0) - stack.min(axis=0))
            print("NOT reproducible: %s spread %.3e" % (key, out[key + "@spread"]))
    np.savez_compressed(dst, **out)
    print("merged %d runs, %d fields, %d with a spread -> %s" % (len(runs), len(runs[0]), sum(k.endswith("@spread") for k in out), dst))


if __name__ == "__main__":
    if sys.argv[1] == "record":
        record(sys.argv[2])
    else:
        merge(sys.argv[3:], sys.argv[2])
