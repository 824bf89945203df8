"""One device call through every entry point of the GRADIENT half of gpboost_amd/csrc/gpb_laplace.inc, and what tests/golden/laplace_grad_sites_parent.npz holds: the
float64 results of collect() and the messages of refusals() from a library built at the commit BEFORE that half was cut into stages, recorded twice
(scripts/record_laplace_grad_sites.py).  tests/test_zz_laplace_grad_sites_gpu.py runs both on the library under test and compares.

Shapes: n = 600, m = 10 neighbours, Matern 1.5, 12 inducing points, preconditioner rank 8, 10 probes (not a multiple of the chunk width 4: the padded last chunk is
exercised), the tight thresholds of smallmat_sites.TIGHT.  Every case runs at d = 2 and at d = 3 (the d3 flag of the derivative kernel's launch); <d> below is d2 / d3.

    <d>/vadu/{g, parts8, vecs2n, gradF}            Vecchia x Bernoulli-logit, laplace_eval_grad(want_parts) then laplace_grad_F: laplace_grad_current's vadu assembly
    <d>/pivoted_cholesky/{...}                     the same with the (W^-1 + Sigma) form: W^-1 P^-1 Z, Sigma U / Sigma P^-1 Z, no control variate
    <d>/fitc/{...}                                 the same with the fitc preconditioner
    <d>/vif_fitc/{...}                             full-scale Vecchia x Bernoulli-logit with fitc: vif_grad_prepare, the block and Q4 sums, vif_grad_assemble
    <d>/dup/{g, gradF}                             300 locations carrying 600 data through laplace_set_data_map, vadu: laplace_grad_F's data-map branch
    <d>/aux_gamma_vadu/{g, aux}                    laplace_grad_aux, information depends on the mode (no Fisher-Laplace trace)
    <d>/aux_t_vadu/{g, aux}                        t, two parameters, the vadu branch of the Fisher-Laplace trace
    <d>/aux_t_pivoted_cholesky/{g, aux}            t, the preconditioner branch (control variate centred with the samples' mean)
    <d>/aux_lognormal_vif_fitc/{g, aux}            lognormal on a full-scale Vecchia handle: the branch centred with the deterministic trace
    <d>/fisher/cov_pars_std                        Gaussian Vecchia model, get_cov_pars(std_err=True) after two L-BFGS steps: gpb_hip_vecchia_fisher_std_errors

refusals() -> the messages, as strings: "no_kept_state" (gradient on a handle that was never evaluated), "aux_before_grad", "gradF_before_grad" (after an evaluation
that kept its state but before the gradient), "vecchia_response", "vif_vifdu".
"""
import ctypes as C

import numpy as np

from tests.smallmat_sites import TIGHT

FIXTURE = "laplace_grad_sites_parent.npz"
N, M, K_IP, RANK, T, COV = 600, 10, 12, 8, 10, 1
N_LOC = 300
VAR, RHO = 0.8, 0.2
A = np.sqrt(3.0) / RHO
DIMS = (2, 3)
EVAL = dict(num_rand_vec=T, **TIGHT)

# Where the two parent recordings differ, the bound is the parent's own spread, widened to no more than what the existing test of that path allows, relative to the
# largest magnitude of the quantity:
#   vadu, dup: tests/test_z_laplace_grad_gpu.py (tight thresholds, 1e-8); pivoted_cholesky, fitc: tests/test_zz_laplace_pivchol_gpu.py (1e-8);
#   vif_fitc, aux_lognormal_vif_fitc: tests/test_zz_vif_laplace_gpu.py (1e-8); aux_gamma_vadu: tests/test_zz_laplace_aux_gpu.py (1e-8);
#   aux_t_*: tests/test_zz_laplace_t_gpu.py (1e-8); fisher: tests/test_optim.py (1e-7, against the oracle at the same parameters)
EXISTING_TOL = {"vadu": 1e-8, "dup": 1e-8, "pivoted_cholesky": 1e-8, "fitc": 1e-8, "vif_fitc": 1e-8, "aux_lognormal_vif_fitc": 1e-8, "aux_gamma_vadu": 1e-8,
                "aux_t_vadu": 1e-8, "aux_t_pivoted_cholesky": 1e-8, "fisher": 1e-7}

_FULL = ("g", "parts8", "vecs2n", "gradF")
CASES = [("vadu", _FULL), ("pivoted_cholesky", _FULL), ("fitc", _FULL), ("vif_fitc", _FULL), ("dup", ("g", "gradF")), ("aux_gamma_vadu", ("g", "aux")),
         ("aux_t_vadu", ("g", "aux")), ("aux_t_pivoted_cholesky", ("g", "aux")), ("aux_lognormal_vif_fitc", ("g", "aux")), ("fisher", ("cov_pars_std",))]
NAMES = ["d%d/%s/%s" % (d, case, q) for d in DIMS for case, qs in CASES for q in qs]
REFUSALS = ["no_kept_state", "aux_before_grad", "gradF_before_grad", "vecchia_response", "vif_vifdu"]


def data(d):
    rng = np.random.default_rng(2025 + d)
    coords = rng.uniform(size=(N, d))
    lat = 0.9 * np.sin(5 * coords[:, 0]) * np.cos(3 * coords[:, -1]) + 0.2
    y = lat + 0.4 * rng.standard_normal(N)
    y01 = (rng.uniform(size=N) < 1.0 / (1.0 + np.exp(-1.5 * lat))).astype(np.int32)
    ip = coords[rng.choice(N, size=K_IP, replace=False)].copy()
    ip_pc = coords[rng.choice(N, size=RANK, replace=False)].copy()
    return dict(coords=coords, y=y, ypos=np.exp(y), y01=y01, ip=ip, ip_pc=ip_pc)


def _state(shim, dat, lik="bernoulli_logit", pc="vadu", vif=False, aux=None, coords=None):
    st = shim.VecchiaState(dat["coords"] if coords is None else coords, M)
    st.find_neighbors()
    if vif:
        st.vif_set_inducing_points(dat["ip"])
    st.laplace_set_likelihood(lik)
    if lik == "bernoulli_logit":
        st.laplace_set_labels(dat["y01"])
    else:
        st.laplace_set_response_real(dat["y"] if lik == "t" else dat["ypos"])
    if aux is not None:
        st.laplace_set_aux(aux)
    st.laplace_set_preconditioner(pc, RANK)
    if pc == "fitc":
        st.laplace_set_inducing_points(dat["ip_pc"])
    return st


def _grad_current(shim, st):
    """gpb_hip_vecchia_laplace_grad_current alone, at whatever state the handle is in"""
    g = np.empty(2)
    shim._shim_call(shim._lib().gpb_hip_vecchia_laplace_grad_current(st.h, C.c_int(1000), C.c_double(1e-12), shim._p(g), None, None))
    return g


def collect():
    """-> {name: float64 array} from the library that gpboost_amd loads"""
    import gpboost_amd as gpb
    from gpboost_amd import shim
    out = {}
    for d in DIMS:
        dat, pre = data(d), "d%d/" % d
        for case, pc, vif in (("vadu", "vadu", False), ("pivoted_cholesky", "pivoted_cholesky", False), ("fitc", "fitc", False), ("vif_fitc", "fitc", True)):
            st = _state(shim, dat, pc=pc, vif=vif)
            nll, g, parts = st.laplace_eval_grad(COV, VAR, A, want_parts=True, **EVAL)
            out[pre + case + "/g"], out[pre + case + "/parts8"] = g, parts["per_par"].ravel()
            out[pre + case + "/vecs2n"] = np.concatenate([parts["dlogdet_dmode"], parts["implicit_solve"]])
            out[pre + case + "/gradF"] = st.laplace_grad_F()
            st.close()

        st = shim.VecchiaState(dat["coords"][:N_LOC], M)
        st.find_neighbors()
        st.laplace_set_likelihood("bernoulli_logit")
        st.laplace_set_data_map(np.arange(0, N + 1, N // N_LOC))
        st.laplace_set_labels(dat["y01"])
        nll, g = st.laplace_eval_grad(COV, VAR, A, **EVAL)
        out[pre + "dup/g"], out[pre + "dup/gradF"] = g, st.laplace_grad_F()
        st.close()

        for case, lik, pc, vif, aux in (("aux_gamma_vadu", "gamma", "vadu", False, 2.0), ("aux_t_vadu", "t", "vadu", False, (0.7, 4.0)),
                                        ("aux_t_pivoted_cholesky", "t", "pivoted_cholesky", False, (0.7, 4.0)),
                                        ("aux_lognormal_vif_fitc", "lognormal", "fitc", True, 0.5)):
            st = _state(shim, dat, lik=lik, pc=pc, vif=vif, aux=aux)
            nll, g = st.laplace_eval_grad(COV, VAR, A, **EVAL)
            out[pre + case + "/g"], out[pre + case + "/aux"] = g, st.laplace_grad_aux()
            st.close()

        mdl = gpb.GPModel(gp_coords=dat["coords"], cov_function="matern", cov_fct_shape=1.5, gp_approx="vecchia", num_neighbors=M, seed=1)
        mdl.fit(dat["y"], params=dict(optimizer_cov="lbfgs", maxit=2, init_cov_pars=np.array([0.2, VAR, RHO]), num_rand_vec_trace=T))
        out[pre + "fisher/cov_pars_std"] = np.asarray(mdl.get_cov_pars(std_err=True))[3:]
    return {k: np.ascontiguousarray(v, dtype=np.float64).reshape(-1).copy() for k, v in out.items()}


def refusals():
    """-> {name: message} of the refusals of the gradient's entry points ("" where a call that must refuse went through)"""
    import gpboost_amd as gpb
    from gpboost_amd import shim
    dat = data(2)
    out = {}

    def message(fn):
        try:
            fn()
        except gpb.GPBoostError as e:
            return str(e)
        return ""

    st = _state(shim, dat)
    out["no_kept_state"] = message(lambda: _grad_current(shim, st))
    o = np.empty(9)
    shim._shim_call(shim._lib().gpb_hip_vecchia_laplace_eval(st.h, C.c_int(COV), C.c_double(VAR), C.c_double(A), C.c_int(T), C.c_int(1), C.c_int(1000), C.c_int(1000),
                                                             C.c_double(1e-12), C.c_double(1e-12), C.c_int(1), C.c_int(1), shim._p(o), None))
    out["gradF_before_grad"] = message(st.laplace_grad_F)
    st.close()
    st = _state(shim, dat, lik="gamma", aux=2.0)
    shim._shim_call(shim._lib().gpb_hip_vecchia_laplace_eval(st.h, C.c_int(COV), C.c_double(VAR), C.c_double(A), C.c_int(T), C.c_int(1), C.c_int(1000), C.c_int(1000),
                                                             C.c_double(1e-12), C.c_double(1e-12), C.c_int(1), C.c_int(1), shim._p(o), None))
    out["aux_before_grad"] = message(st.laplace_grad_aux)
    st.close()
    st = _state(shim, dat, pc="vecchia_response")
    out["vecchia_response"] = message(lambda: st.laplace_eval_grad(COV, VAR, A, **EVAL))
    st.close()
    st = _state(shim, dat, pc="vifdu", vif=True)
    out["vif_vifdu"] = message(lambda: st.laplace_eval_grad(COV, VAR, A, **EVAL))
    st.close()
    return out
