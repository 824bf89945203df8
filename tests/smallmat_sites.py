"""One device call through every site of gpb_hip.cpp / gpb_c_api.cpp whose k x k host algebra lives in gpboost_amd/csrc/gpb_smallmat.h, and what
tests/golden/smallmat_sites_parent.npz holds: the float64 results of collect() from a library built at the commit BEFORE the header existed, recorded twice
(scripts/record_smallmat_sites.py).  tests/test_zz_smallmat_sites_gpu.py runs collect() on the library under test and compares.

Shapes: n = 600, d = 2, m = 10 neighbours, 12 inducing points, preconditioner rank 8, 3 leaves, Matern 1.5 -- small enough for a few seconds in total, large
enough that every k x k matrix has rows that depend on all earlier ones.

    vif_gauss/{nll, grad, pred_mu, pred_var}      full-scale Vecchia, Gaussian likelihood: vif_terms_core (Sigma_m, its factor and inverse, the Woodbury matrix,
                                                  the traces) and the prediction's rows solve
    vif_fitc/{nll, grad, parts}                   full-scale Vecchia x Bernoulli-logit, "fitc" preconditioner, with gradient: ip_cov_factor twice, pc_refresh (fitc
                                                  branch), vif_lap_factor, spd_inverse_kk, vif_grad_prepare, chol_solve_kk
    lap_pivchol/{nll, grad, parts}                Vecchia x Bernoulli-logit, "pivoted_cholesky" preconditioner, with gradient: pc_refresh (the other branch).  The
                                                  full-scale model refuses this preconditioner (its words are asserted by the test), so the handle is a plain Vecchia one
    leaf/values                                   gpb_hip_vecchia_newton_leaf_values: the LP-stride Gram matrix, factor and solve
    fisher/cov_pars_std                           gpb_hip_exact_fisher_std_errors at n = 200 after two gradient steps
    coef/{cov_pars, coef_std}                     a fit with three covariates: profile_out_coef per evaluation, GPB_GetCoef's diagonal of the inverse
"""
import numpy as np

FIXTURE = "smallmat_sites_parent.npz"
N, D, M, K_IP, RANK, LEAVES, COV = 600, 2, 10, 12, 8, 3, 1
VAR, RHO = 0.8, 0.2
A = np.sqrt(3.0) / RHO
TIGHT = dict(cg_delta_conv=1e-12, delta_conv_mode_finding=1e-12)
VIF_PIVCHOL_REFUSAL = "full-scale Vecchia with a non-Gaussian likelihood: cg_preconditioner_type must be 'fitc' (the reference's default), 'vifdu' or 'none'"

# Where the two parent recordings differ (a device reduction whose order is not fixed), the bound is the parent's own spread, widened to no more than what the
# existing test of that path allows: relative to the largest magnitude of the quantity.
#   vif_gauss: tests/test_vif.py (1e-8); vif_fitc, lap_pivchol: tests/test_zz_vif_laplace_gpu.py, tests/test_zz_laplace_pivchol_gpu.py (1e-8);
#   leaf: tests/test_vecchia_gpu.py (1e-8); fisher: tests/test_exact_fisher.py (1e-8); coef: tests/test_coef.py (1e-6)
EXISTING_TOL = {"vif_gauss": 1e-8, "vif_fitc": 1e-8, "lap_pivchol": 1e-8, "leaf": 1e-8, "fisher": 1e-8, "coef": 1e-6}


def data():
    rng = np.random.default_rng(2024)
    coords = rng.uniform(size=(N, D))
    lat = 0.9 * np.sin(5 * coords[:, 0]) * np.cos(3 * coords[:, 1]) + 0.2
    y = lat + 0.4 * rng.standard_normal(N)
    y01 = (rng.uniform(size=N) < 1.0 / (1.0 + np.exp(-1.5 * lat))).astype(np.int32)
    ip = coords[rng.choice(N, size=K_IP, replace=False)].copy()
    ip_pc = coords[rng.choice(N, size=RANK, replace=False)].copy()
    leaf = rng.integers(0, LEAVES, size=N).astype(np.int32)
    X = np.column_stack([np.ones(N), coords[:, 0], rng.standard_normal(N)])
    cpred = rng.uniform(0.1, 0.9, size=(7, D))
    return dict(coords=coords, y=y, y01=y01, ip=ip, ip_pc=ip_pc, leaf=leaf, X=X, cpred=cpred)


def _laplace_state(shim, d, vif):
    st = shim.VecchiaState(d["coords"], M)
    st.find_neighbors()
    if vif:
        st.vif_set_inducing_points(d["ip"])
    st.laplace_set_likelihood("bernoulli_logit")
    st.laplace_set_labels(d["y01"])
    return st


def collect():
    """-> {name: float64 array} from the library that gpboost_amd loads"""
    import gpboost_amd as gpb
    from gpboost_amd import shim
    d = data()
    out = {}

    mdl = gpb.GPModel(gp_coords=d["coords"], cov_function="matern", cov_fct_shape=1.5, gp_approx="full_scale_vecchia", num_neighbors=M, num_ind_points=K_IP, seed=1)
    cp = np.array([0.2, VAR, RHO])
    nll, grad = mdl.neg_log_likelihood_and_gradient(cp, d["y"])
    pr = mdl.predict(y=d["y"], gp_coords_pred=d["cpred"], cov_pars=cp, predict_var=True, predict_response=True)
    out["vif_gauss/nll"], out["vif_gauss/grad"], out["vif_gauss/pred_mu"], out["vif_gauss/pred_var"] = np.array([nll]), grad, pr["mu"], pr["var"]

    st = _laplace_state(shim, d, vif=True)
    st.laplace_set_preconditioner("fitc", RANK)
    st.laplace_set_inducing_points(d["ip_pc"])
    nll, grad, parts = st.laplace_eval_grad(COV, VAR, A, want_parts=True, **TIGHT)
    out["vif_fitc/nll"], out["vif_fitc/grad"], out["vif_fitc/parts"] = np.array([nll]), grad, parts["per_par"].ravel()
    st.close()

    st = _laplace_state(shim, d, vif=False)
    st.laplace_set_preconditioner("pivoted_cholesky", RANK)
    nll, grad, parts = st.laplace_eval_grad(COV, VAR, A, want_parts=True, **TIGHT)
    out["lap_pivchol/nll"], out["lap_pivchol/grad"], out["lap_pivchol/parts"] = np.array([nll]), grad, parts["per_par"].ravel()
    st.close()

    st = shim.VecchiaState(d["coords"], M)
    st.find_neighbors()
    st.set_y(d["y"])
    st.factor(COV, VAR / 0.2, A)
    st.yaux()
    out["leaf/values"] = st.newton_leaf_values(d["leaf"], LEAVES)
    st.close()

    mdl = gpb.GPModel(gp_coords=d["coords"][:200], cov_function="matern", cov_fct_shape=1.5, gp_approx="none")
    mdl.fit(d["y"][:200], params=dict(optimizer_cov="gradient_descent", maxit=2, init_cov_pars=np.array([0.5, 0.8, 0.2])))
    out["fisher/cov_pars_std"] = mdl.get_cov_pars(std_err=True)

    mdl = gpb.GPModel(gp_coords=d["coords"], cov_function="matern", cov_fct_shape=1.5, gp_approx="vecchia", num_neighbors=M, seed=1)
    mdl.fit(d["y"], X=d["X"], params=dict(optimizer_cov="lbfgs", maxit=4, init_cov_pars=np.array([0.2, VAR, RHO])))
    out["coef/cov_pars"], out["coef/coef_std"] = mdl.get_cov_pars(), mdl.get_coef(std_err=True)
    return {k: np.ascontiguousarray(v, dtype=np.float64).reshape(-1).copy() for k, v in out.items()}


def vif_pivchol_refusal():
    """-> the message of a full-scale Vecchia x Bernoulli-logit evaluation asked for the "pivoted_cholesky" preconditioner"""
    import gpboost_amd as gpb
    from gpboost_amd import shim
    st = _laplace_state(shim, data(), vif=True)
    st.laplace_set_preconditioner("pivoted_cholesky", RANK)
    try:
        st.laplace_eval_grad(COV, VAR, A, **TIGHT)
    except gpb.GPBoostError as e:
        return str(e)
    finally:
        st.close()
    return ""
