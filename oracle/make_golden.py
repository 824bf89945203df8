"""Generates tests/golden/*.npz by running the UNMODIFIED reference (oracle/_ref, built by
oracle/Makefile.ref from /root/reference) through oracle/ref_driver.cpp.

    python oracle/make_golden.py

The fixtures are small (inputs are regenerated from seeds by tests/cases.py; only outputs are stored)
and are what the oracle (gpb_oracle.c) and the HIP path are pinned against on machines where
/root/reference does not exist.  TEST INFRASTRUCTURE ONLY.
"""
import os
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
from oracle import refdrv          # noqa: E402
from tests import cases            # noqa: E402


def main():
    if not refdrv.available():
        raise SystemExit("oracle/_ref is not built: run `make -C oracle ref` where /root/reference exists")
    out_dir = os.path.join(ROOT, "tests", "golden")
    os.makedirs(out_dir, exist_ok=True)
    only = [a for a in sys.argv[2:]] if len(sys.argv) > 2 and sys.argv[1] == "cases" else None      # `cases <name> ...`: only these fixtures
    for name, c in cases.GOLDEN_CASES.items():
        if only is not None and name not in only:
            continue
        coords, y = cases.make_data(c)
        mdl = refdrv.RefModel(coords, c["cov_function"], c["shape"], c["m"], c["ordering"], c["seed"])
        perm = mdl.perm()
        nn = mdl.neighbors()
        res = {"perm": perm.astype(np.int32), "nn": nn.astype(np.int32)}
        for k, cp in enumerate(c["cov_pars"]):
            nll, g, pt = mdl.nll_grad(y, np.asarray(cp, dtype=np.float64))
            A, D, ya = mdl.factor()
            res["nll_%d" % k] = np.float64(nll)
            res["grad_%d" % k] = g
            res["pars_trans_%d" % k] = pt
            res["D_%d" % k] = D
            res["yaux_%d" % k] = ya
            if k == 0 and name in cases.LEAF_CASES:      # NewtonUpdateLeafValues at the first parameter set, y = "F - y"
                leaf, L = cases.make_leaf_index(name, mdl.n)
                res["leaf_values_0"] = mdl.newton_leaf_values(leaf, L, cp[0])
            if mdl.n <= 500:
                res["A_%d" % k] = A
            else:   # keep fixtures small: a strided sample of rows
                res["A_rows_%d" % k] = np.arange(0, mdl.n, max(1, mdl.n // 200))
                res["A_%d" % k] = A[res["A_rows_%d" % k]]
        np.savez_compressed(os.path.join(out_dir, name + ".npz"), **res)
        print("wrote", name, "n=%d m=%d" % (mdl.n, mdl.m), "nll0=%.10f" % res["nll_0"])
    if only is not None:
        return
    hist_fixture(out_dir)
    laplace_fixture(out_dir)
    cluster_fixture(out_dir)
    split_fixture(out_dir)
    tree_fixture(out_dir)


def laplace_fixture(out_dir):
    """Reference GPB_EvalNegLogLikelihood for likelihood = 'bernoulli_logit' / 'bernoulli_probit', gp_approx = 'vecchia' (iterative, vadu)."""
    from oracle import orc
    res = {}
    for name, c in cases.LAPLACE_CASES.items():
        coords, y = cases.make_binary_data(c)
        for lik, tag in (("bernoulli_logit", ""), ("bernoulli_probit", "probit_")):
            mdl = refdrv.RefCAPIModel(coords, c["cov_function"], c["shape"], c["m"], c["ordering"], c["seed"], threads=8, likelihood=lik)
            for k, cp in enumerate(c["cov_pars"]):
                key = "%s_%snegll_%d" % (name, tag, k)
                res[key] = np.float64(mdl.neg_log_likelihood(np.asarray(cp, dtype=np.float64), y))
                print("laplace", lik, name, cp, "negll = %.12f" % res[key])
            # with fixed effects (the offset the GPBoost algorithm passes for non-Gaussian data), first parameter set
            key = "%s_fe_%snegll_0" % (name, tag)
            res[key] = np.float64(mdl.neg_log_likelihood(np.asarray(c["cov_pars"][0], dtype=np.float64), y, cases.laplace_fixed_effects(coords)))
            print("laplace", lik, name, "fixed effects negll = %.12f" % res[key])
        # Poisson counts on the same coordinates
        coords, yc = cases.make_count_data(c)
        mdl = refdrv.RefCAPIModel(coords, c["cov_function"], c["shape"], c["m"], c["ordering"], c["seed"], threads=8, likelihood="poisson")
        for k, cp in enumerate(c["cov_pars"]):
            key = "%s_poisson_negll_%d" % (name, k)
            res[key] = np.float64(mdl.neg_log_likelihood(np.asarray(cp, dtype=np.float64), yc))
            print("laplace poisson", name, cp, "negll = %.12f" % res[key])
        key = "%s_fe_poisson_negll_0" % name
        res[key] = np.float64(mdl.neg_log_likelihood(np.asarray(c["cov_pars"][0], dtype=np.float64), yc, cases.laplace_fixed_effects(coords)))
        print("laplace poisson", name, "fixed effects negll = %.12f" % res[key])
    # the R suite's probit fixture through the Vecchia approximation conditioning on all predecessors, iterative methods
    coords, y = orc.r_fixture_probit()
    mdl = refdrv.RefCAPIModel(coords, "exponential", 0.5, 99, "none", 0, threads=8, likelihood="bernoulli_probit")
    res["r_probit_m99_negll"] = np.float64(mdl.neg_log_likelihood(np.array([1.0, 0.2]), y))
    print("laplace r probit fixture (exact-GP golden 67.18342059): %.10f" % res["r_probit_m99_negll"])
    np.savez_compressed(os.path.join(out_dir, "laplace_ref.npz"), **res)


def laplace_grad_fixture(out_dir):
    """Gradients of the reference's approximate negative marginal log-likelihood wrt (log sigma1^2, log a) -- the pin of orc_vecchia_laplace_grad and of
    the device gradient.  Three sets per case and likelihood:
      *_grad_direct / *_negll_direct   the reference's OWN gradient routine (CalcGradPars -> CalcGradNegMargLikelihoodLaplaceApproxVecchia,
                                       likelihoods.h:6521-6700) called through oracle/ref_driver.cpp: refdrv_laplace_nll_grad with cg_delta_conv = 1e-8 and
                                       delta_conv_mode_finding = 1e-13: no stopping-rule noise left (1e-10 thresholds move it by < 1.1e-9) -> the 1e-8 pin;
      *_grad_tight                     read off one gradient-descent step of the reference's optimiser, cg_delta_conv = 1e-6 (round 3's pin; kept);
      *_grad                           the same at the reference's DEFAULT thresholds (1e-2 / 1e-8): the looser, second assertion."""
    res = {}
    for name, c in cases.LAPLACE_CASES.items():
        for lik in ("bernoulli_logit", "bernoulli_probit", "poisson"):
            coords, y = cases.make_count_data(c) if lik == "poisson" else cases.make_binary_data(c)
            cp = np.asarray(c["cov_pars"][0], dtype=np.float64)
            nll, gd, _ = refdrv.ref_laplace_nll_grad(coords, y, cp, lik, None, c["cov_function"], c["shape"], c["m"], c["ordering"], c["seed"],
                                                     cg_delta_conv=cases.LAPLACE_TIGHT["cg_delta_conv"], delta_conv_mode_finding=cases.LAPLACE_TIGHT["delta_conv_mode_finding"])
            res["%s_%s_grad_direct" % (name, lik)] = gd
            res["%s_%s_negll_direct" % (name, lik)] = np.float64(nll)
            print("laplace grad (CalcGradPars, cg 1e-8 / mode 1e-13)", name, lik, gd, "%.12f" % nll, flush=True)
            # the same with fixed effects (the offset of the GPBoost algorithm)
            fe = cases.laplace_fixed_effects(coords)
            nllf, gf, _ = refdrv.ref_laplace_nll_grad(coords, y, cp, lik, fe, c["cov_function"], c["shape"], c["m"], c["ordering"], c["seed"],
                                                      cg_delta_conv=cases.LAPLACE_TIGHT["cg_delta_conv"], delta_conv_mode_finding=cases.LAPLACE_TIGHT["delta_conv_mode_finding"])
            res["%s_%s_fe_grad_direct" % (name, lik)] = gf
            res["%s_%s_fe_negll_direct" % (name, lik)] = np.float64(nllf)
            g = refdrv.ref_laplace_gradient(coords, y, cp, lik, c["cov_function"], c["shape"], c["m"], c["ordering"], c["seed"])
            res["%s_%s_grad" % (name, lik)] = g
            print("laplace grad (optimiser step, default thresholds)", name, lik, g, flush=True)
            gt = refdrv.ref_laplace_gradient(coords, y, cp, lik, c["cov_function"], c["shape"], c["m"], c["ordering"], c["seed"], cg_delta_conv=1e-6)
            res["%s_%s_grad_tight" % (name, lik)] = gt
            print("laplace grad (optimiser step, cg_delta_conv = 1e-6)", name, lik, gt, flush=True)
    np.savez_compressed(os.path.join(out_dir, "laplace_grad_ref.npz"), **res)


def laplace_pivchol_fixture(out_dir, only=()):
    """cg_preconditioner_type = "pivoted_cholesky" (the (W^-1 + Sigma) form of the Vecchia-Laplace solves, P = W^-1 + L_k L_k^T; CG_utils.cpp:231-499,
    likelihoods.h:16277-16296, :16389-16465, :16554-16611, :16716-16736) on cases.LAPLACE_PIVCHOL_CASES, from the reference's own routines:
      *_negll_direct, *_grad_direct   value and gradient wrt (log sigma1^2, log a[, log aux]) from CalcGradPars at cases.LAPLACE_TIGHT (+ *_fe_* with the offset)
      *_negll_default                  GPB_EvalNegLogLikelihood at the reference's default thresholds
      *_gradF                          the boosting gradient d(-mll) / dF at cases.LAPLACE_TIGHT (data order)
      *_fit_*                          one lbfgs fit at cases.LAPLACE_TIGHT: estimates, iterations, final value"""
    res = {}
    path = os.path.join(out_dir, "laplace_pivchol_ref.npz")
    if only and os.path.exists(path):        # `laplace_pivchol <case> ...`: only these cases are (re)generated
        res = dict(np.load(path))
    tight = dict(cg_delta_conv=cases.LAPLACE_TIGHT["cg_delta_conv"], delta_conv_mode_finding=cases.LAPLACE_TIGHT["delta_conv_mode_finding"])
    for name, pc in cases.LAPLACE_PIVCHOL_CASES.items():
        if only and name not in only:
            continue
        c = cases.LAPLACE_CASES[pc["model"]]
        coords, y = cases.make_pivchol_data(pc)
        cp = np.asarray(c["cov_pars"][0], dtype=np.float64)
        rank = -999 if pc["rank"] is None else int(pc["rank"])
        aux = pc.get("aux")
        pcargs = dict(cg_preconditioner_type=pc.get("pc", "pivoted_cholesky"), piv_chol_rank=rank)
        for fe_key, fe in (("", None), ("_fe", cases.laplace_fixed_effects(coords))):
            nll, g, _ = refdrv.ref_laplace_nll_grad(coords, y, cp, pc["lik"], fe, c["cov_function"], c["shape"], c["m"], c["ordering"], c["seed"],
                                                    aux_pars=aux, estimate_aux=aux is not None, **tight, **pcargs)
            res[name + fe_key + "_negll_direct"] = np.float64(nll); res[name + fe_key + "_grad_direct"] = g
            print("pivoted_cholesky (CalcGradPars, tight)", name, fe_key, "%.12f" % nll, g, flush=True)
        mdl = refdrv.RefCAPIModel(coords, c["cov_function"], c["shape"], c["m"], c["ordering"], c["seed"], threads=8, likelihood=pc["lik"])
        mdl.set_optim_config(init_aux_pars=aux, estimate_aux_pars=False, **pcargs)
        res[name + "_negll_default"] = np.float64(mdl.neg_log_likelihood(cp, y))
        print("pivoted_cholesky (default thresholds)", name, "%.12f" % res[name + "_negll_default"], flush=True)
        if aux is None:
            res[name + "_gradF"] = refdrv.ref_laplace_grad_F(coords, y, cp, pc["lik"], None, c["cov_function"], c["shape"], c["m"], c["ordering"], c["seed"],
                                                             **tight, **pcargs)
        # one lbfgs fit (the reference's default optimiser for these models) at the tight thresholds
        mdl = refdrv.RefCAPIModel(coords, c["cov_function"], c["shape"], c["m"], c["ordering"], c["seed"], threads=8, likelihood=pc["lik"])
        mdl.set_optim_config(init_aux_pars=None, estimate_aux_pars=aux is not None, **tight, **pcargs)
        mdl.optim_cov_par(y)
        res[name + "_fit_cov_pars"] = mdl.get_cov_par(2)
        res[name + "_fit_num_it"] = np.int64(mdl.get_num_it())
        res[name + "_fit_negll"] = np.float64(mdl.current_neg_log_likelihood())
        res[name + "_fit_init_cov_pars"] = mdl.get_init_cov_par()
        if aux is not None:
            res[name + "_fit_aux"] = mdl.get_aux_pars(1); res[name + "_fit_init_aux"] = mdl.get_init_aux_pars(1)
        print("pivoted_cholesky fit", name, res[name + "_fit_cov_pars"], res.get(name + "_fit_aux"), int(res[name + "_fit_num_it"]), "%.10f" % res[name + "_fit_negll"], flush=True)
    np.savez_compressed(os.path.join(out_dir, "laplace_pivchol_ref.npz"), **res)


def laplace_pivchol_probes_fixture(out_dir):
    """cases.LAPLACE_PIVCHOL_PROBE_CASES: the low-rank preconditioners with num_rand_vec_trace > 50 -- value and gradient from the reference's own CalcGradPars at
    cases.LAPLACE_TIGHT: <key>_negll_direct, <key>_grad_direct."""
    res = {}
    tight = dict(cg_delta_conv=cases.LAPLACE_TIGHT["cg_delta_conv"], delta_conv_mode_finding=cases.LAPLACE_TIGHT["delta_conv_mode_finding"])
    for key, (name, t) in cases.LAPLACE_PIVCHOL_PROBE_CASES.items():
        pc = cases.LAPLACE_PIVCHOL_CASES[name]
        c = cases.LAPLACE_CASES[pc["model"]]
        coords, y = cases.make_pivchol_data(pc)
        cp = np.asarray(c["cov_pars"][0], dtype=np.float64)
        nll, g, _ = refdrv.ref_laplace_nll_grad(coords, y, cp, pc["lik"], None, c["cov_function"], c["shape"], c["m"], c["ordering"], c["seed"], **tight,
                                                cg_preconditioner_type=pc.get("pc", "pivoted_cholesky"), piv_chol_rank=-999 if pc["rank"] is None else int(pc["rank"]),
                                                num_rand_vec_trace=t)
        res[key + "_negll_direct"] = np.float64(nll); res[key + "_grad_direct"] = g
        print("low-rank preconditioner, %d probes (CalcGradPars, tight)" % t, key, "%.12f" % nll, g, flush=True)
    np.savez_compressed(os.path.join(out_dir, "laplace_pivchol_probes_ref.npz"), **res)


def laplace_aux_fixture(out_dir, only=()):
    """gamma and negative_binomial Vecchia-Laplace models (auxiliary shape parameter estimated with the covariance parameters): the reference's own
      *_negll_0                      GPB_EvalNegLogLikelihood at (cov_pars, aux) with the default thresholds
      *_negll_direct, *_grad_direct  value and gradient wrt (log sigma1^2, log a, log aux) from the reference's CalcGradPars (refdrv_laplace_nll_grad) at
                                     cases.LAPLACE_TIGHT; *_fe_*: with fixed effects
      *_fit_*                        GPB_OptimCovPar (lbfgs, estimate_aux_pars = true, aux initialised by FindInitialAuxPars): cov_pars, aux, init aux,
                                     iterations, negll -- at the default thresholds and (*_fit_tight_*) at cases.LAPLACE_TIGHT
      *_fitfix_*                     the same with the auxiliary parameter held at cases' aux (estimate_aux_pars = false)"""
    res = {}
    path = os.path.join(out_dir, "laplace_aux_ref.npz")
    if only and os.path.exists(path):        # `laplace_aux <case> ...`: only these cases are (re)generated, the others are kept as they are
        res = dict(np.load(path))
    for name, ac in cases.LAPLACE_AUX_CASES.items():
        if only and name not in only:
            continue
        c = cases.LAPLACE_CASES[ac["model"]]
        coords, y = cases.make_aux_data(ac)
        lik, aux = ac["lik"], ac["aux"]
        cp = np.asarray(c["cov_pars"][0], dtype=np.float64)
        args = (c["cov_function"], c["shape"], c["m"], c["ordering"], c["seed"])
        mdl = refdrv.RefCAPIModel(coords, *args, threads=8, likelihood=lik)
        mdl.set_optim_config(init_aux_pars=aux)
        res[name + "_negll_0"] = np.float64(mdl.neg_log_likelihood(cp, y))
        for fe_key, fe in (("", None), ("_fe", cases.aux_fixed_effects(ac, coords))):
            nll, g, _ = refdrv.ref_laplace_nll_grad(coords, y, cp, lik, fe, *args, aux_pars=aux, estimate_aux=True, **cases.LAPLACE_TIGHT)
            res[name + fe_key + "_negll_direct"] = np.float64(nll)
            res[name + fe_key + "_grad_direct"] = g
            print("laplace aux", name, fe_key, "negll %.10f" % nll, "grad", g, flush=True)
        for key, cfg in (("_fit", {}), ("_fit_tight", dict(cases.LAPLACE_TIGHT))):
            m2 = refdrv.RefCAPIModel(coords, *args, threads=8, likelihood=lik)
            m2.set_optim_config(estimate_aux_pars=True, **cfg)
            m2.optim_cov_par(y)
            res[name + key + "_cov_pars"] = m2.get_cov_par(2)
            res[name + key + "_aux"] = m2.get_aux_pars(1)
            res[name + key + "_init_cov_pars"] = m2.get_init_cov_par()[:2].copy()
            res[name + key + "_init_aux"] = m2.get_init_aux_pars(1)
            res[name + key + "_num_it"] = np.int32(m2.get_num_it())
            res[name + key + "_negll"] = np.float64(m2.current_neg_log_likelihood())
            print("laplace aux fit", name, key, res[name + key + "_init_cov_pars"], res[name + key + "_init_aux"], "->", res[name + key + "_cov_pars"],
                  res[name + key + "_aux"], res[name + key + "_num_it"], res[name + key + "_negll"], flush=True)
        m3 = refdrv.RefCAPIModel(coords, *args, threads=8, likelihood=lik)
        m3.set_optim_config(init_aux_pars=aux, estimate_aux_pars=False)
        m3.optim_cov_par(y)
        res[name + "_fitfix_cov_pars"] = m3.get_cov_par(2)
        res[name + "_fitfix_aux"] = m3.get_aux_pars(1)
        res[name + "_fitfix_num_it"] = np.int32(m3.get_num_it())
        res[name + "_fitfix_negll"] = np.float64(m3.current_neg_log_likelihood())
        print("laplace aux fit (aux fixed)", name, res[name + "_fitfix_cov_pars"], res[name + "_fitfix_aux"], res[name + "_fitfix_num_it"], res[name + "_fitfix_negll"], flush=True)
        # predictions at (cov_pars, aux): latent mean / variance and the response's (PredictResponse, likelihoods.h:9715-9728, :9783-9793); Cholesky-based =
        # the exact values the iterative methods estimate (as tests/golden/laplace_predvar_ref.npz)
        cpred = np.random.default_rng(79).uniform(size=(40, c["d"]))
        res[name + "_coords_pred"] = cpred
        m4 = refdrv.RefCAPIModel(coords, *args, threads=8, likelihood=lik, matrix_inversion_method="cholesky")
        m4.set_optim_config(init_aux_pars=aux, **cases.LAPLACE_PRED_REF)
        mu, var = m4.predict(cpred, predict_var=True, predict_response=False, y=y, cov_pars=cp)
        rmu, rvar = m4.predict(cpred, predict_var=True, predict_response=True, y=y, cov_pars=cp)
        res[name + "_latent_mu"] = mu; res[name + "_latent_var"] = var; res[name + "_resp_mu"] = rmu; res[name + "_resp_var"] = rvar
        print("laplace aux predictions", name, mu[:2], var[:2], rmu[:2], rvar[:2], flush=True)
    np.savez_compressed(os.path.join(out_dir, "laplace_aux_ref.npz"), **res)


def laplace_pc_extra_fixture(out_dir):
    """cases.LAPLACE_PC_EXTRA_CASES (pivoted_cholesky / fitc together with sample weights / repeated locations) through the reference library's C API at cases.LAPLACE_TIGHT:
    *_negll (GPB_EvalNegLogLikelihood) and one lbfgs fit (*_fit_cov_pars / _aux / _num_it / _negll) -- tests/golden/laplace_pc_extra_ref.npz."""
    res = {}
    for name, ec in cases.LAPLACE_PC_EXTRA_CASES.items():
        kw, y, cp, aux = cases.pc_extra_model(ec)
        def model():
            m = refdrv.RefCAPIModel(kw["gp_coords"], kw["cov_function"], kw["cov_fct_shape"], kw["num_neighbors"], kw["vecchia_ordering"], kw["seed"], threads=8,
                                    likelihood=kw["likelihood"], weights=kw.get("weights"))
            return m
        m1 = model()
        m1.set_optim_config(init_aux_pars=aux, estimate_aux_pars=False, cg_preconditioner_type=ec["pc"], piv_chol_rank=ec["rank"], **cases.LAPLACE_TIGHT)
        res[name + "_negll"] = np.float64(m1.neg_log_likelihood(cp, y))
        m2 = model()
        m2.set_optim_config(estimate_aux_pars=aux is not None, cg_preconditioner_type=ec["pc"], piv_chol_rank=ec["rank"], **cases.LAPLACE_TIGHT)
        m2.optim_cov_par(y)
        res[name + "_fit_cov_pars"] = m2.get_cov_par(2); res[name + "_fit_num_it"] = np.int64(m2.get_num_it()); res[name + "_fit_negll"] = np.float64(m2.current_neg_log_likelihood())
        if aux is not None:
            res[name + "_fit_aux"] = m2.get_aux_pars(1)
        print("pc extra", name, "%.10f" % res[name + "_negll"], res[name + "_fit_cov_pars"], res.get(name + "_fit_aux"), int(res[name + "_fit_num_it"]), "%.8f" % res[name + "_fit_negll"], flush=True)
    np.savez_compressed(os.path.join(out_dir, "laplace_pc_extra_ref.npz"), **res)


def laplace_vresp_fixture(out_dir):
    """cg_preconditioner_type = "vecchia_response" (likelihoods.h:16315-16323, :16439-16450, :16471-16473; CG_utils.cpp:300-303, :410-416) by the unmodified reference's
    C API -- tests/golden/laplace_vresp_ref.npz.  Per cases.LAPLACE_VRESP_CASES entry: *_negll_tight / *_fe_negll_tight (GPB_EvalNegLogLikelihood at cases.LAPLACE_TIGHT,
    without / with fixed effects), *_negll_tight_1 (a second call of the same model at cases.LAPLACE_VRESP_SECOND_PARS), *_negll_default, and one
    Nelder-Mead fit (the reference refuses gradients with this preconditioner, likelihoods.h:6570-6572) of cases.LAPLACE_VRESP_NM: *_fit_cov_pars / _aux / _num_it / _negll.
    cases.LAPLACE_VRESP_EXTRA_CASES (sample weights, repeated locations): *_negll and the same fit."""
    res = {}
    nm = cases.LAPLACE_VRESP_NM
    for name, pc in cases.LAPLACE_VRESP_CASES.items():
        c = cases.LAPLACE_CASES[pc["model"]]
        coords, y = cases.make_pivchol_data(pc)
        cp = np.asarray(c["cov_pars"][0], dtype=np.float64)
        aux = pc.get("aux")
        args = (c["cov_function"], c["shape"], c["m"], c["ordering"], c["seed"])
        pcargs = dict(cg_preconditioner_type="vecchia_response")
        mdl = refdrv.RefCAPIModel(coords, *args, threads=8, likelihood=pc["lik"])
        mdl.set_optim_config(init_aux_pars=aux, estimate_aux_pars=False, **pcargs, **cases.LAPLACE_TIGHT)
        res[name + "_negll_tight"] = np.float64(mdl.neg_log_likelihood(cp, y))
        res[name + "_negll_tight_1"] = np.float64(mdl.neg_log_likelihood(np.asarray(cases.LAPLACE_VRESP_SECOND_PARS), y))
        mdl = refdrv.RefCAPIModel(coords, *args, threads=8, likelihood=pc["lik"])
        mdl.set_optim_config(init_aux_pars=aux, estimate_aux_pars=False, **pcargs, **cases.LAPLACE_TIGHT)
        res[name + "_fe_negll_tight"] = np.float64(mdl.neg_log_likelihood(cp, y, fixed_effects=cases.laplace_fixed_effects(coords)))
        mdl = refdrv.RefCAPIModel(coords, *args, threads=8, likelihood=pc["lik"])
        mdl.set_optim_config(init_aux_pars=aux, estimate_aux_pars=False, **pcargs)
        res[name + "_negll_default"] = np.float64(mdl.neg_log_likelihood(cp, y))
        mdl = refdrv.RefCAPIModel(coords, *args, threads=8, likelihood=pc["lik"])
        mdl.set_optim_config(estimate_aux_pars=aux is not None, optimizer_cov=nm["optimizer_cov"], max_iter=nm["maxit"], **pcargs, **cases.LAPLACE_TIGHT)
        mdl.optim_cov_par(y)
        res[name + "_fit_cov_pars"] = mdl.get_cov_par(2); res[name + "_fit_num_it"] = np.int64(mdl.get_num_it())
        res[name + "_fit_negll"] = np.float64(mdl.current_neg_log_likelihood())
        if aux is not None:
            res[name + "_fit_aux"] = mdl.get_aux_pars(1)
        print("vecchia_response", name, "%.12f %.12f fe %.12f default %.12f" % (res[name + "_negll_tight"], res[name + "_negll_tight_1"], res[name + "_fe_negll_tight"],
              res[name + "_negll_default"]), "fit", res[name + "_fit_cov_pars"], res.get(name + "_fit_aux"), int(res[name + "_fit_num_it"]), "%.10f" % res[name + "_fit_negll"], flush=True)
    for name, ec in cases.LAPLACE_VRESP_EXTRA_CASES.items():
        kw, y, cp, aux = cases.pc_extra_model(ec)
        def model():
            return refdrv.RefCAPIModel(kw["gp_coords"], kw["cov_function"], kw["cov_fct_shape"], kw["num_neighbors"], kw["vecchia_ordering"], kw["seed"], threads=8,
                                       likelihood=kw["likelihood"], weights=kw.get("weights"))
        m1 = model()
        m1.set_optim_config(init_aux_pars=aux, estimate_aux_pars=False, cg_preconditioner_type=ec["pc"], **cases.LAPLACE_TIGHT)
        res[name + "_negll"] = np.float64(m1.neg_log_likelihood(cp, y))
        m2 = model()
        m2.set_optim_config(estimate_aux_pars=aux is not None, cg_preconditioner_type=ec["pc"], optimizer_cov=nm["optimizer_cov"], max_iter=nm["maxit"], **cases.LAPLACE_TIGHT)
        m2.optim_cov_par(y)
        res[name + "_fit_cov_pars"] = m2.get_cov_par(2); res[name + "_fit_num_it"] = np.int64(m2.get_num_it()); res[name + "_fit_negll"] = np.float64(m2.current_neg_log_likelihood())
        print("vecchia_response extra", name, "%.10f" % res[name + "_negll"], res[name + "_fit_cov_pars"], int(res[name + "_fit_num_it"]), "%.8f" % res[name + "_fit_negll"], flush=True)
    np.savez_compressed(os.path.join(out_dir, "laplace_vresp_ref.npz"), **res)


def laplace_t_fixture(out_dir):
    """Student-t Vecchia-Laplace models (auxiliary parameters scale and df, both estimated; approximation_type fisher_laplace) by the unmodified reference --
    tests/golden/laplace_t_ref.npz, per cases.LAPLACE_T_CASES entry: *_negll_0 (default thresholds), *_negll_direct / *_grad_direct (CalcGradPars at cases.LAPLACE_TIGHT:
    gradient wrt (log sigma1^2, log a, log scale, log df); *_fe_*: with fixed effects), *_fit_* / *_fit_tight_* (lbfgs with both auxiliary parameters estimated), predictions."""
    res = {}
    only = sys.argv[2:]
    path = os.path.join(out_dir, "laplace_t_ref.npz")
    if only and os.path.isfile(path):          # `laplace_t <name> ...`: (re)generate only these cases
        res = dict(np.load(path))
    for name, tc in cases.LAPLACE_T_CASES.items():
        if only and name not in only:
            continue
        lik = tc.get("lik", "t")               # (lognormal: one auxiliary parameter, otherwise the same surface)
        naux = len(tc["aux"])
        c = cases.LAPLACE_CASES[tc["model"]]
        coords, y = cases.make_t_data(tc)
        aux = np.asarray(tc["aux"], dtype=np.float64)
        cp = np.asarray(c["cov_pars"][0], dtype=np.float64)
        args = (c["cov_function"], c["shape"], c["m"], c["ordering"], c["seed"])
        mdl = refdrv.RefCAPIModel(coords, *args, threads=8, likelihood=lik)
        mdl.set_optim_config(init_aux_pars=aux)
        res[name + "_negll_0"] = np.float64(mdl.neg_log_likelihood(cp, y))
        for fe_key, fe in (("", None), ("_fe", cases.laplace_fixed_effects(coords))):
            nll, g, _ = refdrv.ref_laplace_nll_grad(coords, y, cp, lik, fe, *args, aux_pars=aux, estimate_aux=True, **cases.LAPLACE_TIGHT)
            res[name + fe_key + "_negll_direct"] = np.float64(nll); res[name + fe_key + "_grad_direct"] = g
            print("laplace " + lik, name, fe_key, "negll %.10f" % nll, "grad", g, flush=True)
        for key, cfg in (("_fit", {}), ("_fit_tight", dict(cases.LAPLACE_TIGHT))):
            m2 = refdrv.RefCAPIModel(coords, *args, threads=8, likelihood=lik)
            m2.set_optim_config(estimate_aux_pars=True, **cfg)
            m2.optim_cov_par(y)
            res[name + key + "_cov_pars"] = m2.get_cov_par(2); res[name + key + "_aux"] = m2.get_aux_pars(naux)
            res[name + key + "_init_cov_pars"] = m2.get_init_cov_par()[:2].copy()
            res[name + key + "_num_it"] = np.int32(m2.get_num_it()); res[name + key + "_negll"] = np.float64(m2.current_neg_log_likelihood())
            print("laplace t fit", name, key, "->", res[name + key + "_cov_pars"], res[name + key + "_aux"], res[name + key + "_num_it"], res[name + key + "_negll"], flush=True)
        cpred = np.random.default_rng(79).uniform(size=(40, c["d"]))
        res[name + "_coords_pred"] = cpred
        m4 = refdrv.RefCAPIModel(coords, *args, threads=8, likelihood=lik, matrix_inversion_method="cholesky")
        m4.set_optim_config(init_aux_pars=aux, **cases.LAPLACE_PRED_REF)
        mu, var = m4.predict(cpred, predict_var=True, predict_response=False, y=y, cov_pars=cp)
        rmu, rvar = m4.predict(cpred, predict_var=True, predict_response=True, y=y, cov_pars=cp)
        res[name + "_latent_mu"] = mu; res[name + "_latent_var"] = var; res[name + "_resp_mu"] = rmu; res[name + "_resp_var"] = rvar
        print("laplace t predictions", name, mu[:2], var[:2], rmu[:2], rvar[:2], flush=True)
    np.savez_compressed(os.path.join(out_dir, "laplace_t_ref.npz"), **res)


def laplace_pred_refresh(out_dir):
    """Round 6: the PREDICTION entries (*_latent_mu / _var, *_resp_mu / _var) of laplace_aux_ref.npz, laplace_t_ref.npz and laplace_weights_ref.npz
    again, with the reference's Cholesky-based mode finding run to convergence (cases.LAPLACE_PRED_REF: delta_conv_mode_finding = 1e-16).  At 1e-13 -- what the files held --
    the reference's own mode is up to 1.2e-7 from the converged one (negbin_n1500: its Cholesky prediction at 1e-16 and its iterative one at 1e-15 / 1e-11 agree to 3e-13,
    both 1.2e-7 from the 1e-13 values), which is why the device's predictions could only be held to 1e-5 against them.  Everything else in the files is left as it is."""
    jobs = (("laplace_aux_ref.npz", cases.LAPLACE_AUX_CASES, lambda ac: cases.make_aux_data(ac) + (None,), lambda ac: ac["aux"]),
            ("laplace_t_ref.npz", cases.LAPLACE_T_CASES, lambda tc: cases.make_t_data(tc) + (None,), lambda tc: np.asarray(tc["aux"], dtype=np.float64)),
            ("laplace_weights_ref.npz", cases.LAPLACE_WEIGHT_CASES, lambda wc: cases.make_weight_data(wc), lambda wc: wc.get("aux")))
    for fname, table, make, aux_of in jobs:
        path = os.path.join(out_dir, fname)
        res = dict(np.load(path))
        for name, cs in table.items():
            c = cases.LAPLACE_CASES[cs["model"]]
            coords, y, w = make(cs)
            lik = cs.get("lik", "t")
            cp = np.asarray(c["cov_pars"][0], dtype=np.float64)
            args = (c["cov_function"], c["shape"], c["m"], c["ordering"], c["seed"])
            cpred = res[name + "_coords_pred"]
            has_resp = name + "_resp_mu" in res
            out = {}
            for key, cfg in (("ref", cases.LAPLACE_PRED_REF), ("tight", cases.LAPLACE_TIGHT)):
                # (a fresh model per prediction: a second prediction on one model continues from the first one's mode, i.e. is better converged than a first one)
                vals = []
                for resp in ((False, True) if has_resp else (False,)):
                    m4 = refdrv.RefCAPIModel(coords, *args, threads=8, likelihood=lik, matrix_inversion_method="cholesky", weights=w)
                    m4.set_optim_config(init_aux_pars=aux_of(cs), **cfg)
                    vals += list(m4.predict(cpred, predict_var=True, predict_response=resp, y=y, cov_pars=cp))
                out[key] = vals
            # *_pred_spread: by how much the reference's OWN predictions move between delta_conv_mode_finding = 1e-13 and 1e-16 (max abs, per quantity) -- its mode
            # finding stops on the rounding noise of the objective (CheckConvergenceModeFinding, likelihoods.h:16078-16128: a change below the threshold OR any decrease
            # ends it, and the Armijo test :3929-3966 rejects a last step whose gain is below that noise), so the mode is only defined to this spread
            spread = [float(np.abs(a - b).max()) for a, b in zip(out["ref"], out["tight"])]
            res[name + "_latent_mu"], res[name + "_latent_var"] = out["ref"][0], out["ref"][1]
            if has_resp:
                res[name + "_resp_mu"], res[name + "_resp_var"] = out["ref"][2], out["ref"][3]
            res[name + "_pred_spread"] = np.asarray(spread + [0.0] * (4 - len(spread)))
            print("prediction fixtures", fname, name, "reference's own spread (1e-13 vs 1e-16):", ["%.2e" % v for v in spread], flush=True)
        np.savez_compressed(path, **res)


def laplace_aux_se_fixture(out_dir):
    """Round 6: standard deviations of covariance AND auxiliary parameters of non-Gaussian models whose auxiliary parameters are estimated (GPB_GetCovPar / GPB_GetAuxPars with
    calc_std_dev = true -> CalcStdDevCovParAuxParsNonGaussian, re_model_template.h:11029-11117: joint numerical Hessian at step 1e-4) after an lbfgs fit at cases.LAPLACE_TIGHT,
    by the unmodified reference -- tests/golden/laplace_aux_se_ref.npz: <case>_cov_pars (values, standard deviations), <case>_aux (values, standard deviations), <case>_num_it."""
    res = {}
    jobs = [("gamma_n1500", cases.LAPLACE_AUX_CASES["gamma_n1500"], cases.make_aux_data, "gamma", 1, {}),
            ("t_n1500", cases.LAPLACE_T_CASES["t_n1500"], cases.make_t_data, "t", 2, {}),
            ("t_fix_df5_n1500", cases.LAPLACE_T_CASES["t_n1500"], cases.make_t_data, "t_fix_df", 2, dict(likelihood_additional_param=5.0))]
    for name, cs, make, lik, naux, extra in jobs:
        c = cases.LAPLACE_CASES[cs["model"]]
        coords, y = make(cs)
        args = (c["cov_function"], c["shape"], c["m"], c["ordering"], c["seed"])
        m2 = refdrv.RefCAPIModel(coords, *args, threads=8, likelihood=lik, **extra)
        m2.set_optim_config(estimate_aux_pars=True, **cases.LAPLACE_TIGHT)
        m2.optim_cov_par(y)
        res[name + "_num_it"] = np.int32(m2.get_num_it())
        res[name + "_cov_pars"] = m2.get_cov_par(2, std_dev=True)
        res[name + "_aux"] = m2.get_aux_pars(naux, std_dev=True)
        print("aux std devs", name, res[name + "_num_it"], res[name + "_cov_pars"], res[name + "_aux"], flush=True)
    # optimizer_cov = "nelder_mead" with the auxiliary parameter in the simplex (OptimLib nm.hpp over (log sigma1^2, log a, log shape), EvalLLforOptimLib): gamma_n1500 at cases.LAPLACE_TIGHT
    ac = cases.LAPLACE_AUX_CASES["gamma_n1500"]; c = cases.LAPLACE_CASES[ac["model"]]
    coords, y = cases.make_aux_data(ac)
    m3 = refdrv.RefCAPIModel(coords, c["cov_function"], c["shape"], c["m"], c["ordering"], c["seed"], threads=8, likelihood="gamma")
    m3.set_optim_config(estimate_aux_pars=True, optimizer_cov="nelder_mead", **cases.LAPLACE_TIGHT)
    m3.optim_cov_par(y)
    res["gamma_n1500_nm_cov_pars"] = m3.get_cov_par(2); res["gamma_n1500_nm_aux"] = m3.get_aux_pars(1)
    res["gamma_n1500_nm_num_it"] = np.int32(m3.get_num_it()); res["gamma_n1500_nm_negll"] = np.float64(m3.current_neg_log_likelihood())
    print("nelder_mead with the shape in the simplex", res["gamma_n1500_nm_cov_pars"], res["gamma_n1500_nm_aux"], res["gamma_n1500_nm_num_it"], "%.10f" % res["gamma_n1500_nm_negll"], flush=True)
    np.savez_compressed(os.path.join(out_dir, "laplace_aux_se_ref.npz"), **res)


def laplace_aux_gd_fixture(out_dir):
    """Round 6: optimizer_cov = "gradient_descent" for likelihoods whose auxiliary parameters are estimated (cases.LAPLACE_AUX_GD_CASES) by the unmodified reference at
    cases.LAPLACE_TIGHT -- tests/golden/laplace_aux_gd_ref.npz: <case>_{cov_pars, aux, num_it, negll}."""
    res = {}
    for name in cases.LAPLACE_AUX_GD_CASES:
        coords, y, c, lik, naux, cfg = cases.aux_gd_case(name)
        m = refdrv.RefCAPIModel(coords, c["cov_function"], c["shape"], c["m"], c["ordering"], c["seed"], threads=8, likelihood=lik)
        m.set_optim_config(estimate_aux_pars=True, optimizer_cov="gradient_descent", **cfg, **cases.LAPLACE_TIGHT)
        m.optim_cov_par(y)
        res[name + "_cov_pars"] = m.get_cov_par(2); res[name + "_aux"] = m.get_aux_pars(naux)
        res[name + "_num_it"] = np.int32(m.get_num_it()); res[name + "_negll"] = np.float64(m.current_neg_log_likelihood())
        print("gradient_descent with auxiliary parameters", name, res[name + "_cov_pars"], res[name + "_aux"], res[name + "_num_it"], "%.10f" % res[name + "_negll"], flush=True)
    np.savez_compressed(os.path.join(out_dir, "laplace_aux_gd_ref.npz"), **res)


def laplace_coef_weights_fixture(out_dir):
    """Round 6: sample weights TOGETHER with covariates for non-Gaussian models (GPB_CreateREModel(has_weights) + GPB_OptimLinRegrCoefCovPar; weighted intercept start
    FindInitialIntercept likelihoods.h:1455-1560, weighted step-cap constants :2618-2660, the iid model of InitCoefAuxParsFromIidModel created with the weights, re_model.cpp:401-409)
    by the unmodified reference at cases.LAPLACE_TIGHT -- tests/golden/laplace_coef_weights_ref.npz: <lik>_{noiid,iid}_{cov_pars, coef, num_it, negll}."""
    res = {}
    c = cases.LAPLACE_CASES["lap_u2d_n1500_mat15_m30"]
    w = cases.laplace_coef_weights(c["n"])
    for lik in ("bernoulli_logit", "poisson"):
        coords, y, X = cases.laplace_coef_data(lik, 3)
        for tag, iid in (("noiid", False), ("iid", True)):
            mdl = refdrv.RefCAPIModel(coords, c["cov_function"], c["shape"], c["m"], c["ordering"], c["seed"], threads=8, likelihood=lik, weights=w)
            # (the weighted logit fit runs off to a degenerate optimum -- variance 5e2, range 5e-9 -- on these data: it is stopped after 8 iterations, which pins the start and the path)
            mdl.set_optim_config(init_coef_aux_pars_from_iid_model=iid, max_iter=8 if lik == "bernoulli_logit" else -999, **cases.LAPLACE_TIGHT)
            mdl.optim_lin_regr_coef_cov_par(y, X)
            key = "%s_%s" % (lik, tag)
            res[key + "_cov_pars"] = mdl.get_cov_par(2); res[key + "_coef"] = mdl.get_coef()
            res[key + "_num_it"] = np.int32(mdl.get_num_it()); res[key + "_negll"] = np.float64(mdl.current_neg_log_likelihood())
            print("laplace coef + weights", key, res[key + "_cov_pars"], res[key + "_coef"], int(res[key + "_num_it"]), "%.10f" % res[key + "_negll"], flush=True)
    np.savez_compressed(os.path.join(out_dir, "laplace_coef_weights_ref.npz"), **res)


def laplace_t_fixdf_fixture(out_dir):
    """Round 6: likelihood "t_fix_df" (Student-t with the degrees of freedom held at likelihood_additional_param, only the scale estimated: estimate_df_t_ = false,
    likelihoods.h:384-407, :10466-10471, :16179-16183) by the unmodified reference -- tests/golden/laplace_t_fixdf_ref.npz, on cases.LAPLACE_T_CASES["t_n1500"]'s data:
      df5_negll            GPB_EvalNegLogLikelihood at (cov_pars, scale 0.5) with likelihood_additional_param = 5 (init_aux_pars = (0.5, 3): the 3 is NOT taken over), cases.LAPLACE_TIGHT
      df5_fit_*            lbfgs fit, estimate_aux_pars = true: cov_pars, aux = (scale, 5), iterations, negll (tight thresholds)
      dfdef_fit_*          the same without likelihood_additional_param (internal default df = 2), default thresholds
      t_df5_negll          likelihood "t" (df estimated) created WITH likelihood_additional_param = 5 and no init_aux_pars: evaluation at the start values (1, 5) -- pins that
                           GPB_CreateREModel reads the parameter"""
    res = {}
    tc = cases.LAPLACE_T_CASES["t_n1500"]
    c = cases.LAPLACE_CASES[tc["model"]]
    coords, y = cases.make_t_data(tc)
    cp = np.asarray(c["cov_pars"][0], dtype=np.float64)
    args = (c["cov_function"], c["shape"], c["m"], c["ordering"], c["seed"])
    mdl = refdrv.RefCAPIModel(coords, *args, threads=8, likelihood="t_fix_df", likelihood_additional_param=5.0)
    mdl.set_optim_config(init_aux_pars=np.array([0.5, 3.0]), **cases.LAPLACE_TIGHT)
    res["df5_negll"] = np.float64(mdl.neg_log_likelihood(cp, y)); res["df5_aux_after_eval"] = mdl.get_aux_pars(2)
    print("t_fix_df df=5: negll %.10f aux %s" % (res["df5_negll"], res["df5_aux_after_eval"]), flush=True)
    for key, kw, cfg in (("df5", dict(likelihood_additional_param=5.0), dict(cases.LAPLACE_TIGHT)), ("dfdef", {}, {})):
        m2 = refdrv.RefCAPIModel(coords, *args, threads=8, likelihood="t_fix_df", **kw)
        m2.set_optim_config(estimate_aux_pars=True, **cfg)
        m2.optim_cov_par(y)
        res[key + "_fit_cov_pars"] = m2.get_cov_par(2); res[key + "_fit_aux"] = m2.get_aux_pars(2)
        res[key + "_fit_num_it"] = np.int32(m2.get_num_it()); res[key + "_fit_negll"] = np.float64(m2.current_neg_log_likelihood())
        print("t_fix_df fit", key, res[key + "_fit_cov_pars"], res[key + "_fit_aux"], res[key + "_fit_num_it"], "%.10f" % res[key + "_fit_negll"], flush=True)
    m3 = refdrv.RefCAPIModel(coords, *args, threads=8, likelihood="t", likelihood_additional_param=5.0)
    m3.set_optim_config(estimate_aux_pars=False, **cases.LAPLACE_TIGHT)
    res["t_df5_negll"] = np.float64(m3.neg_log_likelihood(cp, y)); res["t_df5_aux"] = m3.get_aux_pars(2)
    print("t with likelihood_additional_param = 5: negll %.10f aux %s" % (res["t_df5_negll"], res["t_df5_aux"]), flush=True)
    np.savez_compressed(os.path.join(out_dir, "laplace_t_fixdf_ref.npz"), **res)


def laplace_weights_fixture(out_dir):
    """Round 5: non-Gaussian Vecchia-Laplace models WITH sample weights (GPB_CreateREModel(has_weights, weights)) by the unmodified reference
    (tests/golden/laplace_weights_ref.npz), per cases.LAPLACE_WEIGHT_CASES entry:
      *_negll_direct, *_grad_direct  value and gradient wrt (log sigma1^2, log a[, log aux]) from the reference's CalcGradPars at cases.LAPLACE_TIGHT (+ *_fe_*)
      *_gradF                        the boosting gradient d(-mll)/dF at cases.LAPLACE_TIGHT
      *_fit_tight_*                  GPB_OptimCovPar (lbfgs; aux estimated where there is one): estimates, iterations, negll
      *_latent_mu / _var, *_resp_mu / _var   predictions at 40 points (Cholesky-based: the exact values the iterative methods estimate)"""
    res = {}
    only = sys.argv[2:]
    path = os.path.join(out_dir, "laplace_weights_ref.npz")
    if only and os.path.isfile(path):          # `laplace_weights <name> ...`: (re)generate only these cases
        res = dict(np.load(path))
    for name, wc in cases.LAPLACE_WEIGHT_CASES.items():
        if only and name not in only:
            continue
        c = cases.LAPLACE_CASES[wc["model"]]
        coords, y, w = cases.make_weight_data(wc)
        lik, aux = wc["lik"], wc.get("aux")
        has_aux = aux is not None
        cp = np.asarray(c["cov_pars"][0], dtype=np.float64)
        args = (c["cov_function"], c["shape"], c["m"], c["ordering"], c["seed"])
        for fe_key, fe in (("", None), ("_fe", cases.laplace_fixed_effects(coords))):
            nll, g, _ = refdrv.ref_laplace_nll_grad(coords, y, cp, lik, fe, *args, aux_pars=aux, estimate_aux=has_aux, weights=w, **cases.LAPLACE_TIGHT)
            res[name + fe_key + "_negll_direct"] = np.float64(nll); res[name + fe_key + "_grad_direct"] = g
            print("laplace weights", name, fe_key, "negll %.10f" % nll, "grad", g, flush=True)
        if not has_aux:
            res[name + "_gradF"] = refdrv.ref_laplace_grad_F(coords, y, cp, lik, cases.laplace_fixed_effects(coords), *args, weights=w, **cases.LAPLACE_TIGHT)
        m2 = refdrv.RefCAPIModel(coords, *args, threads=8, likelihood=lik, weights=w)
        m2.set_optim_config(estimate_aux_pars=has_aux, **cases.LAPLACE_TIGHT)
        m2.optim_cov_par(y)
        res[name + "_fit_tight_cov_pars"] = m2.get_cov_par(2)
        res[name + "_fit_tight_init_cov_pars"] = m2.get_init_cov_par()[:2].copy()
        res[name + "_fit_tight_num_it"] = np.int32(m2.get_num_it())
        res[name + "_fit_tight_negll"] = np.float64(m2.current_neg_log_likelihood())
        if has_aux:
            res[name + "_fit_tight_aux"] = m2.get_aux_pars(1); res[name + "_fit_tight_init_aux"] = m2.get_init_aux_pars(1)
        print("laplace weights fit", name, res[name + "_fit_tight_cov_pars"], res.get(name + "_fit_tight_aux"), res[name + "_fit_tight_num_it"], res[name + "_fit_tight_negll"], flush=True)
        cpred = np.random.default_rng(79).uniform(size=(40, c["d"]))
        res[name + "_coords_pred"] = cpred
        m4 = refdrv.RefCAPIModel(coords, *args, threads=8, likelihood=lik, matrix_inversion_method="cholesky", weights=w)
        m4.set_optim_config(init_aux_pars=aux, **cases.LAPLACE_PRED_REF)
        mu, var = m4.predict(cpred, predict_var=True, predict_response=False, y=y, cov_pars=cp)
        res[name + "_latent_mu"] = mu; res[name + "_latent_var"] = var
        if lik != "quasi_bernoulli_logit":     # (the reference has no response prediction for it: "FirstDerivLogCondMeanLikelihood: Likelihood of type 'quasi_bernoulli_logit' is not supported", a fatal error)
            rmu, rvar = m4.predict(cpred, predict_var=True, predict_response=True, y=y, cov_pars=cp)
            res[name + "_resp_mu"] = rmu; res[name + "_resp_var"] = rvar
        print("laplace weights predictions", name, mu[:2], var[:2], flush=True)
        np.savez_compressed(os.path.join(out_dir, "laplace_weights_ref.npz"), **res)       # (after every case: a fatal error of the reference ends the process)


def split_fixture(out_dir):
    """The reference's FeatureHistogram::FindBestThreshold on its own (fixed) histograms: all inputs of the call + its outputs."""
    res = {}
    for name in cases.SPLIT_DATA_UNIT:
        X, g, h, leaf = cases.make_split_data(name)
        for ci, cfg in [(str(i), c) for i, c in enumerate(cases.SPLIT_CFGS)] + [("r%d" % i, c) for i, c in enumerate(cases.SPLIT_CFGS_REG)]:
            for li, di in enumerate((None, leaf)):
                for hi, hs in enumerate((None, h)):
                    bins, gnb, hist, fx = refdrv.ref_histogram(X, 63, di, g, hs, 1.0, with_fix=True,
                                                               extra_params=cases.SPLIT_DATA[name]["params"], split_cfg=cfg)
                    key = "%s_cfg%s_leaf%d_hess%d" % (name, ci, li, hi)
                    res[name + "_bins"] = bins; res[name + "_group_num_bin"] = gnb
                    res[name + "_view_offset"] = fx["view_offset"]; res[name + "_num_bin"] = fx["num_bin"]
                    res[name + "_most_freq_bin"] = fx["most_freq_bin"]; res[name + "_meta3"] = fx["meta3"]
                    res[key + "_hist_fixed"] = fx["hist_fixed"]; res[key + "_sums"] = fx["sums"]
                    res[key + "_split"] = fx["split"]; res[key + "_default_left"] = fx["split_default_left"]
        # Dataset::Split of the leaf's rows for a grid of (feature, threshold, default_left)
        req = cases.split_partition_requests(res[name + "_num_bin"])
        _, _, _, fx = refdrv.ref_histogram(X, 63, leaf, g, None, 1.0, with_fix=True, extra_params=cases.SPLIT_DATA[name]["params"],
                                           partitions=req)
        res[name + "_part_req"] = np.asarray(req, dtype=np.int32)
        res[name + "_part_lte_count"] = np.asarray([len(a) for a in fx["part_lte"]], dtype=np.int32)
        res[name + "_part_lte"] = np.concatenate(fx["part_lte"]).astype(np.int32)
        print("split fixture", name, "missing types", res[name + "_meta3"][:, 2], "num_bin", res[name + "_num_bin"])
    np.savez_compressed(os.path.join(out_dir, "split_ref.npz"), **res)


def split_cat_fixture(out_dir):
    """Round 5: the reference's FeatureHistogram::FindBestThreshold for CATEGORICAL features (FindBestThresholdCategoricalInner) on its own fixed
    histograms, and Dataset::Split with a bitset over bins (SplitCategorical): tests/golden/split_cat_ref.npz."""
    res = {}
    name = "cat"
    X, g, h, leaf = cases.make_split_data(name)
    extra = cases.SPLIT_DATA[name]["params"]
    for ci, (cfg, cc) in enumerate(cases.SPLIT_CAT_CFGS):
        for li, di in enumerate((None, leaf)):
            for hi, hs in enumerate((None, h)):
                bins, gnb, hist, fx = refdrv.ref_histogram(X, 63, di, g, hs, 1.0, with_fix=True, extra_params=extra, split_cfg=cfg, cat_cfg=cc)
                key = "%s_cfg%d_leaf%d_hess%d" % (name, ci, li, hi)
                res[name + "_bins"] = bins; res[name + "_group_num_bin"] = gnb
                res[name + "_view_offset"] = fx["view_offset"]; res[name + "_num_bin"] = fx["num_bin"]
                res[name + "_most_freq_bin"] = fx["most_freq_bin"]; res[name + "_meta3"] = fx["meta3"]; res[name + "_is_categorical"] = fx["is_categorical"]
                res[key + "_hist_fixed"] = fx["hist_fixed"]; res[key + "_sums"] = fx["sums"]
                res[key + "_split"] = fx["split"]; res[key + "_default_left"] = fx["split_default_left"]; res[key + "_cat_bits"] = fx["split_cat_bits"]
                print("split cat", key, "gains", fx["split"][:, 0], "ncat", fx["split"][fx["is_categorical"] > 0, 1])
    # Dataset::Split of the leaf's rows by bitsets over the bins of the categorical features: the root's winning sets of configuration 0 and fixed patterns
    cats = np.flatnonzero(res[name + "_is_categorical"])
    req, bits = [], []
    for f in cats:
        nb = int(res[name + "_num_bin"][f])
        pats = [res["%s_cfg0_leaf0_hess0_cat_bits" % name][f].copy()]
        for pat in (lambda b: b % 2 == 1, lambda b: b < 3, lambda b: b >= nb - 2, lambda b: True):
            w = np.zeros(8, dtype=np.uint32)
            for b in range(nb):
                if pat(b):
                    w[b >> 5] |= np.uint32(1) << np.uint32(b & 31)
            pats.append(w)
        for w in pats:
            req.append((int(f), 0, 0)); bits.append(w)
    _, _, _, fx = refdrv.ref_histogram(X, 63, leaf, g, None, 1.0, with_fix=True, extra_params=extra, partitions=req, partition_cat_bits=np.asarray(bits))
    res[name + "_part_req"] = np.asarray(req, dtype=np.int32); res[name + "_part_bits"] = np.asarray(bits, dtype=np.uint32)
    res[name + "_part_lte_count"] = np.asarray([len(a) for a in fx["part_lte"]], dtype=np.int32)
    res[name + "_part_lte"] = np.concatenate(fx["part_lte"]).astype(np.int32)
    print("split cat partitions", res[name + "_part_lte_count"])
    np.savez_compressed(os.path.join(out_dir, "split_cat_ref.npz"), **res)


def tree_fixture(out_dir):
    """Whole trees grown by the reference's SerialTreeLearner (constant and per-row hessians).  `tree r5` regenerates only the round-5 cases
    (categorical columns, bundled groups) into tree_ref_r5.npz: their bins are the UNBUNDLED per-feature columns."""
    res = {}
    r5 = "r5" in sys.argv[2:]
    for name in (cases.TREE_CASES_R5 if r5 else [k for k in cases.TREE_CASES if k not in cases.TREE_CASES_R5]):
        data, params, L, cfg = cases.tree_params(name)
        X, g, h, leaf = cases.make_split_data(data)
        for hi, hs in enumerate((None, h)):
            t = refdrv.ref_train_tree(X, params, g, hs, max_leaves=L, unbundle=r5)
            for k, v in t.items():
                res["%s_hess%d_%s" % (name, hi, k)] = np.asarray(v)
            print("tree", name, "hess%d" % hi, "leaves", t["num_leaves"], "root split feature", t["split_feature_inner"][0], "thr", t["threshold_in_bin"][0])
    np.savez_compressed(os.path.join(out_dir, "tree_ref_r5.npz" if r5 else "tree_ref.npz"), **res)


def optim_fixture(out_dir):
    """The reference's own GPB_SetOptimConfig + GPB_OptimCovPar (one OpenMP thread) for tests/cases.py:OPTIM_CASES."""
    res = {}
    path = os.path.join(out_dir, "optim_ref.npz")
    only = sys.argv[2:]                       # `optim <name> ...`: (re)generate only these cases, keep the others as they are
    if only and os.path.exists(path):
        res = dict(np.load(path))
    for name in cases.OPTIM_CASES:
        if only and name not in only:
            continue
        coords, y, ids, mc, init, cfg = cases.optim_case(name)
        mdl = refdrv.RefCAPIModel(coords, mc["cov_function"], mc["shape"], mc["m"], mc["ordering"], mc["seed"], threads=1, cluster_ids=ids)
        if init is not None or cfg:
            mdl.set_optim_config(init_cov_pars=init, **cfg)
        mdl.optim_cov_par(y)
        res[name + "_cov_pars"] = mdl.get_cov_par()
        res[name + "_init_cov_pars"] = mdl.get_init_cov_par()
        res[name + "_num_it"] = np.int32(mdl.get_num_it())
        res[name + "_negll"] = np.float64(mdl.current_neg_log_likelihood())
        print("optim", name, res[name + "_init_cov_pars"], "->", res[name + "_cov_pars"], res[name + "_num_it"], res[name + "_negll"], flush=True)
    np.savez_compressed(path, **res)


def optim_coef_fixture(out_dir):
    """The reference's own GPB_OptimLinRegrCoefCovPar + GPB_GetCoef + GPB_PredictREModel with covariates (one OpenMP thread) for
    tests/cases.py:COEF_CASES (optimizer_coef left at the reference's default for Gaussian data, "wls")."""
    res = {}
    for name in cases.COEF_CASES:
        coords, y, X, mc, init, cfg, Xp = cases.coef_case(name)
        mdl = refdrv.RefCAPIModel(coords, mc["cov_function"], mc["shape"], mc["m"], mc["ordering"], mc["seed"], threads=1)
        if init is not None or cfg:
            mdl.set_optim_config(init_cov_pars=init, **cfg)
        mdl.optim_lin_regr_coef_cov_par(y, X)
        res[name + "_cov_pars"] = mdl.get_cov_par()
        res[name + "_coef"] = mdl.get_coef()
        res[name + "_coef_sd"] = mdl.get_coef(std_dev=True)[mdl.p:]
        res[name + "_num_it"] = np.int32(mdl.get_num_it())
        res[name + "_negll"] = np.float64(mdl.current_neg_log_likelihood())
        mu, var = mdl.predict(cases.COEF_PRED_COORDS, Xp)
        res[name + "_pred_mu"], res[name + "_pred_var"] = mu, var
        mu, var = mdl.predict(cases.COEF_PRED_COORDS, Xp, vecchia_pred_type="order_obs_first_cond_all")
        res[name + "_pred_all_mu"], res[name + "_pred_all_var"] = mu, var
        print("optim coef", name, res[name + "_cov_pars"], res[name + "_coef"], res[name + "_num_it"], res[name + "_negll"], mu, flush=True)
    np.savez_compressed(os.path.join(out_dir, "optim_coef_ref.npz"), **res)


def optim_laplace_fixture(out_dir):
    """The reference's own GPB_OptimCovPar for non-Gaussian Vecchia models (iterative methods, vadu): tests/cases.py:OPTIM_LAPLACE_CASES."""
    res = {}
    path = os.path.join(out_dir, "optim_laplace_ref.npz")
    only = sys.argv[2:]                       # `optim_laplace <name> ...`: (re)generate only these cases, keep the others as they are
    if only and os.path.exists(path):
        res = dict(np.load(path))
    for name, oc in cases.OPTIM_LAPLACE_CASES.items():
        if only and name not in only:
            continue
        c = cases.LAPLACE_CASES[oc["model"]]
        coords, y = cases.make_count_data(c) if oc["lik"] == "poisson" else cases.make_binary_data(c)
        mdl = refdrv.RefCAPIModel(coords, c["cov_function"], c["shape"], c["m"], c["ordering"], c["seed"], threads=8, likelihood=oc["lik"])
        if oc["cfg"]:
            mdl.set_optim_config(**oc["cfg"])
        mdl.optim_cov_par(y, cases.laplace_fixed_effects(coords) if oc.get("fe") else None)
        res[name + "_cov_pars"] = mdl.get_cov_par(2)
        res[name + "_init_cov_pars"] = mdl.get_init_cov_par()[:2].copy()
        res[name + "_num_it"] = np.int32(mdl.get_num_it())
        res[name + "_negll"] = np.float64(mdl.current_neg_log_likelihood())
        print("optim laplace", name, res[name + "_init_cov_pars"], "->", res[name + "_cov_pars"], res[name + "_num_it"], res[name + "_negll"], flush=True)
    np.savez_compressed(path, **res)


def laplace_dup_fixture(out_dir):
    """Non-Gaussian Vecchia models with REPEATED locations (tests/cases.py:LAPLACE_DUP_CASES): the unmodified reference's likelihood values (with and
    without fixed effects), its fit, and the latent predictive mean after the fit (tests/golden/laplace_dup_ref.npz)."""
    res = {}
    for name, (cf, sh, m, ordering, seed) in cases.LAPLACE_DUP_CASES.items():
        for lik in ("bernoulli_logit", "bernoulli_probit", "poisson"):
            coords, y, fe, cpred = cases.laplace_dup_data(lik)
            mdl = refdrv.RefCAPIModel(coords, cf, sh, m, ordering, seed, threads=4, likelihood=lik)
            for k, cp in enumerate(cases.LAPLACE_DUP_COV_PARS):
                res["%s_%s_negll_%d" % (name, lik, k)] = np.float64(mdl.neg_log_likelihood(np.asarray(cp, dtype=np.float64), y))
            res["%s_%s_fe_negll_0" % (name, lik)] = np.float64(mdl.neg_log_likelihood(np.asarray(cases.LAPLACE_DUP_COV_PARS[0], dtype=np.float64), y, fe))
            mdl.set_optim_config(cg_delta_conv=1e-8, delta_conv_mode_finding=1e-13)
            mdl.optim_cov_par(y)
            res["%s_%s_fit_cov_pars" % (name, lik)] = mdl.get_cov_par(2)
            res["%s_%s_fit_num_it" % (name, lik)] = np.int32(mdl.get_num_it())
            res["%s_%s_fit_negll" % (name, lik)] = np.float64(mdl.current_neg_log_likelihood())
            mu, _ = mdl.predict(cpred, predict_var=False, predict_response=False)
            res["%s_%s_pred_latent_mu" % (name, lik)] = mu
            print("laplace dup", name, lik, [float(res["%s_%s_negll_%d" % (name, lik, k)]) for k in range(2)], res["%s_%s_fit_cov_pars" % (name, lik)],
                  int(res["%s_%s_fit_num_it" % (name, lik)]), flush=True)
    np.savez_compressed(os.path.join(out_dir, "laplace_dup_ref.npz"), **res)


def laplace_pred_fixture(out_dir):
    """Latent predictive mean of the reference for non-Gaussian Vecchia models after its own fit (GPB_PredictREModel, predict_response = false,
    no variances; PredictLaplaceApproxVecchia, likelihoods.h:8600-8602) -- tests/cases.py:LAPLACE_CASES lap_u2d_n1500_mat15_m30."""
    res = {}
    c = cases.LAPLACE_CASES["lap_u2d_n1500_mat15_m30"]
    cpred = np.random.default_rng(77).uniform(size=(40, 2))
    res["coords_pred"] = cpred
    for lik in ("bernoulli_logit", "bernoulli_probit", "poisson"):
        coords, y = cases.make_count_data(c) if lik == "poisson" else cases.make_binary_data(c)
        mdl = refdrv.RefCAPIModel(coords, c["cov_function"], c["shape"], c["m"], c["ordering"], c["seed"], threads=8, likelihood=lik)
        mdl.set_optim_config(cg_delta_conv=1e-8, delta_conv_mode_finding=1e-13)     # the mode to ~1e-7: the comparison is of the prediction, not of Newton's stopping rule
        mdl.optim_cov_par(y)
        mu, _ = mdl.predict(cpred, predict_var=False, predict_response=False)
        res[lik + "_cov_pars"] = mdl.get_cov_par(2)
        res[lik + "_pred_latent_mu"] = mu
        print("laplace pred", lik, res[lik + "_cov_pars"], mu[:4], flush=True)
    np.savez_compressed(os.path.join(out_dir, "laplace_pred_ref.npz"), **res)


def laplace_dup_gradF_fixture(out_dir):
    """The reference's boosting gradient (REModel::CalcGradient, data order) for non-Gaussian Vecchia models with REPEATED locations -- the data-scale
    form of likelihoods.h:6944-6966 -- at the first parameters of LAPLACE_DUP_COV_PARS with the fixed effects of laplace_dup_data."""
    res = {}
    for name, (cf, sh, m, ordering, seed) in cases.LAPLACE_DUP_CASES.items():
        for lik in ("bernoulli_logit", "bernoulli_probit", "poisson"):
            coords, y, fe, _ = cases.laplace_dup_data(lik)
            g = refdrv.ref_laplace_grad_F(coords, y, cases.LAPLACE_DUP_COV_PARS[0], lik, fe, cf, sh, m, ordering, seed)
            res["%s_%s_gradF" % (name, lik)] = g
            print("laplace dup grad F", name, lik, np.abs(g).max(), flush=True)
    np.savez_compressed(os.path.join(out_dir, "laplace_dup_gradF_ref.npz"), **res)


def laplace_coef_fixture(out_dir):
    """Fits of non-Gaussian Vecchia models WITH a linear predictor by the unmodified reference (GPB_OptimLinRegrCoefCovPar, default optimiser lbfgs:
    the regression coefficients are part of the lbfgs vector, covariates scaled, re_model_template.h:1218-1300; init_coef_aux_pars_from_iid_model =
    false: the intercept starts at FindInitialIntercept, the other coefficients at 0): covariance parameters, coefficients, iterations, likelihood."""
    res = {}
    c = cases.LAPLACE_CASES["lap_u2d_n1500_mat15_m30"]
    for lik in ("bernoulli_logit", "bernoulli_probit", "poisson"):
        for n_cov in (2, 3):
            coords, y, X = cases.laplace_coef_data(lik, n_cov)
            mdl = refdrv.RefCAPIModel(coords, c["cov_function"], c["shape"], c["m"], c["ordering"], c["seed"], threads=8, likelihood=lik)
            mdl.set_optim_config()
            mdl.optim_lin_regr_coef_cov_par(y, X)
            key = "%s_p%d" % (lik, n_cov)
            res[key + "_cov_pars"] = mdl.get_cov_par(2)
            res[key + "_coef"] = mdl.get_coef()
            res[key + "_num_it"] = np.int32(mdl.get_num_it())
            res[key + "_negll"] = np.float64(mdl.current_neg_log_likelihood())
            res[key + "_coef_sd"] = mdl.get_coef(std_dev=True)[n_cov:]       # CalcStdDevCoefNonGaussian: numerical Hessian at the fitted model (perturbs the state: read last)
            print("laplace coef", key, res[key + "_cov_pars"], res[key + "_coef"], int(res[key + "_num_it"]), float(res[key + "_negll"]), flush=True)
            if n_cov == 2:      # prediction with X_pred after that fit: latent mean (matrix_inversion_method "default": no variances compared)
                cpred = np.random.default_rng(79).uniform(size=(25, 2))
                Xp = np.c_[np.ones(25), np.sin(3 * cpred[:, 0] + cpred[:, 1])]
                mu, _ = mdl.predict(cpred, X_pred=Xp, predict_var=False, predict_response=False)
                res[key + "_pred_coords"] = cpred; res[key + "_pred_X"] = Xp; res[key + "_pred_latent_mu"] = mu
            # the same fit with the iterative solvers' tolerances tightened (cg_delta_conv 1e-8, delta_conv_mode_finding 1e-13): the gradient no longer
            # carries the noise of CG solves stopped at |r| < 1e-2, so that two implementations of the same optimiser stay on the same path
            mdl = refdrv.RefCAPIModel(coords, c["cov_function"], c["shape"], c["m"], c["ordering"], c["seed"], threads=8, likelihood=lik)
            mdl.set_optim_config(cg_delta_conv=1e-8, delta_conv_mode_finding=1e-13)
            mdl.optim_lin_regr_coef_cov_par(y, X)
            res[key + "_tight_cov_pars"] = mdl.get_cov_par(2)
            res[key + "_tight_coef"] = mdl.get_coef()
            res[key + "_tight_num_it"] = np.int32(mdl.get_num_it())
            res[key + "_tight_negll"] = np.float64(mdl.current_neg_log_likelihood())
            print("laplace coef tight", key, res[key + "_tight_cov_pars"], res[key + "_tight_coef"], int(res[key + "_tight_num_it"]), float(res[key + "_tight_negll"]), flush=True)
            m0 = refdrv.RefCAPIModel(coords, c["cov_function"], c["shape"], c["m"], c["ordering"], c["seed"], threads=8, likelihood=lik)
            m0.set_optim_config(max_iter=0); m0.optim_lin_regr_coef_cov_par(y, X)
            res[key + "_init_cov_pars"] = m0.get_cov_par(2)             # the reference's own initial values (FindInitCovPar)
    # edge cases of the set-up (tight tolerances): an intercept alone (no scaling), no intercept (every column scaled, coefficients start at 0),
    # covariates together with fixed effects (Poisson intercept from mean(y / exp(F)))
    coords, _, X3 = cases.laplace_coef_data("bernoulli_logit", 3)
    fe_edge = 0.3 * np.cos(7 * np.arange(c["n"]) / c["n"])
    for tag, lik, cols, fe in (("intercept_only", "bernoulli_logit", slice(0, 1), None), ("no_intercept", "poisson", slice(1, 3), None),
                               ("with_fixed_effects", "poisson", slice(0, 2), fe_edge)):
        _, y, _ = cases.laplace_coef_data(lik, 3)
        X = X3[:, cols]
        mdl = refdrv.RefCAPIModel(coords, c["cov_function"], c["shape"], c["m"], c["ordering"], c["seed"], threads=8, likelihood=lik)
        mdl.set_optim_config(cg_delta_conv=1e-8, delta_conv_mode_finding=1e-13)
        mdl.optim_lin_regr_coef_cov_par(y, X, fixed_effects=fe)
        key = "edge_" + tag
        res[key + "_cov_pars"] = mdl.get_cov_par(2); res[key + "_coef"] = mdl.get_coef()
        res[key + "_num_it"] = np.int32(mdl.get_num_it()); res[key + "_negll"] = np.float64(mdl.current_neg_log_likelihood())
        m0 = refdrv.RefCAPIModel(coords, c["cov_function"], c["shape"], c["m"], c["ordering"], c["seed"], threads=8, likelihood=lik)
        m0.set_optim_config(max_iter=0); m0.optim_lin_regr_coef_cov_par(y, X, fixed_effects=fe)
        res[key + "_init_cov_pars"] = m0.get_cov_par(2)
        print("laplace coef", key, res[key + "_cov_pars"], res[key + "_coef"], int(res[key + "_num_it"]), flush=True)
    # the packages' default: initial coefficients from the "iid model" (init_coef_aux_pars_from_iid_model = true, re_model.cpp:380-470) -- the
    # coefficients it supplies (a fit with max_iter = 0 returns them) and the fit that starts there (tight tolerances)
    for lik in ("bernoulli_logit", "bernoulli_probit", "poisson"):
        coords, y, X = cases.laplace_coef_data(lik, 3)
        key = "iid_" + lik
        m0 = refdrv.RefCAPIModel(coords, c["cov_function"], c["shape"], c["m"], c["ordering"], c["seed"], threads=8, likelihood=lik)
        m0.set_optim_config(max_iter=0, init_coef_aux_pars_from_iid_model=True); m0.optim_lin_regr_coef_cov_par(y, X)
        res[key + "_init_cov_pars"] = m0.get_cov_par(2); res[key + "_init_coef"] = m0.get_coef()
        mdl = refdrv.RefCAPIModel(coords, c["cov_function"], c["shape"], c["m"], c["ordering"], c["seed"], threads=8, likelihood=lik)
        mdl.set_optim_config(cg_delta_conv=1e-8, delta_conv_mode_finding=1e-13, init_coef_aux_pars_from_iid_model=True)
        mdl.optim_lin_regr_coef_cov_par(y, X)
        res[key + "_cov_pars"] = mdl.get_cov_par(2); res[key + "_coef"] = mdl.get_coef()
        res[key + "_num_it"] = np.int32(mdl.get_num_it()); res[key + "_negll"] = np.float64(mdl.current_neg_log_likelihood())
        print("laplace coef", key, res[key + "_init_coef"], res[key + "_cov_pars"], res[key + "_coef"], int(res[key + "_num_it"]), flush=True)
    # a data set whose mean response is ~1: |log(mean y)| = 0.0014, so the floor C_mu >= 1 of the step cap decides the first steps
    # (FindConstantsCapTooLargeLearningRateCoef, likelihoods.h:2741-2743); 700 data, m = 20, with and without the iid-model coefficients
    for iid in (False, True):
        coords, y, X = cases.laplace_coef_data("poisson", 2)
        coords, y, X = coords[:700], y[:700], X[:700]
        key = "cmu_floor_iid%d" % int(iid)
        m0 = refdrv.RefCAPIModel(coords, "matern", 1.5, 20, "random", 2, threads=8, likelihood="poisson")
        m0.set_optim_config(max_iter=0, init_coef_aux_pars_from_iid_model=iid); m0.optim_lin_regr_coef_cov_par(y, X)
        res[key + "_init_cov_pars"] = m0.get_cov_par(2)
        mdl = refdrv.RefCAPIModel(coords, "matern", 1.5, 20, "random", 2, threads=8, likelihood="poisson")
        mdl.set_optim_config(cg_delta_conv=1e-8, delta_conv_mode_finding=1e-13, init_coef_aux_pars_from_iid_model=iid)
        mdl.optim_lin_regr_coef_cov_par(y, X)
        res[key + "_cov_pars"] = mdl.get_cov_par(2); res[key + "_coef"] = mdl.get_coef()
        res[key + "_num_it"] = np.int32(mdl.get_num_it()); res[key + "_negll"] = np.float64(mdl.current_neg_log_likelihood())
        print("laplace coef", key, res[key + "_cov_pars"], res[key + "_coef"], int(res[key + "_num_it"]), flush=True)
    # covariance parameters held fixed (estimate_cov_par_index; tight tolerances): without and with covariates
    for tag, est, n_cov in (("fix_range", [1, 0], 0), ("fix_var", [0, 1], 0), ("fix_var_p2", [0, 1], 2)):
        coords, y, X = cases.laplace_coef_data("bernoulli_logit", max(n_cov, 1))
        mdl = refdrv.RefCAPIModel(coords, c["cov_function"], c["shape"], c["m"], c["ordering"], c["seed"], threads=8, likelihood="bernoulli_logit")
        mdl.set_optim_config(init_cov_pars=np.array([0.5, 0.2]), cg_delta_conv=1e-8, delta_conv_mode_finding=1e-13, estimate_cov_par_index=est)
        if n_cov:
            mdl.optim_lin_regr_coef_cov_par(y, X)
            res["est_" + tag + "_coef"] = mdl.get_coef()
        else:
            mdl.optim_cov_par(y)
        key = "est_" + tag
        res[key + "_cov_pars"] = mdl.get_cov_par(2); res[key + "_num_it"] = np.int32(mdl.get_num_it())
        res[key + "_negll"] = np.float64(mdl.current_neg_log_likelihood())
        out4 = np.empty(4); rc = mdl.L.GPB_GetCovPar(mdl.h, out4.ctypes.data_as(__import__("ctypes").c_void_p), __import__("ctypes").c_bool(True))
        res[key + "_std"] = out4[2:]
        print("laplace coef", key, res[key + "_cov_pars"], int(res[key + "_num_it"]), out4[2:], flush=True)
    np.savez_compressed(os.path.join(out_dir, "laplace_coef_ref.npz"), **res)


def laplace_stderr_fixture(out_dir):
    """Standard errors of the covariance parameters of non-Gaussian Vecchia models: GPB_GetCovPar(calc_std_dev = true) after the reference's own lbfgs
    fit = CalcStdDevCovParAuxParsNonGaussian (re_model_template.h:11029-11117): Hessian of the approximate negative log-likelihood as the numerical
    Jacobian (central differences, step 1e-4 |log theta|) of its analytic gradient, delta method back to the original scale.  One process per case
    (random vectors of the first model of a process)."""
    import subprocess
    res = {}
    for lik in ("bernoulli_logit", "bernoulli_probit", "poisson"):
        code = ("import sys, ctypes as C, numpy as np; sys.path.insert(0, %r); from oracle import refdrv; from tests import cases\n"
                "c = cases.LAPLACE_CASES['lap_u2d_n1500_mat15_m30']\n"
                "coords, y = cases.make_count_data(c) if %r == 'poisson' else cases.make_binary_data(c)\n"
                "mdl = refdrv.RefCAPIModel(coords, c['cov_function'], c['shape'], c['m'], c['ordering'], c['seed'], threads=8, likelihood=%r)\n"
                "mdl.set_optim_config(); mdl.optim_cov_par(y)\n"
                "out = np.empty(4); rc = mdl.L.GPB_GetCovPar(mdl.h, out.ctypes.data_as(C.c_void_p), C.c_bool(True)); assert rc == 0\n"
                "print(' '.join('%%.17g' %% v for v in out))\n") % (ROOT, lik, lik)
        line = subprocess.run([sys.executable, "-c", code], check=True, capture_output=True, text=True).stdout.strip().splitlines()[-1]
        v = np.array([float(t) for t in line.split()])
        res[lik + "_cov_pars"] = v[:2]; res[lik + "_std"] = v[2:]
        print("laplace stderr", lik, v, flush=True)
    np.savez_compressed(os.path.join(out_dir, "laplace_stderr_ref.npz"), **res)


def laplace_train_re_fixture(out_dir):
    """GPB_PredictREModelTrainingDataRandomEffects of the reference for non-Gaussian Vecchia models (re_model_template.h:4683-4725): the mode of the
    latent process at the training locations and, calc_var, diag((Sigma^-1 + W)^-1) (CalcVarLaplaceApproxVecchia) -- with matrix_inversion_method =
    "cholesky", i.e. the exact diagonal that the iterative branch estimates.  Cases: lap_u2d_n1500_mat15_m30 (three likelihoods) and the repeated
    locations of dup_mat15_m20_random (logit)."""
    res = {}
    c = cases.LAPLACE_CASES["lap_u2d_n1500_mat15_m30"]
    cp = np.asarray(c["cov_pars"][0], dtype=np.float64)
    for lik in ("bernoulli_logit", "bernoulli_probit", "poisson"):
        coords, y = cases.make_count_data(c) if lik == "poisson" else cases.make_binary_data(c)
        mdl = refdrv.RefCAPIModel(coords, c["cov_function"], c["shape"], c["m"], c["ordering"], c["seed"], threads=8, likelihood=lik,
                                  matrix_inversion_method="cholesky")
        mdl.set_optim_config(delta_conv_mode_finding=1e-13)
        mu, var = mdl.predict_training_data_random_effects(y, cp, calc_var=True)
        res[lik + "_mu"] = mu; res[lik + "_var"] = var
        print("laplace train re", lik, mu[:3], var[:3], flush=True)
    cf, sh, m, ordering, seed = cases.LAPLACE_DUP_CASES["dup_mat15_m20_random"]
    coords, y, fe, _ = cases.laplace_dup_data("bernoulli_logit")
    mdl = refdrv.RefCAPIModel(coords, cf, sh, m, ordering, seed, threads=4, likelihood="bernoulli_logit", matrix_inversion_method="cholesky")
    mdl.set_optim_config(delta_conv_mode_finding=1e-13)
    mu, var = mdl.predict_training_data_random_effects(y, np.asarray(cases.LAPLACE_DUP_COV_PARS[0], dtype=np.float64), calc_var=True)
    res["dup_bernoulli_logit_mu"] = mu; res["dup_bernoulli_logit_var"] = var
    print("laplace train re dup", mu[:3], var[:3], flush=True)
    np.savez_compressed(os.path.join(out_dir, "laplace_train_re_ref.npz"), **res)


def laplace_predvar_fixture(out_dir):
    """Predictive VARIANCES and RESPONSE predictions of the reference for non-Gaussian Vecchia models at fixed parameters
    (GPB_PredictREModel -> PredictLaplaceApproxVecchia, likelihoods.h:8563-8824, then PredictResponse, :9626-9672), with
    matrix_inversion_method = "cholesky": the exact value Dp + diag(Bpo (Sigma^-1 + W)^-1 Bpo') that the reference's iterative method estimates with
    nsim_var_pred random vectors (:8637-8745).  Also stored: the "iterative" estimate (different random vectors on every platform: a loose sanity
    check only).  Cases: tests/cases.py lap_u2d_n1500_mat15_m30 (first parameters) and the repeated-location data of LAPLACE_DUP_CASES."""
    res = {}
    c = cases.LAPLACE_CASES["lap_u2d_n1500_mat15_m30"]
    cpred = np.random.default_rng(78).uniform(size=(60, 2))
    res["coords_pred"] = cpred
    cp = np.asarray(c["cov_pars"][0], dtype=np.float64)
    for lik in ("bernoulli_logit", "bernoulli_probit", "poisson"):
        coords, y = cases.make_count_data(c) if lik == "poisson" else cases.make_binary_data(c)
        fe = cases.laplace_fixed_effects(coords)
        for inv in ("cholesky", "iterative"):
            mdl = refdrv.RefCAPIModel(coords, c["cov_function"], c["shape"], c["m"], c["ordering"], c["seed"], threads=8, likelihood=lik,
                                      matrix_inversion_method=inv)
            mdl.set_optim_config(cg_delta_conv=1e-8, delta_conv_mode_finding=1e-13)
            mu, var = mdl.predict(cpred, predict_var=True, predict_response=False, y=y, cov_pars=cp)
            rmu, rvar = mdl.predict(cpred, predict_var=True, predict_response=True, y=y, cov_pars=cp)
            key = "%s_%s" % (lik, inv)
            res[key + "_latent_mu"] = mu; res[key + "_latent_var"] = var
            res[key + "_resp_mu"] = rmu; res[key + "_resp_var"] = rvar
            print("laplace predvar", key, mu[:2], var[:2], rmu[:2], rvar[:2], flush=True)
    # 'latent_order_obs_first_cond_all': prediction points condition on each other (clustered points so that they do)
    rngc = np.random.default_rng(80)
    cpc = np.vstack([0.5 + 0.02 * rngc.normal(size=(15, 2)), rngc.uniform(size=(15, 2))])
    res["coords_pred_cond_all"] = cpc
    for lik in ("bernoulli_logit", "poisson"):
        coords, y = cases.make_count_data(c) if lik == "poisson" else cases.make_binary_data(c)
        mdl = refdrv.RefCAPIModel(coords, c["cov_function"], c["shape"], c["m"], c["ordering"], c["seed"], threads=8, likelihood=lik,
                                  matrix_inversion_method="cholesky")
        mdl.set_optim_config(cg_delta_conv=1e-8, delta_conv_mode_finding=1e-13)
        mu, cov = mdl.predict(cpc, predict_cov_mat=True, predict_response=False, y=y, cov_pars=cp, vecchia_pred_type="latent_order_obs_first_cond_all",
                              num_neighbors_pred=40)
        rmu, rvar = mdl.predict(cpc, predict_var=True, predict_response=True, y=y, cov_pars=cp)
        res["cond_all_%s_latent_mu" % lik] = mu; res["cond_all_%s_latent_cov" % lik] = cov
        res["cond_all_%s_resp_mu" % lik] = rmu; res["cond_all_%s_resp_var" % lik] = rvar
        print("laplace predvar cond_all", lik, mu[:2], np.diag(cov)[:2], cov[0, 1], flush=True)
    # repeated locations (the GP on the unique locations; prediction points with repeats too)
    name = "dup_mat15_m20_random"
    cf, sh, m, ordering, seed = cases.LAPLACE_DUP_CASES[name]
    for lik in ("bernoulli_logit", "poisson"):
        coords, y, fe, cpd = cases.laplace_dup_data(lik)
        cpd2 = np.vstack([cpd, cpd[:5]])
        mdl = refdrv.RefCAPIModel(coords, cf, sh, m, ordering, seed, threads=4, likelihood=lik, matrix_inversion_method="cholesky")
        mdl.set_optim_config(cg_delta_conv=1e-8, delta_conv_mode_finding=1e-13)
        cpv = np.asarray(cases.LAPLACE_DUP_COV_PARS[0], dtype=np.float64)
        mu, var = mdl.predict(cpd2, predict_var=True, predict_response=False, y=y, cov_pars=cpv)
        rmu, rvar = mdl.predict(cpd2, predict_var=True, predict_response=True, y=y, cov_pars=cpv)
        key = "dup_%s" % lik
        res[key + "_latent_mu"] = mu; res[key + "_latent_var"] = var
        res[key + "_resp_mu"] = rmu; res[key + "_resp_var"] = rvar
        print("laplace predvar", key, mu[:2], var[:2], rmu[:2], rvar[:2], flush=True)
    np.savez_compressed(os.path.join(out_dir, "laplace_predvar_ref.npz"), **res)


def laplace_grad_F_fixture(out_dir):
    """The reference's boosting gradient for non-Gaussian data (REModel::CalcGradient, data order) at the first parameters of the three
    Laplace cases, with the fixed effects of the other fixtures, for logit / probit / Poisson."""
    res = {}
    for name, c in cases.LAPLACE_CASES.items():
        for lik in ("bernoulli_logit", "bernoulli_probit", "poisson"):
            coords, y = cases.make_count_data(c) if lik == "poisson" else cases.make_binary_data(c)
            g = refdrv.ref_laplace_grad_F(coords, y, c["cov_pars"][0], lik, cases.laplace_fixed_effects(coords), c["cov_function"], c["shape"],
                                          c["m"], c["ordering"], c["seed"])
            res["%s_%s_gradF" % (name, lik)] = g
            print("laplace grad F", name, lik, np.abs(g).max(), flush=True)
            # the pin (round 5): the same at cases.LAPLACE_TIGHT (cg_delta_conv 1e-8, delta_conv_mode_finding 1e-13) -- no stopping-rule noise
            gt = refdrv.ref_laplace_grad_F(coords, y, c["cov_pars"][0], lik, cases.laplace_fixed_effects(coords), c["cov_function"], c["shape"],
                                           c["m"], c["ordering"], c["seed"], **cases.LAPLACE_TIGHT)
            res["%s_%s_gradF_tight" % (name, lik)] = gt
            print("laplace grad F (tight)", name, lik, np.abs(gt).max(), np.abs(gt - g).max(), flush=True)
    np.savez_compressed(os.path.join(out_dir, "laplace_gradF_ref.npz"), **res)


def fisher_fixture(out_dir):
    """Standard errors of the covariance parameters (GPB_GetCovPar(calc_std_dev = true) after the reference's own fit; stochastic Fisher
    information with the default 50 probe vectors, seed 1, first model of the process = run id 0).  One process per case."""
    import ctypes as C
    res = {}
    for name in ("r_gd_nesterov_parcrit", "r_mat15_lbfgs", "u1d_n1000_mat15_lbfgs"):
        code = ("import sys, ctypes as C, numpy as np; sys.path.insert(0, %r); from oracle import refdrv; from tests import cases\n"
                "coords, y, ids, mc, init, cfg = cases.optim_case(%r)\n"
                "mdl = refdrv.RefCAPIModel(coords, mc['cov_function'], mc['shape'], mc['m'], mc['ordering'], mc['seed'], threads=1)\n"
                "mdl.set_optim_config(init_cov_pars=init, **cfg); mdl.optim_cov_par(y)\n"
                "out = np.empty(6); rc = mdl.L.GPB_GetCovPar(mdl.h, out.ctypes.data_as(C.c_void_p), C.c_bool(True)); assert rc == 0\n"
                "print(' '.join('%%.17g' %% v for v in out))\n") % (ROOT, name)
        import subprocess
        line = subprocess.run([sys.executable, "-c", code], check=True, capture_output=True, text=True).stdout.strip().splitlines()[-1]
        v = np.array([float(t) for t in line.split()])
        res[name + "_cov_pars"] = v[:3]; res[name + "_std"] = v[3:]
        print("fisher", name, v, flush=True)
    np.savez_compressed(os.path.join(out_dir, "fisher_ref.npz"), **res)


def cluster_fixture(out_dir):
    """Reference nll of a model with several clusters (independent GP realisations), random Vecchia ordering: pins the cluster
    order (first appearance) and the ONE shared std::mt19937 that shuffles cluster after cluster."""
    c = cases.CLUSTER_CASE
    coords, y, ids = cases.make_cluster_data()
    mdl = refdrv.RefCAPIModel(coords, c["cov_function"], c["shape"], c["m"], c["ordering"], c["seed"], threads=8, cluster_ids=ids)
    nll = mdl.neg_log_likelihood(np.asarray(c["cov_pars"], dtype=np.float64), y)
    np.savez_compressed(os.path.join(out_dir, "clusters_ref.npz"), nll=np.float64(nll))
    print("clusters: nll = %.12f" % nll)


def hist_fixture(out_dir):
    X, g, h, leaf = cases.make_hist_data()
    res = {}
    for li, di in enumerate((None, leaf)):
        for hi, hs in enumerate((None, h)):
            bins, gnb, hist, fx = refdrv.ref_histogram(X, cases.HIST_CASE["max_bin"], di, g, hs, 1.0, with_fix=True)
            res["bins"] = bins; res["group_num_bin"] = gnb
            res["hist_leaf%d_hess%d" % (li, hi)] = hist
            # Dataset::FixHistogram on every feature (row a12): inputs of the call + result
            res["fix_view_offset"] = fx["view_offset"]; res["fix_num_bin"] = fx["num_bin"]; res["fix_most_freq_bin"] = fx["most_freq_bin"]
            res["fix_sums_leaf%d_hess%d" % (li, hi)] = fx["sums"]
            res["hist_fixed_leaf%d_hess%d" % (li, hi)] = fx["hist_fixed"]
    np.savez_compressed(os.path.join(out_dir, "hist_ref.npz"), **res)
    print("wrote hist_ref: groups", len(res["group_num_bin"]), "bins", res["group_num_bin"], "most_freq_bin", res["fix_most_freq_bin"])


# BASELINE.json sizes: what the judge's round-1 review asked for -- value comparisons at n = 1e5 / 1e6, not only invariants.
ATSIZE_CASES = {
    # name: (n, d, m, cov_function, shape, cov_pars)            inputs: tests/cases.synthetic(n, d, seed=1), ordering random, seed 1
    "config2_n1e5_exp_m30": (100000, 2, 30, "exponential", 0.5, (0.1, 1.0, 0.1)),
    "metric_n1e6_exp_m30": (1000000, 2, 30, "exponential", 0.5, (0.1, 1.0, 0.1)),
    "config5_n1e6_d3_mat25_m40": (1000000, 3, 40, "matern", 2.5, (0.1, 1.0, 0.1)),
}


def _sha(a):
    import hashlib
    return hashlib.sha256(np.ascontiguousarray(a).tobytes()).hexdigest()


def atsize_fixture(out_dir, only=None):
    """Reference nll / gradient / D sample / hashes of the ordering and of the WHOLE n x m neighbour table at BASELINE sizes
    (tests/golden/atsize_ref.npz; one reference evaluation each: 0.4 s at n = 1e5, 5-10 s at n = 1e6, neighbour search 24-170 s)."""
    path = os.path.join(out_dir, "atsize_ref.npz")
    res = dict(np.load(path)) if os.path.exists(path) else {}
    for name, (n, d, m, cf, sh, cp) in ATSIZE_CASES.items():
        if only and name not in only:
            continue
        coords, y = cases.synthetic(n, d, seed=1)
        mdl = refdrv.RefModel(coords, cf, sh, m, "random", 1)
        perm = mdl.perm(); nn = mdl.neighbors()
        nll, g, pt = mdl.nll_grad(y, np.asarray(cp, dtype=np.float64))
        A, D, ya = mdl.factor()
        rows = np.arange(0, n, n // 1000)
        res[name + "_nll"] = np.float64(nll); res[name + "_grad"] = g
        res[name + "_perm_sha256"] = np.array(_sha(perm.astype(np.int32)))
        res[name + "_nn_sha256"] = np.array(_sha(nn.astype(np.int32)))
        res[name + "_rows"] = rows; res[name + "_D_rows"] = D[rows]; res[name + "_yaux_rows"] = ya[rows]
        res[name + "_nn_rows"] = nn[rows].astype(np.int32)
        print("atsize", name, "nll = %.10f" % nll, "grad =", g, flush=True)
        del mdl
        np.savez_compressed(path, **res)


def vif_fixture(out_dir, only=None):
    """gp_approx = "full_scale_vecchia" (VIF), Gaussian likelihood: the unmodified reference's GPB_EvalNegLogLikelihood on tests/cases.py:VIF_CASES
    (tests/golden/vif_ref.npz)."""
    import time
    path = os.path.join(out_dir, "vif_ref.npz")
    res = dict(np.load(path)) if os.path.exists(path) else {}
    for name, (n, d, cf, sh, m, k, ordering, seed, cps) in cases.VIF_CASES.items():
        if only and name not in only:
            continue
        coords, y = cases.vif_data(name)
        mdl = refdrv.RefCAPIModel(coords, cf, sh, m, ordering, seed, threads=8, gp_approx="full_scale_vecchia", num_ind_points=k)
        for j, cp in enumerate(cps):
            t0 = time.time()
            res["%s_negll_%d" % (name, j)] = np.float64(mdl.neg_log_likelihood(np.asarray(cp, dtype=np.float64), y))
            print("vif", name, cp, "negll = %.12f" % res["%s_negll_%d" % (name, j)], "%.1f s" % (time.time() - t0), flush=True)
        del mdl
        np.savez_compressed(path, **res)


VIF_FIT_CASES = ["vif_u2d_n1500_exp_m15_k40_none", "vif_u2d_n3000_mat15_m30_k100_random", "vif_u3d_n2000_mat25_m20_k64_random"]


VIF_FIT_CASES = ["vif_u2d_n1500_exp_m15_k40_none", "vif_u2d_n3000_mat15_m30_k100_random", "vif_u3d_n2000_mat25_m20_k64_random"]


def vif_pred_fixture(out_dir):
    """Predictive means and variances (response and latent) of full-scale Vecchia models at given parameters,
    'order_obs_first_cond_obs_only', by the unmodified reference: VIF_FIT_CASES, 25 prediction points default_rng(51)
    (tests/golden/vif_pred_ref.npz)."""
    res = {}
    for name in VIF_FIT_CASES:
        n, d, cf, sh, m, k, ordering, seed, cps = cases.VIF_CASES[name]
        coords, y = cases.vif_data(name)
        cpred = np.random.default_rng(51).uniform(size=(25, d))
        mdl = refdrv.RefCAPIModel(coords, cf, sh, m, ordering, seed, threads=4, gp_approx="full_scale_vecchia", num_ind_points=k)
        cp = np.asarray(cps[0], dtype=np.float64)
        for tag, mp in (("m", m), ("2m", 2 * m)):
            mu, var = mdl.predict(cpred, predict_var=True, predict_response=True, vecchia_pred_type="order_obs_first_cond_obs_only", num_neighbors_pred=mp, y=y, cov_pars=cp)
            mu2, lvar = mdl.predict(cpred, predict_var=True, predict_response=False, vecchia_pred_type="order_obs_first_cond_obs_only", num_neighbors_pred=mp, y=y, cov_pars=cp)
            res["%s_%s_mu" % (name, tag)] = mu; res["%s_%s_var" % (name, tag)] = var; res["%s_%s_latent_var" % (name, tag)] = lvar
            if tag == "m":
                _, cov = mdl.predict(cpred, predict_response=True, vecchia_pred_type="order_obs_first_cond_obs_only", num_neighbors_pred=mp, y=y, cov_pars=cp, predict_cov_mat=True)
                res["%s_%s_cov" % (name, tag)] = cov
        print("vif pred", name, mu[:3], var[:3], lvar[:3], flush=True)
    np.savez_compressed(os.path.join(out_dir, "vif_pred_ref.npz"), **res)


def vif_pred_points(d):
    """40 prediction points of the VIF 'cond_all' fixture: 25 uniform ones and a tight cluster of 15 (so that prediction points are each other's neighbours)."""
    rng = np.random.default_rng(52)
    return np.vstack([rng.uniform(size=(25, d)), 0.37 + 0.02 * rng.uniform(size=(15, d))])


def vif_pred_condall_fixture(out_dir):
    """Round 5: the same for 'order_obs_first_cond_all' (neighbours among observed and preceding prediction points; the only other prediction type the
    reference has for full-scale Vecchia models, re_model_template.h:4057-4085): tests/golden/vif_pred_condall_ref.npz."""
    res = {}
    for name in VIF_FIT_CASES:
        n, d, cf, sh, m, k, ordering, seed, cps = cases.VIF_CASES[name]
        coords, y = cases.vif_data(name)
        cpred = vif_pred_points(d)
        mdl = refdrv.RefCAPIModel(coords, cf, sh, m, ordering, seed, threads=4, gp_approx="full_scale_vecchia", num_ind_points=k)
        cp = np.asarray(cps[0], dtype=np.float64)
        for tag, mp in (("m", m), ("2m", 2 * m)):
            mu, var = mdl.predict(cpred, predict_var=True, predict_response=True, vecchia_pred_type="order_obs_first_cond_all", num_neighbors_pred=mp, y=y, cov_pars=cp)
            mu2, lvar = mdl.predict(cpred, predict_var=True, predict_response=False, vecchia_pred_type="order_obs_first_cond_all", num_neighbors_pred=mp, y=y, cov_pars=cp)
            res["%s_%s_mu" % (name, tag)] = mu; res["%s_%s_var" % (name, tag)] = var; res["%s_%s_latent_var" % (name, tag)] = lvar
            if tag == "m":
                _, cov = mdl.predict(cpred, predict_response=True, vecchia_pred_type="order_obs_first_cond_all", num_neighbors_pred=mp, y=y, cov_pars=cp, predict_cov_mat=True)
                res["%s_%s_cov" % (name, tag)] = cov
        print("vif pred cond_all", name, mu[:3], var[:3], lvar[:3], flush=True)
    np.savez_compressed(os.path.join(out_dir, "vif_pred_condall_ref.npz"), **res)


def vif_fit_fixture(out_dir):
    """The unmodified reference's own lbfgs fits (its default optimiser, analytic gradient) of full-scale Vecchia models from the first
    parameter set of tests/cases.py:VIF_CASES (tests/golden/vif_fit_ref.npz)."""
    res = {}
    for name in VIF_FIT_CASES:
        n, d, cf, sh, m, k, ordering, seed, cps = cases.VIF_CASES[name]
        coords, y = cases.vif_data(name)
        mdl = refdrv.RefCAPIModel(coords, cf, sh, m, ordering, seed, threads=4, gp_approx="full_scale_vecchia", num_ind_points=k)
        mdl.set_optim_config(init_cov_pars=np.asarray(cps[0], dtype=np.float64), optimizer_cov="lbfgs")
        mdl.optim_cov_par(y)
        res[name + "_cov_pars"] = mdl.get_cov_par(3); res[name + "_num_it"] = np.int64(mdl.get_num_it())
        res[name + "_negll"] = np.float64(mdl.current_neg_log_likelihood())
        print("vif fit", name, res[name + "_cov_pars"], int(res[name + "_num_it"]), float(res[name + "_negll"]), flush=True)
    np.savez_compressed(os.path.join(out_dir, "vif_fit_ref.npz"), **res)


VIF_GRAD_CASES = ["vif_u2d_n1500_exp_m15_k40_none", "vif_u2d_n1500_exp_m15_k40_random", "vif_u2d_n3000_mat15_m30_k100_random",
                  "vif_u3d_n2000_mat25_m20_k64_random", "vif_u2d_n20000_exp_m30_k200_random", "vif_u2d_n100000_exp_m30_k200_random",
                  "vif_u2d_n1500_exp_m40_k50_random", "vif_u2d_n1500_mat15_m55_k60_random", "vif_u2d_n1200_exp_m70_k40_random"]
VIF_GRAD_PARS = [(0.1, 1.0, 0.1), (0.3, 0.6, 0.25)]


def vif_grad_fixture(out_dir, only=None):
    """Gradient of the full-scale Vecchia (VIF) likelihood by the unmodified reference (REModelTemplate::CalcGradPars ->
    CalcGradPars_FITC_FSA_GaussLikelihood_Cluster_i through oracle/ref_driver.cpp:refdrv_nll_grad -- the sequence of the L-BFGS functor) at
    VIF_GRAD_PARS for every case of VIF_GRAD_CASES: negll, the three gradient entries wrt the log of the transformed parameters
    (sigma2, sigma1_2 / sigma2, a) and, for n <= 3000, 200 sampled rows of the derivative factors dA / dD of both parameters
    (tests/golden/vif_grad_ref.npz)."""
    import time
    path = os.path.join(out_dir, "vif_grad_ref.npz")
    res = dict(np.load(path)) if os.path.exists(path) else {}
    for name in VIF_GRAD_CASES:
        if only and name not in only:
            continue
        n, d, cf, sh, m, k, ordering, seed, cps = cases.VIF_CASES[name]
        coords, y = cases.vif_data(name)
        mdl = refdrv.RefVifModel(coords, cf, sh, m, ordering, seed, num_ind_points=k, threads=8)
        for j, cp in enumerate(VIF_GRAD_PARS):
            t0 = time.time()
            nll, g, pt = mdl.nll_grad(y, np.asarray(cp, dtype=np.float64))
            res["%s_negll_%d" % (name, j)] = np.float64(nll); res["%s_grad_%d" % (name, j)] = g; res["%s_pars_trans_%d" % (name, j)] = pt
            if n <= 3000:
                rows = np.sort(np.random.default_rng(5).choice(n, size=200, replace=False))
                res["%s_rows" % name] = rows
                for p in range(2):
                    dA, dD = mdl.grad_factor(p)
                    res["%s_dA%d_%d" % (name, p, j)] = dA[rows]; res["%s_dD%d_%d" % (name, p, j)] = dD[rows]
            print("vif grad", name, cp, "negll = %.12f" % nll, g, "%.1f s" % (time.time() - t0), flush=True)
        del mdl
        np.savez_compressed(path, **res)


def vif_laplace_fixture(out_dir, only=None):
    """gp_approx = "full_scale_vecchia" with non-Gaussian likelihoods (tests/cases.py: VIF_LAPLACE_CASES): the unmodified reference's GPB_EvalNegLogLikelihood at
    cases.LAPLACE_TIGHT with the "fitc" (default), "vifdu" and "none" preconditioners (tests/golden/vif_laplace_ref.npz)."""
    import time
    path = os.path.join(out_dir, "vif_laplace_ref.npz")
    res = dict(np.load(path)) if os.path.exists(path) else {}
    for name, c in cases.VIF_LAPLACE_CASES.items():
        if only and name not in only:
            continue
        coords, y = cases.vif_laplace_data(name)
        for pc in ("fitc", "vifdu", "none"):
            if pc == "none" and c["lik"] not in ("bernoulli_logit", "poisson", "gamma"):
                continue                                                           # (hundreds of CG iterations per solve: the first three cases only)
            if pc == "vifdu" and c["lik"] in ("t", "lognormal", "gaussian_latent"):
                continue                                                           # (the reference build aborts in an Eigen assertion: its vifdu Woodbury factor is solved with before it is computed)
            for j, cp in enumerate(c["cov_pars"]):
                if pc != "fitc" and j > 0:
                    continue
                if pc != "fitc" and ("%s_%s_negll_%d" % (name, pc, j)) in res and os.environ.get("VIFL_REDO_ALL") is None:
                    continue                                                       # ("none" takes minutes: kept unless VIFL_REDO_ALL is set)
                mdl = refdrv.RefCAPIModel(coords, c["cov_function"], c["shape"], c["m"], c["ordering"], c["seed"], threads=8, likelihood=c["lik"],
                                          gp_approx="full_scale_vecchia", num_ind_points=c["k"], weights=cases.vif_laplace_weights(name))
                mdl.set_optim_config(cg_preconditioner_type=pc, piv_chol_rank=-999 if c["rank"] is None else c["rank"], init_aux_pars=c["aux"],
                                     **(cases.VIF_LAPLACE_TIGHT if pc == "fitc" else cases.LAPLACE_TIGHT))
                t0 = time.time()
                key = "%s_%s_negll_%d" % (name, pc, j)
                res[key] = np.float64(mdl.neg_log_likelihood(np.asarray(cp, dtype=np.float64), y))
                print("vif_laplace", name, pc, cp, "negll = %.12f" % res[key], "%.1f s" % (time.time() - t0), flush=True)
                del mdl
        np.savez_compressed(path, **res)


def vif_laplace_grad_fixture(out_dir, only=None):
    """The reference's own CalcGradPars for the cases of vif_laplace_fixture ("fitc" preconditioner, first parameter set; gamma: with the shape's component):
    keys <name>_fitc_grad_0, <name>_fitc_negll_direct_0 in tests/golden/vif_laplace_ref.npz."""
    path = os.path.join(out_dir, "vif_laplace_ref.npz")
    res = dict(np.load(path)) if os.path.exists(path) else {}
    for name, c in cases.VIF_LAPLACE_CASES.items():
        if only and name not in only:
            continue
        coords, y = cases.vif_laplace_data(name)
        v, g, vp = refdrv.ref_laplace_nll_grad(coords, y, c["cov_pars"][0], c["lik"], cov_function=c["cov_function"], shape=c["shape"], m=c["m"], ordering=c["ordering"],
                                               seed=c["seed"], threads=8, aux_pars=c["aux"], estimate_aux=c["aux"] is not None, cg_preconditioner_type="fitc", weights=cases.vif_laplace_weights(name),
                                               piv_chol_rank=-999 if c["rank"] is None else c["rank"], gp_approx="full_scale_vecchia", num_ind_points=c["k"],
                                               **cases.VIF_LAPLACE_TIGHT)
        res[name + "_fitc_grad_0"] = g; res[name + "_fitc_negll_direct_0"] = np.float64(v)
        if name.endswith("logit"):      # the boosting gradient d(-mll)/dF (REModel::CalcGradient) at fixed effects 0.3 cos(4 x_0), data order
            fe = 0.3 * np.cos(4 * coords[:, 0])
            res[name + "_gradF"] = refdrv.ref_laplace_grad_F(coords, y, c["cov_pars"][0], c["lik"], fixed_effects=fe, cov_function=c["cov_function"], shape=c["shape"], m=c["m"],
                                                             ordering=c["ordering"], seed=c["seed"], threads=8, cg_preconditioner_type="fitc",
                                                             piv_chol_rank=-999 if c["rank"] is None else c["rank"], gp_approx="full_scale_vecchia", num_ind_points=c["k"],
                                                             **cases.VIF_LAPLACE_TIGHT)
            res[name + "_gradF_fe"] = fe
        print("vif_laplace_grad", name, "negll = %.12f" % v, g, flush=True)
        np.savez_compressed(path, **res)


def vif_laplace_pred_points(c):
    rng = np.random.default_rng(777 + c["n"])
    return rng.uniform(size=(25, c["d"]))


def vif_laplace_pred_fixture(out_dir, only=None):
    """Predictions of VIF x non-Gaussian models at 25 new locations by the unmodified reference with matrix_inversion_method = "cholesky" (PredictLaplaceApproxFSVA's exact branch,
    likelihoods.h:8455-8527; its iterative branch estimates the variances by simulation): latent mean / variance and response mean / variance, keys <name>_pred_* in
    tests/golden/vif_laplace_ref.npz."""
    path = os.path.join(out_dir, "vif_laplace_ref.npz")
    res = dict(np.load(path)) if os.path.exists(path) else {}
    for name, c in cases.VIF_LAPLACE_CASES.items():
        if only and name not in only:
            continue
        coords, y = cases.vif_laplace_data(name)
        cpred = vif_laplace_pred_points(c)
        mdl = refdrv.RefCAPIModel(coords, c["cov_function"], c["shape"], c["m"], c["ordering"], c["seed"], threads=8, likelihood=c["lik"],
                                  gp_approx="full_scale_vecchia", num_ind_points=c["k"], matrix_inversion_method="cholesky", weights=cases.vif_laplace_weights(name))
        mdl.set_optim_config(init_aux_pars=c["aux"], cg_preconditioner_type="", **cases.LAPLACE_PRED_REF)
        cp = np.asarray(c["cov_pars"][0], dtype=np.float64)
        mu, var = mdl.predict(cpred, predict_var=True, predict_response=False, y=y, cov_pars=cp)
        rmu, rvar = mdl.predict(cpred, predict_var=True, predict_response=True, y=y, cov_pars=cp)
        res[name + "_pred_coords"] = cpred
        res[name + "_pred_latent_mu"] = mu; res[name + "_pred_latent_var"] = var
        res[name + "_pred_resp_mu"] = rmu; res[name + "_pred_resp_var"] = rvar
        if name.endswith("logit"):      # the latent predictive covariance matrix (likelihoods.h:8489-8504)
            res[name + "_pred_latent_cov"] = mdl.predict(cpred, predict_cov_mat=True, predict_response=False, y=y, cov_pars=cp)[1]
        if name.endswith("logit") or name.endswith("gamma"):      # 'latent_order_obs_first_cond_all': the prediction points condition on the preceding prediction points too
            mu2, var2 = mdl.predict(cpred, predict_var=True, predict_response=False, y=y, cov_pars=cp, vecchia_pred_type="latent_order_obs_first_cond_all")
            res[name + "_pred_condall_latent_mu"] = mu2; res[name + "_pred_condall_latent_var"] = var2
            if name.endswith("logit"):
                res[name + "_pred_condall_latent_cov"] = mdl.predict(cpred, predict_cov_mat=True, predict_response=False, y=y, cov_pars=cp,
                                                                     vecchia_pred_type="latent_order_obs_first_cond_all")[1]
        print("vif_laplace_pred", name, mu[:3], var[:3], rmu[:3], flush=True)
        np.savez_compressed(path, **res)


def vif_laplace_fit_fixture(out_dir, only=None):
    """The reference's own GPB_OptimCovPar on VIF x non-Gaussian models (tests/cases.py: VIF_LAPLACE_FITS): estimates, auxiliary parameter, iteration count, final value."""
    path = os.path.join(out_dir, "vif_laplace_ref.npz")
    res = dict(np.load(path)) if os.path.exists(path) else {}
    for fit, (name, cfg) in cases.VIF_LAPLACE_FITS.items():
        if only and fit not in only:
            continue
        c = cases.VIF_LAPLACE_CASES[name]
        coords, y = cases.vif_laplace_data(name)
        mdl = refdrv.RefCAPIModel(coords, c["cov_function"], c["shape"], c["m"], c["ordering"], c["seed"], threads=8, likelihood=c["lik"],
                                  gp_approx="full_scale_vecchia", num_ind_points=c["k"])
        kw = dict(cfg); kw["init_cov_pars"] = np.asarray(cfg["init_cov_pars"], dtype=np.float64)
        with_x = kw.pop("covariates", False)
        mdl.set_optim_config(cg_preconditioner_type="fitc", piv_chol_rank=-999 if c["rank"] is None else c["rank"], init_aux_pars=c["aux"], **cases.LAPLACE_TIGHT, **kw)
        if with_x:
            mdl.optim_lin_regr_coef_cov_par(y, cases.vif_laplace_covariates(coords))
            res[fit + "_coef"] = mdl.get_coef()
            # prediction with X_pred after that fit: latent mean (the iterative branch simulates the variances: not compared)
            cpred = vif_laplace_pred_points(c); Xp = cases.vif_laplace_covariates(cpred)
            res[fit + "_pred_coords"] = cpred
            res[fit + "_pred_latent_mu"] = mdl.predict(cpred, X_pred=Xp, predict_var=False, predict_response=False)[0]
        else:
            mdl.optim_cov_par(y)
        res[fit + "_cov_pars"] = mdl.get_cov_par(2)
        res[fit + "_num_it"] = np.int32(mdl.get_num_it())
        res[fit + "_negll"] = np.float64(mdl.current_neg_log_likelihood())
        if fit == "vifl_fit_logit_lbfgs":      # standard deviations of the covariance parameters (CalcStdDevCovParAuxParsNonGaussian: numerical Jacobian of the gradient)
            res[fit + "_cov_pars_sd"] = mdl.get_cov_par(2, std_dev=True)[2:]
        if c["aux"] is not None:
            res[fit + "_aux"] = mdl.get_aux_pars(1)
        print("vif_laplace_fit", fit, res[fit + "_cov_pars"], res[fit + "_num_it"], res[fit + "_negll"], res.get(fit + "_aux"), flush=True)
        np.savez_compressed(path, **res)


def weights_fixture(out_dir, only=None):
    """Sample weights (Gaussian Vecchia model): the unmodified reference's likelihood values, lbfgs fit and predictions after the fit on
    tests/cases.py:WEIGHT_CASES (tests/golden/weights_ref.npz)."""
    path = os.path.join(out_dir, "weights_ref.npz")
    res = dict(np.load(path)) if os.path.exists(path) else {}
    for name, (n, d, cf, sh, m, ordering, seed) in cases.WEIGHT_CASES.items():
        if only and name not in only:
            continue
        coords, y, w, cpred = cases.weight_data(name)
        mdl = refdrv.RefCAPIModel(coords, cf, sh, m, ordering, seed, threads=1, weights=w)
        for j, cp in enumerate(cases.WEIGHT_COV_PARS):
            res["%s_negll_%d" % (name, j)] = np.float64(mdl.neg_log_likelihood(np.asarray(cp, dtype=np.float64), y))
        mdl.set_optim_config(init_cov_pars=np.asarray(cases.WEIGHT_COV_PARS[0], dtype=np.float64), optimizer_cov="lbfgs")
        mdl.optim_cov_par(y)
        res[name + "_fit_cov_pars"] = mdl.get_cov_par(3); res[name + "_fit_num_it"] = np.int64(mdl.get_num_it())
        res[name + "_fit_negll"] = np.float64(mdl.current_neg_log_likelihood())
        for pt in ("order_obs_first_cond_obs_only", "order_obs_first_cond_all") + tuple(cases.PRED_TYPES):
            mu, var = mdl.predict(cpred, predict_var=True, predict_response=True, vecchia_pred_type=pt, num_neighbors_pred=m)
            res["%s_pred_%s_mu" % (name, pt)] = mu; res["%s_pred_%s_var" % (name, pt)] = var
        print("weights", name, [float(res["%s_negll_%d" % (name, j)]) for j in range(2)], res[name + "_fit_cov_pars"], int(res[name + "_fit_num_it"]), flush=True)
        del mdl
        np.savez_compressed(path, **res)


def predtypes_fixture(out_dir, only=None):
    """'order_pred_first' and the two 'latent_*' prediction types of the Gaussian Vecchia model: the unmodified reference's predictive means,
    covariance matrices (response scale) and latent variances on tests/cases.py:PREDTYPE_CASES (tests/golden/predtypes_ref.npz)."""
    path = os.path.join(out_dir, "predtypes_ref.npz")
    res = dict(np.load(path)) if os.path.exists(path) else {}
    for name, (n, d, cf, sh, m, ordering, seed, npred, mpred, cp) in cases.PREDTYPE_CASES.items():
        if only and name not in only:
            continue
        coords, y, cpred = cases.predtype_data(name)
        mdl = refdrv.RefCAPIModel(coords, cf, sh, m, ordering, seed, threads=1)
        for pt in cases.PRED_TYPES:
            mu, cov = mdl.predict(cpred, predict_response=True, vecchia_pred_type=pt, num_neighbors_pred=mpred, y=y, cov_pars=np.asarray(cp, dtype=np.float64),
                                  predict_cov_mat=True)
            mu2, var = mdl.predict(cpred, predict_response=False, predict_var=True, vecchia_pred_type=pt, num_neighbors_pred=mpred, y=y,
                                   cov_pars=np.asarray(cp, dtype=np.float64))
            res["%s_%s_mu" % (name, pt)] = mu; res["%s_%s_cov" % (name, pt)] = cov; res["%s_%s_latent_var" % (name, pt)] = var
            assert np.allclose(mu, mu2, rtol=1e-9, atol=1e-12)
            print("predtypes", name, pt, mu[:3], np.diag(cov)[:3], var[:3], flush=True)
        del mdl
        np.savez_compressed(path, **res)


EXACT_FISHER_CASES = [(400, 2, "matern", 1.5), (300, 3, "matern", 2.5), (500, 2, "exponential", 0.5)]


def exact_fisher_fixture(out_dir):
    """Standard errors of the exact GP's covariance parameters (gp_approx = "none": GPB_GetCovPar(calc_std_dev = true), dense
    CalcFisherInformation) of the unmodified reference after two gradient steps from (0.5, 0.8, 0.2) on cases.synthetic(n, d, seed = n)
    (tests/golden/exact_fisher_ref.npz)."""
    res = {}
    for (n, d, cf, sh) in EXACT_FISHER_CASES:
        c2, y2 = cases.synthetic(n, d, seed=n)
        mdl = refdrv.RefCAPIModel(c2, cf, sh, 30, "none", 1, threads=4, gp_approx="none")
        mdl.set_optim_config(init_cov_pars=np.array([0.5, 0.8, 0.2]), max_iter=2, optimizer_cov="gradient_descent")
        mdl.optim_cov_par(y2)
        v = mdl.get_cov_par(3, std_dev=True)
        key = "n%d_d%d_%s_%g" % (n, d, cf, sh)
        res[key + "_cov_pars"] = v[:3]; res[key + "_std"] = v[3:]
        print("exact fisher", key, v, flush=True)
    np.savez_compressed(os.path.join(out_dir, "exact_fisher_ref.npz"), **res)


def pred_first_perm_fixture(out_dir):
    """'order_pred_first' on SCATTERED prediction points (sparse conditional precision): the unmodified reference's mean, variances and
    covariance matrix -- the latter two come back in the order of its sparse Cholesky's fill-reducing permutation
    (tests/golden/pred_first_perm_ref.npz; tests/test_predtypes.py::test_reference_orders_pred_first_variances_by_its_cholesky_permutation)."""
    n, d = 1500, 2
    coords, _ = cases.synthetic(n, d, seed=5)
    y = np.sin(4 * coords[:, 0]) + 0.3 * np.random.default_rng(6).standard_normal(n)
    cpred = np.random.default_rng(7).uniform(size=(40, d))
    cp = np.array([0.1, 1.0, 0.1])
    mdl = refdrv.RefCAPIModel(coords, "exponential", 0.5, 15, "none", 1, threads=1)
    mu, cov = mdl.predict(cpred, predict_response=True, vecchia_pred_type="order_pred_first", num_neighbors_pred=15, y=y, cov_pars=cp, predict_cov_mat=True)
    np.savez_compressed(os.path.join(out_dir, "pred_first_perm_ref.npz"), mu=mu, cov=cov)
    print("pred_first_perm", mu[:3], np.diag(cov)[:3], flush=True)


def train_re_fixture(out_dir):
    """Posterior mean and variance of the latent GP at the training locations (GPB_PredictREModelTrainingDataRandomEffects with calc_var) of
    the unmodified reference on tests/cases.py:PREDTYPE_CASES (tests/golden/train_re_ref.npz)."""
    res = {}
    for name, (n, d, cf, sh, m, ordering, seed, npred, mpred, cp) in cases.PREDTYPE_CASES.items():
        coords, y, _ = cases.predtype_data(name)
        mdl = refdrv.RefCAPIModel(coords, cf, sh, m, ordering, seed, threads=1)
        mu, var = mdl.predict_training_data_random_effects(y, np.asarray(cp, dtype=np.float64), True)
        res[name + "_mu"] = mu; res[name + "_var"] = var
        print("train_re", name, mu[:3], var[:3], flush=True)
    np.savez_compressed(os.path.join(out_dir, "train_re_ref.npz"), **res)


EXACT_PRED_CASES = [(400, 2, "matern", 1.5, (0.3, 0.9, 0.15)), (300, 3, "matern", 2.5, (0.2, 1.1, 0.3)), (500, 2, "exponential", 0.5, (0.05, 1.5, 0.1))]


def exact_pred_fixture(out_dir):
    """Predictive mean and covariance matrix (response scale) and latent variances of the exact GP (gp_approx = "none") of the unmodified
    reference at given parameters: cases.synthetic(n, d, seed = n), 25 prediction points default_rng(43).uniform(0.2, 0.8)
    (tests/golden/exact_pred_ref.npz)."""
    res = {}
    for (n, d, cf, sh, cp) in EXACT_PRED_CASES:
        c2, y2 = cases.synthetic(n, d, seed=n)
        cpred = np.random.default_rng(43).uniform(0.2, 0.8, size=(25, d))
        mdl = refdrv.RefCAPIModel(c2, cf, sh, 30, "none", 1, threads=4, gp_approx="none")
        key = "n%d_d%d_%s_%g" % (n, d, cf, sh)
        mu, cov = mdl.predict(cpred, predict_response=True, y=y2, cov_pars=np.asarray(cp, dtype=np.float64), predict_cov_mat=True)
        mu2, var = mdl.predict(cpred, predict_response=False, predict_var=True, y=y2, cov_pars=np.asarray(cp, dtype=np.float64))
        res[key + "_mu"] = mu; res[key + "_cov"] = cov; res[key + "_latent_var"] = var
        tmu, tvar = mdl.predict_training_data_random_effects(y2, np.asarray(cp, dtype=np.float64), True)       # PredictTrainingDataRandomEffects, dense branch
        res[key + "_train_mu"] = tmu; res[key + "_train_var"] = tvar
        print("exact pred", key, mu[:3], np.diag(cov)[:3], var[:3], flush=True)
    np.savez_compressed(os.path.join(out_dir, "exact_pred_ref.npz"), **res)


def config4_fixture(out_dir):
    """BASELINE config 4 at its full size: ONE reference evaluation (n = 1e5, m = 30, Bernoulli-logit, iterative methods, vadu) --
    tests/golden/config4_ref.npz.  ~30 s on 8 cores."""
    import time
    n, m = 100000, 30
    coords, y = cases.synthetic_binary(n, 2, seed=1)
    mdl = refdrv.RefCAPIModel(coords, "exponential", 0.5, m, "random", 1, threads=8, likelihood="bernoulli_logit")
    res = {}
    for k, cp in enumerate([(1.0, 0.1)]):
        t0 = time.time()
        res["negll_%d" % k] = np.float64(mdl.neg_log_likelihood(np.asarray(cp, dtype=np.float64), y))
        res["seconds_%d" % k] = np.float64(time.time() - t0)
        print("config4", cp, "negll = %.12f" % res["negll_%d" % k], "%.1f s" % res["seconds_%d" % k], flush=True)
    # the same evaluation with the CG stopping threshold tightened from the default 1e-2 to 1e-6: the value no longer hinges on which
    # iteration a rounded residual norm crosses the threshold, so two correct implementations agree far below 1e-8
    mdl.set_optim_config(cg_delta_conv=1e-6)
    t0 = time.time()
    res["negll_tight_0"] = np.float64(mdl.neg_log_likelihood(np.asarray((1.0, 0.1), dtype=np.float64), y))
    res["seconds_tight_0"] = np.float64(time.time() - t0)
    print("config4 cg_delta_conv=1e-6 negll = %.12f" % res["negll_tight_0"], "%.1f s" % res["seconds_tight_0"], flush=True)
    np.savez_compressed(os.path.join(out_dir, "config4_ref.npz"), **res)


def config4_pivchol_fixture(out_dir):
    """BASELINE config 4's data (n = 1e5, m = 30, Bernoulli-logit) with cg_preconditioner_type = "pivoted_cholesky" (rank 50): ONE reference evaluation at the default
    thresholds and one at cg_delta_conv = 1e-6 -- tests/golden/config4_pivchol_ref.npz."""
    import time
    n, m = 100000, 30
    coords, y = cases.synthetic_binary(n, 2, seed=1)
    res = {}
    for key, cfg in (("negll_0", {}), ("negll_tight_0", dict(cg_delta_conv=1e-6))):
        mdl = refdrv.RefCAPIModel(coords, "exponential", 0.5, m, "random", 1, threads=8, likelihood="bernoulli_logit")
        mdl.set_optim_config(cg_preconditioner_type="pivoted_cholesky", **cfg)
        t0 = time.time()
        res[key] = np.float64(mdl.neg_log_likelihood(np.asarray((1.0, 0.1), dtype=np.float64), y))
        res["seconds_" + key] = np.float64(time.time() - t0)
        print("config4 pivoted_cholesky", key, "negll = %.12f" % res[key], "%.1f s" % res["seconds_" + key], flush=True)
    np.savez_compressed(os.path.join(out_dir, "config4_pivchol_ref.npz"), **res)


def config4_vresp_fixture(out_dir):
    """BASELINE config 4's data with cg_preconditioner_type = "vecchia_response": ONE reference evaluation at the default thresholds and one at cg_delta_conv = 1e-6, with the
    reference's wall-clock seconds on this container's 8 cores -- tests/golden/config4_vresp_ref.npz."""
    import time
    n, m = 100000, 30
    coords, y = cases.synthetic_binary(n, 2, seed=1)
    res = {}
    for key, cfg in (("negll_0", {}), ("negll_tight_0", dict(cg_delta_conv=1e-6))):
        mdl = refdrv.RefCAPIModel(coords, "exponential", 0.5, m, "random", 1, threads=8, likelihood="bernoulli_logit")
        mdl.set_optim_config(cg_preconditioner_type="vecchia_response", **cfg)
        t0 = time.time()
        res[key] = np.float64(mdl.neg_log_likelihood(np.asarray((1.0, 0.1), dtype=np.float64), y))
        res["seconds_" + key] = np.float64(time.time() - t0)
        print("config4 vecchia_response", key, "negll = %.12f" % res[key], "%.1f s" % res["seconds_" + key], flush=True)
    np.savez_compressed(os.path.join(out_dir, "config4_vresp_ref.npz"), **res)


if __name__ == "__main__":
    if len(sys.argv) > 1 and sys.argv[1] == "config4_pivchol":
        config4_pivchol_fixture(os.path.join(ROOT, "tests", "golden"))
    elif len(sys.argv) > 1 and sys.argv[1] == "config4_vresp":
        config4_vresp_fixture(os.path.join(ROOT, "tests", "golden"))
    elif len(sys.argv) > 1 and sys.argv[1] == "atsize":
        atsize_fixture(os.path.join(ROOT, "tests", "golden"), sys.argv[2:])
    elif len(sys.argv) > 1 and sys.argv[1] == "weights":
        weights_fixture(os.path.join(ROOT, "tests", "golden"), sys.argv[2:])
    elif len(sys.argv) > 1 and sys.argv[1] == "exact_pred":
        exact_pred_fixture(os.path.join(ROOT, "tests", "golden"))
    elif len(sys.argv) > 1 and sys.argv[1] == "vif_pred":
        vif_pred_fixture(os.path.join(ROOT, "tests", "golden"))
    elif len(sys.argv) > 1 and sys.argv[1] == "vif_pred_condall":
        vif_pred_condall_fixture(os.path.join(ROOT, "tests", "golden"))
    elif len(sys.argv) > 1 and sys.argv[1] == "vif_fit":
        vif_fit_fixture(os.path.join(ROOT, "tests", "golden"))
    elif len(sys.argv) > 1 and sys.argv[1] == "laplace_dup_gradF":
        laplace_dup_gradF_fixture(os.path.join(ROOT, "tests", "golden"))
    elif len(sys.argv) > 1 and sys.argv[1] == "laplace_coef":
        laplace_coef_fixture(os.path.join(ROOT, "tests", "golden"))
    elif len(sys.argv) > 1 and sys.argv[1] == "laplace_stderr":
        laplace_stderr_fixture(os.path.join(ROOT, "tests", "golden"))
    elif len(sys.argv) > 1 and sys.argv[1] == "laplace_train_re":
        laplace_train_re_fixture(os.path.join(ROOT, "tests", "golden"))
    elif len(sys.argv) > 1 and sys.argv[1] == "laplace_predvar":
        laplace_predvar_fixture(os.path.join(ROOT, "tests", "golden"))
    elif len(sys.argv) > 1 and sys.argv[1] == "laplace_dup":
        laplace_dup_fixture(os.path.join(ROOT, "tests", "golden"))
    elif len(sys.argv) > 1 and sys.argv[1] == "pred_first_perm":
        pred_first_perm_fixture(os.path.join(ROOT, "tests", "golden"))
    elif len(sys.argv) > 1 and sys.argv[1] == "train_re":
        train_re_fixture(os.path.join(ROOT, "tests", "golden"))
    elif len(sys.argv) > 1 and sys.argv[1] == "exact_fisher":
        exact_fisher_fixture(os.path.join(ROOT, "tests", "golden"))
    elif len(sys.argv) > 1 and sys.argv[1] == "predtypes":
        predtypes_fixture(os.path.join(ROOT, "tests", "golden"), sys.argv[2:])
    elif len(sys.argv) > 1 and sys.argv[1] == "vif_grad":
        vif_grad_fixture(os.path.join(ROOT, "tests", "golden"), sys.argv[2:])
    elif len(sys.argv) > 1 and sys.argv[1] == "vif_laplace_pred":
        vif_laplace_pred_fixture(os.path.join(ROOT, "tests", "golden"), sys.argv[2:])
    elif len(sys.argv) > 1 and sys.argv[1] == "vif_laplace_fit":
        vif_laplace_fit_fixture(os.path.join(ROOT, "tests", "golden"), sys.argv[2:])
    elif len(sys.argv) > 1 and sys.argv[1] == "vif_laplace_grad":
        vif_laplace_grad_fixture(os.path.join(ROOT, "tests", "golden"), sys.argv[2:])
    elif len(sys.argv) > 1 and sys.argv[1] == "vif_laplace":
        vif_laplace_fixture(os.path.join(ROOT, "tests", "golden"), sys.argv[2:])
    elif len(sys.argv) > 1 and sys.argv[1] == "vif":
        vif_fixture(os.path.join(ROOT, "tests", "golden"), sys.argv[2:])
    elif len(sys.argv) > 1 and sys.argv[1] == "config4":
        config4_fixture(os.path.join(ROOT, "tests", "golden"))
    elif len(sys.argv) > 1 and sys.argv[1] == "laplace":     # only (re)generate the Laplace fixture
        laplace_fixture(os.path.join(ROOT, "tests", "golden"))
    elif len(sys.argv) > 1 and sys.argv[1] == "laplace_pred":
        laplace_pred_fixture(os.path.join(ROOT, "tests", "golden"))
    elif len(sys.argv) > 1 and sys.argv[1] == "laplace_grad_F":
        laplace_grad_F_fixture(os.path.join(ROOT, "tests", "golden"))
    elif len(sys.argv) > 1 and sys.argv[1] == "fisher":
        fisher_fixture(os.path.join(ROOT, "tests", "golden"))
    elif len(sys.argv) > 1 and sys.argv[1] == "optim_laplace":
        optim_laplace_fixture(os.path.join(ROOT, "tests", "golden"))
    elif len(sys.argv) > 1 and sys.argv[1] == "laplace_weights":
        laplace_weights_fixture(os.path.join(ROOT, "tests", "golden"))
    elif len(sys.argv) > 1 and sys.argv[1] == "laplace_pc_extra":
        laplace_pc_extra_fixture(os.path.join(ROOT, "tests", "golden"))
    elif len(sys.argv) > 1 and sys.argv[1] == "laplace_t":
        laplace_t_fixture(os.path.join(ROOT, "tests", "golden"))
    elif len(sys.argv) > 1 and sys.argv[1] == "laplace_pred_refresh":
        laplace_pred_refresh(os.path.join(ROOT, "tests", "golden"))
    elif len(sys.argv) > 1 and sys.argv[1] == "laplace_aux_se":
        laplace_aux_se_fixture(os.path.join(ROOT, "tests", "golden"))
    elif len(sys.argv) > 1 and sys.argv[1] == "laplace_coef_weights":
        laplace_coef_weights_fixture(os.path.join(ROOT, "tests", "golden"))
    elif len(sys.argv) > 1 and sys.argv[1] == "laplace_t_fixdf":
        laplace_t_fixdf_fixture(os.path.join(ROOT, "tests", "golden"))
    elif len(sys.argv) > 1 and sys.argv[1] == "laplace_aux_gd":
        laplace_aux_gd_fixture(os.path.join(ROOT, "tests", "golden"))
    elif len(sys.argv) > 1 and sys.argv[1] == "laplace_vresp":
        laplace_vresp_fixture(os.path.join(ROOT, "tests", "golden"))
    elif len(sys.argv) > 1 and sys.argv[1] == "laplace_pivchol_probes":
        laplace_pivchol_probes_fixture(os.path.join(ROOT, "tests", "golden"))
    elif len(sys.argv) > 1 and sys.argv[1] == "laplace_pivchol":
        laplace_pivchol_fixture(os.path.join(ROOT, "tests", "golden"), sys.argv[2:])
    elif len(sys.argv) > 1 and sys.argv[1] == "laplace_aux":
        laplace_aux_fixture(os.path.join(ROOT, "tests", "golden"), sys.argv[2:])
    elif len(sys.argv) > 1 and sys.argv[1] == "laplace_grad":
        laplace_grad_fixture(os.path.join(ROOT, "tests", "golden"))
    elif len(sys.argv) > 1 and sys.argv[1] == "optim_coef":
        optim_coef_fixture(os.path.join(ROOT, "tests", "golden"))
    elif len(sys.argv) > 1 and sys.argv[1] == "optim":
        optim_fixture(os.path.join(ROOT, "tests", "golden"))
    elif len(sys.argv) > 1 and sys.argv[1] == "tree":
        tree_fixture(os.path.join(ROOT, "tests", "golden"))
    elif len(sys.argv) > 1 and sys.argv[1] == "split":
        split_fixture(os.path.join(ROOT, "tests", "golden"))
    elif len(sys.argv) > 1 and sys.argv[1] == "split_cat":
        split_cat_fixture(os.path.join(ROOT, "tests", "golden"))
    elif len(sys.argv) > 1 and sys.argv[1] == "clusters":
        cluster_fixture(os.path.join(ROOT, "tests", "golden"))
    elif len(sys.argv) > 1 and sys.argv[1] == "hist":
        hist_fixture(os.path.join(ROOT, "tests", "golden"))
    else:
        main()
