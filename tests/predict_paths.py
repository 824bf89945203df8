"""Case table of tests/test_zz_predict_paths_gpu.py: small predictions through the C entry points GPB_PredictREModel, GPB_SetPredictionData and
GPB_PredictREModelTrainingDataRandomEffects that take every model path of gpboost_amd/csrc/gpb_predict.inc (full-scale Vecchia, Vecchia-Laplace with and without
inducing points, exact GP, clusters, the one-cluster Gaussian Vecchia model with its five prediction types), every refusal those paths can produce, and for each path one
call that meets two refusals at once, so the order of the checks is part of the record.

Every case is a function () -> {field: float64 array | message}.  Base data: n = 300 points in the unit square (cases.synthetic), 10 neighbours, Matern-1.5 at fixed
covariance parameters; 12 prediction points, six of them inside a disc of radius 0.01, so that with num_neighbors_pred = 8 the 'cond_all' types take prediction points
as neighbours (checked by case "gv-types": their variances differ from those of the 'cond_obs_only' types).  The Laplace cases repeat three prediction locations.

The recording is NOT a test: `python -m tests.predict_paths record OUT.npz` runs the table once on whatever library GPBOOST_AMD_LIB selects and writes the fields;
`merge DST.npz A.npz B.npz ...` puts several such files (separate processes) together: a field they all agree on bit for bit is stored once and compared exactly, any other
gets the first run's value and "<key>@spread", the largest absolute difference between two runs.  Cases that the CPU restatement of the shim refuses ("is not restated on
the CPU") are left out of a recording made on it."""
import ctypes as C
import os
import platform
import subprocess
import sys

import numpy as np

N, M, NNP, NP = 300, 10, 8, 12
COV3 = np.array([0.3, 1.2, 0.15])          # error variance, GP variance, range
COV2 = np.array([1.2, 0.15])               # GP variance, range (non-Gaussian models)
TYPES = ("order_obs_first_cond_obs_only", "order_obs_first_cond_all", "order_pred_first", "latent_order_obs_first_cond_obs_only", "latent_order_obs_first_cond_all")
LTYPES = ("latent_order_obs_first_cond_obs_only", "latent_order_obs_first_cond_all")


def data(n=N):
    from tests import cases
    co, y = cases.synthetic(n, 2)
    rng = np.random.default_rng(5)
    cp = rng.uniform(size=(NP, 2))
    ang, rad = rng.uniform(0, 2 * np.pi, 6), 0.01 * np.sqrt(rng.uniform(size=6))
    cp[6:] = np.array([0.5, 0.5]) + np.c_[rad * np.cos(ang), rad * np.sin(ang)]
    cpd = cp.copy()
    cpd[[9, 10, 11]] = cp[[0, 1, 6]]         # three repeated prediction locations
    f = 1.2 * np.sin(5 * co[:, 0]) * np.cos(3 * co[:, 1])
    cod = co.copy()
    cod[2 * n // 3:] = co[:n - 2 * n // 3]    # repeated training locations: the last third repeats the first
    return dict(coords=co, y=y, cp=cp, cpd=cpd, coords_dup=cod, fe=0.5 * np.cos(4 * co[:, 0]), fep=0.5 * np.cos(4 * cp[:, 0]),
                X=np.c_[np.ones(n), np.sin(3 * co[:, 0] + co[:, 1])], Xp=np.c_[np.ones(NP), np.sin(3 * cp[:, 0] + cp[:, 1])],
                w=rng.uniform(0.5, 2.0, size=n), ids=(10 + (np.arange(n) % 2)).astype(np.int32),
                ids_pred=np.array([10, 11, 12, 12, 10, 11, 12, 12, 10, 11, 12, 12], dtype=np.int32),
                y01=(rng.uniform(size=n) < 1.0 / (1.0 + np.exp(-f))).astype(np.float64), ycount=rng.poisson(np.exp(0.5 * f)).astype(np.float64),
                ypos=np.exp(0.5 * f) * rng.gamma(2.0, 0.5, size=n))


def model(d, likelihood="gaussian", gp_approx="vecchia", coords=None, **kw):
    import gpboost_amd as gpb
    if gp_approx == "full_scale_vecchia":
        kw.setdefault("num_ind_points", 20)
    if gp_approx != "none":
        kw.setdefault("num_neighbors", M)
    return gpb.GPModel(likelihood=likelihood, gp_coords=d["coords"] if coords is None else coords, cov_function="matern", cov_fct_shape=1.5, gp_approx=gp_approx,
                       vecchia_ordering="random", seed=1, **kw)


def put(out, tag, fn):
    """Runs one call; stores its arrays under tag + name, or the message of the error it raised under tag + 'error'."""
    from gpboost_amd.basic import GPBoostError
    try:
        res = fn()
    except GPBoostError as e:
        out[tag + "error"] = str(e)
        return None
    if isinstance(res, dict):
        for k, v in res.items():
            if v is not None:
                out[tag + k] = np.asarray(v, dtype=np.float64)
    else:
        out[tag + "out"] = np.asarray(res, dtype=np.float64)
    return res


def raw_predict(mdl, npred, coords_pred=None, y=None, cov_pars=None, cov=False, var=False, response=True, sample_posterior=False, sample_prior=False,
                foreign=False, X_pred=None, use_saved_data=False, cluster_ids_pred=None):
    """GPB_PredictREModel with arguments GPModel.predict does not pass on (samples, grouped-effects data) or checks itself (counts, X_pred without a fit)."""
    from gpboost_amd.basic import _lib, _safe_call, _dptr
    keep = [np.asfortranarray(a, dtype=np.float64) if a is not None else None for a in (coords_pred, y, cov_pars, X_pred)]
    ptr = [C.c_void_p() if a is None else _dptr(a) for a in keep]
    cid = None if cluster_ids_pred is None else np.ascontiguousarray(cluster_ids_pred, dtype=np.int32)
    out = np.zeros(npred * (1 + npred) if 0 < npred <= 64 else 8)      # (a count above 64 is a limit case: refused before anything is written)
    dummy = np.zeros(8)
    _safe_call(_lib().GPB_PredictREModel(
        mdl.handle, ptr[1], C.c_int(npred), _dptr(out), C.c_bool(cov), C.c_bool(var), C.c_bool(response), C.c_bool(sample_posterior), C.c_bool(sample_prior),
        C.c_int(0), C.c_int(0), C.c_void_p() if cid is None else cid.ctypes.data_as(C.c_void_p), C.c_void_p(), _dptr(dummy) if foreign else C.c_void_p(), ptr[0],
        C.c_void_p(), ptr[2], ptr[3], C.c_bool(use_saved_data), C.c_void_p(), C.c_void_p()))
    return out


def common_refusals(out, d, mk, cov_pars, y, **kw):
    """The refusals every path shares, on one model that no call has given a response or covariance parameters; kw: what the path needs to get that far
    (the cluster path: cluster ids; the non-Gaussian path: the latent scale, whose covariance matrix is not refused by itself)."""
    m = mk()
    cp = d["cp"]
    put(out, "samples/", lambda: raw_predict(m, NP, cp, y, cov_pars, sample_posterior=True, **kw))
    put(out, "cov+var/", lambda: raw_predict(m, NP, cp, y, cov_pars, cov=True, var=True, **kw))
    put(out, "foreign/", lambda: raw_predict(m, NP, cp, y, cov_pars, foreign=True, **kw))
    put(out, "no-coords/", lambda: raw_predict(m, NP, None, y, cov_pars, **kw))
    put(out, "no-coords-saved/", lambda: raw_predict(m, 0, None, y, cov_pars, use_saved_data=True, **kw))
    put(out, "no-response/", lambda: raw_predict(m, NP, cp, None, cov_pars, **kw))
    put(out, "no-cov-pars/", lambda: raw_predict(m, NP, cp, y, None, **kw))
    # two conditions at once: which refusal comes first is part of the record
    put(out, "samples&cov+var/", lambda: raw_predict(m, NP, cp, y, cov_pars, cov=True, var=True, sample_prior=True, **kw))
    put(out, "cov+var&foreign/", lambda: raw_predict(m, NP, cp, y, cov_pars, cov=True, var=True, foreign=True, **kw))
    put(out, "foreign&no-coords/", lambda: raw_predict(m, NP, None, y, cov_pars, foreign=True, **kw))
    put(out, "no-coords&no-response/", lambda: raw_predict(m, NP, None, None, cov_pars, **kw))
    put(out, "no-response&no-cov-pars/", lambda: raw_predict(m, NP, cp, None, None, **kw))
    return m


# ---- one-cluster Gaussian Vecchia model ----------------------------------------------------------------------------------------------------------------

def case_gv_types():
    d = data()
    m = model(d)
    out = {}
    for t in TYPES:
        kw = dict(y=d["y"], gp_coords_pred=d["cp"], cov_pars=COV3, vecchia_pred_type=t, num_neighbors_pred=NNP)
        put(out, t + "/mean/", lambda: m.predict(predict_response=True, **kw))
        put(out, t + "/var-latent/", lambda: m.predict(predict_var=True, predict_response=False, **kw))
        put(out, t + "/cov-response/", lambda: m.predict(predict_cov_mat=True, predict_response=True, **kw))
    # prediction points really are neighbours of prediction points
    assert not np.array_equal(out[TYPES[0] + "/var-latent/var"], out[TYPES[1] + "/var-latent/var"])
    assert not np.array_equal(out[TYPES[3] + "/var-latent/var"], out[TYPES[4] + "/var-latent/var"])
    return out


def case_gv_arguments():
    d = data()
    out = {}
    m = model(d)
    put(out, "offset/", lambda: m.predict(y=d["y"], gp_coords_pred=d["cp"], cov_pars=COV3, predict_var=True, offset=d["fe"], offset_pred=d["fep"],
                                          vecchia_pred_type=TYPES[1], num_neighbors_pred=NNP))
    m.set_prediction_data(gp_coords_pred=d["cp"], vecchia_pred_type=TYPES[2], num_neighbors_pred=NNP)
    put(out, "saved/", lambda: m.predict(y=d["y"], cov_pars=COV3, predict_var=True, use_saved_data=True))
    m2 = model(d)
    m2.neg_log_likelihood(cov_pars=COV3, y=d["y"], fixed_effects=d["fe"])
    put(out, "y-none/", lambda: m2.predict(gp_coords_pred=d["cp"], cov_pars=COV3, predict_var=True, vecchia_pred_type=TYPES[0], num_neighbors_pred=NNP))
    put(out, "y-none-offset/", lambda: m2.predict(gp_coords_pred=d["cp"], cov_pars=COV3, predict_var=True, offset=d["fe"]))
    for t in TYPES[:3]:
        put(out, "nnp200/" + t + "/", lambda: m.predict(y=d["y"], gp_coords_pred=d["cp"], cov_pars=COV3, predict_var=True, vecchia_pred_type=t, num_neighbors_pred=200))
    return out


def case_gv_weights():
    """sample weights: a nugget per point (not restated on the CPU)"""
    d = data()
    mw = model(d, weights=d["w"])
    out = {}
    for t in LTYPES:
        put(out, t + "/", lambda: mw.predict(y=d["y"], gp_coords_pred=d["cp"], cov_pars=COV3, predict_var=True, vecchia_pred_type=t, num_neighbors_pred=NNP))
    put(out, TYPES[1] + "/", lambda: mw.predict(y=d["y"], gp_coords_pred=d["cp"], cov_pars=COV3, predict_cov_mat=True, vecchia_pred_type=TYPES[1], num_neighbors_pred=NNP))
    return out


def case_gv_covariates():
    d = data()
    m = model(d)
    m.fit(d["y"] + d["X"] @ np.array([0.5, -1.0]), X=d["X"], params=dict(maxit=3, init_cov_pars=COV3))
    out = {"cov_pars": np.asarray(m.get_cov_pars(), dtype=np.float64), "coef": np.asarray(m.get_coef(), dtype=np.float64)}
    for t in TYPES[:2] + TYPES[3:4]:
        put(out, t + "/", lambda: m.predict(gp_coords_pred=d["cp"], X_pred=d["Xp"], predict_var=True, vecchia_pred_type=t, num_neighbors_pred=NNP))
    put(out, "cov/", lambda: m.predict(gp_coords_pred=d["cp"], X_pred=d["Xp"], predict_cov_mat=True, vecchia_pred_type=TYPES[1], offset_pred=d["fep"]))
    put(out, "missing/", lambda: raw_predict(m, NP, d["cp"]))
    put(out, "saved/", lambda: raw_predict(m, NP, d["cp"], X_pred=d["Xp"], use_saved_data=True))
    put(out, "missing&saved/", lambda: raw_predict(m, NP, d["cp"], use_saved_data=True))
    put(out, "train-re/", lambda: m.predict_training_data_random_effects(predict_var=True))
    return out


def case_gv_refusals():
    d = data()
    out = {}
    m = common_refusals(out, d, lambda: model(d), COV3, d["y"])
    put(out, "superfluous/", lambda: raw_predict(m, NP, d["cp"], d["y"], COV3, X_pred=d["Xp"]))
    put(out, "superfluous&no-coords/", lambda: raw_predict(m, NP, None, d["y"], COV3, X_pred=d["Xp"]))
    put(out, "type/", lambda: m.set_prediction_data(vecchia_pred_type="order_obs_last"))
    put(out, "set-foreign/", lambda: _set_prediction_data_covariates(m, d))
    put(out, "set-count/", lambda: _set_prediction_data_count(m, d))
    # the dense limits through the count alone, where the check comes before anything reads npred points ('order_obs_first_cond_all' and the 5000 distinct
    # locations of the Laplace 'cond_all' type are checked after the device has read the coordinates: left out)
    for t, npred in ((TYPES[2], 24001), (TYPES[3], 24001 - N)):
        m.set_prediction_data(vecchia_pred_type=t)
        put(out, "limit/" + t + "/", lambda: raw_predict(m, npred, d["cp"], d["y"], COV3, var=True))
    cpt = d["cp"].copy()
    cpt[3] = d["coords"][17]
    put(out, "duplicates-latent/", lambda: m.predict(y=d["y"], gp_coords_pred=cpt, cov_pars=COV3, vecchia_pred_type=TYPES[3], num_neighbors_pred=NNP))
    return out


def _set_prediction_data_covariates(m, d):
    from gpboost_amd.basic import _lib, _safe_call, _dptr
    Xp = np.asfortranarray(d["Xp"])
    _safe_call(_lib().GPB_SetPredictionData(m.handle, C.c_int(NP), C.c_void_p(), C.c_void_p(), C.c_void_p(), C.c_void_p(), C.c_void_p(), _dptr(Xp), C.c_void_p(),
                                            C.c_int(-1), C.c_double(-1.), C.c_int(-1), C.c_int(-1)))
    return np.zeros(1)


def _set_prediction_data_count(m, d):
    from gpboost_amd.basic import _lib, _safe_call, _dptr
    cp = np.asfortranarray(d["cp"])
    _safe_call(_lib().GPB_SetPredictionData(m.handle, C.c_int(0), C.c_void_p(), C.c_void_p(), C.c_void_p(), _dptr(cp), C.c_void_p(), C.c_void_p(), C.c_void_p(),
                                            C.c_int(-1), C.c_double(-1.), C.c_int(-1), C.c_int(-1)))
    return np.zeros(1)


# ---- clusters -------------------------------------------------------------------------------------------------------------------------------------------

def case_clusters():
    d = data()
    m = model(d, cluster_ids=d["ids"])
    out = {}
    kw = dict(y=d["y"], gp_coords_pred=d["cp"], cov_pars=COV3, cluster_ids_pred=d["ids_pred"], num_neighbors_pred=NNP)
    for t in TYPES[:2]:
        put(out, t + "/var-latent/", lambda: m.predict(predict_var=True, predict_response=False, vecchia_pred_type=t, **kw))
        put(out, t + "/cov-response/", lambda: m.predict(predict_cov_mat=True, offset=d["fe"], offset_pred=d["fep"], vecchia_pred_type=t, **kw))
    put(out, "train-re/", lambda: m.predict_training_data_random_effects(y=d["y"], cov_pars=COV3, predict_var=True))
    # one-cluster model with prediction cluster ids: cluster 0 is the observed one
    m1 = model(d)
    put(out, "one-cluster/", lambda: m1.predict(y=d["y"], gp_coords_pred=d["cp"], cov_pars=COV3, predict_var=True, cluster_ids_pred=(np.arange(NP) % 2).astype(np.int32)))
    return out


def case_clusters_refusals():
    d = data()
    out = {}
    m = common_refusals(out, d, lambda: model(d, cluster_ids=d["ids"]), COV3, d["y"], cluster_ids_pred=d["ids_pred"])
    ids = d["ids_pred"]
    put(out, "no-cluster-ids/", lambda: raw_predict(m, NP, d["cp"], d["y"], COV3))
    put(out, "saved/", lambda: raw_predict(m, NP, d["cp"], d["y"], COV3, cluster_ids_pred=ids, use_saved_data=True))
    put(out, "covariates/", lambda: raw_predict(m, NP, d["cp"], d["y"], COV3, cluster_ids_pred=ids, X_pred=d["Xp"]))
    put(out, "cov+var&saved/", lambda: raw_predict(m, NP, d["cp"], d["y"], COV3, cluster_ids_pred=ids, cov=True, var=True, use_saved_data=True))
    put(out, "saved&no-cluster-ids/", lambda: raw_predict(m, NP, d["cp"], d["y"], COV3, use_saved_data=True))
    big = np.full(NP, 12, dtype=np.int32)      # 12 > num_neighbors + 1 points in a cluster without observations
    put(out, "prior-cov/", lambda: m.predict(y=d["y"], gp_coords_pred=d["cp"], cov_pars=COV3, cluster_ids_pred=big, predict_cov_mat=True))
    put(out, "prior-var/", lambda: m.predict(y=d["y"], gp_coords_pred=d["cp"], cov_pars=COV3, cluster_ids_pred=big, predict_var=True))
    return out


# ---- exact GP and full-scale Vecchia (device library only) ----------------------------------------------------------------------------------------------

def case_exact():
    d = data(200)
    m = model(d, gp_approx="none")
    out = {}
    for resp in (True, False):
        tag = "response/" if resp else "latent/"
        put(out, tag + "var/", lambda: m.predict(y=d["y"], gp_coords_pred=d["cp"], cov_pars=COV3, predict_var=True, predict_response=resp))
        put(out, tag + "cov/", lambda: m.predict(y=d["y"], gp_coords_pred=d["cp"], cov_pars=COV3, predict_cov_mat=True, predict_response=resp, offset=d["fe"], offset_pred=d["fep"]))
    m.set_prediction_data(gp_coords_pred=d["cp"])
    put(out, "saved/", lambda: m.predict(cov_pars=COV3, use_saved_data=True))
    put(out, "train-re/", lambda: m.predict_training_data_random_effects(y=d["y"], cov_pars=COV3, predict_var=True))
    return out


def case_exact_refusals():
    d = data(200)
    out = {}
    m = common_refusals(out, d, lambda: model(d, gp_approx="none"), COV3, d["y"])
    put(out, "covariates/", lambda: raw_predict(m, NP, d["cp"], d["y"], COV3, X_pred=d["Xp"]))
    put(out, "cov+var&covariates/", lambda: raw_predict(m, NP, d["cp"], d["y"], COV3, X_pred=d["Xp"], cov=True, var=True))
    return out


def case_vif():
    d = data()
    m = model(d, gp_approx="full_scale_vecchia")
    out = {}
    for t in TYPES[:2]:
        for resp in (True, False):
            tag = t + ("/response/" if resp else "/latent/")
            kw = dict(y=d["y"], gp_coords_pred=d["cp"], cov_pars=COV3, predict_response=resp, vecchia_pred_type=t, num_neighbors_pred=NNP)
            put(out, tag + "var/", lambda: m.predict(predict_var=True, **kw))
            put(out, tag + "cov/", lambda: m.predict(predict_cov_mat=True, offset=d["fe"], offset_pred=d["fep"], **kw))
    put(out, "nnp200/", lambda: m.predict(y=d["y"], gp_coords_pred=d["cp"], cov_pars=COV3, vecchia_pred_type=TYPES[1], num_neighbors_pred=200))
    assert not np.array_equal(out[TYPES[0] + "/latent/var/var"], out[TYPES[1] + "/latent/var/var"])
    return out


def case_vif_refusals():
    d = data()
    out = {}
    m = common_refusals(out, d, lambda: model(d, gp_approx="full_scale_vecchia"), COV3, d["y"])
    put(out, "covariates/", lambda: raw_predict(m, NP, d["cp"], d["y"], COV3, X_pred=d["Xp"]))
    put(out, "train-re/", lambda: m.predict_training_data_random_effects(y=d["y"], cov_pars=COV3))
    for t in TYPES[2:4]:
        m.set_prediction_data(vecchia_pred_type=t)
        put(out, "type/" + t + "/", lambda: raw_predict(m, NP, d["cp"], d["y"], COV3))
    put(out, "type&no-coords/", lambda: raw_predict(m, NP, None, d["y"], COV3))
    put(out, "covariates&type/", lambda: raw_predict(m, NP, d["cp"], d["y"], COV3, X_pred=d["Xp"]))
    m.set_prediction_data(vecchia_pred_type=TYPES[1])
    put(out, "limit/", lambda: raw_predict(m, 20001, d["cp"], d["y"], COV3, var=True))      # (checked before anything reads 20001 points)
    return out


# ---- Vecchia-Laplace ------------------------------------------------------------------------------------------------------------------------------------

def _lap(d, lik, gp_approx="vecchia", coords=None):
    m = model(d, likelihood=lik, gp_approx=gp_approx, coords=coords)
    if lik == "gamma":
        m.set_optim_params({"init_aux_pars": [2.0]})
    return m, d[{"bernoulli_logit": "y01", "poisson": "ycount", "gamma": "ypos"}[lik]]


def case_laplace(lik):
    d = data()
    m, y = _lap(d, lik)
    out = {}
    for t in LTYPES:
        kw = dict(y=y, gp_coords_pred=d["cpd"], cov_pars=COV2, vecchia_pred_type=t, num_neighbors_pred=NNP)
        put(out, t + "/var/", lambda: m.predict(predict_var=True, predict_response=False, **kw))
        put(out, t + "/cov/", lambda: m.predict(predict_cov_mat=True, predict_response=False, **kw))
        put(out, t + "/response-var/", lambda: m.predict(predict_var=True, predict_response=True, offset=d["fe"], offset_pred=d["fep"], **kw))
    assert not np.array_equal(out[LTYPES[0] + "/var/var"], out[LTYPES[1] + "/var/var"])
    return out


def case_laplace_arguments():
    d = data()
    out = {}
    m, y = _lap(d, "bernoulli_logit")
    for t in TYPES[:2]:      # for non-Gaussian likelihoods the two names mean their latent counterparts
        put(out, "alias/" + t + "/", lambda: m.predict(y=y, gp_coords_pred=d["cpd"], cov_pars=COV2, predict_var=True, predict_response=False, vecchia_pred_type=t, num_neighbors_pred=NNP))
    m.set_prediction_data(gp_coords_pred=d["cp"], vecchia_pred_type=LTYPES[1], num_neighbors_pred=200)
    put(out, "saved-y-none-nnp200/", lambda: m.predict(cov_pars=COV2, predict_response=True, use_saved_data=True))
    mc, _ = _lap(d, "bernoulli_logit")
    mc.fit(y, X=d["X"], params=dict(maxit=2, init_cov_pars=COV2))
    out["cov_pars"] = np.asarray(mc.get_cov_pars(), dtype=np.float64)
    out["coef"] = np.asarray(mc.get_coef(), dtype=np.float64)
    for t in LTYPES:
        put(out, "covariates/" + t + "/", lambda: mc.predict(gp_coords_pred=d["cpd"], X_pred=d["Xp"], predict_var=True, offset_pred=d["fep"], vecchia_pred_type=t, num_neighbors_pred=NNP))
    put(out, "covariates/train-re/", lambda: mc.predict_training_data_random_effects(predict_var=True))
    put(out, "covariates/missing/", lambda: raw_predict(mc, NP, d["cp"]))
    put(out, "covariates/saved/", lambda: raw_predict(mc, NP, d["cp"], X_pred=d["Xp"], use_saved_data=True))
    put(out, "covariates/missing&saved/", lambda: raw_predict(mc, NP, d["cp"], use_saved_data=True))
    md, _ = _lap(d, "poisson", coords=d["coords_dup"])
    put(out, "train-re-dup/", lambda: md.predict_training_data_random_effects(y=d["ycount"], cov_pars=COV2, predict_var=True, fixed_effects=d["fe"]))
    put(out, "train-re-dup-y-none/", lambda: md.predict_training_data_random_effects(cov_pars=COV2))
    return out


def case_laplace_refusals():
    d = data()
    out = {}
    y = d["y01"]
    m = common_refusals(out, d, lambda: _lap(d, "bernoulli_logit")[0], COV2, y, response=False)
    put(out, "cov-response/", lambda: raw_predict(m, NP, d["cp"], y, COV2, cov=True, response=True))
    put(out, "samples&cov-response/", lambda: raw_predict(m, NP, d["cp"], y, COV2, cov=True, response=True, sample_posterior=True))
    put(out, "cov-response&cov+var/", lambda: raw_predict(m, NP, d["cp"], y, COV2, cov=True, var=True, response=True))
    put(out, "superfluous/", lambda: raw_predict(m, NP, d["cp"], y, COV2, X_pred=d["Xp"], response=False))
    put(out, "negative-cov-pars/", lambda: raw_predict(m, NP, d["cp"], y, np.array([1.2, -0.1]), response=False))
    put(out, "limit-cov/", lambda: raw_predict(m, 20001, d["cp"], y, COV2, cov=True, response=False))
    put(out, "limit-cov&no-cov-pars/", lambda: raw_predict(m, 20001, d["cp"], y, None, cov=True, response=False))
    put(out, "train-re-no-response/", lambda: _lap(d, "bernoulli_logit")[0].predict_training_data_random_effects(cov_pars=COV2))
    put(out, "train-re-no-cov-pars/", lambda: _lap(d, "bernoulli_logit")[0].predict_training_data_random_effects(y=y))
    m.set_prediction_data(vecchia_pred_type=TYPES[2])
    put(out, "type/", lambda: raw_predict(m, NP, d["cp"], y, COV2, response=False))
    put(out, "type&no-coords/", lambda: raw_predict(m, NP, None, y, COV2, response=False))
    put(out, "superfluous&type/", lambda: raw_predict(m, NP, d["cp"], y, COV2, X_pred=d["Xp"], response=False))
    return out


def case_vif_laplace():
    d = data()
    m, y = _lap(d, "bernoulli_logit", gp_approx="full_scale_vecchia")
    out = {}
    for t in LTYPES:
        kw = dict(y=y, gp_coords_pred=d["cpd"], cov_pars=COV2, predict_response=False, vecchia_pred_type=t, num_neighbors_pred=NNP)
        put(out, t + "/var/", lambda: m.predict(predict_var=True, **kw))
        put(out, t + "/cov/", lambda: m.predict(predict_cov_mat=True, **kw))
    put(out, "train-re/", lambda: m.predict_training_data_random_effects(y=y, cov_pars=COV2))
    return out


# ---- training-data random effects -----------------------------------------------------------------------------------------------------------------------

def case_train_re():
    d = data()
    m = model(d)
    out = {}
    put(out, "no-response/", lambda: m.predict_training_data_random_effects(cov_pars=COV3))
    put(out, "no-cov-pars/", lambda: m.predict_training_data_random_effects(y=d["y"]))
    put(out, "no-response&no-cov-pars/", lambda: m.predict_training_data_random_effects())
    put(out, "y/", lambda: m.predict_training_data_random_effects(y=d["y"], cov_pars=COV3, predict_var=True, fixed_effects=d["fe"]))
    put(out, "y-none/", lambda: m.predict_training_data_random_effects(cov_pars=COV3, predict_var=True))
    put(out, "mean/", lambda: m.predict_training_data_random_effects(cov_pars=COV3))
    return out


CASES = {"gv-types": (case_gv_types, {}), "gv-weights": (case_gv_weights, {}), "gv-arguments": (case_gv_arguments, {}), "gv-covariates": (case_gv_covariates, {}), "gv-refusals": (case_gv_refusals, {}),
         "clusters": (case_clusters, {}), "clusters-refusals": (case_clusters_refusals, {}), "exact": (case_exact, {}), "exact-refusals": (case_exact_refusals, {}),
         "vif": (case_vif, {}), "vif-refusals": (case_vif_refusals, {}), "laplace-arguments": (case_laplace_arguments, {}), "laplace-refusals": (case_laplace_refusals, {}),
         "vif-laplace": (case_vif_laplace, {}), "train-re": (case_train_re, {})}
for _lik in ("bernoulli_logit", "poisson", "gamma"):
    CASES["laplace-" + _lik] = (case_laplace, dict(lik=_lik))
DEVICE_ONLY = ("gv-weights", "exact", "exact-refusals", "vif", "vif-refusals", "vif-laplace")      # their shim entry points are not restated on the CPU

NOT_ON_CPU = "is not restated on the CPU"


def on_mock():
    return "mock_shim" in os.environ.get("GPBOOST_AMD_LIB", "")


def fixture_path():
    return os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "predict_paths_mock.npz" if on_mock() else "predict_paths_mi355x.npz")


def case_names():
    return [c for c in CASES if not (on_mock() and c in DEVICE_ONLY)]


def run(name):
    fn, kw = CASES[name]
    got = {name + "/" + k: np.asarray(v) for k, v in fn(**kw).items()}
    return {k: v for k, v in got.items() if not (v.dtype.kind == "U" and NOT_ON_CPU in str(v))}      # (only the CPU restatement says that)


def record(path):
    import time
    out = {}
    for name in case_names():
        t0 = time.perf_counter()
        got = run(name)
        out.update(got)
        print("%-28s %.2f s  %d fields" % (name, time.perf_counter() - t0, len(got)), flush=True)
    if on_mock():
        out["@glibc"] = np.asarray(" ".join(platform.libc_ver()))
        out["@compiler"] = np.asarray(subprocess.run([os.environ.get("CXX", "g++"), "--version"], capture_output=True, text=True).stdout.splitlines()[0])
    np.savez(path, **out)
    print("recorded %d fields of %d cases -> %s" % (len(out), len(case_names()), path))


def merge(paths, dst):
    runs = [dict(np.load(p)) for p in paths]
    out = {}
    for key, first in runs[0].items():
        out[key] = first
        assert all(set(r) == set(runs[0]) for r in runs)
        if not all(np.array_equal(first, r[key]) for r in runs[1:]):
            assert first.dtype.kind == "f", "message %s differs between runs" % key
            stack = np.stack([r[key] for r in runs])
            out[key + "@spread"] = np.max(stack.max(axis=0) - stack.min(axis=0))
            print("NOT reproducible: %s spread %.3e" % (key, out[key + "@spread"]))
    nspread = sum(k.endswith("@spread") for k in out)
    assert nspread <= 0.05 * len(runs[0]), "more than 5 %% of the fields do not reproduce: change the case"
    np.savez_compressed(dst, **out)
    print("merged %d runs, %d fields, %d with a spread -> %s" % (len(runs), len(runs[0]), nspread, dst))


if __name__ == "__main__":
    if sys.argv[1] == "record":
        record(sys.argv[2])
    else:
        merge(sys.argv[3:], sys.argv[2])
