/* gpb_predict.inc -- prediction through the C API (included by gpb_c_api.cpp, after its helpers, outside its extern "C" block):
   GPB_SetPredictionData, GPB_PredictREModel, GPB_PredictREModelTrainingDataRandomEffects and the test seam GPB_HIP_PredictCondAllHost.

   How a prediction is put together (DESIGN.md section 4.8):
     PredCall        the arguments of the C entry point as passed, and what pred_resolve made of them
     pred_path       which of the five model paths a call takes
     predict_*       one function per path: its refusals in its own order, pred_resolve, the device calls, the host algebra
     shared pieces   bp_inverse_rows (forward substitution with Bp = I - A_pp), write_second_moments, scatter_prediction,
                     pred_neighbor_count, location_parameter, add_linear_predictor
   Everything here is host orchestration.  Its sums are taken in a fixed order (neighbour slots ascending, inner index ascending), and
   tests/test_zz_predict_paths_gpu.py holds every result and every message to a recording, bit for bit: an edit that reorders a sum or two checks shows there. */

namespace {

enum class PredPath { VifGauss, Laplace, Exact, Clusters, VecchiaGauss };

struct PredCall {
  // as passed to GPB_PredictREModel
  const double* y_data = nullptr;
  int32_t num_data_pred = 0;
  double* out = nullptr;                     // mean (np), then variances (np) or the covariance matrix (np x np)
  bool cov = false, var = false, response = false, samples = false;
  const int32_t* cluster_ids = nullptr;
  bool grouped = false;                      // grouped effects / random coefficients for prediction: parts of models that are not on this path
  const double* coords_given = nullptr;
  const double* cov_pars = nullptr;
  const double* X_pred = nullptr;
  bool use_saved_data = false;
  const double* fixed_effects = nullptr;
  const double* fixed_effects_pred = nullptr;
  // resolved by pred_resolve
  const double* cp = nullptr;                // prediction coordinates, column-major np x d: given or saved by GPB_SetPredictionData
  int np = 0;
  double c3[3] = {0, 0, 0}, tr[3] = {0, 0, 0};   // Gaussian models: covariance parameters as given (c3: only where they were given, or on the cluster path) and transformed
  double s12 = 0, rho = 0, a_tr = 0;         // non-Gaussian models: GP variance, range, and the range on the kernels' scale
  const double* fe = nullptr;                // offset of the observed data: this call's, else the one saved by GPB_SetOffsetData / a fit
};

const char kBothMoments[] = "Calculation of both the predictive covariance matrix and variances is not supported. Choose one option (predict_cov_mat or predict_var)";   // re_model.cpp Predict
const char kNoCovPars[] = "Covariance parameters have not been estimated or are not given.";                                                                          // re_model.cpp:1119-1121, :1238-1240

PredPath pred_path(const REModelHip* mdl, const PredCall& c) {
  const bool gauss = mdl->likelihood == "gaussian";
  if (mdl->vif && gauss) return PredPath::VifGauss;
  if (!gauss && !mdl->eh && mdl->vhs.size() == 1) return PredPath::Laplace;
  if (gauss && mdl->eh) return PredPath::Exact;
  if (gauss && (mdl->vhs.size() > 1 || c.cluster_ids)) return PredPath::Clusters;
  return PredPath::VecchiaGauss;             // (which refuses what is none of the above)
}

// ---- the pieces of pred_resolve (GPB_PredictREModelTrainingDataRandomEffects uses them one by one) ----

const double* pred_offset(const REModelHip* mdl, const double* fixed_effects) {
  return fixed_effects ? fixed_effects : (mdl->has_offset ? mdl->offset.data() : nullptr);   // re_model_template.h:3601-3607, :4486-4492
}

// (GP variance, range) of a non-Gaussian model, given or stored, and the range parameter of the kernels
int pred_cov_pars_laplace(const REModelHip* mdl, const double* given, double* s12, double* rho, double* a_tr) {
  if (given) { *s12 = given[0]; *rho = given[1]; }
  else {
    if (!mdl->cov_pars_initialized) return set_error("%s", kNoCovPars);
    *s12 = mdl->cov_pars_tr[0]; *rho = range_const(mdl) / mdl->cov_pars_tr[1];
  }
  if (!(*s12 > 0.) || !(*rho > 0.)) return set_error("Covariance parameters need to be positive (found %g, %g)", *s12, *rho);
  *a_tr = range_const(mdl) / *rho;
  return 0;
}

// (error variance, GP variance, range) of a Gaussian model on the original scale, given or transformed back from the stored ones
int pred_cov_pars_original(const REModelHip* mdl, const double* given, double* c3) {
  if (given) { std::copy(given, given + 3, c3); return 0; }
  if (!mdl->cov_pars_initialized) return set_error("%s", kNoCovPars);
  transform_back(mdl, mdl->cov_pars_tr, c3);
  return 0;
}

enum class Resolve { Coords, CovPars, Response, CovMatLimit };

/* The common steps of every path, in the order the path lists them (which of two applicable refusals fires first is part of the interface):
   coordinates given or saved, covariance parameters given or stored, the response check, the dense limit of a non-Gaussian covariance matrix;
   then the choice of the offset, which cannot fail. */
int pred_resolve(const REModelHip* mdl, PredCall& c, PredPath path, std::initializer_list<Resolve> order) {
  for (const Resolve step : order) {
    if (step == Resolve::Coords) {
      c.cp = c.coords_given; c.np = c.num_data_pred;
      if (c.use_saved_data) { c.cp = mdl->coords_pred.empty() ? nullptr : mdl->coords_pred.data(); c.np = mdl->num_data_pred; }
      if (!c.cp || c.np <= 0)      // (the cluster path has refused saved data before it comes here)
        return set_error("GPB_PredictREModel: no coordinates for prediction (%s)", path == PredPath::Clusters ? "gp_coords_data_pred" : "gp_coords_data_pred / GPB_SetPredictionData");
    } else if (step == Resolve::CovPars) {
      if (path == PredPath::Laplace) { if (pred_cov_pars_laplace(mdl, c.cov_pars, &c.s12, &c.rho, &c.a_tr)) return -1; }
      else if (c.cov_pars || path == PredPath::Clusters) {      // the cluster path hands the original scale on to its one-cluster views
        if (pred_cov_pars_original(mdl, c.cov_pars, c.c3) || transform_cov_pars(mdl, c.c3, c.tr)) return -1;
      } else {
        if (!mdl->cov_pars_initialized) return set_error("%s", kNoCovPars);
        std::copy(mdl->cov_pars_tr, mdl->cov_pars_tr + 3, c.tr);
      }
    } else if (step == Resolve::Response) {
      if (!c.y_data && !mdl->y_set) return set_error("GPB_PredictREModel: y_data is NULL and no response has been set by an earlier call");
    } else if (c.cov && c.np > 20000) {
      return set_error("GPB_PredictREModel: predictive covariance matrix for %d points (dense limit: 20000)", c.np);
    }
  }
  c.fe = pred_offset(mdl, c.fixed_effects);
  return 0;
}

// The refusals every path opens with: samples, [non-Gaussian: the covariance matrix of the response,] both second moments at once
int pred_refuse_samples_and_moments(const PredCall& c, const char* samples_what, const char* scope, bool non_gaussian = false) {
  if (c.samples) return set_error("GPB_PredictREModel: %s %s", samples_what, scope);
  if (non_gaussian && c.response && c.cov)      // re_model_template.h:3526-3529
    return set_error("Calculation of the predictive covariance matrix is not supported when predicting the response variable (label) for non-Gaussian likelihoods");
  if (c.cov && c.var) return set_error("%s", kBothMoments);
  return 0;
}

// Covariates of a model fitted with them (re_model.cpp Predict); saved_excuses_missing: the path's check for missing covariates lets saved prediction data through
// to the refusal that names them
int pred_check_covariates(const REModelHip* mdl, const PredCall& c, bool saved_excuses_missing, const char* scope) {
  if (mdl->p_cov > 0 && !mdl->coef_estimated) return set_error("GPB_PredictREModel: the model has covariates but no estimated coefficients");
  if (mdl->p_cov > 0 && !c.X_pred && !(saved_excuses_missing && c.use_saved_data))
    return set_error("No covariate data is provided in 'covariate_data_pred' but the model has linear regression covariates");
  if (mdl->p_cov == 0 && c.X_pred) return set_error("Covariate data is provided in 'covariate_data_pred' but the model has no linear regression covariates");
  if (mdl->p_cov > 0 && c.use_saved_data) return set_error("GPB_PredictREModel: saved prediction data together with covariates %s", scope);
  return 0;
}

// ---- shared host pieces ----

// num_neighbors_pred: default 2 * num_neighbors (re_model_template.h:299), at most `cap` points to choose from (Vecchia_utils.cpp:755-758) and the 126 neighbours
// of the device kernels (GPB_MAX_NEIGHBORS)
int pred_neighbor_count(const REModelHip* mdl, int cap, bool warn) {
  int nnp = mdl->num_neighbors_pred > 0 ? mdl->num_neighbors_pred : 2 * mdl->num_neighbors;
  if (nnp > cap) nnp = cap;
  if (nnp > 126) {
    if (warn) log_info("[GPBoost-AMD] [Warning] num_neighbors_pred = %d exceeds the %d neighbours the MI355X kernels support; %d are used\n", nnp, 126, 126);
    nnp = 126;
  }
  return nnp;
}

// Location parameter of the observed data = fixed effects + X beta for a model fitted with covariates (UpdateFixedEffects, re_model_template.h:2859-2871), else fe itself
const double* location_parameter(const REModelHip* mdl, const double* fe, std::vector<double>* storage) {
  if (!(mdl->p_cov > 0 && mdl->coef_estimated)) return fe;
  storage->assign(mdl->n, 0.);
  for (int i = 0; i < mdl->n; ++i) {
    double v = fe ? fe[i] : 0.;
    for (int j = 0; j < mdl->p_cov; ++j) v += mdl->X[(size_t)j * mdl->n + i] * mdl->beta[j];
    (*storage)[i] = v;
  }
  return storage->data();
}

// mean += X_pred beta (re_model_template.h:3868-3880) and the external fixed effects (:3862-3867); offset_first: the order of the non-Gaussian path
void add_linear_predictor(const REModelHip* mdl, const PredCall& c, double* mean, bool offset_first = false) {
  if (offset_first && c.fixed_effects_pred) for (int k = 0; k < c.np; ++k) mean[k] += c.fixed_effects_pred[k];
  if (mdl->p_cov > 0) for (int j = 0; j < mdl->p_cov; ++j) for (int k = 0; k < c.np; ++k) mean[k] += c.X_pred[(size_t)j * c.np + k] * mdl->beta[j];
  if (!offset_first && c.fixed_effects_pred) for (int k = 0; k < c.np; ++k) mean[k] += c.fixed_effects_pred[k];
}

/* What bp_inverse_rows carries through the recursion; every member may be null */
struct BpCarry {
  double* mean = nullptr;          // in: where every row's sum starts; out: x with Bp x = start [+ A_po y_obs]
  const double* y_obs = nullptr;   // values at the observed points, added to mean in slot order (null: the start values hold that part already)
  double* rows = nullptr;          // n_pred x n_pred, zero on entry: the rows of Bp^-1, columns 0..i of row i
  double* block = nullptr;         // n_pred x k, in place: Bp^-1 times the block
  int k = 0;
};

/* Forward substitution with Bp = I - A_pp, unit lower triangular because a neighbour precedes its point (CalcPredVecchiaObservedFirstOrder with
   CondObsOnly = false, Vecchia_utils.cpp:2061-2090):  row_i = e_i + sum_j a_ij row_q,  q = nn[i][j] - n_obs,  applied to the rows of Bp^-1 and to whatever
   else is carried.  nn: n_pred x m_used indices into (observed, prediction) points, -1 padded; A the factor rows aligned with it.  Terms are added with j
   ascending over the neighbour slots and the inner index ascending.  who: the caller's words for the one refusal; report_from: what it subtracts from the
   neighbour index it reports (n_obs: the index among the prediction points). */
int bp_inverse_rows(int n_obs, int n_pred, int m_used, const int32_t* nn, const double* A, const BpCarry& w, const char* who, int report_from) {
  for (int i = 0; i < n_pred; ++i) {
    double* ri = w.rows ? w.rows + (size_t)i * n_pred : nullptr;
    if (ri) ri[i] = 1.;
    for (int j = 0; j < m_used; ++j) {
      const int c = nn[(size_t)i * m_used + j];
      if (c < 0) continue;
      if (c >= n_obs + i) return set_error("%s %d has neighbour %d that does not precede it", who, i, c - report_from);
      const double a = A[(size_t)i * m_used + j];
      if (c < n_obs) { if (w.mean && w.y_obs) w.mean[i] += a * w.y_obs[c]; continue; }
      const int q = c - n_obs;
      if (w.mean) w.mean[i] += a * w.mean[q];
      if (w.block) {
        double* bi = w.block + (size_t)i * w.k;
        const double* bq = w.block + (size_t)q * w.k;      // (row q is finished: rows are done in order)
        for (int r = 0; r < w.k; ++r) bi[r] += a * bq[r];
      }
      if (ri) {
        const double* rq = w.rows + (size_t)q * n_pred;
        for (int r = 0; r <= q; ++r) ri[r] += a * rq[r];
      }
    }
  }
  return 0;
}

/* Second moments of np points: v_ij = sigma2 f(i, j), plus diag_shift on the diagonal -- over the lower triangle with a symmetric store into cov_out
   (np x np) if that is asked for, over the diagonal otherwise; var_out (np) gets the diagonal.  Either output may be null.  Where a path removes or adds the
   error variance INSIDE the scaled sum, its f does that and diag_shift is 0. */
template <class F>
void write_second_moments(double* var_out, double* cov_out, int np, double sigma2, double diag_shift, F f) {
  for (int i = 0; i < np; ++i)
    for (int j = cov_out ? 0 : i; j <= i; ++j) {
      double v = sigma2 * f(i, j);
      if (i == j && diag_shift != 0.) v += diag_shift;
      if (cov_out) { cov_out[(size_t)i * np + j] = v; cov_out[(size_t)j * np + i] = v; }
      if (var_out && i == j) var_out[i] = v;
    }
}

/* Results of a subset of the prediction points into the caller's order.  Entry k of `count`: position dst[k] of the output (null: k) is entry src[k] of the
   computed set of n_sub (null: k).  mean / var / cov: null where not asked for; cov_out has np columns.  transposed: cov (n_sub x n_sub) is read as
   cov[src[b]][src[a]] for the output's [dst[a]][dst[b]] -- a row-major matrix of the device into the column-major output of the C API. */
void scatter_prediction(double* mean_out, double* var_out, double* cov_out, int np, int count, const int* dst, const int* src, const double* mean,
                        const double* var, const double* cov, int n_sub, bool transposed) {
  const auto D = [&](int k) { return dst ? dst[k] : k; };
  const auto S = [&](int k) { return src ? src[k] : k; };
  for (int k = 0; k < count; ++k) {
    if (mean_out) mean_out[D(k)] = mean[S(k)];
    if (var_out) var_out[D(k)] = var[S(k)];
  }
  if (cov_out)
    for (int a = 0; a < count; ++a)
      for (int b = 0; b < count; ++b)
        cov_out[(size_t)D(a) * np + D(b)] = transposed ? cov[(size_t)S(b) * n_sub + S(a)] : cov[(size_t)S(a) * n_sub + S(b)];
}

double sq_dist(const double* coords_colmajor, int n, int d, int i, int j) {
  double s2 = 0.;
  for (int c = 0; c < d; ++c) { const double t = coords_colmajor[(size_t)c * n + i] - coords_colmajor[(size_t)c * n + j]; s2 += t * t; }
  return s2;
}

// ---- full-scale Vecchia (VIF), Gaussian ----

/* 'order_obs_first_cond_obs_only' (the reference's default for Gaussian data; CalcPredVecchiaObservedFirstOrder with the full_scale_vecchia arguments,
   Vecchia_utils.cpp:1701-2060; re_model_template.h:4041-4056): y_p = C_p Sigma_m^-1 eta + e_p with the residual e_p conditioning on the nearest observed
   points -> mean = A_p y_nn + (B C)_p W^-1 (B C)' D^-1 B y, var = sigma2 (D_p + (B C)_p W^-1 (B C)_p').
   'order_obs_first_cond_all' (CondObsOnly = false, :1975-2046): the device returns the rows of [Bpo Bp] of the appended points, -(Bpo y) and (B~ C~)_p; here the
   forward substitutions with Bp --  mean = Bp^-1 (-Bpo y + (B~ C~)_p v),  T = Bp^-1 (B~ C~)_p,  rows of Bp^-1 --  and
   cov = sigma2 (Bp^-1 Dp Bp^-T + T W^-1 T')  [- sigma2 I for the latent process].  The reference's eight-term expression (:2028-2046) is T W^-1 T' written out
   with W = Sigma_m + (B C)' D^-1 (B C).  Dense in the number of prediction points, as the 'cond_all' type of the plain Vecchia model here.
   (The reference has exactly these two types for full-scale Vecchia models: 'order_pred_first' and the latent types are fatal there, re_model_template.h:4072-4110.) */
int predict_vif_gauss(REModelHip* mdl, PredCall& c) {
  const char* scope = "is not on the MI355X path of this library (full-scale Vecchia prediction: 'order_obs_first_cond_obs_only' / 'order_obs_first_cond_all', no covariates / samples)";
  if (pred_refuse_samples_and_moments(c, "samples of a full-scale Vecchia model", scope)) return -1;
  if (c.cluster_ids || c.grouped || c.X_pred || mdl->p_cov > 0)
    return set_error("GPB_PredictREModel: cluster ids / grouped effects / random coefficients / covariates for prediction %s", scope);
  const bool cond_all = mdl->vecchia_pred_type == "order_obs_first_cond_all";
  if (mdl->vecchia_pred_type != "order_obs_first_cond_obs_only" && !cond_all)
    return set_error("GPB_PredictREModel: vecchia_pred_type '%s' of a full-scale Vecchia model %s", mdl->vecchia_pred_type.c_str(), scope);
  if (pred_resolve(mdl, c, PredPath::VifGauss, {Resolve::Coords, Resolve::CovPars, Resolve::Response})) return -1;
  if (prediction_response(mdl, c.y_data, c.fe)) return -1;
  VifSolve vs;
  double t3[3];
  if (vif_terms(mdl, c.tr[1], c.tr[2], t3, &vs)) return -1;
  const int np = c.np, kv = mdl->num_ind_points;
  const int nnp = pred_neighbor_count(mdl, cond_all ? mdl->n + np - 1 : mdl->n, false);
  const bool second = c.var || c.cov;
  std::vector<double> up(np), Dp(np), BC((size_t)np * kv), mean(np), Lr;      // Lr: rows of Bp^-1 ('cond_all' with second moments)
  if (cond_all) {
    if (second && np > 20000) return set_error("GPB_PredictREModel: predictive (co)variances of 'order_obs_first_cond_all' for %d points (dense limit: 20000)", np);
    int mu = 0;
    std::vector<int32_t> nnr((size_t)np * nnp);
    std::vector<double> Ap((size_t)np * nnp);
    if (gpb_hip_vecchia_vif_predict_cond_all(mdl->vh, np, c.cp, nnp, mdl->ip.data(), mdl->cov_type, c.tr[1], c.tr[2], vs.Linv.data(), &mu, nnr.data(), Ap.data(),
                                             up.data(), Dp.data(), BC.data(), nullptr)) return shim_error();
    for (int i = 0; i < np; ++i) { double w = -up[i]; for (int j = 0; j < kv; ++j) w += BC[(size_t)i * kv + j] * vs.v[j]; mean[i] = w; }
    if (second) Lr.assign((size_t)np * np, 0.);
    BpCarry carry;      // (the observed neighbours are in u and BC already)
    carry.mean = mean.data(); carry.rows = second ? Lr.data() : nullptr; carry.block = second ? BC.data() : nullptr; carry.k = kv;
    if (bp_inverse_rows(mdl->n, np, mu, nnr.data(), Ap.data(), carry, "GPB_PredictREModel: prediction point", mdl->n)) return -1;
  } else {
    if (gpb_hip_vecchia_vif_predict_obs_only(mdl->vh, np, c.cp, nnp, mdl->ip.data(), mdl->cov_type, c.tr[1], c.tr[2], vs.Linv.data(), up.data(), Dp.data(), BC.data(), nullptr))
      return shim_error();
    for (int i = 0; i < np; ++i) { double w = -up[i]; for (int j = 0; j < kv; ++j) w += BC[(size_t)i * kv + j] * vs.v[j]; mean[i] = w; }
  }
  for (int i = 0; i < np; ++i) c.out[i] = mean[i] + (c.fixed_effects_pred ? c.fixed_effects_pred[i] : 0.);
  if (second) {
    // T_i = L_W^-1 (B C)_i: var_p = D_p + ||T_p||^2 and -- obs-only: the residuals of two prediction points are independent given the observed ones
    // (Bp = I) -- cov_pq = T_p . T_q off the diagonal
    gpb_sm::solve_lower_rows(vs.Lw.data(), kv, kv, np, BC.data());      // rows <- rows L_W^-T
    const double* T = BC.data();
    const double sigma2 = c.tr[0], latent = c.response ? 0. : 1.;
    const auto tt = [&](int i, int j) { double qq = 0.; for (int r = 0; r < kv; ++r) qq += T[(size_t)i * kv + r] * T[(size_t)j * kv + r]; return qq; };
    if (cond_all)
      write_second_moments(c.var ? c.out + np : nullptr, c.cov ? c.out + np : nullptr, np, sigma2, 0., [&](int i, int j) {
        double qq = tt(i, j);
        for (int r = 0; r <= j; ++r) qq += Lr[(size_t)i * np + r] * Dp[r] * Lr[(size_t)j * np + r];
        return qq - (i == j ? latent : 0.);
      });
    else
      write_second_moments(c.var ? c.out + np : nullptr, c.cov ? c.out + np : nullptr, np, sigma2, 0.,
                           [&](int i, int j) { return tt(i, j) + (i == j ? Dp[i] - latent : 0.); });
  }
  mdl->yaux_valid = false;
  return 0;
}

// ---- Vecchia-Laplace, with and without inducing points ----

/* 'latent_order_obs_first_cond_all' of the plain Vecchia-Laplace model (PredictLaplaceApproxVecchia with CondObsOnly = false, likelihoods.h:8603-8606,
   8790-8821): the prediction points condition on the observed AND the preceding prediction points.  Device: factor rows of the appended points (latent: no
   nugget); host: the rows of Bp^-1 and of C = Bp^-1 Bpo; device: the quadratic forms C (Sigma^-1 + W)^-1 C'.
     mean = -C mode,   cov = Bp^-1 Dp Bp^-T + C (Sigma^-1 + W)^-1 C'
   nu distinct locations cu; mu_u / var_u / cov_u: null where not asked for. */
int laplace_cond_all_host(REModelHip* mdl, const PredCall& c, const char* scope, int nu, const double* cu, const std::vector<double>& mode, double* mu_u,
                          double* var_u, double* cov_u) {
  if (nu > 5000) return set_error("GPB_PredictREModel: '%s' for %d > 5000 distinct prediction locations %s", mdl->vecchia_pred_type.c_str(), nu, scope);
  const int n_obs = mdl->n_re > 0 ? mdl->n_re : mdl->n;
  const int mcap = pred_neighbor_count(mdl, n_obs + nu - 1, false);
  int mu_ = 0, cg_it = 0;
  std::vector<int32_t> nnr((size_t)nu * mcap);
  std::vector<double> Ap((size_t)nu * mcap), Dp(nu);
  if (gpb_hip_vecchia_predict_cond_all_latent(mdl->vh, nu, cu, mcap, mdl->cov_type, c.s12, c.a_tr, &mu_, nnr.data(), Ap.data(), Dp.data(), nullptr)) return shim_error();
  std::vector<double> R((size_t)nu * nu, 0.);                       // rows of Bp^-1 (unit lower triangular)
  BpCarry carry;
  carry.rows = R.data();
  if (bp_inverse_rows(n_obs, nu, mu_, nnr.data(), Ap.data(), carry, "GPB_PredictREModel: prediction point", n_obs)) return -1;
  std::vector<std::vector<std::pair<int, double>>> Crow(nu);        // rows of C = Bp^-1 Bpo as (column, value), columns ascending
  std::vector<double> acc(n_obs, 0.); std::vector<char> seen(n_obs, 0); std::vector<int> touched;
  for (int k = 0; k < nu; ++k) {
    const double* Rk = R.data() + (size_t)k * nu;
    touched.clear();
    for (int q = 0; q <= k; ++q) {
      const double rq = Rk[q];
      if (rq == 0.) continue;
      for (int j = 0; j < mu_; ++j) {
        const int col = nnr[(size_t)q * mu_ + j];
        if (col < 0 || col >= n_obs) continue;
        if (!seen[col]) { seen[col] = 1; touched.push_back(col); }      // every column once (the device writes one right-hand-side entry per column)
        acc[col] += rq * (-Ap[(size_t)q * mu_ + j]);                    // Bpo = -A_po
      }
    }
    std::sort(touched.begin(), touched.end());
    double m_k = 0.;
    for (int col : touched) { Crow[k].emplace_back(col, acc[col]); m_k -= acc[col] * mode[col]; acc[col] = 0.; seen[col] = 0; }
    mu_u[k] = m_k;
  }
  if (!var_u && !cov_u) return 0;
  size_t mmax = 1;
  for (int k = 0; k < nu; ++k) mmax = std::max(mmax, Crow[k].size());
  std::vector<int32_t> cols((size_t)nu * mmax, -1);
  std::vector<double> vals((size_t)nu * mmax, 0.);
  for (int k = 0; k < nu; ++k) for (size_t e = 0; e < Crow[k].size(); ++e) { cols[(size_t)k * mmax + e] = Crow[k][e].first; vals[(size_t)k * mmax + e] = Crow[k][e].second; }
  std::vector<double> q(cov_u ? (size_t)nu * nu : (size_t)nu);
  if (gpb_hip_vecchia_laplace_quad_forms(mdl->vh, nu, (int)mmax, cols.data(), vals.data(), mdl->cg_max_num_it, kPredVarCgTol, cov_u ? 1 : 0, q.data(), &cg_it)) return shim_error();
  write_second_moments(var_u, cov_u, nu, 1., 0., [&](int r, int c2) {      // prior part Bp^-1 Dp Bp^-T + the quadratic form
    double pr = 0.;
    for (int j = 0; j <= c2; ++j) pr += R[(size_t)r * nu + j] * Dp[j] * R[(size_t)c2 * nu + j];
    return pr + (cov_u ? q[(size_t)r * nu + c2] : q[r]);
  });
  return 0;
}

/* Non-Gaussian (Vecchia-Laplace) models, the reference's default prediction type for them ('latent_order_obs_first_cond_obs_only') and
   'latent_order_obs_first_cond_all':  latent mean -Bpo mode, latent (co)variances Dp + Bpo (Sigma^-1 + W)^-1 Bpo' (PredictLaplaceApproxVecchia,
   likelihoods.h:8563-8824 -- the exact value of its "cholesky" branch, which its "iterative" branch estimates with nsim_var_pred random vectors), and the
   response-scale predictions from them (PredictResponse, :9626-9672).  Repeated prediction locations share a random effect (re_model_template.h:3976-3988).
   Full-scale Vecchia (PredictLaplaceApproxFSVA, likelihoods.h:7999-8535): means, variances and covariance matrices of both latent types on the device.  With
   covariates the mode is found at the location parameter fixed effects + X beta and X_pred beta joins the latent mean. */
int predict_laplace(REModelHip* mdl, PredCall& c) {
  const char* scope = "is not on the MI355X path of this library (non-Gaussian likelihoods: 'latent_order_obs_first_cond_obs_only' / 'latent_order_obs_first_cond_all', no samples)";
  if (pred_refuse_samples_and_moments(c, "posterior / prior samples", scope, true)) return -1;
  if (c.cluster_ids || c.grouped) return set_error("GPB_PredictREModel: cluster ids / grouped effects / random coefficients for prediction %s", scope);
  if (pred_check_covariates(mdl, c, false, scope)) return -1;
  const std::string& pt = mdl->vecchia_pred_type;
  // for non-Gaussian likelihoods the two 'order_obs_first_*' names mean their latent counterparts (re_model_template.h:7112-7124)
  const bool cond_all = pt == "latent_order_obs_first_cond_all" || pt == "order_obs_first_cond_all";
  if (!pt.empty() && pt != "order_obs_first_cond_obs_only" && pt != "latent_order_obs_first_cond_obs_only" && !cond_all)
    return set_error("GPB_PredictREModel: vecchia_pred_type '%s' %s", pt.c_str(), scope);
  if (pred_resolve(mdl, c, PredPath::Laplace, {Resolve::Coords, Resolve::Response, Resolve::CovMatLimit, Resolve::CovPars})) return -1;
  std::vector<double> fe_lin;
  const double* fel = location_parameter(mdl, c.fe, &fe_lin);
  if (c.y_data) { if (laplace_upload_data(mdl, c.y_data, fel)) return -1; }
  else if (laplace_upload_fixed_effects(mdl, fel)) return -1;
  std::vector<double> mode(mdl->n_re > 0 ? mdl->n_re : mdl->n);
  if (laplace_prepare_preconditioner(mdl)) return -1;
  if (gpb_hip_vecchia_laplace_logit(mdl->vh, mdl->cov_type, c.s12, c.a_tr, mdl->num_rand_vec_trace, mdl->seed_rand_vec_trace, mdl->cg_max_num_it,
                                    mdl->cg_max_num_it_tridiag, mdl->cg_delta_conv, mdl->delta_conv_mode_finding, 1, mdl->lap_info, mode.data()))
    return shim_error();
  if (!mdl->vif && gpb_hip_vecchia_set_y(mdl->vh, mode.data())) return shim_error();          // the "response" of the prediction is the mode (Vecchia order)
  const bool need_var = c.var || c.response;            // every likelihood on the path needs the latent variance for its response mean
  // unique prediction locations: first appearances, in the order given (DetermineUniqueDuplicateCoordsFast on the prediction coordinates)
  const int np = c.np, d = mdl->d;
  std::vector<double> cpv(c.cp, c.cp + (size_t)np * d);
  std::vector<int> uq, ui;
  unique_locations(cpv, np, d, &uq, &ui);
  const int nu = (int)uq.size();
  std::vector<double> cu((size_t)nu * d);
  for (int j = 0; j < d; ++j) for (int u = 0; u < nu; ++u) cu[(size_t)j * nu + u] = cpv[(size_t)j * np + uq[u]];
  std::vector<double> mu_u(nu), var_u(need_var ? nu : 0), cov_u(c.cov ? (size_t)nu * nu : 0);
  double* var_p = need_var ? var_u.data() : nullptr;
  double* cov_p = c.cov ? cov_u.data() : nullptr;
  const int nnp = pred_neighbor_count(mdl, std::numeric_limits<int>::max(), false);
  int cg_it = 0;
  if (mdl->vif) {      // both latent types in one call: a negative neighbour count = 'latent_order_obs_first_cond_all'
    if (gpb_hip_vecchia_vif_laplace_predict(mdl->vh, nu, cu.data(), cond_all ? -nnp : nnp, mdl->cov_type, c.s12, c.a_tr, mdl->cg_max_num_it, kPredVarCgTol, mu_u.data(),
                                            var_p, cov_p, nullptr, &cg_it)) return shim_error();
  } else if (cond_all) {
    if (laplace_cond_all_host(mdl, c, scope, nu, cu.data(), mode, mu_u.data(), var_p, cov_p)) return -1;
  } else if (gpb_hip_vecchia_laplace_predict(mdl->vh, nu, cu.data(), nnp, mdl->cov_type, c.s12, c.a_tr, mdl->cg_max_num_it, kPredVarCgTol, mu_u.data(), var_p, cov_p,
                                             nullptr, &cg_it))
    return shim_error();
  std::vector<double> mu(np), var(need_var ? np : 0);
  scatter_prediction(mu.data(), need_var ? var.data() : nullptr, nullptr, np, np, nullptr, ui.data(), mu_u.data(), var_p, nullptr, nu, false);
  add_linear_predictor(mdl, c, mu.data(), true);
  if (c.response && !predict_response_host(mdl->likelihood, np, mu.data(), var.data(), c.var, mdl->delta_conv_mode_finding, mdl->aux_pars[0]))
    return set_error("GPB_PredictREModel: response predictions for likelihood '%s' %s", mdl->likelihood.c_str(), scope);
  std::copy(mu.begin(), mu.end(), c.out);
  if (c.var) std::copy(var.begin(), var.end(), c.out + np);
  // Zpred cov Zpred' (re_model_template.h:4306-4316), column-major like the reference's output
  if (c.cov) scatter_prediction(nullptr, nullptr, c.out + np, np, np, nullptr, ui.data(), nullptr, nullptr, cov_p, nu, true);
  return 0;
}

// ---- exact GP ----

/* Exact GP (gp_approx = "none"): mean = Sigma_po Psi^-1 y, covariance = Sigma_pp [+ sigma2 I] - Sigma_po Psi^-1 Sigma_op (the dense Gaussian branch of
   REModelTemplate::Predict, re_model_template.h:4239-4330); both reductions are blocks of one Schur complement on the device. */
int predict_exact(REModelHip* mdl, PredCall& c) {
  const char* scope = "is not on the MI355X path of this library (exact GP prediction: coordinates only, no covariates / samples)";
  if (pred_refuse_samples_and_moments(c, "posterior / prior samples", scope)) return -1;
  if (c.cluster_ids || c.grouped || c.X_pred || mdl->p_cov > 0)
    return set_error("GPB_PredictREModel: cluster ids / grouped effects / random coefficients / covariates for prediction %s", scope);
  if (pred_resolve(mdl, c, PredPath::Exact, {Resolve::Coords, Resolve::CovPars, Resolve::Response})) return -1;
  if (prediction_response(mdl, c.y_data, c.fe)) return -1;
  const int np = c.np;
  const bool second = c.var || c.cov;
  std::vector<double> q(second ? (size_t)np * np : 0);
  if (gpb_hip_exact_predict(mdl->eh, mdl->cov_type, c.tr[1], c.tr[2], np, c.cp, c.out, second ? q.data() : nullptr)) return shim_error();
  if (c.fixed_effects_pred) for (int k = 0; k < np; ++k) c.out[k] += c.fixed_effects_pred[k];
  const double nug = c.response ? 1. : 0.;
  if (second)
    write_second_moments(c.var ? c.out + np : nullptr, c.cov ? c.out + np : nullptr, np, c.tr[0], 0., [&](int i, int j) {
      const double prior = i == j ? c.tr[1] + nug : gpb_sm::matern_gaussian_paths(mdl->cov_type, c.tr[1], c.tr[2] * std::sqrt(sq_dist(c.cp, np, mdl->d, i, j)));
      return prior - q[(size_t)i * np + j];
    });
  mdl->yaux_valid = false;
  return 0;
}

// ---- the one-cluster Gaussian Vecchia model ----

/* 'order_obs_first_cond_obs_only' (REModel::Predict, re_model.cpp:1083-1215 -> CalcPredVecchiaObservedFirstOrder(CondObsOnly = true),
   Vecchia_utils.cpp:1701-2060): neighbours are observed points only, Bp = I, the predictive covariance is diag(Dp). */
int gauss_obs_only(REModelHip* mdl, const PredCall& c, int nnp) {
  const int np = c.np;
  std::vector<double> D(np);
  if (gpb_hip_vecchia_predict_obs_only(mdl->vh, np, c.cp, nnp, mdl->cov_type, c.tr[1], c.tr[2], c.out, D.data(), nullptr)) return shim_error();
  add_linear_predictor(mdl, c, c.out);
  if (c.var || c.cov)
    write_second_moments(c.var ? c.out + np : nullptr, c.cov ? c.out + np : nullptr, np, c.tr[0], 0.,
                         [&](int i, int j) { return i != j ? 0. : (c.response ? D[i] : D[i] - 1.); });
  return 0;
}

/* 'order_obs_first_cond_all': search + factor of the appended rows on the device, then the forward substitution with Bp and the rows of Bp^-1 on the host
   (Vecchia_utils.cpp:2061-2090, GPB_HIP_PredictCondAllHost); yv: the response of the observed points in Vecchia order. */
int gauss_cond_all(REModelHip* mdl, const PredCall& c, int nnp, const double* yv) {
  const int np = c.np;
  int mu = 0;
  std::vector<int32_t> nn((size_t)np * nnp);
  std::vector<double> Ap((size_t)np * nnp), Dp(np);
  if (gpb_hip_vecchia_predict_cond_all(mdl->vh, np, c.cp, nnp, mdl->cov_type, c.tr[1], c.tr[2], &mu, nn.data(), Ap.data(), Dp.data(), nullptr)) return shim_error();
  if (GPB_HIP_PredictCondAllHost(mdl->n, np, mu, nn.data(), Ap.data(), Dp.data(), yv, c.tr[0], c.response, c.out, c.var ? c.out + np : nullptr, c.cov ? c.out + np : nullptr)) return -1;
  add_linear_predictor(mdl, c, c.out);
  return 0;
}

/* 'order_pred_first' (CalcPredVecchiaPredictedFirstOrder, Vecchia_utils.cpp:2203-2444) and 'latent_order_obs_first_cond_*'
   (CalcPredVecchiaLatentObservedFirstOrder, :2446-2666): neighbour search + factor of EVERY point of the joint ordering on the device; the conditional
   precision is assembled here from the factor rows and solved / inverted by the dense Cholesky on the device.
     order_pred_first: cond_prec = Bp' Dp^-1 Bp + Bop' Do^-1 Bop over the prediction points, mean = -cond_prec^-1 Bop' Do^-1 Bo y (:2419-2423)
     latent_*: the reference forms Sigma = B^-1 D B^-T and conditions on y = b_obs + eps by the Woodbury identity (:2597-2650); the same posterior is
       M^-1 Z_o' R^-1 y and M^-1 restricted to the prediction points with M = B' D^-1 B + Z_o' R^-1 Z_o, which needs no B^-1 */
int gauss_joint_factor(REModelHip* mdl, const PredCall& c, int nnp, const double* yv, bool pred_first, bool cond_all) {
  const bool latent = !pred_first;
  const int np = c.np, n = mdl->n, n_all = n + np;
  const char* dense_scope = "is not on the MI355X path of this library (the conditional precision is handled densely; use 'order_obs_first_cond_obs_only' / 'order_obs_first_cond_all')";
  if (pred_first && np > 24000) return set_error("GPB_PredictREModel: 'order_pred_first' for %d > 24000 prediction points %s", np, dense_scope);
  if (latent && n_all > 24000) return set_error("GPB_PredictREModel: '%s' for %d > 24000 observed + prediction points %s", mdl->vecchia_pred_type.c_str(), n_all, dense_scope);
  std::vector<int32_t> nn((size_t)n_all * nnp);
  std::vector<double> A((size_t)n_all * nnp), D(n_all), u(n_all);
  int mu = 0, dup = 0;
  if (gpb_hip_vecchia_predict_joint_factor(mdl->vh, np, c.cp, nnp, pred_first ? 1 : 0, (pred_first || cond_all) ? 1 : 0, latent ? 0 : 1, mdl->cov_type,
                                           c.tr[1], c.tr[2], &mu, nn.data(), A.data(), D.data(), u.data(), &dup)) return shim_error();
  if (latent && dup) return set_error("Duplicates found among training and test coordinates. This is not supported for predictions with a Vecchia approximation for the latent process ('latent_') ");   // :2563-2566
  const bool second = c.var || c.cov;
  const int q = pred_first ? np : n_all;                  // dimension of the precision matrix = the columns of B that enter it
  std::vector<double> M((size_t)q * q, 0.), rhs(q, 0.), x(q), inv;
  std::vector<int> ec; std::vector<double> ev;
  ec.reserve(mu + 1); ev.reserve(mu + 1);
  for (int i = 0; i < n_all; ++i) {
    ec.clear(); ev.clear();
    if (i < q) { ec.push_back(i); ev.push_back(1.); }
    for (int j = 0; j < mu; ++j) {
      const int col = nn[(size_t)i * mu + j];
      if (col >= 0 && col < q) { ec.push_back(col); ev.push_back(-A[(size_t)i * mu + j]); }
    }
    const double dinv = 1. / D[i];
    for (size_t a1 = 0; a1 < ec.size(); ++a1) {
      const double va = ev[a1] * dinv;
      for (size_t b1 = 0; b1 < ec.size(); ++b1) if (ec[b1] <= ec[a1]) M[(size_t)ec[a1] * q + ec[b1]] += va * ev[b1];      // lower triangle
      if (pred_first && i >= np) rhs[ec[a1]] -= va * u[i];                                                                 // -Bop' Do^-1 (Bo y)
    }
  }
  if (latent) for (int k = 0; k < n; ++k) {               // + Z_o' R^-1 Z_o and the right-hand side Z_o' R^-1 y, R^-1 = diag(w) (:2502-2506)
    const double w = mdl->has_weights ? 1. / mdl->nug_v[k] : 1.;
    M[(size_t)k * q + k] += w;
    rhs[k] = w * yv[k];
  }
  const int sub0 = pred_first ? 0 : n;
  if (second) inv.resize((size_t)np * np);
  if (gpb_hip_dense_spd_solve(q, M.data(), rhs.data(), x.data(), sub0, second ? inv.data() : nullptr)) return shim_error();
  for (int k = 0; k < np; ++k) c.out[k] = x[sub0 + k];
  add_linear_predictor(mdl, c, c.out);
  // latent types: the error variance is ADDED for the response (:2624-2626, 2645-2647); 'order_pred_first' has it in the factor and it is REMOVED for the
  // latent process (re_model_template.h:4134-4150).  (The device's inverse is copied as it is, both triangles: no symmetric store here.)
  const double dshift = latent ? (c.response ? 1. : 0.) : (c.response ? 0. : -1.);
  if (c.var) for (int k = 0; k < np; ++k) c.out[np + k] = c.tr[0] * (inv[(size_t)k * np + k] + dshift);
  if (c.cov) {
    for (size_t k = 0; k < (size_t)np * np; ++k) c.out[np + k] = c.tr[0] * inv[k];
    for (int k = 0; k < np; ++k) c.out[np + (size_t)k * np + k] += c.tr[0] * dshift;
  }
  return 0;
}

/* The Gaussian one-cluster Vecchia model and its five prediction types (c_api.h:1640-1660; SUPPORTED_VECCHIA_PRED_TYPES_GAUSS_ of the reference).  Response and
   offset (SetYCalcCovCalcYAuxForPred, re_model_template.h:11141-11166): with an offset -- the argument, else the one saved by GPB_SetOffsetData (:3601-3607) --
   the residual (y_obs or the stored response as it was passed in, NOT y - offset of the fit) minus the offset becomes the response; with covariates, minus X beta. */
int predict_vecchia_gauss(REModelHip* mdl, PredCall& c) {
  const char* scope = "is not on the MI355X path of this library (prediction: one-cluster Gaussian Vecchia model, 'order_obs_first_cond_obs_only')";
  if (mdl->likelihood != "gaussian" || mdl->eh || mdl->vhs.size() != 1) return set_error("GPB_PredictREModel: this model %s", scope);
  if (pred_refuse_samples_and_moments(c, "posterior / prior samples", scope)) return -1;
  if (c.cluster_ids || c.grouped) return set_error("GPB_PredictREModel: cluster ids / grouped effects / random coefficients for prediction %s", scope);
  if (pred_check_covariates(mdl, c, true, scope)) return -1;
  const std::string& pt = mdl->vecchia_pred_type;
  const bool cond_all = pt == "order_obs_first_cond_all", pred_first = pt == "order_pred_first", latent_all = pt == "latent_order_obs_first_cond_all";
  const bool latent = latent_all || pt == "latent_order_obs_first_cond_obs_only";
  if (pt != "order_obs_first_cond_obs_only" && !cond_all && !pred_first && !latent) return set_error("GPB_PredictREModel: vecchia_pred_type '%s' %s", pt.c_str(), scope);
  if (pred_resolve(mdl, c, PredPath::VecchiaGauss, {Resolve::Coords, Resolve::CovPars, Resolve::Response})) return -1;
  if (prediction_response(mdl, c.y_data, c.fe)) return -1;
  if (mdl->p_cov > 0 && gpb_hip_vecchia_set_resid(mdl->vh, mdl->beta.data())) return shim_error();   // resid -= X beta (:11150-11152); the host copy for the types below
  std::vector<double> resid_v;                          // response the prediction conditions on, Vecchia order
  const double* yv = mdl->ybuf;
  if (mdl->p_cov > 0) {
    resid_v.assign(mdl->ybuf, mdl->ybuf + mdl->n);
    for (int j = 0; j < mdl->p_cov; ++j) for (int k = 0; k < mdl->n; ++k) resid_v[k] -= mdl->X[(size_t)j * mdl->n + mdl->perm[k]] * mdl->beta[j];
    yv = resid_v.data();
  }
  mdl->yaux_valid = false;
  // at most the observed points: every type's own bound (n + np - 1 points to choose from where prediction points are neighbours too) is above that
  const int nnp = pred_neighbor_count(mdl, mdl->n, true);
  if (cond_all) return gauss_cond_all(mdl, c, nnp, yv);
  if (pred_first || latent) return gauss_joint_factor(mdl, c, nnp, yv, pred_first, latent_all);
  return gauss_obs_only(mdl, c, nnp);
}

// ---- several clusters / prediction cluster ids ----

/* Several clusters = independent realisations of the GP (cluster_ids_data of GPB_CreateREModel) and / or cluster ids for the prediction points:
   REModelTemplate::Predict treats every prediction cluster on its own (re_model_template.h:3700-3760) -- a cluster WITH observations conditions on those
   observations only (Case 2, :3940-4330: predict_vecchia_gauss on a view of that cluster's device state); a cluster WITHOUT observations gets the prior
   (Case 1, :3750-3936: mean = fixed effects, covariance sigma1_2 k(.) [+ sigma2 for the response]); no covariance between clusters. */
int predict_clusters(REModelHip* mdl, PredCall& c) {
  const char* scope = "is not on the MI355X path of this library (prediction with cluster ids: Gaussian Vecchia model, no covariates / saved data / samples)";
  if (pred_refuse_samples_and_moments(c, "posterior / prior samples", scope)) return -1;
  if (c.grouped || c.X_pred || mdl->p_cov > 0 || c.use_saved_data)
    return set_error("GPB_PredictREModel: grouped effects / random coefficients / covariates / saved prediction data %s", scope);
  if (!c.cluster_ids) return set_error("Missing cluster_id data ('cluster_ids_pred') for making predictions");   // :3522-3524
  if (pred_resolve(mdl, c, PredPath::Clusters, {Resolve::Coords, Resolve::CovPars, Resolve::Response})) return -1;
  if (prediction_response(mdl, c.y_data, c.fe)) return -1;   // as in the one-cluster path: the residual becomes the response
  mdl->yaux_valid = false;
  // prediction points by cluster, clusters in the order of their first appearance
  const int np = c.np, d = mdl->d;
  std::vector<int32_t> pid; std::vector<std::vector<int>> pidx;
  for (int i = 0; i < np; ++i) {
    size_t k = 0;
    while (k < pid.size() && pid[k] != c.cluster_ids[i]) ++k;
    if (k == pid.size()) { pid.push_back(c.cluster_ids[i]); pidx.emplace_back(); }
    pidx[k].push_back(i);
  }
  if (c.cov) std::fill(c.out + np, c.out + np + (size_t)np * np, 0.);
  for (size_t pc = 0; pc < pid.size(); ++pc) {
    const std::vector<int>& ix = pidx[pc];
    const int npc = (int)ix.size();
    int ci = -1;
    if (mdl->cluster_id_values.empty()) { if (pid[pc] == 0) ci = 0; }
    else for (size_t k = 0; k < mdl->cluster_id_values.size(); ++k) if (mdl->cluster_id_values[k] == pid[pc]) { ci = (int)k; break; }
    std::vector<double> cc((size_t)npc * d), fep;
    for (int j = 0; j < d; ++j) for (int k = 0; k < npc; ++k) cc[(size_t)j * npc + k] = c.cp[(size_t)j * np + ix[k]];
    if (c.fixed_effects_pred) { fep.resize(npc); for (int k = 0; k < npc; ++k) fep[k] = c.fixed_effects_pred[ix[k]]; }
    std::vector<double> outc((size_t)npc * (c.cov ? 1 + (size_t)npc : (c.var ? 2 : 1)), 0.);
    if (ci < 0) {
      // no observations for this cluster: the prior.  The reference builds a Vecchia approximation of the prior among these points (:3760-3838), which is
      // exact for up to num_neighbors + 1 of them; beyond that only the variances are on this path.
      for (int k = 0; k < npc; ++k) outc[k] = c.fixed_effects_pred ? fep[k] : 0.;
      const double vdiag = c.tr[0] * (c.tr[1] + (c.response ? 1. : 0.));
      if (c.var) for (int k = 0; k < npc; ++k) outc[npc + k] = vdiag;
      if (c.cov) {
        if (npc > mdl->num_neighbors + 1) return set_error("GPB_PredictREModel: covariance matrix of %d prediction points in a cluster without observations (more than num_neighbors + 1 = %d) %s", npc, mdl->num_neighbors + 1, scope);
        for (int a1 = 0; a1 < npc; ++a1) for (int b1 = 0; b1 < npc; ++b1)
          outc[npc + (size_t)a1 * npc + b1] = a1 == b1 ? vdiag : c.tr[0] * c.tr[1] * gpb_sm::matern_gaussian_paths(mdl->cov_type, 1., c.tr[2] * std::sqrt(sq_dist(cc.data(), npc, d, a1, b1)));
      }
    } else {
      // a view of cluster ci as a one-cluster model: shares the device state and the resident response, owns nothing
      REModelHip view;
      const auto disown = scope_exit_api([&] { view.vhs.clear(); view.vh = nullptr; view.ybuf = nullptr; view.ybuf_cap = 0; });
      const int o0 = mdl->cl_off[ci], nc = mdl->cl_off[ci + 1] - o0;
      view.n = nc; view.d = d; view.m = mdl->m; view.num_neighbors = mdl->num_neighbors; view.cov_type = mdl->cov_type;
      view.perm.resize(nc); std::iota(view.perm.begin(), view.perm.end(), 0);
      view.vh = mdl->vhs[ci]; view.vhs.assign(1, view.vh); view.cl_off = {0, nc};
      view.has_weights = mdl->has_weights;
      if (mdl->has_weights) view.nug_v.assign(mdl->nug_v.begin() + o0, mdl->nug_v.begin() + o0 + nc);
      view.ybuf = mdl->ybuf + o0; view.ybuf_cap = (size_t)nc; view.y_set = true;
      view.vecchia_pred_type = mdl->vecchia_pred_type; view.num_neighbors_pred = mdl->num_neighbors_pred;
      PredCall sub;
      sub.num_data_pred = npc; sub.out = outc.data(); sub.cov = c.cov; sub.var = c.var; sub.response = c.response;
      sub.coords_given = cc.data(); sub.cov_pars = c.c3; sub.fixed_effects_pred = c.fixed_effects_pred ? fep.data() : nullptr;
      if (predict_vecchia_gauss(&view, sub)) return -1;
    }
    scatter_prediction(c.out, c.var ? c.out + np : nullptr, c.cov ? c.out + np : nullptr, np, npc, ix.data(), nullptr, outc.data(), c.var ? outc.data() + npc : nullptr,
                       c.cov ? outc.data() + npc : nullptr, npc, false);
  }
  return 0;
}

}  // namespace

extern "C" {

/* Host half of the Vecchia prediction 'order_obs_first_cond_all' (CalcPredVecchiaObservedFirstOrder with CondObsOnly = false,
   src/GPBoost/Vecchia_utils.cpp:2061-2090), and test seam for it: given the factor rows of the APPENDED prediction points -- neighbour
   indices into (observed, prediction) points, nn < n_obs + i for row i, -1 padded; A_i = C_nn^-1 c; D_i with the nugget, transformed scale
   (what vecchia_point_kernel<MODE_FACTOR> leaves for them, neighbours searched with end_search_at = -1) --
     mean = Bp^-1 (-Bpo y)          forward substitution: Bp = I - A_pp is unit lower triangular (:2061-2064)
     cov  = sigma2 Bp^-1 Dp Bp^-T   rows of Bp^-1 by the same recursion (:2077-2090); nugget removed from the diagonal unless predict_response
   var_out (n_pred) and cov_out (n_pred x n_pred, row-major) may each be NULL.  Dense in the number of prediction points (the reference keeps
   Bp^-1 sparse): refused above 20000 points.  GPB_PredictREModel reaches it through gauss_cond_all with the device's factor rows. */
int GPB_HIP_PredictCondAllHost(int32_t n_obs, int32_t n_pred, int32_t m, const int32_t* nn_pred, const double* A_pred, const double* D_pred,
                               const double* y_obs, double sigma2, bool predict_response, double* mean_out, double* var_out, double* cov_out) {
  C_API_BEGIN();
  if (!nn_pred || !A_pred || !D_pred || !y_obs || !mean_out || n_obs < 1 || n_pred < 1 || m < 1)
    return set_error("GPB_HIP_PredictCondAllHost: invalid argument");
  const bool need_rows = var_out || cov_out;
  if (need_rows && n_pred > 20000) return set_error("GPB_HIP_PredictCondAllHost: predictive (co)variances for %d points (dense limit: 20000)", n_pred);
  std::vector<double> L(need_rows ? (size_t)n_pred * n_pred : 0, 0.);      // row i of Bp^-1, columns 0..i (lower triangular, row-major full storage)
  std::fill(mean_out, mean_out + n_pred, 0.);
  BpCarry carry;
  carry.mean = mean_out; carry.y_obs = y_obs; carry.rows = need_rows ? L.data() : nullptr;
  if (bp_inverse_rows(n_obs, n_pred, m, nn_pred, A_pred, carry, "GPB_HIP_PredictCondAllHost: row", 0)) return -1;
  if (need_rows) {
    const double* Lp = L.data();
    const size_t ld = (size_t)n_pred;
    write_second_moments(var_out, cov_out, n_pred, sigma2, predict_response ? 0. : -sigma2, [=](int i, int k) {
      double sacc = 0.;
      for (int j = 0; j <= k; ++j) sacc += Lp[i * ld + j] * D_pred[j] * Lp[k * ld + j];
      return sacc;
    });
  }
  C_API_END();
}

/* c_api.h:1588-1610 -- what the prediction paths of this file need is kept: coordinates, prediction type, number of neighbours */
int GPB_SetPredictionData(REModelHandle handle, int32_t num_data_pred, const int32_t* cluster_ids_data_pred, const char* re_group_data_pred,
                          const double* re_group_rand_coef_data_pred, double* gp_coords_data_pred, const double* gp_rand_coef_data_pred,
                          const double* covariate_data_pred, const char* vecchia_pred_type, int num_neighbors_pred,
                          double /*cg_delta_conv_pred*/, int /*nsim_var_pred*/, int /*rank_pred_approx_matrix_lanczos*/) {
  C_API_BEGIN();
  auto* mdl = reinterpret_cast<REModelHip*>(handle);
  if (!mdl) return set_error("GPB_SetPredictionData: null handle");
  const char* scope = "is not on the MI355X path of this library";
  if (cluster_ids_data_pred || re_group_data_pred || re_group_rand_coef_data_pred || gp_rand_coef_data_pred || covariate_data_pred)
    return set_error("GPB_SetPredictionData: cluster ids / grouped effects / random coefficients / covariates for prediction %s", scope);
  if (vecchia_pred_type && vecchia_pred_type[0]) {
    const std::string t = vecchia_pred_type;
    // SUPPORTED_VECCHIA_PRED_TYPES_GAUSS_ of the reference: all five are on the device for the one-cluster Gaussian Vecchia model; the other paths say which they take
    if (t != "order_obs_first_cond_obs_only" && t != "order_obs_first_cond_all" && t != "order_pred_first" &&
        t != "latent_order_obs_first_cond_obs_only" && t != "latent_order_obs_first_cond_all")
      return set_error("Prediction type '%s' is not supported for the Veccia approximation ", t.c_str());
    mdl->vecchia_pred_type = t;
  }
  if (num_neighbors_pred > 0) mdl->num_neighbors_pred = num_neighbors_pred;
  if (gp_coords_data_pred) {
    if (num_data_pred <= 0) return set_error("GPB_SetPredictionData: num_data_pred = %d", num_data_pred);
    mdl->coords_pred.assign(gp_coords_data_pred, gp_coords_data_pred + (size_t)num_data_pred * mdl->d);
    mdl->num_data_pred = num_data_pred;
  }
  C_API_END();
}

/* c_api.h:1640-1660 -- predictive mean and variances or covariance matrix at new locations (REModel::Predict, re_model.cpp:1083-1215): the dispatch over the
   five model paths above; each path's comment says what it computes and from which lines of the reference. */
int GPB_PredictREModel(REModelHandle handle, const double* y_data, int32_t num_data_pred, double* out_predict, bool predict_cov_mat,
                       bool predict_var, bool predict_response, bool sample_posterior, bool sample_prior, int /*num_post_samples*/,
                       int /*num_prior_samples*/, const int32_t* cluster_ids_data_pred, const char* re_group_data_pred,
                       const double* re_group_rand_coef_data_pred, double* gp_coords_data_pred, const double* gp_rand_coef_data_pred,
                       const double* cov_pars, const double* covariate_data_pred, bool use_saved_data, const double* fixed_effects,
                       const double* fixed_effects_pred) {
  C_API_BEGIN();
  auto* mdl = reinterpret_cast<REModelHip*>(handle);
  if (!mdl || !out_predict) return set_error("GPB_PredictREModel: null argument");
  PredCall c;
  c.y_data = y_data; c.num_data_pred = num_data_pred; c.out = out_predict;
  c.cov = predict_cov_mat; c.var = predict_var; c.response = predict_response; c.samples = sample_posterior || sample_prior;
  c.cluster_ids = cluster_ids_data_pred; c.grouped = re_group_data_pred || re_group_rand_coef_data_pred || gp_rand_coef_data_pred;
  c.coords_given = gp_coords_data_pred; c.cov_pars = cov_pars; c.X_pred = covariate_data_pred; c.use_saved_data = use_saved_data;
  c.fixed_effects = fixed_effects; c.fixed_effects_pred = fixed_effects_pred;
  switch (pred_path(mdl, c)) {
    case PredPath::VifGauss: return predict_vif_gauss(mdl, c);
    case PredPath::Laplace: return predict_laplace(mdl, c);
    case PredPath::Exact: return predict_exact(mdl, c);
    case PredPath::Clusters: return predict_clusters(mdl, c);
    case PredPath::VecchiaGauss: return predict_vecchia_gauss(mdl, c);
  }
  C_API_END();
}

/* PredictTrainingDataRandomEffects (re_model.cpp:1217-1275, re_model_template.h:4455-4514): posterior mean of the latent GP at the training locations.
   Gaussian models: b^ = (y - F) - y_aux with y_aux = Psi^-1 (y - F) (:4502-4505); with calc_var the second n entries of out_predict are
   sigma2 (1 - diag(Psi^-1)) (:4508-4514).  Non-Gaussian Vecchia models (:4683-4725): the mode of the latent process, mapped to the data by
   random_effects_indices_of_data_ if locations repeat, and -- calc_var -- diag((Sigma^-1 + W)^-1) (CalcVarLaplaceApproxVecchia): exact, one block solve per
   52 random effects. */
int GPB_PredictREModelTrainingDataRandomEffects(REModelHandle handle, const double* cov_pars_pred, const double* y_obs, double* out_predict,
                                                const double* fixed_effects, bool calc_var) {
  C_API_BEGIN();
  auto* mdl = reinterpret_cast<REModelHip*>(handle);
  if (!mdl || !out_predict) return set_error("GPB_PredictREModelTrainingDataRandomEffects: null argument");
  // re_model.cpp / re_model_template.h: the reference refuses this call for the approximation, Gaussian or not -- the same words
  if (mdl->vif) return set_error("PredictTrainingDataRandomEffects() is currently not implemented for the 'full_scale_vecchia' approximation. Call the predict() function instead ");
  const char* no_response = "Response variable data is not provided and has not been set before";   // :4473-4477
  if (mdl->likelihood != "gaussian") {
    if (mdl->eh || mdl->vhs.size() != 1) return set_error("GPB_PredictREModelTrainingDataRandomEffects: this model is not on the MI355X path of this library");
    double s12, rho, a_tr;
    if (pred_cov_pars_laplace(mdl, cov_pars_pred, &s12, &rho, &a_tr)) return -1;
    std::vector<double> fe_lin;                  // + X beta of a model fitted with covariates
    const double* fel = location_parameter(mdl, pred_offset(mdl, fixed_effects), &fe_lin);
    if (y_obs) { if (laplace_upload_data(mdl, y_obs, fel)) return -1; }
    else {
      if (!mdl->y_set) return set_error("%s", no_response);
      if (laplace_upload_fixed_effects(mdl, fel)) return -1;
    }
    const int nr = mdl->n_re > 0 ? mdl->n_re : mdl->n;
    if (calc_var && nr > 20000) return set_error("GPB_PredictREModelTrainingDataRandomEffects: variances for %d random effects of a non-Gaussian model (one block solve per 52 of them; limit 20000)", nr);
    std::vector<double> mode(nr), var(calc_var ? nr : 0);
    if (laplace_prepare_preconditioner(mdl)) return -1;
    if (gpb_hip_vecchia_laplace_logit(mdl->vh, mdl->cov_type, s12, a_tr, mdl->num_rand_vec_trace, mdl->seed_rand_vec_trace, mdl->cg_max_num_it,
                                      mdl->cg_max_num_it_tridiag, mdl->cg_delta_conv, mdl->delta_conv_mode_finding, 1, mdl->lap_info, mode.data()))
      return shim_error();
    if (calc_var && gpb_hip_vecchia_laplace_mode_var(mdl->vh, mdl->cg_max_num_it, kPredVarCgTol, var.data(), nullptr)) return shim_error();
    for (int k = 0; k < mdl->n; ++k) {
      const int r = mdl->n_re > 0 ? mdl->re_of[k] : k;
      out_predict[mdl->perm[k]] = mode[r];
      if (calc_var) out_predict[(size_t)mdl->n + mdl->perm[k]] = var[r];
    }
    return 0;
  }
  double cp[3];
  if (pred_cov_pars_original(mdl, cov_pars_pred, cp)) return -1;
  const double* fe = pred_offset(mdl, fixed_effects);
  std::vector<double> yc(mdl->n), ya(mdl->n);
  if (y_obs) { for (int i = 0; i < mdl->n; ++i) yc[i] = y_obs[i] - (fe ? fe[i] : 0.); }
  else {
    if (!mdl->y_set) return set_error("%s", no_response);
    for (int i = 0; i < mdl->n; ++i) yc[i] = mdl->y_host[i] - (fe ? fe[i] : 0.);   // y_vec_ - fixed effects (:11143-11160)
  }
  {
    std::vector<double> y_keep;                   // yc is a residual, not a response: y_vec_ stays what the caller passed in last
    if (!y_obs) y_keep.swap(mdl->y_host);
    const int rc = GPB_HIP_CalcYAux(handle, yc.data(), cp, ya.data());
    if (!y_obs) mdl->y_host.swap(y_keep); else mdl->y_host.assign(y_obs, y_obs + mdl->n);
    if (rc) return -1;
  }
  for (int i = 0; i < mdl->n; ++i) out_predict[i] = yc[i] - ya[i];
  if (calc_var) {
    std::vector<double> dg(mdl->n);      // diag(Psi_t^-1), Vecchia order
    if (mdl->eh) {   // exact GP: Cov[b | y] = Sigma - Sigma Psi^-1 Sigma = sigma2 (I - Psi_t^-1) (the dense branch's M_aux products, :4515-4620)
      double trx[3];
      if (transform_cov_pars(mdl, cp, trx)) return -1;
      if (gpb_hip_exact_psi_inv_diag(mdl->eh, mdl->cov_type, trx[1], trx[2], dg.data())) return shim_error();
    } else {         // :4508-4514: sigma2 (1 - column sums of B o (D^-1 B)) = sigma2 (1 - diag(B' D^-1 B)); the factor of CalcYAux is resident
      for (size_t cl = 0; cl < mdl->vhs.size(); ++cl)
        if (gpb_hip_vecchia_psi_inv_diag(mdl->vhs[cl], dg.data() + mdl->cl_off[cl])) return shim_error();
      mdl->yaux_valid = false;                            // the diagonal pass used the y_aux scratch vector
    }
    for (int k = 0; k < mdl->n; ++k) out_predict[mdl->n + mdl->perm[k]] = cp[0] * (1. - dg[k]);
  }
  C_API_END();
}

}  // extern "C"
