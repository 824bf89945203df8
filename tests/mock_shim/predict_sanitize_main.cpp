// TEST INFRASTRUCTURE (make -C tests/mock_shim predict_sanitize): a stand-alone program for a host sanitizer run of the prediction code
// (gpboost_amd/csrc/gpb_predict.inc).  It is built from gpb_c_api.cpp + gpb_optim.cpp + the CPU restatement of the shim with -fsanitize=address,undefined
// and makes one prediction per path the restatement supports, through the C entry points: the one-cluster Gaussian Vecchia model with its five prediction types
// (variances and covariance matrix), two clusters with a prediction cluster that has no observations, a Vecchia-Laplace model with both latent types and
// repeated prediction locations, training-data random effects, the seam GPB_HIP_PredictCondAllHost, and a few refusals.  Data as tests/predict_paths.py:
// n = 300 points in the unit square, 10 neighbours, 12 prediction points of which six lie within 0.01 of each other, num_neighbors_pred = 8.
#include "gpboost_c_api_subset.h"

#include <cmath>
#include <cstdio>
#include <cstdint>
#include <cstring>
#include <vector>

static uint64_t g_state = 88172645463325252ULL;
static double uni() { g_state ^= g_state << 13; g_state ^= g_state >> 7; g_state ^= g_state << 17; return (double)(g_state >> 11) / 9007199254740992.0; }

static int g_fail = 0;
static void expect(bool ok, const char* what) {
  if (!ok) { std::printf("FAILED: %s -- %s\n", what, LGBM_GetLastError()); ++g_fail; }
}

static REModelHandle create(int n, const double* coords, const char* lik, const int32_t* ids) {
  REModelHandle h = nullptr;
  expect(GPB_CreateREModel(n, ids, nullptr, 0, nullptr, nullptr, 0, nullptr, 1, coords, 2, nullptr, 0, "matern", 1.5, "vecchia", 1., 1., 10, "random", -1, 1.,
                           "kmeans++", lik, -999., "default", 1, -1, true, false, nullptr, 1., &h) == 0, "GPB_CreateREModel");
  return h;
}

static int predict(REModelHandle h, const double* y, int np, double* coords_pred, const double* cov_pars, double* out, bool cov, bool var, bool response,
                   const int32_t* ids_pred = nullptr, const double* fe_pred = nullptr) {
  return GPB_PredictREModel(h, y, np, out, cov, var, response, false, false, 0, 0, ids_pred, nullptr, nullptr, coords_pred, nullptr, cov_pars, nullptr, false, nullptr, fe_pred);
}

int main() {
  const int n = 300, np = 12;
  std::vector<double> co(2 * n), y(n), y01(n), cp(2 * np), fep(np);
  for (int i = 0; i < n; ++i) {
    co[i] = uni(); co[n + i] = uni();
    const double f = 1.2 * std::sin(5 * co[i]) * std::cos(3 * co[n + i]);
    y[i] = f + 0.5 * (uni() - 0.5);
    y01[i] = uni() < 1. / (1. + std::exp(-f)) ? 1. : 0.;
  }
  for (int k = 0; k < np; ++k) {
    if (k < 6) { cp[k] = uni(); cp[np + k] = uni(); }
    else { const double a = 6.283185307179586 * uni(), r = 0.01 * std::sqrt(uni()); cp[k] = 0.5 + r * std::cos(a); cp[np + k] = 0.5 + r * std::sin(a); }
    fep[k] = 0.5 * std::cos(4 * cp[k]);
  }
  double cov3[3] = {0.3, 1.2, 0.15}, cov2[2] = {1.2, 0.15};
  std::vector<double> out((size_t)np * (1 + np));      // exactly what the call may write
  const char* types[5] = {"order_obs_first_cond_obs_only", "order_obs_first_cond_all", "order_pred_first", "latent_order_obs_first_cond_obs_only", "latent_order_obs_first_cond_all"};

  REModelHandle g = create(n, co.data(), "gaussian", nullptr);
  for (const char* t : types) {
    expect(GPB_SetPredictionData(g, 0, nullptr, nullptr, nullptr, nullptr, nullptr, nullptr, t, 8, -1., -1, -1) == 0, "GPB_SetPredictionData");
    expect(predict(g, y.data(), np, cp.data(), cov3, out.data(), false, true, false, nullptr, fep.data()) == 0, t);
    expect(predict(g, y.data(), np, cp.data(), cov3, out.data(), true, false, true) == 0, t);
  }
  expect(GPB_SetPredictionData(g, np, nullptr, nullptr, nullptr, cp.data(), nullptr, nullptr, types[1], 200, -1., -1, -1) == 0, "GPB_SetPredictionData (saved)");
  expect(GPB_PredictREModel(g, nullptr, 0, out.data(), true, false, true, false, false, 0, 0, nullptr, nullptr, nullptr, nullptr, nullptr, cov3, nullptr, true, nullptr, nullptr) == 0,
         "saved data, resident response, 126 neighbours");
  std::vector<double> re(2 * n);
  expect(GPB_PredictREModelTrainingDataRandomEffects(g, cov3, y.data(), re.data(), nullptr, true) == 0, "training-data random effects (Gaussian)");
  expect(predict(g, y.data(), np, cp.data(), cov3, out.data(), true, true, true) != 0, "both second moments are refused");
  expect(predict(g, y.data(), np, nullptr, cov3, out.data(), false, false, true) != 0, "no coordinates is refused");
  expect(GPB_REModelFree(g) == 0, "GPB_REModelFree");

  std::vector<int32_t> ids(n), idp(np);
  for (int i = 0; i < n; ++i) ids[i] = 10 + i % 2;
  for (int k = 0; k < np; ++k) idp[k] = k % 4 < 2 ? 10 + k % 2 : 12;      // six points in a cluster without observations
  REModelHandle cl = create(n, co.data(), "gaussian", ids.data());
  expect(GPB_SetPredictionData(cl, 0, nullptr, nullptr, nullptr, nullptr, nullptr, nullptr, types[1], 8, -1., -1, -1) == 0, "GPB_SetPredictionData (clusters)");
  expect(predict(cl, y.data(), np, cp.data(), cov3, out.data(), true, false, true, idp.data(), fep.data()) == 0, "clusters, covariance matrix");
  expect(predict(cl, y.data(), np, cp.data(), cov3, out.data(), false, true, false, idp.data()) == 0, "clusters, variances");
  expect(GPB_PredictREModelTrainingDataRandomEffects(cl, cov3, y.data(), re.data(), nullptr, true) == 0, "training-data random effects (clusters)");
  expect(GPB_REModelFree(cl) == 0, "GPB_REModelFree");

  std::vector<double> cpd = cp;
  for (int j = 0; j < 2; ++j) { cpd[j * np + 9] = cp[j * np + 0]; cpd[j * np + 10] = cp[j * np + 1]; cpd[j * np + 11] = cp[j * np + 6]; }
  REModelHandle lp = create(n, co.data(), "bernoulli_logit", nullptr);
  for (int t = 3; t < 5; ++t) {
    expect(GPB_SetPredictionData(lp, 0, nullptr, nullptr, nullptr, nullptr, nullptr, nullptr, types[t], 8, -1., -1, -1) == 0, "GPB_SetPredictionData (Laplace)");
    expect(predict(lp, y01.data(), np, cpd.data(), cov2, out.data(), false, true, true, nullptr, fep.data()) == 0, types[t]);
    expect(predict(lp, y01.data(), np, cpd.data(), cov2, out.data(), true, false, false) == 0, types[t]);
  }
  expect(GPB_PredictREModelTrainingDataRandomEffects(lp, cov2, y01.data(), re.data(), nullptr, true) == 0, "training-data random effects (Laplace)");
  expect(GPB_REModelFree(lp) == 0, "GPB_REModelFree");

  // the seam on a hand-made factor: three observed points, four prediction points, two slots, one of them padded
  const int32_t nn[8] = {0, 1, 2, 3, 3, 4, 5, -1};
  const double A[8] = {0.5, 0.25, 0.125, 0.5, 0.25, 0.5, 0.75, 0.}, D[4] = {1.5, 1.25, 1.125, 1.0625}, yo[3] = {1., -2., 3.};
  double mean[4], var[4], cov[16];
  expect(GPB_HIP_PredictCondAllHost(3, 4, 2, nn, A, D, yo, 2., false, mean, var, cov) == 0, "GPB_HIP_PredictCondAllHost");
  const int32_t bad[8] = {0, 1, 2, 4, 3, 4, 5, -1};
  expect(GPB_HIP_PredictCondAllHost(3, 4, 2, bad, A, D, yo, 2., false, mean, var, cov) != 0, "a neighbour that does not precede its point is refused");
  std::printf(g_fail ? "%d call(s) failed\n" : "predict_sanitize: all calls as expected\n", g_fail);
  return g_fail ? 1 : 0;
}
