// gpboost_amd/csrc/lik_table.h -- the likelihoods of the Vecchia-Laplace path, written down ONCE: one row per id.  Kernels, device workspace and
// C API ask this table what a likelihood IS (response, auxiliary parameters, what its information depends on) instead of keeping lists of ids.
// Plain C++17, no HIP: the host-only build of the C API includes it too.  shim._LIKELIHOODS keeps (id, num_aux) per name; a test holds the two together.
#pragma once

namespace gpb {
// The numeric values are the ABI of gpb_hip_vecchia_laplace_set_likelihood: they never change, new likelihoods are appended before kNumLik.
enum Lik : int {
  kBernoulliLogit = 0, kBernoulliProbit = 1, kPoisson = 2, kGamma = 3, kNegativeBinomial = 4, kBeta = 5, kT = 6, kLogNormal = 7,
  kGaussianLatent = 8, kNumLik
};
// What the response may be: decides the storage (int labels / counts, or doubles) and the domain check of the response setters.
enum class Resp : int {
  kBinaryOrProportion,   // int labels in {0, 1} (set_labels), or a real proportion in [0, 1] (set_response_real)
  kCount,                // int counts >= 0; never real-valued
  kPositiveReal,         // real, > 0
  kUnitInterval,         // real, strictly inside (0, 1)
  kFiniteReal            // any finite real value
};
struct LikInfo {
  Lik id;
  const char* name;              // canonical name (C API, python shim)
  Resp resp;
  int num_aux;                   // auxiliary parameters: 0, 1 (aux) or 2 (aux, aux2)
  const char* aux_names;         // as GPB_GetAuxPars returns them, joined with "_SEP_"; "" without auxiliary parameters
  const char* aux_label_set;     // the first parameter in gpb_hip_vecchia_laplace_set_aux_pars' "The %s parameter is not > 0"
  const char* aux_label_init;    // ... and in the init_aux_pars check of GPB_SetOptimConfig (the two sites have always differed for gaussian_latent)
  const char* aux2_label;        // the second parameter in both messages
  bool information_depends_on_mode;   // false: d information / d location = 0 (constant, or Fisher information free of the mode)
  bool single_newton_step;       // the log-likelihood is quadratic in the location: one full Newton step finds the mode
};
constexpr LikInfo kLik[kNumLik] = {
  // id                 name                 response                   aux  aux_names         label (set)       label (init)    2nd    info(mode) one step
  { kBernoulliLogit,   "bernoulli_logit",   Resp::kBinaryOrProportion, 0,   "",               "",               "",             "",    true,      false },
  { kBernoulliProbit,  "bernoulli_probit",  Resp::kBinaryOrProportion, 0,   "",               "",               "",             "",    true,      false },
  { kPoisson,          "poisson",           Resp::kCount,              0,   "",               "",               "",             "",    true,      false },
  { kGamma,            "gamma",             Resp::kPositiveReal,       1,   "shape",          "shape",          "shape",        "",    true,      false },
  { kNegativeBinomial, "negative_binomial", Resp::kCount,              1,   "shape",          "shape",          "shape",        "",    true,      false },
  { kBeta,             "beta",              Resp::kUnitInterval,       1,   "precision",      "shape",          "shape",        "",    true,      false },
  { kT,                "t",                 Resp::kFiniteReal,         2,   "scale_SEP_df",   "scale",          "scale",        "df",  false,     false },
  { kLogNormal,        "lognormal",         Resp::kPositiveReal,       1,   "log_variance",   "log_variance",   "log_variance", "",    false,     false },
  { kGaussianLatent,   "gaussian_latent",   Resp::kFiniteReal,         1,   "error_variance", "error_variance", "shape",        "",    false,     true  },
};
constexpr bool lik_rows_in_order(int i = 0) { return i == kNumLik || (kLik[i].id == i && kLik[i].num_aux >= 0 && kLik[i].num_aux <= 2 && lik_rows_in_order(i + 1)); }
static_assert(lik_rows_in_order(), "row i of kLik carries id i, and LikResp has room for two auxiliary parameters");

constexpr bool lik_valid(int id) { return id >= 0 && id < kNumLik; }
constexpr Resp lik_resp(int id) { return kLik[id].resp; }
constexpr bool lik_accepts_real(int id) { return lik_resp(id) != Resp::kCount; }      // set_response_real is accepted (real-only likelihoods, proportions)
constexpr bool lik_real_only(int id) { return lik_accepts_real(id) && lik_resp(id) != Resp::kBinaryOrProportion; }      // ... and set_labels refused
constexpr int lik_num_aux(int id) { return kLik[id].num_aux; }
constexpr bool lik_has_aux(int id) { return lik_num_aux(id) > 0; }
constexpr bool lik_info_depends_on_mode(int id) { return kLik[id].information_depends_on_mode; }
constexpr bool lik_single_newton_step(int id) { return kLik[id].single_newton_step; }
constexpr const char* lik_name(int id) { return kLik[id].name; }

constexpr bool lik_str_eq(const char* a, const char* b) { for (; *a && *a == *b; ++a, ++b) {} return *a == *b; }
constexpr const char* lik_strip_prefix(const char* s, const char* prefix) {      // "<prefix><rest>" -> rest, else nullptr
  for (; *prefix; ++s, ++prefix) if (*s != *prefix) return nullptr;
  return s;
}
// The one place that maps a likelihood name to its id.  The proportion likelihoods are the Bernoulli kernels with a real response:
// binomial_<link> and quasi_bernoulli_<link> resolve to bernoulli_<link>.  -1: not a likelihood of this path.
constexpr int lik_id_of_name(const char* name) {
  const char* link = lik_strip_prefix(name, "binomial_");
  if (!link) link = lik_strip_prefix(name, "quasi_bernoulli_");
  if (link) return lik_str_eq(link, "logit") ? kBernoulliLogit : (lik_str_eq(link, "probit") ? kBernoulliProbit : -1);
  for (int i = 0; i < kNumLik; ++i) if (lik_str_eq(name, kLik[i].name)) return i;
  return -1;
}
static_assert(lik_id_of_name("t") == kT && lik_id_of_name("binomial_probit") == kBernoulliProbit && lik_id_of_name("tweedie") == -1, "");

}  // namespace gpb
