// TEST INFRASTRUCTURE (tests/test_optim_trace.py; make -C tests/optim_trace): a stand-alone program that drives every entry point of
// gpboost_amd/csrc/gpb_optim.h -- the four fits and the three standard-error routines -- with small synthetic evaluators and prints every
// callback it receives (stdout: one line per call with the op and every argument in %a form; one result line per fit).  The library's own
// trace lines and warnings go to stderr.  tests/golden/optim_trace_parent.txt.gz holds both streams as recorded before gpb_optim.cpp was
// reorganised around one lbfgs driver; the test demands them byte for byte.
//
// Evaluators (closed form, + - * / sqrt exp log only):
//   Gaussian   a sum over independent pairs of points at distance d: Psi = I + ratio [[1, c], [c, 1]], c = exp(-a d), eigenvalues
//              1 + ratio (1 +- c) -> y' Psi^-1 y, log det Psi and their derivatives in the seven-sum layout
//   Laplace    a quadratic in (log var, log a) plus a term in a "mode" m that every op 0 / 1 moves half way to a target; ops 3 / 4 set it
//              back / to zero, so resets show in later values.  With fixed effects: + sum (F_i - y_i)^2 / 2; with auxiliary parameters:
//              + sum c_j (log aux_j - t_j)^2 / 2
// A schedule perturbs single calls (by call index): add to the value, NaN, evaluator error, scaled or zero gradient.
#include "gpb_optim.h"

#include <cmath>
#include <cstdio>
#include <cstring>
#include <limits>
#include <vector>

namespace {
enum Kind { ADD, SETNAN, ERR, GRADMUL, ZEROGRAD };
struct Pert { int from, until, kind; double v; };
struct Sched {
  std::vector<Pert> p; int calls = 0;
  const Pert* find(int c, int kind) const { for (const Pert& q : p) if (q.kind == kind && c >= q.from && c < q.until) return &q; return nullptr; }
};
const double kNaN = std::numeric_limits<double>::quiet_NaN();
const double kInf = std::numeric_limits<double>::infinity();

void print_vec(const char* name, const double* v, int n) {
  std::printf(" %s=[", name);
  if (!v) std::printf("null");
  else for (int i = 0; i < n; ++i) std::printf(i ? " %a" : "%a", v[i]);
  std::printf("]");
}

// ---------------------------------------------------------------- Gaussian
const int kPairs = 8;
const double kDist[kPairs] = {0.1, 0.25, 0.5, 0.9, 0.05, 0.15, 0.08, 1.5};
const double kY1[kPairs] = {1.2, -0.8, 0.5, 0.9, -1.5, 0.3, 2.0, -0.4};
const double kY2[kPairs] = {1.0, -1.1, -0.2, -1.3, -1.2, 0.6, 1.6, 0.7};

struct Gauss { Sched s; double slope = 0.; int lag_calls = 0; };

void gauss_sums(double r, double a, double yscale, double slope, double* t) {
  for (int i = 0; i < 7; ++i) t[i] = 0.;
  for (int k = 0; k < kPairs; ++k) {
    const double d = kDist[k], c = std::exp(-a * d), y1 = yscale * kY1[k], y2 = yscale * kY2[k];
    const double u = (y1 + y2) * (y1 + y2) / 2., v = (y1 - y2) * (y1 - y2) / 2.;
    const double lp = 1. + r * (1. + c), lm = 1. + r * (1. - c);
    t[0] += u / lp + v / lm;
    t[1] += std::log(lp) + std::log(lm);
    t[3] += 0.5 * r * (-u * (1. + c) / (lp * lp) - v * (1. - c) / (lm * lm));
    t[4] += 0.5 * r * ((1. + c) / lp + (1. - c) / lm);
    t[5] += 0.5 * a * (r * d * c * (u / (lp * lp) - v / (lm * lm)));
    t[6] += 0.5 * a * (r * d * c * (1. / lm - 1. / lp));
  }
  if (slope != 0.) { t[1] += slope * std::log(r); t[4] += 0.5 * slope; }
}

int perturb_gauss(const Sched& s, int c, double* t) {
  if (s.find(c, ERR)) { std::printf(" -> error\n"); return -1; }
  if (const Pert* q = s.find(c, ADD)) t[1] += 2. * q->v;
  if (s.find(c, SETNAN)) t[0] = kNaN;
  if (const Pert* q = s.find(c, GRADMUL)) for (int i = 3; i < 7; ++i) t[i] *= q->v;
  if (s.find(c, ZEROGRAD)) for (int i = 3; i < 7; ++i) t[i] = 0.;
  std::printf("\n");
  return 0;
}

int gauss_terms(void* ctx, double r, double a, int with_grad, double* t) {
  Gauss& g = *(Gauss*)ctx;
  const int c = g.s.calls++;
  std::printf("  G %d terms ratio=%a a=%a with_grad=%d", c, r, a, with_grad);
  gauss_sums(r, a, 1., g.slope, t);
  return perturb_gauss(g.s, c, t);
}
int gauss_coef_update(void* ctx, double r, double a, double* t) {   // "new residual": the response shrunk by 5 %
  Gauss& g = *(Gauss*)ctx;
  const int c = g.s.calls++;
  std::printf("  G %d coef_update ratio=%a a=%a", c, r, a);
  gauss_sums(r, a, 0.95, g.slope, t);
  return perturb_gauss(g.s, c, t);
}
void gauss_lag(void* ctx, int op) { Gauss& g = *(Gauss*)ctx; std::printf("  G lag %d op=%d\n", g.lag_calls++, op); }

// ---------------------------------------------------------------- Laplace stand-in
struct Lap {
  Sched s;
  double m = 0., mprev = 0.;
  double q11 = 1., q22 = 2., q12 = 0.3, c1 = 0.3, c2 = 1.1, slope = 0.;
  int n = 0; const double* y = nullptr; double gsign = 1.;         // fixed effects
  double ac[8] = {0}, at[8] = {0};                                  // auxiliary parameters: curvature, target of log aux
};

// value and gradient wrt (log var, log a) at the current mode; move: the mode goes half way to its target first
double lap_value(Lap& L, double var, double a, bool move, double* g) {
  const double u = std::log(var) - L.c1, w = std::log(a) - L.c2, tgt = 0.3 * u - 0.2 * w;
  if (move) { L.mprev = L.m; L.m = L.m + 0.5 * (tgt - L.m); }
  const double e = L.m - tgt;
  g[0] = L.q11 * u + L.q12 * w - 0.03 * e + L.slope;
  g[1] = L.q12 * u + L.q22 * w + 0.02 * e;
  return 0.5 * L.q11 * u * u + L.q12 * u * w + 0.5 * L.q22 * w * w + 0.05 * e * e + L.slope * std::log(var) + 3.;
}
bool lap_state_op(Lap& L, int op) {
  if (op == 3) { L.m = L.mprev; std::printf(" (mode back to %a)\n", L.m); return true; }
  if (op == 4) { L.m = 0.; L.mprev = 0.; std::printf(" (mode forgotten)\n"); return true; }
  return false;
}
// common tail: the schedule on value out[0] and gradient entries out[1 .. 1 + ng)
int perturb_lap(Lap& L, int c, double* out, int ng, double* gF) {
  if (L.s.find(c, ERR)) { std::printf(" -> error\n"); return -1; }
  if (const Pert* q = L.s.find(c, ADD)) out[0] += q->v;
  if (L.s.find(c, SETNAN)) out[0] = kNaN;
  if (const Pert* q = L.s.find(c, GRADMUL)) { for (int i = 0; i < ng; ++i) out[1 + i] *= q->v; if (gF) for (int i = 0; i < L.n; ++i) gF[i] *= q->v; }
  if (L.s.find(c, ZEROGRAD)) { for (int i = 0; i < ng; ++i) out[1 + i] = 0.; if (gF) for (int i = 0; i < L.n; ++i) gF[i] = 0.; }
  std::printf(" mode=%a\n", L.m);
  return 0;
}

int lap_fn(void* ctx, int op, double var, double a, double* out3) {
  Lap& L = *(Lap*)ctx;
  std::printf("  L op=%d var=%a a=%a", op, var, a);
  if (lap_state_op(L, op)) return 0;
  const int c = L.s.calls++;
  std::printf(" call=%d", c);
  out3[0] = lap_value(L, var, a, (op & 15) != 2, out3 + 1);
  return perturb_lap(L, c, out3, 2, nullptr);
}

int lap_fe_fn(void* ctx, int op, double var, double a, const double* fe, double* out3, double* gF) {
  Lap& L = *(Lap*)ctx;
  std::printf("  F op=%d var=%a a=%a", op, var, a);
  print_vec("fe", fe, L.n);
  if (lap_state_op(L, op)) return 0;
  const int c = L.s.calls++;
  std::printf(" call=%d", c);
  out3[0] = lap_value(L, var, a, (op & 15) != 2, out3 + 1);
  for (int i = 0; i < L.n; ++i) { const double e = fe[i] - L.y[i]; out3[0] += 0.5 * e * e; gF[i] = L.gsign * e; }
  return perturb_lap(L, c, out3, 2, gF);
}

int lap_aux_fn(void* ctx, int op, double var, double a, const double* aux, int naux, double* out) {
  Lap& L = *(Lap*)ctx;
  std::printf("  A op=%d var=%a a=%a naux=%d", op, var, a, naux);
  print_vec("aux", aux, (op & 15) <= 2 ? naux : 0);
  if (lap_state_op(L, op)) return 0;
  const int c = L.s.calls++;
  std::printf(" call=%d", c);
  out[0] = lap_value(L, var, a, (op & 15) != 2, out + 1);
  for (int j = 0; j < naux; ++j) { const double e = std::log(aux[j]) - L.at[j]; out[0] += 0.5 * L.ac[j] * e * e; out[3 + j] = L.ac[j] * e; }
  return perturb_lap(L, c, out, 2 + naux, nullptr);
}

// ---------------------------------------------------------------- case runners
void header(const char* name) {
  std::printf("== %s\n", name);
  std::fflush(stdout);
  std::fprintf(stderr, "== %s\n", name);
}
GpbOptimConfig cfg_of(const char* optimizer, bool trace = false) {
  GpbOptimConfig c; c.optimizer = optimizer; c.trace = trace; return c;
}

void run_gauss(const char* name, GpbOptimConfig cfg, std::vector<Pert> sched, double t0 = 0.5, double t1 = 2., double t2 = 3., int hooks = 0, double slope = 0.,
               bool null_fn = false) {
  header(name);
  Gauss g; g.s.p = sched; g.slope = slope;
  if (hooks & 1) { cfg.profiled_lag = gauss_lag; cfg.profiled_lag_ctx = &g; }
  if (hooks & 2) { cfg.coef_update = gauss_coef_update; cfg.coef_update_ctx = &g; }
  const double th[3] = {t0, t1, t2};
  GpbOptimResult res; char err[512] = "";
  const int rc = gpb_optimize_gaussian_cov_pars(cfg, 2 * kPairs, null_fn ? nullptr : gauss_terms, &g, th, &res, err, sizeof err);
  std::printf("result rc=%d", rc);
  if (rc == 0) std::printf(" theta=[%a %a %a] num_it=%d negll=%a n_ll=%d n_grad=%d lr=%a", res.theta[0], res.theta[1], res.theta[2], res.num_it, res.negll,
                           res.num_ll_evals, res.num_grad_evals, res.lr_cov_final);
  std::printf(" err='%s'\n", err);
}

void run_lap(const char* name, const GpbOptimConfig& cfg, std::vector<Pert> sched, double t0 = 2., double t1 = 1.5, Lap proto = Lap(), bool null_fn = false) {
  header(name);
  Lap L = proto; L.s.p = sched;
  const double th[2] = {t0, t1};
  GpbLaplaceOptimResult res; char err[512] = "";
  const int rc = gpb_optimize_laplace_cov_pars(cfg, null_fn ? nullptr : lap_fn, &L, th, &res, err, sizeof err);
  std::printf("result rc=%d", rc);
  if (rc == 0) std::printf(" theta=[%a %a] num_it=%d negll=%a n_evals=%d", res.theta[0], res.theta[1], res.num_it, res.negll, res.num_evals);
  std::printf(" err='%s'\n", err);
}

const int kN = 6, kP = 2;
const double kX[kN * kP] = {1., 1., 1., 1., 1., 1., -1.0, -0.4, 0.1, 0.5, 0.8, 1.3};     // column-major: intercept, one covariate
const double kYfe[kN] = {0.2, 0.9, 1.1, 1.8, 2.1, 2.9};
const double kOffset[kN] = {0.1, -0.1, 0.05, 0., 0.2, -0.05};

void run_coef(const char* name, const GpbOptimConfig& cfg, std::vector<Pert> sched, bool learn_cov = true, bool with_offset = true, double t0 = 2., double t1 = 1.5,
              int p = kP, double b0 = 0.5) {
  header(name);
  Lap L; L.s.p = sched; L.n = kN; L.y = kYfe;
  const double th[2] = {t0, t1};
  double beta[kP] = {b0, -0.25};
  GpbLaplaceCoefResult res; char err[512] = "";
  const int rc = gpb_optimize_laplace_coef_cov_pars(cfg, lap_fe_fn, &L, kN, p, kX, with_offset ? kOffset : nullptr, 1., 1., th, beta, &res, err, sizeof err, learn_cov);
  std::printf("result rc=%d", rc);
  if (rc == 0) { std::printf(" theta=[%a %a] num_it=%d negll=%a n_evals=%d", res.theta[0], res.theta[1], res.num_it, res.negll, res.num_evals); print_vec("beta", beta, kP); }
  std::printf(" err='%s'\n", err);
}

Lap aux_proto(int naux) {
  Lap L;
  const double ac[3] = {1.5, 0.8, 2.5}, at[3] = {0.4, -0.3, 1.0};
  for (int j = 0; j < naux && j < 3; ++j) { L.ac[j] = ac[j]; L.at[j] = at[j]; }
  return L;
}
void run_aux(const char* name, const GpbOptimConfig& cfg, std::vector<Pert> sched, int naux = 1, Lap proto = aux_proto(3), double t0 = 2., double t1 = 1.5, double a0 = 2.5,
             bool null_fn = false) {
  header(name);
  Lap L = proto; L.s.p = sched;
  const double th[2] = {t0, t1};
  double aux[8] = {a0, 0.7, 1.9, 1., 1., 1., 1., 1.};
  GpbLaplaceAuxResult res; char err[512] = "";
  const int rc = gpb_optimize_laplace_cov_aux_pars(cfg, null_fn ? nullptr : lap_aux_fn, &L, naux, th, aux, &res, err, sizeof err);
  std::printf("result rc=%d", rc);
  if (rc == 0) { std::printf(" theta=[%a %a] num_it=%d negll=%a n_evals=%d", res.theta[0], res.theta[1], res.num_it, res.negll, res.num_evals); print_vec("aux", aux, naux); }
  std::printf(" err='%s'\n", err);
}

void run_se(const char* name, Lap proto, std::vector<Pert> sched, const int* est, double t0 = 1.4, double t1 = 2.9) {
  header(name);
  Lap L = proto; L.s.p = sched;
  const double th[2] = {t0, t1};
  double se[2] = {-1., -1.}; char err[512] = "";
  const int rc = gpb_laplace_std_errors(lap_fn, &L, th, 1.7, se, err, sizeof err, est);
  std::printf("result rc=%d", rc); print_vec("se", se, 2); std::printf(" err='%s'\n", err);
}
void run_se_aux(const char* name, Lap proto, std::vector<Pert> sched, int naux, const int* est, double a0 = 1.6, double t0 = 1.4) {
  header(name);
  Lap L = proto; L.s.p = sched;
  const double th[2] = {t0, 2.9}, aux[3] = {a0, 0.7, 3.1};
  double se[2] = {-1., -1.}, sea[8] = {-1., -1., -1., -1., -1., -1., -1., -1.}; char err[512] = "";
  const int rc = gpb_laplace_aux_std_errors(lap_aux_fn, &L, th, aux, naux, 1.7, se, sea, err, sizeof err, est);
  std::printf("result rc=%d", rc); print_vec("se_cov", se, 2); print_vec("se_aux", sea, naux < 0 ? 0 : (naux > 8 ? 8 : naux)); std::printf(" err='%s'\n", err);
}
void run_se_coef(const char* name, double gsign, std::vector<Pert> sched, int p = kP) {
  header(name);
  Lap L; L.s.p = sched; L.n = kN; L.y = kYfe; L.gsign = gsign;
  const double th[2] = {1.4, 2.9}, beta[kP] = {1.3, 0.02};
  double se[kP] = {-1., -1.}; char err[512] = "";
  const int rc = gpb_laplace_coef_std_errors(lap_fe_fn, &L, kN, p, kX, kOffset, th, beta, se, err, sizeof err);
  std::printf("result rc=%d", rc); print_vec("se", se, kP); std::printf(" err='%s'\n", err);
}

GpbOptimConfig with(GpbOptimConfig c, int max_iter, double delta = -999., int m = 6) { c.max_iter = max_iter; c.delta_rel_conv_init = delta; c.m_lbfgs = m; return c; }
GpbOptimConfig est(GpbOptimConfig c, int e0, int e1, int e2) { c.estimate_cov_par_index[0] = e0; c.estimate_cov_par_index[1] = e1; c.estimate_cov_par_index[2] = e2; return c; }
GpbOptimConfig crit(GpbOptimConfig c) { c.convergence_criterion = "relative_change_in_parameters"; return c; }
GpbOptimConfig no_nesterov(GpbOptimConfig c) { c.use_nesterov_acc = false; return c; }

void gaussian_cases() {
  run_gauss("gauss lbfgs trace", cfg_of("lbfgs", true), {});
  run_gauss("gauss gradient_descent trace", cfg_of("gradient_descent", true), {});
  run_gauss("gauss gradient_descent no nesterov, parameter criterion", with(crit(no_nesterov(cfg_of("gradient_descent"))), 1000, 1e-3), {});
  run_gauss("gauss nelder_mead trace", cfg_of("nelder_mead", true), {});
  run_gauss("gauss nelder_mead parameter criterion", crit(cfg_of("nelder_mead")), {});
  run_gauss("gauss nelder_mead max_iter 5", with(cfg_of("nelder_mead"), 5), {});
  run_gauss("gauss nelder_mead from log 0", cfg_of("nelder_mead"), {}, 0.5, 1., 3.);
  run_gauss("gauss lbfgs lr_cov_init 0.3", [] { GpbOptimConfig c = cfg_of("lbfgs", true); c.lr_cov_init = 0.3; return c; }(), {});
  run_gauss("gauss lbfgs first trial rejected (small increase: width 1/2)", cfg_of("lbfgs", true), {{1, 2, ADD, 0.5}});
  run_gauss("gauss lbfgs first trial rejected (large increase: width 1/32)", cfg_of("lbfgs", true), {{1, 2, ADD, 1e6}});
  run_gauss("gauss lbfgs line search fails, profiled_lag", cfg_of("lbfgs", true), {{1, 21, ADD, 1e6}}, 0.5, 2., 3., 1);
  run_gauss("gauss lbfgs line search fails in the third iteration, profiled_lag", cfg_of("lbfgs", true), {{3, 23, ADD, 0.25}}, 0.5, 2., 3., 1);
  run_gauss("gauss lbfgs NaN trial", cfg_of("lbfgs", true), {{1, 3, SETNAN, 0.}});
  run_gauss("gauss lbfgs max_iter 2", with(cfg_of("lbfgs", true), 2), {});
  run_gauss("gauss gradient_descent max_iter 2", with(cfg_of("gradient_descent", true), 2), {});
  run_gauss("gauss lbfgs zero gradient at the first point", cfg_of("lbfgs", true), {{0, 1, ZEROGRAD, 0.}});
  for (const char* o : {"lbfgs", "gradient_descent", "nelder_mead"}) { char nm[64]; std::snprintf(nm, sizeof nm, "gauss %s max_iter 0", o); run_gauss(nm, with(cfg_of(o), 0), {}); }
  run_gauss("gauss lbfgs m_lbfgs 1", with(cfg_of("lbfgs", true), 1000, 1e-15, 1), {}, 0.5, 0.2, 20.);
  run_gauss("gauss lbfgs m_lbfgs 2", with(cfg_of("lbfgs", true), 1000, 1e-15, 2), {}, 0.5, 0.2, 20.);
  run_gauss("gauss lbfgs m_lbfgs default, many iterations", with(cfg_of("lbfgs", true), 1000, 1e-15), {}, 0.5, 0.2, 20.);
  run_gauss("gauss lbfgs correction skipped", cfg_of("lbfgs", true), {{1, 2, GRADMUL, 3.}});
  run_gauss("gauss lbfgs nugget fixed", est(cfg_of("lbfgs", true), 0, 1, 1), {});
  run_gauss("gauss lbfgs variance fixed, nugget free", est(cfg_of("lbfgs", true), 1, 0, 1), {});
  run_gauss("gauss lbfgs range fixed", est(cfg_of("lbfgs", true), 1, 1, 0), {});
  run_gauss("gauss gradient_descent nugget fixed", est(cfg_of("gradient_descent", true), 0, 1, 1), {});
  run_gauss("gauss gradient_descent variance fixed, nugget free", with(est(cfg_of("gradient_descent", true), 1, 0, 1), 40), {});
  run_gauss("gauss nelder_mead with a fixed parameter", est(cfg_of("nelder_mead"), 1, 0, 1), {});
  run_gauss("gauss gradient_descent coef_update", cfg_of("gradient_descent", true), {}, 0.5, 2., 3., 2);
  run_gauss("gauss gradient_descent nesterov_schedule_version 1", [] { GpbOptimConfig c = cfg_of("gradient_descent"); c.nesterov_schedule_version = 1; return c; }(), {});
  run_gauss("gauss gradient_descent halving", with(cfg_of("gradient_descent", true), 30), {{1, 4, ADD, 5.}});
  run_gauss("gauss lbfgs -Inf -> restart with nelder_mead", with(cfg_of("lbfgs", true), 3), {{1, 4, ADD, -kInf}});
  run_gauss("gauss lbfgs -Inf -> restart, variance fixed, own tolerance", est(with(cfg_of("lbfgs", true), 3, 1e-4), 1, 0, 1), {{1, 4, ADD, -kInf}});
  run_gauss("gauss gradient_descent NaN -> restart with nelder_mead", cfg_of("gradient_descent", true), {{1, 31, SETNAN, 0.}});
  run_gauss("gauss lbfgs NaN at the initial point", cfg_of("lbfgs"), {{0, 1, SETNAN, 0.}});
  run_gauss("gauss lbfgs Inf at the initial point", cfg_of("lbfgs"), {{0, 1, ADD, kInf}});
  run_gauss("gauss gradient_descent NaN at the initial point", cfg_of("gradient_descent"), {{0, 1, SETNAN, 0.}});
  run_gauss("gauss lbfgs evaluator error at the initial point", cfg_of("lbfgs"), {{0, 1, ERR, 0.}});
  run_gauss("gauss lbfgs evaluator error at a trial", cfg_of("lbfgs"), {{2, 3, ERR, 0.}});
  run_gauss("gauss lbfgs evaluator error at the gradient after a rejected trial", cfg_of("lbfgs"), {{1, 2, ADD, 0.5}, {3, 4, ERR, 0.}});
  run_gauss("gauss gradient_descent evaluator error", cfg_of("gradient_descent"), {{2, 3, ERR, 0.}});
  run_gauss("gauss nelder_mead evaluator error at the first vertex", cfg_of("nelder_mead"), {{0, 1, ERR, 0.}});
  run_gauss("gauss nelder_mead evaluator error at later vertices", with(cfg_of("nelder_mead", true), 12), {{2, 3, ERR, 0.}, {5, 7, ERR, 0.}});
  run_gauss("gauss nelder_mead NaN vertices", with(cfg_of("nelder_mead"), 12), {{1, 2, SETNAN, 0.}, {4, 6, SETNAN, 0.}});
  run_gauss("gauss nelder_mead NaN at the solution", with(cfg_of("nelder_mead"), 3), {{4, 400, SETNAN, 0.}});
  run_gauss("gauss nelder_mead ratio driven to zero", cfg_of("nelder_mead"), {}, 0.5, 1e-300, 3., 0, 1e4);
  run_gauss("gauss lbfgs ratio driven to zero", cfg_of("lbfgs"), {}, 0.5, 1e-305, 3., 0, 1e4);
  run_gauss("gauss null evaluator", cfg_of("lbfgs"), {}, 0.5, 2., 3., 0, 0., true);
  run_gauss("gauss non-positive initial value", cfg_of("lbfgs"), {}, 0.5, 0., 3.);
  run_gauss("gauss NaN initial value", cfg_of("lbfgs"), {}, kNaN, 1., 3.);
  run_gauss("gauss unsupported optimizer", cfg_of("adam"), {});
}

void laplace_cases() {
  run_lap("laplace lbfgs trace", cfg_of("lbfgs", true), {});
  run_lap("laplace gradient_descent trace", cfg_of("gradient_descent", true), {});
  run_lap("laplace gradient_descent no nesterov, parameter criterion", crit(no_nesterov(cfg_of("gradient_descent", true))), {});
  run_lap("laplace nelder_mead trace", cfg_of("nelder_mead", true), {});
  run_lap("laplace nelder_mead parameter criterion", crit(cfg_of("nelder_mead")), {});
  run_lap("laplace nelder_mead max_iter 5", with(cfg_of("nelder_mead"), 5), {});
  run_lap("laplace lbfgs first trial rejected (width 1/2)", cfg_of("lbfgs", true), {{1, 2, ADD, 0.5}});
  run_lap("laplace lbfgs first trial rejected (width 1/32)", cfg_of("lbfgs", true), {{1, 2, ADD, 1e6}});
  run_lap("laplace lbfgs line search fails", cfg_of("lbfgs", true), {{1, 21, ADD, 1e6}});
  run_lap("laplace lbfgs line search fails in the third iteration", cfg_of("lbfgs", true), {{3, 23, ADD, 0.25}});
  run_lap("laplace lbfgs NaN trial", cfg_of("lbfgs", true), {{1, 3, SETNAN, 0.}});
  run_lap("laplace lbfgs max_iter 2", with(cfg_of("lbfgs", true), 2), {});
  run_lap("laplace gradient_descent max_iter 2", with(cfg_of("gradient_descent", true), 2), {});
  run_lap("laplace lbfgs zero gradient at the first point", cfg_of("lbfgs", true), {{0, 1, ZEROGRAD, 0.}});
  for (const char* o : {"lbfgs", "gradient_descent", "nelder_mead"}) { char nm[64]; std::snprintf(nm, sizeof nm, "laplace %s max_iter 0", o); run_lap(nm, with(cfg_of(o), 0), {}); }
  run_lap("laplace lbfgs m_lbfgs 1", with(cfg_of("lbfgs", true), 1000, 1e-15, 1), {}, 40., 0.05);
  run_lap("laplace lbfgs m_lbfgs 2", with(cfg_of("lbfgs", true), 1000, 1e-15, 2), {}, 40., 0.05);
  run_lap("laplace lbfgs m_lbfgs default, many iterations", with(cfg_of("lbfgs", true), 1000, 1e-15), {}, 40., 0.05);
  run_lap("laplace lbfgs correction skipped", cfg_of("lbfgs", true), {{1, 2, GRADMUL, 3.}});
  run_lap("laplace lbfgs variance fixed", est(cfg_of("lbfgs", true), 0, 1, 1), {});
  run_lap("laplace lbfgs range fixed", est(cfg_of("lbfgs", true), 1, 0, 1), {});
  run_lap("laplace gradient_descent with a fixed parameter", est(cfg_of("gradient_descent"), 1, 0, 1), {});
  run_lap("laplace gradient_descent with a fixed parameter, max_iter 0", with(est(cfg_of("gradient_descent"), 1, 0, 1), 0), {});
  run_lap("laplace gradient_descent nesterov_schedule_version 1", [] { GpbOptimConfig c = cfg_of("gradient_descent"); c.nesterov_schedule_version = 1; return c; }(), {});
  run_lap("laplace gradient_descent halving", cfg_of("gradient_descent", true), {{1, 4, ADD, 5.}});
  run_lap("laplace lbfgs -Inf -> restart with nelder_mead", with(cfg_of("lbfgs", true), 3), {{1, 4, ADD, -kInf}});
  run_lap("laplace lbfgs -Inf -> restart, own tolerance", with(cfg_of("lbfgs", true), 3, 1e-4), {{1, 4, ADD, -kInf}});
  run_lap("laplace gradient_descent NaN -> restart with nelder_mead", cfg_of("gradient_descent", true), {{1, 31, SETNAN, 0.}});
  run_lap("laplace lbfgs NaN at the initial point", cfg_of("lbfgs"), {{0, 1, SETNAN, 0.}});
  run_lap("laplace lbfgs Inf at the initial point", cfg_of("lbfgs"), {{0, 1, ADD, kInf}});
  run_lap("laplace gradient_descent Inf at the initial point", cfg_of("gradient_descent"), {{0, 1, ADD, kInf}});
  run_lap("laplace lbfgs evaluator error at the initial point", cfg_of("lbfgs"), {{0, 1, ERR, 0.}});
  run_lap("laplace lbfgs evaluator error at a trial", cfg_of("lbfgs"), {{2, 3, ERR, 0.}});
  run_lap("laplace lbfgs evaluator error at the gradient after a rejected trial", cfg_of("lbfgs"), {{1, 2, ADD, 0.5}, {3, 4, ERR, 0.}});
  run_lap("laplace gradient_descent evaluator error", cfg_of("gradient_descent"), {{2, 3, ERR, 0.}});
  run_lap("laplace nelder_mead evaluator error at the first vertex", cfg_of("nelder_mead"), {{0, 1, ERR, 0.}});
  run_lap("laplace nelder_mead evaluator error at later vertices", with(cfg_of("nelder_mead", true), 12), {{2, 3, ERR, 0.}, {5, 7, ERR, 0.}});
  run_lap("laplace nelder_mead NaN vertices", with(cfg_of("nelder_mead"), 12), {{1, 2, SETNAN, 0.}, {4, 6, SETNAN, 0.}});
  run_lap("laplace nelder_mead NaN at the solution", with(cfg_of("nelder_mead"), 3), {{4, 400, SETNAN, 0.}});
  { Lap L; L.slope = 1e4; run_lap("laplace nelder_mead variance driven to zero", cfg_of("nelder_mead"), {}, 1e-300, 1.5, L);
    run_lap("laplace lbfgs variance driven to zero", cfg_of("lbfgs"), {}, 1e-305, 1.5, L); }
  run_lap("laplace null evaluator", cfg_of("lbfgs"), {}, 2., 1.5, Lap(), true);
  run_lap("laplace non-positive initial value", cfg_of("lbfgs"), {}, 2., -1.);
  run_lap("laplace unsupported optimizer", cfg_of("adam"), {});
}

void coef_cases() {
  run_coef("coef lbfgs learn_cov trace", cfg_of("lbfgs", true), {});
  run_coef("coef lbfgs learn_cov = false trace", cfg_of("lbfgs", true), {}, false);
  run_coef("coef lbfgs no offset", cfg_of("lbfgs", true), {}, true, false);
  run_coef("coef lbfgs first trial rejected (width 1/2)", cfg_of("lbfgs", true), {{1, 2, ADD, 0.5}});
  run_coef("coef lbfgs first trial rejected (width 1/32)", cfg_of("lbfgs", true), {{1, 2, ADD, 1e6}});
  run_coef("coef lbfgs line search fails", cfg_of("lbfgs", true), {{1, 21, ADD, 1e6}});
  run_coef("coef lbfgs line search fails in the third iteration", cfg_of("lbfgs", true), {{3, 23, ADD, 0.25}});
  run_coef("coef lbfgs line search fails, learn_cov = false", cfg_of("lbfgs", true), {{2, 22, ADD, 1e6}}, false);
  run_coef("coef lbfgs NaN trial", cfg_of("lbfgs", true), {{1, 3, SETNAN, 0.}});
  run_coef("coef lbfgs max_iter 2", with(cfg_of("lbfgs", true), 2), {});
  run_coef("coef lbfgs max_iter 0", with(cfg_of("lbfgs", true), 0), {});
  run_coef("coef lbfgs zero gradient at the first point", cfg_of("lbfgs", true), {{0, 1, ZEROGRAD, 0.}});
  run_coef("coef lbfgs m_lbfgs 1", with(cfg_of("lbfgs", true), 1000, 1e-15, 1), {});
  run_coef("coef lbfgs m_lbfgs 2", with(cfg_of("lbfgs", true), 1000, 1e-15, 2), {});
  run_coef("coef lbfgs correction skipped", cfg_of("lbfgs", true), {{1, 2, GRADMUL, 3.}});
  run_coef("coef lbfgs variance fixed", est(cfg_of("lbfgs", true), 0, 1, 1), {});
  run_coef("coef lbfgs range fixed", est(cfg_of("lbfgs", true), 1, 0, 1), {});
  run_coef("coef lbfgs masks with learn_cov = false", est(cfg_of("lbfgs", true), 0, 0, 1), {}, false);
  run_coef("coef lbfgs -Inf", with(cfg_of("lbfgs", true), 3), {{1, 4, ADD, -kInf}});
  run_coef("coef lbfgs NaN at the initial point", cfg_of("lbfgs"), {{0, 1, SETNAN, 0.}});
  run_coef("coef lbfgs evaluator error at the initial point", cfg_of("lbfgs"), {{0, 1, ERR, 0.}});
  run_coef("coef lbfgs evaluator error at a trial", cfg_of("lbfgs"), {{2, 3, ERR, 0.}});
  run_coef("coef lbfgs evaluator error at the gradient after a rejected trial", cfg_of("lbfgs"), {{1, 2, ADD, 0.5}, {3, 4, ERR, 0.}});
  run_coef("coef invalid argument", cfg_of("lbfgs"), {}, true, true, 2., 1.5, 0);
  run_coef("coef non-positive initial value", cfg_of("lbfgs"), {}, true, true, 0., 1.5);
  run_coef("coef unsupported optimizer", cfg_of("gradient_descent"), {});
  run_coef("coef lbfgs far initial coefficient (step capped by the coefficients)", cfg_of("lbfgs", true), {}, true, true, 2., 1.5, kP, 400.);
}

void aux_cases() {
  run_aux("aux lbfgs trace", cfg_of("lbfgs", true), {});
  run_aux("aux lbfgs three auxiliary parameters", cfg_of("lbfgs", true), {}, 3);
  run_aux("aux gradient_descent trace", cfg_of("gradient_descent", true), {});
  run_aux("aux gradient_descent no nesterov, parameter criterion, two parameters", crit(no_nesterov(cfg_of("gradient_descent", true))), {}, 2);
  run_aux("aux nelder_mead trace", cfg_of("nelder_mead", true), {});
  run_aux("aux nelder_mead parameter criterion, two parameters", crit(cfg_of("nelder_mead")), {}, 2);
  run_aux("aux nelder_mead max_iter 5", with(cfg_of("nelder_mead"), 5), {});
  run_aux("aux nelder_mead max_iter 0", with(cfg_of("nelder_mead"), 0), {});
  run_aux("aux lbfgs max_iter 0", with(cfg_of("lbfgs"), 0), {});
  run_aux("aux lbfgs line search fails", cfg_of("lbfgs", true), {{1, 21, ADD, 1e6}});
  run_aux("aux lbfgs NaN trial", cfg_of("lbfgs", true), {{1, 3, SETNAN, 0.}});
  run_aux("aux lbfgs zero gradient of the auxiliary parameter", cfg_of("lbfgs", true), {}, 1, Lap());
  run_aux("aux lbfgs range fixed", est(cfg_of("lbfgs", true), 1, 0, 1), {});
  run_aux("aux lbfgs -Inf", with(cfg_of("lbfgs", true), 3), {{1, 4, ADD, -kInf}});
  run_aux("aux gradient_descent NaN", cfg_of("gradient_descent"), {{1, 31, SETNAN, 0.}});
  run_aux("aux gradient_descent halving", cfg_of("gradient_descent", true), {{1, 4, ADD, 5.}});
  run_aux("aux gradient_descent small covariance rate set back", with(no_nesterov(cfg_of("gradient_descent", true)), 4), {{2, 16, ADD, 5.}, {17, 18, GRADMUL, 1e7}, {18, 400, ADD, -1e12}});
  run_aux("aux gradient_descent nesterov_schedule_version 1", [] { GpbOptimConfig c = cfg_of("gradient_descent"); c.nesterov_schedule_version = 1; return c; }(), {});
  run_aux("aux gradient_descent Inf at the initial point", cfg_of("gradient_descent"), {{0, 1, ADD, kInf}});
  run_aux("aux gradient_descent evaluator error", cfg_of("gradient_descent"), {{2, 3, ERR, 0.}});
  run_aux("aux lbfgs evaluator error at a trial", cfg_of("lbfgs"), {{2, 3, ERR, 0.}});
  run_aux("aux nelder_mead evaluator error at the first vertex", cfg_of("nelder_mead"), {{0, 1, ERR, 0.}});
  run_aux("aux nelder_mead evaluator error at later vertices", with(cfg_of("nelder_mead", true), 12), {{2, 3, ERR, 0.}, {6, 8, ERR, 0.}});
  run_aux("aux nelder_mead NaN vertices", with(cfg_of("nelder_mead"), 12), {{1, 2, SETNAN, 0.}, {5, 7, SETNAN, 0.}});
  run_aux("aux nelder_mead NaN at the solution", with(cfg_of("nelder_mead"), 3), {{5, 400, SETNAN, 0.}});
  { Lap L = aux_proto(1); L.slope = 1e4; run_aux("aux nelder_mead variance driven to zero", with(cfg_of("nelder_mead"), 60), {}, 1, L, 1e-300); }
  run_aux("aux invalid argument", cfg_of("lbfgs"), {}, 9);
  run_aux("aux null evaluator", cfg_of("lbfgs"), {}, 1, aux_proto(1), 2., 1.5, 2.5, true);
  run_aux("aux non-positive initial value", cfg_of("lbfgs"), {}, 1, aux_proto(1), -2.);
  run_aux("aux non-positive initial auxiliary parameter", cfg_of("lbfgs"), {}, 1, aux_proto(1), 2., 1.5, 0.);
  run_aux("aux unsupported optimizer", cfg_of("adam"), {});
}

void std_error_cases() {
  const int e01[2] = {0, 1}, e10[2] = {1, 0}, e11[2] = {1, 1};
  Lap saddle; saddle.q22 = -2.;
  Lap concave; concave.q11 = -1.;
  run_se("se positive definite", Lap(), {}, nullptr);
  run_se("se positive definite, estimated2 given", Lap(), {}, e11);
  run_se("se not positive definite (determinant)", saddle, {}, nullptr);
  run_se("se not positive definite (first entry)", concave, {}, nullptr);
  run_se("se variance excluded", Lap(), {}, e01);
  run_se("se range excluded", Lap(), {}, e10);
  run_se("se range excluded, negative curvature", concave, {}, e10);
  run_se("se evaluator error", Lap(), {{2, 3, ERR, 0.}}, nullptr);
  run_se("se evaluator error at the restoring call", Lap(), {{4, 5, ERR, 0.}}, nullptr);
  run_se("se non-positive parameter", Lap(), {}, nullptr, 0.);
  header("se null argument");
  { double se[2]; char err[256] = ""; const double th[2] = {1., 1.}; const int rc = gpb_laplace_std_errors(nullptr, nullptr, th, 1., se, err, sizeof err); std::printf("result rc=%d err='%s'\n", rc, err); }

  run_se_aux("se_aux positive definite", aux_proto(3), {}, 1, nullptr);
  run_se_aux("se_aux three auxiliary parameters", aux_proto(3), {}, 3, e11);
  { Lap L = aux_proto(3); L.ac[1] = 0.; run_se_aux("se_aux zero gradient of the second auxiliary parameter", L, {}, 3, nullptr); }
  { Lap L = aux_proto(3); L.ac[0] = -1.; run_se_aux("se_aux negative diagonal entry of an auxiliary parameter", L, {}, 2, nullptr); }
  { Lap L = aux_proto(3); L.q22 = -2.; run_se_aux("se_aux not positive definite", L, {}, 2, nullptr); }
  run_se_aux("se_aux variance excluded", aux_proto(3), {}, 2, e01);
  { Lap L = aux_proto(3); L.ac[0] = 0.; const int e00[2] = {0, 0}; run_se_aux("se_aux nothing estimated", L, {}, 1, e00); }
  run_se_aux("se_aux evaluator error", aux_proto(3), {{3, 4, ERR, 0.}}, 1, nullptr);
  run_se_aux("se_aux evaluator error at the restoring call", aux_proto(3), {{6, 7, ERR, 0.}}, 1, nullptr);
  run_se_aux("se_aux invalid argument", aux_proto(3), {}, 7, nullptr);
  run_se_aux("se_aux non-positive parameter", aux_proto(3), {}, 1, nullptr, -1.);

  run_se_coef("se_coef positive definite", 1., {});
  run_se_coef("se_coef not positive definite", -1., {});
  run_se_coef("se_coef evaluator error", 1., {{1, 2, ERR, 0.}});
  run_se_coef("se_coef invalid argument", 1., {}, 0);
}
}  // namespace

int main() {
  gaussian_cases();
  laplace_cases();
  coef_cases();
  aux_cases();
  std_error_cases();
  return 0;
}
