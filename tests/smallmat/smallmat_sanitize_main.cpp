// TEST ONLY: every routine of gpboost_amd/csrc/gpb_smallmat.h at k = 1, 2, 7 under -fsanitize=address,undefined (target smallmat_sanitize of
// tests/mock_shim/Makefile), with exactly sized heap buffers so that one element too far is a report.  Includes the inputs that must fail.  A stand-alone
// program: never loaded into python.
#include "gpb_smallmat.h"

#include <cstdio>
#include <limits>
#include <vector>

namespace sm = gpb_sm;

static int check(bool ok, const char* what, int k) {
  if (!ok) std::fprintf(stderr, "smallmat_sanitize: %s failed at k = %d\n", what, k);
  return ok ? 0 : 1;
}

static int run(int k) {
  int errs = 0;
  const int ld = k + 2;
  unsigned s = 12345u + (unsigned)k;
  auto rnd = [&]() { s = s * 1664525u + 1013904223u; return (double)(s >> 8) / (double)(1u << 24) - 0.5; };
  std::vector<double> B((size_t)k * k), A((size_t)k * ld, -1.), x(k), rows((size_t)3 * k), X((size_t)k * k), inv((size_t)k * k), inv2((size_t)k * k), dg(k),
      P((size_t)k * k), packed((size_t)k * (k + 1) / 2), sym((size_t)k * k);
  for (auto& v : B) v = rnd();
  for (int i = 0; i < k; ++i) for (int j = 0; j < k; ++j) { double a = i == j ? 1. : 0.; for (int q = 0; q < k; ++q) a += B[(size_t)i * k + q] * B[(size_t)j * k + q]; A[(size_t)i * ld + j] = a; }
  std::vector<double> bad_neg(A), bad_inf(A);
  bad_neg[(size_t)(k - 1) * ld + (k - 1)] = -1.;
  bad_inf[0] = std::numeric_limits<double>::infinity();
  int at = -1;
  errs += check(!sm::cholesky_lower(bad_neg.data(), k, ld, nullptr, &at) && at == k - 1, "cholesky_lower (indefinite input)", k);
  errs += check(!sm::cholesky_lower(bad_inf.data(), k, ld, nullptr, &at) && at == 0, "cholesky_lower (+inf diagonal)", k);
  double sl = 0.;
  errs += check(sm::cholesky_lower(A.data(), k, ld, &sl), "cholesky_lower", k);
  sm::zero_upper(A.data(), k, ld);
  for (auto& v : x) v = rnd();
  for (auto& v : rows) v = rnd();
  sm::solve_lower(A.data(), k, ld, x.data());
  sm::solve_lower_transposed(A.data(), k, ld, x.data());
  sm::cholesky_solve(A.data(), k, ld, x.data());
  sm::solve_lower_rows(A.data(), k, ld, 3, rows.data());
  sm::tri_inverse_lower(A.data(), k, ld, X.data());
  sm::spd_inverse_from_tri(X.data(), k, inv.data());
  sm::spd_inverse_by_solves(A.data(), k, ld, inv2.data());
  sm::inverse_diagonal(A.data(), k, ld, dg.data());
  sm::matmul(inv.data(), inv2.data(), k, P.data());
  for (auto& v : packed) v = rnd();
  sm::sym_from_packed(packed.data(), k, sym.data());
  const sm::OptimalC oc = sm::optimal_c(x.data(), dg.data(), k, nullptr), oc2 = sm::optimal_c(x.data(), dg.data(), k, &sl);      // t = k samples, exactly sized
  errs += check(std::isfinite(oc.c) && std::isfinite(oc2.c) && oc.mean1 == oc2.mean1 && (k > 1 || oc.c == 1.), "optimal_c", k);
  for (int c = 0; c < k; ++c) errs += check(std::isfinite(dg[c]) && dg[c] > 0. && std::fabs(dg[c] - inv[(size_t)c * k + c]) <= 1e-12 * dg[c], "inverse_diagonal against spd_inverse_from_tri", k);
  for (int d = 1; d <= 3; ++d) {
    std::vector<double> cm((size_t)k * d), rm((size_t)k * 3, 0.), Sm((size_t)k * k), dSm((size_t)k * k), Sm2((size_t)k * k);
    for (int i = 0; i < k; ++i) for (int c = 0; c < d; ++c) cm[(size_t)c * k + i] = rm[(size_t)i * 3 + c] = rnd();
    for (int cov = 0; cov < 3; ++cov)
      for (sm::MaternForm f : { sm::MaternForm::GaussianPaths, sm::MaternForm::LaplacePaths }) {
        sm::ip_cov(cm.data(), k, d, sm::IpLayout::ColMajorKxD, f, cov, 0.8, 7.5, Sm.data(), dSm.data());
        sm::ip_cov(rm.data(), k, d, sm::IpLayout::RowMajorKx3, f, cov, 0.8, 7.5, Sm2.data(), nullptr);
        errs += check(Sm == Sm2, "ip_cov: the two layouts", k);
      }
  }
  return errs;
}

int main() {
  int errs = 0;
  for (int k : { 1, 2, 7 }) errs += run(k);
  long sum = 0;
  sm::parallel_for(250000, [&](int lo, int hi) { if (lo == 0) sum = hi; });      // the threaded branch
  errs += check(sum > 0, "parallel_for", 0);
  std::printf("smallmat_sanitize: %s\n", errs ? "FAILED" : "ok");
  return errs ? 1 : 0;
}
