// TEST ONLY: gpboost_amd/csrc/gpb_smallmat.h behind a C ABI, compiled by tests/test_smallmat.py (ctypes) and by the smallmat_sanitize target of
// tests/mock_shim/Makefile (its own main, tests/smallmat/smallmat_sanitize_main.cpp).  Nothing here computes: every function is one call into the header.
#include "gpb_smallmat.h"

#define SM_EXPORT extern "C" __attribute__((visibility("default")))
namespace sm = gpb_sm;

SM_EXPORT double sm_jitter_mult() { return sm::JITTER_MULT_IP_FITC_FSA; }
SM_EXPORT int sm_cholesky_lower(double* A, int k, int ld, double* sum_log_diag, int* bad) { return sm::cholesky_lower(A, k, ld, sum_log_diag, bad) ? 1 : 0; }
SM_EXPORT void sm_zero_upper(double* A, int k, int ld) { sm::zero_upper(A, k, ld); }
SM_EXPORT void sm_solve_lower(const double* L, int k, int ld, double* x) { sm::solve_lower(L, k, ld, x); }
SM_EXPORT void sm_solve_lower_transposed(const double* L, int k, int ld, double* x) { sm::solve_lower_transposed(L, k, ld, x); }
SM_EXPORT void sm_cholesky_solve(const double* L, int k, int ld, double* x) { sm::cholesky_solve(L, k, ld, x); }
SM_EXPORT void sm_solve_lower_rows(const double* L, int k, int ld, int n, double* rows) { sm::solve_lower_rows(L, k, ld, n, rows); }
SM_EXPORT void sm_tri_inverse_lower(const double* L, int k, int ld, double* X) { sm::tri_inverse_lower(L, k, ld, X); }
SM_EXPORT void sm_spd_inverse_from_tri(const double* X, int k, double* inv) { sm::spd_inverse_from_tri(X, k, inv); }
SM_EXPORT void sm_spd_inverse_by_solves(const double* L, int k, int ld, double* inv) { sm::spd_inverse_by_solves(L, k, ld, inv); }
SM_EXPORT void sm_inverse_diagonal(const double* L, int k, int ld, double* diag) { sm::inverse_diagonal(L, k, ld, diag); }
SM_EXPORT void sm_matmul(const double* A, const double* B, int k, double* C) { sm::matmul(A, B, k, C); }
SM_EXPORT void sm_sym_from_packed(const double* G, int k, double* out) { sm::sym_from_packed(G, k, out); }
// which: 0 value / 1 d/dloga of the Gaussian paths' form, 2 / 3 of the Laplace paths' form
SM_EXPORT double sm_matern(int which, int cov_type, double scale, double r) {
  return which == 0 ? sm::matern_gaussian_paths(cov_type, scale, r) : which == 1 ? sm::matern_gaussian_paths_dloga(cov_type, scale, r)
       : which == 2 ? sm::matern_laplace_paths(cov_type, scale, r) : sm::matern_laplace_paths_dloga(cov_type, scale, r);
}
// centred_at_value: the control variates are centred with *centre, otherwise with their sample mean; out3 = { c, mean of z1, mean of zP }
SM_EXPORT void sm_optimal_c(const double* z1, const double* zP, int t, int centred_at_value, double centre, double* out3) {
  const sm::OptimalC oc = sm::optimal_c(z1, zP, t, centred_at_value ? &centre : nullptr);
  out3[0] = oc.c; out3[1] = oc.mean1; out3[2] = oc.meanP;
}
SM_EXPORT void sm_ip_cov(const double* ip, int k, int d, int row_major_kx3, int laplace_form, int cov_type, double var, double a, double* Sm, double* dSm) {
  sm::ip_cov(ip, k, d, row_major_kx3 ? sm::IpLayout::RowMajorKx3 : sm::IpLayout::ColMajorKxD, laplace_form ? sm::MaternForm::LaplacePaths : sm::MaternForm::GaussianPaths,
             cov_type, var, a, Sm, dSm);
}
