// gpboost_amd/csrc/gpb_smallmat.h -- the k x k host algebra under every GP path (k: inducing points, preconditioner rank, covariates, leaves, the 3 x 3 Fisher
// information), once.  Header-only plain C++17: no HIP, no model types.  Included by gpb_c_api.cpp (+ gpb_predict.inc), gpb_hip.cpp (+ gpb_dense.inc,
// gpb_laplace.inc) and gpb_optim.cpp; tests/smallmat/smallmat_export.cpp exports it to tests/test_smallmat.py, which holds it to tests/smallmat_ref.py bit for bit.
//
// Matrices are row-major double*, `ld` the distance between rows where a site's matrix is wider than k.  Host code is built with -ffp-contract=off, so a result is
// fixed by the ORDER of its operations; every routine states its order, which is the order its former copies at the call sites had.  The routines report failure;
// the site words the message.
#pragma once

#include <algorithm>
#include <cmath>
#include <cstddef>
#include <thread>
#include <vector>

namespace gpb_sm {

// Diagonal multiplier of the inducing-point covariance that is FACTORISED (utils.h:41 of the reference); the caller that factorises applies it.
constexpr double JITTER_MULT_IP_FITC_FSA = 1. + 1e-6;

// body(lo, hi) over [0, n) on a few threads (one below 200000: the k x k loops stay on the caller's thread, the n-vector gathers of the C API do not).
// Ranges are disjoint and every element is computed by one call, so the thread count changes no result.
template <class F>
void parallel_for(int n, F&& body) {
  const int hw = (int)std::thread::hardware_concurrency();
  const int nt = n < 200000 ? 1 : std::max(1, std::min(8, hw > 0 ? hw : 1));
  if (nt == 1) { body(0, n); return; }
  std::vector<std::thread> th;
  th.reserve(nt - 1);
  const int per = (n + nt - 1) / nt;
  for (int t = 1; t < nt; ++t) th.emplace_back([&, t] { body(std::min(n, t * per), std::min(n, (t + 1) * per)); });
  body(0, std::min(n, per));
  for (auto& x : th) x.join();
}

// ---- 1. Cholesky ---------------------------------------------------------------------------------------------------------------------------------------------
// Lower Cholesky factor of the lower triangle of A, in place: L_ij = (A_ij - sum_{p<j} L_ip L_jp) / L_jj, L_jj = sqrt(A_jj - sum_{p<j} L_jp^2), p ascending.
// false: a pivot is not > 0 or not finite (*bad = its index; A is then partly overwritten).  *sum_log_diag = sum_j log L_jj, added in j order (log|A| is twice
// that).  The upper triangle is neither read nor written: a caller whose matrix leaves the function calls zero_upper.
inline bool cholesky_lower(double* A, int k, int ld, double* sum_log_diag = nullptr, int* bad = nullptr) {
  double sl = 0.;
  for (int i = 0; i < k; ++i)
    for (int j = 0; j <= i; ++j) {
      double s = A[(size_t)i * ld + j];
      for (int p = 0; p < j; ++p) s -= A[(size_t)i * ld + p] * A[(size_t)j * ld + p];
      if (i == j) {
        if (!(s > 0.) || !std::isfinite(s)) { if (bad) *bad = i; return false; }
        const double l = std::sqrt(s);
        A[(size_t)i * ld + i] = l; sl += std::log(l);
      } else A[(size_t)i * ld + j] = s / A[(size_t)j * ld + j];
    }
  if (sum_log_diag) *sum_log_diag = sl;
  return true;
}
inline void zero_upper(double* A, int k, int ld) { for (int i = 0; i < k; ++i) for (int j = i + 1; j < k; ++j) A[(size_t)i * ld + j] = 0.; }

// ---- 2. triangular solves, in place ------------------------------------------------------------------------------------------------------------------------
// L x = b: x_i = (b_i - sum_{p<i} L_ip x_p) / L_ii, i and p ascending
inline void solve_lower(const double* L, int k, int ld, double* x) {
  for (int i = 0; i < k; ++i) { double v = x[i]; for (int p = 0; p < i; ++p) v -= L[(size_t)i * ld + p] * x[p]; x[i] = v / L[(size_t)i * ld + i]; }
}
// L' x = b: x_i = (b_i - sum_{p>i} L_pi x_p) / L_ii, i descending, p ascending
inline void solve_lower_transposed(const double* L, int k, int ld, double* x) {
  for (int i = k - 1; i >= 0; --i) { double v = x[i]; for (int p = i + 1; p < k; ++p) v -= L[(size_t)p * ld + i] * x[p]; x[i] = v / L[(size_t)i * ld + i]; }
}
// (L L')^-1 b
inline void cholesky_solve(const double* L, int k, int ld, double* x) { solve_lower(L, k, ld, x); solve_lower_transposed(L, k, ld, x); }
// rows (n x k) <- rows L^-T: every row r becomes L^-1 r
inline void solve_lower_rows(const double* L, int k, int ld, int n, double* rows) { for (int i = 0; i < n; ++i) solve_lower(L, k, ld, rows + (size_t)i * k); }

// ---- 3. L^-1, lower triangular (k x k, the upper triangle zero), column by column: X_ic = (delta_ic - sum_{p=c}^{i-1} L_ip X_pc) / L_ii, p ascending ----------
inline void tri_inverse_lower(const double* L, int k, int ld, double* X) {
  std::fill(X, X + (size_t)k * k, 0.);
  for (int c = 0; c < k; ++c)
    for (int i = c; i < k; ++i) {
      double v = i == c ? 1. : 0.;
      for (int p = c; p < i; ++p) v -= L[(size_t)i * ld + p] * X[(size_t)p * k + c];
      X[(size_t)i * k + c] = v / L[(size_t)i * ld + i];
    }
}

// ---- 4. / 5. the inverse of A = L L', two ways that ROUND DIFFERENTLY (tests/test_smallmat.py asserts that they do): do not swap one for the other ----------
// 4. from X = L^-1: (X' X)_ij = sum_{q=max(i,j)}^{k-1} X_qi X_qj, q ascending, over the lower triangle, mirrored.  Sites: the Gaussian full-scale gradient
//    (vif_terms_core: W^-1, Sigma_m^-1) and the Laplace full-scale gradient (vif_grad_prepare: Sigma_m^-1 of the model and of the fitc preconditioner).
inline void spd_inverse_from_tri(const double* X, int k, double* inv) {
  parallel_for(k, [&](int lo, int hi) {
    for (int i = lo; i < hi; ++i)
      for (int j = 0; j <= i; ++j) {
        double s = 0.;
        for (int q = i; q < k; ++q) s += X[(size_t)q * k + i] * X[(size_t)q * k + j];
        inv[(size_t)i * k + j] = s;
      }
  });
  for (int i = 0; i < k; ++i) for (int j = i + 1; j < k; ++j) inv[(size_t)i * k + j] = inv[(size_t)j * k + i];
}
// 5. by k pairs of solves: column c = cholesky_solve of e_c (the full forward solve: its leading zeros change nothing).  Every entry is written, the result is
//    symmetric only up to rounding.  Sites: the Laplace paths (pc_refresh: the preconditioner's Woodbury inverse; the Woodbury inverses of the mode finding, the
//    log-determinant and the prediction of the full-scale approximation).
inline void spd_inverse_by_solves(const double* L, int k, int ld, double* inv) {
  std::vector<double> x(k);
  for (int c = 0; c < k; ++c) {
    for (int i = 0; i < k; ++i) x[i] = i == c ? 1. : 0.;
    cholesky_solve(L, k, ld, x.data());
    for (int i = 0; i < k; ++i) inv[(size_t)i * k + c] = x[i];
  }
}

// ---- 6. diagonal of the inverse: (A^-1)_cc = || L^-1 e_c ||^2, the column of item 3 with its squares added as they appear (i ascending) -----------------------
inline void inverse_diagonal(const double* L, int k, int ld, double* diag) {
  std::vector<double> col(k);
  for (int c = 0; c < k; ++c) {
    double ss = 0.;
    for (int i = c; i < k; ++i) {
      double v = i == c ? 1. : 0.;
      for (int p = c; p < i; ++p) v -= L[(size_t)i * ld + p] * col[p];
      col[i] = v / L[(size_t)i * ld + i];
      ss += col[i] * col[i];
    }
    diag[c] = ss;
  }
}

// ---- 7. matrix helpers -----------------------------------------------------------------------------------------------------------------------------------------
// C = A B (k x k): C_ij = sum_q A_iq B_qj from 0., q ascending, terms with A_iq == 0 skipped
inline void matmul(const double* A, const double* B, int k, double* C) {
  std::fill(C, C + (size_t)k * k, 0.);
  parallel_for(k, [&](int lo, int hi) {
    for (int i = lo; i < hi; ++i)
      for (int q = 0; q < k; ++q) {
        const double aiq = A[(size_t)i * k + q];
        if (aiq == 0.) continue;
        for (int j = 0; j < k; ++j) C[(size_t)i * k + j] += aiq * B[(size_t)q * k + j];
      }
  });
}
// the symmetric k x k matrix of a packed lower triangle (row p at p (p + 1) / 2)
inline void sym_from_packed(const double* G, int k, double* out) {
  for (int p = 0; p < k; ++p) for (int q = 0; q <= p; ++q) out[(size_t)p * k + q] = out[(size_t)q * k + p] = G[(size_t)p * (p + 1) / 2 + q];
}

// ---- 8. Matern covariance with shape 0.5 / 1.5 / 2.5 (cov_type 0 / 1 / 2) at the scaled distance r = a |x - x'|, and its derivative wrt log a -----------------
// (GradientRangeMaternShape0_5 / 1_5 / 2_5 on the transformed scale, cov_fcts.h:2535-2554).  TWO forms that differ in the last bit -- (scale e^-r) (1 + r)
// against (scale (1 + r)) e^-r -- each what its paths have always computed.  Merging them moves numbers: a change of its own.
enum class MaternForm {
  GaussianPaths,     // gpb_c_api.cpp: full-scale Vecchia with the Gaussian likelihood, prior covariances of the predictions.  A caller that multiplies its variance
                     // in afterwards passes scale = 1.
  LaplacePaths       // gpb_laplace.inc: the fitc preconditioner and the full-scale approximation with non-Gaussian likelihoods
};
inline double matern_gaussian_paths(int cov_type, double scale, double r) {
  const double e = scale * std::exp(-r);
  return cov_type == 0 ? e : (cov_type == 1 ? e * (1. + r) : e * (1. + r + r * r / 3.));
}
inline double matern_gaussian_paths_dloga(int cov_type, double scale, double r) {
  const double e = scale * std::exp(-r);
  return cov_type == 0 ? -r * e : (cov_type == 1 ? -r * r * e : -r * r * (1. + r) * e / 3.);
}
inline double matern_laplace_paths(int cov_type, double scale, double r) {
  if (cov_type == 0) return scale * std::exp(-r);
  if (cov_type == 1) return scale * (1.0 + r) * std::exp(-r);
  return scale * (1.0 + r + r * r / 3.0) * std::exp(-r);
}
inline double matern_laplace_paths_dloga(int cov_type, double scale, double r) {
  if (cov_type == 0) return -scale * r * std::exp(-r);
  if (cov_type == 1) return -scale * r * r * std::exp(-r);
  return -scale * r * r * (1.0 + r) / 3.0 * std::exp(-r);
}

// ---- 9. covariance of k inducing points: Sm (k x k) and, unless null, dSm = d Sm / d log a; the lower triangle is computed and mirrored --------------------------
// r_ij = a sqrt(sum_c (x_ic - x_jc)^2), c ascending.  No jitter: JITTER_MULT_IP_FITC_FSA belongs to the caller that factorises.
enum class IpLayout {
  ColMajorKxD,       // x_ic at ip[c k + i] (gpb_c_api.cpp)
  RowMajorKx3        // x_ic at ip[3 i + c], columns d.. zero: all three differences are added (gpb_laplace.inc)
};
inline void ip_cov(const double* ip, int k, int d, IpLayout layout, MaternForm form, int cov_type, double var, double a, double* Sm, double* dSm) {
  const bool cm = layout == IpLayout::ColMajorKxD, gp = form == MaternForm::GaussianPaths;
  const int nc = cm ? d : 3;
  const size_t sp = cm ? 1 : 3, sc = cm ? (size_t)k : 1;
  for (int i = 0; i < k; ++i)
    for (int j = 0; j <= i; ++j) {
      double s2 = 0.;
      for (int c = 0; c < nc; ++c) { const double t = ip[c * sc + i * sp] - ip[c * sc + j * sp]; s2 += t * t; }
      const double r = a * std::sqrt(s2);
      Sm[(size_t)i * k + j] = Sm[(size_t)j * k + i] = gp ? matern_gaussian_paths(cov_type, var, r) : matern_laplace_paths(cov_type, var, r);
      if (dSm) dSm[(size_t)i * k + j] = dSm[(size_t)j * k + i] = gp ? matern_gaussian_paths_dloga(cov_type, var, r) : matern_laplace_paths_dloga(cov_type, var, r);
    }
}

// ---- 10. optimal coefficient of a control variate (CalcOptimalC, CG_utils.cpp:1053-1090 of the reference): c = cov(z1, zP) / var(zP) over t samples, 1 where the
// variance is 0.  The control variates are centred with *centre (their deterministic expectation) or, centre = null, with their sample mean; z1 always with its
// mean.  Order: both means as running sums over c ascending, then divided by t; cov and var as running sums of the centred products over c ascending, then divided by t.
// The caller scales its samples first; the estimate it forms is mean1 - c (meanP - expectation).
struct OptimalC { double c, mean1, meanP; };
inline OptimalC optimal_c(const double* z1, const double* zP, int t, const double* centre) {
  double m1 = 0., mP = 0.;
  for (int c = 0; c < t; ++c) { m1 += z1[c]; mP += zP[c]; }
  m1 /= t; mP /= t;
  const double cP = centre ? *centre : mP;
  double cov = 0., var = 0.;
  for (int c = 0; c < t; ++c) { const double a1 = z1[c] - m1, b1 = zP[c] - cP; cov += a1 * b1; var += b1 * b1; }
  cov /= t; var /= t;
  return OptimalC{ (var == 0.) ? 1. : cov / var, m1, mP };
}

}  // namespace gpb_sm
