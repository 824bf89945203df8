// gpboost_amd/csrc/dense_kernels.h -- launch interface of dense_kernels.hip (exact GP path)
#pragma once
#include <hip/hip_runtime.h>

namespace gpb {
// P: row-major np x np (np = n rounded up to 64), lower triangle significant
// ld = leading dimension of P (np, or 2 np when Psi is the top-left block of the augmented matrix of the gradient)
hipError_t launch_dense_cov(int cov, bool d3, const double4* pts, int n, int np, int ld, double var, double a, double nugget,
                            const double* gtab, double* P, hipStream_t st);
hipError_t launch_dense_cholesky(double* P, int np, int* info, hipStream_t st, hipStream_t st2 = nullptr, hipEvent_t ev_panels = nullptr,
                                 hipEvent_t ev_rest = nullptr, int ncols = -1);
// work: np doubles of scratch (required); one launch per 64-wide block step over many workgroups
hipError_t launch_dense_solve(const double* P, int n, int np, int ld, const double* y, double* z, double* out, double* x_out,
                              hipStream_t st, double* work);
// exact-GP gradient (re_model_template.h:2016-2040, CalcPsiInv :6586-6614): identity block of the augmented matrix, and the trace /
// quadratic-form sums over the lower tiles ([4][dense_grad_num_tiles(np)] partials, term-major)
hipError_t launch_dense_aug_identity(double* P2, int np, int ld, hipStream_t st);
int dense_grad_num_tiles(int np);
hipError_t launch_dense_grad(int cov, bool d3, const double4* pts, int n, int np, int ld, double var, double a, const double* gtab,
                             const double* P2, const double* ya, double* part, hipStream_t st);
// NLL without a forward substitution: y as row np of an (np + 64)-row matrix (ld >= np + 64, rows np.. zeroed by the caller); after the
// partial factorisation (ncols = np) that row holds z = L^-1 y and [np][np] holds -z'z.  out = {y' Psi^-1 y, log|Psi|}
hipError_t launch_dense_set_yrow(double* P, int n, int np, int ld, const double* y, hipStream_t st);
hipError_t launch_dense_yrow_sums(const double* P, int n, int np, int ld, double* out, hipStream_t st);
hipError_t launch_dense_solve_backward(const double* P, int np, int ld, double* work, double* x_out, hipStream_t st);
// exact-GP prediction: C = var k(pred, obs) as rows row0.. (columns 0..n) of the augmented matrix; a vector as one of its rows
hipError_t launch_dense_cross_cov(int cov, bool d3, const double4* pts, int n, const double4* pred, int n_pred, int ld, double var, double a,
                                  const double* gtab, double* P, int row0, hipStream_t st);
hipError_t launch_dense_set_row(double* P, int n, int ld, int row, const double* y, hipStream_t st);
// exact-GP Fisher information (re_model_template.h:10066-10127): E1 = Sigma and E2 = dSigma / dlog(a) as full n x n blocks at rows row1.. /
// row2.., columns 0.. of the 4 np x 4 np augmented matrix, and the six traces over the blocks of its Schur complement
// ([6][dense_grad_num_tiles(np)] partials, term-major: 00, 10, 20, 11, 21, 22 with 0 = error variance, 1 = variance, 2 = log range)
hipError_t launch_dense_deriv_blocks(int cov, bool d3, const double4* pts, int n, int ld, double var, double a, const double* gtab, double* P,
                                     int row1, int row2, hipStream_t st);
hipError_t launch_dense_fisher_sums(const double* P, int n, int np, int ld, double* part, hipStream_t st);
}  // namespace gpb
