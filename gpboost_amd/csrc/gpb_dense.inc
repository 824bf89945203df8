// gpboost_amd/csrc/gpb_dense.inc -- included at the end of gpb_hip.cpp.
//
// The dense entry points (exact GP, gpb_hip_dense_spd_solve, gpb_hip_dense_cholesky_check): each assembles a matrix, augments it, runs ONE partial
// factorisation and reads sums or blocks of the Schur complement back.  The helpers are what they share; an entry lists what is particular to it.

namespace {

int exact_need_y(const gpb_hip_exact_t* h) { return h->has_y ? 0 : fail("response data has not been set (call gpb_hip_exact_set_y)"); }
// The stream of the look-ahead ("REST") updates of the blocked Cholesky (dense_kernels.hip: launch_dense_cholesky).
// Round 6, measured and NOT adopted (profiles/r06_f_dense_cholesky_cu_mask_not_adopted.log): creating it with a CU mask (hipExtStreamCreateWithCUMask) that leaves 16 compute
// units to the panel chain on the main stream -- a REST update is one 128 x 128 tile per workgroup with 139 KB of LDS, ~55 us each, so its grid occupies every CU and the ~24 small
// launches of a block column's panel chain queue behind it -- made the n = 16 384 factorisation SLOWER, 65.0 against 43.9 ms (masks of 32 / 64 CUs were not honoured: 43.9 ms).
int create_lookahead_stream(hipStream_t* stream2, hipEvent_t* ev_panels, hipEvent_t* ev_rest) {      // ... and the two events that go with it
  HIP_OK(hipStreamCreateWithFlags(stream2, hipStreamNonBlocking));
  HIP_OK(hipEventCreateWithFlags(ev_panels, hipEventDisableTiming));
  HIP_OK(hipEventCreateWithFlags(ev_rest, hipEventDisableTiming));
  return 0;
}
// created at a handle's first factorisation
int exact_lookahead(gpb_hip_exact_t* h) { return h->stream2 ? 0 : create_lookahead_stream(&h->stream2, &h->ev_panels, &h->ev_rest); }

// the augmented matrix [[Psi, .], [I, 0]], (2 np)^2, and the gradient's partial sums, allocated at their first use
int exact_aug_buffers(gpb_hip_exact_t* h) {
  if (h->d_P2) return 0;
  HIP_OK(hipMalloc(&h->d_P2, sizeof(double) * 4 * (size_t)h->np * h->np));
  HIP_OK(hipMalloc(&h->d_gpart, sizeof(double) * 4 * (size_t)gpb::dense_grad_num_tiles(h->np)));
  HIP_OK(hipMalloc(&h->d_g4, sizeof(double) * 8));
  return 0;
}

// zero the info word and the ld x ld matrix P, then Psi = Sigma(var, a) + I into its leading np x np block (re_model_template.h:9273-9287)
int exact_assemble(gpb_hip_exact_t* h, int cov_type, double var, double a, double* P, int ld) {
  HIP_OK(hipMemsetAsync(h->d_info, 0, sizeof(int), h->stream));
  HIP_OK(hipMemsetAsync(P, 0, sizeof(double) * (size_t)ld * ld, h->stream));
  HIP_OK(gpb::launch_dense_cov(cov_type, h->d == 3, h->d_pts, h->n, h->np, ld, var, a, 1.0, h->d_exp_tab, P, h->stream));
  return 0;
}

// The end of every entry: the factorisation's failure word comes back behind the entry's own read-backs, the stream is waited for.
// 0: factorised; 1: `what` is not positive definite (the error text is set); -1: a HIP call failed.
int dense_finish(hipStream_t st, const int* d_info, const char* what) {
  int info = 0;
  HIP_OK(hipMemcpyAsync(&info, d_info, sizeof(int), hipMemcpyDeviceToHost, st));
  HIP_OK(hipStreamSynchronize(st));
  if (info != 0) { fail("the %s is not positive definite (dense Cholesky failed)", what); return 1; }
  return 0;
}

// a Schur complement holds MINUS the wanted matrix in its lower triangle: n x n row-major, negated and mirrored in place
void negate_symmetrise_lower(double* M, int n) {
  for (int i = 0; i < n; ++i) for (int j = 0; j <= i; ++j) { const double v = -M[(size_t)i * n + j]; M[(size_t)i * n + j] = v; M[(size_t)j * n + i] = v; }
}

}  // namespace

extern "C" {

// Dense symmetric positive definite service for the Vecchia prediction types (the conditional precision matrices the reference hands to
// its sparse Cholesky, Vecchia_utils.cpp:2419-2441, 2601-2650): x = M^-1 rhs and / or rows and columns [sub0, n) of M^-1, by the exact-GP
// machinery -- the blocked MFMA Cholesky (dense_kernels.hip); the inverse as the Schur complement of ONE partial factorisation of
// [[M, .], [I, 0]] (-M^-1 in the bottom-right block, as gpb_hip_exact_grad_terms).  M_host: row-major n x n, lower triangle significant.
// inv_sub_host: (n - sub0)^2 row-major, symmetric.  n <= 24000 with the inverse, <= 60000 without.
int gpb_hip_dense_spd_solve(int32_t n, const double* M_host, const double* rhs_host, double* x_host, int32_t sub0, double* inv_sub_host) {
  API_BEGIN();
  if (!M_host || n < 1 || (!x_host && !inv_sub_host) || (x_host && !rhs_host)) return fail("gpb_hip_dense_spd_solve: invalid argument");
  if (check_device()) return -1;
  const bool inv = inv_sub_host != nullptr;
  if (inv && (sub0 < 0 || sub0 >= n)) return fail("gpb_hip_dense_spd_solve: sub0 = %d", sub0);
  if (n > (inv ? 24000 : 60000)) return fail("gpb_hip_dense_spd_solve: n = %d is too large for the dense path (%s)", n, inv ? "inverse: 24000" : "solve: 60000");
  const int np = ((n + 63) / 64) * 64, ld = inv ? 2 * np : np;
  struct Bufs {
    double *P = nullptr, *y = nullptr, *z = nullptr, *x = nullptr, *work = nullptr, *out = nullptr; int* info = nullptr; hipStream_t st = nullptr;
    ~Bufs() { dev_free(P); dev_free(y); dev_free(z); dev_free(x); dev_free(work); dev_free(out); dev_free(info); if (st) (void)hipStreamDestroy(st); }
  } b;
  HIP_OK(hipStreamCreateWithFlags(&b.st, hipStreamNonBlocking));
  HIP_OK(hipMalloc(&b.P, sizeof(double) * (size_t)ld * ld));
  HIP_OK(hipMalloc(&b.y, sizeof(double) * (size_t)np)); HIP_OK(hipMalloc(&b.z, sizeof(double) * (size_t)np));
  HIP_OK(hipMalloc(&b.x, sizeof(double) * (size_t)np)); HIP_OK(hipMalloc(&b.work, sizeof(double) * (size_t)np));
  HIP_OK(hipMalloc(&b.out, sizeof(double) * 2)); HIP_OK(hipMalloc(&b.info, sizeof(int)));
  HIP_OK(hipMemsetAsync(b.P, 0, sizeof(double) * (size_t)ld * ld, b.st));
  HIP_OK(hipMemsetAsync(b.info, 0, sizeof(int), b.st));
  HIP_OK(hipMemsetAsync(b.y, 0, sizeof(double) * (size_t)np, b.st));
  HIP_OK(hipMemcpy2DAsync(b.P, sizeof(double) * (size_t)ld, M_host, sizeof(double) * (size_t)n, sizeof(double) * (size_t)n, (size_t)n, hipMemcpyHostToDevice, b.st));
  if (np > n) {                                    // identity on the padding: the factor of the padded matrix is that of M
    std::vector<double> ones((size_t)(np - n), 1.0);
    HIP_OK(hipMemcpy2DAsync(b.P + (size_t)n * ld + n, sizeof(double) * ((size_t)ld + 1), ones.data(), sizeof(double), sizeof(double), (size_t)(np - n),
                            hipMemcpyHostToDevice, b.st));
    HIP_OK(hipStreamSynchronize(b.st));
  }
  if (rhs_host) HIP_OK(hipMemcpyAsync(b.y, rhs_host, sizeof(double) * (size_t)n, hipMemcpyHostToDevice, b.st));
  if (inv) HIP_OK(gpb::launch_dense_aug_identity(b.P, np, ld, b.st));
  HIP_OK(gpb::launch_dense_cholesky(b.P, ld, b.info, b.st, nullptr, nullptr, nullptr, np));      // no look-ahead: one stream, no events
  if (x_host) HIP_OK(gpb::launch_dense_solve(b.P, n, np, ld, b.y, b.z, b.out, b.x, b.st, b.work));
  if (x_host) HIP_OK(hipMemcpyAsync(x_host, b.x, sizeof(double) * (size_t)n, hipMemcpyDeviceToHost, b.st));
  const int ns = n - sub0;
  if (inv) HIP_OK(hipMemcpy2DAsync(inv_sub_host, sizeof(double) * (size_t)ns, b.P + (size_t)(np + sub0) * ld + np + sub0, sizeof(double) * (size_t)ld,
                                   sizeof(double) * (size_t)ns, (size_t)ns, hipMemcpyDeviceToHost, b.st));
  if (dense_finish(b.st, b.info, "conditional precision matrix")) return -1;
  if (inv) negate_symmetrise_lower(inv_sub_host, ns);
  API_END();
}

// Test entry (tests/test_zz_dense_kernels_gpu.py): what launch_dense_cholesky leaves behind.  The row-major ld x ld matrix goes to the device as it is
// (both triangles), the first ncols columns are factorised -- with the second stream and the two events of the look-ahead when lookahead != 0, with null
// pointers otherwise -- and the whole array comes back: L in the lower triangle of the first ncols columns, the Schur complement in the lower triangle of
// the rest, the strict upper triangle as uploaded.  *info is the device's failure word; info != 0 is NOT an error of this call.
int gpb_hip_dense_cholesky_check(int32_t ld, int32_t ncols, int32_t lookahead, const double* M_host, double* out_host, int32_t* info) {
  API_BEGIN();
  if (!M_host || !out_host || !info) return fail("gpb_hip_dense_cholesky_check: null argument");
  if (ld < 64 || ld % 64 != 0 || ld > 24000 || ncols < 1 || ncols > ld) return fail("gpb_hip_dense_cholesky_check: ld = %d (a multiple of 64, <= 24000), ncols = %d (1..ld)", ld, ncols);
  if (check_device()) return -1;
  struct Bufs {
    double* P = nullptr; int* info = nullptr; hipStream_t st = nullptr, st2 = nullptr; hipEvent_t ev_panels = nullptr, ev_rest = nullptr;
    ~Bufs() { dev_free(P); dev_free(info); for (hipEvent_t ev : { ev_panels, ev_rest }) if (ev) (void)hipEventDestroy(ev); for (hipStream_t s : { st2, st }) if (s) (void)hipStreamDestroy(s); }
  } b;
  const size_t bytes = sizeof(double) * (size_t)ld * ld;
  HIP_OK(hipStreamCreateWithFlags(&b.st, hipStreamNonBlocking));
  if (lookahead && create_lookahead_stream(&b.st2, &b.ev_panels, &b.ev_rest)) return -1;
  HIP_OK(hipMalloc(&b.P, bytes));
  HIP_OK(hipMalloc(&b.info, sizeof(int)));
  HIP_OK(hipMemsetAsync(b.info, 0, sizeof(int), b.st));
  HIP_OK(hipMemcpyAsync(b.P, M_host, bytes, hipMemcpyHostToDevice, b.st));
  HIP_OK(gpb::launch_dense_cholesky(b.P, ld, b.info, b.st, b.st2, b.ev_panels, b.ev_rest, ncols));
  int dev_info = 0;
  HIP_OK(hipMemcpyAsync(&dev_info, b.info, sizeof(int), hipMemcpyDeviceToHost, b.st));
  HIP_OK(hipMemcpyAsync(out_host, b.P, bytes, hipMemcpyDeviceToHost, b.st));
  HIP_OK(hipStreamSynchronize(b.st));
  if (b.st2) HIP_OK(hipStreamSynchronize(b.st2));
  *info = dev_info;
  API_END();
}

// ------------------------------------------------------------------------------------------
int gpb_hip_exact_create(int32_t n, int32_t d, const double* coords_colmajor, gpb_hip_exact_t** out) {
  API_BEGIN();
  if (!out) return fail("gpb_hip_exact_create: out is NULL");
  *out = nullptr;
  if (check_device()) return -1;
  if (n < 1 || d < 1 || d > 3 || !coords_colmajor) return fail("gpb_hip_exact_create: invalid arguments (n = %d, d = %d; d in 1..3)", n, d);
  if (n > 100000) return fail("gpb_hip_exact_create: n = %d is too large for the dense path (use gp_approx = 'vecchia')", n);
  auto* h = new gpb_hip_exact();
  bool built = false;
  const auto drop_half_built = scope_exit([&] { if (!built) gpb_hip_exact_free(h); });
  h->n = n; h->d = d; h->np = ((n + 63) / 64) * 64;
  HIP_OK(hipGetDevice(&h->device));
  {   // the main stream carries the panel chain of the factorisation (latency-bound, the critical path); the look-ahead updates run on
      // stream2 at normal priority
    int lo = 0, hi = 0;
    HIP_OK(hipDeviceGetStreamPriorityRange(&lo, &hi));
    HIP_OK(hipStreamCreateWithPriority(&h->stream, hipStreamNonBlocking, hi));
  }
  const std::vector<double4> pts = pack_points(coords_colmajor, n, d);
  HIP_OK(hipMalloc(&h->d_pts, sizeof(double4) * (size_t)n));
  HIP_OK(hipMemcpy(h->d_pts, pts.data(), sizeof(double4) * (size_t)n, hipMemcpyHostToDevice));
  HIP_OK(hipMalloc(&h->d_P, sizeof(double) * (size_t)(h->np + 64) * (h->np + 64)));     // + the 64-row block that carries y (gpb_hip_exact_nll_terms)
  HIP_OK(hipMalloc(&h->d_y, sizeof(double) * (size_t)h->np));
  HIP_OK(hipMalloc(&h->d_z, sizeof(double) * (size_t)h->np));
  HIP_OK(hipMalloc(&h->d_x, sizeof(double) * (size_t)h->np));
  HIP_OK(hipMalloc(&h->d_work, sizeof(double) * (size_t)h->np));
  HIP_OK(hipMalloc(&h->d_out, sizeof(double) * 2));
  HIP_OK(hipMalloc(&h->d_info, sizeof(int)));
  const std::vector<double> tab = exp_table();
  HIP_OK(hipMalloc(&h->d_exp_tab, GPB_EXP_TAB_SIZE * sizeof(double)));
  HIP_OK(hipMemcpy(h->d_exp_tab, tab.data(), GPB_EXP_TAB_SIZE * sizeof(double), hipMemcpyHostToDevice));
  built = true;
  *out = h;
  API_END();
}

int gpb_hip_exact_free(gpb_hip_exact_t* h) {
  API_BEGIN();
  if (!h) return 0;
  (void)hipSetDevice(h->device);
  if (h->stream) { (void)hipStreamSynchronize(h->stream); (void)hipStreamDestroy(h->stream); }
  if (h->stream2) { (void)hipStreamSynchronize(h->stream2); (void)hipStreamDestroy(h->stream2); }
  if (h->ev_panels) (void)hipEventDestroy(h->ev_panels);
  if (h->ev_rest) (void)hipEventDestroy(h->ev_rest);
  dev_free(h->d_pts); dev_free(h->d_P); dev_free(h->d_y); dev_free(h->d_z); dev_free(h->d_x); dev_free(h->d_out); dev_free(h->d_work);
  dev_free(h->d_exp_tab); dev_free(h->d_info); dev_free(h->d_P2); dev_free(h->d_gpart); dev_free(h->d_g4);
  delete h;
  API_END();
}

int gpb_hip_exact_set_y(gpb_hip_exact_t* h, const double* y_host) {
  API_BEGIN();
  if (!h || !y_host) return fail("null argument");
  HIP_OK(hipSetDevice(h->device));
  HIP_OK(hipMemcpyAsync(h->d_y, y_host, sizeof(double) * (size_t)h->n, hipMemcpyHostToDevice, h->stream));
  HIP_OK(hipStreamSynchronize(h->stream));
  h->has_y = true;
  API_END();
}

int gpb_hip_exact_nll_terms(gpb_hip_exact_t* h, int cov_type, double var, double a, double* out2_host, double* yaux_host,
                            double* ms3) {
  API_BEGIN();
  if (!h || !out2_host) return fail("null argument");
  if (exact_need_y(h) || check_cov_args(cov_type, var, a)) return -1;
  HIP_OK(hipSetDevice(h->device));
  struct Events { hipEvent_t e[4] = {}; ~Events() { for (hipEvent_t ev : e) if (ev) (void)hipEventDestroy(ev); } } evs; hipEvent_t* const e = evs.e;   // released on every way out
  for (auto& ev : evs.e) HIP_OK(hipEventCreate(&ev));
  HIP_OK(hipMemsetAsync(h->d_info, 0, sizeof(int), h->stream));
  HIP_OK(hipEventRecord(e[0], h->stream));
  // Two forms.  yrow (default): y rides along as row np of the (np + 64)-row matrix -- the panel solves of the factorisation leave
  // z = L^-1 y in that row and the trailing update leaves -z'z at [np][np]: no forward substitution (np / 64 launches less; the backward
  // one only when y_aux is asked for).  (Round 2's form -- the np x np matrix and both substitutions -- was removed in round 4.)
  const int ld = h->np + 64;
  HIP_OK(hipMemsetAsync(h->d_P + (size_t)h->np * ld, 0, sizeof(double) * (size_t)64 * ld, h->stream));
  HIP_OK(gpb::launch_dense_cov(cov_type, h->d == 3, h->d_pts, h->n, h->np, ld, var, a, 1.0, h->d_exp_tab, h->d_P, h->stream));   // Psi = Sigma + I (:9273-9287)
  HIP_OK(gpb::launch_dense_set_yrow(h->d_P, h->n, h->np, ld, h->d_y, h->stream));
  HIP_OK(hipEventRecord(e[1], h->stream));
  if (exact_lookahead(h)) return -1;
  HIP_OK(gpb::launch_dense_cholesky(h->d_P, ld, h->d_info, h->stream, h->stream2, h->ev_panels, h->ev_rest, h->np));
  HIP_OK(hipEventRecord(e[2], h->stream));
  HIP_OK(gpb::launch_dense_yrow_sums(h->d_P, h->n, h->np, ld, h->d_out, h->stream));
  if (yaux_host) {
    HIP_OK(hipMemcpyAsync(h->d_work, h->d_P + (size_t)h->np * ld, sizeof(double) * (size_t)h->np, hipMemcpyDeviceToDevice, h->stream));
    HIP_OK(gpb::launch_dense_solve_backward(h->d_P, h->np, ld, h->d_work, h->d_x, h->stream));
  }
  HIP_OK(hipEventRecord(e[3], h->stream));
  HIP_OK(hipMemcpyAsync(out2_host, h->d_out, sizeof(double) * 2, hipMemcpyDeviceToHost, h->stream));
  if (yaux_host) HIP_OK(hipMemcpyAsync(yaux_host, h->d_x, sizeof(double) * (size_t)h->n, hipMemcpyDeviceToHost, h->stream));
  const int rc = dense_finish(h->stream, h->d_info, "covariance matrix");
  if (rc < 0) return -1;
  if (ms3) for (int k = 0; k < 3; ++k) { float ms = 0.f; HIP_OK(hipEventElapsedTime(&ms, e[k], e[k + 1])); ms3[k] = ms; }   // (also of a failed factorisation)
  if (rc) return -1;
  API_END();
}

/* Likelihood terms AND the covariance-parameter gradient sums of the exact (dense) GP: CalcGradPars, dense branch
   (re_model_template.h:2016-2040) with CalcPsiInv (:6586-6614).  Psi^-1 comes out of ONE partial factorisation: the blocked Cholesky run
   on the first np columns of [[Psi, .], [I, 0]] leaves L in the top-left block, L^-T below it and -L^-T L^-1 = -Psi^-1 as the Schur
   complement in the bottom-right block (the same MFMA trailing updates as the factorisation itself).  out7 has the layout of
   gpb_hip_vecchia_grad_terms: {y' Psi^-1 y, log|Psi|, 0, g1_var, g2_var, g1_range, g2_range}, gradient_k = g1_k / sigma2 + g2_k. */
int gpb_hip_exact_grad_terms(gpb_hip_exact_t* h, int cov_type, double var, double a, double* out7_host) {
  API_BEGIN();
  if (!h || !out7_host) return fail("null argument");
  if (exact_need_y(h) || check_cov_args(cov_type, var, a)) return -1;
  if (h->n > 24000) return fail("gpb_hip_exact_grad_terms: n = %d is too large for the dense gradient (the augmented matrix has (2 n)^2 entries); use gp_approx = 'vecchia'", h->n);
  HIP_OK(hipSetDevice(h->device));
  const int np = h->np, ld = 2 * np;
  if (exact_aug_buffers(h) || exact_lookahead(h) || exact_assemble(h, cov_type, var, a, h->d_P2, ld)) return -1;
  HIP_OK(gpb::launch_dense_aug_identity(h->d_P2, np, ld, h->stream));
  HIP_OK(gpb::launch_dense_cholesky(h->d_P2, ld, h->d_info, h->stream, h->stream2, h->ev_panels, h->ev_rest, np));
  HIP_OK(gpb::launch_dense_solve(h->d_P2, h->n, np, ld, h->d_y, h->d_z, h->d_out, h->d_x, h->stream, h->d_work));           // y' Psi^-1 y, log|Psi|, ya = Psi^-1 y
  HIP_OK(gpb::launch_dense_grad(cov_type, h->d == 3, h->d_pts, h->n, np, ld, var, a, h->d_exp_tab, h->d_P2, h->d_x, h->d_gpart, h->stream));
  HIP_OK(gpb::launch_reduce_partials(h->d_gpart, gpb::dense_grad_num_tiles(np), 4, h->d_g4, nullptr, h->stream));
  double o2[2], g4[4];
  HIP_OK(hipMemcpyAsync(o2, h->d_out, sizeof(double) * 2, hipMemcpyDeviceToHost, h->stream));
  HIP_OK(hipMemcpyAsync(g4, h->d_g4, sizeof(double) * 4, hipMemcpyDeviceToHost, h->stream));
  if (dense_finish(h->stream, h->d_info, "covariance matrix")) return -1;
  // g4 = {S.yy, S.W, dS.yy, dS.W} with W = -Psi^-1:  -1/2 ya' dPsi ya  and  1/2 tr(Psi^-1 dPsi) = -1/2 sum dPsi o W
  out7_host[0] = o2[0]; out7_host[1] = o2[1]; out7_host[2] = 0.;
  out7_host[3] = -0.5 * g4[0]; out7_host[4] = -0.5 * g4[1];
  out7_host[5] = -0.5 * g4[2]; out7_host[6] = -0.5 * g4[3];
  API_END();
}

/* diag(Psi^-1) of the exact GP on the transformed scale: the predictive variances of the training-data random effects are sigma2 (1 - diag)
   (PredictTrainingDataRandomEffects, dense branch: Cov[b | y] = Sigma - Sigma Psi^-1 Sigma = sigma2 (I - Psi_t^-1) with Sigma_t = Psi_t - I).  -Psi^-1 is the
   Schur complement of the partial factorisation of [[Psi, .], [I, 0]] (as gpb_hip_exact_grad_terms); its diagonal is copied out.  n <= 24000. */
int gpb_hip_exact_psi_inv_diag(gpb_hip_exact_t* h, int cov_type, double var, double a, double* diag_host) {
  API_BEGIN();
  if (!h || !diag_host) return fail("null argument");
  if (check_cov_args(cov_type, var, a)) return -1;
  if (h->n > 24000) return fail("gpb_hip_exact_psi_inv_diag: n = %d is too large for the dense inverse (the augmented matrix has (2 n)^2 entries)", h->n);
  HIP_OK(hipSetDevice(h->device));
  const int np = h->np, ld = 2 * np;
  if (exact_aug_buffers(h) || exact_lookahead(h) || exact_assemble(h, cov_type, var, a, h->d_P2, ld)) return -1;
  HIP_OK(gpb::launch_dense_aug_identity(h->d_P2, np, ld, h->stream));
  HIP_OK(gpb::launch_dense_cholesky(h->d_P2, ld, h->d_info, h->stream, h->stream2, h->ev_panels, h->ev_rest, np));
  HIP_OK(hipMemcpy2DAsync(diag_host, sizeof(double), h->d_P2 + (size_t)np * ld + np, sizeof(double) * ((size_t)ld + 1), sizeof(double), (size_t)h->n,
                          hipMemcpyDeviceToHost, h->stream));
  if (dense_finish(h->stream, h->d_info, "covariance matrix")) return -1;
  for (int i = 0; i < h->n; ++i) diag_host[i] = -diag_host[i];
  API_END();
}

/* Prediction of the exact GP at new locations (REModelTemplate::Predict, dense Gaussian branch: mean = Sigma_po Psi^-1 y, covariance =
   Sigma_pp - Sigma_po Psi^-1 Sigma_op; re_model_template.h:4239-4330 with CalcPred).  Transformed scale (Psi = Sigma / sigma2 + I): ONE
   partial factorisation (first np columns) of [[Psi, ., .], [C, 0, .], [y', 0, 0]], C = Sigma_po / sigma2, leaves
     mean_out = C Psi^-1 y  (= -Schur[y row][C columns])      q_out = C Psi^-1 C'  (= -Schur[C rows][C columns], n_pred^2 row-major, may be NULL)
   The caller adds the prior covariance of the prediction points and the scale sigma2.  n_pred <= 20000. */
int gpb_hip_exact_predict(gpb_hip_exact_t* h, int cov_type, double var, double a, int32_t n_pred, const double* coords_pred_colmajor,
                          double* mean_out, double* q_out) {
  API_BEGIN();
  if (!h || !coords_pred_colmajor || !mean_out) return fail("null argument");
  if (exact_need_y(h) || check_cov_args(cov_type, var, a)) return -1;
  if (n_pred < 1 || n_pred > 20000) return fail("gpb_hip_exact_predict: n_pred = %d (1..20000)", n_pred);
  HIP_OK(hipSetDevice(h->device));
  const int n = h->n, np = h->np, npp = ((n_pred + 63) / 64) * 64, ld = np + npp + 64, yrow = np + npp;
  struct Bufs { double* P = nullptr; double4* pred = nullptr; ~Bufs() { dev_free(P); dev_free(pred); } } b;
  HIP_OK(hipMalloc(&b.P, sizeof(double) * (size_t)ld * ld));
  HIP_OK(hipMalloc(&b.pred, sizeof(double4) * (size_t)n_pred));
  const std::vector<double4> pp = pack_points(coords_pred_colmajor, n_pred, h->d);
  HIP_OK(hipMemcpyAsync(b.pred, pp.data(), sizeof(double4) * (size_t)n_pred, hipMemcpyHostToDevice, h->stream));
  if (exact_lookahead(h) || exact_assemble(h, cov_type, var, a, b.P, ld)) return -1;
  HIP_OK(gpb::launch_dense_cross_cov(cov_type, h->d == 3, h->d_pts, n, b.pred, n_pred, ld, var, a, h->d_exp_tab, b.P, np, h->stream));
  HIP_OK(gpb::launch_dense_set_row(b.P, n, ld, yrow, h->d_y, h->stream));
  HIP_OK(gpb::launch_dense_cholesky(b.P, ld, h->d_info, h->stream, h->stream2, h->ev_panels, h->ev_rest, np));
  HIP_OK(hipMemcpyAsync(mean_out, b.P + (size_t)yrow * ld + np, sizeof(double) * (size_t)n_pred, hipMemcpyDeviceToHost, h->stream));
  if (q_out) HIP_OK(hipMemcpy2DAsync(q_out, sizeof(double) * (size_t)n_pred, b.P + (size_t)np * ld + np, sizeof(double) * (size_t)ld,
                                     sizeof(double) * (size_t)n_pred, (size_t)n_pred, hipMemcpyDeviceToHost, h->stream));
  if (dense_finish(h->stream, h->d_info, "covariance matrix")) return -1;
  for (int i = 0; i < n_pred; ++i) mean_out[i] = -mean_out[i];
  if (q_out) negate_symmetrise_lower(q_out, n_pred);            // the Schur complement holds -C Psi^-1 C' in its lower triangle
  API_END();
}

/* Standard errors of (sigma2, sigma1_2, rho) of the exact GP from the Fisher information on the ORIGINAL scale: CalcStdDevCovPar ->
   CalcFisherInformation, dense branch with include_error_var, !transf_scale (re_model_template.h:10788-10815, 10066-10127):
   FI_ab = 1/2 tr(P dPsi_a P dPsi_b), P = (sigma2 Psi)^-1, dPsi = {I, Sigma / sigma1_2, d(Sigma)/d rho}.  All six traces come out of ONE partial
   factorisation of a 4 np x 4 np augmented matrix (dense_kernels.hip); with E1 = Sigma_t = ratio k, E2 = dSigma_t / dlog(a) on the transformed
   scale (ratio = sigma1_2 / sigma2, d/d rho = -(1 / rho) d/dlog a) and T_ab the traces over Psi_t = Sigma_t + I:
     FI_00 = T_00 / (2 s^4)          FI_01 = T_10 / (2 s^4 ratio)         FI_02 = -T_20 / (2 s^2 rho)      (s^2 = sigma2)
     FI_11 = T_11 / (2 s^4 ratio^2)  FI_12 = -T_21 / (2 s^2 rho ratio)    FI_22 = T_22 / (2 rho^2)
   se = sqrt(diag(FI^-1)), NaN where FI is not positive definite (as the reference).  n <= 24000 ((4 n)^2 doubles of device memory). */
int gpb_hip_exact_fisher_std_errors(gpb_hip_exact_t* h, int cov_type, double sigma2, double ratio, double a, double rho, double* se3_host) {
  API_BEGIN();
  if (!h || !se3_host) return fail("null argument");
  if (check_cov_type(cov_type)) return -1;
  if (!(sigma2 > 0.) || !(ratio > 0.) || !(a > 0.) || !(rho > 0.)) return fail("covariance parameters must be positive");
  if (h->n > 24000) return fail("gpb_hip_exact_fisher_std_errors: n = %d is too large for the dense Fisher information (the augmented matrix has (4 n)^2 entries); use gp_approx = 'vecchia'", h->n);
  HIP_OK(hipSetDevice(h->device));
  const int np = h->np, ld = 4 * np, ntiles = gpb::dense_grad_num_tiles(np);
  struct Bufs { double *P = nullptr, *part = nullptr, *t6 = nullptr; ~Bufs() { dev_free(P); dev_free(part); dev_free(t6); } } b;
  HIP_OK(hipMalloc(&b.P, sizeof(double) * (size_t)ld * ld));
  HIP_OK(hipMalloc(&b.part, sizeof(double) * 6 * (size_t)ntiles));
  HIP_OK(hipMalloc(&b.t6, sizeof(double) * 8));
  if (exact_lookahead(h) || exact_assemble(h, cov_type, ratio, a, b.P, ld)) return -1;
  HIP_OK(gpb::launch_dense_aug_identity(b.P, np, ld, h->stream));
  HIP_OK(gpb::launch_dense_deriv_blocks(cov_type, h->d == 3, h->d_pts, h->n, ld, ratio, a, h->d_exp_tab, b.P, 2 * np, 3 * np, h->stream));
  HIP_OK(gpb::launch_dense_cholesky(b.P, ld, h->d_info, h->stream, h->stream2, h->ev_panels, h->ev_rest, np));
  HIP_OK(gpb::launch_dense_fisher_sums(b.P, h->n, np, ld, b.part, h->stream));
  HIP_OK(gpb::launch_reduce_partials(b.part, ntiles, 6, b.t6, nullptr, h->stream));
  double T[6];
  HIP_OK(hipMemcpyAsync(T, b.t6, sizeof(double) * 6, hipMemcpyDeviceToHost, h->stream));
  if (dense_finish(h->stream, h->d_info, "covariance matrix")) return -1;
  const double s2 = sigma2, s4 = sigma2 * sigma2;
  double FI[3][3];
  FI[0][0] = T[0] / (2. * s4);
  FI[0][1] = FI[1][0] = T[1] / (2. * s4 * ratio);
  FI[0][2] = FI[2][0] = -T[2] / (2. * s2 * rho);
  FI[1][1] = T[3] / (2. * s4 * ratio * ratio);
  FI[1][2] = FI[2][1] = -T[4] / (2. * s2 * rho * ratio);
  FI[2][2] = T[5] / (2. * rho * rho);
  // sqrt(diag(FI^-1)) through the Cholesky factor (Eigen::LLT in the reference); NaN if it fails
  const double nan = std::numeric_limits<double>::quiet_NaN();
  for (int j = 0; j < 3; ++j) se3_host[j] = nan;
  if (gpb_sm::cholesky_lower(&FI[0][0], 3, 3)) {
    double ss[3];
    gpb_sm::inverse_diagonal(&FI[0][0], 3, 3, ss);
    for (int c = 0; c < 3; ++c) if (std::isfinite(ss[c]) && ss[c] >= 0.) se3_host[c] = std::sqrt(ss[c]);
  }
  API_END();
}

}  // extern "C"
