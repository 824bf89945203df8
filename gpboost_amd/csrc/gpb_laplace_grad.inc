// gpboost_amd/csrc/gpb_laplace_grad.inc -- the gradient half of gpb_laplace.inc, included at its end (same translation unit: LaplaceState, LapWork, LapSolver, lap_cg,
// pc_apply, lap_draw, and the full-scale Vecchia gradient's device reductions VifGradHost, vif_grad_prepare / _block_sums / _vec_sums).
//
// Gradient of the NEGATIVE approximate marginal log-likelihood wrt (log sigma1^2, log a) at the state the last laplace_eval(..., LAP_KEEP_GRAD_STATE) left behind: the mode,
// the factor, W / dw / rdw at the mode, U and PI_Z of the log-determinant's block CG.  gpb_hip_vecchia_laplace_grad_current is a list of stages over one LapGrad context:
//   lap_grad_refusals          what the gradient is not built for, in one place ('vecchia_response': likelihoods.h:6570-6572)
//   lap_grad_dlogdet_dmode     d log|Sigma W + I| / d mode: CalcLogDetStochDerivModeVecchia, vadu likelihoods.h:16660-16688, pivoted_cholesky / fitc :16554-16611
//   lap_grad_implicit_solve    (Sigma^-1 + W)^-1 d_mll_d_mode, d_mll_d_mode = 0.5 d logdet / d mode (:6599-6608; CGVecchiaLaplaceVec, CG_utils.cpp:21-108, from zero)
//   lap_grad_factor_deriv      dA, dD wrt log(range) and their level-ordered copies (LapDerivEntries); full-scale Vecchia: vif_grad_prepare (Vecchia_utils.cpp:1503-1524,
//                              :1640-1656; sigma_woodbury_grad likelihoods.h:5437-5448, the preconditioner's :5478-5498)
//   lap_grad_trace_operands    per parameter x' SigmaI_deriv y for (mode, sv) and for the probe block through ONE operator (LapSigmaIDeriv): variance SigmaI_deriv = -Sigma^-1
//                              (:6613-6620), range B_grad' D^-1 B + B' D^-1 B_grad - B' D^-1 D_grad D^-1 B (:6621-6640); the control variate's P_deriv (:16760-16775);
//                              pivoted_cholesky / fitc: Sigma U, Sigma P^-1 Z (CalcLogDetStochDerivCovParVecchia :16716-16735)
//   lap_grad_vif_q4            full-scale Vecchia: S0 x, S1 x for x = mode, sv and their products with C', dC' (:5455-5461)
//   lap_grad_fetch             the column sums and the scalars to the host, one synchronisation
//   lap_grad_assemble          per parameter on the host: lap_grad_assemble_vadu (control variate with one optimal c :16776-16790, explicit + implicit part :6641-6664),
//                              lap_grad_assemble_pc (:16734), vif_grad_assemble (CalcGradNegMargLikelihoodLaplaceApproxFSVA :5413-5520)
//   Likelihood::CalcGradNegMargLikelihoodLaplaceApproxVecchia   include/GPBoost/likelihoods.h:6521-6700
//   CalcOptimalC / CalcOptimalCVectorized                       src/GPBoost/CG_utils.cpp:1053-1090 -> gpb_smallmat.h optimal_c, the one copy on the host
// Checker: oracle/gpb_oracle.c orc_vecchia_laplace_grad, oracle/orc.py vif_laplace_grad (same steps, same names).
// Then the entries that start from that state or share its pieces: gpb_hip_vecchia_laplace_grad_F_current, gpb_hip_vecchia_laplace_grad_aux_current (lap_winv_pinv,
// lap_go_buffer), gpb_hip_vecchia_fisher_std_errors (LapDerivEntries, lap_draw).

namespace {

// ---- pieces shared by the entries ---------------------------------------------------------------------------------------------------------------------------
// The reduction buffer of the trace estimators' column sums (d_go, pinned mirror h_go).  grow: at least `need` doubles afterwards; otherwise only the check that an earlier
// gpb_hip_vecchia_laplace_grad_current left that many.
int lap_go_buffer(LaplaceState* s, size_t need, bool grow) {
  if (s->go_cap >= need) return 0;
  if (!grow) return fail("internal: the gradient's reduction buffer is missing (gpb_hip_vecchia_laplace_grad_current first)");
  dev_free(s->d_go);
  if (s->h_go) { (void)hipHostFree(s->h_go); s->h_go = nullptr; }
  s->go_cap = 0;
  HIP_OK(hipMalloc(&s->d_go, sizeof(double) * need));
  HIP_OK(hipHostMalloc(&s->h_go, sizeof(double) * need));
  s->go_cap = need;
  return 0;
}
// dst_host[i] = src[sigma[i]]: an n-vector of the workspace (storage order) to the host in the Vecchia order
int lap_to_vecchia_order(const LaplaceState* s, const double* src, int n, double* dst_host, hipStream_t st) {
  std::vector<double> tmp(n);
  HIP_OK(hipMemcpyAsync(tmp.data(), src, sizeof(double) * (size_t)n, hipMemcpyDeviceToHost, st));
  HIP_OK(hipStreamSynchronize(st));
  for (int i = 0; i < n; ++i) dst_host[i] = tmp[s->sigma[i]];
  return 0;
}
// out = W^-1 P^-1 Z for the probes Z of the low-rank preconditioners: pivoted_cholesky Z - L_k (I_k + L_k' W L_k)^-1 L_k' W Z (likelihoods.h:16554-16611), fitc
// W^-1 .* (D^-1 Z - D^-1 C M C' D^-1 Z) (:16576-16583)
int lap_winv_pinv(LaplaceState* s, int n, const double* W, const double* Zp, double* out, int tch, int nc, hipStream_t st) {
  if (s->pc_type != kPcFitc) return pc_apply(s, n, W, Zp, out, tch, nc, 1, st);
  if (pc_apply(s, n, W, Zp, out, tch, nc, 0, st)) return -1;
  HIP_OK(gpb::pc_rowscale(out, W, n, tch, nc, 1, out, st));
  return 0;
}
// The level-ordered layouts of the two solves with the entries of a derivative dA in place of A: fwd multiplies with dA, bwd with dA'.
struct LapDerivEntries {
  gpb::LapTri fwd, bwd;
  static int alloc_dA(LaplaceState* s, int n, int m) {      // s->d_dA / s->d_dD, once
    if (s->d_dA) return 0;
    HIP_OK(hipMalloc(&s->d_dA, sizeof(double) * (size_t)n * m));
    HIP_OK(hipMalloc(&s->d_dD, sizeof(double) * (size_t)n));
    return 0;
  }
  // Per solve: the entry arrays, allocated once with the sources of the solve's own entries; permute: the coefficients of the current s->d_dA into them.  -> the views
  static int update(LaplaceState* s, const gpb::LapLevels& lv, hipStream_t st, bool permute, LapDerivEntries* out) {
    for (LaplaceState::Tri* tr : { &s->fwd, &s->bwd }) {
      const size_t nh = (size_t)tr->nslots * 32, no = tr->novf > 0 ? tr->novf : 1;
      if (!tr->hent_g) {
        HIP_OK(hipMalloc(&tr->hent_g, sizeof(gpb::LapEnt) * nh));
        HIP_OK(hipMalloc(&tr->oent_g, sizeof(gpb::LapEnt) * no));
        HIP_OK(hipMemcpyAsync(tr->hent_g, tr->hent, sizeof(gpb::LapEnt) * nh, hipMemcpyDeviceToDevice, st));
        HIP_OK(hipMemcpyAsync(tr->oent_g, tr->oent, sizeof(gpb::LapEnt) * no, hipMemcpyDeviceToDevice, st));
      }
      if (permute) HIP_OK(gpb::lap_permute_factor(s->d_dA, tr->hpos, tr->opos, nh, tr->novf, tr->hent_g, tr->oent_g, st));
    }
    out->fwd = lv.fwd; out->fwd.hent = s->fwd.hent_g; out->fwd.oent = s->fwd.oent_g;
    out->bwd = lv.bwd; out->bwd.hent = s->bwd.hent_g; out->bwd.oent = s->bwd.oent_g;
    return 0;
  }
};

// ---- SigmaI_deriv applied to a column or a block ---------------------------------------------------------------------------------------------------------------
// One operand: x (ncol chunks of nc columns), Bx = B x (the caller's), and the scratch of its shape: gx takes dA x, mid the middle factor, back the operand of dA'.
struct LapDerivCols { const double* x; double *Bx, *gx, *mid, *back; int ncol, nc; };
struct LapSigmaIDeriv {
  gpb::LapLevels lv; LapDerivEntries de; int n; const double *Ds, *dDs, *W; hipStream_t st;
  // variance: SigmaI_deriv = -Sigma^-1 (likelihoods.h:6613-6620): out = B' mid, mid = -(B x) / D
  int variance(const LapDerivCols& o, double* out) const {
    const double* nul = nullptr;
    HIP_OK(gpb::lap_deriv_mid(o.Bx, nul, Ds, nul, nul, n, o.ncol, o.nc, 0, o.mid, nullptr, st));
    HIP_OK(gpb::lap_Bt(lv, n, o.mid, out, o.ncol, o.nc, st));
    return 0;
  }
  // range: SigmaI_deriv = B_grad' D^-1 B + B' D^-1 B_grad - B' D^-1 D_grad D^-1 B, B_grad = -dA (:6621-6640), in two halves: SigmaI_deriv x = first - second.
  // first: out = B' mid with gx = dA x; it leaves in o.back the operand of the second half (and, for the trace's control variate, the W parts of P_deriv :16760-16775)
  int range_first(const LapDerivCols& o, double* out) const {
    HIP_OK(gpb::lap_mul(de.fwd, n, o.x, o.gx, o.ncol, o.nc, st));
    HIP_OK(gpb::lap_deriv_mid(o.Bx, o.gx, Ds, dDs, W, n, o.ncol, o.nc, 1, o.mid, o.back, st));
    HIP_OK(gpb::lap_Bt(lv, n, o.mid, out, o.ncol, o.nc, st));
    return 0;
  }
  // second: out = dA' back
  int range_second(const LapDerivCols& o, double* out) const {
    HIP_OK(gpb::lap_mul(de.bwd, n, o.back, out, o.ncol, o.nc, st));
    return 0;
  }
};

// ---- the context of one gradient: who holds what, and what each reused slot of the evaluation's workspace holds at each stage ---------------------------------------
//   d_gblk   U = (Sigma^-1 + W)^-1 Z and PIZ = P^-1 Z (vadu) / U = (W^-1 + Sigma)^-1 Z and PIZ = the probes Z themselves (pivoted_cholesky, fitc), kept from the
//            log-determinant; with a low-rank preconditioner two more blocks, SU = Sigma U and SPZ = Sigma P^-1 Z (lap_grad_trace_operands)
//   d_blk    free after the log-determinant.  R: B PI_Z (vadu) / W^-1 P^-1 Z, then B SPZ (pc) -- from lap_grad_trace_operands on "B x of the block operand";
//            Z: P^-1 Z = W .* R while SU / SPZ are built (pc), then dA x of the block operand; H: the middle factor; Vb: the operand of dA';
//            T: scratch of the solves, then each product whose column sums are taken
//   d_vec    mode, W, rdw: the evaluation's.  rhs: d_mll_d_mode.  r, z, hh, v: the implicit CG's residual, preconditioned residual, direction and A h -- afterwards the
//            four consecutive columns of Q4 = (S0 mode, S0 sv, S1 mode, S1 sv) (full-scale Vecchia).  t1 / t2: scratch of the CG's operator, then t1 = dA' (.) of a
//            column.  Bm, gv, dir, mnew: B x, dA x, the middle factor and the operand of dA' of a single column (col()); upd: B' (.) of its range form
//   d_gvec   dW3, dld = d logdet / d mode and sv = the implicit solve (kept for the F and auxiliary-parameter gradients), SdM = SigmaI_deriv(variance) mode,
//            dDs = dD in storage order
//   d_go     go: 10 tc column sums in blocks of 2 tc (variance; range, B' half; range, dA' half; the two halves of the !pc second pass), then gov: 6 sums of the
//            mode column (variance; range, B' half; range, dA' half -- each for (mode, sv))
struct LapGrad {
  gpb_hip_vecchia_t* h; LaplaceState* s; LapWork w; LapSolver op; hipStream_t st;
  int n, t, cg_max_num_it; double cg_delta_conv;
  bool pc, fitc, vif;               // a low-rank preconditioner (the (W^-1 + Sigma) form); fitc among them; full-scale Vecchia (fitc only)
  const double *U, *PIZ; double *SU, *SPZ;
  size_t go_need; double *go, *gov;
  const double* fe;
  LapDerivCols col(const double* x) const { return LapDerivCols{ x, w.Bm, w.gv, w.dir, w.mnew, 1, 1 }; }
  LapDerivCols blk(const double* x) const { return LapDerivCols{ x, w.R, w.Z, w.H, w.Vb, w.tch, w.NCB }; }
};
// Everything the gradient refuses, before any device work; tests assert the order and the words.
int lap_grad_refusals(const gpb_hip_vecchia_t* h, int cg_max_num_it, const double* grad2_host) {
  if (!h || !grad2_host) return fail("null argument");
  const LaplaceState* s = h->lap;
  if (s && s->pc_type == kPcVecchiaResponse) return fail("Calculation of gradients is currently not correctly implemented for the '%s' preconditioner ", "vecchia_response");   // likelihoods.h:6570-6572
  if (s && h->vif_k > 0 && s->pc_type != kPcFitc) return fail("full-scale Vecchia with a non-Gaussian likelihood: the gradient is built for the fitc preconditioner (the reference's default); '%s' serves evaluations and Nelder-Mead fits", s->pc_type == kPcVifdu ? "vifdu" : "none");
  if (!s || !s->grad_state || !s->d_gblk) return fail("the gradient needs the state of an evaluation that kept it (gpb_hip_vecchia_laplace_eval with keep_grad_state)");
  if (cg_max_num_it < 1) return fail("cg_max_num_it must be positive");
  const bool vif = h->vif_k > 0;
  if (vif && (!s->vif_grad_inputs || !s->d_pcdL)) return fail("full-scale Vecchia: the gradient needs an evaluation with the fitc preconditioner that kept its state");
  if (pc_has_lowrank(s->pc_type) && (s->gblk_cap < 4 * lap_work(h, s, s->g_t).nb || !s->d_pcL || !s->d_pcM)) return fail("the gradient needs an evaluation with the pivoted_cholesky / fitc preconditioner that kept its state");
  if (h->m > 126) return fail("gradient of the Laplace approximation: the per-point derivative kernel handles at most 126 neighbours (this model has %d)", h->m);
  if (h->d > 3) return fail("gradient of the Laplace approximation: the per-point derivative kernel handles coordinate dimensions 1..3 (this model has %d)", h->d);
  return 0;
}
// d log|Sigma W + I| / d mode -> dld.  Leaves R = B PI_Z (vadu) / W^-1 P^-1 Z (pc)
int lap_grad_dlogdet_dmode(const LapGrad& c) {
  LaplaceState* s = c.s; const LapWork& w = c.w;
  HIP_OK(gpb::lap_third_deriv(s->link, w.mode, s->resp(), c.fe, c.n, w.dW3, c.st, s->d_dptr));
  if (c.pc) {
    if (lap_winv_pinv(s, c.n, w.W, c.PIZ, w.R, w.tch, w.NCB, c.st)) return -1;
    HIP_OK(gpb::pc_row_stats(c.U, w.R, s->d_pcL, s->d_pcM, w.W, w.dW3, c.n, s->pc_k, c.t, w.NCB, w.dld, c.st, c.fitc ? s->d_pcwp : nullptr, c.vif ? 1 : 0, w.v));
  } else {
    HIP_OK(gpb::lap_B(c.op.lv, c.n, c.PIZ, w.R, w.tch, w.NCB, c.st));
    HIP_OK(gpb::lap_row_stats(c.U, c.PIZ, w.R, w.dW3, w.rdw, c.n, c.t, w.NCB, w.dld, c.st));
  }
  return 0;
}
// sv = (Sigma^-1 + W)^-1 rhs, rhs = 0.5 dld.  vadu: CGVecchiaLaplaceVec from zero; otherwise Inv_SigmaI_plus_ZtWZ_Vecchia_iterative_given_PC ->
// CGVecchiaLaplace_Version_SigmaPlusWinvVec from zero with the preconditioner of the mode: (W^-1 + Sigma) u' = Sigma rhs, u = W^-1 u'
int lap_grad_implicit_solve(const LapGrad& c) {
  LaplaceState* s = c.s; const LapWork& w = c.w; const int n = c.n; hipStream_t st = c.st;
  HIP_OK(gpb::lap_lincomb(w.rhs, w.dld, w.dld, 0.5, 0.0, n, st));
  HIP_OK(gpb::lap_dot(w.rhs, w.rhs, n, s->d_o, st));
  if (lap_fetch(s, 2, st)) return -1;
  HIP_OK(hipMemsetAsync(w.sv, 0, w.vb, st));
  if (s->h_o[1] < 1e-100) return 0;
  const LapScratch scr{ w.t1, w.t2, nullptr, nullptr };
  if (c.pc) { if (c.op.sigma(w.rhs, w.r, w.t2, 1, 1)) return -1; }
  else HIP_OK(hipMemcpyAsync(w.r, w.rhs, w.vb, hipMemcpyDeviceToDevice, st));
  if (c.op.precond(w.r, w.z, scr, 1, 1)) return -1;
  HIP_OK(hipMemcpyAsync(w.hh, w.z, w.vb, hipMemcpyDeviceToDevice, st));
  int ncg = 0;
  const int end = lap_cg(c.op, scr, w.sv, w.r, w.z, w.hh, w.v, 1, 1, w.sc1, LapCgRule{ std::min(c.cg_max_num_it, n), c.cg_delta_conv, 1, false, 1, false }, &ncg);
  if (end == LAP_CG_ERROR) return -1;
  if (end == LAP_CG_NONFINITE) return fail("NaN or Inf occurred in the conjugate gradient algorithm (implicit derivative)");
  if (c.pc) HIP_OK(gpb::pc_rowscale(w.sv, w.W, n, 1, 1, 1, w.sv, st));
  return 0;
}
// dA, dD wrt the log range (full-scale Vecchia: of the residual process, with the k x k matrices of the host half), dDs, the level-ordered entries of dA -> *D
int lap_grad_factor_deriv(const LapGrad& c, VifGradHost* vg, LapSigmaIDeriv* D) {
  gpb_hip_vecchia_t* h = c.h; LaplaceState* s = c.s; const int n = c.n; hipStream_t st = c.st;
  LapDerivEntries de;
  if (LapDerivEntries::alloc_dA(s, n, h->m)) return -1;
  if (c.vif) { if (vif_grad_prepare(h, s, vg, st)) return -1; }
  else HIP_OK(gpb::lap_range_deriv(h->d_pts, h->d_nn, h->d_A, n, h->m, s->g_cov, h->d == 3 ? 1 : 0, s->g_var, s->g_a, s->d_dA, s->d_dD, st));
  HIP_OK(gpb::lap_scatter(s->d_dD, s->d_sigma, n, c.w.dDs, st));
  if (LapDerivEntries::update(s, c.op.lv, st, true, &de)) return -1;
  HIP_OK(gpb::lap_sums3(c.w.rdw, s->d_Ds, c.w.dDs, n, s->d_o + 4, st));
  *D = LapSigmaIDeriv{ c.op.lv, de, n, s->d_Ds, c.w.dDs, c.w.W, st };
  return 0;
}
// a' SigmaI_deriv(theta_j) x and b' SigmaI_deriv(theta_j) x per column of one operand -> dots (variance: 2 sums per column; range: the two halves, `stride` apart)
int lap_grad_variance_dots(const LapGrad& c, const LapSigmaIDeriv& D, const LapDerivCols& o, const double* a, const double* b, double* out, double* dots) {
  if (D.variance(o, out)) return -1;
  HIP_OK(gpb::lap_coldots(a, b, out, c.n, o.ncol, o.nc, dots, c.st));
  return 0;
}
int lap_grad_range_dots(const LapGrad& c, const LapSigmaIDeriv& D, const LapDerivCols& o, const double* a, const double* b, double* out, double* out2, double* dots, size_t stride) {
  if (D.range_first(o, out)) return -1;
  HIP_OK(gpb::lap_coldots(a, b, out, c.n, o.ncol, o.nc, dots, c.st));
  if (D.range_second(o, out2)) return -1;
  HIP_OK(gpb::lap_coldots(a, b, out2, c.n, o.ncol, o.nc, dots + stride, c.st));
  return 0;
}
// The operands of the trace estimators and of the explicit / implicit parts, per parameter.  The block operand is (U, PI_Z) with R = B PI_Z from lap_grad_dlogdet_dmode
// (vadu), or (Sigma U, Sigma P^-1 Z) without a control variate (pivoted_cholesky / fitc)
int lap_grad_trace_operands(const LapGrad& c, const LapSigmaIDeriv& D, VifGradHost* vg) {
  LaplaceState* s = c.s; const LapWork& w = c.w; const int n = c.n, tch = w.tch, NCB = w.NCB; const size_t tc = (size_t)w.tc; hipStream_t st = c.st;
  const gpb::LapLevels& lv = c.op.lv;
  const LapDerivCols mcol = c.col(w.mode);
  HIP_OK(gpb::lap_B(lv, n, w.mode, w.Bm, 1, 1, st));
  if (lap_grad_variance_dots(c, D, mcol, w.mode, w.sv, w.SdM, c.gov)) return -1;
  const double *Ub = c.U, *Pb = c.PIZ;
  if (c.pc) {
    HIP_OK(gpb::pc_rowscale(w.R, w.W, n, tch, NCB, 0, w.Z, st));                          // P^-1 Z = W .* (W^-1 P^-1 Z)
    if (c.vif && vif_grad_block_sums(c.h, s, vg, c.U, w.Z, w.T, w.dDs, tch, NCB, st)) return -1;   // the k-vectors C' U_c, dC' U_c, ... of the host half; the control variate's diagonal parts
    HIP_OK(gpb::lap_vadu(lv, n, s->d_Ds, w.Z, c.SPZ, w.T, tch, NCB, st));
    HIP_OK(gpb::lap_vadu(lv, n, s->d_Ds, c.U, c.SU, w.T, tch, NCB, st));
    HIP_OK(gpb::lap_B(lv, n, c.SPZ, w.R, tch, NCB, st));
    Ub = c.SU; Pb = c.SPZ;
  }
  const LapDerivCols mblk = c.blk(Pb);
  if (lap_grad_variance_dots(c, D, mblk, Ub, Pb, w.T, c.go)) return -1;
  if (lap_grad_range_dots(c, D, mcol, w.mode, w.sv, w.upd, w.t1, c.gov + 2, 2)) return -1;
  if (lap_grad_range_dots(c, D, mblk, Ub, Pb, w.T, w.T, c.go + 2 * tc, 2 * tc)) return -1;
  // the control variate's second pass, vadu only: P_deriv's B' W B_grad + B_grad' W B with (U, PI_Z) (:16760-16775)
  if (c.pc) { HIP_OK(hipMemsetAsync(c.go + 6 * tc, 0, sizeof(double) * 4 * tc, st)); return 0; }
  HIP_OK(gpb::lap_deriv_mid(w.R, w.Z, s->d_Ds, w.dDs, w.W, n, tch, NCB, 2, w.H, w.Vb, st));
  HIP_OK(gpb::lap_Bt(lv, n, w.H, w.T, tch, NCB, st));
  HIP_OK(gpb::lap_coldots(c.U, c.PIZ, w.T, n, tch, NCB, c.go + 6 * tc, st));
  if (D.range_second(mblk, w.T)) return -1;
  HIP_OK(gpb::lap_coldots(c.U, c.PIZ, w.T, n, tch, NCB, c.go + 8 * tc, st));
  return 0;
}
// S0 x = -Sigma_v^-1 x and S1 x = SigmaI_deriv(range) x for x = mode, sv -> the four columns r, z, hh, v (consecutive n-vectors); their products with C' and dC'
int lap_grad_vif_q4(const LapGrad& c, const LapSigmaIDeriv& D, VifGradHost* vg) {
  const LapWork& w = c.w; const int n = c.n;
  double* Q4 = w.r;
  const double* xs[2] = { w.mode, w.sv };
  for (int q = 0; q < 2; ++q) {
    double* S0 = Q4 + (size_t)q * n; double* S1 = Q4 + (size_t)(2 + q) * n;
    const LapDerivCols o = c.col(xs[q]);
    HIP_OK(gpb::lap_B(c.op.lv, n, xs[q], w.Bm, 1, 1, c.st));
    if (D.variance(o, S0) || D.range_first(o, S1) || D.range_second(o, w.t1)) return -1;
    HIP_OK(gpb::lap_lincomb(S1, S1, w.t1, 1.0, -1.0, n, c.st));
  }
  return vif_grad_vec_sums(c.h, c.s, vg, Q4, c.st);
}
int lap_grad_fetch(const LapGrad& c) {
  LaplaceState* s = c.s;
  HIP_OK(hipMemcpyAsync(s->h_go, c.go, sizeof(double) * c.go_need, hipMemcpyDeviceToHost, c.st));
  if (lap_check_solves(s, c.st)) return -1;
  return lap_fetch(s, 8, c.st);
}

// ---- host assembly: out4 = { mode' SigmaI_deriv mode, d logdet / d theta_j, optimal c, implicit part } per parameter, -> d(-mll) / d theta_j --------------------------
// vadu: the control variate z' P_deriv P^-1 z with one optimal c (:16776-16790); its deterministic trace trD and the deterministic part det0 of d logdet / d theta_j
double lap_grad_assemble_vadu(int t, const double* z1, const double* zP, double det0, double trD, double mSm, double sSm, double* out4) {
  const sm::OptimalC oc = sm::optimal_c(z1, zP, t, nullptr);
  const double dl = (oc.mean1 + det0) + (oc.c * trD - oc.c * oc.meanP);
  out4[0] = mSm; out4[1] = dl; out4[2] = oc.c; out4[3] = -sSm;
  return 0.5 * (mSm + dl) - sSm;
}
// pivoted_cholesky / fitc: d logdet / d theta_j = -mean_c (Sigma U_c)' SigmaI_deriv (Sigma P^-1 Z_c)  (:16734), no control variate
double lap_grad_assemble_pc(int t, const double* z1, double mSm, double sSm, double* out4) {
  double m1 = 0.;
  for (int c = 0; c < t; ++c) m1 += z1[c];
  const double dlp = -1.0 * (m1 / t);
  out4[0] = mSm; out4[1] = dlp; out4[2] = 0.; out4[3] = -sSm;
  return 0.5 * (mSm + dlp) - sSm;
}
// full-scale Vecchia, parameter j (0: log variance, 1: log range): z1[c] = (Sigma_v U_c)' SigmaI_deriv (Sigma_v P^-1 Z_c) from the Vecchia path's block products,
// mSm0 / sSm0 = mode' S_deriv mode, sv' S_deriv mode
double vif_grad_assemble(const LaplaceState* s, const VifGradHost& vg, int j, int t, const double* z1, double mSm0, double sSm0, double* parts4) {
  const int k = vg.k, kp = vg.kp, nc = 4;
  auto dot = [](const double* a, const double* b, int kk) { double r = 0.0; for (int i = 0; i < kk; ++i) r += a[i] * b[i]; return r; };
  auto matvec = [](const std::vector<double>& M, const double* x, int kk, double* out) { for (int i = 0; i < kk; ++i) { double r = 0.0; for (int p = 0; p < kk; ++p) r += M[(size_t)i * kk + p] * x[p]; out[i] = r; } };
  // ---- x' SigmaI_deriv_mode for x = mode, sv ----
  const double* yC = vg.yC.data(); const double* ydC = (j == 0) ? vg.yC.data() : vg.ydC.data();
  const int a1col = (j == 0) ? 0 : 2;
  std::vector<double> wsol(k), kv(k), Mgw(k);
  for (int q = 0; q < k; ++q) wsol[q] = -yC[q];                                 // C' S mode
  sm::cholesky_solve(s->vif_cholM.data(), k, k, wsol.data());
  matvec(vg.Mg[j], wsol.data(), k, Mgw.data());
  for (int q = 0; q < k; ++q) kv[q] = yC[(size_t)a1col * k + q] + (-ydC[q]) - Mgw[q];        // C' a1 + dC' S mode - Mg wsol
  sm::cholesky_solve(s->vif_cholM.data(), k, k, kv.data());
  double val[2];
  for (int x = 0; x < 2; ++x) {
    const double xa1 = x == 0 ? mSm0 : sSm0;
    const double* CtSIdx = yC + (size_t)((j == 0) ? x : 2 + x) * k;
    const double* CtS0x = yC + (size_t)x * k;                                   // = -C' S x
    const double* dCtS0x = ydC + (size_t)x * k;                                 // = -dC' S x
    val[x] = xa1 - dot(CtSIdx, wsol.data(), k) + dot(CtS0x, kv.data(), k) + dot(dCtS0x, wsol.data(), k);
  }
  const double mSm = val[0], sSm = val[1];
  // ---- stochastic trace with the preconditioner's control variate ----
  std::vector<double> sS(t), sP(t), cu(k), dcu(k), cp(k), dcp(k), sicu(k), sicp(k), tv(k), cpp(kp), dcpp(kp), s1(kp), tvp(kp);
  const std::vector<double>& dCUv = (j == 0) ? vg.CU : vg.dCU;
  const std::vector<double>& dCPv = (j == 0) ? vg.CP : vg.dCP;
  const std::vector<double>& dCpPv = (j == 0) ? vg.CpP : vg.dCpP;
  for (int c = 0; c < t; ++c) {
    const int ch = c / nc, cc = c % nc;
    for (int q = 0; q < k; ++q) {
      const size_t o = ((size_t)ch * k + q) * nc + cc;
      cu[q] = vg.CU[o]; dcu[q] = dCUv[o]; cp[q] = vg.CP[o]; dcp[q] = dCPv[o];
    }
    apply_linv_sym(s->vif_Linv, k, cu.data(), sicu.data());
    apply_linv_sym(s->vif_Linv, k, cp.data(), sicp.data());
    matvec(vg.dSm[j], sicp.data(), k, tv.data());
    const double part1 = dot(dcu.data(), sicp.data(), k) + dot(sicu.data(), dcp.data(), k) - dot(sicu.data(), tv.data(), k);
    sS[c] = part1 - z1[c];
    for (int q = 0; q < kp; ++q) { const size_t o = ((size_t)ch * kp + q) * nc + cc; cpp[q] = vg.CpP[o]; dcpp[q] = dCpPv[o]; }
    apply_linv_sym(s->pc_Linv, kp, cpp.data(), s1.data());
    matvec(vg.dSmp[j], s1.data(), kp, tvp.data());
    sP[c] = 2.0 * dot(dcpp.data(), s1.data(), kp) - dot(s1.data(), tvp.data(), kp) + vg.wn[j][c];
  }
  // deterministic tr(P^-1 dP): sum dgrad wp - tr(Sigma_m,p^-1 dSigma_m,p) + tr(M_p^-1 sigma_woodbury_grad_preconditioner)
  double tr = vg.sum_dgrad_wp[j];
  {
    std::vector<double> col(kp), out(kp);
    for (int c = 0; c < kp; ++c) {
      for (int q = 0; q < kp; ++q) col[q] = vg.dSmp[j][(size_t)q * kp + c];
      apply_linv_sym(s->pc_Linv, kp, col.data(), out.data());
      tr -= out[c];
    }
    for (int i = 0; i < kp; ++i) for (int p = 0; p < kp; ++p) tr += s->pc_Minv[(size_t)i * kp + p] * vg.Mgp[j][(size_t)p * kp + i];
  }
  const sm::OptimalC oc = sm::optimal_c(sS.data(), sP.data(), t, &tr);      // (CalcOptimalC centres this control variate with its deterministic trace: likelihoods.h:5500-5510)
  const double dl = oc.mean1 - oc.c * (oc.meanP - tr);
  parts4[0] = mSm; parts4[1] = dl; parts4[2] = oc.c; parts4[3] = -sSm;
  return 0.5 * (mSm + dl) - sSm;
}
// h_go / h_o -> the two derivatives.  Per column c: g[c], g[tc + c] = U_c' S PI_Z_c and PI_Z_c' S PI_Z_c for the variance's S, the following blocks of 2 tc for the range
int lap_grad_assemble(const LapGrad& c, const VifGradHost& vg, double* grad2_host, double* parts_host) {
  const LaplaceState* s = c.s;
  const int t = c.t, tc = c.w.tc;
  const double *g = s->h_go, *gvh = g + (size_t)10 * tc;
  const double sum_rdw_D = s->h_o[4], sum_rdw_dD_D2 = s->h_o[5], sum_dD_D = s->h_o[6];
  std::vector<double> z1(t), zP(t);
  for (int j = 0; j < 2; ++j) {
    for (int cc = 0; cc < t; ++cc) {
      if (j == 0) { z1[cc] = g[cc]; zP[cc] = g[tc + cc]; }
      else {
        z1[cc] = g[2 * tc + cc] - g[4 * tc + cc];
        zP[cc] = (g[3 * tc + cc] - g[5 * tc + cc]) + (g[7 * tc + cc] - g[9 * tc + cc]);
      }
    }
    const double mSm = (j == 0) ? gvh[0] : gvh[2] - gvh[4];
    const double sSm = (j == 0) ? gvh[1] : gvh[3] - gvh[5];
    double parts4[4];
    if (c.vif) grad2_host[j] = vif_grad_assemble(s, vg, j, t, z1.data(), mSm, sSm, parts4);
    else if (c.pc) grad2_host[j] = lap_grad_assemble_pc(t, z1.data(), mSm, sSm, parts4);
    else grad2_host[j] = lap_grad_assemble_vadu(t, z1.data(), zP.data(), j == 0 ? (double)c.n : sum_dD_D, j == 0 ? -sum_rdw_D : -sum_rdw_dD_D2, mSm, sSm, parts4);
    if (parts_host) for (int q = 0; q < 4; ++q) parts_host[4 * j + q] = parts4[q];
  }
  return 0;
}

// ---- auxiliary parameters -------------------------------------------------------------------------------------------------------------------------------------
// One branch of the Fisher-Laplace trace 0.5 tr((Sigma^-1 + W)^-1 dW / d log aux) with dW = f W: per column the sample sign f h_go[c] and the control variate
// sign f h_go[2 tc + c], the control variate's deterministic trace f det_a - f det_b, and f extra = tr(W^-1 dW) where the estimator leaves it out.
struct LapAuxTrace { double sign, det_a, det_b, extra; bool centre_det; };
// The column sums of the branch to h_go and its deterministic sums to *tr.  U and PI_Z of the log-determinant's block CG; R, T, Z: free after the covariance-parameter gradient
int lap_aux_trace_sums(gpb_hip_vecchia_t* h, LaplaceState* s, const LapWork& w, LapAuxTrace* tr) {
  const int n = h->n, tch = w.tch, NCB = w.NCB; const size_t tc = (size_t)w.tc; hipStream_t st = h->stream;
  const double *U = s->d_gblk, *PIZ = s->d_gblk + w.nb;
  const bool pc = pc_has_lowrank(s->pc_type), fitc = s->pc_type == kPcFitc;
  if (lap_go_buffer(s, 4 * tc + 2, false)) return -1;
  if (pc) {
    // pivoted_cholesky / fitc branches (:16800-16837) with dW = f W:  stochastic -f mean_c U_c' (W^-1 P^-1 Z_c) + n f;  control variate -f mean_c (W^-1 P^-1 Z_c)' W (W^-1 P^-1 Z_c)
    // against f [sum_i sdiag_i W_i - n] (pivoted_cholesky) / f [sum_i sdiag_i wp_i^2 / W_i - sum_i wp_i / W_i] (fitc); PIZ holds the probes Z here
    if (lap_winv_pinv(s, n, w.W, PIZ, w.R, tch, NCB, st)) return -1;                                 // R = W^-1 P^-1 Z
    HIP_OK(gpb::pc_rowscale(w.R, w.W, n, tch, NCB, 0, w.Z, st));                                     // W .* R
    HIP_OK(gpb::lap_coldots(U, U, w.R, n, tch, NCB, s->d_go, st));                                   // U_c . R_c
    HIP_OK(gpb::lap_coldots(w.R, w.R, w.Z, n, tch, NCB, s->d_go + 2 * tc, st));                      // R_c . (W R_c)
    HIP_OK(gpb::pc_aux_sums(s->d_pcL, s->d_pcM, w.W, fitc ? s->d_pcwp : nullptr, n, s->pc_k, s->d_o, st));
  } else {
    // vadu (CalcLogDetStochDerivAuxParVecchia :16838-16856): stochastic f mean_c U_c' W PI_Z_c, control variate f mean_c (B PI_Z_c)' W (B PI_Z_c) against f sum rdw W
    HIP_OK(gpb::lap_B(make_levels(h, s), n, PIZ, w.R, tch, NCB, st));                                // B PI_Z
    HIP_OK(gpb::pc_rowscale(PIZ, w.W, n, tch, NCB, 0, w.T, st));                                     // W .* PI_Z
    HIP_OK(gpb::pc_rowscale(w.R, w.W, n, tch, NCB, 0, w.Z, st));                                     // W .* (B PI_Z)
    HIP_OK(gpb::lap_coldots(U, U, w.T, n, tch, NCB, s->d_go, st));                                   // U_c . (W PI_Z_c)
    HIP_OK(gpb::lap_coldots(w.R, w.R, w.Z, n, tch, NCB, s->d_go + 2 * tc, st));                      // (B PI_Z_c) . (W B PI_Z_c)
    HIP_OK(gpb::lap_dot(w.rdw, w.W, n, s->d_o, st));                                                 // sum rdw W
  }
  HIP_OK(hipMemcpyAsync(s->h_go, s->d_go, sizeof(double) * (4 * tc + 2), hipMemcpyDeviceToHost, st));
  if (lap_fetch(s, 2, st)) return -1;
  // (full-scale Vecchia, likelihoods.h:5666-5672: CalcOptimalC centres the control variate with its deterministic trace; the Vecchia path, :16830-16837, with the samples' mean)
  *tr = pc ? LapAuxTrace{ -1., s->h_o[0], fitc ? s->h_o[1] : (double)n, (double)n, h->vif_k > 0 } : LapAuxTrace{ 1., s->h_o[0], 0., 0., false };
  return 0;
}
// Likelihoods whose information does not depend on the mode (Fisher-Laplace, likelihoods.h:6800-6815, grad_information_wrt_mode_non_zero_ = false): per parameter
// CalcGradNegLogLikAuxPars + 0.5 tr((Sigma^-1 + W)^-1 dW / d log aux), no implicit part; dW_r / d log aux = (sum of the weights of r's data) dFI / d log aux
// (:15369-15400), and W_r = (sum of weights) FI, so dW / d log aux = W .* (dFI / FI).  out: 4 doubles per parameter.
//   t (log scale, log df): CalcGradNegLogLikAuxPars :14241-14262
//   lognormal (the variance of log y): :14275-14286, information 1 / aux, d information / d log aux = -1 / aux :14891-14900
//   gaussian_latent (the error variance): :14262-14274 = 0.5 n - 0.5 / aux sum w resid^2, information 1 / aux, d information / d log aux = -1 / aux :14881-14890
int lap_grad_aux_fisher_laplace(gpb_hip_vecchia_t* h, LaplaceState* s, const LapWork& w, const double* o3, int nd, double* out4_host) {
  const double r = s->aux, nu = s->aux2, sigma2 = r * r;
  // per parameter: CalcGradNegLogLikAuxPars from the kernel's sums; FI = the information per unit weight, dFI = d FI / d log(parameter)
  double g_scale, FI = 1. / r, dFI[2] = { -1. / r, 0. };      // (lognormal, gaussian_latent: one parameter, FI = 1 / aux)
  const double g_df = (o3[1] + nd * (-1.0 + nu * (host_digamma((nu + 1.) / 2.) - host_digamma(nu / 2.)))) / -2.0;
  switch (s->link) {
    case gpb::kT: g_scale = o3[0] + nd; FI = (nu + 1.) / (nu + 3.) / sigma2; dFI[0] = -2. * (nu + 1.) / (nu + 3.) / sigma2; dFI[1] = nu * 2. / sigma2 / (nu + 3.) / (nu + 3.); break;
    case gpb::kLogNormal: g_scale = o3[0]; break;
    case gpb::kGaussianLatent: g_scale = -0.5 / r * o3[0] + 0.5 * nd; break;
    default: return fail("gpb_hip_vecchia_laplace_grad_aux_current: the Fisher-Laplace gradient of likelihood id %d is missing", s->link);
  }
  LapAuxTrace tr;
  if (lap_aux_trace_sums(h, s, w, &tr)) return -1;
  const int t = s->g_t; const size_t tc = (size_t)w.tc;
  std::vector<double> z1(t), zP(t);
  for (int ia = 0; ia < gpb::lik_num_aux(s->link); ++ia) {
    const double f = dFI[ia] / FI, sf = tr.sign * f;
    for (int c = 0; c < t; ++c) { z1[c] = sf * s->h_go[c]; zP[c] = sf * s->h_go[2 * tc + c]; }
    const double det = f * tr.det_a - f * tr.det_b;
    const sm::OptimalC oc = sm::optimal_c(z1.data(), zP.data(), t, tr.centre_det ? &det : nullptr);
    const double ddet = oc.mean1 + f * tr.extra + oc.c * det - oc.c * oc.meanP;
    const double nld = ia == 0 ? g_scale : g_df;
    out4_host[4 * ia] = nld + 0.5 * ddet; out4_host[4 * ia + 1] = nld; out4_host[4 * ia + 2] = 0.5 * ddet; out4_host[4 * ia + 3] = 0.;
  }
  return 0;
}
// ---- standard errors of a Gaussian Vecchia model ------------------------------------------------------------------------------------------------------------------
// se = sqrt(diag(FI^-1)), FI_kl = f_k f_l mean_c dots[block(k, l)][c] / 2 for the six column-sum blocks 00, 10, 11, 21, 02, 22 (tc columns each, the first t averaged)
int fisher_se_from_dots(const std::vector<double>& dots, int t, int tc, const double* f, double* se3_host) {
  auto meanc = [&](int block) { double acc = 0.; for (int c = 0; c < t; ++c) acc += dots[(size_t)block * tc + c]; return acc / t; };
  double FI[3][3];
  FI[0][0] = meanc(0) * f[0] * f[0] / 2.; FI[1][0] = FI[0][1] = meanc(1) * f[1] * f[0] / 2.;
  FI[1][1] = meanc(2) * f[1] * f[1] / 2.; FI[2][1] = FI[1][2] = meanc(3) * f[2] * f[1] / 2.;
  FI[2][0] = FI[0][2] = meanc(4) * f[0] * f[2] / 2.; FI[2][2] = meanc(5) * f[2] * f[2] / 2.;
  // diagonal of the inverse of the symmetric 3 x 3 matrix by cofactors
  const double c00 = FI[1][1] * FI[2][2] - FI[1][2] * FI[2][1], c11 = FI[0][0] * FI[2][2] - FI[0][2] * FI[2][0], c22 = FI[0][0] * FI[1][1] - FI[0][1] * FI[1][0];
  const double det = FI[0][0] * c00 - FI[0][1] * (FI[1][0] * FI[2][2] - FI[1][2] * FI[2][0]) + FI[0][2] * (FI[1][0] * FI[2][1] - FI[1][1] * FI[2][0]);
  if (!(det > 0.)) return fail("the Fisher information is not positive definite (det = %g)", det);
  se3_host[0] = std::sqrt(c00 / det); se3_host[1] = std::sqrt(c11 / det); se3_host[2] = std::sqrt(c22 / det);
  return 0;
}

}  // namespace

extern "C" {

// parts_host (optional, 8 doubles): per parameter { mode' SigmaI_deriv mode, d logdet / d theta, optimal c, implicit part }; vecs_host (optional, 2 n doubles, Vecchia
// order): d logdet / d mode and (Sigma^-1 + W)^-1 d_mll_d_mode -- the intermediate values the step-wise parity tests compare.
int gpb_hip_vecchia_laplace_grad_current(gpb_hip_vecchia_t* h, int cg_max_num_it, double cg_delta_conv, double* grad2_host, double* parts_host, double* vecs_host) {
  API_BEGIN();
  if (lap_grad_refusals(h, cg_max_num_it, grad2_host)) return -1;
  LaplaceState* s = h->lap;
  HIP_OK(hipSetDevice(h->device));
  const LapWork w = lap_work(h, s, s->g_t);
  const bool pc = pc_has_lowrank(s->pc_type);
  LapGrad c{ h, s, w, lap_solver(h, s, w, lap_form(s)), h->stream, h->n, s->g_t, cg_max_num_it, cg_delta_conv, pc, s->pc_type == kPcFitc, h->vif_k > 0,
             s->d_gblk, s->d_gblk + w.nb, pc ? s->d_gblk + 2 * w.nb : nullptr, pc ? s->d_gblk + 3 * w.nb : nullptr,
             (size_t)10 * w.tc + 6, nullptr, nullptr, s->has_fe ? s->d_fe : nullptr };
  if (lap_go_buffer(s, c.go_need, true)) return -1;
  c.go = s->d_go; c.gov = c.go + (size_t)10 * w.tc;
  VifGradHost vg;
  LapSigmaIDeriv D;
  if (lap_grad_dlogdet_dmode(c) || lap_grad_implicit_solve(c) || lap_grad_factor_deriv(c, &vg, &D) || lap_grad_trace_operands(c, D, &vg)) return -1;
  if (c.vif && lap_grad_vif_q4(c, D, &vg)) return -1;
  if (lap_grad_fetch(c) || lap_grad_assemble(c, vg, grad2_host, parts_host)) return -1;
  s->gvec_state = true;
  if (vecs_host && (lap_to_vecchia_order(s, w.dld, c.n, vecs_host, c.st) || lap_to_vecchia_order(s, w.sv, c.n, vecs_host + c.n, c.st))) return -1;
  API_END();
}

// Boosting gradient for non-Gaussian data at the state of the last gpb_hip_vecchia_laplace_grad_current: d(-mll) / dF, Vecchia order (CalcGradNegMargLikelihoodLaplaceApproxVecchia with
// calc_F_grad, likelihoods.h:6996-7001).  Full-scale Vecchia handles too: CalcGradNegMargLikelihoodLaplaceApproxFSVA's calc_F_grad part, likelihoods.h:5598-5604, is the
// same expression in d logdet / d mode and the implicit solve.
int gpb_hip_vecchia_laplace_grad_F_current(gpb_hip_vecchia_t* h, double* gradF_host) {
  API_BEGIN();
  if (!h || !gradF_host) return fail("null argument");
  LaplaceState* s = h->lap;
  if (!s || !s->grad_state || !s->gvec_state) return fail("the gradient wrt the fixed effects needs the state of gpb_hip_vecchia_laplace_grad_current");
  HIP_OK(hipSetDevice(h->device));
  const int n = h->n;
  const LapWork w = lap_work(h, s, s->g_t);
  if (s->re_ptr.empty()) {
    HIP_OK(gpb::lap_grad_F(s->link, w.mode, s->resp(), s->has_fe ? s->d_fe : nullptr, w.dld, w.sv, n, w.t2, h->stream));      // (t2: free between evaluations)
    return lap_to_vecchia_order(s, w.t2, n, gradF_host, h->stream);
  }
  // repeated locations: per DATUM, in the order labels / fixed effects were handed over (grouped by random effect, Vecchia order of the random
  // effects) -- the data-scale form of likelihoods.h:6944-6966
  const int nd = s->n_data;
  if (!s->d_dptr) return fail("the data map has not been uploaded (no evaluation since gpb_hip_vecchia_laplace_set_data_map)");
  DevBuf<double> d_out;
  HIP_OK(d_out.alloc((size_t)nd));
  HIP_OK(gpb::lap_grad_F_map(s->link, w.mode, s->resp(), s->has_fe ? s->d_fe : nullptr, w.dld, w.dW3, w.sv, n, s->d_dptr, d_out, h->stream));
  std::vector<double> tmp(nd);
  HIP_OK(hipMemcpyAsync(tmp.data(), d_out, sizeof(double) * (size_t)nd, hipMemcpyDeviceToHost, h->stream));
  HIP_OK(hipStreamSynchronize(h->stream));
  std::vector<int> inv(n), sptr(n + 1);                     // storage slot -> Vecchia position; CSR of the data in storage order (as laplace_eval)
  for (int i = 0; i < n; ++i) inv[s->sigma[i]] = i;
  sptr[0] = 0;
  for (int p = 0; p < n; ++p) sptr[p + 1] = sptr[p] + (s->re_ptr[inv[p] + 1] - s->re_ptr[inv[p]]);
  for (int i = 0; i < n; ++i) {
    const int p = s->sigma[i], cnt = s->re_ptr[i + 1] - s->re_ptr[i];
    for (int k = 0; k < cnt; ++k) gradF_host[s->re_ptr[i] + k] = tmp[sptr[p] + k];
  }
  API_END();
}

// Gradient of the negative approximate marginal log-likelihood wrt log(auxiliary parameter) at the state of the last gpb_hip_vecchia_laplace_grad_current
// (CalcGradNegMargLikelihoodLaplaceApproxVecchia's calc_aux_par_grad branch, likelihoods.h:6743-6808): out4 = { gradient, CalcGradNegLogLikAuxPars
// part, 0.5 * log-determinant part, implicit part }.
int gpb_hip_vecchia_laplace_grad_aux_current(gpb_hip_vecchia_t* h, double* out4_host) {
  API_BEGIN();
  if (!h || !out4_host) return fail("null argument");
  LaplaceState* s = h->lap;
  if (!s || !gpb::lik_has_aux(s->link)) return fail("gpb_hip_vecchia_laplace_grad_aux_current: the likelihood has no auxiliary parameter");
  if (!s->grad_state || !s->gvec_state) return fail("the gradient wrt the auxiliary parameter needs the state of gpb_hip_vecchia_laplace_grad_current");
  HIP_OK(hipSetDevice(h->device));
  const int n = h->n;
  const int nd = s->re_ptr.empty() ? n : s->n_data;
  const LapWork w = lap_work(h, s, s->g_t);
  HIP_OK(gpb::lap_aux_grad(s->link, w.mode, s->resp(), s->has_fe ? s->d_fe : nullptr, w.dld, w.dW3, w.sv, n, s->d_dptr, s->d_o, h->stream));
  double o3[3];
  HIP_OK(hipMemcpyAsync(o3, s->d_o, sizeof(double) * 3, hipMemcpyDeviceToHost, h->stream));
  HIP_OK(hipStreamSynchronize(h->stream));
  if (!gpb::lik_info_depends_on_mode(s->link)) return lap_grad_aux_fisher_laplace(h, s, w, o3, nd, out4_host);
  const double r = s->aux;
  double nld;
  switch (s->link) {      // CalcGradNegLogLikAuxPars
    case gpb::kBeta: nld = -r * o3[0]; break;      // grad[0] = -precision * sum_d w_d (...) (likelihoods.h:14229-14241)
    case gpb::kGamma: nld = o3[0] - nd * (std::log(r) + 1.0 - host_digamma(r)) - s->sum_log_y; nld *= r; break;      // :14189-14202
    case gpb::kNegativeBinomial: nld = o3[0] + nd * r * (host_digamma(r) - std::log(r) - 1.0); break;      // :14203-14215
    default: return fail("gpb_hip_vecchia_laplace_grad_aux_current: the gradient of likelihood id %d is missing", s->link);
  }
  out4_host[0] = nld + 0.5 * o3[1] + o3[2];
  out4_host[1] = nld; out4_host[2] = 0.5 * o3[1]; out4_host[3] = o3[2];
  API_END();
}

/* Standard errors of (sigma2, sigma1_2, rho) of a Gaussian Vecchia model from the stochastic (Hutchinson) Fisher information on the ORIGINAL
   scale: REModelTemplate::CalcFisherInformation_Vecchia (include/GPBoost/re_model_template.h:10137-10230, the default since
   use_stochastic_trace_for_Fisher_information_Vecchia_ = true, :6033) behind CalcStdDevCovPar / GPB_GetCovPar(calc_std_dev = true):
       v_0 = Psi^-1 z,   v_k = B' D^-1 (-dB_k Psi z + dD_k B^-T z) - dB_k' B^-T z,   FI_kl = mean_z (v_k . v_l) / 2,   se = sqrt(diag(FI^-1))
   with the reference's probe vectors (GenRandVecNormalParallel(seed_rand_vec_trace, run id 0): lap_draw).  Everything O(n t) runs on the device with the
   level-scheduled solves of the Laplace path: ONE pass of the two triangular solves gives B^-T Z and B^-1 D B^-T Z for the whole probe
   block; dB_k = -dA_k come from the per-point derivative kernel (nugget included) and are multiplied in the level-ordered layouts (LapDerivEntries).
   With f_0 = 1 / sigma2, f_var = 1 / sigma1_2, f_rho = -1 / rho (chain rule from the log scale of the transformed parameters):
       v_0 = f_0 B' D^-1 B z,        v_k = f_k [ B' D^-1 (dA_k U + dD_k o T) + dA_k' T ],   T = B^-T z, U = B^-1 (D o T)   (sigma2 cancels). */
int gpb_hip_vecchia_fisher_std_errors(gpb_hip_vecchia_t* h, int cov_type, double sigma2, double sigma1_2, double rho, double ratio, double a,
                                      int num_rand_vec, int seed_rand_vec, double* se3_host) {
  API_BEGIN();
  if (!h || !se3_host) return fail("null argument");
  if (!h->has_nn) return fail("neighbours have not been determined");
  if (h->i_begin != 0 || h->i_end != h->n) return fail("the Fisher information needs the whole factor on one device (shard is [%d,%d))", h->i_begin, h->i_end);
  if (num_rand_vec < 1) return fail("num_rand_vec must be positive");
  if (h->m > 126) return fail("standard errors: the per-point derivative kernel handles at most 126 neighbours (this model has %d)", h->m);
  if (h->d > 3) return fail("standard errors: the per-point derivative kernel handles coordinate dimensions 1..3 (this model has %d)", h->d);
  HIP_OK(hipSetDevice(h->device));
  if (!h->lap) h->lap = new LaplaceState();
  LaplaceState* s = h->lap;
  s->grad_state = false; s->gvec_state = false;
  const int n = h->n, m = h->m, t = num_rand_vec;
  hipStream_t st = h->stream;
  if (alloc_factor(h)) return -1;
  if (lap_launch_factor(h, cov_type, ratio, a, 1)) return -1;
  HIP_OK(hipStreamSynchronize(st));
  h->has_factor = false; h->u_stale = false; h->has_yaux = false;   // the factor on the device no longer belongs to a y_aux computed earlier
  if (!h->has_transpose && build_transpose(h)) return -1;
  if (!h->has_levels && build_levels(h, s)) return -1;              // (the level schedules depend on the neighbour table only)
  if (!s->d_Ds) HIP_OK(hipMalloc(&s->d_Ds, sizeof(double) * (size_t)n));
  HIP_OK(gpb::lap_scatter(h->d_D, s->d_sigma, n, s->d_Ds, st));
  const LapWork w = lap_work(h, s, t);                  // (the chunk geometry; this computation has its own workspace)
  const int NCB = w.NCB, tch = w.tch, tc = w.tc;
  const size_t blk = w.nb;
  // workspace of this computation only (freed at the end): probes + 8 blocks + dD in storage order
  DevBuf<double> d_ws;
  HIP_OK(d_ws.alloc(blk * 9 + (size_t)n * 2));
  HIP_OK(hipMemsetAsync(d_ws, 0, sizeof(double) * (blk * 9 + (size_t)n * 2), st));
  double *Z = d_ws, *T = d_ws + blk, *U = d_ws + 2 * blk, *V0 = d_ws + 3 * blk, *V1 = d_ws + 4 * blk, *V2 = d_ws + 5 * blk, *P = d_ws + 6 * blk,
         *H = d_ws + 7 * blk, *Q = d_ws + 8 * blk, *dDs = d_ws + 9 * blk;
  std::vector<double> rv(blk);                           // (the columns padding the last chunk repeat real ones: they are not averaged, and columns are independent)
  lap_draw(seed_rand_vec, 0u, n, s->sigma.data(), t, w, rv.data());
  HIP_OK(hipMemcpyAsync(Z, rv.data(), sizeof(double) * blk, hipMemcpyHostToDevice, st));
  HIP_OK(hipStreamSynchronize(st));
  const gpb::LapLevels lv = make_levels(h, s);
  for (LaplaceState::Tri* tr : { &s->fwd, &s->bwd })
    HIP_OK(gpb::lap_permute_factor(h->d_A, tr->hpos, tr->opos, (size_t)tr->nslots * 32, tr->novf, tr->hent, tr->oent, st));
  HIP_OK(gpb::lap_dense_build(lv.fdense, h->d_A, st));      // the inverses of the solves' dense blocks for this A
  HIP_OK(gpb::lap_dense_build(lv.bdense, h->d_A, st));
  const double* Ds = s->d_Ds;
  HIP_OK(gpb::lap_vadu(lv, n, Ds, Z, U, T, tch, NCB, st));                       // T = B^-T Z,  U = B^-1 (D o T)
  HIP_OK(gpb::lap_apply(lv, n, Ds, nullptr, Z, V0, P, tch, NCB, st));             // V0 = B' D^-1 B Z
  LapDerivEntries de;
  if (LapDerivEntries::alloc_dA(s, n, m) || LapDerivEntries::update(s, lv, st, false, &de)) return -1;
  for (int k = 0; k < 2; ++k) {            // k = 0: variance ratio, k = 1: range  (derivatives wrt the LOG of the transformed parameters)
    double* Vk = k == 0 ? V1 : V2;
    HIP_OK(gpb::lap_factor_deriv(h->d_pts, h->d_nn, h->d_A, n, m, cov_type, h->d == 3 ? 1 : 0, ratio, a, ratio + 1.0, 1.0, k == 0 ? 1 : 0,
                                 s->d_dA, s->d_dD, st));
    HIP_OK(gpb::lap_scatter(s->d_dD, s->d_sigma, n, dDs, st));
    if (LapDerivEntries::update(s, lv, st, true, &de)) return -1;
    HIP_OK(gpb::lap_mul(de.fwd, n, U, P, tch, NCB, st));                            // P = dA_k U
    HIP_OK(gpb::lap_fisher_mid(P, T, Ds, dDs, n, tch, NCB, H, st));                 // H = (dA_k U + dD_k o T) / D
    HIP_OK(gpb::lap_Bt(lv, n, H, Q, tch, NCB, st));                                 // Q = B' H
    HIP_OK(gpb::lap_mul(de.bwd, n, T, P, tch, NCB, st));                            // P = dA_k' T
    HIP_OK(gpb::lap_lincomb(Vk, Q, P, 1.0, 1.0, (int)blk, st));                     // V_k = Q + P
  }
  DevBuf<double> d_dots;
  HIP_OK(d_dots.alloc((size_t)6 * tc));
  HIP_OK(gpb::lap_coldots(V0, V1, V0, n, tch, NCB, d_dots, st));                    // 00, 10
  HIP_OK(gpb::lap_coldots(V1, V2, V1, n, tch, NCB, d_dots + 2 * tc, st));           // 11, 21
  HIP_OK(gpb::lap_coldots(V0, V2, V2, n, tch, NCB, d_dots + 4 * tc, st));           // 02, 22
  std::vector<double> dots((size_t)6 * tc);
  HIP_OK(hipMemcpyAsync(dots.data(), d_dots, sizeof(double) * dots.size(), hipMemcpyDeviceToHost, st));
  HIP_OK(hipStreamSynchronize(st));
  const double f[3] = { 1.0 / sigma2, 1.0 / sigma1_2, -1.0 / rho };
  if (fisher_se_from_dots(dots, t, tc, f, se3_host)) return -1;
  API_END();
}

}  // extern "C"
