// gpboost_amd/csrc/gpb_laplace.inc -- included at the end of gpb_hip.cpp (same translation unit: uses gpb_hip_vecchia,
// fail(), HIP_OK, vecchia_launch, build_transpose).
//
// Host control flow of the Vecchia-Laplace approximation for a Bernoulli-logit likelihood with the reference's default
// iterative methods (BASELINE config 4 / SURVEY.md section 8 row a13):
//   FindModePostRandEffCalcMLLVecchia     include/GPBoost/likelihoods.h:3773-4059   Newton + Armijo backtracking
//   Inv_SigmaI_plus_ZtWZ_Vecchia_iterative :16264-16348 -> src/GPBoost/CG_utils.cpp:21-108 (CGVecchiaLaplaceVec, "vadu")
//   CalcLogDetStochVecchia                 :16376-16525 -> CG_utils.cpp:110-229 (CGTridiagVecchiaLaplace), :1035-1051
//   GenRandVecNormalParallel               CG_utils.cpp:978-994 (probe vectors; libstdc++ engine + distribution)
// Everything O(n) runs on the device (laplace_kernels.hip); the host keeps the loop counters, reads ONE residual norm
// (or t of them) per CG iteration, and diagonalises the t small Lanczos tridiagonals at the end.
#include "laplace_kernels.h"
#include "lik_table.h"
#include "pivchol_kernels.h"

#include <chrono>
#include <random>

// LaplaceState::pc_type, cg_preconditioner_type of the iterative methods.  The values are the ABI of gpb_hip_vecchia_laplace_set_preconditioner.
enum LapPc : int {
  kPcVadu = 0,              // P = B^T (D^-1 + W) B, the (Sigma^-1 + W) form of the solves
  kPcPivChol = 1,           // "pivoted_cholesky": P = W^-1 + L_k L_k^T, the (W^-1 + Sigma) form
  kPcFitc = 2,              // "fitc": P = diag(W^-1 + Sigma_m[0][0] - ||V_i||^2) + C Sigma_m^-1 C', the (W^-1 + Sigma) form
  kPcVecchiaResponse = 3,   // "vecchia_response": P^-1 = B_p' D_p^-1 B_p, the Vecchia factor of W^-1 + Sigma (evaluation only)
  kPcVifdu = 4,             // "vifdu": full-scale Vecchia only, the (Sigma^-1 + W) form with Sigma^-1 = S - Q M^-1 Q'
  kPcNone = 5               // "none": the same form without a preconditioner
};
inline bool pc_has_lowrank(int pc) { return pc == kPcPivChol || pc == kPcFitc; }             // holds the low-rank factor d_pcL; the only ones besides vadu the gradient is built for
inline bool pc_vif_only(int pc) { return pc == kPcVifdu || pc == kPcNone; }                    // belongs to full-scale Vecchia handles only

struct LaplaceState {
  int n = 0, m = 0, t = 0, p_max = 0, seed = 0;
  struct Tri {                    // one level-scheduled triangular solve in level order (laplace_kernels.h: LapTri)
    int* ptr = nullptr; int* lsplit = nullptr; int4* meta = nullptr; int* hpos = nullptr; int* opos = nullptr;
    gpb::LapEnt* hent = nullptr; gpb::LapEnt* oent = nullptr;
    gpb::LapEnt* hent_g = nullptr; gpb::LapEnt* oent_g = nullptr;      // the same layout with the entries of dA / d log(range) (gradient only)
    int nlev = 0, nslots = 0; size_t novf = 0;
    int npad = 0, nmulti = 0, nlong = 0;      // padding slots, rows of several slots, slots of more than 64 entries (what the schedule holds: gpb_hip_vecchia_laplace_ops_check)
    std::vector<int> ptr_host;      // host copy of ptr (slot range of a run of levels: the barrier-free solves)
    // dense block of the solve (laplace_kernels.h: LapDense): K rows, device arrays, host level boundaries
    int dK = 0; int* d_rows = nullptr; int* d_iptr = nullptr; int* d_icol = nullptr; int* d_ipos = nullptr;
    int* d_optr = nullptr; int* d_osrc = nullptr; int* d_opos = nullptr; double* d_inv = nullptr; double* d_tbuf = nullptr;
    std::vector<int> blev;
  } fwd, bwd;
  std::vector<gpb::LapSeg> fseg, bseg;   // launch segments of the two solves (runs of narrow levels / single wide levels)
  std::vector<int> sigma;         // Vecchia position -> storage slot of this workspace (Morton rank of the coordinates)
  int* d_sigma = nullptr;
  double* d_Ds = nullptr;         // D in storage order
  std::vector<int> labels;        // y in {0,1}, Vecchia order (host copy; uploaded in storage order)
  int* d_y = nullptr; bool has_y = false, y_dirty = false;
  std::vector<double> fe;         // fixed effects (offset of the location parameter), Vecchia order; uploaded in storage order
  double* d_fe = nullptr; bool has_fe = false, fe_dirty = false;
  // repeated locations (gpb_hip_vecchia_laplace_set_data_map): n_data data belong to the n random effects of the handle; re_ptr (n + 1, Vecchia
  // order) = CSR of a random effect's data in the order labels / fe are handed over (grouped by random effect); d_dptr = the same CSR in the
  // workspace's storage order with the data regrouped accordingly.  Empty = one datum per random effect.
  int n_data = 0; std::vector<int> re_ptr; int* d_dptr = nullptr; bool map_dirty = false;
  int link = gpb::kBernoulliLogit;   // a gpb::Lik: row of lik_table.h (gpb_hip_vecchia_laplace_set_likelihood)
  double log_norm_const = 0.;     // log_normalizing_constant_: part of every LogLikelihood() value (likelihoods.h:11290)
  // likelihoods with an auxiliary parameter (round 5): aux = shape of gamma / negative_binomial (gpb_hip_vecchia_laplace_set_aux_pars); gamma's
  // real-valued response (host copy in the order of `labels`, device copy in storage order); sum_log_y = aux_log_normalizing_constant_ of gamma
  // (likelihoods.h:10576-10583), sum_lgamma_y1 = sum lgamma(y + 1) of negative_binomial (:10585-10592); the normalising constant itself depends on
  // aux and is renewed when aux or the response changed (norm_dirty)
  double aux = 1.0; std::vector<double> resp_real; double* d_yd = nullptr; double sum_log_y = 0., sum_lgamma_y1 = 0.; bool norm_dirty = false;
  // sample weights (round 5; likelihoods.h:666-668): host copy in the order of `labels`, device copy in storage order; every per-datum term of the likelihood
  // is multiplied by them, the per-datum parts of the normalising constants too (w_dirty: upload + constants at the next evaluation)
  std::vector<double> weights; double* d_w = nullptr; bool w_dirty = false;
  // real_resp: the response is real-valued (gamma always; the logit / probit links when it is a proportion: binomial_*, quasi_bernoulli_*); binomial: the normalising
  // constant sum lgamma(w + 1) - lgamma(k + 1) - lgamma(w - k + 1), k = w y, of the binomial likelihoods (likelihoods.h:10612-10622, :10884-10886)
  bool real_resp = false, binomial = false;
  double aux2 = 2.0;              // second auxiliary parameter (t: the degrees of freedom; aux = its scale)
  gpb::LikResp resp() const { return gpb::LikResp{ d_y, (gpb::lik_real_only(link) || real_resp) ? d_yd : nullptr, aux, weights.empty() ? nullptr : d_w, aux2 }; }
  double* d_vec = nullptr;        // 16 n-vectors (mode finding)
  double* d_rv = nullptr;         // probes N(0,1), layout [chunk of 4 columns][storage slot][4]
  double* d_blk = nullptr;        // 5 blocks of the same layout (R, Z, H, V, T)
  double* d_sc = nullptr;         // CG scalars: [5] vector CG, [5 t] block CG, [2 t p_max] Lanczos coefficients
  double* d_o = nullptr;          // 8 doubles of reduction results
  int* d_err = nullptr;           // device word the barrier-free triangular solves set when a bounded spin ran out
  // barrier-free triangular solves (one launch per solve; 0 = level-per-launch solves, the fallback lap_check_solves switches to when a bounded spin ran out): bit 0 single vectors with one 16-lane group
  // per row (mode finding: 243 -> 140 ms per evaluation at config 4), bit 2 the probe block with one WAVEFRONT per (row, unit of four chunks) and
  // 32-byte L1-bypassing gathers (round 4, lap_sptrsv_sfw_kernel: log-determinant at config 4 363 -> 279 ms, profiles/r04_c_*).  The block with
  // one 16-lane group per (row, chunk) was measured slower than the level launches (362 -> 442 ms, profiles/r03_h_*) and is gone.
  int syncfree = 5;
  double* h_o = nullptr;          // pinned mirror: [0..8) reductions, [8..8+t) residual norms
  bool has_mode = false;
  // ---- gradient of the approximate marginal likelihood (gpb_laplace_grad.inc) ----
  double* d_gblk = nullptr;       // 2 blocks kept from the log-determinant's block CG: U = (Sigma^-1 + W)^-1 Z and PI_Z = P^-1 Z
  size_t gblk_cap = 0;
  double* d_gvec = nullptr;       // 6 n-vectors: previous mode, third derivatives, d logdet / d mode, implicit solve, SigmaI_deriv mode, dD (storage order)
  double* d_dA = nullptr;         // dA / d log(range), Vecchia order [n][m]
  double* d_dD = nullptr;         // dD / d log(range), Vecchia order
  double* d_go = nullptr; double* h_go = nullptr; size_t go_cap = 0;   // column dot products of the trace estimators (device, pinned mirror)
  bool grad_state = false;        // U / PI_Z / the factor belong to the current mode and parameters
  bool gvec_state = false;        // d logdet / d mode and the implicit solve (d_gvec) belong to them too (gpb_hip_vecchia_laplace_grad_current has run)
  int g_cov = 0, g_t = 0; double g_var = 0., g_a = 0.;
  // ---- cg_preconditioner_type = "pivoted_cholesky" (gpb_hip_vecchia_laplace_set_preconditioner; pivchol_kernels.hip) ----
  int pc_type = kPcVadu;          // a LapPc
  int pc_rank = 50;               // fitc_piv_chol_preconditioner_rank_ (re_model_template.h:5922 default_piv_chol_preconditioner_rank_)
  int pc_k = 0;                   // columns of L_k = min(rank, n)
  double* d_pcL = nullptr;        // L_k [n][pc_k], rows in storage order; renewed by every evaluation (the covariance parameters changed)
  double* d_pcM = nullptr;        // (I_k + L_k^T W L_k)^-1, k x k
  double* d_pcG = nullptr;        // packed lower triangle of L_k^T W L_k
  double* d_pcpart = nullptr; size_t pcpart_cap = 0;     // partial sums of the tall-skinny reductions
  double* d_pcx2 = nullptr; size_t pcx2_cap = 0;         // small operands [chunk][k][nc]
  double* d_pcrv2 = nullptr;      // rand_vec_trace_I2_ (k x t normals) in the layout [chunk][k][4]
  double* d_pcdiag = nullptr; int* d_pcpi = nullptr; int* d_pcpos = nullptr; int* d_pcdone = nullptr;    // work arrays of the factorisation
  double pc_logdet = 0.;          // log|I_k + L_k^T W L_k| of the last pc_refresh
  int pc_cols = 0;                // columns the last factorisation computed before its error bound was met
  int rv_pc = -1, rv_k = -1;      // preconditioner type / k the cached probe vectors were drawn for
  // ---- cg_preconditioner_type = "fitc" (kPcFitc): P = diag(W^-1 + Sigma_m[0][0] - ||V_i||^2) + C Sigma_m^-1 C'; d_pcL holds C, the cross-covariance with the inducing points ----
  std::vector<double> pc_ip;      // inducing points, k x 3 row-major (unused coordinates 0; gpb_hip_vecchia_laplace_set_inducing_points)
  int pc_nip = 0;
  double* d_pcip = nullptr;       // the same on the device
  double* d_pcV = nullptr;        // V = (L_m^-1 C')' [n][k], storage order (chol_ip_cross_cov^T)
  double* d_pcvn2 = nullptr;      // ||V_i||^2
  double* d_pcwp = nullptr;       // D^-1, the diagonal of the preconditioner's inverse for the current W
  double* d_pctmp = nullptr; size_t pctmp_cap = 0;   // [n][kq] scratch of the cross-covariance kernels (Vecchia order), twice
  std::vector<double> pc_Linv, pc_Minv;   // host: inverse of chol(Sigma_m) (pc_factor_fitc) and (Sigma_m + C' D^-1 C)^-1 of the last pc_refresh (the VIF gradient's k x k algebra)
  double* d_pcI = nullptr;        // k x k identity (multiplier of plain L' X reductions)
  std::vector<double> pc_Sm;      // Sigma_m with the jittered diagonal, k x k
  double pc_logdet_Sm = 0.;
  const double* pc_wp(const double* W) const { return pc_type == kPcFitc ? d_pcwp : W; }
  // ---- cg_preconditioner_type = "vecchia_response" (kPcVecchiaResponse): P^-1 = B_p' D_p^-1 B_p, the Vecchia factor of W^-1 + Sigma on the same neighbour sets, renewed for
  // every W by a MODE_FACTOR launch of the point kernel with the diagonal additions 1 / W_i (likelihoods.h:16315-16323; CalcVecchiaApproxLatentAddDiagonal) ----
  double* d_vrA = nullptr;        // A_p [n][m], Vecchia order
  double* d_vrD = nullptr;        // D_p (+ the jitter), Vecchia order; then [n] u (unused), [n] the nuggets 1 / W_i + jitter (Vecchia order)
  double* d_vrDs = nullptr;       // D_p and sqrt(D_p) in storage order
  gpb::LapEnt* vr_hent[2] = { nullptr, nullptr }; gpb::LapEnt* vr_oent[2] = { nullptr, nullptr };     // A_p in the level-ordered layouts of fwd / bwd
  double* d_vrinv = nullptr;      // inverse of the forward solve's dense block for A_p
  double* d_vrtmp = nullptr; size_t vrtmp_cap = 0;     // one block vector of scratch
  int vr_cov = 0; double vr_var = 0., vr_a = 0.;      // this evaluation's kernel and parameters (pc_refresh factors with them)  // ---- full-scale Vecchia ("VIF") with a non-Gaussian likelihood (the handle has inducing points: h->vif_k > 0; FindModePostRandEffCalcMLLFSVA, likelihoods.h:3379-3750):
  // Sigma = V V' + B^-1 D B^-T with (B, D) the factor of the RESIDUAL process; "fitc" preconditioner = the (W^-1 + Sigma) form of the solves ----
  int vif_kk = 0;                 // k the buffers below were sized for
  double* d_vifV = nullptr;       // V = (L_m^-1 C')' [n][k], rows in storage order (chol_ip_cross_cov^T)
  double* d_vifBC = nullptr;      // B C [n][k], rows in storage order (B_cross_cov)
  double* d_vifones = nullptr;    // n ones, then n x 1 / D (storage order)
  double* d_vifu = nullptr;       // u' = W u of the previous Newton step (mode_update_part, likelihoods.h:3540-3543)
  double* d_vifI = nullptr;       // k x k: -I, then +I (the small multipliers of pc_ltwx)
  double* d_vifx2 = nullptr; size_t vifx2_cap = 0;
  double* h_vk = nullptr;         // pinned: 2 slots of k doubles ((B C)' D^-1 B x of the quadratic forms)
  std::vector<double> vif_cholM;  // lower Cholesky factor of the Woodbury matrix Sigma_m + (B C)' D^-1 (B C), k x k row-major
  std::vector<double> vif_Sm, vif_Linv;   // Sigma_m (jittered diagonal) and the inverse of its Cholesky factor
  double vif_logdet_Sm = 0.;
  std::vector<double> vif_G;      // (B C)' D^-1 (B C), k x k row-major
  // gradient (gpb_laplace_grad.inc): storage-order copies [n][k] of C, dC / d log(range), B dC; the preconditioner's dC_p / d log(range); scratch
  double* d_vifC = nullptr; double* d_vifdC = nullptr; double* d_vifBdC = nullptr; double* d_pcdL = nullptr; double* d_vifT = nullptr; size_t vifT_cap = 0;
  double* d_vifq = nullptr; size_t vifq_cap = 0;      // small operands of the block reductions
  bool vif_grad_inputs = false;   // dC, B dC (and the preconditioner's dC_p) belong to the current parameters
  // "vifdu" (kPcVifdu) / "none" (kPcNone): the (Sigma^-1 + W) form with Sigma^-1 = S - Q M^-1 Q' (CGFVIFLaplaceVec / CGTridiagVIFLaplace, CG_utils.cpp:501-742)
  std::vector<double> vif_M;      // the Woodbury matrix M = Sigma_m + (B C)' D^-1 (B C), k x k row-major (its factor: vif_cholM)
  double* d_vifMinv = nullptr;    // M^-1, then (M - (D^-1 B C)' diag((W + D^-1)^-1) (D^-1 B C))^-1 ("vifdu", renewed for every W): 2 x k x k
  double* d_vifblk = nullptr; size_t vifblk_cap = 0;    // two block vectors + two n-vectors of scratch
  double* d_vifrv3 = nullptr;     // rand_vec_trace_I3_ (n x t normals, generator counter 2) in the probe block's layout
  double vif_logdet_M = 0., vif_logdet_MM = 0.;
};


static void laplace_state_free(LaplaceState* s) {
  if (!s) return;
  for (LaplaceState::Tri* t : { &s->fwd, &s->bwd }) {
    dev_free(t->ptr); dev_free(t->lsplit); dev_free(t->meta); dev_free(t->hpos); dev_free(t->opos); dev_free(t->hent); dev_free(t->oent);
    dev_free(t->hent_g); dev_free(t->oent_g);
    dev_free(t->d_rows); dev_free(t->d_iptr); dev_free(t->d_icol); dev_free(t->d_ipos); dev_free(t->d_optr); dev_free(t->d_osrc); dev_free(t->d_opos);
    dev_free(t->d_inv); dev_free(t->d_tbuf);
  }
  dev_free(s->d_pcL); dev_free(s->d_pcM); dev_free(s->d_pcG); dev_free(s->d_pcpart); dev_free(s->d_pcx2); dev_free(s->d_pcrv2);
  dev_free(s->d_pcdiag); dev_free(s->d_pcpi); dev_free(s->d_pcpos); dev_free(s->d_pcdone);
  dev_free(s->d_pcip); dev_free(s->d_pcV); dev_free(s->d_pcvn2); dev_free(s->d_pcwp); dev_free(s->d_pctmp);
  dev_free(s->d_vrA); dev_free(s->d_vrD); dev_free(s->d_vrDs); dev_free(s->d_vrinv); dev_free(s->d_vrtmp);
  dev_free(s->d_vifV); dev_free(s->d_vifBC); dev_free(s->d_vifones); dev_free(s->d_vifu); dev_free(s->d_vifI); dev_free(s->d_vifx2);
  dev_free(s->d_vifC); dev_free(s->d_vifdC); dev_free(s->d_vifBdC); dev_free(s->d_pcdL); dev_free(s->d_vifT); dev_free(s->d_vifq); dev_free(s->d_pcI);
  dev_free(s->d_vifMinv); dev_free(s->d_vifblk); dev_free(s->d_vifrv3);
  if (s->h_vk) (void)hipHostFree(s->h_vk);
  for (int q = 0; q < 2; ++q) { dev_free(s->vr_hent[q]); dev_free(s->vr_oent[q]); }
  dev_free(s->d_gblk); dev_free(s->d_gvec); dev_free(s->d_dA); dev_free(s->d_dD); dev_free(s->d_go);
  if (s->h_go) (void)hipHostFree(s->h_go);
  dev_free(s->d_sigma); dev_free(s->d_Ds); dev_free(s->d_y); dev_free(s->d_yd); dev_free(s->d_w); dev_free(s->d_fe); dev_free(s->d_dptr); dev_free(s->d_vec); dev_free(s->d_rv); dev_free(s->d_blk); dev_free(s->d_sc); dev_free(s->d_o); dev_free(s->d_err);
  if (s->h_o) (void)hipHostFree(s->h_o);
  delete s;
}

namespace {

// device memory of one call: freed on every way out of the scope
template <class T>
struct DevBuf {
  T* p = nullptr;
  DevBuf() = default;
  DevBuf(DevBuf&& o) noexcept : p(o.p) { o.p = nullptr; }
  DevBuf& operator=(DevBuf&& o) noexcept { if (this != &o) { dev_free(p); p = o.p; o.p = nullptr; } return *this; }
  DevBuf(const DevBuf&) = delete;
  DevBuf& operator=(const DevBuf&) = delete;
  ~DevBuf() { dev_free(p); }
  hipError_t alloc(size_t count) { return hipMalloc(&p, sizeof(T) * count); }
  operator T*() const { return p; }
};

// Dependency levels of the two triangular solves with B = I - A (row i depends on rows nn[i][.] < i) and B^T (row j
// depends on the rows i > j that have j as a neighbour).  Rows of one level are independent; inside a level they are kept in
// ascending order (counting sort), so the schedule -- and with it every result -- is deterministic.  Each solve gets its
// matrix in LEVEL ORDER: position q -> row, a 32-wide head of (source row, position in A) plus an overflow CSR.
int upload_tri(int n, const std::vector<int>& lev, int nlev, const std::vector<int>& e_ptr, const std::vector<int>& e_src,
               const std::vector<int>& e_pos, const std::vector<int>& sigma, LaplaceState::Tri* t, std::vector<gpb::LapSeg>* segs, bool dense_at_tail) {
  const int RR = gpb::kTriRowsPerRound;
  std::vector<int> lptr(nlev + 1, 0), lrows(n);
  for (int i = 0; i < n; ++i) lptr[lev[i] + 1]++;
  for (int l = 0; l < nlev; ++l) lptr[l + 1] += lptr[l];
  {
    std::vector<int> fill(lptr.begin(), lptr.end() - 1);
    for (int i = 0; i < n; ++i) lrows[fill[lev[i]]++] = i;
  }
  // inside a level: by storage slot, so that the rows sharing a wavefront are spatial neighbours (their gathers overlap)
  for (int l = 0; l < nlev; ++l)
    std::sort(lrows.begin() + lptr[l], lrows.begin() + lptr[l + 1], [&](int a, int b) { return sigma[a] < sigma[b]; });
  // slots: a row of len entries takes nseg = ceil(len / 64) consecutive slots (at most 64, then the slots get longer) that all lie
  // in the same round of 64 positions counted from the start of the level (padding slots, row = -1, keep that true)
  std::vector<int> ptr(nlev + 1, 0), lsplit(nlev + 1, 0), rows, nseg, hsrc, hpos, optr(1, 0), osrc, opos;
  rows.reserve(n + n / 8); nseg.reserve(n + n / 8); hsrc.reserve((size_t)(n + n / 8) * 32); hpos.reserve((size_t)(n + n / 8) * 32);
  auto push_slot = [&](int row, int ns, const int* src, const int* pos, int cnt) {
    rows.push_back(row); nseg.push_back(ns);
    for (int l = 0; l < 32; ++l) { hsrc.push_back(l < cnt ? sigma[src[l]] : 0); hpos.push_back(l < cnt ? pos[l] : -1); }
    for (int l = 32; l < cnt; ++l) { osrc.push_back(sigma[src[l]]); opos.push_back(pos[l]); }
    optr.push_back((int)osrc.size());
  };
  t->npad = t->nmulti = t->nlong = 0;
  for (int l = 0; l < nlev; ++l) {
    ptr[l] = (int)rows.size();
    for (int k = lptr[l]; k < lptr[l + 1]; ++k) {
      const int i = lrows[k];
      const int len = e_ptr[i + 1] - e_ptr[i];
      int ns = std::max(1, (len + 63) / 64);
      if (ns > RR) ns = RR;
      if (ns > 1) lsplit[l] = 1;
      const int per = (len + ns - 1) / ns;                    // entries per slot (<= 64 unless len > 64 * 64)
      const int in_round = ((int)rows.size() - ptr[l]) % RR;
      if (in_round + ns > RR) for (int z = in_round; z < RR; ++z) { push_slot(-1, 0, nullptr, nullptr, 0); t->npad++; }
      if (ns > 1) t->nmulti++;
      for (int sgi = 0; sgi < ns; ++sgi) {
        const int lo = std::min(len, sgi * per), hi = std::min(len, lo + per);
        if (hi - lo > 64) t->nlong++;
        push_slot(sgi == 0 ? sigma[i] : -1, sgi == 0 ? ns : 0, e_src.data() + e_ptr[i] + lo, e_pos.data() + e_ptr[i] + lo, hi - lo);
      }
    }
  }
  ptr[nlev] = (int)rows.size();
  const int nslots = (int)rows.size();
  if ((unsigned long long)nslots * 32ull * sizeof(gpb::LapEnt) >= (1ull << 32))      // the kernels form byte offsets in 32 bits
    return fail("the Vecchia-Laplace workspace supports up to ~8e6 matrix slots per solve (this model needs %d)", nslots);
  t->novf = osrc.size();
  if (osrc.empty()) { osrc.push_back(0); opos.push_back(0); }      // the kernels clamp masked overflow loads to entry 0
  t->nlev = nlev; t->nslots = nslots; t->ptr_host = ptr;
  // launch segments: a level with >= kWide slots is launched on its own, one workgroup per round of 64 slots and right-hand
  // side; runs of narrower levels share one launch (one workgroup per right-hand side, barrier per level)
  const int kWide = 256;
  // the dense block: the run of narrow levels at the head (forward solve) or at the tail (backward solve), at most kDenseMax rows --
  // there the levels hold a handful of rows each (the first points of the ordering all depend on each other) and a level costs a
  // dependent L2 round trip whatever its size
  const int kDenseMax = 8192, kDenseMinLevels = 16;
  int La = dense_at_tail ? nlev : 0, Lb = La, K = 0;
  if (!dense_at_tail) {
    while (Lb < nlev && ptr[Lb + 1] - ptr[Lb] < kWide && K + (lptr[Lb + 1] - lptr[Lb]) <= kDenseMax) { K += lptr[Lb + 1] - lptr[Lb]; ++Lb; }
  } else {
    while (La > 0 && ptr[La] - ptr[La - 1] < kWide && K + (lptr[La] - lptr[La - 1]) <= kDenseMax) { K += lptr[La] - lptr[La - 1]; --La; }
  }
  if (Lb - La < kDenseMinLevels) { La = Lb = dense_at_tail ? nlev : 0; K = 0; }
  segs->clear();
  for (int l = 0; l < nlev;) {
    if (l >= La && l < Lb) { l = Lb; continue; }           // the block's levels are not launched
    const int lend = l < La ? La : nlev;
    const int cnt = ptr[l + 1] - ptr[l];
    if (cnt >= kWide) { segs->push_back({ l, l + 1, (cnt + RR - 1) / RR, 1 }); ++l; continue; }
    int e = l, rounds = 0;
    while (e < lend && ptr[e + 1] - ptr[e] < kWide) { rounds += (ptr[e + 1] - ptr[e] + RR - 1) / RR; ++e; }
    segs->push_back({ l, e, 1, rounds });
    l = e;
  }
  auto up = [&](int** d, const std::vector<int>& v) -> int {
    dev_free(*d);
    HIP_OK(hipMalloc(d, sizeof(int) * v.size()));
    HIP_OK(hipMemcpy(*d, v.data(), sizeof(int) * v.size(), hipMemcpyHostToDevice));
    return 0;
  };
  if (up(&t->ptr, ptr) || up(&t->lsplit, lsplit) || up(&t->hpos, hpos) || up(&t->opos, opos)) return -1;
  t->dK = K;
  t->blev.clear();
  dev_free(t->d_inv); t->d_inv = nullptr; dev_free(t->d_tbuf); t->d_tbuf = nullptr;
  if (K > 0) {
    std::vector<int> loc(n, -1), brow(K), iptr(1, 0), icol, ipos, optr(1, 0), osrc, opos_;
    for (int k = 0; k < K; ++k) loc[lrows[lptr[La] + k]] = k;
    for (int l = La; l <= Lb; ++l) t->blev.push_back(lptr[l] - lptr[La]);
    for (int k = 0; k < K; ++k) {
      const int i = lrows[lptr[La] + k];
      brow[k] = sigma[i];
      for (int e = e_ptr[i]; e < e_ptr[i + 1]; ++e) {
        const int c = loc[e_src[e]];
        if (c >= 0) { icol.push_back(c); ipos.push_back(e_pos[e]); }
        else { osrc.push_back(sigma[e_src[e]]); opos_.push_back(e_pos[e]); }
      }
      iptr.push_back((int)icol.size()); optr.push_back((int)osrc.size());
    }
    if (icol.empty()) { icol.push_back(0); ipos.push_back(0); }
    if (osrc.empty()) { osrc.push_back(0); opos_.push_back(0); }
    if (up(&t->d_rows, brow) || up(&t->d_iptr, iptr) || up(&t->d_icol, icol) || up(&t->d_ipos, ipos) || up(&t->d_optr, optr) || up(&t->d_osrc, osrc) ||
        up(&t->d_opos, opos_)) return -1;
    HIP_OK(hipMalloc(&t->d_inv, sizeof(double) * (size_t)K * K));
    HIP_OK(hipMalloc(&t->d_tbuf, sizeof(double) * (size_t)K * gpb::kDenseCols * (1 + gpb::kDenseSplit)));
  }
  std::vector<int4> meta(nslots);
  for (int q = 0; q < nslots; ++q) meta[q] = make_int4(rows[q], nseg[q], optr[q], optr[q + 1]);
  std::vector<gpb::LapEnt> hent((size_t)nslots * 32), oent(osrc.size());
  for (size_t g = 0; g < hent.size(); ++g) hent[g] = { 0.0, hsrc[g], 0 };
  for (size_t g = 0; g < oent.size(); ++g) oent[g] = { 0.0, osrc[g], 0 };
  dev_free(t->meta); dev_free(t->hent); dev_free(t->oent); dev_free(t->hent_g); dev_free(t->oent_g);
  HIP_OK(hipMalloc(&t->meta, sizeof(int4) * meta.size()));
  HIP_OK(hipMalloc(&t->hent, sizeof(gpb::LapEnt) * hent.size()));
  HIP_OK(hipMalloc(&t->oent, sizeof(gpb::LapEnt) * oent.size()));
  HIP_OK(hipMemcpy(t->meta, meta.data(), sizeof(int4) * meta.size(), hipMemcpyHostToDevice));
  HIP_OK(hipMemcpy(t->hent, hent.data(), sizeof(gpb::LapEnt) * hent.size(), hipMemcpyHostToDevice));
  HIP_OK(hipMemcpy(t->oent, oent.data(), sizeof(gpb::LapEnt) * oent.size(), hipMemcpyHostToDevice));
  return 0;
}

// Storage order of the workspace: Morton (Z-order) rank of the coordinates.  The neighbours of a point are spatially close, so
// in this order their entries share cache lines; the Vecchia ordering itself (random) has no such locality.
void morton_order(const gpb_hip_vecchia_t* h, std::vector<int>* sigma) {
  const int n = h->n, d = h->d;
  const int bits = 63 / d > 21 ? 21 : 63 / d;
  std::vector<std::pair<unsigned long long, int>> key(n);
  std::vector<double> lo(d), sc(d);
  for (int c = 0; c < d; ++c) {
    const double* x = h->coords.data() + (size_t)c * n;
    double mn = x[0], mx = x[0];
    for (int i = 1; i < n; ++i) { mn = std::min(mn, x[i]); mx = std::max(mx, x[i]); }
    lo[c] = mn; sc[c] = mx > mn ? ((double)((1ull << bits) - 1)) / (mx - mn) : 0.0;
  }
  for (int i = 0; i < n; ++i) {
    unsigned long long code = 0;
    for (int c = 0; c < d; ++c) {
      const unsigned long long v = (unsigned long long)((h->coords[(size_t)c * n + i] - lo[c]) * sc[c]);
      for (int b = 0; b < bits; ++b) code |= ((v >> b) & 1ull) << (b * d + c);
    }
    key[i] = { code, i };
  }
  std::sort(key.begin(), key.end());
  sigma->assign(n, 0);
  for (int k = 0; k < n; ++k) (*sigma)[key[k].second] = k;
}

// the barrier-free triangular solves bound their spins; a dependency that never arrived leaves a flag instead of a hung device
int lap_check_solves(LaplaceState* s, hipStream_t st) {
  if (!s->d_err) return 0;
  int e = 0;
  HIP_OK(hipMemcpyAsync(&e, s->d_err, sizeof(int), hipMemcpyDeviceToHost, st));
  HIP_OK(hipStreamSynchronize(st));
  if (e) {
    HIP_OK(hipMemsetAsync(s->d_err, 0, sizeof(int), st));
    s->syncfree = 0;      // the level-per-launch solves need no resident grid: this state uses them from now on
    return fail("a barrier-free triangular solve gave up waiting for a dependency (are other kernels occupying the device?); this evaluation is lost, the next ones of this model use the level-per-launch solves");
  }
  return 0;
}

gpb::LapLevels make_levels(const gpb_hip_vecchia_t* h, const LaplaceState* s) {
  auto tri = [](const LaplaceState::Tri& t) { return gpb::LapTri{ t.ptr, t.lsplit, t.meta, t.hent, t.oent, t.nlev, t.nslots, t.novf > 0 ? 1 : 0 }; };
  auto dense = [](const LaplaceState::Tri& t) {
    return gpb::LapDense{ t.dK, t.dK, t.d_rows, t.d_iptr, t.d_icol, t.d_ipos, t.d_optr, t.d_osrc, t.d_opos, t.d_inv, t.d_tbuf, t.blev.data(),
                          t.dK > 0 ? (int)t.blev.size() - 1 : 0 };
  };
  gpb::LapLevels lv{ tri(s->fwd), tri(s->bwd), s->fseg.data(), (int)s->fseg.size(), s->bseg.data(), (int)s->bseg.size(), dense(s->fwd), dense(s->bwd),
                     h->d_A };
  lv.syncfree = s->d_err ? s->syncfree : 0;
  lv.fwd_ptr_host = s->fwd.ptr_host.data(); lv.bwd_ptr_host = s->bwd.ptr_host.data(); lv.err = s->d_err;
  return lv;
}

int build_levels(gpb_hip_vecchia_t* h, LaplaceState* s) {
  const int n = h->n, m = h->m;
  const std::vector<int>& nn = h->nn_host;
  // the "vecchia_response" preconditioner's copies of the layouts below belong to the schedules being replaced
  dev_free(s->d_vrA); dev_free(s->d_vrD); dev_free(s->d_vrDs); dev_free(s->d_vrinv);
  for (int q = 0; q < 2; ++q) { dev_free(s->vr_hent[q]); dev_free(s->vr_oent[q]); }
  morton_order(h, &s->sigma);
  dev_free(s->d_sigma);
  HIP_OK(hipMalloc(&s->d_sigma, sizeof(int) * (size_t)n));
  HIP_OK(hipMemcpy(s->d_sigma, s->sigma.data(), sizeof(int) * (size_t)n, hipMemcpyHostToDevice));
  s->y_dirty = true;           // labels and probes are stored in this order
  s->t = 0;
  std::vector<int> lf(n, 0), lb(n, 0);
  int maxf = 0, maxb = 0;
  for (int i = 0; i < n; ++i) {
    int l = 0;
    for (int j = 0; j < m; ++j) { const int c = nn[(size_t)i * m + j]; if (c >= 0 && lf[c] + 1 > l) l = lf[c] + 1; }
    lf[i] = l; if (l > maxf) maxf = l;
  }
  for (int i = n - 1; i >= 0; --i) {        // lb[i] is final here: every row that has i as a neighbour is > i
    const int l = lb[i] + 1;
    for (int j = 0; j < m; ++j) { const int c = nn[(size_t)i * m + j]; if (c >= 0 && l > lb[c]) lb[c] = l; }
    if (lb[i] > maxb) maxb = lb[i];
  }
  // entries of B's rows (source = neighbour, position in A = i m + j) and of B^T's rows (source = row, same positions)
  std::vector<int> fp(n + 1, 0), fs, fq, bp(n + 1, 0);
  fs.reserve((size_t)n * m); fq.reserve((size_t)n * m);
  for (int i = 0; i < n; ++i) {
    for (int j = 0; j < m; ++j) {
      const int c = nn[(size_t)i * m + j];
      if (c >= 0) { fs.push_back(c); fq.push_back(i * m + j); bp[c + 1]++; }
    }
    fp[i + 1] = (int)fs.size();
  }
  for (int j = 0; j < n; ++j) bp[j + 1] += bp[j];
  std::vector<int> bs(fs.size()), bq(fs.size()), fill(bp.begin(), bp.end() - 1);
  for (int i = 0; i < n; ++i)
    for (int e = fp[i]; e < fp[i + 1]; ++e) { const int c = fs[e]; bs[fill[c]] = i; bq[fill[c]] = fq[e]; fill[c]++; }
  if (upload_tri(n, lf, maxf + 1, fp, fs, fq, s->sigma, &s->fwd, &s->fseg, false)) return -1;
  if (upload_tri(n, lb, maxb + 1, bp, bs, bq, s->sigma, &s->bwd, &s->bseg, true)) return -1;
  h->has_levels = true;
  return 0;
}

// e1^T log(T) e1 of a symmetric tridiagonal (diagonal dg[0..k), sub-diagonal sd[0..k-1)): implicit-shift QL iteration
// that carries only the first row of the eigenvector matrix (Gauss quadrature weights = its squares).  Stands in for
// Eigen::SelfAdjointEigenSolver::computeFromTridiagonal in LogDetStochTridiag (CG_utils.cpp:1035-1051).
double tridiag_quadrature_log(const double* dg, const double* sd, int k) {
  std::vector<double> d(dg, dg + k), e(k, 0.0), w(k, 0.0);
  for (int i = 0; i + 1 < k; ++i) e[i] = sd[i];
  w[0] = 1.0;
  const double eps = 2.220446049250313e-16;
  for (int l = 0; l < k; ++l) {
    for (int sweep = 0; sweep <= 200; ++sweep) {
      int mm = l;
      while (mm < k - 1 && std::fabs(e[mm]) > eps * (std::fabs(d[mm]) + std::fabs(d[mm + 1]))) ++mm;
      if (mm == l) break;
      double g = (d[l + 1] - d[l]) / (2.0 * e[l]);
      double r = std::hypot(g, 1.0);
      g = d[mm] - d[l] + e[l] / (g + std::copysign(r, g));
      double sn = 1.0, cs = 1.0, p = 0.0;
      bool deflated = false;
      for (int i = mm - 1; i >= l; --i) {
        double f = sn * e[i];
        const double b = cs * e[i];
        r = std::hypot(f, g);
        e[i + 1] = r;
        if (r == 0.0) { d[i + 1] -= p; e[mm] = 0.0; deflated = true; break; }
        sn = f / r; cs = g / r;
        g = d[i + 1] - p;
        r = (d[i] - g) * sn + 2.0 * cs * b;
        p = sn * r;
        d[i + 1] = g + p;
        g = cs * r - b;
        f = w[i + 1];
        w[i + 1] = sn * w[i] + cs * f;
        w[i] = cs * w[i] - sn * f;
      }
      if (deflated) continue;
      d[l] -= p; e[l] = g; e[mm] = 0.0;
    }
  }
  double q = 0.0;
  for (int i = 0; i < k; ++i) q += w[i] * std::log(d[i]) * w[i];
  return q;
}

// digamma as GPBoost::digamma (src/GPBoost/DF_utils.cpp:82-125)
inline double host_digamma(double x) {
  if (x <= 0.000001) return -0.57721566490153286060 - 1.0 / x + 1.6449340668482264365 * x;
  double v = 0.0;
  while (x < 8.5) { v -= 1.0 / x; x += 1.0; }
  double r = 1.0 / x;
  v += std::log(x) - 0.5 * r;
  r = r * r;
  return v - r * (1.0 / 12.0 - r * (1.0 / 120.0 - r * (1.0 / 252.0 - r * (1.0 / 240.0 - r * (1.0 / 132.0)))));
}

inline double ms_since(const std::chrono::steady_clock::time_point& t0) {
  return std::chrono::duration<double, std::milli>(std::chrono::steady_clock::now() - t0).count();
}

}  // namespace

extern "C" {

int gpb_hip_vecchia_laplace_set_labels(gpb_hip_vecchia_t* h, const int32_t* y01) {
  API_BEGIN();
  if (!h || !y01) return fail("null argument");
  if (!h->lap) h->lap = new LaplaceState();
  LaplaceState* s = h->lap;
  const int nd = s->re_ptr.empty() ? h->n : s->n_data;
  const char* name = gpb::lik_name(s->link);
  if (gpb::lik_real_only(s->link)) return fail("%s: the response is real-valued (call gpb_hip_vecchia_laplace_set_response_real)", name);
  for (int i = 0; i < nd; ++i) {
    if (gpb::lik_resp(s->link) == gpb::Resp::kCount) {      // likelihoods.h:1338-1350
      if (y01[i] < 0) return fail("%s: the response must be >= 0 (found %d at Vecchia position %d)", name, y01[i], i);
    } else if (y01[i] != 0 && y01[i] != 1)
      return fail("bernoulli_logit / bernoulli_probit: labels must be 0 or 1 (found %d at Vecchia position %d)", y01[i], i);   // likelihoods.h:1321-1329
  }
  s->log_norm_const = 0.;
  s->real_resp = false;
  s->norm_dirty = true;                  // the constants (with the sample weights, if any) are summed at the next evaluation: laplace_norm_consts
  s->labels.assign(y01, y01 + nd);       // uploaded in the workspace's storage order by the next evaluation
  s->has_y = true; s->y_dirty = true;
  s->grad_state = s->gvec_state = false; // the kept gradient state described the previous response
  API_END();
}

// real-valued response (its domain: Resp of lik_table.h), same order as gpb_hip_vecchia_laplace_set_labels takes its labels
int gpb_hip_vecchia_laplace_set_response_real(gpb_hip_vecchia_t* h, const double* y) {
  API_BEGIN();
  if (!h || !y) return fail("null argument");
  if (!h->lap) h->lap = new LaplaceState();
  LaplaceState* s = h->lap;
  if (!gpb::lik_accepts_real(s->link))
    return fail("gpb_hip_vecchia_laplace_set_response_real: a real-valued response is for gamma, beta, t, lognormal, gaussian_latent and for proportions under the logit / probit links (likelihood id %d)", s->link);
  const int nd = s->re_ptr.empty() ? h->n : s->n_data;
  const char* name = gpb::lik_name(s->link);
  for (int i = 0; i < nd; ++i) {
    switch (gpb::lik_resp(s->link)) {      // likelihoods.h:1365-1373, :1403-1409, :1330-1337
      case gpb::Resp::kPositiveReal: if (!(y[i] > 0.)) return fail("%s: the response must be > 0 (found %g at Vecchia position %d)", name, y[i], i); break;
      case gpb::Resp::kUnitInterval: if (!(y[i] > 0. && y[i] < 1.)) return fail(" Must have 0 < y < 1 for the response variable ('y') for likelihood = '%s', found %g ", name, y[i]); break;
      case gpb::Resp::kFiniteReal: if (!std::isfinite(y[i])) return fail("%s: the response must be finite (found %g at Vecchia position %d)", name, y[i], i); break;
      case gpb::Resp::kBinaryOrProportion: if (!(y[i] >= 0. && y[i] <= 1.)) return fail(" Must have 0 <= y <= 1 for the response variable ('y') (found %g at Vecchia position %d)", y[i], i); break;
      case gpb::Resp::kCount: break;      // refused above
    }
  }
  s->real_resp = true;
  s->norm_dirty = true;
  s->resp_real.assign(y, y + nd);
  s->labels.assign((size_t)nd, 0);
  s->has_y = true; s->y_dirty = true;
  s->grad_state = s->gvec_state = false;
  API_END();
}

// Sample weights of the non-Gaussian likelihood (round 5; Likelihood's weights_, likelihoods.h:666-668: log-likelihood, its derivatives wrt the location
// parameter, the per-datum parts of the normalising constants and of the auxiliary-parameter gradients are multiplied by w_d), in the order
// gpb_hip_vecchia_laplace_set_labels takes its labels; NULL: no weights.  Finite and >= 0.
int gpb_hip_vecchia_laplace_set_weights(gpb_hip_vecchia_t* h, const double* w) {
  API_BEGIN();
  if (!h) return fail("null argument");
  if (!h->lap) h->lap = new LaplaceState();
  LaplaceState* s = h->lap;
  const int nd = s->re_ptr.empty() ? h->n : s->n_data;
  if (!w) { if (!s->weights.empty()) { s->weights.clear(); s->norm_dirty = true; s->grad_state = s->gvec_state = false; } return 0; }
  for (int i = 0; i < nd; ++i) if (!(w[i] >= 0.) || !std::isfinite(w[i])) return fail("sample weights must be finite and >= 0 (found %g at Vecchia position %d)", w[i], i);
  s->weights.assign(w, w + nd);
  s->w_dirty = true; s->norm_dirty = true;
  s->grad_state = s->gvec_state = false;
  API_END();
}

// auxiliary parameters of the likelihood (how many and which: lik_table.h; original scale, > 0): Likelihood::SetAuxPars (likelihoods.h:2622-2760)
int gpb_hip_vecchia_laplace_set_aux_pars(gpb_hip_vecchia_t* h, const double* aux, int32_t num_aux) {
  API_BEGIN();
  if (!h || !aux) return fail("null argument");
  if (!h->lap) h->lap = new LaplaceState();
  LaplaceState* s = h->lap;
  const gpb::LikInfo& lk = gpb::kLik[s->link];
  if (!lk.num_aux) return fail("gpb_hip_vecchia_laplace_set_aux_pars: likelihood id %d has no auxiliary parameters", s->link);
  if (num_aux != lk.num_aux) return fail("gpb_hip_vecchia_laplace_set_aux_pars: %d parameters (gamma / negative_binomial have one, the shape; beta one, the precision; t two: scale, df; lognormal one, the variance of log y)", num_aux);
  if (!(aux[0] > 0.) || !std::isfinite(aux[0])) return fail("The %s parameter is not > 0 (found %g)", lk.aux_label_set, aux[0]);      // likelihoods.h:2649-2656
  if (lk.num_aux == 2 && (!(aux[1] > 0.) || !std::isfinite(aux[1]))) return fail("The %s parameter is not > 0 (found %g)", lk.aux2_label, aux[1]);
  if (aux[0] != s->aux) { s->aux = aux[0]; s->norm_dirty = true; s->grad_state = s->gvec_state = false; }
  if (lk.num_aux == 2 && aux[1] != s->aux2) { s->aux2 = aux[1]; s->norm_dirty = true; s->grad_state = s->gvec_state = false; }
  API_END();
}

int gpb_hip_vecchia_laplace_set_fixed_effects(gpb_hip_vecchia_t* h, const double* fixed_effects) {
  API_BEGIN();
  if (!h) return fail("null argument");
  if (!h->lap) h->lap = new LaplaceState();
  LaplaceState* s = h->lap;
  s->grad_state = s->gvec_state = false; // ... and the previous offset
  if (!fixed_effects) { s->has_fe = false; s->fe.clear(); return 0; }
  s->fe.assign(fixed_effects, fixed_effects + (s->re_ptr.empty() ? h->n : s->n_data));
  s->has_fe = true; s->fe_dirty = true;
  API_END();
}

// Repeated locations for the non-Gaussian models (RECompGP with use_Z_for_duplicates, include/GPBoost/re_comp.h:863-885; Vecchia_utils.cpp:1156-1168):
// the handle's n points are the UNIQUE locations = random effects; re_ptr (n + 1) is the CSR of their data.  Afterwards
// gpb_hip_vecchia_laplace_set_labels / _set_fixed_effects take n_data = re_ptr[n] values grouped by random effect (Vecchia order of the random
// effects), and every likelihood term of a random effect is the sum over its data.  re_ptr = NULL: back to one datum per random effect.
int gpb_hip_vecchia_laplace_set_data_map(gpb_hip_vecchia_t* h, const int32_t* re_ptr) {
  API_BEGIN();
  if (!h) return fail("null argument");
  if (!h->lap) h->lap = new LaplaceState();
  LaplaceState* s = h->lap;
  s->has_y = false; s->has_fe = false; s->fe.clear(); s->grad_state = s->gvec_state = false;     // labels / offsets of another layout
  if (!re_ptr) { s->re_ptr.clear(); s->n_data = 0; s->map_dirty = true; return 0; }
  if (re_ptr[0] != 0) return fail("gpb_hip_vecchia_laplace_set_data_map: re_ptr[0] = %d", re_ptr[0]);
  for (int i = 0; i < h->n; ++i) if (re_ptr[i + 1] <= re_ptr[i]) return fail("gpb_hip_vecchia_laplace_set_data_map: random effect %d has no data", i);
  s->re_ptr.assign(re_ptr, re_ptr + h->n + 1);
  s->n_data = re_ptr[h->n];
  s->map_dirty = true;
  API_END();
}

int gpb_hip_vecchia_laplace_set_likelihood(gpb_hip_vecchia_t* h, int likelihood_id) {
  API_BEGIN();
  if (!h) return fail("null argument");
  if (!gpb::lik_valid(likelihood_id)) {
    std::string ids;      // "0 = bernoulli_logit, 1 = bernoulli_probit, ..."
    for (int i = 0; i < gpb::kNumLik; ++i) ids += (i ? ", " : "") + std::to_string(i) + " = " + gpb::lik_name(i);
    return fail("gpb_hip_vecchia_laplace_set_likelihood: id %d (%s)", likelihood_id, ids.c_str());
  }
  if (!h->lap) h->lap = new LaplaceState();
  if (h->lap->link != likelihood_id) { h->lap->has_y = false; h->lap->grad_state = h->lap->gvec_state = false; }   // labels are validated against the likelihood: set them again
  h->lap->link = likelihood_id;
  API_END();
}

// the binomial likelihoods' normalising constant (on != 0): sum lgamma(w + 1) - lgamma(k + 1) - lgamma(w - k + 1), k = w y, with the proportions set by
// gpb_hip_vecchia_laplace_set_response_real and the trials by gpb_hip_vecchia_laplace_set_weights (likelihoods.h:10612-10622); quasi_bernoulli_*: 0 (:10880-10883)
int gpb_hip_vecchia_laplace_set_binomial(gpb_hip_vecchia_t* h, int on) {
  API_BEGIN();
  if (!h) return fail("null argument");
  if (!h->lap) h->lap = new LaplaceState();
  if (h->lap->binomial != (on != 0)) { h->lap->binomial = on != 0; h->lap->norm_dirty = true; }
  API_END();
}

// cg_preconditioner_type of the iterative methods (GPB_SetOptimConfig; SUPPORTED_PRECONDITIONERS_NONGAUSS_VECCHIA_, re_model_template.h:5906):
// type 0 = "vadu", 1 = "pivoted_cholesky" with `rank` columns (fitc_piv_chol_preconditioner_rank_; <= 0: the reference's default 50, :5922), 2 = "fitc" with `rank`
// inducing points, 3 = "vecchia_response" (rank unused; evaluation only -- the reference refuses the gradient with it, likelihoods.h:6570-6572).
int gpb_hip_vecchia_laplace_set_preconditioner(gpb_hip_vecchia_t* h, int type, int rank) {
  if (!h) return fail("null argument");
  if (type < kPcVadu || type > kPcNone) return fail("preconditioner type %d is not on this path (0 = vadu, 1 = pivoted_cholesky, 2 = fitc, 3 = vecchia_response; full-scale Vecchia: 2 = fitc, 4 = vifdu, 5 = none)", type);
  if (pc_vif_only(type) && h->vif_k < 1) return fail("the 'vifdu' / 'none' preconditioners belong to gp_approx = 'full_scale_vecchia'");
  if (!h->lap) h->lap = new LaplaceState();
  LaplaceState* s = h->lap;
  const int rk = rank > 0 ? rank : (type == kPcFitc ? 200 : 50);            // default_fitc_preconditioner_rank_ / default_piv_chol_preconditioner_rank_ (re_model_template.h:5921-5922)
  if (type == kPcPivChol && rk > h->n) return fail("'fitc_piv_chol_preconditioner_rank' cannot be larger than the dimension of the mode (= number of unique locations) ");   // likelihoods.h:936-938
  if (type == kPcPivChol && rk > gpb::pc_max_rank)
    return fail("pivoted_cholesky preconditioner: at most %d columns on this path (the k x 4 operand of a probe chunk is kept in 64 KB of LDS; got fitc_piv_chol_preconditioner_rank = %d)", gpb::pc_max_rank, rk);
  if (s->pc_type != type || s->pc_rank != rk) { s->grad_state = false; s->gvec_state = false; }
  if (s->pc_type != type) {
    // "fitc" and "pivoted_cholesky" share d_pcL / d_pcM / d_pcG but each owns further work arrays: with the same rank k a handle that ran one of them would
    // pass the other's `pc_k != k || !d_pcL` test with ITS arrays still null (ADVICE r05) -- a change of type drops every buffer, the next factorisation re-allocates
    HIP_OK(hipSetDevice(h->device));
    dev_free(s->d_pcL); dev_free(s->d_pcM); dev_free(s->d_pcG); dev_free(s->d_pcdiag); dev_free(s->d_pcpi); dev_free(s->d_pcpos); dev_free(s->d_pcdone);
    dev_free(s->d_pcV); dev_free(s->d_pcvn2); dev_free(s->d_pcwp); dev_free(s->d_pcdL); dev_free(s->d_pcI);
    s->pc_k = 0; s->pc_cols = 0;
  }
  s->pc_type = type; s->pc_rank = rk;
  return 0;
}
// The inducing points of the "fitc" preconditioner: k x d, column-major (the reference draws them by kmeans++ from the model's generator at the first covariance
// factor, Calc_FITC_Preconditioner_Vecchia, re_model_template.h:9502-9593 -- libstdc++'s discrete_distribution: the host's part).  k < n.
int gpb_hip_vecchia_laplace_set_inducing_points(gpb_hip_vecchia_t* h, int32_t k, const double* ip_colmajor) {
  if (!h || !ip_colmajor) return fail("null argument");
  if (k < 1 || k >= h->n) return fail("Need to have less inducing points (currently fitc_piv_chol_preconditioner_rank = %d) than data points (%d) for cg_preconditioner_type = 'fitc' ", k, h->n);   // :9512-9515
  if (h->d > 3) return fail("fitc preconditioner: coordinate dimensions 1..3 (this model has %d)", h->d);
  if (k > 256) return fail("fitc preconditioner: at most 256 inducing points on this path (the cross-covariance kernels of vif_kernels.hip; got %d)", k);
  if (!h->lap) h->lap = new LaplaceState();
  LaplaceState* s = h->lap;
  HIP_OK(hipSetDevice(h->device));
  s->pc_ip.assign((size_t)k * 3, 0.0);
  for (int j = 0; j < k; ++j) for (int c = 0; c < h->d; ++c) s->pc_ip[(size_t)j * 3 + c] = ip_colmajor[(size_t)c * k + j];
  dev_free(s->d_pcip);
  HIP_OK(hipMalloc(&s->d_pcip, sizeof(double) * (size_t)k * 3));
  HIP_OK(hipMemcpy(s->d_pcip, s->pc_ip.data(), sizeof(double) * (size_t)k * 3, hipMemcpyHostToDevice));
  s->pc_nip = k;
  s->grad_state = false; s->gvec_state = false;
  return 0;
}

}  // extern "C"

// Test entry (include/gpb_hip.h): one of the block operations of the low-rank preconditioners on host data, sized and called as pc_refresh / pc_apply do it.
// Every input lies between two runs of NaN on the device and the scratch starts as NaN: a value read from beyond an operand, or a partial sum that was never written,
// shows in the result.  `out` travels to the device whole (guard + result + guard doubles) and comes back whole.
int gpb_hip_lowrank_ops_check(int32_t op, int32_t n, int32_t k, int32_t ncol, int32_t nc, int32_t mode, const double* L, const double* W, const double* M, const double* X,
                              const double* x2, int32_t in_place, int32_t guard, double* out) {
  API_BEGIN();
  if (check_device()) return -1;
  if (op < 0 || op > 2 || n < 1 || k < 1 || k > gpb::pc_max_rank || ncol < 1 || (nc != 1 && nc != 4) || mode < 0 || mode > 4 || guard < 0 || !L || !W || !out)
    return fail("gpb_hip_lowrank_ops_check: invalid argument (op 0..2, n, k (<= %d), ncol >= 1, nc 1 or 4, mode 0..4)", gpb::pc_max_rank);
  if ((op == 1 && (!M || !X)) || (op == 2 && (!x2 || (!X && !in_place)))) return fail("gpb_hip_lowrank_ops_check: null operand");
  constexpr size_t PAD = 64;
  std::vector<double*> bufs;
  const auto free_tmp = scope_exit([&] { for (double* b : bufs) (void)hipFree(b); });
  std::vector<double> stage;
  const auto upload = [&](const double* src, size_t cnt, double** dev) -> hipError_t {      // NaN | src | NaN
    stage.assign(cnt + 2 * PAD, std::nan(""));
    std::memcpy(stage.data() + PAD, src, sizeof(double) * cnt);
    double* d = nullptr;
    hipError_t e = hipMalloc(&d, sizeof(double) * stage.size());
    if (e != hipSuccess) return e;
    bufs.push_back(d);
    *dev = d + PAD;
    return hipMemcpy(d, stage.data(), sizeof(double) * stage.size(), hipMemcpyHostToDevice);
  };
  const int parts = gpb::pc_parts(n);
  const size_t nblk = (size_t)ncol * n * nc, nx2 = (size_t)ncol * k * nc, npairs = (size_t)k * (k + 1) / 2;
  const size_t nout = op == 0 ? npairs : (op == 1 ? nx2 : nblk);
  const size_t npart = std::max((size_t)ncol * parts * k * nc, (size_t)parts * npairs);      // (pc_apply)
  double *d_L = nullptr, *d_W = nullptr, *d_M = nullptr, *d_X = nullptr, *d_x2 = nullptr, *d_part = nullptr, *d_out = nullptr;
  HIP_OK(upload(L, (size_t)n * k, &d_L));
  HIP_OK(upload(W, (size_t)n, &d_W));
  if (op == 1) HIP_OK(upload(M, (size_t)k * k, &d_M));
  if (op == 1 || (op == 2 && !in_place)) HIP_OK(upload(X, nblk, &d_X));
  if (op == 2) HIP_OK(upload(x2, nx2, &d_x2));
  HIP_OK(hipMalloc(&d_out, sizeof(double) * (nout + 2 * (size_t)guard)));
  bufs.push_back(d_out);
  HIP_OK(hipMemcpy(d_out, out, sizeof(double) * (nout + 2 * (size_t)guard), hipMemcpyHostToDevice));
  if (op != 2) {
    stage.assign(npart, std::nan(""));
    HIP_OK(hipMalloc(&d_part, sizeof(double) * npart));
    bufs.push_back(d_part);
    HIP_OK(hipMemcpy(d_part, stage.data(), sizeof(double) * npart, hipMemcpyHostToDevice));
  }
  double* res = d_out + guard;
  if (op == 0) HIP_OK(gpb::pc_gram(d_L, d_W, n, k, d_part, res, nullptr));
  else if (op == 1) HIP_OK(gpb::pc_ltwx(d_L, d_W, d_M, d_X, n, k, ncol, nc, d_part, res, nullptr));
  else HIP_OK(gpb::pc_combine(d_L, d_W, in_place ? res : d_X, d_x2, n, k, ncol, nc, mode, res, nullptr));
  HIP_OK(hipDeviceSynchronize());
  HIP_OK(hipMemcpy(out, d_out, sizeof(double) * (nout + 2 * (size_t)guard), hipMemcpyDeviceToHost));
  API_END();
}

// Test entry (include/gpb_hip.h): one launcher of the sparse Vecchia-Laplace machinery on the caller's A / D / W, with the handle's schedules (build_levels) and a chosen
// solver form.  Entry records, dense inverses, vectors, scratch and the error word are this call's own; the operands travel in Vecchia order as plain columns and are
// scattered here into storage order and the [chunk][row][nc] layout.  The output and every scratch vector start as `prefill`.
int gpb_hip_vecchia_laplace_ops_check(gpb_hip_vecchia_t* h, int32_t op, int32_t form, int32_t ncol, int32_t nc, int32_t prefill, const double* A, const double* D,
                                      const double* W, const double* scale, const double* A2, const double* X, double* out, double* out2, int32_t* info) {
  API_BEGIN();
  if (!h || !A || !X || !out || !info) return fail("gpb_hip_vecchia_laplace_ops_check: null argument");
  if (op < 0 || op > 6 || (form != 0 && form != 1 && form != 4) || ncol < 1 || (nc != 1 && nc != 4) || prefill < 0 || prefill > 3)
    return fail("gpb_hip_vecchia_laplace_ops_check: invalid argument (op 0..6, form 0 / 1 / 4, ncol >= 1, nc 1 or 4, prefill 0..3)");
  if ((op == 2 && (!D || !W)) || ((op == 3 || op == 4) && !scale) || (op >= 5 && !A2) || ((op == 2 || op == 3) && !out2))
    return fail("gpb_hip_vecchia_laplace_ops_check: null operand");
  HIP_OK(hipSetDevice(h->device));
  if (!h->has_nn) return fail("gpb_hip_vecchia_laplace_ops_check: the handle has no neighbour table");
  if (!h->lap) h->lap = new LaplaceState();
  LaplaceState* s = h->lap;
  if (!h->has_transpose && build_transpose(h)) return -1;
  if (!h->has_levels && build_levels(h, s)) return -1;
  const int n = h->n, m = h->m;
  hipStream_t st = h->stream;
  const size_t nblk = (size_t)ncol * nc * n;
  static const unsigned long long kFill[4] = { 0ull, 0x7FF8000000000000ull, 0x7FF0000000000000ull, gpb::kLapEmpty };
  double fillv;
  std::memcpy(&fillv, &kFill[prefill], sizeof(double));
  std::vector<double> stage;
  const auto filled = [&](DevBuf<double>& b, size_t cnt) -> hipError_t {
    stage.assign(cnt, fillv);
    hipError_t e = b.alloc(cnt);
    return e != hipSuccess ? e : hipMemcpy(b, stage.data(), sizeof(double) * cnt, hipMemcpyHostToDevice);
  };
  const auto per_row = [&](DevBuf<double>& b, const double* src) -> hipError_t {      // Vecchia order -> storage order
    stage.resize(n);
    for (int i = 0; i < n; ++i) stage[s->sigma[i]] = src[i];
    hipError_t e = b.alloc(n);
    return e != hipSuccess ? e : hipMemcpy(b, stage.data(), sizeof(double) * n, hipMemcpyHostToDevice);
  };
  DevBuf<double> dA, dA2, dD, dW, dS, dX, dOut, dOut2, dinv[2], dtbuf[2];
  DevBuf<gpb::LapEnt> hent[2], oent[2], hent_g[2], oent_g[2];
  DevBuf<int> derr;
  HIP_OK(dA.alloc((size_t)n * m));
  HIP_OK(hipMemcpy(dA, A, sizeof(double) * (size_t)n * m, hipMemcpyHostToDevice));
  if (D) HIP_OK(per_row(dD, D));
  if (W) HIP_OK(per_row(dW, W));
  if (scale) HIP_OK(per_row(dS, scale));
  stage.resize(nblk);
  for (int c = 0; c < ncol * nc; ++c) {
    double* dst = stage.data() + (size_t)(c / nc) * n * nc + (size_t)(c % nc);
    for (int i = 0; i < n; ++i) dst[(size_t)s->sigma[i] * nc] = X[(size_t)c * n + i];
  }
  HIP_OK(dX.alloc(nblk));
  HIP_OK(hipMemcpy(dX, stage.data(), sizeof(double) * nblk, hipMemcpyHostToDevice));
  HIP_OK(filled(dOut, nblk));
  if (op == 2 || op == 3) HIP_OK(filled(dOut2, nblk));
  HIP_OK(derr.alloc(1));
  HIP_OK(hipMemset(derr, 0, sizeof(int)));
  gpb::LapLevels lv = make_levels(h, s);
  lv.A = dA; lv.syncfree = form; lv.err = derr;
  LaplaceState::Tri* tris[2] = { &s->fwd, &s->bwd };
  gpb::LapTri* lts[2] = { &lv.fwd, &lv.bwd };
  gpb::LapDense* lds[2] = { &lv.fdense, &lv.bdense };
  for (int q = 0; q < 2; ++q) {
    const LaplaceState::Tri* tr = tris[q];
    const size_t nh = (size_t)tr->nslots * 32, no = std::max<size_t>(tr->novf, 1);
    HIP_OK(hent[q].alloc(nh)); HIP_OK(oent[q].alloc(no));
    const bool dense = tr->dK > 0 && (op == 3 || op == 4);
    if (dense) {
      HIP_OK(filled(dinv[q], (size_t)tr->dK * tr->dK));
      HIP_OK(filled(dtbuf[q], (size_t)tr->dK * gpb::kDenseCols * (1 + gpb::kDenseSplit)));
      lds[q]->inv = dinv[q]; lds[q]->tbuf = dtbuf[q];
    }
    // everything from here on is ordered by the handle's stream (a non-blocking one: the synchronous copies above are not ordered against it by themselves)
    HIP_OK(hipDeviceSynchronize());
    HIP_OK(hipMemcpyAsync(hent[q], tr->hent, sizeof(gpb::LapEnt) * nh, hipMemcpyDeviceToDevice, st));      // the sources; the coefficients are refreshed below
    HIP_OK(hipMemcpyAsync(oent[q], tr->oent, sizeof(gpb::LapEnt) * no, hipMemcpyDeviceToDevice, st));
    HIP_OK(gpb::lap_permute_factor(dA, tr->hpos, tr->opos, nh, tr->novf, hent[q], oent[q], st));
    lts[q]->hent = hent[q]; lts[q]->oent = oent[q];
    if (dense) HIP_OK(gpb::lap_dense_build(*lds[q], dA, st));
  }
  gpb::LapTri tg = op == 6 ? lv.bwd : lv.fwd;
  if (op >= 5) {      // the same layout with a second coefficient array, as the gradient holds dA / d log(range)
    const int q = op - 5;
    const LaplaceState::Tri* tr = tris[q];
    const size_t nh = (size_t)tr->nslots * 32, no = std::max<size_t>(tr->novf, 1);
    HIP_OK(dA2.alloc((size_t)n * m));
    HIP_OK(hipMemcpy(dA2, A2, sizeof(double) * (size_t)n * m, hipMemcpyHostToDevice));
    HIP_OK(hipDeviceSynchronize());
    HIP_OK(hent_g[q].alloc(nh)); HIP_OK(oent_g[q].alloc(no));
    HIP_OK(hipMemcpyAsync(hent_g[q], hent[q], sizeof(gpb::LapEnt) * nh, hipMemcpyDeviceToDevice, st));
    HIP_OK(hipMemcpyAsync(oent_g[q], oent[q], sizeof(gpb::LapEnt) * no, hipMemcpyDeviceToDevice, st));
    HIP_OK(gpb::lap_permute_factor(dA2, tr->hpos, tr->opos, nh, tr->novf, hent_g[q], oent_g[q], st));
    tg.hent = hent_g[q]; tg.oent = oent_g[q];
  }
  switch (op) {
    case 0: HIP_OK(gpb::lap_B(lv, n, dX, dOut, ncol, nc, st)); break;
    case 1: HIP_OK(gpb::lap_Bt(lv, n, dX, dOut, ncol, nc, st)); break;
    case 2: HIP_OK(gpb::lap_apply(lv, n, dD, dW, dX, dOut, dOut2, ncol, nc, st)); break;
    case 3: HIP_OK(gpb::lap_vadu(lv, n, dS, dX, dOut, dOut2, ncol, nc, st)); break;
    case 4: HIP_OK(gpb::lap_fwd_solve(lv, n, dS, dX, dOut, ncol, nc, st)); break;
    default: HIP_OK(gpb::lap_mul(tg, n, dX, dOut, ncol, nc, st)); break;
  }
  HIP_OK(hipStreamSynchronize(st));
  int err = 0;
  HIP_OK(hipMemcpy(&err, derr, sizeof(int), hipMemcpyDeviceToHost));
  const auto fetch = [&](const DevBuf<double>& b, double* dst) -> hipError_t {      // storage order, [chunk][row][nc] -> plain columns in Vecchia order
    hipError_t e = hipMemcpy(stage.data(), b, sizeof(double) * nblk, hipMemcpyDeviceToHost);
    if (e != hipSuccess) return e;
    for (int c = 0; c < ncol * nc; ++c) {
      const double* src = stage.data() + (size_t)(c / nc) * n * nc + (size_t)(c % nc);
      for (int i = 0; i < n; ++i) dst[(size_t)c * n + i] = src[(size_t)s->sigma[i] * nc];
    }
    return hipSuccess;
  };
  stage.resize(nblk);
  HIP_OK(fetch(dOut, out));
  if (op == 2 || op == 3) HIP_OK(fetch(dOut2, out2));
  std::memset(info, 0, sizeof(int32_t) * 24);
  for (int q = 0; q < 2; ++q) {
    const LaplaceState::Tri* tr = tris[q];
    int nwide = 0, nrun = 0;
    for (const gpb::LapSeg& sg : (q == 0 ? s->fseg : s->bseg)) { if (sg.nsplit > 1) ++nwide; else ++nrun; }
    const int32_t f[9] = { tr->nlev, tr->nslots, (int32_t)tr->novf, tr->dK, nwide, nrun, tr->npad, tr->nmulti, tr->nlong };
    std::memcpy(info + 9 * q, f, sizeof(f));
  }
  info[18] = err; info[19] = gpb::lap_sf_resident(); info[20] = gpb::lap_sfw_resident();
  API_END();
}

// Test entry (include/gpb_hip.h): the likelihood launchers of laplace_kernels.h on the caller's arrays, no handle and no formula of its own.  op 0: lap_newton_setup,
// lap_objective (all rows, then one launch per row with n = 1 and advanced pointers for the first n_each rows), lap_third_deriv, lap_grad_F / lap_grad_F_map and, for a
// likelihood with auxiliary parameters, lap_aux_grad -- the last two with the dW3 the third-derivative launch just wrote, as in production.  op 1: lap_math_probe.
int gpb_hip_laplace_lik_check(int32_t op, int32_t lik, int32_t n, int32_t n_data, const int32_t* re_ptr, const int32_t* y_int, const double* y_real, const double* weights,
                              const double* fixed_effects, const double* mode, const double* D, const double* Bx, const double* dld, const double* sv, double aux, double aux2,
                              int32_t n_each, double* W, double* rhs, double* dw, double* rdw, double* out2, double* ll_each, double* dW3, double* gradF, double* out3) {
  API_BEGIN();
  if (op != 0 && op != 1) return fail("gpb_hip_laplace_lik_check: op = %d (0: the likelihood launchers, 1: the math probe)", op);
  if (n < 1 || n > (1 << 24) || !mode || !W) return fail("gpb_hip_laplace_lik_check: n = %d (1 .. 2^24), mode and W are needed", n);
  if (check_device()) return -1;
  const auto up = [](auto& buf, const auto* src, size_t cnt) -> hipError_t {
    hipError_t e = buf.alloc(cnt);
    return e != hipSuccess ? e : hipMemcpy(buf, src, sizeof(*src) * cnt, hipMemcpyHostToDevice);
  };
  const auto nan_filled = [](DevBuf<double>& buf, size_t cnt) -> hipError_t {
    const std::vector<double> v(cnt, std::nan(""));
    hipError_t e = buf.alloc(cnt);
    return e != hipSuccess ? e : hipMemcpy(buf, v.data(), sizeof(double) * cnt, hipMemcpyHostToDevice);
  };
  const auto down = [](double* dst, const DevBuf<double>& buf, size_t cnt) -> hipError_t { return hipMemcpy(dst, buf, sizeof(double) * cnt, hipMemcpyDeviceToHost); };
  DevBuf<double> d_mode, d_W;
  HIP_OK(up(d_mode, mode, n));
  HIP_OK(nan_filled(d_W, n));
  if (op == 1) {
    HIP_OK(gpb::lap_math_probe(lik, d_mode, n, d_W, nullptr));
    HIP_OK(hipDeviceSynchronize());
    HIP_OK(down(W, d_W, n));
    return 0;
  }
  if (!gpb::lik_valid(lik)) return fail("gpb_hip_laplace_lik_check: likelihood id %d", lik);
  if (!D || !dld || !sv || !rhs || !dw || !rdw || !out2 || !ll_each || !dW3 || !gradF || !out3) return fail("gpb_hip_laplace_lik_check: null argument");
  if ((y_int != nullptr) == (y_real != nullptr)) return fail("gpb_hip_laplace_lik_check: exactly one of the int and the real response");
  if (y_real ? !gpb::lik_accepts_real(lik) : gpb::lik_real_only(lik)) return fail("gpb_hip_laplace_lik_check: %s does not take this kind of response", gpb::lik_name(lik));
  if (n_each < 0 || n_each > n) return fail("gpb_hip_laplace_lik_check: n_each = %d (0 .. n)", n_each);
  if (re_ptr) {
    bool ok = re_ptr[0] == 0 && re_ptr[n] == n_data;
    for (int i = 0; ok && i < n; ++i) ok = re_ptr[i] <= re_ptr[i + 1];
    if (!ok) return fail("gpb_hip_laplace_lik_check: re_ptr must rise from 0 to n_data");
  } else if (n_data != n) return fail("gpb_hip_laplace_lik_check: n_data = %d without re_ptr (n = %d)", n_data, n);
  if (n_data < 1 || n_data > (1 << 24)) return fail("gpb_hip_laplace_lik_check: n_data = %d", n_data);
  DevBuf<double> d_D, d_Bx, d_dld, d_sv, d_yr, d_w, d_fe, d_rhs, d_dw, d_rdw, d_out2, d_each, d_dW3, d_gF, d_out3;
  DevBuf<int> d_yi, d_ptr;
  HIP_OK(up(d_D, D, n)); HIP_OK(up(d_dld, dld, n)); HIP_OK(up(d_sv, sv, n));
  if (Bx) HIP_OK(up(d_Bx, Bx, n));
  if (re_ptr) HIP_OK(up(d_ptr, re_ptr, (size_t)n + 1));
  if (y_int) HIP_OK(up(d_yi, y_int, n_data)); else HIP_OK(up(d_yr, y_real, n_data));
  if (weights) HIP_OK(up(d_w, weights, n_data));
  if (fixed_effects) HIP_OK(up(d_fe, fixed_effects, n_data));
  HIP_OK(nan_filled(d_rhs, n)); HIP_OK(nan_filled(d_dw, n)); HIP_OK(nan_filled(d_rdw, n)); HIP_OK(nan_filled(d_dW3, n));
  HIP_OK(nan_filled(d_out2, 2)); HIP_OK(nan_filled(d_each, 2 * (size_t)std::max(n_each, 1))); HIP_OK(nan_filled(d_gF, n_data)); HIP_OK(nan_filled(d_out3, 3));
  const gpb::LikResp y{ d_yi, d_yr, aux, d_w, aux2 };
  hipStream_t st = nullptr;
  HIP_OK(gpb::lap_newton_setup(lik, d_mode, y, d_fe, d_D, n, d_W, d_rhs, d_dw, d_rdw, st, d_ptr));
  HIP_OK(gpb::lap_objective(lik, d_mode, y, d_fe, d_Bx, d_D, n, d_out2, st, d_ptr));
  for (int i = 0; i < n_each; ++i) {
    if (re_ptr) HIP_OK(gpb::lap_objective(lik, d_mode.p + i, y, d_fe, nullptr, d_D.p + i, 1, d_each.p + 2 * i, st, d_ptr.p + i));      // re_ptr holds absolute positions: the data stay where they are
    else {
      const gpb::LikResp yi{ d_yi ? d_yi.p + i : nullptr, d_yr ? d_yr.p + i : nullptr, aux, d_w ? d_w.p + i : nullptr, aux2 };
      HIP_OK(gpb::lap_objective(lik, d_mode.p + i, yi, d_fe ? d_fe.p + i : nullptr, nullptr, d_D.p + i, 1, d_each.p + 2 * i, st, nullptr));
    }
  }
  HIP_OK(gpb::lap_third_deriv(lik, d_mode, y, d_fe, n, d_dW3, st, d_ptr));
  if (re_ptr) HIP_OK(gpb::lap_grad_F_map(lik, d_mode, y, d_fe, d_dld, d_dW3, d_sv, n, d_ptr, d_gF, st));
  else HIP_OK(gpb::lap_grad_F(lik, d_mode, y, d_fe, d_dld, d_sv, n, d_gF, st));
  if (gpb::lik_has_aux(lik)) HIP_OK(gpb::lap_aux_grad(lik, d_mode, y, d_fe, d_dld, d_dW3, d_sv, n, d_ptr, d_out3, st));
  HIP_OK(hipDeviceSynchronize());
  HIP_OK(down(W, d_W, n)); HIP_OK(down(rhs, d_rhs, n)); HIP_OK(down(dw, d_dw, n)); HIP_OK(down(rdw, d_rdw, n)); HIP_OK(down(dW3, d_dW3, n));
  HIP_OK(down(out2, d_out2, 2)); HIP_OK(down(gradF, d_gF, n_data)); HIP_OK(down(out3, d_out3, 3));
  if (n_each > 0) {
    std::vector<double> each(2 * (size_t)n_each);
    HIP_OK(down(each.data(), d_each, each.size()));
    for (int i = 0; i < n_each; ++i) ll_each[i] = each[2 * (size_t)i];
  }
  API_END();
}

namespace {
enum : int { LAP_RESET_MODE = 1, LAP_KEEP_GRAD_STATE = 2 };

// ---- preconditioner "pivoted_cholesky" (pivchol_kernels.hip) ------------------------------------------------------------------
// L_k of the covariance matrix at THIS evaluation's parameters (re_model_template.h:9317-9322: before every mode finding): per column one argmax launch, one
// read of {pivot, error bound} by the host (the loop condition of CG_utils.h:456, PIV_CHOL_STOP_TOL = 1e-6, utils.h:44), one update launch.
// "fitc": C = cross-covariance with the inducing points, Sigma_m (jittered diagonal, JITTER_MULT_IP_FITC_FSA = 1 + 1e-6), V = C L_m^-T and ||V_i||^2 at this evaluation's
// parameters (Calc_FITC_Preconditioner_Vecchia, re_model_template.h:9577-9591): the n x k parts with the cross-covariance / product kernels of the full-scale
// approximation (vif_kernels.hip), the k x k part on the host.
namespace sm = gpb_sm;
// Sigma_m of k inducing points (k x 3 row-major) with the jittered diagonal, the inverse of its lower Cholesky factor L_m (row-major) and log|Sigma_m| -- the k x k host
// part of "fitc" and of the full-scale approximation.  -1: not positive definite
int ip_cov_factor(const std::vector<double>& ip3, int k, int cov_type, double var, double a, std::vector<double>* Sm, std::vector<double>* Li, double* logdet) {
  Sm->resize((size_t)k * k); Li->resize((size_t)k * k);
  sm::ip_cov(ip3.data(), k, 3, sm::IpLayout::RowMajorKx3, sm::MaternForm::LaplacePaths, cov_type, var, a, Sm->data(), nullptr);
  for (int p = 0; p < k; ++p) (*Sm)[(size_t)p * k + p] *= sm::JITTER_MULT_IP_FITC_FSA;
  std::vector<double> Lm(*Sm);
  double ld = 0.0;
  if (!sm::cholesky_lower(Lm.data(), k, k, &ld)) return -1;
  *logdet = 2.0 * ld;
  sm::tri_inverse_lower(Lm.data(), k, k, Li->data());
  return 0;
}
int pc_factor_fitc(gpb_hip_vecchia_t* h, LaplaceState* s, int cov_type, double var, double a, hipStream_t st) {
  const int n = h->n, k = s->pc_nip;
  if (k < 1 || !s->d_pcip) return fail("the fitc preconditioner needs its inducing points (gpb_hip_vecchia_laplace_set_inducing_points)");
  const int kq = gpb::vif_kq(k);
  if (s->pc_k != k || !s->d_pcL || !s->d_pcV) {
    dev_free(s->d_pcL); dev_free(s->d_pcM); dev_free(s->d_pcG); dev_free(s->d_pcV); dev_free(s->d_pcvn2); dev_free(s->d_pcwp); dev_free(s->d_pcdL);
    HIP_OK(hipMalloc(&s->d_pcL, sizeof(double) * (size_t)n * k));
    HIP_OK(hipMalloc(&s->d_pcV, sizeof(double) * (size_t)n * k));
    HIP_OK(hipMalloc(&s->d_pcM, sizeof(double) * (size_t)k * k));
    HIP_OK(hipMalloc(&s->d_pcG, sizeof(double) * (size_t)k * (k + 1) / 2));
    HIP_OK(hipMalloc(&s->d_pcvn2, sizeof(double) * (size_t)n));
    HIP_OK(hipMalloc(&s->d_pcwp, sizeof(double) * (size_t)n));
    s->pc_k = k;
  }
  const bool want_dC = h->vif_k > 0;          // full-scale Vecchia: the gradient differentiates the preconditioner (likelihoods.h:5462-5505)
  const size_t need = (size_t)(want_dC ? 3 : 2) * n * kq + (size_t)kq * kq;
  if (s->pctmp_cap < need) { dev_free(s->d_pctmp); s->pctmp_cap = 0; HIP_OK(hipMalloc(&s->d_pctmp, sizeof(double) * need)); s->pctmp_cap = need; }
  double *Ct = s->d_pctmp, *Vt = Ct + (size_t)n * kq, *Mq = Vt + (size_t)n * kq, *dCt = Mq + (size_t)kq * kq;
  if (want_dC && !s->d_pcdL) HIP_OK(hipMalloc(&s->d_pcdL, sizeof(double) * (size_t)n * k));
  if (ip_cov_factor(s->pc_ip, k, cov_type, var, a, &s->pc_Sm, &s->pc_Linv, &s->pc_logdet_Sm))
    return fail("the covariance matrix of the inducing points of the fitc preconditioner is not positive definite");
  std::vector<double> Mh((size_t)kq * kq, 0.0);              // V = C L_m^-T: M[p][q] = (L_m^-T)[p][q] = (L_m^-1)[q][p]
  for (int p = 0; p < k; ++p) for (int q = 0; q < k; ++q) Mh[(size_t)p * kq + q] = s->pc_Linv[(size_t)q * k + p];
  HIP_OK(hipMemcpyAsync(Mq, Mh.data(), sizeof(double) * Mh.size(), hipMemcpyHostToDevice, st));
  HIP_OK(gpb::launch_vif_crosscov(cov_type, h->d_pts, s->d_pcip, 0, n, k, kq, h->d, var, a, Ct, want_dC ? dCt : nullptr, st));
  HIP_OK(gpb::launch_vif_gemm(Ct, Mq, n, kq, Vt, false, st));
  if (want_dC) HIP_OK(gpb::pc_pack_rows(dCt, kq, s->d_sigma, n, k, s->d_pcdL, nullptr, st));
  HIP_OK(gpb::pc_pack_rows(Ct, kq, s->d_sigma, n, k, s->d_pcL, nullptr, st));
  HIP_OK(gpb::pc_pack_rows(Vt, kq, s->d_sigma, n, k, s->d_pcV, s->d_pcvn2, st));
  HIP_OK(hipStreamSynchronize(st));                          // Mh leaves scope
  s->pc_cols = k;
  return 0;
}
int pc_factor_sigma(gpb_hip_vecchia_t* h, LaplaceState* s, int cov_type, double var, double a, hipStream_t st) {
  if (s->pc_type == kPcFitc) return pc_factor_fitc(h, s, cov_type, var, a, st);
  const int n = h->n, k = std::min(s->pc_rank, n);
  if (h->d > 3) return fail("pivoted_cholesky preconditioner: coordinate dimensions 1..3 (this model has %d)", h->d);
  if (s->pc_k != k || !s->d_pcL || !s->d_pcdiag) {
    dev_free(s->d_pcL); dev_free(s->d_pcM); dev_free(s->d_pcG); dev_free(s->d_pcdiag); dev_free(s->d_pcpi); dev_free(s->d_pcpos); dev_free(s->d_pcdone);
    HIP_OK(hipMalloc(&s->d_pcL, sizeof(double) * (size_t)n * k));
    HIP_OK(hipMalloc(&s->d_pcM, sizeof(double) * (size_t)k * k));
    HIP_OK(hipMalloc(&s->d_pcG, sizeof(double) * (size_t)k * (k + 1) / 2));
    HIP_OK(hipMalloc(&s->d_pcdiag, sizeof(double) * (size_t)n));
    HIP_OK(hipMalloc(&s->d_pcpi, sizeof(int) * (size_t)n));
    HIP_OK(hipMalloc(&s->d_pcpos, sizeof(int) * (size_t)n));
    HIP_OK(hipMalloc(&s->d_pcdone, sizeof(int) * (size_t)n));
    s->pc_k = k;
  }
  HIP_OK(gpb::pc_piv_init(n, k, var, s->d_pcL, s->d_pcdiag, s->d_pcpi, s->d_pcpos, s->d_pcdone, st));
  int mcol = 0;
  for (;;) {
    HIP_OK(gpb::pc_piv_argmax(n, mcol, s->d_pcdiag, s->d_pcpi, s->d_pcpos, s->d_o + 6, st));
    HIP_OK(hipMemcpyAsync(s->h_o + 6, s->d_o + 6, sizeof(double) * 2, hipMemcpyDeviceToHost, st));
    HIP_OK(hipStreamSynchronize(st));
    const double err = s->h_o[7];
    if (!(mcol == 0 || (mcol < k && err > 1e-6))) break;
    HIP_OK(gpb::pc_piv_update(h->d_pts, s->d_sigma, n, k, mcol, (int)s->h_o[6], cov_type, h->d == 3 ? 1 : 0, var, a, s->d_pcL, s->d_pcdiag, s->d_pcdone, st));
    ++mcol;
    if (mcol >= n) break;
  }
  s->pc_cols = mcol;
  return 0;
}
// one launch of the point kernel in factor mode -- the response slot of pts is not used on these paths (u is discarded)
int lap_launch_factor(gpb_hip_vecchia_t* h, int cov_type, double var, double a, int gauss) {
  const bool had_y = h->has_y;
  h->has_y = true;
  const int rc = vecchia_launch(h, gpb::MODE_FACTOR, cov_type, var, a, gauss, nullptr, 0);
  h->has_y = had_y;
  return rc;
}
// M = (I_k + L_k^T W L_k)^-1 and its log-determinant for this W (likelihoods.h:16291-16295, :16413-16418): the Gram matrix is reduced on the device, the k x k
// factorisation runs on the host (Cholesky, then the inverse by k pairs of triangular solves).  *bad = 1: not positive definite / not finite.
gpb::LapLevels make_levels_vr(const gpb_hip_vecchia_t* h, const LaplaceState* s) {      // the level schedules of B with the entries of A_p
  gpb::LapLevels lv = make_levels(h, s);
  lv.fwd.hent = s->vr_hent[0]; lv.fwd.oent = s->vr_oent[0]; lv.bwd.hent = s->vr_hent[1]; lv.bwd.oent = s->vr_oent[1];
  lv.fdense.inv = s->d_vrinv; lv.A = s->d_vrA;
  return lv;
}
// "vecchia_response": (B_p, D_p) of W^-1 + Sigma for this W -- one MODE_FACTOR launch of the point kernel (the hot kernel of the Gaussian path, with per-point diagonal
// additions as for sample weights) into the preconditioner's own buffers, then the level-ordered copies of A_p.  pc_logdet = log|P| = sum log D_p (likelihoods.h:16471-16473).
// with_solve: also the inverse of the forward solve's dense block for A_p -- only the probe vectors of the log-determinant solve with B_p (~300 small launches at config 4's size)
int pc_refresh_vr(gpb_hip_vecchia_t* h, LaplaceState* s, const double* W, hipStream_t st, int* bad, bool with_solve) {
  const int n = h->n, m = h->m;
  *bad = 0;
  if (!s->d_vrA) {
    HIP_OK(hipMalloc(&s->d_vrA, sizeof(double) * (size_t)n * m));
    HIP_OK(hipMalloc(&s->d_vrD, sizeof(double) * (size_t)n * 3));
    HIP_OK(hipMalloc(&s->d_vrDs, sizeof(double) * (size_t)n * 2));
    int q = 0;
    for (LaplaceState::Tri* tr : { &s->fwd, &s->bwd }) {
      HIP_OK(hipMalloc(&s->vr_hent[q], sizeof(gpb::LapEnt) * (size_t)tr->nslots * 32));
      HIP_OK(hipMalloc(&s->vr_oent[q], sizeof(gpb::LapEnt) * std::max<size_t>(tr->novf, 1)));
      HIP_OK(hipMemcpy(s->vr_hent[q], tr->hent, sizeof(gpb::LapEnt) * (size_t)tr->nslots * 32, hipMemcpyDeviceToDevice));      // the source rows (and the padding) are the factor's
      HIP_OK(hipMemcpy(s->vr_oent[q], tr->oent, sizeof(gpb::LapEnt) * std::max<size_t>(tr->novf, 1), hipMemcpyDeviceToDevice));
      ++q;
    }
    if (s->fwd.dK > 0) HIP_OK(hipMalloc(&s->d_vrinv, sizeof(double) * (size_t)s->fwd.dK * s->fwd.dK));
  }
  const double jit = s->vr_var * 1e-10;             // JITTER_MULT_VECCHIA - 1 (Vecchia_utils.cpp:1606-1609)
  double *D2 = s->d_vrD, *u2 = D2 + n, *nug = D2 + 2 * (size_t)n;
  HIP_OK(gpb::pc_vr_nugget(W, s->d_sigma, n, jit, nug, st));
  gpb_hip_vecchia::FactorOverride fo{ s->d_vrA, D2, u2, nug };
  h->factor_override = &fo;
  const int rc = lap_launch_factor(h, s->vr_cov, s->vr_var, s->vr_a, 0);
  h->factor_override = nullptr;
  if (rc) return -1;
  HIP_OK(gpb::pc_vr_diag(D2, s->d_sigma, n, jit, s->d_vrDs, s->d_vrDs + n, st));
  HIP_OK(gpb::lap_logsums(s->d_vrDs, s->d_vrDs, n, s->d_o + 6, st));                    // d_o[6] = sum log(1 / D_p), d_o[7] = sum log D_p
  HIP_OK(hipMemcpyAsync(s->h_o + 6, s->d_o + 6, sizeof(double) * 2, hipMemcpyDeviceToHost, st));
  int q = 0;
  for (LaplaceState::Tri* tr : { &s->fwd, &s->bwd }) {
    HIP_OK(gpb::lap_permute_factor(s->d_vrA, tr->hpos, tr->opos, (size_t)tr->nslots * 32, tr->novf, s->vr_hent[q], s->vr_oent[q], st));
    ++q;
  }
  if (with_solve) HIP_OK(gpb::lap_dense_build(make_levels_vr(h, s).fdense, s->d_vrA, st));
  HIP_OK(hipStreamSynchronize(st));
  h->launches_unfetched = 0;                          // the factor launch's sums are not fetched: the next vecchia_fetch synchronises
  if (!std::isfinite(s->h_o[7])) { *bad = 1; return 0; }                                 // a D_p <= 0 (or a zero / negative W)
  s->pc_logdet = s->h_o[7];
  return 0;
}
int pc_apply_vr(gpb_hip_vecchia_t* h, LaplaceState* s, const double* X, double* out, int ncol, int nc, hipStream_t st) {      // out = B_p' (D_p^-1 (B_p X))  (CG_utils.cpp:300-303)
  const int n = h->n;
  const size_t need = (size_t)n * ncol * nc;
  if (s->vrtmp_cap < need) { dev_free(s->d_vrtmp); s->vrtmp_cap = 0; HIP_OK(hipMalloc(&s->d_vrtmp, sizeof(double) * need)); s->vrtmp_cap = need; }
  const gpb::LapLevels lv2 = make_levels_vr(h, s);
  HIP_OK(gpb::lap_apply(lv2, n, s->d_vrDs, nullptr, X, out, s->d_vrtmp, ncol, nc, st));
  return 0;
}
int pc_refresh(LaplaceState* s, int n, const double* W, hipStream_t st, int* bad) {
  const int k = s->pc_k, npairs = k * (k + 1) / 2, parts = gpb::pc_parts(n);
  *bad = 0;
  const size_t need = (size_t)parts * npairs;
  if (s->pcpart_cap < need) { dev_free(s->d_pcpart); s->pcpart_cap = 0; HIP_OK(hipMalloc(&s->d_pcpart, sizeof(double) * need)); s->pcpart_cap = need; }
  const bool fitc = s->pc_type == kPcFitc;
  double sum_log_wp = 0.0;
  if (fitc) {       // D^-1 for this W (likelihoods.h:16302-16308) and sum log D^-1 (the log|P| of :16465-16470)
    HIP_OK(gpb::pc_fitc_diag(W, s->d_pcvn2, s->pc_Sm[0], n, s->d_pcwp, st));
    HIP_OK(gpb::lap_logsums(s->d_pcwp, s->d_pcwp, n, s->d_o + 6, st));      // d_o[7] = sum log wp
    HIP_OK(hipMemcpyAsync(s->h_o + 6, s->d_o + 6, sizeof(double) * 2, hipMemcpyDeviceToHost, st));
    HIP_OK(hipStreamSynchronize(st));
    sum_log_wp = s->h_o[7];
    if (!std::isfinite(sum_log_wp)) { *bad = 1; return 0; }                 // a non-positive diagonal
  }
  HIP_OK(gpb::pc_gram(s->d_pcL, s->pc_wp(W), n, k, s->d_pcpart, s->d_pcG, st));
  std::vector<double> G(npairs), C((size_t)k * k, 0.0), M((size_t)k * k, 0.0);
  HIP_OK(hipMemcpyAsync(G.data(), s->d_pcG, sizeof(double) * npairs, hipMemcpyDeviceToHost, st));
  HIP_OK(hipStreamSynchronize(st));
  for (int p = 0; p < k; ++p) for (int q = 0; q <= p; ++q) C[(size_t)p * k + q] = G[(size_t)p * (p + 1) / 2 + q] + (fitc ? s->pc_Sm[(size_t)p * k + q] : (p == q ? 1.0 : 0.0));
  double ld = 0.0;
  if (!sm::cholesky_lower(C.data(), k, k, &ld)) { *bad = 1; return 0; }
  s->pc_logdet = fitc ? 2.0 * ld - s->pc_logdet_Sm - sum_log_wp : 2.0 * ld;      // fitc: log|P| itself; pivoted_cholesky: log|I_k + L_k' W L_k| (log|P| = that - log|W|)
  sm::spd_inverse_by_solves(C.data(), k, k, M.data());
  HIP_OK(hipMemcpyAsync(s->d_pcM, M.data(), sizeof(double) * (size_t)k * k, hipMemcpyHostToDevice, st));
  HIP_OK(hipStreamSynchronize(st));
  if (fitc) s->pc_Minv = M;
  return 0;
}
// out = P^-1 X (mode 0) or W^-1 P^-1 X (mode 1) for block vectors of ncol chunks x nc columns (CG_utils.cpp:282-288)
int pc_apply(LaplaceState* s, int n, const double* W, const double* X, double* out, int ncol, int nc, int mode, hipStream_t st) {
  const int k = s->pc_k, parts = gpb::pc_parts(n);
  const size_t need = std::max((size_t)ncol * parts * k * nc, (size_t)parts * k * (k + 1) / 2), need2 = (size_t)ncol * k * nc;
  if (s->pcpart_cap < need) { dev_free(s->d_pcpart); s->pcpart_cap = 0; HIP_OK(hipMalloc(&s->d_pcpart, sizeof(double) * need)); s->pcpart_cap = need; }
  if (s->pcx2_cap < need2) { dev_free(s->d_pcx2); s->pcx2_cap = 0; HIP_OK(hipMalloc(&s->d_pcx2, sizeof(double) * need2)); s->pcx2_cap = need2; }
  const double* wp = s->pc_wp(W);       // the diagonal of the preconditioner's inverse: W (pivoted_cholesky) or D^-1 (fitc)
  HIP_OK(gpb::pc_ltwx(s->d_pcL, wp, s->d_pcM, X, n, k, ncol, nc, s->d_pcpart, s->d_pcx2, st));
  HIP_OK(gpb::pc_combine(s->d_pcL, wp, X, s->d_pcx2, n, k, ncol, nc, mode, out, st));
  return 0;
}

// ---- full-scale Vecchia with a non-Gaussian likelihood: the device half of CalcSigmaComps + CalcCovFactorVecchia + CalcCovFactorFITC_FSA for a LATENT process
// (re_model_template.h:8151-8200, :9646-9672; Vecchia_utils.cpp:1412-1414, :1461-1500, :1599-1609): cross-covariances C, V = C L_m^-T, the residual process's factor
// without a nugget (the neighbours' diagonal x (1 + 1e-10) after the low-rank part is taken off), B C, the Woodbury matrix Sigma_m + (B C)' D^-1 (B C) (k x k: host) ----
int vif_lap_factor(gpb_hip_vecchia_t* h, LaplaceState* s, int cov_type, double var, double a, bool with_grad) {
  const int n = h->n, k = h->vif_k, kq = h->vif_kq;
  const hipStream_t st = h->stream;
  if ((int)h->vif_ip_host.size() != k * 3) return fail("full-scale Vecchia: the inducing points are not on the host");
  std::vector<double>& Sm = s->vif_Sm; std::vector<double>& Li = s->vif_Linv;
  if (ip_cov_factor(h->vif_ip_host, k, cov_type, var, a, &Sm, &Li, &s->vif_logdet_Sm)) return fail("the covariance matrix of the inducing points is not positive definite");
  const size_t nkb = sizeof(double) * (size_t)n * kq;
  if (with_grad && !h->d_vdC) { HIP_OK(hipMalloc(&h->d_vdC, nkb)); HIP_OK(hipMalloc(&h->d_vQdC, nkb)); }
  h->vif_has_grad_inputs = false; h->vif_has_grad_factor = false; s->vif_grad_inputs = false;
  if (vif_resid_factor(h, 0, Li.data(), cov_type, var, a, true, with_grad ? h->d_vdC : nullptr)) return -1;
  HIP_OK(gpb::launch_reduce_partials(h->d_vif_part, n, 3, h->d_vout, nullptr, st, nullptr));
  HIP_OK(gpb::launch_vif_spmm(h->d_A, h->d_nn, 0, n, h->m, kq, h->d_vC, h->d_vQ, with_grad ? h->d_vdC : nullptr, with_grad ? h->d_vQdC : nullptr, st));
  HIP_OK(gpb::launch_vif_gram(h->d_vQ, h->d_D, n, k, kq, h->d_vgpart, h->d_vG, st));
  double o[3];
  std::vector<double> G((size_t)kq * kq);
  HIP_OK(hipMemcpyAsync(o, h->d_vout, sizeof(double) * 3, hipMemcpyDeviceToHost, st));
  HIP_OK(hipMemcpyAsync(G.data(), h->d_vG, sizeof(double) * G.size(), hipMemcpyDeviceToHost, st));
  HIP_OK(hipStreamSynchronize(st));
  if (o[gpb::GPB_P_BAD] > 0.) return fail("The matrix D in the Vecchia approximation contains negative or zero values. This likely results from numerical instabilities ");   // Vecchia_utils.cpp:1688-1697
  std::vector<double>& Cm = s->vif_cholM;
  Cm.assign((size_t)k * k, 0.0);
  s->vif_G.assign((size_t)k * k, 0.0);
  for (int p = 0; p < k; ++p) for (int q = 0; q < k; ++q) s->vif_G[(size_t)p * k + q] = G[(size_t)std::max(p, q) * kq + std::min(p, q)];
  h->vif_has_grad_inputs = with_grad;
  for (int p = 0; p < k; ++p) for (int q = 0; q <= p; ++q) Cm[(size_t)p * k + q] = Sm[(size_t)p * k + q] + G[(size_t)p * kq + q];
  s->vif_M.assign((size_t)k * k, 0.0);
  for (int p = 0; p < k; ++p) for (int q = 0; q <= p; ++q) s->vif_M[(size_t)p * k + q] = s->vif_M[(size_t)q * k + p] = Cm[(size_t)p * k + q];
  double ld = 0.0;
  if (!sm::cholesky_lower(Cm.data(), k, k, &ld)) return fail("the Woodbury matrix of the full-scale Vecchia approximation is not positive definite");
  s->vif_logdet_M = 2.0 * ld;
  h->has_factor = true;
  return 0;
}
// A <- A^-1 for a symmetric positive definite k x k matrix, by solves with its Cholesky factor; *logdet its log-determinant; false: not positive definite
bool spd_invert(std::vector<double>& A, int k, double* logdet) {
  std::vector<double> C(A);
  double ld = 0.0;
  if (!sm::cholesky_lower(C.data(), k, k, &ld)) return false;
  sm::spd_inverse_by_solves(C.data(), k, k, A.data());
  *logdet = 2.0 * ld;
  return true;
}
// the storage-order copies of V and B C, 1 / D, the small multipliers (after build_levels: needs sigma)
int vif_lap_pack(gpb_hip_vecchia_t* h, LaplaceState* s, bool with_grad, hipStream_t st) {
  const int n = h->n, k = h->vif_k, kq = h->vif_kq;
  if (pc_vif_only(s->pc_type) && !with_grad) {       // "vifdu" / "none": C in storage order (the preconditioner, the probes)
    if (!s->d_vifC || s->vif_kk != k) { dev_free(s->d_vifC); HIP_OK(hipMalloc(&s->d_vifC, sizeof(double) * (size_t)n * k)); }
    HIP_OK(gpb::pc_pack_rows(h->d_vC, kq, s->d_sigma, n, k, s->d_vifC, nullptr, st));
  }
  if (with_grad) {
    if (!s->d_vifC || !s->d_vifdC || !s->d_vifBdC || s->vif_kk != k) {      // (d_vifC alone may exist already: "vifdu" / "none", predictions)
      dev_free(s->d_vifC); dev_free(s->d_vifdC); dev_free(s->d_vifBdC);
      HIP_OK(hipMalloc(&s->d_vifC, sizeof(double) * (size_t)n * k)); HIP_OK(hipMalloc(&s->d_vifdC, sizeof(double) * (size_t)n * k)); HIP_OK(hipMalloc(&s->d_vifBdC, sizeof(double) * (size_t)n * k));
    }
    HIP_OK(gpb::pc_pack_rows(h->d_vC, kq, s->d_sigma, n, k, s->d_vifC, nullptr, st));
    HIP_OK(gpb::pc_pack_rows(h->d_vdC, kq, s->d_sigma, n, k, s->d_vifdC, nullptr, st));
    HIP_OK(gpb::pc_pack_rows(h->d_vQdC, kq, s->d_sigma, n, k, s->d_vifBdC, nullptr, st));
    s->vif_grad_inputs = true;
  }
  if (s->vif_kk != k || !s->d_vifV) {
    dev_free(s->d_vifV); dev_free(s->d_vifBC); dev_free(s->d_vifones); dev_free(s->d_vifu); dev_free(s->d_vifI);
    if (s->h_vk) { (void)hipHostFree(s->h_vk); s->h_vk = nullptr; }
    HIP_OK(hipMalloc(&s->d_vifV, sizeof(double) * (size_t)n * k));
    HIP_OK(hipMalloc(&s->d_vifBC, sizeof(double) * (size_t)n * k));
    HIP_OK(hipMalloc(&s->d_vifones, sizeof(double) * (size_t)n * 2));
    HIP_OK(hipMalloc(&s->d_vifu, sizeof(double) * (size_t)n));
    HIP_OK(hipMalloc(&s->d_vifI, sizeof(double) * (size_t)k * k * 2));
    HIP_OK(hipHostMalloc(&s->h_vk, sizeof(double) * (size_t)k * 2));
    std::vector<double> ones((size_t)n, 1.0), I2((size_t)k * k * 2, 0.0);
    for (int q = 0; q < k; ++q) { I2[(size_t)q * k + q] = -1.0; I2[(size_t)k * k + (size_t)q * k + q] = 1.0; }
    HIP_OK(hipMemcpy(s->d_vifones, ones.data(), sizeof(double) * (size_t)n, hipMemcpyHostToDevice));
    HIP_OK(hipMemcpy(s->d_vifI, I2.data(), sizeof(double) * I2.size(), hipMemcpyHostToDevice));
    s->vif_kk = k;
  }
  HIP_OK(gpb::pc_pack_rows(h->d_V, kq, s->d_sigma, n, k, s->d_vifV, nullptr, st));
  HIP_OK(gpb::pc_pack_rows(h->d_vQ, kq, s->d_sigma, n, k, s->d_vifBC, nullptr, st));
  HIP_OK(gpb::pc_rowscale(s->d_vifones, s->d_Ds, n, 1, 1, 1, s->d_vifones + n, st));       // 1 / D
  return 0;
}
int vif_small(LaplaceState* s, int n, int k, int ncol, int nc) {        // scratch of the tall-skinny products
  const int parts = gpb::pc_parts(n);
  const size_t need = std::max((size_t)ncol * parts * k * nc, (size_t)parts * k * (k + 1) / 2), need2 = (size_t)ncol * k * nc;
  if (s->pcpart_cap < need) { dev_free(s->d_pcpart); s->pcpart_cap = 0; HIP_OK(hipMalloc(&s->d_pcpart, sizeof(double) * need)); s->pcpart_cap = need; }
  if (s->vifx2_cap < need2) { dev_free(s->d_vifx2); s->vifx2_cap = 0; HIP_OK(hipMalloc(&s->d_vifx2, sizeof(double) * need2)); s->vifx2_cap = need2; }
  return 0;
}
// out += V (V' X): the predictive-process part of Sigma X (CG_utils.cpp:790-791, :889-890)
int vif_lowrank_add(LaplaceState* s, int n, const double* X, double* out, int ncol, int nc, hipStream_t st) {
  const int k = s->vif_kk;
  if (vif_small(s, n, k, ncol, nc)) return -1;
  HIP_OK(gpb::pc_ltwx(s->d_vifV, s->d_vifones, s->d_vifI, X, n, k, ncol, nc, s->d_pcpart, s->d_vifx2, st));          // x2 = -V' X
  HIP_OK(gpb::pc_combine(s->d_vifV, s->d_vifones, out, s->d_vifx2, n, k, ncol, nc, 1, out, st));                    // out - V x2
  return 0;
}
// slot (0 / 1) of h_vk <- (B C)' D^-1 Bx (asynchronous; Bx = B x in storage order), and, after the stream has been synchronised, x' Q M^-1 Q' x: what the Woodbury
// identity takes off x' B'D^-1B x (likelihoods.h:3430-3433, :3585-3600)
int vif_qf_enqueue(LaplaceState* s, int n, const double* Bx, int slot, hipStream_t st) {
  const int k = s->vif_kk;
  if (vif_small(s, n, k, 1, 1)) return -1;
  HIP_OK(gpb::pc_ltwx(s->d_vifBC, s->d_vifones + n, s->d_vifI + (size_t)k * k, Bx, n, k, 1, 1, s->d_pcpart, s->d_vifx2, st));
  HIP_OK(hipMemcpyAsync(s->h_vk + (size_t)slot * k, s->d_vifx2, sizeof(double) * (size_t)k, hipMemcpyDeviceToHost, st));
  return 0;
}
double vif_qf_value(const LaplaceState* s, int slot) {
  const int k = s->vif_kk;
  std::vector<double> x(s->h_vk + (size_t)slot * k, s->h_vk + (size_t)(slot + 1) * k);
  sm::solve_lower(s->vif_cholM.data(), k, k, x.data());
  double r = 0.0;
  for (int i = 0; i < k; ++i) r += x[i] * x[i];      // |L^-1 y|^2
  return r;
}

// ---- the workspace map: the ONE place that knows how d_vec / d_blk / d_gvec / d_sc are cut up ------------------------------------------------------
// Views for t probe vectors (tc columns with the padding of the last chunk of NCB); a buffer that is not allocated yet leaves its views null.  The order of the
// slots is the order of the lists in lap_work; the sizes the allocations use come from the same struct.
struct LapWork {
  static constexpr int kVec = 16, kBlk = 5, kGvec = 6;      // n-vectors of d_vec, block vectors of d_blk, n-vectors of d_gvec
  static constexpr size_t kParts = 64;                      // partial sums per column and dot product (>= lap_cg_parts(n))
  int NCB = 4, tch = 0, tc = 0;                             // columns per chunk of the layout [chunk][row][NCB], chunks, columns including the padding
  size_t nb = 0, vb = 0;                                    // doubles of a block vector, bytes of an n-vector
  double *mode, *W, *rhs, *dw, *upd, *mnew, *Bm, *dir, *gv, *r, *z, *hh, *v, *t1, *t2, *rdw;      // d_vec (mode finding; W / dw / rdw: the information at the mode afterwards)
  double *R, *Z, *H, *Vb, *T;                               // d_blk (block CG; free after the log-determinant)
  double *mprev, *dW3, *dld, *sv, *SdM, *dDs;               // d_gvec: previous mode, third derivatives, d logdet / d mode, implicit solve, SigmaI_deriv mode, dD (storage order)
  gpb::CgScalars sc1{}, sct{};                              // d_sc: scalars of the single-vector CG; of the block CG (sct.a .. sct.rnorm: 5 tc consecutive doubles, then Td, Ts)
  gpb::CgScalars sct_plain() const { gpb::CgScalars c = sct; c.Td = c.Ts = nullptr; return c; }      // block CG that records no tridiagonal entries
  static size_t vec_bytes(int n) { return sizeof(double) * (size_t)n * kVec; }
  static size_t blk_bytes(int n, int tc) { return sizeof(double) * (size_t)n * tc * kBlk; }
  static size_t gvec_bytes(int n) { return sizeof(double) * (size_t)n * kGvec; }
  static size_t sc_doubles(int tc, int p_max) { return (size_t)5 + (size_t)5 * tc + (size_t)2 * tc * p_max + 3 * kParts * ((size_t)tc + 1); }
};
template <size_t Want, size_t K>
void lap_cut(double* base, size_t step, double** const (&slots)[K]) {      // slot i = base + i step, in the order of the list
  static_assert(K == Want, "the list of slots and the size the buffer is allocated with");
  for (double** f : slots) { *f = base; if (base) base += step; }
}
LapWork lap_work(const gpb_hip_vecchia_t* h, const LaplaceState* s, int t) {
  LapWork w;
  const size_t n = (size_t)h->n;
  w.tch = (t + w.NCB - 1) / w.NCB; w.tc = w.tch * w.NCB;
  w.nb = n * w.tc; w.vb = sizeof(double) * n;
  lap_cut<LapWork::kVec>(s->d_vec, n, { &w.mode, &w.W, &w.rhs, &w.dw, &w.upd, &w.mnew, &w.Bm, &w.dir, &w.gv, &w.r, &w.z, &w.hh, &w.v, &w.t1, &w.t2, &w.rdw });
  lap_cut<LapWork::kBlk>(s->d_blk, w.nb, { &w.R, &w.Z, &w.H, &w.Vb, &w.T });
  lap_cut<LapWork::kGvec>(s->d_gvec, n, { &w.mprev, &w.dW3, &w.dld, &w.sv, &w.SdM, &w.dDs });
  if (double* c1 = s->d_sc) {      // [5] single-vector CG, [5 tc] block CG, [tc p_max] + [tc p_max] Lanczos coefficients, per column 2 P partial sums (r.z, h.v) + P (r.r): one column, then tc
    const size_t tc = (size_t)w.tc, P = LapWork::kParts;
    double *cb = c1 + 5, *Td = cb + 5 * tc, *Ts = Td + tc * s->p_max, *part = Ts + tc * s->p_max, *partb = part + 3 * P;
    w.sc1 = gpb::CgScalars{ c1, c1 + 1, c1 + 2, c1 + 3, c1 + 4, nullptr, nullptr, part, part + 2 * P };
    w.sct = gpb::CgScalars{ cb, cb + tc, cb + 2 * tc, cb + 3 * tc, cb + 4 * tc, Td, Ts, partb, partb + 2 * P * tc };
  }
  return w;
}
// a = 1, b = 0 for every column of the block CG (CG_utils.cpp:141-144)
int lap_cg_reset(const LapWork& w, hipStream_t st) {
  std::vector<double> init((size_t)5 * w.tc, 0.0);
  for (int c = 0; c < w.tc; ++c) init[c] = 1.0;
  HIP_OK(hipMemcpyAsync(w.sct.a, init.data(), sizeof(double) * init.size(), hipMemcpyHostToDevice, st));
  HIP_OK(hipStreamSynchronize(st));
  return 0;
}
int lap_fetch(LaplaceState* s, int count, hipStream_t st) {      // d_o[0..count) -> h_o, one sync
  HIP_OK(hipMemcpyAsync(s->h_o, s->d_o, sizeof(double) * count, hipMemcpyDeviceToHost, st));
  HIP_OK(hipStreamSynchronize(st));
  return 0;
}

// ---- the three forms of the solves with (Sigma^-1 + W) -------------------------------------------------------------------------------------------
//   kVadu             (Sigma^-1 + W) x,   P = B' (D^-1 + W) B                                                  ("vadu"; every predictive variance)
//   kVifSigmaInv      the same with Sigma^-1 = S - Q M^-1 Q' (full-scale Vecchia), P of "vifdu" or the identity ("none")
//   kWinvPlusSigma    (W^-1 + Sigma) x,   P of pivoted_cholesky / fitc / vecchia_response (Sigma with its low-rank part for full-scale Vecchia)
enum class LapForm { kVadu, kVifSigmaInv, kWinvPlusSigma };
LapForm lap_form(const LaplaceState* s) { return s->pc_type == kPcVadu ? LapForm::kVadu : (pc_vif_only(s->pc_type) ? LapForm::kVifSigmaInv : LapForm::kWinvPlusSigma); }
// scratch of the operand's shape: ap for apply, pc for precond, x1 / x2 for the Woodbury parts of either (kVifSigmaInv only)
struct LapScratch { double *ap, *pc, *x1, *x2; };
struct LapSolver {
  gpb_hip_vecchia_t* h; LaplaceState* s; gpb::LapLevels lv; hipStream_t st; int n; LapForm form; bool vif;
  const double *Ds, *W, *rdw, *Dinv;                       // D (storage order), the information, 1 / (W + 1 / D), 1 / D (full-scale Vecchia)
  double *vblkA = nullptr, *vblkB = nullptr, *vwdd = nullptr, *vwgt = nullptr;      // kVifSigmaInv: two block vectors and two n-vectors of d_vifblk

  // out = Sigma x = B^-1 D B^-T x (+ V V' x: CG_utils.cpp:267-268, :790-791)
  int sigma(const double* x, double* out, double* tmp, int ncol, int nc) const {
    HIP_OK(gpb::lap_vadu(lv, n, Ds, x, out, tmp, ncol, nc, st));
    if (vif && vif_lowrank_add(s, n, x, out, ncol, nc, st)) return -1;
    return 0;
  }
  // out += -Q M^-1 Q' x (CG_utils.cpp:561-562)
  int sigI_corr(const double* x, double* out, double* tA, double* tB, int ncol, int nc) const {
    const int vk = h->vif_k;
    HIP_OK(gpb::lap_B(lv, n, x, tA, ncol, nc, st));
    if (vif_small(s, n, vk, ncol, nc)) return -1;
    HIP_OK(gpb::pc_ltwx(s->d_vifBC, Dinv, s->d_vifMinv, tA, n, vk, ncol, nc, s->d_pcpart, s->d_vifx2, st));        // M^-1 (B C)' D^-1 B x
    HIP_OK(gpb::pc_combine(s->d_vifBC, Dinv, tA, s->d_vifx2, n, vk, ncol, nc, 3, tA, st));                           // -D^-1 (B C) (.)
    HIP_OK(gpb::lap_Bt(lv, n, tA, tB, ncol, nc, st));
    HIP_OK(gpb::lap_lincomb(out, out, tB, 1.0, 1.0, n * ncol * nc, st));
    return 0;
  }
  int apply(const double* x, double* out, const LapScratch& t, int ncol, int nc) const {
    switch (form) {
      case LapForm::kVadu:
      case LapForm::kVifSigmaInv:
        HIP_OK(gpb::lap_apply(lv, n, Ds, W, x, out, t.ap, ncol, nc, st));
        return form == LapForm::kVadu ? 0 : sigI_corr(x, out, t.x1, t.x2, ncol, nc);
      case LapForm::kWinvPlusSigma:                                                  // (CG_utils.cpp:412-418)
        if (sigma(x, out, t.ap, ncol, nc)) return -1;
        HIP_OK(gpb::pc_add_div(out, x, W, n, ncol, nc, st));
        return 0;
    }
    return fail("internal: solver form");
  }
  // z = P^-1 r
  int precond(const double* r, double* z, const LapScratch& t, int ncol, int nc) const {
    switch (form) {
      case LapForm::kVadu:
        HIP_OK(gpb::lap_vadu(lv, n, rdw, r, z, t.pc, ncol, nc, st));
        return 0;
      case LapForm::kVifSigmaInv:
        return vif_precond(r, z, t.pc, t.x1, t.x2, ncol, nc);
      case LapForm::kWinvPlusSigma:
        return s->pc_type == kPcVecchiaResponse ? pc_apply_vr(h, s, r, z, ncol, nc, st) : pc_apply(s, n, W, r, z, ncol, nc, 0, st);
    }
    return fail("internal: solver form");
  }
  // "none" the identity; "vifdu" B^-1 [x + (W + D^-1)^-1 D^-1 B C MM^-1 C' B' D^-1 x], x = (W + D^-1)^-1 B^-T rr (CG_utils.cpp:539-543)
  int vif_precond(const double* rr, double* zz, double* tt, double* tA, double* tB, int ncol, int nc) const {
    const int vk = h->vif_k;
    if (s->pc_type == kPcNone) { HIP_OK(hipMemcpyAsync(zz, rr, sizeof(double) * (size_t)n * ncol * nc, hipMemcpyDeviceToDevice, st)); return 0; }
    HIP_OK(gpb::lap_vadu(lv, n, rdw, rr, zz, tt, ncol, nc, st));                                               // tt = B^-T rr, zz = B^-1 x
    HIP_OK(gpb::pc_rowscale(tt, vwdd, n, ncol, nc, 0, tA, st));                                                // D^-1 x
    HIP_OK(gpb::lap_Bt(lv, n, tA, tB, ncol, nc, st));
    if (vif_small(s, n, vk, ncol, nc)) return -1;
    HIP_OK(gpb::pc_ltwx(s->d_vifC, s->d_vifones, s->d_vifMinv + (size_t)vk * vk, tB, n, vk, ncol, nc, s->d_pcpart, s->d_vifx2, st));
    HIP_OK(gpb::pc_combine(s->d_vifC, s->d_vifones, tB, s->d_vifx2, n, vk, ncol, nc, 3, tA, st));              // -C MM^-1 C' B' D^-1 x
    HIP_OK(gpb::lap_B(lv, n, tA, tB, ncol, nc, st));
    HIP_OK(gpb::pc_rowscale(tB, vwdd, n, ncol, nc, 0, tA, st));
    HIP_OK(gpb::lap_fwd_solve(lv, n, s->d_vifones, tA, tB, ncol, nc, st));
    HIP_OK(gpb::lap_lincomb(zz, zz, tB, 1.0, -1.0, n * ncol * nc, st));
    return 0;
  }
  // "vifdu" for this W (likelihoods.h:3488-3500): sigma_woodbury_woodbury = M - (D^-1 B C)' diag((W + D^-1)^-1) (D^-1 B C), its inverse to the device
  int vifdu_refresh(int* pbad) const {
    const int vk = h->vif_k;
    *pbad = 0;
    HIP_OK(gpb::pc_mul3(rdw, Dinv, nullptr, n, vwdd, st));                   // (W + D^-1)^-1 D^-1
    HIP_OK(gpb::pc_mul3(vwdd, Dinv, nullptr, n, vwgt, st));
    if (vif_small(s, n, vk, vk, 1)) return -1;                               // (d_vifx2 takes the packed Gram matrix: k (k + 1) / 2 <= k x k doubles)
    const int npairs = vk * (vk + 1) / 2;
    std::vector<double> G(npairs), MM((size_t)vk * vk);
    HIP_OK(gpb::pc_gram(s->d_vifBC, vwgt, n, vk, s->d_pcpart, s->d_vifx2, st));
    HIP_OK(hipMemcpyAsync(G.data(), s->d_vifx2, sizeof(double) * npairs, hipMemcpyDeviceToHost, st));
    HIP_OK(hipStreamSynchronize(st));
    for (int p = 0; p < vk; ++p) for (int q = 0; q <= p; ++q) MM[(size_t)p * vk + q] = MM[(size_t)q * vk + p] = s->vif_M[(size_t)p * vk + q] - G[(size_t)p * (p + 1) / 2 + q];
    if (!spd_invert(MM, vk, &s->vif_logdet_MM)) { *pbad = 1; return 0; }
    HIP_OK(hipMemcpy(s->d_vifMinv + (size_t)vk * vk, MM.data(), sizeof(double) * (size_t)vk * vk, hipMemcpyHostToDevice));
    return 0;
  }
  // the preconditioner of the (W^-1 + Sigma) form for this W
  int pc_renew(int* pbad, bool for_logdet) const { return s->pc_type == kPcVecchiaResponse ? pc_refresh_vr(h, s, W, st, pbad, for_logdet) : pc_refresh(s, n, W, st, pbad); }
};
LapSolver lap_solver(gpb_hip_vecchia_t* h, LaplaceState* s, const LapWork& w, LapForm form) {
  const int n = h->n;
  const bool vif = h->vif_k > 0;
  LapSolver op{ h, s, make_levels(h, s), h->stream, n, form, vif, s->d_Ds, w.W, w.rdw, vif ? s->d_vifones + n : nullptr };
  if (form == LapForm::kVifSigmaInv) { op.vblkA = s->d_vifblk; op.vblkB = op.vblkA + w.nb; op.vwdd = op.vblkB + w.nb; op.vwgt = op.vwdd + n; }
  return op;
}

// ---- preconditioned CG on a LapSolver from a prepared (X, R, Z, H): Z = P^-1 R, H = Z -------------------------------------------------------------
// Every step: V = A H -> lap_cg_alpha -> lap_cg_update (X += a H, R -= a V; X may be null) -> the residual norms to h_o + 8 -> test -> Z = P^-1 R -> lap_cg_beta.
struct LapCgRule {
  int cap;                  // steps at most
  double tol;
  int ncheck;               // the test looks at the norms of this many leading columns ...
  bool worst;               // ... at their maximum (every column must be below tol), otherwise at their mean
  int beta_pmax;            // last argument of lap_cg_beta: the stride of the recorded tridiagonal entries (1: nothing recorded)
  bool stop_after_beta;     // a met tolerance ends the loop after this step's preconditioner + beta (step j of the tridiagonal matrix is recorded), otherwise before them
};
enum : int { LAP_CG_ERROR = -1, LAP_CG_CONVERGED = 0, LAP_CG_CAP = 1, LAP_CG_NONFINITE = 2 };
// *iters: steps whose update ran (stop_after_beta: whose beta ran).  LAP_CG_ERROR: a HIP call or a solve failed, fail() has the message.
int lap_cg(const LapSolver& op, const LapScratch& scr, double* X, double* R, double* Z, double* H, double* V, int ncol, int nc, const gpb::CgScalars& sc,
           const LapCgRule& rule, int* iters) {
  LaplaceState* s = op.s;
  const int n = op.n;
  hipStream_t st = op.st;
  *iters = 0;
  for (int j = 0; j < rule.cap; ++j) {
    if (op.apply(H, V, scr, ncol, nc)) return LAP_CG_ERROR;
    HIP_OK(gpb::lap_cg_alpha(R, Z, H, V, n, ncol, nc, sc, st));
    HIP_OK(gpb::lap_cg_update(X, R, H, V, n, ncol, nc, sc, st));
    HIP_OK(hipMemcpyAsync(s->h_o + 8, sc.rnorm, sizeof(double) * (size_t)ncol * nc, hipMemcpyDeviceToHost, st));
    HIP_OK(hipStreamSynchronize(st));
    if (!rule.stop_after_beta) *iters = j + 1;
    double norm = 0.0;
    for (int c = 0; c < rule.ncheck; ++c) {
      const double rn = s->h_o[8 + c];
      if (!rule.worst) norm += rn;
      else if (std::isnan(rn) || std::isinf(rn)) return LAP_CG_NONFINITE;
      else norm = std::max(norm, rn);
    }
    if (!rule.worst) norm /= rule.ncheck;
    if (std::isnan(norm) || std::isinf(norm)) return LAP_CG_NONFINITE;
    const bool met = norm < rule.tol;
    if (!rule.stop_after_beta && (met || j + 1 == rule.cap)) return met ? LAP_CG_CONVERGED : LAP_CG_CAP;
    if (op.precond(R, Z, scr, ncol, nc)) return LAP_CG_ERROR;
    HIP_OK(gpb::lap_cg_beta(R, Z, H, n, ncol, nc, sc, j, rule.beta_pmax, st));
    if (rule.stop_after_beta) { *iters = j + 1; if (met) return LAP_CG_CONVERGED; }
  }
  return LAP_CG_CAP;
}

// ---- one evaluation of the approximate marginal likelihood, in stages -------------------------------------------------------------------------------
struct LapEvalArgs {
  int cov_type; double var, a;
  int t, seed, cg_max_num_it, cg_max_num_it_tridiag;
  double cg_delta_conv, delta_conv_mode_finding;
  bool reset_mode, keep;
};
// factor of Sigma^-1 = B^T D^-1 B without nugget (Vecchia_utils.cpp:1599-1609 jitter); full-scale Vecchia: of the residual process, with the low-rank parts
int lap_eval_factor(gpb_hip_vecchia_t* h, LaplaceState* s, const LapEvalArgs& e) {
  hipStream_t st = h->stream;
  if (alloc_factor(h)) return -1;
  if (h->vif_k > 0) {       // gp_approx = "full_scale_vecchia": Sigma = V V' + B^-1 D B^-T (FindModePostRandEffCalcMLLFSVA, likelihoods.h:3379-3750)
    if (s->pc_type != kPcFitc && !pc_vif_only(s->pc_type)) return fail("full-scale Vecchia with a non-Gaussian likelihood: cg_preconditioner_type must be 'fitc' (the reference's default), 'vifdu' or 'none'");
    if (!s->re_ptr.empty()) return fail("full-scale Vecchia with a non-Gaussian likelihood: repeated locations are not on the HIP hot path");
    return vif_lap_factor(h, s, e.cov_type, e.var, e.a, e.keep && s->pc_type == kPcFitc);
  }
  if (pc_vif_only(s->pc_type)) return fail("the 'vifdu' / 'none' preconditioners belong to gp_approx = 'full_scale_vecchia'");
  if (lap_launch_factor(h, e.cov_type, e.var, e.a, 0)) return -1;
  HIP_OK(hipStreamSynchronize(st));
  h->has_factor = true;
  return 0;
}
// log_normalizing_constant_ (part of every LogLikelihood() value, likelihoods.h:11290), per-datum parts weighted, the closed-form parts the reference
// multiplies by num_data_ not (:10750-10757 Poisson; :10998-11007 gamma, exactly 0 at shape 1; :11019-11030 negative_binomial)
int laplace_norm_consts(LaplaceState* s, int nd) {
  const bool hw = !s->weights.empty();
  if (hw && (int)s->weights.size() != nd) return fail("the sample weights were set for %d data, the data map has %d", (int)s->weights.size(), nd);
  const double r = s->aux;
  s->log_norm_const = 0.;
  auto wt = [&](int i) { return hw ? s->weights[i] : 1.0; };
  auto binomial_const = [&]() -> int {      // the binomial likelihoods under either link; plain / quasi Bernoulli: 0
    if (!s->binomial) return 0;
    if (!hw || !s->real_resp) return fail("binomial likelihoods need the proportions (gpb_hip_vecchia_laplace_set_response_real) and the numbers of trials as sample weights");
    for (int i = 0; i < nd; ++i) { const double w = s->weights[i], k = w * s->resp_real[i]; s->log_norm_const += std::lgamma(w + 1.) - std::lgamma(k + 1.) - std::lgamma(w - k + 1.); }
    return 0;
  };
  auto weighted_sum_log_y = [&]() { double sl = 0.; for (int i = 0; i < nd; ++i) sl += wt(i) * std::log(s->resp_real[i]); return sl; };
  const double nu = s->aux2, gauss_const = nd * (0.91893853320467274178 + 0.5 * std::log(r));
  switch (s->link) {
    case gpb::kBernoulliLogit: if (binomial_const()) return -1; break;
    case gpb::kBernoulliProbit: if (binomial_const()) return -1; break;
    case gpb::kPoisson: for (int i = 0; i < nd; ++i) s->log_norm_const -= wt(i) * std::lgamma((double)s->labels[i] + 1.0); break;     // log(y!): O(1) per observation whatever the count
    case gpb::kGamma: s->sum_log_y = weighted_sum_log_y(); s->log_norm_const = (r == 1.0) ? 0.0 : (r - 1.0) * s->sum_log_y + nd * (r * std::log(r) - std::lgamma(r)); break;
    case gpb::kNegativeBinomial: {
      double a1 = 0., slg = 0.;
      for (int i = 0; i < nd; ++i) { a1 += wt(i) * std::lgamma((double)s->labels[i] + r); slg += wt(i) * std::lgamma((double)s->labels[i] + 1.0); }
      s->sum_lgamma_y1 = slg;
      s->log_norm_const = a1 - s->sum_lgamma_y1 + nd * (r * std::log(r) - std::lgamma(r));
    } break;
    case gpb::kBeta: s->log_norm_const = nd * std::lgamma(r); break;                                      // likelihoods.h:10866-10868
    case gpb::kT: s->log_norm_const = nd * (-std::log(r) + std::lgamma((nu + 1.) / 2.) - 0.5 * std::log(nu) - std::lgamma(nu / 2.) - 0.5 * std::log(M_PI)); break;      // :10869-10873 (r = scale, aux2 = df)
    case gpb::kLogNormal: s->sum_log_y = weighted_sum_log_y(); s->log_norm_const = -s->sum_log_y - gauss_const; break;      // :10623-10631, :10887-10889 (r = variance of log y)
    case gpb::kGaussianLatent: s->log_norm_const = -gauss_const; break;                                   // :10874-10876 (r = error variance)
    default: return fail("the normalising constant of likelihood id %d is missing", s->link);
  }
  s->norm_dirty = false;
  return 0;
}
// what changed since the last evaluation, in the workspace's storage order: data map, response, weights (then the normalising constant), fixed effects; D; the
// storage-order copies of the full-scale approximation
int lap_eval_upload(gpb_hip_vecchia_t* h, LaplaceState* s, const LapEvalArgs& e) {
  const int n = h->n;
  hipStream_t st = h->stream;
  if (!h->has_transpose && build_transpose(h)) return -1;      // fills nn_host
  if (!h->has_levels && build_levels(h, s)) return -1;
  const bool mapped = !s->re_ptr.empty();
  const int nd = mapped ? s->n_data : n;
  // storage-order CSR of the random effects' data: the random effect in storage slot p is Vecchia position inv[p]
  std::vector<int> sptr;
  if (mapped) {
    std::vector<int> inv(n);
    for (int i = 0; i < n; ++i) inv[s->sigma[i]] = i;
    sptr.resize(n + 1); sptr[0] = 0;
    for (int p = 0; p < n; ++p) sptr[p + 1] = sptr[p] + (s->re_ptr[inv[p] + 1] - s->re_ptr[inv[p]]);
    if (s->map_dirty) {
      dev_free(s->d_dptr); dev_free(s->d_y); dev_free(s->d_fe); s->d_y = nullptr; s->d_fe = nullptr;
      HIP_OK(hipMalloc(&s->d_dptr, sizeof(int) * (size_t)(n + 1)));
      HIP_OK(hipMemcpy(s->d_dptr, sptr.data(), sizeof(int) * (size_t)(n + 1), hipMemcpyHostToDevice));
      s->y_dirty = true; s->fe_dirty = s->has_fe;
      s->map_dirty = false;
    }
  } else if (s->map_dirty) {
    dev_free(s->d_dptr); s->d_dptr = nullptr; dev_free(s->d_y); dev_free(s->d_fe); s->d_y = nullptr; s->d_fe = nullptr;
    s->y_dirty = true; s->fe_dirty = s->has_fe; s->map_dirty = false;
  }
  auto to_storage = [&](auto& dst, const auto& src) {        // per-datum values regrouped in the storage order of their random effects
    if (!mapped) { for (int i = 0; i < n; ++i) dst[s->sigma[i]] = src[i]; return; }
    for (int i = 0; i < n; ++i) {
      const int p = s->sigma[i], cnt = s->re_ptr[i + 1] - s->re_ptr[i];
      for (int k = 0; k < cnt; ++k) dst[sptr[p] + k] = src[s->re_ptr[i] + k];
    }
  };
  if (s->y_dirty) {
    if ((int)s->labels.size() != nd) return fail("the labels were set for %d data, the data map has %d", (int)s->labels.size(), nd);
    std::vector<int> ys(nd);
    to_storage(ys, s->labels);
    if (!s->d_y) HIP_OK(hipMalloc(&s->d_y, sizeof(int) * (size_t)nd));
    HIP_OK(hipMemcpy(s->d_y, ys.data(), sizeof(int) * (size_t)nd, hipMemcpyHostToDevice));
    if (gpb::lik_real_only(s->link) || s->real_resp) {
      if ((int)s->resp_real.size() != nd) return fail("the response was set for %d data, the data map has %d", (int)s->resp_real.size(), nd);
      std::vector<double> yr(nd);
      to_storage(yr, s->resp_real);
      dev_free(s->d_yd); s->d_yd = nullptr;
      HIP_OK(hipMalloc(&s->d_yd, sizeof(double) * (size_t)nd));
      HIP_OK(hipMemcpy(s->d_yd, yr.data(), sizeof(double) * (size_t)nd, hipMemcpyHostToDevice));
    }
    s->y_dirty = false;
  }
  if (!s->weights.empty() && (s->w_dirty || !s->d_w)) {
    if ((int)s->weights.size() != nd) return fail("the sample weights were set for %d data, the data map has %d", (int)s->weights.size(), nd);
    std::vector<double> ws(nd);
    to_storage(ws, s->weights);
    dev_free(s->d_w); s->d_w = nullptr;
    HIP_OK(hipMalloc(&s->d_w, sizeof(double) * (size_t)nd));
    HIP_OK(hipMemcpy(s->d_w, ws.data(), sizeof(double) * (size_t)nd, hipMemcpyHostToDevice));
    s->w_dirty = false;
  }
  if (s->norm_dirty && laplace_norm_consts(s, nd)) return -1;
  if (s->has_fe && s->fe_dirty) {
    if ((int)s->fe.size() != nd) return fail("the fixed effects were set for %d data, the data map has %d", (int)s->fe.size(), nd);
    std::vector<double> fs(nd);
    to_storage(fs, s->fe);
    if (!s->d_fe) HIP_OK(hipMalloc(&s->d_fe, sizeof(double) * (size_t)nd));
    HIP_OK(hipMemcpy(s->d_fe, fs.data(), sizeof(double) * (size_t)nd, hipMemcpyHostToDevice));
    s->fe_dirty = false;
  }
  if (!s->d_Ds) HIP_OK(hipMalloc(&s->d_Ds, sizeof(double) * (size_t)n));
  HIP_OK(gpb::lap_scatter(h->d_D, s->d_sigma, n, s->d_Ds, st));
  if (h->vif_k > 0 && vif_lap_pack(h, s, e.keep && s->pc_type == kPcFitc, st)) return -1;
  return 0;
}
// Probe columns N(0,1) in the layout [chunk][row][NCB]: column c from mt19937(seed_seq{seed, counter, 0, c}) (GenRandVecNormalParallel with run id `counter`), element i
// of it in row perm[i] (perm = null: row i); the columns padding the last chunk repeat real ones (finite, never read back)
void lap_draw(int seed, uint32_t counter, int rows, const int* perm, int t, const LapWork& w, double* dst) {
  std::vector<double> col(rows);
  for (int c = 0; c < t; ++c) {
    std::normal_distribution<double> ndist(0.0, 1.0);
    std::seed_seq seq{ static_cast<uint32_t>(seed), counter, 0u, static_cast<uint32_t>(c) };
    std::mt19937 gen(seq);
    for (int i = 0; i < rows; ++i) col[i] = ndist(gen);                 // element i of the reference's column c
    for (int cc = c; cc < w.tc; cc += t) {
      double* d = dst + (size_t)(cc / w.NCB) * rows * w.NCB + (cc % w.NCB);
      for (int i = 0; i < rows; ++i) d[(size_t)(perm ? perm[i] : i) * w.NCB] = col[i];
    }
  }
}
// workspace of t probe vectors and p_max Lanczos steps; the probes, drawn again when t, the seed or the preconditioner changed
int lap_eval_workspace(gpb_hip_vecchia_t* h, LaplaceState* s, const LapEvalArgs& e) {
  const int n = h->n, t = e.t;
  const LapWork w = lap_work(h, s, t);                 // (its sizes; the views are taken once everything is allocated)
  const int tc = w.tc, p_max = std::min(e.cg_max_num_it_tridiag, n);
  if (!s->d_vec) {      // zero-initialised (the solves themselves select padding entries out: their results do not depend on what a vector held before)
    HIP_OK(hipMalloc(&s->d_vec, LapWork::vec_bytes(n)));
    HIP_OK(hipMemset(s->d_vec, 0, LapWork::vec_bytes(n)));
  }
  if (!s->d_gvec) {
    HIP_OK(hipMalloc(&s->d_gvec, LapWork::gvec_bytes(n)));
    HIP_OK(hipMemset(s->d_gvec, 0, LapWork::gvec_bytes(n)));
  }
  if (!s->d_o) { HIP_OK(hipMalloc(&s->d_o, sizeof(double) * 8)); }
  if (!s->d_err) {
    HIP_OK(hipMalloc(&s->d_err, sizeof(int)));
    HIP_OK(hipMemset(s->d_err, 0, sizeof(int)));
  }
  const bool vif = h->vif_k > 0;
  const bool pc = lap_form(s) == LapForm::kWinvPlusSigma;
  const bool vifdu = s->pc_type == kPcVifdu, fitc = s->pc_type == kPcFitc;
  const bool vr = s->pc_type == kPcVecchiaResponse;                    // no low-rank part: no second set of normals, the probes are drawn with generator counter 0 (likelihoods.h:3993-4009)
  if (vr) { s->vr_cov = e.cov_type; s->vr_var = e.var; s->vr_a = e.a; }
  if (fitc && s->pc_nip < 1) return fail("the fitc preconditioner needs its inducing points (gpb_hip_vecchia_laplace_set_inducing_points)");
  const int pck = fitc ? s->pc_nip : ((pc && !vr) ? std::min(s->pc_rank, n) : (vifdu ? h->vif_k : 0));
  if (s->t != t || s->p_max != p_max || s->seed != e.seed || !s->d_rv || s->rv_pc != s->pc_type || s->rv_k != pck) {
    dev_free(s->d_rv); dev_free(s->d_blk); dev_free(s->d_sc); dev_free(s->d_pcrv2); dev_free(s->d_vifrv3);
    if (s->h_o) { (void)hipHostFree(s->h_o); s->h_o = nullptr; }
    HIP_OK(hipMalloc(&s->d_rv, sizeof(double) * (size_t)n * tc));
    HIP_OK(hipMalloc(&s->d_blk, LapWork::blk_bytes(n, tc)));
    HIP_OK(hipMemset(s->d_blk, 0, LapWork::blk_bytes(n, tc)));
    HIP_OK(hipMalloc(&s->d_sc, sizeof(double) * LapWork::sc_doubles(tc, p_max)));
    HIP_OK(hipHostMalloc(&s->h_o, sizeof(double) * (size_t)(8 + tc)));
    // pivoted_cholesky: rand_vec_trace_I2_ (k x t) is drawn FIRST (generator counter 0), rand_vec_trace_I_ second (counter 1) -- likelihoods.h:3993-4009
    // (full-scale Vecchia: rand_vec_trace_I2_ (n x t) is drawn FIRST, rand_vec_trace_P_ (k x t) second, likelihoods.h:3633-3652)
    if ((pc && !vr) || vifdu) {               // ("vifdu": rand_vec_trace_P_, k x t, generator counter 1, likelihoods.h:3641-3646)
      std::vector<double> rv2((size_t)pck * tc);
      lap_draw(e.seed, vif ? 1u : 0u, pck, nullptr, t, w, rv2.data());
      HIP_OK(hipMalloc(&s->d_pcrv2, sizeof(double) * (size_t)pck * tc));
      HIP_OK(hipMemcpy(s->d_pcrv2, rv2.data(), sizeof(double) * (size_t)pck * tc, hipMemcpyHostToDevice));
    }
    std::vector<double> rv((size_t)n * tc);
    lap_draw(e.seed, (pc && !vr && !vif) ? 1u : 0u, n, s->sigma.data(), t, w, rv.data());
    HIP_OK(hipMemcpy(s->d_rv, rv.data(), sizeof(double) * (size_t)n * tc, hipMemcpyHostToDevice));
    if (vifdu) {                               // rand_vec_trace_I3_: generator counter 2
      lap_draw(e.seed, 2u, n, s->sigma.data(), t, w, rv.data());
      HIP_OK(hipMalloc(&s->d_vifrv3, sizeof(double) * (size_t)n * tc));
      HIP_OK(hipMemcpy(s->d_vifrv3, rv.data(), sizeof(double) * (size_t)n * tc, hipMemcpyHostToDevice));
    }
    s->t = t; s->p_max = p_max; s->seed = e.seed; s->rv_pc = s->pc_type; s->rv_k = pck;
  }
  return 0;
}
// this evaluation's A in the level-ordered layouts, the inverses of the solves' dense blocks, the covariance part of the low-rank preconditioners; "vifdu" / "none":
// the scratch of Sigma^-1 = S - Q M^-1 Q' (S = B'D^-1B, Q = S C) and M^-1 on the device
int lap_eval_operators(gpb_hip_vecchia_t* h, LaplaceState* s, const LapEvalArgs& e, const LapWork& w) {
  const int n = h->n;
  hipStream_t st = h->stream;
  const gpb::LapLevels lv = make_levels(h, s);
  for (LaplaceState::Tri* tr : { &s->fwd, &s->bwd })
    HIP_OK(gpb::lap_permute_factor(h->d_A, tr->hpos, tr->opos, (size_t)tr->nslots * 32, tr->novf, tr->hent, tr->oent, st));
  HIP_OK(gpb::lap_dense_build(lv.fdense, h->d_A, st));
  HIP_OK(gpb::lap_dense_build(lv.bdense, h->d_A, st));
  if (pc_has_lowrank(s->pc_type) && pc_factor_sigma(h, s, e.cov_type, e.var, e.a, st)) return -1;
  if (lap_form(s) == LapForm::kVifSigmaInv) {
    const int vk = h->vif_k;
    const size_t need = (size_t)2 * w.nb + (size_t)2 * n;      // (LapSolver: vblkA, vblkB, vwdd, vwgt)
    if (s->vifblk_cap < need) { dev_free(s->d_vifblk); s->vifblk_cap = 0; HIP_OK(hipMalloc(&s->d_vifblk, sizeof(double) * need)); s->vifblk_cap = need; }
    if (!s->d_vifMinv) HIP_OK(hipMalloc(&s->d_vifMinv, sizeof(double) * (size_t)2 * vk * vk));
    std::vector<double> Mi(s->vif_M);
    double ldm = 0.0;
    if (!spd_invert(Mi, vk, &ldm)) return fail("the Woodbury matrix of the full-scale Vecchia approximation is not positive definite");
    HIP_OK(hipMemcpy(s->d_vifMinv, Mi.data(), sizeof(double) * (size_t)vk * vk, hipMemcpyHostToDevice));
  }
  return 0;
}
// mode finding (likelihoods.h:3773-3978): Newton steps with Armijo backtracking, every step one preconditioned CG solve
struct LapMode { int it = 0, total_cg = 0; double amll = 0.; bool bad = false; };
int lap_find_mode(gpb_hip_vecchia_t* h, LaplaceState* s, const LapEvalArgs& e, const LapWork& w, const LapSolver& op, LapMode* res) {
  const int n = h->n;
  hipStream_t st = h->stream;
  const size_t vb = w.vb;
  const gpb::LapLevels& lv = op.lv;
  const double* Ds = s->d_Ds;
  const double* fe = s->has_fe ? s->d_fe : nullptr;
  const bool vif = op.vif, pc = op.form == LapForm::kWinvPlusSigma, vsi = op.form == LapForm::kVifSigmaInv;
  const LapScratch scr{ w.t1, w.t2, w.dir, w.gv };
  // (gaussian_latent: the objective is quadratic in the mode -- ONE Newton step with ONE trial point, likelihoods.h:473-474)
  const bool one_step = gpb::lik_single_newton_step(s->link);
  const int maxit_mode_newton = one_step ? 1 : 1000, max_lr_shrink = one_step ? 1 : 20;        // :17316, :17322
  const double c_armijo = 1e-4, thr_zero_rhs = 1e-100;            // :17332; ZERO_RHS_CG_THRESHOLD
  if (e.reset_mode || !s->has_mode) HIP_OK(hipMemsetAsync(w.mode, 0, vb, st));
  HIP_OK(hipMemcpyAsync(w.mprev, w.mode, vb, hipMemcpyDeviceToDevice, st));       // mode_previous_value_ (likelihoods.h:3790-3797)
  HIP_OK(gpb::lap_B(lv, n, w.mode, w.Bm, 1, 1, st));
  HIP_OK(gpb::lap_objective(s->link, w.mode, s->resp(), fe, w.Bm, Ds, n, s->d_o, st, s->d_dptr));
  if (vif && vif_qf_enqueue(s, n, w.Bm, 0, st)) return -1;
  if (lap_fetch(s, 2, st)) return -1;
  double amll = s->h_o[0] + s->log_norm_const - 0.5 * (s->h_o[1] - (vif ? vif_qf_value(s, 0) : 0.0)), amll_new = amll;
  int it = 0, total_cg = 0;
  bool bad = false, upd_is_zero = false;
  const LapCgRule rule{ std::min(e.cg_max_num_it, n), e.cg_delta_conv, 1, false, 1, false };
  for (it = 0; it < maxit_mode_newton; ++it) {
    HIP_OK(gpb::lap_newton_setup(s->link, w.mode, s->resp(), fe, Ds, n, w.W, w.rhs, w.dw, w.rdw, st, s->d_dptr));
    // --- CGVecchiaLaplaceVec ---
    HIP_OK(gpb::lap_dot(w.rhs, w.rhs, n, s->d_o, st));
    if (lap_fetch(s, 2, st)) return -1;
    int ncg = 0;
    if (s->h_o[1] < thr_zero_rhs) {
      HIP_OK(hipMemsetAsync(w.upd, 0, vb, st));
      if (vif) HIP_OK(hipMemsetAsync(s->d_vifu, 0, vb, st));
      upd_is_zero = true;
    } else {
      if (pc || vsi) {      // the Woodbury inverses are unstable for a very large information (likelihoods.h:16282-16284, :3501-3509); the preconditioner for this W (:16282-16295)
        HIP_OK(gpb::pc_wmax(w.W, n, s->d_o, st));
        if (lap_fetch(s, 1, st)) return -1;
        if (!(s->h_o[0] <= 1e10)) { bad = true; break; }
        int pbad = 0;
        if (pc ? op.pc_renew(&pbad, false) : (s->pc_type == kPcVifdu && op.vifdu_refresh(&pbad))) return -1;
        if (pbad) { bad = true; break; }
      }
      if (pc) {
        // --- CGVecchiaLaplace_Version_SigmaPlusWinvVec (CG_utils.cpp:231-343): (W^-1 + Sigma) u' = Sigma rhs, u = W^-1 u' ---
        if (op.sigma(w.rhs, w.gv, w.t2, 1, 1)) return -1;                           // Sigma rhs (:267-268; + C Sigma_m^-1 C' rhs, likelihoods.h:3535-3538)
        if (it == 0 || upd_is_zero) {
          HIP_OK(hipMemsetAsync(w.upd, 0, vb, st));
          HIP_OK(hipMemcpyAsync(w.r, w.gv, vb, hipMemcpyDeviceToDevice, st));
        } else if (vif) {                                                           // the iterate is u' of the previous Newton step: r = Sigma rhs - (W^-1 + Sigma) u' (CG_utils.cpp:781-785)
          HIP_OK(hipMemcpyAsync(w.upd, s->d_vifu, vb, hipMemcpyDeviceToDevice, st));
          if (op.apply(w.upd, w.dir, LapScratch{ w.t2, nullptr, nullptr, nullptr }, 1, 1)) return -1;
          HIP_OK(gpb::lap_lincomb(w.r, w.gv, w.dir, 1.0, -1.0, n, st));
        } else {                                                                    // r = Sigma rhs - u - Sigma W u, the iterate becomes u' = W u (:277-284)
          HIP_OK(gpb::lap_lincomb(w.r, w.gv, w.upd, 1.0, -1.0, n, st));
          HIP_OK(gpb::pc_rowscale(w.upd, w.W, n, 1, 1, 0, w.upd, st));
          if (op.sigma(w.upd, w.dir, w.t2, 1, 1)) return -1;
          HIP_OK(gpb::lap_lincomb(w.r, w.r, w.dir, 1.0, -1.0, n, st));
        }
      } else if (it == 0) {
        HIP_OK(hipMemsetAsync(w.upd, 0, vb, st));
        HIP_OK(hipMemcpyAsync(w.r, w.rhs, vb, hipMemcpyDeviceToDevice, st));
      } else {
        if (op.apply(w.upd, w.v, scr, 1, 1)) return -1;
        HIP_OK(gpb::lap_lincomb(w.r, w.rhs, w.v, 1.0, -1.0, n, st));
      }
      upd_is_zero = false;
      if (op.precond(w.r, w.z, scr, 1, 1)) return -1;
      HIP_OK(hipMemcpyAsync(w.hh, w.z, vb, hipMemcpyDeviceToDevice, st));
      const int end = lap_cg(op, scr, w.upd, w.r, w.z, w.hh, w.v, 1, 1, w.sc1, rule, &ncg);
      if (end == LAP_CG_ERROR) return -1;
      if (end == LAP_CG_NONFINITE) { bad = true; break; }
      if (pc) {                                                                     // converged or at the cap
        if (vif) HIP_OK(hipMemcpyAsync(s->d_vifu, w.upd, vb, hipMemcpyDeviceToDevice, st));      // mode_update_part: the next Newton step's start (likelihoods.h:3540-3543)
        HIP_OK(gpb::pc_rowscale(w.upd, w.W, n, 1, 1, 1, w.upd, st));                             // u = W^-1 u' (:305-307)
      }
    }
    total_cg += ncg;
    // --- Armijo backtracking (:3929-3966) ---
    HIP_OK(gpb::lap_lincomb(w.dir, w.upd, w.mode, 1.0, -1.0, n, st));
    HIP_OK(gpb::lap_apply(lv, n, Ds, w.W, w.dir, w.gv, w.t1, 1, 1, st));
    HIP_OK(gpb::lap_dot(w.dir, w.gv, n, s->d_o + 2, st));
    if (vif) {                                                                      // - dir' Q M^-1 Q' dir: the Woodbury part of dir' Sigma^-1 dir (likelihoods.h:3585-3588)
      HIP_OK(gpb::lap_B(lv, n, w.dir, w.t2, 1, 1, st));
      if (vif_qf_enqueue(s, n, w.t2, 1, st)) return -1;
    }
    double lr = 1.0, gdd = 0.0;
    for (int ih = 0; ih < max_lr_shrink; ++ih) {
      if (ih == 0) HIP_OK(hipMemcpyAsync(w.mnew, w.upd, vb, hipMemcpyDeviceToDevice, st));
      else HIP_OK(gpb::lap_lincomb(w.mnew, w.mode, w.upd, 1.0 - lr, lr, n, st));
      HIP_OK(gpb::lap_B(lv, n, w.mnew, w.Bm, 1, 1, st));
      HIP_OK(gpb::lap_objective(s->link, w.mnew, s->resp(), fe, w.Bm, Ds, n, s->d_o, st, s->d_dptr));
      if (vif && vif_qf_enqueue(s, n, w.Bm, 0, st)) return -1;
      if (lap_fetch(s, 4, st)) return -1;
      gdd = s->h_o[2] - (vif ? vif_qf_value(s, 1) : 0.0);
      amll_new = s->h_o[0] + s->log_norm_const - 0.5 * (s->h_o[1] - (vif ? vif_qf_value(s, 0) : 0.0));
      if (amll_new < (amll + c_armijo * lr * gdd) || std::isnan(amll_new) || std::isinf(amll_new)) lr *= 0.5;
      else break;
    }
    HIP_OK(hipMemcpyAsync(w.mode, w.mnew, vb, hipMemcpyDeviceToDevice, st));
    // --- CheckConvergenceModeFinding (:16078-16128) ---
    if (std::isnan(amll_new) || std::isinf(amll_new)) { bad = true; break; }
    bool term;
    if (it == 0) term = std::fabs(amll_new - amll) < e.delta_conv_mode_finding * std::fabs(amll);
    else term = (amll_new - amll) < e.delta_conv_mode_finding * std::fabs(amll);
    amll = amll_new;
    if (term) break;
  }
  s->has_mode = !bad;
  HIP_OK(hipStreamSynchronize(st));
  res->it = it; res->total_cg = total_cg; res->amll = amll; res->bad = bad;
  return 0;
}
// log|Sigma W + I| by stochastic Lanczos quadrature (likelihoods.h:16476-16515) at the mode; out9_host[0], [3], [4]
int lap_logdet(gpb_hip_vecchia_t* h, LaplaceState* s, const LapEvalArgs& e, const LapWork& w, const LapSolver& op, double amll, double* out9_host) {
  const int n = h->n, t = e.t, tch = w.tch, NCB = w.NCB, tc = w.tc, p_max = s->p_max, vk = h->vif_k;
  hipStream_t st = h->stream;
  const size_t nb = w.nb;
  const gpb::LapLevels& lv = op.lv;
  const double* Ds = s->d_Ds;
  const bool vif = op.vif, pc = op.form == LapForm::kWinvPlusSigma, vsi = op.form == LapForm::kVifSigmaInv;
  const bool fitc = s->pc_type == kPcFitc, vr = s->pc_type == kPcVecchiaResponse, vifdu = s->pc_type == kPcVifdu;
  double *R = w.R, *Z = w.Z, *H = w.H, *Vb = w.Vb, *T = w.T;
  const LapScratch scr{ T, T, op.vblkA, op.vblkB };
  auto lost = [&](int k_done) { out9_host[0] = NAN; out9_host[3] = NAN; out9_host[4] = k_done; };
  HIP_OK(gpb::lap_newton_setup(s->link, w.mode, s->resp(), s->has_fe ? s->d_fe : nullptr, Ds, n, w.W, nullptr, w.dw, w.rdw, st, s->d_dptr));      // information at the mode (:3981-3984)
  if (pc) {
    // pivoted_cholesky (:16389-16419): the preconditioner at the information of the mode, probes z_c = L_k r2_c + W^-1/2 r_c with Cov(z_c) = P, Z = P^-1 R
    HIP_OK(gpb::lap_logsums(Ds, w.W, n, s->d_o + 4, st));                                   // d_o[5] = sum log W
    int pbad = 0;
    // (full-scale Vecchia: the reference keeps the preconditioner of the LAST NEWTON STEP's information -- diagonal_approx_preconditioner_ / chol_fact_woodbury_preconditioner_ are
    //  renewed inside the Newton loop only, likelihoods.h:3511-3534; the probes :3687 and the log-determinant's terms :16240-16246 use them)
    if (!vif && op.pc_renew(&pbad, true)) return -1;
    if (pbad) {
      lost(0);
      if (vr) return fail("the Vecchia factor of W^-1 + Sigma is not positive (vecchia_response preconditioner of the log-determinant; zeros or negative values in the information?)");   // likelihoods.h:16389-16397
      return fail("the Cholesky factorisation of I_k + L_k' W L_k failed (pivoted_cholesky preconditioner of the log-determinant)");     // CheckCholeskyFactorization, :16417
    }
    // (fitc: z_c = V r2_c + D^1/2 r_c, :16437;  vecchia_response: z_c = B_p^-1 D_p^1/2 r_c, :16446-16450)
    if (vr) HIP_OK(gpb::lap_fwd_solve(make_levels_vr(h, s), n, s->d_vrDs + n, s->d_rv, R, tch, NCB, st));
    else HIP_OK(gpb::pc_combine(fitc ? s->d_pcV : s->d_pcL, s->pc_wp(w.W), s->d_rv, s->d_pcrv2, n, s->pc_k, tch, NCB, 2, R, st));
  } else if (vsi) {
    HIP_OK(gpb::lap_logsums(Ds, w.dw, n, s->d_o + 4, st));
    if (!vifdu) HIP_OK(hipMemcpyAsync(R, s->d_rv, sizeof(double) * nb, hipMemcpyDeviceToDevice, st));      // "none": rand_vec_trace_I_ = rand_vec_trace_I2_ (likelihoods.h:3689-3691)
    else {
      // "vifdu": P^1/2 r = B' W^1/2 r_2 + Sigma^-1 (V r_P + B^-1 D^1/2 r_3)  (likelihoods.h:3654-3685); the preconditioner at the information of the mode (:3693-3707)
      int pbad = 0;
      if (op.vifdu_refresh(&pbad)) return -1;
      if (pbad) { lost(0); return fail("the Cholesky factorisation of the vifdu preconditioner's Woodbury matrix failed (log-determinant)"); }
      HIP_OK(gpb::lap_scale_probes(s->d_rv, w.W, n, tch, NCB, T, st));
      HIP_OK(gpb::lap_Bt(lv, n, T, R, tch, NCB, st));                                            // B' W^1/2 r_2
      HIP_OK(gpb::lap_scale_probes(s->d_vifrv3, Ds, n, tch, NCB, T, st));
      HIP_OK(gpb::lap_fwd_solve(lv, n, s->d_vifones, T, Vb, tch, NCB, st));                       // B^-1 D^1/2 r_3
      if (vif_small(s, n, vk, tch, NCB)) return -1;
      HIP_OK(gpb::pc_combine(s->d_vifV, s->d_vifones, Vb, s->d_pcrv2, n, vk, tch, NCB, 2, H, st));   // Sigma^1/2 r = V r_P + B^-1 D^1/2 r_3
      HIP_OK(gpb::lap_B(lv, n, H, T, tch, NCB, st));
      HIP_OK(gpb::pc_rowscale(T, op.Dinv, n, tch, NCB, 0, T, st));
      HIP_OK(gpb::lap_Bt(lv, n, T, Vb, tch, NCB, st));                                           // S Sigma^1/2 r
      HIP_OK(gpb::lap_lincomb(R, R, Vb, 1.0, 1.0, (int)nb, st));
      HIP_OK(gpb::pc_ltwx(s->d_vifC, s->d_vifones, s->d_vifMinv, Vb, n, vk, tch, NCB, s->d_pcpart, s->d_vifx2, st));       // M^-1 C' S Sigma^1/2 r
      HIP_OK(gpb::pc_combine(s->d_vifBC, op.Dinv, T, s->d_vifx2, n, vk, tch, NCB, 3, T, st));                              // -D^-1 B C (.)
      HIP_OK(gpb::lap_Bt(lv, n, T, Vb, tch, NCB, st));                                                                    // -Q M^-1 C' S Sigma^1/2 r
      HIP_OK(gpb::lap_lincomb(R, R, Vb, 1.0, 1.0, (int)nb, st));
    }
  } else {
    HIP_OK(gpb::lap_logsums(Ds, w.dw, n, s->d_o + 4, st));
    HIP_OK(gpb::lap_scale_probes(s->d_rv, w.dw, n, tch, NCB, T, st));                        // z_c = B^T (D^-1 + W)^0.5 r_c
    HIP_OK(gpb::lap_Bt(lv, n, T, R, tch, NCB, st));
  }
  if (op.precond(R, Z, scr, tch, NCB)) return -1;
  HIP_OK(hipMemcpyAsync(H, Z, sizeof(double) * nb, hipMemcpyDeviceToDevice, st));
  const bool keep = e.keep && !vr && !vsi;
  double* Ublk = nullptr;
  if (keep) {
    const size_t gneed = (pc ? 4 : 2) * nb;               // pivoted_cholesky: U, the probes Z, and Sigma U / Sigma W W^-1 P^-1 Z of the gradient
    if (s->gblk_cap < gneed) {
      dev_free(s->d_gblk); s->gblk_cap = 0;
      HIP_OK(hipMalloc(&s->d_gblk, sizeof(double) * gneed));
      s->gblk_cap = gneed;
    }
    Ublk = s->d_gblk;
    HIP_OK(hipMemsetAsync(Ublk, 0, sizeof(double) * nb, st));
    HIP_OK(hipMemcpyAsync(s->d_gblk + nb, pc ? R : Z, sizeof(double) * nb, hipMemcpyDeviceToDevice, st));     // PI_Z (vadu) / rand_vec_trace_P_ (pivoted_cholesky)
  }
  if (lap_cg_reset(w, st)) return -1;
  int k_done = 0;
  // (the mean over the t real columns: the padding columns are not looked at)
  const int end = lap_cg(op, scr, Ublk, R, Z, H, Vb, tch, NCB, w.sct, LapCgRule{ p_max, e.cg_delta_conv, t, false, p_max, true }, &k_done);
  if (end == LAP_CG_ERROR) return -1;
  if (end == LAP_CG_NONFINITE) {
    lost(k_done);
    return fail("NaN or Inf occurred in the conjugate gradient algorithm (log-determinant)");       // CG_utils.cpp:183-186
  }
  std::vector<double> Tds((size_t)2 * tc * p_max);
  HIP_OK(hipMemcpyAsync(Tds.data(), w.sct.Td, sizeof(double) * Tds.size(), hipMemcpyDeviceToHost, st));
  if (lap_fetch(s, 6, st)) return -1;
  if (lap_check_solves(s, st)) return -1;
  double ldet = 0.0;
  for (int c = 0; c < t; ++c) ldet += tridiag_quadrature_log(Tds.data() + (size_t)c * p_max, Tds.data() + (size_t)tc * p_max + (size_t)c * p_max, k_done);
  ldet = ldet * n / t;                                                              // CG_utils.cpp:1050
  // vadu: log|P^-1 (Sigma^-1 + W)| + log|P| + log|Sigma| (:16504-16509); pivoted_cholesky: log|P^-1 (W^-1 + Sigma)| + log|W| + log|P|,
  // log|P| = log|I_k + L_k' W L_k| - log|W| (:16457-16465)
  // fitc: log|P| = log|Sigma_m + C' D^-1 C| - log|Sigma_m| - log|D^-1| (:16465-16470; pc_refresh)
  // vecchia_response: log|P| = -log|D_p^-1| (:16471-16473; pc_refresh_vr)
  // full-scale Vecchia, "vifdu" / "none" (CalcLogDetStochFSVA, :16248-16256): - log|Sigma_m| - sum log D^-1 + (sum log(W + D^-1) + log|sigma_woodbury_woodbury| or log|sigma_woodbury|)
  const double log_det = vsi ? ldet - s->vif_logdet_Sm - s->h_o[4] + (vifdu ? s->h_o[5] + s->vif_logdet_MM : s->vif_logdet_M)
                       : pc ? (ldet + s->h_o[5]) + ((fitc || vr) ? s->pc_logdet : s->pc_logdet - s->h_o[5]) : ldet - s->h_o[4] + s->h_o[5];
  out9_host[0] = amll - 0.5 * log_det;                                              // :4026
  out9_host[3] = log_det; out9_host[4] = k_done;
  if (keep) { s->grad_state = true; s->g_cov = e.cov_type; s->g_var = e.var; s->g_a = e.a; s->g_t = t; }
  return 0;
}

// One evaluation of the approximate marginal likelihood (mode finding + log-determinant).  flags & LAP_KEEP_GRAD_STATE: the block CG of
// the log-determinant also accumulates U (CG_utils.cpp:173) and PI_Z is kept, as the reference does when the gradient may follow.
int laplace_eval(gpb_hip_vecchia_t* h, int cov_type, double var, double a, int num_rand_vec, int seed_rand_vec,
                 int cg_max_num_it, int cg_max_num_it_tridiag, double cg_delta_conv, double delta_conv_mode_finding,
                 int flags, double* out9_host, double* mode_host) {
  if (!h || !out9_host) return fail("null argument");
  if (!h->lap || !h->lap->has_y) return fail("labels have not been set (call gpb_hip_vecchia_laplace_set_labels)");
  if (h->i_begin != 0 || h->i_end != h->n) return fail("the Vecchia-Laplace path needs the whole factor on one device (shard is [%d,%d))", h->i_begin, h->i_end);
  if (num_rand_vec < 1 || cg_max_num_it < 1 || cg_max_num_it_tridiag < 1) return fail("num_rand_vec, cg_max_num_it and cg_max_num_it_tridiag must be positive");
  HIP_OK(hipSetDevice(h->device));
  LaplaceState* s = h->lap;
  const int n = h->n;
  hipStream_t st = h->stream;
  const LapEvalArgs e{ cov_type, var, a, num_rand_vec, seed_rand_vec, cg_max_num_it, cg_max_num_it_tridiag, cg_delta_conv, delta_conv_mode_finding,
                       (flags & LAP_RESET_MODE) != 0, (flags & LAP_KEEP_GRAD_STATE) != 0 };
  const auto t_start = std::chrono::steady_clock::now();
  s->grad_state = false; s->gvec_state = false;
  if (lap_eval_factor(h, s, e)) return -1;
  const double ms_factor = ms_since(t_start);
  if (lap_eval_upload(h, s, e)) return -1;
  if (lap_eval_workspace(h, s, e)) return -1;
  const LapWork w = lap_work(h, s, e.t);
  if (lap_eval_operators(h, s, e, w)) return -1;
  const LapSolver op = lap_solver(h, s, w, lap_form(s));
  LapMode md;
  if (lap_find_mode(h, s, e, w, op, &md)) return -1;
  const double ms_mode = ms_since(t_start);
  out9_host[1] = md.it; out9_host[2] = md.total_cg; out9_host[5] = md.amll;
  out9_host[6] = ms_factor; out9_host[7] = ms_mode - ms_factor; out9_host[8] = 0.;
  if (mode_host) {                       // back to the Vecchia order
    std::vector<double> ms(n);
    HIP_OK(hipMemcpyAsync(ms.data(), w.mode, w.vb, hipMemcpyDeviceToHost, st));
    HIP_OK(hipStreamSynchronize(st));
    for (int i = 0; i < n; ++i) mode_host[i] = ms[s->sigma[i]];
  }
  if (md.bad) {
    out9_host[0] = NAN; out9_host[3] = NAN; out9_host[4] = 0;
    return fail("NaN or Inf occurred in the mode finding algorithm for the Laplace approximation");   // likelihoods.h:16100-16103
  }
  const auto t_det = std::chrono::steady_clock::now();
  if (lap_logdet(h, s, e, w, op, md.amll, out9_host)) return -1;
  out9_host[8] = ms_since(t_det);
  return 0;
}
// ---- full-scale Vecchia x non-Gaussian likelihood: the covariance parameters' part of CalcGradNegMargLikelihoodLaplaceApproxFSVA (likelihoods.h:5413-5520), "fitc" preconditioner.
// Everything that is n x k stays on the device and is reduced to k-vectors / k x k Gram matrices (pc_ltwx, pc_gram); the k x k algebra of the Woodbury terms runs on the host:
//   explicit + implicit part   x' SigmaI_deriv_mode for x = mode, (Sigma^-1 + W)^-1 d_mll_d_mode, SigmaI_deriv_mode written with Sigma^-1 = S - S C M^-1 C' S (S = B'D^-1B, M the Woodbury
//                              matrix) and its derivative (:5455-5461), reduced to C' S x, C' S_deriv x, dC' S x (k-vectors) by the symmetry of S and S_deriv
//   stochastic trace           mean_c U_c' (dSigma / dtheta) P^-1 Z_c, dSigma = d(C Sigma_m^-1 C') - Sigma_v S_deriv Sigma_v (:5462-5472; the second half is the Vecchia path's own code)
//   variance reduction         with dP / dtheta of the fitc preconditioner: its low-rank part, the derivative of its diagonal (:5478-5486), the deterministic trace (:5488-5499), optimal c
// Checker: oracle/orc.py vif_laplace_grad (same steps, same names).
struct VifGradHost {
  int k = 0, kp = 0;
  std::vector<double> dSm[2], dSmp[2];      // derivatives of the UN-jittered Sigma_m / the preconditioner's (GetZSigmaZtGrad): [0] = the matrix itself (log variance), [1] = wrt log(range)
  std::vector<double> Mg[2], Mgp[2];        // sigma_woodbury_grad, sigma_woodbury_grad_preconditioner
  double sum_dgrad_wp[2] = { 0., 0. };
  std::vector<double> CU, dCU, CP, dCP, CpP, dCpP;      // block reductions, layout [chunk][k][4]
  std::vector<double> wn[2];                // sum_i dgrad_i (P^-1 Z)_ic^2 per column
  std::vector<double> yC, ydC;              // [4][k]: C' / dC' times (S0 mode, S0 sv, S1 mode, S1 sv)
  double *d_dgrad[2] = { nullptr, nullptr };
};
namespace {
// x <- (L L')^-1 x given Linv = L^-1 (lower, row-major)
void apply_linv_sym(const std::vector<double>& Linv, int k, const double* x, double* out) {
  std::vector<double> t(k);
  for (int i = 0; i < k; ++i) { double a = 0.0; for (int p = 0; p <= i; ++p) a += Linv[(size_t)i * k + p] * x[p]; t[i] = a; }
  for (int i = 0; i < k; ++i) { double a = 0.0; for (int p = i; p < k; ++p) a += Linv[(size_t)p * k + i] * t[p]; out[i] = a; }
}
}  // namespace
int vif_grad_prepare(gpb_hip_vecchia_t* h, LaplaceState* s, VifGradHost* vg, hipStream_t st) {
  const int n = h->n, m = h->m, k = h->vif_k, kq = h->vif_kq, kp = s->pc_k;
  const int K = std::max(k, kp);
  vg->k = k; vg->kp = kp;
  const int cov = s->g_cov; const double var = s->g_var, a = s->g_a;
  const size_t k2 = (size_t)k * k, kp2 = (size_t)kp * kp;
  for (int p = 0; p < 2; ++p) { vg->dSm[p].resize(k2); vg->dSmp[p].resize(kp2); }
  sm::ip_cov(h->vif_ip_host.data(), k, 3, sm::IpLayout::RowMajorKx3, sm::MaternForm::LaplacePaths, cov, var, a, vg->dSm[0].data(), vg->dSm[1].data());
  sm::ip_cov(s->pc_ip.data(), kp, 3, sm::IpLayout::RowMajorKx3, sm::MaternForm::LaplacePaths, cov, var, a, vg->dSmp[0].data(), vg->dSmp[1].data());
  // ---- dA / dD of the latent residual process (Vecchia_utils.cpp:1503-1524, :1640-1656): the VIF derivative kernel; of its inputs only Si = Sigma_m^-1, N0 = 2 Si - Si dSm0 Si
  //      and negMp1 = -Si dSm1 Si matter here (the Gaussian path's sums are not used) ----
  std::vector<double> Si(k2), N0(k2), negMp1(k2), Iw(k2, 0.0), w0(k, 0.0), tmp((size_t)K * K), tmp2(k2);
  sm::spd_inverse_from_tri(s->vif_Linv.data(), k, Si.data());
  for (int i = 0; i < k; ++i) Iw[(size_t)i * k + i] = 1.0;
  sm::matmul(Si.data(), vg->dSm[0].data(), k, tmp.data()); sm::matmul(tmp.data(), Si.data(), k, tmp2.data());
  for (size_t e = 0; e < k2; ++e) N0[e] = 2.0 * Si[e] - tmp2[e];
  sm::matmul(Si.data(), vg->dSm[1].data(), k, tmp.data()); sm::matmul(tmp.data(), Si.data(), k, tmp2.data());
  for (size_t e = 0; e < k2; ++e) negMp1[e] = -tmp2[e];
  double sums12[GPB_VIF_GRAD_TERMS];
  if (vif_grad_sums_impl(h, cov, var, a, Iw.data(), Si.data(), N0.data(), negMp1.data(), w0.data(), 1, sums12, true)) return -1;
  HIP_OK(hipMemcpyAsync(s->d_dA, h->d_vdA + (size_t)n * m, sizeof(double) * (size_t)n * m, hipMemcpyDeviceToDevice, st));
  HIP_OK(hipMemcpyAsync(s->d_dD, h->d_vdD + (size_t)n, sizeof(double) * (size_t)n, hipMemcpyDeviceToDevice, st));
  // ---- scratch: two [n][K] matrices, six n-vectors ----
  const size_t needT = (size_t)2 * n * K + (size_t)6 * n, needq = std::max((size_t)4 * K * K, (size_t)64 * K * 4);
  if (s->vifT_cap < needT) { dev_free(s->d_vifT); s->vifT_cap = 0; HIP_OK(hipMalloc(&s->d_vifT, sizeof(double) * needT)); s->vifT_cap = needT; }
  if (s->vifq_cap < needq) { dev_free(s->d_vifq); s->vifq_cap = 0; HIP_OK(hipMalloc(&s->d_vifq, sizeof(double) * needq)); s->vifq_cap = needq; }
  if (!s->d_pcI) {
    std::vector<double> Ik((size_t)kp * kp, 0.0); for (int q = 0; q < kp; ++q) Ik[(size_t)q * kp + q] = 1.0;
    HIP_OK(hipMalloc(&s->d_pcI, sizeof(double) * Ik.size()));
    HIP_OK(hipMemcpy(s->d_pcI, Ik.data(), sizeof(double) * Ik.size(), hipMemcpyHostToDevice));
  }
  double *T1 = s->d_vifT, *T2 = T1 + (size_t)n * K, *vecs = T2 + (size_t)n * K;
  double *dg0 = vecs, *dg1 = vecs + n, *wDD = vecs + 2 * (size_t)n, *wtmp = vecs + 3 * (size_t)n, *dDs = vecs + 4 * (size_t)n;
  vg->d_dgrad[0] = dg0; vg->d_dgrad[1] = dg1;
  if (vif_small(s, n, K, 64, 4)) return -1;
  const double* wD = s->d_vifones + n;                    // 1 / D, storage order
  auto gram = [&](const double* L, const double* Wv, int kk, std::vector<double>* out) -> int {
    const int npairs = kk * (kk + 1) / 2;
    std::vector<double> G(npairs);
    HIP_OK(gpb::pc_gram(L, Wv, n, kk, s->d_pcpart, s->d_vifq, st));
    HIP_OK(hipMemcpyAsync(G.data(), s->d_vifq, sizeof(double) * npairs, hipMemcpyDeviceToHost, st));
    HIP_OK(hipStreamSynchronize(st));
    out->resize((size_t)kk * kk);
    sm::sym_from_packed(G.data(), kk, out->data());
    return 0;
  };
  const size_t nk = (size_t)n * k;
  if (nk > 2000000000u) return fail("full-scale Vecchia gradient: n x k too large");
  // ---- sigma_woodbury_grad (:5437-5448): dSm + C' S_deriv C + Q' dC + dC' Q, Q = S C ----
  const std::vector<double>& G = s->vif_G;
  vg->Mg[0].resize((size_t)k * k);
  for (size_t e = 0; e < vg->Mg[0].size(); ++e) vg->Mg[0][e] = vg->dSm[0][e] + G[e];              // -G + 2 G
  {
    HIP_OK(gpb::lap_scatter(s->d_dD, s->d_sigma, n, dDs, st));
    HIP_OK(gpb::pc_mul3(dDs, wD, wD, n, wDD, st));                                                   // dD / D^2
    // B_grad C = -dA C: the sparse product of the factor kernels with A := dA gives C - dA C (Vecchia order), packed to storage order
    HIP_OK(gpb::launch_vif_spmm(s->d_dA, h->d_nn, 0, n, m, kq, h->d_vC, h->d_vX1, nullptr, nullptr, st));
    HIP_OK(gpb::pc_pack_rows(h->d_vX1, kq, s->d_sigma, n, k, T1, nullptr, st));
    HIP_OK(gpb::lap_lincomb(T1, T1, s->d_vifC, 1.0, -1.0, (int)nk, st));                             // T1 = B_grad C
    std::vector<double> g1, g2, g3, g4, g5;
    HIP_OK(gpb::lap_lincomb(T2, T1, s->d_vifBC, 1.0, 1.0, (int)nk, st));
    if (gram(T2, wD, k, &g1) || gram(T1, wD, k, &g2)) return -1;                                     // S + S' = g1 - g2 - G,  S = (B_grad C)' D^-1 (B C)
    HIP_OK(gpb::lap_lincomb(T2, s->d_vifBC, s->d_vifBdC, 1.0, 1.0, (int)nk, st));
    if (gram(T2, wD, k, &g3) || gram(s->d_vifBdC, wD, k, &g4)) return -1;                            // Q' dC + dC' Q = g3 - g4 - G
    if (gram(s->d_vifBC, wDD, k, &g5)) return -1;                                                     // (B C)' D^-1 dD D^-1 (B C)
    vg->Mg[1].resize((size_t)k * k);
    for (size_t e = 0; e < vg->Mg[1].size(); ++e) vg->Mg[1][e] = vg->dSm[1][e] + (g1[e] - g2[e] - G[e]) - g5[e] + (g3[e] - g4[e] - G[e]);
  }
  // ---- the preconditioner: derivative of its diagonal (:5478-5486), sigma_woodbury_grad_preconditioner (:5490-5498) ----
  {
    std::vector<double> Sip(kp2), M2(kp2);
    sm::spd_inverse_from_tri(s->pc_Linv.data(), kp, Sip.data());
    std::vector<double> Gp, ga, gb, gc;
    if (gram(s->d_pcL, s->d_pcwp, kp, &Gp)) return -1;
    for (int p = 0; p < 2; ++p) {
      sm::matmul(Sip.data(), vg->dSmp[p].data(), kp, tmp.data()); sm::matmul(tmp.data(), Sip.data(), kp, M2.data());
      HIP_OK(hipMemcpyAsync(s->d_vifq, Sip.data(), sizeof(double) * Sip.size(), hipMemcpyHostToDevice, st));
      HIP_OK(hipMemcpyAsync(s->d_vifq + (size_t)kp * kp, M2.data(), sizeof(double) * M2.size(), hipMemcpyHostToDevice, st));
      HIP_OK(gpb::pc_row_quad(s->d_pcL, p == 0 ? s->d_pcL : s->d_pcdL, s->d_vifq, s->d_vifq + (size_t)kp * kp, n, kp, vg->dSmp[p][0], vg->d_dgrad[p], st));
      HIP_OK(gpb::pc_mul3(s->d_pcwp, s->d_pcwp, vg->d_dgrad[p], n, wtmp, st));                       // D^-1 dgrad D^-1
      HIP_OK(gpb::lap_coldots(vg->d_dgrad[p], vg->d_dgrad[p], s->d_pcwp, n, 1, 1, s->d_o + 6, st));     // sum dgrad wp
      HIP_OK(hipMemcpyAsync(s->h_o + 6, s->d_o + 6, sizeof(double) * 2, hipMemcpyDeviceToHost, st));
      HIP_OK(hipStreamSynchronize(st));                                                              // (also: the host matrices just uploaded may go)
      vg->sum_dgrad_wp[p] = s->h_o[6];
      if (gram(s->d_pcL, wtmp, kp, &gc)) return -1;
      vg->Mgp[p].resize((size_t)kp * kp);
      if (p == 0) { for (size_t e = 0; e < gc.size(); ++e) vg->Mgp[0][e] = vg->dSmp[0][e] + 2.0 * Gp[e] - gc[e]; }
      else {
        const size_t nkp = (size_t)n * kp;
        HIP_OK(gpb::lap_lincomb(T2, s->d_pcL, s->d_pcdL, 1.0, 1.0, (int)nkp, st));
        if (gram(T2, s->d_pcwp, kp, &ga) || gram(s->d_pcdL, s->d_pcwp, kp, &gb)) return -1;
        for (size_t e = 0; e < gc.size(); ++e) vg->Mgp[1][e] = vg->dSmp[1][e] + (ga[e] - Gp[e] - gb[e]) - gc[e];
      }
    }
  }
  return 0;
}
// k-vectors of the stochastic parts: L' X for L in {C, dC} (x U, P^-1 Z) and {C_p, dC_p} (x P^-1 Z); sum_i dgrad_i (P^-1 Z)_ic^2.  T: one block of scratch.
int vif_grad_block_sums(gpb_hip_vecchia_t* h, LaplaceState* s, VifGradHost* vg, const double* U, const double* PIZ, double* T, const double* /*dDs*/, int tch, int nc, hipStream_t st) {
  const int n = h->n, k = vg->k, kp = vg->kp, tc = tch * nc;
  if (vif_small(s, n, std::max(k, kp), tch, nc)) return -1;
  auto ltx = [&](const double* L, const double* Ik, int kk, const double* X, std::vector<double>* out) -> int {
    out->resize((size_t)tch * kk * nc);
    HIP_OK(gpb::pc_ltwx(L, s->d_vifones, Ik, X, n, kk, tch, nc, s->d_pcpart, s->d_vifx2, st));
    HIP_OK(hipMemcpyAsync(out->data(), s->d_vifx2, sizeof(double) * out->size(), hipMemcpyDeviceToHost, st));
    HIP_OK(hipStreamSynchronize(st));
    return 0;
  };
  const double* Ik = s->d_vifI + (size_t)k * k;
  if (ltx(s->d_vifC, Ik, k, U, &vg->CU) || ltx(s->d_vifdC, Ik, k, U, &vg->dCU) || ltx(s->d_vifC, Ik, k, PIZ, &vg->CP) || ltx(s->d_vifdC, Ik, k, PIZ, &vg->dCP)) return -1;
  if (ltx(s->d_pcL, s->d_pcI, kp, PIZ, &vg->CpP) || ltx(s->d_pcdL, s->d_pcI, kp, PIZ, &vg->dCpP)) return -1;
  for (int p = 0; p < 2; ++p) {
    vg->wn[p].resize((size_t)2 * tc);
    HIP_OK(gpb::pc_rowscale(PIZ, vg->d_dgrad[p], n, tch, nc, 0, T, st));
    HIP_OK(gpb::lap_coldots(PIZ, PIZ, T, n, tch, nc, s->d_vifq, st));
    HIP_OK(hipMemcpyAsync(vg->wn[p].data(), s->d_vifq, sizeof(double) * (size_t)2 * tc, hipMemcpyDeviceToHost, st));
    HIP_OK(hipStreamSynchronize(st));
  }
  return 0;
}
// C' / dC' times the four n-vectors Q4 = (S0 mode, S0 sv, S1 mode, S1 sv)
int vif_grad_vec_sums(gpb_hip_vecchia_t* h, LaplaceState* s, VifGradHost* vg, const double* Q4, hipStream_t st) {
  const int n = h->n, k = vg->k;
  if (vif_small(s, n, k, 4, 1)) return -1;
  const double* Ik = s->d_vifI + (size_t)k * k;
  vg->yC.resize((size_t)4 * k); vg->ydC.resize((size_t)4 * k);
  HIP_OK(gpb::pc_ltwx(s->d_vifC, s->d_vifones, Ik, Q4, n, k, 4, 1, s->d_pcpart, s->d_vifx2, st));
  HIP_OK(hipMemcpyAsync(vg->yC.data(), s->d_vifx2, sizeof(double) * (size_t)4 * k, hipMemcpyDeviceToHost, st));
  HIP_OK(hipStreamSynchronize(st));
  HIP_OK(gpb::pc_ltwx(s->d_vifdC, s->d_vifones, Ik, Q4, n, k, 4, 1, s->d_pcpart, s->d_vifx2, st));
  HIP_OK(hipMemcpyAsync(vg->ydC.data(), s->d_vifx2, sizeof(double) * (size_t)4 * k, hipMemcpyDeviceToHost, st));
  HIP_OK(hipStreamSynchronize(st));
  return 0;
}
// One block solve of the predictive variances: X += (Sigma^-1 + W)^-1 R for the right-hand sides in w.R by preconditioned CG ('vadu', the solver of the mode finding), the cnt
// leading columns iterated until each residual norm is below tol; the tridiagonal entries are not recorded.  *total_it grows by the steps taken.
int lap_pred_solve(const LapSolver& op, const LapWork& w, double* X, int cnt, int cg_max_num_it, double tol, const char* what, int* total_it) {
  const LapScratch scr{ w.T, w.T, nullptr, nullptr };
  if (op.precond(w.R, w.Z, scr, w.tch, w.NCB)) return -1;
  HIP_OK(hipMemcpyAsync(w.H, w.Z, sizeof(double) * w.nb, hipMemcpyDeviceToDevice, op.st));
  if (lap_cg_reset(w, op.st)) return -1;
  const int p = std::min(cg_max_num_it, op.n);
  int it = 0;
  const int end = lap_cg(op, scr, X, w.R, w.Z, w.H, w.Vb, w.tch, w.NCB, w.sct_plain(), LapCgRule{ p, tol, cnt, true, 1, false }, &it);
  *total_it += it;
  if (end == LAP_CG_ERROR) return -1;
  if (end == LAP_CG_NONFINITE) return fail("NaN or Inf occurred in the conjugate gradient algorithm (%s)", what);
  if (end == LAP_CG_CAP) return fail("the conjugate gradient algorithm of the predictive variances has not converged after %d iterations (residual norm above %g)", p, tol);
  return 0;
}
// Quadratic forms b_p' (Sigma^-1 + W)^-1 b_q of the rows b_p = -A_p of Bpo (prediction points conditioning on observed points) at the state the
// last laplace_eval left behind -- the mode, W / rdw at the mode, this factor in the level-ordered layouts: the part of the predictive (co)variance
// of the latent process that PredictLaplaceApproxVecchia (likelihoods.h:8563-8824) adds to Dp.  The reference's "cholesky" branch computes it
// exactly (:8783-8821); its "iterative" branch estimates it with nsim_var_pred random vectors (:8637-8745, ~10 % scatter at 1000 vectors).  Here:
// the EXACT value by preconditioned CG ('vadu', the solver of the mode finding) on blocks of right-hand sides Bpo' e_p in the probe block's
// layout -- one block of tc columns per tc prediction points, every column iterated until its residual norm is below tol.
//   nn_p / A_p: device, n_pred x m (Vecchia positions of the neighbours, -1 padded; the factor rows).  quad_host: n_pred, or n_pred x n_pred
//   (row-major; want_cov).  iters_host (optional): CG iterations summed over the blocks.
int laplace_pred_quad(gpb_hip_vecchia_t* h, int n_pred, int m, const int* nn_p, const double* A_p, int cg_max_num_it, double tol, bool want_cov,
                      double* quad_host, int* iters_host) {
  LaplaceState* s = h->lap;
  if (!s || !s->has_mode || !s->d_blk || !s->d_vec || !s->d_sc) return fail("predictive variances need the state of a likelihood evaluation (mode, information, factor)");
  HIP_OK(hipSetDevice(h->device));
  const int n = h->n;
  hipStream_t st = h->stream;
  const LapWork w = lap_work(h, s, s->t);
  const int NCB = w.NCB, tch = w.tch, tc = w.tc;
  const size_t nb = w.nb;
  if (s->gblk_cap < nb) {
    dev_free(s->d_gblk); s->gblk_cap = 0;
    HIP_OK(hipMalloc(&s->d_gblk, sizeof(double) * 2 * nb));
    s->gblk_cap = 2 * nb;
  }
  s->grad_state = false; s->gvec_state = false;          // U / PI_Z of the log-determinant are overwritten
  double* X = s->d_gblk;
  const LapSolver op = lap_solver(h, s, w, LapForm::kVadu);
  const size_t out_cap = want_cov ? (size_t)n_pred * tc : (size_t)tc;
  DevBuf<double> d_out;
  HIP_OK(d_out.alloc(out_cap));
  std::vector<double> out(out_cap);
  int total_it = 0;
  for (int p0 = 0; p0 < n_pred; p0 += tc) {
    const int cnt = std::min(tc, n_pred - p0);
    HIP_OK(hipMemsetAsync(w.R, 0, sizeof(double) * nb, st));
    HIP_OK(hipMemsetAsync(X, 0, sizeof(double) * nb, st));
    HIP_OK(gpb::lap_pred_rhs(nn_p, A_p, s->d_sigma, n, m, p0, cnt, tch, NCB, w.R, st));
    if (lap_pred_solve(op, w, X, cnt, cg_max_num_it, tol, "predictive variances", &total_it)) return -1;
    if (want_cov) {
      HIP_OK(gpb::lap_pred_quad(nn_p, A_p, s->d_sigma, X, n, m, 0, n_pred, cnt, NCB, 0, d_out, st));
      HIP_OK(hipMemcpyAsync(out.data(), d_out, sizeof(double) * (size_t)n_pred * cnt, hipMemcpyDeviceToHost, st));
      HIP_OK(hipStreamSynchronize(st));
      for (int r = 0; r < n_pred; ++r) for (int c = 0; c < cnt; ++c) quad_host[(size_t)r * n_pred + p0 + c] = out[(size_t)r * cnt + c];
    } else {
      HIP_OK(gpb::lap_pred_quad(nn_p, A_p, s->d_sigma, X, n, m, p0, cnt, cnt, NCB, 1, d_out, st));
      HIP_OK(hipMemcpyAsync(out.data(), d_out, sizeof(double) * (size_t)cnt, hipMemcpyDeviceToHost, st));
      HIP_OK(hipStreamSynchronize(st));
      for (int c = 0; c < cnt; ++c) quad_host[p0 + c] = out[c];
    }
  }
  if (lap_check_solves(s, st)) return -1;
  if (iters_host) *iters_host = total_it;
  return 0;
}
}  // namespace

// Prediction of the latent process of a full-scale Vecchia model with a NON-GAUSSIAN likelihood at new locations, 'order_obs_first_cond_obs_only' (PredictLaplaceApproxFSVA,
// likelihoods.h:7999-8535) at the state the last evaluation left behind (mode, information, the residual process's factor at the same covariance parameters):
//   mean_p = -Bpo s + C_p Sigma_m^-1 Q' s,   s = mode - C M^-1 Q' mode  (:8049-8057; Q = B'D^-1B C, M the Woodbury matrix)
//   var_p  = Dp + b_p' K^-1 b_p + |V_p|^2 - a_p' G2 a_p + a_p' G2 M2^-1 G2 a_p + 2 a_p' m3_p - 2 (M2^-1 G2 a_p)' m3_p + m3_p' M2^-1 m3_p       (the EXACT expression of the
//            reference's Cholesky branch, :8455-8527; its iterative branch estimates the same by simulation)
//   with K = B'D^-1B + W, b_p the row of Bpo, a_p = Sigma_m^-1 C_p', V_p = L_m^-1 C_p', X = K^-1 W C (n x k: k right-hand sides through the block CG of the predictive variances),
//   G2 = Q' X = C' W (C - X), M2 = Sigma_m + G2, m3_p = b_p' X.
int vif_laplace_predict_impl(gpb_hip_vecchia_t* h, int32_t n_pred, const double* coords_pred_colmajor, int32_t num_neighbors_pred, int cov_type, double var, double a,
                             int cg_max_num_it, double tol, double* pred_mean, double* pred_var, double* pred_cov, int* has_duplicates, int* cg_iterations, bool cond_all) {
  LaplaceState* s = h ? h->lap : nullptr;
  if (!h || !pred_mean || !coords_pred_colmajor) return fail("null argument");
  if (h->vif_k < 1) return fail("gpb_hip_vecchia_vif_laplace_predict: the handle has no inducing points (full-scale Vecchia models only)");
  if (!s || !s->has_mode || !s->d_vec || !s->d_blk || !s->d_sc || !h->has_factor) return fail("predictions need the state of a likelihood evaluation (mode, information, factor)");
  HIP_OK(hipSetDevice(h->device));
  const int n = h->n, k = h->vif_k, kq = h->vif_kq;
  hipStream_t st = h->stream;
  const LapWork w = lap_work(h, s, s->t);
  const int NCB = w.NCB, tch = w.tch, tc = w.tc;
  const size_t nb = w.nb, vb = w.vb;
  double *mode = w.mode, *W = w.W, *Bm = w.Bm, *dir = w.dir;
  const LapSolver op = lap_solver(h, s, w, LapForm::kVadu);
  const gpb::LapLevels& lv = op.lv;
  s->grad_state = false; s->gvec_state = false;
  if (!s->d_vifC) { HIP_OK(hipMalloc(&s->d_vifC, sizeof(double) * (size_t)n * k)); }
  HIP_OK(gpb::pc_pack_rows(h->d_vC, kq, s->d_sigma, n, k, s->d_vifC, nullptr, st));
  // ---- s = mode - C M^-1 Q' mode, Q' s ----
  std::vector<double> w0(k), y1(k), low(k);
  HIP_OK(gpb::lap_B(lv, n, mode, Bm, 1, 1, st));
  if (vif_qf_enqueue(s, n, Bm, 0, st)) return -1;
  HIP_OK(hipStreamSynchronize(st));
  std::copy(s->h_vk, s->h_vk + k, w0.begin());
  sm::cholesky_solve(s->vif_cholM.data(), k, k, w0.data());
  if (vif_small(s, n, k, 1, 1)) return -1;
  HIP_OK(hipMemcpyAsync(s->d_vifx2, w0.data(), sizeof(double) * (size_t)k, hipMemcpyHostToDevice, st));
  HIP_OK(gpb::pc_combine(s->d_vifC, s->d_vifones, mode, s->d_vifx2, n, k, 1, 1, 1, dir, st));          // s (storage order)
  HIP_OK(hipStreamSynchronize(st));
  HIP_OK(gpb::lap_B(lv, n, dir, Bm, 1, 1, st));
  if (vif_qf_enqueue(s, n, Bm, 1, st)) return -1;
  std::vector<double> sim_s(n), sim_v(n);
  HIP_OK(hipMemcpyAsync(sim_s.data(), dir, vb, hipMemcpyDeviceToHost, st));
  HIP_OK(hipStreamSynchronize(st));
  for (int q = 0; q < k; ++q) y1[q] = s->h_vk[(size_t)k + q];
  apply_linv_sym(s->vif_Linv, k, y1.data(), low.data());                                             // Sigma_m^-1 Q' s
  for (int i = 0; i < n; ++i) sim_v[i] = sim_s[s->sigma[i]];
  // ---- the appended rows: neighbours among the observed points, the residual process's factor rows (latent), C_p ----
  if (gpb_hip_vecchia_set_y(h, sim_v.data())) return -1;                                              // the "response" of the appended factor rows: u_p = -A_p s_nn
  TempVecchia tmp; int m = 0;
  if (cond_all && n_pred > 5000) return fail("full-scale Vecchia prediction, 'latent_order_obs_first_cond_all': %d > 5000 prediction points (dense B_p^-1)", n_pred);
  PredictOpts o; o.cond_all = cond_all; o.latent = true; o.factor = false;
  if (predict_factor_appended(h, n_pred, coords_pred_colmajor, num_neighbors_pred, o, cov_type, var, a, &tmp, &m, has_duplicates)) return -1;
  gpb_hip_vecchia_t* tp = tmp.get();
  const int n_obs = n;
  std::vector<double> ipc((size_t)k * h->d);
  for (int j = 0; j < k; ++j) for (int c = 0; c < h->d; ++c) ipc[(size_t)c * k + j] = h->vif_ip_host[(size_t)j * 3 + c];
  if (gpb_hip_vecchia_vif_set_inducing_points(tp, k, ipc.data()) || vif_resid_factor(tp, n_obs, s->vif_Linv.data(), cov_type, var, a, true, nullptr)) return -1;
  std::vector<double> up(n_pred), Dp(n_pred), Cp((size_t)n_pred * k);
  if (copy_factor_rows(tp, n_obs, n_pred, true, nullptr, nullptr, Dp.data(), up.data())) return -1;
  HIP_OK(hipMemcpy2DAsync(Cp.data(), sizeof(double) * (size_t)k, tp->d_vC + (size_t)n_obs * kq, sizeof(double) * (size_t)kq, sizeof(double) * (size_t)k, (size_t)n_pred,
                          hipMemcpyDeviceToHost, tp->stream));
  HIP_OK(hipStreamSynchronize(tp->stream));
  if (tp->m != m) return fail("internal: the appended factor has %d columns, %d neighbours were used", tp->m, m);
  // rows b_p of the operator that maps the observed latent values to the prediction points (minus sign): B_po ('cond_obs_only') or B_p^-1 B_po ('cond_all': the prediction points
  // condition on the preceding prediction points too, B_p = I - A_pp unit lower triangular; likelihoods.h:8052-8056, :8477-8483), and the prior part D_p or B_p^-1 D_p B_p^-T
  const int* nn_p = tp->d_nn + (size_t)n_obs * m;
  const double* A_p = tp->d_A + (size_t)n_obs * m;
  int mrow = m;
  DevBuf<int> d_cols; DevBuf<double> d_negv;
  std::vector<double> Rm;                                  // rows of B_p^-1 ('cond_all')
  std::vector<double> xmean(up);                           // B_p^-1 (B_po s)
  if (cond_all) {
    std::vector<int32_t> nnh((size_t)n_pred * m);
    std::vector<double> Ah((size_t)n_pred * m);
    if (copy_factor_rows(tp, n_obs, n_pred, false, nnh.data(), Ah.data(), nullptr, nullptr)) return -1;
    Rm.assign((size_t)n_pred * n_pred, 0.0);
    std::vector<std::vector<std::pair<int, double>>> Crow(n_pred);
    std::vector<double> acc(n_obs, 0.0); std::vector<char> seen(n_obs, 0); std::vector<int> touched;
    for (int r = 0; r < n_pred; ++r) {
      double* Rk = Rm.data() + (size_t)r * n_pred;
      Rk[r] = 1.0;
      double xm = up[r];
      for (int j = 0; j < m; ++j) {
        const int c = nnh[(size_t)r * m + j];
        if (c < n_obs) continue;
        if (c >= n_obs + r) return fail("prediction point %d has neighbour %d that does not precede it", r, c - n_obs);
        const double av = Ah[(size_t)r * m + j];
        const double* Rj = Rm.data() + (size_t)(c - n_obs) * n_pred;
        for (int q = 0; q <= c - n_obs; ++q) Rk[q] += av * Rj[q];         // row_r(B_p^-1) = e_r + sum_j A_rj row_j(B_p^-1)
        xm += av * xmean[c - n_obs];                                      // forward substitution of B_p x = B_po s
      }
      xmean[r] = xm;
      touched.clear();
      for (int q = 0; q <= r; ++q) {
        const double rq = Rk[q];
        if (rq == 0.0) continue;
        for (int j = 0; j < m; ++j) {
          const int c = nnh[(size_t)q * m + j];
          if (c < 0 || c >= n_obs) continue;
          if (!seen[c]) { seen[c] = 1; touched.push_back(c); }
          acc[c] += rq * (-Ah[(size_t)q * m + j]);                        // B_po = -A_po
        }
      }
      std::sort(touched.begin(), touched.end());
      for (int c : touched) { Crow[r].emplace_back(c, acc[c]); acc[c] = 0.0; seen[c] = 0; }
    }
    size_t mmax = 1;
    for (int r = 0; r < n_pred; ++r) mmax = std::max(mmax, Crow[r].size());
    mrow = (int)mmax;
    std::vector<int32_t> cols((size_t)n_pred * mmax, -1);
    std::vector<double> negv((size_t)n_pred * mmax, 0.0);
    for (int r = 0; r < n_pred; ++r) for (size_t e = 0; e < Crow[r].size(); ++e) { cols[(size_t)r * mmax + e] = Crow[r][e].first; negv[(size_t)r * mmax + e] = -Crow[r][e].second; }     // (the kernels take A with b = -A)
    HIP_OK(d_cols.alloc(cols.size()));
    HIP_OK(d_negv.alloc(negv.size()));
    HIP_OK(hipMemcpy(d_cols, cols.data(), sizeof(int) * cols.size(), hipMemcpyHostToDevice));
    HIP_OK(hipMemcpy(d_negv, negv.data(), sizeof(double) * negv.size(), hipMemcpyHostToDevice));
    nn_p = d_cols; A_p = d_negv;
  }
  for (int r = 0; r < n_pred; ++r) {
    double acc = -xmean[r];
    for (int q = 0; q < k; ++q) acc += Cp[(size_t)r * k + q] * low[q];
    pred_mean[r] = acc;
  }
  if (cg_iterations) *cg_iterations = 0;
  if (!pred_var && !pred_cov) return 0;
  const int m_rows = mrow;
  // ---- b_p' K^-1 b_p: the Vecchia path's quadratic forms (K = B'D^-1B + W of THIS factor) ----
  const bool want_cov = pred_cov != nullptr;
  std::vector<double> qd(want_cov ? (size_t)n_pred * n_pred : (size_t)n_pred);
  int it1 = 0;
  if (laplace_pred_quad(h, n_pred, m_rows, nn_p, A_p, cg_max_num_it, tol, want_cov, qd.data(), &it1)) return -1;
  // ---- X = K^-1 W C in blocks of tc columns: G2 = C' W (C - X), M3 = Bpo X ----
  double* X = s->d_gblk;                                   // (sized by laplace_pred_quad)
  if (vif_small(s, n, k, std::max(tch, k), NCB)) return -1;
  std::vector<double> G2((size_t)k * k), M3((size_t)n_pred * k), blk((size_t)tch * k * NCB), outp((size_t)n_pred * tc), Gc(k * (k + 1) / 2);
  DevBuf<double> d_outp;
  HIP_OK(d_outp.alloc((size_t)n_pred * tc));
  HIP_OK(gpb::pc_gram(s->d_vifC, W, n, k, s->d_pcpart, s->d_vifx2, st));                               // C' W C
  HIP_OK(hipMemcpyAsync(Gc.data(), s->d_vifx2, sizeof(double) * Gc.size(), hipMemcpyDeviceToHost, st));
  HIP_OK(hipStreamSynchronize(st));
  int total_it = it1;
  for (int col0 = 0; col0 < k; col0 += tc) {
    const int cnt = std::min(tc, k - col0);
    HIP_OK(gpb::pc_cols_to_block(s->d_vifC, W, n, k, col0, cnt, tch, NCB, w.R, st));
    HIP_OK(hipMemsetAsync(X, 0, sizeof(double) * nb, st));
    if (lap_pred_solve(op, w, X, cnt, cg_max_num_it, tol, "predictive variances, full-scale Vecchia", &total_it)) return -1;
    HIP_OK(gpb::pc_ltwx(s->d_vifC, W, s->d_vifI + (size_t)k * k, X, n, k, tch, NCB, s->d_pcpart, s->d_vifx2, st));      // C' W X
    HIP_OK(hipMemcpyAsync(blk.data(), s->d_vifx2, sizeof(double) * blk.size(), hipMemcpyDeviceToHost, st));
    HIP_OK(gpb::lap_pred_quad(nn_p, A_p, s->d_sigma, X, n, m_rows, 0, n_pred, cnt, NCB, 0, d_outp, st));                   // Bpo X (or B_p^-1 Bpo X)
    HIP_OK(hipMemcpyAsync(outp.data(), d_outp, sizeof(double) * (size_t)n_pred * cnt, hipMemcpyDeviceToHost, st));
    HIP_OK(hipStreamSynchronize(st));
    for (int c = 0; c < cnt; ++c) {
      for (int q = 0; q < k; ++q) {
        const double cwc = Gc[(size_t)std::max(q, col0 + c) * (std::max(q, col0 + c) + 1) / 2 + std::min(q, col0 + c)];
        G2[(size_t)q * k + col0 + c] = cwc - blk[((size_t)(c / NCB) * k + q) * NCB + (c % NCB)];
      }
      for (int r = 0; r < n_pred; ++r) M3[(size_t)r * k + col0 + c] = outp[(size_t)r * cnt + c];
    }
  }
  if (lap_check_solves(s, st)) return -1;
  if (cg_iterations) *cg_iterations = total_it;
  // ---- host: k x k algebra per prediction point ----
  std::vector<double> M2((size_t)k * k);
  for (int p = 0; p < k; ++p) for (int q = 0; q < k; ++q) M2[(size_t)p * k + q] = s->vif_Sm[(size_t)p * k + q] + 0.5 * (G2[(size_t)p * k + q] + G2[(size_t)q * k + p]);
  double ld2 = 0.0;
  if (!spd_invert(M2, k, &ld2)) return fail("Laplace prediction Woodbury matrix: not positive definite");      // CheckCholeskyFactorization, likelihoods.h:8463
  std::vector<double> ap(k), vp(k), m1(k), m2(k), m4(k);
  // (covariance matrix, :8489-8504: the same terms between two prediction points -- the per-point k-vectors are kept)
  std::vector<double> APm, VPm, M1m, M2m, M4m;
  if (want_cov) { APm.resize((size_t)n_pred * k); VPm.resize((size_t)n_pred * k); M1m.resize((size_t)n_pred * k); M2m.resize((size_t)n_pred * k); M4m.resize((size_t)n_pred * k); }
  for (int r = 0; r < n_pred; ++r) {
    const double* c = Cp.data() + (size_t)r * k;
    const double* m3 = M3.data() + (size_t)r * k;
    apply_linv_sym(s->vif_Linv, k, c, ap.data());                                                     // Sigma_m^-1 C_p'
    double v2 = 0.0;
    for (int i = 0; i < k; ++i) { double acc = 0.0; for (int q = 0; q <= i; ++q) acc += s->vif_Linv[(size_t)i * k + q] * c[q]; vp[i] = acc; v2 += acc * acc; }      // |L_m^-1 C_p'|^2
    for (int q = 0; q < k; ++q) { double acc = 0.0; for (int i = 0; i < k; ++i) acc += ap[i] * 0.5 * (G2[(size_t)i * k + q] + G2[(size_t)q * k + i]); m1[q] = acc; }     // M_aux_1 row
    for (int q = 0; q < k; ++q) { double acc = 0.0, acc4 = 0.0; for (int i = 0; i < k; ++i) { acc += M2[(size_t)q * k + i] * m1[i]; acc4 += M2[(size_t)q * k + i] * m3[i]; } m2[q] = acc; m4[q] = acc4; }
    double d_am1 = 0., d_m2m1 = 0., d_am3 = 0., d_m2m3 = 0., d_m4m3 = 0.;
    for (int q = 0; q < k; ++q) { d_am1 += ap[q] * m1[q]; d_m2m1 += m2[q] * m1[q]; d_am3 += ap[q] * m3[q]; d_m2m3 += m2[q] * m3[q]; d_m4m3 += m4[q] * m3[q]; }
    double prior = Dp[r];
    if (cond_all) { prior = 0.0; for (int j = 0; j <= r; ++j) prior += Rm[(size_t)r * n_pred + j] * Dp[j] * Rm[(size_t)r * n_pred + j]; }      // (B_p^-1 D_p B_p^-T)_rr
    const double vr = prior + (want_cov ? qd[(size_t)r * n_pred + r] : qd[r]) + v2 - d_am1 + d_m2m1 + 2.0 * d_am3 - 2.0 * d_m2m3 + d_m4m3;
    if (pred_var) pred_var[r] = vr;
    if (want_cov) for (int q = 0; q < k; ++q) { APm[(size_t)r * k + q] = ap[q]; VPm[(size_t)r * k + q] = vp[q]; M1m[(size_t)r * k + q] = m1[q]; M2m[(size_t)r * k + q] = m2[q]; M4m[(size_t)r * k + q] = m4[q]; }
  }
  if (want_cov) {
    auto dotk = [&](const std::vector<double>& A_, int i, const std::vector<double>& B_, int j) { double acc = 0.0; for (int q = 0; q < k; ++q) acc += A_[(size_t)i * k + q] * B_[(size_t)j * k + q]; return acc; };
    for (int i = 0; i < n_pred; ++i)
      for (int j = 0; j <= i; ++j) {
        const double qij = 0.5 * (qd[(size_t)i * n_pred + j] + qd[(size_t)j * n_pred + i]);
        double prior = (i == j ? Dp[i] : 0.0);
        if (cond_all) { prior = 0.0; for (int q = 0; q <= j; ++q) prior += Rm[(size_t)i * n_pred + q] * Dp[q] * Rm[(size_t)j * n_pred + q]; }
        const double v = prior + qij + dotk(VPm, i, VPm, j) - 0.5 * (dotk(M1m, i, APm, j) + dotk(M1m, j, APm, i)) + 0.5 * (dotk(M1m, i, M2m, j) + dotk(M1m, j, M2m, i))
                         + dotk(M3, i, APm, j) + dotk(APm, i, M3, j) - dotk(M3, i, M2m, j) - dotk(M2m, i, M3, j) + 0.5 * (dotk(M3, i, M4m, j) + dotk(M3, j, M4m, i));
        pred_cov[(size_t)i * n_pred + j] = pred_cov[(size_t)j * n_pred + i] = v;
      }
  }
  return 0;
}

extern "C" {

// Latent prediction of a non-Gaussian (Vecchia-Laplace) model at new locations, 'latent_order_obs_first_cond_obs_only': mean = -Bpo mode
// (likelihoods.h:8600-8602), variance = Dp + b_p' (Sigma^-1 + W)^-1 b_p, covariance the same with the off-diagonal forms (:8783-8821, the value the
// reference's "cholesky" branch computes).  Needs: the mode as the handle's "response" (gpb_hip_vecchia_set_y(mode)) and the state of the
// likelihood evaluation that found it.  pred_var (n_pred) / pred_cov (n_pred x n_pred, row-major) may be NULL.
int gpb_hip_vecchia_laplace_predict(gpb_hip_vecchia_t* h, int32_t n_pred, const double* coords_pred_colmajor, int32_t num_neighbors_pred,
                                    int cov_type, double var, double a, int cg_max_num_it, double tol, double* pred_mean, double* pred_var,
                                    double* pred_cov, int* has_duplicates, int* cg_iterations) {
  API_BEGIN();
  if (h && h->vif_k > 0) return fail("gpb_hip_vecchia_laplace_predict: full-scale Vecchia handles take gpb_hip_vecchia_vif_laplace_predict / the evaluation and gradient entry points; this one restates the plain Vecchia formulas");
  if (!pred_mean) return fail("null argument");
  TempVecchia t; int m = 0;
  PredictOpts o; o.latent = true;
  if (predict_factor_appended(h, n_pred, coords_pred_colmajor, num_neighbors_pred, o, cov_type, var, a, &t, &m, has_duplicates)) return -1;
  const int n_obs = h->n;
  std::vector<double> u(n_pred), Dp(n_pred);
  if (copy_factor_rows(t.get(), n_obs, n_pred, false, nullptr, nullptr, nullptr, u.data())) return -1;
  for (int k = 0; k < n_pred; ++k) pred_mean[k] = -u[k];
  if (cg_iterations) *cg_iterations = 0;
  if (pred_var || pred_cov) {
    if (t->m != m) return fail("internal: the appended factor has %d columns, %d neighbours were used", t->m, m);
    if (copy_factor_rows(t.get(), n_obs, n_pred, false, nullptr, nullptr, Dp.data(), nullptr)) return -1;
    HIP_OK(hipStreamSynchronize(t->stream));
    const bool cov = pred_cov != nullptr;
    std::vector<double> q(cov ? (size_t)n_pred * n_pred : (size_t)n_pred);
    if (laplace_pred_quad(h, n_pred, m, t->d_nn + (size_t)n_obs * m, t->d_A + (size_t)n_obs * m, cg_max_num_it, tol, cov, q.data(), cg_iterations)) return -1;
    if (cov) {
      for (int r = 0; r < n_pred; ++r) for (int c = 0; c < n_pred; ++c) pred_cov[(size_t)r * n_pred + c] = 0.5 * (q[(size_t)r * n_pred + c] + q[(size_t)c * n_pred + r]) + (r == c ? Dp[r] : 0.0);
      if (pred_var) for (int k = 0; k < n_pred; ++k) pred_var[k] = pred_cov[(size_t)k * n_pred + k];
    } else {
      for (int k = 0; k < n_pred; ++k) pred_var[k] = Dp[k] + q[k];
    }
  }
  API_END();
}

// Quadratic forms c_r' (Sigma^-1 + W)^-1 c_s of sparse rows handed over by the host (n_rows x mmax: Vecchia positions, -1 padded, and values) at the state
// of the last evaluation: the general form of the block solves of the predictive variances -- rows of Bp^-1 Bpo for prediction points that condition
// on each other ('latent_order_obs_first_cond_all', PredictLaplaceApproxVecchia with CondObsOnly = false, likelihoods.h:8790-8821).
// out_host: n_rows values (the diagonal), or n_rows x n_rows row-major (want_cov).
int gpb_hip_vecchia_vif_laplace_predict(gpb_hip_vecchia_t* h, int32_t n_pred, const double* coords_pred_colmajor, int32_t num_neighbors_pred, int cov_type, double var, double a,
                                        int cg_max_num_it, double tol, double* pred_mean, double* pred_var, double* pred_cov, int* has_duplicates, int* cg_iterations) {
  API_BEGIN();
  if (vif_laplace_predict_impl(h, n_pred, coords_pred_colmajor, num_neighbors_pred < 0 ? -num_neighbors_pred : num_neighbors_pred, cov_type, var, a, cg_max_num_it, tol, pred_mean, pred_var,
                               pred_cov, has_duplicates, cg_iterations, num_neighbors_pred < 0)) return -1;
  API_END();
}
int gpb_hip_vecchia_laplace_quad_forms(gpb_hip_vecchia_t* h, int32_t n_rows, int32_t mmax, const int32_t* cols_host, const double* vals_host, int cg_max_num_it,
                                       double tol, int want_cov, double* out_host, int* cg_iterations) {
  API_BEGIN();
  if (h && h->vif_k > 0) return fail("gpb_hip_vecchia_laplace_quad_forms: full-scale Vecchia handles take gpb_hip_vecchia_vif_laplace_predict / the evaluation and gradient entry points; this one restates the plain Vecchia formulas");
  if (!h || !cols_host || !vals_host || !out_host || n_rows < 1 || mmax < 1) return fail("invalid argument");
  HIP_OK(hipSetDevice(h->device));
  const size_t cnt = (size_t)n_rows * mmax;
  for (size_t k = 0; k < cnt; ++k) if (cols_host[k] >= h->n) return fail("gpb_hip_vecchia_laplace_quad_forms: column %d of a handle with %d points", cols_host[k], h->n);
  std::vector<double> neg(cnt);
  for (size_t k = 0; k < cnt; ++k) neg[k] = -vals_host[k];                      // the kernels take A_p with b_p = -A_p
  DevBuf<int> d_cols; DevBuf<double> d_neg;
  HIP_OK(d_cols.alloc(cnt));
  HIP_OK(d_neg.alloc(cnt));
  HIP_OK(hipMemcpy(d_cols, cols_host, sizeof(int) * cnt, hipMemcpyHostToDevice));
  HIP_OK(hipMemcpy(d_neg, neg.data(), sizeof(double) * cnt, hipMemcpyHostToDevice));
  if (laplace_pred_quad(h, n_rows, mmax, d_cols, d_neg, cg_max_num_it, tol, want_cov != 0, out_host, cg_iterations)) return -1;
  if (want_cov)
    for (int r = 0; r < n_rows; ++r) for (int c = 0; c < r; ++c) {
      const double v = 0.5 * (out_host[(size_t)r * n_rows + c] + out_host[(size_t)c * n_rows + r]);
      out_host[(size_t)r * n_rows + c] = out_host[(size_t)c * n_rows + r] = v;
    }
  API_END();
}

// diag((Sigma^-1 + W)^-1) at the mode, Vecchia order: the variances of the latent process at the TRAINING locations
// (Likelihood::CalcVarLaplaceApproxVecchia behind GPB_PredictREModelTrainingDataRandomEffects, re_model_template.h:4683-4725) -- exact, with the
// block solves of the predictive variances on the unit vectors (n / 52 block solves: meant for moderate n; the caller bounds it).
int gpb_hip_vecchia_laplace_mode_var(gpb_hip_vecchia_t* h, int cg_max_num_it, double tol, double* var_host, int* cg_iterations) {
  API_BEGIN();
  if (h && h->vif_k > 0) return fail("gpb_hip_vecchia_laplace_mode_var: full-scale Vecchia handles take gpb_hip_vecchia_vif_laplace_predict / the evaluation and gradient entry points; this one restates the plain Vecchia formulas");
  if (!h || !var_host) return fail("null argument");
  const int n = h->n;
  HIP_OK(hipSetDevice(h->device));
  std::vector<int> idx(n);
  std::iota(idx.begin(), idx.end(), 0);
  std::vector<double> minus_one((size_t)n, -1.0);                // b_i = -A_i = e_i
  DevBuf<int> d_idx; DevBuf<double> d_coef;
  HIP_OK(d_idx.alloc((size_t)n));
  HIP_OK(d_coef.alloc((size_t)n));
  HIP_OK(hipMemcpy(d_idx, idx.data(), sizeof(int) * (size_t)n, hipMemcpyHostToDevice));
  HIP_OK(hipMemcpy(d_coef, minus_one.data(), sizeof(double) * (size_t)n, hipMemcpyHostToDevice));
  if (laplace_pred_quad(h, n, 1, d_idx, d_coef, cg_max_num_it, tol, false, var_host, cg_iterations)) return -1;
  API_END();
}

int gpb_hip_vecchia_laplace_logit(gpb_hip_vecchia_t* h, int cov_type, double var, double a, int num_rand_vec, int seed_rand_vec,
                                  int cg_max_num_it, int cg_max_num_it_tridiag, double cg_delta_conv, double delta_conv_mode_finding,
                                  int reset_mode, double* out9_host, double* mode_host) {
  API_BEGIN();
  if (laplace_eval(h, cov_type, var, a, num_rand_vec, seed_rand_vec, cg_max_num_it, cg_max_num_it_tridiag, cg_delta_conv,
                   delta_conv_mode_finding, reset_mode ? LAP_RESET_MODE : 0, out9_host, mode_host)) return -1;
  API_END();
}
// Evaluation that can be followed by the gradient (keep_grad_state) / gradient of the current state / the mode bookkeeping of the
// optimiser (include/gpb_hip.h).
int gpb_hip_vecchia_laplace_eval(gpb_hip_vecchia_t* h, int cov_type, double var, double a, int num_rand_vec, int seed_rand_vec,
                                 int cg_max_num_it, int cg_max_num_it_tridiag, double cg_delta_conv, double delta_conv_mode_finding,
                                 int reset_mode, int keep_grad_state, double* out9_host, double* mode_host) {
  API_BEGIN();
  if (laplace_eval(h, cov_type, var, a, num_rand_vec, seed_rand_vec, cg_max_num_it, cg_max_num_it_tridiag, cg_delta_conv,
                   delta_conv_mode_finding, (reset_mode ? LAP_RESET_MODE : 0) | (keep_grad_state ? LAP_KEEP_GRAD_STATE : 0), out9_host, mode_host)) return -1;
  API_END();
}

int gpb_hip_vecchia_laplace_reset_mode_to_previous(gpb_hip_vecchia_t* h) {
  API_BEGIN();
  if (!h || !h->lap || !h->lap->d_gvec || !h->lap->d_vec) return fail("no mode has been found yet");
  HIP_OK(hipSetDevice(h->device));
  LaplaceState* s = h->lap;
  HIP_OK(hipMemcpyAsync(s->d_vec, s->d_gvec, sizeof(double) * (size_t)h->n, hipMemcpyDeviceToDevice, h->stream));   // likelihoods.h:997-1004
  HIP_OK(hipStreamSynchronize(h->stream));
  s->grad_state = false; s->gvec_state = false;
  s->has_mode = true;          // a failed mode finding (NaN) is followed by this reset: the next one warm-starts from the restored mode
  API_END();
}

int gpb_hip_vecchia_laplace_get_aux_pars(gpb_hip_vecchia_t* h, double* aux_out, int32_t* num_aux) {
  API_BEGIN();
  if (!h || !num_aux) return fail("null argument");
  *num_aux = h->lap ? gpb::lik_num_aux(h->lap->link) : 0;
  if (aux_out && *num_aux) aux_out[0] = h->lap->aux;
  if (aux_out && *num_aux == 2) aux_out[1] = h->lap->aux2;
  API_END();
}

// test seam: dA / d log(range) and dD / d log(range) of the factor without nugget at (var, a), Vecchia order (checked against
// orc_vecchia_factor's A_grad / D_grad)
int gpb_hip_vecchia_laplace_range_deriv(gpb_hip_vecchia_t* h, int cov_type, double var, double a, double* dA_host, double* dD_host) {
  API_BEGIN();
  if (!h || !dA_host || !dD_host) return fail("null argument");
  HIP_OK(hipSetDevice(h->device));
  const int n = h->n, m = h->m;
  if (h->i_begin != 0 || h->i_end != n) return fail("the Vecchia-Laplace path needs the whole factor on one device");
  if (alloc_factor(h)) return -1;
  if (lap_launch_factor(h, cov_type, var, a, 0)) return -1;
  h->has_factor = true;
  if (h->lap) h->lap->grad_state = false;
  DevBuf<double> dA, dD;
  HIP_OK(dA.alloc((size_t)n * m));
  HIP_OK(dD.alloc((size_t)n));
  if (m > 126) return fail("gpb_hip_vecchia_laplace_range_deriv: at most 126 neighbours (this model has %d)", m);
  if (h->d > 3) return fail("gpb_hip_vecchia_laplace_range_deriv: coordinate dimensions 1..3 (this model has %d)", h->d);
  hipError_t e = gpb::lap_range_deriv(h->d_pts, h->d_nn, h->d_A, n, m, cov_type, h->d == 3 ? 1 : 0, var, a, dA, dD, h->stream);
  if (e == hipSuccess) e = hipMemcpyAsync(dA_host, dA, sizeof(double) * (size_t)n * m, hipMemcpyDeviceToHost, h->stream);
  if (e == hipSuccess) e = hipMemcpyAsync(dD_host, dD, sizeof(double) * (size_t)n, hipMemcpyDeviceToHost, h->stream);
  if (e == hipSuccess) e = hipStreamSynchronize(h->stream);
  if (e != hipSuccess) return fail("HIP error: %s", hipGetErrorString(e));
  API_END();
}

}  // extern "C"

// The gradient half: gpb_hip_vecchia_laplace_grad_current in stages, the gradients wrt F and the auxiliary parameters, the standard errors of a Gaussian Vecchia model.
#include "gpb_laplace_grad.inc"
