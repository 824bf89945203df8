// gpboost_amd/csrc/tree_shap_kernels.hip -- per-feature contributions (TreeSHAP) of a range of stored trees to binned rows.
//
// Stands in for Tree::PredictContrib -> the recursive Tree::TreeSHAP on raw values (src/LightGBM/io/tree.cpp:827-998) on binned data.  The recursion is
// gone: the host compiles every leaf's root-to-leaf path into its DISTINCT columns (tree_shap_kernels.h: per element the column, the 256-bit set of stored
// bins that keep a row on the path at every node of that column, and the zero fraction = the product of count(child) / count(node) over those nodes) --
// the reference's unique path with repeated features already merged (its UnwindPath-then-re-extend yields the same products, and the permutation weights do
// not depend on the order of the elements).  A row's one fraction of an element is 1 when its stored bin of the column is in the set, else 0.  Per
// (row, leaf of E elements, leaf value v), with D = E and element 0 the reference's root placeholder (zero = one = 1):
//   extend  (ExtendPath)      pw[0] = 1;  for d = 1 .. E:  new pw[k] = z_d pw[k] (d - k) / (d + 1) + one_d pw[k - 1] k / (d + 1),  k = d .. 0
//   unwind  (UnwoundPathSum)  one_e = 1:  n = pw[D]; for i = D - 1 .. 0: t = n (D + 1) / (i + 1); w += t; n = pw[i] - t z_e (D - i) / (D + 1)
//                             one_e = 0:  w = (1 / z_e) sum_i pw[i] (D + 1) / (D - i)
//   out[row][column_e] += w (one_e - z_e) v
// and out[row][F] += the tree's expected value.  The quotients of small integers come from a table and 1 / z_e from the path table, so the kernel divides
// nowhere; both unwind recurrences run in one loop over the shared pw[i] and the lane keeps the one its one fraction selects (no divergence).
//
// Mapping: one lane owns a row for the whole call.  A workgroup stages the padded rows of its lanes in LDS once (the row-staging idea of
// tree_predict_kernels.hip: 16-byte pieces, row stride fpad + 4 bytes), keeps the permutation weights in LDS as [index][lane] (a lane's column is private:
// no barrier after the staging; consecutive lanes read consecutive doubles) and adds to its row's entries of out in global memory, strictly in
// (tree, leaf, element) order onto the running value: the entry is loaded before the unwind loop and stored after it, so its latency hides behind the loop.
// Nothing depends on the other rows of the call, on the rows per workgroup or on how a range of trees is split over calls; there are no atomics, no
// spin-waits and no hand-off between workgroups.  Trees, leaves and elements are the same for all lanes, so every path-table and ratio-table address is
// wave-uniform (scalar loads).  All loops are bounded by table sizes the host has validated (and clamped to max_unique once more here).
#include "tree_shap_kernels.h"

namespace gpb {

namespace {

__global__ __launch_bounds__(256) void tree_shap_kernel(const uint8_t* __restrict__ bins_rm, const int* __restrict__ rows, const uint32_t* __restrict__ tables,
                                                        const int4* __restrict__ desc, const double* __restrict__ ratio, double* __restrict__ out, int fpad, int F,
                                                        int cnt, int tree_begin, int tree_end, int max_unique) {
  extern __shared__ __attribute__((aligned(16))) unsigned char s_raw[];
  const int R = blockDim.x, tid = threadIdx.x;
  const int rstride = fpad + 4;
  double* s_pw = reinterpret_cast<double*>(s_raw);                                 // [max_unique + 1][R]
  int* s_rows = reinterpret_cast<int*>(s_raw + (size_t)(max_unique + 1) * R * 8);  // [R]
  unsigned char* s_bins = reinterpret_cast<unsigned char*>(s_rows + R);            // [R][rstride]
  const int base = blockIdx.x * R;
  const int nrows = min(R, cnt - base);
  const bool live = tid < nrows;
  const int row = live ? (rows ? rows[base + tid] : base + tid) : 0;
  s_rows[tid] = row;
  __syncthreads();
  const int ppr = fpad >> 4;                                                       // 16-byte pieces per row
  for (int p = tid; p < nrows * ppr; p += R) {
    const int r = p / ppr, part = p - r * ppr;
    const uint4 v = *reinterpret_cast<const uint4*>(bins_rm + (size_t)s_rows[r] * fpad + part * 16);
    uint32_t* d = reinterpret_cast<uint32_t*>(s_bins + r * rstride + part * 16);
    d[0] = v.x; d[1] = v.y; d[2] = v.z; d[3] = v.w;
  }
  __syncthreads();
  const unsigned char* my_bins = s_bins + tid * rstride;                           // (a lane without a row reads unstaged bytes: its results are never stored)
  double* pw = s_pw + tid;                                                         // pw[k * R]
  double* my_out = out + (size_t)row * (size_t)(F + 1);
  const double* inv_all = ratio + GPB_SHAP_RATIO_ENTRIES;
  for (int t = tree_begin; t < tree_end; ++t) {
    const int4 td = desc[t];
    const uint32_t* tb = tables + td.x;
    const int nl = td.y;
    const double ev = *reinterpret_cast<const double*>(tb);
    const double* vals = reinterpret_cast<const double*>(tb + 4);
    const int* first = reinterpret_cast<const int*>(tb + 4 + 2 * nl);
    const uint32_t* elems = tb + 4 + 2 * nl + (nl + 1 + 3) / 4 * 4;
    for (int leaf = 0; leaf < nl && nl > 1; ++leaf) {
      const int e0 = first[leaf];
      const int E = min(first[leaf + 1] - e0, max_unique);
      const double v = vals[leaf];
      const uint32_t* el = elems + (size_t)e0 * GPB_SHAP_ELEM_WORDS;
      // the row's one fractions (bit d - 1: element d) and the permutation weights of the whole path
      unsigned obits = 0u;
      pw[0] = 1.0;
      for (int d = 1; d <= E; ++d) {
        const uint32_t* e = el + (d - 1) * GPB_SHAP_ELEM_WORDS;
        const unsigned b = my_bins[e[8]];
        const unsigned wi = b >> 5;
        unsigned word = 0u;
#pragma unroll
        for (unsigned j = 0; j < 8; ++j) word = wi == j ? e[j] : word;
        const bool one = ((word >> (b & 31u)) & 1u) != 0u;
        obits |= (one ? 1u : 0u) << (d - 1);
        const double z = *reinterpret_cast<const double*>(e + 12);
        const double* fr = ratio + d * GPB_SHAP_RATIO_STRIDE;
        double hi = 0.0;                                                           // the old pw[k] (pw[d] = 0 before the step)
        for (int k = d; k >= 1; --k) {
          const double lo = pw[(k - 1) * R];
          pw[k * R] = hi * (z * fr[d - k]) + (one ? lo * fr[k] : 0.0);
          hi = lo;
        }
        pw[0] = hi * (z * fr[d]);
      }
      const double* fr = ratio + E * GPB_SHAP_RATIO_STRIDE;
      const double* iv = inv_all + E * GPB_SHAP_RATIO_STRIDE;
      for (int ei = 1; ei <= E; ++ei) {
        const uint32_t* e = el + (ei - 1) * GPB_SHAP_ELEM_WORDS;
        const int col = (int)e[8];
        const double z = *reinterpret_cast<const double*>(e + 12), invz = *reinterpret_cast<const double*>(e + 14);
        const bool one = ((obits >> (ei - 1)) & 1u) != 0u;
        const double cur = live ? my_out[col] : 0.0;
        double next_one = pw[E * R], tot1 = 0.0, tot0 = 0.0;
        for (int i = E - 1; i >= 0; --i) {
          const double p = pw[i * R];
          const double tmp = next_one * iv[i + 1];
          tot1 = tot1 + tmp;
          next_one = p - tmp * (z * fr[E - i]);
          tot0 = tot0 + p * iv[E - i];
        }
        const double w = one ? tot1 : tot0 * invz;
        const double x = w * ((one ? 1.0 : 0.0) - z) * v;
        if (live) my_out[col] = cur + x;
      }
    }
    if (live) my_out[F] = my_out[F] + ev;
  }
}

}  // namespace

hipError_t launch_tree_shap(const TreeShapArgs& a, hipStream_t st) {
  if (a.cnt <= 0 || a.tree_begin >= a.tree_end) return hipSuccess;
  if (a.fpad < 16 || (a.fpad & 15) || a.F < 1 || a.F > a.fpad || a.max_unique < 0 || a.max_unique > GPB_SHAP_MAX_UNIQUE) return hipErrorInvalidValue;
  const int R = tree_shap_rows_per_block(a.fpad, a.max_unique);
  if (R == 0) return hipErrorInvalidValue;
  const size_t lds = (size_t)R * (4 + (size_t)a.fpad + 4 + 8 * ((size_t)a.max_unique + 1));
  hipLaunchKernelGGL(tree_shap_kernel, dim3((a.cnt + R - 1) / R), dim3(R), lds, st, a.bins_rm, a.rows, a.tables, a.desc, a.ratio, a.out, a.fpad, a.F, a.cnt,
                     a.tree_begin, a.tree_end, a.max_unique);
  return hipGetLastError();
}

}  // namespace gpb
