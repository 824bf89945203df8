// gpboost_amd/csrc/tree_raw_kernels.hip -- which leaf does a row of raw feature values fall into, and the score update of a range of trees.
//
// Stands in for Tree::AddPredictionToScore / Tree::GetLeaf on feature VALUES (src/LightGBM/io/tree.cpp, include/LightGBM/tree.h:418, :545-560) with
// Tree::Decision per node (tree.h:329-401): real-valued thresholds, a missing type and a default direction per node, a bitset over category values.  The rows
// need no binning: the matrix is row-major float64 or float32 as the caller holds it (NaN, zero-as-missing and categorical semantics of the reference).
//
// Mapping: one lane per row.  A workgroup stages the rows of its lanes in LDS once per call, IN THE MATRIX'S OWN TYPE (float32 rows take half the LDS): along
// every row consecutive lanes load consecutive 16-byte pieces, aligned to 16 bytes in memory whatever the row's own alignment (the pieces that straddle the ends
// of a row are loaded element by element, so nothing outside a row is read), gathered through the row list when there is one.  A staged row takes F | 1 elements:
// an odd number of 8-byte (float32: 4-byte) words, so that the lanes' reads of one column fall on different banks.  Then the trees are applied chunk by chunk as in
// tree_predict_kernels.hip: the raw forms of a chunk's trees are copied to LDS together, every lane walks every tree of the chunk and adds the leaf's value to
// its row's score IN TREE ORDER, in a register, one plain addition per tree (and per occurrence of the row); the score is read once and written once.  Chunks are
// formed inside the kernel by the greedy rule of tree_raw_kernels.h, so the result does not depend on them.  No atomics, no waiting, no hand-off between workgroups.
// A walk takes at most num_leaves - 1 steps whatever the tables hold (they are validated by the host when a rule is stored).
//
// One step is the reference's rule in plain double arithmetic (this file is compiled without contraction and without fast-math):
//   x = (double)row[column]                                   exact for float32
//   numerical:    if (isnan(x) && mt != NaN) x = 0
//                 if ((mt == Zero && -kZeroThreshold <= x <= kZeroThreshold) || (mt == NaN && isnan(x))) go the default way
//                 else go x <= threshold ? left : right       kZeroThreshold = 1e-35f promoted to double (include/LightGBM/meta.h:56)
//   categorical:  NaN: right if mt == NaN, else c = 0;  a value outside [-2^31, 2^31): right (the reference's static_cast<int> is undefined there);
//                 c = (int)x, c < 0: right;  left iff c < 32 * words and bit c of the node's set is on (Common::FindInBitset)
#include "tree_raw_kernels.h"

namespace gpb {

namespace {

template <typename T> struct RawPiece;
template <> struct RawPiece<double> { using V = double2; static constexpr int N = 2; };
template <> struct RawPiece<float> { using V = float4; static constexpr int N = 4; };

template <typename T>
__global__ __launch_bounds__(256) void tree_raw_kernel(TreeRawArgs a) {
  extern __shared__ __attribute__((aligned(16))) unsigned char s_raw[];
  constexpr int EPP = RawPiece<T>::N;                                              // elements per 16-byte piece
  const int R = blockDim.x, tid = threadIdx.x;
  const int F = a.F, lstride = F | 1;
  const uint32_t* s_trees = reinterpret_cast<const uint32_t*>(s_raw);              // [lds_tree_bytes]
  int* s_rows = reinterpret_cast<int*>(s_raw + a.lds_tree_bytes);                  // [R]
  T* s_x = reinterpret_cast<T*>(s_raw + a.lds_tree_bytes + R * 4);                 // [R][lstride]
  const T* x = static_cast<const T*>(a.x);
  const int base = blockIdx.x * R;
  const int nrows = min(R, a.cnt - base);
  const int i = base + tid;
  const bool live = tid < nrows;
  const int row = live ? (a.rows ? a.rows[i] : i) : 0;
  s_rows[tid] = row;
  __syncthreads();
  // a row of F elements that starts `mis` elements behind a 16-byte boundary is covered by at most (F + EPP - 1) / EPP + 1 aligned pieces
  const int ppr = (F + EPP - 1) / EPP + 1;
  for (int p = tid; p < nrows * ppr; p += R) {
    const int r = p / ppr, part = p - r * ppr;
    const T* src = x + (size_t)s_rows[r] * (size_t)a.row_stride;
    const int mis = (int)((reinterpret_cast<uintptr_t>(src) / sizeof(T)) & (uintptr_t)(EPP - 1));
    const int e = part * EPP - mis;                                                // first element of the piece, relative to the row
    T* dst = s_x + r * lstride;
    if (e >= 0 && e + EPP <= F) {
      const typename RawPiece<T>::V v = *reinterpret_cast<const typename RawPiece<T>::V*>(src + e);
      const T* ve = reinterpret_cast<const T*>(&v);
#pragma unroll
      for (int k = 0; k < EPP; ++k) dst[e + k] = ve[k];
    } else {
#pragma unroll
      for (int k = 0; k < EPP; ++k)
        if (e + k >= 0 && e + k < F) dst[e + k] = src[e + k];
    }
  }
  const T* my_x = s_x + tid * lstride;
  const double kzero = (double)1e-35f;
  double s = (a.score && live) ? a.score[row] : 0.0;
  const int reps = (a.mult && live) ? a.mult[i] : 1;
  int t = a.tree_begin;
  while (t < a.tree_end) {
    const int c0 = t, w0 = a.desc[c0].x;
    int bytes = 0;
    while (t < a.tree_end) {                                                       // the chunk rule of tree_raw_kernels.h
      const int4 d = a.desc[t];
      if (t > c0 && (bytes + d.z > GPB_TR_CHUNK_BYTES || d.x != w0 + (bytes >> 2))) break;
      bytes += d.z; ++t;
    }
    bytes = min(bytes, a.lds_tree_bytes);
    __syncthreads();                                                               // the walks of the previous chunk (first chunk: the staging) are done
    const uint4* src = reinterpret_cast<const uint4*>(a.forest + w0);
    for (int q = tid; q < (bytes >> 4); q += R) reinterpret_cast<uint4*>(s_raw)[q] = src[q];
    __syncthreads();
    for (int tt = c0; tt < t; ++tt) {
      const int4 d = a.desc[tt];
      const int nl = d.y;
      const uint32_t* tree = s_trees + (d.x - w0);
      const uint32_t* sets = tree + (nl - 1) * (GPB_TR_NODE_BYTES / 4);
      const double* vals = reinterpret_cast<const double*>(sets + d.w);
      int node = (live && nl > 1) ? 0 : -1;                                        // (a tree of one leaf has no nodes: leaf 0)
      for (int step = 1; step < nl && node >= 0; ++step) {
        const uint32_t* nd = tree + node * (GPB_TR_NODE_BYTES / 4);
        const int4 lo = *reinterpret_cast<const int4*>(nd);                        // {threshold (two words), column, left child}
        const int2 hi = *reinterpret_cast<const int2*>(nd + 4);                    // {right child, flags_and_cat}
        const double thr = __hiloint2double(lo.y, lo.x);
        const int flags = hi.y, mt = flags & 3;
        double v = (double)my_x[lo.z];
        const bool nan = isnan(v);
        bool left;
        if (!(flags & GPB_TR_FLAG_CATEGORICAL)) {
          if (nan && mt != 2) v = 0.0;
          if ((mt == 1 && v >= -kzero && v <= kzero) || (mt == 2 && nan)) left = (flags & GPB_TR_FLAG_DEFAULT_LEFT) != 0;
          else left = v <= thr;
        } else {
          const int words = (flags >> GPB_TR_CAT_WORDS_SHIFT) & GPB_TR_CAT_WORDS_MASK;
          const int first = (int)((unsigned)flags >> GPB_TR_CAT_FIRST_SHIFT);
          int c = -1;                                                              // (negative: right)
          if (nan) c = mt == 2 ? -1 : 0;
          else if (v >= -2147483648.0 && v < 2147483648.0) c = (int)v;
          left = false;
          if (c >= 0 && (c >> 5) < words) left = ((sets[first + (c >> 5)] >> (c & 31)) & 1u) != 0u;
        }
        node = left ? lo.w : hi.x;
      }
      if (!live) continue;
      if (a.score) {
        if (node < 0) {
          const double val = vals[~node];
          for (int j = 0; j < reps; ++j) s = s + val;
        }
      } else {
        a.leaf_out[i] = node < 0 ? ~node : -1;
      }
    }
  }
  if (a.score && live) a.score[row] = s;
}

}  // namespace

hipError_t launch_tree_raw(const TreeRawArgs& a, hipStream_t st) {
  if (a.cnt <= 0 || a.tree_begin >= a.tree_end) return hipSuccess;
  const int eb = a.dtype == 0 ? 8 : 4;
  if ((a.dtype != 0 && a.dtype != 1) || a.F < 1 || a.F > (a.dtype == 0 ? GPB_TR_MAX_COLS_F64 : GPB_TR_MAX_COLS_F32) || a.row_stride < a.F || !a.x ||
      (reinterpret_cast<uintptr_t>(a.x) & (uintptr_t)(eb - 1)) || a.lds_tree_bytes < 0 || a.lds_tree_bytes > GPB_TR_CHUNK_BYTES || (a.lds_tree_bytes & 15))
    return hipErrorInvalidValue;
  const int R = tree_raw_rows_per_block(a.F, eb, a.lds_tree_bytes);
  if (R == 0) return hipErrorInvalidValue;
  const size_t lds = (size_t)a.lds_tree_bytes + (size_t)R * 4 + (size_t)R * tree_raw_lds_stride(a.F) * eb;
  if (a.dtype == 0) hipLaunchKernelGGL(tree_raw_kernel<double>, dim3((a.cnt + R - 1) / R), dim3(R), lds, st, a);
  else hipLaunchKernelGGL(tree_raw_kernel<float>, dim3((a.cnt + R - 1) / R), dim3(R), lds, st, a);
  return hipGetLastError();
}

}  // namespace gpb
