// gpboost_amd/csrc/tree_predict_kernels.hip -- which leaf does a binned row fall into, and the score update of a range of trees.
//
// Stands in for Tree::AddPredictionToScore on binned data (src/LightGBM/io/tree.cpp:147, :226) with Tree::DecisionInner
// (include/LightGBM/tree.h:349-409) per node, as GBDT::UpdateScore needs it for out-of-bag rows and validation sets
// (src/LightGBM/boosting/gbdt.cpp:606-623, score_updater.hpp:93-96, :118-122).
//
// Per node the decision is a function of the row's STORED bin of the node's column only, so the host compiles every node into a 256-bit
// set of stored bins that go left (gpb_hip_hist_node_go_left_mask: the partition kernels' rule) and the walk has no missing-type or
// categorical branches:  b = row[col]; left = (set[b >> 5] >> (b & 31)) & 1; node = left ? left_child : right_child;  until node < 0.
//
// Mapping: one lane per row.  A workgroup stages the padded rows of its lanes in LDS once (16-byte pieces, coalesced for consecutive rows,
// one 64-byte sector per row of a row list at fpad = 64; row stride fpad + 4 bytes, so that the lanes' byte reads of one column fall on
// 32 different banks at fpad = 64), then applies the trees chunk by chunk: the stored forms of the chunk's trees are copied to LDS
// together, every lane walks every tree of the chunk and adds the leaf's value to its row's score IN TREE ORDER, in a register; the score
// is read and written once.  Chunks are formed inside the kernel by the rule of tree_predict_kernels.h, so the result does not depend on
// them, and a row's bins come from HBM once per call however many trees are applied.
// A walk takes at most num_leaves - 1 steps whatever the tables hold (they are validated by the host when a tree is stored).
#include "tree_predict_kernels.h"

namespace gpb {

namespace {

__global__ __launch_bounds__(256) void tree_predict_kernel(TreePredictArgs a) {
  extern __shared__ __attribute__((aligned(16))) unsigned char s_raw[];
  const int R = blockDim.x, tid = threadIdx.x;
  const int rstride = a.fpad + 4;
  uint32_t* s_trees = reinterpret_cast<uint32_t*>(s_raw);                          // [lds_tree_bytes]
  int* s_rows = reinterpret_cast<int*>(s_raw + a.lds_tree_bytes);                  // [R]
  unsigned char* s_bins = s_raw + a.lds_tree_bytes + R * 4;                        // [R][rstride]
  const int base = blockIdx.x * R;
  const int nrows = min(R, a.cnt - base);
  const int i = base + tid;
  const bool live = tid < nrows;
  const int row = live ? (a.rows ? a.rows[i] : i) : 0;
  s_rows[tid] = row;
  __syncthreads();
  const int ppr = a.fpad >> 4;                                                     // 16-byte pieces per row
  for (int p = tid; p < nrows * ppr; p += R) {
    const int r = p / ppr, part = p - r * ppr;
    const uint4 v = *reinterpret_cast<const uint4*>(a.bins_rm + (size_t)s_rows[r] * a.fpad + part * 16);
    uint32_t* d = reinterpret_cast<uint32_t*>(s_bins + r * rstride + part * 16);
    d[0] = v.x; d[1] = v.y; d[2] = v.z; d[3] = v.w;
  }
  const unsigned char* my_bins = s_bins + tid * rstride;
  double s = (a.score && live) ? a.score[row] : 0.0;
  const int reps = (a.mult && live) ? a.mult[i] : 1;
  int t = a.tree_begin;
  while (t < a.tree_end) {
    const int c0 = t, w0 = a.desc[c0].x;
    int bytes = 0;
    while (t < a.tree_end) {                                                       // the chunk rule of tree_predict_kernels.h
      const int b = a.desc[t].z;
      if (t > c0 && bytes + b > GPB_TP_CHUNK_BYTES) break;
      bytes += b; ++t;
    }
    bytes = min(bytes, a.lds_tree_bytes);
    __syncthreads();                                                               // the walks of the previous chunk (first chunk: the staging) are done
    const uint4* src = reinterpret_cast<const uint4*>(a.forest + w0);
    for (int q = tid; q < (bytes >> 4); q += R) reinterpret_cast<uint4*>(s_trees)[q] = src[q];
    __syncthreads();
    for (int tt = c0; tt < t; ++tt) {
      const int4 d = a.desc[tt];
      const int nl = d.y;
      const uint32_t* nodes = s_trees + (d.x - w0);
      const double* vals = reinterpret_cast<const double*>(nodes + (nl - 1) * GPB_TP_NODE_WORDS);
      int node = (live && nl > 1) ? 0 : -1;                                        // (a tree of one leaf has no nodes: leaf 0)
      for (int step = 1; step < nl && node >= 0; ++step) {
        const uint32_t* nd = nodes + node * GPB_TP_NODE_WORDS;
        const int4 m = *reinterpret_cast<const int4*>(nd + 8);                     // {column, left child, right child, 0}
        const unsigned b = my_bins[m.x];
        node = ((nd[b >> 5] >> (b & 31u)) & 1u) ? m.y : m.z;
      }
      if (!live) continue;
      if (a.score) {
        if (node < 0) {
          const double v = vals[~node];
          for (int j = 0; j < reps; ++j) s = s + v;
        }
      } else {
        a.leaf_out[i] = node < 0 ? ~node : -1;
      }
    }
  }
  if (a.score && live) a.score[row] = s;
}

}  // namespace

hipError_t launch_tree_predict(const TreePredictArgs& a, hipStream_t st) {
  if (a.cnt <= 0 || a.tree_begin >= a.tree_end) return hipSuccess;
  if (a.fpad < 16 || (a.fpad & 15) || a.fpad > GPB_TP_MAX_FPAD || a.lds_tree_bytes < 0 || a.lds_tree_bytes > GPB_TP_CHUNK_BYTES || (a.lds_tree_bytes & 15))
    return hipErrorInvalidValue;
  const int R = a.fpad <= GPB_TP_WIDE_FPAD ? 256 : 64;
  const size_t lds = (size_t)a.lds_tree_bytes + (size_t)R * 4 + (size_t)R * (a.fpad + 4);
  hipLaunchKernelGGL(tree_predict_kernel, dim3((a.cnt + R - 1) / R), dim3(R), lds, st, a);
  return hipGetLastError();
}

}  // namespace gpb
