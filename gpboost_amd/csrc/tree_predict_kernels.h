// gpboost_amd/csrc/tree_predict_kernels.h -- launch interface of tree_predict_kernels.hip and the stored form of a tree
#pragma once
#include <hip/hip_runtime.h>
#include <stdint.h>

namespace gpb {

// A stored tree is one contiguous, 16-byte aligned run of 32-bit words in the forest buffer:
//   num_leaves - 1 nodes of GPB_TP_NODE_WORDS words: [0..7] the 256-bit set of STORED bins of the node's column that go left,
//                                                    [8] the column, [9] left child, [10] right child (~leaf for a leaf), [11] 0
//   num_leaves doubles: leaf_value * shrinkage, rounded once on the host (Tree::Shrinkage, include/LightGBM/tree.h:188)
//   padding to a multiple of 16 bytes
#define GPB_TP_NODE_WORDS 12
// The trees of a call are applied in CHUNKS of consecutive trees whose stored forms fit this many bytes of LDS together (greedy, in tree order:
// a chunk is closed by the first tree that would overflow it); a single tree may not be larger (439 leaves).
#define GPB_TP_CHUNK_BYTES 24576
// One lane per row, the rows of a workgroup staged in LDS once per call: 256 rows while a row's padded width is at most GPB_TP_WIDE_FPAD bytes, 64 rows up to
// GPB_TP_MAX_FPAD; wider matrices are refused by the host.
#define GPB_TP_WIDE_FPAD 128
#define GPB_TP_MAX_FPAD 560

inline int tree_predict_tree_bytes(int num_leaves) {
  return (((num_leaves - 1) * GPB_TP_NODE_WORDS * 4 + num_leaves * 8) + 15) / 16 * 16;
}

struct TreePredictArgs {
  const uint8_t* bins_rm;   // [n][fpad] row-major stored bins
  int fpad;
  const int* rows;          // cnt row indices (validated by the host), or nullptr: rows 0 .. cnt - 1
  const int* mult;          // score update of a list with repeats: occurrences of rows[i] (the list is then run-length encoded); nullptr: 1
  int cnt;
  const uint32_t* forest;   // stored trees
  const int4* desc;         // per tree {first word in forest, num_leaves, stored bytes, 0}
  int tree_begin, tree_end;
  double* score;            // score[row] += sum over the trees, in tree order (nullptr: leaf_out is written)
  int* leaf_out;            // leaf_out[i] = leaf of rows[i] in tree tree_begin
  int lds_tree_bytes;       // LDS reserved for tree tables: the largest chunk of [tree_begin, tree_end)
};

hipError_t launch_tree_predict(const TreePredictArgs& a, hipStream_t st);

}  // namespace gpb
