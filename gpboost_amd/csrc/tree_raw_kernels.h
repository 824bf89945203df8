// gpboost_amd/csrc/tree_raw_kernels.h -- launch interface of tree_raw_kernels.hip and the raw form of a stored tree
#pragma once
#include <hip/hip_runtime.h>
#include <stdint.h>

namespace gpb {

// The raw form of a stored tree decides on feature VALUES (Tree::Decision, include/LightGBM/tree.h:329-401), not on bins.  It is one contiguous, 16-byte aligned
// run of 32-bit words in the raw forest buffer:
//   num_leaves - 1 nodes of GPB_TR_NODE_BYTES bytes: {double threshold; int column; int left; int right; int flags_and_cat; 8 bytes of padding}
//                  (children as in the bin form: ~leaf for a leaf); two 16-byte reads
//   the bitset words of its categorical nodes, node after node (bit c of a node's set = category c goes left), padded to an even number of words
//   num_leaves doubles: leaf_value * shrinkage -- the doubles of the bin form, copied
//   padding to a multiple of 16 bytes
#define GPB_TR_NODE_BYTES 32
// flags_and_cat: bits 0-1 the missing type (0 None, 1 Zero, 2 NaN), bit 2 default-left, bit 3 categorical; of a categorical node bits 4-15 the number of words of
// its bitset and bits 16-31 its first word, counted from the tree's first bitset word (both bounded by GPB_TR_CHUNK_BYTES / 4 = 3072)
#define GPB_TR_FLAG_DEFAULT_LEFT 4
#define GPB_TR_FLAG_CATEGORICAL 8
#define GPB_TR_CAT_WORDS_SHIFT 4
#define GPB_TR_CAT_WORDS_MASK 0xfff
#define GPB_TR_CAT_FIRST_SHIFT 16
// The trees of a call are applied in chunks of consecutive trees whose raw forms fit this many bytes of LDS together (the greedy rule of
// tree_predict_kernels.h) AND lie back to back in the buffer (rules may arrive in any order, a chunk is one copy); a single tree may not be larger.  12 KB: a 255-leaf tree (10168 bytes + its bitsets) fits, and next to it 128 rows of 50 doubles
// (128 x (51 x 8 + 4) = 52736 bytes) stay within the 64 KB of a launch.
#define GPB_TR_CHUNK_BYTES 12288
#define GPB_TR_LDS_BYTES 65536
// A staged row takes its columns rounded up to an ODD number of elements; 64 rows, their indices and a full chunk must fit a launch.  Wider matrices are refused.
#define GPB_TR_MAX_ROW_BYTES ((GPB_TR_LDS_BYTES - GPB_TR_CHUNK_BYTES - 64 * 4) / 64)
#define GPB_TR_MAX_COLS_F64 (((GPB_TR_MAX_ROW_BYTES / 8) - 1) | 1)      // 103
#define GPB_TR_MAX_COLS_F32 (((GPB_TR_MAX_ROW_BYTES / 4) - 1) | 1)      // 207

inline int tree_raw_tree_bytes(int num_leaves, int bitset_words) {
  return ((num_leaves - 1) * GPB_TR_NODE_BYTES + (bitset_words + 1) / 2 * 8 + num_leaves * 8 + 15) / 16 * 16;
}
inline int tree_raw_lds_stride(int F) { return F | 1; }                 // elements per staged row
// Rows per workgroup: the largest of 256, 128, 64 for which the rows, their indices and the call's largest chunk fit a launch (0: none does)
inline int tree_raw_rows_per_block(int F, int elem_bytes, int lds_tree_bytes) {
  for (int R = 256; R >= 64; R >>= 1)
    if ((size_t)lds_tree_bytes + (size_t)R * (4 + (size_t)tree_raw_lds_stride(F) * elem_bytes) <= GPB_TR_LDS_BYTES) return R;
  return 0;
}

struct TreeRawArgs {
  const void* x;            // [n][row_stride] row-major feature values, float64 (dtype 0) or float32 (dtype 1)
  int dtype;
  int F;
  long long row_stride;     // in elements, >= F
  const int* rows;          // cnt row indices (validated by the host), or nullptr: rows 0 .. cnt - 1
  const int* mult;          // score update of a list with repeats: occurrences of rows[i] (the list is then run-length encoded); nullptr: 1
  int cnt;
  const uint32_t* forest;   // raw forms
  const int4* desc;         // per tree {first word in forest, num_leaves, stored bytes (0: the tree has no raw form), bitset words padded to even}
  int tree_begin, tree_end;
  double* score;            // score[row] += sum over the trees, in tree order (nullptr: leaf_out is written)
  int* leaf_out;            // leaf_out[i] = leaf of rows[i] in tree tree_begin
  int lds_tree_bytes;       // LDS reserved for trees: the largest chunk of [tree_begin, tree_end)
};

hipError_t launch_tree_raw(const TreeRawArgs& a, hipStream_t st);

}  // namespace gpb
