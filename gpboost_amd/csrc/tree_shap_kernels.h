// gpboost_amd/csrc/tree_shap_kernels.h -- launch interface of tree_shap_kernels.hip and the compiled path table of a stored tree
#pragma once
#include <hip/hip_runtime.h>
#include <stdint.h>

namespace gpb {

// A root-to-leaf path holds at most this many DISTINCT columns (elements); a tree with a longer one gets no path table.  The permutation weights
// lose about two digits per 8 further elements (the algorithm's own conditioning, the reference's too): 2.8e-14 of sum |leaf value| at 24, 3.2e-12 at 32,
// 1.2e-10 at 40 on chains.
#define GPB_SHAP_MAX_UNIQUE 32
// One element of a path: [0..7] the 256-bit set of STORED bins of the column that keep a row on the path at every node of that column,
// [8] the column, [9..11] 0, [12..13] the zero fraction z (double), [14..15] 1 / z (double)
#define GPB_SHAP_ELEM_WORDS 16
// The path table of one tree is one contiguous, 16-byte aligned run of 32-bit words:
//   [0..1] the tree's expected value (double), [2..3] 0
//   num_leaves doubles: the stored leaf values (leaf_value * shrinkage, the words of the stored tree)
//   num_leaves + 1 ints: first element of every leaf (relative to the tree's first element), padded to a multiple of 4 ints
//   elements of GPB_SHAP_ELEM_WORDS words, leaf after leaf, in order of first appearance on the path
inline int tree_shap_first_words(int num_leaves) { return (num_leaves + 1 + 3) / 4 * 4; }
inline size_t tree_shap_table_words(int num_leaves, int num_elements) {
  return 4 + 2 * (size_t)num_leaves + (size_t)tree_shap_first_words(num_leaves) + (size_t)num_elements * GPB_SHAP_ELEM_WORDS;
}
// The ratio tables every launch reads: entry [d * GPB_SHAP_RATIO_STRIDE + k], d = 0 .. GPB_SHAP_MAX_UNIQUE, k = 0 .. d + 1:
//   frac = k / (d + 1)   (ExtendPath's (i + 1) / (unique_depth + 1) and (unique_depth - i) / (unique_depth + 1))
//   inv  = (d + 1) / k   (UnwoundPathSum's quotients; entry k = 0 is 0 and never read)
#define GPB_SHAP_RATIO_STRIDE (GPB_SHAP_MAX_UNIQUE + 2)
#define GPB_SHAP_RATIO_ENTRIES ((GPB_SHAP_MAX_UNIQUE + 1) * GPB_SHAP_RATIO_STRIDE)

// Rows per workgroup: the largest of 256, 128, 64 whose dynamic LDS -- per row 4 bytes of index, fpad + 4 bytes of bins, (max_unique + 1) * 8 bytes of
// permutation weights -- stays at or below 64 KB (0: none does)
inline int tree_shap_rows_per_block(int fpad, int max_unique) {
  for (int R = 256; R >= 64; R >>= 1)
    if ((size_t)R * (4 + (size_t)fpad + 4 + 8 * ((size_t)max_unique + 1)) <= 65536) return R;
  return 0;
}

struct TreeShapArgs {
  const uint8_t* bins_rm;   // [n][fpad] row-major stored bins
  int fpad;
  int F;                    // columns: a row of out has F + 1 entries
  const int* rows;          // cnt DISTINCT row indices (validated by the host), or nullptr: rows 0 .. cnt - 1
  int cnt;
  const uint32_t* tables;   // path tables
  const int4* desc;         // per tree {first word of its table, num_leaves, largest number of elements of a leaf, 1}
  int tree_begin, tree_end;
  const double* ratio;      // frac at [0, GPB_SHAP_RATIO_ENTRIES), inv behind it
  double* out;              // [n][F + 1]
  int max_unique;           // the largest number of elements of a leaf of the trees in the call
};

hipError_t launch_tree_shap(const TreeShapArgs& a, hipStream_t st);

}  // namespace gpb
