// gpboost_amd/csrc/gpb_tree.inc -- included at the end of gpb_hip.cpp.
//
// One regression tree grown leaf-wise on the device-resident primitives of this library, with the row lists of the leaves resident
// too (what DataPartition keeps on the host in the reference).  One split = ONE host synchronisation: partition of the chosen leaf
// (count / scan / scatter into the other one of two row buffers), histogram of the smaller child (which child that is, is decided on
// the device from the partition's counts), and one fused launch for FixHistogram + parent - smaller + the threshold search of both
// children are enqueued back to back; then the left counts and the two candidate sets (2 x F x 10 doubles) come back together.
// (The first version synchronised twice per split and launched fix / subtract / search / search separately: 3.9 ms per 31-leaf tree at
// n = 1e5, of which kernels were 2 ms.)  Control flow restated from
//   SerialTreeLearner::Train                     src/LightGBM/treelearner/serial_tree_learner.cpp:159-210
//   BeforeFindBestSplit                          :283-323   (leaves too small to split, smaller / larger leaf)
//   FindBestSplits / ...FromHistograms           :325-449   (is_splittable inheritance, parent - smaller)
//   SplitInner + DataPartition::Split            :565-690, data_partition.hpp:101-130 (left keeps the leaf id and the front of the segment)
//   SplitInfo::operator>                         split_info.hpp:126-153 (ties: smaller feature index)
//   Tree::Split bookkeeping                      include/LightGBM/tree.h
// for numerical features, the default regularisation path (lambda_l2, min_data_in_leaf, min_sum_hessian_in_leaf,
// min_gain_to_split), no forced splits / constraints / bagging.  tests/tree_harness.py is the same control flow in Python over the
// single-step entry points; both are pinned by the reference's own trees (tests/golden/tree_ref.npz).
//
// Data-parallel form (SURVEY.md 8e; DataParallelTreeLearner, data_parallel_tree_learner.cpp:55-80 root sums, :155-173 histograms,
// :240-260 global leaf counts): when the handle has a communicator (gpb_hip_hist_comm_init / _comm_init_local) every rank holds a shard
// of the rows and the function all-reduces (i) every freshly built leaf histogram before FixHistogram -- as INTEGER fixed-point totals,
// converted once (hist_finish_sharded) --, (ii) the left count of every split; the root's sums and row count are read off the root
// histogram's integer totals (the caller's sum_gradient / sum_hessian are ignored).  All ranks then hold bit-identical histograms and
// counts -- identical, too, for EVERY way of dealing the rows to ranks --, take identical decisions and return the same tree; row
// lists, partitions and data_leaf_index stay local.

namespace {

struct TreeLeafBest { double gain = -INFINITY; int feature = -1; double row[10]; int dl = 0; bool has_row = false;
                      unsigned cat_bits[8] = {0u, 0u, 0u, 0u, 0u, 0u, 0u, 0u}; };      // categorical winner: the set of bins going left

inline bool split_better(double ga, int fa, double gb, int fb) {     // SplitInfo::operator>; feature -1 compares as INT32_MAX
  const long long a = fa >= 0 ? fa : 2147483647LL, b = fb >= 0 ? fb : 2147483647LL;
  return ga != gb ? ga > gb : a < b;
}

}  // namespace

extern "C" int gpb_hip_hist_grow_tree(gpb_hip_hist_t* h, int32_t num_leaves, double sum_gradient, double sum_hessian, double lambda_l2,
                                      int32_t min_data_in_leaf, double min_sum_hessian_in_leaf, double min_gain_to_split, double const_hess,
                                      int32_t* out_num_leaves, int32_t* split_feature_inner, uint32_t* threshold_in_bin, int32_t* default_left,
                                      int32_t* left_child, int32_t* right_child, double* split_gain, int32_t* internal_count,
                                      double* leaf_value, int32_t* leaf_count, int32_t* data_leaf_index) {
  API_BEGIN();
  if (!h || !out_num_leaves || !split_feature_inner || !threshold_in_bin || !default_left || !left_child || !right_child || !split_gain ||
      !internal_count || !leaf_value || !leaf_count)
    return fail("gpb_hip_hist_grow_tree: null argument");
  if (num_leaves < 2) return fail("gpb_hip_hist_grow_tree: num_leaves = %d", num_leaves);
  if (!h->has_grad) return fail("gradients have not been set (call gpb_hip_hist_set_gradients)");
  if (!h->has_fix || !h->has_split_info) return fail("gpb_hip_hist_grow_tree: feature views / metas have not been set (gpb_hip_hist_set_fix_info, gpb_hip_hist_set_split_info)");
  if (h->nslots < num_leaves) return fail("gpb_hip_hist_grow_tree: the histogram pool holds %d slots, %d leaves need %d (gpb_hip_hist_pool_resize)", h->nslots, num_leaves, num_leaves);
  HIP_OK(hipSetDevice(h->device));
  const int n = h->n, F = h->F, L = num_leaves;
  hipStream_t st = h->stream;
  // workspaces: resident row lists, partition scratch, two search result sets (smaller / larger leaf in one sync)
  if (!h->d_rows) HIP_OK(hipMalloc(&h->d_rows, sizeof(int) * (size_t)n));
  if (!h->d_rows2) HIP_OK(hipMalloc(&h->d_rows2, sizeof(int) * (size_t)n));
  if (!h->d_counts) {
    // d_counts: {left rows of this rank, of all ranks, ticket of the search kernel, error word}; h_counts (pinned): {the two counts, the
    // sequence number the kernels of a split leave for the polling host}; d_ptags: the one-pass partition's 256 granules
    HIP_OK(hipMalloc(&h->d_counts, sizeof(int) * 4)); HIP_OK(hipMemset(h->d_counts, 0, sizeof(int) * 4));
    HIP_OK(hipHostMalloc(&h->h_counts, sizeof(int) * 4)); std::memset(h->h_counts, 0, sizeof(int) * 4);
    HIP_OK(hipMalloc(&h->d_ptags, sizeof(unsigned long long) * 256)); HIP_OK(hipMemset(h->d_ptags, 0, sizeof(unsigned long long) * 256));
  }
  const int nblk_max = (n + 1023) / 1024;
  const int need = 2 * (nblk_max + 1) + 3 * n;
  if (h->part_cap < need) { dev_free(h->d_part); HIP_OK(hipMalloc(&h->d_part, sizeof(int) * (size_t)need)); h->part_cap = need; }
  if (!h->d_split2) {
    HIP_OK(hipMalloc(&h->d_split2, sizeof(double) * (size_t)F * 10 * 2));
    HIP_OK(hipMalloc(&h->d_split2_i, sizeof(int) * (size_t)(F + 1) * 2));
    HIP_OK(hipMalloc(&h->d_used2, (size_t)F * 2));
    HIP_OK(hipHostMalloc(&h->h_split2, sizeof(double) * (size_t)F * 10 * 2));
    HIP_OK(hipHostMalloc(&h->h_split2_i, sizeof(int) * (size_t)(F + 1) * 2));
  }
  std::vector<int> begin(L, 0), cnt(L, 0), gcnt(L, 0), slot_of(L, 0), parent_node(L, -1), buf(L, 0);   // cnt: rows of this rank, gcnt: of all ranks; buf: row buffer
  std::vector<char> is_left(L, 1);
  std::vector<double> sg(L, 0.), sh(L, 0.);
  std::vector<TreeLeafBest> best(L);
  std::vector<std::vector<signed char>> splittable(L, std::vector<signed char>(F, 0));
  std::vector<double> lval(L, 0.);
  std::vector<int> depth(L, 0);                    // Tree::leaf_depth_ (root 0)
  int* const rows_buf[2] = {h->d_rows, h->d_rows2};
  h->tree_node_info.clear(); h->tree_node_is_cat.clear(); h->tree_node_cat_bits.clear();
  const bool any_cat = h->any_cat;
  int ncat_nodes = 0;                              // Tree::SplitCategorical numbers the categorical nodes: threshold_in_bin_ = that index (tree.cpp:76-108)
  bool rows_identity = true;                       // until the first split the root's rows are 0..n-1 (no index list)
  // bagging: the root holds the rows of gpb_hip_hist_set_root_rows (DataPartition::Init with used_data_indices_, data_partition.hpp:57-63)
  const int nroot = h->root_cnt > 0 ? h->root_cnt : n;
  if (h->root_cnt > 0) {
    HIP_OK(hipMemcpyAsync(h->d_rows, h->d_root_rows, sizeof(int) * (size_t)nroot, hipMemcpyDeviceToDevice, st));
    rows_identity = false;
  }
  cnt[0] = nroot; gcnt[0] = nroot; sg[0] = sum_gradient; sh[0] = sum_hessian;
  int next_free = 1, nleaves = 1, nnodes = 0;
  const bool dist = h->comm.active();
  // feature-block exchange (round 5): after the root, a freshly built histogram is reduce-SCATTERED by feature block, every rank converts, fixes, subtracts and
  // searches the features it owns, and the ranks' best candidates of the two children are exchanged (one small all-reduce of zero-padded records: a sum whose
  // other terms are zeros is a gather).  The root keeps the all-reduce: its totals also give the job's sums and row count.
  // (auto mode only up to the 16 ranks the exchange records are sized for -- hist_blocks_setup; larger jobs keep the all-reduce instead of failing, ADVICE r05)
  const bool bx = dist && (h->block_exchange > 0 || (h->block_exchange < 0 && h->comm.world <= 16 && (size_t)h->total_bins * (h->has_hess ? 5 : 3) * 8 >= ((size_t)2 << 20)));
  if (bx && hist_blocks_setup(h)) return -1;
  const int own_f0 = bx ? h->blk_f0[h->comm.rank] : 0, own_f1 = bx ? h->blk_f0[h->comm.rank + 1] : F;
  // every feature's view lies inside its own entries (num_bin entries from view_offset when most_freq_bin > 0, one fewer otherwise: offset = 1)?
  // then the search workgroups can work from the build's chunk partials of their feature alone
  bool views_local = !dist;
  for (int f = 0; f < F && views_local; ++f) {
    const int rel = h->h_fix[f] - h->h_bin_offsets[f], ext = h->h_fix[F + f] - (h->h_fix[2 * F + f] == 0 ? 1 : 0);
    if (rel < 0 || rel + ext > h->h_bin_offsets[f + 1] - h->h_bin_offsets[f]) views_local = false;
  }

  // the kernel evaluates every feature; the mask (the parent's is_splittable flags) is applied when the candidates are collected on
  // the host, so nothing is uploaded
  auto search_collect = [&](int leaf, const signed char* used, int which, bool own_only) {
    const double* out = h->h_split2 + (size_t)which * F * 10;
    const int* fl = h->h_split2_i + (size_t)which * (F + 1);
    TreeLeafBest b;
    for (int f = 0; f < F; ++f) {
      if (own_only && (f < own_f0 || f >= own_f1)) { splittable[leaf][f] = 0; continue; }      // another rank's feature: searched there
      splittable[leaf][f] = used[f] ? (signed char)((fl[f] >> 1) & 1) : 0;
      if (!used[f]) continue;
      if (split_better(out[(size_t)f * 10], f, b.gain, b.feature)) {
        b.gain = out[(size_t)f * 10]; b.feature = f; b.dl = fl[f] & 1; b.has_row = true;
        std::copy(out + (size_t)f * 10, out + (size_t)f * 10 + 10, b.row);
        if (any_cat && h->h_is_cat[f]) std::copy(h->h_cat_bits2 + ((size_t)which * F + f) * 8, h->h_cat_bits2 + ((size_t)which * F + f) * 8 + 8, b.cat_bits);
      }
    }
    best[leaf] = b;
  };

  // root: construct + FixHistogram + search
  std::vector<signed char> all_used(F, 1), used(F, 0);
  if ((int)h->feature_mask.size() == F) all_used = h->feature_mask;      // feature_fraction: the tree's sampled columns (ColSampler::is_feature_used_bytree)
  if (hist_build_impl(h, nullptr, nroot, const_hess, nullptr, nullptr, 1, nullptr, hist_slot(h, 0), rows_identity ? nullptr : h->d_rows, rows_identity)) return -1;
  if (dist) {
    // root of a sharded tree: (sum of gradients, sum of hessians, rows) of ALL ranks, read off the all-reduced integer totals the build has
    // left in d_limbs -- fl(q * sum k), the exact total of the once-rounded gradients -- so that, like the histograms, they do not depend
    // on how the rows were dealt to the ranks (a sum of per-rank fp64 sums would); the caller's (local) sum_gradient / sum_hessian are not used
    if (!h->d_tree_red) HIP_OK(hipMalloc(&h->d_tree_red, sizeof(double) * 4));
    double glob[3];
    HIP_OK(gpb::launch_hist_root_sums(h->d_limbs, h->total_bins, h->d_bin_offsets, h->d_absmax, h->d_absmax + 1, const_hess, h->has_hess ? 1 : 0, h->d_tree_red, st));
    HIP_OK(hipMemcpyAsync(glob, h->d_tree_red, sizeof(glob), hipMemcpyDeviceToHost, st));
    HIP_OK(hipStreamSynchronize(st));
    sg[0] = glob[0]; sh[0] = glob[1]; gcnt[0] = (int)glob[2];
  }
  HIP_OK(gpb::launch_hist_fix(hist_slot(h, 0), F, h->d_fix, h->d_fix + F, h->d_fix + 2 * (size_t)F, sg[0], sh[0], st));
  // parent_output of the root's search: its own output with L1 / max_delta_step and without smoothing (SerialTreeLearner::GetParentOutput,
  // serial_tree_learner.cpp:758-770 -> CalculateSplittedLeafOutput, feature_histogram.hpp:743-765)
  double root_out;
  {
    const double g0 = sg[0], h0 = sh[0], l1 = h->reg_l1;
    const double sgn = (double)((g0 > 0.0) - (g0 < 0.0));
    root_out = l1 > 0.0 ? -(sgn * std::max(0.0, std::fabs(g0) - l1)) / (h0 + lambda_l2) : -g0 / (h0 + lambda_l2);
    if (h->reg_max_delta_step > 0.0 && std::fabs(root_out) > h->reg_max_delta_step)
      root_out = (double)((root_out > 0.0) - (root_out < 0.0)) * h->reg_max_delta_step;
  }
  HIP_OK(gpb::launch_hist_best_split(hist_slot(h, 0), F, h->d_fix, h->d_fix + F, h->d_meta3, sg[0], sh[0], gcnt[0], lambda_l2, min_data_in_leaf,
                                     min_sum_hessian_in_leaf, min_gain_to_split,
                                     gpb::SplitReg{ h->reg_l1, h->reg_max_delta_step, h->reg_path_smooth, root_out }, nullptr, h->d_split2,
                                     h->d_split2_i, nullptr, st, any_cat ? h->d_is_cat : nullptr, h->cat, h->d_cat_bits2));
  if (any_cat) HIP_OK(hipMemcpyAsync(h->h_cat_bits2, h->d_cat_bits2, sizeof(unsigned) * (size_t)F * 8, hipMemcpyDeviceToHost, st));
  HIP_OK(hipMemcpyAsync(h->h_split2, h->d_split2, sizeof(double) * (size_t)F * 10, hipMemcpyDeviceToHost, st));
  HIP_OK(hipMemcpyAsync(h->h_split2_i, h->d_split2_i, sizeof(int) * (size_t)(F + 1), hipMemcpyDeviceToHost, st));
  HIP_OK(hipStreamSynchronize(st));
  search_collect(0, all_used.data(), 0, false);
  // (feature-block exchange: the root was searched on every rank in full, but its is_splittable flags are kept for the rank's own features only below the root --
  //  the children inherit them, and a child's search covers the rank's own features)
  // the ranks' best candidates of a pair of children: record (child, rank) = {gain, feature, default_left, has_row, row[10], cat_bits[8]} as doubles
  auto exchange_bests = [&](int leaf_a, int leaf_b) -> int {
    const int W = h->comm.world, R = h->comm.rank;
    std::memset(h->h_xchg, 0, sizeof(double) * 2 * 16 * 24);
    const int leaves[2] = {leaf_a, leaf_b};
    for (int c = 0; c < 2; ++c) {
      double* rec = h->h_xchg + ((size_t)c * 16 + R) * 24;
      const TreeLeafBest& b = best[leaves[c]];
      rec[0] = b.has_row ? b.gain : 0.0; rec[1] = (double)b.feature; rec[2] = (double)b.dl; rec[3] = b.has_row ? 1.0 : 0.0;
      if (b.has_row) { for (int k = 0; k < 10; ++k) rec[4 + k] = b.row[k]; for (int k = 0; k < 8; ++k) rec[14 + k] = (double)b.cat_bits[k]; }
    }
    HIP_OK(hipMemcpyAsync(h->d_xchg, h->h_xchg, sizeof(double) * 2 * 16 * 24, hipMemcpyHostToDevice, st));
    if (comm_allreduce(h->comm, h->d_xchg, 2 * 16 * 24, GPB_T_F64, GPB_OP_SUM, st)) return -1;
    HIP_OK(hipMemcpyAsync(h->h_xchg, h->d_xchg, sizeof(double) * 2 * 16 * 24, hipMemcpyDeviceToHost, st));
    HIP_OK(hipStreamSynchronize(st));
    for (int c = 0; c < 2; ++c) {
      TreeLeafBest g;
      for (int r = 0; r < W; ++r) {
        const double* rec = h->h_xchg + ((size_t)c * 16 + r) * 24;
        if (rec[3] == 0.0) continue;
        const int f = (int)rec[1];
        if (split_better(rec[0], f, g.gain, g.feature)) {       // SplitInfo::operator> over the ranks' winners (the features are disjoint: no ties on a feature)
          g.gain = rec[0]; g.feature = f; g.dl = (int)rec[2]; g.has_row = true;
          for (int k = 0; k < 10; ++k) g.row[k] = rec[4 + k];
          for (int k = 0; k < 8; ++k) g.cat_bits[k] = (unsigned)rec[14 + k];
        }
      }
      best[leaves[c]] = g;
    }
    return 0;
  };

  for (int split = 0; split < L - 1; ++split) {
    int top_leaf = -1; double tg = -INFINITY; int tf = -1;
    for (int leaf = 0; leaf < nleaves; ++leaf)
      if (top_leaf < 0 || split_better(best[leaf].gain, best[leaf].feature, tg, tf)) { top_leaf = leaf; tg = best[leaf].gain; tf = best[leaf].feature; }
    const TreeLeafBest b = best[top_leaf];
    if (!(b.gain > 0.0) || !b.has_row) break;
    // max_depth (BeforeFindBestSplit :286-295): children at the depth limit are never searched, their best gain stays kMinScore
    const bool depth_stop = h->max_depth > 0 && depth[top_leaf] + 1 >= h->max_depth;
    const bool more = split + 1 < L - 1 && !depth_stop;      // the children are searched only when another split can follow
    // ---- enqueue: DataPartition::Split on the resident row list -> smaller child's histogram -> both children's search
    const int f = b.feature, c = cnt[top_leaf], gc = gcnt[top_leaf];
    const bool cat_split = any_cat && h->h_is_cat[f];
    const uint32_t thr = cat_split ? (uint32_t)ncat_nodes : (uint32_t)b.row[1];
    if (cat_split) ++ncat_nodes;
    int *blk_cnt = h->d_part, *blk_off = blk_cnt + nblk_max + 1;
    const int max_bin = h->h_bin_offsets[f + 1] - h->h_bin_offsets[f] - 1;
    const int sb = rows_identity ? 0 : buf[top_leaf], db = 1 - sb;
    // the host's wait for this split: not a stream synchronisation but a poll of one word of pinned memory that the split's LAST kernel
    // writes after its results (the children's search when one follows, else the partition); the data-parallel form synchronises the stream
    // (its collectives sit in between)
    constexpr bool poll_enabled = true;
    const bool poll = !dist;
    const int seq = poll ? ++h->tree_seq : 0;
    bool seq_from_partition = false;
    HIP_OK(gpb::launch_hist_partition_segment(h->d_bins_rm, h->fpad, f, max_bin, h->h_meta3[3 * f + 1], h->h_fix[2 * F + f], h->h_meta3[3 * f + 2],
                                              b.dl, thr, rows_identity ? nullptr : rows_buf[sb] + begin[top_leaf], c, blk_cnt, blk_off,
                                              rows_buf[db] + begin[top_leaf], h->d_counts, dist ? nullptr : h->h_counts, st,
                                              poll_enabled ? h->d_ptags : nullptr, ++h->part_epoch, (poll && !more) ? seq : 0, h->d_counts + 3,
                                              &seq_from_partition, cat_split ? b.cat_bits : nullptr));
    if (dist && comm_allreduce(h->comm, h->d_counts + 1, 1, GPB_T_I32, GPB_OP_SUM, st)) return -1;   // global left count (data_parallel_tree_learner.cpp:240-260)
    const int p_slot = slot_of[top_leaf];
    int s_slot = -1;
    if (more) {
      s_slot = next_free++;
      // smaller leaf: construct (:400-403); a rank may hold up to all c rows of it when the rows are sharded
      int chunks_for_search = 0;
      if (hist_build_planned(h, rows_buf[db], begin[top_leaf], c, gc, min_data_in_leaf, dist ? c : c / 2, const_hess, hist_slot(h, s_slot),
                             views_local ? &chunks_for_search : nullptr, bx)) return -1;
      gpb::ChildrenSearchArgs ca;
      if (chunks_for_search > 0) {      // no reduce launch: the search workgroups sum the chunk partials of their own feature (hist_kernels.h)
        ca.part_grad = h->d_part_grad; ca.part_hess = h->d_part_hess; ca.part_hess_hi = h->d_part_hess_hi; ca.part_cnt = h->d_part_cnt;
        ca.grad_max_bits = h->d_absmax; ca.hess_max_bits = h->d_absmax + 1;
        ca.fpad = h->fpad; ca.nchunks = chunks_for_search; ca.has_hess = h->has_hess ? 1 : 0; ca.const_hess = const_hess;
      }
      ca.smaller = hist_slot(h, s_slot); ca.parent = hist_slot(h, p_slot); ca.counts = h->d_counts;
      ca.bin_offsets = h->d_bin_offsets; ca.view_offset = h->d_fix; ca.num_bin = h->d_fix + F; ca.most_freq_bin = h->d_fix + 2 * (size_t)F; ca.meta3 = h->d_meta3;
      ca.num_features = F; ca.gcnt = gc; ca.min_data_in_leaf = min_data_in_leaf;
      ca.left_sum_gradient = b.row[6]; ca.left_sum_hessian = b.row[7]; ca.right_sum_gradient = b.row[8]; ca.right_sum_hessian = b.row[9];
      ca.lambda_l2 = lambda_l2; ca.min_sum_hessian = min_sum_hessian_in_leaf; ca.min_gain_to_split = min_gain_to_split;
      ca.lambda_l1 = h->reg_l1; ca.max_delta_step = h->reg_max_delta_step; ca.path_smooth = h->reg_path_smooth;
      ca.left_output = b.row[4]; ca.right_output = b.row[5];
      ca.out10 = h->h_split2; ca.out_flags = h->h_split2_i;          // pinned host memory, written by the kernel itself: no copy launches
      if (any_cat) { ca.is_cat = h->d_is_cat; ca.cat = h->cat; ca.out_cat = h->h_cat_bits2; }
      if (bx) { ca.own_f0 = own_f0; ca.own_f1 = own_f1; }
      if (poll) { ca.ticket = reinterpret_cast<unsigned*>(h->d_counts + 2); ca.host_seq = h->h_counts + 2; ca.seq = seq; }
      HIP_OK(gpb::launch_hist_children_search(ca, st));
    }
    if (dist) HIP_OK(hipMemcpyAsync(h->h_counts, h->d_counts, sizeof(int) * 2, hipMemcpyDeviceToHost, st));   // the all-reduced count
    bool seen = false;
    if (poll && (more || seq_from_partition)) {       // the one wait of this split
      volatile int* flag = h->h_counts + 2;
      for (long spin = 0; spin < 40000000L; ++spin) {   // (~ seconds: a fault or a lost kernel ends in the synchronisation below, which reports it)
        if (*flag == seq) { seen = true; break; }
        __builtin_ia32_pause();
      }
      std::atomic_thread_fence(std::memory_order_acquire);
    }
    if (!seen) HIP_OK(hipStreamSynchronize(st));
    // ---- bookkeeping of the split (SplitInner :565-690; Tree::Split)
    const int nl = h->h_counts[0], gnl = dist ? h->h_counts[1] : nl;
    rows_identity = false;
    const int left = top_leaf, right = nleaves;
    const int node = nnodes++;
    const int pn = parent_node[top_leaf];
    if (pn >= 0) { if (is_left[top_leaf]) left_child[pn] = node; else right_child[pn] = node; }
    split_feature_inner[node] = f; threshold_in_bin[node] = thr; default_left[node] = b.dl;
    left_child[node] = ~left; right_child[node] = ~right;
    split_gain[node] = (double)(float)(b.row[0] + min_gain_to_split);
    {       // what Tree::Split is handed for this node (tree.h:63-66): outputs, counts, sums of hessians of the two children
      const double info[6] = {b.row[4], b.row[5], (double)gnl, (double)(gc - gnl), b.row[7], b.row[9]};
      h->tree_node_info.insert(h->tree_node_info.end(), info, info + 6);
      h->tree_node_is_cat.push_back(cat_split ? 1 : 0);
      for (int w = 0; w < 8; ++w) h->tree_node_cat_bits.push_back(cat_split ? b.cat_bits[w] : 0u);
    }
    internal_count[node] = gc;
    parent_node[left] = node; parent_node[right] = node; is_left[left] = 1; is_left[right] = 0;
    begin[right] = begin[top_leaf] + nl; cnt[right] = c - nl; cnt[left] = nl;         // update_cnt (:591-595)
    gcnt[right] = gc - gnl; gcnt[left] = gnl;
    buf[left] = db; buf[right] = db;
    sg[left] = b.row[6]; sh[left] = b.row[7]; sg[right] = b.row[8]; sh[right] = b.row[9];
    lval[left] = b.row[4]; lval[right] = b.row[5];
    depth[right] = depth[left] = depth[top_leaf] + 1;         // (left == top_leaf: read before written)
    ++nleaves;
    if (depth_stop) { best[left].gain = -INFINITY; best[left].has_row = false; best[right] = TreeLeafBest(); }
    if (!more) continue;
    // ---- the children's candidates (BeforeFindBestSplit :296-306, FindBestSplitsFromHistograms :375-449)
    const int nl_ = gcnt[left], nr_ = gcnt[right];
    if (nr_ < 2 * min_data_in_leaf && nl_ < 2 * min_data_in_leaf) {
      best[left].gain = -INFINITY; best[left].has_row = false;
      best[right] = TreeLeafBest();
      --next_free;                                  // the kernels skipped the pair: the slot was not used
    } else {
      const int smaller = nl_ < nr_ ? left : right, larger = nl_ < nr_ ? right : left;
      used = splittable[left];                      // the parent's is_splittable flags (:330-334); `left` kept the parent's id
      slot_of[smaller] = s_slot;
      slot_of[larger] = p_slot;                     // the parent's histogram became the larger child's (:419-421)
      search_collect(smaller, used.data(), 0, bx);
      search_collect(larger, used.data(), 1, bx);
      if (bx && exchange_bests(smaller, larger)) return -1;       // (every rank takes this branch together: the counts that decide it are global)
    }
  }
  *out_num_leaves = nleaves;
  for (int k = 0; k < nleaves; ++k) { leaf_value[k] = lval[k]; leaf_count[k] = gcnt[k]; }
  if (data_leaf_index) {
    if (nleaves == 1) {                              // never split: every row of the root is in leaf 0, rows outside a bag in none (-1)
      std::fill(data_leaf_index, data_leaf_index + n, h->root_cnt > 0 ? -1 : 0);
      if (h->root_cnt > 0) {
        std::vector<int> rr((size_t)nroot);
        HIP_OK(hipMemcpyAsync(rr.data(), h->d_root_rows, sizeof(int) * (size_t)nroot, hipMemcpyDeviceToHost, st));
        HIP_OK(hipStreamSynchronize(st));
        for (int r : rr) data_leaf_index[r] = 0;
      }
    } else {
      // segments sorted by their begin -> leaf id of every position, scattered to the rows
      std::vector<int> order(nleaves);
      for (int k = 0; k < nleaves; ++k) order[k] = k;
      // (begin, cnt): a leaf without local rows (possible on a rank of a sharded handle) shares its begin with the next segment and must
      // come BEFORE it, because the labelling kernel gives a position to the LAST segment whose begin is <= the position
      std::sort(order.begin(), order.end(), [&](int a, int b2) { return begin[a] != begin[b2] ? begin[a] < begin[b2] : cnt[a] < cnt[b2]; });
      std::vector<int> seg(3 * (size_t)nleaves);
      for (int k = 0; k < nleaves; ++k) { seg[k] = begin[order[k]]; seg[nleaves + k] = order[k]; seg[2 * nleaves + k] = buf[order[k]]; }
      int* d_seg = h->d_part;                                   // scratch: the partition workspace is free now
      int* d_lab = h->d_part + 3 * nleaves;
      HIP_OK(hipMemcpyAsync(d_seg, seg.data(), sizeof(int) * seg.size(), hipMemcpyHostToDevice, st));
      if (h->root_cnt > 0) HIP_OK(hipMemsetAsync(d_lab, 0xFF, sizeof(int) * (size_t)n, st));      // rows outside the bag: -1
      HIP_OK(gpb::launch_hist_label_rows(h->d_rows, h->d_rows2, nroot, d_seg, d_seg + nleaves, d_seg + 2 * nleaves, nleaves, d_lab, st));
      HIP_OK(hipMemcpyAsync(data_leaf_index, d_lab, sizeof(int) * (size_t)n, hipMemcpyDeviceToHost, st));
    }
  }
  int part_err = 0;
  HIP_OK(hipMemcpyAsync(&part_err, h->d_counts + 3, sizeof(int), hipMemcpyDeviceToHost, st));
  HIP_OK(hipStreamSynchronize(st));
  if (part_err) { (void)hipMemset(h->d_counts + 3, 0, sizeof(int)); return fail("gpb_hip_hist_grow_tree: a block of the one-pass partition gave up waiting for its peers "); }
  API_END();
}

// per node of the LAST tree grown on this handle: {left output, right output, left count, right count, left sum of hessians, right sum of
// hessians} -- the arguments Tree::Split (include/LightGBM/tree.h:63-66) takes next to what gpb_hip_hist_grow_tree returns; out: 6 x nodes
extern "C" int gpb_hip_hist_last_tree_node_info(gpb_hip_hist_t* h, int32_t num_nodes, double* out6) {
  API_BEGIN();
  if (!h || !out6) return fail("null argument");
  if (num_nodes < 0 || (size_t)num_nodes * 6 > h->tree_node_info.size()) return fail("gpb_hip_hist_last_tree_node_info: the last tree has %d nodes", (int)(h->tree_node_info.size() / 6));
  std::copy(h->tree_node_info.begin(), h->tree_node_info.begin() + (size_t)num_nodes * 6, out6);
  API_END();
}

// per node of the LAST tree grown on this handle: is the split categorical, and the set of the feature's BINS that go left (8 words, bit b = bin b) --
// what Tree::SplitCategorical takes as cat_bitset_inner (serial_tree_learner.cpp:617-640); for such a node threshold_in_bin is its running index
// among the tree's categorical nodes (the reference's index into cat_boundaries_inner_, tree.cpp:76-108)
extern "C" int gpb_hip_hist_last_tree_cat_nodes(gpb_hip_hist_t* h, int32_t num_nodes, int32_t* is_categorical, uint32_t* cat_bits8) {
  API_BEGIN();
  if (!h || !is_categorical || !cat_bits8) return fail("null argument");
  if (num_nodes < 0 || (size_t)num_nodes > h->tree_node_is_cat.size()) return fail("gpb_hip_hist_last_tree_cat_nodes: the last tree has %d nodes", (int)h->tree_node_is_cat.size());
  std::copy(h->tree_node_is_cat.begin(), h->tree_node_is_cat.begin() + num_nodes, is_categorical);
  std::copy(h->tree_node_cat_bits.begin(), h->tree_node_cat_bits.begin() + (size_t)num_nodes * 8, cat_bits8);
  API_END();
}
