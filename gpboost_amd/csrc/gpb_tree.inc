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
  h->tree_node_info.clear(); h->tree_node_is_cat.clear(); h->tree_node_cat_bits.clear(); h->last_tree.valid = false;
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
  {       // the tree as handed to the caller, for gpb_hip_hist_forest_keep_last_tree (valid once this call has succeeded)
    gpb_hip_hist::LastTree& lt = h->last_tree;
    lt.num_leaves = nleaves;
    lt.split_feature.assign(split_feature_inner, split_feature_inner + nnodes); lt.threshold.assign(threshold_in_bin, threshold_in_bin + nnodes);
    lt.default_left.assign(default_left, default_left + nnodes); lt.left_child.assign(left_child, left_child + nnodes);
    lt.right_child.assign(right_child, right_child + nnodes); lt.leaf_value.assign(lval.begin(), lval.begin() + nleaves);
    lt.leaf_count.assign(gcnt.begin(), gcnt.begin() + nleaves);
  }
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
  h->last_tree.valid = true;
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

// ---- tree scoring: which leaf does a binned row fall into, score += leaf value (tree_predict_kernels.hip) ----------------------------------
// Stands in for Tree::AddPredictionToScore on binned rows (src/LightGBM/io/tree.cpp:147, :226; Tree::DecisionInner, include/LightGBM/tree.h:349-409) as
// GBDT::UpdateScore uses it for the out-of-bag rows and the validation sets of every iteration (src/LightGBM/boosting/gbdt.cpp:606-623,
// score_updater.hpp:93-96, :118-122).  A tree is compiled when it is stored: per node the 256-bit set of STORED bins of its column that go left.
namespace {

// The rule of the partition kernels (hist_kernels.hip: make_split_rule + goes_left; DenseBin::SplitInner / SplitCategoricalInner, dense_bin.hpp:176-342,
// single-feature group: min_bin = 1) restated for the host, stored bins 0 .. 255.  The kernels' own code is left as it is.
void node_go_left_mask(int max_bin, int default_bin, int most_freq_bin, int missing_type, int default_left, uint32_t threshold, const uint32_t* cat_bits8,
                       uint32_t* mask8) {
  for (int w = 0; w < 8; ++w) mask8[w] = 0u;
  const auto set = [&](int bin, bool left) { if (left) mask8[bin >> 5] |= 1u << (bin & 31); };
  if (cat_bits8) {
    const int cat_offset = most_freq_bin == 0 ? 1 : 0;
    const bool default_goes_left = most_freq_bin > 0 && most_freq_bin < 256 && ((cat_bits8[most_freq_bin >> 5] >> (most_freq_bin & 31)) & 1u);   // :316-320
    set(0, default_goes_left);
    for (int bin = 1; bin < 256; ++bin) { const int b = bin - 1 + cat_offset; set(bin, ((cat_bits8[b >> 5] >> (b & 31)) & 1u) != 0u); }
    return;
  }
  const bool miss_zero = missing_type == 1, miss_na = missing_type == 2;
  const bool mfb_zero = miss_zero && default_bin == most_freq_bin;                                   // dense_bin.hpp:268-272
  const bool mfb_na = miss_na && (max_bin == most_freq_bin + 1 && most_freq_bin > 0);                // :294-298 with min_bin = 1
  int th = (int)((threshold + 1u) & 0xffu), tz = (1 + default_bin) & 0xff;                           // VAL_T = uint8_t arithmetic (:182-187)
  if (most_freq_bin == 0) { th = (th - 1) & 0xff; tz = (tz - 1) & 0xff; }
  const bool default_goes_left = (unsigned)most_freq_bin <= threshold;                               // :196-199
  const bool missing_goes_left = (miss_zero || miss_na) && default_left;                             // :200-205
  const bool zero_is_missing = (miss_na && mfb_na) || (miss_zero && mfb_zero);
  for (int bin = 0; bin < 256; ++bin) {
    bool left;
    if (1 < max_bin) {
      if ((miss_zero && !mfb_zero && bin == tz) || (miss_na && !mfb_na && bin == max_bin)) left = missing_goes_left;
      else if (bin == 0) left = zero_is_missing ? missing_goes_left : default_goes_left;
      else left = !(bin > th);
    } else {
      if (miss_zero && !mfb_zero && bin == tz) left = missing_goes_left;
      else if (bin != max_bin) left = zero_is_missing ? missing_goes_left : default_goes_left;
      else left = (miss_na && !mfb_na) ? missing_goes_left : (max_bin <= th);
    }
    set(bin, left);
  }
}

// the stored trees on the device: everything not there yet is uploaded (buffers grow by doubling); ends with a synchronisation, so that the scoring calls
// themselves copy nothing
int forest_upload(gpb_hip_hist_t* h, int first_new_tree) {
  const int ntrees = (int)(h->forest_desc.size() / 4);
  HIP_OK(hipSetDevice(h->device));
  HIP_OK(hipStreamSynchronize(h->stream));                 // no scoring kernel is reading the buffers
  int from_tree = first_new_tree;
  if (h->forest_words.size() > h->forest_cap_words || ntrees > h->forest_cap_trees) {
    const size_t cw = std::max<size_t>(2 * h->forest_words.size(), 1u << 14);
    const int ct = std::max(2 * ntrees, 64);
    dev_free(h->d_forest); dev_free(h->d_forest_desc); h->forest_cap_words = 0; h->forest_cap_trees = 0;
    HIP_OK(hipMalloc(&h->d_forest, sizeof(uint32_t) * cw));
    HIP_OK(hipMalloc(&h->d_forest_desc, sizeof(int) * 4 * (size_t)ct));
    h->forest_cap_words = cw; h->forest_cap_trees = ct;
    from_tree = 0;
  }
  if (from_tree < ntrees) {
    const size_t w0 = (size_t)h->forest_desc[4 * (size_t)from_tree];
    HIP_OK(hipMemcpy(h->d_forest + w0, h->forest_words.data() + w0, sizeof(uint32_t) * (h->forest_words.size() - w0), hipMemcpyHostToDevice));
    HIP_OK(hipMemcpy(h->d_forest_desc + 4 * (size_t)from_tree, h->forest_desc.data() + 4 * (size_t)from_tree, sizeof(int) * 4 * (size_t)(ntrees - from_tree),
                     hipMemcpyHostToDevice));
  }
  return 0;
}

// validate, compile and store one tree given as the arrays of include/LightGBM/tree.h
int forest_store(gpb_hip_hist_t* h, const char* who, int num_leaves, const int32_t* split_feature_inner, const uint32_t* threshold_in_bin, const int32_t* default_left,
                 const int32_t* left_child, const int32_t* right_child, const int32_t* node_is_cat, const uint32_t* node_cat_bits8, const double* leaf_value,
                 double shrinkage, int32_t* tree_id) {
  if (!h->has_fix || !h->has_split_info)
    return fail("%s: the feature metas have not been set (gpb_hip_hist_set_fix_info, gpb_hip_hist_set_split_info): the go-left sets of the nodes need them", who);
  if (num_leaves < 1) return fail("%s: invalid tree: num_leaves = %d", who, num_leaves);
  if (!leaf_value) return fail("%s: null argument", who);
  const int nn = num_leaves - 1, F = h->F;
  if (nn > 0 && (!split_feature_inner || !threshold_in_bin || !default_left || !left_child || !right_child)) return fail("%s: null argument", who);
  if ((long long)nn * GPB_TP_NODE_WORDS * 4 + (long long)num_leaves * 8 > GPB_TP_CHUNK_BYTES)
    return fail("%s: a tree of %d leaves does not fit the %d bytes of LDS a chunk of trees may take (at most 439 leaves)", who, num_leaves, GPB_TP_CHUNK_BYTES);
  // a tree that cannot spin a walk: every child is a leaf (~leaf, leaf < num_leaves) or a LATER node, every node but the root and every leaf is referenced exactly once
  std::vector<int> node_refs((size_t)nn, 0), leaf_refs((size_t)num_leaves, 0);
  for (int i = 0; i < nn; ++i) {
    if (split_feature_inner[i] < 0 || split_feature_inner[i] >= F) return fail("%s: invalid tree: node %d splits column %d of %d", who, i, split_feature_inner[i], F);
    for (const int c : {left_child[i], right_child[i]}) {
      if (c < 0) {
        if (~c >= num_leaves) return fail("%s: invalid tree: node %d points to leaf %d of %d", who, i, ~c, num_leaves);
        ++leaf_refs[(size_t)~c];
      } else {
        if (c <= i || c >= nn) return fail("%s: invalid tree: node %d has the child node %d (children are later nodes, below %d)", who, i, c, nn);
        ++node_refs[(size_t)c];
      }
    }
    const bool cat_column = h->any_cat && h->h_is_cat[(size_t)split_feature_inner[i]];
    const bool cat_node = node_is_cat ? node_is_cat[i] != 0 : cat_column;
    if (cat_node && (!node_is_cat || !node_cat_bits8)) return fail("%s: node %d is a categorical node without a set of bins (node_is_cat / node_cat_bits8)", who, i);
  }
  for (int i = 1; i < nn; ++i) if (node_refs[(size_t)i] != 1) return fail("%s: invalid tree: node %d is referenced %d times", who, i, node_refs[(size_t)i]);
  if (nn > 0) for (int k = 0; k < num_leaves; ++k) if (leaf_refs[(size_t)k] != 1) return fail("%s: invalid tree: leaf %d is referenced %d times", who, k, leaf_refs[(size_t)k]);
  const int bytes = gpb::tree_predict_tree_bytes(num_leaves);
  const size_t w0 = h->forest_words.size();
  if (w0 + (size_t)bytes / 4 > (size_t)0x7fffffff) return fail("%s: the forest is full", who);
  h->forest_words.resize(w0 + (size_t)bytes / 4, 0u);
  uint32_t* w = h->forest_words.data() + w0;
  for (int i = 0; i < nn; ++i) {
    const int f = split_feature_inner[i];
    const bool cat_node = node_is_cat && node_is_cat[i] != 0;
    node_go_left_mask(h->h_bin_offsets[(size_t)f + 1] - h->h_bin_offsets[(size_t)f] - 1, h->h_meta3[3 * (size_t)f + 1], h->h_fix[2 * (size_t)F + f], h->h_meta3[3 * (size_t)f + 2],
                      default_left[i] ? 1 : 0, threshold_in_bin[i], cat_node ? node_cat_bits8 + 8 * (size_t)i : nullptr, w + (size_t)i * GPB_TP_NODE_WORDS);
    uint32_t* m = w + (size_t)i * GPB_TP_NODE_WORDS + 8;
    m[0] = (uint32_t)f; m[1] = (uint32_t)left_child[i]; m[2] = (uint32_t)right_child[i]; m[3] = 0u;
  }
  for (int k = 0; k < num_leaves; ++k) {
    const double v = leaf_value[k] * shrinkage;              // rounded once, here (Tree::Shrinkage, include/LightGBM/tree.h:188)
    std::memcpy(w + (size_t)nn * GPB_TP_NODE_WORDS + 2 * (size_t)k, &v, sizeof(double));
  }
  const int id = (int)(h->forest_desc.size() / 4);
  const int desc[4] = {(int)w0, num_leaves, bytes, 0};
  h->forest_desc.insert(h->forest_desc.end(), desc, desc + 4);
  if (forest_upload(h, id)) { h->forest_words.resize(w0); h->forest_desc.resize(4 * (size_t)id); return -1; }
  if (tree_id) *tree_id = id;
  return 0;
}

// One scoring call.  rows: HOST indices into the matrix `which` (nullptr: all its rows).  Exactly one of d_score (device, all rows of the matrix) / leaf_out_host.
int tree_predict_impl(gpb_hip_hist_t* h, const char* who, int which, int tree_begin, int tree_end, const int32_t* rows, int cnt, double* d_score,
                      int32_t* leaf_out_host, int reps = 0, double* ms_avg = nullptr) {
  const int ntrees = (int)(h->forest_desc.size() / 4);
  if (tree_begin < 0 || tree_end > ntrees || tree_begin >= tree_end)
    return fail("%s: trees [%d, %d): the forest holds %d (unknown tree id or empty range)", who, tree_begin, tree_end, ntrees);
  if (which != 0 && which != 1) return fail("%s: which = %d (0: training rows, 1: the attached matrix)", who, which);
  if (which == 1 && !h->d_pred_rm) return fail("%s: no second matrix is attached (gpb_hip_hist_set_pred_bins)", who);
  if (h->fpad > GPB_TP_MAX_FPAD) return fail("%s: rows of %d columns are wider than the %d bytes a staged row may take", who, h->F, GPB_TP_MAX_FPAD);
  const int N = which == 0 ? h->n : h->n_pred;
  if (!rows) cnt = N;
  if (cnt < 0) return fail("%s: cnt = %d", who, cnt);
  if (cnt == 0) return 0;
  HIP_OK(hipSetDevice(h->device));
  hipStream_t st = h->stream;
  gpb::TreePredictArgs a;
  a.bins_rm = which == 0 ? h->d_bins_rm : h->d_pred_rm; a.fpad = h->fpad; a.rows = nullptr; a.mult = nullptr; a.cnt = cnt;
  a.forest = h->d_forest; a.desc = reinterpret_cast<const int4*>(h->d_forest_desc); a.tree_begin = tree_begin; a.tree_end = tree_end;
  a.score = d_score; a.leaf_out = nullptr;
  if (rows) {
    bool ascending = true;
    for (int i = 0; i < cnt; ++i) {
      if (rows[i] < 0 || rows[i] >= N) return fail("%s: row index %d (position %d) outside the matrix of %d rows", who, rows[i], i, N);
      if (i > 0 && rows[i] <= rows[i - 1]) ascending = false;
    }
    if (h->prows_pending) { HIP_OK(hipEventSynchronize(h->ev_prows)); h->prows_pending = false; }      // the staging buffer is free again
    if (h->prows_cap < 2 * cnt) {
      HIP_OK(hipStreamSynchronize(st));
      dev_free(h->d_prows); if (h->h_prows) { (void)hipHostFree(h->h_prows); h->h_prows = nullptr; } h->prows_cap = 0;
      HIP_OK(hipMalloc(&h->d_prows, sizeof(int) * 2 * (size_t)cnt));
      HIP_OK(hipHostMalloc(&h->h_prows, sizeof(int) * 2 * (size_t)cnt));
      h->prows_cap = 2 * cnt;
    }
    if (!h->ev_prows) HIP_OK(hipEventCreateWithFlags(&h->ev_prows, hipEventDisableTiming));
    int m = cnt;
    bool with_mult = false;
    if (d_score && !ascending) {
      // a list that is unsorted or has repeats: AddPredictionToScore adds once per OCCURRENCE (tree.cpp:226); one lane owns a row, so the list is sorted and
      // run-length encoded and the lane adds the leaf value as many times as the row occurs -- per row the same additions in the same order
      std::vector<int> sorted(rows, rows + cnt);
      std::sort(sorted.begin(), sorted.end());
      m = 0;
      for (int i = 0; i < cnt; ++i) {
        if (m > 0 && h->h_prows[m - 1] == sorted[(size_t)i]) { ++h->h_prows[cnt + m - 1]; continue; }
        h->h_prows[m] = sorted[(size_t)i]; h->h_prows[cnt + m] = 1; ++m;
      }
      with_mult = true;
    } else {
      std::copy(rows, rows + cnt, h->h_prows);
    }
    HIP_OK(hipMemcpyAsync(h->d_prows, h->h_prows, sizeof(int) * (size_t)(with_mult ? 2 * cnt : cnt), hipMemcpyHostToDevice, st));
    HIP_OK(hipEventRecord(h->ev_prows, st));
    h->prows_pending = true;
    a.rows = h->d_prows; a.mult = with_mult ? h->d_prows + cnt : nullptr; a.cnt = m;
  }
  int lds = 0, chunk = 0;                                  // the largest chunk of the range, by the rule of tree_predict_kernels.h
  for (int t = tree_begin; t < tree_end; ++t) {
    const int b = h->forest_desc[4 * (size_t)t + 2];
    if (chunk > 0 && chunk + b > GPB_TP_CHUNK_BYTES) chunk = 0;
    chunk += b; lds = std::max(lds, chunk);
  }
  a.lds_tree_bytes = lds;
  if (leaf_out_host) {
    if (h->pleaf_cap < cnt) { HIP_OK(hipStreamSynchronize(st)); dev_free(h->d_pleaf); h->pleaf_cap = 0; HIP_OK(hipMalloc(&h->d_pleaf, sizeof(int) * (size_t)cnt)); h->pleaf_cap = cnt; }
    a.leaf_out = h->d_pleaf;
  }
  HIP_OK(gpb::launch_tree_predict(a, st));
  if (ms_avg) {      // measurement helper: the launch above was the warm-up; `reps` more of the same launch between two events
    hipEvent_t e0 = nullptr, e1 = nullptr;
    HIP_OK(hipEventCreate(&e0)); HIP_OK(hipEventCreate(&e1));
    const auto drop = scope_exit([&] { (void)hipEventDestroy(e0); (void)hipEventDestroy(e1); });
    HIP_OK(hipEventRecord(e0, st));
    for (int rep = 0; rep < reps; ++rep) HIP_OK(gpb::launch_tree_predict(a, st));
    HIP_OK(hipEventRecord(e1, st));
    HIP_OK(hipStreamSynchronize(st));
    float ms = 0.f;
    HIP_OK(hipEventElapsedTime(&ms, e0, e1));
    *ms_avg = ms / reps;
  }
  if (leaf_out_host) {
    HIP_OK(hipMemcpyAsync(leaf_out_host, h->d_pleaf, sizeof(int) * (size_t)cnt, hipMemcpyDeviceToHost, st));
    HIP_OK(hipStreamSynchronize(st));
  }
  return 0;
}

// ---- per-feature contributions (TreeSHAP) of stored trees (tree_shap_kernels.hip) ------------------------------------------------------------------------
// Stands in for Tree::PredictContrib -> Tree::TreeSHAP (src/LightGBM/io/tree.cpp:827-998) on binned rows.  The recursion's unique path is compiled per leaf,
// once, when the cover counts of a tree arrive (tree_shap_kernels.h); the kernel then works one (row, leaf) at a time.

struct ShapElem { int col; uint32_t set[8]; double zero; };

// The path table of one tree: per leaf the DISTINCT columns on its root-to-leaf path in order of first appearance, each with the AND of the go-left sets of its
// nodes on the path (complemented for right turns) and the product of count(child) / count(node) over those nodes, multiplied root to leaf.  count(node) =
// the sum of the leaf counts below it (the reference's internal_count_ after training).  Host only; the input is validated (a walk cannot spin or leave it).
int tree_shap_paths(const char* who, int num_leaves, const int32_t* split_feature_inner, const int32_t* left_child, const int32_t* right_child,
                    const uint32_t* node_sets8, const int32_t* leaf_count, std::vector<int>* first, std::vector<ShapElem>* elems) {
  first->assign(1, 0); elems->clear();
  if (num_leaves < 1) return fail("%s: invalid tree: num_leaves = %d", who, num_leaves);
  if (num_leaves == 1) { first->push_back(0); return 0; }                      // no nodes, no elements, no counts needed
  if (!split_feature_inner || !left_child || !right_child || !node_sets8 || !leaf_count) return fail("%s: null argument", who);
  const int nn = num_leaves - 1;
  for (int k = 0; k < num_leaves; ++k)
    if (leaf_count[k] < 1) return fail("%s: leaf %d has the count %d (a leaf count is at least 1)", who, k, leaf_count[k]);
  std::vector<long long> ncnt((size_t)nn, 0);
  for (int i = nn - 1; i >= 0; --i) {
    if (split_feature_inner[i] < 0) return fail("%s: invalid tree: node %d splits column %d", who, i, split_feature_inner[i]);
    for (const int c : {left_child[i], right_child[i]}) {
      if (c < 0) { if (~c >= num_leaves) return fail("%s: invalid tree: node %d points to leaf %d of %d", who, i, ~c, num_leaves); ncnt[(size_t)i] += leaf_count[~c]; }
      else { if (c <= i || c >= nn) return fail("%s: invalid tree: node %d has the child node %d (children are later nodes, below %d)", who, i, c, nn); ncnt[(size_t)i] += ncnt[(size_t)c]; }
    }
  }
  std::vector<std::vector<ShapElem>> paths((size_t)num_leaves);
  std::vector<char> seen((size_t)num_leaves, 0);
  std::vector<ShapElem> path;
  int bad_leaf = -1;
  std::function<void(int)> walk = [&](int node) {
    const int f = split_feature_inner[node];
    for (int side = 0; side < 2; ++side) {
      const int c = side == 0 ? left_child[node] : right_child[node];
      const double q = (double)(c < 0 ? (long long)leaf_count[~c] : ncnt[(size_t)c]) / (double)ncnt[(size_t)node];
      size_t at = 0;
      while (at < path.size() && path[at].col != f) ++at;
      const bool fresh = at == path.size();
      if (fresh) { ShapElem e; e.col = f; for (int w = 0; w < 8; ++w) e.set[w] = 0xffffffffu; e.zero = 1.0; path.push_back(e); }
      const ShapElem saved = path[at];
      for (int w = 0; w < 8; ++w) path[at].set[w] &= side == 0 ? node_sets8[8 * (size_t)node + w] : ~node_sets8[8 * (size_t)node + w];
      path[at].zero *= q;
      if (c < 0) { if (seen[(size_t)~c]) bad_leaf = ~c; else { seen[(size_t)~c] = 1; paths[(size_t)~c] = path; } }
      else walk(c);
      if (fresh) path.pop_back(); else path[at] = saved;
    }
  };
  walk(0);
  if (bad_leaf >= 0) return fail("%s: invalid tree: leaf %d is referenced more than once", who, bad_leaf);
  for (int k = 0; k < num_leaves; ++k) {
    if (!seen[(size_t)k]) return fail("%s: invalid tree: leaf %d is referenced 0 times", who, k);
    if ((int)paths[(size_t)k].size() > GPB_SHAP_MAX_UNIQUE)
      return fail("%s: the path to leaf %d has %d distinct columns, more than the %d the permutation weights stay accurate for", who, k, (int)paths[(size_t)k].size(),
                  GPB_SHAP_MAX_UNIQUE);
    elems->insert(elems->end(), paths[(size_t)k].begin(), paths[(size_t)k].end());
    first->push_back((int)elems->size());
  }
  return 0;
}

// compile the path table of the stored tree tree_id from its cover counts (nullptr: a tree of one leaf), append it and bring the device copy up to date
int shap_set_counts(gpb_hip_hist_t* h, const char* who, int tree_id, const int32_t* leaf_count) {
  const int ntrees = (int)(h->forest_desc.size() / 4);
  if (tree_id < 0 || tree_id >= ntrees) return fail("%s: tree %d: the forest holds %d (unknown tree id)", who, tree_id, ntrees);
  const int nl = h->forest_desc[4 * (size_t)tree_id + 1], nn = nl - 1;
  if (nl > 1 && !leaf_count) return fail("%s: null argument", who);
  const uint32_t* w = h->forest_words.data() + (size_t)h->forest_desc[4 * (size_t)tree_id];
  std::vector<int32_t> sf((size_t)nn), lc((size_t)nn), rc((size_t)nn);
  std::vector<uint32_t> sets(8 * (size_t)nn);
  for (int i = 0; i < nn; ++i) {
    const uint32_t* nd = w + (size_t)i * GPB_TP_NODE_WORDS;
    std::copy(nd, nd + 8, sets.begin() + 8 * (size_t)i);
    sf[(size_t)i] = (int32_t)nd[8]; lc[(size_t)i] = (int32_t)nd[9]; rc[(size_t)i] = (int32_t)nd[10];
  }
  std::vector<int> first; std::vector<ShapElem> elems;
  if (tree_shap_paths(who, nl, sf.data(), lc.data(), rc.data(), sets.data(), leaf_count, &first, &elems)) return -1;
  std::vector<double> vals((size_t)nl);
  std::memcpy(vals.data(), w + (size_t)nn * GPB_TP_NODE_WORDS, sizeof(double) * (size_t)nl);
  double ev = vals[0];                                                         // Tree::ExpectedValue (tree.cpp:990-998)
  if (nl > 1) {
    double total = 0.0;
    for (int k = 0; k < nl; ++k) total += (double)leaf_count[k];
    ev = 0.0;
    for (int k = 0; k < nl; ++k) ev += ((double)leaf_count[k] / total) * vals[(size_t)k];
  }
  const size_t w0 = h->shap_words.size(), nw = (gpb::tree_shap_table_words(nl, (int)elems.size()) + 3) / 4 * 4;
  if (w0 + nw > (size_t)0x7fffffff) return fail("%s: the path tables are full", who);
  int emax = 0;
  for (int k = 0; k < nl; ++k) emax = std::max(emax, first[(size_t)k + 1] - first[(size_t)k]);
  h->shap_words.resize(w0 + nw, 0u);
  uint32_t* tb = h->shap_words.data() + w0;
  std::memcpy(tb, &ev, sizeof(double));
  std::memcpy(tb + 4, vals.data(), sizeof(double) * (size_t)nl);
  std::memcpy(tb + 4 + 2 * (size_t)nl, first.data(), sizeof(int) * ((size_t)nl + 1));
  uint32_t* eb = tb + 4 + 2 * (size_t)nl + gpb::tree_shap_first_words(nl);
  for (size_t e = 0; e < elems.size(); ++e) {
    uint32_t* x = eb + e * GPB_SHAP_ELEM_WORDS;
    std::copy(elems[e].set, elems[e].set + 8, x);
    x[8] = (uint32_t)elems[e].col;
    const double z = elems[e].zero, invz = 1.0 / z;
    std::memcpy(x + 12, &z, sizeof(double)); std::memcpy(x + 14, &invz, sizeof(double));
  }
  h->shap_desc.resize(4 * (size_t)ntrees, 0); h->shap_expected.resize((size_t)ntrees, 0.0);
  const int desc[4] = {(int)w0, nl, emax, 1};
  std::copy(desc, desc + 4, h->shap_desc.begin() + 4 * (size_t)tree_id);
  h->shap_expected[(size_t)tree_id] = ev;
  // device copy: no contribution kernel is reading the buffers; they grow by doubling; the new table and the (small) descriptor array are uploaded
  HIP_OK(hipSetDevice(h->device));
  HIP_OK(hipStreamSynchronize(h->stream));
  if (!h->d_shap_ratio) {
    std::vector<double> r(2 * (size_t)GPB_SHAP_RATIO_ENTRIES, 0.0);
    for (int d = 0; d <= GPB_SHAP_MAX_UNIQUE; ++d)
      for (int k = 0; k <= d + 1; ++k) {
        r[(size_t)d * GPB_SHAP_RATIO_STRIDE + k] = (double)k / (double)(d + 1);
        if (k > 0) r[(size_t)GPB_SHAP_RATIO_ENTRIES + (size_t)d * GPB_SHAP_RATIO_STRIDE + k] = (double)(d + 1) / (double)k;
      }
    HIP_OK(hipMalloc(&h->d_shap_ratio, sizeof(double) * r.size()));
    HIP_OK(hipMemcpy(h->d_shap_ratio, r.data(), sizeof(double) * r.size(), hipMemcpyHostToDevice));
  }
  size_t from = w0;
  if (h->shap_words.size() > h->shap_cap_words) {
    const size_t cw = std::max<size_t>(2 * h->shap_words.size(), 1u << 14);
    dev_free(h->d_shap); h->shap_cap_words = 0;
    HIP_OK(hipMalloc(&h->d_shap, sizeof(uint32_t) * cw));
    h->shap_cap_words = cw; from = 0;
  }
  if (ntrees > h->shap_cap_trees) {
    const int ct = std::max(2 * ntrees, 64);
    dev_free(h->d_shap_desc); h->shap_cap_trees = 0;
    HIP_OK(hipMalloc(&h->d_shap_desc, sizeof(int) * 4 * (size_t)ct));
    h->shap_cap_trees = ct;
  }
  HIP_OK(hipMemcpy(h->d_shap + from, h->shap_words.data() + from, sizeof(uint32_t) * (h->shap_words.size() - from), hipMemcpyHostToDevice));
  HIP_OK(hipMemcpy(h->d_shap_desc, h->shap_desc.data(), sizeof(int) * h->shap_desc.size(), hipMemcpyHostToDevice));
  return 0;
}

bool shap_has_table(const gpb_hip_hist_t* h, int t) { return 4 * (size_t)t + 3 < h->shap_desc.size() && h->shap_desc[4 * (size_t)t + 3] == 1; }

// One contribution call.  rows: HOST indices into the matrix `which` (nullptr: all its rows), no row twice.  d_out: device, [rows of the matrix][F + 1].
int tree_shap_impl(gpb_hip_hist_t* h, const char* who, int which, int tree_begin, int tree_end, const int32_t* rows, int cnt, double* d_out, int reps = 0,
                   double* ms_avg = nullptr) {
  const int ntrees = (int)(h->forest_desc.size() / 4);
  if (tree_begin < 0 || tree_end > ntrees || tree_begin >= tree_end)
    return fail("%s: trees [%d, %d): the forest holds %d (unknown tree id or empty range)", who, tree_begin, tree_end, ntrees);
  if (which != 0 && which != 1) return fail("%s: which = %d (0: training rows, 1: the attached matrix)", who, which);
  if (which == 1 && !h->d_pred_rm) return fail("%s: no second matrix is attached (gpb_hip_hist_set_pred_bins)", who);
  if (h->fpad > GPB_TP_MAX_FPAD) return fail("%s: rows of %d columns are wider than the %d bytes a staged row may take", who, h->F, GPB_TP_MAX_FPAD);
  const int N = which == 0 ? h->n : h->n_pred;
  if (!rows) cnt = N;
  if (cnt < 0) return fail("%s: cnt = %d", who, cnt);
  for (int t = tree_begin; t < tree_end; ++t)
    if (h->forest_desc[4 * (size_t)t + 1] > 1 && !shap_has_table(h, t))
      return fail("%s: tree %d has no leaf counts (gpb_hip_hist_forest_set_leaf_counts): the branches a row does not take are weighted by them", who, t);
  if (rows) {
    std::vector<unsigned char> listed((size_t)N, 0);
    for (int i = 0; i < cnt; ++i) {
      if (rows[i] < 0 || rows[i] >= N) return fail("%s: row index %d (position %d) outside the matrix of %d rows", who, rows[i], i, N);
      if (listed[(size_t)rows[i]]) return fail("%s: row %d is listed twice (position %d): a row's entries are updated once per call", who, rows[i], i);
      listed[(size_t)rows[i]] = 1;
    }
  }
  if (cnt == 0) return 0;
  for (int t = tree_begin; t < tree_end; ++t)                                 // a tree of one leaf needs no counts: its table is its value
    if (!shap_has_table(h, t) && shap_set_counts(h, who, t, nullptr)) return -1;
  int emax = 0;
  for (int t = tree_begin; t < tree_end; ++t) emax = std::max(emax, h->shap_desc[4 * (size_t)t + 2]);
  if (emax > GPB_SHAP_MAX_UNIQUE || gpb::tree_shap_rows_per_block(h->fpad, emax) == 0) return fail("%s: internal error: %d elements on a path", who, emax);
  HIP_OK(hipSetDevice(h->device));
  hipStream_t st = h->stream;
  gpb::TreeShapArgs a;
  a.bins_rm = which == 0 ? h->d_bins_rm : h->d_pred_rm; a.fpad = h->fpad; a.F = h->F; a.rows = nullptr; a.cnt = cnt;
  a.tables = h->d_shap; a.desc = reinterpret_cast<const int4*>(h->d_shap_desc); a.tree_begin = tree_begin; a.tree_end = tree_end;
  a.ratio = h->d_shap_ratio; a.out = d_out; a.max_unique = emax;
  if (rows) {                                                                  // the row list's staging buffer is the scoring calls' (same protocol)
    if (h->prows_pending) { HIP_OK(hipEventSynchronize(h->ev_prows)); h->prows_pending = false; }
    if (h->prows_cap < cnt) {
      HIP_OK(hipStreamSynchronize(st));
      dev_free(h->d_prows); if (h->h_prows) { (void)hipHostFree(h->h_prows); h->h_prows = nullptr; } h->prows_cap = 0;
      HIP_OK(hipMalloc(&h->d_prows, sizeof(int) * (size_t)cnt));
      HIP_OK(hipHostMalloc(&h->h_prows, sizeof(int) * (size_t)cnt));
      h->prows_cap = cnt;
    }
    if (!h->ev_prows) HIP_OK(hipEventCreateWithFlags(&h->ev_prows, hipEventDisableTiming));
    std::copy(rows, rows + cnt, h->h_prows);
    HIP_OK(hipMemcpyAsync(h->d_prows, h->h_prows, sizeof(int) * (size_t)cnt, hipMemcpyHostToDevice, st));
    HIP_OK(hipEventRecord(h->ev_prows, st));
    h->prows_pending = true;
    a.rows = h->d_prows;
  }
  HIP_OK(gpb::launch_tree_shap(a, st));
  if (ms_avg) {      // measurement helper: the launch above was the warm-up; `reps` more of the same launch between two events
    hipEvent_t e0 = nullptr, e1 = nullptr;
    HIP_OK(hipEventCreate(&e0)); HIP_OK(hipEventCreate(&e1));
    const auto drop = scope_exit([&] { (void)hipEventDestroy(e0); (void)hipEventDestroy(e1); });
    HIP_OK(hipEventRecord(e0, st));
    for (int rep = 0; rep < reps; ++rep) HIP_OK(gpb::launch_tree_shap(a, st));
    HIP_OK(hipEventRecord(e1, st));
    HIP_OK(hipStreamSynchronize(st));
    float ms = 0.f;
    HIP_OK(hipEventElapsedTime(&ms, e0, e1));
    *ms_avg = ms / reps;
  }
  return 0;
}

}  // namespace

extern "C" int gpb_hip_hist_node_go_left_mask(int32_t max_bin, int32_t default_bin, int32_t most_freq_bin, int32_t missing_type, int32_t default_left,
                                              uint32_t threshold, const uint32_t* cat_bits8, uint32_t* mask8_out) {
  API_BEGIN();
  if (!mask8_out) return fail("null argument");
  if (max_bin < 0 || max_bin > 255 || missing_type < 0 || missing_type > 2)
    return fail("gpb_hip_hist_node_go_left_mask: max_bin %d (0..255), missing type %d (0..2)", max_bin, missing_type);
  node_go_left_mask(max_bin, default_bin, most_freq_bin, missing_type, default_left ? 1 : 0, threshold, cat_bits8, mask8_out);
  API_END();
}

extern "C" int gpb_hip_hist_forest_add_tree(gpb_hip_hist_t* h, int32_t num_leaves, const int32_t* split_feature_inner, const uint32_t* threshold_in_bin,
                                            const int32_t* default_left, const int32_t* left_child, const int32_t* right_child, const int32_t* node_is_cat,
                                            const uint32_t* node_cat_bits8, const double* leaf_value, double shrinkage, int32_t* tree_id) {
  API_BEGIN();
  if (!h) return fail("null handle");
  if (forest_store(h, "gpb_hip_hist_forest_add_tree", num_leaves, split_feature_inner, threshold_in_bin, default_left, left_child, right_child, node_is_cat,
                   node_cat_bits8, leaf_value, shrinkage, tree_id)) return -1;
  API_END();
}

extern "C" int gpb_hip_hist_forest_keep_last_tree(gpb_hip_hist_t* h, double shrinkage, int32_t* tree_id) {
  API_BEGIN();
  if (!h) return fail("null handle");
  const gpb_hip_hist::LastTree& lt = h->last_tree;
  if (!lt.valid) return fail("gpb_hip_hist_forest_keep_last_tree: no tree has been grown on this handle (gpb_hip_hist_grow_tree)");
  std::vector<int> is_cat(h->tree_node_is_cat.begin(), h->tree_node_is_cat.end());
  int32_t id = -1;
  if (forest_store(h, "gpb_hip_hist_forest_keep_last_tree", lt.num_leaves, lt.split_feature.data(), lt.threshold.data(), lt.default_left.data(), lt.left_child.data(),
                   lt.right_child.data(), is_cat.data(), h->tree_node_cat_bits.data(), lt.leaf_value.data(), shrinkage, &id)) return -1;
  if (tree_id) *tree_id = id;
  // the tree's own cover counts (the global counts of gpb_hip_hist_grow_tree; with a bag the in-bag counts): its path table for the contributions.  A tree
  // that cannot have one (a path of more than GPB_SHAP_MAX_UNIQUE distinct columns) is stored all the same: scoring needs no table, a contribution call names it
  if (lt.num_leaves > 1 && (int)lt.leaf_count.size() == lt.num_leaves) (void)shap_set_counts(h, "gpb_hip_hist_forest_keep_last_tree", id, lt.leaf_count.data());
  API_END();
}

extern "C" int gpb_hip_hist_forest_size(gpb_hip_hist_t* h, int32_t* num_trees) {
  API_BEGIN();
  if (!h || !num_trees) return fail("null argument");
  *num_trees = (int32_t)(h->forest_desc.size() / 4);
  API_END();
}

extern "C" int gpb_hip_hist_forest_clear(gpb_hip_hist_t* h) {
  API_BEGIN();
  if (!h) return fail("null handle");
  HIP_OK(hipSetDevice(h->device));
  HIP_OK(hipStreamSynchronize(h->stream));
  h->forest_words.clear(); h->forest_desc.clear();
  h->shap_words.clear(); h->shap_desc.clear(); h->shap_expected.clear();
  API_END();
}

extern "C" int gpb_hip_hist_set_pred_bins(gpb_hip_hist_t* h, int32_t n_pred, const uint8_t* bins_fm) {
  API_BEGIN();
  if (!h) return fail("null handle");
  HIP_OK(hipSetDevice(h->device));
  HIP_OK(hipStreamSynchronize(h->stream));
  dev_free(h->d_pred_rm); h->n_pred = 0;
  if (!bins_fm || n_pred <= 0) return 0;
  uint8_t* d_fm = nullptr;
  const auto free_tmp = scope_exit([&] { (void)hipFree(d_fm); });
  HIP_OK(hipMalloc(&d_fm, (size_t)n_pred * h->F));
  HIP_OK(hipMemcpy(d_fm, bins_fm, (size_t)n_pred * h->F, hipMemcpyHostToDevice));
  HIP_OK(hipMalloc(&h->d_pred_rm, (size_t)n_pred * h->fpad));
  HIP_OK(gpb::launch_bins_transpose(d_fm, h->d_pred_rm, n_pred, h->F, h->fpad, h->stream));
  HIP_OK(hipStreamSynchronize(h->stream));
  h->n_pred = n_pred;
  API_END();
}

extern "C" int gpb_hip_hist_predict_leaf(gpb_hip_hist_t* h, int32_t which, int32_t tree_id, const int32_t* rows, int32_t cnt, int32_t* leaf_out) {
  API_BEGIN();
  if (!h || !leaf_out) return fail("null argument");
  if (tree_predict_impl(h, "gpb_hip_hist_predict_leaf", which, tree_id, tree_id + 1, rows, cnt, nullptr, leaf_out)) return -1;
  API_END();
}

extern "C" int gpb_hip_hist_add_score_dev(gpb_hip_hist_t* h, int32_t which, int32_t tree_begin, int32_t tree_end, const int32_t* rows, int32_t cnt,
                                          double* score_dev) {
  API_BEGIN();
  if (!h || !score_dev) return fail("null argument");
  if (tree_predict_impl(h, "gpb_hip_hist_add_score_dev", which, tree_begin, tree_end, rows, cnt, score_dev, nullptr)) return -1;
  API_END();
}

extern "C" int gpb_hip_hist_add_score_bench(gpb_hip_hist_t* h, int32_t which, int32_t tree_begin, int32_t tree_end, const int32_t* rows, int32_t cnt,
                                            double* score_dev, int32_t reps, double* ms_avg) {
  API_BEGIN();
  if (!h || !score_dev || !ms_avg || reps < 1) return fail("invalid argument");
  if (tree_predict_impl(h, "gpb_hip_hist_add_score_bench", which, tree_begin, tree_end, rows, cnt, score_dev, nullptr, reps, ms_avg)) return -1;
  API_END();
}

extern "C" int gpb_hip_hist_add_score(gpb_hip_hist_t* h, int32_t which, int32_t tree_begin, int32_t tree_end, const int32_t* rows, int32_t cnt, double* score) {
  API_BEGIN();
  if (!h || !score) return fail("null argument");
  if (which == 1 && !h->d_pred_rm) return fail("gpb_hip_hist_add_score: no second matrix is attached (gpb_hip_hist_set_pred_bins)");
  if (which != 0 && which != 1) return fail("gpb_hip_hist_add_score: which = %d (0: training rows, 1: the attached matrix)", which);
  const int N = which == 0 ? h->n : h->n_pred;
  HIP_OK(hipSetDevice(h->device));
  if (h->pscore_cap < N) {
    HIP_OK(hipStreamSynchronize(h->stream));
    dev_free(h->d_pscore); h->pscore_cap = 0;
    HIP_OK(hipMalloc(&h->d_pscore, sizeof(double) * (size_t)N)); h->pscore_cap = N;
  }
  HIP_OK(hipMemcpyAsync(h->d_pscore, score, sizeof(double) * (size_t)N, hipMemcpyHostToDevice, h->stream));
  if (tree_predict_impl(h, "gpb_hip_hist_add_score", which, tree_begin, tree_end, rows, cnt, h->d_pscore, nullptr)) { (void)hipStreamSynchronize(h->stream); return -1; }
  HIP_OK(hipMemcpyAsync(score, h->d_pscore, sizeof(double) * (size_t)N, hipMemcpyDeviceToHost, h->stream));
  HIP_OK(hipStreamSynchronize(h->stream));
  API_END();
}

extern "C" int gpb_hip_tree_shap_paths(int32_t num_leaves, const int32_t* split_feature_inner, const int32_t* left_child, const int32_t* right_child,
                                       const uint32_t* node_sets8, const int32_t* leaf_count, int32_t elem_cap, int32_t* leaf_first, int32_t* elem_column,
                                       uint32_t* elem_set8, double* elem_zero) {
  API_BEGIN();
  if (!leaf_first || elem_cap < 0 || (elem_cap > 0 && (!elem_column || !elem_set8 || !elem_zero))) return fail("gpb_hip_tree_shap_paths: null argument");
  std::vector<int> first; std::vector<ShapElem> elems;
  if (tree_shap_paths("gpb_hip_tree_shap_paths", num_leaves, split_feature_inner, left_child, right_child, node_sets8, leaf_count, &first, &elems)) return -1;
  if ((int)elems.size() > elem_cap) return fail("gpb_hip_tree_shap_paths: the table has %d elements, the output arrays hold %d", (int)elems.size(), elem_cap);
  std::copy(first.begin(), first.end(), leaf_first);
  for (size_t e = 0; e < elems.size(); ++e) {
    elem_column[e] = elems[e].col; elem_zero[e] = elems[e].zero;
    std::copy(elems[e].set, elems[e].set + 8, elem_set8 + 8 * e);
  }
  API_END();
}

extern "C" int gpb_hip_hist_forest_set_leaf_counts(gpb_hip_hist_t* h, int32_t tree_id, const int32_t* leaf_count) {
  API_BEGIN();
  if (!h) return fail("null handle");
  if (shap_set_counts(h, "gpb_hip_hist_forest_set_leaf_counts", tree_id, leaf_count)) return -1;
  API_END();
}

extern "C" int gpb_hip_hist_tree_expected_value(gpb_hip_hist_t* h, int32_t tree_id, double* expected_value) {
  API_BEGIN();
  if (!h || !expected_value) return fail("null argument");
  const int ntrees = (int)(h->forest_desc.size() / 4);
  if (tree_id < 0 || tree_id >= ntrees) return fail("gpb_hip_hist_tree_expected_value: tree %d: the forest holds %d (unknown tree id)", tree_id, ntrees);
  if (shap_has_table(h, tree_id)) { *expected_value = h->shap_expected[(size_t)tree_id]; return 0; }
  if (h->forest_desc[4 * (size_t)tree_id + 1] > 1) return fail("gpb_hip_hist_tree_expected_value: tree %d has no leaf counts (gpb_hip_hist_forest_set_leaf_counts)", tree_id);
  std::memcpy(expected_value, h->forest_words.data() + (size_t)h->forest_desc[4 * (size_t)tree_id], sizeof(double));      // one leaf: its stored value
  API_END();
}

extern "C" int gpb_hip_hist_add_contrib_dev(gpb_hip_hist_t* h, int32_t which, int32_t tree_begin, int32_t tree_end, const int32_t* rows, int32_t cnt, void* out_dev) {
  API_BEGIN();
  if (!h || !out_dev) return fail("null argument");
  if (tree_shap_impl(h, "gpb_hip_hist_add_contrib_dev", which, tree_begin, tree_end, rows, cnt, static_cast<double*>(out_dev))) return -1;
  API_END();
}

extern "C" int gpb_hip_hist_add_contrib_bench(gpb_hip_hist_t* h, int32_t which, int32_t tree_begin, int32_t tree_end, const int32_t* rows, int32_t cnt, void* out_dev,
                                              int32_t reps, double* ms_avg) {
  API_BEGIN();
  if (!h || !out_dev || !ms_avg || reps < 1) return fail("invalid argument");
  if (tree_shap_impl(h, "gpb_hip_hist_add_contrib_bench", which, tree_begin, tree_end, rows, cnt, static_cast<double*>(out_dev), reps, ms_avg)) return -1;
  API_END();
}

extern "C" int gpb_hip_hist_add_contrib(gpb_hip_hist_t* h, int32_t which, int32_t tree_begin, int32_t tree_end, const int32_t* rows, int32_t cnt, double* out) {
  API_BEGIN();
  if (!h || !out) return fail("null argument");
  if (which == 1 && !h->d_pred_rm) return fail("gpb_hip_hist_add_contrib: no second matrix is attached (gpb_hip_hist_set_pred_bins)");
  if (which != 0 && which != 1) return fail("gpb_hip_hist_add_contrib: which = %d (0: training rows, 1: the attached matrix)", which);
  const size_t len = (size_t)(which == 0 ? h->n : h->n_pred) * (size_t)(h->F + 1);
  HIP_OK(hipSetDevice(h->device));
  if (h->pcontrib_cap < len) {
    HIP_OK(hipStreamSynchronize(h->stream));
    dev_free(h->d_pcontrib); h->pcontrib_cap = 0;
    HIP_OK(hipMalloc(&h->d_pcontrib, sizeof(double) * len)); h->pcontrib_cap = len;
  }
  HIP_OK(hipMemcpyAsync(h->d_pcontrib, out, sizeof(double) * len, hipMemcpyHostToDevice, h->stream));
  if (tree_shap_impl(h, "gpb_hip_hist_add_contrib", which, tree_begin, tree_end, rows, cnt, h->d_pcontrib)) { (void)hipStreamSynchronize(h->stream); return -1; }
  HIP_OK(hipMemcpyAsync(out, h->d_pcontrib, sizeof(double) * len, hipMemcpyDeviceToHost, h->stream));
  HIP_OK(hipStreamSynchronize(h->stream));
  API_END();
}

extern "C" int gpb_hip_hist_sync(gpb_hip_hist_t* h) {
  API_BEGIN();
  if (!h) return fail("null handle");
  HIP_OK(hipSetDevice(h->device));
  HIP_OK(hipStreamSynchronize(h->stream));
  API_END();
}
