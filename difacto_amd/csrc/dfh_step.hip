// dfh_step.hip — a training step on the main stream: the views of table and minibatch its launches take, forward, AUC,
// update / backward, the two stages dfh_sgd_step and the sharded schedules (dfh_shard.hip) are built from, and the step calls.
namespace {
RowSrc table_src(const dfh_table* t, const uint32_t* urow) {
  RowSrc s;
  s.wbase = reinterpret_cast<const float*>(t->v.hdr);
  s.wstride = sizeof(RowHdr) / sizeof(float);
  s.vbase = t->v.va;
  s.vstride = (size_t)2 * t->v.kp;
  s.urow = urow;
  s.flag_is_float = 0;
  return s;
}

RowSrc packed_src(const float* rows, int V_dim) {
  RowSrc s;
  size_t stride = dfh_row_stride(V_dim);
  s.wbase = rows;
  s.wstride = stride;
  s.vbase = rows + 4;
  s.vstride = stride;
  s.urow = nullptr;
  s.flag_is_float = 1;
  return s;
}

BatchView batch_view(const dfh_batch* b) {
  BatchView v;
  v.nrows = (uint32_t)b->nrows;
  v.nnz = (uint32_t)b->nnz;
  v.d_U = b->d_U;
  v.offset = b->d_offset;
  v.index = b->d_index;
  v.value = b->has_value ? b->d_value : nullptr;
  v.label = b->d_label;
  v.feaids = b->d_feaids;
  v.col_ptr = b->d_col_ptr;
  v.s_row = b->d_s_row;
  v.s_val = b->has_value ? b->d_s_val : nullptr;
  v.urow = b->d_urow;
  v.uw = nullptr;
  v.pred = b->d_pred;
  v.slope = b->d_slope;
  v.xv = b->d_xv;
  v.prog = b->d_prog;
  v.seg.mid = b->d_mid;
  v.seg.mid_ent = b->d_mid_ent;
  v.seg.hot = b->d_hot;
  v.seg.hot_ent = b->d_hot_ent;
  v.seg.few = b->d_few;
  v.seg.few_ent = b->d_few_ent;
  v.seg.split_ent = b->d_split_ent;
  v.seg.split_n = split_counter(b);   // the batch's device scalar block: [0] U, [1] REFRAND total, [2], [3] entries of the split list (SplitOut)
  return v;
}

int ensure_xv(dfh_batch* b, int kp) {
  size_t need = b->max_rows * (size_t)std::max(kp, 4);
  if (need <= b->xv_floats) return DFH_OK;
  if (b->d_xv) {
    int rc = sync_all(b->ctx);
    if (rc) return rc;
    DFH_HIP(hipFree(b->d_xv));
  }
  DFH_HIP(hipMalloc(&b->d_xv, need * sizeof(float)));
  b->xv_floats = need;
  return DFH_OK;
}

int launch_forward(dfh_batch* b, const RowSrc& src, int k, int kp, const uint2* uw = nullptr, const MixSrc* mix = nullptr,
                   bool riders = false) {
  BatchView bv = batch_view(b);
  bv.uw = uw;
  // one wave per example, all resident at once where possible: the kernel is
  // bound by the latency of its dependent gathers, not by launch size
  int grid = (int)std::max<size_t>(1, std::min<size_t>((b->nrows + 3) / 4, PROG_SLOTS));
  dfh_ctx* c = b->ctx;
  hipStream_t s = c->stream;
  const int fwd_depth = c->fwd_depth;
  if (c->fwd_blocks > 0) grid = std::min(grid, c->fwd_blocks);
  MixSrc mx{nullptr, 0};
  if (mix) mx = *mix;
  // single-queue step: the stages of later minibatches' Localizer that belong into a forward launch ride in this one
  RiderSet rs;
  rs.n = 0;
  if (riders && c->single_queue) collect_riders(c, 1, !mix && fwd_depth == 5, ((uint32_t)grid + 7u) / 8u, &rs);
  int rc = dispatch_L(kp, [&](auto Lc) {
    constexpr int L = decltype(Lc)::value;
    if (rs.n) {
      launch_k(c, DFH_K_FORWARD, k_forward_riders<L, 5>, dim3((((unsigned)grid + 7u) / 8u + rs.ngroups) * 8u), dim3(256),
               std::max<size_t>(rider_smem(rs), 4 * sizeof(double)), s, bv, src, k, kp, (uint32_t)grid, rs);
      return;
    }
    auto fwd = [&](auto kernel) { launch_k(c, DFH_K_FORWARD, kernel, dim3(grid), dim3(256), 0, s, bv, src, k, kp, mx); };
#define DFH_FWD(D) mix ? fwd(k_forward<L, D, true>) : fwd(k_forward<L, D, false>)
    switch (fwd_depth) {
      case 4: DFH_FWD(4); break;
      case 10: DFH_FWD(10); break;
      case 8: DFH_FWD(8); break;
      default: DFH_FWD(5); break;
    }
#undef DFH_FWD
  });
  if (rc) return rc;
  DFH_HIP(hipGetLastError());
  return DFH_OK;
}

// an AUC whose units have run (inside an update launch) but whose slots have not been added up yet
AucFin auc_pending(dfh_batch* b) { return AucFin{b->d_auc_part, b->auc_pending_n, b->d_prog + PROG_AUC * PROG_SLOTS}; }
int auc_flush_pending(dfh_batch* b) {
  if (!b->auc_pending_n) return DFH_OK;
  hipLaunchKernelGGL(k_auc_finalize, dim3(1), dim3(256), 0, b->ctx->stream, auc_pending(b));
  b->auc_pending_n = 0;
  DFH_HIP(hipGetLastError());
  return DFH_OK;
}

// BinClassMetric::AUC of the batch's predictions, accumulated into the progress block
int launch_auc(dfh_batch* b) {
  hipStream_t s = b->ctx->stream;
  const uint32_t n = (uint32_t)b->nrows;
  if (n <= AUC_PAIRS_MAX_N) {
    // minibatch-sized: pair counting (auc_pairs_block units), then one block adds the units' slots up
    int rc = auc_flush_pending(b);
    if (rc) return rc;
    hipLaunchKernelGGL(k_auc_pairs, dim3(auc_units(n)), dim3(256), 0, s, b->d_pred, b->d_label, n, b->d_auc_part);
    hipLaunchKernelGGL(k_auc_finalize, dim3(1), dim3(256), 0, s, AucFin{b->d_auc_part, n, b->d_prog + PROG_AUC * PROG_SLOTS});
    DFH_HIP(hipGetLastError());
    return DFH_OK;
  }
  hipLaunchKernelGGL(k_auc_keys, dim3(grid_for_threads(n, b->ctx)), dim3(256), 0, s, b->d_pred, b->d_label, n, b->d_auc_keys,
                     b->d_auc_lab);
  size_t tb = b->temp_bytes;
  // NB: d_temp is shared with the localizer's library-sort path, which only runs on the prep stream of
  // ANOTHER batch object; within one batch the step follows its own preparation
  DFH_HIP(rocprim::radix_sort_pairs(b->d_temp, tb, b->d_auc_keys, b->d_auc_skeys, b->d_auc_lab, b->d_auc_slab, (size_t)n, 0, 32, s));
  hipLaunchKernelGGL(k_auc_area, dim3(1), dim3(1024), 0, s, b->d_auc_slab, n, b->d_prog + PROG_AUC * PROG_SLOTS);
  DFH_HIP(hipGetLastError());
  return DFH_OK;
}

// argument block of k_update_fused for one localized minibatch
UpdArgs upd_args(dfh_batch* b, const TableView& tv, int k, int kp, uint32_t* need, const uint2* uw, KeyRange rg, bool add_cnt) {
  dfh_ctx* c = b->ctx;
  UpdArgs a;
  a.offset = b->d_offset;
  a.index = b->d_index;
  a.value = b->has_value ? b->d_value : nullptr;
  a.uw = uw;
  a.col_ptr = b->d_col_ptr;
  a.feaids = b->d_feaids;
  a.feacnt = (add_cnt && b->has_cnt) ? b->d_feacnt : nullptr;
  a.s_row = b->d_s_row;
  a.s_val = b->has_value ? b->d_s_val : nullptr;
  a.slope = b->d_slope;
  a.xv = b->d_xv;
  a.hdr = tv.hdr;
  a.va = tv.va;
  a.need_init = need;
  a.prog = b->d_prog;
  a.seg.mid = b->d_mid;
  a.seg.mid_ent = b->d_mid_ent;
  a.seg.hot = b->d_hot;
  a.seg.hot_ent = b->d_hot_ent;
  a.seg.few = b->d_few;
  a.seg.few_ent = b->d_few_ent;
  a.seg.split_ent = b->d_split_ent;
  a.seg.split_n = split_counter(b);   // (inside a step: the counter its listing launches filled; otherwise an empty one)
  a.split_part = b->d_split_part;
  a.split_ticket = b->d_split_ticket;
  a.nb_split = 0;
  a.nrows = (uint32_t)b->nrows;
  a.nlist = b->seg_nb;
  a.k = k;
  a.kp = kp;
  a.rg = rg;
  a.p = tv.p;
  a.ileave = (uint32_t)c->upd_interleave;
  a.nb_hot = a.nb_mid = a.nb_few = 0;
  a.auc_pred = nullptr;
  a.auc_label = nullptr;
  a.auc_part = nullptr;
  a.nb_auc = 0;
  a.rrows = nullptr;
  a.grows = nullptr;
  a.rstride = 0;
  return a;
}

// the fused update on the resident table (k_update_fused, dfh_update.hip): needs the {row | flags, w} words this
// step's k_lookup left per unique key
// rrows / grows (sharded store): the keys of other ranks (kRemoteRow in uw) read the rows their owners sent and leave
// gradient rows, in the same launch that updates this rank's own keys in place (k_update_fused<..., MIXED>)
int launch_update_fused(dfh_batch* b, const TableView& tv, int k, int kp, uint32_t* need, const uint2* uw, KeyRange rg, bool add_cnt,
                        bool with_auc = false, const float* rrows = nullptr, float* grows = nullptr, size_t rstride = 0,
                        bool riders = false) {
  dfh_ctx* c = b->ctx;
  hipStream_t s = c->stream;
  const int L = lanes_for(kp);
  UpdArgs a = upd_args(b, tv, k, kp, need, uw, rg, add_cnt);
  const bool mixed = rrows != nullptr && grows != nullptr;
  a.rrows = rrows;
  a.grows = grows;
  a.rstride = (uint32_t)rstride;
  if (with_auc) {  // the minibatch's AUC rides in this launch (dfh_sgd_step, compute_auc)
    a.auc_pred = b->d_pred;
    a.auc_label = b->d_label;
    int rcf = auc_flush_pending(b);  // the slots are about to be overwritten (normally closed by this step's k_lookup already)
    if (rcf) return rcf;
    a.auc_part = b->d_auc_part;
    a.nb_auc = (auc_units((uint32_t)b->nrows) + 7u) & ~7u;  // a multiple of 8: the roles behind keep their XCDs
    b->auc_pending_n = (uint32_t)b->nrows;  // finalised by the next launch that carries it (k_lookup of the next step, dfh_batch_progress)
  }
  // blocks per role (U and the list sizes live on the device; nnz bounds them): surplus blocks find their
  // list exhausted and leave at once
  const size_t nnz = b->nnz, G = 64 / (size_t)L;
  a.nb_hot = (uint32_t)std::max<size_t>(1, std::min<size_t>(nnz / (BWD_MID + 1) + 1, (size_t)c->upd_hot_blocks));
  a.nb_mid = (uint32_t)std::max<size_t>(1, std::min<size_t>((nnz / (BWD_SMALL + 1)) / UPD_NW + 1, (size_t)c->upd_mid_blocks));
  a.nb_few = (uint32_t)std::max<size_t>(1, std::min<size_t>((nnz / 2) / (UPD_NW * G) + 1, (size_t)c->upd_few_blocks));
  // singles block b on the XCD that ran the forward's block b (workgroups go round-robin over the 8 XCDs; the XV rows and
  // slopes of a block's four examples sit in that XCD's L2): the blocks before it add up to a multiple of 8.  (Measured in
  // round 4 by shifting the role 1 or 4 blocks: no difference, 86.0 against 85.9 M examples/sec — kept because it is free.)
  a.nb_few += (8u - (a.nb_hot + a.nb_mid + a.nb_few) % 8u) % 8u;
  // the parts of keys with more than HOT_SPLIT_MIN occurrences: taken by the hot role's blocks before their own lists
  a.nb_split = (b->split_listing && nnz > HOT_SPLIT_MIN) ? (uint32_t)b->split_cap : 0u;
  const size_t nb_single = std::max<size_t>(1, std::min<size_t>((b->nrows + UPD_NW - 1) / UPD_NW, (size_t)c->upd_single_blocks));
  const dim3 grid((unsigned)(a.nb_auc + a.nb_hot + a.nb_mid + a.nb_few + nb_single)), block(UPD_THREADS);
  // single-queue step: the stages of later minibatches' Localizer that belong into an update launch ride in this one
  RiderSet rs;
  rs.n = 0;
  if (riders && c->single_queue) collect_riders(c, 2, !mixed && UPD_THREADS == RID_THREADS, (grid.x + 7u) / 8u, &rs);
  const bool exact = kp == 4 * L, hv = b->has_value;
  int rc = dispatch_L(kp, [&](auto Lc) {
    constexpr int LL = decltype(Lc)::value;
    if (rs.n) {
      auto upd = [&](auto kernel) {
        launch_k(c, DFH_K_BACKWARD, kernel, dim3(((grid.x + 7u) / 8u + rs.ngroups) * 8u), block, std::max<size_t>(rider_smem(rs), UPD_SMEM), s,
                 a, grid.x, rs);
      };
#define DFH_UPD(EXACT, HV) upd(k_update_fused_riders<LL, EXACT, HV>)
      exact ? (hv ? DFH_UPD(true, true) : DFH_UPD(true, false)) : (hv ? DFH_UPD(false, true) : DFH_UPD(false, false));
#undef DFH_UPD
      return;
    }
    auto upd = [&](auto kernel) { launch_k(c, DFH_K_BACKWARD, kernel, grid, block, 0, s, a); };
#define DFH_UPD(EXACT, HV) (mixed ? upd(k_update_fused<LL, EXACT, HV, true>) : upd(k_update_fused<LL, EXACT, HV, false>))
    exact ? (hv ? DFH_UPD(true, true) : DFH_UPD(true, false)) : (hv ? DFH_UPD(false, true) : DFH_UPD(false, false));
#undef DFH_UPD
  });
  if (rc) return rc;
  DFH_HIP(hipGetLastError());
  return DFH_OK;
}

// with_auc: the minibatch's AUC rides in the launch — the caller has made sure that the launch is k_update_fused (step_math)
template <bool FUSED>
int launch_backward(dfh_batch* b, const RowSrc& src, const TableView& tv, float* grads, size_t gstride, int k, int kp,
                    uint32_t* need, KeyRange rg = kAllKeys, const uint2* uw = nullptr, bool add_cnt = false, bool with_auc = false,
                    bool riders = false) {
  if (FUSED && src.urow && uw && b->ctx->upd_kernel)
    return launch_update_fused(b, tv, k, kp, need, uw, rg, add_cnt, with_auc, nullptr, nullptr, 0, riders);
  if (riders) {  // no rider form of k_backward_all: the stages due in an update launch run alone
    RiderSet none;
    collect_riders(b->ctx, 2, false, 0, &none);
  }
  BatchView bv = batch_view(b);
  hipStream_t s = b->ctx->stream;
  const int L = lanes_for(kp);
  dfh_ctx* c = b->ctx;
  // U and the list sizes live on the device; nnz bounds them.  One launch of BWD_THREADS blocks:
  //   [0, nb_hot)            one hot key (> BWD_MID occurrences) per block and iteration
  //   [nb_hot, +nb_mid)      one mid key per wave and iteration
  //   the rest               short segments: (64/L) keys per wave and iteration, grid-stride
  // the long chains start first; surplus blocks find their list exhausted and leave at once
  constexpr size_t NWB = BWD_THREADS / 64;
  const size_t nb_hot = std::max<size_t>(1, std::min<size_t>(b->nnz / (BWD_MID + 1) + 1, 256));
#ifndef DFH_BWD_MID_BLOCKS
#define DFH_BWD_MID_BLOCKS 512
#endif
  const size_t nb_mid = std::max<size_t>(1, std::min<size_t>((b->nnz / (BWD_SMALL + 1)) / NWB + 1, DFH_BWD_MID_BLOCKS));
  const size_t small_cap = (size_t)c->bwd_small_blocks;
  const size_t keys_per_block = NWB * (64 / L);
  const size_t nb_small = std::max<size_t>(1, std::min<size_t>((b->nnz + keys_per_block - 1) / keys_per_block, small_cap));
  const dim3 grid((unsigned)(nb_hot + nb_mid + nb_small)), block(BWD_THREADS);
  const uint32_t nh = (uint32_t)nb_hot, nm = (uint32_t)nb_mid, nlist = b->seg_nb;
  int rc = dispatch_L(kp, [&](auto Lc) {
    constexpr int LL = decltype(Lc)::value;
    const bool lean = FUSED && src.urow;
    auto bwd = [&](auto kernel) {
      launch_k(c, DFH_K_BACKWARD, kernel, grid, block, 0, s, bv, src, tv, grads, gstride, k, kp, need, nh, nm, nlist, rg);
    };
    if (lean && kp == 4 * LL) bwd(k_backward_all<LL, FUSED, FUSED, true>);
    else if (lean) bwd(k_backward_all<LL, FUSED, FUSED, false>);
    else bwd(k_backward_all<LL, FUSED, false, false>);
  });
  if (rc) return rc;
  DFH_HIP(hipGetLastError());
  return DFH_OK;
}

// ---- The worker's two stages of a training step, each written once.  dfh_sgd_step is the schedule "every key is this
// rank's own" over them; flight_L and flight_F (dfh_shard.hip) are the sharded store's, for the slice of the minibatch's
// keys the rank owns, with the rows of the other owners beside it.

// Push(kFeaCount) of a step: 0 none, 1 by the lookup, 2 deferred — a training step's update kernel rewrites every key's
// header, so it takes the count push of the keys that have their V along (k_lookup then only reads them)
inline int count_mode(const dfh_ctx* c, int is_train, int push_cnt) { return push_cnt ? ((is_train && c->upd_kernel) ? 2 : 1) : 0; }

// what only the single-GPU schedule turns on: the sharded store refuses REFRAND tables, never resolves rows ahead of the
// step, carries no riders and times its stages (StageScope) rather than the launches inside them
struct StepExtras {
  uint32_t* need = nullptr;  // REFRAND: the rows to initialise in key order after the launch (refrand_flush)
  bool pre = false;          // the rows are resolved (dfh_batch_lookup on a preparation stream): no probe of the index
  bool riders = false;       // single-queue step: stages of later minibatches' Localizer may ride in the launches
  bool spans = false;        // the lookup and a separate AUC are timed like the ctx's other kernel classes
};

// Pull (key -> row) and, with push_cnt, Push(kFeaCount) (sgd_learner.cc:214-217) of keys [lo, lo + n) of the minibatch on
// this rank's table, and {row, w} per key into d_uw for the forward (w is current: the previous step's update precedes this
// launch on the stream), so that the forward touches nothing of a row but its V lines.  d_n: the count is *d_n (n bounds
// it for the grid).  With pre what remains is one pass over the known rows; the count push stays here because it must
// stay ordered with the previous step's update.  The pass that sees every unique key's segment also lists the parts of
// the very hot ones for the update's split role, and its first block adds up the AUC slots the batch object's previous
// step left behind.  rrows (overlap schedule): the rows of the other owners, U keys in all, complete at rows_in — the
// launch waits for them and writes the row words of the others' keys too (k_lookup_uw_remote: one launch boundary less).
int step_lookup(dfh_table* t, dfh_batch* b, int is_train, int push_cnt, uint32_t lo, const uint32_t* d_n, size_t n, const StepExtras& x,
                const float* rrows = nullptr, size_t U = 0, hipEvent_t rows_in = nullptr) {
  dfh_ctx* c = t->ctx;
  hipStream_t s = c->stream;
  const float* cnt = b->has_cnt ? b->d_feacnt + lo : (const float*)nullptr;
  const int mode = count_mode(c, is_train, push_cnt), gl = grid_for_threads(n, c);
  const uint32_t n_static = d_n ? 0u : (uint32_t)n;
  // DFH_GAP_TRACE=1 (measurement): the lookup dispatch carries its own start / stop events, like the forward and the update,
  // and dfh_ctx_get_timing prints the time between the end of one timed launch and the start of the next
  static const bool gap_trace = getenv("DFH_GAP_TRACE") != nullptr;
  const bool ride = x.spans && gap_trace && ((c->timing >> DFH_K_LOOKUP) & 1u);
  TimeScope ts(c, (x.spans && !ride) ? DFH_K_LOOKUP : DFH_K_COUNT);
  const SplitOut so = split_out(c, b, is_train, lo);
  RiderSet rs;
  rs.n = 0;
  if (x.riders) collect_riders(c, 0, true, ((uint32_t)gl + 7u) / 8u, &rs);
  if (rrows) {
    DFH_HIP(hipStreamWaitEvent(s, rows_in, 0));
    const UwRemote m{rrows, dfh_row_stride(t->v.k), b->d_U, lo, lo + (uint32_t)n, b->d_uw, b->d_col_ptr, split_out(c, b, is_train, 0u), t->v.err};
    hipLaunchKernelGGL(k_lookup_uw_remote, dim3(grid_for_threads(U, c)), dim3(256), 0, s, t->v, b->d_feaids + lo, n_static, b->d_urow + lo,
                       cnt, b->d_col_ptr + lo, mode, b->d_uw + lo, auc_pending(b), m, so);
  } else if (rs.n) {
    hipLaunchKernelGGL(k_lookup_riders, dim3((((unsigned)gl + 7u) / 8u + rs.ngroups) * 8u), dim3(256), rider_smem(rs), s, t->v,
                       b->d_feaids + lo, d_n, n_static, b->d_urow + lo, cnt, b->d_col_ptr + lo, mode, x.need, x.pre ? 1 : 0, b->d_uw + lo,
                       auc_pending(b), so, (uint32_t)gl, rs);
  } else {
    launch_span(c, ride, DFH_K_LOOKUP, 1, k_lookup_step, dim3(gl), dim3(256), 0, s, t->v, b->d_feaids + lo, d_n, n_static, b->d_urow + lo,
                cnt, b->d_col_ptr + lo, mode, x.need, x.pre ? 1 : 0, b->d_uw + lo, auc_pending(b), so);
  }
  b->auc_pending_n = 0;
  DFH_HIP(hipGetLastError());
  return DFH_OK;
}

// the keys of other ranks in the minibatch (sharded store): the rows their owners sent, the gradient rows that go back
struct StepRemote {
  const float* rows;  // row u belongs to key u of the minibatch; NULL: this minibatch has keys of this rank only
  float* grads;
  size_t stride;
};

// FMLoss::Predict, BinClassMetric::AUC of the minibatch (sgd_learner.cc:153-155), then EvaluatePenalty (a validation step)
// or CalcGrad and the update: the keys in `own` on the table in place; with rem, the others on the pulled rows — their
// part leaves gradient rows and comes first.  d_uw holds {row, w} of every key (step_lookup, k_uw_remote).  between(bool):
// called once the others' gradient rows are queued, told whether a launch for the own keys is still to come.
template <typename Between>
int step_math(dfh_table* t, dfh_batch* b, int is_train, int push_cnt, KeyRange own, const StepRemote* rem, const StepExtras& x,
              Between&& between) {
  dfh_ctx* c = t->ctx;
  hipStream_t s = c->stream;
  const int k = t->v.k, kp = t->v.kp;
  const bool any_own = b->nnz > 0 && own.hi > own.lo, any_remote = rem && rem->rows;
  const bool add_cnt = count_mode(c, is_train, push_cnt) == 2;
  // with keys of other ranks in the minibatch ONE launch of k_update_fused<MIXED> serves all keys — gradient rows for the
  // others' keys, the in-place update for the own ones (ctx option shard_mixed_update = 0: a launch each)
  const bool mixed = is_train && any_remote && c->upd_kernel != 0 && c->shard_mixed_update != 0;
  // the AUC rides in the update launch of a training step's own keys (k_update_fused: the pair counting is VALU work beside
  // a memory-bound kernel); where there is no such launch, or the minibatch is beyond the pair-counting size, it is a
  // launch of its own behind the forward
  const bool auc_rides = b->compute_auc && is_train && (any_own || mixed) && c->auc_in_update != 0 && c->upd_kernel != 0 &&
                         b->nrows <= AUC_PAIRS_MAX_N && UPD_THREADS == 256;
  const int pgrid = std::min(grid_for_waves(b->nnz, c), PROG_SLOTS);
  const RowSrc src = table_src(t, b->d_urow);
  RiderSet none;  // (stages of later minibatches due in a launch this step does not make: they run alone)
  // one rank: no MixSrc at all, the forward that reads the table only
  const MixSrc mix{any_remote ? rem->rows + 4 : nullptr, rem ? rem->stride : 0};
  int rc = launch_forward(b, src, k, kp, b->d_uw, rem ? &mix : nullptr, x.riders);
  if (rc) return rc;
  if (b->compute_auc && !auc_rides) {
    TimeScope ts(c, x.spans ? DFH_K_AUC : DFH_K_COUNT);
    rc = launch_auc(b);
    if (rc) return rc;
  }
  if (mixed) {
    rc = launch_update_fused(b, t->v, k, kp, b->d_need, b->d_uw, kAllKeys, add_cnt, auc_rides, rem->rows, rem->grads, rem->stride);
  } else if (any_remote && is_train) {  // the gradient-row launch reads every pulled row anyway: it adds up their penalty too
    rc = launch_backward<false>(b, packed_src(rem->rows, k), t->v, rem->grads, rem->stride, k, kp, nullptr, KeyRange{own.lo, own.hi, 3u});
  } else if (any_remote) {  // EvaluatePenalty over the pulled weights (sgd_learner.cc:249-273)
    hipLaunchKernelGGL((k_penalty<1>), dim3(pgrid), dim3(256), 0, s, batch_view(b), packed_src(rem->rows, k), t->v, k, kp,
                       KeyRange{own.lo, own.hi, 1u});
    DFH_HIP(hipGetLastError());
  }
  if (rc) return rc;
  if ((rc = between(!mixed))) return rc;
  if (mixed || !any_own) return DFH_OK;
  if (is_train)  // the fused in-place update accumulates the own keys' penalty itself
    return launch_backward<true>(b, src, t->v, nullptr, 0, k, kp, b->d_need, own, b->d_uw, add_cnt, auc_rides, x.riders);
  if (x.riders) collect_riders(c, 2, false, 0, &none);
  hipLaunchKernelGGL((k_penalty<1>), dim3(pgrid), dim3(256), 0, s, batch_view(b), src, t->v, k, kp, own);
  DFH_HIP(hipGetLastError());
  return DFH_OK;
}

}  // namespace

extern "C" {

// ------------------------------------------------------------ the fused step
int dfh_sgd_step(dfh_table* t, dfh_batch* b, int is_train, int push_cnt) {
  DFH_ARG(t && b, "dfh_sgd_step: NULL argument");
  DFH_ARG(t->ctx == b->ctx, "table and batch must share a context");
  if (!b->localized) {
    set_error("dfh_sgd_step: batch is not localized (call dfh_localize first)");
    return DFH_ERR_STATE;
  }
  if (is_train) {
    if (int rca = require_aux(t, "dfh_sgd_step(is_train)")) return rca;
  }
  dfh_ctx* c = t->ctx;
  DFH_HIP(hipSetDevice(c->device));
  hipStream_t s = c->stream;
  const int k = t->v.k, kp = t->v.kp;
  DFH_ARG(kp <= 256, "V_dim > 256 is not supported by the fused step");
  int rc = ensure_xv(b, kp);
  if (rc) return rc;
  b->nrows_seen += (float)b->nrows;
  RiderSet none;  // (stages of later minibatches due in a launch this step does not make: they run alone)
  if (b->nnz == 0) {
    // rows without features: pred = 0 for every example; nothing to pull or push
    RowSrc src = table_src(t, b->d_urow);
    rc = main_begin(b);
    if (rc) return rc;
    collect_riders(c, 0, false, 0, &none);
    rc = launch_forward(b, src, k, kp, nullptr, nullptr, true);
    if (rc) return rc;
    collect_riders(c, 2, false, 0, &none);
    return main_end(b);
  }
  const bool refrand = t->v.p.init_mode == DFH_INIT_REFRAND && k > 0;
  const uint32_t Nb = (uint32_t)b->nnz;  // upper bound of U for grids
  // every key is this rank's own; what dfh_batch_lookup resolved on a preparation stream is not probed again
  const StepExtras x{refrand ? b->d_need : nullptr, b->looked_up == t, true, true};
  if (!x.pre) {  // the step's own lookup probes the index: up to U <= nnz new keys
    rc = table_reserve(t, Nb);
    if (rc) return rc;
  }
  rc = main_begin(b);
  if (rc) return rc;
  rc = step_lookup(t, b, is_train, push_cnt, 0u, b->d_U, Nb, x);
  if (rc) return rc;
  if (push_cnt && refrand) {
    rc = refrand_flush(t, b->d_feaids, b->d_U, Nb, b->d_urow, b->d_need, b->d_rank, b->d_total);
    if (rc) return rc;
  }
  rc = step_math(t, b, is_train, push_cnt, kAllKeys, nullptr, x, [&](bool) -> int {
    if (is_train && refrand) DFH_HIP(hipMemsetAsync(b->d_need, 0, (size_t)Nb * 4, s));  // (the update flags the rows it wants initialised)
    return DFH_OK;
  });
  if (rc) return rc;
  if (is_train && refrand) {
    rc = refrand_flush(t, b->d_feaids, b->d_U, Nb, b->d_urow, b->d_need, b->d_rank, b->d_total);
    if (rc) return rc;
  }
  return main_end(b);
}

int dfh_batch_forward(dfh_batch* b, int V_dim, const float* d_rows) {
  DFH_ARG(b && b->localized && d_rows, "dfh_batch_forward: bad argument");
  const int kp = (V_dim + 3) / 4 * 4;
  int rc = ensure_xv(b, kp);
  if (rc) return rc;
  b->nrows_seen += (float)b->nrows;
  rc = main_begin(b);
  if (rc) return rc;
  rc = launch_forward(b, packed_src(d_rows, V_dim), V_dim, kp);
  if (rc) return rc;
  return main_end(b);  // a prediction-only step ends here; dfh_batch_backward moves the mark
}

int dfh_batch_backward(dfh_batch* b, int V_dim, const float* d_rows, float* d_grads) {
  DFH_ARG(b && b->localized && d_rows && d_grads, "dfh_batch_backward: bad argument");
  const int kp = (V_dim + 3) / 4 * 4;
  if (b->nnz == 0) return DFH_OK;
  TableView dummy{};
  int rc = launch_backward<false>(b, packed_src(d_rows, V_dim), dummy, d_grads, dfh_row_stride(V_dim), V_dim, kp, nullptr);
  if (rc) return rc;
  return main_end(b);
}

int dfh_auc_times_n(dfh_ctx* c, const float* label, const float* pred, size_t n, float* auc_n) {
  DFH_ARG(c && auc_n, "NULL argument");
  *auc_n = 1.0f;
  if (n == 0) return DFH_OK;
  DFH_ARG(label && pred && n < 0xFFFFFFF0ULL, "dfh_auc_times_n: bad argument");
  DFH_HIP(hipSetDevice(c->device));
  const bool pairs = n <= AUC_PAIRS_MAX_N;
  size_t tb = 0;
  if (!pairs)
    rocprim::radix_sort_pairs(nullptr, tb, (uint32_t*)nullptr, (uint32_t*)nullptr, (uint32_t*)nullptr, (uint32_t*)nullptr, n, 0, 32,
                              c->stream);
  int rc = ensure_scratch(c, 2 * padded<float>(n) + (pairs ? 0 : 4 * padded<uint32_t>(n)) + tb + padded<uint32_t>(AUC_PART_WORDS) + 2048);
  if (rc) return rc;
  Carver cv(c->scratch);
  float* d_l = cv.take<float>(n);
  float* d_p = cv.take<float>(n);
  double* d_o = cv.take<double>(1);
  uint32_t* d_part = cv.take<uint32_t>(AUC_PART_WORDS);
  hipStream_t s = c->stream;
  DFH_HIP(hipMemcpyAsync(d_l, label, n * 4, hipMemcpyHostToDevice, s));
  DFH_HIP(hipMemcpyAsync(d_p, pred, n * 4, hipMemcpyHostToDevice, s));
  DFH_HIP(hipMemsetAsync(d_o, 0, sizeof(double), s));
  if (pairs) {
    hipLaunchKernelGGL(k_auc_pairs, dim3(auc_units((uint32_t)n)), dim3(256), 0, s, d_p, d_l, (uint32_t)n, d_part);
    hipLaunchKernelGGL(k_auc_finalize, dim3(1), dim3(256), 0, s, AucFin{d_part, (uint32_t)n, d_o});
  } else {
    uint32_t* k0 = cv.take<uint32_t>(n);
    uint32_t* k1 = cv.take<uint32_t>(n);
    uint32_t* l0 = cv.take<uint32_t>(n);
    uint32_t* l1 = cv.take<uint32_t>(n);
    char* temp = cv.take<char>(tb + 16);
    hipLaunchKernelGGL(k_auc_keys, dim3(grid_for_threads(n, c)), dim3(256), 0, s, d_p, d_l, (uint32_t)n, k0, l0);
    DFH_HIP(rocprim::radix_sort_pairs(temp, tb, k0, k1, l0, l1, n, 0, 32, s));
    hipLaunchKernelGGL(k_auc_area, dim3(1), dim3(1024), 0, s, l1, (uint32_t)n, d_o);
  }
  DFH_HIP(hipGetLastError());
  double o = 0;
  DFH_HIP(hipMemcpyAsync(&o, d_o, sizeof(double), hipMemcpyDeviceToHost, s));
  DFH_HIP(hipStreamSynchronize(s));
  *auc_n = (float)o;
  return DFH_OK;
}

#ifdef DFH_BWD_TRACE
// measurement build only (tools/): {role, start, end} of every block of the last k_backward_all launch
int dfh_debug_bwd_trace(unsigned long long* out, size_t n) {
  DFH_HIP(hipDeviceSynchronize());
  DFH_HIP(hipMemcpyFromSymbol(out, HIP_SYMBOL(g_bwd_trace), std::min<size_t>(n, 3 * 8192) * sizeof(unsigned long long)));
  return DFH_OK;
}
#endif
}  // extern "C"
