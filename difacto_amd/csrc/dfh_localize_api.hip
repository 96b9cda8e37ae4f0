// dfh_localize_api.hip — Localizer::Compact of a loaded minibatch (localize_impl: sample sort or library sort, the feed's
// pending gather first) and the calls over it: dfh_localize, dfh_localize_lookup, dfh_batch_lookup.
namespace {
// Localizer::Compact of the loaded minibatch; with a table also the key-index probe of dfh_batch_lookup, done by the
// emit pass itself (the thread that writes a unique key looks it up: one launch and one event record fewer per minibatch)
int localize_impl(dfh_batch* b, uint64_t max_index, dfh_table* probe) {
  dfh_ctx* c = b->ctx;
  DFH_HIP(hipSetDevice(c->device));
  const uint32_t N = (uint32_t)b->nnz;
  if (probe && N) {
    if (int rcr = table_reserve(probe, N)) return rcr;  // before anything of this phase is queued: growth drains the streams
  }
  {
    int rc = prep_begin(b);
    if (rc) return rc;
  }
  hipStream_t s = prep_of(b);
  b->looked_up = nullptr;
  if (b->pend_stage < RID_STAGES) {  // localized twice without a step in between
    int rc = flush_pending(b);
    if (rc) return rc;
  }
  if (N == 0) {
    if (b->gather_pending) {  // rows without a single feature: their offsets and labels still have to arrive
      int rcg = gather_alone(b, s);
      if (rcg) return rcg;
    }
    // reference would index an empty vector (localizer.cc:35); define: no keys
    DFH_HIP(hipMemsetAsync(b->d_U, 0, 64 * sizeof(uint32_t), s));  // U = 0
    DFH_HIP(hipMemsetAsync(b->d_col_ptr, 0, 4, s));
    b->seg_nb = 0;  // no long segments
    b->view_P = 0;
    b->localized = true;
    return prep_end(b);
  }
  const int g = grid_for_threads(N, c);
  TimeScope* tsp = new TimeScope(c, DFH_K_LOCALIZE, s);
  // bucket count: the stored splitters' while the average bucket stays in a sane range (they
  // describe the data distribution, not this minibatch), else sized for this minibatch and
  // bootstrapped from a sample
  int P = 0;
  bool cold = true;
  if (b->spl_P > 0 && N / (uint32_t)b->spl_P >= (uint32_t)LOC_MIN_AVG && N / (uint32_t)b->spl_P <= (uint32_t)LOC_MAX_AVG) {
    P = b->spl_P;
    cold = false;
  } else {
    // the small size class (<= 1024 buckets, up to 700 pairs each) as long as it holds the minibatch, then the large one
    // (<= 4096 buckets: 2.9 M pairs); beyond that the library sort
    // small minibatches (the reference's batch-of-100 quick start) are a chain of launch latencies, not of bandwidth: half-size
    // buckets are one 64-run per wave and one merge round less in k_loc_sort (round 5, profiles/r05v_*)
#ifndef DFH_LOC_SMALL_AVG
#define DFH_LOC_SMALL_AVG 192
#endif
    const size_t avg_bucket = N <= 65536u ? (size_t)DFH_LOC_SMALL_AVG : (size_t)LOC_AVG_BUCKET;
    const size_t P_want = (N + avg_bucket - 1) / avg_bucket;
    if (P_want <= (size_t)LOC_MAX_BUCKETS) P = (int)std::max<size_t>(1, P_want);
    else if (N / LOC_MAX_BUCKETS <= (uint32_t)LOC_MAX_AVG) P = LOC_MAX_BUCKETS;
    else if (P_want <= (size_t)LOC_BIG_BUCKETS) P = (int)P_want;
    else if (N / LOC_BIG_BUCKETS <= (uint32_t)LOC_MAX_AVG) P = LOC_BIG_BUCKETS;
  }
  // a described minibatch (device feed): the count pass of the small size class gathers the rows itself; everywhere else —
  // a first call samples the raw ids before anything is counted, the large size class has no LDS to spare, the library sort
  // has no count pass, the single-queue step may run the count pass much later — the gather is queued here, first
  b->loc_fuse_gather = b->gather_pending && b->gather_fusable && !cold && P > 0 && P <= LOC_MAX_BUCKETS && !b->force_radix &&
                       !c->single_queue && !getenv("DFH_GATHER_ALONE");
  if (b->gather_pending && !b->loc_fuse_gather) {
    int rcg = gather_alone(b, s);
    if (rcg) return rcg;
  }
  if (P > 0 && !b->force_radix) {
    // hand-written sample sort (dfh_localize.hip)
    LocView& v = b->loc_v;
    v.raw = b->d_raw;
    v.n = N;
    v.max_index = max_index;
    v.P = P;
    const bool big = P > LOC_MAX_BUCKETS;
    v.bstride = big ? LOC_BIG_BUCKETS : LOC_MAX_BUCKETS;
    v.ntiles = (int)((N + LOC_TILE - 1) / LOC_TILE);
    v.force_global = b->force_sort_fallback ? 1 : 0;
    v.tb = N > 1 ? std::min(16, __builtin_clz(N - 1)) : 16;  // (N - 1) << tb fits 32 bits
    v.nrows = (uint32_t)b->nrows;
    v.offset = b->d_offset;
    v.rowid = b->d_pos;
    v.smp_key = b->d_smp_key;
    v.smp_pos = b->d_smp_pos;
    v.smp_rank = b->d_smp_rank;
    v.spl_key = b->d_spl_key;
    v.spl_pos = b->d_spl_pos;
    v.packed = b->d_packed;
    v.run_off = b->d_run_off;
    v.btotal = b->d_btotal;
    v.bstart = b->d_bstart;
    v.bkeys = b->d_keys;
    v.bpos = b->d_bpos;
    v.skeys = b->d_skeys;
    v.spos = b->d_spos;
    v.first_key = b->d_first_key;
    v.last_key = b->d_last_key;
    v.nheads = b->d_nheads;
    v.lh = b->d_lh;
    EmitOut& o = b->loc_o;
    o.value = b->has_value ? b->d_value : (const float*)nullptr;
    o.feaids = b->d_feaids;
    o.col_ptr = b->d_col_ptr;
    o.index = b->d_index;
    o.s_row = b->d_s_row;
    o.s_val = b->d_s_val;
    o.d_U = b->d_U;
    o.sl.mid = b->d_mid;
    o.sl.mid_ent = b->d_mid_ent;
    o.sl.hot = b->d_hot;
    o.sl.hot_ent = b->d_hot_ent;
    o.sl.few = b->d_few;
    o.sl.few_ent = b->d_few_ent;
    v.split_n = b->d_U + 2;
    b->loc_big = big;
#ifndef DFH_LOC_GRID_CAP
#define DFH_LOC_GRID_CAP 1024
#endif
    b->loc_gsort = (unsigned)std::min<int>(P, big ? LOC_BIG_BUCKETS : DFH_LOC_GRID_CAP);
    if (cold && P > 1) {
      const uint32_t S = (uint32_t)P * LOC_OVERSAMPLE;
      const uint32_t nt = (S + 255) / 256;
      hipLaunchKernelGGL(k_ss_sample, dim3(nt), dim3(256), 0, s, v);
      hipLaunchKernelGGL(k_ss_rank, dim3(nt * nt), dim3(256), 0, s, v);
      hipLaunchKernelGGL(k_loc_splitters, dim3(nt), dim3(256), 0, s, v);
    }
    // single-queue step: note the four stages; they ride in the launches of the steps that follow (dfh_riders.hip).  Not
    // for a first call (its splitters are being bootstrapped right here), the large size class (64 KB of LDS in count) or a
    // probe folded into emit
    if (c->single_queue && !cold && !big && !probe) {
      b->pend_stage = 0;
      c->pend.push_back(b);
    } else {
      for (int st = 0; st < RID_STAGES; ++st) {
        launch_loc_stage(b, st, s, probe);
        if (st == RID_COUNT && b->loc_fuse_gather) {  // the rows have been read once this launch is through
          int rcg = gather_queued(b, s);
          b->loc_fuse_gather = false;
          if (rcg) return rcg;
        }
      }
    }
    b->spl_P = P;  // k_loc_emit leaves this minibatch's exact P-quantiles as the next call's splitters
    b->seg_nb = (uint32_t)P;
    b->view_P = (uint32_t)P;
  } else {
    // very large batches: library LSD radix sort
    hipLaunchKernelGGL(k_rdx_keys, dim3(g), dim3(256), 0, s, b->d_raw, N, max_index, b->d_keys, b->d_pos);
    size_t tb = b->temp_bytes;
    DFH_HIP(rocprim::radix_sort_pairs(b->d_temp, tb, b->d_keys, b->d_skeys, b->d_pos, b->d_spos, (size_t)N, 0, 64, s));
    hipLaunchKernelGGL(k_rdx_heads, dim3(g), dim3(256), 0, s, b->d_skeys, N, b->d_head);
    tb = b->temp_bytes;
    DFH_HIP(rocprim::inclusive_scan(b->d_temp, tb, b->d_head, b->d_uid, (size_t)N, rocprim::plus<uint32_t>(), s));
    hipLaunchKernelGGL(k_rdx_emit, dim3(g), dim3(256), 0, s, b->d_skeys, b->d_spos, b->d_head, b->d_uid, N, (uint32_t)b->nrows,
                       b->d_offset, b->has_value ? b->d_value : (const float*)nullptr, b->d_feaids, b->d_col_ptr, b->d_index,
                       b->d_s_row, b->d_s_val, b->d_U);
    // keys with long segments, for the backward pass: one list bucket
    hipLaunchKernelGGL(k_seg_lists_reset, dim3(1), dim3(64), 0, s, b->d_mid, b->d_hot, b->d_few, b->d_U + 2);
    hipLaunchKernelGGL(k_seg_lists, dim3((unsigned)std::max<size_t>(1, std::min<size_t>((N + 1023) / 1024, 256))), dim3(1024), 0, s,
                       b->d_col_ptr, b->d_U, b->d_mid, b->d_hot, b->d_few, b->d_mid_ent, b->d_hot_ent, b->d_few_ent);
    b->seg_nb = 1;
    b->view_P = 0;
    if (probe)  // the library sort's path has no emit pass to carry the probe
      hipLaunchKernelGGL(k_lookup, dim3(grid_for_threads(b->nnz, c)), dim3(256), 0, s, probe->v, b->d_feaids, b->d_U, 0u, b->d_urow,
                         (const float*)nullptr, b->d_col_ptr, 0, (uint32_t*)nullptr, 0, (uint2*)nullptr, AucFin{nullptr, 0u, nullptr});
  }
  delete tsp;
  DFH_HIP(hipGetLastError());
  b->localized = true;
  b->has_cnt = false;
  if (probe) b->looked_up = probe;
  return prep_end(b);
}
}  // namespace

extern "C" {

int dfh_localize(dfh_batch* b, uint64_t max_index) {
  DFH_ARG(b && b->nrows > 0, "dfh_localize: no batch loaded");
  DFH_ARG(max_index != 0, "max_index must be nonzero");
  return localize_impl(b, max_index, nullptr);
}

int dfh_localize_lookup(dfh_table* t, dfh_batch* b, uint64_t max_index) {
  DFH_ARG(t && b && t->ctx == b->ctx, "dfh_localize_lookup: bad argument");
  DFH_ARG(b->nrows > 0, "dfh_localize_lookup: no batch loaded");
  DFH_ARG(max_index != 0, "max_index must be nonzero");
  return localize_impl(b, max_index, t);
}

int dfh_batch_lookup(dfh_table* t, dfh_batch* b) {
  DFH_ARG(t && b && t->ctx == b->ctx, "dfh_batch_lookup: bad argument");
  if (!b->localized) {
    set_error("dfh_batch_lookup: batch is not localized");
    return DFH_ERR_STATE;
  }
  dfh_ctx* c = b->ctx;
  if (b->nnz == 0) return DFH_OK;
  // A small minibatch is bound by the number of launches, not by what they move (C2, 7 500 pairs: the worker loop's step
  // takes exactly as long as the host needs to queue it): the step's own lookup pass probes in the launch it makes anyway.
  // 50.9 -> 44.8 us per step on the rcv1 shape (profiles/r05b_c2_launch_bound.txt).
  if (b->nnz <= kSmallBatchPairs) return DFH_OK;
  if (c->single_queue) return DFH_OK;  // no preparation stream to probe on: the step's own pass probes and pushes in one
  DFH_HIP(hipSetDevice(c->device));
  int rc = table_reserve(t, b->nnz);  // U <= nnz keys may be new
  if (rc) return rc;
  rc = prep_begin(b);
  if (rc) return rc;
  {
    hipStream_t ps = prep_of(b);
    TimeScope ts(c, DFH_K_LOOKUP, ps);
    hipLaunchKernelGGL(k_lookup, dim3(grid_for_threads(b->nnz, c)), dim3(256), 0, ps, t->v, b->d_feaids, b->d_U, 0u,
                       b->d_urow, (const float*)nullptr, b->d_col_ptr, 0, (uint32_t*)nullptr, 0, (uint2*)nullptr, AucFin{nullptr, 0u, nullptr});
  }
  DFH_HIP(hipGetLastError());
  b->looked_up = t;
  return prep_end(b);
}
}  // extern "C"
