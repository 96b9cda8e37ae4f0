// dfh_batch.hip — the batch object: its one arena, the load / attach calls (staging helpers: dfh_feed.hip), its options, and
// what is read back from it: shape, localized view, key ranges, key view, progress, predictions.
extern "C" {

// ------------------------------------------------------------------ batches
namespace {
// several batch objects carved from ONE device allocation (dfh_batch_create_many): the last one destroyed frees it
struct SharedArena {
  void* base = nullptr;
  int refs = 0;
};
}  // namespace

// shared != NULL: the object's arrays are carved at shared->base + at (sized by a first call with size_only = true)
static int batch_create_impl(dfh_ctx* c, size_t max_rows, size_t max_nnz, dfh_batch** out, SharedArena* shared, size_t at,
                             size_t* size_only, bool sync) {
  DFH_ARG(c && (out || size_only) && max_rows >= 1 && max_nnz >= 1, "dfh_batch_create: bad argument");
  DFH_ARG(max_nnz < 0xFFFFFFF0ULL && max_rows < 0xFFFFFFF0ULL, "batch too large for 32-bit positions");
  DFH_HIP(hipSetDevice(c->device));
  dfh_batch* b = new (std::nothrow) dfh_batch();
  DFH_ARG(b != nullptr, "out of host memory");
  b->ctx = c;
  b->max_rows = max_rows;
  b->max_nnz = max_nnz;
  const size_t N = max_nnz, B = max_rows;
  size_t sort_bytes = 0, scan_bytes = 0;
  rocprim::radix_sort_pairs(nullptr, sort_bytes, (uint64_t*)nullptr, (uint64_t*)nullptr, (uint32_t*)nullptr,
                            (uint32_t*)nullptr, N, 0, 64, c->stream);
  rocprim::inclusive_scan(nullptr, scan_bytes, (uint32_t*)nullptr, (uint32_t*)nullptr, N, rocprim::plus<uint32_t>(), c->stream);
  size_t auc_bytes = 0;
  rocprim::radix_sort_pairs(nullptr, auc_bytes, (uint32_t*)nullptr, (uint32_t*)nullptr, (uint32_t*)nullptr,
                            (uint32_t*)nullptr, B, 0, 32, c->stream);
  b->temp_bytes = std::max(std::max(sort_bytes, scan_bytes), auc_bytes) + 256;
  // ONE device allocation per batch object, carved below (256 B aligned pieces).  Until round 5 every array was its own
  // hipMalloc — 61 of them, ~40 us each: the worker loop's twelve objects cost a job ~35 ms of its ~65 ms start-up.  Two passes
  // over the same list: the first adds the sizes up, the second hands the pieces out.
  char* arena_at = nullptr;
  size_t arena_need = 0;
  bool sizing = true;
#define DFH_ALLOC(ptr, count, type)                                                        \
  do {                                                                                     \
    const size_t bytes__ = (((size_t)(count) * sizeof(type)) + 255) & ~(size_t)255;        \
    if (sizing) {                                                                          \
      arena_need += bytes__;                                                               \
    } else {                                                                               \
      (ptr) = reinterpret_cast<type*>(arena_at);                                           \
      arena_at += bytes__;                                                                 \
    }                                                                                      \
  } while (0)
  for (int pass = 0; pass < 2; ++pass) {
  sizing = pass == 0;
  if (!sizing) {
    if (size_only) {   // the caller only asked how much one object takes
      *size_only = arena_need;
      delete b;
      return DFH_OK;
    }
    if (shared) {
      b->shared_arena = shared;
      ++shared->refs;
      arena_at = static_cast<char*>(shared->base) + at;
    } else {
      hipError_t e__ = hipMalloc(reinterpret_cast<void**>(&b->arena), arena_need);
      if (e__ != hipSuccess) {
        set_error(std::string("dfh_batch_create: hipMalloc: ") + hipGetErrorString(e__));
        dfh_batch_destroy(b);
        return DFH_ERR_HIP;
      }
      arena_at = static_cast<char*>(b->arena);
    }
  }
  DFH_ALLOC(b->o_raw, N, uint64_t);
  DFH_ALLOC(b->o_offset, B + 1, uint32_t);
  DFH_ALLOC(b->o_value, N, float);
  DFH_ALLOC(b->o_label, B, float);
  b->d_raw = b->o_raw;
  b->d_offset = b->o_offset;
  b->d_value = b->o_value;
  b->d_label = b->o_label;
  DFH_ALLOC(b->d_keys, N, uint64_t);
  DFH_ALLOC(b->d_skeys, N, uint64_t);
  DFH_ALLOC(b->d_pos, N, uint32_t);
  DFH_ALLOC(b->d_spos, N, uint32_t);
  DFH_ALLOC(b->d_bpos, N, uint32_t);
  DFH_ALLOC(b->d_head, N, uint32_t);
  DFH_ALLOC(b->d_uid, N, uint32_t);
  DFH_ALLOC(b->d_temp, b->temp_bytes, char);
  b->max_tiles = (N + LOC_TILE - 1) / LOC_TILE;
  b->stage = StageLayout(max_rows, max_nnz, b->max_tiles);
  DFH_ALLOC(b->d_spl_key, LOC_BIG_BUCKETS, uint64_t);
  DFH_ALLOC(b->d_spl_pos, LOC_BIG_BUCKETS, uint32_t);
  DFH_ALLOC(b->d_smp_key, LOC_BIG_BUCKETS * LOC_OVERSAMPLE, uint64_t);
  DFH_ALLOC(b->d_smp_pos, LOC_BIG_BUCKETS * LOC_OVERSAMPLE, uint32_t);
  DFH_ALLOC(b->d_smp_rank, LOC_BIG_BUCKETS * LOC_OVERSAMPLE, uint32_t);
  DFH_ALLOC(b->d_first_key, LOC_BIG_BUCKETS, uint64_t);
  DFH_ALLOC(b->d_last_key, LOC_BIG_BUCKETS, uint64_t);
  DFH_ALLOC(b->d_packed, N, uint32_t);
  DFH_ALLOC(b->d_run_off, b->max_tiles * LOC_BIG_BUCKETS, uint32_t);
  DFH_ALLOC(b->d_bstart, LOC_BIG_BUCKETS + 1, uint32_t);
  DFH_ALLOC(b->d_btotal, LOC_XCDS * LOC_BIG_BUCKETS, uint32_t);
  DFH_ALLOC(b->d_nheads, LOC_BIG_BUCKETS, uint32_t);
  DFH_ALLOC(b->d_lh, LOC_BIG_BUCKETS, uint32_t);
  DFH_ALLOC(b->d_feaids, N, uint64_t);
  DFH_ALLOC(b->d_feacnt, N, float);
  DFH_ALLOC(b->d_col_ptr, N + 1, uint32_t);
  DFH_ALLOC(b->d_index, N, uint32_t);
  DFH_ALLOC(b->d_s_row, N, uint32_t);
  DFH_ALLOC(b->d_s_val, N, float);
  DFH_ALLOC(b->d_U, 64, uint32_t);
  DFH_ALLOC(b->d_urow, N, uint32_t);
  DFH_ALLOC(b->d_uw, N, uint2);
  // bucket q of the sample sort may list n_q / 2 + 2 few, n_q / (BWD_SMALL + 1) + 2 mid and n_q / (BWD_MID + 1) + 2 hot keys
  // (k_loc_emit: its slot range starts at beg_q / 2 + 2 q, beg_q / (BWD_SMALL + 1) + 2 q and beg_q / (BWD_MID + 1) + 2 q)
  b->mid_cap = N / (BWD_SMALL + 1) + 2 * LOC_BIG_BUCKETS + 16;
  b->hot_cap = N / (BWD_MID + 1) + 2 * LOC_BIG_BUCKETS + 16;
  b->few_cap = N / 2 + 2 * LOC_BIG_BUCKETS + 16;
  DFH_ALLOC(b->d_mid_ent, b->mid_cap, SegEnt);
  DFH_ALLOC(b->d_hot_ent, b->hot_cap, SegEnt);
  DFH_ALLOC(b->d_few_ent, b->few_cap, SegEnt);
  b->split_cap = 2 * (N / HOT_SPLIT) + 16;   // >= the sum over the segments longer than HOT_SPLIT_MIN of ceil(len / HOT_SPLIT)
  DFH_ALLOC(b->d_split_ent, b->split_cap, SegEnt);
  DFH_ALLOC(b->d_split_ticket, b->split_cap, uint32_t);
  DFH_ALLOC(b->d_split_part, b->split_cap * UPD_SPLIT_STRIDE, float);
  DFH_ALLOC(b->d_mid, LOC_BIG_BUCKETS, uint2);
  DFH_ALLOC(b->d_hot, LOC_BIG_BUCKETS, uint2);
  DFH_ALLOC(b->d_few, LOC_BIG_BUCKETS, uint2);
  DFH_ALLOC(b->d_need, N, uint32_t);
  DFH_ALLOC(b->d_rank, N, uint32_t);
  DFH_ALLOC(b->d_pred, B, float);
  DFH_ALLOC(b->d_slope, B, float);
  DFH_ALLOC(b->d_prog, dfh_batch::kProgDoubles, double);
  DFH_ALLOC(b->d_auc_keys, B, uint32_t);
  DFH_ALLOC(b->d_auc_skeys, B, uint32_t);
  DFH_ALLOC(b->d_auc_lab, B, uint32_t);
  DFH_ALLOC(b->d_auc_slab, B, uint32_t);
  DFH_ALLOC(b->d_auc_part, AUC_PART_WORDS, uint32_t);
  }  // sizing pass, carving pass
#undef DFH_ALLOC
  b->arena_bytes = arena_need;
  b->d_total = b->d_U + 1;
  // ev_ready / ev_free order streams of ONE device: no system-scope fence (cache write-back + invalidate) at the record
  const unsigned evf = hipEventDisableTiming | (c->event_flags ? hipEventDisableSystemFence : 0u);
  // (a failure from here on gives the object — and its reference on a shared arena — back: ADVICE r5)
  hipError_t e2 = hipEventCreateWithFlags(&b->ev_ready, evf);
  if (e2 == hipSuccess) e2 = hipEventCreateWithFlags(&b->ev_free, evf);
  if (e2 == hipSuccess) e2 = chunks::reset_prog(b, c->stream);
  if (e2 == hipSuccess) e2 = hipMemsetAsync(b->d_U, 0, 64 * sizeof(uint32_t), c->stream);
  // a key's ticket is back at zero when its last part has been applied (upd_split_role)
  if (e2 == hipSuccess) e2 = hipMemsetAsync(b->d_split_ticket, 0, b->split_cap * sizeof(uint32_t), c->stream);
  // k_loc_sort keeps the bucket totals zero between calls
  if (e2 == hipSuccess) e2 = hipMemsetAsync(b->d_btotal, 0, LOC_XCDS * LOC_BIG_BUCKETS * sizeof(uint32_t), c->stream);
  // row ids are written by the lookups of the keys a step resolves; anything else must never be used as one:
  // all-ones makes a stray use fault at once instead of reading some row
  if (e2 == hipSuccess) e2 = hipMemsetAsync(b->d_urow, 0xFF, N * sizeof(uint32_t), c->stream);
  if (e2 == hipSuccess) e2 = hipMemsetAsync(b->d_uw, 0xFF, N * sizeof(uint2), c->stream);
  if (e2 == hipSuccess && sync) e2 = hipStreamSynchronize(c->stream);
  if (e2 != hipSuccess) {
    set_error(std::string("dfh_batch_create: ") + hipGetErrorString(e2));
    dfh_batch_destroy(b);
    return DFH_ERR_HIP;
  }
  *out = b;
  return DFH_OK;
}

int dfh_batch_create(dfh_ctx* c, size_t max_rows, size_t max_nnz, dfh_batch** out) {
  return batch_create_impl(c, max_rows, max_nnz, out, nullptr, 0, nullptr, true);
}

int dfh_batch_create_many(dfh_ctx* c, int n, size_t max_rows, size_t max_nnz, dfh_batch** out) {
  DFH_ARG(c && out && n >= 1 && n <= 64, "dfh_batch_create_many: 1 <= n <= 64 objects");
  size_t each = 0;
  int rc = batch_create_impl(c, max_rows, max_nnz, nullptr, nullptr, 0, &each, false);
  if (rc) return rc;
  each = (each + 4095) & ~(size_t)4095;
  SharedArena* sa = new (std::nothrow) SharedArena();
  DFH_ARG(sa != nullptr, "out of host memory");
  DFH_HIP(hipSetDevice(c->device));
  if (hipMalloc(&sa->base, each * (size_t)n) != hipSuccess) {
    delete sa;
    set_error("dfh_batch_create_many: hipMalloc failed");
    return DFH_ERR_HIP;
  }
  for (int i = 0; i < n; ++i) out[i] = nullptr;
  sa->refs = 1;  // this call's own reference: the arena outlives every failure path below
  for (int i = 0; i < n && !rc; ++i) rc = batch_create_impl(c, max_rows, max_nnz, &out[i], sa, each * (size_t)i, nullptr, false);
  if (!rc && hipStreamSynchronize(c->stream) != hipSuccess) {   // the objects' memsets
    set_error("dfh_batch_create_many: hipStreamSynchronize failed");
    rc = DFH_ERR_HIP;
  }
  if (rc) {
    for (int j = 0; j < n; ++j) {
      if (out[j]) dfh_batch_destroy(out[j]);
      out[j] = nullptr;
    }
  }
  if (--sa->refs == 0) {  // no object holds it (every creation failed)
    hipFree(sa->base);
    delete sa;
  }
  return rc;
}

int dfh_batch_destroy(dfh_batch* b) {
  if (b && b->n_prof)
    fprintf(stderr, "dfh_batch_prepare_rows x %llu: begin %.4f s, wait staged %.4f, write description %.4f, gather %.4f, localize %.4f, lookup + ready %.4f\n",
            (unsigned long long)b->n_prof, b->t_prof[0], b->t_prof[1], b->t_prof[2], b->t_prof[3], b->t_prof[4], b->t_prof[5]);
  if (!b) return DFH_OK;
  hipSetDevice(b->ctx->device);
  pend_remove(b->ctx, b);  // stages noted but never queued die with the object
  sync_all(b->ctx);
  if (b->ev_ready) hipEventDestroy(b->ev_ready);
  if (b->ev_free) hipEventDestroy(b->ev_free);
  if (b->ev_staged) hipEventDestroy(b->ev_staged);
  if (b->h_stage) hipHostFree(b->h_stage);
  if (b->d_xv) hipFree(b->d_xv);      // (grows with V_dim: its own allocation, ensure_xv)
  if (b->arena) hipFree(b->arena);   // every other device array of the object
  if (b->shared_arena) {             // ... or its share of an allocation made for several objects
    SharedArena* sa = static_cast<SharedArena*>(b->shared_arena);
    if (--sa->refs == 0) {
      hipFree(sa->base);
      delete sa;
    }
  }
  delete b;
  return DFH_OK;
}

int dfh_batch_load_host(dfh_batch* b, size_t nrows, const size_t* offset, const uint64_t* index, const float* value,
                        const float* label) {
  DFH_ARG(b && offset && label, "dfh_batch_load_host: NULL argument");
  DFH_ARG(nrows >= 1 && nrows <= b->max_rows, "dfh_batch_load_host: nrows out of range");
  std::vector<uint32_t> off32;
  int rc = to_u32_offsets(offset, nrows, &off32);
  if (rc) return rc;
  const size_t base = offset[0], nnz = off32[nrows];
  DFH_ARG(nnz <= b->max_nnz, "dfh_batch_load_host: nnz exceeds max_nnz");
  DFH_ARG(nnz == 0 || index, "index is NULL");
  DFH_HIP(hipSetDevice(b->ctx->device));
  rc = phase_own_arrays(b);
  if (rc) return rc;
  hipStream_t s = prep_of(b);
  // Pinned staging: the caller's (pageable) arrays are copied into page-locked memory owned by the
  // batch object and sent with asynchronous copies on the preparation stream — the call returns as
  // soon as the bytes are staged, the caller may reuse its arrays, and with two batch objects used
  // alternately the transfer of minibatch t+1 overlaps the training of minibatch t.
  const StageLayout& L = b->stage;
  rc = ensure_stage(b, L.load_host_bytes, false);
  if (!rc) rc = stage_wait(b);
  if (rc) return rc;
  memcpy(b->h_stage + L.o_off, off32.data(), (nrows + 1) * 4);
  memcpy(b->h_stage + L.o_lab, label, nrows * 4);
  if (nnz) memcpy(b->h_stage + L.o_idx, index + base, nnz * 8);
  if (nnz && value) memcpy(b->h_stage + L.o_val, value + base, nnz * 4);
  DFH_HIP(hipMemcpyAsync(b->d_offset, b->h_stage + L.o_off, (nrows + 1) * 4, hipMemcpyHostToDevice, s));
  DFH_HIP(hipMemcpyAsync(b->d_label, b->h_stage + L.o_lab, nrows * 4, hipMemcpyHostToDevice, s));
  if (nnz) DFH_HIP(hipMemcpyAsync(b->d_raw, b->h_stage + L.o_idx, nnz * 8, hipMemcpyHostToDevice, s));
  if (nnz && value) DFH_HIP(hipMemcpyAsync(b->d_value, b->h_stage + L.o_val, nnz * 4, hipMemcpyHostToDevice, s));
  DFH_HIP(hipEventRecord(b->ev_staged, s));
  b->staged_pending = true;
  batch_loaded(b, nrows, nnz, value != nullptr);
  return DFH_OK;
}

int dfh_batch_load_device(dfh_batch* b, size_t nrows, size_t nnz, const uint32_t* d_offset, const uint64_t* d_index,
                          const float* d_value, const float* d_label) {
  DFH_ARG(b && d_offset && d_label && (nnz == 0 || d_index), "dfh_batch_load_device: NULL argument");
  DFH_ARG(nrows >= 1 && nrows <= b->max_rows && nnz <= b->max_nnz, "dfh_batch_load_device: shape out of range");
  int rc = phase_own_arrays(b);
  if (rc) return rc;
  hipStream_t s = prep_of(b);
  DFH_HIP(hipMemcpyAsync(b->d_offset, d_offset, (nrows + 1) * 4, hipMemcpyDeviceToDevice, s));
  if (nnz) DFH_HIP(hipMemcpyAsync(b->d_raw, d_index, nnz * 8, hipMemcpyDeviceToDevice, s));
  if (nnz && d_value) DFH_HIP(hipMemcpyAsync(b->d_value, d_value, nnz * 4, hipMemcpyDeviceToDevice, s));
  DFH_HIP(hipMemcpyAsync(b->d_label, d_label, nrows * 4, hipMemcpyDeviceToDevice, s));
  batch_loaded(b, nrows, nnz, d_value != nullptr);
  return DFH_OK;
}

int dfh_batch_attach_device(dfh_batch* b, size_t nrows, size_t nnz, const uint32_t* d_offset, const uint64_t* d_index,
                            const float* d_value, const float* d_label) {
  DFH_ARG(b && d_offset && d_label && (nnz == 0 || d_index), "dfh_batch_attach_device: NULL argument");
  DFH_ARG(nrows >= 1 && nrows <= b->max_rows && nnz <= b->max_nnz, "dfh_batch_attach_device: shape out of range");
  phase_begin(b);
  {
    int rc = prep_begin(b);  // a queued step may still read the previously attached memory; nothing of ours is overwritten
    if (rc) return rc;
  }
  b->d_offset = const_cast<uint32_t*>(d_offset);
  b->d_raw = const_cast<uint64_t*>(d_index);
  b->d_value = d_value ? const_cast<float*>(d_value) : b->o_value;
  b->d_label = const_cast<float*>(d_label);
  batch_loaded(b, nrows, nnz, d_value != nullptr);
  return DFH_OK;
}

int dfh_batch_set_option(dfh_batch* b, const char* name, int value) {
  DFH_ARG(b && name, "NULL argument");
  if (std::string(name) == "force_radix_sort") {
    b->force_radix = value != 0;
    return DFH_OK;
  }
  if (std::string(name) == "compute_auc") {
    b->compute_auc = value != 0;
    return DFH_OK;
  }
  if (std::string(name) == "force_sort_fallback") {
    b->force_sort_fallback = value != 0;
    return DFH_OK;
  }
  if (std::string(name) == "reset_splitters") {
    if (value) b->spl_P = 0;  // the next dfh_localize bootstraps its splitters from a sample again
    return DFH_OK;
  }
  set_error(std::string("unknown batch option ") + name);
  return DFH_ERR_ARG;
}

int dfh_batch_load_localized_host(dfh_batch* b, size_t nrows, const size_t* offset, const uint32_t* index, const float* value,
                                  const float* label, const uint64_t* feaids, const float* feacnt, size_t U) {
  DFH_ARG(b && offset && label && feaids, "dfh_batch_load_localized_host: NULL argument");
  DFH_ARG(nrows >= 1 && nrows <= b->max_rows, "nrows out of range");
  std::vector<uint32_t> off32;
  int rc = to_u32_offsets(offset, nrows, &off32);
  if (rc) return rc;
  const size_t base = offset[0], nnz = off32[nrows];
  DFH_ARG(nnz <= b->max_nnz && U <= b->max_nnz, "batch exceeds max_nnz");
  DFH_ARG(nnz == 0 || index, "index is NULL");
  for (size_t u = 0; u < U; ++u) {
    DFH_ARG(feaids[u] != kEmptyKey, "key ~0 is reserved");
    DFH_ARG(u == 0 || feaids[u] > feaids[u - 1], "feaids must be strictly ascending (Localizer output)");
  }
  // key-ordered occurrence view: stable counting sort of the nnz by compact index
  std::vector<uint32_t> col_ptr(U + 1, 0), s_row(std::max<size_t>(nnz, 1));
  std::vector<float> s_val(value ? std::max<size_t>(nnz, 1) : 0);
  for (size_t j = 0; j < nnz; ++j) {
    DFH_ARG(index[base + j] < U, "compact index out of range");
    ++col_ptr[index[base + j] + 1];
  }
  for (size_t u = 0; u < U; ++u) col_ptr[u + 1] += col_ptr[u];
  {
    std::vector<uint32_t> fill(col_ptr.begin(), col_ptr.end() - 1);
    for (size_t i = 0; i < nrows; ++i)
      for (uint32_t j = off32[i]; j < off32[i + 1]; ++j) {
        uint32_t q = fill[index[base + j]]++;
        s_row[q] = (uint32_t)i;
        if (value) s_val[q] = value[base + j];
      }
  }
  DFH_HIP(hipSetDevice(b->ctx->device));
  rc = phase_own_arrays(b);
  if (rc) return rc;
  hipStream_t s = prep_of(b);
  b->looked_up = nullptr;
  uint32_t U32 = (uint32_t)U;
  DFH_HIP(hipMemcpyAsync(b->d_offset, off32.data(), (nrows + 1) * 4, hipMemcpyHostToDevice, s));
  if (nnz) {
    DFH_HIP(hipMemcpyAsync(b->d_index, index + base, nnz * 4, hipMemcpyHostToDevice, s));
    DFH_HIP(hipMemcpyAsync(b->d_s_row, s_row.data(), nnz * 4, hipMemcpyHostToDevice, s));
    if (value) {
      DFH_HIP(hipMemcpyAsync(b->d_value, value + base, nnz * 4, hipMemcpyHostToDevice, s));
      DFH_HIP(hipMemcpyAsync(b->d_s_val, s_val.data(), nnz * 4, hipMemcpyHostToDevice, s));
    }
  }
  DFH_HIP(hipMemcpyAsync(b->d_label, label, nrows * 4, hipMemcpyHostToDevice, s));
  if (U) DFH_HIP(hipMemcpyAsync(b->d_feaids, feaids, U * 8, hipMemcpyHostToDevice, s));
  if (U && feacnt) DFH_HIP(hipMemcpyAsync(b->d_feacnt, feacnt, U * 4, hipMemcpyHostToDevice, s));
  DFH_HIP(hipMemcpyAsync(b->d_col_ptr, col_ptr.data(), (U + 1) * 4, hipMemcpyHostToDevice, s));
  DFH_HIP(hipMemcpyAsync(b->d_U, &U32, 4, hipMemcpyHostToDevice, s));
  hipLaunchKernelGGL(k_seg_lists_reset, dim3(1), dim3(64), 0, s, b->d_mid, b->d_hot, b->d_few, b->d_U + 2);
  if (U) {
    hipLaunchKernelGGL(k_seg_lists, dim3((unsigned)std::min<size_t>((U + 1023) / 1024, 256)), dim3(1024), 0, s, b->d_col_ptr,
                       b->d_U, b->d_mid, b->d_hot, b->d_few, b->d_mid_ent, b->d_hot_ent, b->d_few_ent);
  }
  b->seg_nb = 1;
  b->view_P = 0;
  DFH_HIP(hipGetLastError());
  DFH_HIP(hipStreamSynchronize(s));
  b->nrows = nrows;
  b->nnz = nnz;
  b->has_value = value != nullptr;
  b->has_cnt = feacnt != nullptr;
  b->localized = true;
  return prep_end(b);
}

int dfh_batch_shape(dfh_batch* b, size_t* nrows, size_t* nnz, size_t* U) {
  DFH_ARG(b, "NULL batch");
  if (nrows) *nrows = b->nrows;
  if (nnz) *nnz = b->nnz;
  if (U) {
    DFH_ARG(b->localized, "batch is not localized");
    uint32_t u = 0;
    int rc = flush_pending(b);
    if (rc) return rc;
    rc = sync_all(b->ctx);
    if (rc) return rc;
    DFH_HIP(hipMemcpyAsync(&u, b->d_U, 4, hipMemcpyDeviceToHost, b->ctx->stream));
    DFH_HIP(hipStreamSynchronize(b->ctx->stream));
    *U = u;
  }
  return DFH_OK;
}

int dfh_batch_get_localized(dfh_batch* b, size_t* U, uint64_t* feaids, float* feacnt, uint32_t* index) {
  DFH_ARG(b && b->localized, "batch is not localized");
  size_t u = 0;
  int rc = dfh_batch_shape(b, nullptr, nullptr, &u);
  if (rc) return rc;
  if (U) *U = u;
  hipStream_t s = b->ctx->stream;
  if (feaids && u) DFH_HIP(hipMemcpyAsync(feaids, b->d_feaids, u * 8, hipMemcpyDeviceToHost, s));
  if (feacnt && u) {
    if (!b->has_cnt) {
      hipLaunchKernelGGL(k_loc_counts, dim3(grid_for_threads(u, b->ctx)), dim3(256), 0, s, b->d_col_ptr, b->d_U, b->d_feacnt);
      DFH_HIP(hipGetLastError());
    }
    DFH_HIP(hipMemcpyAsync(feacnt, b->d_feacnt, u * 4, hipMemcpyDeviceToHost, s));
  }
  if (index && b->nnz) DFH_HIP(hipMemcpyAsync(index, b->d_index, b->nnz * 4, hipMemcpyDeviceToHost, s));
  DFH_HIP(hipStreamSynchronize(s));
  return DFH_OK;
}

int dfh_batch_device_keys(dfh_batch* b, const uint64_t** d_feaids, const float** d_feacnt, size_t* U) {
  DFH_ARG(b && b->localized, "batch is not localized");
  if (int rcf = flush_pending(b)) return rcf;  // the caller is about to read the arrays
  if (d_feaids) *d_feaids = b->d_feaids;
  if (d_feacnt) {
    if (!b->has_cnt) {
      // ordered after the batch's preparation, on the stream the consumers of the counts run on
      int rc = main_begin(b);
      if (rc) return rc;
      hipLaunchKernelGGL(k_loc_counts, dim3(grid_for_threads(b->nnz, b->ctx)), dim3(256), 0, b->ctx->stream, b->d_col_ptr,
                         b->d_U, b->d_feacnt);
      DFH_HIP(hipGetLastError());
      b->has_cnt = true;
    }
    *d_feacnt = b->d_feacnt;
  }
  if (U) return dfh_batch_shape(b, nullptr, nullptr, U);  // synchronises; pass NULL to stay asynchronous
  return DFH_OK;
}

int dfh_batch_key_ranges_device(dfh_batch* b, int nparts, const uint64_t* d_splits, int64_t* d_bounds) {
  DFH_ARG(b && b->localized && d_bounds && nparts >= 1 && nparts <= 1024, "dfh_batch_key_ranges_device: bad argument");
  dfh_ctx* c = b->ctx;
  int rc = main_begin(b);
  if (rc) return rc;
  const uint64_t span = nparts == 1 ? ~0ULL : (~0ULL / (uint64_t)nparts) + 1;
  hipLaunchKernelGGL(k_key_ranges64, dim3((nparts + 256) / 256), dim3(256), 0, c->stream, b->d_feaids, b->d_U, nparts, span,
                     d_splits, d_bounds, (uint32_t)(b->nnz == 0));
  DFH_HIP(hipGetLastError());
  return DFH_OK;
}

int dfh_batch_key_ranges(dfh_batch* b, int nparts, uint32_t* bounds) {
  DFH_ARG(b && b->localized && bounds && nparts >= 1 && nparts <= 1024, "dfh_batch_key_ranges: bad argument");
  dfh_ctx* c = b->ctx;
  int rc = ensure_scratch(c, (size_t)(nparts + 1) * 4 + 256);
  if (rc) return rc;
  uint32_t* d_bounds = static_cast<uint32_t*>(c->scratch);
  // span = ceil(2^64 / nparts): shard d owns keys in [d*span, (d+1)*span)
  const uint64_t span = nparts == 1 ? ~0ULL : (~0ULL / (uint64_t)nparts) + 1;
  hipStream_t s = prep_of(b);
  if (b->nnz == 0) {
    for (int d = 0; d <= nparts; ++d) bounds[d] = 0;
    return DFH_OK;
  }
  if (int rcf = flush_pending(b)) return rcf;
  hipLaunchKernelGGL(k_key_ranges, dim3((nparts + 256) / 256), dim3(256), 0, s, b->d_feaids, b->d_U, nparts, span, d_bounds);
  DFH_HIP(hipGetLastError());
  DFH_HIP(hipMemcpyAsync(bounds, d_bounds, (size_t)(nparts + 1) * 4, hipMemcpyDeviceToHost, s));
  DFH_HIP(hipStreamSynchronize(s));
  return DFH_OK;
}

int dfh_batch_split_entries(dfh_batch* b, uint32_t* n) {
  DFH_ARG(b && n, "dfh_batch_split_entries: NULL argument");
  dfh_ctx* c = b->ctx;
  DFH_HIP(hipSetDevice(c->device));
  if (b->pend_stage < RID_STAGES) {  // (single-queue step: Localizer stages still noted are queued first; they zero the counter)
    int rc = flush_pending(b);
    if (rc) return rc;
  }
  if (b->ready_pending) DFH_HIP(hipStreamWaitEvent(c->stream, b->ev_ready, 0));
  DFH_HIP(hipMemcpyAsync(n, b->d_U + 2 + b->split_last, sizeof(uint32_t), hipMemcpyDeviceToHost, c->stream));
  DFH_HIP(hipStreamSynchronize(c->stream));
  return DFH_OK;
}

namespace {
// what both key-view calls do first: everything queued for the batch has run (as dfh_batch_shape), U and the split counter read
int key_view_begin(dfh_batch* b, uint32_t* U, uint32_t* split_n) {
  dfh_ctx* c = b->ctx;
  DFH_HIP(hipSetDevice(c->device));
  int rc = flush_pending(b);
  if (rc) return rc;
  rc = sync_all(c);
  if (rc) return rc;
  DFH_HIP(hipMemcpy(U, b->d_U, sizeof(uint32_t), hipMemcpyDeviceToHost));
  DFH_HIP(hipMemcpy(split_n, b->d_U + 2 + b->split_last, sizeof(uint32_t), hipMemcpyDeviceToHost));
  if (*U > b->nnz) *U = (uint32_t)b->nnz;   // (never more keys than pairs: what is copied stays inside the arrays)
  return DFH_OK;
}
}  // namespace

int dfh_batch_key_view_info(dfh_batch* b, dfh_key_view_info* out) {
  DFH_ARG(b && out, "dfh_batch_key_view_info: NULL argument");
  if (!b->localized) {
    set_error("dfh_batch_key_view_info: batch is not localized");
    return DFH_ERR_STATE;
  }
  uint32_t U = 0, sn = 0;
  int rc = key_view_begin(b, &U, &sn);
  if (rc) return rc;
  out->U = U;
  out->nnz = b->nnz;
  out->has_value = b->has_value ? 1u : 0u;
  out->seg_nb = b->seg_nb;
  out->P = b->view_P;
  out->split_n = sn;
  out->few_cap = b->few_cap;
  out->mid_cap = b->mid_cap;
  out->hot_cap = b->hot_cap;
  out->split_cap = b->split_cap;
  out->bwd_small = BWD_SMALL;
  out->bwd_mid = BWD_MID;
  out->hot_split = HOT_SPLIT;
  out->hot_split_min = HOT_SPLIT_MIN;
  return DFH_OK;
}

int dfh_batch_get_key_view(dfh_batch* b, uint32_t* col_ptr, uint32_t* s_row, float* s_val, uint32_t* few_desc, uint32_t* few_ent,
                           uint32_t* mid_desc, uint32_t* mid_ent, uint32_t* hot_desc, uint32_t* hot_ent, uint32_t* split_ent,
                           uint32_t* bstart) {
  DFH_ARG(b, "dfh_batch_get_key_view: NULL batch");
  if (!b->localized) {
    set_error("dfh_batch_get_key_view: batch is not localized");
    return DFH_ERR_STATE;
  }
  uint32_t U = 0, sn = 0;
  int rc = key_view_begin(b, &U, &sn);
  if (rc) return rc;
  const size_t nnz = b->nnz, nb = b->seg_nb;
  if (col_ptr) DFH_HIP(hipMemcpy(col_ptr, b->d_col_ptr, ((size_t)U + 1) * 4, hipMemcpyDeviceToHost));
  if (s_row && nnz) DFH_HIP(hipMemcpy(s_row, b->d_s_row, nnz * 4, hipMemcpyDeviceToHost));
  if (s_val && nnz && b->has_value) DFH_HIP(hipMemcpy(s_val, b->d_s_val, nnz * 4, hipMemcpyDeviceToHost));
  if (few_desc && nb) DFH_HIP(hipMemcpy(few_desc, b->d_few, nb * sizeof(uint2), hipMemcpyDeviceToHost));
  if (mid_desc && nb) DFH_HIP(hipMemcpy(mid_desc, b->d_mid, nb * sizeof(uint2), hipMemcpyDeviceToHost));
  if (hot_desc && nb) DFH_HIP(hipMemcpy(hot_desc, b->d_hot, nb * sizeof(uint2), hipMemcpyDeviceToHost));
  if (few_ent) DFH_HIP(hipMemcpy(few_ent, b->d_few_ent, b->few_cap * sizeof(SegEnt), hipMemcpyDeviceToHost));
  if (mid_ent) DFH_HIP(hipMemcpy(mid_ent, b->d_mid_ent, b->mid_cap * sizeof(SegEnt), hipMemcpyDeviceToHost));
  if (hot_ent) DFH_HIP(hipMemcpy(hot_ent, b->d_hot_ent, b->hot_cap * sizeof(SegEnt), hipMemcpyDeviceToHost));
  const size_t ns = std::min<size_t>(sn, b->split_cap);
  if (split_ent && ns) DFH_HIP(hipMemcpy(split_ent, b->d_split_ent, ns * sizeof(SegEnt), hipMemcpyDeviceToHost));
  if (bstart && b->view_P) DFH_HIP(hipMemcpy(bstart, b->d_bstart, ((size_t)b->view_P + 1) * 4, hipMemcpyDeviceToHost));
  return DFH_OK;
}

int dfh_batch_progress(dfh_batch* b, dfh_progress* out, int reset) {
  DFH_ARG(b && out, "NULL argument");
  std::vector<double> p(2 * PROG_SLOTS + 1);
  hipStream_t s = b->ctx->stream;
  {
    int rc = auc_flush_pending(b);  // the last step's AUC slots, if no later step has added them up
    if (rc) return rc;
    rc = sync_all(b->ctx);
    if (rc) return rc;
  }
  DFH_HIP(hipMemcpyAsync(p.data(), b->d_prog, p.size() * sizeof(double), hipMemcpyDeviceToHost, s));
  DFH_HIP(hipStreamSynchronize(s));
  double loss = 0, pen = 0;
  for (int i = 0; i < PROG_SLOTS; ++i) {
    loss += p[PROG_LOSS * PROG_SLOTS + i];
    pen += p[PROG_PENALTY * PROG_SLOTS + i];
  }
  out->loss = (float)loss;
  out->penalty = (float)pen;
  out->auc = (float)p[PROG_AUC * PROG_SLOTS];
  out->nnz_w = 0;
  out->nrows = b->nrows_seen;
  if (reset) {
    DFH_HIP(chunks::reset_prog(b, s));
    b->nrows_seen = 0;
  }
  return DFH_OK;
}

int dfh_batch_get_pred(dfh_batch* b, float* pred) {
  DFH_ARG(b && pred, "NULL argument");
  hipStream_t s = b->ctx->stream;
  DFH_HIP(hipMemcpyAsync(pred, b->d_pred, b->nrows * 4, hipMemcpyDeviceToHost, s));
  DFH_HIP(hipStreamSynchronize(s));
  return DFH_OK;
}
}  // extern "C"
