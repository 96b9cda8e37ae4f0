// dfh_store_calls.hip — the owner-side store calls on device pointers (one shape: store_begin, the launch, launched), and
// the literal Store calls on host pointers that stage their arguments and call them.
namespace {
int make_segoff(const size_t* seg, int nsrc, int mask_slot, SegOff* out) {
  DFH_ARG(seg && nsrc >= 1 && nsrc <= 32, "seg must hold nsrc+1 offsets, 1 <= nsrc <= 32");
  DFH_ARG(mask_slot == 0 || mask_slot == 1, "mask_slot must be 0 or 1");
  out->slot = mask_slot;
  DFH_ARG(seg[0] == 0, "seg[0] must be 0");
  for (int s = 0; s <= nsrc; ++s) {
    DFH_ARG(seg[s] < (1ULL << 27) - 1 && (s == 0 || seg[s] >= seg[s - 1]), "seg must be ascending offsets below 2^27");
    out->off[s] = (uint32_t)seg[s];
  }
  out->nsrc = nsrc;
  return DFH_OK;
}
bool hash_init_only(const dfh_table* t) { return t->v.p.init_mode == DFH_INIT_HASH || t->v.k == 0; }
bool refrand_init(const dfh_table* t) { return t->v.p.init_mode == DFH_INIT_REFRAND && t->v.k > 0; }

// What an owner-side call asks of store_begin, which makes the checks in this one order (it decides which error a caller
// gets when two conditions fail at once): the table, and without seg the pointers; ST_AUX; ST_HASH; seg -> *g, *n and the
// pointers; n == 0 (the caller returns DFH_OK); ST_RESERVE; ST_REFRAND.
// ST_AUX: Push(kGradient), require_aux.  ST_HASH: works on row ids resolved earlier, V_init = hash only.  ST_RESERVE: may insert
// up to n keys, table_reserve.  ST_REFRAND: REFRAND tables get the need / rank / urow scratch (the caller ends with refrand_flush).
enum : unsigned { ST_AUX = 1, ST_HASH = 2, ST_RESERVE = 4, ST_REFRAND = 8 };
// ptrs: the call's device pointers are all there (they may be NULL when there are no keys).  seg: the `_multi` forms, all
// source ranks' keys in one array, n = seg[nsrc]
int store_begin(dfh_table* t, const char* who, bool ptrs, unsigned ask, size_t* n, const size_t* seg = nullptr, int nsrc = 0,
                int mask_slot = 0, SegOff* g = nullptr) {
  auto null_arg = [who] { return std::string(who) + ": NULL argument"; };
  if (g) DFH_ARG(t, "NULL table");
  else DFH_ARG(t && (*n == 0 || ptrs), null_arg());
  if (ask & ST_AUX) {
    if (int rca = require_aux(t, who)) return rca;
  }
  if ((ask & ST_HASH) && !hash_init_only(t)) {
    set_error(g ? "multi-source store calls need V_init = hash (order independent)"
                : "resolved store calls need V_init = hash (order independent)");
    return DFH_ERR_STATE;
  }
  if (g) {
    int rc = make_segoff(seg, nsrc, mask_slot, g);
    if (rc) return rc;
    *n = g->off[nsrc];
    DFH_ARG(*n == 0 || ptrs, null_arg());
  }
  if (*n == 0) return DFH_OK;
  if (ask & ST_RESERVE) {
    if (int rcr = table_reserve(t, *n)) return rcr;
  }
  if ((ask & ST_REFRAND) && refrand_init(t)) return ensure_table_aux(t, *n);
  return DFH_OK;
}
int launched() {
  DFH_HIP(hipGetLastError());
  return DFH_OK;
}
// blocks of a wave-per-row launch over n rows of L lanes each (8 / 32 blocks per CU: 61.0 / 58.6 against 57.4 us), or over
// nchunk chunks of MULTI_CH keys
unsigned store_blocks(const dfh_table* t, size_t blocks) { return (unsigned)std::min<size_t>(blocks, (size_t)t->ctx->num_cu * 16); }
unsigned store_blocks(const dfh_table* t, size_t n, int L) { return store_blocks(t, (n * L + 255) / 256); }
}  // namespace

extern "C" {

// ---- device-pointer (sharded) store calls
int dfh_shard_pull(dfh_table* t, const uint64_t* d_keys, size_t n, float* d_rows) {
  // Get inserts an entry for every id ever pulled (sgd_updater.cc:44)
  int rc = store_begin(t, "dfh_shard_pull", d_keys && d_rows, ST_RESERVE, &n);
  if (rc || n == 0) return rc;
  TimeScope ts(t->ctx, DFH_K_PULL);
  hipLaunchKernelGGL(k_pull_rows, dim3(grid_for_waves(n, t->ctx)), dim3(256), 0, t->ctx->stream, t->v, d_keys,
                     (uint32_t)n, d_rows, dfh_row_stride(t->v.k));
  return launched();
}

int dfh_shard_push_count(dfh_table* t, const uint64_t* d_keys, size_t n, const float* d_cnt) {
  int rc = store_begin(t, "dfh_shard_push_count", d_keys && d_cnt, ST_RESERVE | ST_REFRAND, &n);
  if (rc || n == 0) return rc;
  const bool refrand = refrand_init(t);
  hipLaunchKernelGGL(k_lookup, dim3(grid_for_threads(n, t->ctx)), dim3(256), 0, t->ctx->stream, t->v, d_keys,
                     (const uint32_t*)nullptr, (uint32_t)n, refrand ? t->d_urow : (uint32_t*)nullptr, d_cnt,
                     (const uint32_t*)nullptr, 1, refrand ? t->d_need : (uint32_t*)nullptr, 0, (uint2*)nullptr, AucFin{nullptr, 0u, nullptr});
  DFH_HIP(hipGetLastError());
  if (refrand) return refrand_flush(t, d_keys, nullptr, (uint32_t)n, t->d_urow, t->d_need, t->d_rank, t->d_total);
  return DFH_OK;
}

int dfh_shard_push_grad(dfh_table* t, const uint64_t* d_keys, size_t n, const float* d_grads) {
  int rc = store_begin(t, "dfh_shard_push_grad", d_keys && d_grads, ST_AUX | ST_RESERVE | ST_REFRAND, &n);
  if (rc || n == 0) return rc;
  const bool refrand = refrand_init(t);
  {
    TimeScope ts(t->ctx, DFH_K_PUSH);
    hipLaunchKernelGGL(k_push_grad, dim3(grid_for_waves(n, t->ctx)), dim3(256), 0, t->ctx->stream, t->v, d_keys,
                       (uint32_t)n, d_grads, dfh_row_stride(t->v.k), refrand ? t->d_need : (uint32_t*)nullptr,
                       refrand ? t->d_urow : (uint32_t*)nullptr);
  }
  DFH_HIP(hipGetLastError());
  if (refrand) return refrand_flush(t, d_keys, nullptr, (uint32_t)n, t->d_urow, t->d_need, t->d_rank, t->d_total);
  return DFH_OK;
}

// ---- resolved owner-side calls: probe once per step, then work on row ids
int dfh_shard_resolve(dfh_table* t, const uint64_t* d_keys, size_t n, uint32_t* d_rowid) {
  int rc = store_begin(t, "dfh_shard_resolve", d_keys && d_rowid, ST_RESERVE, &n);
  if (rc || n == 0) return rc;
  TimeScope ts(t->ctx, DFH_K_LOOKUP);
  hipLaunchKernelGGL(k_resolve, dim3(grid_for_threads(n, t->ctx)), dim3(256), 0, t->ctx->stream, t->v, d_keys, (uint32_t)n,
                     d_rowid);
  return launched();
}

int dfh_shard_pull_resolved(dfh_table* t, const uint32_t* d_rowid, size_t n, float* d_rows) {
  int rc = store_begin(t, "dfh_shard_pull_resolved", d_rowid && d_rows, 0, &n);
  if (rc || n == 0) return rc;
  TimeScope ts(t->ctx, DFH_K_PULL);
  const size_t stride = dfh_row_stride(t->v.k);
  rc = dispatch_L(std::max(t->v.kp, 4), [&](auto Lc) {
    constexpr int L = decltype(Lc)::value;
    hipLaunchKernelGGL((k_pull_resolved<L>), dim3(store_blocks(t, n, L)), dim3(256), 0, t->ctx->stream, t->v, d_rowid, (uint32_t)n,
                       d_rows, stride);
  });
  return rc ? rc : launched();
}

int dfh_shard_push_count_resolved(dfh_table* t, const uint32_t* d_rowid, const uint64_t* d_keys, size_t n, const float* d_cnt) {
  int rc = store_begin(t, "dfh_shard_push_count_resolved", d_rowid && d_keys && d_cnt, ST_HASH, &n);
  if (rc || n == 0) return rc;
  hipLaunchKernelGGL(k_lookup, dim3(grid_for_threads(n, t->ctx)), dim3(256), 0, t->ctx->stream, t->v, d_keys,
                     (const uint32_t*)nullptr, (uint32_t)n, const_cast<uint32_t*>(d_rowid), d_cnt, (const uint32_t*)nullptr, 1,
                     (uint32_t*)nullptr, 1, (uint2*)nullptr, AucFin{nullptr, 0u, nullptr});
  return launched();
}

int dfh_shard_push_grad_resolved(dfh_table* t, const uint32_t* d_rowid, const uint64_t* d_keys, size_t n, const float* d_grads) {
  int rc = store_begin(t, "dfh_shard_push_grad_resolved", d_rowid && d_keys && d_grads, ST_AUX | ST_HASH, &n);
  if (rc || n == 0) return rc;
  TimeScope ts(t->ctx, DFH_K_PUSH);
  const size_t stride = dfh_row_stride(t->v.k);
  rc = dispatch_L(std::max(t->v.kp, 4), [&](auto Lc) {
    constexpr int L = decltype(Lc)::value;
    hipLaunchKernelGGL((k_push_grad_resolved<L>), dim3(store_blocks(t, n, L)), dim3(256), 0, t->ctx->stream, t->v, d_rowid, d_keys,
                       (uint32_t)n, d_grads, stride);
  });
  return rc ? rc : launched();
}

// ---- all source ranks of a step in one launch per operation
int dfh_shard_resolve_multi(dfh_table* t, const uint64_t* d_keys, const size_t* seg, int nsrc, int mask_slot,
                            uint32_t* d_rowid) {
  SegOff g;
  size_t n = 0;
  int rc = store_begin(t, "dfh_shard_resolve_multi", d_keys && d_rowid, ST_RESERVE, &n, seg, nsrc, mask_slot, &g);
  if (rc || n == 0) return rc;
  TimeScope ts(t->ctx, DFH_K_LOOKUP);
  hipLaunchKernelGGL(k_resolve_multi, dim3(grid_for_threads(n, t->ctx)), dim3(256), 0, t->ctx->stream, t->v, d_keys, g, d_rowid);
  return launched();
}

int dfh_shard_push_count_multi(dfh_table* t, const uint32_t* d_rowid, const uint64_t* d_keys, const size_t* seg, int nsrc,
                               int mask_slot, const float* d_cnt) {
  SegOff g;
  size_t n = 0;
  int rc = store_begin(t, "dfh_shard_push_count_multi", d_rowid && d_keys && d_cnt, ST_HASH, &n, seg, nsrc, mask_slot, &g);
  if (rc || n == 0) return rc;
  TimeScope ts(t->ctx, DFH_K_LOOKUP);
  hipLaunchKernelGGL(k_push_count_multi, dim3(grid_for_threads(n, t->ctx)), dim3(256), 0, t->ctx->stream, t->v, d_rowid, d_keys, g,
                     d_cnt);
  return launched();
}

int dfh_shard_push_grad_multi(dfh_table* t, const uint32_t* d_rowid, const uint64_t* d_keys, const size_t* seg, int nsrc,
                              int mask_slot, const float* d_grads) {
  SegOff g;
  size_t n = 0;
  int rc = store_begin(t, "dfh_shard_push_grad_multi", d_rowid && d_keys && d_grads, ST_AUX | ST_HASH, &n, seg, nsrc, mask_slot, &g);
  if (rc || n == 0) return rc;
  TimeScope ts(t->ctx, DFH_K_PUSH);
  const size_t stride = dfh_row_stride(t->v.k);
  rc = dispatch_L(std::max(t->v.kp, 4), [&](auto Lc) {
    constexpr int L = decltype(Lc)::value;
    hipLaunchKernelGGL((k_push_grad_multi<L>), dim3(store_blocks(t, n, L)), dim3(256), 0, t->ctx->stream, t->v, d_rowid, d_keys, g,
                       d_grads, stride);
  });
  return rc ? rc : launched();
}

// Push(kFeaCount) of all sources (d_cnt, or NULL: none this step) and Pull, per distinct key, in one launch; leaves the key
// lists dfh_shard_push_grad_listed runs over
int dfh_shard_count_pull_multi(dfh_table* t, uint32_t* d_rowid, const uint64_t* d_keys, const size_t* seg, int nsrc, int mask_slot,
                               const float* d_cnt, float* d_rows) {
  SegOff g;
  size_t n = 0;
  int rc = store_begin(t, "dfh_shard_count_pull_multi", d_rowid && d_keys && d_rows, d_cnt ? ST_HASH : 0, &n, seg, nsrc, mask_slot, &g);
  if (rc || n == 0) return rc;
  TimeScope ts(t->ctx, DFH_K_PULL);
  const size_t stride = dfh_row_stride(t->v.k);
  const size_t nchunk = (n + MULTI_CH - 1) / MULTI_CH;
  rc = dispatch_L(std::max(t->v.kp, 4), [&](auto Lc) {
    constexpr int L = decltype(Lc)::value;
    const dim3 grid(store_blocks(t, nchunk));
    if (d_cnt)
      hipLaunchKernelGGL((k_count_pull_multi<L, true>), grid, dim3(256), 0, t->ctx->stream, t->v, d_rowid, d_keys, g, d_cnt, d_rows, stride);
    else
      hipLaunchKernelGGL((k_count_pull_multi<L, false>), grid, dim3(256), 0, t->ctx->stream, t->v, d_rowid, d_keys, g, d_cnt, d_rows, stride);
  });
  return rc ? rc : launched();
}

// Push(kGradient) of all sources over the key lists dfh_shard_count_pull_multi left in d_rowid (same seg, same slot)
int dfh_shard_push_grad_listed(dfh_table* t, const uint32_t* d_rowid, const uint64_t* d_keys, const size_t* seg, int nsrc,
                               int mask_slot, const float* d_grads) {
  SegOff g;
  size_t n = 0;
  int rc = store_begin(t, "dfh_shard_push_grad_listed", d_rowid && d_keys && d_grads, ST_AUX | ST_HASH, &n, seg, nsrc, mask_slot, &g);
  if (rc || n == 0) return rc;
  TimeScope ts(t->ctx, DFH_K_PUSH);
  const size_t stride = dfh_row_stride(t->v.k);
  const size_t nchunk = (n + MULTI_CH - 1) / MULTI_CH;
  rc = dispatch_L(std::max(t->v.kp, 4), [&](auto Lc) {
    constexpr int L = decltype(Lc)::value;
    hipLaunchKernelGGL((k_push_grad_chunks<L>), dim3(store_blocks(t, nchunk)), dim3(256), 0, t->ctx->stream, t->v, d_rowid, d_keys, g,
                       d_grads, stride);
  });
  return rc ? rc : launched();
}

size_t dfh_shard_multi_words(size_t n, int nsrc) { return multi_words(n, nsrc < 1 ? 1 : nsrc); }

int dfh_shard_release(dfh_table* t, const uint32_t* d_rowid, size_t n, int mask_slot) {
  DFH_ARG(t && (n == 0 || d_rowid), "dfh_shard_release: NULL argument");
  DFH_ARG(mask_slot == 0 || mask_slot == 1, "mask_slot must be 0 or 1");
  if (n == 0) return DFH_OK;
  hipLaunchKernelGGL(k_release_rows, dim3(grid_for_threads(n, t->ctx)), dim3(256), 0, t->ctx->stream, t->v, d_rowid, (uint32_t)n,
                     mask_slot);
  DFH_HIP(hipGetLastError());
  return DFH_OK;
}

// ---- literal Store API (host pointers)
namespace {
// the literal calls hand every key to its own lane: a key listed twice would be updated by two
// lanes at once (the reference applies them one after the other; the Localizer never produces them)
int check_keys(const uint64_t* keys, size_t n) {
  bool ascending = true;
  for (size_t i = 0; i < n; ++i) {
    DFH_ARG(keys[i] != kEmptyKey, "key ~0 is reserved");
    if (i && keys[i] <= keys[i - 1]) ascending = false;
  }
  if (ascending) return DFH_OK;  // Localizer output: strictly ascending, hence unique
  std::vector<uint64_t> tmp(keys, keys + n);
  std::sort(tmp.begin(), tmp.end());
  DFH_ARG(std::adjacent_find(tmp.begin(), tmp.end()) == tmp.end(), "duplicate key inside one push/pull");
  return DFH_OK;
}
}  // namespace

int dfh_pull(dfh_table* t, const uint64_t* keys, size_t n, float* vals, size_t* nvals, int* lens, size_t* nlens) {
  DFH_ARG(t && nvals && nlens && (n == 0 || (keys && vals && lens)), "dfh_pull: NULL argument");
  const int k = t->v.k;
  *nvals = 0;
  *nlens = k == 0 ? 0 : n;  // sgd_updater.cc:40
  if (n == 0) return DFH_OK;
  if (int rck = check_keys(keys, n)) return rck;
  dfh_ctx* c = t->ctx;
  DFH_HIP(hipSetDevice(c->device));
  const size_t stride = dfh_row_stride(k);
  int rc = ensure_scratch(c, padded<uint64_t>(n) + padded<float>(n * stride));
  if (rc) return rc;
  Carver cv(c->scratch);
  uint64_t* d_keys = cv.take<uint64_t>(n);
  float* d_rows = cv.take<float>(n * stride);
  DFH_HIP(hipMemcpyAsync(d_keys, keys, n * sizeof(uint64_t), hipMemcpyHostToDevice, c->stream));
  rc = dfh_shard_pull(t, d_keys, n, d_rows);
  if (rc) return rc;
  std::vector<float> rows(n * stride);
  DFH_HIP(hipMemcpyAsync(rows.data(), d_rows, rows.size() * sizeof(float), hipMemcpyDeviceToHost, c->stream));
  DFH_HIP(hipStreamSynchronize(c->stream));
  rc = check_table_err(t);
  if (rc) return rc;
  size_t p = 0;
  for (size_t i = 0; i < n; ++i) {  // ragged layout of SGDUpdater::Get (sgd_updater.cc:46-53)
    const float* r = rows.data() + i * stride;
    vals[p++] = r[0];
    if (r[1] != 0.0f) {
      memcpy(vals + p, r + 4, sizeof(float) * (size_t)k);
      p += (size_t)k;
      lens[i] = k + 1;
    } else if (k != 0) {
      lens[i] = 1;
    }
  }
  *nvals = p;
  return DFH_OK;
}

int dfh_push(dfh_table* t, const uint64_t* keys, size_t n, int val_type, const float* vals, size_t nvals,
             const int* lens, size_t nlens) {
  DFH_ARG(t && (n == 0 || keys), "dfh_push: NULL argument");
  DFH_ARG(val_type == DFH_FEA_COUNT || val_type == DFH_GRADIENT, "dfh_push: unknown val_type (sgd_updater.cc:99)");
  dfh_ctx* c = t->ctx;
  DFH_HIP(hipSetDevice(c->device));
  const int k = t->v.k;
  if (int rck = check_keys(keys, n)) return rck;
  if (val_type == DFH_FEA_COUNT) {
    DFH_ARG(nvals == n, "kFeaCount: CHECK_EQ(fea_ids.size(), values.size()) (sgd_updater.cc:63)");
    if (n == 0) return DFH_OK;
    int rc = ensure_scratch(c, padded<uint64_t>(n) + padded<float>(n));
    if (rc) return rc;
    Carver cv(c->scratch);
    uint64_t* d_keys = cv.take<uint64_t>(n);
    float* d_cnt = cv.take<float>(n);
    DFH_HIP(hipMemcpyAsync(d_keys, keys, n * sizeof(uint64_t), hipMemcpyHostToDevice, c->stream));
    DFH_HIP(hipMemcpyAsync(d_cnt, vals, n * sizeof(float), hipMemcpyHostToDevice, c->stream));
    rc = dfh_shard_push_count(t, d_keys, n, d_cnt);
    if (rc) return rc;
    return check_table_err(t);
  }
  // kGradient (sgd_updater.cc:74-97)
  if (int rca = require_aux(t, "dfh_push(kGradient)")) return rca;
  const bool w_only = nlens == 0;
  if (w_only) {
    DFH_ARG(nvals == n, "kGradient: CHECK_EQ(values.size(), size) (sgd_updater.cc:79)");
  } else {
    DFH_ARG(nlens == n && lens, "kGradient: CHECK_EQ(lens.size(), size) (sgd_updater.cc:81)");
  }
  if (n == 0) return DFH_OK;
  const size_t stride = dfh_row_stride(k);
  std::vector<float> rows(n * stride, 0.0f);
  size_t p = 0;
  for (size_t i = 0; i < n; ++i) {
    float* r = rows.data() + i * stride;
    DFH_ARG(p < nvals, "kGradient: values shorter than lens imply (sgd_updater.cc:96)");
    r[0] = vals[p++];
    if (!w_only && lens[i] > 1) {
      DFH_ARG(lens[i] == k + 1, "kGradient: CHECK_EQ(lens[i], V_dim+1) (sgd_updater.cc:91)");
      DFH_ARG(p + (size_t)k <= nvals, "kGradient: values shorter than lens imply (sgd_updater.cc:96)");
      r[1] = 1.0f;
      memcpy(r + 4, vals + p, sizeof(float) * (size_t)k);
      p += (size_t)k;
    }
  }
  DFH_ARG(p == nvals, "kGradient: CHECK_EQ(p, values.size()) (sgd_updater.cc:96)");
  int rc = ensure_scratch(c, padded<uint64_t>(n) + padded<float>(n * stride));
  if (rc) return rc;
  Carver cv(c->scratch);
  uint64_t* d_keys = cv.take<uint64_t>(n);
  float* d_rows = cv.take<float>(n * stride);
  DFH_HIP(hipMemcpyAsync(d_keys, keys, n * sizeof(uint64_t), hipMemcpyHostToDevice, c->stream));
  DFH_HIP(hipMemcpyAsync(d_rows, rows.data(), rows.size() * sizeof(float), hipMemcpyHostToDevice, c->stream));
  rc = dfh_shard_push_grad(t, d_keys, n, d_rows);
  if (rc) return rc;
  return check_table_err(t);
}
}  // extern "C"
