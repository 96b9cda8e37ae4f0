// dfh_table.hip — the model table: its error word, REFRAND scratch, growth (table_reserve before every launch that may
// insert), and the table calls: create .. check, export / import, model files.
namespace {
int check_table_err(dfh_table* t) {
  uint32_t e = 0;
  DFH_HIP(hipMemcpyAsync(&e, t->v.err, sizeof(e), hipMemcpyDeviceToHost, t->ctx->stream));
  DFH_HIP(hipStreamSynchronize(t->ctx->stream));
  if (e & 1u) {
    set_error("model table is full (capacity_rows exceeded)");
    return DFH_ERR_CAPACITY;
  }
  if (e & 2u) {
    set_error("a source's key list repeats a key (dfh_shard_resolve_multi: the lists must be unique, as a Localizer emits them)");
    return DFH_ERR_ARG;
  }
  if (e & 4u) {
    set_error("gradient carries V for a key whose V is not allocated (reference CHECK(e.V != nullptr))");
    return DFH_ERR_ARG;
  }
  if (e & 8u) {
    set_error("key index: a claimed slot never received its row id (find_or_insert gave up waiting)");
    return DFH_ERR_STATE;
  }
  if (e & 16u) {
    set_error("split list: a very hot key's parts did not fit (lookup_split; the list was not empty when the step began)");
    return DFH_ERR_STATE;
  }
  return DFH_OK;
}

int ensure_table_aux(dfh_table* t, size_t n) {
  if (n <= t->aux_cap) return DFH_OK;
  if (t->d_need) {
    DFH_HIP(hipStreamSynchronize(t->ctx->stream));
    DFH_HIP(hipFree(t->d_need));
    DFH_HIP(hipFree(t->d_rank));
    DFH_HIP(hipFree(t->d_urow));
  }
  size_t cap = std::max<size_t>(n, 1024);
  DFH_HIP(hipMalloc(&t->d_need, cap * sizeof(uint32_t)));
  DFH_HIP(hipMalloc(&t->d_rank, cap * sizeof(uint32_t)));
  DFH_HIP(hipMalloc(&t->d_urow, cap * sizeof(uint32_t)));
  t->aux_cap = cap;
  return DFH_OK;
}

// REFRAND: initialise the rows flagged in need[0..n) in key order, advance the chain
int refrand_flush(dfh_table* t, const uint64_t* d_keys, const uint32_t* d_n, uint32_t n_static, const uint32_t* d_urow,
                  const uint32_t* d_need, uint32_t* d_rank, uint32_t* d_total) {
  hipStream_t s = t->ctx->stream;
  TimeScope ts(t->ctx, DFH_K_MISC);
  hipLaunchKernelGGL(k_refrand_scan, dim3(1), dim3(1024), 0, s, d_need, d_n, n_static, d_rank, d_total);
  hipLaunchKernelGGL(k_refrand_init, dim3(grid_for_threads(n_static, t->ctx)), dim3(256), 0, s, t->v, d_keys, d_n,
                     n_static, d_urow, d_need, d_rank);
  hipLaunchKernelGGL(k_refrand_advance, dim3(1), dim3(64), 0, s, t->v, d_total);
  DFH_HIP(hipGetLastError());
  return DFH_OK;
}

// SGDUpdater::Update(kGradient) starts with CHECK(has_aux_) << "no aux data" (sgd_updater.cc:75)
int require_aux(const dfh_table* t, const char* who) {
  if (t->has_aux) return DFH_OK;
  set_error(std::string(who) + ": no aux data — the model was loaded without optimiser state (reference CHECK(has_aux_), "
                               "sgd_updater.cc:75)");
  return DFH_ERR_STATE;
}

// the largest pow2 index with load factor <= 0.5
inline uint64_t hslots_for(uint64_t capacity_rows) {
  uint64_t H = 1024;
  while (H < 2 * capacity_rows) H <<= 1;
  return H;
}

// re-allocate an auto-growing table at new_cap rows: row ids are stable (rows are handed out by a counter and never move
// inside hdr / va), so the two row arrays are copied as they are and only the key index is rebuilt.  Every stream of the
// context is drained first: no launch holds the old pointers.
int table_grow(dfh_table* t, uint64_t new_cap) {
  dfh_ctx* c = t->ctx;
  TableView& v = t->v;
  int rc = sync_all(c);
  if (rc) return rc;
  uint32_t nrows = 0;
  DFH_HIP(hipMemcpy(&nrows, v.nrows, sizeof(nrows), hipMemcpyDeviceToHost));
  nrows = std::min<uint32_t>(nrows, v.capacity);
  const uint64_t H = hslots_for(new_cap);
  const size_t ht_b = H * sizeof(HEntry), hdr_b = new_cap * sizeof(RowHdr);
  const size_t row_b = (size_t)(2 * v.kp) * sizeof(float);
  const size_t va_b = std::max<size_t>(new_cap * row_b, 256);
  HEntry* ht2 = nullptr;
  RowHdr* hdr2 = nullptr;
  float* va2 = nullptr;
  hipError_t e;
  if ((e = hipMalloc(&ht2, ht_b)) != hipSuccess || (e = hipMalloc(&hdr2, hdr_b)) != hipSuccess || (e = hipMalloc(&va2, va_b)) != hipSuccess) {
    if (ht2) (void)hipFree(ht2);
    if (hdr2) (void)hipFree(hdr2);
    if (va2) (void)hipFree(va2);
    (void)hipGetLastError();
    set_error("model table: cannot grow to " + std::to_string(new_cap) + " rows (" + hipGetErrorString(e) +
              "); set table capacity explicitly to what fits the HBM");
    return DFH_ERR_CAPACITY;
  }
  hipStream_t s = c->stream;
  DFH_HIP(hipMemsetAsync(ht2, 0xFF, ht_b, s));
  DFH_HIP(hipMemcpyAsync(hdr2, v.hdr, (size_t)nrows * sizeof(RowHdr), hipMemcpyDeviceToDevice, s));
  DFH_HIP(hipMemsetAsync(hdr2 + nrows, 0, hdr_b - (size_t)nrows * sizeof(RowHdr), s));
  if (row_b) {
    DFH_HIP(hipMemcpyAsync(va2, v.va, (size_t)nrows * row_b, hipMemcpyDeviceToDevice, s));
    DFH_HIP(hipMemsetAsync(reinterpret_cast<char*>(va2) + (size_t)nrows * row_b, 0, va_b - (size_t)nrows * row_b, s));
  } else {
    DFH_HIP(hipMemsetAsync(va2, 0, va_b, s));
  }
  hipLaunchKernelGGL(k_rehash, dim3(grid_for_threads(t->hslots, c)), dim3(256), 0, s, v.ht, t->hslots, ht2, H - 1);
  DFH_HIP(hipGetLastError());
  DFH_HIP(hipStreamSynchronize(s));
  DFH_HIP(hipFree(v.ht));
  DFH_HIP(hipFree(v.hdr));
  DFH_HIP(hipFree(v.va));
  v.ht = ht2;
  v.hdr = hdr2;
  v.va = va2;
  v.hmask = H - 1;
  v.capacity = (uint32_t)new_cap;
  t->hslots = H;
  t->bytes = ht_b + hdr_b + va_b;
  ++t->grows;
  return DFH_OK;
}

// before a launch that may insert up to n new keys into the index.  Tables of a fixed capacity: nothing (an overflow is
// flagged by the device and reported as DFH_ERR_CAPACITY).  Growing tables: keep rows_bound + n inside the capacity.
int table_reserve(dfh_table* t, uint64_t n) {
  if (!t->auto_grow) return DFH_OK;
  TableView& v = t->v;
  if (t->rows_bound + n <= v.capacity) {
    t->rows_bound += n;
    return DFH_OK;
  }
  // the bound is spent: read the true row count (one drain of the context's streams; rare, see the headroom below)
  int rc = sync_all(t->ctx);
  if (rc) return rc;
  uint32_t nrows = 0;
  DFH_HIP(hipMemcpy(&nrows, v.nrows, sizeof(nrows), hipMemcpyDeviceToHost));
  t->rows_bound = nrows;
  // grow when fewer than 32 launches of this size fit (at most 2^24 rows of slack for a bulk load): the drain above then
  // recurs every 32 launches at worst
  const uint64_t want = t->rows_bound + n + std::min<uint64_t>(31 * n, 1ull << 24);
  uint64_t cap = v.capacity;
  while (cap < (uint64_t)kRowMask && want > cap) cap = std::min<uint64_t>(2 * cap, (uint64_t)kRowMask);
  if (cap != v.capacity) {
    rc = table_grow(t, cap);
    if (rc == DFH_ERR_CAPACITY && t->rows_bound + n <= v.capacity) rc = DFH_OK;  // no room to grow yet, but this launch still fits
    if (rc == DFH_ERR_CAPACITY) {  // try the smallest capacity that holds this launch
      const uint64_t least = std::min<uint64_t>((uint64_t)kRowMask, t->rows_bound + 2 * n);
      if (least > v.capacity && least >= t->rows_bound + n) rc = table_grow(t, least);
    }
    if (rc) return rc;
  }
  if (t->rows_bound + n > v.capacity) {
    set_error("model table is full: " + std::to_string(t->rows_bound) + " rows + " + std::to_string(n) + " keys exceed 2^28 - 1 rows");
    return DFH_ERR_CAPACITY;
  }
  t->rows_bound += n;
  return DFH_OK;
}
}  // namespace

extern "C" {

// -------------------------------------------------------------------- table
int dfh_table_create(dfh_ctx* c, const dfh_updater_param* p, uint64_t capacity_rows, dfh_table** out) {
  DFH_ARG(c && p && out, "dfh_table_create: NULL argument");
  DFH_ARG(p->V_dim >= 0 && p->V_dim <= 10000, "V_dim out of range [0, 10000] (FMLossParam, fm_loss.h:25)");
  // the four top bits of a row word carry flags (kRemoteRow, kSingleRow, kCountLater, kHasV); 2^28 rows of V_dim 64 are 150 GB,
  // of V_dim 128 (C5: 1.25e8 rows per GPU) 296 GB: more than the HBM either way
  DFH_ARG(capacity_rows <= (uint64_t)kRowMask, "capacity_rows must be in [1, 2^28), or 0: a table that grows");
  const bool auto_grow = capacity_rows == 0;
  if (auto_grow) capacity_rows = (uint64_t)c->grow_initial_rows;  // the first allocation (2^20 rows: 0.6 GB at V_dim 64); doubled as the model grows
  DFH_ARG(p->lr > 0, "lr must be > 0");
  DFH_ARG(p->init_mode == DFH_INIT_HASH || p->init_mode == DFH_INIT_REFRAND, "bad init_mode");
  DFH_HIP(hipSetDevice(c->device));
  dfh_table* t = new (std::nothrow) dfh_table();
  DFH_ARG(t != nullptr, "out of host memory");
  t->ctx = c;
  t->auto_grow = auto_grow;
  TableView& v = t->v;
  v.p = *p;
  v.k = p->V_dim;
  v.kp = (p->V_dim + 3) / 4 * 4;
  v.capacity = (uint32_t)capacity_rows;
  const uint64_t H = hslots_for(capacity_rows);
  t->hslots = H;
  v.hmask = H - 1;
  size_t ht_b = H * sizeof(HEntry);
  size_t hdr_b = capacity_rows * sizeof(RowHdr);
  size_t va_b = std::max<size_t>(capacity_rows * (size_t)(2 * v.kp) * sizeof(float), 256);
  hipError_t e;
  if ((e = hipMalloc(&v.ht, ht_b)) != hipSuccess || (e = hipMalloc(&v.hdr, hdr_b)) != hipSuccess ||
      (e = hipMalloc(&v.va, va_b)) != hipSuccess || (e = hipMalloc(&v.nrows, 256)) != hipSuccess) {
    set_error(std::string("dfh_table_create: hipMalloc: ") + hipGetErrorString(e));
    if (v.ht) hipFree(v.ht);
    if (v.hdr) hipFree(v.hdr);
    if (v.va) hipFree(v.va);
    delete t;
    return DFH_ERR_HIP;
  }
  v.err = v.nrows + 1;
  v.rng_state = v.nrows + 2;
  t->d_total = v.nrows + 3;
  t->bytes = ht_b + hdr_b + va_b;
  DFH_HIP(hipMemsetAsync(v.ht, 0xFF, ht_b, c->stream));  // key = ~0 (empty), row = ~0
  DFH_HIP(hipMemsetAsync(v.hdr, 0, hdr_b, c->stream));
  DFH_HIP(hipMemsetAsync(v.va, 0, va_b, c->stream));
  DFH_HIP(hipMemsetAsync(v.nrows, 0, 256, c->stream));
  uint32_t seed = p->seed;
  DFH_HIP(hipMemcpyAsync(v.rng_state, &seed, sizeof(seed), hipMemcpyHostToDevice, c->stream));
  DFH_HIP(hipStreamSynchronize(c->stream));
  *out = t;
  return DFH_OK;
}

int dfh_table_destroy(dfh_table* t) {
  if (!t) return DFH_OK;
  hipSetDevice(t->ctx->device);
  sync_all(t->ctx);  // preparation streams may still probe the table
  hipFree(t->v.ht);
  hipFree(t->v.hdr);
  hipFree(t->v.va);
  hipFree(t->v.nrows);
  if (t->d_need) {
    hipFree(t->d_need);
    hipFree(t->d_rank);
    hipFree(t->d_urow);
  }
  delete t;
  return DFH_OK;
}

int dfh_table_size(dfh_table* t, uint64_t* nkeys) {
  DFH_ARG(t && nkeys, "NULL argument");
  uint32_t n = 0;
  {
    int rc = sync_all(t->ctx);  // a preparation-stream lookup may still be inserting keys
    if (rc) return rc;
  }
  DFH_HIP(hipMemcpyAsync(&n, t->v.nrows, sizeof(n), hipMemcpyDeviceToHost, t->ctx->stream));
  DFH_HIP(hipStreamSynchronize(t->ctx->stream));
  *nkeys = std::min<uint64_t>(n, t->v.capacity);
  return check_table_err(t);
}

int dfh_table_param(dfh_table* t, dfh_updater_param* out) {
  DFH_ARG(t && out, "NULL argument");
  *out = t->v.p;
  return DFH_OK;
}
uint64_t dfh_table_bytes(dfh_table* t) { return t ? t->bytes : 0; }

int dfh_table_capacity(dfh_table* t, uint64_t* capacity_rows, uint64_t* grows) {
  DFH_ARG(t, "NULL table");
  if (capacity_rows) *capacity_rows = t->v.capacity;
  if (grows) *grows = t->grows;
  return DFH_OK;
}

int dfh_table_set_has_aux(dfh_table* t, int has_aux) {
  DFH_ARG(t, "NULL table");
  t->has_aux = has_aux != 0;
  return DFH_OK;
}
int dfh_table_has_aux(dfh_table* t) { return (t && t->has_aux) ? 1 : 0; }

int dfh_table_warm_start(dfh_table* t, const uint64_t* d_keys, size_t n, float w0, float cnt0) {
  DFH_ARG(t && (n == 0 || d_keys), "dfh_table_warm_start: NULL argument");
  if (n == 0) return DFH_OK;
  if (int rcr = table_reserve(t, n)) return rcr;
  hipLaunchKernelGGL(k_warm_start, dim3(grid_for_waves(n, t->ctx)), dim3(256), 0, t->ctx->stream, t->v, d_keys,
                     (uint64_t)n, w0, cnt0);
  DFH_HIP(hipGetLastError());
  return DFH_OK;
}

int dfh_table_check(dfh_table* t) {
  DFH_ARG(t, "NULL table");
  return check_table_err(t);
}

int dfh_table_export(dfh_table* t, uint64_t cap, uint64_t* keys, float* scal, int* has_V, float* V, uint64_t* n) {
  DFH_ARG(t && n, "NULL argument");
  dfh_ctx* c = t->ctx;
  DFH_HIP(hipSetDevice(c->device));
  uint64_t cnt = 0;
  int rc = dfh_table_size(t, &cnt);
  if (rc) return rc;
  *n = cnt;
  if (cap == 0 || cnt == 0) return DFH_OK;
  DFH_ARG(cap >= cnt && keys && scal && has_V, "dfh_table_export: buffers too small");
  const int k = t->v.k;
  size_t vfl = (size_t)cnt * 2 * (size_t)std::max(k, 1);
  rc = ensure_scratch(c, padded<uint64_t>(cnt) + padded<float>(cnt * 4) + padded<int>(cnt) + padded<float>(vfl) + 512);
  if (rc) return rc;
  Carver cv(c->scratch);
  uint64_t* d_keys = cv.take<uint64_t>(cnt);
  float* d_scal = cv.take<float>(cnt * 4);
  int* d_has = cv.take<int>(cnt);
  float* d_V = cv.take<float>(vfl);
  unsigned long long* d_counter = cv.take<unsigned long long>(1);
  DFH_HIP(hipMemsetAsync(d_counter, 0, sizeof(unsigned long long), c->stream));
  hipLaunchKernelGGL(k_export, dim3(grid_for_threads(t->hslots, c)), dim3(256), 0, c->stream, t->v, t->hslots, cnt,
                     d_keys, d_scal, d_has, d_V, d_counter);
  DFH_HIP(hipGetLastError());
  DFH_HIP(hipMemcpyAsync(keys, d_keys, cnt * sizeof(uint64_t), hipMemcpyDeviceToHost, c->stream));
  DFH_HIP(hipMemcpyAsync(scal, d_scal, cnt * 4 * sizeof(float), hipMemcpyDeviceToHost, c->stream));
  DFH_HIP(hipMemcpyAsync(has_V, d_has, cnt * sizeof(int), hipMemcpyDeviceToHost, c->stream));
  if (k > 0 && V) DFH_HIP(hipMemcpyAsync(V, d_V, (size_t)cnt * 2 * k * sizeof(float), hipMemcpyDeviceToHost, c->stream));
  DFH_HIP(hipStreamSynchronize(c->stream));
  return DFH_OK;
}

int dfh_table_import(dfh_table* t, uint64_t n, const uint64_t* keys, const float* scal, const int* has_V, const float* V) {
  DFH_ARG(t && (n == 0 || (keys && scal && has_V)), "NULL argument");
  if (n == 0) return DFH_OK;
  dfh_ctx* c = t->ctx;
  DFH_HIP(hipSetDevice(c->device));
  const int k = t->v.k;
  DFH_ARG(k == 0 || V, "V is NULL");
  if (int rcr = table_reserve(t, n)) return rcr;
  size_t vfl = (size_t)n * 2 * (size_t)std::max(k, 1);
  int rc = ensure_scratch(c, padded<uint64_t>(n) + padded<float>(n * 4) + padded<int>(n) + padded<float>(vfl));
  if (rc) return rc;
  Carver cv(c->scratch);
  uint64_t* d_keys = cv.take<uint64_t>(n);
  float* d_scal = cv.take<float>(n * 4);
  int* d_has = cv.take<int>(n);
  float* d_V = cv.take<float>(vfl);
  DFH_HIP(hipMemcpyAsync(d_keys, keys, n * sizeof(uint64_t), hipMemcpyHostToDevice, c->stream));
  DFH_HIP(hipMemcpyAsync(d_scal, scal, n * 4 * sizeof(float), hipMemcpyHostToDevice, c->stream));
  DFH_HIP(hipMemcpyAsync(d_has, has_V, n * sizeof(int), hipMemcpyHostToDevice, c->stream));
  if (k > 0) DFH_HIP(hipMemcpyAsync(d_V, V, (size_t)n * 2 * k * sizeof(float), hipMemcpyHostToDevice, c->stream));
  hipLaunchKernelGGL(k_import, dim3(grid_for_threads(n, c)), dim3(256), 0, c->stream, t->v, n, d_keys, d_scal, d_has, d_V);
  DFH_HIP(hipGetLastError());
  return check_table_err(t);
}

// ---- model files (Updater::Save / Load, include/difacto/updater.h:40-47: stubs in the reference, so the
// format is ours and shared with the C++ host's DeviceSGDUpdater):
//   "DFHM", u32 version, i32 V_dim, i32 has_aux, u64 n, then n entries
//   {u64 key, f32 w, [f32 fea_cnt, sqrt_g, z if aux], i32 has_V, [V_dim f32 V, [V_dim f32 acc if aux]] if has_V}
int dfh_table_save(dfh_table* t, const char* path, int save_aux, uint64_t* n_saved) {
  DFH_ARG(t && path, "dfh_table_save: NULL argument");
  uint64_t n = 0;
  int rc = dfh_table_size(t, &n);
  if (rc) return rc;
  const int k = t->v.k;
  const size_t kk = (size_t)std::max(k, 1);
  const uint64_t cap = std::max<uint64_t>(n, 1);
  std::vector<uint64_t> keys(cap);
  std::vector<float> scal(cap * 4), V(cap * 2 * kk);
  std::vector<int> hasv(cap);
  uint64_t m = 0;
  rc = dfh_table_export(t, cap, keys.data(), scal.data(), hasv.data(), V.data(), &m);
  if (rc) return rc;
  FILE* f = fopen(path, "wb");
  if (!f) {
    set_error(std::string("dfh_table_save: cannot open ") + path);
    return DFH_ERR_ARG;
  }
  std::vector<char> iobuf(1 << 22);
  setvbuf(f, iobuf.data(), _IOFBF, iobuf.size());
  // entries with w == 0 and no V carry nothing a predictor needs: skipped unless aux is wanted
  uint64_t kept = 0;
  for (uint64_t i = 0; i < m; ++i) kept += (save_aux || scal[i * 4 + 1] != 0 || hasv[i]) ? 1 : 0;
  const uint32_t ver = 1;
  const int32_t kv = k, aux = save_aux ? 1 : 0;
  bool ok = fwrite("DFHM", 1, 4, f) == 4 && fwrite(&ver, 4, 1, f) == 1 && fwrite(&kv, 4, 1, f) == 1 &&
            fwrite(&aux, 4, 1, f) == 1 && fwrite(&kept, 8, 1, f) == 1;
  for (uint64_t i = 0; ok && i < m; ++i) {
    if (!(save_aux || scal[i * 4 + 1] != 0 || hasv[i])) continue;
    ok = ok && fwrite(&keys[i], 8, 1, f) == 1 && fwrite(&scal[i * 4 + 1], 4, 1, f) == 1;
    if (save_aux) {
      const float a3[3] = {scal[i * 4 + 0], scal[i * 4 + 2], scal[i * 4 + 3]};
      ok = ok && fwrite(a3, 4, 3, f) == 3;
    }
    const int32_t hv = hasv[i];
    ok = ok && fwrite(&hv, 4, 1, f) == 1;
    if (hv && k > 0) {
      ok = ok && fwrite(&V[i * 2 * k], 4, (size_t)k, f) == (size_t)k;
      if (save_aux) ok = ok && fwrite(&V[i * 2 * k + k], 4, (size_t)k, f) == (size_t)k;
    }
  }
  ok = (fclose(f) == 0) && ok;
  if (!ok) {
    set_error(std::string("dfh_table_save: write error on ") + path);
    return DFH_ERR_ARG;
  }
  if (n_saved) *n_saved = kept;
  return DFH_OK;
}

int dfh_table_load(dfh_table* t, const char* path, uint64_t key_lo, uint64_t key_hi, int* has_aux, uint64_t* n_loaded) {
  DFH_ARG(t && path, "dfh_table_load: NULL argument");
  FILE* f = fopen(path, "rb");
  if (!f) {
    set_error(std::string("dfh_table_load: cannot open ") + path);
    return DFH_ERR_ARG;
  }
  std::vector<char> iobuf(1 << 22);
  setvbuf(f, iobuf.data(), _IOFBF, iobuf.size());
  char magic[4];
  uint32_t ver = 0;
  int32_t k = 0, aux = 0;
  uint64_t n = 0;
  bool ok = fread(magic, 1, 4, f) == 4 && !memcmp(magic, "DFHM", 4) && fread(&ver, 4, 1, f) == 1 && fread(&k, 4, 1, f) == 1 &&
            fread(&aux, 4, 1, f) == 1 && fread(&n, 8, 1, f) == 1;
  if (!ok || k != t->v.k) {
    fclose(f);
    set_error(!ok ? "dfh_table_load: not a difacto-hip model file" : "dfh_table_load: model V_dim differs from the table's");
    return DFH_ERR_ARG;
  }
  if (has_aux) *has_aux = aux != 0;
  const size_t kk = (size_t)std::max(k, 1);
  const size_t chunk = 1 << 20;
  std::vector<uint64_t> keys;
  std::vector<float> scal, V, row(2 * kk);
  std::vector<int> hasv;
  uint64_t loaded = 0;
  int rc = DFH_OK;
  auto flush = [&]() -> int {
    if (keys.empty()) return DFH_OK;
    int r = dfh_table_import(t, keys.size(), keys.data(), scal.data(), hasv.data(), V.data());
    loaded += keys.size();
    keys.clear(); scal.clear(); V.clear(); hasv.clear();
    return r;
  };
  for (uint64_t i = 0; ok && rc == DFH_OK && i < n; ++i) {
    uint64_t key;
    float w, a3[3] = {0.f, 0.f, 0.f};
    int32_t hv;
    ok = fread(&key, 8, 1, f) == 1 && fread(&w, 4, 1, f) == 1;
    if (ok && aux) ok = fread(a3, 4, 3, f) == 3;
    ok = ok && fread(&hv, 4, 1, f) == 1;
    std::fill(row.begin(), row.end(), 0.f);
    if (ok && hv && k > 0) {
      ok = fread(row.data(), 4, (size_t)k, f) == (size_t)k;
      if (ok && aux) ok = fread(row.data() + k, 4, (size_t)k, f) == (size_t)k;
    }
    if (!ok) break;
    if (key < key_lo || (key_hi != 0 && key >= key_hi)) continue;  // another shard's key
    keys.push_back(key);
    scal.push_back(a3[0]); scal.push_back(w); scal.push_back(a3[1]); scal.push_back(a3[2]);
    hasv.push_back(hv);
    V.insert(V.end(), row.begin(), row.begin() + 2 * kk);
    if (keys.size() == chunk) rc = flush();
  }
  fclose(f);
  if (!ok) {
    set_error(std::string("dfh_table_load: truncated model file ") + path);
    return DFH_ERR_ARG;
  }
  if (rc == DFH_OK) rc = flush();
  if (n_loaded) *n_loaded = loaded;
  if (rc == DFH_OK && !aux && loaded > 0) t->has_aux = false;  // entries now lack fea_cnt / FTRL / AdaGrad state
  return rc;
}
}  // extern "C"
