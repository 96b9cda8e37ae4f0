// dfh_chunks.hip — the resident chunk set behind learner = lbfgs and learner = bcd (included in dfh_api.hip before
// dfh_lbfgs.hip and dfh_bcd.hip): how a reader block becomes a localized batch that stays in HBM, the merge of the
// chunks' feature counts into one ascending key list, and the map of a chunk's keys onto a model's keys.  Host code
// only.  Each learner keeps its own argument checks, its filter on the merged counts and its device layouts.
namespace dfh {
namespace chunks {

// one chunk: the Localizer's view of its rows (b) and the host copy of its ascending keys with their counts
struct Resident {
  dfh_batch* b = nullptr;
  size_t nrows = 0, nnz = 0, U = 0;
  std::vector<uint64_t> keys;
  std::vector<float> cnt;
};

// "<who>: <what> needs <need> bytes of HBM, <free> are free (<tail>)" and DFH_ERR_CAPACITY when need exceeds the free bytes
inline int check_free(const char* who, const char* what, const char* tail, size_t need) {
  size_t free_b = 0, total_b = 0;
  DFH_HIP(hipMemGetInfo(&free_b, &total_b));
  if (need > free_b) {
    char buf[256];
    snprintf(buf, sizeof(buf), "%s: %s needs %zu bytes of HBM, %zu are free (%s)", who, what, need, free_b, tail);
    set_error(buf);
    return DFH_ERR_CAPACITY;
  }
  return DFH_OK;
}

inline void release(Resident& r) {
  if (r.b) dfh_batch_destroy(r.b);
  r.b = nullptr;
}

// rows [0, nrows) of a reader block as a resident chunk: the batch object (after check_free of its bytes + extra_bytes,
// what the learner allocates per chunk later), the rows, Localizer(-1) and the host copy of keys and counts.  who
// ("dfh_lbfgs" / "dfh_bcd") and tail are check_free's; <who>_add_chunk prefixes the other message.  On failure nothing
// is kept and out->b stays NULL.
inline int add(dfh_ctx* c, const char* who, const char* tail, size_t extra_bytes, size_t nrows, const size_t* offset,
               const uint64_t* index, const float* value, const float* label, Resident* out) {
  const size_t nnz = offset[nrows] - offset[0];
  DFH_HIP(hipSetDevice(c->device));
  size_t need = 0;
  int rc = batch_create_impl(c, nrows, std::max<size_t>(nnz, 1), nullptr, nullptr, 0, &need, false);
  if (rc) return rc;
  rc = check_free(who, "a data chunk", tail, need + extra_bytes);
  if (rc) return rc;
  dfh_batch* b = nullptr;
  rc = dfh_batch_create(c, nrows, std::max<size_t>(nnz, 1), &b);
  if (rc) return rc;
  rc = dfh_batch_load_host(b, nrows, offset, index, value, label);
  if (!rc) rc = dfh_localize(b, ~0ULL);   // Localizer(-1): TileBuilder::Add, src/data/tile_builder.h:139-147
  size_t U = 0;
  std::vector<uint64_t> keys;
  std::vector<float> cnt;
  if (!rc) rc = dfh_batch_get_localized(b, &U, nullptr, nullptr, nullptr);
  if (!rc) {
    keys.resize(U);
    cnt.resize(U);
    if (U) rc = dfh_batch_get_localized(b, &U, keys.data(), cnt.data(), nullptr);
  }
  // the chunk is never loaded again: its page-locked staging copy of the rows (12 B per nnz) goes back to the host
  if (!rc && b->h_stage) {
    if (b->staged_pending) {
      if (hipEventSynchronize(b->ev_staged) != hipSuccess) rc = DFH_ERR_HIP;
      b->staged_pending = false;
    }
    if (!rc && hipHostFree(b->h_stage) != hipSuccess) rc = DFH_ERR_HIP;
    b->h_stage = nullptr;
    b->stage_bytes = 0;
    b->d_stage_view = nullptr;
    if (rc) set_error(std::string(who) + "_add_chunk: releasing the staging buffer failed");
  }
  if (rc) {
    dfh_batch_destroy(b);
    return rc;
  }
  out->b = b;
  out->nrows = nrows;
  out->nnz = nnz;
  out->U = U;
  out->keys = std::move(keys);
  out->cnt = std::move(cnt);
  return DFH_OK;
}

// KVUnion of the chunks' (key, count) pairs in chunk order (tile_builder.h:171-176): keys ascending, the counts of a
// key added up as floats in chunk order.  No filter: every learner applies its own to the result.
inline void merged_counts(const std::vector<const Resident*>& rs, std::vector<uint64_t>* keys, std::vector<float>* cnt) {
  size_t tot = 0;
  for (const Resident* r : rs) tot += r->U;
  std::vector<std::pair<uint64_t, float>> kc;
  kc.reserve(tot);
  for (const Resident* r : rs)
    for (size_t u = 0; u < r->U; ++u) kc.emplace_back(r->keys[u], r->cnt[u]);
  std::stable_sort(kc.begin(), kc.end(), [](const std::pair<uint64_t, float>& a, const std::pair<uint64_t, float>& b) {
    return a.first < b.first;
  });
  keys->clear();
  cnt->clear();
  for (size_t i = 0; i < kc.size();) {
    size_t j = i;
    float c = 0;
    for (; j < kc.size() && kc[j].first == kc[i].first; ++j) c += kc[j].second;
    keys->push_back(kc[i].first);
    cnt->push_back(c);
    i = j;
  }
}

// map [max(U, 1)]: the position of every chunk key among the ascending model keys, -1 = not in the model
// (TileBuilder::BuildColmap, tile_builder.h:59-76)
inline void colmap(const Resident& r, const std::vector<uint64_t>& model_keys, std::vector<int32_t>* map) {
  map->assign(std::max<size_t>(r.U, 1), -1);
  const size_t K = model_keys.size();
  size_t j = 0;
  for (size_t u = 0; u < r.U; ++u) {
    while (j < K && model_keys[j] < r.keys[u]) ++j;
    if (j < K && model_keys[j] == r.keys[u]) (*map)[u] = (int32_t)j;
  }
}

}  // namespace chunks
}  // namespace dfh
