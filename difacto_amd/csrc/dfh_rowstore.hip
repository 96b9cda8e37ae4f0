// dfh_rowstore.hip — the rows of a whole data set in HBM, one order over them, and the ragged gather that turns a range of that
// order into a row block (included in dfh_api.hip last: it uses the encoder of dfh_lz4enc.hip, the parsed chunks of
// dfh_textparse.hip and chunks::check_free's message).  task = convert with shuffle_rows / val_fraction appends every chunk
// of the input, fixes the order once and then encodes records of R rows out of it.
//
// Storage.  Ids live in slabs of slab_bytes (u64 [slab_bytes / 8]); a row never straddles two slabs and a row longer than a
// slab gets a slab of its own size.  A slab has a value array (f32, same positions) from the first append with values that
// touches it on; the array is born all 1.0f, so rows appended without values need nothing and a slab without the array reads
// as 1.0f.  A row is one 16-byte record {slab, position, length, label}; bit 31 of the length says that one of the row's values
// differs from 1.0f.  The records (and the weights) live in segments of slab_bytes / 16 rows, rounded down to a power of two.
// Growing the store is one more slab or segment: nothing that is stored is ever copied again.
//
// Order.  k_rs_keys writes key(r) = output r of splitmix64(seed) and r; rocprim's radix sort of the pairs over all 64 bits is
// stable, so equal keys keep ascending r: the order is ascending (key(r), r), numpy's stable argsort of the keys.
//
// Gathering rows order[first .. first + count):
//   k_rs_rows   a lane per row: the record -> label, weight, length (as u64), and the block's "a value differs" bit -> flag
//   scan        lengths -> the block's 64-bit offsets from 0 (count + 1 of them)
//   k_rs_copy   16 lanes per row (a wave holds 4 rows): a criteo row of 39 ids is 3 steps of 16 x 8 B = 128 contiguous bytes
//               on both sides, issued together before the first store; longer rows loop.  Every id and value is read once and
//               written once, by plain vector loads and stores.
// The host waits once, between scan and copy, for the block's nnz and flag: they size the destination.
struct dfh_rowstore {
  dfh_ctx* ctx = nullptr;
  hipStream_t s = nullptr;   // the context's parse stream: appends of parsed chunks are ordered behind nothing they need to wait for
  hipEvent_t ev = nullptr;
  std::mutex mu;             // append, order and read; encoders only read what order left
  size_t slab_elems = 0;
  uint32_t seg_shift = 0;    // a segment holds 1 << seg_shift rows
  std::vector<uint64_t*> slab_ids;
  std::vector<float*> slab_val;   // NULL: all 1.0f
  std::vector<size_t> slab_cap;   // elements
  size_t slab_used = 0;           // of the last slab
  std::vector<void*> seg_rows;
  std::vector<float*> seg_wgt;
  uint64_t nrows = 0, nnz = 0;
  bool has_value = false, has_weight = false, any_rows = false;
  size_t data_bytes = 0, order_bytes = 0;
  // what dfh_rowstore_order leaves
  void* d_tables = nullptr;   // slab_ids | slab_val | seg_rows | seg_wgt, pointers
  size_t n_slabs = 0, n_segs = 0;
  uint32_t* d_order = nullptr;
  size_t cap_order = 0;
  bool ordered = false;
  // dfh_rowstore_read's block
  char *d_rd_rows = nullptr, *d_rd_data = nullptr;
  size_t cap_rd_rows = 0, cap_rd_data = 0;
  uint64_t* h_head = nullptr;   // page-locked {nnz, flag}
};

namespace {
constexpr size_t RS_DEFAULT_SLAB = 64ull << 20;
constexpr uint64_t RS_MAX_ROWS = (1ull << 32) - 16;
constexpr uint32_t RS_LEN_MASK = 0x7FFFFFFFu, RS_VALUED = 0x80000000u;
constexpr uint32_t RS_GROUP = 16;   // lanes per row in k_rs_copy

struct RsRow { uint32_t slab, at, len; float label; };
static_assert(sizeof(RsRow) == 16, "a row record is one 16-byte load");

struct RsTables {
  const uint64_t* const* slab_ids;
  const float* const* slab_val;
  const RsRow* const* seg_rows;
  const float* const* seg_wgt;
  uint32_t seg_shift;
};

__device__ __forceinline__ RsRow rs_row(const RsTables& t, uint32_t r) {
  const uint4 v = *reinterpret_cast<const uint4*>(t.seg_rows[r >> t.seg_shift] + (r & ((1u << t.seg_shift) - 1u)));
  return RsRow{v.x, v.y, v.z, __uint_as_float(v.w)};
}

__global__ void __launch_bounds__(256) k_rs_iota(uint32_t* __restrict__ order, uint32_t n) {
  for (uint32_t r = blockIdx.x * 256u + threadIdx.x; r < n; r += gridDim.x * 256u) order[r] = r;
}

__global__ void __launch_bounds__(256) k_rs_keys(uint64_t* __restrict__ keys, uint32_t* __restrict__ rows, uint32_t n, uint64_t seed) {
  for (uint32_t r = blockIdx.x * 256u + threadIdx.x; r < n; r += gridDim.x * 256u) {
    uint64_t z = seed + ((uint64_t)r + 1ull) * 0x9E3779B97F4A7C15ull;
    z = (z ^ (z >> 30)) * 0xBF58476D1CE4E5B9ull;
    z = (z ^ (z >> 27)) * 0x94D049BB133111EBull;
    keys[r] = z ^ (z >> 31);
    rows[r] = r;
  }
}

// lens [count + 1] (the last one 0: the scan's total lands in off[count]); wgt_out NULL: the store carries no weights
__global__ void __launch_bounds__(256) k_rs_rows(const uint32_t* __restrict__ order, uint32_t count, RsTables t, float* __restrict__ label_out,
                                                 uint64_t* __restrict__ lens, float* __restrict__ wgt_out, uint32_t* __restrict__ flag) {
  bool valued = false;
  for (uint32_t i = blockIdx.x * 256u + threadIdx.x; i <= count; i += gridDim.x * 256u) {
    if (i == count) {
      lens[i] = 0ull;
      break;
    }
    const uint32_t r = order[i];
    const RsRow row = rs_row(t, r);
    label_out[i] = row.label;
    lens[i] = (uint64_t)(row.len & RS_LEN_MASK);
    valued |= (row.len & RS_VALUED) != 0u;
    if (wgt_out) wgt_out[i] = t.seg_wgt[r >> t.seg_shift][r & ((1u << t.seg_shift) - 1u)];
  }
  if (__any(valued) && (threadIdx.x & 63u) == 0u) atomicOr(flag, 1u);
}

// val_out NULL: the block's values are not wanted (the store has none, or all of the block's are 1.0f)
__global__ void __launch_bounds__(256) k_rs_copy(const uint32_t* __restrict__ order, uint32_t count, RsTables t, const uint64_t* __restrict__ off,
                                                 uint64_t* __restrict__ ids_out, float* __restrict__ val_out) {
  const uint32_t sub = threadIdx.x & (RS_GROUP - 1u);
  const uint32_t groups = gridDim.x * (256u / RS_GROUP);
  for (uint32_t i = (blockIdx.x * 256u + threadIdx.x) / RS_GROUP; i < count; i += groups) {
    const RsRow row = rs_row(t, order[i]);
    const uint32_t len = row.len & RS_LEN_MASK;
    const uint64_t* __restrict__ src = t.slab_ids[row.slab] + row.at;
    uint64_t* __restrict__ dst = ids_out + off[i];
    for (uint32_t j = sub; j < len; j += 4u * RS_GROUP) {   // four loads in flight per lane, then their stores
      const uint32_t j1 = j + RS_GROUP, j2 = j + 2u * RS_GROUP, j3 = j + 3u * RS_GROUP;
      const uint64_t a0 = src[j];
      const uint64_t a1 = j1 < len ? src[j1] : 0ull;
      const uint64_t a2 = j2 < len ? src[j2] : 0ull;
      const uint64_t a3 = j3 < len ? src[j3] : 0ull;
      dst[j] = a0;
      if (j1 < len) dst[j1] = a1;
      if (j2 < len) dst[j2] = a2;
      if (j3 < len) dst[j3] = a3;
    }
    if (val_out) {
      const float* vs = t.slab_val[row.slab];
      float* __restrict__ vd = val_out + off[i];
      if (vs) vs += row.at;
      for (uint32_t j = sub; j < len; j += 2u * RS_GROUP) {
        const uint32_t j1 = j + RS_GROUP;
        const float a0 = vs ? vs[j] : 1.0f;
        const float a1 = vs && j1 < len ? vs[j1] : 1.0f;
        vd[j] = a0;
        if (j1 < len) vd[j1] = a1;
      }
    }
  }
}

inline unsigned rs_grid(size_t threads) { return (unsigned)std::min<size_t>(std::max<size_t>((threads + 255) / 256, 1), 2048); }

int rs_wait(dfh_rowstore* st) {
  DFH_HIP(hipEventRecord(st->ev, st->s));
  DFH_HIP(hipEventSynchronize(st->ev));
  return DFH_OK;
}

// hipMalloc whose failure is the capacity message of the resident objects
int rs_alloc(dfh_rowstore* st, void** out, size_t bytes, const char* what) {
  *out = nullptr;
  if (hipMalloc(out, bytes) == hipSuccess) return DFH_OK;
  (void)hipGetLastError();
  *out = nullptr;
  size_t free_b = 0, total_b = 0;
  (void)hipMemGetInfo(&free_b, &total_b);
  char buf[320];
  snprintf(buf, sizeof(buf), "dfh_rowstore: %s needs %zu bytes of HBM, %zu are free (the store holds %zu bytes in %llu rows; an order over the "
           "whole input needs all of its rows in HBM)", what, bytes, free_b, st->data_bytes + st->order_bytes, (unsigned long long)st->nrows);
  set_error(buf);
  return DFH_ERR_CAPACITY;
}

struct RsRun { size_t slab, at, src, count; };   // `count` elements from the chunk's element `src` on go to slab[at ..]

// the append both sources share.  off[r] .. off[r + 1]: the chunk's elements of row r; ids/values are copied run by run with
// `kind` from ids + src (values + src); values NULL: none
template <typename Off>
int rs_append(dfh_rowstore* st, const char* who, size_t nrows, const Off* off, const float* label, const uint64_t* ids, hipMemcpyKind kind,
              const float* value, const float* weight) {
  if (nrows == 0) return DFH_OK;
  std::lock_guard<std::mutex> lk(st->mu);
  if (st->nrows + nrows >= RS_MAX_ROWS) {
    set_error(std::string(who) + ": a store holds fewer than 2^32 - 16 rows");
    return DFH_ERR_ARG;
  }
  if (st->any_rows && st->has_weight != (weight != nullptr)) {
    set_error(std::string(who) + ": a chunk " + (weight ? "with" : "without") + " weights behind chunks " + (weight ? "without" : "with") +
              " them: weights are carried only when every chunk has them");
    return DFH_ERR_ARG;
  }
  DFH_HIP(hipSetDevice(st->ctx->device));
  // where the rows go: into the last slab while they fit, then into new ones
  const size_t first0 = (size_t)off[0];
  std::vector<RsRow> recs(nrows);
  std::vector<RsRun> runs;
  std::vector<size_t> new_caps;
  size_t slab = st->slab_ids.size(), used = st->slab_used, cap = 0;
  if (slab) {
    --slab;
    cap = st->slab_cap[slab];
  }
  bool have = !st->slab_ids.empty();
  for (size_t r = 0; r < nrows; ++r) {
    if (off[r + 1] < off[r] || (size_t)(off[r + 1] - off[r]) > RS_LEN_MASK) {
      set_error(std::string(who) + ": offsets decrease, or a row has 2^31 ids or more");
      return DFH_ERR_ARG;
    }
    const size_t len = (size_t)(off[r + 1] - off[r]);
    if (!have || used + len > cap) {
      slab = st->slab_ids.size() + new_caps.size();
      cap = std::max(st->slab_elems, len);
      new_caps.push_back(cap);
      used = 0;
      have = true;
    }
    uint32_t bits = (uint32_t)len;
    if (value && kind == hipMemcpyHostToDevice) {
      const float* v = value + ((size_t)off[r] - first0);
      for (size_t j = 0; j < len; ++j)
        if (!(v[j] == 1.0f)) {
          bits |= RS_VALUED;
          break;
        }
    }
    recs[r] = RsRow{(uint32_t)slab, (uint32_t)used, bits, label[r]};
    if (len) {
      if (!runs.empty() && runs.back().slab == slab && runs.back().at + runs.back().count == used)
        runs.back().count += len;
      else
        runs.push_back(RsRun{slab, used, (size_t)off[r] - first0, len});
    }
    used += len;
  }
  // the new slabs, segments and value arrays; on failure the store is what it was
  const size_t seg_rows = (size_t)1 << st->seg_shift;
  const size_t segs_need = (size_t)((st->nrows + nrows + seg_rows - 1) >> st->seg_shift);
  std::vector<void*> fresh;
  size_t fresh_bytes = 0;
  auto undo = [&] {
    for (void* p : fresh) hipFree(p);
  };
  std::vector<uint64_t*> new_slabs;
  std::vector<void*> new_segs;
  std::vector<float*> new_wgts;
  std::vector<std::pair<size_t, float*>> new_vals;   // slab -> its value array
  int rc = DFH_OK;
  for (size_t k = 0; k < new_caps.size() && !rc; ++k) {
    void* p = nullptr;
    rc = rs_alloc(st, &p, std::max<size_t>(new_caps[k], 1) * sizeof(uint64_t), "a slab of ids");
    if (rc) break;
    fresh.push_back(p);
    fresh_bytes += std::max<size_t>(new_caps[k], 1) * sizeof(uint64_t);
    new_slabs.push_back(static_cast<uint64_t*>(p));
  }
  for (size_t k = st->seg_rows.size(); k < segs_need && !rc; ++k) {
    void* p = nullptr;
    rc = rs_alloc(st, &p, seg_rows * sizeof(RsRow), "a segment of row records");
    if (rc) break;
    fresh.push_back(p);
    fresh_bytes += seg_rows * sizeof(RsRow);
    new_segs.push_back(p);
    if (weight) {
      rc = rs_alloc(st, &p, seg_rows * sizeof(float), "a segment of weights");
      if (rc) break;
      fresh.push_back(p);
      fresh_bytes += seg_rows * sizeof(float);
      new_wgts.push_back(static_cast<float*>(p));
    }
  }
  auto cap_of = [&](size_t sl) { return sl < st->slab_cap.size() ? st->slab_cap[sl] : new_caps[sl - st->slab_cap.size()]; };
  if (value && !rc) {
    size_t last = ~(size_t)0;
    for (const RsRun& run : runs) {
      if (run.slab == last) continue;
      last = run.slab;
      if (run.slab < st->slab_val.size() && st->slab_val[run.slab]) continue;
      void* p = nullptr;
      const size_t elems = std::max<size_t>(cap_of(run.slab), 1);
      rc = rs_alloc(st, &p, elems * sizeof(float), "a slab of values");
      if (rc) break;
      fresh.push_back(p);
      fresh_bytes += elems * sizeof(float);
      new_vals.emplace_back(run.slab, static_cast<float*>(p));
      if (hipMemsetD32Async(reinterpret_cast<hipDeviceptr_t>(p), 0x3F800000, elems, st->s) != hipSuccess) {   // 1.0f
        set_error(std::string(who) + ": filling a slab of values failed");
        rc = DFH_ERR_HIP;
      }
    }
  }
  if (rc) {
    hipStreamSynchronize(st->s);
    undo();
    return rc;
  }
  auto ids_of = [&](size_t sl) { return sl < st->slab_ids.size() ? st->slab_ids[sl] : new_slabs[sl - st->slab_ids.size()]; };
  auto val_of = [&](size_t sl) -> float* {
    for (const auto& nv : new_vals)
      if (nv.first == sl) return nv.second;
    return st->slab_val[sl];
  };
  auto seg_of = [&](size_t k) { return k < st->seg_rows.size() ? st->seg_rows[k] : new_segs[k - st->seg_rows.size()]; };
  auto wgt_of = [&](size_t k) { return k < st->seg_wgt.size() ? st->seg_wgt[k] : new_wgts[k - st->seg_wgt.size()]; };
  hipError_t err = hipSuccess;
  for (size_t k = 0; k < runs.size() && err == hipSuccess; ++k) {
    const RsRun& run = runs[k];
    err = hipMemcpyAsync(ids_of(run.slab) + run.at, ids + run.src, run.count * sizeof(uint64_t), kind, st->s);
    if (value && err == hipSuccess) err = hipMemcpyAsync(val_of(run.slab) + run.at, value + run.src, run.count * sizeof(float), kind, st->s);
  }
  for (size_t r = 0; r < nrows && err == hipSuccess;) {   // the records (and weights), segment by segment
    const size_t g = st->nrows + r, k = g >> st->seg_shift, in = g & (seg_rows - 1), cnt = std::min(nrows - r, seg_rows - in);
    err = hipMemcpyAsync(static_cast<RsRow*>(seg_of(k)) + in, recs.data() + r, cnt * sizeof(RsRow), hipMemcpyHostToDevice, st->s);
    if (weight && err == hipSuccess) err = hipMemcpyAsync(wgt_of(k) + in, weight + r, cnt * sizeof(float), hipMemcpyHostToDevice, st->s);
    r += cnt;
  }
  if (err == hipSuccess) err = hipEventRecord(st->ev, st->s);
  if (err == hipSuccess) err = hipEventSynchronize(st->ev);   // the caller's arrays, the chunk and recs may go
  if (err != hipSuccess) {
    set_error(std::string(who) + ": " + hipGetErrorString(err));
    hipStreamSynchronize(st->s);
    undo();
    return DFH_ERR_HIP;
  }
  // commit
  for (size_t k = 0; k < new_caps.size(); ++k) {
    st->slab_ids.push_back(new_slabs[k]);
    st->slab_val.push_back(nullptr);
    st->slab_cap.push_back(new_caps[k]);
  }
  for (const auto& nv : new_vals) st->slab_val[nv.first] = nv.second;
  for (void* p : new_segs) st->seg_rows.push_back(p);
  for (float* p : new_wgts) st->seg_wgt.push_back(p);
  st->slab_used = used;
  st->nrows += nrows;
  st->nnz += (size_t)off[nrows] - first0;
  st->has_value = st->has_value || value != nullptr;
  st->has_weight = weight != nullptr;
  st->any_rows = true;
  st->data_bytes += fresh_bytes;
  st->ordered = false;
  return DFH_OK;
}

RsTables rs_tables(const dfh_rowstore* st) {
  const char* p = static_cast<const char*>(st->d_tables);
  RsTables t;
  t.slab_ids = reinterpret_cast<const uint64_t* const*>(p);
  t.slab_val = reinterpret_cast<const float* const*>(p + st->n_slabs * sizeof(void*));
  t.seg_rows = reinterpret_cast<const RsRow* const*>(p + 2 * st->n_slabs * sizeof(void*));
  t.seg_wgt = reinterpret_cast<const float* const*>(p + (2 * st->n_slabs + st->n_segs) * sizeof(void*));
  t.seg_shift = st->seg_shift;
  return t;
}

// the layout of a gathered block's row arrays inside one allocation, every array at a multiple of 16
struct RsBlock {
  size_t label, off, wgt, lens, flag, tmp, tmp_bytes, bytes;
  explicit RsBlock(size_t count) {
    size_t at = 0;
    auto take = [&at](size_t b) {
      const size_t was = at;
      at += (b + 15) & ~static_cast<size_t>(15);
      return was;
    };
    label = take(count * sizeof(float));
    off = take((count + 1) * sizeof(uint64_t));
    wgt = take(count * sizeof(float));
    lens = take((count + 1) * sizeof(uint64_t));
    flag = take(16);
    tmp_bytes = 0;
    (void)rocprim::exclusive_scan(nullptr, tmp_bytes, (uint64_t*)nullptr, (uint64_t*)nullptr, (uint64_t)0, count + 1, rocprim::plus<uint64_t>(),
                                  (hipStream_t) nullptr);
    tmp_bytes = std::max<size_t>(tmp_bytes, 256);
    tmp = take(tmp_bytes);
    bytes = at;
  }
};

// labels, weights and offsets of rows order[first .. first + count) into `rows` (laid out by `lay`), the block's nnz at h[0..1]
// and its "a value differs from 1.0f" flag at h[2] once the caller has waited for the stream
int rs_gather_rows(const dfh_rowstore* st, hipStream_t s, uint64_t first, size_t count, char* rows, const RsBlock& lay, uint32_t* h) {
  uint32_t* flag = reinterpret_cast<uint32_t*>(rows + lay.flag);
  uint64_t* off = reinterpret_cast<uint64_t*>(rows + lay.off);
  DFH_HIP(hipMemsetAsync(flag, 0, sizeof(uint32_t), s));
  hipLaunchKernelGGL(k_rs_rows, dim3(rs_grid(count + 1)), dim3(256), 0, s, st->d_order + first, (uint32_t)count, rs_tables(st),
                     reinterpret_cast<float*>(rows + lay.label), reinterpret_cast<uint64_t*>(rows + lay.lens),
                     st->has_weight ? reinterpret_cast<float*>(rows + lay.wgt) : nullptr, flag);
  DFH_HIP(hipGetLastError());
  size_t tb = lay.tmp_bytes;
  DFH_HIP(rocprim::exclusive_scan(rows + lay.tmp, tb, reinterpret_cast<uint64_t*>(rows + lay.lens), off, (uint64_t)0, count + 1,
                                  rocprim::plus<uint64_t>(), s));
  DFH_HIP(hipMemcpyAsync(h, off + count, sizeof(uint64_t), hipMemcpyDeviceToHost, s));
  DFH_HIP(hipMemcpyAsync(h + 2, flag, sizeof(uint32_t), hipMemcpyDeviceToHost, s));
  return DFH_OK;
}

int rs_gather_data(const dfh_rowstore* st, hipStream_t s, uint64_t first, size_t count, size_t nnz, const char* rows, const RsBlock& lay,
                   uint64_t* ids_out, float* val_out) {
  if (count == 0 || nnz == 0) return DFH_OK;
  hipLaunchKernelGGL(k_rs_copy, dim3(rs_grid(count * RS_GROUP)), dim3(256), 0, s, st->d_order + first, (uint32_t)count, rs_tables(st),
                     reinterpret_cast<const uint64_t*>(rows + lay.off), ids_out, val_out);
  DFH_HIP(hipGetLastError());
  return DFH_OK;
}

int rs_check_range(const dfh_rowstore* st, const char* who, uint64_t first, size_t count) {
  if (!st->ordered) {
    set_error(std::string(who) + ": the store has no order (call dfh_rowstore_order after the last append)");
    return DFH_ERR_STATE;
  }
  if (first > st->nrows || count > st->nrows - first || count >= (1ULL << 31)) {
    set_error(std::string(who) + ": rows [" + std::to_string(first) + ", " + std::to_string(first) + " + " + std::to_string(count) +
              ") of an order of " + std::to_string(st->nrows) + " rows (a block holds fewer than 2^31 rows)");
    return DFH_ERR_ARG;
  }
  return DFH_OK;
}
}  // namespace

extern "C" {

int dfh_rowstore_destroy(dfh_rowstore* st) {
  if (!st) return DFH_OK;
  hipSetDevice(st->ctx->device);
  if (st->ev) {
    hipEventRecord(st->ev, st->s);
    hipEventSynchronize(st->ev);
    hipEventDestroy(st->ev);
  }
  for (void* p : st->slab_ids) hipFree(p);
  for (void* p : st->slab_val)
    if (p) hipFree(p);
  for (void* p : st->seg_rows) hipFree(p);
  for (void* p : st->seg_wgt) hipFree(p);
  for (void* p : {st->d_tables, (void*)st->d_order, (void*)st->d_rd_rows, (void*)st->d_rd_data})
    if (p) hipFree(p);
  if (st->h_head) hipHostFree(st->h_head);
  delete st;
  return DFH_OK;
}

int dfh_rowstore_create(dfh_ctx* c, size_t slab_bytes, dfh_rowstore** out) {
  DFH_ARG(c && out, "dfh_rowstore_create: NULL argument");
  if (slab_bytes == 0) slab_bytes = RS_DEFAULT_SLAB;
  DFH_ARG(slab_bytes >= 1024 && slab_bytes <= (16ULL << 30), "dfh_rowstore_create: slab_bytes is 0 (the default, 64 MiB) or 1 KiB .. 16 GiB");
  DFH_HIP(hipSetDevice(c->device));
  {
    std::lock_guard<std::mutex> lk(c->parse_mu);
    if (!c->parse) DFH_HIP(hipStreamCreateWithFlags(&c->parse, hipStreamNonBlocking));
  }
  dfh_rowstore* st = new (std::nothrow) dfh_rowstore();
  if (!st) {
    set_error("dfh_rowstore_create: out of host memory");
    return DFH_ERR_HIP;
  }
  st->ctx = c;
  st->s = c->parse;
  st->slab_elems = slab_bytes / sizeof(uint64_t);
  while ((sizeof(RsRow) << (st->seg_shift + 1)) <= slab_bytes) ++st->seg_shift;
  hipError_t e;
  if ((e = hipEventCreateWithFlags(&st->ev, hipEventDisableTiming)) != hipSuccess ||
      (e = hipHostMalloc(reinterpret_cast<void**>(&st->h_head), 2 * sizeof(uint64_t), hipHostMallocDefault)) != hipSuccess) {
    set_error(std::string("dfh_rowstore_create: ") + hipGetErrorString(e));
    dfh_rowstore_destroy(st);
    return DFH_ERR_HIP;
  }
  *out = st;
  return DFH_OK;
}

int dfh_rowstore_append_host(dfh_rowstore* st, size_t nrows, const size_t* offset, const float* label, const uint64_t* index, const float* value,
                             const float* weight) {
  DFH_ARG(st && offset && (label || nrows == 0), "dfh_rowstore_append_host: NULL argument (offset and label are required)");
  DFH_ARG(index || offset[nrows] == offset[0], "dfh_rowstore_append_host: ids are required for a chunk that has nonzeros");
  return rs_append(st, "dfh_rowstore_append_host", nrows, offset, label, index, hipMemcpyHostToDevice, value, weight);
}

int dfh_rowstore_append_textchunk(dfh_rowstore* st, dfh_textchunk* tc) {
  DFH_ARG(st && tc, "dfh_rowstore_append_textchunk: NULL argument");
  DFH_ARG(tc->valid && tc->ctx == st->ctx, "dfh_rowstore_append_textchunk: no regular chunk parsed / a chunk of another context");
  // (the parse call has waited for its own work: the chunk's ids are complete, its offsets and labels are on the host)
  return rs_append(st, "dfh_rowstore_append_textchunk", tc->nrows, reinterpret_cast<const uint32_t*>(tc->h_rows),
                   reinterpret_cast<const float*>(tc->h_rows + tc->h_rows_cap * 4), tc->d_ids, hipMemcpyDeviceToDevice, nullptr, nullptr);
}

int dfh_rowstore_shape(dfh_rowstore* st, uint64_t* nrows, uint64_t* nnz, int* has_value, int* has_weight, uint64_t* device_bytes) {
  DFH_ARG(st, "dfh_rowstore_shape: NULL argument");
  std::lock_guard<std::mutex> lk(st->mu);
  if (nrows) *nrows = st->nrows;
  if (nnz) *nnz = st->nnz;
  if (has_value) *has_value = st->has_value ? 1 : 0;
  if (has_weight) *has_weight = st->has_weight ? 1 : 0;
  if (device_bytes) *device_bytes = st->data_bytes + st->order_bytes;
  return DFH_OK;
}

int dfh_rowstore_order(dfh_rowstore* st, int shuffle, uint64_t seed) {
  DFH_ARG(st && (shuffle == 0 || shuffle == 1), "dfh_rowstore_order: NULL argument / shuffle is 0 or 1");
  std::lock_guard<std::mutex> lk(st->mu);
  DFH_HIP(hipSetDevice(st->ctx->device));
  st->ordered = false;
  const size_t n = (size_t)st->nrows;
  // the pointer tables the kernels walk (small: one word per slab and segment)
  const size_t ns = st->slab_ids.size(), ng = st->seg_rows.size();
  std::vector<void*> tab;
  tab.insert(tab.end(), st->slab_ids.begin(), st->slab_ids.end());
  tab.insert(tab.end(), st->slab_val.begin(), st->slab_val.end());
  tab.insert(tab.end(), st->seg_rows.begin(), st->seg_rows.end());
  tab.insert(tab.end(), st->seg_wgt.begin(), st->seg_wgt.end());
  tab.resize(2 * ns + 2 * ng, nullptr);
  if (st->d_tables) DFH_HIP(hipFree(st->d_tables));
  st->d_tables = nullptr;
  const size_t tab_bytes = std::max<size_t>(tab.size(), 1) * sizeof(void*);
  int rc = rs_alloc(st, &st->d_tables, tab_bytes, "the tables of slabs and segments");
  if (rc) return rc;
  if (!tab.empty()) DFH_HIP(hipMemcpyAsync(st->d_tables, tab.data(), tab.size() * sizeof(void*), hipMemcpyHostToDevice, st->s));
  st->n_slabs = ns;
  st->n_segs = ng;
  if (st->cap_order < n || !st->d_order) {
    if (st->d_order) DFH_HIP(hipFree(st->d_order));
    st->d_order = nullptr;
    st->cap_order = 0;
    void* p = nullptr;
    rc = rs_alloc(st, &p, std::max<size_t>(n, 1) * sizeof(uint32_t), "the order");
    if (rc) return rc;
    st->d_order = static_cast<uint32_t*>(p);
    st->cap_order = std::max<size_t>(n, 1);
  }
  st->order_bytes = tab_bytes + st->cap_order * sizeof(uint32_t);
  void* tmp = nullptr;
  if (n && !shuffle) {
    hipLaunchKernelGGL(k_rs_iota, dim3(rs_grid(n)), dim3(256), 0, st->s, st->d_order, (uint32_t)n);
    DFH_HIP(hipGetLastError());
  } else if (n) {
    size_t tb = 0;
    DFH_HIP(rocprim::radix_sort_pairs(nullptr, tb, (uint64_t*)nullptr, (uint64_t*)nullptr, (uint32_t*)nullptr, (uint32_t*)nullptr, n, 0, 64, st->s));
    tb = std::max<size_t>(tb, 256);
    const size_t keys_b = (n * sizeof(uint64_t) + 255) & ~static_cast<size_t>(255), rows_b = (n * sizeof(uint32_t) + 255) & ~static_cast<size_t>(255);
    rc = rs_alloc(st, &tmp, 2 * keys_b + rows_b + tb, "the sort of the order's keys");
    if (rc) return rc;
    char* w = static_cast<char*>(tmp);
    uint64_t *k0 = reinterpret_cast<uint64_t*>(w), *k1 = reinterpret_cast<uint64_t*>(w + keys_b);
    uint32_t* r0 = reinterpret_cast<uint32_t*>(w + 2 * keys_b);
    hipLaunchKernelGGL(k_rs_keys, dim3(rs_grid(n)), dim3(256), 0, st->s, k0, r0, (uint32_t)n, seed);
    hipError_t e = hipGetLastError();
    if (e == hipSuccess) e = rocprim::radix_sort_pairs(w + 2 * keys_b + rows_b, tb, k0, k1, r0, st->d_order, n, 0, 64, st->s);
    if (e != hipSuccess) {
      set_error(std::string("dfh_rowstore_order: ") + hipGetErrorString(e));
      hipStreamSynchronize(st->s);
      hipFree(tmp);
      return DFH_ERR_HIP;
    }
  }
  rc = rs_wait(st);
  if (tmp) hipFree(tmp);
  if (rc) return rc;
  st->ordered = true;
  return DFH_OK;
}

int dfh_rowstore_get_order(dfh_rowstore* st, uint32_t* order) {
  DFH_ARG(st && (order || st->nrows == 0), "dfh_rowstore_get_order: NULL argument");
  std::lock_guard<std::mutex> lk(st->mu);
  if (!st->ordered) {
    set_error("dfh_rowstore_get_order: the store has no order (call dfh_rowstore_order after the last append)");
    return DFH_ERR_STATE;
  }
  DFH_HIP(hipSetDevice(st->ctx->device));
  if (st->nrows) DFH_HIP(hipMemcpy(order, st->d_order, (size_t)st->nrows * sizeof(uint32_t), hipMemcpyDeviceToHost));
  return DFH_OK;
}

int dfh_rowstore_read(dfh_rowstore* st, uint64_t first, size_t count, size_t* offset, float* label, uint64_t* index, float* value, float* weight,
                      size_t* nnz_out) {
  DFH_ARG(st && offset && (label || count == 0), "dfh_rowstore_read: NULL argument (offset and label are required)");
  std::lock_guard<std::mutex> lk(st->mu);
  int rc = rs_check_range(st, "dfh_rowstore_read", first, count);
  if (rc) return rc;
  DFH_ARG(!weight || st->has_weight, "dfh_rowstore_read: weights asked of a store that carries none");
  DFH_HIP(hipSetDevice(st->ctx->device));
  const RsBlock lay(count);
  rc = tp_reserve(&st->d_rd_rows, &st->cap_rd_rows, lay.bytes);
  if (rc) return rc;
  uint32_t* h = reinterpret_cast<uint32_t*>(st->h_head);
  rc = rs_gather_rows(st, st->s, first, count, st->d_rd_rows, lay, h);
  if (!rc) rc = rs_wait(st);
  if (rc) return rc;
  const size_t nnz = (size_t)st->h_head[0];
  if (nnz_out) *nnz_out = nnz;
  static_assert(sizeof(size_t) == sizeof(uint64_t), "offsets are read back as 64-bit words");
  DFH_HIP(hipMemcpyAsync(offset, st->d_rd_rows + lay.off, (count + 1) * sizeof(uint64_t), hipMemcpyDeviceToHost, st->s));
  if (count) DFH_HIP(hipMemcpyAsync(label, st->d_rd_rows + lay.label, count * sizeof(float), hipMemcpyDeviceToHost, st->s));
  if (count && weight) DFH_HIP(hipMemcpyAsync(weight, st->d_rd_rows + lay.wgt, count * sizeof(float), hipMemcpyDeviceToHost, st->s));
  if (index && nnz) {
    const bool vals = value && st->has_value;
    const size_t ids_b = (nnz * sizeof(uint64_t) + 15) & ~static_cast<size_t>(15);
    rc = tp_reserve(&st->d_rd_data, &st->cap_rd_data, ids_b + (vals ? nnz * sizeof(float) : 0));
    if (rc) return rc;
    rc = rs_gather_data(st, st->s, first, count, nnz, st->d_rd_rows, lay, reinterpret_cast<uint64_t*>(st->d_rd_data),
                        vals ? reinterpret_cast<float*>(st->d_rd_data + ids_b) : nullptr);
    if (rc) return rc;
    DFH_HIP(hipMemcpyAsync(index, st->d_rd_data, nnz * sizeof(uint64_t), hipMemcpyDeviceToHost, st->s));
    if (vals) DFH_HIP(hipMemcpyAsync(value, st->d_rd_data + ids_b, nnz * sizeof(float), hipMemcpyDeviceToHost, st->s));
  }
  rc = rs_wait(st);
  if (rc) return rc;
  if (index && value && !st->has_value) std::fill(value, value + nnz, 1.0f);
  return DFH_OK;
}

int dfh_crb_encode_rowstore(dfh_crb* e, dfh_rowstore* st, uint64_t first, size_t count, size_t* record_bytes) {
  DFH_ARG(e && st && record_bytes, "dfh_crb_encode_rowstore: NULL argument");
  DFH_ARG(e->ctx == st->ctx, "dfh_crb_encode_rowstore: a store of another context");
  e->valid = false;
  int rc = rs_check_range(st, "dfh_crb_encode_rowstore", first, count);
  if (rc) return rc;
  DFH_HIP(hipSetDevice(e->ctx->device));
  const RsBlock lay(count);
  rc = tp_reserve(&e->d_gather, &e->cap_gather, lay.bytes);
  if (rc) return rc;
  rc = rs_gather_rows(st, e->s, first, count, e->d_gather, lay, e->h_head);
  if (!rc) rc = lz_wait(e);
  if (rc) return rc;
  uint64_t nnz64 = 0;
  memcpy(&nnz64, e->h_head, sizeof(nnz64));
  const size_t nnz = (size_t)nnz64;
  const bool vals = st->has_value && e->h_head[2] != 0u;   // all ones: the field is dropped, as dfh_crb_encode_host does
  const size_t bytes[5] = {count * sizeof(float), (count + 1) * sizeof(uint64_t), nnz * sizeof(uint64_t), vals ? nnz * sizeof(float) : 0,
                           st->has_weight ? count * sizeof(float) : 0};
  rc = lz_reserve(e, bytes, 5, lz_align16(bytes[2]) + lz_align16(bytes[3]));
  if (rc) return rc;
  uint64_t* ids = reinterpret_cast<uint64_t*>(e->d_in);
  float* val = vals ? reinterpret_cast<float*>(e->d_in + lz_align16(bytes[2])) : nullptr;
  rc = rs_gather_data(st, e->s, first, count, nnz, e->d_gather, lay, ids, val);
  if (rc) return rc;
  const char* dev[5] = {e->d_gather + lay.label, e->d_gather + lay.off, reinterpret_cast<const char*>(ids), reinterpret_cast<const char*>(val),
                        st->has_weight ? e->d_gather + lay.wgt : nullptr};
  rc = crb_encode_device(e, count, dev, bytes);
  if (rc) return rc;
  *record_bytes = e->record_bytes;
  return DFH_OK;
}

}  // extern "C"
