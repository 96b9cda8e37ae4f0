// dfh_dumptext.hip — a model table as sorted text on the device (included at the end of dfh_api.hip; task = dump of the command
// line): one line "<id>\t<w>[\t<V_0> .. \t<V_{k-1}>]\n" per kept entry (w != 0 || has_V, dfh_table_save's rule without aux), in
// ascending order of the printed id, every float as fprintf("%.9g") writes it.  The arithmetic is dfh_predtext_fmt.h (the
// floats, used as it is) and dfh_dumptext_fmt.h (the id's digits, a field, where things go in a line); a value pt_format does
// not format is counted, and the caller formats such a unit on the host from dfh_dump_entries.
// dfh_dump_open queues
//   k_dump_select   a lane per slot of the key index: {printed id, row | kHasV} of the kept entries, appended through one atomic
//                   per wave (any order: the sort follows), and the two counts
//   rocprim::radix_sort_pairs by the id: keys are unique, so the sorted list — and with it every byte of the text — is a
//                   function of the model alone, whatever slots, capacity or import order it has.  12 B per entry stay (twice
//                   that and rocprim's workspace while the sort runs); rows are read IN PLACE afterwards, the exported table
//                   never exists.
// dfh_dump_format(first, count) is the two passes of dfh_textout.hip with k_dumptext, the entries' lengths carried between them:
// a tile is T entries (T by V_dim, so that a tile's longest text fits the LDS image); an entry is P = min(64, pow2 >= 1 + V_dim)
// lanes, a lane per value and round, 64 / P entries per wave and round, R = ceil((1 + V_dim) / P) rounds per entry; the fields'
// lengths are summed by a scan inside the P lanes, the id's digits are made once per entry, by the entry's first lane.
// These kernels are not in the timing registry (dfh_kernel_name) and no other launch changes.
#include "dfh_dumptext_fmt.h"

struct dfh_dump {
  dfh_ctx* ctx = nullptr;
  dfh_table* t = nullptr;
  uint64_t n = 0, n_with_V = 0;   // kept entries, those of them with V
  uint64_t* d_id = nullptr;       // [n] the printed ids, ascending
  uint32_t* d_row = nullptr;      // [n] row | kHasV
  uint32_t k = 0, tile = 0, lp = 0;   // V_dim, entries per tile (0: a line does not fit the image), log2 of the lanes per entry
  TextWork text;                  // format's workspace (dfh_textout.hip); dfh_dump_pairs' scan borrows its d_tmp
  uint32_t* d_cnt = nullptr;      // [2] {kept, with V} of the select
  char* d_ent = nullptr;          // dfh_dump_entries' arrays
  size_t ent_cap = 0;
  bool formatted = false;
  // dfh_dump_pairs' (dfh_pairs.hip): built by its first call, kept
  struct Pairs {
    bool built = false;
    uint32_t kd = 0;              // floats per packed row
    uint64_t rows = 0;            // packed rows, the padding included
    float* P = nullptr;           // [rows][kd] the has-V entries' V, in position order
    uint32_t* epos = nullptr;     // [n + 1] entry -> position (the entries with V before it)
    uint32_t* map = nullptr;      // [n_with_V] position -> entry
    unsigned long long* part = nullptr;   // the splits' partial lists of the last call
    size_t part_cap = 0;
    char* out = nullptr;          // a call's lists before their download
    size_t out_cap = 0;
    unsigned long long* d_nf = nullptr;
  } pr;
};

namespace {
void pairs_release(dfh_dump* p);   // dfh_pairs.hip

// a lane per slot (the index has a multiple of 64 slots: a wave's lanes are in the loop together)
__global__ void __launch_bounds__(256) k_dump_select(TableView t, uint64_t nslots, int feature_ids, uint64_t cap, uint64_t* __restrict__ ids,
                                                     uint32_t* __restrict__ rows, uint32_t* __restrict__ counts) {
  const uint32_t lane = threadIdx.x & 63u;
  for (uint64_t s0 = (uint64_t)blockIdx.x * 256 + (threadIdx.x & ~63u); s0 < nslots; s0 += (uint64_t)gridDim.x * 256) {
    const uint64_t s = s0 + lane;
    bool keep = false, hv = false;
    uint64_t key = kEmptyKey;
    uint32_t r = 0;
    if (s < nslots) {
      key = t.ht[s].key;
      r = t.ht[s].row;
      if (key != kEmptyKey && r < t.capacity) {
        const uint2 wh = *reinterpret_cast<const uint2*>(&t.hdr[r]);   // {w, has_V}
        hv = wh.y != 0u;
        keep = __uint_as_float(wh.x) != 0.f || hv;
      }
    }
    const unsigned long long m = __ballot(keep), mv = __ballot(keep && hv);
    if (m == 0ull) continue;
    uint32_t at = 0;
    if (lane == 0) {
      at = atomicAdd(&counts[0], (uint32_t)__popcll(m));
      if (mv) atomicAdd(&counts[1], (uint32_t)__popcll(mv));
    }
    at = (uint32_t)__shfl((int)at, 0, 64) + (uint32_t)__popcll(m & ((1ull << lane) - 1ull));
    if (keep && at < cap) {
      ids[at] = feature_ids ? reverse_bytes(key) : key;
      rows[at] = r | (hv ? kHasV : 0u);
    }
  }
}

// EMIT = 0: elen[e], tile_bytes[t] (and tile_bytes[ntiles] = 0), *irregular.  EMIT = 1: elen and tile_scan in, text out.
// ids / rows / elen point at the unit's first entry.
template <int EMIT>
__global__ void __launch_bounds__(256) k_dumptext(const RowHdr* __restrict__ hdr, const float* __restrict__ va, uint32_t k, uint32_t kp,
                                                  const uint64_t* __restrict__ ids, const uint32_t* __restrict__ rows, uint64_t count,
                                                  uint32_t T, uint32_t lp, uint32_t* __restrict__ elen, uint64_t* __restrict__ tile_bytes,
                                                  const uint64_t* __restrict__ tile_scan, unsigned char* __restrict__ out,
                                                  uint32_t* __restrict__ irregular) {
  __shared__ uint32_t s_acc[2];                          // EMIT = 0: the tile's bytes, its irregular values
  __shared__ typename TextScan::storage_type s_scan;     // EMIT = 1
  __shared__ uint32_t s_off[EMIT ? TO_TILE_MAX : 1];     // EMIT = 1: where each entry's line starts in the tile's text
  __shared__ __attribute__((aligned(16))) unsigned char img[EMIT ? TO_IMG + 16 : 16];
  const uint32_t P = 1u << lp, G = 64u >> lp;         // lanes per entry; entries per wave and round
  const uint32_t lane = threadIdx.x & 63u, wave = threadIdx.x >> 6, g = lane & (P - 1u), lead = lane & ~(P - 1u);
  const uint64_t base = (uint64_t)blockIdx.x * T;
  const uint32_t tn = (uint32_t)(count - base < (uint64_t)T ? count - base : (uint64_t)T);   // entries of this tile: 1 .. T
  const uint32_t R = (k + P) >> lp;                   // rounds of an entry: ceil((1 + k) / P)
  TextTile tt = {};
  if (!EMIT)
    to_measure_begin(s_acc);
  else
    tt = to_tile_begin(elen, base, tn, tile_scan, s_off, s_scan);
  uint32_t irr = 0;
  for (uint32_t e0 = wave * G; e0 < tn; e0 += 4 * G) {   // the same trips for every lane of a wave
    const uint32_t le = e0 + (lane >> lp);
    const bool valid = le < tn;
    const uint32_t rw = valid ? rows[base + le] : 0u, r = rw & kRowMask;
    const uint32_t nv = valid ? 1u + ((rw & kHasV) ? k : 0u) : 0u;
    dfh_dt::Id d;
    d.c0 = 0;
    d.c1 = d.c2 = 0;
    d.nd = 0;
    if (valid && g == 0) d = dfh_dt::dt_id(ids[base + le]);   // the digits once per entry
    uint32_t at = (uint32_t)__shfl((int)d.nd, (int)lead, 64);  // bytes of the line so far
    unsigned char* const line = img + (EMIT ? tt.run0 + s_off[valid ? le : 0] : 0u);   // at most 15 + T * dt_max_line(k) <= 15 + TO_IMG behind img
    for (uint32_t rd = 0; rd < R; ++rd) {
      const uint32_t j = (rd << lp) + g;
      dfh_dt::Field F;
      F.lo = F.hi = 0;
      F.len = 0;
      if (j < nv) {
        const uint32_t bits = j == 0 ? __float_as_uint(hdr[r].w) : __float_as_uint(va[(size_t)r * (2 * kp) + (j - 1)]);
        F = dfh_dt::dt_field(bits);
        irr += F.len == 0 ? 1u : 0u;
      }
      uint32_t total;
      const uint32_t x = to_group_scan(F.len, P, g, lead, &total);
      if (EMIT && F.len) dfh_dt::dt_put_field(line + at + (x - F.len), F);
      at += total;
    }
    if (valid && g == 0) {
      if (!EMIT) {
        elen[base + le] = at + 1;
        atomicAdd(&s_acc[0], at + 1);
      } else {
        dfh_dt::dt_put_id(line, d);
        line[at] = '\n';
      }
    }
  }
  if (!EMIT) {
    to_measure_end(s_acc, irr, tile_bytes, irregular);
    return;
  }
  __syncthreads();   // the image is complete
  to_store(out, img, tt.g_first, tt.g_end, tt.g_img);
}

// the unit's entries as arrays: a thread per (entry, V column)
__global__ void __launch_bounds__(256) k_dump_entries(const RowHdr* __restrict__ hdr, const float* __restrict__ va, uint32_t k, uint32_t kp,
                                                      const uint64_t* __restrict__ ids, const uint32_t* __restrict__ rows, uint64_t count,
                                                      uint64_t* __restrict__ o_id, float* __restrict__ o_w, int* __restrict__ o_has,
                                                      float* __restrict__ o_V) {
  const uint64_t kk = k ? k : 1u, total = count * kk;
  for (uint64_t i = (uint64_t)blockIdx.x * 256 + threadIdx.x; i < total; i += (uint64_t)gridDim.x * 256) {
    const uint64_t e = i / kk;
    const uint32_t j = (uint32_t)(i - e * kk), rw = rows[e], r = rw & kRowMask;
    if (j == 0) {
      o_id[e] = ids[e];
      o_w[e] = hdr[r].w;
      o_has[e] = (rw & kHasV) ? 1 : 0;
    }
    if (k) o_V[e * k + j] = (rw & kHasV) ? va[(size_t)r * (2 * kp) + j] : 0.f;
  }
}
}  // namespace

extern "C" {

int dfh_dump_close(dfh_dump* p) {
  if (!p) return DFH_OK;
  (void)hipSetDevice(p->ctx->device);
  (void)hipStreamSynchronize(p->ctx->stream);
  if (p->d_id) (void)hipFree(p->d_id);
  if (p->d_row) (void)hipFree(p->d_row);
  to_release(&p->text);
  if (p->d_cnt) (void)hipFree(p->d_cnt);
  if (p->d_ent) (void)hipFree(p->d_ent);
  pairs_release(p);
  delete p;
  return DFH_OK;
}

int dfh_dump_open(dfh_table* t, int ids_mode, dfh_dump** out, uint64_t* n_entries) {
  DFH_ARG(t && out && n_entries, "dfh_dump_open: NULL argument");
  DFH_ARG(ids_mode == DFH_DUMP_IDS_FEATURE || ids_mode == DFH_DUMP_IDS_KEY,
          "dfh_dump_open: ids_mode must be DFH_DUMP_IDS_FEATURE or DFH_DUMP_IDS_KEY");
  *out = nullptr;
  *n_entries = 0;
  dfh_ctx* c = t->ctx;
  DFH_HIP(hipSetDevice(c->device));
  uint64_t cnt = 0;
  int rc = dfh_table_size(t, &cnt);   // drains the context's streams: nothing is still inserting
  if (rc) return rc;
  dfh_dump* p = new (std::nothrow) dfh_dump();
  if (!p) {
    set_error("dfh_dump_open: out of host memory (" + std::to_string(sizeof(dfh_dump)) + " bytes needed)");
    return DFH_ERR_CAPACITY;
  }
  p->ctx = c;
  p->t = t;
  p->k = (uint32_t)t->v.k;
  const uint64_t max_line = dfh_dt::dt_max_line(p->k);
  p->tile = (uint32_t)std::min<uint64_t>(TO_TILE_MAX, TO_IMG / max_line);
  while ((1u << p->lp) < 64u && (1u << p->lp) < 1u + p->k) ++p->lp;
  hipStream_t s = c->stream;
  uint64_t* id0 = nullptr;
  uint32_t* row0 = nullptr;
  void* tmp = nullptr;
  auto fail = [&](int code, const std::string& msg) {
    if (id0) (void)hipFree(id0);
    if (row0) (void)hipFree(row0);
    if (tmp) (void)hipFree(tmp);
    (void)hipGetLastError();
    set_error(msg);
    dfh_dump_close(p);
    return code;
  };
  hipError_t e = hipMalloc(reinterpret_cast<void**>(&p->d_cnt), 2 * sizeof(uint32_t));
  if (e == hipSuccess) e = hipMemsetAsync(p->d_cnt, 0, 2 * sizeof(uint32_t), s);
  if (e != hipSuccess) return fail(DFH_ERR_HIP, std::string("dfh_dump_open: ") + hipGetErrorString(e));
  if (cnt) {
    size_t tb = 0;
    e = rocprim::radix_sort_pairs(nullptr, tb, (uint64_t*)nullptr, (uint64_t*)nullptr, (uint32_t*)nullptr, (uint32_t*)nullptr, (size_t)cnt, 0, 64, s);
    if (e != hipSuccess) return fail(DFH_ERR_HIP, std::string("dfh_dump_open: ") + hipGetErrorString(e));
    tb = std::max<size_t>(tb, 256);
    const size_t need = 2 * cnt * (sizeof(uint64_t) + sizeof(uint32_t)) + tb;
    if (hipMalloc(reinterpret_cast<void**>(&id0), cnt * sizeof(uint64_t)) != hipSuccess ||
        hipMalloc(reinterpret_cast<void**>(&row0), cnt * sizeof(uint32_t)) != hipSuccess ||
        hipMalloc(reinterpret_cast<void**>(&p->d_id), cnt * sizeof(uint64_t)) != hipSuccess ||
        hipMalloc(reinterpret_cast<void**>(&p->d_row), cnt * sizeof(uint32_t)) != hipSuccess || hipMalloc(&tmp, tb) != hipSuccess)
      return fail(DFH_ERR_CAPACITY, "dfh_dump_open: no device memory for the ids and rows of " + std::to_string(cnt) + " entries and their sort (" +
                                        std::to_string(need) + " bytes needed)");
    hipLaunchKernelGGL(k_dump_select, dim3(grid_for_threads(t->hslots, c)), dim3(256), 0, s, t->v, t->hslots,
                       ids_mode == DFH_DUMP_IDS_FEATURE ? 1 : 0, cnt, id0, row0, p->d_cnt);
    e = hipGetLastError();
    uint32_t h_cnt[2] = {0, 0};
    if (e == hipSuccess) e = hipMemcpyAsync(h_cnt, p->d_cnt, sizeof(h_cnt), hipMemcpyDeviceToHost, s);
    if (e == hipSuccess) e = hipStreamSynchronize(s);
    if (e != hipSuccess) return fail(DFH_ERR_HIP, std::string("dfh_dump_open: ") + hipGetErrorString(e));
    p->n = std::min<uint64_t>(h_cnt[0], cnt);
    p->n_with_V = h_cnt[1];
    if (p->n) {
      e = rocprim::radix_sort_pairs(tmp, tb, id0, p->d_id, row0, p->d_row, (size_t)p->n, 0, 64, s);
      if (e == hipSuccess) e = hipStreamSynchronize(s);
      if (e != hipSuccess) return fail(DFH_ERR_HIP, std::string("dfh_dump_open: ") + hipGetErrorString(e));
    }
    (void)hipFree(id0);
    (void)hipFree(row0);
    (void)hipFree(tmp);
  }
  *out = p;
  *n_entries = p->n;
  return DFH_OK;
}

int dfh_dump_shape(dfh_dump* p, uint64_t* n_entries, uint64_t* n_with_V, int* V_dim) {
  DFH_ARG(p, "dfh_dump_shape: NULL argument");
  if (n_entries) *n_entries = p->n;
  if (n_with_V) *n_with_V = p->n_with_V;
  if (V_dim) *V_dim = (int)p->k;
  return DFH_OK;
}

int dfh_dump_tile(dfh_dump* p) { return p ? (int)p->tile : 0; }

int dfh_dump_format(dfh_dump* p, uint64_t first, size_t count, size_t* nbytes, uint64_t* irregular) {
  DFH_ARG(p && nbytes && irregular, "dfh_dump_format: NULL argument");
  *nbytes = 0;
  *irregular = 0;
  DFH_ARG(first <= p->n && count <= p->n - first, "dfh_dump_format: first + count exceeds the dump's entries");
  DFH_ARG(p->tile > 0, "dfh_dump_format: a line of this V_dim does not fit the formatter's LDS image (V_dim above 2045); format the "
                       "entries of dfh_dump_entries on the host");
  hipStream_t s = p->ctx->stream;
  DFH_HIP(hipSetDevice(p->ctx->device));
  p->formatted = false;
  const TableView& v = p->t->v;
  const uint64_t* ids = p->d_id + first;
  const uint32_t* rows = p->d_row + first;
  const int rc = to_format(p->ctx, &p->text, count, p->tile, (size_t)dfh_dt::dt_max_line(p->k), true, nullptr, "dfh_dump_format",
                           [&](int emit, unsigned ntiles, const TextPass& a) {
                             hipLaunchKernelGGL(emit ? k_dumptext<1> : k_dumptext<0>, dim3(ntiles), dim3(256), 0, s, (const RowHdr*)v.hdr,
                                                (const float*)v.va, p->k, (uint32_t)v.kp, ids, rows, (uint64_t)count, p->tile, p->lp, a.rlen,
                                                a.tile_bytes, a.tile_scan, a.out, a.irregular);
                           },
                           nbytes, irregular);
  if (rc) return rc;
  p->formatted = true;
  return DFH_OK;
}

int dfh_dump_read(dfh_dump* p, char* dst) {
  DFH_ARG(p && (dst || p->text.text_bytes == 0), "dfh_dump_read: NULL argument");
  if (!p->formatted) {
    set_error("dfh_dump_read: nothing formatted (call dfh_dump_format first)");
    return DFH_ERR_STATE;
  }
  return to_read(p->ctx, &p->text, dst);
}

int dfh_dump_entries(dfh_dump* p, uint64_t first, size_t count, uint64_t* ids, float* w, int* has_V, float* V) {
  DFH_ARG(p, "dfh_dump_entries: NULL argument");
  DFH_ARG(first <= p->n && count <= p->n - first, "dfh_dump_entries: first + count exceeds the dump's entries");
  if (count == 0) return DFH_OK;
  DFH_ARG(ids && w && has_V && (V || p->k == 0), "dfh_dump_entries: NULL argument");
  hipStream_t s = p->ctx->stream;
  DFH_HIP(hipSetDevice(p->ctx->device));
  const size_t k = p->k, per = sizeof(uint64_t) + sizeof(float) + sizeof(int) + k * sizeof(float);
  int rc = dev_grow(&p->d_ent, &p->ent_cap, count * per + 256, "dfh_dump_entries", "the entries");
  if (rc) return rc;
  uint64_t* o_id = reinterpret_cast<uint64_t*>(p->d_ent);   // 8 B, then the 4 B arrays: each aligned to its type
  float* o_w = reinterpret_cast<float*>(o_id + count);
  int* o_has = reinterpret_cast<int*>(o_w + count);
  float* o_V = reinterpret_cast<float*>(o_has + count);
  const TableView& v = p->t->v;
  hipLaunchKernelGGL(k_dump_entries, dim3(grid_for_threads(count * std::max<size_t>(k, 1), p->ctx)), dim3(256), 0, s, (const RowHdr*)v.hdr,
                     (const float*)v.va, p->k, (uint32_t)v.kp, (const uint64_t*)(p->d_id + first), (const uint32_t*)(p->d_row + first),
                     (uint64_t)count, o_id, o_w, o_has, o_V);
  DFH_HIP(hipGetLastError());
  DFH_HIP(hipMemcpyAsync(ids, o_id, count * sizeof(uint64_t), hipMemcpyDeviceToHost, s));
  DFH_HIP(hipMemcpyAsync(w, o_w, count * sizeof(float), hipMemcpyDeviceToHost, s));
  DFH_HIP(hipMemcpyAsync(has_V, o_has, count * sizeof(int), hipMemcpyDeviceToHost, s));
  if (k) DFH_HIP(hipMemcpyAsync(V, o_V, count * k * sizeof(float), hipMemcpyDeviceToHost, s));
  DFH_HIP(hipStreamSynchronize(s));
  return DFH_OK;
}

int dfh_dump_ids(dfh_dump* p, uint64_t first, size_t count, uint64_t* ids, int* has_V) {
  DFH_ARG(p, "dfh_dump_ids: NULL argument");
  DFH_ARG(first <= p->n && count <= p->n - first, "dfh_dump_ids: first + count exceeds the dump's entries");
  if (count == 0) return DFH_OK;
  DFH_ARG(ids && has_V, "dfh_dump_ids: NULL argument");
  hipStream_t s = p->ctx->stream;
  DFH_HIP(hipSetDevice(p->ctx->device));
  static_assert(sizeof(int) == sizeof(uint32_t), "the row words land in has_V");
  DFH_HIP(hipMemcpyAsync(ids, p->d_id + first, count * sizeof(uint64_t), hipMemcpyDeviceToHost, s));
  DFH_HIP(hipMemcpyAsync(has_V, p->d_row + first, count * sizeof(uint32_t), hipMemcpyDeviceToHost, s));
  DFH_HIP(hipStreamSynchronize(s));
  for (size_t i = 0; i < count; ++i) has_V[i] = ((uint32_t)has_V[i] & kHasV) ? 1 : 0;
  return DFH_OK;
}

}  // extern "C"
