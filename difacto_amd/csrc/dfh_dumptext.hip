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
// dfh_dump_format(first, count) queues, in the shape of k_predtext:
//   k_dumptext<0>   a block per tile of T entries (T by V_dim, so that a tile's longest text fits the LDS image).  An entry is
//                   P = min(64, pow2 >= 1 + V_dim) lanes, a lane per value and round, 64 / P entries per wave and round; the
//                   fields' lengths are summed by a scan inside the P lanes.  Out: each entry's length (4 B), the tile's
//                   bytes, the irregular values (an atomic per block that has any)
//   rocprim::exclusive_scan over the tiles' bytes
//   k_dumptext<1>   a block per tile again: the entries' lengths scanned in the block place the lines in LDS, the values are
//                   formatted ONCE MORE into their places (the id's digits once per entry, by the entry's first lane), the image
//                   is shifted by the tile's first byte mod 16 and written with aligned 16 B stores; only the tile's unaligned
//                   head and tail go byte by byte
// and reads back {bytes, irregular}: one host round trip.  The launches are ordered by the stream alone: no block waits for
// another.  Plain C++, no scratch.  These kernels are not in the timing registry (dfh_kernel_name) and no other launch changes.
#include "dfh_dumptext_fmt.h"

struct dfh_dump {
  dfh_ctx* ctx = nullptr;
  dfh_table* t = nullptr;
  uint64_t n = 0, n_with_V = 0;   // kept entries, those of them with V
  uint64_t* d_id = nullptr;       // [n] the printed ids, ascending
  uint32_t* d_row = nullptr;      // [n] row | kHasV
  uint32_t k = 0, tile = 0, lp = 0;   // V_dim, entries per tile (0: a line does not fit the image), log2 of the lanes per entry
  // format's workspace, grown to what a format needs, kept
  char* d_text = nullptr;
  size_t text_cap = 0, text_bytes = 0;
  uint32_t* d_elen = nullptr;     // [elen_cap] bytes per entry of the unit
  size_t elen_cap = 0;
  uint64_t *d_tile = nullptr, *d_tile_scan = nullptr;   // bytes per tile (and a 0), their exclusive scan (the last: all bytes)
  size_t tile_cap = 0, scan_cap = 0;
  void* d_tmp = nullptr;          // rocprim's
  size_t tmp_bytes = 0;
  uint32_t* d_cnt = nullptr;      // [4] {kept, with V} of the select, [2] the irregular values of the last format
  uint64_t* h_head = nullptr;     // page-locked {bytes, irregular}
  char* h_text = nullptr;         // page-locked: read's download lands here
  size_t h_text_cap = 0;
  char* d_ent = nullptr;          // dfh_dump_entries' arrays
  size_t ent_cap = 0;
  bool formatted = false;
};

namespace {
constexpr uint32_t DT_IMG = 32768, DT_TILE_MAX = 1024;   // the LDS image of a tile's text (and 16 B for its shift); entries per tile at most

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
  using Scan = rocprim::block_scan<uint32_t, 256>;
  __shared__ uint32_t s_acc[2];                       // EMIT = 0: the tile's bytes, its irregular values
  __shared__ typename Scan::storage_type s_scan;      // EMIT = 1
  __shared__ uint32_t s_off[EMIT ? DT_TILE_MAX : 1];  // EMIT = 1: where each entry's line starts in the tile's text
  __shared__ __attribute__((aligned(16))) unsigned char img[EMIT ? DT_IMG + 16 : 16];
  const uint32_t P = 1u << lp, G = 64u >> lp;         // lanes per entry; entries per wave and round
  const uint32_t lane = threadIdx.x & 63u, wave = threadIdx.x >> 6, g = lane & (P - 1u), lead = lane & ~(P - 1u);
  const uint64_t base = (uint64_t)blockIdx.x * T;
  const uint32_t tn = (uint32_t)(count - base < (uint64_t)T ? count - base : (uint64_t)T);   // entries of this tile: 1 .. T
  const uint32_t R = (k + P) >> lp;                   // rounds of an entry: ceil((1 + k) / P)
  uint64_t g_first = 0, g_end = 0, g_img = 0;
  uint32_t run0 = 0;
  if (!EMIT) {
    if (threadIdx.x < 2) s_acc[threadIdx.x] = 0;
    __syncthreads();
  } else {
    uint32_t len4[4], off4[4];
#pragma unroll
    for (uint32_t i = 0; i < 4; ++i) {
      const uint32_t e = 4 * threadIdx.x + i;
      len4[i] = e < tn ? elen[base + e] : 0u;
    }
    Scan().exclusive_scan(len4, off4, 0u, s_scan);
#pragma unroll
    for (uint32_t i = 0; i < 4; ++i) s_off[4 * threadIdx.x + i] = off4[i];   // 4 * 256 = DT_TILE_MAX
    g_first = tile_scan[blockIdx.x];
    g_end = tile_scan[blockIdx.x + 1];
    g_img = g_first & ~15ULL;   // the text position of img[0]: a 16 B word of the text is a 16 B word of the image
    run0 = (uint32_t)(g_first - g_img);
    __syncthreads();
  }
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
    unsigned char* const line = img + (EMIT ? run0 + s_off[valid ? le : 0] : 0u);   // at most 15 + T * dt_max_line(k) <= 15 + DT_IMG behind img
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
      uint32_t x = F.len;   // inclusive scan inside the entry's P lanes
      for (uint32_t o = 1; o < P; o <<= 1) {
        const uint32_t y = (uint32_t)__shfl_up((int)x, o, 64);
        if (g >= o) x += y;
      }
      if (EMIT && F.len) dfh_dt::dt_put_field(line + at + (x - F.len), F);
      at += (uint32_t)__shfl((int)x, (int)(lead + P - 1u), 64);
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
    if (irr) atomicAdd(&s_acc[1], irr);
    __syncthreads();
    if (threadIdx.x == 0) {
      tile_bytes[blockIdx.x] = s_acc[0];
      if (blockIdx.x == 0) tile_bytes[gridDim.x] = 0;
      if (s_acc[1]) atomicAdd(irregular, s_acc[1]);
    }
    return;
  }
  __syncthreads();   // the image is complete
  const uint64_t a0 = (g_first + 15) & ~15ULL, a1 = g_end & ~15ULL;   // the aligned words lie in [a0, a1)
  const uint64_t head_end = a0 < g_end ? a0 : g_end;
  for (uint64_t q = g_first + threadIdx.x; q < head_end; q += 256) out[q] = img[q - g_img];
  for (uint64_t q = a0 + 16ULL * threadIdx.x; q < a1; q += 16ULL * 256)
    *reinterpret_cast<uint4*>(out + q) = *reinterpret_cast<const uint4*>(img + (q - g_img));
  for (uint64_t q = (a1 > head_end ? a1 : head_end) + threadIdx.x; q < g_end; q += 256) out[q] = img[q - g_img];
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

// a workspace array of at least `count` T (the call that used it last has waited for its work)
template <typename T>
int dt_grow(T** ptr, size_t* cap, size_t count, const char* who, const char* what) {
  if (count <= *cap) return DFH_OK;
  if (*ptr) (void)hipFree(*ptr);
  *ptr = nullptr;
  *cap = 0;
  if (hipMalloc(reinterpret_cast<void**>(ptr), count * sizeof(T)) != hipSuccess) {
    (void)hipGetLastError();
    *ptr = nullptr;
    set_error(std::string(who) + ": no device memory for " + what + " (" + std::to_string(count * sizeof(T)) + " bytes needed)");
    return DFH_ERR_CAPACITY;
  }
  *cap = count;
  return DFH_OK;
}
}  // namespace

extern "C" {

int dfh_dump_close(dfh_dump* p) {
  if (!p) return DFH_OK;
  (void)hipSetDevice(p->ctx->device);
  (void)hipStreamSynchronize(p->ctx->stream);
  if (p->d_id) (void)hipFree(p->d_id);
  if (p->d_row) (void)hipFree(p->d_row);
  if (p->d_text) (void)hipFree(p->d_text);
  if (p->d_elen) (void)hipFree(p->d_elen);
  if (p->d_tile) (void)hipFree(p->d_tile);
  if (p->d_tile_scan) (void)hipFree(p->d_tile_scan);
  if (p->d_tmp) (void)hipFree(p->d_tmp);
  if (p->d_cnt) (void)hipFree(p->d_cnt);
  if (p->d_ent) (void)hipFree(p->d_ent);
  if (p->h_head) (void)hipHostFree(p->h_head);
  if (p->h_text) (void)hipHostFree(p->h_text);
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
  p->tile = (uint32_t)std::min<uint64_t>(DT_TILE_MAX, DT_IMG / max_line);
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
  hipError_t e = hipMalloc(reinterpret_cast<void**>(&p->d_cnt), 4 * sizeof(uint32_t));
  if (e == hipSuccess) e = hipHostMalloc(reinterpret_cast<void**>(&p->h_head), 2 * sizeof(uint64_t), hipHostMallocDefault);
  if (e == hipSuccess) e = hipMemsetAsync(p->d_cnt, 0, 4 * sizeof(uint32_t), s);
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
  p->text_bytes = 0;
  if (count == 0) {
    p->formatted = true;
    return DFH_OK;
  }
  const size_t ntiles = (count + p->tile - 1) / p->tile;
  size_t need = 0;
  DFH_HIP(rocprim::exclusive_scan(nullptr, need, (uint64_t*)nullptr, (uint64_t*)nullptr, (uint64_t)0, ntiles + 1, rocprim::plus<uint64_t>(), s));
  const char* who = "dfh_dump_format";
  int rc = dt_grow(&p->d_text, &p->text_cap, count * (size_t)dfh_dt::dt_max_line(p->k), who, "the text");
  if (!rc) rc = dt_grow(&p->d_elen, &p->elen_cap, count, who, "the entries' byte counts");
  if (!rc) rc = dt_grow(&p->d_tile, &p->tile_cap, ntiles + 1, who, "the tiles' byte counts");
  if (!rc) rc = dt_grow(&p->d_tile_scan, &p->scan_cap, ntiles + 1, who, "the tiles' offsets");
  if (!rc) {
    char* tmp = static_cast<char*>(p->d_tmp);
    rc = dt_grow(&tmp, &p->tmp_bytes, std::max<size_t>(need, 256), who, "the scan");
    p->d_tmp = tmp;
  }
  if (rc) return rc;
  uint32_t* d_irr = p->d_cnt + 2;
  DFH_HIP(hipMemsetAsync(d_irr, 0, sizeof(uint32_t), s));
  const TableView& v = p->t->v;
  const uint64_t* ids = p->d_id + first;
  const uint32_t* rows = p->d_row + first;
  hipLaunchKernelGGL(k_dumptext<0>, dim3((unsigned)ntiles), dim3(256), 0, s, (const RowHdr*)v.hdr, (const float*)v.va, p->k, (uint32_t)v.kp, ids,
                     rows, (uint64_t)count, p->tile, p->lp, p->d_elen, p->d_tile, (const uint64_t*)nullptr, (unsigned char*)nullptr, d_irr);
  DFH_HIP(hipGetLastError());
  size_t tb = p->tmp_bytes;
  DFH_HIP(rocprim::exclusive_scan(p->d_tmp, tb, p->d_tile, p->d_tile_scan, (uint64_t)0, ntiles + 1, rocprim::plus<uint64_t>(), s));
  hipLaunchKernelGGL(k_dumptext<1>, dim3((unsigned)ntiles), dim3(256), 0, s, (const RowHdr*)v.hdr, (const float*)v.va, p->k, (uint32_t)v.kp, ids,
                     rows, (uint64_t)count, p->tile, p->lp, p->d_elen, (uint64_t*)nullptr, (const uint64_t*)p->d_tile_scan,
                     reinterpret_cast<unsigned char*>(p->d_text), (uint32_t*)nullptr);
  DFH_HIP(hipGetLastError());
  p->h_head[0] = p->h_head[1] = 0;
  DFH_HIP(hipMemcpyAsync(&p->h_head[0], p->d_tile_scan + ntiles, sizeof(uint64_t), hipMemcpyDeviceToHost, s));
  DFH_HIP(hipMemcpyAsync(&p->h_head[1], d_irr, sizeof(uint32_t), hipMemcpyDeviceToHost, s));
  DFH_HIP(hipStreamSynchronize(s));
  p->text_bytes = (size_t)p->h_head[0];
  p->formatted = true;
  *nbytes = p->text_bytes;
  *irregular = p->h_head[1];
  return DFH_OK;
}

int dfh_dump_read(dfh_dump* p, char* dst) {
  DFH_ARG(p && (dst || p->text_bytes == 0), "dfh_dump_read: NULL argument");
  if (!p->formatted) {
    set_error("dfh_dump_read: nothing formatted (call dfh_dump_format first)");
    return DFH_ERR_STATE;
  }
  const size_t nb = p->text_bytes;
  if (nb == 0) return DFH_OK;
  DFH_HIP(hipSetDevice(p->ctx->device));
  if (nb > p->h_text_cap) {   // the download lands in page-locked memory of the object's, kept
    if (p->h_text) DFH_HIP(hipHostFree(p->h_text));
    p->h_text = nullptr;
    p->h_text_cap = 0;
    const size_t c = nb + nb / 4;
    DFH_HIP(hipHostMalloc(reinterpret_cast<void**>(&p->h_text), c, hipHostMallocDefault));
    p->h_text_cap = c;
  }
  DFH_HIP(hipMemcpyAsync(p->h_text, p->d_text, nb, hipMemcpyDeviceToHost, p->ctx->stream));
  DFH_HIP(hipStreamSynchronize(p->ctx->stream));
  memcpy(dst, p->h_text, nb);
  return DFH_OK;
}

int dfh_dump_entries(dfh_dump* p, uint64_t first, size_t count, uint64_t* ids, float* w, int* has_V, float* V) {
  DFH_ARG(p, "dfh_dump_entries: NULL argument");
  DFH_ARG(first <= p->n && count <= p->n - first, "dfh_dump_entries: first + count exceeds the dump's entries");
  if (count == 0) return DFH_OK;
  DFH_ARG(ids && w && has_V && (V || p->k == 0), "dfh_dump_entries: NULL argument");
  hipStream_t s = p->ctx->stream;
  DFH_HIP(hipSetDevice(p->ctx->device));
  const size_t k = p->k, per = sizeof(uint64_t) + sizeof(float) + sizeof(int) + k * sizeof(float);
  int rc = dt_grow(&p->d_ent, &p->ent_cap, count * per + 256, "dfh_dump_entries", "the entries");
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

}  // extern "C"
