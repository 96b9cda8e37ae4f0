// dfh_textparse.hip — the device text parse of the SGD feed (included in dfh_api.hip ahead of dfh_feed.hip, whose uploads
// take the parsed ids where this file leaves them).  CriteoParser::ParseNext (src/reader/criteo_parser.h:40-94) for the
// chunks every real file is made of: a REGULAR chunk is non-empty, ends with '\n', holds no '\r' and no empty line, every line
// has exactly `ntab` tabs (39: criteo, 38: criteo_test), the label is one character '0'..'9', an integer field has 0..16 bytes
// (hashed as they are), a categorical field has 0 bytes or 8 that do not start with ' ', '\v' or '\f' (the condition of
// CriteoChunkParser::ParseFast, host/batch_reader.h).  For such a chunk row r field j lies between delimiters
// r (ntab + 1) + j - 1 and r (ntab + 1) + j, and the ids are what the host parser writes, bit for bit; any other chunk is
// reported as not regular and nothing else is said about it: the caller parses it on the host.
//
// Five launches and two library scans, ordered by the stream alone; nothing is handed from block to block inside a launch,
// the only word blocks share is the flag word they OR their findings into:
//   k_tp_count      per tile of 4 096 bytes: the number of '\t' + '\n' and of '\n' (one u64), '\r' seen -> flag
//   scan            tile counts -> the first delimiter of every tile; the totals go to the host, which sizes the arrays
//   k_tp_positions  the delimiters' byte positions, compacted; every (ntab + 1)-th must be the '\n' -> flag
//   k_tp_fields     a wave per row, a lane per field: length classes, the label, the row's non-empty fields -> flag
//   scan            non-empty counts -> row offsets
//   k_tp_emit       (CityHash64(token) << 12) | slot at offset[row] + the field's rank among the row's non-empty fields
// The text buffer is padded: a lane's 16-byte load and the five aligned words a token is assembled from (tokens start at
// any byte; no unaligned load is issued) stay inside the allocation.
struct dfh_lzd;   // the LZ4 decoder's arrays of a chunk that holds decoded records (dfh_lz4dec.hip)
namespace {
void lzd_free(dfh_lzd* z);
}
struct dfh_textchunk {
  dfh_ctx* ctx = nullptr;
  hipStream_t s = nullptr;   // the context's parse stream (one per context, not one per chunk: a process has 4 hardware queues)
  hipEvent_t ev = nullptr;
  size_t cap_bytes = 0, cap_tile = 0, cap_tile_scan = 0, cap_delims = 0, cap_cnt = 0, cap_off = 0, cap_lab = 0, cap_nnz = 0, tmp_bytes = 0;   // elements each array holds
  char* d_text = nullptr;
  uint64_t *d_tile = nullptr, *d_tile_scan = nullptr;   // [tiles + 1]: delimiters | newlines << 32 per tile, and before it
  uint32_t* d_pos = nullptr;                            // [delimiters]
  uint32_t *d_cnt = nullptr, *d_off = nullptr;          // [rows + 1]
  float* d_lab = nullptr;                               // [rows]
  uint64_t* d_ids = nullptr;                            // [nnz]
  uint32_t* d_flag = nullptr;
  void* d_tmp = nullptr;
  uint64_t* h_head = nullptr;                           // page-locked: totals, flag
  char* h_rows = nullptr;                               // page-locked: offsets [rows + 1] | labels [rows]
  size_t h_rows_cap = 0;
  size_t nrows = 0, nnz = 0;
  bool valid = false;                                   // the last parse found a regular chunk
  dfh_lzd* lzd = nullptr;                               // rec_decode = device: created by the first record
};

namespace {
constexpr uint32_t TP_TILE = 4096;       // 256 lanes x 16 bytes
constexpr uint32_t TP_PAD = 64;          // bytes behind the last tile
constexpr uint32_t TP_FLAG_CR = 1u, TP_FLAG_PATTERN = 2u, TP_FLAG_FIELD = 4u;
constexpr uint32_t TP_ROWS_PER_BLOCK = 4;   // a wave per row

// 0x80 in every byte of x that equals the byte c4 repeats (exact per byte: no borrow crosses a byte)
__device__ __forceinline__ uint32_t tp_eq(uint32_t x, uint32_t c4) {
  const uint32_t y = x ^ c4;
  const uint32_t t = (y & 0x7f7f7f7fu) + 0x7f7f7f7fu;
  return ~(t | y | 0x7f7f7f7fu);
}
// bits 7, 15, 23, 31 -> bits 0 .. 3 (the sixteen partial products land on different bits)
__device__ __forceinline__ uint32_t tp_bits(uint32_t t) { return (((t >> 7) * 0x00204081u) >> 21) & 0xFu; }

struct TpMasks { uint32_t delim, nl, cr; };   // bit b: byte at + b is a '\t' or '\n' / a '\n' / a '\r'
// the lane's 16 bytes at `at` (a multiple of 16 inside the padded allocation); bytes at or beyond len do not count
__device__ __forceinline__ TpMasks tp_masks(const char* __restrict__ text, uint32_t len, uint32_t at) {
  TpMasks m{0u, 0u, 0u};
  if (at >= len) return m;
  const uint4 v = *reinterpret_cast<const uint4*>(text + at);
  const uint32_t w[4] = {v.x, v.y, v.z, v.w};
  uint32_t tab = 0;
#pragma unroll
  for (int k = 0; k < 4; ++k) {
    tab |= tp_bits(tp_eq(w[k], 0x09090909u)) << (4 * k);
    m.nl |= tp_bits(tp_eq(w[k], 0x0a0a0a0au)) << (4 * k);
    m.cr |= tp_bits(tp_eq(w[k], 0x0d0d0d0du)) << (4 * k);
  }
  const uint32_t valid = len - at >= 16u ? 0xFFFFu : (1u << (len - at)) - 1u;
  m.nl &= valid;
  m.cr &= valid;
  m.delim = (tab & valid) | m.nl;
  return m;
}

__global__ void __launch_bounds__(256) k_tp_count(const char* __restrict__ text, uint32_t len, uint64_t* __restrict__ tile_cnt,
                                                  uint32_t* __restrict__ flag) {
  __shared__ uint32_t s_d[4], s_n[4];
  const uint32_t lane = threadIdx.x & 63u, w = threadIdx.x >> 6;
  const TpMasks m = tp_masks(text, len, blockIdx.x * TP_TILE + threadIdx.x * 16u);
  uint32_t d = __popc(m.delim), n = __popc(m.nl);
#pragma unroll
  for (int o = 32; o > 0; o >>= 1) {
    d += __shfl_xor(d, o);
    n += __shfl_xor(n, o);
  }
  const unsigned long long any_cr = __ballot(m.cr != 0u);
  if (lane == 0) {
    s_d[w] = d;
    s_n[w] = n;
    if (any_cr) atomicOr(flag, TP_FLAG_CR);
  }
  __syncthreads();
  if (threadIdx.x == 0) {
    tile_cnt[blockIdx.x] = (uint64_t)(s_d[0] + s_d[1] + s_d[2] + s_d[3]) | ((uint64_t)(s_n[0] + s_n[1] + s_n[2] + s_n[3]) << 32);
    if (blockIdx.x == 0) tile_cnt[gridDim.x] = 0;   // the scan's last input: its output there is the total
  }
}

__global__ void __launch_bounds__(256) k_tp_positions(const char* __restrict__ text, uint32_t len, const uint64_t* __restrict__ tile_first,
                                                      uint32_t* __restrict__ pos, uint32_t ndelims, uint32_t period,
                                                      uint32_t* __restrict__ flag) {
  using Scan = rocprim::block_scan<uint32_t, 256>;
  __shared__ typename Scan::storage_type s_scan;
  const uint32_t at = blockIdx.x * TP_TILE + threadIdx.x * 16u;
  const TpMasks m = tp_masks(text, len, at);
  uint32_t before = 0;
  Scan().exclusive_scan(__popc(m.delim), before, 0u, s_scan);
  uint32_t g = (uint32_t)tile_first[blockIdx.x] + before;   // this lane's first delimiter
  uint32_t r = (g + 1u) % period;                           // 0: delimiter g ends a row
  bool bad = false;
  for (uint32_t d = m.delim; d; d &= d - 1u) {
    const uint32_t b = __ffs(d) - 1u;
    if (g < ndelims) pos[g] = at + b;
    bad |= (r == 0u) != (((m.nl >> b) & 1u) != 0u);
    r = r + 1u == period ? 0u : r + 1u;
    ++g;
  }
  if (__ballot(bad) && (threadIdx.x & 63u) == 0) atomicOr(flag, TP_FLAG_PATTERN);
}

// field j of row r: [start, start + len), slot = j - is_train (-1: the label)
struct TpField { uint32_t start, len; int slot; bool active; };
__device__ __forceinline__ TpField tp_field(const uint32_t* __restrict__ pos, uint32_t r, uint32_t lane, uint32_t period, int is_train) {
  TpField f{0u, 0u, (int)lane - is_train, lane < period};
  if (f.active) {
    const uint32_t g = r * period + lane;
    f.start = g ? pos[g - 1u] + 1u : 0u;
    f.len = pos[g] - f.start;
  }
  return f;
}

__global__ void __launch_bounds__(256) k_tp_fields(const char* __restrict__ text, const uint32_t* __restrict__ pos, uint32_t nrows,
                                                   uint32_t period, int is_train, uint32_t* __restrict__ cnt, float* __restrict__ lab,
                                                   uint32_t* __restrict__ flag) {
  const uint32_t lane = threadIdx.x & 63u, r = blockIdx.x * TP_ROWS_PER_BLOCK + (threadIdx.x >> 6);
  if (blockIdx.x == 0 && threadIdx.x == 0) cnt[nrows] = 0;   // the scan's last input: its output there is nnz
  if (r >= nrows) return;
  const TpField f = tp_field(pos, r, lane, period, is_train);
  bool bad = false, nonempty = false;
  if (f.active) {
    const uint32_t c = (uint8_t)text[f.start];   // (an empty field: the delimiter that ends it)
    if (f.slot < 0) {   // atof of one digit
      const bool ok = f.len == 1u && c - (uint32_t)'0' < 10u;
      bad = !ok;
      lab[r] = ok ? (float)(c - (uint32_t)'0') : 0.0f;
    } else if (f.slot < 13) {
      bad = f.len > 16u;
      nonempty = f.len != 0u;
    } else {
      nonempty = f.len != 0u;
      bad = nonempty && (f.len != 8u || c == (uint32_t)' ' || c == (uint32_t)'\v' || c == (uint32_t)'\f');
    }
  }
  const unsigned long long ne = __ballot(nonempty), anybad = __ballot(bad);
  if (lane == 0) {
    cnt[r] = (uint32_t)__popcll(ne);
    if (!is_train) lab[r] = 0.0f;
    if (anybad) atomicOr(flag, TP_FLAG_FIELD);
  }
}

// CityHash64 of a token of 1 .. 16 bytes at byte `start` (city.cc HashLen0to16; host/cityhash.h): the token's first 16 bytes
// as four words put together from five ALIGNED words, what lies behind the token is masked by the length class
__device__ __forceinline__ uint64_t tp_rot(uint64_t v, int s) { return (v >> s) | (v << (64 - s)); }
__device__ __forceinline__ uint64_t tp_hash_len16(uint64_t u, uint64_t v, uint64_t mul) {
  uint64_t a = (u ^ v) * mul;
  a ^= a >> 47;
  uint64_t b = (v ^ a) * mul;
  b ^= b >> 47;
  return b * mul;
}
__device__ __forceinline__ uint64_t tp_cityhash(const char* __restrict__ text, uint32_t start, uint32_t len) {
  constexpr uint64_t k0 = 0xc3a5c85c97cb3127ULL, k2 = 0x9ae16a3b2f90404fULL;
  const uint32_t* wp = reinterpret_cast<const uint32_t*>(text + (start & ~3u));
  const uint32_t sh = start & 3u;
  const uint32_t a0 = wp[0], a1 = wp[1];
  const uint32_t w0 = __builtin_amdgcn_alignbyte(a1, a0, sh);
  if (len < 4u) {
    const uint32_t a = w0 & 0xffu, b = (w0 >> (8u * (len >> 1))) & 0xffu, c = (w0 >> (8u * (len - 1u))) & 0xffu;
    const uint32_t y = a + (b << 8), z = len + (c << 2);
    const uint64_t h = y * k2 ^ z * k0;
    return (h ^ (h >> 47)) * k2;
  }
  const uint32_t a2 = wp[2];
  const uint64_t lo = (uint64_t)w0 | ((uint64_t)__builtin_amdgcn_alignbyte(a2, a1, sh) << 32);   // bytes 0 .. 7
  const uint64_t mul = k2 + 2ull * len;
  if (len < 8u) return tp_hash_len16(len + ((uint64_t)w0 << 3), (uint32_t)(lo >> (8u * (len - 4u))), mul);
  const uint32_t a3 = wp[3], a4 = wp[4];
  const uint64_t hi = (uint64_t)__builtin_amdgcn_alignbyte(a3, a2, sh) | ((uint64_t)__builtin_amdgcn_alignbyte(a4, a3, sh) << 32);
  const uint32_t k = 8u * (len - 8u);   // the last 8 bytes start k bits into lo
  const uint64_t b = k == 0u ? lo : (k == 64u ? hi : (lo >> k) | (hi << (64u - k)));
  const uint64_t a = lo + k2;
  return tp_hash_len16(tp_rot(b, 37) * mul + a, (tp_rot(a, 25) + b) * mul, mul);
}

__global__ void __launch_bounds__(256) k_tp_emit(const char* __restrict__ text, const uint32_t* __restrict__ pos, uint32_t nrows,
                                                 uint32_t period, int is_train, const uint32_t* __restrict__ off,
                                                 uint64_t* __restrict__ ids, const uint32_t* __restrict__ flag) {
  const uint32_t lane = threadIdx.x & 63u, r = blockIdx.x * TP_ROWS_PER_BLOCK + (threadIdx.x >> 6);
  if (r >= nrows || *flag != 0u) return;   // (not regular: the lengths are not what the hash expects, and nobody reads the ids)
  const TpField f = tp_field(pos, r, lane, period, is_train);
  const bool nonempty = f.active && f.slot >= 0 && f.len != 0u;
  const unsigned long long ne = __ballot(nonempty);
  if (!nonempty) return;
  const uint32_t rank = (uint32_t)__popcll(ne & ((1ull << lane) - 1ull));
  ids[off[r] + rank] = (tp_cityhash(text, f.start, f.len) << 12) | (uint64_t)f.slot;   // EncodeFeaGrpID(h, slot, 12)
}

// *d_ptr (*cap elements) holds at least `need` elements afterwards; what it held is not kept
template <typename T>
int tp_reserve(T** d_ptr, size_t* cap, size_t need) {
  if (*d_ptr && *cap >= need) return DFH_OK;
  if (*d_ptr) DFH_HIP(hipFree(*d_ptr));
  *d_ptr = nullptr;
  *cap = 0;
  const size_t n = need + need / 8;
  DFH_HIP(hipMalloc(reinterpret_cast<void**>(d_ptr), n * sizeof(T)));
  *cap = n;
  return DFH_OK;
}
int tp_wait(dfh_textchunk* tc) {
  DFH_HIP(hipEventRecord(tc->ev, tc->s));
  DFH_HIP(hipEventSynchronize(tc->ev));
  return DFH_OK;
}
}  // namespace

extern "C" {

int dfh_textchunk_destroy(dfh_textchunk* tc) {
  if (!tc) return DFH_OK;
  hipSetDevice(tc->ctx->device);
  if (tc->ev) {
    hipEventSynchronize(tc->ev);
    hipEventDestroy(tc->ev);
  }
  for (void* p : {(void*)tc->d_text, (void*)tc->d_tile, (void*)tc->d_tile_scan, (void*)tc->d_pos, (void*)tc->d_cnt, (void*)tc->d_off,
                  (void*)tc->d_lab, (void*)tc->d_ids, (void*)tc->d_flag, tc->d_tmp})
    if (p) hipFree(p);
  if (tc->h_head) hipHostFree(tc->h_head);
  if (tc->h_rows) hipHostFree(tc->h_rows);
  lzd_free(tc->lzd);
  delete tc;
  return DFH_OK;
}

int dfh_textchunk_create(dfh_ctx* c, size_t max_bytes, dfh_textchunk** out) {
  DFH_ARG(c && out && max_bytes >= 1 && max_bytes < (1ULL << 31), "dfh_textchunk_create: bad argument / a chunk holds fewer than 2^31 bytes");
  DFH_HIP(hipSetDevice(c->device));
  {
    std::lock_guard<std::mutex> lk(c->parse_mu);
    if (!c->parse) DFH_HIP(hipStreamCreateWithFlags(&c->parse, hipStreamNonBlocking));
  }
  dfh_textchunk* tc = new (std::nothrow) dfh_textchunk();
  if (!tc) {
    set_error("dfh_textchunk_create: out of host memory");
    return DFH_ERR_HIP;
  }
  tc->ctx = c;
  tc->s = c->parse;
  const size_t bytes = (max_bytes + TP_TILE - 1) / TP_TILE * TP_TILE + TP_PAD;
  hipError_t e;
  if ((e = hipMalloc(reinterpret_cast<void**>(&tc->d_text), bytes)) != hipSuccess ||
      (e = hipMalloc(reinterpret_cast<void**>(&tc->d_flag), sizeof(uint32_t))) != hipSuccess ||
      (e = hipHostMalloc(reinterpret_cast<void**>(&tc->h_head), 2 * sizeof(uint64_t), hipHostMallocDefault)) != hipSuccess ||
      (e = hipEventCreateWithFlags(&tc->ev, hipEventDisableTiming)) != hipSuccess) {
    set_error(std::string("dfh_textchunk_create: ") + hipGetErrorString(e));
    dfh_textchunk_destroy(tc);
    return DFH_ERR_HIP;
  }
  tc->cap_bytes = bytes;
  *out = tc;
  return DFH_OK;
}

int dfh_textchunk_parse_criteo(dfh_textchunk* tc, const char* text, size_t len, int is_train, int* regular, size_t* nrows, size_t* nnz) {
  DFH_ARG(tc && regular && nrows && nnz && (text || len == 0), "dfh_textchunk_parse_criteo: NULL argument");
  *regular = 0;
  *nrows = *nnz = 0;
  tc->valid = false;
  if (len == 0 || len >= (1ULL << 31) || text[len - 1] != '\n') return DFH_OK;   // empty, beyond 32-bit positions, no final '\n'
  DFH_HIP(hipSetDevice(tc->ctx->device));
  hipStream_t s = tc->s;
  const uint32_t period = is_train ? 40u : 39u;   // delimiters per row: ntab tabs and the '\n'
  const size_t ntiles = (len + TP_TILE - 1) / TP_TILE, bytes = ntiles * TP_TILE + TP_PAD;
  int rc = tp_reserve(&tc->d_text, &tc->cap_bytes, bytes);
  if (!rc) rc = tp_reserve(&tc->d_tile, &tc->cap_tile, ntiles + 1);
  if (!rc) rc = tp_reserve(&tc->d_tile_scan, &tc->cap_tile_scan, ntiles + 1);
  if (rc) return rc;
  size_t need = 0;
  DFH_HIP(rocprim::exclusive_scan(nullptr, need, (uint64_t*)nullptr, (uint64_t*)nullptr, (uint64_t)0, ntiles + 1, rocprim::plus<uint64_t>(), s));
  {
    char* tmp = static_cast<char*>(tc->d_tmp);
    rc = tp_reserve(&tmp, &tc->tmp_bytes, std::max<size_t>(need, 256));
    tc->d_tmp = tmp;
    if (rc) return rc;
  }
  DFH_HIP(hipMemcpyAsync(tc->d_text, text, len, hipMemcpyHostToDevice, s));
  DFH_HIP(hipMemsetAsync(tc->d_text + len, 0, bytes - len, s));
  DFH_HIP(hipMemsetAsync(tc->d_flag, 0, sizeof(uint32_t), s));
  hipLaunchKernelGGL(k_tp_count, dim3((unsigned)ntiles), dim3(256), 0, s, tc->d_text, (uint32_t)len, tc->d_tile, tc->d_flag);
  DFH_HIP(hipGetLastError());
  size_t tb = tc->tmp_bytes;
  DFH_HIP(rocprim::exclusive_scan(tc->d_tmp, tb, tc->d_tile, tc->d_tile_scan, (uint64_t)0, ntiles + 1, rocprim::plus<uint64_t>(), s));
  DFH_HIP(hipMemcpyAsync(&tc->h_head[0], tc->d_tile_scan + ntiles, sizeof(uint64_t), hipMemcpyDeviceToHost, s));
  DFH_HIP(hipMemcpyAsync(&tc->h_head[1], tc->d_flag, sizeof(uint32_t), hipMemcpyDeviceToHost, s));
  rc = tp_wait(tc);
  if (rc) return rc;
  const uint64_t ndel = tc->h_head[0] & 0xFFFFFFFFULL, nl = tc->h_head[0] >> 32;
  if ((uint32_t)tc->h_head[1] != 0u || nl == 0 || ndel != nl * period) return DFH_OK;   // a '\r', or the counts do not fit
  // rows <= '\n', ids <= 39 per row: the arrays grow to what this chunk needs
  const size_t rows = (size_t)nl, max_ids = rows * 39;
  rc = tp_reserve(&tc->d_pos, &tc->cap_delims, (size_t)ndel);
  if (!rc) rc = tp_reserve(&tc->d_cnt, &tc->cap_cnt, rows + 1);
  if (!rc) rc = tp_reserve(&tc->d_off, &tc->cap_off, rows + 1);
  if (!rc) rc = tp_reserve(&tc->d_lab, &tc->cap_lab, rows);
  if (!rc) rc = tp_reserve(&tc->d_ids, &tc->cap_nnz, std::max<size_t>(max_ids, 1));
  if (rc) return rc;
  if (tc->h_rows_cap < rows + 1) {
    if (tc->h_rows) DFH_HIP(hipHostFree(tc->h_rows));
    tc->h_rows = nullptr;
    tc->h_rows_cap = 0;
    const size_t n = rows + 1 + rows / 8;
    DFH_HIP(hipHostMalloc(reinterpret_cast<void**>(&tc->h_rows), n * 8, hipHostMallocDefault));
    tc->h_rows_cap = n;
  }
  need = 0;
  DFH_HIP(rocprim::exclusive_scan(nullptr, need, (uint32_t*)nullptr, (uint32_t*)nullptr, 0u, rows + 1, rocprim::plus<uint32_t>(), s));
  {
    char* tmp = static_cast<char*>(tc->d_tmp);
    rc = tp_reserve(&tmp, &tc->tmp_bytes, std::max<size_t>(need, 256));
    tc->d_tmp = tmp;
    if (rc) return rc;
  }
  const unsigned row_blocks = (unsigned)((rows + TP_ROWS_PER_BLOCK - 1) / TP_ROWS_PER_BLOCK);
  hipLaunchKernelGGL(k_tp_positions, dim3((unsigned)ntiles), dim3(256), 0, s, tc->d_text, (uint32_t)len, tc->d_tile_scan, tc->d_pos,
                     (uint32_t)ndel, period, tc->d_flag);
  hipLaunchKernelGGL(k_tp_fields, dim3(row_blocks), dim3(256), 0, s, tc->d_text, tc->d_pos, (uint32_t)rows, period, is_train ? 1 : 0,
                     tc->d_cnt, tc->d_lab, tc->d_flag);
  DFH_HIP(hipGetLastError());
  tb = tc->tmp_bytes;
  DFH_HIP(rocprim::exclusive_scan(tc->d_tmp, tb, tc->d_cnt, tc->d_off, 0u, rows + 1, rocprim::plus<uint32_t>(), s));
  hipLaunchKernelGGL(k_tp_emit, dim3(row_blocks), dim3(256), 0, s, tc->d_text, tc->d_pos, (uint32_t)rows, period, is_train ? 1 : 0, tc->d_off,
                     tc->d_ids, tc->d_flag);
  DFH_HIP(hipGetLastError());
  DFH_HIP(hipMemcpyAsync(tc->h_rows, tc->d_off, (rows + 1) * sizeof(uint32_t), hipMemcpyDeviceToHost, s));
  DFH_HIP(hipMemcpyAsync(tc->h_rows + tc->h_rows_cap * 4, tc->d_lab, rows * sizeof(float), hipMemcpyDeviceToHost, s));
  DFH_HIP(hipMemcpyAsync(&tc->h_head[1], tc->d_flag, sizeof(uint32_t), hipMemcpyDeviceToHost, s));
  rc = tp_wait(tc);
  if (rc) return rc;
  if ((uint32_t)tc->h_head[1] != 0u) return DFH_OK;
  tc->nrows = rows;
  tc->nnz = reinterpret_cast<const uint32_t*>(tc->h_rows)[rows];
  tc->valid = true;
  *regular = 1;
  *nrows = tc->nrows;
  *nnz = tc->nnz;
  return DFH_OK;
}

int dfh_textchunk_rows(dfh_textchunk* tc, uint32_t* offset, float* label) {
  DFH_ARG(tc && tc->valid && offset && label, "dfh_textchunk_rows: no regular chunk parsed / NULL argument");
  memcpy(offset, tc->h_rows, (tc->nrows + 1) * sizeof(uint32_t));
  memcpy(label, tc->h_rows + tc->h_rows_cap * 4, tc->nrows * sizeof(float));
  return DFH_OK;
}

int dfh_textchunk_ids(dfh_textchunk* tc, uint64_t* index) {
  DFH_ARG(tc && tc->valid && (index || tc->nnz == 0), "dfh_textchunk_ids: no regular chunk parsed / NULL argument");
  DFH_HIP(hipSetDevice(tc->ctx->device));
  if (tc->nnz) DFH_HIP(hipMemcpy(index, tc->d_ids, tc->nnz * sizeof(uint64_t), hipMemcpyDeviceToHost));
  return DFH_OK;
}

}  // extern "C"
