// dfh_lz4enc.hip — the device LZ4 block encoder and the CompressedRowBlock writer of task = convert (included in dfh_api.hip
// behind dfh_textparse.hip, whose parsed chunks it encodes where they lie).  One array in HBM -> ONE LZ4 block (the format is
// described at the top of host/lz4_block.h) that honours the end rules LZ4_decompress_safe relies on: the last sequence is
// literals only, the last 5 bytes are literals, no match starts within the last 12 bytes, offsets are 1 .. 65535.  The bytes
// are not liblz4's; the same input gives the same bytes on every run.
//
// The input is cut into segments of LZ_SEG bytes, a wave per segment, and goes through four launches ordered by the stream:
//   k_lz4_find   candidate positions are the 4-byte-aligned ones (the arrays are made of 4- and 8-byte elements).  The wave
//                first enters the LZ_LOOKBACK words before its segment into a hash table in LDS (atomicMax on the position: the
//                table's content does not depend on the order of the lanes), then walks the segment 64 positions per step:
//                every lane reads its candidate — the table holds the positions of EARLIER steps only — and tries it, the
//                nearest earlier lane of the step that holds the same word, and the fixed candidates one and two words back
//                (the distances 4 and 8 that offsets, labels and runs live on); of equally long matches the first tried
//                stays.  A match is extended forward up to the segment's end and the block's last 5 bytes, and up to 3 bytes
//                backward; then the step's positions are entered.  A greedy chain is picked per step: the first lane at or behind the end of the
//                previous match that has one.  A match refers back into earlier segments freely but never runs over its own
//                segment's end, so segments do not depend on each other.  Per segment: the sequence list {match start, length,
//                distance}, the end of its last match, its first literal run, its output size when no literals come in.
//   k_lz4_place  one block scans the segments: the literals behind a segment's last match belong to the first sequence of the
//                next segment that has a match (to the block's last sequence when none has), so a segment's size depends on
//                the CARRY coming in = its first byte - the end of the last match before it (a prefix maximum); the carry fixes
//                the sizes, a prefix sum of the sizes the output positions.  The block's total size goes to `head`.
//   k_lz4_emit   a wave per segment writes its sequences at those positions: token, length bytes (15, then 255-runs),
//                literals, offset; a lane per sequence, literal runs of more than 32 bytes copied by the whole wave.
//   k_lz4_last   the block's last sequence (literals only), by the whole grid.
// Vector byte stores and plain C++ only.  Nothing waits on the host except the read-back of the sizes.
struct dfh_crb {
  dfh_ctx* ctx = nullptr;
  hipStream_t s = nullptr;
  hipEvent_t ev = nullptr;
  char* d_in = nullptr;         // uploaded / widened arrays, each at a 16-byte aligned position
  char* d_out = nullptr;        // the blocks, each in a region of its bound
  uint2* d_seq = nullptr;       // [segments x LZ_MAX_SEQ] {match start, length | distance << 16}
  uint4* d_meta = nullptr;      // [segments] {sequences, end of the last match (0: none), size without carry, first literal run}
  uint2* d_segpos = nullptr;    // [segments] {output position, start of the literals that come in}
  uint4* d_head = nullptr;      // [5] {block size, start of the last literals, their output position, 0}
  uint32_t* h_head = nullptr;   // page-locked copy
  char* d_gather = nullptr;     // labels, offsets and weights of a block gathered out of a row store (dfh_rowstore.hip)
  size_t cap_in = 0, cap_out = 0, cap_seq = 0, cap_meta = 0, cap_segpos = 0, cap_gather = 0;
  // the last encode
  int nrows = 0;
  size_t out_at[5] = {0, 0, 0, 0, 0};
  uint32_t out_size[5] = {0, 0, 0, 0, 0};   // 0: the array is absent
  size_t record_bytes = 0;
  bool valid = false;
};

namespace {
constexpr uint32_t LZ_SEG = 4096, LZ_SEG_WORDS = LZ_SEG / 4, LZ_MAX_SEQ = LZ_SEG_WORDS;   // a match starts at most once per word
constexpr uint32_t LZ_TAB = 4096;                      // 16 KiB of LDS per wave
constexpr uint32_t LZ_LOOKBACK = 3 * LZ_SEG_WORDS;     // words ahead of the segment that are entered into its table
constexpr uint32_t LZ_LONG_LIT = 32;                   // literal runs beyond this are copied by the whole wave
constexpr size_t LZ_MAX_INPUT = (1ULL << 31) - (1ULL << 25);   // liblz4's LZ4_MAX_INPUT_SIZE is one below

__host__ __device__ __forceinline__ uint32_t lz_ext(uint32_t len) { return len >= 15u ? 1u + (len - 15u) / 255u : 0u; }
__device__ __forceinline__ uint32_t lz_hash(uint32_t v) { return (v * 2654435761u) >> 20; }
static_assert(LZ_TAB == 1u << 12, "lz_hash keeps 12 bits");
inline size_t lz_bound(size_t n) { return n + n / 255 + 16; }

struct LzMatch { uint32_t len, back, dist; };   // len forward from the lane's position, `back` bytes before it also match
// candidate word c for word p (c < p), whose word is v; a match ends at or before byte `limit`
__device__ __forceinline__ void lz_try(const uint32_t* __restrict__ w, const uint8_t* __restrict__ b, uint32_t p, uint32_t c, uint32_t v,
                                       uint32_t limit, LzMatch* best) {
  const uint32_t pb = p * 4u, cb = c * 4u, dist = pb - cb;
  if (dist > 65535u || w[c] != v) return;
  uint32_t len = 4u;
  for (uint32_t q = 1u; pb + 4u * q < limit; ++q) {
    const uint32_t x = w[p + q] ^ w[c + q];
    if (x) {
      len += (uint32_t)(__ffs(x) - 1) >> 3;
      break;
    }
    len += 4u;
  }
  len = min(len, limit - pb);
  uint32_t back = 0u;
  while (back < 3u && cb > back && b[pb - 1u - back] == b[cb - 1u - back]) ++back;
  if (len + back > best->len + best->back) *best = LzMatch{len, back, dist};
}

__global__ void __launch_bounds__(64) k_lz4_find(const uint32_t* __restrict__ w, uint32_t n, uint2* __restrict__ seqs,
                                                 uint4* __restrict__ meta) {
  __shared__ uint32_t tab[LZ_TAB];   // word position + 1; 0: empty
  const uint32_t lane = threadIdx.x, seg = blockIdx.x;
  const uint8_t* b = reinterpret_cast<const uint8_t*>(w);
  const uint32_t seg_beg = seg * LZ_SEG, seg_end = min(seg_beg + LZ_SEG, n);
  const uint32_t limit = min(seg_end, n >= 5u ? n - 5u : 0u);   // where a match of this segment ends at the latest
  for (uint32_t i = lane; i < LZ_TAB; i += 64u) tab[i] = 0u;
  __syncthreads();
  const uint32_t first_word = seg_beg / 4u;
  for (uint32_t q = (first_word > LZ_LOOKBACK ? first_word - LZ_LOOKBACK : 0u) + lane; q < first_word; q += 64u)
    atomicMax(&tab[lz_hash(w[q])], q + 1u);
  __syncthreads();
  uint2* out = seqs + (size_t)seg * LZ_MAX_SEQ;
  uint32_t cur = seg_beg;   // the first byte no sequence covers yet
  uint32_t nseq = 0u, size = 0u, first_lit = 0u;
  for (uint32_t step = first_word; step * 4u < seg_end; step += 64u) {
    if (cur >= (step + 64u) * 4u) continue;   // the whole step lies inside a match
    const uint32_t p = step + lane, pb = p * 4u;
    const bool whole = pb + 4u <= seg_end;                            // a whole word of the segment (and of the input)
    const bool start = whole && pb + 12u <= n && pb + 4u <= limit;    // a match may start here
    const uint32_t v = whole ? w[p] : 0u;
    const uint32_t h = lz_hash(v);
    const uint32_t cand = tab[h];
    __syncthreads();
    if (whole) atomicMax(&tab[h], p + 1u);
    // inside the step: the nearest earlier lane that holds the same word (the table does not know this step's positions yet)
    const unsigned long long wholes = __ballot(whole);
    int near = -1;
#pragma unroll
    for (int k = 0; k < 63; ++k)
      if ((uint32_t)__shfl((int)v, k) == v && ((wholes >> k) & 1ull) && (uint32_t)k < lane) near = k;
    LzMatch best{0u, 0u, 0u};
    if (start) {
      if (near >= 0) lz_try(w, b, p, step + (uint32_t)near, v, limit, &best);
      if (cand) lz_try(w, b, p, cand - 1u, v, limit, &best);
      if (p >= 1u) lz_try(w, b, p, p - 1u, v, limit, &best);
      if (p >= 2u) lz_try(w, b, p, p - 2u, v, limit, &best);
    }
    const unsigned long long has = __ballot(best.len >= 4u);
    for (;;) {
      const uint32_t next_word = (cur + 3u) / 4u;
      const uint32_t lo = next_word > step ? next_word - step : 0u;
      if (lo >= 64u) break;
      const unsigned long long m = has & (~0ull << lo);
      if (!m || nseq >= LZ_MAX_SEQ) break;
      const int l = __ffsll((long long)m) - 1;
      const uint32_t mpos = (step + (uint32_t)l) * 4u;
      const uint32_t back = min((uint32_t)__shfl((int)best.back, l), mpos - cur);
      const uint32_t len = (uint32_t)__shfl((int)best.len, l) + back, dist = (uint32_t)__shfl((int)best.dist, l);
      const uint32_t mstart = mpos - back, lit = mstart - cur;
      if (lane == 0u) out[nseq] = make_uint2(mstart, len | (dist << 16));
      if (nseq == 0u) first_lit = lit;
      size += 1u + lz_ext(lit) + lit + 2u + lz_ext(len - 4u);
      ++nseq;
      cur = mstart + len;
    }
    __syncthreads();
  }
  if (lane == 0u) meta[seg] = make_uint4(nseq, nseq ? cur : 0u, size, first_lit);
}

// exclusive scans over the 256 threads of a block (s_w: 4 words); *total: the block's reduction
template <bool IS_MAX>
__device__ __forceinline__ uint32_t lz_block_scan(uint32_t v, uint32_t* s_w, uint32_t* total) {
  const uint32_t lane = threadIdx.x & 63u, wv = threadIdx.x >> 6;
  uint32_t inc = v;
#pragma unroll
  for (int o = 1; o < 64; o <<= 1) {
    const uint32_t u = (uint32_t)__shfl_up((int)inc, o);
    if (lane >= (uint32_t)o) inc = IS_MAX ? max(inc, u) : inc + u;
  }
  __syncthreads();   // (s_w of the previous call has been read)
  if (lane == 63u) s_w[wv] = inc;
  __syncthreads();
  uint32_t before = 0u, all = 0u;
#pragma unroll
  for (uint32_t k = 0; k < 4u; ++k) {
    if (k < wv) before = IS_MAX ? max(before, s_w[k]) : before + s_w[k];
    all = IS_MAX ? max(all, s_w[k]) : all + s_w[k];
  }
  *total = all;
  uint32_t exc = (uint32_t)__shfl_up((int)inc, 1);
  if (lane == 0u) exc = 0u;
  return IS_MAX ? max(before, exc) : before + exc;
}

__global__ void __launch_bounds__(256) k_lz4_place(const uint4* __restrict__ meta, uint32_t nseg, uint32_t n, uint2* __restrict__ segpos,
                                                   uint4* __restrict__ head) {
  __shared__ uint32_t s_w[4];
  uint32_t anchor_run = 0u, pos_run = 0u;   // the end of the last match and the bytes written, before this tile
  for (uint32_t base = 0u; base < nseg; base += 256u) {
    const uint32_t k = base + threadIdx.x;
    const uint4 m = k < nseg ? meta[k] : make_uint4(0u, 0u, 0u, 0u);
    uint32_t tile_anchor, tile_size;
    const uint32_t anchor = max(anchor_run, lz_block_scan<true>(m.y, s_w, &tile_anchor));
    uint32_t size = 0u;
    if (m.x) {
      const uint32_t carry = k * LZ_SEG - anchor;
      size = m.z + carry + lz_ext(m.w + carry) - lz_ext(m.w);
    }
    const uint32_t at = lz_block_scan<false>(size, s_w, &tile_size);
    if (k < nseg) segpos[k] = make_uint2(pos_run + at, anchor);
    anchor_run = max(anchor_run, tile_anchor);
    pos_run += tile_size;
  }
  if (threadIdx.x == 0u) {
    const uint32_t lit = n - anchor_run;
    *head = make_uint4(pos_run + 1u + lz_ext(lit) + lit, anchor_run, pos_run, 0u);
  }
}

// the bytes behind a token's nibble 15: 255 .. 255, (len - 15) % 255
__device__ __forceinline__ void lz_put_ext(uint8_t* __restrict__ dst, uint32_t len) {
  if (len < 15u) return;
  uint32_t left = len - 15u;
  for (; left >= 255u; left -= 255u) *dst++ = 255u;
  *dst = (uint8_t)left;
}

__global__ void __launch_bounds__(64) k_lz4_emit(const uint8_t* __restrict__ src, const uint2* __restrict__ seqs,
                                                 const uint4* __restrict__ meta, const uint2* __restrict__ segpos, uint8_t* __restrict__ dst) {
  const uint32_t lane = threadIdx.x, seg = blockIdx.x;
  const uint32_t nseq = meta[seg].x;
  if (nseq == 0u) return;
  const uint2* in = seqs + (size_t)seg * LZ_MAX_SEQ;
  const uint2 sp = segpos[seg];
  uint32_t pos = sp.x;
  for (uint32_t base = 0u; base < nseq; base += 64u) {
    const uint32_t i = base + lane;
    const bool valid = i < nseq;
    uint32_t lit_from = 0u, lit = 0u, mlen = 4u, dist = 0u, size = 0u;
    if (valid) {
      const uint2 sq = in[i];
      mlen = sq.y & 0xFFFFu;
      dist = sq.y >> 16;
      if (i == 0u) {
        lit_from = sp.y;
      } else {
        const uint2 pv = in[i - 1u];
        lit_from = pv.x + (pv.y & 0xFFFFu);
      }
      lit = sq.x - lit_from;
      size = 1u + lz_ext(lit) + lit + 2u + lz_ext(mlen - 4u);
    }
    uint32_t inc = size;
#pragma unroll
    for (int o = 1; o < 64; o <<= 1) {
      const uint32_t u = (uint32_t)__shfl_up((int)inc, o);
      if (lane >= (uint32_t)o) inc += u;
    }
    const uint32_t total = (uint32_t)__shfl((int)inc, 63);
    uint8_t* o = dst + pos + (inc - size);
    uint8_t* lit_to = o + 1u + lz_ext(lit);
    if (valid) {
      *o = (uint8_t)((min(lit, 15u) << 4) | min(mlen - 4u, 15u));
      lz_put_ext(o + 1u, lit);
      if (lit <= LZ_LONG_LIT)
        for (uint32_t j = 0u; j < lit; ++j) lit_to[j] = src[lit_from + j];
      uint8_t* q = lit_to + lit;
      q[0] = (uint8_t)(dist & 0xFFu);
      q[1] = (uint8_t)(dist >> 8);
      lz_put_ext(q + 2u, mlen - 4u);
    }
    for (unsigned long long lg = __ballot(valid && lit > LZ_LONG_LIT); lg; lg &= lg - 1ull) {
      const int l = __ffsll((long long)lg) - 1;
      const uint32_t from = (uint32_t)__shfl((int)lit_from, l), cnt = (uint32_t)__shfl((int)lit, l);
      const unsigned long long to = __shfl((unsigned long long)(uintptr_t)lit_to, l);
      uint8_t* t = reinterpret_cast<uint8_t*>((uintptr_t)to);
      for (uint32_t j = lane; j < cnt; j += 64u) t[j] = src[from + j];
    }
    pos += total;
  }
}

__global__ void __launch_bounds__(256) k_lz4_last(const uint8_t* __restrict__ src, uint32_t n, const uint4* __restrict__ head,
                                                  uint8_t* __restrict__ dst) {
  const uint4 hd = *head;
  const uint32_t from = hd.y, lit = n - from, ext = lz_ext(lit);
  uint8_t* o = dst + hd.z;
  const uint32_t tid = blockIdx.x * 256u + threadIdx.x, stride = gridDim.x * 256u;
  if (tid == 0u) *o = (uint8_t)(min(lit, 15u) << 4);
  for (uint32_t j = tid; j < ext; j += stride) o[1u + j] = j + 1u < ext ? (uint8_t)255u : (uint8_t)((lit - 15u) % 255u);
  uint8_t* t = o + 1u + ext;
  for (uint32_t j = tid; j < lit; j += stride) t[j] = src[from + j];
}

__global__ void __launch_bounds__(256) k_crb_widen(const uint32_t* __restrict__ in, uint64_t* __restrict__ out, uint32_t count) {
  const uint32_t i = blockIdx.x * 256u + threadIdx.x;
  if (i < count) out[i] = in[i];
}

inline size_t lz_segments(size_t n) { return (n + LZ_SEG - 1) / LZ_SEG; }

// the four launches for one array: d_src [n] (readable up to the next multiple of 4) -> d_dst (lz_bound(n) bytes), sizes in head
int lz_encode(dfh_crb* e, const char* d_src, size_t n, char* d_dst, uint4* head) {
  const unsigned nseg = (unsigned)lz_segments(n);
  if (nseg)
    hipLaunchKernelGGL(k_lz4_find, dim3(nseg), dim3(64), 0, e->s, reinterpret_cast<const uint32_t*>(d_src), (uint32_t)n, e->d_seq, e->d_meta);
  hipLaunchKernelGGL(k_lz4_place, dim3(1), dim3(256), 0, e->s, e->d_meta, nseg, (uint32_t)n, e->d_segpos, head);
  if (nseg)
    hipLaunchKernelGGL(k_lz4_emit, dim3(nseg), dim3(64), 0, e->s, reinterpret_cast<const uint8_t*>(d_src), e->d_seq, e->d_meta, e->d_segpos,
                       reinterpret_cast<uint8_t*>(d_dst));
  hipLaunchKernelGGL(k_lz4_last, dim3(std::min<unsigned>(std::max<unsigned>(nseg, 1u), 1024u)), dim3(256), 0, e->s,
                     reinterpret_cast<const uint8_t*>(d_src), (uint32_t)n, head, reinterpret_cast<uint8_t*>(d_dst));
  DFH_HIP(hipGetLastError());
  return DFH_OK;
}

int lz_wait(dfh_crb* e) {
  DFH_HIP(hipEventRecord(e->ev, e->s));
  DFH_HIP(hipEventSynchronize(e->ev));
  return DFH_OK;
}

inline size_t lz_align16(size_t x) { return (x + 15) & ~static_cast<size_t>(15); }

// room for arrays of these sizes: the scratch of the longest, the input behind each other, the blocks behind each other
int lz_reserve(dfh_crb* e, const size_t* bytes, int count, size_t in_bytes) {
  size_t longest = 0, out_bytes = 0;
  for (int a = 0; a < count; ++a) {
    DFH_ARG(bytes[a] < LZ_MAX_INPUT, "an array of a row block has 2^31 - 2^25 bytes or more, which one LZ4 block does not hold: lower chunk_size");
    longest = std::max(longest, bytes[a]);
    out_bytes += lz_align16(lz_bound(bytes[a]));
  }
  const size_t nseg = std::max<size_t>(lz_segments(longest), 1);
  int rc = tp_reserve(&e->d_in, &e->cap_in, std::max<size_t>(in_bytes, 16));
  if (!rc) rc = tp_reserve(&e->d_out, &e->cap_out, out_bytes);
  if (!rc) rc = tp_reserve(&e->d_seq, &e->cap_seq, nseg * LZ_MAX_SEQ);
  if (!rc) rc = tp_reserve(&e->d_meta, &e->cap_meta, nseg);
  if (!rc) rc = tp_reserve(&e->d_segpos, &e->cap_segpos, nseg);
  return rc;
}

// the five arrays of a row block, already in HBM (src[a] = NULL or bytes[a] = 0: absent) -> blocks and sizes
int crb_encode_device(dfh_crb* e, size_t nrows, const char* const* src, const size_t* bytes) {
  size_t at = 0;
  for (int a = 0; a < 5; ++a) {
    e->out_at[a] = at;
    e->out_size[a] = 0;
    if (!src[a] || bytes[a] == 0) continue;
    at += lz_align16(lz_bound(bytes[a]));
    const int rc = lz_encode(e, src[a], bytes[a], e->d_out + e->out_at[a], e->d_head + a);
    if (rc) return rc;
  }
  DFH_HIP(hipMemcpyAsync(e->h_head, e->d_head, 5 * sizeof(uint4), hipMemcpyDeviceToHost, e->s));
  const int rc = lz_wait(e);
  if (rc) return rc;
  size_t total = 3 * sizeof(int32_t) + 5 * sizeof(int32_t);
  for (int a = 0; a < 5; ++a) {
    if (!src[a] || bytes[a] == 0) continue;
    e->out_size[a] = e->h_head[4 * a];
    total += e->out_size[a];
  }
  e->nrows = (int)nrows;
  e->record_bytes = total;
  e->valid = true;
  return DFH_OK;
}
}  // namespace

extern "C" {

int dfh_crb_destroy(dfh_crb* e) {
  if (!e) return DFH_OK;
  hipSetDevice(e->ctx->device);
  if (e->s) hipStreamSynchronize(e->s);
  if (e->ev) hipEventDestroy(e->ev);
  for (void* p : {(void*)e->d_in, (void*)e->d_out, (void*)e->d_seq, (void*)e->d_meta, (void*)e->d_segpos, (void*)e->d_head,
                  (void*)e->d_gather})
    if (p) hipFree(p);
  if (e->h_head) hipHostFree(e->h_head);
  if (e->s) hipStreamDestroy(e->s);
  delete e;
  return DFH_OK;
}

int dfh_crb_create(dfh_ctx* c, dfh_crb** out) {
  DFH_ARG(c && out, "dfh_crb_create: NULL argument");
  DFH_HIP(hipSetDevice(c->device));
  dfh_crb* e = new (std::nothrow) dfh_crb();
  if (!e) {
    set_error("dfh_crb_create: out of host memory");
    return DFH_ERR_HIP;
  }
  e->ctx = c;
  hipError_t err;
  if ((err = hipStreamCreateWithFlags(&e->s, hipStreamNonBlocking)) != hipSuccess ||
      (err = hipEventCreateWithFlags(&e->ev, hipEventDisableTiming)) != hipSuccess ||
      (err = hipMalloc(reinterpret_cast<void**>(&e->d_head), 5 * sizeof(uint4))) != hipSuccess ||
      (err = hipHostMalloc(reinterpret_cast<void**>(&e->h_head), 5 * sizeof(uint4), hipHostMallocDefault)) != hipSuccess) {
    set_error(std::string("dfh_crb_create: ") + hipGetErrorString(err));
    dfh_crb_destroy(e);
    return DFH_ERR_HIP;
  }
  *out = e;
  return DFH_OK;
}

int dfh_crb_encode_host(dfh_crb* e, size_t nrows, const size_t* offset, const float* label, const uint64_t* index, const float* value,
                        const float* weight, size_t* record_bytes) {
  DFH_ARG(e && offset && label && record_bytes, "dfh_crb_encode_host: NULL argument (offset and label are required)");
  DFH_ARG(nrows < (1ULL << 31) && offset[nrows] >= offset[0], "dfh_crb_encode_host: a record holds fewer than 2^31 rows; offsets do not decrease");
  e->valid = false;
  const size_t nnz = offset[nrows] - offset[0];
  DFH_ARG(index || nnz == 0, "dfh_crb_encode_host: ids are required for a block that has nonzeros");
  if (value) {   // all ones: the field is dropped (compressed_row_block.h:31-39)
    bool binary = true;
    for (size_t i = 0; i < nnz && binary; ++i) binary = value[i] == 1.0f;
    if (binary) value = nullptr;
  }
  DFH_HIP(hipSetDevice(e->ctx->device));
  // index and value are the block's own: they start at offset[0] of the caller's arrays' view (RowBlock: index + offset[0])
  const char* host[5] = {reinterpret_cast<const char*>(label), reinterpret_cast<const char*>(offset), reinterpret_cast<const char*>(index),
                         reinterpret_cast<const char*>(value), reinterpret_cast<const char*>(weight)};
  const size_t bytes[5] = {nrows * sizeof(float), (nrows + 1) * sizeof(uint64_t), index ? nnz * sizeof(uint64_t) : 0,
                           value ? nnz * sizeof(float) : 0, weight ? nrows * sizeof(float) : 0};
  static_assert(sizeof(size_t) == sizeof(uint64_t), "offsets are written as 64-bit words");
  size_t in_bytes = 0;
  for (int a = 0; a < 5; ++a) in_bytes += lz_align16(bytes[a]);
  int rc = lz_reserve(e, bytes, 5, in_bytes);
  if (rc) return rc;
  const char* dev[5];
  size_t at = 0;
  for (int a = 0; a < 5; ++a) {
    dev[a] = nullptr;
    if (!host[a] || bytes[a] == 0) continue;
    dev[a] = e->d_in + at;
    DFH_HIP(hipMemcpyAsync(e->d_in + at, host[a], bytes[a], hipMemcpyHostToDevice, e->s));
    at += lz_align16(bytes[a]);
  }
  rc = crb_encode_device(e, nrows, dev, bytes);
  if (rc) return rc;
  *record_bytes = e->record_bytes;
  return DFH_OK;
}

int dfh_crb_encode_textchunk(dfh_crb* e, dfh_textchunk* tc, size_t* record_bytes) {
  DFH_ARG(e && tc && record_bytes, "dfh_crb_encode_textchunk: NULL argument");
  DFH_ARG(tc->valid && tc->ctx == e->ctx, "dfh_crb_encode_textchunk: no regular chunk parsed / a chunk of another context");
  e->valid = false;
  DFH_HIP(hipSetDevice(e->ctx->device));
  const size_t nrows = tc->nrows, nnz = tc->nnz;
  const size_t bytes[5] = {nrows * sizeof(float), (nrows + 1) * sizeof(uint64_t), nnz * sizeof(uint64_t), 0, 0};
  int rc = lz_reserve(e, bytes, 5, lz_align16(bytes[1]));
  if (rc) return rc;
  // (the parse call has waited for its own work: the chunk's arrays are complete)
  hipLaunchKernelGGL(k_crb_widen, dim3((unsigned)((nrows + 1 + 255) / 256)), dim3(256), 0, e->s, tc->d_off, reinterpret_cast<uint64_t*>(e->d_in),
                     (uint32_t)(nrows + 1));
  DFH_HIP(hipGetLastError());
  const char* dev[5] = {reinterpret_cast<const char*>(tc->d_lab), e->d_in, reinterpret_cast<const char*>(tc->d_ids), nullptr, nullptr};
  rc = crb_encode_device(e, nrows, dev, bytes);
  if (rc) return rc;
  *record_bytes = e->record_bytes;
  return DFH_OK;
}

int dfh_crb_record(dfh_crb* e, void* dst) {
  DFH_ARG(e && e->valid && dst, "dfh_crb_record: nothing encoded / NULL argument");
  DFH_HIP(hipSetDevice(e->ctx->device));
  char* p = static_cast<char*>(dst);
  const int32_t head[3] = {1196140743, 8, (int32_t)e->nrows};
  memcpy(p, head, sizeof(head));
  p += sizeof(head);
  for (int a = 0; a < 5; ++a) {
    const int32_t size = (int32_t)e->out_size[a];
    memcpy(p, &size, sizeof(size));
    p += sizeof(size);
    if (size) DFH_HIP(hipMemcpyAsync(p, e->d_out + e->out_at[a], (size_t)size, hipMemcpyDeviceToHost, e->s));
    p += size;
  }
  return lz_wait(e);
}

int dfh_lz4_compress(dfh_ctx* c, const void* src, size_t n, void* dst, size_t cap, size_t* out_bytes) {
  DFH_ARG(c && dst && out_bytes && (src || n == 0), "dfh_lz4_compress: NULL argument");
  DFH_ARG(n < LZ_MAX_INPUT, "dfh_lz4_compress: 2^31 - 2^25 bytes or more do not go into one LZ4 block: lower chunk_size");
  dfh_crb* e = nullptr;
  int rc = dfh_crb_create(c, &e);
  if (rc) return rc;
  rc = lz_reserve(e, &n, 1, lz_align16(n));
  if (!rc && n && hipMemcpyAsync(e->d_in, src, n, hipMemcpyHostToDevice, e->s) != hipSuccess) {
    set_error("dfh_lz4_compress: the upload failed");
    rc = DFH_ERR_HIP;
  }
  if (!rc) rc = lz_encode(e, e->d_in, n, e->d_out, e->d_head);
  if (!rc && hipMemcpyAsync(e->h_head, e->d_head, sizeof(uint4), hipMemcpyDeviceToHost, e->s) != hipSuccess) {
    set_error("dfh_lz4_compress: the read-back of the size failed");
    rc = DFH_ERR_HIP;
  }
  if (!rc) rc = lz_wait(e);
  if (!rc) {
    *out_bytes = e->h_head[0];
    if (*out_bytes > cap) {
      set_error("dfh_lz4_compress: the block has " + std::to_string(*out_bytes) + " bytes, dst holds " + std::to_string(cap));
      rc = DFH_ERR_ARG;
    } else if (hipMemcpy(dst, e->d_out, *out_bytes, hipMemcpyDeviceToHost) != hipSuccess) {
      set_error("dfh_lz4_compress: the read-back of the block failed");
      rc = DFH_ERR_HIP;
    }
  }
  dfh_crb_destroy(e);
  return rc;
}

}  // extern "C"
