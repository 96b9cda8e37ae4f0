// dfh_lz4dec.hip — the device LZ4 block decoder and the CompressedRowBlock reader of rec_decode = device (included in dfh_api.hip
// behind dfh_lz4enc.hip; the block format is described at the top of host/lz4_block.h, whose verdict this decoder repeats bit for
// bit).  Up to five blocks (the arrays of one record) are decoded together; a chunk object (dfh_textchunk) ends in the state
// dfh_textchunk_parse_criteo leaves a regular chunk in.
//
// A block is a chain: sequence k + 1 starts where sequence k ends, and a match reads what earlier sequences wrote.  Both are
// resolved without any workgroup waiting for another one; the stream orders the launches, and the only words blocks share are
// the status word they OR findings into and the round flags of the pointer jumping:
//   k_lzd_ff      per tile of 4 096 compressed bytes: the first byte that is not 0xFF (length extensions are runs of 0xFF)
//   k_lzd_ffnext  a wave per block: suffix minimum of those, so that a run of 0xFF is skipped tile-wise
//   k_lzd_links   per tile: EVERY byte position is read as if a token stood there: where the sequence ends, its literal and match
//                 lengths, every read bounded by the block's end (a position whose fields run past it is BAD).  The pointers are
//                 then doubled in LDS — (last position inside the tile, sequences passed, output bytes), one 64-bit word per
//                 position, updated in place — until none moves, and (exit position, output bytes up to there) is stored per
//                 position.
//   k_lzd_chain   a wave per block walks tile by tile from position 0: entry[t + 1] = exit(entry[t]); a literal run may skip whole
//                 tiles, which then have no entry.  Per tile: entry and first output byte.  Per block: ok (the chain meets no BAD
//                 position and ends exactly at the block's end in a sequence of literals only) and the output size.
//   -- the host reads the five {ok, size} and compares them with what the caller (the record's header) expects --
//   k_lzd_list    per tile that has an entry: the tile's sequences from its entry, in LDS; literals are copied to their output
//                 positions, and every output byte gets a POINTER: a literal byte to itself, a match byte to the byte `offset`
//                 before it (1 <= offset <= output position is checked here; a match that overlaps its own output is simply a
//                 chain of such pointers).
//   k_lzd_jump    pointer jumping over the output bytes, ptr[i] = ptr[ptr[i]], in place.  After round r a pointer has gone
//                 2^r steps or reached a literal, so ceil(log2(size)) launches are enqueued; a round in which nothing moved
//                 leaves the next round's flag 0 and the remaining launches return at once.  The matches therefore cost
//                 O(log depth) passes over the output by the whole chip instead of a serial walk in output order.
//   k_lzd_gather  every match byte is read from the literal its pointer names.
// A stale pointer read in k_lzd_jump is an earlier value of that pointer, which is another valid ancestor: the result does not
// depend on the order of the blocks, and the values read at the start of a round are at least those of the round before (kernel
// boundary), which is what the doubling bound needs.  Plain C++, vector loads and stores only.
struct dfh_lzd {
  uint8_t* d_comp = nullptr;                         // the compressed blocks, each from a tile boundary
  uint32_t *d_exit = nullptr, *d_outv = nullptr;     // per compressed position
  uint32_t *d_tnext = nullptr, *d_tentry = nullptr, *d_tout = nullptr;   // per tile
  uint32_t* d_ptr = nullptr;                         // per output byte
  uint8_t* d_dst = nullptr;                          // outputs that do not live in the chunk's own arrays
  uint32_t* d_head = nullptr;                        // [64]: five {ok, size} pairs, [10] status, [16 ..] round flags
  uint32_t* h_head = nullptr;                        // page-locked copy
  size_t cap_comp = 0, cap_exit = 0, cap_outv = 0, cap_tnext = 0, cap_tentry = 0, cap_tout = 0, cap_ptr = 0, cap_dst = 0;
};

namespace {
constexpr uint32_t LZD_TILE = 4096, LZD_BAD = 0xFFFFFFFFu, LZD_NONE = 0xFFFFFFFFu;
constexpr uint32_t LZD_SHORT = 32;       // longer literal runs and matches are written by the whole workgroup
constexpr uint32_t LZD_MAXSEQ = 2048;    // a sequence that is followed by another has at least 3 bytes: 1 366 per tile
constexpr uint32_t LZD_ST_OFFSET = 1u, LZD_ST_ROWS = 2u;
constexpr size_t LZD_MAX_POINTERS = (1ULL << 32) - 4096;   // pointer positions and grid sizes are 32-bit
constexpr uint32_t LZD_HEAD_WORDS = 64, LZD_STATUS = 10, LZD_ROUND0 = 16, LZD_MAX_ROUNDS = 32;

struct LzdJob {
  const uint8_t* src[5];
  uint8_t* dst[5];
  uint32_t n[5], expect[5];   // n = 0: the array is absent
  uint32_t tile0[6];          // the first tile of each block
  uint32_t obase[6];          // the first pointer of each block's output
};

__device__ __forceinline__ int lzd_array_of(const uint32_t* bounds, uint32_t x) {
  int a = 0;
#pragma unroll
  for (int k = 1; k < 5; ++k) a += x >= bounds[k] ? 1 : 0;
  return a;
}

// a length extension at q: acc += the run's bytes, q behind its last byte; false = the run reaches the block's end
__device__ __forceinline__ bool lzd_ext(const uint8_t* __restrict__ src, uint32_t n, const uint32_t* __restrict__ tnext, uint32_t& q,
                                        uint64_t& acc) {
  if (q >= n) return false;
  const uint32_t tend = min((q | (LZD_TILE - 1u)) + 1u, n);
  uint32_t e = q;
  while (e < tend && src[e] == 255u) ++e;
  if (e == tend && e < n) e = tnext[e / LZD_TILE];   // the first byte that is not 0xFF from that tile on; n: none
  if (e >= n) return false;
  acc += 255ull * (e - q) + src[e];
  q = e + 1u;
  return true;
}

struct LzdSeq { uint32_t next, lit, ml, litsrc, off; };   // next = LZD_BAD: no sequence; ml = 0: literals only, the block's last
__device__ __forceinline__ LzdSeq lzd_parse(const uint8_t* __restrict__ src, uint32_t n, const uint32_t* __restrict__ tnext, uint32_t p) {
  LzdSeq s{LZD_BAD, 0u, 0u, 0u, 0u};
  const uint32_t tok = src[p];
  uint32_t q = p + 1u;
  uint64_t lit = tok >> 4;
  if (lit == 15u && !lzd_ext(src, n, tnext, q, lit)) return s;
  if (lit > (uint64_t)(n - q)) return s;
  s.litsrc = q;
  s.lit = (uint32_t)lit;
  q += (uint32_t)lit;
  if (q == n) {
    s.next = n;
    return s;
  }
  if (n - q < 2u) return s;
  s.off = (uint32_t)src[q] | ((uint32_t)src[q + 1u] << 8);
  q += 2u;
  uint64_t ml = tok & 15u;
  if (ml == 15u && !lzd_ext(src, n, tnext, q, ml)) return s;
  ml += 4u;
  if (q >= n || lit + ml > 0x7FFFFFFFull) return s;   // a match is never the last thing in a block; sizes stay below 2^31
  s.ml = (uint32_t)ml;
  s.next = q;
  return s;
}

// the tile's positions from `from` on (tile-relative), read as tokens: where each ends and how many bytes it gives
__device__ __forceinline__ void lzd_fill(const uint8_t* __restrict__ src, uint32_t n, const uint32_t* __restrict__ tnext, uint32_t start,
                                         uint32_t from, uint32_t* s_next, uint32_t* s_out) {
  for (uint32_t i = threadIdx.x; i < LZD_TILE; i += 256u) {
    const uint32_t p = start + i;
    uint32_t nx = LZD_BAD, o = 0u;
    if (p < n && i >= from) {
      const LzdSeq q = lzd_parse(src, n, tnext, p);
      nx = q.next;
      o = nx == LZD_BAD ? 0u : q.lit + q.ml;
    }
    s_next[i] = nx;
    s_out[i] = o;
  }
}

__global__ void __launch_bounds__(256) k_lzd_ff(LzdJob job, uint32_t* __restrict__ tfirst) {
  __shared__ uint32_t s_min[4];
  const int a = lzd_array_of(job.tile0, blockIdx.x);
  const uint8_t* __restrict__ src = job.src[a];
  const uint32_t n = job.n[a], at = (blockIdx.x - job.tile0[a]) * LZD_TILE + threadIdx.x * 16u;
  uint32_t first = LZD_NONE;
  if (at < n) {
    const uint4 v = *reinterpret_cast<const uint4*>(src + at);   // (tiles are whole inside the allocation)
    const uint32_t w[4] = {v.x, v.y, v.z, v.w};
#pragma unroll
    for (int k = 3; k >= 0; --k)
      if (w[k] != 0xFFFFFFFFu) first = at + 4u * k + ((uint32_t)(__ffs(~w[k]) - 1) >> 3);
    if (first >= n) first = LZD_NONE;
  }
#pragma unroll
  for (int o = 32; o > 0; o >>= 1) first = min(first, (uint32_t)__shfl_xor(first, o));
  if ((threadIdx.x & 63u) == 0) s_min[threadIdx.x >> 6] = first;
  __syncthreads();
  if (threadIdx.x == 0) tfirst[blockIdx.x] = min(min(s_min[0], s_min[1]), min(s_min[2], s_min[3]));
}

// in place: tnext[t] = the first byte that is not 0xFF at or behind the start of tile t (n: none)
__global__ void __launch_bounds__(64) k_lzd_ffnext(LzdJob job, uint32_t* __restrict__ tnext) {
  const int a = blockIdx.x;
  const uint32_t nt = job.tile0[a + 1] - job.tile0[a], lane = threadIdx.x;
  uint32_t* t = tnext + job.tile0[a];
  uint32_t carry = job.n[a];
  for (uint32_t base = (nt + 63u) / 64u * 64u; base > 0u; base -= 64u) {
    const uint32_t i = base - 64u + lane;
    uint32_t v = i < nt ? t[i] : LZD_NONE;
#pragma unroll
    for (int o = 1; o < 64; o <<= 1) {
      const uint32_t u = __shfl_down(v, o);
      if (lane + o < 64u) v = min(v, u);
    }
    v = min(v, carry);
    if (i < nt) t[i] = v;
    carry = __shfl(v, 0);
  }
}

__global__ void __launch_bounds__(256) k_lzd_links(LzdJob job, const uint32_t* __restrict__ tnext, uint32_t* __restrict__ exitp,
                                                   uint32_t* __restrict__ outv) {
  __shared__ uint32_t s_next[LZD_TILE], s_out[LZD_TILE];
  __shared__ unsigned long long s_link[LZD_TILE];   // last position in the tile [0, 12) | sequences passed [12, 24) | bytes [24, 64)
  const int a = lzd_array_of(job.tile0, blockIdx.x);
  const uint32_t n = job.n[a], start = (blockIdx.x - job.tile0[a]) * LZD_TILE, end = start + LZD_TILE;
  lzd_fill(job.src[a], n, tnext + job.tile0[a], start, 0u, s_next, s_out);
  for (uint32_t i = threadIdx.x; i < LZD_TILE; i += 256u) {
    const uint32_t nx = s_next[i];
    s_link[i] = nx == LZD_BAD || nx >= end || nx >= n ? (unsigned long long)i
                                                      : (unsigned long long)(nx - start) | (1ull << 12) | ((unsigned long long)s_out[i] << 24);
  }
  __syncthreads();
  // in place: a word read while others are rewritten is an earlier, equally valid composition (64-bit LDS accesses are whole)
  int moved;
  do {
    moved = 0;
    for (uint32_t i = threadIdx.x; i < LZD_TILE; i += 256u) {
      const unsigned long long li = __hip_atomic_load(&s_link[i], __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_WORKGROUP);
      const uint32_t j = (uint32_t)li & 4095u;
      if (j == i) continue;
      const unsigned long long lj = __hip_atomic_load(&s_link[j], __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_WORKGROUP);
      if (((uint32_t)lj & 4095u) == j) continue;
      __hip_atomic_store(&s_link[i], (lj & 4095ull) + (li & ~4095ull) + (lj & ~4095ull), __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_WORKGROUP);
      moved = 1;
    }
  } while (__syncthreads_or(moved));
  const size_t g = (size_t)blockIdx.x * LZD_TILE;
  for (uint32_t i = threadIdx.x; i < LZD_TILE; i += 256u) {
    const unsigned long long li = s_link[i];
    const uint32_t j = (uint32_t)li & 4095u;
    exitp[g + i] = s_next[j];
    outv[g + i] = (uint32_t)(li >> 24) + s_out[j];   // (below 2^21 + 2^31)
  }
}

__global__ void __launch_bounds__(64) k_lzd_chain(LzdJob job, const uint32_t* __restrict__ exitp, const uint32_t* __restrict__ outv,
                                                  uint32_t* __restrict__ tentry, uint32_t* __restrict__ tout, uint32_t* __restrict__ head) {
  if (threadIdx.x != 0) return;
  const int a = blockIdx.x;
  const uint32_t n = job.n[a];
  uint32_t ok = 0u, pos = 0u;
  unsigned long long out = 0ull;
  if (n) {
    const size_t g = (size_t)job.tile0[a] * LZD_TILE;
    for (;;) {   // exit(pos) lies beyond pos's tile: at most one step per tile
      const uint32_t t = job.tile0[a] + pos / LZD_TILE;
      tentry[t] = pos;
      tout[t] = (uint32_t)out;
      const uint32_t e = exitp[g + pos];
      if (e == LZD_BAD) break;
      out += outv[g + pos];
      if (out > 0x7FFFFFFFull) break;
      if (e >= n) {
        ok = 1u;
        break;
      }
      pos = e;
    }
  }
  head[2 * a] = ok;
  head[2 * a + 1] = ok ? (uint32_t)out : 0u;
}

__global__ void __launch_bounds__(256) k_lzd_list(LzdJob job, const uint32_t* __restrict__ tnext, const uint32_t* __restrict__ tentry,
                                                  const uint32_t* __restrict__ tout, uint32_t* __restrict__ ptr, uint32_t* __restrict__ head) {
  __shared__ uint32_t s_next[LZD_TILE], s_out[LZD_TILE], s_o[LZD_MAXSEQ];
  __shared__ uint16_t s_pos[LZD_MAXSEQ], s_long[LZD_MAXSEQ];
  __shared__ uint32_t s_count, s_nlong;
  const uint32_t entry = tentry[blockIdx.x];
  if (entry == LZD_NONE) return;
  const int a = lzd_array_of(job.tile0, blockIdx.x);
  const uint8_t* __restrict__ src = job.src[a];
  uint8_t* __restrict__ dst = job.dst[a];
  uint32_t* __restrict__ p_out = ptr + job.obase[a];
  const uint32_t* __restrict__ tn = tnext + job.tile0[a];
  const uint32_t n = job.n[a], expect = job.expect[a], start = (blockIdx.x - job.tile0[a]) * LZD_TILE, end = start + LZD_TILE;
  lzd_fill(src, n, tn, start, entry - start, s_next, s_out);
  if (threadIdx.x == 0) s_nlong = 0u;
  __syncthreads();
  if (threadIdx.x == 0) {
    uint32_t k = 0u, p = entry, o = tout[blockIdx.x];
    while (p < end && p < n && k < LZD_MAXSEQ) {
      const uint32_t nx = s_next[p - start];
      if (nx == LZD_BAD) break;   // (the chain kernel has refused such a block: nothing is launched for it)
      s_pos[k] = (uint16_t)(p - start);
      s_o[k] = o;
      o += s_out[p - start];
      p = nx;
      ++k;
    }
    s_count = k;
  }
  __syncthreads();
  const uint32_t count = s_count;
  bool bad = false;
  for (uint32_t k = threadIdx.x; k < count; k += 256u) {
    const LzdSeq q = lzd_parse(src, n, tn, start + s_pos[k]);
    const uint32_t o = s_o[k], m = o + q.lit;
    if ((unsigned long long)m + q.ml > expect) continue;   // (sizes were compared before this launch: never taken)
    const bool bad_off = q.ml != 0u && (q.off == 0u || q.off > m);
    bad |= bad_off;
    if (q.lit > LZD_SHORT || q.ml > LZD_SHORT) s_long[atomicAdd(&s_nlong, 1u)] = (uint16_t)k;
    if (q.lit <= LZD_SHORT)
      for (uint32_t i = 0; i < q.lit; ++i) {
        dst[o + i] = src[q.litsrc + i];
        p_out[o + i] = o + i;
      }
    if (q.ml <= LZD_SHORT)
      for (uint32_t i = 0; i < q.ml; ++i) p_out[m + i] = bad_off ? m + i : m + i - q.off;
  }
  if (__ballot(bad) && (threadIdx.x & 63u) == 0) atomicOr(head + LZD_STATUS, LZD_ST_OFFSET);
  __syncthreads();
  const uint32_t nlong = s_nlong;
  for (uint32_t l = 0; l < nlong; ++l) {
    const uint32_t k = s_long[l];
    const LzdSeq q = lzd_parse(src, n, tn, start + s_pos[k]);
    const uint32_t o = s_o[k], m = o + q.lit;
    const bool bad_off = q.off == 0u || q.off > m;
    if (q.lit > LZD_SHORT)
      for (uint32_t i = threadIdx.x; i < q.lit; i += 256u) {
        dst[o + i] = src[q.litsrc + i];
        p_out[o + i] = o + i;
      }
    if (q.ml > LZD_SHORT)
      for (uint32_t i = threadIdx.x; i < q.ml; i += 256u) p_out[m + i] = bad_off ? m + i : m + i - q.off;
  }
}

// element x of the pointer array -> its block and the position inside it; false: padding between the blocks
__device__ __forceinline__ bool lzd_locate(const LzdJob& job, uint32_t x, int* a, uint32_t* i) {
  *a = lzd_array_of(job.obase, x);
  *i = x - job.obase[*a];
  return *i < job.expect[*a];
}

// four consecutive pointers per lane (one 16-byte load; the outputs start at multiples of 16 pointers).  Plain loads and stores:
// a value that another block is just replacing is read old or new, and both name a byte this one is a copy of
__global__ void __launch_bounds__(256) k_lzd_jump(LzdJob job, uint32_t* ptr, uint32_t* round, int first) {
  if (!first && round[0] == 0u) return;   // the round before moved nothing: every pointer names a literal
  const uint32_t x = (blockIdx.x * 256u + threadIdx.x) * 4u;
  int a;
  uint32_t i;
  bool moved = false;
  if (x < job.obase[5] && lzd_locate(job, x, &a, &i)) {
    uint32_t* p = ptr + job.obase[a];
    const uint32_t expect = job.expect[a];
    const uint4 v = *reinterpret_cast<const uint4*>(p + i);   // (the array holds obase[5] pointers, a multiple of 16)
    const uint32_t q[4] = {v.x, v.y, v.z, v.w};
#pragma unroll
    for (uint32_t k = 0; k < 4u; ++k) {
      // (every pointer was written by k_lzd_list and lies below its own position; the bounds cost nothing)
      if (i + k >= expect || q[k] == i + k || q[k] >= expect) continue;
      const uint32_t qq = p[q[k]];
      if (qq != q[k] && qq < expect) {
        p[i + k] = qq;
        moved = true;
      }
    }
  }
  if (__ballot(moved) && (threadIdx.x & 63u) == 0) atomicOr(round + 1, 1u);
}

__global__ void __launch_bounds__(256) k_lzd_gather(LzdJob job, const uint32_t* __restrict__ ptr) {
  const uint32_t x = blockIdx.x * 256u + threadIdx.x;
  int a;
  uint32_t i;
  if (x >= job.obase[5] || !lzd_locate(job, x, &a, &i)) return;
  const uint32_t q = ptr[job.obase[a] + i];
  uint8_t* dst = job.dst[a];   // (read and written: literal bytes are read, match bytes written)
  if (q != i && q < job.expect[a]) dst[i] = dst[q];
}

// the offsets of a record as they were written (64 bits, from any first value) -> 32 bits from 0; what does not fit -> status
__global__ void __launch_bounds__(256) k_lzd_offsets(const uint64_t* __restrict__ raw, uint32_t nrows, uint32_t nnz, uint32_t* __restrict__ off,
                                                     uint32_t* __restrict__ head) {
  const uint32_t i = blockIdx.x * 256u + threadIdx.x;
  bool bad = false;
  if (i <= nrows) {
    const uint64_t first = raw[0], v = raw[i];
    bad = v < first || v - first > nnz || (i < nrows && raw[i + 1u] < v) || (i == nrows && v - first != nnz);
    off[i] = (uint32_t)(v - first);
  }
  if (__ballot(bad) && (threadIdx.x & 63u) == 0) atomicOr(head + LZD_STATUS, LZD_ST_ROWS);
}

void lzd_free(dfh_lzd* z) {
  if (!z) return;
  for (void* p : {(void*)z->d_comp, (void*)z->d_exit, (void*)z->d_outv, (void*)z->d_tnext, (void*)z->d_tentry, (void*)z->d_tout,
                  (void*)z->d_ptr, (void*)z->d_dst, (void*)z->d_head})
    if (p) hipFree(p);
  if (z->h_head) hipHostFree(z->h_head);
  delete z;
}

int lzd_get(dfh_textchunk* tc, dfh_lzd** out) {
  if (!tc->lzd) {
    dfh_lzd* z = new (std::nothrow) dfh_lzd();
    if (!z) {
      set_error("rec decode: out of host memory");
      return DFH_ERR_HIP;
    }
    hipError_t e;
    if ((e = hipMalloc(reinterpret_cast<void**>(&z->d_head), LZD_HEAD_WORDS * sizeof(uint32_t))) != hipSuccess ||
        (e = hipHostMalloc(reinterpret_cast<void**>(&z->h_head), LZD_HEAD_WORDS * sizeof(uint32_t), hipHostMallocDefault)) != hipSuccess) {
      set_error(std::string("rec decode: ") + hipGetErrorString(e));
      lzd_free(z);
      return DFH_ERR_HIP;
    }
    tc->lzd = z;
  }
  *out = tc->lzd;
  return DFH_OK;
}

inline uint32_t lzd_tiles(size_t n) { return (uint32_t)((n + LZD_TILE - 1) / LZD_TILE); }

// the blocks at host[a] (job->n[a] bytes; 0: absent) are uploaded and their chains walked; h_head holds {ok, size} of each
int lzd_chains(dfh_textchunk* tc, dfh_lzd* z, LzdJob* job, const void* const* host) {
  hipStream_t s = tc->s;
  job->tile0[0] = 0;
  for (int a = 0; a < 5; ++a) job->tile0[a + 1] = job->tile0[a] + lzd_tiles(job->n[a]);
  const size_t ntiles = job->tile0[5], bytes = ntiles * LZD_TILE;
  int rc = tp_reserve(&z->d_comp, &z->cap_comp, std::max<size_t>(bytes, 16));
  if (!rc) rc = tp_reserve(&z->d_exit, &z->cap_exit, std::max<size_t>(bytes, 16));
  if (!rc) rc = tp_reserve(&z->d_outv, &z->cap_outv, std::max<size_t>(bytes, 16));
  if (!rc) rc = tp_reserve(&z->d_tnext, &z->cap_tnext, ntiles + 1);
  if (!rc) rc = tp_reserve(&z->d_tentry, &z->cap_tentry, ntiles + 1);
  if (!rc) rc = tp_reserve(&z->d_tout, &z->cap_tout, ntiles + 1);
  if (rc) return rc;
  for (int a = 0; a < 5; ++a) {
    job->src[a] = z->d_comp + (size_t)job->tile0[a] * LZD_TILE;
    if (job->n[a]) DFH_HIP(hipMemcpyAsync(z->d_comp + (size_t)job->tile0[a] * LZD_TILE, host[a], job->n[a], hipMemcpyHostToDevice, s));
  }
  DFH_HIP(hipMemsetAsync(z->d_tentry, 0xFF, (ntiles + 1) * sizeof(uint32_t), s));
  DFH_HIP(hipMemsetAsync(z->d_head, 0, LZD_HEAD_WORDS * sizeof(uint32_t), s));
  if (ntiles) {
    hipLaunchKernelGGL(k_lzd_ff, dim3((unsigned)ntiles), dim3(256), 0, s, *job, z->d_tnext);
    hipLaunchKernelGGL(k_lzd_ffnext, dim3(5), dim3(64), 0, s, *job, z->d_tnext);
    hipLaunchKernelGGL(k_lzd_links, dim3((unsigned)ntiles), dim3(256), 0, s, *job, z->d_tnext, z->d_exit, z->d_outv);
  }
  hipLaunchKernelGGL(k_lzd_chain, dim3(5), dim3(64), 0, s, *job, z->d_exit, z->d_outv, z->d_tentry, z->d_tout, z->d_head);
  DFH_HIP(hipGetLastError());
  DFH_HIP(hipMemcpyAsync(z->h_head, z->d_head, 10 * sizeof(uint32_t), hipMemcpyDeviceToHost, s));
  return tp_wait(tc);
}

// job->dst and job->expect are set and equal the sizes the chains gave: literals, pointers, jumps, matches (nothing waits here)
int lzd_outputs(dfh_textchunk* tc, dfh_lzd* z, LzdJob* job) {
  hipStream_t s = tc->s;
  job->obase[0] = 0;
  uint32_t longest = 0;
  size_t sum = 0;
  for (int a = 0; a < 5; ++a) {
    sum += ((size_t)job->expect[a] + 15) & ~static_cast<size_t>(15);
    DFH_ARG(sum <= LZD_MAX_POINTERS, "rec decode: the outputs of one call hold 2^32 bytes or more");   // (callers check first)
    job->obase[a + 1] = (uint32_t)sum;
    longest = std::max(longest, job->expect[a]);
  }
  const uint32_t total = job->obase[5];
  if (!total) return DFH_OK;
  int rc = tp_reserve(&z->d_ptr, &z->cap_ptr, (size_t)total);
  if (rc) return rc;
  hipLaunchKernelGGL(k_lzd_list, dim3(job->tile0[5]), dim3(256), 0, s, *job, z->d_tnext, z->d_tentry, z->d_tout, z->d_ptr, z->d_head);
  uint32_t rounds = 1;
  while (rounds < LZD_MAX_ROUNDS - 1 && (1ull << rounds) < longest) ++rounds;   // a pointer is at most `longest` steps from its literal
  const unsigned grid = (total + 255u) / 256u;
  for (uint32_t r = 0; r < rounds; ++r)
    hipLaunchKernelGGL(k_lzd_jump, dim3((total / 4u + 255u) / 256u), dim3(256), 0, s, *job, z->d_ptr, z->d_head + LZD_ROUND0 + r, r == 0 ? 1 : 0);
  hipLaunchKernelGGL(k_lzd_gather, dim3(grid), dim3(256), 0, s, *job, z->d_ptr);
  DFH_HIP(hipGetLastError());
  return DFH_OK;
}
}  // namespace

extern "C" {

int dfh_lz4_decompress(dfh_ctx* c, const void* src, size_t n, void* dst, size_t expect, int* ok) {
  DFH_ARG(c && ok && (src || n == 0) && (dst || expect == 0), "dfh_lz4_decompress: NULL argument");
  DFH_ARG(n < LZ_MAX_INPUT && expect < LZ_MAX_INPUT, "dfh_lz4_decompress: 2^31 - 2^25 bytes or more do not go into one LZ4 block");
  *ok = 0;
  if (n == 0) {   // the host decoder's rule
    *ok = expect == 0 ? 1 : 0;
    return DFH_OK;
  }
  dfh_textchunk* tc = nullptr;
  int rc = dfh_textchunk_create(c, 1, &tc);
  if (rc) return rc;
  dfh_lzd* z = nullptr;
  rc = lzd_get(tc, &z);
  LzdJob job{};
  job.n[0] = (uint32_t)n;
  const void* host[5] = {src, nullptr, nullptr, nullptr, nullptr};
  if (!rc) rc = lzd_chains(tc, z, &job, host);
  if (!rc && z->h_head[0] == 1u && z->h_head[1] == (uint32_t)expect) {
    rc = tp_reserve(&z->d_dst, &z->cap_dst, std::max<size_t>(expect, 16));
    job.dst[0] = z->d_dst;
    job.expect[0] = (uint32_t)expect;
    if (!rc) rc = lzd_outputs(tc, z, &job);
    if (!rc && hipMemcpyAsync(z->h_head + LZD_STATUS, z->d_head + LZD_STATUS, sizeof(uint32_t), hipMemcpyDeviceToHost, tc->s) != hipSuccess) {
      set_error("dfh_lz4_decompress: the read-back of the status failed");
      rc = DFH_ERR_HIP;
    }
    if (!rc) rc = tp_wait(tc);
    if (!rc && z->h_head[LZD_STATUS] == 0u) {
      if (expect && hipMemcpy(dst, z->d_dst, expect, hipMemcpyDeviceToHost) != hipSuccess) {
        set_error("dfh_lz4_decompress: the read-back of the bytes failed");
        rc = DFH_ERR_HIP;
      } else {
        *ok = 1;
      }
    }
  }
  dfh_textchunk_destroy(tc);
  return rc;
}

int dfh_textchunk_decode_crb(dfh_textchunk* tc, const void* record, size_t len, int* regular, size_t* nrows_out, size_t* nnz_out) {
  DFH_ARG(tc && regular && nrows_out && nnz_out && (record || len == 0), "dfh_textchunk_decode_crb: NULL argument");
  *regular = 0;
  *nrows_out = *nnz_out = 0;
  tc->valid = false;
  // the header DecompressRowBlock accepts (host/batch_reader.h); whatever it would refuse or this path does not hold is left to it
  const char* data = static_cast<const char*>(record);
  size_t cur = 0;
  int32_t word[3];
  if (len < sizeof(word)) return DFH_OK;
  memcpy(word, data, sizeof(word));
  cur = sizeof(word);
  if (word[0] != 1196140743 || word[1] != 8 || word[2] < 1) return DFH_OK;
  const size_t nrows = (size_t)word[2];
  if (nrows * sizeof(float) > (len - cur) * 255 + 64) return DFH_OK;
  LzdJob job{};
  const void* host[5] = {nullptr, nullptr, nullptr, nullptr, nullptr};
  for (int a = 0; a < 5; ++a) {
    int32_t cp;
    if (cur + sizeof(cp) > len) return DFH_OK;
    memcpy(&cp, data + cur, sizeof(cp));
    cur += sizeof(cp);
    if (cp <= 0) continue;
    if (cur + (size_t)cp > len || (size_t)cp >= LZ_MAX_INPUT) return DFH_OK;
    host[a] = data + cur;
    job.n[a] = (uint32_t)cp;
    cur += (size_t)cp;
  }
  if (!job.n[1] || !job.n[2] || job.n[3] || job.n[4]) return DFH_OK;   // offsets and ids are needed; values and weights stay on the host
  DFH_HIP(hipSetDevice(tc->ctx->device));
  dfh_lzd* z = nullptr;
  int rc = lzd_get(tc, &z);
  if (!rc) rc = lzd_chains(tc, z, &job, host);
  if (rc) return rc;
  const uint32_t* h = z->h_head;
  const size_t lab_bytes = nrows * sizeof(float), off_bytes = (nrows + 1) * sizeof(uint64_t), idx_bytes = h[5];
  if ((job.n[0] && (h[0] != 1u || h[1] != lab_bytes)) || h[2] != 1u || h[3] != off_bytes || h[4] != 1u || idx_bytes == 0 || idx_bytes % 8 != 0 ||
      idx_bytes >= LZ_MAX_INPUT || off_bytes >= LZ_MAX_INPUT || lab_bytes + off_bytes + idx_bytes + 64 > LZD_MAX_POINTERS)
    return DFH_OK;   // (the last two: each size is below 2^31, their sum must stay below 2^32 too; the host decoder takes such a record)
  const size_t nnz = idx_bytes / 8;
  rc = tp_reserve(&tc->d_off, &tc->cap_off, nrows + 1);
  if (!rc) rc = tp_reserve(&tc->d_lab, &tc->cap_lab, nrows);
  if (!rc) rc = tp_reserve(&tc->d_ids, &tc->cap_nnz, nnz);
  if (!rc) rc = tp_reserve(&z->d_dst, &z->cap_dst, off_bytes);
  if (rc) return rc;
  if (tc->h_rows_cap < nrows + 1) {
    if (tc->h_rows) DFH_HIP(hipHostFree(tc->h_rows));
    tc->h_rows = nullptr;
    tc->h_rows_cap = 0;
    const size_t cap = nrows + 1 + nrows / 8;
    DFH_HIP(hipHostMalloc(reinterpret_cast<void**>(&tc->h_rows), cap * 8, hipHostMallocDefault));
    tc->h_rows_cap = cap;
  }
  hipStream_t s = tc->s;
  job.dst[0] = reinterpret_cast<uint8_t*>(tc->d_lab);
  job.dst[1] = z->d_dst;
  job.dst[2] = reinterpret_cast<uint8_t*>(tc->d_ids);
  job.expect[0] = job.n[0] ? (uint32_t)lab_bytes : 0u;
  job.expect[1] = (uint32_t)off_bytes;
  job.expect[2] = (uint32_t)idx_bytes;
  if (!job.n[0]) DFH_HIP(hipMemsetAsync(tc->d_lab, 0, lab_bytes, s));   // no label array: labels are 0
  rc = lzd_outputs(tc, z, &job);
  if (rc) return rc;
  hipLaunchKernelGGL(k_lzd_offsets, dim3((unsigned)((nrows + 1 + 255) / 256)), dim3(256), 0, s, reinterpret_cast<const uint64_t*>(z->d_dst),
                     (uint32_t)nrows, (uint32_t)nnz, tc->d_off, z->d_head);
  DFH_HIP(hipGetLastError());
  DFH_HIP(hipMemcpyAsync(tc->h_rows, tc->d_off, (nrows + 1) * sizeof(uint32_t), hipMemcpyDeviceToHost, s));
  DFH_HIP(hipMemcpyAsync(tc->h_rows + tc->h_rows_cap * 4, tc->d_lab, nrows * sizeof(float), hipMemcpyDeviceToHost, s));
  DFH_HIP(hipMemcpyAsync(z->h_head + LZD_STATUS, z->d_head + LZD_STATUS, sizeof(uint32_t), hipMemcpyDeviceToHost, s));
  rc = tp_wait(tc);
  if (rc) return rc;
  if (z->h_head[LZD_STATUS] != 0u) return DFH_OK;
  tc->nrows = nrows;
  tc->nnz = nnz;
  tc->valid = true;
  *regular = 1;
  *nrows_out = nrows;
  *nnz_out = nnz;
  return DFH_OK;
}

}  // extern "C"
