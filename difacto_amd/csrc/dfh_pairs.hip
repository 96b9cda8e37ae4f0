// dfh_pairs.hip — each feature's strongest FM interaction partners (included behind dfh_dumptext.hip; pairs_out of task = dump).
//
// DEFINITION.  The CANDIDATES are the dump's entries that have V: nV of them, numbered 0 .. nV - 1 in the dump's sorted order
// (their POSITIONS).  The model's weight on the product x_i x_j is s(i, j) = sum_d V_i[d] * V_j[d], computed in fp32: fp32
// products, fp32 accumulation over d.  A QUERY entry i gets the K candidates j != i with the largest key, where the key is
// |s(i, j)| for by = DFH_PAIRS_ABS and s(i, j) for by = DFH_PAIRS_POS (+0 and -0 are one key).  Inside a list and at the K
// boundary: key descending, equal keys by ascending position — that is ascending printed id, which is unique.  A query without
// V gets an empty list; a query with fewer than K other candidates gets all of them.  A pair whose score is not finite (NaN or
// +-Inf) never enters a list; such (query, candidate) pairs, j != i, of the call's queries are counted and reported.  Every
// pair's sum runs over d in the same instruction order whichever block computes it, so with the tie rule the output is a
// function of the model alone: not of the window, the splits or the grid.
//
// dfh_dump_pairs queues, the first time, k_pairs_flags + rocprim::exclusive_scan (entry -> position: epos[e] = entries with V
// before e, epos[n] = nV) and k_pairs_pack; their results are kept with the dfh_dump and cost
// 4 * kd * (roundup(nV, 128) + 128) + 4 * nV + 4 * (n + 1) bytes of device memory, kd = roundup(V_dim, 8).  Every call queues
// k_pairs_topk and k_pairs_merge.  S = "pairs_split" of the context, or chosen so that the grid has two blocks per CU while a
// split is no shorter than four tiles; no bit of the output depends on it.
// Limits: K in 1 .. 32; any V_dim the table holds.  Inputs stay fp32 (no bf16 / xf32 form: the scores are model quantities).
// The three stages are timed as DFH_K_PAIRS_PACK / _SWEEP / _MERGE when the context's timing is on.
//
//   k_pairs_flags   1 per entry with V, for the scan that numbers the candidates' positions
//   k_pairs_pack    P[rows][kd], the has-V entries' V rows in position order.  kd = V_dim rounded up to the staged chunk of 8
//                   floats (four K-steps of the 32x32x2 MFMA per lane half); rows = nV rounded up to the tile of 128, and one
//                   more tile so that a query window that starts inside a tile never reads past the end.  All padding is zero
//                   (the caller clears P; 0 * 0 adds an exact 0 to every sum).  16 B loads from the table's rows, 16 B stores;
//                   and the position -> entry map.
//   k_pairs_topk    grid (query tiles, S candidate splits), 256 threads.  A block owns 128 query positions and sweeps its range
//                   of candidate tiles of 128; the n x n scores are never written to memory.  Both operands of a tile go
//                   through LDS in chunks of 8 floats of d, row-major with a row stride of 12 floats: 16 consecutive rows start
//                   at 16 distinct multiples of 4 banks, so the ds_read_b128 a lane makes per operand and chunk (its row, its
//                   half's 4 floats) is free of bank conflicts.  The chunks are double-buffered: the 16 B global loads of
//                   chunk t + 1 are in flight while chunk t's MFMAs run, one barrier per chunk.  Wave w holds the
//                   accumulators of query rows 32 w .. 32 w + 31 against all 128 candidates of the tile (four 32x32 blocks
//                   of v_mfma_f32_32x32x2_f32, 64 registers), so a query row's list belongs to ONE wave and the selection
//                   needs no barrier and no atomic.  Every pair's sum is one chain of MFMA steps, chunk after chunk, the
//                   same in every block.  LDS: 24 KB staging + 128 * K * 8 B lists + 512 B thresholds <= 56.5 KB: two
//                   workgroups per CU.
//                   Selection, when a tile's accumulators are complete: every row keeps its K best as 64-bit words
//                   {orderable key : 31 bits of (2^31 - 1 - position) : sign of s}, descending — one unsigned compare IS the
//                   composite order (key descending, then the smaller position) — and the float key of its K-th (-inf while
//                   the list is short, +inf for a row that is no query).  A lane compares each accumulator element with its
//                   row's threshold; the wave's survivors (and non-finite elements) are taken one at a time: masked (self,
//                   padding, not a query), counted if not finite, else inserted by the whole wave — lane e holds entry e, a
//                   ballot gives the place, the tail moves up one.  The first tiles insert much; a row's expected insertions
//                   over n candidates are about K (1 + ln(n / K)), so after them nearly every element costs its one compare.
//                   Out: the block's K words per row, the partial list of split y.
//   k_pairs_merge   a wave per query entry: the S partial lists (each descending: a list is left at its first word that does
//                   not enter) merged into K under the same order; printed ids through the map and the dump's ids, scores,
//                   lengths.  Entries without V get length 0.

namespace {
constexpr uint32_t PR_T = 128, PR_KC = 8, PR_LS = 12;   // tile rows; floats of d per staged chunk; LDS row stride in floats
constexpr uint32_t PR_KMAX = 32, PR_SMAX = 64;          // partners per list; candidate splits

typedef float pr_f16 __attribute__((ext_vector_type(16)));

__device__ __forceinline__ uint32_t pr_orderable(float f) {   // monotone: a < b  <=>  orderable(a) < orderable(b)
  const uint32_t u = __float_as_uint(f);
  return u ^ ((u >> 31) ? 0xFFFFFFFFu : 0x80000000u);
}
__device__ __forceinline__ float pr_key_of(uint32_t o) { return __uint_as_float(o ^ ((o >> 31) ? 0x80000000u : 0xFFFFFFFFu)); }
__device__ __forceinline__ bool pr_finite(float s) { return fabsf(s) <= 3.402823466e+38f; }
// orders the wave's own LDS accesses where lanes read what other lanes of the wave wrote: a fence of wavefront scope for the memory
// model and a barrier the compiler moves nothing across (a wave's DS operations complete in order: no instruction is needed)
__device__ __forceinline__ void pr_wave_sync() {
  __builtin_amdgcn_fence(__ATOMIC_ACQ_REL, "wavefront");
  __builtin_amdgcn_wave_barrier();
}

__global__ void __launch_bounds__(256) k_pairs_flags(const uint32_t* __restrict__ rows, uint64_t n, uint32_t* __restrict__ flags) {
  for (uint64_t e = (uint64_t)blockIdx.x * 256 + threadIdx.x; e <= n; e += (uint64_t)gridDim.x * 256)
    flags[e] = e < n && (rows[e] & kHasV) ? 1u : 0u;
}

// a thread per (entry, group of 4 floats): kd / 4 groups per entry
__global__ void __launch_bounds__(256) k_pairs_pack(const float* __restrict__ va, uint32_t k, uint32_t kp, uint32_t kd,
                                                    const uint32_t* __restrict__ rows, const uint32_t* __restrict__ epos, uint64_t n,
                                                    float* __restrict__ P, uint32_t* __restrict__ map) {
  const uint64_t G = kd / 4, total = n * G;
  for (uint64_t i = (uint64_t)blockIdx.x * 256 + threadIdx.x; i < total; i += (uint64_t)gridDim.x * 256) {
    const uint64_t e = i / G;
    const uint32_t g = (uint32_t)(i - e * G), rw = rows[e];
    if (!(rw & kHasV)) continue;
    const uint32_t pos = epos[e];
    float4 v = make_float4(0.f, 0.f, 0.f, 0.f);
    if (4 * g < k) {   // (a table row's V is 2 * kp floats, kp = V_dim rounded up to 4: 16 B aligned, the group inside it)
      v = *reinterpret_cast<const float4*>(va + (size_t)(rw & kRowMask) * (2 * kp) + 4 * g);
      if (4 * g + 1 >= k) v.y = 0.f;
      if (4 * g + 2 >= k) v.z = 0.f;
      if (4 * g + 3 >= k) v.w = 0.f;
    }
    *reinterpret_cast<float4*>(P + (size_t)pos * kd + 4 * g) = v;
    if (g == 0) map[pos] = (uint32_t)e;
  }
}

// grid (query tiles, S); dynamic LDS: PR_T * K * 8 bytes.  Queries are positions [vq0, vq1); P has a tile of zero rows
// behind roundup(nV, PR_T), so rows vq0 + 128 x + 127 exist.  CT candidate tiles; split y takes [y CT / S, (y + 1) CT / S).
__global__ void __launch_bounds__(256, 2) k_pairs_topk(const float* __restrict__ P, uint32_t kd, uint32_t nV, uint32_t vq0, uint32_t vq1,
                                                       uint32_t CT, uint32_t K, int by_pos, unsigned long long* __restrict__ part,
                                                       unsigned long long* __restrict__ nonfinite) {
  __shared__ __attribute__((aligned(16))) float s_stage[2][2][PR_T * PR_LS];   // [buffer][queries | candidates]
  __shared__ float s_thr[PR_T];
  extern __shared__ __attribute__((aligned(16))) unsigned long long s_list[];  // [PR_T][K], descending, 0: empty
  const uint32_t tid = threadIdx.x, lane = tid & 63u, wave = tid >> 6, h = lane >> 5, li = lane & 31u;
  const uint32_t S = gridDim.y, y = blockIdx.y;
  const uint32_t t0 = (uint32_t)((uint64_t)y * CT / S), t1 = (uint32_t)((uint64_t)(y + 1) * CT / S);
  const uint32_t qbase = vq0 + blockIdx.x * PR_T, wrow0 = wave * 32u;
  const uint32_t NC = kd / PR_KC, total = (t1 - t0) * NC;
  // the wave's own rows: lists empty, thresholds open (closed for rows that are no query)
  for (uint32_t i = lane; i < 32u * K; i += 64u) s_list[(size_t)wrow0 * K + i] = 0ull;
  if (lane < 32u) s_thr[wrow0 + lane] = qbase + wrow0 + lane < vq1 ? -__builtin_inff() : __builtin_inff();
  // staging: thread -> (row tid / 2, the 4 floats of half tid % 2) of both operands
  const uint32_t lr = tid >> 1, lq = tid & 1u;
  const float* const gA = P + (size_t)(qbase + lr) * kd + 4 * lq;
  const float* const gB = P + (size_t)lr * kd + 4 * lq;
  const uint32_t st_at = lr * PR_LS + 4 * lq;
  float4 ra = make_float4(0.f, 0.f, 0.f, 0.f), rb = ra;
  if (total) {
    ra = *reinterpret_cast<const float4*>(gA);
    rb = *reinterpret_cast<const float4*>(gB + (size_t)t0 * PR_T * kd);
    *reinterpret_cast<float4*>(&s_stage[0][0][st_at]) = ra;
    *reinterpret_cast<float4*>(&s_stage[0][1][st_at]) = rb;
  }
  __syncthreads();
  pr_f16 acc[4];
  uint32_t nf = 0;   // the wave's non-finite pairs (the same in every lane)
  uint32_t tile = t0, ch = 0;
  for (uint32_t it = 0; it < total; ++it) {
    const uint32_t buf = it & 1u;
    uint32_t ntile = tile, nch = ch + 1;
    if (nch == NC) {
      nch = 0;
      ++ntile;
    }
    const bool more = it + 1 < total;
    if (more) {   // chunk it + 1 on its way while this one is multiplied
      ra = *reinterpret_cast<const float4*>(gA + nch * PR_KC);
      rb = *reinterpret_cast<const float4*>(gB + (size_t)ntile * PR_T * kd + nch * PR_KC);
    }
    if (ch == 0) {
#pragma unroll
      for (int c = 0; c < 4; ++c)
#pragma unroll
        for (int r = 0; r < 16; ++r) acc[c][r] = 0.f;
    }
    {
      const float4 a = *reinterpret_cast<const float4*>(&s_stage[buf][0][(wrow0 + li) * PR_LS + 4 * h]);
      float4 b[4];
#pragma unroll
      for (int c = 0; c < 4; ++c) b[c] = *reinterpret_cast<const float4*>(&s_stage[buf][1][(c * 32u + li) * PR_LS + 4 * h]);
      // four K-steps, each over {a d of half 0, a d of half 1}; the four blocks interleaved so that no step waits for the one before
#pragma unroll
      for (int c = 0; c < 4; ++c) acc[c] = __builtin_amdgcn_mfma_f32_32x32x2f32(a.x, b[c].x, acc[c], 0, 0, 0);
#pragma unroll
      for (int c = 0; c < 4; ++c) acc[c] = __builtin_amdgcn_mfma_f32_32x32x2f32(a.y, b[c].y, acc[c], 0, 0, 0);
#pragma unroll
      for (int c = 0; c < 4; ++c) acc[c] = __builtin_amdgcn_mfma_f32_32x32x2f32(a.z, b[c].z, acc[c], 0, 0, 0);
#pragma unroll
      for (int c = 0; c < 4; ++c) acc[c] = __builtin_amdgcn_mfma_f32_32x32x2f32(a.w, b[c].w, acc[c], 0, 0, 0);
    }
    if (ch + 1 == NC) {   // the tile is complete: element r of block c is (row 8 (r / 4) + 4 h + r % 4, candidate 32 c + li)
      const uint32_t cbase = tile * PR_T;
#pragma unroll
      for (int c = 0; c < 4; ++c) {
#pragma unroll
        for (int r = 0; r < 16; ++r) {
          const float s = acc[c][r];
          const uint32_t rr = wrow0 + 8u * (r >> 2) + (r & 3u);
          const float key = by_pos ? s : fabsf(s);
          unsigned long long m = __ballot(key >= s_thr[rr + 4u * h] || !pr_finite(s));
          while (m) {   // wave-uniform from here on
            const uint32_t src = (uint32_t)__ffsll((long long)m) - 1u;
            m &= m - 1ull;
            const float sv = __shfl(s, (int)src, 64);
            const uint32_t qr = rr + 4u * (src >> 5), qpos = qbase + qr, cpos = cbase + 32u * c + (src & 31u);
            if (qpos >= vq1 || cpos >= nV || cpos == qpos) continue;
            if (!pr_finite(sv)) {
              ++nf;
              continue;
            }
            float kf = by_pos ? sv : fabsf(sv);
            if (kf == 0.f) kf = 0.f;   // -0 and +0: one key
            const uint32_t sign = by_pos ? 0u : (__float_as_uint(sv) >> 31);
            const unsigned long long w64 = ((unsigned long long)pr_orderable(kf) << 32) | (unsigned long long)(((0x7FFFFFFFu - cpos) << 1) | sign);
            unsigned long long* const L = s_list + (size_t)qr * K;
            const unsigned long long v = lane < K ? L[lane] : 0ull;
            const uint32_t p = (uint32_t)__popcll(__ballot(lane < K && v > w64));   // the entries that stay in front
            if (p >= K) continue;
            if (lane >= p && lane + 1 < K) L[lane + 1] = v;
            if (lane == p) L[p] = w64;
            pr_wave_sync();   // other lanes' stores, before the K-th is read
            const unsigned long long last = L[K - 1];
            if (last != 0ull && lane == 0) s_thr[qr] = pr_key_of((uint32_t)(last >> 32));
            pr_wave_sync();   // the list and the threshold, before the next element's reads
          }
        }
      }
    }
    if (more) {
      *reinterpret_cast<float4*>(&s_stage[buf ^ 1u][0][st_at]) = ra;
      *reinterpret_cast<float4*>(&s_stage[buf ^ 1u][1][st_at]) = rb;
    }
    __syncthreads();
    tile = ntile;
    ch = nch;
  }
  unsigned long long* const out = part + ((size_t)blockIdx.x * S + y) * PR_T * K;
  for (uint32_t i = tid; i < PR_T * K; i += 256u) out[i] = s_list[i];
  if (nf && lane == 0) atomicAdd(nonfinite, (unsigned long long)nf);
}

// a wave per entry of [first, first + count); part == nullptr: no entry of the window has V
__global__ void __launch_bounds__(256) k_pairs_merge(const unsigned long long* __restrict__ part, uint32_t S, uint32_t K, uint32_t vq0,
                                                     const uint32_t* __restrict__ epos, const uint32_t* __restrict__ rows,
                                                     const uint64_t* __restrict__ ids, const uint32_t* __restrict__ map, uint64_t first,
                                                     uint64_t count, uint64_t* __restrict__ o_id, float* __restrict__ o_score,
                                                     uint32_t* __restrict__ o_n) {
  const uint32_t lane = threadIdx.x & 63u;
  const uint64_t x = (uint64_t)blockIdx.x * 4 + (threadIdx.x >> 6);
  if (x >= count) return;
  const uint64_t e = first + x;
  unsigned long long v = 0ull;   // lane l < K: entry l of the list
  if (part != nullptr && (rows[e] & kHasV)) {
    const uint32_t q = epos[e] - vq0;
    for (uint32_t y = 0; y < S; ++y) {
      const unsigned long long* const L = part + (((size_t)(q / PR_T) * S + y) * PR_T + q % PR_T) * K;
      for (uint32_t j = 0; j < K; ++j) {
        const unsigned long long w64 = L[j];
        if (w64 == 0ull) break;
        const uint32_t p = (uint32_t)__popcll(__ballot(lane < K && v > w64));
        if (p >= K) break;   // the rest of this list is smaller still
        const uint32_t lo = (uint32_t)__shfl_up((int)(uint32_t)v, 1, 64), hi = (uint32_t)__shfl_up((int)(uint32_t)(v >> 32), 1, 64);
        if (lane == p) v = w64;
        else if (lane > p) v = ((unsigned long long)hi << 32) | lo;
      }
    }
  }
  const uint32_t len = (uint32_t)__popcll(__ballot(lane < K && v != 0ull));
  if (lane == 0) o_n[x] = len;
  if (lane < K) {
    uint64_t id = 0;
    float score = 0.f;
    if (v != 0ull) {
      const uint32_t lo = (uint32_t)v;
      const float key = pr_key_of((uint32_t)(v >> 32));
      id = ids[map[0x7FFFFFFFu - (lo >> 1)]];
      score = (lo & 1u) ? -key : key;
    }
    o_id[x * K + lane] = id;
    o_score[x * K + lane] = score;
  }
}

void pairs_release(dfh_dump* p) {
  dfh_dump::Pairs& r = p->pr;
  if (r.P) (void)hipFree(r.P);
  if (r.epos) (void)hipFree(r.epos);
  if (r.map) (void)hipFree(r.map);
  if (r.part) (void)hipFree(r.part);
  if (r.out) (void)hipFree(r.out);
  if (r.d_nf) (void)hipFree(r.d_nf);
  r = dfh_dump::Pairs();
}

// the first call's work: epos, map, P
int pairs_build(dfh_dump* p) {
  dfh_dump::Pairs& r = p->pr;
  const char* who = "dfh_dump_pairs";
  hipStream_t s = p->ctx->stream;
  const uint64_t n = p->n, nV = p->n_with_V;
  r.kd = (p->k + PR_KC - 1) / PR_KC * PR_KC;
  r.rows = (nV + PR_T - 1) / PR_T * PR_T + PR_T;
  size_t fcap = 0, ecap = 0, mcap = 0, pcap = 0, ncap = 0;
  uint32_t* flags = nullptr;
  size_t need = 0;
  DFH_HIP(rocprim::exclusive_scan(nullptr, need, (uint32_t*)nullptr, (uint32_t*)nullptr, 0u, (size_t)n + 1, rocprim::plus<uint32_t>(), s));
  int rc = dev_grow(&flags, &fcap, (size_t)n + 1, who, "the has-V flags");
  if (!rc) rc = dev_grow(&r.epos, &ecap, (size_t)n + 1, who, "the entries' positions");
  if (!rc) rc = dev_grow(&r.map, &mcap, (size_t)nV, who, "the positions' entries");
  if (!rc) rc = dev_grow(&r.P, &pcap, (size_t)r.rows * r.kd, who, "the packed V rows");
  if (!rc) rc = dev_grow(&r.d_nf, &ncap, 1, who, "the non-finite count");
  if (!rc) rc = dev_grow(&p->text.d_tmp, &p->text.tmp_bytes, std::max<size_t>(need, 256), who, "the scan");
  hipError_t e = hipSuccess;
  if (!rc) {
    TimeScope ts(p->ctx, DFH_K_PAIRS_PACK);
    const TableView& v = p->t->v;
    size_t tb = p->text.tmp_bytes;
    e = hipMemsetAsync(r.P, 0, (size_t)r.rows * r.kd * sizeof(float), s);
    if (e == hipSuccess) {
      hipLaunchKernelGGL(k_pairs_flags, dim3((unsigned)grid_for_threads((size_t)n + 1, p->ctx)), dim3(256), 0, s, (const uint32_t*)p->d_row, n, flags);
      e = hipGetLastError();
    }
    if (e == hipSuccess) e = rocprim::exclusive_scan(p->text.d_tmp, tb, flags, r.epos, 0u, (size_t)n + 1, rocprim::plus<uint32_t>(), s);
    if (e == hipSuccess) {
      hipLaunchKernelGGL(k_pairs_pack, dim3((unsigned)grid_for_threads((size_t)n * (r.kd / 4), p->ctx)), dim3(256), 0, s, (const float*)v.va, p->k,
                         (uint32_t)v.kp, r.kd, (const uint32_t*)p->d_row, (const uint32_t*)r.epos, n, r.P, r.map);
      e = hipGetLastError();
    }
  }
  if (!rc && e == hipSuccess) e = hipStreamSynchronize(s);
  if (flags) (void)hipFree(flags);
  if (rc || e != hipSuccess) {
    pairs_release(p);
    if (rc) return rc;
    (void)hipGetLastError();
    set_error(std::string("dfh_dump_pairs: ") + hipGetErrorString(e));
    return DFH_ERR_HIP;
  }
  r.built = true;
  return DFH_OK;
}
}  // namespace

extern "C" int dfh_dump_pairs(dfh_dump* p, uint64_t first, size_t count, int topk, int by, uint64_t* partner_ids, float* scores,
                              uint32_t* npartners, uint64_t* nonfinite) {
  DFH_ARG(p && nonfinite, "dfh_dump_pairs: NULL argument");
  *nonfinite = 0;
  DFH_ARG(first <= p->n && count <= p->n - first, "dfh_dump_pairs: first + count exceeds the dump's entries");
  DFH_ARG(topk >= 1 && topk <= (int)PR_KMAX, "dfh_dump_pairs: topk must be in [1, 32]");
  DFH_ARG(by == DFH_PAIRS_ABS || by == DFH_PAIRS_POS, "dfh_dump_pairs: by must be DFH_PAIRS_ABS or DFH_PAIRS_POS");
  if (count == 0) return DFH_OK;
  DFH_ARG(partner_ids && scores && npartners, "dfh_dump_pairs: NULL argument");
  const uint32_t K = (uint32_t)topk;
  if (p->n_with_V == 0 || p->k == 0) {   // no candidates: no launch, every list is empty
    memset(partner_ids, 0, count * K * sizeof(uint64_t));
    memset(scores, 0, count * K * sizeof(float));
    memset(npartners, 0, count * sizeof(uint32_t));
    return DFH_OK;
  }
  dfh_ctx* c = p->ctx;
  hipStream_t s = c->stream;
  DFH_HIP(hipSetDevice(c->device));
  dfh_dump::Pairs& r = p->pr;
  if (!r.built) {
    int rc = pairs_build(p);
    if (rc) return rc;
  }
  uint32_t vq[2] = {0, 0};   // the window's positions
  DFH_HIP(hipMemcpyAsync(&vq[0], r.epos + first, sizeof(uint32_t), hipMemcpyDeviceToHost, s));
  DFH_HIP(hipMemcpyAsync(&vq[1], r.epos + first + count, sizeof(uint32_t), hipMemcpyDeviceToHost, s));
  DFH_HIP(hipStreamSynchronize(s));
  const uint32_t nV = (uint32_t)p->n_with_V;
  DFH_ARG(vq[0] <= vq[1] && vq[1] <= nV, "dfh_dump_pairs: the table changed while the dump is open");
  const uint32_t nq = vq[1] - vq[0], QT = (nq + PR_T - 1) / PR_T, CT = (nV + PR_T - 1) / PR_T;
  uint32_t S = (uint32_t)c->pairs_split;
  if (S == 0 && QT) {   // enough blocks for two per CU, a split no shorter than four tiles
    S = (2u * (uint32_t)c->num_cu + QT - 1) / QT;
    S = std::min(S, std::max(1u, CT / 4));
  }
  S = std::max(1u, std::min(std::min(S, CT), PR_SMAX));
  const char* who = "dfh_dump_pairs";
  const size_t out_bytes = count * K * (sizeof(uint64_t) + sizeof(float)) + count * sizeof(uint32_t);
  int rc = dev_grow(&r.out, &r.out_cap, out_bytes, who, "the lists");
  if (!rc && QT) rc = dev_grow(&r.part, &r.part_cap, (size_t)QT * S * PR_T * K, who, "the splits' partial lists");
  if (rc) return rc;
  uint64_t* o_id = reinterpret_cast<uint64_t*>(r.out);   // 8 B, then the 4 B arrays
  float* o_score = reinterpret_cast<float*>(o_id + count * K);
  uint32_t* o_n = reinterpret_cast<uint32_t*>(o_score + count * K);
  DFH_HIP(hipMemsetAsync(r.d_nf, 0, sizeof(unsigned long long), s));
  if (QT) {
    TimeScope ts(c, DFH_K_PAIRS_SWEEP);
    hipLaunchKernelGGL(k_pairs_topk, dim3(QT, S), dim3(256), (size_t)PR_T * K * sizeof(unsigned long long), s, (const float*)r.P, r.kd, nV, vq[0],
                       vq[1], CT, K, by == DFH_PAIRS_POS ? 1 : 0, r.part, r.d_nf);
    DFH_HIP(hipGetLastError());
  }
  {
    TimeScope ts(c, DFH_K_PAIRS_MERGE);
    hipLaunchKernelGGL(k_pairs_merge, dim3((unsigned)((count + 3) / 4)), dim3(256), 0, s, (const unsigned long long*)(QT ? r.part : nullptr), S, K,
                       vq[0], (const uint32_t*)r.epos, (const uint32_t*)p->d_row, (const uint64_t*)p->d_id, (const uint32_t*)r.map, first,
                       (uint64_t)count, o_id, o_score, o_n);
    DFH_HIP(hipGetLastError());
  }
  unsigned long long nf = 0;
  DFH_HIP(hipMemcpyAsync(partner_ids, o_id, count * K * sizeof(uint64_t), hipMemcpyDeviceToHost, s));
  DFH_HIP(hipMemcpyAsync(scores, o_score, count * K * sizeof(float), hipMemcpyDeviceToHost, s));
  DFH_HIP(hipMemcpyAsync(npartners, o_n, count * sizeof(uint32_t), hipMemcpyDeviceToHost, s));
  DFH_HIP(hipMemcpyAsync(&nf, r.d_nf, sizeof(nf), hipMemcpyDeviceToHost, s));
  DFH_HIP(hipStreamSynchronize(s));
  *nonfinite = nf;
  return DFH_OK;
}
