// dfh_recommend.hip — each row's best catalogue items (included behind dfh_explain.hip; uses the order helpers of dfh_pairs.hip;
// recommend_out of task = predict).
//
// DEFINITION.  ROW QUANTITIES.  A row r of a stepped minibatch has, all in fp32,
//   S_r[d] = sum_j x_j V_j[d]           over the positions j of the row whose key has V (kHasV in uw[index[j]].x, the forward's rule)
//   Q_r[d] = sum_j (x_j V_j[d])^2       over the same positions
//   lin_r  = sum_j x_j w_j              over ALL positions (a weight that is exactly 0 is skipped, not multiplied: fma_skip0)
//   b_r    = lin_r + 1/2 sum_d (S_r[d]^2 - Q_r[d])          the row's own logit (= a_r when the row is a query), not clamped
// A missing value array means x = 1; a key the model does not hold has w = 0 and no V.  Every sum over positions is ONE chain in
// ascending position order per d (S = fma(x, V, S); t = x V, Q = fma(t, t, Q); lin = fma(w, x, lin)); the sum over d adds
// fma(S, S, -Q) of a lane's four d in ascending order and then the lanes by the xor butterfly 32, 16, .. 1.  So S_r and b_r are
// functions of the model and the row alone.  The empty row has S = 0, b = 0.
// THE CATALOGUE is the rows handed to dfh_recommend_add_items, numbered 0 .. M - 1 in the order they came.  A query row q gets the
// K items with the largest s(q, i) = b_i + <S_q, S_i>, computed in fp32 as one chain of fused MFMA steps over d with the bias as
// the product 1 * b_i in column V_dim of the same chain, the same in every block.  Order: s descending, equal s (+0 and -0 are
// one key) by ascending item number; all M items when M < K.  The value handed out is the logit a_q + s(q, i): one fp32 add.
// An item whose s is not finite enters no list; such (query, item) pairs are counted.
// This is the logit of the concatenated row q u i when their positions are disjoint: logit = a_q + b_i + <S_q, S_i>.  A key that
// query and item SHARE is treated as two positions, as a concatenated row in which the key occurs twice: its cross term
// x_q x_i <V, V> is in <S_q, S_i> once, neither doubled nor dropped.
//
//   k_rec_embed   a wave per row of a stepped minibatch, lanes across d (a lane owns 4 consecutive d: one 16 B load per has-V
//                 position and 256 d; a longer V takes the row again per 256 d, each table row is still read once).  The wave
//                 stages 64 positions' {row word, w, x} and walks them with broadcasts, four row loads in flight before any is
//                 used, consuming in position order.  The forward's d_xv is NOT used: k_forward sums a row's positions in G lane
//                 groups and joins them by a butterfly, an order that depends on V_dim.  Out: the row's packed operand
//                 P[row][kd], kd = roundup(V_dim + 1, 8): S, then column V_dim = b (an item) or 1.0f (a query), zeros behind;
//                 and a[row] = b (queries).
//   the item store  P_items in HBM, appended batch by batch; capacity a multiple of the tile of 128 rows plus one zero tile behind
//                 (as k_pairs_pack leaves its array), zero wherever no item has been written; grows by doubling, the rows copied
//                 on the stream; retired arrays are freed behind the next wait (dfh_recommend_read / _destroy).
//   k_rec_topk    grid (query tiles of 128, S item splits), 256 threads, the blocking of k_pairs_topk on two operands: both go
//                 through LDS in double-buffered chunks of 8 floats of d, row stride 12 floats (16 consecutive rows start at 16
//                 distinct multiples of 4 banks: the ds_read_b128 are conflict-free); wave w owns query rows 32 w .. 32 w + 31
//                 against the tile's 128 items, four 32x32 blocks of v_mfma_f32_32x32x2_f32 (64 accumulator registers), so a
//                 row's list belongs to ONE wave: no barrier, no atomic in the selection.  The R x M scores never leave the chip.
//                 Selection: a lane compares each accumulator with its row's threshold (the K-th score; -inf while the list is
//                 short, +inf for a padding row); the wave's survivors are taken one at a time: masked by number (padding
//                 items, padding queries), counted if not finite, else inserted by the whole wave into the row's sorted list of
//                 64-bit words {orderable s : 2^31 - 1 - item} — one unsigned compare IS the composite order.  No |.|, no self
//                 mask.  LDS: 24 576 B staging + 128 K 8 B lists + 512 B thresholds <= 57 856 B: two workgroups per CU (160 KB),
//                 8 waves per CU; registers as k_pairs_topk (launch bound 2).
//   k_rec_merge   a wave per query row: the S partial lists merged under the same order; out: n, K x {item, a_q + s}, zeros
//                 behind n.
// S = "rec_split" of the context, or about two blocks per CU (floor(2 CUs / query tiles): the grid is one even round, where
// k_pairs_topk's rounds up — its grids are many rounds long) with no split shorter than four tiles; no bit of the output depends
// on S, on the grid or on how the catalogue was cut into batches.  Limits: K in 1 .. 32, M < 2^31, any V_dim the table holds
// (V_dim = 0: kd = 8, s = b_i).  Inputs stay fp32.  Plain C++, vector stores, no scratch.
// Timed as DFH_K_REC_EMBED / _SWEEP / _MERGE.

struct dfh_recommend {
  dfh_ctx* ctx = nullptr;
  uint32_t K = 0, kd = 0;
  dfh_table* table = nullptr;        // the model of the catalogue; queries are stepped on the same
  float* d_items = nullptr;          // [(items_cap + 128) * kd]
  size_t items_cap = 0, M = 0, hint = 0;
  size_t cap = 0, n = 0;             // query rows the out arrays hold / appended since the last reset
  char* d_out = nullptr;             // one allocation: items u32 [cap K], logits f32 [cap K], n u32 [cap]
  float* d_pq = nullptr;             // the appended minibatch's packed queries and a_q: one append's kernels after another use them
  size_t pq_cap = 0;
  float* d_aq = nullptr;
  size_t aq_cap = 0;
  unsigned long long* d_part = nullptr;
  size_t part_cap = 0;
  std::vector<void*> retired;        // arrays a growth replaced: queued kernels and copies may still use them
  unsigned long long* d_nf = nullptr;
  TextWork text;                     // the workspace of dfh_recommend_format (dfh_listtext.hip over dfh_textout.hip)
  bool formatted = false;            // text holds the lines of every query appended
};

namespace {
constexpr uint32_t RC_T = 128, RC_KC = 8, RC_LS = 12, RC_KMAX = 32, RC_SMAX = 64;
constexpr uint64_t RC_MAX_ITEMS = 0x7FFFFFFFULL - RC_T, RC_MAX_ROWS = 0xFFFFFFF0ULL;

struct RcIn {
  const uint32_t* offset;
  const uint32_t* index;
  const float* value;   // or NULL: x = 1
  const uint2* uw;      // {table row | flags, w} per key of the minibatch (the step's lookup)
  const float* va;      // the table's rows: [V[0 .. kp) | accumulators[0 .. kp)]
  uint32_t nrows, k, kp;
};

__global__ void __launch_bounds__(256) k_rec_embed(RcIn in, uint32_t kd, int is_item, float* __restrict__ P, float* __restrict__ a) {
  const uint32_t lane = threadIdx.x & 63u, k = in.k, kp = in.kp;
  const uint32_t rounds = (kd + 255u) / 256u;
  for (uint32_t row = blockIdx.x * 4u + (threadIdx.x >> 6); row < in.nrows; row += gridDim.x * 4u) {
    const uint32_t beg = in.offset[row], end = in.offset[row + 1];
    float lin = 0.f, quad = 0.f;
    float4 held = make_float4(0.f, 0.f, 0.f, 0.f);   // the 16 B that hold column V_dim, stored when b is known
    uint32_t held_d = 0xFFFFFFFFu;
    for (uint32_t rd = 0; rd < rounds; ++rd) {
      const uint32_t d = 256u * rd + 4u * lane;
      const bool ld_ok = d < kp;
      float4 S = make_float4(0.f, 0.f, 0.f, 0.f), Q = S;
      for (uint32_t base = beg; base < end; base += 64u) {
        const uint32_t j = base + lane, cnt = min(64u, end - base);
        uint32_t rw = 0;
        float x = 0.f, w = 0.f;
        if (j < end) {
          const uint2 e = in.uw[in.index[j]];
          rw = e.x;
          w = __uint_as_float(e.y);
          x = in.value ? in.value[j] : 1.f;
        }
        for (uint32_t t0 = 0; t0 < cnt; t0 += 4u) {
          float4 v[4];
          float xs[4], ws[4];
          bool hs[4];
#pragma unroll
          for (int q = 0; q < 4; ++q) {   // wave-uniform: every lane looks at the same position
            const uint32_t t = t0 + q;
            const uint32_t rr = (uint32_t)__shfl((int)rw, (int)(t & 63u), 64);
            xs[q] = __shfl(x, (int)(t & 63u), 64);
            ws[q] = t < cnt ? __shfl(w, (int)(t & 63u), 64) : 0.f;
            hs[q] = t < cnt && (rr & kHasV) != 0u;
            v[q] = (hs[q] && ld_ok) ? ld4(in.va + (size_t)(rr & kRowMask) * (2u * kp) + d) : make_float4(0.f, 0.f, 0.f, 0.f);
          }
#pragma unroll
          for (int q = 0; q < 4; ++q) {
            if (rd == 0) lin = fma_skip0(ws[q], xs[q], lin);
            if (!hs[q]) continue;
            const float xx = xs[q];
            float u;
            S.x = __builtin_fmaf(xx, v[q].x, S.x); u = xx * v[q].x; Q.x = __builtin_fmaf(u, u, Q.x);
            S.y = __builtin_fmaf(xx, v[q].y, S.y); u = xx * v[q].y; Q.y = __builtin_fmaf(u, u, Q.y);
            S.z = __builtin_fmaf(xx, v[q].z, S.z); u = xx * v[q].z; Q.z = __builtin_fmaf(u, u, Q.z);
            S.w = __builtin_fmaf(xx, v[q].w, S.w); u = xx * v[q].w; Q.w = __builtin_fmaf(u, u, Q.w);
          }
        }
      }
      // (a table row's floats between V_dim and kp take no part)
      if (d >= k) S.x = Q.x = 0.f;
      if (d + 1u >= k) S.y = Q.y = 0.f;
      if (d + 2u >= k) S.z = Q.z = 0.f;
      if (d + 3u >= k) S.w = Q.w = 0.f;
      quad += __builtin_fmaf(S.x, S.x, -Q.x);
      quad += __builtin_fmaf(S.y, S.y, -Q.y);
      quad += __builtin_fmaf(S.z, S.z, -Q.z);
      quad += __builtin_fmaf(S.w, S.w, -Q.w);
      if (d < kd) {
        if (k >= d && k < d + 4u) {
          held = S;
          held_d = d;
        } else {
          st4(P + (size_t)row * kd + d, S);
        }
      }
    }
    const float b = lin + 0.5f * wave_sum(quad);
    if (held_d != 0xFFFFFFFFu) {
      const float col = is_item ? b : 1.f;
      const uint32_t c = k - held_d;
      if (c == 0u) held.x = col;
      if (c == 1u) held.y = col;
      if (c == 2u) held.z = col;
      if (c == 3u) held.w = col;
      st4(P + (size_t)row * kd + held_d, held);
    }
    if (a != nullptr && lane == 0) a[row] = b;
  }
}

// grid (query tiles, S); dynamic LDS: RC_T * K * 8 bytes.  A: roundup(nq, 128) query rows; B: the item store, CT = ceil(M / 128)
// tiles, all of whose rows exist; split y takes the tiles [y CT / S, (y + 1) CT / S).
__global__ void __launch_bounds__(256, 2) k_rec_topk(const float* __restrict__ A, const float* __restrict__ B, uint32_t kd, uint32_t nq, uint32_t M,
                                                     uint32_t CT, uint32_t K, unsigned long long* __restrict__ part,
                                                     unsigned long long* __restrict__ nonfinite) {
  __shared__ __attribute__((aligned(16))) float s_stage[2][2][RC_T * RC_LS];   // [buffer][queries | items]
  __shared__ float s_thr[RC_T];
  extern __shared__ __attribute__((aligned(16))) unsigned long long s_list[];  // [RC_T][K], descending, 0: empty
  const uint32_t tid = threadIdx.x, lane = tid & 63u, wave = tid >> 6, h = lane >> 5, li = lane & 31u;
  const uint32_t S = gridDim.y, y = blockIdx.y;
  const uint32_t t0 = (uint32_t)((uint64_t)y * CT / S), t1 = (uint32_t)((uint64_t)(y + 1) * CT / S);
  const uint32_t qbase = blockIdx.x * RC_T, wrow0 = wave * 32u;
  const uint32_t NC = kd / RC_KC, total = (t1 - t0) * NC;
  for (uint32_t i = lane; i < 32u * K; i += 64u) s_list[(size_t)wrow0 * K + i] = 0ull;
  if (lane < 32u) s_thr[wrow0 + lane] = qbase + wrow0 + lane < nq ? -__builtin_inff() : __builtin_inff();
  // staging: thread -> (row tid / 2, the 4 floats of half tid % 2) of both operands
  const uint32_t lr = tid >> 1, lq = tid & 1u;
  const float* const gA = A + (size_t)(qbase + lr) * kd + 4u * lq;
  const float* const gB = B + (size_t)lr * kd + 4u * lq;
  const uint32_t st_at = lr * RC_LS + 4u * lq;
  float4 ra = make_float4(0.f, 0.f, 0.f, 0.f), rb = ra;
  if (total) {
    ra = ld4(gA);
    rb = ld4(gB + (size_t)t0 * RC_T * kd);
    st4(&s_stage[0][0][st_at], ra);
    st4(&s_stage[0][1][st_at], rb);
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
      ra = ld4(gA + nch * RC_KC);
      rb = ld4(gB + (size_t)ntile * RC_T * kd + nch * RC_KC);
    }
    if (ch == 0) {
#pragma unroll
      for (int c = 0; c < 4; ++c)
#pragma unroll
        for (int r = 0; r < 16; ++r) acc[c][r] = 0.f;
    }
    {
      const float4 a = *reinterpret_cast<const float4*>(&s_stage[buf][0][(wrow0 + li) * RC_LS + 4u * h]);
      float4 b[4];
#pragma unroll
      for (int c = 0; c < 4; ++c) b[c] = *reinterpret_cast<const float4*>(&s_stage[buf][1][(c * 32u + li) * RC_LS + 4u * h]);
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
    if (ch + 1 == NC) {   // the tile is complete: element r of block c is (row 8 (r / 4) + 4 h + r % 4, item 32 c + li)
      const uint32_t cbase = tile * RC_T;
#pragma unroll
      for (int c = 0; c < 4; ++c) {
#pragma unroll
        for (int r = 0; r < 16; ++r) {
          const float s = acc[c][r];
          const uint32_t rr = wrow0 + 8u * (r >> 2) + (r & 3u);
          unsigned long long m = __ballot(s >= s_thr[rr + 4u * h] || !pr_finite(s));
          while (m) {   // wave-uniform from here on
            const uint32_t src = (uint32_t)__ffsll((long long)m) - 1u;
            m &= m - 1ull;
            float sv = __shfl(s, (int)src, 64);
            const uint32_t qr = rr + 4u * (src >> 5), item = cbase + 32u * c + (src & 31u);
            if (qbase + qr >= nq || item >= M) continue;
            if (!pr_finite(sv)) {
              ++nf;
              continue;
            }
            if (sv == 0.f) sv = 0.f;   // -0 and +0: one key
            const unsigned long long w64 = ((unsigned long long)pr_orderable(sv) << 32) | (unsigned long long)(0x7FFFFFFFu - item);
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
      st4(&s_stage[buf ^ 1u][0][st_at], ra);
      st4(&s_stage[buf ^ 1u][1][st_at], rb);
    }
    __syncthreads();
    tile = ntile;
    ch = nch;
  }
  unsigned long long* const out = part + ((size_t)blockIdx.x * S + y) * RC_T * K;
  for (uint32_t i = tid; i < RC_T * K; i += 256u) out[i] = s_list[i];
  if (nf && lane == 0) atomicAdd(nonfinite, (unsigned long long)nf);
}

// a wave per query row of the append
__global__ void __launch_bounds__(256) k_rec_merge(const unsigned long long* __restrict__ part, uint32_t S, uint32_t K, uint32_t nq,
                                                   const float* __restrict__ aq, uint32_t* __restrict__ o_item, float* __restrict__ o_logit,
                                                   uint32_t* __restrict__ o_n) {
  const uint32_t lane = threadIdx.x & 63u;
  const uint32_t q = blockIdx.x * 4u + (threadIdx.x >> 6);
  if (q >= nq) return;
  unsigned long long v = 0ull;   // lane l < K: entry l of the list
  for (uint32_t y = 0; y < S; ++y) {
    const unsigned long long* const L = part + (((size_t)(q / RC_T) * S + y) * RC_T + q % RC_T) * K;
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
  const uint32_t len = (uint32_t)__popcll(__ballot(lane < K && v != 0ull));
  if (lane == 0) o_n[q] = len;
  if (lane < K) {
    uint32_t item = 0;
    float logit = 0.f;
    if (v != 0ull) {
      item = 0x7FFFFFFFu - (uint32_t)v;
      logit = aq[q] + pr_key_of((uint32_t)(v >> 32));
    }
    o_item[(size_t)q * K + lane] = item;
    o_logit[(size_t)q * K + lane] = logit;
  }
}

struct RcOut {
  uint32_t* item;
  float* logit;
  uint32_t* n;
};
inline size_t rc_row_bytes(uint32_t K) { return (size_t)K * (sizeof(uint32_t) + sizeof(float)) + sizeof(uint32_t); }
inline RcOut rc_arrays(char* base, size_t cap, uint32_t K, size_t at) {
  RcOut o;
  uint32_t* p4 = reinterpret_cast<uint32_t*>(base);
  o.item = p4 + at * K;
  o.logit = reinterpret_cast<float*>(p4 + cap * K) + at * K;
  o.n = p4 + 2 * cap * K + at;
  return o;
}

void rc_free_retired(dfh_recommend* r) {
  for (void* a : r->retired) (void)hipFree(a);
  r->retired.clear();
}

// a workspace of at least `need` elements; what it held is not kept
template <typename T>
int rc_workspace(dfh_recommend* r, T** p, size_t* cap, size_t need, const char* what) {
  if (need <= *cap) return DFH_OK;
  size_t nc = std::max<size_t>(*cap, (size_t)1 << 12);
  while (nc < need) nc *= 2;
  T* nv = nullptr;
  if (hipMalloc((void**)&nv, nc * sizeof(T)) != hipSuccess) {
    (void)hipGetLastError();
    set_error(std::string("dfh_recommend: no device memory for ") + what + " (" + std::to_string(nc * sizeof(T)) + " bytes needed)");
    return DFH_ERR_CAPACITY;
  }
  if (*p) r->retired.push_back(*p);
  *p = nv;
  *cap = nc;
  return DFH_OK;
}

// room for `extra` more items: a multiple of the tile, one zero tile behind; the rows held so far are copied on the stream
int rc_reserve_items(dfh_recommend* r, size_t extra) {
  const size_t need = r->M + extra;
  if (r->d_items && need <= r->items_cap) return DFH_OK;
  size_t cap = r->items_cap ? r->items_cap : std::max<size_t>((r->hint + RC_T - 1) / RC_T * RC_T, RC_T);
  while (cap < need) cap *= 2;
  float* nv = nullptr;
  const size_t bytes = (cap + RC_T) * r->kd * sizeof(float);
  if (hipMalloc((void**)&nv, bytes) != hipSuccess) {
    (void)hipGetLastError();
    set_error("dfh_recommend_add_items: no device memory for " + std::to_string(cap) + " items (" + std::to_string(bytes) + " bytes needed)");
    return DFH_ERR_CAPACITY;
  }
  hipStream_t s = r->ctx->stream;
  hipError_t er = hipMemsetAsync(nv, 0, bytes, s);
  if (er == hipSuccess && r->M) er = hipMemcpyAsync(nv, r->d_items, r->M * r->kd * sizeof(float), hipMemcpyDeviceToDevice, s);
  if (er != hipSuccess) {
    r->retired.push_back(nv);
    set_error(std::string("dfh_recommend_add_items: ") + hipGetErrorString(er));
    return DFH_ERR_HIP;
  }
  if (r->d_items) r->retired.push_back(r->d_items);
  r->d_items = nv;
  r->items_cap = cap;
  return DFH_OK;
}

// room for `extra` more query rows in the out arrays; the rows held so far are copied on the stream
int rc_reserve_out(dfh_recommend* r, size_t extra) {
  const size_t need = r->n + extra;
  if (need <= r->cap) return DFH_OK;
  size_t cap = r->cap ? r->cap : (size_t)1 << 14;
  while (cap < need) cap *= 2;
  char* nv = nullptr;
  const size_t bytes = cap * rc_row_bytes(r->K);
  if (hipMalloc((void**)&nv, bytes) != hipSuccess) {
    (void)hipGetLastError();
    set_error("dfh_recommend_append_batch: no device memory for " + std::to_string(cap) + " rows (" + std::to_string(bytes) + " bytes needed)");
    return DFH_ERR_CAPACITY;
  }
  if (r->n) {
    const RcOut a = rc_arrays(r->d_out, r->cap, r->K, 0), b = rc_arrays(nv, cap, r->K, 0);
    const size_t nk = r->n * r->K;
    hipStream_t s = r->ctx->stream;
    hipError_t er = hipMemcpyAsync(b.item, a.item, nk * sizeof(uint32_t), hipMemcpyDeviceToDevice, s);
    if (er == hipSuccess) er = hipMemcpyAsync(b.logit, a.logit, nk * sizeof(float), hipMemcpyDeviceToDevice, s);
    if (er == hipSuccess) er = hipMemcpyAsync(b.n, a.n, r->n * sizeof(uint32_t), hipMemcpyDeviceToDevice, s);
    if (er != hipSuccess) {
      r->retired.push_back(nv);
      set_error(std::string("dfh_recommend_append_batch: hipMemcpyAsync: ") + hipGetErrorString(er));
      return DFH_ERR_HIP;
    }
  }
  if (r->d_out) r->retired.push_back(r->d_out);
  r->d_out = nv;
  r->cap = cap;
  return DFH_OK;
}

// the checks both appends share; binds the object to the table the first time
int rc_check(dfh_recommend* r, dfh_batch* b, dfh_table* t, const char* who) {
  DFH_ARG(r && b && t, std::string(who) + ": NULL argument");
  DFH_ARG(b->ctx == r->ctx && t->ctx == r->ctx, std::string(who) + ": the batch or the table belongs to another context");
  if (b->stepped != t) {
    set_error(std::string(who) + ": the batch's last step was not dfh_sgd_step on this table (not stepped since its load, or stepped "
              "through the sharded store, whose row words point into the rows other owners sent)");
    return DFH_ERR_STATE;
  }
  DFH_ARG(r->table == nullptr || r->table == t, std::string(who) + ": the catalogue was built on another table");
  return DFH_OK;
}

RcIn rc_in(dfh_batch* b, dfh_table* t) {
  RcIn in;
  in.offset = b->d_offset;
  in.index = b->d_index;
  in.value = b->has_value ? b->d_value : nullptr;
  in.uw = b->d_uw;
  in.va = t->v.va;
  in.nrows = (uint32_t)b->nrows;
  in.k = (uint32_t)t->v.k;
  in.kp = (uint32_t)t->v.kp;
  return in;
}

// the batch object's NEXT load waits for ev_free alone (the hazard dfh_explain_append_batch documents)
int rc_batch_used(dfh_ctx* c, dfh_batch* b) {
  if (c->pipeline) {
    DFH_HIP(hipEventRecord(b->ev_free, c->stream));
    b->free_pending = true;
  }
  return DFH_OK;
}
}  // namespace

extern "C" {

int dfh_recommend_create(dfh_ctx* ctx, int topk, size_t capacity_hint, dfh_recommend** out) {
  DFH_ARG(ctx && out, "dfh_recommend_create: NULL argument");
  DFH_ARG(topk >= 1 && topk <= (int)RC_KMAX, "dfh_recommend_create: topk must be in [1, 32]");
  DFH_ARG(capacity_hint <= RC_MAX_ITEMS, "dfh_recommend_create: capacity_hint must be below 2^31 - 128 items");
  dfh_recommend* r = new (std::nothrow) dfh_recommend();
  if (!r) {
    set_error("dfh_recommend_create: out of host memory (" + std::to_string(sizeof(dfh_recommend)) + " bytes needed)");
    return DFH_ERR_CAPACITY;
  }
  r->ctx = ctx;
  r->K = (uint32_t)topk;
  r->hint = capacity_hint;
  hipError_t er = hipSetDevice(ctx->device);
  if (er == hipSuccess) er = hipMalloc(reinterpret_cast<void**>(&r->d_nf), sizeof(unsigned long long));
  if (er == hipSuccess) er = hipMemsetAsync(r->d_nf, 0, sizeof(unsigned long long), ctx->stream);
  if (er != hipSuccess) {
    (void)hipGetLastError();
    set_error(std::string("dfh_recommend_create: ") + hipGetErrorString(er));
    dfh_recommend_destroy(r);
    return DFH_ERR_HIP;
  }
  *out = r;
  return DFH_OK;
}

int dfh_recommend_destroy(dfh_recommend* r) {
  if (!r) return DFH_OK;
  (void)hipSetDevice(r->ctx->device);
  (void)hipStreamSynchronize(r->ctx->stream);   // queued kernels and copies read and write the arrays
  rc_free_retired(r);
  if (r->d_items) (void)hipFree(r->d_items);
  if (r->d_out) (void)hipFree(r->d_out);
  if (r->d_pq) (void)hipFree(r->d_pq);
  if (r->d_aq) (void)hipFree(r->d_aq);
  if (r->d_part) (void)hipFree(r->d_part);
  if (r->d_nf) (void)hipFree(r->d_nf);
  to_release(&r->text);
  delete r;
  return DFH_OK;
}

int dfh_recommend_reset(dfh_recommend* r) {
  DFH_ARG(r, "dfh_recommend_reset: NULL argument");
  DFH_HIP(hipSetDevice(r->ctx->device));
  DFH_HIP(hipMemsetAsync(r->d_nf, 0, sizeof(unsigned long long), r->ctx->stream));   // behind the kernels that still count
  r->n = 0;   // the catalogue and the arrays stay
  r->formatted = false;
  return DFH_OK;
}

int dfh_recommend_add_items(dfh_recommend* r, dfh_batch* b, dfh_table* t) {
  int rc = rc_check(r, b, t, "dfh_recommend_add_items");
  if (rc) return rc;
  if (r->n) {
    set_error("dfh_recommend_add_items: queries are held; the catalogue grows only before the first query or behind a reset");
    return DFH_ERR_STATE;
  }
  DFH_ARG(r->M + (uint64_t)b->nrows <= RC_MAX_ITEMS, "dfh_recommend_add_items: the catalogue holds fewer than 2^31 - 128 items");
  const size_t rows = b->nrows;
  if (rows == 0) return DFH_OK;
  dfh_ctx* c = r->ctx;
  DFH_HIP(hipSetDevice(c->device));
  r->table = t;
  r->kd = ((uint32_t)t->v.k + 1u + RC_KC - 1u) / RC_KC * RC_KC;
  rc = rc_reserve_items(r, rows);
  if (rc) return rc;
  launch_k(c, DFH_K_REC_EMBED, k_rec_embed, dim3((unsigned)grid_for_waves(rows, c)), dim3(256), 0, c->stream, rc_in(b, t), r->kd, 1,
           r->d_items + r->M * r->kd, (float*)nullptr);
  DFH_HIP(hipGetLastError());
  r->M += rows;
  return rc_batch_used(c, b);
}

int dfh_recommend_item_count(dfh_recommend* r, uint64_t* m) {
  DFH_ARG(r && m, "dfh_recommend_item_count: NULL argument");
  *m = r->M;
  return DFH_OK;
}

int dfh_recommend_append_batch(dfh_recommend* r, dfh_batch* b, dfh_table* t) {
  int rc = rc_check(r, b, t, "dfh_recommend_append_batch");
  if (rc) return rc;
  if (r->M == 0) {
    set_error("dfh_recommend_append_batch: the catalogue is empty (dfh_recommend_add_items comes first)");
    return DFH_ERR_STATE;
  }
  DFH_ARG(r->n + (uint64_t)b->nrows < RC_MAX_ROWS, "dfh_recommend_append_batch: the object holds fewer than 2^32 - 16 rows");
  const size_t rows = b->nrows;
  if (rows == 0) return DFH_OK;
  dfh_ctx* c = r->ctx;
  hipStream_t s = c->stream;
  DFH_HIP(hipSetDevice(c->device));
  const uint32_t K = r->K, kd = r->kd, nq = (uint32_t)rows, M = (uint32_t)r->M;
  const uint32_t QT = (nq + RC_T - 1) / RC_T, CT = (M + RC_T - 1) / RC_T;
  uint32_t S = (uint32_t)c->rec_split;
  if (S == 0) {   // two blocks per CU and no more (rounded DOWN: a grid a little over that runs three blocks on some CUs while the
                  // others wait; measured in profiles/recommend_ab.txt), a split no shorter than four tiles
    S = std::max(1u, 2u * (uint32_t)c->num_cu / QT);
    S = std::min(S, std::max(1u, CT / 4));
  }
  S = std::max(1u, std::min(std::min(S, CT), RC_SMAX));
  rc = rc_reserve_out(r, rows);
  if (!rc) rc = rc_workspace(r, &r->d_pq, &r->pq_cap, (size_t)QT * RC_T * kd, "the packed queries");
  if (!rc) rc = rc_workspace(r, &r->d_aq, &r->aq_cap, rows, "the queries' own logits");
  if (!rc) rc = rc_workspace(r, &r->d_part, &r->part_cap, (size_t)QT * S * RC_T * K, "the splits' partial lists");
  if (rc) return rc;
  const RcOut o = rc_arrays(r->d_out, r->cap, K, r->n);
  // the padding rows of the last query tile: zero, so that the MFMAs read finite numbers
  if (QT * RC_T > nq) DFH_HIP(hipMemsetAsync(r->d_pq + (size_t)nq * kd, 0, (size_t)(QT * RC_T - nq) * kd * sizeof(float), s));
  launch_k(c, DFH_K_REC_EMBED, k_rec_embed, dim3((unsigned)grid_for_waves(rows, c)), dim3(256), 0, s, rc_in(b, t), kd, 0, r->d_pq, r->d_aq);
  DFH_HIP(hipGetLastError());
  launch_k(c, DFH_K_REC_SWEEP, k_rec_topk, dim3(QT, S), dim3(256), (size_t)RC_T * K * sizeof(unsigned long long), s, (const float*)r->d_pq,
           (const float*)r->d_items, kd, nq, M, CT, K, r->d_part, r->d_nf);
  DFH_HIP(hipGetLastError());
  launch_k(c, DFH_K_REC_MERGE, k_rec_merge, dim3((nq + 3u) / 4u), dim3(256), 0, s, (const unsigned long long*)r->d_part, S, K, nq,
           (const float*)r->d_aq, o.item, o.logit, o.n);
  DFH_HIP(hipGetLastError());
  r->n += rows;
  r->formatted = false;
  return rc_batch_used(c, b);
}

int dfh_recommend_count(dfh_recommend* r, uint64_t* n) {
  DFH_ARG(r && n, "dfh_recommend_count: NULL argument");
  *n = r->n;
  return DFH_OK;
}

int dfh_recommend_read(dfh_recommend* r, uint32_t* n, uint32_t* items, float* logits, uint64_t* nonfinite) {
  DFH_ARG(r && nonfinite, "dfh_recommend_read: NULL argument");
  *nonfinite = 0;
  DFH_ARG(r->n == 0 || (n && items && logits), "dfh_recommend_read: NULL argument");
  hipStream_t s = r->ctx->stream;
  DFH_HIP(hipSetDevice(r->ctx->device));
  unsigned long long nf = 0;
  if (r->n) {
    const RcOut o = rc_arrays(r->d_out, r->cap, r->K, 0);
    const size_t nk = r->n * r->K;
    DFH_HIP(hipMemcpyAsync(items, o.item, nk * sizeof(uint32_t), hipMemcpyDeviceToHost, s));
    DFH_HIP(hipMemcpyAsync(logits, o.logit, nk * sizeof(float), hipMemcpyDeviceToHost, s));
    DFH_HIP(hipMemcpyAsync(n, o.n, r->n * sizeof(uint32_t), hipMemcpyDeviceToHost, s));
  }
  DFH_HIP(hipMemcpyAsync(&nf, r->d_nf, sizeof(nf), hipMemcpyDeviceToHost, s));
  DFH_HIP(hipStreamSynchronize(s));
  rc_free_retired(r);
  *nonfinite = nf;
  return DFH_OK;
}

}  // extern "C"
