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
//
// DEFINITION, "rec_precision" = 1 (read with "rec_shortlist" at dfh_recommend_create, fixed for the object's life; 0, the
// default, is everything above and none of its bits change).  A query row gets its list in three steps.
// 1. OPERANDS.  k_rec_embed is unchanged; S_r, b_r, a_q stay the fp32 quantities above.  k_rec_tobf16 writes, from P[row][kd], a
//    bf16 operand Pb[row][kb], kb = roundup(V_dim + 3, 16): columns 0 .. V_dim - 1 = S[d] rounded to nearest even; the three
//    behind them the bias in three pieces b1 = bf16(b), b2 = bf16(b - b1), b3 = bf16(b - b1 - b2) (their sum is b whenever b is
//    finite and the pieces are normal) for an item, 1, 1, 1 for a query; zeros behind.  A non-finite S or b stays non-finite (a
//    NaN keeps a mantissa bit).  The item store keeps BOTH arrays; they grow and are retired together, same capacity, same zero
//    tile.
// 2. CANDIDATES.  k_rec_cand keeps, per query, the C items with the largest s^(q, i) = sum_c Pb_q[c] Pb_i[c], accumulated in fp32
//    by v_mfma_f32_32x32x16_bf16 as one chain over c in ascending chunks of 16; ties by ascending item number (the same 64-bit
//    word).  C = "rec_shortlist", or min(64, max(16, 4 K)) when that is 0; all M items when M < C.  A non-finite s^ enters no
//    list and is counted.  No bit of the short list depends on "rec_split", the grid or the batches.
// 3. RE-RANK.  k_rec_rescore computes, for each of a query's <= C candidates, s(q, i) EXACTLY as above: the same chain of
//    v_mfma_f32_32x32x2_f32 steps over the fp32 P rows (per 8 d: {d, d + 4}, {d + 1, d + 5}, ..), the bias column included, so a
//    (q, i) pair gets the same bits from either precision; keeps the K largest under the order above and hands out a_q + s.  A
//    non-finite s is dropped and counted.  THE COUNT is: pairs whose s^ is not finite (never candidates), plus candidate pairs
//    whose s is not finite; the two sets are disjoint, no pair is counted twice.  (A pair with a finite s^ and a non-finite s
//    that is not a candidate is not counted.)
// GUARANTEES.  Every (item, logit) handed out has the fp32 path's logit for that pair, bit for bit.  The list is the exact top K
// of the short list; it IS the fp32 path's list whenever that list's items all reach the short list.  When every S is a bf16
// number, every b three bf16 pieces and every partial sum exact in fp32, s^ = s and the whole output equals the fp32 path's.
//
//   k_rec_tobf16  a thread per (row, 8 columns): one 16 B store.  Rows behind the batch's (a query tile's padding) become zero.
//   k_rec_cand    k_rec_topk's blocking with one MFMA per 32x32 block and chunk of 16 columns: the staging geometry is the same
//                 in BYTES (a chunk is 32 B of a row, row stride 48 B, a lane's fragment for one K-step = 8 consecutive bf16 of
//                 one row = one conflict-free ds_read_b128; double-buffered).  The MFMA work per tile is a tenth of fp32's, so
//                 the selection sets the pace; it differs from k_rec_topk's in two ways: a lane holds the thresholds of its 16
//                 rows in REGISTERS (refreshed only by the insertion that moves them: an insertion's row belongs to one h and
//                 one r), and a whole 32x32 block is skipped by ONE ballot over "any of my 16 reaches its threshold or is not
//                 finite".  A row's list of C words still belongs to one wave: no barrier, no atomic.  Query tile 128 rows, lists
//                 128 C 8 B of dynamic LDS behind 24 576 B of staging: C <= 40 fits two workgroups per CU (65 536 B each), a
//                 longer list one (90 112 B at C = 64); resources in DESIGN section 4.
//   k_rec_rescore a wave per query row: merges the S partial candidate lists (lane l: candidate l), then one or two 32x32 MFMA
//                 blocks whose 32 rows are all the query and whose columns are candidates 0 .. 31 / 32 .. 63, operands straight
//                 from HBM (no LDS); lane l reads its candidate's s from element 0 of block l / 32.  Mostly idle MFMA lanes,
//                 accepted: R C kd work.  Rank = the number of larger words among the <= 64; rank < K stores.
// Timed as DFH_K_REC_CONVERT / _CAND / _RESCORE.

struct dfh_recommend {
  dfh_ctx* ctx = nullptr;
  uint32_t K = 0, kd = 0;
  uint32_t bf16 = 0, C = 0, kb = 0;  // "rec_precision" at creation; the short list's length; Pb's row length
  uint16_t* d_items_b = nullptr;     // [(items_cap + 128) * kb]: the items' bf16 operand (bf16 only)
  uint16_t* d_pqb = nullptr;         // the appended minibatch's bf16 queries
  size_t pqb_cap = 0;
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

// ---------------------------------------------------------------- "rec_precision" = 1
constexpr uint32_t RC_KB = 16, RC_CMAX = 64;
typedef __bf16 rc_bf8 __attribute__((ext_vector_type(8)));

__device__ __forceinline__ uint32_t rc_bf16(float f) {   // round to nearest even; Inf stays Inf, a NaN keeps a mantissa bit
  const uint32_t u = __float_as_uint(f);
  if ((u & 0x7FFFFFFFu) > 0x7F800000u) return (u >> 16) | 0x40u;
  return (u + 0x7FFFu + ((u >> 16) & 1u)) >> 16;
}
__device__ __forceinline__ float rc_bf16_value(uint32_t h) { return __uint_as_float(h << 16); }

// P[rows][kd] -> Pb[total][kb], total >= rows: the rows behind `rows` become zero.  A thread per (row, 8 columns).
__global__ void __launch_bounds__(256) k_rec_tobf16(const float* __restrict__ P, uint32_t kd, uint32_t k, uint32_t kb, uint32_t rows,
                                                    uint32_t total, int is_item, uint16_t* __restrict__ Pb) {
  const uint32_t G = kb / 8u;
  const uint64_t n = (uint64_t)total * G;
  for (uint64_t e = (uint64_t)blockIdx.x * 256u + threadIdx.x; e < n; e += (uint64_t)gridDim.x * 256u) {
    const uint32_t row = (uint32_t)(e / G), c0 = 8u * (uint32_t)(e % G);
    uint32_t hv[8] = {0u, 0u, 0u, 0u, 0u, 0u, 0u, 0u};
    if (row < rows && c0 < k + 3u) {
      const float* const p = P + (size_t)row * kd;
      uint32_t piece[3] = {0x3F80u, 0x3F80u, 0x3F80u};   // 1.0
      if (is_item && c0 + 8u > k) {
        float b = p[k];
        for (int j = 0; j < 3; ++j) {
          piece[j] = rc_bf16(b);
          b -= rc_bf16_value(piece[j]);
        }
      }
#pragma unroll
      for (uint32_t j = 0; j < 8u; ++j) {
        const uint32_t c = c0 + j;
        if (c < k) hv[j] = rc_bf16(p[c]);
        else if (c < k + 3u) hv[j] = c == k ? piece[0] : c == k + 1u ? piece[1] : piece[2];
      }
    }
    uint4 o;
    o.x = hv[0] | (hv[1] << 16);
    o.y = hv[2] | (hv[3] << 16);
    o.z = hv[4] | (hv[5] << 16);
    o.w = hv[6] | (hv[7] << 16);
    *reinterpret_cast<uint4*>(Pb + (size_t)row * kb + c0) = o;
  }
}

// grid (query tiles, S), as k_rec_topk; dynamic LDS: RC_T * C * 8 bytes.  A: roundup(nq, 128) bf16 query rows; B: the items' bf16
// array.  Out: part[(tile x, split y)][128][C], descending, 0: empty.
__global__ void __launch_bounds__(256, 2) k_rec_cand(const uint16_t* __restrict__ A, const uint16_t* __restrict__ B, uint32_t kb, uint32_t nq,
                                                     uint32_t M, uint32_t CT, uint32_t C, unsigned long long* __restrict__ part,
                                                     unsigned long long* __restrict__ nonfinite) {
  __shared__ __attribute__((aligned(16))) uint32_t s_stage[2][2][RC_T * RC_LS];   // [buffer][queries | items], 48 B per row
  extern __shared__ __attribute__((aligned(16))) unsigned long long s_list[];     // [RC_T][C], descending, 0: empty
  const uint32_t tid = threadIdx.x, lane = tid & 63u, wave = tid >> 6, h = lane >> 5, li = lane & 31u;
  const uint32_t S = gridDim.y, y = blockIdx.y;
  const uint32_t t0 = (uint32_t)((uint64_t)y * CT / S), t1 = (uint32_t)((uint64_t)(y + 1) * CT / S);
  const uint32_t qbase = blockIdx.x * RC_T, wrow0 = wave * 32u;
  const uint32_t NC = kb / RC_KB, total = (t1 - t0) * NC;
  for (uint32_t i = lane; i < 32u * C; i += 64u) s_list[(size_t)wrow0 * C + i] = 0ull;
  // element r of a block is row wrow0 + 8 (r / 4) + 4 h + r % 4: the thresholds of this lane's 16 rows (the C-th score; -inf while
  // the list is short, +inf for a padding row)
  float thr[16];
#pragma unroll
  for (int r = 0; r < 16; ++r) thr[r] = qbase + wrow0 + 8u * (r >> 2) + 4u * h + (r & 3u) < nq ? -__builtin_inff() : __builtin_inff();
  // staging: thread -> (row tid / 2, the 8 bf16 of half tid % 2) of both operands
  const uint32_t lr = tid >> 1, lq = tid & 1u;
  const uint16_t* const gA = A + (size_t)(qbase + lr) * kb + 8u * lq;
  const uint16_t* const gB = B + (size_t)lr * kb + 8u * lq;
  const uint32_t st_at = lr * RC_LS + 4u * lq;
  uint4 ra = make_uint4(0u, 0u, 0u, 0u), rb = ra;
  if (total) {
    ra = *reinterpret_cast<const uint4*>(gA);
    rb = *reinterpret_cast<const uint4*>(gB + (size_t)t0 * RC_T * kb);
    *reinterpret_cast<uint4*>(&s_stage[0][0][st_at]) = ra;
    *reinterpret_cast<uint4*>(&s_stage[0][1][st_at]) = rb;
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
      ra = *reinterpret_cast<const uint4*>(gA + nch * RC_KB);
      rb = *reinterpret_cast<const uint4*>(gB + (size_t)ntile * RC_T * kb + nch * RC_KB);
    }
    if (ch == 0) {
#pragma unroll
      for (int c = 0; c < 4; ++c)
#pragma unroll
        for (int r = 0; r < 16; ++r) acc[c][r] = 0.f;
    }
    {
      // a lane's fragment: columns 8 h .. 8 h + 7 of the chunk, of query row li / of item 32 c + li
      const rc_bf8 a = __builtin_bit_cast(rc_bf8, *reinterpret_cast<const uint4*>(&s_stage[buf][0][(wrow0 + li) * RC_LS + 4u * h]));
#pragma unroll
      for (int c = 0; c < 4; ++c) {
        const rc_bf8 b = __builtin_bit_cast(rc_bf8, *reinterpret_cast<const uint4*>(&s_stage[buf][1][(c * 32u + li) * RC_LS + 4u * h]));
        acc[c] = __builtin_amdgcn_mfma_f32_32x32x16_bf16(a, b, acc[c], 0, 0, 0);
      }
    }
    if (ch + 1 == NC) {   // the tile is complete: element r of block c is (row 8 (r / 4) + 4 h + r % 4, item 32 c + li)
      const uint32_t cbase = tile * RC_T;
#pragma unroll
      for (int c = 0; c < 4; ++c) {
        bool any = false;
#pragma unroll
        for (int r = 0; r < 16; ++r) any |= !(acc[c][r] < thr[r]) | !pr_finite(acc[c][r]);
        if (__ballot(any) == 0ull) continue;   // no lane has anything for its rows in this block
#pragma unroll
        for (int r = 0; r < 16; ++r) {
          const float s = acc[c][r];
          const uint32_t rr = wrow0 + 8u * (r >> 2) + (r & 3u);
          unsigned long long m = __ballot(!(s < thr[r]) || !pr_finite(s));
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
            unsigned long long* const L = s_list + (size_t)qr * C;
            const unsigned long long v = lane < C ? L[lane] : 0ull;
            const uint32_t p = (uint32_t)__popcll(__ballot(lane < C && v > w64));   // the entries that stay in front
            if (p >= C) continue;
            if (lane >= p && lane + 1 < C) L[lane + 1] = v;
            if (lane == p) L[p] = w64;
            pr_wave_sync();   // other lanes' stores, before the C-th is read
            const unsigned long long last = L[C - 1];
            if (last != 0ull && h == (src >> 5)) thr[r] = pr_key_of((uint32_t)(last >> 32));   // row qr is element r of the lanes of that h
            pr_wave_sync();   // the list, before the next element's reads
          }
        }
      }
    }
    if (more) {
      *reinterpret_cast<uint4*>(&s_stage[buf ^ 1u][0][st_at]) = ra;
      *reinterpret_cast<uint4*>(&s_stage[buf ^ 1u][1][st_at]) = rb;
    }
    __syncthreads();
    tile = ntile;
    ch = nch;
  }
  unsigned long long* const out = part + ((size_t)blockIdx.x * S + y) * RC_T * C;
  for (uint32_t i = tid; i < RC_T * C; i += 256u) out[i] = s_list[i];
  if (nf && lane == 0) atomicAdd(nonfinite, (unsigned long long)nf);
}

// a wave per query row of the append.  Pq: the fp32 queries [nq][kd]; Pi: the fp32 item store.
__global__ void __launch_bounds__(256) k_rec_rescore(const unsigned long long* __restrict__ part, uint32_t S, uint32_t C, uint32_t K, uint32_t nq,
                                                     const float* __restrict__ Pq, const float* __restrict__ Pi, uint32_t kd,
                                                     const float* __restrict__ aq, uint32_t* __restrict__ o_item, float* __restrict__ o_logit,
                                                     uint32_t* __restrict__ o_n, unsigned long long* __restrict__ nonfinite) {
  const uint32_t lane = threadIdx.x & 63u, h = lane >> 5, li = lane & 31u;
  const uint32_t q = blockIdx.x * 4u + (threadIdx.x >> 6);
  if (q >= nq) return;
  unsigned long long v = 0ull;   // lane l < C: entry l of the merged short list (k_rec_merge's loop)
  for (uint32_t y = 0; y < S; ++y) {
    const unsigned long long* const L = part + (((size_t)(q / RC_T) * S + y) * RC_T + q % RC_T) * C;
    for (uint32_t j = 0; j < C; ++j) {
      const unsigned long long w64 = L[j];
      if (w64 == 0ull) break;
      const uint32_t p = (uint32_t)__popcll(__ballot(lane < C && v > w64));
      if (p >= C) break;   // the rest of this list is smaller still
      const uint32_t lo = (uint32_t)__shfl_up((int)(uint32_t)v, 1, 64), hi = (uint32_t)__shfl_up((int)(uint32_t)(v >> 32), 1, 64);
      if (lane == p) v = w64;
      else if (lane > p) v = ((unsigned long long)hi << 32) | lo;
    }
  }
  if (lane >= C) v = 0ull;   // (the shifts ran past the list's end)
  const uint32_t cnt = (uint32_t)__popcll(__ballot(v != 0ull));   // candidates 0 .. cnt - 1, in lanes 0 .. cnt - 1
  const uint32_t item = v != 0ull ? 0x7FFFFFFFu - (uint32_t)v : 0u;
  // block 0: columns = candidates 0 .. 31, block 1: 32 .. 63; all 32 rows are the query.  k_rec_topk's chain: per 8 d four steps,
  // half h supplying d = 8 ch + 4 h + {0, 1, 2, 3}
  const bool two = cnt > 32u, has0 = li < cnt, has1 = 32u + li < cnt;
  const float* const ga = Pq + (size_t)q * kd + 4u * h;
  const float* const g0 = Pi + (size_t)(uint32_t)__shfl((int)item, (int)li, 64) * kd + 4u * h;
  const float* const g1 = Pi + (size_t)(uint32_t)__shfl((int)item, (int)(32u + li), 64) * kd + 4u * h;
  pr_f16 acc0, acc1;
#pragma unroll
  for (int r = 0; r < 16; ++r) acc0[r] = acc1[r] = 0.f;
  const float4 zero = make_float4(0.f, 0.f, 0.f, 0.f);
  for (uint32_t d = 0; d < kd; d += RC_KC) {
    const float4 a = ld4(ga + d), b0 = has0 ? ld4(g0 + d) : zero;
    acc0 = __builtin_amdgcn_mfma_f32_32x32x2f32(a.x, b0.x, acc0, 0, 0, 0);
    acc0 = __builtin_amdgcn_mfma_f32_32x32x2f32(a.y, b0.y, acc0, 0, 0, 0);
    acc0 = __builtin_amdgcn_mfma_f32_32x32x2f32(a.z, b0.z, acc0, 0, 0, 0);
    acc0 = __builtin_amdgcn_mfma_f32_32x32x2f32(a.w, b0.w, acc0, 0, 0, 0);
    if (two) {   // wave-uniform
      const float4 b1 = has1 ? ld4(g1 + d) : zero;
      acc1 = __builtin_amdgcn_mfma_f32_32x32x2f32(a.x, b1.x, acc1, 0, 0, 0);
      acc1 = __builtin_amdgcn_mfma_f32_32x32x2f32(a.y, b1.y, acc1, 0, 0, 0);
      acc1 = __builtin_amdgcn_mfma_f32_32x32x2f32(a.z, b1.z, acc1, 0, 0, 0);
      acc1 = __builtin_amdgcn_mfma_f32_32x32x2f32(a.w, b1.w, acc1, 0, 0, 0);
    }
  }
  float s = h ? acc1[0] : acc0[0];   // element 0 of lane (h, li): (row 4 h, column li) of its block: candidate `lane`
  const bool held = lane < cnt, fin = pr_finite(s);
  const uint32_t nf = (uint32_t)__popcll(__ballot(held && !fin));
  if (nf && lane == 0) atomicAdd(nonfinite, (unsigned long long)nf);
  if (s == 0.f) s = 0.f;   // -0 and +0: one key
  const unsigned long long w = held && fin ? ((unsigned long long)pr_orderable(s) << 32) | (unsigned long long)(0x7FFFFFFFu - item) : 0ull;
  uint32_t rank = 0;   // the words are distinct (the items are): the number of larger ones
  for (uint32_t j = 0; j < cnt; ++j) {
    const uint32_t lo = (uint32_t)__shfl((int)(uint32_t)w, (int)j, 64), hi = (uint32_t)__shfl((int)(uint32_t)(w >> 32), (int)j, 64);
    rank += (((unsigned long long)hi << 32) | lo) > w;
  }
  const uint32_t len = min(K, (uint32_t)__popcll(__ballot(w != 0ull)));
  if (lane == 0) o_n[q] = len;
  if (w != 0ull && rank < K) {
    o_item[(size_t)q * K + rank] = item;
    o_logit[(size_t)q * K + rank] = aq[q] + s;
  }
  if (lane >= len && lane < K) {
    o_item[(size_t)q * K + lane] = 0u;
    o_logit[(size_t)q * K + lane] = 0.f;
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
  uint16_t* nb = nullptr;   // the bf16 operand beside it ("rec_precision" = 1): same rows, same zero tile
  const size_t bytes = (cap + RC_T) * r->kd * sizeof(float), bbytes = r->bf16 ? (cap + RC_T) * r->kb * sizeof(uint16_t) : 0;
  if (hipMalloc((void**)&nv, bytes) != hipSuccess || (bbytes && hipMalloc((void**)&nb, bbytes) != hipSuccess)) {
    (void)hipGetLastError();
    if (nv) (void)hipFree(nv);
    set_error("dfh_recommend_add_items: no device memory for " + std::to_string(cap) + " items (" + std::to_string(bytes + bbytes) +
              " bytes needed)");
    return DFH_ERR_CAPACITY;
  }
  hipStream_t s = r->ctx->stream;
  hipError_t er = hipMemsetAsync(nv, 0, bytes, s);
  if (er == hipSuccess && r->M) er = hipMemcpyAsync(nv, r->d_items, r->M * r->kd * sizeof(float), hipMemcpyDeviceToDevice, s);
  if (er == hipSuccess && nb) er = hipMemsetAsync(nb, 0, bbytes, s);
  if (er == hipSuccess && nb && r->M) er = hipMemcpyAsync(nb, r->d_items_b, r->M * r->kb * sizeof(uint16_t), hipMemcpyDeviceToDevice, s);
  if (er != hipSuccess) {
    r->retired.push_back(nv);
    if (nb) r->retired.push_back(nb);
    set_error(std::string("dfh_recommend_add_items: ") + hipGetErrorString(er));
    return DFH_ERR_HIP;
  }
  if (r->d_items) r->retired.push_back(r->d_items);
  if (r->d_items_b) r->retired.push_back(r->d_items_b);
  r->d_items = nv;
  r->d_items_b = nb;
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

unsigned rc_tobf16_grid(size_t rows, uint32_t kb, const dfh_ctx* c) {
  const size_t blocks = (rows * (kb / 8u) + 255) / 256;
  return (unsigned)std::max<size_t>(1, std::min(blocks, (size_t)c->num_cu * 8));
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
  DFH_ARG(!(ctx->rec_precision == 1 && ctx->rec_shortlist > 0 && ctx->rec_shortlist < topk),
          "dfh_recommend_create: rec_precision = 1 with rec_shortlist = " + std::to_string(ctx->rec_shortlist) + " below topk = " +
              std::to_string(topk) + ": the short list holds the candidates of the topk (0: min(64, max(16, 4 topk)))");
  dfh_recommend* r = new (std::nothrow) dfh_recommend();
  if (!r) {
    set_error("dfh_recommend_create: out of host memory (" + std::to_string(sizeof(dfh_recommend)) + " bytes needed)");
    return DFH_ERR_CAPACITY;
  }
  r->ctx = ctx;
  r->K = (uint32_t)topk;
  r->hint = capacity_hint;
  r->bf16 = (uint32_t)ctx->rec_precision;
  r->C = ctx->rec_shortlist ? (uint32_t)ctx->rec_shortlist : std::min(RC_CMAX, std::max(16u, 4u * r->K));
  hipError_t er = hipSetDevice(ctx->device);
  // k_rec_cand's lists behind its staging pass 64 KB of LDS from C = 41 on
  if (er == hipSuccess && r->bf16)
    er = hipFuncSetAttribute(reinterpret_cast<const void*>(k_rec_cand), hipFuncAttributeMaxDynamicSharedMemorySize,
                             (int)(RC_T * RC_CMAX * sizeof(unsigned long long)));
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
  if (r->d_items_b) (void)hipFree(r->d_items_b);
  if (r->d_pqb) (void)hipFree(r->d_pqb);
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
  r->kb = ((uint32_t)t->v.k + 3u + RC_KB - 1u) / RC_KB * RC_KB;
  rc = rc_reserve_items(r, rows);
  if (rc) return rc;
  launch_k(c, DFH_K_REC_EMBED, k_rec_embed, dim3((unsigned)grid_for_waves(rows, c)), dim3(256), 0, c->stream, rc_in(b, t), r->kd, 1,
           r->d_items + r->M * r->kd, (float*)nullptr);
  DFH_HIP(hipGetLastError());
  if (r->bf16) {
    launch_k(c, DFH_K_REC_CONVERT, k_rec_tobf16, dim3(rc_tobf16_grid(rows, r->kb, c)), dim3(256), 0, c->stream,
             (const float*)(r->d_items + r->M * r->kd), r->kd, (uint32_t)t->v.k, r->kb, (uint32_t)rows, (uint32_t)rows, 1,
             r->d_items_b + r->M * r->kb);
    DFH_HIP(hipGetLastError());
  }
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
  if (!rc) rc = rc_workspace(r, &r->d_part, &r->part_cap, (size_t)QT * S * RC_T * (r->bf16 ? r->C : K), "the splits' partial lists");
  if (!rc && r->bf16) rc = rc_workspace(r, &r->d_pqb, &r->pqb_cap, (size_t)QT * RC_T * r->kb, "the packed bf16 queries");
  if (rc) return rc;
  const RcOut o = rc_arrays(r->d_out, r->cap, K, r->n);
  if (r->bf16) {   // embed, convert (which zeroes the last tile's padding rows), candidate sweep, re-rank
    const uint32_t kb = r->kb, C = r->C;
    launch_k(c, DFH_K_REC_EMBED, k_rec_embed, dim3((unsigned)grid_for_waves(rows, c)), dim3(256), 0, s, rc_in(b, t), kd, 0, r->d_pq, r->d_aq);
    DFH_HIP(hipGetLastError());
    launch_k(c, DFH_K_REC_CONVERT, k_rec_tobf16, dim3(rc_tobf16_grid((size_t)QT * RC_T, kb, c)), dim3(256), 0, s, (const float*)r->d_pq, kd,
             (uint32_t)t->v.k, kb, nq, QT * RC_T, 0, r->d_pqb);
    DFH_HIP(hipGetLastError());
    launch_k(c, DFH_K_REC_CAND, k_rec_cand, dim3(QT, S), dim3(256), (size_t)RC_T * C * sizeof(unsigned long long), s,
             (const uint16_t*)r->d_pqb, (const uint16_t*)r->d_items_b, kb, nq, M, CT, C, r->d_part, r->d_nf);
    DFH_HIP(hipGetLastError());
    launch_k(c, DFH_K_REC_RESCORE, k_rec_rescore, dim3((nq + 3u) / 4u), dim3(256), 0, s, (const unsigned long long*)r->d_part, S, C, K, nq,
             (const float*)r->d_pq, (const float*)r->d_items, kd, (const float*)r->d_aq, o.item, o.logit, o.n, r->d_nf);
    DFH_HIP(hipGetLastError());
    r->n += rows;
    r->formatted = false;
    return rc_batch_used(c, b);
  }
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
