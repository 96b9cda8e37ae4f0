// dfh_explain.hip — each row's strongest FM interaction pairs (included behind dfh_pairs.hip, whose order helpers it uses;
// explain_out of task = predict).
//
// DEFINITION.  The logit of a row is sum_j x_j w_j + sum_{i<j} c_ij with c_ij = x_i x_j <V_i, V_j> over the POSITIONS i < j of
// the row whose key has V (kHasV in uw[index[j]].x, the forward's rule; a missing value array means x = 1).  A pair is formed
// between positions, not between distinct keys: a key that occurs twice in a row pairs with itself, as the formula the forward
// evaluates counts it.  c_ij is computed in fp32 as sum_d (x_i V_id)(x_j V_jd): fp32 products, fp32 accumulation over d.  A row
// gets the K pairs with the largest key, |c| for by = DFH_PAIRS_ABS and c for DFH_PAIRS_POS (+0 and -0 are one key): key
// descending, equal keys by ascending (i, j) in the row's own position numbering; all of them when the row has fewer.
// inter[r] = sum_{i<j} c_ij over ALL pairs of the row, summed in fp32 from the same tiles (not through the forward's
// (XV)^2 - XXVV identity, which cancels).  A pair whose c is not finite enters no list and is left out of inter; such pairs are
// counted.  A row with fewer than two has-V positions gets an empty list and inter = 0.
//
// k_explain, 256 threads: ONE WAVE OWNS ONE ROW (a block holds four, rows taken grid-stride), so a row's list belongs to one
// wave and nothing in the kernel needs a block barrier or an atomic but the non-finite count.
//   compaction   the row is walked 64 positions at a time; ballot and prefix number the has-V positions 0 .. P - 1, and the
//                position of number c goes to cpos[offset[r] + c] (a workspace of the call, 4 B per nonzero of the minibatch),
//                read back by the same wave behind a fence.  The has-V positions are cut into PANELS of 32.
//   units        NP panels: the work is the panel pairs (pa, pb), pa < pb, each a 32 x 32 Gram tile A B^T on
//                v_mfma_f32_32x32x2_f32.  The diagonal tile A A^T rides in the unit (pa, pa + 1) and the last panel's B B^T in
//                the unit (NP - 2, NP - 1): three accumulator tiles (48 registers) over ONE staging of two panels.  So a row of
//                up to 64 has-V positions (the Criteo shape: 39) is one unit and gathers each V row from the table exactly
//                once; a longer row takes a panel through LDS once per unit it is part of, from L2 after the first.  NP = 1:
//                one unit with A A^T alone.
//   staging      lanes 0-31 hold {table row, x, position} of panel A's slots, lanes 32-63 panel B's.  V goes through LDS in
//                chunks of 16 floats of d: 64 rows x 4 float4 = four 16 B loads per lane, four consecutive lanes on one row's
//                64 B; all four are issued before any is used, and chunk t + 1's are in flight while chunk t's MFMAs run.  The
//                lane scales what it loaded by the row's x (c_ij = <x_i V_i, x_j V_j>; the accumulators need no pass of their
//                own) and zeroes what lies beyond V_dim or belongs to no position: 0 * 0 adds an exact 0.
//   LDS          per wave two panels [32][20 floats]: 5 120 B, whatever V_dim and the row's length.  Row stride 20 floats =
//                16 + 4: a lane reads its row's 8 floats of its half (two ds_read_b128 at 80 row + 32 h bytes); 16 consecutive
//                rows start at 16 distinct multiples of 4 banks (20 r mod 64, 5 odd), so the reads are free of bank conflicts.
//                Plus the list (32 x 12 B) and the slots' positions (256 B) per wave: 23 040 B per block.
//   selection    when a unit's tiles are complete, a lane filters its 16 accumulators per tile against the wave's current K-th
//                key (a register; -inf while the list is short); on a diagonal tile only row < column counts.  The survivors
//                (and non-finite elements) are taken one at a time as in k_pairs_topk: counted if not finite, else inserted
//                by the whole wave into the sorted list in LDS — lane e holds entry e, a ballot gives the place, the tail
//                moves up one.  An entry is the 64-bit word {orderable key : 2^32 - 1 - i} and the 32-bit word
//                {2^31 - 1 - j : sign of c}: 96 bits, because (i, j) of a row of any length does not fit the 31 bits a
//                dump's position has; compared as a pair, the order IS the composite order.  (A row holds fewer than 2^31
//                positions.)
//   out          n, K x {position i, position j, c, printed id i, printed id j} with zeros behind n, inter.  The printed id
//                is reverse_bytes(feaids[index[position]]), as task = dump dump_ids = feature prints it.
// Plain C++, vector stores, no scratch.  Timed as DFH_K_EXPLAIN.

struct dfh_explain {
  dfh_ctx* ctx = nullptr;
  uint32_t K = 0;
  int by = 0;
  size_t cap = 0, n = 0, hint = 0;   // rows the arrays hold / appended since the last reset / of the first allocation
  char* d_out = nullptr;             // one allocation: the seven arrays of ExOut for cap rows
  std::vector<void*> retired;        // arrays a growth replaced: kernels and copies on them may still be queued, freed behind the next wait
  uint32_t* d_cpos = nullptr;        // [cpos_cap] the compaction's workspace: one append's kernel after another uses it, in stream order
  size_t cpos_cap = 0;
  unsigned long long* d_nf = nullptr;   // non-finite pairs since the last reset
  TextWork text;                        // the workspace of dfh_explain_format (dfh_listtext.hip over dfh_textout.hip)
  bool formatted = false;               // text holds the lines of everything appended
};

namespace {
constexpr uint32_t EX_P = 32, EX_KC = 16, EX_LS = 20;   // positions per panel; floats of d per staged chunk; LDS row stride in floats
constexpr uint32_t EX_KMAX = 32, EX_WAVES = 4;
constexpr uint64_t EX_MAX_ROWS = 0xFFFFFFF0ULL;

struct ExIn {
  const uint32_t* offset;
  const uint32_t* index;
  const float* value;     // or NULL: x = 1
  const uint2* uw;        // {table row | flags, w} per key of the minibatch (the step's lookup)
  const uint64_t* feaids;
  const float* va;        // the table's rows: [V[0 .. kp) | accumulators[0 .. kp)]
  uint32_t nrows, k, kp;
};
struct ExOut {   // row r of this call at index r (the host hands the arrays in at the object's row count)
  uint64_t *ids_i, *ids_j;   // [K] per row
  float* c;                  // [K]
  uint32_t *pos_i, *pos_j;   // [K]
  uint32_t* n;
  float* inter;
};
inline size_t ex_row_bytes(uint32_t K) { return (size_t)K * (2 * sizeof(uint64_t) + sizeof(float) + 2 * sizeof(uint32_t)) + 2 * sizeof(uint32_t); }
inline ExOut ex_arrays(char* base, size_t cap, uint32_t K, size_t at) {   // 8 B arrays first
  ExOut o;
  uint64_t* p8 = reinterpret_cast<uint64_t*>(base);
  o.ids_i = p8 + at * K;
  o.ids_j = p8 + cap * K + at * K;
  uint32_t* p4 = reinterpret_cast<uint32_t*>(p8 + 2 * cap * K);
  o.c = reinterpret_cast<float*>(p4) + at * K;
  o.pos_i = p4 + cap * K + at * K;
  o.pos_j = p4 + 2 * cap * K + at * K;
  o.n = p4 + 3 * cap * K + at;
  o.inter = reinterpret_cast<float*>(p4 + 3 * cap * K + cap) + at;
  return o;
}

// a wave's selection state: the list in LDS, the K-th key, the row's sums (nf is the same in every lane, inter is per lane)
struct ExSel {
  unsigned long long* hi;
  uint32_t* lo;
  float thr, inter;
  uint32_t nf, K;
  int by_pos;
};

// one complete tile: element r of a lane is (slot 8 (r / 4) + 4 h + r % 4 of the row panel, slot li of the column panel)
__device__ __forceinline__ void ex_select(const pr_f16& acc, const uint32_t* posR, const uint32_t* posC, uint32_t nR, uint32_t nC, bool diag,
                                          ExSel& s, uint32_t lane) {
  const uint32_t h = lane >> 5, li = lane & 31u, K = s.K;
#pragma unroll
  for (int r = 0; r < 16; ++r) {
    const float v = acc[r];
    const uint32_t row = 8u * (r >> 2) + 4u * h + (r & 3u);
    const bool ok = row < nR && li < nC && (!diag || row < li), fin = pr_finite(v);
    if (ok && fin) s.inter += v;
    unsigned long long m = __ballot(ok && (!fin || (s.by_pos ? v : fabsf(v)) >= s.thr));
    while (m) {   // wave-uniform from here on
      const uint32_t src = (uint32_t)__ffsll((long long)m) - 1u;
      m &= m - 1ull;
      const float sv = __shfl(v, (int)src, 64);
      if (!pr_finite(sv)) {
        ++s.nf;
        continue;
      }
      const uint32_t pi = posR[8u * (r >> 2) + 4u * (src >> 5) + (r & 3u)], pj = posC[src & 31u];
      float kf = s.by_pos ? sv : fabsf(sv);
      if (kf == 0.f) kf = 0.f;   // -0 and +0: one key
      const uint32_t sign = s.by_pos ? 0u : (__float_as_uint(sv) >> 31);
      const unsigned long long whi = ((unsigned long long)pr_orderable(kf) << 32) | (unsigned long long)(0xFFFFFFFFu - pi);
      const uint32_t wlo = ((0x7FFFFFFFu - pj) << 1) | sign;
      const unsigned long long vh = lane < K ? s.hi[lane] : 0ull;
      const uint32_t vl = lane < K ? s.lo[lane] : 0u;
      const uint32_t p = (uint32_t)__popcll(__ballot(lane < K && (vh > whi || (vh == whi && vl > wlo))));   // the entries that stay in front
      if (p >= K) continue;
      if (lane >= p && lane + 1 < K) {
        s.hi[lane + 1] = vh;
        s.lo[lane + 1] = vl;
      }
      if (lane == p) {
        s.hi[p] = whi;
        s.lo[p] = wlo;
      }
      pr_wave_sync();   // other lanes' stores, before the K-th is read
      const unsigned long long last = s.hi[K - 1];
      if (last != 0ull) s.thr = pr_key_of((uint32_t)(last >> 32));
      pr_wave_sync();   // the list, before the next element's reads
    }
  }
}

__global__ void __launch_bounds__(256) k_explain(ExIn in, uint32_t K, int by_pos, uint32_t* __restrict__ cpos, ExOut out,
                                                 unsigned long long* __restrict__ nonfinite) {
  __shared__ __attribute__((aligned(16))) float s_pan[EX_WAVES][2 * EX_P * EX_LS];   // [panel A | panel B][slot][EX_LS]
  __shared__ unsigned long long s_hi[EX_WAVES][EX_KMAX];                             // the list, descending; 0: empty
  __shared__ uint32_t s_lo[EX_WAVES][EX_KMAX];
  __shared__ uint32_t s_pos[EX_WAVES][2 * EX_P];                                     // the slots' positions in the row
  const uint32_t lane = threadIdx.x & 63u, wave = threadIdx.x >> 6, h = lane >> 5, li = lane & 31u, f4 = lane & 3u;
  float* const pan = s_pan[wave];
  uint32_t* const spos = s_pos[wave];
  const uint32_t k = in.k, kp = in.kp, NC = (k + EX_KC - 1) / EX_KC;
  uint32_t nf_all = 0;
  for (uint32_t row = blockIdx.x * EX_WAVES + wave; row < in.nrows; row += gridDim.x * EX_WAVES) {
    const uint32_t beg = in.offset[row], end = in.offset[row + 1];
    uint32_t P = 0;   // the row's has-V positions
    for (uint32_t base = beg; base < end; base += min(64u, end - base)) {
      const uint32_t j = base + lane;
      const bool hv = j < end && (in.uw[in.index[j]].x & kHasV) != 0u;
      const unsigned long long m = __ballot(hv);
      if (hv) cpos[beg + P + (uint32_t)__popcll(m & ((1ull << lane) - 1ull))] = j - beg;
      P += (uint32_t)__popcll(m);
    }
    __threadfence();   // the wave reads back what other lanes of it stored
    if (lane < K) {
      s_hi[wave][lane] = 0ull;
      s_lo[wave][lane] = 0u;
    }
    pr_wave_sync();
    ExSel sel{s_hi[wave], s_lo[wave], -__builtin_inff(), 0.f, 0u, K, by_pos};
    const uint32_t NP = (P + EX_P - 1) / EX_P, lastA = NP > 1 ? NP - 2 : 0;
    for (uint32_t pa = 0; P >= 2 && pa <= lastA; ++pa) {
      for (uint32_t pb = NP > 1 ? pa + 1 : 0; pb < NP; ++pb) {
        const bool useB = pb != pa, doAA = !useB || pb == pa + 1, doBB = useB && pa == lastA && pb + 1 == NP;
        const uint32_t nA = min(EX_P, P - EX_P * pa), nB = useB ? min(EX_P, P - EX_P * pb) : 0u;
        // the slots: lanes 0-31 panel A's, lanes 32-63 panel B's
        const uint32_t ci = EX_P * (h ? pb : pa) + li;
        const bool valid = li < (h ? nB : nA);
        uint32_t mrow = 0, mpos = 0;
        float mx = 0.f;
        if (valid) {
          mpos = cpos[beg + ci];
          mrow = in.uw[in.index[beg + mpos]].x & kRowMask;
          mx = in.value ? in.value[beg + mpos] : 1.f;
        }
        spos[lane] = mpos;
        // staging: load q of a lane is the float4 f4 of slot 16 q + lane / 4
        const float* rp[4];
        float rx[4];
#pragma unroll
        for (int q = 0; q < 4; ++q) {
          const int rs = 16 * q + (int)(lane >> 2);
          const uint32_t rr = (uint32_t)__shfl((int)mrow, rs, 64);
          rx[q] = __shfl(mx, rs, 64);
          rp[q] = __shfl((int)valid, rs, 64) ? in.va + (size_t)rr * (2 * kp) + 4 * f4 : nullptr;
        }
        auto load = [&](uint32_t t, float4* v) {
          const uint32_t d = EX_KC * t + 4 * f4;
#pragma unroll
          for (int q = 0; q < 4; ++q) v[q] = (rp[q] && d < kp) ? ld4(rp[q] + EX_KC * t) : make_float4(0.f, 0.f, 0.f, 0.f);
        };
        float4 cur[4];
        load(0, cur);
        pr_f16 aa, ab, bb;
#pragma unroll
        for (int r = 0; r < 16; ++r) aa[r] = ab[r] = bb[r] = 0.f;
        for (uint32_t t = 0; t < NC; ++t) {
          const uint32_t d = EX_KC * t + 4 * f4;
          pr_wave_sync();   // the chunk before has been read
#pragma unroll
          for (int q = 0; q < 4; ++q) {
            float4 v = cur[q];
            const float x = rx[q];
            v.x = d < k ? v.x * x : 0.f;
            v.y = d + 1 < k ? v.y * x : 0.f;
            v.z = d + 2 < k ? v.z * x : 0.f;
            v.w = d + 3 < k ? v.w * x : 0.f;
            if (!rp[q]) v = make_float4(0.f, 0.f, 0.f, 0.f);
            *reinterpret_cast<float4*>(&pan[(16 * q + (lane >> 2)) * EX_LS + 4 * f4]) = v;
          }
          pr_wave_sync();
          if (t + 1 < NC) load(t + 1, cur);   // on its way while this chunk is multiplied
          const float4 a0 = *reinterpret_cast<const float4*>(&pan[li * EX_LS + 8 * h]);
          const float4 a1 = *reinterpret_cast<const float4*>(&pan[li * EX_LS + 8 * h + 4]);
          const float4 b0 = *reinterpret_cast<const float4*>(&pan[(EX_P + li) * EX_LS + 8 * h]);
          const float4 b1 = *reinterpret_cast<const float4*>(&pan[(EX_P + li) * EX_LS + 8 * h + 4]);
          // eight K-steps per tile, each over {a d of half 0, a d of half 1}; a pair's sum is one chain, chunk after chunk
#define EX_TILE(ACC, L0, L1, R0, R1)                                      \
  ACC = __builtin_amdgcn_mfma_f32_32x32x2f32(L0.x, R0.x, ACC, 0, 0, 0);   \
  ACC = __builtin_amdgcn_mfma_f32_32x32x2f32(L0.y, R0.y, ACC, 0, 0, 0);   \
  ACC = __builtin_amdgcn_mfma_f32_32x32x2f32(L0.z, R0.z, ACC, 0, 0, 0);   \
  ACC = __builtin_amdgcn_mfma_f32_32x32x2f32(L0.w, R0.w, ACC, 0, 0, 0);   \
  ACC = __builtin_amdgcn_mfma_f32_32x32x2f32(L1.x, R1.x, ACC, 0, 0, 0);   \
  ACC = __builtin_amdgcn_mfma_f32_32x32x2f32(L1.y, R1.y, ACC, 0, 0, 0);   \
  ACC = __builtin_amdgcn_mfma_f32_32x32x2f32(L1.z, R1.z, ACC, 0, 0, 0);   \
  ACC = __builtin_amdgcn_mfma_f32_32x32x2f32(L1.w, R1.w, ACC, 0, 0, 0)
          if (doAA) { EX_TILE(aa, a0, a1, a0, a1); }
          if (useB) { EX_TILE(ab, a0, a1, b0, b1); }
          if (doBB) { EX_TILE(bb, b0, b1, b0, b1); }
#undef EX_TILE
        }
        if (doAA) ex_select(aa, spos, spos, nA, nA, true, sel, lane);
        if (useB) ex_select(ab, spos, spos + EX_P, nA, nB, false, sel, lane);
        if (doBB) ex_select(bb, spos + EX_P, spos + EX_P, nB, nB, true, sel, lane);
        pr_wave_sync();   // the slots' positions, before the next unit's
      }
    }
    const unsigned long long vh = lane < K ? s_hi[wave][lane] : 0ull;
    const uint32_t vl = lane < K ? s_lo[wave][lane] : 0u;
    const uint32_t n = (uint32_t)__popcll(__ballot(vh != 0ull));
    const float inter = wave_sum(sel.inter);
    if (lane == 0) {
      out.n[row] = n;
      out.inter[row] = inter;
    }
    if (lane < K) {
      uint32_t pi = 0, pj = 0;
      uint64_t idi = 0, idj = 0;
      float c = 0.f;
      if (vh != 0ull) {
        const float key = pr_key_of((uint32_t)(vh >> 32));
        pi = 0xFFFFFFFFu - (uint32_t)vh;
        pj = 0x7FFFFFFFu - (vl >> 1);
        c = (vl & 1u) ? -key : key;
        idi = reverse_bytes(in.feaids[in.index[beg + pi]]);
        idj = reverse_bytes(in.feaids[in.index[beg + pj]]);
      }
      const size_t at = (size_t)row * K + lane;
      out.pos_i[at] = pi;
      out.pos_j[at] = pj;
      out.c[at] = c;
      out.ids_i[at] = idi;
      out.ids_j[at] = idj;
    }
    nf_all += sel.nf;
    pr_wave_sync();   // the list, before the next row empties it
  }
  if (nf_all && lane == 0) atomicAdd(nonfinite, (unsigned long long)nf_all);
}

void ex_free_retired(dfh_explain* e) {
  for (void* a : e->retired) (void)hipFree(a);
  e->retired.clear();
}

// room for `extra` more rows; the rows held so far are copied on the stream, behind the kernels that wrote them
int ex_reserve(dfh_explain* e, size_t extra) {
  const size_t need = e->n + extra;
  if (need <= e->cap) return DFH_OK;
  size_t cap = e->cap ? e->cap : (e->hint ? e->hint : (size_t)1 << 14);
  while (cap < need) cap *= 2;
  char* nv = nullptr;
  const size_t bytes = cap * ex_row_bytes(e->K);
  if (hipMalloc((void**)&nv, bytes) != hipSuccess) {
    (void)hipGetLastError();
    set_error("dfh_explain: no device memory for " + std::to_string(cap) + " rows (" + std::to_string(bytes) + " bytes needed)");
    return DFH_ERR_CAPACITY;
  }
  if (e->n) {
    const ExOut a = ex_arrays(e->d_out, e->cap, e->K, 0), b = ex_arrays(nv, cap, e->K, 0);
    const size_t nk = e->n * e->K;
    hipStream_t s = e->ctx->stream;
    hipError_t er = hipMemcpyAsync(b.ids_i, a.ids_i, nk * sizeof(uint64_t), hipMemcpyDeviceToDevice, s);
    if (er == hipSuccess) er = hipMemcpyAsync(b.ids_j, a.ids_j, nk * sizeof(uint64_t), hipMemcpyDeviceToDevice, s);
    if (er == hipSuccess) er = hipMemcpyAsync(b.c, a.c, nk * sizeof(float), hipMemcpyDeviceToDevice, s);
    if (er == hipSuccess) er = hipMemcpyAsync(b.pos_i, a.pos_i, nk * sizeof(uint32_t), hipMemcpyDeviceToDevice, s);
    if (er == hipSuccess) er = hipMemcpyAsync(b.pos_j, a.pos_j, nk * sizeof(uint32_t), hipMemcpyDeviceToDevice, s);
    if (er == hipSuccess) er = hipMemcpyAsync(b.n, a.n, e->n * sizeof(uint32_t), hipMemcpyDeviceToDevice, s);
    if (er == hipSuccess) er = hipMemcpyAsync(b.inter, a.inter, e->n * sizeof(float), hipMemcpyDeviceToDevice, s);
    if (er != hipSuccess) {   // the object keeps its arrays; the new ones go once nothing queued can touch them
      e->retired.push_back(nv);
      set_error(std::string("dfh_explain: hipMemcpyAsync: ") + hipGetErrorString(er));
      return DFH_ERR_HIP;
    }
  }
  if (e->d_out) e->retired.push_back(e->d_out);
  e->d_out = nv;
  e->cap = cap;
  return DFH_OK;
}
}  // namespace

extern "C" {

int dfh_explain_create(dfh_ctx* ctx, int topk, int by, size_t capacity_hint, dfh_explain** out) {
  DFH_ARG(ctx && out, "dfh_explain_create: NULL argument");
  DFH_ARG(topk >= 1 && topk <= (int)EX_KMAX, "dfh_explain_create: topk must be in [1, 32]");
  DFH_ARG(by == DFH_PAIRS_ABS || by == DFH_PAIRS_POS, "dfh_explain_create: by must be DFH_PAIRS_ABS or DFH_PAIRS_POS");
  DFH_ARG(capacity_hint < EX_MAX_ROWS, "dfh_explain_create: capacity_hint must be below 2^32 - 16 rows");
  dfh_explain* e = new (std::nothrow) dfh_explain();
  if (!e) {
    set_error("dfh_explain_create: out of host memory (" + std::to_string(sizeof(dfh_explain)) + " bytes needed)");
    return DFH_ERR_CAPACITY;
  }
  e->ctx = ctx;
  e->K = (uint32_t)topk;
  e->by = by;
  e->hint = capacity_hint;
  hipError_t er = hipSetDevice(ctx->device);
  if (er == hipSuccess) er = hipMalloc(reinterpret_cast<void**>(&e->d_nf), sizeof(unsigned long long));
  if (er == hipSuccess) er = hipMemsetAsync(e->d_nf, 0, sizeof(unsigned long long), ctx->stream);
  if (er != hipSuccess) {
    (void)hipGetLastError();
    set_error(std::string("dfh_explain_create: ") + hipGetErrorString(er));
    dfh_explain_destroy(e);
    return DFH_ERR_HIP;
  }
  *out = e;
  return DFH_OK;
}

int dfh_explain_destroy(dfh_explain* e) {
  if (!e) return DFH_OK;
  (void)hipSetDevice(e->ctx->device);
  (void)hipStreamSynchronize(e->ctx->stream);   // queued kernels and copies read and write the arrays
  ex_free_retired(e);
  if (e->d_out) (void)hipFree(e->d_out);
  if (e->d_cpos) (void)hipFree(e->d_cpos);
  if (e->d_nf) (void)hipFree(e->d_nf);
  to_release(&e->text);
  delete e;
  return DFH_OK;
}

int dfh_explain_reset(dfh_explain* e) {
  DFH_ARG(e, "dfh_explain_reset: NULL argument");
  DFH_HIP(hipSetDevice(e->ctx->device));
  DFH_HIP(hipMemsetAsync(e->d_nf, 0, sizeof(unsigned long long), e->ctx->stream));   // behind the kernels that still count
  e->n = 0;   // the arrays stay; later appends are queued behind whatever still reads them
  e->formatted = false;
  return DFH_OK;
}

int dfh_explain_append_batch(dfh_explain* e, dfh_batch* b, dfh_table* t) {
  DFH_ARG(e && b && t, "dfh_explain_append_batch: NULL argument");
  DFH_ARG(b->ctx == e->ctx && t->ctx == e->ctx, "dfh_explain_append_batch: the batch or the table belongs to another context");
  DFH_ARG(e->n + (uint64_t)b->nrows < EX_MAX_ROWS, "dfh_explain_append_batch: the object holds fewer than 2^32 - 16 rows");
  if (b->stepped != t) {
    set_error("dfh_explain_append_batch: the batch's last step was not dfh_sgd_step on this table (not stepped since its load, or "
              "stepped through the sharded store, whose row words point into the rows other owners sent)");
    return DFH_ERR_STATE;
  }
  const size_t rows = b->nrows;
  if (rows == 0) return DFH_OK;
  dfh_ctx* c = e->ctx;
  hipStream_t s = c->stream;
  DFH_HIP(hipSetDevice(c->device));
  int rc = ex_reserve(e, rows);
  if (rc) return rc;
  const uint32_t K = e->K;
  const ExOut o = ex_arrays(e->d_out, e->cap, K, e->n);
  if (t->v.k == 0) {   // no V: nothing is launched, every list is empty
    DFH_HIP(hipMemsetAsync(o.ids_i, 0, rows * K * sizeof(uint64_t), s));
    DFH_HIP(hipMemsetAsync(o.ids_j, 0, rows * K * sizeof(uint64_t), s));
    DFH_HIP(hipMemsetAsync(o.c, 0, rows * K * sizeof(float), s));
    DFH_HIP(hipMemsetAsync(o.pos_i, 0, rows * K * sizeof(uint32_t), s));
    DFH_HIP(hipMemsetAsync(o.pos_j, 0, rows * K * sizeof(uint32_t), s));
    DFH_HIP(hipMemsetAsync(o.n, 0, rows * sizeof(uint32_t), s));
    DFH_HIP(hipMemsetAsync(o.inter, 0, rows * sizeof(float), s));
  } else {
    if (b->nnz > e->cpos_cap) {
      size_t cap = std::max<size_t>(e->cpos_cap, (size_t)1 << 16);
      while (cap < b->nnz) cap *= 2;
      uint32_t* nv = nullptr;
      if (hipMalloc((void**)&nv, cap * sizeof(uint32_t)) != hipSuccess) {
        (void)hipGetLastError();
        set_error("dfh_explain_append_batch: no device memory for the has-V positions of " + std::to_string(cap) + " nonzeros (" +
                  std::to_string(cap * sizeof(uint32_t)) + " bytes needed)");
        return DFH_ERR_CAPACITY;
      }
      if (e->d_cpos) e->retired.push_back(e->d_cpos);
      e->d_cpos = nv;
      e->cpos_cap = cap;
    }
    ExIn in;
    in.offset = b->d_offset;
    in.index = b->d_index;
    in.value = b->has_value ? b->d_value : nullptr;
    in.uw = b->d_uw;
    in.feaids = b->d_feaids;
    in.va = t->v.va;
    in.nrows = (uint32_t)rows;
    in.k = (uint32_t)t->v.k;
    in.kp = (uint32_t)t->v.kp;
    launch_k(c, DFH_K_EXPLAIN, k_explain, dim3((unsigned)grid_for_waves(rows, c)), dim3(256), 0, s, in, K, e->by == DFH_PAIRS_POS ? 1 : 0, e->d_cpos,
             o, e->d_nf);
    DFH_HIP(hipGetLastError());
  }
  e->n += rows;
  e->formatted = false;
  // The kernel runs on the context's stream, behind the batch's step, and reads the batch's arrays; the batch object's NEXT load
  // runs on a preparation stream that waits for ev_free alone (the hazard dfh_eval_append_batch documents): with pipelining on,
  // ev_free is recorded again behind the kernel.  Call it before the next minibatch is loaded into the batch object.
  if (c->pipeline) {
    DFH_HIP(hipEventRecord(b->ev_free, s));
    b->free_pending = true;
  }
  return DFH_OK;
}

int dfh_explain_count(dfh_explain* e, uint64_t* n) {
  DFH_ARG(e && n, "dfh_explain_count: NULL argument");
  *n = e->n;
  return DFH_OK;
}

int dfh_explain_read(dfh_explain* e, uint32_t* n, uint64_t* ids_i, uint64_t* ids_j, float* c, float* inter, uint64_t* nonfinite) {
  DFH_ARG(e && nonfinite, "dfh_explain_read: NULL argument");
  *nonfinite = 0;
  DFH_ARG(e->n == 0 || (n && ids_i && ids_j && c && inter), "dfh_explain_read: NULL argument");
  hipStream_t s = e->ctx->stream;
  DFH_HIP(hipSetDevice(e->ctx->device));
  unsigned long long nf = 0;
  if (e->n) {
    const ExOut o = ex_arrays(e->d_out, e->cap, e->K, 0);
    const size_t nk = e->n * e->K;
    DFH_HIP(hipMemcpyAsync(ids_i, o.ids_i, nk * sizeof(uint64_t), hipMemcpyDeviceToHost, s));
    DFH_HIP(hipMemcpyAsync(ids_j, o.ids_j, nk * sizeof(uint64_t), hipMemcpyDeviceToHost, s));
    DFH_HIP(hipMemcpyAsync(c, o.c, nk * sizeof(float), hipMemcpyDeviceToHost, s));
    DFH_HIP(hipMemcpyAsync(inter, o.inter, e->n * sizeof(float), hipMemcpyDeviceToHost, s));
    DFH_HIP(hipMemcpyAsync(n, o.n, e->n * sizeof(uint32_t), hipMemcpyDeviceToHost, s));
  }
  DFH_HIP(hipMemcpyAsync(&nf, e->d_nf, sizeof(nf), hipMemcpyDeviceToHost, s));
  DFH_HIP(hipStreamSynchronize(s));
  ex_free_retired(e);
  *nonfinite = nf;
  return DFH_OK;
}

int dfh_explain_read_positions(dfh_explain* e, uint32_t* pos_i, uint32_t* pos_j) {
  DFH_ARG(e && (e->n == 0 || (pos_i && pos_j)), "dfh_explain_read_positions: NULL argument");
  DFH_HIP(hipSetDevice(e->ctx->device));
  if (e->n) {
    const ExOut o = ex_arrays(e->d_out, e->cap, e->K, 0);
    const size_t nk = e->n * e->K;
    DFH_HIP(hipMemcpyAsync(pos_i, o.pos_i, nk * sizeof(uint32_t), hipMemcpyDeviceToHost, e->ctx->stream));
    DFH_HIP(hipMemcpyAsync(pos_j, o.pos_j, nk * sizeof(uint32_t), hipMemcpyDeviceToHost, e->ctx->stream));
  }
  DFH_HIP(hipStreamSynchronize(e->ctx->stream));
  ex_free_retired(e);
  return DFH_OK;
}

}  // extern "C"
