// dfh_lookup.hip — the pass over a minibatch's unique keys that opens a step: key -> table row (inserted on a miss), with
// Push(kFeaCount) and the InitV it may trigger, {row | flags, w} per key for the forward, and the parts of the very hot keys
// for the update's split role (SplitOut).  k_lookup is the probe of a preparation stream, k_lookup_step the step's own pass,
// k_uw_remote / k_lookup_uw_remote the row words of keys other ranks own (sharded store); k_refrand_* initialise the rows a
// pass flagged, in key order (parity mode).  Launched by dfh_step.hip, dfh_shard.hip, dfh_store_calls.hip, dfh_feed.hip,
// dfh_localize_api.hip and dfh_table.hip (refrand_flush); dfh_riders.hip builds the rider form of the step's pass from lookup_body.
#ifndef DFH_LOOKUP_HIP_
#define DFH_LOOKUP_HIP_
#include "dfh_index.hip"   // the probes; init_v_hash_row, lcg_jump, refrand_value by way of dfh_updater.h
#include "dfh_auc.hip"     // AucFin, auc_finalize_block: a step's pass closes the previous step's AUC

namespace dfh {

// ---------------------------------------------------------------------------
// k_lookup: one thread per unique key.  urow[u] = row of feaids[u] (inserted as
// a zero row if unseen: sgd_updater.cc:44).  With cnt != NULL it also applies
// Push(kFeaCount): fea_cnt += cnt, maybe InitV (sgd_updater.cc:62-73).
// cnt_from_ptr: counts are the segment lengths of the localized batch.
// ---------------------------------------------------------------------------
// The parts of the keys with more than HOT_SPLIT_MIN occurrences in the minibatch (SegLists::split_ent), listed by the pass that
// visits every unique key before the update and has its segment at hand (col_ptr): one atomic on the list's counter per such key —
// a handful per minibatch at most.  (Round 6's first form listed them in k_loc_emit: the inlined loop took that kernel's allocation
// from 56 to 72 registers, and the first epoch's steps, where emit runs beside the update, lost 15 % — profiles/r06r_*.  Those
// profiles quote rocprofv3's `vgpr` column, 28 -> 36, which is HALF the allocation for every kernel of this library; the allocation
// is the kernel descriptor's next free VGPR in granules of 8.  Emit did not fit in the 32 registers five 96-register waves of
// k_update_fused leave free on a SIMD at either size; since the register fit of the preparation kernels it is allocated 32 —
// tests/test_prep_registers.py.)
// INVARIANT (one owner): the list is empty when a training step's first listing launch starts.  The STEP keeps it.  A batch
// object has TWO counters (d_U + 2, d_U + 3; both zero at creation): the listing launches of a step append to one (`n`) and
// leave the OTHER at zero (split_other: one store by the launch's first thread), and the step that listed then swaps them
// (split_out / main_end, dfh_phases.hip) — so the next step, whenever it comes and whether or not a localize came between, starts
// from a counter that the previous step's launches zeroed, and this step's update reads the one just filled.  The reset
// costs no launch of its own (a 4-byte memset node per step was measured at -3 % on the default benchmark line).  A step may
// make two listing launches, the own keys' lookup and the others' row words (sharded store): both append to the same
// counter and zero the same other one.  A batch object can be stepped any number of times per localize (later epochs,
// dfh_batch_load_localized_host): when only the Localizer emptied the list every very hot key was listed once more per
// step and updated once per copy.  The Localizer's count pass and k_seg_lists_reset still zero d_U + 2; no step relies on it.
struct SplitOut {
  SegEnt* ent;        // NULL: no list (the update's hot role takes every key whole)
  uint32_t* n;        // entries so far (zero when the step begins: see above); the OTHER counter is its neighbour, split_other(n)
  uint32_t u_base;    // rank of the first key this launch sees (the sharded store looks up its own keys only)
  uint32_t cap;       // entries the list can hold (dfh_batch::split_cap: enough for any minibatch the batch object can hold)
};   // (24 bytes, as before the capacity was added: the step's lookup is short of scalar registers)
// d_U + 2 <-> d_U + 3 (d_U is 256-byte aligned: the two counters differ in address bit 2)
__device__ __forceinline__ uint32_t* split_other(uint32_t* n) { return reinterpret_cast<uint32_t*>(reinterpret_cast<uintptr_t>(n) ^ 4u); }
// err: the table's error word — bit 16 = a key's parts did not fit (dfh_table_check)
__device__ __forceinline__ void lookup_split(const SplitOut& so, uint32_t* err, uint32_t u, uint32_t beg, uint32_t end) {
  if (!(DFH_HOT_SPLIT_BUILD & 1) || !so.ent || end - beg <= HOT_SPLIT_MIN) return;
  const uint32_t nparts = (end - beg + HOT_SPLIT - 1u) / HOT_SPLIT;
  const uint32_t base = atomicAdd(so.n, nparts);
  if (base + nparts > so.cap) {   // cannot happen with an emptied list (split_cap); nothing is written, the counter stays beyond
    atomicOr(err, 16u);           // cap, and the update, which sees that, leaves the whole list alone (upd_split_role)
    return;
  }
  for (uint32_t p = 0; p < nparts; ++p)
    so.ent[base + p] = make_uint4(u + so.u_base, beg + p * HOT_SPLIT, min(beg + (p + 1u) * HOT_SPLIT, end), (p << 16) | nparts);
}

template <bool SPLIT = true>
__device__ __forceinline__ void lookup_body(const TableView& t, const uint64_t* __restrict__ keys, const uint32_t* __restrict__ d_n,
                         uint32_t n_static, uint32_t* __restrict__ urow, const float* __restrict__ cnt,
                         const uint32_t* __restrict__ col_ptr, int push_cnt, uint32_t* __restrict__ need_init,
                         int rows_known, uint2* __restrict__ uw, AucFin fin, const uint32_t bid, const uint32_t nblk,
                         const SplitOut so = SplitOut{nullptr, nullptr, 0u, 0u}) {
  // a step's lookup also closes the AUC its batch object's previous step left pending (dfh_sgd_step; fin.n == 0: none)
  if (fin.n && bid == 0) auc_finalize_block(fin);
  if (SPLIT && so.n && bid == 0 && threadIdx.x == 0) *split_other(so.n) = 0u;   // the NEXT step's split list starts empty (SplitOut)
  uint32_t n = d_n ? *d_n : n_static;
  __shared__ uint32_t ins_sh[8];
  // (block-uniform trip count: the insert below is a block-wide call)
  for (uint32_t u0 = bid * blockDim.x; u0 < n; u0 += nblk * blockDim.x) {
    const uint32_t u = u0 + threadIdx.x;
    const bool active = u < n;
    uint64_t key = active ? keys[u] : 0ull;
    // rows_known: urow was filled by an earlier (prep-stream) lookup of the same keys
    // (rows_known: a row word of k_resolve_multi may carry its worker mark in bit 31 — dfh_shard_push_count_resolved)
    uint32_t r;
    if (rows_known) r = active ? (urow[u] & kRowMask) : 0u;
    else if (blockDim.x == 256) r = find_or_insert_block(t, key, active, ins_sh);
    else r = active ? find_or_insert(t, key) : 0u;
    if (!active) continue;
    if (urow && !rows_known) urow[u] = r;
    if (SPLIT && col_ptr) lookup_split(so, t.err, u, col_ptr[u], col_ptr[u + 1]);
    float w = 0.f;
    bool hasv = false;
    if (push_cnt) {
      float c = cnt ? cnt[u] : (float)(col_ptr[u + 1] - col_ptr[u]);
      RowHdr& h = t.hdr[r];
      w = h.w;
      // push_cnt == 2: a training step follows whose update kernel rewrites this header anyway.  A key that HAS its V can
      // take its count there (k_update_fused adds it): nothing reads fea_cnt of such a key again — it only gates InitV
      // (sgd_updater.cc:62-73, :122-126) — so the value is the same and this pass stays read-only for it.
      if (push_cnt == 2 && uw && h.has_V != 0) {
        if (need_init) need_init[u] = 0u;
        uw[u] = make_uint2(r | kCountLater | kHasV | ((col_ptr != nullptr && col_ptr[u + 1] - col_ptr[u] == 1u) ? kSingleRow : 0u),
                           __float_as_uint(w));
        continue;
      }
      float fc = h.fea_cnt + c;
      h.fea_cnt = fc;
      hasv = h.has_V != 0;
      bool init = t.k > 0 && !hasv && w != 0 && fc > (float)t.p.V_threshold;
      if (t.p.init_mode == DFH_INIT_HASH) {
        if (init) {
          init_v_hash_row(t, r, key);
          h.has_V = 1;
        }
      } else if (need_init) {
        need_init[u] = init ? 1u : 0u;   // (REFRAND: the row is written by k_refrand_init right after this launch, before the forward)
      }
      hasv = hasv || init;   // InitV at count-push time (sgd_updater.cc:69-72): this step's Pull sees the new V
    } else if (uw) {
      const uint2 wh = *reinterpret_cast<const uint2*>(&t.hdr[r]);  // {w, has_V}: one 8 B load
      w = __uint_as_float(wh.x);
      hasv = wh.y != 0u;
    }
    // {row, w} per unique key, batch-local and L2-resident: the forward then touches nothing of a
    // row but its V lines (the weight is read here once per KEY instead of once per nonzero)
    // bit 30 of the row word: the key occurs once in this minibatch (k_update_fused updates such keys example by
    // example, without the key-ordered view)
    if (uw) {
      const bool single = col_ptr != nullptr && col_ptr[u + 1] - col_ptr[u] == 1u;
      uw[u] = make_uint2(r | (single ? kSingleRow : 0u) | (hasv ? kHasV : 0u), __float_as_uint(w));
    }
  }
}

// (two kernels: the probe that runs on a preparation stream BESIDE the update must stay small in registers — its waves take what
// five 96-register update waves leave free on a SIMD — so only the step's own pass carries the split-list code)
__global__ void k_lookup(TableView t, const uint64_t* __restrict__ keys, const uint32_t* __restrict__ d_n,
                         uint32_t n_static, uint32_t* __restrict__ urow, const float* __restrict__ cnt,
                         const uint32_t* __restrict__ col_ptr, int push_cnt, uint32_t* __restrict__ need_init,
                         int rows_known, uint2* __restrict__ uw, AucFin fin) {
  lookup_body<false>(t, keys, d_n, n_static, urow, cnt, col_ptr, push_cnt, need_init, rows_known, uw, fin, blockIdx.x, gridDim.x);
}
__global__ void k_lookup_step(TableView t, const uint64_t* __restrict__ keys, const uint32_t* __restrict__ d_n,
                              uint32_t n_static, uint32_t* __restrict__ urow, const float* __restrict__ cnt,
                              const uint32_t* __restrict__ col_ptr, int push_cnt, uint32_t* __restrict__ need_init,
                              int rows_known, uint2* __restrict__ uw, AucFin fin, SplitOut so) {
  lookup_body<true>(t, keys, d_n, n_static, urow, cnt, col_ptr, push_cnt, need_init, rows_known, uw, fin, blockIdx.x, gridDim.x, so);
}

// sharded store: {u | kRemoteRow, w} for the keys OTHER ranks own, from the rows they sent (row u of
// the pulled-rows buffer belongs to key u; the slots of this rank's own keys [lo, hi) are unused)
struct UwRemote {
  const float* rows;
  size_t stride;
  const uint32_t* d_U;
  uint32_t lo, hi;
  uint2* uw;                 // the whole minibatch's array (the lookup's `uw` starts at the rank's own keys)
  const uint32_t* col_ptr;   // likewise
  SplitOut so;               // the others' keys can be very hot too (u_base 0: ranks are the minibatch's)
  uint32_t* err;             // the table's error word (lookup_split)
};
__device__ __forceinline__ void uw_remote_body(const UwRemote& m) {
  const uint32_t U = *m.d_U;
  if (m.so.n && blockIdx.x == 0 && threadIdx.x == 0) *split_other(m.so.n) = 0u;   // (as lookup_body: SplitOut)
  for (uint32_t u = blockIdx.x * blockDim.x + threadIdx.x; u < U; u += gridDim.x * blockDim.x) {
    if (u - m.lo < m.hi - m.lo) continue;
    // (bit 30: the key occurs once in the minibatch — the singles role of the mixed update launch takes it)
    const uint32_t single = (m.col_ptr && m.col_ptr[u + 1] - m.col_ptr[u] == 1u) ? kSingleRow : 0u;
    if (m.col_ptr) lookup_split(m.so, m.err, u, m.col_ptr[u], m.col_ptr[u + 1]);
    const float2 wh = *reinterpret_cast<const float2*>(m.rows + (size_t)u * m.stride);   // [w, has_V (0 / 1 as float), ...]
    m.uw[u] = make_uint2(u | kRemoteRow | single | (wh.y != 0.f ? kHasV : 0u), __float_as_uint(wh.x));
  }
}
__global__ void k_uw_remote(const float* __restrict__ rows, size_t stride, const uint32_t* __restrict__ d_U, uint32_t lo,
                            uint32_t hi, uint2* __restrict__ uw, const uint32_t* __restrict__ col_ptr, SplitOut so, uint32_t* err) {
  uw_remote_body(UwRemote{rows, stride, d_U, lo, hi, uw, col_ptr, so, err});
}
// the own keys' lookup and the others' row words in ONE launch (overlapped exchange: the rows of the other owners arrived
// during the previous step; one launch boundary less on the main stream of the sharded step)
__global__ void k_lookup_uw_remote(TableView t, const uint64_t* __restrict__ keys, uint32_t n_static, uint32_t* __restrict__ urow,
                                   const float* __restrict__ cnt, const uint32_t* __restrict__ col_ptr, int push_cnt,
                                   uint2* __restrict__ uw, AucFin fin, UwRemote m, SplitOut so) {
  lookup_body(t, keys, nullptr, n_static, urow, cnt, col_ptr, push_cnt, nullptr, 0, uw, fin, blockIdx.x, gridDim.x, so);
  uw_remote_body(m);
}

// ---------------------------------------------------------------------------
// REFRAND lazy init (parity mode): rows flagged in need[] are initialised in
// ascending key order from the mutated rand_r chain, exactly as the serial
// loop of SGDUpdater::Update would (sgd_updater.cc:62-73, :86-95, :140-147).
// k_refrand_scan: single block, exclusive scan of need[0..n) -> rank[], total.
// ---------------------------------------------------------------------------
__global__ void k_refrand_scan(const uint32_t* __restrict__ need, const uint32_t* __restrict__ d_n, uint32_t n_static,
                               uint32_t* __restrict__ rank, uint32_t* __restrict__ total) {
  __shared__ uint32_t wsum[16];
  __shared__ uint32_t carry_s;
  uint32_t n = d_n ? *d_n : n_static;
  if (threadIdx.x == 0) carry_s = 0;
  __syncthreads();
  for (uint32_t base = 0; base < n; base += blockDim.x) {
    uint32_t i = base + threadIdx.x;
    uint32_t v = i < n ? need[i] : 0;
    // inclusive scan inside the wave
    uint32_t s = v;
#pragma unroll
    for (int o = 1; o < 64; o <<= 1) {
      uint32_t y = __shfl_up(s, o, 64);
      if (lane_id() >= o) s += y;
    }
    int w = threadIdx.x >> 6;
    if (lane_id() == 63) wsum[w] = s;
    __syncthreads();
    uint32_t woff = 0;
    for (int j = 0; j < w; ++j) woff += wsum[j];
    uint32_t carry = carry_s;
    if (i < n) rank[i] = carry + woff + s - v;
    __syncthreads();
    if (threadIdx.x == blockDim.x - 1) carry_s = carry + woff + s;
    __syncthreads();
  }
  if (threadIdx.x == 0) *total = carry_s;
}

__global__ void k_refrand_init(TableView t, const uint64_t* __restrict__ keys, const uint32_t* __restrict__ d_n,
                               uint32_t n_static, const uint32_t* __restrict__ urow,
                               const uint32_t* __restrict__ need, const uint32_t* __restrict__ rank) {
  uint32_t n = d_n ? *d_n : n_static;
  uint32_t state0 = *t.rng_state;
  for (uint32_t u = blockIdx.x * blockDim.x + threadIdx.x; u < n; u += gridDim.x * blockDim.x) {
    if (!need[u]) continue;
    uint32_t r = urow ? urow[u] : find_only(t, keys[u]);
    uint32_t st = lcg_jump(state0, (uint64_t)3 * (uint64_t)t.k * (uint64_t)rank[u]);
    float* va = t.va + (size_t)r * (2 * t.kp);
    for (int j = 0; j < t.kp; ++j) {
      va[j] = j < t.k ? refrand_value(st, t.p.V_init_scale) : 0.0f;
      va[t.kp + j] = 0.0f;
    }
    t.hdr[r].has_V = 1;
  }
}

__global__ void k_refrand_advance(TableView t, const uint32_t* __restrict__ total) {
  if (threadIdx.x == 0 && blockIdx.x == 0) {
    *t.rng_state = lcg_jump(*t.rng_state, (uint64_t)3 * (uint64_t)t.k * (uint64_t)(*total));
  }
}

}  // namespace dfh
#endif  // DFH_LOOKUP_HIP_
