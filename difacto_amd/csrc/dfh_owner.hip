// Owner side of the sharded store (device pointers, fixed-stride rows) for gfx950, four forms behind the C ABI, bit-identical:
//   literal     k_pull_rows / k_push_grad                            one wave per key, probes per call; the REFRAND path
//   resolved    k_resolve / k_pull_resolved / k_push_grad_resolved   probe once per step, then L lanes per key on row ids
//   per entry   k_resolve_multi / k_push_count_multi / k_pull_resolved / k_push_grad_multi (+ k_release_rows): the default
//   per key     k_resolve_multi / k_count_pull_multi / k_push_grad_chunks                    (ctx option owner_per_key)
// What they share stands once: LaneGroup, RowRegs (load, refuse, apply, store), sort8 / next_ascending, put_pull_row.  The
// key index and the update arithmetic are dfh_kernels.hip's (find_or_insert, ftrl_update_w, adagrad_update_v, init_v_hash_*).
// ---------------------------------------------------------------------------
// Owner side, one launch for ALL source ranks of a step.  The received keys are the
// concatenation of nsrc ascending lists (SegOff).  k_resolve_multi resolves every entry to
// its row and elects ONE entry per key, the first to arrive, as the key's WORKER: it claims the
// row's step word (RowHdr::pad[slot], 0 outside a step) with a compare-and-swap, leaving
// (entry + 1) << 5 there; every later entry of the key bumps the word's low 5 bits (one
// atomic add: the old value names the worker and the entry's place k) and writes its own index
// into the worker's extras, extra[worker * XS + k].  In the Push kernels the worker — bit 31 of
// its row word — has the number of the key's other entries with the header it reads anyway and
// their indices in one 16 / 32 B read; it orders them by source (sources are concatenated in
// ascending order: by entry index) and applies their values one after the other in source
// order — exactly what per-source launches would do — storing the row once.  Every other entry
// skips on its row word alone.  (Round 4 searched each later source's list by bisection, 14
// dependent loads per source; a linked list through the entries, tried first in round 5, still
// cost one dependent — and, written by another launch, cold — load per entry: 57 us for the
// gradient push at C4 size against 25 us for the same rows without the multi-source keys.)
// The last Push of a step (or k_release_rows) clears the step word.
// rowid holds multi_words(n, nsrc) words: [0, n) the row words, from multi_extra_base(n) on
// XS = multi_xs(nsrc) extras per entry.
// ---------------------------------------------------------------------------
#ifndef DFH_OWNER_HIP_
#define DFH_OWNER_HIP_
#include "dfh_internal.h"

namespace dfh {

struct SegOff {
  uint32_t off[33];  // entries of source s are [off[s], off[s+1])
  int nsrc;
  int slot;          // which of the two per-row step words (RowHdr::pad[0..1]) this step uses: two steps
                     // may be in flight on an owner (one resolved and pulled, the other awaiting its gradients)
};
constexpr uint32_t ROW_WORKER = 0x80000000u;   // beside the row id (kRowMask: a table holds fewer than 2^28 rows)
constexpr uint32_t NO_ENTRY = 0xFFFFFFFFu;     // sorts behind every entry
constexpr int MULTI_FAST = 8;                  // entries per key ordered in registers (one node: 7 peers)
__host__ __device__ __forceinline__ uint32_t multi_xs(int nsrc) { return (uint32_t)((nsrc - 1 + 3) / 4 * 4 > 0 ? (nsrc - 1 + 3) / 4 * 4 : 4); }
__host__ __device__ __forceinline__ size_t multi_extra_base(size_t n) { return (n + 3) & ~(size_t)3; }
// Behind the row words and the extras, the key lists k_count_pull_multi leaves for k_push_grad_chunks: the entries are cut
// into chunks of MULTI_CH; a chunk's keys of ONE source (its workers without extras) stand in slist[c * MULTI_CH ...) as
// {entry, row}, its keys of several sources in mrec[(c * MULTI_CH + j) * (XS + 4) ...) as {entry | m << 27, row, -, -,
// the other entries in ascending (= source) order}, chdr[c] = {keys of one source, keys of several}.
#ifndef DFH_MULTI_CH
#define DFH_MULTI_CH 32   // (16 / 32 / 64 / 128: push 48.7 / 45.1 / 53.2 / 66.6 us, count + pull 36 / 36 / 40 / 45 us at N = 8 size)
#endif
constexpr uint32_t MULTI_CH = DFH_MULTI_CH;
__host__ __device__ __forceinline__ size_t multi_slist_base(size_t n, int nsrc) { return multi_extra_base(n) + n * multi_xs(nsrc); }
__host__ __device__ __forceinline__ size_t multi_ch_entries(size_t n) { return (n + MULTI_CH - 1) / MULTI_CH * MULTI_CH; }  // whole chunks: the readers request a chunk's first entries with its counts
__host__ __device__ __forceinline__ size_t multi_mrec_base(size_t n, int nsrc) { return multi_slist_base(n, nsrc) + 2 * multi_ch_entries(n); }
__host__ __device__ __forceinline__ size_t multi_chdr_base(size_t n, int nsrc) {
  return multi_mrec_base(n, nsrc) + multi_ch_entries(n) * (multi_xs(nsrc) + 4);
}
__host__ __device__ __forceinline__ size_t multi_words(size_t n, int nsrc) {
  return multi_chdr_base(n, nsrc) + 2 * ((n + MULTI_CH - 1) / MULTI_CH + 1);
}

// L lanes work on one row: lane `sub` of the group holds the row's floats [d, d + 4) — 4 * L >= kp by dispatch, one float4
// per lane covers the row.  Lanes beyond the row (with V_dim = 0: all) read valid addresses they do not use — the row's
// header, a gradient row's head (goff = 0) — so the loads stay unconditional.
template <int L>
struct LaneGroup {
  static constexpr int GPW = 64 / L;        // groups per wave
  static constexpr uint32_t GPB = 256 / L;  // groups per block
  const int sub = lane_id() % L, d = sub * 4;
  const uint32_t group = ((blockIdx.x * blockDim.x + threadIdx.x) >> 6) * GPW + lane_id() / L;  // among the grid's
  const uint32_t ngroups = ((gridDim.x * blockDim.x) >> 6) * GPW;
  const uint32_t grp = threadIdx.x / L;                                                         // among the block's
  const bool d_ok;
  const int goff;
  __device__ __forceinline__ explicit LaneGroup(const TableView& t) : d_ok(d < t.kp), goff(d_ok ? 4 + d : 0) {}
};

__device__ __forceinline__ float4 zero4() { return make_float4(0.f, 0.f, 0.f, 0.f); }

// A table row in the registers of its lane group, for Push(kGradient) = SGDUpdater::Update (sgd_updater.cc:74-138): load it,
// refuse it or apply the sources' gradient rows one after the other, store it once.  STEP_WORD: the row's step word
// (RowHdr::pad[slot], above) is cleared with the row's last store.
template <int L, bool STEP_WORD>
struct RowRegs {
  const TableView& t;
  const LaneGroup<L>& ln;
  const int slot;
  uint32_t r, has_v;
  RowHdr* hp;
  float* va;
  float w, sqrt_g, z, fea_cnt;
  float4 v, acc;  // this lane's slices of V and of the AdaGrad accumulators
  bool had_v;     // the gradient rows carry V: the row was pulled with V (lens[i] > 1 in sgd_updater.cc:90)
  __device__ __forceinline__ RowRegs(const TableView& t_, const LaneGroup<L>& ln_, int slot_ = 0) : t(t_), ln(ln_), slot(slot_) {}

  // one round trip, requested before anything is known about the row: the header as {w, has_V, sqrt_g, z}, fea_cnt, the slices
  __device__ __forceinline__ void load(uint32_t row) {
    r = row;
    hp = t.hdr + r;
    va = t.va + (size_t)r * (2 * t.kp);
    const float* hf = reinterpret_cast<const float*>(hp);
    const float4 h0 = ld4(hf);
    fea_cnt = hp->fea_cnt;
    v = ld4(ln.d_ok ? va + ln.d : hf);
    acc = ld4(ln.d_ok ? va + t.kp + ln.d : hf);
    w = h0.x, sqrt_g = h0.z, z = h0.w;
    has_v = __float_as_uint(h0.y);
  }

  // CHECK(e.V != nullptr), sgd_updater.cc:92: a gradient with V for a row without.  Every source pulled the same model
  // version, so one gradient row's flag answers for all of them.  True: error bit 4, the row is out of the step.
  __device__ __forceinline__ bool refuse(bool grad_has_v) {
    had_v = grad_has_v;
    if (!had_v || has_v) return false;
    if (ln.sub == 0) {
      atomicOr(t.err, 4u);
      if (STEP_WORD) hp->pad[slot] = 0;
    }
    return true;
  }

  // one source's gradient row {gw | this lane's gv}: FTRL on w, lazy InitV, AdaGrad on V iff the row was pulled with V
  __device__ __forceinline__ void apply(float gw, const float4& gv, const uint64_t* key) {
    const float w_old = w;
    w = ftrl_update_w(gw, w_old, sqrt_g, z, t.p);
    // lazy InitV when w leaves zero (sgd_updater.cc:122-126); the pulled rows had no V, so no gradient of this step touches
    // the fresh values.  Every lane of the group reaches this with the same w: each writes its own 16 B of V and of the
    // accumulators.  HASH init only on this path
    if (w_old == 0 && w != 0 && t.k > 0 && has_v == 0 && fea_cnt > (float)t.p.V_threshold) {
      if (ln.d_ok) init_v_hash_slice(t, r, *key, ln.d);
      has_v = 1;
    }
    if (had_v && ln.d_ok) {
      adagrad_update_v(gv.x, v.x, acc.x, t.p);
      adagrad_update_v(gv.y, v.y, acc.y, t.p);
      adagrad_update_v(gv.z, v.z, acc.z, t.p);
      adagrad_update_v(gv.w, v.w, acc.w, t.p);
    }
  }

  // the header in one 16 B store, the slices with zeros beyond V_dim
  __device__ __forceinline__ void store() {
    if (ln.sub == 0) {
      st4(reinterpret_cast<float*>(hp), make_float4(w, __uint_as_float(has_v), sqrt_g, z));
      if (STEP_WORD) hp->pad[slot] = 0;
    }
    if (had_v && ln.d_ok) {
      const int d = ln.d;
      if (d + 0 >= t.k) { v.x = 0.f; acc.x = 0.f; }
      if (d + 1 >= t.k) { v.y = 0.f; acc.y = 0.f; }
      if (d + 2 >= t.k) { v.z = 0.f; acc.z = 0.f; }
      if (d + 3 >= t.k) { v.w = 0.f; acc.w = 0.f; }
      st4(va + d, v);
      st4(va + t.kp + d, acc);
    }
  }
};

// The entries of one key in ascending order (sources are concatenated in ascending order: by source).  Up to MULTI_FAST of them
// in registers: ent[nvalid ...) are masked out, then an odd-even transposition network
__device__ __forceinline__ void sort8(uint32_t (&ent)[MULTI_FAST], uint32_t nvalid) {
#pragma unroll
  for (int i = 0; i < MULTI_FAST; ++i)
    if ((uint32_t)i >= nvalid) ent[i] = NO_ENTRY;
#pragma unroll
  for (int pass = 0; pass < MULTI_FAST; ++pass) {
#pragma unroll
    for (int i = pass & 1; i + 1 < MULTI_FAST; i += 2) {
      const uint32_t lo = min(ent[i], ent[i + 1]), hi = max(ent[i], ent[i + 1]);
      ent[i] = lo;
      ent[i + 1] = hi;
    }
  }
}
// more of them (a job beyond one node) by selection out of memory: the smallest of xp[0 .. m) and `own` (NO_ENTRY: none) that
// is not below `from`; the walk starts from 0 and goes on from the entry it got + 1 (a key's entries are distinct)
__device__ __forceinline__ uint32_t next_ascending(const uint32_t* xp, uint32_t m, uint32_t own, uint32_t from) {
  uint32_t best = own >= from ? own : NO_ENTRY;
  for (uint32_t i = 0; i < m; ++i) {
    const uint32_t x = xp[i];
    if (x >= from && x < best) best = x;
  }
  return best;
}

// This lane's part of a pull row [w, has_V, 0, 0 | V] = SGDUpdater::Get: the head from the group's first lane, floats
// [d, d + 4) of V (zeros for a row without V) from the lanes inside the row
__device__ __forceinline__ void put_pull_row(float* out, bool first_lane, float w, bool has_v, int d, bool d_ok, const float4& v) {
  if (first_lane) st4(out, make_float4(w, has_v ? 1.0f : 0.0f, 0.f, 0.f));
  if (d_ok) st4(out + 4 + d, v);
}

// ---------------------------------------------------------------------------
// Literal form.  k_pull_rows: Store::Pull -> SGDUpdater::Get for n unique keys: one wave per key copies the row into the
// exchange buffer (rows beyond 256 floats in further rounds).
// ---------------------------------------------------------------------------
__global__ void __launch_bounds__(256) k_pull_rows(TableView t, const uint64_t* __restrict__ keys, uint32_t n,
                                                   float* __restrict__ rows, size_t stride) {
  const LaneGroup<64> ln(t);  // the wave
  for (uint32_t u = ln.group; u < n; u += ln.ngroups) {
    uint32_t r = 0;
    if (ln.sub == 0) r = find_or_insert(t, keys[u]);
    r = __shfl(r, 0, 64);
    const RowHdr h = t.hdr[r];
    const float* va = t.va + (size_t)r * (2 * t.kp);
    int d = ln.d;
    do {
      const bool d_ok = d < t.kp;
      put_pull_row(rows + (size_t)u * stride, d == 0, h.w, h.has_V, d, d_ok, h.has_V && d_ok ? ld4(va + d) : zero4());
      d += 256;
    } while (d < t.kp);
  }
}

// Push(kGradient) for n unique keys from fixed-stride gradient rows; one wave per key, lane 0 the header, the lanes stride over
// V: the REFRAND path (need_init, urow_out: the rows whose V the host's rand_r chain fills, refrand_flush).
// The V part is applied iff the gradient row says V was present at pull time
// (lens[i] > 1 in sgd_updater.cc:90).
__global__ void __launch_bounds__(256) k_push_grad(TableView t, const uint64_t* __restrict__ keys, uint32_t n,
                                                   const float* __restrict__ grads, size_t stride,
                                                   uint32_t* __restrict__ need_init, uint32_t* __restrict__ urow_out) {
  const int lane = lane_id();
  const int wave = (blockIdx.x * blockDim.x + threadIdx.x) >> 6;
  const int nwaves = (gridDim.x * blockDim.x) >> 6;
  for (uint32_t u = wave; u < n; u += nwaves) {
    uint32_t r = 0;
    if (lane == 0) r = find_or_insert(t, keys[u]);
    r = __shfl(r, 0, 64);
    if (urow_out && lane == 0) urow_out[u] = r;
    const float* g = grads + (size_t)u * stride;
    const float4 g0 = ld4(g);
    const bool had_v = g0.y != 0.0f;
    RowHdr* hp = t.hdr + r;
    if (need_init && lane == 0) need_init[u] = 0;
    if (lane == 0) {
      const float w_old = hp->w;
      float sqrt_g = hp->sqrt_g, z = hp->z;
      const float w_new = ftrl_update_w(g0.x, w_old, sqrt_g, z, t.p);
      hp->w = w_new;
      hp->sqrt_g = sqrt_g;
      hp->z = z;
      if (w_old == 0 && w_new != 0 && t.k > 0 && hp->has_V == 0 && hp->fea_cnt > (float)t.p.V_threshold) {
        if (t.p.init_mode == DFH_INIT_HASH) {
          init_v_hash_row(t, r, keys[u]);
          hp->has_V = 1;
        } else if (need_init) {
          need_init[u] = 1;
        }
      }
    }
    if (had_v && hp->has_V == 0) {  // CHECK(e.V != nullptr), sgd_updater.cc:92
      if (lane == 0) atomicOr(t.err, 4u);
    } else if (had_v) {
      float* va = t.va + (size_t)r * (2 * t.kp);
      for (int d = lane; d < t.k; d += 64) {
        float vv = va[d], acc = va[t.kp + d];
        adagrad_update_v(g[4 + d], vv, acc, t.p);
        va[d] = vv;
        va[t.kp + d] = acc;
      }
    }
  }
}

// ---------------------------------------------------------------------------
// Resolved form: the keys an owner receives from G source ranks are
// resolved to table rows ONCE per step (k_resolve, duplicates across sources
// allowed), then Pull is one gather over all of them and the two Push kinds run
// per source rank on known rows (no probing, sequential in source order).
// ---------------------------------------------------------------------------
__global__ void k_resolve(TableView t, const uint64_t* __restrict__ keys, uint32_t n, uint32_t* __restrict__ rowid) {
  for (uint32_t u = blockIdx.x * blockDim.x + threadIdx.x; u < n; u += gridDim.x * blockDim.x)
    rowid[u] = find_or_insert(t, keys[u]);
}

// Pull on resolved rows: L lanes per key copy the row (float4 per lane)
template <int L>
__global__ void __launch_bounds__(256) k_pull_resolved(TableView t, const uint32_t* __restrict__ rowid, uint32_t n,
                                                       float* __restrict__ rows, size_t stride) {
  const LaneGroup<L> ln(t);
  for (uint32_t u = ln.group; u < n; u += ln.ngroups) {
    const uint32_t r = rowid[u] & kRowMask;  // (k_resolve_multi marks a key's worker entry in bit 31)
    const float4 h0 = ld4(reinterpret_cast<const float*>(t.hdr + r));  // {w, has_V, sqrt_g, z}
    const bool hv = __float_as_uint(h0.y) != 0u;
    const float* va = t.va + (size_t)r * (2 * t.kp);
    put_pull_row(rows + (size_t)u * stride, ln.sub == 0, h0.x, hv, ln.d, ln.d_ok, hv && ln.d_ok ? ld4(va + ln.d) : zero4());
  }
}

// Push(kGradient) on resolved rows of ONE source rank (unique inside the launch): L lanes per key, no step word
template <int L>
__global__ void __launch_bounds__(256) k_push_grad_resolved(TableView t, const uint32_t* __restrict__ rowid,
                                                            const uint64_t* __restrict__ keys, uint32_t n,
                                                            const float* __restrict__ grads, size_t stride) {
  const LaneGroup<L> ln(t);
  for (uint32_t u = ln.group; u < n; u += ln.ngroups) {
    RowRegs<L, false> row(t, ln);
    row.load(rowid[u] & kRowMask);
    const float* g = grads + (size_t)u * stride;
    const float4 g0 = ld4(g);
    const float4 gv = ld4(g + ln.goff);
    if (row.refuse(g0.y != 0.0f)) row.had_v = false;  // flagged; like k_push_grad this form still takes the row's w step
    row.apply(g0.x, gv, keys + u);
    row.store();
  }
}

// ---------------------------------------------------------------------------
// Per entry: one launch for all source ranks of a step (the election and the layout: head of the file)
// ---------------------------------------------------------------------------
__global__ void k_resolve_multi(TableView t, const uint64_t* __restrict__ keys, SegOff g, uint32_t* __restrict__ rowid) {
  const uint32_t n = g.off[g.nsrc];
  const uint32_t XS = multi_xs(g.nsrc);
  uint32_t* __restrict__ extra = rowid + multi_extra_base(n);
  for (uint32_t e = blockIdx.x * blockDim.x + threadIdx.x; e < n; e += gridDim.x * blockDim.x) {
    const uint32_t r = find_or_insert(t, keys[e]);
    uint32_t* word = &t.hdr[r].pad[g.slot];
    uint32_t old = atomicCAS(word, 0u, (e + 1) << 5);
    const bool worker = old == 0u;
    if (!worker) {  // the key has its worker: take a place among its extras
      // A source's list is unique, so a key has at most nsrc - 1 <= XS extras.  More entries on one row are an error of the
      // caller (a list that repeats a key) or a table that overflowed (find_or_insert parks every key beyond the capacity on
      // the last row): flagged, and the count SATURATES — the Push kernels are queued before the host reads the error word,
      // and a count beyond the extras (or a carry out of the low five bits into the worker's index) would have them read
      // indices that were never written.
      const uint32_t lim = (uint32_t)(g.nsrc - 1);
      for (;;) {
        if ((old & 31u) >= lim) {
          atomicOr(t.err, 2u);
          break;
        }
        const uint32_t seen = atomicCAS(word, old, old + 1u);
        if (seen == old) {
          extra[(size_t)((old >> 5) - 1u) * XS + (old & 31u)] = e;
          break;
        }
        old = seen;
      }
    }
    rowid[e] = r | (worker ? ROW_WORKER : 0u);
  }
}

__global__ void k_release_rows(TableView t, const uint32_t* __restrict__ rowid, uint32_t n, int slot) {
  for (uint32_t e = blockIdx.x * blockDim.x + threadIdx.x; e < n; e += gridDim.x * blockDim.x) {
    const uint32_t rw = rowid[e];
    if (rw & ROW_WORKER) t.hdr[rw & kRowMask].pad[slot] = 0;
  }
}

// Push(kFeaCount) of all sources: one thread per entry, the key's worker adds every source's count
// (small integers: the sum is exact in any order) and then takes the InitV decision once —
// w does not change during count pushes and fea_cnt only grows, so the outcome equals the
// sequential one (sgd_updater.cc:62-73)
__global__ void k_push_count_multi(TableView t, const uint32_t* __restrict__ rowid, const uint64_t* __restrict__ keys,
                                   SegOff g, const float* __restrict__ cnt) {
  const uint32_t n = g.off[g.nsrc];
  const uint32_t XS = multi_xs(g.nsrc);
  const uint32_t* __restrict__ extra = rowid + multi_extra_base(n);
  for (uint32_t e = blockIdx.x * blockDim.x + threadIdx.x; e < n; e += gridDim.x * blockDim.x) {
    const uint32_t rw = rowid[e];
    if (!(rw & ROW_WORKER)) continue;  // another entry of this key works for it
    const uint32_t r = rw & kRowMask;
    RowHdr& h = t.hdr[r];
    float fc = h.fea_cnt + cnt[e];
    const uint32_t m = min(h.pad[g.slot] & 31u, XS);
    for (uint32_t i = 0; i < m; ++i) fc += cnt[extra[(size_t)e * XS + i]];
    h.fea_cnt = fc;
    if (t.k > 0 && h.has_V == 0 && h.w != 0 && fc > (float)t.p.V_threshold) {
      init_v_hash_row(t, r, keys[e]);
      h.has_V = 1;
    }
  }
}

// Push(kGradient) of all sources: L lanes per entry; the key's worker applies the sources' gradient rows
// one after the other (FTRL on w with lazy InitV, AdaGrad on V iff the rows were pulled with V) on
// registers and stores the row once; clears the row's step word.  The header, the worker's own gradient
// row, the V / accumulator slices and the extras are requested together, before anything is known about
// the key: a key of one source (80 %) is row word -> {header, row, gradient} -> store, a key of several
// sources one round trip more (the other sources' gradient rows, four at a time).
template <int L>
__global__ void __launch_bounds__(256) k_push_grad_multi(TableView t, const uint32_t* __restrict__ rowid,
                                                         const uint64_t* __restrict__ keys, SegOff g,
                                                         const float* __restrict__ grads, size_t stride) {
  const LaneGroup<L> ln(t);
  const uint32_t n = g.off[g.nsrc];
  const uint32_t XS = multi_xs(g.nsrc);
  const uint32_t* __restrict__ extra = rowid + multi_extra_base(n);
  for (uint32_t e = ln.group; e < n; e += ln.ngroups) {
    const uint32_t rw = rowid[e];
    if (!(rw & ROW_WORKER)) continue;
    // one round trip: the row, its step word, the own gradient row, the extras
    RowRegs<L, true> row(t, ln, g.slot);
    row.load(rw & kRowMask);
    const uint32_t word = row.hp->pad[g.slot];
    const float* g_own = grads + (size_t)e * stride;
    const float4 go0 = ld4(g_own);
    const float4 go_v = ld4(g_own + ln.goff);
    const uint32_t* xp = extra + (size_t)e * XS;
    const uint4 x0 = *reinterpret_cast<const uint4*>(xp);
    const uint4 x1 = *reinterpret_cast<const uint4*>(xp + (XS >= 8 ? 4 : 0));
    if (row.refuse(go0.y != 0.0f)) continue;
    const uint64_t* key = keys + e;
    const uint32_t m = min(word & 31u, XS);  // entries of this key besides the worker's own
    if (m == 0) {                   // the usual case: one source carries the key
      row.apply(go0.x, go_v, key);
    } else if (m < MULTI_FAST) {
      // the worker's and the other sources' entries in ascending order
      uint32_t ent[MULTI_FAST] = {e, x0.x, x0.y, x0.z, x0.w, x1.x, x1.y, x1.z};
      sort8(ent, m + 1);
      // four gradient rows per round trip (unconditional loads on clamped entries), applied in order
#pragma unroll
      for (int b0 = 0; b0 < MULTI_FAST; b0 += 4) {
        if ((uint32_t)b0 > m) break;  // uniform per lane group
        float gws[4];
        float4 gvs[4];
#pragma unroll
        for (int i = 0; i < 4; ++i) {
          const float* gp = grads + (size_t)((uint32_t)(b0 + i) <= m ? ent[b0 + i] : e) * stride;
          gws[i] = ld4(gp).x;
          gvs[i] = ld4(gp + ln.goff);
        }
#pragma unroll
        for (int i = 0; i < 4; ++i)
          if ((uint32_t)(b0 + i) <= m) row.apply(gws[i], gvs[i], key);
      }
    } else {
      // more than 8 sources carry the key: the next entry is searched among the worker's own and its extras for every application
      for (uint32_t done = 0, from = 0; done <= m; ++done) {
        const uint32_t x = next_ascending(xp, m, e, from);
        const float* gp = grads + (size_t)x * stride;
        row.apply(ld4(gp).x, ld4(gp + ln.goff), key);
        from = x + 1;
      }
    }
    row.store();
  }
}

// ---------------------------------------------------------------------------
// Per DISTINCT key (round 6).  k_count_pull_multi is Push(kFeaCount) of all sources and Pull in ONE launch:
// a key's worker adds the sources' counts, takes the InitV decision once (sgd_updater.cc:62-73), reads the row ONCE and
// writes [w, has_V, 0, 0 | V] to the output row of every entry of the key (its own and its extras') — the duplicate keys of
// k_pull_resolved re-read their row (81.7 MB counted for 58.8 MB at N = 8 size), and the count push was a launch of its own.
// On the way it leaves the step's keys as lists per chunk of MULTI_CH entries (layout above), so that k_push_grad_chunks
// runs over keys, not entries: in k_push_grad_multi 36 % of the lane groups idle on entries that are not workers and a
// wave takes the several-sources path (a third round trip) when ONE of its four keys has extras — 59 % of the waves for
// 20 % of the keys.  Here a wave's keys are all of one kind, the keys of several sources have their other entries in
// source order with the first read, and their gradient rows are requested with the row: two round trips for both kinds.
// ---------------------------------------------------------------------------
template <int L, bool HAS_CNT>
__global__ void __launch_bounds__(256) k_count_pull_multi(TableView t, uint32_t* __restrict__ rowid, const uint64_t* __restrict__ keys,
                                                          SegOff g, const float* __restrict__ cnt, float* __restrict__ rows,
                                                          size_t stride) {
  __shared__ uint32_t sh_n[2];
  const LaneGroup<L> ln(t);
  const int d = ln.d;
  const uint32_t n = g.off[g.nsrc];
  const uint32_t XS = multi_xs(g.nsrc), RS = XS + 4;
  const uint32_t* __restrict__ extra = rowid + multi_extra_base(n);
  uint2* __restrict__ slist = reinterpret_cast<uint2*>(rowid + multi_slist_base(n, g.nsrc));
  uint32_t* __restrict__ mrec = rowid + multi_mrec_base(n, g.nsrc);
  uint2* __restrict__ chdr = reinterpret_cast<uint2*>(rowid + multi_chdr_base(n, g.nsrc));
  const uint32_t nchunk = (n + MULTI_CH - 1) / MULTI_CH;
  for (uint32_t c = blockIdx.x; c < nchunk; c += gridDim.x) {
    if (threadIdx.x == 0) sh_n[0] = sh_n[1] = 0;
    __syncthreads();
    for (uint32_t i = ln.grp; i < MULTI_CH; i += ln.GPB) {
      const uint32_t e = c * MULTI_CH + i;
      if (e >= n) continue;
      const uint32_t rw = rowid[e];
      if (!(rw & ROW_WORKER)) continue;  // another entry of this key works for it
      const uint32_t r = rw & kRowMask;
      RowHdr* hp = t.hdr + r;
      const float* va = t.va + (size_t)r * (2 * t.kp);
      // one round trip: the header (both halves), this lane's V slice, the extras
      const float4 h0 = ld4(reinterpret_cast<const float*>(hp));  // {w, has_V, sqrt_g, z}
      const float fea_cnt = hp->fea_cnt;
      const uint32_t word = hp->pad[g.slot];
      float4 v = ld4(ln.d_ok ? va + d : reinterpret_cast<const float*>(hp));
      const uint32_t* xp = extra + (size_t)e * XS;
      const uint4 x0 = *reinterpret_cast<const uint4*>(xp);
      const uint4 x1 = *reinterpret_cast<const uint4*>(xp + (XS >= 8 ? 4 : 0));
      const uint32_t m = min(word & 31u, XS);  // entries of this key besides the worker's own
      bool hv = __float_as_uint(h0.y) != 0u;
      // the other entries in ascending order: in registers (m <= XS masks the second read of four extras); more than 8 are
      // ordered by selection out of memory, below
      uint32_t ent[MULTI_FAST] = {x0.x, x0.y, x0.z, x0.w, x1.x, x1.y, x1.z, x1.w};
      const bool fast = m <= (uint32_t)MULTI_FAST;
      if (m > 0 && fast) sort8(ent, m);
      if (HAS_CNT) {
        float fc = fea_cnt + cnt[e];  // small integers: the sum is exact in any order
        if (fast) {
#pragma unroll
          for (int j = 0; j < MULTI_FAST; ++j)
            if ((uint32_t)j < m) fc += cnt[ent[j]];
        } else {
          for (uint32_t j = 0; j < m; ++j) fc += cnt[xp[j]];
        }
        if (t.k > 0 && !hv && h0.x != 0 && fc > (float)t.p.V_threshold) {
          // every lane of the group writes its own 16 B of V and of the accumulators, and answers with what it wrote
          if (ln.d_ok) {
            init_v_hash_slice(t, r, keys[e], d);
            v.x = d + 0 < t.k ? hash_init_value(keys[e], d + 0, t.p.seed, t.p.V_init_scale) : 0.0f;
            v.y = d + 1 < t.k ? hash_init_value(keys[e], d + 1, t.p.seed, t.p.V_init_scale) : 0.0f;
            v.z = d + 2 < t.k ? hash_init_value(keys[e], d + 2, t.p.seed, t.p.V_init_scale) : 0.0f;
            v.w = d + 3 < t.k ? hash_init_value(keys[e], d + 3, t.p.seed, t.p.V_init_scale) : 0.0f;
          }
          hv = true;
          if (ln.sub == 0) hp->has_V = 1;
        }
        if (ln.sub == 0) hp->fea_cnt = fc;
      }
      if (!hv) v = zero4();
      auto put = [&](uint32_t idx) { put_pull_row(rows + (size_t)idx * stride, ln.sub == 0, h0.x, hv, d, ln.d_ok, v); };
      put(e);
      if (fast) {
#pragma unroll
        for (int j = 0; j < MULTI_FAST; ++j)
          if ((uint32_t)j < m) put(ent[j]);
      } else {
        for (uint32_t j = 0; j < m; ++j) put(xp[j]);
      }
      if (ln.sub == 0) {
        if (m == 0) {
          slist[(size_t)c * MULTI_CH + atomicAdd(&sh_n[0], 1u)] = make_uint2(e, r);
        } else {
          uint32_t* rec = mrec + ((size_t)c * MULTI_CH + atomicAdd(&sh_n[1], 1u)) * RS;
          *reinterpret_cast<uint4*>(rec) = make_uint4(e | (m << 27), r, 0u, 0u);
          if (fast) {
            *reinterpret_cast<uint4*>(rec + 4) = make_uint4(ent[0], ent[1], ent[2], ent[3]);
            if (XS >= 8) *reinterpret_cast<uint4*>(rec + 8) = make_uint4(ent[4], ent[5], ent[6], ent[7]);
          } else {
            for (uint32_t done = 0, from = 0; done < m; ++done) {
              rec[4 + done] = next_ascending(xp, m, NO_ENTRY, from);
              from = rec[4 + done] + 1;
            }
          }
        }
      }
    }
    __syncthreads();
    if (threadIdx.x == 0) chdr[c] = make_uint2(sh_n[0], sh_n[1]);
    __syncthreads();
  }
}

// Push(kGradient) of all sources over the key lists of k_count_pull_multi: L lanes per KEY, a block per chunk; FTRL on w
// with lazy InitV, AdaGrad on V iff the rows were pulled with V, the sources' gradient rows applied in source order on
// registers, the row stored once, its step word cleared (what k_push_grad_multi does per entry).
template <int L>
__global__ void __launch_bounds__(256) k_push_grad_chunks(TableView t, const uint32_t* __restrict__ rowid,
                                                          const uint64_t* __restrict__ keys, SegOff g,
                                                          const float* __restrict__ grads, size_t stride) {
  const LaneGroup<L> ln(t);
  const uint32_t n = g.off[g.nsrc];
  const uint32_t XS = multi_xs(g.nsrc), RS = XS + 4;
  const uint2* __restrict__ slist = reinterpret_cast<const uint2*>(rowid + multi_slist_base(n, g.nsrc));
  const uint32_t* __restrict__ mrec = rowid + multi_mrec_base(n, g.nsrc);
  const uint2* __restrict__ chdr = reinterpret_cast<const uint2*>(rowid + multi_chdr_base(n, g.nsrc));
  const uint32_t nchunk = (n + MULTI_CH - 1) / MULTI_CH;
  RowRegs<L, true> row(t, ln, g.slot);
  for (uint32_t c = blockIdx.x; c < nchunk; c += gridDim.x) {
    const uint2 ch = chdr[c];
    const size_t base = (size_t)c * MULTI_CH;
    uint2 en = slist[base + min(ln.grp, MULTI_CH - 1)];  // requested with the chunk's counts
    uint4 r0 = *reinterpret_cast<const uint4*>(mrec + (base + min(ln.grp, MULTI_CH - 1)) * RS);
    // ---- keys of one source: row word -> {header, row, gradient} -> store
    for (uint32_t i = ln.grp; i < ch.x; i += ln.GPB) {
      if (i != ln.grp) en = slist[base + i];
      const uint32_t e = en.x;
      row.load(en.y);
      const float* g_own = grads + (size_t)e * stride;
      const float4 go0 = ld4(g_own);
      const float4 go_v = ld4(g_own + ln.goff);
      if (row.refuse(go0.y != 0.0f)) continue;
      row.apply(go0.x, go_v, keys + e);
      row.store();
    }
    // ---- keys of several sources: record -> {header, row, the first four gradient rows} -> [the others] -> store
    for (uint32_t i = ln.grp; i < ch.y; i += ln.GPB) {
      const uint32_t* rec = mrec + (base + i) * RS;
      if (i != ln.grp) r0 = *reinterpret_cast<const uint4*>(rec);
      const uint4 x0 = *reinterpret_cast<const uint4*>(rec + 4);
      const uint32_t e = r0.x & 0x07FFFFFFu, m = r0.x >> 27;
      row.load(r0.y);
      const float* g_own = grads + (size_t)e * stride;
      const float4 go0 = ld4(g_own);
      const float4 go_v = ld4(g_own + ln.goff);
      if (row.refuse(go0.y != 0.0f)) continue;
      const uint64_t* key = keys + e;
      // the first four of the other entries' gradient rows travel with the row (unconditional loads on clamped entries)
      const uint32_t xs[4] = {x0.x, x0.y, x0.z, x0.w};
      float gws[4];
      float4 gvs[4];
#pragma unroll
      for (int j = 0; j < 4; ++j) {
        const float* gp = grads + (size_t)((uint32_t)j < m ? xs[j] : e) * stride;
        gws[j] = ld4(gp).x;
        gvs[j] = ld4(gp + ln.goff);
      }
      bool own_done = false;  // the worker's own entry takes its place in the ascending order
#pragma unroll
      for (int j = 0; j < 4; ++j) {
        if ((uint32_t)j < m) {
          if (!own_done && e < xs[j]) {
            row.apply(go0.x, go_v, key);
            own_done = true;
          }
          row.apply(gws[j], gvs[j], key);
        }
      }
      for (uint32_t j = 4; j < m; ++j) {  // rare: a key five or more sources carry
        const uint32_t x = rec[4 + j];
        const float* gp = grads + (size_t)x * stride;
        const float gw = ld4(gp).x;
        const float4 gv = ld4(gp + ln.goff);
        if (!own_done && e < x) {
          row.apply(go0.x, go_v, key);
          own_done = true;
        }
        row.apply(gw, gv, key);
      }
      if (!own_done) row.apply(go0.x, go_v, key);
      row.store();
    }
  }
}

}  // namespace dfh
#endif  // DFH_OWNER_HIP_
