// dfh_index.hip — the key index of a table (HEntry[H], open addressing, linear probing): find_or_insert for one thread,
// find_or_insert_block for a block of distinct keys, find_only, and k_rehash for growth; then the kernels that take a whole
// table as arrays of keys and rows: k_warm_start, k_export, k_import.  The probes are device functions, used by the lookup
// passes (dfh_lookup.hip), the Localizer's probing emit (dfh_localize.hip) and the owner side of the store (dfh_owner.hip);
// the kernels are launched by dfh_table.hip.
#ifndef DFH_INDEX_HIP_
#define DFH_INDEX_HIP_
#include "dfh_updater.h"   // hash_init_value (k_warm_start); lane_id by way of dfh_device.h

namespace dfh {

// ---- key index: open addressing, linear probing.  Launches that probe the table may run
// concurrently (preparation streams resolve the keys of later minibatches while the main stream
// pulls, pushes or imports) and may carry the same new key, inside one launch (owner side of the
// sharded store: several source ranks) or across launches.  The thread that wins a slot's 64-bit
// CAS takes the next row and publishes its id with a device-scope atomic store; every other
// carrier of the key finds the key in the slot and waits for the id (the table is created with
// all row words = ~0).  A row id is the whole message: rows are zero until an update writes them.
__device__ __forceinline__ uint32_t find_or_insert(const TableView& t, uint64_t key) {
  uint64_t h = splitmix64(key) & t.hmask;
  // Two lanes of ONE wavefront may carry the same new key (k_resolve_multi: several source ranks), and lanes of a
  // wavefront make progress together: a lane waiting for a row id must not keep the winner of its slot from storing it.
  // Every iteration is therefore straight-line: (1) claim, (2) the winners publish, (3) everyone looks — in program
  // order, no early exit between them, so that (2) of a winner always precedes (3) of the lanes that share its
  // wavefront.  The wait is bounded: a slot whose row id never appears sets error bit 3 instead of hanging the device.
  for (uint32_t spins = 0;;) {
    uint64_t k = __hip_atomic_load(&t.ht[h].key, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
    bool won = false;
    if (k == kEmptyKey) {
      const unsigned long long old = atomicCAS(reinterpret_cast<unsigned long long*>(&t.ht[h].key),
                                               (unsigned long long)kEmptyKey, (unsigned long long)key);
      won = old == kEmptyKey;
      k = won ? key : (uint64_t)old;
    }
    uint32_t r = kNoRow;
    if (won) {
      r = atomicAdd(t.nrows, 1u);
      if (r >= t.capacity) {
        atomicOr(t.err, 1u);
        r = t.capacity - 1;  // keep memory safe; the host reports DFH_ERR_CAPACITY
      }
      __hip_atomic_store(&t.ht[h].row, r, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
    }
    if (k == key) {
      if (!won) r = __hip_atomic_load(&t.ht[h].row, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
      if (r != kNoRow) return r;
      if (++spins > (1u << 22)) {  // seconds: the winner of this slot is gone
        atomicOr(t.err, 8u);
        return 0u;
      }
      __builtin_amdgcn_s_sleep(1);
      continue;  // the winner of this slot (another wavefront) is between its CAS and its store
    }
    h = (h + 1) & t.hmask;
  }
}

// growth of a table (dfh_table.hip table_grow): every {key, row} of the old index into the new, larger one.  Runs alone on
// the table (every stream drained); distinct keys only race for slots.
__global__ void k_rehash(const HEntry* __restrict__ old_ht, uint64_t old_slots, HEntry* __restrict__ ht, uint64_t hmask) {
  for (uint64_t i = blockIdx.x * (uint64_t)blockDim.x + threadIdx.x; i < old_slots; i += (uint64_t)gridDim.x * blockDim.x) {
    const uint64_t key = old_ht[i].key;
    if (key == kEmptyKey) continue;
    uint64_t h = splitmix64(key) & hmask;
    for (;;) {
      const unsigned long long old = atomicCAS(reinterpret_cast<unsigned long long*>(&ht[h].key), (unsigned long long)kEmptyKey,
                                               (unsigned long long)key);
      if (old == kEmptyKey) {
        ht[h].row = old_ht[i].row;
        break;
      }
      h = (h + 1) & hmask;
    }
  }
}

// find_or_insert for a whole 256-thread block of DISTINCT keys (k_lookup: one thread per unique key of a minibatch), rows
// handed out per BLOCK: the threads that win a slot are counted (ballot, one LDS atomic per wavefront) and ONE atomicAdd on the
// table's row counter serves them all.  Every row a launch allocates used to cost an atomic on that one address per
// wavefront with a winner, and same-address atomics serialise at ~12 ns each on this part: a first-epoch minibatch (every key
// new: ~147 000 inserts) queued ~1 600 of them, ~20 us of one memory channel's time beside whatever else ran (profiles/r05j_*:
// "probe + 20 us"), now a quarter of that.  Same protocol as find_or_insert towards concurrent launches: a slot's winner publishes
// the row id with a device-scope store, other carriers of the key wait for it — but only AFTER this block's own winners have
// published (nobody waits inside the counted phase: a block that waited there could hold back the winner it waits for).
// All threads of the block call it together (`active`: this thread has a key); sh: 8 shared words.
__device__ __forceinline__ uint32_t find_or_insert_block(const TableView& t, uint64_t key, bool active, uint32_t* sh) {
  const int lane = threadIdx.x & 63, w = threadIdx.x >> 6;
  __syncthreads();  // sh may still be read from the previous call
  if (threadIdx.x == 0) sh[0] = 0u;
  __syncthreads();
  uint64_t h = splitmix64(key) & t.hmask;
  uint32_t r = kNoRow;
  bool won = false, pending = false;
  if (active) {
    for (;;) {
      uint64_t k = __hip_atomic_load(&t.ht[h].key, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
      if (k == kEmptyKey) {
        const unsigned long long old = atomicCAS(reinterpret_cast<unsigned long long*>(&t.ht[h].key), (unsigned long long)kEmptyKey,
                                                 (unsigned long long)key);
        if (old == kEmptyKey) {
          won = true;
          break;
        }
        k = (uint64_t)old;
      }
      if (k == key) {
        r = __hip_atomic_load(&t.ht[h].row, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
        pending = r == kNoRow;  // its winner (another launch) is between its CAS and its store: looked at again below
        break;
      }
      h = (h + 1) & t.hmask;
    }
  }
  // rows for this block's winners: rank inside the wavefront from the ballot, the wavefront's offset from one LDS atomic
  const unsigned long long m = __ballot(won);
  uint32_t woff = 0;
  if (lane == 0 && m) woff = atomicAdd(&sh[0], (uint32_t)__popcll(m));
  woff = __shfl(woff, 0, 64);
  __syncthreads();
  if (threadIdx.x == 0) sh[1] = sh[0] ? atomicAdd(t.nrows, sh[0]) : 0u;
  __syncthreads();
  if (won) {
    r = sh[1] + woff + (uint32_t)__popcll(m & ((1ull << lane) - 1ull));
    if (r >= t.capacity) {
      atomicOr(t.err, 1u);
      r = t.capacity - 1;  // keep memory safe; the host reports DFH_ERR_CAPACITY
    }
    __hip_atomic_store(&t.ht[h].row, r, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
  }
  if (pending) {
    for (uint32_t spins = 0;; ++spins) {
      r = __hip_atomic_load(&t.ht[h].row, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
      if (r != kNoRow) break;
      if (spins > (1u << 22)) {  // seconds: the winner of this slot is gone
        atomicOr(t.err, 8u);
        r = 0u;
        break;
      }
      __builtin_amdgcn_s_sleep(1);
    }
  }
  (void)w;
  return r;
}

// read-only probe (export / tests)
__device__ __forceinline__ uint32_t find_only(const TableView& t, uint64_t key) {
  uint64_t h = splitmix64(key) & t.hmask;
  for (;;) {
    uint64_t k = t.ht[h].key;
    if (k == key) return t.ht[h].row;
    if (k == kEmptyKey) return kNoRow;
    h = (h + 1) & t.hmask;
  }
}

// warm start (model preload for benchmarks / resume): one wave per unique key:
// row gets w = w0, fea_cnt = cnt0 and an allocated, hash-initialised V.
__global__ void __launch_bounds__(256) k_warm_start(TableView t, const uint64_t* __restrict__ keys, uint64_t n, float w0,
                                                    float cnt0) {
  const int lane = lane_id();
  const uint64_t wave = (blockIdx.x * (uint64_t)blockDim.x + threadIdx.x) >> 6;
  const uint64_t nwaves = ((uint64_t)gridDim.x * blockDim.x) >> 6;
  for (uint64_t u = wave; u < n; u += nwaves) {
    const uint64_t key = keys[u];
    uint32_t r = 0;
    if (lane == 0) r = find_or_insert(t, key);
    r = __shfl(r, 0, 64);
    if (lane == 0) {
      RowHdr h = {};
      h.w = w0;
      h.has_V = t.k > 0 ? 1u : 0u;
      h.sqrt_g = 0.f;
      h.z = 0.f;
      h.fea_cnt = cnt0;
      h.pad[0] = h.pad[1] = h.pad[2] = 0;
      t.hdr[r] = h;
    }
    float* va = t.va + (size_t)r * (2 * t.kp);
    for (int d = lane; d < t.kp; d += 64) {
      va[d] = d < t.k ? hash_init_value(key, d, t.p.seed, t.p.V_init_scale) : 0.0f;
      va[t.kp + d] = 0.0f;
    }
  }
}

// table export: one thread per hash slot
__global__ void k_export(TableView t, uint64_t nslots, uint64_t cap, uint64_t* keys, float* scal, int* has_V, float* V,
                         unsigned long long* counter) {
  for (uint64_t s = blockIdx.x * (uint64_t)blockDim.x + threadIdx.x; s < nslots; s += (uint64_t)gridDim.x * blockDim.x) {
    const uint64_t key = t.ht[s].key;
    if (key == kEmptyKey) continue;
    const unsigned long long o = atomicAdd(counter, 1ULL);
    if (o >= cap) continue;
    const uint32_t r = t.ht[s].row;
    const RowHdr h = t.hdr[r];
    keys[o] = key;
    scal[o * 4 + 0] = h.fea_cnt;
    scal[o * 4 + 1] = h.w;
    scal[o * 4 + 2] = h.sqrt_g;
    scal[o * 4 + 3] = h.z;
    has_V[o] = h.has_V ? 1 : 0;
    if (t.k > 0) {
      const float* va = t.va + (size_t)r * (2 * t.kp);
      for (int d = 0; d < t.k; ++d) {
        V[o * 2 * t.k + d] = h.has_V ? va[d] : 0.f;
        V[o * 2 * t.k + t.k + d] = h.has_V ? va[t.kp + d] : 0.f;
      }
    }
  }
}

__global__ void k_import(TableView t, uint64_t n, const uint64_t* keys, const float* scal, const int* has_V, const float* V) {
  for (uint64_t i = blockIdx.x * (uint64_t)blockDim.x + threadIdx.x; i < n; i += (uint64_t)gridDim.x * blockDim.x) {
    const uint32_t r = find_or_insert(t, keys[i]);
    RowHdr h = {};
    h.fea_cnt = scal[i * 4 + 0];
    h.w = scal[i * 4 + 1];
    h.sqrt_g = scal[i * 4 + 2];
    h.z = scal[i * 4 + 3];
    h.has_V = has_V[i] ? 1u : 0u;
    h.pad[0] = h.pad[1] = h.pad[2] = 0;
    t.hdr[r] = h;
    if (t.k > 0) {
      float* va = t.va + (size_t)r * (2 * t.kp);
      for (int d = 0; d < t.kp; ++d) {
        va[d] = (has_V[i] && d < t.k) ? V[i * 2 * t.k + d] : 0.f;
        va[t.kp + d] = (has_V[i] && d < t.k) ? V[i * 2 * t.k + t.k + d] : 0.f;
      }
    }
  }
}

}  // namespace dfh
#endif  // DFH_INDEX_HIP_
