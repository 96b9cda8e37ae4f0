// dfh_auc.hip — BinClassMetric::AUC of one minibatch's predictions (src/loss/bin_class_metric.h:35-56), times n, in two
// forms that count the same pairs:
//   pairs   n <= AUC_PAIRS_MAX_N: every (positive, negative) pair is compared, no sort.  Units of 256 rows (auc_pairs_block)
//           run as blocks of k_auc_pairs or as a role of k_update_fused (dfh_update.hip); auc_finalize_block adds their slots
//           up, in k_auc_finalize or in the first block of the next step's lookup (dfh_lookup.hip).
//   sort    beyond (n^2 would pass the cost of sorting): k_auc_keys, a library radix sort of (image of pred, label),
//           k_auc_area over the sorted labels.
// Both order predictions by auc_key and end in auc_times_n.  The host side, one function for either form, is
// dfh_auc_api.hip.  (The whole-set evaluator of dfh_eval.hip has tie and NaN rules of its own, on purpose.)
#ifndef DFH_AUC_HIP_
#define DFH_AUC_HIP_
#include "dfh_device.h"

namespace dfh {

// order-preserving u32 image of a prediction
__device__ __forceinline__ uint32_t auc_key(float pred) {
  const uint32_t bits = __float_as_uint(pred + 0.0f);  // -0 and +0 compare equal in the reference: one image
  return (bits & 0x80000000u) ? ~bits : (bits | 0x80000000u);
}

// BinClassMetric::AUC without a sort, for minibatch-sized n: the reference's area is the number of
// (positive j, negative i) pairs in which j comes before i in the sorted order (bin_class_metric.h:44-50),
// and "before" can be decided pair by pair: pred_j < pred_i, ties by index (the order a stable sort gives;
// std::sort leaves the order of ties unspecified).  The count is an integer: exact, whatever the order.
// Round 4: only positive columns are compared (a tile of AUC_TILE examples is compacted to its positives in LDS,
// any order) and (image of pred, index) is ONE 64-bit key, so a pair costs a broadcast LDS read, one v_cmp_lt_u64
// and one add-with-carry: ~2e7 pairs of 2 VALU operations for a 10 000-row minibatch with 25 % positives, where
// round 3 spent 1e8 pairs of 7.  auc_pairs_block is one unit of work: 256 rows (this block's threads) against the
// column tiles ct, ct + nct, ...; units are independent, write their count to a slot of their own — no atomics,
// no fence, no ticket (round 3's three same-address atomics + a device-scope fence per block were most of the
// kernel's 27 us) — and may run as blocks of k_auc_pairs or as a role of k_update_fused (the update launch has idle
// VALUs).  auc_finalize_block (one block, any later launch on the stream) adds the slots up and turns
// {area, positives} into AUC * n (:51-53).
constexpr int AUC_TILE = 1024;
constexpr uint32_t AUC_PAIRS_MAX_N = 32768;   // beyond: the radix-sort path (n^2 would pass the cost of sorting)
constexpr uint32_t AUC_COL_SPLIT = 16;        // column tiles are dealt to this many units per row tile (10 000 rows: one tile per unit)
constexpr uint32_t AUC_MAX_ROWTILES = AUC_PAIRS_MAX_N / 256;
constexpr uint32_t AUC_PART_WORDS = AUC_MAX_ROWTILES * (AUC_COL_SPLIT + 1);  // [units] counts | [row tiles] positives

__host__ __device__ inline uint32_t auc_nct(uint32_t n) {  // units per row tile
  const uint32_t ntile = (n + AUC_TILE - 1) / AUC_TILE;
  return ntile < AUC_COL_SPLIT ? ntile : AUC_COL_SPLIT;
}
__host__ __device__ inline uint32_t auc_units(uint32_t n) { return ((n + 255) / 256) * auc_nct(n); }

// a finished set of units waiting for its finalisation: part (device), n examples; n == 0: nothing pending
struct AucFin {
  const uint32_t* part;
  uint32_t n;
  double* out_slot;
};

// unit `unit` of auc_units(n): 256-thread blocks only.  part[unit] = pairs counted; part[auc_units(n) + rt] = positives of
// row tile rt (written by the tile's first unit)
constexpr size_t AUC_SMEM = (size_t)AUC_TILE * 8 + 16 * 4;  // working memory of auc_pairs_block
__device__ __forceinline__ void auc_pairs_block(const float* __restrict__ pred, const float* __restrict__ label, uint32_t n, uint32_t unit,
                                                uint32_t* __restrict__ part, char* smem /* AUC_SMEM bytes, 16 B aligned */) {
  unsigned long long* colp = reinterpret_cast<unsigned long long*>(smem);  // positives of the current column tile: image of pred_j << 32 | j
  uint32_t* red = reinterpret_cast<uint32_t*>(colp + AUC_TILE);            // [8]
  uint32_t& npos_tile = red[8];
  const uint32_t ntile = (n + AUC_TILE - 1) / AUC_TILE;
  const uint32_t nct = auc_nct(n);
  const uint32_t rt = unit / nct, ct = unit % nct;
  const uint32_t i = rt * 256u + threadIdx.x;
  unsigned long long ki = 0;
  bool neg = false, pos = false;
  if (i < n) {
    ki = ((unsigned long long)auc_key(pred[i]) << 32) | i;
    pos = label[i] > 0;
    neg = !pos;
  }
  uint32_t cnt = 0;
  const int lane = threadIdx.x & 63;
  for (uint32_t tile = ct; tile < ntile; tile += nct) {
    __syncthreads();  // the previous tile has been consumed
    if (threadIdx.x == 0) npos_tile = 0;
    const uint32_t j0 = tile * AUC_TILE;
    // all of the tile's loads first (one round trip), then the compaction: a ballot per wave and ONE LDS atomic per wave
    // and quarter
    float pj[AUC_TILE / 256], lj[AUC_TILE / 256];
#pragma unroll
    for (int r = 0; r < AUC_TILE / 256; ++r) {
      const uint32_t j = min(j0 + r * 256u + threadIdx.x, n - 1);
      pj[r] = pred[j];
      lj[r] = label[j];
    }
    __syncthreads();
#pragma unroll
    for (int r = 0; r < AUC_TILE / 256; ++r) {
      const uint32_t j = j0 + r * 256u + threadIdx.x;
      const bool pj_pos = j < n && lj[r] > 0;
      const unsigned long long m = __ballot(pj_pos);
      uint32_t base = 0;
      if (lane == 0 && m) base = atomicAdd(&npos_tile, (uint32_t)__popcll(m));
      base = __shfl(base, 0, 64);
      if (pj_pos) colp[base + __popcll(m & ((1ull << lane) - 1ull))] = ((unsigned long long)auc_key(pj[r]) << 32) | j;
    }
    __syncthreads();
    const uint32_t np = npos_tile;
#pragma unroll 8
    for (uint32_t t = 0; t < np; ++t) cnt += colp[t] < ki ? 1u : 0u;  // (pred_j, j) before (pred_i, i)
  }
  if (!neg) cnt = 0;
  uint32_t npos = pos ? 1u : 0u;
#pragma unroll
  for (int o = 32; o > 0; o >>= 1) {
    cnt += __shfl_xor(cnt, o, 64);
    npos += __shfl_xor(npos, o, 64);
  }
  __syncthreads();
  if (lane == 0) {
    red[threadIdx.x >> 6] = cnt;
    red[4 + (threadIdx.x >> 6)] = npos;
  }
  __syncthreads();
  if (threadIdx.x == 0) {
    part[unit] = red[0] + red[1] + red[2] + red[3];
    if (ct == 0) part[auc_units(n) + rt] = red[4] + red[5] + red[6] + red[7];
  }
}

// {area, positives, n} -> AUC * n, the end of either form (:51-53)
__device__ __forceinline__ double auc_times_n(double area, double tp, double n) {
  if (tp == 0.0 || tp == n) return 1.0;  // :51 (the reference returns 1, not n)
  const double a = area / (tp * (n - tp));
  return (a < 0.5 ? 1.0 - a : a) * n;
}

// one 256-thread block: the units' slots -> AUC * n, added to *out_slot
__device__ __forceinline__ void auc_finalize_block(const AucFin f) {
  __shared__ unsigned long long fsum[2][4];
  const uint32_t nu = auc_units(f.n), nrt = (f.n + 255) / 256;
  unsigned long long area = 0, tp = 0;
  for (uint32_t q = threadIdx.x; q < nu; q += 256u) area += f.part[q];
  for (uint32_t q = threadIdx.x; q < nrt; q += 256u) tp += f.part[nu + q];
#pragma unroll
  for (int o = 32; o > 0; o >>= 1) {
    area += __shfl_xor(area, o, 64);
    tp += __shfl_xor(tp, o, 64);
  }
  if ((threadIdx.x & 63) == 0) {
    fsum[0][threadIdx.x >> 6] = area;
    fsum[1][threadIdx.x >> 6] = tp;
  }
  __syncthreads();
  if (threadIdx.x == 0) {
    const double a_all = (double)(fsum[0][0] + fsum[0][1] + fsum[0][2] + fsum[0][3]);
    const double tpd = (double)(fsum[1][0] + fsum[1][1] + fsum[1][2] + fsum[1][3]);
    *f.out_slot += auc_times_n(a_all, tpd, (double)f.n);
  }
}

__global__ void __launch_bounds__(256) k_auc_pairs(const float* __restrict__ pred, const float* __restrict__ label, uint32_t n,
                                                   uint32_t* __restrict__ part) {
  __shared__ __attribute__((aligned(16))) char smem[AUC_SMEM];
  auc_pairs_block(pred, label, n, blockIdx.x, part, smem);
}
__global__ void __launch_bounds__(256) k_auc_finalize(AucFin f) { auc_finalize_block(f); }

// ---------------------------------------------------------------------------
// BinClassMetric::AUC (src/loss/bin_class_metric.h:35-56): sort by prediction,
// area = sum over negatives of the positives ranked below them.
// k_auc_keys: order-preserving u32 image of the float prediction + label bit.
// k_auc_area: one block walks the sorted labels (n is a minibatch: ~1e4).
// ---------------------------------------------------------------------------
__global__ void k_auc_keys(const float* __restrict__ pred, const float* __restrict__ label, uint32_t n,
                           uint32_t* __restrict__ keys, uint32_t* __restrict__ pos) {
  for (uint32_t i = blockIdx.x * blockDim.x + threadIdx.x; i < n; i += gridDim.x * blockDim.x) {
    keys[i] = auc_key(pred[i]);
    pos[i] = label[i] > 0 ? 1u : 0u;
  }
}

__global__ void __launch_bounds__(1024) k_auc_area(const uint32_t* __restrict__ sorted_pos, uint32_t n, double* __restrict__ out_slot) {
  __shared__ uint32_t wsum[16];
  __shared__ double dsum[16];
  uint32_t carry = 0;  // positives seen so far (identical in every thread)
  double area = 0.0;
  for (uint32_t base = 0; base < n; base += blockDim.x) {
    const uint32_t i = base + threadIdx.x;
    const uint32_t p = i < n ? sorted_pos[i] : 0u;
    uint32_t s = p;
#pragma unroll
    for (int o = 1; o < 64; o <<= 1) {
      const uint32_t y = __shfl_up(s, o, 64);
      if ((int)(threadIdx.x & 63) >= o) s += y;
    }
    __syncthreads();
    if ((threadIdx.x & 63) == 63) wsum[threadIdx.x >> 6] = s;
    __syncthreads();
    uint32_t woff = 0, tot = 0;
    for (int w = 0; w < 16; ++w) {
      if (w < (int)(threadIdx.x >> 6)) woff += wsum[w];
      tot += wsum[w];
    }
    if (i < n && p == 0) area += (double)(carry + woff + s);  // cum_tp at a negative
    carry += tot;
  }
  area = wave_sum_d(area);
  if ((threadIdx.x & 63) == 0) dsum[threadIdx.x >> 6] = area;
  __syncthreads();
  if (threadIdx.x == 0) {
    double a = 0.0;
    for (int w = 0; w < 16; ++w) a += dsum[w];
    *out_slot += auc_times_n(a, (double)carry, (double)n);
  }
}

}  // namespace dfh
#endif  // DFH_AUC_HIP_
