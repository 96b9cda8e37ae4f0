// dfh_device.h — what a lane does with its wavefront and with 16 bytes: lane id, sums over a wave, over a lane group and
// across groups, float4 loads and stores (plain and streaming), the zero-skipping multiply-add of SpMV.  No table, no
// minibatch: every kernel file of the library uses it.  64-lane wavefronts are assumed throughout.
#ifndef DFH_DEVICE_H_
#define DFH_DEVICE_H_
#include "dfh_internal.h"

namespace dfh {

// ---------------------------------------------------------------------------
// small device helpers
// ---------------------------------------------------------------------------
__device__ __forceinline__ int lane_id() { return threadIdx.x & 63; }

__device__ __forceinline__ float wave_sum(float v) {
#pragma unroll
  for (int o = 32; o > 0; o >>= 1) v += __shfl_xor(v, o, 64);
  return v;
}

// sum over lanes whose ids differ only in bits >= log2(L) (same "sub" lane of every group)
template <int L>
__device__ __forceinline__ float cross_group_sum(float v) {
#pragma unroll
  for (int o = L; o < 64; o <<= 1) v += __shfl_xor(v, o, 64);
  return v;
}
// sum over the L lanes of one group
template <int L>
__device__ __forceinline__ float in_group_sum(float v) {
#pragma unroll
  for (int o = L >> 1; o > 0; o >>= 1) v += __shfl_xor(v, o, 64);
  return v;
}

__device__ __forceinline__ float4 ld4(const float* p) { return *reinterpret_cast<const float4*>(p); }
__device__ __forceinline__ void st4(float* p, float4 v) { *reinterpret_cast<float4*>(p) = v; }
// streaming variants (nt): model rows are touched once per step; keeping them out of the L2's
// way leaves the batch-sized arrays (XV, slopes, occurrence lists) resident there
typedef float nt_float4 __attribute__((ext_vector_type(4)));
__device__ __forceinline__ float4 ld4_nt(const float* p) {
  nt_float4 v = __builtin_nontemporal_load(reinterpret_cast<const nt_float4*>(p));
  return make_float4(v.x, v.y, v.z, v.w);
}
__device__ __forceinline__ void st4_nt(float* p, float4 v) {
  nt_float4 t = {v.x, v.y, v.z, v.w};
  __builtin_nontemporal_store(t, reinterpret_cast<nt_float4*>(p));
}

// acc + a * b the way SpMV does it (src/common/spmv.h:125, :155): an operand `a` that is exactly zero is SKIPPED, not
// multiplied.  Neutral for finite b; for b = Inf / NaN (a non-finite feature value) it is the difference between the
// reference's result and NaN: a zero weight (pulled as 0: no entry yet, or clipped by l1) and a slope that underflowed to 0
// do not see the value at all.  V rows: a key WITHOUT V is skipped by SpMM (V_pos = -1, spmm.h:108) and is an all-zero row
// here, loaded speculatively; the forward multiplies it by x = 0 instead of the value, decided by the key's has-V flag
// (kHasV in its row word, the header flag of packed rows) — an ALLOCATED row is used whatever it holds, as in the reference
// (round 6: the test of the loaded slice for all-zero that stood in for the flag through round 5 is gone, and with it the
// one documented deviation).
__device__ __forceinline__ float fma_skip0(float a, float b, float acc) { return a != 0.f ? __builtin_fmaf(a, b, acc) : acc; }

__device__ __forceinline__ double wave_sum_d(double v) {
#pragma unroll
  for (int o = 32; o > 0; o >>= 1) v += __shfl_xor(v, o, 64);
  return v;
}

}  // namespace dfh
#endif  // DFH_DEVICE_H_
