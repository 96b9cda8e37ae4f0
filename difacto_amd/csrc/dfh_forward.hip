// dfh_forward.hip — the forward pass over a minibatch and the progress block it opens: k_forward leaves predictions,
// slopes and XV rows and adds the logloss to the block's slots; the penalty goes to the slots beside them, from k_penalty
// (a validation step, here) or from the launch that updates (flush_penalty: k_backward_all, dfh_backward.hip).  KeyRange is
// the restriction of such a launch to the keys a rank owns.  Launched by dfh_step.hip; dfh_riders.hip builds the rider form
// from forward_body, dfh_update.hip takes the slots and KeyRange.
#ifndef DFH_FORWARD_HIP_
#define DFH_FORWARD_HIP_
#include "dfh_device.h"

namespace dfh {

#ifndef DFH_FWD_WAVES
#define DFH_FWD_WAVES 5
#endif

// ---------------------------------------------------------------------------
// k_forward<L>: FMLoss::Predict (src/loss/fm_loss.h:67-119) fused with the
// gather (Store::Pull, sgd_updater.cc:32-56), the logistic slope
// (fm_loss.h:157-161) and Loss::Evaluate (include/difacto/loss.h:57-66).
//
// One wavefront per example.  A V row is read by L = kp/4 lanes as one float4
// each (16 B/lane: k=64 -> 16 lanes x 16 B = two full 128 B lines), so a wave
// has G = 64/L rows in flight per load instruction.  The wave first stages up
// to 64 nnz of the example (one coalesced index load, one gather of
// {row, w, has_V}), then the groups walk the staged nnz with cross-lane
// broadcasts, issuing FWD_DEPTH independent row loads before consuming any
// (the kernel is latency-bound on the random gather: depth, not width, is
// what fills the memory pipe).
//
//   pred_i = sum_j x_ij w_j + 1/2 sum_d [ (sum_j x_ij V_jd)^2 - sum_j x_ij^2 V_jd^2 ]
// ---------------------------------------------------------------------------
// progress partials: prog[kind * PROG_SLOTS + blockIdx.x], summed on the host
constexpr int PROG_SLOTS = 16384;
constexpr int PROG_LOSS = 0, PROG_PENALTY = 1, PROG_AUC = 2;  // [PROG_AUC * PROG_SLOTS] is a single accumulator

// MIXED (sharded store): a key's V row lives either in this rank's table (the keys this rank owns) or in
// the buffer of rows pulled from the other owners; bit 31 of the row word k_lookup / k_uw_remote leave
// in uw[] says which, and the address is chosen per row.
struct MixSrc {
  const float* vbase2;   // V of the pulled rows (packed layout)
  size_t vstride2;
};

// block `bid` of `nblk` 256-thread blocks (the whole launch of k_forward; a block range of a launch that also carries
// riders: dfh_riders.hip)
template <int L, int FWD_DEPTH, bool MIXED>
__device__ __forceinline__ void forward_body(const BatchView& b, const RowSrc& src, const int k, const int kp, const MixSrc& mix,
                                             const uint32_t bid, const uint32_t nblk, double* blk /* [4] shared */) {
  constexpr int G = 64 / L;
  const int lane = lane_id();
  const int grp = lane / L;
  const int sub = lane % L;
  const bool sub_ok = sub * 4 < kp;  // L may exceed kp/4 when kp/4 is not a power of two
  const int wave = (bid * 256u + threadIdx.x) >> 6;
  const int nwaves = (nblk * 256u) >> 6;
  double loss_acc = 0.0;

  for (uint32_t i = wave; i < b.nrows; i += nwaves) {
    const uint32_t beg = b.offset[i], end = b.offset[i + 1];
    float4 xv = make_float4(0.f, 0.f, 0.f, 0.f);
    float4 xxvv = make_float4(0.f, 0.f, 0.f, 0.f);
    float wsum = 0.f;
    for (uint32_t base = beg; base < end; base += 64) {
      const uint32_t j = base + lane;
      const bool valid = j < end;
      uint32_t r = 0;
      float x = 0.f;
      uint32_t hv = 0;
      if (valid) {
        x = b.value ? b.value[j] : 1.0f;
        if (b.uw) {
          // {row, w} of the key from the batch-local table k_lookup left in L2: no header access;
          // a row without V holds zeros, so its flag is not needed either
          const uint2 e = b.uw[b.index[j]];
          r = e.x & (kRowMask | kRemoteRow);
          hv = e.x & kHasV;   // SpMM::Times skips a key without V (spmm.h:108); an allocated row is used whatever it holds
          wsum = fma_skip0(__uint_as_float(e.y), x, wsum);  // spmv.h:125
        } else {
          const uint32_t u = b.index[j];
          r = src.urow ? src.urow[u] : u;
          const float* wp = src.wbase + (size_t)r * src.wstride;
          // {w, has_V} are adjacent: one 8 B load
          float2 wf = *reinterpret_cast<const float2*>(wp);
          hv = __float_as_uint(wf.y);
          wsum = fma_skip0(wf.x, x, wsum);  // spmv.h:125
        }
      }
      const int cnt = min(64u, end - base);
      if (k > 0) {
        for (int t0 = 0; t0 < cnt; t0 += FWD_DEPTH * G) {
          float4 v[FWD_DEPTH];
          float xs[FWD_DEPTH];
#pragma unroll
          for (int q = 0; q < FWD_DEPTH; ++q) {
            const int t = t0 + q * G + grp;
            const uint32_t rr = __shfl(r, t & 63, 64);
            const float xx = __shfl(x, t & 63, 64);
            const uint32_t hh = __shfl(hv, t & 63, 64);
            // the row load does not wait for has_V: a row without V holds zeros
            const bool ok = t < cnt && sub_ok;
            xs[q] = (ok && hh != 0) ? xx : 0.f;
            if (MIXED) {
              const bool rem = (rr & kRemoteRow) != 0u;
              const float* vb = rem ? mix.vbase2 : src.vbase;
              const size_t vs = rem ? mix.vstride2 : src.vstride;
              v[q] = ok ? ld4(vb + (size_t)(rr & ~kRemoteRow) * vs + sub * 4) : make_float4(0.f, 0.f, 0.f, 0.f);
            } else {
              v[q] = ok ? ld4(src.vbase + (size_t)rr * src.vstride + sub * 4) : make_float4(0.f, 0.f, 0.f, 0.f);
            }
          }
#pragma unroll
          for (int q = 0; q < FWD_DEPTH; ++q) {
            // a key WITHOUT V is skipped by SpMM (V_pos = -1, spmm.h:108): its x is 0 here (xs[q], from the key's has-V flag),
            // so that an Inf / NaN feature value on such a key meets the speculatively loaded row of zeros as 0 * 0, not as NaN
            const float xx = xs[q];
            xv.x += v[q].x * xx; xv.y += v[q].y * xx; xv.z += v[q].z * xx; xv.w += v[q].w * xx;
            const float x2 = xx * xx;
            xxvv.x += (v[q].x * v[q].x) * x2; xxvv.y += (v[q].y * v[q].y) * x2;
            xxvv.z += (v[q].z * v[q].z) * x2; xxvv.w += (v[q].w * v[q].w) * x2;
          }
        }
      }
    }
    wsum = wave_sum(wsum);
    float pred = wsum;
    if (k > 0) {
      // combine the G groups' partial rows: every group now holds the full XV / XXVV slice
      xv.x = cross_group_sum<L>(xv.x); xv.y = cross_group_sum<L>(xv.y);
      xv.z = cross_group_sum<L>(xv.z); xv.w = cross_group_sum<L>(xv.w);
      xxvv.x = cross_group_sum<L>(xxvv.x); xxvv.y = cross_group_sum<L>(xxvv.y);
      xxvv.z = cross_group_sum<L>(xxvv.z); xxvv.w = cross_group_sum<L>(xxvv.w);
      // s = sum_d (XV_d^2 - XXVV_d), per-dimension difference first as fm_loss.h:113
      float s = (xv.x * xv.x - xxvv.x) + (xv.y * xv.y - xxvv.y) + (xv.z * xv.z - xxvv.z) + (xv.w * xv.w - xxvv.w);
      s = in_group_sum<L>(s);
      pred += 0.5f * s;
      pred = pred > 20.f ? 20.f : (pred < -20.f ? -20.f : pred);  // fm_loss.h:118 (only when V_dim > 0, :77)
      if (grp == 0 && sub_ok && b.xv) st4(b.xv + (size_t)i * kp + sub * 4, xv);
    }
    if (lane == 0) {
      const float y = b.label[i] > 0 ? 1.0f : -1.0f;
      b.pred[i] = pred;
      b.slope[i] = -y / (1.0f + expf(y * pred));            // fm_loss.h:160
      // log(1 + exp(-y pred)) (loss.h:63) in its stable fp32 form; the batch sum is kept in double
      const float m = -y * pred;
      loss_acc += (double)(fmaxf(m, 0.f) + log1pf(expf(-fabsf(m))));
    }
  }
  // the batch's logloss: one private slot per block (same-address atomics
  // serialise at ~12 ns each on this chip: 2k blocks would cost 25 us)
  if (lane == 0) blk[threadIdx.x >> 6] = loss_acc;
  __syncthreads();
  if (threadIdx.x == 0) atomicAdd(&b.prog[PROG_LOSS * PROG_SLOTS + (bid % PROG_SLOTS)], blk[0] + blk[1] + blk[2] + blk[3]);
}

template <int L, int FWD_DEPTH, bool MIXED>
__global__ void __launch_bounds__(256, DFH_FWD_WAVES) k_forward(BatchView b, RowSrc src, int k, int kp, MixSrc mix) {
  __shared__ double blk[4];
  forward_body<L, FWD_DEPTH, MIXED>(b, src, k, kp, mix, blockIdx.x, gridDim.x, blk);
}

// a launch of k_backward_all / k_penalty may be restricted to the keys whose rank u lies inside
// (inv = 0) or outside (inv = 1) [lo, hi): the sharded store runs the keys this rank owns through the
// fused in-place update and the others through the gradient-row form.  Default: every key.
struct KeyRange {
  uint32_t lo, hi, inv;  // inv bit 0: the keys OUTSIDE [lo, hi); bit 1: the gradient-row form also adds up the penalty of the
                         // rows it reads (EvaluatePenalty over the weights pulled from other owners, sgd_learner.cc:249-273)
};
__device__ __forceinline__ bool key_in(const KeyRange& kr, uint32_t u) { return ((u - kr.lo < kr.hi - kr.lo) ? 1u : 0u) != (kr.inv & 1u); }
__device__ __forceinline__ bool key_pen(const KeyRange& kr) { return (kr.inv & 2u) != 0; }

// block-wide sum of the per-lane penalty partials into one of PROG_SLOTS slots
// (distinct addresses: no same-address atomic serialisation)
__device__ __forceinline__ void flush_penalty(const BatchView& b, double pen_acc) {
  __shared__ double pen_blk[16];
  pen_acc = wave_sum_d(pen_acc);
  if (lane_id() == 0) pen_blk[threadIdx.x >> 6] = pen_acc;
  __syncthreads();
  if (threadIdx.x == 0) {
    double t = 0.0;
    for (int i = 0; i < (int)(blockDim.x >> 6); ++i) t += pen_blk[i];
    if (t != 0.0) atomicAdd(&b.prog[PROG_PENALTY * PROG_SLOTS + (blockIdx.x % PROG_SLOTS)], t);
  }
}

// penalty only (validation batches: no backward pass)
template <int L>
__global__ void __launch_bounds__(256) k_penalty(BatchView b, RowSrc src, TableView t, int k, int kp, KeyRange rg) {
  const int lane = lane_id();
  const int wave = (blockIdx.x * blockDim.x + threadIdx.x) >> 6;
  const int nwaves = (gridDim.x * blockDim.x) >> 6;
  const uint32_t U = *b.d_U;
  double pen_acc = 0.0;
  for (uint32_t u = wave; u < U; u += nwaves) {
    if (!key_in(rg, u)) continue;
    const uint32_t r = src.urow ? src.urow[u] : u;
    const float2 wf = *reinterpret_cast<const float2*>(src.wbase + (size_t)r * src.wstride);
    float pen = 0.f;
    if (k > 0 && __float_as_uint(wf.y) != 0) {
      for (int d = lane; d < k; d += 64) {
        float vv = src.vbase[(size_t)r * src.vstride + d];
        pen += 0.5f * t.p.V_l2 * vv * vv;
      }
    }
    pen = wave_sum(pen);
    if (lane == 0) pen_acc += (double)pen + (double)t.p.l1 * fabs((double)wf.x) + 0.5 * (double)t.p.l2 * (double)wf.x * (double)wf.x;
  }
  flush_penalty(b, lane == 0 ? pen_acc : 0.0);
}

}  // namespace dfh
#endif  // DFH_FORWARD_HIP_
