// dfh_backward.hip — k_backward_all, the backward pass of a minibatch in one launch with its three roles (the banner below
// has the design), and k_seg_lists, which lists the keys with long segments for them.  The form of the update that serves
// packed rows (gradient rows out: dfh_batch_backward, the sharded store's keys of other ranks) and the table with
// ctx option upd_kernel = 0; k_update_fused (dfh_update.hip) is the default on the table and shares the BWD_* thresholds, as
// does the Localizer's emit (dfh_localize.hip), which fills the same lists.  Launched by dfh_step.hip, dfh_batch.hip and
// dfh_localize_api.hip.
#ifndef DFH_BACKWARD_HIP_
#define DFH_BACKWARD_HIP_
#include "dfh_updater.h"     // ftrl_update_w, adagrad_update_v, init_v_hash_row
#include "dfh_forward.hip"   // PROG_*, KeyRange, flush_penalty

namespace dfh {

#ifndef DFH_BWD_SMALL
#define DFH_BWD_SMALL 8
#endif
#ifndef DFH_BWD_MID
#define DFH_BWD_MID 64
#endif
#ifndef DFH_BWD_DEPTH
#define DFH_BWD_DEPTH 2
#endif
#ifndef DFH_BWD_SMALL_DEPTH
#define DFH_BWD_SMALL_DEPTH 2
#endif
#ifndef DFH_BWD_INTERLEAVE
#define DFH_BWD_INTERLEAVE 0
#endif
constexpr uint32_t BWD_SMALL = DFH_BWD_SMALL;
constexpr uint32_t BWD_MID = DFH_BWD_MID;
constexpr int BWD_DEPTH = DFH_BWD_DEPTH;
constexpr int BWD_SMALL_DEPTH = DFH_BWD_SMALL_DEPTH;
#ifndef DFH_BWD_THREADS
#define DFH_BWD_THREADS 512
#endif
constexpr int BWD_THREADS = DFH_BWD_THREADS;    // threads per block of k_backward_all
#ifdef DFH_BWD_TRACE
__device__ unsigned long long g_bwd_trace[3 * 8192];
#endif

// ---------------------------------------------------------------------------
// Backward / update: FMLoss::CalcGrad (src/loss/fm_loss.h:148-199) as a
// segmented sum over the key-ordered occurrence list the Localizer's sort
// leaves behind (runs of equal key, src/data/localizer.cc:28):
//   gw_u   = sum_occ x p_i
//   gV_u,d = sum_occ x (p_i XV_i,d) - V_u,d sum_occ x^2 p_i
// FUSED: apply SGDUpdater::Update for the key in place (FTRL on w, AdaGrad on
// V, lazy InitV) — no gradient ever reaches HBM.
// !FUSED: write [gw, has_V, 0, 0 | gV] rows of `gstride` floats (exchange layout).
//
// Segment lengths are Zipf-distributed (1 .. ~B/8), so ONE launch (k_backward_all)
// runs three roles, chosen by block range (long chains first so they start early):
//   hot    one key of the hot list (cnt > BWD_MID) per block and iteration: the
//          block's waves split the segment, partials combined in LDS in wave order
//   mid    one key of the mid list (BWD_SMALL < cnt <= BWD_MID) per wave
//   short  one L-lane group per key (G keys per wave), occurrences summed serially
//          in row order — the reference's own order
// The two lists are compacted once per minibatch by k_seg_lists.  Every key is
// handled by exactly one role; nothing is communicated between blocks.  Each role
// issues all of a key's independent loads (header, V row, AdaGrad row, occurrence
// list) before consuming any; V rows are read speculatively (a row without V holds
// zeros, in the table and in packed rows alike).
// ---------------------------------------------------------------------------

struct KeySums {
  float gw;    // sum p x
  float xxp;   // sum p x^2
  float4 gv;   // sum (XV p) x, this lane's 4 dims
};

struct KeyRow {   // what a role prefetches for one key
  uint32_t r;
  float w_old;
  bool has_v;
  float sqrt_g, z, fea_cnt;
  float4 v, acc;  // this lane's slices
};

template <bool FUSED>
__device__ __forceinline__ KeyRow load_key_row(const RowSrc& src, const TableView& t, uint32_t u, int sub, bool sub_ok,
                                               int k, int kp, bool resolved = true) {
  KeyRow kr;
  // resolved = false: the key is outside the launch's range and may have no row id (speculative load: row 0)
  kr.r = src.urow ? (resolved ? src.urow[u] : 0u) : u;
  const float* wp = src.wbase + (size_t)kr.r * src.wstride;
  kr.v = make_float4(0.f, 0.f, 0.f, 0.f);
  kr.acc = kr.v;
  kr.sqrt_g = kr.z = kr.fea_cnt = 0.f;
  // independent loads, issued back to back
  float4 h0 = ld4(wp);  // table: {w, has_V, sqrt_g, z}; packed: {w, has_V, 0, 0}
  if (k > 0 && sub_ok) {
    kr.v = FUSED ? ld4_nt(src.vbase + (size_t)kr.r * src.vstride + sub * 4) : ld4(src.vbase + (size_t)kr.r * src.vstride + sub * 4);
    if (FUSED) kr.acc = ld4_nt(t.va + (size_t)kr.r * (2 * kp) + kp + sub * 4);
  }
  if (FUSED) kr.fea_cnt = t.hdr[kr.r].fea_cnt;
  kr.w_old = h0.x;
  kr.has_v = k > 0 && __float_as_uint(h0.y) != 0;
  kr.sqrt_g = h0.z;
  kr.z = h0.w;
  if (!kr.has_v) kr.v = make_float4(0.f, 0.f, 0.f, 0.f);
  return kr;
}

// Everything after the sums, executed by the L lanes of ONE group (the caller
// masks the others).
template <int L, bool FUSED>
__device__ __forceinline__ void finish_key(const BatchView& b, const TableView& t, uint32_t u, const KeyRow& kr, int sub,
                                           bool sub_ok, KeySums s, float* __restrict__ grads, size_t gstride, int k,
                                           int kp, uint32_t* __restrict__ need_init, double& pen_acc, bool pen_rows = false) {
  float4 gv = s.gv;
  const float4 v = kr.v;
  if (kr.has_v) {
    // grad_V = X'(diag(p) XV) - diag(XXp) V   (fm_loss.h:181-198)
    gv.x -= v.x * s.xxp; gv.y -= v.y * s.xxp; gv.z -= v.z * s.xxp; gv.w -= v.w * s.xxp;
  }
  if (!FUSED) {
    float* g = grads + (size_t)u * gstride;
    if (sub == 0) st4(g, make_float4(s.gw, kr.has_v ? 1.0f : 0.0f, 0.f, 0.f));
    if (sub_ok && k > 0) st4(g + 4 + sub * 4, kr.has_v ? gv : make_float4(0.f, 0.f, 0.f, 0.f));
    if (pen_rows) {  // the rows came from another owner: their penalty is nobody else's to count
      if (kr.has_v && sub_ok) pen_acc += (double)(0.5f * t.p.V_l2 * (v.x * v.x + v.y * v.y + v.z * v.z + v.w * v.w));
      if (sub == 0) pen_acc += (double)(t.p.l1 * fabsf(kr.w_old) + 0.5f * t.p.l2 * kr.w_old * kr.w_old);
    }
    return;
  }
  // penalty of the PULLED weights (SGDLearner::EvaluatePenalty, sgd_learner.cc:249-273)
  // per-lane partials in fp32 (a handful of terms each), widened when the block flushes
  if (kr.has_v && sub_ok) pen_acc += (double)(0.5f * t.p.V_l2 * (v.x * v.x + v.y * v.y + v.z * v.z + v.w * v.w));
  RowHdr* hp = t.hdr + kr.r;
  if (sub == 0) {
    const float w_old = kr.w_old;
    pen_acc += (double)(t.p.l1 * fabsf(w_old) + 0.5f * t.p.l2 * w_old * w_old);
    // SGDUpdater::Update(kGradient) for this key (sgd_updater.cc:86-95)
    float sqrt_g = kr.sqrt_g, z = kr.z;
    const float w_new = ftrl_update_w(s.gw, w_old, sqrt_g, z, t.p);
    // one 16 B store of {w, has_V, sqrt_g, z}
    uint32_t hv = kr.has_v ? 1u : 0u;
    // lazy InitV when w leaves zero (sgd_updater.cc:122-126)
    if (w_old == 0 && w_new != 0 && k > 0 && !kr.has_v && kr.fea_cnt > (float)t.p.V_threshold) {
      if (t.p.init_mode == DFH_INIT_HASH) {
        init_v_hash_row(t, kr.r, b.feaids[u]);
        hv = 1u;
      } else {
        need_init[u] = 1;
      }
    }
    st4(reinterpret_cast<float*>(hp), make_float4(w_new, __uint_as_float(hv), sqrt_g, z));
  }
  if (kr.has_v && sub_ok) {
    float* va = t.va + (size_t)kr.r * (2 * kp);
    float4 acc = kr.acc;
    float4 nv = v;
    adagrad_update_v(gv.x, nv.x, acc.x, t.p);
    adagrad_update_v(gv.y, nv.y, acc.y, t.p);
    adagrad_update_v(gv.z, nv.z, acc.z, t.p);
    adagrad_update_v(gv.w, nv.w, acc.w, t.p);
    // padded coordinates (>= k) stay exactly zero
    const int d0 = sub * 4;
    if (d0 + 0 >= k) { nv.x = 0.f; acc.x = 0.f; }
    if (d0 + 1 >= k) { nv.y = 0.f; acc.y = 0.f; }
    if (d0 + 2 >= k) { nv.z = 0.f; acc.z = 0.f; }
    if (d0 + 3 >= k) { nv.w = 0.f; acc.w = 0.f; }
    st4_nt(va + sub * 4, nv);
    st4_nt(va + kp + sub * 4, acc);
  }
}

// partial sums of occurrences [beg,end) taken by this wave: tiles of 64
// starting at tile w0, stride wstep tiles; result: gw/xxp wave-reduced, gv
// reduced across groups (every group holds the sums of its lane slice)
template <int L>
__device__ __forceinline__ KeySums wave_segment_sums(const BatchView& b, uint32_t beg, uint32_t end, uint32_t w0,
                                                     uint32_t wstep, bool want_v, bool sub_ok, int grp, int sub, int kp) {
  constexpr int G = 64 / L;
  const int lane = lane_id();
  KeySums s;
  s.gw = 0.f; s.xxp = 0.f; s.gv = make_float4(0.f, 0.f, 0.f, 0.f);
  for (uint32_t base = beg + w0 * 64; base < end; base += wstep * 64) {
    const uint32_t j = base + lane;
    const bool valid = j < end;
    uint32_t row = 0;
    float x = 0.f, p = 0.f;
    if (valid) {
      row = b.s_row[j];
      x = b.s_val ? b.s_val[j] : 1.0f;
      p = b.slope[row];
      s.gw = fma_skip0(p, x, s.gw);          // spmv.h:155-163
      s.xxp = fma_skip0(p, x * x, s.xxp);    // fm_loss.h:171-178 with XX = value^2
    }
    if (want_v) {
      const int cnt = min(64u, end - base);
      for (int t0 = 0; t0 < cnt; t0 += BWD_DEPTH * G) {
        float4 a[BWD_DEPTH];
        float xs[BWD_DEPTH], ps[BWD_DEPTH];
#pragma unroll
        for (int q = 0; q < BWD_DEPTH; ++q) {
          const int tt = t0 + q * G + grp;
          const uint32_t rowi = __shfl(row, tt & 63, 64);
          const float xx = __shfl(x, tt & 63, 64);
          const float pp = __shfl(p, tt & 63, 64);
          const bool ok = tt < cnt && sub_ok;
          xs[q] = ok ? xx : 0.f;
          ps[q] = pp;
          a[q] = ok ? ld4(b.xv + (size_t)rowi * kp + sub * 4) : make_float4(0.f, 0.f, 0.f, 0.f);
        }
#pragma unroll
        for (int q = 0; q < BWD_DEPTH; ++q) {
          const float pp = ps[q], xx = xs[q];
          s.gv.x += (a[q].x * pp) * xx; s.gv.y += (a[q].y * pp) * xx;
          s.gv.z += (a[q].z * pp) * xx; s.gv.w += (a[q].w * pp) * xx;
        }
      }
    }
  }
  s.gw = wave_sum(s.gw);
  s.xxp = wave_sum(s.xxp);
  if (want_v) {
    s.gv.x = cross_group_sum<L>(s.gv.x); s.gv.y = cross_group_sum<L>(s.gv.y);
    s.gv.z = cross_group_sum<L>(s.gv.z); s.gv.w = cross_group_sum<L>(s.gv.w);
  }
  return s;
}

// ---- long segments (cnt > BWD_SMALL), taken from the two lists k_seg_lists compacts once per
// minibatch: every wave of the mid blocks takes mid keys (whole wave per key), every hot block
// takes hot keys one at a time (its NW waves split the segment, partials combined through LDS in
// wave order).  The lists are in arbitrary order; a key's result does not depend on it.
template <int L, bool FUSED, int NW>
__device__ __forceinline__ void mid_role(const BatchView& b, const RowSrc& src, const TableView& t, float* __restrict__ grads,
                                         size_t gstride, int k, int kp, uint32_t* __restrict__ need_init, uint32_t wave,
                                         uint32_t nwaves, uint32_t nb, const KeyRange& rg, double& pen_acc) {
  const int lane = lane_id();
  const int grp = lane / L;
  const int sub = lane % L;
  const bool sub_ok = sub * 4 < kp;
  // waves are dealt to the list buckets: G waves per bucket when there are more waves than buckets
  if (nb == 0) return;
  const uint32_t G = max(1u, nwaves / nb), ngroups = nwaves / G;
  const uint32_t grp_w = wave / G, sub_w = wave % G;
  if (grp_w >= ngroups) return;
  for (uint32_t lb = grp_w; lb < nb; lb += ngroups) {
    const uint2 co = b.seg.mid[lb];
    const uint32_t nm = co.x;
    if (nm == 0) continue;
    const SegEnt* __restrict__ ent = b.seg.mid_ent + co.y;
    for (uint32_t q = sub_w; q < nm; q += G) {
      const SegEnt e = ent[q];
      const uint32_t u = e.x;
      if (!key_in(rg, u)) continue;  // uniform per wave
      const uint32_t beg = e.y, end = e.z;
      KeySums s = wave_segment_sums<L>(b, beg, end, 0, 1, k > 0, sub_ok, grp, sub, kp);
      // the key's row is fetched after the sums: one more round trip for a segment of 9+ occurrences,
      // 14 registers fewer alive through the loop (the kernel runs at 64 registers, 8 waves per SIMD)
      if (grp == 0) {
        const KeyRow kr = load_key_row<FUSED>(src, t, u, sub, sub_ok, k, kp);
        finish_key<L, FUSED>(b, t, u, kr, sub, sub_ok, s, grads, gstride, k, kp, need_init, pen_acc, key_pen(rg));
      }
    }
  }
}

template <int L, bool FUSED, int NW>
__device__ __forceinline__ void hot_role(const BatchView& b, const RowSrc& src, const TableView& t, float* __restrict__ grads,
                                         size_t gstride, int k, int kp, uint32_t* __restrict__ need_init, uint32_t blk,
                                         uint32_t nblk, uint32_t nb, const KeyRange& rg, double& pen_acc) {
  __shared__ float part[NW][2 + 256];  // per wave: gw, xxp, gv[kp <= 256]
  const int lane = lane_id();
  const int grp = lane / L;
  const int sub = lane % L;
  const bool sub_ok = sub * 4 < kp;
  const int w = threadIdx.x >> 6;
  // blocks are dealt to the list buckets like the waves of the mid role (uniform per block: the
  // barriers below are reached by all of its threads)
  if (nb == 0) return;
  const uint32_t G = max(1u, nblk / nb), ngroups = nblk / G;
  const uint32_t grp_b = blk / G, sub_b = blk % G;
  if (grp_b >= ngroups) return;
  for (uint32_t lb = grp_b; lb < nb; lb += ngroups) {
  const uint2 co = b.seg.hot[lb];
  const uint32_t nh = co.x;
  if (nh == 0) continue;
  const SegEnt* __restrict__ ent = b.seg.hot_ent + co.y;
  for (uint32_t q = sub_b; q < nh; q += G) {
    const SegEnt e = ent[q];
    const uint32_t u = e.x;
    if (!key_in(rg, u)) continue;  // uniform per block
    const uint32_t beg = e.y, end = e.z;
    KeySums s = wave_segment_sums<L>(b, beg, end, (uint32_t)w, NW, k > 0, sub_ok, grp, sub, kp);
    __syncthreads();  // previous key's partials consumed
    if (grp == 0) {
      if (sub == 0) { part[w][0] = s.gw; part[w][1] = s.xxp; }
      if (sub_ok) {
        part[w][2 + sub * 4 + 0] = s.gv.x; part[w][2 + sub * 4 + 1] = s.gv.y;
        part[w][2 + sub * 4 + 2] = s.gv.z; part[w][2 + sub * 4 + 3] = s.gv.w;
      }
    }
    __syncthreads();
    if (w == 0 && grp == 0) {
      KeySums tot;
      tot.gw = 0.f; tot.xxp = 0.f; tot.gv = make_float4(0.f, 0.f, 0.f, 0.f);
#pragma unroll
      for (int i = 0; i < NW; ++i) {
        tot.gw += part[i][0];
        tot.xxp += part[i][1];
        if (sub_ok) {
          tot.gv.x += part[i][2 + sub * 4 + 0]; tot.gv.y += part[i][2 + sub * 4 + 1];
          tot.gv.z += part[i][2 + sub * 4 + 2]; tot.gv.w += part[i][2 + sub * 4 + 3];
        }
      }
      const KeyRow kr = load_key_row<FUSED>(src, t, u, sub, sub_ok, k, kp);  // after the sums, as in the mid role
      finish_key<L, FUSED>(b, t, u, kr, sub, sub_ok, tot, grads, gstride, k, kp, need_init, pen_acc, key_pen(rg));
    }
  }
  }
}

// ---- small segments (cnt <= BWD_SMALL): one L-lane group per key, G keys per wave,
// occurrences summed serially in row order (the reference's own order).  Its own
// launch so that it gets its own register budget (8 waves/SIMD): the kernel is a
// chain of dependent random accesses and only occupancy hides them.  Runs
// concurrently with k_backward_big (other stream): the two touch disjoint keys.
template <int L, bool FUSED>
__device__ __forceinline__ void small_role(const BatchView& b, const RowSrc& src, const TableView& t, float* __restrict__ grads,
                                           size_t gstride, int k, int kp, uint32_t* __restrict__ need_init, uint32_t wave,
                                           uint32_t nwaves, const KeyRange& rg, double& pen_acc) {
  constexpr int G = 64 / L;
  const int lane = lane_id();
  const int grp = lane / L;
  const int sub = lane % L;
  const bool sub_ok = sub * 4 < kp;
  const uint32_t U = *b.d_U;
  {
    for (uint32_t u0 = wave * G; u0 < U; u0 += nwaves * G) {
      // no branch before the loads: the segment bounds, the row id and then the row itself are
      // requested for every lane group (keys left to the mid / hot roles waste one speculative read)
      const uint32_t u = min(u0 + grp, U - 1);
      const uint32_t beg = b.col_ptr[u], end_all = b.col_ptr[u + 1];
      const bool in_rg = key_in(rg, u);
      const KeyRow kr = load_key_row<FUSED>(src, t, u, sub, sub_ok, k, kp, in_rg);
      const bool mine = (u0 + grp) < U && end_all - beg <= BWD_SMALL && in_rg;
      const uint32_t end = mine ? end_all : beg;
      KeySums s;
      s.gw = 0.f; s.xxp = 0.f; s.gv = make_float4(0.f, 0.f, 0.f, 0.f);
      for (uint32_t j0 = beg; j0 < end; j0 += BWD_SMALL_DEPTH) {
        float4 a[BWD_SMALL_DEPTH];
        float xs[BWD_SMALL_DEPTH], ps[BWD_SMALL_DEPTH];
#pragma unroll
        for (int q = 0; q < BWD_SMALL_DEPTH; ++q) {
          const uint32_t j = j0 + q;
          const bool ok = j < end;
          const uint32_t row = ok ? b.s_row[j] : 0;
          xs[q] = ok ? (b.s_val ? b.s_val[j] : 1.0f) : 0.f;
          ps[q] = ok ? b.slope[row] : 0.f;
          a[q] = (ok && k > 0 && sub_ok) ? ld4(b.xv + (size_t)row * kp + sub * 4) : make_float4(0.f, 0.f, 0.f, 0.f);
        }
#pragma unroll
        for (int q = 0; q < BWD_SMALL_DEPTH; ++q) {  // ascending rows: the reference's order (spmm.h:137-156)
          const float pp = ps[q], xx = xs[q];
          s.gw = fma_skip0(pp, xx, s.gw);
          s.xxp = fma_skip0(pp, xx * xx, s.xxp);
          s.gv.x += (a[q].x * pp) * xx; s.gv.y += (a[q].y * pp) * xx;
          s.gv.z += (a[q].z * pp) * xx; s.gv.w += (a[q].w * pp) * xx;
        }
      }
      if (mine) finish_key<L, FUSED>(b, t, u, kr, sub, sub_ok, s, grads, gstride, k, kp, need_init, pen_acc, key_pen(rg));
    }
  }
}

// ---------------------------------------------------------------------------
// k_update_small<L>: the table-resident, fused form of the short-segment role
// (cnt <= BWD_SMALL, ~95 % of the keys of a Zipf batch), written lean on the
// pattern tools/rmw_bench.hip measures at ~40 us for a whole batch: a compact
// argument block (few SGPRs), compile-time row strides when kp == 4L, one level
// of index loads (segment bounds + row id), then every independent load of the
// key at once (header, V, accumulators, first occurrences).
// ---------------------------------------------------------------------------
struct SmallArgs {
  const uint32_t* d_U;
  const uint32_t* col_ptr;
  const uint32_t* urow;
  const uint32_t* s_row;
  const float* s_val;
  const float* slope;
  const float* xv;
  const uint64_t* feaids;
  RowHdr* hdr;
  float* va;
  uint32_t* need_init;
  double* prog;
  int k, kp;
  dfh_updater_param p;
};

#ifndef DFH_BWD_SMALL_KEYS
#define DFH_BWD_SMALL_KEYS 1
#endif
// KPG keys per lane group and iteration, all of their loads in flight together: the role is a chain
// of dependent round trips (segment bounds + row id -> model row + occurrence list -> slopes + XV
// rows), and with the register file capping the waves per SIMD, more independent chains per wave
// are the only way to more requests in flight.
template <int L, bool EXACT>
__device__ __forceinline__ void small_role_lean(const SmallArgs& a, uint32_t wave, uint32_t nwaves, const KeyRange& rg, double& pen_acc) {
  constexpr int G = 64 / L;
  constexpr int KPG = DFH_BWD_SMALL_KEYS;
  const int lane = lane_id();
  const int grp = lane / L;
  const int sub = lane % L;
  const int kp = EXACT ? 4 * L : a.kp;
  const int k = a.k;
  const bool sub_ok = EXACT ? true : (sub * 4 < kp);
  const uint32_t U = *a.d_U;
  float pen = 0.f;
  for (uint32_t u0 = wave * (G * KPG); u0 < U; u0 += nwaves * (G * KPG)) {
    uint32_t u[KPG], beg[KPG], end[KPG], r[KPG];
    bool mine[KPG];
#pragma unroll
    for (int h = 0; h < KPG; ++h) {  // round trip 1: segment bounds + row id
      const uint32_t uu = u0 + h * G + grp;
      u[h] = min(uu, U - 1);
      beg[h] = a.col_ptr[u[h]];
      end[h] = a.col_ptr[u[h] + 1];
      // keys outside the launch's range have no row id in urow (the sharded store resolves only the keys
      // this rank owns): their speculative row loads below go to row 0
      r[h] = key_in(rg, u[h]) ? a.urow[u[h]] : 0u;
    }
    float4 h0[KPG], v[KPG], acc[KPG], gv[KPG];
    float fea_cnt[KPG], gw[KPG], xxp[KPG];
    uint32_t rows[KPG][BWD_SMALL_DEPTH];
    float xs[KPG][BWD_SMALL_DEPTH];
#pragma unroll
    for (int h = 0; h < KPG; ++h) {  // round trip 2: the model row and the first occurrences, back to back
      mine[h] = (u0 + h * G + grp) < U && end[h] - beg[h] <= BWD_SMALL && key_in(rg, u[h]);
      if (!mine[h]) end[h] = beg[h];
      const RowHdr* hp = a.hdr + r[h];
      const float* va = a.va + (size_t)r[h] * (2 * kp);
      h0[h] = ld4(reinterpret_cast<const float*>(hp));  // {w, has_V, sqrt_g, z}
      fea_cnt[h] = hp->fea_cnt;
      v[h] = make_float4(0.f, 0.f, 0.f, 0.f);
      acc[h] = v[h];
      if (k > 0 && sub_ok) {
        v[h] = ld4_nt(va + sub * 4);
        acc[h] = ld4_nt(va + kp + sub * 4);
      }
#pragma unroll
      for (int q = 0; q < BWD_SMALL_DEPTH; ++q) {
        const bool ok = beg[h] + q < end[h];
        rows[h][q] = ok ? a.s_row[beg[h] + q] : 0u;
        xs[h][q] = ok ? (a.s_val ? a.s_val[beg[h] + q] : 1.0f) : 0.f;
      }
      gw[h] = 0.f;
      xxp[h] = 0.f;
      gv[h] = make_float4(0.f, 0.f, 0.f, 0.f);
    }
    uint32_t longest = 0;
#pragma unroll
    for (int h = 0; h < KPG; ++h) longest = max(longest, end[h] - beg[h]);
    for (uint32_t j0 = 0; j0 < longest; j0 += BWD_SMALL_DEPTH) {
      float ps[KPG][BWD_SMALL_DEPTH];
      float4 av[KPG][BWD_SMALL_DEPTH];
#pragma unroll
      for (int h = 0; h < KPG; ++h) {  // round trip 3 (+): slopes and XV rows of these occurrences
#pragma unroll
        for (int q = 0; q < BWD_SMALL_DEPTH; ++q) {
          const bool ok = beg[h] + j0 + q < end[h];
          ps[h][q] = ok ? a.slope[rows[h][q]] : 0.f;
          av[h][q] = (ok && k > 0 && sub_ok) ? ld4(a.xv + (size_t)rows[h][q] * kp + sub * 4) : make_float4(0.f, 0.f, 0.f, 0.f);
        }
      }
      const bool more = j0 + BWD_SMALL_DEPTH < longest;
#pragma unroll
      for (int h = 0; h < KPG; ++h) {
#pragma unroll
        for (int q = 0; q < BWD_SMALL_DEPTH; ++q) {  // ascending rows: the reference's order (spmm.h:137-156)
          const float pp = ps[h][q], xx = xs[h][q];
          gw[h] = fma_skip0(pp, xx, gw[h]); xxp[h] = fma_skip0(pp, xx * xx, xxp[h]);
          gv[h].x += (av[h][q].x * pp) * xx; gv[h].y += (av[h][q].y * pp) * xx;
          gv[h].z += (av[h][q].z * pp) * xx; gv[h].w += (av[h][q].w * pp) * xx;
        }
        if (more) {  // the next occurrences of the longer segments
#pragma unroll
          for (int q = 0; q < BWD_SMALL_DEPTH; ++q) {
            const uint32_t j = beg[h] + j0 + BWD_SMALL_DEPTH + q;
            const bool ok = j < end[h];
            rows[h][q] = ok ? a.s_row[j] : 0u;
            xs[h][q] = ok ? (a.s_val ? a.s_val[j] : 1.0f) : 0.f;
          }
        }
      }
    }
#pragma unroll
    for (int h = 0; h < KPG; ++h) {
      if (!mine[h]) continue;
      RowHdr* hp = a.hdr + r[h];
      float* va = a.va + (size_t)r[h] * (2 * kp);
      const float w_old = h0[h].x;
      const bool has_v = k > 0 && __float_as_uint(h0[h].y) != 0;
      float4 g4 = gv[h];
      const float4 vv = v[h];
      if (has_v) {
        // grad_V = X'(diag(p) XV) - diag(XXp) V   (fm_loss.h:181-198); rows without V hold zeros
        g4.x -= vv.x * xxp[h]; g4.y -= vv.y * xxp[h]; g4.z -= vv.z * xxp[h]; g4.w -= vv.w * xxp[h];
        if (sub_ok) pen += 0.5f * a.p.V_l2 * (vv.x * vv.x + vv.y * vv.y + vv.z * vv.z + vv.w * vv.w);
      }
      if (sub == 0) {
        pen += a.p.l1 * fabsf(w_old) + 0.5f * a.p.l2 * w_old * w_old;
        float sqrt_g = h0[h].z, z = h0[h].w;
        const float w_new = ftrl_update_w(gw[h], w_old, sqrt_g, z, a.p);
        uint32_t hv = has_v ? 1u : 0u;
        if (w_old == 0 && w_new != 0 && k > 0 && !has_v && fea_cnt[h] > (float)a.p.V_threshold) {  // sgd_updater.cc:122-126
          if (a.p.init_mode == DFH_INIT_HASH) {
            const uint64_t key = a.feaids[u[h]];
            for (int j = 0; j < kp; ++j) {
              va[j] = j < k ? hash_init_value(key, j, a.p.seed, a.p.V_init_scale) : 0.0f;
              va[kp + j] = 0.0f;
            }
            hv = 1u;
          } else {
            a.need_init[u[h]] = 1;
          }
        }
        st4(reinterpret_cast<float*>(hp), make_float4(w_new, __uint_as_float(hv), sqrt_g, z));
      }
      if (has_v && sub_ok) {
        float4 nv = vv, na = acc[h];
        adagrad_update_v(g4.x, nv.x, na.x, a.p);
        adagrad_update_v(g4.y, nv.y, na.y, a.p);
        adagrad_update_v(g4.z, nv.z, na.z, a.p);
        adagrad_update_v(g4.w, nv.w, na.w, a.p);
        if (!EXACT || k != kp) {
          const int d0 = sub * 4;
          if (d0 + 0 >= k) { nv.x = 0.f; na.x = 0.f; }
          if (d0 + 1 >= k) { nv.y = 0.f; na.y = 0.f; }
          if (d0 + 2 >= k) { nv.z = 0.f; na.z = 0.f; }
          if (d0 + 3 >= k) { nv.w = 0.f; na.w = 0.f; }
        }
        st4_nt(va + sub * 4, nv);
        st4_nt(va + kp + sub * 4, na);
      }
    }
  }
  pen_acc += (double)pen;  // penalty of the pulled weights (sgd_learner.cc:249-273); flushed once per block
}

// ---------------------------------------------------------------------------
// k_backward_all: ONE launch for the whole backward/update of a minibatch.  Blocks
// [0, nb_big) run the long-segment roles (they start first: their chains are the
// longest), the others the short-segment role.  LEAN selects the table-specialised
// short-segment code (fused update on the resident table).
// ---------------------------------------------------------------------------
#ifndef DFH_BWD_WAVES
#define DFH_BWD_WAVES 8
#endif
template <int L, bool FUSED, bool LEAN, bool EXACT>
__global__ void __launch_bounds__(BWD_THREADS, DFH_BWD_WAVES) k_backward_all(BatchView b, RowSrc src, TableView t, float* __restrict__ grads,
                                                                size_t gstride, int k, int kp, uint32_t* __restrict__ need_init,
                                                                uint32_t nb_hot, uint32_t nb_mid, uint32_t nlist, KeyRange rg) {
  constexpr int NW = BWD_THREADS / 64;
  double pen_acc = 0.0;
#ifdef DFH_BWD_TRACE
  const unsigned long long trace_t0 = wall_clock64();
#endif
  // block -> role.  The long-segment blocks come first in dispatch order (their chains are the
  // longest), optionally interleaved 1 : (R - 1) with short-segment blocks so that the first
  // resident set is not long-segment blocks only
  const uint32_t nb_big = nb_hot + nb_mid;
  uint32_t big_id = blockIdx.x, small_id = blockIdx.x - min(blockIdx.x, nb_big);
  bool is_big = blockIdx.x < nb_big;
  if (DFH_BWD_INTERLEAVE > 1) {
    constexpr uint32_t R = DFH_BWD_INTERLEAVE > 1 ? DFH_BWD_INTERLEAVE : 2;
    const uint32_t before = min(nb_big, (blockIdx.x + R - 1) / R);  // long-segment blocks with a smaller id
    is_big = blockIdx.x % R == 0 && blockIdx.x / R < nb_big;
    big_id = blockIdx.x / R;
    small_id = blockIdx.x - before;
  }
  if (is_big && big_id < nb_hot) {
    hot_role<L, FUSED, NW>(b, src, t, grads, gstride, k, kp, need_init, big_id, nb_hot, nlist, rg, pen_acc);
  } else if (is_big) {
    mid_role<L, FUSED, NW>(b, src, t, grads, gstride, k, kp, need_init, (big_id - nb_hot) * NW + (threadIdx.x >> 6),
                           nb_mid * NW, nlist, rg, pen_acc);
  } else {
    const uint32_t wave = small_id * NW + (threadIdx.x >> 6);
    const uint32_t nwaves = (gridDim.x - nb_big) * NW;
    if (LEAN) {
      SmallArgs sa;
      sa.d_U = b.d_U; sa.col_ptr = b.col_ptr; sa.urow = src.urow; sa.s_row = b.s_row; sa.s_val = b.s_val;
      sa.slope = b.slope; sa.xv = b.xv; sa.feaids = b.feaids; sa.hdr = t.hdr; sa.va = t.va; sa.need_init = need_init;
      sa.prog = b.prog; sa.k = k; sa.kp = kp; sa.p = t.p;
      small_role_lean<L, EXACT>(sa, wave, nwaves, rg, pen_acc);
    } else {
      small_role<L, FUSED>(b, src, t, grads, gstride, k, kp, need_init, wave, nwaves, rg, pen_acc);
    }
  }
  if (FUSED || key_pen(rg)) flush_penalty(b, pen_acc);
#ifdef DFH_BWD_TRACE
  if (threadIdx.x == 0 && blockIdx.x < 8192) {  // measurement build only (tools/): per-block role and wall-clock span
    g_bwd_trace[blockIdx.x * 3 + 0] = is_big ? (big_id < nb_hot ? 0ull : 1ull) : 2ull;
    g_bwd_trace[blockIdx.x * 3 + 1] = trace_t0;
    g_bwd_trace[blockIdx.x * 3 + 2] = wall_clock64();
  }
#endif
}

// k_seg_lists: one pass over the unique keys of a localized minibatch, compacting the keys with
// 2 .. BWD_SMALL ("few"), BWD_SMALL+1 .. BWD_MID ("mid") and more ("hot") occurrences into ONE list
// bucket each (one atomic per block and list; the three counters zeroed before).  Used where the minibatch did not come out of k_rdx_emit (library-sort Localizer for
// very large batches, batches localized on the host).
__global__ void __launch_bounds__(1024) k_seg_lists(const uint32_t* __restrict__ col_ptr, const uint32_t* __restrict__ d_U,
                                                    uint2* __restrict__ mid0, uint2* __restrict__ hot0, uint2* __restrict__ few0,
                                                    SegEnt* __restrict__ mid_ent, SegEnt* __restrict__ hot_ent,
                                                    SegEnt* __restrict__ few_ent) {
  __shared__ uint32_t cnt[3], base[3];
  const uint32_t U = *d_U;
  for (uint32_t u0 = blockIdx.x * blockDim.x; u0 < U; u0 += gridDim.x * blockDim.x) {
    if (threadIdx.x < 3) cnt[threadIdx.x] = 0;
    __syncthreads();
    const uint32_t u = u0 + threadIdx.x;
    uint32_t len = 0, slot = 0, cbeg = 0, cend = 0;
    if (u < U) {
      cbeg = col_ptr[u];
      cend = col_ptr[u + 1];
      len = cend - cbeg;
    }
    const int which = len > BWD_MID ? 1 : (len > BWD_SMALL ? 0 : (len > 1 ? 2 : -1));
    if (which >= 0) slot = atomicAdd(&cnt[which], 1u);
    __syncthreads();
    if (threadIdx.x == 0 && cnt[0]) base[0] = atomicAdd(&mid0->x, cnt[0]);
    if (threadIdx.x == 1 && cnt[1]) base[1] = atomicAdd(&hot0->x, cnt[1]);
    if (threadIdx.x == 2 && cnt[2]) base[2] = atomicAdd(&few0->x, cnt[2]);
    __syncthreads();
    const SegEnt e = make_uint4(u, cbeg, cend, 0u);
    if (which == 0) mid_ent[base[0] + slot] = e;
    if (which == 1) hot_ent[base[1] + slot] = e;
    if (which == 2) few_ent[base[2] + slot] = e;
    __syncthreads();
  }
}

// one list bucket at offset 0, empty: what k_seg_lists adds to
__global__ void k_seg_lists_reset(uint2* mid0, uint2* hot0, uint2* few0, uint32_t* split_n) {
  if (threadIdx.x == 0 && blockIdx.x == 0) {
    *mid0 = make_uint2(0u, 0u);
    *hot0 = make_uint2(0u, 0u);
    *few0 = make_uint2(0u, 0u);
    *split_n = 0u;   // (an empty split list until the first training step; every step empties it itself: SplitOut)
  }
}

}  // namespace dfh
#endif  // DFH_BACKWARD_HIP_
