// dfh_lbfgs.hip — the full-batch L-BFGS learner's device side (included at the end of dfh_api.hip):
// the vector kernels of LBFGSUpdater, the gather / scatter around dfh_batch_forward / dfh_batch_backward that
// LBFGSLearner::CalcGrad needs, and the dfh_lbfgs object that keeps the training data, the model and the
// optimiser state (w, the gradients, the s / y history) resident in HBM.
//
// Restated from the reference (src/lbfgs/):
//   Inner / Add / Times       lbfgs_utils.h:62-98      fp32 products summed in fp64; Add skips x == 0, x == 1 is a plain add
//   CalcIncreB                lbfgs_twoloop.h:19-43    the 6m+1 inner products: k_lb_inner, one pass over the 2m+1 vectors
//   PrepareCalcDirection      lbfgs_updater.h:86-101   g = g_new + grad r(w), y = g - g_old, s_last *= alpha: folded into k_lb_inner
//   CalcDirection             lbfgs_updater.h:107-123  p = sum of Add(d_i, v_i) in order, clamp to +-5, <g, p>: k_lb_combine
//   LineSearch / Evaluate     lbfgs_updater.h:125-133, 170-203   w += (alpha - alpha_) p, r(w), <grad r(w), p>: k_lb_wstep
//   CalcGrad                  lbfgs_learner.cc:246-305 per chunk: k_lb_gather -> forward -> backward -> k_lb_scatter
//   InitWeight                lbfgs_updater.h:33-76    tail filter, lens, V from the rand_r(seed = 0) chain in key order
//
// Warm start (dfh_lbfgs_set_model; the reference declares model_in, lbfgs_param.h:58, and never reads it): the input keys
// are joined onto the object's ascending keys on the device (dfh_join.hip); k_lb_set_model copies a matched key's w, and
// its V where both sides carry one, into the ragged model.  Every other float keeps what InitWeight gave it.
//
// l1 on w (dfh_lbfgs_set_l1 with l1 > 0; the reference declares l1 and comments it out, lbfgs_param.h:84-93): the orthant-wise
// forms of the three vector passes live in dfh_owlqn.hip, included right after this file; with l1 == 0 nothing here changes.
//
// Every reduction is deterministic: per-thread fp64 sums, a fixed-order block reduction into one partial per block
// (the grid depends on n only), then one ordered pass over the partials.  No float atomics.
#include <cmath>
#include <cstdlib>

#pragma clang fp contract(off)

namespace dfh {
namespace lb {

constexpr int MAXM = 16;              // history pairs the one-pass product kernel carries in registers
constexpr int NA = 3;                 // left-hand vectors of k_lb_inner: s_last, y_last, g
constexpr int NB = 2 * MAXM + 1;      // right-hand vectors: s_0 .. s_{m-1}, y_0 .. y_{m-1}, g
constexpr int THREADS = 256;
constexpr int MAXBLOCKS = 2048;

inline int blocks_for(uint64_t n, int per_thread) {
  const uint64_t b = (n + (uint64_t)THREADS * per_thread - 1) / ((uint64_t)THREADS * per_thread);
  return (int)std::max<uint64_t>(1, std::min<uint64_t>(b, MAXBLOCKS));
}

// PrepareCalcDirection folded into the product pass (lbfgs_updater.h:86-101): in the element's own thread, before the
// products, g' = g_new + coef w (AddRegularizerGrad, :170-184), y_last = g' - g (the new history slot), s_last *= alpha
struct Prep {
  const float* gnew;
  const float* w;
  const uint32_t* vmask;   // bit i: element i is a V entry (coef V_l2); NULL: every element is a w (coef l2)
  float l2, V_l2;
  float alpha;             // Times(alpha, s_last): skipped when alpha == 1
  int is, iy, ig;          // indices of s_last, y_last, g in the right-hand list
};

struct InnerArgs {
  const float* a[NA];
  const float* b[NB];
  int alias[NA];   // a[i] is b[alias[i]] (its loaded value is reused), -1: a vector of its own
  int na, nb;
  uint64_t n;
  double* part;    // [gridDim.x][na * nb]
};

__device__ __forceinline__ float coef_of(const uint32_t* vmask, uint64_t i, float l2, float V_l2) {
  return (vmask && ((vmask[i >> 5] >> (i & 31)) & 1u)) ? V_l2 : l2;
}

template <int V>
__device__ __forceinline__ void load_v(const float* p, uint64_t i0, uint64_t n, float (&v)[V]) {
  if (i0 + V <= n) {
    if (V == 4) {
      const float4 t = *reinterpret_cast<const float4*>(p + i0);
      v[0] = t.x; v[1] = t.y; v[2] = t.z; v[3] = t.w;
    } else if (V == 2) {
      const float2 t = *reinterpret_cast<const float2*>(p + i0);
      v[0] = t.x; v[1] = t.y;
    } else {
      v[0] = p[i0];
    }
  } else {
#pragma unroll
    for (int j = 0; j < V; ++j) v[j] = i0 + j < n ? p[i0 + j] : 0.f;
  }
}

template <int V>
__device__ __forceinline__ void store_v(float* p, uint64_t i0, uint64_t n, const float (&v)[V]) {
  if (i0 + V <= n) {
    if (V == 4) {
      *reinterpret_cast<float4*>(p + i0) = make_float4(v[0], v[1], v[2], v[3]);
    } else if (V == 2) {
      *reinterpret_cast<float2*>(p + i0) = make_float2(v[0], v[1]);
    } else {
      p[i0] = v[0];
    }
  } else {
#pragma unroll
    for (int j = 0; j < V; ++j)
      if (i0 + j < n) p[i0 + j] = v[j];
  }
}

__device__ __forceinline__ double wave_sum_dbl(double v) {
#pragma unroll
  for (int o = 32; o > 0; o >>= 1) v += __shfl_xor(v, o, 64);
  return v;
}

// sum of every thread's acc[q] (q < np) in a fixed order: lanes by butterfly, then the block's waves in order;
// part[q] = the block's total.  sh: [THREADS / 64][np] doubles of LDS.
template <int P>
__device__ __forceinline__ void block_partials(const double (&acc)[P], int np, double* sh, double* part) {
  const int wv = threadIdx.x >> 6, nw = THREADS / 64;
#pragma unroll
  for (int q = 0; q < P; ++q) {
    if (q < np) {
      const double s = wave_sum_dbl(acc[q]);
      if ((threadIdx.x & 63) == 0) sh[wv * np + q] = s;
    }
  }
  __syncthreads();
  for (int q = threadIdx.x; q < np; q += THREADS) {
    double s = 0.0;
    for (int w = 0; w < nw; ++w) s += sh[w * np + q];
    part[q] = s;
  }
}

// CalcIncreB's inner products (and, with PREP, PrepareCalcDirection before them), one pass: every right-hand vector is
// read once, a left-hand vector that is one of them is not read again.  NBT: the compile-time bound on nb; V: elements
// per thread and iteration (fewer for more vectors, to stay in registers)
template <int NBT, int V, bool PREP>
__global__ void __launch_bounds__(THREADS) k_lb_inner(InnerArgs a, Prep pr, float* __restrict__ g_out, float* __restrict__ y_out,
                                                      float* __restrict__ s_out) {
  extern __shared__ double lb_sh[];
  double acc[NA * NBT];
#pragma unroll
  for (int q = 0; q < NA * NBT; ++q) acc[q] = 0.0;
  const uint64_t stride = (uint64_t)gridDim.x * THREADS * V;
  for (uint64_t i0 = ((uint64_t)blockIdx.x * THREADS + threadIdx.x) * V; i0 < a.n; i0 += stride) {
    float vb[NBT][V];
#pragma unroll
    for (int ib = 0; ib < NBT; ++ib) {
      if (ib < a.nb && !(PREP && ib == pr.iy)) {
        load_v<V>(a.b[ib], i0, a.n, vb[ib]);
      } else {
#pragma unroll
        for (int j = 0; j < V; ++j) vb[ib][j] = 0.f;
      }
    }
    if (PREP) {
      float gn[V], w[V], gold[V], slast[V];
      load_v<V>(pr.gnew, i0, a.n, gn);
      load_v<V>(pr.w, i0, a.n, w);
#pragma unroll
      for (int ib = 0; ib < NBT; ++ib) {
#pragma unroll
        for (int j = 0; j < V; ++j) {
          if (ib == pr.ig) gold[j] = vb[ib][j];
          if (ib == pr.is) slast[j] = vb[ib][j];
        }
      }
      float gp[V], yn[V], sn[V];
#pragma unroll
      for (int j = 0; j < V; ++j) {
        const float c = coef_of(pr.vmask, i0 + j, pr.l2, pr.V_l2);
        gp[j] = gn[j] + c * w[j];                          // AddRegularizerGrad
        yn[j] = gp[j] + (-1.f) * gold[j];                  // y = g_new; Add(-1, g_old, &y)
        sn[j] = pr.alpha == 1.f ? slast[j] : slast[j] * pr.alpha;   // Times(alpha, &s.back())
      }
#pragma unroll
      for (int ib = 0; ib < NBT; ++ib) {
#pragma unroll
        for (int j = 0; j < V; ++j) {
          if (ib == pr.ig) vb[ib][j] = gp[j];
          if (ib == pr.iy) vb[ib][j] = yn[j];
          if (ib == pr.is) vb[ib][j] = sn[j];
        }
      }
      store_v<V>(g_out, i0, a.n, gp);
      store_v<V>(y_out, i0, a.n, yn);
      if (pr.alpha != 1.f) store_v<V>(s_out, i0, a.n, sn);
    }
#pragma unroll
    for (int ia = 0; ia < NA; ++ia) {
      if (ia >= a.na) continue;
      float va[V];
      if (a.alias[ia] >= 0) {
#pragma unroll
        for (int ib = 0; ib < NBT; ++ib)
          if (ib == a.alias[ia]) {
#pragma unroll
            for (int j = 0; j < V; ++j) va[j] = vb[ib][j];
          }
      } else {
        load_v<V>(a.a[ia], i0, a.n, va);
      }
#pragma unroll
      for (int ib = 0; ib < NBT; ++ib) {
        if (ib >= a.nb) continue;
        double s = acc[ia * NBT + ib];
#pragma unroll
        for (int j = 0; j < V; ++j) s += (double)(va[j] * vb[ib][j]);   // Inner: float product, double sum
        acc[ia * NBT + ib] = s;
      }
    }
  }
  block_partials<NA * NBT>(acc, NA * NBT, lb_sh, a.part + (size_t)blockIdx.x * (NA * NBT));
}

// epoch 0 of PrepareCalcDirection: g = g_new + grad r(w) (AddRegularizerGrad, lbfgs_updater.h:170-184), no history yet
__global__ void __launch_bounds__(THREADS) k_lb_addreg(float* __restrict__ g, const float* __restrict__ gnew, const float* __restrict__ w,
                                                       const uint32_t* __restrict__ vmask, float l2, float V_l2, uint64_t n) {
  for (uint64_t i = (uint64_t)blockIdx.x * THREADS + threadIdx.x; i < n; i += (uint64_t)gridDim.x * THREADS)
    g[i] = gnew[i] + coef_of(vmask, i, l2, V_l2) * w[i];
}

// one block per quantity: the blocks' partials in order (per-thread strided sums, then a fixed tree)
__global__ void __launch_bounds__(THREADS) k_lb_finish(const double* __restrict__ part, int nparts, int np, double* __restrict__ out) {
  __shared__ double sh[THREADS];
  const int q = blockIdx.x;
  double s = 0.0;
  for (int b = threadIdx.x; b < nparts; b += THREADS) s += part[(size_t)b * np + q];
  sh[threadIdx.x] = s;
  __syncthreads();
  for (int h = THREADS / 2; h > 0; h >>= 1) {
    if (threadIdx.x < h) sh[threadIdx.x] += sh[threadIdx.x + h];
    __syncthreads();
  }
  if (threadIdx.x == 0) out[q] = sh[0];
}

// CalcDirection (lbfgs_updater.h:107-123 with Twoloop::CalcDirection's closing Adds, lbfgs_twoloop.h:103-107): per element,
// p = 0; Add(c_k, v_k, &p) for k in order (c == 0 skipped, c == 1 a plain add); clamp to +-clampv; out = p (out may be one
// of the v_k: every element is read before it is written, by the same thread); and <dot, p> (Inner(grads_, dir))
struct CombArgs {
  const float* v[NB];
  float c[NB];
  int nv;
  float clampv;
  uint64_t n;
  float* out;
  const float* dot;
  double* part;
};

template <int V>
__global__ void __launch_bounds__(THREADS) k_lb_combine(CombArgs a) {
  __shared__ double sh[THREADS / 64];
  double acc[1] = {0.0};
  const uint64_t stride = (uint64_t)gridDim.x * THREADS * V;
  for (uint64_t i0 = ((uint64_t)blockIdx.x * THREADS + threadIdx.x) * V; i0 < a.n; i0 += stride) {
    float p[V];
#pragma unroll
    for (int j = 0; j < V; ++j) p[j] = 0.f;
    for (int k = 0; k < a.nv; ++k) {
      const float x = a.c[k];
      if (x == 0.f) continue;
      float v[V];
      load_v<V>(a.v[k], i0, a.n, v);
      if (x == 1.f) {
#pragma unroll
        for (int j = 0; j < V; ++j) p[j] += v[j];
      } else {
#pragma unroll
        for (int j = 0; j < V; ++j) p[j] += x * v[j];
      }
    }
    const float cl = a.clampv;
#pragma unroll
    for (int j = 0; j < V; ++j) p[j] = p[j] > cl ? cl : (p[j] < -cl ? -cl : p[j]);
    if (a.dot) {
      float d[V];
      load_v<V>(a.dot, i0, a.n, d);
#pragma unroll
      for (int j = 0; j < V; ++j)
        if (i0 + j < a.n) acc[0] += (double)(d[j] * p[j]);
    }
    store_v<V>(a.out, i0, a.n, p);
  }
  block_partials<1>(acc, 1, sh, a.part + blockIdx.x);
}

// line-search step on the model (LBFGSUpdater::LineSearch + Evaluate, lbfgs_updater.h:125-133, 170-203):
// w += x p (Add: x == 0 skipped, x == 1 plain), then r(w) = sum .5 coef w^2, <grad r(w), p> = sum (coef w) p and nnz(w)
struct WstepArgs {
  float* w;
  const float* p;   // NULL: no step, no <grad r, p>
  float x;
  const uint32_t* vmask;
  float l2, V_l2;
  uint64_t n;
  double* part;     // [gridDim.x][3]
};

template <int V>
__global__ void __launch_bounds__(THREADS) k_lb_wstep(WstepArgs a) {
  __shared__ double sh[(THREADS / 64) * 3];
  double acc[3] = {0.0, 0.0, 0.0};
  const uint64_t stride = (uint64_t)gridDim.x * THREADS * V;
  for (uint64_t i0 = ((uint64_t)blockIdx.x * THREADS + threadIdx.x) * V; i0 < a.n; i0 += stride) {
    float w[V], p[V];
    load_v<V>(a.w, i0, a.n, w);
    if (a.p) load_v<V>(a.p, i0, a.n, p);
    if (a.p && a.x != 0.f) {
#pragma unroll
      for (int j = 0; j < V; ++j) w[j] = a.x == 1.f ? w[j] + p[j] : w[j] + a.x * p[j];
      store_v<V>(a.w, i0, a.n, w);
    }
#pragma unroll
    for (int j = 0; j < V; ++j) {
      if (i0 + j >= a.n) continue;
      const float c = coef_of(a.vmask, i0 + j, a.l2, a.V_l2);
      acc[0] += .5 * (double)c * (double)w[j] * (double)w[j];   // objv += .5 * coef * w * w
      if (a.p) acc[1] += (double)((c * w[j]) * p[j]);           // grads = coef w; Inner(grads, p)
      acc[2] += w[j] != 0.f ? 1.0 : 0.0;
    }
  }
  block_partials<3>(acc, 3, sh, a.part + (size_t)blockIdx.x * 3);
}

// CalcGrad's data side, per chunk: the chunk's packed rows [w, has_V, 0, 0 | V..] (dfh_row_stride) out of the model
// (GetPos, lbfgs_learner.cc:351-367: a key the model does not hold, map = -1, gets a zero row) ...
// Lane layout of both kernels, without divisions: a wave holds 64 >> shift keys side by side, each on (1 << shift) lanes
// (the row stride rounded up to a power of two, at most 64) that step through the row's floats.
struct RowLanes {
  uint32_t U, stride, shift;
};

__device__ __forceinline__ void row_lanes(const RowLanes& r, uint32_t* u0, uint32_t* c0, uint32_t* ustep) {
  const uint32_t lane = threadIdx.x & 63u, wave = (blockIdx.x * THREADS + threadIdx.x) >> 6;
  const uint32_t per_wave = 64u >> r.shift;
  *u0 = wave * per_wave + (lane >> r.shift);
  *c0 = lane & ((1u << r.shift) - 1u);
  *ustep = (gridDim.x * (THREADS / 64)) * per_wave;
}

__global__ void __launch_bounds__(THREADS) k_lb_gather(const float* __restrict__ w, const int64_t* __restrict__ pos,
                                                       const int32_t* __restrict__ map, RowLanes r, float* __restrict__ rows) {
  uint32_t u, c0, ustep;
  row_lanes(r, &u, &c0, &ustep);
  for (; u < r.U; u += ustep) {
    const int32_t i = map[u];
    int64_t p0 = 0, len = 0;
    if (i >= 0) {
      p0 = pos[i];
      len = pos[i + 1] - p0;
    }
    float* row = rows + (size_t)u * r.stride;
    for (uint32_t c = c0; c < r.stride; c += 1u << r.shift) {
      float v = 0.f;
      if (i >= 0) {
        if (c == 0) v = w[p0];
        else if (c == 1) v = len > 1 ? 1.f : 0.f;
        else if (c >= 4 && (int64_t)c - 3 < len) v = w[p0 + (c - 3)];
      }
      row[c] = v;
    }
  }
}

// ... and the chunk's gradient rows added into the model-shaped gradient: the first lens floats of each key only (a key
// without V gets no V gradient).  A key occurs once per chunk and chunks run in order on one stream: no atomics.
__global__ void __launch_bounds__(THREADS) k_lb_scatter(const float* __restrict__ grows, const int64_t* __restrict__ pos,
                                                        const int32_t* __restrict__ map, RowLanes r, float* __restrict__ g) {
  uint32_t u, c0, ustep;
  row_lanes(r, &u, &c0, &ustep);
  for (; u < r.U; u += ustep) {
    const int32_t i = map[u];
    if (i < 0) continue;
    const int64_t p0 = pos[i], len = pos[i + 1] - p0;
    const float* row = grows + (size_t)u * r.stride;
    for (uint32_t c = c0; c < r.stride; c += 1u << r.shift) {
      if (c >= 1 && c <= 3) continue;
      const int64_t j = c == 0 ? 0 : (int64_t)c - 3;
      if (j < len) g[p0 + j] += row[c];
    }
  }
}

// warm start: input key u (model position jpos[u], -1 = not in the model) brings ilen = ipos[u + 1] - ipos[u] floats
// (w [, V]); the model's entry holds mlen.  Both are 1 or 1 + V_dim: the first min(mlen, ilen) floats are copied, so V
// only where both sides have one.  Input keys are unique: one writer per float.  Lanes as k_lb_gather's.
__global__ void __launch_bounds__(THREADS) k_lb_set_model(const int32_t* __restrict__ jpos, const uint64_t* __restrict__ ipos,
                                                          const float* __restrict__ vals, const int64_t* __restrict__ pos, RowLanes r,
                                                          float* __restrict__ w) {
  uint32_t u, c0, ustep;
  row_lanes(r, &u, &c0, &ustep);
  for (; u < r.U; u += ustep) {
    const int32_t i = jpos[u];
    if (i < 0) continue;
    const int64_t p0 = pos[i], mlen = pos[i + 1] - p0;
    const uint64_t q0 = ipos[u];
    const int64_t ilen = (int64_t)(ipos[u + 1] - q0);
    const int64_t len = mlen < ilen ? mlen : ilen;
    for (int64_t c = c0; c < len; c += 1u << r.shift) w[p0 + c] = vals[q0 + c];
  }
}

// CalcGrad's closing transform when gamma != 1 (lbfgs_learner.cc:300-302): pow of the float arguments evaluated in double
// (C++'s pow on the float gamma and fabs), the signed result rounded to float on assignment
__global__ void __launch_bounds__(THREADS) k_lb_gamma(float* __restrict__ g, uint64_t n, float gamma) {
  for (uint64_t i = (uint64_t)blockIdx.x * THREADS + threadIdx.x; i < n; i += (uint64_t)gridDim.x * THREADS) {
    const float x = g[i];
    g[i] = (float)((x > 0 ? 1 : -1) * pow((double)fabsf(x), (double)gamma));
  }
}

// The sharded object's exchange around CalcGrad (dfh_lbfgs_create_sharded).  Both index lists are built once, in
// init_model, and the data never changes.
// Owner side, before the pull: the ragged rows of the pull list, requester after requester, out of the owned slice
// of w: send[i] = w[src[i]].  The buffer is contiguous in peer order, the layout of the all-to-all-v's send side.
__global__ void __launch_bounds__(THREADS) k_lb_pack(const float* __restrict__ w, const uint32_t* __restrict__ src, uint64_t cnt,
                                                     float* __restrict__ send) {
  for (uint64_t i = (uint64_t)blockIdx.x * THREADS + threadIdx.x; i < cnt; i += (uint64_t)gridDim.x * THREADS) send[i] = w[src[i]];
}

// Owner side, after the push: the gradient rows come back in the layout the pack wrote, so the contributions to owned
// element p sit at recv[idx[rptr[p] .. rptr[p+1])], ascending, which is ascending source rank.  g[p] = 0 + each of them
// in that order, written once: the same bits on every run and over every transport (no atomics).
__global__ void __launch_bounds__(THREADS) k_lb_reduce(const float* __restrict__ recv, const uint32_t* __restrict__ rptr,
                                                       const uint32_t* __restrict__ idx, uint64_t n, float* __restrict__ g) {
  for (uint64_t p = (uint64_t)blockIdx.x * THREADS + threadIdx.x; p < n; p += (uint64_t)gridDim.x * THREADS) {
    float s = 0.f;
    for (uint32_t e = rptr[p], e1 = rptr[p + 1]; e < e1; ++e) s += recv[idx[e]];
    g[p] = s;
  }
}

// a chunk's loss (the forward's per-block partials, in slot order per thread, then a fixed tree) and AUC x n into
// out[0..1]; the slots are cleared for the next chunk by the caller
__global__ void __launch_bounds__(THREADS) k_lb_take_prog(const double* __restrict__ prog, double* __restrict__ out) {
  __shared__ double sh[THREADS];
  double s = 0.0;
  for (int i = threadIdx.x; i < PROG_SLOTS; i += THREADS) s += prog[PROG_LOSS * PROG_SLOTS + i];
  sh[threadIdx.x] = s;
  __syncthreads();
  for (int h = THREADS / 2; h > 0; h >>= 1) {
    if (threadIdx.x < h) sh[threadIdx.x] += sh[threadIdx.x + h];
    __syncthreads();
  }
  if (threadIdx.x == 0) {
    out[0] = sh[0];
    out[1] = prog[PROG_AUC * PROG_SLOTS];
  }
}

// ------------------------------------------------------------------ host-side launchers
inline size_t part_bytes(int np) { return (size_t)MAXBLOCKS * np * sizeof(double) + (size_t)np * sizeof(double) + 512; }

bool aligned16(const void* p) { return (reinterpret_cast<uintptr_t>(p) & 15u) == 0; }

// the partials (part) and results (res) live in device memory the caller provides; res is left on the device
int launch_inner(hipStream_t s, InnerArgs a, const Prep* pr, float* g_out, float* y_out, float* s_out, double* part, double* res) {
  const int np_bound = a.nb <= 3 ? 3 : a.nb <= 11 ? 11 : a.nb <= 21 ? 21 : NB;
  Prep p0{};
  p0.is = p0.iy = p0.ig = -1;
  const Prep& P = pr ? *pr : p0;
  int nblk = 0;
  a.part = part;
#define LB_INNER(NBT, V)                                                                                                    \
  do {                                                                                                                      \
    nblk = blocks_for(a.n, V);                                                                                              \
    const size_t shm = (size_t)(THREADS / 64) * NA * NBT * sizeof(double);                                                  \
    if (pr) hipLaunchKernelGGL((k_lb_inner<NBT, V, true>), dim3(nblk), dim3(THREADS), shm, s, a, P, g_out, y_out, s_out); \
    else hipLaunchKernelGGL((k_lb_inner<NBT, V, false>), dim3(nblk), dim3(THREADS), shm, s, a, P, g_out, y_out, s_out);   \
  } while (0)
  switch (np_bound) {
    case 3: LB_INNER(3, 4); break;
    case 11: LB_INNER(11, 4); break;
    case 21: LB_INNER(21, 2); break;
    default: LB_INNER(NB, 1); break;
  }
#undef LB_INNER
  DFH_HIP(hipGetLastError());
  const int np = NA * np_bound;
  hipLaunchKernelGGL(k_lb_finish, dim3(np), dim3(THREADS), 0, s, part, nblk, np, res);
  DFH_HIP(hipGetLastError());
  return DFH_OK;
}
// the [ia][ib] products out of launch_inner's result block
inline double inner_at(const std::vector<double>& res, int nb, int ia, int ib) {
  const int np_bound = nb <= 3 ? 3 : nb <= 11 ? 11 : nb <= 21 ? 21 : NB;
  return res[(size_t)ia * np_bound + ib];
}
inline size_t inner_res_size(int nb) { return (size_t)NA * (nb <= 3 ? 3 : nb <= 11 ? 11 : nb <= 21 ? 21 : NB); }

int launch_combine(hipStream_t s, CombArgs a, double* part, double* res) {
  const int nblk = blocks_for(a.n, 4);
  a.part = part;
  hipLaunchKernelGGL((k_lb_combine<4>), dim3(nblk), dim3(THREADS), 0, s, a);
  hipLaunchKernelGGL(k_lb_finish, dim3(1), dim3(THREADS), 0, s, part, nblk, 1, res);
  DFH_HIP(hipGetLastError());
  return DFH_OK;
}

int launch_wstep(hipStream_t s, WstepArgs a, double* part, double* res) {
  const int nblk = blocks_for(a.n, 4);
  a.part = part;
  hipLaunchKernelGGL((k_lb_wstep<4>), dim3(nblk), dim3(THREADS), 0, s, a);
  hipLaunchKernelGGL(k_lb_finish, dim3(3), dim3(THREADS), 0, s, part, nblk, 3, res);
  DFH_HIP(hipGetLastError());
  return DFH_OK;
}

}  // namespace lb
}  // namespace dfh

#pragma clang fp contract(fast)

using namespace dfh;

struct dfh_lbfgs {
  dfh_ctx* ctx = nullptr;
  int V_dim = 0, m = 0;
  size_t stride = 4;
  struct Chunk : chunks::Resident {
    int32_t* d_map = nullptr;
  };
  std::vector<Chunk> chunks[2];   // [0] training, [1] validation
  size_t max_U = 0;
  // the model: keys ascending, lens, w (ragged: w [, V]) — LBFGSUpdater's feaids_ / weight_lens_ / weights_
  bool inited = false;
  std::vector<uint64_t> keys;
  std::vector<int> lens;
  std::vector<float> cnts;
  uint64_t n = 0;
  float l2 = 0, V_l2 = 0;
  void* arena = nullptr;           // every model-sized vector below, one allocation
  int64_t* d_pos = nullptr;        // [nkeys + 1]
  uint32_t* d_vmask = nullptr;     // [n / 32 + 1] or NULL (V_dim == 0)
  float *d_w = nullptr, *d_gnew = nullptr, *d_g = nullptr;
  std::vector<float*> s, y;        // m slots each
  int s_first = 0, s_count = 0, y_first = 0, y_count = 0;
  bool have_g = false;
  bool grad_run = false;           // a gradient pass has run: the model can no longer be replaced by key
  float alpha = 0;                 // alpha_ of LBFGSUpdater / LBFGSLearner: the last line-search step taken
  float* d_rows = nullptr;         // [max_U x stride] packed rows / gradient rows of the current chunk
  float* d_grows = nullptr;
  double* d_part = nullptr;        // block partials
  double* d_res = nullptr;         // small results: [0, 2 x chunks) per-chunk {loss, AUC x n}, then reduction outputs
  size_t res_cap = 0;
  // the model the chunks read and the gradient they write: d_w / d_pos / d_gnew, or on a sharded object the rank's
  // local ragged model (every key of its chunks that survived, ascending) and its local gradient
  float* d_mw = nullptr;
  int64_t* d_mpos = nullptr;
  float* d_mg = nullptr;
  uint64_t nm = 0;
  // ---- sharded (dfh_lbfgs_create_sharded): a worker for its own chunks, the owner of one slice of the ascending keys
  dfh_comm* comm = nullptr;
  void* sh_arena = nullptr;        // the buffers below, one allocation
  float *d_lw = nullptr, *d_lg = nullptr;   // local ragged model (the pull's receive buffer) and gradient (the push's send buffer)
  int64_t* d_lpos = nullptr;       // [local keys + 1]
  float* d_xbuf = nullptr;         // [nx]: the pack's output (pull send) and the push's receive buffer, same layout
  uint32_t* d_src = nullptr;       // [nx] owned element of every float of the pull list
  uint32_t *d_rptr = nullptr, *d_ridx = nullptr;   // [n + 1], [nx]: the inverted list, ascending source rank per element
  uint64_t nx = 0;
  std::vector<size_t> own_b, loc_b;   // bytes per peer: owner side (pull send = push receive), worker side (the reverse)
  bool pulled = false;             // d_lw holds the current w
  std::vector<uint64_t> splits;    // [world - 1] first keys of shards 1..: the owner of a key is the number of them <= it
  // ---- l1 on w (dfh_lbfgs_set_l1 with l1 > 0, dfh_owlqn.hip): the pseudo-gradient and the line search's origin
  float l1 = 0;
  void* ow_arena = nullptr;        // d_pg and d_w0, allocated by set_l1
  float *d_pg = nullptr, *d_w0 = nullptr;
  bool have_w0 = false;            // a direction has been computed: w0 holds its origin
  double moved = 0;                // elements the last line-search trial moved off w0, over the ranks
};

namespace {

inline float* lb_s(dfh_lbfgs* o, int logical) { return o->s[(o->s_first + logical) % o->m]; }
inline float* lb_y(dfh_lbfgs* o, int logical) { return o->y[(o->y_first + logical) % o->m]; }

// the small-results block's tail (behind the per-chunk {loss, AUC x n} pairs): reduction outputs
inline double* lb_tail(dfh_lbfgs* o) { return o->d_res + 2 * std::max(o->chunks[0].size(), o->chunks[1].size()); }
constexpr size_t kTail = 128;

int lb_fetch(dfh_lbfgs* o, const double* d, size_t cnt, std::vector<double>* out) {
  out->resize(cnt);
  hipStream_t s = o->ctx->stream;
  DFH_HIP(hipMemcpyAsync(out->data(), d, cnt * sizeof(double), hipMemcpyDeviceToHost, s));
  DFH_HIP(hipStreamSynchronize(s));
  return DFH_OK;
}

constexpr const char* kLbWho = "dfh_lbfgs";
constexpr const char* kLbTail = "out-of-core L-BFGS is not supported";

// the l1 > 0 forms of prepare_direction, calc_direction, line_search and of evaluate's r(w), defined in dfh_owlqn.hip
int ow_prepare_direction(dfh_lbfgs* o, float* incr_B, int* mcur);
int ow_calc_direction(dfh_lbfgs* o, const float* d, float* p_g);
int ow_line_search(dfh_lbfgs* o, float alpha, float gamma, float* objv, float* p_g, float* auc_n);
int ow_reg(dfh_lbfgs* o, double out[3]);

// forward (+ AUC) over a chunk's rows, its loss / AUC into res[0..1]; with grad, the backward and the scatter into g
int lb_chunk_pass(dfh_lbfgs* o, dfh_lbfgs::Chunk& ch, bool grad, double* res) {
  dfh_ctx* c = o->ctx;
  hipStream_t s = c->stream;
  const uint32_t U = (uint32_t)ch.U, st = (uint32_t)o->stride;
  uint32_t shift = 0;
  while ((1u << shift) < st && shift < 6) ++shift;
  const lb::RowLanes rl{U, st, shift};
  const uint64_t waves = ((uint64_t)U + (64u >> shift) - 1) / (64u >> shift);
  const int gb = (int)std::max<uint64_t>(1, std::min<uint64_t>((waves + 3) / 4, 8192));
  if (U) hipLaunchKernelGGL(lb::k_lb_gather, dim3(gb), dim3(lb::THREADS), 0, s, o->d_mw, o->d_mpos, ch.d_map, rl, o->d_rows);
  DFH_HIP(hipGetLastError());
  int rc = dfh_batch_forward(ch.b, o->V_dim, o->d_rows);
  if (rc) return rc;
  rc = launch_auc(ch.b);
  if (rc) return rc;
  if (grad && U) {
    rc = dfh_batch_backward(ch.b, o->V_dim, o->d_rows, o->d_grows);
    if (rc) return rc;
    hipLaunchKernelGGL(lb::k_lb_scatter, dim3(gb), dim3(lb::THREADS), 0, s, o->d_grows, o->d_mpos, ch.d_map, rl, o->d_mg);
  }
  hipLaunchKernelGGL(lb::k_lb_take_prog, dim3(1), dim3(lb::THREADS), 0, s, ch.b->d_prog, res);
  DFH_HIP(hipGetLastError());
  DFH_HIP(chunks::reset_prog(ch.b, s));
  ch.b->nrows_seen = 0;
  return DFH_OK;
}

// the sums over ranks of a sharded object's fp64 partials, in rank order (the same bits on every rank); a no-op on a
// plain object.  dfh_comm_allreduce_sum takes 64 values per call.
int lb_allsum(dfh_lbfgs* o, double* v, size_t n) {
  if (!o->comm) return DFH_OK;
  for (size_t i = 0; i < n; i += 64) {
    const int rc = dfh_comm_allreduce_sum(o->comm, v + i, (int)std::min<size_t>(64, n - i));
    if (rc) return rc;
  }
  return DFH_OK;
}

// sharded: the owners' rows of w to the workers that use them.  The receive buffer is the worker's local ragged model.
int lb_pull(dfh_lbfgs* o) {
  hipStream_t s = o->ctx->stream;
  if (o->nx) {
    hipLaunchKernelGGL(lb::k_lb_pack, dim3(lb::blocks_for(o->nx, 1)), dim3(lb::THREADS), 0, s, o->d_w, o->d_src, o->nx, o->d_xbuf);
    DFH_HIP(hipGetLastError());
  }
  const int rc = comm_alltoallv(o->comm, o->d_xbuf, o->own_b.data(), o->d_lw, o->loc_b.data(), nullptr, DFH_XCHG_ROWS);
  if (rc) return rc;
  o->pulled = true;
  return DFH_OK;
}

// sharded: the local gradient back to the owners (it is ordered by owner already), then each owned element's
// contributions added in ascending source rank into g_new
int lb_push_reduce(dfh_lbfgs* o) {
  hipStream_t s = o->ctx->stream;
  const int rc = comm_alltoallv(o->comm, o->d_lg, o->loc_b.data(), o->d_xbuf, o->own_b.data(), nullptr, DFH_XCHG_GRADS);
  if (rc) return rc;
  if (o->n) {
    hipLaunchKernelGGL(lb::k_lb_reduce, dim3(lb::blocks_for(o->n, 1)), dim3(lb::THREADS), 0, s, o->d_xbuf, o->d_rptr, o->d_ridx,
                       (uint64_t)o->n, o->d_gnew);
    DFH_HIP(hipGetLastError());
  }
  return DFH_OK;
}

// LBFGSLearner::CalcGrad (lbfgs_learner.cc:246-305) into g_new; loss and AUC x n summed over the chunks as the reference
// sums them (each chunk's value as a float, in chunk order), on a sharded object then over the ranks in fp64
int lb_calc_grad(dfh_lbfgs* o, float gamma, float* loss, float* auc_n) {
  auto& tr = o->chunks[0];
  hipStream_t s = o->ctx->stream;
  int rc = DFH_OK;
  o->grad_run = true;
  if (o->comm) {
    rc = lb_pull(o);
    if (rc) return rc;
  }
  if (o->nm) DFH_HIP(hipMemsetAsync(o->d_mg, 0, o->nm * sizeof(float), s));
  for (size_t i = 0; i < tr.size(); ++i) {
    rc = lb_chunk_pass(o, tr[i], true, o->d_res + 2 * i);
    if (rc) return rc;
  }
  if (o->comm) {
    rc = lb_push_reduce(o);
    if (rc) return rc;
  }
  if (gamma != 1.f) {
    hipLaunchKernelGGL(lb::k_lb_gamma, dim3(lb::blocks_for(o->n, 1)), dim3(lb::THREADS), 0, s, o->d_gnew, (uint64_t)o->n, gamma);
    DFH_HIP(hipGetLastError());
  }
  std::vector<double> r;
  rc = lb_fetch(o, o->d_res, 2 * tr.size(), &r);
  if (rc) return rc;
  float l = 0, a = 0;
  for (size_t i = 0; i < tr.size(); ++i) {
    l += (float)r[2 * i];
    a += (float)r[2 * i + 1];
  }
  if (o->comm) {
    double t[2] = {l, a};
    rc = lb_allsum(o, t, 2);
    if (rc) return rc;
    l = (float)t[0];
    a = (float)t[1];
  }
  if (loss) *loss = l;
  if (auc_n) *auc_n = a;
  return DFH_OK;
}

int lb_wstep(dfh_lbfgs* o, const float* p, float x, double out[3]) {
  lb::WstepArgs a{o->d_w, p, x, o->d_vmask, o->l2, o->V_l2, (uint64_t)o->n, nullptr};
  double* res = lb_tail(o);
  int rc = lb::launch_wstep(o->ctx->stream, a, o->d_part, res);
  if (rc) return rc;
  std::vector<double> r;
  rc = lb_fetch(o, res, 3, &r);
  if (rc) return rc;
  if (p && x != 0.f) o->pulled = false;
  rc = lb_allsum(o, r.data(), 3);
  if (rc) return rc;
  for (int i = 0; i < 3; ++i) out[i] = r[i];
  return DFH_OK;
}

int lb_free(dfh_lbfgs* o) {
  if (!o) return DFH_OK;
  if (o->ctx) (void)hipSetDevice(o->ctx->device);
  for (auto& cs : o->chunks)
    for (auto& ch : cs) {
      chunks::release(ch);
      if (ch.d_map) (void)hipFree(ch.d_map);
    }
  if (o->arena) (void)hipFree(o->arena);
  if (o->d_rows) (void)hipFree(o->d_rows);
  if (o->d_grows) (void)hipFree(o->d_grows);
  if (o->d_part) (void)hipFree(o->d_part);
  if (o->d_res) (void)hipFree(o->d_res);
  if (o->sh_arena) (void)hipFree(o->sh_arena);
  if (o->ow_arena) (void)hipFree(o->ow_arena);
  delete o;
  return DFH_OK;
}

}  // namespace

extern "C" {

int dfh_vec_inner_multi(dfh_ctx* c, uint64_t n, int na, const float* const* a, int nb, const float* const* b, double* out) {
  DFH_ARG(c && out && a && b, "dfh_vec_inner_multi: NULL argument");
  DFH_ARG(na >= 1 && na <= lb::NA && nb >= 1 && nb <= lb::NB, "dfh_vec_inner_multi: 1 <= na <= 3 and 1 <= nb <= 33");
  lb::InnerArgs ia{};
  ia.na = na;
  ia.nb = nb;
  ia.n = n;
  for (int j = 0; j < nb; ++j) {
    DFH_ARG(b[j] && lb::aligned16(b[j]), "dfh_vec_inner_multi: vectors must be 16-byte aligned device pointers");
    ia.b[j] = b[j];
  }
  for (int i = 0; i < na; ++i) {
    DFH_ARG(a[i] && lb::aligned16(a[i]), "dfh_vec_inner_multi: vectors must be 16-byte aligned device pointers");
    ia.a[i] = a[i];
    ia.alias[i] = -1;
    for (int j = 0; j < nb; ++j)
      if (b[j] == a[i]) ia.alias[i] = j;
  }
  DFH_HIP(hipSetDevice(c->device));
  const size_t rs = lb::inner_res_size(nb);
  int rc = ensure_scratch(c, lb::part_bytes((int)rs) + padded<double>(rs));
  if (rc) return rc;
  Carver cv(c->scratch);
  double* part = cv.take<double>((size_t)lb::MAXBLOCKS * rs);
  double* res = cv.take<double>(rs);
  rc = lb::launch_inner(c->stream, ia, nullptr, nullptr, nullptr, nullptr, part, res);
  if (rc) return rc;
  std::vector<double> h(rs);
  DFH_HIP(hipMemcpyAsync(h.data(), res, rs * sizeof(double), hipMemcpyDeviceToHost, c->stream));
  DFH_HIP(hipStreamSynchronize(c->stream));
  for (int i = 0; i < na; ++i)
    for (int j = 0; j < nb; ++j) out[i * nb + j] = lb::inner_at(h, nb, i, j);
  return DFH_OK;
}

int dfh_vec_combine(dfh_ctx* c, uint64_t n, int nv, const float* const* v, const float* coef, float clampv, float* out,
                    const float* dot, double* out_dot) {
  DFH_ARG(c && out && (nv == 0 || (v && coef)), "dfh_vec_combine: NULL argument");
  DFH_ARG(nv >= 0 && nv <= lb::NB, "dfh_vec_combine: 0 <= nv <= 33");
  DFH_ARG(lb::aligned16(out) && (!dot || lb::aligned16(dot)), "dfh_vec_combine: vectors must be 16-byte aligned");
  lb::CombArgs ca{};
  for (int k = 0; k < nv; ++k) {
    DFH_ARG(coef[k] == 0.f || (v[k] && lb::aligned16(v[k])), "dfh_vec_combine: vectors must be 16-byte aligned device pointers");
    ca.v[k] = v[k];
    ca.c[k] = coef[k];
  }
  ca.nv = nv;
  ca.clampv = clampv;
  ca.n = n;
  ca.out = out;
  ca.dot = dot;
  DFH_HIP(hipSetDevice(c->device));
  int rc = ensure_scratch(c, lb::part_bytes(1) + padded<double>(1));
  if (rc) return rc;
  Carver cv(c->scratch);
  double* part = cv.take<double>(lb::MAXBLOCKS);
  double* res = cv.take<double>(1);
  rc = lb::launch_combine(c->stream, ca, part, res);
  if (rc) return rc;
  double h = 0;
  DFH_HIP(hipMemcpyAsync(&h, res, sizeof(double), hipMemcpyDeviceToHost, c->stream));
  DFH_HIP(hipStreamSynchronize(c->stream));
  if (out_dot) *out_dot = h;
  return DFH_OK;
}

int dfh_vec_line_step(dfh_ctx* c, uint64_t n, float* w, const float* p, float x, const uint32_t* vmask, float l2, float V_l2,
                      double* out3) {
  DFH_ARG(c && w && out3, "dfh_vec_line_step: NULL argument");
  DFH_ARG(lb::aligned16(w) && (!p || lb::aligned16(p)), "dfh_vec_line_step: vectors must be 16-byte aligned");
  DFH_HIP(hipSetDevice(c->device));
  int rc = ensure_scratch(c, lb::part_bytes(3) + padded<double>(3));
  if (rc) return rc;
  Carver cv(c->scratch);
  double* part = cv.take<double>((size_t)lb::MAXBLOCKS * 3);
  double* res = cv.take<double>(3);
  rc = lb::launch_wstep(c->stream, lb::WstepArgs{w, p, x, vmask, l2, V_l2, n, nullptr}, part, res);
  if (rc) return rc;
  DFH_HIP(hipMemcpyAsync(out3, res, 3 * sizeof(double), hipMemcpyDeviceToHost, c->stream));
  DFH_HIP(hipStreamSynchronize(c->stream));
  return DFH_OK;
}

int dfh_lbfgs_create(dfh_ctx* c, int V_dim, int m, dfh_lbfgs** out) {
  DFH_ARG(c && out, "dfh_lbfgs_create: NULL argument");
  DFH_ARG(V_dim >= 0 && V_dim <= 256, "dfh_lbfgs_create: 0 <= V_dim <= 256");
  DFH_ARG(m >= 1 && m <= lb::MAXM, "dfh_lbfgs_create: this build keeps 1 <= m <= 16 history pairs");
  dfh_lbfgs* o = new (std::nothrow) dfh_lbfgs();
  DFH_ARG(o != nullptr, "out of host memory");
  o->ctx = c;
  o->V_dim = V_dim;
  o->m = m;
  o->stride = dfh_row_stride(V_dim);
  *out = o;
  return DFH_OK;
}

int dfh_lbfgs_destroy(dfh_lbfgs* o) { return lb_free(o); }

int dfh_lbfgs_add_chunk(dfh_lbfgs* o, int is_val, size_t nrows, const size_t* offset, const uint64_t* index, const float* value,
                        const float* label) {
  DFH_ARG(o && offset && label && nrows >= 1, "dfh_lbfgs_add_chunk: bad argument");
  DFH_ARG(!o->inited, "dfh_lbfgs_add_chunk: the model is already initialised");
  const size_t nnz = offset[nrows] - offset[0];
  // + the key map and the X V buffer the first forward allocates (ensure_xv)
  const size_t extra = (nnz + 1) * sizeof(int32_t) + nrows * (size_t)std::max((o->V_dim + 3) / 4 * 4, 4) * sizeof(float);
  dfh_lbfgs::Chunk ch;
  const int rc = chunks::add(o->ctx, kLbWho, kLbTail, extra, nrows, offset, index, value, label, &ch);
  if (rc) return rc;
  o->max_U = std::max(o->max_U, ch.U);
  o->chunks[is_val ? 1 : 0].push_back(std::move(ch));
  return DFH_OK;
}

}  // extern "C"

namespace {

// what a worker asks a key's owner: the key, this rank's merged training count, whether its training chunks hold it
// (a key of the validation chunks alone is asked for its row and never enters the model)
struct LbReq {
  uint64_t key;
  float cnt;
  uint32_t train;
};

// Set-up of a sharded object.  Split keys balanced on the ranks' training keys; every rank's requests to the owners;
// the owner adds the counts over ranks (in rank order), filters on the global counts and builds its slice (keys,
// cnts, lens); it answers every request with the key's lens, 0 when the key is not in the model.  Out: the worker's
// local model (its surviving keys ascending, grouped by owner, and their lens), the pull list (src: the owned
// element of every float the owner sends, requester after requester) and the bytes per peer of both sides.
int lb_shard_model(dfh_lbfgs* o, float filter, int V_threshold, const std::vector<uint64_t>& tk, const std::vector<float>& tc,
                   std::vector<uint64_t>* lkeys, std::vector<int>* llens, std::vector<uint32_t>* src) {
  const int W = o->comm->world, k = o->V_dim;
  std::vector<uint64_t> vk;
  for (auto& ch : o->chunks[1]) vk.insert(vk.end(), ch.keys.begin(), ch.keys.end());
  std::sort(vk.begin(), vk.end());
  vk.erase(std::unique(vk.begin(), vk.end()), vk.end());
  std::vector<LbReq> req;
  req.reserve(tk.size() + vk.size());
  for (size_t i = 0, j = 0; i < tk.size() || j < vk.size();) {
    if (j < vk.size() && (i == tk.size() || vk[j] < tk[i])) {
      req.push_back(LbReq{vk[j++], 0.f, 0u});
    } else {
      if (j < vk.size() && vk[j] == tk[i]) ++j;
      req.push_back(LbReq{tk[i], tc[i], 1u});
      ++i;
    }
  }
  std::vector<uint64_t> splits(std::max(W - 1, 1), 0);
  int rc = dfh_shard_balanced_splits(o->comm, tk.data(), tk.size(), splits.data());
  if (rc) return rc;
  o->splits.assign(splits.begin(), splits.begin() + (W - 1));
  // the owner of a key: the number of split keys at or below it
  std::vector<int> owner(req.size());
  std::vector<uint64_t> nreq(W, 0), nrecv(W, 0);
  for (size_t i = 0; i < req.size(); ++i) {
    owner[i] = (int)(std::upper_bound(splits.begin(), splits.begin() + (W - 1), req[i].key) - splits.begin());
    ++nreq[owner[i]];
  }
  // the set-up's three all-to-all-vs of host bytes: the host-staged exchange (dfh_comm.hip) with transient buffers; synchronous
  std::vector<size_t> sb(W, 8), rb(W, 8), seg(W + 1, 0);
  rc = HostXchg{o->comm, "dfh_lbfgs_init_model", HostXchg::TRANSIENT}.exchange(nreq.data(), sb.data(), nullptr, nrecv.data(), rb.data(), DFH_XCHG_OTHER);
  if (rc) return rc;
  for (int p = 0; p < W; ++p) {
    sb[p] = nreq[p] * sizeof(LbReq);
    rb[p] = nrecv[p] * sizeof(LbReq);
    seg[p + 1] = seg[p] + nrecv[p];
  }
  std::vector<LbReq> got(seg[W]);
  rc = HostXchg{o->comm, "dfh_lbfgs_init_model", HostXchg::TRANSIENT}.exchange(req.data(), sb.data(), nullptr, got.data(), rb.data(), DFH_XCHG_OTHER);
  if (rc) return rc;
  // owner: every source's list is ascending and the sources lie in rank order; a stable sort by key keeps that order
  std::vector<uint32_t> ord(got.size());
  for (size_t i = 0; i < ord.size(); ++i) ord[i] = (uint32_t)i;
  std::stable_sort(ord.begin(), ord.end(), [&](uint32_t a, uint32_t b) { return got[a].key < got[b].key; });
  for (size_t i = 0; i < ord.size();) {
    size_t j = i;
    float cnt = 0;
    bool train = false;
    for (; j < ord.size() && got[ord[j]].key == got[ord[i]].key; ++j) {
      cnt += got[ord[j]].cnt;
      train = train || got[ord[j]].train;
    }
    // RemoveTailFeatures on the global count (lbfgs_utils.h:100-116)
    if (train && (!(filter > 0) || cnt > filter)) {
      o->keys.push_back(got[ord[i]].key);
      o->cnts.push_back(cnt);
    }
    i = j;
  }
  const size_t K = o->keys.size();
  o->lens.assign(K, 1);
  std::vector<uint64_t> pos(K + 1, 0);
  for (size_t i = 0; i < K; ++i) {
    if (k) o->lens[i] = 1 + (o->cnts[i] > V_threshold ? k : 0);
    pos[i + 1] = pos[i] + o->lens[i];
  }
  // the answers, and the pull list in the requesters' order
  std::vector<int32_t> reply(got.size(), 0), ans(req.size(), 0);
  o->own_b.assign(W, 0);
  for (int q = 0; q < W; ++q) {
    size_t j = 0;
    for (size_t e = seg[q]; e < seg[q + 1]; ++e) {
      while (j < K && o->keys[j] < got[e].key) ++j;
      if (j < K && o->keys[j] == got[e].key) {
        reply[e] = o->lens[j];
        for (int c = 0; c < o->lens[j]; ++c) src->push_back((uint32_t)(pos[j] + c));
        o->own_b[q] += (size_t)o->lens[j] * sizeof(float);
      }
    }
  }
  if (pos[K] >= (1ull << 32) || src->size() >= (1ull << 32)) {
    set_error("dfh_lbfgs_init_model: a shard of more than 2^32 - 1 floats or pull entries is not supported");
    return DFH_ERR_CAPACITY;
  }
  for (int p = 0; p < W; ++p) {
    sb[p] = nrecv[p] * sizeof(int32_t);
    rb[p] = nreq[p] * sizeof(int32_t);
  }
  rc = HostXchg{o->comm, "dfh_lbfgs_init_model", HostXchg::TRANSIENT}.exchange(reply.data(), sb.data(), nullptr, ans.data(), rb.data(), DFH_XCHG_OTHER);
  if (rc) return rc;
  // worker: its local model, the surviving keys in ascending order (grouped by owner: the owners' slices ascend)
  o->loc_b.assign(W, 0);
  for (size_t i = 0; i < req.size(); ++i) {
    if (ans[i] <= 0) continue;
    lkeys->push_back(req[i].key);
    llens->push_back(ans[i]);
    o->loc_b[owner[i]] += (size_t)ans[i] * sizeof(float);
  }
  return DFH_OK;
}

}  // namespace

extern "C" {

int dfh_lbfgs_create_sharded(dfh_ctx* c, dfh_comm* comm, int V_dim, int m, dfh_lbfgs** out) {
  DFH_ARG(c && comm && out && comm->ctx == c, "dfh_lbfgs_create_sharded: the context and the communicator must match");
  DFH_ARG(!comm->loopback, "dfh_lbfgs_create_sharded: the loop-back transport is for dfh_shard_step measurements only");
  const int rc = dfh_lbfgs_create(c, V_dim, m, out);
  if (rc) return rc;
  (*out)->comm = comm;
  return DFH_OK;
}

int dfh_lbfgs_init_model(dfh_lbfgs* o, float tail_feature_filter, int V_threshold, float V_init_scale, float l2, float V_l2,
                         uint64_t* nkeys, uint64_t* nparams) {
  DFH_ARG(o && !o->inited, "dfh_lbfgs_init_model: bad argument or called twice");
  DFH_ARG(o->comm || !o->chunks[0].empty(), "dfh_lbfgs_init_model: no training chunk");
  DFH_HIP(hipSetDevice(o->ctx->device));
  const int k = o->V_dim;
  // merged feature counts (KVUnion of every chunk's counts in chunk order, tile_builder.h:171-176)
  std::vector<uint64_t> tk;
  std::vector<float> tc;
  {
    std::vector<const chunks::Resident*> train(o->chunks[0].size());
    for (size_t i = 0; i < train.size(); ++i) train[i] = &o->chunks[0][i];
    chunks::merged_counts(train, &tk, &tc);
  }
  std::vector<uint64_t> lkeys;   // sharded: the worker's local model
  std::vector<int> llens;
  std::vector<uint32_t> src;
  if (o->comm) {
    const int rc = lb_shard_model(o, tail_feature_filter, V_threshold, tk, tc, &lkeys, &llens, &src);
    if (rc) return rc;
  } else {
    for (size_t i = 0; i < tk.size(); ++i) {
      // RemoveTailFeatures (lbfgs_utils.h:100-116): a key survives with cnt > filter
      if (!(tail_feature_filter > 0) || tc[i] > tail_feature_filter) {
        o->keys.push_back(tk[i]);
        o->cnts.push_back(tc[i]);
      }
    }
    o->lens.assign(o->keys.size(), 1);
    if (k)
      for (size_t i = 0; i < o->keys.size(); ++i) o->lens[i] = 1 + (o->cnts[i] > V_threshold ? k : 0);   // InitWeight, lbfgs_updater.h:47-52
  }
  const size_t K = o->keys.size();
  std::vector<int64_t> pos(K + 1, 0);
  for (size_t i = 0; i < K; ++i) pos[i + 1] = pos[i] + o->lens[i];
  o->n = (uint64_t)pos[K];
  o->l2 = l2;
  o->V_l2 = V_l2;
  const uint64_t n = o->n;
  // the rand_r chain runs over the keys of every shard in order: this shard starts behind the draws of shards 0 .. r-1
  uint64_t skip = 0;
  if (o->comm && k) {
    const int W = o->comm->world;
    const uint64_t mine = n - K;
    std::vector<uint64_t> draws(W, 0);
    const int rc = dfh_comm_allgather(o->comm, &mine, sizeof(mine), draws.data());
    if (rc) return rc;
    for (int q = 0; q < o->comm->rank; ++q) skip += draws[q];
  }
  // every model-sized vector in one allocation: w, g_new, g, m s slots, m y slots (each padded to 64 floats), pos, V mask
  const size_t vecf = ((n + 63) / 64) * 64, vec = vecf * sizeof(float);
  const size_t mask_words = k ? (n + 31) / 32 + 1 : 0;
  const size_t arena = (size_t)(3 + 2 * o->m) * vec + ((K + 1) * sizeof(int64_t) + 255) / 256 * 256 + mask_words * 4 + 256;
  const size_t rows = std::max<size_t>(o->max_U, 1) * o->stride * sizeof(float);
  const size_t part = lb::part_bytes(lb::NA * lb::NB);
  // sharded: local model and gradient, local pos, the exchange buffer, the pull list and the inverted list
  uint64_t nl = 0;
  for (int l : llens) nl += (uint64_t)l;
  const uint64_t nx = src.size();
  auto pad = [](size_t b) { return (std::max<size_t>(b, 1) + 255) / 256 * 256; };
  const size_t sh_arena = o->comm ? 2 * pad(nl * sizeof(float)) + pad((lkeys.size() + 1) * sizeof(int64_t)) +
                                        3 * pad(nx * sizeof(uint32_t)) + pad((n + 1) * sizeof(uint32_t))
                                  : 0;
  {
    const int rc = chunks::check_free(kLbWho, "the model and the optimiser state", kLbTail, arena + 2 * rows + part + sh_arena);
    if (rc) return rc;
  }
  DFH_HIP(hipMalloc(&o->arena, arena));
  DFH_HIP(hipMalloc(&o->d_rows, rows));
  DFH_HIP(hipMalloc(&o->d_grows, rows));
  DFH_HIP(hipMalloc(&o->d_part, part));
  o->res_cap = 2 * std::max(o->chunks[0].size(), o->chunks[1].size()) + kTail;
  DFH_HIP(hipMalloc(&o->d_res, o->res_cap * sizeof(double)));
  Carver cv(o->arena);
  o->d_w = cv.take<float>(vecf);
  o->d_gnew = cv.take<float>(vecf);
  o->d_g = cv.take<float>(vecf);
  o->s.resize(o->m);
  o->y.resize(o->m);
  for (int i = 0; i < o->m; ++i) o->s[i] = cv.take<float>(vecf);
  for (int i = 0; i < o->m; ++i) o->y[i] = cv.take<float>(vecf);
  o->d_pos = cv.take<int64_t>(K + 1);
  o->d_vmask = k ? cv.take<uint32_t>(mask_words) : nullptr;
  // w = 0, V from the rand_r(seed = 0) chain in key order (InitWeight, lbfgs_updater.h:58-69)
  std::vector<float> w(n, 0.f);
  std::vector<uint32_t> mask(mask_words, 0u);
  if (k) {
    unsigned seed = 0;
    for (uint64_t d = 0; d < skip; ++d) (void)rand_r(&seed);
    const float scale = V_init_scale * 2;
    for (size_t i = 0; i < K; ++i) {
      for (int j = 1; j < o->lens[i]; ++j) {
        w[pos[i] + j] = (rand_r(&seed) / static_cast<float>(RAND_MAX) - .5) * scale;
        const uint64_t e = (uint64_t)pos[i] + j;
        mask[e >> 5] |= 1u << (e & 31);
      }
    }
  }
  hipStream_t s = o->ctx->stream;
  if (n) DFH_HIP(hipMemcpyAsync(o->d_w, w.data(), n * sizeof(float), hipMemcpyHostToDevice, s));
  DFH_HIP(hipMemcpyAsync(o->d_pos, pos.data(), (K + 1) * sizeof(int64_t), hipMemcpyHostToDevice, s));
  if (k) DFH_HIP(hipMemcpyAsync(o->d_vmask, mask.data(), mask_words * 4, hipMemcpyHostToDevice, s));
  o->d_mw = o->d_w;
  o->d_mpos = o->d_pos;
  o->d_mg = o->d_gnew;
  o->nm = n;
  std::vector<int64_t> lpos;
  std::vector<uint32_t> rptr, ridx;
  if (o->comm) {
    DFH_HIP(hipMalloc(&o->sh_arena, sh_arena));
    // an empty vector still gets a piece of its own, as sh_arena counts it (pad)
    const uint64_t nl1 = std::max<uint64_t>(nl, 1), nx1 = std::max<uint64_t>(nx, 1);
    Carver cs(o->sh_arena);
    o->d_lw = cs.take<float>(nl1);
    o->d_lg = cs.take<float>(nl1);
    o->d_lpos = cs.take<int64_t>(lkeys.size() + 1);
    o->d_xbuf = cs.take<float>(nx1);
    o->d_src = cs.take<uint32_t>(nx1);
    o->d_ridx = cs.take<uint32_t>(nx1);
    o->d_rptr = cs.take<uint32_t>(n + 1);
    o->nx = nx;
    lpos.assign(lkeys.size() + 1, 0);
    for (size_t i = 0; i < lkeys.size(); ++i) lpos[i + 1] = lpos[i] + llens[i];
    // the inverted list: every owned element's entries of the pull list in ascending order (= ascending source rank)
    rptr.assign(n + 1, 0);
    ridx.resize(nx);
    for (uint32_t e : src) ++rptr[e + 1];
    for (uint64_t i = 0; i < n; ++i) rptr[i + 1] += rptr[i];
    std::vector<uint32_t> cur(rptr.begin(), rptr.end() - 1);
    for (uint64_t i = 0; i < nx; ++i) ridx[cur[src[i]]++] = (uint32_t)i;
    DFH_HIP(hipMemcpyAsync(o->d_lpos, lpos.data(), lpos.size() * sizeof(int64_t), hipMemcpyHostToDevice, s));
    if (nx) DFH_HIP(hipMemcpyAsync(o->d_src, src.data(), nx * sizeof(uint32_t), hipMemcpyHostToDevice, s));
    if (nx) DFH_HIP(hipMemcpyAsync(o->d_ridx, ridx.data(), nx * sizeof(uint32_t), hipMemcpyHostToDevice, s));
    DFH_HIP(hipMemcpyAsync(o->d_rptr, rptr.data(), (n + 1) * sizeof(uint32_t), hipMemcpyHostToDevice, s));
    o->d_mw = o->d_lw;
    o->d_mpos = o->d_lpos;
    o->d_mg = o->d_lg;
    o->nm = nl;
  }
  // each chunk's key -> model key map (TileBuilder::BuildColmap, tile_builder.h:59-76: -1 = not in the model); on a
  // sharded object into the local model
  const std::vector<uint64_t>& mkeys = o->comm ? lkeys : o->keys;
  for (auto& cs : o->chunks)
    for (auto& ch : cs) {
      std::vector<int32_t> map;
      chunks::colmap(ch, mkeys, &map);
      DFH_HIP(hipMalloc(&ch.d_map, map.size() * sizeof(int32_t)));
      DFH_HIP(hipMemcpyAsync(ch.d_map, map.data(), map.size() * sizeof(int32_t), hipMemcpyHostToDevice, s));
      DFH_HIP(hipStreamSynchronize(s));
    }
  DFH_HIP(hipStreamSynchronize(s));
  o->inited = true;
  if (nkeys) *nkeys = K;
  if (nparams) *nparams = n;
  return DFH_OK;
}

int dfh_lbfgs_shape(dfh_lbfgs* o, uint64_t* nkeys, uint64_t* nparams, int* ntrain_chunks, int* nval_chunks) {
  DFH_ARG(o, "NULL argument");
  if (nkeys) *nkeys = o->keys.size();
  if (nparams) *nparams = o->n;
  if (ntrain_chunks) *ntrain_chunks = (int)o->chunks[0].size();
  if (nval_chunks) *nval_chunks = (int)o->chunks[1].size();
  return DFH_OK;
}

int dfh_lbfgs_get_model(dfh_lbfgs* o, uint64_t* keys, int* lens, float* feacnt, float* w) {
  DFH_ARG(o && o->inited, "dfh_lbfgs_get_model: the model is not initialised");
  if (keys) std::copy(o->keys.begin(), o->keys.end(), keys);
  if (lens) std::copy(o->lens.begin(), o->lens.end(), lens);
  if (feacnt) std::copy(o->cnts.begin(), o->cnts.end(), feacnt);
  if (w && o->n) {
    DFH_HIP(hipSetDevice(o->ctx->device));
    DFH_HIP(hipMemcpyAsync(w, o->d_w, o->n * sizeof(float), hipMemcpyDeviceToHost, o->ctx->stream));
    DFH_HIP(hipStreamSynchronize(o->ctx->stream));
  }
  return DFH_OK;
}

int dfh_lbfgs_set_weights(dfh_lbfgs* o, const float* w) {
  DFH_ARG(o && o->inited && (w || !o->n), "dfh_lbfgs_set_weights: bad argument");
  DFH_ARG(!o->have_g, "dfh_lbfgs_set_weights: training has started");
  o->pulled = false;
  if (!o->n) return DFH_OK;
  DFH_HIP(hipSetDevice(o->ctx->device));
  DFH_HIP(hipMemcpyAsync(o->d_w, w, o->n * sizeof(float), hipMemcpyHostToDevice, o->ctx->stream));
  DFH_HIP(hipStreamSynchronize(o->ctx->stream));
  return DFH_OK;
}

int dfh_lbfgs_owned_range(dfh_lbfgs* o, uint64_t* key_lo, uint64_t* key_hi) {
  DFH_ARG(o && o->inited, "dfh_lbfgs_owned_range: the model is not initialised");
  uint64_t lo = 0, hi = 0;
  if (o->comm) {
    const int r = o->comm->rank, W = o->comm->world;
    if (r > 0) lo = o->splits[r - 1];
    if (r + 1 < W) hi = o->splits[r];
  }
  if (key_lo) *key_lo = lo;
  if (key_hi) *key_hi = hi;
  return DFH_OK;
}

int dfh_lbfgs_set_model(dfh_lbfgs* o, uint64_t n, const uint64_t* keys, const int* lens, const float* vals, uint64_t* n_matched) {
  DFH_ARG(o && o->inited, "dfh_lbfgs_set_model: the model is not initialised");
  DFH_ARG(n == 0 || (keys && lens && vals), "dfh_lbfgs_set_model: NULL argument");
  if (o->grad_run || o->have_g) {
    set_error("dfh_lbfgs_set_model: a gradient pass has run: the model is set before the first dfh_lbfgs_calc_grad");
    return DFH_ERR_STATE;
  }
  DFH_HIP(hipSetDevice(o->ctx->device));
  hipStream_t s = o->ctx->stream;
  const int k = o->V_dim;
  // on a sharded object a rank that refuses its input still meets the others in the one all-reduce
  int rc = DFH_OK;
  std::string why;
  std::vector<uint64_t> ipos(n + 1, 0);
  for (uint64_t i = 0; i < n && !rc; ++i) {
    if (lens[i] != 1 && !(k > 0 && lens[i] == 1 + k)) {
      rc = DFH_ERR_ARG;
      why = "dfh_lbfgs_set_model: lens must be 1 or 1 + V_dim";
    }
    ipos[i + 1] = ipos[i] + (uint64_t)std::max(lens[i], 0);
    if (!rc && o->comm) {
      const int owner = (int)(std::upper_bound(o->splits.begin(), o->splits.end(), keys[i]) - o->splits.begin());
      if (owner != o->comm->rank) {
        rc = DFH_ERR_ARG;
        why = "dfh_lbfgs_set_model: an entry outside this rank's key range (dfh_lbfgs_owned_range)";
      }
    }
  }
  if (!rc && n >= (uint64_t(1) << 31)) {
    rc = DFH_ERR_ARG;
    why = "dfh_lbfgs_set_model: fewer than 2^31 input keys";
  }
  uint64_t matched = 0;
  const size_t K = o->keys.size();
  if (!rc && n && K) {
    join::Result j;
    const size_t pos_b = ((n + 1) * sizeof(uint64_t) + 255) / 256 * 256;
    rc = join::run(o->ctx, o->keys.data(), K, keys, n, pos_b + ipos[n] * sizeof(float), &j);
    if (!rc && j.dups) {
      rc = DFH_ERR_ARG;
      why = "dfh_lbfgs_set_model: the input keys are not unique";
    }
    if (!rc && j.matched) {
      uint64_t* d_ipos = reinterpret_cast<uint64_t*>(j.extra);
      float* d_vals = reinterpret_cast<float*>(j.extra + pos_b);
      const uint32_t st = (uint32_t)(1 + k);
      uint32_t shift = 0;
      while ((1u << shift) < st && shift < 6) ++shift;
      const lb::RowLanes rl{(uint32_t)n, st, shift};
      const uint64_t waves = (n + (64u >> shift) - 1) / (64u >> shift);
      const int gb = (int)std::max<uint64_t>(1, std::min<uint64_t>((waves + 3) / 4, 8192));
      if (hipMemcpyAsync(d_ipos, ipos.data(), (n + 1) * sizeof(uint64_t), hipMemcpyHostToDevice, s) != hipSuccess ||
          hipMemcpyAsync(d_vals, vals, ipos[n] * sizeof(float), hipMemcpyHostToDevice, s) != hipSuccess) {
        rc = DFH_ERR_HIP;
      } else {
        hipLaunchKernelGGL(lb::k_lb_set_model, dim3(gb), dim3(lb::THREADS), 0, s, j.pos, d_ipos, d_vals, o->d_pos, rl, o->d_w);
        if (hipGetLastError() != hipSuccess || hipStreamSynchronize(s) != hipSuccess) rc = DFH_ERR_HIP;
      }
      if (rc) why = "dfh_lbfgs_set_model: setting the model on the device failed";
      o->pulled = false;
    }
    if (j.mem) (void)hipFree(j.mem);
    if (!rc) matched = j.matched;
  }
  if (o->comm) {   // the one exchange of this call: the matched count, and whether every rank accepted its entries
    double t[2] = {(double)matched, rc ? 1.0 : 0.0};
    const int rc2 = dfh_comm_allreduce_sum(o->comm, t, 2);
    if (rc2 && !rc) return rc2;
    if (!rc && t[1] > 0) {
      rc = DFH_ERR_ARG;
      why = "dfh_lbfgs_set_model: another rank refused its entries";
    }
    matched = (uint64_t)t[0];
  }
  if (rc) {
    if (!why.empty()) set_error(why);
    return rc;
  }
  if (n_matched) *n_matched = matched;
  return DFH_OK;
}

int dfh_lbfgs_calc_grad(dfh_lbfgs* o, float gamma, float* loss, float* auc_n) {
  DFH_ARG(o && o->inited, "dfh_lbfgs_calc_grad: the model is not initialised");
  DFH_HIP(hipSetDevice(o->ctx->device));
  return lb_calc_grad(o, gamma, loss, auc_n);
}

int dfh_lbfgs_prepare_direction(dfh_lbfgs* o, float* incr_B, int* mcur) {
  DFH_ARG(o && o->inited && mcur, "dfh_lbfgs_prepare_direction: bad argument");
  DFH_HIP(hipSetDevice(o->ctx->device));
  if (o->l1 > 0.f) return ow_prepare_direction(o, incr_B, mcur);
  hipStream_t s = o->ctx->stream;
  const uint64_t n = o->n;
  if (!o->have_g) {  // epoch 0: g = g_new + grad r(w), no history yet (lbfgs_updater.h:89-90)
    hipLaunchKernelGGL(lb::k_lb_addreg, dim3(lb::blocks_for(n, 1)), dim3(lb::THREADS), 0, s, o->d_g, o->d_gnew, o->d_w, o->d_vmask,
                       o->l2, o->V_l2, n);
    DFH_HIP(hipGetLastError());
    o->have_g = true;
    *mcur = 0;
    return DFH_OK;
  }
  // y: drop the oldest when full, the new pair goes last
  if (o->y_count == o->m) {
    o->y_first = (o->y_first + 1) % o->m;
    --o->y_count;
  }
  ++o->y_count;
  const int k = o->y_count;
  DFH_ARG(o->s_count == k, "dfh_lbfgs_prepare_direction: s / y history out of step");
  lb::InnerArgs ia{};
  ia.n = n;
  ia.na = 3;
  ia.nb = 2 * k + 1;
  for (int i = 0; i < k; ++i) {
    ia.b[i] = lb_s(o, i);
    ia.b[k + i] = lb_y(o, i);
  }
  ia.b[2 * k] = o->d_g;
  ia.a[0] = lb_s(o, k - 1);
  ia.a[1] = lb_y(o, k - 1);
  ia.a[2] = o->d_g;
  ia.alias[0] = k - 1;
  ia.alias[1] = 2 * k - 1;
  ia.alias[2] = 2 * k;
  lb::Prep pr{o->d_gnew, o->d_w, o->d_vmask, o->l2, o->V_l2, o->alpha, k - 1, 2 * k - 1, 2 * k};
  const size_t rs = lb::inner_res_size(ia.nb);
  int rc = lb::launch_inner(s, ia, &pr, o->d_g, lb_y(o, k - 1), lb_s(o, k - 1), o->d_part, lb_tail(o));
  if (rc) return rc;
  o->alpha = 0;
  std::vector<double> h;
  rc = lb_fetch(o, lb_tail(o), rs, &h);
  if (rc) return rc;
  rc = lb_allsum(o, h.data(), rs);
  if (rc) return rc;
  // Twoloop::CalcIncreB's layout (lbfgs_twoloop.h:25-37)
  const int nb = ia.nb;
  for (int i = 0; i < k; ++i) {
    incr_B[i] = (float)lb::inner_at(h, nb, 0, i);
    incr_B[i + k] = (float)lb::inner_at(h, nb, 0, k + i);
    incr_B[i + 2 * k] = (float)lb::inner_at(h, nb, 1, i);
    incr_B[i + 3 * k] = (float)lb::inner_at(h, nb, 1, k + i);
    incr_B[i + 4 * k] = (float)lb::inner_at(h, nb, 2, i);
    incr_B[i + 5 * k] = (float)lb::inner_at(h, nb, 2, k + i);
  }
  incr_B[6 * k] = (float)lb::inner_at(h, nb, 2, 2 * k);
  *mcur = k;
  return DFH_OK;
}

int dfh_lbfgs_calc_direction(dfh_lbfgs* o, const float* d, float* p_g) {
  DFH_ARG(o && o->inited && o->have_g && p_g, "dfh_lbfgs_calc_direction: bad argument or no gradient prepared");
  DFH_ARG(o->y_count == 0 || d, "dfh_lbfgs_calc_direction: the coefficients are missing");
  DFH_HIP(hipSetDevice(o->ctx->device));
  if (o->l1 > 0.f) return ow_calc_direction(o, d, p_g);
  const int k = o->y_count;
  lb::CombArgs ca{};
  if (k) {
    for (int i = 0; i < k; ++i) {
      ca.v[i] = lb_s(o, i);
      ca.v[k + i] = lb_y(o, i);
    }
    ca.v[2 * k] = o->d_g;
    for (int i = 0; i < 2 * k + 1; ++i) ca.c[i] = d[i];
    ca.nv = 2 * k + 1;
  } else {  // dir = -g (lbfgs_updater.h:113-116)
    ca.v[0] = o->d_g;
    ca.c[0] = -1.f;
    ca.nv = 1;
  }
  // the new direction replaces the oldest s when the history is full (s_.erase(s_.begin()); s_.push_back(dir))
  float* target;
  if (o->s_count == o->m) {
    target = o->s[o->s_first];
    o->s_first = (o->s_first + 1) % o->m;
  } else {
    target = o->s[(o->s_first + o->s_count) % o->m];
    ++o->s_count;
  }
  ca.clampv = 5.f;
  ca.n = o->n;
  ca.out = target;
  ca.dot = o->d_g;
  int rc = lb::launch_combine(o->ctx->stream, ca, o->d_part, lb_tail(o));
  if (rc) return rc;
  std::vector<double> h;
  rc = lb_fetch(o, lb_tail(o), 1, &h);
  if (rc) return rc;
  rc = lb_allsum(o, h.data(), 1);
  if (rc) return rc;
  *p_g = (float)h[0];
  o->alpha = 0;
  return DFH_OK;
}

int dfh_lbfgs_line_search(dfh_lbfgs* o, float alpha, float gamma, float* objv, float* p_g, float* auc_n) {
  DFH_ARG(o && o->inited && o->s_count > 0 && objv && p_g, "dfh_lbfgs_line_search: bad argument or no direction");
  DFH_HIP(hipSetDevice(o->ctx->device));
  if (o->l1 > 0.f) return ow_line_search(o, alpha, gamma, objv, p_g, auc_n);
  const float* p = lb_s(o, o->s_count - 1);
  double r[3];
  int rc = lb_wstep(o, p, alpha - o->alpha, r);   // Add(alpha - alpha_, p, &w)
  if (rc) return rc;
  o->alpha = alpha;
  float loss = 0;
  rc = lb_calc_grad(o, gamma, &loss, auc_n);
  if (rc) return rc;
  // <g_new, p>: the worker's Inner(grads_, directions_)
  lb::InnerArgs ia{};
  ia.n = o->n;
  ia.na = 1;
  ia.nb = 1;
  ia.a[0] = o->d_gnew;
  ia.alias[0] = -1;
  ia.b[0] = p;
  double* res = lb_tail(o);
  rc = lb::launch_inner(o->ctx->stream, ia, nullptr, nullptr, nullptr, nullptr, o->d_part, res);
  if (rc) return rc;
  std::vector<double> h;
  rc = lb_fetch(o, res, 1, &h);
  if (rc) return rc;
  rc = lb_allsum(o, h.data(), 1);
  if (rc) return rc;
  // the worker's then the server's share of the job's status (lbfgs_learner.cc:147-150, 232-243; lbfgs_updater.h:125-133)
  *objv = loss + (float)r[0];
  *p_g = (float)h[0] + (float)r[1];
  return DFH_OK;
}

int dfh_lbfgs_evaluate(dfh_lbfgs* o, float* val_auc_n, float* nnz_w, float* r_w) {
  DFH_ARG(o && o->inited, "dfh_lbfgs_evaluate: the model is not initialised");
  DFH_HIP(hipSetDevice(o->ctx->device));
  double r[3];
  int rc = o->l1 > 0.f ? ow_reg(o, r) : lb_wstep(o, nullptr, 0.f, r);
  if (rc) return rc;
  if (nnz_w) *nnz_w = (float)r[2];
  if (r_w) *r_w = (float)r[0];
  if (val_auc_n) {
    auto& va = o->chunks[1];
    if (o->comm && !o->pulled) {   // the validation chunks read the local model: w has moved since the last pull
      rc = lb_pull(o);
      if (rc) return rc;
    }
    for (size_t i = 0; i < va.size(); ++i) {
      rc = lb_chunk_pass(o, va[i], false, o->d_res + 2 * i);
      if (rc) return rc;
    }
    std::vector<double> h;
    rc = lb_fetch(o, o->d_res, 2 * va.size(), &h);
    if (rc) return rc;
    float a = 0;
    for (size_t i = 0; i < va.size(); ++i) a += (float)h[2 * i + 1];
    if (o->comm) {
      double t = a;
      rc = lb_allsum(o, &t, 1);
      if (rc) return rc;
      a = (float)t;
    }
    *val_auc_n = a;
  }
  return DFH_OK;
}

int dfh_lbfgs_get_vector(dfh_lbfgs* o, int which, int i, float* out) {
  DFH_ARG(o && o->inited && (out || !o->n), "dfh_lbfgs_get_vector: the model is not initialised or out is NULL");
  DFH_ARG(which >= 0 && which <= 3, "dfh_lbfgs_get_vector: which must be 0 (g_new), 1 (g), 2 (s) or 3 (y)");
  const float* src = nullptr;
  if (which == 0) {
    src = o->d_gnew;
  } else if (which == 1) {
    DFH_ARG(o->have_g, "dfh_lbfgs_get_vector: g does not exist before the first dfh_lbfgs_prepare_direction");
    src = o->d_g;
  } else if (which == 2) {
    DFH_ARG(i >= 0 && i < o->s_count, "dfh_lbfgs_get_vector: the s index is outside the history");
    src = lb_s(o, i);
  } else {
    DFH_ARG(i >= 0 && i < o->y_count, "dfh_lbfgs_get_vector: the y index is outside the history");
    src = lb_y(o, i);
  }
  if (!o->n) return DFH_OK;
  DFH_HIP(hipSetDevice(o->ctx->device));
  DFH_HIP(hipMemcpyAsync(out, src, o->n * sizeof(float), hipMemcpyDeviceToHost, o->ctx->stream));
  DFH_HIP(hipStreamSynchronize(o->ctx->stream));
  return DFH_OK;
}

}  // extern "C"
