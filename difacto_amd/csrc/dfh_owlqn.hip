// dfh_owlqn.hip — l1 on w for the full-batch L-BFGS learner: orthant-wise L-BFGS (OWL-QN, Andrew & Gao, ICML 2007) on the
// vector kernels of dfh_lbfgs.hip (included in dfh_api.hip right after it).  The reference declares l1 for its LBFGSUpdater
// and comments it out (src/lbfgs/lbfgs_param.h:84-93); it has no code for it, so the rules are stated here.
//
// Objective F(w) = loss + r(w), r(w) = sum .5 coef w^2 + l1 sum_{w elements} |w|; a "w element" is one whose vmask bit is 0
// (every element when vmask is NULL).  V elements keep V_l2 alone and are never projected.  Everything here runs only on
// an object whose dfh_lbfgs_set_l1 got l1 > 0: the kernels and launches of dfh_lbfgs.hip are untouched.
//
// The fp32 operation order of every element-wise expression (fp contract(off): a product rounds before its sum; no
// x == 0 / x == 1 shortcut anywhere in this file, an exact factor changes no bit):
//   g'   = gnew + coef * w                             the smooth gradient (AddRegularizerGrad); stored as g
//   y    = g' + (-1) * g_old                           a difference of SMOOTH gradients
//   s    = w - w0                                      the real displacement of the accepted step, always stored
//   pg   = g'                     on a V element       the pseudo-gradient
//        = g' + l1                w > 0
//        = g' - l1                w < 0
//        = a = g' + l1 if a < 0; else b = g' - l1 if b > 0; else +0      w == 0 (-0.0 included)
//   p    = the Add chain of k_lb_combine over s_i, y_i, pg, in order, without its shortcuts: p = 0; p = p + c_k * v_k;
//          clamp to +-5; then on a w element p is kept iff p and pg have strictly opposite signs (p > 0 and pg < 0, or
//          p < 0 and pg > 0: the sign of p pg without the product's underflow), else +0
//   trial  w = w0 + alpha * p; on a w element xi = sign(w0) if w0 != 0 else sign(-pg); w is kept iff w and xi have the same
//          strict sign, else +0 (so a projected zero is +0.0)
//   sums (per-thread fp64, block_partials, k_lb_finish, as everywhere in dfh_lbfgs.hip; no float atomics):
//          <pg, p>           += (double)(pg * p)
//          Armijo term       += (double)(pg * (w - w0))          both operations in fp32
//          r2                += .5 * (double)coef * (double)w * (double)w
//          r1                += (double)fabsf(w)  on w elements; r(w) = r2 + (double)l1 * r1 on the host
//          nnz               += w != 0;   moved += w != w0
//          the 6m+1 products += (double)(a * b), a in {s_last, y_last, pg}, b in {s_i, y_i, pg}
//
// Passes per epoch: the pseudo-gradient and s = w - w0 ride in the Prep / inner pass (one more load, w0, and one more
// store, pg), the alignment in the combine pass (one more load: the mask words), the projection and both new sums in the
// step pass (w0 and pg read, w not read).  One extra launch per epoch: the copy of w into w0 after the direction.

#pragma clang fp contract(off)

namespace dfh {
namespace ow {

using lb::THREADS;
using lb::NA;
using lb::NB;

__device__ __forceinline__ bool is_v(const uint32_t* vmask, uint64_t i) { return vmask && ((vmask[i >> 5] >> (i & 31)) & 1u); }

__device__ __forceinline__ float pseudo(float gp, float w, float l1, bool isv) {
  if (isv) return gp;
  if (w > 0.f) return gp + l1;
  if (w < 0.f) return gp - l1;
  const float a = gp + l1;
  if (a < 0.f) return a;
  const float b = gp - l1;
  if (b > 0.f) return b;
  return 0.f;
}

// epoch 0 of PrepareCalcDirection: g = g', pg = its pseudo-gradient
__global__ void __launch_bounds__(THREADS) k_ow_addreg(float* __restrict__ g, float* __restrict__ pg, const float* __restrict__ gnew,
                                                       const float* __restrict__ w, const uint32_t* __restrict__ vmask, float l2,
                                                       float V_l2, float l1, uint64_t n) {
  for (uint64_t i = (uint64_t)blockIdx.x * THREADS + threadIdx.x; i < n; i += (uint64_t)gridDim.x * THREADS) {
    const bool isv = is_v(vmask, i);
    const float gp = gnew[i] + (isv ? V_l2 : l2) * w[i];
    g[i] = gp;
    pg[i] = pseudo(gp, w[i], l1, isv);
  }
}

struct Prep {
  const float* gnew;
  const float* w;
  const float* w0;
  const uint32_t* vmask;
  float l2, V_l2, l1;
  int is, iy, ig;          // indices of s_last, y_last, g in the right-hand list; slot ig holds g_old on entry, pg after
  float* g_out;
  float* y_out;
  float* s_out;
  float* pg_out;
};

// k_lb_inner<NBT, V, true> with the rules above: slot is takes w - w0, slot iy takes y, slot ig takes pg for the products
template <int NBT, int V>
__global__ void __launch_bounds__(THREADS) k_ow_inner(lb::InnerArgs a, Prep pr) {
  extern __shared__ double ow_sh[];
  double acc[NA * NBT];
#pragma unroll
  for (int q = 0; q < NA * NBT; ++q) acc[q] = 0.0;
  const uint64_t stride = (uint64_t)gridDim.x * THREADS * V;
  for (uint64_t i0 = ((uint64_t)blockIdx.x * THREADS + threadIdx.x) * V; i0 < a.n; i0 += stride) {
    float vb[NBT][V];
#pragma unroll
    for (int ib = 0; ib < NBT; ++ib) {
      if (ib < a.nb && ib != pr.iy && ib != pr.is) {
        lb::load_v<V>(a.b[ib], i0, a.n, vb[ib]);
      } else {
#pragma unroll
        for (int j = 0; j < V; ++j) vb[ib][j] = 0.f;
      }
    }
    float gn[V], w[V], w0[V], gold[V];
    lb::load_v<V>(pr.gnew, i0, a.n, gn);
    lb::load_v<V>(pr.w, i0, a.n, w);
    lb::load_v<V>(pr.w0, i0, a.n, w0);
#pragma unroll
    for (int ib = 0; ib < NBT; ++ib) {
#pragma unroll
      for (int j = 0; j < V; ++j)
        if (ib == pr.ig) gold[j] = vb[ib][j];
    }
    float gp[V], yn[V], sn[V], pg[V];
#pragma unroll
    for (int j = 0; j < V; ++j) {
      const bool isv = is_v(pr.vmask, i0 + j);
      gp[j] = gn[j] + (isv ? pr.V_l2 : pr.l2) * w[j];
      yn[j] = gp[j] + (-1.f) * gold[j];
      sn[j] = w[j] - w0[j];
      pg[j] = pseudo(gp[j], w[j], pr.l1, isv);
    }
#pragma unroll
    for (int ib = 0; ib < NBT; ++ib) {
#pragma unroll
      for (int j = 0; j < V; ++j) {
        if (ib == pr.ig) vb[ib][j] = pg[j];
        if (ib == pr.iy) vb[ib][j] = yn[j];
        if (ib == pr.is) vb[ib][j] = sn[j];
      }
    }
    lb::store_v<V>(pr.g_out, i0, a.n, gp);
    lb::store_v<V>(pr.y_out, i0, a.n, yn);
    lb::store_v<V>(pr.s_out, i0, a.n, sn);
    lb::store_v<V>(pr.pg_out, i0, a.n, pg);
#pragma unroll
    for (int ia = 0; ia < NA; ++ia) {
      float va[V];
#pragma unroll
      for (int ib = 0; ib < NBT; ++ib)
        if (ib == a.alias[ia]) {
#pragma unroll
          for (int j = 0; j < V; ++j) va[j] = vb[ib][j];
        }
#pragma unroll
      for (int ib = 0; ib < NBT; ++ib) {
        if (ib >= a.nb) continue;
        double s = acc[ia * NBT + ib];
#pragma unroll
        for (int j = 0; j < V; ++j) s += (double)(va[j] * vb[ib][j]);
        acc[ia * NBT + ib] = s;
      }
    }
  }
  lb::block_partials<NA * NBT>(acc, NA * NBT, ow_sh, a.part + (size_t)blockIdx.x * (NA * NBT));
}

struct CombArgs {
  lb::CombArgs c;          // c.dot: the pseudo-gradient
  const uint32_t* vmask;
};

template <int V>
__global__ void __launch_bounds__(THREADS) k_ow_combine(CombArgs a) {
  __shared__ double sh[THREADS / 64];
  double acc[1] = {0.0};
  const uint64_t n = a.c.n;
  const uint64_t stride = (uint64_t)gridDim.x * THREADS * V;
  for (uint64_t i0 = ((uint64_t)blockIdx.x * THREADS + threadIdx.x) * V; i0 < n; i0 += stride) {
    float p[V];
#pragma unroll
    for (int j = 0; j < V; ++j) p[j] = 0.f;
    for (int k = 0; k < a.c.nv; ++k) {
      const float x = a.c.c[k];
      float v[V];
      lb::load_v<V>(a.c.v[k], i0, n, v);
#pragma unroll
      for (int j = 0; j < V; ++j) p[j] = p[j] + x * v[j];
    }
    const float cl = a.c.clampv;
    float d[V];
    lb::load_v<V>(a.c.dot, i0, n, d);
#pragma unroll
    for (int j = 0; j < V; ++j) {
      p[j] = p[j] > cl ? cl : (p[j] < -cl ? -cl : p[j]);
      if (!is_v(a.vmask, i0 + j)) {
        const bool keep = (p[j] > 0.f && d[j] < 0.f) || (p[j] < 0.f && d[j] > 0.f);
        p[j] = keep ? p[j] : 0.f;
      }
      if (i0 + j < n) acc[0] += (double)(d[j] * p[j]);
    }
    lb::store_v<V>(a.c.out, i0, n, p);
  }
  lb::block_partials<1>(acc, 1, sh, a.c.part + blockIdx.x);
}

constexpr int NSUM = 5;    // r2, Armijo term, nnz, r1, moved

struct WstepArgs {
  float* w;
  const float* w0;
  const float* p;          // NULL: no step (w is read, nothing is written; the Armijo term and moved stay 0)
  const float* pg;
  float alpha;
  const uint32_t* vmask;
  float l2, V_l2;
  uint64_t n;
  double* part;            // [gridDim.x][NSUM]
};

template <int V>
__global__ void __launch_bounds__(THREADS) k_ow_wstep(WstepArgs a) {
  __shared__ double sh[(THREADS / 64) * NSUM];
  double acc[NSUM] = {0.0, 0.0, 0.0, 0.0, 0.0};
  const uint64_t stride = (uint64_t)gridDim.x * THREADS * V;
  for (uint64_t i0 = ((uint64_t)blockIdx.x * THREADS + threadIdx.x) * V; i0 < a.n; i0 += stride) {
    float w[V], w0[V], p[V], pg[V];
    if (a.p) {
      lb::load_v<V>(a.w0, i0, a.n, w0);
      lb::load_v<V>(a.p, i0, a.n, p);
      lb::load_v<V>(a.pg, i0, a.n, pg);
#pragma unroll
      for (int j = 0; j < V; ++j) {
        float t = w0[j] + a.alpha * p[j];
        if (!is_v(a.vmask, i0 + j)) {
          const bool pos = w0[j] > 0.f || (!(w0[j] < 0.f) && pg[j] < 0.f);    // xi > 0
          const bool neg = w0[j] < 0.f || (!(w0[j] > 0.f) && pg[j] > 0.f);    // xi < 0
          t = ((t > 0.f && pos) || (t < 0.f && neg)) ? t : 0.f;
        }
        w[j] = t;
      }
      lb::store_v<V>(a.w, i0, a.n, w);
    } else {
      lb::load_v<V>(a.w, i0, a.n, w);
    }
#pragma unroll
    for (int j = 0; j < V; ++j) {
      if (i0 + j >= a.n) continue;
      const bool isv = is_v(a.vmask, i0 + j);
      const float c = isv ? a.V_l2 : a.l2;
      acc[0] += .5 * (double)c * (double)w[j] * (double)w[j];
      if (a.p) {
        acc[1] += (double)(pg[j] * (w[j] - w0[j]));
        acc[4] += w[j] != w0[j] ? 1.0 : 0.0;
      }
      acc[2] += w[j] != 0.f ? 1.0 : 0.0;
      if (!isv) acc[3] += (double)fabsf(w[j]);
    }
  }
  lb::block_partials<NSUM>(acc, NSUM, sh, a.part + (size_t)blockIdx.x * NSUM);
}

// ------------------------------------------------------------------ host-side launchers
int launch_inner(hipStream_t s, lb::InnerArgs a, const Prep& pr, double* part, double* res) {
  const int np_bound = a.nb <= 3 ? 3 : a.nb <= 11 ? 11 : a.nb <= 21 ? 21 : NB;
  int nblk = 0;
  a.part = part;
#define OW_INNER(NBT, V)                                                                           \
  do {                                                                                             \
    nblk = lb::blocks_for(a.n, V);                                                                 \
    const size_t shm = (size_t)(THREADS / 64) * NA * NBT * sizeof(double);                         \
    hipLaunchKernelGGL((k_ow_inner<NBT, V>), dim3(nblk), dim3(THREADS), shm, s, a, pr);            \
  } while (0)
  switch (np_bound) {
    case 3: OW_INNER(3, 4); break;
    case 11: OW_INNER(11, 4); break;
    case 21: OW_INNER(21, 2); break;
    default: OW_INNER(NB, 1); break;
  }
#undef OW_INNER
  DFH_HIP(hipGetLastError());
  const int np = NA * np_bound;
  hipLaunchKernelGGL(lb::k_lb_finish, dim3(np), dim3(THREADS), 0, s, part, nblk, np, res);
  DFH_HIP(hipGetLastError());
  return DFH_OK;
}

int launch_combine(hipStream_t s, CombArgs a, double* part, double* res) {
  const int nblk = lb::blocks_for(a.c.n, 4);
  a.c.part = part;
  hipLaunchKernelGGL((k_ow_combine<4>), dim3(nblk), dim3(THREADS), 0, s, a);
  hipLaunchKernelGGL(lb::k_lb_finish, dim3(1), dim3(THREADS), 0, s, part, nblk, 1, res);
  DFH_HIP(hipGetLastError());
  return DFH_OK;
}

int launch_wstep(hipStream_t s, WstepArgs a, double* part, double* res) {
  const int nblk = lb::blocks_for(a.n, 4);
  a.part = part;
  hipLaunchKernelGGL((k_ow_wstep<4>), dim3(nblk), dim3(THREADS), 0, s, a);
  hipLaunchKernelGGL(lb::k_lb_finish, dim3(NSUM), dim3(THREADS), 0, s, part, nblk, NSUM, res);
  DFH_HIP(hipGetLastError());
  return DFH_OK;
}

}  // namespace ow
}  // namespace dfh

#pragma clang fp contract(fast)

namespace {

// the step pass and its five sums over the ranks; p == NULL: the sums of w as it stands
int ow_wstep(dfh_lbfgs* o, const float* p, float alpha, double out[ow::NSUM]) {
  ow::WstepArgs a{o->d_w, o->d_w0, p, o->d_pg, alpha, o->d_vmask, o->l2, o->V_l2, (uint64_t)o->n, nullptr};
  double* res = lb_tail(o);
  int rc = ow::launch_wstep(o->ctx->stream, a, o->d_part, res);
  if (rc) return rc;
  std::vector<double> r;
  rc = lb_fetch(o, res, ow::NSUM, &r);
  if (rc) return rc;
  if (p) o->pulled = false;
  rc = lb_allsum(o, r.data(), ow::NSUM);
  if (rc) return rc;
  for (int i = 0; i < ow::NSUM; ++i) out[i] = r[i];
  return DFH_OK;
}

// dfh_lbfgs_evaluate's {r(w), -, nnz(w)} with the l1 term
int ow_reg(dfh_lbfgs* o, double out[3]) {
  double r[ow::NSUM];
  const int rc = ow_wstep(o, nullptr, 0.f, r);
  if (rc) return rc;
  out[0] = r[0] + (double)o->l1 * r[3];
  out[1] = 0.0;
  out[2] = r[2];
  return DFH_OK;
}

int ow_prepare_direction(dfh_lbfgs* o, float* incr_B, int* mcur) {
  hipStream_t s = o->ctx->stream;
  const uint64_t n = o->n;
  if (!o->have_g) {
    hipLaunchKernelGGL(ow::k_ow_addreg, dim3(lb::blocks_for(n, 1)), dim3(lb::THREADS), 0, s, o->d_g, o->d_pg, o->d_gnew, o->d_w,
                       o->d_vmask, o->l2, o->V_l2, o->l1, n);
    DFH_HIP(hipGetLastError());
    o->have_g = true;
    *mcur = 0;
    return DFH_OK;
  }
  DFH_ARG(o->have_w0, "dfh_lbfgs_prepare_direction: no direction since the last call");
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
  ia.alias[0] = k - 1;
  ia.alias[1] = 2 * k - 1;
  ia.alias[2] = 2 * k;
  const ow::Prep pr{o->d_gnew, o->d_w, o->d_w0, o->d_vmask, o->l2, o->V_l2, o->l1, k - 1, 2 * k - 1, 2 * k,
                    o->d_g, lb_y(o, k - 1), lb_s(o, k - 1), o->d_pg};
  const size_t rs = lb::inner_res_size(ia.nb);
  int rc = ow::launch_inner(s, ia, pr, o->d_part, lb_tail(o));
  if (rc) return rc;
  o->alpha = 0;
  std::vector<double> h;
  rc = lb_fetch(o, lb_tail(o), rs, &h);
  if (rc) return rc;
  rc = lb_allsum(o, h.data(), rs);
  if (rc) return rc;
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

int ow_calc_direction(dfh_lbfgs* o, const float* d, float* p_g) {
  hipStream_t s = o->ctx->stream;
  const int k = o->y_count;
  ow::CombArgs ca{};
  if (k) {
    for (int i = 0; i < k; ++i) {
      ca.c.v[i] = lb_s(o, i);
      ca.c.v[k + i] = lb_y(o, i);
    }
    ca.c.v[2 * k] = o->d_pg;
    for (int i = 0; i < 2 * k + 1; ++i) ca.c.c[i] = d[i];
    ca.c.nv = 2 * k + 1;
  } else {
    ca.c.v[0] = o->d_pg;
    ca.c.c[0] = -1.f;
    ca.c.nv = 1;
  }
  float* target;
  if (o->s_count == o->m) {
    target = o->s[o->s_first];
    o->s_first = (o->s_first + 1) % o->m;
  } else {
    target = o->s[(o->s_first + o->s_count) % o->m];
    ++o->s_count;
  }
  ca.c.clampv = 5.f;
  ca.c.n = o->n;
  ca.c.out = target;
  ca.c.dot = o->d_pg;
  ca.vmask = o->d_vmask;
  int rc = ow::launch_combine(s, ca, o->d_part, lb_tail(o));
  if (rc) return rc;
  // the line search's origin: the one extra launch of an epoch
  if (o->n) DFH_HIP(hipMemcpyAsync(o->d_w0, o->d_w, o->n * sizeof(float), hipMemcpyDeviceToDevice, s));
  o->have_w0 = true;
  std::vector<double> h;
  rc = lb_fetch(o, lb_tail(o), 1, &h);
  if (rc) return rc;
  rc = lb_allsum(o, h.data(), 1);
  if (rc) return rc;
  *p_g = (float)h[0];
  o->alpha = 0;
  return DFH_OK;
}

int ow_line_search(dfh_lbfgs* o, float alpha, float gamma, float* objv, float* p_g, float* auc_n) {
  DFH_ARG(o->have_w0, "dfh_lbfgs_line_search: no direction");
  const float* p = lb_s(o, o->s_count - 1);
  double r[ow::NSUM];
  int rc = ow_wstep(o, p, alpha, r);
  if (rc) return rc;
  o->alpha = alpha;
  o->moved = r[4];
  float loss = 0;
  rc = lb_calc_grad(o, gamma, &loss, auc_n);
  if (rc) return rc;
  *objv = loss + (float)(r[0] + (double)o->l1 * r[3]);
  *p_g = (float)r[1];
  return DFH_OK;
}

}  // namespace

extern "C" {

int dfh_lbfgs_set_l1(dfh_lbfgs* o, float l1) {
  DFH_ARG(o && o->inited, "dfh_lbfgs_set_l1: the model is not initialised");
  DFH_ARG(l1 >= 0.f, "dfh_lbfgs_set_l1: l1 must be >= 0");   // refuses NaN too
  if (o->grad_run || o->have_g) {
    set_error("dfh_lbfgs_set_l1: a gradient pass has run: l1 is set before the first dfh_lbfgs_calc_grad");
    return DFH_ERR_STATE;
  }
  if (l1 == 0.f) return DFH_OK;
  DFH_HIP(hipSetDevice(o->ctx->device));
  if (!o->ow_arena) {
    const size_t vecf = std::max<size_t>(((o->n + 63) / 64) * 64, 64), vec = vecf * sizeof(float);
    const int rc = chunks::check_free(kLbWho, "the pseudo-gradient and the line search's origin (l1 > 0)", kLbTail, 2 * vec);
    if (rc) return rc;
    DFH_HIP(hipMalloc(&o->ow_arena, 2 * vec));
    Carver cv(o->ow_arena);
    o->d_pg = cv.take<float>(vecf);
    o->d_w0 = cv.take<float>(vecf);
  }
  o->l1 = l1;
  return DFH_OK;
}

int dfh_lbfgs_get_owlqn_vector(dfh_lbfgs* o, int which, float* out) {
  DFH_ARG(o && o->inited && (out || !o->n), "dfh_lbfgs_get_owlqn_vector: the model is not initialised or out is NULL");
  DFH_ARG(o->l1 > 0.f, "dfh_lbfgs_get_owlqn_vector: the object has no l1 (dfh_lbfgs_set_l1)");
  DFH_ARG(which == 0 || which == 1, "dfh_lbfgs_get_owlqn_vector: which must be 0 (pseudo-gradient) or 1 (w0)");
  if (which == 0) DFH_ARG(o->have_g, "dfh_lbfgs_get_owlqn_vector: no pseudo-gradient before the first dfh_lbfgs_prepare_direction");
  if (which == 1) DFH_ARG(o->have_w0, "dfh_lbfgs_get_owlqn_vector: no w0 before the first dfh_lbfgs_calc_direction");
  if (!o->n) return DFH_OK;
  DFH_HIP(hipSetDevice(o->ctx->device));
  DFH_HIP(hipMemcpyAsync(out, which == 0 ? o->d_pg : o->d_w0, o->n * sizeof(float), hipMemcpyDeviceToHost, o->ctx->stream));
  DFH_HIP(hipStreamSynchronize(o->ctx->stream));
  return DFH_OK;
}

int dfh_lbfgs_drop_last_pair(dfh_lbfgs* o) {
  DFH_ARG(o && o->inited, "dfh_lbfgs_drop_last_pair: the model is not initialised");
  DFH_ARG(o->s_count >= 1 && o->s_count == o->y_count,
          "dfh_lbfgs_drop_last_pair: no complete (s, y) pair: call it between dfh_lbfgs_prepare_direction and dfh_lbfgs_calc_direction");
  --o->s_count;
  --o->y_count;
  return DFH_OK;
}

int dfh_lbfgs_get_owlqn_moved(dfh_lbfgs* o, double* moved) {
  DFH_ARG(o && o->inited && moved, "dfh_lbfgs_get_owlqn_moved: bad argument");
  DFH_ARG(o->l1 > 0.f, "dfh_lbfgs_get_owlqn_moved: the object has no l1 (dfh_lbfgs_set_l1)");
  *moved = o->moved;
  return DFH_OK;
}

}  // extern "C"
