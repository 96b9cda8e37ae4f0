// dfh_eval.hip — whole-set evaluation on the device: exact AUC, logloss and accuracy of every (label, prediction) pair appended
// since the last reset (included at the end of dfh_api.hip; the learner's exact_metrics = 1).  The reference has no counterpart:
// BinClassMetric::AUC (src/loss/bin_class_metric.h:35-56) is computed per minibatch and averaged, which is not the AUC of the
// set.  An evaluator keeps the appended rows in two device arrays (8 B per row; they grow by doubling) and ranks them ONCE, in
// dfh_eval_finish:
//   k_eval_keys    a row -> an order-preserving 32-bit key of its score (-0.0 as +0.0; every NaN as the largest key, so the
//                  NaN rows are the tail of the sorted order) and a label byte (label > 0).  The same pass takes, over the rows
//                  whose score is not a NaN, the logloss terms max(-m, 0) + log1p(exp(-|m|)), m = y s, in fp64, the correct
//                  rows and the positives — per block partials, the fp64 sum of a block in a fixed tree
//   k_eval_reduce  one block adds the partials in index order and writes the header (n, n_pos, n_neg, n_nan, correct, objv)
//   rocprim::radix_sort_pairs (key, label byte), out of place: the appended rows stay as they are
//   k_eval_tile<0> a block per tile of EV_TILE sorted rows: the tile's negatives, and its last HEAD (the first row of a tie
//                  group: a row whose key differs from the row before it) with the negatives of the tile in front of it
//   k_eval_scan    one block scans the tiles: the negatives in front of every tile, and the last head in front of every tile
//                  with NP(head) = the negatives of the WHOLE order in front of it
//   k_eval_tile<1> a block per tile again: at every head e, the tie group that ENDS there — it starts at the head s before e,
//                  in this tile or (the scan's record) tiles back, so a group may span any number of tiles — contributes
//                      p_g (2 negatives_below + n_g) = ((e - NP(e)) - (s - NP(s))) (NP(s) + NP(e))
//                  in u64; a partial per tile
//   k_eval_final   one block adds the tiles' partials and the last group, which ends at the first NaN row (or at n)
// Everything between two launches is ordered by the stream alone: no block waits on another block, there are no floating-point
// atomics (no atomics at all), and a reduction's order is a function of n only — the same appended sequence gives the same
// bits in every field on every run, however it was cut into appends.  Vector stores and plain C++ only.  These kernels are not
// in the timing registry (dfh_kernel_name) and no launch of a step changes.
struct dfh_eval {
  dfh_ctx* ctx = nullptr;
  float* d_pred = nullptr;    // [cap] the appended rows
  float* d_label = nullptr;
  size_t cap = 0, n = 0, hint = 0;
  std::vector<void*> retired;   // arrays a growth replaced: copies out of them may still be queued, freed behind the next wait
  // finish's workspace, grown to what a finish needs, kept
  char* d_work = nullptr;
  size_t work_bytes = 0;
};

namespace {
constexpr uint32_t EV_ITEMS = 8, EV_TILE = 256 * EV_ITEMS;
static_assert(EV_ITEMS == 8, "k_eval_tile loads a thread's rows as 2 x uint4 keys and 1 x uint2 label bytes");
constexpr uint64_t EV_MAX_ROWS = 0xFFFFFFF0ULL;   // n < 2^32 - 16: auc2 <= 2 n_pos n_neg < 2^63, a head index + 1 fits 32 bits

struct EvalHdr {   // (dfh_eval_result's fields in front, in its order)
  uint64_t n, n_pos, n_neg, n_nan, auc2, correct;
  double objv;
  uint64_t m;   // n - n_nan: the sorted rows that take part in the ranking
};

// inclusive scan over the 256 threads of a block (Hillis-Steele in LDS: eight rounds); sh holds 256 T
template <typename T, typename Op>
__device__ __forceinline__ T ev_block_scan(T v, T* sh, Op op) {
  const uint32_t t = threadIdx.x;
  __syncthreads();   // sh may still be read by the previous use
  sh[t] = v;
  __syncthreads();
#pragma unroll
  for (uint32_t d = 1; d < 256; d <<= 1) {
    const T o = t >= d ? sh[t - d] : T(0);
    __syncthreads();
    if (t >= d) {
      v = op(v, o);
      sh[t] = v;
    }
    __syncthreads();
  }
  return v;
}
struct EvSum { template <typename T> __device__ T operator()(T a, T b) const { return a + b; } };
struct EvMax { template <typename T> __device__ T operator()(T a, T b) const { return a > b ? a : b; } };

// the sum of a block's 256 values in a fixed tree (thread 0 has it); sh holds 256 T
template <typename T>
__device__ __forceinline__ T ev_block_sum(T v, T* sh) {
  const uint32_t t = threadIdx.x;
  __syncthreads();
  sh[t] = v;
  __syncthreads();
#pragma unroll
  for (uint32_t d = 128; d > 0; d >>= 1) {
    if (t < d) sh[t] = sh[t] + sh[t + d];
    __syncthreads();
  }
  return sh[0];
}

__global__ void __launch_bounds__(256) k_eval_keys(const float* __restrict__ pred, const float* __restrict__ label, uint64_t n,
                                                   uint32_t* __restrict__ keys, uint8_t* __restrict__ flags,
                                                   double* __restrict__ part_objv, uint4* __restrict__ part_cnt) {
  __shared__ double sh_d[256];
  __shared__ uint32_t sh_u[256];
  const uint64_t base = (uint64_t)blockIdx.x * EV_TILE;
  double objv = 0;
  uint32_t npos = 0, nnan = 0, correct = 0;
#pragma unroll
  for (uint32_t j = 0; j < EV_ITEMS; ++j) {
    const uint64_t i = base + j * 256 + threadIdx.x;
    if (i >= n) break;
    const float s = pred[i];
    const bool pos = label[i] > 0.0f;   // the reference's rule: a NaN label is negative
    uint32_t key = 0xFFFFFFFFu;         // every NaN: behind +inf (0xFF800000)
    if (s != s) {
      ++nnan;
    } else {
      const uint32_t u = s == 0.0f ? 0u : __float_as_uint(s);   // -0.0 ties with +0.0
      key = (u & 0x80000000u) ? ~u : (u | 0x80000000u);
      const double m = pos ? (double)s : -(double)s;
      objv += fmax(-m, 0.0) + log1p(exp(-fabs(m)));
      npos += pos ? 1u : 0u;
      correct += ((pos && s > 0.0f) || (!pos && s <= 0.0f)) ? 1u : 0u;
    }
    keys[i] = key;
    flags[i] = pos ? 1 : 0;
  }
  const double o = ev_block_sum(objv, sh_d);
  const uint32_t a = ev_block_sum(npos, sh_u);
  const uint32_t b = ev_block_sum(nnan, sh_u);
  const uint32_t c = ev_block_sum(correct, sh_u);
  if (threadIdx.x == 0) {
    part_objv[blockIdx.x] = o;
    part_cnt[blockIdx.x] = make_uint4(a, b, c, 0u);
  }
}

__global__ void __launch_bounds__(256) k_eval_reduce(const double* __restrict__ part_objv, const uint4* __restrict__ part_cnt,
                                                     uint32_t nparts, uint64_t n, EvalHdr* __restrict__ hdr) {
  __shared__ double sh_d[256];
  __shared__ uint64_t sh_u[256];
  double objv = 0;
  uint64_t npos = 0, nnan = 0, correct = 0;
  for (uint32_t p = threadIdx.x; p < nparts; p += 256) {   // ascending p per thread, then the fixed tree
    objv += part_objv[p];
    const uint4 c = part_cnt[p];
    npos += c.x;
    nnan += c.y;
    correct += c.z;
  }
  const double o = ev_block_sum(objv, sh_d);
  const uint64_t a = ev_block_sum(npos, sh_u);
  const uint64_t b = ev_block_sum(nnan, sh_u);
  const uint64_t c = ev_block_sum(correct, sh_u);
  if (threadIdx.x == 0) {
    hdr->n = n;
    hdr->n_pos = a;
    hdr->n_neg = n - b - a;
    hdr->n_nan = b;
    hdr->auc2 = 0;
    hdr->correct = c;
    hdr->objv = o;
    hdr->m = n - b;
  }
}

// a head record: (index of the head + 1) << 32 | negatives in front of it; 0 = none.  A later head is a larger word.
__device__ __forceinline__ uint64_t ev_head(uint64_t i, uint32_t np) { return (i + 1) << 32 | np; }

// FINAL = 0: tile_neg[t], tile_head[t] (the negatives counted from the tile's first row).
// FINAL = 1: tile_pre[t] / tile_prev[t] (k_eval_scan) in, part[t] out.
template <int FINAL>
__global__ void __launch_bounds__(256) k_eval_tile(const uint32_t* __restrict__ keys, const uint8_t* __restrict__ flags,
                                                   const EvalHdr* __restrict__ hdr, uint32_t* __restrict__ tile_neg,
                                                   uint64_t* __restrict__ tile_head, const uint32_t* __restrict__ tile_pre,
                                                   const uint64_t* __restrict__ tile_prev, uint64_t* __restrict__ part) {
  __shared__ uint32_t sh_u[256];
  __shared__ uint64_t sh_w[256];
  const uint64_t m = hdr->m;
  const uint64_t first = (uint64_t)blockIdx.x * EV_TILE + (uint64_t)threadIdx.x * EV_ITEMS;   // this thread's rows: consecutive
  uint32_t k[EV_ITEMS], neg[EV_ITEMS];
  uint32_t before = first > 0 && first < m ? keys[first - 1] : 0u;
  uint32_t tneg = 0;
  if (first + EV_ITEMS <= m) {   // all eight rows: two 16 B loads and one 8 B load (first is a multiple of 8, the arrays are 256 B aligned)
    const uint4 a = *reinterpret_cast<const uint4*>(keys + first), b = *reinterpret_cast<const uint4*>(keys + first + 4);
    const uint2 f = *reinterpret_cast<const uint2*>(flags + first);
    k[0] = a.x; k[1] = a.y; k[2] = a.z; k[3] = a.w; k[4] = b.x; k[5] = b.y; k[6] = b.z; k[7] = b.w;
#pragma unroll
    for (uint32_t j = 0; j < EV_ITEMS; ++j) neg[j] = 1u - (((j < 4 ? f.x : f.y) >> (8 * (j & 3))) & 0xFFu);
  } else {
#pragma unroll
    for (uint32_t j = 0; j < EV_ITEMS; ++j) {
      const uint64_t i = first + j;
      k[j] = i < m ? keys[i] : 0u;
      neg[j] = i < m ? 1u - (uint32_t)flags[i] : 0u;
    }
  }
#pragma unroll
  for (uint32_t j = 0; j < EV_ITEMS; ++j) tneg += neg[j];
  const uint32_t incl = ev_block_scan(tneg, sh_u, EvSum());
  uint32_t np = incl - tneg;   // negatives of the tile in front of this thread's rows
  if (FINAL) np += tile_pre[blockIdx.x];
  // this thread's last head
  uint64_t last = 0;
  {
    uint32_t q = np, kb = before;
#pragma unroll
    for (uint32_t j = 0; j < EV_ITEMS; ++j) {
      const uint64_t i = first + j;
      if (i < m && (i == 0 || k[j] != kb)) last = ev_head(i, q);
      q += neg[j];
      kb = k[j];
    }
  }
  const uint64_t hincl = ev_block_scan(last, sh_w, EvMax());
  if (!FINAL) {
    if (threadIdx.x == 255) {
      tile_neg[blockIdx.x] = incl;
      tile_head[blockIdx.x] = hincl;
    }
    return;
  }
  // the last head in front of this thread's rows: in the tile (the exclusive scan) or before it
  __syncthreads();
  sh_w[threadIdx.x] = hincl;
  __syncthreads();
  uint64_t prev = threadIdx.x > 0 ? sh_w[threadIdx.x - 1] : 0;
  const uint64_t carry = tile_prev[blockIdx.x];
  if (carry > prev) prev = carry;
  uint64_t acc = 0;
  uint32_t q = np, kb = before;
#pragma unroll
  for (uint32_t j = 0; j < EV_ITEMS; ++j) {
    const uint64_t i = first + j;
    if (i < m && (i == 0 || k[j] != kb)) {
      if (prev) {   // the group [s, i)
        const uint64_t s = (prev >> 32) - 1, nps = prev & 0xFFFFFFFFu;
        acc += ((i - q) - (s - nps)) * (nps + q);
      }
      prev = ev_head(i, q);
    }
    q += neg[j];
    kb = k[j];
  }
  const uint64_t sum = ev_block_sum(acc, sh_w);
  if (threadIdx.x == 0) part[blockIdx.x] = sum;
}

// tile_pre[t] = negatives in front of tile t, tile_prev[t] = the last head in front of tile t with the negatives of the whole
// order in front of it; entry [ntiles]: the totals
__global__ void __launch_bounds__(256) k_eval_scan(const uint32_t* __restrict__ tile_neg, const uint64_t* __restrict__ tile_head,
                                                   uint32_t ntiles, uint32_t* __restrict__ tile_pre, uint64_t* __restrict__ tile_prev) {
  __shared__ uint32_t sh_u[256];
  __shared__ uint64_t sh_w[256];
  uint32_t run_neg = 0;
  uint64_t run_head = 0;
  for (uint32_t b = 0; b < ntiles; b += 256) {
    const uint32_t t = b + threadIdx.x;
    const uint32_t v = t < ntiles ? tile_neg[t] : 0u;
    const uint32_t incl = ev_block_scan(v, sh_u, EvSum());
    const uint32_t pre = run_neg + incl - v;
    uint64_t h = t < ntiles ? tile_head[t] : 0;
    if (h) h += pre;   // the low word: negatives of the tile in front of the head -> of the whole order (< 2^32: no carry)
    const uint64_t hincl = ev_block_scan(h, sh_w, EvMax());
    __syncthreads();
    sh_w[threadIdx.x] = hincl;
    __syncthreads();
    uint64_t hpre = threadIdx.x > 0 ? sh_w[threadIdx.x - 1] : 0;
    if (run_head > hpre) hpre = run_head;
    if (t < ntiles) {
      tile_pre[t] = pre;
      tile_prev[t] = hpre;
    }
    const uint64_t hl = sh_w[255];
    if (hl > run_head) run_head = hl;
    __syncthreads();
    sh_u[threadIdx.x] = incl;
    __syncthreads();
    run_neg += sh_u[255];
  }
  if (threadIdx.x == 0) {
    tile_pre[ntiles] = run_neg;
    tile_prev[ntiles] = run_head;
  }
}

__global__ void __launch_bounds__(256) k_eval_final(const uint64_t* __restrict__ part, uint32_t ntiles,
                                                    const uint64_t* __restrict__ tile_prev, EvalHdr* __restrict__ hdr) {
  __shared__ uint64_t sh_w[256];
  uint64_t acc = 0;
  for (uint32_t t = threadIdx.x; t < ntiles; t += 256) acc += part[t];
  const uint64_t sum = ev_block_sum(acc, sh_w);
  if (threadIdx.x == 0) {
    uint64_t auc2 = sum;
    const uint64_t prev = tile_prev[ntiles];
    if (prev) {   // the last group [s, m): P(m) = n_pos, NP(m) = n_neg
      const uint64_t s = (prev >> 32) - 1, nps = prev & 0xFFFFFFFFu;
      auc2 += (hdr->n_pos - (s - nps)) * (nps + hdr->n_neg);
    }
    hdr->auc2 = auc2;
  }
}

inline size_t ev_pad(size_t bytes) { return (bytes + 255) & ~(size_t)255; }

void ev_free_retired(dfh_eval* e) {
  for (void* p : e->retired) (void)hipFree(p);
  e->retired.clear();
}

// room for `extra` more rows; the rows held so far are copied on the stream, behind the appends that wrote them
int ev_reserve(dfh_eval* e, size_t extra) {
  const size_t need = e->n + extra;
  if (need <= e->cap) return DFH_OK;
  size_t cap = e->cap ? e->cap : (e->hint ? e->hint : (size_t)1 << 16);
  while (cap < need) cap *= 2;
  float *np = nullptr, *nl = nullptr;
  if (hipMalloc((void**)&np, cap * sizeof(float)) != hipSuccess || hipMalloc((void**)&nl, cap * sizeof(float)) != hipSuccess) {
    (void)hipGetLastError();
    if (np) (void)hipFree(np);
    set_error("dfh_eval: no device memory for " + std::to_string(cap) + " rows (" + std::to_string(2 * cap * sizeof(float)) +
              " bytes needed)");
    return DFH_ERR_CAPACITY;
  }
  if (e->n) {
    hipError_t er = hipMemcpyAsync(np, e->d_pred, e->n * sizeof(float), hipMemcpyDeviceToDevice, e->ctx->stream);
    if (er == hipSuccess) er = hipMemcpyAsync(nl, e->d_label, e->n * sizeof(float), hipMemcpyDeviceToDevice, e->ctx->stream);
    if (er != hipSuccess) {   // the evaluator keeps its arrays; the new ones go once nothing queued can touch them
      e->retired.push_back(np);
      e->retired.push_back(nl);
      set_error(std::string("dfh_eval: hipMemcpyAsync: ") + hipGetErrorString(er));
      return DFH_ERR_HIP;
    }
  }
  if (e->d_pred) e->retired.push_back(e->d_pred);
  if (e->d_label) e->retired.push_back(e->d_label);
  e->d_pred = np;
  e->d_label = nl;
  e->cap = cap;
  return DFH_OK;
}

int ev_append(dfh_eval* e, const float* label, const float* pred, size_t n, hipMemcpyKind kind) {
  if (n == 0) return DFH_OK;
  DFH_HIP(hipSetDevice(e->ctx->device));
  const int rc = ev_reserve(e, n);
  if (rc) return rc;
  DFH_HIP(hipMemcpyAsync(e->d_pred + e->n, pred, n * sizeof(float), kind, e->ctx->stream));
  DFH_HIP(hipMemcpyAsync(e->d_label + e->n, label, n * sizeof(float), kind, e->ctx->stream));
  e->n += n;
  return DFH_OK;
}
}  // namespace

extern "C" {

int dfh_eval_create(dfh_ctx* ctx, size_t capacity_hint, dfh_eval** out) {
  DFH_ARG(ctx && out, "dfh_eval_create: NULL argument");
  DFH_ARG(capacity_hint < EV_MAX_ROWS, "dfh_eval_create: capacity_hint must be below 2^32 - 16 rows");
  dfh_eval* e = new (std::nothrow) dfh_eval();
  if (!e) {
    set_error("dfh_eval_create: out of host memory (" + std::to_string(sizeof(dfh_eval)) + " bytes needed)");
    return DFH_ERR_CAPACITY;
  }
  e->ctx = ctx;
  e->hint = capacity_hint;
  *out = e;
  return DFH_OK;
}

int dfh_eval_destroy(dfh_eval* e) {
  if (!e) return DFH_OK;
  (void)hipSetDevice(e->ctx->device);
  (void)hipStreamSynchronize(e->ctx->stream);   // queued copies read and write the arrays
  ev_free_retired(e);
  if (e->d_pred) (void)hipFree(e->d_pred);
  if (e->d_label) (void)hipFree(e->d_label);
  if (e->d_work) (void)hipFree(e->d_work);
  delete e;
  return DFH_OK;
}

int dfh_eval_reset(dfh_eval* e) {
  DFH_ARG(e, "dfh_eval_reset: NULL argument");
  e->n = 0;   // the arrays stay; later appends are queued behind whatever still reads them
  return DFH_OK;
}

int dfh_eval_append_batch(dfh_eval* e, dfh_batch* b) {
  DFH_ARG(e && b, "dfh_eval_append_batch: NULL argument");
  DFH_ARG(b->ctx == e->ctx, "dfh_eval_append_batch: the batch belongs to another context");
  DFH_ARG(e->n + (uint64_t)b->nrows < EV_MAX_ROWS, "dfh_eval_append_batch: an evaluator holds fewer than 2^32 - 16 rows");
  // The two copies run on the context's stream, behind the batch's step.  d_pred is written on that stream only; d_label is
  // written by the batch object's NEXT load, on a preparation stream that waits for ev_free alone — and the step has
  // recorded ev_free already (main_end).  So, with pipelining on, ev_free is recorded again behind the copies: the next load
  // (prep_begin) waits for the latest record.  Call it before the next minibatch is loaded into the batch object.
  const int rc = ev_append(e, b->d_label, b->d_pred, b->nrows, hipMemcpyDeviceToDevice);
  if (rc) return rc;
  if (b->nrows && e->ctx->pipeline) {
    DFH_HIP(hipEventRecord(b->ev_free, e->ctx->stream));
    b->free_pending = true;
  }
  return DFH_OK;
}

int dfh_eval_append_host(dfh_eval* e, const float* label, const float* pred, size_t n) {
  DFH_ARG(e, "dfh_eval_append_host: NULL argument");
  DFH_ARG(n < EV_MAX_ROWS && e->n + (uint64_t)n < EV_MAX_ROWS, "dfh_eval_append_host: an evaluator holds fewer than 2^32 - 16 rows");
  DFH_ARG(n == 0 || (label && pred), "dfh_eval_append_host: NULL argument");
  const int rc = ev_append(e, label, pred, n, hipMemcpyHostToDevice);
  if (rc) return rc;
  DFH_HIP(hipStreamSynchronize(e->ctx->stream));   // the caller's arrays are free on return
  return DFH_OK;
}

int dfh_eval_finish(dfh_eval* e, dfh_eval_result* out) {
  DFH_ARG(e && out, "dfh_eval_finish: NULL argument");
  static_assert(sizeof(dfh_eval_result) == 7 * 8 && offsetof(dfh_eval_result, objv) == offsetof(EvalHdr, objv), "EvalHdr starts with the result");
  memset(out, 0, sizeof(*out));
  hipStream_t s = e->ctx->stream;
  DFH_HIP(hipSetDevice(e->ctx->device));
  const size_t n = e->n;
  if (n == 0) {
    DFH_HIP(hipStreamSynchronize(s));
    ev_free_retired(e);
    return DFH_OK;
  }
  const uint32_t ntiles = (uint32_t)((n + EV_TILE - 1) / EV_TILE);
  size_t tb = 0;
  DFH_HIP(rocprim::radix_sort_pairs(nullptr, tb, (uint32_t*)nullptr, (uint32_t*)nullptr, (uint8_t*)nullptr, (uint8_t*)nullptr, n, 0, 32, s));
  // the workspace: header | keys x 2 | flags x 2 | per tile: objv, counts, neg, head, pre, prev, part | the sort's
  const size_t o_hdr = 0;
  const size_t o_k0 = o_hdr + ev_pad(sizeof(EvalHdr)), o_k1 = o_k0 + ev_pad(n * 4);
  const size_t o_f0 = o_k1 + ev_pad(n * 4), o_f1 = o_f0 + ev_pad(n);
  const size_t o_pobjv = o_f1 + ev_pad(n), o_pcnt = o_pobjv + ev_pad((size_t)ntiles * 8);
  const size_t o_tneg = o_pcnt + ev_pad((size_t)ntiles * 16), o_thead = o_tneg + ev_pad((size_t)ntiles * 4);
  const size_t o_tpre = o_thead + ev_pad((size_t)ntiles * 8), o_tprev = o_tpre + ev_pad(((size_t)ntiles + 1) * 4);
  const size_t o_part = o_tprev + ev_pad(((size_t)ntiles + 1) * 8), o_temp = o_part + ev_pad((size_t)ntiles * 8);
  const size_t bytes = o_temp + ev_pad(tb + 16);
  if (bytes > e->work_bytes) {   // (only a finish uses the block, and the last one has waited for its work)
    if (e->d_work) (void)hipFree(e->d_work);
    e->d_work = nullptr;
    e->work_bytes = 0;
    if (hipMalloc((void**)&e->d_work, bytes) != hipSuccess) {
      (void)hipGetLastError();
      e->d_work = nullptr;
      set_error("dfh_eval_finish: no device memory to rank " + std::to_string(n) + " rows (" + std::to_string(bytes) + " bytes needed)");
      return DFH_ERR_CAPACITY;
    }
    e->work_bytes = bytes;
  }
  char* w = e->d_work;
  EvalHdr* hdr = (EvalHdr*)(w + o_hdr);
  uint32_t *k0 = (uint32_t*)(w + o_k0), *k1 = (uint32_t*)(w + o_k1);
  uint8_t *f0 = (uint8_t*)(w + o_f0), *f1 = (uint8_t*)(w + o_f1);
  double* pobjv = (double*)(w + o_pobjv);
  uint4* pcnt = (uint4*)(w + o_pcnt);
  uint32_t *tneg = (uint32_t*)(w + o_tneg), *tpre = (uint32_t*)(w + o_tpre);
  uint64_t *thead = (uint64_t*)(w + o_thead), *tprev = (uint64_t*)(w + o_tprev), *part = (uint64_t*)(w + o_part);
  hipLaunchKernelGGL(k_eval_keys, dim3(ntiles), dim3(256), 0, s, e->d_pred, e->d_label, (uint64_t)n, k0, f0, pobjv, pcnt);
  hipLaunchKernelGGL(k_eval_reduce, dim3(1), dim3(256), 0, s, pobjv, pcnt, ntiles, (uint64_t)n, hdr);
  DFH_HIP(rocprim::radix_sort_pairs(w + o_temp, tb, k0, k1, f0, f1, n, 0, 32, s));
  hipLaunchKernelGGL(k_eval_tile<0>, dim3(ntiles), dim3(256), 0, s, k1, f1, hdr, tneg, thead, (const uint32_t*)nullptr,
                     (const uint64_t*)nullptr, (uint64_t*)nullptr);
  hipLaunchKernelGGL(k_eval_scan, dim3(1), dim3(256), 0, s, tneg, thead, ntiles, tpre, tprev);
  hipLaunchKernelGGL(k_eval_tile<1>, dim3(ntiles), dim3(256), 0, s, k1, f1, hdr, (uint32_t*)nullptr, (uint64_t*)nullptr, tpre, tprev,
                     part);
  hipLaunchKernelGGL(k_eval_final, dim3(1), dim3(256), 0, s, part, ntiles, tprev, hdr);
  DFH_HIP(hipGetLastError());
  EvalHdr h;
  DFH_HIP(hipMemcpyAsync(&h, hdr, sizeof(h), hipMemcpyDeviceToHost, s));
  DFH_HIP(hipStreamSynchronize(s));
  ev_free_retired(e);
  out->n = h.n;
  out->n_pos = h.n_pos;
  out->n_neg = h.n_neg;
  out->n_nan = h.n_nan;
  out->auc2 = (h.n_pos && h.n_neg) ? h.auc2 : 0;
  out->correct = h.correct;
  out->objv = h.objv;
  return DFH_OK;
}

}  // extern "C"
